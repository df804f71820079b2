// dispatch_plan.h — how a frame is dispatched, decided in one place: which
// tiles split into quarter-, one-pixel and one-sample waves, whether the
// order's sky tail is batched, and which render_kernel / render_batch_kernel /
// levels instance runs.  Pure host logic over plain numbers (no HIP runtime
// call, no rt_ctx, no allocation): rt_frame.cpp lpt_prepare gathers a PlanIn,
// allocates what the Plan asks for, and trace.hip launches Plan::instance.
// Every threshold of these rules is defined here, once.
#pragma once

#include "rt_device.h"

namespace rtp {

// Sky tiles per wave at the end of a longest-first order (FrameDev
// sky_batch_tiles): a tile whose every sample surely misses the scene box is
// a background store, too little work for a wave of its own (60 % of a C3
// frame's waves, 12 % of its wave time: wclk_r05s).
#ifdef RT_EXP_SKYBATCH
constexpr int kSkyBatch = RT_EXP_SKYBATCH;  // measuring builds only (1: off)
#else
constexpr int kSkyBatch = 32;  // C3 in flight: 16 -> 32 +1.2 % / +0.2 % on two boxes, C4 +-0 (r06b, r05w)
#endif

// Frames (row shards) of at most this many tiles launch render_kernel's
// 5-wave instances (trace.hip), the only ones with the one-sample split path.
constexpr int kShardTilesMax = 70000;  // a 1/2 shard of 1080p at 4 spp
// ... but a shard of more tiles than this with other frames in flight beside
// it takes the 6-wave split instance: a 1/4 C3 share in flight -11.4 % per
// frame (0.0812 -> 0.0719 ms), a 1/8 share +8 %, lone shards +7 to +21 % (r06j);
// then (r06k) 1/2 -13.6 %, 1/4 -9.8 %, 1/8 +-0
#ifdef RT_EXP_SHARDW6
constexpr int kShardW6InFlight = RT_EXP_SHARDW6;  // measuring builds only
#else
constexpr int kShardW6InFlight = 24000;
#endif

// all-packet levels pay off where a wave's tile is small on screen (its
// mirror rays stay coherent): 16+ samples per pixel = at most 2x2 pixels
constexpr int kLevelsMinSpp = 16;

// Quarter-wave splitting of a frame's slowest tiles trades extra work (each
// quarter re-walks the BVH top) for a shorter critical path; it pays only
// when the frame (shard) is small enough for its slowest wave to set its
// time: measured with 3 frames in flight, a 1/8 C3 shard (16,200 tiles)
// +18 %, a 1/4 shard (32,400) -7 %, a whole frame (129,600) -7 %.  The very
// slowest of them (1/2048 of the tiles) go further, to sixteen waves of one
// pixel each: a 1/8 shard's single frame -14 % more, throughput with frames
// in flight +-1 % (1/512 or more: -5..-15 %).
#ifdef RT_EXP_SPLIT16DIV
constexpr int kSplit16Div = RT_EXP_SPLIT16DIV;  // measuring builds only
#else
constexpr int kSplit16Div = 2048;  // of those, 1/kSplit16Div of the tiles as sixteenth-waves; 0: off
#endif
#ifdef RT_EXP_SPLITDIV
constexpr int kSplitDiv = RT_EXP_SPLITDIV;  // measuring builds only
#else
constexpr int kSplitDiv = 256;  // 1/kSplitDiv of the tiles (the slowest) run as quarter-waves; 0: off
#endif
// A lone shard's finely split tiles run as one-sample waves traced by the
// whole wave (trace.hip render_sample_wave, csrc/coop.h): cheap enough to
// split its slowest 1/256 so (1/1024 before the whole-wave traversal: the
// rest of a 1/8 C3 share's slowest waves were whole tiles of ~105 us):
// single frame -13 % on two 1/8 shares against 1/1024 (r05q).
#ifdef RT_EXP_SPLIT16SAMPLE
constexpr int kSplit16DivSample = RT_EXP_SPLIT16SAMPLE;  // measuring builds only
#else
constexpr int kSplit16DivSample = 256;
#endif
// Larger shards (up to 70,000 tiles: a 1/2 or 1/4 shard of 1080p) split only
// their slowest 1/4096 into sixteenth-waves: single frame -15..-30 %,
// throughput with frames in flight +2..4 % on a 1/4 shard; a whole frame
// (129,600 tiles) loses 2-6 % and does not split.
#ifdef RT_EXP_SPLITMAX
constexpr int kSplitMaxTiles = RT_EXP_SPLITMAX;  // measuring builds only
#else
constexpr int kSplitMaxTiles = 24000;    // ... in frames/shards of at most this many tiles
#endif
#ifdef RT_EXP_SPLIT16MAX
constexpr int kSplit16MaxTiles = RT_EXP_SPLIT16MAX;  // measuring builds only
#else
constexpr int kSplit16MaxTiles = 70000;
#endif
constexpr int kSplit16DivLarge = 4096;
// A lone whole frame (more than kSplit16MaxTiles tiles, no other frame beside
// it) splits only its slowest 1/16384: C3 single frame -1.7 %, C2 -2.1 %
// against 1/4096 (1/8192: -1.1 / -1.1 %; r04aq, r04ar); 1/32768 +6 %, one
// tile +15 % on C3 (r04au).
#ifdef RT_EXP_SPLIT16WHOLE
constexpr int kSplit16DivWhole = RT_EXP_SPLIT16WHOLE;  // measuring builds only
#else
constexpr int kSplit16DivWhole = 16384;
#endif
#ifdef RT_EXP_S64LONE
constexpr int kSample16LoneTiles = RT_EXP_S64LONE;  // measuring builds only
#else
constexpr int kSample16LoneTiles = 40000;  // lone shards up to this many tiles: a sample per wave
#endif
// ... and a shard of that size with no other frame beside it (lpt_prepare
// overlapped_frame: a synchronous Update() frame of one rank) its slowest
// 1/1024: a 1/2 C3 shard's single frame -10.6 %, frames in flight +-0 (r04n;
// its slowest waves were whole tiles of ~190 us against a 148-us dispatch).
// One whose split tiles run as one-sample waves (<= kSample16LoneTiles: a 1/4
// shard) 1/512 since those trace with the whole wave (its slowest waves were
// then whole tiles of 120-130 us, wclk_r05p): -12.5 % and +1.4 % on two 1/4
// shares (r05q).
#ifdef RT_EXP_SPLIT16LONE
constexpr int kSplit16DivLone = RT_EXP_SPLIT16LONE;  // measuring builds only
constexpr int kSplit16DivLoneSample = RT_EXP_SPLIT16LONE;
#else
constexpr int kSplit16DivLone = 1024;
constexpr int kSplit16DivLoneSample = 512;
#endif
#ifdef RT_EXP_NOSYNCSPLIT
constexpr bool kSplitSync = false;  // measuring builds only
#else
constexpr bool kSplitSync = true;
#endif
// A frame with no other frame beside it (synchronous: Update() waits for it,
// RayTracingSetup.cs:171-199; or async frames on a single stream) has nothing to
// hide its tail behind, so whole frames of any size split their slowest 1/4096
// into sixteenth-waves too: C3 single frame -9 % (0.290 -> 0.264 ms,
// profiles/r04/abx_split) — a C3 frame's slowest wave, one tile's mirror chains,
// ran 0.32 ms against 0.24 ms for all the others (tools/wave_clock.py, r04i);
// frames in flight on several streams keep the 70,000-tile limit.
// Sky batches only for frames in flight of more than this many tiles: the
// batch waves run after the frame's render launch, and a small frame in
// flight is bound by its own latency (a 1/8 C3 share: +32 %; 1/4 −3.1 %, 1/2
// −1.5 %, whole frames −4.9 % per frame, r06d).
#ifdef RT_EXP_SKYMIN
constexpr int kSkyMinTiles = RT_EXP_SKYMIN;  // measuring builds only
#else
constexpr int kSkyMinTiles = 24000;
#endif
// Lone whole frames take sky batches too (measuring builds: -DRT_EXP_SKYLONE=1)
#ifdef RT_EXP_SKYLONE
constexpr bool kSkyLone = RT_EXP_SKYLONE != 0;
#else
constexpr bool kSkyLone = false;
#endif
#ifdef RT_EXP_LPTPERIOD
constexpr int kLptPeriod = RT_EXP_LPTPERIOD;  // measuring builds only
#else
// frames between longest-first re-sorts (one hipCUB sort ~46 us, plus the
// measuring launch's clock reads): 32 since round 5 (C3 in flight +1.9 %
// against 16, 64 +0.4 %: r06p)
constexpr int kLptPeriod = 32;
#endif

// Waves per SIMD of the megakernel's instances (trace.hip kMkMinWaves,
// kMkMinWavesShard: the launch bounds), as the tokens the instance names show.
#ifdef RT_EXP_MKWAVES
#define RT_PLAN_W6 RT_EXP_MKWAVES  // measuring builds only
#else
#define RT_PLAN_W6 6
#endif
#ifdef RT_EXP_MKWSHARD
#define RT_PLAN_W5 RT_EXP_MKWSHARD  // measuring builds only
#else
#define RT_PLAN_W5 5
#endif

// The kernel instances a plan may choose: X(id, kernel, template arguments).
// render_kernel<COUNT, SPLIT, DEEP, Q4, W, SAMPLE>, render_batch_kernel<SPLIT>,
// and sky_batch_kernel<Q4>, which takes a single frame's sky tail after them.
// trace.hip takes each instance's kernel from this list and instance_name()
// its name, so a name cannot drift from what is launched.  (The list's order
// is the order of these kernels in trace.hip's code object.)
#define RT_PLAN_INSTANCES(X)                                                      \
    X(kDeepCount, render_kernel, true, false, true, false, RT_PLAN_W5, false)     \
    X(kDeep, render_kernel, false, false, true, false, RT_PLAN_W5, false)         \
    X(kCount, render_kernel, true, false, false, false, RT_PLAN_W5, false)        \
    X(kSplitQ4ShardSample, render_kernel, false, true, false, true, RT_PLAN_W5, true)   \
    X(kSplitQ4Shard, render_kernel, false, true, false, true, RT_PLAN_W5, false)  \
    X(kSplitQ4, render_kernel, false, true, false, true, RT_PLAN_W6, false)       \
    X(kSplitShardSample, render_kernel, false, true, false, false, RT_PLAN_W5, true)    \
    X(kSplitShard, render_kernel, false, true, false, false, RT_PLAN_W5, false)   \
    X(kSplit, render_kernel, false, true, false, false, RT_PLAN_W6, false)        \
    X(kSkyTail, sky_batch_kernel, false)                                          \
    X(kQ4, render_kernel, false, false, false, true, RT_PLAN_W6, false)           \
    X(kPlain, render_kernel, false, false, false, false, RT_PLAN_W6, false)       \
    X(kSkyTailQ4, sky_batch_kernel, true)                                         \
    X(kBatchSplit, render_batch_kernel, true)                                     \
    X(kBatch, render_batch_kernel, false)

enum Instance {
#define RT_PLAN_X(id, kernel, ...) id,
    RT_PLAN_INSTANCES(RT_PLAN_X)
#undef RT_PLAN_X
    kInstances,  // (the launchable ones: trace.hip's table)
    kLevels = kInstances,  // launch_render_levels picks the levels instance (spp, fold depth) and names it
    kNone,                 // not a megakernel frame
};

#define RT_PLAN_STR2(...) #__VA_ARGS__
#define RT_PLAN_STR(...) RT_PLAN_STR2(__VA_ARGS__)
inline const char *instance_name(Instance i) {
    static const char *const names[] = {
#define RT_PLAN_X(id, kernel, ...) #kernel "<" RT_PLAN_STR(__VA_ARGS__) ">",
        RT_PLAN_INSTANCES(RT_PLAN_X)
#undef RT_PLAN_X
        "render_levels_kernel", ""};
    return names[i];
}

// whether an instance's waves hand their sample off (render_kernel's SAMPLE)
inline bool instance_hands_off(Instance i) { return i == kSplitQ4ShardSample || i == kSplitShardSample; }

struct PlanIn {
    int num_tiles, spp, tile_w, tile_h, max_bounces;
    bool bvh4;
    bool count_tests, row_order;  // RT_FLAG_COUNT_TESTS, RT_FLAG_ROW_ORDER
    bool mega;                    // the megakernel path (not packets, not the wavefront)
    bool overlapped;              // rt_frame.cpp overlapped_frame, evaluated once by the caller
    bool group_sample_waves;      // rt_frame.cpp group_sample_waves
    bool batch;                   // a batch launch (rt_render_device_batch)
    // the (stream, slab) slot's state
    bool has_slot;       // (more pairs than slots: no slot, row-major order)
    bool order_valid;    // a sorted order of this layout exists
    long long frames;    // frames dispatched by it since that sort
    int sky_tail;        // the order's last sky_tail tiles were sky when measured
};

enum PlanError { kPlanOk = 0, kPlanErrSample, kPlanErrSky, kPlanErrUnordered, kPlanErrLevels };

struct Plan {
    PlanError error;       // a violated invariant (below): the caller fails the frame
    bool lpt;              // the frame dispatches longest-first through its slot
    bool use_order;        // ... by the slot's last order
    bool measure;          // this frame records tile costs and the caller sorts them after it
    int split_tiles, split16_tiles, s16_shift, sky_batch_tiles;  // FrameDev's fields of these names
    bool hints, handoff, tallies;  // buffers of the launch: occluder hints, one-sample hand-off, per-wave tallies
    bool in_flight;        // FrameDev in_flight
    bool sky_tail_usable;  // a frame like this one takes sky batches: its slot's first sort waits for the count
    Instance instance;
    Instance tail;         // a single frame's sky tail: kSkyTail, kSkyTailQ4, or kNone (a batch's: sky_batch_batch_kernel)
    int waves;            // waves of the render launch (tiles + the extra waves of split tiles - the sky tail)
};

inline bool plan_deep(const PlanIn &in) { return in.max_bounces > rtd::kMaxBounces; }
// the levels kernel's frames (deep ones take render_kernel's deep-chain instance)
inline bool plan_levels(const PlanIn &in) { return in.bvh4 && in.spp >= kLevelsMinSpp && !plan_deep(in); }
// The frames a (stream, slab) slot serves, which the caller finds or claims
// one for: megakernel frames not in row order
// (a counting launch measures tests, not costs: its per-lane walk is not the
// frame a longest-first order is for, and it never answers a tile as sky)
inline bool plan_wants_slot(const PlanIn &in) {
    return in.mega && !in.count_tests && !in.row_order && in.num_tiles > 0;
}
inline bool plan_lpt(const PlanIn &in) { return plan_wants_slot(in) && in.has_slot; }

// Whether a frame like `in` takes sky batches, i.e. whether the sky tail of
// its order is worth a host wait: megakernel frames in flight of more than
// kSkyMinTiles tiles, 16-spp levels frames in flight.  Lone frames, small
// shares and rt_render's row slabs never use the tail.
inline bool sky_tail_usable(const PlanIn &in) {
    if (kSkyBatch <= 1 || !plan_lpt(in) || plan_deep(in)) return false;
    // The levels kernel's 16-spp instance (the one with the sky test) measures
    // which tiles are sky, and whole frames in flight leave those to
    // sky_batch_kernel: its positions are then the measured non-sky tiles,
    // longest first (trace_levels.hip kLvRowKeys: or in row order) (C4 all-sky
    // frames cost 0.955 ms in flight as a wave per tile; skycost, r05z).
    if (plan_levels(in)) return in.spp == 16 && in.overlapped;
    // The sorted order ends with the tiles the last measurement found to be
    // sky (cost key 0, row order): with other frames in flight beside this
    // one, sky_batch_kernel takes them kSkyBatch a wave after render_kernel,
    // together with the launch's tallies (C3 frames in flight -4.9 % per frame,
    // r06d; a lone frame, whose critical path the batches lengthen, +0.5 % C3,
    // +5 % a 1/8 shard: abx_r05t).
    return in.num_tiles > kSkyMinTiles && (in.overlapped || (kSkyLone && in.num_tiles > kShardTilesMax));
}

inline Plan plan_dispatch(const PlanIn &in) {
    Plan p{};
    p.s16_shift = 2;  // finely split tiles: a pixel per wave
    p.instance = p.tail = kNone;
    const int n = in.num_tiles;
    const bool deep = plan_deep(in), levels = plan_levels(in);
    p.lpt = plan_lpt(in);
    p.in_flight = in.overlapped && plan_wants_slot(in);
    if (p.lpt) {
        const bool ov = in.overlapped;
        p.use_order = in.order_valid;
        // costs are measured and re-sorted every kLptPeriod frames (the sort
        // costs more than a small frame's tail)
        p.measure = !in.order_valid || in.frames % kLptPeriod == 0;
        p.tallies = true;
        // In small shards the finely split tiles go one step further, to a
        // sample per wave (s16_shift 0; the shard instance sums each pixel's
        // four samples when the last arrives): a pixel's four samples no longer
        // wait for each other's divergent mirror chains.  Lone frames only
        // (nothing beside them hides their slowest chain): a 1/8 C3 shard's
        // single frame -20 %, a 1/4 shard's -15 %; a lone 1/2 shard +5 %, whole
        // frames +6 %; with four frames in flight a 1/8 shard's throughput is
        // -3 % to +-0 (r04r, r04ag, r04ai, 200-frame runs alternated on one
        // box).  The bands of a multi-device frame too, unless
        // rt_debug_set(RT_DEBUG_GROUP_SAMPLE_WAVES, 0).  Never a batch launch:
        // its 6-wave instances split tiles into quarter- and one-pixel waves.
        const bool sample_waves = in.spp == 4 && n <= kShardTilesMax && n <= kSample16LoneTiles && !ov &&
                                  in.group_sample_waves && !in.batch;
        // the most expensive tiles of the last measurement are split into
        // quarter-waves (a frame's time is bounded below by its slowest wave);
        // render_kernel only: 16 lanes must hold whole pixels
        if (p.use_order && !levels && !deep) {
            if (kSplitDiv > 0 && 16 % in.spp == 0 && n <= kSplitMaxTiles) {
                p.split_tiles = n / kSplitDiv > 1 ? n / kSplitDiv : 1;
                // sixteenth-waves (4 lanes) must hold whole pixels too
                if (kSplit16Div > 0 && 4 % in.spp == 0) {
                    // a lone shard's (one-sample waves) more (kSplit16DivSample)
                    const int div = sample_waves ? kSplit16DivSample : kSplit16Div;
                    const int want = n / div > 1 ? n / div : 1;
                    p.split16_tiles = p.split_tiles < want ? p.split_tiles : want;
                    p.split_tiles -= p.split16_tiles;
                }
            } else if (kSplit16DivLarge > 0 && 4 % in.spp == 0 && (n <= kSplit16MaxTiles || (kSplitSync && !ov))) {
                const bool lone_shard = n <= kSplit16MaxTiles && !ov;
                const int div = lone_shard && sample_waves ? kSplit16DivLoneSample
                                : lone_shard               ? kSplit16DivLone
                                : n > kSplit16MaxTiles     ? kSplit16DivWhole
                                                           : kSplit16DivLarge;
                p.split16_tiles = n / div > 1 ? n / div : 1;
            }
        }
        const bool split = p.split_tiles > 0 || p.split16_tiles > 0;
        p.hints = split;  // (a batch's head too; its frame blocks take none)
        if (p.split16_tiles > 0 && sample_waves) p.s16_shift = 0;
        p.handoff = p.s16_shift == 0;
        p.sky_tail_usable = sky_tail_usable(in);
        // Only the grids depend on the sky count (a stale one costs time, not
        // pixels: a batch renders any tile that is not sky in full).
        // (render_kernel keeps one wave at least: its launch and tallies stay, an all-sky view included)
        if (p.use_order && p.sky_tail_usable) {
            const int room = n - p.split_tiles - p.split16_tiles - 1;
            const int sky = in.sky_tail < room ? in.sky_tail : room;
            p.sky_batch_tiles = sky > 0 ? sky : 0;
        }
        if (levels) {
            // the levels kernel dispatches XCD-aware stripes (trace_levels.hip)
            // in row order, without splits; by the order only with a sky tail
            if (in.spp == 16 && kSkyBatch > 1) {
                if (p.sky_batch_tiles == 0) p.use_order = false;  // plain stripes
            } else {
                p.use_order = false;
                p.measure = false;
            }
        }
    }
    const bool split = p.split_tiles > 0 || p.split16_tiles > 0;
    if (in.mega && n > 0) {
        const bool q4 = in.spp == 4 && in.tile_w == 4 && in.tile_h == 4;
        // a small frame: its slowest waves set its time (unless frames in flight hide them)
        const bool shard = n <= kShardTilesMax && !(p.in_flight && n > kShardW6InFlight);
        if (in.batch)
            p.instance = split ? kBatchSplit : kBatch;
        else if (deep)  // mirror chains may outgrow the fold stack
            p.instance = in.count_tests ? kDeepCount : kDeep;
        else if (in.count_tests)
            p.instance = kCount;
        else if (split && shard && p.handoff)
            p.instance = q4 ? kSplitQ4ShardSample : kSplitShardSample;
        else if (split && shard)
            p.instance = q4 ? kSplitQ4Shard : kSplitShard;
        else if (split)
            p.instance = q4 ? kSplitQ4 : kSplit;
        else if (levels)
            p.instance = kLevels;
        else
            p.instance = q4 ? kQ4 : kPlain;
        if (p.sky_batch_tiles > 0 && !in.batch) p.tail = q4 ? kSkyTailQ4 : kSkyTail;
    }
    p.waves = n <= 0 ? 0 : n - p.sky_batch_tiles + ((64 >> p.s16_shift) - 1) * p.split16_tiles + 3 * p.split_tiles;
    // What the kernels rely on, and no single rule above states:
    // one-sample waves hand their sample off, which only the SAMPLE instances do
    // (a split tile's pixels would never be stored by another), lone frames only
    if (p.s16_shift == 0 && !(instance_hands_off(p.instance) && p.split16_tiles > 0 && !in.batch && !in.overlapped))
        p.error = kPlanErrSample;
    // the sky tail is the end of an order, its tiles counted by the tallies'
    // launch; the render launch keeps a wave and the splits their tiles
    else if (p.sky_batch_tiles > 0 &&
             !(p.use_order && p.tallies && p.split_tiles + p.split16_tiles + p.sky_batch_tiles <= n - 1))
        p.error = kPlanErrSky;
    // counting and row-order frames run row-major, whole tiles
    else if ((in.count_tests || in.row_order) && (p.use_order || p.measure || split || p.sky_batch_tiles > 0))
        p.error = kPlanErrUnordered;
    // the levels and deep-chain instances have no split path
    else if ((p.instance == kLevels || deep) && split)
        p.error = kPlanErrLevels;
    return p;
}

}  // namespace rtp
