// Driver of csrc/dispatch_plan.h (host logic only, no GPU):
//   plan_asan table   the plan of every input of the table, one line each
//                     (tests/golden/dispatch_plan.tsv, tests/test_host_logic.py)
//   plan_asan sweep   every tile count from 1 to 140,000 at 4 spp under each flag
//                     combination: the plan's invariants hold, no plan reports an error
//   plan_asan         both, silently, under ASan + UBSan (tests/test_asan.py)
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dispatch_plan.h"

using rtp::Plan;
using rtp::PlanIn;

// the tile of a wave at spp samples per pixel (rt_frame.cpp prepare_frame)
static void tile_shape(PlanIn &in) {
    const int ppw = 64 / in.spp;
    int tw = ppw, th = 1;
    if ((ppw & (ppw - 1)) == 0) {
        int lg = 0;
        while ((1 << lg) < ppw) ++lg;
        th = 1 << (lg / 2);
        tw = ppw / th;
    }
    in.tile_w = tw;
    in.tile_h = th;
}

static const int kTiles[] = {1,     255,   256,   336,   2047,  2048,  23999, 24000, 24001,
                             39999, 40000, 40001, 69999, 70000, 70001, 129600, 518400};
static const int kFew[] = {336, 24000, 24001, 70000, 70001};  // on and beside the thresholds other dimensions read

// the slot's states: no order; an order at its first frame with a sky tail of
// 100 / 0 / every tile; an order due for its re-sort
struct Slot {
    bool valid;
    long long frames;
    int sky;  // -1: every tile
};
static const Slot kSlots[] = {{false, 0, 0}, {true, 1, 100}, {true, 1, 0}, {true, 1, -1}, {true, rtp::kLptPeriod, 100}};

template <class F>
static void with_slots(PlanIn in, int first, int last, F &&f) {
    for (int s = first; s <= last; ++s) {
        in.has_slot = true;
        in.order_valid = kSlots[s].valid;
        in.frames = kSlots[s].frames;
        in.sky_tail = kSlots[s].sky < 0 ? in.num_tiles : kSlots[s].sky;
        f(in);
    }
}

// The table's inputs: C2/C3-like frames (4 spp, depth 8, a 4-wide tree) of
// every tile count under every slot state, lone and overlapped, and around
// them each other dimension's values one dimension at a time.
template <class F>
static void table_inputs(F &&f) {
    for (int ov = 0; ov < 2; ++ov) {
        auto frame = [&](int n, int spp) {
            PlanIn in{};
            in.num_tiles = n;
            in.spp = spp;
            tile_shape(in);
            in.max_bounces = 8;
            in.bvh4 = in.mega = in.group_sample_waves = true;
            in.overlapped = ov != 0;
            return in;
        };
        for (int n : kTiles) {
            PlanIn in = frame(n, 4);
            with_slots(in, 0, 4, f);
            in.bvh4 = false;
            with_slots(in, 1, 1, f);
            in = frame(n, 4);
            in.group_sample_waves = false;  // a group band kept on one-pixel waves
            with_slots(in, 1, 1, f);
            in = frame(n, 4);
            in.batch = true;  // (4 spp only: rt_frame.cpp batch_launchable)
            with_slots(in, 1, 1, f);
        }
        for (int n : kFew) {
            for (int spp : {1, 9, 16, 25, 64})
                for (int bvh4 = 0; bvh4 < 2; ++bvh4) {
                    PlanIn in = frame(n, spp);
                    in.bvh4 = bvh4 != 0;
                    with_slots(in, 1, 1, f);
                }
            with_slots(frame(n, 16), 3, 4, f);  // the levels kernel's sky tail
            for (int spp : {4, 16}) {
                for (int mb : {0, 32, 33}) {  // fold depths, deep chains
                    PlanIn in = frame(n, spp);
                    in.max_bounces = mb;
                    with_slots(in, 1, 1, f);
                }
                for (int cr = 1; cr < 4; ++cr) {  // counting, row order, both
                    PlanIn in = frame(n, spp);
                    in.count_tests = (cr & 1) != 0;
                    in.row_order = (cr & 2) != 0;
                    with_slots(in, 1, 1, f);
                }
            }
            PlanIn in = frame(n, 4);
            in.count_tests = true;
            in.max_bounces = 33;
            with_slots(in, 1, 1, f);
            in = frame(n, 4);  // more (stream, slab) pairs than slots; the packet and wavefront paths
            f(in);
            in.mega = false;
            f(in);
        }
    }
}

static void print_plan(const PlanIn &in, const Plan &p) {
    std::printf("%d\t%d\t%d\t%d%d%d%d%d%d%d\t%d%d\t%lld\t%d\t|\t%d\t%d%d%d\t%d\t%d\t%d\t%d\t%d%d%d\t%d%d\t%d\t%s\t%s\n",
                in.num_tiles, in.spp, in.max_bounces, (int)in.bvh4, (int)in.mega, (int)in.overlapped,
                (int)in.group_sample_waves, (int)in.batch, (int)in.count_tests, (int)in.row_order, (int)in.has_slot,
                (int)in.order_valid, in.frames, in.sky_tail, (int)p.error, (int)p.lpt, (int)p.use_order,
                (int)p.measure, p.split_tiles, p.split16_tiles, p.s16_shift, p.sky_batch_tiles, (int)p.hints,
                (int)p.handoff, (int)p.tallies, (int)p.in_flight, (int)p.sky_tail_usable, p.waves,
                p.instance == rtp::kNone ? "-" : rtp::instance_name(p.instance),
                p.tail == rtp::kNone ? "-" : rtp::instance_name(p.tail));
}

// The invariants the kernels rely on, stated apart from plan_dispatch's own checks.
static const char *broken(const PlanIn &in, const Plan &p) {
    const bool split = p.split_tiles > 0 || p.split16_tiles > 0;
    if (p.error) return "plan_dispatch reports an error";
    if (p.s16_shift != 0 && p.s16_shift != 2) return "s16_shift";
    if ((p.s16_shift == 0) != p.handoff) return "hand-off buffers";
    if (p.s16_shift == 0 &&
        !(rtp::instance_hands_off(p.instance) && p.split16_tiles > 0 && !in.batch && !in.overlapped))
        return "one-sample waves without a SAMPLE instance";
    if (rtp::instance_hands_off(p.instance) && p.s16_shift != 0) return "a SAMPLE instance without one-sample waves";
    if (p.sky_batch_tiles > 0 &&
        !(p.use_order && p.tallies && p.split_tiles + p.split16_tiles + p.sky_batch_tiles <= in.num_tiles - 1))
        return "sky tail";
    if ((p.sky_batch_tiles > 0 && !in.batch) != (p.tail != rtp::kNone)) return "sky tail kernel";
    if ((in.count_tests || in.row_order) && (p.use_order || p.measure || split || p.sky_batch_tiles > 0))
        return "a counting or row-order frame carries an order";
    if ((p.instance == rtp::kLevels || in.max_bounces > rtd::kMaxBounces) && split) return "levels or deep frame splits";
    if (split && !p.use_order) return "splits without an order";
    if (split != p.hints) return "hints";
    if (p.waves < (in.num_tiles > 0 ? 1 : 0)) return "no wave left";
    return nullptr;
}

static long long sweep() {
    long long bad = 0, plans = 0;
    for (int flags = 0; flags < 64; ++flags)
        for (int n = 1; n <= 140000; ++n) {
            PlanIn in{};
            in.num_tiles = n;
            in.spp = 4;
            tile_shape(in);
            in.max_bounces = 8;
            in.mega = true;
            in.bvh4 = (flags & 1) != 0;
            in.overlapped = (flags & 2) != 0;
            in.group_sample_waves = (flags & 4) != 0;
            in.batch = (flags & 8) != 0;
            in.count_tests = (flags & 16) != 0;
            in.row_order = (flags & 32) != 0;
            with_slots(in, 0, 4, [&](const PlanIn &i) {
                const Plan p = rtp::plan_dispatch(i);
                ++plans;
                if (const char *why = broken(i, p)) {
                    if (++bad <= 20) {
                        std::printf("sweep: %s:\n", why);
                        print_plan(i, p);
                    }
                }
            });
        }
    std::printf("sweep: %lld plans, %lld broken\n", plans, bad);
    return bad;
}

int main(int argc, char **argv) {
    const bool table = argc > 1 && !std::strcmp(argv[1], "table"), only_sweep = argc > 1 && !std::strcmp(argv[1], "sweep");
    long long bad = 0, lines = 0;
    if (!only_sweep)
        table_inputs([&](const PlanIn &in) {
            const Plan p = rtp::plan_dispatch(in);
            ++lines;
            if (table) print_plan(in, p);
            if (broken(in, p)) ++bad;
        });
    if (!table) {
        if (!only_sweep) std::printf("table: %lld plans, %lld broken\n", lines, bad);
        bad += sweep();
        if (!bad) std::printf("ALL OK\n");
    }
    return bad ? 1 : 0;
}
