// kernels.h — host-side launchers of the gfx950 kernels in trace.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "dispatch_plan.h"
#include "rt_device.h"
#include "wavefront.h"

namespace rtk {

// Measuring builds (-DRT_WAVE_CLOCK): render_kernel records per-wave clocks
// into F.wave_clock (rt_debug_set RT_DEBUG_WAVE_CLOCKS); the product build
// compiles no such store.
#ifdef RT_WAVE_CLOCK
constexpr bool kWaveClockBuild = true;
#else
constexpr bool kWaveClockBuild = false;
#endif

using rtp::kSkyBatch;  // sky tiles per wave at the end of a longest-first order (dispatch_plan.h)
// Count of the tiles before the sorted order's sky tail (cost key 0) into
// host-mapped memory, one 64-bit store tagged with the sort's sequence number:
// (seq << 32) | count.
hipError_t launch_sky_count(const unsigned *cost_sorted, int n, unsigned seq, unsigned long long *out,
                            hipStream_t stream);

// One frame (or one row shard of it): CastPixelRays + Shade, RayTracingSetup.cs:275-366.
// Megakernel: one lane per sample, whole Whitted chain in one launch (trace.hip).
// Longest-first tile order for the next frame (trace.hip).
size_t tile_sort_scratch_bytes(int n);
// Sums the kCounterSlots sharded counter slots into kCounterWords words at out.
hipError_t launch_fold_counters(const unsigned long long *counters, unsigned long long *out, hipStream_t stream);
hipError_t launch_iota(int *p, int n, hipStream_t stream);
hipError_t sort_tiles_by_cost(const unsigned *cost, unsigned *cost_sorted, const int *iota, int *order, int n,
                              void *scratch, size_t scratch_bytes, hipStream_t stream);

// The top-level cut of a 4-wide tree (rtd::CutTable), after every tree build
// or refit, on the stream of that build.
hipError_t launch_build_cut(const rtd::BvhNode4 *nodes, rtd::CutTable *out, hipStream_t stream);
// the same cut with its boxes re-read from the (refitted) tree
hipError_t launch_refresh_cut(const rtd::BvhNode4 *nodes, rtd::CutTable *out, hipStream_t stream);

// Launches P.instance (dispatch_plan.h: the plan F's dispatch fields were
// filled from), then the order's sky tail and the launch's tallies as P says.
// *instance (nullable): the name of the kernel instance launched (static
// storage; null when nothing was launched) — rt_debug_read RT_DEBUG_LAST_LAUNCH.
hipError_t launch_render_mega(const rtd::SceneDev &S, const rtd::FrameDev &F, const rtp::Plan &P,
                              hipStream_t stream, const char **instance = nullptr);

// The frames of a batch (rtd::FrameBatch: whole 4-spp frames of one layout)
// in one launch: render_batch_kernel, then the batch's sky tail and tallies
// (sky_batch_batch_kernel) or its tallies alone.
hipError_t launch_render_batch(const rtd::SceneDev &S, const rtd::FrameBatch &B, const rtp::Plan &P,
                               hipStream_t stream, const char **instance = nullptr);

// Level-synchronous all-packet megakernel (trace_levels.hip), rtp::kLevels:
// >= 16 spp on a 4-wide BVH.  *instance (nullable): the instance's name.
hipError_t launch_render_levels(const rtd::SceneDev &S, const rtd::FrameDev &F, hipStream_t stream,
                                const char **instance = nullptr);

// Packet megakernel: wave-synchronous levels, coherent rays traced one BVH
// path per wave (packet.h).
hipError_t launch_render_packet(const rtd::SceneDev &S, const rtd::FrameDev &F, bool count_tests,
                                hipStream_t stream);

// Wavefront: per-level queues in HBM, persistent traversal with dynamic ray
// fetch (trace_wf.hip); chunk_tiles tiles (64 slots each) per pass sequence.
hipError_t launch_render_wavefront(const rtd::SceneDev &S, const rtd::FrameDev &F, const rtw::Args &A,
                                   int chunk_tiles, bool count_tests, hipStream_t stream);

// Batch closest hit, Scene.IntersectRay (Scene.cs:43-122): rays are 6 floats
// (origin, direction); out[i] = {rank or -1, distance bits, rank of the closest
// mesh-triangle hit or -1 (the reference's stale MeshIndex), -}.
hipError_t launch_intersect(const rtd::SceneDev &S, const float *rays, int n, int4 *out,
                            hipStream_t stream);

// Device-resident ray queries (ray_stream.hip): rays are rt_ray records (6
// floats) in HBM, one lane per ray; n <= 0 launches nothing.
// Closest hit with the ObjectId decoded on the device: out[i] = rt_hit {type,
// index, mesh_index, distance bits}; mesh_count entries (+ 1) in S.mesh_rank_first.
hipError_t launch_intersect_rays(const rtd::SceneDev &S, const float *rays, int n, int mesh_count, int4 *out,
                                 hipStream_t stream);
// The shadow test: out[i] = 1 iff ray i hits with Distance * Distance <
// limit_sq[i] (null limit_sq: iff it hits at all); stops at the first occluder.
hipError_t launch_occluded_rays(const rtd::SceneDev &S, const float *rays, const float *limit_sq, int n, int *out,
                                hipStream_t stream);
// Shade(ray, 0) per ray: out[i] = Color (float RGBA, alpha 1); max_bounces <=
// rtd::kMaxBounces; counters (kCounterSlots slots, null: none) receive the
// primary / shadow / reflection ray and shaded-hit counts.
hipError_t launch_shade_rays(const rtd::SceneDev &S, const float *rays, int n, int max_bounces, const float bg255[3],
                             float4 *out, unsigned long long *counters, hipStream_t stream);

// Row-order reassembly of block-cyclic shards gathered back to back.
hipError_t launch_assemble(const void *gathered, int res_x, int res_y, int band_count, int band_rows,
                           int local_rows, int pixel_bytes, void *image, hipStream_t stream);

}  // namespace rtk
