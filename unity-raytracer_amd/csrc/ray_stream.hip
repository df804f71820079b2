// ray_stream.hip — device-resident ray queries (rt_intersect_rays_device,
// rt_occluded_rays_device, rt_shade_rays_device): the caller's rays are read
// from HBM, one lane per ray, and the answers written to HBM, stream-ordered.
// Closest hit is Scene.IntersectRay (Data/Objects/Scene.cs:43-122) with the
// ObjectId decoded on the device, occlusion the reference's shadow test
// (RayTracingSetup.cs:333-345) as a query of its own, shading
// RayTracingSetup.Shade(ray, 0) (:304-366) for rays no camera built.
//
// All three walk per lane (traverse.h) over the LDS-plus-private hybrid stack
// exactly as trace.hip's intersect_kernel sets it up; the arithmetic is the
// render kernels' (shade.h), so a camera's rays shade to the frame's bits.
#include <float.h>

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "rt_device.h"
#include "rt_math.h"
#include "shade.h"
#include "traverse.h"

using namespace rtd;
using rtm::f3;
using rtm::mk;
using rtt::Counts;

namespace {

__device__ __forceinline__ void load_ray(const float *rays, int i, f3 &o, f3 &d) {
    const float *rr = rays + (size_t)i * 6;  // rt_ray: 24 B, 4-B aligned
    o = mk(rr[0], rr[1], rr[2]);
    d = mk(rr[3], rr[4], rr[5]);
}

// The mesh holding mesh-triangle rank rk: the last m in [0, mesh_count) with
// first[m] <= rk (empty meshes share their successor's first rank and never win).
__device__ __forceinline__ int mesh_of_rank(const int *first, int mesh_count, int rk) {
    int lo = 0, hi = mesh_count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= rk)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// intersect_kernel's two walks, then IntersectionResult / ObjectId on the
// device: {type, index, mesh_index, distance} as one 16-B store.
__global__ __launch_bounds__(kBlockThreads) void intersect_rays_kernel(SceneDev S, const float *rays, int n,
                                                                       int mesh_count, int4 *out) {
    __shared__ int stack_mem[kWavesPerBlock * kStackSize * kWaveSize];
    const int wave = threadIdx.x >> 6;
    int ovf[kStackTotal - kStackSize];
    const rtt::Stack st{stack_mem + wave * kStackSize * kWaveSize, ovf};  // + lane per query (traverse)
    const int i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    f3 o, d;
    load_ray(rays, i, o, d);
    rtt::RayCtx r;
    rtt::setup_ray(r, o, d);
    float bt;
    int br;
    Counts cnt = {0, 0, 0, 0, 0, 0, 0};
    rtt::traverse<false, false>(S, r, 0.0f, 0.0f, bt, br, st, cnt);
    // the stale MeshIndex of a sphere / loose-triangle winner (Scene.cs:76-79
    // vs :94-97, :109-112): the mesh of the closest mesh-triangle hit, if any
    int mesh_rank = br >= 0 && br < S.mesh_tri_total ? br : -1;
    if (br >= S.mesh_tri_total && S.mesh_tri_total > 0) {
        float mt;
        rtt::traverse<false, false, true>(S, r, 0.0f, 0.0f, mt, mesh_rank, st, cnt);
    }
    int type = 0, index = -1;
    if (br < 0) {
        bt = FLT_MAX;  // float.MaxValue
    } else if (br < S.mesh_tri_total) {
        type = 3;
    } else if (br < S.mesh_tri_total + S.sphere_count) {
        type = 1;
        index = br - S.mesh_tri_total;
    } else {
        type = 2;
        index = br - S.mesh_tri_total - S.sphere_count;
    }
    int mesh = -1;
    if (mesh_rank >= 0 && mesh_rank < S.mesh_tri_total && mesh_count > 0) {
        mesh = mesh_of_rank(S.mesh_rank_first, mesh_count, mesh_rank);
        if (type == 3) index = br - S.mesh_rank_first[mesh];
    }
    out[i] = make_int4(type, index, mesh, __float_as_int(bt));
}

// The shadow test as a query.  LIMITS: traverse<ANY> with the light distance
// bound the render kernels pass (tlimit = sqrt(d2) * 1.001, d2): occluded iff
// a hit with t * t < d2 exists, which is the closest hit's test since t >= 0
// makes t -> t * t monotone.  Without limits no d2 says "any hit" for every t
// (t * t may overflow to +inf, and +inf < +inf is false), so the closest-hit
// walk is stepped here and left at the first leaf that records a hit.
template <bool LIMITS>
__global__ __launch_bounds__(kBlockThreads) void occluded_rays_kernel(SceneDev S, const float *rays,
                                                                      const float *limit_sq, int n, int *out) {
    __shared__ int stack_mem[kWavesPerBlock * kStackSize * kWaveSize];
    const int wave = threadIdx.x >> 6;
    int ovf[kStackTotal - kStackSize];
    const rtt::Stack st{stack_mem + wave * kStackSize * kWaveSize, ovf};
    const int i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    f3 o, d;
    load_ray(rays, i, o, d);
    rtt::RayCtx r;
    rtt::setup_ray(r, o, d);
    Counts cnt = {0, 0, 0, 0, 0, 0, 0};
    bool occ = false;
    if (LIMITS) {
        const float d2 = limit_sq[i];
        float dt;
        int dr;
        occ = rtt::traverse<true, false>(S, r, sqrtf(d2) * 1.001f, d2, dt, dr, st, cnt);
    } else {
        rtt::Trav t;
        if (rtt::trav_begin<false, false>(S, r, 0.0f, t, cnt)) {
            const rtt::Stack lane_st{st.lds + rtt::lane_id(), st.ovf, st.n};
            while (!rtt::trav_step<false, false>(S, r, t, 0.0f, lane_st, cnt) && t.best_rank < 0) {
            }
            occ = t.best_rank >= 0;
        }
    }
    out[i] = occ ? 1 : 0;
}

struct ShadeRaysArgs {
    const float *rays;
    float4 *out;
    unsigned long long *counters;  // kCounterSlots x kCounterWords (rt_stats order); null: not counted
    int n;
    int max_bounces;  // <= kMaxBounces
    float bg255[3];   // new Rgb(BackgroundColor).Value
};

// render_packet_kernel<COUNT, 0> (trace.hip) with the lane's ray loaded in
// place of primary_ray and a plain float4 store in place of store_pixel: the
// wave-synchronous level loop, every ray traced per lane, every shadow ray
// traversed, the mirror recursion folded back to front.  Lanes past n stay in
// the kernel (alive = false): the loop's ballot and the counters' reduction
// are the whole wave's.
__global__ __launch_bounds__(kBlockThreads) void shade_rays_kernel(SceneDev S, ShadeRaysArgs A) {
    __shared__ int stack_mem[kWavesPerBlock * kStackSize * kWaveSize];
    const int wave = threadIdx.x >> 6;
    int ovf[kStackTotal - kStackSize];
    const rtt::Stack st{stack_mem + wave * kStackSize * kWaveSize, ovf};
    const int i = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool active = i < A.n;
    Counts cnt = {0, 0, 0, 0, 0, 0, 0};
    float fold_c[kMaxBounces][3];
    float fold_k[kMaxBounces][3];
    int depth = 0;
    f3 term = mk(0.0f, 0.0f, 0.0f);
    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    bool alive = active;
    if (active) {
        load_ray(A.rays, i, o, d);
        cnt.primary = 1;
    }
    for (int level = 0; __ballot(alive) != 0; ++level) {  // wave-uniform
        rtt::RayCtx r;
        rtt::setup_ray(r, o, d);
        float bt = FLT_MAX;
        int br = -1;
        if (alive) rtt::traverse<false, false>(S, r, 0.0f, 0.0f, bt, br, st, cnt);
        const bool hit = alive && br >= 0;
        if (alive && !hit) term = rtt::ld3(A.bg255);  // :310-311
        rts::Surface sf;
        DevMaterial m;
        f3 col = mk(0.0f, 0.0f, 0.0f);
        if (hit) {
            cnt.shading++;
            sf = rts::surface(S, o, d, bt, br);
            m = S.mats[sf.mat];
            col = rts::ambient(S, m);
        }
        for (int l = 0; l < S.num_lights; ++l) {  // :327-356, wave-uniform
            if (!hit) continue;
            const DevLight L = S.lights[l];
            const rts::ShadowRay sr = rts::shadow_ray(sf, L);
            cnt.shadow++;
            rtt::RayCtx rs;
            rtt::setup_ray(rs, sr.o, sr.dir);
            float dt;
            int dr;
            const bool occ = rtt::traverse<true, false>(S, rs, sqrtf(sr.d2) * 1.001f, sr.d2, dt, dr, st, cnt);
            if (!occ) col = col + rts::light_term(S, sf, m, L, sr);
        }
        const bool mirror = hit && m.ka_mirror.w != 0.0f && level < A.max_bounces;  // :358
        if (mirror) {
            fold_c[depth][0] = col.x; fold_c[depth][1] = col.y; fold_c[depth][2] = col.z;
            fold_k[depth][0] = m.km.x; fold_k[depth][1] = m.km.y; fold_k[depth][2] = m.km.z;
            rts::reflect(sf, o, d);
            ++depth;
            cnt.reflection++;
        } else if (hit) {
            term = col;
        }
        alive = mirror;
    }
    for (int k = depth - 1; k >= 0; --k)
        term = mk(fold_c[k][0], fold_c[k][1], fold_c[k][2]) + mk(fold_k[k][0], fold_k[k][1], fold_k[k][2]) * term;
    // Rgb.Color = Value / 255 (Rgb.cs:13), alpha 1
    if (active) A.out[i] = make_float4(term.x / 255.0f, term.y / 255.0f, term.z / 255.0f, 1.0f);
    if (A.counters) rtt::flush_counts<true>(cnt, A.counters);  // kernel-uniform
}

}  // namespace

namespace rtk {

static int ray_blocks(int n) { return (int)(((long long)n + kBlockThreads - 1) / kBlockThreads); }

hipError_t launch_intersect_rays(const SceneDev &S, const float *rays, int n, int mesh_count, int4 *out,
                                 hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(intersect_rays_kernel, dim3(ray_blocks(n)), dim3(kBlockThreads), 0, stream, S, rays, n,
                       mesh_count, out);
    return hipGetLastError();
}

hipError_t launch_occluded_rays(const SceneDev &S, const float *rays, const float *limit_sq, int n, int *out,
                                hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (limit_sq)
        hipLaunchKernelGGL(occluded_rays_kernel<true>, dim3(ray_blocks(n)), dim3(kBlockThreads), 0, stream, S, rays,
                           limit_sq, n, out);
    else
        hipLaunchKernelGGL(occluded_rays_kernel<false>, dim3(ray_blocks(n)), dim3(kBlockThreads), 0, stream, S, rays,
                           limit_sq, n, out);
    return hipGetLastError();
}

hipError_t launch_shade_rays(const SceneDev &S, const float *rays, int n, int max_bounces, const float bg255[3],
                             float4 *out, unsigned long long *counters, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    ShadeRaysArgs A;
    A.rays = rays;
    A.out = out;
    A.counters = counters;
    A.n = n;
    A.max_bounces = max_bounces;
    for (int k = 0; k < 3; ++k) A.bg255[k] = bg255[k];
    hipLaunchKernelGGL(shade_rays_kernel, dim3(ray_blocks(n)), dim3(kBlockThreads), 0, stream, S, A);
    return hipGetLastError();
}

}  // namespace rtk
