"""Throughput of the device-resident ray queries (rt_intersect_rays_device,
rt_occluded_rays_device, rt_shade_rays_device) on one GPU, with their
baselines measured in the same run:

  python tools/ray_stream_bench.py

closest hit  C3, 2^20 rays (half the C3 camera's primary rays, half the random
             rays of tests/test_gpu_parity.py::test_intersect_rays_exact):
             Mrays/s over --timed calls after --warmup calls, one
             rt_synchronize per timed group; the wall time per batch of
             rt_intersect_rays (host rays in, host hits out) on the same rays
             is the baseline.  The tool fails if the device call is not
             faster per batch: it does strictly less work.
occlusion    the same rays, without limits and with limits equal to the
             squared closest distance.
shading      the C3 camera's 1920x1080 1-spp primary rays at depth 8, Mrays/s
             from the returned ray counts; the same frame through
             rt_render_device at 1 spp (the packet megakernel) beside it.

Groups of the compared calls alternate (--groups), so a drift of the machine
shows as spread, not as a difference.  Answers are compared before anything
is timed.  One JSON line is printed at the end; the tool stops at the first
failure."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import _rt_pkg  # noqa: E402

f32 = np.float32


def primary_rays(fr):
    """The 1-spp camera rays of a frame in float32 (CastPixelRays,
    RayTracingSetup.cs:286-298), row-major."""
    cam, pl = fr.camera, fr.plane
    pos = np.asarray(cam.Position, f32)
    fwd, right, up = (np.asarray(v, f32) for v in (cam.Forward, cam.Right, cam.Up))
    rx, ry = pl.ResolutionX, pl.ResolutionY
    center = pos + fwd * f32(pl.DistanceToCamera)
    tl = (center - right * f32(pl.HalfHorizontalLength)) + up * f32(pl.HalfVerticalLength)
    hl = f32(pl.HalfHorizontalLength) * f32(2)
    vl = f32(pl.HalfVerticalLength) * f32(2)
    ys, xs = np.meshgrid(np.arange(ry), np.arange(rx), indexing="ij")
    rm = ((xs.reshape(-1).astype(f32) + f32(0.5)) * hl) / f32(rx)
    dm = ((ys.reshape(-1).astype(f32) + f32(0.5)) * vl) / f32(ry)
    p = (tl[None, :] + rm[:, None] * right[None, :]) - up[None, :] * dm[:, None]
    v = p - pos[None, :]
    # math.normalize = rsqrt(dot(x, x)) * x, the dot summed left to right
    d = (f32(1) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))[:, None] * v
    return np.ascontiguousarray(np.concatenate([np.tile(pos, (len(d), 1)), d], 1), f32)


def random_rays(n, seed=11):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.2, 1.2, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 10, 0] = 0.0
    return np.concatenate([o, d.astype(f32)], 1)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--shade-frames", type=int, default=10)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    rt = _rt_pkg.load()
    lib_hash = hashlib.sha256(open(rt.abi.LIB_PATH, "rb").read()).hexdigest()[:12]
    fr = rt.make("C3").with_(spp=1, max_bounces=8)
    ctx = rt.Context()
    ctx.set_scene(fr.scene)
    cam = primary_rays(fr)
    n = a.rays
    half = n // 2
    rays = np.ascontiguousarray(np.concatenate([cam[:: max(1, len(cam) // half)][:half], random_rays(n - half)]), f32)
    assert len(rays) == n, (len(rays), n)
    rays_t = torch.from_numpy(rays).cuda()
    hits_t = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    occ_t = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {"tool": "ray_stream_bench", "library": lib_hash, "command": "python " + " ".join(sys.argv), "scene": "C3",
           "rays": n, "warmup": a.warmup, "timed": a.timed, "groups": a.groups,
           "device": torch.cuda.get_device_name(0)}

    # ---- answers first: the device call returns what the host call returns
    ctx.intersect_rays_device(rays_t, n, hits_t)
    ctx.synchronize()
    dev_hits = hits_t.cpu().numpy()
    host_hits = ctx.intersect_rays(rays)
    if dev_hits.tobytes() != host_hits.tobytes():
        raise SystemExit("rt_intersect_rays_device and rt_intersect_rays disagree")
    hit = dev_hits[:, 0] != 0
    res["hit_fraction"] = float(hit.mean())

    def device_group(call):
        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.timed):
            call()
        ctx.synchronize()
        return (time.perf_counter() - t0) / a.timed * 1e3  # ms per batch

    def host_group():
        for _ in range(a.warmup):
            ctx.intersect_rays(rays)
        t0 = time.perf_counter()
        for _ in range(a.timed):
            ctx.intersect_rays(rays)
        return (time.perf_counter() - t0) / a.timed * 1e3

    # ---- closest hit: device against host, alternating groups
    dev_ms, host_ms = [], []
    for _ in range(a.groups):
        dev_ms.append(device_group(lambda: ctx.intersect_rays_device(rays_t, n, hits_t)))
        host_ms.append(host_group())
    res["closest_hit"] = {"device_ms_per_batch": spread(dev_ms), "host_ms_per_batch": spread(host_ms),
                          "device_mrays_per_s": n / (statistics.median(dev_ms) * 1e3),
                          "host_mrays_per_s": n / (statistics.median(host_ms) * 1e3)}
    print(json.dumps({"closest_hit": res["closest_hit"]}), flush=True)
    if not max(dev_ms) < min(host_ms):
        print(json.dumps(res))
        raise SystemExit(f"rt_intersect_rays_device ({max(dev_ms):.3f} ms per batch) is not faster than "
                         f"rt_intersect_rays ({min(host_ms):.3f} ms) on the same rays")

    # ---- occlusion: any hit, and limits at the squared closest distance
    dist = hits_t.view(torch.float32)[:, 3]
    lim_t = (dist * dist).contiguous()  # misses: FLT_MAX^2 = +inf
    torch.cuda.synchronize()
    ctx.occluded_rays_device(rays_t, None, n, occ_t)
    ctx.synchronize()
    if not np.array_equal(occ_t.cpu().numpy() != 0, hit):
        raise SystemExit("rt_occluded_rays_device (no limits) disagrees with the closest hits")
    ctx.occluded_rays_device(rays_t, lim_t, n, occ_t)
    ctx.synchronize()
    if occ_t.cpu().numpy().any():
        raise SystemExit("rt_occluded_rays_device: t * t < t * t held for some ray")
    any_ms = [device_group(lambda: ctx.occluded_rays_device(rays_t, None, n, occ_t)) for _ in range(a.groups)]
    lim_ms = [device_group(lambda: ctx.occluded_rays_device(rays_t, lim_t, n, occ_t)) for _ in range(a.groups)]
    res["occlusion"] = {"no_limits_ms_per_batch": spread(any_ms), "limits_ms_per_batch": spread(lim_ms),
                        "no_limits_mrays_per_s": n / (statistics.median(any_ms) * 1e3),
                        "limits_mrays_per_s": n / (statistics.median(lim_ms) * 1e3)}
    print(json.dumps({"occlusion": res["occlusion"]}), flush=True)

    # ---- shading: the frame's own primary rays, beside the frame itself
    W, H = fr.plane.ResolutionX, fr.plane.ResolutionY
    m = W * H
    cam_t = torch.from_numpy(cam).cuda()
    col_t = torch.empty((m, 4), dtype=torch.float32, device="cuda")
    img_t = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    prm = rt.frame_params(fr)
    st = ctx.shade_rays_device(cam_t, m, prm, col_t, m * 16, want_stats=True)
    sf = ctx.render_device(fr.camera, fr.plane, prm, img_t.data_ptr(), m * 16)
    torch.cuda.synchronize()
    diff = float((col_t.view(H, W, 4) - img_t).abs().max().item())
    counts = (st.primary_rays, st.shadow_rays, st.reflection_rays)
    if counts != (sf.primary_rays, sf.shadow_rays, sf.reflection_rays) or diff > 1e-4:
        raise SystemExit(f"shaded rays differ from the frame: max diff {diff}, rays {counts} vs "
                         f"{(sf.primary_rays, sf.shadow_rays, sf.reflection_rays)}")
    total = sum(counts)
    sh_k, sh_w, fr_k, fr_w = [], [], [], []
    for k in range(a.shade_frames + 2):  # alternating; the first two of each are warm-up
        t0 = time.perf_counter()
        st = ctx.shade_rays_device(cam_t, m, prm, col_t, m * 16, want_stats=True)
        t1 = time.perf_counter()
        sf = ctx.render_device(fr.camera, fr.plane, prm, img_t.data_ptr(), m * 16)
        t2 = time.perf_counter()
        if k >= 2:
            sh_k.append(st.kernel_ms)
            sh_w.append((t1 - t0) * 1e3)
            fr_k.append(sf.kernel_ms)
            fr_w.append((t2 - t1) * 1e3)
    res["shading"] = {"frame": f"C3 {W}x{H} 1 spp depth {fr.max_bounces}", "rays_per_frame": total,
                      "primary_shadow_reflection": counts, "max_abs_diff_to_frame": diff,
                      "shade_rays_kernel_ms": spread(sh_k), "shade_rays_wall_ms": spread(sh_w),
                      "render_device_kernel_ms": spread(fr_k), "render_device_wall_ms": spread(fr_w),
                      "shade_rays_mrays_per_s": total / (statistics.median(sh_k) * 1e3),
                      "render_device_mrays_per_s": total / (statistics.median(fr_k) * 1e3),
                      "render_device_speedup": statistics.median(sh_k) / statistics.median(fr_k)}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
