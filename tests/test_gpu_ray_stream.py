"""Device-resident ray queries (rt_intersect_rays_device, rt_occluded_rays_device,
rt_shade_rays_device): rays, limits and answers are torch tensors in HBM, the
calls are enqueued on the context's stream and checked against the oracles the
project already has — the brute-force closest hit (oracle.intersect), the
reference's Distance * Distance < lightDistanceSq comparison on top of it, and
np_oracle.shade for arbitrary rays.

Every output buffer is longer than n and pre-filled with a sentinel; the tail
must come back untouched.  References are computed once per scene (module
caches) and never modified.
"""
import numpy as np
import pytest

import kat_scenes
import np_oracle as npo

pytestmark = pytest.mark.gpu

f32 = np.float32
TOL = 1e-4          # per RGB channel, Color units (tests/test_gpu_parity.py TOL)
PAD = 9             # sentinel records behind the n answers
SENT_I = 0x5A5A5A5A
SENT_F = -12345.5
FLT_MAX = np.finfo(f32).max
TAILS = (1, 63, 64, 65, 255, 256, 257)  # a partial wave, a partial 256-thread block

_cache = {}


def _cached(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- ray sets ---------------------------------------------------------------

def _random_rays(name, n=4000):
    """The recipe of tests/test_gpu_parity.py::test_intersect_rays_exact."""
    def make():
        rng = np.random.default_rng(11)
        o = rng.uniform(-1.2, 1.2, (n, 3)).astype(f32)
        if name == "demo":
            o *= 30
        d = rng.normal(size=(n, 3)).astype(f32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[: n // 10, 0] = 0.0  # axis-parallel components (rcp = +-inf)
        return np.concatenate([o, d.astype(f32)], 1)
    return _cached(("random", name, n), make)


def _scene(rt, name):
    return _cached(("scene", name), lambda: rt.make(name).scene)


def _oracle_hits(rt, orc, name, kind="random"):
    rays = _random_rays(name) if kind == "random" else _surface_rays(rt, orc, name)
    return _cached(("hits", name, kind), lambda: orc.intersect(_scene(rt, name), rays))


def _surface_rays(rt, orc, name, cap=4000):
    """Rays leaving surfaces towards the point lights (the shading's own shadow
    rays in kind): from the random set's oracle hit points, moved 1e-4 back
    along the arriving ray (a unit vector), towards every light."""
    def make():
        rays, ref = _random_rays(name), _oracle_hits(rt, orc, name)
        hit = ref["type"] != 0
        o, d, t = rays[hit, :3], rays[hit, 3:], ref["distance"][hit]
        p = (o + d * t[:, None]).astype(f32)
        org = (p - f32(1e-4) * d).astype(f32)
        out = []
        for L in np.asarray(_scene(rt, name).PointLights, f32)[:, :3]:
            v = (L[None, :] - org).astype(f32)
            v /= np.linalg.norm(v, axis=1, keepdims=True).astype(f32)
            out.append(np.concatenate([org, v.astype(f32)], 1))
        assert out, name
        r = np.stack(out, 1).reshape(-1, 6)[:cap]  # a hit point's rays to all lights stay together
        return np.ascontiguousarray(r, f32)
    return _cached(("surface", name), make)


def camera_rays(fr):
    """The 1-spp primary rays of a frame, float32 as np_oracle.render builds them."""
    cam, pl = fr.camera, fr.plane
    pos = np.asarray(cam.Position, f32)
    fwd, right, up = (np.asarray(v, f32) for v in (cam.Forward, cam.Right, cam.Up))
    rx, ry = pl.ResolutionX, pl.ResolutionY
    center = pos + fwd * f32(pl.DistanceToCamera)
    tl = (center - right * f32(pl.HalfHorizontalLength)) + up * f32(pl.HalfVerticalLength)
    H = f32(pl.HalfHorizontalLength) * f32(2)
    Vl = f32(pl.HalfVerticalLength) * f32(2)
    ys, xs = np.meshgrid(np.arange(ry), np.arange(rx), indexing="ij")
    xs = xs.reshape(-1).astype(f32)
    ys = ys.reshape(-1).astype(f32)
    rm = ((xs + f32(0.5)) * H) / f32(rx)
    dm = ((ys + f32(0.5)) * Vl) / f32(ry)
    P = (tl[None, :] + rm[:, None] * right[None, :]) - up[None, :] * dm[:, None]
    D = npo.normalize(P - pos[None, :])
    O = np.tile(pos, (len(D), 1))
    return np.ascontiguousarray(np.concatenate([O, D], 1), f32)


def occlusion_case(ref):
    """Limits cycled through {0, below t2, t2, above t2, +inf, FLT_MAX} (misses:
    1.0) and the definition's answer, all in float32."""
    n = len(ref)
    t = ref["distance"].astype(f32)
    with np.errstate(over="ignore"):
        t2 = (t * t).astype(f32)
    kind = np.arange(n) % 6
    lim = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                    [np.zeros(n, f32), np.nextafter(t2, f32(0)), t2, np.nextafter(t2, f32(np.inf)),
                     np.full(n, np.inf, f32)], np.full(n, FLT_MAX, f32)).astype(f32)
    hit = ref["type"] != 0
    lim[~hit] = f32(1.0)
    want = hit & (t2 < lim)
    return lim, want.astype(np.int32), kind, hit


# ---- device calls -----------------------------------------------------------

def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, copy=True, order="C")).cuda()  # (cached references are read-only)
    torch.cuda.synchronize()  # the context's own stream does not wait for torch's
    return t


def _sentinel(shape, dtype, value):
    import torch
    t = torch.full(shape, value, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return t


def dev_hits(rt, ctx, rays_t, n):
    import torch
    out = _sentinel((n + PAD, 4), torch.int32, SENT_I)
    ctx.intersect_rays_device(rays_t, n, out)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[n:] == SENT_I).all(), "closest hit wrote past n"
    return np.ascontiguousarray(h[:n]).view(rt.raytracing.HIT_DTYPE).reshape(-1)


def dev_occluded(ctx, rays_t, limits_t, n):
    import torch
    out = _sentinel((n + PAD,), torch.int32, SENT_I)
    ctx.occluded_rays_device(rays_t, limits_t, n, out)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[n:] == SENT_I).all(), "occlusion wrote past n"
    return h[:n].copy()


def dev_shade(ctx, rays_t, n, params, want_stats=True):
    import torch
    out = _sentinel((n + PAD, 4), torch.float32, SENT_F)
    st = ctx.shade_rays_device(rays_t, n, params, out, n * 16, want_stats=want_stats)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[n:] == f32(SENT_F)).all(), "shading wrote past n"
    return h[:n].copy(), st


def _same_hits(a, b, tag):
    for f in ("type", "index", "mesh_index"):
        assert np.array_equal(a[f], b[f]), (tag, f)
    assert np.array_equal(a["distance"].view(np.uint32), b["distance"].view(np.uint32)), tag


def _rays3(st):
    return (st.primary_rays, st.shadow_rays, st.reflection_rays)


# ---- closest hit ------------------------------------------------------------

@pytest.mark.parametrize("name", ["demo", "C2", "C3"])
def test_closest_hit_equals_oracle_and_host_path(gpu_ctx, rt, orc, name):
    """type, index, mesh_index equal and distance equal as uint32 against the
    brute-force oracle; byte-equal to rt_intersect_rays on the same rays."""
    gpu_ctx.set_scene(_scene(rt, name))
    rays = _random_rays(name)
    ref = _oracle_hits(rt, orc, name)
    got = dev_hits(rt, gpu_ctx, _dev(rays), len(rays))
    _same_hits(got, ref, name)
    assert (ref["type"] == 0).any() and (ref["type"] != 0).any(), name
    if name == "C3":
        # a sphere / loose triangle won after a mesh triangle had been the running
        # closest hit (Scene.cs:76-79 vs :94-97, :109-112): second walk + its decode
        assert ((ref["type"] != 3) & (ref["mesh_index"] >= 0)).any()
    host = gpu_ctx.intersect_rays(rays)
    assert got.tobytes() == host.tobytes(), name


def test_tail_shapes_all_three_calls(gpu_ctx, rt, orc):
    """n in a partial wave and a partial block: each answer equals the first n
    of the 4000-ray answer, nothing behind n is written."""
    name = "demo"
    gpu_ctx.set_scene(_scene(rt, name))
    rays = _random_rays(name)
    N = len(rays)
    rays_t = _dev(rays)
    ref = _oracle_hits(rt, orc, name)
    lim, want, _, _ = occlusion_case(ref)
    lim_t = _dev(lim)
    prm = rt.params_struct((0.25, 0.5, 0.75, 1.0), 3)
    full_hits = dev_hits(rt, gpu_ctx, rays_t, N)
    _same_hits(full_hits, ref, "full")
    full_occ = dev_occluded(gpu_ctx, rays_t, lim_t, N)
    assert np.array_equal(full_occ, want)
    full_any = dev_occluded(gpu_ctx, rays_t, None, N)
    assert np.array_equal(full_any, (ref["type"] != 0).astype(np.int32))
    full_col, full_st = dev_shade(gpu_ctx, rays_t, N, prm)
    assert full_st.primary_rays == N
    for n in TAILS:
        assert dev_hits(rt, gpu_ctx, rays_t, n).tobytes() == full_hits[:n].tobytes(), n
        assert np.array_equal(dev_occluded(gpu_ctx, rays_t, lim_t, n), full_occ[:n]), n
        assert np.array_equal(dev_occluded(gpu_ctx, rays_t, None, n), full_any[:n]), n
        col, st = dev_shade(gpu_ctx, rays_t, n, prm)
        assert np.array_equal(col.view(np.uint32), full_col[:n].view(np.uint32)), n
        assert st.primary_rays == n, n
        col2, none = dev_shade(gpu_ctx, rays_t, n, prm, want_stats=False)  # the stream-ordered form
        assert none is None and np.array_equal(col2.view(np.uint32), col.view(np.uint32)), n


def test_deep_tree_fills_the_private_stack(gpu_ctx, rt, orc):
    """tests/test_gpu_deep_tree.py's `loose` scene (device LBVH, one 4-wide level
    per key bit: the walks overflow the 16 LDS entries into the private stack),
    its 48x27 camera rays: closest hit and occlusion equal the oracle."""
    fr = rt.scenes.deep_chain(levels=30, res=(48, 27), spp=1)
    gpu_ctx.set_scene(fr.scene, rt.abi.RT_BUILD_LBVH_GPU)
    assert gpu_ctx.scene_info()["build"] == rt.abi.RT_BUILD_LBVH_GPU
    rays = camera_rays(fr)
    n = len(rays)
    assert n == 48 * 27
    ref = orc.intersect(fr.scene, rays)
    assert (ref["type"] != 0).sum() > n // 2
    rays_t = _dev(rays)
    _same_hits(dev_hits(rt, gpu_ctx, rays_t, n), ref, "deep")
    lim, want, _, _ = occlusion_case(ref)
    assert np.array_equal(dev_occluded(gpu_ctx, rays_t, _dev(lim), n), want)
    assert np.array_equal(dev_occluded(gpu_ctx, rays_t, None, n), (ref["type"] != 0).astype(np.int32))


# ---- occlusion --------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "surface"])
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_occlusion_definition_at_the_boundary(gpu_ctx, rt, orc, name, kind):
    """occluded = (type != 0) & (Distance * Distance < limit), float32, strict.
    Limits sit on, one ulp below and one ulp above t2 = t * t, at 0, +inf and
    FLT_MAX.  The two boundary classes — hit rays whose limit is exactly t2
    (answer 0) and hit rays whose limit is the next float above t2 (answer 1)
    — each hold at least 5 % of the set's rays, by the oracle alone."""
    gpu_ctx.set_scene(_scene(rt, name))
    rays = _random_rays(name) if kind == "random" else _surface_rays(rt, orc, name)
    ref = _oracle_hits(rt, orc, name, kind)
    n = len(rays)
    lim, want, lk, hit = occlusion_case(ref)
    at, above = hit & (lk == 2), hit & (lk == 3)
    assert at.mean() >= 0.05 and above.mean() >= 0.05, (at.mean(), above.mean())
    assert not want[at].any() and want[above].all()  # the strict '<' decides both classes
    rays_t = _dev(rays)
    got = dev_occluded(gpu_ctx, rays_t, _dev(lim), n)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, kind, bad[:8], lk[bad[:8]])
    got_any = dev_occluded(gpu_ctx, rays_t, None, n)
    assert np.array_equal(got_any, hit.astype(np.int32)), (name, kind)


# ---- stream order -----------------------------------------------------------

def test_queries_are_ordered_with_the_callers_stream(gpu_ctx, rt, orc):
    """The rays are produced by a torch op on the stream the context was
    given; the queries follow with no host synchronisation in between."""
    import torch
    name = "C2"
    gpu_ctx.set_scene(_scene(rt, name))
    rays = _random_rays(name)
    n = len(rays)
    ref = _oracle_hits(rt, orc, name)
    o_t, d_t = _dev(rays[:, :3]), _dev(rays[:, 3:])
    s = torch.cuda.Stream()
    gpu_ctx.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            hits = torch.full((n + PAD, 4), SENT_I, dtype=torch.int32, device="cuda")
            occ = torch.full((n + PAD,), SENT_I, dtype=torch.int32, device="cuda")
            rays_t = torch.cat([o_t, d_t], 1).contiguous()  # produced on s
            gpu_ctx.intersect_rays_device(rays_t, n, hits)
            gpu_ctx.occluded_rays_device(rays_t, None, n, occ)
        s.synchronize()
        h = hits.cpu().numpy()
        assert (h[n:] == SENT_I).all()
        _same_hits(np.ascontiguousarray(h[:n]).view(rt.raytracing.HIT_DTYPE).reshape(-1), ref, "stream")
        q = occ.cpu().numpy()
        assert (q[n:] == SENT_I).all()
        assert np.array_equal(q[:n], (ref["type"] != 0).astype(np.int32))
    finally:
        gpu_ctx.set_stream(None)


# ---- shading ----------------------------------------------------------------

def _shade_frames(rt):
    return {"demo": rt.make("demo"), "mirror_sphere": kat_scenes.mirror_sphere(rt, 5)[0]}


def _scene_rays(orc, scene, n=300, seed=5):
    """Random rays through a scene's box: origins in the box grown by half,
    aimed at points in the box."""
    box = orc.scene_aabb(scene).astype(np.float64)
    c, e = (box[0] + box[1]) / 2, (box[1] - box[0]) / 2
    rng = np.random.default_rng(seed)
    o = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    tgt = c + rng.uniform(-1.0, 1.0, (n, 3)) * e
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(f32)
    return np.ascontiguousarray(np.concatenate([o.astype(f32), d], 1), f32)


@pytest.mark.parametrize("max_b", [0, 3, 8])
@pytest.mark.parametrize("name", ["demo", "mirror_sphere"])
def test_shade_arbitrary_rays_equals_np_oracle(gpu_ctx, rt, orc, name, max_b):
    """300 rays no camera built, a non-black background: Color within 1e-4 per
    RGB channel of np_oracle.shade / 255, alpha exactly 1, ray counts exact."""
    fr = _shade_frames(rt)[name]
    gpu_ctx.set_scene(fr.scene)
    rays = _cached(("shade_rays", name), lambda: _scene_rays(orc, fr.scene))
    n = len(rays)
    bg = (0.25, 0.5, 0.125, 1.0)

    def reference():
        cnt = npo.Counts()
        O, D = np.array(rays[:, :3]), np.array(rays[:, 3:])
        c = npo.shade(npo.Scene(fr.scene), O, D, 0, max_b, np.asarray(bg[:3], f32) * f32(255), cnt)
        return (c / f32(255)).astype(f32), (cnt.shadow, cnt.reflection)
    want, (shadow, refl) = _cached(("shade_ref", name, max_b), reference)
    if name == "mirror_sphere":
        assert (refl > 0) == (max_b > 0)  # mirror chains are exercised
    col, st = dev_shade(gpu_ctx, _dev(rays), n, rt.params_struct(bg, max_b))
    assert np.isfinite(col).all() == np.isfinite(want).all()
    err = float(np.nanmax(np.abs(col[:, :3].astype(np.float64) - want)))
    print(f"{name} depth {max_b}: max |gpu - np_oracle| = {err:.3g}, rays {_rays3(st)}")
    assert err <= TOL, (name, max_b, err)
    assert (col[:, 3] == f32(1.0)).all()
    assert _rays3(st) == (n, shadow, refl), (name, max_b)
    assert st.shading_fetches > 0 and st.kernel_ms > 0.0 and st.total_ms > 0.0


def test_shade_camera_rays_equals_the_frame(gpu_ctx, rt, orc):
    """C2 64x36, 1 spp, depth 8: the frame's primary rays, built on the host
    with np_oracle.render's float32 formula, shade to the oracle's frame (1e-4,
    ray counts exact) and to rt_render's frame."""
    fr = rt.make("C2").with_resolution(64, 36).with_(spp=1, max_bounces=8)
    gpu_ctx.set_scene(fr.scene)
    rays = camera_rays(fr)
    n = len(rays)
    ref, counts = orc.render(fr)
    col, st = dev_shade(gpu_ctx, _dev(rays), n, rt.frame_params(fr))
    col = col.reshape(36, 64, 4)
    err = float(np.max(np.abs(col.astype(np.float64) - ref)))
    assert err <= TOL, err
    assert _rays3(st) == (counts["primary_rays"], counts["shadow_rays"], counts["reflection_rays"])
    assert counts["reflection_rays"] > 0
    img, sf = gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr))
    diff = float(np.max(np.abs(col.astype(np.float64) - img)))
    assert diff <= TOL, f"max |shade_rays - rt_render| = {diff} (0 expected)"
    assert _rays3(st) == _rays3(sf)


# ---- scene updates ----------------------------------------------------------

def test_closest_hit_after_a_transform_update(gpu_ctx, rt, orc):
    """rt_set_scene_source + rt_update_mesh_transforms: ranks (and the device
    rank table) stay, geometry moves; hits equal the oracle on the moved scene."""
    from test_gpu_scene_source import _mixed_sources
    S = rt.scenes
    fr0 = rt.make("C2").with_resolution(8, 8)
    base = S.without_meshes(fr0.scene)
    srcs = _mixed_sources(rt)
    try:
        gpu_ctx.set_scene_source(base, srcs)
        mats = np.stack([np.asarray(s.LocalToWorld, f32).reshape(4, 4) for s in srcs]).copy()
        mats[0, :3, 3] += np.array((0.3, 0.25, -0.2), f32)  # the knot
        mats[3, :3, 3] += np.array((0.0, 0.4, 0.1), f32)    # the mirror cube
        gpu_ctx.update_mesh_transforms(mats)
        host = S.extracted(fr0.with_(scene=base), srcs, mats)
        rng = np.random.default_rng(3)
        n = 3000
        o = rng.uniform(-0.9, 0.9, (n, 3)).astype(f32)
        d = rng.normal(size=(n, 3)).astype(f32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([o, d.astype(f32)], 1)
        ref = orc.intersect(host.scene, rays)
        still = orc.intersect(S.extracted(fr0.with_(scene=base), srcs).scene, rays)
        assert (ref["type"] == 3).sum() > 250
        assert not np.array_equal(ref["distance"], still["distance"])  # the move is visible to these rays
        _same_hits(dev_hits(rt, gpu_ctx, _dev(rays), n), ref, "moved")
    finally:
        gpu_ctx.set_scene(rt.make("C1").scene)


# ---- errors -----------------------------------------------------------------

def _status(rt, call):
    with pytest.raises(rt.RtError) as e:
        call()
    return e.value.status


def test_errors(gpu_ctx, rt, orc):
    import torch
    A = rt.abi
    fr = rt.make("C2").with_resolution(32, 18).with_(spp=1)
    n = 64
    rays_t = _dev(camera_rays(fr)[:n])
    hits = _sentinel((n, 4), torch.int32, SENT_I)
    occ = _sentinel((n,), torch.int32, SENT_I)
    col = _sentinel((n, 4), torch.float32, SENT_F)
    ok = rt.params_struct((0, 0, 0, 1), 2)
    fresh = rt.Context()
    try:
        assert _status(rt, lambda: fresh.intersect_rays_device(rays_t, n, hits)) == A.RT_E_STATE
        assert _status(rt, lambda: fresh.occluded_rays_device(rays_t, None, n, occ)) == A.RT_E_STATE
        assert _status(rt, lambda: fresh.shade_rays_device(rays_t, n, ok, col, n * 16)) == A.RT_E_STATE
    finally:
        fresh.close()
    gpu_ctx.set_scene(fr.scene)
    c = gpu_ctx
    bad = [
        lambda: c.intersect_rays_device(None, n, hits),
        lambda: c.intersect_rays_device(rays_t, n, None),
        lambda: c.intersect_rays_device(rays_t, -1, hits),
        lambda: c.occluded_rays_device(None, None, n, occ),
        lambda: c.occluded_rays_device(rays_t, None, n, None),
        lambda: c.occluded_rays_device(rays_t, None, -1, occ),
        lambda: c.shade_rays_device(None, n, ok, col, n * 16),
        lambda: c.shade_rays_device(rays_t, n, ok, None, n * 16),
        lambda: c.shade_rays_device(rays_t, -1, ok, col, n * 16),
        lambda: c.shade_rays_device(rays_t, n, ok, col, n * 16 - 1),
        lambda: c.shade_rays_device(rays_t, n, rt.params_struct((0, 0, 0, 1), 33), col, n * 16),
        lambda: c.shade_rays_device(rays_t, n, rt.params_struct((0, 0, 0, 1), 2, spp=4), col, n * 16),
        lambda: c.shade_rays_device(rays_t, n, rt.params_struct((0, 0, 0, 1), 2, flags=A.RT_FLAG_OUT_RGBA8), col,
                                    n * 16),
    ]
    for k, call in enumerate(bad):
        assert _status(rt, call) == A.RT_E_INVALID, k
    # n = 0: RT_OK, nothing launched, nothing written
    c.intersect_rays_device(rays_t, 0, hits)
    c.occluded_rays_device(rays_t, None, 0, occ)
    st = c.shade_rays_device(rays_t, 0, ok, col, 0, want_stats=True)
    assert _rays3(st) == (0, 0, 0)
    c.synchronize()
    assert (hits.cpu().numpy() == SENT_I).all() and (occ.cpu().numpy() == SENT_I).all()
    assert (col.cpu().numpy() == f32(SENT_F)).all()
    # the context still renders correctly
    img, sf = c.render(fr.camera, fr.plane, rt.frame_params(fr))
    ref, counts = orc.render(fr)
    assert float(np.max(np.abs(img - ref))) <= TOL
    assert _rays3(sf) == (counts["primary_rays"], counts["shadow_rays"], counts["reflection_rays"])
