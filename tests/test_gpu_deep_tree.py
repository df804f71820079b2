"""Adversarially deep trees (scenes.deep_chain): every traversal walks a tree
that fills its stacks, the too-deep rejection of the device builder and the
fallback of rt_set_scene to the host SAH run.

The suite's other scenes build shallow, balanced trees (about a dozen 4-wide
levels at most); the stacks of the packet walk (packet.h kWaveStack), the
whole-wave walk of one-sample waves (coop.h kStackReserve), the levels
kernel, the wavefront path and the shadow (ANY) walks are sized by the
builders' depth guarantee 3 * (depth4 + 1) <= kStackTotal = 128 and were
never filled by a real tree.  deep_chain makes the device LBVH one 4-wide
level deep per key bit.

That the scenes are adequate is asserted from the export and the oracle, not
taken from the kernels: the exported tree's depth (tests/bvh_invariants.py)
and the stack high-water of the oracle's walk of that tree (rt_oracle.c
bvh4_query, which makes the same box and primitive tests in number as the
per-lane kernel, tests/test_gpu_counts.py, so its high-water stands in for
the kernel's).

Reached on the MI355X (device LBVH, 48x27, 1 spp; asserted below and, for
the depths, by the CPU restatement of the build, tests/lbvh_reference.py,
in tests/test_bvh_invariants.py):
  loose  levels 30: depth4 25 (85 nodes), 2-wide depth 34; oracle stack
         high-water camera 60 / reflection 25 / shadow 42
  mesh   levels 48: depth4 38 (135 nodes), 2-wide depth 52; high-water
         camera 80 / reflection 14 / shadow 73
  outside (the loose scene seen from 2.5 in front of the box): camera 11 /
         shadow 13: near-first order from outside meets the big outer
         clusters first and prunes the chain
  mesh   levels 52: rejected, "LBVH 4-wide depth 42 exceeds the traversal
         stack" (2-wide depth 56, accepted by build 2); the host SAH tree
         rt_set_scene falls back to has depth4 11
The aim for the loose scene was 3 * depth4 - 3 = 72.  With the camera at P
the entry keys of the boxes around it tie at 0 and the chain is not always
the first child taken, hence 60.  Moving the camera off P (the same as moving
the clusters the other way) did not raise it: in the restated build's tree
the oracle's camera high-water is 58 at (0.002, 0.002, -0.004), 51 at
(0, 0, -0.01), 36 at (0, 0, -0.05), 35 at (0, 0, 0.05) and 14 at (0, 0, 0.3).
"""
import re

import numpy as np
import pytest

import bvh_invariants as bi
import lbvh_reference
from test_gpu_counts import check_counts

pytestmark = pytest.mark.gpu

TOL = 1e-4
SAH, LBVH, LBVH2 = 0, 1, 2
MESH_LEVELS = 48    # 36 <= depth4 <= 41
REJECT_LEVELS = 52  # depth4 42: 3 * 43 = 129 > 128

SCENES = {
    "loose": dict(levels=30),
    "spheres": dict(levels=30, variant="spheres"),
    "mesh": dict(levels=MESH_LEVELS, variant="mesh"),
    "outside": dict(levels=30, camera_offset=(0.0, 0.0, -2.5)),
    "far": dict(levels=30, origin=(1.0e4, 0.0, 0.0)),
}
_frames, _refs = {}, {}


def _frame(rt, name, res=(48, 27), spp=1):
    key = (name, res, spp)
    if key not in _frames:
        _frames[key] = rt.scenes.deep_chain(res=res, spp=spp, **SCENES[name])
    return _frames[key]


def _oracle(rt, orc, name, res=(48, 27), spp=1):
    """The brute-force frame, computed once per (scene, size, spp)."""
    key = (name, res, spp)
    if key not in _refs:
        _refs[key] = orc.render(_frame(rt, name, res, spp))
    return _refs[key]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _rays(st):
    return (st.primary_rays, st.shadow_rays, st.reflection_rays)


def _set(ctx, fr, build):
    """Sets the scene; a 4-wide tree is checked (its depth against the stack
    included) before any kernel walks it."""
    ctx.set_scene(fr.scene, build)
    if ctx.scene_info()["bvh_width"] == 4:
        bi.check_bvh(*ctx.export_bvh(), bi.Prims.of_scene(fr.scene), expect_nodes=ctx.scene_info()["nodes"])


def _walk(ctx, orc, fr):
    """Checker measurements of the exported tree and the oracle's walk of it."""
    tree = ctx.export_bvh()
    m = bi.check_bvh(*tree, bi.Prims.of_scene(fr.scene), expect_nodes=ctx.scene_info()["nodes"])
    b4 = orc.Bvh4Scene(fr, *tree)
    try:
        img, c = b4.render_pixels(np.arange(fr.plane.ResolutionX * fr.plane.ResolutionY, dtype=np.int32))
    finally:
        b4.close()
    return m, img, c


# scene -> oracle stack high-water (camera, reflection, shadow) of the device tree, as reached
HIGH_WATER = {"loose": (60, 25, 42), "mesh": (80, 14, 73), "outside": (11, 0, 13)}


@pytest.mark.parametrize("name", list(HIGH_WATER))
def test_deep_scenes_are_adequate(gpu_ctx, rt, orc, name):
    """The loose scene's exported depth4 satisfies 3 * depth4 > 48 (twice the
    larger LDS part of the lane stack) and the oracle's stack high-water over
    the frame's camera rays, and again over its shadow rays, exceeds 24; the
    mesh scene reaches 36 <= depth4 <= 41.  The device's tree has the depth
    and node count of the restated build, and the oracle's walk of it the
    high-waters recorded in the module docstring."""
    fr = _frame(rt, name)
    gpu_ctx.set_scene(fr.scene, LBVH)
    m, img, c = _walk(gpu_ctx, orc, fr)
    _, want = lbvh_reference.build(fr.scene)
    assert (m["depth4"], m["nodes"]) == (want["depth4"], want["nodes4"])
    assert _same(img.reshape(fr.plane.ResolutionY, -1, 4), _oracle(rt, orc, name)[0])
    high = (c["stack_high_camera"], c["stack_high_reflection"], c["stack_high_shadow"])
    if name == "loose":
        assert 3 * m["depth4"] > 48
        assert c["reflection_rays"] > 0
    if name == "mesh":
        assert 36 <= m["depth4"] <= 41
    if name != "outside":
        assert high[0] > 24 and high[2] > 24
    assert high == HIGH_WATER[name]


@pytest.mark.parametrize("build", [SAH, LBVH, LBVH2])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_traversal_equals_the_oracle(gpu_ctx, rt, orc, name, build):
    """Megakernel, wavefront, packet and row-order launches at 1 and 4 spp
    (48x27) and the levels kernel (16 spp, 24x14): each within 1e-4 of the
    brute-force frame with the same ray counts, and bit-identical to one
    another (as tests/test_gpu_parity.py holds them on the shallow scenes)."""
    A = rt.abi
    _set(gpu_ctx, _frame(rt, name), build)
    for res, spp in (((48, 27), 1), ((48, 27), 4), ((24, 14), 16)):
        fr = _frame(rt, name, res, spp)
        ref, counts = _oracle(rt, orc, name, res, spp)
        first = None
        for flags in (0, A.RT_FLAG_WAVEFRONT, A.RT_FLAG_PACKET, A.RT_FLAG_ROW_ORDER):
            img, st = gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr, flags=flags))
            tag = (name, build, res, spp, flags)
            assert np.array_equal(np.isnan(img), np.isnan(ref)), tag
            assert float(np.nanmax(np.abs(img.astype(np.float64) - ref))) <= TOL, tag
            assert _rays(st) == (counts["primary_rays"], counts["shadow_rays"], counts["reflection_rays"]), tag
            if first is None:
                first = img
            assert _same(img, first), tag


@pytest.mark.parametrize("build", [SAH, LBVH])
@pytest.mark.parametrize("name", ["loose", "spheres", "mesh"])
def test_counting_launch_equals_oracle_walk_of_the_deep_tree(gpu_ctx, rt, orc, name, build):
    """RT_FLAG_COUNT_TESTS (the per-lane traversal): box, triangle, sphere and
    shading counts equal the oracle's walk of the exported tree."""
    c = check_counts(rt, gpu_ctx, orc, _frame(rt, name), build)
    assert c["box_tests"] > 0 and c["shadow_rays"] > 0


@pytest.mark.parametrize("build", [SAH, LBVH, LBVH2])
@pytest.mark.parametrize("name", ["loose", "mesh"])
def test_intersect_rays_exact_on_the_deep_tree(gpu_ctx, rt, orc, name, build):
    fr = _frame(rt, name)
    _set(gpu_ctx, fr, build)
    rng = np.random.default_rng(21)
    n = 2000
    o = rng.uniform(-3.0, 3.0, (n, 3))
    o[: n // 2] = np.asarray(fr.camera.Position) + rng.normal(scale=0.05, size=(n // 2, 3))  # inside the chain
    d = rng.normal(size=(n, 3))
    d[n // 2:] = (np.asarray(fr.camera.Position) + rng.normal(scale=0.2, size=(n - n // 2, 3))) - o[n // 2:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    hits = gpu_ctx.intersect_rays(rays)
    ref = orc.intersect(fr.scene, rays)
    assert (ref["type"] != 0).sum() > n // 2
    for f in ("type", "index"):
        assert np.array_equal(hits[f], ref[f]), f
    mesh = ref["type"] == 3
    assert np.array_equal(hits["mesh_index"][mesh], ref["mesh_index"][mesh])
    assert np.array_equal(hits["distance"].view(np.uint32), ref["distance"].view(np.uint32))


@pytest.mark.parametrize("cap", [0, 40, 1])
def test_one_sample_waves_on_the_deep_tree(gpu_ctx, rt, orc, cap):
    """The whole-wave walk of one-sample waves (coop.h; its kStackReserve
    argument rests on the builders' depth guarantee): a lone 480x270 4-spp
    shard, three frames, against the row-order frame, which the 48x27
    comparisons above tie to the oracle."""
    fr = _frame(rt, "loose", (480, 270), 4)
    _set(gpu_ctx, fr, None)
    assert gpu_ctx.scene_info()["build"] == LBVH
    lib = gpu_ctx.lib
    assert lib.rt_debug_set(gpu_ctx.h, rt.abi.RT_DEBUG_SAMPLE_WAVE_STACK, cap) == 0
    try:
        row, sr = gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr, flags=rt.abi.RT_FLAG_ROW_ORDER))
        for _ in range(3):  # the first frame measures and sorts; later ones split
            img, st = gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr))
            assert _same(img, row)
            assert _rays(st) == _rays(sr)
        assert "s16_shift=0" in gpu_ctx.last_launch(), gpu_ctx.last_launch()
    finally:
        assert lib.rt_debug_set(gpu_ctx.h, rt.abi.RT_DEBUG_SAMPLE_WAVE_STACK, 0) == 0


def test_too_deep_tree_is_rejected_and_falls_back(gpu_ctx, rt, orc):
    """A mesh chain four key bits longer: the device builder's 4-wide tree is
    rejected (RT_E_SCENE, a depth above 41), the 2-wide build holds its own
    bound (depth2 + 1 <= 128) and renders, and rt_set_scene falls back to the
    host SAH, whose tree passes the checker and renders the oracle's frame."""
    fr = rt.scenes.deep_chain(levels=REJECT_LEVELS, variant="mesh")
    ref, counts = orc.render(fr)
    with pytest.raises(rt.RtError) as e:
        gpu_ctx.set_scene(fr.scene, LBVH)
    assert e.value.status == rt.abi.RT_E_SCENE
    msg = str(e.value)
    assert "exceeds the traversal stack" in msg
    assert int(re.search(r"4-wide depth (\d+)", msg).group(1)) > 41
    with pytest.raises(rt.RtError):  # no scene: an error, not a frame of the tree that was refused
        gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr))
    for build, want in ((LBVH2, LBVH2), (None, SAH)):
        gpu_ctx.set_scene(fr.scene, build)
        assert gpu_ctx.scene_info()["build"] == want
        img, st = gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr))
        assert float(np.nanmax(np.abs(img.astype(np.float64) - ref))) <= TOL, build
        assert _rays(st) == (counts["primary_rays"], counts["shadow_rays"], counts["reflection_rays"]), build
    m, img, c = _walk(gpu_ctx, orc, fr)
    assert m["depth4"] < 20  # the SAH splits by area and count, not by key bits (11 here)
    assert _same(img.reshape(fr.plane.ResolutionY, -1, 4), ref)
    gpu_ctx.set_scene(rt.make("C1").scene)


def test_update_that_deepens_the_tree_past_the_bound_is_an_error(gpu_ctx, rt, orc):
    """The same meshes as sources, the innermost mesh first parked in a corner
    of the scene box (its chain hangs off a shallow top: accepted, equals the
    oracle), then moved home by rt_update_mesh_transforms: the rebuilt tree is
    too deep, the update fails with RT_E_SCENE and the context reports an
    error instead of rendering."""
    S = rt.scenes
    fr = S.deep_chain(levels=REJECT_LEVELS, variant="mesh")
    base = S.without_meshes(fr.scene)
    eye = np.eye(4, dtype=np.float32)
    srcs = [rt.MeshSource(m.Triangles.reshape(-1, 3), np.arange(3 * len(m.Triangles), dtype=np.int32), eye,
                          m.MaterialData) for m in fr.scene.Meshes]
    home = np.stack([eye] * len(srcs))
    away = home.copy()
    away[-1, :3, 3] = (-0.9, 0.6, -1.0)
    parked = [rt.MeshSource(s.Vertices, s.Indices, m, s.MaterialData) for s, m in zip(srcs, away)]
    try:
        gpu_ctx.set_scene_source(base, parked)
        host = S.extracted(fr.with_(scene=base), srcs, away)
        m = bi.check_bvh(*gpu_ctx.export_bvh(), bi.Prims.of_scene(host.scene), expect_nodes=gpu_ctx.scene_info()["nodes"])
        assert m["depth4"] == lbvh_reference.build(host.scene)[1]["depth4"] < 41  # 25
        img, st = gpu_ctx.render(host.camera, host.plane, rt.frame_params(host))
        ref, counts = orc.render(host)
        assert float(np.nanmax(np.abs(img.astype(np.float64) - ref))) <= TOL
        assert _rays(st) == (counts["primary_rays"], counts["shadow_rays"], counts["reflection_rays"])
        with pytest.raises(rt.RtError) as e:
            gpu_ctx.update_mesh_transforms(home)
        assert e.value.status == rt.abi.RT_E_SCENE and "exceeds the traversal stack" in str(e.value)
        with pytest.raises(rt.RtError) as e:
            gpu_ctx.render(fr.camera, fr.plane, rt.frame_params(fr))
        assert e.value.status == rt.abi.RT_E_STATE
    finally:
        gpu_ctx.set_scene(rt.make("C1").scene)
