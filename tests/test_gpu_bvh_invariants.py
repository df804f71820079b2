"""The trees the library builds, looked at as trees (tests/bvh_invariants.py):
the host SAH build, the device LBVH (csrc/lbvh.hip: sort, Karras, k_bounds,
k_small, k_slots / k_keep / k_collapse), the per-update device rebuild with
its on-device scene box and pad (scene_xform.hip k_scene_box) and the refit
kernels (k_refit_prims / k_refit_nodes / k_refit_links).  Frames at test
resolution rarely cross one stale box among tens of thousands; the checker
looks at every slot: topology, coverage, empty slots, records bit for bit,
box containment with the builders' pad, box tightness and the 4-wide depth
the traversal stacks are sized by (3 * (depth4 + 1) <= kStackTotal)."""
import numpy as np
import pytest

import bvh_invariants as bi
from lbvh_scenes import degenerate_scenes, translated
from test_gpu_fuzz import random_frame

pytestmark = pytest.mark.gpu

SAH, LBVH = 0, 1


def _check(ctx, scene, build=None):
    info = ctx.scene_info()
    if build is not None:
        assert info["build"] == build
    assert info["bvh_width"] == 4
    tree = ctx.export_bvh()
    m = bi.check_bvh(*tree, bi.Prims.of_scene(scene), expect_nodes=info["nodes"])
    assert 1 <= m["largest_leaf"] <= 4
    return m, tree


@pytest.mark.parametrize("build", [SAH, LBVH])
@pytest.mark.parametrize("name", ["C2", "C3", "demo"])
def test_named_scene_trees(gpu_ctx, rt, name, build):
    fr = rt.make(name)
    gpu_ctx.set_scene(fr.scene, build)
    m, _ = _check(gpu_ctx, fr.scene, build)
    assert m["leaves"] >= 1


@pytest.mark.parametrize("build", [SAH, LBVH])
@pytest.mark.parametrize("which", range(6))
def test_degenerate_scene_trees(gpu_ctx, rt, which, build):
    """Colliding Morton codes, lone primitives, zero-area triangles, huge coordinates."""
    sc = degenerate_scenes(rt, rt.make("C1").with_resolution(40, 30))[which]
    gpu_ctx.set_scene(sc, build)
    _check(gpu_ctx, sc, build)


@pytest.mark.parametrize("build", [SAH, LBVH])
@pytest.mark.parametrize("seed", range(10))
def test_fuzz_scene_trees(gpu_ctx, rt, seed, build):
    fr = random_frame(rt, seed)
    gpu_ctx.set_scene(fr.scene, build)
    _check(gpu_ctx, fr.scene, build)


@pytest.mark.parametrize("build", [SAH, LBVH])
def test_far_from_origin_tree(gpu_ctx, rt, build):
    """pad_abs follows the coordinate scale (2^-13 of it): the margins hold at 2.5e4."""
    fr = translated(rt, random_frame(rt, 501, res=(48, 36)), (1.0e4, -3.0e3, 2.5e4))
    gpu_ctx.set_scene(fr.scene, build)
    m, _ = _check(gpu_ctx, fr.scene, build)
    assert m["pad_abs"] > 2.5e4 * 2.0 ** -13


def _hall_updates(rt, ctx, build, times):
    """instanced_hall(400) as a source scene: the checked tree after the
    set and after each update, against the host-extracted primitives."""
    fr, srcs, mats = rt.scenes.instanced_hall(400, res=(96, 54), spp=1, bounces=4)
    if build is None:
        ctx.set_scene_source(fr.scene, srcs)
    else:
        ctx.set_scene_source(fr.scene, srcs, build=build)
    trees = [_check(ctx, rt.scenes.extracted(fr, srcs, mats(0.0)).scene)[1]]
    for t in times:
        m = mats(t)
        ctx.update_mesh_transforms(m)
        trees.append(_check(ctx, rt.scenes.extracted(fr, srcs, m).scene)[1])
    return trees


def test_updated_source_scene_rebuilds(gpu_ctx, rt):
    """rt_update_mesh_transforms, default builder: the scene box and pad_abs
    are folded on the device; the rebuilt tree is sound after each update."""
    trees = _hall_updates(rt, gpu_ctx, None, (0.37, 1.1, 2.5))
    assert gpu_ctx.scene_info()["build"] == LBVH
    assert not np.array_equal(trees[0][0], trees[1][0])


def _refits(trees):
    """How many of the updates kept the child refs and changed the boxes."""
    child = [bi.parse(*t)[2] for t in trees]
    return sum(a.shape == b.shape and np.array_equal(a, b) and not np.array_equal(x[0], y[0])
               for a, b, x, y in zip(child, child[1:], trees, trees[1:]))


def test_updated_source_scene_refits(gpu_ctx, rt):
    """RT_BUILD_SAH_REFIT: new records and boxes from k_refit_prims /
    k_refit_nodes / k_refit_links after each update.  Of the hall's own steps
    some take the host rebuild (the refitted area grows past kRefitRebuild);
    of three small steps at least one is a refit: same child refs, new boxes."""
    _hall_updates(rt, gpu_ctx, rt.abi.RT_BUILD_SAH_REFIT, (0.37, 1.1, 2.5))
    assert gpu_ctx.scene_info()["build"] == rt.abi.RT_BUILD_SAH_REFIT
    trees = _hall_updates(rt, gpu_ctx, rt.abi.RT_BUILD_SAH_REFIT, (0.01, 0.02, 0.03))
    assert gpu_ctx.scene_info()["build"] == rt.abi.RT_BUILD_SAH_REFIT
    assert _refits(trees) >= 1


def test_refit_large_motion_rebuild_tree(gpu_ctx, rt):
    """Every box jumps to another box's place: the refitted tree's area
    explodes and the update rebuilds it on the host; the tree stays sound."""
    fr, srcs, mats = rt.scenes.instanced_hall(400, res=(96, 54), spp=1, bounces=4)
    gpu_ctx.set_scene_source(fr.scene, srcs, build=rt.abi.RT_BUILD_SAH_REFIT)
    m0 = mats(0.0)
    _, before = _check(gpu_ctx, rt.scenes.extracted(fr, srcs, m0).scene)
    rng = np.random.default_rng(5)
    rebuilt = 0
    for step in range(3):
        m = m0.copy()
        m[:, :3, 3] = m0[rng.permutation(len(m)), :3, 3]
        gpu_ctx.update_mesh_transforms(m)
        _, tree = _check(gpu_ctx, rt.scenes.extracted(fr, srcs, m).scene)
        a, b = bi.parse(*before)[2], bi.parse(*tree)[2]
        rebuilt += a.shape != b.shape or not np.array_equal(a, b)
        before = tree
    assert rebuilt >= 1  # the case is the host rebuild, not one more refit


def test_ten_lbvh_builds_of_c3_are_sound_and_equal(gpu_ctx, rt):
    """k_bounds hands child boxes to the parent with relaxed agent-scope
    stores and an arrival counter: ten builds in a row, each checked slot by
    slot, all bitwise equal."""
    fr = rt.make("C3")
    prims = bi.Prims.of_scene(fr.scene)
    first = None
    for k in range(10):
        gpu_ctx.set_scene(fr.scene, LBVH)
        tree = gpu_ctx.export_bvh()
        bi.check_bvh(*tree, prims, expect_nodes=gpu_ctx.scene_info()["nodes"])
        if first is None:
            first = tree
        for x, y in zip(first, tree):
            assert np.array_equal(x, y), k
