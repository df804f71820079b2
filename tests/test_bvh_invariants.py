"""The tree checker (tests/bvh_invariants.py) checked on the CPU: a small
median-split builder written here emits the export format of rt_export_bvh
for a mixed scene (two meshes, spheres, loose triangles); the checker passes
on that tree and raises, with the right kind of violation, on every single
mutation the GPU tests (tests/test_gpu_bvh_invariants.py) rely on it to see."""
import numpy as np
import pytest

import bvh_invariants as bi
import lbvh_reference

f32 = np.float32


def _scene(rt):
    S = rt.scenes
    rng = np.random.default_rng(7)
    sc = rt.Scene()
    cv, ci = S.unit_cube()
    for pos, yaw in (((-0.6, 0.1, 0.2), 0.3), ((0.7, -0.2, -0.1), 1.1)):
        m = rt.scene.quaternion_trs(pos, S.yaw_quaternion(yaw), (0.4, 0.5, 0.3))
        sc.add_mesh(rt.Mesh.from_vertices(cv, ci, S.BOX_MAT, m))
    for _ in range(6):
        sc.add_sphere_r2(rng.uniform(-1, 1, 3), float(rng.uniform(0.01, 0.1)), S.MIRROR)
    c = rng.uniform(-1, 1, (10, 1, 3))
    sc.add_triangles((c + rng.uniform(-0.2, 0.2, (10, 3, 3))).astype(f32), [S.BOX_MAT] * 10)
    return sc


def _padded(prims):
    """Per rank: padded float32 box (the builders' rule), centroid, kind, gate."""
    pad_abs = f32(prims.pad_abs())
    out = []
    tri_sets = [(prims.mesh_tris, prims.mesh_gate, 0), (prims.loose_tris, np.full(prims.nl, -1), prims.mt + prims.ns)]
    for tris, gates, base in tri_sets:
        for i, t in enumerate(tris):
            lo, hi = t.min(0), t.max(0)
            pad = f32(pad_abs + f32((hi - lo).max() * f32(1e-4)))
            out.append((base + i, lo - pad, hi + pad, 0.5 * (lo + hi), 0, int(gates[i])))
    for i, s in enumerate(prims.spheres):
        r = f32(np.sqrt(s[3]))
        pad = f32(pad_abs + f32(r * f32(1e-4)))
        out.append((prims.mt + i, s[:3] - r - pad, s[:3] + r + pad, s[:3].copy(), 1, -1))
    return sorted(out, key=lambda p: p[0])


def _records(prims, tri_ranks, sph_ranks):
    tri = np.zeros((len(tri_ranks) + 1, 12), f32)
    ti = tri.view(np.int32)
    for k, r in enumerate(tri_ranks):
        t = prims.mesh_tris[r] if r < prims.mt else prims.loose_tris[r - prims.mt - prims.ns]
        tri[k, :9] = np.concatenate([t[0], t[1] - t[0], t[2] - t[0]])
        ti[k, 9], ti[k, 10] = r, prims.mesh_gate[r] if r < prims.mt else -1
    ti[-1, 9], ti[-1, 10] = 0x7fffffff, -1
    sph = np.zeros((len(sph_ranks), 8), f32)
    for k, r in enumerate(sph_ranks):
        sph[k, :4] = prims.spheres[r - prims.mt]
        sph.view(np.int32)[k, 4:6] = r, -1
    return tri.view(np.uint8).reshape(-1), sph.view(np.uint8).reshape(-1)


def _emit(node_list, n_tri):
    """node_list: per node a list of <= 4 (lo, hi, ref); the rest are empty slots."""
    w = np.full((len(node_list), 32), np.inf, f32)
    wi = w.view(np.int32)
    wi[:, 24:28] = bi.leaf_ref(n_tri, 1, 0)
    wi[:, 28:32] = 0
    for n, slots in enumerate(node_list):
        for s, (lo, hi, ref) in enumerate(slots):
            for a in range(3):
                w[n, 8 * a + s], w[n, 8 * a + 4 + s] = lo[a], hi[a]
            wi[n, 24 + s] = ref
    return w.view(np.uint8).reshape(-1)


def build_median(prims):
    """Median splits on the longest centroid axis, two per node, into the
    export format; leaves hold <= 4 primitives of one kind and gate."""
    P = _padded(prims)
    tri_ranks, sph_ranks, node_list = [], [], []

    def box(ps):
        return np.min([p[1] for p in ps], 0), np.max([p[2] for p in ps], 0)

    def halves(ps):
        c = np.array([p[3] for p in ps])
        a = int(np.argmax(c.max(0) - c.min(0)))
        ps = sorted(ps, key=lambda p: p[3][a])
        return ps[:len(ps) // 2], ps[len(ps) // 2:]

    def leafable(ps):
        return len(ps) <= 4 and len({(p[4], p[5]) for p in ps}) == 1

    def node(ps):
        idx = len(node_list)
        node_list.append(None)
        parts = []
        for h in halves(ps):
            parts += [h] if leafable(h) else list(halves(h))
        slots = []
        for part in parts:
            lo, hi = box(part)
            if leafable(part):
                order = tri_ranks if part[0][4] == 0 else sph_ranks
                slots.append((lo, hi, bi.leaf_ref(len(order), len(part), part[0][4])))
                order += [p[0] for p in part]
            else:
                slots.append((lo, hi, node(part)))
        node_list[idx] = slots
        return idx

    node(P)
    tris, sphs = _records(prims, tri_ranks, sph_ranks)
    return _emit(node_list, len(tri_ranks)), tris, sphs


def build_chain(n_nodes):
    """A comb: node i holds one triangle leaf and node i + 1; 4-wide depth n_nodes - 1."""
    rng = np.random.default_rng(3)
    c = rng.uniform(-1, 1, (n_nodes + 1, 1, 3))
    loose = (c + rng.uniform(-0.1, 0.1, (n_nodes + 1, 3, 3))).astype(f32)
    prims = bi.Prims([], [], [], loose, [])
    P = _padded(prims)
    node_list = []
    for i in range(n_nodes):
        rest = P[i + 1:]
        lo, hi = np.min([p[1] for p in rest], 0), np.max([p[2] for p in rest], 0)
        nxt = (lo, hi, i + 1) if i + 1 < n_nodes else (P[i + 1][1], P[i + 1][2], bi.leaf_ref(i + 1, 1, 0))
        node_list.append([(P[i][1], P[i][2], bi.leaf_ref(i, 1, 0)), nxt])
    tris, sphs = _records(prims, list(range(n_nodes + 1)), [])
    return prims, (_emit(node_list, n_nodes + 1), tris, sphs)


@pytest.fixture(scope="module")
def tree(rt):
    prims = bi.Prims.of_scene(_scene(rt))
    return prims, build_median(prims)


def _words(nodes):
    w = nodes.view(f32).reshape(-1, 32)
    return w, w.view(np.int32)


def _slots(nodes, want):
    """(node, slot) of the used slots whose ref is a node (want 'node') or a leaf."""
    _, wi = _words(nodes)
    refs = wi[:, 24:28]
    empty = np.isposinf(nodes.view(f32).reshape(-1, 32)[:, 0:4])
    m = ((refs >= 0) if want == "node" else (refs < 0)) & ~empty
    return np.argwhere(m)


def test_checker_passes_on_a_sound_tree(tree):
    prims, (nodes, tris, sphs) = tree
    assert prims.mt == 24 and prims.ns == 6 and prims.nl == 10
    m = bi.check_bvh(nodes, tris, sphs, prims, expect_nodes=len(nodes) // 128)
    assert m["nodes"] == len(nodes) // 128 > 4 and m["depth4"] >= 2
    assert 1 <= m["largest_leaf"] <= 4 and m["empty_slots"] >= 0
    # the builders' pad, less the inward rounding of the float32 subtraction
    assert 0.5 * m["pad_abs"] <= m["min_margin"] <= 1.5 * m["pad_abs"]
    with pytest.raises(bi.BvhViolation) as e:
        bi.check_bvh(nodes, tris, sphs, prims, expect_nodes=len(nodes) // 128 + 1)
    assert e.value.what == "topology"


def _mutations():
    def face_inward(nodes, tris, sphs, prims):
        w, _ = _words(nodes)
        n, s = _slots(nodes, "leaf")[0]
        w[n, s] = 0.5 * (w[n, s] + w[n, 4 + s])  # lo.x to the middle of the box
        return "box-inside"

    def face_outward(nodes, tris, sphs, prims):
        w, _ = _words(nodes)
        n, s = _slots(nodes, "node")[-1]
        w[n, 8 + 4 + s] += f32(1e-3) * (w[n, 8 + 4 + s] - w[n, 8 + s])  # hi.y out by 1e-3 of the extent
        return "box-outside"

    def leaf_face_outward(nodes, tris, sphs, prims):
        w, _ = _words(nodes)
        n, s = _slots(nodes, "leaf")[-1]
        w[n, 16 + s] -= f32(1e-3) * (w[n, 16 + 4 + s] - w[n, 16 + s])  # lo.z
        return "box-outside"

    def primitive_dropped(nodes, tris, sphs, prims):
        _, wi = _words(nodes)
        for n, s in _slots(nodes, "leaf"):
            v = ~wi[n, 24 + s]
            if (v >> 27) & 3:
                wi[n, 24 + s] = ~(v - (1 << 27))
                return "coverage"
        raise AssertionError("no leaf of two")

    def leaf_duplicated(nodes, tris, sphs, prims):
        _, wi = _words(nodes)
        (n0, s0), (n1, s1) = _slots(nodes, "leaf")[[0, -1]]
        wi[n1, 24 + s1] = wi[n0, 24 + s0]
        return "coverage"

    def gates_mixed(nodes, tris, sphs, prims):
        t = tris.view(np.int32).reshape(-1, 12)
        a = int(np.argmax(t[:, 10] == 0))
        b = int(np.argmax(t[:, 10] == 1))
        t[[a, b]] = t[[b, a]]  # two whole records swap places: each is right, their leaves are not
        return "gate"

    def kinds_mixed(nodes, tris, sphs, prims):
        tris.view(np.int32).reshape(-1, 12)[3, 9] = prims.mt + 1  # a sphere's rank in a triangle leaf
        return "kind"

    def kind_bit_flipped(nodes, tris, sphs, prims):
        _, wi = _words(nodes)
        n, s = _slots(nodes, "leaf")[0]
        wi[n, 24 + s] = ~((~wi[n, 24 + s]) ^ (1 << 29))
        return "coverage"

    def empty_to_root(nodes, tris, sphs, prims):
        w, wi = _words(nodes)
        n, s = np.argwhere(np.isposinf(w[:, 0:4]))[0]
        wi[n, 24 + s] = 0
        return "empty"

    def empty_with_a_box(nodes, tris, sphs, prims):
        w, _ = _words(nodes)
        n, s = np.argwhere(np.isposinf(w[:, 0:4]))[0]
        w[n, 4 + s] = -np.inf  # hi.x = -inf: a slot the kernels' "lo == hi == +inf" test takes for used
        return "empty"

    def ref_out_of_range(nodes, tris, sphs, prims):
        _, wi = _words(nodes)
        n, s = _slots(nodes, "node")[0]
        wi[n, 24 + s] = len(nodes) // 128
        return "topology"

    def node_unreachable(nodes, tris, sphs, prims):
        _, wi = _words(nodes)
        (n0, s0), (n1, s1) = _slots(nodes, "node")[[0, 1]]
        wi[n1, 24 + s1] = wi[n0, 24 + s0]  # one node twice, another never
        return "topology"

    def back_to_root(nodes, tris, sphs, prims):
        _, wi = _words(nodes)
        n, s = _slots(nodes, "node")[-1]
        wi[n, 24 + s] = 0
        return "topology"

    def e1_bit(nodes, tris, sphs, prims):
        tris.view(np.uint32).reshape(-1, 12)[5, 4] ^= 1
        return "record"

    def v0_bit(nodes, tris, sphs, prims):
        tris.view(np.uint32).reshape(-1, 12)[0, 2] ^= 1
        return "record"

    def sphere_r2_bit(nodes, tris, sphs, prims):
        sphs.view(np.uint32).reshape(-1, 8)[2, 3] ^= 1
        return "record"

    def wrong_gate(nodes, tris, sphs, prims):
        t = tris.view(np.int32).reshape(-1, 12)
        t[t[:, 10] == 1, 10] = 0  # a whole mesh under the other mesh's gate: leaves stay homogeneous
        return "gate"

    def sentinel_not_last(nodes, tris, sphs, prims):
        tris.view(np.int32).reshape(-1, 12)[-1, 9] = 0
        return "coverage"

    return [face_inward, face_outward, leaf_face_outward, primitive_dropped, leaf_duplicated, gates_mixed, kinds_mixed,
            kind_bit_flipped, empty_to_root, empty_with_a_box, ref_out_of_range, node_unreachable, back_to_root, e1_bit,
            v0_bit, sphere_r2_bit, wrong_gate, sentinel_not_last]


@pytest.mark.parametrize("mutate", _mutations(), ids=lambda f: f.__name__)
def test_checker_sees_a_single_mutation(tree, mutate):
    prims, arrays = tree
    nodes, tris, sphs = (a.copy() for a in arrays)
    what = mutate(nodes, tris, sphs, prims)
    assert any(not np.array_equal(a, b) for a, b in zip(arrays, (nodes, tris, sphs)))
    with pytest.raises(bi.BvhViolation) as e:
        bi.check_bvh(nodes, tris, sphs, prims)
    assert e.value.what == what, str(e.value)


def test_checker_sees_a_tree_one_level_too_deep():
    """3 * (depth4 + 1) <= 128: depth 41 is the deepest tree the traversal
    stack holds; a chain one level deeper is rejected."""
    prims, arrays = build_chain(42)
    assert bi.check_bvh(*arrays, prims)["depth4"] == 41
    prims, arrays = build_chain(43)
    with pytest.raises(bi.BvhViolation) as e:
        bi.check_bvh(*arrays, prims)
    assert e.value.what == "depth" and "42" in str(e.value)
    assert bi.check_bvh(*arrays, prims, stack_total=129)["depth4"] == 42


def test_oracle_walk_reports_its_stack_high_water(rt, orc):
    """Bvh4Scene.render_pixels counts carry the most entries the 4-wide walk
    (rt_oracle.c bvh4_query) held at once, per ray class: on a comb of two
    children per node that is at most one entry per level, and at least one
    where a ray enters both children of the root."""
    prims, arrays = build_chain(12)
    S = rt.scenes
    sc = rt.Scene()
    sc.add_triangles(prims.loose_tris, [S.BOX_MAT] * prims.nl)
    sc.add_point_light((0.0, 0.0, -2.0), 50.0)
    sc.AmbientLight = np.array(S.AMBIENT, f32)
    fr = S.Frame("comb", sc, S.CameraData(Position=(0.0, 0.0, -3.4)), S.ImagePlane(32, 32, 1.0, 0.5, 0.5))
    b4 = orc.Bvh4Scene(fr, *arrays)
    try:
        idx = np.arange(32 * 32, dtype=np.int32)
        img, c = b4.render_pixels(idx, threads=2)
        ref, cr = orc.render_pixels(fr, idx, threads=2)
    finally:
        b4.close()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert c["shadow_rays"] == cr["shadow_rays"] > 0
    assert 1 <= c["stack_high_camera"] <= 12 and 1 <= c["stack_high_shadow"] <= 12
    assert c["stack_high_reflection"] == 0  # no mirrors
    assert "stack_high_camera" not in cr  # the brute-force scan has no stack


def test_deep_chain_scenes(rt, orc):
    """scenes.deep_chain: 16 primitives per key bit plus the two pins, the
    scene box pinned to [-1, 1]^3, the camera inside it; the mesh variant has
    one mesh per top-level key bit and the innermost mesh that carries the
    rest of the chain, centred on the camera's cell."""
    S = rt.scenes
    fr = S.deep_chain(levels=30)
    assert fr.scene.triangle_count == 2 + 30 * 16 and not fr.scene.Meshes
    assert np.array_equal(orc.scene_aabb(fr.scene), [[-1, -1, -1], [1, 1, 1]])
    assert np.all(np.abs(fr.camera.Position) < 1)
    sp = S.deep_chain(levels=30, variant="spheres").scene
    assert len(sp.SphereData.Spheres) == 10 * 16 and sp.triangle_count == 2 + 20 * 16
    cam = np.asarray(fr.camera.Position, f32)
    assert np.all(np.linalg.norm(sp.SphereData.Spheres[:, :3] - cam, axis=1) ** 2 > sp.SphereData.Spheres[:, 3])
    me = S.deep_chain(levels=48, variant="mesh").scene
    assert len(me.Meshes) == 31 and me.triangle_count == 2 + 30 * 16 + 2 + 18 * 16
    inner = me.Meshes[-1].AABB
    assert np.all(np.abs(0.5 * (inner[0] + inner[1]) - cam) < 2.0 / 1024)
    assert np.array_equal(orc.scene_aabb(me), [[-1, -1, -1], [1, 1, 1]])
    far = S.deep_chain(levels=30, origin=(1.0e4, 0.0, 0.0))
    assert np.array_equal(orc.scene_aabb(far.scene), np.array([[9999, -1, -1], [10001, 1, 1]], f32))


# scene -> (2-wide depth, 4-wide depth, 4-wide nodes) of the device LBVH, by its CPU restatement
DEEP_DEPTHS = {
    "loose30": (dict(levels=30), (34, 25, 85)),
    "spheres30": (dict(levels=30, variant="spheres"), (34, 19, 73)),
    "mesh48": (dict(levels=48, variant="mesh"), (52, 38, 135)),
    "mesh52": (dict(levels=52, variant="mesh"), (56, 42, 147)),  # 3 * (42 + 1) = 129 > 128: rejected
}


@pytest.mark.parametrize("name", list(DEEP_DEPTHS))
def test_deep_chain_depths_by_the_cpu_restatement_of_the_lbvh(rt, name):
    """tests/lbvh_reference.py builds what csrc/lbvh.hip builds: its tree of
    each deep_chain scene is sound (checker) and one 4-wide level deep per
    key bit where the clusters are triangles.  tests/test_gpu_deep_tree.py
    holds the device's trees to the same depths and node counts."""
    kw, (depth2, depth4, nodes4) = DEEP_DEPTHS[name]
    fr = rt.scenes.deep_chain(**kw)
    tree, info = lbvh_reference.build(fr.scene)
    m = bi.check_bvh(*tree, bi.Prims.of_scene(fr.scene), expect_nodes=nodes4, stack_total=3 * (depth4 + 1))
    assert (info["depth2"], info["depth4"], info["nodes4"]) == (depth2, depth4, nodes4)
    assert m["depth4"] == depth4
    if depth4 > 41:
        with pytest.raises(bi.BvhViolation) as e:
            bi.check_bvh(*tree, bi.Prims.of_scene(fr.scene))
        assert e.value.what == "depth"


def test_lbvh_restatement_on_ordinary_scenes(rt, orc):
    """The restated build on C2 and the demo (meshes, spheres, loose
    triangles): a sound tree whose oracle walk renders the brute-force frame."""
    for name, res in (("C2", (48, 27)), ("demo", None)):
        fr = rt.make(name)
        if res:
            fr = fr.with_resolution(*res)
        tree, info = lbvh_reference.build(fr.scene)
        assert bi.check_bvh(*tree, bi.Prims.of_scene(fr.scene))["depth4"] == info["depth4"]
        b4 = orc.Bvh4Scene(fr, *tree)
        try:
            idx = np.arange(fr.plane.ResolutionX * fr.plane.ResolutionY, dtype=np.int32)
            img, _ = b4.render_pixels(idx, threads=2)
            ref, _ = orc.render_pixels(fr, idx, threads=2)
        finally:
            b4.close()
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), name
