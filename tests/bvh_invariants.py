"""A checker for the 4-wide BVH as Context.export_bvh() returns it (the byte
records of rt_device.h: 128-B nodes, 48-B triangle and 32-B sphere records),
against the scene the tree was built from.  Plain numpy; float64 wherever
arithmetic is done.  The walk is one vectorised step per tree level.

check_bvh() returns a dict of measurements and raises BvhViolation, naming
the offending node / slot / record, on the first broken invariant:

topology  every node index in [0, nodes) is reached exactly once from node 0;
          no child ref points to node 0 or out of range
coverage  every triangle rank and every sphere rank sits in exactly one leaf;
          leaf ranges are disjoint and inside the record arrays; leaf count
          1..4; the sentinel record is last and only empty slots refer to it
empty     lo = hi = +inf on all three axes; the ref is the sentinel leaf
leaves    homogeneous in kind and mesh gate; rank and gate agree with the
          scene; v0, e1 = fl32(v1 - v0), e2 = fl32(v2 - v0) and the sphere's
          centre and r^2 bit for bit
boxes     lower bound: each slot's box contains the float64 union of the
          primitives under it (triangle vertices, centre +- sqrt(r^2)) with a
          margin of at least half the builders' pad, pad_abs + ext * 1e-4
          (half: the float32 subtractions may round inward by less than that)
          upper bound: no face lies further out than the float64 union of the
          padded primitive boxes plus 2 float32 ulp of the largest coordinate
          magnitude of the box (the rounding of lo - pad and of pad itself;
          min / max are exact) — a stale or foreign box fails this
depth     3 * (depth4 + 1) <= 128 (kStackTotal), depth4 measured by the walk
          with the root at depth 0
"""
import numpy as np

STACK_TOTAL = 128  # rt_device.h kStackTotal
F32_MAX = np.float32(np.finfo(np.float32).max)


class BvhViolation(AssertionError):
    def __init__(self, what, detail):
        super().__init__(f"{what}: {detail}")
        self.what = what


class Prims:
    """The scene's primitives in rank order: mesh triangles (mesh by mesh),
    then spheres, then loose triangles; and the mesh gate boxes."""

    def __init__(self, mesh_tris, mesh_gate, spheres, loose_tris, gates):
        self.mesh_tris = np.ascontiguousarray(mesh_tris, np.float32).reshape(-1, 3, 3)
        self.mesh_gate = np.ascontiguousarray(mesh_gate, np.int32).reshape(-1)
        self.spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        self.loose_tris = np.ascontiguousarray(loose_tris, np.float32).reshape(-1, 3, 3)
        self.gates = np.ascontiguousarray(gates, np.float32).reshape(-1, 2, 3)
        assert len(self.mesh_gate) == len(self.mesh_tris)
        self.mt, self.ns, self.nl = len(self.mesh_tris), len(self.spheres), len(self.loose_tris)

    @staticmethod
    def of_scene(scene):
        ms = scene.Meshes
        mesh_tris = np.concatenate([np.asarray(m.Triangles, np.float32).reshape(-1, 3, 3) for m in ms]) if ms else []
        mesh_gate = np.concatenate([np.full(len(m.Triangles), i, np.int32) for i, m in enumerate(ms)]) if ms else []
        gates = np.stack([np.asarray(m.AABB, np.float32) for m in ms]) if ms else []
        return Prims(mesh_tris, mesh_gate, scene.SphereData.Spheres, scene.TriangleData.Triangles, gates)

    def pad_abs(self):
        """rt_scene.cpp pad_abs_of over Scene.CalculateAABB (mesh gate boxes,
        loose vertices, sphere centre -+ fl32(sqrt(r^2)) in float32): 2^-13 of
        the largest finite coordinate magnitude of the scene box, at least 1."""
        lo = np.full(3, F32_MAX, np.float32)
        hi = np.full(3, -F32_MAX, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            if len(self.gates):
                lo = np.fmin(lo, np.nanmin(self.gates[:, 0], 0))
                hi = np.fmax(hi, np.nanmax(self.gates[:, 1], 0))
            if self.nl:
                v = self.loose_tris.reshape(-1, 3)
                lo, hi = np.fmin(lo, v.min(0)), np.fmax(hi, v.max(0))
            if self.ns:
                r = np.sqrt(self.spheres[:, 3]).astype(np.float32)[:, None]
                c = self.spheres[:, :3]
                lo, hi = np.fmin(lo, (c - r).min(0)), np.fmax(hi, (c + r).max(0))
        v = np.abs(np.concatenate([lo, hi]).astype(np.float64))
        v = v[np.isfinite(v)]
        return float(np.float32(max(1.0, v.max() if len(v) else 1.0)) * np.float32(2.0 ** -13))


def leaf_ref(first, count, kind):
    return ~(int(first) | ((int(count) - 1) << 27) | (int(kind) << 29))


def parse(nodes, tris, sphs):
    """(lo[N,4,3], hi[N,4,3], child[N,4], tri_f[T,12], tri_i[T,12], sph_f[S,8], sph_i[S,8])"""
    nb = np.ascontiguousarray(nodes, np.uint8)
    tb = np.ascontiguousarray(tris, np.uint8)
    sb = np.ascontiguousarray(sphs, np.uint8)
    if len(nb) % 128 or len(tb) % 48 or len(sb) % 32:
        raise BvhViolation("format", f"byte lengths {len(nb)}, {len(tb)}, {len(sb)}")
    w = nb.view(np.float32).reshape(-1, 32)
    lo = np.stack([w[:, 0:4], w[:, 8:12], w[:, 16:20]], -1)
    hi = np.stack([w[:, 4:8], w[:, 12:16], w[:, 20:24]], -1)
    child = nb.view(np.int32).reshape(-1, 32)[:, 24:28]
    return (lo, hi, child, tb.view(np.float32).reshape(-1, 12), tb.view(np.int32).reshape(-1, 12),
            sb.view(np.float32).reshape(-1, 8), sb.view(np.int32).reshape(-1, 8))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_bvh(nodes, tris, sphs, prims, expect_nodes=None, stack_total=STACK_TOTAL):
    lo, hi, child, tri_f, tri_i, sph_f, sph_i = parse(nodes, tris, sphs)
    N, T, S = len(lo), len(tri_f) - 1, len(sph_f)
    MT, NS, NL = prims.mt, prims.ns, prims.nl
    if N < 1:
        raise BvhViolation("topology", "no nodes")
    if expect_nodes is not None and N != expect_nodes:
        raise BvhViolation("topology", f"{N} exported nodes, scene_info says {expect_nodes}")
    if T != MT + NL or S != NS:
        raise BvhViolation("coverage", f"{T} triangle and {S} sphere records for {MT + NL} triangles and {NS} spheres")
    # ---- the sentinel record is last: never hit (zero edges), no rank of the scene
    if tri_i[T, 9] != 0x7fffffff or tri_i[T, 10] != -1 or np.any(tri_f[T, 3:9] != 0.0):
        raise BvhViolation("coverage", f"the last triangle record {T} is not the sentinel")
    sentinel = leaf_ref(T, 1, 0)

    # ---- slots: empty, node, leaf
    is_node = child >= 0
    v = ~child
    first = v & ((1 << 27) - 1)
    count = ((v >> 27) & 3) + 1
    kind = (v >> 29) & 1
    pinf = np.isposinf(lo).all(-1) & np.isposinf(hi).all(-1)
    any_pinf = np.isposinf(lo).any(-1) | np.isposinf(hi).any(-1)
    to_sentinel = ~is_node & (kind == 0) & (first + count > T)
    empty = any_pinf | (child == sentinel)
    bad = empty & ~(pinf & (child == sentinel))
    if bad.any():
        n, s = np.argwhere(bad)[0]
        raise BvhViolation("empty", f"node {n} slot {s}: ref {child[n, s]} (sentinel {sentinel}), lo {lo[n, s]}, hi {hi[n, s]}")
    bad = to_sentinel & ~empty
    if bad.any():
        n, s = np.argwhere(bad)[0]
        raise BvhViolation("coverage", f"node {n} slot {s}: a used leaf [{first[n, s]}, +{count[n, s]}) reaches the sentinel {T}")
    bad = ~is_node & ((v >> 30) != 0)
    if bad.any():
        n, s = np.argwhere(bad)[0]
        raise BvhViolation("topology", f"node {n} slot {s}: malformed leaf ref {child[n, s]}")
    node_slot = is_node
    leaf_slot = ~is_node & ~empty

    # ---- topology: level by level from node 0
    bad = node_slot & ((child >= N) | (child == 0))
    if bad.any():
        n, s = np.argwhere(bad)[0]
        raise BvhViolation("topology", f"node {n} slot {s}: child ref {child[n, s]} (nodes {N})")
    seen = np.zeros(N, np.int64)
    seen[0] = 1
    parent = np.full(N, -1, np.int64)
    pslot = np.full(N, -1, np.int64)
    levels = [np.zeros(1, np.int64)]
    while True:
        f = levels[-1]
        m = node_slot[f]
        if not m.any():
            break
        kids = child[f][m].astype(np.int64)
        pn = np.repeat(f, 4).reshape(-1, 4)[m]
        ps = np.tile(np.arange(4), len(f)).reshape(-1, 4)[m]
        np.add.at(seen, kids, 1)
        if (seen[kids] > 1).any():
            k = kids[seen[kids] > 1][0]
            raise BvhViolation("topology", f"node {k} is reached more than once (again from node {pn[kids == k][-1]})")
        parent[kids], pslot[kids] = pn, ps
        levels.append(kids)
    if (seen != 1).any():
        raise BvhViolation("topology", f"node {int(np.argmin(seen))} is not reachable from node 0")
    depth4 = len(levels) - 1

    # ---- leaves: ranges, coverage
    ln, ls = np.nonzero(leaf_slot)
    lf, lc, lk = first[ln, ls].astype(np.int64), count[ln, ls].astype(np.int64), kind[ln, ls]
    cap = np.where(lk == 0, T, S)
    bad = lf + lc > cap
    if bad.any():
        i = np.argmax(bad)
        raise BvhViolation("coverage", f"node {ln[i]} slot {ls[i]}: leaf [{lf[i]}, +{lc[i]}) of kind {lk[i]} outside {cap[i]} records")
    for k, n_rec, name in ((0, T, "triangle"), (1, S, "sphere")):
        use = np.zeros(n_rec + 1, np.int64)
        sel = lk == k
        np.add.at(use, lf[sel], 1)
        np.add.at(use, lf[sel] + lc[sel], -1)
        use = np.cumsum(use)[:n_rec]
        if (use > 1).any():
            r = int(np.argmax(use > 1))
            raise BvhViolation("coverage", f"{name} record {r} lies in {use[r]} leaves")
        if (use < 1).any():
            r = int(np.argmax(use < 1))
            raise BvhViolation("coverage", f"{name} record {r} lies in no leaf")
    # ---- records against the scene
    trank, tgate = tri_i[:T, 9], tri_i[:T, 10]
    is_mesh = (trank >= 0) & (trank < MT)
    is_loose = (trank >= MT + NS) & (trank < MT + NS + NL)
    if (~(is_mesh | is_loose)).any():
        r = int(np.argmax(~(is_mesh | is_loose)))
        raise BvhViolation("kind", f"triangle record {r} carries rank {trank[r]}, no triangle rank "
                                   f"(mesh [0, {MT}), loose [{MT + NS}, {MT + NS + NL}))")
    srank = sph_i[:, 4]
    if ((srank < MT) | (srank >= MT + NS)).any():
        r = int(np.argmax((srank < MT) | (srank >= MT + NS)))
        raise BvhViolation("kind", f"sphere record {r} carries rank {srank[r]}, no sphere rank [{MT}, {MT + NS})")
    for ranks, n_rank, base, name in ((trank[is_mesh], MT, 0, "mesh triangle"),
                                      (trank[is_loose], NL, MT + NS, "loose triangle"), (srank, NS, MT, "sphere")):
        c = np.bincount(ranks - base, minlength=n_rank)
        if (c != 1).any():
            r = int(np.argmax(c != 1))
            raise BvhViolation("coverage", f"{name} rank {base + r} appears in {c[r]} records")
    # homogeneity per leaf (before the per-record comparison with the scene:
    # two whole records swapped between leaves are each right, the leaves not)
    sel = lk == 0
    tn, tsl, tf_, tc = ln[sel], ls[sel], lf[sel], lc[sel]
    for j in range(1, 4):
        m = tc > j
        bad = tgate[tf_[m] + j] != tgate[tf_[m]]
        if bad.any():
            i = np.argmax(bad)
            raise BvhViolation("gate", f"node {tn[m][i]} slot {tsl[m][i]}: leaf [{tf_[m][i]}, +{tc[m][i]}) mixes mesh gates "
                                       f"{tgate[tf_[m][i]]} and {tgate[tf_[m][i] + j]}")
    want_gate = np.full(T, -1, np.int32)
    want_gate[is_mesh] = prims.mesh_gate[trank[is_mesh]]
    if (tgate != want_gate).any():
        r = int(np.argmax(tgate != want_gate))
        raise BvhViolation("gate", f"triangle record {r} (rank {trank[r]}) has gate {tgate[r]}, the scene says {want_gate[r]}")
    if NS and (sph_i[:, 5] != -1).any():
        raise BvhViolation("gate", f"sphere record {int(np.argmax(sph_i[:, 5] != -1))} has a gate")
    verts = np.empty((T, 3, 3), np.float32)
    verts[is_mesh] = prims.mesh_tris[trank[is_mesh]]
    verts[is_loose] = prims.loose_tris[trank[is_loose] - MT - NS]
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.concatenate([verts[:, 0], verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]], 1).astype(np.float32)
    diff = _bits(tri_f[:T, :9]) != _bits(want)
    if diff.any():
        r, c = np.argwhere(diff)[0]
        raise BvhViolation("record", f"triangle record {r} (rank {trank[r]}): {('v0', 'e1', 'e2')[c // 3]}.{'xyz'[c % 3]} is "
                                     f"{tri_f[r, c]!r}, the scene gives {want[r, c]!r}")
    if NS:
        diff = _bits(sph_f[:, :4]) != _bits(prims.spheres[srank - MT])
        if diff.any():
            r, c = np.argwhere(diff)[0]
            raise BvhViolation("record", f"sphere record {r} (rank {srank[r]}): field {c} is {sph_f[r, c]!r}")

    # ---- boxes: exact, half-padded and padded unions per record, leaf, slot (float64)
    pad_abs = prims.pad_abs()
    inf = np.inf

    def rec_boxes(plo, phi, ext):
        pad = pad_abs + ext * 1e-4
        return (plo, phi, plo - 0.5 * pad[:, None], phi + 0.5 * pad[:, None], plo - pad[:, None], phi + pad[:, None])

    v64 = verts.astype(np.float64)
    tlo, thi = v64.min(1), v64.max(1)
    tri_b = rec_boxes(tlo, thi, (thi - tlo).max(1) if T else np.zeros(0))
    c64 = sph_f[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        r64 = np.sqrt(sph_f[:, 3].astype(np.float64))
    sph_b = rec_boxes(c64 - r64[:, None], c64 + r64[:, None], r64)
    # per slot: [exact lo, exact hi, half lo, half hi, padded lo, padded hi]
    U = [np.full((N, 4, 3), inf if i % 2 == 0 else -inf) for i in range(6)]
    for k, boxes in ((0, tri_b), (1, sph_b)):
        sel = lk == k
        n_, s_, f_, c_ = ln[sel], ls[sel], lf[sel], lc[sel]
        for j in range(4):
            m = c_ > j
            for i in range(6):
                op = np.minimum if i % 2 == 0 else np.maximum
                U[i][n_[m], s_[m]] = op(U[i][n_[m], s_[m]], boxes[i][f_[m] + j])
    for lev in levels[:0:-1]:  # bottom-up: a node's union becomes its parent's slot's
        for i in range(6):
            U[i][parent[lev], pslot[lev]] = U[i][lev].min(1) if i % 2 == 0 else U[i][lev].max(1)
    used = ~empty
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    finite = np.isfinite(U[4]).all(-1) & np.isfinite(U[5]).all(-1) & used
    # lower bound: containment with half the pad
    with np.errstate(invalid="ignore"):
        bad = used[..., None] & ((lo64 > U[2]) | (hi64 < U[3]))
    if bad.any():
        n, s, a = np.argwhere(bad)[0]
        raise BvhViolation("box-inside", f"node {n} slot {s} axis {a}: box [{lo[n, s, a]!r}, {hi[n, s, a]!r}] does not keep "
                                         f"half the pad around its primitives [{U[0][n, s, a]!r}, {U[1][n, s, a]!r}] "
                                         f"(needs [{U[2][n, s, a]!r}, {U[3][n, s, a]!r}])")
    # upper bound: no further out than the padded union + 2 float32 ulp
    mag = np.maximum(np.abs(lo64), np.abs(hi64)).max(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        slack = 2.0 * np.spacing(np.where(np.isfinite(mag), mag, 0.0).astype(np.float32)).astype(np.float64)
    bad = finite[..., None] & ((lo64 < U[4] - slack[..., None]) | (hi64 > U[5] + slack[..., None]))
    if bad.any():
        n, s, a = np.argwhere(bad)[0]
        raise BvhViolation("box-outside", f"node {n} slot {s} axis {a}: box [{lo[n, s, a]!r}, {hi[n, s, a]!r}] lies outside "
                                          f"the padded primitives [{U[4][n, s, a]!r}, {U[5][n, s, a]!r}] + {slack[n, s]!r}")
    with np.errstate(invalid="ignore"):
        margin = np.minimum(U[0] - lo64, hi64 - U[1])[finite]

    # ---- depth
    if 3 * (depth4 + 1) > stack_total:
        raise BvhViolation("depth", f"4-wide depth {depth4} needs {3 * (depth4 + 1)} stack entries, the traversal has {stack_total}")
    return {"depth4": depth4, "nodes": N, "leaves": int(len(ln)), "largest_leaf": int(lc.max()) if len(lc) else 0,
            "min_margin": float(margin.min()) if margin.size else float("inf"), "pad_abs": pad_abs,
            "empty_slots": int(empty.sum())}
