"""A CPU restatement of the device LBVH build (csrc/lbvh.hip) for small
scenes, in the export format of rt_export_bvh: the two-level sort keys
(30-bit Morton code of the centroid in the scene box | mesh id + 1 | in-mesh
Morton code), a stable sort, Karras' splits (ties by index), boxes bottom-up,
the small-subtree leaves of k_small, and the 4-wide collapse of expand4
(largest surface area among the internal, not-small children first, first on
ties).  Plain Python per node: for scenes of hundreds of primitives.

It exists so that the depth of a scene's device tree — 2-wide and 4-wide —
can be worked out and asserted without a GPU (tests/test_bvh_invariants.py)
and compared with what the device built (tests/test_gpu_deep_tree.py).  It
does not claim the device's node numbering."""
import numpy as np

import bvh_invariants as bi

f32 = np.float32


def expand_bits(v):
    v = np.asarray(v, np.uint64)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton(c, lo, hi, bits):
    cells = f32(1 << bits)
    q = []
    for a in range(3):
        ext = f32(hi[a] - lo[a])
        t = ((c[:, a] - lo[a]) / ext).astype(f32) if ext > 0 else np.full(len(c), 0.5, f32)
        t = np.clip(t, 0, 1).astype(f32)
        q.append(np.minimum((t * cells).astype(f32), cells - 1).astype(np.uint64))
    return (expand_bits(q[0]) << np.uint64(2)) | (expand_bits(q[1]) << np.uint64(1)) | expand_bits(q[2])


def build(scene):
    """-> ((nodes, tris, sphs) byte arrays, {"depth2", "depth4", "nodes4"})"""
    P = bi.Prims.of_scene(scene)
    MT, NS, NL = P.mt, P.ns, P.nl
    n = MT + NS + NL
    pad_abs = f32(P.pad_abs())
    # scene box
    lo = np.full(3, np.finfo(f32).max, f32)
    hi = -lo
    if len(P.gates):
        lo = np.minimum(lo, P.gates[:, 0].min(0))
        hi = np.maximum(hi, P.gates[:, 1].max(0))
    if NL:
        v = P.loose_tris.reshape(-1, 3)
        lo = np.minimum(lo, v.min(0))
        hi = np.maximum(hi, v.max(0))
    if NS:
        r = np.sqrt(P.spheres[:, 3]).astype(f32)[:, None]
        lo = np.minimum(lo, (P.spheres[:, :3] - r).min(0))
        hi = np.maximum(hi, (P.spheres[:, :3] + r).max(0))
    plo = np.zeros((n, 3), f32)
    phi = np.zeros((n, 3), f32)
    cen = np.zeros((n, 3), f32)
    gate = np.full(n, -1, np.int64)
    tris_all = np.concatenate([P.mesh_tris, np.zeros((NS, 3, 3), f32), P.loose_tris])
    for sl in (slice(0, MT), slice(MT + NS, n)):
        t = tris_all[sl]
        if len(t) == 0:
            continue
        l, h = t.min(1), t.max(1)
        pad = (pad_abs + ((h - l).max(1) * f32(1e-4)).astype(f32)).astype(f32)[:, None]
        cen[sl] = (f32(0.5) * (l + h)).astype(f32)
        plo[sl] = l - pad
        phi[sl] = h + pad
    gate[:MT] = P.mesh_gate
    if NS:
        r = np.sqrt(P.spheres[:, 3]).astype(f32)[:, None]
        pad = (pad_abs + (r * f32(1e-4)).astype(f32)).astype(f32)
        c = P.spheres[:, :3]
        cen[MT:MT + NS] = c
        plo[MT:MT + NS] = (c - r).astype(f32) - pad
        phi[MT:MT + NS] = (c + r).astype(f32) + pad
    keys = morton(cen, lo, hi, 10) << np.uint64(34)
    M = len(P.gates)
    if M:
        mesh_bits = 0
        while (1 << mesh_bits) <= M:
            mesh_bits += 1
        low_bits = 34 - mesh_bits
        per_axis = 10 if low_bits >= 30 else low_bits // 3
        mc = (f32(0.5) * (P.gates[:, 0] + P.gates[:, 1])).astype(f32)
        top = morton(mc, lo, hi, 10)
        for m in range(M):
            sel = np.nonzero(P.mesh_gate == m)[0]
            low = morton(cen[sel], P.gates[m, 0], P.gates[m, 1], per_axis) if per_axis > 0 else 0
            keys[sel] = (top[m] << np.uint64(34)) | (np.uint64(m + 1) << np.uint64(low_bits)) | low
    order = np.argsort(keys, kind="stable")
    k = keys[order]
    slo, shi = plo[order], phi[order]
    is_sph = (order >= MT) & (order < MT + NS)
    sph_idx = np.cumsum(is_sph) - is_sph  # exclusive
    gate_pos = np.where(is_sph, -2, gate[order])
    leaf_ref = [bi.leaf_ref(sph_idx[i], 1, 1) if is_sph[i] else bi.leaf_ref(i - sph_idx[i], 1, 0) for i in range(n)]
    # records
    tri_ranks = [int(order[i]) for i in range(n) if not is_sph[i]]
    sph_ranks = [int(order[i]) for i in range(n) if is_sph[i]]
    tri = np.zeros((len(tri_ranks) + 1, 12), f32)
    ti = tri.view(np.int32)
    for j, r in enumerate(tri_ranks):
        t = tris_all[r]
        tri[j, :9] = np.concatenate([t[0], t[1] - t[0], t[2] - t[0]])
        ti[j, 9], ti[j, 10] = r, gate[r]
    ti[-1, 9], ti[-1, 10] = 0x7fffffff, -1
    sph = np.zeros((len(sph_ranks), 8), f32)
    for j, r in enumerate(sph_ranks):
        sph[j, :4] = P.spheres[r - MT]
        sph.view(np.int32)[j, 4:6] = r, -1
    # Karras top-down
    nodes = {}  # idx -> dict(first,last,children refs (idx or ('L',pos)), boxes)

    def split(a, b):
        if k[a] == k[b]:
            hb = (a ^ b).bit_length() - 1
            return (b & ~((1 << hb) - 1)) - 1
        x = int(k[a]) ^ int(k[b])
        hb = x.bit_length() - 1
        mask = np.uint64(1 << hb)
        # last index in [a,b] with bit hb == 0
        seg = (k[a:b + 1] & mask) != 0
        return a + int(np.argmax(seg)) - 1

    depth2 = [0]

    def mk(a, b, idx, d):
        g = split(a, b)
        depth2[0] = max(depth2[0], d + 1)
        nd = {"first": a, "last": b}
        ch = []
        for (x, y, ci) in ((a, g, g), (g + 1, b, g + 1)):
            if x == y:
                ch.append((("L", x), slo[x], shi[x]))
            else:
                mk(x, y, ci, d + 1)
                c = nodes[ci]
                ch.append((ci, np.minimum(c["ch"][0][1], c["ch"][1][1]), np.maximum(c["ch"][0][2], c["ch"][1][2])))
        nd["ch"] = ch
        nodes[idx] = nd

    if n == 1:
        raise NotImplementedError("a lone primitive: nothing to measure")
    mk(0, n - 1, 0, 0)

    def harea(l, h):
        d = (h - l).astype(f32)
        return f32(f32(f32(d[0] * d[1]) + f32(d[1] * d[2])) + f32(d[2] * d[0]))

    small = {}
    for i, nd in nodes.items():
        cnt = nd["last"] - nd["first"] + 1
        ok = i != 0 and cnt <= 4 and len(set(gate_pos[nd["first"]:nd["last"] + 1])) == 1
        if ok and cnt > 1:
            (r0, l0, h0), (r1, l1, h1) = nd["ch"]
            c0 = 1 if isinstance(r0, tuple) else nodes[r0]["last"] - nodes[r0]["first"] + 1
            ap = max(harea(np.minimum(l0, l1), np.maximum(h0, h1)), f32(1e-30))
            ok = f32(cnt) <= f32(1.0) + (harea(l0, h0) * f32(c0) + harea(l1, h1) * f32(cnt - c0)) / ap
        small[i] = bool(ok)

    def expand4(i):
        S = [list(c) for c in nodes[i]["ch"]]
        while len(S) < 4:
            best, best_a = -1, f32(-1)
            for s, (ref, l, h) in enumerate(S):
                if isinstance(ref, tuple) or small[ref]:
                    continue
                ar = harea(l, h)
                if ar > best_a:
                    best_a, best = ar, s
            if best < 0:
                break
            c = nodes[S[best][0]]["ch"]
            S[best] = list(c[0])
            S.append(list(c[1]))
        return S

    keep = {0}
    depth4 = [0]
    stackq = [(0, 0)]
    slots_of = {}
    while stackq:
        i, d = stackq.pop()
        depth4[0] = max(depth4[0], d)
        S = expand4(i)
        slots_of[i] = S
        for ref, l, h in S:
            if not isinstance(ref, tuple) and not small[ref]:
                keep.add(ref)
                stackq.append((ref, d + 1))
    idx4 = {x: j for j, x in enumerate(sorted(keep))}
    w = np.full((len(keep), 32), np.inf, f32)
    wi = w.view(np.int32)
    wi[:, 24:28] = bi.leaf_ref(len(tri_ranks), 1, 0)
    wi[:, 28:32] = 0
    for i in keep:
        for s, (ref, l, h) in enumerate(slots_of[i]):
            for a in range(3):
                w[idx4[i], 8 * a + s], w[idx4[i], 8 * a + 4 + s] = l[a], h[a]
            if isinstance(ref, tuple):
                r = leaf_ref[ref[1]]
            elif small[ref]:
                f = nodes[ref]["first"]
                c = nodes[ref]["last"] - f + 1
                r = bi.leaf_ref(sph_idx[f], c, 1) if is_sph[f] else bi.leaf_ref(f - sph_idx[f], c, 0)
            else:
                r = idx4[ref]
            wi[idx4[i], 24 + s] = r
    return (w.view(np.uint8).reshape(-1), tri.view(np.uint8).reshape(-1), sph.view(np.uint8).reshape(-1)), \
        {"depth2": depth2[0], "depth4": depth4[0], "nodes4": len(keep)}
