"""Scenes shared by the GPU tests (test_gpu_lbvh.py, test_gpu_cut.py,
test_gpu_bvh_invariants.py)."""
import numpy as np


def degenerate_scenes(rt, fr0):
    """Morton-code collisions (identical centroids), a single primitive, a
    one-triangle mesh, zero-area triangles, a huge-coordinate scene; lit like
    the frame fr0."""
    S = rt.Scene
    mats = fr0.scene.SphereData.Materials
    scenes = []
    # 300 identical spheres plus 200 identical triangles: every key collides
    a = S()
    for i in range(300):
        a.add_sphere_r2((0.1, -0.2, 0.3), 0.2, mats[i % 2])
    tri = np.array([[[-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.5, 0.5]]], np.float32)
    a.add_triangles(np.repeat(tri, 200, 0), [mats[1]] * 200)
    scenes.append(a)
    # single sphere; single loose triangle; one mesh with one triangle
    b = S()
    b.add_sphere_r2((0.0, 0.0, 0.0), 0.25, mats[1])
    scenes.append(b)
    c = S()
    c.add_triangles(tri, [mats[1]])
    scenes.append(c)
    d = S()
    d.add_mesh(rt.Mesh.from_vertices(tri.reshape(-1, 3), [0, 1, 2], mats[1]))
    scenes.append(d)
    # zero-area triangles among normal ones
    e = S()
    z = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
                  [[-0.3, 0.0, 0.2], [0.3, 0.0, 0.2], [0.6, 0.0, 0.2]]], np.float32)
    e.add_triangles(np.concatenate([z, tri]), [mats[0]] * 3)
    scenes.append(e)
    # big coordinates: a far plane of spheres
    f = S()
    for i in range(64):
        f.add_sphere_r2((1.0e4 * (i % 8 - 3.5), 1.0e4 * (i // 8 - 3.5), 5.0e4), 1.0e7, mats[i % 2])
    scenes.append(f)
    for sc in scenes:
        sc.PointLights = fr0.scene.PointLights
        sc.AmbientLight = fr0.scene.AmbientLight
    return scenes


def translated(rt, fr, off):
    """The frame with every position moved by `off` (float32 adds, the camera
    too): the same picture far from the origin."""
    import copy

    o = np.asarray(off, np.float32)
    sc = copy.deepcopy(fr.scene)
    td = sc.TriangleData
    if len(td.Triangles):
        td.Triangles = (td.Triangles + o).astype(np.float32)
    for m in sc.Meshes:
        m.Triangles = (m.Triangles + o).astype(np.float32)
        m.AABB = (m.AABB + o).astype(np.float32)
    if len(sc.SphereData.Spheres):
        sc.SphereData.Spheres[:, :3] = (sc.SphereData.Spheres[:, :3] + o).astype(np.float32)
    if len(sc.PointLights):
        sc.PointLights[:, :3] = (sc.PointLights[:, :3] + o).astype(np.float32)
    cam = fr.camera.__class__(**{**fr.camera.__dict__,
                                 "Position": tuple((np.asarray(fr.camera.Position, np.float32) + o).tolist())})
    return fr.with_(scene=sc, camera=cam)
