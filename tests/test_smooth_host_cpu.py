"""The host side of smooth shading (jadehost::vertex_normals, SceneBuilder::set_smoothing, BuiltScene::vertex_normals; host.vertex_normals,
SceneBuilder.set_smoothing, HostScene.vertex_normals): the normals against a numpy restatement, the crease rule, and the table following
its triangles through the SAH sort and through build_with_bvh.  No GPU."""
import numpy as np

import jaderaytracerendering_amd as J
import spec_scenes as SP
from jaderaytracerendering_amd import host as H

F32 = np.float32


def restated(vertices, indices, crease_deg):
    """host.vertex_normals in numpy: flat normals in fp32 as add_mesh forms them are taken from the library at crease 0 (the statement
    starts from them); per corner the angle-weighted sum in float64 over the triangles that share the vertex index and whose flat normal
    is within the crease; the flat normal itself where nothing else contributes or every contributor's equals this one's."""
    v = np.asarray(vertices, F32).astype(np.float64)
    idx = np.asarray(indices, np.int32)
    flat32 = H.vertex_normals(vertices, indices, 0.0)[:, 0]
    flat = flat32.astype(np.float64)
    cosc = np.cos(np.deg2rad(float(crease_deg)))
    out = np.zeros((len(idx), 3, 3))
    users = {}
    for i, tri in enumerate(idx):
        for k in range(3):
            users.setdefault(int(tri[k]), []).append((i, k))

    def angle(i, k):
        o, a, b = v[idx[i][k]], v[idx[i][(k + 1) % 3]], v[idx[i][(k + 2) % 3]]
        c = np.cross(a - o, b - o)
        return np.arctan2(np.sqrt(c @ c), (a - o) @ (b - o))

    for i, tri in enumerate(idx):
        for k in range(3):
            s, others, same = np.zeros(3), 0, True
            for j, kj in users[int(tri[k])]:
                if j != i and not flat[i] @ flat[j] >= cosc:
                    continue
                others += j != i
                same = same and bool((flat32[j] == flat32[i]).all())
                s = s + angle(j, kj) * flat[j]
            ln = np.sqrt(s @ s)
            out[i, k] = flat[i] if (others == 0 or same or not ln > 0) else s / ln
    return out


def geodesic():
    """make_geodesic(2)'s 80 triangles with shared vertices, recovered from the builder's triangles (positions are exact copies)."""
    b = J.SceneBuilder()
    b.add_proc("geodesic", 2, H.material())
    t = b.triangles_original().view(F32).reshape(-1, 28)
    corners = t[:, 1:10].reshape(-1, 3)
    verts, inv = np.unique(corners.view(np.dtype((np.void, 12))), return_inverse=True)
    return verts.view(F32).reshape(-1, 3), inv.reshape(-1, 3).astype(np.int32)


def test_vertex_normals_are_the_restatement_within_one_rounding():
    v, i = geodesic()
    assert len(i) == 80 and len(v) == 42
    for crease in (25.0, 60.0, 180.0):
        got = H.vertex_normals(v, i, crease)
        assert got.dtype == F32 and got.shape == (80, 3, 3)
        assert np.abs(got.astype(np.float64) - restated(v, i, crease)).max() <= 1e-6, crease
    rng = np.random.default_rng(5)
    v2 = (v + 0.15 * rng.normal(size=v.shape)).astype(F32)          # a lumpy ball: the crease cuts some neighbours and keeps others
    for crease in (20.0, 45.0):
        got, want = H.vertex_normals(v2, i, crease), restated(v2, i, crease)
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-6, crease
    flat = H.vertex_normals(v2, i, 0.0)
    cut = (np.abs(H.vertex_normals(v2, i, 20.0) - flat).max((1, 2)) == 0).sum()
    assert 0 < cut < 80 or (H.vertex_normals(v2, i, 20.0) != H.vertex_normals(v2, i, 45.0)).any(), "the crease angle decides something on this mesh"


def test_crease_zero_is_the_flat_normal_thrice_bitwise():
    v, i = geodesic()
    got = H.vertex_normals(v, i, 0.0)
    b = J.SceneBuilder()
    b.add_mesh(v, i, H.material())
    norm = b.triangles_original().view(F32).reshape(-1, 28)[:, 10:13]
    for k in range(3):
        assert np.array_equal(got[:, k].view(np.uint32), norm.view(np.uint32))
    assert np.array_equal(H.vertex_normals(v, i, -5.0).view(np.uint32), got.view(np.uint32))


def test_a_cube_at_crease_30_is_flat():
    got = H.vertex_normals(SP.CUBE_V, SP.CUBE_I, 30.0)
    flat = H.vertex_normals(SP.CUBE_V, SP.CUBE_I, 0.0)
    assert np.array_equal(got.view(np.uint32), flat.view(np.uint32)), "faces meet at 90 degrees, and a face's two triangles share one normal"
    assert (np.abs(flat) == 1).sum() == 12 * 3                      # axis-aligned: exact
    round_ = H.vertex_normals(SP.CUBE_V, SP.CUBE_I, 95.0)
    assert np.abs(round_ - flat).max() > 0.2, "at 95 degrees the corners are rounded"


def test_at_crease_180_a_vertex_has_one_normal_in_every_triangle():
    v, i = geodesic()
    got = H.vertex_normals(v, i, 180.0).astype(np.float64)
    for vert in range(len(v)):
        mine = got[i == vert]
        assert len(mine) >= 5 and np.abs(mine - mine[0]).max() <= 1e-5
        assert abs(mine[0] @ v[vert]) / np.sqrt(v[vert] @ v[vert]) > 0.9995, "along the sphere's own normal (the mesh's winding gives its sign)"
    assert np.abs(np.sqrt((got * got).sum(-1)) - 1).max() <= 1e-6


def smoothed_scene():
    b = J.SceneBuilder()
    b.add_mesh(SP.quad(-0.9, 3.0), SP.QUAD_I, H.material(**SP.FLOOR))         # flat, before any smoothing
    b.set_smoothing(180.0)
    b.add_proc("geodesic", 2, H.material(**SP.JADE), H.transform_matrix(rot_deg=(20, 30, 0), trans=(0.2, 0.1, -0.3), scale=(0.7, 0.5, 0.6)))
    b.set_smoothing(0.0)
    b.add_mesh(SP.quad(1.5, 0.5, flip=True), SP.QUAD_I, H.material(**SP.LIGHT))
    return b


def test_the_table_follows_the_triangles_through_build_and_build_with_bvh():
    b = smoothed_scene()
    orig = b.triangles_original().view(F32).reshape(-1, 28)
    hs = b.build()
    assert hs.vertex_normals is not None and hs.vertex_normals.shape == (84, 3, 3)
    t = hs.tri_f32()
    ball = hs.tri_i32()[:, 0] == 1
    assert ball.sum() == 80
    # flat meshes: the flat normal thrice, bitwise - added before and after the smoothed one
    for k in range(3):
        assert np.array_equal(hs.vertex_normals[~ball, k].view(np.uint32), t[~ball, 10:13].view(np.uint32))
    # the ball: formed AFTER the transform - host.vertex_normals on the transformed corners, triangle by triangle in BVH order
    corners = t[ball, 1:10].reshape(-1, 3)
    verts, inv = np.unique(corners.view(np.dtype((np.void, 12))), return_inverse=True)
    want = H.vertex_normals(verts.view(F32).reshape(-1, 3), inv.reshape(-1, 3).astype(np.int32), 180.0)
    assert np.array_equal(hs.vertex_normals[ball].view(np.uint32), want.view(np.uint32))
    assert (np.abs(hs.vertex_normals[ball] - t[ball, None, 10:13]).max((1, 2)) > 1e-3).all(), "and they are not the flat normals"
    # build_with_bvh with the SAH build's own order reversed inside every... any permutation: the rows travel with their triangles
    order = np.array([int(np.flatnonzero((orig[:, 1:10] == t[i, 1:10]).all(1))[0]) for i in range(len(t))], np.int32)
    again = b.build_with_bvh(order, hs.a["nodes"])
    assert np.array_equal(again.tri_f32().view(np.uint32), t.view(np.uint32))
    assert np.array_equal(again.vertex_normals.view(np.uint32), hs.vertex_normals.view(np.uint32))


def test_nothing_smoothed_nothing_carried_and_npz_round_trip(tmp_path):
    assert SP.build("jade_cube").vertex_normals is None
    hs = smoothed_scene().build()
    hs.save_npz(tmp_path / "s.npz")
    back = H.HostScene.from_npz(tmp_path / "s.npz")
    assert np.array_equal(back.vertex_normals.view(np.uint32), hs.vertex_normals.view(np.uint32))
    SP.build("jade_cube").save_npz(tmp_path / "f.npz")
    assert H.HostScene.from_npz(tmp_path / "f.npz").vertex_normals is None
