"""The host side of normal maps (libjade_host.so, jaderaytracerendering_amd/host.py): load_normal_map - a P6 file read linearly as 2 c - 1,
a PF file as given -, height_to_normal_map - a constant gives (0, 0, 1) exactly, a ramp a constant tilt, the borders wrap -, the
builder's table carried with the triangles through the SAH sort and through build_with_bvh, independent of the albedo table's, and the
command line's refusals.  No GPU."""
import subprocess

import numpy as np
import pytest

import jaderaytracerendering_amd as J
import spec_scenes as SP
from conftest import ORACLE_LIB
from jaderaytracerendering_amd import host as H
from render_helpers import CLI

F32 = np.float32


def test_load_normal_map_reads_a_ppm_linearly_and_a_pfm_as_given(tmp_path):
    rng = np.random.default_rng(41)
    img = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    img[0, 0] = (0, 255, 128)
    (tmp_path / "n.ppm").write_bytes(b"P6\n# a comment\n7 5\n255\n" + img.tobytes())
    got = H.load_normal_map(tmp_path / "n.ppm")
    want = (2.0 * (img.astype(np.float64) / 255.0) - 1.0).astype(F32)
    assert got.shape == (5, 7, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), "2 c - 1 in double, rounded once"
    assert got[0, 0, 0] == -1 and got[0, 0, 1] == 1 and abs(got[0, 0, 2] - 1 / 255) < 1e-7
    srgb = H.load_texture(tmp_path / "n.ppm")
    assert not np.allclose(2 * srgb - 1, got, atol=0.05), "... and not the sRGB decode an albedo image gets"
    vec = rng.uniform(-2, 2, (3, 4, 3)).astype(F32)
    (tmp_path / "n.pfm").write_bytes(b"PF\n4 3\n-1.0\n" + vec[::-1].astype("<f4").tobytes())
    assert np.array_equal(H.load_normal_map(tmp_path / "n.pfm").view(np.uint32), vec.view(np.uint32)), "a PF file as given, its rows flipped to top first"
    with pytest.raises(RuntimeError, match="open failed"):
        H.load_normal_map(tmp_path / "none.ppm")
    (tmp_path / "bad.ppm").write_bytes(b"P5\n2 2\n255\n0000")
    with pytest.raises(RuntimeError, match="not a P6"):
        H.load_normal_map(tmp_path / "bad.ppm")


def test_height_to_normal_map():
    flat = H.height_to_normal_map(np.full((6, 9), 0.375, F32), 3.0)
    assert flat.shape == (6, 9, 3)
    assert np.array_equal(flat.view(np.uint32), np.broadcast_to(np.array([0, 0, 1], F32), (6, 9, 3)).view(np.uint32)), "a constant: (+0, +0, 1) in every bit"
    # a ramp in u: height = i / 8 on 8 x 4 texels - dh/du = (2 / 8) * (8 / 2) = 1 inside, and the border columns see the wrap
    Hh, W = 4, 8
    ramp = np.broadcast_to(np.arange(W, dtype=F32) / 8, (Hh, W)).copy()
    m = H.height_to_normal_map(ramp, 0.5)
    assert (m[:, 1:-1, 0] == -0.5).all() and (m[..., 1] == 0).all() and (m[..., 2] == 1).all(), "a constant tilt inside"
    assert (m[:, 0, 0] == -0.5 * ((1 / 8 - 7 / 8) * 4)).all() and (m[:, -1, 0] == -0.5 * ((0 - 6 / 8) * 4)).all(), "the borders wrap"
    # any field: the stated differences, bit for bit
    rng = np.random.default_rng(42)
    h = rng.uniform(-1, 1, (5, 7)).astype(F32)
    s = F32(0.75)
    du = (np.roll(h, -1, 1) - np.roll(h, 1, 1)) * F32(0.5 * 7)
    dv = (np.roll(h, -1, 0) - np.roll(h, 1, 0)) * F32(0.5 * 5)
    want = np.stack([F32(0) - s * du, F32(0) - s * dv, np.ones_like(h)], -1).astype(F32)
    assert np.array_equal(H.height_to_normal_map(h, 0.75).view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        H.height_to_normal_map(np.zeros((2, 2, 3), F32))


def mapped_scene():
    """A floor without a map, a quad with map 0 (its own UVs) and an albedo texture, a ball with map 1 (spherical UVs), a cube with map 1
    again through add_mesh's uvs, a light without."""
    rng = np.random.default_rng(43)
    a, b_ = rng.uniform(-1, 1, (4, 4, 3)).astype(F32), rng.uniform(-1, 1, (8, 2, 3)).astype(F32)
    uv_own = rng.uniform(-1, 2, (12, 3, 2)).astype(F32)
    b = J.SceneBuilder()
    b.add_mesh(SP.quad(-0.9, 3.0), SP.QUAD_I, H.material(**SP.FLOOR))
    b.set_normal_map(a, strength=0.5)
    b.set_texture(H.texture_checker(4, 2))
    b.add_proc("quad", 0, H.material())
    b.set_texture(None)
    b.set_normal_map(b_, H.UV_SPHERICAL, strength=1.5)
    b.add_proc("geodesic", 2, H.material(), H.transform_matrix(scale=(0.5, 0.5, 0.5)))
    b.add_mesh(SP.CUBE_V, SP.CUBE_I, H.material(), uvs=uv_own)
    b.set_normal_map(None)
    b.add_mesh(SP.quad(1.5, 0.5, flip=True), SP.QUAD_I, H.material(**SP.LIGHT))
    return b, (a, b_), uv_own


def test_the_table_follows_the_triangles_through_build_and_build_with_bvh():
    b, images, uv_own = mapped_scene()
    orig = b.triangles_original().view(F32).reshape(-1, 28)
    hs = b.build()
    got_images, uv, image_of, strength = hs.normal_maps
    n = hs.n_triangles
    assert n == 2 + 2 + 80 + 12 + 2 and uv.shape == (n, 3, 2) and image_of.shape == (n,)
    assert strength == 1.5, "one strength for the table: the last given"
    assert len(got_images) == 2 and all(np.array_equal(g, w) for g, w in zip(got_images, images))
    t, obj = hs.tri_f32(), hs.tri_i32()[:, 0]
    order = np.array([int(np.flatnonzero((orig[:, 1:10] == t[i, 1:10]).all(1))[0]) for i in range(n)], np.int32)   # BVH position -> original index
    assert not np.array_equal(order, np.arange(n)), "the SAH sort moved the triangles"
    want_image = np.concatenate([[-1] * 2, [0] * 2, [1] * 80, [1] * 12, [-1] * 2])
    assert np.array_equal(image_of, want_image[order])
    assert (uv[image_of < 0] == 0).all()
    quad_uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], F32)
    assert np.array_equal(uv[obj == 1], quad_uv[order[obj == 1] - 2]), "make_quad's own UVs"
    assert np.array_equal(uv[obj == 3], uv_own[order[obj == 3] - 84]), "add_mesh's uvs"
    ball = J.SceneBuilder()
    ball.add_proc("geodesic", 2, H.material())
    p = ball.triangles_original().view(F32).reshape(-1, 28)[:, 1:10]
    want = H.project_uvs(p.reshape(-1, 3), np.arange(240).reshape(-1, 3), H.UV_SPHERICAL)
    assert np.array_equal(uv[obj == 2].view(np.uint32), want[order[obj == 2] - 4].view(np.uint32))
    # the albedo table is its own: the quad alone names an image there
    assert hs.textures is not None and np.array_equal(hs.textures[2] >= 0, obj == 1)
    # build_with_bvh: the rows travel with their triangles by their original index
    again = b.build_with_bvh(order, hs.a["nodes"])
    assert np.array_equal(again.tri_f32().view(np.uint32), t.view(np.uint32))
    assert np.array_equal(again.normal_maps[1].view(np.uint32), uv.view(np.uint32)) and np.array_equal(again.normal_maps[2], image_of)
    assert all(np.array_equal(g, w) for g, w in zip(again.normal_maps[0], images)) and again.normal_maps[3] == 1.5


def test_nothing_mapped_nothing_carried_and_the_builder_refuses_a_bad_strength(tmp_path):
    assert SP.build("jade_cube").normal_maps is None
    hs = mapped_scene()[0].build()
    hs.save_npz(tmp_path / "m.npz")
    back = H.HostScene.from_npz(tmp_path / "m.npz")
    assert len(back.normal_maps[0]) == 2 and all(np.array_equal(a, b) for a, b in zip(back.normal_maps[0], hs.normal_maps[0]))
    assert np.array_equal(back.normal_maps[1].view(np.uint32), hs.normal_maps[1].view(np.uint32)) and np.array_equal(back.normal_maps[2], hs.normal_maps[2])
    assert back.normal_maps[3] == hs.normal_maps[3] and back.textures is not None
    SP.build("jade_cube").save_npz(tmp_path / "f.npz")
    assert H.HostScene.from_npz(tmp_path / "f.npz").normal_maps is None
    b = J.SceneBuilder()
    b.set_normal_map(np.zeros((2, 2, 3), F32))
    b.set_normal_map(None)
    b.add_mesh(SP.CUBE_V, SP.CUBE_I, H.material())
    assert b.build().normal_maps is None
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="strength"):
            b.set_normal_map(np.zeros((2, 2, 3), F32), strength=bad)
        with pytest.raises(RuntimeError, match="strength"):
            b.set_object_normal_map(0, np.zeros((2, 2, 3), F32), strength=bad)
    b = J.SceneBuilder()
    b.set_object_normal_map(2, np.ones((2, 2, 3), F32), H.UV_PLANAR_Y, 0.25)
    b.config("tiny")
    hs = b.build()
    assert hs.normal_maps is not None and hs.normal_maps[3] == 0.25 and set(hs.normal_maps[2].tolist()) == {-1, 0}
    assert np.array_equal(hs.normal_maps[2] >= 0, hs.tri_i32()[:, 0] == 2)


def test_the_command_lines_refusals(tmp_path):
    common = [CLI, "--config", "tiny", "--width", "16", "--height", "16", "--spp", "1", "--out", "x.pfm"]
    for bad, code, words in ((["--normal-map", "bumps"], 2, "K=IMAGE"), (["--normal-map", "99=bumps"], 2, "objects 0 .. 5"),
                             (["--normal-map", "0=bumps@sideways"], 2, "projection"), (["--normal-map", "0=none.ppm"], 1, "open failed"),
                             (["--normal-map", "0=bumps:64:4:-2"], 2, "strength"), (["--normal-map", "0=bumps@planar-y:x"], 2, "strength"),
                             (["--normal-map", "0=bumps:8:8"], 2, "half as many bumps"),
                             (["--normal-map", "0=bumps", "--normal-map", "0=bumps"], 2, "twice")):
        r = subprocess.run(common + bad, capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == code and words in r.stderr, (bad, r.returncode, r.stderr)
    orc = subprocess.run(common + ["--normal-map", "0=bumps:64:4@planar-y:0.5", "--backend", ORACLE_LIB], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert orc.returncode == 2 and "--normal-map needs the HIP backend" in orc.stderr


OBJ = """# a quad with texture coordinates, and a triangle without
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 2 2 2
vt 0.25 0.5
vt 0.75 0.5
vt 0.75 1.0
vt 0.25 1.0
f 1/1 2/2 3/3
f 1/1 3/3 4/4
f 3 4 5
"""


@pytest.mark.parametrize("how", ("set_normal_map", "set_object_normal_map"))
def test_an_obj_added_under_a_normal_map_alone_carries_its_own_uvs(tmp_path, how):
    """An authored normal map is tied to the mesh's UV layout: with a map set - the builder's or the object's own - and no albedo texture,
    add_obj reads the file's vt lines, and they, not the projection's, are the map's UVs."""
    path = tmp_path / "q.obj"
    path.write_text(OBJ)
    v, i, uv_file = H.load_obj_textured(path)
    image = np.ones((2, 2, 3), F32)
    b = J.SceneBuilder()
    if how == "set_normal_map":
        b.set_normal_map(image, H.UV_PLANAR_Z)
    else:
        b.set_object_normal_map(0, image, H.UV_PLANAR_Z)
    b.add_obj(path, H.material())
    orig = b.triangles_original().view(F32).reshape(-1, 28)
    assert np.array_equal(orig[:, 1:10], v[i].reshape(-1, 9)), "read with its vt lines: the corners are the file's"
    hs = b.build()
    assert hs.textures is None and hs.normal_maps is not None
    t = hs.tri_f32()
    order = np.array([int(np.flatnonzero((orig[:, 1:10] == t[k, 1:10]).all(1))[0]) for k in range(hs.n_triangles)])
    assert np.array_equal(hs.normal_maps[1], uv_file[order]) and (hs.normal_maps[2] == 0).all()
    assert not np.array_equal(hs.normal_maps[1], H.project_uvs(v, i, H.UV_PLANAR_Z)[order]), "... and not the projection's"
