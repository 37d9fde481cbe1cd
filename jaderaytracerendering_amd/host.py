"""Python face of the host scene pipeline (libjade_host.so, C++).

Roles of PathTrace.cu:355-628, 1487-1612 and PathTrace.cpp:343-359, 684-687:
mesh loading / procedural stand-ins, SAH BVH, flattening, camera.  The heavy
lifting is native; this module only marshals.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
_host = None


def host_lib():
    global _host
    if _host is None:
        path = os.path.join(_LIBDIR, "libjade_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make host` (or __graft_entry__.build())")
        _host = _abi.bind(C.CDLL(path), _abi.HOST_SYMBOLS)
    return _host


def _check(rc):
    if rc != 0:
        raise RuntimeError(host_lib().jadeh_last_error().decode())


def material(emissive=(0, 0, 0), brdf=(0.8, 0.8, 0.8), reflex_mode=_abi.DIFFUSE, refract_mode=_abi.NO_REFRACT,
             refract_rate=(0.8, 0.8, 0.8), refract_albedo=(0.8, 0.8, 0.8), refract_index=1.0):
    m = _abi.Material()
    m.emissive[:] = emissive
    m.brdf[:] = brdf
    m.reflex_mode = reflex_mode
    m.refract_mode = refract_mode
    m.refract_rate[:] = refract_rate
    m.refract_albedo[:] = refract_albedo
    m.refract_index = refract_index
    return m


def jade_material():
    """The reference's jade: PathTrace.cpp:981-989."""
    return material(brdf=(0.02,) * 3, reflex_mode=_abi.MIRROR, refract_mode=_abi.SUB_SURFACE, refract_rate=(0.1,) * 3,
                    refract_albedo=(0.3,) * 3, refract_index=2.66)


def transform_matrix(rot_deg=(0, 0, 0), trans=(0, 0, 0), scale=(1, 1, 1)):
    """getTransformMatrix (PathTrace.cpp:343-359): T * Rx * Ry * Rz * S, [col][row] order."""
    out = np.zeros(16, np.float32)
    r, t, s = (np.asarray(v, np.float32) for v in (rot_deg, trans, scale))
    host_lib().jadeh_transform_matrix(r.ctypes.data, t.ctypes.data, s.ctypes.data, out.ctypes.data)
    return out


def camera_orbit(r=4.0, up_deg=0.0, rot_deg=0.0, center=(0, 0, 0)):
    """(eye[3], camera[16]) as the GL host computes them (PathTrace.cpp:684-687)."""
    eye = np.zeros(3, np.float32)
    cam = np.zeros(16, np.float32)
    c = np.asarray(center, np.float32)
    host_lib().jadeh_camera_orbit(r, up_deg, rot_deg, c.ctypes.data, eye.ctypes.data, cam.ctypes.data)
    return eye, cam


def camera_move(eye, cam, truck=None, orbit_deg=0.0, pivot=None):
    """jadeh_camera_move: (eye[3], camera[16]) after a truck (a translation in camera space) and then a rotation by `orbit_deg` about the
    axis through `pivot` parallel to the camera's up column (pivot None: the eye, a pan) - a second pose for Scene.set_shutter."""
    e = np.ascontiguousarray(eye, np.float32)
    m = np.ascontiguousarray(cam, np.float32)
    t = None if truck is None else np.ascontiguousarray(truck, np.float32)
    c = None if pivot is None else np.ascontiguousarray(pivot, np.float32)
    assert e.shape == (3,) and m.shape == (16,) and (t is None or t.shape == (3,)) and (c is None or c.shape == (3,))
    eye_out = np.zeros(3, np.float32)
    cam_out = np.zeros(16, np.float32)
    lib = host_lib()
    if lib.jadeh_camera_move(e.ctypes.data, m.ctypes.data, None if t is None else t.ctypes.data, float(orbit_deg),
                             None if c is None else c.ctypes.data, eye_out.ctypes.data, cam_out.ctypes.data) != 0:
        raise RuntimeError(lib.jadeh_last_error().decode())
    return eye_out, cam_out


def vertex_normals(vertices, indices, crease_deg):
    """jadeh_vertex_normals: float32 [n_triangles, 3, 3], a normal per corner of every triangle of the mesh (vertices [nv, 3], indices
    [nt, 3]) - the angle-weighted sum of the flat normals of the triangles that share the corner's vertex index and lie within
    crease_deg of the corner's triangle.  crease_deg <= 0: the flat normal thrice, bitwise.  What Scene.set_vertex_normals takes, for a
    mesh whose triangles are the scene's in this order."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    i = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    out = np.zeros((len(i), 3, 3), np.float32)
    _check(host_lib().jadeh_vertex_normals(v.ctypes.data, len(v), i.ctypes.data, len(i), float(crease_deg), out.ctypes.data))
    return out


UV_PLANAR_X, UV_PLANAR_Y, UV_PLANAR_Z, UV_SPHERICAL = 0, 1, 2, 3


def _texture_array(handle):
    """The image of a jadeh_texture handle as float32 [height, width, 3] (a copy); the handle is freed."""
    lib = host_lib()
    if not handle:
        raise RuntimeError(lib.jadeh_last_error().decode())
    try:
        w, h, p = C.c_int(), C.c_int(), C.c_void_p()
        _check(lib.jadeh_texture_get(handle, C.byref(w), C.byref(h), C.byref(p)))
        return np.frombuffer((C.c_char * (12 * w.value * h.value)).from_address(p.value), dtype=np.float32).copy().reshape(h.value, w.value, 3)
    finally:
        lib.jadeh_texture_free(handle)


def load_texture(path):
    """jadeh_texture_load: a P6 file (8 bits, sRGB decoded to linear) or a PF file (linear) as float32 [height, width, 3], row 0 the top
    of the image - what Scene.set_textures and SceneBuilder.set_texture take."""
    return _texture_array(host_lib().jadeh_texture_load(os.fsencode(path)))


def texture_checker(size, squares, a=(0.9, 0.9, 0.9), b=(0.1, 0.1, 0.1)):
    """jadeh_texture_checker: size x size texels in squares x squares squares of colours a and b."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return _texture_array(host_lib().jadeh_texture_checker(int(size), int(squares), a.ctypes.data, b.ctypes.data))


def load_normal_map(path):
    """jadeh_normal_map_load: a P6 file read linearly - no sRGB decode - as 2 c - 1 per channel, or a PF file as given, as float32 [height,
    width, 3] tangent-space vectors, row 0 the top of the image - what Scene.set_normal_maps and SceneBuilder.set_normal_map take."""
    return _texture_array(host_lib().jadeh_normal_map_load(os.fsencode(path)))


def height_to_normal_map(height, scale=1.0):
    """jadeh_height_to_normal_map: float32 [H, W] heights (row 0 at v = 0) -> the map [H, W, 3] of the surface z = scale * height(u, v):
    central differences, repeating at the borders, (-scale dh/du, -scale dh/dv, 1) unnormalised; a constant height gives (0, 0, 1) exactly."""
    h = np.ascontiguousarray(height, np.float32)
    if h.ndim != 2:
        raise ValueError("heights are [height, width]")
    return _texture_array(host_lib().jadeh_height_to_normal_map(h.shape[1], h.shape[0], h.ctypes.data, float(scale)))


def project_uvs(vertices, indices, projection=UV_SPHERICAL):
    """jadeh_project_uvs: float32 [n_triangles, 3, 2] for a mesh without UVs - UV_PLANAR_X / _Y / _Z: the two other coordinates over the
    mesh's bounding box; UV_SPHERICAL: longitude and latitude about the box's centre, the seam mended per triangle."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    i = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    out = np.zeros((len(i), 3, 2), np.float32)
    _check(host_lib().jadeh_project_uvs(v.ctypes.data, len(v), i.ctypes.data, len(i), int(projection), out.ctypes.data))
    return out


def load_obj_textured(path):
    """jadeh_load_obj_textured: (vertices [nv, 3], indices [nt, 3], uvs [nt, 3, 2] or None) of an OBJ file with `v`, `vt` and `f a/b[/c]` lines."""
    lib = host_lib()
    nv, nt, has = C.c_int(), C.c_int(), C.c_int()
    _check(lib.jadeh_load_obj_textured(os.fsencode(path), C.byref(nv), C.byref(nt), C.byref(has), None, None, None))
    v, i, uv = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32), np.zeros((nt.value, 3, 2), np.float32)
    _check(lib.jadeh_load_obj_textured(os.fsencode(path), C.byref(nv), C.byref(nt), C.byref(has), v.ctypes.data, i.ctypes.data, uv.ctypes.data))
    return v, i, (uv if has.value else None)


class HostScene:
    """Flattened scene: the arrays that cross the jade_rt.h boundary, and - optional, beside them - vertex_normals: float32
    [n_triangles, 3, 3] in the triangles' order, which Backend.scene() puts on the handle (Scene.set_vertex_normals), or None; and
    textures: (images - a list of float32 [height, width, 3], uv - float32 [n_triangles, 3, 2], image_of - int32 [n_triangles]) in the
    triangles' order, which Backend.scene() puts on the handle as well (Scene.set_textures), or None; and normal_maps: (images, uv,
    image_of, strength) the same way (Scene.set_normal_maps), or None."""

    def __init__(self, arrays, bvh_depth=None, build_seconds=0.0, vertex_normals=None, textures=None, normal_maps=None):
        # arrays: dict of numpy arrays (owned copies)
        self.a = arrays
        self.bvh_depth = bvh_depth
        self.build_seconds = build_seconds
        self.vertex_normals = vertex_normals
        self.textures = textures
        self.normal_maps = normal_maps

    ARRAY_KEYS = ("triangles", "nodes", "emit", "mapping", "prefix", "segs", "env")

    @classmethod
    def from_handle(cls, handle):
        lib = host_lib()
        d = _abi.SceneDesc()
        lib.jadeh_scene_desc(handle, C.byref(d))

        def grab(ptr, n, dtype):
            if n == 0:
                return np.zeros(0, dtype)
            buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(C.addressof(ptr.contents))
            return np.frombuffer(buf, dtype=dtype).copy()

        arrays = {
            "triangles": grab(d.triangles, d.n_triangles * 28, np.uint32).reshape(-1, 28),
            "nodes": grab(d.nodes, d.n_nodes * 10, np.uint32).reshape(-1, 10),
            "emit": grab(d.emit_indices, d.n_emit, np.int32),
            "mapping": grab(d.index_mapping, d.n_triangles, np.int32),
            "prefix": grab(d.prefix_area, d.n_triangles, np.float32),
            "segs": grab(d.obj_segs, d.n_objects * 2, np.int32).reshape(-1, 2),
            "env": grab(d.env_rgb, d.env_width * d.env_height * 3, np.float32).reshape(d.env_height, d.env_width, 3),
        }
        vn, p = None, C.c_void_p()
        n = lib.jadeh_scene_vertex_normals(handle, C.byref(p))
        if n:
            vn = np.frombuffer((C.c_char * (n * 36)).from_address(p.value), dtype=np.float32).copy().reshape(n, 3, 3)
        tex, pu, pi = None, C.c_void_p(), C.c_void_p()
        n_images = lib.jadeh_scene_textures(handle, C.byref(pu), C.byref(pi))
        if n_images:
            nt = d.n_triangles
            images = []
            for k in range(n_images):
                w, h, p = C.c_int(), C.c_int(), C.c_void_p()
                _check(lib.jadeh_scene_texture(handle, k, C.byref(w), C.byref(h), C.byref(p)))
                images.append(np.frombuffer((C.c_char * (12 * w.value * h.value)).from_address(p.value), dtype=np.float32).copy().reshape(h.value, w.value, 3))
            tex = (images, np.frombuffer((C.c_char * (24 * nt)).from_address(pu.value), dtype=np.float32).copy().reshape(nt, 3, 2),
                   np.frombuffer((C.c_char * (4 * nt)).from_address(pi.value), dtype=np.int32).copy())
        maps, pu, pi, strength = None, C.c_void_p(), C.c_void_p(), C.c_float(1.0)
        n_maps = lib.jadeh_scene_normal_maps(handle, C.byref(pu), C.byref(pi), C.byref(strength))
        if n_maps:
            nt = d.n_triangles
            images = []
            for k in range(n_maps):
                w, h, p = C.c_int(), C.c_int(), C.c_void_p()
                _check(lib.jadeh_scene_normal_map(handle, k, C.byref(w), C.byref(h), C.byref(p)))
                images.append(np.frombuffer((C.c_char * (12 * w.value * h.value)).from_address(p.value), dtype=np.float32).copy().reshape(h.value, w.value, 3))
            maps = (images, np.frombuffer((C.c_char * (24 * nt)).from_address(pu.value), dtype=np.float32).copy().reshape(nt, 3, 2),
                    np.frombuffer((C.c_char * (4 * nt)).from_address(pi.value), dtype=np.int32).copy(), float(strength.value))
        return cls(arrays, lib.jadeh_scene_bvh_depth(handle), lib.jadeh_scene_build_seconds(handle), vn, tex, maps)

    @classmethod
    def from_npz(cls, path):
        with np.load(path, allow_pickle=False) as z:
            tex = None
            if "texture_uv" in z.files:
                n = sum(1 for k in z.files if k.startswith("texture_image_") and k != "texture_image_of")
                tex = ([z[f"texture_image_{k}"].copy() for k in range(n)], z["texture_uv"].copy(), z["texture_image_of"].copy())
            maps = None
            if "normal_map_uv" in z.files:
                n = sum(1 for k in z.files if k.startswith("normal_map_image_") and k != "normal_map_image_of")
                maps = ([z[f"normal_map_image_{k}"].copy() for k in range(n)], z["normal_map_uv"].copy(), z["normal_map_image_of"].copy(), float(z["normal_map_strength"]))
            return cls({k: z[k].copy() for k in cls.ARRAY_KEYS}, vertex_normals=z["vertex_normals"].copy() if "vertex_normals" in z.files else None, textures=tex,
                       normal_maps=maps)

    def save_npz(self, path, **extra):
        if self.vertex_normals is not None:
            extra = dict(extra, vertex_normals=self.vertex_normals)
        if self.textures is not None:
            images, uv, image_of = self.textures
            extra = dict(extra, texture_uv=np.asarray(uv, np.float32), texture_image_of=np.asarray(image_of, np.int32),
                         **{f"texture_image_{k}": np.asarray(im, np.float32) for k, im in enumerate(images)})
        if self.normal_maps is not None:
            images, uv, image_of, strength = self.normal_maps
            extra = dict(extra, normal_map_uv=np.asarray(uv, np.float32), normal_map_image_of=np.asarray(image_of, np.int32), normal_map_strength=np.float32(strength),
                         **{f"normal_map_image_{k}": np.asarray(im, np.float32) for k, im in enumerate(images)})
        np.savez_compressed(path, **self.a, **extra)

    @property
    def n_triangles(self):
        return self.a["triangles"].shape[0]

    @property
    def n_nodes(self):
        return self.a["nodes"].shape[0]

    # structured views (fields of Triangle_cu / BVHNode_cu)
    def tri_f32(self):
        return self.a["triangles"].view(np.float32)

    def tri_i32(self):
        return self.a["triangles"].view(np.int32)

    def vertices(self):
        """(nT, 3, 3) float32: p1, p2, p3."""
        return self.tri_f32()[:, 1:10].reshape(-1, 3, 3)

    def node_i32(self):
        return self.a["nodes"].view(np.int32)

    def node_f32(self):
        return self.a["nodes"].view(np.float32)

    def desc(self):
        """A SceneDesc pointing into this object's arrays (keep `self` alive)."""
        a = self.a
        for k in self.ARRAY_KEYS:
            a[k] = np.ascontiguousarray(a[k])
        d = _abi.SceneDesc()
        d.abi_version = _abi.JADE_ABI_VERSION
        d.n_triangles = a["triangles"].shape[0]
        d.triangles = C.cast(a["triangles"].ctypes.data, C.POINTER(_abi.Triangle))
        d.n_nodes = a["nodes"].shape[0]
        d.nodes = C.cast(a["nodes"].ctypes.data, C.POINTER(_abi.BvhNode))
        d.n_emit = a["emit"].shape[0]
        d.emit_indices = C.cast(a["emit"].ctypes.data, C.POINTER(C.c_int32))
        d.index_mapping = C.cast(a["mapping"].ctypes.data, C.POINTER(C.c_int32))
        d.prefix_area = C.cast(a["prefix"].ctypes.data, C.POINTER(C.c_float))
        d.n_objects = a["segs"].shape[0]
        d.obj_segs = C.cast(a["segs"].ctypes.data, C.POINTER(_abi.ObjSeg))
        d.env_height, d.env_width = a["env"].shape[:2]
        d.env_rgb = C.cast(a["env"].ctypes.data, C.POINTER(C.c_float))
        return d


class SceneBuilder:
    """One add_*() call == one readObj() call of the reference (one object)."""

    def __init__(self):
        self._lib = host_lib()
        self._h = self._lib.jadeh_builder_new()

    def close(self):
        if self._h:
            self._lib.jadeh_builder_free(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _t(trans):
        if trans is None:
            trans = transform_matrix()
        return np.ascontiguousarray(trans, np.float32)

    def add_mesh(self, vertices, indices, mat, trans=None, normalize=False, uvs=None):
        """uvs: float32 [n_triangles, 3, 2], the mesh's own texture coordinates (used while a texture is set: set_texture)."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
        t = self._t(trans)
        if uvs is not None:
            u = np.ascontiguousarray(uvs, np.float32)
            if u.size != 6 * len(i):
                raise ValueError("add_mesh: 6 floats of uv per triangle")
            _check(self._lib.jadeh_builder_add_mesh_uv(self._h, v.ctypes.data, len(v), i.ctypes.data, len(i), u.ctypes.data, C.byref(mat),
                                                       t.ctypes.data, int(normalize)))
            return
        _check(self._lib.jadeh_builder_add_mesh(self._h, v.ctypes.data, len(v), i.ctypes.data, len(i), C.byref(mat),
                                                t.ctypes.data, int(normalize)))

    def add_obj(self, path, mat, trans=None, normalize=False):
        t = self._t(trans)
        _check(self._lib.jadeh_builder_add_obj(self._h, os.fsencode(path), C.byref(mat), t.ctypes.data, int(normalize)))

    def add_proc(self, kind, param, mat, trans=None, normalize=False, seed=0):
        t = self._t(trans)
        _check(self._lib.jadeh_builder_add_proc(self._h, kind.encode(), int(param), int(seed), C.byref(mat),
                                                t.ctypes.data, int(normalize)))

    def set_smoothing(self, crease_deg):
        """jadeh_builder_set_smoothing: the meshes added from now on get vertex normals (vertex_normals() after the mesh's transform;
        <= 0: flat again).  The built HostScene then carries `vertex_normals`."""
        _check(self._lib.jadeh_builder_set_smoothing(self._h, float(crease_deg)))

    def set_texture(self, image, projection=UV_SPHERICAL):
        """jadeh_builder_set_texture: the meshes added from now on carry `image` (float32 [height, width, 3], linear, row 0 at v = 0; None:
        no image again) with their own UVs - add_mesh's uvs, a "quad"'s, an OBJ's `vt` lines - or, where they have none, those of
        `projection` (UV_*).  The built HostScene then carries `textures`."""
        if image is None:
            _check(self._lib.jadeh_builder_set_texture(self._h, None, int(projection)))
            return
        self._with_texture(image, lambda t: self._lib.jadeh_builder_set_texture(self._h, t, int(projection)))

    def set_object_texture(self, obj, image, projection=UV_SPHERICAL):
        """jadeh_builder_set_object_texture: the obj'th object to be added (0-based; the objects of config() count) carries `image`,
        whatever set_texture says when it arrives - what jade_render --texture OBJ=IMAGE does."""
        self._with_texture(image, lambda t: self._lib.jadeh_builder_set_object_texture(self._h, int(obj), t, int(projection)))

    def set_normal_map(self, image, projection=UV_SPHERICAL, strength=1.0):
        """jadeh_builder_set_normal_map: the meshes added from now on carry the normal map `image` (float32 [height, width, 3] tangent-space
        vectors; None: no map again) with their own UVs or those of `projection`, as set_texture; one strength for the scene, the last
        given.  The built HostScene then carries `normal_maps`."""
        if image is None:
            _check(self._lib.jadeh_builder_set_normal_map(self._h, None, int(projection), float(strength)))
            return
        self._with_texture(image, lambda t: self._lib.jadeh_builder_set_normal_map(self._h, t, int(projection), float(strength)))

    def set_object_normal_map(self, obj, image, projection=UV_SPHERICAL, strength=1.0):
        """jadeh_builder_set_object_normal_map: the obj'th object to be added carries the normal map `image` - what jade_render
        --normal-map OBJ=FILE does."""
        self._with_texture(image, lambda t: self._lib.jadeh_builder_set_object_normal_map(self._h, int(obj), t, int(projection), float(strength)))

    def _with_texture(self, image, call):
        im = np.ascontiguousarray(image, np.float32)
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("an image is [height, width, 3]")
        t = self._lib.jadeh_texture_data(im.shape[1], im.shape[0], im.ctypes.data)
        if not t:
            raise RuntimeError(self._lib.jadeh_last_error().decode())
        try:
            _check(call(t))
        finally:
            self._lib.jadeh_texture_free(t)

    def set_env_constant(self, r, g, b):
        _check(self._lib.jadeh_builder_set_env_constant(self._h, r, g, b))

    def set_env_sky(self, w=1024, h=512):
        _check(self._lib.jadeh_builder_set_env_sky(self._h, w, h))

    def set_env_data(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.float32)
        h, w = rgb.shape[:2]
        _check(self._lib.jadeh_builder_set_env_data(self._h, w, h, rgb.ctypes.data))

    def set_env_hdr(self, path):
        _check(self._lib.jadeh_builder_set_env_hdr(self._h, os.fsencode(path)))

    def config(self, name):
        """Fill the builder with a built-in configuration; returns its Config."""
        cfg = _abi.Config()
        _check(self._lib.jadeh_builder_config(self._h, name.encode(), C.byref(cfg)))
        return cfg

    def load_render_args(self, path):
        cfg = _abi.Config()
        _check(self._lib.jadeh_builder_load_render_args(self._h, os.fsencode(path), C.byref(cfg)))
        return cfg

    @property
    def triangle_count(self):
        return self._lib.jadeh_builder_triangle_count(self._h)

    def triangles_original(self):
        """(n, 28) uint32 view of the Triangle_cu records in ORIGINAL order (input of an external BVH builder)."""
        n = self.triangle_count
        out = np.zeros((n, 28), np.uint32)
        _check(self._lib.jadeh_builder_triangles(self._h, out.ctypes.data, n))
        return out

    def build_with_bvh(self, order, nodes):
        """Flatten around a BVH built elsewhere: order[i] = original index of sorted triangle i."""
        order = np.ascontiguousarray(order, np.int32)
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 10)
        h = self._lib.jadeh_builder_build_with_bvh(self._h, order.ctypes.data, nodes.ctypes.data, len(nodes))
        if not h:
            raise RuntimeError(self._lib.jadeh_last_error().decode())
        try:
            return HostScene.from_handle(h)
        finally:
            self._lib.jadeh_scene_free(h)

    def build_device_bvh(self, backend, kind="ploc", leaf_size=8, device_id=0):
        """(HostScene, device build milliseconds) with the BVH built on the GPU (include/jade_bvh.h): "lbvh" (Morton order +
        Karras' radix tree) or "ploc" (locally-ordered clustering by surface area)."""
        if kind not in ("lbvh", "ploc"):
            raise ValueError(f"unknown device BVH builder {kind!r}")
        tris = self.triangles_original()
        n = len(tris)
        lib = _abi.bind(backend.lib, _abi.BVH_SYMBOLS)
        order = np.zeros(n, np.int32)
        nodes = np.zeros((2 * n + 1, 10), np.uint32)
        n_nodes = C.c_int32(0)
        ms = C.c_double(0)
        fn = lib.jade_bvh_build_lbvh if kind == "lbvh" else lib.jade_bvh_build_ploc
        backend.check(fn(tris.ctypes.data, n, leaf_size, device_id, order.ctypes.data, nodes.ctypes.data, len(nodes), C.byref(n_nodes),
                         C.byref(ms)))
        return self.build_with_bvh(order, nodes[: n_nodes.value]), ms.value

    def build_lbvh(self, backend, leaf_size=8, device_id=0):
        return self.build_device_bvh(backend, "lbvh", leaf_size, device_id)

    def build_ploc(self, backend, leaf_size=3, device_id=0):
        # 3 triangles per leaf: measured on C3 / C5 the best trade of node records against triangle tests for this builder
        return self.build_device_bvh(backend, "ploc", leaf_size, device_id)

    def build(self, leaf_size=8):
        h = self._lib.jadeh_builder_build(self._h, leaf_size)
        if not h:
            raise RuntimeError(self._lib.jadeh_last_error().decode())
        try:
            return HostScene.from_handle(h)
        finally:
            self._lib.jadeh_scene_free(h)


def build_config(name):
    """(HostScene, Config) for a built-in configuration: tiny, tinyjade, C1..C5."""
    b = SceneBuilder()
    try:
        cfg = b.config(name)
        return b.build(), cfg
    finally:
        b.close()


def object_tiles(hs, eye, camera, width, height, obj=0):
    """{tile id (ty * tiles_x + tx): vertices of object `obj` that project into it}: the camera mapping of
    PathTrace.cu:1430-1437 inverted (dir ~ M . (lx * W/H, ly, -1.5, 0), lx = -1 + 2/W (x + u - 0.5), M[col][row])."""
    v = hs.vertices()[hs.tri_i32()[:, 0] == obj].reshape(-1, 3).astype(np.float64)
    m = np.asarray(list(camera), np.float64).reshape(4, 4)
    rel = v - np.asarray(list(eye), np.float64)
    a, b, c = rel @ m[0, :3], rel @ m[1, :3], rel @ m[2, :3]
    front = c < 0
    s = -1.5 / c[front]
    lx, ly = a[front] * s / (width / height), b[front] * s
    x, y = np.floor((lx + 1) * width / 2), np.floor((ly + 1) * height / 2)
    ok = (x >= 0) & (x < width) & (y >= 0) & (y < height)
    tiles_x = (width + 15) // 16
    ids, cnt = np.unique((y[ok] // 16).astype(np.int64) * tiles_x + (x[ok] // 16).astype(np.int64), return_counts=True)
    return dict(zip(ids.tolist(), cnt.tolist()))


def write_bmp(path, bgr8):
    h, w = bgr8.shape[:2]
    a = np.ascontiguousarray(bgr8, np.uint8)
    _check(host_lib().jadeh_write_bmp(os.fsencode(path), a.ctypes.data, w, h))


def write_ppm(path, bgr8):
    h, w = bgr8.shape[:2]
    a = np.ascontiguousarray(bgr8, np.uint8)
    _check(host_lib().jadeh_write_ppm(os.fsencode(path), a.ctypes.data, w, h))


def write_pfm(path, rgb):
    h, w = rgb.shape[:2]
    a = np.ascontiguousarray(rgb, np.float32)
    _check(host_lib().jadeh_write_pfm(os.fsencode(path), a.ctypes.data, w, h))
