"""ctypes mirrors of include/jade_rt.h and include/jade_host_c.h.

Field order and types must match the headers exactly; tests/test_abi.py checks
the struct sizes against the C compiler's (112 / 40 / 8 bytes for the three
reference device structs, PathTrace.cu:327-351).
"""
import ctypes as C

JADE_ABI_VERSION = 7
JADE_SAMPLE_LANES = 1024
JADE_OK, JADE_ERR_INVALID, JADE_ERR_DEVICE, JADE_ERR_NOMEM, JADE_ERR_UNSUPPORTED = range(5)
DIFFUSE, MIRROR = 0, 1
NO_REFRACT, SUB_SURFACE, DIR_REFRACT = 0, 1, 2
TILE_SIZE = 16
TONEMAP_ACES, TONEMAP_REINHARD = 0, 1
Q_RECORDS_PER_PIXEL, Q_STATE_BYTES, Q_SUM_LANES = 0, 1, 2
WALK_REFERENCE, WALK_EARLY_EXIT, WALK_EARLY_EXIT_CACHED = 0, 1, 2
ENV_REFERENCE, ENV_IMPORTANCE, ENV_MIXTURE = 0, 1, 2
LIGHTS_ALL, LIGHTS_ONE = 0, 1  # include/jade_bvh.h, jade_scene_set_light_sampling
BOUNCE_UNIFORM, BOUNCE_COSINE = 0, 1  # include/jade_bvh.h, jade_scene_set_bounce_sampling
DIRECT_RAYS, DIRECT_MIS = 0, 1  # include/jade_bvh.h, jade_scene_set_direct_sampling
BRANCH_RANDOM, BRANCH_STRATIFIED = 0, 1  # include/jade_bvh.h, jade_scene_set_branch_sampling
PASS_COUNT = 15  # include/jade_bvh.h, jade_render_passes; jade_pass_name gives these
PASS_NAMES = ("background", "emission", "specular_sky") + tuple(
    f"{kind}_{source}_{depth}" for kind in ("diffuse", "sss", "bssrdf") for source in ("emitter", "sky") for depth in ("first", "later"))
EXPOSURE_MANUAL, EXPOSURE_AUTO = 0, 1
METER_BINS = 512

f3 = C.c_float * 3
f16 = C.c_float * 16


class Triangle(C.Structure):  # == Triangle_cu, PathTrace.cu:327-338
    _fields_ = [
        ("obj_idx", C.c_int32),
        ("p1", f3), ("p2", f3), ("p3", f3),
        ("norm", f3), ("emissive", f3), ("brdf", f3),
        ("reflex_mode", C.c_int32), ("refract_mode", C.c_int32),
        ("refract_rate", f3), ("refract_albedo", f3),
        ("refract_index", C.c_float),
    ]


class BvhNode(C.Structure):  # == BVHNode_cu, PathTrace.cu:341-345
    _fields_ = [("left", C.c_int32), ("right", C.c_int32), ("n", C.c_int32), ("index", C.c_int32),
                ("aa", f3), ("bb", f3)]


class ObjSeg(C.Structure):  # == Obj_seg, PathTrace.cu:348-351
    _fields_ = [("begin_idx", C.c_int32), ("end_idx", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_triangles", C.c_int32), ("triangles", C.POINTER(Triangle)),
        ("n_nodes", C.c_int32), ("nodes", C.POINTER(BvhNode)),
        ("n_emit", C.c_int32), ("emit_indices", C.POINTER(C.c_int32)),
        ("index_mapping", C.POINTER(C.c_int32)),
        ("prefix_area", C.POINTER(C.c_float)),
        ("n_objects", C.c_int32), ("obj_segs", C.POINTER(ObjSeg)),
        ("env_width", C.c_int32), ("env_height", C.c_int32),
        ("env_rgb", C.POINTER(C.c_float)),
    ]


class RenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("frame", C.c_uint32),
        ("eye", f3), ("camera", f16),
        ("tile_rank", C.c_int32), ("tile_nranks", C.c_int32),
        ("device_id", C.c_int32), ("threads", C.c_int32),
        ("max_state_bytes", C.c_uint64),
        ("walk", C.c_int32),
        ("env_sampling", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("rays_primary", C.c_uint64), ("rays_secondary", C.c_uint64),
        ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64),
        ("shaded_hits", C.c_uint64), ("samples", C.c_uint64),
        ("kernel_ms", C.c_double),
        ("trace_ms", C.c_double), ("trace_launches", C.c_uint64),
        ("rays_shadow", C.c_uint64), ("rays_env", C.c_uint64), ("rays_indirect", C.c_uint64),
        ("rays_mirror", C.c_uint64), ("rays_refract", C.c_uint64), ("host_syncs", C.c_uint64),
        ("rays_inline", C.c_uint64), ("light_ms", C.c_double),
        ("nodes_inline", C.c_uint64), ("tris_inline", C.c_uint64),
        ("rays_cached", C.c_uint64),
        ("rays_tail", C.c_uint64), ("nodes_tail", C.c_uint64), ("tris_tail", C.c_uint64),
        ("tail_ms", C.c_double), ("tail_launches", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    @property
    def rays(self):
        return self.rays_primary + self.rays_secondary


class DenoiseParams(C.Structure):  # == jade_denoise_params, include/jade_bvh.h
    _fields_ = [
        ("iterations", C.c_int32), ("guide_spp", C.c_int32),
        ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
    ]


class MeterStruct(C.Structure):  # == jade_meter, include/jade_bvh.h
    _fields_ = [
        ("bins", C.c_uint64 * METER_BINS),
        ("n_positive", C.c_uint64), ("n_zero", C.c_uint64), ("n_negative", C.c_uint64), ("n_nonfinite", C.c_uint64),
        ("lum_min", C.c_float), ("lum_max", C.c_float),
    ]


class DisplayParams(C.Structure):  # == jade_display_params, include/jade_bvh.h
    _fields_ = [
        ("tonemap", C.c_int32), ("limit", C.c_float),
        ("exposure_mode", C.c_int32), ("exposure", C.c_float),
        ("key", C.c_float), ("p_lo", C.c_float), ("p_hi", C.c_float),
        ("min_exposure", C.c_float), ("max_exposure", C.c_float),
    ]


class GlareParams(C.Structure):  # == jade_glare_params, include/jade_bvh.h
    _fields_ = [("levels", C.c_int32), ("strength", C.c_float), ("falloff", C.c_float)]


class DespeckleParams(C.Structure):  # == jade_despeckle_params, include/jade_bvh.h
    _fields_ = [("iterations", C.c_int32), ("radius", C.c_int32), ("rank", C.c_int32),
                ("gain", C.c_float), ("floor", C.c_float), ("sigmas", C.c_float)]


class DespeckleReport(C.Structure):  # == jade_despeckle_report, include/jade_bvh.h
    _fields_ = [("n_usable", C.c_uint64), ("n_above", C.c_uint64), ("n_established", C.c_uint64), ("n_clamped", C.c_uint64)]


class LensParams(C.Structure):  # == jade_lens_params, include/jade_bvh.h
    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float)]


class ShutterParams(C.Structure):  # == jade_shutter_params, include/jade_bvh.h
    _fields_ = [("eye_close", f3), ("camera_close", C.c_float * 16), ("t_open", C.c_float), ("t_close", C.c_float)]


class TextureImage(C.Structure):  # == jade_texture_image, include/jade_bvh.h
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_float))]


class Material(C.Structure):  # == Material, PathTrace.cu:293-301
    _fields_ = [
        ("emissive", f3), ("brdf", f3),
        ("reflex_mode", C.c_int32), ("refract_mode", C.c_int32),
        ("refract_rate", f3), ("refract_albedo", f3),
        ("refract_index", C.c_float),
    ]


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("eye", f3), ("camera", f16)]


# every symbol jade_rt.h declares: name -> (restype, argtypes)
RT_SYMBOLS = {
    "jade_abi_version": (C.c_int, []),
    "jade_backend_name": (C.c_char_p, []),
    "jade_last_error": (C.c_char_p, []),
    "jade_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "jade_scene_create": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "jade_scene_destroy": (None, [C.c_void_p]),
    "jade_render": (C.c_int, [C.c_void_p, C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "jade_render_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(RenderParams), C.c_void_p, C.c_void_p,
                                    C.POINTER(Stats)]),
    "jade_render_begin": (C.c_int, [C.c_void_p, C.POINTER(RenderParams)]),
    "jade_render_step": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Stats)]),
    "jade_render_flush": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "jade_render_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "jade_render_resolve_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "jade_render_resolve_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "jade_render_query": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "jade_owned_tile_count": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "jade_trace_rays": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(Stats)]),
}

# include/jade_bvh.h (exported by libjade_hip.so)
_BVH_SIG = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                      C.POINTER(C.c_double)])
BVH_SYMBOLS = {
    "jade_bvh_build_lbvh": _BVH_SIG,
    "jade_bvh_build_ploc": _BVH_SIG,
    # adaptive sampling and its noise map (scene, params, min_spp, rel_error, error_floor, rgb, bgr8, tile_spp, stats)
    "jade_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(RenderParams), C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(Stats)]),
    "jade_render_error": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p]),
    # the denoiser: defaults, guides (scene, guide_spp, albedo, normal, depth, variance), the render's frame (scene, params, tonemap,
    # limit, rgb, bgr8) and caller images (device, width, height, rgb, variance, albedo, normal, depth, params, out rgb)
    "jade_denoise_defaults": (None, [C.POINTER(DenoiseParams)]),
    "jade_render_guides": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jade_render_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "jade_denoise_image": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(DenoiseParams), C.c_void_p]),
    # exposure: defaults, the policy (meter, params) -> e, the render's meter, the exposed resolve (scene, params, rgb, bgr8, exposure
    # used, meter) and caller images (device, width, height, rgb, params, bgr8, exposure used, meter)
    "jade_display_defaults": (None, [C.POINTER(DisplayParams)]),
    "jade_meter_exposure": (C.c_float, [C.POINTER(MeterStruct), C.POINTER(DisplayParams)]),
    "jade_render_meter": (C.c_int, [C.c_void_p, C.POINTER(MeterStruct)]),
    "jade_render_resolve_exposed": (C.c_int, [C.c_void_p, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                                              C.POINTER(MeterStruct)]),
    "jade_expose_image": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(DisplayParams), C.c_void_p,
                                    C.POINTER(C.c_float), C.POINTER(MeterStruct)]),
    # glare: defaults, caller images (device, width, height, rgb, params, out rgb) and the render's frame (scene, params, display
    # params or null, rgb, bgr8, exposure used)
    "jade_glare_defaults": (None, [C.POINTER(GlareParams)]),
    "jade_glare_image": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(GlareParams), C.c_void_p]),
    "jade_render_glare": (C.c_int, [C.c_void_p, C.POINTER(GlareParams), C.POINTER(DisplayParams), C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_float)]),
    # despeckle: defaults, caller images (device, width, height, rgb, variance or null, params, out rgb, out variance or null, out
    # scale or null, report or null) and the render's frame (scene, params, denoise params or null, tonemap, limit, rgb, bgr8, scale,
    # report)
    "jade_despeckle_defaults": (None, [C.POINTER(DespeckleParams)]),
    "jade_despeckle_image": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(DespeckleParams), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(DespeckleReport)]),
    "jade_render_despeckle": (C.c_int, [C.c_void_p, C.POINTER(DespeckleParams), C.POINTER(DenoiseParams), C.c_int, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DespeckleReport)]),
    # the thin lens of a scene handle (scene, lens or null) / (scene, out)
    "jade_scene_set_lens": (C.c_int, [C.c_void_p, C.POINTER(LensParams)]),
    "jade_scene_get_lens": (C.c_int, [C.c_void_p, C.POINTER(LensParams)]),
    # the shutter of a scene handle (scene, shutter or null) / (scene, out, is_set)
    "jade_scene_set_shutter": (C.c_int, [C.c_void_p, C.POINTER(ShutterParams)]),
    "jade_scene_get_shutter": (C.c_int, [C.c_void_p, C.POINTER(ShutterParams), C.POINTER(C.c_int)]),
    # the light sampling of a scene handle (scene, mode) / (scene, out)
    "jade_scene_set_light_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "jade_scene_get_light_sampling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # the bounce sampling of a scene handle (scene, mode) / (scene, out)
    "jade_scene_set_bounce_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "jade_scene_get_bounce_sampling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # the direct sampling of a scene handle (scene, mode) / (scene, out)
    "jade_scene_set_direct_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "jade_scene_get_direct_sampling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # the passes of a scene handle (scene, on) / (scene, out); a pass's name; the render's passes (scene, out: PASS_COUNT x H x W x 3 floats)
    "jade_scene_set_passes": (C.c_int, [C.c_void_p, C.c_int]),
    "jade_scene_get_passes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jade_pass_name": (C.c_char_p, [C.c_int]),
    "jade_render_passes": (C.c_int, [C.c_void_p, C.c_void_p]),
    # the branch sampling of a scene handle (scene, mode) / (scene, out)
    "jade_scene_set_branch_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "jade_scene_get_branch_sampling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # the vertex normals of a scene handle (scene, 9 floats per triangle or null, n_triangles) / (scene, out: 1 if a table is set)
    "jade_scene_set_vertex_normals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "jade_scene_get_vertex_normals": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # the textures of a scene handle (scene, n_images, images, 6 floats of uv per triangle, an image number per triangle, n_triangles) / (scene, out: 1 if set)
    "jade_scene_set_textures": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(TextureImage), C.c_void_p, C.c_void_p, C.c_int32]),
    "jade_scene_get_textures": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # the normal maps of a scene handle: as the textures, the map's own uv and image numbers, and a strength / (scene, out: 1 if set)
    "jade_scene_set_normal_maps": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(TextureImage), C.c_void_p, C.c_void_p, C.c_int32, C.c_float]),
    "jade_scene_get_normal_maps": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
}

HOST_SYMBOLS = {
    "jadeh_last_error": (C.c_char_p, []),
    "jadeh_builder_new": (C.c_void_p, []),
    "jadeh_builder_free": (None, [C.c_void_p]),
    "jadeh_builder_triangle_count": (C.c_int, [C.c_void_p]),
    "jadeh_builder_add_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(Material),
                                         C.c_void_p, C.c_int]),
    "jadeh_builder_add_obj": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(Material), C.c_void_p, C.c_int]),
    "jadeh_builder_add_proc": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.POINTER(Material), C.c_void_p,
                                         C.c_int]),
    "jadeh_write_proc_obj": (C.c_int, [C.c_char_p, C.c_int, C.c_uint, C.c_char_p]),
    "jadeh_builder_set_smoothing": (C.c_int, [C.c_void_p, C.c_float]),
    "jadeh_vertex_normals": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "jadeh_scene_vertex_normals": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    # textures: images (load / checker / data -> handle), the builder's current texture, UVs, the built scene's table
    "jadeh_texture_load": (C.c_void_p, [C.c_char_p]),
    "jadeh_texture_checker": (C.c_void_p, [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "jadeh_texture_data": (C.c_void_p, [C.c_int, C.c_int, C.c_void_p]),
    "jadeh_texture_free": (None, [C.c_void_p]),
    "jadeh_texture_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "jadeh_builder_set_texture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "jadeh_builder_set_object_texture": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "jadeh_builder_add_mesh_uv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Material), C.c_void_p, C.c_int]),
    "jadeh_project_uvs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "jadeh_load_obj_textured": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
    "jadeh_scene_textures": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "jadeh_scene_texture": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    # normal maps: images (load / heights -> handle), the builder's current map and an object's, the built scene's table
    "jadeh_normal_map_load": (C.c_void_p, [C.c_char_p]),
    "jadeh_height_to_normal_map": (C.c_void_p, [C.c_int, C.c_int, C.c_void_p, C.c_float]),
    "jadeh_builder_set_normal_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float]),
    "jadeh_builder_set_object_normal_map": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float]),
    "jadeh_scene_normal_maps": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_float)]),
    "jadeh_scene_normal_map": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "jadeh_builder_set_env_constant": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "jadeh_builder_set_env_sky": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jadeh_builder_set_env_data": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "jadeh_builder_set_env_hdr": (C.c_int, [C.c_void_p, C.c_char_p]),
    "jadeh_builder_config": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(Config)]),
    "jadeh_builder_load_render_args": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(Config)]),
    "jadeh_builder_build": (C.c_void_p, [C.c_void_p, C.c_int]),
    "jadeh_builder_triangles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "jadeh_builder_build_with_bvh": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "jadeh_scene_free": (None, [C.c_void_p]),
    "jadeh_scene_desc": (None, [C.c_void_p, C.POINTER(SceneDesc)]),
    "jadeh_scene_bvh_depth": (C.c_int, [C.c_void_p]),
    "jadeh_scene_build_seconds": (C.c_double, [C.c_void_p]),
    "jadeh_transform_matrix": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jadeh_camera_orbit": (None, [C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    # autofocus (the backend's jade_trace_rays, scene, params, px, py, out)
    "jadeh_focus_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RenderParams), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    # a second pose for the shutter (eye, cam, truck or null, orbit_deg, pivot or null, eye_out, cam_out)
    "jadeh_camera_move": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jadeh_write_bmp": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "jadeh_write_ppm": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "jadeh_write_pfm": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
}


def bind(lib, table):
    """Attach restype/argtypes; raises AttributeError naming a missing symbol."""
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
