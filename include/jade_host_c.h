/*
 * jade_host_c.h — C entry points of the host scene pipeline (libjade_host.so).
 *
 * This is NOT the drop-in boundary (that is jade_rt.h); it is the repo's own
 * host side — OBJ / render_args.txt loading, procedural stand-ins for the
 * reference's git-ignored assets, the SAH BVH builder, camera and image
 * writers (roles of PathTrace.cu:355-628, 1487-1612, 74-106 and
 * PathTrace.cpp:343-359, 684-687, 883-918) — exposed with C linkage so the
 * CLI, the Python package and the tests can produce a jade_scene_desc.
 * All functions returning int return 0 on success; jadeh_last_error() holds
 * the message otherwise.
 */
#ifndef JADE_HOST_C_H
#define JADE_HOST_C_H

#include <stdint.h>

#include "jade_rt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* == Material, PathTrace.cu:293-301 */
typedef struct jadeh_material {
  float emissive[3];
  float brdf[3];
  int32_t reflex_mode;
  int32_t refract_mode;
  float refract_rate[3];
  float refract_albedo[3];
  float refract_index;
} jadeh_material;

typedef struct jadeh_config {
  int32_t width, height, spp;
  float eye[3];
  float camera[16];
} jadeh_config;

typedef struct jadeh_builder jadeh_builder;
typedef struct jadeh_scene jadeh_scene;

const char* jadeh_last_error(void);

jadeh_builder* jadeh_builder_new(void);
void jadeh_builder_free(jadeh_builder* b);
int jadeh_builder_triangle_count(const jadeh_builder* b);

/* one object = one readObj() call: optional normalise (reference quirk
 * included), 4x4 transform ([col][row] order), flat normals */
int jadeh_builder_add_mesh(jadeh_builder* b, const float* verts, int nv, const int* idx, int nt,
                           const jadeh_material* mat, const float* trans16, int normalize);
int jadeh_builder_add_obj(jadeh_builder* b, const char* path, const jadeh_material* mat,
                          const float* trans16, int normalize);
/* kind: "box" | "quad" | "geodesic" (param = frequency, 20*f^2 triangles) |
 *       "statue" | "dragon" (param = frequency, seed) */
int jadeh_builder_add_proc(jadeh_builder* b, const char* kind, int param, unsigned seed,
                           const jadeh_material* mat, const float* trans16, int normalize);
int jadeh_write_proc_obj(const char* kind, int param, unsigned seed, const char* path);

/* Smooth shading (include/jade_bvh.h, jade_scene_set_vertex_normals).  jadeh_builder_set_smoothing: the meshes added from now on get
 * vertex normals - a corner's is the angle-weighted sum of the flat normals of the mesh's triangles that share its vertex index and lie
 * within crease_deg of the corner's triangle, formed after the mesh's transform; <= 0 (the default): flat.  OBJ `vn` lines are not read.
 * jadeh_vertex_normals: the same function on a caller's mesh, 9 floats per triangle into out9.  jadeh_scene_vertex_normals: the built
 * scene's table in BVH order (*out; owned by s) and its triangle count, or 0 and NULL if no mesh was smoothed. */
int jadeh_builder_set_smoothing(jadeh_builder* b, float crease_deg);
int jadeh_vertex_normals(const float* verts, int nv, const int* idx, int nt, float crease_deg, float* out9);
int jadeh_scene_vertex_normals(const jadeh_scene* s, const float** out);

/* Albedo textures (include/jade_bvh.h, jade_scene_set_textures).  A jadeh_texture is an image of linear RGB, row 0 at v = 0 (the top of
 * an image file): jadeh_texture_load reads a P6 file of 8 bits per channel (sRGB decoded in double, rounded once) or a PF file (linear;
 * its rows, stored bottom to top, are flipped) by the file's own magic; jadeh_texture_checker makes size x size texels in squares x
 * squares squares of colours a and b; jadeh_texture_data copies a caller's width x height x 3 floats.  NULL on failure.
 * jadeh_builder_set_texture: the meshes added from now on carry the image (NULL: none, the default), with their own UVs - a quad's, those
 * jadeh_builder_add_mesh_uv or an OBJ's `vt` lines give - or, where they have none, those of `projection`: 0 1 2 planar along x y z,
 * 3 spherical (jadeh_project_uvs: the same function on a caller's mesh, 6 floats per triangle into out6).  While a texture is set,
 * jadeh_builder_add_obj reads its file with the `v` / `vt` / `f a/b[/c]` reader; without one it reads as it always did.
 * jadeh_load_obj_textured: that reader by itself - counts first (NULL arrays), then the arrays: verts 3 per vertex, idx 3 per triangle,
 * uv6 6 per triangle (*has_uv = 0 and zeros if the file has no `vt` line).
 * jadeh_scene_textures: the built scene's table in BVH order - *uv 6 floats and *image_of one number per triangle (owned by s) - and
 * the number of images, 0 if no mesh was textured; jadeh_scene_texture: image k of it (*rgb owned by s). */
typedef struct jadeh_texture jadeh_texture;
jadeh_texture* jadeh_texture_load(const char* path);
jadeh_texture* jadeh_texture_checker(int size, int squares, const float a[3], const float b[3]);
jadeh_texture* jadeh_texture_data(int width, int height, const float* rgb);
void jadeh_texture_free(jadeh_texture* t);
int jadeh_texture_get(const jadeh_texture* t, int* width, int* height, const float** rgb);
int jadeh_builder_set_texture(jadeh_builder* b, const jadeh_texture* t, int projection);
/* ... and the texture of the object'th mesh to be added (0-based, in the order of the add calls, a configuration's included), whatever
 * jadeh_builder_set_texture says when it arrives: one object of a configuration the caller does not build itself. */
int jadeh_builder_set_object_texture(jadeh_builder* b, int object, const jadeh_texture* t, int projection);
int jadeh_builder_add_mesh_uv(jadeh_builder* b, const float* verts, int nv, const int* idx, int nt, const float* uv6, const jadeh_material* mat,
                              const float* trans16, int normalize);
int jadeh_project_uvs(const float* verts, int nv, const int* idx, int nt, int projection, float* out6);
int jadeh_load_obj_textured(const char* path, int* nv, int* nt, int* has_uv, float* verts, int* idx, float* uv6);
int jadeh_scene_textures(const jadeh_scene* s, const float** uv, const int32_t** image_of);
int jadeh_scene_texture(const jadeh_scene* s, int k, int* width, int* height, const float** rgb);

/* Normal maps (include/jade_bvh.h, jade_scene_set_normal_maps).  A map is a jadeh_texture of tangent-space vectors (x, y, z), decoded:
 * jadeh_normal_map_load reads a P6 file LINEARLY - no sRGB decode - as 2 c - 1 per channel, or a PF file as given;
 * jadeh_height_to_normal_map makes the map of the surface z = scale * height(u, v) from width x height heights (row 0 at v = 0) by
 * central differences, the image repeating at its borders: (0 - scale dh/du, 0 - scale dh/dv, 1), not normalised - a constant height
 * gives (0, 0, 1) exactly.  NULL on failure; freed with jadeh_texture_free, read with jadeh_texture_get.
 * jadeh_builder_set_normal_map / jadeh_builder_set_object_normal_map: as the two texture setters, with the map's own UVs - the mesh's
 * or the projection's - independent of the albedo texture; the table has one strength (finite, >= 0), the last one given.
 * jadeh_scene_normal_maps / jadeh_scene_normal_map: the built scene's table in BVH order, as jadeh_scene_textures / jadeh_scene_texture. */
jadeh_texture* jadeh_normal_map_load(const char* path);
jadeh_texture* jadeh_height_to_normal_map(int width, int height, const float* heights, float scale);
int jadeh_builder_set_normal_map(jadeh_builder* b, const jadeh_texture* t, int projection, float strength);
int jadeh_builder_set_object_normal_map(jadeh_builder* b, int object, const jadeh_texture* t, int projection, float strength);
int jadeh_scene_normal_maps(const jadeh_scene* s, const float** uv, const int32_t** image_of, float* strength);
int jadeh_scene_normal_map(const jadeh_scene* s, int k, int* width, int* height, const float** xyz);
int jadeh_builder_set_env_constant(jadeh_builder* b, float r, float g, float bl);
int jadeh_builder_set_env_sky(jadeh_builder* b, int w, int h);
int jadeh_builder_set_env_data(jadeh_builder* b, int w, int h, const float* rgb);
int jadeh_builder_set_env_hdr(jadeh_builder* b, const char* path); /* Radiance RGBE */

/* built-in configurations: "tiny", "tinyjade", "C1".."C5"  */
int jadeh_builder_config(jadeh_builder* b, const char* name, jadeh_config* out);
/* render_args.txt (PathTrace.cu:1487-1525); OBJ paths relative to the file */
int jadeh_builder_load_render_args(jadeh_builder* b, const char* path, jadeh_config* out);

/* prefix sums + SAH BVH (leaf_size 8 in the reference) + encode */
jadeh_scene* jadeh_builder_build(jadeh_builder* b, int leaf_size);
/* the same flattening around a BVH built elsewhere (include/jade_bvh.h: the GPU LBVH builder):
 * jadeh_builder_triangles() gives that builder its input (original order), and
 * jadeh_builder_build_with_bvh() takes its output (order[i] = original index of sorted triangle i) */
int jadeh_builder_triangles(const jadeh_builder* b, jade_triangle* out, int capacity);
jadeh_scene* jadeh_builder_build_with_bvh(jadeh_builder* b, const int32_t* order, const jade_bvh_node* nodes, int n_nodes);
void jadeh_scene_free(jadeh_scene* s);
void jadeh_scene_desc(const jadeh_scene* s, jade_scene_desc* out); /* pointers owned by s */
int jadeh_scene_bvh_depth(const jadeh_scene* s);
double jadeh_scene_build_seconds(const jadeh_scene* s);

void jadeh_transform_matrix(const float rot_deg[3], const float trans[3], const float scale[3], float out16[16]);
void jadeh_camera_orbit(float r, float up_deg, float rot_deg, const float center[3], float eye_out[3],
                        float cam_out[16]);

/* Autofocus for the thin lens (include/jade_bvh.h): the depth, along the camera's axis, of what pixel (px, py) of the frame `params`
 * describes shows at its centre.  The pinhole ray of that pixel with both jitter draws replaced by 0.5 is traced with `trace_rays`,
 * the backend's jade_trace_rays (this library links against no backend), and *out = hit distance * 1.5 / |(left_offset, up_offset,
 * -1.5)|: what jade_lens_params.focus_distance wants.  A miss (the sky) is an error, as is a pixel outside the frame. */
typedef int (*jadeh_trace_rays_fn)(jade_scene* scene, int32_t n, const float* origins, const float* dirs, const int32_t* skip,
                                   int32_t* hit_index, float* hit_dist, float* hit_point, jade_stats* stats);
int jadeh_focus_distance(jadeh_trace_rays_fn trace_rays, jade_scene* scene, const jade_render_params* params, int px, int py,
                         float* out);

/* A second camera pose for the shutter (include/jade_bvh.h, jade_shutter_params): the pose (eye, cam) after two moves, in this order.
 * First a truck: the eye is translated by truck[3], given in camera space (x along the right column, y along the up column, z along
 * the third column, which points backwards); null = no truck.  Then a rotation by orbit_deg degrees, right-handed, about the axis
 * through pivot[3] parallel to the camera's up column: the eye and the three direction columns all turn.  pivot == null: the eye
 * itself, after the truck - a pan.  The pivot at the subject is the turntable.  Computed in double and rounded once; columns 12 .. 14
 * of cam_out carry the new eye as jadeh_camera_orbit's do.  A zero move returns the pose bit for bit.  Returns 0, or -1
 * (jadeh_last_error) on a null pose, a non-finite argument or an up column of length 0.  The outputs may alias the inputs. */
int jadeh_camera_move(const float eye[3], const float cam[16], const float truck[3], float orbit_deg, const float pivot[3],
                      float eye_out[3], float cam_out[16]);

int jadeh_write_bmp(const char* path, const uint8_t* bgr, int w, int h);
int jadeh_write_ppm(const char* path, const uint8_t* bgr, int w, int h);
int jadeh_write_pfm(const char* path, const float* rgb, int w, int h);

#ifdef __cplusplus
}
#endif
#endif /* JADE_HOST_C_H */
