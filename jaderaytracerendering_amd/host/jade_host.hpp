// jade_host.hpp — host-side scene pipeline (the repo's own C++).
//
// Everything ABOVE the drop-in boundary of include/jade_rt.h: mesh loading and
// procedural stand-ins for the git-ignored reference assets, the reference's
// SAH BVH conventions, scene flattening into the boundary's arrays, camera,
// environment map, image writers and the render_args.txt hand-off file.
// Mirrors the roles of PathTrace.cu:355-628, 1487-1612 and
// PathTrace.cpp:343-359, 684-687, 883-918 without sharing their code.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "jade_fpmath.h"
#include "jade_rt.h"

namespace jadehost {

// == Material, PathTrace.cu:293-301
struct Material {
  float emissive[3] = {0, 0, 0};
  float brdf[3] = {0.8f, 0.8f, 0.8f};
  int reflex_mode = JADE_DIFFUSE;
  int refract_mode = JADE_NO_REFRACT;
  float refract_rate[3] = {0.8f, 0.8f, 0.8f};
  float refract_albedo[3] = {0.8f, 0.8f, 0.8f};
  float refract_index = 1.0f;
};

struct Mat4 {
  float m[16];  // [col][row] memory order, like glm and camera_transform_dv
  static Mat4 identity();
};
Mat4 mul(const Mat4& a, const Mat4& b);
// getTransformMatrix(rotateCtrl(deg), translateCtrl, scaleCtrl) = T * Rx * Ry * Rz * S
// (PathTrace.cpp:343-359)
Mat4 transform_matrix(const float rot_deg[3], const float trans[3], const float scale[3]);

struct Mesh {
  std::vector<jvec3> vertices;
  std::vector<int> indices;  // 3 per triangle, 0-based
  std::vector<float> uvs;    // optional: 6 per triangle - (u, v) of its three corners, in the order of its indices; empty: the mesh has none
};

// -- mesh sources -----------------------------------------------------------
// readObj's parser (PathTrace.cu:378-408): '#' lines skipped, '/' -> ' ',
// "v x y z", "f a b c" (first three integers only).
bool load_obj(const std::string& path, Mesh& out, std::string& err);
// An OBJ file with texture coordinates: "v x y z", "vt u v" and "f a/b[/c] ..." (the first three corners only; a corner without a `vt`
// index, or with one out of range, gets (0, 0)).  out.uvs is filled when the file has a `vt` line.  load_obj above - the reference's
// parser, with its way of reading a '/' - stays what every existing caller uses.
bool load_obj_textured(const std::string& path, Mesh& out, std::string& err);
bool write_obj(const std::string& path, const Mesh& mesh);
Mesh make_quad(jvec3 a, jvec3 b, jvec3 c, jvec3 d);
Mesh make_box();                     // unit cube centred at 0, 12 triangles
Mesh make_geodesic(int freq);        // unit sphere, 20*freq^2 triangles, shared vertices
// Closed star-shaped "jade statue" stand-in: geodesic sphere displaced by a
// seeded multi-octave field.  style 0 = upright statue, 1 = elongated "dragon".
Mesh make_statue(int freq, uint32_t seed, int style);
void append(Mesh& dst, const Mesh& src);
// Vertex normals for smooth shading (include/jade_bvh.h, jade_scene_set_vertex_normals): 9 floats per triangle, corners in the order of its
// indices.  A corner's normal is the sum, over the mesh's triangles that share its vertex INDEX and whose flat normal is within
// crease_deg of this triangle's, of those flat normals, each weighted by its triangle's interior angle at the vertex; formed in double
// from the fp32 flat normals (add_mesh's own statement), normalised, rounded once.  crease_deg <= 0, or a corner nothing but its own
// triangle contributes to, or one whose contributors all have this triangle's flat normal (component by component, -0 = 0), or a sum without a direction: the
// flat normal, bitwise.
std::vector<float> vertex_normals(const Mesh& mesh, float crease_deg);

// -- albedo textures (include/jade_bvh.h, jade_scene_set_textures) -----------
// UVs for a mesh that has none, 6 floats per triangle, formed in double from the mesh's own (untransformed) vertices and rounded once.
// planar_uvs: the two coordinates other than `axis` (0 x, 1 y, 2 z; in cyclic order: y z, z x, x y), each mapped from the mesh's bounding
// box to [0, 1] (an extent of 0: 0).  spherical_uvs: about the centre of the bounding box, u = 0.5 + atan2(z, x) / 2 pi, v = 0.5 -
// asin(y / r) / pi (v = 0 at the top, where the image's row 0 is); a triangle that crosses the seam u = 0 | 1 has 1 added to its corners
// below 0.5 - the image repeats - and a corner at a pole takes the mean u of the other two.
std::vector<float> planar_uvs(const Mesh& mesh, int axis);
std::vector<float> spherical_uvs(const Mesh& mesh);
enum UvProjection { UV_PLANAR_X = 0, UV_PLANAR_Y = 1, UV_PLANAR_Z = 2, UV_SPHERICAL = 3 };

struct Texture {
  int width = 0, height = 0;
  std::vector<float> rgb;  // linear, interleaved, row 0 at v = 0 (the top of an image file)
};
// P6, 8 bits per channel: sRGB decoded in double - c / 12.92 up to 0.04045, ((c + 0.055) / 1.055)^2.4 above, c = byte / 255 - and rounded once.
bool load_ppm(const std::string& path, Texture& out, std::string& err);
// PF: linear values as stored - the sign of the header's scale gives the byte order, its magnitude is ignored; the file's rows run bottom
// to top and are flipped, so that row 0 is the top.
bool load_pfm(const std::string& path, Texture& out, std::string& err);
// size x size texels in squares x squares squares of colours a and b, (0, 0) being a
Texture make_texture_checker(int size, int squares, const float a[3], const float b[3]);

// -- normal maps (include/jade_bvh.h, jade_scene_set_normal_maps) -------------
// A map is a Texture of tangent-space vectors (x, y, z), decoded.  load_normal_map: a P6 file read LINEARLY - no sRGB decode - and then
// 2 c - 1 per channel, c = byte / 255, in double and rounded once; a PF file as given (load_pfm).
bool load_normal_map(const std::string& path, Texture& out, std::string& err);
// width x height heights (row 0 at v = 0) -> the map of the surface z = scale * height(u, v): central differences in u and v over the
// neighbouring texels, the image repeating at its borders - dh/du = (h(i + 1, j) - h(i - 1, j)) * (W / 2), dh/dv the same with H - in
// fp32, and the UNNORMALISED vector (0 - scale * dh/du, 0 - scale * dh/dv, 1): a constant height gives (0, 0, 1) exactly.
Texture height_to_normal_map(const float* height, int width, int height_texels, float scale);

// -- scene builder (host triangles, pre-BVH) -------------------------------
struct HostTriangle {  // == Triangle, PathTrace.cu:305-311
  int index;
  int obj_idx;
  jvec3 p1, p2, p3, norm;
  Material material;
};

struct EnvMap {
  int width = 0, height = 0;
  std::vector<float> rgb;  // interleaved, row 0 = top
};
EnvMap make_env_constant(float r, float g, float b);
EnvMap make_env_sky(int width, int height);  // gradient + sun lobe, values in [0, 10]
bool load_hdr(const std::string& path, EnvMap& out, std::string& err);  // Radiance RGBE

struct BuiltScene {
  std::vector<jade_triangle> triangles;  // BVH order
  std::vector<jade_bvh_node> nodes;      // [0] dummy, [1] root
  std::vector<int32_t> emit;
  std::vector<int32_t> mapping;          // original -> sorted
  std::vector<float> prefix;             // original order
  std::vector<jade_obj_seg> segs;
  std::vector<float> vertex_normals;     // 9 per triangle, BVH order: what jade_scene_set_vertex_normals takes; empty if no mesh was smoothed
  // what jade_scene_set_textures takes, BVH order: 6 floats of UV and an image number (-1: none) per triangle, and the images; empty if no mesh was textured
  std::vector<float> uv;
  std::vector<int32_t> image_of;
  std::vector<Texture> textures;
  // ... and what jade_scene_set_normal_maps takes, the same way: the map's own UVs and image numbers, its images and the strength
  std::vector<float> map_uv;
  std::vector<int32_t> map_image_of;
  std::vector<Texture> normal_maps;
  float map_strength = 1.0f;
  EnvMap env;
  int bvh_depth = 0;
  double build_seconds = 0;
  jade_scene_desc desc() const;
};

class SceneBuilder {
 public:
  // The body of readObj after parsing (PathTrace.cu:410-456): optional
  // normalise-to-unit (with the reference's max/min quirk, :399-400, :411-423),
  // 4x4 transform, flat normals, one object segment.
  void add_mesh(const Mesh& mesh, const Material& mat, const Mat4& trans, bool normalize);
  void set_env(EnvMap env) { env_ = std::move(env); }
  // The smoothing angle of the meshes added from now on (degrees; <= 0: flat, the default): add_mesh forms their vertex normals with
  // vertex_normals(), after the mesh's transform.  load_obj reads no `vn` lines: normals come from the geometry alone.
  void set_smoothing(float crease_deg) { smooth_deg_ = crease_deg; }
  // The texture of the meshes added from now on (nullptr: none, the default): add_mesh gives their triangles the image and the mesh's own
  // UVs or, where it has none, those of `fallback` - formed from the mesh as given, before normalize and the transform.
  void set_texture(const Texture* texture, UvProjection fallback = UV_SPHERICAL);
  bool texture_set() const { return texture_ >= 0; }
  // ... and the texture of the object'th mesh to be added (0-based, in the order of the add_mesh calls), whatever set_texture says when it
  // arrives: how a caller textures one object of a configuration it does not build itself (jade_render --texture).
  void set_object_texture(int object, const Texture& texture, UvProjection fallback = UV_SPHERICAL);
  bool object_texture_set(int object) const { return object_texture_.count(object) != 0; }
  // The normal map of the meshes added from now on, and of the object'th mesh to be added: as set_texture and set_object_texture, with
  // the mesh's own UVs or those of `fallback`, independent of the albedo texture's.  The table has ONE strength: the last one given.
  void set_normal_map(const Texture* map, UvProjection fallback = UV_SPHERICAL, float strength = 1.0f);
  void set_object_normal_map(int object, const Texture& map, UvProjection fallback = UV_SPHERICAL, float strength = 1.0f);
  bool normal_map_set() const { return map_ >= 0; }
  bool object_normal_map_set(int object) const { return object_map_.count(object) != 0; }
  int object_count() const { return (int)segs_.size(); }
  int triangle_count() const { return (int)tris_.size(); }
  // Area prefix sums (PathTrace.cu:1539-1546), SAH BVH with leaf size 8
  // (:1557-1565), encode (:1570-1612).
  BuiltScene build(int leaf_size = 8) const;
  // The same flattening around a BVH built elsewhere (e.g. jade_bvh_build_lbvh on the GPU):
  // `order[i]` = original index of the triangle at sorted position i, `nodes` in the reference's
  // conventions.  triangles_original() is what such a builder takes as input.
  std::vector<jade_triangle> triangles_original() const;
  bool build_with_bvh(const int32_t* order, const jade_bvh_node* nodes, int n_nodes, BuiltScene& out, std::string& err) const;

 private:
  void finish(std::vector<HostTriangle>& sorted, BuiltScene& out) const;
  std::vector<HostTriangle> tris_;
  std::vector<jade_obj_seg> segs_;
  std::vector<float> vnorm_;  // 9 per triangle of tris_, original order; empty until a mesh is smoothed
  float smooth_deg_ = 0.0f;
  std::vector<float> uv_;          // 6 per triangle of tris_, original order; empty until a mesh is textured
  std::vector<int32_t> image_of_;  // ... and its image, -1 for none
  std::vector<Texture> textures_;
  int texture_ = -1;               // set_texture: the image of the meshes to come
  UvProjection fallback_ = UV_SPHERICAL;
  std::map<int, std::pair<int, UvProjection>> object_texture_;  // set_object_texture: object -> (its image in textures_, its fallback)
  std::vector<float> map_uv_;          // the normal maps, member for member as the textures above
  std::vector<int32_t> map_image_of_;
  std::vector<Texture> maps_;
  int map_ = -1;
  UvProjection map_fallback_ = UV_SPHERICAL;
  std::map<int, std::pair<int, UvProjection>> object_map_;
  float map_strength_ = 1.0f;
  EnvMap env_;
};

// buildBVHwithSAH conventions (PathTrace.cu:497-628): reorders `tris`.
void build_bvh_sah(std::vector<HostTriangle>& tris, std::vector<jade_bvh_node>& nodes, int leaf_size);
int bvh_depth(const std::vector<jade_bvh_node>& nodes);

// -- camera (PathTrace.cpp:209-211, 684-687) ---------------------------------
// eye on the sphere of radius r around `center`, camera = inverse(lookAt).
void camera_orbit(float r, float up_angle_deg, float rotate_angle_deg, const float center[3], float eye_out[3],
                  float cam_out[16]);

// -- render_args.txt (writer PathTrace.cpp:883-918, reader PathTrace.cu:1487-1525)
struct RenderArgsObject {
  std::string file;
  Mat4 trans;
  Material material;
  bool normalize = false;
};
struct RenderArgs {
  float eye[3];
  float camera[16];
  std::vector<RenderArgsObject> objects;
};
bool read_render_args(const std::string& path, RenderArgs& out, std::string& err);
bool write_render_args(const std::string& path, const RenderArgs& in);

// -- image output -------------------------------------------------------------
// save_image (PathTrace.cu:74-106): 24-bit BMP, BGR, bottom-up, rows unpadded.
bool write_bmp(const std::string& path, const uint8_t* bgr, int width, int height);
bool write_ppm(const std::string& path, const uint8_t* bgr, int width, int height);  // P6, top-down RGB
bool write_pfm(const std::string& path, const float* rgb, int width, int height);    // PF, bottom-up

// -- built-in benchmark configurations (C1..C5, plus "tiny") ----
struct Config {
  std::string name;
  int width = 0, height = 0, spp = 0;
  float eye[3];
  float camera[16];
};
bool make_config(const std::string& name, SceneBuilder& builder, Config& cfg, std::string& err);

}  // namespace jadehost
