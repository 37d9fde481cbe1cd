// host_capi.cpp — C entry points over the host scene pipeline, for the CLI,
// the Python bindings (ctypes) and the tests.  Declared in jade_host_c.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "jade_host.hpp"
#include "jade_host_c.h"

using namespace jadehost;

static thread_local std::string g_err;
static int fail(const std::string& m) {
  g_err = m;
  return 1;
}

struct jadeh_builder {
  SceneBuilder b;
};
struct jadeh_scene {
  BuiltScene s;
};
struct jadeh_texture {
  Texture t;
};

static Material to_mat(const jadeh_material* m) {
  Material r;
  if (!m) return r;
  memcpy(r.emissive, m->emissive, sizeof r.emissive);
  memcpy(r.brdf, m->brdf, sizeof r.brdf);
  r.reflex_mode = m->reflex_mode;
  r.refract_mode = m->refract_mode;
  memcpy(r.refract_rate, m->refract_rate, sizeof r.refract_rate);
  memcpy(r.refract_albedo, m->refract_albedo, sizeof r.refract_albedo);
  r.refract_index = m->refract_index;
  return r;
}
static Mat4 to_mat4(const float* t) {
  Mat4 r = Mat4::identity();
  if (t) memcpy(r.m, t, sizeof r.m);
  return r;
}

extern "C" {

const char* jadeh_last_error(void) { return g_err.c_str(); }

jadeh_builder* jadeh_builder_new(void) { return new jadeh_builder(); }
void jadeh_builder_free(jadeh_builder* b) { delete b; }
int jadeh_builder_triangle_count(const jadeh_builder* b) { return b ? b->b.triangle_count() : 0; }

int jadeh_builder_add_mesh(jadeh_builder* b, const float* verts, int nv, const int* idx, int nt, const jadeh_material* mat,
                           const float* trans16, int normalize) {
  if (!b || !verts || !idx || nv <= 0 || nt <= 0) return fail("add_mesh: bad arguments");
  Mesh m;
  m.vertices.resize(nv);
  for (int i = 0; i < nv; ++i) m.vertices[i] = jv(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2]);
  m.indices.assign(idx, idx + 3 * (size_t)nt);
  for (int i : m.indices)
    if (i < 0 || i >= nv) return fail("add_mesh: index out of range");
  b->b.add_mesh(m, to_mat(mat), to_mat4(trans16), normalize != 0);
  return 0;
}

static bool mesh_from(const float* verts, int nv, const int* idx, int nt, Mesh& m) {
  m.vertices.resize((size_t)nv);
  for (int i = 0; i < nv; ++i) m.vertices[i] = jv(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2]);
  m.indices.assign(idx, idx + 3 * (size_t)nt);
  for (int i : m.indices)
    if (i < 0 || i >= nv) return false;
  return true;
}

int jadeh_builder_add_mesh_uv(jadeh_builder* b, const float* verts, int nv, const int* idx, int nt, const float* uv6, const jadeh_material* mat,
                              const float* trans16, int normalize) {
  if (!b || !verts || !idx || !uv6 || nv <= 0 || nt <= 0) return fail("add_mesh_uv: bad arguments");
  Mesh m;
  if (!mesh_from(verts, nv, idx, nt, m)) return fail("add_mesh_uv: index out of range");
  m.uvs.assign(uv6, uv6 + 6 * (size_t)nt);
  b->b.add_mesh(m, to_mat(mat), to_mat4(trans16), normalize != 0);
  return 0;
}

int jadeh_builder_add_obj(jadeh_builder* b, const char* path, const jadeh_material* mat, const float* trans16, int normalize) {
  if (!b || !path) return fail("add_obj: bad arguments");
  Mesh m;
  std::string err;
  // (the vt lines are read where something will use them: a texture that is set, or a normal map - the builder's or this object's own)
  const bool wants_uvs = b->b.texture_set() || b->b.normal_map_set() || b->b.object_normal_map_set(b->b.object_count());
  if (!(wants_uvs ? load_obj_textured(path, m, err) : load_obj(path, m, err))) return fail(err);
  b->b.add_mesh(m, to_mat(mat), to_mat4(trans16), normalize != 0);
  return 0;
}

int jadeh_builder_add_proc(jadeh_builder* b, const char* kind, int param, unsigned seed, const jadeh_material* mat,
                           const float* trans16, int normalize) {
  if (!b || !kind) return fail("add_proc: bad arguments");
  std::string k = kind;
  Mesh m;
  if (k == "box") m = make_box();
  else if (k == "quad") m = make_quad(jv(-0.5f, 0, -0.5f), jv(0.5f, 0, -0.5f), jv(0.5f, 0, 0.5f), jv(-0.5f, 0, 0.5f));
  else if (k == "geodesic") m = make_geodesic(param);
  else if (k == "statue") m = make_statue(param, seed, 0);
  else if (k == "dragon") m = make_statue(param, seed, 1);
  else return fail("add_proc: unknown kind " + k);
  b->b.add_mesh(m, to_mat(mat), to_mat4(trans16), normalize != 0);
  return 0;
}

int jadeh_write_proc_obj(const char* kind, int param, unsigned seed, const char* path) {
  std::string k = kind ? kind : "";
  Mesh m;
  if (k == "box") m = make_box();
  else if (k == "quad") m = make_quad(jv(-0.5f, 0, -0.5f), jv(0.5f, 0, -0.5f), jv(0.5f, 0, 0.5f), jv(-0.5f, 0, 0.5f));
  else if (k == "geodesic") m = make_geodesic(param);
  else if (k == "statue") m = make_statue(param, seed, 0);
  else if (k == "dragon") m = make_statue(param, seed, 1);
  else return fail("write_proc_obj: unknown kind " + k);
  return write_obj(path, m) ? 0 : fail(std::string("cannot write ") + path);
}

int jadeh_builder_set_smoothing(jadeh_builder* b, float crease_deg) {
  if (!b) return fail("null builder");
  if (!(crease_deg == crease_deg)) return fail("set_smoothing: the angle is not a number");
  b->b.set_smoothing(crease_deg);
  return 0;
}
int jadeh_vertex_normals(const float* verts, int nv, const int* idx, int nt, float crease_deg, float* out9) {
  if (!verts || !idx || !out9 || nv < 0 || nt < 0) return fail("vertex_normals: bad arguments");
  Mesh m;
  m.vertices.resize((size_t)nv);
  for (int i = 0; i < nv; ++i) m.vertices[i] = jv(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2]);
  for (int i = 0; i < 3 * nt; ++i) {
    if (idx[i] < 0 || idx[i] >= nv) return fail("vertex_normals: index out of range");
    m.indices.push_back(idx[i]);
  }
  const std::vector<float> vn = vertex_normals(m, crease_deg);
  if (!vn.empty()) memcpy(out9, vn.data(), vn.size() * sizeof(float));
  return 0;
}
static jadeh_texture* texture_fail(const std::string& m) {
  fail(m);
  return nullptr;
}
jadeh_texture* jadeh_texture_load(const char* path) {
  if (!path) return texture_fail("texture_load: bad arguments");
  FILE* f = fopen(path, "rb");
  if (!f) return texture_fail(std::string("File ") + path + " open failed.");
  char magic[2] = {0, 0};
  const size_t got = fread(magic, 1, 2, f);
  fclose(f);
  jadeh_texture* t = new jadeh_texture();
  std::string err;
  const bool pfm = got == 2 && magic[0] == 'P' && magic[1] == 'F';
  if (!(pfm ? load_pfm(path, t->t, err) : load_ppm(path, t->t, err))) {
    delete t;
    return texture_fail(err);
  }
  return t;
}
jadeh_texture* jadeh_texture_checker(int size, int squares, const float a[3], const float b[3]) {
  if (!a || !b || size < 1 || size > 16384 || squares < 1) return texture_fail("texture_checker: bad arguments");
  jadeh_texture* t = new jadeh_texture();
  t->t = make_texture_checker(size, squares, a, b);
  return t;
}
jadeh_texture* jadeh_texture_data(int width, int height, const float* rgb) {
  if (!rgb || width < 1 || width > 16384 || height < 1 || height > 16384) return texture_fail("texture_data: bad arguments");
  jadeh_texture* t = new jadeh_texture();
  t->t.width = width;
  t->t.height = height;
  t->t.rgb.assign(rgb, rgb + (size_t)3 * width * height);
  return t;
}
void jadeh_texture_free(jadeh_texture* t) { delete t; }
int jadeh_texture_get(const jadeh_texture* t, int* width, int* height, const float** rgb) {
  if (!t || !width || !height || !rgb) return fail("texture_get: bad arguments");
  *width = t->t.width;
  *height = t->t.height;
  *rgb = t->t.rgb.data();
  return 0;
}
int jadeh_builder_set_texture(jadeh_builder* b, const jadeh_texture* t, int projection) {
  if (!b) return fail("null builder");
  if (projection < 0 || projection > 3) return fail("set_texture: projection is 0 1 2 (planar along x y z) or 3 (spherical)");
  b->b.set_texture(t ? &t->t : nullptr, (UvProjection)projection);
  return 0;
}
int jadeh_builder_set_object_texture(jadeh_builder* b, int object, const jadeh_texture* t, int projection) {
  if (!b || !t || object < 0) return fail("set_object_texture: bad arguments");
  if (projection < 0 || projection > 3) return fail("set_object_texture: projection is 0 1 2 (planar along x y z) or 3 (spherical)");
  b->b.set_object_texture(object, t->t, (UvProjection)projection);
  return 0;
}
jadeh_texture* jadeh_normal_map_load(const char* path) {
  if (!path) return texture_fail("normal_map_load: bad arguments");
  jadeh_texture* t = new jadeh_texture();
  std::string err;
  if (!load_normal_map(path, t->t, err)) {
    delete t;
    return texture_fail(err);
  }
  return t;
}
jadeh_texture* jadeh_height_to_normal_map(int width, int height, const float* heights, float scale) {
  if (!heights || width < 1 || width > 16384 || height < 1 || height > 16384 || !std::isfinite(scale)) return texture_fail("height_to_normal_map: bad arguments");
  jadeh_texture* t = new jadeh_texture();
  t->t = height_to_normal_map(heights, width, height, scale);
  return t;
}
static bool strength_ok(float s) { return s >= 0.0f && std::isfinite(s); }
int jadeh_builder_set_normal_map(jadeh_builder* b, const jadeh_texture* t, int projection, float strength) {
  if (!b) return fail("null builder");
  if (projection < 0 || projection > 3) return fail("set_normal_map: projection is 0 1 2 (planar along x y z) or 3 (spherical)");
  if (!strength_ok(strength)) return fail("set_normal_map: the strength is finite and >= 0");
  b->b.set_normal_map(t ? &t->t : nullptr, (UvProjection)projection, strength);
  return 0;
}
int jadeh_builder_set_object_normal_map(jadeh_builder* b, int object, const jadeh_texture* t, int projection, float strength) {
  if (!b || !t || object < 0) return fail("set_object_normal_map: bad arguments");
  if (projection < 0 || projection > 3) return fail("set_object_normal_map: projection is 0 1 2 (planar along x y z) or 3 (spherical)");
  if (!strength_ok(strength)) return fail("set_object_normal_map: the strength is finite and >= 0");
  b->b.set_object_normal_map(object, t->t, (UvProjection)projection, strength);
  return 0;
}
int jadeh_project_uvs(const float* verts, int nv, const int* idx, int nt, int projection, float* out6) {
  if (!verts || !idx || !out6 || nv < 0 || nt < 0 || projection < 0 || projection > 3) return fail("project_uvs: bad arguments");
  Mesh m;
  if (!mesh_from(verts, nv, idx, nt, m)) return fail("project_uvs: index out of range");
  const std::vector<float> uv = projection == 3 ? spherical_uvs(m) : planar_uvs(m, projection);
  if (!uv.empty()) memcpy(out6, uv.data(), uv.size() * sizeof(float));
  return 0;
}
int jadeh_load_obj_textured(const char* path, int* nv, int* nt, int* has_uv, float* verts, int* idx, float* uv6) {
  if (!path || !nv || !nt || !has_uv) return fail("load_obj_textured: bad arguments");
  Mesh m;
  std::string err;
  if (!load_obj_textured(path, m, err)) return fail(err);
  *nv = (int)m.vertices.size();
  *nt = (int)(m.indices.size() / 3);
  *has_uv = m.uvs.empty() ? 0 : 1;
  if (verts)
    for (size_t i = 0; i < m.vertices.size(); ++i) {
      verts[3 * i] = m.vertices[i].x;
      verts[3 * i + 1] = m.vertices[i].y;
      verts[3 * i + 2] = m.vertices[i].z;
    }
  if (idx) std::copy(m.indices.begin(), m.indices.end(), idx);
  if (uv6)
    for (size_t i = 0; i < m.indices.size() * 2; ++i) uv6[i] = m.uvs.empty() ? 0.0f : m.uvs[i];
  return 0;
}
int jadeh_builder_set_env_constant(jadeh_builder* b, float r, float g, float bl) {
  if (!b) return fail("null builder");
  b->b.set_env(make_env_constant(r, g, bl));
  return 0;
}
int jadeh_builder_set_env_sky(jadeh_builder* b, int w, int h) {
  if (!b || w <= 0 || h <= 0) return fail("set_env_sky: bad arguments");
  b->b.set_env(make_env_sky(w, h));
  return 0;
}
int jadeh_builder_set_env_data(jadeh_builder* b, int w, int h, const float* rgb) {
  if (!b || w <= 0 || h <= 0 || !rgb) return fail("set_env_data: bad arguments");
  EnvMap e;
  e.width = w;
  e.height = h;
  e.rgb.assign(rgb, rgb + (size_t)3 * w * h);
  b->b.set_env(std::move(e));
  return 0;
}
int jadeh_builder_set_env_hdr(jadeh_builder* b, const char* path) {
  if (!b || !path) return fail("set_env_hdr: bad arguments");
  EnvMap e;
  std::string err;
  if (!load_hdr(path, e, err)) return fail(err);
  b->b.set_env(std::move(e));
  return 0;
}

int jadeh_builder_config(jadeh_builder* b, const char* name, jadeh_config* out) {
  if (!b || !name || !out) return fail("config: bad arguments");
  Config c;
  std::string err;
  if (!make_config(name, b->b, c, err)) return fail(err);
  out->width = c.width;
  out->height = c.height;
  out->spp = c.spp;
  memcpy(out->eye, c.eye, sizeof c.eye);
  memcpy(out->camera, c.camera, sizeof c.camera);
  return 0;
}

int jadeh_builder_load_render_args(jadeh_builder* b, const char* path, jadeh_config* out) {
  if (!b || !path || !out) return fail("load_render_args: bad arguments");
  RenderArgs ra;
  std::string err;
  if (!read_render_args(path, ra, err)) return fail(err);
  std::string dir = path;
  size_t slash = dir.find_last_of('/');
  dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
  for (const RenderArgsObject& o : ra.objects) {
    Mesh m;
    std::string file = (!o.file.empty() && o.file[0] == '/') ? o.file : dir + o.file;
    if (!load_obj(file, m, err)) return fail(err);
    b->b.add_mesh(m, o.material, o.trans, o.normalize);
  }
  memset(out, 0, sizeof *out);
  memcpy(out->eye, ra.eye, sizeof ra.eye);
  memcpy(out->camera, ra.camera, sizeof ra.camera);
  return 0;
}

jadeh_scene* jadeh_builder_build(jadeh_builder* b, int leaf_size) {
  if (!b || b->b.triangle_count() == 0) {
    fail("build: empty scene");
    return nullptr;
  }
  jadeh_scene* s = new jadeh_scene();
  s->s = b->b.build(leaf_size > 0 ? leaf_size : 8);
  return s;
}
int jadeh_builder_triangles(const jadeh_builder* b, jade_triangle* out, int capacity) {
  if (!b || !out) return fail("builder_triangles: bad arguments");
  std::vector<jade_triangle> v = b->b.triangles_original();
  if ((int)v.size() > capacity) return fail("builder_triangles: buffer too small");
  memcpy(out, v.data(), v.size() * sizeof(jade_triangle));
  return 0;
}

jadeh_scene* jadeh_builder_build_with_bvh(jadeh_builder* b, const int32_t* order, const jade_bvh_node* nodes, int n_nodes) {
  if (!b || b->b.triangle_count() == 0) {
    fail("build_with_bvh: empty scene");
    return nullptr;
  }
  jadeh_scene* s = new jadeh_scene();
  std::string err;
  if (!b->b.build_with_bvh(order, nodes, n_nodes, s->s, err)) {
    fail(err);
    delete s;
    return nullptr;
  }
  return s;
}

void jadeh_scene_free(jadeh_scene* s) { delete s; }
void jadeh_scene_desc(const jadeh_scene* s, jade_scene_desc* out) {
  if (s && out) *out = s->s.desc();
}
int jadeh_scene_vertex_normals(const jadeh_scene* s, const float** out) {
  if (!s) return 0;
  if (out) *out = s->s.vertex_normals.empty() ? nullptr : s->s.vertex_normals.data();
  return (int)(s->s.vertex_normals.size() / 9);
}
int jadeh_scene_textures(const jadeh_scene* s, const float** uv, const int32_t** image_of) {
  if (!s) return 0;
  if (uv) *uv = s->s.uv.empty() ? nullptr : s->s.uv.data();
  if (image_of) *image_of = s->s.image_of.empty() ? nullptr : s->s.image_of.data();
  return (int)s->s.textures.size();
}
int jadeh_scene_texture(const jadeh_scene* s, int k, int* width, int* height, const float** rgb) {
  if (!s || !width || !height || !rgb || k < 0 || k >= (int)s->s.textures.size()) return fail("scene_texture: bad arguments");
  *width = s->s.textures[k].width;
  *height = s->s.textures[k].height;
  *rgb = s->s.textures[k].rgb.data();
  return 0;
}
int jadeh_scene_normal_maps(const jadeh_scene* s, const float** uv, const int32_t** image_of, float* strength) {
  if (!s) return 0;
  if (uv) *uv = s->s.map_uv.empty() ? nullptr : s->s.map_uv.data();
  if (image_of) *image_of = s->s.map_image_of.empty() ? nullptr : s->s.map_image_of.data();
  if (strength) *strength = s->s.map_strength;
  return (int)s->s.normal_maps.size();
}
int jadeh_scene_normal_map(const jadeh_scene* s, int k, int* width, int* height, const float** xyz) {
  if (!s || !width || !height || !xyz || k < 0 || k >= (int)s->s.normal_maps.size()) return fail("scene_normal_map: bad arguments");
  *width = s->s.normal_maps[k].width;
  *height = s->s.normal_maps[k].height;
  *xyz = s->s.normal_maps[k].rgb.data();
  return 0;
}
int jadeh_scene_bvh_depth(const jadeh_scene* s) { return s ? s->s.bvh_depth : 0; }
double jadeh_scene_build_seconds(const jadeh_scene* s) { return s ? s->s.build_seconds : 0; }

void jadeh_transform_matrix(const float rot_deg[3], const float trans[3], const float scale[3], float out16[16]) {
  Mat4 m = transform_matrix(rot_deg, trans, scale);
  memcpy(out16, m.m, sizeof m.m);
}
void jadeh_camera_orbit(float r, float up_deg, float rot_deg, const float center[3], float eye_out[3], float cam_out[16]) {
  camera_orbit(r, up_deg, rot_deg, center, eye_out, cam_out);
}

int jadeh_focus_distance(jadeh_trace_rays_fn trace_rays, jade_scene* scene, const jade_render_params* p, int px, int py, float* out) {
  if (!trace_rays || !scene || !p || !out) return fail("focus_distance: bad arguments");
  if (p->width <= 0 || p->height <= 0 || px < 0 || py < 0 || px >= p->width || py >= p->height) return fail("focus_distance: pixel outside the frame");
  // the camera ray's statements (PathTrace.cu:1428-1437) with 0.5 for both jitter draws
  const double aspect = (double)p->width / (double)p->height;
  const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
  const float left_offset = (float)((-1.0 + 2.0 / (double)p->width * ((double)fx - 0.5)) * aspect);
  const float up_offset = (float)(-1.0 + 2.0 / (double)p->height * ((double)fy - 0.5));
  const jvec3 d = jv_normalize(jade_transform(jv(left_offset, up_offset, -1.5f), 0.0f, p->camera));
  const float o3[3] = {p->eye[0], p->eye[1], p->eye[2]}, d3[3] = {d.x, d.y, d.z};
  const int32_t skip = -1;
  int32_t hit = -1;
  float dist = 0.0f, point[3] = {0, 0, 0};
  jade_stats st;
  memset(&st, 0, sizeof st);
  if (trace_rays(scene, 1, o3, d3, &skip, &hit, &dist, point, &st) != JADE_OK) return fail("focus_distance: jade_trace_rays failed");
  if (hit < 0) return fail("focus_distance: pixel (" + std::to_string(px) + ", " + std::to_string(py) + ") sees no surface");
  const double len = std::sqrt((double)left_offset * left_offset + (double)up_offset * up_offset + 2.25);
  *out = (float)((double)dist * 1.5 / len);
  return 0;
}

int jadeh_camera_move(const float eye[3], const float cam[16], const float truck[3], float orbit_deg, const float pivot[3], float eye_out[3],
                      float cam_out[16]) {
  if (!eye || !cam || !eye_out || !cam_out) return fail("camera_move: bad arguments");
  bool finite = std::isfinite(orbit_deg);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(eye[i]) && (!truck || std::isfinite(truck[i])) && (!pivot || std::isfinite(pivot[i]));
  for (int j = 0; j < 16; ++j) finite = finite && std::isfinite(cam[j]);
  if (!finite) return fail("camera_move: non-finite argument");
  double e[3], col[3][3], a[3];
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) col[c][r] = cam[4 * c + r];
  const double ulen = std::sqrt(col[1][0] * col[1][0] + col[1][1] * col[1][1] + col[1][2] * col[1][2]);
  if (!(ulen > 0.0)) return fail("camera_move: the camera's up column has length 0");
  for (int r = 0; r < 3; ++r) a[r] = col[1][r] / ulen;
  // the truck, in camera space
  const bool trucked = truck && (truck[0] != 0.0f || truck[1] != 0.0f || truck[2] != 0.0f);  // (a zero move returns the pose bit for bit, a -0 included)
  for (int r = 0; r < 3; ++r) e[r] = trucked ? (double)eye[r] + (col[0][r] * truck[0] + col[1][r] * truck[1] + col[2][r] * truck[2]) : (double)eye[r];
  // the rotation about the axis through the pivot (Rodrigues): v cos + (a x v) sin + a (a . v) (1 - cos)
  const double th = (double)orbit_deg * 0.017453292519943295;
  const double cs = std::cos(th), sn = std::sin(th);
  auto rotate = [&](const double v[3], double out[3]) {
    if (orbit_deg == 0.0f) {
      for (int r = 0; r < 3; ++r) out[r] = v[r];
      return;
    }
    const double d = a[0] * v[0] + a[1] * v[1] + a[2] * v[2];
    const double x[3] = {a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]};
    for (int r = 0; r < 3; ++r) out[r] = v[r] * cs + x[r] * sn + a[r] * d * (1.0 - cs);
  };
  double rel[3], turned[3], centre[3];
  for (int r = 0; r < 3; ++r) centre[r] = pivot ? (double)pivot[r] : e[r];
  for (int r = 0; r < 3; ++r) rel[r] = e[r] - centre[r];
  rotate(rel, turned);
  float m[16];
  memcpy(m, cam, sizeof m);
  for (int c = 0; c < 3; ++c) {
    double t[3];
    rotate(col[c], t);
    for (int r = 0; r < 3; ++r) m[4 * c + r] = (float)t[r];
  }
  for (int r = 0; r < 3; ++r) {
    eye_out[r] = orbit_deg == 0.0f ? (float)e[r] : (float)(centre[r] + turned[r]);
    m[12 + r] = eye_out[r];
  }
  memcpy(cam_out, m, sizeof m);
  return 0;
}

int jadeh_write_bmp(const char* path, const uint8_t* bgr, int w, int h) { return write_bmp(path, bgr, w, h) ? 0 : fail("write_bmp failed"); }
int jadeh_write_ppm(const char* path, const uint8_t* bgr, int w, int h) { return write_ppm(path, bgr, w, h) ? 0 : fail("write_ppm failed"); }
int jadeh_write_pfm(const char* path, const float* rgb, int w, int h) { return write_pfm(path, rgb, w, h) ? 0 : fail("write_pfm failed"); }

}  // extern "C"
