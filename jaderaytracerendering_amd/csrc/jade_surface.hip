// jade_surface.hip — the surface tables of a scene handle (SurfaceTables, jade_runtime.h): vertex normals, textures, normal maps.  Host code
// only, no kernel: the setters and getters of include/jade_bvh.h, the one check of an image set they share, and surface_begin, which is what
// jade_render_begin does about the tables.  The records themselves are made by jade_smooth.h, jade_texture.h and jade_normal_map.h.
#include <cmath>
#include <cstring>

#include "jade_runtime.h"
#include "jade_smooth.h"

// The scene's triangles as the handle holds them, copied back from the device: every table's records are made from them.
static int scene_triangles(jade_scene* s, std::vector<jade_triangle>* tris) {
  HIP_TRY(hipSetDevice(s->device));
  tris->resize((size_t)s->dev.n_tris);
  HIP_TRY(hipMemcpyAsync(tris->data(), s->b_tris.p, sizeof(jade_triangle) * tris->size(), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

static void clear_images(SurfaceImages* im) {
  for (auto* v : {&im->rec, &im->texels}) {
    v->clear();
    v->shrink_to_fit();
  }
  im->images.clear();
  im->any = false;
}

int surface_check_images(const char* who, int32_t n_images, const jade_texture_image* images, const int32_t* image_of, int32_t n_triangles,
                         int32_t n_scene, std::vector<uint4>* heads, std::vector<float4>* texels, bool* any) {
  const std::string w(who);
  if (n_images < 0 || n_images > JADE_TEX_MAX_IMAGES)
    return jade_fail(JADE_ERR_INVALID, w + std::to_string(n_images) + " images (at most " + std::to_string(JADE_TEX_MAX_IMAGES) + ")");
  if (n_triangles != n_scene) return jade_fail(JADE_ERR_INVALID, w + "the triangle count " + std::to_string(n_triangles) + " is not the scene's");
  heads->assign((size_t)n_images, make_uint4(0u, 0u, 0u, 0u));
  size_t total = 0;
  for (int32_t k = 0; k < n_images; ++k) {
    const jade_texture_image& im = images[k];
    if (im.width < 1 || im.width > JADE_TEX_MAX_SIZE || im.height < 1 || im.height > JADE_TEX_MAX_SIZE)
      return jade_fail(JADE_ERR_INVALID, w + "image " + std::to_string(k) + " is " + std::to_string(im.width) + " x " + std::to_string(im.height) +
                                             " (a width and a height of 1 .. " + std::to_string(JADE_TEX_MAX_SIZE) + ")");
    if (!im.rgb) return jade_fail(JADE_ERR_INVALID, w + "image " + std::to_string(k) + " has no texels");
    (*heads)[k] = make_uint4((uint32_t)(total & 0xffffffffu), (uint32_t)(total >> 32), (uint32_t)im.width, (uint32_t)im.height);
    total += (size_t)im.width * (size_t)im.height;
  }
  *any = false;
  for (int32_t t = 0; t < n_triangles; ++t) {
    if (image_of[t] < -1 || image_of[t] >= n_images)
      return jade_fail(JADE_ERR_INVALID, w + "image_of[" + std::to_string(t) + "] = " + std::to_string(image_of[t]) + " is outside -1 .. " + std::to_string(n_images - 1));
    *any = *any || image_of[t] >= 0;
  }
  texels->assign(total, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  for (int32_t k = 0; k < n_images; ++k) {
    const uint4 hd = (*heads)[k];
    const size_t first = ((size_t)hd.y << 32) | hd.x, n = (size_t)hd.z * hd.w;
    const float* rgb = images[k].rgb;
    for (size_t i = 0; i < n; ++i) {
      if (!std::isfinite(rgb[3 * i]) || !std::isfinite(rgb[3 * i + 1]) || !std::isfinite(rgb[3 * i + 2]))
        return jade_fail(JADE_ERR_INVALID, w + "image " + std::to_string(k) + " has a texel that is not finite at (" + std::to_string(i % hd.z) + ", " +
                                               std::to_string(i / hd.z) + ")");
      (*texels)[first + i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
    }
  }
  return JADE_OK;
}

// The normal maps' records as the setter left them, joined with the vertex normals the handle has now (jade_normal_map.h: a mapped vertex reads
// the normal it bends from the map's own record) ...
std::vector<float4> surface_join_maps(const SurfaceTables& t) {
  std::vector<float4> rec(t.set.maps.rec);
  const size_t n = rec.size() / JADE_NMAP_REC;
  for (size_t i = 0; i < n; ++i) normal_map_join(&rec[i * JADE_NMAP_REC], t.set.normals_any ? &t.set.normals[i * JADE_SMOOTH_REC] : nullptr);
  return rec;
}
// ... so new vertex normals make the joined records on the device stale as well as their own buffer: the one place that says so
static void normals_changed(SurfaceTables* t) {
  t->dev.normals_current = false;
  t->dev.maps_current = false;
}

// The vertex normals of the scene handle (include/jade_bvh.h, "The shading normal, stated"): the table's records (jade_smooth.h) are made here,
// from the triangles as the handle holds them, and uploaded by the next jade_render_begin - a render in progress keeps the table it began with.
int jade_scene_set_vertex_normals(jade_scene* s, const float* normals, int32_t n_triangles) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  SurfaceTables& T = s->surf;
  if (!normals) {
    T.set.normals.clear();
    T.set.normals.shrink_to_fit();
    T.set.normals_any = false;
    normals_changed(&T);
    return JADE_OK;
  }
  if (n_triangles != s->dev.n_tris) return jade_fail(JADE_ERR_INVALID, "vertex normals: the triangle count is not the scene's");
  std::vector<jade_triangle> tris;
  if (const int rc = scene_triangles(s, &tris)) return rc;
  std::vector<float4> rec(tris.size() * JADE_SMOOTH_REC);
  bool any = false;
  for (size_t i = 0; i < tris.size(); ++i) {
    const jade_triangle& t = tris[i];
    smooth_record(t.p1, t.p2, t.p3, normals + 9 * i, t.norm, &rec[i * JADE_SMOOTH_REC]);
    uint32_t flag;
    memcpy(&flag, &rec[i * JADE_SMOOTH_REC].w, 4);
    any = any || flag != SMOOTH_FLAT;
  }
  T.set.normals.swap(rec);
  T.set.normals_any = any;
  normals_changed(&T);
  return JADE_OK;
}
int jade_scene_get_vertex_normals(jade_scene* s, int* set) {
  if (!s || !set) return jade_fail(JADE_ERR_INVALID, "null argument");
  *set = s->surf.set.normals.empty() ? 0 : 1;
  return JADE_OK;
}

// The textures of the scene handle (include/jade_bvh.h, "The surface colour, stated"): the records and the texel buffer (jade_texture.h) are made
// here, from the triangles as the handle holds them, and uploaded by the next jade_render_begin - a render in progress keeps the table it began
// with.  Everything is checked before anything of the handle changes: a refused call leaves the table that was there.
int jade_scene_set_textures(jade_scene* s, int32_t n_images, const jade_texture_image* images, const float* uv, const int32_t* image_of, int32_t n_triangles) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  SurfaceTables& T = s->surf;
  if (n_images == 0 || !images || !uv || !image_of) {
    clear_images(&T.set.textures);
    T.dev.textures_current = false;
    return JADE_OK;
  }
  SurfaceImages next;
  if (const int rc = surface_check_images("textures: ", n_images, images, image_of, n_triangles, s->dev.n_tris, &next.images, &next.texels, &next.any)) return rc;
  std::vector<jade_triangle> tris;
  if (const int rc = scene_triangles(s, &tris)) return rc;
  next.rec.resize(tris.size() * JADE_TEX_REC);
  for (size_t i = 0; i < tris.size(); ++i) texture_record(tris[i].p1, tris[i].p2, tris[i].p3, uv + 6 * i, image_of[i], &next.rec[i * JADE_TEX_REC]);
  std::swap(T.set.textures, next);
  T.dev.textures_current = false;
  return JADE_OK;
}
int jade_scene_get_textures(jade_scene* s, int* set) {
  if (!s || !set) return jade_fail(JADE_ERR_INVALID, "null argument");
  *set = s->surf.set.textures.rec.empty() ? 0 : 1;
  return JADE_OK;
}

// The normal maps of the scene handle (include/jade_bvh.h, "The mapped normal, stated"): the records and the texel buffer (jade_normal_map.h) are
// made here as the textures' are, checked in the same order - the strength first - and refused in the same way; the vertex normals a mapped vertex
// bends are joined to the records by the next jade_render_begin (surface_join_maps), which uploads them.
int jade_scene_set_normal_maps(jade_scene* s, int32_t n_images, const jade_texture_image* images, const float* uv, const int32_t* image_of, int32_t n_triangles,
                               float strength) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  SurfaceTables& T = s->surf;
  if (n_images == 0 || !images || !uv || !image_of) {
    clear_images(&T.set.maps);
    T.dev.maps_current = false;
    return JADE_OK;
  }
  if (!(strength >= 0.0f && strength < INFINITY))
    return jade_fail(JADE_ERR_INVALID, "normal maps: the strength " + std::to_string(strength) + " is not finite and >= 0");
  SurfaceImages next;
  if (const int rc = surface_check_images("normal maps: ", n_images, images, image_of, n_triangles, s->dev.n_tris, &next.images, &next.texels, &next.any)) return rc;
  std::vector<jade_triangle> tris;
  if (const int rc = scene_triangles(s, &tris)) return rc;
  next.rec.resize(tris.size() * JADE_NMAP_REC);
  next.any = false;
  for (size_t i = 0; i < tris.size(); ++i) {
    normal_map_record(tris[i].p1, tris[i].p2, tris[i].p3, uv + 6 * i, image_of[i], &next.rec[i * JADE_NMAP_REC]);
    int32_t stored;
    memcpy(&stored, &next.rec[i * JADE_NMAP_REC].w, 4);
    next.any = next.any || stored >= 0;  // (a triangle whose frame cannot be formed is stored unmapped)
  }
  std::swap(T.set.maps, next);
  T.set.strength = strength;
  T.dev.maps_current = false;
  return JADE_OK;
}
int jade_scene_get_normal_maps(jade_scene* s, int* set) {
  if (!s || !set) return jade_fail(JADE_ERR_INVALID, "null argument");
  *set = s->surf.set.maps.rec.empty() ? 0 : 1;
  return JADE_OK;
}

int surface_begin(jade_scene* s, uint32_t mode) {
  SurfaceTables& T = s->surf;
  const bool tex = (mode & SM_TEX) != 0, maps = (mode & SM_NMAP) != 0, smooth = (mode & SM_SMOOTH) != 0;
  // the handle's tables as they are now: the render keeps them whatever the setters are told before the next begin
  const bool send_textures = tex && T.set.textures.any && !T.dev.textures_current;
  const bool send_maps = maps && !T.dev.maps_current;
  const bool send_normals = smooth && T.set.normals_any && !T.dev.normals_current;
  if (send_textures || send_maps || send_normals) s->have_rp = false;  // (the earlier render's kernels would read a buffer that is given back here)
  if (send_textures) {
    HIP_TRY(upload(T.dev.tex_rec, T.set.textures.rec.data(), T.set.textures.rec.size(), s->stream));
    HIP_TRY(upload(T.dev.tex_texels, T.set.textures.texels.data(), T.set.textures.texels.size(), s->stream));
    HIP_TRY(upload(T.dev.tex_images, T.set.textures.images.data(), T.set.textures.images.size(), s->stream));
    T.dev.textures_current = true;
  }
  if (tex && !T.dev.flat.p) {
    const size_t bytes = sizeof(float4) * JADE_SMOOTH_REC * (size_t)s->dev.n_tris;
    HIP_TRY(T.dev.flat.alloc(bytes));
    HIP_TRY(hipMemsetAsync(T.dev.flat.p, 0, bytes, s->stream));
  }
  if (tex) T.dev.tex_none = !T.set.textures.any;
  if (maps && T.dev.tex_none && !T.dev.no_image.p) {  // texture records that say "no image" (-1, the 16 bytes such a vertex reads)
    const int32_t no_image = -1;
    float w;
    memcpy(&w, &no_image, 4);
    const std::vector<float4> none((size_t)s->dev.n_tris * JADE_TEX_REC, make_float4(0.0f, 0.0f, 0.0f, w));
    HIP_TRY(upload(T.dev.no_image, none.data(), none.size(), s->stream));
  }
  if (send_maps) {
    const std::vector<float4> rec = surface_join_maps(T);
    HIP_TRY(upload(T.dev.map_rec, rec.data(), rec.size(), s->stream));
    HIP_TRY(upload(T.dev.map_texels, T.set.maps.texels.data(), T.set.maps.texels.size(), s->stream));
    HIP_TRY(upload(T.dev.map_images, T.set.maps.images.data(), T.set.maps.images.size(), s->stream));
    T.dev.maps_current = true;
  }
  if (maps) T.dev.strength = T.set.strength;
  if (send_normals) {
    HIP_TRY(upload(T.dev.normals, T.set.normals.data(), T.set.normals.size(), s->stream));
    T.dev.normals_current = true;
  }
  if (tex) T.dev.tex_normals = (T.set.normals_any ? T.dev.normals : T.dev.flat).as<float4>();  // the handle's vertex normals, or the all-flat table where it carries none
  return JADE_OK;
}
