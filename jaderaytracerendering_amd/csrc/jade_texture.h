// jade_texture.h — albedo textures (include/jade_bvh.h, "The surface colour, stated"; the kernels of a mode with SM_TEX only, jade_runtime.h):
// an image filtered at every path vertex and multiplied into the vertex's brdf and refract_albedo.  The record a triangle's table entry is
// made of and the texel buffer (host), and the one function of (triangle, point) every use goes through (device): the shade kernels'
// (jade_smooth_shade.h), the denoiser's guide pass (jade_denoise.hip) and the unit entries' (jade_debug_units.hip).  CDNA has no filtering
// units: a fetch is four 16-byte loads and the fp32 operations the header writes out.
#pragma once
#include <cmath>
#include <cstring>
#include <type_traits>

#include "jade_device.h"

// ---- The table: JADE_TEX_REC float4 per triangle (64 B, one request per vertex), in the scene description's triangle order.
//   [0] = {p1, image}   image (int bits): the triangle's image, or -1 - a vertex of such a triangle reads these 16 bytes and nothing else
//   [1] = {d2, d3.x}    the dual basis of jade_smooth.h's record: b2 = w.d2, b3 = w.d3; both 0 where N.N is not in (0, inf)
//   [2] = {d3.y, d3.z, u1, v1}
//   [3] = {du2.x, du2.y, du3.x, du3.y}   du2 = uv2 - uv1, du3 = uv3 - uv1
// ---- The images: one buffer of float4 texels {r, g, b, 0}, image after image, row 0 (v = 0) first, and one uint4 {first texel (low, high
// word), W, H} per image.  The two taps of a row are adjacent except at the wrap.
#define JADE_TEX_REC 4
#define JADE_TEX_MAX_SIZE 16384
#define JADE_TEX_MAX_IMAGES 65536

// What the kernels of a textured mode take: the vertex-normal records (the scene's, or an all-flat table: jade_smooth.h's SMOOTH_FLAT is 0)
// and the three arrays above.  It stands where the smooth family takes its `const float4* table` and converts to it.
struct TexTables {
  const float4* smooth;
  const float4* rec;
  const float4* texels;
  const uint4* images;
  __device__ operator const float4*() const { return smooth; }
};
template <class ST>
static constexpr bool has_textures = std::is_base_of<TexTables, ST>::value;  // (TexTables itself, or the tables of a mapped mode that carry it: jade_normal_map.h)

// The record of one triangle, as the header states it: the dual basis in double from the fp32 corners, each component rounded once (the
// smooth record's); du2 and du3 one fp32 subtraction per component.  uv6: the corners' (u, v) in the order p1 p2 p3.  Host only.
static inline void texture_record(const float* p1, const float* p2, const float* p3, const float* uv6, int32_t image, float4* rec) {
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = (double)p2[k] - (double)p1[k];
    e2[k] = (double)p3[k] - (double)p1[k];
  }
  const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double NN = N[0] * N[0] + N[1] * N[1] + N[2] * N[2];
  float d2[3] = {0, 0, 0}, d3[3] = {0, 0, 0};
  if (NN > 0.0 && NN < (double)INFINITY) {
    const double a[3] = {e2[1] * N[2] - e2[2] * N[1], e2[2] * N[0] - e2[0] * N[2], e2[0] * N[1] - e2[1] * N[0]};  // e2 x N
    const double b[3] = {N[1] * e1[2] - N[2] * e1[1], N[2] * e1[0] - N[0] * e1[2], N[0] * e1[1] - N[1] * e1[0]};  // N x e1
    for (int k = 0; k < 3; ++k) {
      d2[k] = (float)(a[k] / NN);
      d3[k] = (float)(b[k] / NN);
    }
  }
  float fi;
  memcpy(&fi, &image, 4);
  rec[0] = make_float4(p1[0], p1[1], p1[2], fi);
  rec[1] = make_float4(d2[0], d2[1], d2[2], d3[0]);
  rec[2] = make_float4(d3[1], d3[2], uv6[0], uv6[1]);
  rec[3] = make_float4(uv6[2] - uv6[0], uv6[3] - uv6[1], uv6[4] - uv6[0], uv6[5] - uv6[1]);
}

// uv(triangle, p) from the record's last three float4
static __device__ __forceinline__ void surface_uv_rec(float4 r0, float4 r1, float4 r2, float4 r3, jvec3 p, float* u, float* v) {
  const jvec3 w = jv_sub(p, jv(r0.x, r0.y, r0.z));
  const float b2 = jv_dot(w, jv(r1.x, r1.y, r1.z));
  const float b3 = jv_dot(w, jv(r1.w, r2.x, r2.y));
  *u = jade_fma(b3, r3.z, jade_fma(b2, r3.x, r2.z));
  *v = jade_fma(b3, r3.w, jade_fma(b2, r3.y, r2.w));
}
static __device__ __forceinline__ void surface_uv(const float4* rec_table, int tri, jvec3 p, float* u, float* v) {
  const float4* rec = rec_table + (size_t)tri * JADE_TEX_REC;
  surface_uv_rec(rec[0], rec[1], rec[2], rec[3], p, u, v);
}

// One axis of the fetch: the two taps i0, i1 in [0, n) (repeat) and the weight of the second
static __device__ __forceinline__ void texture_axis(float u, int n, int* i0, int* i1, float* f) {
  const float up = u - floorf(u);
  const float x = jade_fma(up, (float)n, -0.5f);
  const float xf = floorf(x);
  *f = x - xf;
  int a = (int)xf, b = a + 1;
  if (a < 0) a = n - 1;
  if (b >= n) b = 0;  // (b == n is the statement's case; >= keeps every load in range whatever an image header holds)
  *i0 = a;
  *i1 = b;
}
// texel colour(image, u, v): the bilinear filter of the header, op by op
static __device__ __forceinline__ jvec3 texture_fetch(const float4* texels, const uint4* images, int image, float u, float v) {
  const uint32_t inf = 0x7f800000u;
  if ((jade_f2u(u) & inf) == inf || (jade_f2u(v) & inf) == inf) return jv(1.0f, 1.0f, 1.0f);
  const uint4 im = images[image];
  const int W = (int)im.z, H = (int)im.w;
  int i0, i1, j0, j1;
  float fx, fy;
  texture_axis(u, W, &i0, &i1, &fx);
  texture_axis(v, H, &j0, &j1, &fy);
  const float4* t = texels + (((size_t)im.y << 32) | (size_t)im.x);
  const float4 t00 = t[(size_t)j0 * W + i0], t10 = t[(size_t)j0 * W + i1], t01 = t[(size_t)j1 * W + i0], t11 = t[(size_t)j1 * W + i1];
  jvec3 c;
  {
    const float top = jade_fma(fx, t10.x - t00.x, t00.x), bottom = jade_fma(fx, t11.x - t01.x, t01.x);
    c.x = jade_fma(fy, bottom - top, top);
  }
  {
    const float top = jade_fma(fx, t10.y - t00.y, t00.y), bottom = jade_fma(fx, t11.y - t01.y, t01.y);
    c.y = jade_fma(fy, bottom - top, top);
  }
  {
    const float top = jade_fma(fx, t10.z - t00.z, t00.z), bottom = jade_fma(fx, t11.z - t01.z, t01.z);
    c.z = jade_fma(fy, bottom - top, top);
  }
  return c;
}

// The surface colour c of triangle `tri` at point p - THE function of (triangle, point): (1, 1, 1) for a triangle without an image
static __device__ __forceinline__ jvec3 surface_colour(const TexTables& T, int tri, jvec3 p) {
  const float4* rec = T.rec + (size_t)tri * JADE_TEX_REC;
  const float4 r0 = rec[0];
  const int image = __float_as_int(r0.w);
  if (image < 0) return jv(1.0f, 1.0f, 1.0f);
  float u, v;
  surface_uv_rec(r0, rec[1], rec[2], rec[3], p, &u, &v);
  return texture_fetch(T.texels, T.images, image, u, v);
}
// The material at a vertex: brdf_eff = fl(brdf * c), albedo_eff = fl(refract_albedo * c).  In a mode without textures - ST is the smooth
// family's `const float4*` - the material's own value, and no instruction.
template <class ST>
static __device__ __forceinline__ jvec3 textured(const ST& table, int tri, jvec3 p, jvec3 material) {
  if constexpr (has_textures<ST>) return jv_mul(material, surface_colour(table, tri, p));
  else return material;
}
// ... with the colour at hand
template <class ST>
static __device__ __forceinline__ jvec3 tinted(jvec3 material, jvec3 colour) {
  if constexpr (has_textures<ST>) return jv_mul(material, colour);
  else return material;
}
