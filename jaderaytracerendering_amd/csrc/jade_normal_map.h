// jade_normal_map.h — normal maps (include/jade_bvh.h, "The mapped normal, stated"; the kernels of a mode with SM_NMAP only, jade_runtime.h):
// a tangent-space image filtered at every path vertex bends the vertex's shading normal.  The record a triangle's table entry is made of
// (host) and the one function of (triangle, point, reference direction) every use goes through (device): the shade kernels'
// (jade_smooth_shade.h, through the overload of shading_normal below), the denoiser's guide pass (jade_denoise.hip) and the unit entry's
// (jade_debug_units.hip).  The fetch and the uv are jade_texture.h's, the fall-backs jade_smooth.h's.
#pragma once
#include <cmath>
#include <cstring>

#include "jade_device.h"
#include "jade_smooth.h"
#include "jade_texture.h"

// ---- The table: JADE_NMAP_REC float4 per triangle - 128 B, one aligned cache line and one request per vertex - in the scene description's
// triangle order.  A mapped vertex needs the uv, the frame AND the interpolated normal it bends: with the texture record (64 B) and the smooth
// record (80 B) that would be two gathers of three lines; d2, d3 and p1 are common to both, and what is left of the two fits one line.
//   [0] = {p1, image}   image (int bits): the map's image, or -1 for an UNMAPPED triangle - a vertex of such a triangle reads these 16 bytes
//                       and then normal(triangle, p, r) from the vertex-normal table, as an unmapped render does
//   [1] .. [3]          the texture record's (jade_texture.h): d2, d3, uv1, du2, du3 of the MAP's uv
//   [4] = {T, flag}     T = dP/du, normalised; flag: the smooth record's (SMOOTH_FLAT where the handle carries no vertex normals)
//   [5] = {B, n1.x}     B = dP/dv, normalised
//   [6] = {n1.y, n1.z, m2.x, m2.y}      n1, m2, m3: the smooth record's, written by normal_map_join when the table is uploaded
//   [7] = {m2.z, m3}
#define JADE_NMAP_REC 8
// the rules a mapped vertex adds to jade_smooth.h's SMOOTH_RULE_* (jade_debug_mapped_normal reports them): the bent normal; a tilt of zero or
// a NaN among (mx, my, mz) - the result is normal(); a base or a sum whose squared length is not in (0, inf) - normal(); the bent normal on the
// wrong side and normal() gave ns.  Where the bent normal is on the wrong side and normal() gave g, the rule is normal()'s own.
enum : int32_t { SMOOTH_RULE_MAPPED = 5, SMOOTH_RULE_MAP_ZERO = 6, SMOOTH_RULE_MAP_SUM = 7, SMOOTH_RULE_MAP_SIDE_NS = 8 };

// What the kernels of a mapped mode take: the textured family's tables and the map's own three arrays, with its strength.  It stands where
// the family takes its table and converts as TexTables does (has_textures holds for it).
struct MapTables : TexTables {
  const float4* nrec;
  const float4* ntexels;
  const uint4* nimages;
  float strength;
};

// The record of one triangle, as the header states it: the texture record of the map's uv, and T and B in double from the fp32 corners and
// the record's fp32 du2, du3, each normalised and rounded once per component.  A triangle that names no image, or whose frame cannot be
// formed, is stored UNMAPPED.  The smooth part is zero (FLAT) until normal_map_join.  Host only.
static inline void normal_map_record(const float* p1, const float* p2, const float* p3, const float* uv6, int32_t image, float4* rec) {
  texture_record(p1, p2, p3, uv6, image, rec);
  for (int k = 4; k < JADE_NMAP_REC; ++k) rec[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const auto in_range = [](double x) { return x > 0.0 && x < (double)INFINITY; };
  bool mapped = image >= 0;
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = (double)p2[k] - (double)p1[k];
    e2[k] = (double)p3[k] - (double)p1[k];
  }
  const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  mapped = mapped && in_range(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
  const double du2x = rec[3].x, du2y = rec[3].y, du3x = rec[3].z, du3y = rec[3].w;
  const double det = du2x * du3y - du3x * du2y;
  mapped = mapped && det != 0.0 && std::isfinite(det);
  if (mapped) {
    double T[3], B[3];
    for (int k = 0; k < 3; ++k) {
      T[k] = (e1[k] * du3y - e2[k] * du2y) / det;
      B[k] = (e2[k] * du2x - e1[k] * du3x) / det;
    }
    const double lt = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]), lb = std::sqrt(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]);
    mapped = in_range(lt) && in_range(lb);
    if (mapped) {
      rec[4] = make_float4((float)(T[0] / lt), (float)(T[1] / lt), (float)(T[2] / lt), 0.0f);
      rec[5] = make_float4((float)(B[0] / lb), (float)(B[1] / lb), (float)(B[2] / lb), 0.0f);
    }
  }
  if (!mapped) {
    const int32_t none = -1;
    memcpy(&rec[0].w, &none, 4);
  }
}
// ... and the vertex normals a mapped vertex bends: the smooth record `smooth` of the same triangle (jade_smooth.h), or nullptr for FLAT
static inline void normal_map_join(float4* rec, const float4* smooth) {
  rec[4].w = smooth ? smooth[0].w : 0.0f;  // (SMOOTH_FLAT is 0)
  rec[5].w = smooth ? smooth[2].z : 0.0f;
  rec[6] = smooth ? make_float4(smooth[2].w, smooth[3].x, smooth[3].y, smooth[3].z) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  rec[7] = smooth ? make_float4(smooth[3].w, smooth[4].x, smooth[4].y, smooth[4].z) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// normal'(triangle, p, r) - THE function of a mapped render: the statement's steps in their order.  g: the triangle's stored flat normal.
static __device__ __forceinline__ jvec3 mapped_normal_rule(const MapTables& M, int tri, jvec3 g, jvec3 p, jvec3 r, int32_t* rule) {
  const float INF = jade_u2f(0x7f800000u);
  const float4* rec = M.nrec + (size_t)tri * JADE_NMAP_REC;
  const float4 r0 = rec[0];
  const int image = __float_as_int(r0.w);
  int32_t fell = -1;  // the step that fell back to normal(): none yet (an unmapped triangle, a uv that is not finite)
  if (image >= 0) {
    const float4 r1 = rec[1], r2 = rec[2], r3 = rec[3];
    float u, v;
    surface_uv_rec(r0, r1, r2, r3, p, &u, &v);
    const uint32_t inf = 0x7f800000u;
    if ((jade_f2u(u) & inf) != inf && (jade_f2u(v) & inf) != inf) {
      const jvec3 m = texture_fetch(M.ntexels, M.nimages, image, u, v);
      const float mx = M.strength * m.x, my = M.strength * m.y, mz = m.z;
      if ((mx == 0.0f && my == 0.0f) || mx != mx || my != my || mz != mz) {
        fell = SMOOTH_RULE_MAP_ZERO;
      } else {
        const float4 r4 = rec[4], r5 = rec[5], r6 = rec[6], r7 = rec[7];
        jvec3 nb = jv(0.0f, 0.0f, 0.0f);
        bool have = false;
        if (__float_as_uint(r4.w) == SMOOTH_ON) {  // ns before its side rule: the arithmetic of shading_normal_rule on the same numbers
          const jvec3 w = jv_sub(p, jv(r0.x, r0.y, r0.z));
          const float b2 = jv_dot(w, jv(r1.x, r1.y, r1.z));
          const float b3 = jv_dot(w, jv(r1.w, r2.x, r2.y));
          jvec3 s;
          s.x = jade_fma(b3, r7.y, jade_fma(b2, r6.z, r5.w));
          s.y = jade_fma(b3, r7.z, jade_fma(b2, r6.w, r6.x));
          s.z = jade_fma(b3, r7.w, jade_fma(b2, r7.x, r6.y));
          const float ss = jv_dot(s, s);
          if (ss > 0 && ss < INF) {
            nb = jv_divs(s, jade_sqrt(ss));
            have = true;
          }
        }
        if (!have) {
          const float gg = jv_dot(g, g);
          if (gg > 0 && gg < INF) {
            nb = jv_divs(g, jade_sqrt(gg));
            have = true;
          }
        }
        fell = SMOOTH_RULE_MAP_SUM;
        if (have) {
          jvec3 t;
          t.x = jade_fma(mz, nb.x, jade_fma(my, r5.x, mx * r4.x));
          t.y = jade_fma(mz, nb.y, jade_fma(my, r5.y, mx * r4.y));
          t.z = jade_fma(mz, nb.z, jade_fma(my, r5.z, mx * r4.z));
          const float tt = jv_dot(t, t);
          if (tt > 0 && tt < INF) {
            const jvec3 nm = jv_divs(t, jade_sqrt(tt));
            const float a = jv_dot(nm, r), b = jv_dot(g, r);
            if ((a > 0 && b > 0) || (a < 0 && b < 0)) {
              *rule = SMOOTH_RULE_MAPPED;
              return nm;
            }
            fell = SMOOTH_RULE_MAP_SIDE_NS;
          }
        }
      }
    }
  }
  int32_t base;
  const jvec3 n = shading_normal_rule(M.smooth, tri, g, p, r, &base);
  *rule = fell < 0 || (fell == SMOOTH_RULE_MAP_SIDE_NS && base != SMOOTH_RULE_NS) ? base : fell;
  return n;
}
// ... which is what the smooth family's one call resolves to under these tables
static __device__ __forceinline__ jvec3 shading_normal(const MapTables& M, int tri, jvec3 g, jvec3 p, jvec3 r) {
  int32_t rule;
  return mapped_normal_rule(M, tri, g, p, r, &rule);
}
