// jade_smooth.h — smooth shading (include/jade_bvh.h, "The shading normal, stated"; the kernels of a mode with SM_SMOOTH only, jade_runtime.h):
// the vertex normals of a triangle interpolated at every path vertex.  The record a triangle's table entry is made of (host) and the one
// function of (triangle, point, reference direction) every use goes through (device): the shade kernels' (jade_smooth_shade.h), the
// denoiser's guide pass (jade_denoise.hip) and the unit entry's (jade_debug_units.hip).
#pragma once
#include <cmath>
#include <cstring>

#include "jade_device.h"

// ---- The table: JADE_SMOOTH_REC float4 per triangle, in the scene description's triangle order.
//   [0] = {p1, flag}   flag (uint bits): SMOOTH_FLAT - the three normals are bitwise the triangle's norm; SMOOTH_DEGENERATE - N.N is 0 (or not
//                      finite); SMOOTH_ON otherwise.  A vertex of a triangle that is not SMOOTH_ON reads these 16 bytes and nothing else.
//   [1] = {d2, d3.x}   d2 = (e2 x N) / (N.N), d3 = (N x e1) / (N.N): the dual basis, so that b2 = w.d2 and b3 = w.d3
//   [2] = {d3.y, d3.z, n1.x, n1.y}
//   [3] = {n1.z, m2}   m2 = n2 - n1
//   [4] = {m3, 0}      m3 = n3 - n1
// One gather of 80 B and 15 FMAs per vertex, in place of the triangle's 36 B of corners, its 36 B of normals, two cross products and a division.
#define JADE_SMOOTH_REC 5
enum : uint32_t { SMOOTH_FLAT = 0u, SMOOTH_ON = 1u, SMOOTH_DEGENERATE = 2u };
// which rule gave the normal (jade_debug_shading_normal reports it; the kernels ask for the normal alone)
enum : int32_t { SMOOTH_RULE_NS = 0, SMOOTH_RULE_FLAT = 1, SMOOTH_RULE_DEGENERATE = 2, SMOOTH_RULE_SUM = 3, SMOOTH_RULE_SIDE = 4 };

// The record of one triangle, as the header states it: the edges, N, N.N and the two dual vectors in double from the fp32 corners, each
// component rounded to fp32 once; m2 and m3 one fp32 subtraction per component.  Host only.
static inline void smooth_record(const float* p1, const float* p2, const float* p3, const float* n9, const float* g, float4* rec) {
  const bool flat = memcmp(n9, g, 12) == 0 && memcmp(n9 + 3, g, 12) == 0 && memcmp(n9 + 6, g, 12) == 0;
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = (double)p2[k] - (double)p1[k];
    e2[k] = (double)p3[k] - (double)p1[k];
  }
  const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double NN = N[0] * N[0] + N[1] * N[1] + N[2] * N[2];
  const bool degenerate = !(NN > 0.0 && NN < (double)INFINITY);
  const uint32_t flag = flat ? SMOOTH_FLAT : degenerate ? SMOOTH_DEGENERATE : SMOOTH_ON;
  float d2[3] = {0, 0, 0}, d3[3] = {0, 0, 0};
  if (flag == SMOOTH_ON) {
    const double a[3] = {e2[1] * N[2] - e2[2] * N[1], e2[2] * N[0] - e2[0] * N[2], e2[0] * N[1] - e2[1] * N[0]};  // e2 x N
    const double b[3] = {N[1] * e1[2] - N[2] * e1[1], N[2] * e1[0] - N[0] * e1[2], N[0] * e1[1] - N[1] * e1[0]};  // N x e1
    for (int k = 0; k < 3; ++k) {
      d2[k] = (float)(a[k] / NN);
      d3[k] = (float)(b[k] / NN);
    }
  }
  uint32_t fw;
  memcpy(&fw, &flag, 4);
  float ff;
  memcpy(&ff, &fw, 4);
  rec[0] = make_float4(p1[0], p1[1], p1[2], ff);
  rec[1] = make_float4(d2[0], d2[1], d2[2], d3[0]);
  rec[2] = make_float4(d3[1], d3[2], n9[0], n9[1]);
  rec[3] = make_float4(n9[2], n9[3] - n9[0], n9[4] - n9[1], n9[5] - n9[2]);
  rec[4] = make_float4(n9[6] - n9[0], n9[7] - n9[1], n9[8] - n9[2], 0.0f);
}

// The shading normal of triangle `tri` at point p for the reference direction r; g: the triangle's stored flat normal.  *rule: SMOOTH_RULE_*.
static __device__ __forceinline__ jvec3 shading_normal_rule(const float4* table, int tri, jvec3 g, jvec3 p, jvec3 r, int32_t* rule) {
  const float4* rec = table + (size_t)tri * JADE_SMOOTH_REC;
  const float4 r0 = rec[0];
  const uint32_t flag = __float_as_uint(r0.w);
  if (flag != SMOOTH_ON) {
    *rule = flag == SMOOTH_FLAT ? SMOOTH_RULE_FLAT : SMOOTH_RULE_DEGENERATE;
    return g;
  }
  const float4 r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
  const jvec3 w = jv_sub(p, jv(r0.x, r0.y, r0.z));
  const float b2 = jv_dot(w, jv(r1.x, r1.y, r1.z));
  const float b3 = jv_dot(w, jv(r1.w, r2.x, r2.y));
  jvec3 s;
  s.x = jade_fma(b3, r4.x, jade_fma(b2, r3.y, r2.z));
  s.y = jade_fma(b3, r4.y, jade_fma(b2, r3.z, r2.w));
  s.z = jade_fma(b3, r4.z, jade_fma(b2, r3.w, r3.x));
  const float ss = jv_dot(s, s);
  if (!(ss > 0 && ss < jade_u2f(0x7f800000u))) {
    *rule = SMOOTH_RULE_SUM;
    return g;
  }
  const jvec3 ns = jv_divs(s, jade_sqrt(ss));
  const float a = jv_dot(ns, r), b = jv_dot(g, r);
  if (!((a > 0 && b > 0) || (a < 0 && b < 0))) {  // (ns.r)(g.r) <= 0, or not a number: the product is never formed, so it cannot underflow
    *rule = SMOOTH_RULE_SIDE;
    return g;
  }
  *rule = SMOOTH_RULE_NS;
  return ns;
}
static __device__ __forceinline__ jvec3 shading_normal(const float4* table, int tri, jvec3 g, jvec3 p, jvec3 r) {
  int32_t rule;
  return shading_normal_rule(table, tri, g, p, r, &rule);
}
// two vectors on one side of the plane of g: both dot products positive or both negative (zero or NaN: no)
static __device__ __forceinline__ bool same_side(jvec3 a, jvec3 b, jvec3 g) {
  const float x = jv_dot(a, g), y = jv_dot(b, g);
  return (x > 0 && y > 0) || (x < 0 && y < 0);
}
static __device__ __forceinline__ bool other_side(jvec3 a, jvec3 b, jvec3 g) {
  const float x = jv_dot(a, g), y = jv_dot(b, g);
  return (x > 0 && y < 0) || (x < 0 && y > 0);
}

