/* Exposes the inline routines of include/jade_fpmath.h to ctypes (test-only). */
#include "jade_fpmath.h"
#include "jade_rt.h"
#include <stddef.h>

#define EXPORT __attribute__((visibility("default")))
EXPORT int t_selftest(float one) { return jade_fp_selftest(one); }
EXPORT void t_sincos(const float* x, float* s, float* c, int n) { for (int i = 0; i < n; ++i) jade_sincosf(x[i], &s[i], &c[i]); }
EXPORT void t_log2(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_log2f(x[i]); }
EXPORT void t_exp2(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_exp2f(x[i]); }
EXPORT void t_pow(const float* a, const float* b, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_powf(a[i], b[i]); }
EXPORT void t_atan2(const float* a, const float* b, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_atan2f(a[i], b[i]); }
EXPORT void t_asin(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_asinf(x[i]); }
EXPORT void t_floor(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_floorf(x[i]); }
EXPORT void t_rand(uint32_t seed, uint32_t* states, float* u, int n) { for (int i = 0; i < n; ++i) { u[i] = jade_rand(&seed); states[i] = seed; } }
EXPORT uint32_t t_seed(uint32_t x, uint32_t y, uint32_t f) { return jade_rng_seed(x, y, f); }
EXPORT float t_dot(const float* a, const float* b) { return jv_dot(jv(a[0], a[1], a[2]), jv(b[0], b[1], b[2])); }
EXPORT float t_mixed(const float* a, const float* b, const float* c) { return jv_mixed(jv(a[0], a[1], a[2]), jv(b[0], b[1], b[2]), jv(c[0], c[1], c[2])); }
EXPORT void t_cross(const float* a, const float* b, float* o) { jvec3 r = jv_cross(jv(a[0], a[1], a[2]), jv(b[0], b[1], b[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
EXPORT void t_normalize(const float* a, float* o) { jvec3 r = jv_normalize(jv(a[0], a[1], a[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
EXPORT void t_transform(const float* v, float f4, const float* m, float* o) { jvec3 r = jade_transform(jv(v[0], v[1], v[2]), f4, m); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
EXPORT float t_fmin(float a, float b) { return jade_fminf(a, b); }
EXPORT float t_fmax(float a, float b) { return jade_fmaxf(a, b); }
/* array forms for the device twin (tests/test_gpu_fpmath.py): rows of 3 floats for the vector ops, one matrix for all rows */
#define R3(p, i) jv((p)[3 * (i)], (p)[3 * (i) + 1], (p)[3 * (i) + 2])
#define W3(o, i, r) do { jvec3 r_ = (r); (o)[3 * (i)] = r_.x; (o)[3 * (i) + 1] = r_.y; (o)[3 * (i) + 2] = r_.z; } while (0)
EXPORT void t_atan(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_atanf(x[i]); }
EXPORT void t_sqrt(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_sqrt(x[i]); }
EXPORT void t_div(const float* a, const float* b, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = a[i] / b[i]; }
EXPORT void t_rcp(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = 1.0f / x[i]; }
EXPORT void t_fmin_n(const float* a, const float* b, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_fminf(a[i], b[i]); }
EXPORT void t_fmax_n(const float* a, const float* b, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jade_fmaxf(a[i], b[i]); }
EXPORT void t_dot_n(const float* a, const float* b, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jv_dot(R3(a, i), R3(b, i)); }
EXPORT void t_cross_n(const float* a, const float* b, float* o, int n) { for (int i = 0; i < n; ++i) W3(o, i, jv_cross(R3(a, i), R3(b, i))); }
EXPORT void t_mixed_n(const float* a, const float* b, const float* c, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jv_mixed(R3(a, i), R3(b, i), R3(c, i)); }
EXPORT void t_len_n(const float* a, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = jv_len(R3(a, i)); }
EXPORT void t_normalize_n(const float* a, float* o, int n) { for (int i = 0; i < n; ++i) W3(o, i, jv_normalize(R3(a, i))); }
EXPORT void t_transform_n(const float* v, const float* f4, const float* m, float* o, int n) { for (int i = 0; i < n; ++i) W3(o, i, jade_transform(R3(v, i), f4[i], m)); }
EXPORT void t_vdiv_n(const float* a, const float* b, float* o, int n) { for (int i = 0; i < n; ++i) W3(o, i, jv_div(R3(a, i), R3(b, i))); }
EXPORT void t_vdivs_n(const float* a, const float* s, float* o, int n) { for (int i = 0; i < n; ++i) W3(o, i, jv_divs(R3(a, i), s[i])); }
EXPORT void t_seed_n(const uint32_t* x, const uint32_t* y, const uint32_t* f, uint32_t* o, int n) { for (int i = 0; i < n; ++i) o[i] = jade_rng_seed(x[i], y[i], f[i]); }
EXPORT void t_rand_n(const uint32_t* seeds, int k, float* u, uint32_t* states, int n) {
  for (int i = 0; i < n; ++i) { uint32_t s = seeds[i]; for (int j = 0; j < k; ++j) { u[(size_t)i * k + j] = jade_rand(&s); states[(size_t)i * k + j] = s; } }
}
EXPORT void t_selftest_n(const float* one, int32_t* o, int n) { for (int i = 0; i < n; ++i) o[i] = jade_fp_selftest(one[i]); }
/* layout of the boundary structs as the C compiler sees them */
EXPORT void t_layout(int* out) {
  out[0] = (int)sizeof(jade_triangle); out[1] = (int)sizeof(jade_bvh_node); out[2] = (int)sizeof(jade_obj_seg);
  out[3] = (int)sizeof(jade_scene_desc); out[4] = (int)sizeof(jade_render_params); out[5] = (int)sizeof(jade_stats);
  out[6] = (int)offsetof(jade_triangle, norm); out[7] = (int)offsetof(jade_triangle, emissive);
  out[8] = (int)offsetof(jade_triangle, brdf); out[9] = (int)offsetof(jade_triangle, reflex_mode);
  out[10] = (int)offsetof(jade_triangle, refract_rate); out[11] = (int)offsetof(jade_triangle, refract_albedo);
  out[12] = (int)offsetof(jade_triangle, refract_index); out[13] = (int)offsetof(jade_bvh_node, aa);
}
