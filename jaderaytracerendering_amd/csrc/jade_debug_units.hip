// jade_debug_units.hip — test-only entry points that run the shared numeric pieces on the device one by one: every routine of
// include/jade_fpmath.h, the environment lookup (sample_hdr, jade_shade.h), the environment importance draw (env_sample, jade_shade.h,
// and its table, env_alias_table, jade_scene_prep.hip; the environment mixture's draw over the same table, env_mix_sample_with and env_texel_of, tests/test_gpu_env_mixture.py; the one-light draw, light_sample, and its table, light_alias_table; the cosine bounce draw, cosine_dir_with; the weights of JADE_DIRECT_MIS, mis_terms, and its table, mis_table), the tone curve (tone_pack_bgr8, jade_device.h) the thin-lens ray (lens_ray,
// jade_device.h; tests/test_lens_cpu.py, tests/test_gpu_lens.py) and the BSSRDF branch's exit-triangle search (exit_search, jade_shade.h, and
// its tables, guide_tables, jade_scene_prep.hip; tests/test_area_search_cpu.py, tests/test_gpu_area_search.py).
// NOT part of jade_rt.h and NOT in libjade_hip.so: only a -DJADE_DEBUG_EXPORTS=1 build (libjade_hip_debug.so) has them
// (tests/test_gpu_fpmath.py, tests/test_gpu_env_lookup.py, tests/test_gpu_env_importance.py, tests/test_gpu_tone.py, tests/test_tone_spec.py).  Each kernel is elementwise: element i reads
// row i of its inputs and writes row i of its outputs, nothing else.
#include <cstring>

#include "jade_runtime.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // jade_shade.h's non-inline statics this file does not call
#include "jade_shade.h"
#include "jade_smooth.h"
#include "jade_normal_map.h"
#pragma clang diagnostic pop

#if JADE_DEBUG_EXPORTS

// One code per routine of jade_fpmath.h (tests/test_gpu_fpmath.py mirrors this list).  Every array element is 4 bytes wide; the
// comment gives the elements per row of a, b, c -> out0, out1 ("-" = not read / not written, may be null).
enum DebugFpOp {
  FP_FLOOR = 0,      // a 1 -> 1
  FP_SINCOS = 1,     // a 1 -> sin 1, cos 1
  FP_LOG2 = 2,       // a 1 -> 1
  FP_EXP2 = 3,       // a 1 -> 1
  FP_POW = 4,        // a 1, b 1 -> 1
  FP_ATAN = 5,       // a 1 -> 1
  FP_ATAN2 = 6,      // a 1 (y), b 1 (x) -> 1
  FP_ASIN = 7,       // a 1 -> 1
  FP_FMIN = 8,       // a 1, b 1 -> 1
  FP_FMAX = 9,       // a 1, b 1 -> 1
  FP_SQRT = 10,      // a 1 -> 1
  FP_DIV = 11,       // a 1, b 1 -> a / b
  FP_RCP = 12,       // a 1 -> 1.0f / a
  FP_DOT = 13,       // a 3, b 3 -> 1
  FP_CROSS = 14,     // a 3, b 3 -> 3
  FP_MIXED = 15,     // a 3, b 3, c 3 -> 1
  FP_LEN = 16,       // a 3 -> 1
  FP_NORMALIZE = 17, // a 3 -> 3
  FP_TRANSFORM = 18, // a 3 (v), b 1 (f4), c: ONE matrix of 16 floats for all rows -> 3
  FP_VDIV = 19,      // a 3, b 3 -> 3 (jv_div)
  FP_VDIVS = 20,     // a 3, b 1 -> 3 (jv_divs)
  FP_RNG_SEED = 21,  // a, b, c: uint32 px, py, frame -> uint32 seed
  FP_RAND = 22,      // a: uint32 state, b: ONE int32 k for all rows -> out0 k floats (k successive jade_rand), out1 k uint32 (the state after each)
  FP_SELFTEST = 23,  // a 1 (`one`) -> int32 jade_fp_selftest(one)
  FP_N_OPS
};

struct DebugFpShape { int a, b, c, o0, o1; bool b_once, c_once; };
static const DebugFpShape kFpShape[] = {  // one row per DebugFpOp, in its order
    {1, 0, 0, 1, 0, false, false},  // FP_FLOOR
    {1, 0, 0, 1, 1, false, false},  // FP_SINCOS
    {1, 0, 0, 1, 0, false, false},  // FP_LOG2
    {1, 0, 0, 1, 0, false, false},  // FP_EXP2
    {1, 1, 0, 1, 0, false, false},  // FP_POW
    {1, 0, 0, 1, 0, false, false},  // FP_ATAN
    {1, 1, 0, 1, 0, false, false},  // FP_ATAN2
    {1, 0, 0, 1, 0, false, false},  // FP_ASIN
    {1, 1, 0, 1, 0, false, false},  // FP_FMIN
    {1, 1, 0, 1, 0, false, false},  // FP_FMAX
    {1, 0, 0, 1, 0, false, false},  // FP_SQRT
    {1, 1, 0, 1, 0, false, false},  // FP_DIV
    {1, 0, 0, 1, 0, false, false},  // FP_RCP
    {3, 3, 0, 1, 0, false, false},  // FP_DOT
    {3, 3, 0, 3, 0, false, false},  // FP_CROSS
    {3, 3, 3, 1, 0, false, false},  // FP_MIXED
    {3, 0, 0, 1, 0, false, false},  // FP_LEN
    {3, 0, 0, 3, 0, false, false},  // FP_NORMALIZE
    {3, 1, 16, 3, 0, false, true},  // FP_TRANSFORM
    {3, 3, 0, 3, 0, false, false},  // FP_VDIV
    {3, 1, 0, 3, 0, false, false},  // FP_VDIVS
    {1, 1, 1, 1, 0, false, false},  // FP_RNG_SEED
    {1, 1, 0, 1, 1, true, false},   // FP_RAND
    {1, 0, 0, 1, 0, false, false},  // FP_SELFTEST
};
static_assert(sizeof kFpShape / sizeof kFpShape[0] == FP_N_OPS, "kFpShape needs one row per DebugFpOp");

static __device__ __forceinline__ void put3(float* o, int i, jvec3 v) {
  o[3 * i] = v.x;
  o[3 * i + 1] = v.y;
  o[3 * i + 2] = v.z;
}

__global__ void k_debug_fpmath(int op, int n, int k, const float* a, const float* b, const float* c, float* o0, float* o1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* ua = reinterpret_cast<const uint32_t*>(a);
  const uint32_t* ub = reinterpret_cast<const uint32_t*>(b);
  const uint32_t* uc = reinterpret_cast<const uint32_t*>(c);
  switch (op) {
    case FP_FLOOR: o0[i] = jade_floorf(a[i]); break;
    case FP_SINCOS: {
      float s, cs;
      jade_sincosf(a[i], &s, &cs);
      o0[i] = s;
      o1[i] = cs;
      break;
    }
    case FP_LOG2: o0[i] = jade_log2f(a[i]); break;
    case FP_EXP2: o0[i] = jade_exp2f(a[i]); break;
    case FP_POW: o0[i] = jade_powf(a[i], b[i]); break;
    case FP_ATAN: o0[i] = jade_atanf(a[i]); break;
    case FP_ATAN2: o0[i] = jade_atan2f(a[i], b[i]); break;
    case FP_ASIN: o0[i] = jade_asinf(a[i]); break;
    case FP_FMIN: o0[i] = jade_fminf(a[i], b[i]); break;
    case FP_FMAX: o0[i] = jade_fmaxf(a[i], b[i]); break;
    case FP_SQRT: o0[i] = jade_sqrt(a[i]); break;
    case FP_DIV: o0[i] = a[i] / b[i]; break;
    case FP_RCP: o0[i] = 1.0f / a[i]; break;
    case FP_DOT: o0[i] = jv_dot(V3(a + 3 * i), V3(b + 3 * i)); break;
    case FP_CROSS: put3(o0, i, jv_cross(V3(a + 3 * i), V3(b + 3 * i))); break;
    case FP_MIXED: o0[i] = jv_mixed(V3(a + 3 * i), V3(b + 3 * i), V3(c + 3 * i)); break;
    case FP_LEN: o0[i] = jv_len(V3(a + 3 * i)); break;
    case FP_NORMALIZE: put3(o0, i, jv_normalize(V3(a + 3 * i))); break;
    case FP_TRANSFORM: put3(o0, i, jade_transform(V3(a + 3 * i), b[i], c)); break;
    case FP_VDIV: put3(o0, i, jv_div(V3(a + 3 * i), V3(b + 3 * i))); break;
    case FP_VDIVS: put3(o0, i, jv_divs(V3(a + 3 * i), b[i])); break;
    case FP_RNG_SEED: reinterpret_cast<uint32_t*>(o0)[i] = jade_rng_seed(ua[i], ub[i], uc[i]); break;
    case FP_RAND: {
      uint32_t s = ua[i];
      for (int j = 0; j < k; ++j) {
        o0[(size_t)i * k + j] = jade_rand(&s);
        reinterpret_cast<uint32_t*>(o1)[(size_t)i * k + j] = s;
      }
      break;
    }
    case FP_SELFTEST: reinterpret_cast<int32_t*>(o0)[i] = jade_fp_selftest(a[i]); break;
    default: break;
  }
}

__global__ void k_debug_sample_hdr(DevScene S, int n, const float* d, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) put3(out, i, sample_hdr(S, V3(d + 3 * i)));
}

// row i: the importance draw with the four uniforms u[4 i ..] (jade_rt.h, JADE_ENV_IMPORTANCE)
__global__ void k_debug_env_sample(DevScene S, int n, const float* u, float* dir, float* ratio, uint32_t* texel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  put3(dir, i, env_sample_at(S, u + 4 * i, ratio + i, texel + i));
}

// row i: the draw as the shading kernel makes it, from RNG state rng[i]; the state it leaves is written back
// light_sample's body on the four uniforms of row i: the entry drawn, the folded (rx, ry), and the weight twice - as the draw forms it
// and as consume forms it again from the entry alone (light_weight)
__global__ void k_debug_light_sample(const uint4* table, uint32_t nE, int n, const float* u, uint32_t* entry, float* rxy, float* weight) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* u4 = u + 4 * i;
  int k = 0;
  float rx, ry, w;
  const uint32_t e = light_sample_with(table, nE, [u4, &k]() { return u4[k++]; }, &rx, &ry, &w);
  entry[i] = e;
  rxy[2 * i] = rx;
  rxy[2 * i + 1] = ry;
  weight[2 * i] = w;
  weight[2 * i + 1] = light_weight(table, nE, e);
}

__global__ void k_debug_env_sample_rng(DevScene S, int n, uint32_t* rng, float* dir, float* ratio) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t state = rng[i];
  put3(dir, i, env_sample(S, &state, ratio + i));
  rng[i] = state;
}

// env_mix_sample_with's body (jade_shade.h; include/jade_rt.h, JADE_ENV_MIXTURE) on row i = (u0..u4, n[3], side, bounce technique), MIX_ROW
// floats: the direction, m and the info word (EMI_*) ...
#define MIX_ROW 10
#define MIX_ROW_RNG 5
__global__ void k_debug_env_mix_sample(DevScene S, int n, const float* rows, float* dir, float* m, uint32_t* info) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rows + MIX_ROW * (size_t)i;
  const jvec3 nrm = jv(r[5], r[6], r[7]);
  put3(dir, i, r[9] != 0.0f ? env_mix_sample_at<true>(S, r, nrm, r[8], m + i, info + i) : env_mix_sample_at<false>(S, r, nrm, r[8], m + i, info + i));
}
// ... and the wrapper the shading kernel calls, on row i = (n[3], side, bounce technique) from RNG state rng[i]; the state it leaves is written back
__global__ void k_debug_env_mix_sample_rng(DevScene S, int n, const float* rows, uint32_t* rng, float* dir, float* m, uint32_t* info) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rows + MIX_ROW_RNG * (size_t)i;
  const jvec3 nrm = jv(r[0], r[1], r[2]);
  uint32_t state = rng[i];
  put3(dir, i, r[4] != 0.0f ? env_mix_sample<true>(S, &state, nrm, r[3], m + i, info + i) : env_mix_sample<false>(S, &state, nrm, r[3], m + i, info + i));
  rng[i] = state;
}
__global__ void k_debug_env_texel_of(DevScene S, int n, const float* d, uint32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = env_texel_of(S, V3(d + 3 * i));
}

// cosine_dir_with's body (jade_shade.h; include/jade_bvh.h "The bounce, stated") on row i = (n[3], s, u1, u2): the direction and whether
// the normal gave no axis ...
__global__ void k_debug_bounce_dir(int n, const float* rows, float* dir, int32_t* fallback) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rows + 6 * (size_t)i;
  bool fb;
  put3(dir, i, cosine_dir_at(r + 4, jv(r[0], r[1], r[2]), r[3], &fb));
  fallback[i] = fb ? 1 : 0;
}
// ... and the wrapper the shading kernel calls, on row i = (n[3], s) from RNG state rng[i]; the state it leaves is written back
__global__ void k_debug_bounce_dir_rng(int n, const float* rows, uint32_t* rng, float* dir) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rows + 4 * (size_t)i;
  uint32_t state = rng[i];
  put3(dir, i, cosine_dir_rng(&state, jv(r[0], r[1], r[2]), r[3]));
  rng[i] = state;
}

// mis_terms (jade_shade.h; include/jade_bvh.h "The direct light, stated") on row i = (n[3], ne[3], A, m, mu, l[3], Le, f), 14 floats:
// out[2 i] = w_L, out[2 i + 1] = T_B of one channel = ((Le * f) * g_B) / fl(0.9), as consume forms it
__global__ void k_debug_mis_terms(int n, const float* rows, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rows + 14 * (size_t)i;
  float w_L, g_B;
  mis_terms(jv(r[0], r[1], r[2]), jv(r[3], r[4], r[5]), r[6], r[7], r[8], jv(r[9], r[10], r[11]), &w_L, &g_B);
  out[2 * (size_t)i] = w_L;
  out[2 * (size_t)i + 1] = r[12] * r[13] * g_B / (float)JADE_RR_RATE_D;
}

__global__ void k_debug_tone_pack(int n, const float* rgb, int tonemap, float limit, uint8_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tone_pack_bgr8(V3(rgb + 3 * i), tonemap, limit, true, out + 3 * (size_t)i);
}

// A row of the lens ray's test entries, 32 floats: x, y, W, H (whole numbers), eye[3], cam[16], A, f, u1, u2, u3, u4, 3 unused.
// The jitter statements are the render's (camera_ray_dir, jade_device.h) with u1, u2 in place of the two draws; k = f / 1.5f as
// jade_render_begin forms it.  out: origin[3], dir[3].
#define LENS_ROW 32
static __host__ __device__ __forceinline__ void debug_lens_row(const float* row, float* out) {
  const float x = row[0], y = row[1];
  const double two_over_w = 2.0 / (double)(int)row[2], two_over_h = 2.0 / (double)(int)row[3];
  const double aspect = (double)(int)row[2] / (double)(int)row[3];
  const float fx = (float)(int)x + row[25];
  const double lo = -1.0 + two_over_w * ((double)fx - 0.5);
  const float left_offset = (float)(lo * aspect);
  const float fy = (float)(int)y + row[26];
  const float up_offset = (float)(-1.0 + two_over_h * ((double)fy - 0.5));
  const float k = row[24] / 1.5f;
  jvec3 o, d;
  lens_ray(row + 7, row + 4, row[23], k, left_offset, up_offset, row[27], row[28], &o, &d);
  out[0] = o.x; out[1] = o.y; out[2] = o.z;
  out[3] = d.x; out[4] = d.y; out[5] = d.z;
}
__global__ void k_debug_lens_ray(int n, const float* rows, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) debug_lens_row(rows + (size_t)LENS_ROW * i, out + 6 * (size_t)i);
}
// row i: the lens ray as the shading kernel draws it, for sample sidx[i] of pixel (px[i], py[i]); the stream's state after the four draws
__global__ void k_debug_lens_ray_rng(RenderConst R, float lens_k, int n, const int32_t* px, const int32_t* py, const uint32_t* sidx, float* out,
                                     uint32_t* rng_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t rng;
  jvec3 o;
  const jvec3 d = camera_ray_lens(R, lens_k, px[i], py[i], sidx[i], &rng, &o);
  put3(out, 2 * i, o);
  put3(out, 2 * i + 1, d);
  rng_out[i] = rng;
}

// row i: the BSSRDF branch's exit triangle for the draw u[i] on object obj_idx[i] - the last midpoint, and what S.mapping makes of it
__global__ void k_debug_exit_search(DevScene S, int n, const int32_t* obj_idx, const float* u, int32_t* middle, int32_t* mapped) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int m = exit_search(S, obj_idx[i], u[i]);
  middle[i] = m;
  mapped[i] = S.mapping[m];
}

// A row of the shutter ray's test entries, 64 floats: the lens row's first 29 (x, y, W, H, eye[3], cam[16], A, f, u1 .. u4; A == 0: no lens),
// then ut, t_open, t_close, eye_close[3], cam_close[16], 13 unused.  The constants are formed as jade_render_begin forms them
// (shutter_const, jade_device.h).  out: origin[3], dir[3].
#define SHUTTER_ROW 64
static __host__ __device__ __forceinline__ void debug_shutter_row(const float* row, float* out) {
  const float x = row[0], y = row[1];
  const double two_over_w = 2.0 / (double)(int)row[2], two_over_h = 2.0 / (double)(int)row[3];
  const double aspect = (double)(int)row[2] / (double)(int)row[3];
  const float fx = (float)(int)x + row[25];
  const double lo = -1.0 + two_over_w * ((double)fx - 0.5);
  const float left_offset = (float)(lo * aspect);
  const float fy = (float)(int)y + row[26];
  const float up_offset = (float)(-1.0 + two_over_h * ((double)fy - 0.5));
  const float A = row[23];
  const float k = A > 0.0f ? row[24] / 1.5f : 0.0f;
  const ShutterConst H = shutter_const(row + 4, row + 7, row + 32, row + 35, row[30], row[31]);
  jvec3 o, d;
  shutter_ray(row + 7, row + 4, H, A, k, left_offset, up_offset, row[27], row[28], row[29], &o, &d);
  out[0] = o.x; out[1] = o.y; out[2] = o.z;
  out[3] = d.x; out[4] = d.y; out[5] = d.z;
}
__global__ void k_debug_shutter_ray(int n, const float* rows, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) debug_shutter_row(rows + (size_t)SHUTTER_ROW * i, out + 6 * (size_t)i);
}
// row i: the shutter ray as the shading kernel draws it, for sample sidx[i] of pixel (px[i], py[i]); the stream's state after the three or five draws
__global__ void k_debug_shutter_ray_rng(RenderConst R, ShutterConst H, float lens_k, int n, const int32_t* px, const int32_t* py, const uint32_t* sidx,
                                        float* out, uint32_t* rng_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t rng;
  jvec3 o;
  const jvec3 d = camera_ray_shutter(R, H, lens_k, px[i], py[i], sidx[i], &rng, &o);
  put3(out, 2 * i, o);
  put3(out, 2 * i + 1, d);
  rng_out[i] = rng;
}

// row i: the stratified number U (branch_number, jade_shade.h) of sample rows[5 i + 3] of pixel (rows[5 i], rows[5 i + 1]) in a render with
// frame rows[5 i + 2], at a vertex of depth rows[5 i + 4] (0 or 1)
#define BRANCH_ROW 5
static __host__ __device__ __forceinline__ uint32_t debug_branch_row(const uint32_t* row) {
  RenderConst R{};
  R.frame = row[2];
  return branch_number(R, (int)row[0], (int)row[1], row[3], row[4]);
}
__global__ void k_debug_branch_number(int n, const uint32_t* rows, uint32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = debug_branch_row(rows + (size_t)BRANCH_ROW * i);
}

// the shading normal of row i (jade_debug_shading_normal, below): the record of row i is entry i of `table`
enum { SMOOTH_ROW = 27 };
__global__ void k_debug_shading_normal(int n, const float4* table, const float* rows, float* out_n, int32_t* out_rule) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rows + (size_t)SMOOTH_ROW * i;
  int32_t rule;
  put3(out_n, i, shading_normal_rule(table, i, V3(r + 18), V3(r + 21), V3(r + 24), &rule));
  out_rule[i] = rule;
}

// the texture pieces (jade_texture.h) on row i: uv(tri[i], p[i]); colour(image[i], uv[i]); the surface colour c(tri[i], p[i]).  The host checks every index.
__global__ void k_debug_surface_uv(int n, const float4* rec, const int32_t* tri, const float* p, float* out_uv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  surface_uv(rec, tri[i], V3(p + (size_t)3 * i), out_uv + (size_t)2 * i, out_uv + (size_t)2 * i + 1);
}
__global__ void k_debug_texture_fetch(int n, const float4* texels, const uint4* images, const int32_t* image, const float* uv, float* out_rgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) put3(out_rgb, i, texture_fetch(texels, images, image[i], uv[(size_t)2 * i], uv[(size_t)2 * i + 1]));
}
__global__ void k_debug_surface_colour(int n, TexTables T, const int32_t* tri, const float* p, float* out_rgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) put3(out_rgb, i, surface_colour(T, tri[i], V3(p + (size_t)3 * i)));
}

// the mapped normal of row i (jade_debug_mapped_normal, below): normal'(tri[i], p[i], r[i]) with the triangle's stored flat normal.  The host checks every index.
__global__ void k_debug_mapped_normal(int n, MapTables T, const float4* tnorm, const int32_t* tri, const float* p, const float* r, float* out_n, int32_t* out_rule) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 tn = tnorm[tri[i]];
  int32_t rule = -1;
  put3(out_n, i, mapped_normal_rule(T, tri[i], jv(tn.x, tn.y, tn.z), V3(p + (size_t)3 * i), V3(r + (size_t)3 * i), &rule));
  out_rule[i] = rule;
}

static const int32_t kDebugMaxRows = 1 << 22;  // rows per call: every index above stays far below 2^31

static hipError_t upload0(DevBuf& b, const void* src, size_t elems) {  // on the null stream: these entry points have no scene
  hipError_t e = b.alloc(4 * elems);
  if (e == hipSuccess && elems) e = hipMemcpy(b.p, src, 4 * elems, hipMemcpyHostToDevice);
  return e;
}

extern "C" {
// out0 / out1 of routine `op` of jade_fpmath.h on n rows of a, b, c (host arrays; shapes: DebugFpOp).
int jade_debug_fpmath(int device_id, int op, int32_t n, const void* a, const void* b, const void* c, void* out0, void* out1) {
  if (op < 0 || op >= FP_N_OPS) return jade_fail(JADE_ERR_INVALID, "unknown op");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  const DebugFpShape& sh = kFpShape[op];
  if (!a || (sh.b && !b) || (sh.c && !c) || !out0 || (sh.o1 && !out1)) return jade_fail(JADE_ERR_INVALID, "null argument");
  int k = 1;
  if (op == FP_RAND) {
    k = *static_cast<const int32_t*>(b);
    if (k <= 0 || (int64_t)k * n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "draw count out of range");
  }
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf ba, bb, bc, b0, b1;
  HIP_TRY(upload0(ba, a, sh.a * N));
  HIP_TRY(upload0(bb, b, sh.b_once ? (size_t)sh.b : sh.b * N));
  HIP_TRY(upload0(bc, c, sh.c_once ? (size_t)sh.c : sh.c * N));
  HIP_TRY(b0.alloc(4 * sh.o0 * N * k));
  HIP_TRY(b1.alloc(4 * sh.o1 * N * k));
  hipLaunchKernelGGL(k_debug_fpmath, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, op, n, k, ba.as<float>(), bb.as<float>(),
                     bc.as<float>(), b0.as<float>(), b1.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out0, b0.p, 4 * sh.o0 * N * k, hipMemcpyDeviceToHost));
  if (sh.o1) HIP_TRY(hipMemcpy(out1, b1.p, 4 * sh.o1 * N * k, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// out_rgb[i] = sample_hdr(scene, dirs[i]): the environment lookup every sky sample runs.
int jade_debug_sample_hdr(jade_scene* s, int32_t n, const float* dirs, float* out_rgb) {
  if (!s || !dirs || !out_rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (!s->dev.env || s->dev.env_w <= 0 || s->dev.env_h <= 0) return jade_fail(JADE_ERR_INVALID, "the scene has no environment map");
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bd, bo;
  HIP_TRY(upload(bd, dirs, 3 * N, s->stream));
  HIP_TRY(bo.alloc(N * 12));
  hipLaunchKernelGGL(k_debug_sample_hdr, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bd.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_rgb, bo.p, N * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

static int env_sample_scene_ok(const jade_scene* s) {
  if (!s->dev.env_alias || !env_importance_fits(s->dev.env_w, s->dev.env_h))
    return jade_fail(JADE_ERR_UNSUPPORTED, "the scene's environment map is not one JADE_ENV_IMPORTANCE takes");
  return JADE_OK;
}

// (out_dir[i], out_ratio[i], out_texel[i]) = env_sample's body on the uniforms u[i][0..3]: the draw of JADE_ENV_IMPORTANCE.
// out_texel: the texel in bits 0..24, bit 31 set iff the slot's own texel was taken.
int jade_debug_env_sample(jade_scene* s, int32_t n, const float* u, float* out_dir, float* out_ratio, uint32_t* out_texel) {
  if (!s || !u || !out_dir || !out_ratio || !out_texel) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (int rc = env_sample_scene_ok(s)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bu, bd, br, bt;
  HIP_TRY(upload(bu, u, 4 * N, s->stream));
  HIP_TRY(bd.alloc(N * 12));
  HIP_TRY(br.alloc(N * 4));
  HIP_TRY(bt.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_env_sample, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bu.as<float>(), bd.as<float>(),
                     br.as<float>(), bt.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_dir, bd.p, N * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_ratio, br.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_texel, bt.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// ... and the wrapper the shading kernel calls, from the RNG states rng_in[i]: rng_out[i] is the state after the draw (its count and order).
int jade_debug_env_sample_rng(jade_scene* s, int32_t n, const uint32_t* rng_in, uint32_t* rng_out, float* out_dir, float* out_ratio) {
  if (!s || !rng_in || !rng_out || !out_dir || !out_ratio) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (int rc = env_sample_scene_ok(s)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bs, bd, br;
  HIP_TRY(upload(bs, rng_in, N, s->stream));
  HIP_TRY(bd.alloc(N * 12));
  HIP_TRY(br.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_env_sample_rng, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bs.as<uint32_t>(), bd.as<float>(),
                     br.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(rng_out, bs.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_dir, bd.p, N * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_ratio, br.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// The rows jade_debug_env_mix_sample (width = MIX_ROW: u0..u4, n[3], side, technique) and jade_debug_env_mix_sample_rng (width = MIX_ROW_RNG:
// n[3], side, technique) run: every uniform lies in [0, 1] (a NaN does not) - the slot is formed from u1 x N - and the technique is
// JADE_BOUNCE_UNIFORM or JADE_BOUNCE_COSINE as a float.  The normal and the side may hold anything: no index is formed from them (the
// texel of a direction is clamped into the map, env_texel_of).  Checked on the host before anything is launched.  No HIP call.
int jade_debug_env_mix_rows(int32_t n, int32_t width, const float* rows) {
  if (!rows) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (width != MIX_ROW && width != MIX_ROW_RNG) return jade_fail(JADE_ERR_INVALID, "row width is neither the draw's nor the RNG entry's");
  if (n <= 0 || n > kDebugMaxRows / width) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  for (int32_t i = 0; i < n; ++i) {
    const float* r = rows + (size_t)width * i;
    for (int k = 0; width == MIX_ROW && k < 5; ++k)
      if (!(r[k] >= 0.0f && r[k] <= 1.0f)) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": a uniform outside [0, 1]");
    const float t = r[width - 1];
    if (!(t == (float)JADE_BOUNCE_UNIFORM || t == (float)JADE_BOUNCE_COSINE)) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": unknown bounce technique");
  }
  return JADE_OK;
}

// (out_dir[i], out_m[i], out_info[i]) = env_mix_sample_with's body on rows[i] = (u0..u4, n[3], side, technique): the draw of JADE_ENV_MIXTURE.
// out_info: the texel in bits 0..23, bit 29 = a sky draw on the wrong side, bit 30 = the hemisphere technique, bit 31 = own (sky draws).
int jade_debug_env_mix_sample(jade_scene* s, int32_t n, const float* rows, float* out_dir, float* out_m, uint32_t* out_info) {
  if (!s || !out_dir || !out_m || !out_info) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (int rc = jade_debug_env_mix_rows(n, MIX_ROW, rows)) return rc;
  if (int rc = env_sample_scene_ok(s)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bu, bd, br, bt;
  HIP_TRY(upload(bu, rows, MIX_ROW * N, s->stream));
  HIP_TRY(bd.alloc(N * 12));
  HIP_TRY(br.alloc(N * 4));
  HIP_TRY(bt.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_env_mix_sample, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bu.as<float>(), bd.as<float>(),
                     br.as<float>(), bt.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_dir, bd.p, N * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_m, br.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_info, bt.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// ... and the wrapper the shading kernel calls, on rows[i] = (n[3], side, technique) from the RNG states rng_in[i]: rng_out[i] is the state after.
int jade_debug_env_mix_sample_rng(jade_scene* s, int32_t n, const float* rows, const uint32_t* rng_in, uint32_t* rng_out, float* out_dir, float* out_m,
                                  uint32_t* out_info) {
  if (!s || !rng_in || !rng_out || !out_dir || !out_m || !out_info) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (int rc = jade_debug_env_mix_rows(n, MIX_ROW_RNG, rows)) return rc;
  if (int rc = env_sample_scene_ok(s)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bu, bs, bd, br, bt;
  HIP_TRY(upload(bu, rows, MIX_ROW_RNG * N, s->stream));
  HIP_TRY(upload(bs, rng_in, N, s->stream));
  HIP_TRY(bd.alloc(N * 12));
  HIP_TRY(br.alloc(N * 4));
  HIP_TRY(bt.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_env_mix_sample_rng, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bu.as<float>(), bs.as<uint32_t>(),
                     bd.as<float>(), br.as<float>(), bt.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(rng_out, bs.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_dir, bd.p, N * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_m, br.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_info, bt.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// out_texel[i] = env_texel_of(scene, dirs[i]) (jade_shade.h): the texel the mixture looks q up in for a hemisphere direction.  Any
// direction may be asked - the answer is clamped into the map - so the rows' check is the scene's: it has a map.
int jade_debug_env_texel_of(jade_scene* s, int32_t n, const float* dirs, uint32_t* out_texel) {
  if (!s || !dirs || !out_texel) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / 3) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (!s->dev.env || s->dev.env_w <= 0 || s->dev.env_h <= 0) return jade_fail(JADE_ERR_INVALID, "the scene has no environment map");
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bd, bo;
  HIP_TRY(upload(bd, dirs, 3 * N, s->stream));
  HIP_TRY(bo.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_env_texel_of, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bd.as<float>(), bo.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_texel, bo.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// env_alias_table (jade_scene_prep.hip) on a w x h map: out_u32x4[t] = {accept, alias, q_own, q_alias} as bits.  No HIP call.
int jade_debug_env_alias_host(int32_t w, int32_t h, const float* rgb, uint32_t* out_u32x4) {
  if (w <= 0 || h <= 0 || !rgb || !out_u32x4) return jade_fail(JADE_ERR_INVALID, "bad argument");
  if (!env_importance_fits(w, h)) return jade_fail(JADE_ERR_UNSUPPORTED, "more texels than JADE_ENV_IMPORTANCE_MAX_TEXELS");
  std::vector<uint4> table;
  env_alias_table(w, h, rgb, table);
  for (size_t t = 0; t < table.size(); ++t) {
    out_u32x4[4 * t] = table[t].x;
    out_u32x4[4 * t + 1] = table[t].y;
    out_u32x4[4 * t + 2] = table[t].z;
    out_u32x4[4 * t + 3] = table[t].w;
  }
  return JADE_OK;
}

// light_alias_table (jade_scene_prep.hip) on the n_emit entries emit_indices of n_triangles caller's records: out_u32x4[i] = {accept, alias,
// q_own, q_alias} as bits.  No HIP call.
int jade_debug_light_table_host(const jade_triangle* triangles, int32_t n_triangles, const int32_t* emit_indices, int32_t n_emit, uint32_t* out_u32x4) {
  if (!triangles || n_triangles <= 0 || n_emit < 0 || (n_emit > 0 && (!emit_indices || !out_u32x4))) return jade_fail(JADE_ERR_INVALID, "bad argument");
  if (!light_sampling_fits(n_emit)) return jade_fail(JADE_ERR_UNSUPPORTED, "more emitter entries than JADE_LIGHTS_ONE_MAX_ENTRIES");
  for (int32_t i = 0; i < n_emit; ++i)
    if (emit_indices[i] < 0 || emit_indices[i] >= n_triangles) return jade_fail(JADE_ERR_INVALID, "emitter index out of range");
  std::vector<uint4> table;
  light_alias_table(triangles, emit_indices, n_emit, table);
  for (size_t t = 0; t < table.size(); ++t) {
    out_u32x4[4 * t] = table[t].x;
    out_u32x4[4 * t + 1] = table[t].y;
    out_u32x4[4 * t + 2] = table[t].z;
    out_u32x4[4 * t + 3] = table[t].w;
  }
  return JADE_OK;
}

// (out_entry[i], out_rxy[i][0..1], out_weight[i][0..1]) = light_sample's body on the uniforms u[i][0..3], over the scene's own table: the
// draw of JADE_LIGHTS_ONE.  out_weight: {the draw's weight, light_weight of the entry drawn}.
int jade_debug_light_sample(jade_scene* s, int32_t n, const float* u, uint32_t* out_entry, float* out_rxy, float* out_weight) {
  if (!s || !u || !out_entry || !out_rxy || !out_weight) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (s->n_emit <= 0 || !light_sampling_fits(s->n_emit) || s->b_light_alias.bytes != (size_t)s->n_emit * sizeof(uint4))
    return jade_fail(JADE_ERR_UNSUPPORTED, "the scene's emitter list is not one JADE_LIGHTS_ONE draws from");
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bu, be, bx, bw;
  HIP_TRY(upload(bu, u, 4 * N, s->stream));
  HIP_TRY(be.alloc(N * 4));
  HIP_TRY(bx.alloc(N * 8));
  HIP_TRY(bw.alloc(N * 8));
  hipLaunchKernelGGL(k_debug_light_sample, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, (const uint4*)s->b_light_alias.as<uint4>(),
                     (uint32_t)s->n_emit, n, bu.as<float>(), be.as<uint32_t>(), bx.as<float>(), bw.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_entry, be.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_rxy, bx.p, N * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_weight, bw.p, N * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// mis_table (jade_scene_prep.hip) on n_triangles caller's records and the n_emit entries emit_indices, with light_alias_table's table
// where that is made: out_m_M[2 h] = m(h), out_m_M[2 h + 1] = M(h).  No HIP call.
int jade_debug_mis_table_host(const jade_triangle* triangles, int32_t n_triangles, const int32_t* emit_indices, int32_t n_emit, float* out_m_M) {
  if (!triangles || n_triangles <= 0 || n_emit < 0 || (n_emit > 0 && !emit_indices) || !out_m_M) return jade_fail(JADE_ERR_INVALID, "bad argument");
  for (int32_t i = 0; i < n_emit; ++i)
    if (emit_indices[i] < 0 || emit_indices[i] >= n_triangles) return jade_fail(JADE_ERR_INVALID, "emitter index out of range");
  std::vector<uint4> alias;
  if (light_sampling_fits(n_emit)) light_alias_table(triangles, emit_indices, n_emit, alias);
  std::vector<float2> table;
  mis_table(triangles, n_triangles, emit_indices, n_emit, alias, table);
  for (size_t h = 0; h < table.size(); ++h) {
    out_m_M[2 * h] = table[h].x;
    out_m_M[2 * h + 1] = table[h].y;
  }
  return JADE_OK;
}

// out[i] = (w_L, T_B of one channel) of mis_terms (jade_shade.h) on rows[i] = (n[3], ne[3], A, m, mu, l[3], Le, f), 14 floats.
int jade_debug_mis_terms(int device_id, int32_t n, const float* rows, float* out) {
  if (!rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / 14) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bo;
  HIP_TRY(upload0(bi, rows, 14 * N));
  HIP_TRY(bo.alloc(8 * N));
  hipLaunchKernelGGL(k_debug_mis_terms, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, bo.p, 8 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// out_dir[i], out_fallback[i] = the draw of JADE_BOUNCE_COSINE (cosine_dir_with, jade_shade.h) on rows[i] = (n[3], s, u1, u2), 6 floats.
int jade_debug_bounce_dir(int device_id, int32_t n, const float* rows, float* out_dir, int32_t* out_fallback) {
  if (!rows || !out_dir || !out_fallback) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / 6) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bd, bf;
  HIP_TRY(upload0(bi, rows, 6 * N));
  HIP_TRY(bd.alloc(12 * N));
  HIP_TRY(bf.alloc(4 * N));
  hipLaunchKernelGGL(k_debug_bounce_dir, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<float>(), bd.as<float>(), bf.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out_dir, bd.p, 12 * N, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_fallback, bf.p, 4 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// ... and as bounce_branch draws it: rows[i] = (n[3], s), 4 floats, from the RNG states rng_in[i]; rng_out[i] is the state after the draw.
int jade_debug_bounce_dir_rng(int device_id, int32_t n, const float* rows, const uint32_t* rng_in, uint32_t* rng_out, float* out_dir) {
  if (!rows || !rng_in || !rng_out || !out_dir) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / 4) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bs, bd;
  HIP_TRY(upload0(bi, rows, 4 * N));
  HIP_TRY(upload0(bs, rng_in, N));
  HIP_TRY(bd.alloc(12 * N));
  hipLaunchKernelGGL(k_debug_bounce_dir_rng, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<float>(), bs.as<uint32_t>(), bd.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(rng_out, bs.p, 4 * N, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_dir, bd.p, 12 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// The map sizes jade_render_begin takes with JADE_ENV_IMPORTANCE (its own predicate, env_importance_fits): 1 / 0.  No HIP call.
int jade_debug_env_importance_fits(int32_t w, int32_t h) { return env_importance_fits(w, h) ? 1 : 0; }

// out_bgr[i] = tone_pack_bgr8(rgb[i], tonemap, limit, valid = true): k_resolve's and k_dn_out's statements.
int jade_debug_tone_pack(int device_id, int32_t n, const float* rgb, int tonemap, float limit, uint8_t* out_bgr) {
  if (!rgb || !out_bgr) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (tonemap != JADE_TONEMAP_ACES && tonemap != JADE_TONEMAP_REINHARD) return jade_fail(JADE_ERR_INVALID, "unknown tone operator");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bo;
  HIP_TRY(upload0(bi, rgb, 3 * N));
  HIP_TRY(bo.alloc(3 * N));
  hipLaunchKernelGGL(k_debug_tone_pack, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<float>(), tonemap, limit, bo.as<uint8_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out_bgr, bo.p, 3 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// ... and the same function compiled for the HOST: what jade_render_multi packs the gathered frame with (jade_multi.hip).  No HIP call.
int jade_debug_tone_pack_host(int32_t n, const float* rgb, int tonemap, float limit, uint8_t* out_bgr) {
  if (n < 0 || !rgb || !out_bgr) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (tonemap != JADE_TONEMAP_ACES && tonemap != JADE_TONEMAP_REINHARD) return jade_fail(JADE_ERR_INVALID, "unknown tone operator");
  for (int32_t i = 0; i < n; ++i) {
    const float* m = rgb + 3 * (size_t)i;
    tone_pack_bgr8(jv(m[0], m[1], m[2]), tonemap, limit, true, out_bgr + 3 * (size_t)i);
  }
  return JADE_OK;
}

// The lens ray (lens_ray, jade_device.h; include/jade_bvh.h "The lens, stated") on n rows of LENS_ROW floats (above): out[i] = origin[3],
// dir[3].  The HOST build of the function, no HIP call: what tests/test_lens_cpu.py holds against the float64 statement.
int jade_debug_lens_ray_host(int32_t n, const float* rows, float* out) {
  if (n < 0 || !rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  for (int32_t i = 0; i < n; ++i) debug_lens_row(rows + (size_t)LENS_ROW * i, out + 6 * (size_t)i);
  return JADE_OK;
}

// ... and the same rows on the device.
int jade_debug_lens_ray(int device_id, int32_t n, const float* rows, float* out) {
  if (!rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / LENS_ROW) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bo;
  HIP_TRY(upload0(bi, rows, LENS_ROW * N));
  HIP_TRY(bo.alloc(24 * N));
  hipLaunchKernelGGL(k_debug_lens_ray, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, bo.p, 24 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// The lens ray from the stream, as the render draws it: sample sidx[i] of pixel (px[i], py[i]) of a width x height frame from (eye,
// camera) with `frame`, under lens (A, f).  out[i] = origin[3], dir[3]; rng_out[i] = the stream's state after the four draws.
int jade_debug_lens_ray_rng(int device_id, int32_t n, int32_t width, int32_t height, uint32_t frame, const float* eye, const float* camera, float A, float f,
                            const int32_t* px, const int32_t* py, const uint32_t* sidx, float* out, uint32_t* rng_out) {
  if (!eye || !camera || !px || !py || !sidx || !out || !rng_out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows || width <= 0 || height <= 0) return jade_fail(JADE_ERR_INVALID, "row count or frame size out of range");
  HIP_TRY(hipSetDevice(device_id));
  RenderConst R{};
  R.width = width; R.height = height; R.tiles_x = (width + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE; R.frame = frame;
  memcpy(R.eye, eye, sizeof R.eye);
  memcpy(R.cam, camera, sizeof R.cam);
  R.lens_radius = A;
  R.two_over_w = 2.0 / (double)width;   // (jade_render_begin's statements)
  R.two_over_h = 2.0 / (double)height;
  R.aspect = (double)width / (double)height;
  const size_t N = (size_t)n;
  DevBuf bx, by, bs, bo, br;
  HIP_TRY(upload0(bx, px, N));
  HIP_TRY(upload0(by, py, N));
  HIP_TRY(upload0(bs, sidx, N));
  HIP_TRY(bo.alloc(24 * N));
  HIP_TRY(br.alloc(4 * N));
  hipLaunchKernelGGL(k_debug_lens_ray_rng, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, R, f / 1.5f, n, bx.as<int32_t>(), by.as<int32_t>(),
                     bs.as<uint32_t>(), bo.as<float>(), br.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, bo.p, 24 * N, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rng_out, br.p, 4 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}
// guide_tables (jade_scene_prep.hip) on the caller's arrays: out_guide_obj[2 o] = object o's first entry, [2 o + 1] = its cells Gn (0:
// no table, the kernel bisects); out_guide[0 .. *out_n_guide) = the entries.  guide_cap: the entries out_guide holds (the tables never
// need more than 8 x n_triangles + 2 x n_objects + 1 when the objects' segments are disjoint; more is refused, nothing is written past
// it).  Of the desc only n_triangles, n_objects, prefix_area and obj_segs are read, and the segments are checked as jade_scene_create
// checks them.  No HIP call.
int jade_debug_guide_tables_host(const jade_scene_desc* d, uint32_t* out_guide_obj, uint32_t* out_guide, int32_t guide_cap, int32_t* out_n_guide) {
  if (!d || !out_guide_obj || !out_guide || !out_n_guide || guide_cap < 0) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (d->n_triangles <= 0 || d->n_objects <= 0 || !d->prefix_area || !d->obj_segs) return jade_fail(JADE_ERR_INVALID, "missing prefix areas / object segments");
  for (int i = 0; i < d->n_objects; ++i)
    if (d->obj_segs[i].begin_idx < 0 || d->obj_segs[i].end_idx >= d->n_triangles || d->obj_segs[i].begin_idx > d->obj_segs[i].end_idx)
      return jade_fail(JADE_ERR_INVALID, "object segment out of range");
  std::vector<uint32_t> guide;
  std::vector<uint2> guide_obj;
  guide_tables(d, guide, guide_obj);
  if (guide.size() > (size_t)guide_cap) return jade_fail(JADE_ERR_INVALID, "out_guide is too small");
  for (size_t o = 0; o < guide_obj.size(); ++o) {
    out_guide_obj[2 * o] = guide_obj[o].x;
    out_guide_obj[2 * o + 1] = guide_obj[o].y;
  }
  memcpy(out_guide, guide.data(), 4 * guide.size());
  *out_n_guide = (int32_t)guide.size();
  return JADE_OK;
}

// validate_desc + prepare_scene (jade_scene_prep.hip) on the caller's descriptor, as jade_scene_create runs them, and what they made:
// the binary records, the wide records (none unless wide_mode > 0, or < 0 and the records outgrow the L2: Tunables.wide_mode - the
// environment is not read) and the pair records, as float4s, and info[0 .. 11) = their three counts in float4s, root_ref, n_internal,
// n_pairs, missing_child, nested, wide_fits, cache_fits, the tree's levels.  cap[3]: the float4s each array holds (4, 8 and 40 x n_nodes
// always do); more is refused, nothing is written past it.  A descriptor jade_scene_create refuses is refused with the same code.  No HIP
// call (tests/test_scene_prep_cpu.py).
int jade_debug_prepare_scene_host(const jade_scene_desc* d, int32_t wide_mode, const int64_t cap[3], float* out_nodes, float* out_nodes4, float* out_tverts,
                                  int64_t info[11]) {
  if (!d || !cap || !out_nodes || !out_nodes4 || !out_tverts || !info) return jade_fail(JADE_ERR_INVALID, "null argument");
  int depth = 0;
  if (int rc = validate_desc(d, &depth)) return rc;
  Tunables tun;
  tun.wide_mode = wide_mode;
  ScenePrep p;
  if (int rc = prepare_scene(*d, depth, tun, &p)) return rc;
  if ((int64_t)p.nodes.size() > cap[0] || (int64_t)p.nodes4.size() > cap[1] || (int64_t)p.tverts.size() > cap[2]) return jade_fail(JADE_ERR_INVALID, "an output array is too small");
  memcpy(out_nodes, p.nodes.data(), sizeof(float4) * p.nodes.size());
  if (!p.nodes4.empty()) memcpy(out_nodes4, p.nodes4.data(), sizeof(float4) * p.nodes4.size());
  memcpy(out_tverts, p.tverts.data(), sizeof(float4) * p.tverts.size());
  const int64_t v[11] = {(int64_t)p.nodes.size(), (int64_t)p.nodes4.size(), (int64_t)p.tverts.size(), (int64_t)p.root_ref, p.n_internal, (int64_t)p.n_pairs,
                         p.missing_child, p.nested, p.wide_fits, p.cache_fits, depth};
  memcpy(info, v, sizeof v);
  return JADE_OK;
}

// The two queue rules of jade_runtime.h as setup_state and launch_trace use them (tests/test_queue_rules_cpu.py): the ray-record boundary of a
// queue of `slots` positions (enabled: Tunables.ray_records; hook: JADE_RAYQ_CAP), and the rays a wave of k_trace claims per queue atomic in a
// launch of n_rays over `waves` waves (hook: JADE_TRACE_CHUNK_RAYS).  The environment is not read.  No HIP call.
int64_t jade_debug_ray_record_cap_host(uint64_t slots, int32_t enabled, int64_t hook) { return (int64_t)ray_record_cap((size_t)slots, enabled != 0, hook); }
uint32_t jade_debug_trace_chunk_host(uint32_t n_rays, uint64_t waves, uint32_t hook) { return trace_chunk_for(n_rays, waves, hook); }

// What jade_render_begin makes of a render's settings (shade_mode_for, jade_runtime.h; tests/test_shade_modes_cpu.py): JADE_OK and the mode's
// bits in *mode, or the refusal's code - returned, with its text in jade_last_error() - and *mode untouched.  No HIP call.
int jade_debug_shade_mode_host(int32_t env_importance, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                               uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_importance != 0 ? JADE_ENV_IMPORTANCE : JADE_ENV_REFERENCE, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why)) return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// ... and with the value of jade_render_params.env_sampling (JADE_ENV_*; any other value is JADE_ERR_INVALID, as jade_render_begin answers it).
int jade_debug_shade_mode_env_host(int32_t env_sampling, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                                   uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (env_sampling != JADE_ENV_REFERENCE && env_sampling != JADE_ENV_IMPORTANCE && env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_sampling, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why)) return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// ... and with jade_scene_set_passes' value (tests/test_passes_cpu.py).
int jade_debug_shade_mode_passes_host(int32_t env_sampling, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                                      int32_t passes, uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (env_sampling != JADE_ENV_REFERENCE && env_sampling != JADE_ENV_IMPORTANCE && env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_sampling, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why, passes != 0)) return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// ... and with jade_scene_set_branch_sampling's value (JADE_BRANCH_*; any other is JADE_ERR_INVALID, as the setter answers it; tests/test_branch_cpu.py).
int jade_debug_shade_mode_branch_host(int32_t env_sampling, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                                      int32_t passes, int32_t branch_sampling, uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (env_sampling != JADE_ENV_REFERENCE && env_sampling != JADE_ENV_IMPORTANCE && env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  if (branch_sampling != JADE_BRANCH_RANDOM && branch_sampling != JADE_BRANCH_STRATIFIED) return jade_fail(JADE_ERR_INVALID, "unknown branch sampling (JADE_BRANCH_*)");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_sampling, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why, passes != 0,
                                    branch_sampling == JADE_BRANCH_STRATIFIED))
    return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// ... and with whether the handle carries vertex normals that are not flat everywhere (jade_scene_set_vertex_normals; tests/test_smooth_modes_cpu.py).
int jade_debug_shade_mode_smooth_host(int32_t env_sampling, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                                      int32_t passes, int32_t branch_sampling, int32_t smooth, uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (env_sampling != JADE_ENV_REFERENCE && env_sampling != JADE_ENV_IMPORTANCE && env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  if (branch_sampling != JADE_BRANCH_RANDOM && branch_sampling != JADE_BRANCH_STRATIFIED) return jade_fail(JADE_ERR_INVALID, "unknown branch sampling (JADE_BRANCH_*)");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_sampling, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why, passes != 0,
                                    branch_sampling == JADE_BRANCH_STRATIFIED, smooth != 0))
    return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// The shading normal (shading_normal_rule, jade_smooth.h; include/jade_bvh.h "The shading normal, stated") on n rows of SMOOTH_ROW floats:
// p1, p2, p3, n1, n2, n3, g, p, r (27).  Each row's record is made by smooth_record, as jade_scene_set_vertex_normals makes it;
// out_n[i] = the normal the vertex uses, out_rule[i] = which rule gave it (SMOOTH_RULE_*; tests/test_gpu_smooth.py).
int jade_debug_shading_normal(int device_id, int32_t n, const float* rows, float* out_n, int32_t* out_rule) {
  if (!rows || !out_n || !out_rule) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / SMOOTH_ROW) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  std::vector<float4> rec(N * JADE_SMOOTH_REC);
  for (size_t i = 0; i < N; ++i) {
    const float* r = rows + SMOOTH_ROW * i;
    smooth_record(r, r + 3, r + 6, r + 9, r + 18, &rec[i * JADE_SMOOTH_REC]);
  }
  DevBuf bt, bi, bn, br;
  HIP_TRY(upload0(bt, rec.data(), 4 * rec.size()));  // (upload0 counts 4-byte elements: a record is JADE_SMOOTH_REC float4)
  HIP_TRY(upload0(bi, rows, SMOOTH_ROW * N));
  HIP_TRY(bn.alloc(12 * N));
  HIP_TRY(br.alloc(4 * N));
  hipLaunchKernelGGL(k_debug_shading_normal, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bt.as<float4>(), bi.as<float>(), bn.as<float>(), br.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out_n, bn.p, 12 * N, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_rule, br.p, 4 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// ... and with whether the handle carries textures in which a triangle names an image (jade_scene_set_textures; tests/test_texture_modes_cpu.py).
int jade_debug_shade_mode_textures_host(int32_t env_sampling, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                                        int32_t passes, int32_t branch_sampling, int32_t smooth, int32_t textures, uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (env_sampling != JADE_ENV_REFERENCE && env_sampling != JADE_ENV_IMPORTANCE && env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  if (branch_sampling != JADE_BRANCH_RANDOM && branch_sampling != JADE_BRANCH_STRATIFIED) return jade_fail(JADE_ERR_INVALID, "unknown branch sampling (JADE_BRANCH_*)");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_sampling, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why, passes != 0,
                                    branch_sampling == JADE_BRANCH_STRATIFIED, smooth != 0, textures != 0))
    return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// The pieces of "The surface colour, stated" (include/jade_bvh.h; jade_texture.h) on n rows, with the table the handle carries as
// jade_scene_set_textures left it (no render is begun; tests/test_gpu_texture.py):
//   jade_debug_surface_uv:      out_uv[i] = uv(tri[i], points[i])
//   jade_debug_texture_fetch:   out_rgb[i] = colour(image[i], uv[i])
//   jade_debug_surface_colour:  out_rgb[i] = c(tri[i], points[i]), (1, 1, 1) for a triangle without an image
struct DebugTextures {
  DevBuf rec, texels, images;
  TexTables T{};
};
static int debug_textures(jade_scene* s, int32_t n, const int32_t* index, int32_t index_lo, size_t index_n, DebugTextures* d) {
  if (n <= 0 || n > kDebugMaxRows / 4) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  if (s->surf.set.textures.rec.empty()) return jade_fail(JADE_ERR_INVALID, "the scene carries no textures (jade_scene_set_textures)");
  for (int32_t i = 0; i < n; ++i)
    if (index[i] < index_lo || (size_t)index[i] >= index_n) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": index out of range");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(upload(d->rec, s->surf.set.textures.rec.data(), s->surf.set.textures.rec.size(), s->stream));
  HIP_TRY(upload(d->texels, s->surf.set.textures.texels.data(), s->surf.set.textures.texels.size(), s->stream));
  HIP_TRY(upload(d->images, s->surf.set.textures.images.data(), s->surf.set.textures.images.size(), s->stream));
  d->T = TexTables{nullptr, d->rec.as<float4>(), d->texels.as<float4>(), d->images.as<uint4>()};
  return JADE_OK;
}
int jade_debug_surface_uv(jade_scene* s, int32_t n, const int32_t* tri, const float* points, float* out_uv) {
  if (!s || !tri || !points || !out_uv) return jade_fail(JADE_ERR_INVALID, "null argument");
  DebugTextures d;
  if (const int rc = debug_textures(s, n, tri, 0, s->surf.set.textures.rec.size() / JADE_TEX_REC, &d)) return rc;
  const size_t N = (size_t)n;
  DevBuf bt, bp, bo;
  HIP_TRY(upload(bt, tri, N, s->stream));
  HIP_TRY(upload(bp, points, 3 * N, s->stream));
  HIP_TRY(bo.alloc(8 * N));
  hipLaunchKernelGGL(k_debug_surface_uv, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, n, d.T.rec, bt.as<int32_t>(), bp.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_uv, bo.p, 8 * N, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}
int jade_debug_texture_fetch(jade_scene* s, int32_t n, const int32_t* image, const float* uv, float* out_rgb) {
  if (!s || !image || !uv || !out_rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  DebugTextures d;
  if (const int rc = debug_textures(s, n, image, 0, s->surf.set.textures.images.size(), &d)) return rc;
  const size_t N = (size_t)n;
  DevBuf bi, bu, bo;
  HIP_TRY(upload(bi, image, N, s->stream));
  HIP_TRY(upload(bu, uv, 2 * N, s->stream));
  HIP_TRY(bo.alloc(12 * N));
  hipLaunchKernelGGL(k_debug_texture_fetch, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, n, d.T.texels, d.T.images, bi.as<int32_t>(), bu.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_rgb, bo.p, 12 * N, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}
int jade_debug_surface_colour(jade_scene* s, int32_t n, const int32_t* tri, const float* points, float* out_rgb) {
  if (!s || !tri || !points || !out_rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  DebugTextures d;
  if (const int rc = debug_textures(s, n, tri, 0, s->surf.set.textures.rec.size() / JADE_TEX_REC, &d)) return rc;
  const size_t N = (size_t)n;
  DevBuf bt, bp, bo;
  HIP_TRY(upload(bt, tri, N, s->stream));
  HIP_TRY(upload(bp, points, 3 * N, s->stream));
  HIP_TRY(bo.alloc(12 * N));
  hipLaunchKernelGGL(k_debug_surface_colour, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, n, d.T, bt.as<int32_t>(), bp.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_rgb, bo.p, 12 * N, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// ... and with whether the handle carries normal maps in which a triangle is mapped (jade_scene_set_normal_maps; tests/test_normal_map_modes_cpu.py):
// the full rule.
int jade_debug_shade_mode_normal_maps_host(int32_t env_sampling, int32_t lens, int32_t shutter, int32_t light_sampling, int32_t bounce_sampling, int32_t direct_sampling,
                                           int32_t passes, int32_t branch_sampling, int32_t smooth, int32_t textures, int32_t normal_maps, uint32_t* mode) {
  if (!mode) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (env_sampling != JADE_ENV_REFERENCE && env_sampling != JADE_ENV_IMPORTANCE && env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  if (branch_sampling != JADE_BRANCH_RANDOM && branch_sampling != JADE_BRANCH_STRATIFIED) return jade_fail(JADE_ERR_INVALID, "unknown branch sampling (JADE_BRANCH_*)");
  uint32_t m = 0;
  std::string why;
  if (const int rc = shade_mode_for(env_sampling, lens != 0, shutter != 0, light_sampling, bounce_sampling, direct_sampling, &m, &why, passes != 0,
                                    branch_sampling == JADE_BRANCH_STRATIFIED, smooth != 0, textures != 0, normal_maps != 0))
    return jade_fail(rc, why);
  *mode = m;
  return JADE_OK;
}

// The mapped normal (mapped_normal_rule, jade_normal_map.h; include/jade_bvh.h "The mapped normal, stated") on n rows, with the tables the handle
// carries as jade_scene_set_normal_maps and jade_scene_set_vertex_normals left them, joined as jade_render_begin joins them (surface_join_maps; no render is begun;
// tests/test_gpu_normal_map.py): out_n[i] = normal'(tri[i], points[i], refs[i]), out_rule[i] = the SMOOTH_RULE_* that gave it.
int jade_debug_mapped_normal(jade_scene* s, int32_t n, const int32_t* tri, const float* points, const float* refs, float* out_n, int32_t* out_rule) {
  if (!s || !tri || !points || !refs || !out_n || !out_rule) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / 4) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  const auto& set = s->surf.set;
  if (set.maps.rec.empty()) return jade_fail(JADE_ERR_INVALID, "the scene carries no normal maps (jade_scene_set_normal_maps)");
  const size_t n_tris = set.maps.rec.size() / JADE_NMAP_REC;
  for (int32_t i = 0; i < n; ++i)
    if (tri[i] < 0 || (size_t)tri[i] >= n_tris) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": index out of range");
  HIP_TRY(hipSetDevice(s->device));
  const std::vector<float4> rec = surface_join_maps(s->surf);
  std::vector<float4> flat;
  if (set.normals.empty()) flat.assign(n_tris * JADE_SMOOTH_REC, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  DevBuf brec, btex, bimg, bsm, bt, bp, br, bn, bo;
  HIP_TRY(upload(brec, rec.data(), rec.size(), s->stream));
  HIP_TRY(upload(btex, set.maps.texels.data(), set.maps.texels.size(), s->stream));
  HIP_TRY(upload(bimg, set.maps.images.data(), set.maps.images.size(), s->stream));
  HIP_TRY(upload(bsm, set.normals.empty() ? flat.data() : set.normals.data(), n_tris * JADE_SMOOTH_REC, s->stream));
  const size_t N = (size_t)n;
  HIP_TRY(upload(bt, tri, N, s->stream));
  HIP_TRY(upload(bp, points, 3 * N, s->stream));
  HIP_TRY(upload(br, refs, 3 * N, s->stream));
  HIP_TRY(bn.alloc(12 * N));
  HIP_TRY(bo.alloc(4 * N));
  const MapTables T{TexTables{bsm.as<float4>(), nullptr, nullptr, nullptr}, brec.as<float4>(), btex.as<float4>(), bimg.as<uint4>(), set.strength};
  hipLaunchKernelGGL(k_debug_mapped_normal, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, n, T, s->b_tnorm.as<float4>(), bt.as<int32_t>(), bp.as<float>(),
                     br.as<float>(), bn.as<float>(), bo.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_n, bn.p, 12 * N, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_rule, bo.p, 4 * N, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// The stratified number of the branch draws (branch_number, jade_shade.h; include/jade_bvh.h "The branch draws, stated") on n rows of
// BRANCH_ROW uint32 (x, y, frame, sidx, depth; depth 0 or 1): out[i] = U.  The HOST build of the function, no HIP call (tests/test_branch_cpu.py).
int jade_debug_branch_number_host(int32_t n, const uint32_t* rows, uint32_t* out) {
  if (n < 0 || !rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  for (int32_t i = 0; i < n; ++i) {
    if (rows[(size_t)BRANCH_ROW * i + 4] > 1u) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": depth is 0 or 1");
    out[i] = debug_branch_row(rows + (size_t)BRANCH_ROW * i);
  }
  return JADE_OK;
}
// ... and the same rows on the device (tests/test_gpu_branch.py).
int jade_debug_branch_number(int device_id, int32_t n, const uint32_t* rows, uint32_t* out) {
  if (!rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / BRANCH_ROW) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  for (int32_t i = 0; i < n; ++i)
    if (rows[(size_t)BRANCH_ROW * i + 4] > 1u) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": depth is 0 or 1");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bo;
  HIP_TRY(upload0(bi, rows, BRANCH_ROW * N));
  HIP_TRY(bo.alloc(4 * N));
  hipLaunchKernelGGL(k_debug_branch_number, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<uint32_t>(), bo.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, bo.p, 4 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// The rows jade_debug_exit_search runs: every obj_idx[i] names an object and every u[i] lies in [0, 1] (a NaN does not).  exit_search
// forms its table cell from u x Gn: a row outside that range would read past the object's table - a wild read on a device, which no
// assertion there could catch - so the rows are refused here, on the host, before anything is launched.  No HIP call.
int jade_debug_exit_search_rows(int32_t n_objects, int32_t n, const int32_t* obj_idx, const float* u) {
  if (!obj_idx || !u) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  for (int32_t i = 0; i < n; ++i) {
    if (obj_idx[i] < 0 || obj_idx[i] >= n_objects) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": obj_idx out of range");
    if (!(u[i] >= 0.0f && u[i] <= 1.0f)) return jade_fail(JADE_ERR_INVALID, "row " + std::to_string(i) + ": u outside [0, 1]");
  }
  return JADE_OK;
}

// out_middle[i] = exit_search(scene, obj_idx[i], u[i]) (jade_shade.h: the BSSRDF branch's search, before the mapping), out_mapped[i] =
// index_mapping[out_middle[i]]: one thread per row.  Every row is checked first (jade_debug_exit_search_rows; a null scene has no objects).
int jade_debug_exit_search(jade_scene* s, int32_t n, const int32_t* obj_idx, const float* u, int32_t* out_middle, int32_t* out_mapped) {
  if (!out_middle || !out_mapped) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (int rc = jade_debug_exit_search_rows(s ? s->n_objects : 0, n, obj_idx, u)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bo, bu, bm, bp;
  HIP_TRY(upload(bo, obj_idx, N, s->stream));
  HIP_TRY(upload(bu, u, N, s->stream));
  HIP_TRY(bm.alloc(N * 4));
  HIP_TRY(bp.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_exit_search, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bo.as<int32_t>(), bu.as<float>(),
                     bm.as<int32_t>(), bp.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_middle, bm.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_mapped, bp.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// The shutter ray (shutter_ray, jade_device.h; include/jade_bvh.h "The shutter, stated") on n rows of SHUTTER_ROW floats (above): out[i] =
// origin[3], dir[3].  The HOST build of the function, no HIP call: what tests/test_shutter_cpu.py holds against the float64 statement.
int jade_debug_shutter_ray_host(int32_t n, const float* rows, float* out) {
  if (n < 0 || !rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  for (int32_t i = 0; i < n; ++i) debug_shutter_row(rows + (size_t)SHUTTER_ROW * i, out + 6 * (size_t)i);
  return JADE_OK;
}

// ... and the same rows on the device.
int jade_debug_shutter_ray(int device_id, int32_t n, const float* rows, float* out) {
  if (!rows || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows / SHUTTER_ROW) return jade_fail(JADE_ERR_INVALID, "row count out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t N = (size_t)n;
  DevBuf bi, bo;
  HIP_TRY(upload0(bi, rows, SHUTTER_ROW * N));
  HIP_TRY(bo.alloc(24 * N));
  hipLaunchKernelGGL(k_debug_shutter_ray, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, n, bi.as<float>(), bo.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, bo.p, 24 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}

// The shutter ray from the stream, as the render draws it: sample sidx[i] of pixel (px[i], py[i]) of a width x height frame from (eye,
// camera) with `frame`, under lens (A, f) - A == 0: none - and the shutter `sh`.  out[i] = origin[3], dir[3]; rng_out[i] = the stream's
// state after the three (no lens) or five draws.
int jade_debug_shutter_ray_rng(int device_id, int32_t n, int32_t width, int32_t height, uint32_t frame, const float* eye, const float* camera, float A, float f,
                               const jade_shutter_params* sh, const int32_t* px, const int32_t* py, const uint32_t* sidx, float* out, uint32_t* rng_out) {
  if (!eye || !camera || !sh || !px || !py || !sidx || !out || !rng_out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n <= 0 || n > kDebugMaxRows || width <= 0 || height <= 0) return jade_fail(JADE_ERR_INVALID, "row count or frame size out of range");
  HIP_TRY(hipSetDevice(device_id));
  RenderConst R{};
  R.width = width; R.height = height; R.tiles_x = (width + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE; R.frame = frame;
  memcpy(R.eye, eye, sizeof R.eye);
  memcpy(R.cam, camera, sizeof R.cam);
  R.lens_radius = A > 0.0f ? A : 0.0f;
  R.two_over_w = 2.0 / (double)width;   // (jade_render_begin's statements)
  R.two_over_h = 2.0 / (double)height;
  R.aspect = (double)width / (double)height;
  const ShutterConst H = shutter_const(eye, camera, sh->eye_close, sh->camera_close, sh->t_open, sh->t_close);
  const size_t N = (size_t)n;
  DevBuf bx, by, bs, bo, br;
  HIP_TRY(upload0(bx, px, N));
  HIP_TRY(upload0(by, py, N));
  HIP_TRY(upload0(bs, sidx, N));
  HIP_TRY(bo.alloc(24 * N));
  HIP_TRY(br.alloc(4 * N));
  hipLaunchKernelGGL(k_debug_shutter_ray_rng, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, R, H, A > 0.0f ? f / 1.5f : 0.0f, n, bx.as<int32_t>(),
                     by.as<int32_t>(), bs.as<uint32_t>(), bo.as<float>(), br.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, bo.p, 24 * N, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rng_out, br.p, 4 * N, hipMemcpyDeviceToHost));
  return JADE_OK;
}
}  // extern "C"

#endif  // JADE_DEBUG_EXPORTS
