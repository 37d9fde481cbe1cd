// jade_denoise.hip — the denoiser (include/jade_bvh.h: jade_render_guides, jade_render_denoise, jade_denoise_image): kernels and host side.
//
//   k_pixel_variance  one block of 256 threads per tile: each pixel's lanes of partial sums -> the variance of its mean luminance
//                     (lane_moments, jade_lanes.h: k_tile_error's statements)
//   k_guide_camera    the guide pass: one camera ray per owned in-image pixel (camera_ray_dir, jade_device.h) into a throw-away
//                     PathState that k_trace walks unchanged (reference walk, nearest hit)
//   k_guide_hits      consumes k_trace's hits: a mirror vertex queues the reflected ray for the next k_trace launch; a final vertex or
//                     a miss adds the sample's albedo, normal and depth to the pixel's sums.  A pixel has one ray in flight at a time
//                     and the host runs the samples one after the other, so every pixel adds its samples in increasing s whatever
//                     order the queue's atomics give
//   k_dn_pack_tiles   the render's compact tiles (resolve, variance, guide sums) -> the filter's records in image layout
//   k_dn_pack_image   the same records from caller-provided images (jade_denoise_image)
//   k_atrous          one a-trous pass (jade_bvh.h's formulas), ping-pong between two colour buffers, no atomics
//   k_dn_out          the filtered colour -> linear RGB and BGR8 (tone_pack_bgr8, jade_device.h: k_resolve's statements)
//
// The filter's record of a pixel is three float4: A = {r, g, b, variance} (the only part a pass writes), N = {nhat, depth},
// L = {albedo, 0}.  A tap reads 48 B, from L2: a 5x5 footprint at step 2^i touches the same lines for neighbouring pixels.
// The guide pass's rays are walked by k_trace, which lives in jade_hip.hip: launch_trace (jade_runtime.h).
#include <math.h>

#include <cmath>
#include <cstring>

#include "jade_lanes.h"
#include "jade_normal_map.h"
#include "jade_runtime.h"
#include "jade_smooth.h"
#include "jade_texture.h"

#define JADE_DN_BLOCK 256

// (dn_pixel_xy and dn_pack, which the despeckle pass's pack kernels call as well: jade_runtime.h)

// ---------------------------------------------------------------------------------------------------------------- variance --

// v = sum (Y_l - m)^2 / (K (K - 1)) in fp64, stored as float; NaN where the tile's count cannot give it.  tile_n (nullable): each
// owned tile's count (after jade_render_adaptive); otherwise every tile has n.
__global__ __launch_bounds__(JADE_ERR_BLOCK) void k_pixel_variance(PathState P, const int32_t* tile_n, int64_t n_all, float* var_out) {
  __shared__ jade_err_v4f stage[JADE_ERR_STAGE_LANES * 192];
  const uint32_t t = blockIdx.x;
  const int i = threadIdx.x;
  const int64_t n = tile_n ? tile_n[t] : n_all;
  const bool estimable = lanes_estimable(n);
  const int K = (int)(n < JADE_SAMPLE_LANES ? n : JADE_SAMPLE_LANES);
  const double c = estimable ? (double)(n / K) : 1.0;
  float v = __builtin_nanf("");
  if (estimable) {
    const LaneMoments lm = lane_moments(P.sum, P.npx, t, i, K, c, stage);
    const double kk = (double)K;
    v = (float)(lane_sum_sq(lm.sd, lm.sdd, kk) / (kk * (kk - 1.0)));
  }
  var_out[(size_t)t * 256 + i] = v;
}

// -------------------------------------------------------------------------------------------------------------- guide pass --

// G: the throw-away PathState (one record and one slot per owned pixel: orgs, slot, hitp).  Sample sidx of every listed pixel.
// state[p] = {throughput, depth so far}, mirrors[p] = mirror vertices passed.  One text for the three cameras; the kernels below name them.
// (One text per family is safe here: the library is built with -ffp-contract=off, so the same statements in the same order give the same
// bits whatever the form they are compiled in, and tests/test_gpu_guide_tables_exact.py pins the guides' bits under every table.)
enum GuideCamera { GUIDE_PINHOLE, GUIDE_LENS, GUIDE_SHUTTER };
template <GuideCamera CAM>
static __device__ __forceinline__ void guide_camera_body(PathState G, const RenderConst& R, float lens_k, const ShutterConst& H, const int32_t* tile_ids,
                                                         const uint32_t* list, uint32_t n, uint32_t sidx, float4* state, uint32_t* mirrors) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = (int)list[i];
  int x, y;
  (void)dn_pixel_xy(R, tile_ids, p, &x, &y);  // (the list holds in-image pixels only)
  uint32_t rng;
  jvec3 dir;
  if constexpr (CAM == GUIDE_PINHOLE) {
    dir = camera_ray_dir(R, x, y, sidx, &rng);
    G.orgs[p] = make_float4(R.eye[0], R.eye[1], R.eye[2], __int_as_float(JADE_SKIP_CAMERA));  // (k_trace takes a camera ray's origin from P.eye)
  } else {
    // the sample's own origin, stored with "no source triangle" (-1) as jade_trace_rays' rays are, so k_trace reads it instead of P.eye
    jvec3 org;
    if constexpr (CAM == GUIDE_LENS) dir = camera_ray_lens(R, lens_k, x, y, sidx, &rng, &org);
    else dir = camera_ray_shutter(R, H, lens_k, x, y, sidx, &rng, &org);
    G.orgs[p] = make_float4(org.x, org.y, org.z, __int_as_float(-1));
  }
  G.slot[p] = make_float4(dir.x, dir.y, dir.z, __int_as_float(-1));  // -1: the nearest hit is wanted
  state[p] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
  mirrors[p] = 0u;
}
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_camera(PathState G, RenderConst R, const int32_t* tile_ids, const uint32_t* list, uint32_t n,
                                                                uint32_t sidx, float4* state, uint32_t* mirrors) {
  guide_camera_body<GUIDE_PINHOLE>(G, R, 0.0f, ShutterConst{}, tile_ids, list, n, sidx, state, mirrors);
}
// ... in a render under a thin lens (lens_k = PathState.lens_k of that render): the guides follow the lens (include/jade_bvh.h)
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_camera_lens(PathState G, RenderConst R, float lens_k, const int32_t* tile_ids, const uint32_t* list,
                                                                     uint32_t n, uint32_t sidx, float4* state, uint32_t* mirrors) {
  guide_camera_body<GUIDE_LENS>(G, R, lens_k, ShutterConst{}, tile_ids, list, n, sidx, state, mirrors);
}
// ... and in a render under a shutter (H = that render's constants), with a lens or without
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_camera_shutter(PathState G, RenderConst R, float lens_k, const int32_t* tile_ids, const uint32_t* list,
                                                                        uint32_t n, uint32_t sidx, float4* state, uint32_t* mirrors, ShutterConst H) {
  guide_camera_body<GUIDE_SHUTTER>(G, R, lens_k, H, tile_ids, list, n, sidx, state, mirrors);
}

// The hits of the rays queue[0 .. *count): a mirror vertex (reflex_mode == JADE_MIRROR, not emissive by bounce_mirror's test, fewer than
// JADE_MAX_FULL_REFLEX_TIME passed) goes on with bounce_mirror's reflected ray, appended to next_queue; anything else ends the sample
// and adds {a, z} to acc_az[p] and {n, 0} to acc_n[p].  last: this is the last guide sample, the sums are scaled by inv_g.
// One text for the four forms, by what the render's kernels take as their table (ST):
//   NoTables         the parity form: the flat normal, the material's brdf
//   const float4*    a smooth render (SM_SMOOTH; include/jade_bvh.h, "The shading normal, stated"): the shading normal of the hit - normal(triangle,
//                    hit point, -d) - in the mirror's reflection, formed again with the flat normal where it does not leave on the viewer's side of
//                    it, and in the normal guide
//   TexTables        a textured render (SM_TEX; "The surface colour, stated"): brdf_eff - the brdf times the surface colour at the hit - in the
//                    throughput and in the albedo guide as well, at every vertex of the mirror chain; the table carries the vertex normals the
//                    render began with, or the all-flat table
//   MapTables        a mapped render (SM_NMAP; "The mapped normal, stated"): the mapped normal in the shading normal's place
struct NoTables {};
template <class ST>
static __device__ __forceinline__ void guide_hits_body(const DevScene& S, PathState G, const uint32_t* queue, const uint32_t* count, float4* state,
                                                       uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g, uint32_t* next_queue,
                                                       uint32_t* next_count, const ST& table) {
  constexpr bool flat_only = std::is_same<ST, NoTables>::value;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *count) return;
  const int p = (int)queue[i];
  const float4 sl = G.slot[p];
  const jvec3 d = jv(sl.x, sl.y, sl.z);
  const int h = __float_as_int(sl.w);
  float4 st = state[p];
  jvec3 t = jv(st.x, st.y, st.z);
  float z = st.w;
  jvec3 a, n;
  if (h < 0) {
    a = t;
    n = jv(0.0f, 0.0f, 0.0f);
    z = 0.0f;
  } else {
    const float4 hp = G.hitp[p];
    const float4 tn = S.tnorm[h];
    const DevMaterial* m = S.mats + __float_as_uint(tn.w);
    const jvec3 flat = jv(tn.x, tn.y, tn.z);
    const jvec3 o = jv_neg(d);
    jvec3 norm = flat;
    if constexpr (!flat_only) norm = shading_normal(table, h, flat, jv(hp.x, hp.y, hp.z), o);
    const jvec3 brdf = textured(table, h, jv(hp.x, hp.y, hp.z), V3(m->brdf));
    const bool emissive = m->emissive[0] > 1.5e-4f || m->emissive[1] > 1.5e-4f || m->emissive[0] > 1.5e-4f;  // (bounce_mirror's test, as written)
    const uint32_t k = mirrors[p];
    if (m->reflex_mode == JADE_MIRROR && !emissive && k < (uint32_t)JADE_MAX_FULL_REFLEX_TIME) {
      t = jv_mul(t, brdf);
      z = z + hp.w;
      jvec3 refl = jv_sub(jv_scale(norm, 2 * jv_dot(o, norm)), o);  // bounce_mirror's statement
      if constexpr (!flat_only)
        if (!same_side(refl, o, flat)) refl = jv_sub(jv_scale(flat, 2 * jv_dot(o, flat)), o);
      G.orgs[p] = make_float4(hp.x, hp.y, hp.z, __int_as_float(h));
      G.slot[p] = make_float4(refl.x, refl.y, refl.z, __int_as_float(-1));
      state[p] = make_float4(t.x, t.y, t.z, z);
      mirrors[p] = k + 1u;
      next_queue[atomicAdd(next_count, 1u)] = (uint32_t)p;
      return;
    }
    z = z + hp.w;
    a = jv_mul(t, brdf);
    n = jv_dot(norm, d) > 0.0f ? jv_neg(norm) : norm;
  }
  float4 s0 = acc_az[p], s1 = acc_n[p];
  s0 = make_float4(s0.x + a.x, s0.y + a.y, s0.z + a.z, s0.w + z);
  s1 = make_float4(s1.x + n.x, s1.y + n.y, s1.z + n.z, 0.0f);
  if (last) {
    s0 = make_float4(s0.x * inv_g, s0.y * inv_g, s0.z * inv_g, s0.w * inv_g);
    s1 = make_float4(s1.x * inv_g, s1.y * inv_g, s1.z * inv_g, 0.0f);
  }
  acc_az[p] = s0;
  acc_n[p] = s1;
}
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_hits(DevScene S, PathState G, const uint32_t* queue, const uint32_t* count, float4* state,
                                                              uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g,
                                                              uint32_t* next_queue, uint32_t* next_count) {
  guide_hits_body(S, G, queue, count, state, mirrors, acc_az, acc_n, last, inv_g, next_queue, next_count, NoTables{});
}
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_hits_smooth(DevScene S, PathState G, const uint32_t* queue, const uint32_t* count, float4* state,
                                                                     uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g,
                                                                     uint32_t* next_queue, uint32_t* next_count, const float4* table) {
  guide_hits_body(S, G, queue, count, state, mirrors, acc_az, acc_n, last, inv_g, next_queue, next_count, table);
}
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_hits_textured(DevScene S, PathState G, const uint32_t* queue, const uint32_t* count, float4* state,
                                                                       uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g,
                                                                       uint32_t* next_queue, uint32_t* next_count, TexTables table) {
  guide_hits_body(S, G, queue, count, state, mirrors, acc_az, acc_n, last, inv_g, next_queue, next_count, table);
}
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_hits_mapped(DevScene S, PathState G, const uint32_t* queue, const uint32_t* count, float4* state,
                                                                     uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g,
                                                                     uint32_t* next_queue, uint32_t* next_count, MapTables table) {
  guide_hits_body(S, G, queue, count, state, mirrors, acc_az, acc_n, last, inv_g, next_queue, next_count, table);
}

// ------------------------------------------------------------------------------------------------------------------ filter --

// The render's owned tiles (compact layout: rgb as k_resolve writes it, variance, guide sums) -> image layout
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_dn_pack_tiles(RenderConst R, const int32_t* tile_ids, int npx, const float* rgb, const float* var,
                                                                 const float4* acc_az, const float4* acc_n, float4* A, float4* N, float4* L) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  int x, y;
  if (!dn_pixel_xy(R, tile_ids, p, &x, &y)) return;
  const float4 az = acc_az[p], n = acc_n[p];
  const float* c = rgb + 3 * (size_t)p;
  dn_pack(c[0], c[1], c[2], var[p], az.x, az.y, az.z, n.x, n.y, n.z, az.w, A, N, L, (size_t)y * R.width + x);
}

__global__ __launch_bounds__(JADE_DN_BLOCK) void k_dn_pack_image(int npix, const float* rgb, const float* var, const float* alb, const float* nrm,
                                                                 const float* dep, float4* A, float4* N, float4* L) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t q = 3 * (size_t)p;
  dn_pack(rgb[q], rgb[q + 1], rgb[q + 2], var[p], alb[q], alb[q + 1], alb[q + 2], nrm[q], nrm[q + 1], nrm[q + 2], dep[p], A, N, L, (size_t)p);
}

struct DnSigma {
  float l, n, z, a;
};

// One pass at step s over a 16x16 block of pixels (jade_bvh.h's formulas).  Taps are read straight from L2 (48 B each).
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_atrous(const float4* __restrict__ Ain, const float4* __restrict__ N, const float4* __restrict__ L,
                                                          float4* __restrict__ Aout, int W, int H, int s, DnSigma sg) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const size_t p = (size_t)y * W + x;
  const float4 ap = Ain[p], lp = L[p];
  if (lp.w != 0.0f) {  // unusable: colour and variance as they came in, every pass
    Aout[p] = ap;
    return;
  }
  // g_p: 3x3 (1/4, 1/2, 1/4)^2 blur of the variance over the in-image usable neighbours, renormalised
  float gs = 0.0f, gw = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= W) continue;
      if (L[(size_t)yy * W + xx].w != 0.0f) continue;
      const float w = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
      gs += w * Ain[(size_t)yy * W + xx].w;
      gw += w;
    }
  }
  const float g = gs / gw;
  const float4 np = N[p];
  const float lum_p = 0.3f * ap.x + 0.6f * ap.y + 0.1f * ap.z;
  const float den_l = sg.l * sqrtf(g) + 1e-10f;
  const bool pz = np.x == 0.0f && np.y == 0.0f && np.z == 0.0f;
  const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  float sw = 0.0f, sr = 0.0f, sgc = 0.0f, sb = 0.0f, sv = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = y + s * dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int xx = x + s * dx;
      if (xx < 0 || xx >= W) continue;
      const size_t q = (size_t)yy * W + xx;
      const float4 lq = L[q];
      if (lq.w != 0.0f) continue;  // an unusable pixel is no tap (skipped, not weighted by 0: 0 * inf is NaN)
      const float4 aq = Ain[q], nq = N[q];
      const bool qz = nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f;
      float wn;
      if (pz || qz) {
        wn = (pz && qz) ? 1.0f : 0.0f;
      } else {
        const float dn = np.x * nq.x + np.y * nq.y + np.z * nq.z;
        wn = powf(fmaxf(dn, 0.0f), sg.n);
      }
      const float lum_q = 0.3f * aq.x + 0.6f * aq.y + 0.1f * aq.z;
      const float wl = expf(-fabsf(lum_p - lum_q) / den_l);
      const float wz = expf(-fabsf(np.w - nq.w) / (sg.z * fmaxf(np.w, nq.w) + 1e-10f));
      const float wa = expf(-(fabsf(lp.x - lq.x) + fabsf(lp.y - lq.y) + fabsf(lp.z - lq.z)) / sg.a);
      const float w = h[dx + 2] * h[dy + 2] * wl * wn * wz * wa;
      sw += w;
      sr += w * aq.x;
      sgc += w * aq.y;
      sb += w * aq.z;
      sv += w * w * aq.w;
    }
  }
  Aout[p] = make_float4(sr / sw, sgc / sw, sb / sw, sv / (sw * sw));
}

// the filtered colour -> linear RGB (3 floats per pixel) and / or BGR8, image layout
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_dn_out(const float4* A, int npix, int tonemap, float limit, float* out_rgb, uint8_t* out_bgr) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const float4 a = A[p];
  if (out_rgb) {
    out_rgb[3 * (size_t)p] = a.x;
    out_rgb[3 * (size_t)p + 1] = a.y;
    out_rgb[3 * (size_t)p + 2] = a.z;
  }
  if (out_bgr) tone_pack_bgr8(jv(a.x, a.y, a.z), tonemap, limit, true, out_bgr + 3 * (size_t)p);
}

// ------------------------------------------------------------------------------------------------------------ host side --

static inline unsigned dn_grid(size_t n) { return (unsigned)((n + JADE_DN_BLOCK - 1) / JADE_DN_BLOCK); }

void jade_denoise_defaults(jade_denoise_params* p) {
  if (!p) return;
  // of SVGF's 5 passes and sigma_l = 4 and the sweep around them, 3 passes and sigma_l = 2 gave the lowest relMSE of the
  // denoised 64-spp frames of C2 and C3 (profiles/denoise_ab.json); sigma_n made no difference there and stays SVGF's 128
  p->iterations = 3;
  p->guide_spp = 4;
  p->sigma_luminance = 2.0f;
  p->sigma_normal = 128.0f;
  p->sigma_depth = 0.1f;
  p->sigma_albedo = 0.1f;
}

JADE_HIDDEN int dn_check_params(const jade_denoise_params* dp) {
  if (!dp) return jade_fail(JADE_ERR_INVALID, "null denoise parameters");
  if (dp->iterations < 0 || dp->iterations > 8) return jade_fail(JADE_ERR_INVALID, "iterations must be 0..8");
  if (dp->guide_spp < 1 || dp->guide_spp > 64) return jade_fail(JADE_ERR_INVALID, "guide_spp must be 1..64");
  if (!std::isfinite(dp->sigma_luminance) || !(dp->sigma_luminance > 0.0f)) return jade_fail(JADE_ERR_INVALID, "sigma_luminance must be finite and > 0");
  if (!std::isfinite(dp->sigma_normal) || !(dp->sigma_normal >= 0.0f)) return jade_fail(JADE_ERR_INVALID, "sigma_normal must be finite and >= 0");
  if (!std::isfinite(dp->sigma_depth) || !(dp->sigma_depth > 0.0f)) return jade_fail(JADE_ERR_INVALID, "sigma_depth must be finite and > 0");
  if (!std::isfinite(dp->sigma_albedo) || !(dp->sigma_albedo > 0.0f)) return jade_fail(JADE_ERR_INVALID, "sigma_albedo must be finite and > 0");
  return JADE_OK;
}

// grow-only: the denoiser's buffers are allocated on first use and kept (they do not come out of the records' budget, which
// jade_render_begin sizes before any of them exists)
static hipError_t dn_alloc(DevBuf& b, size_t bytes) { return (b.p && b.bytes >= bytes) ? hipSuccess : b.alloc(bytes); }

// Finish the paths the last step carried over, as resolve does; their work counters wait in dn_carried for the next step.
static int dn_flush(jade_scene* s) {
  jade_stats st{};
  if (int rc = jade_render_flush(s, &st)) return rc;
  s->dn_carried = st;  // (the flush took over what dn_carried held)
  return JADE_OK;
}

// each owned tile's sample count: its own after jade_render_adaptive, otherwise spp_done
JADE_HIDDEN std::vector<int32_t> dn_tile_counts(const jade_scene* s) {
  if (!s->tile_n.empty()) return s->tile_n;
  return std::vector<int32_t>(s->tile_ids.size(), (int32_t)std::min<int64_t>(s->spp_done, INT32_MAX));
}

// the variance of every owned pixel into b_dn_var (compact layout)
JADE_HIDDEN int dn_variance(jade_scene* s) {
  const size_t nt = s->tile_ids.size();
  HIP_TRY(dn_alloc(s->b_dn_var, (size_t)s->ps.npx * 4));
  DevBuf b_n;
  const int32_t* tile_n = nullptr;
  if (!s->tile_n.empty()) {
    HIP_TRY(upload(b_n, s->tile_n.data(), nt, s->stream));
    tile_n = b_n.as<int32_t>();
  }
  hipLaunchKernelGGL(k_pixel_variance, dim3((unsigned)nt), dim3(JADE_ERR_BLOCK), 0, s->stream, s->ps, tile_n, (int64_t)s->spp_done, s->b_dn_var.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));  // (b_n goes out of scope)
  return JADE_OK;
}

// The guide pass: G camera samples of every owned in-image pixel, one sample after the other, into b_dn_az = {albedo, depth} and
// b_dn_n = {normal, 0} (compact layout).  k_trace itself walks the rays (reference walk, nearest hit) on a throw-away PathState, with
// queue words and work counters of its own: neither the render's state nor its statistics see these rays.  The host waits once per
// k_trace launch, for the number of mirror continuations (a sample ends after at most JADE_MAX_FULL_REFLEX_TIME + 1 launches).
JADE_HIDDEN int dn_guides(jade_scene* s, int G) {
  const size_t n = (size_t)s->ps.npx;
  HIP_TRY(dn_alloc(s->b_dn_orgs, n * 16));
  HIP_TRY(dn_alloc(s->b_dn_slot, n * 16));
  HIP_TRY(dn_alloc(s->b_dn_hitp, n * 16));
  HIP_TRY(dn_alloc(s->b_dn_state, n * 16));
  HIP_TRY(dn_alloc(s->b_dn_mirrors, n * 4));
  HIP_TRY(dn_alloc(s->b_dn_list, n * 4));
  HIP_TRY(dn_alloc(s->b_dn_q[0], n * 4));
  HIP_TRY(dn_alloc(s->b_dn_q[1], n * 4));
  HIP_TRY(dn_alloc(s->b_dn_az, n * 16));
  HIP_TRY(dn_alloc(s->b_dn_n, n * 16));
  HIP_TRY(dn_alloc(s->b_dn_ctl, 2 * sizeof(QueueCtl)));
  HIP_TRY(dn_alloc(s->b_dn_ctr, sizeof(DevCounters) * JADE_CTR_SHARDS));
  if (!s->b_spill.p)
    HIP_TRY(s->b_spill.alloc((size_t)(JADE_BVH_STACK_CAPACITY - JADE_LDS_STACK) * s->trace_blocks * JADE_TRACE_BLOCK * 4));
  // the owned in-image pixels, in owned order: the first queue of every sample
  std::vector<uint32_t> list;
  list.reserve(n);
  for_each_owned_tile(s->tile_ids, s->rp.width, s->rp.height, [&](size_t t, int, int, int ww, int hh) {
    for (int l = 0; l < 256; ++l)
      if ((l & 15) < ww && (l >> 4) < hh) list.push_back((uint32_t)(t * 256 + (size_t)l));
  });
  const uint32_t n_in = (uint32_t)list.size();
  HIP_TRY(hipMemcpyAsync(s->b_dn_list.p, list.data(), (size_t)n_in * 4, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemsetAsync(s->b_dn_az.p, 0, n * 16, s->stream));
  HIP_TRY(hipMemsetAsync(s->b_dn_n.p, 0, n * 16, s->stream));
  PathState g{};
  g.npix = (int32_t)n;
  g.npx = (int32_t)n;
  g.rpp = 1;
  g.nslots = 1;
  g.orgs = s->b_dn_orgs.as<float4>();
  g.slot = s->b_dn_slot.as<float4>();
  g.hitp = s->b_dn_hitp.as<float4>();
  g.write_all_hits = 1u;  // every ray reports point and distance (as jade_trace_rays)
  g.early_exit = 0u;      // the reference walk: the nearest hit
  memcpy(g.eye, s->ps.eye, sizeof g.eye);
  QueueCtl* qc = s->b_dn_ctl.as<QueueCtl>();
  float4* state = s->b_dn_state.as<float4>();
  uint32_t* mirrors = s->b_dn_mirrors.as<uint32_t>();
  const float inv_g = (float)(1.0 / (double)G);
  for (int smp = 0; smp < G && n_in; ++smp) {
    if (shutter_on(s))
      hipLaunchKernelGGL(k_guide_camera_shutter, dim3(dn_grid(n_in)), dim3(JADE_DN_BLOCK), 0, s->stream, g, s->rc, s->ps.lens_k, s->b_tiles.as<int32_t>(),
                         s->b_dn_list.as<uint32_t>(), n_in, (uint32_t)smp, state, mirrors, s->sh);
    else if (lens_on(s))
      hipLaunchKernelGGL(k_guide_camera_lens, dim3(dn_grid(n_in)), dim3(JADE_DN_BLOCK), 0, s->stream, g, s->rc, s->ps.lens_k, s->b_tiles.as<int32_t>(),
                         s->b_dn_list.as<uint32_t>(), n_in, (uint32_t)smp, state, mirrors);
    else
      hipLaunchKernelGGL(k_guide_camera, dim3(dn_grid(n_in)), dim3(JADE_DN_BLOCK), 0, s->stream, g, s->rc, s->b_tiles.as<int32_t>(), s->b_dn_list.as<uint32_t>(),
                         n_in, (uint32_t)smp, state, mirrors);
    HIP_TRY(hipGetLastError());
    QueueCtl q0{};
    q0.count = n_in;
    HIP_TRY(hipMemcpyAsync(qc, &q0, sizeof q0, hipMemcpyHostToDevice, s->stream));
    const uint32_t* queue = s->b_dn_list.as<uint32_t>();
    uint32_t count = n_in;
    int cur = 0, qi = 0;
    for (;;) {
      launch_trace(s, g, queue, qc + cur, s->b_spill.as<uint32_t>(), s->b_dn_ctr.as<DevCounters>(), count);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemsetAsync(qc + (cur ^ 1), 0, sizeof(QueueCtl), s->stream));
      uint32_t* next_queue = s->b_dn_q[qi].as<uint32_t>();
      if (normal_maps_on(s))
        hipLaunchKernelGGL(k_guide_hits_mapped, dim3(dn_grid(count)), dim3(JADE_DN_BLOCK), 0, s->stream, s->dev, g, queue, &qc[cur].count, state, mirrors,
                           s->b_dn_az.as<float4>(), s->b_dn_n.as<float4>(), smp == G - 1 ? 1 : 0, inv_g, next_queue, &qc[cur ^ 1].count,
                           map_tables(s));
      else if (textures_on(s))
        hipLaunchKernelGGL(k_guide_hits_textured, dim3(dn_grid(count)), dim3(JADE_DN_BLOCK), 0, s->stream, s->dev, g, queue, &qc[cur].count, state, mirrors,
                           s->b_dn_az.as<float4>(), s->b_dn_n.as<float4>(), smp == G - 1 ? 1 : 0, inv_g, next_queue, &qc[cur ^ 1].count,
                           texture_tables(s));
      else if (smooth_on(s))
        hipLaunchKernelGGL(k_guide_hits_smooth, dim3(dn_grid(count)), dim3(JADE_DN_BLOCK), 0, s->stream, s->dev, g, queue, &qc[cur].count, state, mirrors,
                           s->b_dn_az.as<float4>(), s->b_dn_n.as<float4>(), smp == G - 1 ? 1 : 0, inv_g, next_queue, &qc[cur ^ 1].count, smooth_table(s));
      else
      hipLaunchKernelGGL(k_guide_hits, dim3(dn_grid(count)), dim3(JADE_DN_BLOCK), 0, s->stream, s->dev, g, queue, &qc[cur].count, state, mirrors,
                         s->b_dn_az.as<float4>(), s->b_dn_n.as<float4>(), smp == G - 1 ? 1 : 0, inv_g, next_queue, &qc[cur ^ 1].count);
      HIP_TRY(hipGetLastError());
      uint32_t next = 0;
      HIP_TRY(hipMemcpyAsync(&next, &qc[cur ^ 1].count, 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      if (next == 0) break;
      if (next > count) return jade_fail(JADE_ERR_DEVICE, "guide pass: the mirror queue grew");
      queue = next_queue;
      count = next;
      cur ^= 1;
      qi ^= 1;
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// compact tiles (npx entries of `stride` floats, the first `comps` of which are wanted; pixel t*256 + ly*16 + lx) -> the caller's image,
// other ranks' pixels untouched
static void dn_scatter(const jade_scene* s, const float* compact, int stride, int comps, float* out) {
  const int W = s->rp.width;
  for_each_owned_tile(s->tile_ids, W, s->rp.height, [&](size_t t, int x0, int y0, int ww, int hh) {
    for (int ly = 0; ly < hh; ++ly)
      for (int lx = 0; lx < ww; ++lx)
        for (int k = 0; k < comps; ++k)
          out[((size_t)(y0 + ly) * W + x0 + lx) * comps + k] = compact[(t * 256 + (size_t)ly * 16 + lx) * stride + k];
  });
}

int jade_render_guides(jade_scene* s, int32_t guide_spp, float* out_albedo, float* out_normal, float* out_depth, float* out_variance) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (guide_spp < 1 || guide_spp > 64) return jade_fail(JADE_ERR_INVALID, "guide_spp must be 1..64");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = dn_flush(s)) return rc;
  const size_t npx = (size_t)s->ps.npx;
  if (npx == 0) return JADE_OK;
  if (out_variance) {
    if (int rc = dn_variance(s)) return rc;
    std::vector<float> v(npx);
    HIP_TRY(hipMemcpyAsync(v.data(), s->b_dn_var.p, npx * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    dn_scatter(s, v.data(), 1, 1, out_variance);
  }
  if (out_albedo || out_normal || out_depth) {
    if (int rc = dn_guides(s, guide_spp)) return rc;
    std::vector<float> az(npx * 4), nn(npx * 4);
    HIP_TRY(hipMemcpyAsync(az.data(), s->b_dn_az.p, npx * 16, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(nn.data(), s->b_dn_n.p, npx * 16, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (out_albedo) dn_scatter(s, az.data(), 4, 3, out_albedo);
    if (out_normal) dn_scatter(s, nn.data(), 4, 3, out_normal);
    if (out_depth) dn_scatter(s, az.data() + 3, 4, 1, out_depth);
  }
  return JADE_OK;
}

// The filter on records already packed in b_dn_rec[0] (colour, variance), [2] (normal, depth), [3] (albedo): the passes, then one
// output kernel into b_dn_rgb / b_dn_bgr (image layout).
JADE_HIDDEN int dn_filter_out(hipStream_t stream, int W, int H, const jade_denoise_params* dp, int tonemap, float limit, float* dev_rgb,
                         uint8_t* dev_bgr, float4* const* rec) {
  int cur = 0;  // the passes, ping-pong between rec[0] and rec[1]
  const DnSigma sg{dp->sigma_luminance, dp->sigma_normal, dp->sigma_depth, dp->sigma_albedo};
  const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
  for (int i = 0; i < dp->iterations; ++i) {
    hipLaunchKernelGGL(k_atrous, grid, dim3(JADE_DN_BLOCK), 0, stream, rec[cur], rec[2], rec[3], rec[cur ^ 1], W, H, 1 << i, sg);
    HIP_TRY(hipGetLastError());
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_dn_out, dim3(dn_grid((size_t)W * H)), dim3(JADE_DN_BLOCK), 0, stream, rec[cur], W * H, tonemap, limit, dev_rgb, dev_bgr);
  HIP_TRY(hipGetLastError());
  return JADE_OK;
}

int jade_render_denoise(jade_scene* s, const jade_denoise_params* dp, int tonemap, float limit, float* out_rgb, uint8_t* out_bgr8) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (int rc = dn_check_params(dp)) return rc;
  if (tonemap != JADE_TONEMAP_ACES && tonemap != JADE_TONEMAP_REINHARD) return jade_fail(JADE_ERR_INVALID, "unknown tone operator");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  if (s->rp.tile_nranks > 1)
    return jade_fail(JADE_ERR_UNSUPPORTED, "jade_render_denoise needs the full frame: gather rgb and jade_render_guides, then jade_denoise_image");
  for (int32_t n : dn_tile_counts(s))
    if (!(n >= 2 && (n <= JADE_SAMPLE_LANES || n % JADE_SAMPLE_LANES == 0)))
      return jade_fail(JADE_ERR_INVALID, "a tile's sample count (" + std::to_string(n) + ") cannot give a variance: n >= 2, and a multiple of " +
                                        std::to_string(JADE_SAMPLE_LANES) + " above it");
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = dn_flush(s)) return rc;
  const int npx = s->ps.npx;
  if (npx == 0) return JADE_OK;
  const int W = s->rp.width, H = s->rp.height;
  const size_t npix = (size_t)W * (size_t)H;
  // the mean (k_resolve, compact tiles), the variance, the guides
  HIP_TRY(dn_alloc(s->b_out_rgb, (size_t)npx * 12));
  if (int rc = resolve_to(s, JADE_TONEMAP_ACES, 0.0f, s->b_out_rgb.as<float>(), nullptr, s->stream)) return rc;
  if (int rc = dn_variance(s)) return rc;
  if (int rc = dn_guides(s, dp->guide_spp)) return rc;
  // scattered once into the filter's records, image layout
  for (DevBuf& b : s->b_dn_rec) HIP_TRY(dn_alloc(b, npix * 16));
  float4* rec[4] = {s->b_dn_rec[0].as<float4>(), s->b_dn_rec[1].as<float4>(), s->b_dn_rec[2].as<float4>(), s->b_dn_rec[3].as<float4>()};
  hipLaunchKernelGGL(k_dn_pack_tiles, dim3(dn_grid((size_t)npx)), dim3(JADE_DN_BLOCK), 0, s->stream, s->rc, s->b_tiles.as<int32_t>(), npx, s->b_out_rgb.as<float>(),
                     s->b_dn_var.as<float>(), s->b_dn_az.as<float4>(), s->b_dn_n.as<float4>(), rec[0], rec[2], rec[3]);
  HIP_TRY(hipGetLastError());
  if (out_rgb) HIP_TRY(dn_alloc(s->b_dn_rgb, npix * 12));
  if (out_bgr8) HIP_TRY(dn_alloc(s->b_dn_bgr, npix * 3));
  if (int rc = dn_filter_out(s->stream, W, H, dp, tonemap, limit, out_rgb ? s->b_dn_rgb.as<float>() : nullptr,
                             out_bgr8 ? s->b_dn_bgr.as<uint8_t>() : nullptr, rec))
    return rc;
  if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, s->b_dn_rgb.p, npix * 12, hipMemcpyDeviceToHost, s->stream));
  if (out_bgr8) HIP_TRY(hipMemcpyAsync(out_bgr8, s->b_dn_bgr.p, npix * 3, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

int jade_denoise_image(int device_id, int32_t width, int32_t height, const float* rgb, const float* variance, const float* albedo, const float* normal,
                       const float* depth, const jade_denoise_params* dp, float* out_rgb) {
  if (!rgb || !variance || !albedo || !normal || !depth || !out_rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 3) return jade_fail(JADE_ERR_INVALID, "bad image size");
  if (int rc = dn_check_params(dp)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return jade_fail(JADE_ERR_DEVICE, "no HIP device");
  if (device_id < 0 || device_id >= ndev) return jade_fail(JADE_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  const size_t npix = (size_t)width * (size_t)height;
  hipStream_t stream = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } guard{stream};
  DevBuf b_rgb, b_var, b_alb, b_nrm, b_dep, b_rec[4], b_out;
  HIP_TRY(upload(b_rgb, rgb, npix * 3, stream));
  HIP_TRY(upload(b_var, variance, npix, stream));
  HIP_TRY(upload(b_alb, albedo, npix * 3, stream));
  HIP_TRY(upload(b_nrm, normal, npix * 3, stream));
  HIP_TRY(upload(b_dep, depth, npix, stream));
  for (DevBuf& b : b_rec) HIP_TRY(b.alloc(npix * 16));
  HIP_TRY(b_out.alloc(npix * 12));
  float4* rec[4] = {b_rec[0].as<float4>(), b_rec[1].as<float4>(), b_rec[2].as<float4>(), b_rec[3].as<float4>()};
  hipLaunchKernelGGL(k_dn_pack_image, dim3(dn_grid(npix)), dim3(JADE_DN_BLOCK), 0, stream, (int)npix, b_rgb.as<float>(), b_var.as<float>(), b_alb.as<float>(),
                     b_nrm.as<float>(), b_dep.as<float>(), rec[0], rec[2], rec[3]);
  HIP_TRY(hipGetLastError());
  if (int rc = dn_filter_out(stream, width, height, dp, JADE_TONEMAP_ACES, 0.0f, b_out.as<float>(), nullptr, rec)) return rc;
  HIP_TRY(hipMemcpyAsync(out_rgb, b_out.p, npix * 12, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return JADE_OK;
}
