// jade_denoise.hip — the denoiser's device side (include/jade_bvh.h: jade_render_guides, jade_render_denoise, jade_denoise_image).
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
// The host glue sits beside jade_render_step in jade_hip.hip: the guide pass launches k_trace, which lives there.
#include <hip/hip_runtime.h>

#include <math.h>

#include "jade_device.h"
#include "jade_lanes.h"

#define JADE_DN_BLOCK 256

// owned pixel p (tile t = p >> 8) -> image (x, y); false outside the image (edge tiles)
static __device__ __forceinline__ bool dn_pixel_xy(const RenderConst& R, const int32_t* tile_ids, int p, int* x, int* y) {
  const int tid = tile_ids[p >> 8], l = p & 255;
  *x = (tid % R.tiles_x) * JADE_TILE_SIZE + (l & 15);
  *y = (tid / R.tiles_x) * JADE_TILE_SIZE + (l >> 4);
  return *x < R.width && *y < R.height;
}

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
// state[p] = {throughput, depth so far}, mirrors[p] = mirror vertices passed.
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_camera(PathState G, RenderConst R, const int32_t* tile_ids, const uint32_t* list, uint32_t n,
                                                                uint32_t sidx, float4* state, uint32_t* mirrors) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = (int)list[i];
  int x, y;
  (void)dn_pixel_xy(R, tile_ids, p, &x, &y);  // (the list holds in-image pixels only)
  uint32_t rng;
  const jvec3 dir = camera_ray_dir(R, x, y, sidx, &rng);
  G.orgs[p] = make_float4(R.eye[0], R.eye[1], R.eye[2], __int_as_float(JADE_SKIP_CAMERA));  // (k_trace takes a camera ray's origin from P.eye)
  G.slot[p] = make_float4(dir.x, dir.y, dir.z, __int_as_float(-1));                          // -1: the nearest hit is wanted
  state[p] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
  mirrors[p] = 0u;
}

// The hits of the rays queue[0 .. *count): a mirror vertex (reflex_mode == JADE_MIRROR, not emissive by bounce_mirror's test, fewer than
// JADE_MAX_FULL_REFLEX_TIME passed) goes on with bounce_mirror's reflected ray, appended to next_queue; anything else ends the sample
// and adds {a, z} to acc_az[p] and {n, 0} to acc_n[p].  last: this is the last guide sample, the sums are scaled by inv_g.
__global__ __launch_bounds__(JADE_DN_BLOCK) void k_guide_hits(DevScene S, PathState G, const uint32_t* queue, const uint32_t* count, float4* state,
                                                              uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g,
                                                              uint32_t* next_queue, uint32_t* next_count) {
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
    const jvec3 norm = jv(tn.x, tn.y, tn.z);
    const jvec3 brdf = V3(m->brdf);
    const bool emissive = m->emissive[0] > 1.5e-4f || m->emissive[1] > 1.5e-4f || m->emissive[0] > 1.5e-4f;  // (bounce_mirror's test, as written)
    const uint32_t k = mirrors[p];
    if (m->reflex_mode == JADE_MIRROR && !emissive && k < (uint32_t)JADE_MAX_FULL_REFLEX_TIME) {
      t = jv_mul(t, brdf);
      z = z + hp.w;
      const jvec3 o = jv_neg(d);
      const jvec3 refl = jv_sub(jv_scale(norm, 2 * jv_dot(o, norm)), o);  // bounce_mirror's statement
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

// ------------------------------------------------------------------------------------------------------------------ filter --

// One pixel's filter record from its inputs; the two pack kernels call it, so the render's path and jade_denoise_image's are the
// same bits.  nhat = n / |n|, or 0 for the zero normal (a miss in every guide sample).
static __device__ __forceinline__ void dn_pack(float r, float g, float b, float v, float ax, float ay, float az, float nx, float ny, float nz,
                                               float z, float4* A, float4* N, float4* L, size_t o) {
  float hx = 0.0f, hy = 0.0f, hz = 0.0f;
  if (nx != 0.0f || ny != 0.0f || nz != 0.0f) {
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    hx = nx / len;
    hy = ny / len;
    hz = nz / len;
  }
  A[o] = make_float4(r, g, b, v);
  N[o] = make_float4(hx, hy, hz, z);
  L[o] = make_float4(ax, ay, az, 0.0f);
}

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
  // g_p: 3x3 (1/4, 1/2, 1/4)^2 blur of the variance over the in-image neighbours, renormalised
  float gs = 0.0f, gw = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= W) continue;
      const float w = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
      gs += w * Ain[(size_t)yy * W + xx].w;
      gw += w;
    }
  }
  const float g = gs / gw;
  const float4 ap = Ain[p], np = N[p], lp = L[p];
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
      const float4 aq = Ain[q], nq = N[q], lq = L[q];
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

// ------------------------------------------------------------------------------------------------------------- launches --
// For jade_hip.hip (hidden: libjade_hip.so exports only what the headers declare).

#define DN_HIDDEN __attribute__((visibility("hidden")))
static inline unsigned dn_grid(size_t n) { return (unsigned)((n + JADE_DN_BLOCK - 1) / JADE_DN_BLOCK); }

DN_HIDDEN hipError_t denoise_variance(hipStream_t stream, uint32_t n_tiles, const PathState& P, const int32_t* tile_n, int64_t n_all, float* var_out) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pixel_variance, dim3(n_tiles), dim3(JADE_ERR_BLOCK), 0, stream, P, tile_n, n_all, var_out);
  return hipGetLastError();
}

DN_HIDDEN hipError_t denoise_guide_camera(hipStream_t stream, const PathState& G, const RenderConst& R, const int32_t* tile_ids, const uint32_t* list,
                                          uint32_t n, uint32_t sidx, float4* state, uint32_t* mirrors) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_guide_camera, dim3(dn_grid(n)), dim3(JADE_DN_BLOCK), 0, stream, G, R, tile_ids, list, n, sidx, state, mirrors);
  return hipGetLastError();
}

DN_HIDDEN hipError_t denoise_guide_hits(hipStream_t stream, uint32_t n_max, const DevScene& S, const PathState& G, const uint32_t* queue, const uint32_t* count,
                                        float4* state, uint32_t* mirrors, float4* acc_az, float4* acc_n, int last, float inv_g, uint32_t* next_queue,
                                        uint32_t* next_count) {
  if (n_max == 0) return hipSuccess;
  hipLaunchKernelGGL(k_guide_hits, dim3(dn_grid(n_max)), dim3(JADE_DN_BLOCK), 0, stream, S, G, queue, count, state, mirrors, acc_az, acc_n, last, inv_g,
                     next_queue, next_count);
  return hipGetLastError();
}

DN_HIDDEN hipError_t denoise_pack_tiles(hipStream_t stream, const RenderConst& R, const int32_t* tile_ids, int npx, const float* rgb, const float* var,
                                        const float4* acc_az, const float4* acc_n, float4* A, float4* N, float4* L) {
  if (npx == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dn_pack_tiles, dim3(dn_grid((size_t)npx)), dim3(JADE_DN_BLOCK), 0, stream, R, tile_ids, npx, rgb, var, acc_az, acc_n, A, N, L);
  return hipGetLastError();
}

DN_HIDDEN hipError_t denoise_pack_image(hipStream_t stream, int npix, const float* rgb, const float* var, const float* alb, const float* nrm, const float* dep,
                                        float4* A, float4* N, float4* L) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dn_pack_image, dim3(dn_grid((size_t)npix)), dim3(JADE_DN_BLOCK), 0, stream, npix, rgb, var, alb, nrm, dep, A, N, L);
  return hipGetLastError();
}

// the passes, ping-pong between A[0] and A[1]; returns which of the two holds the result
DN_HIDDEN hipError_t denoise_filter(hipStream_t stream, int W, int H, int iterations, float sl, float sn, float sz, float sa, float4* A0, float4* A1,
                                    const float4* N, const float4* L, int* result) {
  float4* a[2] = {A0, A1};
  int cur = 0;
  const DnSigma sg{sl, sn, sz, sa};
  const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
  for (int i = 0; i < iterations; ++i) {
    hipLaunchKernelGGL(k_atrous, grid, dim3(JADE_DN_BLOCK), 0, stream, a[cur], N, L, a[cur ^ 1], W, H, 1 << i, sg);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cur ^= 1;
  }
  *result = cur;
  return hipSuccess;
}

DN_HIDDEN hipError_t denoise_out(hipStream_t stream, const float4* A, int npix, int tonemap, float limit, float* out_rgb, uint8_t* out_bgr) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dn_out, dim3(dn_grid((size_t)npix)), dim3(JADE_DN_BLOCK), 0, stream, A, npix, tonemap, limit, out_rgb, out_bgr);
  return hipGetLastError();
}
