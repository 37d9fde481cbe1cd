// jade_expose.hip — exposure (include/jade_bvh.h: jade_render_meter, jade_render_resolve_exposed, jade_expose_image, jade_meter_exposure):
// kernels and host side.
//
//   k_meter         the luminance histogram of a resolved frame: compact tiles as k_resolve leaves them (12 B per pixel, pixel_xy gives
//                   validity) or a plain image.  A bounded grid strides over the pixels; every block keeps its own histogram in LDS
//                   (512 bins, lanes add with LDS integer atomics) and writes it as one row; the three other classes and the extremes
//                   stay in registers until the block's end.  Integers only: the result does not depend on any order.
//   k_meter_sum     adds the rows (minimum / maximum for the two extreme words): one thread per word, no atomics
//   k_expose_pack   bytes = tone_pack_bgr8(e * m) (jade_device.h: k_resolve's statements), the same two layouts
//
// The host reads 2 KB back between the two halves: the policy (jade_meter_exposure) is double-precision host code, so that it is one
// function for a rank's meter and for the sum of several ranks' meters.
#include <math.h>

#include <cmath>
#include <cstring>

#include "jade_runtime.h"

#define JADE_EX_BLOCK 256
#define JADE_EX_MAX_BLOCKS 1024 /* k_meter's grid: four blocks per CU; a 1080p frame is 8 pixels per thread and 2 MB of rows */
// a row: the bins, then zero / negative / non-finite counts, then the bits of the largest and of the smallest positive luminance
#define JADE_EX_ZERO JADE_METER_BINS
#define JADE_EX_NEG (JADE_METER_BINS + 1)
#define JADE_EX_NONFINITE (JADE_METER_BINS + 2)
#define JADE_EX_MAX (JADE_METER_BINS + 3)
#define JADE_EX_MIN (JADE_METER_BINS + 4)
#define JADE_EX_WORDS (JADE_METER_BINS + 5)
// JADE_METER_AGGREGATE=1 (A/B builds): a wave whose lanes all fall into one bin adds their number once instead of lane by lane
#ifndef JADE_METER_AGGREGATE
#define JADE_METER_AGGREGATE 0
#endif

// Luminance, class and bin of one pixel - jade_bvh.h's statements, the one copy.  Returns the bin (>= 0) of a positive luminance, or
// the row word of its class negated - 1; *y_bits: the luminance's bits.
static __host__ __device__ __forceinline__ int meter_classify(float r, float g, float b, uint32_t* y_bits) {
  const float y = (float)(0.3 * (double)r + 0.6 * (double)g + 0.1 * (double)b);
  uint32_t u;
  __builtin_memcpy(&u, &y, 4);
  *y_bits = u;
  if ((u & 0x7f800000u) == 0x7f800000u) return -1 - JADE_EX_NONFINITE;
  if (y < 0.0f) return -1 - JADE_EX_NEG;
  if (y == 0.0f) return -1 - JADE_EX_ZERO;
  const int bin = (int)(u >> 20) - 760;
  return bin < 0 ? 0 : bin > JADE_METER_BINS - 1 ? JADE_METER_BINS - 1 : bin;
}

// owned pixel p (tile p >> 8) lies inside the image (pixel_xy's statement, jade_shade.h)
static __device__ __forceinline__ bool ex_in_image(const RenderConst& R, const int32_t* tile_ids, int p) {
  const int tid = tile_ids[p >> 8], l = p & 255;
  return (tid % R.tiles_x) * JADE_TILE_SIZE + (l & 15) < R.width && (tid / R.tiles_x) * JADE_TILE_SIZE + (l >> 4) < R.height;
}

// rgb: n pixels of 3 floats.  TILES: compact tiles, out-of-image pixels (written as 0 by k_resolve) are not counted.
// rows[blockIdx.x * JADE_EX_WORDS ..]: this block's histogram.
template <bool TILES>
__global__ __launch_bounds__(JADE_EX_BLOCK) void k_meter(const float* __restrict__ rgb, int n, RenderConst R, const int32_t* __restrict__ tile_ids,
                                                         uint32_t* __restrict__ rows) {
  __shared__ uint32_t h[JADE_EX_WORDS];
  for (int i = threadIdx.x; i < JADE_EX_WORDS; i += JADE_EX_BLOCK) h[i] = i == JADE_EX_MIN ? 0xffffffffu : 0u;
  __syncthreads();
  uint32_t n_zero = 0u, n_neg = 0u, n_nonf = 0u, ymax = 0u, ymin = 0xffffffffu;  // positive floats order as their bits
  const int stride = (int)gridDim.x * JADE_EX_BLOCK;
  for (int p = (int)blockIdx.x * JADE_EX_BLOCK + (int)threadIdx.x; p < n; p += stride) {
    if (TILES && !ex_in_image(R, tile_ids, p)) continue;
    const float* c = rgb + 3 * (size_t)p;
    uint32_t u;
    const int b = meter_classify(c[0], c[1], c[2], &u);
    if (b < 0) {
      const int w = -1 - b;
      n_zero += w == JADE_EX_ZERO;
      n_neg += w == JADE_EX_NEG;
      n_nonf += w == JADE_EX_NONFINITE;
      continue;
    }
    ymax = u > ymax ? u : ymax;
    ymin = u < ymin ? u : ymin;
#if JADE_METER_AGGREGATE
    const int first = __builtin_amdgcn_readfirstlane(b);
    const unsigned long long act = __ballot(1), same = __ballot(b == first);
    if (same == act) {
      if ((int)__lane_id() == __ffsll((long long)act) - 1) atomicAdd(&h[first], (uint32_t)__popcll(act));
    } else {
      atomicAdd(&h[b], 1u);
    }
#else
    atomicAdd(&h[b], 1u);
#endif
  }
  if (n_zero) atomicAdd(&h[JADE_EX_ZERO], n_zero);
  if (n_neg) atomicAdd(&h[JADE_EX_NEG], n_neg);
  if (n_nonf) atomicAdd(&h[JADE_EX_NONFINITE], n_nonf);
  if (ymax) {
    atomicMax(&h[JADE_EX_MAX], ymax);
    atomicMin(&h[JADE_EX_MIN], ymin);
  }
  __syncthreads();
  uint32_t* row = rows + (size_t)blockIdx.x * JADE_EX_WORDS;
  for (int i = threadIdx.x; i < JADE_EX_WORDS; i += JADE_EX_BLOCK) row[i] = h[i];
}

__global__ __launch_bounds__(64) void k_meter_sum(const uint32_t* __restrict__ rows, int n_rows, uint32_t* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= JADE_EX_WORDS) return;
  uint32_t v = rows[j];
  for (int r = 1; r < n_rows; ++r) {
    const uint32_t w = rows[(size_t)r * JADE_EX_WORDS + j];
    v = j == JADE_EX_MAX ? (w > v ? w : v) : j == JADE_EX_MIN ? (w < v ? w : v) : v + w;
  }
  out[j] = v;
}

template <bool TILES>
__global__ __launch_bounds__(JADE_EX_BLOCK) void k_expose_pack(const float* __restrict__ rgb, int n, RenderConst R, const int32_t* __restrict__ tile_ids,
                                                               float e, int tonemap, float limit, uint8_t* __restrict__ out_bgr) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const bool valid = TILES ? ex_in_image(R, tile_ids, p) : true;
  const float* c = rgb + 3 * (size_t)p;
  tone_pack_bgr8(jv(e * c[0], e * c[1], e * c[2]), tonemap, limit, valid, out_bgr + 3 * (size_t)p);
}

// ------------------------------------------------------------------------------------------------------------ host side --

void jade_display_defaults(jade_display_params* p) {
  if (!p) return;
  p->tonemap = JADE_TONEMAP_ACES;
  p->limit = 1.5f;  // (the preview's Reinhard limit, pass3.fsh; ACES does not read it)
  p->exposure_mode = JADE_EXPOSURE_MANUAL;
  p->exposure = 1.0f;
  p->key = 0.18f;
  p->p_lo = 0.05f;
  p->p_hi = 0.95f;
  p->min_exposure = 1.0f / 65536.0f;
  p->max_exposure = 65536.0f;
}

// the parameters of the mode in use; null = fine, otherwise what is wrong
static const char* ex_bad_params(const jade_display_params* p) {
  if (!p) return "null display parameters";
  if (p->exposure_mode == JADE_EXPOSURE_MANUAL) {
    if (!std::isfinite(p->exposure) || !(p->exposure > 0.0f)) return "exposure must be finite and > 0";
    return nullptr;
  }
  if (p->exposure_mode != JADE_EXPOSURE_AUTO) return "unknown exposure mode";
  if (!std::isfinite(p->key) || !(p->key > 0.0f)) return "key must be finite and > 0";
  if (!(p->p_lo >= 0.0f) || !(p->p_lo < p->p_hi) || !(p->p_hi <= 1.0f)) return "the exposure window needs 0 <= p_lo < p_hi <= 1";
  if (!std::isfinite(p->min_exposure) || !std::isfinite(p->max_exposure) || !(p->min_exposure > 0.0f) || !(p->min_exposure <= p->max_exposure))
    return "the exposure clamp needs 0 < min_exposure <= max_exposure, both finite";
  return nullptr;
}

float jade_meter_exposure(const jade_meter* m, const jade_display_params* p) {
  if (const char* bad = ex_bad_params(p)) {
    (void)jade_fail(JADE_ERR_INVALID, bad);
    return std::nanf("");
  }
  if (p->exposure_mode == JADE_EXPOSURE_MANUAL) return p->exposure;
  if (!m) {
    (void)jade_fail(JADE_ERR_INVALID, "null meter");
    return std::nanf("");
  }
  double total = 0.0;
  for (int b = 0; b < JADE_METER_BINS; ++b) total += (double)m->bins[b];
  const double lo = (double)p->p_lo * total, hi = (double)p->p_hi * total;
  double c = 0.0, sw = 0.0, swl = 0.0;
  for (int b = 0; b < JADE_METER_BINS; ++b) {
    const double c1 = c + (double)m->bins[b];
    const double w = std::max(0.0, std::min(c1, hi) - std::max(c, lo));
    const double l = (double)((b >> 3) - 32) + std::log2(1.0 + (double)(2 * (b & 7) + 1) / 16.0);
    swl += w * l;
    sw += w;
    c = c1;
  }
  float e = sw > 0.0 ? (float)((double)p->key * std::exp2(-(swl / sw))) : 1.0f;
  e = e < p->min_exposure ? p->min_exposure : e;
  e = e > p->max_exposure ? p->max_exposure : e;
  return e;
}

JADE_HIDDEN int ex_check(const jade_display_params* p) {
  if (const char* bad = ex_bad_params(p)) return jade_fail(JADE_ERR_INVALID, bad);
  if (p->tonemap != JADE_TONEMAP_ACES && p->tonemap != JADE_TONEMAP_REINHARD) return jade_fail(JADE_ERR_INVALID, "unknown tone operator");
  return JADE_OK;
}

// grow-only, as the denoiser's buffers
JADE_HIDDEN hipError_t ex_alloc(DevBuf& b, size_t bytes) { return (b.p && b.bytes >= bytes) ? hipSuccess : b.alloc(bytes); }

// Finish the paths the last step carried over, as resolve does; their work counters wait in dn_carried for the next step (the
// denoiser's hand-over, jade_denoise.hip).
static int ex_flush(jade_scene* s) {
  jade_stats st{};
  if (int rc = jade_render_flush(s, &st)) return rc;
  s->dn_carried = st;
  return JADE_OK;
}

// The meter of n pixels at dev_rgb (tile_ids: compact tiles of a render; null: a plain image) - two kernels, 2 KB back, one wait.
JADE_HIDDEN int ex_meter(DevBuf& b_rows, DevBuf& b_words, const float* dev_rgb, int n, const RenderConst& R, const int32_t* tile_ids, hipStream_t stream,
                         jade_meter* out) {
  memset(out, 0, sizeof *out);
  if (n <= 0) return JADE_OK;
  const int blocks = std::min((n + JADE_EX_BLOCK - 1) / JADE_EX_BLOCK, JADE_EX_MAX_BLOCKS);
  HIP_TRY(ex_alloc(b_rows, (size_t)blocks * JADE_EX_WORDS * 4));
  HIP_TRY(ex_alloc(b_words, (size_t)JADE_EX_WORDS * 4));
  if (tile_ids)
    hipLaunchKernelGGL(k_meter<true>, dim3((unsigned)blocks), dim3(JADE_EX_BLOCK), 0, stream, dev_rgb, n, R, tile_ids, b_rows.as<uint32_t>());
  else
    hipLaunchKernelGGL(k_meter<false>, dim3((unsigned)blocks), dim3(JADE_EX_BLOCK), 0, stream, dev_rgb, n, R, tile_ids, b_rows.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_meter_sum, dim3((JADE_EX_WORDS + 63) / 64), dim3(64), 0, stream, b_rows.as<uint32_t>(), blocks, b_words.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  uint32_t w[JADE_EX_WORDS];
  HIP_TRY(hipMemcpyAsync(w, b_words.p, sizeof w, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int b = 0; b < JADE_METER_BINS; ++b) {
    out->bins[b] = w[b];
    out->n_positive += w[b];
  }
  out->n_zero = w[JADE_EX_ZERO];
  out->n_negative = w[JADE_EX_NEG];
  out->n_nonfinite = w[JADE_EX_NONFINITE];
  if (out->n_positive) {
    memcpy(&out->lum_max, &w[JADE_EX_MAX], 4);
    memcpy(&out->lum_min, &w[JADE_EX_MIN], 4);
  }
  return JADE_OK;
}

JADE_HIDDEN void ex_launch_pack(const float* dev_rgb, int n, const RenderConst& R, const int32_t* tile_ids, float e, const jade_display_params* p,
                                uint8_t* dev_bgr, hipStream_t stream) {
  const dim3 grid((unsigned)((n + JADE_EX_BLOCK - 1) / JADE_EX_BLOCK));
  if (tile_ids)
    hipLaunchKernelGGL(k_expose_pack<true>, grid, dim3(JADE_EX_BLOCK), 0, stream, dev_rgb, n, R, tile_ids, e, (int)p->tonemap, p->limit, dev_bgr);
  else
    hipLaunchKernelGGL(k_expose_pack<false>, grid, dim3(JADE_EX_BLOCK), 0, stream, dev_rgb, n, R, tile_ids, e, (int)p->tonemap, p->limit, dev_bgr);
}

// flush + k_resolve into b_out_rgb (compact tiles), what both render entry points start with
JADE_HIDDEN int ex_resolve(jade_scene* s) {
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = ex_flush(s)) return rc;
  if (s->ps.npx == 0) return JADE_OK;
  HIP_TRY(ex_alloc(s->b_out_rgb, (size_t)s->ps.npx * 12));
  return resolve_to(s, JADE_TONEMAP_ACES, 0.0f, s->b_out_rgb.as<float>(), nullptr, s->stream);
}

int jade_render_meter(jade_scene* s, jade_meter* out) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (!out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  if (int rc = ex_resolve(s)) return rc;
  return ex_meter(s->b_ex_rows, s->b_ex_meter, s->b_out_rgb.as<float>(), s->ps.npx, s->rc, s->b_tiles.as<int32_t>(), s->stream, out);
}

int jade_render_resolve_exposed(jade_scene* s, const jade_display_params* dp, float* out_rgb, uint8_t* out_bgr8, float* exposure_used,
                                jade_meter* meter_out) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (int rc = ex_check(dp)) return rc;
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  if (int rc = ex_resolve(s)) return rc;
  const int npix = s->ps.npx;
  jade_meter m;
  memset(&m, 0, sizeof m);
  if (dp->exposure_mode == JADE_EXPOSURE_AUTO || meter_out)
    if (int rc = ex_meter(s->b_ex_rows, s->b_ex_meter, s->b_out_rgb.as<float>(), npix, s->rc, s->b_tiles.as<int32_t>(), s->stream, &m)) return rc;
  const float e = jade_meter_exposure(&m, dp);
  if (exposure_used) *exposure_used = e;
  if (meter_out) *meter_out = m;
  if (npix == 0) return JADE_OK;
  std::vector<float> hrgb;
  std::vector<uint8_t> hbgr;
  if (out_bgr8) {
    HIP_TRY(ex_alloc(s->b_out_bgr, (size_t)npix * 3));
    ex_launch_pack(s->b_out_rgb.as<float>(), npix, s->rc, s->b_tiles.as<int32_t>(), e, dp, s->b_out_bgr.as<uint8_t>(), s->stream);
    HIP_TRY(hipGetLastError());
    hbgr.resize((size_t)npix * 3);
    HIP_TRY(hipMemcpyAsync(hbgr.data(), s->b_out_bgr.p, hbgr.size(), hipMemcpyDeviceToHost, s->stream));
  }
  if (out_rgb) {
    hrgb.resize((size_t)npix * 3);
    HIP_TRY(hipMemcpyAsync(hrgb.data(), s->b_out_rgb.p, hrgb.size() * 4, hipMemcpyDeviceToHost, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  // scatter the compact tiles into the caller's frame as jade_render_resolve_ex does; other ranks' pixels untouched
  const int W = s->rp.width;
  for_each_owned_tile(s->tile_ids, W, s->rp.height, [&](size_t t, int x0, int y0, int ww, int hh) {
    for (int ly = 0; ly < hh; ++ly) {
      const size_t src = (t * 256 + (size_t)ly * 16) * 3, dst = ((size_t)(y0 + ly) * W + x0) * 3;
      if (out_rgb) memcpy(out_rgb + dst, hrgb.data() + src, (size_t)ww * 12);
      if (out_bgr8) memcpy(out_bgr8 + dst, hbgr.data() + src, (size_t)ww * 3);
    }
  });
  return JADE_OK;
}

int jade_expose_image(int device_id, int32_t width, int32_t height, const float* rgb, const jade_display_params* dp, uint8_t* out_bgr8,
                      float* exposure_used, jade_meter* meter_out) {
  if (!rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 3) return jade_fail(JADE_ERR_INVALID, "bad image size");
  if (int rc = ex_check(dp)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return jade_fail(JADE_ERR_DEVICE, "no HIP device");
  if (device_id < 0 || device_id >= ndev) return jade_fail(JADE_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  const int npix = width * height;
  hipStream_t stream = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } guard{stream};
  DevBuf b_rgb, b_rows, b_words, b_bgr;
  HIP_TRY(upload(b_rgb, rgb, (size_t)npix * 3, stream));
  const RenderConst none{};
  jade_meter m;
  memset(&m, 0, sizeof m);
  if (dp->exposure_mode == JADE_EXPOSURE_AUTO || meter_out)
    if (int rc = ex_meter(b_rows, b_words, b_rgb.as<float>(), npix, none, nullptr, stream, &m)) return rc;
  const float e = jade_meter_exposure(&m, dp);
  if (exposure_used) *exposure_used = e;
  if (meter_out) *meter_out = m;
  if (out_bgr8) {
    HIP_TRY(b_bgr.alloc((size_t)npix * 3));
    ex_launch_pack(b_rgb.as<float>(), npix, none, nullptr, e, dp, b_bgr.as<uint8_t>(), stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_bgr8, b_bgr.p, (size_t)npix * 3, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return JADE_OK;
}
