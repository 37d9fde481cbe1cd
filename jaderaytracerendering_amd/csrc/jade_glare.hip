// jade_glare.hip — glare (include/jade_bvh.h: jade_glare_defaults, jade_glare_image, jade_render_glare): kernels and host side.
//
//   k_gl_scatter    the render's compact tiles (k_resolve's 12 B per pixel) -> the frame in image layout
//   k_gl_pack       the frame (12 B per pixel) -> L_0, one float4 per pixel; a non-finite pixel enters as 0
//   k_gl_reduce     L_k -> L_{k+1}: the 5x5 separable filter at stride 2.  One block of 256 threads makes 32 x 8 outputs from a
//                   67 x 19 source tile staged in LDS, filters its rows into a second LDS array and then the columns from there
//   k_gl_expand_add A_k = w_k L_k + EXPAND(A_{k+1}) in place of L_k (every thread reads and writes its own pixel of L_k); at most 9
//                   taps of the four times smaller coarser level, straight from L2.  Without a coarser level: A_k = w_k L_k
//   k_gl_out        out = (1 - s) c + s EXPAND(A_1), a non-finite pixel of c passed through as its bits; writes 12 B per pixel
//
// No atomics: every output word has one writer and a fixed order of additions, so the result does not depend on the launch order.
//
// k_gl_reduce's LDS, 30.7 KB per block (five blocks per CU):
//   S[19][69] float4  the source tile, rows 2 oy0 - 2 .. + 18 and columns 2 ox0 - 2 .. + 66, both clamped to the level.  In a row the
//                     even columns c = 2j lie at [j] (34 of them) and the odd ones c = 2j + 1 at [36 + j] (33): the row filter's taps
//                     of output ox are [ox], [36 + ox], [ox + 1], [36 + ox + 1], [ox + 2] - unit stride over the lanes.
//   T[19][32] float4  the rows filtered: T[r][ox].
// Reads (ds_read_b128, banks (a/4) mod 64, four groups of 16 lanes: 0-3 12-15 20-27 | 4-11 16-19 28-31 | ...): a wave's lanes are 32
// consecutive ox of two rows (row filter: 608 items dealt in order; column filter: thread = oy * 32 + ox), so each group of 16 lanes
// lies in one row and covers sixteen 16-B slots that are distinct mod 16 - one 256-B bank row, no conflict, whatever the row stride.
// That is what the 32-wide tile is for: with 16 outputs per row a group spans two rows and needs a row stride of 0 mod 16 slots.
// Writes (ds_write_b128, banks (a/4) mod 32, groups of 8 consecutive lanes): the staging loop takes the tile's elements in order, so
// 8 lanes hold 4 even and 4 odd columns; the odd half starts 36 slots (4 mod 8) behind the even one, so the two runs of 4 slots fall
// into different halves of the 128-B bank row when the group starts at an even column and share one slot when it starts at an odd
// one: at most 2-way, on one slot (the tile's row of 67 makes the two cases alternate).  A block stores 1273 and reads 4320 float4.
// The emitted code has these instructions and no narrower one (ten ds_read_b128, two ds_write_b128 in k_gl_reduce): gl_h5 says why.
// A source pixel is fetched 67 * 19 / (4 * 32 * 8) = 1.24 times per level (25 / 4 = 6.25 without the staging).
#include <math.h>

#include <cmath>
#include <cstring>

#include "jade_runtime.h"

#define JADE_GL_BLOCK 256
#define JADE_GL_MAX_LEVELS 12
#define JADE_GL_TW 32                      /* outputs of a k_gl_reduce block: 32 x 8 */
#define JADE_GL_TH 8
#define JADE_GL_SW (2 * JADE_GL_TW + 3)    /* its source tile: 67 x 19 */
#define JADE_GL_SH (2 * JADE_GL_TH + 3)
#define JADE_GL_ODD 36                     /* slot of the first odd column in a row of S */
#define JADE_GL_STRIDE (JADE_GL_ODD + JADE_GL_TW + 1)
#define JADE_GL_MAX_HEIGHT (16 * 65535)    /* rows go into grid.y (at most 65535 blocks): 16 per block in k_gl_out, 2 x 8 source rows in k_gl_reduce */

static __device__ __forceinline__ bool gl_finite(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

// h(0) a + h(1) b + h(2) c + h(3) d + h(4) e, added in this order (jade_bvh.h: REDUCE).  The fourth word (0, and 0 it stays) is
// filtered like the colour: left out, the compiler narrows k_gl_reduce's LDS reads to ds_read_b96, which are served in eight lane
// groups over 32 banks at 8 LDS cycles each instead of ds_read_b128's four groups at 4.
static __device__ __forceinline__ float4 gl_h5(float4 a, float4 b, float4 c, float4 d, float4 e) {
  const float h0 = 1.0f / 16.0f, h1 = 4.0f / 16.0f, h2 = 6.0f / 16.0f;
  float4 r;
  r.x = h0 * a.x;
  r.y = h0 * a.y;
  r.z = h0 * a.z;
  r.w = h0 * a.w;
  r.x = r.x + h1 * b.x;
  r.y = r.y + h1 * b.y;
  r.z = r.z + h1 * b.z;
  r.w = r.w + h1 * b.w;
  r.x = r.x + h2 * c.x;
  r.y = r.y + h2 * c.y;
  r.z = r.z + h2 * c.z;
  r.w = r.w + h2 * c.w;
  r.x = r.x + h1 * d.x;
  r.y = r.y + h1 * d.y;
  r.z = r.z + h1 * d.z;
  r.w = r.w + h1 * d.w;
  r.x = r.x + h0 * e.x;
  r.y = r.y + h0 * e.y;
  r.z = r.z + h0 * e.z;
  r.w = r.w + h0 * e.w;
  return r;
}

// One axis of EXPAND at fine index 2j (even) or 2j + 1 (odd) from a(j-1), a(j), a(j+1) = a, b, c (jade_bvh.h: EXPAND)
static __device__ __forceinline__ float4 gl_e3(float4 a, float4 b, float4 c, bool even) {
  float4 r;
  r.x = even ? (0.125f * a.x + 0.75f * b.x) + 0.125f * c.x : 0.5f * b.x + 0.5f * c.x;
  r.y = even ? (0.125f * a.y + 0.75f * b.y) + 0.125f * c.y : 0.5f * b.y + 0.5f * c.y;
  r.z = even ? (0.125f * a.z + 0.75f * b.z) + 0.125f * c.z : 0.5f * b.z + 0.5f * c.z;
  r.w = 0.0f;
  return r;
}

// EXPAND(A)(x, y), A the coarser level of mw x mh pixels: rows (y) first, then columns (x)
static __device__ __forceinline__ float4 gl_expand(const float4* __restrict__ A, int mw, int mh, int x, int y) {
  const int jx = x >> 1, jy = y >> 1;
  const bool ex = !(x & 1), ey = !(y & 1);
  const int y0 = max(jy - 1, 0), y1 = min(jy, mh - 1), y2 = min(jy + 1, mh - 1);
  const int x0 = max(jx - 1, 0), x1 = min(jx, mw - 1), x2 = min(jx + 1, mw - 1);
  const float4* r0 = A + (size_t)y0 * mw;
  const float4* r1 = A + (size_t)y1 * mw;
  const float4* r2 = A + (size_t)y2 * mw;
  const float4 t0 = gl_e3(r0[x0], r1[x0], r2[x0], ey);
  const float4 t1 = gl_e3(r0[x1], r1[x1], r2[x1], ey);
  const float4 t2 = gl_e3(r0[x2], r1[x2], r2[x2], ey);
  return gl_e3(t0, t1, t2, ex);
}

// owned pixel p (tile p >> 8) of a full-frame render -> its place in the image; pixels of edge tiles outside the image are skipped
__global__ __launch_bounds__(JADE_GL_BLOCK) void k_gl_scatter(RenderConst R, const int32_t* __restrict__ tile_ids, int npx, const uint32_t* __restrict__ tiles,
                                                              uint32_t* __restrict__ image) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  const int tid = tile_ids[p >> 8], l = p & 255;
  const int x = (tid % R.tiles_x) * JADE_TILE_SIZE + (l & 15), y = (tid / R.tiles_x) * JADE_TILE_SIZE + (l >> 4);
  if (x >= R.width || y >= R.height) return;
  const uint32_t* c = tiles + 3 * (size_t)p;
  uint32_t* o = image + 3 * ((size_t)y * R.width + x);
  o[0] = c[0];
  o[1] = c[1];
  o[2] = c[2];
}

__global__ __launch_bounds__(JADE_GL_BLOCK) void k_gl_pack(const uint32_t* __restrict__ rgb, int npix, float4* __restrict__ L0) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const uint32_t* c = rgb + 3 * (size_t)p;
  const uint32_t r = c[0], g = c[1], b = c[2];
  const bool ok = gl_finite(r) && gl_finite(g) && gl_finite(b);
  L0[p] = ok ? make_float4(__uint_as_float(r), __uint_as_float(g), __uint_as_float(b), 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// src: sw x sh pixels; dst: dw x dh = ceil(sw / 2) x ceil(sh / 2).  Every source index is clamped to the level, so no read leaves it.
__global__ __launch_bounds__(JADE_GL_BLOCK) void k_gl_reduce(const float4* __restrict__ src, int sw, int sh, float4* __restrict__ dst, int dw, int dh) {
  __shared__ float4 S[JADE_GL_SH][JADE_GL_STRIDE];
  __shared__ float4 T[JADE_GL_SH][JADE_GL_TW];
  const int t = threadIdx.x;
  const int bx = 2 * (int)blockIdx.x * JADE_GL_TW - 2, by = 2 * (int)blockIdx.y * JADE_GL_TH - 2;
  for (int i = t; i < JADE_GL_SW * JADE_GL_SH; i += JADE_GL_BLOCK) {
    const int r = i / JADE_GL_SW, c = i - r * JADE_GL_SW;
    const int x = min(max(bx + c, 0), sw - 1), y = min(max(by + r, 0), sh - 1);
    S[r][(c & 1) * JADE_GL_ODD + (c >> 1)] = src[(size_t)y * sw + x];
  }
  __syncthreads();
  for (int i = t; i < JADE_GL_TW * JADE_GL_SH; i += JADE_GL_BLOCK) {
    const int r = i / JADE_GL_TW, ox = i - r * JADE_GL_TW;
    const float4* e = &S[r][ox];
    const float4* o = &S[r][JADE_GL_ODD + ox];
    T[r][ox] = gl_h5(e[0], o[0], e[1], o[1], e[2]);
  }
  __syncthreads();
  const int lx = t & (JADE_GL_TW - 1), ly = t / JADE_GL_TW;
  const int ox = (int)blockIdx.x * JADE_GL_TW + lx, oy = (int)blockIdx.y * JADE_GL_TH + ly;
  if (ox >= dw || oy >= dh) return;
  dst[(size_t)oy * dw + ox] = gl_h5(T[2 * ly][lx], T[2 * ly + 1][lx], T[2 * ly + 2][lx], T[2 * ly + 3][lx], T[2 * ly + 4][lx]);
}

// L: w x h pixels, becomes A in place.  A_up: the coarser level's A (mw x mh), null at the top of the pyramid.
__global__ __launch_bounds__(JADE_GL_BLOCK) void k_gl_expand_add(float4* __restrict__ L, int w, int h, float wk, const float4* __restrict__ A_up, int mw, int mh) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * w + x;
  const float4 l = L[p];
  float4 a = make_float4(wk * l.x, wk * l.y, wk * l.z, 0.0f);
  if (A_up) {
    const float4 e = gl_expand(A_up, mw, mh, x, y);
    a.x = a.x + e.x;
    a.y = a.y + e.y;
    a.z = a.z + e.z;
  }
  L[p] = a;
}

// out may be rgb: a thread reads and writes its own pixel only
__global__ __launch_bounds__(JADE_GL_BLOCK) void k_gl_out(const uint32_t* rgb, int w, int h, const float4* __restrict__ A1, int mw, int mh, float s,
                                                          float one_minus_s, uint32_t* out) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= w || y >= h) return;
  const size_t q = 3 * ((size_t)y * w + x);
  uint32_t r = rgb[q], g = rgb[q + 1], b = rgb[q + 2];
  if (gl_finite(r) && gl_finite(g) && gl_finite(b)) {
    const float4 e = gl_expand(A1, mw, mh, x, y);
    r = __float_as_uint(one_minus_s * __uint_as_float(r) + s * e.x);
    g = __float_as_uint(one_minus_s * __uint_as_float(g) + s * e.y);
    b = __float_as_uint(one_minus_s * __uint_as_float(b) + s * e.z);
  }
  out[q] = r;
  out[q + 1] = g;
  out[q + 2] = b;
}

// ------------------------------------------------------------------------------------------------------------ host side --

void jade_glare_defaults(jade_glare_params* p) {
  if (!p) return;
  // a look, not a measurement: 1/2 per octave is an r^-3 halo, and a tenth of the light scattered is a guess
  p->levels = 6;
  p->strength = 0.1f;
  p->falloff = 0.5f;
}

static int gl_check(const jade_glare_params* gp) {
  if (!gp) return jade_fail(JADE_ERR_INVALID, "null glare parameters");
  if (gp->levels < 1 || gp->levels > JADE_GL_MAX_LEVELS) return jade_fail(JADE_ERR_INVALID, "levels must be 1..12");
  if (!std::isfinite(gp->strength) || !(gp->strength >= 0.0f) || !(gp->strength <= 1.0f)) return jade_fail(JADE_ERR_INVALID, "strength must be in [0, 1]");
  if (!std::isfinite(gp->falloff) || !(gp->falloff > 0.0f)) return jade_fail(JADE_ERR_INVALID, "falloff must be finite and > 0");
  return JADE_OK;
}

// The pyramid and the output kernel on a frame in image layout at dev_rgb (W x H, 12 B per pixel); dev_out may be dev_rgb.  pyr holds
// every level, grown on first use.  strength > 0.
static int gl_run(hipStream_t stream, DevBuf& pyr, int W, int H, const jade_glare_params* gp, const float* dev_rgb, float* dev_out) {
  const int n = gp->levels;
  int lw[JADE_GL_MAX_LEVELS + 1], lh[JADE_GL_MAX_LEVELS + 1];
  size_t off[JADE_GL_MAX_LEVELS + 2];
  lw[0] = W, lh[0] = H, off[0] = 0;
  for (int k = 0; k < n; ++k) {
    lw[k + 1] = (lw[k] + 1) / 2;
    lh[k + 1] = (lh[k] + 1) / 2;
    off[k + 1] = off[k] + (size_t)lw[k] * lh[k];
  }
  off[n + 1] = off[n] + (size_t)lw[n] * lh[n];
  double wsum = 0.0, wd[JADE_GL_MAX_LEVELS + 1];
  // f^(k-1) over their sum; for f > 1 every power is taken relative to the largest, f^(n-1), so that none overflows
  const int k0 = gp->falloff > 1.0f ? n : 1;
  for (int k = 1; k <= n; ++k) wsum += wd[k] = std::pow((double)gp->falloff, (double)(k - k0));
  HIP_TRY(ex_alloc(pyr, off[n + 1] * sizeof(float4)));
  float4* L = pyr.as<float4>();
  const int npix = W * H;
  hipLaunchKernelGGL(k_gl_pack, dim3((unsigned)((npix + JADE_GL_BLOCK - 1) / JADE_GL_BLOCK)), dim3(JADE_GL_BLOCK), 0, stream,
                     reinterpret_cast<const uint32_t*>(dev_rgb), npix, L);
  HIP_TRY(hipGetLastError());
  for (int k = 0; k < n; ++k) {
    const dim3 grid((unsigned)((lw[k + 1] + JADE_GL_TW - 1) / JADE_GL_TW), (unsigned)((lh[k + 1] + JADE_GL_TH - 1) / JADE_GL_TH));
    hipLaunchKernelGGL(k_gl_reduce, grid, dim3(JADE_GL_BLOCK), 0, stream, L + off[k], lw[k], lh[k], L + off[k + 1], lw[k + 1], lh[k + 1]);
    HIP_TRY(hipGetLastError());
  }
  for (int k = n; k >= 1; --k) {
    const dim3 grid((unsigned)((lw[k] + 15) / 16), (unsigned)((lh[k] + 15) / 16));
    const float4* up = k < n ? L + off[k + 1] : nullptr;
    hipLaunchKernelGGL(k_gl_expand_add, grid, dim3(JADE_GL_BLOCK), 0, stream, L + off[k], lw[k], lh[k], (float)(wd[k] / wsum), up, k < n ? lw[k + 1] : 0,
                       k < n ? lh[k + 1] : 0);
    HIP_TRY(hipGetLastError());
  }
  const float s = gp->strength;
  hipLaunchKernelGGL(k_gl_out, dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)), dim3(JADE_GL_BLOCK), 0, stream,
                     reinterpret_cast<const uint32_t*>(dev_rgb), W, H, L + off[1], lw[1], lh[1], s, 1.0f - s, reinterpret_cast<uint32_t*>(dev_out));
  HIP_TRY(hipGetLastError());
  return JADE_OK;
}

int jade_glare_image(int device_id, int32_t width, int32_t height, const float* rgb, const jade_glare_params* gp, float* out_rgb) {
  if (!rgb || !out_rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 3 || height > JADE_GL_MAX_HEIGHT)
    return jade_fail(JADE_ERR_INVALID, "bad image size");
  if (int rc = gl_check(gp)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return jade_fail(JADE_ERR_DEVICE, "no HIP device");
  if (device_id < 0 || device_id >= ndev) return jade_fail(JADE_ERR_INVALID, "device_id out of range");
  const size_t npix = (size_t)width * (size_t)height;
  if (gp->strength == 0.0f) {  // the identity, bit for bit: no pyramid
    if (out_rgb != rgb) memmove(out_rgb, rgb, npix * 12);
    return JADE_OK;
  }
  HIP_TRY(hipSetDevice(device_id));
  hipStream_t stream = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } guard{stream};
  DevBuf b_rgb, b_pyr;
  HIP_TRY(upload(b_rgb, rgb, npix * 3, stream));
  if (int rc = gl_run(stream, b_pyr, width, height, gp, b_rgb.as<float>(), b_rgb.as<float>())) return rc;
  HIP_TRY(hipMemcpyAsync(out_rgb, b_rgb.p, npix * 12, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return JADE_OK;
}

int jade_render_glare(jade_scene* s, const jade_glare_params* gp, const jade_display_params* display, float* out_rgb, uint8_t* out_bgr8,
                      float* exposure_used) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (int rc = gl_check(gp)) return rc;
  jade_display_params dflt;
  jade_display_defaults(&dflt);
  const jade_display_params* dp = display ? display : &dflt;
  if (int rc = ex_check(dp)) return rc;
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  if (s->rp.tile_nranks > 1)
    return jade_fail(JADE_ERR_UNSUPPORTED, "jade_render_glare needs the full frame: gather rgb (jade_render_resolve_ex), then jade_glare_image");
  if (s->rp.height > JADE_GL_MAX_HEIGHT) return jade_fail(JADE_ERR_INVALID, "bad image size: jade_render_glare takes at most 1048560 rows");
  if (int rc = ex_resolve(s)) return rc;  // flush (its counters handed on, as the denoiser's) + k_resolve, compact tiles
  const int npx = s->ps.npx, W = s->rp.width, H = s->rp.height;
  if (npx == 0) return JADE_OK;
  const int npix = W * H;
  HIP_TRY(ex_alloc(s->b_gl_rgb, (size_t)npix * 12));
  float* frame = s->b_gl_rgb.as<float>();
  hipLaunchKernelGGL(k_gl_scatter, dim3((unsigned)((npx + JADE_GL_BLOCK - 1) / JADE_GL_BLOCK)), dim3(JADE_GL_BLOCK), 0, s->stream, s->rc,
                     s->b_tiles.as<int32_t>(), npx, s->b_out_rgb.as<uint32_t>(), s->b_gl_rgb.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  if (gp->strength != 0.0f)
    if (int rc = gl_run(s->stream, s->b_gl_pyr, W, H, gp, frame, frame)) return rc;
  const RenderConst none{};
  jade_meter m;
  memset(&m, 0, sizeof m);
  if (dp->exposure_mode == JADE_EXPOSURE_AUTO && (out_bgr8 || exposure_used))
    if (int rc = ex_meter(s->b_ex_rows, s->b_ex_meter, frame, npix, none, nullptr, s->stream, &m)) return rc;
  const float e = jade_meter_exposure(&m, dp);
  if (exposure_used) *exposure_used = e;
  if (out_bgr8) {
    HIP_TRY(ex_alloc(s->b_gl_bgr, (size_t)npix * 3));
    ex_launch_pack(frame, npix, none, nullptr, e, dp, s->b_gl_bgr.as<uint8_t>(), s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_bgr8, s->b_gl_bgr.p, (size_t)npix * 3, hipMemcpyDeviceToHost, s->stream));
  }
  if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, frame, (size_t)npix * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}
