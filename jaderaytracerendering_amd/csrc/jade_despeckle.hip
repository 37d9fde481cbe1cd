// jade_despeckle.hip — the despeckle pass (include/jade_bvh.h, "Despeckle, stated": jade_despeckle_defaults, jade_despeckle_image,
// jade_render_despeckle): kernels and host side.
//
//   k_ds_pack_image   a caller's frame (12 B per pixel) and variance (nullable: 0) -> the denoiser's record 0, float4 {rgb, variance}
//   k_ds_pack_tiles   the same records from the render's compact tiles (k_resolve's colour, k_pixel_variance's variance), image layout
//   k_despeckle<R>    one pass: record in, record out (ping-pong), the pixel's scale and the four counts.  One block of 256 threads
//                     makes 32 x 8 pixels from a (32 + 2R) x (8 + 2R) tile of luminances staged in LDS
//   k_ds_unpack       the records -> the caller's layout (colour 12 B, variance 4 B)
//   k_ds_pack_guides  the despeckled records + the guide sums (compact tiles) -> the filter's three records (dn_pack, jade_runtime.h):
//                     what k_dn_pack_tiles does for jade_render_denoise, with the despeckled colour and variance in the resolve's place
//
// No floating-point atomic: every output word has one writer, and a pass reads nothing that it writes.  The counts are integers: a
// wave takes each by ballot and popcount, and its lanes 0..3 add the four of them to the report in one 64-bit integer atomic
// instruction (lanes whose count is 0 stay out of it).  The report on the device is JADE_DS_ROWS rows of four words, a wave adding to
// the row of its number, and the host adds the rows up: with ONE row every wave of a frame would queue at one cache line of the L2
// (measured on C3 at 1080p, radius 2: 396 us a pass with one row, 20 us with the rows).  For the same reason the first word counts the UNUSABLE in-image
// pixels, which are rare, and n_usable is the frame's pixels less their sum: a wave of a clean frame with nothing above adds nothing.
//
// k_despeckle's LDS, (32 + 2R) x (8 + 2R) floats per block, dense (row stride 32 + 2R words): 1360 / 1728 / 2128 B at R = 1 / 2 / 3.
//   T[r][c] = Y of pixel (32 bx - R + c, 8 by - R + r), or -inf where that pixel is outside the image or unusable: every usable Y is
//   finite, so -inf is never a neighbour's value, and a K-th largest of -inf says "fewer than K neighbours".
// Reads (ds_read_b32, banks (a/4) mod 32, groups = the two 32-lane halves of a wave): a half is 32 consecutive x of one row, so a
// tap reads 32 consecutive words - one 128-B bank row, no conflict, whatever R makes of the row stride.  (2R + 1)^2 - 1 = 8 / 24 / 48
// taps per thread, all at compile-time offsets from one address.
// Writes (ds_write_b32, the same banks and groups): a thread stores its own pixel's Y at T[ly + R][lx + R] - a half stores 32
// consecutive words - and the 84 / 176 / 276 halo entries are dealt in order over the threads: the two R-row bands above and below
// run along rows (consecutive words but for one row change per half: conflict-free or 2-way on 2R words), the side bands are 2R
// words per row (a half covers 32 / 2R rows: words r (32 + 2R) + {0..R-1, 32 + R..}, 2-way at most for R = 1, 2 and up to 4-way
// for the 6-word runs of R = 3).  276 of 788 stores at worst, once per block, against 48 x 256 reads.
// A pixel's 16-B record is read once by its own thread and (32 + 2R)(8 + 2R) / 256 - 1 = 0.33 / 0.69 / 1.08 times as somebody's halo.
#include <math.h>

#include <cmath>
#include <cstring>

#include "jade_runtime.h"

#define JADE_DS_BLOCK 256
#define JADE_DS_TW 32                      /* pixels of a k_despeckle block: 32 x 8 */
#define JADE_DS_TH 8
#define JADE_DS_MAX_HEIGHT (JADE_DS_TH * 65535) /* rows go into grid.y (at most 65535 blocks), 8 per block */
#define JADE_DS_ROWS 256                   /* rows of the device report, 32 B each (a power of two) */
#define JADE_DS_REPORT_BYTES (JADE_DS_ROWS * 4 * sizeof(unsigned long long))

// Y(p), three products and two sums (jade_bvh.h)
static __host__ __device__ __forceinline__ float ds_lum(float r, float g, float b) { return (0.3f * r + 0.6f * g) + 0.1f * b; }
static __host__ __device__ __forceinline__ bool ds_finite(float x) { return x - x == 0.0f; }
static __host__ __device__ __forceinline__ bool ds_usable(float r, float g, float b, float y) {
  return ds_finite(r) && ds_finite(g) && ds_finite(b) && ds_finite(y);
}

// what a neighbour contributes: its Y, or -inf
static __device__ __forceinline__ float ds_key(const float4 a) {
  const float y = ds_lum(a.x, a.y, a.z);
  return ds_usable(a.x, a.y, a.z, y) ? y : -INFINITY;
}

struct DsPass {
  int W, H, K;
  float g, f, zz;
  int has_v;  // record.w is a variance (otherwise it is carried through untouched)
  int first;  // the first pass: counts the unusable pixels and starts the scale at 1.0f
};

__global__ __launch_bounds__(JADE_DS_BLOCK) void k_ds_pack_image(const uint32_t* __restrict__ rgb, const uint32_t* __restrict__ var, int npix,
                                                                 uint4* __restrict__ A) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const uint32_t* c = rgb + 3 * (size_t)p;
  A[p] = make_uint4(c[0], c[1], c[2], var ? var[p] : 0u);
}

// (the full frame: every in-image pixel belongs to an owned tile)
__global__ __launch_bounds__(JADE_DS_BLOCK) void k_ds_pack_tiles(RenderConst R, const int32_t* __restrict__ tile_ids, int npx, const uint32_t* __restrict__ rgb,
                                                                 const uint32_t* __restrict__ var, uint4* __restrict__ A) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  int x, y;
  if (!dn_pixel_xy(R, tile_ids, p, &x, &y)) return;
  const uint32_t* c = rgb + 3 * (size_t)p;
  A[(size_t)y * R.width + x] = make_uint4(c[0], c[1], c[2], var[p]);
}

__global__ __launch_bounds__(JADE_DS_BLOCK) void k_ds_unpack(const uint4* __restrict__ A, int npix, uint32_t* __restrict__ rgb, uint32_t* __restrict__ var) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const uint4 a = A[p];
  uint32_t* c = rgb + 3 * (size_t)p;
  c[0] = a.x;
  c[1] = a.y;
  c[2] = a.z;
  if (var) var[p] = a.w;
}

// Ain: the despeckled records (image layout); may be A (a thread reads and writes its own pixel only)
__global__ __launch_bounds__(JADE_DS_BLOCK) void k_ds_pack_guides(RenderConst R, const int32_t* tile_ids, int npx, const float4* Ain, const float4* acc_az,
                                                                  const float4* acc_n, float4* A, float4* N, float4* L) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  int x, y;
  if (!dn_pixel_xy(R, tile_ids, p, &x, &y)) return;
  const size_t o = (size_t)y * R.width + x;
  const float4 a = Ain[o], az = acc_az[p], n = acc_n[p];
  dn_pack(a.x, a.y, a.z, a.w, az.x, az.y, az.z, n.x, n.y, n.z, az.w, A, N, L, o);
}

// One pass (jade_bvh.h).  in and out are different buffers; scale_in may be scale_out (a thread's own word), both null: no scale kept.
// Every index is checked against the image: an out-of-image tile entry is -inf and is never loaded.
template <int R>
__global__ __launch_bounds__(JADE_DS_BLOCK) void k_despeckle(const float4* __restrict__ in, float4* __restrict__ out, DsPass a, const float* scale_in,
                                                             float* scale_out, unsigned long long* report) {
  constexpr int TWP = JADE_DS_TW + 2 * R, THP = JADE_DS_TH + 2 * R;
  constexpr int NHALO = TWP * THP - JADE_DS_TW * JADE_DS_TH, BAND = R * TWP;
  __shared__ float T[THP * TWP];
  const int t = threadIdx.x, lx = t & (JADE_DS_TW - 1), ly = t / JADE_DS_TW;
  const int x0 = (int)blockIdx.x * JADE_DS_TW, y0 = (int)blockIdx.y * JADE_DS_TH;
  const int x = x0 + lx, y = y0 + ly;
  const bool inside = x < a.W && y < a.H;
  const size_t p = (size_t)y * a.W + x;
  float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float yp = 0.0f;
  bool usable = false;
  if (inside) {
    rec = in[p];
    yp = ds_lum(rec.x, rec.y, rec.z);
    usable = ds_usable(rec.x, rec.y, rec.z, yp);
  }
  T[(ly + R) * TWP + lx + R] = usable ? yp : -INFINITY;
  for (int h = t; h < NHALO; h += JADE_DS_BLOCK) {
    int r, c;
    if (h < 2 * BAND) {  // the R rows above, then the R rows below
      r = h / TWP;
      c = h - r * TWP;
      if (r >= R) r += JADE_DS_TH;
    } else {  // the R columns left and right of each of the block's rows
      const int s = h - 2 * BAND;
      r = s / (2 * R);
      c = s - r * (2 * R);
      r += R;
      if (c >= R) c += JADE_DS_TW;
    }
    const int gx = x0 - R + c, gy = y0 - R + r;
    float key = -INFINITY;
    if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) key = ds_key(in[(size_t)gy * a.W + gx]);
    T[r * TWP + c] = key;
  }
  __syncthreads();
  // the four largest neighbours, t0 >= t1 >= t2 >= t3: a max / min insertion chain (a tie goes in as an entry of its own)
  float t0 = -INFINITY, t1 = -INFINITY, t2 = -INFINITY, t3 = -INFINITY;
  const float* centre = &T[(ly + R) * TWP + lx + R];
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      if (dx == 0 && dy == 0) continue;
      float v = centre[dy * TWP + dx];
      float m = fmaxf(t0, v);
      v = fminf(t0, v);
      t0 = m;
      m = fmaxf(t1, v);
      v = fminf(t1, v);
      t1 = m;
      m = fmaxf(t2, v);
      v = fminf(t2, v);
      t2 = m;
      t3 = fmaxf(t3, v);
    }
  }
  const float B = a.K == 1 ? t0 : a.K == 2 ? t1 : a.K == 3 ? t2 : t3;
  const float C = a.g * (B > 0.0f ? B : 0.0f) + a.f;
  const bool above = usable && B != -INFINITY && yp > C;
  bool established = false;
  if (above && a.has_v) {
    const float v = rec.w, d = yp - C;
    established = ds_finite(v) && v >= 0.0f && d * d > a.zz * v;
  }
  const bool clamped = above && !established;
  float k = 1.0f;
  if (clamped) {
    k = C / yp;
    rec.x = k * rec.x;
    rec.y = k * rec.y;
    rec.z = k * rec.z;
    if (a.has_v) rec.w = (k * k) * rec.w;
  }
  if (inside) {
    out[p] = rec;
    if (scale_out) {
      float s = a.first ? 1.0f : scale_in[p];
      if (clamped) s = s * k;
      scale_out[p] = s;
    }
  }
  const unsigned long long n_unusable = (unsigned long long)__popcll(__ballot(inside && !usable && a.first));
  const unsigned long long n_above = (unsigned long long)__popcll(__ballot(above));
  const unsigned long long n_established = (unsigned long long)__popcll(__ballot(established));
  const unsigned long long n_clamped = (unsigned long long)__popcll(__ballot(clamped));
  const int lane = t & 63;
  if (lane < 4) {
    const unsigned long long n = lane == 0 ? n_unusable : lane == 1 ? n_above : lane == 2 ? n_established : n_clamped;
    const unsigned wave = ((unsigned)blockIdx.y * gridDim.x + blockIdx.x) * (JADE_DS_BLOCK / 64) + ((unsigned)t >> 6);
    if (n) atomicAdd(report + 4 * (wave & (JADE_DS_ROWS - 1)) + lane, n);
  }
}

// ------------------------------------------------------------------------------------------------------------ host side --

static inline unsigned ds_grid(size_t n) { return (unsigned)((n + JADE_DS_BLOCK - 1) / JADE_DS_BLOCK); }

void jade_despeckle_defaults(jade_despeckle_params* p) {
  if (!p) return;
  // the starting point of the sweep, and what it kept
  p->iterations = 1;
  p->radius = 1;
  p->rank = 2;
  p->gain = 2.0f;
  p->floor = 0.0f;
  p->sigmas = 2.0f;
}

static int ds_check(const jade_despeckle_params* p) {
  if (!p) return jade_fail(JADE_ERR_INVALID, "null despeckle parameters");
  if (p->iterations < 0 || p->iterations > 4) return jade_fail(JADE_ERR_INVALID, "iterations must be 0..4");
  if (p->radius < 1 || p->radius > 3) return jade_fail(JADE_ERR_INVALID, "radius must be 1..3");
  if (p->rank < 1 || p->rank > 4) return jade_fail(JADE_ERR_INVALID, "rank must be 1..4");
  if (!std::isfinite(p->gain) || !(p->gain >= 1.0f)) return jade_fail(JADE_ERR_INVALID, "gain must be finite and >= 1");
  if (!std::isfinite(p->floor) || !(p->floor >= 0.0f)) return jade_fail(JADE_ERR_INVALID, "floor must be finite and >= 0");
  if (!std::isfinite(p->sigmas) || !(p->sigmas >= 0.0f)) return jade_fail(JADE_ERR_INVALID, "sigmas must be finite and >= 0");
  return JADE_OK;
}

// n_usable of a host frame whose pixels lie `stride` floats apart (3: a frame, 4: records), by the statement's own operations
static uint64_t ds_count_usable(const float* px, size_t npix, int stride) {
  uint64_t n = 0;
  for (size_t i = 0; i < npix; ++i) {
    const float* c = px + i * (size_t)stride;
    n += ds_usable(c[0], c[1], c[2], ds_lum(c[0], c[1], c[2])) ? 1u : 0u;
  }
  return n;
}

// The passes on records at rec[0] (W x H, image layout), ping-pong with rec[1]; *cur: where the result lies.  dev_scale (nullable):
// W x H floats, written by every pass.  dev_report: JADE_DS_ROWS x 4 64-bit words, zeroed here.  iterations >= 1.
static int ds_run(hipStream_t stream, int W, int H, const jade_despeckle_params* dp, bool has_v, float4* const* rec, float* dev_scale,
                  unsigned long long* dev_report, int* cur) {
  HIP_TRY(hipMemsetAsync(dev_report, 0, JADE_DS_REPORT_BYTES, stream));
  const dim3 grid((unsigned)((W + JADE_DS_TW - 1) / JADE_DS_TW), (unsigned)((H + JADE_DS_TH - 1) / JADE_DS_TH));
  DsPass a{W, H, dp->rank, dp->gain, dp->floor, dp->sigmas * dp->sigmas, has_v ? 1 : 0, 1};
  int c = 0;
  for (int i = 0; i < dp->iterations; ++i) {
    a.first = i == 0 ? 1 : 0;
    if (dp->radius == 1)
      hipLaunchKernelGGL(k_despeckle<1>, grid, dim3(JADE_DS_BLOCK), 0, stream, rec[c], rec[c ^ 1], a, dev_scale, dev_scale, dev_report);
    else if (dp->radius == 2)
      hipLaunchKernelGGL(k_despeckle<2>, grid, dim3(JADE_DS_BLOCK), 0, stream, rec[c], rec[c ^ 1], a, dev_scale, dev_scale, dev_report);
    else
      hipLaunchKernelGGL(k_despeckle<3>, grid, dim3(JADE_DS_BLOCK), 0, stream, rec[c], rec[c ^ 1], a, dev_scale, dev_scale, dev_report);
    HIP_TRY(hipGetLastError());
    c ^= 1;
  }
  *cur = c;
  return JADE_OK;
}

// the device report's rows added up; n_usable = the frame's pixels less the unusable ones
static void ds_report_from(const unsigned long long* rows, size_t npix, jade_despeckle_report* out) {
  unsigned long long w[4] = {0, 0, 0, 0};
  for (int r = 0; r < JADE_DS_ROWS; ++r)
    for (int k = 0; k < 4; ++k) w[k] += rows[4 * r + k];
  out->n_usable = npix - w[0];
  out->n_above = w[1];
  out->n_established = w[2];
  out->n_clamped = w[3];
}

int jade_despeckle_image(int device_id, int32_t width, int32_t height, const float* rgb, const float* variance, const jade_despeckle_params* dp,
                         float* out_rgb, float* out_variance, float* out_scale, jade_despeckle_report* report) {
  if (!rgb || !out_rgb) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 3 || height > JADE_DS_MAX_HEIGHT)
    return jade_fail(JADE_ERR_INVALID, "bad image size");
  if (out_variance && !variance) return jade_fail(JADE_ERR_INVALID, "out_variance needs variance");
  if (int rc = ds_check(dp)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return jade_fail(JADE_ERR_DEVICE, "no HIP device");
  if (device_id < 0 || device_id >= ndev) return jade_fail(JADE_ERR_INVALID, "device_id out of range");
  const size_t npix = (size_t)width * (size_t)height;
  if (dp->iterations == 0) {  // the identity, bit for bit: no kernel
    if (report) {
      memset(report, 0, sizeof *report);
      report->n_usable = ds_count_usable(rgb, npix, 3);
    }
    if (out_rgb != rgb) memmove(out_rgb, rgb, npix * 12);
    if (out_variance && out_variance != variance) memmove(out_variance, variance, npix * 4);
    if (out_scale) std::fill(out_scale, out_scale + npix, 1.0f);
    return JADE_OK;
  }
  HIP_TRY(hipSetDevice(device_id));
  hipStream_t stream = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } guard{stream};
  DevBuf b_rgb, b_var, b_rec[2], b_scale, b_report;
  HIP_TRY(upload(b_rgb, rgb, npix * 3, stream));
  if (variance) HIP_TRY(upload(b_var, variance, npix, stream));
  for (DevBuf& b : b_rec) HIP_TRY(b.alloc(npix * 16));
  if (out_scale) HIP_TRY(b_scale.alloc(npix * 4));
  HIP_TRY(b_report.alloc(JADE_DS_REPORT_BYTES));
  float4* rec[2] = {b_rec[0].as<float4>(), b_rec[1].as<float4>()};
  hipLaunchKernelGGL(k_ds_pack_image, dim3(ds_grid(npix)), dim3(JADE_DS_BLOCK), 0, stream, b_rgb.as<uint32_t>(), variance ? b_var.as<uint32_t>() : nullptr,
                     (int)npix, b_rec[0].as<uint4>());
  HIP_TRY(hipGetLastError());
  int cur = 0;
  if (int rc = ds_run(stream, width, height, dp, variance != nullptr, rec, out_scale ? b_scale.as<float>() : nullptr, b_report.as<unsigned long long>(), &cur))
    return rc;
  hipLaunchKernelGGL(k_ds_unpack, dim3(ds_grid(npix)), dim3(JADE_DS_BLOCK), 0, stream, b_rec[cur].as<uint4>(), (int)npix, b_rgb.as<uint32_t>(),
                     out_variance ? b_var.as<uint32_t>() : nullptr);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words(JADE_DS_ROWS * 4);
  HIP_TRY(hipMemcpyAsync(out_rgb, b_rgb.p, npix * 12, hipMemcpyDeviceToHost, stream));
  if (out_variance) HIP_TRY(hipMemcpyAsync(out_variance, b_var.p, npix * 4, hipMemcpyDeviceToHost, stream));
  if (out_scale) HIP_TRY(hipMemcpyAsync(out_scale, b_scale.p, npix * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(words.data(), b_report.p, JADE_DS_REPORT_BYTES, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (report) ds_report_from(words.data(), npix, report);
  return JADE_OK;
}

int jade_render_despeckle(jade_scene* s, const jade_despeckle_params* dp, const jade_denoise_params* dn, int tonemap, float limit, float* out_rgb,
                          uint8_t* out_bgr8, float* out_scale, jade_despeckle_report* report) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (int rc = ds_check(dp)) return rc;
  if (dn)
    if (int rc = dn_check_params(dn)) return rc;
  if (tonemap != JADE_TONEMAP_ACES && tonemap != JADE_TONEMAP_REINHARD) return jade_fail(JADE_ERR_INVALID, "unknown tone operator");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  if (s->rp.tile_nranks > 1)
    return jade_fail(JADE_ERR_UNSUPPORTED,
                     "jade_render_despeckle needs the full frame: gather rgb and jade_render_guides' variance, then jade_despeckle_image");
  if (s->rp.height > JADE_DS_MAX_HEIGHT) return jade_fail(JADE_ERR_INVALID, "bad image size: jade_render_despeckle takes at most 524280 rows");
  if (dn)
    for (int32_t n : dn_tile_counts(s))
      if (!(n >= 2 && (n <= JADE_SAMPLE_LANES || n % JADE_SAMPLE_LANES == 0)))
        return jade_fail(JADE_ERR_INVALID, "a tile's sample count (" + std::to_string(n) + ") cannot give a variance: n >= 2, and a multiple of " +
                                               std::to_string(JADE_SAMPLE_LANES) + " above it");
  if (int rc = ex_resolve(s)) return rc;  // flush (its counters handed on, as the denoiser's) + k_resolve, compact tiles
  const int npx = s->ps.npx, W = s->rp.width, H = s->rp.height;
  if (report) memset(report, 0, sizeof *report);
  if (npx == 0) return JADE_OK;
  const size_t npix = (size_t)W * (size_t)H;
  if (int rc = dn_variance(s)) return rc;
  for (DevBuf& b : s->b_dn_rec) HIP_TRY(ex_alloc(b, npix * 16));
  float4* rec[4] = {s->b_dn_rec[0].as<float4>(), s->b_dn_rec[1].as<float4>(), s->b_dn_rec[2].as<float4>(), s->b_dn_rec[3].as<float4>()};
  hipLaunchKernelGGL(k_ds_pack_tiles, dim3(ds_grid((size_t)npx)), dim3(JADE_DS_BLOCK), 0, s->stream, s->rc, s->b_tiles.as<int32_t>(), npx,
                     s->b_out_rgb.as<uint32_t>(), s->b_dn_var.as<uint32_t>(), s->b_dn_rec[0].as<uint4>());
  HIP_TRY(hipGetLastError());
  int cur = 0;
  std::vector<unsigned long long> words(JADE_DS_ROWS * 4, 0ull);
  if (out_scale) HIP_TRY(ex_alloc(s->b_ds_scale, npix * 4));
  if (dp->iterations > 0) {
    HIP_TRY(ex_alloc(s->b_ds_report, JADE_DS_REPORT_BYTES));
    if (int rc = ds_run(s->stream, W, H, dp, true, rec, out_scale ? s->b_ds_scale.as<float>() : nullptr, s->b_ds_report.as<unsigned long long>(), &cur))
      return rc;
    HIP_TRY(hipMemcpyAsync(words.data(), s->b_ds_report.p, JADE_DS_REPORT_BYTES, hipMemcpyDeviceToHost, s->stream));
  } else if (report) {  // no pass: n_usable from the frame itself
    std::vector<float> host(npix * 4);
    HIP_TRY(hipMemcpyAsync(host.data(), rec[0], npix * 16, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    words[0] = npix - ds_count_usable(host.data(), npix, 4);
  }
  jade_denoise_params none{};  // the output kernel alone
  float4* order[4] = {rec[cur], rec[cur ^ 1], rec[2], rec[3]};
  if (dn) {
    if (int rc = dn_guides(s, dn->guide_spp)) return rc;
    // the filter's records from the despeckled colour and variance: usable or not is decided from these, as jade_denoise_image decides it
    hipLaunchKernelGGL(k_ds_pack_guides, dim3(ds_grid((size_t)npx)), dim3(JADE_DS_BLOCK), 0, s->stream, s->rc, s->b_tiles.as<int32_t>(), npx, rec[cur],
                       s->b_dn_az.as<float4>(), s->b_dn_n.as<float4>(), rec[cur], rec[2], rec[3]);
    HIP_TRY(hipGetLastError());
  }
  if (out_rgb) HIP_TRY(ex_alloc(s->b_dn_rgb, npix * 12));
  if (out_bgr8) HIP_TRY(ex_alloc(s->b_dn_bgr, npix * 3));
  if (int rc = dn_filter_out(s->stream, W, H, dn ? dn : &none, tonemap, limit, out_rgb ? s->b_dn_rgb.as<float>() : nullptr,
                             out_bgr8 ? s->b_dn_bgr.as<uint8_t>() : nullptr, order))
    return rc;
  if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, s->b_dn_rgb.p, npix * 12, hipMemcpyDeviceToHost, s->stream));
  if (out_bgr8) HIP_TRY(hipMemcpyAsync(out_bgr8, s->b_dn_bgr.p, npix * 3, hipMemcpyDeviceToHost, s->stream));
  if (out_scale) {
    if (dp->iterations > 0) {
      HIP_TRY(hipMemcpyAsync(out_scale, s->b_ds_scale.p, npix * 4, hipMemcpyDeviceToHost, s->stream));
    } else {
      std::fill(out_scale, out_scale + npix, 1.0f);
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (report) ds_report_from(words.data(), npix, report);
  return JADE_OK;
}
