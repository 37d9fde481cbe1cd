// jade_adaptive.hip — adaptive sampling (include/jade_bvh.h: jade_render_adaptive, jade_render_error): its kernel and the host side.
//
//   k_tile_error  one block of 256 threads per tile (a thread per pixel): streams the tile's K lanes of partial sums, turns each
//                 pixel's lanes into the error estimate of jade_bvh.h and takes the tile's maximum in LDS.  In a round of
//                 jade_render_adaptive it also decides: a converged tile's records get the stop offset added to their sample
//                 counters (PathState.hdr), so that no kernel starts another sample on them, and a tile that goes on is appended to
//                 the next round's active list (one atomic per block).
#include <math.h>

#include <cmath>
#include <cstring>

#include "jade_runtime.h"

#define JADE_ERR_BLOCK 256      /* one thread per pixel of a 16x16 tile */
#define JADE_ERR_STAGE_LANES 4  /* lanes of a tile staged through LDS at a time: 4 x 3 KB */

typedef float jade_err_v4f __attribute__((ext_vector_type(4)));

// Lane l of owned pixel t*256 + i sits at floats (l * npx + t * 256 + i) * 3 .. + 2 (PathState.sum).  npx is a multiple of 256, so
// one (lane, tile) is 3 KB, contiguous and 16-B aligned: 192 16-B loads by the block, handed to each pixel's thread through LDS.
__global__ __launch_bounds__(JADE_ERR_BLOCK) void k_tile_error(PathState P, RenderConst R, const int32_t* tile_ids, const uint32_t* list,
                                                              const int32_t* tile_n, double error_floor, float rel_error, int32_t target,
                                                              uint32_t stop_add, uint32_t* next_list, uint32_t* next_count, int32_t* tile_spp,
                                                              float* err_out, uint32_t* not_idle) {
  __shared__ jade_err_v4f stage[JADE_ERR_STAGE_LANES * 192];
  __shared__ float wave_max[JADE_ERR_BLOCK / 64];
  const uint32_t t = list ? list[blockIdx.x] : blockIdx.x;  // owned tile
  const int i = threadIdx.x;
  const int64_t n = tile_n ? tile_n[t] : target;  // samples the tile has (a round: every active tile is at the round's target)
  // K = min(n, JADE_SAMPLE_LANES) lanes of c = n / K samples each.  Not estimable: n < 2, or n above the lane count and not a
  // multiple of it (the lanes would hold unequal counts).
  const bool estimable = n >= 2 && (n <= JADE_SAMPLE_LANES || n % JADE_SAMPLE_LANES == 0);
  const int K = (int)(n < JADE_SAMPLE_LANES ? n : JADE_SAMPLE_LANES);
  const double c = estimable ? (double)(n / K) : 1.0;
  // one pass over the lanes, shifted by lane 0's value: the two-pass result without its second read, and no cancellation when the
  // lanes agree
  double y0 = 0.0, sd = 0.0, sdd = 0.0;
  if (estimable) {
    const jade_err_v4f* base = reinterpret_cast<const jade_err_v4f*>(P.sum + (size_t)t * 256 * 3);
    const size_t lane_step = (size_t)P.npx * 3 / 4;  // 16-B words per lane
    const float* mine = reinterpret_cast<const float*>(stage) + 3 * i;
    for (int l0 = 0; l0 < K; l0 += JADE_ERR_STAGE_LANES) {
      const int nv = K - l0 < JADE_ERR_STAGE_LANES ? K - l0 : JADE_ERR_STAGE_LANES;
      for (int j = i; j < nv * 192; j += JADE_ERR_BLOCK) {
        const int q = j / 192;
        stage[j] = __builtin_nontemporal_load(base + (size_t)(l0 + q) * lane_step + (j - q * 192));
      }
      __syncthreads();
      for (int q = 0; q < nv; ++q) {
        const float* s = mine + q * 768;
        const double y = (0.3 * (double)s[0] + 0.6 * (double)s[1] + 0.1 * (double)s[2]) / c;
        if (l0 + q == 0) y0 = y;
        const double d = y - y0;
        sd += d;
        sdd += d * d;
      }
      __syncthreads();
    }
  }
  float err = __builtin_nanf("");
  if (estimable) {
    // m = y0 + sd / K;  sum (Y_l - m)^2 = sdd - sd^2 / K
    const double kk = (double)K;
    const double m = y0 + sd / kk;
    double ss = sdd - sd * sd / kk;
    if (ss < 0.0) ss = 0.0;
    err = (float)(sqrt(ss / (kk * (kk - 1.0))) / (m + error_floor));
  }
  if (err_out) err_out[(size_t)t * 256 + i] = err;
  if (!(rel_error > 0.0f)) return;  // the noise map only
  // the tile's error: the maximum over its in-image pixels; an estimate that is NaN counts as not converged
  const int gid = tile_ids[t];
  const int x = (gid % R.tiles_x) * JADE_TILE_SIZE + (i & 15), y = (gid / R.tiles_x) * JADE_TILE_SIZE + (i >> 4);
  float v = (x < R.width && y < R.height) ? (err == err ? err : INFINITY) : -INFINITY;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  if ((i & 63) == 0) wave_max[i >> 6] = v;
  __syncthreads();
  float tmax = wave_max[0];
#pragma unroll
  for (int w = 1; w < JADE_ERR_BLOCK / 64; ++w) tmax = fmaxf(tmax, wave_max[w]);
  if (tmax <= rel_error) {
    // stop: the tile's records (m * npx + t * 256 + i, m < rpp) are idle after the round's flush; their next sample index moves up by
    // 2^31 (PathState.hdr), past any target
    for (int m = 0; m < P.rpp; ++m) {
      uint32_t* h = reinterpret_cast<uint32_t*>(P.hdr + (size_t)m * P.npx + (size_t)t * 256 + i);
#if JADE_DEBUG_EXPORTS
      if ((h[2] & 255u) != ST_IDLE) atomicAdd(not_idle, 1u);
#endif
      h[1] += stop_add;
    }
    if (i == 0) tile_spp[t] = target;
  } else if (i == 0) {
    next_list[atomicAdd(next_count, 1u)] = t;
  }
}

// ---------------------------------------------------------------- host side --

// k_tile_error over n_tiles owned tiles (all of them, or those of `list`).  rel_error <= 0: the noise map only.
static void launch_tile_error(jade_scene* s, uint32_t n_tiles, const uint32_t* list, const int32_t* tile_n, double error_floor, float rel_error,
                              int32_t target, uint32_t* next_list, uint32_t* next_count, int32_t* tile_spp, float* err_out, uint32_t* not_idle) {
  const PathState& P = s->ps;
  const uint32_t rpp_log2 = 31u - (uint32_t)__builtin_clz((uint32_t)P.rpp);
  const uint32_t per_log2 = (31u - (uint32_t)__builtin_clz((uint32_t)JADE_SAMPLE_LANES)) - rpp_log2;  // samples per record per lane block
  const uint32_t stop_add = (1u << 21) << per_log2;  // + 2^31 on the next sample index (PathState.hdr)
  hipLaunchKernelGGL(k_tile_error, dim3(n_tiles), dim3(JADE_ERR_BLOCK), 0, s->stream, P, s->rc, s->b_tiles.as<int32_t>(), list, tile_n, error_floor,
                     rel_error, target, stop_add, next_list, next_count, tile_spp, err_out, not_idle);
}

// Rounds of step + flush at the targets min_spp, 2 min_spp, ... spp; after each round below the cap k_tile_error stops the converged
// tiles (their records' sample counters move past every target, PathState.hdr) and lists the others.  The host waits once per round,
// for the number of tiles that go on.  The render is begun with spp = the cap, so records per pixel and sum lanes are a cap render's.
int jade_render_adaptive(jade_scene* s, const jade_render_params* rp, int32_t min_spp, float rel_error, float error_floor, float* out_rgb,
                         uint8_t* out_bgr8, int32_t* out_tile_spp, jade_stats* st) {
  if (!s || !rp) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (rp->spp <= 0) return jade_fail(JADE_ERR_INVALID, "spp (the cap) must be positive");
  if (min_spp < 2 || min_spp > rp->spp || (min_spp & (min_spp - 1)) != 0)
    return jade_fail(JADE_ERR_INVALID, "min_spp must be a power of two with 2 <= min_spp <= spp");
  if (!std::isfinite(rel_error) || !(rel_error > 0.0f)) return jade_fail(JADE_ERR_INVALID, "rel_error must be finite and > 0");
  if (!std::isfinite(error_floor) || !(error_floor > 0.0f)) return jade_fail(JADE_ERR_INVALID, "error_floor must be finite and > 0");
  if (s->tun.pixel_rotate) return jade_fail(JADE_ERR_UNSUPPORTED, "adaptive sampling with JADE_PIXEL_ROTATE (records move between pixels)");
  if (int rc = jade_render_begin(s, rp)) return rc;
  const size_t nt = s->tile_ids.size();
  uint32_t n_active = s->ps.npix ? (uint32_t)nt : 0u;
  if (n_active) {
    std::vector<uint32_t> all(nt);
    for (size_t t = 0; t < nt; ++t) all[t] = (uint32_t)t;
    std::vector<int32_t> cap(nt, rp->spp);  // a tile that never stops ends at the cap
    HIP_TRY(upload(s->b_alist[0], all.data(), nt, s->stream));
    HIP_TRY(upload(s->b_tile_n, cap.data(), nt, s->stream));
    HIP_TRY(s->b_alist[1].alloc(nt * 4));
    HIP_TRY(s->b_actl.alloc(8));
    HIP_TRY(ensure_events(s->ev_err));
  }
  int cur = 0;
  for (int32_t prev = 0, target = min_spp;;) {
    if (int rc = jade_render_step(s, target - prev, st)) return rc;
    if (int rc = jade_render_flush(s, st)) return rc;
    if (target >= rp->spp || n_active == 0) break;
    HIP_TRY(hipMemsetAsync(s->b_actl.p, 0, 8, s->stream));
    HIP_TRY(hipEventRecord(s->ev_err[0], s->stream));
    uint32_t* ctl = s->b_actl.as<uint32_t>();
    launch_tile_error(s, n_active, s->b_alist[cur].as<uint32_t>(), nullptr, (double)error_floor, rel_error, target, s->b_alist[cur ^ 1].as<uint32_t>(), ctl,
                      s->b_tile_n.as<int32_t>(), nullptr, ctl + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev_err[1], s->stream));
    uint32_t h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h, ctl, 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev_err[0], s->ev_err[1]));
    if (st) {
      st->kernel_ms += ms;
      st->host_syncs += 1;
    }
    if (h[1]) return jade_fail(JADE_ERR_DEVICE, "adaptive: " + std::to_string(h[1]) + " records of stopped tiles were not idle");  // (debug builds count them)
    n_active = h[0];
    cur ^= 1;
    if (n_active == 0) break;
    prev = target;
    target = (int32_t)std::min<int64_t>(2 * (int64_t)target, rp->spp);
  }
  // each tile's count, once; its 1 / n exactly as resolve_to makes the uniform one
  s->tile_n.assign(nt, rp->spp);
  if (nt && s->ps.npix) {
    HIP_TRY(hipMemcpyAsync(s->tile_n.data(), s->b_tile_n.p, nt * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::vector<float> inv(nt);
    for (size_t t = 0; t < nt; ++t) inv[t] = (float)(1.0 / (double)s->tile_n[t]);
    HIP_TRY(upload(s->b_tile_inv, inv.data(), nt, s->stream));
  }
  s->adaptive_done = true;
  if (out_tile_spp) {
    const size_t all = (size_t)s->rc.tiles_x * (size_t)((rp->height + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE);
    std::fill(out_tile_spp, out_tile_spp + all, 0);
    for (size_t t = 0; t < nt; ++t) out_tile_spp[s->tile_ids[t]] = s->tile_n[t];
  }
  if (!out_rgb && !out_bgr8) return jade_render_flush(s, nullptr);
  return jade_render_resolve(s, out_rgb, out_bgr8);
}

int jade_render_error(jade_scene* s, float error_floor, float* out_error) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (!out_error) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (!std::isfinite(error_floor) || !(error_floor > 0.0f)) return jade_fail(JADE_ERR_INVALID, "error_floor must be finite and > 0");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = jade_render_flush(s, nullptr)) return rc;
  const int npx = s->ps.npx;
  if (npx == 0) return JADE_OK;
  const size_t nt = s->tile_ids.size();
  std::vector<int32_t> n(nt, (int32_t)std::min<int64_t>(s->spp_done, INT32_MAX));
  if (!s->tile_n.empty()) n = s->tile_n;
  DevBuf b_n;
  HIP_TRY(upload(b_n, n.data(), nt, s->stream));
  HIP_TRY(s->b_err.alloc((size_t)npx * 4));
  launch_tile_error(s, (uint32_t)nt, nullptr, b_n.as<int32_t>(), (double)error_floor, 0.0f, 0, nullptr, nullptr, nullptr, s->b_err.as<float>(), nullptr);
  HIP_TRY(hipGetLastError());
  std::vector<float> e((size_t)npx);
  HIP_TRY(hipMemcpyAsync(e.data(), s->b_err.p, e.size() * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // scatter the compact tiles into the caller's map, as jade_render_resolve_ex does with the radiance
  const int W = s->rp.width;
  for_each_owned_tile(s->tile_ids, W, s->rp.height, [&](size_t t, int x0, int y0, int ww, int hh) {
    for (int ly = 0; ly < hh; ++ly) memcpy(out_error + (size_t)(y0 + ly) * W + x0, e.data() + t * 256 + (size_t)ly * 16, (size_t)ww * 4);
  });
  return JADE_OK;
}
