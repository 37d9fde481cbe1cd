// jade_adaptive.hip — adaptive sampling's device side (include/jade_bvh.h: jade_render_adaptive, jade_render_error).
//
//   k_tile_error  one block of 256 threads per tile (a thread per pixel): streams the tile's K lanes of partial sums, turns each
//                 pixel's lanes into the error estimate of jade_bvh.h and takes the tile's maximum in LDS.  In a round of
//                 jade_render_adaptive it also decides: a converged tile's records get the stop offset added to their sample
//                 counters (PathState.hdr), so that no kernel starts another sample on them, and a tile that goes on is appended to
//                 the next round's active list (one atomic per block).
//
// The host glue (round loop, per-tile resolve, the noise map) sits beside jade_render_step in jade_hip.hip: it needs the scene.
#include <hip/hip_runtime.h>

#include <math.h>

#include "jade_device.h"

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

// The launch, for jade_hip.hip (hidden: libjade_hip.so exports only what the headers declare).  rel_error <= 0: the noise map only.
__attribute__((visibility("hidden"))) hipError_t adaptive_tile_error(hipStream_t stream, uint32_t n_tiles, const PathState& P, const RenderConst& R,
                                                                      const int32_t* tile_ids, const uint32_t* list, const int32_t* tile_n,
                                                                      double error_floor, float rel_error, int32_t target, uint32_t* next_list,
                                                                      uint32_t* next_count, int32_t* tile_spp, float* err_out, uint32_t* not_idle) {
  if (n_tiles == 0) return hipSuccess;
  const uint32_t rpp_log2 = 31u - (uint32_t)__builtin_clz((uint32_t)P.rpp);
  const uint32_t per_log2 = (31u - (uint32_t)__builtin_clz((uint32_t)JADE_SAMPLE_LANES)) - rpp_log2;  // samples per record per lane block
  const uint32_t stop_add = (1u << 21) << per_log2;  // + 2^31 on the next sample index (PathState.hdr)
  hipLaunchKernelGGL(k_tile_error, dim3(n_tiles), dim3(JADE_ERR_BLOCK), 0, stream, P, R, tile_ids, list, tile_n, error_floor, rel_error, target,
                     stop_add, next_list, next_count, tile_spp, err_out, not_idle);
  return hipGetLastError();
}
