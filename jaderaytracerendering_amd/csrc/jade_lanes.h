// jade_lanes.h — the per-pixel lane statistics of a tile (include/jade_bvh.h): the variance of jade_render_guides /
// jade_render_denoise (k_pixel_variance, jade_denoise.hip).  These are k_tile_error's statements (jade_adaptive.hip), the same loop over
// the same LDS staging.  k_tile_error keeps its own inline copy: calling this function from it changed its generated code (VGPRs 34 -> 24;
// the compiler unrolls the inner loop differently once it sits in a function), and k_tile_error's code is to stay as measured.
#pragma once
#include <hip/hip_runtime.h>

#include "jade_device.h"

#define JADE_ERR_BLOCK 256      /* one thread per pixel of a 16x16 tile */
#define JADE_ERR_STAGE_LANES 4  /* lanes of a tile staged through LDS at a time: 4 x 3 KB */

typedef float jade_err_v4f __attribute__((ext_vector_type(4)));

// A tile with n samples: K = min(n, JADE_SAMPLE_LANES) lanes of c = n / K samples each.  Not estimable: n < 2, or n above the lane
// count and not a multiple of it (the lanes would hold unequal counts).
static __device__ __forceinline__ bool lanes_estimable(int64_t n) { return n >= 2 && (n <= JADE_SAMPLE_LANES || n % JADE_SAMPLE_LANES == 0); }

// Lane l of owned pixel t*256 + i sits at floats (l * npx + t * 256 + i) * 3 .. + 2 (PathState.sum).  npx is a multiple of 256, so
// one (lane, tile) is 3 KB, contiguous and 16-B aligned: 192 16-B loads by the block, handed to each pixel's thread through LDS.
// One pass over the K lanes of the block's tile t, shifted by lane 0's value: the two-pass result without its second read, and no
// cancellation when the lanes agree.  Every thread of the block calls it (it synchronises; stage: the block's 12 KB of LDS); thread i gets pixel i's
//   y0 = Y_0,  sd = sum (Y_l - y0),  sdd = sum (Y_l - y0)^2,   Y_l = (0.3 S_l.r + 0.6 S_l.g + 0.1 S_l.b) / c
struct LaneMoments {
  double y0, sd, sdd;
};
static __device__ __forceinline__ LaneMoments lane_moments(const float* sum, int32_t npx, uint32_t t, int i, int K, double c, jade_err_v4f* stage) {
  double y0 = 0.0, sd = 0.0, sdd = 0.0;
  const jade_err_v4f* base = reinterpret_cast<const jade_err_v4f*>(sum + (size_t)t * 256 * 3);
  const size_t lane_step = (size_t)npx * 3 / 4;  // 16-B words per lane
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
  return LaneMoments{y0, sd, sdd};
}

// sum (Y_l - m)^2 from the moments: sdd - sd^2 / K, clamped at 0
static __device__ __forceinline__ double lane_sum_sq(double sd, double sdd, double kk) {
  double ss = sdd - sd * sd / kk;
  if (ss < 0.0) ss = 0.0;
  return ss;
}
