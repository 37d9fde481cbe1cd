/*
 * jade_bvh.h — device-side BVH construction.
 *
 * The reference builds its BVH on the host with a full-sweep SAH that sorts
 * every node's range three times (buildBVHwithSAH, PathTrace.cu:497-628):
 * 0.4 s for 70 k triangles, 8.3 s for 870 k in this repo's host pipeline.  That
 * builder stays the reference-faithful default (host/scene_build.cpp).  This
 * entry point builds a linear BVH on the GPU instead — Morton order, Karras'
 * binary radix tree, subtrees of <= leaf_size triangles collapsed into leaves —
 * and returns it in the SAME conventions the integrator consumes
 * (BVHNode_cu: node 0 dummy, root 1, child 0 = none, n > 0 marks a leaf over
 * triangles [index, index + n - 1] of the reordered array; PathTrace.cu:341-345,
 * 525-529, 804, 1557-1565), so everything downstream is unchanged.
 *
 * The traversal never prunes, so generic rays find the same closest hit in any
 * valid BVH (tests: 200 000 random rays, bit-identical).  CAVEAT: the reference's
 * triangle test has no epsilon, so a ray leaving a large coplanar face (the
 * mirror floor) "hits" the coplanar neighbour at ~1e-7 whenever that
 * neighbour's leaf is entered; the SAH tree happens to put such triangles in a
 * flat leaf box, which the "slab value > 0" rule (PathTrace.cu:770, 835-855)
 * skips, while another tree may not.  On scenes with big coplanar faces an
 * LBVH render therefore differs from the SAH render in part of the pixels.
 * Parity is defined per tree: the HIP integrator and the oracle agree exactly
 * (counters) on whichever tree both are given.  The work counters (nodes
 * visited / triangles tested) differ between trees, as the trees do.
 *
 * The header also holds the HIP module's other entry points that the CPU
 * oracle does not implement: adaptive sampling and its noise map, the
 * edge-aware denoiser, exposure with its luminance meter, glare, the
 * despeckle pass, the thin-lens camera and the camera shutter (below).
 * Exported by libjade_hip.so only; the oracle has none of them.
 */
#ifndef JADE_BVH_H
#define JADE_BVH_H

#include "jade_rt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* triangles: n records in ORIGINAL order (only p1, p2, p3 are read), host memory.
 * order_out[n]:   sorted position -> original index (the caller reorders its triangles with it)
 * nodes_out[max_nodes], *n_nodes_out: the tree; 2*n + 1 entries always suffice.  With fewer than the tree needs the call
 *                 returns JADE_ERR_INVALID and writes nothing.
 * build_ms (nullable): device time of the build kernels (sort included), without the copies
 * leaf_size: 1..15 (the reference uses 8)
 * JADE_ERR_INVALID: a null pointer (build_ms excepted), n <= 0, leaf_size outside 1..15, a non-finite vertex (below);
 * JADE_ERR_UNSUPPORTED: n >= 2^27; JADE_ERR_DEVICE: no device of that id.
 *
 * ---- The tree, stated ----
 * Both builders are deterministic, and what they build is fixed here completely enough to be built a second time, bit for
 * bit: tests/bvh_ref.py does so in numpy and tests/test_gpu_bvh_exact.py compares.  Every operation below is ONE float32
 * operation, correctly rounded, nothing contracted, denormals kept.
 *
 * [Centroid and keys]
 *   c      = ((p1 + p2) + p3) / 3                                 per axis
 *   cmin, cmax = the minimum and maximum of c over the triangles, per axis
 *   scale  = 1023.999f / (cmax - cmin) where cmax > cmin, else 0  (an axis without extent; a denormal extent gives +inf)
 *   q      = (c - cmin) * scale, clamped to [0, 1023] with a NaN (0 * inf, inf * 0) going to 0, then truncated to an integer
 *   code   = the three 10-bit values interleaved, x highest: bit k of qx at bit 3k + 2, of qy at 3k + 1, of qz at 3k
 *   key    = code << 32 | original index                          64 bits, unique; sorted ascending
 *   The box of a triangle is the minimum and maximum of its three vertices, the box of a node the union (min, max) of its
 *   children's: no arithmetic, so a box does not depend on the tree's shape above or below it.
 *
 * [LBVH]  The binary radix tree of the keys (Karras 2012).  A node over the key range [a, b], a < b, splits after the last
 *   key that shares with key[a] more leading bits than key[b] does; the lower keys are the left child.  Triangles with one
 *   code are split on the bits of their indices.
 *
 * [PLOC]  Clusters form a row, at first the triangles in key order.  One round:
 *   - Every cluster i looks at the positions j != i with |j - i| <= 16 inside the row and chooses the j with the least
 *     tuple (A, d, (low / d) & 1, low), compared lexicographically, where d = |j - i|, low = min(i, j), the division is the
 *     integers', and A = (x * y + y * z) + z * x in float32 of the extents x, y, z (maximum corner - minimum corner) of the
 *     union of the two boxes.  Equal areas are ties, +inf = +inf included; a NaN area (inf * 0: an extent that overflows
 *     beside a flat one) counts as +inf.  The tuple belongs to the PAIR and no two pairs share one, so the least pair of the
 *     row is always mutual: every round merges, whatever the areas.  The third member makes a row of equal areas pair up as
 *     (0, 1), (2, 3), ... instead of chaining.
 *   - Pairs that chose each other merge.  The lower position keeps its place in the row and is the LEFT child, the upper
 *     one leaves the row and is the right child; everyone else stays, in order.
 *   Rounds repeat until one cluster is left: the root.
 *
 * [Both builders]
 *   - A subtree of <= leaf_size triangles is ONE leaf (the topmost such subtree: nothing below it is emitted).
 *   - Triangle order (order_out): depth-first through the binary tree, left before right.  For the LBVH that is the key
 *     order.  A leaf's triangles are [index, index + n - 1] of it.
 *   - [Records] node 0 is the reference's dummy (left 255, right 128, n 30, index 0, aa (1, 1, 0), bb (0, 1, 0)), the root is
 *     node 1, a leaf has left = right = 0 and n > 0, an internal node n = index = 0 and both children > 0.  WHICH number a
 *     node gets beyond that is not part of the contract; two trees are the same if they agree walked together from node 1.
 *
 * [Non-finite input]  A triangle with a NaN or an infinite vertex coordinate is refused by both builders with
 *   JADE_ERR_INVALID, and jade_last_error names the first such triangle.  (A NaN box is nobody's nearest neighbour, and
 *   PLOC used to end with JADE_ERR_DEVICE "merged nothing" on it while the LBVH built a tree.)  Finite coordinates of any
 *   magnitude build: where (p1 + p2) + p3 overflows the centroid is +-inf and the rules above still give every q. */
int jade_bvh_build_lbvh(const jade_triangle* triangles, int32_t n, int32_t leaf_size, int device_id,
                        int32_t* order_out, jade_bvh_node* nodes_out, int32_t max_nodes,
                        int32_t* n_nodes_out, double* build_ms);

/* Same contract, better tree: PLOC (parallel locally-ordered clustering, Meister & Bittner 2018).  Clusters are merged
 * bottom-up by the surface area of their union, i.e. by the measure the reference's sweep-SAH builder minimises top-down
 * (PathTrace.cu:532-628) rather than by the Morton code's bits; subtrees of <= leaf_size triangles become leaves as in the
 * reference (:525-529).  Tens of rounds of four small kernels: milliseconds at 870 k triangles. */
int jade_bvh_build_ploc(const jade_triangle* triangles, int32_t n, int32_t leaf_size, int device_id,
                        int32_t* order_out, jade_bvh_node* nodes_out, int32_t max_nodes,
                        int32_t* n_nodes_out, double* build_ms);

/* ---- Adaptive sampling: each 16x16 tile stops once it has converged ----
 *
 * jade_render_adaptive renders the owned tiles of `params` (tile_rank / tile_nranks as jade_render) in rounds.
 * params->spp is the cap: no pixel gets more samples.  Round targets are T0 = min_spp, T(k+1) = min(2 Tk, spp);
 * min_spp is a power of two, 2 <= min_spp <= spp.  After every round with Tk < spp each still-active tile gets an
 * error, the MAXIMUM over its in-image pixels of the pixel error below; a tile whose error is <= rel_error stops at
 * Tk samples, the others go on.  The render ends when no tile is active or the cap has been rendered.
 * rel_error and error_floor must be finite and > 0.
 *
 * Pixel error of a pixel with n samples: K = min(n, 1024), c = n / K (lane l < K holds the sum S_l of c samples):
 *   Y_l = (0.3 S_l.r + 0.6 S_l.g + 0.1 S_l.b) / c        (the reference's luminance weights, PathTrace.cu:669-672)
 *   m   = (1/K) sum Y_l
 *   err = sqrt( sum (Y_l - m)^2 / (K (K - 1)) ) / (m + error_floor)
 * evaluated in fp64 and stored as float: the standard error of the pixel's mean luminance, relative to it.  It is
 * NaN where n cannot be estimated: n < 2, or n > 1024 and not a multiple of 1024.
 *
 * A tile stopped at k samples is bit for bit that tile of jade_render at spp = k (samples are independent work
 * items, jade_rt.h), and stats is the sum over tiles of what that render counts for the tile.
 *   out_rgb / out_bgr8  as jade_render, each tile divided by its own count
 *   out_tile_spp        nullable: one int32 per tile of the WHOLE grid, id ty * tiles_x + tx; tiles of other ranks: 0
 * After the call jade_render_resolve / _resolve_ex / _resolve_tiles_device divide each tile by its own count,
 * jade_render_step returns JADE_ERR_INVALID until the next jade_render_begin, and jade_render_error reads the
 * per-tile counts.  JADE_ERR_UNSUPPORTED with the pixel-rotation schedule (records move between pixels). */
int jade_render_adaptive(jade_scene* scene, const jade_render_params* params, int32_t min_spp, float rel_error,
                         float error_floor, float* out_rgb, uint8_t* out_bgr8, int32_t* out_tile_spp,
                         jade_stats* stats);

/* The noise map of the render in progress (after jade_render_begin + steps, or after jade_render_adaptive):
 * the pixel error above for every pixel of the owned tiles, width*height floats laid out as out_rgb's pixels
 * (pixel (x, y) at y*width + x); pixels of tiles not owned are left untouched.  Flushes first, like resolve.
 * Fails only when no render has been begun or no sample rendered. */
int jade_render_error(jade_scene* scene, float error_floor, float* out_error);

/* ---- Denoiser: an edge-aware a-trous filter guided by albedo, normal, depth and variance ----
 *
 * The spatial part of SVGF (Schied et al. 2017) over the a-trous wavelet filter of Dammertz et al. (2010).  Non-parity: the
 * reference has no denoiser.  Every image below is width*height pixels laid out as out_rgb's (pixel (x, y) at y*width + x).
 *
 * Guides of pixel (x, y), over guide samples s = 0 .. G-1: the camera ray of sample s exactly as the render makes it (seed
 * jade_rng_seed(x, y, frame + s), two jitter draws, origin = eye), walked with the reference walk (nearest hit, as
 * jade_trace_rays).  t = (1,1,1), z = 0.  While the hit triangle is a mirror (reflex_mode == JADE_MIRROR), not emissive (the
 * render's mirror test) and fewer than JADE_MAX_FULL_REFLEX_TIME mirror vertices have been passed: t *= brdf, z += hit
 * distance, and the ray goes on from the hit point in direction n (2 (o.n)) - o, o = -d.  At the final vertex k: z += hit
 * distance, a = t * brdf_k, n = norm_k negated if dot(norm_k, d) > 0.  A miss: a = t, n = 0, z = 0.  The guide of the pixel is
 * the float sum over s in increasing order times (float)(1/G); the normal is not renormalised.
 * The guides follow the lens: in a render begun under a lens (jade_scene_set_lens, below) guide sample s takes its origin and its
 * direction by "The lens, stated" - four draws instead of two - and everything after that is the statement above.  The guides then
 * have the blurred edges the frame has; pinhole guides would tell the filter to keep edges that are not there.
 * They follow the shutter in the same way: in a render begun under a shutter (jade_scene_set_shutter, below) guide sample s takes its
 * origin and direction by "The shutter, stated" - three draws, or five under a lens.
 *
 * Variance of pixel p: the variance of its mean luminance, the square of the pixel error's numerator above:
 *   v = sum (Y_l - m)^2 / (K (K - 1))       (Y_l, m, K as above; fp64, stored as float; NaN where n cannot be estimated)
 *
 * Filter, pass i = 0 .. iterations-1 with step s = 2^i, luminance l = 0.3 r + 0.6 g + 0.1 b, h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   g_p = the 3x3 blur of v with weights (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4) over in-image taps, renormalised
 *   for each in-image tap q = p + s (dx, dy), dx, dy in -2..2:
 *     w_l = exp(-|l_p - l_q| / (sigma_luminance sqrt(g_p) + 1e-10))
 *     w_n = 1 if both normals are 0, 0 if exactly one is, else max(0, nhat_p . nhat_q)^sigma_normal
 *     w_z = exp(-|z_p - z_q| / (sigma_depth max(z_p, z_q) + 1e-10))
 *     w_a = exp(-|a_p - a_q|_1 / sigma_albedo)
 *     w   = h(dx) h(dy) w_l w_n w_z w_a
 *   c'_p = sum w c_q / sum w          v'_p = sum w^2 v_q / (sum w)^2
 * iterations = 0 returns the input colour bit for bit.
 * The normal: nhat = n / |n| for every finite non-zero n, whatever its length (a normal whose squared length leaves the float range
 * is first scaled by a power of two); nhat = 0 for n = 0, which is what "the normal is 0" means in w_n.
 * Unusable pixels: a pixel is unusable if a channel of its c, a or n is non-finite, or its z is non-finite, or its v is non-finite
 * or negative.  This is decided once, from the inputs.  In every pass an unusable pixel keeps its c and v bit for bit, and it is no
 * tap of any other pixel: neither in the 5x5 sums nor in the 3x3 blur of v, which is renormalised over the in-image usable taps.
 * The centre tap of a usable pixel is usable, so no sum is empty.  So: finite inputs give a finite output; one non-finite pixel
 * stays one pixel, whatever the number of passes; a variance that is NaN everywhere (what jade_render_guides gives for a count that
 * cannot be estimated) returns the input colour bit for bit. */
typedef struct jade_denoise_params {
  int32_t iterations;    /* a-trous passes, 0..8; pass i uses a step of 2^i pixels; 0 = identity */
  int32_t guide_spp;     /* camera samples averaged into the guides, 1..64 */
  float sigma_luminance; /* > 0 */
  float sigma_normal;    /* >= 0, exponent */
  float sigma_depth;     /* > 0, relative */
  float sigma_albedo;    /* > 0 */
} jade_denoise_params;

/* The defaults DESIGN.md 3.6 chose from its measurement. */
void jade_denoise_defaults(jade_denoise_params* p);

/* The denoiser's inputs for the owned tiles of the render in progress (flushes first, like resolve).  Each output is
 * width*height floats (x3 for albedo and normal) in out_rgb's pixel layout; pixels of tiles this rank does not own are left
 * untouched.  Any output may be null.  guide_spp: 1..64.  The variance is NaN where the pixel's sample count cannot give
 * one, as jade_render_error's estimate is.  The render's sums, counters and next step are not changed. */
int jade_render_guides(jade_scene* scene, int32_t guide_spp, float* out_albedo, float* out_normal, float* out_depth,
                       float* out_variance);

/* Denoise the render in progress on its device: resolve, variance and guides, then the filter, all on the device, one copy
 * back.  Full frame only: tile_nranks > 1 gives JADE_ERR_UNSUPPORTED.  tonemap / limit as jade_render_resolve_ex.  Works
 * after jade_render_adaptive too, with each tile's own count.  JADE_ERR_INVALID where a pixel's count cannot give a
 * variance (n < 2, or n > 1024 and not a multiple of 1024).  Bit for bit jade_denoise_image on jade_render_resolve_ex's
 * out_rgb and jade_render_guides' outputs.  The render is not changed. */
int jade_render_denoise(jade_scene* scene, const jade_denoise_params* params, int tonemap, float limit, float* out_rgb,
                        uint8_t* out_bgr8);

/* The same filter on caller-provided host buffers (rgb and albedo / normal x3 floats per pixel).  This is what a multi-rank
 * host calls after it has gathered rgb (resolve) and the guides (jade_render_guides) of every rank. */
int jade_denoise_image(int device_id, int32_t width, int32_t height, const float* rgb, const float* variance,
                       const float* albedo, const float* normal, const float* depth, const jade_denoise_params* params,
                       float* out_rgb);

/* ---- Exposure: a luminance histogram of the frame, an exposure chosen from it, and the tone pack of the exposed frame ----
 *
 * Non-parity: the reference tone-maps the raw mean (PathTrace.cu:1457-1473), which is what jade_render_resolve_ex does and goes
 * on doing.  Here the linear mean m of a pixel is multiplied by one exposure e for the whole frame before the tone curve:
 *   bytes = the tone pack of jade_render_resolve_ex (ACES or Reinhard, gamma, BGR) applied to (e * m.r, e * m.g, e * m.b),
 *   each product one float multiplication.  out_rgb is never scaled.  e = 1 gives jade_render_resolve_ex's bytes.
 *
 * Luminance of a pixel with linear colour (r, g, b) - the Reinhard operator's statement (PathTrace.cu:669-672):
 *   Y = (float)(0.3 * (double)r + 0.6 * (double)g + 0.1 * (double)b)          (added from left to right)
 * Class of a pixel, decided in this order: non-finite (Y is a NaN or +-inf), negative (Y < 0), zero (Y == +-0), positive.
 * Bin of a positive Y, with u the 32 bits of the float Y:
 *   b = clamp((int)(u >> 20) - 760, 0, JADE_METER_BINS - 1)
 * i.e. the exponent and the top three bits of the mantissa: 8 bins per stop over the 64 stops [2^-32, 2^32), Y = 1.0f in bin 256.
 * Bin b, with E = (b >> 3) - 32 and k = b & 7, covers [2^E (1 + k/8), 2^E (1 + (k+1)/8)).  No logarithm is taken per pixel.
 * Subnormals and everything else below the range count in bin 0, everything above it (up to FLT_MAX) in bin 511.
 *
 * The histogram is integers, so it does not depend on the order in which pixels are counted, and it is additive: the meters of
 * the ranks of a tile partition, added field by field (minimum and maximum of lum_min / lum_max over the ranks with positive
 * pixels), are the meter of the frame.
 *
 * The exposure of a meter under AUTO (jade_meter_exposure; host code, double precision):
 *   N = sum of bins, lo = p_lo N, hi = p_hi N
 *   for b = 0 .. 511 in increasing order, C = sum of bins[j] over j < b:
 *     w_b = max(0, min(C + bins[b], hi) - max(C, lo))         the part of the bin's pixels inside the window of ranks [lo, hi]
 *     l_b = E + log2(1 + (2 k + 1) / 16)                      log2 of the bin's centre
 *   L = (sum w_b l_b) / (sum w_b), both summed in increasing b
 *   e = (float)(key * exp2(-L)), or 1.0f if sum w_b is 0; then clamped to [min_exposure, max_exposure]
 * With the window [0, 1] this is Reinhard's log-average key (Reinhard et al. 2002): the frame's geometric mean luminance goes to
 * `key`.  The window leaves out the darkest and the brightest pixels (a sun, black borders).  Under MANUAL e = exposure.
 * Of the parameters only those of the mode in use are checked. */
#define JADE_METER_BINS 512
typedef struct jade_meter {
  uint64_t bins[JADE_METER_BINS];
  uint64_t n_positive;     /* == sum of bins */
  uint64_t n_zero, n_negative, n_nonfinite;
  float lum_min, lum_max;  /* over the positive pixels, exact values; both 0 when n_positive == 0 */
} jade_meter;

#define JADE_EXPOSURE_MANUAL 0
#define JADE_EXPOSURE_AUTO 1
typedef struct jade_display_params {
  int32_t tonemap;                  /* JADE_TONEMAP_*, as jade_render_resolve_ex */
  float limit;                      /* ... and its Reinhard limit */
  int32_t exposure_mode;            /* JADE_EXPOSURE_* */
  float exposure;                   /* MANUAL: the multiplier; finite, > 0 */
  float key;                        /* AUTO: finite, > 0 */
  float p_lo, p_hi;                 /* AUTO: 0 <= p_lo < p_hi <= 1 */
  float min_exposure, max_exposure; /* AUTO: 0 < min_exposure <= max_exposure, finite */
} jade_display_params;

/* ACES, MANUAL with exposure 1, key 0.18, window [0.05, 0.95], clamp [2^-16, 2^16] (limit 1.5, used by Reinhard only). */
void jade_display_defaults(jade_display_params* p);

/* The exposure above.  Makes no HIP call: callable without a GPU.  `m` may be null under MANUAL.  Invalid parameters (a null
 * pointer, an unknown mode, a value outside the ranges above) return a NaN and set jade_last_error. */
float jade_meter_exposure(const jade_meter* m, const jade_display_params* p);

/* The meter of the render in progress (after jade_render_begin + steps, or after jade_render_adaptive, where each tile is
 * divided by its own count) over the in-image pixels of the owned tiles: the classes' counts add up to that number of pixels.
 * Flushes first, like resolve; fails as jade_render_resolve_ex does before begin or with no sample rendered.  The render's sums,
 * counters and next step are not changed. */
int jade_render_meter(jade_scene* scene, jade_meter* out);

/* Resolve with exposure.  out_rgb (nullable): the linear mean, NOT scaled - jade_render_resolve_ex's bit for bit.  out_bgr8
 * (nullable): the tone pack of e * mean as stated above, with e = jade_meter_exposure(this rank's own meter, params).
 * exposure_used, meter_out: nullable; the meter is taken under AUTO or when meter_out is given.  Pixels of tiles this rank does
 * not own are left untouched.  A tile partition that wants ONE exposure for the frame adds the ranks' meters
 * (jade_render_meter), calls jade_meter_exposure on the sum and resolves every rank under MANUAL with that value. */
int jade_render_resolve_exposed(jade_scene* scene, const jade_display_params* params, float* out_rgb, uint8_t* out_bgr8,
                                float* exposure_used, jade_meter* meter_out);

/* The same on a caller's host frame, width*height pixels in out_rgb's layout, every pixel counted: what exposes a denoised
 * frame (jade_render_denoise, jade_denoise_image) or the gathered frame of several ranks (jade_render_multi).  out_bgr8 is
 * nullable (meter only), as are exposure_used and meter_out. */
int jade_expose_image(int device_id, int32_t width, int32_t height, const float* rgb, const jade_display_params* params,
                      uint8_t* out_bgr8, float* exposure_used, jade_meter* meter_out);

/* ---- Glare: a light-conserving bloom pyramid ahead of the tone pack ----
 *
 * Non-parity: the reference has no glare.  A share s of every pixel's light is scattered over a pyramid of ever wider blurs and added
 * back, so that a pixel brighter than white shows as a halo instead of as flat white.  Linear and image-space: the render is not
 * changed.  Every image below is width*height pixels laid out as out_rgb's (pixel (x, y) at y*width + x).
 *
 * Source: L_0 = c, the linear frame; a pixel with any non-finite channel enters L_0 as (0, 0, 0).
 *
 * REDUCE, h = (1, 4, 6, 4, 1)/16, W_{k+1} = ceil(W_k / 2), H_{k+1} = ceil(H_k / 2) (a 1x1 level stays 1x1):
 *   L_{k+1}(x, y) = sum over i, j = -2..2 of h(i) h(j) L_k(clamp(2x + i), clamp(2y + j))
 * with the coordinates clamped to the level (the border is replicated: a constant frame does not darken at its edges).  Separable:
 * rows first (x), then columns (y); each 1-D sum is added in increasing i.
 *
 * EXPAND to a finer level of n columns from m, per axis, source indices clamped to [0, m-1]:
 *   even x = 2j:     (1/8) a(j-1) + (3/4) a(j) + (1/8) a(j+1)        (added from left to right)
 *   odd  x = 2j + 1: (1/2) a(j) + (1/2) a(j+1)
 * Rows (y) first, then columns (x).  Both operators keep a constant, and away from the borders both keep the sum of the frame: a
 * source pixel gives 1/2 per axis to the coarser level, and EXPAND gives it back.
 *
 * Weights: w_k = f^(k-1) / sum over j = 1..levels of f^(j-1), computed in double on the host and passed on as float; for f > 1
 * every power is taken relative to the largest, f^(k-levels) over the sum of those (added in increasing k), so that none overflows.
 *
 * Accumulation, from the top down:
 *   A_levels = w_levels L_levels
 *   A_k      = w_k L_k + EXPAND(A_{k+1})          k = levels-1 .. 1
 *   B        = EXPAND(A_1)                        at frame size
 * Output: out = (1 - s) L_0 + s B, with (1 - s) one float subtraction and each product and the sum one float operation.  A pixel
 * that was non-finite in c is written back as its input, bit for bit.  strength == 0 returns the input bit for bit (-0.0 and NaN
 * payloads included) without running the pyramid, as iterations = 0 does in the denoiser.
 *
 * The defaults are a look, not a measurement: see DESIGN.md 3.8. */
typedef struct jade_glare_params {
  int32_t levels;   /* 1..12 pyramid levels */
  float strength;   /* s in [0, 1]: the share of every pixel's light that is scattered */
  float falloff;    /* f, finite and > 0: level k (1-based) weighs f^(k-1), normalised over the levels */
} jade_glare_params;

/* levels 6, strength 0.1, falloff 0.5. */
void jade_glare_defaults(jade_glare_params* p);

/* Glare of a caller's host frame on device `device_id`.  out_rgb == rgb is allowed.  A null pointer, a bad size (as
 * jade_denoise_image; also a height above 1048560 = 16 * 65535 rows, which the kernels' grids do not hold) or a parameter outside
 * its range or non-finite returns JADE_ERR_INVALID before any HIP call; device_id is checked as jade_denoise_image checks it.
 * This is what glares a denoised frame (jade_render_denoise -> jade_glare_image -> jade_expose_image) or the gathered frame of
 * several ranks. */
int jade_glare_image(int device_id, int32_t width, int32_t height, const float* rgb, const jade_glare_params* params,
                     float* out_rgb);

/* Glare the render in progress on its device, one copy back: flush (as resolve), resolve (after jade_render_adaptive with each
 * tile's own count), the pyramid, the meter of the glared frame under AUTO, jade_meter_exposure, the tone pack of e x glared colour.
 * display may be null: jade_display_defaults.  out_rgb (nullable): the glared linear frame, NOT scaled by e - bit for bit
 * jade_glare_image of jade_render_resolve_ex's out_rgb.  out_bgr8, exposure_used (nullable): bit for bit jade_expose_image of that
 * glared frame under `display`.  Full frame only: tile_nranks > 1 gives JADE_ERR_UNSUPPORTED (gather, then jade_glare_image).
 * Fails as jade_render_resolve_ex does before begin or with no sample rendered.  The render's sums, counters and next step are
 * not changed. */
int jade_render_glare(jade_scene* scene, const jade_glare_params* params, const jade_display_params* display,
                      float* out_rgb, uint8_t* out_bgr8, float* exposure_used);

/* ---- Despeckle, stated: clamp the firefly pixels that the variance does not back ----
 *
 * Non-parity: the reference has no such pass.  Image-space, on the resolved linear frame, ahead of the denoiser; the render is not
 * changed.  A pixel whose luminance stands above g times the K-th brightest of its neighbours is scaled down to that bound, unless the
 * variance of its mean says that the excess is real: an excess carried by k of a pixel's samples stands about sqrt(k) standard errors
 * above the neighbourhood, so "established at z sigmas" reads "at least about z^2 samples back it".  A lamp seen directly is kept, a
 * highlight that a quarter of the samples hit is kept, one huge sample among 64 is kept by nothing.
 *
 * Everything is float32; every operation written below is ONE float operation, nothing is contracted, and the division is the
 * correctly rounded one.
 *
 * Inputs: a frame c of W x H pixels in out_rgb's layout (pixel (x, y) at y*W + x); optionally v, W x H floats, the variance of each
 * pixel's mean luminance as jade_render_guides gives it; the parameters iterations (0..4), radius R (1..3), rank K (1..4), gain g
 * (finite, >= 1), floor f (finite, >= 0) and sigmas z (finite, >= 0).  zz = z * z, one float multiplication on the host.
 *
 * One pass.  Every decision is taken from the pass's INPUT, never from pixels already written:
 *   Y(p) = (0.3f * r + 0.6f * g) + 0.1f * b          the denoiser's luminance, whose weights are the weights of v
 *   p is usable if its three channels and Y(p) are finite.  An unusable pixel keeps its c and v bit for bit and is nobody's neighbour.
 *   N(p) = the usable pixels q != p with |dx| <= R and |dy| <= R inside the image; nothing is replicated at the border.
 *          If N(p) has fewer than K pixels, p is unchanged.
 *   B = the K-th largest Y over N(p); ties count as separate entries
 *   C = g * max(B, 0.0f) + f                          max(B, 0.0f) is B where B > 0 and +0.0f otherwise
 *   if not Y(p) > C, p is unchanged.  Otherwise p is ABOVE.
 *   p is ESTABLISHED if v is given, v(p) is finite and >= 0, and with d = Y(p) - C the test d * d > zz * v(p) holds - taken as
 *   written, whatever under- or overflow it has.  An established pixel is unchanged.
 *   Otherwise p is CLAMPED:  k = C / Y(p);  c'(p) = (k r, k g, k b);  v'(p) = (k * k) * v(p) where v is given;
 *                            scale(p) = scale(p) * k, and scale starts at 1.0f.
 * `iterations` passes run one after another, each on the previous pass's c and v.  iterations = 0 returns c (and v) bit for bit - -0.0
 * and NaN payloads included - and runs no kernel, as strength = 0 does in the glare.
 * 0 <= k < 1, so a clamped pixel never gains light and a finite frame stays finite.
 *
 * The report is all integers, so it does not depend on the order in which pixels are counted, and the reports of several frames add:
 * n_usable is taken from the input frame; n_above, n_established and n_clamped are each summed over the passes; always
 * n_above == n_established + n_clamped.  No floating-point atomic anywhere: every output word has one writer.
 *
 * The defaults come from the measurement in DESIGN.md 3.23. */
typedef struct jade_despeckle_params {
  int32_t iterations; /* passes, 0..4; 0 = identity */
  int32_t radius;     /* R, 1..3: the neighbourhood is (2R + 1)^2 - 1 pixels */
  int32_t rank;       /* K, 1..4: the K-th brightest neighbour sets the bound (K - 1 neighbouring speckles are seen through) */
  float gain;         /* g, finite, >= 1 */
  float floor;        /* f, finite, >= 0 */
  float sigmas;       /* z, finite, >= 0: the standard errors by which an excess must stand above the bound to be kept */
} jade_despeckle_params; /* 24 B */

typedef struct jade_despeckle_report {
  uint64_t n_usable, n_above, n_established, n_clamped;
} jade_despeckle_report;

/* 1 iteration, radius 1, rank 2, gain 2, floor 0, sigmas 2. */
void jade_despeckle_defaults(jade_despeckle_params* p);

/* The passes on a caller's host frame on device `device_id`.  variance (nullable): without it nothing is established.  out_variance
 * (nullable) needs variance.  out_scale (nullable): W x H floats, the product of every k a pixel was clamped by, 1.0f elsewhere.
 * out_rgb == rgb and out_variance == variance are allowed.  A null rgb, out_rgb or params, a bad size (as jade_denoise_image; also a
 * height above 524280 = 8 * 65535 rows, which the kernel's grid does not hold), out_variance without variance, or a parameter outside
 * its range or non-finite returns JADE_ERR_INVALID before any HIP call; device_id is checked as jade_denoise_image checks it.  This is
 * what despeckles the gathered frame of several ranks: gather rgb (resolve) and jade_render_guides' variance, then this, then
 * jade_denoise_image; the ranks' reports add. */
int jade_despeckle_image(int device_id, int32_t width, int32_t height, const float* rgb, const float* variance,
                         const jade_despeckle_params* params, float* out_rgb, float* out_variance, float* out_scale,
                         jade_despeckle_report* report);

/* Despeckle the render in progress on its device, one copy back: flush (as resolve), resolve (after jade_render_adaptive with each
 * tile's own count), the variance, the passes; with denoise parameters the guides and the a-trous filter on the despeckled colour and
 * variance; the tone pack (tonemap / limit as jade_render_resolve_ex).  out_rgb, out_bgr8, out_scale and report are nullable.
 * denoise == null: out_rgb is bit for bit jade_despeckle_image on jade_render_resolve_ex's out_rgb and jade_render_guides' variance.
 *   A sample count that gives no variance (NaN: n < 2, or n > 1024 and not a multiple of 1024) is no refusal here: it simply
 *   establishes nothing, and every pixel above is clamped.
 * denoise != null: out_rgb is bit for bit jade_denoise_image on that result's rgb and variance and jade_render_guides' other outputs,
 *   and the call refuses what jade_render_denoise refuses (such a sample count included).
 * Full frame only: tile_nranks > 1 gives JADE_ERR_UNSUPPORTED (gather, then jade_despeckle_image).  Fails as jade_render_resolve_ex
 * does before begin or with no sample rendered.  The render's sums, counters and next step are not changed. */
int jade_render_despeckle(jade_scene* scene, const jade_despeckle_params* params, const jade_denoise_params* denoise, int tonemap,
                          float limit, float* out_rgb, uint8_t* out_bgr8, float* out_scale, jade_despeckle_report* report);

/* ---- Thin lens: depth of field ----
 *
 * Non-parity: the reference's camera is a pinhole (PathTrace.cu:1428-1437).  The lens is a property of the scene handle, read by the
 * next jade_render_begin - so by whatever begins a render: jade_render, jade_render_adaptive, jade_render_multi (per scene) - and a
 * render in progress keeps the lens it began with.  With no lens, or aperture_radius == 0, every kernel, schedule, bit and counter is
 * the pinhole's; the mode is entered only for aperture_radius > 0.  It is another estimator of another image: none of jade_rt.h's
 * parity statements apply to it, as for JADE_ENV_IMPORTANCE.  It composes with JADE_ENV_IMPORTANCE, adaptive sampling, the denoiser,
 * exposure and glare.
 *
 * ---- The lens, stated ----
 * tests/lens_spec.py is this text in float64.  Every operation below is ONE float32 operation, nothing contracted; jade_transform,
 * normalize and jade_sincosf are include/jade_fpmath.h's routines.  A = aperture_radius, a disk in the camera's plane z = 0, in the
 * units of the scene; the plane of focus is camera-space z = -focus_distance.
 *
 * For sample s of pixel (x, y) the stream is seeded as jade_rt.h says.  u1, u2 are the two jitter draws and give left_offset and
 * up_offset by the pinhole's statements, unchanged.  Then two more draws u3, u4, in this order, BEFORE any draw of the path:
 *   r   = A * sqrt(u3)
 *   phi = fl(2 PI) * u4                      PI = 3.1415926 as everywhere; (sn, cs) = jade_sincosf(phi)
 *   lx  = r * cs,  ly = r * sn               the lens point (lx, ly, 0) in camera space: uniform over the disk
 *   k   = focus_distance / 1.5f              one float division, on the host, once per render
 *   d_c = (left_offset * k - lx, up_offset * k - ly, -1.5f * k)
 *   dir    = normalize(jade_transform(d_c, 0, camera))
 *   origin = eye + jade_transform((lx, ly, 0), 0, camera)         three float additions
 * The pinhole ray of the same jitter and every lens ray of it meet in the plane of focus, at (left_offset, up_offset, -1.5) * k.  A
 * point at camera depth z shows as a disk of radius 0.75 * height * A * |1/z - 1/focus_distance| pixels.  Every later draw of the
 * sample sits two places further on in the stream than the pinhole's.  jade_stats.rays_primary still counts one query per sample.
 *
 * The schedule under a lens is the list schedule (the first pass is shaded and traced by separate kernels): there is
 * no fused first pass yet, so rays_inline and tail_launches are 0.  Results do not depend on steps, tile partitions or records per
 * pixel, as for the pinhole.
 *
 * jade_scene_set_lens: lens == null, or aperture_radius == 0: the pinhole.  aperture_radius must be finite and >= 0; focus_distance
 * must be finite and > 0 whenever aperture_radius > 0 and is not checked otherwise (of the parameters only those in use are checked,
 * as for exposure).  JADE_ERR_INVALID leaves the previous lens in place.
 * jade_render_multi: all scenes must carry the same lens, bit for bit, else JADE_ERR_INVALID before anything is launched. */
typedef struct jade_lens_params {
  float aperture_radius; /* A >= 0, scene units; 0 = the pinhole */
  float focus_distance;  /* > 0: depth of the plane of focus along the camera's axis */
} jade_lens_params;

int jade_scene_set_lens(jade_scene* scene, const jade_lens_params* lens);
int jade_scene_get_lens(jade_scene* scene, jade_lens_params* out);

/* ---- Camera shutter: motion blur between two camera poses ----
 *
 * Non-parity, like the lens: the reference renders an instant.  The shutter is a property of the scene handle, read by the next
 * jade_render_begin - so by jade_render, jade_render_adaptive, jade_render_multi (per scene) - and a render in progress keeps the
 * shutter it began with.  The shutter opens at the pose of jade_render_params (eye, camera) and closes at (eye_close, camera_close);
 * every sample draws a time of its own within the exposure and is traced from the pose at that time.  With no shutter every kernel,
 * schedule, bit and counter is today's, for the pinhole and under a lens alike.  The mode is entered whenever a shutter is set, even one
 * whose two poses are equal.  It composes with the lens (depth of field and motion blur together, as a camera gives them), with
 * JADE_ENV_IMPORTANCE, adaptive sampling, the denoiser (the guides follow the shutter as they follow the lens), exposure and glare.
 * Only the camera moves: the scene is the same at every time.
 *
 * ---- The shutter, stated ----
 * tests/shutter_spec.py is this text in float64.  Every operation below is ONE float32 operation, nothing contracted.
 *
 * For sample s of pixel (x, y) the stream is seeded as jade_rt.h says.  u1, u2 are the two jitter draws and give left_offset and
 * up_offset by the pinhole's statements, unchanged.  Under a lens (aperture_radius > 0) u3 and u4 follow, as "The lens, stated" says.
 * Then ONE more draw ut, BEFORE any draw of the path.
 * On the host, once per render, one float subtraction each:
 *   t_span = t_close - t_open
 *   de[i]  = eye_close[i] - eye[i]                   i = 0, 1, 2
 *   dc[j]  = camera_close[j] - camera[j]             for the nine entries jade_transform(v, 0, .) multiplies by v: j = 0, 1, 2, 4, 5, 6, 8, 9, 10
 * Per sample:
 *   t        = t_open + ut * t_span                  a multiplication, then an addition
 *   eye_t[i] = eye[i] + t * de[i]                    a multiplication, then an addition
 *   cam_t[j] = camera[j] + t * dc[j]                 a multiplication, then an addition; every other entry of cam_t is camera's
 *   no lens:  dir = normalize(jade_transform((left_offset, up_offset, -1.5f), 0, cam_t));  origin = eye_t
 *   lens:     the statements of "The lens, stated" from r to origin, with cam_t and eye_t in place of camera and eye
 * Every later draw of the sample sits one place further on in the stream than without a shutter: the path's first draw is the
 * fourth of the stream without a lens and the sixth with one.  jade_stats.rays_primary still counts one query per sample.
 *
 * A property of the mode: the matrix is interpolated entry by entry, not as a rotation.  Between two poses that differ by a rotation
 * by theta about an axis, the matrix at mid-exposure is the rotation by theta / 2 shrunk by cos(theta / 2) across that axis (along
 * the axis nothing changes): a direction is normalised afterwards, so what remains is a view compressed by that factor across
 * the axis - 0.4 % at 10 degrees, 3.4 % at 30 - and a sweep that is uniform in the chord, not in the angle.  Keep theta small: a few
 * degrees per exposure.  It is a recommendation and is not checked; a longer move is several exposures, each a render of its own
 * with its own two poses.  With a lens, the aperture disk lies in the plane the interpolated matrix spans and is shrunk with it.
 *
 * The schedule is the lens's list schedule: no fused first pass, no tail kernel; rays_inline and tail_launches
 * are 0.  Results do not depend on steps, tile partitions or records per pixel.
 *
 * jade_scene_set_shutter: shutter == null: no shutter.  All 19 pose floats must be finite; t_open and t_close must be finite with
 * 0 <= t_open <= t_close <= 1 (t_open == t_close: every sample at that one time).  JADE_ERR_INVALID leaves the previous shutter in
 * place.  jade_scene_get_shutter: *is_set = 1 and *out = the shutter as set, or *is_set = 0 and *out zeroed; either may be null.
 * jade_render_multi: all scenes must carry the same shutter, bit for bit, or none, else JADE_ERR_INVALID before anything is launched. */
typedef struct jade_shutter_params {
  float eye_close[3];      /* the eye when the shutter closes; it opens at jade_render_params.eye */
  float camera_close[16];  /* the camera matrix when it closes; same layout as jade_render_params' */
  float t_open, t_close;   /* 0 <= t_open <= t_close <= 1: the part of the move the exposure covers */
} jade_shutter_params;

int jade_scene_set_shutter(jade_scene* scene, const jade_shutter_params* shutter);
int jade_scene_get_shutter(jade_scene* scene, jade_shutter_params* out, int* is_set);

/* ---- One-light sampling: one emitter per vertex, drawn by power ----
 *
 * Non-parity: the reference sends one shadow ray to EVERY entry of emit_indices at every diffuse, SSS-diffuse and BSSRDF vertex
 * (PathTrace.cu:945-, 1085-, 1281-), so rays, random draws and the size of a path record all grow with the emitter count.  Under
 * JADE_LIGHTS_ONE such a vertex draws ONE entry, with probability proportional to area x luminance of emission plus a floor, traces
 * that entry's shadow ray as the reference traces it and divides its term by the probability: another estimator of the SAME integral,
 * not the reference's sample for sample - none of jade_rt.h's parity statements apply to it, as for JADE_ENV_IMPORTANCE.  A path record
 * then has min(n_emit, 1) + 2 ray slots whatever n_emit is, so the records per pixel (JADE_Q_RECORDS_PER_PIXEL) and the largest frame
 * that fits no longer depend on the emitter count.  The mode is a property of the scene handle, read by the next jade_render_begin - so
 * by jade_render, jade_render_adaptive, jade_render_multi (per scene) - and a render in progress keeps the mode it began with.
 * JADE_LIGHTS_ALL (0, the default) is today's render in every kernel, bit and counter.  JADE_LIGHTS_ONE composes with both env_sampling
 * values, the three walks, tile partitions, progressive steps, adaptive sampling, the guides and the denoiser, exposure and glare.
 *
 * ---- The lights, stated ----
 * tests/lights_spec.py is this text in float64 for the draw itself, and the light_sampling arm of tests/jade_spec.py for what the
 * integrator does with a draw (where the four uniforms sit in each branch's stream, the entry's term and its weight, what follows).
 * nE = n_emit; entry i names triangle t_i = emit_indices[i].  Duplicates are separate
 * entries, and an entry whose triangle does not emit is still an entry.  fl() rounds to fp32.
 *
 * The distribution.  a_i = the area the integrator itself multiplies the entry's term by - 0.5f * sqrt(dot(c, c)) with c = cross(p2 - p1,
 * p3 - p1), every operation one fp32 operation (tri_size, PathTrace.cu:897-903) - and 0 where that is not finite;
 * l_i = 0.2126 max(er, 0) + 0.7152 max(eg, 0) + 0.0722 max(eb, 0) of t_i's emission, and 0 where that is not finite (a NaN or an
 * infinite channel); w_i = a_i * l_i, and 0 where that is not finite; floor = 0.01 * (sum of w) / nE, or 1 if the sum is 0;
 *     p_i = (w_i + floor) / (sum over j of (w_j + floor)),     q_i = p_i * nE     (mean 1, every p_i > 0).
 * l, w, floor, p and q are formed in double.  The table (made once, at jade_scene_create, by the builder of JADE_ENV_IMPORTANCE's table)
 * has nE entries {accept, alias, q_own, q_alias}: a draw that lands in slot s takes entry s with probability accept_s and entry alias_s
 * otherwise (alias_s < nE; 0 <= accept_s <= 1, and alias_s = s where accept_s = 1), such that entry i is drawn with probability
 * P_i = (accept_i + sum over s != i with alias_s = i of (1 - accept_s)) / nE = p_i up to the fp32 rounding of accept:
 * |P_i - p_i| <= (1 + m_i) * 2^-24 / nE with m_i the number of slots whose alias is i.  q_own = fl(q_s) and q_alias = fl(q_{alias_s}):
 * the probability the weight below divides by is the INTENDED one, p.  Which small entry is paired with which large one is not part
 * of this statement.
 *
 * The draw.  Where the reference draws (rand_x, rand_y) for entry 0 (PathTrace.cu:945-, 1085-, 1281-) this mode draws FOUR uniforms
 * u1..u4 from the sample's stream, in this order, and nothing for the other entries - each is jade_rand's fl(uint32) * 2^-32, in
 * [0, 1], 1.0f included:
 *     slot    s = min((uint32)fl(u1 * fl(nE)), nE - 1)                  (the product in fp32: a discrete decision)
 *     own     iff u2 < accept_s;      i = own ? s : alias_s,   q = own ? q_own_s : q_alias_s
 *     (rx, ry) = (u3, u4), folded as the reference folds them: if rx + ry > 1 then rx = 1 - rx, ry = 1 - ry
 *     weight  = fl(fl(nE) / q)                                          (= 1 / p_i up to rounding)
 * Everything the reference then does for entry i is done for this ONE entry: the point p1 + (p2 - p1) rx + (p3 - p1) ry on t_i; in the
 * diffuse and SSS-diffuse branch the side test dot(point - vertex, n) * dot(out, n) < 0 and its `continue` (no ray; the four uniforms
 * stay drawn, every later draw of the sample is where it would be); the shadow ray and its early-exit limit; the hit test
 * "hitBVH's triangle == t_i"; the entry's term, statement for statement.  The term is multiplied by weight, one fp32 multiplication
 * per channel, before it is added to l_dir.  nE = 0 draws nothing and traces nothing: the render is JADE_LIGHTS_ALL's in every bit
 * and counter.  Nothing else of the sample changes: the environment ray (either env_sampling), the roulette and the indirect ray
 * follow as they do in the reference, behind four draws where the reference has made 2 nE.
 * The estimator is unbiased because every p_i > 0: E[weight * term_i] = sum over i of p_i * term_i / p_i, the reference's sum.
 * jade_stats.rays_shadow counts at most one shadow ray per sampling vertex.
 *
 * The schedule is JADE_ENV_IMPORTANCE's: the fused first pass stays (it samples no emitter), there is no tail kernel
 * (tail_launches is 0) and JADE_SHADE_BINNED is ignored.  Results do not depend on steps, tile partitions or records per pixel.
 *
 * jade_scene_set_light_sampling: an unknown mode returns JADE_ERR_INVALID and leaves the previous mode in place.
 * jade_render_begin refuses JADE_LIGHTS_ONE with JADE_ERR_UNSUPPORTED on a scene with more than JADE_LIGHTS_ONE_MAX_ENTRIES emitter
 * entries (the slot is formed from a 24-bit uniform and reaches every slot only up to 2^24), and together with a lens
 * (jade_scene_set_lens, aperture_radius > 0) or a shutter (jade_scene_set_shutter): those kernels do not exist yet.
 * jade_render_multi: all scenes must carry the same mode, else JADE_ERR_INVALID before anything is launched. */
#define JADE_LIGHTS_ALL 0
#define JADE_LIGHTS_ONE 1
#define JADE_LIGHTS_ONE_MAX_ENTRIES 16777216 /* 2^24 */

int jade_scene_set_light_sampling(jade_scene* scene, int mode);
int jade_scene_get_light_sampling(jade_scene* scene, int* mode);

/* ---- Cosine-weighted bounce sampling ----
 *
 * Non-parity: at every diffuse, SSS-diffuse and BSSRDF vertex the reference draws its environment ray and its indirect ray uniformly on
 * the sphere, flips them into a hemisphere (pdf 1 / 2 pi) and weighs them with a bare |dot(n, d)| (PathTrace.cu:968-974, 992-998,
 * 1111-1117, 1136-1142, 1304-1310, 1328-1334).  Under JADE_BOUNCE_COSINE those two rays are drawn with pdf cos / pi about the normal
 * instead, and the cosine leaves the weight: another estimator of the SAME integral, not the reference's sample for sample - none of
 * jade_rt.h's parity statements apply to it, as for JADE_ENV_IMPORTANCE and JADE_LIGHTS_ONE.  The rays per vertex, the number of draws
 * and their places in the sample's stream, and the layout of a path record are the reference's.  The mode is a property of the scene
 * handle, read by the next jade_render_begin - so by jade_render, jade_render_adaptive, jade_render_multi (per scene) - and a render in
 * progress keeps the mode it began with.  JADE_BOUNCE_UNIFORM (0, the default) is today's render in every kernel, bit and counter.
 * JADE_BOUNCE_COSINE composes with both env_sampling values (under JADE_ENV_IMPORTANCE the environment ray stays the importance draw
 * with its own weight, and only the indirect ray changes), both light samplings, the three walks, tile partitions, progressive steps,
 * adaptive sampling, the guides and the denoiser, exposure and glare.
 *
 * ---- The bounce, stated ----
 * tests/bounce_spec.py is this text in float64.  fl() rounds to fp32; every operation below is one fp32 operation unless it says double.
 * Where the reference's sphere direction takes two uniforms from the sample's stream (cosine first, angle second) this mode takes the
 * same two, u1 then u2 - each jade_rand's fl(uint32) * 2^-32, in [0, 1], 1.0f included.
 *
 * Axis.  n is the normal the branch already uses - the vertex's flat normal at a diffuse or SSS-diffuse vertex, the exit triangle's
 * (t_norm) at a BSSRDF vertex - as stored, of any length.  nn = dot(n, n) = fma(n.z, n.z, fma(n.y, n.y, n.x * n.x)).
 *   If !(nn > 0 && nn < inf) the vertex FALLS BACK: the direction is the reference's sphere direction on the same two uniforms
 *   (cos = fl(2 (double(u1) - 0.5)), sin = sqrt(1 - cos * cos), phi as below, d = (sin * cos phi, sin * sin phi, cos)) with the
 *   reference's own flip, and every weight is the reference's.
 *   Otherwise a = s * (n / sqrt(nn)), the division per component, with s = -1 where the reference would flip a direction along +n and +1
 *   elsewhere: diffuse / SSS-diffuse, both rays: s = -1 iff side < 0 (side = dot(out, n));  BSSRDF environment ray: s = -1 iff
 *   dot(inner, t_norm) < 0;  BSSRDF indirect ray: s = -1 iff dot(inner, t_norm) > 0 - the OPPOSITE hemisphere, as the reference has it.
 * Frame (branchless; Duff, Burgess, Christensen, Hery, Kensler, Liani, Villemin: Building an Orthonormal Basis, Revisited, JCGT 2017):
 *     sg = a.z >= 0 ? 1 : -1        (-0 counts as >= 0)
 *     p  = -1 / (sg + a.z)
 *     q  = (a.x * a.y) * p
 *     t  = (1 + ((sg * a.x) * a.x) * p,   sg * q,                -sg * a.x)
 *     b  = (q,                            sg + (a.y * a.y) * p,  -a.y)
 * Direction.  r = sqrt(u1), cz = sqrt(1 - u1);  phi = fl(2 pi * double(u2)), the product in double, as the reference forms it;
 * (sn, cs) = jade_sincosf(phi);
 *     d = (t * (r * cs) + b * (r * sn)) + a * cz          (per component: three products, two sums, in this order)
 * so that dot(d, a) = cz up to rounding: pdf(d) = cz / pi.
 * Weight.  Against the reference's pdf 1 / 2 pi its term is multiplied by 1 / (2 cz), and |dot(n, d)| / (2 cz) = sqrt(nn) / 2: the
 * module uses that closed form.  In the four places where the reference multiplies by |dot(n, d)| - the environment term and the
 * indirect rate of the diffuse / SSS-diffuse branch, the environment term and the indirect rate of the BSSRDF branch (there with t_norm)
 * - this mode multiplies by 0.5f * sqrt(nn) instead, unless the vertex falls back (the predicate is formed again from the same normal),
 * and changes nothing else of the statement: Schlick's term of |dot(d, t_norm)| is part of the integrand and stays.  Nothing travels
 * with the record.  There is no division by cz, so u1 = 1.0f - a direction in the tangent plane - carries a finite weight.
 * Under JADE_ENV_IMPORTANCE the environment ray and its term are that mode's, unchanged; the indirect ray is this mode's.
 * The estimator is unbiased because pdf > 0 wherever the integrand's cosine is: E[f / pdf] over the hemisphere is the reference's.
 * jade_stats: every counter keeps its meaning; nodes_visited and tris_tested differ because the rays do.
 *
 * The schedule is JADE_ENV_IMPORTANCE's: the fused first pass stays (it draws no hemisphere direction), there is no tail
 * kernel (tail_launches is 0) and JADE_SHADE_BINNED is ignored.  Results do not depend on steps, tile partitions or records per pixel.
 *
 * jade_scene_set_bounce_sampling: an unknown mode returns JADE_ERR_INVALID and leaves the previous mode in place.
 * jade_render_begin refuses JADE_BOUNCE_COSINE with JADE_ERR_UNSUPPORTED together with a lens (jade_scene_set_lens, aperture_radius > 0)
 * or a shutter (jade_scene_set_shutter): those kernels do not exist yet.
 * jade_render_multi: all scenes must carry the same mode, else JADE_ERR_INVALID before anything is launched. */
#define JADE_BOUNCE_UNIFORM 0
#define JADE_BOUNCE_COSINE 1

int jade_scene_set_bounce_sampling(jade_scene* scene, int mode);
int jade_scene_get_bounce_sampling(jade_scene* scene, int* mode);

/* ---- Multiple importance sampling of the emitters ----
 *
 * Non-parity, on top of JADE_BOUNCE_COSINE: the emitter term of a diffuse or SSS-diffuse vertex, Le f |n.l| |ne.l| / (l.l)^2 A, has no
 * bound as the vertex approaches the emitter, and an indirect ray that lands on an emitter is thrown away (the path ends with nothing
 * when the hit is not `nonemissive`).  Under JADE_DIRECT_MIS the emitter rays and the indirect ray are two techniques for the SAME
 * integral over the emitters listed in emit_indices, combined with the balance heuristic: every emitter term is multiplied by a weight
 * in [0, 1], and an indirect ray that lands on a listed emitter adds that emitter's light with the complementary weight.  Every weighted
 * emitter term is then at most pi f Le |n| |ne| mu (below).  It costs no ray, no draw and no word of a path record: rays, draws, their
 * places in the sample's stream, the record layout, path lengths and EVERY jade_stats counter are JADE_BOUNCE_COSINE's; only radiance
 * changes.  None of jade_rt.h's parity statements apply.  The mode is a property of the scene handle, read by the next
 * jade_render_begin, and a render in progress keeps the mode it began with.  JADE_DIRECT_RAYS (0, the default) is today's render in every
 * kernel, bit and counter.  It composes with what JADE_BOUNCE_COSINE composes with: both env_sampling values, both light samplings, the
 * three walks, tile partitions, progressive steps, adaptive sampling, the guides and the denoiser, exposure and glare.
 *
 * ---- The direct light, stated ----
 * tests/mis_spec.py is this text in float64.  fl() rounds to fp32; every operation below is one fp32 operation unless it says double;
 * dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)).  It applies at diffuse and SSS-diffuse vertices only.  A BSSRDF vertex is
 * JADE_BOUNCE_COSINE's, unchanged: its emitter rays have no side test and its indirect ray takes the opposite hemisphere, so the two
 * techniques do not sample one domain there.
 *
 * The table (made once, at jade_scene_create, on the host): two numbers (m, M) per triangle h.  h is WEIGHTED iff it fails the
 * reference's indirect-hit test `nonemissive` (not all three channels of its emission < 1.5e-4f - so a NaN channel counts), its area
 * A = tri_size(h) (0.5f * sqrt(dot(c, c)), c = cross(p2 - p1, p3 - p1), PathTrace.cu:897-903) is finite and > 0, and nne = dot(ne, ne) of
 * its stored normal ne is finite and > 0.  For a weighted h, m(h) = fl(the number of entries of emit_indices that name h) and
 * M(h) = fl((sum over those entries i, in list order, of double(q_own_i)) / double(nE)), the probability with which JADE_LIGHTS_ONE's
 * table realises them (q_own_i: "The lights, stated"; 0 where n_emit exceeds JADE_LIGHTS_ONE_MAX_ENTRIES and that table is not made).
 * For every other triangle - an emitter that is not listed, a listed triangle that does not emit or emits below the threshold, a
 * degenerate one - both are 0.  mu(h) = m(h) under JADE_LIGHTS_ALL and M(h) under JADE_LIGHTS_ONE.
 *
 * The densities, from a vector l from the vertex to a point of h and the vertex's stored normal n (nn = dot(n, n)), both per solid angle:
 *     ll = dot(l, l);  rl = sqrt(ll)
 *     pA = ((ll * rl) * sqrt(nne)) / (A * |dot(ne, l)|)          (a uniform point of h)
 *     PL = mu(h) * pA
 *     pB = |dot(n, l)| / ((rl * sqrt(nn)) * fl(pi))               (the cosine bounce; pi = the reference's 3.1415926)
 *     w_L = 1 / (1 + pB / PL)                                      (= PL / (PL + pB))
 *     g_B = ((m(h) * (|dot(n, l)| / rl)) * sqrt(nne)) / (PL + pB)
 * One function forms them on both sides: on the emitter side l = the shadow ray's direction as recorded (point - vertex, not
 * normalised), on the bounce side l = fl(hit point - vertex), the indirect ray's recorded hit point.
 * Edges.  If m(h) is not > 0 (h is not weighted), or the vertex falls back under JADE_BOUNCE_COSINE (!(nn > 0 && nn < inf)):
 * w_L = 1 and g_B = 0 - no weight, no bounce term.  dot(ne, l) = 0 or an overflowing numerator gives pA = PL = inf: w_L = 1 / (1 + 0) = 1
 * (the term it multiplies is 0 in the first case) and g_B = 0.  PL = 0 by underflow with pB > 0: pB / PL = inf, w_L = 0, and the bounce
 * term carries everything.  pB = 0 with PL > 0: w_L = 1.  NaN arises only from l.l = 0 (where today's term is NaN as well), from
 * numerator and denominator of pA overflowing together, or from PL and pB both 0; there is no inf / inf for l.l > 0 otherwise.
 *
 * The emitter term.  An emitter term whose entry names a weighted triangle is JADE_BOUNCE_COSINE's term times w_L, one multiplication
 * per channel - under JADE_LIGHTS_ONE after the multiplication by that mode's weight.  An entry whose triangle is not weighted keeps its
 * term.
 * The bounce term.  When the vertex survived the roulette, its indirect ray's nearest hit is h and h is weighted,
 *     T_B = ((Le(h) * f) * g_B) / fl(0.9)            per channel
 * is added to l_dir BEFORE the vertex's scale (k, or k / 0.5 at an SSS-diffuse vertex); f is the factor of the vertex's direct light
 * (brdf fl(1 / pi) at a diffuse vertex, refract_albedo fl(1 / pi) at an SSS-diffuse one - not the indirect rate's brdf).  The path ends
 * there as it does in the reference.  With omega = l / |l|, T_B = m Le f |n.omega| sqrt(nne) / (PL + pB) / RR.
 * Why the integral is unchanged.  Per listed entry the reference's expectation is the integral of Le f |n.omega| sqrt(nne) V over the
 * hemisphere on the vertex's side (the area measure dA = d omega ll rl sqrt(nne) / |ne.l| turns its term into that).  At every
 * (omega, h) the m emitter samples carry w_L = PL / (PL + pB) each, and the bounce sample - drawn with density pB, kept with
 * probability RR - carries m pB / (PL + pB): together m, the reference's count.  Both techniques see the same visibility (nearest hit
 * from the vertex, its own triangle excluded) and the same side.  Unweighted triangles contribute exactly as before.
 * The bound: term x w_L <= term x PL / pB = pi f Le sqrt(nn) sqrt(nne) mu per entry (under JADE_LIGHTS_ONE x 1 / p_i), and
 * T_B <= m Le f |n.omega| sqrt(nne) / pB / RR = pi f Le sqrt(nn) sqrt(nne) m / RR.
 *
 * The schedule is JADE_BOUNCE_COSINE's.  Results do not depend on steps, tile partitions or records per pixel.
 *
 * jade_scene_set_direct_sampling: an unknown mode returns JADE_ERR_INVALID and leaves the previous mode in place.
 * jade_render_begin refuses JADE_DIRECT_MIS without JADE_BOUNCE_COSINE (jade_scene_set_bounce_sampling) with JADE_ERR_UNSUPPORTED; a
 * lens or a shutter is refused by JADE_BOUNCE_COSINE's own check.
 * jade_render_multi: all scenes must carry the same mode, else JADE_ERR_INVALID before anything is launched. */
#define JADE_DIRECT_RAYS 0
#define JADE_DIRECT_MIS 1

int jade_scene_set_direct_sampling(jade_scene* scene, int mode);
int jade_scene_get_direct_sampling(jade_scene* scene, int* mode);

/* ---- Light passes ----
 *
 * A render can keep, beside its frame, the same radiance split into JADE_PASS_COUNT passes by the statement that produced each addend:
 * emission, background, sky light and lamp light, each direct and indirect, per kind of vertex - what an offline renderer calls render
 * passes or light AOVs, and what says where a frame's bright samples come from.  jade_scene_set_passes(scene, 1) is a property of the
 * scene handle, read by the next jade_render_begin; a render in progress keeps what it began with.  With passes off (the default) a
 * render is today's in every kernel, bit and counter.  With passes on the FRAME is unchanged in every bit, and so is every integer
 * counter of jade_stats, against the same render under the list schedule (below); jade_render_passes returns the split.
 *
 * ---- The passes, stated ----
 * tests/passes_spec.py is this text in float64.  A finished sample's colour is le + acc + thr * l_final, where acc is the sum over the
 * pushed vertices of thr_at_that_vertex * l_dir (jade_rt.h; PathTrace.cu:1410-1413 unwinds the same sum).  Every addend belongs to
 * exactly one pass, decided by the statement that formed it:
 *
 *   JADE_PASS_BACKGROUND (0)    sampleHdr(d) of a camera ray that hit nothing
 *   JADE_PASS_EMISSION (1)      le, the emission of the camera ray's triangle; and thr * emissive where the head of the bounce loop ends a
 *                               path on an emitter (PathTrace.cu:916-920, and the mirror branch's emissive statement).  The reference
 *                               counts a directly seen emitter twice: both addends land here.
 *   JADE_PASS_SPECULAR_SKY (2)  thr * l_final of a mirror ray that hit nothing (:1383-1398) and of a refraction's exit ray that hit
 *                               nothing (:1239-1257): the sky at the end of a mirror or glass chain
 *   3 + 4 kind + 2 source + depth (3 .. 14)   the parts of a sampling vertex's l_dir:
 *       kind    0 diffuse (:1266-1364), 1 SSS-diffuse (:931-1028), 2 BSSRDF (:1029-1178)
 *       source  0 the emitters: the shadow-ray loop's terms and, under JADE_DIRECT_MIS, the bounce term T_B; 1 the sky: the environment
 *               ray's term, with its JADE_ENV_IMPORTANCE ratio or JADE_ENV_MIXTURE m
 *       depth   0 if nothing has been pushed when the vertex is folded (the path's push count is 0): the camera ray's own vertex;
 *               otherwise 1 - a mirror or a refraction pushes too, so a vertex seen through either is a later one
 *
 * A part is thr * (scale * sum_of_that_source), all in fp32: the source's terms are added in the order l_dir adds them, scale is the
 * branch's own (k, k / 0.5 at an SSS-diffuse vertex, k / (1 - 0.5) at a BSSRDF vertex, the constants l_dir is multiplied with), thr the
 * throughput before that vertex's push.  l_dir, acc and thr themselves are formed by the unchanged statements.  A part that is 0 in all
 * three channels is not added.
 *
 * Two quirks of the reference are followed, not repaired:
 *   "surface is not close" (:1231): the refraction loop returns 0 and the sample's colour is le alone.  The parts the sample has
 *   gathered are dropped; only le goes to JADE_PASS_EMISSION.
 *   The 128th push: the path ends with le + acc + thr_new * l_final, where l_final is the l_dir just pushed - that vertex is counted
 *   again with the new throughput.  The second addend is split exactly as the first.
 *
 * Per record the parts of a sample are added in the order they are formed, then le; a finished sample's sums are added to the
 * record's totals in the order its samples end; jade_render_passes adds a pixel's records in ascending order and multiplies with the
 * factor jade_render_resolve uses for that pixel (1 / samples, or its tile's after jade_render_adaptive).  No atomics: the same bits
 * every time, under every step split, tile partition and schedule switch; across JADE_RECORDS_PER_PIXEL only the order of the last sum
 * differs.  For every pixel the sum over the passes equals the frame up to fp32 summation order.
 *
 * The schedule is the one a lens runs: no fused first pass, no k_tail, JADE_SHADE_BINNED ignored (those kernels book nothing).  A
 * record carries 424 bytes more, which jade_render_begin counts when it chooses the records per pixel and when it answers
 * JADE_ERR_NOMEM.  jade_render_query's JADE_Q_STATE_BYTES counts them.  The jade_render_begin of a render that keeps no passes frees
 * that memory before it measures what is free; the render in progress ends there, also where that jade_render_begin then fails.
 *
 * jade_render_begin refuses passes together with a lens, a shutter or JADE_LIGHTS_ONE with JADE_ERR_UNSUPPORTED (those kernels are
 * not built yet), after the other modes' own refusals, and together with JADE_PIXEL_ROTATE.  jade_render_multi refuses a handle that
 * has passes on with JADE_ERR_UNSUPPORTED: each rank renders its share and calls jade_render_passes.
 * jade_render_passes: out is JADE_PASS_COUNT x height x width x 3 floats, pass by pass, each laid out and treated for tile shares
 * exactly as jade_render_resolve's out_rgb; callable wherever jade_render_resolve is, with the same meaning (the samples finished so
 * far; carried paths are flushed).  JADE_ERR_INVALID, naming the setter, if the render in progress keeps no passes.
 * jade_pass_name: "background", "emission", "specular_sky", then "<diffuse|sss|bssrdf>_<emitter|sky>_<first|later>"; null out of range. */
#define JADE_PASS_COUNT 15
#define JADE_PASS_BACKGROUND 0
#define JADE_PASS_EMISSION 1
#define JADE_PASS_SPECULAR_SKY 2
#define JADE_PASS_DIFFUSE_EMITTER_FIRST 3
#define JADE_PASS_DIFFUSE_EMITTER_LATER 4
#define JADE_PASS_DIFFUSE_SKY_FIRST 5
#define JADE_PASS_DIFFUSE_SKY_LATER 6
#define JADE_PASS_SSS_EMITTER_FIRST 7
#define JADE_PASS_SSS_EMITTER_LATER 8
#define JADE_PASS_SSS_SKY_FIRST 9
#define JADE_PASS_SSS_SKY_LATER 10
#define JADE_PASS_BSSRDF_EMITTER_FIRST 11
#define JADE_PASS_BSSRDF_EMITTER_LATER 12
#define JADE_PASS_BSSRDF_SKY_FIRST 13
#define JADE_PASS_BSSRDF_SKY_LATER 14

int jade_scene_set_passes(jade_scene* scene, int on);
int jade_scene_get_passes(jade_scene* scene, int* on);
const char* jade_pass_name(int pass);
int jade_render_passes(jade_scene* scene, float* out);

/* ---- Branch sampling ----
 *
 * Non-parity.  At a vertex the reference tosses coins: select_reflex_refract < 0.5 takes a material's refraction arm (glass, or the jade's
 * sub-surface arms) and weighs it 1 / 0.5, a second select < JADE_SSS_RATE_D takes the SSS-diffuse arm of a JADE_SUB_SURFACE material,
 * and the mirror's roulette goes on with probability JADE_RR_RATE.  A branch taken with probability q and weighted 1 / q whose value is T
 * adds T^2 q (1 - q) of per-sample variance from the coin alone.  Every pixel draws its samples with known indices 0 .. spp - 1, so under
 * JADE_BRANCH_STRATIFIED the coins of a path's first two vertices are shared out among a pixel's samples instead of tossed: exactly half
 * of any aligned 2^k samples take each arm, and of those the stated share goes on.  The probabilities, the weights and every other
 * statement are unchanged, each sample's number is uniform, so the estimator is unbiased; it costs no ray, no record word and no draw.
 * jade_scene_set_branch_sampling is a property of the scene handle, read by the next jade_render_begin; a render in progress keeps the
 * mode it began with.  JADE_BRANCH_RANDOM (0, the default) is today's render in every kernel, bit and counter.  An unknown value is
 * JADE_ERR_INVALID.
 *
 * ---- The branch draws, stated ----
 * tests/branch_spec.py is this text in numpy.  All integers are uint32_t and arithmetic wraps.
 *
 * The two sequences.  A(i) is the bit reversal of i (van der Corput in base 2 as 32-bit fixed point; __brev on the device).  B(i) is
 * Sobol's second dimension: r = 0; v = 0x80000000; then for every bit of i, lowest first: if (i & 1) r ^= v; i >>= 1; v ^= v >> 1; B = r.
 * Together they are a (0, 2)-sequence in base 2: every aligned block of 2^k indices puts one point into each elementary interval of
 * area 2^-k, and a digital shift (an XOR of each dimension with a constant) keeps that.
 *
 * The shift of a pixel's render.  D(x, y, frame, d): s = jade_rng_seed(x, y, frame) ^ (d == 0 ? 0x68E31DA4u : 0xB5297A4Du); jade_wang is
 * applied to s twice, and D is the second result.  frame is jade_render_params.frame, NOT frame + sidx.
 *
 * The stratified number of sample sidx of pixel (x, y) at a vertex of depth d - the path's push count when the vertex is shaded, 0 at
 * the camera ray's vertex -, for d < 2:
 *   U = (d == 0 ? A(sidx) : B(sidx)) ^ D(x, y, frame, d)
 * Vertices of depth 2 and more use the stream's draws.  su(W) = (float)W * 2.3283064365386963e-10f, jade_rand's own conversion.
 *
 * What U replaces, at a vertex of depth 0 or 1:
 *   the first select_reflex_refract is su(U);
 *   on a material with refract_mode != JADE_NO_REFRACT that one bit is spent, and every later decision at that vertex uses V = U << 1:
 *     the second select of a JADE_SUB_SURFACE material, su(V) < (float)JADE_SSS_RATE_D, and the mirror branch's rr_result = su(V);
 *   on a material without a refraction arm the select decides nothing, and the mirror branch's rr_result = su(U).
 * Every comparison stays the float comparison it is.  The jade_rand calls stay where they are and their values are discarded, so every
 * other draw of the path keeps its position in the sample's stream.  Nothing else is stratified: the diffuse branches' roulette for the
 * indirect ray, the refraction loop's reflex_refract_select, the area draw, all directions and the film jitter are the stream's.
 *
 * A dimension is used at most once per path: a vertex is shaded only as the camera ray's (depth 0) or after the fold of a bounce's rays
 * moved the path on, and every such move is a push, which counts the depth up; so no two vertices of a path share a depth, and the one
 * vertex of depth 0 and the one of depth 1 read different dimensions.  (Two vertices sharing a number would bias the estimator.)
 *
 * The schedule is the one a lens runs: no fused first pass, no k_tail, JADE_SHADE_BINNED ignored.  Rays per kind, path lengths and the
 * record layout are the random mode's in distribution; no counter is the same number.  Results do not depend on steps, tile partitions,
 * the walk or the records per pixel.  The denoiser, exposure, glare and passes (under the reference estimator) run on top unchanged.
 *
 * JADE_PIXEL_ROTATE stays legal: a record's samples then move between pixels, each pixel's numbers are still uniform and the render
 * unbiased, but a pixel no longer sees an aligned run of indices, so the stratification is no longer guaranteed.
 * jade_render_adaptive runs on top, and a stopped tile is that tile of the uniform stratified render at its count.  Its error estimate
 * assumes independent samples; a pixel's stratified samples are negatively correlated, so under this mode the estimate is an
 * over-estimate of the error and tiles stop later than they could.  A limitation, not a defect.
 *
 * jade_render_begin refuses JADE_BRANCH_STRATIFIED with JADE_ERR_UNSUPPORTED together with a lens, a shutter or JADE_LIGHTS_ONE, and
 * together with passes under anything but the reference estimator (those kernels are not built yet), after the other modes' own
 * refusals.  The oracle backend knows the parity estimator only and has no such entry.  jade_render_multi compares the setting between
 * its scenes as it compares the others. */
#define JADE_BRANCH_RANDOM 0
#define JADE_BRANCH_STRATIFIED 1
int jade_scene_set_branch_sampling(jade_scene* scene, int mode);
int jade_scene_get_branch_sampling(jade_scene* scene, int* mode);

/* ---- Smooth shading: vertex normals interpolated at every path vertex ----
 *
 * Non-parity.  Every triangle carries one flat normal (jade_triangle.norm), and the reference shades with nothing else, so a curved
 * object shows its facets in the mirror arm, in the Fresnel factors, in every hemisphere and in the denoiser's normal guide.
 * jade_scene_set_vertex_normals gives the handle three normals per triangle - 9 floats, corners in the order p1 p2 p3, triangles in the
 * scene description's order; NULL clears - and every vertex a path is shaded at then uses the normal interpolated at its point.  The table
 * is a property of the handle, taken by the next jade_render_begin like the lens; a render in progress keeps the table it began with.  A
 * count that is not the scene's is JADE_ERR_INVALID.  Entries that are not finite are not refused: they fall back as stated below.
 * jade_scene_get_vertex_normals: *set = 1 if a table is set.  A triangle whose three normals are bitwise its norm is FLAT; a table that
 * is flat everywhere, like no table, is today's render in every kernel, bit and counter.
 *
 * ---- The shading normal, stated ----
 * tests/smooth_spec.py is this text in float64.  fl() rounds to fp32; dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)).
 *
 * The record of a triangle with corners p1 p2 p3, corner normals n1 n2 n3 and stored flat normal g (of any length), made when the table
 * is set: in double, from the fp32 corners, e1 = p2 - p1, e2 = p3 - p1, N = e1 x e2, NN = N.N; the triangle is FLAT as said above, else
 * DEGENERATE if !(NN > 0 && NN < inf), else it keeps d2 = fl((e2 x N) / NN) and d3 = fl((N x e1) / NN) per component - the dual basis, so
 * that with w = p - p1 the barycentrics are b2 = ((w x e2).N) / NN = w.d2 and b3 = ((e1 x w).N) / NN = w.d3, b1 = 1 - b2 - b3 - and
 * m2 = n2 - n1, m3 = n3 - n1, one fp32 subtraction per component.
 *
 * normal(triangle, p, r), the ONE function every use goes through - the BSSRDF exit point too, although its barycentrics are known:
 *   FLAT or DEGENERATE: g.
 *   w = p - p1;  b2 = dot(w, d2);  b3 = dot(w, d3);  s = fma(b3, m3, fma(b2, m2, n1)) per component   ( = b1 n1 + b2 n2 + b3 n3 )
 *   There is no clamp: a point a rounding outside the triangle extrapolates.
 *   ss = dot(s, s);  if !(ss > 0 && ss < inf): g  (the predicate of "The bounce, stated").   ns = s / sqrt(ss), the division per component.
 *   The side rule: a = dot(ns, r), b = dot(g, r); unless (a > 0 && b > 0) || (a < 0 && b < 0): g, for everything at this vertex - a viewer
 *   never sees the back of a shading normal.  The product (ns.r)(g.r) <= 0 of the rule is never formed, so it cannot underflow.
 *   Otherwise n = ns.
 * r is `out` at a vertex a ray arrived at (a camera ray's, a mirror's, an indirect ray's, a glass chain's), inner_direction = exit point -
 * entry vertex at a BSSRDF exit, and the reversed incoming direction at a hit of the refraction loop.
 *
 * Directions the normal FORMS.  same(d, r): dot(d, g) and dot(r, g) are both > 0 or both < 0; other(d, r): one > 0, the other < 0.
 *   mirror: refl = n * (2 dot(out, n)) - out; unless same(refl, out) it is formed again with g in place of n.
 *   refraction entry: gen_refract_ray(-out, n, 1 / index) and the Fresnel factor of |dot(n, out)|; unless other(ray, out) both are formed
 *     again with g.
 *   refraction loop, with hn = normal(hit triangle, hit point, -ray): gen_refract_ray(ray, hn, index), the Fresnel factor of |dot(new ray,
 *     hn)|, and - on total reflection or where the iteration's draw says reflect - the reflection about hn; unless the direction the
 *     iteration leaves with is same(d, -ray) when reflected and other(d, -ray) when refracted, all of it - total reflection's decision
 *     included - is formed again with the flat normal, on the same draw.
 *   So no ray starts into the wrong side of its own triangle.
 * Directions that are DRAWN, at diffuse, SSS-diffuse and BSSRDF vertices, under both bounce samplings and the three environment samplings:
 *   every side test, flip, axis and cosine the statements make against the vertex's normal - n at a diffuse or SSS-diffuse vertex, t_norm =
 *   normal(exit triangle, exit point, inner_direction) at a BSSRDF exit, the entry's Fresnel factor with n - is made against this normal.
 *   A direction that passes is tested against g with the same expression - dot(d, g) * dot(out, g) < 0 at a diffuse vertex,
 *   dot(d, g) * dot(inner, g) < 0 for the BSSRDF environment ray and > 0 for its indirect ray - and one that fails there is not traced
 *   and contributes nothing: an emitter ray as the reference's `continue`, the environment ray as a direction on the wrong side under
 *   JADE_ENV_IMPORTANCE (the mixture's hemisphere technique included), the indirect ray as a roulette that failed.  The reference tests no
 *   side for the BSSRDF branch's emitter rays, so none is tested against g.  All draws are made before these tests: a sample's stream
 *   positions are those of the flat render of the same decisions.  Rays that are not traced are not counted in jade_stats.
 * What stays g: an emitter's own normal in an emitter term - the measure of its area.
 * The denoiser's guide pass follows its mirror chain with the mirror statement above and its normal guide is the shading normal, turned
 * towards the viewer as the flat one is.
 * Known: the cull against g darkens a coarse mesh at grazing light (the shadow terminator); nothing softens it.
 *
 * The schedule is the one a lens runs: no fused first pass, no k_tail, JADE_SHADE_BINNED ignored.  Results do not depend on steps, tile
 * partitions, the walk or the records per pixel.  Adaptive sampling, the guides and the denoiser, exposure and glare run on top.
 * jade_render_begin takes a table that is not flat everywhere with the three environment samplings, with JADE_BOUNCE_COSINE and with a
 * lens (not both), and refuses it with JADE_ERR_UNSUPPORTED together with a shutter, JADE_LIGHTS_ONE, JADE_DIRECT_MIS, passes or
 * JADE_BRANCH_STRATIFIED (those kernels are not built yet), after the other modes' own refusals.  jade_render_multi: every scene's handle
 * carries such a table or none does, else JADE_ERR_INVALID.  The oracle backend has no such entry. */
int jade_scene_set_vertex_normals(jade_scene* scene, const float* normals, int32_t n_triangles);
int jade_scene_get_vertex_normals(jade_scene* scene, int* set);

/* ---- Albedo textures: UVs per triangle, images filtered at every path vertex ----
 *
 * Non-parity.  Every triangle has one brdf and one refract_albedo (jade_material), so a colour cannot vary over a surface.
 * jade_scene_set_textures gives the handle n_images images, six floats of UV per triangle - (u, v) of the corners p1 p2 p3, triangles in
 * the scene description's order - and one image number per triangle, -1 for a triangle without an image.  An image is width x height
 * texels of linear RGB, interleaved, row 0 at v = 0, texel (i, j) covering u in [i / W, (i + 1) / W).  The texels are copied: the caller's
 * arrays may go after the call.  n_images = 0 or a NULL array clears.  The table is a property of the handle, taken by the next
 * jade_render_begin like the lens and the vertex normals; a render in progress keeps the table it began with.
 * JADE_ERR_INVALID, with a message that names the offender, and the handle's table left as it was: an n_triangles that is not the scene's,
 * an image_of outside [-1, n_images), a width or height outside 1 .. 16384, more than 65 536 images, a texel that is not finite.  UVs that
 * are not finite are NOT refused (the statement says what they give), and texels are otherwise used as given: negative values and values
 * above 1 pass through.  jade_scene_get_textures: *set = 1 if a table is set.  A table in which no triangle names an image, like no table,
 * is today's render in every kernel, bit and counter.
 *
 * ---- The surface colour, stated ----
 * tests/texture_spec.py is this text: the lookup in float64, the fetch in emulated fp32 as well.  fl() rounds to fp32; fma(a, b, c) is
 * a * b + c rounded once; dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), as in "The shading normal, stated".
 *
 * The record of a triangle with corners p1 p2 p3 and corner UVs uv1 uv2 uv3, made when the table is set: d2 and d3 exactly as the smooth
 * record's - in double, from the fp32 corners, e1 = p2 - p1, e2 = p3 - p1, N = e1 x e2, NN = N.N, d2 = fl((e2 x N) / NN), d3 = fl((N x e1)
 * / NN) per component - except that a triangle whose NN is not in (0, inf) keeps d2 = d3 = 0, so that every one of its points has uv1;
 * du2 = uv2 - uv1 and du3 = uv3 - uv1, one fp32 subtraction per component.
 *
 * uv(triangle, p):  w = p - p1;  b2 = dot(w, d2);  b3 = dot(w, d3);  u = fma(b3, du3.x, fma(b2, du2.x, uv1.x));  v the same with .y.
 *   There is no clamp: a point a rounding outside its triangle extrapolates.
 *
 * colour(image, u, v), each line one fp32 operation, W and H the image's size, t(i, j) texel i of row j:
 *   If u or v is NaN or infinite the colour is (1, 1, 1) and nothing below is formed.
 *   u' = u - floor(u)                  in [0, 1]: 1 itself where u is a small negative number
 *   x  = fma(u', fl(W), -0.5f)         texel centres at the integers
 *   xf = floor(x);  fx = x - xf;  i0 = (int)xf  in [-1, W - 1];  i1 = i0 + 1
 *   an i0 of -1 becomes W - 1, an i1 of W becomes 0                                    (the image repeats)
 *   v, H, y, yf, fy, j0, j1 the same.  Then per channel:
 *   top = fma(fx, t(i1, j0) - t(i0, j0), t(i0, j0));  bottom = fma(fx, t(i1, j1) - t(i0, j1), t(i0, j1));  c = fma(fy, bottom - top, top)
 *   So every index is in range for every float input, a constant image returns its constant exactly (every difference is 0), a texel
 *   centre returns its texel exactly where x and y are formed exactly (a power-of-two size), and c has period 1 in u and in v.
 *
 * The surface colour c(triangle, p) is (1, 1, 1) for a triangle without an image - it costs the first 16 bytes of its record - and
 * colour(its image, uv(triangle, p)) otherwise.  The material at a vertex: brdf_eff = fl(brdf * c) and albedo_eff = fl(refract_albedo * c)
 * per channel, formed first; every statement that reads brdf or refract_albedo of the vertex's triangle reads these instead, with p the
 * vertex's point: the mirror's emissive term, its rate and its sky term, the f of a diffuse or SSS-diffuse vertex and its indirect rate.
 * NOT touched: emissive and its two thresholds, refract_rate, refract_index, the modes, the emitter table and its power, and every draw.
 * A texture multiplies radiance: it changes no ray, no draw and no jade_stats counter.  An image of ones is the untextured render bit for
 * bit, a constant image the render with fl(brdf * c) and fl(refract_albedo * c) written into the materials.
 * The denoiser's guide pass multiplies its throughput and its albedo guide by brdf_eff, at every vertex of its mirror chain.
 *
 * A textured render runs the kernels and the schedule of a smooth render (above), with the handle's vertex normals or, where it carries
 * none, the flat ones: no fused first pass, no k_tail.  Results do not depend on steps, tile partitions, the walk or the records per pixel.
 * Adaptive sampling, the guides and the denoiser, exposure and glare run on top.  jade_render_begin takes a table that names an image with
 * the three environment samplings, with JADE_BOUNCE_COSINE and with a lens (not both), with vertex normals and without, and refuses it
 * with JADE_ERR_UNSUPPORTED together with a shutter, JADE_LIGHTS_ONE, JADE_DIRECT_MIS, passes or JADE_BRANCH_STRATIFIED, after the other
 * modes' own refusals and in smooth shading's words.  jade_render_multi: every scene's handle carries such a table or none does, else
 * JADE_ERR_INVALID.  The oracle backend has no such entry.
 * Not here: mip maps or any filtering by footprint (a minified image aliases, and the samples of a pixel average it); textures on
 * emissive, refract_rate or the normal. */
typedef struct jade_texture_image {
  int32_t width, height;
  const float* rgb; /* width * height * 3 floats */
} jade_texture_image;
int jade_scene_set_textures(jade_scene* scene, int32_t n_images, const jade_texture_image* images, const float* uv, const int32_t* image_of,
                            int32_t n_triangles);
int jade_scene_get_textures(jade_scene* scene, int* set);

/* ---- Normal maps: tangent-space images bend the shading normal at every path vertex ----
 *
 * Non-parity.  Vertex normals give a surface a normal that varies over a triangle and textures a colour that does; relief - the grain of a
 * carved statue, the joints of a tiled floor - still takes triangles, and those are what k_trace pays for.  jade_scene_set_normal_maps
 * gives the handle n_images images of tangent-space vectors (x, y, z) per texel, ALREADY DECODED (the 2c - 1 of an 8-bit file is the host
 * loader's: load_normal_map), in the layout and within the size limits of jade_scene_set_textures; six floats of UV and an image number
 * per triangle, the map's OWN - independent of the albedo table's; -1 for a triangle without a map - and a strength, finite and >= 0,
 * that scales x and y.  n_images = 0 or a NULL array clears.  The table is a property of the handle, taken by the next jade_render_begin
 * like the vertex normals and the textures; a render in progress keeps the table - and the strength - it began with.
 * JADE_ERR_INVALID, with a message that names the offender, and the handle's table left as it was: an n_triangles that is not the scene's,
 * an image_of outside [-1, n_images), a width or height outside 1 .. 16384, more than 65 536 images, a texel that is not finite, a strength
 * that is not finite or is negative.  UVs that are not finite are NOT refused (the statement says what they give).  Texels are not
 * normalised and need not be: the statement normalises what it forms.  jade_scene_get_normal_maps: *set = 1 if a table is set.  A table
 * that maps no triangle, like no table, is today's render in every kernel, bit and counter.
 *
 * ---- The mapped normal, stated ----
 * tests/normal_map_spec.py is this text in float64, the per-vertex arithmetic in emulated fp32 as well.  fl(), fma() and dot() as in "The
 * surface colour, stated"; normal(triangle, p, r), ns, g and the side rule as in "The shading normal, stated"; uv() and colour() as in
 * "The surface colour, stated".
 *
 * The record of a triangle, made when the table is set.  Its UV part is the texture record's, statement for statement, from the map's UVs:
 * d2, d3, uv1, du2, du3.  Then, in double from the fp32 corners and the record's fp32 du2 and du3:
 *   det = du2.x * du3.y - du3.x * du2.y
 *   T = (e1 * du3.y - e2 * du2.y) / det        B = (e2 * du2.x - e1 * du3.x) / det
 * each divided by its length and rounded to fp32 once per component.  They are dP/du and dP/dv: constant over the triangle, NOT made
 * orthogonal to each other or to any normal, NOT interpolated - a sheared UV layout shears the relief with it, as it shears the image.
 * The triangle is UNMAPPED, and stored with image -1, if it names no image, if NN is not in (0, inf), if det is zero or not finite, or
 * if the length of T or of B is not in (0, inf).
 *
 * normal'(triangle, p, r) stands for normal(triangle, p, r) at EVERY use, when a map table is set:
 *   1. An unmapped triangle: normal(triangle, p, r).  It costs the first 16 bytes of its record, then what normal() costs.
 *   2. (u, v) = uv(triangle, p) with the map's record.  If u or v is NaN or infinite: as unmapped.
 *   3. m = colour(the map's image, u, v) by the fetch statement, operation for operation.
 *   4. mx = fl(strength * m.x);  my = fl(strength * m.y);  mz = m.z.
 *   5. If mx == 0 && my == 0, or any of mx my mz is NaN: as unmapped, and nothing below is formed.  So a texel (0, 0, z) - whatever z,
 *      negative included - and a strength of 0 give today's normal bit for bit.
 *   6. The base nb: the ns of normal(triangle, p, r) BEFORE its side rule; where the triangle is FLAT or the sum rule fails,
 *      g / sqrt(dot(g, g)), the division per component; and if dot(g, g) is not in (0, inf): as unmapped.
 *   7. t = fma(mz, nb, fma(my, B, fl(mx * T))) per component;  tt = dot(t, t);  if !(tt > 0 && tt < inf): as unmapped;  nm = t / sqrt(tt).
 *   8. The side rule, as a cascade: a = dot(nm, r), b = dot(g, r); if (a > 0 && b > 0) || (a < 0 && b < 0) the result is nm.  Otherwise
 *      it is normal(triangle, p, r) - ns under its own side rule, and then g.
 * Everything "The shading normal, stated" says after the normal stays, word for word, with normal' for normal: directions the normal forms
 * are formed again with g unless they leave on the right side; drawn directions are made against normal' and culled against g; all draws
 * come before the tests, so a sample's stream positions are the flat render's; an emitter's own normal stays g; the guide pass follows its
 * mirror chain with normal' and its normal guide is normal', turned towards the viewer.  A map changes rays through these rules only.
 * The codes jade_smooth.h's SMOOTH_RULE_* gain: MAPPED (nm), MAP_ZERO (step 5), MAP_SUM (steps 6 and 7), MAP_SIDE_NS (step 8 gave ns).
 *
 * A mapped render runs the kernels and the schedule of a textured render (above) - with the handle's textures or, where it names no
 * image, a table that names none; with its vertex normals or the flat ones: no fused first pass, no k_tail.  jade_render_begin takes a
 * table that maps a triangle with the three environment samplings, with JADE_BOUNCE_COSINE and with a lens (not both), and refuses it with
 * JADE_ERR_UNSUPPORTED together with a shutter, JADE_LIGHTS_ONE, JADE_DIRECT_MIS, passes or JADE_BRANCH_STRATIFIED, after the other
 * modes' own refusals, in the words of smooth shading or of textures where the handle carries those and in its own name otherwise.
 * jade_render_multi: every scene's handle carries such a table or none does, else JADE_ERR_INVALID.  The oracle backend has no such entry.
 * Not here: mip maps or any filtering by footprint; interpolated or orthogonalised tangents; displacement - the surface a ray hits is
 * the triangle's, and only its normal bends. */
int jade_scene_set_normal_maps(jade_scene* scene, int32_t n_images, const jade_texture_image* images, const float* uv, const int32_t* image_of,
                               int32_t n_triangles, float strength);
int jade_scene_get_normal_maps(jade_scene* scene, int* set);

#ifdef __cplusplus
}
#endif
#endif /* JADE_BVH_H */
