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
 * oracle does not implement: adaptive sampling and its noise map (below).
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
 * nodes_out[max_nodes], *n_nodes_out: the tree; 2*n + 1 entries always suffice
 * build_ms (nullable): device time of the build kernels (sort included), without the copies
 * leaf_size: 1..15 (the reference uses 8) */
int jade_bvh_build_lbvh(const jade_triangle* triangles, int32_t n, int32_t leaf_size, int device_id,
                        int32_t* order_out, jade_bvh_node* nodes_out, int32_t max_nodes,
                        int32_t* n_nodes_out, double* build_ms);

/* Same contract, better tree: PLOC (parallel locally-ordered clustering).  Clusters - at first the triangles in Morton
 * order - are merged bottom-up, each with the neighbour within 16 positions whose union with it has the smallest
 * surface area, i.e. by the measure the reference's sweep-SAH builder minimises top-down (PathTrace.cu:532-628)
 * rather than by the Morton code's bits; subtrees of <= leaf_size triangles become leaves as in the reference
 * (:525-529).  Tens of rounds of four small kernels: milliseconds at 870 k triangles. */
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

#ifdef __cplusplus
}
#endif
#endif /* JADE_BVH_H */
