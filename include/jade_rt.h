/*
 * jade_rt.h — the C ABI of the jade path-tracing hot path.
 *
 * This is the seam SURVEY.md §8(b) identifies in the reference: everything
 * between "the flat host arrays are ready" (PathTrace.cu:1570-1612) and "the
 * BGR bytes are back on the host" (PathTrace.cu:1739).  The reference has no
 * plugin/FFI API; its implicit interface is the argument list of the
 * `render_pixel` kernel plus six __constant__ symbols
 * (PathTrace.cu:643-648, 1418, 1704-1710, 1731).  The entry points below carry
 * exactly that information: plain pointers and sizes, `int` status codes, no
 * exceptions, no exit() across the boundary (the reference prints CUDA errors
 * and carries on, PathTrace.cu:1476-1482; here every failure is a status plus
 * a thread-local message).
 *
 * Two shared libraries implement this same header:
 *   libjade_hip.so     the product: hand-written HIP for gfx950 (MI355X)
 *   libjade_oracle.so  test infrastructure: a single-purpose CPU restatement
 *                      of PathTrace.cu:669-1474 (oracle/), never shipped and
 *                      never called by the product path
 *
 * The array element types mirror the reference's device structs byte for
 * byte so that a maintainer can pass `&triangles_encoded[0]` and
 * `&nodes_encoded[0]` straight through.
 */
#ifndef JADE_RT_H
#define JADE_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bump whenever a struct layout or a documented semantic changes; callers compare
 * jade_abi_version() with the value they were compiled against */
#define JADE_ABI_VERSION 7

/* status codes */
#define JADE_OK 0
#define JADE_ERR_INVALID 1     /* bad argument / inconsistent scene arrays */
#define JADE_ERR_DEVICE 2      /* HIP runtime failure, no device */
#define JADE_ERR_NOMEM 3       /* host or device allocation failed */
#define JADE_ERR_UNSUPPORTED 4 /* e.g. BVH deeper than the traversal stack */

/* material modes (PathTrace.cu:41-45; DIR_REFRACT: PathTrace.cpp:34) */
#define JADE_DIFFUSE 0
#define JADE_MIRROR 1
#define JADE_NO_REFRACT 0
#define JADE_SUB_SURFACE 1
#define JADE_DIR_REFRACT 2

/* Fixed constants of the integrator (PathTrace.cu:32-39); not parameters. */
#define JADE_TILE_SIZE 16
/* JADE_STACK_CAPACITY: bounce pushes per sample.  The reference loops `while (stack_offset < 128)` and then unwinds its (dir, rate)
 * stacks from whatever l_dir the last iteration left (PathTrace.cu:1410-1413).  A sample whose 128th push fills the stacks therefore
 * traces that push's continuation ray, shades nothing at the vertex it finds (128 shaded vertices, not 129), and returns the
 * unwinding SEEDED WITH THE LAST BOUNCE'S l_dir - which that bounce has already pushed as stack_dir[127]: the term counts twice, the
 * second time through stack_indir_rate[127].  (0 for a mirror or refraction push, whose l_dir is 0.)  Every backend reproduces
 * this; a forward-summing one returns acc + thr * l_dir with the 128th push already in acc and thr.
 * JADE_MAX_FULL_REFLEX_TIME: iterations of the refraction loop (PathTrace.cu:1196).  A ray still inside after the 32nd - reflected
 * there, totally or by its draw - leaves the loop as it is: the roulette draw and the exit ray follow in that direction, 33
 * refraction rays in all.  tests/long_paths.py makes samples that reach either limit; tests/test_gpu_long_paths.py renders them. */
#define JADE_STACK_CAPACITY 128
#define JADE_BVH_STACK_CAPACITY 128 /* traversal stack entries: a BVH of up to 127 levels (the root is level 1) is accepted, and walked at that depth by tests/test_gpu_deep_trees.py; 128 levels are refused (JADE_ERR_UNSUPPORTED) */
#define JADE_MAX_FULL_REFLEX_TIME 32

/* Sample scheduling (this ABI's definition; the reference races 31 cuRAND
 * states and is not reproducible).  Sample s (0-based, counted
 * across render_step calls) of pixel (x, y) draws from its own Wang-hash
 * stream seeded (x*1973 + y*9277 + (frame + s)*26699) | 1 — the reference's
 * GLSL seed (fshader_render.fsh:82-85) with the frame counter advanced per
 * sample, which is what its progressive preview does (one sample per frame,
 * fshader_preview.fsh:82-85, 402-403).  Samples are therefore independent work
 * items.  A pixel's radiance is summed in JADE_SAMPLE_LANES interleaved
 * partial sums (sample s goes to lane s % JADE_SAMPLE_LANES, in increasing s)
 * which are added in lane order at resolve time: the result does not depend
 * on how samples are batched into steps, on the tile partition, or on how
 * many of a pixel's samples a backend keeps in flight at once.  The lane
 * count is also the most samples of one pixel that can be in flight at once:
 * 1024 lets a GPU that holds an eighth of a 1080p frame (8-GPU tiling) keep as
 * many paths in flight as one that holds the whole frame.
 *
 * Seed reuse: the seed is 32 bits wide and forced odd, i.e. 2^31 distinct streams.  A 1920x1080 frame at
 * 4096 spp draws 8.5e9 of them, so every seed serves about four (pixel, sample) pairs: their random numbers
 * are identical (correlated noise between those samples; they see different camera rays, so their paths
 * differ from the first hit on).  It is the property of the reference's GLSL generator itself (same seed
 * expression, fshader_render.fsh:82-85), kept so that results stay comparable with it; a host that needs
 * more distinct streams varies `frame` between renders. */
#define JADE_SAMPLE_LANES 1024

/* == Triangle_cu, PathTrace.cu:327-338 (112 bytes). */
typedef struct jade_triangle {
  int32_t obj_idx;
  float p1[3], p2[3], p3[3];
  float norm[3];
  float emissive[3];
  float brdf[3];
  int32_t reflex_mode;
  int32_t refract_mode;
  float refract_rate[3];
  float refract_albedo[3];
  float refract_index;
} jade_triangle;

/* == BVHNode_cu, PathTrace.cu:341-345 (40 bytes).  nodes[0] is a dummy, the
 * root is nodes[1], a child index of 0 means "none", n > 0 marks a leaf
 * holding triangles [index, index + n - 1] (PathTrace.cu:525-529, 804, 825,
 * 1557-1565).
 *
 * The array is the caller's; what it has to be is what hitBVH (:795-859) needs:
 *   - Only the nodes the root reaches through child indices are ever read, by
 *     either backend - checked (ranges), laid out, walked.  Whatever else the
 *     array holds - spare capacity behind or between the nodes of the tree, zeros,
 *     stale records with indices far out of range - is never looked at.
 *   - A node may be reached along several paths: a leaf or a subtree with two
 *     parents, left == right.  It is walked once per path, as the reference walks
 *     it (a triangle met twice is tested twice and counted twice), as long as the
 *     whole walk - every node once per path to it - stays within 4 * n_nodes + 8
 *     visits; a longer one (a cycle never ends) is JADE_ERR_UNSUPPORTED, as is a path
 *     of more than JADE_BVH_STACK_CAPACITY - 1 levels.
 *   - Leaves may overlap, and a triangle may lie in no leaf: it is then never
 *     hit, though emit_indices may still list it and index_mapping may still name it.
 *   - A leaf's box need not contain its triangles, nor a parent's box its
 *     children's: a box that a ray does not enter (hitAABB, :758-771, value > 0)
 *     hides what lies under it, exactly as in the reference.
 *   - n <= 0 is an internal node, whatever `index` holds; n < 0 is as good as 0.
 *   - An internal node may lack one child or both (index 0); under a root
 *     without children every ray misses. */
typedef struct jade_bvh_node {
  int32_t left, right;
  int32_t n, index;
  float aa[3], bb[3];
} jade_bvh_node;

/* == Obj_seg, PathTrace.cu:348-351: inclusive range in ORIGINAL (pre-BVH)
 * triangle order. */
typedef struct jade_obj_seg {
  int32_t begin_idx;
  int32_t end_idx;
} jade_obj_seg;

/* Everything `render_pixel` reads (PathTrace.cu:1418 + 639-648).  All
 * pointers are host pointers; jade_scene_create copies, the caller keeps
 * ownership.
 *
 * What is checked is ranges - every index names an element, every segment
 * lies inside the array with begin <= end, the tree can be walked from its root
 * (jade_bvh_node above: nodes the root does not reach are not read) - and ONE value
 * (an object's total area, below).  Beyond that
 * the arrays are read the way PathTrace.cu reads them, whatever they hold, and
 * both backends give the same frame.  In particular NOT assumed:
 *   prefix_area    need not be a running sum.  Per object the BSSRDF search
 *                  (:1031-1048) bisects [begin_idx, end_idx] with u * prefix[end_idx]
 *                  and returns the LAST midpoint it looked at (0 for an object of one
 *                  or two triangles: index_mapping[0]).  The HIP module answers from
 *                  a table when the object's values are finite, non-negative, below
 *                  3e38 and non-decreasing; any other object costs it the
 *                  reference's bisection, ~log2(n) dependent loads per BSSRDF vertex,
 *                  with the same result.  A comparison with a NaN ends the search at
 *                  that midpoint (the reference would not return).  One value is
 *                  more than a search key: an object's total, prefix_area[end_idx],
 *                  multiplies the radiance that leaves through the object (:1105,
 *                  :1160).  Not finite, it gives rates of inf and NaN, whose sum
 *                  depends on the order of summation (the HIP module adds a path's
 *                  radiance forward, the reference unwinds a stack: same counters,
 *                  NaN in other pixels), and at u = 0 a search key of NaN.  So
 *                  jade_scene_create refuses, with JADE_ERR_INVALID in both
 *                  backends, a scene that has SUB_SURFACE triangles and an object
 *                  whose total is NaN or +-inf; without such triangles
 *                  prefix_area is never read by a render.  Radiance that overflows
 *                  for other reasons (emission or areas near FLT_MAX) is outside the
 *                  parity statement in the same way.
 *   index_mapping  need not be a permutation, nor stay inside the object: the exit
 *                  triangle is index_mapping[midpoint], and its refract_rate,
 *                  refract_index, norm and obj_idx are that triangle's own.
 *   emit_indices   is walked as given, one shadow ray per entry and vertex:
 *                  duplicates are sampled twice, an entry that does not emit adds
 *                  its zero, an emissive triangle that is not listed lights the
 *                  scene only where a path hits it, and n_emit = 0 is legal.
 *   obj_segs       may overlap, and need not cover the triangles whose obj_idx names
 *                  them: obj_idx only selects the segment to search.
 *   norm           is used as given - never normalised, re-derived from the
 *                  vertices or oriented.
 *   materials      are per TRIANGLE (words 13-27 of the record): neighbouring
 *                  triangles of one object may differ in every field, the two
 *                  emissive thresholds (1.4e-5, 1.5e-4) included. */
typedef struct jade_scene_desc {
  uint32_t abi_version;           /* JADE_ABI_VERSION */
  int32_t n_triangles;            /* nTriangles_dv */
  const jade_triangle* triangles; /* triangles_cu, BVH (sorted) order */
  int32_t n_nodes;                /* nNodes_dv, including the dummy node 0 */
  const jade_bvh_node* nodes;     /* node_cu */
  int32_t n_emit;                 /* nEmitTriangles_dv */
  const int32_t* emit_indices;    /* emitTrianglesIndices_cu (sorted order) */
  const int32_t* index_mapping;   /* triangle_index_mapping_cu: original -> sorted, [n_triangles] */
  const float* prefix_area;       /* prefix_size_sum_cu: per-object running area, original order */
  int32_t n_objects;
  const jade_obj_seg* obj_segs;   /* obj_segs_cu */
  int32_t env_width, env_height;  /* HDR environment, equirectangular */
  const float* env_rgb;           /* hdrRes.cols: interleaved RGB, row 0 = top (v = 0) */
} jade_scene_desc;

typedef struct jade_render_params {
  int32_t width, height; /* RENDER_WIDTH / RENDER_HEIGHT, run-time here */
  int32_t spp;           /* samples per pixel rendered by this call */
  uint32_t frame;        /* RNG frame counter of sample 0 (seed term), normally 0 */
  float eye[3];          /* eye_dv */
  float camera[16];      /* camera_transform_dv, [col][row] memory order */
  /* image partition: this call renders the 16x16 tiles (tx, ty) with
   * (tx + ty) % tile_nranks == tile_rank — diagonal interleave, so that an
   * object's pixels spread over all ranks (single GPU: 0 of 1) */
  int32_t tile_rank, tile_nranks;
  int32_t device_id;     /* HIP device ordinal (ignored by the oracle) */
  int32_t threads;       /* oracle: worker threads (0 = all cores); HIP: ignored */
  /* HIP: most device memory (bytes) this render may hold for path records and partial sums; 0 = the
   * default (60 % of what is free at jade_render_begin).  The module keeps as many of a pixel's samples
   * in flight as fit - never more than `spp` rounded up to a power of two, so a small render stays
   * small; a progressive host that will add many samples per step passes that number in `spp` here.
   * The image does not depend on either.  Oracle: ignored. */
  uint64_t max_state_bytes;
  /* How a hitBVH query (PathTrace.cu:795-859) is answered - JADE_WALK_*.  The reference walks every node whose box the
   * ray meets and keeps the nearest hit, whatever the caller then does with it.  Two of its three kinds of secondary
   * query only ask a yes/no question of that hit: a shadow ray (:956, 1096, 1292) is used as "is the nearest hit the
   * emitter it aims at" (:957, 1097, 1293), an environment-visibility ray (:980, 1123, 1316) as "is there any hit"
   * (:981, 1124, 1317).  JADE_WALK_EARLY_EXIT ends such a walk at the first recorded hit that settles the question -
   * any hit for the environment ray; for the shadow ray a hit strictly nearer than the emitter's own hitTriangle
   * distance, computed up front with the same statements - so the answer, and with it every sample, pixel and ray
   * count, is the reference's bit for bit (nothing is judged by a tolerance; no box is left out by distance), while
   * nodes_visited / tris_tested count what was actually read and are smaller.  JADE_WALK_REFERENCE (0, what a
   * zero-filled struct asks for) visits what the reference visits: nodes_visited / tris_tested equal the oracle's.
   * Oracle: ignored (it is the reference walk). */
  int32_t walk;
  /* How the direction of an environment-visibility ray is drawn - JADE_ENV_*.  JADE_ENV_REFERENCE (0, what a zero-filled struct asks
   * for): uniformly over the hemisphere, as the reference does (PathTrace.cu:968-979, 1111-1122, 1304-1315) - the mode every parity
   * statement of this header is about.  JADE_ENV_IMPORTANCE (ABI 7; SURVEY 8f rank 3, "optional importance sampling (non-parity
   * mode)"): proportionally to the environment map's luminance x sin(theta) per texel, weighted by 1 / pdf (a direction on the wrong
   * side of the surface contributes nothing and no ray is traced for it).  A different estimator of the SAME integral: the image
   * converges to the same mean with less noise under a sky with a sun, and is NOT the reference's sample for sample - none of the
   * parity claims apply to it, and the oracle refuses it (JADE_ERR_UNSUPPORTED).  Stated draw by draw below, at JADE_ENV_IMPORTANCE. */
  int32_t env_sampling;
} jade_render_params;
#define JADE_ENV_REFERENCE 0
/* JADE_ENV_IMPORTANCE, completely (tests/env_importance_spec.py is this text in float64).  W x H = env_width x env_height,
 * N = W * H, texel t = j * W + i (row j from the top, column i); PI = 3.1415926 (PathTrace.cu:36); fl() rounds to fp32.
 *
 * The distribution.  l_t = 0.2126 max(r, 0) + 0.7152 max(g, 0) + 0.0722 max(b, 0) of texel t, and 0 where that is not finite (a
 * NaN or an infinite channel); floor = 0.01 * (sum of l) / N, or 1 if the sum is 0 (a black map);
 *     w_t = (l_t + floor) * sin(PI * (j + 0.5) / H),     p_t = w_t / (sum of w),     q_t = p_t * N     (mean 1, every q_t > 0).
 * The table (made once, at jade_scene_create) has N entries {accept, alias, q_own, q_alias}: a draw that lands in slot s takes
 * texel s with probability accept_s and texel alias_s otherwise (alias_s < N; 0 <= accept_s <= 1, and alias_s = s where accept_s = 1),
 * such that texel t is drawn with probability P_t = (accept_t + sum over s != t with alias_s = t of (1 - accept_s)) / N = p_t up
 * to the fp32 rounding of accept: |P_t - p_t| <= (1 + m_t) * 2^-24 / N with m_t the number of slots whose alias is t.  q_own =
 * fl(q_s) and q_alias = fl(q_{alias_s}): the density the weight below divides by is the INTENDED one, p.  Which small texel is
 * paired with which large one is not part of this statement.
 *
 * A draw takes four uniforms u1..u4 from the sample's stream, in this order, where the reference draws the two of its uniform
 * direction (PathTrace.cu:968-971, 1111-1114, 1304-1307) - each is jade_rand's fl(uint32) * 2^-32, in [0, 1], 1.0f included:
 *     slot   s = min((uint32)fl(u1 * fl(N)), N - 1)                    (the product in fp32: a discrete decision)
 *     own    iff u2 < accept_s;      t = own ? s : alias_s,   q = own ? q_own_s : q_alias_s;      j = t / W, i = t - j * W
 *     u = (i + u3) / W,   v = (j + u4) / H,   theta = fl(PI) * v,   phi = fl(2 PI) * (u - 0.5)
 *     direction = (st * cos(phi), cos(theta), st * sin(phi))   with st = max(sin(theta), 0)
 *     ratio = fl(PI) * st / q
 * The direction is the one SampleSphericalMap (PathTrace.cu:686-692) sends to the point (u, v) of the map; its density over
 * directions is q / (2 pi^2 sin(theta)) - the map (u, v) -> direction has the Jacobian 2 pi^2 sin(theta) - and ratio is the
 * reference's density, 1 / (2 pi), over that.  theta reaches fl(PI) = 3.14159250 (u4 = 1.0f in the bottom row), 1.5e-7 short of pi, so
 * the sine is >= 0 on the whole range; the clamp makes ratio >= 0 hold whatever an fp32 sine rounds to at that end (jade_sincosf
 * gives +1.51e-7 there and nothing below 0 on [0, fl(PI)], so today the clamp changes no value); a pole's direction is (0, +-1, 0)
 * up to rounding.
 * The device evaluates u, v, theta, phi, the sines and the products in fp32 (include/jade_fpmath.h); every component of the
 * direction is then within 2.81e-6 of this statement.
 *
 * The wrong side.  Where the reference flips its direction into the surface's hemisphere (the diffuse and SSS-diffuse branch:
 * dot(direction, n) * dot(out, n) < 0; the BSSRDF branch: dot(direction, n_exit) * dot(exit - entry, n_exit) < 0), this mode
 * does NOT flip: no ray is traced, nothing is added for the environment at this vertex (it is not counted in rays_env either),
 * and the four uniforms stay drawn - every later draw of the sample is where it would be.  Otherwise the environment ray is
 * traced as the reference's is, and where it meets nothing the reference's term - sampleHdr(direction) x its weight, 2 PI
 * included - is added multiplied by ratio.  Nothing else of the sample changes.
 *
 * Map size.  The slot is formed from a 24-bit uniform and reaches every slot only while N <= 2^24: jade_render_begin refuses this
 * mode (JADE_ERR_UNSUPPORTED) on a scene whose map has more texels than JADE_ENV_IMPORTANCE_MAX_TEXELS - an 8192 x 4096 map renders
 * with JADE_ENV_REFERENCE only (jade_scene_create accepts it). */
#define JADE_ENV_IMPORTANCE 1
#define JADE_ENV_IMPORTANCE_MAX_TEXELS 16777216 /* 2^24 */
/* JADE_ENV_MIXTURE, completely (tests/env_mixture_spec.py is this text in float64): a third value of env_sampling - a value of an
 * existing field, so the ABI version stays.  JADE_ENV_IMPORTANCE draws from the map alone and knows nothing of which way the surface
 * faces: under a bright sky at least half the draws of a surface that looks sideways, and almost all of one that looks down, lie on
 * the wrong side and carry nothing.  This mode is the one-sample mixture of that draw and the render's own bounce sampling, weighed
 * by the balance heuristic: no extra ray, no extra record word, one more uniform and one 16-B gather.
 *
 * At every vertex where the reference draws its environment direction (diffuse, SSS-diffuse, BSSRDF) the sample draws FIVE uniforms
 * u0..u4, in this order, where JADE_ENV_IMPORTANCE draws four.  All five are always drawn, so every later draw of the sample is where
 * it would be whichever technique was picked.  n, side: the normal and the side term of the reference's flip at that vertex (diffuse
 * and SSS-diffuse: the vertex's normal, dot(out, n); BSSRDF: n_exit, dot(exit - entry, n_exit)).
 *
 *   u0 < 0.5 (in fp32) - the sky technique.  Slot, own / alias, texel t, q, theta, phi, st and the direction w are exactly
 *     JADE_ENV_IMPORTANCE's from (u1, u2, u3, u4);  s = st.  A direction on the wrong side follows that mode's rule unchanged -
 *     dot(w, n) * side < 0: no ray, not counted in rays_env, nothing added for the environment at this vertex.
 *   otherwise - the hemisphere technique.  w is the direction the render's bounce sampling draws from (u1, u2), as it stands:
 *     JADE_BOUNCE_UNIFORM gives the reference's statements (PathTrace.cu:968-971) and its flip, JADE_BOUNCE_COSINE the draw of "The
 *     bounce, stated" (jade_bvh.h), fallback included.  u3 and u4 are drawn and not used.  It is never on the wrong side.
 *         s = sqrt(wx^2 + wz^2);     t = the texel of w:  (u, v) = SampleSphericalMap's coordinates of w (sampleHdr's statements,
 *         PathTrace.cu:686-692, a NaN counting as 0),  i = min((uint32)fl(u * W), W - 1),  j = min((uint32)fl(v * H), H - 1)  - a
 *         negative product counts as 0 -,  t = j * W + i;     q = q_own of entry t of the table (= fl(q_t)).
 *   The weight.  m stands where JADE_ENV_IMPORTANCE has ratio - the reference's term, 2 PI included, is multiplied by it where the
 *     ray meets nothing.  With P = fl(PI):
 *         uniform hemisphere:   m = (2 P s) / (q + P s)
 *         cosine hemisphere:    m = (2 P s) / (q + 2 P s c),     c = |dot(n, w)| / sqrt(dot(n, n))
 *     and a vertex whose normal gives the cosine draw no axis (dot(n, n) is 0, infinite or NaN) uses the uniform form; its term is 0
 *     or not finite in every mode.  m = (1 / 2 pi) / (p_sky / 2 + p_hemi / 2) with p_sky = q / (2 pi^2 s) and p_hemi = 1 / 2 pi or
 *     c / pi on the surface's side, 0 off it.  Hence 0 <= m <= 2 in the uniform form and m c <= 1 in the cosine form; q > 0, so no
 *     denominator vanishes; at a pole m = 0.  The second moment of the mixture is at most twice that of either technique alone.
 *
 * Nothing else of the sample changes.  Non-parity: the oracle refuses it (JADE_ERR_UNSUPPORTED).  Maps above
 * JADE_ENV_IMPORTANCE_MAX_TEXELS are refused with it as with JADE_ENV_IMPORTANCE.  0 and 1 stay today's render in every kernel, bit
 * and counter; every other value of env_sampling stays JADE_ERR_INVALID.  It is not the default anywhere.  The device forms s, c and
 * m in fp32; DESIGN.md 3.16 derives how far m may then lie from this statement. */
#define JADE_ENV_MIXTURE 2
#define JADE_WALK_REFERENCE 0
#define JADE_WALK_EARLY_EXIT 1
/* JADE_WALK_EARLY_EXIT plus an occluder cache (ABI 7).  The reference tests a leaf's triangles iff the ray meets the leaf's box
 * and every ancestor's, and boxes are nested (jade_scene_create checks it; otherwise this mode walks as JADE_WALK_EARLY_EXIT), so
 * a yes/no query may look ANYWHERE in the tree first: whatever triangle it finds hit below its limit there, the reference's walk
 * finds too.  The module remembers, per (source triangle, kind of query), the subtrees in which the last such queries found their
 * answer and walks those before the root.  The frame, the rays and the samples are the reference's bit for bit, as with
 * JADE_WALK_EARLY_EXIT; nodes_visited / tris_tested count what was read and - the cache being shared by all waves of the device -
 * are not the same from run to run.  jade_stats.rays_cached counts the queries the cached subtrees answered.  Oracle: ignored. */
#define JADE_WALK_EARLY_EXIT_CACHED 2

/* Exact integer work counters; the oracle's and the HIP module's must be
 * equal for the same inputs.  One "ray" is one hitBVH query
 * (PathTrace.cu:795). */
typedef struct jade_stats {
  uint64_t rays_primary;   /* PathTrace.cu:1440 */
  uint64_t rays_secondary; /* every other hitBVH call site */
  uint64_t nodes_visited;  /* V: root + both children of each internal node popped */
  uint64_t tris_tested;    /* T: hitTriangle calls (source triangle excluded) */
  uint64_t shaded_hits;    /* H: pathTracing loop iterations (vertices shaded) */
  uint64_t samples;        /* pixels * spp rendered by this call */
  double kernel_ms;        /* device (or CPU wall) time inside the integrator */
  /* the dominant kernel alone (HIP: k_trace, timed with HIP events on its own
   * stream, summed over launches; oracle: 0) — feeds the roofline figure */
  double trace_ms;
  uint64_t trace_launches;
  /* rays_secondary by call site (exact; oracle == HIP): NEE shadow rays (PathTrace.cu:956, 1096, 1292),
   * environment-visibility rays (:980, 1123, 1316), indirect rays (:1003, 1150, 1339), mirror rays
   * (:1383), refraction rays (:1202, 1241) */
  uint64_t rays_shadow, rays_env, rays_indirect, rays_mirror, rays_refract;
  uint64_t host_syncs;     /* HIP: times the host waited for the device inside step/flush; oracle: 0 */
  /* HIP: rays (of the counts above) that were traced inside the fused first-pass kernel k_light, not by k_trace:
   * trace_ms / trace_launches cover the other rays only.  Oracle: 0. */
  uint64_t rays_inline;
  double light_ms;         /* HIP: device time of k_light (HIP events), summed over launches; oracle: 0 */
  /* HIP: the node records / triangle tests (of nodes_visited / tris_tested) that belong to the rays_inline rays, so that
   * SURVEY 8(d)'s algorithmic bytes 40 V + 36 T can be stated per kernel: k_trace's are the difference.  Oracle: 0. */
  uint64_t nodes_inline, tris_inline;
  /* HIP, JADE_WALK_EARLY_EXIT_CACHED: shadow / environment-visibility queries (of rays_shadow + rays_env) that the occluder cache
   * answered without a walk from the root.  Oracle and the other walks: 0. */
  uint64_t rays_cached;
  /* HIP (ABI 7): the last paths of a render - an active list of at most a few ten thousand records - are finished by ONE kernel,
   * k_tail, in which every wave shades and traces its own records; its rays (of the counts above), node records, triangle tests,
   * device time and launches.  trace_ms / trace_launches do not include them.  Oracle: 0. */
  uint64_t rays_tail, nodes_tail, tris_tail;
  double tail_ms;
  uint64_t tail_launches;
} jade_stats;

typedef struct jade_scene jade_scene; /* opaque */

int jade_abi_version(void);
const char* jade_backend_name(void);  /* "hip-gfx950" | "oracle-cpu" */
const char* jade_last_error(void);    /* thread-local text of the last failure */
int jade_device_count(int* n);

/* Validates the arrays (index ranges, BVH depth <= JADE_BVH_STACK_CAPACITY - 1)
 * and builds the backend's private copy.  Replaces PathTrace.cu:1618-1698. */
int jade_scene_create(const jade_scene_desc* desc, int device_id, jade_scene** out);
void jade_scene_destroy(jade_scene* scene);

/* Renders the caller's tiles.  Replaces PathTrace.cu:1704-1739 (constant
 * upload, RNG init, kernel launch, sync, D2H copy).
 *   out_rgb  nullable, width*height*3 floats: linear mean radiance before tone
 *            mapping (PathTrace.cu:1457), RGB, pixel (x, y) at 3*(y*width+x),
 *            y grows upward as in the reference (PathTrace.cu:1470).
 *   out_bgr8 nullable, width*height*3 bytes: ACES + gamma + BGR pack exactly
 *            as PathTrace.cu:1461-1473 (what save_image() writes).
 * Pixels of tiles this rank does not own are left untouched.
 * Synchronous; one render in flight per scene. */
int jade_render(jade_scene* scene, const jade_render_params* params, float* out_rgb,
                uint8_t* out_bgr8, jade_stats* stats);

/* Progressive form: the sample counter and the radiance sums persist on the
 * backend between calls, so N calls of spp samples equal one call of N*spp
 * (the reference's own running-mean preview, fshader_preview.fsh:402-403, is
 * the model).  begin() resets the accumulation; step() adds `spp` samples to
 * every owned pixel and leaves the results on the backend; resolve() writes
 * the mean so far.  jade_render == begin + step + resolve. */
int jade_render_begin(jade_scene* scene, const jade_render_params* params);
int jade_render_step(jade_scene* scene, int32_t spp, jade_stats* stats_accum);
int jade_render_resolve(jade_scene* scene, float* out_rgb, uint8_t* out_bgr8);
/* A backend may return from step() while the last, longest paths of that step
 * are still unfinished and carry them into the next step (samples are
 * independent work items, so the result is the same; what it saves is the
 * nearly empty passes at the end of every step).  flush() finishes them: after
 * it every sample requested so far is in the sums and in stats_accum.  Every
 * resolve variant flushes first; a caller only needs flush() to close a timed
 * region or to read final statistics without resolving. */
int jade_render_flush(jade_scene* scene, jade_stats* stats_accum);

/* Resolve with a choice of tone operator for out_bgr8 (out_rgb is always the
 * linear mean):
 *   JADE_TONEMAP_ACES      ACESToneMapping, PathTrace.cu:680-682 (what the CUDA
 *                          program writes; jade_render_resolve uses this)
 *   JADE_TONEMAP_REINHARD  toneMapping(c, limit) = c / (1 + luminance/limit),
 *                          PathTrace.cu:669-672 == shaders/pass3.fsh:8-18, the
 *                          GL preview's post pass (limit 1.5 there)
 * followed in both cases by gamma 1/2.2, x255, clamp, BGR (PathTrace.cu:1464-1473). */
#define JADE_TONEMAP_ACES 0
#define JADE_TONEMAP_REINHARD 1
int jade_render_resolve_ex(jade_scene* scene, int tonemap, float limit, float* out_rgb, uint8_t* out_bgr8);

/* Device-resident resolve for multi-GPU gathers (HIP backend only; the oracle
 * returns JADE_ERR_UNSUPPORTED).  Writes this rank's tiles compactly into
 * device memory: tile t (t-th owned tile in increasing row-major id) occupies
 * floats [t*768, (t+1)*768) as 16x16 RGB rows.  `dev_tiles` must hold
 * jade_owned_tile_count()*768 floats.  `stream` is a hipStream_t (0 = null
 * stream).  Out-of-image pixels of edge tiles are written as 0. */
int jade_render_resolve_tiles_device(jade_scene* scene, float* dev_tiles, void* stream);
int jade_owned_tile_count(int32_t width, int32_t height, int32_t tile_rank, int32_t tile_nranks);

/* One frame on several GPUs from ONE process.  scenes[i] must have been created
 * on the device that renders share i (jade_scene_create(desc, device_i, ..)); tiles are dealt
 * (tx + ty) % ndev exactly as with tile_rank / tile_nranks, every device renders its share
 * concurrently (one host thread per device), then the device scenes[0] lives on collects the
 * compact tile buffers with ONE RCCL gather over xGMI (ncclCommInitAll over the devices + grouped
 * ncclSend / ncclRecv; librccl is loaded on first use) and the frame is assembled and tone-mapped
 * once.  If the same device appears more than once (a one-GPU rehearsal of the partition) the
 * shares are copied device-to-device instead: RCCL cannot put two ranks on one device.
 * The result is bit-identical to jade_render on one device.  params->tile_rank / tile_nranks /
 * device_id are ignored.  (The one-process-per-GPU form with torch.distributed's RCCL gather is
 * what bench.py and jaderaytracerendering_amd/distributed.py use.) */
int jade_render_multi(jade_scene* const* scenes, int ndev, const jade_render_params* params,
                      float* out_rgb, uint8_t* out_bgr8, jade_stats* stats);

/* What a backend holds for the render begun last (after jade_render_begin; values are the backend's own choices and
 * never change a result - jade_render_params.max_state_bytes / .spp are what a caller steers them with):
 *   JADE_Q_RECORDS_PER_PIXEL  HIP: samples of one pixel in flight at once (a power of two <= JADE_SAMPLE_LANES); oracle: 1
 *   JADE_Q_STATE_BYTES        HIP: device bytes held for path records, ray queue, lists and partial sums; oracle: host
 *                             bytes of its partial sums
 *   JADE_Q_SUM_LANES          partial sums kept per pixel: min(JADE_SAMPLE_LANES, the announced spp rounded up to a power
 *                             of two); grows by itself if steps add more samples than were announced
 * (The reference has no counterpart: its one kernel keeps a pixel's whole state in registers, PathTrace.cu:1418-1474.) */
#define JADE_Q_RECORDS_PER_PIXEL 0
#define JADE_Q_STATE_BYTES 1
#define JADE_Q_SUM_LANES 2
int jade_render_query(jade_scene* scene, int what, int64_t* value);

/* Single-query entry point used by the parity tests: traces `n` rays through
 * the scene's BVH with hitBVH semantics (PathTrace.cu:795-859).
 *   origins/dirs: n*3 floats; skip: n source-triangle indices (-1 = none)
 *   hit_index: n (-1 on miss); hit_dist: n; hit_point: n*3
 *   stats: nodes_visited / tris_tested / rays_secondary are accumulated */
int jade_trace_rays(jade_scene* scene, int32_t n, const float* origins, const float* dirs,
                    const int32_t* skip, int32_t* hit_index, float* hit_dist, float* hit_point,
                    jade_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* JADE_RT_H */
