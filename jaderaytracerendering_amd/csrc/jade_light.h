// jade_light.h — the first pass of a step, fused: k_light_packet and k_light, with the kernels that close their hand-over list
// (k_heavy_scan, k_heavy_pack) and k_packet_rays, the packet walk on raw rays.  Part of jade_hip.hip's translation unit.
//
// Both first-pass kernels sit at their 128-VGPR limit, and what the compiler makes of either answers almost any change of its text:
// k_light's spill count moved between 80 and 112 bytes, k_light_packet took 0.6 to 3 % longer (profiles/first_pass_refactor_bench.json).
// So they share the pieces that leave their instructions the parent's - vertex_from_primary and store_ctx (jade_shade.h),
// light_hand_over and light_flush below - and each KEEPS ITS OWN TEXT of the rest, statement for statement the other's where the
// comments say so: the record prologue, the advance step with the camera ray (film_point's and next_live_sample's statements,
// jade_device.h / jade_shade.h), the finished sample (add_sample's), the fold and the header store.  Through shared functions for
// those k_light_packet compiled to other instructions and ran slower, whatever the form.  A change to one of these
// pieces - a lens form of the camera ray - is made in both kernels and in the helper that states it;
// tests/test_gpu_first_pass.py and test_result_independent_of_shade_schedule hold the copies to one another, bit for bit.
// The two texts differ in three ways only: k_light_packet saves rng_vertex before begin_bounce_lean and restores it when a packet
// is given up (k_light never gives a ray up); it sets st = ST_IDLE at the fold, because it picks the lanes to advance by their
// stage, where k_light advances right behind the fold; and rp.d starts as (0, 0, 1) there and (0, 0, 0) in k_light - no result
// depends on either value (k_light reads rp.d only behind a set_dir; packet_trace puts every lane's direction through 1 / d and
// normalize and discards what those make of a lane without a ray).
#pragma once
#include "jade_shade.h"
#include "jade_trace.h"

#if JADE_TRACE_PROFILE
__device__ unsigned long long g_packet_prof[PKL_N];  // development profile of k_light_packet: shader clocks per piece of the loop, summed over waves
#endif

// ---- the pieces both kernels call

// Hand-over: the records with `defer` are appended to this wave's region of the list (every lane of the wave calls it)
static __device__ __forceinline__ void light_hand_over(bool defer, int p, uint32_t* my_region, uint32_t& n_deferred) {
  const unsigned long long dm = __ballot(defer);
  if (defer) my_region[n_deferred + lanes_below(dm)] = (uint32_t)p;
  n_deferred += (uint32_t)__popcll(dm);
}
// Work counters: per wave into LDS, then one set of atomics per block (as shade_tail), and V / T as k_trace (vcnt, tcnt: this lane's
// node and triangle counts).  Every thread of the block calls it.  n_packets / n_given_up: packets started / given up, wave-uniform
// (k_light_packet; JADE_LOG_PASSES)
static __device__ __forceinline__ void light_flush(DevCounters* ctr, uint32_t (&sh_ctr)[JADE_TRACE_BLOCK / 64][8], const ShadeCtx& c, uint32_t n_mirror, uint32_t vcnt,
                                                   uint32_t tcnt, uint32_t n_packets = 0, uint32_t n_given_up = 0) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t s0 = (uint32_t)wave_sum_u32(c.c_primary), s2 = (uint32_t)wave_sum_u32(c.c_shaded), s3 = (uint32_t)wave_sum_u32(c.c_samples);
  const unsigned long long s6 = wave_sum_u32(n_mirror);
  const unsigned long long sv = wave_sum_u32(vcnt), stt = wave_sum_u32(tcnt);
  if (lane == 0) {
    sh_ctr[w][0] = s0;
    sh_ctr[w][1] = 0;
    sh_ctr[w][2] = s2;
    sh_ctr[w][3] = s3;
    sh_ctr[w][4] = 0;
    sh_ctr[w][5] = 0;
    sh_ctr[w][6] = (uint32_t)s6;
    sh_ctr[w][7] = 0;
    DevCounters* cs = ctr + (blockIdx.x % JADE_CTR_SHARDS);
    if (sv) atomicAdd(&cs->nodes_visited, sv);
    if (stt) atomicAdd(&cs->tris_tested, stt);
    if (sv) atomicAdd(&cs->nodes_inline, sv);
    if (stt) atomicAdd(&cs->tris_inline, stt);
    if (s0 + s6) atomicAdd(&cs->rays_inline, (unsigned long long)s0 + s6);  // every camera and mirror ray of the pass was traced here
    if (n_packets) atomicAdd(&cs->pad[0], (unsigned long long)n_packets);
    if (n_given_up) atomicAdd(&cs->pad[1], (unsigned long long)n_given_up);
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    unsigned long long t = 0;
    for (int i = 0; i < JADE_TRACE_BLOCK / 64; ++i) t += sh_ctr[i][threadIdx.x];
    DevCounters* cs = ctr + (blockIdx.x % JADE_CTR_SHARDS);
    // word of DevCounters: primary 0, shadow 1, shaded 4, samples 5, env / indirect / mirror / refract 8-11
    const int i = (int)threadIdx.x, wordi = i < 2 ? i : i < 4 ? i + 2 : i + 4;
    if (t) atomicAdd(reinterpret_cast<unsigned long long*>(cs) + wordi, t);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// k_light: the first pass of a step, fused.  Most samples of most frames are LIGHT: the camera ray misses (sky), or it
// meets an emitter, or a pure mirror whose reflected ray then misses (the floor).  Run as shade / trace passes, such a
// sample crosses memory six times (camera ray out, its result back, mirror ray out, ...) for a handful of arithmetic:
// k_shade_lean was bound by those bytes (3.5 TB/s of HBM, 15 % of a step) and the rays' records by their round trip
// through the queue.  Here a record keeps its light samples in registers: it generates the camera ray, traces it IN
// THIS KERNEL (the same node / triangle steps as k_trace, a wave's rays side by side until all have ended - camera and
// floor-mirror rays of neighbouring pixels are coherent), folds the result in, follows a pure mirror, adds the finished
// sample to its partial sum and starts the next one, until it runs out of samples or meets a surface the light path
// cannot shade (jade, diffuse, glass).  Then it parks the path exactly where k_shade_lean would have (ST_VERTEX, context
// stored) and hands the record to k_shade through the same list.  Statements, draw order and sums are those of
// shade_record<true> + k_trace, so every bit of the result is the same (test_result_independent_of_shade_schedule).
// ---------------------------------------------------------------------------------------------------------------
#ifndef JADE_LIGHT_WAVES
#define JADE_LIGHT_WAVES 4
#endif
#ifndef JADE_LIGHT_REFILL_MIN
#define JADE_LIGHT_REFILL_MIN 32 /* waiting lanes of a wave that trigger k_light's shading block */
#endif
__global__ __launch_bounds__(JADE_TRACE_BLOCK, JADE_LIGHT_WAVES) void k_light(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                                                            uint32_t target_spp, uint32_t* heavy_regions, uint32_t region_cap,
                                                                            uint32_t* wave_counts, uint32_t* spill, DevCounters* ctr) {
  __shared__ __attribute__((aligned(JADE_COLS_ALIGN))) uint32_t lds_cols[LW_END * JADE_TRACE_BLOCK];
  __shared__ uint32_t sh_ctr[JADE_TRACE_BLOCK / 64][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  LdsStack stk;
  stk.lds = lds_cols + threadIdx.x;
  stk.col = lds_addr_of(stk.lds);
  stk.spill = spill + (blockIdx.x * blockDim.x + threadIdx.x);
  stk.stride_spill = gridDim.x * blockDim.x;
  stk.top = nullptr;
  stk.top_k = 0;
#if JADE_LDS_TOP_NODES > 0
  __shared__ float4 lds_top[4 * JADE_LDS_TOP_NODES];
  {
    const uint32_t k = S.top_k;
    for (uint32_t i = threadIdx.x; i < 4u * k; i += JADE_TRACE_BLOCK) lds_top[(i & 3u) * JADE_LDS_TOP_NODES + (i >> 2)] = S.nodes[i];
    __syncthreads();
    stk.top = lds_top;
    stk.top_k = k;
  }
#endif
  const int npix = P.npix;
  const size_t sn = (size_t)P.sum_lanes * (size_t)P.npx;
  uint32_t vcnt = 0, tcnt = 0, n_mirror = 0;
  ShadeCtx c;
  c.n_emit_rays = 0;
  c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
  // records are dealt to the resident blocks in chunks of one block (a persistent grid: the LDS copy of the tree top is
  // made once per block, not once per 256 records)
  // (per WAVE: a wave that is through its 64 records takes its next 64 at once - no barrier, no shared counter; the
  // records it hands to k_shade go into a region of the list that is this wave's own, compacted by k_heavy_pack)
  const uint32_t wave_id = blockIdx.x * (JADE_TRACE_BLOCK / 64) + (uint32_t)w;
  uint32_t* const my_region = heavy_regions + (size_t)wave_id * region_cap;
  uint32_t n_deferred = 0;
  for (size_t base = (size_t)wave_id * 64; base < (size_t)npix; base += (size_t)gridDim.x * JADE_TRACE_BLOCK) {
    const size_t p64 = base + (size_t)lane;
    const bool have = p64 < (size_t)npix;
    const int p = have ? (int)p64 : 0;
    const uint4 hdr0 = P.hdr[p];
    const uint32_t word = hdr0.z;
    uint32_t st = have ? (word & 255u) : (uint32_t)ST_INVALID;
    const uint32_t rec_m = (uint32_t)p / (uint32_t)P.npx;
    const int home_pix = (int)((uint32_t)p - rec_m * (uint32_t)P.npx);
    const int tid0 = tile_ids[home_pix >> 8];
    uint32_t done = hdr0.y;
    bool defer = false;  // hand the record to k_shade
    // a record that is in the middle of a path (carried over from the last step, its rays traced and their results
    // waiting in memory) goes to k_shade untouched, as k_shade_lean does; an idle one is this kernel's to run
    bool mine = st == ST_IDLE;
    const bool untouched = have && st != ST_IDLE && st != ST_INVALID;
    if (untouched) defer = true;
    c.rng = hdr0.x;
    c.depth = 0;
    c.flags = 0;
    c.thr = jv(1, 1, 1);
    c.acc = jv(0, 0, 0);
    c.le = jv(0, 0, 0);
    c.obj = 0;
    c.src = jv(0, 0, 0);
    c.out = jv(0, 0, 0);
    RegPx rp;
    rp.d = jv(0, 0, 0);
    rp.o = jv(0, 0, 0);
    rp.hp = jv(0, 0, 0);
    rp.h = -1;
    rp.sk = -1;
    bool finished = false;
    jvec3 color = jv(0, 0, 0), l_final = jv(0, 0, 0);
    // A lane is tracing (`active`), or waits to be shaded: its ray's result folded in and the next ray set up.  Shading
    // runs for >= JADE_LIGHT_REFILL_MIN waiting lanes at a time (or when nothing is being traced): it is k_trace's refill, with
    // the next ray coming from the lane's own path instead of from a queue.
    bool active = false;   // a ray in flight
    bool pending = false;  // its result has not been folded in yet
    RayState r;
    ray_clear(r, stk);
    for (;;) {
      const unsigned long long tracing = __ballot(active);
      const int n_wait = __popcll(__ballot(mine && !active));
      if (tracing == 0ull && n_wait == 0) break;  // every lane is out of samples or parked
      if (n_wait >= JADE_LIGHT_REFILL_MIN || tracing == 0ull) {
        if (mine && !active) {
          // ---- fold the result in (shade_record's part (a))
          if (pending) {
            pending = false;
            rp.h = ray_best_index(stk);
            if (rp.h >= 0) rp.hp = ray_hit_point(stk);
            if (st == ST_PRIMARY) {
              if (rp.h < 0) {
                color = sample_hdr(S, rp.d);  // PathTrace.cu:1443-1445
                finished = true;
              } else {
                vertex_from_primary(S, c, rp.h, rp.hp, rp.d);
                st = ST_VERTEX;
              }
            } else {  // ST_MIRROR
              c.stage = ST_MIRROR;
              const int rr = consume_mirror(S, rp, c, &l_final);
              if (rr == CONSUME_VERTEX) {
                st = ST_VERTEX;
              } else {
                color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
                finished = true;
              }
            }
          }
          // ---- advance until this lane has a ray to trace, is out of samples, or parks (part (b))
          bool ray = false;
          for (;;) {
            if (finished) {
              const NextSample cs = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);  // the sample that just ended
              const size_t si = (size_t)(cs.sidx % JADE_SAMPLE_LANES) * (size_t)P.npx + (size_t)cs.pixel;
              st3w(P.sum, sn, si, jv_add(ld3w(P.sum, sn, si), color));
              done += 1;
              c.c_samples += 1;
              finished = false;
              st = ST_IDLE;
            }
            if (st == ST_VERTEX) {
              if (!lean_can_shade(shade_tri(S, c.obj).m)) {  // jade / diffuse / glass: k_shade continues from here
                defer = true;
                mine = false;
                break;
              }
              if (begin_bounce_lean(S, rp, c, &l_final)) {  // the mirror ray is in rp
                n_mirror += 1;
                st = ST_MIRROR;
                ray = true;
                break;
              }
              color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
              finished = true;
              continue;
            }
            // ST_IDLE: the next sample of this record; samples of out-of-image pixels (edge tiles) are skipped
            int x, y;
            NextSample ns = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
            while (ns.sidx < target_spp && !pixel_xy_t(R, ns.pixel == home_pix ? tid0 : tile_ids[ns.pixel >> 8], ns.pixel, &x, &y)) {
              done += 1;
              ns = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
            }
            if (ns.sidx >= target_spp) {  // nothing left for this record in this step
              mine = false;
              break;
            }
            // camera ray, PathTrace.cu:1428-1437 (the statements of shade_record)
            c.rng = jade_rng_seed((uint32_t)x, (uint32_t)y, R.frame + ns.sidx);
            float fx = (float)x + jade_rand(&c.rng);
            double lo = -1.0 + R.two_over_w * ((double)fx - 0.5);
            float left_offset = (float)(lo * R.aspect);
            float fy = (float)y + jade_rand(&c.rng);
            float up_offset = (float)(-1.0 + R.two_over_h * ((double)fy - 0.5));
            jvec3 dir = jade_transform(jv(left_offset, up_offset, -1.5f), 0.0f, R.cam);
            dir = jv_normalize(dir);
            rp.set_origin(jv(P.eye[0], P.eye[1], P.eye[2]), JADE_SKIP_CAMERA);
            rp.set_dir(0, dir);
            c.c_primary += 1;
            c.depth = 0;
            c.flags = 0;
            st = ST_PRIMARY;
            ray = true;
            break;
          }
          if (ray) {
            ray_begin(r, stk, S, rp.o, rp.d, rp.sk);
            vcnt += 1;  // the root record
            active = true;
            pending = true;
          }
        }
        if (__ballot(active) == 0ull) continue;  // (every lane went out or parked: the loop ends at its top)
      }
      // ---- one kind of work for every tracing lane that has some (hitBVH, PathTrace.cu:795-859).  The lane tests the leaves
      // of its own ray here (a FIFO per lane, jade_trace.h): camera and floor-mirror rays of neighbouring pixels are short and
      // walk side by side, and k_trace's wave-wide queue of leaves costs this kernel more than it saves (282 vs 238 ms per step)
      {
        const bool cw = active && ray_can_walk(r), ct = active && ray_can_test(r);
        const int nw = __popcll(__ballot(cw)), nt = __popcll(__ballot(ct));
        if (JADE_COST_TRI * nw >= JADE_COST_NODE * nt) {
          if (S.general_walk || __ballot(active && (int32_t)r.skipx < 0) != 0ull) {
#pragma nounroll
            for (int rep = 0; rep < JADE_STEPS_PER_PICK; ++rep)
              if (active && ray_can_walk(r)) ray_step_node_s<true>(r, S, stk, vcnt);
          } else {
#pragma nounroll
            for (int rep = 0; rep < JADE_STEPS_PER_PICK; ++rep)
              if (active && ray_can_walk(r)) ray_step_node_s<false>(r, S, stk, vcnt);
          }
        } else {
#pragma nounroll
          for (int rep = 0; rep < JADE_STEPS_PER_PICK; ++rep)
            if (active && ray_can_test(r)) ray_step_tri_s(r, S, stk, tcnt);
        }
        if (active && ray_done(r)) active = false;  // its result stays in the LDS column until the lane is shaded
      }
    }
    // ---- store what the next kernel needs
    if (have && st != ST_INVALID && !untouched) {  // (a carried-over record was not touched)
      P.hdr[p] = make_uint4(c.rng, done, st == ST_VERTEX ? ST_VERTEX | (c.depth << 8) | (c.flags << 16) : (uint32_t)ST_IDLE, 0u);
      if (st == ST_VERTEX) {  // parked: the path context, as shade_record stores it for this stage
        store_ctx(P, p, c);
      }
    }
    light_hand_over(defer, p, my_region, n_deferred);
  }
  if (lane == 0) wave_counts[wave_id] = n_deferred;
  light_flush(ctr, sh_ctr, c, n_mirror, vcnt, tcnt);
}

// ---------------------------------------------------------------------------------------------------------------
// k_light_packet: k_light with the wave's rays walked together (jade_trace.h, "Packet form").  What k_light traces - camera
// rays of 64 neighbouring pixels, their reflections off the mirror floor - is as coherent as rays get, and its time is the
// traversal (two thirds of its instructions): one scalar cursor and stack per wave, the node and pair records through
// scalar loads, no per-lane stack / FIFO / column in LDS.  A wave alternates two phases so that a packet holds one kind of
// ray: all its lanes' camera rays, then the mirror rays those produced.  Shading statements, draw order and sums are those
// of k_light (and of shade_record<true> + k_trace): the same bits (test_result_independent_of_shade_schedule).
// ---------------------------------------------------------------------------------------------------------------
#ifndef JADE_PACKET_WAVES
#define JADE_PACKET_WAVES 4 /* 128 VGPRs; at 5 (96 VGPRs, 168 bytes of scratch) the kernel took 228 instead of 191 ms per step on C3 */
#endif
__global__ __launch_bounds__(JADE_TRACE_BLOCK, JADE_PACKET_WAVES) void k_light_packet(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                                                                   uint32_t target_spp, uint32_t* heavy_regions, uint32_t region_cap,
                                                                                   uint32_t* wave_counts, DevCounters* ctr, uint32_t budget) {
  __shared__ __attribute__((aligned(16))) uint32_t lds_stack[JADE_TRACE_BLOCK / 64][8 * (JADE_PACKET_MAX_DEPTH + 1)];
  __shared__ uint32_t sh_ctr[JADE_TRACE_BLOCK / 64][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t stack = lds_addr_of(&lds_stack[w][0]);
  uint32_t n_given_up = 0, n_packets = 0;
  TraceProf pr;
#if JADE_TRACE_PROFILE
  __shared__ __attribute__((aligned(8))) unsigned long long lds_pprof[JADE_TRACE_BLOCK / 64][PKL_N > PL_N ? PKL_N : PL_N];
  pr.begin(lds_addr_of(reinterpret_cast<const uint32_t*>(&lds_pprof[w][0])), lane);
#endif
  const int npix = P.npix;
  const size_t sn = (size_t)P.sum_lanes * (size_t)P.npx;
  uint32_t vcnt = 0, tcnt = 0, n_mirror = 0;
  ShadeCtx c;
  c.n_emit_rays = 0;
  c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
  const uint32_t wave_id = blockIdx.x * (JADE_TRACE_BLOCK / 64) + (uint32_t)w;
  uint32_t* const my_region = heavy_regions + (size_t)wave_id * region_cap;
  uint32_t n_deferred = 0;
  for (size_t base = (size_t)wave_id * 64; base < (size_t)npix; base += (size_t)gridDim.x * JADE_TRACE_BLOCK) {
    const size_t p64 = base + (size_t)lane;
    const bool have = p64 < (size_t)npix;
    const int p = have ? (int)p64 : 0;
    const uint4 hdr0 = P.hdr[p];
    const uint32_t word = hdr0.z;
    uint32_t st = have ? (word & 255u) : (uint32_t)ST_INVALID;
    const uint32_t rec_m = (uint32_t)p / (uint32_t)P.npx;
    const int home_pix = (int)((uint32_t)p - rec_m * (uint32_t)P.npx);
    const int tid0 = tile_ids[home_pix >> 8];
    uint32_t done = hdr0.y;
    bool defer = false;
    bool mine = st == ST_IDLE;  // (a record in the middle of a carried-over path goes to k_shade untouched, as in k_light)
    const bool untouched = have && st != ST_IDLE && st != ST_INVALID;
    if (untouched) defer = true;
    c.rng = hdr0.x;
    c.depth = 0;
    c.flags = 0;
    c.thr = jv(1, 1, 1);
    c.acc = jv(0, 0, 0);
    c.le = jv(0, 0, 0);
    c.obj = 0;
    c.src = jv(0, 0, 0);
    c.out = jv(0, 0, 0);
    RegPx rp;
    rp.d = jv(0, 0, 1);
    rp.o = jv(0, 0, 0);
    rp.hp = jv(0, 0, 0);
    rp.h = -1;
    rp.sk = -1;
    bool finished = false;
    jvec3 color = jv(0, 0, 0), l_final = jv(0, 0, 0);
    uint32_t rng_vertex = 0;
    for (;;) {
      // ---- every lane without a ray advances until it has one (camera or mirror), is out of samples, or parks
      if (mine && st != ST_PRIMARY && st != ST_MIRROR) {
        for (;;) {
          if (finished) {
            const NextSample cs = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);  // the sample that just ended
            const size_t si = (size_t)(cs.sidx % JADE_SAMPLE_LANES) * (size_t)P.npx + (size_t)cs.pixel;
            st3w(P.sum, sn, si, jv_add(ld3w(P.sum, sn, si), color));
            done += 1;
            c.c_samples += 1;
            finished = false;
            st = ST_IDLE;
          }
          if (st == ST_VERTEX) {
            if (!lean_can_shade(shade_tri(S, c.obj).m)) {  // jade / diffuse / glass: k_shade continues from here
              defer = true;
              mine = false;
              break;
            }
            rng_vertex = c.rng;  // (a mirror packet that is given up goes back to this vertex)
            if (begin_bounce_lean(S, rp, c, &l_final)) {  // the mirror ray is in rp
              n_mirror += 1;
              st = ST_MIRROR;
              break;
            }
            color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
            finished = true;
            continue;
          }
          // ST_IDLE: the next sample of this record; samples of out-of-image pixels (edge tiles) are skipped
          int x, y;
          NextSample ns = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
          while (ns.sidx < target_spp && !pixel_xy_t(R, ns.pixel == home_pix ? tid0 : tile_ids[ns.pixel >> 8], ns.pixel, &x, &y)) {
            done += 1;
            ns = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
          }
          if (ns.sidx >= target_spp) {  // nothing left for this record in this step
            mine = false;
            break;
          }
          // camera ray, PathTrace.cu:1428-1437 (the statements of shade_record)
          c.rng = jade_rng_seed((uint32_t)x, (uint32_t)y, R.frame + ns.sidx);
          float fx = (float)x + jade_rand(&c.rng);
          double lo = -1.0 + R.two_over_w * ((double)fx - 0.5);
          float left_offset = (float)(lo * R.aspect);
          float fy = (float)y + jade_rand(&c.rng);
          float up_offset = (float)(-1.0 + R.two_over_h * ((double)fy - 0.5));
          jvec3 dir = jade_transform(jv(left_offset, up_offset, -1.5f), 0.0f, R.cam);
          dir = jv_normalize(dir);
          rp.set_origin(jv(P.eye[0], P.eye[1], P.eye[2]), JADE_SKIP_CAMERA);
          rp.set_dir(0, dir);
          c.c_primary += 1;
          c.depth = 0;
          c.flags = 0;
          st = ST_PRIMARY;
          break;
        }
      }
      const bool cam = mine && st == ST_PRIMARY, mir = mine && st == ST_MIRROR;
      const unsigned long long mc = __ballot(cam), mm = __ballot(mir);
      PROF_DRAIN();
      PROF_LAP(pr, PKL_ADVANCE);  // (and the fold of the packet before)
      if ((mc | mm) == 0ull) break;  // every lane is out of samples or parked
      // ---- one packet of ONE kind of ray, the kind more lanes hold (a lane with the other kind waits: a wave whose pixels
      // all see the floor alternates camera packets and mirror packets of 64 rays each)
      const bool go = __popcll(mc) >= __popcll(mm) ? cam : mir;
      bool whole = true;
      {
        const jvec3 o = rp.o, d = rp.d;
        const bool exact = !(finite_f(1.0f / d.x) && finite_f(1.0f / d.y) && finite_f(1.0f / d.z)) || !finite_f(o.x) || !finite_f(o.y) || !finite_f(o.z);
        PacketBest best;
        uint32_t pv = 0, pt = 0;  // the packet's counts: kept only if it runs to the end
        const bool general = S.general_walk || __ballot(go && exact) != 0ull;
        whole = general ? packet_trace<true>(S, stack, lane, go, o, d, rp.sk, pv, pt, best, budget, pr)
                        : packet_trace<false>(S, stack, lane, go, o, d, rp.sk, pv, pt, best, budget, pr);
        n_packets += 1;
        PROF_COUNT(pr, PKC_PACKETS, 1);
        PROF_COUNT(pr, PKC_GIVEN_UP, whole ? 0ull : 1ull);
        PROF_COUNT(pr, PKC_LANES, (unsigned long long)__popcll(__ballot(go)));
        if (whole) {
          if (go) {
            vcnt += pv + 1u;  // + the root record
            tcnt += pt;
            rp.h = (int32_t)best.index;
            rp.hp = best.point;
          }
        } else if (go) {
          // ---- given up (the rays fan out, e.g. into the statue): these lanes go back to where the ray came from and hand
          // their records to the wavefront passes, whose per-lane walk is the right tool for such rays - a camera ray back to
          // "sample not started" (its stream is seeded per sample), a mirror ray back to the vertex it left, with the random
          // state it had there.  k_shade continues from either (shade_record); nothing of the partial walk is kept.
          if (st == ST_PRIMARY) {
            c.c_primary -= 1;
            st = ST_IDLE;
          } else {
            c.rng = rng_vertex;
            c.c_shaded -= 1;
            n_mirror -= 1;
            st = ST_VERTEX;
          }
          defer = true;
          mine = false;
        }
      }
      if (!whole) {
        n_given_up += 1;
        continue;
      }
      // ---- fold the result in (shade_record's part (a))
      PROF_DRAIN();
      PROF_LAP(pr, PKL_POP);  // (what is left of the walk after its last lap)
      if (go) {
        if (st == ST_PRIMARY) {
          if (rp.h < 0) {
            color = sample_hdr(S, rp.d);  // PathTrace.cu:1443-1445
            finished = true;
            st = ST_IDLE;
          } else {
            vertex_from_primary(S, c, rp.h, rp.hp, rp.d);
            st = ST_VERTEX;
          }
        } else {  // ST_MIRROR
          c.stage = ST_MIRROR;
          const int rr = consume_mirror(S, rp, c, &l_final);
          if (rr == CONSUME_VERTEX) {
            st = ST_VERTEX;
          } else {
            color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
            finished = true;
            st = ST_IDLE;
          }
        }
      }
      PROF_DRAIN();
      PROF_LAP(pr, PKL_FOLD);
    }
    // ---- store what the next kernel needs
    if (have && st != ST_INVALID && !untouched) {  // (a carried-over record was not touched)
      P.hdr[p] = make_uint4(c.rng, done, st == ST_VERTEX ? ST_VERTEX | (c.depth << 8) | (c.flags << 16) : (uint32_t)ST_IDLE, 0u);
      if (st == ST_VERTEX) {  // parked: the path context, as shade_record stores it for this stage
        store_ctx(P, p, c);
      }
    }
    light_hand_over(defer, p, my_region, n_deferred);
    PROF_DRAIN();
    PROF_LAP(pr, PKL_STORE);
  }
#if JADE_TRACE_PROFILE
  PROF_DRAIN();
  if (lane < PKL_N) {
    const unsigned long long v = pr.get(lane);
    if (v) atomicAdd(&g_packet_prof[lane], v);
  }
#endif
  if (lane == 0) wave_counts[wave_id] = n_deferred;
  light_flush(ctr, sh_ctr, c, n_mirror, vcnt, tcnt, n_packets, n_given_up);
}

// Development / tests: packet_trace on raw rays, 64 per wave in the order given; per-ray hit, distance, point, V and T.
__global__ __launch_bounds__(JADE_TRACE_BLOCK) void k_packet_rays(DevScene S, int n, const float* origins, const float* dirs, const int32_t* skip, int32_t* hit,
                                                                 float* dist, float* point, uint32_t* v_out, uint32_t* t_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds_stack[JADE_TRACE_BLOCK / 64][8 * (JADE_PACKET_MAX_DEPTH + 1)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool have = i < n;
  const int k = have ? i : 0;
  const jvec3 o = jv(origins[3 * k], origins[3 * k + 1], origins[3 * k + 2]), d = jv(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
  const bool exact = !(finite_f(1.0f / d.x) && finite_f(1.0f / d.y) && finite_f(1.0f / d.z)) || !finite_f(o.x) || !finite_f(o.y) || !finite_f(o.z);
  uint32_t vcnt = have ? 1u : 0u, tcnt = 0;
  PacketBest best;
  bool whole;
  TraceProf pr;
#if JADE_TRACE_PROFILE
  __shared__ __attribute__((aligned(8))) unsigned long long lds_pprof[JADE_TRACE_BLOCK / 64][PKL_N > PL_N ? PKL_N : PL_N];
  pr.begin(lds_addr_of(reinterpret_cast<const uint32_t*>(&lds_pprof[w][0])), lane);
#endif
  if (S.general_walk || __ballot(have && exact) != 0ull) whole = packet_trace<true>(S, lds_addr_of(&lds_stack[w][0]), lane, have, o, d, skip[k], vcnt, tcnt, best, 0xffffffffu, pr);
  else whole = packet_trace<false>(S, lds_addr_of(&lds_stack[w][0]), lane, have, o, d, skip[k], vcnt, tcnt, best, 0xffffffffu, pr);
  if (have && !whole) {  // the packet was given up (no budget here: two leaves tied for some ray's best distance) - k_light_packet hands such rays to the wavefront passes
    hit[i] = -3;
    dist[i] = 0.0f;
    point[3 * i] = point[3 * i + 1] = point[3 * i + 2] = 0.0f;
    v_out[i] = t_out[i] = 0u;
  } else if (have) {
    hit[i] = (int32_t)best.index;
    dist[i] = best.dist;
    point[3 * i] = best.point.x;
    point[3 * i + 1] = best.point.y;
    point[3 * i + 2] = best.point.z;
    v_out[i] = vcnt;
    t_out[i] = tcnt;
  }
}

// Hand-over list of k_light: every wave filled a region of its own; one block turns the per-wave counts into offsets
// (and the total into qc->heavy, where k_shade reads it), then each region is copied to its place in the dense list.
__global__ __launch_bounds__(1024) void k_heavy_scan(uint32_t* wave_counts, uint32_t n_waves, QueueCtl* qc) {
  __shared__ uint32_t sh[1024];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n_waves; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_waves ? wave_counts[i] : 0u;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
      const uint32_t t = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    const uint32_t incl = sh[threadIdx.x], c0 = carry;
    if (i < n_waves) wave_counts[n_waves + i] = c0 + incl - v;  // exclusive offsets live behind the counts
    __syncthreads();
    if (threadIdx.x == 1023) carry = c0 + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) qc->heavy = carry;
}

__global__ void k_heavy_pack(const uint32_t* heavy_regions, uint32_t region_cap, const uint32_t* wave_counts, uint32_t n_waves, uint32_t* dense) {
  const uint32_t wv = blockIdx.x;
  const uint32_t n = wave_counts[wv], off = wave_counts[n_waves + wv];
  const uint32_t* src = heavy_regions + (size_t)wv * region_cap;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dense[off + i] = src[i];
}
