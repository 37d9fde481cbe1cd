// jade_hip.hip — libjade_hip.so: the jade_rt.h C ABI on MI355X (gfx950).
//
// Replaces PathTrace.cu:1618-1741 (upload, constants, RNG init, the single
// render_pixel launch, sync, download).  Kernel structure (one HIP stream):
//
//   k_init          resets the path records (the partial sums are cleared with the allocation)
//   k_light_packet  a step's FIRST pass, fused: camera rays, the sky, emitters and pure mirrors traced and shaded in one
//                   kernel, a wave's 64 rays walked together as a packet (jade_trace.h); records that meet jade / diffuse /
//                   glass, or whose packet fans out, are handed to k_shade.  k_light: the same pass, one lane per ray
//                   (trees deeper than 63, frames the statue fills); k_heavy_scan / k_heavy_pack close the hand-over list.
//                   These four and k_packet_rays live in jade_light.h
//   k_shade         every branch of pathTracing, over the hand-over list, then over the active list: folds last pass's hit
//                   results into the path, starts the next sample when a path ends, emits the next bounce's rays into a
//                   compacted queue (wave prefix sums + one 64-bit atomic per block)
//   k_ray_keys      (+ rocPRIM pairs sort) orders the queue for scenes whose tree does not fit the L2
//   k_trace         persistent workgroups claim chunks of the queue and run the BVH traversal (jade_trace.h) - the
//                   dominant kernel.  With jade_render_params.walk = JADE_WALK_EARLY_EXIT a shadow / environment-visibility
//                   walk ends at the first recorded hit that settles what the integrator asks of it (the limit k_shade puts
//                   beside the ray); k_trace_wide: the same kernel visiting four grandchildren per node, launched instead for
//                   such renders on trees that do not fit the L2
//   k_resolve       adds the partial sums; mean, ACES, gamma, BGR8 pack (PathTrace.cu:1457-1473)
//   k_arm / k_shade_lean  list the records with work / shade light samples over all records: the schedules without the
//                   fused pass (flushes, JADE_FUSED=0)
//   k_shade_mode<M> / k_shade_lean_mode<M>  k_shade / k_shade_lean of a non-parity render mode M (ShadeMode, jade_runtime.h: environment
//                   importance or the environment mixture, lens, shutter, one-light, cosine bounces, MIS, passes), one instantiation per built mode; k_shade,
//                   k_shade_binned and k_shade_lean themselves are mode 0, the parity shading.  shade_launcher picks by the render's mode
//
// shade/trace alternate until a shade pass emits nothing (every path record has
// finished its samples), or until so few are active that the step hands them to the
// next one (jade_render_flush).  There is no CPU fallback: if HIP is unavailable the
// entry points return JADE_ERR_DEVICE.
//
// This file: the render kernels above but the first pass's, then the host side that drives them - jade_scene_create (upload, selftest, size_grids),
// jade_render_begin, run_passes (the schedule of a step: PassRun and its pieces), step / flush / resolve, jade_trace_rays and
// the JADE_DEBUG_EXPORTS entry points.  The rest of libjade_hip.so's host side sits beside the kernels it drives:
//   jade_shade.h         the bounce loop as a per-record state machine, and the record steps (how a sample begins, ends and parks)
//                        that shade_record, k_shade_binned and the first pass share
//   jade_trace.h         the BVH traversal: k_trace's wave-wide walk, k_light's per-lane walk, the packet walk
//   jade_light.h         the fused first pass: k_light_packet, k_light, k_packet_rays, k_heavy_scan, k_heavy_pack and their tunables
//   jade_runtime.h       what the files share: jade_fail, HIP_TRY, DevBuf, DevEvent, Tunables, struct jade_scene, and the two
//                        functions through which another file reaches a kernel of this one (launch_trace, resolve_to)
//   jade_scene_prep.hip  validate_desc + prepare_scene: the caller's scene -> the records uploaded here; host only, no HIP call
//   jade_adaptive.hip    jade_render_adaptive, jade_render_error + k_tile_error
//   jade_denoise.hip     jade_render_guides, jade_render_denoise, jade_denoise_image + their kernels
//   jade_multi.hip       jade_render_multi and its RCCL gather
//   jade_bvh.hip         the BVH builders
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "jade_runtime.h"
#include "jade_shade.h"
#include "jade_smooth_shade.h"
#include "jade_trace.h"
#include "jade_light.h"

// ------------------------------------------------------------------ kernels --

#ifndef JADE_TRACE_NT
#define JADE_TRACE_NT 1 /* k_trace reads and writes the ray records with non-temporal hints */
#endif
#if JADE_TRACE_NT
#define NT_LD(p) __builtin_nontemporal_load(p)
#define NT_ST(p, v) __builtin_nontemporal_store((v), (p))
#else
#define NT_LD(p) (*(p))
#define NT_ST(p, v) (*(p) = (v))
#endif
#if JADE_TRACE_PROFILE
__device__ unsigned long long g_trace_prof[PL_N];  // development profile of k_trace: shader clocks per piece of the loop, summed over waves
#endif
typedef float jade_v4f __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ float4 nt_ld4(const float4* p) {
  const jade_v4f v = NT_LD(reinterpret_cast<const jade_v4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
static __device__ __forceinline__ void nt_st4(float4* p, float x, float y, float z, float w) {
  const jade_v4f v = {x, y, z, w};
  NT_ST(reinterpret_cast<jade_v4f*>(p), v);
}

// The sort key of a queued ray (ordered queues, k_ray_keys below): the kind of ray - shadow ray towards emitter k / environment ray /
// indirect ray / single-ray stage - then the triangle it leaves (its index in BVH order is a place on the tree's own space-filling
// curve), then the octant it heads into; left-aligned in 32 bits.
static __device__ __forceinline__ uint32_t ray_sort_key(uint32_t st, uint32_t k, int n_emit, int32_t skip, float dx, float dy, float dz, uint32_t tri_bits) {
  uint32_t cls = 7u;  // single-ray stages (mirror, refraction, camera)
  if (st == ST_DIFFUSE || st == ST_BSSRDF) cls = (int)k < n_emit ? (k < 5u ? k : 4u) : ((int)k == n_emit ? 5u : 6u);
  const uint32_t tri = skip < 0 ? 0u : ((uint32_t)skip & ((1u << tri_bits) - 1u));
  const uint32_t oct = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
  return (cls << 29) | (((tri << 3) | oct) << (26u - tri_bits));
}

__global__ void k_selftest(QueueCtl* q, float one) { q->fp_bad = (uint32_t)jade_fp_selftest(one); }

__global__ void k_init(PathState P) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.npix) return;
  P.hdr[p] = make_uint4(0u, 0u, ST_IDLE, 0u);
}

#define JADE_ARM_BLOCK 1024
#define JADE_ARM_PER_THREAD 8
// Lists every record that has work in this step (samples left to start, or a
// path suspended by a previous step): the input of the first shade pass.
__global__ __launch_bounds__(JADE_ARM_BLOCK) void k_arm(PathState P, uint32_t target_spp, uint32_t* active_out, QueueCtl* qc) {
  // a block lists JADE_ARM_PER_THREAD * 1024 consecutive records with ONE list atomic (same-address atomics
  // cost ~12 ns each: at 534 M records one per 1024 was 6 ms), in record order
  constexpr int NW = JADE_ARM_BLOCK / 64, NJ = JADE_ARM_PER_THREAD;
  __shared__ uint32_t sh_cnt[NJ * NW + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t base = (size_t)blockIdx.x * (JADE_ARM_BLOCK * NJ);
  uint32_t wantm = 0, off[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const size_t p = base + (size_t)j * JADE_ARM_BLOCK + threadIdx.x;
    bool want = false;
    if (p < (size_t)P.npix) {
      const uint4 h = P.hdr[p];
      const uint32_t st = h.z & 255u;
      want = st != ST_IDLE || next_sample(P, (int)p, h.y).sidx < target_spp;
    }
    const unsigned long long m = __ballot(want);
    off[j] = lanes_below(m);
    if (want) wantm |= 1u << j;
    if (lane == 0) sh_cnt[j * NW + w] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // exclusive prefix over (j, wave), then the block's place in the list
    uint32_t tot = 0;
    for (int i = 0; i < NJ * NW; ++i) {
      const uint32_t c = sh_cnt[i];
      sh_cnt[i] = tot;
      tot += c;
    }
    sh_cnt[NJ * NW] = tot ? atomicAdd(&qc->active, tot) : 0u;
  }
  __syncthreads();
  const uint32_t blk = sh_cnt[NJ * NW];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (wantm & (1u << j)) active_out[blk + sh_cnt[j * NW + w] + off[j]] = (uint32_t)(base + (size_t)j * JADE_ARM_BLOCK + threadIdx.x);
}

#ifndef JADE_SHADE_BLOCK
#define JADE_SHADE_BLOCK 512 /* threads per k_shade block: one queue + one list atomic per block (512: +1.8 % over 256; 1024: none) */
#endif
#define JADE_SHADE_NW (JADE_SHADE_BLOCK / 64)
#ifndef JADE_LEAN_BLOCK
#define JADE_LEAN_BLOCK 512 /* threads per k_shade_lean block (1024 = half the list atomics, but 26 vs 20 ms per pass at 534 M records) */
#endif
#ifndef JADE_SHADE_WAVES
#define JADE_SHADE_WAVES 6 /* k_shade: 75 VGPRs, no spill (7 would spill 16 B).  +4 % over 5 when it runs alone, +-0 behind k_shade_lean */
#endif
// One record's shade pass (see the file header).  LEAN = the kernel that only knows camera rays, the sky and pure mirrors: it hands every other
// record to the full kernel through `defer` (either untouched, or parked at ST_VERTEX with its path state stored).  Same statements either way: the
// lean paths are the shared helpers consume_mirror / begin_bounce_lean / bounce_mirror.
// M: the render's mode (ShadeMode, jade_runtime.h; 0: the parity shading), read by bit through sm; every bit is non-parity, its code in the
// kernels of a mode that carries it only.  A: what those kernels take for it (ShadeArgs<M>, jade_shade.h).  "stated": include/jade_bvh.h.
// SM_ENVIS: environment rays by importance.  SM_LENS: the camera ray leaves a point of a thin lens ("The lens, stated")
// SM_SHUTTER: the camera ray leaves the pose of a time drawn within the exposure, through a lens or not, by the constants *A.H() ("The shutter, stated")
// SM_LIGHTS: one emitter per sampling vertex, drawn from the table A.lights() ("The lights, stated").  The entry drawn travels in the fourth
// word of the record's header, which this function reads and writes anyway.
// SM_COSINE: the environment and indirect rays of a sampling vertex are drawn with pdf cos / pi about the normal ("The bounce, stated").  Nothing of it travels with the record.
// SM_MIS: the emitter rays and the indirect ray weighed against each other ("The direct light, stated"; with SM_COSINE), from the per-triangle table A.mis().  consume alone reads it.
// SM_ENVMIX: the environment ray by the one-sample mixture of SM_ENVIS's draw and the bounce sampling's (include/jade_rt.h, JADE_ENV_MIXTURE;
// with SM_ENVIS).  begin_bounce alone knows it: m travels where SM_ENVIS's ratio does.
// SM_PASSES: every addend of a sample's colour is booked in its pass as well ("The passes, stated"), in the planes *A.L() (jade_shade.h,
// PassPlanes).  The colour itself is formed by the statements it always was.
// SM_BRANCH: the draws that choose the arm at a vertex of depth 0 or 1 are read off the sample's stratified number U ("The branch draws, stated";
// branch_number, jade_shade.h), formed here from the record's `done` and home pixel.  Nothing of it travels with the record.
// SM_SMOOTH: the normal of every vertex shaded is the triangle's vertex normals interpolated at the vertex ("The shading normal, stated"), from the records
// A.smooth() (jade_smooth_shade.h), where the bounce and the fold stand a second time with it.  Nothing of it travels with the record.
// SM_TEX (with SM_SMOOTH): A.smooth() carries the texture tables as well (jade_texture.h) and the same family multiplies the surface colour at (c.obj, c.src)
// into every brdf and refract_albedo it reads ("The surface colour, stated"); the lean kernel's mirror fold is consume_mirror_textured.
// SM_NMAP (with SM_TEX | SM_SMOOTH): A.smooth() carries the normal map's tables as well (jade_normal_map.h) and the family's one call for the normal
// resolves to the mapped normal ("The mapped normal, stated").
template <bool LEAN, uint32_t M = 0>
static __device__ __forceinline__ void shade_record(const DevScene& S, const PathState& P, const RenderConst& R, const int32_t* tile_ids,
                                                    uint32_t target_spp, const int p, ShadeCtx& c, uint32_t& st_out, bool& defer,
                                                    const ShadeArgs<M>& A = SHADE_ARGS_NONE) {
  constexpr bool ENVIS = sm(M, SM_ENVIS), LENS = sm(M, SM_LENS), SHUTTER = sm(M, SM_SHUTTER), LIGHTS = sm(M, SM_LIGHTS), PASSES = sm(M, SM_PASSES), BRANCH = sm(M, SM_BRANCH), SMOOTH = sm(M, SM_SMOOTH);
  const int npix = P.npix;
  uint32_t st = ST_INVALID;
  defer = false;
  // Prologue: everything most record-passes need, requested together so the pass is one
  // round trip deep instead of one per field (the kernel is latency-bound: PMC shows its
  // waves parked on s_waitcnt 74 % of the time).
  const int pp = p < npix ? p : 0;
  const uint4 hdr0 = P.hdr[pp];
  const uint32_t word = hdr0.z;
  const uint32_t rng0 = hdr0.x;
  const uint32_t done0 = hdr0.y;
  const float4 slot0 = P.slot[(size_t)pp * P.nslots];  // slot 0: {direction, hit}
  const int hit0 = __float_as_int(slot0.w);
  const jvec3 dir0 = jv(slot0.x, slot0.y, slot0.z);
  const uint32_t rec_m = (uint32_t)pp / (uint32_t)P.npx;
  const int home_pix = (int)((uint32_t)pp - rec_m * (uint32_t)P.npx);
  const int tid0 = tile_ids[home_pix >> 8];
  if (p < npix) st = word & 255u;
  if (st != ST_INVALID) {
    const Px px(P, p);
    // State is loaded and stored by need: a background record (camera ray ->
    // sky, or -> mirror floor -> sky) touches ~90 B per pass, not the whole
    // ~230-B record; only records on a multi-bounce path carry thr/acc/le/....
    const bool on_path = st >= ST_DIFFUSE && st <= ST_REFRACT_EXIT;
    if (LEAN && on_path && st != ST_MIRROR) {  // needs the full kernel: hand it over untouched
      defer = true;
      st_out = st;
      return;
    }
    const bool has_ctx = on_path || st == ST_VERTEX;  // ST_VERTEX: handed over by the lean kernel this pass
    c.rng = rng0;
    c.depth = (word >> 8) & 255u;
    c.flags = word >> 16;
    c.stage = st;
    c.thr = jv(1, 1, 1);
    c.acc = jv(0, 0, 0);
    c.le = jv(0, 0, 0);
    c.obj = 0;
    c.src = jv(0, 0, 0);
    c.out = jv(0, 0, 0);
    if (has_ctx) {
      // Stored and loaded by need (the lean kernel is bound by these bytes): before the first
      // path_push thr is 1 and acc 0 (only path_push changes them, and it counts depth up); a
      // mirror ray in flight needs neither the vertex it left nor, at depth 0, a stored Le
      // (it is the emissive of the triangle still in obj).
      const float4* cx = P.ctx + (size_t)p * 4;
      const float4 b0 = cx[0], b1 = cx[1], b2 = cx[2], b3 = cx[3];
      c.obj = __float_as_int(b0.w);
      if (c.depth != 0) {
        c.thr = jv(b0.x, b0.y, b0.z);
        c.acc = jv(b1.x, b1.y, b1.z);
      }
      if (st == ST_MIRROR && c.depth == 0) c.le = V3(shade_tri(S, c.obj).m->emissive);
      else c.le = jv(b2.x, b2.y, b2.z);
      if (st != ST_MIRROR) {
        c.src = jv(b2.w, b3.x, b3.y);
        c.out = jv(b3.z, b3.w, b1.w);
      }
    }
    uint32_t done = done0;
    uint32_t light = LIGHTS ? hdr0.w : 0u;  // JADE_LIGHTS_ONE: the emitter entry the bounce in flight drew
    uint32_t pmask = 0u;  // PASSES: the passes the sample in flight has touched
    PassParts parts;
    if (PASSES) {
      pmask = A.L()->mask[p];
      parts.cls = -1;
    }
    jvec3 l_final;
    bool finished = false;  // a sample ended: colour in `color`
    jvec3 color = jv(0, 0, 0);

    // (a) fold in the results of the rays issued by the previous pass
    if (st == ST_PRIMARY) {
      int h = hit0;
      jvec3 d = dir0;
      if (h < 0) {
        color = sample_hdr(S, d);  // PathTrace.cu:1443-1445
        if (PASSES) pass_add(*A.L(), p, pmask, PASS_BACKGROUND, color);
        finished = true;
      } else {
        vertex_from_primary(S, c, h, px.hpt(0), d);
        st = ST_VERTEX;
      }
    } else if (on_path) {
      int r;
      if constexpr (SMOOTH && !LEAN) r = consume_smooth<M>(S, px, c, &l_final, A.smooth());
      else if constexpr (sm(M, SM_TEX)) r = consume_mirror_textured(S, px, c, &l_final, A.smooth());
      else r = LEAN ? consume_mirror<Px, M>(S, px, c, &l_final, &parts) : consume<M>(S, px, c, &l_final, A.lights(), light, A.mis(), &parts);
      if (PASSES) pass_fold(*A.L(), p, pmask, parts, c.thr, r == CONSUME_END, r == CONSUME_ZERO);
      if (r == CONSUME_VERTEX) {
        st = ST_VERTEX;
      } else if (r == CONSUME_EMITTED) {
        st = c.stage;
      } else {
        if (r == CONSUME_END) color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
        else color = c.le;  // pathTracing returned 0
        finished = true;
      }
    }
    // (b) advance until this record has rays in flight or no samples left
    for (;;) {
      if (finished) {
        if (PASSES) {  // c.le of the sample's camera vertex (0 for a camera ray that met nothing), then the sample's parts to the totals
          pass_add(*A.L(), p, pmask, PASS_EMISSION, c.le);
          pass_commit(*A.L(), p, pmask);
        }
        add_sample(P, rec_m, home_pix, done, c, color);
        finished = false;
        st = ST_IDLE;
      }
      if (st == ST_VERTEX) {
        if (LEAN && !lean_can_shade(shade_tri(S, c.obj).m)) {  // jade / diffuse / glass: the full kernel continues from here
          defer = true;
          break;
        }
        // A mode with SM_BRANCH: the statement below and what follows it, with the vertex's stratified number - U of the sample in flight, which the
        // record's `done` names.  A second text, since a flag or a helper woven into the one below moves the registers of every other kernel.
        if constexpr (BRANCH) {
          uint32_t bu = 0u;
          if (c.depth < 2u) {
            const NextSample cs = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
            int bx, by;
            (void)pixel_xy_t(R, cs.pixel == home_pix ? tid0 : tile_ids[cs.pixel >> 8], cs.pixel, &bx, &by);
            bu = branch_number(R, bx, by, cs.sidx, c.depth);
          }
          if (LEAN ? begin_bounce_lean_branch(S, px, c, &l_final, bu) : begin_bounce_branch<M>(S, px, c, &l_final, A.lights(), &light, bu)) {
            st = c.stage;
            if (!ENVIS || c.n_emit_rays != 0) break;
            const int r = consume<M>(S, px, c, &l_final, A.lights(), light, A.mis(), &parts);
            if (PASSES) pass_fold(*A.L(), p, pmask, parts, c.thr, r == CONSUME_END, r == CONSUME_ZERO);
            if (r == CONSUME_VERTEX) {
              st = ST_VERTEX;
              continue;
            }
            color = r == CONSUME_END ? jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final))) : c.le;
            finished = true;
            continue;
          }
        } else if constexpr (SMOOTH) {
          // A mode with SM_SMOOTH: the same step with the shading normal (jade_smooth_shade.h).  A bounce may emit no ray under any environment sampling -
          // every drawn direction can fail against the flat normal - and then has all its results already, as under SM_ENVIS below.
          if (LEAN ? begin_bounce_lean_smooth(S, px, c, &l_final, A.smooth()) : begin_bounce_smooth<M>(S, px, c, &l_final, A.smooth())) {
            st = c.stage;
            if (LEAN || c.n_emit_rays != 0) break;  // (the lean kernel's mirror always emits its ray)
            const int r = consume_smooth<M>(S, px, c, &l_final, A.smooth());
            if (r == CONSUME_VERTEX) {
              st = ST_VERTEX;
              continue;
            }
            color = r == CONSUME_END ? jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final))) : c.le;
            finished = true;
            continue;
          }
        } else
        if (LEAN ? begin_bounce_lean(S, px, c, &l_final) : begin_bounce<M>(S, px, c, &l_final, A.lights(), &light)) {
          st = c.stage;
          if (!ENVIS || c.n_emit_rays != 0) break;
          // env_sampling only: a bounce that emitted NO ray (the drawn sky direction lay on the wrong side, no shadow ray faced its
          // emitter, the roulette ended the path) has all its results already - nothing is visible: folded in right here (with the
          // reference's sampling there is always the environment ray)
          const int r = consume<M>(S, px, c, &l_final, A.lights(), light, A.mis(), &parts);
          if (PASSES) pass_fold(*A.L(), p, pmask, parts, c.thr, r == CONSUME_END, r == CONSUME_ZERO);
          if (r == CONSUME_VERTEX) {
            st = ST_VERTEX;
            continue;
          }
          color = r == CONSUME_END ? jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final))) : c.le;
          finished = true;
          continue;
        }
        color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
        if (PASSES) pass_add(*A.L(), p, pmask, PASS_EMISSION, jv_mul(c.thr, l_final));  // the path ended on an emitter (or with 0: the mirror's roulette)
        finished = true;
        continue;
      }
      if (st == ST_IDLE) {
        // next sample of this record
        int x, y;
        uint32_t sidx;
        if (!next_live_sample(P, R, tile_ids, target_spp, rec_m, home_pix, tid0, done, &sidx, &x, &y)) break;
        // camera ray, PathTrace.cu:1428-1437
        float left_offset, up_offset;
        film_point(R, x, y, sidx, &c.rng, &left_offset, &up_offset);
        jvec3 dir;
        if (SHUTTER) {
          // the lens's two draws if there is a lens (wave-uniform), then the time's; the origin is the ray's own, stored as the lens's is
          float u3 = 0.0f, u4 = 0.0f;
          if (R.lens_radius > 0.0f) {
            u3 = jade_rand(&c.rng);
            u4 = jade_rand(&c.rng);
          }
          const float ut = jade_rand(&c.rng);
          jvec3 org;
          shutter_ray(R.cam, R.eye, *A.H(), R.lens_radius, P.lens_k, left_offset, up_offset, u3, u4, ut, &org, &dir);
          px.set_origin(org, -1);
        } else if (LENS) {
          // two more draws before any draw of the path, and an origin of the ray's own: stored with "no source triangle" (-1), which
          // shade_tail, k_trace's refill and k_ray_keys read as they read jade_trace_rays' rays
          const float u3 = jade_rand(&c.rng);
          const float u4 = jade_rand(&c.rng);
          jvec3 org;
          lens_ray(R.cam, R.eye, R.lens_radius, P.lens_k, left_offset, up_offset, u3, u4, &org, &dir);
          px.set_origin(org, -1);
        } else {
          dir = pinhole_dir(R, left_offset, up_offset);
          reinterpret_cast<int*>(P.orgs + p)[3] = JADE_SKIP_CAMERA;  // no source triangle, and the origin is the eye: k_trace takes it from P.eye
        }
        px.set_dir(0, dir);
        px.set_hit(0, -1);
        c.n_emit_rays = 1;
        c.c_primary += 1;
        st = ST_PRIMARY;
        break;
      }
      break;  // a pending stage that just emitted (refraction loop)
    }
    count_secondary(c, st);
    P.hdr[p] = make_uint4(c.rng, done, st | (c.depth << 8) | (c.flags << 16), light);
    if ((st >= ST_DIFFUSE && st <= ST_REFRACT_EXIT) || st == ST_VERTEX) store_ctx(P, p, c);
    if (PASSES) A.L()->mask[p] = pmask;
  }
  st_out = st;
}

// Queue the emitted rays, list the record for the next pass and/or for the full kernel: wave scans,
// then ONE atomic per block for queue + list (not per wave: see DevCounters).
template <bool LEAN, int NW>  // NW: waves per block
static __device__ __forceinline__ void shade_tail(const PathState& P, int p, uint32_t st, const ShadeCtx& c, bool defer,
                                                  uint32_t* active_out, uint32_t* heavy_out, uint32_t* queue, QueueCtl* qc,
                                                  DevCounters* ctr) {
  __shared__ uint32_t sh_rays[NW], sh_act[NW], sh_def[NW], sh_base[3];
  __shared__ uint32_t sh_ctr[NW][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t total;
  const uint32_t off = wave_excl_scan((uint32_t)c.n_emit_rays, &total);
  const bool live = c.n_emit_rays > 0;
  const unsigned long long am = __ballot(live), dm = LEAN ? __ballot(defer) : 0ull;
  const uint32_t aoff = lanes_below(am), doff = lanes_below(dm);
  if (lane == 0) {
    sh_rays[w] = total;
    sh_act[w] = (uint32_t)__popcll(am);
    sh_def[w] = (uint32_t)__popcll(dm);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tr = 0, ta = 0, td = 0;
    for (int i = 0; i < NW; ++i) {
      tr += sh_rays[i];
      ta += sh_act[i];
      td += sh_def[i];
    }
    // count can never carry into active: a pass emits < 2^32 rays (nslots * npix < 2^32 is checked in jade_render_begin)
    const unsigned long long got =
        (tr | ta) ? atomicAdd(reinterpret_cast<unsigned long long*>(&qc->count), (unsigned long long)tr | ((unsigned long long)ta << 32)) : 0ull;
    sh_base[0] = (uint32_t)got;
    sh_base[1] = (uint32_t)(got >> 32);
    sh_base[2] = (LEAN && td) ? atomicAdd(&qc->heavy, td) : 0u;
  }
  __syncthreads();
  if (live || (LEAN && defer)) {
    uint32_t wq = sh_base[0] + off, wa = sh_base[1] + aoff, wd = sh_base[2] + doff;
    for (int i = 0; i < w; ++i) {
      wq += sh_rays[i];
      wa += sh_act[i];
      wd += sh_def[i];
    }
    if (LEAN && defer) heavy_out[wd] = (uint32_t)p;
    if (live && active_out) active_out[wa] = (uint32_t)p;
    (void)wq;
  }
  {
    // The wave's rays go into its stretch of the queue SLOT BY SLOT: all its records' slot-0 rays (shadow rays towards
    // the first emitter), then the slot-1 rays, ...  The 64 entries a wave of k_trace takes are then one kind of ray from
    // 64 neighbouring records - same target or same sky, origins side by side: they walk the same part of the tree
    // (L1 hits) and end together - instead of the four rays of 16 records.
    uint32_t wbase = sh_base[0];
    for (int i = 0; i < w; ++i) wbase += sh_rays[i];
    const int used = !live ? 0 : (st == ST_DIFFUSE || st == ST_BSSRDF) ? P.nslots : 1;
    // ... and, for the first rayq_cap entries, the ray as k_trace's refill needs it (PathState.rayq): origin and source triangle are
    // the record's (camera rays: the eye), direction and limit the slot's, just written by this thread
    jvec3 ro = jv(0, 0, 0);
    int32_t rskip = -1;
    if (used && (P.rayq_cap || P.keyq)) {
      const float4 og = P.orgs[p];
      rskip = __float_as_int(og.w);
      ro = rskip == JADE_SKIP_CAMERA ? jv(P.eye[0], P.eye[1], P.eye[2]) : jv(og.x, og.y, og.z);
    }
    for (int k = 0; k < P.nslots; ++k) {
      const float4* sl = P.slot + ((size_t)p * P.nslots + k);
      const bool q = k < used && reinterpret_cast<const int*>(sl)[3] != -2;  // (-2: no ray in this slot; anything else: the queued ray's limit, jade_device.h)
      const unsigned long long m = __ballot(q);
      const uint32_t pos = wbase + lanes_below(m);
      const uint32_t e = (uint32_t)p * (uint32_t)P.nslots + (uint32_t)k;
      if (q) queue[pos] = e;
      if (q && P.keyq && pos < P.keyq_cap) {  // ordered queue: the key beside the entry (k_ray_keys read three scattered sectors per ray for it)
        const float4 dv = sl[0];
        P.keyq[pos] = ray_sort_key(st, (uint32_t)k, P.nslots - 2, rskip, dv.x, dv.y, dv.z, P.key_tri_bits);
      }
      if (q && pos < P.rayq_cap) {
        const float4 dv = sl[0];
        jvec3 inv, dn;
        uint32_t skipx;
        walk_prepare(ro, jv(dv.x, dv.y, dv.z), rskip, dv.w, &inv, &dn, &skipx);
        float4* rq = P.rayq + (size_t)pos * 3;
        nt_st4(rq, ro.x, ro.y, ro.z, __uint_as_float(skipx));
        nt_st4(rq + 1, inv.x, inv.y, inv.z, P.early_exit ? dv.w : __int_as_float(-1));
        nt_st4(rq + 2, dn.x, dn.y, dn.z, __uint_as_float(e));
      }
      wbase += (uint32_t)__popcll(m);
    }
  }
  // work counters: per wave into LDS, then one set of atomics per block
  const uint32_t s0 = (uint32_t)wave_sum_u32(c.c_primary), s1 = (uint32_t)wave_sum_u32(c.c_shadow),
                 s2 = (uint32_t)wave_sum_u32(c.c_shaded), s3 = (uint32_t)wave_sum_u32(c.c_samples),
                 s4 = (uint32_t)wave_sum_u32(c.c_cls);  // four byte-wide sums of at most 64 each: no carry between them
  if (lane == 0) {
    sh_ctr[w][0] = s0;
    sh_ctr[w][1] = s1;
    sh_ctr[w][2] = s2;
    sh_ctr[w][3] = s3;
    sh_ctr[w][4] = s4 & 255u;
    sh_ctr[w][5] = (s4 >> 8) & 255u;
    sh_ctr[w][6] = (s4 >> 16) & 255u;
    sh_ctr[w][7] = s4 >> 24;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    unsigned long long t = 0;
    for (int i = 0; i < NW; ++i) t += sh_ctr[i][threadIdx.x];
    DevCounters* cs = ctr + (blockIdx.x % JADE_CTR_SHARDS);
    // word of DevCounters: primary 0, shadow 1, shaded 4, samples 5, env / indirect / mirror / refract 8-11
    const int i = (int)threadIdx.x, word = i < 2 ? i : i < 4 ? i + 2 : i + 4;
    if (t) atomicAdd(reinterpret_cast<unsigned long long*>(cs) + word, t);
  }
}

// The full shade kernel: one thread per entry of `list` (the active list, or — after k_shade_lean —
// the records that kernel handed over, whose count lives on the device: n_dev).  75 VGPRs, 6 waves/SIMD (JADE_SHADE_WAVES).
// M and A are shade_record's: k_shade is mode 0 and passes nothing, k_shade_mode<M> its mode and the argument it was launched with.
template <uint32_t M = 0>
static __device__ __forceinline__ void shade_kernel_body(const DevScene& S, const PathState& P, const RenderConst& R, const int32_t* tile_ids,
                                               uint32_t target_spp, const uint32_t* list, uint32_t n_host, const uint32_t* n_dev,
                                               uint32_t* active_out, uint32_t* queue, QueueCtl* qc, DevCounters* ctr, const QueueCtl* prev,
                                               uint32_t stop_below, const ShadeArgs<M>& A = SHADE_ARGS_NONE) {
  const uint32_t n = n_dev ? *n_dev : n_host;
  // A pass of a batch (prev = the pass before it, on the device): nothing to do once the paths have ended (that pass
  // emitted no ray) or once fewer than stop_below records are active - the point where the host would hand the rest to
  // the next step (carry-over).  Such a pass leaves the lists alone and passes the count on, so that every later pass
  // of the batch stops too and the host finds, in the ring, where the batch really ended.
  if (prev && (prev->count == 0 || n < stop_below)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) qc->active = prev->count == 0 ? 0u : n;
    return;
  }
  if (blockIdx.x * blockDim.x >= n) return;  // block-uniform: the grid is sized for an upper bound of n_dev
  const uint32_t t_idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = t_idx < n ? (int)list[t_idx] : P.npix;
  ShadeCtx c;
  c.n_emit_rays = 0;
  c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
  uint32_t st;
  bool defer;
  shade_record<false, M>(S, P, R, tile_ids, target_spp, p, c, st, defer, A);
  shade_tail<false, JADE_SHADE_NW>(P, p, st, c, false, active_out, nullptr, queue, qc, ctr);
}
__global__ __launch_bounds__(JADE_SHADE_BLOCK, JADE_SHADE_WAVES) void k_shade(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                               uint32_t target_spp, const uint32_t* list, uint32_t n_host, const uint32_t* n_dev,
                                               uint32_t* active_out, uint32_t* queue, QueueCtl* qc, DevCounters* ctr, const QueueCtl* prev,
                                               uint32_t stop_below) {
  shade_kernel_body(S, P, R, tile_ids, target_spp, list, n_host, n_dev, active_out, queue, qc, ctr, prev, stop_below);
}
// ... and every non-parity mode (ShadeMode): one kernel per built mode M, instantiated where it is launched (launch_full).  k_shade's arguments, then what
// mode M takes beyond them in one piece, T = ShadeArgs<M> (jade_shade.h; mode_args fills it) - but under SM_MIS its members apart, T = (ArgPlanes,) ArgLights,
// ArgMis: a struct of two pointers reaches a kernel by reference and is loaded in the first block, which costs COSINE|MIS(|PASSES) exec masks kept in VGPR lanes.
template <uint32_t M, class... T>
__global__ __launch_bounds__(JADE_SHADE_BLOCK, JADE_SHADE_WAVES) void k_shade_mode(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                               uint32_t target_spp, const uint32_t* list, uint32_t n_host, const uint32_t* n_dev,
                                               uint32_t* active_out, uint32_t* queue, QueueCtl* qc, DevCounters* ctr, const QueueCtl* prev,
                                               uint32_t stop_below, T... a) {
  ShadeArgs<M> A;
  ((static_cast<T&>(A) = a), ...);
  shade_kernel_body<M>(S, P, R, tile_ids, target_spp, list, n_host, n_dev, active_out, queue, qc, ctr, prev, stop_below, A);
}

// ---------------------------------------------------------------------------------------------------------------
// k_shade_binned (round 4; VERDICT r1-r3: "k_shade is one divergent kernel at 13 of 64 lanes").  k_shade's instructions are mostly
// the BRANCH of the bounce it samples - BSSRDF (six powf, the exit-point search), SSS / diffuse (shadow limits, two sphere
// directions), mirror, refraction - and a wave whose 64 records take four different branches runs all four, each for a quarter of
// its lanes.  Which branch a record takes is known after the emissive test and one or two random draws (bounce_classify), and the
// branch itself needs little of the record: its random state, the vertex (triangle, position, outgoing direction) and the
// record's number, through which it writes its rays.  So the block DEALS the records by branch through LDS: every thread loads
// and folds its own record as before (shade_record's part (a)), classifies it, and puts those few words into a pool in which
// every branch's records form a stretch that starts at a multiple of 64; then every thread runs bounce_branch for the pool entry
// with its own index - a wave's 64 entries are one branch - and writes the outcome back; the record's own thread picks it up,
// finishes the sample / starts the next one if the path ended, and stores and queues as ever (shade_tail).  Same statements, same
// draws in the same order per record: every bit and counter is k_shade's (the schedule matrix runs both: JADE_SHADE_BINNED).
// ---------------------------------------------------------------------------------------------------------------
#ifndef JADE_SHADE_BIN_WAVES
#define JADE_SHADE_BIN_WAVES 4 /* 109 VGPRs, no scratch: "rest" of a 1024-spp step of C3 134.6 ms; 5 waves (96 VGPRs, 20 bytes of scratch) 141.8; 6 (80, 128 bytes) 166.7; k_shade: 132.1 */
#endif
#define JADE_BIN_POOL (JADE_SHADE_BLOCK + (BT_N - 1) * 64) /* pool entries: 512 records + the padding of four stretches */
struct alignas(16) BinSlot {  // 48 bytes
  int32_t p;       // the record
  uint32_t rng;    // its random state: in = after bounce_classify's draws, out = after the branch's
  int32_t obj;     // the vertex: triangle ...
  uint32_t sf;     // in: stage | flags << 8 (BT_DIFFUSE: set by bounce_classify); out: stage | flags << 8 | rays emitted << 16 | path ended << 31
  float src[3];    // ... position            (out: l_final of a path that ended)
  float out[3];    // ... outgoing direction
  float pad[2];
};
__global__ __launch_bounds__(JADE_SHADE_BLOCK, JADE_SHADE_BIN_WAVES) void k_shade_binned(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                               uint32_t target_spp, const uint32_t* list, uint32_t n_host, const uint32_t* n_dev,
                                               uint32_t* active_out, uint32_t* queue, QueueCtl* qc, DevCounters* ctr, const QueueCtl* prev,
                                               uint32_t stop_below) {
  const uint32_t n = n_dev ? *n_dev : n_host;
  if (prev && (prev->count == 0 || n < stop_below)) {  // (as k_shade: a pass of a batch behind the end of the step)
    if (blockIdx.x == 0 && threadIdx.x == 0) qc->active = prev->count == 0 ? 0u : n;
    return;
  }
  if (blockIdx.x * blockDim.x >= n) return;
  __shared__ BinSlot pool[JADE_BIN_POOL];
  __shared__ uint32_t sh_cnt[JADE_SHADE_NW][BT_N];
  __shared__ uint32_t sh_base[BT_N], sh_n[BT_N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t t_idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int npix = P.npix;
  const int p = t_idx < n ? (int)list[t_idx] : npix;
  ShadeCtx c;
  c.n_emit_rays = 0;
  c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
  // ---- (1) the thread's own record: load, fold in the results of the rays issued last pass (shade_record<false>, prologue + (a))
  uint32_t st = ST_INVALID;
  const int pp = p < npix ? p : 0;
  const uint4 hdr0 = P.hdr[pp];
  const uint32_t word = hdr0.z;
  const float4 slot0 = P.slot[(size_t)pp * P.nslots];
  const int hit0 = __float_as_int(slot0.w);
  const jvec3 dir0 = jv(slot0.x, slot0.y, slot0.z);
  const uint32_t rec_m = (uint32_t)pp / (uint32_t)P.npx;
  const int home_pix = (int)((uint32_t)pp - rec_m * (uint32_t)P.npx);
  const int tid0 = tile_ids[home_pix >> 8];
  if (p < npix) st = word & 255u;
  const bool have = st != ST_INVALID;
  const Px px(P, pp);
  uint32_t done = hdr0.y;
  jvec3 l_final = jv(0, 0, 0), color = jv(0, 0, 0);
  bool finished = false;
  int type = -1;  // the branch this record's bounce takes (BT_*), -1 = none this pass
  if (have) {
    const bool on_path = st >= ST_DIFFUSE && st <= ST_REFRACT_EXIT;
    const bool has_ctx = on_path || st == ST_VERTEX;
    c.rng = hdr0.x;
    c.depth = (word >> 8) & 255u;
    c.flags = word >> 16;
    c.stage = st;
    c.thr = jv(1, 1, 1);
    c.acc = jv(0, 0, 0);
    c.le = jv(0, 0, 0);
    c.obj = 0;
    c.src = jv(0, 0, 0);
    c.out = jv(0, 0, 0);
    if (has_ctx) {
      const float4* cx = P.ctx + (size_t)p * 4;
      const float4 b0 = cx[0], b1 = cx[1], b2 = cx[2], b3 = cx[3];
      c.obj = __float_as_int(b0.w);
      if (c.depth != 0) {
        c.thr = jv(b0.x, b0.y, b0.z);
        c.acc = jv(b1.x, b1.y, b1.z);
      }
      if (st == ST_MIRROR && c.depth == 0) c.le = V3(shade_tri(S, c.obj).m->emissive);
      else c.le = jv(b2.x, b2.y, b2.z);
      if (st != ST_MIRROR) {
        c.src = jv(b2.w, b3.x, b3.y);
        c.out = jv(b3.z, b3.w, b1.w);
      }
    }
    if (st == ST_PRIMARY) {
      if (hit0 < 0) {
        color = sample_hdr(S, dir0);  // PathTrace.cu:1443-1445
        finished = true;
      } else {
        vertex_from_primary(S, c, hit0, px.hpt(0), dir0);
        st = ST_VERTEX;
      }
    } else if (on_path) {
      const int r = consume(S, px, c, &l_final);
      if (r == CONSUME_VERTEX) {
        st = ST_VERTEX;
      } else if (r == CONSUME_EMITTED) {
        st = c.stage;
      } else {
        color = r == CONSUME_END ? jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final))) : c.le;
        finished = true;
      }
    }
    // ---- (2) the branch of the bounce at a vertex (the emissive test ends the path right here)
    if (!finished && st == ST_VERTEX) {
      type = bounce_classify(S, c, &l_final);
      if (type == BT_END) {
        color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
        finished = true;
        type = -1;
      }
    }
  }
  // ---- (3) deal: every branch's records into a stretch of the pool that starts at a multiple of 64
  uint32_t rank = 0;
#pragma unroll
  for (int T = 1; T < BT_N; ++T) {
    const unsigned long long m = __ballot(type == T);
    if (type == T) rank = lanes_below(m);
    if (lane == 0) sh_cnt[w][T] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t base = 0;
    for (int T = 1; T < BT_N; ++T) {
      uint32_t tot = 0;
      for (int i = 0; i < JADE_SHADE_NW; ++i) {
        const uint32_t v = sh_cnt[i][T];
        sh_cnt[i][T] = tot;  // exclusive over the waves
        tot += v;
      }
      sh_base[T] = base;
      sh_n[T] = tot;
      base += (tot + 63u) & ~63u;
    }
    sh_base[0] = base;  // the end of the pool
  }
  __syncthreads();
  uint32_t my_entry = 0;
  if (type >= 1) {
    my_entry = sh_base[type] + sh_cnt[w][type] + rank;
    BinSlot& e = pool[my_entry];
    e.p = p;
    e.rng = c.rng;
    e.obj = c.obj;
    e.sf = c.stage | (c.flags << 8);
    e.src[0] = c.src.x; e.src[1] = c.src.y; e.src[2] = c.src.z;
    e.out[0] = c.out.x; e.out[1] = c.out.y; e.out[2] = c.out.z;
  }
  __syncthreads();
  // ---- (4) the branch, for the pool entry with this thread's index: one branch per wave
  {
    const uint32_t pool_end = sh_base[0];
    for (uint32_t ei = threadIdx.x; ei < pool_end; ei += JADE_SHADE_BLOCK) {  // (a second turn only when the padding pushes the pool past the block)
      int T = 0;
#pragma unroll
      for (int k = 1; k < BT_N; ++k)
        if (ei >= sh_base[k] && ei < sh_base[k] + sh_n[k]) T = k;
      if (T != 0) {
        BinSlot& e = pool[ei];
        ShadeCtx wc;
        wc.rng = e.rng;
        wc.obj = e.obj;
        wc.stage = e.sf & 255u;
        wc.flags = (e.sf >> 8) & 255u;
        wc.depth = 0;
        wc.src = jv(e.src[0], e.src[1], e.src[2]);
        wc.out = jv(e.out[0], e.out[1], e.out[2]);
        wc.thr = wc.acc = wc.le = jv(0, 0, 0);
        wc.n_emit_rays = 0;
        wc.c_primary = wc.c_shadow = wc.c_shaded = wc.c_samples = wc.c_cls = 0;
        const Px wpx(P, e.p);
        jvec3 wl = jv(0, 0, 0);
        const bool emitted = bounce_branch(T, S, wpx, wc, &wl);
        e.rng = wc.rng;
        e.sf = (wc.stage & 255u) | ((wc.flags & 255u) << 8) | ((uint32_t)wc.n_emit_rays << 16) | (emitted ? 0u : 0x80000000u);
        e.src[0] = wl.x; e.src[1] = wl.y; e.src[2] = wl.z;
      }
    }
  }
  __syncthreads();
  // ---- (5) back with the record's own thread: the branch's outcome, then shade_record's part (b) for a sample that ended
  if (type >= 1) {
    const BinSlot& e = pool[my_entry];
    c.rng = e.rng;
    if (e.sf & 0x80000000u) {
      l_final = jv(e.src[0], e.src[1], e.src[2]);
      color = jv_add(c.le, jv_add(c.acc, jv_mul(c.thr, l_final)));
      finished = true;
    } else {
      c.stage = e.sf & 255u;
      c.flags = (e.sf >> 8) & 255u;
      c.n_emit_rays = (int)((e.sf >> 16) & 0x7fffu);
      st = c.stage;
    }
  }
  if (have) {
    if (finished) {
      add_sample(P, rec_m, home_pix, done, c, color);
      st = ST_IDLE;
    }
    if (st == ST_IDLE) {
      // next sample of this record
      int x, y;
      uint32_t sidx;
      if (next_live_sample(P, R, tile_ids, target_spp, rec_m, home_pix, tid0, done, &sidx, &x, &y)) {
        // camera ray, PathTrace.cu:1428-1437
        float left_offset, up_offset;
        film_point(R, x, y, sidx, &c.rng, &left_offset, &up_offset);
        reinterpret_cast<int*>(P.orgs + p)[3] = JADE_SKIP_CAMERA;
        px.set_dir(0, pinhole_dir(R, left_offset, up_offset));
        px.set_hit(0, -1);
        c.n_emit_rays = 1;
        c.c_primary += 1;
        st = ST_PRIMARY;
      }
    }
    count_secondary(c, st);
    P.hdr[p] = make_uint4(c.rng, done, st | (c.depth << 8) | (c.flags << 16), 0u);
    if ((st >= ST_DIFFUSE && st <= ST_REFRACT_EXIT) || st == ST_VERTEX) store_ctx(P, p, c);
  }
  shade_tail<false, JADE_SHADE_NW>(P, p, st, c, false, active_out, nullptr, queue, qc, ctr);
}

// The lean shade kernel: camera rays, the sky and pure mirrors only — what most records of most
// scenes do most of the time — in 56 VGPRs (8 waves/SIMD; the kernel is latency-bound).  It walks
// ALL records in record order (no list: perfectly coalesced, and nothing to fragment) and hands
// every record that needs anything else to k_shade through heavy_out / qc->heavy.
__global__ __launch_bounds__(JADE_LEAN_BLOCK) void k_shade_lean(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                                                 uint32_t target_spp, uint32_t* heavy_out, uint32_t* queue,
                                                                 QueueCtl* qc, DevCounters* ctr) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);  // >= npix: no record (shade_record checks)
  ShadeCtx c;
  c.n_emit_rays = 0;
  c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
  uint32_t st;
  bool defer;
  shade_record<true>(S, P, R, tile_ids, target_spp, p, c, st, defer);
  shade_tail<true, JADE_LEAN_BLOCK / 64>(P, p, st, c, defer, nullptr, heavy_out, queue, qc, ctr);
}
// ... under a thin lens (M = SM_LENS) or a shutter (M = SM_SHUTTER): the same kernel with that ray in its camera arm; or keeping passes
// (M = SM_PASSES): it finishes background, emission and mirror-sky samples, so it books them.  A: the constants, the planes (ShadeArgs<M>).
// The other bits of a mode mean nothing to it: what they change, it hands over (launch_lean).
template <uint32_t M>
__global__ __launch_bounds__(JADE_LEAN_BLOCK) void k_shade_lean_mode(DevScene S, PathState P, RenderConst R, const int32_t* tile_ids,
                                                                      uint32_t target_spp, uint32_t* heavy_out, uint32_t* queue,
                                                                      QueueCtl* qc, DevCounters* ctr, ShadeArgs<M> A) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  ShadeCtx c;
  c.n_emit_rays = 0;
  c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
  uint32_t st;
  bool defer;
  shade_record<true, M>(S, P, R, tile_ids, target_spp, p, c, st, defer, A);
  shade_tail<true, JADE_LEAN_BLOCK / 64>(P, p, st, c, defer, nullptr, heavy_out, queue, qc, ctr);
}

// ---------------------------------------------------------------------------------------------------------------
// Ray-queue ordering (north_star: "ray compaction/sort via wave-ballot/prefix-sum primitives"), OPT-IN (JADE_SORT=1).  Which ray
// sits beside which in the queue is free to choose: every result is written back to the ray's own slot, so no bit of any
// result depends on the order.  A ray's key: the kind of ray (shadow ray towards emitter i / environment ray / indirect ray /
// single-ray stage), then the triangle it leaves - its index in BVH order is a place on the tree's own space-filling curve -
// then the octant it heads into; rocPRIM sorts (key, queue entry) pairs, so the host has to know the queue's length: passes are
// host-followed while this is on.  Measured (profiles/r03_ray_ordering.json, r03_packet_shadow_probe.json): on C3, whose tree
// sits in the L2, a wave whose rays read the same lines is 2.6 % faster and the sort costs 9 %; it is meant for scenes whose
// geometry does not fit the L2 (C5: k_trace is bound by the rate of 64-B sector misses there).
// ---------------------------------------------------------------------------------------------------------------
__global__ void k_ray_keys(PathState P, const uint32_t* queue, uint32_t n, uint32_t* keys, uint32_t* positions, int n_emit, uint32_t tri_bits) {  // tri_bits: bits of the largest triangle index
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  positions[i] = i;  // what the sort moves with the key: the entry's POSITION (PathState.idxq)
  const uint32_t e = queue[i];
  const uint32_t p = e / (uint32_t)P.nslots, k = e - p * (uint32_t)P.nslots;
  const uint32_t st = P.hdr[p].z & 255u;
  const float4 og = P.orgs[p];
  const int32_t skip = __float_as_int(og.w);
  const float4 dv = P.slot[(size_t)e];
  keys[i] = ray_sort_key(st, k, n_emit, skip, dv.x, dv.y, dv.z, tri_bits);
}
// positions 0 .. n-1: what the sort moves with the keys when the keys came from the queueing kernel (written once per render)
__global__ void k_iota(uint32_t* v, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i;
}

#ifndef JADE_TRACE_WAVES
#define JADE_TRACE_WAVES 5 /* waves per SIMD the register allocation leaves room for: 5 = at most 96 VGPRs (12 bytes of scratch) and 5 x 31 KB of LDS per CU.  Round 3, same process, C3 / statue close-up: 4 waves (102 VGPRs) 133.6 / 1037 ms of k_trace per 256-spp step, 5 waves 126.9 / 983 (round 2's "5 and 6 blocks per CU are no faster" was measured on a 102-VGPR build, which the hardware never ran at more than 4) */
#endif
// occluder cache (jade_trace.h): the key of a yes/no query - k: its slot in the record (shadow ray towards emitter k, then the
// environment-visibility ray), d: its direction
static __device__ __forceinline__ uint32_t anyhit_key(uint32_t k, uint32_t n_emit, jvec3 d) {
  const uint32_t oct = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
  return k < n_emit ? (k != 0u ? 1u : 0u) : 2u + oct;
}
typedef uint32_t jade_v4u __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ uint4 ld_anyhit(const uint4* p) {
  const jade_v4u v = NT_LD(reinterpret_cast<const jade_v4u*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
// occluder cache: a query's walk starts with the cached subtrees - the lane's stack begins with them instead of the root
static __device__ __forceinline__ void anyhit_seed(WalkState& r, const LdsStack& stk, uint4 c) {
  uint32_t cur = JADE_REF_NONE, sp = stk.col;
  const uint32_t e4[4] = {c.w, c.z, c.y, c.x};  // way 0 is walked first: the others go under it
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool have = e4[i] != 0u, push = have && cur != JADE_REF_NONE;
    lds_st(push ? sp : stk.col + TW_DUMMY * JADE_COL_STRIDE, cur);
    sp += push ? JADE_COL_STRIDE : 0u;
    cur = have ? e4[i] - 1u : cur;
  }
  if (cur != JADE_REF_NONE) {
    r.cur = cur;
    r.sp = sp;
    r.skipx |= JADE_ATTEMPT;
  }
}
// WIDE: the walk may take wide units (jade_trace.h, "Wide walk"): k_trace_wide, launched instead of k_trace for renders with
// early exits on trees that have wide records.
// TAIL (k_tail): the kernel also SHADES - every wave owns 64 records of a short list and alternates, on its own, k_shade's pass over
// them (shade_record, the rays emitted into a stretch of the queue that is the wave's own) and this loop over those rays, until its
// records have run out of samples.  No other wave is waited for: what a render's last paths cost is their own chain of bounces,
// not one launch (and, at the end of a batch, one host wait) per bounce.
struct TailArgs {
  RenderConst R;
  const int32_t* tile_ids;
  uint32_t target_spp;
  const uint32_t* list;  // the records (the active list)
  uint32_t n_list;
  uint32_t* queue;       // a wave's stretch: 64 * nslots entries
};
template <bool WIDE, bool TAIL = false>
static __device__ __forceinline__ void trace_body(const DevScene& S, const PathState& P, const uint32_t* queue, QueueCtl* qc, uint32_t* spill, DevCounters* ctr,
                                                  uint32_t chunk, const TailArgs* tail = nullptr) {
  __shared__ uint32_t lds_cols[TW_END * JADE_TRACE_BLOCK];
  __shared__ __attribute__((aligned(8))) uint32_t lds_wq[JADE_TRACE_BLOCK / 64][2 * JADE_WQ];  // a wave's ring of leaves to test (jade_trace.h)
  __shared__ __attribute__((aligned(8))) uint32_t lds_hq[JADE_TRACE_BLOCK / 64][2 * JADE_HQ];  // and its ring of hit candidates  // a wave's queue of leaves to test (jade_trace.h)
  const int lane = threadIdx.x & 63;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  LdsStack stk;
  stk.lds = lds_cols + threadIdx.x;
  stk.col = lds_addr_of(stk.lds);
  stk.spill = spill + gtid;
  stk.stride_spill = gridDim.x * blockDim.x;
  stk.top = nullptr;
  stk.top_k = 0;
  stk.top4 = nullptr;
  stk.top4_k = 0;
  if (!TAIL && qc->count == 0) return;  // (a pass of a batch behind the one that ended the step: nothing was queued)
  // The grid is sized for a full queue (in a batch of passes the host does not know the length); a short queue keeps one
  // block per JADE_TRACE_BLOCK rays and the others leave before they stage anything: the thin passes at the end of a render
  // (under 10 k rays: 40 blocks instead of 1280) were mostly 1280 copies of the tree top into LDS.  The blocks that stay claim
  // chunks until the queue is empty, as ever.
  if (!TAIL && (unsigned long long)blockIdx.x * JADE_TRACE_BLOCK >= (unsigned long long)qc->count) return;
#if JADE_TRACE_TOP_NODES > 0 && JADE_LDS_TOP_NODES > 0
  static_assert(7 * JADE_TRACE_TOP4 <= 4 * JADE_TRACE_TOP_NODES, "the wide top shares the binary top's LDS");
  __shared__ float4 lds_top[4 * JADE_TRACE_TOP_NODES];
  if (WIDE) {
    // the top of the tree as wide records, seven planes (the eighth 16 bytes of a record are unused); a binary unit in this
    // kernel (a ray walked again after a tie, a ray with a non-finite 1/d) reads its records from memory
    const uint32_t k = S.top_k < JADE_TRACE_TOP4 ? S.top_k : JADE_TRACE_TOP4;
    for (uint32_t i = threadIdx.x; i < 8u * k; i += JADE_TRACE_BLOCK)
      if ((i & 7u) != 7u) lds_top[(i & 7u) * JADE_TRACE_TOP4 + (i >> 3)] = S.nodes4[i];
    __syncthreads();
    stk.top4 = lds_top;
    stk.top4_k = k;
    stk.top = lds_top;  // (node_fetch reads entry 0 of four planes for every lane and ignores it: top_k = 0)
    stk.top_k = 0;
  } else {  // stage the top of the tree: record i's j-th 16 bytes -> plane j, entry i (coalesced reads of S.nodes)
    const uint32_t k = S.top_k < JADE_TRACE_TOP_NODES ? S.top_k : JADE_TRACE_TOP_NODES;
    for (uint32_t i = threadIdx.x; i < 4u * k; i += JADE_TRACE_BLOCK) lds_top[(i & 3u) * JADE_TRACE_TOP_NODES + (i >> 2)] = S.nodes[i];
    __syncthreads();
    stk.top = lds_top;
    stk.top_k = k;
  }
#endif
  uint32_t n = TAIL ? 0u : qc->count;
  if (!TAIL && chunk == 0) {  // batched passes: the host has not seen the queue length (trace_chunk's rule, on the device)
    const uint32_t waves = gridDim.x * (JADE_TRACE_BLOCK / 64);
    uint32_t per = n / (waves * 64u * 8u);
    per = per < 1u ? 1u : (per > JADE_TRACE_CHUNK / 64 ? JADE_TRACE_CHUNK / 64 : per);
    chunk = per * 64u;
  }
  uint32_t V = 0, T = 0;  // wave totals (uniform: they live in SGPRs)
  uint32_t vcnt = 0, tcnt = 0;  // per lane, summed over the wave once at the end (a ballot + popcount per unit was 8 instructions)
  uint32_t ccnt = 0;            // ... queries answered by the occluder cache
  const bool anyhit = P.early_exit == 2u && S.anyhit != nullptr;  // (uniform)
  // wave-local chunk of the queue: [lbase, lend) (wave-uniform)
  uint32_t lbase = 0, lend = 0;
  bool queue_empty = false;
  bool active = false;  // this lane walks a ray, or waits for the last of its leaves to be tested
  bool wb = false;      // this lane's ray has ended and its result is still in the LDS column
  uint32_t my_e = 0;    // this lane's queue entry: the slot number, record * nslots + slot
  WalkState r;
  r.od.a = r.od.b = r.od.c = f2{0.0f, 0.0f};
  r.skipx = 0;
  r.cur = JADE_REF_NONE;
  r.sp = stk.col;
  r.pushed = 0;
  r.inv = jv(0, 0, 0);
#if JADE_PREFETCH
  r.pre.a = r.pre.b = r.pre.c = make_float4(0, 0, 0, 0);
  r.pre.rf = make_uint2(0u, 0u);
#endif
  WaveTrace wt;  // the wave's rings of leaves to test and of hit candidates, and the item this lane is testing (jade_trace.h)
  wt.init(lds_addr_of(&lds_wq[threadIdx.x >> 6][0]), lds_addr_of(&lds_hq[threadIdx.x >> 6][0]), lane, WIDE);
#if JADE_COOP_LEAF
  __shared__ __attribute__((aligned(16))) uint32_t lds_stage[JADE_TRACE_BLOCK / 64][64 * 20];
  wt.stage = lds_addr_of(&lds_stage[threadIdx.x >> 6][0]);
#endif
  TraceProf pr;
#if JADE_TRACE_PROFILE
  __shared__ __attribute__((aligned(8))) unsigned long long lds_prof[JADE_TRACE_BLOCK / 64][PL_N];
  pr.begin(lds_addr_of(reinterpret_cast<const uint32_t*>(&lds_prof[threadIdx.x >> 6][0])), lane);
#endif
  // ---- TAIL: this wave's records, and the totals of what shading them counts (shade_tail's counters, per wave here)
  int tail_p = P.npix;     // this lane's record (npix = none)
  bool tail_alive = false;
  unsigned long long tail_rays = 0;  // rays this wave traced (uniform)
  unsigned long long tc_primary = 0, tc_shadow = 0, tc_shaded = 0, tc_samples = 0, tc_env = 0, tc_ind = 0, tc_mirror = 0, tc_refract = 0;  // (valid in lane 0)
  if (TAIL) {
    const uint32_t wave_id = blockIdx.x * (JADE_TRACE_BLOCK / 64) + (threadIdx.x >> 6);
    const uint32_t t_idx = wave_id * 64u + (uint32_t)lane;
    if (t_idx < tail->n_list) {
      tail_p = (int)tail->list[t_idx];
      tail_alive = true;
    }
    queue = tail->queue + (size_t)wave_id * 64u * (uint32_t)P.nslots;
  }
  for (;;) {  // (TAIL: one turn per bounce of the wave's records; otherwise one turn)
  if (TAIL) {
    // ---- k_shade's pass over the wave's records: last turn's hit results folded in, the next bounce's rays emitted
    __threadfence();  // the results this wave's lanes wrote for each other's records
    ShadeCtx c;
    c.n_emit_rays = 0;
    c.c_primary = c.c_shadow = c.c_shaded = c.c_samples = c.c_cls = 0;
    uint32_t st = ST_INVALID;
    if (tail_alive) {
      bool defer;
      shade_record<false>(S, P, tail->R, tail->tile_ids, tail->target_spp, tail_p, c, st, defer);
      tail_alive = c.n_emit_rays > 0;  // a record without a ray in flight has run out of samples
    }
    tc_primary += wave_sum_u32(c.c_primary); tc_shadow += wave_sum_u32(c.c_shadow); tc_shaded += wave_sum_u32(c.c_shaded); tc_samples += wave_sum_u32(c.c_samples);
    tc_env += wave_sum_u32(c.c_cls & 255u); tc_ind += wave_sum_u32((c.c_cls >> 8) & 255u); tc_mirror += wave_sum_u32((c.c_cls >> 16) & 255u); tc_refract += wave_sum_u32(c.c_cls >> 24);
    if (__ballot(tail_alive) == 0ull) break;
    // the wave's rays, slot by slot as shade_tail queues them
    uint32_t m_rays = 0;
    const int used = !tail_alive ? 0 : (st == ST_DIFFUSE || st == ST_BSSRDF) ? P.nslots : 1;
    for (int k = 0; k < P.nslots; ++k) {
      const bool q = k < used && reinterpret_cast<const int*>(P.slot + ((size_t)tail_p * P.nslots + k))[3] != -2;
      const unsigned long long m = __ballot(q);
      if (q) const_cast<uint32_t*>(queue)[m_rays + wt.rank_in(m)] = (uint32_t)tail_p * (uint32_t)P.nslots + (uint32_t)k;
      m_rays += (uint32_t)__popcll(m);
    }
    __threadfence();  // rays and queue entries are read by other lanes of this wave
    n = m_rays;
    tail_rays += m_rays;
    lbase = 0;
    lend = n;
    queue_empty = false;
  }
  for (;;) {
    // ---- a ray has ended when its walk has and all the leaves it pushed have been finished
    if (active && WaveTrace::ray_ended(r, stk)) {
      // (occluder cache: the cached subtrees held no answer - the whole walk, from the root)
      const bool retry = (r.skipx & (JADE_ATTEMPT | JADE_CUT)) == JADE_ATTEMPT;
      // (wide walk: two leaves tied for this ray's best distance and the walk was not the reference's order - once more, with
      // binary units only; a ray that ended early has its answer whatever the order)
      const bool again = WIDE && lds_get(stk, TW_LIMIT) == JADE_LIMIT_TIE && (r.skipx & (JADE_CUT | JADE_FORCE_BINARY)) == 0u;
      if (retry || again) {
        // the ray is still in the lane's registers (origin, directions, source triangle, the limit in its column): only the walk
        // starts over - from the root, with nothing found (a hit of the first walk is found again; keeping it would mix the two
        // walks' leaf numbers in hitArray's tie rule).  No memory access: this runs whenever ANY lane of the wave restarts.
        walk_restart(r, stk, S);
        r.skipx = (r.skipx & ~JADE_ATTEMPT) | (retry ? 0u : JADE_FORCE_BINARY);
        if (WIDE && lds_get(stk, TW_LIMIT) == JADE_LIMIT_TIE)  // (rare: the tie marker sits where the limit was - the ray's own comes back from its slot)
          lds_putf(stk, TW_LIMIT, P.early_exit ? NT_LD(reinterpret_cast<const float*>(P.slot + (size_t)my_e) + 3) : __int_as_float(-1));
      } else {
        active = false;
        wb = true;
      }
    }
    // ---- once enough lanes are idle (or all are): write their results back and refill them.  Both are done for >=
    // JADE_REFILL_MIN lanes at a time, not whenever a single ray ends: a block of code that
    // runs for one lane costs as much as for 64.
    const unsigned long long idle = __ballot(!active);
    const int n_idle = __popcll(idle);
    PROF_DRAIN();
    PROF_LAP(pr, PL_TOP);
    if (n_idle >= JADE_REFILL_MIN) {
      PROF_COUNT(pr, PC_REFILLS, 1);
      if (wb) {
        // ray records stream through once per pass: non-temporal, so that they do not push the BVH out of the XCD's
        // 4 MB L2 (C3's node + vertex records are 4.1 MB; PMC: 124 of the 172 HBM bytes per ray were BVH lines re-fetched)
        float dist;
        jvec3 hp = jv(0, 0, 0);
        uint32_t parent1 = 0;
        // (a yes/no query gets the triangle alone: nobody reads its hit point - jade_device.h, PathState.hitp)
        const bool want_point = (r.skipx & JADE_WANTS_POINT) != 0u || P.write_all_hits != 0u;
        const int32_t best = walk_result(stk, S, r.od, &dist, &hp, &parent1, want_point);
        NT_ST(reinterpret_cast<int32_t*>(P.slot + (size_t)my_e) + 3, best);
        if (want_point) nt_st4(P.hitp + (size_t)(my_e / (uint32_t)P.nslots), hp.x, hp.y, hp.z, dist);  // (the hit point of a miss is never read; its distance stays INF, PathTrace.cu:799)
        if (anyhit) {
          // occluder cache: an answer the cached subtrees gave is counted; one that took the whole walk leaves its leaf's parent
          // in one of the key's four ways (a plain store: entries are hints)
          ccnt += (r.skipx & (JADE_CUT | JADE_ATTEMPT)) == (JADE_CUT | JADE_ATTEMPT) ? 1u : 0u;
          const uint32_t src = r.skipx & JADE_SKIP_MASK;
          const float lim = lds_getf(stk, TW_LIMIT);
          if ((r.skipx & (JADE_CUT | JADE_ATTEMPT | 0x80000000u)) == JADE_CUT && parent1 != 0u && lim == lim && src != JADE_SKIP_MASK) {
            const uint32_t k = my_e - (my_e / (uint32_t)P.nslots) * (uint32_t)P.nslots;
            const jvec3 dn = od_dn(r.od);
            const uint32_t key = anyhit_key(k, (uint32_t)S.n_emit, dn);
            const uint32_t way = (my_e * 2654435761u) >> 30;
            reinterpret_cast<uint32_t*>(S.anyhit)[((size_t)src * JADE_ANYHIT_KEYS + key) * 4u + way] = parent1;
          }
        }
        wb = false;
      }
      PROF_DRAIN();
      PROF_LAP(pr, PL_WRITEBACK);
      if (!queue_empty) {
        if (TAIL && lbase >= lend) queue_empty = true;  // (the wave's own stretch: nothing to claim.  Found here, with nothing taken -
        // not when the last entries are taken: the lanes that took them are counted idle by this turn of the loop)
        if (!TAIL && lbase >= lend) {
          uint32_t nb = 0;
          if (lane == 0) nb = atomicAdd(&qc->next, chunk);
          nb = __shfl(nb, 0, 64);
          if (nb >= n) {
            queue_empty = true;
            lbase = lend = n;
          } else {
            lbase = nb;
            lend = nb + chunk < n ? nb + chunk : n;
          }
        }
        const uint32_t avail = lend - lbase;
        const uint32_t take = (uint32_t)n_idle < avail ? (uint32_t)n_idle : avail;
        const uint32_t rank = wt.rank_in(idle);
        // (an ordered queue holds positions: PathState.idxq)
        uint32_t qpos = lbase + rank;
        if (!TAIL && P.idxq && !active && rank < take) qpos = NT_LD(&queue[lbase + rank]);
        if (!TAIL && !active && rank < take && qpos < P.rayq_cap) {
          // ---- the ray as a record (PathState.rayq): three 16-B loads (coalesced unless the queue is ordered), nothing to compute
          const float4* rq = P.rayq + (size_t)qpos * 3;
          const float4 r0 = nt_ld4(rq), r1 = nt_ld4(rq + 1), r2 = nt_ld4(rq + 2);
          my_e = __float_as_uint(r2.w);
          const uint32_t skipx = __float_as_uint(r0.w);
          const uint32_t src = skipx & JADE_SKIP_MASK;
          const bool anyq = anyhit && r1.w == r1.w && src != JADE_SKIP_MASK;
          uint4 c = make_uint4(0u, 0u, 0u, 0u);
          if (anyq) {
            const uint32_t p = my_e / (uint32_t)P.nslots;
            c = ld_anyhit(S.anyhit + (size_t)src * JADE_ANYHIT_KEYS + anyhit_key(my_e - p * (uint32_t)P.nslots, (uint32_t)S.n_emit, jv(r2.x, r2.y, r2.z)));
          }
          walk_begin_prepared(r, stk, S, jv(r0.x, r0.y, r0.z), jv(r1.x, r1.y, r1.z), jv(r2.x, r2.y, r2.z), skipx, r1.w);
          if (anyq && (int32_t)skipx >= 0) anyhit_seed(r, stk, c);
          active = true;
        } else if (!active && rank < take) {
          my_e = (!TAIL && P.idxq) ? NT_LD(&P.idxq[qpos]) : NT_LD(&queue[lbase + rank]);
          const uint32_t p = my_e / (uint32_t)P.nslots;  // the entry is the slot number p * nslots + k
          const float4 og = nt_ld4(&P.orgs[p]);
          const int32_t skip = __float_as_int(og.w);
          const jvec3 o = skip == JADE_SKIP_CAMERA ? jv(P.eye[0], P.eye[1], P.eye[2]) : jv(og.x, og.y, og.z);
          const float4 dv = nt_ld4(&P.slot[(size_t)my_e]);
          const jvec3 d = jv(dv.x, dv.y, dv.z);
          // occluder cache (jade_trace.h): a yes/no query starts with the subtrees in which the last such queries from this
          // triangle found their answer - the lane's stack begins with them instead of the root.  (The entry is requested before
          // walk_begin's arithmetic so that the two overlap.)
          const bool anyq = anyhit && dv.w == dv.w && skip >= 0;
          uint4 c = make_uint4(0u, 0u, 0u, 0u);
          if (anyq) c = ld_anyhit(S.anyhit + (size_t)skip * JADE_ANYHIT_KEYS + anyhit_key(my_e - p * (uint32_t)P.nslots, (uint32_t)S.n_emit, d));
          walk_begin(r, stk, S, o, d, skip, P.early_exit ? dv.w : __int_as_float(-1), dv.w);
          if (anyq && (int32_t)r.skipx >= 0) anyhit_seed(r, stk, c);  // (a ray with a non-finite 1/d takes the NaN-faithful walk from the root)
          active = true;
        }
        V += take;  // the root record of every ray started
        lbase += take;
      }
      PROF_DRAIN();
      PROF_LAP(pr, PL_REFILL);
    }
    if (n_idle == 64 && queue_empty) break;  // nothing in flight (so no leaf is waiting either), nothing left to claim
    // ---- one iteration of work for the wave: walk units, test units or a pass over the hit candidates (jade_trace.h)
    wt.template iterate<WIDE>(r, active, S, stk, vcnt, tcnt, pr);
  }
  if (!TAIL) break;
  }
  if (TAIL && lane == 0) {  // what shading counted (shade_tail's words of DevCounters)
    DevCounters* cs = ctr + (blockIdx.x % JADE_CTR_SHARDS);
    if (tc_primary) atomicAdd(&cs->rays_primary, tc_primary);
    if (tc_shadow) atomicAdd(&cs->rays_shadow, tc_shadow);
    if (tc_shaded) atomicAdd(&cs->shaded_hits, tc_shaded);
    if (tc_samples) atomicAdd(&cs->samples, tc_samples);
    if (tc_env) atomicAdd(&cs->rays_env, tc_env);
    if (tc_ind) atomicAdd(&cs->rays_indirect, tc_ind);
    if (tc_mirror) atomicAdd(&cs->rays_mirror, tc_mirror);
    if (tc_refract) atomicAdd(&cs->rays_refract, tc_refract);
  }
#if JADE_TRACE_PROFILE
  pr.count(PC_WAVES, 1);
  PROF_DRAIN();
  if (lane < PL_N) {
    const unsigned long long v = pr.get(lane);
    if (v) atomicAdd(&g_trace_prof[lane], v);
  }
#endif
  V += (uint32_t)wave_sum_u32(vcnt);  // (valid in lane 0, the only lane that uses it)
  T += (uint32_t)wave_sum_u32(tcnt);
  if (lane == 0) {
    DevCounters* cs = ctr + (blockIdx.x % JADE_CTR_SHARDS);
    if (V) atomicAdd(&cs->nodes_visited, (unsigned long long)V);
    if (T) atomicAdd(&cs->tris_tested, (unsigned long long)T);
    if (TAIL) {  // k_tail's own share (jade_stats.rays_tail ...): its rays are not k_trace's
      if (tail_rays) atomicAdd(&cs->rays_tail, tail_rays);
      if (V) atomicAdd(&cs->nodes_tail, (unsigned long long)V);
      if (T) atomicAdd(&cs->tris_tail, (unsigned long long)T);
    }
  }
  if (anyhit) {
    const uint32_t C = (uint32_t)wave_sum_u32(ccnt);
    if (lane == 0 && C) atomicAdd(&(ctr + (blockIdx.x % JADE_CTR_SHARDS))->rays_cached, (unsigned long long)C);
  }
}
__global__ __launch_bounds__(JADE_TRACE_BLOCK, JADE_TRACE_WAVES) void k_trace(DevScene S, PathState P, const uint32_t* queue, QueueCtl* qc,
                                                           uint32_t* spill, DevCounters* ctr, uint32_t chunk) {
  trace_body<false>(S, P, queue, qc, spill, ctr, chunk);
}
#ifndef JADE_TRACE_WIDE_WAVES
#define JADE_TRACE_WIDE_WAVES 4 /* 106 VGPRs, no scratch.  At 5 (96 VGPRs, 20 bytes of scratch) C5's k_trace takes 166.6 instead of 160.8 ms per step: the wide unit's four boxes want the registers more than the kernel wants the fifth wave */
#endif
__global__ __launch_bounds__(JADE_TRACE_BLOCK, JADE_TRACE_WIDE_WAVES) void k_trace_wide(DevScene S, PathState P, const uint32_t* queue, QueueCtl* qc,
                                                                uint32_t* spill, DevCounters* ctr, uint32_t chunk) {
  trace_body<true>(S, P, queue, qc, spill, ctr, chunk);
}
#ifndef JADE_TAIL_WAVES
#define JADE_TAIL_WAVES 2 /* k_tail holds k_shade's registers and k_trace's at once (152 VGPRs; at 4 waves per SIMD it spills 372 bytes); at most a few hundred waves ever run, so occupancy is not what it needs */
#endif
// k_tail: the end of a render's (or a small render's) paths in ONE launch - see TailArgs.  Binary units only: the walk is the
// reference's in every mode, and early exits work as in k_trace (the limit travels in the slot).
__global__ __launch_bounds__(JADE_TRACE_BLOCK, JADE_TAIL_WAVES) void k_tail(DevScene S, PathState P, TailArgs tail, uint32_t* spill, DevCounters* ctr) {
  trace_body<false, true>(S, P, nullptr, nullptr, spill, ctr, 64u, &tail);
}
// which of the two a launch takes: wide units need early exits (the order of the walk is then nobody's business but a tie's) and
// a tree with wide records
static inline bool trace_wide(const DevScene& S, const PathState& P) { return JADE_WIDE_WALK && P.early_exit && S.nodes4 != nullptr; }

// ACESToneMapping + gamma + BGR pack, PathTrace.cu:680-682, 1457-1473.
// tile_inv (nullable): 1 / samples of each owned tile, after jade_render_adaptive; otherwise every tile has inv_spp
__global__ void k_resolve(PathState P, RenderConst R, const int32_t* tile_ids, const float* tile_inv, float inv_spp, int tonemap, float limit,
                          float* out_rgb, uint8_t* out_bgr) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;  // owned pixel
  if (p >= P.npx) return;
  if (tile_inv) inv_spp = tile_inv[p >> 8];
  int px_, py_;
  bool valid = pixel_xy(R, tile_ids, p, &px_, &py_);
  jvec3 m = jv(0, 0, 0);
  if (valid) {
    // add the JADE_SAMPLE_LANES partial sums in lane order (jade_rt.h)
    const size_t sn = (size_t)P.sum_lanes * (size_t)P.npx;
    jvec3 s = ld3w(P.sum, sn, (size_t)p);
    for (int l = 1; l < P.sum_lanes; ++l) s = jv_add(s, ld3w(P.sum, sn, (size_t)l * (size_t)P.npx + (size_t)p));
    // lanes the render never needed are not kept (PathState.sum_lanes): they would all be +0.0, and adding +0.0 any number
    // of times is adding it once (it only turns a -0.0 total into +0.0)
    if (P.sum_lanes < JADE_SAMPLE_LANES) s = jv_add(s, jv(0.0f, 0.0f, 0.0f));
    m = jv(s.x * inv_spp, s.y * inv_spp, s.z * inv_spp);
  }
  if (out_rgb) {
    out_rgb[3 * (size_t)p] = m.x;
    out_rgb[3 * (size_t)p + 1] = m.y;
    out_rgb[3 * (size_t)p + 2] = m.z;
  }
  if (out_bgr) tone_pack_bgr8(m, tonemap, limit, valid, out_bgr + 3 * (size_t)p);
}

// ---------------------------------------------------------------- host side --

static thread_local std::string g_err;
int jade_fail(int code, const std::string& msg) {  // jade_runtime.h
  g_err = msg;
  return code;
}

#ifndef JADE_PACKET_GIVE_UP_LIMIT
#define JADE_PACKET_GIVE_UP_LIMIT 0.25 /* share of a step's packets given up above which the next steps of the render use the per-lane first pass */
#endif

// (the entry points below have C linkage from their declarations in jade_rt.h / jade_bvh.h)

int jade_abi_version(void) { return JADE_ABI_VERSION; }
const char* jade_backend_name(void) { return "hip-gfx950"; }
const char* jade_last_error(void) { return g_err.c_str(); }

int jade_device_count(int* n) {
  if (!n) return jade_fail(JADE_ERR_INVALID, "null argument");
  *n = 0;
  HIP_TRY(hipGetDeviceCount(n));
  return JADE_OK;
}

int jade_owned_tile_count(int32_t width, int32_t height, int32_t rank, int32_t nranks) {
  if (width <= 0 || height <= 0 || nranks <= 0 || rank < 0 || rank >= nranks) return -1;
  int tx = (width + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE, ty = (height + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE;
  int count = 0;
  for (int y = 0; y < ty; ++y)
    for (int x = 0; x < tx; ++x) count += (x + y) % nranks == rank;
  return count;
}

// uploads what prepare_scene made and the caller's own arrays, and points s->dev at them
static int upload_scene(jade_scene* s, const jade_scene_desc* d, const ScenePrep& p) {
  hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = upload(s->b_nodes, p.nodes.data(), p.nodes.size(), s->stream);
  if (e == hipSuccess && !p.nodes4.empty()) e = upload(s->b_nodes4, p.nodes4.data(), p.nodes4.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_tverts, p.tverts.data(), p.tverts.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_tris, d->triangles, (size_t)d->n_triangles, s->stream);
  if (e == hipSuccess) e = upload(s->b_emit, d->emit_indices, (size_t)d->n_emit, s->stream);
  if (e == hipSuccess) e = upload(s->b_mapping, d->index_mapping, (size_t)d->n_triangles, s->stream);
  if (e == hipSuccess) e = upload(s->b_prefix, d->prefix_area, (size_t)d->n_triangles, s->stream);
  if (e == hipSuccess) e = upload(s->b_segs, d->obj_segs, (size_t)d->n_objects, s->stream);
  if (e == hipSuccess) e = upload(s->b_env, d->env_rgb, (size_t)3 * d->env_width * d->env_height, s->stream);
  if (e == hipSuccess) e = upload(s->b_env_alias, p.env_alias.data(), p.env_alias.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_light_alias, p.light_alias.data(), p.light_alias.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_mis, p.mis.data(), p.mis.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_tnorm, p.tnorm.data(), p.tnorm.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_mats, p.mats.data(), p.mats.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_guide, p.guide.data(), p.guide.size(), s->stream);
  if (e == hipSuccess) e = upload(s->b_guide_obj, p.guide_obj.data(), p.guide_obj.size(), s->stream);
  const bool want_anyhit = s->tun.anyhit && p.nested && p.cache_fits && !p.missing_child && p.n_internal > 1;
  if (e == hipSuccess && want_anyhit) {
    e = s->b_anyhit.alloc((size_t)d->n_triangles * JADE_ANYHIT_KEYS * sizeof(uint4));
    if (e == hipSuccess) e = hipMemsetAsync(s->b_anyhit.p, 0, s->b_anyhit.bytes, s->stream);
  }
  if (e == hipSuccess) e = s->b_ctl.alloc(sizeof(QueueCtl) * (JADE_CTL_RING + 1));  // (+ 1: k_arm's count when the host does not wait for it)
  if (e == hipSuccess) e = s->b_ctr.alloc(sizeof(DevCounters) * JADE_CTR_SHARDS);
  if (e != hipSuccess)
    return jade_fail(e == hipErrorOutOfMemory ? JADE_ERR_NOMEM : JADE_ERR_DEVICE, std::string("scene upload: ") + hipGetErrorString(e));
  s->dev.nodes = s->b_nodes.as<float4>();
  s->dev.nodes4 = p.nodes4.empty() ? nullptr : s->b_nodes4.as<float4>();
  s->dev.tverts = s->b_tverts.as<float4>();
  s->dev.tris = s->b_tris.as<jade_triangle>();
  s->dev.emit = s->b_emit.as<int32_t>();
  s->dev.mapping = s->b_mapping.as<int32_t>();
  s->dev.prefix = s->b_prefix.as<float>();
  s->dev.segs = s->b_segs.as<jade_obj_seg>();
  s->dev.env = s->b_env.as<float>();
  s->dev.tnorm = s->b_tnorm.as<float4>();
  s->dev.mats = s->b_mats.as<DevMaterial>();
  s->dev.guide = s->b_guide.as<uint32_t>();
  s->dev.guide_obj = s->b_guide_obj.as<uint2>();
  s->dev.env_w = d->env_width;
  s->dev.env_h = d->env_height;
  s->dev.n_tris = d->n_triangles;
  s->dev.n_emit = d->n_emit;
  s->dev.root_ref = p.root_ref;
  s->dev.top_k = (uint32_t)std::min(p.n_internal, (int)JADE_LDS_TOP_NODES);
  s->dev.general_walk = p.missing_child ? 1u : 0u;
  s->dev.anyhit = want_anyhit ? s->b_anyhit.as<uint4>() : nullptr;
  s->dev.env_alias = s->b_env_alias.as<uint4>();
  s->boxes_nested = p.nested;
  // Ray ordering pays when the traversal's records do not fit the XCDs' L2s (C5: 55 MB, k_trace bound by the rate of 64-B sector
  // misses: 4 235 -> 5 275 Mray/s); on a tree that does (C3: 3.8 MB) it costs more than it gives
  s->sort_rays = s->tun.sort_mode < 0 ? p.geometry_bytes > JADE_SORT_GEOMETRY_BYTES : s->tun.sort_mode > 0;
  return JADE_OK;
}

// blocks per CU a persistent kernel gets: what the occupancy query allows, at least 1, at most `cap`
template <class K>
static int blocks_per_cu(K kernel, int cap) {
  int n = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, JADE_TRACE_BLOCK, 0);
  return std::min(std::max(n, 1), cap);
}

// persistent grids: as many blocks per CU as registers and the LDS columns (20 KB/block) allow
static int size_grids(jade_scene* s, int depth) {
  hipDeviceProp_t prop;
  if (hipError_t pe = hipGetDeviceProperties(&prop, s->device); pe != hipSuccess)
    return jade_fail(JADE_ERR_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(pe));
  int per_cu = blocks_per_cu(k_trace, 8);
  if (s->tun.trace_blocks_per_cu >= 1 && s->tun.trace_blocks_per_cu < per_cu) per_cu = s->tun.trace_blocks_per_cu;  // development: occupancy sweeps
  if (s->tun.log_passes) fprintf(stderr, "[jade] k_trace: %d blocks of %d threads per CU, %d CUs\n", per_cu, JADE_TRACE_BLOCK, prop.multiProcessorCount);
  s->trace_blocks = prop.multiProcessorCount * per_cu;
  // k_trace_wide keeps fewer waves: its own grid; it and k_light stay within k_trace's (the stack spill area is sized for that one)
  s->trace_blocks_wide = prop.multiProcessorCount * blocks_per_cu(k_trace_wide, per_cu);
  s->light_blocks = prop.multiProcessorCount * blocks_per_cu(k_light, per_cu);
  if (depth <= JADE_PACKET_MAX_DEPTH) s->packet_blocks = prop.multiProcessorCount * blocks_per_cu(k_light_packet, 8);
  if (s->tun.log_passes) fprintf(stderr, "[jade] first pass: k_light %d blocks, k_light_packet %d blocks (tree depth %d)\n", s->light_blocks, s->packet_blocks, depth);
  return JADE_OK;
}

// the arithmetic contract of jade_fpmath.h, checked on the device once
static int selftest(jade_scene* s) {
  hipLaunchKernelGGL(k_selftest, dim3(1), dim3(1), 0, s->stream, s->b_ctl.as<QueueCtl>(), 1.0f);
  QueueCtl qc{};
  hipError_t e = hipMemcpyAsync(&qc, s->b_ctl.p, sizeof qc, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return jade_fail(JADE_ERR_DEVICE, std::string("selftest: ") + hipGetErrorString(e));
  if (qc.fp_bad) return jade_fail(JADE_ERR_DEVICE, "device code was built with FP contraction on (see include/jade_fpmath.h)");
  return JADE_OK;
}

int jade_scene_create(const jade_scene_desc* d, int device_id, jade_scene** out) {
  if (!d || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  int depth = 0;
  int rc = validate_desc(d, &depth);
  if (rc) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return jade_fail(JADE_ERR_DEVICE, "no such HIP device");
  HIP_TRY(hipSetDevice(device_id));
  Tunables tun;
  tun.read();
  ScenePrep prep;
  if ((rc = prepare_scene(*d, depth, tun, &prep))) return rc;
  std::unique_ptr<jade_scene> s(new (std::nothrow) jade_scene());
  if (!s) return jade_fail(JADE_ERR_NOMEM, "out of memory");
  s->device = device_id;
  s->tun = tun;
  s->n_emit = d->n_emit;
  s->n_objects = d->n_objects;
  s->bvh_depth = depth;
  if ((rc = upload_scene(s.get(), d, prep))) return rc;
  if ((rc = selftest(s.get()))) return rc;
  if ((rc = size_grids(s.get(), depth))) return rc;
  *out = s.release();
  return JADE_OK;
}

void jade_scene_destroy(jade_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}

static int setup_state(jade_scene* s, int npx, int rpp, int nslots, int sum_lanes) {
  const int npix = npx * rpp;
  // carve every per-pixel array out of one allocation
  size_t words = 0;
  auto take = [&](size_t n) { size_t o = words; words += (n + 63) & ~(size_t)63; return o; };
  const size_t N = (size_t)npix, K = (size_t)nslots;
  size_t o_hdr = take(4 * N), o_ctx = take(16 * N), o_aux = take(4 * N), o_orgs = take(4 * N), o_slot = take(4 * K * N), o_hitp = take(4 * N);
  HIP_TRY(s->b_state.alloc(words * 4));
  HIP_TRY(hipMemsetAsync(s->b_state.p, 0, words * 4, s->stream));
  // the partial sums are an allocation of their own: they grow if steps add more samples than were announced (grow_sums)
  HIP_TRY(s->b_sum.alloc((size_t)3 * sum_lanes * npx * 4));
  HIP_TRY(hipMemsetAsync(s->b_sum.p, 0, (size_t)3 * sum_lanes * npx * 4, s->stream));
  uint32_t* b = s->b_state.as<uint32_t>();
  PathState& P = s->ps;
  P.npix = npix;
  P.npx = npx;
  P.rpp = rpp;
  {
    // Pixel rotation is OFF by default: measured on C3 it cuts the passes per 256-sample block
    // from 172 to 142 but de-synchronised records lose coalescing and ray coherence in the
    // heavy passes (2155 vs 2229 Mray/s).  JADE_PIXEL_ROTATE=1 turns it on for experiments.
    const int per = JADE_SAMPLE_LANES / rpp;
    P.stride = (s->tun.pixel_rotate && per > 1) ? (npx / per) | 1 : 0;
  }
  P.nslots = nslots;
  P.hdr = (uint4*)(b + o_hdr);
  P.sum_lanes = sum_lanes;
  P.sum = s->b_sum.as<float>(); P.ctx = (float4*)(b + o_ctx); P.aux = (float4*)(b + o_aux); P.orgs = (float4*)(b + o_orgs);
  P.slot = (float4*)(b + o_slot);
  P.hitp = (float4*)(b + o_hitp);
  P.write_all_hits = 0u;
  HIP_TRY(s->b_queue.alloc(K * N * 4));
  // ray records for the head of the queue (PathState.rayq): as many as an eighth of all slots - a pass after the fused first one
  // queues rays for a few per cent of the records - but every slot of a small render; none when switched off
  {
    const size_t cap = ray_record_cap(K * N, s->tun.ray_records, 0);
    if (cap) HIP_TRY(s->b_rayq.alloc(cap * 48));
    P.rayq = cap ? s->b_rayq.as<float4>() : nullptr;
    // (JADE_RAYQ_CAP lowers the boundary, not the allocation: a position either side of a lowered boundary is still inside b_rayq)
    P.rayq_cap = (uint32_t)std::min<size_t>(ray_record_cap(K * N, s->tun.ray_records, s->tun.rayq_cap), 0xffffffffu);
  }
  // b_active[0] doubles as k_light's per-wave hand-over regions: up to 64 records of slack per wave of its grid
  const size_t first_pass_blocks = (size_t)std::max(s->light_blocks, s->packet_blocks);
  HIP_TRY(s->b_active[0].alloc((N + first_pass_blocks * JADE_TRACE_BLOCK + 64) * 4));
  HIP_TRY(s->b_active[1].alloc(N * 4));
  HIP_TRY(s->b_wavecnt.alloc((size_t)2 * first_pass_blocks * (JADE_TRACE_BLOCK / 64) * 4));
  s->sort_cap = 0;
  P.keyq = nullptr;
  P.keyq_cap = 0;
  P.key_tri_bits = 1;
  if (s->sort_rays) {
    const size_t cap = std::min<size_t>(K * N, (size_t)1 << 28);
    size_t tmp = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, cap, 0u, 32u, s->stream));
    HIP_TRY(s->b_sortkey.alloc(cap * 4));
    HIP_TRY(s->b_sortkey2.alloc(cap * 4));
    HIP_TRY(s->b_sortpos.alloc(cap * 4));
    HIP_TRY(s->b_sortq.alloc(cap * 4));
    HIP_TRY(s->b_sorttmp.alloc(tmp));
    s->sort_tmp_bytes = tmp;
    s->sort_cap = cap;
    P.keyq = s->tun.sort_keys_kernel ? nullptr : s->b_sortkey.as<uint32_t>();
    P.keyq_cap = s->tun.sort_keys_kernel ? 0u : (uint32_t)std::min<size_t>(cap, 0xffffffffu);
    while (P.key_tri_bits < 23 && ((uint32_t)(s->dev.n_tris - 1) >> P.key_tri_bits)) ++P.key_tri_bits;
    // the queueing kernel writes the keys itself (PathState.keyq); the positions the sort moves with them are 0 .. cap-1, made once
    hipLaunchKernelGGL(k_iota, dim3(1024), dim3(256), 0, s->stream, s->b_sortpos.as<uint32_t>(), (uint32_t)std::min<size_t>(cap, 0xffffffffu));
    HIP_TRY(hipGetLastError());
  }
  // The stack spill area: level k >= JADE_LDS_STACK of thread gtid is word (k - JADE_LDS_STACK) * grid threads + gtid, so the last level an
  // accepted tree can fill (JADE_BVH_STACK_CAPACITY - 1) ends below these 120 x (k_trace's grid) words for every kernel whose grid is
  // no larger than k_trace's: k_trace_wide and k_light (size_grids), k_tail (run_passes clamps its list), the guide pass and
  // jade_trace_rays (launch_trace).  tests/test_gpu_deep_trees.py::test_grids_stay_within_the_spill_area holds the grids to it.
  if (!s->b_spill.p)
    HIP_TRY(s->b_spill.alloc((size_t)(JADE_BVH_STACK_CAPACITY - JADE_LDS_STACK) * s->trace_blocks * JADE_TRACE_BLOCK * 4));
  return JADE_OK;
}

int jade_render_begin(jade_scene* s, const jade_render_params* rp) {
  if (!s || !rp) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (rp->width <= 0 || rp->height <= 0 || rp->tile_nranks <= 0 || rp->tile_rank < 0 || rp->tile_rank >= rp->tile_nranks)
    return jade_fail(JADE_ERR_INVALID, "bad image size or tile partition");
  if (rp->walk != JADE_WALK_REFERENCE && rp->walk != JADE_WALK_EARLY_EXIT && rp->walk != JADE_WALK_EARLY_EXIT_CACHED)
    return jade_fail(JADE_ERR_INVALID, "unknown walk (JADE_WALK_*)");
  if (rp->env_sampling != JADE_ENV_REFERENCE && rp->env_sampling != JADE_ENV_IMPORTANCE && rp->env_sampling != JADE_ENV_MIXTURE)
    return jade_fail(JADE_ERR_INVALID, "unknown env_sampling (JADE_ENV_*)");
  if (rp->env_sampling != JADE_ENV_REFERENCE && !env_importance_fits(s->dev.env_w, s->dev.env_h))  // (the mixture draws from the same table)
    return jade_fail(JADE_ERR_UNSUPPORTED, "env_sampling: JADE_ENV_IMPORTANCE takes environment maps of at most 2^24 texels (JADE_ENV_IMPORTANCE_MAX_TEXELS)");
  if (s->light_sampling == JADE_LIGHTS_ONE && !light_sampling_fits(s->n_emit))
    return jade_fail(JADE_ERR_UNSUPPORTED, "light sampling: JADE_LIGHTS_ONE takes at most 2^24 emitter entries (JADE_LIGHTS_ONE_MAX_ENTRIES)");
  // the scene's settings as they are now make the render's mode, if that mode is built (shade_mode_for, jade_runtime.h)
  uint32_t mode = 0;
  std::string why;
  if (const int rc = shade_mode_for(rp->env_sampling, s->lens.aperture_radius > 0.0f, s->shutter_set, s->light_sampling, s->bounce_sampling,
                                    s->direct_sampling, &mode, &why, s->passes, s->branch_sampling == JADE_BRANCH_STRATIFIED, s->surf.set.normals_any,
                                    s->surf.set.textures.any, s->surf.set.maps.any))
    return jade_fail(rc, why);
  if ((mode & SM_PASSES) && s->tun.pixel_rotate)
    return jade_fail(JADE_ERR_UNSUPPORTED, "passes (jade_scene_set_passes) with JADE_PIXEL_ROTATE (a record's samples move between pixels)");
  HIP_TRY(hipSetDevice(s->device));
  if (const int rc = surface_begin(s, mode)) return rc;  // the surface tables the render reads (jade_surface.hip)
  const int tx = (rp->width + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE, ty = (rp->height + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE;
  s->tile_ids.clear();
  for (int y = 0; y < ty; ++y)
    for (int x = 0; x < tx; ++x)
      if ((x + y) % rp->tile_nranks == rp->tile_rank) s->tile_ids.push_back(y * tx + x);
  // the record's layout: a shadow slot per emitter entry - or one for the entry drawn (JADE_LIGHTS_ONE) -, the environment ray's, the indirect ray's
  const int nslots = ((mode & SM_LIGHTS) ? std::min(s->n_emit, 1) : s->n_emit) + 2;
  const int64_t npx64 = (int64_t)s->tile_ids.size() * 256;
  // Records per pixel: as many paths in flight as JADE_RECORD_MEMORY of the free device memory holds (the
  // partial sums come out of the same share), whatever the image share of this GPU: more records = fewer,
  // wider passes.  288 GB is what makes 530 M paths (112 GB) for a full 1080p frame affordable.
  const double bytes_per_record = 4.0 * (34 + 5 * nslots) + (s->tun.ray_records ? 6.0 * nslots : 0.0) +
                                  ((mode & SM_PASSES) ? 28.0 * PASS_COUNT + 4.0 : 0.0);  // (passes: a float4 and three floats per pass, one word; jade_shade.h PassPlanes)
  // PathState (a float4 per slot, one hit point per record) + queue entry + two list entries + 48-B ray records for an eighth of the slots
  // partial sums per pixel: one lane per sample up to JADE_SAMPLE_LANES, never more than the render was announced with
  // (rounded up to a power of two): a 1-spp 4K frame is 100 MB of sums, not 102 GB
  int sum_lanes = JADE_SAMPLE_LANES;
  if (rp->spp > 0)
    for (sum_lanes = 1; sum_lanes < rp->spp && sum_lanes < JADE_SAMPLE_LANES;) sum_lanes <<= 1;
  const double sums_bytes = 12.0 * sum_lanes * (double)npx64;
  // A render that keeps no passes gives the planes and images of an earlier one back before the memory is measured: they are up to
  // 424 B per record of that render, and a handle must not hold them for life.  The earlier render ends here - its shade kernels
  // would write to them - so a begin that fails below leaves no render in progress, as one that fails in setup_state does.
  if (!(mode & SM_PASSES) && (s->b_pass_cur.p || s->b_pass_tot.p || s->b_pass_mask.p || s->b_pass_out.p)) {
    s->have_rp = false;
    passes_release(s);
  }
  size_t mem_free = 0, mem_total = 0;
  HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
  mem_free += s->b_state.bytes + s->b_sum.bytes + s->b_queue.bytes + s->b_rayq.bytes + s->b_active[0].bytes + s->b_active[1].bytes +
              s->b_pass_cur.bytes + s->b_pass_tot.bytes + s->b_pass_mask.bytes;  // ours to reuse
  // the caller's bound (jade_render_params.max_state_bytes) replaces the default share of the free memory
  double state_budget = JADE_RECORD_MEMORY * (double)mem_free;
  if (rp->max_state_bytes) state_budget = std::min((double)rp->max_state_bytes, 0.95 * (double)mem_free);
  const double budget = state_budget - sums_bytes;
  // never more records per pixel than samples this render was announced with (rounded up to a power of two):
  // a 64-spp render of a small image must not claim, clear and scan gigabytes of records that never get a sample
  int rpp = JADE_SAMPLE_LANES;
  if (rp->spp > 0)
    for (rpp = 1; rpp < rp->spp && rpp < JADE_SAMPLE_LANES;) rpp <<= 1;
  // (3 * npix must fit an int: the three planes of a per-record vec3 are indexed with int arithmetic)
  while (rpp > 1 && ((double)npx64 * rpp * bytes_per_record > budget || npx64 * rpp * nslots >= ((int64_t)1 << 32) ||
                     npx64 * rpp * 3 >= ((int64_t)1 << 31)))
    rpp >>= 1;
  if (const int v = s->tun.records_per_pixel; v >= 1 && v <= JADE_SAMPLE_LANES && (v & (v - 1)) == 0) {  // test hook: results must not depend on it
    rpp = v;
    if (sum_lanes < rpp) sum_lanes = rpp;
  }
  const int64_t npix64 = npx64 * rpp;
  if (npix64 * nslots >= ((int64_t)1 << 32) || npix64 * 3 >= ((int64_t)1 << 31))
    return jade_fail(JADE_ERR_UNSUPPORTED, "pixels x records x (emitters + 2) exceeds the 32-bit ray-slot index");  // (JADE_LIGHTS_ONE: x 3 at most)
  if (sums_bytes + (double)npix64 * bytes_per_record > (rp->max_state_bytes ? std::max(state_budget, 0.0) : 0.95 * (double)mem_free))
    return jade_fail(JADE_ERR_NOMEM, rp->max_state_bytes ? "frame does not fit max_state_bytes (partial sums + one record per pixel)"
                                                    : "frame does not fit the device memory (partial sums + one record per pixel)");
  if (s->tun.log_passes)
    fprintf(stderr, "[jade] %lld pixels x %d records, %.1f GB of path state + %.1f GB of partial sums in %d lanes (%.0f GB free)\n", (long long)npx64,
            rpp, npix64 * bytes_per_record / 1e9, 12.0 * sum_lanes * (double)npx64 / 1e9, sum_lanes, mem_free / 1e9);
  s->have_rp = false;
  s->rp = *rp;
  RenderConst& R = s->rc;
  R.width = rp->width; R.height = rp->height; R.tiles_x = tx; R.frame = rp->frame;
  memcpy(R.eye, rp->eye, sizeof R.eye);
  memcpy(R.cam, rp->camera, sizeof R.cam);
  R.two_over_w = 2.0 / (double)rp->width;
  R.two_over_h = 2.0 / (double)rp->height;
  R.aspect = (double)rp->width / (double)rp->height;
  // the scene's lens as it is now: the render keeps it whatever jade_scene_set_lens is told before the next begin
  R.lens_radius = s->lens.aperture_radius > 0.0f ? s->lens.aperture_radius : 0.0f;
  const float lens_k = R.lens_radius > 0.0f ? s->lens.focus_distance / 1.5f : 0.0f;  // k of the statement: one float division
  s->spp_done = 0;
  s->tail_pending = false;
  s->carried_active = 0;
  s->packets_given_up = 0;
  s->rays_recorded = s->rays_indexed = 0;
  s->tile_n.clear();
  s->adaptive_done = false;
  s->dn_carried = jade_stats{};
  // ... its mode, and with it its shutter: the constants of the statement, one float subtraction each
  s->mode = mode;
  s->sh = (mode & SM_SHUTTER) ? shutter_const(rp->eye, rp->camera, s->shutter.eye_close, s->shutter.camera_close, s->shutter.t_open, s->shutter.t_close) : ShutterConst{};
  if (npix64 == 0) { s->ps.npix = 0; s->ps.npx = 0; s->have_rp = true; return JADE_OK; }
  int rc = setup_state(s, (int)npx64, rpp, nslots, sum_lanes);
  if (rc) return rc;
  if (mode & SM_PASSES)
    if ((rc = passes_setup(s, (size_t)npix64))) return rc;
  s->ps.early_exit = rp->walk == JADE_WALK_EARLY_EXIT_CACHED ? 2u : rp->walk == JADE_WALK_EARLY_EXIT ? 1u : 0u;
  s->ps.env_sampling = rp->env_sampling != JADE_ENV_REFERENCE ? 1u : 0u;  // (either mode may leave a bounce without a ray: shade_record)
  memcpy(s->ps.eye, rp->eye, sizeof s->ps.eye);
  s->ps.lens_k = lens_k;  // (setup_state wrote the record layout into s->ps)
  HIP_TRY(upload(s->b_tiles, s->tile_ids.data(), s->tile_ids.size(), s->stream));
  HIP_TRY(hipMemsetAsync(s->b_ctr.p, 0, sizeof(DevCounters) * JADE_CTR_SHARDS, s->stream));
  hipLaunchKernelGGL(k_init, dim3((unsigned)((npix64 + 255) / 256)), dim3(256), 0, s->stream, s->ps);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->have_rp = true;
  return JADE_OK;
}

static hipError_t sum_counters(jade_scene* s, DevCounters* out) {
  std::vector<DevCounters> sh(JADE_CTR_SHARDS);
  hipError_t e = hipMemcpyAsync(sh.data(), s->b_ctr.p, sizeof(DevCounters) * JADE_CTR_SHARDS, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  memset(out, 0, sizeof *out);
  for (const DevCounters& c : sh) {
    out->rays_primary += c.rays_primary; out->rays_shadow += c.rays_shadow;
    out->nodes_visited += c.nodes_visited; out->tris_tested += c.tris_tested;
    out->shaded_hits += c.shaded_hits; out->samples += c.samples;
    out->rays_env += c.rays_env; out->rays_indirect += c.rays_indirect;
    out->rays_mirror += c.rays_mirror; out->rays_refract += c.rays_refract;
    out->rays_inline += c.rays_inline;
    out->nodes_inline += c.nodes_inline; out->tris_inline += c.tris_inline;
    out->rays_cached += c.rays_cached;
    out->rays_tail += c.rays_tail; out->nodes_tail += c.nodes_tail; out->tris_tail += c.tris_tail;
    out->pad[0] += c.pad[0]; out->pad[1] += c.pad[1];
  }
  return e;
}

// ---- run_passes: the schedule of one step / flush ----

// The shade kernels of a mode as the passes launch them: `full` over a list (launch_shade), `lean` over all records, handing over to
// heavy_out / qc->heavy (shade_pass).  One per built mode: shade_launcher.
struct ShadeLaunch {
  void (*full)(jade_scene* s, uint32_t target_spp, unsigned blocks, const uint32_t* list, uint32_t n, const uint32_t* n_dev, uint32_t* next, QueueCtl* ctl,
               const QueueCtl* prev, uint32_t stop_below);
  void (*lean)(jade_scene* s, uint32_t target_spp, uint32_t* heavy_out, QueueCtl* qc);
};
// the kernel that runs mode M: its own, but the shutter kernels handle "with a lens" themselves (R.lens_radius)
static constexpr uint32_t shade_kernel_mode(uint32_t M) { return (M & SM_SHUTTER) ? M & ~(uint32_t)SM_LENS : M; }
// the argument the kernels of mode K take beyond the parity kernels' (ShadeArgs, jade_shade.h), filled from the scene: a line per member
template <uint32_t K>
static ShadeArgs<K> mode_args(const jade_scene* s) {
  ShadeArgs<K> a{};
  if constexpr (sm(K, SM_PASSES)) a.planes = PassPlanes{s->b_pass_cur.as<float4>(), s->b_pass_tot.as<float>(), s->b_pass_mask.as<uint32_t>(), (uint32_t)s->ps.npix};
  if constexpr (sm(K, SM_SHUTTER)) a.shutter = s->sh;
  if constexpr ((K & (SM_LIGHTS | SM_COSINE | SM_MIS)) != 0) a.light_table = s->b_light_alias.as<uint4>();
  if constexpr (sm(K, SM_MIS)) a.mis_table = s->b_mis.as<float2>();
  if constexpr (sm(K, SM_NMAP))
    a.map_tables = map_tables(s);
  else if constexpr (sm(K, SM_TEX))
    a.tex_tables = texture_tables(s);
  else if constexpr (sm(K, SM_SMOOTH)) a.smooth_table = smooth_table(s);
  return a;
}
template <uint32_t M>
static void launch_full(jade_scene* s, uint32_t target_spp, unsigned blocks, const uint32_t* list, uint32_t n, const uint32_t* n_dev, uint32_t* next,
                        QueueCtl* ctl, const QueueCtl* prev, uint32_t stop_below) {
  constexpr uint32_t K = shade_kernel_mode(M);
  auto go = [&](auto kernel, auto... a) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(JADE_SHADE_BLOCK), 0, s->stream, s->dev, s->ps, s->rc, s->b_tiles.as<int32_t>(), target_spp, list, n, n_dev,
                       next, s->b_queue.as<uint32_t>(), ctl, s->b_ctr.as<DevCounters>(), prev, stop_below, a...);
  };
  // the parity mode: k_shade, or - JADE_SHADE_BINNED - with the records dealt by branch through LDS (k_shade_binned), the one mode with that form
  if constexpr (K == 0) go(s->tun.shade_binned ? k_shade_binned : k_shade);
  else if constexpr (!sm(K, SM_MIS)) go(k_shade_mode<K, ShadeArgs<K>>, mode_args<K>(s));
  else if constexpr (const ShadeArgs<K> a = mode_args<K>(s); sm(K, SM_PASSES)) go(k_shade_mode<K, ArgPlanes, ArgLights, ArgMis>, (ArgPlanes)a, (ArgLights)a, (ArgMis)a);
  else go(k_shade_mode<K, ArgLights, ArgMis>, (ArgLights)a, (ArgMis)a);  // SM_MIS: the bundle's members apart (k_shade_mode)
}
template <uint32_t M>
static void launch_lean(jade_scene* s, uint32_t target_spp, uint32_t* heavy_out, QueueCtl* qc) {
  constexpr uint32_t K = shade_kernel_mode(M) & (SM_LENS | SM_SHUTTER | SM_PASSES | SM_BRANCH | SM_SMOOTH | SM_TEX | SM_NMAP);  // (the camera arm, the passes, the mirror's shared-out roulette, its shading normal - mapped or not - and its colour are all of a mode the lean kernel carries)
  auto go = [&](auto kernel, auto... a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((s->ps.npix + JADE_LEAN_BLOCK - 1) / JADE_LEAN_BLOCK)), dim3(JADE_LEAN_BLOCK), 0, s->stream, s->dev, s->ps, s->rc,
                       s->b_tiles.as<int32_t>(), target_spp, heavy_out, s->b_queue.as<uint32_t>(), qc, s->b_ctr.as<DevCounters>(), a...);
  };
  if constexpr (K == 0) go(k_shade_lean);
  else go(k_shade_lean_mode<K>, mode_args<K>(s));
}
// The lookup: a row per mode of JADE_SHADE_MODES_BUILT (jade_runtime.h) - the list jade_render_begin accepts from - and no other.
static const ShadeLaunch* shade_launcher(uint32_t mode) {
  switch (mode) {
#define JADE_X(m) case (m): { static const ShadeLaunch l{launch_full<(m)>, launch_lean<(m)>}; return &l; }
    JADE_SHADE_MODES_BUILT(JADE_X)
#undef JADE_X
  }
  return nullptr;
}

// The per-call state of run_passes.  Its pieces below each do one thing to it; every one queues its work on s->stream in the order written.
struct PassRun {
  jade_scene* s;
  uint32_t target_spp;
  QueueCtl* qc;                       // s->b_ctl: entry 0 for passes the host follows, the ring for a batch
  const ShadeLaunch* shade;           // the shade kernels of the render's mode (shade_launcher)
  bool batching, tail_ok;
  uint32_t tail_max;                  // active records at or below which k_tail finishes the list
  uint32_t carry_below = 0;           // ... and below which the step leaves them to the next one (0: never)
  uint32_t n_active = 0;
  const uint32_t* arm_dev = nullptr;  // k_arm's count, on the device, when the host has not waited for it
  uint32_t host_ctl[3] = {0, 0, 0};   // {count, active, next} of the last pass the host followed
  int cur = 0, pass_no = 0;
  bool have_list = true;              // b_active[cur] lists the active records
  bool trace_pending = false;         // the k_trace launch timed by (TA, TB) is not accounted for yet
  bool closed = false;                // EV1 is recorded and waited for: the last wait was also the wait for the end of the call
  bool done = false;                  // the call ends with records still active (carried over), or with nothing emitted
  double trace_ms = 0;
  uint64_t launches = 0;
  float shade_ms = 0, lean_ms = 0;    // JADE_LOG_PASSES
  enum { EV0, EV1, TA, TB, SA, SB, SM };  // s->ev
  hipEvent_t ev(int i) const { return s->ev[i].e; }
  bool carry_now(uint32_t act) const { return act < carry_below; }
};

// The carry-over point: a step may leave its paths to the next one once fewer than this many records are active - fewer than
// JADE_CARRY_RECORDS and than 1/1024 of the n_armed records the call started with, or fewer than carry_frac of them.  The host's
// decision (PassRun::carry_now) and the device's (k_shade's stop_below, inside a batch) are both "active < this".
static uint32_t carry_threshold(const jade_scene* s, bool may_carry, uint32_t n_armed) {
  if (!may_carry) return 0;
  const double frac = s->tun.carry_frac;
  const uint64_t a = std::min<uint64_t>(JADE_CARRY_RECORDS, ((uint64_t)n_armed + 1023) / 1024);  // act < CARRY_RECORDS && act * 1024 < n_armed
  const uint64_t b = frac > 0 ? (uint64_t)std::min(std::ceil(frac * (double)n_armed), 4294967295.0) : 0;  // act < frac * n_armed
  return (uint32_t)std::max(a, b);
}

// Rays claimed per queue atomic (trace_chunk_for, jade_runtime.h).  n_rays = 0 - a pass of a batch (run_batch), whose queue length only the
// device knows: 0, "size them yourself" - unless JADE_TRACE_CHUNK_RAYS names the size: then the device takes the host's value here too.
static uint32_t trace_chunk(const jade_scene* s, uint32_t n_rays) {
  const uint32_t hook = s->tun.trace_chunk_rays;
  if (n_rays == 0) return trace_chunk_hook_ok(hook) ? hook : 0u;
  return trace_chunk_for(n_rays, (uint64_t)s->trace_blocks * (JADE_TRACE_BLOCK / 64), hook);
}

void launch_trace(jade_scene* s, const PathState& P, const uint32_t* queue, QueueCtl* qc, uint32_t* spill, DevCounters* ctr, uint32_t n_rays) {
  const bool wide = trace_wide(s->dev, P);
  // k_trace tells a shadow ray from an environment ray by its slot number against n_emit (anyhit_key): it is handed the shadow slots of
  // the render's LAYOUT, which under JADE_LIGHTS_ONE is not the length of the scene's list (the single-slot callers - the guide pass,
  // jade_trace_rays - ask about slot 0 alone, which reads the same against either count)
  DevScene S = s->dev;
  if (one_light_on(s)) S.n_emit = std::min(s->n_emit, 1);
  hipLaunchKernelGGL(wide ? k_trace_wide : k_trace, dim3((unsigned)(wide ? s->trace_blocks_wide : s->trace_blocks)), dim3(JADE_TRACE_BLOCK), 0, s->stream,
                     S, P, queue, qc, spill, ctr, trace_chunk(s, n_rays));
}

// A k_trace launch of a render took the n rays of queue positions 0 .. n-1 (an ordered queue: the same positions in another order): those
// below the record boundary came as records, the rest through the index queue.  Host arithmetic on a count the host has read anyway.
static void count_queue(jade_scene* s, uint32_t n) {
  const uint32_t below = std::min(n, s->ps.rayq_cap);
  s->rays_recorded += below;
  s->rays_indexed += n - below;
}

// k_arm: clears the first `clear_bytes` of *ctl, then lists the records with work in b_active[0] and counts them in ctl->active
static int launch_arm(jade_scene* s, uint32_t target_spp, QueueCtl* ctl, size_t clear_bytes) {
  HIP_TRY(hipMemsetAsync(ctl, 0, clear_bytes, s->stream));
  const size_t per_block = (size_t)JADE_ARM_BLOCK * JADE_ARM_PER_THREAD;
  hipLaunchKernelGGL(k_arm, dim3((unsigned)(((size_t)s->ps.npix + per_block - 1) / per_block)), dim3(JADE_ARM_BLOCK), 0, s->stream, s->ps, target_spp,
                     s->b_active[0].as<uint32_t>(), ctl);
  return JADE_OK;
}

// the mode's shade kernel over `list`: n entries, or - n_dev not null - as many as the device counted there; the records it leaves
// active go to `next` (nullable)
static void launch_shade(const PassRun& r, unsigned blocks, const uint32_t* list, uint32_t n, const uint32_t* n_dev, uint32_t* next, QueueCtl* ctl,
                         const QueueCtl* prev, uint32_t stop_below) {
  r.shade->full(r.s, r.target_spp, blocks, list, n, n_dev, next, ctl, prev, stop_below);
}

// a finished k_trace launch, timed by the events (a, b)
static int account_trace(PassRun& r, hipEvent_t a, hipEvent_t b) {
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, a, b));
  r.trace_ms += t;
  r.launches += 1;
  return JADE_OK;
}
// ... the one of the last host-followed pass, if it is still open (the stream has been waited for since)
static int account_pending_trace(PassRun& r) {
  if (!r.trace_pending) return JADE_OK;
  r.trace_pending = false;
  return account_trace(r, r.ev(PassRun::TA), r.ev(PassRun::TB));
}

// A render under a thin lens (jade_scene_set_lens; taken by jade_render_begin) runs the lens kernels: k_shade_lean_mode<SM_LENS> +
// k_shade_mode<SM_LENS | ...> + k_trace, the schedule JADE_FUSED=0 JADE_TAIL=0 gives the pinhole.  k_light, k_light_packet, k_tail and
// k_shade_binned have no lens form, so JADE_FUSED, JADE_LIGHT_PACKET, JADE_TAIL and JADE_SHADE_BINNED have no effect there.
// A render under a shutter (jade_scene_set_shutter) runs the same schedule with the shutter kernels, which handle "with a lens" and "without"
// themselves.  What the schedule asks is own_origin (jade_runtime.h).
// A render that keeps passes (jade_scene_set_passes) runs that schedule as well: k_light and k_light_packet book nothing.
// A render with the branch draws shared out (jade_scene_set_branch_sampling) runs it too: k_light and k_light_packet shade the camera vertex with the
// stream's draws.
// A smooth render (jade_scene_set_vertex_normals) runs it as well: k_light and k_light_packet shade the camera vertex's mirror with the flat normal.
static bool fused_first_pass(const jade_scene* s) { return s->tun.fused && !own_origin(s) && !passes_on(s) && !branch_on(s) && !smooth_on(s); }

// The records with work in this call: all of them when the step gives every record a sample (k_light then walks the
// records itself); otherwise - a flush, a step of fewer samples than records per pixel - k_arm lists and counts them.
static int arm_step(PassRun& r, int64_t from_spp) {
  jade_scene* s = r.s;
  if (fused_first_pass(s) && s->ps.stride == 0 && (int64_t)r.target_spp - from_spp >= (int64_t)s->ps.rpp) {
    r.n_active = (uint32_t)s->ps.npix;
  } else if ((int64_t)r.target_spp == from_spp && s->carried_active > 0 && s->tun.batching && !s->sort_rays && !s->tun.log_passes && s->ps.stride == 0) {
    // A flush: no sample is started, so the records with work are exactly the ones the last step carried over, and the host knows
    // how many those were - k_arm lists them, the first pass of the batch reads the count on the device, nobody waits.
    QueueCtl* qa = r.qc + JADE_CTL_RING;
    if (int rc = launch_arm(s, r.target_spp, qa, 12)) return rc;
    r.n_active = s->carried_active;  // (an upper bound is all the grids need)
    r.arm_dev = &qa->active;
  } else {
    if (int rc = launch_arm(s, r.target_spp, r.qc, 12)) return rc;
    HIP_TRY(hipMemcpyAsync(r.host_ctl, r.qc, 12, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->host_syncs += 1;
    r.n_active = r.host_ctl[1];
  }
  s->carried_active = 0;
  return JADE_OK;
}

// k_tail: once the active list is short - and is not about to be carried over - ONE launch finishes its records (every wave
// shades and traces its own 64 until they are out of samples).  The records' last rays have been traced: k_tail starts by shading.
static int finish_by_tail(PassRun& r) {
  jade_scene* s = r.s;
  TailArgs ta;
  ta.R = s->rc;
  ta.tile_ids = s->b_tiles.as<int32_t>();
  ta.target_spp = r.target_spp;
  ta.list = s->b_active[r.cur].as<uint32_t>();
  ta.n_list = r.n_active;
  ta.queue = s->b_queue.as<uint32_t>();
  HIP_TRY(ensure_events(s->ev_tail));
  HIP_TRY(hipEventRecord(s->ev_tail[0], s->stream));
  hipLaunchKernelGGL(k_tail, dim3((r.n_active + JADE_TRACE_BLOCK - 1) / JADE_TRACE_BLOCK), dim3(JADE_TRACE_BLOCK), 0, s->stream, s->dev, s->ps, ta,
                     s->b_spill.as<uint32_t>(), s->b_ctr.as<DevCounters>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev_tail[1], s->stream));
  HIP_TRY(hipEventRecord(r.ev(PassRun::EV1), s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->host_syncs += 1;
  float tt = 0;
  HIP_TRY(hipEventElapsedTime(&tt, s->ev_tail[0], s->ev_tail[1]));
  s->tail_ms += tt;
  s->tail_launches += 1;
  s->tail_records += r.n_active;
  if (s->tun.log_passes) fprintf(stderr, "[jade] tail: %u records finished by k_tail in %.3f ms\n", r.n_active, tt);
  r.n_active = 0;
  r.closed = true;
  return JADE_OK;
}

// A BATCH of list-mode passes without the host in between: pass j's k_shade takes its length from the record
// count pass j-1 left on the device (QueueCtl ring), k_trace sizes its chunks itself; a pass that finds nothing
// to do is three empty launches.  The host looks once per batch: where the paths ended, whether to carry.
static int run_batch(PassRun& r) {
  jade_scene* s = r.s;
  QueueCtl* qc = r.qc;
  const int B = JADE_CTL_RING;
  const unsigned nbb = (r.n_active + JADE_SHADE_BLOCK - 1) / JADE_SHADE_BLOCK;  // the active count only shrinks: an upper bound for all
  // the device stops at the carry-over point - passes of the batch behind it do nothing (k_shade) - and at the point below which
  // k_tail finishes the list: the host then launches it (run_passes)
  uint32_t stop_below = r.carry_below;
  if (r.tail_ok) stop_below = std::max(stop_below, r.tail_max + 1u);
  HIP_TRY(ensure_events(s->ev_batch));
  HIP_TRY(hipMemsetAsync(qc, 0, sizeof(QueueCtl) * B, s->stream));
  const int cur0 = r.cur;
  for (int j = 0; j < B; ++j) {
    launch_shade(r, nbb, s->b_active[r.cur].as<uint32_t>(), r.n_active, j ? &qc[j - 1].active : r.arm_dev, s->b_active[r.cur ^ 1].as<uint32_t>(), qc + j,
                 j ? qc + (j - 1) : (const QueueCtl*)nullptr, stop_below);
    r.cur ^= 1;
    HIP_TRY(hipEventRecord(s->ev_batch[2 * j], s->stream));
    launch_trace(s, s->ps, s->b_queue.as<uint32_t>(), qc + j, s->b_spill.as<uint32_t>(), s->b_ctr.as<DevCounters>(), 0u);
    HIP_TRY(hipEventRecord(s->ev_batch[2 * j + 1], s->stream));
  }
  HIP_TRY(hipGetLastError());
  QueueCtl host_ring[JADE_CTL_RING];
  HIP_TRY(hipMemcpyAsync(host_ring, qc, sizeof(QueueCtl) * B, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipEventRecord(r.ev(PassRun::EV1), s->stream));  // the end of the call, if this batch is its last (recorded again otherwise)
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->host_syncs += 1;
  if (int rc = account_pending_trace(r)) return rc;  // the k_trace launch of the pass before the batch
  bool ended = false, stopped = false;
  int real = 0;        // passes of the batch that ran (the rest found the paths ended, or the carry-over point reached)
  int pass_timed = 0;  // k_trace launches of the batch accounted for so far
  for (int j = 0; j < B; ++j) {
    if (host_ring[j].count == 0) {
      if (host_ring[j].active == 0) {  // this pass emitted nothing and left nothing active: every path has ended
        // (a pass that ran and finished the last paths, or - behind it - one that found nothing to do)
        if (j == 0 || host_ring[j - 1].count != 0) real = j + 1;
        r.n_active = 0;
        ended = true;
      } else {  // the device stopped here: fewer than stop_below records are active
        r.n_active = host_ring[j].active;
        stopped = true;
      }
      break;
    }
    if (int rc = account_trace(r, s->ev_batch[2 * j], s->ev_batch[2 * j + 1])) return rc;
    count_queue(s, host_ring[j].count);
    pass_timed = j + 1;
    r.n_active = host_ring[j].active;
    ++r.pass_no;
    real = j + 1;
  }
  // the launches behind the end of the step were made all the same (k_trace leaves at its first instruction): they count
  // as launches, with their few microseconds, so that launches and time are what a profiler sees
  for (int j = pass_timed; j < B; ++j)
    if (int rc = account_trace(r, s->ev_batch[2 * j], s->ev_batch[2 * j + 1])) return rc;
  r.cur = cur0 ^ (real & 1);  // the list the last pass that ran wrote
  r.arm_dev = nullptr;        // (the host has seen a count since)
  if (ended) {
    r.closed = true;
  } else if (r.carry_now(r.n_active) || (stopped && !(r.tail_ok && r.n_active <= r.tail_max))) {
    s->tail_pending = true;
    s->carried_active = r.n_active;
    r.closed = true;
    r.done = true;
  }
  return JADE_OK;  // (otherwise: another batch - or, the list being short now, k_tail)
}

// The step's first pass, fused: light samples run to completion inside k_light / k_light_packet, everything else is handed over
// (k_heavy_scan, k_heavy_pack) in b_active[1], counted in qc->heavy.
static int launch_first_pass(PassRun& r) {
  jade_scene* s = r.s;
  const int npix = s->ps.npix;
  // packets, unless the last step gave most of them up (a frame the statue fills: every packet fans out, and the per-lane
  // kernel is then the better first pass - same bits, so the choice is free to make per step)
  const bool packet = s->tun.light_packet && s->packet_blocks > 0 && s->packets_given_up < JADE_PACKET_GIVE_UP_LIMIT;
  const unsigned lb = (unsigned)std::min<size_t>((size_t)(packet ? s->packet_blocks : s->light_blocks), ((size_t)npix + JADE_TRACE_BLOCK - 1) / JADE_TRACE_BLOCK);
  const uint32_t n_waves = lb * (JADE_TRACE_BLOCK / 64);
  // a wave takes every n_waves-th chunk of 64 records: its region must hold all of them
  const uint32_t region_cap = (uint32_t)((((size_t)npix + 63) / 64 + n_waves - 1) / n_waves) * 64u;
  if ((size_t)region_cap * n_waves > s->b_active[0].bytes / 4 || (size_t)2 * n_waves * 4 > s->b_wavecnt.bytes)
    return jade_fail(JADE_ERR_DEVICE, "hand-over regions do not fit (internal sizing error)");
  if (packet)
    hipLaunchKernelGGL(k_light_packet, dim3(lb), dim3(JADE_TRACE_BLOCK), 0, s->stream, s->dev, s->ps, s->rc, s->b_tiles.as<int32_t>(), r.target_spp,
                       s->b_active[0].as<uint32_t>(), region_cap, s->b_wavecnt.as<uint32_t>(), s->b_ctr.as<DevCounters>(),
                       (uint32_t)s->tun.packet_budget);
  else
    hipLaunchKernelGGL(k_light, dim3(lb), dim3(JADE_TRACE_BLOCK), 0, s->stream, s->dev, s->ps, s->rc, s->b_tiles.as<int32_t>(), r.target_spp,
                       s->b_active[0].as<uint32_t>(), region_cap, s->b_wavecnt.as<uint32_t>(), s->b_spill.as<uint32_t>(),
                       s->b_ctr.as<DevCounters>());
  hipLaunchKernelGGL(k_heavy_scan, dim3(1), dim3(1024), 0, s->stream, s->b_wavecnt.as<uint32_t>(), n_waves, r.qc);
  hipLaunchKernelGGL(k_heavy_pack, dim3(n_waves), dim3(256), 0, s->stream, s->b_active[0].as<uint32_t>(), region_cap,
                     s->b_wavecnt.as<uint32_t>(), n_waves, s->b_active[1].as<uint32_t>());
  return JADE_OK;
}

// One pass the host follows, its shading half: in one of three forms, then the wait for its counts (r.host_ctl).
//   fused (a step's first pass)  k_light / k_light_packet, then the shade kernel over what they handed over
//   lean                         k_shade_lean over all records (record order, no list), then the shade kernel over what it handed over
//   list                         the shade kernel alone over the active list, which k_arm rebuilds first if a lean pass came before
static int shade_pass(PassRun& r, bool lean_mode) {
  jade_scene* s = r.s;
  QueueCtl* qc = r.qc;
  const bool log_passes = s->tun.log_passes;
  const bool first_fused = lean_mode && fused_first_pass(s) && r.pass_no == 0;
  if (!lean_mode && !r.have_list) {
    r.cur = 0;
    if (int rc = launch_arm(s, r.target_spp, qc, 16)) return rc;
    r.have_list = true;
  }
  HIP_TRY(hipMemsetAsync(qc, 0, 16, s->stream));  // count, active, next, heavy
  if (log_passes) HIP_TRY(hipEventRecord(r.ev(PassRun::SA), s->stream));
  const unsigned nb = (r.n_active + JADE_SHADE_BLOCK - 1) / JADE_SHADE_BLOCK;
  if (first_fused) {
    HIP_TRY(ensure_events(s->ev_light));
    HIP_TRY(hipEventRecord(s->ev_light[0], s->stream));
    if (int rc = launch_first_pass(r)) return rc;
    HIP_TRY(hipEventRecord(s->ev_light[1], s->stream));
    if (log_passes) HIP_TRY(hipEventRecord(r.ev(PassRun::SM), s->stream));
    // k_light has run every other record to the end of its samples, so the records this pass leaves active ARE the active
    // list (written over k_light's regions, which k_heavy_pack has emptied): no k_arm scan of all records after it
    launch_shade(r, nb, s->b_active[1].as<uint32_t>(), 0u, &qc->heavy, s->b_active[0].as<uint32_t>(), qc, nullptr, 0u);
    r.have_list = true;
    r.cur = 0;
  } else if (lean_mode) {
    // b_active[1] carries the hand-over list; no active list is kept in this mode
    r.shade->lean(s, r.target_spp, s->b_active[1].as<uint32_t>(), qc);
    if (log_passes) HIP_TRY(hipEventRecord(r.ev(PassRun::SM), s->stream));
    // only a record that was active can be handed over: n_active bounds the grid, the count stays on the device
    launch_shade(r, nb, s->b_active[1].as<uint32_t>(), 0u, &qc->heavy, nullptr, qc, nullptr, 0u);
    r.have_list = false;
  } else {
    if (log_passes) HIP_TRY(hipEventRecord(r.ev(PassRun::SM), s->stream));
    launch_shade(r, nb, s->b_active[r.cur].as<uint32_t>(), r.n_active, nullptr, s->b_active[r.cur ^ 1].as<uint32_t>(), qc, nullptr, 0u);
    r.cur ^= 1;
  }
  HIP_TRY(hipGetLastError());
  if (log_passes) HIP_TRY(hipEventRecord(r.ev(PassRun::SB), s->stream));
  HIP_TRY(hipMemcpyAsync(r.host_ctl, qc, 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->host_syncs += 1;
  if (first_fused) {  // (the stream was just synchronised)
    float lt = 0;
    HIP_TRY(hipEventElapsedTime(&lt, s->ev_light[0], s->ev_light[1]));
    s->light_ms += lt;
  }
  if (log_passes) {
    HIP_TRY(hipEventElapsedTime(&r.shade_ms, r.ev(PassRun::SA), r.ev(PassRun::SB)));
    HIP_TRY(hipEventElapsedTime(&r.lean_ms, r.ev(PassRun::SA), r.ev(PassRun::SM)));
  }
  return account_pending_trace(r);
}

// Orders the queue of n rays by (kind, source triangle, octant) when the scene asks for it and the queue is long enough:
// *trace_queue then is the list of positions in the order k_trace is to take them (PathState.idxq)
static int order_queue(jade_scene* s, uint32_t n, const uint32_t** trace_queue) {
  if (!(s->sort_rays && n >= s->tun.sort_min && n <= s->sort_cap)) return JADE_OK;
  // (the keys are in b_sortkey already: the shading kernel wrote each beside its queue entry - PathState.keyq, round 4; until then
  // k_ray_keys made them here, from three scattered sectors per ray, 2 % of a C5 step.  JADE_SORT_KEYS_KERNEL=1 brings that back.)
  if (s->tun.sort_keys_kernel)
    hipLaunchKernelGGL(k_ray_keys, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ps, s->b_queue.as<uint32_t>(), n, s->b_sortkey.as<uint32_t>(),
                       s->b_sortpos.as<uint32_t>(), s->ps.nslots - 2, s->ps.key_tri_bits);  // (the layout's shadow slots: JADE_LIGHTS_ONE has one)
  // The temporary storage was sized once, for (sort_cap entries, bits 0..32).  rocPRIM's need shrinks with the length and with
  // the bit range (fewer digit places, fewer look-back states; a short queue takes its merge-sort path: two buffers of n), and a
  // buffer that is too small is an error return, not a fault (rocprim/detail/temp_storage.hpp: partition) - asked again here,
  // on the host, for THIS length, so that the claim is checked and not assumed ("the round-3 fault").
  size_t need = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, 32u, s->stream));
  if (need > s->sort_tmp_bytes) return jade_fail(JADE_ERR_DEVICE, "ray-queue sort: temporary storage smaller than rocPRIM asks for this length (internal sizing error)");
  size_t tmp = s->sort_tmp_bytes;
  HIP_TRY(rocprim::radix_sort_pairs(s->b_sorttmp.p, tmp, s->b_sortkey.as<uint32_t>(), s->b_sortkey2.as<uint32_t>(), s->b_sortpos.as<uint32_t>(),
                                    s->b_sortq.as<uint32_t>(), (size_t)n, 0u, 32u, s->stream));
  *trace_queue = s->b_sortq.as<uint32_t>();
  return JADE_OK;
}

// JADE_LOG_PASSES: one line for the pass whose k_trace launch was just made (waits for it)
static int log_pass(PassRun& r) {
  jade_scene* s = r.s;
  HIP_TRY(hipEventSynchronize(r.ev(PassRun::TB)));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, r.ev(PassRun::TA), r.ev(PassRun::TB)));
  DevCounters cc{};  // development log only: node records and triangle tests of this launch (counters accumulate over the step)
  HIP_TRY(sum_counters(s, &cc));
  static thread_local unsigned long long v_prev = 0, t_prev = 0;
  if (r.pass_no == 0 && (cc.nodes_visited < v_prev || cc.tris_tested < t_prev)) v_prev = t_prev = 0;
  if (cc.nodes_visited < v_prev) v_prev = t_prev = 0;
  fprintf(stderr, "[jade] pass %4d active %9u rays %9u shade %7.3f ms (lean %6.3f) trace %8.3f ms (%7.1f Mray/s) V/ray %6.1f T/ray %5.1f\n", r.pass_no,
          r.n_active, r.host_ctl[0], r.shade_ms, r.lean_ms, t, r.host_ctl[0] / (t * 1e3), (double)(cc.nodes_visited - v_prev) / r.host_ctl[0],
          (double)(cc.tris_tested - t_prev) / r.host_ctl[0]);
  v_prev = cc.nodes_visited;
  t_prev = cc.tris_tested;
  return JADE_OK;
}

// One pass the host follows: shade, wait for the counts, then - unless nothing was emitted - order the queue and launch the trace,
// which stays open (trace_pending) until the next wait.
static int run_host_pass(PassRun& r, bool lean_mode) {
  jade_scene* s = r.s;
  if (int rc = shade_pass(r, lean_mode)) return rc;
  r.n_active = r.host_ctl[1];
  if (r.host_ctl[0] == 0) {
    r.done = true;
    return JADE_OK;
  }
  const uint32_t* trace_queue = s->b_queue.as<uint32_t>();
  HIP_TRY(hipEventRecord(r.ev(PassRun::TA), s->stream));  // (the ordering counts as trace time)
  if (int rc = order_queue(s, r.host_ctl[0], &trace_queue)) return rc;
  PathState tps = s->ps;
  tps.idxq = trace_queue != s->b_queue.as<uint32_t>() ? s->b_queue.as<uint32_t>() : nullptr;
  launch_trace(s, tps, trace_queue, r.qc, s->b_spill.as<uint32_t>(), s->b_ctr.as<DevCounters>(), r.host_ctl[0]);
  HIP_TRY(hipGetLastError());
  count_queue(s, r.host_ctl[0]);
  HIP_TRY(hipEventRecord(r.ev(PassRun::TB), s->stream));
  r.trace_pending = true;
  if (r.carry_now(r.n_active)) {
    // The few long paths left would take dozens of nearly empty passes: leave them suspended (their
    // rays are traced, their hits wait to be folded in) for the next step's first pass, or for flush.
    s->tail_pending = true;
    s->carried_active = r.n_active;
    r.done = true;
  }
  if (s->tun.log_passes)
    if (int rc = log_pass(r)) return rc;
  ++r.pass_no;
  return JADE_OK;
}

// shade/trace passes until a shade pass emits no ray (or the step may carry the rest over).  What runs next, by the records active:
//   at least a quarter of all records (JADE_SHADE_SPLIT=0: never)     a pass the host follows, fused (a step's first) or lean
//   a short list that is not about to be carried over                 k_tail finishes it: the end of the call
//   a list, after the first pass (JADE_BATCH=0, ordered queues,       a batch of JADE_CTL_RING passes, one wait; it ends the call,
//   JADE_LOG_PASSES: never)                                           carries over, or leaves a shorter list
//   otherwise                                                         a pass the host follows, over the list
static int run_passes(jade_scene* s, int64_t from_spp, uint32_t target_spp, bool may_carry, double* ms_out, double* trace_ms_out, uint64_t* launches_out) {
  HIP_TRY(ensure_events(s->ev));
  PassRun r{s, target_spp, s->b_ctl.as<QueueCtl>()};
  HIP_TRY(hipEventRecord(r.ev(PassRun::EV0), s->stream));
  s->tail_pending = false;  // whatever an earlier step left is part of this call's work
  if (int rc = arm_step(r, from_spp)) return rc;
  r.carry_below = carry_threshold(s, may_carry, r.n_active);
  r.shade = shade_launcher(s->mode);
  if (!r.shade) return jade_fail(JADE_ERR_DEVICE, "no shade kernel for the render's mode (internal error: jade_render_begin accepts built modes only)");
  r.batching = s->tun.batching && !s->sort_rays;  // (rocPRIM wants the queue's length on the host)
  r.tail_ok = s->tun.tail && s->tun.tail_max > 0 && parity_shading(s) && !passes_on(s);  // (k_tail shades with the parity code only, and books no pass)
  r.tail_max = std::min<uint32_t>(s->tun.tail_max, (uint32_t)(s->b_queue.bytes / 4 / (size_t)std::max(s->ps.nslots, 1)));
  // (k_tail is launched with one thread per record and is handed the stack spill area, which is sized for k_trace's grid: setup_state)
  r.tail_max = std::min<uint32_t>(r.tail_max, (uint32_t)s->trace_blocks * JADE_TRACE_BLOCK);
  while (r.n_active && !r.done) {
    const bool lean_mode = s->tun.shade_split && (uint64_t)r.n_active * 4 >= (uint64_t)s->ps.npix;
    const bool list_mode = !lean_mode && r.have_list;
    int rc;
    if (r.tail_ok && list_mode && r.pass_no > 0 && !r.arm_dev && r.n_active <= r.tail_max && !r.carry_now(r.n_active))
      rc = finish_by_tail(r);
    else if (list_mode && r.batching && !s->tun.log_passes && (r.pass_no > 0 || r.arm_dev))
      rc = run_batch(r);
    else
      rc = run_host_pass(r, lean_mode);
    if (rc) return rc;
  }
  if (r.trace_pending) {  // the launch timed by (TA, TB) when the loop stopped right after it
    HIP_TRY(hipEventSynchronize(r.ev(PassRun::TB)));
    if (int rc = account_pending_trace(r)) return rc;
  }
  if (!r.closed) {
    HIP_TRY(hipEventRecord(r.ev(PassRun::EV1), s->stream));
    HIP_TRY(hipEventSynchronize(r.ev(PassRun::EV1)));
    s->host_syncs += 1;
  }
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, r.ev(PassRun::EV0), r.ev(PassRun::EV1)));
  *ms_out = ms;
  *trace_ms_out = r.trace_ms;
  *launches_out = r.launches;
  return JADE_OK;
}

// runs the passes for every sample up to spp_done; may_carry: the last paths may be left for later
static int advance(jade_scene* s, int64_t from0, bool may_carry, jade_stats* st) {
  HIP_TRY(hipMemsetAsync(s->b_ctr.p, 0, sizeof(DevCounters) * JADE_CTR_SHARDS, s->stream));
  double ms = 0, trace_ms = 0;
  uint64_t launches = 0;
  // pixel rotation only: one block of JADE_SAMPLE_LANES samples at a time (see PathState): records may not
  // run ahead into the next block while another record still owns a (pixel, lane) sum of this one
  for (int64_t from = from0;;) {
    int64_t to = (from / JADE_SAMPLE_LANES + 1) * JADE_SAMPLE_LANES;
    if (to > s->spp_done || s->ps.stride == 0) to = s->spp_done;  // no rotation: no block barrier needed
    double m1 = 0, t1 = 0;
    uint64_t l1 = 0;
    int rc = run_passes(s, from, (uint32_t)to, may_carry && s->ps.stride == 0, &m1, &t1, &l1);
    if (rc) return rc;
    ms += m1; trace_ms += t1; launches += l1;
    from = to;
    if (from >= s->spp_done) break;
  }
  DevCounters c{};
  HIP_TRY(sum_counters(s, &c));  // (32 KB: also read when the caller wants no statistics - the next step's choice of first pass depends on it)
  if (c.pad[0]) s->packets_given_up = (double)c.pad[1] / (double)c.pad[0];
  if (s->tun.log_passes && c.pad[0])
    fprintf(stderr, "[jade] first pass: %llu packets, %llu given up and handed to the wavefront passes (%.2f %%)\n", (unsigned long long)c.pad[0],
            (unsigned long long)c.pad[1], 100.0 * (double)c.pad[1] / (double)c.pad[0]);
  if (st) {
    st->rays_primary += c.rays_primary;
    st->rays_secondary += c.rays_shadow + c.rays_env + c.rays_indirect + c.rays_mirror + c.rays_refract;
    st->rays_shadow += c.rays_shadow;
    st->rays_env += c.rays_env;
    st->rays_indirect += c.rays_indirect;
    st->rays_mirror += c.rays_mirror;
    st->rays_refract += c.rays_refract;
    st->rays_inline += c.rays_inline;
    st->nodes_inline += c.nodes_inline;
    st->tris_inline += c.tris_inline;
    st->rays_cached += c.rays_cached;
    st->rays_tail += c.rays_tail;
    st->nodes_tail += c.nodes_tail;
    st->tris_tail += c.tris_tail;
    st->tail_ms += s->tail_ms;
    st->tail_launches += s->tail_launches;
    st->light_ms += s->light_ms;
    st->nodes_visited += c.nodes_visited;
    st->tris_tested += c.tris_tested;
    st->shaded_hits += c.shaded_hits;
    st->samples += c.samples;
    st->kernel_ms += ms;
    st->trace_ms += trace_ms;
    st->trace_launches += launches;
    st->host_syncs += s->host_syncs;
  }
  s->host_syncs = 0;
  s->light_ms = 0;
  s->tail_ms = 0;
  s->tail_launches = 0;
  s->tail_records = 0;
  return JADE_OK;
}

// The steps add more samples than jade_render_begin was told of: more lanes of partial sums (jade_rt.h,
// JADE_Q_SUM_LANES).
static int grow_sums(jade_scene* s, int64_t spp_total) {
  PathState& P = s->ps;
  int lanes = P.sum_lanes;
  while (lanes < JADE_SAMPLE_LANES && lanes < spp_total) lanes <<= 1;
  if (lanes == P.sum_lanes) return JADE_OK;
  DevBuf nb;
  // (lane l of pixel p sits at (l * npx + p) * 3: more lanes are more of the same behind the old ones; the new lanes are +0)
  const size_t bytes_old = (size_t)P.sum_lanes * P.npx * 12, bytes_new = (size_t)lanes * P.npx * 12;
  HIP_TRY(nb.alloc(bytes_new));
  HIP_TRY(hipMemsetAsync(nb.p, 0, bytes_new, s->stream));
  HIP_TRY(hipMemcpyAsync(nb.p, s->b_sum.p, bytes_old, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::swap(s->b_sum.p, nb.p);
  std::swap(s->b_sum.bytes, nb.bytes);
  P.sum = s->b_sum.as<float>();
  P.sum_lanes = lanes;
  return JADE_OK;
}

int jade_render_query(jade_scene* s, int what, int64_t* value) {
  if (!s || !value || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  switch (what) {
    case JADE_Q_RECORDS_PER_PIXEL: *value = s->ps.npix ? s->ps.rpp : 0; return JADE_OK;
    case JADE_Q_STATE_BYTES:
      *value = s->ps.npix ? (int64_t)(s->b_state.bytes + s->b_sum.bytes + s->b_queue.bytes + s->b_rayq.bytes + s->b_active[0].bytes + s->b_active[1].bytes +
                                      s->b_wavecnt.bytes + s->b_spill.bytes + s->b_pass_cur.bytes + s->b_pass_tot.bytes + s->b_pass_mask.bytes + s->b_sortkey.bytes + s->b_sortkey2.bytes + s->b_sortpos.bytes + s->b_sortq.bytes + s->b_sorttmp.bytes)
                          : 0;
      return JADE_OK;
    case JADE_Q_SUM_LANES: *value = s->ps.npix ? s->ps.sum_lanes : 0; return JADE_OK;
    default: return jade_fail(JADE_ERR_INVALID, "unknown query");
  }
}

// The work counters a denoiser entry point's flush counted (jade_scene.dn_carried) go to the caller's statistics of the next step or flush.
static void dn_hand_over(jade_scene* s, jade_stats* st) {
  jade_stats& c = s->dn_carried;
  if (st) {
    st->rays_primary += c.rays_primary; st->rays_secondary += c.rays_secondary;
    st->nodes_visited += c.nodes_visited; st->tris_tested += c.tris_tested;
    st->shaded_hits += c.shaded_hits; st->samples += c.samples;
    st->rays_shadow += c.rays_shadow; st->rays_env += c.rays_env; st->rays_indirect += c.rays_indirect;
    st->rays_mirror += c.rays_mirror; st->rays_refract += c.rays_refract;
    st->rays_inline += c.rays_inline; st->nodes_inline += c.nodes_inline; st->tris_inline += c.tris_inline;
    st->rays_cached += c.rays_cached;
    st->rays_tail += c.rays_tail; st->nodes_tail += c.nodes_tail; st->tris_tail += c.tris_tail;
  }
  c = jade_stats{};
}

int jade_render_step(jade_scene* s, int32_t spp, jade_stats* st) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (spp < 0) return jade_fail(JADE_ERR_INVALID, "negative spp");
  if (s->adaptive_done) return jade_fail(JADE_ERR_INVALID, "the adaptive render has ended: jade_render_begin starts a new one");
  dn_hand_over(s, st);
  HIP_TRY(hipSetDevice(s->device));
  if (s->ps.npix == 0 || spp == 0) {
    s->spp_done += spp;
    return JADE_OK;
  }
  // (the sample count moves only once the partial sums have room for the new samples: after a failed grow_sums - out of memory -
  // a resolve must not divide by samples that were never rendered)
  if (s->spp_done + spp > s->ps.sum_lanes && s->ps.sum_lanes < JADE_SAMPLE_LANES)
    if (int rc = grow_sums(s, s->spp_done + spp)) return rc;
  s->spp_done += spp;
  return advance(s, s->spp_done - spp, s->tun.carry, st);
}

int jade_render_flush(jade_scene* s, jade_stats* st) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (st) dn_hand_over(s, st);  // (the flushes inside resolve and the denoiser pass no statistics: the counters wait for the next step)
  if (!s->tail_pending || s->ps.npix == 0) return JADE_OK;
  HIP_TRY(hipSetDevice(s->device));
  return advance(s, s->spp_done, false, st);
}

int resolve_to(jade_scene* s, int tonemap, float limit, float* dev_rgb, uint8_t* dev_bgr, hipStream_t stream) {
  const int npix = s->ps.npx;
  if (npix == 0) return JADE_OK;
  float inv = (float)(1.0 / (double)s->spp_done);  // vec3(1.0 / spp), PathTrace.cu:1457
  // after jade_render_adaptive: each tile's own (float)(1.0 / (double)n), made the same way (jade_render_adaptive)
  const float* tile_inv = s->tile_n.empty() ? nullptr : s->b_tile_inv.as<float>();
  hipLaunchKernelGGL(k_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, s->ps, s->rc, s->b_tiles.as<int32_t>(), tile_inv, inv, tonemap, limit,
                     dev_rgb, dev_bgr);
  HIP_TRY(hipGetLastError());
  return JADE_OK;
}

int jade_render_resolve(jade_scene* s, float* out_rgb, uint8_t* out_bgr8) {
  return jade_render_resolve_ex(s, JADE_TONEMAP_ACES, 0.0f, out_rgb, out_bgr8);
}

int jade_render_resolve_ex(jade_scene* s, int tonemap, float limit, float* out_rgb, uint8_t* out_bgr8) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (tonemap != JADE_TONEMAP_ACES && tonemap != JADE_TONEMAP_REINHARD) return jade_fail(JADE_ERR_INVALID, "unknown tone operator");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = jade_render_flush(s, nullptr)) return rc;
  const int npix = s->ps.npx;
  if (npix == 0) return JADE_OK;
  if (out_rgb) HIP_TRY(s->b_out_rgb.alloc((size_t)npix * 12));
  if (out_bgr8) HIP_TRY(s->b_out_bgr.alloc((size_t)npix * 3));
  int rc = resolve_to(s, tonemap, limit, out_rgb ? s->b_out_rgb.as<float>() : nullptr, out_bgr8 ? s->b_out_bgr.as<uint8_t>() : nullptr, s->stream);
  if (rc) return rc;
  std::vector<float> hrgb;
  std::vector<uint8_t> hbgr;
  if (out_rgb) {
    hrgb.resize((size_t)npix * 3);
    HIP_TRY(hipMemcpyAsync(hrgb.data(), s->b_out_rgb.p, hrgb.size() * 4, hipMemcpyDeviceToHost, s->stream));
  }
  if (out_bgr8) {
    hbgr.resize((size_t)npix * 3);
    HIP_TRY(hipMemcpyAsync(hbgr.data(), s->b_out_bgr.p, hbgr.size(), hipMemcpyDeviceToHost, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  // scatter the compact tiles into the caller's frame; other ranks' pixels untouched
  const int W = s->rp.width;
  for_each_owned_tile(s->tile_ids, W, s->rp.height, [&](size_t t, int x0, int y0, int ww, int hh) {
    for (int ly = 0; ly < hh; ++ly) {
      size_t src = (t * 256 + (size_t)ly * 16) * 3, dst = ((size_t)(y0 + ly) * W + x0) * 3;
      if (out_rgb) memcpy(out_rgb + dst, hrgb.data() + src, (size_t)ww * 12);
      if (out_bgr8) memcpy(out_bgr8 + dst, hbgr.data() + src, (size_t)ww * 3);
    }
  });
  return JADE_OK;
}

int jade_render_resolve_tiles_device(jade_scene* s, float* dev_tiles, void* stream) {
  if (!s || !s->have_rp || !dev_tiles) return jade_fail(JADE_ERR_INVALID, "bad arguments");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = jade_render_flush(s, nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (int rc = resolve_to(s, JADE_TONEMAP_ACES, 0.0f, dev_tiles, nullptr, (hipStream_t)stream)) return rc;
  // k_resolve reads the partial sums on the CALLER's stream: the scene's own stream must not start the next
  // step (which adds to them) before it has finished
  if (!s->ev_resolve.e) HIP_TRY(hipEventCreateWithFlags(&s->ev_resolve.e, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(s->ev_resolve, (hipStream_t)stream));
  HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_resolve, 0));
  return JADE_OK;
}

int jade_render(jade_scene* s, const jade_render_params* rp, float* out_rgb, uint8_t* out_bgr8, jade_stats* st) {
  if (!rp) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (rp->spp <= 0) return jade_fail(JADE_ERR_INVALID, "spp must be positive");
  int rc = jade_render_begin(s, rp);
  if (rc) return rc;
  rc = jade_render_step(s, rp->spp, st);
  if (rc == JADE_OK) rc = jade_render_flush(s, st);  // (resolve would flush too, but without the statistics)
  if (rc) return rc;
  return jade_render_resolve(s, out_rgb, out_bgr8);
}

// limits (nullable): per ray, the distance below which a recorded hit ends the walk (JADE_WALK_EARLY_EXIT as k_shade asks
// for it, jade_device.h); null = the reference's walk
static int trace_rays_impl(jade_scene* s, int32_t n, const float* origins, const float* dirs, const int32_t* skip, const float* limits,
                           int32_t* hit_index, float* hit_dist, float* hit_point, jade_stats* st, bool cached = false) {
  if (!s || n < 0 || !origins || !dirs || !skip || !hit_index) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (n == 0) return JADE_OK;
  HIP_TRY(hipSetDevice(s->device));
  // a throw-away PathState with one slot per "pixel"
  const size_t N = (size_t)n;
  std::vector<float4> so(N), sl(N), hp(N, make_float4(0.0f, 0.0f, 0.0f, 0.0f));  // (the hit point of a miss is reported as zeros)
  for (size_t i = 0; i < N; ++i) {
    const int32_t sk = skip[i] < 0 ? -1 : skip[i];  // any negative value means "no source triangle" (the device keeps -2 for camera rays)
    float skf, qf;
    const int32_t queued = -1;
    memcpy(&skf, &sk, 4);
    memcpy(&qf, &queued, 4);
    so[i] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], skf);
    sl[i] = make_float4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], limits ? limits[i] : qf);
  }
  std::vector<uint32_t> q(N);
  for (size_t i = 0; i < N; ++i) q[i] = (uint32_t)i;
  DevBuf b_orgs, b_slot, b_hitp, b_q, b_spill;
  HIP_TRY(upload(b_orgs, so.data(), so.size(), s->stream));
  HIP_TRY(upload(b_slot, sl.data(), sl.size(), s->stream));
  HIP_TRY(upload(b_hitp, hp.data(), hp.size(), s->stream));
  HIP_TRY(upload(b_q, q.data(), N, s->stream));
  HIP_TRY(b_spill.alloc((size_t)(JADE_BVH_STACK_CAPACITY - JADE_LDS_STACK) * s->trace_blocks * JADE_TRACE_BLOCK * 4));
  PathState P{};
  P.npix = n;
  P.nslots = 1;
  P.orgs = b_orgs.as<float4>();
  P.slot = b_slot.as<float4>();
  P.hitp = b_hitp.as<float4>();
  P.write_all_hits = 1u;  // (this entry point reports point and distance of EVERY ray, also of one that carries a yes/no limit)
  P.early_exit = limits ? (cached ? 2u : 1u) : 0u;
  // everything on the scene's own (non-blocking) stream: the null stream does not order against it
  QueueCtl qc{};
  qc.count = (uint32_t)n;
  HIP_TRY(hipMemcpyAsync(s->b_ctl.p, &qc, 12, hipMemcpyHostToDevice, s->stream));  // count, active, next
  HIP_TRY(hipMemsetAsync(s->b_ctr.p, 0, sizeof(DevCounters) * JADE_CTR_SHARDS, s->stream));
  DevEvent ev0, ev1;
  HIP_TRY(ev0.create());
  HIP_TRY(ev1.create());
  HIP_TRY(hipEventRecord(ev0.e, s->stream));
  launch_trace(s, P, b_q.as<uint32_t>(), s->b_ctl.as<QueueCtl>(), b_spill.as<uint32_t>(), s->b_ctr.as<DevCounters>(), (uint32_t)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev1.e, s->stream));
  HIP_TRY(hipEventSynchronize(ev1.e));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ev0.e, ev1.e));
  // HitResult.distance (PathTrace.cu:740) exactly as the kernel compared it (hitArray's `<`, :787); a miss keeps INF (:799)
  HIP_TRY(hipMemcpyAsync(sl.data(), b_slot.p, N * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(hp.data(), b_hitp.p, N * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (size_t i = 0; i < N; ++i) {
    memcpy(&hit_index[i], &sl[i].w, 4);
    if (hit_dist) hit_dist[i] = hp[i].w;
    if (hit_point) {
      const bool hit = hit_index[i] >= 0;
      hit_point[3 * i] = hit ? hp[i].x : 0.0f;
      hit_point[3 * i + 1] = hit ? hp[i].y : 0.0f;
      hit_point[3 * i + 2] = hit ? hp[i].z : 0.0f;
    }
  }
  if (st) {
    DevCounters c{};
    HIP_TRY(sum_counters(s, &c));
    st->rays_secondary += (uint64_t)n;
    st->nodes_visited += c.nodes_visited;
    st->tris_tested += c.tris_tested;
    st->rays_cached += c.rays_cached;
    st->kernel_ms += ms;
    st->trace_ms += ms;
    st->trace_launches += 1;
  }
  return JADE_OK;
}

int jade_trace_rays(jade_scene* s, int32_t n, const float* origins, const float* dirs, const int32_t* skip, int32_t* hit_index,
                    float* hit_dist, float* hit_point, jade_stats* st) {
  return trace_rays_impl(s, n, origins, dirs, skip, nullptr, hit_index, hit_dist, hit_point, st);
}

// ---- development / test entry points: NOT part of jade_rt.h and NOT in libjade_hip.so.  Only builds with -DJADE_DEBUG_EXPORTS=1
// have them: libjade_hip_debug.so (make hipvariants; tests/conftest.py `hip_debug`) and the JADE_TRACE_PROFILE build.
// (jade_runtime.h gives JADE_DEBUG_EXPORTS its default; the piece-by-piece arithmetic entry points are in jade_debug_units.hip.)
#if JADE_DEBUG_EXPORTS
extern "C" {
// Development / tests (not part of jade_rt.h): jade_trace_rays with a limit per ray - k_trace's early exit on its own, outside
// the integrator.  For a ray whose nearest hit is not nearer than its limit the answer is the reference's; otherwise it is SOME
// recorded hit nearer than the limit (which one depends on the schedule of the wave).
int jade_debug_trace_rays_limit(jade_scene* s, int32_t n, const float* origins, const float* dirs, const int32_t* skip, const float* limits,
                                int32_t* hit_index, float* hit_dist, float* hit_point, jade_stats* st) {
  if (!limits) return jade_fail(JADE_ERR_INVALID, "null argument");
  return trace_rays_impl(s, n, origins, dirs, skip, limits, hit_index, hit_dist, hit_point, st);
}
// ... and with the occluder cache (JADE_WALK_EARLY_EXIT_CACHED): a ray with a source triangle and a limit that is not a NaN is a
// yes/no query keyed by that triangle (query kind: "towards emitter 0", or by octant in a scene without emitters)
int jade_debug_trace_rays_cached(jade_scene* s, int32_t n, const float* origins, const float* dirs, const int32_t* skip, const float* limits,
                                 int32_t* hit_index, float* hit_dist, float* hit_point, jade_stats* st) {
  if (!limits) return jade_fail(JADE_ERR_INVALID, "null argument");
  return trace_rays_impl(s, n, origins, dirs, skip, limits, hit_index, hit_dist, hit_point, st, true);
}
// whether jade_scene_create found every child's box inside its parent's (1), what the wide walk and the occluder cache rest on; and
// whether the scene got wide records (bit 1) / an occluder cache (bit 2)
int jade_debug_scene_flags(jade_scene* s) {
  if (!s) return -1;
  return (s->boxes_nested ? 1 : 0) | (s->dev.nodes4 ? 2 : 0) | (s->dev.anyhit ? 4 : 0);
}
// the persistent grids size_grids chose, in blocks of JADE_TRACE_BLOCK threads: k_trace's, k_trace_wide's, k_light's, k_light_packet's (0: the
// tree is too deep for the packet form).  The stack spill area holds JADE_BVH_STACK_CAPACITY - JADE_LDS_STACK levels for out[0] blocks:
// no kernel that is handed the area may be launched with more (setup_state; tests/test_gpu_deep_trees.py).  Host code only.
int jade_debug_scene_grids(jade_scene* s, int32_t out[4]) {
  if (!s || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  out[0] = s->trace_blocks;
  out[1] = s->trace_blocks_wide;
  out[2] = s->light_blocks;
  out[3] = s->packet_blocks;
  return JADE_OK;
}
// the rays k_trace took, since jade_render_begin, from queue positions below the record boundary (out[0]: as ray records) and at or beyond it
// (out[1]: through the index queue) - summed over the launches whose queue counts the host reads (run_host_pass, run_batch).  k_tail's own rays
// are not counted: it runs with no records.  Host code only.
int jade_debug_ray_record_use(jade_scene* s, int64_t out[2]) {
  if (!s || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  out[0] = s->rays_recorded;
  out[1] = s->rays_indexed;
  return JADE_OK;
}

// Development / tests (not part of jade_rt.h): shadow_limit (jade_shade.h) for n rays against triangle tri (BVH order): what
// k_shade writes beside a shadow ray's direction.
__global__ void k_debug_shadow_limit(DevScene S, int n, const float* o, const float* d, const int32_t* tri, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = shadow_limit(&S.tris[tri[i]], jv(o[3 * i], o[3 * i + 1], o[3 * i + 2]), jv(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
}
int jade_debug_shadow_limit(jade_scene* s, int32_t n, const float* origins, const float* dirs, const int32_t* tri, float* limit) {
  if (!s || n <= 0 || !origins || !dirs || !tri || !limit) return jade_fail(JADE_ERR_INVALID, "null argument");
  for (int i = 0; i < n; ++i)
    if (tri[i] < 0 || tri[i] >= s->dev.n_tris) return jade_fail(JADE_ERR_INVALID, "triangle index out of range");
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bo, bd, bt, bl;
  HIP_TRY(upload(bo, origins, 3 * N, s->stream));
  HIP_TRY(upload(bd, dirs, 3 * N, s->stream));
  HIP_TRY(upload(bt, tri, N, s->stream));
  HIP_TRY(bl.alloc(N * 4));
  hipLaunchKernelGGL(k_debug_shadow_limit, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->dev, n, bo.as<float>(), bd.as<float>(),
                     bt.as<int32_t>(), bl.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(limit, bl.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return JADE_OK;
}

// Development / tests (not part of jade_rt.h): hitBVH through the PACKET form of the walk (jade_trace.h; what k_light_packet
// runs), rays taken 64 at a time in the order given.  Like jade_trace_rays, plus per-ray counts of node records and triangle tests.
int jade_debug_packet_rays(jade_scene* s, int32_t n, const float* origins, const float* dirs, const int32_t* skip, int32_t* hit_index,
                           float* hit_dist, float* hit_point, uint32_t* v_per_ray, uint32_t* t_per_ray, double* kernel_ms /* nullable */) {
  if (!s || n <= 0 || !origins || !dirs || !skip || !hit_index || !hit_dist || !hit_point || !v_per_ray || !t_per_ray) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (s->bvh_depth > JADE_PACKET_MAX_DEPTH) return jade_fail(JADE_ERR_UNSUPPORTED, "tree too deep for the packet form");
  HIP_TRY(hipSetDevice(s->device));
  const size_t N = (size_t)n;
  DevBuf bo, bd, bs, bh, bt, bp, bv, bc;
  HIP_TRY(upload(bo, origins, 3 * N, s->stream));
  HIP_TRY(upload(bd, dirs, 3 * N, s->stream));
  HIP_TRY(upload(bs, skip, N, s->stream));
  HIP_TRY(bh.alloc(N * 4)); HIP_TRY(bt.alloc(N * 4)); HIP_TRY(bp.alloc(N * 12)); HIP_TRY(bv.alloc(N * 4)); HIP_TRY(bc.alloc(N * 4));
  DevEvent e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(hipEventRecord(e0.e, s->stream));
  hipLaunchKernelGGL(k_packet_rays, dim3((unsigned)((N + JADE_TRACE_BLOCK - 1) / JADE_TRACE_BLOCK)), dim3(JADE_TRACE_BLOCK), 0, s->stream, s->dev, n,
                     bo.as<float>(), bd.as<float>(), bs.as<int32_t>(), bh.as<int32_t>(), bt.as<float>(), bp.as<float>(), bv.as<uint32_t>(), bc.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1.e, s->stream));
  HIP_TRY(hipMemcpyAsync(hit_index, bh.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(hit_dist, bt.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(hit_point, bp.p, N * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(v_per_ray, bv.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(t_per_ray, bc.p, N * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
    *kernel_ms = ms;
  }
  return JADE_OK;
}

// Development only (not part of jade_rt.h): the laps of a -DJADE_TRACE_PROFILE=1 build, PL_N values; reset != 0 clears them.
// A product build reports JADE_ERR_UNSUPPORTED.
// the same for k_light_packet's laps and counts (jade_trace.h, PKL_*)
int jade_debug_packet_profile(unsigned long long* out, int n, int reset) {
#if JADE_TRACE_PROFILE
  if (!out || n < PKL_N) return jade_fail(JADE_ERR_INVALID, "need room for PKL_N values");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_packet_prof), sizeof(unsigned long long) * PKL_N));
  if (reset) {
    unsigned long long z[PKL_N] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_packet_prof), z, sizeof z));
  }
  return PKL_N;
#else
  (void)out; (void)n; (void)reset;
  return -jade_fail(JADE_ERR_UNSUPPORTED, "not a JADE_TRACE_PROFILE build");
#endif
}
int jade_debug_trace_profile(unsigned long long* out, int n, int reset) {
#if JADE_TRACE_PROFILE
  if (!out || n < PL_N) return jade_fail(JADE_ERR_INVALID, "need room for PL_N values");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace_prof), sizeof(unsigned long long) * PL_N));
  if (reset) {
    unsigned long long z[PL_N] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_prof), z, sizeof z));
  }
  return PL_N;
#else
  (void)out; (void)n; (void)reset;
  return -jade_fail(JADE_ERR_UNSUPPORTED, "not a JADE_TRACE_PROFILE build");
#endif
}
}  // extern "C"
#endif  // JADE_DEBUG_EXPORTS
