// jade_runtime.h — what more than one .hip file of libjade_hip.so needs on the host side: error reporting, the device buffer and
// event guards, the development switches, struct jade_scene, and the few internal functions that cross files.  Nothing here is
// exported: the library's boundary is include/jade_rt.h + jade_bvh.h (tests/test_abi.py).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "jade_bvh.h"
#include "jade_device.h"
#include "jade_normal_map.h"
#include "jade_texture.h"

#define JADE_HIDDEN __attribute__((visibility("hidden")))

// The jade_debug_* entry points (jade_hip.hip, jade_debug_units.hip): only in builds with -DJADE_DEBUG_EXPORTS=1
// (libjade_hip_debug.so) and in a -DJADE_TRACE_PROFILE=1 build; libjade_hip.so has none of them (tests/test_abi.py).
#ifndef JADE_DEBUG_EXPORTS
#if defined(JADE_TRACE_PROFILE) && JADE_TRACE_PROFILE
#define JADE_DEBUG_EXPORTS 1
#else
#define JADE_DEBUG_EXPORTS 0
#endif
#endif

struct alignas(8) QueueCtl {
  uint32_t count;   // rays emitted by the last shade pass          } one 64-bit word: k_shade reserves its queue
  uint32_t active;  // records with rays in flight after that pass } and list space with ONE atomic per block
  uint32_t next;    // next unclaimed queue entry (trace)
  uint32_t heavy;   // records k_shade_lean handed to k_shade this pass
  uint32_t fp_bad;  // jade_fp_selftest result (checked once)
  uint32_t pad[3];
};

// A step hands its unfinished paths to the next step (or to flush) once fewer than JADE_CARRY_FRACTION of the records it
// started with are still active.  The paths left are the long ones (jade: ~10 bounces against 1-2 for the sky and the
// mirror floor): finishing them inside every step means dozens of thin passes per step, whose sparse record accesses
// waste most of every cache line; carried over, they ride along with the next step's full passes and the thin tail
// is paid once per render (round 1, C3: 364 -> 286 k_trace launches per 4096 spp, +3 % Mray/s at 0.02 against none).  What
// is carried is work moved, not saved: the flush at the end of a render finishes it, so the fraction sets how long that
// flush is - round 3, 4 x 1024 spp of C3 with the flush inside the clock: 0.001 / 0.002 / 0.003 / 0.005 / 0.02 / 0.05 = 708.6 /
// 707.9 / 705.5 / 705.4 / 709.5 / 698 + 167 ms per step, with a final flush of 32 / 40 / 49 / 67 / 210 / 669 ms.  0.003: as fast as
// any, and a render's last call returns in 49 ms.  JADE_CARRY_FRACTION in the environment overrides it (0 = only the
// absolute floor below).
#ifndef JADE_CARRY_FRACTION
#define JADE_CARRY_FRACTION 0.003
#endif
#ifndef JADE_CARRY_RECORDS
#define JADE_CARRY_RECORDS 32768u /* ... and in any case once fewer than this (and < 0.1 % of its records) are active */
#endif
#define JADE_CTL_RING 96 /* QueueCtl records: entry 0 for passes the host follows one by one, all of them for a batch of passes (round 4: 96 - a 1024-spp step of C3 is ~65 passes down to its carry-over point, the flush ~65 more down to k_tail's threshold: one batch, one wait each; the launches behind the stop are empty) */
#ifndef JADE_TAIL_MAX
#define JADE_TAIL_MAX 32768u /* records: a shorter active list is finished by k_tail instead of by further passes */
#endif
#ifndef JADE_SORT_GEOMETRY_BYTES
#define JADE_SORT_GEOMETRY_BYTES ((size_t)16 << 20) /* node + pair records above which the ray queue is ordered by default: four XCD L2s' worth */
#endif
#ifndef JADE_PACKET_BUDGET
#define JADE_PACKET_BUDGET 32 /* C3: k_light 153 / 159 / 167 / 181 ms per step at 16 / 32 / 64 / 128, and the step as a whole fastest at 32 (a lower budget hands more samples to the wavefront passes); C5: 32 / 33 / 36 ms at 16 / 32 / 64 */
#endif

// sets the calling thread's jade_last_error() text and returns `code` (jade_hip.hip)
int jade_fail(int code, const std::string& msg);
#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return jade_fail(e_ == hipErrorOutOfMemory ? JADE_ERR_NOMEM : JADE_ERR_DEVICE,       \
                       std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    bytes = 0;
    const hipError_t e = hipMalloc(&p, n ? n : 16);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct DevEvent {  // an event that is destroyed on every return path
  hipEvent_t e = nullptr;
  ~DevEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreate(&e); }
  operator hipEvent_t() const { return e; }
};
// the scene's events are made on first use and kept
template <size_t N>
static hipError_t ensure_events(DevEvent (&ev)[N]) {
  for (DevEvent& e : ev)
    if (!e.e)
      if (const hipError_t r = e.create(); r != hipSuccess) return r;
  return hipSuccess;
}

// Copies on `stream` and waits for it: the scene's stream is non-blocking, so a copy on the null stream would
// not be ordered before the kernels launched on it.
template <class T>
static hipError_t upload(DevBuf& b, const T* src, size_t count, hipStream_t stream) {
  hipError_t e = b.alloc(sizeof(T) * count);
  if (e != hipSuccess) return e;
  if (count) {
    e = hipMemcpyAsync(b.p, src, sizeof(T) * count, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  return e;
}

// Development switches, read from the environment ONCE, at jade_scene_create (the product path reads no environment
// variable per call).  Every one of them changes the schedule only, never a result (tests/test_gpu_parity.py).
struct Tunables {
  bool shade_split = true;    // JADE_SHADE_SPLIT=0: k_shade alone over the active list from the first pass on
  bool fused = true;          // JADE_FUSED=0: the step's first pass as k_shade_lean + k_shade + k_trace instead of k_light
  bool batching = true;       // JADE_BATCH=0: the host follows every pass
  bool carry = true;          // JADE_CARRY=0: every step finishes all its paths
  double carry_frac = JADE_CARRY_FRACTION;
  bool log_passes = false;    // JADE_LOG_PASSES: one line per pass on stderr (forces one host wait per pass)
  bool pixel_rotate = false;  // JADE_PIXEL_ROTATE=1
  int records_per_pixel = 0;  // JADE_RECORDS_PER_PIXEL: test hook, results must not depend on it
  int trace_blocks_per_cu = 0;  // JADE_TRACE_BLOCKS_PER_CU: occupancy sweeps
  bool force_rccl = false;    // JADE_FORCE_RCCL=1 (tests): the RCCL path for a single share too
  bool sort_keys_kernel = false;  // JADE_SORT_KEYS_KERNEL=1: the keys of an ordered queue come from k_ray_keys (a kernel per pass) instead of from the queueing kernel
  int sort_mode = -1;         // JADE_SORT: order the ray queue by (kind, source triangle, octant) before every k_trace launch (host-followed
                              // passes): 1 always, 0 never, unset = when the traversal's records do not fit the L2 (jade_scene.sort_rays)
  uint32_t sort_min = 65536;  // JADE_SORT_MIN: queues shorter than this are traced as they are
  bool light_packet = true;   // JADE_LIGHT_PACKET=0: the fused first pass walks its rays per lane (k_light) instead of as packets
  int packet_budget = JADE_PACKET_BUDGET;  // JADE_PACKET_BUDGET: records a packet may read before it is given up and walked per lane
  int wide_mode = -1;         // JADE_WIDE: with early exits k_trace walks four grandchildren per visit (k_trace_wide): 1 always, 0 never, unset =
                              // when the traversal's records do not fit the L2 (the rule of sort_mode; jade_scene_create then builds wide records)
  bool ray_records = true;    // JADE_RAY_RECORDS=0: k_trace's refill gathers every ray through its queue entry (before round 4)
  bool shade_binned = false;  // JADE_SHADE_BINNED=1: k_shade_binned - the records of a block dealt by branch through LDS (measured level with k_shade: DESIGN.md 3.4)
  bool tail = true;           // JADE_TAIL=0: no k_tail - the last paths are finished by passes, as before round 4
  uint32_t tail_max = JADE_TAIL_MAX;  // JADE_TAIL_MAX: active records at or below which k_tail takes over
  bool anyhit = true;         // JADE_ANYHIT=0: no occluder cache (JADE_WALK_EARLY_EXIT_CACHED then walks as JADE_WALK_EARLY_EXIT)
  long long rayq_cap = 0;     // JADE_RAYQ_CAP=<entries>: test hook - lowers PathState.rayq_cap (never raises it; b_rayq keeps the rule's size), so that a
                              // small render queues rays on both sides of the record boundary (ray_record_cap; tests/test_gpu_ray_records.py).  <= 0: the rule
  uint32_t trace_chunk_rays = 0;  // JADE_TRACE_CHUNK_RAYS=<64|128|...|512>: test hook - the rays a wave of k_trace claims per queue atomic, in place of the
                              // rule's answer on the host and on the device (trace_chunk_for; tests/test_gpu_trace_chunks.py); k_tail claims nothing.
                              // Anything but a multiple of 64 in 64..512 is ignored.  Results must depend on neither hook
  void read() {
    auto flag0 = [](const char* n) { const char* e = getenv(n); return e && atoi(e) == 0; };
    anyhit = !flag0("JADE_ANYHIT");
    tail = !flag0("JADE_TAIL");
    if (const char* e = getenv("JADE_TAIL_MAX")) tail_max = (uint32_t)atoi(e);
    auto flag1 = [](const char* n) { const char* e = getenv(n); return e && atoi(e) > 0; };
    shade_binned = flag1("JADE_SHADE_BINNED");
    ray_records = !flag0("JADE_RAY_RECORDS");
    shade_split = !flag0("JADE_SHADE_SPLIT");
    fused = shade_split && !flag0("JADE_FUSED");
    batching = !flag0("JADE_BATCH");
    carry = !flag0("JADE_CARRY");
    if (const char* e = getenv("JADE_CARRY_FRACTION")) carry_frac = atof(e);
    log_passes = getenv("JADE_LOG_PASSES") != nullptr;
    pixel_rotate = flag1("JADE_PIXEL_ROTATE");
    if (const char* e = getenv("JADE_RECORDS_PER_PIXEL")) records_per_pixel = atoi(e);
    if (const char* e = getenv("JADE_TRACE_BLOCKS_PER_CU")) trace_blocks_per_cu = atoi(e);
    force_rccl = getenv("JADE_FORCE_RCCL") != nullptr;
    light_packet = !flag0("JADE_LIGHT_PACKET");
    if (const char* e = getenv("JADE_SORT")) sort_mode = atoi(e) > 0 ? 1 : 0;
    if (const char* e = getenv("JADE_SORT_KEYS_KERNEL")) sort_keys_kernel = atoi(e) > 0;
    if (const char* e = getenv("JADE_SORT_MIN")) sort_min = (uint32_t)atoi(e);
    if (const char* e = getenv("JADE_PACKET_BUDGET")) packet_budget = atoi(e);
    if (const char* e = getenv("JADE_WIDE")) wide_mode = atoi(e) > 0 ? 1 : 0;
    if (const char* e = getenv("JADE_RAYQ_CAP")) rayq_cap = atoll(e);
    if (const char* e = getenv("JADE_TRACE_CHUNK_RAYS")) trace_chunk_rays = (uint32_t)atoi(e);
  }
};

// The ray queue's record boundary (setup_state): of `slots` queue positions the first ray_record_cap have a 48-B ray record (PathState.rayq) -
// an eighth of all slots, but every slot of a render of up to 2^22; none when the records are switched off.  hook > 0 (JADE_RAYQ_CAP) may
// only lower the answer.  Pure: no HIP call, no scene (tests/test_queue_rules_cpu.py).
static inline size_t ray_record_cap(size_t slots, bool enabled, long long hook) {
  size_t cap = enabled ? std::max<size_t>((slots + 7) / 8, std::min<size_t>(slots, (size_t)1 << 22)) : 0;
  cap = std::min<size_t>(cap, slots);
  if (hook > 0) cap = std::min<size_t>(cap, (size_t)hook);
  return cap;
}
// Rays claimed per queue atomic by a wave of k_trace: large launches amortise the atomic over up to JADE_TRACE_CHUNK rays, small ones keep
// 64 so every wave gets work (the aim: >= 8 claims per wave).  trace_body states the same rule on the device for batched passes, whose
// queue length the host has not seen.  hook (JADE_TRACE_CHUNK_RAYS): a multiple of 64 in 64..JADE_TRACE_CHUNK replaces the answer, anything
// else is ignored.  Pure.
static inline bool trace_chunk_hook_ok(uint32_t hook) { return hook >= 64u && hook <= (uint32_t)JADE_TRACE_CHUNK && hook % 64u == 0u; }
static inline uint32_t trace_chunk_for(uint32_t n_rays, uint64_t waves, uint32_t hook) {
  if (trace_chunk_hook_ok(hook)) return hook;
  uint64_t per = n_rays / (std::max<uint64_t>(waves, 1) * 64 * 8);
  if (per < 1) per = 1;
  if (per > JADE_TRACE_CHUNK / 64) per = JADE_TRACE_CHUNK / 64;
  return (uint32_t)per * 64u;
}

// The mode of a render: which non-parity pieces its shade kernels carry, one bit each.  0 is the parity shading - the reference's
// estimator through the pinhole, the only mode k_tail, k_shade_binned and the oracle know.
enum ShadeMode : uint32_t {
  SM_ENVIS = 1u,     // jade_render_params.env_sampling = JADE_ENV_IMPORTANCE
  SM_LENS = 2u,      // jade_scene_set_lens with a radius > 0
  SM_SHUTTER = 4u,   // jade_scene_set_shutter
  SM_LIGHTS = 8u,    // jade_scene_set_light_sampling = JADE_LIGHTS_ONE
  SM_COSINE = 16u,   // jade_scene_set_bounce_sampling = JADE_BOUNCE_COSINE
  SM_MIS = 32u,      // jade_scene_set_direct_sampling = JADE_DIRECT_MIS
  SM_ENVMIX = 64u,   // jade_render_params.env_sampling = JADE_ENV_MIXTURE: raised together with SM_ENVIS, whose record steps it shares
  SM_PASSES = 128u,  // jade_scene_set_passes: the frame's radiance kept split into the light passes as well (include/jade_bvh.h, "The passes, stated")
  SM_BRANCH = 256u,  // jade_scene_set_branch_sampling = JADE_BRANCH_STRATIFIED: the branch draws of a path's first two vertices shared out (include/jade_bvh.h, "The branch draws, stated")
  SM_SMOOTH = 512u,  // jade_scene_set_vertex_normals with at least one triangle that is not flat: the vertex normals interpolated at every path vertex (include/jade_bvh.h, "The shading normal, stated")
  SM_TEX = 1024u,    // jade_scene_set_textures with at least one triangle that names an image: the image filtered at every path vertex (include/jade_bvh.h, "The surface colour, stated").  Raised together with SM_SMOOTH, whose family it runs
  SM_NMAP = 2048u,   // jade_scene_set_normal_maps with at least one mapped triangle: the tangent-space image bends the shading normal at every path vertex (include/jade_bvh.h, "The mapped normal, stated").  Raised together with SM_TEX | SM_SMOOTH, whose family it runs
};
// How the device code reads a mode: whether mask M carries bit b.  The shade kernels and every function they are made of (jade_shade.h,
// jade_hip.hip) are templates over the one mask and ask by name - sm(M, SM_COSINE) - so no flag has a position to be wrong in.
static constexpr bool sm(uint32_t M, ShadeMode b) { return (M & (uint32_t)b) != 0; }
// THE list of the modes that are built, written once: X(m) for each, under each of the three environment samplings.  shade_mode_built (so what
// jade_render_begin accepts) and shade_launcher (jade_hip.hip: the kernel a render's passes launch) are both made from it, so a mode
// cannot be accepted without a kernel or have a kernel that is never reached.  Adding a render mode: DESIGN.md 3.14.
#define JADE_SHADE_MODES_BUILT(X) \
  JADE_SHADE_MODE_BOTH_ENV(X, 0u) JADE_SHADE_MODE_BOTH_ENV(X, SM_LENS) JADE_SHADE_MODE_BOTH_ENV(X, SM_SHUTTER) JADE_SHADE_MODE_BOTH_ENV(X, SM_SHUTTER | SM_LENS) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_LIGHTS) JADE_SHADE_MODE_BOTH_ENV(X, SM_COSINE) JADE_SHADE_MODE_BOTH_ENV(X, SM_COSINE | SM_LIGHTS) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_COSINE | SM_MIS) JADE_SHADE_MODE_BOTH_ENV(X, SM_COSINE | SM_MIS | SM_LIGHTS) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_PASSES) JADE_SHADE_MODE_BOTH_ENV(X, SM_PASSES | SM_COSINE) JADE_SHADE_MODE_BOTH_ENV(X, SM_PASSES | SM_COSINE | SM_MIS) JADE_SHADE_MODES_BRANCH(X) JADE_SHADE_MODES_SMOOTH(X) JADE_SHADE_MODES_TEX(X) JADE_SHADE_MODES_NMAP(X)
// ... its rows under SM_BRANCH: the pinhole with all lights - the reference estimator, the cosine bounce, MIS - and the passes on the reference estimator
#define JADE_SHADE_MODES_BRANCH(X) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_BRANCH) JADE_SHADE_MODE_BOTH_ENV(X, SM_BRANCH | SM_COSINE) JADE_SHADE_MODE_BOTH_ENV(X, SM_BRANCH | SM_COSINE | SM_MIS) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_BRANCH | SM_PASSES)
// ... and under SM_SMOOTH: the reference estimator, the cosine bounce, the lens - all lights, no shutter, no MIS, no passes, the stream's branch draws
#define JADE_SHADE_MODES_SMOOTH(X) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_SMOOTH) JADE_SHADE_MODE_BOTH_ENV(X, SM_SMOOTH | SM_COSINE) JADE_SHADE_MODE_BOTH_ENV(X, SM_SMOOTH | SM_LENS)
// ... and the same three rows with textures: a textured render runs the smooth family whether the handle carries vertex normals or not
#define JADE_SHADE_MODES_TEX(X) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_TEX | SM_SMOOTH) JADE_SHADE_MODE_BOTH_ENV(X, SM_TEX | SM_SMOOTH | SM_COSINE) JADE_SHADE_MODE_BOTH_ENV(X, SM_TEX | SM_SMOOTH | SM_LENS)
// ... and once more with normal maps: a mapped render runs the textured family whether the handle carries textures or not
#define JADE_SHADE_MODES_NMAP(X) \
  JADE_SHADE_MODE_BOTH_ENV(X, SM_NMAP | SM_TEX | SM_SMOOTH) JADE_SHADE_MODE_BOTH_ENV(X, SM_NMAP | SM_TEX | SM_SMOOTH | SM_COSINE) JADE_SHADE_MODE_BOTH_ENV(X, SM_NMAP | SM_TEX | SM_SMOOTH | SM_LENS)
#define JADE_SHADE_MODE_BOTH_ENV(X, m) X((m)) X((m) | SM_ENVIS) X((m) | SM_ENVIS | SM_ENVMIX)
static inline bool shade_mode_built(uint32_t mode) {
#define JADE_X(m) if (mode == (m)) return true;
  JADE_SHADE_MODES_BUILT(JADE_X)
#undef JADE_X
  return false;
}
// What jade_render_begin makes of the settings a render is asked with: JADE_OK and its mode, or the refusal's code and text.  A mode
// is accepted if and only if it is in the list above; the texts say why the others are not, first reason first: one-light sampling's
// own check, then the cosine bounce's, then what MIS needs.  Pure: no HIP call, no scene (tests/test_shade_modes_cpu.py).
// env_sampling: JADE_ENV_* (a value jade_render_begin has checked); the mixture is refused exactly where importance is, in the same words.
// passes: jade_scene_set_passes.  Their kernels are built for the pinhole with all lights; a refusal of theirs comes after the others', which
// keep their texts whether passes are on or not.
// branch: jade_scene_set_branch_sampling = JADE_BRANCH_STRATIFIED.  Its kernels are built for the pinhole with all lights as well, and for the passes on
// the reference estimator; its refusals come last, after everybody else's, whose texts stay.
// smooth: jade_scene_set_vertex_normals with a table that is not flat everywhere.  Its kernels are built for the reference estimator and the cosine
// bounce through the pinhole and for the reference estimator through a lens; its refusals come after all of the above, whose texts stay.
// textures: jade_scene_set_textures with a table in which a triangle names an image.  They run the smooth family (SM_SMOOTH is raised with SM_TEX,
// whether the handle carries vertex normals or not) and are refused where it is, in its words.
// normal_maps: jade_scene_set_normal_maps with a table in which a triangle is mapped.  They run the textured family (SM_TEX | SM_SMOOTH are raised
// with SM_NMAP, whatever else the handle carries) and are refused where textures are, in the same words - their own name where neither other table is set.
static inline int shade_mode_for(int env_sampling, bool lens, bool shutter, int light_sampling, int bounce_sampling, int direct_sampling, uint32_t* mode,
                                 std::string* why, bool passes = false, bool branch = false, bool smooth = false, bool textures = false, bool normal_maps = false) {
  const uint32_t m = (env_sampling == JADE_ENV_IMPORTANCE ? SM_ENVIS : env_sampling == JADE_ENV_MIXTURE ? SM_ENVIS | SM_ENVMIX : 0u) | (lens ? SM_LENS : 0u) | (shutter ? SM_SHUTTER : 0u) | (light_sampling == JADE_LIGHTS_ONE ? SM_LIGHTS : 0u) |
                     (bounce_sampling == JADE_BOUNCE_COSINE ? SM_COSINE : 0u) | (direct_sampling == JADE_DIRECT_MIS ? SM_MIS : 0u) | (passes ? SM_PASSES : 0u) |
                     (branch ? SM_BRANCH : 0u) | (smooth || textures || normal_maps ? SM_SMOOTH : 0u) | (textures || normal_maps ? SM_TEX : 0u) | (normal_maps ? SM_NMAP : 0u);
  if (shade_mode_built(m)) {
    *mode = m;
    return JADE_OK;
  }
  // smooth shading's and the textures' own refusals: only where the same settings without the table are accepted - otherwise the refusal a caller
  // reads is the one they would read without it, in the same words.  With both tables on the handle the words are smooth shading's.
  if ((m & SM_SMOOTH) && shade_mode_built(m & ~(uint32_t)(SM_SMOOTH | SM_TEX | SM_NMAP))) {
    const std::string who = smooth     ? "smooth shading (jade_scene_set_vertex_normals) does not run "
                            : textures ? "textures (jade_scene_set_textures) do not run "
                                       : "normal maps (jade_scene_set_normal_maps) do not run ";
    const char* built = " yet: those kernels are not built";
    if (m & SM_SHUTTER)
      *why = who + "together with a shutter (jade_scene_set_shutter)" + built;
    else if (m & SM_LIGHTS)
      *why = who + "together with light sampling JADE_LIGHTS_ONE (jade_scene_set_light_sampling)" + built;
    else if (m & SM_MIS)
      *why = who + "together with direct sampling JADE_DIRECT_MIS (jade_scene_set_direct_sampling)" + built;
    else if (m & SM_PASSES)
      *why = who + "together with passes (jade_scene_set_passes)" + built;
    else if (m & SM_BRANCH)
      *why = who + "together with branch sampling JADE_BRANCH_STRATIFIED (jade_scene_set_branch_sampling)" + built;
    else
      *why = who + "with this combination of render modes" + built;
    return JADE_ERR_UNSUPPORTED;
  }
  const std::string camera = std::string(lens ? "a lens (jade_scene_set_lens)" : "a shutter (jade_scene_set_shutter)") + " yet: those kernels are not built";
  if ((m & SM_LIGHTS) && (m & (SM_LENS | SM_SHUTTER)))
    *why = "light sampling: JADE_LIGHTS_ONE (jade_scene_set_light_sampling) does not run together with " + camera;
  else if ((m & SM_COSINE) && (m & (SM_LENS | SM_SHUTTER)))
    *why = "bounce sampling: JADE_BOUNCE_COSINE (jade_scene_set_bounce_sampling) does not run together with " + camera;
  else if ((m & SM_MIS) && !(m & SM_COSINE))
    *why = "direct sampling: JADE_DIRECT_MIS (jade_scene_set_direct_sampling) weighs the emitter rays against the cosine bounce "
           "and needs JADE_BOUNCE_COSINE (jade_scene_set_bounce_sampling)";
  else if ((m & SM_PASSES) && (m & (SM_LENS | SM_SHUTTER)))
    *why = "passes (jade_scene_set_passes) do not run together with " + camera;
  else if ((m & SM_PASSES) && (m & SM_LIGHTS))
    *why = "passes (jade_scene_set_passes) do not run together with light sampling JADE_LIGHTS_ONE (jade_scene_set_light_sampling) yet: those kernels are not built";
  else if ((m & SM_BRANCH) && (m & (SM_LENS | SM_SHUTTER)))
    *why = "branch sampling: JADE_BRANCH_STRATIFIED (jade_scene_set_branch_sampling) does not run together with " + camera;
  else if ((m & SM_BRANCH) && (m & SM_LIGHTS))
    *why = "branch sampling: JADE_BRANCH_STRATIFIED (jade_scene_set_branch_sampling) does not run together with light sampling JADE_LIGHTS_ONE "
           "(jade_scene_set_light_sampling) yet: those kernels are not built";
  else if ((m & SM_BRANCH) && (m & SM_PASSES))
    *why = "branch sampling: JADE_BRANCH_STRATIFIED (jade_scene_set_branch_sampling) keeps passes (jade_scene_set_passes) under the reference estimator only "
           "(JADE_BOUNCE_UNIFORM, JADE_DIRECT_RAYS) yet: those kernels are not built";
  else
    *why = "this combination of render modes is not built";
  return JADE_ERR_UNSUPPORTED;
}

// The surface tables of a scene handle - vertex normals (jade_smooth.h), textures (jade_texture.h), normal maps (jade_normal_map.h) - kept by
// jade_surface.hip in two parts: what the setters left, which the next jade_render_begin takes, and what the render in progress took, which
// no setter touches.  Adding a per-triangle table: DESIGN.md 3.22.
struct SurfaceImages {  // an image set as jade_texture.h lays it out: the triangles' records, the texels of all images, a head per image
  std::vector<float4> rec, texels;
  std::vector<uint4> images;
  bool any = false;  // a triangle names an image (empty records: no table set)
};
struct SurfaceTables {
  struct {
    std::vector<float4> normals;  // the vertex normals' records (empty: none set) ...
    bool normals_any = false;     // ... and whether any triangle of them is not flat
    SurfaceImages textures;
    SurfaceImages maps;           // (the records without their smooth part: surface_join_maps adds it)
    float strength = 1.0f;        // the maps'
  } set;
  struct {
    DevBuf normals, tex_rec, tex_texels, tex_images, map_rec, map_texels, map_images;
    bool normals_current = false, textures_current = false, maps_current = false;  // the buffers hold what the setters left (surface_begin uploads once)
    DevBuf flat;      // the all-flat vertex normals a textured render reads where the handle carries none (zeros: SMOOTH_FLAT), made on first need
    DevBuf no_image;  // the texture records of a mapped render whose handle names no image (every triangle -1), made on first need
    const float4* tex_normals = nullptr;  // the vertex normals the textured render in progress began with: normals or flat
    bool tex_none = false;                // ... it reads no_image in place of tex_rec
    float strength = 1.0f;                // ... and the maps' strength it began with
  } dev;
};

struct jade_scene {
  int device = 0;
  Tunables tun;
  hipStream_t stream = nullptr;
  DevScene dev{};
  DevBuf b_nodes, b_nodes4, b_tverts, b_tris, b_emit, b_mapping, b_prefix, b_segs, b_env, b_guide, b_guide_obj, b_tnorm, b_mats, b_anyhit, b_env_alias, b_light_alias, b_mis;
  bool boxes_nested = true;   // every child's box lies inside its parent's (jade_scene_create): what the wide walk and the occluder cache need
  int n_emit = 0;
  int n_objects = 0;
  int bvh_depth = 0;
  // what the next jade_render_begin takes (the setters' state; jade_render_multi compares it between scenes) ...
  jade_lens_params lens{};    // jade_scene_set_lens
  jade_shutter_params shutter{};  // jade_scene_set_shutter, if shutter_set
  bool shutter_set = false;
  int light_sampling = JADE_LIGHTS_ALL;       // jade_scene_set_light_sampling
  int bounce_sampling = JADE_BOUNCE_UNIFORM;  // jade_scene_set_bounce_sampling
  int direct_sampling = JADE_DIRECT_RAYS;     // jade_scene_set_direct_sampling
  bool passes = false;                        // jade_scene_set_passes
  int branch_sampling = JADE_BRANCH_RANDOM;   // jade_scene_set_branch_sampling
  SurfaceTables surf;                         // jade_scene_set_vertex_normals / _textures / _normal_maps, and what the render in progress took of them
  // ... and what the render in progress took, whatever the setters are told before the next begin: its mode (ShadeMode bits; read through
  // the predicates below), with rc.lens_radius + ps.lens_k under SM_LENS and the shutter kernels' argument under SM_SHUTTER
  uint32_t mode = 0;
  ShutterConst sh{};
  bool sort_rays = false;     // the ray queue is ordered before every k_trace launch (Tunables.sort_mode; then passes are host-followed)
  // render state
  bool have_rp = false;
  jade_render_params rp{};
  RenderConst rc{};
  PathState ps{};
  DevBuf b_sortkey, b_sortkey2, b_sortpos, b_sortq, b_sorttmp;  // JADE_SORT: keys in / out, the entries' positions, the ordered queue (of positions), rocPRIM's temporary storage
  size_t sort_cap = 0, sort_tmp_bytes = 0;
  double sort_ms = 0;
  DevBuf b_state, b_sum, b_tiles, b_queue, b_rayq, b_active[2], b_ctl, b_ctr, b_spill, b_out_rgb, b_out_bgr, b_wavecnt;
  std::vector<int32_t> tile_ids;
  int trace_blocks = 0;
  int trace_blocks_wide = 0;  // ... of k_trace_wide (fewer waves per SIMD)
  int light_blocks = 0;       // persistent grid of k_light
  int packet_blocks = 0;      // ... and of k_light_packet (0: the tree is too deep for the packet form)
  double packets_given_up = 0;  // share of the last fused pass's packets that were given up (reset by jade_render_begin)
  int64_t spp_done = 0;
  bool tail_pending = false;  // the last step left its longest paths unfinished (jade_render_flush)
  uint32_t carried_active = 0;  // ... this many records (0: unknown)
  int64_t rays_recorded = 0, rays_indexed = 0;  // rays k_trace took since jade_render_begin from queue positions below PathState.rayq_cap / at or beyond it,
                                                // from the queue counts the host reads anyway (count_queue; jade_debug_ray_record_use)
  DevEvent ev[7];             // run_passes' timing events, made once (ev0, ev1, ta, tb, sa, sb, sm)
  DevEvent ev_resolve;  // jade_render_resolve_tiles_device: caller's stream -> scene stream
  uint64_t host_syncs = 0;    // host waits inside step/flush since the last advance() reported them
  double light_ms = 0;        // k_light device time since then
  DevEvent ev_light[2];
  DevEvent ev_tail[2];
  double tail_ms = 0;         // k_tail device time since the last advance() reported it
  uint64_t tail_launches = 0, tail_records = 0;
  DevEvent ev_batch[2 * JADE_CTL_RING];  // k_trace timing of a batch of passes
  // adaptive sampling (jade_render_adaptive, jade_adaptive.hip): samples of each owned tile once the render has ended (empty: every
  // tile has spp_done), their reciprocals for k_resolve, the rounds' active lists, per-tile counts and {count, not-idle} word
  std::vector<int32_t> tile_n;
  bool adaptive_done = false;  // jade_render_step refuses until the next begin
  DevBuf b_tile_inv, b_tile_n, b_alist[2], b_actl, b_err;
  DevEvent ev_err[2];
  // denoiser (jade_denoise.hip), allocated on first use and kept: the guide pass's throw-away PathState (orgs, slot, hitp), per-pixel
  // state {throughput, depth} and mirror count, the list of owned in-image pixels and two ray queues, its own queue words and work
  // counters (the render's are not touched), the guide sums {albedo, depth} {normal, 0}, the variance, the filter's records (two
  // colour buffers, normal + depth, albedo) and the output images
  DevBuf b_dn_orgs, b_dn_slot, b_dn_hitp, b_dn_state, b_dn_mirrors, b_dn_list, b_dn_q[2], b_dn_ctl, b_dn_ctr, b_dn_az, b_dn_n, b_dn_var;
  DevBuf b_dn_rec[4], b_dn_rgb, b_dn_bgr;
  // the work counters of the flush a denoiser entry point made (carried paths finished early): handed to the next step / flush's
  // statistics, so that a render's counters do not depend on whether it was denoised between its steps
  jade_stats dn_carried{};
  // exposure (jade_expose.hip), allocated on first use and kept: k_meter's rows (one histogram per block) and their sum
  DevBuf b_ex_rows, b_ex_meter;
  // glare (jade_glare.hip), allocated on first use and kept: the frame in image layout (glared in place), its bytes, and every level
  // of the pyramid in one allocation
  DevBuf b_gl_rgb, b_gl_bgr, b_gl_pyr;
  // despeckle (jade_despeckle.hip), allocated on first use and kept: each pixel's scale and the report's four words (its passes run on
  // the denoiser's records, b_dn_rec[0] and [1])
  DevBuf b_ds_scale, b_ds_report;
  // passes (jade_shade.h PassPlanes, jade_passes.hip): the planes of a render with SM_PASSES - cleared by its jade_render_begin - and the
  // 15 resolved images in the compact tile layout, allocated on first use and kept
  DevBuf b_pass_cur, b_pass_tot, b_pass_mask, b_pass_out;
  ~jade_scene() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};
// The render in progress, asked by what its mode means to the schedule:
static inline bool lens_on(const jade_scene* s) { return (s->mode & SM_LENS) != 0; }
static inline bool shutter_on(const jade_scene* s) { return (s->mode & SM_SHUTTER) != 0; }
// ... the camera ray has an origin of its own, stored per record: no k_light / k_light_packet, which have no such form
static inline bool own_origin(const jade_scene* s) { return lens_on(s) || shutter_on(s); }
// ... one shadow slot per record, for the entry drawn, whatever the length of the scene's emitter list (k_trace's n_emit, the record layout)
static inline bool one_light_on(const jade_scene* s) { return (s->mode & SM_LIGHTS) != 0; }
// ... the parity shading, the only one k_tail and k_shade_binned carry: no bit at all
static inline bool parity_shading(const jade_scene* s) { return s->mode == 0; }
// ... the passes are kept: the list schedule a lens runs - k_light, k_light_packet, k_tail and k_shade_binned have no such form
static inline bool passes_on(const jade_scene* s) { return (s->mode & SM_PASSES) != 0; }
// ... the branch draws are shared out: the list schedule again - k_light and k_light_packet shade a camera vertex's mirror with the stream's draw
static inline bool branch_on(const jade_scene* s) { return (s->mode & SM_BRANCH) != 0; }
// ... the vertex normals are interpolated: the list schedule once more - k_light, k_light_packet and k_tail shade with the flat normal
static inline bool smooth_on(const jade_scene* s) { return (s->mode & SM_SMOOTH) != 0; }
// ... the textures are read: a smooth render (smooth_on is true as well) whose kernels take the texture tables beside the vertex normals
static inline bool textures_on(const jade_scene* s) { return (s->mode & SM_TEX) != 0; }
// ... and what its kernels take (jade_texture.h): the tables as jade_render_begin left them
static inline TexTables texture_tables(const jade_scene* s) {
  const auto& d = s->surf.dev;
  return TexTables{d.tex_normals, (d.tex_none ? d.no_image : d.tex_rec).as<float4>(), d.tex_texels.as<float4>(), d.tex_images.as<uint4>()};
}
// ... the normal maps are read: a textured render (textures_on is true as well) whose kernels take the map's tables beside the others
static inline bool normal_maps_on(const jade_scene* s) { return (s->mode & SM_NMAP) != 0; }
static inline MapTables map_tables(const jade_scene* s) {
  const auto& d = s->surf.dev;
  return MapTables{texture_tables(s), d.map_rec.as<float4>(), d.map_texels.as<float4>(), d.map_images.as<uint4>(), d.strength};
}
// ... and the vertex normals a smooth render without textures takes
static inline const float4* smooth_table(const jade_scene* s) { return s->surf.dev.normals.as<float4>(); }

// What jade_scene_create uploads, prepared on the host without a HIP call (jade_scene_prep.hip), and the facts derived from it.
struct ScenePrep {
  std::vector<float4> nodes, nodes4, tverts, tnorm;  // binary records, wide records (empty: none), pair records, flat normal + material number
  std::vector<uint32_t> guide;                        // BSSRDF exit-point guide tables ...
  std::vector<uint2> guide_obj;                       // ... and each object's {first entry, cells}
  std::vector<DevMaterial> mats;
  std::vector<uint4> env_alias;
  std::vector<uint4> light_alias;                     // JADE_LIGHTS_ONE: the alias table over emit_indices (n_emit entries)
  std::vector<float2> mis;                            // JADE_DIRECT_MIS: {m, M} per triangle (n_triangles entries)
  int n_internal = 0;
  size_t n_pairs = 0;
  bool missing_child = false;  // the reference's "child 0" under an internal node: the walk then needs its general form
  bool nested = true;          // every child's box lies inside its parent's
  bool wide_fits = false, cache_fits = false;  // the traversal stack holds a wide walk / a walk that starts with the cached subtrees
  uint32_t root_ref = 0;
  size_t geometry_bytes = 0;   // node + pair records
};
// validate_desc first (the ranges, the tree walked from the root: *depth_out = its levels), then prepare_scene on what it accepted
JADE_HIDDEN int validate_desc(const jade_scene_desc* d, int* depth_out);
JADE_HIDDEN int prepare_scene(const jade_scene_desc& d, int depth, const Tunables& tun, ScenePrep* out);
// ... its guide tables for the BSSRDF exit-point search (exit_search, jade_shade.h): per object {first entry, cells Gn}, and the entries
JADE_HIDDEN void guide_tables(const jade_scene_desc* d, std::vector<uint32_t>& guide, std::vector<uint2>& guide_obj);
// ... its alias table over the environment map's texels (JADE_ENV_IMPORTANCE, include/jade_rt.h), and the map sizes that mode takes:
// env_sample (jade_shade.h) forms the slot from a 24-bit uniform, which reaches every slot of at most 2^24
JADE_HIDDEN void env_alias_table(int32_t env_width, int32_t env_height, const float* env_rgb, std::vector<uint4>& env_alias);
static inline bool env_importance_fits(int32_t env_width, int32_t env_height) {
  return env_width > 0 && env_height > 0 && (uint64_t)env_width * (uint64_t)env_height <= JADE_ENV_IMPORTANCE_MAX_TEXELS;
}
// ... its alias table over the emitter entries (JADE_LIGHTS_ONE, include/jade_bvh.h "The lights, stated": weight = area x luminance of
// emission + a floor), made by env_alias_table's builder, and the emitter counts that mode takes: light_sample (jade_shade.h) forms the
// slot from a 24-bit uniform, as env_sample does
JADE_HIDDEN void light_alias_table(const jade_triangle* triangles, const int32_t* emit_indices, int32_t n_emit, std::vector<uint4>& light_alias);
// ... and its per-triangle table for JADE_DIRECT_MIS (include/jade_bvh.h "The direct light, stated"): {m, M} of a weighted triangle, {0, 0} of
// every other; light_alias is light_alias_table's (n_emit entries, or empty: M = 0)
JADE_HIDDEN void mis_table(const jade_triangle* triangles, int32_t n_triangles, const int32_t* emit_indices, int32_t n_emit,
                           const std::vector<uint4>& light_alias, std::vector<float2>& mis);
static inline bool light_sampling_fits(int64_t n_emit) { return n_emit >= 0 && n_emit <= JADE_LIGHTS_ONE_MAX_ENTRIES; }

// The two places where host code of one file needs a kernel of another (this tree is not built with -fgpu-rdc), both in jade_hip.hip:
// the k_trace / k_trace_wide launch - kernel and grid chosen from (scene, P); n_rays sizes the chunks a wave claims, 0 = the kernel
// sizes them from the queue's length on the device - and k_resolve over the owned pixels.  The caller asks hipGetLastError.
JADE_HIDDEN void launch_trace(jade_scene* s, const PathState& P, const uint32_t* queue, QueueCtl* qc, uint32_t* spill, DevCounters* ctr, uint32_t n_rays);
JADE_HIDDEN int resolve_to(jade_scene* s, int tonemap, float limit, float* dev_rgb, uint8_t* dev_bgr, hipStream_t stream);
// ... and the planes of a render that keeps passes (jade_passes.hip): allocated and cleared by jade_render_begin for npix records
JADE_HIDDEN int passes_setup(jade_scene* s, size_t npix);
// ... and given back by the jade_render_begin of a render that keeps none, with the resolved images
JADE_HIDDEN void passes_release(jade_scene* s);

// The surface tables (jade_surface.hip).  surface_begin: what jade_render_begin does about them once `mode` is accepted - the uploads that are
// due, the stand-in tables on first need, and what the render keeps; it ends the earlier render (have_rp) where a buffer that render reads is
// replaced.  surface_join_maps: the normal maps' records as the setter left them, joined with the vertex normals the handle has now.
// surface_check_images: the check of an image set (textures and normal maps, `who` is the message's prefix) - plain C++, no HIP call, nothing of
// a handle read or written: the heads, the packed texels and whether a triangle names an image, or the refusal
JADE_HIDDEN int surface_begin(jade_scene* s, uint32_t mode);
JADE_HIDDEN std::vector<float4> surface_join_maps(const SurfaceTables& t);
JADE_HIDDEN int surface_check_images(const char* who, int32_t n_images, const jade_texture_image* images, const int32_t* image_of, int32_t n_triangles,
                                     int32_t n_scene, std::vector<uint4>* heads, std::vector<float4>* texels, bool* any);

// What the glare (jade_glare.hip) takes from exposure (jade_expose.hip) rather than copying it: the check of display parameters, the
// grow-only allocation, flush + k_resolve into b_out_rgb (compact tiles), the meter of n pixels at dev_rgb (tile_ids: compact tiles of
// a render; null: a plain image - two kernels, 2 KB back, one wait) and the launch of the tone pack of e x colour.
JADE_HIDDEN int ex_check(const jade_display_params* p);
JADE_HIDDEN hipError_t ex_alloc(DevBuf& b, size_t bytes);
JADE_HIDDEN int ex_resolve(jade_scene* s);
JADE_HIDDEN int ex_meter(DevBuf& b_rows, DevBuf& b_words, const float* dev_rgb, int n, const RenderConst& R, const int32_t* tile_ids, hipStream_t stream,
                         jade_meter* out);
JADE_HIDDEN void ex_launch_pack(const float* dev_rgb, int n, const RenderConst& R, const int32_t* tile_ids, float e, const jade_display_params* p,
                                uint8_t* dev_bgr, hipStream_t stream);

// What the despeckle pass (jade_despeckle.hip) takes from the denoiser (jade_denoise.hip) rather than copying it.  On the host: the check of
// denoise parameters, each owned tile's sample count, the variance of every owned pixel into b_dn_var and the guide sums into b_dn_az /
// b_dn_n (compact layout), and the a-trous passes + output kernel on packed records (rec[0] colour + variance, rec[1] its ping-pong
// partner, rec[2] normal + depth, rec[3] albedo; with iterations = 0 the output kernel alone, which reads rec[0] only).
JADE_HIDDEN int dn_check_params(const jade_denoise_params* dp);
JADE_HIDDEN std::vector<int32_t> dn_tile_counts(const jade_scene* s);
JADE_HIDDEN int dn_variance(jade_scene* s);
JADE_HIDDEN int dn_guides(jade_scene* s, int G);
JADE_HIDDEN int dn_filter_out(hipStream_t stream, int W, int H, const jade_denoise_params* dp, int tonemap, float limit, float* dev_rgb, uint8_t* dev_bgr,
                              float4* const* rec);
// ... and on the device, for the pack kernels of both files:
// owned pixel p (tile t = p >> 8) -> image (x, y); false outside the image (edge tiles)
static __device__ __forceinline__ bool dn_pixel_xy(const RenderConst& R, const int32_t* tile_ids, int p, int* x, int* y) {
  const int tid = tile_ids[p >> 8], l = p & 255;
  *x = (tid % R.tiles_x) * JADE_TILE_SIZE + (l & 15);
  *y = (tid / R.tiles_x) * JADE_TILE_SIZE + (l >> 4);
  return *x < R.width && *y < R.height;
}
// One pixel's filter record from its inputs; every pack kernel calls it, so the render's paths and jade_denoise_image's are the
// same bits.  nhat = n / |n|, or 0 for the zero normal (a miss in every guide sample).  Where the float sum of squares is 0,
// subnormal or infinite, n is first scaled by the power of two that brings its largest component into [1, 2) (exact; every other
// normal takes the plain statements).  L.w = 1 marks an unusable pixel (jade_bvh.h: a non-finite input, a negative variance):
// k_atrous copies it and never taps it.
static __device__ __forceinline__ void dn_pack(float r, float g, float b, float v, float ax, float ay, float az, float nx, float ny, float nz,
                                               float z, float4* A, float4* N, float4* L, size_t o) {
  const bool usable = isfinite(r) && isfinite(g) && isfinite(b) && isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(nx) && isfinite(ny) &&
                      isfinite(nz) && isfinite(z) && isfinite(v) && v >= 0.0f;
  float hx = 0.0f, hy = 0.0f, hz = 0.0f;
  if (usable && (nx != 0.0f || ny != 0.0f || nz != 0.0f)) {
    float ss = nx * nx + ny * ny + nz * nz;
    if (!(ss >= 1.17549435e-38f && ss <= 3.40282347e+38f)) {
      const int e = -ilogbf(fmaxf(fabsf(nx), fmaxf(fabsf(ny), fabsf(nz))));
      nx = ldexpf(nx, e);
      ny = ldexpf(ny, e);
      nz = ldexpf(nz, e);
      ss = nx * nx + ny * ny + nz * nz;
    }
    const float len = sqrtf(ss);
    hx = nx / len;
    hy = ny / len;
    hz = nz / len;
  }
  A[o] = make_float4(r, g, b, v);
  N[o] = make_float4(hx, hy, hz, z);
  L[o] = make_float4(ax, ay, az, usable ? 0.0f : 1.0f);
}

// Visits the owned tiles of a W x H image in owned order: f(t, x0, y0, ww, hh) - owned tile t (its pixels are t*256 + ly*16 + lx in
// the compact layout) covers ww x hh image pixels from (x0, y0).
template <class F>
static void for_each_owned_tile(const std::vector<int32_t>& tile_ids, int W, int H, F&& f) {
  const int tx = (W + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE;
  for (size_t t = 0; t < tile_ids.size(); ++t) {
    const int x0 = (tile_ids[t] % tx) * JADE_TILE_SIZE, y0 = (tile_ids[t] / tx) * JADE_TILE_SIZE;
    f(t, x0, y0, std::min(JADE_TILE_SIZE, W - x0), std::min(JADE_TILE_SIZE, H - y0));
  }
}
