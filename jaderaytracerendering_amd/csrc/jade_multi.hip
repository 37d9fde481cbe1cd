// jade_multi.hip — jade_render_multi (include/jade_rt.h): one frame over several devices.  Every device renders and resolves its
// share of the tiles (one host thread each), the shares are gathered on the first device - RCCL over distinct devices, plain copies
// for a one-GPU rehearsal of the partition - and un-tiled and tone-mapped once on the host.  No kernel lives here: the shares are
// resolved by resolve_to (jade_hip.hip).
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is loaded on first use (jade_render_multi on distinct devices)

#include <cstring>
#include <mutex>
#include <thread>

#include "jade_runtime.h"

// RCCL is loaded on first use (dlopen): the single-GPU product path never needs it, and a process that also hosts
// PyTorch keeps whichever librccl it loaded first.
namespace {
struct Rccl {
  void* h = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool load(std::string* why) {
    if (h) return true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) { *why = std::string("cannot load librccl: ") + dlerror(); return false; }
    auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) *why = std::string("librccl lacks ") + n; return p; };
    CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
    GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
    Send = (decltype(Send))sym("ncclSend");
    Recv = (decltype(Recv))sym("ncclRecv");
    GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
    return CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString;
  }
};
Rccl g_rccl;
}  // namespace

// Communicators are made once per device list and kept for the life of the process (ncclCommInitAll is a bootstrap of
// all ranks: tens of milliseconds on 8 GPUs - not something to pay inside every frame).
namespace {
struct CommSet {
  std::vector<int> devs;
  std::vector<ncclComm_t> comms;
};
std::mutex g_comm_mu;
std::vector<CommSet> g_comm_sets;
}  // namespace

// Gather of every share's resolved tile buffer (scenes[i]->b_out_rgb, npx * 3 floats) into `dst` on scenes[0]'s device,
// share i at off[i]: one communicator per device from this one process, all sends and receives in one group.
static int rccl_gather(jade_scene* const* scenes, int ndev, float* dst, const std::vector<size_t>& off) {
  std::string why;
  std::lock_guard<std::mutex> lock(g_comm_mu);  // one gather at a time per process: the communicators are shared
  if (!g_rccl.load(&why)) return jade_fail(JADE_ERR_DEVICE, why);
  std::vector<int> devs(ndev);
  for (int i = 0; i < ndev; ++i) devs[i] = scenes[i]->device;
  CommSet* cs = nullptr;
  for (CommSet& c : g_comm_sets)
    if (c.devs == devs) cs = &c;
  if (!cs) {
    CommSet fresh;
    fresh.devs = devs;
    fresh.comms.assign(ndev, nullptr);
    const ncclResult_t r = g_rccl.CommInitAll(fresh.comms.data(), ndev, devs.data());
    if (r != ncclSuccess) return jade_fail(JADE_ERR_DEVICE, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r));
    g_comm_sets.push_back(std::move(fresh));
    cs = &g_comm_sets.back();
  }
  const std::vector<ncclComm_t>& comms = cs->comms;
  // every exit below this line goes through GroupEnd: an open group would stall the next RCCL user of the process
  ncclResult_t r = g_rccl.GroupStart();
  const bool opened = r == ncclSuccess;
  const char* dev_err = nullptr;
  for (int i = 1; i < ndev && r == ncclSuccess && !dev_err; ++i) {
    const size_t count = (size_t)scenes[i]->ps.npx * 3;
    if (!count) continue;
    if (hipSetDevice(scenes[i]->device) != hipSuccess) { dev_err = "hipSetDevice failed"; break; }
    r = g_rccl.Send(scenes[i]->b_out_rgb.p, count, ncclFloat, 0, comms[i], scenes[i]->stream);
    if (r != ncclSuccess) break;
    if (hipSetDevice(scenes[0]->device) != hipSuccess) { dev_err = "hipSetDevice failed"; break; }
    r = g_rccl.Recv(dst + off[i], count, ncclFloat, i, comms[0], scenes[0]->stream);
  }
  if (opened) {
    const ncclResult_t r2 = g_rccl.GroupEnd();
    if (r == ncclSuccess) r = r2;
  }
  if (dev_err || r != ncclSuccess) {
    // a communicator that saw a failed send / receive / group may be in an error state: it is destroyed and forgotten, the next
    // gather over these devices bootstraps fresh ones
    for (size_t k = 0; k < g_comm_sets.size(); ++k)
      if (&g_comm_sets[k] == cs) {
        for (ncclComm_t c : g_comm_sets[k].comms)
          if (c) (void)g_rccl.CommDestroy(c);
        g_comm_sets.erase(g_comm_sets.begin() + (long)k);
        break;
      }
    if (dev_err) return jade_fail(JADE_ERR_DEVICE, dev_err);
    return jade_fail(JADE_ERR_DEVICE, std::string("RCCL gather: ") + g_rccl.GetErrorString(r));
  }
  // rank 0's own share does not travel; then every stream involved drains before the caller reads the buffer
  hipError_t e = hipSetDevice(scenes[0]->device);
  const size_t own = (size_t)scenes[0]->ps.npx * 12;
  if (e == hipSuccess && own) e = hipMemcpyAsync(dst + off[0], scenes[0]->b_out_rgb.p, own, hipMemcpyDeviceToDevice, scenes[0]->stream);
  for (int i = ndev - 1; i >= 0 && e == hipSuccess; --i) {
    e = hipSetDevice(scenes[i]->device);
    if (e == hipSuccess) e = hipStreamSynchronize(scenes[i]->stream);
  }
  if (e != hipSuccess) return jade_fail(JADE_ERR_DEVICE, std::string("RCCL gather: ") + hipGetErrorString(e));
  return JADE_OK;
}

int jade_render_multi(jade_scene* const* scenes, int ndev, const jade_render_params* rp, float* out_rgb, uint8_t* out_bgr8,
                      jade_stats* st) {
  if (!scenes || ndev <= 0 || !rp) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (rp->spp <= 0 || rp->width <= 0 || rp->height <= 0) return jade_fail(JADE_ERR_INVALID, "bad image size or spp");
  for (int i = 0; i < ndev; ++i)
    if (!scenes[i]) return jade_fail(JADE_ERR_INVALID, "null scene");
  // one frame, one camera: every share is rendered under the same lens (jade_scene_set_lens), bit for bit
  for (int i = 1; i < ndev; ++i)
    if (memcmp(&scenes[i]->lens, &scenes[0]->lens, sizeof(jade_lens_params)) != 0)
      return jade_fail(JADE_ERR_INVALID, "the scenes carry different lenses (jade_scene_set_lens): scene " + std::to_string(i) + " against scene 0");
  // ... and under the same shutter (jade_scene_set_shutter), or none
  for (int i = 1; i < ndev; ++i)
    if (scenes[i]->shutter_set != scenes[0]->shutter_set || memcmp(&scenes[i]->shutter, &scenes[0]->shutter, sizeof(jade_shutter_params)) != 0)
      return jade_fail(JADE_ERR_INVALID, "the scenes carry different shutters (jade_scene_set_shutter): scene " + std::to_string(i) + " against scene 0");
  // ... and with the same light, bounce, direct and branch sampling
  static const struct { int jade_scene::*mode; const char* setter; const char* noun; } kSampling[] = {
      {&jade_scene::light_sampling, "jade_scene_set_light_sampling", "light"},
      {&jade_scene::bounce_sampling, "jade_scene_set_bounce_sampling", "bounce"},
      {&jade_scene::direct_sampling, "jade_scene_set_direct_sampling", "direct"},
      {&jade_scene::branch_sampling, "jade_scene_set_branch_sampling", "branch"}};
  for (const auto& k : kSampling)
    for (int i = 1; i < ndev; ++i)
      if (scenes[i]->*k.mode != scenes[0]->*k.mode)
        return jade_fail(JADE_ERR_INVALID, std::string("the scenes carry different ") + k.noun + " sampling modes (" + k.setter + "): scene " + std::to_string(i) + " against scene 0");
  // ... and either every scene carries a surface table that acts or none does: vertex normals that are not flat everywhere, textures in which a
  // triangle names an image, normal maps in which a triangle is mapped
  const auto table_any = [](const jade_scene* s, int k) { return k == 0 ? s->surf.set.normals_any : k == 1 ? s->surf.set.textures.any : s->surf.set.maps.any; };
  static const char* const kTables[] = {"vertex normals (jade_scene_set_vertex_normals)", "textures (jade_scene_set_textures)", "normal maps (jade_scene_set_normal_maps)"};
  for (int k = 0; k < 3; ++k)
    for (int i = 1; i < ndev; ++i)
      if (table_any(scenes[i], k) != table_any(scenes[0], k))
        return jade_fail(JADE_ERR_INVALID, std::string("the scenes do not all carry ") + kTables[k] + ": scene " + std::to_string(i) + " against scene 0");
  // ... and none keeps passes: only the frame is gathered here (each rank renders its share and calls jade_render_passes)
  for (int i = 0; i < ndev; ++i)
    if (scenes[i]->passes)
      return jade_fail(JADE_ERR_UNSUPPORTED, "passes (jade_scene_set_passes) are on for scene " + std::to_string(i) +
                                                 ": jade_render_multi gathers the frame only - render each share with jade_render_begin / jade_render_step and call jade_render_passes per rank");
  // 1. every device renders its share (one host thread each) and resolves it into a device buffer
  std::vector<int> rcs(ndev, JADE_OK);
  std::vector<std::string> msgs(ndev);
  std::vector<jade_stats> sts(ndev);
  for (auto& x : sts) memset(&x, 0, sizeof x);
  auto work = [&](int i) {
    jade_scene* s = scenes[i];
    jade_render_params p = *rp;
    p.tile_rank = i;
    p.tile_nranks = ndev;
    p.device_id = s->device;
    int rc = jade_render_begin(s, &p);
    if (rc == JADE_OK) rc = jade_render_step(s, p.spp, &sts[i]);
    if (rc == JADE_OK) rc = jade_render_flush(s, &sts[i]);
    if (rc == JADE_OK && s->ps.npx > 0) {
      hipError_t e = s->b_out_rgb.alloc((size_t)s->ps.npx * 12);
      if (e != hipSuccess) rc = jade_fail(JADE_ERR_NOMEM, "tile buffer allocation failed");
      if (rc == JADE_OK) rc = resolve_to(s, JADE_TONEMAP_ACES, 0.0f, s->b_out_rgb.as<float>(), nullptr, s->stream);
      if (rc == JADE_OK && hipStreamSynchronize(s->stream) != hipSuccess) rc = jade_fail(JADE_ERR_DEVICE, "stream sync failed");
    }
    rcs[i] = rc;
    if (rc) msgs[i] = jade_last_error();  // the text is thread-local: carry it back to the caller's thread
  };
  std::vector<std::thread> th;
  for (int i = 1; i < ndev; ++i) th.emplace_back(work, i);
  work(0);
  for (auto& t : th) t.join();
  for (int i = 0; i < ndev; ++i)
    if (rcs[i]) return jade_fail(rcs[i], "device share " + std::to_string(i) + ": " + msgs[i]);
  // 2. the ONE exchange step: gather the compact tile buffers on the device of scenes[0].  Distinct devices: an RCCL
  // gather over xGMI (ncclCommInitAll + grouped send/recv, the form ncclGather itself expands to, so
  // that ranks may contribute different tile counts).  The same device several times (a one-GPU rehearsal of the
  // partition): RCCL cannot put two ranks on one device, the shares are copied device-to-device instead.
  jade_scene* s0 = scenes[0];
  HIP_TRY(hipSetDevice(s0->device));
  size_t total = 0;
  std::vector<size_t> off(ndev);
  for (int i = 0; i < ndev; ++i) {
    off[i] = total;
    total += (size_t)scenes[i]->ps.npx * 3;
  }
  DevBuf gather;
  HIP_TRY(gather.alloc(total * 4));
  bool distinct = true;
  for (int i = 0; i < ndev; ++i)
    for (int j = 0; j < i; ++j) distinct = distinct && scenes[i]->device != scenes[j]->device;
  // JADE_FORCE_RCCL=1 (tests): take the RCCL path for a single share too - library load, communicator, empty group
  if (distinct && (ndev > 1 || s0->tun.force_rccl)) {
    if (int rc = rccl_gather(scenes, ndev, gather.as<float>(), off)) return rc;
  } else {
    for (int i = 0; i < ndev; ++i) {
      size_t bytes = (size_t)scenes[i]->ps.npx * 12;
      if (!bytes) continue;
      HIP_TRY(hipMemcpyAsync(gather.as<float>() + off[i], scenes[i]->b_out_rgb.p, bytes, hipMemcpyDeviceToDevice, s0->stream));
    }
  }
  std::vector<float> host(total);
  HIP_TRY(hipMemcpyAsync(host.data(), gather.p, total * 4, hipMemcpyDeviceToHost, s0->stream));
  HIP_TRY(hipStreamSynchronize(s0->stream));
  // 3. un-tile into the caller's frame, tone-map once
  const int W = rp->width, H = rp->height;
  std::vector<float> frame;
  float* dst_rgb = out_rgb;
  if (!dst_rgb) {
    frame.resize((size_t)W * H * 3);
    dst_rgb = frame.data();
  }
  for (int i = 0; i < ndev; ++i)
    for_each_owned_tile(scenes[i]->tile_ids, W, H, [&](size_t t, int x0, int y0, int ww, int hh) {
      for (int ly = 0; ly < hh; ++ly)
        memcpy(dst_rgb + ((size_t)(y0 + ly) * W + x0) * 3, host.data() + off[i] + (t * 256 + (size_t)ly * 16) * 3, (size_t)ww * 12);
    });
  if (out_bgr8)
    for (size_t p = 0; p < (size_t)W * H; ++p)  // k_resolve's own statements on the host (tone_pack_bgr8, jade_device.h): the same bits
      tone_pack_bgr8(jv(dst_rgb[3 * p], dst_rgb[3 * p + 1], dst_rgb[3 * p + 2]), JADE_TONEMAP_ACES, 0.0f, true, out_bgr8 + 3 * p);
  if (st)
    for (int i = 0; i < ndev; ++i) {
      st->rays_primary += sts[i].rays_primary; st->rays_secondary += sts[i].rays_secondary;
      st->rays_shadow += sts[i].rays_shadow; st->rays_env += sts[i].rays_env; st->rays_indirect += sts[i].rays_indirect;
      st->rays_mirror += sts[i].rays_mirror; st->rays_refract += sts[i].rays_refract; st->host_syncs += sts[i].host_syncs;
      st->rays_inline += sts[i].rays_inline;
      st->nodes_inline += sts[i].nodes_inline; st->tris_inline += sts[i].tris_inline;
      st->rays_cached += sts[i].rays_cached; st->rays_tail += sts[i].rays_tail; st->nodes_tail += sts[i].nodes_tail; st->tris_tail += sts[i].tris_tail;
      st->tail_ms = std::max(st->tail_ms, sts[i].tail_ms); st->tail_launches += sts[i].tail_launches;
      st->light_ms = std::max(st->light_ms, sts[i].light_ms);
      st->nodes_visited += sts[i].nodes_visited; st->tris_tested += sts[i].tris_tested;
      st->shaded_hits += sts[i].shaded_hits; st->samples += sts[i].samples;
      st->kernel_ms = std::max(st->kernel_ms, sts[i].kernel_ms);  // the shares run concurrently
      st->trace_ms = std::max(st->trace_ms, sts[i].trace_ms);
      st->trace_launches += sts[i].trace_launches;
    }
  return JADE_OK;
}
