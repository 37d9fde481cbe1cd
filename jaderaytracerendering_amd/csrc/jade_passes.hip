// jade_passes.hip — the light passes of a render (include/jade_bvh.h: jade_pass_name, jade_render_passes; "The passes, stated"): the
// resolve kernel and the host side.  The shade kernels of a mode with SM_PASSES book every addend of a sample's colour in the planes of
// jade_shade.h's PassPlanes; this file makes the 15 images from them.
//
//   k_passes_resolve  one thread per (pass, owned pixel): the pixel's records' totals tot[pass][m * npx + pixel], m = 0 .. rpp - 1, added
//                     in ascending m, times the factor k_resolve gives that pixel (1 / spp_done, or its tile's 1 / n after
//                     jade_render_adaptive); 12 B out per thread, in the compact tile layout of k_resolve's out_rgb, pass by pass.
//
// A wave's 64 threads are 64 neighbouring pixels of one pass: its reads of a record row are 768 contiguous bytes, its writes likewise.
// No LDS, no atomics: every output word has one writer and a fixed order of additions.
#include <cstring>
#include <vector>

#include "jade_runtime.h"
#include "jade_shade.h"

static_assert(PASS_COUNT == JADE_PASS_COUNT, "jade_shade.h's planes and include/jade_bvh.h's images are the same 15 passes");
static_assert(PASS_BACKGROUND == JADE_PASS_BACKGROUND && PASS_EMISSION == JADE_PASS_EMISSION && PASS_SPECULAR_SKY == JADE_PASS_SPECULAR_SKY &&
                  PASS_SAMPLED == JADE_PASS_DIFFUSE_EMITTER_FIRST && PASS_COUNT - 1 == JADE_PASS_BSSRDF_SKY_LATER,
              "pass indices");

#define JADE_PASSES_BLOCK 256

__global__ __launch_bounds__(JADE_PASSES_BLOCK) void k_passes_resolve(PathState P, PassPlanes L, RenderConst R, const int32_t* tile_ids, const float* tile_inv,
                                                                      float inv_spp, float* out) {
  const size_t t = (size_t)blockIdx.x * JADE_PASSES_BLOCK + threadIdx.x;
  const size_t npx = (size_t)P.npx;
  if (t >= npx * PASS_COUNT) return;
  const size_t pass = t / npx;
  const int p = (int)(t - pass * npx);  // owned pixel
  if (tile_inv) inv_spp = tile_inv[p >> 8];
  int x, y;
  jvec3 m = jv(0, 0, 0);
  if (pixel_xy(R, tile_ids, p, &x, &y)) {
    const float* row = L.tot + 3 * (pass * (size_t)L.npix + (size_t)p);  // record m of the pixel: 3 npx floats further on
    jvec3 s = jv(row[0], row[1], row[2]);
    for (int k = 1; k < P.rpp; ++k) {
      const float* r = row + 3 * ((size_t)k * npx);
      s = jv_add(s, jv(r[0], r[1], r[2]));
    }
    m = jv(s.x * inv_spp, s.y * inv_spp, s.z * inv_spp);
  }
  float* o = out + 3 * t;
  o[0] = m.x;
  o[1] = m.y;
  o[2] = m.z;
}

// ---------------------------------------------------------------- host side --

const char* jade_pass_name(int pass) {
  static const char* const names[JADE_PASS_COUNT] = {
      "background",           "emission",           "specular_sky",      "diffuse_emitter_first", "diffuse_emitter_later",
      "diffuse_sky_first",    "diffuse_sky_later",  "sss_emitter_first", "sss_emitter_later",     "sss_sky_first",
      "sss_sky_later",        "bssrdf_emitter_first", "bssrdf_emitter_later", "bssrdf_sky_first", "bssrdf_sky_later"};
  return pass >= 0 && pass < JADE_PASS_COUNT ? names[pass] : nullptr;
}

// jade_render_begin of a render with SM_PASSES: the planes for npix records, cleared (mask = 0 is "nothing gathered", tot = +0)
int passes_setup(jade_scene* s, size_t npix) {
  const size_t n = npix * PASS_COUNT;
  if (s->b_pass_cur.bytes != n * 16) HIP_TRY(s->b_pass_cur.alloc(n * 16));
  if (s->b_pass_tot.bytes != n * 12) HIP_TRY(s->b_pass_tot.alloc(n * 12));
  if (s->b_pass_mask.bytes != npix * 4) HIP_TRY(s->b_pass_mask.alloc(npix * 4));
  HIP_TRY(hipMemsetAsync(s->b_pass_tot.p, 0, n * 12, s->stream));
  HIP_TRY(hipMemsetAsync(s->b_pass_mask.p, 0, npix * 4, s->stream));
  return JADE_OK;
}

void passes_release(jade_scene* s) {
  for (DevBuf* b : {&s->b_pass_cur, &s->b_pass_tot, &s->b_pass_mask, &s->b_pass_out}) b->release();
}

int jade_render_passes(jade_scene* s, float* out) {
  if (!s || !s->have_rp) return jade_fail(JADE_ERR_INVALID, "jade_render_begin not called");
  if (!out) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (!passes_on(s))
    return jade_fail(JADE_ERR_INVALID, "the render in progress keeps no passes: jade_scene_set_passes(scene, 1) before jade_render_begin");
  if (s->spp_done <= 0) return jade_fail(JADE_ERR_INVALID, "no samples rendered yet");
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = jade_render_flush(s, nullptr)) return rc;
  const size_t npx = (size_t)s->ps.npx;
  if (npx == 0) return JADE_OK;
  const size_t n = npx * JADE_PASS_COUNT;
  if (s->b_pass_out.bytes < n * 12) HIP_TRY(s->b_pass_out.alloc(n * 12));
  const float inv = (float)(1.0 / (double)s->spp_done);  // resolve_to's factors (jade_hip.hip)
  const float* tile_inv = s->tile_n.empty() ? nullptr : s->b_tile_inv.as<float>();
  const PassPlanes L{s->b_pass_cur.as<float4>(), s->b_pass_tot.as<float>(), s->b_pass_mask.as<uint32_t>(), (uint32_t)s->ps.npix};
  hipLaunchKernelGGL(k_passes_resolve, dim3((unsigned)((n + JADE_PASSES_BLOCK - 1) / JADE_PASSES_BLOCK)), dim3(JADE_PASSES_BLOCK), 0, s->stream, s->ps, L, s->rc,
                     s->b_tiles.as<int32_t>(), tile_inv, inv, s->b_pass_out.as<float>());
  HIP_TRY(hipGetLastError());
  std::vector<float> h(n * 3);
  HIP_TRY(hipMemcpyAsync(h.data(), s->b_pass_out.p, n * 12, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // scatter every pass's compact tiles into its image, as jade_render_resolve_ex does with the frame; other ranks' pixels untouched
  const int W = s->rp.width, H = s->rp.height;
  for (int pass = 0; pass < JADE_PASS_COUNT; ++pass) {
    float* img = out + (size_t)pass * (size_t)H * (size_t)W * 3;
    const float* src0 = h.data() + (size_t)pass * npx * 3;
    for_each_owned_tile(s->tile_ids, W, H, [&](size_t t, int x0, int y0, int ww, int hh) {
      for (int ly = 0; ly < hh; ++ly)
        memcpy(img + ((size_t)(y0 + ly) * W + x0) * 3, src0 + (t * 256 + (size_t)ly * 16) * 3, (size_t)ww * 12);
    });
  }
  return JADE_OK;
}
