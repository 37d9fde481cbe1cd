// jade_render_cli.cpp — the repo's own C++ front end over the C-ABI HIP module.
//
// Mirrors main() of PathTrace.cu:1484-1741: scene (render_args.txt or a
// built-in configuration) -> BVH -> [boundary: jade_rt.h] -> BMP / PPM / PFM.
// The backend is loaded at run time (dlopen) so this binary has no HIP
// dependency of its own; the default is libjade_hip.so beside the executable.
#include <dlfcn.h>
#include <libgen.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "jade_bvh.h"
#include "jade_host.hpp"
#include "jade_host_c.h"

using namespace jadehost;

struct Api {
  void* h = nullptr;
  int (*abi_version)(void);
  const char* (*backend_name)(void);
  const char* (*last_error)(void);
  int (*scene_create)(const jade_scene_desc*, int, jade_scene**);
  void (*scene_destroy)(jade_scene*);
  int (*render)(jade_scene*, const jade_render_params*, float*, uint8_t*, jade_stats*);
  // include/jade_bvh.h, looked up only for --adaptive: the oracle backend has no such entry point
  int (*render_adaptive)(jade_scene*, const jade_render_params*, int32_t, float, float, float*, uint8_t*, int32_t*, jade_stats*) = nullptr;
  // ... and only for --denoise / --guides (looked up with dlsym alone: without them the backend is refused with status 2)
  void (*denoise_defaults)(jade_denoise_params*) = nullptr;
  int (*render_denoise)(jade_scene*, const jade_denoise_params*, int, float, float*, uint8_t*) = nullptr;
  int (*render_guides)(jade_scene*, int32_t, float*, float*, float*, float*) = nullptr;
  // ... and only for --exposure / --histogram
  void (*display_defaults)(jade_display_params*) = nullptr;
  int (*render_resolve_exposed)(jade_scene*, const jade_display_params*, float*, uint8_t*, float*, jade_meter*) = nullptr;
  int (*expose_image)(int, int32_t, int32_t, const float*, const jade_display_params*, uint8_t*, float*, jade_meter*) = nullptr;
  // ... and only for --despeckle
  void (*despeckle_defaults)(jade_despeckle_params*) = nullptr;
  int (*render_despeckle)(jade_scene*, const jade_despeckle_params*, const jade_denoise_params*, int, float, float*, uint8_t*, float*,
                          jade_despeckle_report*) = nullptr;
  // ... and only for --glare
  void (*glare_defaults)(jade_glare_params*) = nullptr;
  int (*glare_image)(int, int32_t, int32_t, const float*, const jade_glare_params*, float*) = nullptr;
  int (*render_glare)(jade_scene*, const jade_glare_params*, const jade_display_params*, float*, uint8_t*, float*) = nullptr;
  // ... and only for --aperture (jade_trace_rays: --focus-at)
  int (*scene_set_lens)(jade_scene*, const jade_lens_params*) = nullptr;
  jadeh_trace_rays_fn trace_rays = nullptr;
  // ... and only for --shutter-truck / --shutter-orbit
  int (*scene_set_shutter)(jade_scene*, const jade_shutter_params*) = nullptr;
  // ... and only for --one-light
  int (*scene_set_light_sampling)(jade_scene*, int) = nullptr;
  // ... and only for --bounce
  int (*scene_set_bounce_sampling)(jade_scene*, int) = nullptr;
  // ... and only for --direct
  int (*scene_set_direct_sampling)(jade_scene*, int) = nullptr;
  // ... and only for --branch
  int (*scene_set_branch_sampling)(jade_scene*, int) = nullptr;
  // ... and only for --smooth
  int (*scene_set_vertex_normals)(jade_scene*, const float*, int32_t) = nullptr;
  // ... and only for --texture
  int (*scene_set_textures)(jade_scene*, int32_t, const jade_texture_image*, const float*, const int32_t*, int32_t) = nullptr;
  // ... and only for --normal-map
  int (*scene_set_normal_maps)(jade_scene*, int32_t, const jade_texture_image*, const float*, const int32_t*, int32_t, float) = nullptr;
  // ... and only for --passes
  int (*scene_set_passes)(jade_scene*, int) = nullptr;
  int (*render_passes)(jade_scene*, float*) = nullptr;
  const char* (*pass_name)(int) = nullptr;
};

static bool load_api(const std::string& path, Api& a, bool adaptive) {
  a.h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!a.h) {
    fprintf(stderr, "cannot load backend %s: %s\n", path.c_str(), dlerror());
    return false;
  }
#define SYM(field, name)                                            \
  *(void**)(&a.field) = dlsym(a.h, name);                           \
  if (!a.field) { fprintf(stderr, "backend lacks %s\n", name); return false; }
  SYM(abi_version, "jade_abi_version")
  SYM(backend_name, "jade_backend_name")
  SYM(last_error, "jade_last_error")
  SYM(scene_create, "jade_scene_create")
  SYM(scene_destroy, "jade_scene_destroy")
  SYM(render, "jade_render")
  if (adaptive) { SYM(render_adaptive, "jade_render_adaptive") }
#undef SYM
  if (a.abi_version() != JADE_ABI_VERSION) {
    // a stale pair would silently disagree on struct layouts (jade_stats, jade_render_params)
    fprintf(stderr, "backend %s speaks jade_rt ABI %d, this program was built against %d: rebuild both (make)\n", path.c_str(),
            a.abi_version(), JADE_ABI_VERSION);
    return false;
  }
  return true;
}

// one channel: the "Pf" form of PFM (rows bottom to top, as write_pfm's)
static bool write_pfm1(const std::string& path, const float* v, int width, int height) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  fprintf(f, "Pf\n%d %d\n-1.0\n", width, height);
  const size_t n = (size_t)width * height;
  const bool ok = fwrite(v, sizeof(float), n, f) == n;
  return fclose(f) == 0 && ok;
}

static void usage() {
  fprintf(stderr,
          "usage: jade_render (--config NAME | --args render_args.txt) [--width W --height H] [--spp N]\n"
          "                   [--out file.bmp|.ppm|.pfm] [--env sky|file.hdr] [--backend lib.so] [--device N] [--reference-walk] [--env-importance | --env-mixture] [--one-light]\n"
          "                   [--bounce uniform|cosine] [--direct rays|mis] [--branch random|stratified] [--passes PREFIX] [--smooth [DEG]]\n"
          "                   [--texture K=checker[:SIZE[:SQUARES]]|FILE[@PROJECTION]]...\n"
          "                   [--normal-map K=FILE|bumps[:SIZE[:N]][@PROJECTION][:STRENGTH]]...\n"
          "                   [--adaptive REL [--min-spp N] [--error-floor F]] [--denoise] [--guides PREFIX]\n"
          "                   [--glare STRENGTH [--glare-levels N] [--glare-falloff F]]\n"
          "                   [--despeckle [--despeckle-sigmas Z] [--despeckle-gain G] [--despeckle-rank K] [--despeckle-radius R]\n"
          "                    [--despeckle-iterations N] [--despeckle-map FILE.pfm]]\n"
          "                   [--exposure EV|auto [--key K] [--exposure-window LO,HI]] [--histogram FILE]\n"
          "                   [--aperture A (--focus D | --focus-at PX,PY)]\n"
          "  --aperture A: a thin lens of radius A >= 0 (scene units) instead of the pinhole: depth of field (HIP backend only; NOT the\n"
          "                reference's samples; include/jade_bvh.h).  It needs exactly one of --focus D, the depth D > 0 of the plane of focus\n"
          "                along the camera's axis, and --focus-at PX,PY, which focuses on what the centre of pixel (PX, PY) shows (row 0 =\n"
          "                the bottom row) and prints the distance found; onto the sky it exits 1\n"
          "                   [--shutter-truck DX,DY,DZ] [--shutter-orbit DEG [--shutter-pivot X,Y,Z]] [--shutter-interval T0,T1]\n"
          "  --shutter-truck / --shutter-orbit: motion blur (HIP backend only; NOT the reference's samples; include/jade_bvh.h).  The shutter\n"
          "                opens at the configuration's pose and closes at that pose moved by DX,DY,DZ in camera space (x right, y up, z\n"
          "                backwards) and then turned by DEG degrees about the axis through X,Y,Z parallel to the camera's up (default: the\n"
          "                eye, a pan; the subject's position gives a turntable).  --shutter-interval T0,T1 with 0 <= T0 <= T1 <= 1 exposes\n"
          "                that part of the move only (default 0,1).  Keep DEG to a few degrees; with --aperture, both blurs apply\n"
          "  --one-light: every diffuse and sub-surface vertex sends ONE shadow ray, to an emitter drawn by power, instead of one to every emitter\n"
          "               (HIP backend only; NOT the reference's samples; include/jade_bvh.h).  For scenes with many emissive triangles; not together\n"
          "               with --aperture or --shutter-*\n"
          "  --bounce cosine: the environment and indirect rays of every diffuse and sub-surface vertex are drawn with density cos / pi about the\n"
          "                   normal instead of uniformly (HIP backend only; NOT the reference's samples; include/jade_bvh.h).  Same rays per\n"
          "                   sample, less noise under open sky; not together with --aperture or --shutter-*.  uniform is the default\n"
          "  --direct mis: the emitter rays and the indirect ray of every diffuse vertex are weighed against each other (multiple importance\n"
          "                sampling, balance heuristic), which bounds the bright samples next to a lamp (HIP backend only; NOT the reference's\n"
          "                samples; include/jade_bvh.h).  Needs --bounce cosine and implies nothing.  rays is the default\n"
          "  --branch stratified: at a path's first two vertices a pixel's samples share out the coins that choose the arm - mirror or sub-surface,\n"
          "                       SSS or BSSRDF, the mirror's roulette - instead of tossing them (HIP backend only; NOT the reference's samples;\n"
          "                       include/jade_bvh.h).  Same rays per sample on average; not together with --aperture, --shutter-* or --one-light.\n"
          "                       random is the default\n"
          "  --smooth [DEG]: vertex normals for every object - at each corner the angle-weighted mean of the flat normals of the triangles that\n"
          "                       share its vertex and lie within DEG degrees (default 60) of its triangle - interpolated at every path vertex\n"
          "                       (HIP backend only; NOT the reference's image; include/jade_bvh.h).  OBJ vn lines are not read.  Not together\n"
          "                       with --shutter-*, --one-light, --direct mis, --passes or --branch stratified\n"
          "  --texture K=IMAGE[@PROJECTION]: an albedo texture on object K of the scene (0-based, in the order the configuration or the\n"
          "                       arguments file adds its objects), multiplied into its brdf and refract_albedo at every path vertex (HIP backend\n"
          "                       only; NOT the reference's image; include/jade_bvh.h).  IMAGE is a .ppm file (P6, 8 bits, sRGB), a .pfm file\n"
          "                       (linear) or checker[:SIZE[:SQUARES]] (default 256 texels a side in 8 x 8 squares).  The object's own UVs are used\n"
          "                       where it has them (a quad's; an OBJ file's vt lines); otherwise PROJECTION: spherical (the default), planar-x,\n"
          "                       planar-y or planar-z.  May be given once per object.  Not together with what --smooth is not together with\n"
          "  --glare STRENGTH: a share STRENGTH in [0, 1] of every pixel's light is scattered over a pyramid of N blurs (1..12, default 6),\n"
          "                    level k weighing F^(k-1) (default 0.5), and added back (HIP backend only; include/jade_bvh.h).  The order is\n"
          "                    resolve, --denoise, glare, --exposure / tone; the .pfm output is the glared linear frame\n"
          "  --despeckle: a pixel whose luminance stands above G times (default 2) the K-th brightest (1..4, default 2) of its neighbours within\n"
          "               R pixels (1..3, default 1) is scaled down to that bound, unless the variance of its mean puts the excess Z standard\n"
          "               errors (default 2) above it; N passes (0..4, default 1) (HIP backend only; include/jade_bvh.h).  The order is resolve,\n"
          "               despeckle, --denoise, --glare, --exposure / tone.  --despeckle-map FILE.pfm: each pixel's scale (1 = untouched).\n"
          "               The counts of the report go to stderr\n"
          "  --exposure EV: the frame is multiplied by 2^EV before the tone curve (HIP backend only; the .pfm output is never scaled)\n"
          "  --exposure auto: the multiplier comes from the frame's luminance histogram (include/jade_bvh.h): the log-average luminance of\n"
          "                   the pixels between the LO and HI quantiles (default 0.05,0.95) goes to K (default 0.18)\n"
          "  --histogram FILE: the luminance histogram as text: 512 lines `lower edge, count` (8 bins per stop from 2^-32), then the\n"
          "                    counts of the positive, zero, negative and non-finite pixels and the smallest / largest positive luminance\n"
          "                    (HIP backend only).  With --denoise and / or --glare both read the denoised / glared frame\n"
          "  --denoise: write the frame filtered by the edge-aware denoiser (HIP backend only; include/jade_bvh.h, default parameters)\n"
          "  --passes PREFIX: keep the frame's radiance split into the 15 light passes as well and write them as PREFIX.<name>.pfm (background,\n"
          "                   emission, specular_sky, diffuse_emitter_first, ... bssrdf_sky_later; HIP backend only; the frame itself is unchanged;\n"
          "                   not with --aperture, --shutter or --one-light)\n"
          "  --guides PREFIX: write the denoiser's inputs as PREFIX_albedo.pfm, PREFIX_normal.pfm, PREFIX_depth.pfm, PREFIX_variance.pfm\n"
          "                   (HIP backend only; 4 guide samples)\n"
          "  --adaptive REL: adaptive sampling (HIP backend only): each 16x16 tile stops at the first of N, 2N, 4N, ... samples at which\n"
          "                  every pixel's relative standard error of the mean luminance is <= REL; --spp is the cap.  --min-spp N: a power of\n"
          "                  two >= 2 (default 16); --error-floor F > 0 (default 0.01) is added to the mean in the error's denominator\n"
          "  --env-importance: environment-visibility rays drawn by the sky's luminance instead of uniformly (NOT the reference's samples: the\n"
          "                    same image with less noise under a sky with a sun; the oracle backend refuses it)\n"
          "  --env-mixture: each such ray drawn either by the sky's luminance or as the bounce sampling draws it, half and half, weighed by the\n"
          "                 balance heuristic (JADE_ENV_MIXTURE; NOT the reference's samples; excludes --env-importance; the oracle backend refuses it)\n"
          "  --reference-walk: every hitBVH query walks what the reference walks (nodes_visited / tris_tested equal the oracle's);\n"
          "                    default: shadow / environment-visibility walks end at the hit that settles them - the same image, bit for bit\n"
          "  NAME: tiny, tinyjade, C1, C2, C3, C4, C5 (SURVEY.md section 8d); C3G = C3 with a DIR_REFRACT glass statue\n");
}

int main(int argc, char** argv) {
  std::string config, args_file, out = "RenderResultHip.bmp", backend, env;
  int width = 0, height = 0, spp = 0, device = 0;
  bool reference_walk = false;
  bool env_importance = false, env_mixture = false;
  double adaptive = 0.0, error_floor = 0.01;
  int min_spp = 16;
  bool use_adaptive = false;
  bool use_denoise = false;
  std::string guides;
  bool use_exposure = false, auto_exposure = false, have_key = false, have_window = false;
  double exposure_ev = 0.0, key = 0.18, win_lo = 0.05, win_hi = 0.95;
  std::string histogram;
  bool use_glare = false, have_glare_levels = false, have_glare_falloff = false;
  double glare_strength = 0.0, glare_levels = 6, glare_falloff = 0.5;
  bool use_despeckle = false, have_despeckle_option = false;
  double ds_sigmas = 2.0, ds_gain = 2.0, ds_rank = 2, ds_radius = 1, ds_iterations = 1;
  std::string despeckle_map;
  bool use_aperture = false, have_focus = false, have_focus_at = false;
  double aperture = 0.0, focus = 0.0, focus_px = 0, focus_py = 0;
  bool one_light = false;
  int bounce = -1;  // --bounce: JADE_BOUNCE_*, -1 = not given
  int direct = -1;  // --direct: JADE_DIRECT_*, -1 = not given
  int branch = -1;  // --branch: JADE_BRANCH_*, -1 = not given
  std::string passes;  // --passes PREFIX
  double smooth_deg = 0.0;  // --smooth [DEG]: the objects' smoothing angle, 0 = not given
  struct TextureFlag { int object; std::string image; UvProjection projection; };
  std::vector<TextureFlag> texture_flags;  // --texture K=IMAGE[@PROJECTION]
  struct MapFlag { int object; std::string image; UvProjection projection; float strength; };
  std::vector<MapFlag> map_flags;          // --normal-map K=FILE|bumps[:SIZE[:N]][@PROJECTION][:STRENGTH]
  bool have_truck = false, have_orbit = false, have_pivot = false, have_interval = false;
  double truck[3] = {0, 0, 0}, orbit_deg = 0.0, pivot[3] = {0, 0, 0}, interval[2] = {0.0, 1.0};
  auto number = [](const char* flag, const char* v) {
    char* end = nullptr;
    const double x = strtod(v, &end);
    if (end == v || *end != 0 || !std::isfinite(x)) { fprintf(stderr, "%s: not a finite number: %s\n", flag, v); exit(2); }
    return x;
  };
  // n finite numbers separated by commas
  auto numbers = [&](const char* flag, const char* v, double* out, int n) {
    std::string rest = v;
    for (int k = 0; k < n; ++k) {
      const size_t comma = rest.find(',');
      if ((comma == std::string::npos) != (k == n - 1)) { fprintf(stderr, "%s: expected %d numbers separated by commas: %s\n", flag, n, v); return false; }
      out[k] = number(flag, rest.substr(0, comma).c_str());
      if (k < n - 1) rest = rest.substr(comma + 1);
    }
    return true;
  };
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto need = [&](const char* what) -> const char* {
      if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", what); exit(2); }
      return argv[++i];
    };
    if (a == "--config") config = need("--config");
    else if (a == "--args") args_file = need("--args");
    else if (a == "--width") width = atoi(need("--width"));
    else if (a == "--height") height = atoi(need("--height"));
    else if (a == "--spp") spp = atoi(need("--spp"));
    else if (a == "--out") out = need("--out");
    else if (a == "--env") env = need("--env");
    else if (a == "--backend") backend = need("--backend");
    else if (a == "--device") device = atoi(need("--device"));
    else if (a == "--reference-walk") reference_walk = true;
    else if (a == "--env-importance") env_importance = true;
    else if (a == "--env-mixture") env_mixture = true;
    else if (a == "--one-light") one_light = true;
    else if (a == "--bounce") {
      const std::string v = need("--bounce");
      if (v == "uniform") bounce = JADE_BOUNCE_UNIFORM;
      else if (v == "cosine") bounce = JADE_BOUNCE_COSINE;
      else { fprintf(stderr, "--bounce takes uniform or cosine, not %s\n", v.c_str()); return 2; }
    }
    else if (a == "--branch") {
      const std::string v = need("--branch");
      if (v == "random") branch = JADE_BRANCH_RANDOM;
      else if (v == "stratified") branch = JADE_BRANCH_STRATIFIED;
      else { fprintf(stderr, "--branch takes random or stratified, not %s\n", v.c_str()); return 2; }
    }
    else if (a == "--passes") passes = need("--passes");
    else if (a == "--texture") {
      const std::string v = need("--texture");
      const size_t eq = v.find('='), at = v.rfind('@');
      char* end = nullptr;
      const long k = strtol(v.c_str(), &end, 10);
      if (eq == std::string::npos || eq == 0 || end != v.c_str() + eq || k < 0 || k > 1000000 || eq + 1 >= (at == std::string::npos ? v.size() : at)) {
        fprintf(stderr, "--texture takes K=IMAGE[@PROJECTION] with K an object number from 0, not %s\n", v.c_str());
        return 2;
      }
      UvProjection proj = UV_SPHERICAL;
      if (at != std::string::npos) {
        const std::string pn = v.substr(at + 1);
        if (pn == "spherical") proj = UV_SPHERICAL;
        else if (pn == "planar-x") proj = UV_PLANAR_X;
        else if (pn == "planar-y") proj = UV_PLANAR_Y;
        else if (pn == "planar-z") proj = UV_PLANAR_Z;
        else { fprintf(stderr, "--texture: the projection is spherical, planar-x, planar-y or planar-z, not %s\n", pn.c_str()); return 2; }
      }
      for (const TextureFlag& t : texture_flags)
        if (t.object == (int)k) { fprintf(stderr, "--texture: object %ld is given twice\n", k); return 2; }
      texture_flags.push_back({(int)k, v.substr(eq + 1, (at == std::string::npos ? v.size() : at) - eq - 1), proj});
    }
    else if (a == "--normal-map") {
      // K=IMAGE[@PROJECTION][:STRENGTH]: a tangent-space normal map on object K - a P6 file (read linearly, 2 c - 1) or a PF file, or
      // bumps[:SIZE[:N]], a lattice of N x N bumps on SIZE x SIZE texels.  Without @PROJECTION a strength follows the image as :STRENGTH
      // (after bumps: as its third number).
      const std::string v = need("--normal-map");
      const size_t eq = v.find('='), at = v.rfind('@');
      char* end = nullptr;
      const long k = strtol(v.c_str(), &end, 10);
      if (eq == std::string::npos || eq == 0 || end != v.c_str() + eq || k < 0 || k > 1000000 || eq + 1 >= (at == std::string::npos ? v.size() : at)) {
        fprintf(stderr, "--normal-map takes K=IMAGE[@PROJECTION][:STRENGTH] with K an object number from 0, not %s\n", v.c_str());
        return 2;
      }
      std::string image = v.substr(eq + 1, (at == std::string::npos ? v.size() : at) - eq - 1), tail;
      UvProjection proj = UV_SPHERICAL;
      if (at != std::string::npos) {
        std::string pn = v.substr(at + 1);
        const size_t colon = pn.find(':');
        if (colon != std::string::npos) {
          tail = pn.substr(colon + 1);
          pn = pn.substr(0, colon);
        }
        if (pn == "spherical") proj = UV_SPHERICAL;
        else if (pn == "planar-x") proj = UV_PLANAR_X;
        else if (pn == "planar-y") proj = UV_PLANAR_Y;
        else if (pn == "planar-z") proj = UV_PLANAR_Z;
        else { fprintf(stderr, "--normal-map: the projection is spherical, planar-x, planar-y or planar-z, not %s\n", pn.c_str()); return 2; }
      } else {
        const bool bumps = image.compare(0, 5, "bumps") == 0 && (image.size() == 5 || image[5] == ':');
        size_t colons = 0, last = std::string::npos;
        for (size_t c = 0; c < image.size(); ++c)
          if (image[c] == ':') { ++colons; last = c; }
        if (last != std::string::npos && (bumps ? colons == 3 : true)) {
          char* e2 = nullptr;
          (void)strtod(image.c_str() + last + 1, &e2);
          if (e2 != image.c_str() + last + 1 && *e2 == 0) {
            tail = image.substr(last + 1);
            image = image.substr(0, last);
          }
        }
      }
      float strength = 1.0f;
      if (!tail.empty()) {
        char* e3 = nullptr;
        const double s = strtod(tail.c_str(), &e3);
        if (e3 == tail.c_str() || *e3 != 0 || !(s >= 0.0) || !std::isfinite(s)) { fprintf(stderr, "--normal-map: the strength is a number >= 0, not %s\n", tail.c_str()); return 2; }
        strength = (float)s;
      }
      for (const MapFlag& t : map_flags)
        if (t.object == (int)k) { fprintf(stderr, "--normal-map: object %ld is given twice\n", k); return 2; }
      map_flags.push_back({(int)k, image, proj, strength});
    }
    else if (a == "--smooth") {  // the angle is optional: taken if the next argument is a number
      smooth_deg = 60.0;
      if (i + 1 < argc) {
        char* end = nullptr;
        const double v = strtod(argv[i + 1], &end);
        if (end != argv[i + 1] && *end == 0) {
          ++i;
          if (!std::isfinite(v) || !(v > 0.0 && v <= 180.0)) { fprintf(stderr, "--smooth takes an angle in (0, 180] degrees, not %s\n", argv[i]); return 2; }
          smooth_deg = v;
        }
      }
    }
    else if (a == "--direct") {
      const std::string v = need("--direct");
      if (v == "rays") direct = JADE_DIRECT_RAYS;
      else if (v == "mis") direct = JADE_DIRECT_MIS;
      else { fprintf(stderr, "--direct takes rays or mis, not %s\n", v.c_str()); return 2; }
    }
    else if (a == "--adaptive") { adaptive = number("--adaptive", need("--adaptive")); use_adaptive = true; }
    else if (a == "--min-spp") { const double v = number("--min-spp", need("--min-spp")); min_spp = v >= 0 && v <= (1 << 30) && v == (int)v ? (int)v : -1; }
    else if (a == "--error-floor") error_floor = number("--error-floor", need("--error-floor"));
    else if (a == "--denoise") use_denoise = true;
    else if (a == "--guides") guides = need("--guides");
    else if (a == "--exposure") {
      const char* v = need("--exposure");
      use_exposure = true;
      auto_exposure = strcmp(v, "auto") == 0;
      if (!auto_exposure) exposure_ev = number("--exposure", v);
    }
    else if (a == "--key") { key = number("--key", need("--key")); have_key = true; }
    else if (a == "--exposure-window") {
      const std::string v = need("--exposure-window");
      const size_t comma = v.find(',');
      if (comma == std::string::npos) { fprintf(stderr, "--exposure-window: expected LO,HI: %s\n", v.c_str()); return 2; }
      win_lo = number("--exposure-window", v.substr(0, comma).c_str());
      win_hi = number("--exposure-window", v.substr(comma + 1).c_str());
      have_window = true;
    }
    else if (a == "--histogram") histogram = need("--histogram");
    else if (a == "--despeckle") use_despeckle = true;
    else if (a == "--despeckle-sigmas") { ds_sigmas = number("--despeckle-sigmas", need("--despeckle-sigmas")); have_despeckle_option = true; }
    else if (a == "--despeckle-gain") { ds_gain = number("--despeckle-gain", need("--despeckle-gain")); have_despeckle_option = true; }
    else if (a == "--despeckle-rank") { ds_rank = number("--despeckle-rank", need("--despeckle-rank")); have_despeckle_option = true; }
    else if (a == "--despeckle-radius") { ds_radius = number("--despeckle-radius", need("--despeckle-radius")); have_despeckle_option = true; }
    else if (a == "--despeckle-iterations") { ds_iterations = number("--despeckle-iterations", need("--despeckle-iterations")); have_despeckle_option = true; }
    else if (a == "--despeckle-map") { despeckle_map = need("--despeckle-map"); have_despeckle_option = true; }
    else if (a == "--glare") { glare_strength = number("--glare", need("--glare")); use_glare = true; }
    else if (a == "--glare-levels") { glare_levels = number("--glare-levels", need("--glare-levels")); have_glare_levels = true; }
    else if (a == "--glare-falloff") { glare_falloff = number("--glare-falloff", need("--glare-falloff")); have_glare_falloff = true; }
    else if (a == "--aperture") { aperture = number("--aperture", need("--aperture")); use_aperture = true; }
    else if (a == "--focus") { focus = number("--focus", need("--focus")); have_focus = true; }
    else if (a == "--focus-at") {
      const std::string v = need("--focus-at");
      const size_t comma = v.find(',');
      if (comma == std::string::npos) { fprintf(stderr, "--focus-at: expected PX,PY: %s\n", v.c_str()); return 2; }
      focus_px = number("--focus-at", v.substr(0, comma).c_str());
      focus_py = number("--focus-at", v.substr(comma + 1).c_str());
      have_focus_at = true;
    }
    else if (a == "--shutter-truck") { if (!numbers("--shutter-truck", need("--shutter-truck"), truck, 3)) return 2; have_truck = true; }
    else if (a == "--shutter-orbit") { orbit_deg = number("--shutter-orbit", need("--shutter-orbit")); have_orbit = true; }
    else if (a == "--shutter-pivot") { if (!numbers("--shutter-pivot", need("--shutter-pivot"), pivot, 3)) return 2; have_pivot = true; }
    else if (a == "--shutter-interval") { if (!numbers("--shutter-interval", need("--shutter-interval"), interval, 2)) return 2; have_interval = true; }
    else { usage(); return 2; }
  }
  // bad values end here, before a scene is built or a backend loaded
  if (env_importance && env_mixture) { fprintf(stderr, "--env-importance and --env-mixture exclude each other: give one of them\n"); return 2; }
  if (use_adaptive && !(adaptive > 0.0)) { fprintf(stderr, "--adaptive must be > 0\n"); return 2; }
  if (min_spp < 2 || (min_spp & (min_spp - 1)) != 0) { fprintf(stderr, "--min-spp must be a power of two >= 2\n"); return 2; }
  if (!(error_floor > 0.0)) { fprintf(stderr, "--error-floor must be > 0\n"); return 2; }
  if (use_exposure && !auto_exposure && !(std::fabs(exposure_ev) <= 64.0)) { fprintf(stderr, "--exposure must be auto or within -64 .. 64 stops\n"); return 2; }
  if ((have_key || have_window) && !auto_exposure) { fprintf(stderr, "--key and --exposure-window belong to --exposure auto\n"); return 2; }
  if (!(key > 0.0) || !std::isfinite((float)key) || !((float)key > 0.0f)) { fprintf(stderr, "--key must be > 0\n"); return 2; }
  if (!(win_lo >= 0.0 && (float)win_lo < (float)win_hi && win_hi <= 1.0)) { fprintf(stderr, "--exposure-window needs 0 <= LO < HI <= 1\n"); return 2; }
  if ((have_glare_levels || have_glare_falloff) && !use_glare) { fprintf(stderr, "--glare-levels and --glare-falloff belong to --glare\n"); return 2; }
  if (have_despeckle_option && !use_despeckle) { fprintf(stderr, "--despeckle-sigmas, -gain, -rank, -radius, -iterations and -map belong to --despeckle\n"); return 2; }
  if (!((float)ds_sigmas >= 0.0f) || !std::isfinite((float)ds_sigmas)) { fprintf(stderr, "--despeckle-sigmas must be >= 0\n"); return 2; }
  if (!((float)ds_gain >= 1.0f) || !std::isfinite((float)ds_gain)) { fprintf(stderr, "--despeckle-gain must be >= 1\n"); return 2; }
  if (!(ds_rank >= 1 && ds_rank <= 4 && ds_rank == (int)ds_rank)) { fprintf(stderr, "--despeckle-rank must be a whole number 1 .. 4\n"); return 2; }
  if (!(ds_radius >= 1 && ds_radius <= 3 && ds_radius == (int)ds_radius)) { fprintf(stderr, "--despeckle-radius must be a whole number 1 .. 3\n"); return 2; }
  if (!(ds_iterations >= 0 && ds_iterations <= 4 && ds_iterations == (int)ds_iterations)) { fprintf(stderr, "--despeckle-iterations must be a whole number 0 .. 4\n"); return 2; }
  if (!(glare_strength >= 0.0 && glare_strength <= 1.0)) { fprintf(stderr, "--glare must be within 0 .. 1\n"); return 2; }
  if (!(glare_levels >= 1 && glare_levels <= 12 && glare_levels == (int)glare_levels)) { fprintf(stderr, "--glare-levels must be a whole number 1 .. 12\n"); return 2; }
  if (!((float)glare_falloff > 0.0f) || !std::isfinite((float)glare_falloff)) { fprintf(stderr, "--glare-falloff must be > 0\n"); return 2; }
  if ((have_focus || have_focus_at) && !use_aperture) { fprintf(stderr, "--focus and --focus-at belong to --aperture\n"); return 2; }
  if (use_aperture && have_focus == have_focus_at) { fprintf(stderr, "--aperture needs exactly one of --focus D and --focus-at PX,PY\n"); return 2; }
  if (use_aperture && (!(aperture >= 0.0) || !std::isfinite((float)aperture))) { fprintf(stderr, "--aperture must be >= 0\n"); return 2; }
  if (have_focus && (!((float)focus > 0.0f) || !std::isfinite((float)focus))) { fprintf(stderr, "--focus must be > 0\n"); return 2; }
  if (have_focus_at && !(focus_px >= 0 && focus_py >= 0 && focus_px <= (1 << 30) && focus_py <= (1 << 30) && focus_px == (int)focus_px && focus_py == (int)focus_py)) {
    fprintf(stderr, "--focus-at needs two whole numbers PX,PY >= 0\n");
    return 2;
  }
  const bool use_shutter = have_truck || have_orbit;
  if ((have_pivot && !have_orbit) || (have_interval && !use_shutter)) {
    fprintf(stderr, "--shutter-pivot belongs to --shutter-orbit, --shutter-interval to --shutter-truck or --shutter-orbit\n");
    return 2;
  }
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite((float)truck[i]) || !std::isfinite((float)pivot[i])) { fprintf(stderr, "--shutter-truck and --shutter-pivot must be finite\n"); return 2; }
  if (!std::isfinite((float)orbit_deg)) { fprintf(stderr, "--shutter-orbit must be finite\n"); return 2; }
  if (!((float)interval[0] >= 0.0f && (float)interval[0] <= (float)interval[1] && (float)interval[1] <= 1.0f)) {
    fprintf(stderr, "--shutter-interval needs 0 <= T0 <= T1 <= 1\n");
    return 2;
  }
  if (config.empty() == args_file.empty()) { usage(); return 2; }
  if (backend.empty()) {
    char self[4096];
    ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
    self[n > 0 ? n : 0] = 0;
    backend = std::string(dirname(self)) + "/libjade_hip.so";
  }

  SceneBuilder builder;
  builder.set_smoothing((float)smooth_deg);  // (0: flat) - every object of the configuration or of render_args
  Config cfg;
  std::string err;
  for (const TextureFlag& t : texture_flags) {
    Texture tex;
    if (t.image.compare(0, 7, "checker") == 0 && (t.image.size() == 7 || t.image[7] == ':')) {
      int size = 256, squares = 8;
      if (t.image.size() > 7 && (sscanf(t.image.c_str() + 8, "%d:%d", &size, &squares) < 1 || size < 1 || size > 16384 || squares < 1 || squares > size)) {
        fprintf(stderr, "--texture: checker[:SIZE[:SQUARES]] takes 1 .. 16384 texels a side and at most as many squares, not %s\n", t.image.c_str());
        return 2;
      }
      const float light[3] = {0.9f, 0.9f, 0.9f}, dark[3] = {0.15f, 0.15f, 0.15f};
      tex = make_texture_checker(size, squares, light, dark);
    } else if (!(t.image.size() > 4 && t.image.compare(t.image.size() - 4, 4, ".pfm") == 0 ? load_pfm(t.image, tex, err) : load_ppm(t.image, tex, err))) {
      fprintf(stderr, "--texture: %s\n", err.c_str());
      return 1;
    }
    builder.set_object_texture(t.object, tex, t.projection);
  }
  for (const MapFlag& t : map_flags) {
    Texture map;
    if (t.image.compare(0, 5, "bumps") == 0 && (t.image.size() == 5 || t.image[5] == ':')) {
      int size = 256, n = 8;
      if (t.image.size() > 5 && (sscanf(t.image.c_str() + 6, "%d:%d", &size, &n) < 1 || size < 1 || size > 16384 || n < 1 || 2 * n > size)) {
        fprintf(stderr, "--normal-map: bumps[:SIZE[:N]] takes 1 .. 16384 texels a side and at most half as many bumps, not %s\n", t.image.c_str());
        return 2;
      }
      // a lattice of n x n bumps: height = (0.08 / n) sin(2 pi n u) sin(2 pi n v), so that the steepest slope is 0.5 whatever n is
      std::vector<float> height((size_t)size * size);
      for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x)
          height[(size_t)y * size + x] = (float)(0.08 / n * std::sin(2.0 * M_PI * n * (x + 0.5) / size) * std::sin(2.0 * M_PI * n * (y + 0.5) / size));
      map = height_to_normal_map(height.data(), size, size, 1.0f);
    } else if (!load_normal_map(t.image, map, err)) {
      fprintf(stderr, "--normal-map: %s\n", err.c_str());
      return 1;
    }
    builder.set_object_normal_map(t.object, map, t.projection, t.strength);
  }
  if (!config.empty()) {
    if (!make_config(config, builder, cfg, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  } else {
    RenderArgs ra;
    if (!read_render_args(args_file, ra, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    std::string dir = args_file;
    size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
    for (const RenderArgsObject& o : ra.objects) {
      Mesh m;
      std::string f = (!o.file.empty() && o.file[0] == '/') ? o.file : dir + o.file;
      // (a textured object is read with its vt lines; every other one as the reference reads it)
      if (!(builder.object_texture_set(builder.object_count()) || builder.object_normal_map_set(builder.object_count()) ? load_obj_textured(f, m, err) : load_obj(f, m, err))) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
      builder.add_mesh(m, o.material, o.trans, o.normalize);
    }
    memcpy(cfg.eye, ra.eye, sizeof cfg.eye);
    memcpy(cfg.camera, ra.camera, sizeof cfg.camera);
    cfg.width = cfg.height = 1024;  // the reference's -DLARGE size, PathTrace.cu:25-26
    cfg.spp = 64;
    if (env.empty()) env = "sky";
  }
  for (const TextureFlag& t : texture_flags)
    if (t.object >= builder.object_count()) {
      fprintf(stderr, "--texture: the scene has objects 0 .. %d, not %d\n", builder.object_count() - 1, t.object);
      return 2;
    }
  for (const MapFlag& t : map_flags)
    if (t.object >= builder.object_count()) {
      fprintf(stderr, "--normal-map: the scene has objects 0 .. %d, not %d\n", builder.object_count() - 1, t.object);
      return 2;
    }
  if (env == "sky") builder.set_env(make_env_sky(1024, 512));
  else if (!env.empty()) {
    EnvMap e;
    if (!load_hdr(env, e, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    builder.set_env(std::move(e));
  }
  if (width > 0) cfg.width = width;
  if (height > 0) cfg.height = height;
  if (spp > 0) cfg.spp = spp;
  if (have_focus_at && (focus_px >= cfg.width || focus_py >= cfg.height)) {
    fprintf(stderr, "--focus-at %d,%d lies outside the %d x %d frame\n", (int)focus_px, (int)focus_py, cfg.width, cfg.height);
    return 2;
  }
  if (use_adaptive && min_spp > cfg.spp) { fprintf(stderr, "--min-spp %d is above the cap --spp %d\n", min_spp, cfg.spp); return 2; }

  printf("Model load done:  %d Triangles.\n", builder.triangle_count());
  BuiltScene scene = builder.build(8);
  printf("BVH Build done: %zu nodes, depth %d, %.2f s.\n", scene.nodes.size(), scene.bvh_depth, scene.build_seconds);

  Api api;
  if (!load_api(backend, api, use_adaptive)) return 1;
  if (use_denoise || !guides.empty()) {
    *(void**)(&api.denoise_defaults) = dlsym(api.h, "jade_denoise_defaults");
    *(void**)(&api.render_denoise) = dlsym(api.h, "jade_render_denoise");
    *(void**)(&api.render_guides) = dlsym(api.h, "jade_render_guides");
    if (!api.denoise_defaults || !api.render_denoise || !api.render_guides) {
      fprintf(stderr, "%s needs the HIP backend: %s has no jade_render_denoise / jade_render_guides\n", use_denoise ? "--denoise" : "--guides",
              backend.c_str());
      return 2;
    }
  }
  if (use_despeckle) {
    *(void**)(&api.despeckle_defaults) = dlsym(api.h, "jade_despeckle_defaults");
    *(void**)(&api.render_despeckle) = dlsym(api.h, "jade_render_despeckle");
    if (!api.despeckle_defaults || !api.render_despeckle) {
      fprintf(stderr, "--despeckle needs the HIP backend: %s has no jade_render_despeckle\n", backend.c_str());
      return 2;
    }
  }
  if (use_glare) {
    *(void**)(&api.glare_defaults) = dlsym(api.h, "jade_glare_defaults");
    *(void**)(&api.glare_image) = dlsym(api.h, "jade_glare_image");
    *(void**)(&api.render_glare) = dlsym(api.h, "jade_render_glare");
    if (!api.glare_defaults || !api.glare_image || !api.render_glare) {
      fprintf(stderr, "--glare needs the HIP backend: %s has no jade_render_glare / jade_glare_image\n", backend.c_str());
      return 2;
    }
  }
  if (use_aperture) {
    *(void**)(&api.scene_set_lens) = dlsym(api.h, "jade_scene_set_lens");
    *(void**)(&api.trace_rays) = dlsym(api.h, "jade_trace_rays");
    if (!api.scene_set_lens || !api.trace_rays) {
      fprintf(stderr, "--aperture needs the HIP backend: %s has no jade_scene_set_lens\n", backend.c_str());
      return 2;
    }
  }
  if (use_shutter) {
    *(void**)(&api.scene_set_shutter) = dlsym(api.h, "jade_scene_set_shutter");
    if (!api.scene_set_shutter) {
      fprintf(stderr, "--shutter-truck / --shutter-orbit need the HIP backend: %s has no jade_scene_set_shutter\n", backend.c_str());
      return 2;
    }
  }
  if (one_light) {
    *(void**)(&api.scene_set_light_sampling) = dlsym(api.h, "jade_scene_set_light_sampling");
    if (!api.scene_set_light_sampling) {
      fprintf(stderr, "--one-light needs the HIP backend: %s has no jade_scene_set_light_sampling\n", backend.c_str());
      return 2;
    }
  }
  if (bounce >= 0) {
    *(void**)(&api.scene_set_bounce_sampling) = dlsym(api.h, "jade_scene_set_bounce_sampling");
    if (!api.scene_set_bounce_sampling) {
      fprintf(stderr, "--bounce needs the HIP backend: %s has no jade_scene_set_bounce_sampling\n", backend.c_str());
      return 2;
    }
  }
  if (direct == JADE_DIRECT_MIS && bounce != JADE_BOUNCE_COSINE) {
    fprintf(stderr, "--direct mis weighs the emitter rays against the cosine bounce: it needs --bounce cosine\n");
    return 2;
  }
  if (direct >= 0) {
    *(void**)(&api.scene_set_direct_sampling) = dlsym(api.h, "jade_scene_set_direct_sampling");
    if (!api.scene_set_direct_sampling) {
      fprintf(stderr, "--direct needs the HIP backend: %s has no jade_scene_set_direct_sampling\n", backend.c_str());
      return 2;
    }
  }
  if (branch >= 0) {
    *(void**)(&api.scene_set_branch_sampling) = dlsym(api.h, "jade_scene_set_branch_sampling");
    if (!api.scene_set_branch_sampling) {
      fprintf(stderr, "--branch needs the HIP backend: %s has no jade_scene_set_branch_sampling\n", backend.c_str());
      return 2;
    }
  }
  if (smooth_deg > 0.0) {
    *(void**)(&api.scene_set_vertex_normals) = dlsym(api.h, "jade_scene_set_vertex_normals");
    if (!api.scene_set_vertex_normals) {
      fprintf(stderr, "--smooth needs the HIP backend: %s has no jade_scene_set_vertex_normals\n", backend.c_str());
      return 2;
    }
  }
  if (!texture_flags.empty()) {
    *(void**)(&api.scene_set_textures) = dlsym(api.h, "jade_scene_set_textures");
    if (!api.scene_set_textures) {
      fprintf(stderr, "--texture needs the HIP backend: %s has no jade_scene_set_textures\n", backend.c_str());
      return 2;
    }
  }
  if (!map_flags.empty()) {
    *(void**)(&api.scene_set_normal_maps) = dlsym(api.h, "jade_scene_set_normal_maps");
    if (!api.scene_set_normal_maps) {
      fprintf(stderr, "--normal-map needs the HIP backend: %s has no jade_scene_set_normal_maps\n", backend.c_str());
      return 2;
    }
  }
  if (!passes.empty()) {
    *(void**)(&api.scene_set_passes) = dlsym(api.h, "jade_scene_set_passes");
    *(void**)(&api.render_passes) = dlsym(api.h, "jade_render_passes");
    *(void**)(&api.pass_name) = dlsym(api.h, "jade_pass_name");
    if (!api.scene_set_passes || !api.render_passes || !api.pass_name) {
      fprintf(stderr, "--passes needs the HIP backend: %s has no jade_scene_set_passes\n", backend.c_str());
      return 2;
    }
  }
  // (a denoised or despeckled frame is on the host when the glare comes: it gets its bytes from jade_expose_image even without --exposure)
  const bool host_frame = use_denoise || use_despeckle;
  const bool need_display = use_exposure || !histogram.empty() || (use_glare && host_frame);
  if (need_display) {
    *(void**)(&api.display_defaults) = dlsym(api.h, "jade_display_defaults");
    *(void**)(&api.render_resolve_exposed) = dlsym(api.h, "jade_render_resolve_exposed");
    *(void**)(&api.expose_image) = dlsym(api.h, "jade_expose_image");
    if (!api.display_defaults || !api.render_resolve_exposed || !api.expose_image) {
      fprintf(stderr, "%s needs the HIP backend: %s has no jade_render_resolve_exposed / jade_expose_image\n",
              use_exposure ? "--exposure" : !histogram.empty() ? "--histogram" : "--glare with --denoise / --despeckle", backend.c_str());
      return 2;
    }
  }
  jade_scene_desc desc = scene.desc();
  jade_scene* dev = nullptr;
  if (api.scene_create(&desc, device, &dev) != JADE_OK) { fprintf(stderr, "scene: %s\n", api.last_error()); return 1; }
  jade_render_params rp;
  memset(&rp, 0, sizeof rp);
  rp.width = cfg.width; rp.height = cfg.height; rp.spp = cfg.spp;
  memcpy(rp.eye, cfg.eye, sizeof rp.eye);
  memcpy(rp.camera, cfg.camera, sizeof rp.camera);
  rp.tile_nranks = 1;
  rp.device_id = device;
  rp.walk = reference_walk ? JADE_WALK_REFERENCE : JADE_WALK_EARLY_EXIT;
  rp.env_sampling = env_mixture ? JADE_ENV_MIXTURE : env_importance ? JADE_ENV_IMPORTANCE : JADE_ENV_REFERENCE;  // (non-parity: another estimator of the same image; HIP backend only)
  if (use_aperture) {
    jade_lens_params lens;
    lens.aperture_radius = (float)aperture;
    lens.focus_distance = (float)focus;
    if (have_focus_at) {
      if (jadeh_focus_distance(api.trace_rays, dev, &rp, (int)focus_px, (int)focus_py, &lens.focus_distance) != 0) {
        fprintf(stderr, "--focus-at: %s\n", jadeh_last_error());
        return 1;
      }
      printf("focus: pixel (%d, %d) is %.9g away along the axis\n", (int)focus_px, (int)focus_py, lens.focus_distance);
    }
    if (api.scene_set_lens(dev, &lens) != JADE_OK) { fprintf(stderr, "lens: %s\n", api.last_error()); return 1; }
    printf("lens: aperture radius %.9g, focus distance %.9g\n", lens.aperture_radius, lens.focus_distance);
  }
  if (use_shutter) {
    jade_shutter_params sh;
    const float truck_f[3] = {(float)truck[0], (float)truck[1], (float)truck[2]}, pivot_f[3] = {(float)pivot[0], (float)pivot[1], (float)pivot[2]};
    if (jadeh_camera_move(rp.eye, rp.camera, truck_f, (float)orbit_deg, have_pivot ? pivot_f : nullptr, sh.eye_close, sh.camera_close) != 0) {
      fprintf(stderr, "shutter: %s\n", jadeh_last_error());
      return 1;
    }
    sh.t_open = (float)interval[0];
    sh.t_close = (float)interval[1];
    if (api.scene_set_shutter(dev, &sh) != JADE_OK) { fprintf(stderr, "shutter: %s\n", api.last_error()); return 1; }
    printf("shutter: closes at eye (%.9g, %.9g, %.9g), exposure %.9g .. %.9g of the move\n", sh.eye_close[0], sh.eye_close[1], sh.eye_close[2], sh.t_open,
           sh.t_close);
  }
  if (one_light && api.scene_set_light_sampling(dev, JADE_LIGHTS_ONE) != JADE_OK) { fprintf(stderr, "light sampling: %s\n", api.last_error()); return 1; }
  if (bounce >= 0 && api.scene_set_bounce_sampling(dev, bounce) != JADE_OK) { fprintf(stderr, "bounce sampling: %s\n", api.last_error()); return 1; }
  if (direct >= 0 && api.scene_set_direct_sampling(dev, direct) != JADE_OK) { fprintf(stderr, "direct sampling: %s\n", api.last_error()); return 1; }
  if (branch >= 0 && api.scene_set_branch_sampling(dev, branch) != JADE_OK) { fprintf(stderr, "branch sampling: %s\n", api.last_error()); return 1; }
  if (smooth_deg > 0.0 && !scene.vertex_normals.empty() &&
      api.scene_set_vertex_normals(dev, scene.vertex_normals.data(), (int32_t)(scene.vertex_normals.size() / 9)) != JADE_OK) {
    fprintf(stderr, "vertex normals: %s\n", api.last_error());
    return 1;
  }
  if (!scene.textures.empty()) {
    std::vector<jade_texture_image> images;
    for (const Texture& t : scene.textures) images.push_back({t.width, t.height, t.rgb.data()});
    if (api.scene_set_textures(dev, (int32_t)images.size(), images.data(), scene.uv.data(), scene.image_of.data(), (int32_t)scene.image_of.size()) != JADE_OK) {
      fprintf(stderr, "textures: %s\n", api.last_error());
      return 1;
    }
  }
  if (!scene.normal_maps.empty()) {
    std::vector<jade_texture_image> images;
    for (const Texture& t : scene.normal_maps) images.push_back({t.width, t.height, t.rgb.data()});
    if (api.scene_set_normal_maps(dev, (int32_t)images.size(), images.data(), scene.map_uv.data(), scene.map_image_of.data(), (int32_t)scene.map_image_of.size(), scene.map_strength) != JADE_OK) {
      fprintf(stderr, "normal maps: %s\n", api.last_error());
      return 1;
    }
  }
  if (!passes.empty() && api.scene_set_passes(dev, 1) != JADE_OK) { fprintf(stderr, "passes: %s\n", api.last_error()); return 1; }
  const std::string lights_note_s = std::string(one_light ? ", one light per vertex" : "") + (bounce == JADE_BOUNCE_COSINE ? ", cosine-weighted bounces" : "") +
                                    (direct == JADE_DIRECT_MIS ? ", emitters by multiple importance sampling" : "") +
                                    (env_mixture ? ", sky importance mixed with the hemisphere draw" : "") + (branch == JADE_BRANCH_STRATIFIED ? ", branch draws shared out" : "") + (smooth_deg > 0.0 ? ", smooth shading" : "") + (!texture_flags.empty() ? ", textures" : "") + (!map_flags.empty() ? ", normal maps" : "") + (!passes.empty() ? ", light passes kept" : "");
  const char* lights_note = lights_note_s.c_str();
  std::vector<float> rgb((size_t)3 * rp.width * rp.height);
  std::vector<uint8_t> bgr((size_t)3 * rp.width * rp.height);
  jade_stats st;
  memset(&st, 0, sizeof st);
  const int tiles = ((rp.width + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE) * ((rp.height + JADE_TILE_SIZE - 1) / JADE_TILE_SIZE);
  std::vector<int32_t> tile_spp(use_adaptive ? tiles : 0);
  if (use_adaptive) {
    printf("Start... %dx%d, adaptive %g (%d .. %d spp) on %s%s\n", rp.width, rp.height, adaptive, min_spp, rp.spp, api.backend_name(), lights_note);
    if (api.render_adaptive(dev, &rp, min_spp, (float)adaptive, (float)error_floor, rgb.data(), bgr.data(), tile_spp.data(), &st) != JADE_OK) {
      fprintf(stderr, "render: %s\n", api.last_error());
      return 1;
    }
  } else {
    printf("Start... %dx%d, %d spp on %s%s\n", rp.width, rp.height, rp.spp, api.backend_name(), lights_note);
    if (api.render(dev, &rp, rgb.data(), bgr.data(), &st) != JADE_OK) { fprintf(stderr, "render: %s\n", api.last_error()); return 1; }
  }
  if (!passes.empty()) {
    const size_t np = (size_t)rp.width * rp.height;
    std::vector<float> pv((size_t)JADE_PASS_COUNT * 3 * np);
    if (api.render_passes(dev, pv.data()) != JADE_OK) { fprintf(stderr, "passes: %s\n", api.last_error()); return 1; }
    for (int i = 0; i < JADE_PASS_COUNT; ++i) {
      const std::string path = passes + "." + api.pass_name(i) + ".pfm";
      if (!write_pfm(path, pv.data() + (size_t)i * 3 * np, rp.width, rp.height)) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
      printf("wrote %s\n", path.c_str());
    }
  }
  if (!guides.empty()) {
    const size_t np = (size_t)rp.width * rp.height;
    std::vector<float> ga(3 * np), gn(3 * np), gz(np), gv(np);
    if (api.render_guides(dev, 4, ga.data(), gn.data(), gz.data(), gv.data()) != JADE_OK) { fprintf(stderr, "guides: %s\n", api.last_error()); return 1; }
    const std::pair<const char*, const std::vector<float>*> files[] = {{"albedo", &ga}, {"normal", &gn}, {"depth", &gz}, {"variance", &gv}};
    for (const auto& f : files) {
      const std::string path = guides + "_" + f.first + ".pfm";
      const bool ok = f.second->size() == 3 * np ? write_pfm(path, f.second->data(), rp.width, rp.height) : write_pfm1(path, f.second->data(), rp.width, rp.height);
      if (!ok) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
      printf("wrote %s\n", path.c_str());
    }
  }
  if (use_despeckle) {
    // resolve, the passes and - with --denoise - the filter on the despeckled colour and variance, all on the render's device
    jade_despeckle_params ds;
    api.despeckle_defaults(&ds);
    ds.sigmas = (float)ds_sigmas;
    ds.gain = (float)ds_gain;
    ds.rank = (int32_t)ds_rank;
    ds.radius = (int32_t)ds_radius;
    ds.iterations = (int32_t)ds_iterations;
    jade_denoise_params dn;
    if (use_denoise) api.denoise_defaults(&dn);
    jade_despeckle_report rep;
    memset(&rep, 0, sizeof rep);
    std::vector<float> scale(despeckle_map.empty() ? 0 : (size_t)rp.width * rp.height);
    if (api.render_despeckle(dev, &ds, use_denoise ? &dn : nullptr, JADE_TONEMAP_ACES, 0.0f, rgb.data(), bgr.data(),
                             scale.empty() ? nullptr : scale.data(), &rep) != JADE_OK) { fprintf(stderr, "despeckle: %s\n", api.last_error()); return 1; }
    fprintf(stderr, "despeckle: %llu usable pixels, %llu above, %llu established, %llu clamped\n", (unsigned long long)rep.n_usable,
            (unsigned long long)rep.n_above, (unsigned long long)rep.n_established, (unsigned long long)rep.n_clamped);
    printf("despeckled: %d passes, radius %d, rank %d, gain %.9g, sigmas %.9g\n", ds.iterations, ds.radius, ds.rank, ds.gain, ds.sigmas);
    if (use_denoise) printf("denoised: %d a-trous passes, %d guide samples\n", dn.iterations, dn.guide_spp);
    if (!despeckle_map.empty()) {
      if (!write_pfm1(despeckle_map, scale.data(), rp.width, rp.height)) { fprintf(stderr, "cannot write %s\n", despeckle_map.c_str()); return 1; }
      printf("wrote %s\n", despeckle_map.c_str());
    }
  } else if (use_denoise) {
    jade_denoise_params dp;
    api.denoise_defaults(&dp);
    if (api.render_denoise(dev, &dp, JADE_TONEMAP_ACES, 0.0f, rgb.data(), bgr.data()) != JADE_OK) { fprintf(stderr, "denoise: %s\n", api.last_error()); return 1; }
    printf("denoised: %d a-trous passes, %d guide samples\n", dp.iterations, dp.guide_spp);
  }
  jade_display_params dp;
  memset(&dp, 0, sizeof dp);
  if (need_display) {
    api.display_defaults(&dp);
    if (auto_exposure) {
      dp.exposure_mode = JADE_EXPOSURE_AUTO;
      dp.key = (float)key;
      dp.p_lo = (float)win_lo;
      dp.p_hi = (float)win_hi;
    } else {
      dp.exposure = (float)std::exp2(exposure_ev);
    }
  }
  bool bytes_exposed = false;  // jade_render_glare made the bytes under dp already
  if (use_glare) {
    jade_glare_params gp;
    api.glare_defaults(&gp);
    gp.strength = (float)glare_strength;
    gp.levels = (int32_t)glare_levels;
    gp.falloff = (float)glare_falloff;
    int rc;
    float e = 1.0f;
    if (host_frame) {
      // a denoised or despeckled frame is on the host by now; its bytes come from jade_expose_image below
      rc = api.glare_image(device, rp.width, rp.height, rgb.data(), &gp, rgb.data());
    } else if (!histogram.empty()) {
      // the histogram wants the meter, which only jade_expose_image hands back: the glared frame alone here, bytes and meter below
      rc = api.render_glare(dev, &gp, nullptr, rgb.data(), nullptr, nullptr);
    } else {
      // the whole chain on the render's device: glare, meter, exposure and tone pack, one copy back
      rc = api.render_glare(dev, &gp, use_exposure ? &dp : nullptr, rgb.data(), bgr.data(), &e);
      bytes_exposed = use_exposure;
    }
    if (rc != JADE_OK) { fprintf(stderr, "glare: %s\n", api.last_error()); return 1; }
    printf("glare: strength %.9g over %d levels, falloff %.9g\n", gp.strength, gp.levels, gp.falloff);
    if (bytes_exposed) printf("exposure: x%.9g (%+.3f EV%s)\n", e, std::log2((double)e), auto_exposure ? ", auto" : "");
  }
  if (need_display && !bytes_exposed) {
    // the bytes again, from exposure x frame; the linear frame (a .pfm output) stays as it is
    float e = 0.0f;
    jade_meter m;
    const int rc = host_frame || use_glare ? api.expose_image(device, rp.width, rp.height, rgb.data(), &dp, bgr.data(), &e, &m)
                               : api.render_resolve_exposed(dev, &dp, nullptr, bgr.data(), &e, &m);
    if (rc != JADE_OK) { fprintf(stderr, "exposure: %s\n", api.last_error()); return 1; }
    if (use_exposure || !histogram.empty())
      printf("exposure: x%.9g (%+.3f EV%s), luminance %.9g .. %.9g over %llu positive pixels\n", e, std::log2((double)e), auto_exposure ? ", auto" : "",
             m.lum_min, m.lum_max, (unsigned long long)m.n_positive);
    if (!histogram.empty()) {
      FILE* f = fopen(histogram.c_str(), "w");
      if (!f) { fprintf(stderr, "cannot write %s\n", histogram.c_str()); return 1; }
      for (int b = 0; b < JADE_METER_BINS; ++b)  // bin b starts at 2^E (1 + k/8), E = (b >> 3) - 32, k = b & 7
        fprintf(f, "%.17g %llu\n", std::ldexp(1.0 + (b & 7) / 8.0, (b >> 3) - 32), (unsigned long long)m.bins[b]);
      fprintf(f, "positive %llu\nzero %llu\nnegative %llu\nnonfinite %llu\nlum_min %.9g\nlum_max %.9g\n", (unsigned long long)m.n_positive,
              (unsigned long long)m.n_zero, (unsigned long long)m.n_negative, (unsigned long long)m.n_nonfinite, m.lum_min, m.lum_max);
      if (fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", histogram.c_str()); return 1; }
      printf("wrote %s\n", histogram.c_str());
    }
  }
  api.scene_destroy(dev);
  std::string hist;
  if (use_adaptive) {  // tiles per final sample count
    std::map<int32_t, int> h;
    for (int32_t k : tile_spp) h[k] += 1;
    for (const auto& kv : h) hist += (hist.empty() ? "" : ", ") + ("\"" + std::to_string(kv.first) + "\": " + std::to_string(kv.second));
    hist = ", \"tile_spp\": {" + hist + "}";
  }
  double rays = (double)(st.rays_primary + st.rays_secondary);
  printf("{\"rays\": %.0f, \"kernel_ms\": %.3f, \"mray_per_s\": %.3f, \"rays_primary\": %llu, \"rays_secondary\": %llu, "
         "\"nodes_visited\": %llu, \"tris_tested\": %llu, \"shaded_hits\": %llu, \"samples\": %llu%s}\n",
         rays, st.kernel_ms, rays / st.kernel_ms / 1e3, (unsigned long long)st.rays_primary, (unsigned long long)st.rays_secondary,
         (unsigned long long)st.nodes_visited, (unsigned long long)st.tris_tested, (unsigned long long)st.shaded_hits,
         (unsigned long long)st.samples, hist.c_str());
  bool ok;
  size_t dot = out.find_last_of('.');
  std::string ext = dot == std::string::npos ? "" : out.substr(dot);
  if (ext == ".pfm") ok = write_pfm(out, rgb.data(), rp.width, rp.height);
  else if (ext == ".ppm") ok = write_ppm(out, bgr.data(), rp.width, rp.height);
  else ok = write_bmp(out, bgr.data(), rp.width, rp.height);
  if (!ok) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
  printf("wrote %s\n", out.c_str());
  return 0;
}
