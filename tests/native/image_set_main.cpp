// image_set_main.cpp - surface_check_images (jade_surface.hip: the check jade_scene_set_textures and jade_scene_set_normal_maps share; host
// code, no HIP call) on the image sets at the edges of what it accepts, as a stand-alone program for AddressSanitizer + UBSan (make
// asan-check).  No Python, no device: built with hipcc --offload-host-only together with jade_surface.hip itself.
// Per case: the status and, where refused, a piece of the message; an accepted set's heads and texels are read back in full, so the
// sanitizer sees every element the check wrote.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "jade_runtime.h"

static std::string g_err;
int jade_fail(int code, const std::string& msg) {  // jade_runtime.h (jade_hip.hip's in the module)
  g_err = msg;
  return code;
}

namespace {

int g_bad = 0;

// runs the check under both prefixes; `want` is the status, `text` a piece of the refusal (after the prefix), `texels` the count accepted
void expect(const char* name, int32_t n_images, const jade_texture_image* images, const std::vector<int32_t>& image_of, int32_t n_scene, int want,
            const char* text, size_t texels = 0, bool any = false) {
  for (const char* who : {"textures: ", "normal maps: "}) {
    std::vector<uint4> heads;
    std::vector<float4> tx;
    bool got_any = !any;
    g_err.clear();
    const int rc = surface_check_images(who, n_images, images, image_of.data(), (int32_t)image_of.size(), n_scene, &heads, &tx, &got_any);
    bool ok = rc == want;
    if (want != JADE_OK) {
      ok = ok && g_err.rfind(who, 0) == 0 && g_err.find(text) != std::string::npos;
    } else {
      ok = ok && heads.size() == (size_t)n_images && tx.size() == texels && got_any == any;
      size_t next = 0;
      for (int32_t k = 0; ok && k < n_images; ++k) {
        ok = (((size_t)heads[k].y << 32) | heads[k].x) == next && (int32_t)heads[k].z == images[k].width && (int32_t)heads[k].w == images[k].height;
        for (size_t i = 0; ok && i < (size_t)images[k].width * images[k].height; ++i)
          ok = memcmp(&tx[next + i], images[k].rgb + 3 * i, 12) == 0 && tx[next + i].w == 0.0f;
        next += (size_t)images[k].width * images[k].height;
      }
    }
    if (!ok) {
      fprintf(stderr, "%s (%s): status %d, expected %d; message \"%s\"\n", name, who, rc, want, g_err.c_str());
      ++g_bad;
    }
  }
  printf("%-44s %s\n", name, want == JADE_OK ? "accepted" : g_err.c_str());
}

}  // namespace

int main() {
  std::vector<float> one(3, 0.5f), big(3 * 5 * 7);
  for (size_t i = 0; i < big.size(); ++i) big[i] = 0.25f + (float)i;
  const jade_texture_image img1{1, 1, one.data()};
  const jade_texture_image img57{5, 7, big.data()};
  const std::vector<int32_t> none(4, -1), first(4, 0);

  // zero images: nothing to name (the setters clear on it before they come here)
  expect("zero images, no triangle names one", 0, nullptr, none, 4, JADE_OK, "", 0, false);
  expect("zero images, a triangle names image 0", 0, nullptr, first, 4, JADE_ERR_INVALID, "image_of[0] = 0 is outside -1 .. -1");
  expect("a negative image count", -1, nullptr, none, 4, JADE_ERR_INVALID, "-1 images (at most");
  // one more than the count accepted: refused before any image is looked at
  expect("JADE_TEX_MAX_IMAGES + 1 images", JADE_TEX_MAX_IMAGES + 1, nullptr, none, 4, JADE_ERR_INVALID, "images (at most 65536)");
  {
    std::vector<jade_texture_image> many((size_t)JADE_TEX_MAX_IMAGES, img1);
    std::vector<int32_t> last(4, JADE_TEX_MAX_IMAGES - 1);
    expect("JADE_TEX_MAX_IMAGES images", JADE_TEX_MAX_IMAGES, many.data(), last, 4, JADE_OK, "", (size_t)JADE_TEX_MAX_IMAGES, true);
  }
  expect("a triangle count that is not the scene's", 1, &img1, none, 5, JADE_ERR_INVALID, "the triangle count 4 is not the scene's");
  // the sizes
  expect("a 1 x 1 image", 1, &img1, first, 4, JADE_OK, "", 1, true);
  {
    const jade_texture_image imgs[2] = {img57, img1};
    expect("a 5 x 7 image and a 1 x 1 image", 2, imgs, std::vector<int32_t>{1, -1, 0, 1}, 4, JADE_OK, "", 36, true);
    expect("two images no triangle names", 2, imgs, none, 4, JADE_OK, "", 36, false);
  }
  {
    const jade_texture_image wide{JADE_TEX_MAX_SIZE + 1, 1, one.data()}, tall{1, JADE_TEX_MAX_SIZE + 1, one.data()}, flat{4, 0, one.data()};
    expect("an image one texel too wide", 1, &wide, first, 4, JADE_ERR_INVALID, "image 0 is 16385 x 1 (a width and a height of 1 .. 16384)");
    expect("an image one texel too tall", 1, &tall, first, 4, JADE_ERR_INVALID, "image 0 is 1 x 16385 (a width and a height of 1 .. 16384)");
    expect("an image of height 0", 1, &flat, first, 4, JADE_ERR_INVALID, "image 0 is 4 x 0");
    const jade_texture_image imgs[2] = {img1, jade_texture_image{2, 2, nullptr}};
    expect("an image without texels", 2, imgs, first, 4, JADE_ERR_INVALID, "image 1 has no texels");
  }
  // image_of at either end of its range
  expect("image_of = -2", 1, &img1, std::vector<int32_t>{0, -1, -2, 0}, 4, JADE_ERR_INVALID, "image_of[2] = -2 is outside -1 .. 0");
  expect("image_of = n_images", 1, &img1, std::vector<int32_t>{0, -1, 0, 1}, 4, JADE_ERR_INVALID, "image_of[3] = 1 is outside -1 .. 0");
  // a texel that is not finite, in the last position of the last image
  for (const float v : {(float)NAN, (float)INFINITY, -(float)INFINITY}) {
    std::vector<float> spoilt(big);
    spoilt.back() = v;
    const jade_texture_image imgs[2] = {img1, jade_texture_image{5, 7, spoilt.data()}};
    expect("a texel that is not finite at the very end", 2, imgs, first, 4, JADE_ERR_INVALID, "image 1 has a texel that is not finite at (4, 6)");
  }
  if (g_bad) {
    fprintf(stderr, "image_set: %d cases failed\n", g_bad);
    return 1;
  }
  printf("image_set: clean\n");
  return 0;
}
