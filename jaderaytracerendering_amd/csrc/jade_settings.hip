// jade_settings.hip — the settings of a scene handle (include/jade_bvh.h): lens, shutter, light / bounce / direct / branch sampling, passes.
// Host code only, no kernel: each setter checks its argument and stores it; the next jade_render_begin reads it (shade_mode_for,
// jade_runtime.h) and a render in progress is not touched.
#include <cmath>

#include "jade_runtime.h"

// The thin lens of the scene handle (include/jade_bvh.h): checked here, read by the next jade_render_begin.
int jade_scene_set_lens(jade_scene* s, const jade_lens_params* lens) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (!lens) {
    s->lens = jade_lens_params{};
    return JADE_OK;
  }
  if (!std::isfinite(lens->aperture_radius) || !(lens->aperture_radius >= 0.0f)) return jade_fail(JADE_ERR_INVALID, "aperture_radius must be finite and >= 0");
  if (lens->aperture_radius > 0.0f && (!std::isfinite(lens->focus_distance) || !(lens->focus_distance > 0.0f)))
    return jade_fail(JADE_ERR_INVALID, "focus_distance must be finite and > 0 with an open aperture");
  s->lens = *lens;
  return JADE_OK;
}
int jade_scene_get_lens(jade_scene* s, jade_lens_params* out) {
  if (!s || !out) return jade_fail(JADE_ERR_INVALID, "null argument");
  *out = s->lens;
  return JADE_OK;
}

// The shutter of the scene handle (include/jade_bvh.h): checked here, read by the next jade_render_begin.
int jade_scene_set_shutter(jade_scene* s, const jade_shutter_params* sh) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (!sh) {
    s->shutter = jade_shutter_params{};
    s->shutter_set = false;
    return JADE_OK;
  }
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(sh->eye_close[i])) return jade_fail(JADE_ERR_INVALID, "eye_close must be finite");
  for (int j = 0; j < 16; ++j)
    if (!std::isfinite(sh->camera_close[j])) return jade_fail(JADE_ERR_INVALID, "camera_close must be finite");
  if (!std::isfinite(sh->t_open) || !std::isfinite(sh->t_close) || !(0.0f <= sh->t_open && sh->t_open <= sh->t_close && sh->t_close <= 1.0f))
    return jade_fail(JADE_ERR_INVALID, "the shutter interval must satisfy 0 <= t_open <= t_close <= 1");
  s->shutter = *sh;
  s->shutter_set = true;
  return JADE_OK;
}
int jade_scene_get_shutter(jade_scene* s, jade_shutter_params* out, int* is_set) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (out) *out = s->shutter_set ? s->shutter : jade_shutter_params{};
  if (is_set) *is_set = s->shutter_set ? 1 : 0;
  return JADE_OK;
}

// The two-valued settings (include/jade_bvh.h): one of the two values, or refused in the setting's own words; read by the next jade_render_begin.
static int set_choice(jade_scene* s, int jade_scene::*field, int value, int a, int b, const char* unknown) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  if (value != a && value != b) return jade_fail(JADE_ERR_INVALID, unknown);
  s->*field = value;
  return JADE_OK;
}
static int get_choice(jade_scene* s, int jade_scene::*field, int* value) {
  if (!s || !value) return jade_fail(JADE_ERR_INVALID, "null argument");
  *value = s->*field;
  return JADE_OK;
}
int jade_scene_set_light_sampling(jade_scene* s, int mode) {
  return set_choice(s, &jade_scene::light_sampling, mode, JADE_LIGHTS_ALL, JADE_LIGHTS_ONE, "unknown light sampling (JADE_LIGHTS_*)");
}
int jade_scene_get_light_sampling(jade_scene* s, int* mode) { return get_choice(s, &jade_scene::light_sampling, mode); }
int jade_scene_set_bounce_sampling(jade_scene* s, int mode) {
  return set_choice(s, &jade_scene::bounce_sampling, mode, JADE_BOUNCE_UNIFORM, JADE_BOUNCE_COSINE, "unknown bounce sampling (JADE_BOUNCE_*)");
}
int jade_scene_get_bounce_sampling(jade_scene* s, int* mode) { return get_choice(s, &jade_scene::bounce_sampling, mode); }
int jade_scene_set_direct_sampling(jade_scene* s, int mode) {
  return set_choice(s, &jade_scene::direct_sampling, mode, JADE_DIRECT_RAYS, JADE_DIRECT_MIS, "unknown direct sampling (JADE_DIRECT_*)");
}
int jade_scene_get_direct_sampling(jade_scene* s, int* mode) { return get_choice(s, &jade_scene::direct_sampling, mode); }
int jade_scene_set_branch_sampling(jade_scene* s, int mode) {
  return set_choice(s, &jade_scene::branch_sampling, mode, JADE_BRANCH_RANDOM, JADE_BRANCH_STRATIFIED, "unknown branch sampling (JADE_BRANCH_*)");
}
int jade_scene_get_branch_sampling(jade_scene* s, int* mode) { return get_choice(s, &jade_scene::branch_sampling, mode); }
// ... and the passes, which take any int: zero or not
int jade_scene_set_passes(jade_scene* s, int on) {
  if (!s) return jade_fail(JADE_ERR_INVALID, "null argument");
  s->passes = on != 0;
  return JADE_OK;
}
int jade_scene_get_passes(jade_scene* s, int* on) {
  if (!s || !on) return jade_fail(JADE_ERR_INVALID, "null argument");
  *on = s->passes ? 1 : 0;
  return JADE_OK;
}
