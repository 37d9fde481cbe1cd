// jade_smooth_shade.h — the bounce and the fold a second time, with the shading normal (jade_smooth.h; include/jade_bvh.h, "The shading normal,
// stated"): bounce_branch, bounce_mirror, begin_bounce_lean and consume (jade_shade.h) are every other kernel's, k_light's and k_tail's among
// them, and an argument more on them moves those kernels' registers.  The texts below carry the bits a smooth mode is built with (SM_ENVIS,
// SM_ENVMIX, SM_COSINE) and no other; shade_record (jade_hip.hip) calls them in the kernels of a mode with SM_SMOOTH.
// A textured mode (SM_TEX, raised with SM_SMOOTH; jade_texture.h; "The surface colour, stated") runs these texts too: `table` is then a TexTables -
// the vertex normals together with the texture tables - in place of the `const float4*`, and the four places that read the vertex's brdf or
// refract_albedo read them times the surface colour at the vertex, each under `if constexpr (has_textures<ST>)`: in the other modes no instruction moves.
// A mapped mode (SM_NMAP, raised with both; jade_normal_map.h; "The mapped normal, stated") runs them a third way: `table` is a MapTables, which
// has_textures holds for, and every shading_normal(table, ...) below resolves to that header's overload - the mapped normal.  No other text changes.
#pragma once
#include "jade_shade.h"
#include "jade_smooth.h"
#include "jade_texture.h"
#include "jade_normal_map.h"

// bounce_mirror with the vertex's shading normal n; g: its flat normal.  A reflected direction that does not leave on the side of g that
// `out` is on is formed again with g.
template <class PX, class ST = const float4*>
static __device__ __forceinline__ bool bounce_mirror_smooth(PX& px, ShadeCtx& c, const DevMaterial* ot, jvec3 obj_emissive, jvec3 n, jvec3 g, jvec3* l_final, ST table = ST()) {
  const float RR_F = (float)JADE_RR_RATE_D;
  jvec3 obj_hit_fr = jv_scale(V3(ot->brdf), (float)(1.0 / JADE_PI_D));
  int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  if (obj_emissive.x > 1.5e-4f || obj_emissive.y > 1.5e-4f || obj_emissive.x > 1.5e-4f) {
    if constexpr (has_textures<ST>) obj_hit_fr = jv_scale(textured(table, c.obj, c.src, V3(ot->brdf)), (float)(1.0 / JADE_PI_D));  // (the one term of this step that reads the brdf)
    *l_final = jv_scale(jv_mul(obj_emissive, obj_hit_fr), (float)k);
    return false;
  }
  float rr_result = jade_rand(&c.rng);
  if (!(rr_result < RR_F)) return false;
  jvec3 refl = jv_sub(jv_scale(n, 2 * jv_dot(c.out, n)), c.out);
  if (!same_side(refl, c.out, g)) refl = jv_sub(jv_scale(g, 2 * jv_dot(c.out, g)), c.out);
  px.set_origin(c.src, c.obj);
  px.set_dir(0, refl);
  px.set_hit(0, -1);
  c.n_emit_rays++;
  c.stage = ST_MIRROR;
  c.flags = 0;
  return true;
}
// begin_bounce_lean with the shading normal
template <class PX, class ST>
static __device__ bool begin_bounce_lean_smooth(const DevScene& S, PX& px, ShadeCtx& c, jvec3* l_final, ST table) {
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  c.c_shaded += 1;
  jvec3 obj_emissive = V3(ot->emissive);
  if (obj_emissive.x > 1.4e-5f || obj_emissive.y > 1.4e-5f || obj_emissive.z > 1.4e-5f) {
    *l_final = obj_emissive;
    return false;
  }
  *l_final = jv(0, 0, 0);
  (void)jade_rand(&c.rng);  // select_reflex_refract: drawn for every material, decides nothing for a pure mirror
  return bounce_mirror_smooth(px, c, ot, obj_emissive, shading_normal(table, c.obj, ots.norm, c.src, c.out), ots.norm, l_final, table);
}

// bounce_branch with the shading normal: n at (c.obj, c.src) for c.out, t_norm at the BSSRDF exit for inner_direction.  Every side test, flip
// and cosine is made against that normal; a drawn direction that passes is tested against the flat normal the same way and, failing there,
// is not traced: an emitter ray as the reference's `continue`, the environment ray as STF_NOENV, the indirect ray as a roulette that
// failed.  All draws are the flat render's, in its order.  The refraction entry's direction and Fresnel factor are formed again with the
// flat normal where the direction does not cross the triangle.
template <uint32_t M, class ST>
static __device__ __forceinline__ bool bounce_branch_smooth(int type, const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final, ST table) {
  constexpr bool ENVIS = sm(M, SM_ENVIS), COSINE = sm(M, SM_COSINE), ENVMIX = sm(M, SM_ENVMIX);
  const jade_triangle* T = S.tris;  // vertices only
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  const int nE = S.n_emit;
  const int nL = nE;
  const float RR_F = (float)JADE_RR_RATE_D;
  const jvec3 g = ots.norm;
  const jvec3 n = shading_normal(table, c.obj, g, c.src, c.out);
  *l_final = jv(0, 0, 0);
  if (type == BT_DIFFUSE) goto diffuse_like;
  if (type == BT_MIRROR) return bounce_mirror_smooth(px, c, ot, V3(ot->emissive), n, g, l_final, table);
  if (type == BT_BSSRDF) {
    {
      int middle = S.mapping[exit_search(S, ot->obj_idx, jade_rand(&c.rng))];
      float rand_x = jade_rand(&c.rng);
      float rand_y = jade_rand(&c.rng);
      if (rand_x + rand_y > 1) {
        rand_x = 1 - rand_x;
        rand_y = 1 - rand_y;
      }
      const ShadeTri t_is = shade_tri(S, middle);
      const DevMaterial* t_i = t_is.m;
      const jvec3 t_g = t_is.norm;
      const jvec3 rate = V3(t_i->refract_rate);
      jvec3 random_point = tri_point(&T[middle], rand_x, rand_y);
      jvec3 inner_direction = jv_sub(random_point, c.src);
      const jvec3 t_norm = shading_normal(table, middle, t_g, random_point, inner_direction);
      float inner_distance = jade_sqrt(jv_dot(inner_direction, inner_direction));
      float neg_d = -1.0f * inner_distance;
      float neg_d3 = (float)((double)neg_d / 3.0);
      const float E_F = (float)JADE_E_D;
      jvec3 e1 = jv(jade_powf(E_F, neg_d / rate.x), jade_powf(E_F, neg_d / rate.y), jade_powf(E_F, neg_d / rate.z));
      jvec3 e2 = jv(jade_powf(E_F, neg_d3 / rate.x), jade_powf(E_F, neg_d3 / rate.y), jade_powf(E_F, neg_d3 / rate.z));
      jvec3 bssrdf = jv_div(jv_add(e1, e2), jv_scale(rate, (float)(8 * JADE_PI_D * (double)inner_distance)));
      float eta = t_i->refract_index;
      float R0 = (eta - 1) / (eta + 1) * (eta - 1) / (eta + 1);
      float one_cosine_i = 1 - jade_fabs(jv_dot(n, c.out));
      float one_cosine_i_sqr = one_cosine_i * one_cosine_i;
      float fresnel_rate_i = R0 + (1 - R0) * one_cosine_i_sqr * one_cosine_i_sqr * one_cosine_i;
      bssrdf = jv_scale(bssrdf, fresnel_rate_i);

      px.set_origin(random_point, middle);
      px.set_aux(bssrdf);
      for (int i = 0; i < nL; ++i) {  // (the reference tests no side here, so none is tested against the flat normal either)
        float rx = jade_rand(&c.rng);
        float ry = jade_rand(&c.rng);
        if (rx + ry > 1) {
          rx = 1 - rx;
          ry = 1 - ry;
        }
        const jade_triangle* et = &T[S.emit[i]];
        jvec3 random_emit_point = tri_point(et, rx, ry);
        const jvec3 sd = jv_sub(random_emit_point, random_point);
        px.set_dir(i, sd);
        px.set_limit(i, shadow_limit(et, random_point, sd));
        c.n_emit_rays++;
      }
      const float inn = jv_dot(inner_direction, t_norm), inn_g = jv_dot(inner_direction, t_g);
      uint32_t noenv = 0;
      {
        float ratio = 0.0f;
        uint32_t mix = 0;
        bool wrong = false;
        jvec3 ray_direction;
        if (ENVIS) {
          ray_direction = ENVMIX ? env_mix_sample<COSINE>(S, &c.rng, t_norm, inn, &ratio, &mix) : env_sample(S, &c.rng, &ratio);
          wrong = ENVMIX ? (mix & EMI_WRONG) != 0 : jv_dot(ray_direction, t_norm) * inn < 0;
        } else {
          ray_direction = COSINE ? cosine_dir_rng(&c.rng, t_norm, inn) : sphere_dir(&c.rng);
          if (!COSINE && jv_dot(ray_direction, t_norm) * inn < 0) ray_direction = jv_neg(ray_direction);
        }
        if (wrong || jv_dot(ray_direction, t_g) * inn_g < 0) {
          px.set_hit(nL, -2);
          noenv = STF_NOENV;
        } else {
          px.set_dir(nL, ray_direction);
          px.set_limit(nL, JADE_INF_F);
          if (ENVIS) px.set_auxi(__float_as_int(ratio));
          c.n_emit_rays++;
        }
      }
      // (COSINE: the opposite hemisphere, as the reference has it)
      jvec3 ray_direction = COSINE ? cosine_dir_rng(&c.rng, t_norm, -inn) : sphere_dir(&c.rng);
      if (!COSINE && jv_dot(ray_direction, t_norm) * inn > 0) ray_direction = jv_neg(ray_direction);
      float rr_result = jade_rand(&c.rng);
      c.stage = ST_BSSRDF;
      c.flags = noenv;
      if (rr_result < RR_F && !(jv_dot(ray_direction, t_g) * inn_g > 0)) {
        c.flags |= STF_RR;
        px.set_dir(nL + 1, ray_direction);
        px.set_hit(nL + 1, -1);
        c.n_emit_rays++;
      } else {
        px.set_hit(nL + 1, -2);
      }
      return true;
    }
  }
  // ---- direct refraction entry ----
  {
    {
      float triangle_miu = ot->refract_index;
      float R0 = (1 - triangle_miu) / (1 + triangle_miu) * (1 - triangle_miu) / (1 + triangle_miu);
      jvec3 rev_out_direction = jv_scale(c.out, -1.0f);
      bool full_reflex = false;
      jvec3 nn = n;
      jvec3 refract_ray = gen_refract_ray(rev_out_direction, nn, (float)(1.0 / (double)triangle_miu), &full_reflex);
      if (!other_side(refract_ray, c.out, g)) {
        nn = g;
        refract_ray = gen_refract_ray(rev_out_direction, nn, (float)(1.0 / (double)triangle_miu), &full_reflex);
      }
      float one_cosine_i = 1 - jade_fabs(jv_dot(nn, c.out));
      float one_cosine_i_sqr = one_cosine_i * one_cosine_i;
      float fresnel_rate_i = R0 + (1 - R0) * one_cosine_i_sqr * one_cosine_i_sqr * one_cosine_i;
      px.set_aux(jv(1 - fresnel_rate_i, 1 - fresnel_rate_i, 1 - fresnel_rate_i));
      px.set_auxi(0);
      px.set_origin(c.src, c.obj);
      px.set_dir(0, refract_ray);
      px.set_hit(0, -1);
      c.n_emit_rays++;
      c.stage = ST_REFRACT_LOOP;
      c.flags = 0;
      return true;
    }
  }

diffuse_like:
  {
    px.set_origin(c.src, c.obj);
    const float side = jv_dot(c.out, n), side_g = jv_dot(c.out, g);
    for (int i = 0; i < nL; ++i) {
      float rand_x = jade_rand(&c.rng);
      float rand_y = jade_rand(&c.rng);
      if (rand_x + rand_y > 1) {
        rand_x = 1 - rand_x;
        rand_y = 1 - rand_y;
      }
      const jade_triangle* et = &T[S.emit[i]];
      jvec3 random_point = tri_point(et, rand_x, rand_y);
      jvec3 obj_light_direction = jv_sub(random_point, c.src);
      px.set_dir(i, obj_light_direction);
      if (jv_dot(obj_light_direction, n) * side < 0 || jv_dot(obj_light_direction, g) * side_g < 0) {
        px.set_hit(i, -2);  // `continue`: no shadow ray
      } else {
        px.set_limit(i, shadow_limit(et, c.src, obj_light_direction));
        c.n_emit_rays++;
      }
    }
    {
      float ratio = 0.0f;
      uint32_t mix = 0;
      bool wrong = false;
      jvec3 ray_direction;
      if (ENVIS) {
        ray_direction = ENVMIX ? env_mix_sample<COSINE>(S, &c.rng, n, side, &ratio, &mix) : env_sample(S, &c.rng, &ratio);
        wrong = ENVMIX ? (mix & EMI_WRONG) != 0 : jv_dot(ray_direction, n) * side < 0;
      } else {
        ray_direction = COSINE ? cosine_dir_rng(&c.rng, n, side) : sphere_dir(&c.rng);
        if (!COSINE && jv_dot(ray_direction, n) * side < 0) ray_direction = jv_neg(ray_direction);
      }
      if (wrong || jv_dot(ray_direction, g) * side_g < 0) {
        px.set_hit(nL, -2);
        c.flags |= STF_NOENV;
      } else {
        px.set_dir(nL, ray_direction);
        px.set_limit(nL, JADE_INF_F);
        if (ENVIS) px.set_auxi(__float_as_int(ratio));
        c.n_emit_rays++;
      }
    }
    float rr_result = jade_rand(&c.rng);
    bool go_on = false;
    if (rr_result < RR_F) {
      jvec3 ray_direction = COSINE ? cosine_dir_rng(&c.rng, n, side) : sphere_dir(&c.rng);
      if (!COSINE && jv_dot(ray_direction, n) * side < 0) ray_direction = jv_neg(ray_direction);
      if (!(jv_dot(ray_direction, g) * side_g < 0)) {
        go_on = true;
        c.flags |= STF_RR;
        px.set_dir(nL + 1, ray_direction);
        px.set_hit(nL + 1, -1);
        c.n_emit_rays++;
      }
    }
    if (!go_on) px.set_hit(nL + 1, -2);
    return true;
  }
}
template <uint32_t M, class ST>
static __device__ bool begin_bounce_smooth(const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final, ST table) {
  const int type = bounce_classify(S, c, l_final);
  if (type == BT_END) return false;
  return bounce_branch_smooth<M>(type, S, px, c, l_final, table);
}

// consume with the shading normal: the vertex's again from (c.obj, c.src, c.out), the BSSRDF exit's from (the record's source triangle, its
// origin, origin - c.src), a refraction hit's from (the triangle hit, the hit point, the reversed ray).  Nothing travels with the record.
// An environment slot may hold "no ray" (-2) whatever the environment sampling is.  An emitter's own normal stays its flat one.
// consume_mirror (jade_shade.h) for a textured mode: its text again, with the vertex's brdf_eff - the colour at the vertex the mirror ray
// left from, read before the path moves on.  No passes in these modes.
template <class PX>
static __device__ __forceinline__ int consume_mirror_textured(const DevScene& S, const PX& px, ShadeCtx& c, jvec3* l_final, const TexTables& table) {
  const DevMaterial* ot = shade_tri(S, c.obj).m;
  const int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  const jvec3 obj_hit_fr = jv_scale(textured(table, c.obj, px.origin(), V3(ot->brdf)), (float)(1.0 / JADE_PI_D));  // (the ray's origin IS the vertex's point - bounce_mirror_smooth stored c.src there - and a record in ST_MIRROR does not keep c.src)
  float kk = (float)(k / (JADE_RR_RATE_D / JADE_PI_D));
  jvec3 refl = px.dir(0);
  int nh = px.hit(0);
  if (nh >= 0) {
    c.out = jv_neg(refl);
    c.src = px.hpt(0);
    c.obj = nh;
    *l_final = jv(0, 0, 0);
    return path_push(c, jv(0, 0, 0), jv_scale(obj_hit_fr, kk)) ? CONSUME_END : CONSUME_VERTEX;
  }
  *l_final = jv_scale(jv_mul(sample_hdr(S, refl), obj_hit_fr), kk);
  return CONSUME_END;
}

// A textured mode (ST = TexTables, jade_texture.h): the ST_DIFFUSE fold's brdf and refract_albedo are the vertex's brdf_eff and albedo_eff,
// and the mirror's fold is consume_mirror_textured.  The other stages read neither.
template <uint32_t M, class ST>
static __device__ int consume_smooth(const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final, ST table) {
  constexpr bool ENVIS = sm(M, SM_ENVIS), COSINE = sm(M, SM_COSINE);
  const jade_triangle* T = S.tris;  // vertices only
  const int nE = S.n_emit;
  const int nL = nE;
  const float PI_F = (float)JADE_PI_D;
  const float RR_F = (float)JADE_RR_RATE_D;
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  const int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  jvec3 colour = jv(1.0f, 1.0f, 1.0f);  // (read by a textured mode alone)
  if constexpr (has_textures<ST>)
    if (c.stage == ST_DIFFUSE) colour = surface_colour(table, c.obj, c.src);
  const jvec3 obj_hit_fr = jv_scale(tinted<ST>(V3(ot->brdf), colour), (float)(1.0 / JADE_PI_D));
  jvec3 l_dir = jv(0, 0, 0);

  if (c.stage == ST_DIFFUSE) {
    const jvec3 n = shading_normal(table, c.obj, ots.norm, c.src, c.out);
    const bool sss = (c.flags & STF_SSS) != 0;
    const jvec3 f = sss ? jv_scale(tinted<ST>(V3(ot->refract_albedo), colour), (float)(1.0 / JADE_PI_D)) : obj_hit_fr;
    for (int i = 0; i < nL; ++i) {
      int h = px.hit(i);
      int emit_tri_idx = S.emit[i];
      if (h >= 0 && h == emit_tri_idx) {
        jvec3 ld = px.dir(i);
        const ShadeTri t_i = shade_tri(S, emit_tri_idx);
        float dls = jv_dot(ld, ld);
        jvec3 w = jv_mul(V3(t_i.m->emissive), f);
        w = jv_scale(w, jade_fabs(jv_dot(n, ld) * jv_dot(t_i.norm, ld)));
        w = jv_divs(jv_divs(w, dls), dls);
        w = jv_scale(w, tri_size(&T[emit_tri_idx]));
        l_dir = jv_add(l_dir, w);
      }
    }
    if (px.hit(nL) == -1) {  // (-1: traced and nothing hit; -2: no environment ray this bounce)
      jvec3 rd = px.dir(nL);
      jvec3 w = jv_mul(sample_hdr(S, rd), f);
      w = jv_scale(w, COSINE && !ENVIS ? cosine_weight(n, rd) : jade_fabs(jv_dot(n, rd)));
      w = jv_scale(jv_scale(w, 2.0f), PI_F);
      if (ENVIS) w = jv_scale(w, __int_as_float(px.auxi()));
      l_dir = jv_add(l_dir, w);
    }
    l_dir = jv_scale(l_dir, sss ? (float)(k / JADE_SSS_RATE_D) : (float)k);
    *l_final = l_dir;
    if (!(c.flags & STF_RR)) return CONSUME_END;
    int nh = px.hit(nL + 1);
    if (nh >= 0 && nonemissive(shade_tri(S, nh).m)) {
      jvec3 rd = jv_neg(px.dir(nL + 1));
      jvec3 indir_rate = jv_divs(jv_scale(obj_hit_fr, COSINE ? cosine_weight(n, rd) : jade_fabs(jv_dot(rd, n))), RR_F);
      jvec3 rate = sss ? jv_divs(jv_scale(indir_rate, (float)k), (float)JADE_SSS_RATE_D) : jv_scale(indir_rate, (float)k);
      c.src = px.hpt(nL + 1);
      c.out = rd;
      c.obj = nh;
      return path_push(c, l_dir, rate) ? CONSUME_END : CONSUME_VERTEX;
    }
    return CONSUME_END;
  }

  if (c.stage == ST_BSSRDF) {
    const int middle = px.skip();
    const ShadeTri t_is = shade_tri(S, middle);
    const DevMaterial* t_i = t_is.m;
    const jvec3 exit_point = px.origin();
    const jvec3 t_norm = shading_normal(table, middle, t_is.norm, exit_point, jv_sub(exit_point, c.src));
    const jvec3 bssrdf = px.aux();
    const float eta = t_i->refract_index;
    const float R0 = (eta - 1) / (eta + 1) * (eta - 1) / (eta + 1);
    const float area_total = S.prefix[S.segs[t_i->obj_idx].end_idx];
    for (int i = 0; i < nL; ++i) {
      int h = px.hit(i);
      int emit_tri_idx = S.emit[i];
      if (h >= 0 && h == emit_tri_idx) {
        jvec3 ld = px.dir(i);
        const ShadeTri emit_i = shade_tri(S, emit_tri_idx);
        float fresnel_rate_o = schlick_out(R0, jade_fabs(jv_dot(jv_normalize(ld), t_norm)));
        float dls = jv_dot(ld, ld);
        jvec3 w = jv_scale(V3(emit_i.m->emissive), fresnel_rate_o);
        w = jv_mul(w, bssrdf);
        w = jv_scale(w, jade_fabs(jv_dot(t_norm, ld) * jv_dot(emit_i.norm, ld)));
        w = jv_divs(jv_divs(w, dls), dls);
        w = jv_scale(w, tri_size(&T[emit_tri_idx]));
        w = jv_divs(w, PI_F);
        w = jv_scale(w, area_total);
        l_dir = jv_add(l_dir, w);
      }
    }
    if (px.hit(nL) == -1) {
      jvec3 rd = px.dir(nL);
      float fresnel_rate_o = schlick_out(R0, jade_fabs(jv_dot(rd, t_norm)));
      jvec3 w = jv_mul(jv_scale(sample_hdr(S, rd), fresnel_rate_o), bssrdf);
      w = jv_scale(jv_scale(w, COSINE && !ENVIS ? cosine_weight(t_norm, rd) : jade_fabs(jv_dot(t_norm, rd))), 2.0f);
      if (ENVIS) w = jv_scale(w, __int_as_float(px.auxi()));
      l_dir = jv_add(l_dir, w);
    }
    l_dir = jv_scale(l_dir, (float)(k / (1 - JADE_SSS_RATE_D)));
    *l_final = l_dir;
    if (!(c.flags & STF_RR)) return CONSUME_END;
    int nh = px.hit(nL + 1);
    if (nh >= 0 && nonemissive(shade_tri(S, nh).m)) {
      jvec3 rd = jv_neg(px.dir(nL + 1));
      float fresnel_rate_o = schlick_out(R0, jade_fabs(jv_dot(rd, t_norm)));
      jvec3 indir_rate = jv_scale(bssrdf, fresnel_rate_o);
      indir_rate = jv_scale(indir_rate, COSINE ? cosine_weight(t_norm, rd) : jade_fabs(jv_dot(rd, t_norm)));
      indir_rate = jv_scale(indir_rate, area_total);
      indir_rate = jv_divs(jv_scale(indir_rate, 2.0f), RR_F);
      jvec3 rate = jv_divs(jv_scale(indir_rate, (float)k), (float)(1 - JADE_SSS_RATE_D));
      c.src = px.hpt(nL + 1);
      c.out = rd;
      c.obj = nh;
      return path_push(c, l_dir, rate) ? CONSUME_END : CONSUME_VERTEX;
    }
    return CONSUME_END;
  }

  if (c.stage == ST_MIRROR) {  // (no normal in it)
    if constexpr (has_textures<ST>) return consume_mirror_textured(S, px, c, l_final, table);
    else return consume_mirror<Px, 0>(S, px, c, l_final, nullptr);
  }

  if (c.stage == ST_REFRACT_LOOP) {
    const float triangle_miu = ot->refract_index;
    const float R0 = (1 - triangle_miu) / (1 + triangle_miu) * (1 - triangle_miu) / (1 + triangle_miu);
    int nh = px.hit(0);
    if (nh < 0) return CONSUME_ZERO;
    const ShadeTri hts = shade_tri(S, nh);
    const DevMaterial* ht = hts.m;
    const jvec3 in_ray = px.dir(0);
    jvec3 start = px.origin();
    jvec3 hp = px.hpt(0);
    const jvec3 rev = jv_neg(in_ray);
    jvec3 l_indir_rate = px.aux();
    jvec3 distance = jv_sub(start, hp);
    float dist = jade_sqrt(jv_dot(distance, distance));
    l_indir_rate = jv_mul(l_indir_rate, jv(jade_powf(ht->refract_rate[0], dist), jade_powf(ht->refract_rate[1], dist),
                                           jade_powf(ht->refract_rate[2], dist)));
    float reflex_refract_select = jade_rand(&c.rng);
    int it = px.auxi() + 1;
    // the iteration's direction and Fresnel factor with normal hn: reflected (on the side of the flat normal the ray came from) or refracted (on the other)
    jvec3 refract_ray;
    float fresnel_rate_o = 0.0f;
    bool full_reflex = false, reflected = false;
    auto form = [&](jvec3 hn) {
      full_reflex = false;
      refract_ray = gen_refract_ray(in_ray, hn, triangle_miu, &full_reflex);
      fresnel_rate_o = schlick_out(R0, jade_fabs(jv_dot(refract_ray, hn)));
      reflected = full_reflex || reflex_refract_select < 0.2f;
      if (reflected) refract_ray = jv_sub(refract_ray, jv_scale(hn, 2 * jv_dot(refract_ray, hn)));
    };
    form(shading_normal(table, nh, hts.norm, hp, rev));
    if (!(reflected ? same_side(refract_ray, rev, hts.norm) : other_side(refract_ray, rev, hts.norm))) form(hts.norm);
    bool leave = true;
    if (reflected) {
      if (!full_reflex) l_indir_rate = jv_scale(l_indir_rate, fresnel_rate_o * 5);
      leave = it >= JADE_MAX_FULL_REFLEX_TIME;
    } else {
      l_indir_rate = jv_scale(l_indir_rate, (float)((1.0 - (double)fresnel_rate_o) * 1.25));
    }
    px.set_origin(hp, nh);
    px.set_aux(l_indir_rate);
    px.set_auxi(it);
    px.set_dir(0, refract_ray);
    px.set_hit(0, -1);
    *l_final = jv(0, 0, 0);
    if (!leave) {
      c.n_emit_rays++;
      return CONSUME_EMITTED;
    }
    float rr_result = jade_rand(&c.rng);
    if (!(rr_result < RR_F)) return CONSUME_END;
    c.stage = ST_REFRACT_EXIT;
    c.n_emit_rays++;
    return CONSUME_EMITTED;
  }

  // ST_REFRACT_EXIT
  {
    jvec3 refract_ray = px.dir(0);
    jvec3 l_indir_rate = px.aux();
    float kk = (float)(k / JADE_RR_RATE_D);
    int nh = px.hit(0);
    if (nh >= 0) {
      c.out = jv_scale(refract_ray, -1.0f);
      c.src = px.hpt(0);
      c.obj = nh;
      *l_final = jv(0, 0, 0);
      return path_push(c, jv(0, 0, 0), jv_scale(l_indir_rate, kk)) ? CONSUME_END : CONSUME_VERTEX;
    }
    *l_final = jv_scale(jv_mul(sample_hdr(S, refract_ray), l_indir_rate), kk);
    return CONSUME_END;
  }
}
