// jade_shade.h — the bounce loop of pathTracing (PathTrace.cu:905-1416) and the
// sample loop of render_pixel (:1418-1455) as a per-pixel state machine.
//
// The reference runs one thread per pixel through `spp` samples and calls
// hitBVH inline (nEmit + 2 times per bounce).  Here a pixel is a record in
// HBM; each pass of k_shade (a) folds the hit results of the rays it issued on
// the previous pass into the path, (b) samples the next bounce and (c) emits
// ALL rays of that bounce at once into a compacted queue for k_trace.  That is
// possible because no random draw of a bounce depends on a hit result of the
// same bounce: the draw order below is the textual order of the
// curand_uniform calls, only the hitBVH calls are deferred.
//
// Radiance bookkeeping: the reference pushes (dir, rate) pairs on two
// 128-entry stacks and unwinds them Horner-style (:1410-1413).  The same sum
// is accumulated forward here (acc += thr * dir; thr *= rate), which differs
// from the unwind only by fp32 rounding of the radiance (never of a decision).
#pragma once
#include <type_traits>
#include "jade_device.h"
#include "jade_runtime.h"  // ShadeMode and sm: the functions below that differ by render mode are templates over the mode's mask
#include "jade_texture.h"  // TexTables: what a textured mode's argument bundle carries
#include "jade_normal_map.h"  // MapTables: ... and a mapped mode's

static __device__ __forceinline__ int mirror_index(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  if (m >= n) m = 2 * n - 1 - m;
  return m;
}

// SampleSphericalMap's coordinates of direction v (PathTrace.cu:686-692), NaN rule included: the statements sample_hdr and env_texel_of share
static __device__ __forceinline__ void env_uv_of(jvec3 v, float* u_out, float* v_out) {
  jvec3 nv = jv_normalize(v);
  float ux = jade_atan2f(nv.z, nv.x);
  float uy = jade_asinf(nv.y);
  // (float)((double)x / C) written as (float)((double)x * (1.0 / C)): NOT the same in general, but the same for EVERY float |x| <= 3.2
  // with C = 2 * JADE_PI_D and |x| <= 1.6 with C = JADE_PI_D - all 4.3e9 of them compared (tests/native/dpdiv_exhaustive.c,
  // tests/test_fpmath.py) - and atan2 / asin return nothing outside those ranges.  Two double-precision divisions (~15 instructions
  // each at half rate or less) become two multiplications in a function every sky sample of the first pass runs.
  ux = (float)((double)ux * (1.0 / (2.0 * JADE_PI_D)));
  uy = (float)((double)uy * (1.0 / JADE_PI_D));
  ux = (float)((double)ux + 0.5);
  uy = (float)((double)uy + 0.5);
  uy = (float)(1.0 - (double)uy);
  if (jade_isnan(ux)) ux = 0.0f;
  if (jade_isnan(uy)) uy = 0.0f;
  *u_out = ux;
  *v_out = uy;
}

// sampleHdr / SampleSphericalMap, PathTrace.cu:686-702; software bilinear with
// mirror addressing in place of tex2D (gfx950 has no sampler path).
static __device__ jvec3 sample_hdr(const DevScene& S, jvec3 v) {
  float ux, uy;
  env_uv_of(v, &ux, &uy);
  const int W = S.env_w, H = S.env_h;
  float x = ux * (float)W - 0.5f;
  float y = uy * (float)H - 0.5f;
  float xf = jade_floorf(x), yf = jade_floorf(y);
  float ax = x - xf, ay = y - yf;
  int i0 = mirror_index((int)xf, W), i1 = mirror_index((int)xf + 1, W);
  int j0 = mirror_index((int)yf, H), j1 = mirror_index((int)yf + 1, H);
  float w00 = (1.0f - ax) * (1.0f - ay), w10 = ax * (1.0f - ay);
  float w01 = (1.0f - ax) * ay, w11 = ax * ay;
  const float* t00 = S.env + 3 * ((size_t)j0 * W + i0);
  const float* t10 = S.env + 3 * ((size_t)j0 * W + i1);
  const float* t01 = S.env + 3 * ((size_t)j1 * W + i0);
  const float* t11 = S.env + 3 * ((size_t)j1 * W + i1);
  jvec3 c;
  c.x = ((w00 * t00[0] + w10 * t10[0]) + w01 * t01[0]) + w11 * t11[0];
  c.y = ((w00 * t00[1] + w10 * t10[1]) + w01 * t01[1]) + w11 * t11[1];
  c.z = ((w00 * t00[2] + w10 * t10[2]) + w01 * t01[2]) + w11 * t11[2];
  c.x = c.x < 10.0f ? c.x : 10.0f;
  c.y = c.y < 10.0f ? c.y : 10.0f;
  c.z = c.z < 10.0f ? c.z : 10.0f;
  return c;
}

// The texel of the map direction v lies in (JADE_ENV_MIXTURE, include/jade_rt.h): column min((uint32)fl(u W), W - 1), row
// min((uint32)fl(v H), H - 1) of env_uv_of's coordinates - a negative product or a NaN converts to 0 - so the answer is below W * H
// whatever v holds.
static __device__ __forceinline__ uint32_t env_texel_of(const DevScene& S, jvec3 v) {
  float ux, uy;
  env_uv_of(v, &ux, &uy);
  const uint32_t W = (uint32_t)S.env_w, H = (uint32_t)S.env_h;
  const float fx = ux * (float)W, fy = uy * (float)H;
  uint32_t i = fx > 0.0f ? (uint32_t)fx : 0u;  // (a NaN compares false)
  uint32_t j = fy > 0.0f ? (uint32_t)fy : 0u;
  i = i < W - 1u ? i : W - 1u;
  j = j < H - 1u ? j : H - 1u;
  return j * W + i;
}

// PathTrace.cu:968-971 on two uniforms from `next`, cosine first
template <class NextUniform>
static __device__ __forceinline__ jvec3 sphere_dir_with(NextUniform next) {
  float cosine_theta = (float)(2.0 * ((double)next() - 0.5));
  float sine_theta = jade_sqrt(1.0f - cosine_theta * cosine_theta);
  float fai_value = (float)(2.0 * JADE_PI_D * (double)next());
  float sn, cs;
  jade_sincosf(fai_value, &sn, &cs);
  return jv(sine_theta * cs, sine_theta * sn, cosine_theta);
}
static __device__ __forceinline__ jvec3 sphere_dir(uint32_t* rng) {  // ... with two successive jade_rand draws
  return sphere_dir_with([rng]() { return jade_rand(rng); });
}

// Environment importance sampling (jade_render_params.env_sampling = JADE_ENV_IMPORTANCE; NOT the reference's estimator), as
// include/jade_rt.h states it draw by draw: a texel of the map by the alias method (u1 the slot, u2 own / alias), a point in it
// uniformly (u3, u4), the direction SampleSphericalMap (PathTrace.cu:686-692) maps to that point.  ratio = (pdf of the reference's
// uniform hemisphere sampling, 1 / 2 pi) / (pdf of this direction): what the reference's weight is multiplied with; never negative.
// The body takes its uniforms from `next` where it needs them - u1 (the slot), u2 (own / alias), u3, u4 (the point) - so that the
// shading kernel's code is what it was with jade_rand written in those four places, and a test can feed the four numbers
// (jade_debug_units.hip).  *texel: the texel drawn, bit 31 = own (tests only; a caller that passes a dead variable pays nothing for it).
// env_sample_core_with: the draw up to the direction, with what a weight is formed from - *st_out = st, *q_out = the chosen texel's q -
// so that JADE_ENV_MIXTURE's sky technique (env_mix_sample_with) is these very statements.
template <class NextUniform>
static __device__ __forceinline__ jvec3 env_sample_core_with(const DevScene& S, NextUniform next, float* st_out, float* q_out, uint32_t* texel) {
  const uint32_t W = (uint32_t)S.env_w, N = W * (uint32_t)S.env_h;  // N <= 2^24: jade_render_begin refuses the mode otherwise
  uint32_t idx = (uint32_t)(next() * (float)N);
  idx = idx < N ? idx : N - 1u;
  const float u2 = next();
  const uint4 e = S.env_alias[idx];
  const bool own = u2 < jade_u2f(e.x);
  const float pdf_n = jade_u2f(own ? e.z : e.w);  // the chosen texel's probability x N
  idx = own ? idx : e.y;
  *texel = idx | (own ? 0x80000000u : 0u);
  const uint32_t j = idx / W, i = idx - j * W;
  const float u3 = next();
  const float u = ((float)i + u3) / (float)W, v = ((float)j + next()) / (float)S.env_h;
  const float theta = (float)JADE_PI_D * v, phi = (float)(2.0 * JADE_PI_D) * (u - 0.5f);
  float st, ct, sp, cp;
  jade_sincosf(theta, &st, &ct);
  jade_sincosf(phi, &sp, &cp);
  st = st > 0.0f ? st : 0.0f;  // a weight is never negative, whatever a sine rounds to at theta = fl(PI) (u4 = 1 in the bottom row; jade_sincosf: +1.5e-7)
  *st_out = st;
  *q_out = pdf_n;
  return jv(st * cp, ct, st * sp);
}
template <class NextUniform>
static __device__ __forceinline__ jvec3 env_sample_with(const DevScene& S, NextUniform next, float* ratio, uint32_t* texel) {
  float st, pdf_n;
  const jvec3 d = env_sample_core_with(S, next, &st, &pdf_n, texel);
  // pdf(direction) = pdf_n / (2 pi^2 sin theta); against 1 / (2 pi): ratio = pi sin theta / pdf_n
  *ratio = (float)JADE_PI_D * st / pdf_n;
  return d;
}
// ... with four successive jade_rand draws: what bounce_branch calls
static __device__ __forceinline__ jvec3 env_sample(const DevScene& S, uint32_t* rng, float* ratio) {
  uint32_t texel;
  return env_sample_with(S, [rng]() { return jade_rand(rng); }, ratio, &texel);
}
// ... and with four given numbers
static __device__ __forceinline__ jvec3 env_sample_at(const DevScene& S, const float* u4, float* ratio, uint32_t* texel) {
  int k = 0;
  return env_sample_with(S, [u4, &k]() { return u4[k++]; }, ratio, texel);
}

// One-light sampling (jade_scene_set_light_sampling = JADE_LIGHTS_ONE; NOT the reference's estimator), as include/jade_bvh.h states it
// draw by draw ("The lights, stated"): an entry of emit_indices by the alias method over `table` (nE entries {accept, alias, q_own, q_alias},
// light_alias_table, jade_scene_prep.hip; one 16-B gather per draw) - u1 the slot, u2 own / alias - then the reference's two numbers for
// the point on that entry's triangle (u3, u4), folded as the reference folds them.  Returns the entry; *weight = fl(nE) / q, what the
// entry's term is multiplied with.  The uniforms come from `next`, as env_sample_with's do.  nE >= 1 (<= 2^24: jade_render_begin).
template <class NextUniform>
static __device__ __forceinline__ uint32_t light_sample_with(const uint4* table, uint32_t nE, NextUniform next, float* rx, float* ry, float* weight) {
  uint32_t s = (uint32_t)(next() * (float)nE);
  s = s < nE ? s : nE - 1u;
  const float u2 = next();
  const uint4 e = table[s];
  const bool own = u2 < jade_u2f(e.x);
  const float q = jade_u2f(own ? e.z : e.w);  // the chosen entry's probability x nE
  float x = next();
  float y = next();
  if (x + y > 1) {
    x = 1 - x;
    y = 1 - y;
  }
  *rx = x;
  *ry = y;
  *weight = (float)nE / q;
  return own ? s : e.y;
}
// ... with four successive jade_rand draws: what bounce_branch calls (the weight is consume's to form, below)
static __device__ __forceinline__ uint32_t light_sample(const uint4* table, uint32_t nE, uint32_t* rng, float* rx, float* ry) {
  float weight;
  return light_sample_with(table, nE, [rng]() { return jade_rand(rng); }, rx, ry, &weight);
}
// The weight of entry i again, where its shadow ray's answer is folded in: q_alias of a slot is q_own of the entry it names, bit for bit
// (both are fl(q_i)), so the weight is a function of the entry alone and does not travel with the record.
static __device__ __forceinline__ float light_weight(const uint4* table, uint32_t nE, uint32_t i) {
  return (float)nE / jade_u2f(table[i].z);
}

// Cosine-weighted bounce sampling (jade_scene_set_bounce_sampling = JADE_BOUNCE_COSINE; NOT the reference's estimator), as include/jade_bvh.h
// states it ("The bounce, stated"): where sphere_dir takes its two uniforms this takes the same two - u1 first, u2 second, from `next` -
// and forms a direction with pdf cos / pi about the axis a = sign * n / |n|, in a branchless frame (Duff et al. 2017).  s: a number whose
// sign is the side - the axis points along -n where s < 0 - and, where the normal gives no axis (*fallback: n.n is 0, infinite or NaN),
// what the reference multiplies dot(direction, n) with in its flip: the direction is then sphere_dir's on the same two uniforms, flipped
// if dot(direction, n) * s < 0.  The kernels pass the very product term of the reference's flip (side, dot(inner, t_norm) or its
// negation), so a fallback vertex is the reference's statement; a test passes +-1.  The weight is consume's to form (cosine_weight).
template <class NextUniform>
static __device__ __forceinline__ jvec3 cosine_dir_with(NextUniform next, jvec3 n, float s, bool* fallback) {
  const float u1 = next();
  const float fai_value = (float)(2.0 * JADE_PI_D * (double)next());
  float sn, cs;
  jade_sincosf(fai_value, &sn, &cs);
  const float nn = jv_dot(n, n);
  if (!(nn > 0 && nn < jade_u2f(0x7f800000u))) {  // (+inf: JADE_INF_F is the reference's finite INF)
    *fallback = true;
    const float cosine_theta = (float)(2.0 * ((double)u1 - 0.5));  // sphere_dir, PathTrace.cu:968-971
    const float sine_theta = jade_sqrt(1.0f - cosine_theta * cosine_theta);
    const jvec3 d = jv(sine_theta * cs, sine_theta * sn, cosine_theta);
    return jv_dot(d, n) * s < 0 ? jv_neg(d) : d;
  }
  *fallback = false;
  jvec3 a = jv_divs(n, jade_sqrt(nn));
  if (s < 0) a = jv_neg(a);
  const float sg = a.z >= 0 ? 1.0f : -1.0f;
  const float p = -1.0f / (sg + a.z);
  const float q = a.x * a.y * p;
  const jvec3 t = jv(1.0f + sg * a.x * a.x * p, sg * q, -sg * a.x);
  const jvec3 b = jv(q, sg + a.y * a.y * p, -a.y);
  const float r = jade_sqrt(u1), cz = jade_sqrt(1.0f - u1);
  return jv_add(jv_add(jv_scale(t, r * cs), jv_scale(b, r * sn)), jv_scale(a, cz));
}
// ... with two successive jade_rand draws: what bounce_branch calls
static __device__ __forceinline__ jvec3 cosine_dir_rng(uint32_t* rng, jvec3 n, float s) {
  bool fallback;
  return cosine_dir_with([rng]() { return jade_rand(rng); }, n, s, &fallback);
}
// ... and with two given numbers
static __device__ __forceinline__ jvec3 cosine_dir_at(const float* u2, jvec3 n, float s, bool* fallback) {
  int k = 0;
  return cosine_dir_with([u2, &k]() { return u2[k++]; }, n, s, fallback);
}
// What consume multiplies with where the reference has |dot(n, rd)|: pdf cos / pi against the reference's 1 / 2 pi makes the factor
// |dot(n, rd)| / (2 cos) = |n| / 2, formed from the normal alone - no division by the cosine, nothing travels with the record.  A normal
// that gave no axis (cosine_dir_with's predicate, re-formed here) keeps the reference's factor.
static __device__ __forceinline__ float cosine_weight(jvec3 n, jvec3 rd) {
  const float nn = jv_dot(n, n);
  return (nn > 0 && nn < jade_u2f(0x7f800000u)) ? 0.5f * jade_sqrt(nn) : jade_fabs(jv_dot(n, rd));
}

// The environment mixture (jade_render_params.env_sampling = JADE_ENV_MIXTURE; NOT the reference's estimator), as include/jade_rt.h states
// it draw by draw: five uniforms from `next` - u0 picks the technique, u1..u4 are env_sample_with's four (the sky technique, u0 < 0.5) or
// the bounce sampling's two and two that are drawn and dropped (the hemisphere technique: cosine_dir_with under COSINE, sphere_dir's
// statements and the reference's flip otherwise).  n, side: the normal and the number whose sign is the surface's side, as cosine_dir_with
// takes them - the kernels pass the product term of the reference's flip.  *m = (1 / 2 pi) / (the mixture's density), what the
// reference's weight is multiplied with: it stands where JADE_ENV_IMPORTANCE has ratio.  *info (EMI_*): the texel of the direction, the
// technique, own / alias of a sky draw, and whether a sky draw lay on the wrong side - the caller traces no ray then.  A hemisphere
// direction is never tested again: it is on the surface's side by construction, whatever its dot product with n rounds to.
// One 16-B gather either way (the slot's entry, or the entry of the direction's texel: q_own of entry t is fl(q_t)).
enum : uint32_t { EMI_TEXEL = 0x00ffffffu, EMI_WRONG = 1u << 29, EMI_HEMI = 1u << 30, EMI_OWN = 1u << 31 };
template <bool COSINE, class NextUniform>
static __device__ __forceinline__ jvec3 env_mix_sample_with(const DevScene& S, NextUniform next, jvec3 n, float side, float* m, uint32_t* info) {
  const float u0 = next();
  const float nn = jv_dot(n, n);
  const bool axis = COSINE && nn > 0 && nn < jade_u2f(0x7f800000u);  // cosine_dir_with's predicate: otherwise the uniform form of m
  jvec3 w;
  float s, q;
  uint32_t word;
  if (u0 < 0.5f) {
    w = env_sample_core_with(S, next, &s, &q, &word);  // (bit 31 of the texel word is EMI_OWN)
    if (jv_dot(w, n) * side < 0) word |= EMI_WRONG;
  } else {
    if (COSINE) {
      bool fallback;
      w = cosine_dir_with(next, n, side, &fallback);
    } else {
      w = sphere_dir_with(next);
      if (jv_dot(w, n) * side < 0) w = jv_neg(w);
    }
    (void)next();  // u3, u4: drawn, so that every later draw of the sample is where the sky technique leaves it
    (void)next();
    s = jade_sqrt(w.x * w.x + w.z * w.z);
    const uint32_t t = env_texel_of(S, w);
    q = jade_u2f(S.env_alias[t].z);
    word = t | EMI_HEMI;
  }
  // m = (1 / 2 pi) / (p_sky / 2 + p_hemi / 2), p_sky = q / (2 pi^2 s), p_hemi = 1 / 2 pi or c / pi
  const float ps = (float)JADE_PI_D * s;
  const float c = jade_fabs(jv_dot(n, w)) / jade_sqrt(nn);
  *m = (2.0f * ps) / (axis ? q + (2.0f * ps) * c : q + ps);
  *info = word;
  return w;
}
// ... with five successive jade_rand draws: what bounce_branch calls
template <bool COSINE>
static __device__ __forceinline__ jvec3 env_mix_sample(const DevScene& S, uint32_t* rng, jvec3 n, float side, float* m, uint32_t* info) {
  return env_mix_sample_with<COSINE>(S, [rng]() { return jade_rand(rng); }, n, side, m, info);
}
// ... and with five given numbers
template <bool COSINE>
static __device__ __forceinline__ jvec3 env_mix_sample_at(const DevScene& S, const float* u5, jvec3 n, float side, float* m, uint32_t* info) {
  int k = 0;
  return env_mix_sample_with<COSINE>(S, [u5, &k]() { return u5[k++]; }, n, side, m, info);
}

// Multiple importance sampling of the emitters (jade_scene_set_direct_sampling = JADE_DIRECT_MIS; NOT the reference's estimator), as
// include/jade_bvh.h states it ("The direct light, stated"): the balance heuristic between a uniform point of emitter triangle h (density
// PL = mu * pA per solid angle) and the cosine bounce (pB), from ONE vector l - vertex to a point of h - on both sides.  n: the vertex's
// stored normal; ne, A: h's stored normal and tri_size; (m, mu): h's row of the table (mis_table, jade_scene_prep.hip; mu = m with all
// lights, M with one).  *w_L: what an emitter term towards h is multiplied with; *g_B: the scalar factor of the bounce term,
// T_B = Le f g_B / RR.  h not weighted (m not > 0), or a normal that gives the cosine draw no axis: w_L = 1, g_B = 0.
static __device__ __forceinline__ void mis_terms(jvec3 n, jvec3 ne, float A, float m, float mu, jvec3 l, float* w_L, float* g_B) {
  const float nn = jv_dot(n, n);
  if (!(m > 0) || !(nn > 0 && nn < jade_u2f(0x7f800000u))) {
    *w_L = 1.0f;
    *g_B = 0.0f;
    return;
  }
  const float ll = jv_dot(l, l), rl = jade_sqrt(ll), sne = jade_sqrt(jv_dot(ne, ne));
  const float nl = jade_fabs(jv_dot(n, l));
  const float pA = ll * rl * sne / (A * jade_fabs(jv_dot(ne, l)));
  const float PL = mu * pA;
  const float pB = nl / (rl * jade_sqrt(nn) * (float)JADE_PI_D);
  *w_L = 1.0f / (1.0f + pB / PL);  // (PL = inf: 1; no inf / inf for l.l > 0)
  *g_B = m * (nl / rl) * sne / (PL + pB);
}

static __device__ __forceinline__ jvec3 tri_point(const jade_triangle* t, float rx, float ry) {
  jvec3 p1 = V3(t->p1);
  return jv_add(jv_add(p1, jv_scale(jv_sub(V3(t->p2), p1), rx)), jv_scale(jv_sub(V3(t->p3), p1), ry));
}

static __device__ __forceinline__ float tri_size(const jade_triangle* t) {  // PathTrace.cu:897-903
  jvec3 cp = jv_cross(jv_sub(V3(t->p2), V3(t->p1)), jv_sub(V3(t->p3), V3(t->p1)));
  return 0.5f * jade_sqrt(jv_dot(cp, cp));
}

// The LIMIT a shadow ray carries to k_trace (jade_device.h, PathState.early_exit): hitTriangle (PathTrace.cu:705-754) of the ray
// with the emitter it aims at, statement for statement as the walk's own test evaluates it (jade_trace.h pair_core / tri_hit: the
// same helpers, so the same bits - test_gpu_early_exit.py compares them) - the distance if HitResult.isHit and hitArray would
// record it (distance < INF, :787), else JADE_INF_F: hitBVH can then not return this emitter, and any hit settles the query.
// The caller's use of the query (:957, 1097, 1293) is "isHit && index == emitter": true iff no triangle of the walk is recorded
// before the emitter with a distance <= its own, so a recorded hit STRICTLY nearer than this value makes it false for good.
static __device__ float shadow_limit(const jade_triangle* t, jvec3 o, jvec3 d) {
  const jvec3 p1 = V3(t->p1), p2 = V3(t->p2), p3 = V3(t->p3);
  const jvec3 dn = jv_normalize(d);
  const jvec3 sa = jv_sub(p1, jv_scale(dn, jv_dot(dn, jv_sub(p1, o))));
  const jvec3 sb = jv_sub(p2, jv_scale(dn, jv_dot(dn, jv_sub(p2, o))));
  const jvec3 sc = jv_sub(p3, jv_scale(dn, jv_dot(dn, jv_sub(p3, o))));
  const jvec3 pa = jv_sub(sa, o), pb = jv_sub(sb, o), pc = jv_sub(sc, o);
  const float papb = jv_mixed(dn, pa, pb), pbpc = jv_mixed(dn, pb, pc), pcpa = jv_mixed(dn, pc, pa);
  if (!((papb > 0 && pbpc > 0 && pcpa > 0) || (papb < 0 && pbpc < 0 && pcpa < 0))) return JADE_INF_F;
  const jvec3 eb = jv_sub(sb, sa), ec = jv_sub(sc, sa), q = jv_sub(o, sa);
  const float divider = jade_diffprod(eb.x, ec.y, eb.y, ec.x);
  const float rate_a = jade_diffprod(ec.y, q.x, ec.x, q.y) / divider;
  const float rate_b = jade_fma(eb.x, q.y, (-eb.y) * q.x) / divider;
  const jvec3 P = jv_add(jv_add(p1, jv_scale(jv_sub(p2, p1), rate_a)), jv_scale(jv_sub(p3, p1), rate_b));
  const float distance = jv_dot(jv_sub(P, o), dn);
  return (distance > 0 && distance < JADE_INF_F) ? distance : JADE_INF_F;
}

// a triangle as shading sees it: its flat normal and its object's material (jade_device.h, DevMaterial)
struct ShadeTri {
  jvec3 norm;
  const DevMaterial* m;
};
static __device__ __forceinline__ ShadeTri shade_tri(const DevScene& S, int idx) {
  const float4 v = S.tnorm[idx];
  ShadeTri t;
  t.norm = jv(v.x, v.y, v.z);
  t.m = S.mats + __float_as_uint(v.w);
  return t;
}

static __device__ __forceinline__ bool nonemissive(const DevMaterial* t) {
  return t->emissive[0] < 1.5e-4f && t->emissive[1] < 1.5e-4f && t->emissive[2] < 1.5e-4f;
}

static __device__ __forceinline__ float schlick_out(float R0, float cosine_abs) {  // "R0 - (1-R0)(...)^5", :1102
  float one_cosine_o = 1 - cosine_abs;
  float one_cosine_o_sqr = one_cosine_o * one_cosine_o;
  return R0 - (1 - R0) * one_cosine_o_sqr * one_cosine_o_sqr * one_cosine_o;
}

// gen_refract_ray, PathTrace.cu:876-894
static __device__ jvec3 gen_refract_ray(jvec3 direction_in, jvec3 normal_line, float eta, bool* full_reflex) {
  float cosi = jv_dot(direction_in, normal_line);
  if (cosi > 0) normal_line = jv_neg(normal_line);
  else cosi *= -1;
  float cost2 = 1.0f - eta * eta * (1.0f - cosi * cosi);
  if (cost2 > 0) {
    *full_reflex = false;
    return jv_add(jv_scale(direction_in, eta), jv_scale(normal_line, eta * cosi - jade_sqrt(cost2)));
  }
  *full_reflex = true;
  return direction_in;
}

// One lane's view of its pixel record.
struct Px {
  const PathState& P;
  int p;
  __device__ Px(const PathState& ps, int pix) : P(ps), p(pix) {}
  // the record's ray slots: one float4 per slot, side by side per record; one hit point per record (jade_device.h)
  __device__ float4* slot(int k) const { return P.slot + ((size_t)p * P.nslots + k); }
  __device__ jvec3 dir(int k) const {
    const float4 v = slot(k)[0];
    return jv(v.x, v.y, v.z);
  }
  __device__ void set_dir(int k, jvec3 v) const {
    float* f = reinterpret_cast<float*>(slot(k));
    f[0] = v.x; f[1] = v.y; f[2] = v.z;
  }
  __device__ jvec3 hpt(int k) const {  // (k: the slot of the record's one ray whose nearest hit was wanted - the caller knows which)
    (void)k;
    const float4 v = P.hitp[p];
    return jv(v.x, v.y, v.z);
  }
  __device__ int hit(int k) const { return reinterpret_cast<const int*>(slot(k))[3]; }
  __device__ void set_hit(int k, int v) const { reinterpret_cast<int*>(slot(k))[3] = v; }
  __device__ void set_limit(int k, float v) const { reinterpret_cast<float*>(slot(k))[3] = v; }  // a queued ray that may end early (jade_device.h)
  // origin shared by the record's pending rays + the triangle they leave: one float4
  __device__ void set_origin(jvec3 o, int skip) const { P.orgs[p] = make_float4(o.x, o.y, o.z, __int_as_float(skip)); }
  __device__ jvec3 origin() const {
    const float4 v = P.orgs[p];
    return jv(v.x, v.y, v.z);
  }
  __device__ int skip() const { return reinterpret_cast<const int*>(P.orgs + p)[3]; }
  // aux / auxi of the path (jade_device.h, PathState.aux): a float4 of their own, touched by the BSSRDF and refraction stages only
  __device__ jvec3 aux() const {
    const float4 v = P.aux[p];
    return jv(v.x, v.y, v.z);
  }
  __device__ void set_aux(jvec3 v) const {
    float* f = reinterpret_cast<float*>(P.aux + p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z;
  }
  __device__ int auxi() const { return reinterpret_cast<const int*>(P.aux + p)[3]; }
  __device__ void set_auxi(int v) const { reinterpret_cast<int*>(P.aux + p)[3] = v; }
};

// The same view held in registers: k_light traces a record's single ray (camera or mirror) in the kernel that shades
// it, so the ray and its result never travel through memory.  Slot 0 only.
struct RegPx {
  jvec3 d, o, hp;
  int h, sk;
  __device__ jvec3 dir(int) const { return d; }
  __device__ void set_dir(int, jvec3 v) { d = v; }
  __device__ jvec3 hpt(int) const { return hp; }
  __device__ int hit(int) const { return h; }
  __device__ void set_hit(int, int v) { h = v; }
  __device__ void set_origin(jvec3 org, int skip) {
    o = org;
    sk = skip;
  }
};

struct ShadeCtx {
  uint32_t rng;
  uint32_t stage, depth, flags;
  jvec3 thr, acc, le;
  int32_t obj;
  jvec3 src, out;
  // what this pass emits
  int n_emit_rays;  // number of active slots written
  // counters
  uint32_t c_primary, c_shadow, c_shaded, c_samples;
  uint32_t c_cls;  // rays emitted by call site, one byte each: env | indirect << 8 | mirror << 16 | refract << 24 (a record emits once per pass)
};

// ---- The passes (include/jade_bvh.h, "The passes, stated"; the kernels of a mode with SM_PASSES only, jade_runtime.h): beside its frame a
// render keeps every addend of a sample's colour in the pass of the statement that formed it.  Nothing of it rides in ShadeCtx or
// PathState - no other kernel's arguments or registers move: the planes come as an argument of their own, and consume hands the parts
// of a sampling vertex's l_dir to shade_record through PassParts.
//   cur[pass][p]  float4   the parts of record p's sample in flight (.w unused); meaningful only where bit `pass` of mask[p] is set, so
//                          that dropping a sample's parts (CONSUME_ZERO) and starting the next one is mask[p] = 0 and touches no plane
//   tot[pass][p]  3 floats the finished samples of record p: += cur when a sample ends, in the order the samples end
//   mask[p]                the passes record p's sample in flight has touched
// [pass][p]: a wave's neighbouring records touch neighbouring addresses.  Only record p touches its entries: no race, no atomics, the
// same bits every time.  k_passes_resolve (jade_passes.hip) adds a pixel's records in ascending order.
enum { PASS_BACKGROUND = 0, PASS_EMISSION = 1, PASS_SPECULAR_SKY = 2, PASS_SAMPLED = 3, PASS_COUNT = 15 };
struct PassPlanes {
  float4* cur;
  float* tot;
  uint32_t* mask;
  uint32_t npix;
};
// What the kernels of mode M take beyond the parity kernels' arguments, in one piece: a by-value kernel argument, the last (k_shade_mode, which says why SM_MIS is
// the exception; k_shade_lean_mode; mode_args, jade_hip.hip).  A member is there only in the modes that take it - in the others its base is the empty one, which takes
// no space and whose accessor answers nullptr, so shade_record is one text - in this order: the pass planes under SM_PASSES; the shutter's constants under SM_SHUTTER; the
// alias table over the scene's emitter entries under SM_LIGHTS, SM_COSINE or SM_MIS (read under SM_LIGHTS only); the per-triangle table {m, M} under SM_MIS; the
// vertex-normal records under SM_SMOOTH - and under SM_TEX, which is raised with it, those together with the texture tables; under SM_NMAP, raised
// with both, all of those together with the normal map's.
struct ArgPlanes { PassPlanes planes; __device__ const PassPlanes* L() const { return &planes; } };
struct NoPlanes { __device__ const PassPlanes* L() const { return nullptr; } };
struct ArgShutter { ShutterConst shutter; __device__ const ShutterConst* H() const { return &shutter; } };
struct NoShutter { __device__ const ShutterConst* H() const { return nullptr; } };
struct ArgLights { const uint4* light_table; __device__ const uint4* lights() const { return light_table; } };
struct NoLights { __device__ const uint4* lights() const { return nullptr; } };
struct ArgMis { const float2* mis_table; __device__ const float2* mis() const { return mis_table; } };
struct NoMis { __device__ const float2* mis() const { return nullptr; } };
struct ArgSmooth { const float4* smooth_table; __device__ const float4* smooth() const { return smooth_table; } };  // SM_SMOOTH: the vertex-normal records (jade_smooth.h)
struct NoSmooth { __device__ const float4* smooth() const { return nullptr; } };
struct ArgTextures { TexTables tex_tables; __device__ const TexTables& smooth() const { return tex_tables; } };  // SM_TEX: the smooth family's table, with the textures (jade_texture.h)
struct ArgNormalMaps { MapTables map_tables; __device__ const MapTables& smooth() const { return map_tables; } };  // SM_NMAP: the textured family's tables, with the normal map (jade_normal_map.h)
template <uint32_t M>
struct ShadeArgs : std::conditional_t<sm(M, SM_PASSES), ArgPlanes, NoPlanes>, std::conditional_t<sm(M, SM_SHUTTER), ArgShutter, NoShutter>,
                   std::conditional_t<(M & (SM_LIGHTS | SM_COSINE | SM_MIS)) != 0, ArgLights, NoLights>, std::conditional_t<sm(M, SM_MIS), ArgMis, NoMis>,
                   std::conditional_t<sm(M, SM_NMAP), ArgNormalMaps, std::conditional_t<sm(M, SM_TEX), ArgTextures, std::conditional_t<sm(M, SM_SMOOTH), ArgSmooth, NoSmooth>>> {};
static __device__ const ShadeArgs<0> SHADE_ARGS_NONE{};  // what mode 0 passes, by name: with a temporary on the caller's stack k_shade_lean and k_tail come out in another order
// What consume / consume_mirror tell shade_record about the vertex they folded: cls < 0 - nothing to book (l_final is 0);
// PASS_EMISSION / PASS_SPECULAR_SKY - *l_final is that pass's (e holds it); otherwise 3 + 4 kind + depth, the vertex's emitter pass, its sky
// pass two above: e and s are the two parts of l_dir, each with the branch's scale, thr0 the throughput before the vertex's push.
struct PassParts {
  jvec3 e, s, thr0;
  int cls;
  bool pushed;
};
static __device__ __forceinline__ void pass_add(const PassPlanes& L, int p, uint32_t& mask, int pass, jvec3 v) {
  if (!(v.x != 0 || v.y != 0 || v.z != 0)) return;  // adding 0 changes no sum (a NaN is not 0: it is booked)
  float4* c = L.cur + ((size_t)pass * L.npix + (size_t)p);
  if ((mask >> pass) & 1u) {
    const float4 o = *c;
    v = jv_add(jv(o.x, o.y, o.z), v);
  }
  *c = make_float4(v.x, v.y, v.z, 0.0f);
  mask |= 1u << pass;
}
// the sample of record p ended: its parts go to the record's totals
static __device__ __forceinline__ void pass_commit(const PassPlanes& L, int p, uint32_t& mask) {
  for (uint32_t m = mask; m; m &= m - 1u) {
    const size_t i = (size_t)(__ffs(m) - 1) * L.npix + (size_t)p;
    const float4 v = L.cur[i];
    float* t = L.tot + 3 * i;
    t[0] += v.x;
    t[1] += v.y;
    t[2] += v.z;
  }
  mask = 0u;
}
// consume's / consume_mirror's outcome r (CONSUME_*, below) and parts, booked: a pushed vertex with the throughput before the push; the
// last l_dir of a path that ended with the throughput it ends with - after a 128th push the same vertex again (the reference's double
// count); CONSUME_ZERO drops what the sample has gathered.
static __device__ __forceinline__ void pass_fold(const PassPlanes& L, int p, uint32_t& mask, const PassParts& pp, jvec3 thr, bool ended, bool zero) {
  if (zero) {
    mask = 0u;
    return;
  }
  if (pp.cls < 0) return;
  if (pp.cls < PASS_SAMPLED) {
    if (ended) pass_add(L, p, mask, pp.cls, jv_mul(thr, pp.e));
    return;
  }
  if (pp.pushed) {
    pass_add(L, p, mask, pp.cls, jv_mul(pp.thr0, pp.e));
    pass_add(L, p, mask, pp.cls + 2, jv_mul(pp.thr0, pp.s));
  }
  if (ended) {
    pass_add(L, p, mask, pp.cls, jv_mul(thr, pp.e));
    pass_add(L, p, mask, pp.cls + 2, jv_mul(thr, pp.s));
  }
}

// ---- The record steps: how a sample begins, ends and parks.  One text each for shade_record and k_shade_binned (jade_hip.hip); the
// first-pass kernels (jade_light.h) call vertex_from_primary and store_ctx and keep their own text of the other steps, statement for
// statement these (their instructions answer any change of their text: see there).  The film point and the pinhole direction of a
// camera ray are jade_device.h's film_point / pinhole_dir, which the denoiser's guide pass shares.

// Record p has finished `done` samples: which sample comes next and for which owned pixel.
struct NextSample {
  uint32_t sidx;  // global sample index (jade_rt.h)
  int pixel;      // owned-pixel index it belongs to
};
// (m, home) = (p / npx, p % npx): where record p sits; computed once per thread, an integer division each.
// rpp and JADE_SAMPLE_LANES are powers of two, so everything else is shifts — and the 64-bit modulo of the
// pixel rotation only runs when rotation is on (it is not, by default).  A record of a tile that adaptive sampling has stopped carries
// the stop offset in `done` (PathState.hdr): its sidx is 2^31 above its last sample's, past any target.
static __device__ __forceinline__ NextSample next_sample_mh(const PathState& P, uint32_t m, uint32_t home, uint32_t done) {
  const uint32_t rpp_log2 = 31u - (uint32_t)__clz(P.rpp);
  const uint32_t per_log2 = (31u - (uint32_t)__clz(JADE_SAMPLE_LANES)) - rpp_log2;  // samples per record per block = LANES / rpp
  const uint32_t blk = done >> per_log2, n = done - (blk << per_log2);
  NextSample r;
  r.sidx = JADE_SAMPLE_LANES * blk + m + (n << rpp_log2);
  r.pixel = P.stride == 0 ? (int)home
                          : (int)(((unsigned long long)home + (unsigned long long)n * (uint32_t)P.stride) % (uint32_t)P.npx);
  return r;
}
static __device__ __forceinline__ NextSample next_sample(const PathState& P, int p, uint32_t done) {
  const uint32_t m = (uint32_t)p / (uint32_t)P.npx;
  return next_sample_mh(P, m, (uint32_t)p - m * (uint32_t)P.npx, done);
}
static __device__ __forceinline__ bool pixel_xy_t(const RenderConst& R, int tid, int pixel, int* x, int* y) {
  int l = pixel & 255;
  *x = (tid % R.tiles_x) * JADE_TILE_SIZE + (l & 15);
  *y = (tid / R.tiles_x) * JADE_TILE_SIZE + (l >> 4);
  return *x < R.width && *y < R.height;
}
static __device__ __forceinline__ bool pixel_xy(const RenderConst& R, const int32_t* tile_ids, int pixel, int* x, int* y) {
  return pixel_xy_t(R, tile_ids[pixel >> 8], pixel, x, y);
}

// The next live sample of the record (rec_m, home_pix; tid0: its home pixel's tile): samples of out-of-image pixels (edge tiles) are skipped,
// `done` counted past them.  False: nothing is left for this record below target_spp.  Otherwise *sidx is the sample, (*x, *y) its pixel.
static __device__ __forceinline__ bool next_live_sample(const PathState& P, const RenderConst& R, const int32_t* tile_ids, uint32_t target_spp,
                                                        uint32_t rec_m, int home_pix, int tid0, uint32_t& done, uint32_t* sidx, int* x, int* y) {
  NextSample ns = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
  while (ns.sidx < target_spp && !pixel_xy_t(R, ns.pixel == home_pix ? tid0 : tile_ids[ns.pixel >> 8], ns.pixel, x, y)) {
    done += 1;
    ns = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);
  }
  *sidx = ns.sidx;
  return ns.sidx < target_spp;
}
// A sample of the record ended with `color`: final_result = final_result + color (PathTrace.cu:1454), into the partial sum of this
// sample's (pixel, lane) - only this record touches it in this pass
static __device__ __forceinline__ void add_sample(const PathState& P, uint32_t rec_m, int home_pix, uint32_t& done, ShadeCtx& c, const jvec3& color) {
  const NextSample cs = next_sample_mh(P, rec_m, (uint32_t)home_pix, done);  // the sample that just ended
  const size_t si = (size_t)(cs.sidx % JADE_SAMPLE_LANES) * (size_t)P.npx + (size_t)cs.pixel;
  const size_t sn = (size_t)P.sum_lanes * (size_t)P.npx;
  st3w(P.sum, sn, si, jv_add(ld3w(P.sum, sn, si), color));
  done += 1;
  c.c_samples += 1;
}
// The path context of record p, for a record on a path or parked at a vertex.  Stored and loaded by need (shade_record): before the first
// path_push thr is 1 and acc 0, and a mirror ray in flight needs neither the vertex it left nor, at depth 0, a stored Le.
// (aux and auxi - P.aux - are begin_bounce's and consume's: written through Px while the record was shaded)
static __device__ __forceinline__ void store_ctx(const PathState& P, int p, const ShadeCtx& c) {
  float4* cx = P.ctx + (size_t)p * 4;
  cx[0] = make_float4(c.thr.x, c.thr.y, c.thr.z, __int_as_float(c.obj));
  cx[1] = make_float4(c.acc.x, c.acc.y, c.acc.z, c.out.z);
  cx[2] = make_float4(c.le.x, c.le.y, c.le.z, c.src.x);
  cx[3] = make_float4(c.src.y, c.src.z, c.out.x, c.out.y);
}
// A camera ray with direction d met triangle `hit` at hp: the first vertex of a path
static __device__ __forceinline__ void vertex_from_primary(const DevScene& S, ShadeCtx& c, int hit, const jvec3& hp, const jvec3& d) {
  c.le = V3(shade_tri(S, hit).m->emissive);
  c.thr = jv(1, 1, 1);
  c.acc = jv(0, 0, 0);
  c.depth = 0;
  c.obj = hit;
  c.src = hp;
  c.out = jv_neg(d);
}
// The secondary rays a record emitted this pass (st: its stage after it), by hitBVH call site (jade_rt.h)
static __device__ __forceinline__ void count_secondary(ShadeCtx& c, uint32_t st) {
  if (st == ST_PRIMARY || !c.n_emit_rays) return;
  if (st == ST_DIFFUSE || st == ST_BSSRDF) {
    const uint32_t ind = (c.flags & STF_RR) ? 1u : 0u;
    const uint32_t env = (c.flags & STF_NOENV) ? 0u : 1u;  // one environment ray always (env_sampling: unless its direction lay on the wrong side)
    c.c_cls += env | (ind << 8);  // ... and the indirect ray if the roulette passed
    c.c_shadow += (uint32_t)c.n_emit_rays - env - ind;
  } else {
    c.c_cls += st == ST_MIRROR ? (1u << 16) : (1u << 24);
  }
}

// push (dir, rate) — forward form of stack_dir / stack_indir_rate.  Returns
// true when the reference's `while (stack_offset < STACK_CAPACITY)` would stop.
static __device__ __forceinline__ bool path_push(ShadeCtx& c, jvec3 dirv, jvec3 rate) {
  c.acc = jv_add(c.acc, jv_mul(c.thr, dirv));
  c.thr = jv_mul(c.thr, rate);
  c.depth += 1;
  return c.depth >= JADE_STACK_CAPACITY;
}

// The mirror branch of the bounce loop (PathTrace.cu:1365-1405): RR, then the reflected ray.
// Shared by the full shading kernel and the lean one (k_shade<true>).
template <class PX>
static __device__ __forceinline__ bool bounce_mirror(PX& px, ShadeCtx& c, const DevMaterial* ot, jvec3 obj_emissive, jvec3 n,
                                                     jvec3* l_final) {
  const float RR_F = (float)JADE_RR_RATE_D;
  jvec3 obj_hit_fr = jv_scale(V3(ot->brdf), (float)(1.0 / JADE_PI_D));
  int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  if (obj_emissive.x > 1.5e-4f || obj_emissive.y > 1.5e-4f || obj_emissive.x > 1.5e-4f) {
    *l_final = jv_scale(jv_mul(obj_emissive, obj_hit_fr), (float)k);
    return false;
  }
  float rr_result = jade_rand(&c.rng);
  if (!(rr_result < RR_F)) return false;
  jvec3 refl = jv_sub(jv_scale(n, 2 * jv_dot(c.out, n)), c.out);
  px.set_origin(c.src, c.obj);
  px.set_dir(0, refl);
  px.set_hit(0, -1);
  c.n_emit_rays++;
  c.stage = ST_MIRROR;
  c.flags = 0;
  return true;
}

// What the lean kernel may shade at a vertex: an emitter (the loop's first test ends the path) or a
// pure mirror (no refraction branch, not diffuse).  Everything else needs the full kernel.
static __device__ __forceinline__ bool lean_can_shade(const DevMaterial* ot) {
  if (ot->emissive[0] > 1.4e-5f || ot->emissive[1] > 1.4e-5f || ot->emissive[2] > 1.4e-5f) return true;
  return ot->refract_mode == JADE_NO_REFRACT && ot->reflex_mode != JADE_DIFFUSE;
}

// begin_bounce restricted to those two cases: the same statements in the same order
// (emissive test :916-920, the select draw :924, then the mirror branch).
template <class PX>
static __device__ bool begin_bounce_lean(const DevScene& S, PX& px, ShadeCtx& c, jvec3* l_final) {
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
  return bounce_mirror(px, c, ot, obj_emissive, ots.norm, l_final);
}

// Round 4: the bounce in two parts, so that k_shade can run the second one for records GROUPED BY BRANCH (bounce_classify by the
// thread that holds the record, bounce_branch by whichever thread of the block the record is dealt to; k_shade, jade_hip.hip).
// begin_bounce = the two in a row: the statements, and the order of the random draws, are the ones they always were.
enum { BT_END = 0, BT_MIRROR, BT_DIFFUSE, BT_BSSRDF, BT_REFRACT, BT_N };
// The head of the bounce: the emissive test (PathTrace.cu:916-920; BT_END: *l_final = the emission), then the draws that choose
// the branch (:924-930).  BT_DIFFUSE covers the diffuse and the SSS-diffuse branch: stage and flags are set here.
static __device__ __forceinline__ int bounce_classify(const DevScene& S, ShadeCtx& c, jvec3* l_final) {
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  c.c_shaded += 1;
  jvec3 obj_emissive = V3(ot->emissive);
  if (obj_emissive.x > 1.4e-5f || obj_emissive.y > 1.4e-5f || obj_emissive.z > 1.4e-5f) {
    *l_final = obj_emissive;  // PathTrace.cu:916-920
    return BT_END;
  }
  *l_final = jv(0, 0, 0);
  float select_reflex_refract = jade_rand(&c.rng);
  if (select_reflex_refract < 0.5f && ot->refract_mode != JADE_NO_REFRACT) {
    if (ot->refract_mode == JADE_SUB_SURFACE) {
      select_reflex_refract = jade_rand(&c.rng);
      if (select_reflex_refract < (float)JADE_SSS_RATE_D) {
        c.stage = ST_DIFFUSE;
        c.flags = STF_SSS;
        return BT_DIFFUSE;
      }
      return BT_BSSRDF;
    }
    return BT_REFRACT;
  }
  if (ot->reflex_mode == JADE_DIFFUSE) {
    c.stage = ST_DIFFUSE;
    c.flags = 0;
    return BT_DIFFUSE;
  }
  return BT_MIRROR;
}
// The BSSRDF branch's search for the exit triangle (PathTrace.cu:1031-1048), on the draw u_area of [0, 1]: the LAST midpoint the
// reference's bisection of object obj_idx's prefix areas looks at, before S.mapping (bounce_branch draws u_area and maps the result;
// libjade_hip_debug.so's jade_debug_exit_search runs this function alone, row by row, tests/test_gpu_area_search.py).
static __device__ __forceinline__ int exit_search(const DevScene& S, int obj_idx, float u_area) {
  const jade_obj_seg seg = S.segs[obj_idx];
  float random_idx = u_area * S.prefix[seg.end_idx];
  int left = seg.begin_idx, right = seg.end_idx, middle = 0;
  const uint2 gd = S.guide_obj[obj_idx];
  if (gd.y != 0u) {
    // The reference bisects prefix[] (:1031-1048): ~17 DEPENDENT loads, the longest latency chain of this kernel, and what
    // it returns is not the boundary but the LAST midpoint it looked at.  Both are reproduced without the chain: the
    // boundary b = the first i with random_idx <= prefix[i] comes from a guide table (jade_scene_create: prefix is
    // checked to be finite and non-decreasing, so "random_idx <= prefix[mid]" is "mid >= b"; the cell's bounds hold
    // because rounding is monotone: c / Gn <= u implies fl(c / Gn * A) <= fl(u * A)), then the bisection is replayed
    // on indices alone.
    const uint32_t cell = (uint32_t)(u_area * (float)gd.y);  // u in [0, 1], Gn a power of two: exact
    const uint32_t* gp = S.guide + gd.x + cell;
    const uint32_t b_hi = gp[1];
    uint32_t b = gp[0];
    while (b < b_hi && !(random_idx <= S.prefix[b])) ++b;
    while (left < right - 1) {
      middle = (left + right) / 2;
      if ((uint32_t)middle >= b) right = middle;
      else left = middle;
    }
  } else {
    while (left < right - 1) {
      middle = (left + right) / 2;
      float pm = S.prefix[middle];
      if (random_idx <= pm) right = middle;
      else if (random_idx >= pm) left = middle;
      else break;
    }
  }
  return middle;
}

// The branch itself: its draws, its rays (written through px), stage / flags / n_emit_rays.  Returns false if the path ended at
// this vertex (*l_final holds the last l_dir).  `type` is uniform over the waves k_shade runs it for.
// M: the render's mode (ShadeMode, jade_runtime.h); each bit's code is compiled apart: the parity kernels (M = 0) carry none.  SM_ENVIS: JADE_ENV_IMPORTANCE (include/jade_rt.h)
// SM_LIGHTS: JADE_LIGHTS_ONE (include/jade_bvh.h): ONE entry of S.emit, drawn from `lights`, in slot 0; nL = the shadow slots of the
// record's layout, so the environment ray sits in slot nL and the indirect ray in slot nL + 1.  *light = the entry drawn: it travels with
// the record (the fourth word of PathState.hdr, shade_record) to consume.
// SM_COSINE: JADE_BOUNCE_COSINE (include/jade_bvh.h, "The bounce, stated"): the environment ray - unless SM_ENVIS draws it - and the
// indirect ray come from cosine_dir_rng in place of sphere_dir and its flip, on the same two draws.
// SM_ENVMIX: JADE_ENV_MIXTURE (include/jade_rt.h; with SM_ENVIS only): where SM_ENVIS calls env_sample this calls env_mix_sample - five
// draws, the sky technique or the bounce sampling's own direction - and m travels where ratio does.
template <uint32_t M = 0>
static __device__ __forceinline__ bool bounce_branch(int type, const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final,
                                                     const uint4* lights = nullptr, uint32_t* light = nullptr) {
  constexpr bool ENVIS = sm(M, SM_ENVIS), LIGHTS = sm(M, SM_LIGHTS), COSINE = sm(M, SM_COSINE), ENVMIX = sm(M, SM_ENVMIX);
  const jade_triangle* T = S.tris;  // vertices only
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  const int nE = S.n_emit;
  const int nL = LIGHTS ? (nE > 0 ? 1 : 0) : nE;
  const float RR_F = (float)JADE_RR_RATE_D;
  const jvec3 n = ots.norm;
  *l_final = jv(0, 0, 0);  // (as bounce_classify left it: a worker thread of k_shade brings its own)
  if (type == BT_DIFFUSE) goto diffuse_like;
  if (type == BT_MIRROR) return bounce_mirror(px, c, ot, V3(ot->emissive), n, l_final);  // ---- mirror, PathTrace.cu:1365-1405 ----
  if (type == BT_BSSRDF) {
    {
      // ---- BSSRDF, PathTrace.cu:1029-1178 ----
      int middle = S.mapping[exit_search(S, ot->obj_idx, jade_rand(&c.rng))];
      float rand_x = jade_rand(&c.rng);
      float rand_y = jade_rand(&c.rng);
      if (rand_x + rand_y > 1) {
        rand_x = 1 - rand_x;
        rand_y = 1 - rand_y;
      }
      const ShadeTri t_is = shade_tri(S, middle);
      const DevMaterial* t_i = t_is.m;
      const jvec3 t_norm = t_is.norm;
      const jvec3 rate = V3(t_i->refract_rate);
      jvec3 random_point = tri_point(&T[middle], rand_x, rand_y);
      jvec3 inner_direction = jv_sub(random_point, c.src);
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
      for (int i = 0; i < nL; ++i) {
        float rx, ry;
        int ei = i;
        if (LIGHTS) {
          *light = light_sample(lights, (uint32_t)nE, &c.rng, &rx, &ry);
          ei = (int)*light;
        } else {
          rx = jade_rand(&c.rng);
          ry = jade_rand(&c.rng);
          if (rx + ry > 1) {
            rx = 1 - rx;
            ry = 1 - ry;
          }
        }
        const jade_triangle* et = &T[S.emit[ei]];
        jvec3 random_emit_point = tri_point(et, rx, ry);
        const jvec3 sd = jv_sub(random_emit_point, random_point);
        px.set_dir(i, sd);
        px.set_limit(i, shadow_limit(et, random_point, sd));
        c.n_emit_rays++;
      }
      uint32_t noenv = 0;
      if (ENVIS) {  // (non-parity mode: by importance; a direction on the wrong side contributes nothing and is not traced)
        float ratio;
        uint32_t mix = 0;
        const jvec3 ray_direction = ENVMIX ? env_mix_sample<COSINE>(S, &c.rng, t_norm, jv_dot(inner_direction, t_norm), &ratio, &mix) : env_sample(S, &c.rng, &ratio);
        if (ENVMIX ? (mix & EMI_WRONG) != 0 : jv_dot(ray_direction, t_norm) * jv_dot(inner_direction, t_norm) < 0) {
          px.set_hit(nL, -2);
          noenv = STF_NOENV;
        } else {
          px.set_dir(nL, ray_direction);
          px.set_limit(nL, JADE_INF_F);
          px.set_auxi(__float_as_int(ratio));
          c.n_emit_rays++;
        }
      } else {
        jvec3 ray_direction = COSINE ? cosine_dir_rng(&c.rng, t_norm, jv_dot(inner_direction, t_norm)) : sphere_dir(&c.rng);
        if (!COSINE && jv_dot(ray_direction, t_norm) * jv_dot(inner_direction, t_norm) < 0) ray_direction = jv_neg(ray_direction);
        px.set_dir(nL, ray_direction);
        px.set_limit(nL, JADE_INF_F);  // environment visibility: any recorded hit
        c.n_emit_rays++;
      }
      // (COSINE: the opposite hemisphere, as the reference has it)
      jvec3 ray_direction = COSINE ? cosine_dir_rng(&c.rng, t_norm, -jv_dot(inner_direction, t_norm)) : sphere_dir(&c.rng);
      if (!COSINE && jv_dot(ray_direction, t_norm) * jv_dot(inner_direction, t_norm) > 0) ray_direction = jv_neg(ray_direction);
      float rr_result = jade_rand(&c.rng);
      c.stage = ST_BSSRDF;
      c.flags = noenv;
      if (rr_result < RR_F) {
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
  // ---- direct refraction entry, PathTrace.cu:1180-1199 ----
  {
    {
      float triangle_miu = ot->refract_index;
      float R0 = (1 - triangle_miu) / (1 + triangle_miu) * (1 - triangle_miu) / (1 + triangle_miu);
      float one_cosine_i = 1 - jade_fabs(jv_dot(n, c.out));
      float one_cosine_i_sqr = one_cosine_i * one_cosine_i;
      float fresnel_rate_i = R0 + (1 - R0) * one_cosine_i_sqr * one_cosine_i_sqr * one_cosine_i;
      bool full_reflex = false;
      jvec3 rev_out_direction = jv_scale(c.out, -1.0f);
      jvec3 refract_ray = gen_refract_ray(rev_out_direction, n, (float)(1.0 / (double)triangle_miu), &full_reflex);
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
  // ---- diffuse (:1266-1364) and SSS-diffuse (:931-1028): same ray set ----
  {
    px.set_origin(c.src, c.obj);
    const float side = jv_dot(c.out, n);
    for (int i = 0; i < nL; ++i) {
      float rand_x, rand_y;
      int ei = i;
      if (LIGHTS) {
        *light = light_sample(lights, (uint32_t)nE, &c.rng, &rand_x, &rand_y);
        ei = (int)*light;
      } else {
        rand_x = jade_rand(&c.rng);
        rand_y = jade_rand(&c.rng);
        if (rand_x + rand_y > 1) {
          rand_x = 1 - rand_x;
          rand_y = 1 - rand_y;
        }
      }
      const jade_triangle* et = &T[S.emit[ei]];
      jvec3 random_point = tri_point(et, rand_x, rand_y);
      jvec3 obj_light_direction = jv_sub(random_point, c.src);
      px.set_dir(i, obj_light_direction);
      if (jv_dot(obj_light_direction, n) * side < 0) {
        px.set_hit(i, -2);  // `continue`: no shadow ray
      } else {
        px.set_limit(i, shadow_limit(et, c.src, obj_light_direction));
        c.n_emit_rays++;
      }
    }
    if (ENVIS) {  // (non-parity mode, as in the BSSRDF branch)
      float ratio;
      uint32_t mix = 0;
      const jvec3 ray_direction = ENVMIX ? env_mix_sample<COSINE>(S, &c.rng, n, side, &ratio, &mix) : env_sample(S, &c.rng, &ratio);
      if (ENVMIX ? (mix & EMI_WRONG) != 0 : jv_dot(ray_direction, n) * side < 0) {
        px.set_hit(nL, -2);
        c.flags |= STF_NOENV;
      } else {
        px.set_dir(nL, ray_direction);
        px.set_limit(nL, JADE_INF_F);
        px.set_auxi(__float_as_int(ratio));
        c.n_emit_rays++;
      }
    } else {
      jvec3 ray_direction = COSINE ? cosine_dir_rng(&c.rng, n, side) : sphere_dir(&c.rng);
      if (!COSINE && jv_dot(ray_direction, n) * side < 0) ray_direction = jv_neg(ray_direction);
      px.set_dir(nL, ray_direction);
      px.set_limit(nL, JADE_INF_F);  // environment visibility: any recorded hit
      c.n_emit_rays++;
    }
    float rr_result = jade_rand(&c.rng);
    if (rr_result < RR_F) {
      jvec3 ray_direction = COSINE ? cosine_dir_rng(&c.rng, n, side) : sphere_dir(&c.rng);
      if (!COSINE && jv_dot(ray_direction, n) * side < 0) ray_direction = jv_neg(ray_direction);
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

// Sample the bounce at the current vertex and emit its rays.  Returns false
// if the path ended at this vertex (l_final holds the last l_dir).
template <uint32_t M = 0>
static __device__ bool begin_bounce(const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final, const uint4* lights = nullptr,
                                    uint32_t* light = nullptr) {
  const int type = bounce_classify(S, c, l_final);
  if (type == BT_END) return false;
  return bounce_branch<M>(type, S, px, c, l_final, lights, light);
}

// ---- The branch draws (include/jade_bvh.h, "The branch draws, stated"; the kernels of a mode with SM_BRANCH only, jade_runtime.h): at a
// vertex of depth 0 or 1 the draws that choose the arm - the select, the SSS select, the mirror's roulette - are read off one stratified
// number U of the sample instead of the stream, whose draws are made all the same and dropped.  Nothing of it rides in ShadeCtx or
// PathState: shade_record forms U from the record's `done` where it shades such a vertex.  The head of the bounce and its mirror arm
// stand here a second time, with U: the functions above are every other kernel's, k_light's and k_tail's among them, and one more
// argument or template parameter on them moves those kernels' registers (profiles/branch_kernel_resources.txt).
// A: the bit reversal (van der Corput, base 2); B: Sobol's second dimension; D: the pixel's shift for dimension d.  Host and device.
static __host__ __device__ __forceinline__ uint32_t branch_A(uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __brev(i);
#else
  i = (i >> 16) | (i << 16);
  i = ((i & 0xff00ff00u) >> 8) | ((i & 0x00ff00ffu) << 8);
  i = ((i & 0xf0f0f0f0u) >> 4) | ((i & 0x0f0f0f0fu) << 4);
  i = ((i & 0xccccccccu) >> 2) | ((i & 0x33333333u) << 2);
  return ((i & 0xaaaaaaaau) >> 1) | ((i & 0x55555555u) << 1);
#endif
}
static __host__ __device__ __forceinline__ uint32_t branch_B(uint32_t i) {
  uint32_t r = 0u;
  for (uint32_t v = 0x80000000u; i; i >>= 1, v ^= v >> 1)
    if (i & 1u) r ^= v;
  return r;
}
static __host__ __device__ __forceinline__ uint32_t branch_D(uint32_t x, uint32_t y, uint32_t frame, uint32_t d) {
  uint32_t s = jade_rng_seed(x, y, frame) ^ (d == 0u ? 0x68E31DA4u : 0xB5297A4Du);
  (void)jade_wang(&s);
  return jade_wang(&s);
}
// U of sample sidx of pixel (x, y) at a vertex of depth 0 or 1 (R.frame: the render's, not the sample's)
static __host__ __device__ __forceinline__ uint32_t branch_number(const RenderConst& R, int x, int y, uint32_t sidx, uint32_t depth) {
  return (depth == 0u ? branch_A(sidx) : branch_B(sidx)) ^ branch_D((uint32_t)x, (uint32_t)y, R.frame, depth);
}
// su: jade_rand's own conversion
static __host__ __device__ __forceinline__ float branch_su(uint32_t w) { return (float)w * 2.3283064365386963e-10f; }

// bounce_mirror with the roulette's number: u is U - or U << 1 on a material with a refraction arm, whose select spent a bit - at a
// vertex of depth < 2 (strat), the stream's draw otherwise; the stream's draw is made either way
template <class PX>
static __device__ __forceinline__ bool bounce_mirror_branch(PX& px, ShadeCtx& c, const DevMaterial* ot, jvec3 obj_emissive, jvec3 n, jvec3* l_final,
                                                            bool strat, uint32_t u) {
  const float RR_F = (float)JADE_RR_RATE_D;
  jvec3 obj_hit_fr = jv_scale(V3(ot->brdf), (float)(1.0 / JADE_PI_D));
  int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  if (obj_emissive.x > 1.5e-4f || obj_emissive.y > 1.5e-4f || obj_emissive.x > 1.5e-4f) {
    *l_final = jv_scale(jv_mul(obj_emissive, obj_hit_fr), (float)k);
    return false;
  }
  float rr_result = jade_rand(&c.rng);
  if (strat) rr_result = branch_su(k == 2 ? u << 1 : u);
  if (!(rr_result < RR_F)) return false;
  jvec3 refl = jv_sub(jv_scale(n, 2 * jv_dot(c.out, n)), c.out);
  px.set_origin(c.src, c.obj);
  px.set_dir(0, refl);
  px.set_hit(0, -1);
  c.n_emit_rays++;
  c.stage = ST_MIRROR;
  c.flags = 0;
  return true;
}
// begin_bounce_lean with U
template <class PX>
static __device__ bool begin_bounce_lean_branch(const DevScene& S, PX& px, ShadeCtx& c, jvec3* l_final, uint32_t u) {
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  c.c_shaded += 1;
  jvec3 obj_emissive = V3(ot->emissive);
  if (obj_emissive.x > 1.4e-5f || obj_emissive.y > 1.4e-5f || obj_emissive.z > 1.4e-5f) {
    *l_final = obj_emissive;
    return false;
  }
  *l_final = jv(0, 0, 0);
  (void)jade_rand(&c.rng);  // select_reflex_refract: made and dropped
  return bounce_mirror_branch(px, c, ot, obj_emissive, ots.norm, l_final, c.depth < 2u, u);
}
// begin_bounce with U: bounce_classify's statements with the two selects read off U and U << 1 at a vertex of depth < 2, then the mirror
// arm above or - every other arm draws from the stream alone - bounce_branch as it is
template <uint32_t M>
static __device__ bool begin_bounce_branch(const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final, const uint4* lights, uint32_t* light, uint32_t u) {
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  c.c_shaded += 1;
  jvec3 obj_emissive = V3(ot->emissive);
  if (obj_emissive.x > 1.4e-5f || obj_emissive.y > 1.4e-5f || obj_emissive.z > 1.4e-5f) {
    *l_final = obj_emissive;  // PathTrace.cu:916-920
    return false;
  }
  *l_final = jv(0, 0, 0);
  const bool strat = c.depth < 2u;
  int type = BT_MIRROR;
  float select_reflex_refract = jade_rand(&c.rng);
  if (strat) select_reflex_refract = branch_su(u);
  if (select_reflex_refract < 0.5f && ot->refract_mode != JADE_NO_REFRACT) {
    type = BT_REFRACT;
    if (ot->refract_mode == JADE_SUB_SURFACE) {
      select_reflex_refract = jade_rand(&c.rng);
      if (strat) select_reflex_refract = branch_su(u << 1);
      type = BT_BSSRDF;
      if (select_reflex_refract < (float)JADE_SSS_RATE_D) {
        c.stage = ST_DIFFUSE;
        c.flags = STF_SSS;
        type = BT_DIFFUSE;
      }
    }
  } else if (ot->reflex_mode == JADE_DIFFUSE) {
    c.stage = ST_DIFFUSE;
    c.flags = 0;
    type = BT_DIFFUSE;
  }
  if (type == BT_MIRROR) return bounce_mirror_branch(px, c, ot, obj_emissive, ots.norm, l_final, strat, u);
  return bounce_branch<M>(type, S, px, c, l_final, lights, light);
}

// Outcome of folding the pending rays' results into the path.
enum { CONSUME_VERTEX = 0, CONSUME_END = 1, CONSUME_ZERO = 2, CONSUME_EMITTED = 3 };

// Result of the mirror ray (PathTrace.cu:1383-1398).  Shared by both shading kernels.
// M: the render's mode; SM_PASSES: *pp says which pass *l_final belongs to (the sky at the end of a mirror chain), or that there is nothing to book
template <class PX, uint32_t M = 0>
static __device__ __forceinline__ int consume_mirror(const DevScene& S, const PX& px, ShadeCtx& c, jvec3* l_final, PassParts* pp = nullptr) {
  constexpr bool PASSES = sm(M, SM_PASSES);
  const DevMaterial* ot = shade_tri(S, c.obj).m;
  const int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  const jvec3 obj_hit_fr = jv_scale(V3(ot->brdf), (float)(1.0 / JADE_PI_D));
  float kk = (float)(k / (JADE_RR_RATE_D / JADE_PI_D));
  jvec3 refl = px.dir(0);
  int nh = px.hit(0);
  if (nh >= 0) {
    c.out = jv_neg(refl);
    c.src = px.hpt(0);
    c.obj = nh;
    *l_final = jv(0, 0, 0);
    if (PASSES) pp->cls = -1;
    return path_push(c, jv(0, 0, 0), jv_scale(obj_hit_fr, kk)) ? CONSUME_END : CONSUME_VERTEX;
  }
  *l_final = jv_scale(jv_mul(sample_hdr(S, refl), obj_hit_fr), kk);
  if (PASSES) {
    pp->cls = PASS_SPECULAR_SKY;
    pp->e = *l_final;
  }
  return CONSUME_END;
}

// Fold the results of the rays issued last pass.  CONSUME_VERTEX: the path
// moved to a new vertex (c.obj/src/out updated); CONSUME_END: it ended with
// *l_final; CONSUME_ZERO: pathTracing returned 0 (:1231); CONSUME_EMITTED: the
// refraction loop issued its next ray.
// M: the render's mode, as bounce_branch reads it.  SM_LIGHTS: slot 0 holds the shadow ray towards entry `light`, whose term is multiplied by light_weight
// SM_COSINE: where a ray came from cosine_dir_rng, the reference's |dot(normal, direction)| is cosine_weight - four places, nothing else
// SM_MIS: JADE_DIRECT_MIS (include/jade_bvh.h, "The direct light, stated"; with SM_COSINE only): at a diffuse or SSS-diffuse vertex an
// emitter term towards a weighted triangle is multiplied by w_L, and an indirect ray that lands on one adds T_B before the vertex's
// scale.  `mis`: the per-triangle table {m, M}.  Rays, draws, records and counters are SM_COSINE's.
// SM_PASSES: include/jade_bvh.h, "The passes, stated": beside l_dir - formed by the statements it always was - the emitter terms (the
// loop's and T_B) and the sky term are summed apart and leave in *pp with the branch's scale (PassParts, above).
template <uint32_t M = 0>
static __device__ int consume(const DevScene& S, const Px& px, ShadeCtx& c, jvec3* l_final, const uint4* lights = nullptr, uint32_t light = 0u,
                              const float2* mis = nullptr, PassParts* pp = nullptr) {
  constexpr bool ENVIS = sm(M, SM_ENVIS), LIGHTS = sm(M, SM_LIGHTS), COSINE = sm(M, SM_COSINE), MIS = sm(M, SM_MIS), PASSES = sm(M, SM_PASSES);
  const jade_triangle* T = S.tris;  // vertices only
  const int nE = S.n_emit;
  const int nL = LIGHTS ? (nE > 0 ? 1 : 0) : nE;
  const float PI_F = (float)JADE_PI_D;
  const float RR_F = (float)JADE_RR_RATE_D;
  const ShadeTri ots = shade_tri(S, c.obj);
  const DevMaterial* ot = ots.m;
  const jvec3 n = ots.norm;
  const int k = ot->refract_mode != JADE_NO_REFRACT ? 2 : 1;
  const jvec3 obj_hit_fr = jv_scale(V3(ot->brdf), (float)(1.0 / JADE_PI_D));
  jvec3 l_dir = jv(0, 0, 0);
  jvec3 part_e = jv(0, 0, 0), part_s = jv(0, 0, 0);  // PASSES only
  if (PASSES) {
    pp->cls = -1;
    pp->pushed = false;
    pp->thr0 = c.thr;
  }

  if (c.stage == ST_DIFFUSE) {
    const bool sss = (c.flags & STF_SSS) != 0;
    const jvec3 f = sss ? jv_scale(V3(ot->refract_albedo), (float)(1.0 / JADE_PI_D)) : obj_hit_fr;
    for (int i = 0; i < nL; ++i) {
      int h = px.hit(i);
      int emit_tri_idx = S.emit[LIGHTS ? (int)light : i];
      if (h >= 0 && h == emit_tri_idx) {
        jvec3 ld = px.dir(i);
        const ShadeTri t_i = shade_tri(S, emit_tri_idx);
        float dls = jv_dot(ld, ld);
        jvec3 w = jv_mul(V3(t_i.m->emissive), f);
        w = jv_scale(w, jade_fabs(jv_dot(n, ld) * jv_dot(t_i.norm, ld)));
        w = jv_divs(jv_divs(w, dls), dls);
        w = jv_scale(w, tri_size(&T[emit_tri_idx]));
        if (LIGHTS) w = jv_scale(w, light_weight(lights, (uint32_t)nE, light));  // x 1 / (the probability the entry was drawn with)
        if (MIS) {
          const float2 e = mis[emit_tri_idx];
          float w_L, g_B;
          mis_terms(n, t_i.norm, tri_size(&T[emit_tri_idx]), e.x, LIGHTS ? e.y : e.x, ld, &w_L, &g_B);
          w = jv_scale(w, w_L);
        }
        l_dir = jv_add(l_dir, w);
        if (PASSES) part_e = jv_add(part_e, w);
      }
    }
    if (ENVIS ? px.hit(nL) == -1 : px.hit(nL) < 0) {  // (-1: traced and nothing hit; -2: no environment ray this bounce - env_sampling only)
      jvec3 rd = px.dir(nL);
      jvec3 w = jv_mul(sample_hdr(S, rd), f);
      w = jv_scale(w, COSINE && !ENVIS ? cosine_weight(n, rd) : jade_fabs(jv_dot(n, rd)));
      w = jv_scale(jv_scale(w, 2.0f), PI_F);
      if (ENVIS) w = jv_scale(w, __int_as_float(px.auxi()));  // x (1 / 2 pi) / pdf: the reference's weight is 1 / its own pdf
      l_dir = jv_add(l_dir, w);
      if (PASSES) part_s = w;
    }
    if (MIS && (c.flags & STF_RR)) {  // the bounce term: the indirect ray found a weighted emitter
      const int bh = px.hit(nL + 1);
      if (bh >= 0) {
        const float2 e = mis[bh];
        if (e.x > 0) {
          const ShadeTri t_b = shade_tri(S, bh);
          float w_L, g_B;
          mis_terms(n, t_b.norm, tri_size(&T[bh]), e.x, LIGHTS ? e.y : e.x, jv_sub(px.hpt(nL + 1), c.src), &w_L, &g_B);
          const jvec3 t_B = jv_divs(jv_scale(jv_mul(V3(t_b.m->emissive), f), g_B), RR_F);
          l_dir = jv_add(l_dir, t_B);
          if (PASSES) part_e = jv_add(part_e, t_B);
        }
      }
    }
    l_dir = jv_scale(l_dir, sss ? (float)(k / JADE_SSS_RATE_D) : (float)k);
    *l_final = l_dir;
    if (PASSES) {
      pp->cls = PASS_SAMPLED + (sss ? 4 : 0) + (c.depth != 0 ? 1 : 0);
      pp->e = jv_scale(part_e, sss ? (float)(k / JADE_SSS_RATE_D) : (float)k);
      pp->s = jv_scale(part_s, sss ? (float)(k / JADE_SSS_RATE_D) : (float)k);
    }
    if (!(c.flags & STF_RR)) return CONSUME_END;
    int nh = px.hit(nL + 1);
    if (nh >= 0 && nonemissive(shade_tri(S, nh).m)) {
      jvec3 rd = jv_neg(px.dir(nL + 1));
      jvec3 indir_rate = jv_divs(jv_scale(obj_hit_fr, COSINE ? cosine_weight(n, rd) : jade_fabs(jv_dot(rd, n))), RR_F);
      jvec3 rate = sss ? jv_divs(jv_scale(indir_rate, (float)k), (float)JADE_SSS_RATE_D) : jv_scale(indir_rate, (float)k);
      c.src = px.hpt(nL + 1);
      c.out = rd;
      c.obj = nh;
      if (PASSES) pp->pushed = true;
      return path_push(c, l_dir, rate) ? CONSUME_END : CONSUME_VERTEX;
    }
    return CONSUME_END;
  }

  if (c.stage == ST_BSSRDF) {
    const int middle = px.skip();
    const ShadeTri t_is = shade_tri(S, middle);
    const DevMaterial* t_i = t_is.m;
    const jvec3 t_norm = t_is.norm;
    const jvec3 bssrdf = px.aux();
    const float eta = t_i->refract_index;
    const float R0 = (eta - 1) / (eta + 1) * (eta - 1) / (eta + 1);
    const float area_total = S.prefix[S.segs[t_i->obj_idx].end_idx];
    for (int i = 0; i < nL; ++i) {
      int h = px.hit(i);
      int emit_tri_idx = S.emit[LIGHTS ? (int)light : i];
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
        if (LIGHTS) w = jv_scale(w, light_weight(lights, (uint32_t)nE, light));
        l_dir = jv_add(l_dir, w);
        if (PASSES) part_e = jv_add(part_e, w);
      }
    }
    if (ENVIS ? px.hit(nL) == -1 : px.hit(nL) < 0) {
      jvec3 rd = px.dir(nL);
      float fresnel_rate_o = schlick_out(R0, jade_fabs(jv_dot(rd, t_norm)));
      jvec3 w = jv_mul(jv_scale(sample_hdr(S, rd), fresnel_rate_o), bssrdf);
      w = jv_scale(jv_scale(w, COSINE && !ENVIS ? cosine_weight(t_norm, rd) : jade_fabs(jv_dot(t_norm, rd))), 2.0f);
      if (ENVIS) w = jv_scale(w, __int_as_float(px.auxi()));
      l_dir = jv_add(l_dir, w);
      if (PASSES) part_s = w;
    }
    l_dir = jv_scale(l_dir, (float)(k / (1 - JADE_SSS_RATE_D)));
    *l_final = l_dir;
    if (PASSES) {
      pp->cls = PASS_SAMPLED + 8 + (c.depth != 0 ? 1 : 0);
      pp->e = jv_scale(part_e, (float)(k / (1 - JADE_SSS_RATE_D)));
      pp->s = jv_scale(part_s, (float)(k / (1 - JADE_SSS_RATE_D)));
    }
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
      if (PASSES) pp->pushed = true;
      return path_push(c, l_dir, rate) ? CONSUME_END : CONSUME_VERTEX;
    }
    return CONSUME_END;
  }

  if (c.stage == ST_MIRROR) return consume_mirror<Px, M>(S, px, c, l_final, pp);

  if (c.stage == ST_REFRACT_LOOP) {
    // one iteration of the for loop at PathTrace.cu:1201-1234
    const float triangle_miu = ot->refract_index;
    const float R0 = (1 - triangle_miu) / (1 + triangle_miu) * (1 - triangle_miu) / (1 + triangle_miu);
    int nh = px.hit(0);
    if (nh < 0) return CONSUME_ZERO;  // "obj surface is not close": return vec3(0)
    const ShadeTri hts = shade_tri(S, nh);
    const DevMaterial* ht = hts.m;
    const jvec3 hn = hts.norm;
    jvec3 refract_ray = px.dir(0);
    jvec3 start = px.origin();
    jvec3 hp = px.hpt(0);
    jvec3 l_indir_rate = px.aux();
    bool full_reflex = false;
    refract_ray = gen_refract_ray(refract_ray, hn, triangle_miu, &full_reflex);
    jvec3 distance = jv_sub(start, hp);
    float dist = jade_sqrt(jv_dot(distance, distance));
    l_indir_rate = jv_mul(l_indir_rate, jv(jade_powf(ht->refract_rate[0], dist), jade_powf(ht->refract_rate[1], dist),
                                           jade_powf(ht->refract_rate[2], dist)));
    float fresnel_rate_o = schlick_out(R0, jade_fabs(jv_dot(refract_ray, hn)));
    float reflex_refract_select = jade_rand(&c.rng);
    int it = px.auxi() + 1;
    bool leave = true;
    if (full_reflex || reflex_refract_select < 0.2f) {
      refract_ray = jv_sub(refract_ray, jv_scale(hn, 2 * jv_dot(refract_ray, hn)));
      if (!full_reflex) l_indir_rate = jv_scale(l_indir_rate, fresnel_rate_o * 5);
      leave = it >= JADE_MAX_FULL_REFLEX_TIME;  // loop exhausted: fall through to the RR test
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

  // ST_REFRACT_EXIT, PathTrace.cu:1239-1257
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
    if (PASSES) {  // the sky at the end of a glass chain
      pp->cls = PASS_SPECULAR_SKY;
      pp->e = *l_final;
    }
    return CONSUME_END;
  }
}
