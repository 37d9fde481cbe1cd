// jade_scene_prep.hip — the host-only half of jade_scene_create: the caller's BVH, triangles and environment map turned into the
// records the kernels read (jade_device.h, jade_trace.h).  No HIP call is made here; jade_hip.hip uploads what prepare_scene returns.
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

#include "jade_runtime.h"

namespace {

// Where the caller's nodes go: internal node -> its record, leaf -> its first pair record.  Only what the root reaches is laid out
// (include/jade_rt.h, jade_bvh_node): the reference's hitBVH never reads another node, so whatever lies in the rest of the caller's
// array - spare capacity, junk - is never read here either.  A node the root reaches along several paths gets ONE record.
struct Layout {
  const jade_scene_desc* d;
  std::vector<int32_t> compact;
  std::vector<uint32_t> pair_first;
  std::vector<int32_t> internals;    // the distinct internal nodes the root reaches, every parent before its children
  std::vector<int32_t> leaves;       // the distinct leaves the root reaches, in the order the internal nodes name them
  std::vector<int32_t> leaf_parent;  // leaf -> the first internal node of `internals` that names it (0: none, the root is a leaf)
  int n_internal = 0;
  size_t n_pairs = 0;
  void number_internal_nodes();
  void number_pairs();
  uint32_t ref_of(int child) const {
    if (child <= 0) return JADE_REF_NONE;
    const jade_bvh_node& c = d->nodes[child];
    if (c.n > 0) return JADE_REF_LEAF | ((pair_first[child] * 5u) << 4) | (uint32_t)((c.n + 1) / 2);  // bits 4-30: byte offset / 16 of the first pair record
    return (uint32_t)compact[child];
  }
};

// Re-lay the BVH: compact the internal nodes, children's boxes in the parent.  Internal nodes are numbered by
// decreasing surface area of their own box (the SAH's measure of how often a node is visited), so that any prefix
// [0, k) of the array is a connected top of the tree - a child's box is never larger than its parent's, ties keep
// the breadth-first order - and k_trace can keep that prefix in LDS (jade_device.h, JADE_LDS_TOP_NODES).
void Layout::number_internal_nodes() {
  const int nN = d->n_nodes;
  compact.assign(nN, -1);
  leaf_parent.assign(nN, 0);
  auto internal = [&](int i) { return i > 0 && d->nodes[i].n <= 0; };
  // The internal nodes the root reaches, each once.  The caller's "tree" may name a node from several parents (validate_desc bounds
  // the walk, so there is no cycle): a node is taken once all the edges into it have been followed, which puts every parent before
  // its children and, on a tree, is the breadth-first order.
  std::vector<int32_t> edges_in(nN, 0);
  {
    std::vector<uint8_t> seen(nN, 0);
    std::vector<int32_t> todo;
    if (internal(1)) { seen[1] = 1; todo.push_back(1); }
    while (!todo.empty()) {
      const jade_bvh_node& nd = d->nodes[todo.back()];
      todo.pop_back();
      for (int ch : {nd.left, nd.right})
        if (internal(ch)) {
          ++edges_in[ch];
          if (!seen[ch]) { seen[ch] = 1; todo.push_back(ch); }
        }
    }
  }
  std::vector<int32_t>& bfs = internals;
  bfs.reserve(nN);
  std::vector<uint8_t> leaf_seen(nN, 0);
  if (internal(1)) bfs.push_back(1);
  else { leaf_seen[1] = 1; leaves.push_back(1); }
  for (size_t h = 0; h < bfs.size(); ++h) {
    const jade_bvh_node& nd = d->nodes[bfs[h]];
    for (int ch : {nd.left, nd.right}) {
      if (ch <= 0) continue;
      if (internal(ch)) {
        if (--edges_in[ch] == 0) bfs.push_back(ch);
      } else if (!leaf_seen[ch]) {
        leaf_seen[ch] = 1;
        leaves.push_back(ch);
        leaf_parent[ch] = bfs[h];
      }
    }
  }
  auto area = [&](int i) {
    const jade_bvh_node& nd = d->nodes[i];
    const double x = (double)nd.bb[0] - nd.aa[0], y = (double)nd.bb[1] - nd.aa[1], z = (double)nd.bb[2] - nd.aa[2];
    return x * y + y * z + z * x;
  };
  std::vector<double> ar(bfs.size());
  for (size_t h = 0; h < bfs.size(); ++h) ar[h] = area(bfs[h]);
  // a child inherits at most its parents' keys, so a prefix of the order is always closed under "parent of"
  std::vector<double> key(nN, 0.0);
  std::vector<uint8_t> keyed(nN, 0);
  for (size_t h = 0; h < bfs.size(); ++h) {
    const int i = bfs[h];
    if (h == 0) key[i] = ar[0];
    const jade_bvh_node& nd = d->nodes[i];
    for (int ch : {nd.left, nd.right})
      if (internal(ch)) {
        const double k = std::min(key[i], area(ch));
        key[ch] = keyed[ch] ? std::min(key[ch], k) : k;
        keyed[ch] = 1;
      }
  }
  std::vector<int32_t> order(bfs.size());
  for (size_t h = 0; h < bfs.size(); ++h) order[h] = (int32_t)h;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[bfs[a]] > key[bfs[b]]; });
  for (int32_t h : order) compact[bfs[h]] = n_internal++;
}

// vertex records hold two consecutive triangles of a leaf each (jade_trace.h): number the pairs leaf by leaf, by first triangle
// (leaves may overlap: those that start at the same triangle keep the order in which the tree names them)
void Layout::number_pairs() {
  pair_first.assign(d->n_nodes, 0);
  std::vector<int32_t> by_index = leaves;
  std::stable_sort(by_index.begin(), by_index.end(), [&](int a, int b) { return d->nodes[a].index < d->nodes[b].index; });
  for (int i : by_index) {
    pair_first[i] = (uint32_t)n_pairs;
    n_pairs += (size_t)(d->nodes[i].n + 1) / 2;
  }
}

// the binary records: an internal node holds its children's boxes and references
void binary_records(const jade_scene_desc* d, const Layout& lay, std::vector<float4>& nodes, bool* missing_child_out) {
  nodes.assign((size_t)4 * std::max(lay.n_internal, 1), float4{});
  bool missing_child = false;  // the reference's "child 0" under an internal node: the walk then needs its general form
  for (int i : lay.internals) {
    const jade_bvh_node& nd = d->nodes[i];
    if (nd.left <= 0 || nd.right <= 0) missing_child = true;
    float la[3] = {0, 0, 0}, lb[3] = {0, 0, 0}, ra[3] = {0, 0, 0}, rb[3] = {0, 0, 0};
    if (nd.left > 0) { memcpy(la, d->nodes[nd.left].aa, 12); memcpy(lb, d->nodes[nd.left].bb, 12); }
    if (nd.right > 0) { memcpy(ra, d->nodes[nd.right].aa, 12); memcpy(rb, d->nodes[nd.right].bb, 12); }
    float4* o = &nodes[(size_t)4 * lay.compact[i]];
    o[0] = make_float4(la[0], ra[0], la[1], ra[1]);
    o[1] = make_float4(la[2], ra[2], lb[0], rb[0]);
    o[2] = make_float4(lb[1], rb[1], lb[2], rb[2]);
    uint32_t refs[4] = {lay.ref_of(nd.left), lay.ref_of(nd.right), 0u, 0u};
    memcpy(&o[3], refs, 16);
  }
  *missing_child_out = missing_child;
}

// The wide walk and the occluder cache both rest on "a ray that meets a node's box meets every ancestor's" (jade_trace.h), which
// holds when every child's box lies inside its parent's, bound by bound, with no NaN - true of any tree built by min / max over
// the triangles (this repo's builders, the reference's), but the caller's array is the caller's: a tree with padded,
// refitted or NaN boxes is walked with binary units from the root only, which needs no such property.  Over the nodes the root reaches.
bool boxes_nested(const jade_scene_desc* d, const Layout& lay) {
  for (int i : lay.internals) {
    const jade_bvh_node& nd = d->nodes[i];
    for (int ch : {nd.left, nd.right}) {
      if (ch <= 0) continue;
      const jade_bvh_node& c = d->nodes[ch];
      for (int a = 0; a < 3; ++a)
        if (!(c.aa[a] >= nd.aa[a] && c.bb[a] <= nd.bb[a] && c.aa[a] <= c.bb[a])) return false;  // (a NaN fails every comparison)
    }
  }
  return true;
}

// the four-wide records (jade_device.h): node i's record holds its grandchildren - each child's own record, or the child twice
// if it is a leaf
void wide_records(const jade_scene_desc* d, const Layout& lay, const std::vector<float4>& nodes, std::vector<float4>& nodes4) {
  nodes4.assign((size_t)8 * lay.n_internal, make_float4(0, 0, 0, 0));
  for (int i : lay.internals) {
    const jade_bvh_node& nd = d->nodes[i];
    float4* o = &nodes4[(size_t)8 * lay.compact[i]];
    uint32_t refs[4];
    const int ch[2] = {nd.left, nd.right};
    for (int h = 0; h < 2; ++h) {
      const jade_bvh_node& c = d->nodes[ch[h]];
      if (c.n > 0) {  // a leaf: its own box in both lanes of the half, one reference
        o[3 * h + 0] = make_float4(c.aa[0], c.aa[0], c.aa[1], c.aa[1]);
        o[3 * h + 1] = make_float4(c.aa[2], c.aa[2], c.bb[0], c.bb[0]);
        o[3 * h + 2] = make_float4(c.bb[1], c.bb[1], c.bb[2], c.bb[2]);
        refs[2 * h] = lay.ref_of(ch[h]);
        refs[2 * h + 1] = JADE_REF_NONE;
      } else {
        const float4* src = &nodes[(size_t)4 * lay.compact[ch[h]]];
        o[3 * h + 0] = src[0];
        o[3 * h + 1] = src[1];
        o[3 * h + 2] = src[2];
        refs[2 * h] = lay.ref_of(c.left);
        refs[2 * h + 1] = lay.ref_of(c.right);
      }
    }
    memcpy(&o[6], refs, 16);
  }
}

// the pair records: two consecutive triangles of a leaf each, vertices interleaved (jade_trace.h)
void pair_records(const jade_scene_desc* d, const Layout& lay, std::vector<float4>& tverts) {
  tverts.assign((size_t)5 * std::max<size_t>(lay.n_pairs, 1), float4{});
  for (int i : lay.leaves) {
    const jade_bvh_node& nd = d->nodes[i];
    for (int k = 0; k < nd.n; k += 2) {
      const bool has_b = k + 1 < nd.n;
      const jade_triangle& a = d->triangles[nd.index + k];
      const jade_triangle& b = d->triangles[nd.index + k + (has_b ? 1 : 0)];  // an odd leaf's last record repeats A
      float4* o = &tverts[5 * ((size_t)lay.pair_first[i] + (size_t)k / 2)];
      o[0] = make_float4(a.p1[0], b.p1[0], a.p1[1], b.p1[1]);
      o[1] = make_float4(a.p1[2], b.p1[2], a.p2[0], b.p2[0]);
      o[2] = make_float4(a.p2[1], b.p2[1], a.p2[2], b.p2[2]);
      o[3] = make_float4(a.p3[0], b.p3[0], a.p3[1], b.p3[1]);
      // flag word: bit 0 = B is a triangle; bits 1-31 = the leaf's parent + 1 (occluder cache, jade_trace.h; 0 = the root or none: a
      // walk "from the root" is the whole walk, nothing to cache)
      const int par = lay.leaf_parent[i];
      const uint32_t parent1 = (par > 1 && lay.compact[par] > 0) ? (uint32_t)lay.compact[par] + 1u : 0u;
      const uint32_t tag[2] = {(uint32_t)(nd.index + k), (has_b ? 1u : 0u) | (parent1 << 1)};
      float tagf[2];
      memcpy(tagf, tag, 8);
      o[4] = make_float4(a.p3[2], b.p3[2], tagf[0], tagf[1]);
    }
  }
}

}  // namespace

// Guide tables for the BSSRDF exit-point search (jade_shade.h, begin_bounce; PathTrace.cu:1031-1048).  Per object with
// finite, non-decreasing prefix areas: Gn = the power of two >= 4 x its triangles cells, guide[c] = the first triangle i with
// fl(c / Gn * A) <= prefix[i] - the product rounded once to fp32, as the kernel's `u * A` is (this file is built
// -ffp-contract=off like the device code) - for c = 0 .. Gn, and one more entry so that cell Gn (u == 1) has an upper bound.
// An object whose prefix areas are not monotone or not finite gets Gn = 0: the kernel then bisects as the reference does.  No HIP call
// (libjade_hip_debug.so's jade_debug_guide_tables_host returns these tables as they are, tests/test_area_search_cpu.py).
void guide_tables(const jade_scene_desc* d, std::vector<uint32_t>& guide, std::vector<uint2>& guide_obj) {
  guide_obj.assign((size_t)d->n_objects, make_uint2(0u, 0u));
  for (int o = 0; o < d->n_objects; ++o) {
    const int b = d->obj_segs[o].begin_idx, e = d->obj_segs[o].end_idx;
    bool ok = true;
    for (int i = b; i <= e && ok; ++i) {
      const float v = d->prefix_area[i];
      ok = v == v && v >= 0.0f && v < 3.0e38f && (i == b || v >= d->prefix_area[i - 1]);
    }
    const size_t nt = (size_t)(e - b + 1);
    if (!ok || nt < 2 || nt > ((size_t)1 << 21)) continue;
    uint32_t gn = 1;
    while (gn < 4 * nt) gn <<= 1;
    const float A = d->prefix_area[e];
    const size_t first = guide.size();
    guide.resize(first + gn + 2);
    int i = b;
    for (uint32_t c = 0; c <= gn; ++c) {
      const float u = (float)c / (float)gn;  // exact: both are powers of two apart
      volatile float x = u * A;              // one rounding (volatile: no excess precision, whatever the host compiler does)
      const float xv = x;
      while (i < e && !(xv <= d->prefix_area[i])) ++i;
      guide[first + c] = (uint32_t)i;
    }
    guide[first + gn + 1] = guide[first + gn];
    guide_obj[(size_t)o] = make_uint2((uint32_t)first, gn);
  }
  if (guide.empty()) guide.push_back(0u);
}

namespace {

// What shading reads of a triangle (jade_device.h, DevMaterial): the distinct {object, material} tuples of the caller's
// records - the reference copies an object's material into each of its triangles, PathTrace.cu:451 - and per triangle
// the flat normal + the number of its tuple.  Same bytes, read from 16 B + a cached table instead of a 112-B record.
void materials(const jade_scene_desc* d, std::vector<DevMaterial>& mats, std::vector<float4>& tnorm) {
  tnorm.assign((size_t)d->n_triangles, float4{});
  std::map<std::string, uint32_t> seen;  // key: the 64 bytes of the tuple
  std::string last_key;
  uint32_t last_id = 0;
  for (int i = 0; i < d->n_triangles; ++i) {
    const jade_triangle& t = d->triangles[i];
    DevMaterial m;
    memcpy(m.emissive, t.emissive, 12);
    memcpy(m.brdf, t.brdf, 12);
    m.reflex_mode = t.reflex_mode;
    m.refract_mode = t.refract_mode;
    memcpy(m.refract_rate, t.refract_rate, 12);
    memcpy(m.refract_albedo, t.refract_albedo, 12);
    m.refract_index = t.refract_index;
    m.obj_idx = t.obj_idx;
    std::string key(reinterpret_cast<const char*>(&m), sizeof m);
    uint32_t id;
    if (i > 0 && key == last_key) {
      id = last_id;
    } else {
      auto it = seen.find(key);
      if (it == seen.end()) {
        id = (uint32_t)mats.size();
        mats.push_back(m);
        seen.emplace(key, id);
      } else {
        id = it->second;
      }
      last_key = std::move(key);
      last_id = id;
    }
    float idf;
    memcpy(&idf, &id, 4);
    tnorm[(size_t)i] = make_float4(t.norm[0], t.norm[1], t.norm[2], idf);
  }
}

}  // namespace

// Environment importance sampling (jade_render_params.env_sampling; non-parity): Vose's alias table over the texels, weight =
// (luminance + 1 % of the mean luminance) x sin(theta of the row's centre) - the floor keeps every texel drawable, so the
// estimator stays unbiased wherever the sky is not black.  include/jade_rt.h (JADE_ENV_IMPORTANCE) states the weight and what an
// entry means; how small and large texels are paired is not part of that statement.  No HIP call.
static void alias_table_of(const std::vector<double>& wgt, double total, std::vector<uint4>& table);
void env_alias_table(int32_t env_width, int32_t env_height, const float* env_rgb, std::vector<uint4>& env_alias) {
  const size_t W = (size_t)env_width, H = (size_t)env_height, N = W * H;
  std::vector<double> wgt(N);
  double lum_sum = 0;
  for (size_t i = 0; i < N; ++i) {
    const float* t = env_rgb + 3 * i;
    const double l = 0.2126 * std::max(t[0], 0.0f) + 0.7152 * std::max(t[1], 0.0f) + 0.0722 * std::max(t[2], 0.0f);
    wgt[i] = std::isfinite(l) ? l : 0.0;
    lum_sum += wgt[i];
  }
  const double floor_l = lum_sum > 0 ? 0.01 * lum_sum / (double)N : 1.0;
  double total = 0;
  for (size_t j = 0; j < H; ++j) {
    const double st = std::sin(JADE_PI_D * ((double)j + 0.5) / (double)H);
    for (size_t i = 0; i < W; ++i) {
      wgt[j * W + i] = (wgt[j * W + i] + floor_l) * st;
      total += wgt[j * W + i];
    }
  }
  alias_table_of(wgt, total, env_alias);
}

// Vose's alias table for the weights wgt (sum: total > 0): entry i = {accept, alias, fl(q_i), fl(q_alias)} with q_i = wgt_i / total x N.
// Shared by the environment's texels (above) and the emitter entries (light_alias_table, below).
static void alias_table_of(const std::vector<double>& wgt, double total, std::vector<uint4>& env_alias) {
  const size_t N = wgt.size();
  std::vector<double> q(N);
  std::vector<uint32_t> small, large, alias(N);
  std::vector<float> accept(N, 1.0f);
  for (size_t i = 0; i < N; ++i) {
    q[i] = wgt[i] / total * (double)N;  // the entry's probability x N (mean 1)
    alias[i] = (uint32_t)i;
    (q[i] < 1.0 ? small : large).push_back((uint32_t)i);
  }
  std::vector<double> r = q;
  while (!small.empty() && !large.empty()) {
    const uint32_t a = small.back(), g = large.back();
    small.pop_back();
    accept[a] = (float)r[a];
    alias[a] = g;
    r[g] = (r[g] + r[a]) - 1.0;
    if (r[g] < 1.0) { large.pop_back(); small.push_back(g); }
  }
  env_alias.resize(N);
  for (size_t i = 0; i < N; ++i) {
    const float ps = (float)q[i], pa = (float)q[alias[i]];
    uint4 e;
    memcpy(&e.x, &accept[i], 4);
    e.y = alias[i];
    memcpy(&e.z, &ps, 4);
    memcpy(&e.w, &pa, 4);
    env_alias[i] = e;
  }
}

// One-light sampling (jade_scene_set_light_sampling = JADE_LIGHTS_ONE; non-parity): the alias table over the entries of emit_indices,
// weight = area x luminance of emission + 1 % of the mean of that - the floor keeps every entry drawable, so the estimator stays
// unbiased whatever an entry's triangle emits.  include/jade_bvh.h ("The lights, stated") states the weight and what an entry means.  The
// area is the one the integrator multiplies an entry's term by: tri_size's statements (jade_shade.h; PathTrace.cu:897-903) in fp32.  No HIP call.
void light_alias_table(const jade_triangle* triangles, const int32_t* emit_indices, int32_t n_emit, std::vector<uint4>& light_alias) {
  const size_t N = n_emit > 0 ? (size_t)n_emit : 0;
  light_alias.clear();
  if (N == 0) return;
  std::vector<double> wgt(N);
  double sum = 0;
  for (size_t i = 0; i < N; ++i) {
    const jade_triangle& t = triangles[emit_indices[i]];
    const jvec3 p1 = jv(t.p1[0], t.p1[1], t.p1[2]);
    const jvec3 cp = jv_cross(jv_sub(jv(t.p2[0], t.p2[1], t.p2[2]), p1), jv_sub(jv(t.p3[0], t.p3[1], t.p3[2]), p1));
    const float area = 0.5f * jade_sqrt(jv_dot(cp, cp));
    const double a = std::isfinite(area) ? (double)area : 0.0;
    double l = 0.2126 * std::max(t.emissive[0], 0.0f) + 0.7152 * std::max(t.emissive[1], 0.0f) + 0.0722 * std::max(t.emissive[2], 0.0f);
    if (!std::isfinite(l)) l = 0.0;
    const double w = a * l;
    wgt[i] = std::isfinite(w) ? w : 0.0;
    sum += wgt[i];
  }
  const double floor_w = sum > 0 ? 0.01 * sum / (double)N : 1.0;
  double total = 0;
  for (size_t i = 0; i < N; ++i) {
    wgt[i] += floor_w;
    total += wgt[i];
  }
  alias_table_of(wgt, total, light_alias);
}

// Multiple importance sampling of the emitters (jade_scene_set_direct_sampling = JADE_DIRECT_MIS; non-parity): per triangle h the number
// of entries of emit_indices that name it, m, and the probability with which JADE_LIGHTS_ONE's table realises them, M - for a WEIGHTED
// triangle (emits at or above the indirect-hit threshold, area and stored normal finite and positive: include/jade_bvh.h, "The direct
// light, stated"); {0, 0} for every other.  The area is tri_size's statements in fp32, as in light_alias_table.  No HIP call.
void mis_table(const jade_triangle* triangles, int32_t n_triangles, const int32_t* emit_indices, int32_t n_emit, const std::vector<uint4>& light_alias,
               std::vector<float2>& mis) {
  const size_t N = n_triangles > 0 ? (size_t)n_triangles : 0, nE = n_emit > 0 ? (size_t)n_emit : 0;
  std::vector<uint32_t> count(N, 0u);
  std::vector<double> prob(N, 0.0);
  const bool have_q = nE > 0 && light_alias.size() == nE;
  for (size_t i = 0; i < nE; ++i) {
    const size_t h = (size_t)emit_indices[i];
    count[h]++;
    if (have_q) {
      float q;
      memcpy(&q, &light_alias[i].z, 4);
      prob[h] += (double)q;
    }
  }
  mis.assign(N, make_float2(0.0f, 0.0f));
  for (size_t h = 0; h < N; ++h) {
    if (count[h] == 0) continue;
    const jade_triangle& t = triangles[h];
    if (t.emissive[0] < 1.5e-4f && t.emissive[1] < 1.5e-4f && t.emissive[2] < 1.5e-4f) continue;  // nonemissive (jade_shade.h)
    const jvec3 p1 = jv(t.p1[0], t.p1[1], t.p1[2]);
    const jvec3 cp = jv_cross(jv_sub(jv(t.p2[0], t.p2[1], t.p2[2]), p1), jv_sub(jv(t.p3[0], t.p3[1], t.p3[2]), p1));
    const float area = 0.5f * jade_sqrt(jv_dot(cp, cp));
    const jvec3 ne = jv(t.norm[0], t.norm[1], t.norm[2]);
    const float nne = jv_dot(ne, ne);
    if (!(area > 0 && std::isfinite(area)) || !(nne > 0 && std::isfinite(nne))) continue;
    mis[h] = make_float2((float)count[h], (float)(prob[h] / (double)nE));
  }
}

// What jade_scene_create checks of the caller's descriptor before anything is derived from it: ranges, and a walk of the tree from the
// root - the nodes the root does not reach are not read (include/jade_rt.h).  No HIP call.
int validate_desc(const jade_scene_desc* d, int* depth_out) {
  if (d->abi_version != JADE_ABI_VERSION) return jade_fail(JADE_ERR_INVALID, "abi_version mismatch");
  if (d->n_triangles <= 0 || d->n_nodes < 2 || !d->triangles || !d->nodes)
    return jade_fail(JADE_ERR_INVALID, "scene needs triangles and a BVH (dummy node 0 + root 1)");
  if (d->n_triangles >= JADE_MAX_TRIS) return jade_fail(JADE_ERR_UNSUPPORTED, "too many triangles for the 27-bit leaf cursor (44.7 M)");
  if (d->n_emit < 0 || (d->n_emit > 0 && !d->emit_indices)) return jade_fail(JADE_ERR_INVALID, "bad emitter list");
  if (!d->index_mapping || !d->prefix_area || d->n_objects <= 0 || !d->obj_segs)
    return jade_fail(JADE_ERR_INVALID, "missing mapping / prefix areas / object segments");
  if (d->env_width <= 0 || d->env_height <= 0 || !d->env_rgb) return jade_fail(JADE_ERR_INVALID, "missing environment map");
  for (int i = 0; i < d->n_emit; ++i)
    if (d->emit_indices[i] < 0 || d->emit_indices[i] >= d->n_triangles) return jade_fail(JADE_ERR_INVALID, "emitter index out of range");
  for (int i = 0; i < d->n_triangles; ++i) {
    if (d->index_mapping[i] < 0 || d->index_mapping[i] >= d->n_triangles) return jade_fail(JADE_ERR_INVALID, "index_mapping out of range");
    if (d->triangles[i].obj_idx < 0 || d->triangles[i].obj_idx >= d->n_objects) return jade_fail(JADE_ERR_INVALID, "obj_idx out of range");
  }
  for (int i = 0; i < d->n_objects; ++i)
    if (d->obj_segs[i].begin_idx < 0 || d->obj_segs[i].end_idx >= d->n_triangles || d->obj_segs[i].begin_idx > d->obj_segs[i].end_idx)
      return jade_fail(JADE_ERR_INVALID, "object segment out of range");
  // prefix_area is read by the BSSRDF branch alone.  Most of it only steers the search (any value will do, jade_rt.h), but an object's
  // total, prefix_area[end_idx], is a FACTOR of that branch's radiance (PathTrace.cu:1105, 1160): not finite, it makes rates of inf
  // and NaN, whose sum depends on the order of summation - this module adds a path's radiance forward where the reference unwinds
  // its stacks - and at u = 0 the reference's search does not end.  Refused by both backends where the branch can run.
  bool sub_surface = false;
  for (int i = 0; i < d->n_triangles && !sub_surface; ++i) sub_surface = d->triangles[i].refract_mode == JADE_SUB_SURFACE;
  for (int i = 0; i < d->n_objects && sub_surface; ++i)
    if (!std::isfinite(d->prefix_area[d->obj_segs[i].end_idx]))
      return jade_fail(JADE_ERR_INVALID, "an object's total prefix_area is not finite in a scene with SUB_SURFACE triangles");
  // walk the tree: ranges, cycles (visit budget), depth <= stack capacity - 1
  std::vector<std::pair<int, int>> st;
  st.push_back({1, 1});
  int64_t budget = 4 * (int64_t)d->n_nodes + 8;
  int depth = 0;
  while (!st.empty()) {
    auto [id, dp] = st.back();
    st.pop_back();
    if (--budget < 0) return jade_fail(JADE_ERR_UNSUPPORTED, "BVH malformed (cycle)");
    if (dp > JADE_BVH_STACK_CAPACITY - 1) return jade_fail(JADE_ERR_UNSUPPORTED, "BVH deeper than the traversal stack");
    depth = std::max(depth, dp);
    const jade_bvh_node& nd = d->nodes[id];
    if (nd.n > 0) {
      if (nd.index < 0 || (int64_t)nd.index + nd.n > d->n_triangles) return jade_fail(JADE_ERR_INVALID, "leaf range out of bounds");
      if (nd.n > JADE_MAX_LEAF) return jade_fail(JADE_ERR_UNSUPPORTED, "leaf with more than 15 triangles");
      continue;
    }
    if (nd.left < 0 || nd.left >= d->n_nodes || nd.right < 0 || nd.right >= d->n_nodes)
      return jade_fail(JADE_ERR_INVALID, "child index out of range");
    if (nd.left > 0) st.push_back({nd.left, dp + 1});
    if (nd.right > 0) st.push_back({nd.right, dp + 1});
  }
  *depth_out = depth;
  return JADE_OK;
}

int prepare_scene(const jade_scene_desc& desc, int depth, const Tunables& tun, ScenePrep* out) {
  const jade_scene_desc* d = &desc;
  Layout lay{d};
  lay.number_internal_nodes();
  lay.number_pairs();
  if (lay.n_pairs * 5 >= ((size_t)1 << 27)) return jade_fail(JADE_ERR_UNSUPPORTED, "too many triangle pairs for the 27-bit leaf cursor");
  out->n_internal = lay.n_internal;
  out->n_pairs = lay.n_pairs;
  out->root_ref = lay.ref_of(1);
  binary_records(d, lay, out->nodes, &out->missing_child);
  pair_records(d, lay, out->tverts);
  out->geometry_bytes = out->nodes.size() * sizeof(float4) + out->tverts.size() * sizeof(float4);
  out->nested = boxes_nested(d, lay);
  // stack levels a walk may need (validate_desc bounds the binary walk's: depth <= capacity - 1): a wide unit pushes up to three
  // entries for every two levels it descends; a walk that starts with the cached subtrees has three more under it
  out->wide_fits = 3 * ((depth + 1) / 2) + 1 + 3 <= JADE_BVH_STACK_CAPACITY;
  out->cache_fits = depth + 3 <= JADE_BVH_STACK_CAPACITY - 1;
  // The wide records are built where the wide walk pays: measured with early exits, same process, k_trace per step: C5 (55 MB of node +
  // pair records, bound by dependent 64-B sector misses) 180.0 -> 166.6 ms; C3 (3.8 MB, L2-resident: a unit's own instructions count, and a wide unit
  // has more of them) 106.7 -> 110.2 ms, close-up 723 -> 755.  So: the rule of the ordered ray queue (JADE_SORT_GEOMETRY_BYTES);
  // JADE_WIDE=0 / 1 overrides it.
  const bool want_wide = tun.wide_mode < 0 ? out->geometry_bytes > JADE_SORT_GEOMETRY_BYTES : tun.wide_mode > 0;
  if (JADE_WIDE_WALK && want_wide && !out->missing_child && lay.n_internal > 0 && out->nested && out->wide_fits) wide_records(d, lay, out->nodes, out->nodes4);
  guide_tables(d, out->guide, out->guide_obj);
  materials(d, out->mats, out->tnorm);
  env_alias_table(d->env_width, d->env_height, d->env_rgb, out->env_alias);
  if (light_sampling_fits(d->n_emit)) light_alias_table(d->triangles, d->emit_indices, d->n_emit, out->light_alias);  // (a longer list renders with JADE_LIGHTS_ALL only)
  mis_table(d->triangles, d->n_triangles, d->emit_indices, d->n_emit, out->light_alias, out->mis);
  return JADE_OK;
}
