// prep_shapes_main.cpp - validate_desc + prepare_scene (jade_scene_prep.hip: host code, no HIP call) on every descriptor that
// `python tests/tree_shapes.py --dump DIR` wrote, as a stand-alone program for AddressSanitizer + UBSan (make asan-check).  No Python,
// no device: built with hipcc --offload-host-only together with jade_scene_prep.hip itself.
//   usage: prep_shapes DIR
// Per descriptor: the status must be the one the dump expects; an accepted one is prepared without and with wide records, and every
// reference of the records made is decoded and checked against the arrays' sizes (the sanitizer sees what the preparation reads,
// this sees what a kernel would read).
#include <dirent.h>

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

struct Dump {
  int32_t head[8];  // magic, n_triangles, n_nodes, n_emit, n_objects, env_width, env_height, the status expected
  std::vector<uint32_t> tri, nodes, env;
  std::vector<int32_t> emit, mapping, segs;
  std::vector<float> prefix;
};

template <class T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool load(const std::string& path, Dump& d) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  bool ok = fread(d.head, 4, 8, f) == 8 && d.head[0] == 0x4A545348;
  if (ok) {
    const size_t nt = (size_t)d.head[1], nn = (size_t)d.head[2];
    ok = read_n(f, d.tri, 28 * nt) && read_n(f, d.nodes, 10 * nn) && read_n(f, d.emit, (size_t)d.head[3]) && read_n(f, d.mapping, nt) &&
         read_n(f, d.prefix, nt) && read_n(f, d.segs, 2 * (size_t)d.head[4]) && read_n(f, d.env, 3 * (size_t)d.head[5] * (size_t)d.head[6]);
  }
  ok = ok && fgetc(f) == EOF;
  fclose(f);
  return ok;
}

bool ref_ok(uint32_t ref, const ScenePrep& p) {
  if (ref == JADE_REF_NONE) return true;
  if (ref & JADE_REF_LEAF) {
    const uint32_t units = (ref >> 4) & 0x7ffffffu, cnt = ref & 15u;
    return units % 5 == 0 && cnt >= 1 && (size_t)units / 5 + cnt <= p.n_pairs;
  }
  return ref < (uint32_t)p.n_internal;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(jade_triangle) == 112 && sizeof(jade_bvh_node) == 40 && sizeof(jade_obj_seg) == 8, "the dump's record sizes");
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  std::vector<std::string> names;
  if (DIR* dir = opendir(argv[1])) {
    while (dirent* e = readdir(dir)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.substr(n.size() - 4) == ".bin") names.push_back(n);
    }
    closedir(dir);
  }
  std::sort(names.begin(), names.end());
  if (names.empty()) {
    fprintf(stderr, "no descriptors in %s\n", argv[1]);
    return 2;
  }
  int bad = 0;
  for (const std::string& n : names) {
    Dump d;
    if (!load(std::string(argv[1]) + "/" + n, d)) {
      fprintf(stderr, "%s: unreadable\n", n.c_str());
      return 2;
    }
    jade_scene_desc desc{};
    desc.abi_version = JADE_ABI_VERSION;
    desc.n_triangles = d.head[1];
    desc.triangles = reinterpret_cast<const jade_triangle*>(d.tri.data());
    desc.n_nodes = d.head[2];
    desc.nodes = reinterpret_cast<const jade_bvh_node*>(d.nodes.data());
    desc.n_emit = d.head[3];
    desc.emit_indices = d.emit.data();
    desc.index_mapping = d.mapping.data();
    desc.prefix_area = d.prefix.data();
    desc.n_objects = d.head[4];
    desc.obj_segs = reinterpret_cast<const jade_obj_seg*>(d.segs.data());
    desc.env_width = d.head[5];
    desc.env_height = d.head[6];
    desc.env_rgb = reinterpret_cast<const float*>(d.env.data());
    int depth = 0;
    const int rc = validate_desc(&desc, &depth);
    if (rc != d.head[7]) {
      fprintf(stderr, "%s: status %d, expected %d (%s)\n", n.c_str(), rc, d.head[7], g_err.c_str());
      ++bad;
      continue;
    }
    if (rc) {
      printf("%-28s refused (%d: %s)\n", n.c_str(), rc, g_err.c_str());
      continue;
    }
    for (int wide = 0; wide < 2; ++wide) {
      Tunables tun;
      tun.wide_mode = wide;
      ScenePrep p;
      if (prepare_scene(desc, depth, tun, &p) != JADE_OK) {
        fprintf(stderr, "%s: prepare_scene: %s\n", n.c_str(), g_err.c_str());
        ++bad;
        break;
      }
      bool ok = ref_ok(p.root_ref, p) && p.nodes.size() == (size_t)4 * std::max(p.n_internal, 1) && p.tverts.size() == 5 * std::max<size_t>(p.n_pairs, 1) &&
                (p.nodes4.empty() || p.nodes4.size() == (size_t)8 * p.n_internal);
      for (int k = 0; ok && k < p.n_internal; ++k) {
        uint32_t r[4];
        memcpy(r, &p.nodes[4 * (size_t)k + 3], 16);
        ok = ref_ok(r[0], p) && ref_ok(r[1], p);
        if (ok && !p.nodes4.empty()) {
          memcpy(r, &p.nodes4[8 * (size_t)k + 6], 16);
          ok = ref_ok(r[0], p) && ref_ok(r[1], p) && ref_ok(r[2], p) && ref_ok(r[3], p);
        }
      }
      for (size_t k = 0; ok && k < p.n_pairs; ++k) {
        uint32_t tag[2];
        memcpy(tag, &p.tverts[5 * k + 4].z, 8);
        ok = tag[0] + (tag[1] & 1u) < (uint32_t)desc.n_triangles && (tag[1] >> 1) <= (uint32_t)p.n_internal;
      }
      if (!ok) {
        fprintf(stderr, "%s (wide %d): a reference outside its array\n", n.c_str(), wide);
        ++bad;
        break;
      }
      if (wide)
        printf("%-28s depth %3d  internal %4d  pairs %4zu  missing_child %d  nested %d  wide records %zu\n", n.c_str(), depth, p.n_internal, p.n_pairs,
               (int)p.missing_child, (int)p.nested, p.nodes4.size() / 8);
    }
  }
  if (bad) {
    fprintf(stderr, "prep_shapes: %d of %zu descriptors failed\n", bad, names.size());
    return 1;
  }
  printf("prep_shapes: %zu descriptors, clean\n", names.size());
  return 0;
}
