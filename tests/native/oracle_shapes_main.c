/* oracle_shapes_main.c - the oracle on every descriptor that `python tests/tree_shapes.py --dump DIR` wrote, as a stand-alone program
 * for AddressSanitizer + UBSan (make asan-check; built with gcc together with oracle/jade_oracle.c and -DJADE_ORACLE_PROBE, the build
 * that has the cached walk and its tables, occ_prepare).
 *   usage: oracle_shapes DIR
 * Per descriptor: jade_scene_create must answer the status the dump expects; on an accepted scene 256 rays go through jade_trace_rays
 * with the reference's walk and again with the cached walk switched on (jade_oracle_set_prune mode 5), and - raw rays being no
 * yes/no queries, which alone consult the cache - a 16 x 16 frame of 2 spp is rendered in that mode: its shadow and environment
 * rays build the tables over the nodes the root reaches and walk from the cached subtrees. */
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jade_rt.h"

void jade_oracle_set_prune(int mode, float rel, float abs_, float min_dz); /* oracle/jade_oracle.c, JADE_ORACLE_PROBE */
void jade_oracle_occ_reset(void);

static void* read_n(FILE* f, size_t size, size_t n, int* ok) {
  void* p = malloc(size * n ? size * n : 1);
  if (!p || (n && fread(p, size, n, f) != n)) *ok = 0;
  return p;
}

static int by_name(const void* a, const void* b) { return strcmp(*(char* const*)a, *(char* const*)b); }

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  char* names[512];
  int n_names = 0;
  DIR* dir = opendir(argv[1]);
  if (dir) {
    struct dirent* e;
    while ((e = readdir(dir)) != NULL && n_names < 512) {
      size_t l = strlen(e->d_name);
      if (l > 4 && strcmp(e->d_name + l - 4, ".bin") == 0) names[n_names++] = strdup(e->d_name);
    }
    closedir(dir);
  }
  if (n_names == 0) {
    fprintf(stderr, "no descriptors in %s\n", argv[1]);
    return 2;
  }
  qsort(names, (size_t)n_names, sizeof names[0], by_name);
  int bad = 0;
  for (int k = 0; k < n_names; ++k) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", argv[1], names[k]);
    FILE* f = fopen(path, "rb");
    int32_t head[8];
    int ok = f && fread(head, 4, 8, f) == 8 && head[0] == 0x4A545348;
    if (!ok) {
      fprintf(stderr, "%s: unreadable\n", names[k]);
      return 2;
    }
    const size_t nt = (size_t)head[1], nn = (size_t)head[2];
    jade_scene_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = JADE_ABI_VERSION;
    d.n_triangles = head[1];
    d.n_nodes = head[2];
    d.n_emit = head[3];
    d.n_objects = head[4];
    d.env_width = head[5];
    d.env_height = head[6];
    jade_triangle* tris = (jade_triangle*)read_n(f, sizeof(jade_triangle), nt, &ok);
    void* nodes = read_n(f, sizeof(jade_bvh_node), nn, &ok);
    void* emit = read_n(f, 4, (size_t)head[3], &ok);
    void* mapping = read_n(f, 4, nt, &ok);
    void* prefix = read_n(f, 4, nt, &ok);
    void* segs = read_n(f, sizeof(jade_obj_seg), (size_t)head[4], &ok);
    void* env = read_n(f, 12, (size_t)head[5] * (size_t)head[6], &ok);
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) {
      fprintf(stderr, "%s: short file\n", names[k]);
      return 2;
    }
    d.triangles = tris;
    d.nodes = (const jade_bvh_node*)nodes;
    d.emit_indices = (const int32_t*)emit;
    d.index_mapping = (const int32_t*)mapping;
    d.prefix_area = (const float*)prefix;
    d.obj_segs = (const jade_obj_seg*)segs;
    d.env_rgb = (const float*)env;

    jade_scene* s = NULL;
    const int rc = jade_scene_create(&d, 0, &s);
    if (rc != head[7]) {
      fprintf(stderr, "%s: status %d, expected %d (%s)\n", names[k], rc, head[7], jade_last_error());
      ++bad;
    } else if (rc) {
      printf("%-28s refused (%d: %s)\n", names[k], rc, jade_last_error());
    } else {
      /* rays from around the scene's box towards points inside it (a plain LCG: the same rays on every run) */
      float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
      for (size_t t = 0; t < nt; ++t)
        for (int v = 0; v < 3; ++v)
          for (int a = 0; a < 3; ++a) {
            const float x = (&tris[t].p1[0])[3 * v + a];
            if (x < lo[a]) lo[a] = x;
            if (x > hi[a]) hi[a] = x;
          }
      enum { N = 256 };
      static float o[3 * N], dir3[3 * N], dist[N], dist2[N], pt[3 * N];
      static int32_t skip[N], hit[N], hit2[N];
      uint32_t lcg = 12345u;
      for (int i = 0; i < N; ++i) {
        for (int a = 0; a < 3; ++a) {
          lcg = lcg * 1664525u + 1013904223u;
          const float u = (float)(lcg >> 8) / 16777216.0f;
          lcg = lcg * 1664525u + 1013904223u;
          const float w = (float)(lcg >> 8) / 16777216.0f;
          o[3 * i + a] = lo[a] + (hi[a] - lo[a]) * (u * 1.6f - 0.3f);
          dir3[3 * i + a] = lo[a] + (hi[a] - lo[a]) * w - o[3 * i + a];
        }
        skip[i] = i % 4 == 0 ? (int32_t)((size_t)i % nt) : -1;
      }
      jade_stats st;
      memset(&st, 0, sizeof st);
      int r1 = jade_trace_rays(s, N, o, dir3, skip, hit, dist, pt, &st);
      jade_oracle_set_prune(5, 1.0f, 0.0f, 4.0f); /* the cached walk: subtrees one level above the leaf, four ways */
      int r2 = jade_trace_rays(s, N, o, dir3, skip, hit2, dist2, pt, &st);
      jade_render_params p;
      memset(&p, 0, sizeof p);
      p.width = p.height = 16;
      p.spp = 2;
      p.eye[0] = 0.5f * (lo[0] + hi[0]);
      p.eye[1] = 0.5f * (lo[1] + hi[1]) + 0.3f * (hi[1] - lo[1]);
      p.eye[2] = hi[2] + 0.8f * (hi[2] - lo[2]) + 1.0f;
      p.camera[0] = p.camera[5] = p.camera[10] = p.camera[15] = 1.0f; /* looking down -z */
      p.tile_nranks = 1;
      p.threads = 1;
      static float rgb[16 * 16 * 3];
      static uint8_t bgr[16 * 16 * 3];
      int r3 = jade_render(s, &p, rgb, bgr, &st);
      jade_oracle_set_prune(0, 0.0f, 0.0f, 0.0f);
      jade_oracle_occ_reset();
      /* (the probe tells a query's kind from the counters of the thread it runs on: what the second batch answers is a probe's
       * business, not a parity statement - it is here for what it reads) */
      int hits = 0;
      for (int i = 0; i < N; ++i) hits += hit[i] >= 0;
      if (r1 || r2 || r3) {
        fprintf(stderr, "%s: trace %d / %d, render %d (%s)\n", names[k], r1, r2, r3, jade_last_error());
        ++bad;
      } else {
        printf("%-28s %3d of %d rays hit; shadow %llu + environment %llu rays rendered with the cached walk\n", names[k], hits, N,
               (unsigned long long)st.rays_shadow, (unsigned long long)st.rays_env);
      }
      jade_scene_destroy(s);
    }
    free(tris); free(nodes); free(emit); free(mapping); free(prefix); free(segs); free(env);
  }
  for (int k = 0; k < n_names; ++k) free(names[k]);
  if (bad) {
    fprintf(stderr, "oracle_shapes: %d of %d descriptors failed\n", bad, n_names);
    return 1;
  }
  printf("oracle_shapes: %d descriptors, clean\n", n_names);
  return 0;
}
