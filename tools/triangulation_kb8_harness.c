/*
 * triangulation_kb8_harness.c -- SearchForTriangulation between two KannalaBrandt8 rig keyframes, the two routes of the library in one
 * process, wall time per call (upload, kernels, download and synchronisation included: both are per-call host entry points):
 *
 *   (a) orbm_search_for_triangulation_kb8: the epipolar test on the device;
 *   (b) orbm_search_for_triangulation_pred around a C predicate that evaluates KannalaBrandt8::TriangulateMatches on the host
 *       (orbm_fisheye_triangulate with n = 1, the library's host build of the same arithmetic, standing in for the reference's
 *       epipolarConstrain) - the route the adapter took before (a) existed, without a callback through an interpreter.
 *
 * Input: the scene file tools/triangulation_kb8_bench.py writes -
 *   int32  n1, n2, n_left1, n_left2, n_nodes1, n_nodes2, n_idx1, n_idx2, nlevels
 *   float  ep[2], cams1[2][8], cams2[2][8], T12[4][12], scale_factors[nlevels], level_sigma2[nlevels]
 *   per keyframe: keypoints[n] (28 bytes each), descriptors[n][32], has_mappoint[n], node_id[n_nodes], node_start[n_nodes + 1], node_idx[n_idx]
 * Legs alternate inside every round.  Exit status 1 if the two routes disagree on matches12.  One JSON line.
 *
 *   gcc -O2 -I include tools/triangulation_kb8_harness.c -o build/triangulation_kb8_harness -L 3_orb_slam3_selfnote_amd -lorbhip -Wl,-rpath,... -lm
 *   build/triangulation_kb8_harness scene.bin [--rounds 7] [--calls 20] [--warmup 5] [--only a|b]
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "orbhip.h"

static double now_ms(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}
static int cmp_d(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return x < y ? -1 : x > y; }

static void *take(FILE *f, size_t bytes) {
  void *p = malloc(bytes ? bytes : 1);
  if (!p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "scene file too short\n"); exit(2); }
  return p;
}

typedef struct {
  const orbm_keyframe_t *k1, *k2;
  int n_left1, n_left2;
  const float *cams1, *cams2, *T12;
  long evals;
} Pred;

/* ORBmatcher.cc:1115-1148 for a rig: the camera pair and pose of (bRight1, bRight2), then KannalaBrandt8::epipolarConstrain */
static int pred_call(void *user, int idx1, int idx2) {
  Pred *c = (Pred *)user;
  const int r1 = idx1 >= c->n_left1, r2 = idx2 >= c->n_left2;
  const orbx_keypoint_t *a = &c->k1->keys_un[idx1], *b = &c->k2->keys_un[idx2];
  const float kp1[2] = {a->x, a->y}, kp2[2] = {b->x, b->y};
  const float s1 = c->k1->level_sigma2[a->octave], s2 = c->k2->level_sigma2[b->octave];
  float depth = -1.f, p3D[3];
  c->evals++;
  if (orbm_fisheye_triangulate(1, kp1, kp2, &s1, &s2, c->T12 + 12 * (2 * r1 + r2), c->cams1 + 8 * r1, c->cams2 + 8 * r2, &depth, p3D) != 0) return 0;
  return depth > 0.0001f;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s scene.bin [--rounds R] [--calls C] [--warmup W] [--only a|b]\n", argv[0]); return 2; }
  int rounds = 7, calls = 20, warmup = 5;
  char only = 0;
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--rounds")) rounds = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--calls")) calls = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--warmup")) warmup = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--only")) only = argv[i + 1][0];
  }
  if (rounds < 1 || rounds > 1000 || calls < 1) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t *h = (int32_t *)take(f, 9 * sizeof(int32_t));
  const int n[2] = {h[0], h[1]}, n_left[2] = {h[2], h[3]}, n_nodes[2] = {h[4], h[5]}, n_idx[2] = {h[6], h[7]}, nlevels = h[8];
  if (n[0] < 0 || n[1] < 0 || n_nodes[0] < 0 || n_nodes[1] < 0 || n_idx[0] < 0 || n_idx[1] < 0 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return 2;
  float *ep = (float *)take(f, 2 * sizeof(float));
  float *cams1 = (float *)take(f, 16 * sizeof(float)), *cams2 = (float *)take(f, 16 * sizeof(float)), *T12 = (float *)take(f, 48 * sizeof(float));
  float *sf = (float *)take(f, (size_t)nlevels * sizeof(float)), *sigma2 = (float *)take(f, (size_t)nlevels * sizeof(float));
  orbm_keyframe_t k[2];
  for (int s = 0; s < 2; s++) {
    memset(&k[s], 0, sizeof(k[s]));
    k[s].n = n[s];
    k[s].keys_un = (const orbx_keypoint_t *)take(f, sizeof(orbx_keypoint_t) * (size_t)n[s]);
    k[s].descriptors = (const uint8_t *)take(f, 32 * (size_t)n[s]);
    k[s].has_mappoint = (const uint8_t *)take(f, (size_t)n[s]);
    k[s].n_nodes = n_nodes[s];
    k[s].node_id = (const uint32_t *)take(f, sizeof(uint32_t) * (size_t)n_nodes[s]);
    k[s].node_start = (const int32_t *)take(f, sizeof(int32_t) * ((size_t)n_nodes[s] + 1));
    k[s].node_idx = (const int32_t *)take(f, sizeof(int32_t) * (size_t)n_idx[s]);
    float *ur = (float *)malloc(sizeof(float) * ((size_t)n[s] + 1));      /* the predicate route wants mvuRight, all negative on a rig */
    for (int i = 0; i < n[s]; i++) ur[i] = -1.f;
    k[s].u_right = ur;
    k[s].scale_factors = sf; k[s].level_sigma2 = sigma2; k[s].nlevels = nlevels;
  }
  fclose(f);

  orbm_t *m = orbm_create(0);
  if (!m) { fprintf(stderr, "no usable HIP device (there is no fallback)\n"); return 3; }
  int32_t *ma = (int32_t *)malloc(sizeof(int32_t) * ((size_t)n[0] + 1)), *mb = (int32_t *)malloc(sizeof(int32_t) * ((size_t)n[0] + 1));
  Pred P = {&k[0], &k[1], n_left[0], n_left[1], cams1, cams2, T12, 0};
  int na = 0, nb = 0;
#define LEG_A() (na = orbm_search_for_triangulation_kb8(m, &k[0], n_left[0], &k[1], n_left[1], ep[0], ep[1], cams1, cams2, T12, 0, 0, 1, ma))
#define LEG_B() (nb = orbm_search_for_triangulation_pred(m, &k[0], &k[1], ep[0], ep[1], 0, 0, 0, 1, pred_call, &P, mb))
  for (int w = 0; w < warmup; w++) {
    if (only != 'b' && LEG_A() < 0) { fprintf(stderr, "kb8 route: %d %s\n", na, orbm_last_error(m)); return 3; }
    if (only != 'a' && LEG_B() < 0) { fprintf(stderr, "predicate route: %d %s\n", nb, orbm_last_error(m)); return 3; }
  }
  double *ta = (double *)calloc((size_t)rounds, sizeof(double)), *tb = (double *)calloc((size_t)rounds, sizeof(double));
  P.evals = 0;
  long timed_b = 0;
  for (int r = 0; r < rounds; r++) {
    if (only != 'b') {
      const double t0 = now_ms();
      for (int c = 0; c < calls; c++) LEG_A();
      ta[r] = (now_ms() - t0) / calls;
    }
    if (only != 'a') {
      const double t0 = now_ms();
      for (int c = 0; c < calls; c++) LEG_B();
      tb[r] = (now_ms() - t0) / calls;
      timed_b += calls;
    }
  }
  /* candidates in front of the test = evaluations of route (a) */
  int32_t *start = (int32_t *)malloc(sizeof(int32_t) * ((size_t)n[0] + 1));
  const int total = orbm_triangulation_candidates(m, &k[0], &k[1], ep[0], ep[1], 0, 0, start, NULL, NULL, 0);
  int lists = 0;
  for (int i = 0; i < n[0]; i++) lists += start[i + 1] > start[i];
  int differ = 0;
  if (!only) {
    differ = na != nb;
    for (int i = 0; i < n[0]; i++) differ |= ma[i] != mb[i];
  }
  qsort(ta, (size_t)rounds, sizeof(double), cmp_d);
  qsort(tb, (size_t)rounds, sizeof(double), cmp_d);
  printf("{\"n1\": %d, \"n2\": %d, \"n_left1\": %d, \"n_left2\": %d, \"nodes1\": %d, \"nodes2\": %d, \"rounds\": %d, \"calls_per_round\": %d, \"warmup\": %d, "
         "\"candidates\": %d, \"lists\": %d, \"matches_kb8\": %d, \"matches_pred\": %d, \"evals_kb8_per_call\": %d, \"evals_pred_per_call\": %.1f, "
         "\"kb8_ms_median\": %.4f, \"kb8_ms_min\": %.4f, \"kb8_ms_max\": %.4f, \"pred_ms_median\": %.4f, \"pred_ms_min\": %.4f, \"pred_ms_max\": %.4f, "
         "\"identical\": %s}\n",
         n[0], n[1], n_left[0], n_left[1], n_nodes[0], n_nodes[1], rounds, calls, warmup, total, lists, na, nb, total,
         timed_b ? (double)P.evals / (double)timed_b : 0.0, ta[rounds / 2], ta[0], ta[rounds - 1], tb[rounds / 2], tb[0], tb[rounds - 1],
         only ? "null" : differ ? "false" : "true");
  orbm_destroy(m);
  return differ ? 1 : 0;
}
