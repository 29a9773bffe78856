/*
 * ref_voc_selfcheck.cc -- a main() around ref_voc_driver.cc (TEST INFRASTRUCTURE).
 *
 * The driver hands raw pointers to and from the reference's vocabulary.  This program writes a small vocabulary file (k = 3, L = 2,
 * complete, one stop word, two equal descriptors among siblings), loads it with the reference's own loadFromTextFile - once as it is and
 * once with two trailing newlines - and runs every export once; `make -C oracle _ref/ref_voc_selfcheck` builds it, with the reference's
 * text, under the address and undefined-behaviour sanitizers.  It runs on the CPU only and is never loaded into Python.
 *
 * What the sanitizers do not see: on an empty line the loader reads `pid` and `nIsLeaf` uninitialised (TemplatedVocabulary.h:1389-1395,
 * the extractions fail at the stream's sentry).  Neither sanitizer flags the read of an indeterminate int; the parent and the flag of
 * such a node are printed here as this build made them, and nothing is concluded from them.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
void *refv_load(const char *path);
void refv_destroy(void *h);
void refv_params(const void *h, int32_t *out);
int refv_nodes(const void *h, uint32_t *parent, int32_t *n_children, uint32_t *word_id, double *weight, uint8_t *desc, uint8_t *flagged);
int refv_desc_stored(const char *path, int n_nodes, uint8_t *stored);
int refv_transform(const void *h, const uint8_t *desc, int n, int levelsup, uint32_t *bow_id, double *bow_val, int32_t *n_bow,
                   uint32_t *fv_node_id, int32_t *fv_start, int32_t *fv_idx, int32_t *n_fv);
int refv_transform_each(const void *h, const uint8_t *desc, int n, int levelsup, uint32_t *word, double *weight, uint32_t *nid);
}

#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "ref_voc_selfcheck: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                                \
    }                                                                          \
  } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static const int K = 3, NODES = 1 + 3 + 9;

/* node ids breadth-first: 1..3 under the root, 4..12 under them */
static void make_tree(uint8_t desc[][32], int parent[], int leaf[], double weight[]) {
  memset(desc[0], 0, 32);
  parent[0] = 0; leaf[0] = 0; weight[0] = 0;
  for (int i = 1; i < NODES; i++) {
    parent[i] = i <= K ? 0 : 1 + (i - 1 - K) / K;
    leaf[i] = i > K;
    weight[i] = leaf[i] ? 0.1 + 0.37 * i : 0.0;
    if (i <= K) {
      for (int b = 0; b < 32; b++) desc[i][b] = (uint8_t)(rnd() >> 24);
    } else {                          /* a child is its parent with six bits flipped, so a copy of it descends to it */
      memcpy(desc[i], desc[parent[i]], 32);
      for (int f = 0; f < 6; f++) {
        const uint32_t bit = (rnd() >> 8) % 256;
        desc[i][bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      }
    }
  }
  weight[6] = 0.0;                    /* a stop word */
  weight[4] = 0.1;
  memcpy(desc[8], desc[7], 32);       /* equal descriptors: the first wins */
}

static int write_file(const char *path, uint8_t desc[][32], const int parent[], const int leaf[], const double weight[], int newlines) {
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "%d %d %d %d\n", K, 2, 0, 0);
  for (int i = 1; i < NODES; i++) {
    fprintf(f, "%d %d", parent[i], leaf[i]);
    for (int b = 0; b < 32; b++) fprintf(f, " %d", desc[i][b]);
    fprintf(f, " %.17g", weight[i]);
    for (int k = 0; k < (i + 1 < NODES ? 1 : newlines); k++) fputc('\n', f);
  }
  fclose(f);
  return 0;
}

static int run(const char *path, int newlines, uint8_t desc[][32], const int parent[], const int leaf[], const double weight[]) {
  CHECK(write_file(path, desc, parent, leaf, weight, newlines) == 0);
  void *h = refv_load(path);
  CHECK(h != NULL);
  int32_t p[6];
  refv_params(h, p);
  const int n = p[4];
  CHECK(p[0] == K && p[1] == 2 && p[2] == 0 && p[3] == 0 && n == NODES + newlines);
  std::vector<uint32_t> par(n), wid(n);
  std::vector<int32_t> nch(n);
  std::vector<double> w(n);
  std::vector<uint8_t> d((size_t)n * 32), flagged(n), stored((size_t)n * 32);
  CHECK(refv_nodes(h, par.data(), nch.data(), wid.data(), w.data(), d.data(), flagged.data()) == n);
  CHECK(refv_desc_stored(path, n, stored.data()) == n - 1);
  int words = 0;
  for (int i = 1; i < NODES; i++) {
    CHECK((int)par[i] == parent[i] && flagged[i] == leaf[i] && w[i] == weight[i] && memcmp(&d[(size_t)i * 32], desc[i], 32) == 0);
    CHECK((int)wid[i] == (leaf[i] ? words : 0));
    words += leaf[i];
    for (int b = 0; b < 32; b++) CHECK(stored[(size_t)i * 32 + b] == 1);
  }
  for (int i = NODES; i < n; i++) {
    CHECK(w[i] == 0 && nch[i] == 0);
    for (int b = 0; b < 32; b++) CHECK(stored[(size_t)i * 32 + b] == 0);
    words += flagged[i] == 1;
    printf("ref_voc_selfcheck: empty line %d -> node %d: parent %u, flagged %d, word id %u (indeterminate reads, as this build made them)\n",
           i - NODES + 1, i, par[i], flagged[i], wid[i]);
  }
  CHECK(p[5] == words);

  /* queries: every node's descriptor twice (so word 0 of weight 0.1 is hit twice and the stop word too), and random ones */
  const int nq = 2 * (NODES - 1) + 8;
  std::vector<uint8_t> q((size_t)nq * 32);
  for (int i = 0; i < nq; i++) {
    if (i < 2 * (NODES - 1)) memcpy(&q[(size_t)i * 32], desc[1 + i / 2], 32);
    else for (int b = 0; b < 32; b++) q[(size_t)i * 32 + b] = (uint8_t)(rnd() >> 24);
  }
  int total_bow = 0, total_fv = 0;
  for (int levelsup = 0; levelsup <= 3; levelsup++) {
    std::vector<uint32_t> bow_id(nq), fv_node(nq), word(nq), nid(nq);
    std::vector<double> bow_val(nq), weight_of(nq);
    std::vector<int32_t> fv_start(nq + 1), fv_idx(nq);
    int32_t n_bow = -1, n_fv = -1;
    CHECK(refv_transform(h, q.data(), nq, levelsup, bow_id.data(), bow_val.data(), &n_bow, fv_node.data(), fv_start.data(), fv_idx.data(), &n_fv) == 0);
    CHECK(refv_transform_each(h, q.data(), nq, levelsup, word.data(), weight_of.data(), nid.data()) == 0);
    CHECK(n_bow > 0 && n_fv > 0 && fv_start[0] == 0);
    double sum = 0;
    for (int b = 0; b < n_bow; b++) {
      CHECK(b == 0 || bow_id[b - 1] < bow_id[b]);
      sum += bow_val[b];
    }
    CHECK(sum > 0.999999 && sum < 1.000001); /* L1_NORM */
    for (int g = 0; g < n_fv; g++) CHECK((g == 0 || fv_node[g - 1] < fv_node[g]) && fv_start[g] < fv_start[g + 1]);
    int live = 0;
    for (int i = 0; i < nq; i++) {
      live += weight_of[i] > 0;
      CHECK(nid[i] != 0xffffffffu);       /* a complete tree: *nid is written for every feature */
      CHECK(levelsup < 2 ? nid[i] != 0 : nid[i] == 0);
    }
    CHECK(fv_start[n_fv] == live);
    /* the copies of node 8's descriptor end in node 7 (the first of two equal distances), the copies of node 6 are stopped */
    CHECK(word[2 * 7] == 7 - 4 && word[2 * 6] == 7 - 4 && weight_of[2 * 5] == 0 && word[2 * 5] == 6 - 4);
    total_bow += n_bow;
    total_fv += n_fv;
  }
  /* n = 0 and a zero-length input */
  int32_t n_bow = -1, n_fv = -1, start0 = -1;
  uint32_t dummy_u = 0;
  double dummy_d = 0;
  int32_t dummy_i = 0;
  CHECK(refv_transform(h, q.data(), 0, 1, &dummy_u, &dummy_d, &n_bow, &dummy_u, &start0, &dummy_i, &n_fv) == 0);
  CHECK(n_bow == 0 && n_fv == 0 && start0 == 0);
  refv_destroy(h);
  printf("ref_voc_selfcheck: %d trailing newline(s): %d nodes, %d words, %d BowVector entries and %d FeatureVector nodes over 4 levelsups\n",
         newlines, n, p[5], total_bow, total_fv);
  return 0;
}

int main(int argc, char **argv) {
  static uint8_t desc[NODES][32];
  int parent[NODES], leaf[NODES];
  double weight[NODES];
  make_tree(desc, parent, leaf, weight);
  std::string path = std::string(argc > 1 ? argv[1] : "/tmp") + "/ref_voc_selfcheck.txt";
  if (run(path.c_str(), 0, desc, parent, leaf, weight)) return 1;
  if (run(path.c_str(), 2, desc, parent, leaf, weight)) return 1;
  remove(path.c_str());
  printf("ref_voc_selfcheck: ok\n");
  return 0;
}
