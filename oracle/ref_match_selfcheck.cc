/*
 * ref_match_selfcheck.cc -- a main() around ref_match_driver.cc (TEST INFRASTRUCTURE).
 *
 * The driver hands many raw pointers to the reference's matcher.  This program runs every entry point once on a fixed tiny scene and
 * prints the match counts; `make -C oracle _ref/ref_match_selfcheck` builds it, with the reference's text, under the address and
 * undefined-behaviour sanitizers.  It runs on the CPU only and is never loaded into Python.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" {
struct refm_frame {
  int32_t N;
  const float *kx, *ky;
  const int32_t *octave;
  const float *angle;
  const uint8_t *desc;
  const float *uRight;
  float minX, maxX, minY, maxY;
  const float *scaleFactors;
  int32_t nlevels;
};
struct refm_keyframe {
  int N;
  const float *kx, *ky;
  const int32_t *octave;
  const float *angle;
  const uint8_t *desc;
  const float *uRight;
  const uint8_t *has_mp;
  int n_nodes;
  const uint32_t *node_id;
  const int32_t *node_start;
  const int32_t *node_idx;
  const float *scaleFactors, *levelSigma2;
};
int refm_descriptor_distance(const uint8_t *a, const uint8_t *b);
void refm_three_maxima(const int *sizes, int L, int *ind1, int *ind2, int *ind3);
float refm_radius_by_viewing_cos(float viewCos);
int refm_get_features_in_area(const refm_frame *f, float x, float y, float r, int minLevel, int maxLevel, int32_t *out);
int refm_search_by_projection_mp(const refm_frame *left, const refm_frame *right, const int32_t *leftToRight, const int32_t *rightToLeft, int nq,
                                 const uint8_t *in_view, const uint8_t *in_view_r, const uint8_t *bad, const float *trackDepth,
                                 const uint8_t *qdesc, const float *projX, const float *projY, const float *viewCos, const int32_t *level,
                                 const float *projXR, const float *projYR, const float *viewCosR, const int32_t *levelR, const uint8_t *qobs,
                                 float th, int bFarPoints, float thFarPoints, float nnratio, int32_t *slot, uint8_t *slot_obs);
int refm_search_by_projection_ff(const refm_frame *left, const refm_frame *right, int nLast, const uint8_t *has_mp, const float *Xw,
                                 const uint8_t *mpdesc, const int32_t *lastOctave, const float *lastAngle, const uint8_t *qobs, const float *Tcw,
                                 const float *Tlw, const float *Trl, int camType, const float *camParams, float mb, float mbf, float th, int bMono,
                                 int checkOri, int32_t *slot, uint8_t *slot_obs);
int refm_search_by_projection_kf(const refm_frame *cur, int nKF, const uint8_t *state, const float *Xw, const uint8_t *mpdesc, const float *kfAngle,
                                 const float *maxDist, const float *minDist, const float *Tcw, int camType, const float *camParams, float th,
                                 int ORBdist, int checkOri, int32_t *slot, uint8_t *slot_obs);
int refm_search_by_bow(const refm_keyframe *KF, const refm_keyframe *F, int Nleft, int kfNleft, float nnratio, int checkOri, int32_t *matchF);
int refm_search_for_initialization(int n1, const int32_t *octave1, const float *angle1, const uint8_t *desc1, const refm_frame *F2,
                                   float *prevMatched, int windowSize, float nnratio, int checkOri, int32_t *vnMatches12);
}

namespace {

uint32_t state = 12345u;
uint32_t next() { state = state * 1664525u + 1013904223u; return state >> 8; }
float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(next() & 0xffff) / 65536.f; }

/* N keypoints on a 16 x 8 lattice of an image, each with the descriptor of its lattice site and two flipped bits */
struct Image {
  std::vector<float> kx, ky, angle, uRight;
  std::vector<int32_t> octave;
  std::vector<uint8_t> desc;
  std::vector<float> sf;
  refm_frame rec;
  Image(int N, const std::vector<uint8_t> &sites, float shift) : kx(N), ky(N), angle(N), uRight(N, -1.f), octave(N), desc((size_t)N * 32), sf(8) {
    sf[0] = 1.f;
    for (int i = 1; i < 8; i++) sf[i] = sf[i - 1] * 1.2f;
    for (int i = 0; i < N; i++) {
      const int site = i % 128;
      kx[i] = 20.f + 45.f * (float)(site % 16) + uniform(-3, 3) + shift;
      ky[i] = 20.f + 55.f * (float)(site / 16) + uniform(-3, 3);
      octave[i] = (site % 3);
      angle[i] = uniform(0, 359);
      memcpy(&desc[(size_t)i * 32], &sites[(size_t)site * 32], 32);
      desc[(size_t)i * 32 + (next() % 32)] ^= (uint8_t)(1u << (next() % 8));
      desc[(size_t)i * 32 + (next() % 32)] ^= (uint8_t)(1u << (next() % 8));
      if (i % 2) uRight[i] = kx[i] - 10.f;
    }
    rec.N = N; rec.kx = kx.data(); rec.ky = ky.data(); rec.octave = octave.data(); rec.angle = angle.data(); rec.desc = desc.data();
    rec.uRight = uRight.data(); rec.minX = 0; rec.maxX = 752; rec.minY = 0; rec.maxY = 480; rec.scaleFactors = sf.data(); rec.nlevels = 8;
  }
};

}  // namespace

int main() {
  std::vector<uint8_t> sites(128 * 32);
  for (size_t i = 0; i < sites.size(); i++) sites[i] = (uint8_t)next();
  Image A(200, sites, 0.f), B(180, sites, 2.f);
  const int N = A.rec.N;

  /* the small members */
  int i1, i2, i3, sizes[30];
  for (int i = 0; i < 30; i++) sizes[i] = (int)(next() % 9);
  refm_three_maxima(sizes, 30, &i1, &i2, &i3);
  const int dd = refm_descriptor_distance(&sites[0], &sites[32]);
  const float rad = refm_radius_by_viewing_cos(0.9985f);
  std::vector<int32_t> area(N);
  const int na = refm_get_features_in_area(&A.rec, 300.f, 200.f, 120.f, 0, 1, area.data());

  /* map points seen from the identity pose: one per keypoint of A, projecting onto it */
  const float cam[4] = {400.f, 400.f, 376.f, 240.f};
  std::vector<float> Xw((size_t)N * 3), maxd(N), mind(N), projX(N), projY(N), projXR(N), viewCos(N, 0.9999f), depth(N), kfAngle(N);
  std::vector<int32_t> level(N);
  std::vector<uint8_t> in_view(N, 1), obs(N, 1), has_mp(N, 1), kfstate(N, 1), bad(N, 0);
  for (int i = 0; i < N; i++) {
    const float z = uniform(2.f, 9.f);
    Xw[3 * i] = (A.kx[i] - cam[2]) / cam[0] * z; Xw[3 * i + 1] = (A.ky[i] - cam[3]) / cam[1] * z; Xw[3 * i + 2] = z;
    const float d = sqrtf(Xw[3 * i] * Xw[3 * i] + Xw[3 * i + 1] * Xw[3 * i + 1] + z * z);
    maxd[i] = d * 1.5f; mind[i] = d * 0.3f; depth[i] = z;
    projX[i] = A.kx[i] + 1.f; projY[i] = A.ky[i] - 1.f; projXR[i] = A.uRight[i]; level[i] = A.octave[i];
    kfAngle[i] = A.angle[i] + 30.f;
    if (i % 17 == 0) { in_view[i] = 0; has_mp[i] = 2; kfstate[i] = 3; }
    if (i % 19 == 0) { obs[i] = 0; has_mp[i] = 0; kfstate[i] = 2; }
    if (i % 23 == 0) bad[i] = 1;
  }
  const float I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float Tlw[16];
  memcpy(Tlw, I4, sizeof(I4));
  Tlw[11] = 0.5f;
  const float Trl[12] = {1, 0, 0, -0.1f, 0, 1, 0, 0, 0, 0, 1, 0};

  std::vector<int32_t> slot(N + B.rec.N);
  std::vector<uint8_t> slot_obs(N + B.rec.N);
  auto reset = [&]() {
    for (size_t i = 0; i < slot.size(); i++) { slot[i] = (i % 11 == 0) ? 100000 + (int)i : -1; slot_obs[i] = (uint8_t)(i % 22 == 0); }
  };

  reset();
  const int n_mp = refm_search_by_projection_mp(&A.rec, NULL, NULL, NULL, N, in_view.data(), NULL, bad.data(), depth.data(), A.desc.data(),
                                                projX.data(), projY.data(), viewCos.data(), level.data(), projXR.data(), NULL, NULL, NULL, obs.data(),
                                                3.f, 1, 8.f, 0.8f, slot.data(), slot_obs.data());
  /* a rig: A left, B right, every fourth left keypoint with a right partner */
  std::vector<int32_t> l2r(N, -1), r2l(B.rec.N, -1), levelR(N);
  for (int i = 0; i < N && i / 4 < B.rec.N; i += 4) { l2r[i] = i / 4; r2l[i / 4] = i; }
  std::vector<float> pXR(N), pYR(N);
  for (int i = 0; i < N; i++) { pXR[i] = B.kx[i % B.rec.N]; pYR[i] = B.ky[i % B.rec.N]; levelR[i] = i % 7 == 0 ? -1 : B.octave[i % B.rec.N]; }
  reset();
  const int n_mp_rig = refm_search_by_projection_mp(&A.rec, &B.rec, l2r.data(), r2l.data(), N, in_view.data(), in_view.data(), NULL, NULL, A.desc.data(),
                                                    projX.data(), projY.data(), viewCos.data(), level.data(), pXR.data(), pYR.data(), viewCos.data(),
                                                    levelR.data(), obs.data(), 3.f, 0, 0.f, 0.8f, slot.data(), slot_obs.data());
  reset();
  const int n_ff = refm_search_by_projection_ff(&A.rec, NULL, N, has_mp.data(), Xw.data(), A.desc.data(), A.octave.data(), kfAngle.data(), obs.data(), I4,
                                                Tlw, NULL, 0, cam, 0.1f, 40.f, 7.f, 0, 1, slot.data(), slot_obs.data());
  reset();
  const int n_ff_rig = refm_search_by_projection_ff(&A.rec, &B.rec, N, has_mp.data(), Xw.data(), A.desc.data(), A.octave.data(), kfAngle.data(),
                                                    obs.data(), I4, Tlw, Trl, 0, cam, 0.1f, 0.f, 7.f, 0, 1, slot.data(), slot_obs.data());
  reset();
  const int n_kf = refm_search_by_projection_kf(&A.rec, N, kfstate.data(), Xw.data(), A.desc.data(), kfAngle.data(), maxd.data(), mind.data(), I4, 0, cam,
                                                10.f, 64, 1, slot.data(), slot_obs.data());

  /* BoW: node = lattice site / 8 */
  auto nodes = [](const Image &im, std::vector<uint32_t> &id, std::vector<int32_t> &start, std::vector<int32_t> &idx) {
    id.clear(); start.assign(1, 0); idx.clear();
    for (uint32_t node = 0; node < 16; node++) {
      for (int i = 0; i < im.rec.N; i++)
        if ((uint32_t)((i % 128) / 8) == node) idx.push_back(i);
      id.push_back(node * 3 + 1);
      start.push_back((int32_t)idx.size());
    }
  };
  std::vector<uint32_t> idA, idB;
  std::vector<int32_t> stA, stB, ixA, ixB;
  nodes(A, idA, stA, ixA);
  nodes(B, idB, stB, ixB);
  const refm_keyframe KA = {N, A.kx.data(), A.ky.data(), A.octave.data(), A.angle.data(), A.desc.data(), A.uRight.data(), has_mp.data(), (int)idA.size(),
                            idA.data(), stA.data(), ixA.data(), A.sf.data(), A.sf.data()};
  const refm_keyframe KB = {B.rec.N, B.kx.data(), B.ky.data(), B.octave.data(), B.angle.data(), B.desc.data(), B.uRight.data(), has_mp.data(),
                            (int)idB.size(), idB.data(), stB.data(), ixB.data(), B.sf.data(), B.sf.data()};
  std::vector<int32_t> matchF(B.rec.N);
  const int n_bow = refm_search_by_bow(&KA, &KB, -1, -1, 0.7f, 1, matchF.data());
  const int n_bow_rig = refm_search_by_bow(&KA, &KB, 100, 120, 0.7f, 1, matchF.data());

  std::vector<float> prev((size_t)N * 2);
  for (int i = 0; i < N; i++) { prev[2 * i] = A.kx[i]; prev[2 * i + 1] = A.ky[i]; }
  std::vector<int32_t> m12(N);
  const int n_init = refm_search_for_initialization(N, A.octave.data(), A.angle.data(), A.desc.data(), &B.rec, prev.data(), 30, 0.9f, 1, m12.data());

  printf("ref_match_selfcheck: maxima %d/%d/%d distance %d radius %.1f area %d | local %d rig %d | last-frame %d rig %d | keyframe %d | bow %d rig %d | "
         "initialization %d\n", i1, i2, i3, dd, rad, na, n_mp, n_mp_rig, n_ff, n_ff_rig, n_kf, n_bow, n_bow_rig, n_init);
  return (n_mp > 0 && n_mp_rig > 0 && n_ff > 0 && n_ff_rig > 0 && n_kf > 0 && n_bow > 0 && n_bow_rig > 0 && n_init > 0) ? 0 : 1;
}
