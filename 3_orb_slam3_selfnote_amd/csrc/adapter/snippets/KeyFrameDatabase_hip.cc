// KeyFrameDatabase_hip.cc -- drop-in bodies of KeyFrameDatabase::add, erase, clear, clearMap (src/KeyFrameDatabase.cc:39-98),
// KeyFrameDatabase::DetectNBestCandidates (src/KeyFrameDatabase.cc:620-811) and KeyFrameDatabase::DetectRelocalizationCandidates
// (src/KeyFrameDatabase.cc:814-926) over orbd_* of include/orbhip.h, against the reference's unmodified KeyFrameDatabase.h.
//
// Delete (or #if 0) those six members in src/KeyFrameDatabase.cc and add this file to the library's sources; the constructor,
// DetectLoopCandidates, DetectCandidates, DetectBestCandidates (no call site), PreSave, PostLoad and SetORBVocabulary stay.  The header
// has no room for a handle, so the handle of a database object is kept in a mutex-guarded side table for the life of the process.
// mvInvertedFile is still maintained by add / erase / clear / clearMap, so PreSave writes what the reference writes; after PostLoad has
// filled mvInvertedFile, call add() for every loaded keyframe once (it carries the keyframe's four members into the handle).
// A keyframe's tag is its pointer.  After every query the four members that only this class touches (mnRelocQuery, mRelocScore,
// mnPlaceRecognitionQuery, mPlaceRecognitionScore) are written back to the KeyFrames, so a saved map holds what the reference would
// save; mnRelocWords / mnPlaceRecognitionWords are scratch of one query and are not reproduced.
// The take loop of :760-783 never advances past a bad keyframe as the reference writes it (`continue` at :764-765 skips `i++; it++`):
// here a bad keyframe is SKIPPED instead of spun on.
// There is no CPU fallback: a failed orbd_* call throws.
#include <cstdlib>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "KeyFrameDatabase.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {

struct Side {
  orbd_t *d;
  std::set<KeyFrame *> live;
  std::mutex mu;
};

Side &side_of(const KeyFrameDatabase *db, const ORBVocabulary *voc) {
  static std::mutex mu;
  static std::map<const KeyFrameDatabase *, Side *> sides;
  std::lock_guard<std::mutex> lock(mu);
  std::map<const KeyFrameDatabase *, Side *>::iterator it = sides.find(db);
  if (it != sides.end()) return *it->second;
  const char *e = std::getenv("ORBHIP_DEVICE");
  Side *s = new Side;
  s->d = orbd_create((int)voc->size(), (int)voc->getScoringType(), ORBD_MAX_KEYFRAMES, e ? std::atoi(e) : 0);
  if (!s->d) throw std::runtime_error(std::string("KeyFrameDatabase: orbd_create failed (there is no CPU fallback): ") + orbd_last_error(NULL));
  sides[db] = s;
  return *s;
}

uint64_t tag_of(const KeyFrame *pKF) { return (uint64_t)(uintptr_t)pKF; }
KeyFrame *kf_of(uint64_t tag) { return (KeyFrame *)(uintptr_t)tag; }

void check(int rc, const char *what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + orbd_last_error(NULL));
}

void flatten(const DBoW2::BowVector &bow, std::vector<uint32_t> &id, std::vector<double> &val) {
  id.clear(); val.clear();
  for (DBoW2::BowVector::const_iterator vit = bow.begin(), vend = bow.end(); vit != vend; vit++) { id.push_back(vit->first); val.push_back(vit->second); }
}

// the four members back into the KeyFrames
void write_back(Side &s) {
  for (std::set<KeyFrame *>::iterator it = s.live.begin(); it != s.live.end(); ++it) {
    orbd_members_t m;
    check(orbd_get_members(s.d, tag_of(*it), &m), "orbd_get_members");
    (*it)->mnRelocQuery = m.reloc_query; (*it)->mRelocScore = m.reloc_score;
    (*it)->mnPlaceRecognitionQuery = m.place_query; (*it)->mPlaceRecognitionScore = m.place_score;
  }
}

// GetBestCovisibilityKeyFrames(10) of the scored keyframes only, at this moment, as the reference reads them (:880, :722)
void covisibles_of(const std::vector<uint64_t> &tags, int n, std::vector<uint64_t> &table) {
  table.assign((size_t)(n > 0 ? n : 1) * ORBD_COVISIBLES, ORBD_NO_TAG);
  for (int i = 0; i < n; i++) {
    const std::vector<KeyFrame *> vpNeighs = kf_of(tags[i])->GetBestCovisibilityKeyFrames(ORBD_COVISIBLES);
    for (size_t k = 0; k < vpNeighs.size() && k < (size_t)ORBD_COVISIBLES; k++) table[(size_t)i * ORBD_COVISIBLES + k] = tag_of(vpNeighs[k]);
  }
}

}  // namespace

void KeyFrameDatabase::add(KeyFrame *pKF) {
  unique_lock<mutex> lock(mMutex);
  Side &s = side_of(this, mpVoc);
  std::vector<uint32_t> id; std::vector<double> val;
  flatten(pKF->mBowVec, id, val);
  orbd_members_t m;
  m.reloc_query = pKF->mnRelocQuery; m.reloc_score = pKF->mRelocScore;
  m.place_query = pKF->mnPlaceRecognitionQuery; m.place_score = pKF->mPlaceRecognitionScore;
  check(orbd_add(s.d, tag_of(pKF), (uint64_t)(uintptr_t)pKF->GetMap(), id.data(), val.data(), (int)id.size(), &m), "orbd_add");
  std::lock_guard<std::mutex> l2(s.mu);
  s.live.insert(pKF);
  for (DBoW2::BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++)
    mvInvertedFile[vit->first].push_back(pKF);
}

void KeyFrameDatabase::erase(KeyFrame *pKF) {
  unique_lock<mutex> lock(mMutex);
  Side &s = side_of(this, mpVoc);
  std::lock_guard<std::mutex> l2(s.mu);
  if (s.live.erase(pKF)) check(orbd_erase(s.d, tag_of(pKF)), "orbd_erase");
  for (DBoW2::BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++)
    mvInvertedFile[vit->first].remove(pKF);   // add() files a keyframe once, so there is one entry to remove
}

void KeyFrameDatabase::clear() {
  Side &s = side_of(this, mpVoc);
  std::lock_guard<std::mutex> l2(s.mu);
  check(orbd_clear(s.d), "orbd_clear");
  s.live.clear();
  mvInvertedFile.clear();
  mvInvertedFile.resize(mpVoc->size());
}

void KeyFrameDatabase::clearMap(Map *pMap) {
  unique_lock<mutex> lock(mMutex);
  Side &s = side_of(this, mpVoc);
  std::lock_guard<std::mutex> l2(s.mu);
  // GetMap() is read now, as the reference reads it (:87): a merge may have moved keyframes since they were added
  for (std::set<KeyFrame *>::iterator it = s.live.begin(); it != s.live.end();) {
    if ((*it)->GetMap() == pMap) { check(orbd_erase(s.d, tag_of(*it)), "orbd_erase"); s.live.erase(it++); }
    else ++it;
  }
  for (std::vector<list<KeyFrame *> >::iterator vit = mvInvertedFile.begin(), vend = mvInvertedFile.end(); vit != vend; vit++)
    for (list<KeyFrame *>::iterator lit = vit->begin(); lit != vit->end();) {
      if ((*lit)->GetMap() == pMap) lit = vit->erase(lit);
      else ++lit;
    }
}

vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F, Map *pMap) {
  Side &s = side_of(this, mpVoc);
  std::vector<uint32_t> id; std::vector<double> val;
  flatten(F->mBowVec, id, val);
  int n = 0;
  std::vector<uint64_t> tags; std::vector<float> scores;
  {
    unique_lock<mutex> lock(mMutex);
    std::lock_guard<std::mutex> l2(s.mu);
    const int cap = orbd_size(s.d) + 1;
    tags.resize(cap); scores.resize(cap);
    int32_t mx = 0, mn = 0, nl = 0, ns = 0;
    check(orbd_query_reloc(s.d, F->mnId, id.data(), val.data(), (int)id.size(), tags.data(), scores.data(), cap, &ns, &mx, &mn, &nl), "orbd_query_reloc");
    n = ns;
    // the map a keyframe belongs to is read now (:915)
    for (int i = 0; i < n; i++) check(orbd_set_map(s.d, tags[i], (uint64_t)(uintptr_t)kf_of(tags[i])->GetMap()), "orbd_set_map");
  }
  if (n == 0) { std::lock_guard<std::mutex> l2(s.mu); write_back(s); return vector<KeyFrame *>(); }
  std::vector<uint64_t> table, out(n);
  covisibles_of(tags, n, table);
  for (size_t k = 0; k < table.size(); k++)
    if (table[k] != ORBD_NO_TAG) (void)orbd_set_map(s.d, table[k], (uint64_t)(uintptr_t)kf_of(table[k])->GetMap());   // unknown neighbours are skipped
  int32_t n_out = 0;
  check(orbd_accumulate_reloc(s.d, F->mnId, (uint64_t)(uintptr_t)pMap, tags.data(), scores.data(), n, table.data(), out.data(), &n_out), "orbd_accumulate_reloc");
  vector<KeyFrame *> vpRelocCandidates;
  vpRelocCandidates.reserve(n);
  for (int i = 0; i < n_out; i++) vpRelocCandidates.push_back(kf_of(out[i]));
  std::lock_guard<std::mutex> l2(s.mu);
  write_back(s);
  return vpRelocCandidates;
}

void KeyFrameDatabase::DetectNBestCandidates(KeyFrame *pKF, vector<KeyFrame *> &vpLoopCand, vector<KeyFrame *> &vpMergeCand, int nNumCandidates) {
  Side &s = side_of(this, mpVoc);
  std::vector<uint32_t> id; std::vector<double> val;
  flatten(pKF->mBowVec, id, val);
  int n = 0;
  std::vector<uint64_t> tags; std::vector<float> scores;
  {
    unique_lock<mutex> lock(mMutex);
    std::lock_guard<std::mutex> l2(s.mu);
    const std::set<KeyFrame *> spConnectedKF = pKF->GetConnectedKeyFrames();
    std::vector<uint64_t> connected;
    for (std::set<KeyFrame *>::const_iterator it = spConnectedKF.begin(); it != spConnectedKF.end(); ++it)
      if (s.live.count(*it)) connected.push_back(tag_of(*it));   // a connected keyframe outside the database is in no list
    const int cap = orbd_size(s.d) + 1;
    tags.resize(cap); scores.resize(cap);
    int32_t mx = 0, mn = 0, nl = 0, ns = 0;
    check(orbd_query_place(s.d, pKF->mnId, connected.data(), (int)connected.size(), id.data(), val.data(), (int)id.size(), tags.data(), scores.data(),
                           cap, &ns, &mx, &mn, &nl), "orbd_query_place");
    n = ns;
  }
  if (n == 0) { std::lock_guard<std::mutex> l2(s.mu); write_back(s); return; }
  std::vector<uint64_t> table, best(n);
  std::vector<float> acc(n);
  covisibles_of(tags, n, table);
  check(orbd_accumulate_place(s.d, pKF->mnId, tags.data(), scores.data(), n, table.data(), acc.data(), best.data()), "orbd_accumulate_place");
  vpLoopCand.reserve(nNumCandidates);
  vpMergeCand.reserve(nNumCandidates);
  set<KeyFrame *> spAlreadyAddedKF;
  for (int i = 0; i < n && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates); i++) {
    KeyFrame *pKFi = kf_of(best[i]);
    if (pKFi->isBad()) continue;   // skipped, not spun on (:764-765)
    if (!spAlreadyAddedKF.count(pKFi)) {
      if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) vpLoopCand.push_back(pKFi);
      else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);
      spAlreadyAddedKF.insert(pKFi);
    }
  }
  std::lock_guard<std::mutex> l2(s.mu);
  write_back(s);
}

}  // namespace ORB_SLAM3
