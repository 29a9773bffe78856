// orb_ref_kfdb.h -- the expressions of KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:814-926) and
// KeyFrameDatabase::DetectNBestCandidates (KeyFrameDatabase.cc:620-811) over DBoW2's L1Scoring::score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68, reached through TemplatedVocabulary.h:1202), stated once for the host entries
// orbd_query_reloc_host / orbd_query_place_host / orbd_accumulate_* and the kernels of orb_kfdb_kernels.h.  Held against the literal
// model of tests/kfdb_model.py; the reference's text itself is NOT compiled against it yet ("reference text unpinned").
// Integer counts, one float product, IEEE-754 double `-`, `+=`, fabs and `/ 2.0` in the reference's order, one double -> float
// conversion, float `+=` and one float product; no contraction, no libm call.
//
// The walk (:822-837, :639-671): the query's words in ascending id, each word's list in insertion order.  A keyframe whose stored
// query id differs from the query's is reset, marked and listed at its first encounter (the place form lists and marks it only when it
// is not connected to the query, :656); every encounter counts one common word.  A keyframe whose stored id EQUALS the query's is
// never listed again by that query (:829, :653).
// ORDER RULE (include/orbhip.h): the list's order is (smallest shared word id, add sequence).
// Gate (:843-861, :679-700): maxCommonWords over the listed keyframes, minCommonWords = maxCommonWords * 0.8f truncated to int,
// a keyframe is scored when its count is strictly greater.
// Score (ScoringObject.cpp:32-65): over the word ids present in both vectors, ascending, `score += fabs(vi - wi) - fabs(vi) - fabs(wi)`
// with vi of the QUERY (v1) and wi of the KEYFRAME (v2); then `-score / 2.0`, stored into a float (`float si`, :864, :704).
// Accumulation (:877-902, :719-744): in list order, accScore = si, then for each of at most 10 covisibles whose stored query id is
// the query's, `accScore += score of the neighbour` (a float add) and the neighbour replaces pBestKF when its score is strictly
// greater than bestScore.  Relocalisation keeps the entries with accScore > 0.75f * bestAccScore (:905-923), of the asked map, first
// occurrence only; the place form sorts by accScore descending, stable (:748, list::sort(compFirst)).
#pragma once
#include <stdint.h>

#define ORB_REF __host__ __device__ __forceinline__

// `int minCommonWords = maxCommonWords*0.8f;` (:850, :687): int -> float, a float product, truncation
ORB_REF int kfdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }
// `mnRelocWords>minCommonWords` (:861, :700)
ORB_REF bool kfdb_passes(int words, int min_common) { return words > min_common; }
// one term of ScoringObject.cpp:41, vi = the query's value, wi = the keyframe's: (fabs(vi - wi) - fabs(vi)) - fabs(wi)
ORB_REF double kfdb_l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
// `score += term` (:41)
ORB_REF void kfdb_l1_add(double *score, double term) { *score += term; }
// `score = -score/2.0` (:65) into `float si` (KeyFrameDatabase.cc:864, :704)
ORB_REF float kfdb_l1_finish(double score) { return (float)(-score / 2.0); }
// the key of the ORDER RULE; unique per keyframe, so any correct sort gives the list
ORB_REF uint64_t kfdb_order_key(uint32_t first_word, uint32_t seq) { return ((uint64_t)first_word << 32) | (uint64_t)seq; }
#define KFDB_NOT_LISTED 0xffffffffffffffffull   // sorts last

// `accScore+=pKF2->mRelocScore` (:891, :733)
ORB_REF void kfdb_acc_add(float *acc, float s) { *acc += s; }
// `pKF2->mRelocScore>bestScore` (:892, :734)
ORB_REF bool kfdb_beats(float s, float best) { return s > best; }
// `0.75f*bestAccScore` (:905) and `si>minScoreToRetain` (:912)
ORB_REF float kfdb_min_retain(float best_acc) { return 0.75f * best_acc; }
ORB_REF bool kfdb_retained(float acc, float min_retain) { return acc > min_retain; }

#undef ORB_REF
