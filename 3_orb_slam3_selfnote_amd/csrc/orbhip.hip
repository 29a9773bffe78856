// orbhip.hip -- liborbhip.so: host side of the C ABI in include/orbhip.h + kernel launches.
//
// Build (see 3_orb_slam3_selfnote_amd/build.py):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared orbhip.hip -o liborbhip.so
// -ffp-contract=off is part of the contract: the reference arithmetic is unfused IEEE.
//
// There is deliberately no CPU fallback in this file: every entry point that computes runs HIP kernels and returns
// ORBX_E_HIP when no device is usable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <type_traits>
#include <initializer_list>
#include <mutex>
#include <map>
#include <chrono>

#include "../../include/orbhip.h"
#include "orb_kernels.h"
#include "orb_match_kernels.h"
#include "orb_match_mfma.h"
#include "orb_project_kernels.h"
#include "orb_stereo_kernels.h"
#include "orb_depth_kernels.h"
#include "orb_rig_stereo_kernels.h"
#include "orb_newpoints_kernels.h"
#include "orb_fuse_kernels.h"
#include "orb_fuse_sim3_kernels.h"
#include "orb_bow_kernels.h"
#include "orb_mappoint_kernels.h"
#include "orb_culling_kernels.h"
#include "orb_localmap_kernels.h"
#include "orb_twoview_kernels.h"
#include "orb_sim3_kernels.h"
#include "orb_voc_kernels.h"
#include "orb_kfdb_kernels.h"

static_assert(sizeof(orbx_keypoint_t) == 28, "cv::KeyPoint layout");
static_assert(sizeof(KpOut) == 28, "cv::KeyPoint layout");

namespace {

inline int cv_round(double v) { return (int)lrint(v); }  // cvRound: round-half-even
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define PROF_DEPTH 32   // batches whose stage events are kept for orbx_get_stage_ms / orbm_get_stage_ms (averaged)

// ORBHIP_TRACE_ALLOC=1: every growth of a device / pinned buffer is reported on stderr with the time its free and its allocation took
// (diagnostic: a re-allocation inside the per-frame path is a latency spike of tens of milliseconds)
static bool trace_alloc() { static const bool on = getenv("ORBHIP_TRACE_ALLOC") != nullptr; return on; }
static double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t need) {
    if (need <= bytes) return hipSuccess;
    const double t0 = trace_alloc() ? wall_ms() : 0.0;
    if (p) (void)hipFree(p);
    const double t1 = trace_alloc() ? wall_ms() : 0.0;
    p = nullptr;
    const size_t old = bytes;
    bytes = 0;
    hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    if (trace_alloc()) fprintf(stderr, "orbhip-alloc: device buffer %zu -> %zu bytes: hipFree %.3f ms, hipMalloc %.3f ms\n", old, need, t1 - t0, wall_ms() - t1);
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

}  // namespace

// --------------------------------------------------------------------------------------------------------------
// extractor handle
// --------------------------------------------------------------------------------------------------------------
struct orbx_handle {
  int device = 0;
  // ORBextractor members (ORBextractor.h:95-109)
  int nfeatures = 0, nlevels = 0, iniThFAST = 0, minThFAST = 0;
  double scaleFactor = 0;
  std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
  std::vector<int> mnFeaturesPerLevel;
  int umax[ORB_HALF_PATCH + 1];
  // configured geometry
  int rows = 0, cols = 0, max_batch = 0;
  std::vector<LevelGeom> geom;
  size_t pyr_fs = 0, blur_fs = 0, slot_fs = 0;
  bool octCellsLds = false;
  bool octCodes = false;   // k_octree runs its rounds on the nodes alone (code tables in d_octTab)
  size_t octHead = 0;      // bytes of k_octree's first LDS region: chcnt / chpos, or the code form's counts and map
  int chainTiles = 0, chainBuf0 = 0, chainBuf1 = 0;   // k_pyramid_chain (single-frame calls); chainTiles = 0: not available
  size_t chainLds = 0;
  size_t octLds = 0;
  int cell_fs = 0, cand_fs = 0, lkp_fs = 0, totalTiles = 0, totalCells = 0, totalGroups = 0, totalKp = 0, octCap = 0;
  int maxKeypoints = 0;
  // device memory
  DevBuf d_pyr, d_blur, d_cellCnt, d_cellOff, d_slots, d_cand, d_knode, d_lkp, d_lrank, d_lcnt, d_candCnt, d_fastRecs, d_resizeRecs, d_tiles, d_xtab,
      d_ytab, d_disc, d_chain, d_octTab;
  DevBuf d_img, d_okps;  // staging for the host entry point (d_okps: counts + keypoints + descriptors, one block)
  hipStream_t stream = nullptr;
  float host_us[4] = {0, 0, 0, 0};          // orbx_extract's last call: staging copy, submission, wait, copy-out (orbx_get_host_us)
  // last call
  FrameParams last{};
  bool have_last = false;
  hipEvent_t last_done = nullptr;   // recorded on the extraction's stream behind its last kernel (asynchronous entry point only)
  bool last_pending = false;        // ... and not yet known to have completed
  bool in_capture = false;          // orbx_extract is capturing its per-frame graph: nothing but the frame's own work is enqueued
  DevBuf stereo[7];  // grow-only buffers of orbx_compute_stereo_matches
  DevBuf stereo_batch[3];  // ... of orbx_compute_stereo_matches_batch_device: row-table records, band starts, SADs
  DevBuf maps[2];    // rectification maps of orbx_remap_linear, kept between calls
  int maps_rows = 0, maps_cols = 0;
  // pinned host staging of the single-frame entry point (orbx_extract): pageable copies would serialise on HIP's own staging
  void *pin_in = nullptr, *pin_out = nullptr;
  size_t pin_in_bytes = 0, pin_out_bytes = 0;
  DevBuf d_pyrpack; void *pin_pyr = nullptr; size_t pin_pyr_bytes = 0;   // orbx_download_pyramid: bordered levels, packed
  // the per-frame sequence of orbx_extract (H2D, 5 launches, 1 D2H) captured once per configuration as a hipGraph:
  // one submission per frame instead of 7
  hipGraphExec_t graph = nullptr;
  struct { int rows = 0, cols = 0, lap0 = 0, lap1 = 0, icap = 0; const void *pin_in = nullptr, *pin_out = nullptr, *d_img = nullptr, *d_okps = nullptr, *d_pyr = nullptr; } graph_key;
  bool graph_ok = true;   // cleared (for good) if capture / instantiation fails: the plain path is used instead
  // profiling
  bool profiling = false;
  hipEvent_t ev[PROF_DEPTH][6] = {};   // ring of event sets: one per batch since profiling was switched on
  int prof_head = 0;                   // batches recorded since then
  bool ev_ok = false;
  float stage_ms[5] = {0, 0, 0, 0, 0};
  bool stage_valid = false;
  std::string err;
};

// Synchronous copies go through the handle's own non-blocking stream, never through the legacy default stream: another host
// thread may be capturing its per-frame graph (orbx_extract), and a legacy-stream operation would implicitly join - and
// invalidate - that capture ("operation would make the legacy stream depend on a capturing blocking stream").
static hipError_t copy_on(hipStream_t s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}
// waits (on the handle's stream) for the last extraction of this handle, whatever stream it ran on
static hipError_t join_last(orbx_handle *h) {
  if (h->last_pending) { hipError_t e = hipStreamWaitEvent(h->stream, h->last_done, 0); if (e != hipSuccess) return e; }
  return hipStreamSynchronize(h->stream);
}

#define XCHECK(h, call)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return ORBX_E_HIP;                                                                      \
    }                                                                                         \
  } while (0)

// The dynamic-LDS limit is an attribute of the kernel FUNCTION (per device), not of a handle or a launch: handles on
// several host threads (Tracking / LocalMapping / LoopClosing each own a matcher, stereo runs two extractors) would race
// a per-launch "set to this launch's size" against each other's launches.  It is raised once per device, to the CU's whole
// 160 KiB (ORB_LDS_LIMIT, orb_lds.h), for every kernel that can ask for more than the 64 KiB default; launches only check their own
// size against it.
struct LdsOnce { std::mutex mu; bool done[64] = {}; };   // the once-table of one kernel list
static hipError_t raise_lds_once(LdsOnce &once, int device, std::initializer_list<const void *> fns) {
  std::lock_guard<std::mutex> lock(once.mu);
  if (device < 0 || device >= 64) return hipErrorInvalidDevice;
  if (once.done[device]) return hipSuccess;
  for (const void *fn : fns) {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, fn);
    if (e != hipSuccess) return e;
    const int room = ORB_LDS_LIMIT - (int)a.sharedSizeBytes;   // static __shared__ of the kernel counts against the same 160 KiB
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, room);
    if (e != hipSuccess) return e;
  }
  once.done[device] = true;
  return hipSuccess;
}
static hipError_t raise_lds_limits(int device) {
  static LdsOnce once;
  return raise_lds_once(once, device, {reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_PLAIN, 1>), reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_UR, 1>),
                       reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_FISHEYE, 1>), reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_FUSE, 1>),
                       reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_PLAIN, 4>), reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_UR, 4>),
                       reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_FISHEYE, 4>), reinterpret_cast<const void *>(&k_match_walk<Key32, SCAN_FUSE, 4>),
                       reinterpret_cast<const void *>(&k_octree<256, true>), reinterpret_cast<const void *>(&k_octree<256, false>),
                       reinterpret_cast<const void *>(&k_octree<1024, true>), reinterpret_cast<const void *>(&k_octree<1024, false>),
                       reinterpret_cast<const void *>(&k_resize),
                       reinterpret_cast<const void *>(&k_match_resolve<Key32, true>), reinterpret_cast<const void *>(&k_match_resolve<Key32, false>),
                       reinterpret_cast<const void *>(&k_match_resolve<Key64, true>), reinterpret_cast<const void *>(&k_match_resolve<Key64, false>),
                       reinterpret_cast<const void *>(&k_match_resolve<Key32, true, true>), reinterpret_cast<const void *>(&k_pyramid_chain)});
}

// The device builds of the scalar replicas on n items (orbx_logf_device, orbx_tanf_device, orbx_cosf_device .. orbx_fast_atan2_device):
// out[i] = F()(in[i]...), where each functor calls the inline function the production kernels call.  tests/test_gpu_libm_device.py
// (logf: tests/test_gpu_local_points.py, tanf: tests/test_gpu_rig_stereo.py) compares the results with the host builds, with the host
// libm and with the oracle's fastAtan2.
struct EvalCosf { __device__ float operator()(float x) const { return orbsc::ref_cosf(x); } };
struct EvalSinf { __device__ float operator()(float x) const { return orbsc::ref_sinf(x); } };
struct EvalAtanf { __device__ float operator()(float x) const { return orbat::ref_atanf(x); } };
struct EvalLogf { __device__ float operator()(float x) const { return orblg::ref_logf(x); } };
struct EvalTanf { __device__ float operator()(float x) const { return orbtn::ref_tanf(x); } };
struct EvalAtan2f { __device__ float operator()(float y, float x) const { return orbat::ref_atan2f(y, x); } };
struct EvalFastAtan2 { __device__ float operator()(float y, float x) const { return fast_atan2_deg(y, x); } };
template <class F, class... In>
__global__ __launch_bounds__(256) void k_eval(uint32_t n, float *out, In... in) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = F()(in[i]...);
}
template <class F, class... In>
static int eval_device(int n, float *d_out, void *stream, In... d_in) {
  if (n < 0 || (n > 0 && (!d_out || (!d_in || ...)))) return ORBX_E_ARG;
  if (n == 0) return 0;
  hipLaunchKernelGGL((k_eval<F, In...>), dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, d_out, d_in...);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

extern "C" {

float orbx_ref_cosf(float x) { return orbsc::ref_cosf(x); }
float orbx_ref_sinf(float x) { return orbsc::ref_sinf(x); }
float orbx_ref_atanf(float x) { return orbat::ref_atanf(x); }
float orbx_ref_atan2f(float y, float x) { return orbat::ref_atan2f(y, x); }
float orbx_ref_logf(float x) { return orblg::ref_logf(x); }
float orbx_ref_tanf(float x) { return orbtn::ref_tanf(x); }
int orbx_tanf_device(const float *d_x, int n, float *d_y, void *stream) { return eval_device<EvalTanf>(n, d_y, stream, d_x); }
int orbx_logf_device(const float *d_x, int n, float *d_y, void *stream) { return eval_device<EvalLogf>(n, d_y, stream, d_x); }
int orbx_cosf_device(const float *d_x, int n, float *d_y, void *stream) { return eval_device<EvalCosf>(n, d_y, stream, d_x); }
int orbx_sinf_device(const float *d_x, int n, float *d_y, void *stream) { return eval_device<EvalSinf>(n, d_y, stream, d_x); }
int orbx_atanf_device(const float *d_x, int n, float *d_y, void *stream) { return eval_device<EvalAtanf>(n, d_y, stream, d_x); }
int orbx_atan2f_device(const float *d_yin, const float *d_xin, int n, float *d_out, void *stream) {
  return eval_device<EvalAtan2f>(n, d_out, stream, d_yin, d_xin);
}
int orbx_fast_atan2_device(const float *d_yin, const float *d_xin, int n, float *d_out, void *stream) {
  return eval_device<EvalFastAtan2>(n, d_out, stream, d_yin, d_xin);
}

orbx_t *orbx_create(int nfeatures, float scaleFactor_, int nlevels, int iniThFAST, int minThFAST, int device) {
  if (nfeatures < 0 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scaleFactor_ > 1.0f)) return nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
  if (hipSetDevice(device) != hipSuccess || raise_lds_limits(device) != hipSuccess) return nullptr;
  orbx_handle *h = new orbx_handle();
  h->device = device;
  h->nfeatures = nfeatures;
  h->nlevels = nlevels;
  h->iniThFAST = std::min(std::max(iniThFAST, 0), 255);  // cv::FAST clamps the threshold to [0,255]
  h->minThFAST = std::min(std::max(minThFAST, 0), 255);
  h->scaleFactor = (double)scaleFactor_;  // double member initialised from float, ORBextractor.h:96
  // ORBextractor.cc:413-429
  h->mvScaleFactor.resize(nlevels);
  h->mvLevelSigma2.resize(nlevels);
  h->mvInvScaleFactor.resize(nlevels);
  h->mvInvLevelSigma2.resize(nlevels);
  h->mvScaleFactor[0] = 1.0f;
  h->mvLevelSigma2[0] = 1.0f;
  for (int i = 1; i < nlevels; i++) {
    h->mvScaleFactor[i] = (float)((double)h->mvScaleFactor[i - 1] * h->scaleFactor);
    h->mvLevelSigma2[i] = h->mvScaleFactor[i] * h->mvScaleFactor[i];
  }
  for (int i = 0; i < nlevels; i++) {
    h->mvInvScaleFactor[i] = 1.0f / h->mvScaleFactor[i];
    h->mvInvLevelSigma2[i] = 1.0f / h->mvLevelSigma2[i];
  }
  // per-level quotas, ORBextractor.cc:432-444
  h->mnFeaturesPerLevel.resize(nlevels);
  const float factor = (float)(1.0 / h->scaleFactor);
  float nDesired = (float)nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
  int sum = 0;
  for (int l = 0; l < nlevels - 1; l++) {
    h->mnFeaturesPerLevel[l] = cv_round(nDesired);
    sum += h->mnFeaturesPerLevel[l];
    nDesired *= factor;
  }
  h->mnFeaturesPerLevel[nlevels - 1] = std::max(nfeatures - sum, 0);
  // circular patch row ends, ORBextractor.cc:452-467
  {
    int v, v0;
    const int vmax = (int)floor(ORB_HALF_PATCH * sqrtf(2.f) / 2 + 1);
    const int vmin = (int)ceil(ORB_HALF_PATCH * sqrtf(2.f) / 2);
    const double hp2 = ORB_HALF_PATCH * ORB_HALF_PATCH;
    for (v = 0; v <= ORB_HALF_PATCH; v++) h->umax[v] = 0;
    for (v = 0; v <= vmax; ++v) h->umax[v] = cv_round(sqrt(hp2 - v * v));
    for (v = ORB_HALF_PATCH, v0 = 0; v >= vmin; --v) {
      while (h->umax[v0] == h->umax[v0 + 1]) ++v0;
      h->umax[v] = v0;
      ++v0;
    }
  }
  std::vector<int8_t> disc;
  for (int v = -ORB_HALF_PATCH; v <= ORB_HALF_PATCH; v++) {
    const int d = h->umax[v < 0 ? -v : v];
    for (int u = -d; u <= d; u++) { disc.push_back((int8_t)u); disc.push_back((int8_t)v); }
  }
  if ((int)disc.size() != 2 * ORB_DISC_PIXELS) { delete h; return nullptr; }
  {
    const DiscTab ref = make_disc_tab();  // the kernels' compile-time table must equal what ORBextractor.cc:452-467 derives
    for (int i = 0; i < ORB_DISC_PIXELS; i++) {
      const int lane = i & 63, k = i >> 6;
      const int8_t u = (int8_t)(ref.w[lane][k >> 2] >> (8 * (k & 3))), v = (int8_t)(ref.w[lane][3 + (k >> 2)] >> (8 * (k & 3)));
      if (u != disc[2 * i] || v != disc[2 * i + 1]) { delete h; return nullptr; }
    }
  }
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return nullptr; }
  if (h->d_disc.reserve(disc.size()) != hipSuccess ||
      copy_on(h->stream, h->d_disc.p, disc.data(), disc.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipStreamDestroy(h->stream);
    delete h;
    return nullptr;
  }
  return h;
}

void orbx_destroy(orbx_t *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  DevBuf *bufs[] = {&h->d_pyr, &h->d_blur, &h->d_cellCnt, &h->d_cellOff, &h->d_slots, &h->d_cand, &h->d_knode, &h->d_lkp,
                    &h->d_lrank, &h->d_lcnt, &h->d_candCnt, &h->d_fastRecs, &h->d_resizeRecs, &h->d_tiles, &h->d_xtab, &h->d_ytab, &h->d_disc, &h->d_chain, &h->d_octTab, &h->d_img, &h->d_okps};
  for (DevBuf *b : bufs) b->release();
  for (DevBuf &b : h->stereo) b.release();
  for (DevBuf &b : h->stereo_batch) b.release();
  for (DevBuf &b : h->maps) b.release();
  if (h->graph) (void)hipGraphExecDestroy(h->graph);
  if (h->last_done) (void)hipEventDestroy(h->last_done);
  if (h->pin_in) (void)hipHostFree(h->pin_in);
  if (h->pin_pyr) (void)hipHostFree(h->pin_pyr);
  h->d_pyrpack.release();
  if (h->pin_out) (void)hipHostFree(h->pin_out);
  if (h->ev_ok)
    for (auto &set : h->ev)
      for (auto &e : set) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

const char *orbx_last_error(const orbx_t *h) { return h ? h->err.c_str() : "null handle"; }
int orbx_get_levels(const orbx_t *h) { return h ? h->nlevels : ORBX_E_ARG; }
float orbx_get_scale_factor(const orbx_t *h) { return h ? (float)h->scaleFactor : 0.f; }

int orbx_get_scale_tables(const orbx_t *h, float *sf, float *isf, float *s2, float *is2) {
  if (!h) return ORBX_E_ARG;
  for (int i = 0; i < h->nlevels; i++) {
    if (sf) sf[i] = h->mvScaleFactor[i];
    if (isf) isf[i] = h->mvInvScaleFactor[i];
    if (s2) s2[i] = h->mvLevelSigma2[i];
    if (is2) is2[i] = h->mvInvLevelSigma2[i];
  }
  return h->nlevels;
}

int orbx_get_features_per_level(const orbx_t *h, int *n) {
  if (!h || !n) return ORBX_E_ARG;
  for (int i = 0; i < h->nlevels; i++) n[i] = h->mnFeaturesPerLevel[i];
  return h->nlevels;
}

// floor(2^32 / n) for xcd_map's division by multiplication (n == 1: the estimate q-1 is corrected on the device)
static uint32_t magic_div(uint32_t n) { return n <= 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / n); }

#if defined(FAST_STAMPS) || defined(OCT_STAMPS) || defined(TILE_STAMPS)
// diagnostic builds only (tools/fast_stamps.py, tools/octree_stamps.py, tools/tile_stamps.py): device buffer [workgroups][8] of u32 cycle stamps
int orbx_debug_fast_stamps(void *d_buf) {
  unsigned int *p = (unsigned int *)d_buf;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_fast_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

int orbx_max_keypoints(const orbx_t *h) { return h ? h->maxKeypoints : ORBX_E_ARG; }

// k_resize's form for level G from level Gs.  Two-pass form (rows and their horizontal interpolation staged in LDS) whenever a tile's
// source rows fit the stage and pass 1's precondition holds (two neighbouring columns' source bytes inside one aligned 8-byte window:
// horizontal scale factor below 3): returns the pitch of the interpolated rows.  Otherwise the one-pass form straight from global
// memory, which stages the x table only: returns 0.
static int resize_form(const LevelGeom &G, const LevelGeom &Gs) {
  const int wq = (G.w + 3) & ~3, tPitch2 = resize_t_pitch(wq);
  const bool twoPass = G.resizeSrcRows <= RESIZE_MAXSRC && (double)Gs.w / G.w < 3.0 &&
                       ResizeCarve::of(G.resizeSrcRows, resize_row_bytes(Gs.w), tPitch2, wq).bytes <= RESIZE_LDS_MAX;   // (very wide images: one-pass)
  return twoPass ? tPitch2 : 0;
}

int orbx_configure(orbx_t *h, int rows, int cols, int max_batch) {
  if (!h || rows <= 0 || cols <= 0 || max_batch <= 0) return ORBX_E_ARG;
  if (rows > 4096 || cols > 4096) { h->err = "image larger than 4096x4096 (12-bit packed coordinates)"; return ORBX_E_ARG; }
  if (max_batch > 65535) { h->err = "batch larger than 65535"; return ORBX_E_ARG; }
  if (h->rows == rows && h->cols == cols && h->max_batch >= max_batch) return h->maxKeypoints;
  XCHECK(h, hipSetDevice(h->device));
  XCHECK(h, hipStreamSynchronize(h->stream));
  const int nl = h->nlevels;
  std::vector<LevelGeom> g(nl);
  std::vector<int2> xtab, ytab;
  std::vector<uint32_t> resizerec;   // k_resize's row-tile records
  size_t pyr = 0, blur = 0;
  int cells = 0, slots = 0, kps = 0, tiles = 0, octCap = 8;
  for (int l = 0; l < nl; l++) {
    LevelGeom &G = g[l];
    memset(&G, 0, sizeof(G));
    const float inv = h->mvInvScaleFactor[l];
    G.w = cv_round((float)cols * inv);  // ORBextractor.cc:1192-1193
    G.h = cv_round((float)rows * inv);
    if (G.w < 1 || G.h < 1) { h->err = "pyramid level collapses to zero size"; return ORBX_E_ARG; }
    G.pitch = (int)align_up((size_t)G.w, 64);
    G.bpitch = G.pitch;
    G.off = pyr;
    if (l > 0) pyr += align_up((size_t)G.pitch * G.h, 256);
    G.boff = blur;
    blur += align_up((size_t)G.bpitch * G.h, 256);
    // FAST grid, ORBextractor.cc:771-785
    G.maxBorderX = G.w - ORB_EDGE_THRESHOLD + 3;
    G.maxBorderY = G.h - ORB_EDGE_THRESHOLD + 3;
    const float width = (float)(G.maxBorderX - ORB_MIN_BORDER), height = (float)(G.maxBorderY - ORB_MIN_BORDER);
    const float W = 30;
    int nCols = width > 0 ? (int)(width / W) : 0, nRows = height > 0 ? (int)(height / W) : 0;
    if (nCols <= 0 || nRows <= 0) {  // the reference divides by zero here; defined as "no keypoints on this level"
      nCols = nRows = 0;
      G.wCell = G.hCell = 1;
    } else {
      G.wCell = (int)ceilf(width / nCols);
      G.hCell = (int)ceilf(height / nRows);
    }
    G.nCols = nCols;
    G.nRows = nRows;
    G.cellCap = ((G.wCell + 1) / 2) * ((G.hCell + 1) / 2);
    G.cellBase = cells;
    G.slotBase = slots;
    G.candBase = slots;
    G.candCap = nCols * nRows * G.cellCap;
    cells += nCols * nRows;
    slots += G.candCap;
    // octree, ORBextractor.cc:541-543
    G.N = h->mnFeaturesPerLevel[l];
    G.nIni = 0;
    G.hX = 1.f;
    if (nCols > 0) {
      G.nIni = (int)roundf(width / height);
      if (G.nIni < 1) { h->err = "level taller than 2x its width: the reference's DistributeOctTree has no root node"; return ORBX_E_ARG; }
      if (G.nIni > 64) { h->err = "aspect ratio above 64 not supported"; return ORBX_E_ARG; }
      G.hX = width / (float)G.nIni;
    }
    G.kpCap = std::max(G.N + 3, 4 * G.nIni) + 1;
    G.kpBase = kps;
    kps += G.kpCap;
    octCap = std::max(octCap, G.kpCap + 3);
    G.scale = h->mvScaleFactor[l];
    G.kpsize = (float)(int)((float)ORB_PATCH_SIZE * h->mvScaleFactor[l]);  // :862
    // blur tiles
    G.tilesX = (G.w + BLUR_TX - 1) / BLUR_TX;
    G.tilesY = (G.h + BLUR_TY - 1) / BLUR_TY;
    G.tileBase = tiles;
    tiles += G.tilesX * G.tilesY;
    // resize tables, SURVEY.md A.3 (cv::resize -> hal::resize: scale = 1./(dsize/ssize))
    G.xtabBase = (int)xtab.size();
    G.ytabBase = (int)ytab.size();
    if (l > 0) {
      const int sw = g[l - 1].w, sh = g[l - 1].h;
      const double inv_x = (double)G.w / sw, inv_y = (double)G.h / sh;
      const double scale_x = 1. / inv_x, scale_y = 1. / inv_y;
      for (int dx = 0; dx < G.w; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        int a0 = std::min(std::max(cv_round((1.f - fx) * 2048), -32768), 32767);
        int a1 = std::min(std::max(cv_round(fx * 2048), -32768), 32767);
        xtab.push_back(make_int2(sx, (a0 & 0xffff) | (a1 << 16)));
      }
      // k_resize reads the table two columns at a time with 16-byte loads and computes whole output quads: a level's entries start at
      // an even index (xtabBase, below) and are followed by copies of the last one up to a multiple of four columns
      while ((xtab.size() - (size_t)G.xtabBase) % 4) xtab.push_back(xtab.back());
      for (int dy = 0; dy < G.h; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floor(fy);
        fy -= sy;
        int b0 = std::min(std::max(cv_round((1.f - fy) * 2048), -32768), 32767);
        int b1 = std::min(std::max(cv_round(fy * 2048), -32768), 32767);
        ytab.push_back(make_int2(sy, (b0 & 0xffff) | (b1 << 16)));
      }
      // k_resize's tile height: 16 output rows while the LDS stage of a tile (its source rows + their horizontally interpolated rows)
      // stays below 64 KB - two workgroups per CU beside everything else -, else 8
      auto src_rows = [&](int rows) {
        int m = 0;
        for (int dy0 = 0; dy0 < G.h; dy0 += rows) {   // as k_resize derives a tile's source rows
          const int nrows = std::min(rows, G.h - dy0);
          const int f = std::min(std::max(ytab[G.ytabBase + dy0].x, 0), sh - 1), la = std::min(std::max(ytab[G.ytabBase + dy0 + nrows - 1].x + 1, 0), sh - 1);
          m = std::max(m, la - f + 1);
        }
        return m;
      };
      const size_t rowStage = (size_t)resize_row_bytes(sw) + (size_t)resize_t_pitch((G.w + 3) & ~3);
      G.resizeRows = RESIZE_ROWS_MAX;
      G.resizeSrcRows = src_rows(G.resizeRows);
      if ((size_t)G.resizeSrcRows * rowStage > RESIZE_STAGE_MAX || G.resizeSrcRows > RESIZE_MAXSRC) { G.resizeRows = 8; G.resizeSrcRows = src_rows(8); }
      // the level's form, and the record of every row tile (layout: orb_common.h), from the table entries above
      G.resizeTPitch = resize_form(G, g[l - 1]);
      G.resizeRecBase = (int)(resizerec.size() / RESIZE_REC_WORDS);
      for (int dy0 = 0; dy0 < G.h; dy0 += G.resizeRows) {
        const int nrows = std::min(G.resizeRows, G.h - dy0);
        const int2 *yt = &ytab[G.ytabBase + dy0];
        const int syFirst = std::min(std::max(yt[0].x, 0), sh - 1), syLast = std::min(std::max(yt[nrows - 1].x + 1, 0), sh - 1);
        resizerec.resize(resizerec.size() + RESIZE_REC_WORDS, 0u);
        uint32_t *Q = &resizerec[resizerec.size() - RESIZE_REC_WORDS];
        Q[0] = (uint32_t)syFirst;
        Q[1] = (uint32_t)std::min(syLast - syFirst + 1, G.resizeSrcRows);
        Q[2] = (uint32_t)nrows;
        Q[3] = (uint32_t)dy0;
        for (int r = 0; r < nrows; r++) {
          const int sy0 = std::min(std::max(yt[r].x, 0), sh - 1), sy1 = std::min(std::max(yt[r].x + 1, 0), sh - 1);
          uint32_t *R = Q + RESIZE_REC_GROUP_WORDS + 4 * r;
          R[0] = (uint32_t)((sy0 - syFirst) * G.resizeTPitch);
          R[1] = (uint32_t)((sy1 - syFirst) * G.resizeTPitch);
          R[2] = (uint32_t)yt[r].y;
          R[3] = (uint32_t)((dy0 + r) * G.pitch);
        }
      }
    } else { G.resizeRows = RESIZE_ROWS_MAX; G.resizeSrcRows = 0; }
  }
  if (slots > (1 << 30)) { h->err = "workspace too large"; return ORBX_E_ARG; }
  // FAST cells: window of every cell as the reference's double loop derives it, ORBextractor.cc:787-803 (the cell words of k_fast's
  // group records, below)
  std::vector<uint32_t> cellrec((size_t)std::max(cells, 1) * 4, 0u);
  for (int l = 0; l < nl; l++) {
    LevelGeom &G = g[l];
    G.rowTileMagic = magic_div((uint32_t)((G.h + G.resizeRows - 1) / G.resizeRows));
    for (int ci = 0; ci < G.nRows; ci++)
      for (int cj = 0; cj < G.nCols; cj++) {
        const int c = ci * G.nCols + cj;
        uint32_t *R = &cellrec[(size_t)(G.cellBase + c) * 4];
        const int iniX = ORB_MIN_BORDER + cj * G.wCell, iniY = ORB_MIN_BORDER + ci * G.hCell;
        const int maxX = std::min(iniX + G.wCell + 6, G.maxBorderX), maxY = std::min(iniY + G.hCell + 6, G.maxBorderY);
        const int tw = maxX - iniX, th = maxY - iniY;
        const bool valid = !(iniX >= G.maxBorderX - 6 || iniY >= G.maxBorderY - 3 || tw - 6 <= 0 || th - 6 <= 0);
        if (valid && (tw > FAST_TILE_COLS || th > FAST_TILE_ROWS)) { h->err = "FAST cell larger than the LDS tile"; return ORBX_E_ARG; }
        R[0] = (uint32_t)iniX | ((uint32_t)iniY << 16);
        R[1] = valid ? ((uint32_t)tw | ((uint32_t)th << 8) | (1u << 24)) : 0u;
        R[2] = (uint32_t)(G.slotBase + c * G.cellCap);
      }
  }
  // k_fast's workgroups: groups of up to 2 x 2 neighbouring cells of a level that fit one LDS tile (80-byte rows from the first cell's
  // column rounded down to 4, FAST_TILE_ROWS rows); levels with larger cells keep one cell per group in that direction
  std::vector<uint32_t> grouprec;
  for (int l = 0; l < nl; l++) {
    const LevelGeom &G = g[l];
    const int sx = (3 + 2 * G.wCell + 6 <= FAST_TILE_PITCH) ? 2 : 1, sy = (2 * G.hCell + 6 <= FAST_TILE_ROWS) ? 2 : 1;
    for (int ci = 0; ci < G.nRows; ci += sy)
      for (int cj = 0; cj < G.nCols; cj += sx) {
        const int gx = std::min(sx, G.nCols - cj), gy = std::min(sy, G.nRows - ci);
        const int first = G.cellBase + ci * G.nCols + cj;
        const uint32_t *F = &cellrec[(size_t)first * 4];
        const int tileX = (int)(F[0] & 0xffffu), tileY = (int)(F[0] >> 16);
        int maxX = 0, maxY = 0, nvalid = 0;
        for (int a = 0; a < gy; a++)
          for (int b = 0; b < gx; b++) {
            const uint32_t *R = &cellrec[(size_t)(first + a * G.nCols + b) * 4];
            if (!(R[1] >> 24)) continue;
            nvalid++;
            maxX = std::max(maxX, (int)(R[0] & 0xffffu) + (int)(R[1] & 0xffu));
            maxY = std::max(maxY, (int)(R[0] >> 16) + (int)((R[1] >> 8) & 0xffu));
          }
        const int gtw = nvalid ? maxX - tileX : 0, gth = nvalid ? maxY - tileY : 0;
        if (nvalid && ((tileX & 3) + gtw > FAST_TILE_PITCH || gth > FAST_TILE_ROWS)) { h->err = "FAST cell group larger than the LDS tile"; return ORBX_E_ARG; }
        // the record k_fast reads (layout: orb_common.h): the group, then cell w = wavefront w's, row-major inside the group
        grouprec.resize(grouprec.size() + FAST_REC_WORDS, 0u);
        uint32_t *Q = &grouprec[grouprec.size() - FAST_REC_WORDS];
        Q[0] = (uint32_t)tileX | ((uint32_t)tileY << 16);
        Q[1] = (uint32_t)gtw | ((uint32_t)gth << 8) | ((uint32_t)l << 16) | (nvalid ? 1u << 24 : 0u);
        Q[2] = (uint32_t)(gx * gy);
        Q[3] = (uint32_t)G.pitch;
        Q[4] = (uint32_t)(G.off & 0xffffffffu);
        Q[5] = (uint32_t)((uint64_t)G.off >> 32);
        Q[6] = (uint32_t)G.cellCap;
        for (int a = 0; a < gy; a++)
          for (int b = 0; b < gx; b++) {
            const int cell = first + a * G.nCols + b;
            const uint32_t *R = &cellrec[(size_t)cell * 4];
            uint32_t *C = Q + FAST_REC_GROUP_WORDS + FAST_REC_CELL_WORDS * (a * gx + b);
            C[0] = R[0];
            C[1] = R[1];
            C[2] = R[2];
            C[3] = (uint32_t)cell;
          }
      }
  }
  h->totalGroups = (int)(grouprec.size() / FAST_REC_WORDS);
  // blur tile records (k_blur)
  std::vector<uint32_t> tilerec((size_t)std::max(tiles, 1) * 8, 0u);
  for (int l = 0; l < nl; l++) {
    const LevelGeom &G = g[l];
    if (G.pitch > 65535 || G.bpitch > 65535) { h->err = "level pitch above 65535"; return ORBX_E_ARG; }
    if (l > 0 && ResizeCarve::of(0, 0, 0, (G.w + 3) & ~3).bytes > RESIZE_LDS_MAX) { h->err = "pyramid level wider than 20000 columns"; return ORBX_E_ARG; }   // k_resize's x table
    for (int ty = 0; ty < G.tilesY; ty++)
      for (int tx = 0; tx < G.tilesX; tx++) {
        uint32_t *R = &tilerec[(size_t)(G.tileBase + ty * G.tilesX + tx) * 8];
        const int x0 = tx * BLUR_TX, y0 = ty * BLUR_TY;
        const int wlim = l == 0 ? G.w : G.pitch;   // bytes of a row that k_blur may read (level 0: the caller's image)
        const bool interior = y0 - 3 >= 0 && y0 + BLUR_TY + 2 < G.h && x0 - 16 >= 0 && x0 + 160 <= wlim && x0 + 131 < G.w;
        bool whole = true;
        for (int x = x0; x < std::min(x0 + BLUR_TX, G.w); x += 16) whole = whole && x + 16 <= G.bpitch;
        R[0] = (uint32_t)x0 | ((uint32_t)y0 << 16);
        R[1] = (uint32_t)l | (interior ? BLUR_TILE_INTERIOR : 0u) | (whole ? BLUR_TILE_WHOLE_STORES : 0u);
        R[2] = (uint32_t)G.w | ((uint32_t)G.h << 16);
        R[3] = (uint32_t)G.pitch | ((uint32_t)G.bpitch << 16);
        R[4] = (uint32_t)(G.off & 0xffffffffu); R[5] = (uint32_t)((uint64_t)G.off >> 32);
        R[6] = (uint32_t)(G.boff & 0xffffffffu); R[7] = (uint32_t)((uint64_t)G.boff >> 32);
      }
  }
  h->geom = g;
  h->pyr_fs = std::max<size_t>(pyr, 256);
  h->blur_fs = blur;
  h->cell_fs = std::max(cells, 1);
  h->slot_fs = (size_t)std::max(slots, 1);
  h->cand_fs = std::max(slots, 1);
  h->lkp_fs = kps;
  h->totalTiles = tiles;
  h->totalCells = cells;
  h->totalKp = kps;
  h->octCap = octCap;
  h->maxKeypoints = kps;
  const size_t B = (size_t)max_batch;
  XCHECK(h, h->d_pyr.reserve(h->pyr_fs * B));
  XCHECK(h, h->d_blur.reserve(h->blur_fs * B));
  XCHECK(h, h->d_cellCnt.reserve(sizeof(uint32_t) * h->cell_fs * B));
  XCHECK(h, h->d_cellOff.reserve(sizeof(uint32_t) * h->cell_fs * B));
  XCHECK(h, h->d_slots.reserve(sizeof(uint32_t) * h->slot_fs * B));
  XCHECK(h, h->d_cand.reserve(sizeof(uint32_t) * (size_t)h->cand_fs * B));
  XCHECK(h, h->d_knode.reserve(sizeof(uint16_t) * (size_t)h->cand_fs * B));
  XCHECK(h, h->d_lkp.reserve(sizeof(uint32_t) * (size_t)h->lkp_fs * B));
  XCHECK(h, h->d_lrank.reserve(sizeof(uint16_t) * (size_t)h->lkp_fs * B));
  XCHECK(h, h->d_lcnt.reserve(sizeof(int32_t) * 2 * nl * B));
  XCHECK(h, h->d_candCnt.reserve(sizeof(int32_t) * nl * B));
  XCHECK(h, h->d_fastRecs.reserve(sizeof(uint32_t) * std::max<size_t>(grouprec.size(), FAST_REC_WORDS)));   // hipMalloc: aligned beyond a record's 128 bytes
  if (!grouprec.empty()) XCHECK(h, copy_on(h->stream, h->d_fastRecs.p, grouprec.data(), sizeof(uint32_t) * grouprec.size(), hipMemcpyHostToDevice));
  XCHECK(h, h->d_resizeRecs.reserve(sizeof(uint32_t) * std::max<size_t>(resizerec.size(), RESIZE_REC_WORDS)));
  if (!resizerec.empty()) XCHECK(h, copy_on(h->stream, h->d_resizeRecs.p, resizerec.data(), sizeof(uint32_t) * resizerec.size(), hipMemcpyHostToDevice));
  XCHECK(h, h->d_tiles.reserve(sizeof(uint32_t) * tilerec.size()));
  XCHECK(h, copy_on(h->stream, h->d_tiles.p, tilerec.data(), sizeof(uint32_t) * tilerec.size(), hipMemcpyHostToDevice));
  XCHECK(h, h->d_xtab.reserve(sizeof(int2) * std::max<size_t>(xtab.size(), 1)));
  XCHECK(h, h->d_ytab.reserve(sizeof(int2) * std::max<size_t>(ytab.size(), 1)));
  if (!xtab.empty()) XCHECK(h, copy_on(h->stream, h->d_xtab.p, xtab.data(), sizeof(int2) * xtab.size(), hipMemcpyHostToDevice));
  if (!ytab.empty()) XCHECK(h, copy_on(h->stream, h->d_ytab.p, ytab.data(), sizeof(int2) * ytab.size(), hipMemcpyHostToDevice));
  // k_pyramid_chain's tile records: for every 32x32 tile of a level L >= 1 the rectangles of levels L-1 .. 0 it depends on,
  // walked down through the resize tables exactly as k_resize indexes them (x: sx, min(sx+1, w-1); y: clamp(sy), clamp(sy+1))
  {
    std::vector<ChainTile> tilesC;
    size_t b0 = 0, b1 = 0, tabMax = 0;
    for (int L = nl - 1; L >= 1; L--)   // highest level first: its workgroups have the longest chains and must not start last
      for (int ty = 0; ty < g[L].h; ty += CHAIN_TILE)
        for (int tx = 0; tx < g[L].w; tx += CHAIN_TILE) {
          ChainTile T;
          memset(&T, 0, sizeof(T));
          T.level = (uint16_t)L;
          int x0 = tx, x1 = std::min(tx + CHAIN_TILE, g[L].w) - 1, y0 = ty, y1 = std::min(ty + CHAIN_TILE, g[L].h) - 1;   // inclusive
          size_t tab = 0;
          for (int l = L; l >= 0; l--) {
            T.x[l] = (uint16_t)x0; T.y[l] = (uint16_t)y0; T.w[l] = (uint16_t)(x1 - x0 + 1); T.h[l] = (uint16_t)(y1 - y0 + 1);
            const size_t area = (size_t)T.w[l] * T.h[l];
            if (l < L) { if (l & 1) b1 = std::max(b1, area); else b0 = std::max(b0, area); }
            if (l == 0) break;
            tab += (size_t)T.w[l] + T.h[l];
            const int sw = g[l - 1].w, sh = g[l - 1].h;
            const int2 *xt = &xtab[g[l].xtabBase], *yt = &ytab[g[l].ytabBase];
            int nx0 = sw, nx1 = 0, ny0 = sh, ny1 = 0;
            for (int x = x0; x <= x1; x++) { nx0 = std::min(nx0, xt[x].x); nx1 = std::max(nx1, std::min(xt[x].x + 1, sw - 1)); }
            for (int y = y0; y <= y1; y++) {
              ny0 = std::min(ny0, std::min(std::max(yt[y].x, 0), sh - 1));
              ny1 = std::max(ny1, std::min(std::max(yt[y].x + 1, 0), sh - 1));
            }
            x0 = nx0; x1 = nx1; y0 = ny0; y1 = ny1;
          }
          tabMax = std::max(tabMax, tab);
          tilesC.push_back(T);
        }
    b0 = align_up(b0, 16); b1 = align_up(b1, 16);
    const size_t lds = ChainCarve::of((int)b0, (int)b1, (int)tabMax).bytes;
    // stage sizes stay below 2^14 pixels (the kernel's index split) and the whole state inside 64 KiB; otherwise (scale factors far
    // from 1.2) single-frame calls keep the level-by-level form
    h->chainTiles = 0;
    if (!tilesC.empty() && lds <= CHAIN_LDS_MAX && b1 <= 16384 && b0 <= 65536 && tilesC.size() < 65536) {
      bool ok = true;
      for (const ChainTile &T : tilesC)
        for (int l = 1; l <= T.level; l++) ok = ok && (size_t)T.w[l] * T.h[l] < 16384;
      if (ok) {
        XCHECK(h, h->d_chain.reserve(sizeof(ChainTile) * tilesC.size()));
        XCHECK(h, copy_on(h->stream, h->d_chain.p, tilesC.data(), sizeof(ChainTile) * tilesC.size(), hipMemcpyHostToDevice));
        h->chainTiles = (int)tilesC.size(); h->chainBuf0 = (int)b0; h->chainBuf1 = (int)b1; h->chainLds = lds;
      }
    }
  }
  // k_octree LDS (OctreeCarve): node arrays (OCT_HEAD_PER_NODE + OCT_BODY_PER_NODE bytes per node) + scan scratch, plus the level's cell offsets when they fit
  int maxCells = 1;
  for (int l = 0; l < nl; l++) maxCells = std::max(maxCells, g[l].nCols * g[l].nRows);
  // (what the check below refuses anyway, taken out before the carve's int arithmetic sees it)
  if (octCap > OCT_LDS_MAX / (OCT_HEAD_PER_NODE + OCT_BODY_PER_NODE)) { h->err = "nfeatures too large for the LDS-resident octree"; return ORBX_E_ARG; }
  // k_octree's code form: per level one byte per column and per row of the detection rectangle - the root and
  // the OCT_D x bits, the OCT_D y bits of the key's path through DivideNode's splits (ORBextractor.cc:479-535), walked with the
  // kernel's own interval arithmetic.  A split line is ul + ((ur - ul + 1) >> 1) and a key goes right / down when it is not below
  // it; an interval of width 1 splits into widths 1 and 0, one of width 0 keeps itself as its right child: the walk just goes on,
  // the bits are what the comparisons give.  The leaf bins, the count pyramid and the leaf map live in the LDS of chcnt / chpos
  // (OCT_HEAD_PER_NODE * octCap bytes): where they fit there - the bench's configurations - octLds is what it is without them; a configuration
  // with fewer nodes gets that head region enlarged as long as the whole stays small (32 KiB), any other keeps the per-key rounds.
  {
    int maxIni = 0;
    for (int l = 0; l < nl; l++) maxIni = std::max(maxIni, g[l].nIni);   // (a level with more than 65535 keys: the kernel's own check)
    size_t limit = ORB_LDS_LIMIT;
    if (const char *e = getenv("ORBHIP_OCTREE_TABLE_LIMIT")) limit = (size_t)strtoul(e, nullptr, 10);   // tests: a bound the tables do not fit
    const size_t tabBytes = align_up(OCT_TABLE_BYTES(std::max(maxIni, 1)), 16);
    h->octCodes = maxIni >= 1 && (maxIni << OCT_D) <= 256 && octCap <= 65535 && tabBytes <= limit;
    h->octHead = OCT_HEAD_PER_NODE * (size_t)octCap;
    if (h->octCodes && tabBytes > h->octHead) {
      if (OctreeCarve::of(octCap, (int)tabBytes, 1024, maxCells).bytes <= OCT_GROWN_HEAD_MAX) h->octHead = tabBytes;
      else h->octCodes = false;
    }
    if (h->octCodes) {
      std::vector<uint8_t> tab;
      auto walk = [](int v, int ul, int ur) {
        int bits = 0;
        for (int d = 0; d < OCT_D; d++) {
          const int half = (ur - ul + 1) >> 1;   // ceil(/2), :481-482
          const int b = v < ul + half ? 0 : 1;
          if (b) ul = ul + half; else ur = ul + half;
          bits = (bits << 1) | b;
        }
        return bits;
      };
      for (int l = 0; l < nl; l++) {
        LevelGeom &G = g[l];
        G.octTabX = G.octTabY = (int)tab.size();
        if (G.nIni < 1) continue;
        const int Wrect = G.maxBorderX - ORB_MIN_BORDER, Hrect = G.maxBorderY - ORB_MIN_BORDER;
        for (int x = 0; x <= Wrect; x++) {   // one entry more than the rectangle has columns: the kernel clamps to it
          const int r = std::min(std::max((int)((float)x / G.hX), 0), G.nIni - 1);   // vpIniNodes[kp.pt.x/hX], :567
          tab.push_back((uint8_t)((r << OCT_D) | walk(x, (int)(G.hX * (float)r), (int)(G.hX * (float)(r + 1)))));
        }
        G.octTabY = (int)tab.size();
        for (int y = 0; y <= Hrect; y++) tab.push_back((uint8_t)walk(y, 0, Hrect));
      }
      h->geom = g;
      XCHECK(h, h->d_octTab.reserve(std::max<size_t>(tab.size(), 1)));
      if (!tab.empty()) XCHECK(h, copy_on(h->stream, h->d_octTab.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    }
  }
  if (OctreeCarve::of(octCap, (int)h->octHead, 1024, 0).bytes > OCT_LDS_MAX) { h->err = "nfeatures too large for the LDS-resident octree"; return ORBX_E_ARG; }
  h->octCellsLds = OctreeCarve::of(octCap, (int)h->octHead, 1024, maxCells).bytes <= OCT_CELLS_LDS_MAX;
  const size_t lds = h->octLds = OctreeCarve::of(octCap, (int)h->octHead, 1024, h->octCellsLds ? maxCells : 0).bytes;
  if (lds > ORB_LDS_LIMIT) { h->err = "octree LDS state exceeds 160 KiB"; return ORBX_E_ARG; }   // limit raised once in orbx_create
  h->rows = rows;
  h->cols = cols;
  h->max_batch = max_batch;
  h->have_last = false;
  return h->maxKeypoints;
}

void orbx_set_profiling(orbx_t *h, int enable) {
  if (!h) return;
  h->profiling = enable != 0;
  h->prof_head = 0;
  h->stage_valid = false;
  if (h->profiling && !h->ev_ok) {
    (void)hipSetDevice(h->device);
    bool ok = true;
    for (auto &set : h->ev)
      for (auto &e : set) ok = ok && hipEventCreate(&e) == hipSuccess;
    h->ev_ok = ok;
  }
}

// Average per stage over the batches launched since profiling was switched on (the PROF_DEPTH most recent ones).
int orbx_get_stage_ms(orbx_t *h, float *ms, int cap) {
  if (!h || !ms || !h->profiling || !h->ev_ok || !h->stage_valid || h->prof_head <= 0) return 0;
  const int nb = std::min(h->prof_head, PROF_DEPTH), n = std::min(cap, 5);
  if (hipEventSynchronize(h->ev[(h->prof_head - 1) % PROF_DEPTH][5]) != hipSuccess) return 0;
  for (int i = 0; i < n; i++) ms[i] = 0.f;
  for (int b = 0; b < nb; b++) {
    const int slot = (h->prof_head - 1 - b) % PROF_DEPTH;
    for (int i = 0; i < n; i++) {
      float t = 0;
      if (hipEventElapsedTime(&t, h->ev[slot][i], h->ev[slot][i + 1]) != hipSuccess) return 0;
      ms[i] += t / (float)nb;
    }
  }
  return n;
}

int orbx_extract_batch_device(orbx_t *h, const uint8_t *d_images, int rows, int cols, size_t stride, size_t frame_stride,
                              int nframes, int lap0, int lap1, orbx_keypoint_t *d_kps, uint8_t *d_desc, int32_t *d_counts,
                              int cap, void *stream_) {
  if (!h) return ORBX_E_ARG;
  if (!d_images || rows <= 0 || cols <= 0 || nframes <= 0) return ORBX_E_EMPTY;
  if (!d_kps || !d_desc || !d_counts || cap <= 0 || stride < (size_t)cols) return ORBX_E_ARG;
  int rc = orbx_configure(h, rows, cols, std::max(nframes, h->rows == rows && h->cols == cols ? h->max_batch : 1));
  if (rc < 0) return rc;
  // asynchronous: an overflow could not be reported, and d_counts feeds the matcher as a live count bounded by its frame stride,
  // so a capacity below the octree's worst case is refused up front
  if (cap < h->maxKeypoints) { h->err = "cap below orbx_configure()'s bound"; return ORBX_E_CAP; }
  XCHECK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream_;  // verbatim: NULL is the device's default stream
  FrameParams P;
  memset(&P, 0, sizeof(P));
  for (int l = 0; l < h->nlevels; l++) P.geom[l] = h->geom[l];
  P.nlevels = h->nlevels;
  P.nframes = nframes;
  P.iniTh = h->iniThFAST;
  P.minTh = h->minThFAST;
  P.lap0 = lap0;
  P.lap1 = lap1;
  P.img0 = d_images;
  P.img0_stride = stride;
  P.img0_frame_stride = frame_stride;
  P.pyr = (uint8_t *)h->d_pyr.p;       P.pyr_fs = h->pyr_fs;
  P.blur = (uint8_t *)h->d_blur.p;     P.blur_fs = h->blur_fs;
  P.cellCnt = (uint32_t *)h->d_cellCnt.p; P.cell_fs = h->cell_fs;
  P.slots = (uint32_t *)h->d_slots.p;  P.slot_fs = h->slot_fs;
  P.cand = (uint32_t *)h->d_cand.p;    P.cand_fs = h->cand_fs;
  P.knode = (uint16_t *)h->d_knode.p;
  P.lkp = (uint32_t *)h->d_lkp.p;      P.lkp_fs = h->lkp_fs;
  P.lrank = (uint16_t *)h->d_lrank.p;
  P.lcnt = (int32_t *)h->d_lcnt.p;
  P.candCnt = (int32_t *)h->d_candCnt.p;
  P.xtab = (const int2 *)h->d_xtab.p;
  P.ytab = (const int2 *)h->d_ytab.p;
  P.disc = (const int8_t *)h->d_disc.p;
  P.totalTiles = h->totalTiles;
  P.totalCells = h->totalCells;
  P.fastRecs = (const uint32_t *)h->d_fastRecs.p;
  P.resizeRecs = (const uint32_t *)h->d_resizeRecs.p;
  P.totalGroups = h->totalGroups;
  P.magicGroups = magic_div((uint32_t)std::max(h->totalGroups, 1));
  P.tiles = (const uint32_t *)h->d_tiles.p;
  P.magicCells = magic_div((uint32_t)std::max(h->totalCells, 1));
  P.magicTiles = magic_div((uint32_t)std::max(h->totalTiles, 1));
  // One workgroup per (frame, level) in k_octree and one launch per level of the pyramid: a batch fills the chip that way; a single frame
  // is all launch gaps and one long workgroup, so few-frame calls ("wide") take the one-launch pyramid, the 1024-thread octree and
  // k_describe with one keypoint per wavefront (blocks of 8 in sequence would leave a 1000-keypoint frame ~130 wavefronts).
  const bool wide = (long long)h->nlevels * nframes <= 32;
  const int describeGroups = wide ? ORB_DESCRIBE_GROUPS(h->totalKp, 1) : ORB_DESCRIBE_GROUPS(h->totalKp, ORB_DESCRIBE_K);
  P.magicKpBlk = magic_div((uint32_t)describeGroups);
  P.totalKp = h->totalKp;
  P.octCap = h->octCap;
  P.octHead = (int)h->octHead;
  P.octTab = h->octCodes ? (const uint8_t *)h->d_octTab.p : nullptr;
  P.chain = (const ChainTile *)h->d_chain.p; P.chainBuf0 = h->chainBuf0; P.chainBuf1 = h->chainBuf1;
  P.out_kps = d_kps;
  P.out_desc = d_desc;
  P.out_counts = d_counts;
  P.cap = cap;
  const bool prof = h->profiling && h->ev_ok;
  hipEvent_t *pev = h->ev[h->prof_head % PROF_DEPTH];
  if (prof) XCHECK(h, hipEventRecord(pev[0], s));
  // ORBHIP_PRINT_EXTRACT_FORMS (tests/test_gpu_batch_layouts.py): one stderr line per call with the host's choices below
  const bool printForms = getenv("ORBHIP_PRINT_EXTRACT_FORMS") != nullptr;
  std::string pyrForm = h->nlevels == 1 ? "none" : "";
  if (wide && h->chainTiles > 0) { hipLaunchKernelGGL(k_pyramid_chain, dim3(h->chainTiles * nframes), dim3(CHAIN_NT), h->chainLds, s, P); pyrForm = "chain"; }
  else
  for (int l = 1; l < h->nlevels; l++) {
    const LevelGeom &G = h->geom[l], &Gs = h->geom[l - 1];
    const int rowBytes = resize_row_bytes(Gs.w);
    const int tPitch = G.resizeTPitch;   // orbx_configure chose the form and built the row-tile records with it
    const bool twoPass = tPitch > 0;
    hipLaunchKernelGGL(k_resize, dim3(((G.h + G.resizeRows - 1) / G.resizeRows) * nframes), dim3(256), ResizeCarve::of(G.resizeSrcRows, rowBytes, tPitch, (G.w + 3) & ~3).bytes, s, P,
                       l, rowBytes, tPitch, G.resizeSrcRows);
    if (printForms) pyrForm += std::string(l > 1 ? "," : "") + (!twoPass ? "1p" : G.resizeRows == 16 ? "2p16" : "2p8");
  }
  if (prof) XCHECK(h, hipEventRecord(pev[1], s));
  if (h->totalGroups > 0) hipLaunchKernelGGL(k_fast, dim3(h->totalGroups * nframes), dim3(FAST_NT), 0, s, P);
  if (prof) XCHECK(h, hipEventRecord(pev[2], s));
  // (k_octree: one workgroup per (frame, level); a single frame has only nlevels of them and the longest, level 0, is the critical
  // path of the whole call, so few-frame launches use 1024 threads per workgroup)
  if (wide) {
    if (h->octCellsLds) hipLaunchKernelGGL((k_octree<1024, true>), dim3(h->nlevels * nframes), dim3(1024), h->octLds, s, P, (uint32_t *)h->d_cellOff.p);
    else hipLaunchKernelGGL((k_octree<1024, false>), dim3(h->nlevels * nframes), dim3(1024), h->octLds, s, P, (uint32_t *)h->d_cellOff.p);
  } else {
    if (h->octCellsLds) hipLaunchKernelGGL((k_octree<256, true>), dim3(h->nlevels * nframes), dim3(256), h->octLds, s, P, (uint32_t *)h->d_cellOff.p);
    else hipLaunchKernelGGL((k_octree<256, false>), dim3(h->nlevels * nframes), dim3(256), h->octLds, s, P, (uint32_t *)h->d_cellOff.p);
  }
  if (prof) XCHECK(h, hipEventRecord(pev[3], s));
  hipLaunchKernelGGL(k_blur, dim3(h->totalTiles * nframes), dim3(256), 0, s, P);
  if (prof) XCHECK(h, hipEventRecord(pev[4], s));
  // also writes the frame totals (>= 1 workgroup per frame: nfeatures == 0)
  if (wide) hipLaunchKernelGGL(k_describe<1>, dim3(describeGroups * nframes), dim3(256), 0, s, P);
  else hipLaunchKernelGGL(k_describe<ORB_DESCRIBE_K>, dim3(describeGroups * nframes), dim3(256), 0, s, P);
  if (prof) { XCHECK(h, hipEventRecord(pev[5], s)); h->prof_head++; h->stage_valid = true; }
  XCHECK(h, hipGetLastError());
  if (printForms) {
    // level 0 is the caller's plane: k_fast, k_resize, k_blur and k_describe take their dword / LDS-DMA paths on it only when its base
    // and stride are multiples of 4, k_blur's DMA tile load also needs a width that is a multiple of 16 and a level of 160 x 40 or more
    int aligned0 = 0;
    for (int f = 0; f < nframes; f++) aligned0 += (((uintptr_t)(d_images + (size_t)f * frame_stride) | (uintptr_t)stride) & 3u) == 0;
    const LevelGeom &G0 = h->geom[0];
    const int blur0dma = G0.w >= 160 && G0.h >= 40 && (G0.w & 15) == 0 ? aligned0 : 0;
    fprintf(stderr, "orbhip: extract nframes %d pyramid %s octree %d/%s aligned0 %d blur0dma %d describe %d rounds %s octLds %zu octCap %d\n", nframes, pyrForm.c_str(), wide ? 1024 : 256,
            h->octCellsLds ? "lds" : "global", aligned0, blur0dma, wide ? 1 : ORB_DESCRIBE_K, h->octCodes ? "codes" : "keys", h->octLds, h->octCap);
  }
  h->last = P;
  h->have_last = true;
  // consumers of this batch on OTHER streams (orbx_compute_stereo_matches, orbx_download_*) order themselves behind it
  if (!h->in_capture) {
    if (!h->last_done) XCHECK(h, hipEventCreateWithFlags(&h->last_done, hipEventDisableTiming));
    XCHECK(h, hipEventRecord(h->last_done, s));
    h->last_pending = true;
  }
  return 0;
}

int orbx_extract(orbx_t *h, const uint8_t *image, int rows, int cols, size_t stride, int lap0, int lap1,
                 orbx_keypoint_t *keypoints, uint8_t *descriptors, int cap, int *n_out) {
  if (!h) return ORBX_E_ARG;
  if (n_out) *n_out = 0;
  if (!image || rows <= 0 || cols <= 0) return ORBX_E_EMPTY;  // ORBextractor.cc:1075-1076
  if (stride < (size_t)cols || !n_out) return ORBX_E_ARG;
  int rc = orbx_configure(h, rows, cols, h->rows == rows && h->cols == cols ? h->max_batch : 1);
  if (rc < 0) return rc;
  const int icap = h->maxKeypoints;
  const size_t dstride = align_up((size_t)cols, 64);
  XCHECK(h, hipSetDevice(h->device));
  XCHECK(h, h->d_img.reserve(dstride * rows));
  // pinned staging: one H2D, all kernels, one D2H (counts, keypoints and descriptors are one device block) and ONE synchronisation
  // per frame
  const size_t in_bytes = dstride * rows, kp_bytes = sizeof(orbx_keypoint_t) * (size_t)icap, de_bytes = 32 * (size_t)icap;
  const size_t kp_off = 64, de_off = kp_off + align_up(kp_bytes, 64), out_bytes = de_off + de_bytes;   // [counts][keypoints][descriptors], 64-byte aligned parts
  XCHECK(h, h->d_okps.reserve(out_bytes));
  if (h->pin_in_bytes < in_bytes) {
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    h->pin_in = nullptr; h->pin_in_bytes = 0;
    XCHECK(h, hipHostMalloc(&h->pin_in, in_bytes, hipHostMallocDefault));
    h->pin_in_bytes = in_bytes;
  }
  if (h->pin_out_bytes < out_bytes) {
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    h->pin_out = nullptr; h->pin_out_bytes = 0;
    XCHECK(h, hipHostMalloc(&h->pin_out, out_bytes, hipHostMallocDefault));
    h->pin_out_bytes = out_bytes;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (int y = 0; y < rows; y++) memcpy((uint8_t *)h->pin_in + (size_t)y * dstride, image + (size_t)y * stride, (size_t)cols);
  const auto t1 = std::chrono::steady_clock::now();
  uint8_t *po = (uint8_t *)h->pin_out;
  auto enqueue = [&]() -> int {  // the whole per-frame sequence on h->stream
    XCHECK(h, hipMemcpyAsync(h->d_img.p, h->pin_in, in_bytes, hipMemcpyHostToDevice, h->stream));
    uint8_t *dout = (uint8_t *)h->d_okps.p;
    const int r = orbx_extract_batch_device(h, (const uint8_t *)h->d_img.p, rows, cols, dstride, dstride * rows, 1, lap0, lap1,
                                            (orbx_keypoint_t *)(dout + kp_off), dout + de_off, (int32_t *)dout, icap, h->stream);
    if (r < 0) return r;
    XCHECK(h, hipMemcpyAsync(po, dout, out_bytes, hipMemcpyDeviceToHost, h->stream));
    return 0;
  };
  bool launched = false;
  if (h->graph_ok && !h->profiling) {
    auto &K = h->graph_key;
    const bool same = h->graph && K.rows == rows && K.cols == cols && K.lap0 == lap0 && K.lap1 == lap1 && K.icap == icap && K.pin_in == h->pin_in &&
                      K.pin_out == h->pin_out && K.d_img == h->d_img.p && K.d_okps == h->d_okps.p && K.d_pyr == h->d_pyr.p;
    if (!same) {
      if (h->graph) { (void)hipGraphExecDestroy(h->graph); h->graph = nullptr; }
      hipGraph_t g = nullptr;
      if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        h->in_capture = true;
        const int r = enqueue();
        h->in_capture = false;
        const hipError_t e = hipStreamEndCapture(h->stream, &g);
        if (r == 0 && e == hipSuccess && g && hipGraphInstantiate(&h->graph, g, nullptr, nullptr, 0) == hipSuccess) {
          K.rows = rows; K.cols = cols; K.lap0 = lap0; K.lap1 = lap1; K.icap = icap; K.pin_in = h->pin_in; K.pin_out = h->pin_out;
          K.d_img = h->d_img.p; K.d_okps = h->d_okps.p; K.d_pyr = h->d_pyr.p;
        } else {
          h->graph = nullptr;
          h->graph_ok = false;
          (void)hipGetLastError();
        }
        if (g) (void)hipGraphDestroy(g);
      } else {
        h->graph_ok = false;
        (void)hipGetLastError();
      }
    }
    if (h->graph) {
      XCHECK(h, hipGraphLaunch(h->graph, h->stream));
      launched = true;
    }
  }
  if (!launched) { rc = enqueue(); if (rc < 0) return rc; }
  const auto t2 = std::chrono::steady_clock::now();
  XCHECK(h, hipStreamSynchronize(h->stream));
  const auto t3 = std::chrono::steady_clock::now();
  h->last_pending = false;   // this entry point returns with the frame's work complete
  int32_t counts[2];
  memcpy(counts, po, sizeof(counts));
  *n_out = counts[0];
  if (counts[0] > cap) return ORBX_E_CAP;
  if (counts[0] > 0) {
    if (!keypoints || !descriptors) return ORBX_E_ARG;
    memcpy(keypoints, po + kp_off, sizeof(orbx_keypoint_t) * (size_t)counts[0]);
    memcpy(descriptors, po + de_off, 32 * (size_t)counts[0]);
  }
  const auto t4 = std::chrono::steady_clock::now();
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<float, std::micro>(b - a).count(); };
  h->host_us[0] = us(t0, t1); h->host_us[1] = us(t1, t2); h->host_us[2] = us(t2, t3); h->host_us[3] = us(t3, t4);
  return counts[1];
}

// Host-side split of the last orbx_extract call, microseconds: copy of the image into pinned staging, submission of the frame's
// sequence (graph launch), wait for its completion, copy of the results to the caller's arrays.
int orbx_get_host_us(const orbx_t *h, float *us, int cap) {
  if (!h || !us || cap < 4) return ORBX_E_ARG;
  for (int i = 0; i < 4; i++) us[i] = h->host_us[i];
  return 4;
}

int orbx_cvt_color_gray_device(const uint8_t *d_src, int rows, int cols, size_t src_stride, int channels, int rgb_order, uint8_t *d_dst,
                               size_t dst_stride, void *stream) {
  if (!d_src || !d_dst || rows <= 0 || cols <= 0 || (channels != 3 && channels != 4) || src_stride < (size_t)cols * channels || dst_stride < (size_t)cols)
    return ORBX_E_ARG;
  hipLaunchKernelGGL(k_cvt_gray, dim3((cols + 1023) / 1024, rows), dim3(256), 0, (hipStream_t)stream, d_src, rows, cols, src_stride, channels,
                     rgb_order ? 1 : 0, d_dst, dst_stride);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbx_cvt_color_gray(orbx_t *h, const uint8_t *src, int rows, int cols, size_t src_stride, int channels, int rgb_order, uint8_t *dst,
                        size_t dst_stride) {
  if (!h || !src || !dst || rows <= 0 || cols <= 0 || (channels != 3 && channels != 4) || src_stride < (size_t)cols * channels || dst_stride < (size_t)cols)
    return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  const size_t sbytes = (size_t)cols * channels, dpitch = align_up((size_t)cols, 64);
  XCHECK(h, h->stereo[0].reserve(sbytes * rows));
  XCHECK(h, h->stereo[1].reserve(dpitch * rows));
  XCHECK(h, hipMemcpy2DAsync(h->stereo[0].p, sbytes, src, src_stride, sbytes, (size_t)rows, hipMemcpyHostToDevice, h->stream));
  const int rc = orbx_cvt_color_gray_device((const uint8_t *)h->stereo[0].p, rows, cols, sbytes, channels, rgb_order, (uint8_t *)h->stereo[1].p, dpitch, h->stream);
  if (rc < 0) return rc;
  XCHECK(h, hipMemcpy2DAsync(dst, dst_stride, h->stereo[1].p, dpitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, h->stream));
  XCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int orbx_clahe_device(const uint8_t *d_src, int rows, int cols, size_t src_stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *d_lut,
                      uint8_t *d_dst, size_t dst_stride, void *stream) {
  if (!d_src || !d_dst || !d_lut || rows <= 0 || cols <= 0 || tiles_x <= 0 || tiles_y <= 0 || tiles_x * tiles_y > 256 || cols < tiles_x || rows < tiles_y ||
      src_stride < (size_t)cols || dst_stride < (size_t)cols || !(clip_limit >= 0.0))
    return ORBX_E_ARG;
  // CLAHE_Impl::apply: tile size of the (possibly extended) image, lutScale and the integer clip limit
  const int ecols = cols % tiles_x == 0 ? cols : cols + tiles_x - cols % tiles_x, erows = rows % tiles_y == 0 ? rows : rows + tiles_y - rows % tiles_y;
  const int tw = ecols / tiles_x, th = erows / tiles_y, tileSizeTotal = tw * th;
  const float lutScale = (float)255 / (float)tileSizeTotal;
  int clipLimit = 0;
  if (clip_limit > 0.0) {
    clipLimit = (int)(clip_limit * tileSizeTotal / 256);
    if (clipLimit < 1) clipLimit = 1;
  }
  hipLaunchKernelGGL(k_clahe_lut, dim3(tiles_x * tiles_y), dim3(256), 0, (hipStream_t)stream, d_src, rows, cols, src_stride, tiles_x, tw, th, clipLimit,
                     lutScale, d_lut);
  const int rowsPerBlock = 4;
  hipLaunchKernelGGL(k_clahe_interp, dim3((rows + rowsPerBlock - 1) / rowsPerBlock), dim3(256), ClaheCarve::of(tiles_y, tiles_x).bytes, (hipStream_t)stream, d_src,
                     rows, cols, src_stride, tiles_x, tiles_y, 1.0f / (float)tw, 1.0f / (float)th, (const uint8_t *)d_lut, d_dst, dst_stride, rowsPerBlock);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbx_clahe(orbx_t *h, const uint8_t *src, int rows, int cols, size_t src_stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *dst,
               size_t dst_stride) {
  if (!h || !src || !dst || rows <= 0 || cols <= 0 || src_stride < (size_t)cols || dst_stride < (size_t)cols) return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  const size_t pitch = align_up((size_t)cols, 64);
  XCHECK(h, h->stereo[0].reserve(pitch * rows));
  XCHECK(h, h->stereo[1].reserve(pitch * rows));
  XCHECK(h, h->stereo[2].reserve(256 * 256));
  XCHECK(h, hipMemcpy2DAsync(h->stereo[0].p, pitch, src, src_stride, (size_t)cols, (size_t)rows, hipMemcpyHostToDevice, h->stream));
  const int rc = orbx_clahe_device((const uint8_t *)h->stereo[0].p, rows, cols, pitch, clip_limit, tiles_x, tiles_y, (uint8_t *)h->stereo[2].p,
                                   (uint8_t *)h->stereo[1].p, pitch, h->stream);
  if (rc < 0) return rc;
  XCHECK(h, hipMemcpy2DAsync(dst, dst_stride, h->stereo[1].p, pitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, h->stream));
  XCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int orbx_remap_linear_device(const uint8_t *d_src, int src_rows, int src_cols, size_t src_stride, const float *d_mapx, const float *d_mapy,
                             size_t map_stride_elems, int rows, int cols, uint8_t *d_dst, size_t dst_stride, void *stream) {
  if (!d_src || !d_mapx || !d_mapy || !d_dst || src_rows <= 0 || src_cols <= 0 || rows <= 0 || cols <= 0 || src_stride < (size_t)src_cols ||
      map_stride_elems < (size_t)cols || dst_stride < (size_t)cols || src_cols > 32767 || src_rows > 32767)
    return ORBX_E_ARG;
  hipLaunchKernelGGL(k_remap_linear, dim3((cols + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream, d_src, src_rows, src_cols, src_stride, d_mapx,
                     d_mapy, map_stride_elems, rows, cols, d_dst, dst_stride);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbx_remap_linear(orbx_t *h, const uint8_t *src, int src_rows, int src_cols, size_t src_stride, const float *mapx, const float *mapy, int rows,
                      int cols, uint8_t *dst, size_t dst_stride) {
  if (!h || !src || !dst || src_rows <= 0 || src_cols <= 0 || rows <= 0 || cols <= 0 || src_stride < (size_t)src_cols || dst_stride < (size_t)cols ||
      ((mapx == nullptr) != (mapy == nullptr)))
    return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  if (mapx) {   // the maps are fixed per camera (computed once, stereo_euroc.cc:113-114): uploaded when given, kept for later calls
    XCHECK(h, h->maps[0].reserve(sizeof(float) * (size_t)rows * cols));
    XCHECK(h, h->maps[1].reserve(sizeof(float) * (size_t)rows * cols));
    XCHECK(h, hipMemcpyAsync(h->maps[0].p, mapx, sizeof(float) * (size_t)rows * cols, hipMemcpyHostToDevice, h->stream));
    XCHECK(h, hipMemcpyAsync(h->maps[1].p, mapy, sizeof(float) * (size_t)rows * cols, hipMemcpyHostToDevice, h->stream));
    h->maps_rows = rows;
    h->maps_cols = cols;
  } else if (h->maps_rows != rows || h->maps_cols != cols) {
    h->err = "orbx_remap_linear: no maps of this size uploaded yet";
    return ORBX_E_ARG;
  }
  const size_t spitch = align_up((size_t)src_cols, 64), dpitch = align_up((size_t)cols, 64);
  XCHECK(h, h->stereo[0].reserve(spitch * src_rows));
  XCHECK(h, h->stereo[1].reserve(dpitch * rows));
  XCHECK(h, hipMemcpy2DAsync(h->stereo[0].p, spitch, src, src_stride, (size_t)src_cols, (size_t)src_rows, hipMemcpyHostToDevice, h->stream));
  const int rc = orbx_remap_linear_device((const uint8_t *)h->stereo[0].p, src_rows, src_cols, spitch, (const float *)h->maps[0].p,
                                          (const float *)h->maps[1].p, (size_t)cols, rows, cols, (uint8_t *)h->stereo[1].p, dpitch, h->stream);
  if (rc < 0) return rc;
  XCHECK(h, hipMemcpy2DAsync(dst, dst_stride, h->stereo[1].p, dpitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, h->stream));
  XCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// Tile size of the (possibly extended) image, lutScale and the integer clip limit of CLAHE_Impl::apply, as orbx_clahe_device has them.
static void clahe_batch_geometry(ClaheBatch &P, double clip_limit) {
  const int ecols = P.cols % P.tilesX == 0 ? P.cols : P.cols + P.tilesX - P.cols % P.tilesX;
  const int erows = P.rows % P.tilesY == 0 ? P.rows : P.rows + P.tilesY - P.rows % P.tilesY;
  P.tw = ecols / P.tilesX;
  P.th = erows / P.tilesY;
  const int tileSizeTotal = P.tw * P.th;
  P.lutScale = (float)255 / (float)tileSizeTotal;
  P.clipLimit = 0;
  if (clip_limit > 0.0) {
    P.clipLimit = (int)(clip_limit * tileSizeTotal / 256);
    if (P.clipLimit < 1) P.clipLimit = 1;
  }
  P.inv_tw = 1.0f / (float)P.tw;
  P.inv_th = 1.0f / (float)P.th;
}

// Bytes from the first byte of frame 0 to one past the last byte of the last frame.
static size_t batch_extent(int nframes, int rows, int cols, size_t stride, size_t frame_stride) {
  return (size_t)(nframes - 1) * frame_stride + (size_t)(rows - 1) * stride + (size_t)cols;
}

static bool ranges_intersect(const uint8_t *a, size_t na, const uint8_t *b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

int orbx_clahe_band_lut_rows(int rows, int tiles_y, int y0, int y1, int *first, int *count) {
  if (!first || !count || tiles_y <= 0 || rows < tiles_y || y0 < 0 || y1 < y0 || y1 >= rows) return ORBX_E_ARG;
  const int erows = rows % tiles_y == 0 ? rows : rows + tiles_y - rows % tiles_y;
  clahe_band_lut_rows(y0, y1, 1.0f / (float)(erows / tiles_y), tiles_y, *first, *count);
  return 0;
}

int orbx_clahe_batch_device(int nframes, const uint8_t *d_src, int rows, int cols, size_t src_stride, size_t src_frame_stride, double clip_limit,
                            int tiles_x, int tiles_y, uint8_t *d_lut, uint8_t *d_dst, size_t dst_stride, size_t dst_frame_stride, void *stream) {
  if (!d_src || !d_dst || !d_lut || nframes < 0 || rows <= 0 || cols <= 0 || tiles_x <= 0 || tiles_y <= 0 || tiles_x * tiles_y > 256 || cols < tiles_x ||
      rows < tiles_y || src_stride < (size_t)cols || dst_stride < (size_t)cols || !(clip_limit >= 0.0))
    return ORBX_E_ARG;
  if (nframes > 1 && (src_frame_stride < batch_extent(1, rows, cols, src_stride, 0) || dst_frame_stride < batch_extent(1, rows, cols, dst_stride, 0)))
    return ORBX_E_ARG;
  if (nframes == 0) return 0;
  const bool in_place = d_dst == d_src && dst_stride == src_stride && (nframes == 1 || dst_frame_stride == src_frame_stride);
  if (!in_place && ranges_intersect(d_src, batch_extent(nframes, rows, cols, src_stride, src_frame_stride), d_dst,
                                    batch_extent(nframes, rows, cols, dst_stride, dst_frame_stride)))
    return ORBX_E_ARG;
  ClaheBatch P;
  P.src = d_src; P.dst = d_dst; P.lut = d_lut;
  P.sstride = src_stride; P.sframe = src_frame_stride; P.dstride = dst_stride; P.dframe = dst_frame_stride;
  P.nframes = nframes; P.rows = rows; P.cols = cols; P.tilesX = tiles_x; P.tilesY = tiles_y;
  clahe_batch_geometry(P, clip_limit);
  const int nbands = (rows + CLAHE_BAND_ROWS - 1) / CLAHE_BAND_ROWS, gridF = std::min(nframes, 65535);
  int maxRows = 0;   // the most table rows any band stages
  for (int b = 0; b < nbands; b++) {
    int first, count;
    clahe_band_lut_rows(b * CLAHE_BAND_ROWS, std::min((b + 1) * CLAHE_BAND_ROWS, rows) - 1, P.inv_th, tiles_y, first, count);
    maxRows = std::max(maxRows, count);
  }
  // threads of the blend: one per column quad, the rest of the workgroup as row phases, whole wavefronts
  const int nq = (cols + 3) / 4;
  const int threads = nq >= 256 ? 256 : std::min(256, (nq * (256 / nq) + 63) / 64 * 64);
  hipLaunchKernelGGL(k_clahe_lut_batch, dim3(tiles_x * tiles_y, gridF), dim3(256), 0, (hipStream_t)stream, P);
  hipLaunchKernelGGL(k_clahe_interp_batch, dim3(nbands, gridF), dim3(threads), ClaheCarve::of(maxRows, tiles_x).bytes, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbx_remap_linear_batch_device(int nframes, const uint8_t *d_src, int src_rows, int src_cols, size_t src_stride, size_t src_frame_stride,
                                   const float *d_mapx, const float *d_mapy, size_t map_stride_elems, int rows, int cols, uint8_t *d_dst,
                                   size_t dst_stride, size_t dst_frame_stride, void *stream) {
  if (!d_src || !d_mapx || !d_mapy || !d_dst || nframes < 0 || src_rows <= 0 || src_cols <= 0 || rows <= 0 || cols <= 0 || src_stride < (size_t)src_cols ||
      map_stride_elems < (size_t)cols || dst_stride < (size_t)cols || src_cols > 32767 || src_rows > 32767 || rows > 65535)
    return ORBX_E_ARG;
  if (nframes > 1 && (src_frame_stride < batch_extent(1, src_rows, src_cols, src_stride, 0) || dst_frame_stride < batch_extent(1, rows, cols, dst_stride, 0)))
    return ORBX_E_ARG;
  if (nframes == 0) return 0;
  if (ranges_intersect(d_src, batch_extent(nframes, src_rows, src_cols, src_stride, src_frame_stride), d_dst,
                       batch_extent(nframes, rows, cols, dst_stride, dst_frame_stride)))
    return ORBX_E_ARG;
  RemapBatch P;
  P.src = d_src; P.dst = d_dst; P.mapx = d_mapx; P.mapy = d_mapy;
  P.sstride = src_stride; P.sframe = src_frame_stride; P.mstride = map_stride_elems; P.dstride = dst_stride; P.dframe = dst_frame_stride;
  P.nframes = nframes; P.srows = src_rows; P.scols = src_cols; P.rows = rows; P.cols = cols;
  const int nchunks = (nframes + REMAP_FRAME_CHUNK - 1) / REMAP_FRAME_CHUNK;
  const dim3 grid((cols + 255) / 256, rows, std::min(nchunks, 65535));
  if (src_cols >= 2) hipLaunchKernelGGL(k_remap_linear_batch<true>, grid, dim3(256), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL(k_remap_linear_batch<false>, grid, dim3(256), 0, (hipStream_t)stream, P);   // no column pair in a one-column source
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbx_level_info(const orbx_t *h, int level, int *rows, int *cols) {
  if (!h || level < 0 || level >= h->nlevels || h->geom.empty()) return ORBX_E_ARG;
  if (rows) *rows = h->geom[level].h;
  if (cols) *cols = h->geom[level].w;
  return 0;
}

static int download_plane(orbx_t *h, const uint8_t *src, size_t spitch, int w, int hh, int border, uint8_t *dst, size_t dst_stride) {
  std::vector<uint8_t> tmp((size_t)w * hh);
  XCHECK(h, join_last(h));
  XCHECK(h, hipMemcpy2DAsync(tmp.data(), (size_t)w, src, spitch, (size_t)w, (size_t)hh, hipMemcpyDeviceToHost, h->stream));
  XCHECK(h, hipStreamSynchronize(h->stream));
  auto refl = [](int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
  };
  for (int y = -border; y < hh + border; y++) {
    const uint8_t *S = tmp.data() + (size_t)refl(y, hh) * w;
    uint8_t *D = dst + (size_t)(y + border) * dst_stride;
    for (int x = -border; x < w + border; x++) D[x + border] = S[refl(x, w)];
  }
  return 0;
}

int orbx_download_level(orbx_t *h, int frame, int level, int border, uint8_t *dst, size_t dst_stride) {
  if (!h || !h->have_last || !dst || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last.nframes || border < 0) return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  const LevelGeom &G = h->geom[level];
  if (dst_stride < (size_t)(G.w + 2 * border)) return ORBX_E_ARG;
  if (level == 0)
    return download_plane(h, h->last.img0 + (size_t)frame * h->last.img0_frame_stride, h->last.img0_stride, G.w, G.h, border, dst, dst_stride);
  return download_plane(h, h->last.pyr + (size_t)frame * h->last.pyr_fs + G.off, (size_t)G.pitch, G.w, G.h, border, dst, dst_stride);
}

// mvImagePyramid of one frame in ONE transfer: every level with its BORDER_REFLECT_101 frame (ORBextractor.cc:1203-1215) is
// written by one kernel into a packed device buffer, copied once into pinned memory and from there into the caller's block.
struct PackLevel { const uint8_t *src; int spitch, w, h, dstride; unsigned doff, dbytes; };
struct PackParams { PackLevel L[ORBX_MAX_LEVELS]; int nlevels, border; uint8_t *dst; };
}  // extern "C"
__global__ __launch_bounds__(256) void k_pyramid_pack(PackParams P) {
  const PackLevel G = P.L[blockIdx.y];
  auto refl = [](int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
  };
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < G.dbytes; i += gridDim.x * 256u) {
    const int y = (int)(i / (unsigned)G.dstride) - P.border, x = (int)(i % (unsigned)G.dstride) - P.border;
    P.dst[G.doff + i] = G.src[(size_t)refl(y, G.h) * G.spitch + refl(x, G.w)];
  }
}
extern "C" {
int orbx_download_pyramid(orbx_t *h, int frame, int border, uint8_t *dst, size_t dst_bytes, size_t *offsets, size_t *strides) {
  if (!h || !h->have_last || frame < 0 || frame >= h->last.nframes || border < 0 || border > 64 || !offsets || !strides) return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  PackParams P;
  memset(&P, 0, sizeof(P));
  P.nlevels = h->nlevels; P.border = border;
  size_t total = 0;
  for (int l = 0; l < h->nlevels; l++) {
    const LevelGeom &G = h->geom[l];
    PackLevel &L = P.L[l];
    L.src = l == 0 ? h->last.img0 + (size_t)frame * h->last.img0_frame_stride : h->last.pyr + (size_t)frame * h->last.pyr_fs + G.off;
    L.spitch = l == 0 ? (int)h->last.img0_stride : G.pitch;
    L.w = G.w; L.h = G.h; L.dstride = G.w + 2 * border;
    L.doff = (unsigned)total; L.dbytes = (unsigned)((size_t)L.dstride * (size_t)(G.h + 2 * border));
    offsets[l] = total; strides[l] = (size_t)L.dstride;
    total += ((size_t)L.dbytes + 63) & ~(size_t)63;
  }
  if (!dst) return (int)std::min<size_t>(total, 0x7fffffff);   // size query
  if (dst_bytes < total) return ORBX_E_CAP;
  XCHECK(h, h->d_pyrpack.reserve(total));
  if (h->pin_pyr_bytes < total) {
    if (h->pin_pyr) (void)hipHostFree(h->pin_pyr);
    h->pin_pyr = nullptr; h->pin_pyr_bytes = 0;
    XCHECK(h, hipHostMalloc(&h->pin_pyr, total, hipHostMallocDefault));
    h->pin_pyr_bytes = total;
  }
  P.dst = (uint8_t *)h->d_pyrpack.p;
  if (h->last_pending) XCHECK(h, hipStreamWaitEvent(h->stream, h->last_done, 0));
  hipLaunchKernelGGL(k_pyramid_pack, dim3(64, h->nlevels), dim3(256), 0, h->stream, P);
  XCHECK(h, hipGetLastError());
  XCHECK(h, hipMemcpyAsync(h->pin_pyr, h->d_pyrpack.p, total, hipMemcpyDeviceToHost, h->stream));
  XCHECK(h, hipStreamSynchronize(h->stream));
  memcpy(dst, h->pin_pyr, total);
  return (int)std::min<size_t>(total, 0x7fffffff);
}

int orbx_download_blurred_level(orbx_t *h, int frame, int level, uint8_t *dst, size_t dst_stride) {
  if (!h || !h->have_last || !dst || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last.nframes) return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  const LevelGeom &G = h->geom[level];
  if (dst_stride < (size_t)G.w) return ORBX_E_ARG;
  return download_plane(h, h->last.blur + (size_t)frame * h->last.blur_fs + G.boff, (size_t)G.bpitch, G.w, G.h, 0, dst, dst_stride);
}

static int download_packed(orbx_t *h, const uint32_t *src, int n, float *xyr, int cap) {
  std::vector<uint32_t> tmp((size_t)std::max(n, 1));
  if (n > 0) XCHECK(h, copy_on(h->stream, tmp.data(), src, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n && i < cap; i++) {
    xyr[3 * i] = (float)(tmp[i] & 0xfff);
    xyr[3 * i + 1] = (float)((tmp[i] >> 12) & 0xfff);
    xyr[3 * i + 2] = (float)(tmp[i] >> 24);
  }
  return n;
}

int orbx_download_candidates(orbx_t *h, int frame, int level, float *xyr, int cap) {
  if (!h || !h->have_last || !xyr || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last.nframes) return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  XCHECK(h, join_last(h));
  int32_t n = 0;
  XCHECK(h, copy_on(h->stream, &n, h->last.candCnt + (size_t)frame * h->nlevels + level, sizeof(n), hipMemcpyDeviceToHost));
  return download_packed(h, h->last.cand + (size_t)frame * h->last.cand_fs + h->geom[level].candBase, n, xyr, cap);
}

int orbx_download_level_keypoints(orbx_t *h, int frame, int level, float *xyr, int cap) {
  if (!h || !h->have_last || !xyr || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last.nframes) return ORBX_E_ARG;
  XCHECK(h, hipSetDevice(h->device));
  XCHECK(h, join_last(h));
  int32_t n[2] = {0, 0};
  XCHECK(h, copy_on(h->stream, n, h->last.lcnt + ((size_t)frame * h->nlevels + level) * 2, sizeof(n), hipMemcpyDeviceToHost));
  return download_packed(h, h->last.lkp + (size_t)frame * h->last.lkp_fs + h->geom[level].kpBase, n[0], xyr, cap);
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------------------
// matcher
// --------------------------------------------------------------------------------------------------------------
struct orbm_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  int scan_mode = 0;        // SCAN_AUTO / SCAN_DENSE / SCAN_WALK of the projection searches (orbm_set_scan_mode)
  int hamming_engine = 2;   // orbm_set_hamming_engine: 0 vector ALU, 1 k_match_scan_mfma, 2 (default) + lists built inside k_match_resolve for all-open pairs
  DevBuf d_block;     // inputs + outputs of one host-pointer entry point, one block (see Staging)
  void *pin = nullptr; size_t pin_bytes = 0;   // its pinned host mirror
  DevBuf d_topk;      // per-query candidate lists of the scan / walk, for the resolve (all projection searches)
  DevBuf d_rank;      // k_match_rank's two tables (accumulator seeds, Key32 tie-break bits) for k_match_scan_mfma
  DevBuf d_cand;      // fused k_match_resolve: every pair's descriptors and candidate records in sorted order (48 B per keypoint)
  DevBuf d_lfq;       // query arrays written by k_lastframe_project (orbm_search_by_projection_last_frame_batch_device)
  DevBuf d_lmq;       // query arrays written by k_local_map_project (orbm_search_local_points*): never shared with d_lfq (kept: two buffers)
  DevBuf d_knn;       // the two nearest right rows of every left lapping row (orbm_stereo_fisheye_matches*)
  DevBuf d_partner;   // stereo-partner table built by k_local_map_project_rig (orbm_search_local_points_fisheye*)
  DevBuf d_tri_count, d_tri_keys;   // k_triangulation_candidates: per-item offsets and counts + total, candidate keys
  DevBuf d_cull;      // tables and state of an open stepwise KeyFrameCulling walk (orbm_keyframe_culling_open / _step): no other entry uses it
  CullParams cull{};  // its device addresses inside d_cull
  bool cull_open = false, cull_any = false;   // a walk is open; one of its erases has been applied
  int cull_next = 0, cull_pending = -1;       // the next keyframe to walk; the passing keyframe the last step returned, or -1
  DevBuf d_lm, d_lm_flag;   // scratch of orbm_update_local_map_device (counters, per-point word, keyframe list) and of orbm_gather_local_map_device ([P] flags)
  std::mutex lm_mu;         // held by the UpdateLocalMap / UpdateConnections / gather entries: threads may share a handle for THESE entries
  std::vector<uint8_t> lm_back;   // orbm_update_connections: its outputs on the host (capacity only grows)
  int vote_form = 0;        // k_covis_vote: 0 LDS table, 1 one global atomic per vote (ORBM_VOTE_FORM, measurements only)
  std::vector<BowCandItem> bow_items;   // host side of the one-call SearchByBoW, kept between calls (capacity only grows)
  std::vector<BowCand> bow_cands;
  std::vector<float> bow_ang;
  int tri_layout = 0;       // item order of the one-call triangulation searches: 0 neighbour-major (the merge walks' order), 1 KF1-keypoint-major (ORBM_TRI_LAYOUT, measurements only)
  bool profiling = false;
  hipEvent_t ev[PROF_DEPTH][3] = {};
  int prof_head = 0;
  bool ev_ok = false, ms_valid = false;
  std::string err;
};

#define MCHECK(m, call)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (m)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return ORBX_E_HIP;                                                                      \
    }                                                                                         \
  } while (0)

#if defined(RESOLVE_STAMPS) || defined(WALK_STAMPS) || defined(SCAN_STAMPS) || defined(MF_STAMPS) || defined(WIDE_STAMPS)
static void *getenv_ptr(const char *name) { const char *e = getenv(name); return e ? (void *)strtoull(e, nullptr, 0) : nullptr; }
#endif

// Inputs of a host-pointer entry point as ONE block: the parts lie at 256-byte offsets in m->d_block, those with a source are
// copied into the pinned mirror m->pin and uploaded with one H2D copy (a dozen pageable copies would each stage and synchronise
// on their own).  A part without a source reserves an output-only region.  The mirror spans the outputs too only when the caller
// downloads them through it (mirror_outputs); a large output copied straight to the caller takes no pinned memory.
// add() / out() return the part's typed handle; its offset in the block is known from then on (offset(): what the records of the
// one-call entries store), after upload() dev() / host() are its device / pinned-mirror address, dev() nullptr for an empty part.
template <class T> struct PartOf { int i; };
struct Staging {
  struct Slot { const void *src; size_t bytes, off; };
  orbm_handle *m;
  int n = 0;
  size_t total = 0, up = 0;   // bytes of the block so far; of its front that ends with the last part that has a source
  bool too_large = false;
  Slot inl[32];               // the largest per-frame block (the rig local-map form) has 29 parts: no allocation on that way
  std::vector<Slot> more;     // the one-call entries, a few parts per neighbour, target or candidate
  const Slot &at(int i) const { return i < 32 ? inl[i] : more[(size_t)i - 32]; }
  template <class T> PartOf<T> add(const T *src, size_t count) {
    const size_t bytes = sizeof(T) * count;   // sizes come from the caller's counts: one beyond any allocation fails as that allocation would
    const bool fits = bytes <= (SIZE_MAX >> 3) - total;
    if (!fits) too_large = true;              // upload() refuses; until then the handle names an empty part
    const Slot p{src, fits ? bytes : 0, total};
    if (n < 32) inl[n] = p;
    else { if (more.empty()) more.reserve(96); more.push_back(p); }   // one allocation serves K = 20 neighbours of six parts
    total += (p.bytes + 255) & ~(size_t)255;  // what a part takes of the block
    if (src) up = total;
    return {n++};
  }
  template <class T> PartOf<T> out(size_t count) { return add((const T *)nullptr, count); }
  int upload(hipStream_t s, bool mirror_outputs = true) {
    if (too_large) { m->err = "staging: inputs too large"; return ORBX_E_HIP; }
    const size_t mirror = mirror_outputs ? total : up;
    if (m->pin_bytes < mirror) {
      if (m->pin) (void)hipHostFree(m->pin);
      m->pin = nullptr; m->pin_bytes = 0;
      MCHECK(m, hipHostMalloc(&m->pin, 2 * mirror, hipHostMallocDefault));   // grown rarely: a re-allocation costs tens of milliseconds
      m->pin_bytes = 2 * mirror;
    }
    MCHECK(m, m->d_block.reserve(m->d_block.bytes >= total ? total : 2 * total));
    for (int i = 0; i < n; i++)
      if (at(i).src && at(i).bytes) memcpy((uint8_t *)m->pin + at(i).off, at(i).src, at(i).bytes);
    if (up) MCHECK(m, hipMemcpyAsync(m->d_block.p, m->pin, up, hipMemcpyHostToDevice, s));
    return 0;
  }
  const uint8_t *block() const { return (const uint8_t *)m->d_block.p; }
  template <class T> size_t offset(PartOf<T> h) const { return at(h.i).off; }
  template <class T> T *dev(PartOf<T> h) const { return at(h.i).bytes ? (T *)((uint8_t *)m->d_block.p + at(h.i).off) : nullptr; }
  template <class T> T *host(PartOf<T> h) const { return (T *)((uint8_t *)m->pin + at(h.i).off); }
  // Adjacent parts as one span, from the start of part a to the end of part b: down into the mirror in one copy, or filled with one byte
  template <class A, class B> size_t span(PartOf<A> a, PartOf<B> b) const { return at(b.i).off + at(b.i).bytes - at(a.i).off; }
  template <class A, class B> hipError_t download(hipStream_t s, PartOf<A> a, PartOf<B> b) const {
    return hipMemcpyAsync((uint8_t *)m->pin + at(a.i).off, block() + at(a.i).off, span(a, b), hipMemcpyDeviceToHost, s);
  }
  template <class A, class B> hipError_t fill(hipStream_t s, PartOf<A> a, PartOf<B> b, int byte) const {
    return hipMemsetAsync((uint8_t *)m->d_block.p + at(a.i).off, byte, span(a, b), s);
  }
};

// The structs the host-pointer forms stage: stage_*() appends the parts (absent arrays as empty ones), on_device() is the device-side struct.
struct StagedFrame { const orbm_frame_t *f; PartOf<orbx_keypoint_t> kp; PartOf<uint8_t> desc; PartOf<float> ur; };
static StagedFrame stage_frame(Staging &S, const orbm_frame_t *f, bool with_ur = true) {   // with_ur false: u_right = NULL on the device
  const size_t n = (size_t)f->n;
  const float *ur = with_ur ? f->u_right : nullptr;
  return {f, S.add(f->keys_un, n), S.add(f->descriptors, 32 * n), S.add(ur, ur ? n : 0)};
}
static orbm_frame_t on_device(const Staging &S, const StagedFrame &h) {
  orbm_frame_t d = *h.f;
  d.keys_un = S.dev(h.kp); d.descriptors = S.dev(h.desc); d.u_right = S.dev(h.ur);
  return d;
}
struct StagedLast { int n; PartOf<uint8_t> has; PartOf<float> xw; PartOf<uint8_t> md; PartOf<orbx_keypoint_t> lk; PartOf<uint8_t> obs; PartOf<float> tc, tl; };
static StagedLast stage_last_frame(Staging &S, const orbm_last_frame_t &l) {   // one problem: 16 floats of Tcw / Tlw
  const size_t n = (size_t)l.n;
  return {l.n, S.add(l.has_mp, n), S.add(l.Xw, 3 * n), S.add(l.mpdesc, 32 * n), S.add(l.last_keys, n), S.add(l.obs, l.obs ? n : 0),
          S.add(l.Tcw, 16), S.add(l.Tlw, 16)};
}
static orbm_last_frame_t on_device(const Staging &S, const StagedLast &h) {
  orbm_last_frame_t d;
  d.n = h.n; d.has_mp = S.dev(h.has); d.Xw = S.dev(h.xw); d.mpdesc = S.dev(h.md); d.last_keys = S.dev(h.lk); d.obs = S.dev(h.obs);
  d.Tcw = S.dev(h.tc); d.Tlw = S.dev(h.tl);
  return d;
}
struct StagedMap { int n; PartOf<uint8_t> elig; PartOf<float> xw, nrm, maxd, mind; PartOf<uint8_t> md, obs; PartOf<float> tc; };
static StagedMap stage_local_map(Staging &S, const orbm_local_map_t *map) {   // one problem: 16 floats of Tcw
  const size_t n = (size_t)map->n;
  return {map->n, S.add(map->eligible, n), S.add(map->Xw, 3 * n), S.add(map->normal, 3 * n), S.add(map->max_dist, n), S.add(map->min_dist, n),
          S.add(map->mpdesc, 32 * n), S.add(map->obs, map->obs ? n : 0), S.add(map->Tcw, 16)};
}
static orbm_local_map_t on_device(const Staging &S, const StagedMap &h) {
  orbm_local_map_t d;
  d.n = h.n; d.eligible = S.dev(h.elig); d.Xw = S.dev(h.xw); d.normal = S.dev(h.nrm); d.max_dist = S.dev(h.maxd); d.min_dist = S.dev(h.mind);
  d.mpdesc = S.dev(h.md); d.obs = S.dev(h.obs); d.Tcw = S.dev(h.tc);
  return d;
}

// One side of a ragged batch: problem p at element offset p * stride, live count d_n[p * n_stride] (device) or, d_n == NULL, n.
struct Ragged {
  int stride; const int32_t *d_n; int n_stride; int n;
  int max() const { return d_n ? stride : n; }                                   // what scratch and grids are sized for
  bool valid() const { return max() > 0 && stride >= max() && n >= 0; }          // the one validity rule of a side
  LiveCount live() const { return {d_n, n_stride, n}; }
};

// Options of one projection search beyond the arguments of orbm_search_by_projection_batch_device (see MatchProblemSet); the
// defaults are a plain search.  Pointers are device addresses.
struct SearchOpts {
  int scan_mode = SCAN_AUTO;   // SCAN_AUTO / SCAN_DENSE / SCAN_WALK; frames beyond 2048 keypoints are scanned whatever it says
  int couple = 0, serial = 0;               // fisheye-stereo frames
  LiveCount nleft = {nullptr, 0, 0};        // Nleft per problem
  const int32_t *partner = nullptr;
  const uint8_t *qside = nullptr;
  uint8_t *qany = nullptr;
  int init_th_low = -1;        // >= 0: SearchForInitialization's resolve instead of the claim loop
  bool fuse = false;           // Fuse: the chi-square gate with inv_sigma2[level]
  float inv_sigma2[16] = {};
};

template <int V> using ScanKind = std::integral_constant<int, V>;

// ---- helpers of the C entry points below that are templates (C++ linkage) ----------------------------------------------------
// A refusal of a one-call entry: m->err names item j of the entry's kind ("neighbour 3: ..."), j < 0 the call as a whole; a kind of NULL
// never names an item (the pair forms).
struct Refuse {
  orbm_handle *m; const char *kind;
  int operator()(int j, const char *why) const {
    m->err = j < 0 || !kind ? std::string(why) : std::string(kind) + " " + std::to_string(j) + ": " + why;
    return ORBX_E_ARG;
  }
};
// Rotation-consistency check of every matcher with checkOri (e.g. ORBmatcher.cc:2177-2185 + :2263-2286): a match goes into the bin
// of the angle difference of its two keypoints (rot_bin); matches outside the three fullest bins (three_maxima) are pruned.  What an id
// is and what pruning does to it stay with the caller.
struct RotHist {
  std::vector<int> bins[ORBM_HISTO_LENGTH];
  void add(float rot, int id) {
    const int bin = rot_bin(rot);
    if (bin >= 0 && bin < ORBM_HISTO_LENGTH) bins[bin].push_back(id);
  }
  template <class F> void for_each_pruned(F fn) const {
    int sizes[ORBM_HISTO_LENGTH], ind1, ind2, ind3;
    for (int i = 0; i < ORBM_HISTO_LENGTH; i++) sizes[i] = (int)bins[i].size();
    three_maxima(sizes, ORBM_HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < ORBM_HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int id : bins[i]) fn(id);
    }
  }
};

// per-level geometry and scale of StereoParams / StereoBatchParams
template <class Params> static void fill_stereo_levels(const orbx_t *hl, Params &S) {
  for (int l = 0; l < hl->nlevels; l++) {
    const LevelGeom &G = hl->geom[l];
    S.w[l] = G.w; S.h[l] = G.h; S.pitch[l] = G.pitch; S.off[l] = G.off;
    S.sf[l] = hl->mvScaleFactor[l]; S.invsf[l] = hl->mvInvScaleFactor[l];
  }
  S.nlevels = hl->nlevels; S.rows = hl->rows;
}

extern "C" {

orbm_t *orbm_create(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
  if (hipSetDevice(device) != hipSuccess || raise_lds_limits(device) != hipSuccess) return nullptr;
  orbm_handle *m = new orbm_handle();
  m->device = device;
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; return nullptr; }
  if (const char *e = getenv("ORBM_SCAN_MODE")) { const int v = atoi(e); if (v >= SCAN_AUTO && v <= SCAN_WALK) m->scan_mode = v; }   // measurements only; see orbm_set_scan_mode
  if (const char *e = getenv("ORBM_VOTE_FORM")) m->vote_form = atoi(e) == 1;   // measurements only; DESIGN.md 6
  if (const char *e = getenv("ORBM_TRI_LAYOUT")) m->tri_layout = atoi(e) == 1;                                                                                           // measurements only; DESIGN.md 6
  if (const char *e = getenv("ORBM_HAMMING_ENGINE")) { const int v = atoi(e); if (v >= 0 && v <= 2) m->hamming_engine = v; }                                               // measurements only; see orbm_set_hamming_engine
  return m;
}

void orbm_destroy(orbm_t *m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  DevBuf *bufs[] = {&m->d_block, &m->d_topk, &m->d_rank, &m->d_cand, &m->d_lfq, &m->d_lmq, &m->d_knn, &m->d_partner, &m->d_tri_count, &m->d_tri_keys, &m->d_cull, &m->d_lm, &m->d_lm_flag};
  for (DevBuf *b : bufs) b->release();
  if (m->pin) (void)hipHostFree(m->pin);
  if (m->ev_ok)
    for (auto &set : m->ev)
      for (auto &e : set) (void)hipEventDestroy(e);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
}

const char *orbm_last_error(const orbm_t *m) { return m ? m->err.c_str() : "null handle"; }

void orbm_set_profiling(orbm_t *m, int enable) {
  if (!m) return;
  m->profiling = enable != 0;
  m->prof_head = 0;
  m->ms_valid = false;
  if (m->profiling && !m->ev_ok) {
    (void)hipSetDevice(m->device);
    bool ok = true;
    for (auto &set : m->ev)
      for (auto &e : set) ok = ok && hipEventCreate(&e) == hipSuccess;
    m->ev_ok = ok;
  }
}

// 0 = decided per frame pair on the device (default), 1 = always k_match_scan, 2 = always k_match_walk (frames of at most 2048
// keypoints; larger ones are scanned whatever the mode).  Results do not depend on the mode.
int orbm_set_scan_mode(orbm_t *m, int mode) {
  if (!m || mode < SCAN_AUTO || mode > SCAN_WALK) return ORBX_E_ARG;
  m->scan_mode = mode;
  return 0;
}

// Where open-window searches compute their Hamming distances: 0 = vector ALU (k_match_scan) like every other block, 1 = the
// all-keypoints scan of open-window query blocks on the matrix pipe (k_match_scan_mfma), 2 (default) = as 1, and frame pairs ALL of
// whose queries are open build their lists inside k_match_resolve (fused form: claimed keypoints masked per 512-query super-chunk).
// Results do not depend on it.
int orbm_set_hamming_engine(orbm_t *m, int engine) {
  if (!m || engine < 0 || engine > 2) return ORBX_E_ARG;
  m->hamming_engine = engine;
  return 0;
}

float orbm_get_last_ms(orbm_t *m) {
  if (!m || !m->profiling || !m->ev_ok || !m->ms_valid || m->prof_head <= 0) return -1.f;
  float t = -1.f;
  hipEvent_t *e = m->ev[(m->prof_head - 1) % PROF_DEPTH];
  if (hipEventSynchronize(e[2]) != hipSuccess) return -1.f;
  if (hipEventElapsedTime(&t, e[0], e[2]) != hipSuccess) return -1.f;
  return t;
}

// {scan, resolve} averaged over the searches launched since profiling was switched on (the PROF_DEPTH most recent ones).
int orbm_get_stage_ms(orbm_t *m, float *ms, int cap) {
  if (!m || !ms || cap < 2 || !m->profiling || !m->ev_ok || !m->ms_valid || m->prof_head <= 0) return 0;
  const int nb = std::min(m->prof_head, PROF_DEPTH);
  if (hipEventSynchronize(m->ev[(m->prof_head - 1) % PROF_DEPTH][2]) != hipSuccess) return 0;
  ms[0] = ms[1] = 0.f;
  for (int b = 0; b < nb; b++) {
    hipEvent_t *e = m->ev[(m->prof_head - 1 - b) % PROF_DEPTH];
    float t0 = 0, t1 = 0;
    if (hipEventElapsedTime(&t0, e[0], e[1]) != hipSuccess || hipEventElapsedTime(&t1, e[1], e[2]) != hipSuccess) return 0;
    ms[0] += t0 / (float)nb;
    ms[1] += t1 / (float)nb;
  }
  return 2;
}

// ORBmatcher.cc:2463-2483 (the bit trick there computes exactly popcount)
int orbm_descriptor_distance(const uint8_t *a, const uint8_t *b) {
  if (!a || !b) return ORBX_E_ARG;
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    uint32_t pa, pb;
    memcpy(&pa, a + 4 * i, 4);
    memcpy(&pb, b + 4 * i, 4);
    dist += __builtin_popcount(pa ^ pb);
  }
  return dist;
}

void orbm_three_maxima(const int *histo, int L, int *ind1, int *ind2, int *ind3) {  // ORBmatcher.cc:2416-2458
  if (!ind1 || !ind2 || !ind3) return;
  three_maxima(histo, histo ? L : 0, *ind1, *ind2, *ind3);   // no histogram: -1, -1, -1
}

float orbm_radius_by_viewing_cos(float viewCos) { return radius_by_viewing_cos(viewCos); }

void orbm_undistort_keypoints(int n, const orbx_keypoint_t *keys, const float *K, const float *D, int nD, orbx_keypoint_t *keys_un) {
  if (!keys || !keys_un || !K || !D) return;
  for (int i = 0; i < n; i++) {
    orbx_keypoint_t k = keys[i];
    if (D[0] != 0.0f) undistort_point((double)keys[i].x, (double)keys[i].y, K, D, nD, &k.x, &k.y);
    keys_un[i] = k;
  }
}

void orbm_image_bounds(int cols, int rows, const float *K, const float *D, int nD, float *min_x, float *max_x, float *min_y, float *max_y) {
  if (!K || !D || !min_x || !max_x || !min_y || !max_y) return;
  if (D[0] != 0.0f) {
    const float c[4][2] = {{0.f, 0.f}, {(float)cols, 0.f}, {0.f, (float)rows}, {(float)cols, (float)rows}};
    float o[4][2];
    for (int i = 0; i < 4; i++) undistort_point((double)c[i][0], (double)c[i][1], K, D, nD, &o[i][0], &o[i][1]);
    *min_x = std::min(o[0][0], o[2][0]);
    *max_x = std::max(o[1][0], o[3][0]);
    *min_y = std::min(o[0][1], o[1][1]);
    *max_y = std::max(o[2][1], o[3][1]);
  } else {
    *min_x = 0.0f; *max_x = (float)cols; *min_y = 0.0f; *max_y = (float)rows;
  }
}

int orbm_undistort_keypoints_batch_device(orbm_t *m, const orbx_keypoint_t *d_keys, int key_stride, const int32_t *d_counts, int count_stride,
                                          int n_const, int nframes, const float *K, const float *D, int nD, orbx_keypoint_t *d_keys_un, void *stream_) {
  if (!m || !d_keys || !d_keys_un || !K || !D || nframes <= 0 || key_stride <= 0 || (nD != 4 && nD != 5)) return ORBX_E_ARG;
  if (!d_counts && (n_const < 0 || n_const > key_stride)) return ORBX_E_ARG;
  MCHECK(m, hipSetDevice(m->device));
  UndistortParams U;
  memset(&U, 0, sizeof(U));
  U.keys = reinterpret_cast<const float *>(d_keys); U.keys_un = reinterpret_cast<float *>(d_keys_un); U.key_stride = key_stride;
  U.count = {d_counts, count_stride, n_const};
  for (int i = 0; i < 4; i++) U.K[i] = K[i];
  for (int i = 0; i < nD; i++) U.D[i] = D[i];
  U.nD = nD;
  const int maxn = d_counts ? key_stride : n_const;
  if (maxn == 0) return 0;
  hipLaunchKernelGGL(k_undistort, dim3((maxn + 255) / 256, nframes), dim3(256), 0, (hipStream_t)stream_, U);
  MCHECK(m, hipGetLastError());
  return 0;
}

void orbm_project(int cam_type, const float *p, float X, float Y, float Z, float *u, float *v) {
  if (!p || !u || !v) return;
  project(cam_type, p, X, Y, Z, *u, *v);
}

// What every search refuses about its frame side (frame.n = f->n); the cores run it before their first launch.  No stride >= n: never asked.
static int check_search_frame(orbm_t *m, const orbm_frame_t *f, const Ragged &frame) {
  if (!f->keys_un || !f->descriptors || !(f->max_x > f->min_x) || !(f->max_y > f->min_y)) return ORBX_E_ARG;
  if (frame.max() > ORBM_MAX_KEYPOINTS) { m->err = "more than 15360 keypoints per frame not supported by the search kernels"; return ORBX_E_ARG; }
  return frame.max() <= 0 ? ORBX_E_ARG : 0;
}

// frame.n = f->n and query.n = q->nq (the callers build both from the structs).
static int search_batch(orbm_t *m, const orbm_frame_t *f, const Ragged &frame, const orbm_queries_t *q, const Ragged &query, int npairs, float nnratio,
                        int th_dist, int use_second, int32_t *d_slot, uint8_t *d_slot_obs, int32_t *d_moq, int32_t *d_bd, int32_t *d_nm, hipStream_t s,
                        const SearchOpts &o) {
  if (!m || !f || !q || npairs <= 0 || !d_slot || !d_slot_obs) return ORBX_E_ARG;
  if (!q->descriptors || !q->u || !q->v || !q->radius || !q->min_level || !q->max_level) return ORBX_E_ARG;
  // bestDist starts at 256 in the reference: a threshold >= 256 would "accept" a query without any candidate (index -1 there)
  if (th_dist < 0 || th_dist > 255) { m->err = "th_dist must be in [0, 255]"; return ORBX_E_ARG; }
  const int rf = check_search_frame(m, f, frame);
  if (rf < 0) return rf;
  const int frame_stride = frame.stride, query_stride = query.stride, maxn = frame.max(), maxq = query.max();
  if (maxq <= 0) return ORBX_E_ARG;
  MCHECK(m, hipSetDevice(m->device));
  MatchProblemSet M;
  memset(&M, 0, sizeof(M));
  M.kp = reinterpret_cast<const float *>(f->keys_un);
  M.desc = f->descriptors;
  M.u_right = f->u_right;
  M.frame_stride = frame_stride; M.frame_n = frame.live();
  M.min_x = f->min_x; M.min_y = f->min_y;
  M.inv_w = (float)ORBM_GRID_COLS / (f->max_x - f->min_x);   // Frame.cc:379
  M.inv_h = (float)ORBM_GRID_ROWS / (f->max_y - f->min_y);   // Frame.cc:380
  M.qdesc = q->descriptors; M.qu = q->u; M.qv = q->v; M.qr = q->radius; M.qur = q->u_r;
  M.qminl = q->min_level; M.qmaxl = q->max_level; M.qflags = q->flags;
  M.query_stride = query_stride; M.query_n = query.live();
  M.nnratio = nnratio; M.th_dist = th_dist; M.use_second = use_second;
  M.slot = d_slot; M.slot_obs = d_slot_obs; M.match_of_query = d_moq; M.best_dist = d_bd; M.nmatches = d_nm;
#if defined(RESOLVE_STAMPS) || defined(WALK_STAMPS) || defined(SCAN_STAMPS) || defined(MF_STAMPS) || defined(WIDE_STAMPS)
  M.dbg = (long long *)getenv_ptr("ORBHIP_DBG_PTR");
#endif
  M.nleft = o.nleft.konst; M.nleft_dev = o.nleft.dev; M.nleft_stride = o.nleft.stride; M.partner = o.partner; M.qside = o.qside; M.couple = o.couple; M.serial = o.serial; M.qany = o.qany;
  for (int i = 0; i < 16; i++) M.inv_sigma2[i] = o.inv_sigma2[i];
  // scratch: TOPK keys per query (grows on demand; not on the steady-state path)
  const bool k32 = maxn <= 2048;  // Key32 holds an 11-bit keypoint index
  // Latency mode: with few problems in flight the scan's candidate loop is the critical path (one workgroup per 256 queries walks
  // every candidate), so the candidate chunks are split over up to 8 workgroups per query block and their top-8 lists merged.
  const int qblocks = (maxq + MATCH_NT - 1) / MATCH_NT;
  int nslices = 1;
  if ((long long)npairs * qblocks <= 32) nslices = std::max(1, std::min(8, (maxn + MATCH_CH - 1) / MATCH_CH));
  const size_t slice_stride = MATCH_TOPK * ((size_t)(npairs - 1) * query_stride + maxq);   // keys per slice
  const size_t need = (k32 ? sizeof(uint32_t) : sizeof(unsigned long long)) * slice_stride * (size_t)nslices;
  if (need > m->d_topk.bytes) {
    MCHECK(m, hipStreamSynchronize(s));
    MCHECK(m, m->d_topk.reserve(need));
  }
  // Window walk (k_match_walk) or full scan (k_match_scan): decided per pair on the device unless a mode is forced; frames beyond
  // 2048 keypoints (Key64) are always scanned.
  const int force = !k32 ? SCAN_DENSE : o.scan_mode;
  // matrix-pipe scan of the open-window query blocks (monocular Key32 problems, batch mode): rank tables for it
  const bool mfma = m->hamming_engine >= 1 && k32 && !o.fuse && !M.qside && !M.partner && !M.u_right && nslices == 1 && force != SCAN_WALK;
  const size_t nrank = (size_t)(npairs - 1) * frame_stride + maxn;
  if (mfma && sizeof(uint32_t) * (2 * nrank + (size_t)npairs) > m->d_rank.bytes) {
    MCHECK(m, hipStreamSynchronize(s));
    MCHECK(m, m->d_rank.reserve(sizeof(uint32_t) * (2 * nrank + (size_t)npairs)));
  }
  const bool prof = m->profiling && m->ev_ok;
  hipEvent_t *pev = m->ev[m->prof_head % PROF_DEPTH];
  if (prof) MCHECK(m, hipEventRecord(pev[0], s));
  M.npairs = npairs; M.scan_qblocks = qblocks;
  const dim3 sgrid(8 * qblocks * ((npairs + 7) / 8), 1, nslices);   // XCD-aware 1-D order, see k_match_scan
  if (nslices > 1 && M.qany) MCHECK(m, hipMemsetAsync(M.qany, 0, (size_t)(npairs - 1) * query_stride + maxq, s));
  // resolve LDS (ResolveCarve, orb_match_kernels.h): records and descriptors in LDS where they fit; the fused form keeps them in d_cand.
  // Serial / coupled problems never take the wide form.
  const ResolveForm rform = resolve_form(maxn, M.partner != nullptr, mfma && m->hamming_engine >= 2 && o.init_th_low < 0 && !M.serial && M.couple == 0);
  const bool ldscand = rform.ldscand, fused = rform.fused;
  const size_t lds = (size_t)rform.bytes;
  // ORBHIP_PRINT_RESOLVE_LDS (measurements, tests/test_gpu_fused_footprint.py): the form and the dynamic LDS of every search launch
  if (getenv("ORBHIP_PRINT_RESOLVE_LDS")) fprintf(stderr, "orbhip: resolve maxn %d fused %d dynamic LDS %zu bytes\n", maxn, (int)fused, lds);
  if (fused && 3 * sizeof(uint4) * (size_t)maxn * (size_t)npairs > m->d_cand.bytes) {
    MCHECK(m, hipStreamSynchronize(s));
    MCHECK(m, m->d_cand.reserve(3 * sizeof(uint4) * (size_t)maxn * (size_t)npairs));
  }
  if (lds > RESOLVE_LDS_MAX) { m->err = "too many keypoints per frame for the search kernels' LDS state (fisheye-stereo frames: at most 13000)"; return ORBX_E_ARG; }
  const dim3 rblock(64 * RESOLVE_NW_OF(fused));
  // The walk's workgroups come first: they are the short ones.
  const int capn = std::min((maxn + 7) & ~7, WALK_MAX_N);
  // few pairs in flight: four lanes per query and four times the workgroups (see k_match_walk)
  const int lpq = (long long)npairs * qblocks <= 32 ? 4 : 1;
  const int wqblocks = (maxq + MATCH_NT / lpq - 1) / (MATCH_NT / lpq);
  const WalkCarve<Key32::T> wcarve = WalkCarve<Key32::T>::of(capn, o.fuse || M.u_right, lpq);
  const dim3 wgrid(8 * wqblocks * ((npairs + 7) / 8));
  auto walk = [&](auto kind) {
    constexpr int K = decltype(kind)::value;
    if (lpq > 1) hipLaunchKernelGGL((k_match_walk<Key32, K, 4>), wgrid, dim3(MATCH_NT), wcarve.bytes, s, M, (Key32::T *)m->d_topk.p, force, capn, wqblocks);
    else hipLaunchKernelGGL((k_match_walk<Key32, K, 1>), wgrid, dim3(MATCH_NT), wcarve.bytes, s, M, (Key32::T *)m->d_topk.p, force, capn, wqblocks);
  };
  if (force != SCAN_DENSE) {
    if (o.fuse) walk(ScanKind<SCAN_FUSE>()); else if (M.qside) walk(ScanKind<SCAN_FISHEYE>()); else if (M.u_right) walk(ScanKind<SCAN_UR>()); else walk(ScanKind<SCAN_PLAIN>());
  }
  uint32_t *rec = mfma ? (uint32_t *)m->d_rank.p : nullptr, *keyrec = mfma ? rec + nrank : nullptr, *pairflag = mfma ? keyrec + nrank : nullptr;
  // Engine 2 (fused): the pairs k_match_rank flags make their lists inside k_match_resolve; what is left (pairs with windowed queries)
  // goes to the walk / the vector-ALU scan.  k_match_scan_mfma is not launched then: a launch whose workgroups only read a flag and
  // leave still queues for the kernel's registers and LDS on every CU (0.32 ms average residence beside three other pipelines).
  if (mfma) {
    hipLaunchKernelGGL(k_match_rank, dim3(npairs), dim3(MF_NT), 0, s, M, rec, keyrec, pairflag, fused ? 1 : 0);
    if (!fused)
      hipLaunchKernelGGL(k_match_scan_mfma, dim3(sgrid.x), dim3(MF_NT), 0, s, M, (uint32_t *)m->d_topk.p, (const uint32_t *)rec, (const uint32_t *)keyrec, (const uint32_t *)pairflag);
  }
  const int mf = mfma && !fused ? 1 : 0;
  // scan (+ merge of the slices), then the resolve: key width KT, candidates in LDS or not (LC)
  auto match = [&](auto kt, auto lc) -> int {
    using KT = decltype(kt);
    constexpr bool LC = decltype(lc)::value;
    typename KT::T *topk = (typename KT::T *)m->d_topk.p;
    if (force != SCAN_WALK) {
      if (o.fuse) hipLaunchKernelGGL((k_match_scan<KT, SCAN_FUSE>), sgrid, dim3(MATCH_NT), 0, s, M, topk, slice_stride, force, 0, (const uint32_t *)nullptr);
      else if (M.qside) hipLaunchKernelGGL((k_match_scan<KT, SCAN_FISHEYE>), sgrid, dim3(MATCH_NT), 0, s, M, topk, slice_stride, force, 0, (const uint32_t *)nullptr);
      else if (M.u_right) hipLaunchKernelGGL((k_match_scan<KT, SCAN_UR>), sgrid, dim3(MATCH_NT), 0, s, M, topk, slice_stride, force, 0, (const uint32_t *)nullptr);
      else hipLaunchKernelGGL((k_match_scan<KT, SCAN_PLAIN>), sgrid, dim3(MATCH_NT), 0, s, M, topk, slice_stride, force, mf, (const uint32_t *)pairflag);
      if (nslices > 1) hipLaunchKernelGGL((k_topk_merge<KT>), dim3(qblocks, npairs), dim3(MATCH_NT), 0, s, M, topk, slice_stride, nslices, force);
    }
    if (prof) MCHECK(m, hipEventRecord(pev[1], s));
    if (o.init_th_low >= 0)
      hipLaunchKernelGGL((k_init_resolve<KT>), dim3(npairs), dim3(64), InitResolveCarve::of(maxn).bytes, s, M, (const typename KT::T *)topk, o.init_th_low);
    else
      hipLaunchKernelGGL((k_match_resolve<KT, LC>), dim3(npairs), rblock, lds, s, M, (const typename KT::T *)topk, maxn, force, (const uint32_t *)nullptr,
                         (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    return 0;
  };
  if (fused) {   // Key32, candidates in LDS: the scan launches as above (they return at once for fused pairs), then the fused resolve
    hipLaunchKernelGGL((k_match_scan<Key32, SCAN_PLAIN>), sgrid, dim3(MATCH_NT), 0, s, M, (Key32::T *)m->d_topk.p, slice_stride, force, mf, (const uint32_t *)pairflag);
    if (prof) MCHECK(m, hipEventRecord(pev[1], s));
    hipLaunchKernelGGL((k_match_resolve<Key32, true, true>), dim3(npairs), rblock, lds, s, M, (const Key32::T *)m->d_topk.p, maxn, force, (const uint32_t *)rec,
                       (const uint32_t *)keyrec, (const uint32_t *)pairflag, (uint4 *)m->d_cand.p);
  } else {
    const int rc = k32 ? (ldscand ? match(Key32(), std::true_type()) : match(Key32(), std::false_type()))
                       : (ldscand ? match(Key64(), std::true_type()) : match(Key64(), std::false_type()));
    if (rc < 0) return rc;
  }
  if (prof) { MCHECK(m, hipEventRecord(pev[2], s)); m->prof_head++; m->ms_valid = true; }
  MCHECK(m, hipGetLastError());
  return 0;
}

int orbm_search_by_projection_batch_device(orbm_t *m, const orbm_frame_t *f, int frame_stride, const int32_t *d_frame_n,
                                           int frame_n_stride, const orbm_queries_t *q, int query_stride,
                                           const int32_t *d_query_n, int query_n_stride, int npairs, float nnratio,
                                           int th_dist, int use_second, int32_t *d_slot, uint8_t *d_slot_obs,
                                           int32_t *d_moq, int32_t *d_bd, int32_t *d_nm, void *stream_) {
  if (!m) return ORBX_E_ARG;
  SearchOpts o;
  o.scan_mode = m->scan_mode;
  return search_batch(m, f, {frame_stride, d_frame_n, frame_n_stride, f ? f->n : 0}, q, {query_stride, d_query_n, query_n_stride, q ? q->nq : 0}, npairs,
                      nnratio, th_dist, use_second, d_slot, d_slot_obs, d_moq, d_bd, d_nm, (hipStream_t)stream_, o);   // verbatim: NULL is the device's default stream
}

// The tail of a host search whose outputs were staged as [slot .. nm] (the one count): that range comes down through the pinned mirror in one copy
// and one synchronisation; slot / slot_obs (n entries; nothing when n == 0) are copied out and the match count is returned.
static int download_slots(orbm_t *m, hipStream_t s, const Staging &S, PartOf<int32_t> hslot, PartOf<uint8_t> hsobs, PartOf<int32_t> hnm, int n,
                          int32_t *slot, uint8_t *slot_obs) {
  MCHECK(m, S.download(s, hslot, hnm));
  MCHECK(m, hipStreamSynchronize(s));
  int32_t nm = 0;
  if (n > 0) {
    memcpy(slot, S.host(hslot), sizeof(int32_t) * (size_t)n);
    memcpy(slot_obs, S.host(hsobs), (size_t)n);
    nm = *S.host(hnm);
  }
  return nm;
}

// One host-pointer search: inputs up as one staged block, outputs down as one block, one synchronisation.  partner / qside: host
// arrays of a fisheye-stereo search, staged here; o carries the rest of its options (o.scan_mode is set here).
static int search_host(orbm_t *m, const orbm_frame_t *f, const orbm_queries_t *q, float nnratio, int th_dist, int use_second, int32_t *slot,
                       uint8_t *slot_obs, int32_t *match_of_query, int32_t *best_dist, SearchOpts o = {}, const int32_t *partner = nullptr,
                       const uint8_t *qside = nullptr) {
  if (!m || !f || !q || !slot || !slot_obs) return ORBX_E_ARG;
  const int n = f->n, nq = q->nq;
  if (n < 0 || nq < 0) return ORBX_E_ARG;
  if (n == 0 || nq == 0) {
    for (int i = 0; i < nq; i++) { if (match_of_query) match_of_query[i] = -1; if (best_dist) best_dist[i] = 256; }
    return 0;
  }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t N = (size_t)n, NQ = (size_t)nq;
  // the inputs, then the in/out and out-only arrays (downloaded as one range)
  Staging S{m};
  const StagedFrame hf = stage_frame(S, f);
  const auto qd = S.add(q->descriptors, 32 * NQ);
  const auto qu = S.add(q->u, NQ), qv = S.add(q->v, NQ), qr = S.add(q->radius, NQ), qur = S.add(q->u_r, q->u_r ? NQ : 0);
  const auto minl = S.add(q->min_level, NQ), maxl = S.add(q->max_level, NQ);
  const auto fl = S.add(q->flags, q->flags ? NQ : 0);
  const auto part = S.add(partner, partner ? N : 0); const auto side = S.add(qside, qside ? NQ : 0);
  const auto dslot = S.add(slot, N); const auto dsobs = S.add(slot_obs, N);
  const auto moq = S.out<int32_t>(NQ), bd = S.out<int32_t>(NQ), nmp = S.out<int32_t>(1);
  const auto any = S.out<uint8_t>(o.couple == 2 ? NQ : 0);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  o.partner = S.dev(part); o.qside = S.dev(side); o.qany = S.dev(any);
  const orbm_frame_t df = on_device(S, hf);
  orbm_queries_t dq = *q;
  dq.descriptors = S.dev(qd); dq.u = S.dev(qu); dq.v = S.dev(qv); dq.radius = S.dev(qr); dq.u_r = S.dev(qur);
  dq.min_level = S.dev(minl); dq.max_level = S.dev(maxl); dq.flags = S.dev(fl);
  // The radii are on the host here: the walk-or-scan decision (pair_walks) is taken now and only the chosen kernels are launched.
  o.scan_mode = m->scan_mode;
  if (m->scan_mode == SCAN_AUTO) {
    const float iw = (float)ORBM_GRID_COLS / (f->max_x - f->min_x), ih = (float)ORBM_GRID_ROWS / (f->max_y - f->min_y);
    bool big = n > WALK_MAX_N;
    for (int i = 0; i < nq && !big; i++) {
      if (q->flags && !(q->flags[i] & 1)) continue;
      const float u = q->u[i], v = q->v[i], r = q->radius[i];
      const int cx0 = std::max(0, (int)floorf((u - f->min_x - r) * iw)), cx1 = std::min(63, (int)ceilf((u - f->min_x + r) * iw));
      const int cy0 = std::max(0, (int)floorf((v - f->min_y - r) * ih)), cy1 = std::min(47, (int)ceilf((v - f->min_y + r) * ih));
      if (cx0 < 64 && cx1 >= 0 && cy0 < 48 && cy1 >= 0 && (cx1 - cx0 + 1) * (cy1 - cy0 + 1) > WALK_MAX_CELLS) big = true;
    }
    o.scan_mode = big ? SCAN_DENSE : SCAN_WALK;
  }
  const int rs = search_batch(m, &df, {n, nullptr, 0, n}, &dq, {nq, nullptr, 0, nq}, 1, nnratio, th_dist, use_second, S.dev(dslot), S.dev(dsobs),
                              S.dev(moq), S.dev(bd), S.dev(nmp), s, o);
  if (rs < 0) return rs;
  const int nm = download_slots(m, s, S, dslot, dsobs, nmp, n, slot, slot_obs);
  if (nm < 0) return nm;
  if (match_of_query) memcpy(match_of_query, S.host(moq), sizeof(int32_t) * NQ);
  if (best_dist) memcpy(best_dist, S.host(bd), sizeof(int32_t) * NQ);
  return nm;
}

int orbm_search_by_projection(orbm_t *m, const orbm_frame_t *f, const orbm_queries_t *q, float nnratio, int th_dist,
                              int use_second, int32_t *slot, uint8_t *slot_obs, int32_t *match_of_query, int32_t *best_dist) {
  return search_host(m, f, q, nnratio, th_dist, use_second, slot, slot_obs, match_of_query, best_dist);
}

// ---- reference expressions of the host paths on top of the shared ones (orb_ref_geometry.h) -----------------------------------------
// Decompose Scw (ORBmatcher.cc:498-503, :1668-1673): scw = sqrt(row0 . row0) (Mat::dot accumulates in double); Rcw = sRcw/scw,
// tcw = t/scw, as a row-major 4x4 T = [Rcw | tcw] so that mat3_mul_add applies; and the camera centre of T.
static void decompose_sim3(const float *Scw, float *T, float *Ow) {
  const float scw = norm3(Scw);
  const double inv = 1. / (double)scw;
  for (int i = 0; i < 16; i++) T[i] = 0.f;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) T[4 * i + j] = (float)((double)Scw[4 * i + j] * inv);
  camera_centre(T, Ow);
}

// The viewing-angle gate: true when PO . Pn < 0.5 * dist, the dot product in double (Mat::dot)
static bool views_too_obliquely(const float *PO, const float *Pn, float dist) { return dot3_double(PO, Pn) < 0.5 * (double)dist; }

// MapPoint::PredictScale, MapPoint.cc:570-602, with libm's logf
static int predict_level(float max_dist, float dist, float log_sf, int nlevels) { return level_from_log(logf(max_dist / dist), log_sf, nlevels); }

// Rotation pruning of the projection searches: ids are keypoints of the searched frame, a pruned one gives its map point back.
static int prune_by_rotation(int nq, const int32_t *moq, const float *query_angle, const orbx_keypoint_t *keys, int32_t *slot,
                             uint8_t *slot_obs, int nmatches) {
  RotHist H;
  for (int i = 0; i < nq; i++)
    if (moq[i] >= 0) H.add(query_angle[i] - keys[moq[i]].angle, moq[i]);
  H.for_each_pruned([&](int idx) { slot[idx] = -1; slot_obs[idx] = 0; nmatches--; });
  return nmatches;
}

// The query arrays of a host-side projection loop and their orbm_queries_t view: queries that fail a gate stay at flags = 0.
struct QueryArrays {
  std::vector<float> u, v, rad, ur;   // ur only with_ur (Fuse's mvuRight test)
  std::vector<int32_t> minl, maxl;
  std::vector<uint8_t> flags;
  bool with_ur;
  explicit QueryArrays(int nq, bool with_ur = false)
      : u(nq, 0.f), v(nq, 0.f), rad(nq, 0.f), ur(with_ur ? nq : 0, 0.f), minl(nq, -1), maxl(nq, -1), flags(nq, 0), with_ur(with_ur) {}
  orbm_queries_t view(const uint8_t *desc) const {
    orbm_queries_t q;
    q.nq = (int)u.size(); q.descriptors = desc; q.u = u.data(); q.v = v.data(); q.radius = rad.data();
    q.min_level = minl.data(); q.max_level = maxl.data(); q.u_r = with_ur ? ur.data() : nullptr; q.flags = flags.data();
    return q;
  }
};

// What a fisheye-stereo projection kernel writes besides: the descriptor of every query, its side byte, the window-non-empty
// byte the search keeps per query, the query count per problem.
struct RigScratch { uint8_t *qdesc, *qside, *qany; int32_t *query_n; };

// The query arrays a projection kernel writes, carved out of `buf` (29 B per query, in blocks of 64 queries; with G 34 B more and
// 4 B per problem) - grows on demand, not on the steady-state path.
static int carve_query_scratch(orbm_t *m, DevBuf &buf, hipStream_t s, int npairs, int stride, QueryScratch &Q, RigScratch *G = nullptr) {
  // every problem gets its full stride: the projection kernels write (dead) queries up to the stride, whatever the live counts are
  const size_t nqa = (size_t)npairs * stride, nq4 = (nqa + 63) & ~(size_t)63;
  const size_t need = nq4 * (4 * sizeof(float) + 3 * sizeof(int32_t) + 1 + (G ? 34 : 0)) + (G ? sizeof(int32_t) * (size_t)npairs : 0);
  if (need > buf.bytes) {
    MCHECK(m, hipStreamSynchronize(s));
    MCHECK(m, buf.reserve(need + (need >> 2)));
  }
  float *qf = (float *)buf.p;
  int32_t *qi = (int32_t *)(qf + 4 * nq4);
  Q.u = qf; Q.v = qf + nq4; Q.r = qf + 2 * nq4; Q.ur = qf + 3 * nq4;
  Q.minl = qi; Q.maxl = qi + nq4; Q.moq = qi + 2 * nq4; Q.flags = (uint8_t *)(qi + 3 * nq4);
  if (G) {   // every part starts at a multiple of 64 bytes
    G->qdesc = Q.flags + nq4; G->qside = G->qdesc + 32 * nq4; G->qany = G->qside + nq4;
    G->query_n = (int32_t *)(G->qany + nq4);
  }
  return 0;
}
static orbm_queries_t scratch_view(const QueryScratch &Q, int nq, const uint8_t *desc, bool with_ur) {
  orbm_queries_t q;
  q.nq = nq; q.descriptors = desc; q.u = Q.u; q.v = Q.v; q.radius = Q.r;
  q.min_level = Q.minl; q.max_level = Q.maxl; q.u_r = with_ur ? Q.ur : nullptr; q.flags = Q.flags;
  return q;
}

// The current frame's part of a projection kernel's parameters (V zeroed by the caller)
static void fill_view(ViewParams &V, const orbm_frame_t *cur, const float *sf, int nlevels, int cam_type, const float *cam_params) {
  V.min_x = cur->min_x; V.max_x = cur->max_x; V.min_y = cur->min_y; V.max_y = cur->max_y;
  for (int l = 0; l < nlevels; l++) V.sf[l] = sf[l];
  V.nlevels = nlevels;
  V.cam_type = cam_type;
  for (int k = 0; k < (cam_type == 0 ? 4 : 8); k++) V.cam[k] = cam_params[k];
}

static bool valid_local_map(const orbm_local_map_t *map) {
  return map->eligible && map->Xw && map->normal && map->max_dist && map->min_dist && map->mpdesc && map->Tcw;
}
static bool valid_track(const orbm_track_t *t) {
  return t->in_view && t->proj_x && t->proj_y && t->proj_xr && t->depth && t->view_cos && t->level;
}

// The host forms of the last-frame searches: the windows are th * scale factor of the last keypoint's octave (ORBmatcher.cc:2109),
// known on the host, so the walk-or-scan decision is taken there from the largest one (an upper bound of every query's cell window)
// and only the chosen kernels are launched.  Octaves are in [0, nlevels) where has_mp is set (checked by the callers).
static int host_scan_mode(const orbm_t *m, const orbm_frame_t *cur, const float *sf, int nLast, const uint8_t *has_mp,
                          const orbx_keypoint_t *last_keys, float th) {
  if (m->scan_mode != SCAN_AUTO || cur->n > WALK_MAX_N || !(cur->max_x > cur->min_x) || !(cur->max_y > cur->min_y)) return m->scan_mode;
  float rmax = 0.f;
  for (int i = 0; i < nLast; i++)
    if (has_mp[i]) rmax = std::max(rmax, th * sf[last_keys[i].octave]);
  const float iw = (float)ORBM_GRID_COLS / (cur->max_x - cur->min_x), ih = (float)ORBM_GRID_ROWS / (cur->max_y - cur->min_y);
  const long long cx = std::min<long long>(ORBM_GRID_COLS, (long long)ceilf(2.f * rmax * iw) + 2), cy = std::min<long long>(ORBM_GRID_ROWS, (long long)ceilf(2.f * rmax * ih) + 2);
  return cx * cy <= WALK_MAX_CELLS ? SCAN_WALK : m->scan_mode;
}

// What a fisheye-stereo current frame (Nleft != -1) adds to the last-frame core
struct RigLastExtras { const float *Trl; LiveCount nleft; };   // Nleft has no stride of its own: only its live count

// The device core of both last-frame searches.  Nleft == -1 (rig == NULL): k_lastframe_project, the search, k_rot_prune<0>.
// Nleft != -1: k_lastframe_project_rig (two queries per last-frame keypoint, their descriptors and side bytes), the search with
// couple = 2, k_rot_prune<1> (slot conversion, then the pruning).  Arguments are checked before anything is launched.
static int search_last_frame_batch(orbm_t *m, const orbm_frame_t *cur0, const Ragged &frame, const orbm_last_frame_t *last0, const Ragged &last,
                                   int npairs, const float *sf, int nlevels, int cam_type, const float *cam_params, float mb, float mbf, float th,
                                   int bMono, int checkOri, int32_t *d_slot, uint8_t *d_slot_obs, int32_t *d_moq, int32_t *d_nmatches, hipStream_t s,
                                   int scan_mode, const RigLastExtras *rig = nullptr) {
  if (!m || !cur0 || !last0 || !sf || !cam_params || (rig && !rig->Trl) || npairs < 0 || !d_slot || !d_slot_obs || !d_nmatches) return ORBX_E_ARG;
  if (nlevels < 1 || nlevels > 16 || (cam_type != 0 && cam_type != 1)) return ORBX_E_ARG;
  if (!last0->has_mp || !last0->Xw || !last0->mpdesc || !last0->last_keys || !last0->Tcw || !last0->Tlw) return ORBX_E_ARG;
  if (!last.valid() || (rig && !frame.valid())) return ORBX_E_ARG;   // kept difference: Nleft == -1 never asked for frame stride >= n
  const int rf = check_search_frame(m, cur0, frame);
  if (rf < 0) return rf;
  if (rig && !rig->nleft.dev && (rig->nleft.konst < 0 || rig->nleft.konst > cur0->n)) return ORBX_E_ARG;
  if (rig && (long long)last.stride * 2 > 0x7fffffff / 2) return ORBX_E_ARG;
  if (npairs == 0) return rig ? 0 : ORBX_E_ARG;   // kept difference: an empty batch is refused for Nleft == -1 and is no work for a rig
  MCHECK(m, hipSetDevice(m->device));
  const int qs = rig ? 2 : 1;                     // queries per last-frame keypoint
  LastFrameParams P;
  memset(&P, 0, sizeof(P));
  QueryScratch &Q = P.Q;
  RigScratch G = {};
  const int rq = carve_query_scratch(m, m->d_lfq, s, npairs, qs * last.stride, Q, rig ? &G : nullptr);   // rig: 2 * stride and the RigScratch extras
  if (rq < 0) return rq;
  int32_t *moq = d_moq ? d_moq : Q.moq;
  P.has_mp = last0->has_mp; P.Xw = last0->Xw; P.last_kp = reinterpret_cast<const float *>(last0->last_keys); P.obs = last0->obs;
  P.Tcw = last0->Tcw; P.Tlw = last0->Tlw;
  P.last_stride = last.stride; P.last_n = last.live();
  fill_view(P.V, cur0, sf, nlevels, cam_type, cam_params);
  P.mb = mb; P.mbf = rig ? 0.f : mbf; P.th = th; P.bMono = bMono ? 1 : 0;   // kept difference: a rig has no mbf (no mvuRight test, :2139)
  const dim3 pgrid((last.stride + 255) / 256, npairs);
  SearchOpts o;
  o.scan_mode = scan_mode;
  orbm_frame_t f = *cur0;
  Ragged query = last;
  if (rig) {
    RigProjectParams R;
    memset(&R, 0, sizeof(R));
    for (int i = 0; i < 12; i++) R.Trl[i] = rig->Trl[i];
    R.mpdesc = last0->mpdesc; R.qdesc = G.qdesc; R.qside = G.qside; R.query_n = G.query_n;
    hipLaunchKernelGGL(k_lastframe_project_rig, pgrid, dim3(256), 0, s, P, R);
    f.u_right = nullptr;   // kept difference: Nleft != -1 passes no u_right to the search and asks for no right coordinate (with_ur false)
    o.nleft = rig->nleft;
    o.couple = 2; o.qside = G.qside; o.qany = G.qany;   // :2126: an empty left window drops the right pass
    query = {2 * last.stride, last.d_n ? G.query_n : nullptr, 1, 2 * last0->n};   // the kernel wrote 2 * the live count per problem
  } else {
    hipLaunchKernelGGL(k_lastframe_project, pgrid, dim3(256), 0, s, P);
  }
  const orbm_queries_t q = scratch_view(Q, query.n, rig ? G.qdesc : last0->mpdesc, f.u_right != nullptr);
  const int rc = search_batch(m, &f, frame, &q, query, npairs, 0.f, ORBM_TH_HIGH, 0, d_slot, d_slot_obs, moq, nullptr, d_nmatches, s, o);   // :2148-2162; rig :2128-2162, :2208-2256
  if (rc < 0) return rc;
  // kept difference: k_rot_prune<0> only with checkOri (:2177-2185, :2263-2286); k_rot_prune<1> always (slot conversion), pruning with checkOri
  if (rig || checkOri) {
    RotPruneParams R;
    memset(&R, 0, sizeof(R));
    R.last_kp = reinterpret_cast<const float *>(last0->last_keys);   // :2169-2171
    R.last_stride = last.stride; R.last_n = last.live();
    R.cur_kp = reinterpret_cast<const float *>(cur0->keys_un); R.frame_stride = frame.stride;
    R.moq = moq; R.slot = d_slot; R.slot_obs = d_slot_obs; R.nmatches = d_nmatches; R.prune = checkOri ? 1 : 0;
    if (rig) hipLaunchKernelGGL(k_rot_prune<1>, dim3(npairs), dim3(256), 0, s, R);
    else hipLaunchKernelGGL(k_rot_prune<0>, dim3(npairs), dim3(256), 0, s, R);
  }
  MCHECK(m, hipGetLastError());
  return 0;
}

int orbm_search_by_projection_last_frame_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                                      int frame_n_stride, const orbm_last_frame_t *last0, int last_stride,
                                                      const int32_t *d_last_n, int last_n_stride, int npairs, const float *sf, int nlevels,
                                                      int cam_type, const float *cam_params, float mb, float mbf, float th, int bMono,
                                                      int checkOri, int32_t *d_slot, uint8_t *d_slot_obs, int32_t *d_moq,
                                                      int32_t *d_nmatches, void *stream_) {
  if (!m) return ORBX_E_ARG;
  return search_last_frame_batch(m, cur0, {frame_stride, d_frame_n, frame_n_stride, cur0 ? cur0->n : 0}, last0,
                                 {last_stride, d_last_n, last_n_stride, last0 ? last0->n : 0}, npairs, sf, nlevels, cam_type, cam_params, mb, mbf, th,
                                 bMono, checkOri, d_slot, d_slot_obs, d_moq, d_nmatches, (hipStream_t)stream_, m->scan_mode);
}

// The host form of both last-frame searches (the rig's own checks are its wrapper's): one block up, one down, one synchronisation; npairs = 1.
static int search_last_frame_host(orbm_t *m, const orbm_frame_t *cur, const float *sf, int nlevels, int nLast, const uint8_t *has_mp, const float *Xw,
                                  const uint8_t *mpdesc, const orbx_keypoint_t *last_keys, const uint8_t *obs, const float *Tcw, const float *Tlw,
                                  int cam_type, const float *cam_params, float mb, float mbf, float th, int bMono, int checkOri, int32_t *slot,
                                  uint8_t *slot_obs, const RigLastExtras *rig) {
  if (!m || !cur || !sf || nLast < 0 || !Tcw || !Tlw || !cam_params || !slot || !slot_obs) return ORBX_E_ARG;
  if (nLast > 0 && (!has_mp || !Xw || !mpdesc || !last_keys)) return ORBX_E_ARG;
  if (nlevels < 1 || nlevels > 16) return ORBX_E_ARG;
  const int n = cur->n;
  if (n < 0) return ORBX_E_ARG;
  if (n == 0 || nLast == 0) return 0;
  if (!cur->keys_un || !cur->descriptors) return ORBX_E_ARG;
  for (int i = 0; i < nLast; i++)
    if (has_mp[i] && (last_keys[i].octave < 0 || last_keys[i].octave >= nlevels)) return ORBX_E_ARG;
  orbm_last_frame_t last;
  last.n = nLast; last.has_mp = has_mp; last.Xw = Xw; last.mpdesc = mpdesc; last.last_keys = last_keys; last.obs = obs; last.Tcw = Tcw; last.Tlw = Tlw;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Staging S{m};
  const StagedFrame hf = stage_frame(S, cur, !rig);
  const StagedLast hl = stage_last_frame(S, last);
  const auto dslot = S.add(slot, (size_t)n); const auto dsobs = S.add(slot_obs, (size_t)n);
  const auto nm = S.out<int32_t>(1);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  const orbm_frame_t df = on_device(S, hf);
  const orbm_last_frame_t dl = on_device(S, hl);
  const int scan_mode = host_scan_mode(m, cur, sf, last.n, last.has_mp, last.last_keys, th);   // kept difference: decided on the host here
  const int rs = search_last_frame_batch(m, &df, {n, nullptr, 0, n}, &dl, {last.n, nullptr, 0, last.n}, 1, sf, nlevels, cam_type, cam_params, mb, mbf,
                                         th, bMono, checkOri, S.dev(dslot), S.dev(dsobs), nullptr, S.dev(nm), s, scan_mode, rig);
  if (rs < 0) return rs;
  return download_slots(m, s, S, dslot, dsobs, nm, n, slot, slot_obs);
}

int orbm_search_by_projection_last_frame(orbm_t *m, const orbm_frame_t *cur, const float *sf, int nlevels, int nLast,
                                         const uint8_t *has_mp, const float *Xw, const uint8_t *mpdesc,
                                         const orbx_keypoint_t *last_keys, const uint8_t *obs, const float *Tcw,
                                         const float *Tlw, int cam_type, const float *cam_params, float mb, float mbf,
                                         float th, int bMono, int checkOri, int32_t *slot, uint8_t *slot_obs) {
  return search_last_frame_host(m, cur, sf, nlevels, nLast, has_mp, Xw, mpdesc, last_keys, obs, Tcw, Tlw, cam_type, cam_params, mb, mbf, th, bMono,
                                checkOri, slot, slot_obs, nullptr);
}

static bool valid_track_rig(const orbm_track_rig_t *t) {
  return t->in_view && t->in_view_r && t->proj_x && t->proj_y && t->depth && t->view_cos && t->proj_xr && t->proj_yr && t->depth_r &&
         t->view_cos_r && t->level && t->level_r;
}

// What Nleft != -1 adds to the local-map core: right camera, stereo matches (device [npairs][frame_stride] or NULL), Nleft, serial
// (see orbm_search_local_points_fisheye_batch_device) and the track fields of both cameras, which stand in for the core's orbm_track_t.
struct RigLocalExtras {
  const float *Trl, *tlr; int cam_type2; const float *cam_params2;
  const int32_t *d_l2r, *d_r2l; LiveCount nleft; int serial;
  const orbm_track_rig_t *track;
};

// Tracking::SearchLocalPoints on the device.  Nleft == -1 (rig == NULL): k_local_map_project (isInFrustum + M2's query preparation), then
// the M2 search (use_second, nnratio, TH_HIGH), claims in local-map order.  Nleft != -1: k_local_map_project_rig (both frustum tests, two
// queries per point, the partner table), the search with couple = 1 (:127), k_rig_slot_convert.  Checks come before any launch.
static int search_local_batch(orbm_t *m, const orbm_frame_t *cur0, const Ragged &frame, const orbm_local_map_t *map0, const Ragged &map, int npairs,
                              const float *sf, int nlevels, float log_sf, int cam_type, const float *cam_params, float mbf, float view_cos_limit,
                              float th, int bFarPoints, float th_far, float nnratio, int32_t *d_slot, uint8_t *d_slot_obs, int32_t *d_moq,
                              const orbm_track_t *track0, int32_t *d_nmatches, hipStream_t s, bool search, const RigLocalExtras *rig = nullptr) {
  if (!m || !cur0 || !map0 || !sf || !cam_params || npairs < 0 || !d_slot || !d_slot_obs || !d_nmatches) return ORBX_E_ARG;
  if (rig ? !rig->track || !rig->cam_params2 || !rig->Trl || !rig->tlr || (rig->cam_type2 != 0 && rig->cam_type2 != 1) : !track0) return ORBX_E_ARG;
  if (nlevels < 1 || nlevels > 16 || (cam_type != 0 && cam_type != 1)) return ORBX_E_ARG;
  if (!valid_local_map(map0) || !(rig ? valid_track_rig(rig->track) : valid_track(track0))) return ORBX_E_ARG;
  if (!map.valid() || (search && !frame.valid())) return ORBX_E_ARG;
  const int rf = search ? check_search_frame(m, cur0, frame) : 0;   // no search (host forms, a frame without keypoints): the frame is not read
  if (rf < 0) return rf;
  if (rig && search && !rig->nleft.dev && (rig->nleft.konst < 0 || rig->nleft.konst > cur0->n)) return ORBX_E_ARG;
  if (rig && (long long)map.stride * 2 > 0x7fffffff / 2) return ORBX_E_ARG;
  if (npairs == 0) return rig ? 0 : ORBX_E_ARG;   // kept difference: an empty batch is refused for Nleft == -1 and is no work for a rig
  MCHECK(m, hipSetDevice(m->device));
  const int qs = rig ? 2 : 1;                     // queries per local map point
  LocalMapParams P;
  memset(&P, 0, sizeof(P));
  QueryScratch &Q = P.Q;
  RigScratch S = {};
  const int rq = carve_query_scratch(m, m->d_lmq, s, npairs, qs * map.stride, Q, rig ? &S : nullptr);   // rig: 2 * stride and the RigScratch extras
  if (rq < 0) return rq;
  const bool partners = rig && search && (rig->d_l2r || rig->d_r2l);
  const size_t pbytes = sizeof(int32_t) * (size_t)npairs * (size_t)frame.stride;
  if (partners && pbytes > m->d_partner.bytes) {
    MCHECK(m, hipStreamSynchronize(s));
    MCHECK(m, m->d_partner.reserve(pbytes + (pbytes >> 2)));
  }
  int32_t *moq = d_moq ? d_moq : Q.moq;
  P.eligible = map0->eligible; P.Xw = map0->Xw; P.normal = map0->normal; P.max_dist = map0->max_dist; P.min_dist = map0->min_dist;
  P.obs = map0->obs; P.Tcw = map0->Tcw;
  P.map_stride = map.stride; P.map_n = map.live();
  fill_view(P.V, cur0, sf, nlevels, cam_type, cam_params);
  P.log_sf = log_sf;
  P.mbf = rig ? 0.f : mbf; P.view_cos_limit = view_cos_limit; P.th = th; P.bFarPoints = bFarPoints ? 1 : 0; P.th_far = th_far;
  const orbm_track_rig_t *r = rig ? rig->track : nullptr;
  const orbm_track_t t = r ? orbm_track_t{r->in_view, r->proj_x, r->proj_y, r->proj_xr, r->depth, r->view_cos, r->level} : *track0;
  P.in_view = t.in_view; P.proj_x = t.proj_x; P.proj_y = t.proj_y; P.proj_xr = t.proj_xr; P.depth = t.depth; P.view_cos = t.view_cos; P.level = t.level;
  const dim3 pgrid((map.stride + 255) / 256, npairs);
  SearchOpts o;
  o.scan_mode = m->scan_mode;   // SCAN_AUTO: the windows exist only on the device, so the vote is taken there
  orbm_frame_t f = *cur0;
  Ragged query = map;
  if (rig) {
    RigLocalParams G;
    memset(&G, 0, sizeof(G));
    for (int i = 0; i < 12; i++) G.Trl[i] = rig->Trl[i];
    for (int i = 0; i < 3; i++) G.tlr[i] = rig->tlr[i];
    G.cam_type2 = rig->cam_type2;
    for (int k = 0; k < (rig->cam_type2 == 0 ? 4 : 8); k++) G.cam2[k] = rig->cam_params2[k];
    G.mpdesc = map0->mpdesc;
    G.in_view_r = r->in_view_r; G.proj_yr = r->proj_yr; G.depth_r = r->depth_r; G.view_cos_r = r->view_cos_r; G.level_r = r->level_r;
    G.qdesc = S.qdesc; G.qside = S.qside; G.query_n = S.query_n;
    G.l2r = rig->d_l2r; G.r2l = rig->d_r2l; G.partner = partners ? (int32_t *)m->d_partner.p : nullptr;
    G.frame_stride = frame.stride; G.frame_n = frame.live(); G.nleft = rig->nleft;
    hipLaunchKernelGGL(k_local_map_project_rig, pgrid, dim3(256), 0, s, P, G);
    f.u_right = nullptr;   // kept difference: Nleft != -1 has no mvuRight test (ORBmatcher.cc:93)
    o.nleft = rig->nleft;
    o.couple = 1; o.qside = S.qside;   // ORBmatcher.cc:127
    o.partner = G.partner; o.serial = partners ? rig->serial : 0;
    query = {2 * map.stride, map.d_n ? S.query_n : nullptr, 1, 2 * map0->n};   // the kernel wrote 2 * the live count per problem
  } else {
    hipLaunchKernelGGL(k_local_map_project, pgrid, dim3(256), 0, s, P);
  }
  if (search) {
    const orbm_queries_t q = scratch_view(Q, query.n, rig ? S.qdesc : map0->mpdesc, f.u_right != nullptr);
    const int rc = search_batch(m, &f, frame, &q, query, npairs, nnratio, ORBM_TH_HIGH, 1, d_slot, d_slot_obs, moq, nullptr, d_nmatches, s, o);   // ORBmatcher.cc:75-139; rig :75-141, :153-209
    if (rc < 0) return rc;
    if (rig) {   // the search left query ids in the slots: back to local-map indices
      RigSlotParams C;
      memset(&C, 0, sizeof(C));
      C.moq = moq; C.map_stride = map.stride; C.map_n = map.live();
      C.partner = o.partner; C.slot = d_slot; C.frame_stride = frame.stride;
      hipLaunchKernelGGL(k_rig_slot_convert, dim3(npairs), dim3(256), 0, s, C);
    }
  }
  MCHECK(m, hipGetLastError());
  return 0;
}

int orbm_search_local_points_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n, int frame_n_stride,
                                          const orbm_local_map_t *map0, int map_stride, const int32_t *d_map_n, int map_n_stride, int npairs,
                                          const float *sf, int nlevels, float log_sf, int cam_type, const float *cam_params, float mbf,
                                          float view_cos_limit, float th, int bFarPoints, float th_far, float nnratio, int32_t *d_slot,
                                          uint8_t *d_slot_obs, int32_t *d_moq, const orbm_track_t *track0, int32_t *d_nmatches, void *stream_) {
  if (!m) return ORBX_E_ARG;
  return search_local_batch(m, cur0, {frame_stride, d_frame_n, frame_n_stride, cur0 ? cur0->n : 0}, map0,
                            {map_stride, d_map_n, map_n_stride, map0 ? map0->n : 0}, npairs, sf, nlevels, log_sf, cam_type, cam_params, mbf,
                            view_cos_limit, th, bFarPoints, th_far, nnratio, d_slot, d_slot_obs, d_moq, track0, d_nmatches, (hipStream_t)stream_, true);
}

int orbm_search_local_points(orbm_t *m, const orbm_frame_t *cur, const float *sf, int nlevels, float log_sf, const orbm_local_map_t *map,
                             int cam_type, const float *cam_params, float mbf, float view_cos_limit, float th, int bFarPoints, float th_far,
                             float nnratio, int32_t *slot, uint8_t *slot_obs, int32_t *match_of_point, const orbm_track_t *track) {
  if (!m || !cur || !map || !track || !sf || !cam_params || !slot || !slot_obs) return ORBX_E_ARG;
  if (nlevels < 1 || nlevels > 16 || (cam_type != 0 && cam_type != 1)) return ORBX_E_ARG;
  if (!valid_local_map(map) || !valid_track(track)) return ORBX_E_ARG;
  const int n = cur->n, nmp = map->n;
  if (n < 0 || nmp < 0) return ORBX_E_ARG;
  if (n > ORBM_MAX_KEYPOINTS) { m->err = "more than 15360 keypoints per frame not supported by the search kernels"; return ORBX_E_ARG; }
  if (n > 0 && (!cur->keys_un || !cur->descriptors || !(cur->max_x > cur->min_x) || !(cur->max_y > cur->min_y))) return ORBX_E_ARG;
  if (nmp == 0) return 0;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  // one staged block up, one block down, one synchronisation; a frame without keypoints still gets its track fields
  const size_t N = (size_t)n, NP = (size_t)nmp;
  Staging S{m};
  const StagedFrame hf = stage_frame(S, cur);
  const StagedMap hm = stage_local_map(S, map);
  const auto hslot = S.add(slot, N); const auto hsobs = S.add(slot_obs, N);
  const auto hmoq = S.out<int32_t>(NP);
  const auto hinv = S.out<uint8_t>(NP);
  const auto hpx = S.out<float>(NP), hpy = S.out<float>(NP), hpxr = S.out<float>(NP), hdep = S.out<float>(NP), hvc = S.out<float>(NP);
  const auto hlvl = S.out<int32_t>(NP), hnm = S.out<int32_t>(1);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  const orbm_frame_t df = on_device(S, hf);
  const orbm_local_map_t dm = on_device(S, hm);
  const orbm_track_t dt = {S.dev(hinv), S.dev(hpx), S.dev(hpy), S.dev(hpxr), S.dev(hdep), S.dev(hvc), S.dev(hlvl)};
  int32_t *dslot = n > 0 ? S.dev(hslot) : S.dev(hmoq);   // n == 0: no search, any non-null pointer
  uint8_t *dsobs = n > 0 ? S.dev(hsobs) : S.dev(hinv);
  const int rs = search_local_batch(m, &df, {n, nullptr, 0, n}, &dm, {nmp, nullptr, 0, nmp}, 1, sf, nlevels, log_sf, cam_type, cam_params, mbf,
                                    view_cos_limit, th, bFarPoints, th_far, nnratio, dslot, dsobs, S.dev(hmoq), &dt, S.dev(hnm), s, n > 0);
  if (rs < 0) return rs;
  const int nm = download_slots(m, s, S, hslot, hsobs, hnm, n, slot, slot_obs);
  if (nm < 0) return nm;
  const int32_t *moq = S.host(hmoq), *lvl = S.host(hlvl);
  const uint8_t *inv = S.host(hinv);
  const float *px = S.host(hpx), *py = S.host(hpy), *pxr = S.host(hpxr), *dep = S.host(hdep), *vc = S.host(hvc);
  // only what isInFrustum writes: in_view always, the projection of eligible points, the rest where in view
  for (int i = 0; i < nmp; i++) {
    if (match_of_point) match_of_point[i] = n > 0 ? moq[i] : -1;
    track->in_view[i] = inv[i];
    if (!map->eligible[i]) continue;
    track->proj_x[i] = px[i]; track->proj_y[i] = py[i];
    if (!inv[i]) continue;
    track->proj_xr[i] = pxr[i]; track->depth[i] = dep[i]; track->view_cos[i] = vc[i]; track->level[i] = lvl[i];
  }
  return nm;
}

// ---- fisheye-stereo frames (Nleft != -1) -------------------------------------------------------------------------
// One problem over the concatenated keypoints [left ; right] with two queries per map point (even = left image,
// odd = right image): the device core handles the image restriction, the stereo-partner writes and the pair coupling.
static int build_partner(int n, int n_left, const int32_t *l2r, const int32_t *r2l, std::vector<int32_t> &partner) {
  partner.assign((size_t)n, -1);
  bool any = false;
  for (int i = 0; i < n_left; i++)
    if (l2r && l2r[i] >= 0) { if (n_left + l2r[i] >= n) return ORBX_E_ARG; partner[i] = n_left + l2r[i]; any = true; }
  for (int j = 0; j < n - n_left; j++)
    if (r2l && r2l[j] >= 0) { if (r2l[j] >= n_left) return ORBX_E_ARG; partner[n_left + j] = r2l[j]; any = true; }
  return any ? 1 : 0;
}

int orbm_search_by_projection_fisheye(orbm_t *m, const orbm_frame_t *f, int n_left, const int32_t *left_to_right,
                                      const int32_t *right_to_left, const orbm_queries_t *q, float nnratio, int th_dist,
                                      int32_t *slot, uint8_t *slot_obs, int32_t *match_of_query, int32_t *best_dist) {
  if (!m || !f || !q || n_left < 0 || n_left > f->n || (q->nq & 1)) return ORBX_E_ARG;
  std::vector<int32_t> partner;
  const int anyp = build_partner(f->n, n_left, left_to_right, right_to_left, partner);
  if (anyp < 0) return anyp;
  std::vector<uint8_t> side((size_t)q->nq);
  bool release = false;  // a taking query without observations can release a claim through a partner write
  for (int i = 0; i < q->nq; i++) {
    side[i] = (uint8_t)(i & 1);
    const uint8_t fl = q->flags ? q->flags[i] : (uint8_t)3;
    if ((fl & 1) && !(fl & 2)) release = true;
  }
  SearchOpts o;
  o.nleft.konst = n_left; o.couple = 1; o.serial = (anyp && release) ? 1 : 0;
  return search_host(m, f, q, nnratio, th_dist, 1, slot, slot_obs, match_of_query, best_dist, o, anyp ? partner.data() : nullptr, side.data());
}

int orbm_search_by_projection_last_frame_fisheye_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                                              int frame_n_stride, const int32_t *d_n_left, int n_left_stride, int n_left,
                                                              const orbm_last_frame_t *last0, int last_stride, const int32_t *d_last_n,
                                                              int last_n_stride, int npairs, const float *sf, int nlevels, const float *Trl,
                                                              int cam_type, const float *cam_params, float mb, float th, int bMono, int checkOri,
                                                              int32_t *d_slot, uint8_t *d_slot_obs, int32_t *d_moq, int32_t *d_nmatches,
                                                              void *stream_) {
  if (!m) return ORBX_E_ARG;
  if (frame_stride > ORBM_FISHEYE_MAX_KEYPOINTS) { m->err = "more than 12960 keypoints (left + right) per fisheye-stereo frame not supported by the resident search"; return ORBX_E_ARG; }
  const RigLastExtras rig = {Trl, {d_n_left, n_left_stride, n_left}};
  return search_last_frame_batch(m, cur0, {frame_stride, d_frame_n, frame_n_stride, cur0 ? cur0->n : 0}, last0,
                                 {last_stride, d_last_n, last_n_stride, last0 ? last0->n : 0}, npairs, sf, nlevels, cam_type, cam_params, mb, 0.f, th,
                                 bMono, checkOri, d_slot, d_slot_obs, d_moq, d_nmatches, (hipStream_t)stream_, m->scan_mode, &rig);
}

int orbm_rig_concat_batch_device(int nframes, const orbx_keypoint_t *d_keysL, const uint8_t *d_descL, const int32_t *d_countsL,
                                 const orbx_keypoint_t *d_keysR, const uint8_t *d_descR, const int32_t *d_countsR, int cap,
                                 orbx_keypoint_t *d_keys, uint8_t *d_desc, int32_t *d_n, void *stream_) {
  if (!d_keysL || !d_descL || !d_countsL || !d_keysR || !d_descR || !d_countsR || !d_keys || !d_desc || !d_n) return ORBX_E_ARG;
  if (nframes < 0 || nframes > 65535 || cap <= 0 || cap > ORBM_FISHEYE_MAX_KEYPOINTS / 2) return ORBX_E_ARG;
  if (nframes == 0) return 0;
  RigConcatParams R;
  R.keysL = reinterpret_cast<const uint32_t *>(d_keysL); R.keysR = reinterpret_cast<const uint32_t *>(d_keysR);
  R.descL = reinterpret_cast<const uint4 *>(d_descL); R.descR = reinterpret_cast<const uint4 *>(d_descR);
  R.countsL = d_countsL; R.countsR = d_countsR; R.cap = cap;
  R.keys = reinterpret_cast<uint32_t *>(d_keys); R.desc = reinterpret_cast<uint4 *>(d_desc); R.n = d_n;
  hipLaunchKernelGGL(k_rig_concat, dim3((18 * cap + 255) / 256, nframes), dim3(256), 0, (hipStream_t)stream_, R);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

// ---- Frame::ComputeStereoFishEyeMatches (Frame.cc:1228-1268) -------------------------------------------------------------------
int orbm_unproject(const float *cam_params, int n, const float *xy, float *rays) {
  if (!cam_params || n < 0 || (n > 0 && (!xy || !rays))) return ORBX_E_ARG;
  for (int i = 0; i < n; i++) kb8_unproject(cam_params, xy[2 * i], xy[2 * i + 1], rays + 3 * (size_t)i);
  return 0;
}

int orbm_fisheye_ratio_test(int d0, int d1) { return fisheye_ratio_test(d0, d1) ? 1 : 0; }

static bool fill_triangulate(TriangulateParams &P, int n, const float *kp1, const float *kp2, const float *sigma1, const float *sigma2,
                             const float *Tlr, const float *cam_params, const float *cam_params2, float *depth, float *p3D) {
  if (n < 0 || !Tlr || !cam_params || !cam_params2 || (n > 0 && (!kp1 || !kp2 || !sigma1 || !sigma2 || !depth || !p3D))) return false;
  P.kp1 = kp1; P.kp2 = kp2; P.sigma1 = sigma1; P.sigma2 = sigma2; P.depth = depth; P.p3d = p3D; P.n = n;
  for (int i = 0; i < 12; i++) P.Tlr[i] = Tlr[i];
  rig_Tcw2(P.Tlr, P.Tcw2);
  for (int k = 0; k < 8; k++) { P.cam1[k] = cam_params[k]; P.cam2[k] = cam_params2[k]; }
  return true;
}

int orbm_fisheye_triangulate(int n, const float *kp1, const float *kp2, const float *sigma1, const float *sigma2, const float *Tlr,
                             const float *cam_params, const float *cam_params2, float *depth, float *p3D) {
  TriangulateParams P;
  if (!fill_triangulate(P, n, kp1, kp2, sigma1, sigma2, Tlr, cam_params, cam_params2, depth, p3D)) return ORBX_E_ARG;
  for (int i = 0; i < n; i++)
    depth[i] = kb8_triangulate_matches(P.cam1, P.cam2, kp1[2 * i], kp1[2 * i + 1], kp2[2 * i], kp2[2 * i + 1], P.Tlr, P.Tcw2, sigma1[i], sigma2[i],
                                       p3D + 3 * (size_t)i);
  return 0;
}

int orbm_fisheye_triangulate_device(int n, const float *d_kp1, const float *d_kp2, const float *d_sigma1, const float *d_sigma2, const float *Tlr,
                                    const float *cam_params, const float *cam_params2, float *d_depth, float *d_p3D, void *stream) {
  TriangulateParams P;
  if (!fill_triangulate(P, n, d_kp1, d_kp2, d_sigma1, d_sigma2, Tlr, cam_params, cam_params2, d_depth, d_p3D)) return ORBX_E_ARG;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_fisheye_triangulate, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbm_stereo_fisheye_matches_batch_device(orbm_t *m, int nframes, const orbx_keypoint_t *d_keysL, const uint8_t *d_descL, const int32_t *d_countsL,
                                             const orbx_keypoint_t *d_keysR, const uint8_t *d_descR, const int32_t *d_countsR, int cap,
                                             const float *level_sigma2, int nlevels, const float *Tlr, const float *cam_params,
                                             const float *cam_params2, int out_stride, int32_t *d_left_to_right, int32_t *d_right_to_left,
                                             float *d_depth, float *d_p3d, int32_t *d_nmatches, void *stream_) {
  if (!m || !d_keysL || !d_descL || !d_countsL || !d_keysR || !d_descR || !d_countsR || !level_sigma2 || !Tlr || !cam_params || !cam_params2 ||
      !d_left_to_right || !d_right_to_left || !d_depth || !d_p3d)
    return ORBX_E_ARG;
  if (nframes < 0 || nframes > 65535 || cap <= 0 || cap > ORBM_FISHEYE_MAX_KEYPOINTS / 2 || out_stride < cap || nlevels < 1 || nlevels > 16) return ORBX_E_ARG;
  if (nframes == 0) return 0;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream_;
  const size_t kbytes = sizeof(uint32_t) * 2 * (size_t)nframes * (size_t)cap;
  if (kbytes > m->d_knn.bytes) {   // growth only (as d_partner)
    MCHECK(m, hipStreamSynchronize(s));
    MCHECK(m, m->d_knn.reserve(kbytes + (kbytes >> 2)));
  }
  RigStereoParams P;
  memset(&P, 0, sizeof(P));
  P.keysL = reinterpret_cast<const uint32_t *>(d_keysL); P.keysR = reinterpret_cast<const uint32_t *>(d_keysR);
  P.descL = reinterpret_cast<const uint32_t *>(d_descL); P.descR = reinterpret_cast<const uint32_t *>(d_descR);
  P.countsL = d_countsL; P.countsR = d_countsR; P.cap = cap; P.out_stride = out_stride; P.nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) P.sigma2[l] = level_sigma2[l];
  for (int i = 0; i < 12; i++) P.Tlr[i] = Tlr[i];
  rig_Tcw2(P.Tlr, P.Tcw2);
  for (int k = 0; k < 8; k++) { P.cam1[k] = cam_params[k]; P.cam2[k] = cam_params2[k]; }
  P.l2r = d_left_to_right; P.r2l = d_right_to_left; P.depth = d_depth; P.p3d = d_p3d; P.nmatches = d_nmatches;
  P.knn = (uint32_t *)m->d_knn.p;
  hipLaunchKernelGGL(k_rig_stereo_knn2, dim3((cap + MF_NT - 1) / MF_NT, nframes), dim3(MF_NT), 0, s, P);
  hipLaunchKernelGGL(k_rig_stereo_triangulate, dim3((cap + 255) / 256, nframes), dim3(256), 0, s, P);
  MCHECK(m, hipGetLastError());
  return 0;
}

int orbm_stereo_fisheye_matches(orbm_t *m, const orbx_keypoint_t *keysL, const uint8_t *descL, int nL, int monoL, const orbx_keypoint_t *keysR,
                                const uint8_t *descR, int nR, int monoR, const float *level_sigma2, int nlevels, const float *Tlr,
                                const float *cam_params, const float *cam_params2, int32_t *left_to_right, int32_t *right_to_left, float *depth,
                                float *p3d, int32_t *nmatches) {
  if (!m || !level_sigma2 || !Tlr || !cam_params || !cam_params2 || nL < 0 || nR < 0 || monoL < 0 || monoL > nL || monoR < 0 || monoR > nR) return ORBX_E_ARG;
  if ((nL > 0 && (!keysL || !descL || !left_to_right || !depth || !p3d)) || (nR > 0 && (!keysR || !descR || !right_to_left))) return ORBX_E_ARG;
  if (nlevels < 1 || nlevels > 16) return ORBX_E_ARG;
  const int cap = std::max(std::max(nL, nR), 1);
  if (cap > ORBM_FISHEYE_MAX_KEYPOINTS / 2) { m->err = "more than 12960 keypoints (left + right) per fisheye-stereo frame not supported"; return ORBX_E_ARG; }
  // mvLevelSigma2[octave] (:1257) of a lapping keypoint outside the pyramid: refused here, a non-match in the batch form
  for (int i = monoL; i < nL; i++) if (keysL[i].octave < 0 || keysL[i].octave >= nlevels) return ORBX_E_ARG;
  for (int j = monoR; j < nR; j++) if (keysR[j].octave < 0 || keysR[j].octave >= nlevels) return ORBX_E_ARG;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  // one staged block up (p3d is in/out: unmatched entries keep the caller's values), one block down, one synchronisation
  const int32_t counts[4] = {nL, monoL, nR, monoR};
  const size_t NL = (size_t)nL, NR = (size_t)nR, CAP = (size_t)cap;
  Staging S{m};
  const auto hkl = S.add(keysL, NL); const auto hdl = S.add(descL, 32 * NL);
  const auto hkr = S.add(keysR, NR); const auto hdr = S.add(descR, 32 * NR);
  const auto hcnt = S.add(counts, 4);
  const auto hp3 = S.add((const float *)p3d, 3 * NL);
  const auto hl2r = S.out<int32_t>(CAP), hr2l = S.out<int32_t>(CAP);
  const auto hdep = S.out<float>(CAP); const auto hnm = S.out<int32_t>(2);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  const int32_t *cnt = S.dev(hcnt);
  // an empty side has no device part: any non-null address stands in, its count keeps every access away
  const orbx_keypoint_t *kl = nL ? S.dev(hkl) : (const orbx_keypoint_t *)cnt, *kr = nR ? S.dev(hkr) : (const orbx_keypoint_t *)cnt;
  const uint8_t *dl = nL ? S.dev(hdl) : (const uint8_t *)cnt, *dr = nR ? S.dev(hdr) : (const uint8_t *)cnt;
  float *dp3 = nL ? S.dev(hp3) : S.dev(hdep);
  const int rs = orbm_stereo_fisheye_matches_batch_device(m, 1, kl, dl, cnt, kr, dr, cnt + 2, cap, level_sigma2, nlevels, Tlr, cam_params, cam_params2, cap,
                                                          S.dev(hl2r), S.dev(hr2l), S.dev(hdep), dp3, S.dev(hnm), s);
  if (rs < 0) return rs;
  MCHECK(m, S.download(s, hp3, hnm));
  MCHECK(m, hipStreamSynchronize(s));
  if (nL > 0) {
    memcpy(p3d, S.host(hp3), 3 * sizeof(float) * NL);
    memcpy(left_to_right, S.host(hl2r), sizeof(int32_t) * NL);
    memcpy(depth, S.host(hdep), sizeof(float) * NL);
  }
  if (nR > 0) memcpy(right_to_left, S.host(hr2l), sizeof(int32_t) * NR);
  if (nmatches) memcpy(nmatches, S.host(hnm), 2 * sizeof(int32_t));
  return 0;
}

int orbm_search_by_projection_last_frame_fisheye(orbm_t *m, const orbm_frame_t *cur, int n_left, const float *sf, int nlevels,
                                                 int nLast, const uint8_t *has_mp, const float *Xw, const uint8_t *mpdesc,
                                                 const orbx_keypoint_t *last_keys, const uint8_t *obs, const float *Tcw,
                                                 const float *Tlw, const float *Trl, int cam_type, const float *cam_params,
                                                 float mb, float th, int bMono, int checkOri, int32_t *slot, uint8_t *slot_obs) {
  if (!cur || !Trl || n_left < 0 || n_left > cur->n) return ORBX_E_ARG;
  const RigLastExtras rig = {Trl, {nullptr, 0, n_left}};
  return search_last_frame_host(m, cur, sf, nlevels, nLast, has_mp, Xw, mpdesc, last_keys, obs, Tcw, Tlw, cam_type, cam_params, mb, 0.f, th, bMono,
                                checkOri, slot, slot_obs, &rig);
}

// ---- Tracking::SearchLocalPoints for a fisheye-stereo frame (Frame.cc:650-660, :1270-1343; ORBmatcher.cc:44-214) ------------------
int orbm_search_local_points_fisheye_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                                  int frame_n_stride, const int32_t *d_n_left, int n_left_stride, int n_left,
                                                  const int32_t *d_left_to_right, const int32_t *d_right_to_left, const orbm_local_map_t *map0,
                                                  int map_stride, const int32_t *d_map_n, int map_n_stride, int npairs, const float *sf,
                                                  int nlevels, float log_sf, const float *Trl, const float *tlr, int cam_type,
                                                  const float *cam_params, int cam_type2, const float *cam_params2, float view_cos_limit, float th,
                                                  int bFarPoints, float th_far, float nnratio, int32_t *d_slot, uint8_t *d_slot_obs,
                                                  int32_t *d_moq, const orbm_track_rig_t *track0, int32_t *d_nmatches, void *stream_) {
  if (!m) return ORBX_E_ARG;
  if (frame_stride > ORBM_FISHEYE_MAX_KEYPOINTS) { m->err = "more than 12960 keypoints (left + right) per fisheye-stereo frame not supported by the resident search"; return ORBX_E_ARG; }
  // obs lives on the device: whether a taking query without observations exists is not known here, so the search is serial whenever
  // one can exist and a partner table is passed (exact in either mode)
  const int serial = map0 && map0->obs ? 1 : 0;
  const RigLocalExtras rig = {Trl, tlr, cam_type2, cam_params2, d_left_to_right, d_right_to_left, {d_n_left, n_left_stride, n_left}, serial, track0};
  return search_local_batch(m, cur0, {frame_stride, d_frame_n, frame_n_stride, cur0 ? cur0->n : 0}, map0,
                            {map_stride, d_map_n, map_n_stride, map0 ? map0->n : 0}, npairs, sf, nlevels, log_sf, cam_type, cam_params, 0.f,
                            view_cos_limit, th, bFarPoints, th_far, nnratio, d_slot, d_slot_obs, d_moq, nullptr, d_nmatches, (hipStream_t)stream_, true,
                            &rig);
}

int orbm_search_local_points_fisheye(orbm_t *m, const orbm_frame_t *cur, int n_left, const int32_t *left_to_right, const int32_t *right_to_left,
                                     const float *sf, int nlevels, float log_sf, const orbm_local_map_t *map, const float *Trl, const float *tlr,
                                     int cam_type, const float *cam_params, int cam_type2, const float *cam_params2, float view_cos_limit, float th,
                                     int bFarPoints, float th_far, float nnratio, int32_t *slot, uint8_t *slot_obs, int32_t *match_of_point,
                                     const orbm_track_rig_t *track) {
  if (!m || !cur || !map || !track || !sf || !cam_params || !cam_params2 || !Trl || !tlr || !slot || !slot_obs) return ORBX_E_ARG;
  if (nlevels < 1 || nlevels > 16 || (cam_type != 0 && cam_type != 1) || (cam_type2 != 0 && cam_type2 != 1)) return ORBX_E_ARG;
  if (!valid_local_map(map) || !valid_track_rig(track)) return ORBX_E_ARG;
  const int n = cur->n, nmp = map->n;
  if (n < 0 || nmp < 0 || n_left < 0 || n_left > n) return ORBX_E_ARG;
  if (n > ORBM_FISHEYE_MAX_KEYPOINTS) { m->err = "more than 12960 keypoints (left + right) per fisheye-stereo frame not supported"; return ORBX_E_ARG; }
  if (n > 0 && (!cur->keys_un || !cur->descriptors || !(cur->max_x > cur->min_x) || !(cur->max_y > cur->min_y))) return ORBX_E_ARG;
  bool anyp = false;   // a bad partner index is refused, as orbm_search_by_projection_fisheye does (build_partner)
  for (int i = 0; left_to_right && i < n_left; i++)
    if (left_to_right[i] >= 0) { if (left_to_right[i] >= n - n_left) return ORBX_E_ARG; anyp = true; }
  for (int j = 0; right_to_left && j < n - n_left; j++)
    if (right_to_left[j] >= 0) { if (right_to_left[j] >= n_left) return ORBX_E_ARG; anyp = true; }
  if (nmp == 0) return 0;
  // a partner write releases a claim only when its query has no observations (k_match_resolve): serial mode only then
  bool release = false;
  for (int i = 0; map->obs && i < nmp && !release; i++) release = map->eligible[i] && !map->obs[i];
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  // one staged block up (depth is in/out: it goes up with the slots), one block down, one synchronisation; a frame without keypoints
  // still gets its track fields
  const size_t N = (size_t)n, NP = (size_t)nmp;
  const int32_t *l2r = anyp ? left_to_right : nullptr, *r2l = anyp ? right_to_left : nullptr;
  Staging S{m};
  const StagedFrame hf = stage_frame(S, cur, false);
  const auto hl2r = S.add(l2r, l2r ? (size_t)n_left : 0), hr2l = S.add(r2l, r2l ? (size_t)(n - n_left) : 0);
  const StagedMap hm = stage_local_map(S, map);
  const auto hslot = S.add(slot, N); const auto hsobs = S.add(slot_obs, N);
  const auto hdep = S.add((const float *)track->depth, NP);
  const auto hmoq = S.out<int32_t>(2 * NP);
  const auto hinv = S.out<uint8_t>(NP), hinvr = S.out<uint8_t>(NP);
  const auto hpx = S.out<float>(NP), hpy = S.out<float>(NP), hvc = S.out<float>(NP), hpxr = S.out<float>(NP), hpyr = S.out<float>(NP);
  const auto hdepr = S.out<float>(NP), hvcr = S.out<float>(NP);
  const auto hlvl = S.out<int32_t>(NP), hlvlr = S.out<int32_t>(NP), hnm = S.out<int32_t>(1);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  const orbm_frame_t df = on_device(S, hf);
  const orbm_local_map_t dm = on_device(S, hm);
  orbm_track_rig_t dt;
  dt.in_view = S.dev(hinv); dt.in_view_r = S.dev(hinvr); dt.proj_x = S.dev(hpx); dt.proj_y = S.dev(hpy);
  dt.depth = S.dev(hdep); dt.view_cos = S.dev(hvc); dt.proj_xr = S.dev(hpxr); dt.proj_yr = S.dev(hpyr);
  dt.depth_r = S.dev(hdepr); dt.view_cos_r = S.dev(hvcr); dt.level = S.dev(hlvl); dt.level_r = S.dev(hlvlr);
  int32_t *dslot = n > 0 ? S.dev(hslot) : S.dev(hmoq);   // n == 0: no search, any non-null pointer
  uint8_t *dsobs = n > 0 ? S.dev(hsobs) : S.dev(hinv);
  // kept difference: serial only when a taking query without observations exists (the scan above); the batch form cannot know
  const RigLocalExtras rig = {Trl, tlr, cam_type2, cam_params2, S.dev(hl2r), S.dev(hr2l), {nullptr, 0, n_left}, release ? 1 : 0, &dt};
  const int rs = search_local_batch(m, &df, {std::max(n, 1), nullptr, 0, n}, &dm, {nmp, nullptr, 0, nmp}, 1, sf, nlevels, log_sf, cam_type, cam_params,
                                    0.f, view_cos_limit, th, bFarPoints, th_far, nnratio, dslot, dsobs, S.dev(hmoq), nullptr, S.dev(hnm), s, n > 0, &rig);
  if (rs < 0) return rs;
  const int nm = download_slots(m, s, S, hslot, hsobs, hnm, n, slot, slot_obs);
  if (nm < 0) return nm;
  const int32_t *moq = S.host(hmoq), *lvl = S.host(hlvl), *lvlr = S.host(hlvlr);
  const uint8_t *inv = S.host(hinv), *invr = S.host(hinvr);
  const float *px = S.host(hpx), *py = S.host(hpy), *dep = S.host(hdep), *vc = S.host(hvc), *pxr = S.host(hpxr), *pyr = S.host(hpyr);
  const float *depr = S.host(hdepr), *vcr = S.host(hvcr);
  // only what isInFrustum writes (Frame.cc:651-657): the flags always, the levels of eligible points, a side's fields where it is in view
  for (int i = 0; i < nmp; i++) {
    if (match_of_point) { match_of_point[2 * i] = n > 0 ? moq[2 * i] : -1; match_of_point[2 * i + 1] = n > 0 ? moq[2 * i + 1] : -1; }
    track->in_view[i] = inv[i]; track->in_view_r[i] = invr[i];
    if (!map->eligible[i]) continue;
    track->level[i] = lvl[i]; track->level_r[i] = lvlr[i];
    if (inv[i]) { track->proj_x[i] = px[i]; track->proj_y[i] = py[i]; track->depth[i] = dep[i]; track->view_cos[i] = vc[i]; }
    if (invr[i]) { track->proj_xr[i] = pxr[i]; track->proj_yr[i] = pyr[i]; track->depth_r[i] = depr[i]; track->view_cos_r[i] = vcr[i]; }
  }
  return nm;
}

void orbm_rig_right_camera(const float *Tcw, const float *Trl, const float *tlr, float *Tr, float *twc) {
  if (!Tcw || !Trl || !tlr || !Tr || !twc) return;
  float Ow[3];
  camera_centre(Tcw, Ow);
  rig_right_pose(Tcw, Trl, Tr);          // Frame.cc:1278-1279
  rig_right_centre(Tcw, tlr, Ow, twc);   // Frame.cc:1280
}

int orbm_search_by_projection_keyframe(orbm_t *m, const orbm_frame_t *cur, const float *sf, int nlevels, float logScaleFactor, int nKF,
                                       const uint8_t *valid, const float *Xw, const uint8_t *mpdesc, const float *kf_angle,
                                       const float *max_dist, const float *min_dist, const float *Tcw, int cam_type,
                                       const float *cam_params, float th, int ORBdist, int checkOri, int32_t *slot, uint8_t *slot_obs) {
  if (!m || !cur || !sf || nlevels < 1 || nKF < 0 || !Tcw || !cam_params || !slot || !slot_obs) return ORBX_E_ARG;
  if (nKF > 0 && (!valid || !Xw || !mpdesc || !kf_angle || !max_dist || !min_dist)) return ORBX_E_ARG;
  const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
  float Ow[3];
  camera_centre(Tcw, Ow);  // Ow = -Rcw.t()*tcw, :2297
  QueryArrays A(nKF);
  std::vector<int32_t> moq(nKF, -1);
  for (int i = 0; i < nKF; i++) {
    if (!valid[i]) continue;
    const float *x3Dw = Xw + 3 * i;
    float x3Dc[3];
    mat3_mul_add(Tcw, x3Dw, tcw, x3Dc);                                        // :2317
    float ux, vy;
    project(cam_type, cam_params, x3Dc[0], x3Dc[1], x3Dc[2], ux, vy);           // :2319
    if (!inside_bounds(ux, vy, cur->min_x, cur->max_x, cur->min_y, cur->max_y)) continue;   // :2321-2324
    float PO[3];
    for (int k = 0; k < 3; k++) PO[k] = x3Dw[k] - Ow[k];
    const float dist3D = norm3(PO);                                              // cv::norm(x3Dw-Ow), :2327-2328
    if (outside_scale_range(dist3D, min_dist, max_dist, i)) continue;            // :2334-2335
    const int lvl = predict_level(max_dist[i], dist3D, logScaleFactor, nlevels); // MapPoint::PredictScale, MapPoint.cc:587-602
    A.u[i] = ux; A.v[i] = vy;
    A.rad[i] = th * sf[lvl];                                                     // :2340
    A.minl[i] = lvl - 1; A.maxl[i] = lvl + 1;                                    // :2342
    A.flags[i] = 3;
  }
  const orbm_queries_t q = A.view(mpdesc);
  orbm_frame_t f = *cur;
  f.u_right = nullptr;  // no stereo gate in this overload
  int nmatches = orbm_search_by_projection(m, &f, &q, 0.f, ORBdist, 0, slot, slot_obs, moq.data(), nullptr);
  if (nmatches < 0 || !checkOri) return nmatches;
  return prune_by_rotation(nKF, moq.data(), kf_angle, cur->keys_un, slot, slot_obs, nmatches);
}

int orbm_search_by_projection_sim3(orbm_t *m, const orbm_frame_t *kf, const float *sf, int nlevels, float logScaleFactor, int nP,
                                   const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc,
                                   const float *max_dist, const float *min_dist, const float *Scw, const float *cam, int th,
                                   float ratioHamming, int32_t *slot, uint8_t *slot_obs) {
  return orbm_search_by_projection_sim3_cam(m, kf, sf, nlevels, logScaleFactor, nP, valid, Xw, normal, mpdesc, max_dist, min_dist, Scw, 0, cam, th,
                                            ratioHamming, slot, slot_obs);
}

int orbm_search_by_projection_sim3_cam(orbm_t *m, const orbm_frame_t *kf, const float *sf, int nlevels, float logScaleFactor, int nP,
                                       const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc,
                                       const float *max_dist, const float *min_dist, const float *Scw, int cam_type, const float *cam, int th,
                                       float ratioHamming, int32_t *slot, uint8_t *slot_obs) {
  if (!m || !kf || !sf || nlevels < 1 || nP < 0 || !Scw || !cam || !slot || !slot_obs || (cam_type != 0 && cam_type != 1)) return ORBX_E_ARG;
  if (nP > 0 && (!valid || !Xw || !normal || !mpdesc || !max_dist || !min_dist)) return ORBX_E_ARG;
  float T[16], Ow[3];
  decompose_sim3(Scw, T, Ow);                                                 // :498-503
  const float tcw[3] = {T[3], T[7], T[11]};
  QueryArrays A(nP);
  for (int i = 0; i < nP; i++) {
    if (!valid[i]) continue;
    const float *p3Dw = Xw + 3 * i;
    float p3Dc[3];
    mat3_mul_add(T, p3Dw, tcw, p3Dc);                                         // :523
    if ((double)p3Dc[2] < 0.0) continue;                                      // :526
    float ux, vy;
    project(cam_type, cam, p3Dc[0], p3Dc[1], p3Dc[2], ux, vy);                // :534, pKF->mpCamera->project
    if (!is_in_image(ux, vy, kf->min_x, kf->max_x, kf->min_y, kf->max_y)) continue;
    float PO[3];
    for (int k = 0; k < 3; k++) PO[k] = p3Dw[k] - Ow[k];
    const float dist = norm3(PO);                                             // cv::norm, :544
    if (outside_scale_range(dist, min_dist, max_dist, i)) continue;           // :546
    if (views_too_obliquely(PO, normal + 3 * i, dist)) continue;              // :552
    const int lvl = predict_level(max_dist[i], dist, logScaleFactor, nlevels);   // MapPoint::PredictScale(dist, pKF), MapPoint.cc:570-585
    A.u[i] = ux; A.v[i] = vy;
    A.rad[i] = (float)th * sf[lvl];                                           // :558
    A.minl[i] = lvl - 1; A.maxl[i] = lvl;                                     // :579-580
    A.flags[i] = 3;
  }
  const orbm_queries_t q = A.view(mpdesc);
  orbm_frame_t f = *kf;
  f.u_right = nullptr;
  // bestDist <= TH_LOW*ratioHamming with an int on the left: same as bestDist <= floor(50.f*ratioHamming)
  const int th_dist = (int)floorf((float)ORBM_TH_LOW * ratioHamming);
  return orbm_search_by_projection(m, &f, &q, 0.f, th_dist, 0, slot, slot_obs, nullptr, nullptr);
}

// ---- Fuse (ORBmatcher.cc:1425-1658 and :1660-1786) ------------------------------------------------------------------------
// The search of one map point does not depend on the others (no claim: a keypoint that already holds a map point stays a
// candidate, :1622-1640), so the device returns (bestIdx, bestDist) per map point and the caller applies the
// Replace / AddObservation bookkeeping on its objects in order.  Projection and gates on the host in fp32 as written.
static int fuse_core(orbm_t *m, const orbm_frame_t *kf, const float *sf, const float *inv_sigma2, int nlevels, float logScaleFactor, int nP,
                     const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc, const float *max_dist,
                     const float *min_dist, const float *T /* row-major 4x4 [Rcw | tcw] */, const float *Ow, int cam_type,
                     const float *cam, float bf, float th, bool chi2, int32_t *best_idx, int32_t *best_dist) {
  const float tcw[3] = {T[3], T[7], T[11]};
  QueryArrays A(nP, true);
  for (int i = 0; i < nP; i++) {
    best_idx[i] = -1; best_dist[i] = 256;
    if (!valid[i]) continue;
    const float *p3Dw = Xw + 3 * i;
    float p3Dc[3];
    mat3_mul_add(T, p3Dw, tcw, p3Dc);                                         // :1472 / :1694
    if (p3Dc[2] < 0.0f) continue;                                             // :1475 / :1697
    const float invz = 1 / p3Dc[2];                                           // :1481
    float ux, vy;
    project(cam_type, cam, p3Dc[0], p3Dc[1], p3Dc[2], ux, vy);                // :1487 / :1704
    if (!is_in_image(ux, vy, kf->min_x, kf->max_x, kf->min_y, kf->max_y)) continue;
    float PO[3];
    for (int k = 0; k < 3; k++) PO[k] = p3Dw[k] - Ow[k];
    const float dist3D = norm3(PO);                                           // cv::norm, :1502 / :1715
    if (outside_scale_range(dist3D, min_dist, max_dist, i)) continue;         // MapPoint.cc:552-563, :1505 / :1718
    if (views_too_obliquely(PO, normal + 3 * i, dist3D)) continue;            // :1514 / :1724
    const int lvl = predict_level(max_dist[i], dist3D, logScaleFactor, nlevels);   // MapPoint::PredictScale, MapPoint.cc:570-585
    A.u[i] = ux; A.v[i] = vy; A.ur[i] = ux - bf * invz;                       // :1495
    A.rad[i] = th * sf[lvl];                                                  // :1524 / :1731
    A.minl[i] = lvl - 1; A.maxl[i] = lvl;                                     // :1555 / :1752
    A.flags[i] = 1;                                                           // takes part, never claims
  }
  const orbm_queries_t q = A.view(mpdesc);
  orbm_frame_t f = *kf;
  std::vector<float> no_ur;
  if (chi2 && !f.u_right) { no_ur.assign((size_t)std::max(kf->n, 1), -1.0f); f.u_right = no_ur.data(); }
  if (!chi2) f.u_right = nullptr;
  std::vector<int32_t> slot((size_t)std::max(kf->n, 1), -1);
  std::vector<uint8_t> sobs((size_t)std::max(kf->n, 1), 0);
  SearchOpts o;
  o.nleft.konst = kf->n;
  o.fuse = chi2;
  if (chi2) for (int l = 0; l < nlevels && l < 16; l++) o.inv_sigma2[l] = inv_sigma2[l];
  const int rc = search_host(m, &f, &q, 0.f, ORBM_TH_LOW, 0, slot.data(), sobs.data(), best_idx, best_dist, o);
  if (rc < 0) return rc;
  int nFused = 0;
  for (int i = 0; i < nP; i++) nFused += best_idx[i] >= 0 ? 1 : 0;           // bestDist <= TH_LOW, :1622 / :1767
  return nFused;
}

int orbm_fuse(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, const float *inv_level_sigma2, int nlevels,
              float log_scale_factor, int nP, const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc,
              const float *max_dist, const float *min_dist, const float *Tcw, const float *Ow, int cam_type, const float *cam_params,
              float bf, float th, int32_t *best_idx, int32_t *best_dist) {
  if (!m || !kf || !scale_factors || !inv_level_sigma2 || nlevels < 1 || nlevels > 16 || nP < 0 || !Tcw || !Ow || !cam_params || !best_idx || !best_dist) return ORBX_E_ARG;
  if (nP > 0 && (!valid || !Xw || !normal || !mpdesc || !max_dist || !min_dist)) return ORBX_E_ARG;
  if (nP == 0) return 0;
  return fuse_core(m, kf, scale_factors, inv_level_sigma2, nlevels, log_scale_factor, nP, valid, Xw, normal, mpdesc, max_dist, min_dist, Tcw, Ow,
                   cam_type, cam_params, bf, th, true, best_idx, best_dist);
}

int orbm_fuse_sim3(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, int nlevels, float log_scale_factor, int nP,
                   const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc, const float *max_dist,
                   const float *min_dist, const float *Scw, const float *cam, float th, int32_t *best_idx, int32_t *best_dist) {
  return orbm_fuse_sim3_cam(m, kf, scale_factors, nlevels, log_scale_factor, nP, valid, Xw, normal, mpdesc, max_dist, min_dist, Scw, 0, cam, th,
                            best_idx, best_dist);
}

int orbm_fuse_sim3_cam(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, int nlevels, float log_scale_factor, int nP,
                       const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc, const float *max_dist,
                       const float *min_dist, const float *Scw, int cam_type, const float *cam, float th, int32_t *best_idx, int32_t *best_dist) {
  if (!m || !kf || !scale_factors || nlevels < 1 || nP < 0 || !Scw || !cam || !best_idx || !best_dist || (cam_type != 0 && cam_type != 1)) return ORBX_E_ARG;
  if (nP > 0 && (!valid || !Xw || !normal || !mpdesc || !max_dist || !min_dist)) return ORBX_E_ARG;
  if (nP == 0) return 0;
  float T[16], Ow[3];
  decompose_sim3(Scw, T, Ow);                                                 // :1668-1673
  return fuse_core(m, kf, scale_factors, nullptr, nlevels, log_scale_factor, nP, valid, Xw, normal, mpdesc, max_dist, min_dist, T, Ow, cam_type, cam,
                   0.f, th, false, best_idx, best_dist);
}

// ---- SearchInNeighbors (LocalMapping.cc:909-1058): Fuse of one point list into every target keyframe, one call ---------------
// What orbm_fuse_keyframes refuses about target t, or NULL.  It is what orbm_fuse refuses plus what k_fuse_keyframes relies on: the
// kernel divides by the bounds' extent and indexes the target's scale tables with PredictScale's level and every keypoint's octave.
// (orbm_fuse_sim3_keyframes: the same set with its own table pointers - no inv_level_sigma2, Scw for Tcw and Ow.)
static const char *fuse_keyframe_refusal(const orbm_frame_t &kf, int nlevels, int cam_type, bool null_table) {
  if (kf.n < 0) return "n < 0";
  if (kf.n > ORBM_MAX_KEYPOINTS) return "more than 15360 keypoints per frame not supported by the search kernels";
  if (kf.n > 0 && (!kf.keys_un || !kf.descriptors)) return "NULL keypoints or descriptors";
  if (!(kf.max_x > kf.min_x) || !(kf.max_y > kf.min_y)) return "empty image bounds";
  if (nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return "nlevels out of range";
  if (null_table) return "NULL scale table, pose or camera";
  if (cam_type != 0 && cam_type != 1) return "cam_type is neither 0 (Pinhole) nor 1 (KannalaBrandt8)";
  for (int i = 0; i < kf.n; i++)
    if (kf.keys_un[i].octave < 0 || kf.keys_un[i].octave >= nlevels) return "keypoint octave outside [0, nlevels)";
  return nullptr;
}
static const char *fuse_target_refusal(const orbm_fuse_target_t &g) {
  return fuse_keyframe_refusal(g.kf, g.nlevels, g.cam_type, !g.scale_factors || !g.inv_level_sigma2 || !g.Tcw || !g.Ow || !g.cam_params);
}
static const char *fuse_sim3_target_refusal(const orbm_fuse_sim3_target_t &g) {
  return fuse_keyframe_refusal(g.kf, g.nlevels, g.cam_type, !g.scale_factors || !g.Scw || !g.cam_params);
}

// What the two Fuse-into-targets entries share: the argument checks, ONE block (the point arrays once, the valid table, the per-target
// records, every target's arrays, the form's own parts, then the two result tables), the launches, both tables down in one copy, one
// synchronisation, the counts.  The records address the arrays by their offsets in the block.  A form names its target and record
// types and gives refusal(g), fill(S, g, R) for what its record has beyond the shared fields, extra(S, T, TP) and launch(...).
extern "C++" {
template <class Form>
static int fuse_into_targets(orbm_t *m, Form form, int T, const typename Form::Target *targets, int nP, const uint8_t *valid, const float *Xw,
                             const float *normal, const uint8_t *mpdesc, const float *max_dist, const float *min_dist, float th, int32_t *best_idx,
                             int32_t *best_dist, int32_t *nfused) {
  if (!m) return ORBX_E_ARG;
  const Refuse refuse{m, "target"};
  if (T < 0 || nP < 0) return refuse(-1, "T < 0 or nP < 0");
  if (T > 0 && !targets) return refuse(-1, "NULL target table");
  if (T > 0 && nP > 0 && (!valid || !Xw || !normal || !mpdesc || !max_dist || !min_dist || !best_idx || !best_dist || !nfused))
    return refuse(-1, "NULL point array or result table");
  for (int t = 0; t < T; t++)
    if (const char *why = Form::refusal(targets[t])) return refuse(t, why);
  if ((unsigned long long)T * (unsigned long long)nP > 0x7fffffffull) return refuse(-1, "more than 2^31 - 1 (target, point) pairs");
  if (T == 0 || nP == 0) {   // nothing to search: the device is not touched
    for (int t = 0; t < T && nfused; t++) nfused[t] = 0;
    return 0;
  }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t NP = (size_t)nP, TP = (size_t)T * NP;
  std::vector<typename Form::Rec> rec((size_t)T);
  Staging S{m};
  const auto hvalid = S.add(valid, TP);
  const auto hxw = S.add(Xw, 3 * NP), hnormal = S.add(normal, 3 * NP);
  const auto hdesc = S.add(mpdesc, 32 * NP);
  const auto hmax = S.add(max_dist, NP), hmin = S.add(min_dist, NP);
  const auto hrec = S.add(rec.data(), (size_t)T);   // copied at the upload, filled until then
  for (int t = 0; t < T; t++) {
    const auto &g = targets[t];
    const size_t n = (size_t)g.kf.n;
    typename Form::Rec &R = rec[(size_t)t];
    memset(&R, 0, sizeof(R));
    R.kp_off = S.offset(S.add(g.kf.keys_un, n));
    R.desc_off = S.offset(S.add(g.kf.descriptors, 32 * n));
    R.n = g.kf.n;
    R.min_x = g.kf.min_x; R.max_x = g.kf.max_x; R.min_y = g.kf.min_y; R.max_y = g.kf.max_y;
    R.inv_w = (float)ORBM_GRID_COLS / (g.kf.max_x - g.kf.min_x);   // Frame.cc:379
    R.inv_h = (float)ORBM_GRID_ROWS / (g.kf.max_y - g.kf.min_y);   // Frame.cc:380
    for (int l = 0; l < g.nlevels; l++) R.sf[l] = g.scale_factors[l];
    R.nlevels = g.nlevels; R.log_sf = g.log_scale_factor;
    R.cam_type = g.cam_type;
    for (int k = 0; k < (g.cam_type == 0 ? 4 : 8); k++) R.cam[k] = g.cam_params[k];
    Form::fill(S, g, R);
  }
  form.extra(S, (size_t)T, TP);
  const auto hidx = S.out<int32_t>(TP), hdist = S.out<int32_t>(TP);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  FusePoints P;
  P.nP = nP;
  P.valid = S.dev(hvalid); P.Xw = S.dev(hxw); P.normal = S.dev(hnormal); P.mpdesc = S.dev(hdesc);
  P.max_dist = S.dev(hmax); P.min_dist = S.dev(hmin);
  P.th = th;
  P.best_idx = S.dev(hidx); P.best_dist = S.dev(hdist);
  form.launch(s, dim3((unsigned)((nP + FUSE_NT - 1) / FUSE_NT), (unsigned)T), S, S.dev(hrec), P);
  MCHECK(m, hipGetLastError());
  MCHECK(m, S.download(s, hidx, hdist));
  MCHECK(m, hipStreamSynchronize(s));
  memcpy(best_idx, S.host(hidx), sizeof(int32_t) * TP);
  memcpy(best_dist, S.host(hdist), sizeof(int32_t) * TP);
  int total = 0;
  for (int t = 0; t < T; t++) {
    int nf = 0;
    for (size_t i = 0; i < NP; i++) nf += best_idx[(size_t)t * NP + i] >= 0 ? 1 : 0;   // bestDist <= TH_LOW, :1622 / :1767
    nfused[t] = nf;
    total += nf;
  }
  return total;
}
}  // extern "C++"

struct FuseKeyframesForm {
  using Target = orbm_fuse_target_t;
  using Rec = FuseTarget;
  static const char *refusal(const Target &g) { return fuse_target_refusal(g); }
  static void fill(Staging &S, const Target &g, Rec &R) {
    const size_t n = (size_t)g.kf.n;
    R.ur_off = g.kf.u_right && n ? S.offset(S.add(g.kf.u_right, n)) : FUSE_NO_UR;
    for (int l = 0; l < g.nlevels; l++) R.inv_sigma2[l] = g.inv_level_sigma2[l];
    for (int k = 0; k < 16; k++) R.Tcw[k] = g.Tcw[k];
    for (int k = 0; k < 3; k++) R.Ow[k] = g.Ow[k];
    R.bf = g.bf;
  }
  void extra(Staging &, size_t, size_t) {}
  void launch(hipStream_t s, dim3 grid, const Staging &S, const Rec *rec, const FusePoints &P) const {
    hipLaunchKernelGGL(k_fuse_keyframes, grid, dim3(FUSE_NT), 0, s, S.block(), rec, P);
  }
};

int orbm_fuse_keyframes(orbm_t *m, int T, const orbm_fuse_target_t *targets, int nP, const uint8_t *valid, const float *Xw, const float *normal,
                        const uint8_t *mpdesc, const float *max_dist, const float *min_dist, float th, int32_t *best_idx, int32_t *best_dist,
                        int32_t *nfused) {
  return fuse_into_targets(m, FuseKeyframesForm{}, T, targets, nP, valid, Xw, normal, mpdesc, max_dist, min_dist, th, best_idx, best_dist, nfused);
}

// ---- LoopClosing::SearchAndFuse (LoopClosing.cc:2631-2707): the Sim3 Fuse of one point list into every corrected keyframe, one call --
// The Sim3 record (no mvuRight), the per-target list lengths (zeros, uploaded with the block) and the lists in front of the result
// tables; every Scw is decomposed here as orbm_fuse_sim3_cam decomposes it (double division, camera_centre), so that the kernels' gates
// start from the same T and Ow.  Two launches (orb_fuse_sim3_kernels.h).
struct FuseSim3KeyframesForm {
  using Target = orbm_fuse_sim3_target_t;
  using Rec = FuseSim3Target;
  std::vector<int32_t> zero_counts;   // the lists' lengths start at 0 with the upload
  PartOf<int32_t> count, list;
  static const char *refusal(const Target &g) { return fuse_sim3_target_refusal(g); }
  static void fill(Staging &, const Target &g, Rec &R) { decompose_sim3(g.Scw, R.Tcw, R.Ow); }   // ORBmatcher.cc:1672-1677
  void extra(Staging &S, size_t T, size_t TP) {
    zero_counts.assign(T, 0);
    count = S.add(zero_counts.data(), T);
    list = S.out<int32_t>(TP);
  }
  void launch(hipStream_t s, dim3 grid, const Staging &S, const Rec *rec, const FusePoints &P) const {
    FuseLists Lst;
    Lst.count = S.dev(count); Lst.list = S.dev(list);
    hipLaunchKernelGGL(k_fuse_sim3_gate, grid, dim3(FUSE_NT), 0, s, rec, P, Lst);
    hipLaunchKernelGGL(k_fuse_sim3_search, grid, dim3(FUSE_NT), 0, s, S.block(), rec, P, Lst);
  }
};

int orbm_fuse_sim3_keyframes(orbm_t *m, int T, const orbm_fuse_sim3_target_t *targets, int nP, const uint8_t *valid, const float *Xw,
                             const float *normal, const uint8_t *mpdesc, const float *max_dist, const float *min_dist, float th,
                             int32_t *best_idx, int32_t *best_dist, int32_t *nfused) {
  return fuse_into_targets(m, FuseSim3KeyframesForm{}, T, targets, nP, valid, Xw, normal, mpdesc, max_dist, min_dist, th, best_idx, best_dist, nfused);
}

// ---- SearchBySim3 (ORBmatcher.cc:1788-2012) ------------------------------------------------------------------------------
// Two independent no-claim searches (map points of KF1 in KF2 and back) and a mutual-consistency pass.  cv::Mat algebra per
// SURVEY.md A.8 [OPENCV-UNVERIFIED]: scalar * Mat scales in double; a product with a transposed or scaled operand
// accumulates in double; plain 3x3 * 3x1 + 3x1 takes the small-matrix float path (mat3_mul_add).
namespace {
// Points of keyframe A (world Xw, pose RAw/tAw) into keyframe B through p_B = sRBA * p_A + tBA: the queries of one direction.
void sim3_project(const orbm_frame_t *kfB, const float *sfB, int nlevelsB, float logSfB, int nA, const uint8_t *valid, const float *Xw,
                  const float *max_dist, const float *min_dist, const float *RAw, const float *tAw, const float *sRBA, const float *tBA,
                  const float *cam, float th, QueryArrays &S) {
  float TA[16] = {0}, TB[16] = {0};
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { TA[4 * i + j] = RAw[3 * i + j]; TB[4 * i + j] = sRBA[3 * i + j]; }
  for (int i = 0; i < nA; i++) {
    if (!valid[i]) continue;                                                   // :1828-1832
    float pA[3], pB[3];
    mat3_mul_add(TA, Xw + 3 * i, tAw, pA);                                     // :1835
    mat3_mul_add(TB, pA, tBA, pB);                                             // :1836
    if ((double)pB[2] < 0.0) continue;                                         // :1839
    const float invz = (float)(1.0 / (double)pB[2]);                           // :1842
    const float x = pB[0] * invz, y = pB[1] * invz;
    const float u = cam[0] * x + cam[2], v = cam[1] * y + cam[3];              // :1846-1847, pKF1's intrinsics in both directions
    if (!is_in_image(u, v, kfB->min_x, kfB->max_x, kfB->min_y, kfB->max_y)) continue;
    const float dist3D = norm3(pB);                                            // cv::norm, :1855
    if (outside_scale_range(dist3D, min_dist, max_dist, i)) continue;          // :1858
    const int lvl = predict_level(max_dist[i], dist3D, logSfB, nlevelsB);      // MapPoint::PredictScale, MapPoint.cc:570-585
    S.u[i] = u; S.v[i] = v; S.rad[i] = th * sfB[lvl];                          // :1865
    S.minl[i] = lvl - 1; S.maxl[i] = lvl;                                      // :1884
    S.flags[i] = 1;
  }
}
}  // namespace

int orbm_search_by_sim3(orbm_t *m, const orbm_frame_t *kf1, const float *sf1, int nlevels1, float log_sf1, const uint8_t *valid1,
                        const float *Xw1, const uint8_t *mpdesc1, const float *max_dist1, const float *min_dist1, const float *R1w,
                        const float *t1w, const orbm_frame_t *kf2, const float *sf2, int nlevels2, float log_sf2, const uint8_t *valid2,
                        const float *Xw2, const uint8_t *mpdesc2, const float *max_dist2, const float *min_dist2, const float *R2w,
                        const float *t2w, float s12, const float *R12, const float *t12, const float *cam1, float th, int32_t *matches12) {
  if (!m || !kf1 || !kf2 || !sf1 || !sf2 || nlevels1 < 1 || nlevels2 < 1 || !R1w || !t1w || !R2w || !t2w || !R12 || !t12 || !cam1 || !matches12)
    return ORBX_E_ARG;
  const int N1 = kf1->n, N2 = kf2->n;
  if (N1 < 0 || N2 < 0) return ORBX_E_ARG;
  for (int i = 0; i < N1; i++) matches12[i] = -1;
  if (N1 == 0 || N2 == 0) return 0;
  if (!valid1 || !Xw1 || !mpdesc1 || !max_dist1 || !min_dist1 || !valid2 || !Xw2 || !mpdesc2 || !max_dist2 || !min_dist2) return ORBX_E_ARG;
  float sR12[9], sR21[9], t21[3];
  const double a21 = 1.0 / (double)s12;                                        // :1806
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      sR12[3 * i + j] = (float)((double)R12[3 * i + j] * (double)s12);         // :1805
      sR21[3 * i + j] = (float)((double)R12[3 * j + i] * a21);
    }
  for (int i = 0; i < 3; i++) {                                                // t21 = -sR21*t12, :1807
    double acc = 0;
    for (int k = 0; k < 3; k++) acc += (double)sR21[3 * i + k] * (double)t12[k];
    t21[i] = (float)(acc * -1.0);
  }
  QueryArrays A(N1), B(N2);
  std::vector<int32_t> bestA(N1, -1), bestB(N2, -1);
  sim3_project(kf2, sf2, nlevels2, log_sf2, N1, valid1, Xw1, max_dist1, min_dist1, R1w, t1w, sR21, t21, cam1, th, A);
  sim3_project(kf1, sf1, nlevels1, log_sf1, N2, valid2, Xw2, max_dist2, min_dist2, R2w, t2w, sR12, t12, cam1, th, B);
  struct Run { const orbm_frame_t *kf; QueryArrays *S; const uint8_t *desc; int32_t *best; } runs[2] = {{kf2, &A, mpdesc1, bestA.data()},
                                                                                                        {kf1, &B, mpdesc2, bestB.data()}};
  for (const Run &r : runs) {
    const orbm_queries_t q = r.S->view(r.desc);
    orbm_frame_t f = *r.kf;
    f.u_right = nullptr;
    std::vector<int32_t> slot((size_t)r.kf->n, -1);
    std::vector<uint8_t> sobs((size_t)r.kf->n, 0);
    const int rc = search_host(m, &f, &q, 0.f, ORBM_TH_HIGH, 0, slot.data(), sobs.data(), r.best, nullptr);  // :1895, :1967
    if (rc < 0) return rc;
  }
  int nFound = 0;                                                              // :1973-1987
  for (int i1 = 0; i1 < N1; i1++) {
    const int idx2 = bestA[i1];
    if (idx2 >= 0 && bestB[idx2] == i1) { matches12[i1] = idx2; nFound++; }
  }
  return nFound;
}

// ---- SearchForTriangulation (ORBmatcher.cc:981-1222), Pinhole / Pinhole, no second camera --------------------------------
namespace {
// cv::Mat algebra of ORBmatcher.cc:988-1010 and Pinhole.cpp:143-148 restated ([OPENCV-UNVERIFIED]):
// products without flags take cv::gemm's small-matrix float path, transposed / scaled operands the generic path with
// double accumulation, cv::invert(3x3 CV_32F) evaluates the cofactor formula in double.
void mul33(const float *A, const float *B, float *D) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) D[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
void inv33(const float *S, float *D) {
  const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7], s22 = S[8];
  double det = s00 * (s11 * s22 - s12 * s21) - s01 * (s10 * s22 - s12 * s20) + s02 * (s10 * s21 - s11 * s20);
  if (det == 0.) { for (int i = 0; i < 9; i++) D[i] = 0.f; return; }
  det = 1. / det;
  D[0] = (float)((s11 * s22 - s12 * s21) * det); D[1] = (float)((s02 * s21 - s01 * s22) * det); D[2] = (float)((s01 * s12 - s02 * s11) * det);
  D[3] = (float)((s12 * s20 - s10 * s22) * det); D[4] = (float)((s00 * s22 - s02 * s20) * det); D[5] = (float)((s02 * s10 - s00 * s12) * det);
  D[6] = (float)((s10 * s21 - s11 * s20) * det); D[7] = (float)((s01 * s20 - s00 * s21) * det); D[8] = (float)((s00 * s11 - s01 * s10) * det);
}
// What SearchForTriangulation forms once per Pinhole keyframe pair: the epipole of KF1 in image 2 and F12
void pinhole_pair_geometry(const float *R1w, const float *t1w, const float *R2w, const float *t2w, const float *Cw1, const float *cam1,
                           const float *cam2, float *F12, float &epx, float &epy) {
  // epipole in image 2: C2 = R2w*Cw+t2w, ep = pCamera2->project(C2), :988-994
  float C2[3];
  for (int i = 0; i < 3; i++) {
    const float t0 = R2w[3 * i] * Cw1[0] + R2w[3 * i + 1] * Cw1[1] + R2w[3 * i + 2] * Cw1[2];
    C2[i] = (float)((double)t0 + (double)t2w[i]);
  }
  project(0, cam2, C2[0], C2[1], C2[2], epx, epy);
  // R12 = R1w*R2w.t(); t12 = -R1w*R2w.t()*t2w+t1w, :1008-1010
  float R12[9], nR[9], t12[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double acc = 0;
      for (int k = 0; k < 3; k++) acc += (double)R1w[3 * i + k] * (double)R2w[3 * j + k];
      R12[3 * i + j] = (float)acc;
      nR[3 * i + j] = (float)(-acc);
    }
  for (int i = 0; i < 3; i++) {
    const float t0 = nR[3 * i] * t2w[0] + nR[3 * i + 1] * t2w[1] + nR[3 * i + 2] * t2w[2];
    t12[i] = (float)((double)t0 + (double)t1w[i]);
  }
  // F12 = K1.t().inv()*t12x*R12*K2.inv(), Pinhole.cpp:145-148
  const float tx[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
  const float K1t[9] = {cam1[0], 0.f, 0.f, 0.f, cam1[1], 0.f, cam1[2], cam1[3], 1.f};
  const float K2[9] = {cam2[0], 0.f, cam2[2], 0.f, cam2[1], cam2[3], 0.f, 0.f, 1.f};
  float K1ti[9], K2i[9], A[9], B[9];
  inv33(K1t, K1ti);
  inv33(K2, K2i);
  mul33(K1ti, tx, A);
  mul33(A, R12, B);
  mul33(B, K2i, F12);
}
}  // namespace

// merge-walk of the two feature vectors (ORBmatcher.cc:1036-1188): one work item per unmatched keypoint of KF1 in a shared node
// ur1 = KF1's mvuRight, NULL for a two-camera rig (bStereo1 is false there, :1057).  Appends to items; nb = the neighbour they name.
static int triangulation_items(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_t *k2, const float *ur1, int bOnlyStereo,
                               std::vector<TriItem> &items, int nb = 0) {
  int f1 = 0, f2 = 0;
  while (f1 < k1->n_nodes && f2 < k2->n_nodes) {
    if (k1->node_id[f1] == k2->node_id[f2]) {
      const int s2 = k2->node_start[f2], l2 = k2->node_start[f2 + 1] - s2;
      if (l2 > 0xffff) { m->err = "vocabulary node with more than 65535 keypoints"; return ORBX_E_ARG; }
      for (int i1 = k1->node_start[f1]; i1 < k1->node_start[f1 + 1]; i1++) {
        const int idx1 = k1->node_idx[i1];
        if (idx1 < 0 || idx1 >= k1->n) return ORBX_E_ARG;
        if (k1->has_mappoint[idx1]) continue;                          // :1050-1055
        if (bOnlyStereo && !(ur1 && ur1[idx1] >= 0)) continue;         // :1057-1061
        if (l2 > 0) items.push_back(TriItem{idx1, s2, l2, nb});
      }
      f1++; f2++;
    } else if (k1->node_id[f1] < k2->node_id[f2]) {
      while (f1 < k1->n_nodes && k1->node_id[f1] < k2->node_id[f2]) f1++;
    } else {
      while (f2 < k2->n_nodes && k2->node_id[f2] < k1->node_id[f1]) f2++;
    }
  }
  return 0;
}

// Candidate lists of SearchForTriangulation, per keypoint of KF1 in CSR form: start[k1->n + 1]; per candidate the keypoint of KF2 and
// the distance, ordered (distance ascending, position in the node descending) = the order in which the reference's running best
// would prefer them ("dist > bestDist -> skip", update on <=: the LAST minimum among the candidates its predicate accepts).
static int triangulation_candidates(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_t *k2, float ep_x, float ep_y, int epipole_gate,
                                    int bOnlyStereo, std::vector<int32_t> &start, std::vector<int32_t> &idx2, std::vector<int32_t> &dist) {
  start.assign((size_t)k1->n + 1, 0);
  idx2.clear(); dist.clear();
  if (k1->n == 0 || k2->n == 0 || k1->n_nodes == 0 || k2->n_nodes == 0) return 0;
  std::vector<TriItem> items;
  const int rc = triangulation_items(m, k1, k2, k1->u_right, bOnlyStereo, items);
  if (rc < 0) return rc;
  if (items.empty()) return 0;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t nidx2 = (size_t)k2->node_start[k2->n_nodes];
  Staging S{m};
  const auto DESC1 = S.add(k1->descriptors, 32 * (size_t)k1->n);
  const auto UR1 = S.add(k1->u_right, (size_t)k1->n);
  const auto DESC2 = S.add(k2->descriptors, 32 * (size_t)k2->n);
  const auto KP2 = S.add(k2->keys_un, (size_t)k2->n);
  const auto UR2 = S.add(k2->u_right, (size_t)k2->n);
  const auto HASMP2 = S.add(k2->has_mappoint, (size_t)k2->n);
  const auto NODE_IDX2 = S.add(k2->node_idx, nidx2);
  const auto ITEMS = S.add(items.data(), items.size());
  const int rs = S.upload(s, false);
  if (rs < 0) return rs;
  TriCandParams T;
  memset(&T, 0, sizeof(T));
  T.desc1 = (const uint32_t *)S.dev(DESC1); T.ur1 = S.dev(UR1);
  T.desc2 = (const uint32_t *)S.dev(DESC2); T.kp2 = (const float *)S.dev(KP2); T.ur2 = S.dev(UR2);
  T.hasmp2 = S.dev(HASMP2); T.node_idx2 = S.dev(NODE_IDX2);
  T.items = S.dev(ITEMS); T.nitems = (int)items.size();
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) T.sf2[l] = l < k2->nlevels ? k2->scale_factors[l] : 0.f;
  T.epx = ep_x; T.epy = ep_y; T.epipole_gate = epipole_gate; T.bOnlyStereo = bOnlyStereo;
  const size_t ni = items.size();
  std::vector<int32_t> off(ni), cnt(ni);
  std::vector<uint32_t> keys;
  size_t cap = std::max<size_t>(16 * ni, 1024);
  for (int attempt = 0; attempt < 2; attempt++) {   // the second attempt knows the exact total
    MCHECK(m, m->d_tri_count.reserve(sizeof(int32_t) * (2 * ni + 1)));
    MCHECK(m, m->d_tri_keys.reserve(sizeof(uint32_t) * cap));
    T.item_off = (int32_t *)m->d_tri_count.p; T.item_cnt = T.item_off + ni; T.total = T.item_cnt + ni;
    T.keys = (uint32_t *)m->d_tri_keys.p; T.cap = (int)std::min<size_t>(cap, 0x7fffffff);
    MCHECK(m, hipMemsetAsync(T.total, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_triangulation_candidates, dim3((T.nitems + 3) / 4), dim3(256), 0, s, T);
    MCHECK(m, hipGetLastError());
    int32_t total = 0;
    MCHECK(m, hipMemcpyAsync(&total, T.total, sizeof(total), hipMemcpyDeviceToHost, s));
    MCHECK(m, hipMemcpyAsync(off.data(), T.item_off, sizeof(int32_t) * ni, hipMemcpyDeviceToHost, s));
    MCHECK(m, hipMemcpyAsync(cnt.data(), T.item_cnt, sizeof(int32_t) * ni, hipMemcpyDeviceToHost, s));
    MCHECK(m, hipStreamSynchronize(s));
    if ((size_t)total <= cap) {
      keys.resize((size_t)total);
      if (total > 0) MCHECK(m, hipMemcpy(keys.data(), T.keys, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost));
      break;
    }
    if (attempt == 1) { m->err = "triangulation candidates: buffer too small twice"; return ORBX_E_HIP; }
    cap = (size_t)total;
  }
  // CSR over the keypoints of KF1 (a keypoint belongs to one node, i.e. to at most one item), every list ordered by key
  for (size_t i = 0; i < ni; i++) start[(size_t)items[i].idx1 + 1] += cnt[i];
  for (int i = 0; i < k1->n; i++) start[(size_t)i + 1] += start[(size_t)i];
  idx2.resize(keys.size()); dist.resize(keys.size());
  for (size_t i = 0; i < ni; i++) {
    if (!cnt[i]) continue;
    uint32_t *kb = keys.data() + off[i];
    std::sort(kb, kb + cnt[i]);
    const int o = start[(size_t)items[i].idx1];
    for (int c = 0; c < cnt[i]; c++) {
      idx2[(size_t)o + c] = k2->node_idx[items[i].start2 + (0xffff - (int)(kb[c] & 0xffffu))];
      dist[(size_t)o + c] = (int32_t)(kb[c] >> 16);
    }
  }
  return (int)keys.size();
}

int orbm_triangulation_candidates(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_t *k2, float ep_x, float ep_y, int epipole_gate,
                                  int bOnlyStereo, int32_t *cand_start, int32_t *cand_idx2, int32_t *cand_dist, int cap) {
  if (!m || !k1 || !k2 || !cand_start || cap < 0 || (cap > 0 && (!cand_idx2 || !cand_dist))) return ORBX_E_ARG;
  if (k1->n < 0 || k2->n < 0 || k2->nlevels < 1 || k2->nlevels > ORBX_MAX_LEVELS) return ORBX_E_ARG;
  if ((k1->n > 0 && (!k1->u_right || !k1->has_mappoint)) || (k2->n > 0 && (!k2->u_right || !k2->has_mappoint))) return ORBX_E_ARG;
  std::vector<int32_t> start, idx2, dist;
  const int total = triangulation_candidates(m, k1, k2, ep_x, ep_y, epipole_gate, bOnlyStereo, start, idx2, dist);
  if (total < 0) return total;
  memcpy(cand_start, start.data(), sizeof(int32_t) * start.size());
  if (total <= cap && total > 0) {
    memcpy(cand_idx2, idx2.data(), sizeof(int32_t) * (size_t)total);
    memcpy(cand_dist, dist.data(), sizeof(int32_t) * (size_t)total);
  }
  return total;   // > cap: nothing but cand_start was written; call again with that capacity
}

// rotation-histogram pruning of SearchForTriangulation's pairs, ORBmatcher.cc:1162-1172, :1191-1207
static int prune_pairs_by_rotation(const orbm_keyframe_t *k1, const orbm_keyframe_t *k2, int32_t *matches12, int nmatches) {
  RotHist H;   // the reference fills the histogram in merge-walk order; only the bin sizes matter afterwards
  for (int i = 0; i < k1->n; i++)
    if (matches12[i] >= 0) H.add(k1->keys_un[i].angle - k2->keys_un[matches12[i]].angle, i);
  H.for_each_pruned([&](int i1) { matches12[i1] = -1; nmatches--; });
  return nmatches;
}

int orbm_search_for_triangulation_pred(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_t *k2, float ep_x, float ep_y, int epipole_gate,
                                       int bOnlyStereo, int bCoarse, int checkOri, orbm_pair_predicate_t pred, void *user, int32_t *matches12) {
  if (!m || !k1 || !k2 || !matches12 || (!pred && !bCoarse)) return ORBX_E_ARG;
  if (k1->n < 0 || k2->n < 0 || k2->nlevels < 1 || k2->nlevels > ORBX_MAX_LEVELS) return ORBX_E_ARG;
  if ((k1->n > 0 && (!k1->u_right || !k1->has_mappoint)) || (k2->n > 0 && (!k2->u_right || !k2->has_mappoint))) return ORBX_E_ARG;
  for (int i = 0; i < k1->n; i++) matches12[i] = -1;
  std::vector<int32_t> start, idx2, dist;
  const int total = triangulation_candidates(m, k1, k2, ep_x, ep_y, epipole_gate, bOnlyStereo, start, idx2, dist);
  if (total < 0) return total;
  int nmatches = 0;
  for (int i = 0; i < k1->n; i++)
    for (int c = start[(size_t)i]; c < start[(size_t)i + 1]; c++)
      if (bCoarse || pred(user, i, idx2[(size_t)c])) { matches12[i] = idx2[(size_t)c]; nmatches++; break; }   // :1148-1153
  if (checkOri && nmatches > 0) nmatches = prune_pairs_by_rotation(k1, k2, matches12, nmatches);
  return nmatches;
}

// Why a keyframe (nlevels in range) cannot be read by the kernels, or NULL.  rig: u_right is not read; scales = false: neither are
// its scale tables (KF1 under Pinhole's test).
static const char *tri_keyframe_refusal(const orbm_keyframe_t *k, bool rig, bool scales = true) {
  if ((scales && (!k->level_sigma2 || !k->scale_factors)) || k->n_nodes < 0) return "keyframe: NULL scale table";
  if (k->n > 0 && (!k->keys_un || !k->descriptors || !k->has_mappoint || (!rig && !k->u_right))) return "keyframe: NULL array";
  if (k->n_nodes > 0 && (!k->node_id || !k->node_start || !k->node_idx || k->node_start[0] < 0)) return "keyframe: NULL feature vector";
  for (int i = 0; scales && i < k->n; i++)   // mvLevelSigma2[kp.octave], :1148
    if (k->keys_un[i].octave < 0 || k->keys_un[i].octave >= k->nlevels) return "keypoint octave outside [0, nlevels)";
  for (int f = 0; f < k->n_nodes; f++)
    if (k->node_start[f + 1] < k->node_start[f]) return "feature vector: node_start decreases";
  return nullptr;
}
// The members of KF2's nodes are keypoints of KF2 (n_nodes > 0)
static const char *tri_members_refusal(const orbm_keyframe_t *k2) {
  const size_t nidx2 = (size_t)k2->node_start[k2->n_nodes];
  for (size_t i = 0; i < nidx2; i++)
    if (k2->node_idx[i] < 0 || k2->node_idx[i] >= k2->n) return "feature vector: keypoint index out of range";
  return nullptr;
}

// ---- SearchForTriangulation of one keyframe against K neighbours in one call (LocalMapping.cc:475-583) ----------------------------
// What the two entries share once every neighbour that is not skipped has been validated: the merge walks, ONE staged block (KF1 once,
// the arrays of every neighbour that has work, the items, the neighbour table), one fill, the kernels over all neighbours, one
// download of [K][n1], one synchronisation.  nb[j] arrives with F12 / epipole / n_left2; kb8 == NULL selects Pinhole's test.
// np != NULL (orbm_create_new_map_points*): the body of the loop runs on the rows in device memory behind the search, its inputs ride in
// the same block, matches12 / nmatches may be NULL (then the rows are not downloaded).
struct NewPointsCall {
  const orbm_keyframe_geometry_t *g1, *g2;
  int cam_type;                         // 0 Pinhole, 1 KannalaBrandt8
  const float *cams1, *cams2;           // mvParameters of kf1's cameras; of neighbour j's at cams2 + j * cams2_stride
  int cams2_stride;
  const int32_t *n_left2;               // NULL: -1 for every neighbour
  float scale_factor1, th_far_points;
  int far_points;
  uint8_t *status;                      // [K][n1] or NULL
  std::vector<orbm_new_point_t> list;   // out: the new points in creation order
};
static void new_point_camera(orbm_new_point_camera_t &c, const orbm_keyframe_t &k, const orbm_keyframe_geometry_t &g, int cam_type, const float *cams,
                             int n_left);

static int triangulation_neighbours(orbm_t *m, const char *kind, const orbm_keyframe_t *k1, int n_left1, int K, const orbm_keyframe_t *k2, const uint8_t *skip,
                                    std::vector<TriNb> &nb, const std::vector<TriKb8Consts> *kb8, int bOnlyStereo, int bCoarse,
                                    int32_t *matches12, int32_t *nmatches, NewPointsCall *np = nullptr) {
  const Refuse refuse{m, kind};   // kind NULL: a pair entry, no item named
  const bool rig = n_left1 != -1;
  const size_t n1 = (size_t)k1->n;
  if (matches12) for (size_t i = 0; i < (size_t)K * n1; i++) matches12[i] = -1;
  if (nmatches) for (int j = 0; j < K; j++) nmatches[j] = 0;
  std::vector<TriItem> items;
  std::vector<uint8_t> live((size_t)K, 0);
  for (int j = 0; j < K; j++) {
    if ((skip && skip[j]) || n1 == 0 || k2[j].n == 0 || k1->n_nodes == 0 || k2[j].n_nodes == 0) continue;
    const size_t before = items.size();
    m->err.clear();
    const int rc = triangulation_items(m, k1, &k2[j], rig ? nullptr : k1->u_right, bOnlyStereo, items, j);
    if (rc < 0) { refuse(j, (m->err.empty() ? std::string("kf1: keypoint index out of range") : std::string(m->err)).c_str()); return rc; }
    live[(size_t)j] = items.size() > before;
  }
  if (items.empty()) return 0;
  const size_t ni = items.size();
  size_t cap = 0;   // every member of an item's node can be a candidate: the key list never outgrows this
  for (const TriItem &it : items) cap += (size_t)it.len2;
  if (cap > 0x7fffffffu || ni > 0x7fffffffu)
    return refuse(-1, refuse.kind ? "more than 2^31 - 1 keypoint pairs in shared vocabulary nodes over all neighbours"
                                  : "more than 2^31 - 1 keypoint pairs in shared vocabulary nodes");
  if (m->tri_layout == 1 && K > 1) {   // KF1-keypoint-major: one idx1 against consecutive neighbours (a stable counting sort on idx1); measured slower, DESIGN.md 6
    std::vector<size_t> at(n1 + 1, 0);
    for (const TriItem &it : items) at[(size_t)it.idx1 + 1]++;
    for (size_t i = 0; i < n1; i++) at[i + 1] += at[i];
    std::vector<TriItem> byKey(ni);
    for (const TriItem &it : items) byKey[at[(size_t)it.idx1]++] = it;
    items.swap(byKey);
  }
  static const int32_t zero = 0;
  Staging S{m};
  const auto KP1 = S.add(k1->keys_un, n1);
  const auto DESC1 = S.add(k1->descriptors, 32 * n1);
  const auto UR1 = S.add(rig ? nullptr : k1->u_right, rig ? 0 : n1);
  for (int j = 0; j < K; j++) {
    if (!live[(size_t)j]) continue;
    const orbm_keyframe_t &k = k2[j];
    const size_t n2 = (size_t)k.n;
    TriNb &N = nb[(size_t)j];
    N.desc2 = S.offset(S.add(k.descriptors, 32 * n2));
    N.kp2 = S.offset(S.add(k.keys_un, n2));
    N.ur2 = S.offset(S.add(rig ? nullptr : k.u_right, rig ? 0 : n2));
    N.hasmp2 = S.offset(S.add(k.has_mappoint, n2));
    N.node_idx2 = S.offset(S.add(k.node_idx, (size_t)k.node_start[k.n_nodes]));
    for (int l = 0; l < k.nlevels; l++) { N.sf2[l] = k.scale_factors[l]; N.sigma2_2[l] = k.level_sigma2[l]; }
  }
  const auto ITEMS = S.add(items.data(), ni);
  const auto NB = S.add(nb.data(), (size_t)K);
  const auto CONSTS = S.add(kb8 ? kb8->data() : nullptr, kb8 ? (size_t)K : 0);
  const auto TOTAL = S.add(kb8 ? &zero : nullptr, kb8 ? 1 : 0);   // the candidate total starts at the uploaded 0
  const size_t out_bytes = sizeof(int32_t) * (size_t)K * n1;
  const auto MATCHES12 = S.out<int32_t>((size_t)K * n1);
  const auto BEST = S.out<uint32_t>(kb8 ? ni : 0);
  const auto KEYS = S.out<uint32_t>(kb8 ? cap : 0);
  const auto KEY_ITEM = S.out<int32_t>(kb8 ? cap : 0);
  // the body's inputs and outputs behind the search's: per keyframe with stereo keypoints {mvDepth, mvKeys.pt}, the constants of the new
  // keyframe and of every neighbour, then status / x3D / first / total + list
  std::vector<orbm_new_point_camera_t> np_cams;
  std::vector<std::vector<float>> np_stereo;
  std::vector<uint64_t> np_stereo2;
  PartOf<float> NP_STEREO1{}, NP_X3D{};
  PartOf<orbm_new_point_camera_t> NP_CAMS{};
  PartOf<uint64_t> NP_STEREO2{};
  PartOf<uint8_t> NP_STATUS{};
  PartOf<int32_t> NP_FIRST{}, NP_TOTAL{};
  PartOf<orbm_new_point_t> NP_LIST{};
  if (np) {
    np_cams.resize((size_t)K + 1);
    memset(np_cams.data(), 0, sizeof(orbm_new_point_camera_t) * np_cams.size());
    np_stereo.resize((size_t)K + 1);
    np_stereo2.assign((size_t)K, ~(uint64_t)0);
    auto pack_stereo = [&](const orbm_keyframe_t &k, const orbm_keyframe_geometry_t &g, std::vector<float> &out) {
      bool any = false;
      for (int i = 0; !rig && i < k.n && !any; i++) any = k.u_right[i] >= 0;
      if (!any) return;
      out.resize(3 * (size_t)k.n);
      for (int i = 0; i < k.n; i++) { out[3 * (size_t)i] = g.depth[i]; out[3 * (size_t)i + 1] = g.keys[i].x; out[3 * (size_t)i + 2] = g.keys[i].y; }
    };
    new_point_camera(np_cams[0], *k1, *np->g1, np->cam_type, np->cams1, n_left1);
    pack_stereo(*k1, *np->g1, np_stereo[0]);
    NP_STEREO1 = S.add(np_stereo[0].empty() ? (const float *)nullptr : np_stereo[0].data(), np_stereo[0].size());
    for (int j = 0; j < K; j++) {
      if (!live[(size_t)j]) continue;
      new_point_camera(np_cams[(size_t)j + 1], k2[j], np->g2[j], np->cam_type, np->cams2 + (size_t)j * (size_t)np->cams2_stride, np->n_left2 ? np->n_left2[j] : -1);
      pack_stereo(k2[j], np->g2[j], np_stereo[(size_t)j + 1]);
      const std::vector<float> &st = np_stereo[(size_t)j + 1];
      if (!st.empty()) np_stereo2[(size_t)j] = S.offset(S.add(st.data(), st.size()));
    }
    NP_CAMS = S.add(np_cams.data(), np_cams.size());
    NP_STEREO2 = S.add(np_stereo2.data(), (size_t)K);
    NP_STATUS = S.out<uint8_t>((size_t)K * n1);
    NP_X3D = S.out<float>(3 * (size_t)K * n1);
    NP_FIRST = S.out<int32_t>(n1);
    NP_TOTAL = S.out<int32_t>(1);
    NP_LIST = S.out<orbm_new_point_t>(n1);
  }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  { const int rs = S.upload(s, false); if (rs < 0) return rs; }   // no output mirror: the rows go straight to the caller
  // matches12 = -1 and best = 0xffffffff in one fill (adjacent parts of the block)
  MCHECK(m, kb8 ? S.fill(s, MATCHES12, BEST, 0xff) : S.fill(s, MATCHES12, MATCHES12, 0xff));
  TriNbParams T;
  memset(&T, 0, sizeof(T));
  T.block = S.block(); T.nb = S.dev(NB);
  T.kp1 = (const float *)S.dev(KP1); T.desc1 = (const uint32_t *)S.dev(DESC1); T.ur1 = S.dev(UR1);
  T.items = S.dev(ITEMS); T.nitems = (int)ni; T.n1 = k1->n;
  T.bOnlyStereo = bOnlyStereo; T.bCoarse = bCoarse;
  T.matches12 = S.dev(MATCHES12);
  if (!kb8) {
    hipLaunchKernelGGL(k_triangulation_match_neighbours, dim3((unsigned)((ni + 3) / 4)), dim3(256), 0, s, T);
    MCHECK(m, hipGetLastError());
  } else {
    TriCandNbParams C;
    memset(&C, 0, sizeof(C));
    C.in = T; C.epipole_gate = rig ? 0 : 1;   // !pKF1->mpCamera2, :1105
    C.keys = S.dev(KEYS); C.cap = (int)cap; C.key_item = S.dev(KEY_ITEM); C.total = S.dev(TOTAL);
    TriKb8NbParams P;
    memset(&P, 0, sizeof(P));
    P.in = T; P.keys = C.keys; P.key_item = C.key_item; P.total = C.total; P.cap = C.cap;
    P.consts = S.dev(CONSTS);
    for (int l = 0; l < k1->nlevels; l++) P.sigma2_1[l] = k1->level_sigma2[l];
    P.n_left1 = n_left1; P.best = S.dev(BEST);
    hipLaunchKernelGGL(k_triangulation_candidates_neighbours, dim3((unsigned)((ni + 3) / 4)), dim3(256), 0, s, C);
    MCHECK(m, hipGetLastError());
    hipLaunchKernelGGL(k_triangulation_kb8_predicate_neighbours, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
    hipLaunchKernelGGL(k_triangulation_kb8_result_neighbours, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
  }
  std::vector<uint8_t> np_out;   // total and the list behind it, adjacent parts of the block: one copy
  if (np) {
    NewPointsParams P;
    memset(&P, 0, sizeof(P));
    P.in = T;
    P.cams = S.dev(NP_CAMS); P.stereo1 = S.dev(NP_STEREO1); P.stereo2 = S.dev(NP_STEREO2);
    P.K = K; P.scale_factor1 = np->scale_factor1; P.th_far_points = np->th_far_points; P.far_points = np->far_points;
    P.status = S.dev(NP_STATUS); P.x3d = S.dev(NP_X3D); P.first = S.dev(NP_FIRST);
    P.list = S.dev(NP_LIST); P.total = S.dev(NP_TOTAL);
    MCHECK(m, S.fill(s, NP_FIRST, NP_FIRST, 0x7f));
    hipLaunchKernelGGL(k_new_points_geometry, dim3((unsigned)(((size_t)K * n1 + 255) / 256)), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
    hipLaunchKernelGGL(k_new_points_emit, dim3((unsigned)K), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
    np_out.resize(S.span(NP_TOTAL, NP_LIST));
    MCHECK(m, hipMemcpyAsync(np_out.data(), S.dev(NP_TOTAL), np_out.size(), hipMemcpyDeviceToHost, s));
    if (np->status) MCHECK(m, hipMemcpyAsync(np->status, S.dev(NP_STATUS), (size_t)K * n1, hipMemcpyDeviceToHost, s));
  }
  if (matches12) MCHECK(m, hipMemcpyAsync(matches12, S.dev(MATCHES12), out_bytes, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipStreamSynchronize(s));
  if (np) {
    int32_t total = 0;
    memcpy(&total, np_out.data(), sizeof(total));
    if (total < 0 || (size_t)total > n1) { m->err = "new points: list count out of range"; return ORBX_E_HIP; }
    np->list.resize((size_t)total);
    if (total) memcpy(np->list.data(), np_out.data() + (S.offset(NP_LIST) - S.offset(NP_TOTAL)), sizeof(orbm_new_point_t) * (size_t)total);
  }
  long long sum = 0;
  for (int j = 0; matches12 && j < K; j++) {
    int nj = 0;
    for (size_t i = 0; i < n1; i++) nj += matches12[(size_t)j * n1 + i] >= 0;
    if (nmatches) nmatches[j] = nj;
    sum += nj;
  }
  return (int)std::min<long long>(sum, 0x7fffffff);
}

// The refusals of a one-call search that do not depend on the epipolar test: the tables, then every neighbour that is not skipped
// as the per-pair entry would refuse it, m->err naming the neighbour.  1: nothing to search (K == 0, every neighbour skipped).
static int triangulation_neighbours_refusal(orbm_t *m, const orbm_keyframe_t *k1, bool rig, bool kb8, int K, const orbm_keyframe_t *k2,
                                            const uint8_t *skip) {
  const Refuse refuse{m, "neighbour"};
  if (K < 0) return refuse(-1, "K < 0");
  if (K > 0 && !k2) return refuse(-1, "NULL neighbour table");
  if (k1->n < 0) return refuse(-1, "kf1: n < 0");
  if (kb8 && (k1->nlevels < 1 || k1->nlevels > ORBX_MAX_LEVELS)) return refuse(-1, "kf1: nlevels out of range");
  int searched = 0;
  for (int j = 0; j < K; j++) searched += !(skip && skip[j]);
  if (searched == 0) return 1;
  if (const char *why = tri_keyframe_refusal(k1, rig, kb8)) return refuse(-1, why);
  for (int j = 0; j < K; j++) {
    if (skip && skip[j]) continue;
    const orbm_keyframe_t &k = k2[j];
    if (k.n < 0) return refuse(j, "n < 0");
    if (k.nlevels < 1 || k.nlevels > ORBX_MAX_LEVELS) return refuse(j, "nlevels out of range");
    if (const char *why = tri_keyframe_refusal(&k, rig)) return refuse(j, why);
    if (k.n_nodes > 0)
      if (const char *why = tri_members_refusal(&k)) return refuse(j, why);
  }
  return 0;
}

int orbm_search_for_triangulation_neighbours(orbm_t *m, const orbm_keyframe_t *k1, int K, const orbm_keyframe_t *k2, const float *R1w, const float *t1w,
                                             const float *Cw1, const float *cam1, const float *R2w, const float *t2w, const float *cam2,
                                             const uint8_t *skip, int bOnlyStereo, int bCoarse, int32_t *matches12, int32_t *nmatches) {
  if (!m || !k1) return ORBX_E_ARG;
  const int rr = triangulation_neighbours_refusal(m, k1, false, false, K, k2, skip);
  if (rr < 0) return rr;
  if (K > 0 && (!matches12 || !nmatches)) { m->err = "NULL result table"; return ORBX_E_ARG; }
  if (rr == 0 && (!R1w || !t1w || !Cw1 || !cam1 || !R2w || !t2w || !cam2)) { m->err = "NULL pose or camera table"; return ORBX_E_ARG; }
  std::vector<TriNb> nb((size_t)K);
  if (K > 0) memset(nb.data(), 0, sizeof(TriNb) * (size_t)K);
  for (int j = 0; j < K && rr == 0; j++)
    if (!(skip && skip[j])) pinhole_pair_geometry(R1w, t1w, R2w + 9 * j, t2w + 3 * j, Cw1, cam1, cam2 + 4 * j, nb[(size_t)j].F12, nb[(size_t)j].epx, nb[(size_t)j].epy);
  return triangulation_neighbours(m, "neighbour", k1, -1, K, k2, skip, nb, nullptr, bOnlyStereo, bCoarse, matches12, nmatches);
}

// The KannalaBrandt8 form's neighbour table and constants from the caller's tables (rr: triangulation_neighbours_refusal's answer)
static int kb8_neighbour_tables(const Refuse &refuse, int rr, bool rig, int K, const orbm_keyframe_t *k2, const int32_t *n_left2, const float *ep, const float *cams1,
                                const float *cams2, const float *T12, const uint8_t *skip, std::vector<TriNb> &nb, std::vector<TriKb8Consts> &consts) {
  if (rr == 0 && (!n_left2 || !ep || !cams1 || !cams2 || !T12)) return refuse(-1, "NULL n_left2, epipole, camera or pose table");
  nb.resize((size_t)K);
  consts.resize((size_t)K);
  if (K > 0) { memset(nb.data(), 0, sizeof(TriNb) * (size_t)K); memset(consts.data(), 0, sizeof(TriKb8Consts) * (size_t)K); }
  for (int j = 0; j < K && rr == 0; j++) {
    if (skip && skip[j]) continue;
    if ((n_left2[j] == -1) != !rig) return refuse(j, "n_left: one keyframe with and one without a second camera");
    if (n_left2[j] < -1 || n_left2[j] > k2[j].n) return refuse(j, "n_left out of range");
    TriNb &N = nb[(size_t)j];
    N.epx = ep[2 * j]; N.epy = ep[2 * j + 1]; N.n_left2 = n_left2[j];
    TriKb8Consts &C = consts[(size_t)j];
    for (int p = 0; p < (rig ? 4 : 1); p++) {
      memcpy(C.T12[p], T12 + 48 * (size_t)j + 12 * p, sizeof(C.T12[p]));
      rig_Tcw2(C.T12[p], C.Tcw2[p]);
    }
    memcpy(C.cams1, cams1, sizeof(float) * (rig ? 16 : 8));
    memcpy(C.cams2, cams2 + 16 * (size_t)j, sizeof(float) * (rig ? 16 : 8));
  }
  return 0;
}

int orbm_search_for_triangulation_kb8_neighbours(orbm_t *m, const orbm_keyframe_t *k1, int n_left1, int K, const orbm_keyframe_t *k2, const int32_t *n_left2,
                                                 const float *ep, const float *cams1, const float *cams2, const float *T12, const uint8_t *skip,
                                                 int bOnlyStereo, int bCoarse, int32_t *matches12, int32_t *nmatches) {
  if (!m || !k1) return ORBX_E_ARG;
  const bool rig = n_left1 != -1;
  const Refuse refuse{m, "neighbour"};
  if (n_left1 < -1 || (k1->n >= 0 && n_left1 > k1->n)) return refuse(-1, "kf1: n_left out of range");
  const int rr = triangulation_neighbours_refusal(m, k1, rig, true, K, k2, skip);
  if (rr < 0) return rr;
  if (K > 0 && (!matches12 || !nmatches)) return refuse(-1, "NULL result table");
  std::vector<TriNb> nb;
  std::vector<TriKb8Consts> consts;
  { const int rt = kb8_neighbour_tables(refuse, rr, rig, K, k2, n_left2, ep, cams1, cams2, T12, skip, nb, consts); if (rt < 0) return rt; }
  return triangulation_neighbours(m, "neighbour", k1, n_left1, K, k2, skip, nb, &consts, bOnlyStereo, bCoarse, matches12, nmatches);
}

// ---- The pair forms (ORBmatcher.cc:981-1222) --------------------------------------------------------------------------------------
// Pinhole: its own kernel with F12, the epipole and the scale tables by value.  (Served as the K = 1 call of the one-call form it
// measured 2 to 6 % slower per call, profiles/host_layer_bench.txt; the KannalaBrandt8 form below did not.)
int orbm_search_for_triangulation(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_t *k2, const float *R1w, const float *t1w,
                                  const float *R2w, const float *t2w, const float *Cw1, const float *cam1, const float *cam2,
                                  int bOnlyStereo, int bCoarse, int checkOri, int32_t *matches12) {
  if (!m || !k1 || !k2 || !R1w || !t1w || !R2w || !t2w || !Cw1 || !cam1 || !cam2 || !matches12) return ORBX_E_ARG;
  if (k1->n < 0 || k2->n < 0 || k2->nlevels < 1 || k2->nlevels > ORBX_MAX_LEVELS) return ORBX_E_ARG;
  for (int i = 0; i < k1->n; i++) matches12[i] = -1;
  if (k1->n == 0 || k2->n == 0 || k1->n_nodes == 0 || k2->n_nodes == 0) return 0;
  if (!k1->u_right || !k2->u_right || !k1->has_mappoint || !k2->has_mappoint) return ORBX_E_ARG;
  TriParams T;
  memset(&T, 0, sizeof(T));
  pinhole_pair_geometry(R1w, t1w, R2w, t2w, Cw1, cam1, cam2, T.F12, T.epx, T.epy);
  std::vector<TriItem> items;
  { const int rc = triangulation_items(m, k1, k2, k1->u_right, bOnlyStereo, items); if (rc < 0) return rc; }
  int nmatches = 0;
  if (!items.empty()) {
    MCHECK(m, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const size_t n1 = (size_t)k1->n, n2 = (size_t)k2->n;
    Staging S{m};
    const auto KP1 = S.add(k1->keys_un, n1);
    const auto DESC1 = S.add(k1->descriptors, 32 * n1);
    const auto UR1 = S.add(k1->u_right, n1);
    const auto DESC2 = S.add(k2->descriptors, 32 * n2);
    const auto KP2 = S.add(k2->keys_un, n2);
    const auto UR2 = S.add(k2->u_right, n2);
    const auto HASMP2 = S.add(k2->has_mappoint, n2);
    const auto NODE_IDX2 = S.add(k2->node_idx, (size_t)k2->node_start[k2->n_nodes]);
    const auto ITEMS = S.add(items.data(), items.size());
    const auto MATCHES12 = S.out<int32_t>(n1);
    const int rs = S.upload(s, false);
    if (rs < 0) return rs;
    MCHECK(m, S.fill(s, MATCHES12, MATCHES12, 0xff));
    T.kp1 = (const float *)S.dev(KP1); T.desc1 = (const uint32_t *)S.dev(DESC1); T.ur1 = S.dev(UR1);
    T.desc2 = (const uint32_t *)S.dev(DESC2); T.kp2 = (const float *)S.dev(KP2); T.ur2 = S.dev(UR2);
    T.hasmp2 = S.dev(HASMP2); T.node_idx2 = S.dev(NODE_IDX2);
    T.items = S.dev(ITEMS); T.nitems = (int)items.size();
    for (int l = 0; l < k2->nlevels; l++) { T.sf2[l] = k2->scale_factors[l]; T.sigma2_2[l] = k2->level_sigma2[l]; }
    T.bOnlyStereo = bOnlyStereo; T.bCoarse = bCoarse;
    T.matches12 = S.dev(MATCHES12);
    hipLaunchKernelGGL(k_triangulation_match, dim3((T.nitems + 3) / 4), dim3(256), 0, s, T);
    MCHECK(m, hipGetLastError());
    MCHECK(m, hipMemcpyAsync(matches12, S.dev(MATCHES12), sizeof(int32_t) * n1, hipMemcpyDeviceToHost, s));
    MCHECK(m, hipStreamSynchronize(s));
    for (int i = 0; i < k1->n; i++) nmatches += matches12[i] >= 0;
  }
  if (checkOri && nmatches > 0) nmatches = prune_pairs_by_rotation(k1, k2, matches12, nmatches);
  return nmatches;
}

// KannalaBrandt8: the one-call search with K = 1 behind the entry's own front checks (no "neighbour 0: " in m->err), then the rotation
// histogram.
int orbm_search_for_triangulation_kb8(orbm_t *m, const orbm_keyframe_t *k1, int n_left1, const orbm_keyframe_t *k2, int n_left2, float ep_x, float ep_y,
                                      const float *cams1, const float *cams2, const float *T12, int bOnlyStereo, int bCoarse, int checkOri,
                                      int32_t *matches12) {
  if (!m || !k1 || !k2 || !cams1 || !cams2 || !T12 || !matches12) return ORBX_E_ARG;
  const bool rig = n_left1 != -1;
  const Refuse refuse{m, nullptr};
  if ((n_left1 == -1) != (n_left2 == -1)) return refuse(-1, "n_left: one keyframe with and one without a second camera");
  if (k1->n < 0 || k2->n < 0 || n_left1 < -1 || n_left1 > k1->n || n_left2 < -1 || n_left2 > k2->n) return refuse(-1, "n or n_left out of range");
  if (k1->nlevels < 1 || k1->nlevels > ORBX_MAX_LEVELS || k2->nlevels < 1 || k2->nlevels > ORBX_MAX_LEVELS) return refuse(-1, "nlevels out of range");
  for (const orbm_keyframe_t *k : {k1, k2})
    if (const char *why = tri_keyframe_refusal(k, rig)) return refuse(-1, why);
  for (int i = 0; i < k1->n; i++) matches12[i] = -1;
  if (k1->n == 0 || k2->n == 0 || k1->n_nodes == 0 || k2->n_nodes == 0) return 0;
  if (const char *why = tri_members_refusal(k2)) return refuse(-1, why);
  const int32_t nl2 = n_left2;
  const float ep[2] = {ep_x, ep_y};
  std::vector<TriNb> nb;
  std::vector<TriKb8Consts> consts;
  { const int rt = kb8_neighbour_tables(refuse, 0, rig, 1, k2, &nl2, ep, cams1, cams2, T12, nullptr, nb, consts); if (rt < 0) return rt; }
  const int nmatches = triangulation_neighbours(m, nullptr, k1, n_left1, 1, k2, nullptr, nb, &consts, bOnlyStereo, bCoarse, matches12, nullptr);
  return checkOri && nmatches > 0 ? prune_pairs_by_rotation(k1, k2, matches12, nmatches) : nmatches;
}

// ---- LocalMapping::CreateNewMapPoints: the searches and the body of the loop (LocalMapping.cc:470-905) -----------------------------
// A keyframe's constants as the body reads them (csrc/orb_ref_newpoints.h); cams: mvParameters of mpCamera, behind them mpCamera2's
static void new_point_camera(orbm_new_point_camera_t &c, const orbm_keyframe_t &k, const orbm_keyframe_geometry_t &g, int cam_type, const float *cams,
                             int n_left) {
  memset(&c, 0, sizeof(c));
  const bool rig = n_left != -1;
  const int np = cam_type == 0 ? 4 : 8;
  memcpy(c.Tcw[0], g.Tcw, sizeof(c.Tcw[0]));
  memcpy(c.Ow[0], g.Ow, sizeof(c.Ow[0]));
  memcpy(c.cam[0], cams, sizeof(float) * (size_t)np);
  if (rig) {
    memcpy(c.Tcw[1], g.Tcw_right, sizeof(c.Tcw[1]));
    memcpy(c.Ow[1], g.Ow_right, sizeof(c.Ow[1]));
    memcpy(c.cam[1], cams + 8, sizeof(float) * (size_t)np);
  }
  if (g.Twc) memcpy(c.Twc, g.Twc, sizeof(c.Twc));
  c.fx = g.fx; c.fy = g.fy; c.cx = g.cx; c.cy = g.cy; c.invfx = g.invfx; c.invfy = g.invfy; c.mb = g.mb; c.mbf = g.mbf;
  for (int l = 0; l < k.nlevels && l < ORBX_MAX_LEVELS; l++) { c.sf[l] = k.scale_factors[l]; c.sigma2[l] = k.level_sigma2[l]; }
  c.cam_type = cam_type; c.n_left = n_left;
}

static bool fill_new_point_pairs(NewPointPairsParams &P, int n, const orbm_new_point_camera_t *c1, const orbm_new_point_camera_t *c2,
                                 const orbm_new_point_obs_t *obs1, const orbm_new_point_obs_t *obs2, float scale_factor1, int far_points,
                                 float th_far_points, uint8_t *status, float *x3D) {
  if (n < 0 || !c1 || !c2 || (n > 0 && (!obs1 || !obs2 || !status || !x3D))) return false;
  if (c1->cam_type < 0 || c1->cam_type > 1 || c2->cam_type < 0 || c2->cam_type > 1) return false;
  P.c1 = *c1; P.c2 = *c2; P.obs1 = obs1; P.obs2 = obs2; P.scale_factor1 = scale_factor1; P.th_far_points = th_far_points;
  P.far_points = far_points; P.n = n; P.status = status; P.x3d = x3D;
  return true;
}

int orbm_new_point_geometry(int n, const orbm_new_point_camera_t *c1, const orbm_new_point_camera_t *c2, const orbm_new_point_obs_t *obs1,
                            const orbm_new_point_obs_t *obs2, float scale_factor1, int far_points, float th_far_points, uint8_t *status, float *x3D) {
  NewPointPairsParams P;
  if (!fill_new_point_pairs(P, n, c1, c2, obs1, obs2, scale_factor1, far_points, th_far_points, status, x3D)) return ORBX_E_ARG;
  for (int i = 0; i < n; i++)
    status[i] = (uint8_t)new_point_geometry(P.c1, P.c2, obs1[i], obs2[i], scale_factor1, far_points, th_far_points, x3D + 3 * (size_t)i);
  return 0;
}

int orbm_new_point_geometry_device(int n, const orbm_new_point_camera_t *c1, const orbm_new_point_camera_t *c2, const orbm_new_point_obs_t *d_obs1,
                                   const orbm_new_point_obs_t *d_obs2, float scale_factor1, int far_points, float th_far_points, uint8_t *d_status,
                                   float *d_x3D, void *stream) {
  NewPointPairsParams P;
  if (!fill_new_point_pairs(P, n, c1, c2, d_obs1, d_obs2, scale_factor1, far_points, th_far_points, d_status, d_x3D)) return ORBX_E_ARG;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_new_point_pairs, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

// What the body needs of keyframe (k, g) beyond the search's arrays, or NULL
static const char *new_points_keyframe_refusal(const orbm_keyframe_t &k, const orbm_keyframe_geometry_t &g, bool rig) {
  if (!g.Tcw || !g.Ow || (rig && (!g.Tcw_right || !g.Ow_right))) return "NULL pose";
  if (!rig && (!g.depth || !g.keys || !g.Twc))
    for (int i = 0; i < k.n; i++)
      if (k.u_right[i] >= 0) return "NULL mvDepth, mvKeys or Twc";
  return nullptr;
}

// The refusals the two forms share behind those of the search (rr = triangulation_neighbours_refusal's answer) and the empty outputs
static int new_points_refusal(orbm_t *m, int rr, const orbm_keyframe_t *k1, const orbm_keyframe_geometry_t *g1, bool rig, int K,
                              const orbm_keyframe_t *k2, const orbm_keyframe_geometry_t *g2, const uint8_t *skip, orbm_new_point_t *points, int cap,
                              uint8_t *status, int32_t *matches12, int32_t *nmatches) {
  const Refuse refuse{m, "neighbour"};
  if (cap < 0 || (cap > 0 && !points)) return refuse(-1, "NULL point list or cap < 0");
  if (nmatches && !matches12) return refuse(-1, "nmatches without matches12");
  if (rr == 0) {
    if (!g1 || !g2) return refuse(-1, "NULL keyframe geometry table");
    if (const char *why = new_points_keyframe_refusal(*k1, *g1, rig)) return refuse(-1, (std::string("kf1: ") + why).c_str());
    for (int j = 0; j < K; j++)
      if (!(skip && skip[j]))
        if (const char *why = new_points_keyframe_refusal(k2[j], g2[j], rig)) return refuse(j, why);
  }
  if (status && K > 0) memset(status, ORBM_NP_NO_MATCH, (size_t)K * (size_t)k1->n);
  return 0;
}

static int new_points_result(const NewPointsCall &np, orbm_new_point_t *points, int cap) {
  const size_t count = np.list.size();
  if (count <= (size_t)cap && count) memcpy(points, np.list.data(), sizeof(orbm_new_point_t) * count);
  return (int)count;
}

int orbm_create_new_map_points(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_geometry_t *g1, float scale_factor1, int K,
                               const orbm_keyframe_t *k2, const orbm_keyframe_geometry_t *g2, const float *R1w, const float *t1w, const float *Cw1,
                               const float *cam1, const float *R2w, const float *t2w, const float *cam2, const uint8_t *skip, int bCoarse,
                               int far_points, float th_far_points, orbm_new_point_t *points, int cap, uint8_t *status, int32_t *matches12,
                               int32_t *nmatches) {
  if (!m || !k1) return ORBX_E_ARG;
  const int rr = triangulation_neighbours_refusal(m, k1, false, false, K, k2, skip);
  if (rr < 0) return rr;
  if (rr == 0 && (!R1w || !t1w || !Cw1 || !cam1 || !R2w || !t2w || !cam2)) { m->err = "NULL pose or camera table"; return ORBX_E_ARG; }
  if (rr == 0 && (k1->nlevels < 1 || k1->nlevels > ORBX_MAX_LEVELS)) { m->err = "kf1: nlevels out of range"; return ORBX_E_ARG; }
  if (rr == 0)   // the body reads kf1's scale tables, which Pinhole's search does not
    if (const char *why = tri_keyframe_refusal(k1, false, true)) { m->err = std::string("kf1: ") + why; return ORBX_E_ARG; }
  { const int rn = new_points_refusal(m, rr, k1, g1, false, K, k2, g2, skip, points, cap, status, matches12, nmatches); if (rn < 0) return rn; }
  std::vector<TriNb> nb((size_t)K);
  if (K > 0) memset(nb.data(), 0, sizeof(TriNb) * (size_t)K);
  for (int j = 0; j < K && rr == 0; j++)
    if (!(skip && skip[j])) pinhole_pair_geometry(R1w, t1w, R2w + 9 * j, t2w + 3 * j, Cw1, cam1, cam2 + 4 * j, nb[(size_t)j].F12, nb[(size_t)j].epx, nb[(size_t)j].epy);
  NewPointsCall np{g1, g2, 0, cam1, cam2, 4, nullptr, scale_factor1, th_far_points, far_points, status, {}};
  const int rc = triangulation_neighbours(m, "neighbour", k1, -1, K, k2, skip, nb, nullptr, 0, bCoarse, matches12, nmatches, &np);
  return rc < 0 ? rc : new_points_result(np, points, cap);
}

int orbm_create_new_map_points_kb8(orbm_t *m, const orbm_keyframe_t *k1, const orbm_keyframe_geometry_t *g1, float scale_factor1, int n_left1, int K,
                                   const orbm_keyframe_t *k2, const orbm_keyframe_geometry_t *g2, const int32_t *n_left2, const float *ep,
                                   const float *cams1, const float *cams2, const float *T12, const uint8_t *skip, int bCoarse, int far_points,
                                   float th_far_points, orbm_new_point_t *points, int cap, uint8_t *status, int32_t *matches12, int32_t *nmatches) {
  if (!m || !k1) return ORBX_E_ARG;
  const bool rig = n_left1 != -1;
  const Refuse refuse{m, "neighbour"};
  if (n_left1 < -1 || (k1->n >= 0 && n_left1 > k1->n)) return refuse(-1, "kf1: n_left out of range");
  const int rr = triangulation_neighbours_refusal(m, k1, rig, true, K, k2, skip);
  if (rr < 0) return rr;
  std::vector<TriNb> nb;
  std::vector<TriKb8Consts> consts;
  { const int rt = kb8_neighbour_tables(refuse, rr, rig, K, k2, n_left2, ep, cams1, cams2, T12, skip, nb, consts); if (rt < 0) return rt; }
  { const int rn = new_points_refusal(m, rr, k1, g1, rig, K, k2, g2, skip, points, cap, status, matches12, nmatches); if (rn < 0) return rn; }
  NewPointsCall np{g1, g2, 1, cams1, cams2, 16, n_left2, scale_factor1, th_far_points, far_points, status, {}};
  const int rc = triangulation_neighbours(m, "neighbour", k1, n_left1, K, k2, skip, nb, &consts, 0, bCoarse, matches12, nmatches, &np);
  return rc < 0 ? rc : new_points_result(np, points, cap);
}

int orbm_search_for_initialization(orbm_t *m, const orbm_frame_t *f1, const orbm_frame_t *f2, float *prev_matched, int window_size,
                                   float nnratio, int checkOri, int32_t *matches12) {
  if (!m || !f1 || !f2 || !matches12 || f1->n < 0 || f2->n < 0) return ORBX_E_ARG;
  if (f1->n > 0 && (!f1->keys_un || !f1->descriptors || !prev_matched)) return ORBX_E_ARG;
  const int n1 = f1->n;
  for (int i = 0; i < n1; i++) matches12[i] = -1;                 // :725
  // queries: the level-0 keypoints of F1 in index order (:737-739), window centre = vbPrevMatched (:741)
  std::vector<int32_t> qi;
  for (int i = 0; i < n1; i++)
    if (f1->keys_un[i].octave <= 0) qi.push_back(i);
  const int nq = (int)qi.size();
  if (nq == 0 || f2->n == 0) return 0;
  std::vector<float> u(nq), v(nq), rad(nq, (float)window_size);
  std::vector<int32_t> lvl(nq, 0), acc(nq, -1);
  std::vector<uint8_t> qd((size_t)nq * 32);
  for (int k = 0; k < nq; k++) {
    u[k] = prev_matched[2 * qi[k]]; v[k] = prev_matched[2 * qi[k] + 1];
    memcpy(&qd[(size_t)k * 32], f1->descriptors + (size_t)qi[k] * 32, 32);
  }
  orbm_queries_t q;
  q.nq = nq; q.descriptors = qd.data(); q.u = u.data(); q.v = v.data(); q.radius = rad.data();
  q.min_level = lvl.data(); q.max_level = lvl.data();             // GetFeaturesInArea(..., level1, level1), level1 == 0
  q.u_r = nullptr; q.flags = nullptr;
  orbm_frame_t f = *f2;
  f.u_right = nullptr;
  std::vector<int32_t> slot((size_t)f2->n, -1);
  std::vector<uint8_t> sobs((size_t)f2->n, 0);
  SearchOpts o;
  o.nleft.konst = f2->n; o.init_th_low = ORBM_TH_LOW;
  const int rc = search_host(m, &f, &q, nnratio, ORBM_TH_LOW, 1, slot.data(), sobs.data(), acc.data(), nullptr, o);
  if (rc < 0) return rc;
  // replay of the bookkeeping the device leaves to the host: steals (:781-785) and the rotation histogram (:791-801)
  int nmatches = 0;
  std::vector<int32_t> m21((size_t)f2->n, -1);
  RotHist H;
  for (int k = 0; k < nq; k++) {
    const int i2 = acc[k];
    if (i2 < 0) continue;
    const int i1 = qi[k];
    if (m21[i2] >= 0) { matches12[m21[i2]] = -1; nmatches--; }
    matches12[i1] = i2; m21[i2] = i1; nmatches++;
    if (checkOri) H.add(f1->keys_un[i1].angle - f2->keys_un[i2].angle, i1);
  }
  if (checkOri)   // a stolen match stays in its bin (it counts for the maxima) and is skipped here, :815-819
    H.for_each_pruned([&](int idx1) { if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; } });
  for (int i = 0; i < n1; i++)                                     // :826-828
    if (matches12[i] >= 0) { prev_matched[2 * i] = f2->keys_un[matches12[i]].x; prev_matched[2 * i + 1] = f2->keys_un[matches12[i]].y; }
  return nmatches;
}

// ---- ComputeStereoMatches: what the two entry points ask of a pair of extractors -----------------------------------------------
// Same device, image size and pyramid depth; same_scale: also the same scale factors, which the batch form asks for and the host
// form never did (it goes on accepting what it accepted).
static int stereo_check_pair(orbx_t *hl, orbx_t *hr, const char *what, bool same_scale) {
  if (hl->device != hr->device || hl->rows != hr->rows || hl->cols != hr->cols || hl->nlevels != hr->nlevels ||
      (same_scale && hl->mvScaleFactor != hr->mvScaleFactor)) {
    hl->err = std::string(what) + ": the two extractors must share device, image size and pyramid";
    return ORBX_E_ARG;
  }
  return 0;
}

int orbx_compute_stereo_matches(orbx_t *hl, int frame_l, orbx_t *hr, int frame_r, int nL, const orbx_keypoint_t *keysL,
                                const uint8_t *descL, int nR, const orbx_keypoint_t *keysR, const uint8_t *descR, float mb, float mbf,
                                float *uRight, float *depth) {
  if (!hl || !hr || nL < 0 || nR < 0 || !uRight || !depth) return ORBX_E_ARG;
  if (!hl->have_last || !hr->have_last) { hl->err = "orbx_compute_stereo_matches: extract both images first"; return ORBX_E_ARG; }
  if (frame_l < 0 || frame_l >= hl->last.nframes || frame_r < 0 || frame_r >= hr->last.nframes) return ORBX_E_ARG;
  if (stereo_check_pair(hl, hr, "orbx_compute_stereo_matches", false) < 0) return ORBX_E_ARG;
  for (int i = 0; i < nL; i++) { uRight[i] = -1.0f; depth[i] = -1.0f; }   // Frame.cc:903-904
  if (nL == 0 || nR == 0) return 0;
  if (!keysL || !descL || !keysR || !descR || nR > 65535) return ORBX_E_ARG;
  if (!(mb > 0.f)) return ORBX_E_ARG;
  XCHECK(hl, hipSetDevice(hl->device));
  hipStream_t s = hl->stream;
  // the two extractions may have run on any stream (the handles' own, or the caller's with orbx_extract_batch_device): the
  // search is ordered behind the last kernel of both; level 0 is read in place from the caller's images (orbhip.h)
  if (hl->last_pending) XCHECK(hl, hipStreamWaitEvent(s, hl->last_done, 0));
  if (hr->last_pending) XCHECK(hl, hipStreamWaitEvent(s, hr->last_done, 0));
  DevBuf *bufs = hl->stereo;
  const size_t sz[7] = {sizeof(orbx_keypoint_t) * (size_t)nL, sizeof(orbx_keypoint_t) * (size_t)nR, 32 * (size_t)nL, 32 * (size_t)nR,
                        sizeof(float) * (size_t)nL, sizeof(float) * (size_t)nL, sizeof(int32_t) * (size_t)nL};
  const void *src[4] = {keysL, keysR, descL, descR};
  for (int i = 0; i < 7; i++) XCHECK(hl, bufs[i].reserve(sz[i]));
  for (int i = 0; i < 4; i++) XCHECK(hl, hipMemcpyAsync(bufs[i].p, src[i], sz[i], hipMemcpyHostToDevice, s));
  StereoParams S;
  memset(&S, 0, sizeof(S));
  S.imgL0 = hl->last.img0 + (size_t)frame_l * hl->last.img0_frame_stride; S.strideL0 = hl->last.img0_stride;
  S.imgR0 = hr->last.img0 + (size_t)frame_r * hr->last.img0_frame_stride; S.strideR0 = hr->last.img0_stride;
  S.pyrL = hl->last.pyr + (size_t)frame_l * hl->last.pyr_fs;
  S.pyrR = hr->last.pyr + (size_t)frame_r * hr->last.pyr_fs;
  fill_stereo_levels(hl, S);
  S.kpL = (const float *)bufs[0].p; S.kpR = (const float *)bufs[1].p;
  S.descL = (const uint32_t *)bufs[2].p; S.descR = (const uint32_t *)bufs[3].p;
  S.nL = nL; S.nR = nR; S.mb = mb; S.mbf = mbf;
  S.uRight = (float *)bufs[4].p; S.depth = (float *)bufs[5].p; S.sad = (int32_t *)bufs[6].p;
  hipLaunchKernelGGL(k_stereo_match, dim3((nL + 3) / 4), dim3(256), 0, s, S);
  XCHECK(hl, hipGetLastError());
  std::vector<int32_t> sad((size_t)nL);
  XCHECK(hl, hipMemcpyAsync(uRight, bufs[4].p, sz[4], hipMemcpyDeviceToHost, s));
  XCHECK(hl, hipMemcpyAsync(depth, bufs[5].p, sz[5], hipMemcpyDeviceToHost, s));
  XCHECK(hl, hipMemcpyAsync(sad.data(), bufs[6].p, sz[6], hipMemcpyDeviceToHost, s));
  XCHECK(hl, hipStreamSynchronize(s));
  // median filter over the accepted matches, Frame.cc:1060-1073 (an empty set - where the reference indexes an empty
  // vector - is defined as "nothing to do")
  std::vector<std::pair<int, int>> vDistIdx;
  for (int i = 0; i < nL; i++)
    if (sad[i] >= 0) vDistIdx.push_back(std::make_pair(sad[i], i));
  if (!vDistIdx.empty()) {
    std::sort(vDistIdx.begin(), vDistIdx.end());
    const float median = (float)vDistIdx[vDistIdx.size() / 2].first;
    const float thDist = 1.5f * 1.4f * median;
    for (int i = (int)vDistIdx.size() - 1; i >= 0; i--) {
      if ((float)vDistIdx[i].first < thDist) break;
      uRight[vDistIdx[i].second] = -1;
      depth[vDistIdx[i].second] = -1;
    }
  }
  return 0;
}

int orbx_compute_stereo_matches_batch_device(orbx_t *hl, orbx_t *hr, int nframes, const orbx_keypoint_t *d_keysL, const uint8_t *d_descL,
                                             const int32_t *d_countsL, const orbx_keypoint_t *d_keysR, const uint8_t *d_descR,
                                             const int32_t *d_countsR, int cap, float mb, float mbf, float *d_uRight, float *d_depth,
                                             int32_t *d_nstereo, void *stream_) {
  if (!hl || !hr) return ORBX_E_ARG;
  if (!d_keysL || !d_descL || !d_countsL || !d_keysR || !d_descR || !d_countsR || !d_uRight || !d_depth) {
    hl->err = "orbx_compute_stereo_matches_batch_device: NULL array";
    return ORBX_E_ARG;
  }
  if (!hl->have_last || !hr->have_last) { hl->err = "orbx_compute_stereo_matches_batch_device: extract both batches first"; return ORBX_E_ARG; }
  if (nframes <= 0 || nframes > hl->last.nframes || nframes > hr->last.nframes) {
    hl->err = "orbx_compute_stereo_matches_batch_device: nframes outside the two extractors' last batches";
    return ORBX_E_ARG;
  }
  if (stereo_check_pair(hl, hr, "orbx_compute_stereo_matches_batch_device", true) < 0) return ORBX_E_ARG;
  if (!(mb > 0.f)) { hl->err = "orbx_compute_stereo_matches_batch_device: mb must be positive"; return ORBX_E_ARG; }
  if (cap < hl->maxKeypoints || cap < hr->maxKeypoints || cap > 65535) {
    hl->err = "orbx_compute_stereo_matches_batch_device: cap must be in [orbx_max_keypoints, 65535]";
    return ORBX_E_ARG;
  }
  XCHECK(hl, hipSetDevice(hl->device));
  hipStream_t s = (hipStream_t)stream_;   // verbatim: NULL is the device's default stream
  StereoBatchParams S;
  memset(&S, 0, sizeof(S));
  S.imgL0 = hl->last.img0; S.strideL0 = hl->last.img0_stride; S.fsL0 = hl->last.img0_frame_stride;
  S.imgR0 = hr->last.img0; S.strideR0 = hr->last.img0_stride; S.fsR0 = hr->last.img0_frame_stride;
  S.pyrL = hl->last.pyr; S.pyrFsL = hl->last.pyr_fs;
  S.pyrR = hr->last.pyr; S.pyrFsR = hr->last.pyr_fs;
  fill_stereo_levels(hl, S);
  float sfMax = 0.f;
  for (int l = 0; l < S.nlevels; l++) sfMax = std::max(sfMax, S.sf[l]);
  S.nbands = (hl->rows + STEREO_BAND - 1) / STEREO_BAND;
  if (S.nbands > STEREO_MAX_BANDS) { hl->err = "orbx_compute_stereo_matches_batch_device: more than 4096 rows"; return ORBX_E_ARG; }
  // a right keypoint covers the rows floor(y - r) .. ceil(y + r), r = 2 * scale (:916-918): at most 2r + 3 of them (+ 1 for the
  // rounding of y +- r), and S consecutive rows touch at most (S + 6) / 8 + 1 bands of 8
  const int spanRows = (int)(4.0f * sfMax) + 4;
  const int bandsPerKp = std::min(S.nbands, (spanRows + 6) / STEREO_BAND + 1);
  S.cap = cap; S.recCap = cap * bandsPerKp;
  S.kpL = (const float *)d_keysL; S.kpR = (const float *)d_keysR;
  S.descL = (const uint32_t *)d_descL; S.descR = (const uint32_t *)d_descR;
  S.countsL = d_countsL; S.countsR = d_countsR;
  S.mb = mb; S.mbf = mbf;
  DevBuf *bufs = hl->stereo_batch;   // grow-only; a growth is the one step that blocks (hipFree / hipMalloc)
  XCHECK(hl, bufs[0].reserve(sizeof(StereoRec) * (size_t)S.recCap * nframes));
  XCHECK(hl, bufs[1].reserve(sizeof(int32_t) * (size_t)(S.nbands + 1) * nframes));
  XCHECK(hl, bufs[2].reserve(sizeof(int32_t) * (size_t)cap * nframes));
  S.recs = (StereoRec *)bufs[0].p; S.bandStart = (int32_t *)bufs[1].p; S.sad = (int32_t *)bufs[2].p;
  S.uRight = d_uRight; S.depth = d_depth; S.nstereo = d_nstereo;
  // the two extractions may have run on any stream: ordered behind the last kernel of both, as the host form does
  if (hl->last_pending) XCHECK(hl, hipStreamWaitEvent(s, hl->last_done, 0));
  if (hr->last_pending) XCHECK(hl, hipStreamWaitEvent(s, hr->last_done, 0));
  hipLaunchKernelGGL(k_stereo_rows, dim3(nframes), dim3(256), 0, s, S);
  hipLaunchKernelGGL(k_stereo_search, dim3((cap + STEREO_KPB - 1) / STEREO_KPB, nframes), dim3(256), 0, s, S);
  hipLaunchKernelGGL(k_stereo_median, dim3(nframes), dim3(256), 0, s, S);
  XCHECK(hl, hipGetLastError());
  return 0;
}

int orbx_stereo_from_rgbd_batch_device(int nframes, const orbx_keypoint_t *d_keys, const orbx_keypoint_t *d_keys_un, const int32_t *d_counts,
                                       int count_stride, int cap, const void *d_depth_image, int depth_type, int rows, int cols, size_t row_stride,
                                       size_t frame_stride, float depth_factor, float mbf, float *d_uRight, float *d_depth, int32_t *d_nstereo,
                                       void *stream) {
  if (!d_keys || !d_keys_un || !d_counts || !d_depth_image || !d_uRight || !d_depth) return ORBX_E_ARG;
  if (nframes < 0 || cap <= 0 || count_stride <= 0 || rows <= 0 || cols <= 0 || (depth_type != 0 && depth_type != 1)) return ORBX_E_ARG;
  const size_t elem = depth_type == 0 ? sizeof(uint16_t) : sizeof(float);
  if (row_stride < (size_t)cols * elem || row_stride % elem || frame_stride % elem) return ORBX_E_ARG;
  if (nframes > 1 && frame_stride < row_stride * (size_t)rows) return ORBX_E_ARG;
  if (nframes == 0) return 0;
  RgbdParams P;
  P.keys = reinterpret_cast<const float *>(d_keys); P.keys_un = reinterpret_cast<const float *>(d_keys_un);
  P.counts = d_counts; P.count_stride = count_stride; P.cap = cap;
  P.img = (const uint8_t *)d_depth_image; P.depth_type = depth_type; P.rows = rows; P.cols = cols; P.row_stride = row_stride; P.frame_stride = frame_stride;
  P.factor = depth_factor; P.mbf = mbf;
  P.uRight = d_uRight; P.depth = d_depth; P.nstereo = d_nstereo;
  hipLaunchKernelGGL(k_stereo_from_rgbd, dim3(nframes), dim3(256), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

int orbx_close_points_batch_device(int nframes, const float *d_depth, const int32_t *d_counts, int count_stride, int cap, float th_depth, int max_point,
                                   int32_t *d_order, int32_t *d_nvisit, const uint8_t *d_tracked, int32_t *d_close, const orbx_keypoint_t *d_keys_un,
                                   float fx, float fy, float cx, float cy, float *d_x3Dc, const float *d_pose, float *d_x3Dw, void *stream) {
  if (!d_depth || !d_counts || !d_order || !d_nvisit) return ORBX_E_ARG;
  if (nframes < 0 || cap <= 0 || cap > ORBX_CLOSE_MAX_KEYPOINTS || count_stride <= 0) return ORBX_E_ARG;
  if ((d_x3Dc && !d_keys_un) || (d_x3Dw && (!d_x3Dc || !d_pose)) || (d_pose && !d_x3Dw)) return ORBX_E_ARG;
  if (nframes == 0) return 0;
  CloseParams P;
  P.depth = d_depth; P.counts = d_counts; P.count_stride = count_stride; P.cap = cap;
  P.th_depth = th_depth; P.max_point = max_point; P.tracked = d_tracked;
  P.order = d_order; P.nvisit = d_nvisit; P.close = d_close;
  P.keys_un = reinterpret_cast<const float *>(d_keys_un); P.cx = cx; P.cy = cy;
  P.invfx = 1.0f / fx; P.invfy = 1.0f / fy;   // Frame.cc:275-276
  P.x3Dc = d_x3Dc; P.pose = d_pose; P.x3Dw = d_x3Dw;
  hipLaunchKernelGGL(k_close_points, dim3(nframes), dim3(CLOSE_THREADS), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : ORBX_E_HIP;
}

// Shared by the two SearchByBoW overloads.  kf_kf: second operand is a keyframe (candidates need a good map point, strict
// threshold, result indexed by the first keyframe's keypoints: out[kf->n]); otherwise out[f->n] is indexed by frame keypoint.
static int bow_core(orbm_t *m, const orbm_keyframe_t *kf, const orbm_keyframe_t *f, float nnratio, int checkOri, bool kf_kf, int nleftF, int32_t *out) {
  if (!m || !kf || !f || !out || kf->n < 0 || f->n < 0) return ORBX_E_ARG;
  const int nout = kf_kf ? kf->n : f->n;
  for (int i = 0; i < nout; i++) out[i] = -1;                     // :277 / :852
  if (kf->n == 0 || f->n == 0 || kf->n_nodes <= 0 || f->n_nodes <= 0) return 0;
  if (!kf->descriptors || !f->descriptors || !kf->has_mappoint || !kf->node_id || !f->node_id || !kf->node_start || !f->node_start ||
      !kf->node_idx || !f->node_idx || !kf->keys_un || !f->keys_un || (kf_kf && !f->has_mappoint)) return ORBX_E_ARG;
  // merge-walk of the two feature vectors (:292-296, :440-447): one work item per shared node
  std::vector<BowItem> items;
  int a = 0, b = 0;
  while (a < kf->n_nodes && b < f->n_nodes) {
    if (kf->node_id[a] == f->node_id[b]) {
      const int lk = kf->node_start[a + 1] - kf->node_start[a], lf = f->node_start[b + 1] - f->node_start[b];
      if (lf > 2048) { m->err = "SearchByBoW: more than 2048 keypoints of the second operand in one vocabulary node"; return ORBX_E_ARG; }
      if (lk > 0 && lf > 0) items.push_back(BowItem{kf->node_start[a], lk, f->node_start[b], lf});
      a++; b++;
    } else if (kf->node_id[a] < f->node_id[b]) {
      while (a < kf->n_nodes && kf->node_id[a] < f->node_id[b]) a++;   // lower_bound
    } else {
      while (b < f->n_nodes && f->node_id[b] < kf->node_id[a]) b++;
    }
  }
  if (items.empty()) return 0;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t nidxKF = (size_t)kf->node_start[kf->n_nodes], nidxF = (size_t)f->node_start[f->n_nodes];
  const size_t out_bytes = sizeof(int32_t) * (size_t)nout;
  Staging S{m};
  const auto DESC_KF = S.add(kf->descriptors, 32 * (size_t)kf->n), DESC_F = S.add(f->descriptors, 32 * (size_t)f->n);
  const auto HASMP_KF = S.add(kf->has_mappoint, (size_t)kf->n);
  const auto NODE_IDX_KF = S.add(kf->node_idx, nidxKF), NODE_IDX_F = S.add(f->node_idx, nidxF);
  const auto ITEMS = S.add(items.data(), items.size());
  const auto OUT = S.add((const int32_t *)out, (size_t)nout);   // uploaded: the rows start at the caller's -1
  const auto HASMP_F = S.add(f->has_mappoint, kf_kf ? (size_t)f->n : 0);
  const int rs = S.upload(s, false);
  if (rs < 0) return rs;
  BowParams B;
  memset(&B, 0, sizeof(B));
  B.descKF = (const uint32_t *)S.dev(DESC_KF); B.descF = (const uint32_t *)S.dev(DESC_F); B.hasmpKF = S.dev(HASMP_KF);
  B.node_idxKF = S.dev(NODE_IDX_KF); B.node_idxF = S.dev(NODE_IDX_F);
  B.items = S.dev(ITEMS); B.nitems = (int)items.size();
  B.nnratio = nnratio;
  B.nleftF = nleftF >= 0 ? nleftF : 0x7fffffff;
  if (kf_kf) { B.match12 = S.dev(OUT); B.hasmpF = S.dev(HASMP_F); B.strict = 1; }
  else B.matchF = S.dev(OUT);
  hipLaunchKernelGGL(k_bow_match, dim3((B.nitems + 3) / 4), dim3(256), 0, s, B);
  MCHECK(m, hipGetLastError());
  MCHECK(m, hipMemcpyAsync(out, S.dev(OUT), out_bytes, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipStreamSynchronize(s));
  int nmatches = 0;
  for (int i = 0; i < nout; i++) nmatches += out[i] >= 0 ? 1 : 0;
  if (!checkOri) return nmatches;
  // rotation histogram (:391-404, :451-466 resp. :929-939, :960-975): bins hold the index `out` is addressed with
  RotHist H;
  for (int i = 0; i < nout; i++) {
    if (out[i] < 0) continue;
    const int idxKF = kf_kf ? i : out[i], idxF = kf_kf ? out[i] : i;
    H.add(kf->keys_un[idxKF].angle - f->keys_un[idxF].angle, i);
  }
  H.for_each_pruned([&](int idx) { out[idx] = -1; nmatches--; });
  return nmatches;
}

int orbm_search_by_bow(orbm_t *m, const orbm_keyframe_t *kf, const orbm_keyframe_t *f, float nnratio, int checkOri, int32_t *matchF) {
  return bow_core(m, kf, f, nnratio, checkOri, false, -1, matchF);
}

int orbm_search_by_bow_fisheye(orbm_t *m, const orbm_keyframe_t *kf, const orbm_keyframe_t *f, int n_left_f, float nnratio, int checkOri,
                               int32_t *matchF) {
  if (n_left_f < 0 || (f && n_left_f > f->n)) return ORBX_E_ARG;
  return bow_core(m, kf, f, nnratio, checkOri, false, n_left_f, matchF);
}

int orbm_search_by_bow_keyframes(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_t *kf2, float nnratio, int checkOri,
                                 int32_t *matches12) {
  return bow_core(m, kf1, kf2, nnratio, checkOri, true, -1, matches12);
}

// ---- SearchByBoW of one frame or keyframe against K candidates in one call (Tracking.cc:3796-3816, LoopClosing.cc:724-739) ----------
// Shared by the two entries.  `fixed` is the operand every pair has: the frame (the SECOND operand of each pair, kf_kf false) or pKF1
// (the FIRST, kf_kf true); W / S below are a pair's walked and second operand as in bow_core.  Everything is validated before the
// outputs or the device are touched; then ONE staged block (the fixed operand once, the arrays of every candidate that shares a node,
// the records, the items), one fill of the rows, k_bow_match_candidates, k_bow_prune_candidates, one download of rows + counts.
static int bow_candidates(orbm_t *m, const orbm_keyframe_t *fixed, int K, const orbm_keyframe_t *cands, const uint8_t *skip, bool kf_kf,
                          int nleftF, float nnratio, int checkOri, int32_t *rows, int32_t *nmatches) {
  if (!m || !fixed) return ORBX_E_ARG;
  const Refuse refuse{m, "candidate"};
  if (K < 0) return refuse(-1, "K < 0");
  if (K > 0 && (!cands || !rows || !nmatches)) return refuse(-1, "NULL candidate or result table");
  if (fixed->n < 0) return refuse(-1, "fixed operand: n < 0");
  if (nleftF < -1 || nleftF > fixed->n) return refuse(-1, "n_left_f outside [-1, f->n]");
  const size_t nout = (size_t)fixed->n;
  std::vector<BowCandItem> &items = m->bow_items;
  std::vector<uint8_t> live((size_t)K, 0);
  items.clear();
  size_t nang = (size_t)fixed->n;
  for (int j = 0; j < K; j++) {
    if (skip && skip[j]) continue;                                 // isBad(): Tracking.cc:3799-3800, LoopClosing.cc:726-727
    const orbm_keyframe_t *c = &cands[j], *W = kf_kf ? fixed : c, *S = kf_kf ? c : fixed;
    if (c->n < 0) return refuse(j, "n < 0");
    if (W->n == 0 || S->n == 0 || W->n_nodes <= 0 || S->n_nodes <= 0) continue;
    if (!W->descriptors || !S->descriptors || !W->has_mappoint || !W->node_id || !S->node_id || !W->node_start || !S->node_start ||
        !W->node_idx || !S->node_idx || !W->keys_un || !S->keys_un || (kf_kf && !S->has_mappoint)) return refuse(j, "NULL array");
    for (const orbm_keyframe_t *k : {W, S}) {                      // the kernels index device memory with these
      if (k->node_start[0] < 0) return refuse(j, "feature vector: node_start negative");
      for (int f = 0; f < k->n_nodes; f++)
        if (k->node_start[f + 1] < k->node_start[f]) return refuse(j, "feature vector: node_start decreases");
    }
    const size_t before = items.size();
    int a = 0, b = 0;                                              // the merge walk of bow_core (:292-296, :440-447)
    while (a < W->n_nodes && b < S->n_nodes) {
      if (W->node_id[a] == S->node_id[b]) {
        const int sw = W->node_start[a], ss = S->node_start[b], lw = W->node_start[a + 1] - sw, ls = S->node_start[b + 1] - ss;
        if (ls > 2048) return refuse(j, "SearchByBoW: more than 2048 keypoints of the second operand in one vocabulary node");
        if (lw > 0 && ls > 0) {
          for (int i = 0; i < lw; i++)
            if (W->node_idx[sw + i] < 0 || W->node_idx[sw + i] >= W->n) return refuse(j, "feature vector: keypoint index out of range");
          for (int i = 0; i < ls; i++)
            if (S->node_idx[ss + i] < 0 || S->node_idx[ss + i] >= S->n) return refuse(j, "feature vector: keypoint index out of range");
          items.push_back(BowCandItem{j, sw, lw, ss, ls, {0, 0, 0}});
        }
        a++; b++;
      } else if (W->node_id[a] < S->node_id[b]) {
        while (a < W->n_nodes && W->node_id[a] < S->node_id[b]) a++;   // lower_bound
      } else {
        while (b < S->n_nodes && S->node_id[b] < W->node_id[a]) b++;
      }
    }
    if (items.size() > 0x7fffffffu) return refuse(-1, "more than 2^31 - 1 shared vocabulary nodes over all candidates");
    live[(size_t)j] = items.size() > before;
    if (live[(size_t)j]) nang += (size_t)c->n;
  }
  for (size_t i = 0; i < (size_t)K * nout; i++) rows[i] = -1;      // :277 / :852
  for (int j = 0; j < K; j++) nmatches[j] = 0;
  if (items.empty()) return 0;
  const size_t ni = items.size();
  // keypoint angles for the rotation histogram, packed out of mvKeysUn
  std::vector<float> &ang = m->bow_ang;
  ang.resize(checkOri ? nang : 0);
  size_t ang_at = 0;
  auto pack_angles = [&](const orbm_keyframe_t &k) -> const float * {
    if (!checkOri) return nullptr;
    float *p = ang.data() + ang_at;
    for (int i = 0; i < k.n; i++) p[i] = k.keys_un[i].angle;
    ang_at += (size_t)k.n;
    return p;
  };
  std::vector<BowCand> &rec = m->bow_cands;
  rec.resize((size_t)K);
  memset(rec.data(), 0, sizeof(BowCand) * (size_t)K);
  Staging S{m};
  const size_t nf = (size_t)fixed->n;
  const bool fixed_hasmp = kf_kf;                                  // the frame's map points are not read (:273-469)
  const size_t F_DESC = S.offset(S.add(fixed->descriptors, 32 * nf));
  const size_t F_HASMP = S.offset(S.add(fixed_hasmp ? fixed->has_mappoint : nullptr, fixed_hasmp ? nf : 0));
  const size_t F_IDX = S.offset(S.add(fixed->node_idx, (size_t)fixed->node_start[fixed->n_nodes]));
  const size_t F_ANG = S.offset(S.add(pack_angles(*fixed), checkOri ? nf : 0));
  for (int j = 0; j < K; j++) {
    if (!live[(size_t)j]) continue;
    const orbm_keyframe_t &c = cands[j];
    const size_t nc = (size_t)c.n;
    const size_t desc = S.offset(S.add(c.descriptors, 32 * nc)), hasmp = S.offset(S.add(c.has_mappoint, nc));
    const size_t idx = S.offset(S.add(c.node_idx, (size_t)c.node_start[c.n_nodes]));
    const size_t an = S.offset(S.add(pack_angles(c), checkOri ? nc : 0));
    BowCand &R = rec[(size_t)j];
    if (kf_kf) {
      R.descW = F_DESC; R.hasmpW = F_HASMP; R.node_idxW = F_IDX; R.angW = F_ANG;
      R.descS = desc; R.hasmpS = hasmp; R.node_idxS = idx; R.angS = an;
    } else {
      R.descW = desc; R.hasmpW = hasmp; R.node_idxW = idx; R.angW = an;
      R.descS = F_DESC; R.hasmpS = BOW_NO_HASMP; R.node_idxS = F_IDX; R.angS = F_ANG;
    }
    R.n_left = nleftF >= 0 ? nleftF : 0x7fffffff;
  }
  const auto RECS = S.add(rec.data(), (size_t)K);
  const auto ITEMS = S.add(items.data(), ni);
  const size_t rows_bytes = sizeof(int32_t) * (size_t)K * nout;
  const auto ROWS = S.out<int32_t>((size_t)K * nout), COUNTS = S.out<int32_t>((size_t)K);
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  { const int rs = S.upload(s); if (rs < 0) return rs; }
  MCHECK(m, S.fill(s, ROWS, ROWS, 0xff));
  BowCandParams B;
  memset(&B, 0, sizeof(B));
  B.block = S.block(); B.cands = S.dev(RECS); B.items = S.dev(ITEMS); B.nitems = (int)ni;
  B.nout = fixed->n; B.nnratio = nnratio; B.kf_kf = kf_kf ? 1 : 0; B.checkOri = checkOri ? 1 : 0;
  B.rows = S.dev(ROWS); B.nmatches = S.dev(COUNTS);
  hipLaunchKernelGGL(k_bow_match_candidates, dim3((unsigned)((ni + 3) / 4)), dim3(256), 0, s, B);
  MCHECK(m, hipGetLastError());
  hipLaunchKernelGGL(k_bow_prune_candidates, dim3((unsigned)K), dim3(256), 0, s, B);
  MCHECK(m, hipGetLastError());
  // rows and counts are adjacent parts of the block: one copy into the pinned mirror
  MCHECK(m, S.download(s, ROWS, COUNTS));
  MCHECK(m, hipStreamSynchronize(s));
  memcpy(rows, S.host(ROWS), rows_bytes);
  memcpy(nmatches, S.host(COUNTS), sizeof(int32_t) * (size_t)K);
  long long sum = 0;
  for (int j = 0; j < K; j++) sum += nmatches[j];
  return (int)std::min<long long>(sum, 0x7fffffff);
}

int orbm_search_by_bow_candidates(orbm_t *m, int K, const orbm_keyframe_t *kf, const orbm_keyframe_t *f, int n_left_f, const uint8_t *skip,
                                  float nnratio, int checkOri, int32_t *matchF, int32_t *nmatches) {
  return bow_candidates(m, f, K, kf, skip, false, n_left_f, nnratio, checkOri, matchF, nmatches);
}

int orbm_search_by_bow_keyframes_candidates(orbm_t *m, const orbm_keyframe_t *kf1, int K, const orbm_keyframe_t *kf2, const uint8_t *skip,
                                            float nnratio, int checkOri, int32_t *matches12, int32_t *nmatches) {
  return bow_candidates(m, kf1, K, kf2, skip, true, -1, nnratio, checkOri, matches12, nmatches);
}

int orbm_distinctive_descriptors(orbm_t *m, int nmp, const int32_t *start, const uint8_t *desc, int32_t *best) {
  if (!m || nmp < 0 || (nmp > 0 && (!start || !best))) return ORBX_E_ARG;
  if (nmp == 0) return 0;
  const int total = start[nmp];
  for (int i = 0; i < nmp; i++) {
    const int n = start[i + 1] - start[i];
    if (n < 0 || n > 64 * DISTINCT_MAXT) { m->err = "ComputeDistinctiveDescriptors: more than 1024 observations of one map point"; return ORBX_E_ARG; }
  }
  if (start[0] < 0 || (total > 0 && !desc)) return ORBX_E_ARG;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Staging S{m};
  const auto hdesc = S.add(desc, 32 * (size_t)total);
  const auto hstart = S.add(start, (size_t)nmp + 1);
  const auto hbest = S.out<int32_t>((size_t)nmp);
  const int rs = S.upload(s, false);
  if (rs < 0) return rs;
  hipLaunchKernelGGL(k_distinctive, dim3((nmp + 3) / 4), dim3(256), 0, s, (const uint32_t *)S.dev(hdesc), (const int32_t *)S.dev(hstart), nmp, S.dev(hbest));
  MCHECK(m, hipGetLastError());
  MCHECK(m, hipMemcpyAsync(best, S.dev(hbest), sizeof(int32_t) * (size_t)nmp, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipStreamSynchronize(s));
  return 0;
}

int orbm_update_map_points(orbm_t *m, const orbm_map_point_update_t *u, int32_t *best, float *normal, float *min_dist, float *max_dist) {
  if (!m || !u || u->nmp < 0) return ORBX_E_ARG;
  const int nmp = u->nmp;
  if (nmp == 0) return 0;
  // everything is validated before anything is uploaded or launched; a refusal writes nothing
  if (!u->start || !u->pos || !u->ref_centre || !u->ref_scale || !u->ref_max_scale || !best || !normal || !min_dist || !max_dist) {
    m->err = "UpdateMapPoints: NULL argument"; return ORBX_E_ARG;
  }
  if (u->start[0] != 0) { m->err = "UpdateMapPoints: start[0] != 0"; return ORBX_E_ARG; }
  for (int p = 0; p < nmp; p++) {
    const int64_t n = (int64_t)u->start[p + 1] - (int64_t)u->start[p];
    if (n < 0) { m->err = "UpdateMapPoints: start decreases"; return ORBX_E_ARG; }
    if (n > 64 * DISTINCT_MAXT) { m->err = "UpdateMapPoints: more than 1024 observations of one map point"; return ORBX_E_ARG; }
  }
  const size_t total = (size_t)u->start[nmp], NP = (size_t)nmp;
  if (total > 0 && (!u->desc || !u->centre || !u->in_desc)) { m->err = "UpdateMapPoints: NULL entry array"; return ORBX_E_ARG; }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Staging S{m};   // one block up, one launch, the four outputs down as one span of the block, one synchronisation
  const auto hdesc = S.add(u->desc, 32 * total); const auto hstart = S.add(u->start, NP + 1);
  const auto hcen = S.add(u->centre, 3 * total); const auto hin = S.add(u->in_desc, total);
  const auto hpos = S.add(u->pos, 3 * NP), hrc = S.add(u->ref_centre, 3 * NP), hrs = S.add(u->ref_scale, NP), hrm = S.add(u->ref_max_scale, NP);
  const auto hbest = S.out<int32_t>(NP);
  const auto hnor = S.out<float>(3 * NP), hmin = S.out<float>(NP), hmax = S.out<float>(NP);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  MapPointUpdateParams P;
  P.desc = (const uint32_t *)S.dev(hdesc); P.start = S.dev(hstart); P.centre = S.dev(hcen); P.in_desc = S.dev(hin);
  P.pos = S.dev(hpos); P.ref_centre = S.dev(hrc); P.ref_scale = S.dev(hrs); P.ref_max_scale = S.dev(hrm);
  P.nmp = nmp; P.best = S.dev(hbest); P.normal = S.dev(hnor); P.min_dist = S.dev(hmin); P.max_dist = S.dev(hmax);
  hipLaunchKernelGGL(k_update_map_points, dim3((unsigned)((nmp + 3) / 4)), dim3(256), 0, s, P);
  MCHECK(m, hipGetLastError());
  MCHECK(m, S.download(s, hbest, hmax));
  MCHECK(m, hipStreamSynchronize(s));
  memcpy(best, S.host(hbest), sizeof(int32_t) * NP);
  const float *nor = S.host(hnor), *mind = S.host(hmin), *maxd = S.host(hmax);
  for (size_t p = 0; p < NP; p++) {
    if (u->start[p + 1] == u->start[p]) continue;   // observations.empty() (MapPoint.cc:483): the member returns without writing
    memcpy(normal + 3 * p, nor + 3 * p, 3 * sizeof(float));
    min_dist[p] = mind[p]; max_dist[p] = maxd[p];
  }
  return 0;
}

int orbm_map_point_normal_depth(int n, const float *centre, const float *pos, const float *ref_centre, float ref_scale, float ref_max_scale,
                                float *normal, float *min_dist, float *max_dist) {
  if (n < 0 || (n > 0 && !centre) || !pos || !ref_centre || !normal || !min_dist || !max_dist) return ORBX_E_ARG;
  if (n == 0) return 0;   // observations.empty() (MapPoint.cc:483)
  map_point_normal_depth(n, centre, pos, ref_centre, ref_scale, ref_max_scale, normal, min_dist, max_dist);
  return 0;
}

// ---- LocalMapping::KeyFrameCulling (LocalMapping.cc:1158-1310): orb_ref_culling.h, orb_culling_kernels.h ----
// What is refused before anything is uploaded, launched or written (include/orbhip.h); nullptr = accepted
static const char *culling_refusal(const orbm_culling_t *c) {
  if (!c) return "KeyFrameCulling: NULL struct";
  if (c->K < 0 || c->P < 0) return "KeyFrameCulling: negative count";
  if (c->K > ORBM_CULL_MAX_KEYFRAMES) return "KeyFrameCulling: K above ORBM_CULL_MAX_KEYFRAMES (1024)";
  if (c->redundant_th != c->redundant_th) return "KeyFrameCulling: redundant_th is NaN";
  if (c->K == 0) return nullptr;
  if (!c->skip || !c->th_depth || !c->row_start || !c->obs_start) return "KeyFrameCulling: NULL argument";
  if (c->P > 0 && (!c->bad || !c->n_obs)) return "KeyFrameCulling: NULL point array";
  if (c->row_start[0] != 0 || c->obs_start[0] != 0) return "KeyFrameCulling: row_start[0] / obs_start[0] != 0";
  for (int k = 0; k < c->K; k++) {
    const int64_t n = (int64_t)c->row_start[k + 1] - (int64_t)c->row_start[k];
    if (n < 0) return "KeyFrameCulling: row_start decreases";
    if (n > ORBM_MAX_KEYPOINTS) return "KeyFrameCulling: more than ORBM_MAX_KEYPOINTS (15360) rows in one keyframe";
  }
  for (int p = 0; p < c->P; p++)
    if (c->obs_start[p + 1] < c->obs_start[p]) return "KeyFrameCulling: obs_start decreases";
  const int R = c->row_start[c->K], E = c->obs_start[c->P];
  if (R > 0 && (!c->row_point || !c->row_level || (!c->mono && !c->row_depth))) return "KeyFrameCulling: NULL row array";
  if (E > 0 && (!c->obs_kf || !c->obs_level || !c->obs_w)) return "KeyFrameCulling: NULL entry array";
  for (int i = 0; i < R; i++)
    if (c->row_point[i] < -1 || c->row_point[i] >= c->P) return "KeyFrameCulling: row_point outside [-1, P)";
  std::vector<int32_t> seen((size_t)c->K, -1);   // seen[kf] = the last point that had an entry of keyframe kf
  for (int p = 0; p < c->P; p++)
    for (int e = c->obs_start[p]; e < c->obs_start[p + 1]; e++) {
      const int kf = c->obs_kf[e];
      if (kf < -1 || kf >= c->K) return "KeyFrameCulling: obs_kf outside [-1, K)";
      if (c->obs_w[e] != 1 && c->obs_w[e] != 2) return "KeyFrameCulling: obs_w outside {1, 2}";
      if (kf >= 0) {
        if (seen[kf] == p) return "KeyFrameCulling: two entries of one point with the same obs_kf";
        seen[kf] = p;
      }
    }
  return nullptr;
}

// The tables and the loop's state as parts of one staged block.  n_obs and bad come last, so that the one-call form's outputs follow
// them and everything that goes back is one span.
struct CullParts {
  PartOf<uint8_t> skip, erasable, obs_w, bad, touched, row_stat;
  PartOf<float> th_depth, row_depth;
  PartOf<int32_t> row_start, row_point, row_level, obs_start, obs_level, obs_kf, n_obs, sums;
  size_t K;
};
static CullParts culling_add(Staging &S, const orbm_culling_t *c, const uint8_t *erasable) {
  CullParts H;
  const size_t K = H.K = (size_t)c->K, NP = (size_t)c->P, R = (size_t)c->row_start[K], E = (size_t)c->obs_start[NP];
  H.skip = S.add(c->skip, K); H.erasable = S.add(erasable, K); H.th_depth = S.add(c->th_depth, K);
  H.row_start = S.add(c->row_start, K + 1); H.row_point = S.add(c->row_point, R); H.row_level = S.add(c->row_level, R);
  H.row_depth = S.add(c->row_depth, c->mono ? 0 : R);
  H.obs_start = S.add(c->obs_start, NP + 1); H.obs_level = S.add(c->obs_level, E); H.obs_w = S.add(c->obs_w, E); H.obs_kf = S.add(c->obs_kf, E);
  // touched [P], sum_mps [K], sum_red [K]: cleared on the device as one span.  With P == 0 touched is an empty part (NULL on the device):
  // the kernels index it with a row's point only, and a row's point lies in [0, P)
  H.touched = S.out<uint8_t>(NP); H.sums = S.out<int32_t>(2 * K);
  H.row_stat = S.out<uint8_t>(R);
  H.n_obs = S.add(c->n_obs, NP); H.bad = S.add(c->bad, NP);
  return H;
}
static CullParams culling_bind(const Staging &S, const CullParts &H, const orbm_culling_t *c) {
  CullParams P;
  P.K = c->K; P.mono = c->mono; P.redundant_th = c->redundant_th;
  P.skip = S.dev(H.skip); P.erasable = S.dev(H.erasable); P.th_depth = S.dev(H.th_depth);
  P.row_start = S.dev(H.row_start); P.row_point = S.dev(H.row_point); P.row_level = S.dev(H.row_level); P.row_depth = S.dev(H.row_depth);
  P.obs_start = S.dev(H.obs_start); P.obs_level = S.dev(H.obs_level); P.obs_w = S.dev(H.obs_w); P.obs_kf = S.dev(H.obs_kf);
  P.bad = S.dev(H.bad); P.n_obs = S.dev(H.n_obs);
  P.touched = S.dev(H.touched);
  P.sum_mps = S.dev(H.sums); P.sum_red = P.sum_mps + H.K;
  P.row_stat = S.dev(H.row_stat);
  return P;
}
// The loop-entry status of every row (k_cull_count) behind the upload
static int culling_count(orbm_t *m, hipStream_t s, const Staging &S, const CullParams &P, const CullParts &H, const orbm_culling_t *c) {
  MCHECK(m, S.fill(s, H.touched, H.sums, 0));
  int most = 0;
  for (int k = 0; k < c->K; k++) most = std::max(most, c->row_start[k + 1] - c->row_start[k]);
  if (most > 0) {
    hipLaunchKernelGGL(k_cull_count, dim3((unsigned)((most + 255) / 256), (unsigned)c->K), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
  }
  return 0;
}

int orbm_keyframe_culling(orbm_t *m, const orbm_culling_t *c, const uint8_t *erasable, int32_t *n_mps, int32_t *n_red, uint8_t *culled,
                          int32_t *n_obs_out, uint8_t *bad_out) {
  if (!m) return ORBX_E_ARG;
  if (const char *why = culling_refusal(c)) { m->err = why; return ORBX_E_ARG; }
  if (c->K == 0) return 0;
  if (!n_mps || !n_red || !culled) { m->err = "KeyFrameCulling: NULL output"; return ORBX_E_ARG; }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t K = (size_t)c->K, NP = (size_t)c->P;
  const std::vector<uint8_t> all(erasable ? 0 : K, (uint8_t)1);
  Staging S{m};   // one block up, two launches, the state and the outputs down as one span of the block, one synchronisation
  const CullParts H = culling_add(S, c, erasable ? erasable : all.data());
  const auto hmps = S.out<int32_t>(K), hred = S.out<int32_t>(K), hres = S.out<int32_t>(1);
  const auto hcul = S.out<uint8_t>(K);
  int rc = S.upload(s);
  if (rc < 0) return rc;
  const CullParams P = culling_bind(S, H, c);
  if ((rc = culling_count(m, s, S, P, H, c)) < 0) return rc;
  CullWalkParams W{0, -1, 0, 0, S.dev(hmps), S.dev(hred), S.dev(hcul), S.dev(hres)};
  hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(CULL_WALK_THREADS), 0, s, P, W);
  MCHECK(m, hipGetLastError());
  MCHECK(m, S.download(s, H.n_obs, hcul));
  MCHECK(m, hipStreamSynchronize(s));
  memcpy(n_mps, S.host(hmps), sizeof(int32_t) * K); memcpy(n_red, S.host(hred), sizeof(int32_t) * K); memcpy(culled, S.host(hcul), K);
  if (n_obs_out && NP) memcpy(n_obs_out, S.host(H.n_obs), sizeof(int32_t) * NP);
  if (bad_out && NP) memcpy(bad_out, S.host(H.bad), NP);
  return 0;
}

int orbm_keyframe_culling_open(orbm_t *m, const orbm_culling_t *c) {
  if (!m) return ORBX_E_ARG;
  if (const char *why = culling_refusal(c)) { m->err = why; return ORBX_E_ARG; }
  m->cull_open = false;   // an unfinished walk is discarded
  m->cull = CullParams{};
  m->cull.K = c->K; m->cull_next = 0; m->cull_pending = -1; m->cull_any = false;
  if (c->K == 0) { m->cull_open = true; return 0; }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const std::vector<uint8_t> all((size_t)c->K, (uint8_t)1);   // the stepwise form never reads erasable
  Staging S{m};
  const CullParts H = culling_add(S, c, all.data());
  int rc = S.upload(s);
  if (rc < 0) return rc;
  CullParams P = culling_bind(S, H, c);
  if ((rc = culling_count(m, s, S, P, H, c)) < 0) return rc;
  // the block moves into the walk's own buffer: other entries reuse d_block between the steps
  const size_t bytes = S.total;
  MCHECK(m, m->d_cull.reserve(m->d_cull.bytes >= bytes ? bytes : 2 * bytes));
  MCHECK(m, hipMemcpyAsync(m->d_cull.p, m->d_block.p, bytes, hipMemcpyDeviceToDevice, s));
  MCHECK(m, hipStreamSynchronize(s));   // the pinned mirror is free for the next entry
  const ptrdiff_t delta = (const uint8_t *)m->d_cull.p - (const uint8_t *)m->d_block.p;
  auto moved = [delta](auto *&p) { if (p) p = (std::remove_reference_t<decltype(p)>)((uintptr_t)p + delta); };
  moved(P.skip); moved(P.erasable); moved(P.th_depth); moved(P.row_start); moved(P.row_point); moved(P.row_level); moved(P.row_depth);
  moved(P.obs_start); moved(P.obs_level); moved(P.obs_w); moved(P.obs_kf); moved(P.bad); moved(P.n_obs); moved(P.touched);
  moved(P.sum_mps); moved(P.sum_red); moved(P.row_stat);
  m->cull = P;
  m->cull_open = true;
  return 0;
}

int orbm_keyframe_culling_step(orbm_t *m, int applied, int32_t *k, int32_t *n_mps, int32_t *n_red) {
  if (!m) return ORBX_E_ARG;
  if (!m->cull_open) { m->err = "KeyFrameCulling: step without open"; return ORBX_E_ARG; }
  if (!k || !n_mps || !n_red) { m->err = "KeyFrameCulling: NULL output"; return ORBX_E_ARG; }
  const int K = m->cull.K, first = m->cull_next;
  if (first >= K) { *k = K; return 0; }   // the walk has ended: nothing is left that an erase could change
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Staging S{m};   // the outputs alone; the tables and the state stay in d_cull
  const auto hmps = S.out<int32_t>((size_t)K), hred = S.out<int32_t>((size_t)K), hres = S.out<int32_t>(1);
  const int rc = S.upload(s);
  if (rc < 0) return rc;
  const bool erase = applied != 0 && m->cull_pending >= 0;
  CullWalkParams W{first, erase ? m->cull_pending : -1, m->cull_any, 1, S.dev(hmps), S.dev(hred), nullptr, S.dev(hres)};
  m->cull_any = m->cull_any || erase;
  hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(CULL_WALK_THREADS), 0, s, m->cull, W);
  MCHECK(m, hipGetLastError());
  MCHECK(m, S.download(s, hmps, hres));
  MCHECK(m, hipStreamSynchronize(s));
  const int at = *S.host(hres);
  for (int j = first; j <= std::min(at, K - 1); j++) { n_mps[j] = S.host(hmps)[j]; n_red[j] = S.host(hred)[j]; }
  m->cull_pending = at < K ? at : -1;
  m->cull_next = at < K ? at + 1 : K;
  *k = at;
  return 0;
}

static thread_local const char *g_cull_host_err = "";
const char *orbm_keyframe_culling_host_error(void) { return g_cull_host_err; }

int orbm_keyframe_culling_host(const orbm_culling_t *c, const uint8_t *erasable, int32_t *n_mps, int32_t *n_red, uint8_t *culled,
                               int32_t *n_obs_out, uint8_t *bad_out) {
  if (const char *why = culling_refusal(c)) { g_cull_host_err = why; return ORBX_E_ARG; }
  if (c->K == 0) return 0;
  if (!n_mps || !n_red || !culled) { g_cull_host_err = "KeyFrameCulling: NULL output"; return ORBX_E_ARG; }
  const CullTables T{c->K, c->skip, c->th_depth, c->row_start, c->row_point, c->row_level, c->row_depth, c->obs_start, c->obs_level, c->obs_w,
                     c->mono != 0, c->redundant_th};
  const size_t NP = (size_t)c->P, E = (size_t)c->obs_start[NP];
  std::vector<uint8_t> bad(c->bad, c->bad + NP);
  std::vector<int32_t> n_obs(c->n_obs, c->n_obs + NP), obs_kf(c->obs_kf, c->obs_kf + E);
  for (int k = 0; k < c->K; k++) {
    n_mps[k] = n_red[k] = 0; culled[k] = 0;
    if (c->skip[k]) continue;                                                        // :1200
    cull_counts_host(T, k, bad.data(), n_obs.data(), obs_kf.data(), &n_mps[k], &n_red[k]);
    if (!cull_test(n_red[k], c->redundant_th, n_mps[k]) || (erasable && !erasable[k])) continue;
    culled[k] = 1;
    cull_erase_host(T, k, bad.data(), n_obs.data(), obs_kf.data());                  // pKF->SetBadFlag() (:1302)
  }
  if (n_obs_out && NP) memcpy(n_obs_out, n_obs.data(), sizeof(int32_t) * NP);
  if (bad_out && NP) memcpy(bad_out, bad.data(), NP);
  return 0;
}

// ---- Tracking::UpdateLocalMap (Tracking.cc:3542-3762) and KeyFrame::UpdateConnections (KeyFrame.cc:407-492): orb_ref_localmap.h,
// orb_localmap_kernels.h ----
// k_local_kf_walk and k_conn_walk sort up to 16384 8-byte keys in dynamic LDS
static LdsOnce g_lm_lds;

// What is refused of the tables before anything is uploaded, launched or written (include/orbhip.h); nullptr = accepted
static const char *graph_refusal(const orbm_map_graph_t *g, bool inertial) {
  if (!g) return "map graph: NULL struct";
  if (g->G < 0 || g->P < 0) return "map graph: negative count";
  if (g->G > ORBM_MAP_MAX_KEYFRAMES) return "map graph: G above ORBM_MAP_MAX_KEYFRAMES (16384)";
  const int G = g->G, P = g->P;
  if (G > 0 && (!g->kf_rank || !g->kf_bad || !g->kf_map || !g->kf_row_start || !g->kf_best || !g->kf_child_start || !g->kf_parent))
    return "map graph: NULL keyframe array";
  if (inertial && G > 0 && !g->kf_prev) return "map graph: inertial with kf_prev == NULL";
  if (P > 0 && (!g->pt_bad || !g->obs_start)) return "map graph: NULL point array";
  if (G > 0 && (g->kf_row_start[0] != 0 || g->kf_child_start[0] != 0)) return "map graph: kf_row_start[0] / kf_child_start[0] != 0";
  if (P > 0 && g->obs_start[0] != 0) return "map graph: obs_start[0] != 0";
  for (int k = 0; k < G; k++) {
    const int64_t n = (int64_t)g->kf_row_start[k + 1] - (int64_t)g->kf_row_start[k];
    if (n < 0) return "map graph: kf_row_start decreases";
    if (n > ORBM_MAX_KEYPOINTS) return "map graph: more than ORBM_MAX_KEYPOINTS (15360) rows in one keyframe";
    if (g->kf_child_start[k + 1] < g->kf_child_start[k]) return "map graph: kf_child_start decreases";
  }
  for (int p = 0; p < P; p++)
    if (g->obs_start[p + 1] < g->obs_start[p]) return "map graph: obs_start decreases";
  const int R = G ? g->kf_row_start[G] : 0, C = G ? g->kf_child_start[G] : 0, E = P ? g->obs_start[P] : 0;
  if (R > 0 && !g->row_point) return "map graph: NULL row_point";
  if (C > 0 && !g->kf_child) return "map graph: NULL kf_child";
  if (E > 0 && !g->obs_kf) return "map graph: NULL obs_kf";
  for (int i = 0; i < R; i++)
    if (g->row_point[i] < -1 || g->row_point[i] >= P) return "map graph: row_point outside [-1, P)";
  for (int i = 0; i < C; i++)
    if (g->kf_child[i] < 0 || g->kf_child[i] >= G) return "map graph: kf_child outside [0, G)";
  for (int i = 0; i < G * ORBM_MAP_BEST; i++)
    if (g->kf_best[i] < -1 || g->kf_best[i] >= G) return "map graph: kf_best outside [-1, G)";
  for (int k = 0; k < G; k++) {
    if (g->kf_parent[k] < -1 || g->kf_parent[k] >= G) return "map graph: kf_parent outside [-1, G)";
    if (g->kf_prev && (g->kf_prev[k] < -1 || g->kf_prev[k] >= G)) return "map graph: kf_prev outside [-1, G)";
  }
  std::vector<int32_t> ranks(g->kf_rank, g->kf_rank + G);
  std::sort(ranks.begin(), ranks.end());
  if (std::adjacent_find(ranks.begin(), ranks.end()) != ranks.end()) return "map graph: duplicate ranks";
  std::vector<int32_t> seen((size_t)G, -1);   // seen[kf] = the last point that had an entry of keyframe kf
  for (int p = 0; p < P; p++) {
    if (g->pt_bad[p]) continue;               // the entries of a bad point are not read
    for (int e = g->obs_start[p]; e < g->obs_start[p + 1]; e++) {
      const int kf = g->obs_kf[e];
      if (kf < 0 || kf >= G) return "map graph: obs_kf outside [0, G)";
      if (seen[(size_t)kf] == p) return "map graph: two entries of one point with the same keyframe";
      seen[(size_t)kf] = p;
    }
  }
  return nullptr;
}
static const char *local_map_refusal(const orbm_map_graph_t *g, int N, const int32_t *frame_point, int inertial, int last_kf, int cap_kf, int cap_pts,
                                     const void *local_kf, const void *n_local_kf, const void *kf_max, const void *max_votes, const void *slot_bad,
                                     const void *local_point, const void *n_local_point, bool host_tables) {
  if (!g) return "UpdateLocalMap: NULL struct";
  if (N < 0 || cap_kf < 0 || cap_pts < 0) return "UpdateLocalMap: negative count or capacity";
  if (!n_local_kf || !kf_max || !max_votes || !n_local_point) return "UpdateLocalMap: NULL output";
  if ((cap_kf > 0 && !local_kf) || (cap_pts > 0 && !local_point)) return "UpdateLocalMap: NULL output list";
  if (N > 0 && (!frame_point || !slot_bad)) return "UpdateLocalMap: NULL frame_point / slot_bad";
  if (host_tables) {
    if (const char *why = graph_refusal(g, inertial != 0)) return why;
    for (int s = 0; s < N; s++)
      if (frame_point[s] < -1 || frame_point[s] >= g->P) return "UpdateLocalMap: frame_point outside [-1, P)";
  } else {
    if (g->G < 0 || g->P < 0 || g->G > ORBM_MAP_MAX_KEYFRAMES) return "UpdateLocalMap: G or P out of range";
    if (g->G > 0 && (!g->kf_rank || !g->kf_bad || !g->kf_map || !g->kf_row_start || !g->row_point || !g->kf_best || !g->kf_child_start || !g->kf_parent))
      return "UpdateLocalMap: NULL keyframe array";
    if (g->P > 0 && (!g->pt_bad || !g->obs_start || !g->obs_kf)) return "UpdateLocalMap: NULL point array";
    if (inertial && g->G > 0 && !g->kf_prev) return "UpdateLocalMap: inertial with kf_prev == NULL";
  }
  if (last_kf < -1 || last_kf >= g->G) return "UpdateLocalMap: last_kf outside [-1, G)";
  return nullptr;
}
static const char *connections_refusal(const orbm_map_graph_t *g, int T, const int32_t *targets, int cap, const void *conn_start, const void *conn_kf,
                                       const void *conn_w, const void *ord_start, const void *ord_kf, const void *ord_w, const void *kf_max, const void *nmax) {
  if (!g) return "UpdateConnections: NULL struct";
  if (T < 0 || cap < 0) return "UpdateConnections: negative count or capacity";
  if (const char *why = graph_refusal(g, false)) return why;
  if (T == 0) return nullptr;
  if (!targets || !conn_start || !ord_start || !kf_max || !nmax) return "UpdateConnections: NULL argument";
  if (cap > 0 && (!conn_kf || !conn_w || !ord_kf || !ord_w)) return "UpdateConnections: NULL output list";
  std::vector<uint8_t> listed((size_t)g->G, 0);
  for (int t = 0; t < T; t++) {
    if (targets[t] < 0 || targets[t] >= g->G) return "UpdateConnections: target outside [0, G)";
    if (listed[(size_t)targets[t]]) return "UpdateConnections: a target listed twice";
    listed[(size_t)targets[t]] = 1;
  }
  return nullptr;
}
static LmGraph lm_graph(const orbm_map_graph_t *g) {
  return {g->G, g->kf_rank, g->kf_bad, g->kf_map, g->kf_row_start, g->row_point, g->kf_best, g->kf_child_start, g->kf_child, g->kf_parent, g->kf_prev,
          g->P, g->pt_bad, g->obs_start, g->obs_kf};
}
static LmTables lm_tables(const orbm_map_graph_t *g) {   // a struct of device pointers
  return {g->G, g->kf_rank, g->kf_bad, g->kf_map, g->kf_row_start, g->row_point, g->kf_best, g->kf_child_start, g->kf_child, g->kf_parent, g->kf_prev,
          g->P, g->pt_bad, g->obs_start, g->obs_kf};
}

// The tables as parts of one staged block
struct GraphParts {
  PartOf<int32_t> rank, map, row_start, row_point, best, child_start, child, parent, prev, obs_start, obs_kf;
  PartOf<uint8_t> kf_bad, pt_bad;
};
static GraphParts graph_add(Staging &S, const orbm_map_graph_t *g, bool with_prev) {
  GraphParts H;
  const size_t G = (size_t)g->G, P = (size_t)g->P;
  const size_t R = G ? (size_t)g->kf_row_start[G] : 0, C = G ? (size_t)g->kf_child_start[G] : 0, E = P ? (size_t)g->obs_start[P] : 0;
  H.rank = S.add(g->kf_rank, G); H.kf_bad = S.add(g->kf_bad, G); H.map = S.add(g->kf_map, G);
  H.row_start = S.add(g->kf_row_start, G ? G + 1 : 0); H.row_point = S.add(g->row_point, R); H.best = S.add(g->kf_best, G * ORBM_MAP_BEST);
  H.child_start = S.add(g->kf_child_start, G ? G + 1 : 0); H.child = S.add(g->kf_child, C); H.parent = S.add(g->kf_parent, G);
  H.prev = S.add(g->kf_prev, with_prev ? G : 0);
  H.pt_bad = S.add(g->pt_bad, P); H.obs_start = S.add(g->obs_start, P ? P + 1 : 0); H.obs_kf = S.add(g->obs_kf, E);
  return H;
}
static LmTables graph_bind(const Staging &S, const GraphParts &H, const orbm_map_graph_t *g) {
  return {g->G, S.dev(H.rank), S.dev(H.kf_bad), S.dev(H.map), S.dev(H.row_start), S.dev(H.row_point), S.dev(H.best), S.dev(H.child_start), S.dev(H.child),
          S.dev(H.parent), S.dev(H.prev), g->P, S.dev(H.pt_bad), S.dev(H.obs_start), S.dev(H.obs_kf)};
}

// The scratch of one UpdateLocalMap call: hdr, count, kf_count and pt_word are ONE span that is zero on entry
struct LmScratch { int32_t *hdr, *count, *kf_count; uint32_t *pt_word; int32_t *list; };
struct LmOutputs { int32_t *local_kf, *n_local_kf, *kf_max, *max_votes; uint8_t *slot_bad; int32_t *local_point, *n_local_point; };
static int local_map_launch(orbm_t *m, hipStream_t s, const LmTables &M, const LmScratch &X, int N, const int32_t *d_frame_point, int inertial, int last_kf,
                            int cap_kf, int cap_pts, const LmOutputs &O) {
  MCHECK(m, raise_lds_once(g_lm_lds, m->device, {reinterpret_cast<const void *>(&k_local_kf_walk), reinterpret_cast<const void *>(&k_conn_walk)}));
  VoteParams V{M, N, d_frame_point, nullptr, O.slot_bad, X.count, m->vote_form};
  hipLaunchKernelGGL(k_covis_vote, dim3((unsigned)((N + 255) / 256), 1u), dim3(256), 0, s, V);
  WalkParams W{M, X.count, inertial, last_kf, cap_kf, X.list, X.hdr, O.local_kf, O.n_local_kf, O.kf_max, O.max_votes, O.n_local_point};
  hipLaunchKernelGGL(k_local_kf_walk, dim3(1), dim3(LM_WALK_THREADS), SortCarve::of(M.G).bytes, s, W);
  LpParams L{M, X.list, X.hdr, X.pt_word, X.kf_count, cap_pts, O.local_point, O.n_local_point};
  hipLaunchKernelGGL(k_lp_first, dim3(LM_TILES_X, LM_KF_BLOCKS), dim3(256), 0, s, L);
  hipLaunchKernelGGL(k_lp_count, dim3(LM_KF_BLOCKS), dim3(256), 0, s, L);
  hipLaunchKernelGGL(k_lp_write, dim3(LM_KF_BLOCKS), dim3(256), 0, s, L);
  MCHECK(m, hipGetLastError());
  return 0;
}

int orbm_update_local_map(orbm_t *m, const orbm_map_graph_t *g, int N, const int32_t *frame_point, int inertial, int last_kf, int cap_kf, int cap_pts,
                          int32_t *local_kf, int32_t *n_local_kf, int32_t *kf_max, int32_t *max_votes, uint8_t *slot_bad, int32_t *local_point,
                          int32_t *n_local_point) {
  if (!m) return ORBX_E_ARG;
  std::lock_guard<std::mutex> lock(m->lm_mu);
  if (const char *why = local_map_refusal(g, N, frame_point, inertial, last_kf, cap_kf, cap_pts, local_kf, n_local_kf, kf_max, max_votes, slot_bad, local_point,
                                          n_local_point, true)) { m->err = why; return ORBX_E_ARG; }
  if (N == 0) { *n_local_kf = 0; *n_local_point = 0; *kf_max = -1; *max_votes = 0; return 0; }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t G = (size_t)g->G, P = (size_t)g->P;
  Staging S{m};   // one block up, five launches, the outputs down as one span of the block, one synchronisation
  const GraphParts H = graph_add(S, g, inertial != 0);
  const auto hfp = S.add(frame_point, (size_t)N);
  const auto hhdr = S.out<int32_t>(LM_HDR), hcount = S.out<int32_t>(G), hkfc = S.out<int32_t>(G + 24);
  const auto hword = S.out<uint32_t>(P);
  const auto hlist = S.out<int32_t>(G + 24);
  const auto hres = S.out<int32_t>(4), hlkf = S.out<int32_t>((size_t)cap_kf), hlpt = S.out<int32_t>((size_t)cap_pts);
  const auto hsb = S.out<uint8_t>((size_t)N);
  int rc = S.upload(s);
  if (rc < 0) return rc;
  MCHECK(m, S.fill(s, hhdr, hword, 0));
  int32_t *res = S.dev(hres);
  const LmScratch X{S.dev(hhdr), S.dev(hcount), S.dev(hkfc), S.dev(hword), S.dev(hlist)};
  const LmOutputs O{S.dev(hlkf), res, res + 1, res + 2, S.dev(hsb), S.dev(hlpt), res + 3};
  if ((rc = local_map_launch(m, s, graph_bind(S, H, g), X, N, S.dev(hfp), inertial, last_kf, cap_kf, cap_pts, O)) < 0) return rc;
  MCHECK(m, S.download(s, hres, hsb));
  MCHECK(m, hipStreamSynchronize(s));
  const int32_t *r = S.host(hres);
  *n_local_kf = r[0]; *kf_max = r[1]; *max_votes = r[2]; *n_local_point = r[3];
  memcpy(slot_bad, S.host(hsb), (size_t)N);
  if (r[0] > cap_kf || r[3] > cap_pts) { m->err = "UpdateLocalMap: a list does not fit its capacity"; return ORBX_E_CAP; }
  if (r[0]) memcpy(local_kf, S.host(hlkf), sizeof(int32_t) * (size_t)r[0]);
  if (r[3]) memcpy(local_point, S.host(hlpt), sizeof(int32_t) * (size_t)r[3]);
  return 0;
}

int orbm_update_local_map_device(orbm_t *m, const orbm_map_graph_t *g, int N, const int32_t *d_frame_point, int inertial, int last_kf, int cap_kf,
                                 int cap_pts, int32_t *d_local_kf, int32_t *d_n_local_kf, int32_t *d_kf_max, int32_t *d_max_votes, uint8_t *d_slot_bad,
                                 int32_t *d_local_point, int32_t *d_n_local_point, void *stream) {
  if (!m) return ORBX_E_ARG;
  std::lock_guard<std::mutex> lock(m->lm_mu);
  if (const char *why = local_map_refusal(g, N, d_frame_point, inertial, last_kf, cap_kf, cap_pts, d_local_kf, d_n_local_kf, d_kf_max, d_max_votes, d_slot_bad,
                                          d_local_point, d_n_local_point, false)) { m->err = why; return ORBX_E_ARG; }
  if (N == 0) return 0;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t G = (size_t)g->G, P = (size_t)g->P;
  const size_t zeroed = sizeof(int32_t) * (LM_HDR + G + (G + 24) + P), bytes = zeroed + sizeof(int32_t) * (G + 24);
  MCHECK(m, m->d_lm.reserve(m->d_lm.bytes >= bytes ? bytes : 2 * bytes));
  int32_t *base = (int32_t *)m->d_lm.p;
  const LmScratch X{base, base + LM_HDR, base + LM_HDR + G, (uint32_t *)(base + LM_HDR + G + G + 24), base + LM_HDR + G + G + 24 + P};
  MCHECK(m, hipMemsetAsync(base, 0, zeroed, s));
  const LmOutputs O{d_local_kf, d_n_local_kf, d_kf_max, d_max_votes, d_slot_bad, d_local_point, d_n_local_point};
  return local_map_launch(m, s, lm_tables(g), X, N, d_frame_point, inertial, last_kf, cap_kf, cap_pts, O);
}

static thread_local const char *g_lm_host_err = "";
const char *orbm_update_local_map_host_error(void) { return g_lm_host_err; }

int orbm_update_local_map_host(const orbm_map_graph_t *g, int N, const int32_t *frame_point, int inertial, int last_kf, int cap_kf, int cap_pts,
                               int32_t *local_kf, int32_t *n_local_kf, int32_t *kf_max, int32_t *max_votes, uint8_t *slot_bad, int32_t *local_point,
                               int32_t *n_local_point) {
  if (const char *why = local_map_refusal(g, N, frame_point, inertial, last_kf, cap_kf, cap_pts, local_kf, n_local_kf, kf_max, max_votes, slot_bad, local_point,
                                          n_local_point, true)) { g_lm_host_err = why; return ORBX_E_ARG; }
  if (N == 0) { *n_local_kf = 0; *n_local_point = 0; *kf_max = -1; *max_votes = 0; return 0; }
  std::vector<int32_t> kfs, pts;
  int best, votes;
  lm_update_local_map_host(lm_graph(g), N, frame_point, inertial != 0, last_kf, kfs, &best, &votes, slot_bad, pts);
  *n_local_kf = (int32_t)kfs.size(); *n_local_point = (int32_t)pts.size(); *kf_max = best; *max_votes = votes;
  if ((int)kfs.size() > cap_kf || (int)pts.size() > cap_pts) { g_lm_host_err = "UpdateLocalMap: a list does not fit its capacity"; return ORBX_E_CAP; }
  if (!kfs.empty()) memcpy(local_kf, kfs.data(), sizeof(int32_t) * kfs.size());
  if (!pts.empty()) memcpy(local_point, pts.data(), sizeof(int32_t) * pts.size());
  return 0;
}

int orbm_update_connections(orbm_t *m, const orbm_map_graph_t *g, int T, const int32_t *targets, int th, int cap, int32_t *conn_start, int32_t *conn_kf,
                            int32_t *conn_w, int32_t *ord_start, int32_t *ord_kf, int32_t *ord_w, int32_t *kf_max, int32_t *nmax) {
  if (!m) return ORBX_E_ARG;
  std::lock_guard<std::mutex> lock(m->lm_mu);
  if (const char *why = connections_refusal(g, T, targets, cap, conn_start, conn_kf, conn_w, ord_start, ord_kf, ord_w, kf_max, nmax)) { m->err = why; return ORBX_E_ARG; }
  if (T == 0) return 0;
  MCHECK(m, hipSetDevice(m->device));
  MCHECK(m, raise_lds_once(g_lm_lds, m->device, {reinterpret_cast<const void *>(&k_local_kf_walk), reinterpret_cast<const void *>(&k_conn_walk)}));
  hipStream_t s = m->stream;
  const size_t G = (size_t)g->G, nT = (size_t)T, TG = nT * G;
  Staging S{m};   // one block up, three launches, the outputs down as one span of the block, one synchronisation
  const GraphParts H = graph_add(S, g, false);
  const auto htar = S.add(targets, nT);
  const auto hcount = S.out<int32_t>(TG), hwork = S.out<int32_t>(4 * TG), hn = S.out<int32_t>(2 * nT);
  const auto hcs = S.out<int32_t>(nT + 1), hos = S.out<int32_t>(nT + 1), hmax = S.out<int32_t>(2 * nT), hlists = S.out<int32_t>(4 * (size_t)cap);
  int rc = S.upload(s, false);   // the mirror of the outputs is made below: the work arrays take no pinned memory
  if (rc < 0) return rc;
  MCHECK(m, S.fill(s, hcount, hcount, 0));
  const LmTables M = graph_bind(S, H, g);
  int most = 0;
  for (int t = 0; t < T; t++) most = std::max(most, g->kf_row_start[targets[t] + 1] - g->kf_row_start[targets[t]]);
  int32_t *work = S.dev(hwork), *lists = S.dev(hlists);
  ConnParams C{M, S.dev(hcount), S.dev(htar), T, th, cap, work, work + TG, work + 2 * TG, work + 3 * TG, S.dev(hn), S.dev(hn) + nT,
               S.dev(hcs), lists, lists + cap, S.dev(hos), lists + 2 * (size_t)cap, lists + 3 * (size_t)cap, S.dev(hmax), S.dev(hmax) + nT};
  if (most > 0) {
    VoteParams V{M, 0, nullptr, S.dev(htar), nullptr, S.dev(hcount), m->vote_form};
    hipLaunchKernelGGL(k_covis_vote, dim3((unsigned)((most + 255) / 256), (unsigned)T), dim3(256), 0, s, V);
  }
  hipLaunchKernelGGL(k_conn_walk, dim3((unsigned)T), dim3(LM_WALK_THREADS), SortCarve::of(g->G).bytes, s, C);
  hipLaunchKernelGGL(k_conn_pack, dim3((unsigned)T), dim3(256), 0, s, C);
  MCHECK(m, hipGetLastError());
  const size_t out_bytes = S.span(hcs, hlists);
  std::vector<uint8_t> &back = m->lm_back;
  back.resize(out_bytes);
  MCHECK(m, hipMemcpyAsync(back.data(), S.block() + S.offset(hcs), out_bytes, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipStreamSynchronize(s));
  auto at = [&](auto h) { return (const int32_t *)(back.data() + (S.offset(h) - S.offset(hcs))); };
  memcpy(conn_start, at(hcs), sizeof(int32_t) * (nT + 1)); memcpy(ord_start, at(hos), sizeof(int32_t) * (nT + 1));
  memcpy(kf_max, at(hmax), sizeof(int32_t) * nT); memcpy(nmax, at(hmax) + nT, sizeof(int32_t) * nT);
  if (conn_start[T] > cap) { m->err = "UpdateConnections: the lists do not fit cap"; return ORBX_E_CAP; }
  const size_t nc = sizeof(int32_t) * (size_t)conn_start[T], no = sizeof(int32_t) * (size_t)ord_start[T];
  if (nc) { memcpy(conn_kf, at(hlists), nc); memcpy(conn_w, at(hlists) + cap, nc); }
  if (no) { memcpy(ord_kf, at(hlists) + 2 * (size_t)cap, no); memcpy(ord_w, at(hlists) + 3 * (size_t)cap, no); }
  return 0;
}

int orbm_update_connections_host(const orbm_map_graph_t *g, int T, const int32_t *targets, int th, int cap, int32_t *conn_start, int32_t *conn_kf,
                                 int32_t *conn_w, int32_t *ord_start, int32_t *ord_kf, int32_t *ord_w, int32_t *kf_max, int32_t *nmax) {
  if (const char *why = connections_refusal(g, T, targets, cap, conn_start, conn_kf, conn_w, ord_start, ord_kf, ord_w, kf_max, nmax)) { g_lm_host_err = why; return ORBX_E_ARG; }
  if (T == 0) return 0;
  const LmGraph M = lm_graph(g);
  std::vector<std::vector<int32_t>> ck((size_t)T), cw((size_t)T), ok((size_t)T), ow((size_t)T);
  conn_start[0] = ord_start[0] = 0;
  for (int t = 0; t < T; t++) {
    conn_update_host(M, targets[t], th, ck[(size_t)t], cw[(size_t)t], ok[(size_t)t], ow[(size_t)t], &kf_max[t], &nmax[t]);
    conn_start[t + 1] = conn_start[t] + (int32_t)ck[(size_t)t].size(); ord_start[t + 1] = ord_start[t] + (int32_t)ok[(size_t)t].size();
  }
  if (conn_start[T] > cap) { g_lm_host_err = "UpdateConnections: the lists do not fit cap"; return ORBX_E_CAP; }
  for (int t = 0; t < T; t++) {
    std::copy(ck[(size_t)t].begin(), ck[(size_t)t].end(), conn_kf + conn_start[t]); std::copy(cw[(size_t)t].begin(), cw[(size_t)t].end(), conn_w + conn_start[t]);
    std::copy(ok[(size_t)t].begin(), ok[(size_t)t].end(), ord_kf + ord_start[t]); std::copy(ow[(size_t)t].begin(), ow[(size_t)t].end(), ord_w + ord_start[t]);
  }
  return 0;
}

int orbm_gather_local_map_device(orbm_t *m, int P, int N, const int32_t *d_frame_point, const int32_t *d_local_point, const int32_t *d_n_local_point, int cap,
                                 const uint8_t *d_pt_bad, const float *d_Xw, const float *d_normal, const float *d_max_dist, const float *d_min_dist,
                                 const uint8_t *d_mpdesc, const uint8_t *d_obs, const orbm_local_map_t *out, int32_t *d_map_n, void *stream) {
  if (!m) return ORBX_E_ARG;
  std::lock_guard<std::mutex> lock(m->lm_mu);
  if (P < 0 || N < 0 || cap < 0) { m->err = "GatherLocalMap: negative count"; return ORBX_E_ARG; }
  if (!d_n_local_point || !out || !d_map_n || (N > 0 && !d_frame_point)) { m->err = "GatherLocalMap: NULL argument"; return ORBX_E_ARG; }
  if (cap > 0 && (!d_local_point || !d_pt_bad || !d_Xw || !d_normal || !d_max_dist || !d_min_dist || !d_mpdesc || !out->eligible || !out->Xw || !out->normal ||
                  !out->max_dist || !out->min_dist || !out->mpdesc)) { m->err = "GatherLocalMap: NULL array"; return ORBX_E_ARG; }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  MCHECK(m, m->d_lm_flag.reserve(std::max<size_t>((size_t)P, 256)));
  GatherParams A{P, N, cap, d_frame_point, d_local_point, d_n_local_point, d_pt_bad, d_Xw, d_normal, d_max_dist, d_min_dist, d_mpdesc, d_obs,
                 (uint8_t *)m->d_lm_flag.p, (uint8_t *)out->eligible, (float *)out->Xw, (float *)out->normal, (float *)out->max_dist, (float *)out->min_dist,
                 (uint8_t *)out->mpdesc, (uint8_t *)out->obs, d_map_n};
  if (P > 0) MCHECK(m, hipMemsetAsync(m->d_lm_flag.p, 0, (size_t)P, s));
  if (N > 0 && P > 0) hipLaunchKernelGGL(k_gather_mark, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_gather_local_map, dim3((unsigned)std::max(1, (cap + 31) / 32)), dim3(256), 0, s, A);
  MCHECK(m, hipGetLastError());
  return 0;
}

// ---- TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc:39-127): orb_ref_twoview.h, orb_twoview_kernels.h ----
// mvMatches12 as the reference fills it (:53-62), the four coordinates of every match, and both frames normalised (:137-139, :188-190)
struct TvProblem {
  const orbx_keypoint_t *keys1, *keys2;
  int n1, n2, N;
  std::vector<int32_t> first, second;
  std::vector<float> mx;   // [N][4]: kp1.pt, kp2.pt
  std::vector<float> pn1, pn2;
  float T1[9], T2[9], T2inv[9], T2t[9];
};
// What is refused before anything is uploaded, launched or written (include/orbhip.h); nullptr = accepted
static const char *two_view_problem(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                    int min_matches, TvProblem &Q) {
  if (!keys1 || !keys2 || !matches12) return "TwoViewReconstruction: NULL argument";
  if (n1 < 0 || n2 < 0) return "TwoViewReconstruction: negative count";
  Q.keys1 = keys1; Q.keys2 = keys2; Q.n1 = n1; Q.n2 = n2;
  for (int i = 0; i < n1; i++) {
    if (matches12[i] < 0) continue;
    if (matches12[i] >= n2) return "TwoViewReconstruction: match index outside [0, n2)";
    Q.first.push_back(i); Q.second.push_back(matches12[i]);
    const orbx_keypoint_t &a = keys1[i], &b = keys2[matches12[i]];
    Q.mx.insert(Q.mx.end(), {a.x, a.y, b.x, b.y});
  }
  Q.N = (int)Q.first.size();
  if (Q.N < min_matches) return min_matches == 8 ? "TwoViewReconstruction: fewer than 8 matches" : "TwoViewReconstruction: no match";
  return nullptr;
}
static const char *two_view_sets(const TvProblem &Q, int iterations, const int32_t *sets) {
  if (iterations < 1) return "TwoViewReconstruction: iterations < 1";
  if (!sets) return "TwoViewReconstruction: NULL argument";
  for (size_t k = 0; k < 8 * (size_t)iterations; k++)
    if (sets[k] < 0 || sets[k] >= Q.N) return "TwoViewReconstruction: set index outside [0, N)";
  return nullptr;
}
static void two_view_normalize(TvProblem &Q) {
  Q.pn1.resize(2 * (size_t)Q.n1); Q.pn2.resize(2 * (size_t)Q.n2);
  tv_normalize(Q.keys1, Q.n1, Q.pn1.data(), Q.T1);
  tv_normalize(Q.keys2, Q.n2, Q.pn2.data(), Q.T2);
  tv_inv33(Q.T2, Q.T2inv);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Q.T2t[3 * i + j] = Q.T2[3 * j + i];
}

// The outputs of the two stages, on the host
struct TvModels {
  std::vector<float> H21, H12, F21, score;   // [iterations][9] x 3, [2][iterations]
  int32_t best[2];
  float top[2], M[18];                       // SH, SF; H21, F21 of the winners
  std::vector<uint8_t> mask;                 // [2][N]
};
struct TvChecked {
  std::vector<float> p3d;                    // [nhyp][n1][3]
  std::vector<uint8_t> good, status;         // [nhyp][n1], [nhyp][N]
  int32_t nGood[8];
  float cos_rank[8], parallax[8];
};
static void two_view_parallax(int nhyp, TvChecked &C) {
  for (int h = 0; h < nhyp; h++) C.parallax[h] = C.nGood[h] > 0 ? tv_parallax_degrees(acosf(C.cos_rank[h])) : 0.f;   // :900-908
}

static void two_view_models_cpu(const TvProblem &Q, float sigma, int iterations, const int32_t *sets, TvModels &M) {
  const size_t I = (size_t)iterations, N = (size_t)Q.N;
  M.H21.assign(9 * I, 0.f); M.H12.assign(9 * I, 0.f); M.F21.assign(9 * I, 0.f); M.score.assign(2 * I, 0.f);
  M.mask.assign(2 * N, 0);
  float ws[TV_WS_FLOATS];
  double W[TV_WS_DOUBLES];
  const float inv = tv_inv_sigma_square(sigma);
  for (int model = 0; model < 2; model++) {
    M.best[model] = -1; M.top[model] = 0.f;
    for (int k = 0; k < 9; k++) M.M[9 * model + k] = 0.f;
    std::vector<uint8_t> cur(N);
    for (size_t it = 0; it < I; it++) {
      float q[32];
      for (int j = 0; j < 8; j++) {
        const int idx = sets[8 * it + j], i1 = Q.first[idx], i2 = Q.second[idx];
        q[4 * j] = Q.pn1[2 * i1]; q[4 * j + 1] = Q.pn1[2 * i1 + 1]; q[4 * j + 2] = Q.pn2[2 * i2]; q[4 * j + 3] = Q.pn2[2 * i2 + 1];
      }
      float *M21 = (model ? M.F21.data() : M.H21.data()) + 9 * it, *M12 = M.H12.data() + 9 * it;
      if (model == 0) tv_homography(q, Q.T1, Q.T2inv, ws, W, M21, M12, TvSolo());
      else tv_fundamental(q, Q.T1, Q.T2t, ws, W, M21, TvSolo());
      float score = 0;
      for (size_t i = 0; i < N; i++) {
        const float *m = &Q.mx[4 * i];
        const TvTerms r = tv_check_model(model, M21, M12, m[0], m[1], m[2], m[3], inv);
        if (r.in1) score += r.t1;
        if (r.in2) score += r.t2;
        cur[i] = r.in1 && r.in2;
      }
      M.score[model * I + it] = score;
      if (score > M.top[model]) {
        M.top[model] = score; M.best[model] = (int32_t)it;
        memcpy(&M.M[9 * model], M21, 9 * sizeof(float));
        memcpy(&M.mask[model * N], cur.data(), N);
      }
    }
  }
}

static void two_view_cameras(const float *K, float sigma, int nhyp, const float *T, TvCamera *cams) {
  for (int h = 0; h < nhyp; h++) tv_camera(K, T + 12 * h, sigma, cams[h]);
}
static void two_view_check_cpu(const TvProblem &Q, const uint8_t *mask, const float *K, float sigma, int nhyp, const float *T, TvChecked &C) {
  const size_t N = (size_t)Q.N, n1 = (size_t)Q.n1;
  C.p3d.assign(3 * n1 * nhyp, 0.f); C.good.assign(n1 * nhyp, 0); C.status.assign(N * nhyp, 0);
  TvCamera cams[8];
  two_view_cameras(K, sigma, nhyp, T, cams);
  for (int h = 0; h < nhyp; h++) {
    std::vector<float> cosv;
    for (size_t i = 0; i < N; i++) {
      if (!mask[i]) { C.status[h * N + i] = TV_NOT_INLIER; continue; }
      const float *m = &Q.mx[4 * i];
      float p[3], cp = 0.f;
      const int st = tv_check_rt(cams[h], m[0], m[1], m[2], m[3], p, &cp);
      C.status[h * N + i] = (uint8_t)st;
      if (st != TV_GOOD && st != TV_LOW_PARALLAX) continue;
      const size_t k = h * n1 + (size_t)Q.first[i];
      C.p3d[3 * k] = p[0]; C.p3d[3 * k + 1] = p[1]; C.p3d[3 * k + 2] = p[2];
      if (st == TV_GOOD) C.good[k] = 1;
      cosv.push_back(cp);
    }
    C.nGood[h] = (int32_t)cosv.size();
    C.cos_rank[h] = 0.f;
    if (!cosv.empty()) {
      std::sort(cosv.begin(), cosv.end());
      C.cos_rank[h] = cosv[std::min<size_t>(50, cosv.size() - 1)];
    }
  }
  two_view_parallax(nhyp, C);
}

// The device side: one staged block for both stages.  Inputs first, then the models' outputs (one span down), then CheckRT's.
struct TvDevice {
  orbm_t *m;
  Staging S;
  PartOf<float> pn1, pn2, mx, H21, H12, F21, score, top, M, cos_list, p3d, cos_rank;
  PartOf<int32_t> first, second, sets, best, nGood;
  PartOf<uint8_t> mask_in, mask, good, status;
  PartOf<TvCamera> cams;
  size_t I, N, n1;
  // iterations == 0: no model stage; hyp == 0: no CheckRT stage; inliers: the caller's mask for CheckRT alone
  int upload(const TvProblem &Q, int iterations, const int32_t *set_idx, int hyp, const uint8_t *inliers) {
    I = (size_t)iterations; N = (size_t)Q.N; n1 = (size_t)Q.n1;
    const size_t H = (size_t)hyp;
    mx = S.add(Q.mx.data(), 4 * N); first = S.add(Q.first.data(), N);
    pn1 = S.add(Q.pn1.data(), I ? 2 * n1 : 0); pn2 = S.add(Q.pn2.data(), I ? 2 * (size_t)Q.n2 : 0);
    second = S.add(Q.second.data(), I ? N : 0); sets = S.add(set_idx, 8 * I);
    mask_in = S.add(inliers, inliers ? N : 0);
    H21 = S.out<float>(9 * I); H12 = S.out<float>(9 * I); F21 = S.out<float>(9 * I); score = S.out<float>(2 * I);
    best = S.out<int32_t>(I ? 2 : 0); top = S.out<float>(I ? 2 : 0); M = S.out<float>(I ? 18 : 0); mask = S.out<uint8_t>(I ? 2 * N : 0);
    cams = S.out<TvCamera>(H); cos_list = S.out<float>(H * N);
    p3d = S.out<float>(3 * H * n1); good = S.out<uint8_t>(H * n1); nGood = S.out<int32_t>(H);
    status = S.out<uint8_t>(H * N); cos_rank = S.out<float>(H);
    return S.upload(m->stream);
  }
  // k_tv_hypotheses, k_tv_score, k_tv_winner, everything down, one synchronisation
  int models(const TvProblem &Q, float sigma, TvModels &R) {
    hipStream_t s = m->stream;
    TvModelParams P;
    memcpy(P.T1, Q.T1, sizeof(P.T1)); memcpy(P.T2inv, Q.T2inv, sizeof(P.T2inv)); memcpy(P.T2t, Q.T2t, sizeof(P.T2t));
    P.pn1 = S.dev(pn1); P.pn2 = S.dev(pn2); P.first = S.dev(first); P.second = S.dev(second); P.sets = S.dev(sets);
    P.mx = (const float4 *)S.dev(mx);
    P.iterations = (int)I; P.N = (int)N; P.invSigmaSquare = tv_inv_sigma_square(sigma);
    P.H21 = S.dev(H21); P.H12 = S.dev(H12); P.F21 = S.dev(F21); P.score = S.dev(score);
    P.best = S.dev(best); P.best_score = S.dev(top); P.best_M = S.dev(M); P.mask = S.dev(mask);
    hipLaunchKernelGGL(k_tv_hypotheses, dim3((unsigned)((2 * I + 3) / 4)), dim3(64), 0, s, P);
    MCHECK(m, hipGetLastError());
    hipLaunchKernelGGL(k_tv_score, dim3((unsigned)I, 2), dim3(64), 0, s, P);
    MCHECK(m, hipGetLastError());
    hipLaunchKernelGGL(k_tv_winner, dim3(2), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
    MCHECK(m, S.download(s, H21, mask));
    MCHECK(m, hipStreamSynchronize(s));
    R.H21.assign(S.host(H21), S.host(H21) + 9 * I); R.H12.assign(S.host(H12), S.host(H12) + 9 * I);
    R.F21.assign(S.host(F21), S.host(F21) + 9 * I); R.score.assign(S.host(score), S.host(score) + 2 * I);
    memcpy(R.best, S.host(best), sizeof(R.best)); memcpy(R.top, S.host(top), sizeof(R.top)); memcpy(R.M, S.host(M), sizeof(R.M));
    R.mask.assign(S.host(mask), S.host(mask) + 2 * N);
    return 0;
  }
  // The hypotheses' cameras up, k_tv_check_rt, k_tv_cos_rank, the results down, one synchronisation.  d_mask: the inlier vector on the device
  int check(const float *K, float sigma, int nhyp, const float *T, const uint8_t *d_mask, TvChecked &C) {
    hipStream_t s = m->stream;
    const size_t H = (size_t)nhyp;
    two_view_cameras(K, sigma, nhyp, T, S.host(cams));
    MCHECK(m, hipMemcpyAsync(S.dev(cams), S.host(cams), sizeof(TvCamera) * H, hipMemcpyHostToDevice, s));
    MCHECK(m, S.fill(s, p3d, nGood, 0));   // vP3D, vbGood, nGood
    TvCheckParams P;
    P.cams = S.dev(cams); P.mx = (const float4 *)S.dev(mx); P.first = S.dev(first); P.mask = d_mask;
    P.nhyp = nhyp; P.N = (int)N; P.n1 = (int)n1;
    P.p3d = S.dev(p3d); P.good = S.dev(good); P.status = S.dev(status); P.nGood = S.dev(nGood);
    P.cos_list = S.dev(cos_list); P.cos_rank = S.dev(cos_rank);
    hipLaunchKernelGGL(k_tv_check_rt, dim3((unsigned)((N + 255) / 256), (unsigned)nhyp), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
    hipLaunchKernelGGL(k_tv_cos_rank, dim3((unsigned)((N + 255) / 256), (unsigned)nhyp), dim3(256), 0, s, P);
    MCHECK(m, hipGetLastError());
    MCHECK(m, S.download(s, p3d, cos_rank));
    MCHECK(m, hipStreamSynchronize(s));
    C.p3d.assign(S.host(p3d), S.host(p3d) + 3 * H * n1); C.good.assign(S.host(good), S.host(good) + H * n1);
    C.status.assign(S.host(status), S.host(status) + H * N);
    memcpy(C.nGood, S.host(nGood), sizeof(int32_t) * H); memcpy(C.cos_rank, S.host(cos_rank), sizeof(float) * H);
    two_view_parallax(nhyp, C);
    return 0;
  }
};

// Reconstruct behind the argument checks, for either side: models(M) and check(mask_index, nhyp, T, C) are the two stages
extern "C++" {
template <class Models, class Check>
static int two_view_reconstruct(const TvProblem &Q, const float *K, float sigma, int iterations, float *R21, float *t21, float *vP3D,
                                uint8_t *vbTriangulated, const orbm_two_view_details_t *d, Models models, Check check) {
  const size_t N = (size_t)Q.N, n1 = (size_t)Q.n1, I = (size_t)iterations;
  static const orbm_two_view_details_t none = {};
  const orbm_two_view_details_t &D = d ? *d : none;
  if (D.used_H) *D.used_H = -1;
  if (D.nhyp) *D.nhyp = 0;
  if (D.chosen) *D.chosen = -1;
  if (D.R) memset(D.R, 0, sizeof(float) * 72);
  if (D.t) memset(D.t, 0, sizeof(float) * 24);
  if (D.nGood) memset(D.nGood, 0, sizeof(int32_t) * 8);
  if (D.parallax) memset(D.parallax, 0, sizeof(float) * 8);
  if (D.status) memset(D.status, 0, 8 * N);
  TvModels M;
  int rc = models(M);
  if (rc < 0) return rc;
  const float SH = M.top[0], SF = M.top[1];
  if (D.SH) *D.SH = SH;
  if (D.SF) *D.SF = SF;
  if (D.best_it) memcpy(D.best_it, M.best, sizeof(M.best));
  if (D.H21) memcpy(D.H21, M.M, 9 * sizeof(float));
  if (D.F21) memcpy(D.F21, M.M + 9, 9 * sizeof(float));
  if (D.inliersH) memcpy(D.inliersH, M.mask.data(), N);
  if (D.inliersF) memcpy(D.inliersF, M.mask.data() + N, N);
  if (D.score) memcpy(D.score, M.score.data(), 2 * I * sizeof(float));
  if (SH + SF == 0.f) return 0;                          // :111
  const float RH = SH / (SH + SF);
  const int model = (double)RH > 0.50 ? 0 : 1;           // :117
  if (D.used_H) *D.used_H = model == 0;
  int inliers = 0;
  for (size_t i = 0; i < N; i++) inliers += M.mask[model * N + i];
  float ws[TV_WS_FLOATS], T[8 * 12];
  double W[TV_WS_DOUBLES];
  const int nhyp = model == 0 ? tv_hypotheses_H(M.M, K, ws, W, T) : tv_hypotheses_F(M.M + 9, K, ws, W, T);
  if (D.nhyp) *D.nhyp = nhyp;
  if (nhyp == 0) return 0;                               // :601
  for (int h = 0; h < nhyp; h++)
    for (int i = 0; i < 3; i++) {
      if (D.R) memcpy(D.R + 9 * h + 3 * i, T + 12 * h + 4 * i, 3 * sizeof(float));
      if (D.t) D.t[3 * h + i] = T[12 * h + 4 * i + 3];
    }
  TvChecked C;
  if ((rc = check(model, nhyp, T, C)) < 0) return rc;
  if (D.nGood) memcpy(D.nGood, C.nGood, sizeof(int32_t) * nhyp);
  if (D.parallax) memcpy(D.parallax, C.parallax, sizeof(float) * nhyp);
  if (D.status) memcpy(D.status, C.status.data(), (size_t)nhyp * N);
  const int chosen = model == 0 ? tv_select_H(C.nGood, C.parallax, inliers) : tv_select_F(C.nGood, C.parallax, inliers);
  if (D.chosen) *D.chosen = chosen;
  if (chosen < 0) return 0;
  for (int i = 0; i < 3; i++) {
    memcpy(R21 + 3 * i, T + 12 * chosen + 4 * i, 3 * sizeof(float));
    t21[i] = T[12 * chosen + 4 * i + 3];
  }
  memcpy(vP3D, C.p3d.data() + 3 * n1 * chosen, 3 * n1 * sizeof(float));
  memcpy(vbTriangulated, C.good.data() + n1 * chosen, n1);
  return 1;
}
}  // extern "C++"

static thread_local const char *g_two_view_host_err = "";
const char *orbm_two_view_host_error(void) { return g_two_view_host_err; }

static const char *two_view_refusal(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                    const float *K, int iterations, const int32_t *sets, const float *R21, const float *t21, const float *vP3D,
                                    const uint8_t *vbTriangulated, TvProblem &Q) {
  if (!K || !R21 || !t21 || !vP3D || !vbTriangulated) return "TwoViewReconstruction: NULL argument";
  if (const char *why = two_view_problem(keys1, n1, keys2, n2, matches12, 8, Q)) return why;
  return two_view_sets(Q, iterations, sets);
}

int orbm_two_view_reconstruct_host(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                   const float *K, float sigma, int iterations, const int32_t *sets, float *R21, float *t21, float *vP3D,
                                   uint8_t *vbTriangulated, const orbm_two_view_details_t *details) {
  TvProblem Q;
  if (const char *why = two_view_refusal(keys1, n1, keys2, n2, matches12, K, iterations, sets, R21, t21, vP3D, vbTriangulated, Q)) {
    g_two_view_host_err = why;
    return ORBX_E_ARG;
  }
  two_view_normalize(Q);
  const uint8_t *masks = nullptr;
  return two_view_reconstruct(
      Q, K, sigma, iterations, R21, t21, vP3D, vbTriangulated, details,
      [&](TvModels &M) { two_view_models_cpu(Q, sigma, iterations, sets, M); masks = M.mask.data(); return 0; },
      [&](int model, int nhyp, const float *T, TvChecked &C) {
        two_view_check_cpu(Q, masks + (size_t)model * Q.N, K, sigma, nhyp, T, C);
        return 0;
      });
}

int orbm_two_view_reconstruct(orbm_t *m, const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                              const float *K, float sigma, int iterations, const int32_t *sets, float *R21, float *t21, float *vP3D,
                              uint8_t *vbTriangulated, const orbm_two_view_details_t *details) {
  if (!m) return ORBX_E_ARG;
  TvProblem Q;
  if (const char *why = two_view_refusal(keys1, n1, keys2, n2, matches12, K, iterations, sets, R21, t21, vP3D, vbTriangulated, Q)) {
    m->err = why;
    return ORBX_E_ARG;
  }
  two_view_normalize(Q);
  MCHECK(m, hipSetDevice(m->device));
  TvDevice D{m, Staging{m}};
  const int rc = D.upload(Q, iterations, sets, 8, nullptr);
  if (rc < 0) return rc;
  return two_view_reconstruct(
      Q, K, sigma, iterations, R21, t21, vP3D, vbTriangulated, details, [&](TvModels &M) { return D.models(Q, sigma, M); },
      [&](int model, int nhyp, const float *T, TvChecked &C) { return D.check(K, sigma, nhyp, T, D.S.dev(D.mask) + (size_t)model * Q.N, C); });
}

static const char *two_view_models_refusal(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                           int iterations, const int32_t *sets, const float *H21, const float *H12, const float *F21,
                                           const float *score, const int32_t *best_it, const uint8_t *masks, TvProblem &Q) {
  if (!H21 || !H12 || !F21 || !score || !best_it || !masks) return "TwoViewReconstruction: NULL argument";
  if (const char *why = two_view_problem(keys1, n1, keys2, n2, matches12, 8, Q)) return why;
  return two_view_sets(Q, iterations, sets);
}
static void two_view_models_out(const TvModels &M, int iterations, int N, float *H21, float *H12, float *F21, float *score, int32_t *best_it,
                                uint8_t *masks) {
  const size_t I = (size_t)iterations;
  memcpy(H21, M.H21.data(), 9 * I * sizeof(float)); memcpy(H12, M.H12.data(), 9 * I * sizeof(float));
  memcpy(F21, M.F21.data(), 9 * I * sizeof(float)); memcpy(score, M.score.data(), 2 * I * sizeof(float));
  memcpy(best_it, M.best, sizeof(M.best)); memcpy(masks, M.mask.data(), 2 * (size_t)N);
}
int orbm_two_view_models_host(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12, float sigma,
                              int iterations, const int32_t *sets, float *H21, float *H12, float *F21, float *score, int32_t *best_it,
                              uint8_t *masks) {
  TvProblem Q;
  if (const char *why = two_view_models_refusal(keys1, n1, keys2, n2, matches12, iterations, sets, H21, H12, F21, score, best_it, masks, Q)) {
    g_two_view_host_err = why;
    return ORBX_E_ARG;
  }
  two_view_normalize(Q);
  TvModels M;
  two_view_models_cpu(Q, sigma, iterations, sets, M);
  two_view_models_out(M, iterations, Q.N, H21, H12, F21, score, best_it, masks);
  return 0;
}
int orbm_two_view_models(orbm_t *m, const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                         float sigma, int iterations, const int32_t *sets, float *H21, float *H12, float *F21, float *score, int32_t *best_it,
                         uint8_t *masks) {
  if (!m) return ORBX_E_ARG;
  TvProblem Q;
  if (const char *why = two_view_models_refusal(keys1, n1, keys2, n2, matches12, iterations, sets, H21, H12, F21, score, best_it, masks, Q)) {
    m->err = why;
    return ORBX_E_ARG;
  }
  two_view_normalize(Q);
  MCHECK(m, hipSetDevice(m->device));
  TvDevice D{m, Staging{m}};
  int rc = D.upload(Q, iterations, sets, 0, nullptr);
  if (rc < 0) return rc;
  TvModels M;
  if ((rc = D.models(Q, sigma, M)) < 0) return rc;
  two_view_models_out(M, iterations, Q.N, H21, H12, F21, score, best_it, masks);
  return 0;
}

static const char *two_view_check_refusal(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                          const uint8_t *inliers, const float *K, int nhyp, const float *R, const float *t, const float *vP3D,
                                          const uint8_t *vbGood, const uint8_t *status, const int32_t *nGood, const float *cos_rank,
                                          const float *parallax, TvProblem &Q, float *T) {
  if (!inliers || !K || !R || !t || !vP3D || !vbGood || !status || !nGood || !cos_rank || !parallax) return "TwoViewReconstruction: NULL argument";
  if (nhyp < 1 || nhyp > 8) return "TwoViewReconstruction: nhyp outside [1, 8]";
  if (const char *why = two_view_problem(keys1, n1, keys2, n2, matches12, 1, Q)) return why;
  for (int h = 0; h < nhyp; h++) tv_store_hypothesis(R + 9 * h, t + 3 * h, 1.f, T + 12 * h);
  return nullptr;
}
static void two_view_check_out(const TvChecked &C, int nhyp, float *vP3D, uint8_t *vbGood, uint8_t *status, int32_t *nGood, float *cos_rank,
                               float *parallax) {
  memcpy(vP3D, C.p3d.data(), C.p3d.size() * sizeof(float)); memcpy(vbGood, C.good.data(), C.good.size());
  memcpy(status, C.status.data(), C.status.size());
  memcpy(nGood, C.nGood, sizeof(int32_t) * nhyp); memcpy(cos_rank, C.cos_rank, sizeof(float) * nhyp);
  memcpy(parallax, C.parallax, sizeof(float) * nhyp);
}
int orbm_two_view_check_rt_host(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                const uint8_t *inliers, const float *K, float sigma, int nhyp, const float *R, const float *t, float *vP3D,
                                uint8_t *vbGood, uint8_t *status, int32_t *nGood, float *cos_rank, float *parallax) {
  TvProblem Q;
  float T[8 * 12];
  if (const char *why = two_view_check_refusal(keys1, n1, keys2, n2, matches12, inliers, K, nhyp, R, t, vP3D, vbGood, status, nGood, cos_rank,
                                               parallax, Q, T)) {
    g_two_view_host_err = why;
    return ORBX_E_ARG;
  }
  TvChecked C;
  two_view_check_cpu(Q, inliers, K, sigma, nhyp, T, C);
  two_view_check_out(C, nhyp, vP3D, vbGood, status, nGood, cos_rank, parallax);
  return 0;
}
int orbm_two_view_check_rt(orbm_t *m, const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                           const uint8_t *inliers, const float *K, float sigma, int nhyp, const float *R, const float *t, float *vP3D,
                           uint8_t *vbGood, uint8_t *status, int32_t *nGood, float *cos_rank, float *parallax) {
  if (!m) return ORBX_E_ARG;
  TvProblem Q;
  float T[8 * 12];
  if (const char *why = two_view_check_refusal(keys1, n1, keys2, n2, matches12, inliers, K, nhyp, R, t, vP3D, vbGood, status, nGood, cos_rank,
                                               parallax, Q, T)) {
    m->err = why;
    return ORBX_E_ARG;
  }
  MCHECK(m, hipSetDevice(m->device));
  TvDevice D{m, Staging{m}};
  int rc = D.upload(Q, 0, nullptr, nhyp, inliers);
  if (rc < 0) return rc;
  TvChecked C;
  if ((rc = D.check(K, sigma, nhyp, T, D.S.dev(D.mask_in), C)) < 0) return rc;
  two_view_check_out(C, nhyp, vP3D, vbGood, status, nGood, cos_rank, parallax);
  return 0;
}

// ---- Sim3Solver (Sim3Solver.cc:35-530): orb_ref_sim3.h, orb_sim3_kernels.h ----
// What the constructor leaves behind (:85-147): camera coordinates, their projections and the thresholds of the N kept pairs
struct Sim3Problem {
  const orbm_sim3_problem_t *p;
  size_t N, n1;
  std::vector<float> X1, X2, im1, im2, th1, th2;
};
// What is refused before anything is uploaded, launched or written (include/orbhip.h); nullptr = accepted
static const char *sim3_problem(const orbm_sim3_problem_t *p, Sim3Problem &Q) {
  if (!p) return "Sim3Solver: NULL argument";
  if (p->n1 < 0 || p->N < 0) return "Sim3Solver: negative count";
  if (p->N > p->n1) return "Sim3Solver: N > n1";
  if (!p->Tcw1 || !p->Tcw2 || !p->cam_params1 || !p->cam_params2) return "Sim3Solver: NULL argument";
  if (p->N > 0 && (!p->idx1 || !p->Xw1 || !p->Xw2 || !p->sigma2_1 || !p->sigma2_2)) return "Sim3Solver: NULL argument";
  if (p->cam_type1 < 0 || p->cam_type1 > 1 || p->cam_type2 < 0 || p->cam_type2 > 1) return "Sim3Solver: unknown camera type";
  if (p->min_inliers < 0) return "Sim3Solver: min_inliers < 0";
  if (p->iterations_done < 0) return "Sim3Solver: iterations_done < 0";
  for (int i = 0; i < p->N; i++) {
    if (p->idx1[i] < 0 || p->idx1[i] >= p->n1) return "Sim3Solver: idx1 outside [0, n1)";
    if (i > 0 && p->idx1[i] <= p->idx1[i - 1]) return "Sim3Solver: idx1 not ascending";
    if (!sim3_sigma2_ok(p->sigma2_1[i]) || !sim3_sigma2_ok(p->sigma2_2[i])) return "Sim3Solver: sigma2 negative, not finite or too large";
  }
  Q.p = p; Q.N = (size_t)p->N; Q.n1 = (size_t)p->n1;
  return nullptr;
}
static const char *sim3_sets(const Sim3Problem &Q, int iterations, const int32_t *sets) {
  if (iterations < 1) return "Sim3Solver: iterations < 1";
  if (!sets) return "Sim3Solver: NULL argument";
  if (Q.N < 3) return "Sim3Solver: fewer than 3 pairs";
  for (size_t k = 0; k < (size_t)iterations; k++) {
    const int32_t *s = sets + 3 * k;
    for (int j = 0; j < 3; j++)
      if (s[j] < 0 || (size_t)s[j] >= Q.N) return "Sim3Solver: set index outside [0, N)";
    if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2]) return "Sim3Solver: set index repeated within a set";
  }
  return nullptr;
}
static void sim3_construct(Sim3Problem &Q) {   // :128-132, :143-144, :119-120
  const orbm_sim3_problem_t &p = *Q.p;
  Q.X1.resize(3 * Q.N); Q.X2.resize(3 * Q.N); Q.im1.resize(2 * Q.N); Q.im2.resize(2 * Q.N); Q.th1.resize(Q.N); Q.th2.resize(Q.N);
  for (size_t i = 0; i < Q.N; i++) {
    sim3_transform(p.Tcw1, p.Xw1 + 3 * i, &Q.X1[3 * i]);
    sim3_transform(p.Tcw2, p.Xw2 + 3 * i, &Q.X2[3 * i]);
    sim3_project(p.cam_type1, p.cam_params1, &Q.X1[3 * i], &Q.im1[2 * i]);
    sim3_project(p.cam_type2, p.cam_params2, &Q.X2[3 * i], &Q.im2[2 * i]);
    Q.th1[i] = sim3_max_error(p.sigma2_1[i]);
    Q.th2[i] = sim3_max_error(p.sigma2_2[i]);
  }
}
static int sim3_cam_floats(int cam_type) { return cam_type == 0 ? 4 : 8; }

static void sim3_gather(const Sim3Problem &Q, const int32_t *set, float *P1, float *P2) {   // copyTo(P3Dc1i.col(i)) :208-209
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) { P1[3 * r + c] = Q.X1[3 * (size_t)set[c] + r]; P2[3 * r + c] = Q.X2[3 * (size_t)set[c] + r]; }
}
// The outputs of the hypothesis stage on the host: per iteration the tail's result and the quaternion row
struct Sim3Hyps { std::vector<Sim3Hyp> H; std::vector<float> quat; };
static void sim3_hypotheses_cpu(const Sim3Problem &Q, int iterations, const int32_t *sets, Sim3Hyps &R) {
  R.H.resize((size_t)iterations); R.quat.resize(4 * (size_t)iterations);
  for (size_t it = 0; it < (size_t)iterations; it++) {
    float P1[9], P2[9];
    sim3_gather(Q, sets + 3 * it, P1, P2);
    Sim3Set S;
    float ws[SIM3_WS_FLOATS];
    int iw[SIM3_WS_INTS];
    sim3_quaternion(P1, P2, S, &R.quat[4 * it], ws, iw);
    sim3_tail(S, &R.quat[4 * it], Q.p->fix_scale != 0, R.H[it]);
  }
}
static void sim3_check_cpu(const Sim3Problem &Q, size_t nhyp, const float *T /*[nhyp][32]*/, int32_t *counts, uint8_t *masks) {
  const orbm_sim3_problem_t &p = *Q.p;
  for (size_t h = 0; h < nhyp; h++) {
    int count = 0;
    for (size_t i = 0; i < Q.N; i++) {
      const bool in = sim3_inlier(T + 32 * h, T + 32 * h + 16, p.cam_type1, p.cam_params1, p.cam_type2, p.cam_params2, &Q.X1[3 * i],
                                  &Q.X2[3 * i], &Q.im1[2 * i], &Q.im2[2 * i], Q.th1[i], Q.th2[i]);
      masks[h * Q.N + i] = in;
      count += in;
    }
    counts[h] = count;
  }
}
static void sim3_pack(const Sim3Hyps &R, std::vector<float> &T) {
  T.resize(32 * R.H.size());
  for (size_t h = 0; h < R.H.size(); h++) { memcpy(&T[32 * h], R.H[h].T12, 64); memcpy(&T[32 * h + 16], R.H[h].T21, 64); }
}

// The device side: one staged block.  Inputs first, then T (uploaded behind the host tail), then the outputs, one span down.
struct Sim3Device {
  orbm_t *m;
  Staging S;
  PartOf<float> X1, X2, im1, im2, th1, th2, T, set_out;
  PartOf<int32_t> idx1, sets, counts, pass;
  PartOf<uint64_t> words;
  PartOf<uint8_t> best_mask, vb;
  size_t I, N, n1, W;
  double wall_ms[4] = {0, 0, 0, 0};   // orbm_sim3_details_t::wall_ms; [0] is the caller's
  using Clock = std::chrono::steady_clock;
  static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
  int upload(const Sim3Problem &Q, size_t iterations, const int32_t *set_idx) {
    I = iterations; N = Q.N; n1 = Q.n1; W = (N + 63) / 64;
    X1 = S.add(Q.X1.data(), 3 * N); X2 = S.add(Q.X2.data(), 3 * N); im1 = S.add(Q.im1.data(), 2 * N); im2 = S.add(Q.im2.data(), 2 * N);
    th1 = S.add(Q.th1.data(), N); th2 = S.add(Q.th2.data(), N); idx1 = S.add(Q.p->idx1, N); sets = S.add(set_idx, set_idx ? 3 * I : 0);
    T = S.out<float>(32 * I); set_out = S.out<float>(set_idx ? SIM3_SET_FLOATS * I : 0);
    counts = S.out<int32_t>(I); words = S.out<uint64_t>(I * W); pass = S.out<int32_t>(8); best_mask = S.out<uint8_t>(N); vb = S.out<uint8_t>(n1 + 1);
    return S.upload(m->stream);
  }
  Sim3Params params(const Sim3Problem &Q) const {
    const orbm_sim3_problem_t &p = *Q.p;
    Sim3Params P = {};
    P.X1 = S.dev(X1); P.X2 = S.dev(X2); P.im1 = S.dev(im1); P.im2 = S.dev(im2); P.th1 = S.dev(th1); P.th2 = S.dev(th2);
    P.idx1 = S.dev(idx1); P.sets = S.dev(sets);
    P.iterations = (int)I; P.N = (int)N; P.n1 = (int)n1; P.words = (int)W;
    P.cam1 = p.cam_type1; P.cam2 = p.cam_type2;
    memcpy(P.p1, p.cam_params1, sizeof(float) * sim3_cam_floats(p.cam_type1));
    memcpy(P.p2, p.cam_params2, sizeof(float) * sim3_cam_floats(p.cam_type2));
    P.set_out = S.dev(set_out); P.T = S.dev(T); P.counts = S.dev(counts); P.mask_words = S.dev(words);
    P.pass = S.dev(pass); P.best_mask = S.dev(best_mask); P.vb = S.dev(vb);
    return P;
  }
  // k_sim3_hypotheses, the sets' centred points and quaternions down, the first synchronisation, the tail on the host
  int hypotheses(const Sim3Problem &Q, Sim3Hyps &R) {
    hipStream_t s = m->stream;
    const Sim3Params P = params(Q);
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, s, P);
    MCHECK(m, hipGetLastError());
    MCHECK(m, hipMemcpyAsync(S.host(set_out), S.dev(set_out), sizeof(float) * SIM3_SET_FLOATS * I, hipMemcpyDeviceToHost, s));
    MCHECK(m, hipStreamSynchronize(s));
    const Clock::time_point t_tail = Clock::now();
    R.H.resize(I); R.quat.resize(4 * I);
    const float *o = S.host(set_out);
    for (size_t it = 0; it < I; it++, o += SIM3_SET_FLOATS) {
      Sim3Set set;
      memcpy(&set, o, sizeof(set));
      memcpy(&R.quat[4 * it], o + 24, 4 * sizeof(float));
      sim3_tail(set, o + 24, Q.p->fix_scale != 0, R.H[it]);
    }
    wall_ms[2] = ms_since(t_tail);
    return 0;
  }
  // T up, k_sim3_check, with `winner` k_sim3_winner, everything down, one synchronisation.  masks: [I][N] bytes or NULL
  int check(const Sim3Problem &Q, const float *Tpacked, bool winner, int best_in, int32_t *counts_out, uint8_t *masks, Sim3Pass *pass_out,
            uint8_t *best_mask_out, uint8_t *vb_out) {
    hipStream_t s = m->stream;
    const Clock::time_point t_check = Clock::now();
    memcpy(S.host(T), Tpacked, sizeof(float) * 32 * I);
    MCHECK(m, hipMemcpyAsync(S.dev(T), S.host(T), sizeof(float) * 32 * I, hipMemcpyHostToDevice, s));
    Sim3Params P = params(Q);
    P.best_in = best_in; P.min_inliers = Q.p->min_inliers; P.done = Q.p->iterations_done; P.max_its = Q.p->max_iterations;
    hipLaunchKernelGGL(k_sim3_check, dim3((unsigned)I), dim3(64), 0, s, P);
    MCHECK(m, hipGetLastError());
    if (winner) {
      hipLaunchKernelGGL(k_sim3_winner, dim3(1), dim3(256), 0, s, P);
      MCHECK(m, hipGetLastError());
    }
    MCHECK(m, S.download(s, counts, vb));
    MCHECK(m, hipStreamSynchronize(s));
    wall_ms[3] = ms_since(t_check);
    if (counts_out) memcpy(counts_out, S.host(counts), sizeof(int32_t) * I);
    if (masks) {
      const uint64_t *w = S.host(words);
      for (size_t it = 0; it < I; it++)
        for (size_t i = 0; i < N; i++) masks[it * N + i] = (uint8_t)((w[it * W + (i >> 6)] >> (i & 63)) & 1);
    }
    if (winner) {
      const int32_t *ps = S.host(pass);
      *pass_out = Sim3Pass{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5]};
      memcpy(best_mask_out, S.host(best_mask), N);
      memcpy(vb_out, S.host(vb), n1);
    }
    return 0;
  }
};

static thread_local const char *g_sim3_host_err = "";
const char *orbm_sim3_host_error(void) { return g_sim3_host_err; }

static void sim3_no_more(const Sim3Problem &Q, int best_in, orbm_sim3_result_t *r) {   // :182-186, :252-256
  uint8_t *bm = r->best_mask, *vb = r->vbInliers;
  memset(r, 0, sizeof(*r));
  r->best_mask = bm; r->vbInliers = vb;
  r->best_it = -1; r->best_inliers = best_in; r->no_more = 1;
  memset(bm, 0, Q.N); memset(vb, 0, Q.n1);
}
// The result and the details from the pass and every iteration's hypothesis
static void sim3_result(const Sim3Problem &Q, size_t I, const Sim3Pass &pass, const Sim3Hyps &R, const int32_t *counts, const uint8_t *masks,
                        orbm_sim3_result_t *r, const orbm_sim3_details_t *d) {
  r->converged = pass.converged; r->it_stop = pass.it_stop; r->best_it = pass.best_it; r->best_inliers = pass.best_inliers;
  r->improved = pass.improved; r->no_more = pass.no_more;
  memset(r->T12, 0, sizeof(r->T12)); memset(r->R12, 0, sizeof(r->R12)); memset(r->t12, 0, sizeof(r->t12)); r->s12 = 0.f;
  if (pass.best_it >= 0) {
    const Sim3Hyp &H = R.H[(size_t)pass.best_it];
    memcpy(r->T12, H.T12, sizeof(r->T12)); memcpy(r->R12, H.R, sizeof(r->R12)); memcpy(r->t12, H.t, sizeof(r->t12)); r->s12 = H.s;
  }
  if (!d) return;
  if (d->counts) memcpy(d->counts, counts, sizeof(int32_t) * I);
  if (d->masks) memcpy(d->masks, masks, I * Q.N);
  for (size_t it = 0; it < I; it++) {
    if (d->T12) memcpy(d->T12 + 16 * it, R.H[it].T12, 64);
    if (d->T21) memcpy(d->T21 + 16 * it, R.H[it].T21, 64);
  }
  if (d->quat) memcpy(d->quat, R.quat.data(), sizeof(float) * 4 * I);
  if (d->wall_ms) memset(d->wall_ms, 0, 4 * sizeof(double));
}
// 0: go on; 1: answered without a launch (N < min_inliers); the refusal's text otherwise
static const char *sim3_solve_refusal(const orbm_sim3_problem_t *p, int iterations, const int32_t *sets, orbm_sim3_result_t *r, Sim3Problem &Q,
                                      bool &no_more) {
  no_more = false;
  if (!r || !r->best_mask || !r->vbInliers) return "Sim3Solver: NULL argument";
  if (const char *why = sim3_problem(p, Q)) return why;
  if (iterations < 1) return "Sim3Solver: iterations < 1";
  if (!sets) return "Sim3Solver: NULL argument";
  if (p->N < p->min_inliers) { no_more = true; return nullptr; }
  return sim3_sets(Q, iterations, sets);
}

int orbm_sim3_solve_host(const orbm_sim3_problem_t *p, int iterations, const int32_t *sets, int best_inliers_in, orbm_sim3_result_t *r,
                         const orbm_sim3_details_t *d) {
  Sim3Problem Q;
  bool no_more;
  if (const char *why = sim3_solve_refusal(p, iterations, sets, r, Q, no_more)) { g_sim3_host_err = why; return ORBX_E_ARG; }
  if (no_more) { sim3_no_more(Q, best_inliers_in, r); return 0; }
  sim3_construct(Q);
  const size_t I = (size_t)iterations;
  Sim3Hyps R;
  sim3_hypotheses_cpu(Q, iterations, sets, R);
  std::vector<float> T;
  sim3_pack(R, T);
  std::vector<int32_t> counts(I);
  std::vector<uint8_t> masks(I * Q.N);
  sim3_check_cpu(Q, I, T.data(), counts.data(), masks.data());
  const Sim3Pass pass = sim3_ordered_pass(counts.data(), iterations, best_inliers_in, p->min_inliers, p->iterations_done, p->max_iterations);
  memset(r->best_mask, 0, Q.N); memset(r->vbInliers, 0, Q.n1);
  if (pass.best_it >= 0) memcpy(r->best_mask, &masks[(size_t)pass.best_it * Q.N], Q.N);
  if (pass.converged)
    for (size_t i = 0; i < Q.N; i++)
      if (r->best_mask[i]) r->vbInliers[p->idx1[i]] = 1;   // :231-233
  sim3_result(Q, I, pass, R, counts.data(), masks.data(), r, d);
  return 0;
}

int orbm_sim3_solve(orbm_t *m, const orbm_sim3_problem_t *p, int iterations, const int32_t *sets, int best_inliers_in, orbm_sim3_result_t *r,
                    const orbm_sim3_details_t *d) {
  if (!m) return ORBX_E_ARG;
  Sim3Problem Q;
  bool no_more;
  if (const char *why = sim3_solve_refusal(p, iterations, sets, r, Q, no_more)) { m->err = why; return ORBX_E_ARG; }
  if (no_more) { sim3_no_more(Q, best_inliers_in, r); return 0; }
  const Sim3Device::Clock::time_point t0 = Sim3Device::Clock::now();
  sim3_construct(Q);
  MCHECK(m, hipSetDevice(m->device));
  const size_t I = (size_t)iterations;
  Sim3Device D{m, Staging{m}};
  D.wall_ms[0] = Sim3Device::ms_since(t0);
  const Sim3Device::Clock::time_point t1 = Sim3Device::Clock::now();
  int rc = D.upload(Q, I, sets);
  if (rc < 0) return rc;
  Sim3Hyps R;
  if ((rc = D.hypotheses(Q, R)) < 0) return rc;
  D.wall_ms[1] = Sim3Device::ms_since(t1) - D.wall_ms[2];
  std::vector<float> T;
  sim3_pack(R, T);
  std::vector<int32_t> counts(I);
  std::vector<uint8_t> masks(d && d->masks ? I * Q.N : 0);
  Sim3Pass pass;
  if ((rc = D.check(Q, T.data(), true, best_inliers_in, counts.data(), masks.empty() ? nullptr : masks.data(), &pass, r->best_mask,
                    r->vbInliers)) < 0)
    return rc;
  sim3_result(Q, I, pass, R, counts.data(), masks.data(), r, d);
  if (d && d->wall_ms) memcpy(d->wall_ms, D.wall_ms, sizeof(D.wall_ms));
  return 0;
}

static const char *sim3_hypotheses_refusal(const orbm_sim3_problem_t *p, int iterations, const int32_t *sets, const float *T12, const float *T21,
                                           const float *quat, Sim3Problem &Q) {
  if (!T12 || !T21 || !quat) return "Sim3Solver: NULL argument";
  if (const char *why = sim3_problem(p, Q)) return why;
  return sim3_sets(Q, iterations, sets);
}
static void sim3_hypotheses_out(const Sim3Hyps &R, float *T12, float *T21, float *quat) {
  for (size_t it = 0; it < R.H.size(); it++) { memcpy(T12 + 16 * it, R.H[it].T12, 64); memcpy(T21 + 16 * it, R.H[it].T21, 64); }
  memcpy(quat, R.quat.data(), sizeof(float) * R.quat.size());
}
int orbm_sim3_hypotheses_host(const orbm_sim3_problem_t *p, int iterations, const int32_t *sets, float *T12, float *T21, float *quat) {
  Sim3Problem Q;
  if (const char *why = sim3_hypotheses_refusal(p, iterations, sets, T12, T21, quat, Q)) { g_sim3_host_err = why; return ORBX_E_ARG; }
  sim3_construct(Q);
  Sim3Hyps R;
  sim3_hypotheses_cpu(Q, iterations, sets, R);
  sim3_hypotheses_out(R, T12, T21, quat);
  return 0;
}
int orbm_sim3_hypotheses(orbm_t *m, const orbm_sim3_problem_t *p, int iterations, const int32_t *sets, float *T12, float *T21, float *quat) {
  if (!m) return ORBX_E_ARG;
  Sim3Problem Q;
  if (const char *why = sim3_hypotheses_refusal(p, iterations, sets, T12, T21, quat, Q)) { m->err = why; return ORBX_E_ARG; }
  sim3_construct(Q);
  MCHECK(m, hipSetDevice(m->device));
  Sim3Device D{m, Staging{m}};
  int rc = D.upload(Q, (size_t)iterations, sets);
  if (rc < 0) return rc;
  Sim3Hyps R;
  if ((rc = D.hypotheses(Q, R)) < 0) return rc;
  sim3_hypotheses_out(R, T12, T21, quat);
  return 0;
}

static const char *sim3_check_refusal(const orbm_sim3_problem_t *p, int nhyp, const float *T12, const float *T21, const int32_t *counts,
                                      const uint8_t *masks, Sim3Problem &Q, std::vector<float> &T) {
  if (!T12 || !T21 || !counts || !masks) return "Sim3Solver: NULL argument";
  if (const char *why = sim3_problem(p, Q)) return why;
  if (nhyp < 1) return "Sim3Solver: nhyp < 1";
  if (Q.N < 1) return "Sim3Solver: no pair";
  T.resize(32 * (size_t)nhyp);
  for (size_t h = 0; h < (size_t)nhyp; h++) { memcpy(&T[32 * h], T12 + 16 * h, 64); memcpy(&T[32 * h + 16], T21 + 16 * h, 64); }
  return nullptr;
}
int orbm_sim3_check_host(const orbm_sim3_problem_t *p, int nhyp, const float *T12, const float *T21, int32_t *counts, uint8_t *masks) {
  Sim3Problem Q;
  std::vector<float> T;
  if (const char *why = sim3_check_refusal(p, nhyp, T12, T21, counts, masks, Q, T)) { g_sim3_host_err = why; return ORBX_E_ARG; }
  sim3_construct(Q);
  sim3_check_cpu(Q, (size_t)nhyp, T.data(), counts, masks);
  return 0;
}
int orbm_sim3_check(orbm_t *m, const orbm_sim3_problem_t *p, int nhyp, const float *T12, const float *T21, int32_t *counts, uint8_t *masks) {
  if (!m) return ORBX_E_ARG;
  Sim3Problem Q;
  std::vector<float> T;
  if (const char *why = sim3_check_refusal(p, nhyp, T12, T21, counts, masks, Q, T)) { m->err = why; return ORBX_E_ARG; }
  sim3_construct(Q);
  MCHECK(m, hipSetDevice(m->device));
  Sim3Device D{m, Staging{m}};
  const int rc = D.upload(Q, (size_t)nhyp, nullptr);
  if (rc < 0) return rc;
  return D.check(Q, T.data(), false, 0, counts, masks, nullptr, nullptr, nullptr);
}

int orbm_sim3_ransac_iterations(double probability, int min_inliers, int max_its, int N) {
  return sim3_ransac_iterations(probability, min_inliers, max_its, N);
}

int orbm_knn_match2(orbm_t *m, const uint8_t *q, int nq, const uint8_t *c, int nc, int32_t *idx2, int32_t *dist2) {
  if (!m || nq < 0 || nc < 0 || (nq > 0 && (!q || !idx2 || !dist2)) || (nc > 0 && !c)) return ORBX_E_ARG;
  if (nq == 0) return 0;
  if (nc == 0) { for (int i = 0; i < 2 * nq; i++) { idx2[i] = -1; dist2[i] = -1; } return 0; }
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Staging S{m};
  const auto hq = S.add(q, 32 * (size_t)nq), hc = S.add(c, 32 * (size_t)nc);
  const auto hout = S.out<int32_t>(4 * (size_t)nq);   // idx, dist
  const int rs = S.upload(s, false);
  if (rs < 0) return rs;
  const uint32_t *d_q = (const uint32_t *)S.dev(hq), *d_c = (const uint32_t *)S.dev(hc);
  int32_t *d_idx = S.dev(hout), *d_dist = d_idx + 2 * (size_t)nq;
  // matrix-pipe form (orb_match_mfma.h) unless the vector-ALU engine is selected; its keys carry the train index in 20 bits
  if (m->hamming_engine >= 1 && nc < (1 << 20))
    hipLaunchKernelGGL(k_knn2_mfma, dim3((nq + MF_NT - 1) / MF_NT), dim3(MF_NT), 0, s, d_q, nq, d_c, nc, d_idx, d_dist);
  else
    hipLaunchKernelGGL(k_knn2, dim3((nq + 3) / 4), dim3(256), 0, s, d_q, nq, d_c, nc, d_idx, d_dist);
  MCHECK(m, hipGetLastError());
  MCHECK(m, hipMemcpyAsync(idx2, d_idx, sizeof(int32_t) * 2 * (size_t)nq, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipMemcpyAsync(dist2, d_dist, sizeof(int32_t) * 2 * (size_t)nq, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipStreamSynchronize(s));
  return 0;
}

int orbm_hamming_matrix(orbm_t *m, const uint8_t *q, int nq, const uint8_t *c, int nc, uint16_t *dist) {
  if (!m || !q || !c || !dist || nq <= 0 || nc <= 0) return ORBX_E_ARG;
  MCHECK(m, hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Staging S{m};
  const auto hq = S.add(q, 32 * (size_t)nq), hc = S.add(c, 32 * (size_t)nc);
  const auto hdist = S.out<uint16_t>((size_t)nq * nc);   // the nq x nc matrix, downloaded straight to the caller
  const int rs = S.upload(s, false);
  if (rs < 0) return rs;
  const uint32_t *d_q = (const uint32_t *)S.dev(hq), *d_c = (const uint32_t *)S.dev(hc);
  uint16_t *d_dist = S.dev(hdist);
  constexpr int QSLAB = 128;   // query rows per workgroup of the matrix-pipe form: four tiles behind one expansion of its 256 candidates
  if (m->hamming_engine >= 1 && (nq + QSLAB - 1) / QSLAB <= 65535)
    hipLaunchKernelGGL(k_hamming_matrix_mfma, dim3((nc + MF_NT - 1) / MF_NT, (nq + QSLAB - 1) / QSLAB), dim3(MF_NT), 0, s, d_q, nq, d_c, nc, d_dist, QSLAB);
  else
    hipLaunchKernelGGL(k_hamming_matrix, dim3((nq + 255) / 256), dim3(256), 0, s, d_q, nq, d_c, nc, d_dist);
  MCHECK(m, hipGetLastError());
  MCHECK(m, hipMemcpyAsync(dist, d_dist, sizeof(uint16_t) * (size_t)nq * nc, hipMemcpyDeviceToHost, s));
  MCHECK(m, hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"

// =====================================================================================================================================
// ORBVocabulary::transform (Frame::ComputeBoW, KeyFrame::ComputeBoW): csrc/orb_ref_voc.h on the host, csrc/orb_voc_kernels.h on the device
// =====================================================================================================================================

// What one call of orbv_transform owns while it runs: a stream, a device block and its pinned mirror.  Tracking and LocalMapping call
// into one vocabulary at the same time, so a call takes one from the handle's pool and gives it back; the tables are read-only.
struct VocWork {
  hipStream_t s = nullptr;
  uint8_t *dev = nullptr, *pin = nullptr;
  size_t bytes = 0;
};

struct orbv_handle {
  int device = -1;
  int k = 0, L = 0, weighting = 0, scoring = 0;
  int n_nodes = 0, n_words = 0, max_children = 0;
  int min_leaf_level = 0; uint32_t min_leaf_node = 0;   // the shallowest childless node of weight > 0 (the lowest id among those)
  std::vector<uint32_t> desc; std::vector<VocRec> rec; std::vector<double> weight;   // by entry
  uint32_t *d_desc = nullptr; VocRec *d_rec = nullptr; double *d_weight = nullptr;
  std::mutex mu;
  std::vector<VocWork *> pool;
};

static thread_local std::string g_voc_err;   // orbv_last_error: of the calling thread, so that concurrent calls do not share a string
static int voc_fail(const std::string &what) { g_voc_err = what; return ORBX_E_ARG; }
#define VCHECK(call)                                                        \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) {                                                 \
      g_voc_err = std::string(#call) + ": " + hipGetErrorString(e_);        \
      return ORBX_E_HIP;                                                    \
    }                                                                       \
  } while (0)

// k_voc_collect sorts up to 16384 8-byte keys: 128 KiB of dynamic LDS, above the 64 KiB a kernel gets unasked.  Raised once per device.
static LdsOnce g_voc_lds;

static void voc_free_work(VocWork *w) {
  if (!w) return;
  if (w->dev) (void)hipFree(w->dev);
  if (w->pin) (void)hipHostFree(w->pin);
  if (w->s) (void)hipStreamDestroy(w->s);
  delete w;
}

// the arguments every transform entry shares; nid_level out
static int voc_check(const orbv_handle *v, int levelsup, int *nid_level) {
  if (!v) return voc_fail("orbv: NULL handle");
  const long long lvl = (long long)v->L - (long long)levelsup;
  *nid_level = lvl > 0x7fffffff ? 0x7fffffff : lvl < 0 ? 0 : (int)lvl;
  if (v->n_words > 0 && *nid_level > 0 && v->min_leaf_level < *nid_level) {
    char buf[256];
    snprintf(buf, sizeof buf, "orbv_transform: node %u has no children and a weight > 0 at level %d, above level m_L - levelsup = %d - %d: the "
             "reference leaves the NodeId of a feature that ends there unset", v->min_leaf_node, v->min_leaf_level, v->L, levelsup);
    return voc_fail(buf);
  }
  return 0;
}

static void voc_launch(const orbv_handle *v, hipStream_t s, const uint8_t *d_q, LiveCount live, int cap, int nframes, int nid_level,
                       int32_t *d_entry, uint32_t *d_word, uint32_t *d_node, uint32_t *d_bow_id, double *d_bow_val, int32_t *d_n_bow,
                       uint32_t *d_fv_node_id, int32_t *d_fv_start, int32_t *d_fv_idx, int32_t *d_n_fv, int descend_form) {
  VocDescendParams D;
  D.desc = v->d_desc; D.rec = v->d_rec; D.q = d_q; D.n = live; D.cap = cap; D.nid_level = nid_level;
  D.entry = d_entry; D.word = d_word; D.node = d_node;
  if (descend_form == 1) hipLaunchKernelGGL(k_voc_descend_lane, dim3((unsigned)((cap + 255) / 256), (unsigned)nframes), dim3(256), 0, s, D);
  else hipLaunchKernelGGL(k_voc_descend, dim3((unsigned)((cap + 15) / 16), (unsigned)nframes), dim3(256), 0, s, D);
  VocCollectParams C;
  C.rec = v->d_rec; C.weight = v->d_weight; C.n = live; C.cap = cap; C.weighting = v->weighting; C.scoring = v->scoring;
  C.entry = d_entry; C.node = d_node; C.bow_id = d_bow_id; C.bow_val = d_bow_val; C.n_bow = d_n_bow;
  C.fv_node_id = d_fv_node_id; C.fv_start = d_fv_start; C.fv_idx = d_fv_idx; C.n_fv = d_n_fv;
  hipLaunchKernelGGL(k_voc_collect, dim3((unsigned)nframes), dim3(VOC_THREADS), SortCarve::of(cap).bytes, s, C);
}

extern "C" {

const char *orbv_last_error(const orbv_t *) { return g_voc_err.c_str(); }

void orbv_destroy(orbv_t *v) {
  if (!v) return;
  if (v->device >= 0) {
    (void)hipSetDevice(v->device);
    for (VocWork *w : v->pool) voc_free_work(w);
    if (v->d_desc) (void)hipFree(v->d_desc);
    if (v->d_rec) (void)hipFree(v->d_rec);
    if (v->d_weight) (void)hipFree(v->d_weight);
  }
  delete v;
}

orbv_t *orbv_create(const orbv_nodes_t *nodes, int device) {
  g_voc_err.clear();
  if (!nodes || nodes->n_nodes < 1 || !nodes->parent || !nodes->is_leaf || !nodes->descriptor || !nodes->weight || device < -1) {
    voc_fail("orbv_create: NULL table, n_nodes < 1 or device < -1");
    return nullptr;
  }
  if (nodes->scoring == VOC_L2_NORM) { voc_fail("orbv_create: L2_NORM scoring is not supported (csrc/orb_ref_voc.h)"); return nullptr; }
  if (nodes->scoring < 0 || nodes->scoring > VOC_DOT_PRODUCT || nodes->weighting < 0 || nodes->weighting > VOC_BINARY) {
    voc_fail("orbv_create: weighting outside [0, 3] or scoring outside [0, 5]");
    return nullptr;
  }
  const int N = nodes->n_nodes;
  for (int i = 1; i < N; i++)
    if (nodes->parent[i] >= (uint32_t)i) {   // the loader appends: a node's parent is loaded before it
      char buf[96];
      snprintf(buf, sizeof buf, "orbv_create: node %d has parent %u, not below its own id", i, nodes->parent[i]);
      voc_fail(buf);
      return nullptr;
    }
  orbv_handle *v = new orbv_handle;
  v->device = device; v->k = nodes->k; v->L = nodes->L; v->weighting = nodes->weighting; v->scoring = nodes->scoring; v->n_nodes = N;
  // children in ascending node id = the loader's push_back order (TemplatedVocabulary.h:1385-1392)
  std::vector<int32_t> nchild(N, 0), first(N + 1, 0), fill(N, 0), child(N > 1 ? N - 1 : 0);
  for (int i = 1; i < N; i++) nchild[nodes->parent[i]]++;
  for (int i = 0; i < N; i++) first[i + 1] = first[i] + nchild[i];
  for (int i = 1; i < N; i++) { const uint32_t p = nodes->parent[i]; child[first[p] + fill[p]++] = i; }
  // word ids over the flagged nodes in id order (:1408-1415); node 0 is not in the file and is never flagged by the loader
  std::vector<uint32_t> word(N, 0);
  for (int i = 1; i < N; i++) if (nodes->is_leaf[i]) word[i] = (uint32_t)v->n_words++;
  // entries: breadth first, so that the children of a node are contiguous and the upper levels share cache lines
  std::vector<int32_t> node_of(N), level(N, 0);
  v->rec.resize(N); v->desc.resize(8 * (size_t)N); v->weight.resize(N);
  node_of[0] = 0;
  int next = 1;
  v->min_leaf_level = 0x7fffffff;
  for (int e = 0; e < N; e++) {
    const int id = node_of[e];
    VocRec &r = v->rec[e];
    r.first = nchild[id] ? next : 0; r.count = nchild[id]; r.node = (uint32_t)id; r.word = word[id];
    for (int c = 0; c < nchild[id]; c++) { const int ch = child[first[id] + c]; level[next] = level[e] + 1; node_of[next++] = ch; }
    memcpy(&v->desc[8 * (size_t)e], nodes->descriptor + 32 * (size_t)id, 32);
    v->weight[e] = nodes->weight[id];
    v->max_children = std::max(v->max_children, nchild[id]);
    if (nchild[id] == 0 && nodes->weight[id] > 0 && (level[e] < v->min_leaf_level || (level[e] == v->min_leaf_level && (uint32_t)id < v->min_leaf_node))) {
      v->min_leaf_level = level[e]; v->min_leaf_node = (uint32_t)id;
    }
  }
  if (device < 0) return v;
  const hipError_t e0 = hipSetDevice(device);
  hipError_t e = e0;
  if (e == hipSuccess) e = raise_lds_once(g_voc_lds, device, {reinterpret_cast<const void *>(&k_voc_collect)});
  if (e == hipSuccess) e = hipMalloc(&v->d_desc, 32 * (size_t)N);
  if (e == hipSuccess) e = hipMalloc(&v->d_rec, sizeof(VocRec) * (size_t)N);
  if (e == hipSuccess) e = hipMalloc(&v->d_weight, sizeof(double) * (size_t)N);
  if (e == hipSuccess) e = hipMemcpy(v->d_desc, v->desc.data(), 32 * (size_t)N, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(v->d_rec, v->rec.data(), sizeof(VocRec) * (size_t)N, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(v->d_weight, v->weight.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    const std::string what = std::string("orbv_create: HIP: ") + hipGetErrorString(e);
    if (e0 != hipSuccess) v->device = -1;   // nothing of the device to free
    orbv_destroy(v);
    g_voc_err = what;
    return nullptr;
  }
  return v;
}

int orbv_n_nodes(const orbv_t *v) { return v ? v->n_nodes : ORBX_E_ARG; }
int orbv_n_words(const orbv_t *v) { return v ? v->n_words : ORBX_E_ARG; }
int orbv_max_children(const orbv_t *v) { return v ? v->max_children : ORBX_E_ARG; }
int orbv_min_leaf_level(const orbv_t *v) { return v ? v->min_leaf_level : ORBX_E_ARG; }

int orbv_transform_host(const orbv_t *v, const uint8_t *descriptors, int n, int levelsup, uint32_t *word_of_feature, uint32_t *node_of_feature,
                        uint32_t *bow_id, double *bow_val, int32_t *n_bow, uint32_t *fv_node_id, int32_t *fv_start, int32_t *fv_idx,
                        int32_t *n_fv) {
  int nid_level;
  const int rc = voc_check(v, levelsup, &nid_level);
  if (rc < 0) return rc;
  if (n < 0 || n > ORBM_MAX_KEYPOINTS) return voc_fail("orbv_transform_host: n outside [0, ORBM_MAX_KEYPOINTS]");
  if (!n_bow || !n_fv || !fv_start || (n > 0 && (!descriptors || !bow_id || !bow_val || !fv_node_id || !fv_idx)))
    return voc_fail("orbv_transform_host: NULL argument");
  std::map<uint32_t, double> bow;                      // DBoW2::BowVector
  std::map<uint32_t, std::vector<uint32_t>> fv;        // DBoW2::FeatureVector
  const bool adds = voc_adds_weight(v->weighting), must = voc_must_normalize(v->scoring);
  if (v->n_words > 0) {                                // empty() (:1134)
    for (int i = 0; i < n; i++) {
      uint32_t q[8];
      memcpy(q, descriptors + 32 * (size_t)i, 32);
      int32_t entry; uint32_t nid;
      voc_descend(v->desc.data(), v->rec.data(), q, nid_level, &entry, &nid);
      const uint32_t id = v->rec[entry].word;
      const double w = v->weight[entry];
      if (word_of_feature) word_of_feature[i] = id;
      if (node_of_feature) node_of_feature[i] = nid;
      if (w > 0) {                                     // :1157, :1185
        auto it = bow.lower_bound(id);
        const bool first = it == bow.end() || bow.key_comp()(id, it->first);
        if (first) it = bow.insert(it, std::make_pair(id, 0.0));
        voc_add(&it->second, w, first, adds);
        fv[nid].push_back((uint32_t)i);
      }
    }
    if (adds && !must && !bow.empty()) {               // :1164-1170
      const double nd = (double)bow.size();
      for (auto &kv : bow) kv.second = voc_div(kv.second, nd);
    }
    if (must) {                                        // BowVector::normalize(L1)
      double norm = 0.0;
      for (auto &kv : bow) voc_l1_step(&norm, kv.second);
      if (norm > 0.0) for (auto &kv : bow) kv.second = voc_div(kv.second, norm);
    }
  } else {
    for (int i = 0; i < n; i++) { if (word_of_feature) word_of_feature[i] = 0; if (node_of_feature) node_of_feature[i] = 0; }
  }
  int t = 0;
  for (const auto &kv : bow) { bow_id[t] = kv.first; bow_val[t] = kv.second; t++; }
  *n_bow = t;
  int g = 0, at = 0;
  for (const auto &kv : fv) {
    fv_node_id[g] = kv.first; fv_start[g] = at; g++;
    for (uint32_t i : kv.second) fv_idx[at++] = (int32_t)i;
  }
  fv_start[g] = at;
  *n_fv = g;
  return 0;
}

int orbv_transform(orbv_t *v, const uint8_t *descriptors, int n, int levelsup, uint32_t *word_of_feature, uint32_t *node_of_feature,
                   uint32_t *bow_id, double *bow_val, int32_t *n_bow, uint32_t *fv_node_id, int32_t *fv_start, int32_t *fv_idx,
                   int32_t *n_fv) {
  // everything is validated before anything is written or launched
  int nid_level;
  const int rc = voc_check(v, levelsup, &nid_level);
  if (rc < 0) return rc;
  if (v->device < 0) return voc_fail("orbv_transform: the handle was created with device = -1 and has no device tables");
  if (n < 0 || n > ORBM_MAX_KEYPOINTS) return voc_fail("orbv_transform: n outside [0, ORBM_MAX_KEYPOINTS]");
  if (!n_bow || !n_fv || !fv_start || (n > 0 && (!descriptors || !bow_id || !bow_val || !fv_node_id || !fv_idx)))
    return voc_fail("orbv_transform: NULL argument");
  if (n == 0 || v->n_words == 0) {
    for (int i = 0; i < n; i++) { if (word_of_feature) word_of_feature[i] = 0; if (node_of_feature) node_of_feature[i] = 0; }
    *n_bow = 0; *n_fv = 0; fv_start[0] = 0;
    return 0;
  }
  VCHECK(hipSetDevice(v->device));
  // one block: descriptors | entry | word | node | bow_id | fv_node_id | fv_idx | fv_start[n + 1] | n_bow, n_fv | bow_val (8-byte aligned)
  const size_t N = (size_t)n;
  const size_t o_entry = 32 * N, o_word = o_entry + 4 * N, o_node = o_word + 4 * N, o_bid = o_node + 4 * N, o_fnode = o_bid + 4 * N,
               o_fidx = o_fnode + 4 * N, o_fstart = o_fidx + 4 * N, o_cnt = o_fstart + 4 * (N + 1), o_bval = (o_cnt + 8 + 7) & ~(size_t)7,
               bytes = o_bval + 8 * N;
  // a workspace from the pool (or a new one) for the length of this call; it goes back on every way out
  struct Lease {
    orbv_handle *v; VocWork *w = nullptr;
    explicit Lease(orbv_handle *h) : v(h) {
      std::lock_guard<std::mutex> lock(v->mu);
      if (!v->pool.empty()) { w = v->pool.back(); v->pool.pop_back(); }
    }
    ~Lease() { if (w) { std::lock_guard<std::mutex> lock(v->mu); v->pool.push_back(w); } }
  } lease(v);
  if (!lease.w) lease.w = new VocWork;
  VocWork *w = lease.w;
  if (!w->s) VCHECK(hipStreamCreateWithFlags(&w->s, hipStreamNonBlocking));
  if (w->bytes < bytes) {
    if (w->dev) VCHECK(hipFree(w->dev));
    w->dev = nullptr;
    if (w->pin) VCHECK(hipHostFree(w->pin));
    w->pin = nullptr; w->bytes = 0;
    const size_t room = bytes + bytes / 2;
    VCHECK(hipMalloc(&w->dev, room));
    VCHECK(hipHostMalloc(&w->pin, room, hipHostMallocDefault));
    w->bytes = room;
  }
  memcpy(w->pin, descriptors, 32 * N);
  VCHECK(hipMemcpyAsync(w->dev, w->pin, 32 * N, hipMemcpyHostToDevice, w->s));
  uint8_t *d = w->dev;
  int32_t *d_cnt = (int32_t *)(d + o_cnt);
  voc_launch(v, w->s, d, LiveCount{nullptr, 0, n}, n, 1, nid_level, (int32_t *)(d + o_entry), (uint32_t *)(d + o_word), (uint32_t *)(d + o_node),
             (uint32_t *)(d + o_bid), (double *)(d + o_bval), d_cnt, (uint32_t *)(d + o_fnode), (int32_t *)(d + o_fstart), (int32_t *)(d + o_fidx),
             d_cnt + 1, 0);
  VCHECK(hipGetLastError());
  VCHECK(hipMemcpyAsync(w->pin + o_word, d + o_word, bytes - o_word, hipMemcpyDeviceToHost, w->s));
  VCHECK(hipStreamSynchronize(w->s));
  const uint8_t *h = w->pin;
  const int32_t nb = ((const int32_t *)(h + o_cnt))[0], nf = ((const int32_t *)(h + o_cnt))[1];
  const int32_t live = nf >= 0 && nf <= n ? ((const int32_t *)(h + o_fstart))[nf] : -1;
  if (nb < 0 || nb > n || nf < 0 || nf > n || live < 0 || live > n) { g_voc_err = "orbv_transform: the device returned counts outside [0, n]"; return ORBX_E_HIP; }
  if (word_of_feature) memcpy(word_of_feature, h + o_word, 4 * N);
  if (node_of_feature) memcpy(node_of_feature, h + o_node, 4 * N);
  memcpy(bow_id, h + o_bid, 4 * (size_t)nb);
  memcpy(bow_val, h + o_bval, 8 * (size_t)nb);
  memcpy(fv_node_id, h + o_fnode, 4 * (size_t)nf);
  memcpy(fv_start, h + o_fstart, 4 * ((size_t)nf + 1));
  memcpy(fv_idx, h + o_fidx, 4 * (size_t)live);
  *n_bow = nb; *n_fv = nf;
  return 0;
}

size_t orbv_batch_scratch_bytes(int nframes, int cap) {
  if (nframes < 0 || cap < 0) return 0;
  return 3 * sizeof(int32_t) * (size_t)nframes * (size_t)cap;
}

static int voc_batch(orbv_t *v, const uint8_t *d_descriptors, int nframes, int cap, const int32_t *d_n, int n_stride, int levelsup,
                     uint32_t *d_word, uint32_t *d_node, uint32_t *d_bow_id, double *d_bow_val, int32_t *d_n_bow, uint32_t *d_fv_node_id,
                     int32_t *d_fv_start, int32_t *d_fv_idx, int32_t *d_n_fv, void *d_scratch, void *stream, int descend_form) {
  int nid_level;
  const int rc = voc_check(v, levelsup, &nid_level);
  if (rc < 0) return rc;
  if (v->device < 0) return voc_fail("orbv_transform_batch_device: the handle was created with device = -1 and has no device tables");
  if (nframes < 0 || nframes > 65535 || cap <= 0 || cap > ORBM_MAX_KEYPOINTS || n_stride <= 0)
    return voc_fail("orbv_transform_batch_device: nframes outside [0, 65535], cap outside [1, ORBM_MAX_KEYPOINTS] or n_stride <= 0");
  if (nframes == 0) return 0;
  if (!d_descriptors || !d_n || !d_bow_id || !d_bow_val || !d_n_bow || !d_fv_node_id || !d_fv_start || !d_fv_idx || !d_n_fv || !d_scratch)
    return voc_fail("orbv_transform_batch_device: NULL argument");
  if (((uintptr_t)d_descriptors & 15) || ((uintptr_t)d_bow_val & 7) || ((uintptr_t)d_scratch & 3))
    return voc_fail("orbv_transform_batch_device: descriptors not 16-byte aligned, bow_val not 8-byte aligned or scratch not 4-byte aligned");
  VCHECK(hipSetDevice(v->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t FC = (size_t)nframes * (size_t)cap;
  if (v->n_words == 0) {   // empty() (:1134): empty containers for every frame
    VCHECK(hipMemsetAsync(d_n_bow, 0, sizeof(int32_t) * (size_t)nframes, s));
    VCHECK(hipMemsetAsync(d_n_fv, 0, sizeof(int32_t) * (size_t)nframes, s));
    VCHECK(hipMemsetAsync(d_fv_start, 0, sizeof(int32_t) * (size_t)nframes * ((size_t)cap + 1), s));
    if (d_word) VCHECK(hipMemsetAsync(d_word, 0, 4 * FC, s));
    if (d_node) VCHECK(hipMemsetAsync(d_node, 0, 4 * FC, s));
    return 0;
  }
  int32_t *sc = (int32_t *)d_scratch;
  voc_launch(v, s, d_descriptors, LiveCount{d_n, n_stride, 0}, cap, nframes, nid_level, sc, d_word ? d_word : (uint32_t *)(sc + FC),
             d_node ? d_node : (uint32_t *)(sc + 2 * FC), d_bow_id, d_bow_val, d_n_bow, d_fv_node_id, d_fv_start, d_fv_idx, d_n_fv, descend_form);
  VCHECK(hipGetLastError());
  return 0;
}

int orbv_transform_batch_device(orbv_t *v, const uint8_t *d_descriptors, int nframes, int cap, const int32_t *d_n, int n_stride, int levelsup,
                                uint32_t *d_word, uint32_t *d_node, uint32_t *d_bow_id, double *d_bow_val, int32_t *d_n_bow,
                                uint32_t *d_fv_node_id, int32_t *d_fv_start, int32_t *d_fv_idx, int32_t *d_n_fv, void *d_scratch, void *stream) {
  return voc_batch(v, d_descriptors, nframes, cap, d_n, n_stride, levelsup, d_word, d_node, d_bow_id, d_bow_val, d_n_bow, d_fv_node_id,
                   d_fv_start, d_fv_idx, d_n_fv, d_scratch, stream, 0);
}

int orbv_transform_batch_device_form(orbv_t *v, int descend_form, const uint8_t *d_descriptors, int nframes, int cap, const int32_t *d_n,
                                     int n_stride, int levelsup, uint32_t *d_word, uint32_t *d_node, uint32_t *d_bow_id, double *d_bow_val,
                                     int32_t *d_n_bow, uint32_t *d_fv_node_id, int32_t *d_fv_start, int32_t *d_fv_idx, int32_t *d_n_fv,
                                     void *d_scratch, void *stream) {
  if (descend_form != 0 && descend_form != 1) return voc_fail("orbv_transform_batch_device_form: descend_form outside {0, 1}");
  return voc_batch(v, d_descriptors, nframes, cap, d_n, n_stride, levelsup, d_word, d_node, d_bow_id, d_bow_val, d_n_bow, d_fv_node_id,
                   d_fv_start, d_fv_idx, d_n_fv, d_scratch, stream, descend_form);
}

}  // extern "C"

// =====================================================================================================================================
// KeyFrameDatabase (KeyFrameDatabase.cc:39-98, :620-811, :814-926): csrc/orb_ref_kfdb.h on the host, csrc/orb_kfdb_kernels.h on the device
// =====================================================================================================================================

struct orbd_handle {
  int device = -1, n_words = 0, capacity = 0;
  std::mutex mu;                                   // where the reference holds mMutex, and around every other use of the tables
  // slots in add order; an erased slot is a tombstone (n = -1) until the next compaction
  std::vector<KfdbSlot> slot;                      // the mirror of d_slot: off, n, tag, rq = mnRelocQuery
  std::vector<uint64_t> map_id, place_q;           // GetMap(), mnPlaceRecognitionQuery
  std::vector<float> reloc_s, place_s;             // mRelocScore, mPlaceRecognitionScore
  std::vector<uint8_t> on_host;                    // the slot's words are in h_ids / h_val (not so after orbd_add_device)
  std::vector<uint32_t> h_ids; std::vector<double> h_val;   // the pool, same offsets as on the device
  size_t pool_used = 0, pool_cap = 0;
  int live = 0;
  std::map<uint64_t, int> by_tag;                  // live entries only
  KfdbSlot *d_slot = nullptr; uint32_t *d_ids = nullptr; double *d_val = nullptr; uint32_t *d_bitmap = nullptr;
  int bm_stride = 0;
  bool rq_dirty = false;                           // d_slot[].rq is behind slot[].rq (only the batch form reads it there)
  hipStream_t s = nullptr;
  uint8_t *d_work = nullptr, *pin = nullptr; size_t work_bytes = 0;
};

static thread_local std::string g_kfdb_err;
static int kfdb_fail(const std::string &what) { g_kfdb_err = what; return ORBX_E_ARG; }
#define DCHECK(call)                                                        \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) {                                                 \
      g_kfdb_err = std::string(#call) + ": " + hipGetErrorString(e_);       \
      return ORBX_E_HIP;                                                    \
    }                                                                       \
  } while (0)

// k_kfdb_order sorts up to 16384 8-byte keys in dynamic LDS
static LdsOnce g_kfdb_lds;

// ids strictly ascending and below n_words, values finite
static int kfdb_check_bow(const orbd_handle *d, const char *who, const uint32_t *id, const double *val, int n) {
  if (n < 0 || n > ORBM_MAX_KEYPOINTS) return kfdb_fail(std::string(who) + ": n outside [0, ORBM_MAX_KEYPOINTS]");
  if (n > 0 && (!id || !val)) return kfdb_fail(std::string(who) + ": NULL BowVector");
  for (int i = 0; i < n; i++) {
    if (id[i] >= (uint32_t)d->n_words) return kfdb_fail(std::string(who) + ": a word id is not below n_words");
    if (i > 0 && id[i] <= id[i - 1]) return kfdb_fail(std::string(who) + ": word ids are not strictly ascending");
    if (val && !std::isfinite(val[i])) return kfdb_fail(std::string(who) + ": a word value is not finite");
  }
  return 0;
}

// the device pool holds at least `need` words: a larger block, the used prefix copied device to device
static int kfdb_reserve_pool(orbd_handle *d, size_t need) {
  if (d->device < 0 || need <= d->pool_cap) return 0;
  size_t cap = d->pool_cap ? d->pool_cap : 65536;
  while (cap < need) cap *= 2;
  uint32_t *ni = nullptr; double *nv = nullptr;
  DCHECK(hipMalloc(&ni, sizeof(uint32_t) * cap));
  hipError_t e = hipMalloc(&nv, sizeof(double) * cap);
  if (e == hipSuccess && d->pool_used) e = hipMemcpy(ni, d->d_ids, sizeof(uint32_t) * d->pool_used, hipMemcpyDeviceToDevice);
  if (e == hipSuccess && d->pool_used) e = hipMemcpy(nv, d->d_val, sizeof(double) * d->pool_used, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) { (void)hipFree(ni); if (nv) (void)hipFree(nv); g_kfdb_err = std::string("orbd: pool: ") + hipGetErrorString(e); return ORBX_E_HIP; }
  if (d->d_ids) (void)hipFree(d->d_ids);
  if (d->d_val) (void)hipFree(d->d_val);
  d->d_ids = ni; d->d_val = nv; d->pool_cap = cap;
  return 0;
}

// Drops the tombstones; the live entries keep their relative order (the ORDER RULE reads the slot index as the add sequence).
static int kfdb_compact(orbd_handle *d) {
  const int ns = (int)d->slot.size();
  if (d->live == ns) return 0;
  std::vector<KfdbSlot> slot; std::vector<uint64_t> map_id, place_q; std::vector<float> reloc_s, place_s; std::vector<uint8_t> on_host;
  std::vector<uint32_t> h_ids(d->h_ids.size()); std::vector<double> h_val(d->h_val.size());
  uint32_t *ni = nullptr; double *nv = nullptr;
  if (d->device >= 0 && d->pool_cap) {
    DCHECK(hipMalloc(&ni, sizeof(uint32_t) * d->pool_cap));
    hipError_t e = hipMalloc(&nv, sizeof(double) * d->pool_cap);
    if (e != hipSuccess) { (void)hipFree(ni); g_kfdb_err = std::string("orbd: compaction: ") + hipGetErrorString(e); return ORBX_E_HIP; }
  }
  size_t used = 0;
  hipError_t e = hipSuccess;
  for (int i = 0; i < ns; i++) {
    const KfdbSlot &o = d->slot[i];
    if (o.n < 0) continue;
    KfdbSlot t = o;
    t.off = (uint32_t)used;
    if (o.n > 0) {
      if (d->on_host[i]) {
        memcpy(&h_ids[used], &d->h_ids[o.off], sizeof(uint32_t) * (size_t)o.n);
        memcpy(&h_val[used], &d->h_val[o.off], sizeof(double) * (size_t)o.n);
      }
      if (ni && e == hipSuccess) e = hipMemcpy(ni + used, d->d_ids + o.off, sizeof(uint32_t) * (size_t)o.n, hipMemcpyDeviceToDevice);
      if (ni && e == hipSuccess) e = hipMemcpy(nv + used, d->d_val + o.off, sizeof(double) * (size_t)o.n, hipMemcpyDeviceToDevice);
    }
    used += (size_t)o.n;
    slot.push_back(t); map_id.push_back(d->map_id[i]); place_q.push_back(d->place_q[i]); reloc_s.push_back(d->reloc_s[i]);
    place_s.push_back(d->place_s[i]); on_host.push_back(d->on_host[i]);
  }
  if (e == hipSuccess && d->device >= 0 && !slot.empty())
    e = hipMemcpy(d->d_slot, slot.data(), sizeof(KfdbSlot) * slot.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (ni) (void)hipFree(ni);
    if (nv) (void)hipFree(nv);
    g_kfdb_err = std::string("orbd: compaction: ") + hipGetErrorString(e);
    return ORBX_E_HIP;
  }
  if (ni) { (void)hipFree(d->d_ids); (void)hipFree(d->d_val); d->d_ids = ni; d->d_val = nv; }
  d->slot.swap(slot); d->map_id.swap(map_id); d->place_q.swap(place_q); d->reloc_s.swap(reloc_s); d->place_s.swap(place_s);
  d->on_host.swap(on_host); d->h_ids.swap(h_ids); d->h_val.swap(h_val);
  d->pool_used = used; d->rq_dirty = false;
  d->by_tag.clear();
  for (int i = 0; i < (int)d->slot.size(); i++) d->by_tag[d->slot[i].tag] = i;
  return 0;
}

static int kfdb_upload_slot(orbd_handle *d, int i) {
  if (d->device < 0) return 0;
  DCHECK(hipMemcpy(d->d_slot + i, &d->slot[i], sizeof(KfdbSlot), hipMemcpyHostToDevice));
  return 0;
}

// room for one more keyframe of n words: a free slot (after a compaction if need be) and pool space
static int kfdb_make_room(orbd_handle *d, const char *who, uint64_t tag, int n) {
  if (tag == ORBD_NO_TAG) return kfdb_fail(std::string(who) + ": tag is the sentinel ORBD_NO_TAG");
  if (d->by_tag.count(tag)) return kfdb_fail(std::string(who) + ": duplicate tag (the keyframe is in the database)");
  if (d->live >= d->capacity) return kfdb_fail(std::string(who) + ": the database holds `capacity` keyframes");
  if (d->device >= 0) DCHECK(hipSetDevice(d->device));
  if ((int)d->slot.size() >= d->capacity || d->pool_used + (size_t)n > 0xffffffffull) {
    const int rc = kfdb_compact(d);
    if (rc < 0) return rc;
  }
  if (d->pool_used + (size_t)n > 0xffffffffull) return kfdb_fail(std::string(who) + ": the word pool is full");
  return kfdb_reserve_pool(d, d->pool_used + (size_t)n);
}

static void kfdb_push(orbd_handle *d, uint64_t tag, uint64_t map_id, int n, bool on_host, const orbd_members_t *init) {
  KfdbSlot t;
  memset(&t, 0, sizeof t);
  t.off = (uint32_t)d->pool_used; t.n = n; t.tag = tag; t.rq = init ? init->reloc_query : 0;
  d->by_tag[tag] = (int)d->slot.size();
  d->slot.push_back(t); d->map_id.push_back(map_id); d->place_q.push_back(init ? init->place_query : 0);
  d->reloc_s.push_back(init ? init->reloc_score : 0.0f); d->place_s.push_back(init ? init->place_score : 0.0f);
  d->on_host.push_back(on_host ? 1 : 0);
  d->pool_used += (size_t)n; d->live++;
  if (d->h_ids.size() < d->pool_used) { d->h_ids.resize(d->pool_used + d->pool_used / 2); d->h_val.resize(d->h_ids.size()); }
}

static int kfdb_erase_slot(orbd_handle *d, int i) {
  d->by_tag.erase(d->slot[i].tag);
  d->slot[i].n = -1;
  d->live--;
  return kfdb_upload_slot(d, i);
}

// What both forms of a query hand to the common tail: the common-word count of every slot and the scored list in list order.
struct KfdbResult {
  std::vector<int32_t> cnt;         // [n_slots]; meaningful where listable
  int32_t hdr[KFDB_HDR] = {0, 0, 0, 0};
  std::vector<int32_t> out_slot; std::vector<float> out_score;
};

// csrc/orb_ref_kfdb.h in plain C++ over the host copy, by the ORDER RULE
static void kfdb_query_host(const orbd_handle *d, const std::vector<uint8_t> &listable, const uint32_t *qid, const double *qval, int n, KfdbResult *R) {
  const int ns = (int)d->slot.size();
  R->cnt.assign(ns, 0);
  std::vector<uint64_t> keys;
  int max_common = 0;
  for (int s = 0; s < ns; s++) {
    if (!listable[s]) continue;
    const KfdbSlot &sl = d->slot[s];
    const uint32_t *ids = d->h_ids.data() + sl.off;
    int a = 0, b = 0, words = 0;
    uint32_t first = 0;
    while (a < n && b < sl.n) {
      if (qid[a] == ids[b]) { if (!words) first = ids[b]; words++; a++; b++; }
      else if (qid[a] < ids[b]) a++;
      else b++;
    }
    R->cnt[s] = words;
    if (words > 0) { keys.push_back(kfdb_order_key(first, (uint32_t)s)); if (words > max_common) max_common = words; }
  }
  std::sort(keys.begin(), keys.end());
  const int min_common = kfdb_min_common(max_common);
  for (uint64_t key : keys) {
    const int s = (int)(uint32_t)key;
    if (!kfdb_passes(R->cnt[s], min_common)) continue;
    const KfdbSlot &sl = d->slot[s];
    const uint32_t *ids = d->h_ids.data() + sl.off;
    const double *val = d->h_val.data() + sl.off;
    double score = 0;
    int a = 0, b = 0;
    while (a < n && b < sl.n) {
      if (qid[a] == ids[b]) { kfdb_l1_add(&score, kfdb_l1_term(qval[a], val[b])); a++; b++; }
      else if (qid[a] < ids[b]) a++;
      else b++;
    }
    R->out_slot.push_back(s);
    R->out_score.push_back(kfdb_l1_finish(score));
  }
  R->hdr[KFDB_H_MAX] = max_common; R->hdr[KFDB_H_MIN] = min_common;
  R->hdr[KFDB_H_SCORED] = (int32_t)R->out_slot.size(); R->hdr[KFDB_H_LISTED] = (int32_t)keys.size();
}

static void kfdb_fill_params(const orbd_handle *d, KfdbParams *P) {
  memset(P, 0, sizeof *P);
  P->slot = d->d_slot; P->n_slots = (int)d->slot.size(); P->ids = d->d_ids; P->val = d->d_val;
  P->n_words = d->n_words; P->bm_stride = d->bm_stride;
}

static void kfdb_launch(const KfdbParams &P, int nq, hipStream_t s, bool unmark) {
  const unsigned gq = (unsigned)std::max(1, (P.cap + 255) / 256), gs = (unsigned)((P.n_slots + 3) / 4);
  hipLaunchKernelGGL(k_kfdb_mark, dim3(gq, (unsigned)nq), dim3(256), 0, s, P);
  hipLaunchKernelGGL(k_kfdb_count, dim3(gs, (unsigned)nq), dim3(256), 0, s, P);
  hipLaunchKernelGGL(k_kfdb_order, dim3((unsigned)nq), dim3(KFDB_THREADS), SortCarve::of(P.n_slots).bytes, s, P);
  hipLaunchKernelGGL(k_kfdb_score, dim3(gs, (unsigned)nq), dim3(256), 0, s, P);
  if (unmark) hipLaunchKernelGGL(k_kfdb_unmark, dim3(gq, 1u), dim3(256), 0, s, P);
}

// one upload (count, values, ids, listable flags), five kernels, one download (header, counts, scored list), one synchronisation
static int kfdb_query_device(orbd_handle *d, const std::vector<uint8_t> &listable, const uint32_t *qid, const double *qval, int n, KfdbResult *R) {
  const size_t ns = d->slot.size(), N = (size_t)n;
  const size_t o_val = 8, o_id = o_val + 8 * N, o_flag = o_id + 4 * N, up = o_flag + ns;
  const size_t o_hdr = (up + 15) & ~(size_t)15, o_cnt = o_hdr + 4 * KFDB_HDR, o_slot = o_cnt + 4 * ns, o_score = o_slot + 4 * ns,
               o_first = o_score + 4 * ns, bytes = o_first + 4 * ns;
  DCHECK(hipSetDevice(d->device));
  if (d->work_bytes < bytes) {
    if (d->d_work) DCHECK(hipFree(d->d_work));
    d->d_work = nullptr;
    if (d->pin) DCHECK(hipHostFree(d->pin));
    d->pin = nullptr; d->work_bytes = 0;
    const size_t room = bytes + bytes / 2;
    DCHECK(hipMalloc(&d->d_work, room));
    DCHECK(hipHostMalloc(&d->pin, room, hipHostMallocDefault));
    d->work_bytes = room;
  }
  uint8_t *h = d->pin, *w = d->d_work;
  *(int32_t *)h = n; *(int32_t *)(h + 4) = 0;
  memcpy(h + o_val, qval, 8 * N);
  memcpy(h + o_id, qid, 4 * N);
  memcpy(h + o_flag, listable.data(), ns);
  DCHECK(hipMemcpyAsync(w, h, up, hipMemcpyHostToDevice, d->s));
  KfdbParams P;
  kfdb_fill_params(d, &P);
  P.bitmap = d->d_bitmap;
  P.q_n = (const int32_t *)w; P.q_val = (const double *)(w + o_val); P.q_id = (const uint32_t *)(w + o_id); P.cap = n;
  P.listable = w + o_flag;
  P.hdr = (int32_t *)(w + o_hdr); P.cnt = (int32_t *)(w + o_cnt); P.out_slot = (int32_t *)(w + o_slot); P.out_score = (float *)(w + o_score);
  P.first = (uint32_t *)(w + o_first); P.out_tag = nullptr; P.out_stride = (int)ns;
  kfdb_launch(P, 1, d->s, true);
  DCHECK(hipGetLastError());
  DCHECK(hipMemcpyAsync(h + o_hdr, w + o_hdr, o_first - o_hdr, hipMemcpyDeviceToHost, d->s));
  DCHECK(hipStreamSynchronize(d->s));
  memcpy(R->hdr, h + o_hdr, 4 * KFDB_HDR);
  const int scored = R->hdr[KFDB_H_SCORED];
  if (scored < 0 || (size_t)scored > ns || R->hdr[KFDB_H_LISTED] < scored || (size_t)R->hdr[KFDB_H_LISTED] > ns) {
    g_kfdb_err = "orbd_query: the device returned counts outside [0, keyframes]";
    return ORBX_E_HIP;
  }
  R->cnt.assign((const int32_t *)(h + o_cnt), (const int32_t *)(h + o_cnt) + ns);
  R->out_slot.assign((const int32_t *)(h + o_slot), (const int32_t *)(h + o_slot) + scored);
  R->out_score.assign((const float *)(h + o_score), (const float *)(h + o_score) + scored);
  for (int s : R->out_slot)
    if (s < 0 || (size_t)s >= ns) { g_kfdb_err = "orbd_query: the device returned a slot outside the database"; return ORBX_E_HIP; }
  return 0;
}

// form 0: DetectRelocalizationCandidates :816-871; form 1: DetectNBestCandidates :627-711
static int kfdb_query(orbd_handle *d, const char *who, int form, bool on_device, uint64_t query_id, const uint64_t *connected, int n_connected,
                      const uint32_t *bow_id, const double *bow_val, int n, uint64_t *out_tag, float *out_score, int out_cap,
                      int32_t *n_scored, int32_t *max_common, int32_t *min_common, int32_t *n_listed) {
  if (!d) return kfdb_fail(std::string(who) + ": NULL handle");
  if (on_device && d->device < 0) return kfdb_fail(std::string(who) + ": the handle was created with device = -1 and has no device tables");
  if (!n_scored || !max_common || !min_common || !n_listed || n_connected < 0 || (n_connected > 0 && !connected))
    return kfdb_fail(std::string(who) + ": NULL argument or n_connected < 0");
  std::lock_guard<std::mutex> lock(d->mu);
  int rc = kfdb_check_bow(d, who, bow_id, bow_val, n);
  if (rc < 0) return rc;
  if (out_cap < d->live || (d->live > 0 && (!out_tag || !out_score)))
    return kfdb_fail(std::string(who) + ": out_cap is below the number of live keyframes, or a NULL output");
  const int ns = (int)d->slot.size();
  std::vector<uint8_t> listable(ns, 0);
  for (int s = 0; s < ns; s++) {
    if (d->slot[s].n < 0) continue;
    if (!on_device && !d->on_host[s]) return kfdb_fail(std::string(who) + ": a keyframe added by orbd_add_device has no host copy");
    listable[s] = (form == 0 ? d->slot[s].rq : d->place_q[s]) != query_id;
  }
  for (int c = 0; c < n_connected; c++) {   // spConnectedKF (:637, :656): counted, never listed, never marked
    const auto it = d->by_tag.find(connected[c]);
    if (it == d->by_tag.end()) return kfdb_fail(std::string(who) + ": a connected tag is not in the database");
    listable[it->second] = 0;
  }
  KfdbResult R;
  if (ns > 0 && n > 0) {
    if (on_device) { rc = kfdb_query_device(d, listable, bow_id, bow_val, n, &R); if (rc < 0) return rc; }
    else kfdb_query_host(d, listable, bow_id, bow_val, n, &R);
    for (int s = 0; s < ns; s++)
      if (listable[s] && R.cnt[s] > 0) {   // :832, :659
        if (form == 0) { d->slot[s].rq = query_id; d->rq_dirty = true; } else d->place_q[s] = query_id;
      }
  }
  for (size_t r = 0; r < R.out_slot.size(); r++) {
    const int s = R.out_slot[r];
    (form == 0 ? d->reloc_s : d->place_s)[s] = R.out_score[r];   // :865, :705
    out_tag[r] = d->slot[s].tag; out_score[r] = R.out_score[r];
  }
  *n_scored = R.hdr[KFDB_H_SCORED]; *max_common = R.hdr[KFDB_H_MAX]; *min_common = R.hdr[KFDB_H_MIN]; *n_listed = R.hdr[KFDB_H_LISTED];
  return 0;
}

// the accumulation over covisibles (:877-902, :719-744) shared by both forms
struct KfdbAcc { float acc; uint64_t best; };
static int kfdb_accumulate(orbd_handle *d, const char *who, int form, uint64_t query_id, const uint64_t *tags, const float *scores, int n,
                           const uint64_t *covisibles, std::vector<KfdbAcc> *out, float *best_acc) {
  if (n < 0 || (n > 0 && (!tags || !scores || !covisibles))) return kfdb_fail(std::string(who) + ": NULL argument or n < 0");
  for (int i = 0; i < n; i++)
    if (!d->by_tag.count(tags[i])) return kfdb_fail(std::string(who) + ": a scored tag is not in the database");
  *best_acc = 0;   // :874, :714
  for (int i = 0; i < n; i++) {
    float best = scores[i], acc = best;
    uint64_t best_kf = tags[i];
    for (int k = 0; k < ORBD_COVISIBLES; k++) {
      const uint64_t t = covisibles[(size_t)i * ORBD_COVISIBLES + k];
      if (t == ORBD_NO_TAG) continue;
      const auto it = d->by_tag.find(t);
      if (it == d->by_tag.end()) continue;                                                        // unknown or erased: "query id differs"
      if ((form == 0 ? d->slot[it->second].rq : d->place_q[it->second]) != query_id) continue;    // :888, :730
      const float s2 = (form == 0 ? d->reloc_s : d->place_s)[it->second];
      kfdb_acc_add(&acc, s2);
      if (kfdb_beats(s2, best)) { best_kf = t; best = s2; }
    }
    out->push_back(KfdbAcc{acc, best_kf});
    if (acc > *best_acc) *best_acc = acc;
  }
  return 0;
}

extern "C" {

const char *orbd_last_error(const orbd_t *) { return g_kfdb_err.c_str(); }

void orbd_destroy(orbd_t *d) {
  if (!d) return;
  if (d->device >= 0) {
    (void)hipSetDevice(d->device);
    if (d->s) { (void)hipStreamSynchronize(d->s); (void)hipStreamDestroy(d->s); }
    if (d->d_slot) (void)hipFree(d->d_slot);
    if (d->d_ids) (void)hipFree(d->d_ids);
    if (d->d_val) (void)hipFree(d->d_val);
    if (d->d_bitmap) (void)hipFree(d->d_bitmap);
    if (d->d_work) (void)hipFree(d->d_work);
    if (d->pin) (void)hipHostFree(d->pin);
  }
  delete d;
}

orbd_t *orbd_create(int n_words, int scoring, int capacity, int device) {
  g_kfdb_err.clear();
  if (n_words < 0 || device < -1) { kfdb_fail("orbd_create: n_words < 0 or device < -1"); return nullptr; }
  if (scoring != VOC_L1_NORM) { kfdb_fail("orbd_create: only L1_NORM scoring (type 0, what ORBvoc uses) is supported (csrc/orb_ref_kfdb.h)"); return nullptr; }
  if (capacity < 1 || capacity > ORBD_MAX_KEYFRAMES) { kfdb_fail("orbd_create: capacity outside [1, ORBD_MAX_KEYFRAMES]"); return nullptr; }
  orbd_handle *d = new orbd_handle;
  d->device = device; d->n_words = n_words; d->capacity = capacity; d->bm_stride = (n_words + 31) / 32 + 1;
  if (device < 0) return d;
  const hipError_t e0 = hipSetDevice(device);
  hipError_t e = e0;
  if (e == hipSuccess) e = raise_lds_once(g_kfdb_lds, device, {reinterpret_cast<const void *>(&k_kfdb_order)});
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->s, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&d->d_slot, sizeof(KfdbSlot) * (size_t)capacity);
  if (e == hipSuccess) e = hipMalloc(&d->d_bitmap, sizeof(uint32_t) * (size_t)d->bm_stride);
  if (e == hipSuccess) e = hipMemset(d->d_bitmap, 0, sizeof(uint32_t) * (size_t)d->bm_stride);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const std::string what = std::string("orbd_create: HIP: ") + hipGetErrorString(e);
    if (e0 != hipSuccess) d->device = -1;
    orbd_destroy(d);
    g_kfdb_err = what;
    return nullptr;
  }
  return d;
}

orbd_t *orbd_create_for_vocabulary(const orbv_t *v, int capacity, int device) {
  if (!v) { kfdb_fail("orbd_create_for_vocabulary: NULL vocabulary"); return nullptr; }
  return orbd_create(v->n_words, v->scoring, capacity, device);
}

int orbd_n_words(const orbd_t *d) { return d ? d->n_words : ORBX_E_ARG; }
int orbd_capacity(const orbd_t *d) { return d ? d->capacity : ORBX_E_ARG; }
int orbd_size(orbd_t *d) {
  if (!d) return ORBX_E_ARG;
  std::lock_guard<std::mutex> lock(d->mu);
  return d->live;
}

int orbd_add(orbd_t *d, uint64_t tag, uint64_t map_id, const uint32_t *bow_id, const double *bow_val, int n, const orbd_members_t *init) {
  if (!d) return kfdb_fail("orbd_add: NULL handle");
  std::lock_guard<std::mutex> lock(d->mu);
  int rc = kfdb_check_bow(d, "orbd_add", bow_id, bow_val, n);
  if (rc < 0) return rc;
  rc = kfdb_make_room(d, "orbd_add", tag, n);
  if (rc < 0) return rc;
  if (d->device >= 0 && n > 0) {
    DCHECK(hipMemcpy(d->d_ids + d->pool_used, bow_id, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
    DCHECK(hipMemcpy(d->d_val + d->pool_used, bow_val, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  }
  const size_t at = d->pool_used;
  kfdb_push(d, tag, map_id, n, true, init);
  if (n > 0) { memcpy(&d->h_ids[at], bow_id, sizeof(uint32_t) * (size_t)n); memcpy(&d->h_val[at], bow_val, sizeof(double) * (size_t)n); }
  return kfdb_upload_slot(d, (int)d->slot.size() - 1);
}

int orbd_add_device(orbd_t *d, uint64_t tag, uint64_t map_id, const uint32_t *d_bow_id, const double *d_bow_val, const int32_t *d_n_bow,
                    int cap, int p, const orbd_members_t *init, void *stream) {
  if (!d) return kfdb_fail("orbd_add_device: NULL handle");
  if (d->device < 0) return kfdb_fail("orbd_add_device: the handle was created with device = -1 and has no device tables");
  if (!d_bow_id || !d_bow_val || !d_n_bow || cap < 1 || cap > ORBM_MAX_KEYPOINTS || p < 0 || p > 65534)
    return kfdb_fail("orbd_add_device: NULL argument, cap outside [1, ORBM_MAX_KEYPOINTS] or p outside [0, 65534]");
  std::lock_guard<std::mutex> lock(d->mu);
  if (tag == ORBD_NO_TAG || d->by_tag.count(tag)) return kfdb_fail("orbd_add_device: duplicate tag, or the sentinel ORBD_NO_TAG");
  DCHECK(hipSetDevice(d->device));
  hipStream_t s = (hipStream_t)stream;
  int32_t n = 0;
  DCHECK(hipMemcpyAsync(&n, d_n_bow + p, sizeof n, hipMemcpyDeviceToHost, s));   // the 4-byte count, nothing else comes back
  DCHECK(hipStreamSynchronize(s));
  n = std::min(std::max(n, 0), cap);
  const int rc = kfdb_make_room(d, "orbd_add_device", tag, n);
  if (rc < 0) return rc;
  if (n > 0) {
    DCHECK(hipMemcpyAsync(d->d_ids + d->pool_used, d_bow_id + (size_t)p * cap, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
    DCHECK(hipMemcpyAsync(d->d_val + d->pool_used, d_bow_val + (size_t)p * cap, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    DCHECK(hipStreamSynchronize(s));
  }
  kfdb_push(d, tag, map_id, n, false, init);
  return kfdb_upload_slot(d, (int)d->slot.size() - 1);
}

int orbd_erase(orbd_t *d, uint64_t tag) {
  if (!d) return kfdb_fail("orbd_erase: NULL handle");
  std::lock_guard<std::mutex> lock(d->mu);
  const auto it = d->by_tag.find(tag);
  if (it == d->by_tag.end()) return kfdb_fail("orbd_erase: the tag is not in the database");
  if (d->device >= 0) DCHECK(hipSetDevice(d->device));
  return kfdb_erase_slot(d, it->second);
}

int orbd_clear(orbd_t *d) {
  if (!d) return kfdb_fail("orbd_clear: NULL handle");
  std::lock_guard<std::mutex> lock(d->mu);
  d->slot.clear(); d->map_id.clear(); d->place_q.clear(); d->reloc_s.clear(); d->place_s.clear(); d->on_host.clear(); d->by_tag.clear();
  d->pool_used = 0; d->live = 0; d->rq_dirty = false;
  return 0;
}

int orbd_clear_map(orbd_t *d, uint64_t map_id) {
  if (!d) return kfdb_fail("orbd_clear_map: NULL handle");
  std::lock_guard<std::mutex> lock(d->mu);
  if (d->device >= 0) DCHECK(hipSetDevice(d->device));
  for (int i = 0; i < (int)d->slot.size(); i++)
    if (d->slot[i].n >= 0 && d->map_id[i] == map_id) {
      const int rc = kfdb_erase_slot(d, i);
      if (rc < 0) return rc;
    }
  return 0;
}

int orbd_set_map(orbd_t *d, uint64_t tag, uint64_t map_id) {
  if (!d) return kfdb_fail("orbd_set_map: NULL handle");
  std::lock_guard<std::mutex> lock(d->mu);
  const auto it = d->by_tag.find(tag);
  if (it == d->by_tag.end()) return kfdb_fail("orbd_set_map: the tag is not in the database");
  d->map_id[it->second] = map_id;
  return 0;
}

int orbd_get_members(orbd_t *d, uint64_t tag, orbd_members_t *out) {
  if (!d || !out) return kfdb_fail("orbd_get_members: NULL argument");
  std::lock_guard<std::mutex> lock(d->mu);
  const auto it = d->by_tag.find(tag);
  if (it == d->by_tag.end()) return kfdb_fail("orbd_get_members: the tag is not in the database");
  const int s = it->second;
  out->reloc_query = d->slot[s].rq; out->place_query = d->place_q[s]; out->reloc_score = d->reloc_s[s]; out->place_score = d->place_s[s];
  return 0;
}

int orbd_query_reloc(orbd_t *d, uint64_t query_id, const uint32_t *bow_id, const double *bow_val, int n, uint64_t *out_tag, float *out_score,
                     int out_cap, int32_t *n_scored, int32_t *max_common, int32_t *min_common, int32_t *n_listed) {
  return kfdb_query(d, "orbd_query_reloc", 0, true, query_id, nullptr, 0, bow_id, bow_val, n, out_tag, out_score, out_cap, n_scored, max_common,
                    min_common, n_listed);
}
int orbd_query_reloc_host(orbd_t *d, uint64_t query_id, const uint32_t *bow_id, const double *bow_val, int n, uint64_t *out_tag,
                          float *out_score, int out_cap, int32_t *n_scored, int32_t *max_common, int32_t *min_common, int32_t *n_listed) {
  return kfdb_query(d, "orbd_query_reloc_host", 0, false, query_id, nullptr, 0, bow_id, bow_val, n, out_tag, out_score, out_cap, n_scored,
                    max_common, min_common, n_listed);
}
int orbd_query_place(orbd_t *d, uint64_t query_id, const uint64_t *connected_tags, int n_connected, const uint32_t *bow_id,
                     const double *bow_val, int n, uint64_t *out_tag, float *out_score, int out_cap, int32_t *n_scored, int32_t *max_common,
                     int32_t *min_common, int32_t *n_listed) {
  return kfdb_query(d, "orbd_query_place", 1, true, query_id, connected_tags, n_connected, bow_id, bow_val, n, out_tag, out_score, out_cap,
                    n_scored, max_common, min_common, n_listed);
}
int orbd_query_place_host(orbd_t *d, uint64_t query_id, const uint64_t *connected_tags, int n_connected, const uint32_t *bow_id,
                          const double *bow_val, int n, uint64_t *out_tag, float *out_score, int out_cap, int32_t *n_scored,
                          int32_t *max_common, int32_t *min_common, int32_t *n_listed) {
  return kfdb_query(d, "orbd_query_place_host", 1, false, query_id, connected_tags, n_connected, bow_id, bow_val, n, out_tag, out_score, out_cap,
                    n_scored, max_common, min_common, n_listed);
}

size_t orbd_batch_scratch_bytes(const orbd_t *d, int nq) {
  if (!d || nq < 0) return 0;
  return (size_t)nq * (8 + 4 * (size_t)d->bm_stride + 12 * (size_t)d->capacity) + 16;
}

int orbd_score_batch_device(orbd_t *d, int nq, const uint64_t *query_id, const uint32_t *d_bow_id, const double *d_bow_val,
                            const int32_t *d_n_bow, int cap, uint64_t *d_out_tag, float *d_out_score, int out_cap, int32_t *d_counts,
                            void *d_scratch, void *stream) {
  if (!d) return kfdb_fail("orbd_score_batch_device: NULL handle");
  if (d->device < 0) return kfdb_fail("orbd_score_batch_device: the handle was created with device = -1 and has no device tables");
  if (nq < 0 || nq > 65535 || cap < 1 || cap > ORBM_MAX_KEYPOINTS)
    return kfdb_fail("orbd_score_batch_device: nq outside [0, 65535] or cap outside [1, ORBM_MAX_KEYPOINTS]");
  if (nq == 0) return 0;
  if (!query_id || !d_bow_id || !d_bow_val || !d_n_bow || !d_out_tag || !d_out_score || !d_counts || !d_scratch)
    return kfdb_fail("orbd_score_batch_device: NULL argument");
  if (((uintptr_t)d_bow_val & 7) || ((uintptr_t)d_out_tag & 7) || ((uintptr_t)d_scratch & 7))
    return kfdb_fail("orbd_score_batch_device: bow_val, out_tag or scratch not 8-byte aligned");
  std::lock_guard<std::mutex> lock(d->mu);
  if (out_cap < std::max(d->live, 1) || out_cap > d->capacity)
    return kfdb_fail("orbd_score_batch_device: out_cap outside [max(live keyframes, 1), capacity]");
  DCHECK(hipSetDevice(d->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t ns = d->slot.size(), Q = (size_t)nq;
  if (ns == 0) { DCHECK(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * KFDB_HDR * Q, s)); return 0; }
  if (d->rq_dirty) {   // mnRelocQuery as the single queries left it
    DCHECK(hipMemcpy(d->d_slot, d->slot.data(), sizeof(KfdbSlot) * ns, hipMemcpyHostToDevice));
    d->rq_dirty = false;
  }
  uint8_t *w = (uint8_t *)d_scratch;
  const size_t o_bm = 8 * Q, o_cnt = o_bm + 4 * Q * (size_t)d->bm_stride, o_first = o_cnt + 4 * Q * ns, o_slot = o_first + 4 * Q * ns;
  DCHECK(hipMemcpyAsync(w, query_id, 8 * Q, hipMemcpyHostToDevice, s));
  DCHECK(hipMemsetAsync(w + o_bm, 0, 4 * Q * (size_t)d->bm_stride, s));
  KfdbParams P;
  kfdb_fill_params(d, &P);
  P.bitmap = (uint32_t *)(w + o_bm);
  P.q_n = d_n_bow; P.q_val = d_bow_val; P.q_id = d_bow_id; P.cap = cap;
  P.listable = nullptr; P.query_id = (const uint64_t *)w;
  P.hdr = d_counts; P.cnt = (int32_t *)(w + o_cnt); P.first = (uint32_t *)(w + o_first); P.out_slot = (int32_t *)(w + o_slot);
  P.out_score = d_out_score; P.out_tag = d_out_tag; P.out_stride = out_cap;
  kfdb_launch(P, nq, s, false);
  DCHECK(hipGetLastError());
  return 0;
}

int orbd_accumulate_reloc(orbd_t *d, uint64_t query_id, uint64_t map_id, const uint64_t *tags, const float *scores, int n,
                          const uint64_t *covisibles, uint64_t *out_tags, int32_t *n_out) {
  if (!d || !n_out || (n > 0 && !out_tags)) return kfdb_fail("orbd_accumulate_reloc: NULL argument");
  std::lock_guard<std::mutex> lock(d->mu);
  std::vector<KfdbAcc> acc;
  float best_acc;
  const int rc = kfdb_accumulate(d, "orbd_accumulate_reloc", 0, query_id, tags, scores, n, covisibles, &acc, &best_acc);
  if (rc < 0) return rc;
  const float min_retain = kfdb_min_retain(best_acc);
  int m = 0;
  for (const KfdbAcc &a : acc) {
    if (!kfdb_retained(a.acc, min_retain)) continue;
    if (d->map_id[d->by_tag.find(a.best)->second] != map_id) continue;   // :915, after the threshold over all maps
    bool seen = false;                                                   // spAlreadyAddedKF
    for (int k = 0; k < m && !seen; k++) seen = out_tags[k] == a.best;
    if (!seen) out_tags[m++] = a.best;
  }
  *n_out = m;
  return 0;
}

int orbd_accumulate_place(orbd_t *d, uint64_t query_id, const uint64_t *tags, const float *scores, int n, const uint64_t *covisibles,
                          float *out_acc, uint64_t *out_best) {
  if (!d || (n > 0 && (!out_acc || !out_best))) return kfdb_fail("orbd_accumulate_place: NULL argument");
  std::lock_guard<std::mutex> lock(d->mu);
  std::vector<KfdbAcc> acc;
  float best_acc;
  const int rc = kfdb_accumulate(d, "orbd_accumulate_place", 1, query_id, tags, scores, n, covisibles, &acc, &best_acc);
  if (rc < 0) return rc;
  std::stable_sort(acc.begin(), acc.end(), [](const KfdbAcc &a, const KfdbAcc &b) { return a.acc > b.acc; });   // list::sort(compFirst), :748
  for (int i = 0; i < n; i++) { out_acc[i] = acc[i].acc; out_best[i] = acc[i].best; }
  return 0;
}

}  // extern "C"
