// orb_mfma_util.h -- Hamming distances of the projection searches on the matrix pipe: the shared pieces (operand expansion,
// per-lane sorted lists) of k_match_scan_mfma (orb_match_mfma.h) and of the list build inside k_match_resolve's fused form.
// Two forms of the same product give the same key: the i8 form (described first; k_match_scan_mfma, k_knn2_mfma,
// k_hamming_matrix_mfma) and the FP4 form (further down, "FP4 form"; the list build of k_match_resolve's fused form, the only one
// on the benchmark's step), which needs a quarter of the operand registers and under half of the expansion instructions.
//
// BASELINE's "1000 x 1000" setting (and every relocalisation-style search whose windows cover the frame) asks for ALL
// Hamming distances between the queries and the keypoints of a frame (ORBmatcher::DescriptorDistance, ORBmatcher.cc:2463-2483,
// inside the loops :99-120 / :2148-2156).  k_match_scan does that with 8 xor + 8 v_bcnt per query-candidate pair and wavefront;
// the popcount issues at a quarter of the VALU rate (profiles/valu_calib.json), so the scan was vector-issue bound while the
// matrix pipe idled.  A 256-bit Hamming distance is an exact int8 dot product:
//
//     with a_k = bit ? -32 : +32 (candidate) and b_k = bit ? +32 : -32 (query):   sum_k a_k b_k = 1024 (2 ham - 256)
//
// so  v_mfma_i32_32x32x32_i8  over the 8 K-steps of 32 bits, started from the accumulator  C[row] = 2^18 + rank[row], leaves
//
//     D[row = candidate][col = query] = ham << 11 | rank[candidate]
//
// i.e. the REDUCTION KEY ITSELF, without a single vector instruction: rank = position of the candidate in the enumeration order
// of Frame::GetFeaturesInArea (Frame.cc:781-809: grid column, then row, then insertion order), which decides ties between equal
// distances (strict <, first minimum wins) exactly as the 23 bits cell << 11 | idx of Key32 do - the rank is the same order,
// compressed to 11 bits so that it fits below a product-scaled distance (k_match_rank computes it once per frame pair).
// A candidate that is outside the grid or already held gets C = 2^18 + 2^30: its keys are larger than every real key.
//
// Layout of a 32 x 32 tile (guide, MFMA C/D map): col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) - a lane owns ONE
// query (its column) and sees 16 of the tile's 32 candidates; the two lanes of a column keep separate sorted top-8 lists of
// their halves of the frame, merged at the end.  Every wavefront holds two query tiles (64 queries) as B fragments in registers
// (the 1024 expanded bytes of a K-step pair never leave them), the candidate tiles are expanded once per workgroup into LDS
// (bit -> byte by a 4-bit multiply spread and one v_perm_b32) and read back as A fragments by conflict-free ds_read_b128
// (16-byte chunks of a row rotated by the row index).
//
// What is left on the VALU is the selection: every key goes through a branch-free sorted insertion, 1 v_min + (K - 1) v_med3
// (new[j] = med3(top[j-1], top[j], t): independent instructions, half the count of a compare-exchange chain).
//
// Users.  The brute-force entries (k_hamming_matrix_mfma, k_knn2_mfma: orb_match_mfma.h) take the product as it is.  k_match_scan_mfma (orb_match_mfma.h): 256-query blocks whose live queries are ALL "open" (window = whole grid, no
// level filter; query_is_open) of monocular problems on frames of at most 2048 keypoints get their top-8 lists from it and
// k_match_scan skips exactly those blocks (same vote); the lists are the same Key32 lists either way.  All three use the i8 form.
// k_match_resolve's FUSED form (orb_match_kernels.h; FP4 form, MfList on the results' bit patterns): frame pairs all of whose queries are open build the lists of each 64-query chunk inside the
// resolve kernel, with every keypoint a committed claim holds masked out through its accumulator seed - a list made that way
// cannot be exhausted by the claims of earlier chunks, which is what the refresh passes of the separate-kernel form
// spent their time on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef int mf_v4i __attribute__((ext_vector_type(4)));
typedef int mf_v16i __attribute__((ext_vector_type(16)));

#define MF_NT 256
#define MF_TILE 32
#define MF_REC_BASE (1u << 18)
#define MF_REC_HELD (1u << 30)
#define MF_REC_UNUSABLE ((1u << 18) + MF_REC_HELD)
#define MF_KEY_LIMIT (1u << 20)   // real keys are < 257 << 11

// median of three as the min / max expression the backend selects v_med3_u32 for.  NOT inline assembly: the compiler pads the
// wait states between an MFMA and the first vector instruction that reads its result only for instructions it emitted itself.
__device__ __forceinline__ uint32_t mf_med3(uint32_t a, uint32_t b, uint32_t c) { return max(min(a, b), min(max(a, b), c)); }

// 16 descriptor bits -> 16 bytes: LUT byte 0 for a 0 bit, LUT byte 1 for a 1 bit (v_perm_b32 selectors 0 / 1 pick bytes of src1)
__device__ __forceinline__ mf_v4i mf_expand16(uint32_t hw, uint32_t lut) {
  mf_v4i o;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t nib = (hw >> (4 * i)) & 0xfu;
    const uint32_t t = (nib * 0x00204081u) & 0x01010101u;          // bit i of the nibble -> byte i (0 / 1)
    o[i] = (int)__builtin_amdgcn_perm(0u, lut, t);
  }
  return o;
}
#define MF_LUT_CAND 0x0000E020u    // candidate: 0 -> +32, 1 -> -32
#define MF_LUT_QUERY 0x000020E0u   // query:     0 -> -32, 1 -> +32

// ---- FP4 form: the same key from v_mfma_scale_f32_32x32x64_f8f6f4, 64 descriptor bits per K-step --------------------------------------
// A bit is one E2M1 nibble: magnitude 2.0 (0100) with the bit as its sign, every block scale 2^4 (E8M0 0x83 in every byte of the
// scale operands, so no scale layout is involved): candidate 0 -> +32, 1 -> -32, query (from ~w) 0 -> -32, 1 -> +32, products
// +-1024 as in the i8 scheme, and from the seed C = float(2^18 + rank) the result is float(ham * 2048 + rank).  Every partial sum
// is an integer below 2^20 in magnitude, exact in f32 (tests/test_gpu_fused_fp4.py: every distance, every bit position).
// The K index of a dot product may be permuted freely as long as both operands use the same permutation, so operand dword j of
// a 32-bit descriptor word w takes bits j, 4 + j, 8 + j, ... : one shift-or and one and, no multiply, no v_perm_b32.  Lane half
// h of K-step s takes descriptor dword 2 s + h of its row (the 4 operand registers FP4 uses of the 8 the instruction names).
// The held / unusable seed 2^18 + 2^30 is exact as well; its results are rounded to multiples of 128 and stay far above
// MF_KEY_LIMIT.  Results are non-negative floats, so MfList orders their bit patterns as unsigned integers exactly as it orders
// the i8 form's keys; its empty entry 0xffffffff is a NaN pattern, so a list entry is converted back to the integer key only
// after the selection and only below MF4_KEY_LIMIT_BITS (mf4_key).
typedef int mf_v8i __attribute__((ext_vector_type(8)));
typedef float mf_v16f __attribute__((ext_vector_type(16)));
#define MF4_SIGN 0x88888888u
#define MF4_MAG 0x44444444u
#define MF4_SCALE 0x83838383                  // E8M0 2^4 in every byte
#define MF4_KEY_LIMIT_BITS 0x49800000u        // bit pattern of float(MF_KEY_LIMIT)

// 32 descriptor bits -> 32 nibbles; the query passes ~w
__device__ __forceinline__ mf_v4i mf4_expand32(uint32_t w) {
  mf_v4i o;
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = (int)(((w << (3 - j)) | MF4_MAG) & (MF4_SIGN | MF4_MAG));   // v_lshl_or_b32, v_and_b32
  return o;
}
// the builtin, not inline assembly (see mf_med3)
__device__ __forceinline__ mf_v16f mf4_mfma(const mf_v4i &a, const mf_v4i &b, const mf_v16f &c) {
  const mf_v8i a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4 /* cbsz: A is FP4 */, 4 /* blgp: B is FP4 */, 0, MF4_SCALE, 0, MF4_SCALE);
}
__device__ __forceinline__ float mf4_seed(uint32_t rec) { return (float)rec; }   // 2^18 + rank and 2^18 + 2^30 are exact
// list entry (bit pattern of a result) -> the i8 form's key, 0xffffffff for held / unusable / empty entries
__device__ __forceinline__ uint32_t mf4_key(uint32_t bits) { return bits < MF4_KEY_LIMIT_BITS ? (uint32_t)__uint_as_float(bits) : 0xffffffffu; }

template <int K>
struct MfList {
  uint32_t top[K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < K; j++) top[j] = 0xffffffffu;
  }
  __device__ __forceinline__ void insert(uint32_t t) {   // sorted insertion; a no-op for t = 0xffffffff
#pragma unroll
    for (int j = K - 1; j >= 1; j--) top[j] = mf_med3(top[j - 1], top[j], t);
    top[0] = min(top[0], t);
  }
  // Every key of the tile goes through the sorted insertion, unconditionally: K independent instructions per key and no vote,
  // no branch, no mask.  With 64 lanes x 16 keys behind every vote "does any key of the tile enter some lane's list" the answer
  // is yes for nearly every tile of a 1000-keypoint frame (a lane's top-8 list changes 8 ln(m / 8) + 8 = 41 times over its 500
  // candidates, 2600 times per wavefront and list), and k_match_scan's parked insertion then pays two ballots, two scalar
  // branches and a VCC select per key ON TOP of the insertions (measured with it: 3700 cycles per tile and wavefront in the
  // selection against 1000 for the MFMAs, tools/mfma_stamps.py; branch-free: 0.174 -> 0.125 ms for 256 frame pairs).
  __device__ __forceinline__ void take(const mf_v16i &k) {
#pragma unroll
    for (int r = 0; r < 16; r++) insert((uint32_t)k[r]);
  }
  __device__ __forceinline__ void take(const mf_v16f &k) {   // FP4 form: non-negative floats order as their bit patterns
#pragma unroll
    for (int r = 0; r < 16; r++) insert(__float_as_uint(k[r]));
  }
};

