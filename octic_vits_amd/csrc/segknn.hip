// The k-NN classifier of the segmentation evaluation (dinov2/eval/segmentation/eval_segmentation.py:172-278) on resident f32
// patch features: for every query row the kmax nearest key rows under the squared L2 distance, the cosine distance, or both
// from ONE pass over the (query, key) pairs.  The distance matrix never reaches memory.
//   1. seg_rownorms_kernel   : |x|^2 per row, one wave per row, a fixed summation order (lane-strided float4 chains, then a
//                              butterfly over the lanes).
//   2. seg_knn_kernel<MET>   : workgroup = 128 query rows x one contiguous range of key tiles (128 keys each).  Both tiles go
//                              through LDS in chunks of 32 channels; the dot products run on the exact-f32 MFMA (16x16x4), one
//                              accumulator chain over all of D per pair.  After a key tile the accumulators become ordering keys
//                                  L2     : (|a|^2 + |b|^2) - 2 a.b            (squared: the root does not change the order)
//                                  cosine : 1 - a.b / (sqrt|a|^2 sqrt|b|^2)
//                              and each is compared with the query's current kmax-th best (one LDS word per query and metric).
//                              Only survivors enter the query's sorted list (LDS, 32 entries), by a wave-wide sorted insert.
//                              MET = 1: L2, 2: cosine, 3: both lists from the same accumulators.
//   3. knn_merge_kernel      : (knn_common.hpp) when the key axis is split over workgroups (few queries), every split writes its
//                              own sorted list and one wave per (query, metric) merges them.
//   4. seg_knn_vote_kernel   : thread = (query, pixel): the running mode of labels[idx[query, 0 .. k-1], pixel] for up to 8
//                              ascending k, ties to the smallest value (torch.mode), written as uint8 [n_k, n, L].
// The streaming loop, the TOTAL ORDER (distance ascending, then key row index) and the DETERMINISM contract are those of
// knn_common.hpp, which this kernel shares with knn_topk_kernel (knn_cls.hip).  Here a distance that is NaN (a zero row under
// cosine) counts as +inf and a skipped key is at +inf, so neither is ever listed.  The distance is a contraction-free expression
// of the pair's dot product and the two row norms.  Limits: D % 64 == 0, 1 <= kmax <= 32, kmax <= M < 2^31.
// BF16 ROWS (the reference's `dtype: bfloat16`): seg_rownorms_kernel<bf16> and seg_knn_kernel<bf16, MET> take rows the caller
// has rounded to bf16 ONCE.  Everything after that cast is f32 and is the code above: the norms are f32 sums of the rounded
// values in a fixed order, the dots come from knn_stream_bf16 (bf16 MFMA, f32 accumulation), the ordering keys, the total
// order, the NaN and skip rules, the lists, the merge and the vote are shared with the f32 rows, not copied.  Both distances
// still come from one pass: there is no second, normalised-then-rounded copy of the keys.
#include "knn_common.hpp"

namespace octic {
namespace {

constexpr int KNN_BT = 2;       // 16-row query tiles per wave
constexpr int KNN_QT = 64 * KNN_BT;   // query rows per workgroup
constexpr int KNN_KMAX = 32;
using KnnAsc = KnnOrder<true>;
using KnnPlan = KnnPlanner<KNN_QT, 4, KNN_KMAX>;   // never below 4 key tiles a split

// The two ordering keys.  Contraction is off: the value must not depend on what the compiler fuses in which instantiation.
__device__ __forceinline__ float knn_l2(float qn, float kn, float dot) {
#pragma clang fp contract(off)
  const float s = qn + kn;
  const float t = 2.f * dot;
  const float d = s - t;
  return d == d ? d : KnnAsc::worst();
}
__device__ __forceinline__ float knn_cos(float qs, float ks, float dot) {   // qs, ks: the roots of the squared norms
#pragma clang fp contract(off)
  const float den = qs * ks;
  const float c = dot / den;
  const float d = 1.f - c;
  return d == d ? d : KnnAsc::worst();
}

// one wave per row; T = float or bf16, 16 bytes per lane and step
template <typename T>
__global__ __launch_bounds__(256) void seg_rownorms_kernel(const T* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                           float* __restrict__ norms) {
  constexpr int W = 16 / (int)sizeof(T);
  typedef __attribute__((ext_vector_type(W))) T vec;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const T* x = X + row * ldx;
  float s = 0.f;
  for (int c = W * lane; c < D; c += 64 * W) {
    const vec v = *(const vec*)(x + c);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float f = (float)v[j];
      s = fmaf(f, f, s);
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  if (lane == 0) norms[row] = s;
}

// Wave-wide sorted insert of (cd, ci) into the kmax-entry list (ld, li) of one query; lane j holds entry j.  The list is
// sorted by the total order, so the entries that precede the candidate are a prefix and its length is the insert position.
__device__ __forceinline__ void knn_insert(float* ld, int* li, float* thr, int kmax, int lane, float cd, int ci) {
  const int j = lane & 31;
  const float dj = ld[j];
  const int ij = li[j];
  const bool before = lane < kmax && KnnAsc::before(dj, ij, cd, ci);
  const int pos = __popcll(__ballot(before));
  if (pos >= kmax) return;                       // wave-uniform
  const float pd = __shfl_up(dj, 1);
  const int pi = __shfl_up(ij, 1);
  __builtin_amdgcn_wave_barrier();
  if (lane < kmax && lane >= pos) {
    const float nd = lane == pos ? cd : pd;
    ld[lane] = nd;
    li[lane] = lane == pos ? ci : pi;
    if (lane == kmax - 1) *thr = nd;
  }
  __builtin_amdgcn_wave_barrier();
}

// The per-key-tile hook of knn_stream: |key|^2 of the tile's keys, -1 for a key that is skipped or past the end of the range.
// Loaded with the tile's first prefetch, stored to Kn with its first staging.
struct SegKeyNorms {
  const float* __restrict__ knorm;
  const uint8_t* __restrict__ skip;
  int M;
  float* Kn;
  float knr;
  __device__ __forceinline__ void load(int kb) {
    if (threadIdx.x < KNN_KT) {
      const unsigned krow = (unsigned)kb + threadIdx.x;
      knr = (krow < (unsigned)M && !(skip && skip[krow])) ? knorm[krow] : -1.f;
    }
  }
  __device__ __forceinline__ void store() {
    if (threadIdx.x < KNN_KT) Kn[threadIdx.x] = knr;
  }
};

// The stream of the operand type: knn_stream for f32 rows, knn_stream_bf16 for bf16 rows, on LDS images of the same bytes.
template <typename T> struct KnnOperand;
template <> struct KnnOperand<float> {
  static constexpr int LD = KNN_LD;
  template <typename... A> static __device__ __forceinline__ void stream(A&&... a) { knn_stream<KNN_BT>(static_cast<A&&>(a)...); }
};
template <> struct KnnOperand<bf16> {
  static constexpr int LD = KNN_LD16;
  template <typename... A> static __device__ __forceinline__ void stream(A&&... a) { knn_stream_bf16<KNN_BT>(static_cast<A&&>(a)...); }
};

// wave w owns query rows 32 w .. 32 w + 31 of the tile (knn_stream<2>) and therefore their lists
template <typename T, int MET>
__global__ __launch_bounds__(256) void seg_knn_kernel(const T* __restrict__ Q, int64_t ldq, int64_t n,
                                                      const T* __restrict__ K, int64_t ldk, int M, int D,
                                                      const float* __restrict__ qnorm, const float* __restrict__ knorm,
                                                      const uint8_t* __restrict__ skip, int kmax, int tiles_per_split,
                                                      int* __restrict__ idx0, float* __restrict__ dist0, int* __restrict__ idx1,
                                                      float* __restrict__ dist1, int64_t ldo, int64_t split_stride) {
  constexpr int NL = MET == 3 ? 2 : 1;
  constexpr bool L2 = (MET & 1) != 0, COS = (MET & 2) != 0;
  constexpr int CS = NL - 1;                      // the list slot of cosine (L2, when asked for, is slot 0)
  __shared__ __attribute__((aligned(16))) T Qs[KNN_QT * KnnOperand<T>::LD];
  __shared__ __attribute__((aligned(16))) T Ks[KNN_KT * KnnOperand<T>::LD];
  __shared__ float Kn[KNN_KT];
  __shared__ float Qn[KNN_QT];
  __shared__ float Ld[NL][KNN_QT][KNN_KMAX];
  __shared__ int Li[NL][KNN_QT][KNN_KMAX];
  __shared__ float Thr[NL][KNN_QT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int64_t q0 = (int64_t)blockIdx.x * KNN_QT;

  for (int i = tid; i < NL * KNN_QT * KNN_KMAX; i += 256) {
    (&Ld[0][0][0])[i] = KnnAsc::worst();
    (&Li[0][0][0])[i] = -1;
  }
  if (tid < KNN_QT) {
    const bool live = q0 + tid < n;
    Qn[tid] = live ? qnorm[q0 + tid] : 0.f;
#pragma unroll
    for (int m = 0; m < NL; ++m) Thr[m][tid] = live ? KnnAsc::worst() : -KnnAsc::worst();   // a row past n admits nothing
  }
  __syncthreads();

  SegKeyNorms meta = {knorm, skip, M, Kn, -1.f};
  // ---- per key tile: ordering keys, the filter, the rare insert
  KnnOperand<T>::stream(Q, ldq, n, K, ldk, M, D, tiles_per_split, Qs, Ks, meta, [&](int t, const f32x4 (&acc)[KNN_BT][8]) {
    const int kb = t * KNN_KT;
    float kn[8], ks[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      kn[ct] = Kn[16 * ct + r];
      ks[ct] = COS ? sqrtf(fmaxf(kn[ct], 0.f)) : 0.f;
    }
#pragma unroll
    for (int bt = 0; bt < KNN_BT; ++bt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rowl = 32 * w + 16 * bt + 4 * q + e;
        const float qn = Qn[rowl];
        const float qs = COS ? sqrtf(qn) : 0.f;
        float thr[NL], d[NL][8];
#pragma unroll
        for (int m = 0; m < NL; ++m) thr[m] = Thr[m][rowl];
        bool any = false;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
          const bool dead = kn[ct] < 0.f;
          const float dot = acc[bt][ct][e];
          if (L2) {
            d[0][ct] = dead ? KnnAsc::worst() : knn_l2(qn, kn[ct], dot);
            any |= KnnAsc::beats(d[0][ct], thr[0]);
          }
          if (COS) {
            d[CS][ct] = dead ? KnnAsc::worst() : knn_cos(qs, ks[ct], dot);
            any |= KnnAsc::beats(d[CS][ct], thr[CS]);
          }
        }
        if (!__any(any)) continue;           // the common case once the lists are warm
#pragma unroll
        for (int m = 0; m < NL; ++m)
#pragma unroll
          for (int ct = 0; ct < 8; ++ct) {
            unsigned long long bal = __ballot(KnnAsc::beats(d[m][ct], thr[m]));
            while (bal) {                    // wave-uniform
              const int l = __ffsll((long long)bal) - 1;
              bal &= bal - 1;
              const float cd = __shfl(d[m][ct], l);
              const int crow = 32 * w + 16 * bt + 4 * (l >> 4) + e;
              const int ci = kb + 16 * ct + (l & 15);
              knn_insert(&Ld[m][crow][0], &Li[m][crow][0], &Thr[m][crow], kmax, lane, cd, ci);
            }
          }
      }
  });

  int* const oi[2] = {idx0, idx1};
  float* const od[2] = {dist0, dist1};
  knn_write_lists<NL, KNN_BT, KNN_KMAX>(&Ld[0][0][0], &Li[0][0][0], n, kmax, oi, od, ldo, split_stride);
}

template <typename T>
__device__ __forceinline__ int knn_label(const void* p, int64_t i) { return (int)((const T*)p)[i] & 255; }
__device__ __forceinline__ int knn_label_at(const void* p, int esize, int64_t i) {
  return esize == 1 ? knn_label<uint8_t>(p, i) : esize == 2 ? knn_label<int16_t>(p, i)
       : esize == 4 ? knn_label<int32_t>(p, i) : knn_label<int64_t>(p, i);
}

// thread = (query, pixel).  Adding neighbour j with value v raises only v's count, so the running mode either stays or becomes
// v: it becomes v when v's count exceeds the best count, or equals it with a smaller value (torch.mode's tie rule).
struct KnnVoteKs { int k[8]; };
__global__ __launch_bounds__(256) void seg_knn_vote_kernel(const int* __restrict__ idx, int64_t ldi, int64_t n,
                                                           const void* __restrict__ labels, int esize, int64_t R, int L,
                                                           KnnVoteKs ks, int nk, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * L) return;
  const int64_t row = i / L;
  const int l = (int)(i - row * L);
  const int kmax = ks.k[nk - 1];
  int v[KNN_KMAX];
  int bestc = 0, bestv = 0, next = 0;
#pragma unroll
  for (int j = 0; j < KNN_KMAX; ++j) {
    v[j] = -1;
    if (j < kmax) {
      const int64_t key = idx[row * ldi + j];
      if (key >= 0 && key < R) {
        v[j] = knn_label_at(labels, esize, key * L + l);
        int c = 1;
#pragma unroll
        for (int u = 0; u < j; ++u) c += v[u] == v[j];
        if (c > bestc || (c == bestc && v[j] < bestv)) { bestc = c; bestv = v[j]; }
      }
      if (next < nk && j + 1 == ks.k[next]) {
        out[((int64_t)next * n + row) * L + l] = (uint8_t)bestv;
        ++next;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline int knn_shape_check(int64_t n, int64_t M, int D, int kmax, int metrics) {
  return (metrics < 1 || metrics > 3) ? OCTIC_ESHAPE : KnnPlan::shape_check(n, M, D, kmax);
}

// the two entry points of each element type: every refusal comes before any launch; strides are in elements, rows 16-byte aligned
template <typename T>
int seg_rownorms(const T* X, int64_t ldx, int64_t N, int D, float* norms, void* stream) {
  if (!X || !norms) return OCTIC_ENULL;
  if (N < 1 || D < 64 || D % 64 || ldx < D || (N + 3) / 4 > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if ((((uintptr_t)X) & 15) || (ldx * sizeof(T) & 15)) return OCTIC_EALIGN;
  seg_rownorms_kernel<T><<<dim3((unsigned)((N + 3) / 4)), 256, 0, (hipStream_t)stream>>>(X, ldx, N, D, norms);
  return launch_status();
}

template <typename T>
int seg_knn(const T* Q, int64_t ldq, int64_t n, const T* K, int64_t ldk, int64_t M, int D, const float* qnorm,
            const float* knorm, const uint8_t* skip, int kmax, int metrics, int splits, int32_t* idx_l2, float* dist_l2,
            int32_t* idx_cos, float* dist_cos, int64_t ldo, void* workspace, void* stream) {
  if (!Q || !K || !qnorm || !knorm) return OCTIC_ENULL;
  if (int e = knn_shape_check(n, M, D, kmax, metrics)) return e;
  if (((metrics & 1) && (!idx_l2 || !dist_l2)) || ((metrics & 2) && (!idx_cos || !dist_cos))) return OCTIC_ENULL;
  if (splits < 0 || splits > KNN_MAX_SPLITS || ldq < D || ldk < D || ldo < kmax) return OCTIC_ESHAPE;
  if ((((uintptr_t)Q) & 15) || (((uintptr_t)K) & 15) || (ldq * sizeof(T) & 15) || (ldk * sizeof(T) & 15)) return OCTIC_EALIGN;
  int* const out_i[2] = {(metrics & 1) ? idx_l2 : idx_cos, idx_cos};
  float* const out_d[2] = {(metrics & 1) ? dist_l2 : dist_cos, dist_cos};
  const hipStream_t st = (hipStream_t)stream;
  return KnnPlan::run<KnnAsc>(n, M, kmax, splits, metrics == 3 ? 2 : 1, out_i, out_d, ldo, workspace, st,
                              [&](dim3 grid, int tps, int* const* ki, float* const* kd, int64_t kld, int64_t stride) {
#define KNN_CALL(MET_) seg_knn_kernel<T, MET_><<<grid, 256, 0, st>>>(Q, ldq, n, K, ldk, (int)M, D, qnorm, knorm, skip, kmax, tps, \
                                                                    ki[0], kd[0], ki[1], kd[1], kld, stride)
    if (metrics == 1) KNN_CALL(1); else if (metrics == 2) KNN_CALL(2); else KNN_CALL(3);
#undef KNN_CALL
  });
}

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_seg_knn_plan(int64_t n, int64_t M, int D, int kmax, int metrics, int* out) {
  if (!out) return OCTIC_ENULL;
  if (int e = knn_shape_check(n, M, D, kmax, metrics)) return e;
  KnnPlan::plan(n, M, out);
  return OCTIC_OK;
}

int64_t octic_seg_knn_workspace_bytes(int64_t n, int64_t M, int D, int kmax, int metrics, int splits) {
  if (int e = knn_shape_check(n, M, D, kmax, metrics)) return e;
  return KnnPlan::workspace_bytes(n, M, kmax, metrics == 3 ? 2 : 1, splits);
}

int octic_seg_rownorms(const float* X, int64_t ldx, int64_t N, int D, float* norms, void* stream) {
  return seg_rownorms(X, ldx, N, D, norms, stream);
}
int octic_seg_rownorms_bf16(const void* X, int64_t ldx, int64_t N, int D, float* norms, void* stream) {
  return seg_rownorms((const bf16*)X, ldx, N, D, norms, stream);
}

int octic_seg_knn(const float* Q, int64_t ldq, int64_t n, const float* K, int64_t ldk, int64_t M, int D, const float* qnorm,
                  const float* knorm, const uint8_t* skip, int kmax, int metrics, int splits, int32_t* idx_l2, float* dist_l2,
                  int32_t* idx_cos, float* dist_cos, int64_t ldo, void* workspace, void* stream) {
  return seg_knn(Q, ldq, n, K, ldk, M, D, qnorm, knorm, skip, kmax, metrics, splits, idx_l2, dist_l2, idx_cos, dist_cos, ldo,
                 workspace, stream);
}
int octic_seg_knn_bf16(const void* Q, int64_t ldq, int64_t n, const void* K, int64_t ldk, int64_t M, int D, const float* qnorm,
                       const float* knorm, const uint8_t* skip, int kmax, int metrics, int splits, int32_t* idx_l2, float* dist_l2,
                       int32_t* idx_cos, float* dist_cos, int64_t ldo, void* workspace, void* stream) {
  return seg_knn((const bf16*)Q, ldq, n, (const bf16*)K, ldk, M, D, qnorm, knorm, skip, kmax, metrics, splits, idx_l2, dist_l2,
                 idx_cos, dist_cos, ldo, workspace, stream);
}

int octic_seg_knn_vote(const int32_t* idx, int64_t ldi, int64_t n, const void* labels, int esize, int64_t R, int L, const int* ks,
                       int nk, uint8_t* out, void* stream) {
  if (!idx || !labels || !ks || !out) return OCTIC_ENULL;
  if (n < 1 || R < 1 || L < 1 || nk < 1 || nk > 8) return OCTIC_ESHAPE;
  if (esize != 1 && esize != 2 && esize != 4 && esize != 8) return OCTIC_EDTYPE;
  if (((uintptr_t)labels) & (esize - 1)) return OCTIC_EALIGN;
  KnnVoteKs k;
  for (int i = 0; i < 8; ++i) k.k[i] = i < nk ? ks[i] : 0;
  for (int i = 0; i < nk; ++i)
    if (k.k[i] < 1 || k.k[i] > KNN_KMAX || (i && k.k[i] <= k.k[i - 1])) return OCTIC_ESHAPE;   // ascending, 1 .. 32
  if (ldi < k.k[nk - 1]) return OCTIC_ESHAPE;
  const int64_t blocks = (n * L + 255) / 256;
  if (blocks > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  seg_knn_vote_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(idx, ldi, n, labels, esize, R, L, k, nk, out);
  return launch_status();
}

}  // extern "C"
