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
//   3. seg_knn_merge_kernel  : when the key axis is split over workgroups (few queries), every split writes its own sorted list
//                              and one wave per (query, metric) merges them.
//   4. seg_knn_vote_kernel   : thread = (query, pixel): the running mode of labels[idx[query, 0 .. k-1], pixel] for up to 8
//                              ascending k, ties to the smallest value (torch.mode), written as uint8 [n_k, n, L].
// TOTAL ORDER: (distance, key row index) - the smaller distance first, on equal distance the lower index first.  torch.topk
// leaves ties unspecified; this rule is ours.  A distance that is NaN (a zero row under cosine) counts as +inf, and a key with
// distance +inf (a skipped row) is never listed: a query with fewer than kmax listable keys ends on (+inf, -1) entries.
// DETERMINISM: the dot product of a pair is one fmaf chain over the channels in an order that depends on D alone (within each
// 16 channels: e, 4 + e, 8 + e, 12 + e for e = 0 .. 3), and the distance is a contraction-free expression of that dot and the
// two row norms.  It does not depend on the pair's place in a tile, on the split or on the batch, so the merged lists are the
// global answer and results are bitwise equal for every split count and every query order.  No floating-point atomics.
// Every row and element offset is 64-bit.  Limits: D % 64 == 0, 1 <= kmax <= 32, kmax <= M < 2^31.
#include "octic_common.hpp"

namespace octic {
namespace {

constexpr int KNN_QT = 128;     // query rows per workgroup
constexpr int KNN_KT = 128;     // keys per tile
constexpr int KNN_LD = 36;      // 32 k + 4: as SEG_FW_LD of segeval.hip
constexpr int KNN_KMAX = 32;
constexpr int KNN_MAX_SPLITS = 64;

__device__ __forceinline__ f32x4 knn_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The two ordering keys.  Contraction is off: the value must not depend on what the compiler fuses in which instantiation.
__device__ __forceinline__ float knn_l2(float qn, float kn, float dot) {
#pragma clang fp contract(off)
  const float s = qn + kn;
  const float t = 2.f * dot;
  const float d = s - t;
  return d == d ? d : INFINITY;
}
__device__ __forceinline__ float knn_cos(float qs, float ks, float dot) {   // qs, ks: the roots of the squared norms
#pragma clang fp contract(off)
  const float den = qs * ks;
  const float c = dot / den;
  const float d = 1.f - c;
  return d == d ? d : INFINITY;
}

__device__ __forceinline__ bool knn_before(float da, int ia, float db, int ib) {   // (da, ia) strictly precedes (db, ib)
  return da < db || (da == db && (unsigned)ia < (unsigned)ib);
}

// one wave per row
__global__ __launch_bounds__(256) void seg_rownorms_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                           float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* x = X + row * ldx;
  float s = 0.f;
  for (int c = 4 * lane; c < D; c += 256) {
    const f32x4 v = *(const f32x4*)(x + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) s = fmaf(v[j], v[j], s);
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
  const bool before = lane < kmax && knn_before(dj, ij, cd, ci);
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

// wave w owns query rows 32 w .. 32 w + 31 of the tile (2 x 8 tiles of 16 x 16) and therefore their lists: accumulator element
// e of tile (bt, ct) in lane (r, q) is dot(query 32 w + 16 bt + 4 q + e, key 16 ct + r).  Keys stream in ascending index order
// inside a split, so a key whose distance EQUALS the current kmax-th best loses to it by the index rule: the filter is a strict <.
template <int MET>
__global__ __launch_bounds__(256) void seg_knn_kernel(const float* __restrict__ Q, int64_t ldq, int64_t n,
                                                      const float* __restrict__ K, int64_t ldk, int M, int D,
                                                      const float* __restrict__ qnorm, const float* __restrict__ knorm,
                                                      const uint8_t* __restrict__ skip, int kmax, int tiles_per_split,
                                                      int* __restrict__ idx0, float* __restrict__ dist0, int* __restrict__ idx1,
                                                      float* __restrict__ dist1, int64_t ldo, int64_t split_stride) {
  constexpr int NL = MET == 3 ? 2 : 1;
  constexpr bool L2 = (MET & 1) != 0, COS = (MET & 2) != 0;
  constexpr int CS = NL - 1;                      // the list slot of cosine (L2, when asked for, is slot 0)
  __shared__ __attribute__((aligned(16))) float Qs[KNN_QT * KNN_LD];
  __shared__ __attribute__((aligned(16))) float Ks[KNN_KT * KNN_LD];
  __shared__ float Kn[KNN_KT];                    // |key|^2, -1 for a key that is skipped or past the end of the range
  __shared__ float Qn[KNN_QT];
  __shared__ float Ld[NL][KNN_QT][KNN_KMAX];
  __shared__ int Li[NL][KNN_QT][KNN_KMAX];
  __shared__ float Thr[NL][KNN_QT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;   // staging: 32 rows x 8 float4 per pass, 4 passes per tile
  const int64_t q0 = (int64_t)blockIdx.x * KNN_QT;
  const int ktiles = (int)(((int64_t)M + KNN_KT - 1) / KNN_KT);
  const int t0 = blockIdx.y * tiles_per_split;
  const int t1 = t0 + tiles_per_split < ktiles ? t0 + tiles_per_split : ktiles;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  for (int i = tid; i < NL * KNN_QT * KNN_KMAX; i += 256) {
    (&Ld[0][0][0])[i] = INFINITY;
    (&Li[0][0][0])[i] = -1;
  }
  if (tid < KNN_QT) {
    const bool live = q0 + tid < n;
    Qn[tid] = live ? qnorm[q0 + tid] : 0.f;
#pragma unroll
    for (int m = 0; m < NL; ++m) Thr[m][tid] = live ? INFINITY : -INFINITY;   // a row past n admits nothing
  }

  __syncthreads();

  f32x4 qr[4], kr[4];
  float knr = -1.f;
  auto fetch = [&](int t, int k0) {
    const int kb = t * KNN_KT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t qrow = q0 + srow + 32 * i;
      qr[i] = qrow < n ? *(const f32x4*)(Q + qrow * ldq + k0 + sc4) : zero;
      const int64_t krow = (int64_t)kb + srow + 32 * i;
      kr[i] = krow < M ? *(const f32x4*)(K + krow * ldk + k0 + sc4) : zero;
    }
    if (k0 == 0 && tid < KNN_KT) {
      const int64_t krow = (int64_t)kb + tid;
      knr = (krow < M && !(skip && skip[krow])) ? knorm[krow] : -1.f;
    }
  };

  if (t0 < t1) fetch(t0, 0);
  for (int t = t0; t < t1; ++t) {
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = zero;
    for (int k0 = 0; k0 < D; k0 += 32) {
      __syncthreads();                       // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *(f32x4*)(Qs + (srow + 32 * i) * KNN_LD + sc4) = qr[i];
        *(f32x4*)(Ks + (srow + 32 * i) * KNN_LD + sc4) = kr[i];
      }
      if (k0 == 0 && tid < KNN_KT) Kn[tid] = knr;
      __syncthreads();
      if (k0 + 32 < D) fetch(t, k0 + 32);    // in flight under the products
      else if (t + 1 < t1) fetch(t + 1, 0);  // ... and under the epilogue
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x4 a4[2];
#pragma unroll
        for (int bt = 0; bt < 2; ++bt) a4[bt] = *(const f32x4*)(Qs + (32 * w + 16 * bt + r) * KNN_LD + 16 * j + 4 * q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x4 b4[4];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) b4[ct] = *(const f32x4*)(Ks + (16 * (ct + 4 * h) + r) * KNN_LD + 16 * j + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int bt = 0; bt < 2; ++bt)
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) acc[bt][ct + 4 * h] = knn_mfma16(a4[bt][e], b4[ct][e], acc[bt][ct + 4 * h]);
        }
      }
    }

    // ---- epilogue: ordering keys, the filter, the rare insert
    const int kb = t * KNN_KT;
    float kn[8], ks[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      kn[ct] = Kn[16 * ct + r];
      ks[ct] = COS ? sqrtf(fmaxf(kn[ct], 0.f)) : 0.f;
    }
#pragma unroll
    for (int bt = 0; bt < 2; ++bt)
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
            d[0][ct] = dead ? INFINITY : knn_l2(qn, kn[ct], dot);
            any |= d[0][ct] < thr[0];
          }
          if (COS) {
            d[CS][ct] = dead ? INFINITY : knn_cos(qs, ks[ct], dot);
            any |= d[CS][ct] < thr[CS];
          }
        }
        if (!__any(any)) continue;           // the common case once the lists are warm
#pragma unroll
        for (int m = 0; m < NL; ++m)
#pragma unroll
          for (int ct = 0; ct < 8; ++ct) {
            unsigned long long bal = __ballot(d[m][ct] < thr[m]);
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
  }

  // ---- the wave's 32 lists, lane = entry
  __builtin_amdgcn_wave_barrier();
  const int64_t sp = (int64_t)blockIdx.y * split_stride;
  for (int i = 0; i < 32; ++i) {
    const int rowl = 32 * w + i;
    const int64_t row = q0 + rowl;
    if (row >= n) break;
    if (lane < kmax) {
      idx0[sp + row * ldo + lane] = Li[0][rowl][lane];
      dist0[sp + row * ldo + lane] = Ld[0][rowl][lane];
      if (NL == 2) {
        idx1[sp + row * ldo + lane] = Li[1][rowl][lane];
        dist1[sp + row * ldo + lane] = Ld[1][rowl][lane];
      }
    }
  }
}

// one wave per (query, list): lane s walks the sorted list of split s; kmax times the smallest head over the lanes is taken
struct KnnMergeArgs {
  const int* pidx[2];
  const float* pdist[2];
  int* idx[2];
  float* dist[2];
};
__global__ __launch_bounds__(256) void seg_knn_merge_kernel(KnnMergeArgs a, int64_t n, int kmax, int splits, int64_t ldo, int nl) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= n * nl) return;                    // wave-uniform
  const int m = (int)(item / n);
  const int64_t row = item - (int64_t)m * n;
  const int* pi = a.pidx[m] + ((int64_t)lane * n + row) * kmax;
  const float* pd = a.pdist[m] + ((int64_t)lane * n + row) * kmax;
  int p = 0;
  for (int j = 0; j < kmax; ++j) {
    const bool has = lane < splits && p < kmax;
    float d = has ? pd[p] : INFINITY;
    int i = has ? pi[p] : -1;
    const float hd = d;
    const int hi = i;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float od = __shfl_xor(d, o);
      const int oi = __shfl_xor(i, o);
      if (knn_before(od, oi, d, i)) { d = od; i = oi; }
    }
    if (has && hi == i && hd == d && i >= 0) ++p;   // a key row lives in exactly one split: one lane advances
    if (lane == 0) {
      a.idx[m][row * ldo + j] = i;
      a.dist[m][row * ldo + j] = d;
    }
  }
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
  if (n < 1 || M < 1 || M > 0x7FFFFFFFll || D < 64 || D % 64 || kmax < 1 || kmax > KNN_KMAX || metrics < 1 || metrics > 3)
    return OCTIC_ESHAPE;
  if (M < kmax) return OCTIC_ESHAPE;             // fewer keys than neighbours asked for
  if ((n + KNN_QT - 1) / KNN_QT > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  return OCTIC_OK;
}
inline int knn_ktiles(int64_t M) { return (int)((M + KNN_KT - 1) / KNN_KT); }
// the key axis is split only when the query tiles alone leave CUs idle, and never below 4 key tiles a split (the lists of a
// split warm up on its first tile)
inline int knn_plan_splits(int64_t n, int64_t M) {
  const int64_t qtiles = (n + KNN_QT - 1) / KNN_QT;
  const int cus = device_cus();
  if (qtiles >= cus) return 1;
  int64_t s = (cus + qtiles - 1) / qtiles;
  const int64_t most = knn_ktiles(M) / 4;
  if (s > most) s = most;
  if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}
// what a requested split count becomes: whole key tiles per split, no empty split
inline void knn_resolve(int64_t n, int64_t M, int requested, int* splits, int* tiles_per_split) {
  const int ktiles = knn_ktiles(M);
  int s = requested > 0 ? requested : knn_plan_splits(n, M);
  if (s > ktiles) s = ktiles;
  const int tps = (ktiles + s - 1) / s;
  *tiles_per_split = tps;
  *splits = (ktiles + tps - 1) / tps;
}
inline int64_t knn_align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_seg_knn_plan(int64_t n, int64_t M, int D, int kmax, int metrics, int* out) {
  if (!out) return OCTIC_ENULL;
  if (int e = knn_shape_check(n, M, D, kmax, metrics)) return e;
  int splits, tps;
  knn_resolve(n, M, 0, &splits, &tps);
  out[0] = splits;
  out[1] = KNN_QT;
  out[2] = KNN_KT;
  out[3] = splits > 1 ? 1 : 0;                   // workspace class: 0 = none read, 1 = the partial lists of the splits
  return OCTIC_OK;
}

int64_t octic_seg_knn_workspace_bytes(int64_t n, int64_t M, int D, int kmax, int metrics, int splits) {
  if (int e = knn_shape_check(n, M, D, kmax, metrics)) return e;
  if (splits < 0 || splits > KNN_MAX_SPLITS) return OCTIC_ESHAPE;
  int s, tps;
  knn_resolve(n, M, splits, &s, &tps);
  if (s == 1) return 256;
  const int nl = metrics == 3 ? 2 : 1;
  return 2 * nl * knn_align256(4ll * s * n * kmax);
}

int octic_seg_rownorms(const float* X, int64_t ldx, int64_t N, int D, float* norms, void* stream) {
  if (!X || !norms) return OCTIC_ENULL;
  if (N < 1 || D < 64 || D % 64 || ldx < D || (N + 3) / 4 > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if ((((uintptr_t)X) & 15) || (ldx & 3)) return OCTIC_EALIGN;
  seg_rownorms_kernel<<<dim3((unsigned)((N + 3) / 4)), 256, 0, (hipStream_t)stream>>>(X, ldx, N, D, norms);
  return launch_status();
}

int octic_seg_knn(const float* Q, int64_t ldq, int64_t n, const float* K, int64_t ldk, int64_t M, int D, const float* qnorm,
                  const float* knorm, const uint8_t* skip, int kmax, int metrics, int splits, int32_t* idx_l2, float* dist_l2,
                  int32_t* idx_cos, float* dist_cos, int64_t ldo, void* workspace, void* stream) {
  if (!Q || !K || !qnorm || !knorm) return OCTIC_ENULL;
  if (int e = knn_shape_check(n, M, D, kmax, metrics)) return e;
  if (((metrics & 1) && (!idx_l2 || !dist_l2)) || ((metrics & 2) && (!idx_cos || !dist_cos))) return OCTIC_ENULL;
  if (splits < 0 || splits > KNN_MAX_SPLITS || ldq < D || ldk < D || ldo < kmax) return OCTIC_ESHAPE;
  if ((((uintptr_t)Q) & 15) || (((uintptr_t)K) & 15) || (ldq & 3) || (ldk & 3)) return OCTIC_EALIGN;
  int s, tps;
  knn_resolve(n, M, splits, &s, &tps);
  if (s > 1 && !workspace) return OCTIC_ENULL;
  if (s > 1 && (((uintptr_t)workspace) & 255)) return OCTIC_EALIGN;
  const int nl = metrics == 3 ? 2 : 1;
  int* out_i[2] = {(metrics & 1) ? idx_l2 : idx_cos, idx_cos};
  float* out_d[2] = {(metrics & 1) ? dist_l2 : dist_cos, dist_cos};
  int* ki[2] = {out_i[0], out_i[1]};
  float* kd[2] = {out_d[0], out_d[1]};
  int64_t kld = ldo, stride = 0;
  if (s > 1) {
    const int64_t part = knn_align256(4ll * s * n * kmax);
    for (int m = 0; m < nl; ++m) {
      ki[m] = (int*)((char*)workspace + (2 * m) * part);
      kd[m] = (float*)((char*)workspace + (2 * m + 1) * part);
    }
    kld = kmax;
    stride = n * kmax;
  }
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + KNN_QT - 1) / KNN_QT), (unsigned)s);
#define KNN_CALL(MET_) seg_knn_kernel<MET_><<<grid, 256, 0, st>>>(Q, ldq, n, K, ldk, (int)M, D, qnorm, knorm, skip, kmax, tps, \
                                                                 ki[0], kd[0], ki[1], kd[1], kld, stride)
  if (metrics == 1) KNN_CALL(1); else if (metrics == 2) KNN_CALL(2); else KNN_CALL(3);
#undef KNN_CALL
  if (s > 1) {
    KnnMergeArgs a;
    for (int m = 0; m < 2; ++m) {
      a.pidx[m] = ki[m < nl ? m : 0];
      a.pdist[m] = kd[m < nl ? m : 0];
      a.idx[m] = out_i[m < nl ? m : 0];
      a.dist[m] = out_d[m < nl ? m : 0];
    }
    const int64_t items = n * nl;
    seg_knn_merge_kernel<<<dim3((unsigned)((items + 3) / 4)), 256, 0, st>>>(a, n, kmax, s, ldo, nl);
  }
  return launch_status();
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
