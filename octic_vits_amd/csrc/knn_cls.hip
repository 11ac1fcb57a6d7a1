// The k-NN classification evaluation (dinov2/eval/knn.py: KnnModule) on resident f32 class-token features: for every query row
// the kmax key rows with the LARGEST inner product, then the temperature-softmax vote over classes and the top-1 / top-5 hits.
// Neither the similarity matrix nor the [batch, kmax, classes] one-hot product reaches memory.
//   1. knn_topk_kernel       : workgroup = 64 query rows x one contiguous range of key tiles (128 keys each).  The design of
//                              seg_knn_kernel (segknn.hip) at half its query tile: both tiles go through LDS in chunks of 32
//                              channels, the dot products run on the exact-f32 MFMA (16x16x4), one accumulator chain over all of D
//                              per pair.  After a key tile every accumulator is compared with the query's current kmax-th best
//                              (one LDS word per query); only survivors enter the query's sorted list (LDS, up to 256 entries) by
//                              a wave-wide sorted insert, lane = four consecutive entries (one LDS round trip).  64 rows x 256
//                              entries x (f32, int32) are 128 KiB of the CU's 160 KiB: one workgroup per CU, as seg_knn_kernel.
//   2. knn_topk_merge_kernel : when the key axis is split over workgroups (few queries), every split writes its own sorted list
//                              and one wave per query merges them.
//   3. knn_vote_kernel       : workgroup = one query row.  w = softmax(sim * inv_T) over all kmax entries (max-subtracted, the sum
//                              in rank order), then thread = class: the rank-order sum of the weights of its class, written at
//                              every k of the ascending list ks.  With targets, the rank of the target class under (proba
//                              descending, class index ascending) is counted on the way and the hits are added to int64 counters.
// TOTAL ORDER: (similarity descending, key row index ascending).  torch.topk leaves ties unspecified; this rule is ours, the
// mirror of segknn.hip's.  A NaN similarity counts as -inf, and a key at -inf is never listed: a query with fewer than kmax
// listable keys ends on (-inf, -1) entries.
// DETERMINISM: the dot product of a pair is one fmaf chain over the channels in an order that depends on D alone (within each 16
// channels: e, 4 + e, 8 + e, 12 + e for e = 0 .. 3, as segknn.hip).  It does not depend on the pair's place in a tile, on the
// split or on the batch, so the merged lists are the global answer and results are bitwise equal for every split count and every
// query order.  No floating-point atomics (the hit counters are integers).  Every row and element offset is 64-bit.
// Limits: D % 64 == 0, 1 <= kmax <= 256 (OCTIC_KNN_KMAX), kmax <= M < 2^31, 0 <= splits <= 64.
#include "octic_common.hpp"

namespace octic {
namespace {

constexpr int KC_QT = 64;       // query rows per workgroup
constexpr int KC_KT = 128;      // keys per tile
constexpr int KC_LD = 36;       // 32 k + 4: as KNN_LD of segknn.hip
constexpr int KC_KMAX = OCTIC_KNN_KMAX;
constexpr int KC_MAX_SPLITS = 64;
constexpr int KC_MIN_TILES = 8; // an automatic split never gets fewer key tiles: its lists warm up on its first kmax keys
static_assert(KC_KMAX == 256, "knn_topk_kernel: 64 lanes x 4 entries, and the LDS budget is worked out for 256 entries");
typedef __attribute__((ext_vector_type(4))) int kc_i32x4;

__device__ __forceinline__ f32x4 kc_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bool kc_before(float sa, int ia, float sb, int ib) {   // (sa, ia) strictly precedes (sb, ib)
  return sa > sb || (sa == sb && (unsigned)ia < (unsigned)ib);
}

// Wave-wide sorted insert of (cs, ci) into the kmax-entry list (ls, li) of one query; lane l holds the four entries 4 l .. 4 l + 3
// (one 16-byte LDS read per array, 64 x 4 = KC_KMAX).  The list is sorted by the total order, so the entries that precede the
// candidate are a prefix: the lanes' counts read 4, .., 4, c, 0, .., 0 and their sum - four ballots - is the insert position.
// The predecessor of a lane's first entry is read with the quad, so an insert is one LDS round trip.  Entries kmax ..
// 4 ceil(kmax / 4) - 1 of the last lane's quad are scratch: never counted, never written out.  A candidate that the list's
// kmax-th entry precedes (the bar rose since the caller's ballot) changes nothing.
__device__ __forceinline__ void kc_insert(float* ls, int* li, float* thr, int kmax, int lane, float cs, int ci) {
  const int e0 = 4 * lane;
  const bool mine = e0 < kmax;
  f32x4 s4 = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  kc_i32x4 i4 = {-1, -1, -1, -1};
  float ps = -INFINITY;                                  // the predecessor of the lane's first entry, read in the same round
  int pi = -1;
  if (mine) {
    s4 = *(const f32x4*)(ls + e0);
    i4 = *(const kc_i32x4*)(li + e0);
    if (lane) {
      ps = ls[e0 - 1];
      pi = li[e0 - 1];
    }
  }
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c += (e0 + j < kmax && kc_before(s4[j], i4[j], cs, ci)) ? 1 : 0;
  const int pos = __popcll(__ballot(c >= 1)) + __popcll(__ballot(c >= 2)) + __popcll(__ballot(c >= 3)) + __popcll(__ballot(c >= 4));
  if (pos >= kmax) return;                               // wave-uniform
  f32x4 ns;
  kc_i32x4 ni;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = e0 + j;
    const float prev_s = j ? s4[j ? j - 1 : 0] : ps;
    const int prev_i = j ? i4[j ? j - 1 : 0] : pi;
    ns[j] = e < pos ? s4[j] : (e == pos ? cs : prev_s);
    ni[j] = e < pos ? i4[j] : (e == pos ? ci : prev_i);
  }
  __builtin_amdgcn_wave_barrier();
  if (mine && e0 + 3 >= pos) {
    *(f32x4*)(ls + e0) = ns;
    *(kc_i32x4*)(li + e0) = ni;
    if (lane == ((kmax - 1) >> 2)) {
      const int j = (kmax - 1) & 3;
      *thr = j == 0 ? ns[0] : j == 1 ? ns[1] : j == 2 ? ns[2] : ns[3];
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// wave w owns query rows 16 w .. 16 w + 15 of the tile (1 x 8 tiles of 16 x 16) and therefore their lists: accumulator element e
// of tile ct in lane (r, q) is dot(query 16 w + 4 q + e, key 16 ct + r).  Keys stream in ascending index order inside a split, so
// a key whose similarity EQUALS the current kmax-th best loses to it by the index rule: the filter is a strict >.
__global__ __launch_bounds__(256) void knn_topk_kernel(const float* __restrict__ Q, int64_t ldq, int64_t n,
                                                       const float* __restrict__ K, int64_t ldk, int M, int D, int kmax,
                                                       int tiles_per_split, int* __restrict__ idx, float* __restrict__ sim,
                                                       int64_t ldo, int64_t split_stride) {
  __shared__ __attribute__((aligned(16))) float Qs[KC_QT * KC_LD];
  __shared__ __attribute__((aligned(16))) float Ks[KC_KT * KC_LD];
  __shared__ __attribute__((aligned(16))) float Ls[KC_QT][KC_KMAX];
  __shared__ __attribute__((aligned(16))) int Li[KC_QT][KC_KMAX];
  __shared__ float Thr[KC_QT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;   // staging: 32 rows x 8 float4 per pass; 2 passes for Q, 4 for K
  const int64_t q0 = (int64_t)blockIdx.x * KC_QT;
  const int ktiles = (int)(((int64_t)M + KC_KT - 1) / KC_KT);
  const int t0 = blockIdx.y * tiles_per_split;
  const int t1 = t0 + tiles_per_split < ktiles ? t0 + tiles_per_split : ktiles;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  for (int i = tid; i < KC_QT * KC_KMAX; i += 256) {
    (&Ls[0][0])[i] = -INFINITY;
    (&Li[0][0])[i] = -1;
  }
  if (tid < KC_QT) Thr[tid] = q0 + tid < n ? -INFINITY : INFINITY;   // a row past n admits nothing
  __syncthreads();

  f32x4 qr[2], kr[4];
  auto fetch = [&](int t, int k0) {
    const int kb = t * KC_KT;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t qrow = q0 + srow + 32 * i;
      qr[i] = qrow < n ? *(const f32x4*)(Q + qrow * ldq + k0 + sc4) : zero;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t krow = (int64_t)kb + srow + 32 * i;
      kr[i] = krow < M ? *(const f32x4*)(K + krow * ldk + k0 + sc4) : zero;
    }
  };

  if (t0 < t1) fetch(t0, 0);
  for (int t = t0; t < t1; ++t) {
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = zero;
    for (int k0 = 0; k0 < D; k0 += 32) {
      __syncthreads();                       // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int i = 0; i < 2; ++i) *(f32x4*)(Qs + (srow + 32 * i) * KC_LD + sc4) = qr[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(Ks + (srow + 32 * i) * KC_LD + sc4) = kr[i];
      __syncthreads();
      if (k0 + 32 < D) fetch(t, k0 + 32);    // in flight under the products
      else if (t + 1 < t1) fetch(t + 1, 0);  // ... and under the epilogue
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4 a4 = *(const f32x4*)(Qs + (16 * w + r) * KC_LD + 16 * j + 4 * q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x4 b4[4];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) b4[ct] = *(const f32x4*)(Ks + (16 * (ct + 4 * h) + r) * KC_LD + 16 * j + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct + 4 * h] = kc_mfma16(a4[e], b4[ct][e], acc[ct + 4 * h]);
        }
      }
    }

    // ---- epilogue: the filter, the rare insert
    const int kb = t * KC_KT;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rowl = 16 * w + 4 * q + e;
      const float thr = Thr[rowl];
      float s[8];
      bool any = false;
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const float dot = acc[ct][e];
        const bool dead = (int64_t)kb + 16 * ct + r >= M;
        s[ct] = (dead || dot != dot) ? -INFINITY : dot;
        any |= s[ct] > thr;
      }
      if (!__any(any)) continue;             // the common case once the lists are warm
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        unsigned long long bal = __ballot(s[ct] > thr);
        while (bal) {                        // wave-uniform
          const int l = __ffsll((long long)bal) - 1;
          bal &= bal - 1;
          const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s[ct]), l));
          const int crow = 16 * w + 4 * (l >> 4) + e;   // (a candidate the row's bar has overtaken since the ballot is refused inside)
          kc_insert(&Ls[crow][0], &Li[crow][0], &Thr[crow], kmax, lane, cs, kb + 16 * ct + (l & 15));
        }
      }
    }
  }

  // ---- the wave's 16 lists, lane = entry modulo 64
  __builtin_amdgcn_wave_barrier();
  const int64_t sp = (int64_t)blockIdx.y * split_stride;
  for (int i = 0; i < 16; ++i) {
    const int rowl = 16 * w + i;
    const int64_t row = q0 + rowl;
    if (row >= n) break;
    for (int e = lane; e < kmax; e += 64) {
      idx[sp + row * ldo + e] = Li[rowl][e];
      sim[sp + row * ldo + e] = Ls[rowl][e];
    }
  }
}

// one wave per query: lane s walks the sorted list of split s; kmax times the best head over the lanes is taken
__global__ __launch_bounds__(256) void knn_topk_merge_kernel(const int* __restrict__ pidx, const float* __restrict__ psim,
                                                             int* __restrict__ idx, float* __restrict__ sim, int64_t n, int kmax,
                                                             int splits, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                          // wave-uniform
  const int* pi = pidx + ((int64_t)lane * n + row) * kmax;
  const float* ps = psim + ((int64_t)lane * n + row) * kmax;
  int p = 0;
  for (int j = 0; j < kmax; ++j) {
    const bool has = lane < splits && p < kmax;
    float s = has ? ps[p] : -INFINITY;
    int i = has ? pi[p] : -1;
    const float hs = s;
    const int hi = i;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float os = __shfl_xor(s, o);
      const int oi = __shfl_xor(i, o);
      if (kc_before(os, oi, s, i)) { s = os; i = oi; }
    }
    if (has && hi == i && hs == s && i >= 0) ++p;   // a key row lives in exactly one split: one lane advances
    if (lane == 0) {
      idx[row * ldo + j] = i;
      sim[row * ldo + j] = s;
    }
  }
}

struct KcVoteKs { int k[8]; };
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ sim, const int* __restrict__ idx, int64_t ldi,
                                                       int64_t n, int kmax, const int64_t* __restrict__ labels, int64_t M, int C,
                                                       float inv_T, KcVoteKs ks, int nk, float* __restrict__ probas,
                                                       const int64_t* __restrict__ targets,
                                                       unsigned long long* __restrict__ counters) {
  __shared__ float Z[KC_KMAX];     // sim * inv_T, then exp(z - max)
  __shared__ float W[KC_KMAX];     // the softmax weights; 0 for an entry that casts no vote
  __shared__ int Lab[KC_KMAX];     // the neighbour's class, -1 for an entry that casts no vote
  __shared__ int Rank[8];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (tid < 8) Rank[tid] = 0;
  if (tid < kmax) {
    const float s = sim[row * ldi + tid];
    const int64_t key = idx[row * ldi + tid];
    int lab = -1;
    if (key >= 0 && key < M) {
      const int64_t v = labels[key];
      if (v >= 0 && v < C) lab = (int)v;
    }
    const float z = s * inv_T;
    Z[tid] = z == z ? z : -INFINITY;
    Lab[tid] = lab;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = 0; j < kmax; ++j) m = fmaxf(m, Z[j]);
  __syncthreads();
  if (tid < kmax) {
    const float z = Z[tid];
    Z[tid] = m == -INFINITY ? 0.f : (z == m ? 1.f : expf(z - m));
  }
  __syncthreads();
  float total = 0.f;
  for (int j = 0; j < kmax; ++j) total += Z[j];      // rank order, the same chain in every thread
  if (tid < kmax) W[tid] = (total > 0.f && Lab[tid] >= 0) ? Z[tid] / total : 0.f;
  __syncthreads();

  // the target's own probas, by the chain its class thread runs below: equal bits
  int64_t tgt = -1;
  float pt[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) pt[i] = 0.f;
  if (targets) {
    tgt = targets[row];
    if (tgt < 0 || tgt >= C) tgt = -1;
    if (tgt >= 0) {
      float a = 0.f;
      int next = 0;
      for (int j = 0; j < kmax; ++j) {
        a += Lab[j] == (int)tgt ? W[j] : 0.f;
        if (next < nk && j + 1 == ks.k[next]) {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (i == next) pt[i] = a;
          ++next;
        }
      }
    }
  }
  int ahead[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ahead[i] = 0;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    int next = 0;
    for (int j = 0; j < kmax; ++j) {
      a += Lab[j] == c ? W[j] : 0.f;
      if (next < nk && j + 1 == ks.k[next]) {
        probas[((int64_t)next * n + row) * C + c] = a;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i == next) ahead[i] += (a > pt[i] || (a == pt[i] && c < tgt)) ? 1 : 0;
        ++next;
      }
    }
  }
  if (tgt < 0) return;                               // block-uniform
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < nk && ahead[i]) atomicAdd(&Rank[i], ahead[i]);
  __syncthreads();
  if (tid < nk) {
    if (Rank[tid] < 1) atomicAdd(&counters[2 * tid], 1ull);
    if (Rank[tid] < 5) atomicAdd(&counters[2 * tid + 1], 1ull);
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline int kc_shape_check(int64_t n, int64_t M, int D, int kmax) {
  if (n < 1 || M < 1 || M > 0x7FFFFFFFll || D < 64 || D % 64 || kmax < 1 || kmax > KC_KMAX) return OCTIC_ESHAPE;
  if (M < kmax) return OCTIC_ESHAPE;             // fewer keys than neighbours asked for
  if ((n + KC_QT - 1) / KC_QT > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  return OCTIC_OK;
}
inline int kc_ktiles(int64_t M) { return (int)((M + KC_KT - 1) / KC_KT); }
// the key axis is split only when the query tiles alone leave CUs idle, and never below KC_MIN_TILES key tiles a split
inline int kc_plan_splits(int64_t n, int64_t M) {
  const int64_t qtiles = (n + KC_QT - 1) / KC_QT;
  const int cus = device_cus();
  if (qtiles >= cus) return 1;
  int64_t s = (cus + qtiles - 1) / qtiles;
  const int64_t most = kc_ktiles(M) / KC_MIN_TILES;
  if (s > most) s = most;
  if (s > KC_MAX_SPLITS) s = KC_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}
// what a requested split count becomes: whole key tiles per split, no empty split
inline void kc_resolve(int64_t n, int64_t M, int requested, int* splits, int* tiles_per_split) {
  const int ktiles = kc_ktiles(M);
  int s = requested > 0 ? requested : kc_plan_splits(n, M);
  if (s > ktiles) s = ktiles;
  const int tps = (ktiles + s - 1) / s;
  *tiles_per_split = tps;
  *splits = (ktiles + tps - 1) / tps;
}
inline int64_t kc_align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_knn_topk_plan(int64_t n, int64_t M, int D, int kmax, int* out) {
  if (!out) return OCTIC_ENULL;
  if (int e = kc_shape_check(n, M, D, kmax)) return e;
  int splits, tps;
  kc_resolve(n, M, 0, &splits, &tps);
  out[0] = splits;
  out[1] = KC_QT;
  out[2] = KC_KT;
  out[3] = splits > 1 ? 1 : 0;                   // workspace class: 0 = none read, 1 = the partial lists of the splits
  return OCTIC_OK;
}

int64_t octic_knn_topk_workspace_bytes(int64_t n, int64_t M, int D, int kmax, int splits) {
  if (int e = kc_shape_check(n, M, D, kmax)) return e;
  if (splits < 0 || splits > KC_MAX_SPLITS) return OCTIC_ESHAPE;
  int s, tps;
  kc_resolve(n, M, splits, &s, &tps);
  if (s == 1) return 256;
  return 2 * kc_align256(4ll * s * n * kmax);
}

int octic_knn_topk(const float* Q, int64_t ldq, int64_t n, const float* K, int64_t ldk, int64_t M, int D, int kmax, int splits,
                   int32_t* idx, float* sim, int64_t ldo, void* workspace, void* stream) {
  if (!Q || !K || !idx || !sim) return OCTIC_ENULL;
  if (int e = kc_shape_check(n, M, D, kmax)) return e;
  if (splits < 0 || splits > KC_MAX_SPLITS || ldq < D || ldk < D || ldo < kmax) return OCTIC_ESHAPE;
  if ((((uintptr_t)Q) & 15) || (((uintptr_t)K) & 15) || (ldq & 3) || (ldk & 3)) return OCTIC_EALIGN;
  if ((((uintptr_t)idx) & 3) || (((uintptr_t)sim) & 3)) return OCTIC_EALIGN;
  int s, tps;
  kc_resolve(n, M, splits, &s, &tps);
  if (s > 1 && !workspace) return OCTIC_ENULL;
  if (s > 1 && (((uintptr_t)workspace) & 255)) return OCTIC_EALIGN;
  int* ki = idx;
  float* kd = sim;
  int64_t kld = ldo, stride = 0;
  if (s > 1) {
    const int64_t part = kc_align256(4ll * s * n * kmax);
    ki = (int*)workspace;
    kd = (float*)((char*)workspace + part);
    kld = kmax;
    stride = n * kmax;
  }
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + KC_QT - 1) / KC_QT), (unsigned)s);
  knn_topk_kernel<<<grid, 256, 0, st>>>(Q, ldq, n, K, ldk, (int)M, D, kmax, tps, ki, kd, kld, stride);
  if (s > 1) knn_topk_merge_kernel<<<dim3((unsigned)((n + 3) / 4)), 256, 0, st>>>(ki, kd, idx, sim, n, kmax, s, ldo);
  return launch_status();
}

int octic_knn_vote(const float* sim, const int32_t* idx, int64_t ldi, int64_t n, int kmax, const int64_t* labels, int64_t M,
                   int C, float inv_T, const int* ks, int nk, float* probas, const int64_t* targets, int64_t* counters,
                   void* stream) {
  if (!sim || !idx || !labels || !ks || !probas) return OCTIC_ENULL;
  if (targets && !counters) return OCTIC_ENULL;
  if (n < 1 || n > 0x7FFFFFFFll || M < 1 || kmax < 1 || kmax > KC_KMAX || ldi < kmax || C < 5 || nk < 1 || nk > 8)
    return OCTIC_ESHAPE;
  if (!(inv_T > 0.f) || inv_T > 3.0e38f) return OCTIC_ESHAPE;     // a positive, finite 1 / T
  KcVoteKs k;
  for (int i = 0; i < 8; ++i) k.k[i] = i < nk ? ks[i] : 0;
  for (int i = 0; i < nk; ++i)
    if (k.k[i] < 1 || k.k[i] > kmax || (i && k.k[i] <= k.k[i - 1])) return OCTIC_ESHAPE;   // strictly ascending, 1 .. kmax
  if ((((uintptr_t)sim) & 3) || (((uintptr_t)idx) & 3) || (((uintptr_t)probas) & 3) || (((uintptr_t)labels) & 7) ||
      (((uintptr_t)targets) & 7) || (((uintptr_t)counters) & 7))
    return OCTIC_EALIGN;
  knn_vote_kernel<<<dim3((unsigned)n), 256, 0, (hipStream_t)stream>>>(sim, idx, ldi, n, kmax, labels, M, C, inv_T, k, nk, probas,
                                                                      targets, (unsigned long long*)counters);
  return launch_status();
}

}  // extern "C"
