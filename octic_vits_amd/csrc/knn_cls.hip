// The k-NN classification evaluation (dinov2/eval/knn.py: KnnModule) on resident f32 class-token features: for every query row
// the kmax key rows with the LARGEST inner product, then the temperature-softmax vote over classes and the top-1 / top-5 hits.
// Neither the similarity matrix nor the [batch, kmax, classes] one-hot product reaches memory.
//   1. knn_topk_kernel       : workgroup = 64 query rows x one contiguous range of key tiles (128 keys each), streamed by
//                              knn_stream<1> (knn_common.hpp: the loop it shares with seg_knn_kernel, at half that kernel's
//                              query tile).  After a key tile every accumulator is compared with the query's current kmax-th
//                              best (one LDS word per query); only survivors enter the query's sorted list (LDS, up to 256
//                              entries) by a wave-wide sorted insert, lane = four consecutive entries (one LDS round trip).
//                              64 rows x 256 entries x (f32, int32) are 128 KiB of the CU's 160 KiB: one workgroup per CU.
//   2. knn_merge_kernel      : (knn_common.hpp) when the key axis is split over workgroups (few queries), every split writes its
//                              own sorted list and one wave per query merges them.
//   3. knn_vote_kernel       : workgroup = one query row.  w = softmax(sim * inv_T) over all kmax entries (max-subtracted, the sum
//                              in rank order), then thread = class: the rank-order sum of the weights of its class, written at
//                              every k of the ascending list ks.  With targets, the rank of the target class under (proba
//                              descending, class index ascending) is counted on the way and the hits are added to int64 counters.
// The TOTAL ORDER (similarity descending, then key row index ascending) and the DETERMINISM contract are those of
// knn_common.hpp.  Here a NaN similarity counts as -inf, so it is never listed.  The hit counters are integers.
// Limits: D % 64 == 0, 1 <= kmax <= 256 (OCTIC_KNN_KMAX), kmax <= M < 2^31, 0 <= splits <= 64.
#include "knn_common.hpp"

namespace octic {
namespace {

constexpr int KC_QT = 64;       // query rows per workgroup: one 16-row query tile per wave
constexpr int KC_KMAX = OCTIC_KNN_KMAX;
using KcDesc = KnnOrder<false>;
using KcPlan = KnnPlanner<KC_QT, 8, KC_KMAX>;   // never below 8 key tiles a split: its lists warm up on its first kmax keys
static_assert(KC_KMAX == 256, "knn_topk_kernel: 64 lanes x 4 entries, and the LDS budget is worked out for 256 entries");
typedef __attribute__((ext_vector_type(4))) int kc_i32x4;

// Wave-wide sorted insert of (cs, ci) into the kmax-entry list (ls, li) of one query; lane l holds the four entries 4 l .. 4 l + 3
// (one 16-byte LDS read per array, 64 x 4 = KC_KMAX).  The list is sorted by the total order, so the entries that precede the
// candidate are a prefix: the lanes' counts read 4, .., 4, c, 0, .., 0 and their sum - four ballots - is the insert position.
// The predecessor of a lane's first entry is read with the quad, so an insert is one LDS round trip.  Entries kmax ..
// 4 ceil(kmax / 4) - 1 of the last lane's quad are scratch: never counted, never written out.  A candidate that the list's
// kmax-th entry precedes (the bar rose since the caller's ballot) changes nothing.
__device__ __forceinline__ void kc_insert(float* ls, int* li, float* thr, int kmax, int lane, float cs, int ci) {
  const int e0 = 4 * lane;
  const bool mine = e0 < kmax;
  f32x4 s4 = {KcDesc::worst(), KcDesc::worst(), KcDesc::worst(), KcDesc::worst()};
  kc_i32x4 i4 = {-1, -1, -1, -1};
  float ps = KcDesc::worst();                            // the predecessor of the lane's first entry, read in the same round
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
  for (int j = 0; j < 4; ++j) c += (e0 + j < kmax && KcDesc::before(s4[j], i4[j], cs, ci)) ? 1 : 0;
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

// wave w owns query rows 16 w .. 16 w + 15 of the tile (knn_stream<1>) and therefore their lists
__global__ __launch_bounds__(256) void knn_topk_kernel(const float* __restrict__ Q, int64_t ldq, int64_t n,
                                                       const float* __restrict__ K, int64_t ldk, int M, int D, int kmax,
                                                       int tiles_per_split, int* __restrict__ idx, float* __restrict__ sim,
                                                       int64_t ldo, int64_t split_stride) {
  __shared__ __attribute__((aligned(16))) float Qs[KC_QT * KNN_LD];
  __shared__ __attribute__((aligned(16))) float Ks[KNN_KT * KNN_LD];
  __shared__ __attribute__((aligned(16))) float Ls[KC_QT][KC_KMAX];
  __shared__ __attribute__((aligned(16))) int Li[KC_QT][KC_KMAX];
  __shared__ float Thr[KC_QT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int64_t q0 = (int64_t)blockIdx.x * KC_QT;

  for (int i = tid; i < KC_QT * KC_KMAX; i += 256) {
    (&Ls[0][0])[i] = KcDesc::worst();
    (&Li[0][0])[i] = -1;
  }
  if (tid < KC_QT) Thr[tid] = q0 + tid < n ? KcDesc::worst() : -KcDesc::worst();   // a row past n admits nothing
  __syncthreads();

  KnnNoTileMeta meta;
  // ---- per key tile: the filter, the rare insert
  knn_stream<1>(Q, ldq, n, K, ldk, M, D, tiles_per_split, Qs, Ks, meta, [&](int t, const f32x4 (&acc)[1][8]) {
    const int kb = t * KNN_KT;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rowl = 16 * w + 4 * q + e;
      const float thr = Thr[rowl];
      float s[8];
      bool any = false;
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const float dot = acc[0][ct][e];
        const bool dead = (unsigned)kb + 16 * ct + r >= (unsigned)M;     // 32-bit: kb + 127 < 2^31 + 127
        s[ct] = (dead || dot != dot) ? KcDesc::worst() : dot;
        any |= KcDesc::beats(s[ct], thr);
      }
      if (!__any(any)) continue;             // the common case once the lists are warm
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        unsigned long long bal = __ballot(KcDesc::beats(s[ct], thr));
        while (bal) {                        // wave-uniform
          const int l = __ffsll((long long)bal) - 1;
          bal &= bal - 1;
          const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s[ct]), l));
          const int crow = 16 * w + 4 * (l >> 4) + e;   // (a candidate the row's bar has overtaken since the ballot is refused inside)
          kc_insert(&Ls[crow][0], &Li[crow][0], &Thr[crow], kmax, lane, cs, kb + 16 * ct + (l & 15));
        }
      }
    }
  });

  int* const oi[1] = {idx};
  float* const od[1] = {sim};
  knn_write_lists<1, 1, KC_KMAX>(&Ls[0][0], &Li[0][0], n, kmax, oi, od, ldo, split_stride);
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

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_knn_topk_plan(int64_t n, int64_t M, int D, int kmax, int* out) {
  if (!out) return OCTIC_ENULL;
  if (int e = KcPlan::shape_check(n, M, D, kmax)) return e;
  KcPlan::plan(n, M, out);
  return OCTIC_OK;
}

int64_t octic_knn_topk_workspace_bytes(int64_t n, int64_t M, int D, int kmax, int splits) {
  if (int e = KcPlan::shape_check(n, M, D, kmax)) return e;
  return KcPlan::workspace_bytes(n, M, kmax, 1, splits);
}

int octic_knn_topk(const float* Q, int64_t ldq, int64_t n, const float* K, int64_t ldk, int64_t M, int D, int kmax, int splits,
                   int32_t* idx, float* sim, int64_t ldo, void* workspace, void* stream) {
  if (!Q || !K || !idx || !sim) return OCTIC_ENULL;
  if (int e = KcPlan::shape_check(n, M, D, kmax)) return e;
  if (splits < 0 || splits > KNN_MAX_SPLITS || ldq < D || ldk < D || ldo < kmax) return OCTIC_ESHAPE;
  if ((((uintptr_t)Q) & 15) || (((uintptr_t)K) & 15) || (ldq & 3) || (ldk & 3)) return OCTIC_EALIGN;
  if ((((uintptr_t)idx) & 3) || (((uintptr_t)sim) & 3)) return OCTIC_EALIGN;
  const hipStream_t st = (hipStream_t)stream;
  return KcPlan::run<KcDesc>(n, M, kmax, splits, 1, &idx, &sim, ldo, workspace, st,
                             [&](dim3 grid, int tps, int* const* ki, float* const* kd, int64_t kld, int64_t stride) {
    knn_topk_kernel<<<grid, 256, 0, st>>>(Q, ldq, n, K, ldk, (int)M, D, kmax, tps, ki[0], kd[0], kld, stride);
  });
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
