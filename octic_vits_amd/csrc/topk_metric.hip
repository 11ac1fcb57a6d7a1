// Top-k accuracy counters of the evaluations (dinov2/eval/metrics.py: MulticlassAccuracy(average = micro | macro | none, top_k)
// and ImageNetReaLAccuracy; the class mapping of linear.py's LinearPostprocessor) on score rows scores[g, r, :] that are
// already on the device: the linear probe's [classifiers, B, C] logits and the k-NN vote's [nk, n, C] probas, without a copy.
// Two launches per update for all groups:
//   1. topk_rank_kernel  : workgroup = ONE WAVE = one (group, row).  The candidates s_j = scores[g, r, map[j]] (map NULL: j) are
//                          read once, every lane holding a strided share (16 bytes a load on the unmapped, aligned path, four
//                          loads in flight), and counted against all A targets of the row in registers; the counts of the 64
//                          lanes meet in a butterfly.  rank[g, r, a] = candidates in front of target a, Cm for an undefined one.
//   2. topk_count_any_kernel / topk_count_class_kernel : thread = one (group, row); a wave's rows are counted with ballots
//                          ("any": one 64-bit integer atomic per wave and counter) or per row ("class": the target's own
//                          counters).  Integer atomics only: the counters do not depend on the launch shape or on how the
//                          rows were split into calls.
// No LDS, no barrier, no floating-point atomics.  A NaN score counts as -inf (as in knn_cls.hip).
#include "octic_common.hpp"

namespace octic {
namespace {

struct TopkKs { int k[8]; };

__device__ __forceinline__ float tm_key(float v) { return v == v ? v : -INFINITY; }

// ORDER 0: j comes before t iff s_j > s_t (probe_ce_kernel's rule).  ORDER 1: ... or s_j == s_t and j < t (knn_vote_kernel's).
template <int ORDER>
__device__ __forceinline__ int tm_before(float sj, int j, float st, int t) {
  if (ORDER == 0) return sj > st ? 1 : 0;
  return (sj > st || (sj == st && j < t)) ? 1 : 0;
}

template <int AMAX, int ORDER>
__global__ __launch_bounds__(64) void topk_rank_kernel(const float* __restrict__ scores, int64_t ld_g, int64_t ld_r, int64_t rows,
                                                       int64_t n, int C, const int* __restrict__ class_map, int Cm,
                                                       const int64_t* __restrict__ targets, int A, int* __restrict__ rank) {
  const int lane = threadIdx.x;
  // a mapped column outside [0, C) is the caller's error (the Python side validates the mapping); it reads nothing and counts as -inf
  auto mapped = [&](const float* x, int j) {
    const unsigned m = (unsigned)class_map[j];
    return m < (unsigned)C ? x[m] : -INFINITY;
  };
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t g = row / n, r = row - g * n;
    const float* x = scores + g * ld_g + r * ld_r;
    // lane a < A owns target a: its candidate index and score (an undefined one stands at +inf, in front of everything)
    int my_t = -1;
    float my_s = INFINITY;
    if (lane < A) {
      const int64_t t64 = targets[r * A + lane];
      if (t64 >= 0 && t64 < Cm) {
        my_t = (int)t64;
        my_s = tm_key(class_map ? mapped(x, my_t) : x[my_t]);
      }
    }
    float st[AMAX];
    int tt[AMAX], cnt[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      st[a] = __shfl(my_s, a);
      tt[a] = __shfl(my_t, a);
      cnt[a] = 0;
    }
    auto take = [&](float v, int j) {
      v = tm_key(v);
#pragma unroll
      for (int a = 0; a < AMAX; ++a) cnt[a] += tm_before<ORDER>(v, j, st[a], tt[a]);
    };
    int j0 = 0;
    if (!class_map && ((((uintptr_t)x) & 15) == 0)) {          // wave-uniform: 16-byte loads, four in flight per lane
      const int nq = Cm >> 2;
      int q = lane;
      for (; q + 192 < nq; q += 256) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(x + 4 * (q + 64 * u));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) take(v[u][e], 4 * (q + 64 * u) + e);
      }
      for (; q < nq; q += 64) {
        const f32x4 v = *(const f32x4*)(x + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) take(v[e], 4 * q + e);
      }
      j0 = nq << 2;
    }
    for (int j = j0 + lane; j < Cm; j += 64) take(class_map ? mapped(x, j) : x[j], j);
    int mine = 0;
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      int c = cnt[a];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if (lane == a) mine = c;
    }
    if (lane < A) rank[row * A + lane] = my_t >= 0 ? mine : Cm;
  }
}

// thread = one row of one group.  A row is defined when some target of it is (rank < Cm), and hits k when its best rank < k.
__global__ __launch_bounds__(256) void topk_count_any_kernel(const int* __restrict__ rank, int G, int64_t n, int A, int Cm, TopkKs ks,
                                                             int nk, unsigned long long* __restrict__ counters) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    int best = Cm;
    if (r < n) {
      const int* rk = rank + ((int64_t)g * n + r) * A;
      for (int a = 0; a < A; ++a) best = min(best, rk[a]);
    }
    unsigned long long* out = counters + (int64_t)g * (1 + nk);
    const int defined = __popcll(__ballot(best < Cm));
    if (lane == 0 && defined) atomicAdd(out, (unsigned long long)defined);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < nk) {
        const int hits = __popcll(__ballot(best < Cm && best < ks.k[i]));
        if (lane == 0 && hits) atomicAdd(out + 1 + i, (unsigned long long)hits);
      }
    }
  }
}

// A == 1.  counters [G, Cm, 1 + nk]: the support of the row's class and its hits.
__global__ __launch_bounds__(256) void topk_count_class_kernel(const int* __restrict__ rank, int G, int64_t n, int Cm,
                                                               const int64_t* __restrict__ targets, TopkKs ks, int nk,
                                                               unsigned long long* __restrict__ counters) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int64_t t = targets[r];
  if (t < 0 || t >= Cm) return;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const int rk = rank[(int64_t)g * n + r];
    unsigned long long* out = counters + ((int64_t)g * Cm + t) * (1 + nk);
    atomicAdd(out, 1ull);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nk && rk < ks.k[i]) atomicAdd(out + 1 + i, 1ull);
  }
}

template <int AMAX>
void rank_launch(int order, unsigned grid, hipStream_t st, const float* scores, int64_t ld_g, int64_t ld_r, int64_t rows, int64_t n,
                 int C, const int* class_map, int Cm, const int64_t* targets, int A, int* rank) {
  if (order == 0)
    topk_rank_kernel<AMAX, 0><<<dim3(grid), 64, 0, st>>>(scores, ld_g, ld_r, rows, n, C, class_map, Cm, targets, A, rank);
  else
    topk_rank_kernel<AMAX, 1><<<dim3(grid), 64, 0, st>>>(scores, ld_g, ld_r, rows, n, C, class_map, Cm, targets, A, rank);
}

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_topk_rank(const float* scores, int64_t ld_g, int64_t ld_r, int64_t G, int64_t n, int64_t C, const int32_t* class_map,
                    int64_t Cm, const int64_t* targets, int A, int order, int32_t* rank, void* stream) {
  if (!scores || !targets || !rank) return OCTIC_ENULL;
  if (G < 1 || n < 1 || C < 1 || C > 0x7FFFFFFFll || Cm < 1 || Cm > 0x7FFFFFFFll || A < 1 || A > OCTIC_TOPK_MAX_TARGETS)
    return OCTIC_ESHAPE;
  if (G > 0x7FFFFFFFll || n > 0x7FFFFFFFll || G * n > 0x7FFFFFFFll || G * n * A > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if (!class_map && Cm != C) return OCTIC_ESHAPE;
  if (order != 0 && order != 1) return OCTIC_ESHAPE;
  if (ld_g < 0 || ld_r < 0 || (n > 1 && ld_r < C) || (G > 1 && ld_g < C)) return OCTIC_ESHAPE;
  if ((((uintptr_t)scores) & 3) || (((uintptr_t)class_map) & 3) || (((uintptr_t)rank) & 3) || (((uintptr_t)targets) & 7))
    return OCTIC_EALIGN;
  const int64_t rows = G * n;
  const unsigned grid = (unsigned)(rows < (1 << 20) ? rows : (1 << 20));
  const hipStream_t st = (hipStream_t)stream;
  if (A == 1) rank_launch<1>(order, grid, st, scores, ld_g, ld_r, rows, n, (int)C, class_map, (int)Cm, targets, A, rank);
  else if (A <= 4) rank_launch<4>(order, grid, st, scores, ld_g, ld_r, rows, n, (int)C, class_map, (int)Cm, targets, A, rank);
  else if (A <= 16) rank_launch<16>(order, grid, st, scores, ld_g, ld_r, rows, n, (int)C, class_map, (int)Cm, targets, A, rank);
  else rank_launch<32>(order, grid, st, scores, ld_g, ld_r, rows, n, (int)C, class_map, (int)Cm, targets, A, rank);
  return launch_status();
}

int octic_topk_count(const int32_t* rank, int64_t G, int64_t n, int A, int64_t Cm, const int64_t* targets, int mode, const int* ks,
                     int nk, int64_t* counters, void* stream) {
  if (!rank || !ks || !counters) return OCTIC_ENULL;
  if (mode != OCTIC_TOPK_ANY && mode != OCTIC_TOPK_CLASS) return OCTIC_ESHAPE;
  if (mode == OCTIC_TOPK_CLASS && !targets) return OCTIC_ENULL;
  if (G < 1 || n < 1 || Cm < 1 || Cm > 0x7FFFFFFFll || A < 1 || A > OCTIC_TOPK_MAX_TARGETS || nk < 1 || nk > 8) return OCTIC_ESHAPE;
  if (G > 0x7FFFFFFFll || n > 0x7FFFFFFFll || G * n > 0x7FFFFFFFll || G * n * A > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if (mode == OCTIC_TOPK_CLASS && A != 1) return OCTIC_ESHAPE;
  TopkKs k;
  for (int i = 0; i < 8; ++i) k.k[i] = i < nk ? ks[i] : 0;
  for (int i = 0; i < nk; ++i)
    if (k.k[i] < 1 || (i && k.k[i] <= k.k[i - 1])) return OCTIC_ESHAPE;       // ascending values >= 1
  if ((((uintptr_t)rank) & 3) || (((uintptr_t)targets) & 7) || (((uintptr_t)counters) & 7)) return OCTIC_EALIGN;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(G < 65535 ? G : 65535));
  const hipStream_t st = (hipStream_t)stream;
  if (mode == OCTIC_TOPK_ANY)
    topk_count_any_kernel<<<grid, 256, 0, st>>>(rank, (int)G, n, A, (int)Cm, k, nk, (unsigned long long*)counters);
  else
    topk_count_class_kernel<<<grid, 256, 0, st>>>(rank, (int)G, n, (int)Cm, targets, k, nk, (unsigned long long*)counters);
  return launch_status();
}

}  // extern "C"
