// The streaming top-k core of the two k-NN searches: seg_knn_kernel (segknn.hip: L2 / cosine distance, ascending, up to 32
// neighbours, query tile 128) and knn_topk_kernel (knn_cls.hip: inner product, descending, up to 256, query tile 64).
// A workgroup of 4 waves owns 64 BT query rows x one contiguous range of key tiles (KNN_KT keys each).  Both tiles go through LDS
// in chunks of 32 channels; the dot products run on the exact-f32 MFMA (16x16x4), one accumulator chain over all of D per pair.
// After a key tile the caller's epilogue turns the accumulators into ordering keys, compares each with the query's current
// kmax-th best (one LDS word per query and list) and inserts the survivors into the query's sorted list in LDS.  When the key
// axis is split over workgroups (few queries), every split writes its own sorted lists and knn_merge_kernel merges them.
// Everything here is parameterised at compile time only (BT, the order, the planner's constants): nothing branches at run time
// on which search called it.  The sorted inserts are NOT here: lane = entry (segknn.hip) and lane = four entries (knn_cls.hip)
// are different algorithms that share only the order.
// TOTAL ORDER (KnnOrder): (ordering key, key row index) - the better key first (the smaller distance, the larger similarity),
// on equal keys the lower index first.  torch.topk leaves ties unspecified; this rule is ours.  A key that is NaN counts as the
// worst value (+inf ascending, -inf descending; the rule is applied where the ordering key is formed), and a key row at the
// worst value is never listed: a query with fewer than kmax listable keys ends on (worst, -1) entries.  Keys stream in ascending
// index order inside a split, so a key that EQUALS the current kmax-th best loses to it by the index rule: the filter
// (KnnOrder::beats) is strict.
// DETERMINISM: the dot product of a pair is one fmaf chain over the channels in an order that depends on D alone (within each
// 16 channels: e, 4 + e, 8 + e, 12 + e for e = 0 .. 3), and the ordering key is a contraction-free expression of that dot (and,
// for the distances, the two row norms).  It does not depend on the pair's place in a tile, on the split or on the batch, so the
// merged lists are the global answer and results are bitwise equal for every split count, every query order and every
// batching.  No floating-point atomics.  Every row and element offset is 64-bit.
// BF16 OPERANDS (knn_stream_bf16, seg_knn_kernel only): rows already rounded to bf16 go through LDS in chunks of 64 channels
// (the same 128 bytes a row as 32 f32 channels, so the same image and the same row stride) and the dot products run on
// mfma_f32_16x16x32_bf16 with f32 accumulation: per pair ONE accumulator chain over the D / 32 k-steps in ascending channel
// order, step s holding channels 32 s .. 32 s + 31.  What the instruction does inside a step is a function of its 32 operand
// pairs alone, so the contract above holds for this stream as it stands: a dot depends on the two rows and on D only.
#pragma once
#include "octic_common.hpp"

namespace octic {

constexpr int KNN_KT = 128;     // keys per tile
constexpr int KNN_LD = 36;      // 32 k + 4: as SEG_FW_LD of segeval.hip
constexpr int KNN_LD16 = 72;    // the same 144-byte row as bf16: 64 k + 8
constexpr int KNN_MAX_SPLITS = 64;

__device__ __forceinline__ f32x4 knn_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <bool ASCENDING>
struct KnnOrder {
  static __device__ __forceinline__ float worst() { return ASCENDING ? INFINITY : -INFINITY; }
  static __device__ __forceinline__ bool beats(float a, float bar) { return ASCENDING ? a < bar : a > bar; }   // strictly
  static __device__ __forceinline__ bool before(float a, int ia, float b, int ib) {   // (a, ia) strictly precedes (b, ib)
    return beats(a, b) || (a == b && (unsigned)ia < (unsigned)ib);
  }
};

struct KnnNoTileMeta {          // the per-key-tile hook of knn_stream, left empty
  __device__ __forceinline__ void load(int) {}
  __device__ __forceinline__ void store() {}
};

// Streams the key tiles of split blockIdx.y past the 64 BT query rows of tile blockIdx.x.  Wave w owns query rows 16 BT w ..
// 16 BT (w + 1) - 1 of the tile (BT x 8 tiles of 16 x 16): accumulator element e of tile (bt, ct) in lane (r, q) is
// dot(query 16 BT w + 16 bt + 4 q + e, key 16 ct + r).  After key tile t, epilogue(t, acc) runs; the next tile's first chunk is
// already in flight under it.  meta.load(first key row of the tile) runs with the tile's first prefetch and meta.store() with its
// first staging, before the barrier that the epilogue's reads are behind.
template <int BT, typename Meta, typename Epilogue>
__device__ __forceinline__ void knn_stream(const float* __restrict__ Q, int64_t ldq, int64_t n, const float* __restrict__ K,
                                           int64_t ldk, int M, int D, int tiles_per_split, float* Qs, float* Ks, Meta& meta,
                                           Epilogue&& epilogue) {
  constexpr int QP = 2 * BT;                        // staging: 32 rows x 8 float4 per pass, QP passes for Q, 4 for K
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  const int64_t q0 = (int64_t)blockIdx.x * (64 * BT);
  const int ktiles = (int)(((int64_t)M + KNN_KT - 1) / KNN_KT);
  const int t0 = blockIdx.y * tiles_per_split;
  const int t1 = t0 + tiles_per_split < ktiles ? t0 + tiles_per_split : ktiles;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  f32x4 qr[QP], kr[4];
  auto fetch = [&](int t, int k0) {
    const int kb = t * KNN_KT;
#pragma unroll
    for (int i = 0; i < QP; ++i) {
      const int64_t qrow = q0 + srow + 32 * i;
      qr[i] = qrow < n ? *(const f32x4*)(Q + qrow * ldq + k0 + sc4) : zero;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned krow = (unsigned)kb + srow + 32 * i;     // a 32-bit bound test (kb + 127 < 2^31 + 127): the 64-bit one
                                                              // costs scalar registers that spill into the chunk loop
      kr[i] = krow < (unsigned)M ? *(const f32x4*)(K + (int64_t)krow * ldk + k0 + sc4) : zero;
    }
    if (k0 == 0) meta.load(kb);
  };

  if (t0 < t1) fetch(t0, 0);
  for (int t = t0; t < t1; ++t) {
    f32x4 acc[BT][8];
#pragma unroll
    for (int i = 0; i < BT; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = zero;
    for (int k0 = 0; k0 < D; k0 += 32) {
      __syncthreads();                       // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int i = 0; i < QP; ++i) *(f32x4*)(Qs + (srow + 32 * i) * KNN_LD + sc4) = qr[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(Ks + (srow + 32 * i) * KNN_LD + sc4) = kr[i];
      if (k0 == 0) meta.store();
      __syncthreads();
      if (k0 + 32 < D) fetch(t, k0 + 32);    // in flight under the products
      else if (t + 1 < t1) fetch(t + 1, 0);  // ... and under the epilogue
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x4 a4[BT];
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) a4[bt] = *(const f32x4*)(Qs + (16 * BT * w + 16 * bt + r) * KNN_LD + 16 * j + 4 * q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x4 b4[4];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) b4[ct] = *(const f32x4*)(Ks + (16 * (ct + 4 * h) + r) * KNN_LD + 16 * j + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int bt = 0; bt < BT; ++bt)
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) acc[bt][ct + 4 * h] = knn_mfma16(a4[bt][e], b4[ct][e], acc[bt][ct + 4 * h]);
        }
      }
    }
    epilogue(t, acc);
  }
}

// knn_stream on rows of bf16: the same ownership, prefetch, barriers and accumulator meaning, 64 channels a chunk.  A fragment
// is one 16-byte LDS read per lane: lane (r, q) holds channels 8 q .. 8 q + 7 of row r of the 32-channel k-step, for the query
// tile (the A operand) and for the key tile (B) alike; the C / D mapping of the 16x16x32 form is that of the 16x16x4 form.
// The row stride of 144 bytes puts the 16 rows of a read on 16 different 4-bank groups, as in the f32 stream.
template <int BT, typename Meta, typename Epilogue>
__device__ __forceinline__ void knn_stream_bf16(const bf16* __restrict__ Q, int64_t ldq, int64_t n, const bf16* __restrict__ K,
                                                int64_t ldk, int M, int D, int tiles_per_split, bf16* Qs, bf16* Ks, Meta& meta,
                                                Epilogue&& epilogue) {
  constexpr int QP = 2 * BT;                        // staging: 32 rows x 8 x 16 bytes per pass, QP passes for Q, 4 for K
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int srow = tid >> 3, sc8 = (tid & 7) * 8;
  const int64_t q0 = (int64_t)blockIdx.x * (64 * BT);
  const int ktiles = (int)(((int64_t)M + KNN_KT - 1) / KNN_KT);
  const int t0 = blockIdx.y * tiles_per_split;
  const int t1 = t0 + tiles_per_split < ktiles ? t0 + tiles_per_split : ktiles;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const u32x4 zero16 = {0u, 0u, 0u, 0u};

  u32x4 qr[QP], kr[4];
  auto fetch = [&](int t, int k0) {
    const int kb = t * KNN_KT;
#pragma unroll
    for (int i = 0; i < QP; ++i) {
      const int64_t qrow = q0 + srow + 32 * i;
      qr[i] = qrow < n ? *(const u32x4*)(Q + qrow * ldq + k0 + sc8) : zero16;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned krow = (unsigned)kb + srow + 32 * i;     // a 32-bit bound test, as in knn_stream
      kr[i] = krow < (unsigned)M ? *(const u32x4*)(K + (int64_t)krow * ldk + k0 + sc8) : zero16;
    }
    if (k0 == 0) meta.load(kb);
  };

  if (t0 < t1) fetch(t0, 0);
  for (int t = t0; t < t1; ++t) {
    f32x4 acc[BT][8];
#pragma unroll
    for (int i = 0; i < BT; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = zero;
    for (int k0 = 0; k0 < D; k0 += 64) {
      __syncthreads();                       // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int i = 0; i < QP; ++i) *(u32x4*)(Qs + (srow + 32 * i) * KNN_LD16 + sc8) = qr[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) *(u32x4*)(Ks + (srow + 32 * i) * KNN_LD16 + sc8) = kr[i];
      if (k0 == 0) meta.store();
      __syncthreads();
      if (k0 + 64 < D) fetch(t, k0 + 64);    // in flight under the products
      else if (t + 1 < t1) fetch(t + 1, 0);  // ... and under the epilogue
#pragma unroll
      for (int j = 0; j < 2; ++j) {          // the two k-steps of the chunk, in channel order
        bf16x8 a8[BT];
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) a8[bt] = *(const bf16x8*)(Qs + (16 * BT * w + 16 * bt + r) * KNN_LD16 + 32 * j + 8 * q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          bf16x8 b8[4];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) b8[ct] = *(const bf16x8*)(Ks + (16 * (ct + 4 * h) + r) * KNN_LD16 + 32 * j + 8 * q);
#pragma unroll
          for (int bt = 0; bt < BT; ++bt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
              acc[bt][ct + 4 * h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8[bt], b8[ct], acc[bt][ct + 4 * h], 0, 0, 0);
        }
      }
    }
    epilogue(t, acc);
  }
}

// The wave's 16 BT lists of each of NL list sets, lane = entry modulo 64.  Ld / Li: [NL][64 BT][CAP] in LDS.
template <int NL, int BT, int CAP>
__device__ __forceinline__ void knn_write_lists(const float* Ld, const int* Li, int64_t n, int kmax, int* const* idx,
                                                float* const* dist, int64_t ldo, int64_t split_stride) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __builtin_amdgcn_wave_barrier();
  const int64_t sp = (int64_t)blockIdx.y * split_stride;
  for (int i = 0; i < 16 * BT; ++i) {
    const int rowl = 16 * BT * w + i;
    const int64_t row = (int64_t)blockIdx.x * (64 * BT) + rowl;
    if (row >= n) break;
#pragma unroll
    for (int e0 = 0; e0 < CAP; e0 += 64) {          // passes fixed by the capacity: a run-time loop over kmax costs the stream
      const int e = e0 + lane;                      // loop scalar registers (measured: spill moves in every chunk)
      if (e < kmax) {
#pragma unroll
        for (int m = 0; m < NL; ++m) {
          idx[m][sp + row * ldo + e] = Li[(m * 64 * BT + rowl) * CAP + e];
          dist[m][sp + row * ldo + e] = Ld[(m * 64 * BT + rowl) * CAP + e];
        }
      }
    }
  }
}

// one wave per (query, list set): lane s walks the sorted list of split s; kmax times the best head over the lanes is taken
struct KnnMergeArgs {
  const int* pidx[2];
  const float* pdist[2];
  int* idx[2];
  float* dist[2];
};
template <typename ORD>
__global__ __launch_bounds__(256) void knn_merge_kernel(KnnMergeArgs a, int64_t n, int kmax, int splits, int64_t ldo, int nl) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= n * nl) return;                    // wave-uniform
  const int m = (int)(item / n);
  const int64_t row = item - (int64_t)m * n;
  const int* pi = a.pidx[m] + ((int64_t)lane * n + row) * kmax;
  const float* pd = a.pdist[m] + ((int64_t)lane * n + row) * kmax;
  int* out_i = a.idx[m] + row * ldo;             // read once: a.idx[m] inside the loop is a load from the arguments per entry
  float* out_d = a.dist[m] + row * ldo;
  int p = 0;
  for (int j = 0; j < kmax; ++j) {
    const bool has = lane < splits && p < kmax;
    float d = has ? pd[p] : ORD::worst();
    int i = has ? pi[p] : -1;
    const float hd = d;
    const int hi = i;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float od = __shfl_xor(d, o);
      const int oi = __shfl_xor(i, o);
      if (ORD::before(od, oi, d, i)) { d = od; i = oi; }
    }
    if (has && hi == i && hd == d && i >= 0) ++p;   // a key row lives in exactly one split: one lane advances
    if (lane == 0) {
      out_i[j] = i;
      out_d[j] = d;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
// QT: query rows per workgroup.  MIN_TILES: an automatic split never gets fewer key tiles (its lists warm up on its first
// keys).  KMAX: the list capacity.
template <int QT, int MIN_TILES, int KMAX>
struct KnnPlanner {
  static int shape_check(int64_t n, int64_t M, int D, int kmax) {
    if (n < 1 || M < 1 || M > 0x7FFFFFFFll || D < 64 || D % 64 || kmax < 1 || kmax > KMAX) return OCTIC_ESHAPE;
    if (M < kmax) return OCTIC_ESHAPE;             // fewer keys than neighbours asked for
    if ((n + QT - 1) / QT > 0x7FFFFFFFll) return OCTIC_ESHAPE;
    return OCTIC_OK;
  }
  static int ktiles(int64_t M) { return (int)((M + KNN_KT - 1) / KNN_KT); }
  // the key axis is split only when the query tiles alone leave CUs idle
  static int plan_splits(int64_t n, int64_t M) {
    const int64_t qtiles = (n + QT - 1) / QT;
    const int cus = device_cus();
    if (qtiles >= cus) return 1;
    int64_t s = (cus + qtiles - 1) / qtiles;
    const int64_t most = ktiles(M) / MIN_TILES;
    if (s > most) s = most;
    if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
  }
  // what a requested split count becomes: whole key tiles per split, no empty split
  static void resolve(int64_t n, int64_t M, int requested, int* splits, int* tiles_per_split) {
    const int kt = ktiles(M);
    int s = requested > 0 ? requested : plan_splits(n, M);
    if (s > kt) s = kt;
    const int tps = (kt + s - 1) / s;
    *tiles_per_split = tps;
    *splits = (kt + tps - 1) / tps;
  }
  static int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
  static int64_t part_bytes(int64_t n, int kmax, int splits) { return align256(4ll * splits * n * kmax); }   // one array of partial lists

  // the answers of the two C entries that describe a shape already checked
  static void plan(int64_t n, int64_t M, int* out) {
    int splits, tps;
    resolve(n, M, 0, &splits, &tps);
    out[0] = splits;
    out[1] = QT;
    out[2] = KNN_KT;
    out[3] = splits > 1 ? 1 : 0;                   // workspace class: 0 = none read, 1 = the partial lists of the splits
  }
  static int64_t workspace_bytes(int64_t n, int64_t M, int kmax, int nl, int splits) {
    if (splits < 0 || splits > KNN_MAX_SPLITS) return OCTIC_ESHAPE;
    int s, tps;
    resolve(n, M, splits, &s, &tps);
    return s == 1 ? 256 : 2 * nl * part_bytes(n, kmax, s);
  }

  // The launch sequence: stream(grid, tiles_per_split, idx[2], dist[2], ld, split_stride) launches the caller's stream kernel
  // into the nl outputs or, with splits, into the partial lists carved from the workspace, which knn_merge_kernel<ORD> then
  // merges into the outputs.
  template <typename ORD, typename Stream>
  static int run(int64_t n, int64_t M, int kmax, int requested, int nl, int* const* out_i, float* const* out_d, int64_t ldo,
                 void* workspace, hipStream_t st, Stream&& stream) {
    int s, tps;
    resolve(n, M, requested, &s, &tps);
    if (s > 1 && !workspace) return OCTIC_ENULL;
    if (s > 1 && (((uintptr_t)workspace) & 255)) return OCTIC_EALIGN;
    int* ki[2];
    float* kd[2];
    KnnMergeArgs a;
    const int64_t part = part_bytes(n, kmax, s);
    for (int m = 0; m < 2; ++m) {
      const int l = m < nl ? m : 0;
      a.idx[m] = out_i[l];
      a.dist[m] = out_d[l];
      a.pidx[m] = ki[m] = s > 1 ? (int*)((char*)workspace + (2 * l) * part) : out_i[l];
      a.pdist[m] = kd[m] = s > 1 ? (float*)((char*)workspace + (2 * l + 1) * part) : out_d[l];
    }
    stream(dim3((unsigned)((n + QT - 1) / QT), (unsigned)s), tps, ki, kd, s > 1 ? (int64_t)kmax : ldo, s > 1 ? n * kmax : 0);
    if (s > 1) knn_merge_kernel<ORD><<<dim3((unsigned)((n * nl + 3) / 4)), 256, 0, st>>>(a, n, kmax, s, ldo, nl);
    return launch_status();
  }
};

}  // namespace octic
