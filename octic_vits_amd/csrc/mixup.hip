// Device-side Mixup / CutMix and the DeiT-III BCE loss (timm/data/mixup.py as the recipe of experiments/train_deit.py uses it:
// mixup 0.8, cutmix 1.0, --bce-loss; deit/engine.py:47-59).  The host draws the per-sample parameters (octic_vits_amd/mixup.py)
// and uploads them as one DEVICE table of octic_mix_row entries; the three kernels here read nothing else about the draw, so
// one captured launch serves every replay:
//   1. mix_images_kernel : dst[i] = inside sample i's box ? src[partner] : lam src[i] + (1 - lam) src[partner]   (out of place)
//   2. mix_targets_kernel: t = lam onehot(y) + (1 - lam) onehot(y[partner]), optionally (t > 0)                  (mixup_target)
//   3. mix_bce_kernel    : BCEWithLogitsLoss(mean) against those targets without materialising them, value and gradient;
//      mix_bce_finish_kernel: the row sums in row order -> the mean.
//   4. mix_ce_kernel     : the soft-target cross entropy against the NON-binarised targets (deit/main.py:372-378: the loop's
//      criterion without --bce-loss; with the identity table, LabelSmoothingCrossEntropy and plain CE), a row per workgroup.
//   5. cosub_bce_kernel  : the four BCE terms of --cosub (deit/engine.py:56-65) on both passes of a sample at once.
// The first three are streams: (1) reads two images and writes one per sample with 16-byte accesses along W (a scalar twin serves
// W % 4 != 0 and unaligned pointers); (2) and (3) touch rows x num_classes elements once.  f32 arithmetic; the loss terms are
// summed in f64 in a fixed order (thread-strided, wave, waves 0..3, rows in lane-strided order): no atomics, so an eager call
// and a graph replay agree bit for bit.
#include "octic_common.hpp"

namespace octic {

typedef octic_mix_row MixRow;

// the row of sample i, with everything that could index memory made safe: a partner outside the batch means "not mixed"
__device__ __forceinline__ MixRow mix_row(const MixRow* __restrict__ table, int i, int B) {
  MixRow r = table[i];
  if (r.partner < 0 || r.partner >= B || !(r.lam >= 0.f && r.lam < 1.f)) {
    r.partner = i;
    r.lam = 1.f;
    r.cut = 0;
  }
  return r;
}

// ------------------------------------------------------------------------------------------------ 1. images
constexpr int MI_THREADS = 256;
constexpr int MI_UNROLL = 4;

template <int V>
struct Vec;
template <>
struct Vec<4> { typedef f32x4 type; };
template <>
struct Vec<1> { typedef float type; };

template <int V>
__device__ __forceinline__ float lane_of(const typename Vec<V>::type& v, int e);
template <>
__device__ __forceinline__ float lane_of<4>(const f32x4& v, int e) { return v[e]; }
template <>
__device__ __forceinline__ float lane_of<1>(const float& v, int) { return v; }
template <int V>
__device__ __forceinline__ void set_lane(typename Vec<V>::type& v, int e, float x);
template <>
__device__ __forceinline__ void set_lane<4>(f32x4& v, int e, float x) { v[e] = x; }
template <>
__device__ __forceinline__ void set_lane<1>(float& v, int, float x) { v = x; }

// workgroup = MI_UNROLL x 256 consecutive V-wide pieces of ONE sample (V = 4: W % 4 == 0, so a piece never leaves its image
// row).  All loads of a thread are issued before the first select.  n = C H W elements per sample (< 2^31), nv = n / V.
template <int V>
__global__ __launch_bounds__(MI_THREADS) void mix_images_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                const MixRow* __restrict__ table, int B, int H, int W,
                                                                int nv, int blocks_per_sample) {
  typedef typename Vec<V>::type vec;
  const int i = blockIdx.x / blocks_per_sample;
  const int v0 = (blockIdx.x - i * blocks_per_sample) * (MI_THREADS * MI_UNROLL) + threadIdx.x;
  const MixRow r = mix_row(table, i, B);
  const int64_t n = (int64_t)nv * V;
  const vec* s = (const vec*)(src + (int64_t)i * n);
  const vec* p = (const vec*)(src + (int64_t)r.partner * n);
  vec* d = (vec*)(dst + (int64_t)i * n);
  const bool mixed = r.lam != 1.f;
  const bool cut = mixed && r.cut != 0;
  const float lam = r.lam, oml = 1.f - r.lam;
  vec sv[MI_UNROLL], pv[MI_UNROLL];
  int hh[MI_UNROLL], ww[MI_UNROLL];
#pragma unroll
  for (int u = 0; u < MI_UNROLL; ++u) {
    const int v = v0 + u * MI_THREADS;
    if (v < nv) {
      const int e = v * V;                      // element index inside the sample
      const int row = e / W;                    // = c H + h
      hh[u] = row % H;
      ww[u] = e - row * W;
      sv[u] = s[v];
      // the partner is read where it can matter: everywhere for a blend, on the box's rows for a cut
      if (mixed && (!cut || (hh[u] >= r.yl && hh[u] < r.yh))) pv[u] = p[v];
      else pv[u] = sv[u];
    }
  }
#pragma unroll
  for (int u = 0; u < MI_UNROLL; ++u) {
    const int v = v0 + u * MI_THREADS;
    if (v < nv) {
      vec o = sv[u];
      if (cut) {
        const bool in_rows = hh[u] >= r.yl && hh[u] < r.yh;
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (in_rows && ww[u] + e >= r.xl && ww[u] + e < r.xh) set_lane<V>(o, e, lane_of<V>(pv[u], e));
      } else if (mixed) {
#pragma unroll
        for (int e = 0; e < V; ++e)
          set_lane<V>(o, e, __builtin_fmaf(lam, lane_of<V>(sv[u], e), oml * lane_of<V>(pv[u], e)));
      }
      d[v] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ 2. targets
// timm's arithmetic, rounding for rounding: y1 * lam + y2 * (1 - lam) on f32 tensors = rn(rn(y1 lam) + rn(y2 (1 - lam)))
// (contraction off: the compiler would otherwise fuse a product into the sum and drop its rounding)
__device__ __forceinline__ float mixed_target(int j, int la, int lb, float lam, float oml, float on, float off, int binarize) {
#pragma clang fp contract(off)
  const float y1 = j == la ? on : off, y2 = j == lb ? on : off;
  const float a = y1 * lam, b = y2 * oml;
  const float t = a + b;
  return binarize ? (t > 0.f ? 1.f : 0.f) : t;
}

// the two labels of batch row b; a label outside [0, num_classes) becomes -1 and matches no column (an all-`off` row)
__device__ __forceinline__ void mix_labels(const int64_t* __restrict__ labels, const MixRow& r, int b, int nc, int& la, int& lb) {
  const int64_t a = labels[b], c = labels[r.partner];
  la = (a >= 0 && a < nc) ? (int)a : -1;
  lb = (c >= 0 && c < nc) ? (int)c : -1;
}

__global__ __launch_bounds__(256) void mix_targets_kernel(const int64_t* __restrict__ labels, const MixRow* __restrict__ table,
                                                          int B, int row0, int nc, float on, float off, int binarize,
                                                          float* __restrict__ targets) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nc) return;
  const int b = row0 + blockIdx.y;
  const MixRow r = mix_row(table, b, B);
  int la, lb;
  mix_labels(labels, r, b, nc, la, lb);
  targets[(int64_t)blockIdx.y * nc + j] = mixed_target(j, la, lb, r.lam, 1.f - r.lam, on, off, binarize);
}

// ------------------------------------------------------------------------------------------------ 3. BCE with logits
__device__ __forceinline__ double wave_total_f64(double v) {   // butterfly: every lane ends with the same sum, fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ __forceinline__ void store_as(T* p, float v);
template <>
__device__ __forceinline__ void store_as<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void store_as<bf16>(bf16* p, float v) { *p = (bf16)v; }

// one workgroup per logit row.  Per element, with e = exp(-|x|): the loss term max(x, 0) - x t + log1p(e) and
// sigmoid(x) = x >= 0 ? 1 / (1 + e) : e / (1 + e); dlogits = ((sigmoid - t) inv_n) gscale.
template <typename T>
__global__ __launch_bounds__(256) void mix_bce_kernel(const T* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels,
                                                      const MixRow* __restrict__ table, int B, int row0, int nc, float on,
                                                      float off, int binarize, float inv_n, const float* __restrict__ gscale,
                                                      double* __restrict__ rowsum, T* __restrict__ dlogits, int64_t ldd) {
  __shared__ double red[4];
  const int row = blockIdx.x, b = row0 + row;
  const MixRow r = mix_row(table, b, B);
  int la, lb;
  mix_labels(labels, r, b, nc, la, lb);
  const float lam = r.lam, oml = 1.f - r.lam;
  const float g = gscale ? gscale[0] : 1.f;
  const T* x = logits + (int64_t)row * ldl;
  T* d = dlogits ? dlogits + (int64_t)row * ldd : nullptr;
  double acc = 0.0;
  for (int j = threadIdx.x; j < nc; j += 256) {
    const float v = (float)x[j];
    const float t = mixed_target(j, la, lb, lam, oml, on, off, binarize);
    const float e = expf(-fabsf(v));
    if (rowsum) acc += (double)((fmaxf(v, 0.f) - v * t) + log1pf(e));
    if (d) {
      const float sig = (v >= 0.f ? 1.f : e) / (1.f + e);
      store_as<T>(d + j, ((sig - t) * inv_n) * g);
    }
  }
  if (rowsum) {
    acc = wave_total_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) rowsum[row] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// one wave: the row sums in lane-strided order, the wave total, times 1 / (rows num_classes)
__global__ __launch_bounds__(64) void mix_bce_finish_kernel(const double* __restrict__ rowsum, int rows, double inv_n,
                                                            float* __restrict__ loss) {
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 64) s += rowsum[i];
  s = wave_total_f64(s);
  if (threadIdx.x == 0) loss[0] = (float)(s * inv_n);
}

// ------------------------------------------------------------------------------------------------ 4. soft-target cross entropy
// one workgroup per logit row.  Element e of the row belongs to thread (e / V) % 256, slot (e / V) / 256, V = 16 bytes of the
// dtype (4 f32, 8 bf16) - the SAME map whether a piece is moved as one 16-byte access (row start and stride allow it, and the
// piece lies inside the row) or element by element, so the sums below do not depend on alignment or stride.  E > 0: the row
// lives in E registers per thread (num_classes <= 256 E) and is read from memory once; E = 0: every pass re-reads it.
//   pass 1: m = max x                                   (f32; NaN elements are skipped here and poison pass 2 instead)
//   pass 2: se = sum expf(x - m) (a slot's V terms in f32, then f64: thread in slot order, wave, waves 0..3) and sx = sum x (f64)
//   S = sum t and tx = sum t x in f64 from the three values a row's targets take (all but one or two columns share one)
//   loss row = S (m + log se) - tx in f64 (finite for every finite row, whatever the logits' size)
//   pass 3: dlogits = ((S expf(x - m) / se - t) / rows) gscale; an element whose two terms cancel to less than 2^-10 of t (it
//           happens with smoothed targets, a few elements in a million) is recomputed in f64 so that it keeps its leading bits
constexpr int CE_SMALL_E = 8, CE_LARGE_E = 96;    // resident up to 2048 and 24576 classes

template <typename T>
__device__ __forceinline__ void ce_load(const T* __restrict__ x, int e0, int nc, bool vec, float (&v)[16 / sizeof(T)]);
template <>
__device__ __forceinline__ void ce_load<float>(const float* __restrict__ x, int e0, int nc, bool vec, float (&v)[4]) {
  if (vec && e0 + 4 <= nc) {
    const f32x4 q = *(const f32x4*)(x + e0);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = e0 + i < nc ? x[e0 + i] : -INFINITY;
  }
}
template <>
__device__ __forceinline__ void ce_load<bf16>(const bf16* __restrict__ x, int e0, int nc, bool vec, float (&v)[8]) {
  if (vec && e0 + 8 <= nc) {
    const bf16x8 q = *(const bf16x8*)(x + e0);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)q[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = e0 + i < nc ? (float)x[e0 + i] : -INFINITY;
  }
}

template <typename T>
__device__ __forceinline__ void ce_store(T* __restrict__ d, int e0, int nc, bool vec, const float (&v)[16 / sizeof(T)]);
template <>
__device__ __forceinline__ void ce_store<float>(float* __restrict__ d, int e0, int nc, bool vec, const float (&v)[4]) {
  if (vec && e0 + 4 <= nc) {
    *(f32x4*)(d + e0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i < nc) d[e0 + i] = v[i];
  }
}
template <>
__device__ __forceinline__ void ce_store<bf16>(bf16* __restrict__ d, int e0, int nc, bool vec, const float (&v)[8]) {
  if (vec && e0 + 8 <= nc) {
    *(bf16x8*)(d + e0) = bf16x8{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3], (bf16)v[4], (bf16)v[5], (bf16)v[6], (bf16)v[7]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (e0 + i < nc) d[e0 + i] = (bf16)v[i];
  }
}

// the four waves' sums in wave order; every thread ends with the same total
__device__ __forceinline__ double block_total_f64(double v, double* red) {
  v = wave_total_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T, int E>
__global__ __launch_bounds__(256) void mix_ce_kernel(const T* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels,
                                                     const MixRow* __restrict__ table, int B, int row0, int nc, float on, float off,
                                                     float inv_rows, const float* __restrict__ gscale, double* __restrict__ rowsum,
                                                     T* __restrict__ dlogits, int64_t ldd, int vec_l, int vec_d) {
  constexpr int V = 16 / sizeof(T);
  constexpr int NS = E / V;                           // resident slots per thread
  constexpr int UNROLL = NS ? NS : 1;                 // (the slot loops: unrolled over the registers, a plain loop otherwise)
  __shared__ float redm[4];
  __shared__ double red[2][4];
  const int row = blockIdx.x, b = row0 + row, tid = threadIdx.x;
  const MixRow r = mix_row(table, b, B);
  int la, lb;
  mix_labels(labels, r, b, nc, la, lb);
  const float lam = r.lam, oml = 1.f - r.lam;
  const T* x = logits + (int64_t)row * ldl;
  const int slots = NS ? NS : (nc + 256 * V - 1) / (256 * V);
  float xr[NS ? NS : 1][V];
  // a slot's V logits: from the registers when the row is resident, from memory otherwise
  auto slot = [&](int k, int e0, float (&v)[V]) {
    if (NS) {
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = xr[NS ? k : 0][i];
    } else {
      ce_load<T>(x, e0, nc, vec_l, v);
    }
  };

  float m = -INFINITY;
#pragma unroll UNROLL
  for (int k = 0; k < slots; ++k) {
    const int e0 = (k * 256 + tid) * V;
    float v[V];
    if (e0 < nc) {
      ce_load<T>(x, e0, nc, vec_l, v);
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (NS) xr[NS ? k : 0][i] = v[i];
      m = fmaxf(m, v[i]);                             // (elements past the row are -inf)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) redm[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));

  // the targets take three values: t_a at the sample's class, t_b at its partner's (equal when the classes are), t_plain elsewhere
  const float t_plain = mixed_target(-2, la, lb, lam, oml, on, off, 0);
  const float t_a = mixed_target(la, la, lb, lam, oml, on, off, 0), t_b = mixed_target(lb, la, lb, lam, oml, on, off, 0);
  const bool has_a = la >= 0, has_b = lb >= 0 && lb != la;
  const double st = (double)t_plain * (double)(nc - (int)has_a - (int)has_b) + (has_a ? (double)t_a : 0.0) + (has_b ? (double)t_b : 0.0);

  double se = 0.0, sx = 0.0;                          // sum expf(x - m): a slot's V terms in f32, the slots in f64; sum x in f64
#pragma unroll UNROLL
  for (int k = 0; k < slots; ++k) {
    const int e0 = (k * 256 + tid) * V;
    if (e0 < nc) {
      float v[V];
      slot(k, e0, v);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (e0 + i < nc) {
          ps += expf(v[i] - m);
          if (rowsum) sx += (double)v[i];
        }
      se += (double)ps;
    }
  }
  se = block_total_f64(se, red[0]);
  if (rowsum) {
    sx = block_total_f64(sx, red[1]);
    if (tid == 0) {
      // sum t x = t_plain (sum x - x_a - x_b) + t_a x_a + t_b x_b: the one or two labelled logits are read again here
      const double xa = has_a ? (double)(float)x[la] : 0.0, xb = has_b ? (double)(float)x[lb] : 0.0;
      const double tx = (double)t_plain * ((sx - xa) - xb) + ((double)t_a * xa + (double)t_b * xb);
      rowsum[row] = st * ((double)m + log(se)) - tx;
    }
  }
  if (dlogits) {
    T* d = dlogits + (int64_t)row * ldd;
    const float g = gscale ? gscale[0] : 1.f;
    const float inv = (float)(1.0 / se), s = (float)st;
#pragma unroll UNROLL
    for (int k = 0; k < slots; ++k) {
      const int e0 = (k * 256 + tid) * V;
      if (e0 < nc) {
        float v[V];
        slot(k, e0, v);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const int j = e0 + i;
          const float t = j == la ? t_a : j == lb ? t_b : t_plain;   // (a label of -1 matches no column)
          float gr = s * (expf(v[i] - m) * inv) - t;
          // S p and a smoothed target nearly cancel: the f32 difference has lost 10 of its bits - this element again in f64
          if (fabsf(gr) < t * 0x1p-10f) gr = (float)(st * (exp((double)v[i] - (double)m) / se) - (double)t);
          v[i] = (gr * inv_rows) * g;
        }
        ce_store<T>(d, e0, nc, vec_d, v);
      }
    }
  }
}

template <typename T>
static void mix_ce_launch(const void* logits, int64_t ldl, const int64_t* labels, const MixRow* table, int B, int row0, int rows,
                          int nc, float on, float off, const float* gscale, double* rowsum, void* dlogits, int64_t ldd,
                          hipStream_t st) {
  const int es = (int)sizeof(T);
  // 16-byte pieces only where every row of the operand starts on a 16-byte boundary
  const int vec_l = !(((uintptr_t)logits) & 15) && !((ldl * es) & 15);
  const int vec_d = dlogits && !(((uintptr_t)dlogits) & 15) && !((ldd * es) & 15);
  const float inv_rows = (float)(1.0 / (double)rows);
  const dim3 grid((unsigned)rows);
#define OCTIC_CE_LAUNCH(E)                                                                                                   \
  mix_ce_kernel<T, E><<<grid, 256, 0, st>>>((const T*)logits, ldl, labels, table, B, row0, nc, on, off, inv_rows, gscale, rowsum, \
                                            (T*)dlogits, ldd, vec_l, vec_d)
  if (nc <= 256 * CE_SMALL_E) OCTIC_CE_LAUNCH(CE_SMALL_E);
  else if (nc <= 256 * CE_LARGE_E) OCTIC_CE_LAUNCH(CE_LARGE_E);
  else OCTIC_CE_LAUNCH(0);
#undef OCTIC_CE_LAUNCH
}

// ------------------------------------------------------------------------------------------------ 5. cosub: four BCE terms
// one workgroup per SAMPLE: its first-pass row a and its second-pass row b (rows further down) are read once, both gradient rows
// written.  bce(x, t) is mix_bce_kernel's expression; the sigmoid targets are constants.  The expressions are mirror images in
// (a, b), and f32 / f64 addition commutes, so swapping the halves swaps the gradients and leaves the loss, bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void cosub_bce_kernel(const T* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels,
                                                        const MixRow* __restrict__ table, int B, int row0, int rows, int nc, float on,
                                                        float off, int binarize, float scale, const float* __restrict__ gscale,
                                                        double* __restrict__ rowsum, T* __restrict__ dlogits, int64_t ldd) {
  __shared__ double red[4];
  const int row = blockIdx.x, b = row0 + row;
  const MixRow r = mix_row(table, b, B);
  int la, lb;
  mix_labels(labels, r, b, nc, la, lb);
  const float lam = r.lam, oml = 1.f - r.lam;
  const float g = gscale ? gscale[0] : 1.f;
  const T* xa = logits + (int64_t)row * ldl;
  const T* xb = logits + ((int64_t)rows + row) * ldl;
  T* da = dlogits ? dlogits + (int64_t)row * ldd : nullptr;
  T* db = dlogits ? dlogits + ((int64_t)rows + row) * ldd : nullptr;
  double acc = 0.0;
  for (int j = threadIdx.x; j < nc; j += 256) {
    const float va = (float)xa[j], vb = (float)xb[j];
    const float t = mixed_target(j, la, lb, lam, oml, on, off, binarize);
    const float ea = expf(-fabsf(va)), eb = expf(-fabsf(vb));
    const float sa = (va >= 0.f ? 1.f : ea) / (1.f + ea), sb = (vb >= 0.f ? 1.f : eb) / (1.f + eb);
    if (rowsum) {
      const float la1 = log1pf(ea), lb1 = log1pf(eb), pa = fmaxf(va, 0.f), pb = fmaxf(vb, 0.f);
      const double hard = (double)((pa - va * t) + la1) + (double)((pb - vb * t) + lb1);
      const double soft = (double)((pa - va * sb) + la1) + (double)((pb - vb * sa) + lb1);
      acc += hard + soft;
    }
    if (da) {
      store_as<T>(da + j, (((sa - t) + (sa - sb)) * scale) * g);
      store_as<T>(db + j, (((sb - t) + (sb - sa)) * scale) * g);
    }
  }
  if (rowsum) {
    acc = wave_total_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) rowsum[row] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

static bool overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_mix_images(const float* src, float* dst, const octic_mix_row* table, int B, int C, int H, int W, void* stream) {
  if (!src || !dst || !table) return OCTIC_ENULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return OCTIC_ESHAPE;
  const int64_t n = (int64_t)C * H * W;
  if (n > 0x7FFFFFFFll - 4) return OCTIC_ESHAPE;
  if ((((uintptr_t)src) & 3) || (((uintptr_t)dst) & 3) || (((uintptr_t)table) & 3)) return OCTIC_EALIGN;
  if (overlap(src, dst, n * B * 4)) return OCTIC_ESHAPE;
  const bool vec = (W % 4) == 0 && !(((uintptr_t)src) & 15) && !(((uintptr_t)dst) & 15);
  const int nv = (int)(vec ? n / 4 : n);
  const int per_block = MI_THREADS * MI_UNROLL;
  const int bps = (nv + per_block - 1) / per_block;
  if ((int64_t)bps * B > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  const dim3 grid((unsigned)((int64_t)bps * B));
  if (vec)
    mix_images_kernel<4><<<grid, MI_THREADS, 0, (hipStream_t)stream>>>(src, dst, table, B, H, W, nv, bps);
  else
    mix_images_kernel<1><<<grid, MI_THREADS, 0, (hipStream_t)stream>>>(src, dst, table, B, H, W, nv, bps);
  return launch_status();
}

static int mix_rows_check(const void* labels, const void* table, int B, int row0, int rows, int num_classes) {
  if (!labels || !table) return OCTIC_ENULL;
  if (B <= 0 || num_classes <= 0 || rows <= 0 || row0 < 0 || (int64_t)row0 + rows > B) return OCTIC_ESHAPE;
  if ((((uintptr_t)labels) & 7) || (((uintptr_t)table) & 3)) return OCTIC_EALIGN;
  return OCTIC_OK;
}

int octic_mix_targets(const int64_t* labels, const octic_mix_row* table, int B, int row0, int rows, int num_classes, float on,
                      float off, int binarize, float* targets, void* stream) {
  if (!targets) return OCTIC_ENULL;
  if (int e = mix_rows_check(labels, table, B, row0, rows, num_classes)) return e;
  if (rows > 65535) return OCTIC_ESHAPE;
  if (((uintptr_t)targets) & 3) return OCTIC_EALIGN;
  const dim3 grid((unsigned)((num_classes + 255) / 256), (unsigned)rows);
  mix_targets_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(labels, table, B, row0, num_classes, on, off, binarize, targets);
  return launch_status();
}

int octic_mix_bce(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B, int row0,
                  int rows, int num_classes, float on, float off, int binarize, float* loss, const float* gscale,
                  void* dlogits, int64_t ldd, void* workspace, void* stream) {
  if (!logits || (!loss && !dlogits) || (loss && !workspace)) return OCTIC_ENULL;
  if (int e = mix_rows_check(labels, table, B, row0, rows, num_classes)) return e;
  if (dtype != OCTIC_F32 && dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  if (ldl < num_classes || (dlogits && ldd < num_classes)) return OCTIC_ESHAPE;
  const int es = elem_size(dtype);
  if ((((uintptr_t)logits) & (es - 1)) || (dlogits && (((uintptr_t)dlogits) & (es - 1))) || (loss && (((uintptr_t)loss) & 3)) ||
      (workspace && (((uintptr_t)workspace) & 7)) || (gscale && (((uintptr_t)gscale) & 3)))
    return OCTIC_EALIGN;
  const double n = (double)rows * (double)num_classes;
  const float inv_n = (float)(1.0 / n);
  double* rowsum = loss ? (double*)workspace : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == OCTIC_BF16)
    mix_bce_kernel<bf16><<<dim3((unsigned)rows), 256, 0, st>>>((const bf16*)logits, ldl, labels, table, B, row0, num_classes, on,
                                                               off, binarize, inv_n, gscale, rowsum, (bf16*)dlogits, ldd);
  else
    mix_bce_kernel<float><<<dim3((unsigned)rows), 256, 0, st>>>((const float*)logits, ldl, labels, table, B, row0, num_classes, on,
                                                                off, binarize, inv_n, gscale, rowsum, (float*)dlogits, ldd);
  if (loss) mix_bce_finish_kernel<<<dim3(1), 64, 0, st>>>(rowsum, rows, 1.0 / n, loss);
  return launch_status();
}

// what octic_mix_ce and octic_cosub_bce check alike
static int criterion_check(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B,
                           int row0, int rows, int num_classes, const float* loss, const float* gscale, const void* dlogits,
                           int64_t ldd, const void* workspace) {
  if (!logits || (!loss && !dlogits) || (loss && !workspace)) return OCTIC_ENULL;
  if (int e = mix_rows_check(labels, table, B, row0, rows, num_classes)) return e;
  if (num_classes < 2 || num_classes > 0x7FFF0000) return OCTIC_ESHAPE;
  if (dtype != OCTIC_F32 && dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  if (ldl < num_classes || (dlogits && ldd < num_classes)) return OCTIC_ESHAPE;
  const int es = elem_size(dtype);
  if ((((uintptr_t)logits) & (es - 1)) || (dlogits && (((uintptr_t)dlogits) & (es - 1))) || (loss && (((uintptr_t)loss) & 3)) ||
      (workspace && (((uintptr_t)workspace) & 7)) || (gscale && (((uintptr_t)gscale) & 3)))
    return OCTIC_EALIGN;
  return OCTIC_OK;
}

int octic_mix_ce(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B, int row0,
                 int rows, int num_classes, float on, float off, float* loss, const float* gscale, void* dlogits, int64_t ldd,
                 void* workspace, void* stream) {
  if (int e = criterion_check(logits, dtype, ldl, labels, table, B, row0, rows, num_classes, loss, gscale, dlogits, ldd, workspace))
    return e;
  double* rowsum = loss ? (double*)workspace : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == OCTIC_BF16)
    mix_ce_launch<bf16>(logits, ldl, labels, table, B, row0, rows, num_classes, on, off, gscale, rowsum, dlogits, ldd, st);
  else
    mix_ce_launch<float>(logits, ldl, labels, table, B, row0, rows, num_classes, on, off, gscale, rowsum, dlogits, ldd, st);
  if (loss) mix_bce_finish_kernel<<<dim3(1), 64, 0, st>>>(rowsum, rows, 1.0 / (double)rows, loss);
  return launch_status();
}

int octic_cosub_bce(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B, int row0,
                    int rows, int num_classes, float on, float off, int binarize, float* loss, const float* gscale, void* dlogits,
                    int64_t ldd, void* workspace, void* stream) {
  if (int e = criterion_check(logits, dtype, ldl, labels, table, B, row0, rows, num_classes, loss, gscale, dlogits, ldd, workspace))
    return e;
  const double quarter_mean = 0.25 / ((double)rows * (double)num_classes);
  double* rowsum = loss ? (double*)workspace : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == OCTIC_BF16)
    cosub_bce_kernel<bf16><<<dim3((unsigned)rows), 256, 0, st>>>((const bf16*)logits, ldl, labels, table, B, row0, rows, num_classes,
                                                                 on, off, binarize, (float)quarter_mean, gscale, rowsum,
                                                                 (bf16*)dlogits, ldd);
  else
    cosub_bce_kernel<float><<<dim3((unsigned)rows), 256, 0, st>>>((const float*)logits, ldl, labels, table, B, row0, rows,
                                                                  num_classes, on, off, binarize, (float)quarter_mean, gscale, rowsum,
                                                                  (float*)dlogits, ldd);
  if (loss) mix_bce_finish_kernel<<<dim3(1), 64, 0, st>>>(rowsum, rows, quarter_mean, loss);
  return launch_status();
}

}  // extern "C"
