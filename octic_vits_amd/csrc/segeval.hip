// Linear segmentation evaluation of a frozen backbone (dinov2/eval/segmentation/eval_segmentation.py:281-337, the logreg
// half of eval_model :346-470): multinomial logistic regression on standardised f32 patch features X [N, D] that stay
// resident in HBM, N in the millions.  One value-and-gradient evaluation of  J = scale * sum_n CE(x_n W^T + b, y_n) + lambda/2 |W|^2
// is three launches plus two tiny finishes:
//   1. seg_forward_kernel<NT>  : 128 rows x ALL classes per workgroup (the class axis is padded to ldd = 32 ceil(C / 32) = 16 NT),
//                                logits on the exact-f32 MFMA, then softmax / loss / dlogits = softmax - onehot from the
//                                accumulators: the logits never reach HBM.  Predict mode writes the row arg-max only.
//      seg_value_kernel        : the per-workgroup f64 loss partials in index order.
//   2. seg_wgrad_kernel<NT,DT> : dW partial = dlogits^T X over one row slab, tile = ALL 16 NT classes x DT columns
//                                (DT = 256 when D % 256 == 0 and NT <= 10, else 128, else 64).  Every X element is read by
//                                exactly one workgroup, so X crosses HBM once; dlogits is read D / DT times.  Algorithmic
//                                bytes at N = 3.564 M, D = 1280, C = 150 (ldd 160, DT 256): X 18.2 GB + 5 x 2.28 GB dlogits
//                                = 29.7 GB, against 1.46 TFLOP of MFMA work.
//      seg_wgrad_finish_kernel : slab partials summed in slab order in f64, times scale, plus lambda W (the regulariser).
//   3. seg_colstats_kernel / seg_standardize_kernel : StandardScaler.fit in f64 and its transform in place.
//   4. seg_mode_kernel      : patch label = mode of the patch's pixels, ties to the smallest value (torch.mode).
//   5. seg_confusion_kernel : integer counts of (pixel label, predicted patch label) over the non-ignored pixels.
// No floating-point atomics, every sum in a fixed order: results are bitwise equal from run to run.  Every row and
// element offset is 64-bit (N D exceeds 2^31 at real sizes).
// Rounding: a logit is the sum of D / 64 fmaf chains of 64 products, each started from zero; a weight-gradient element is one
// fmaf chain per row slab (N / slabs rows, in row order), the slab sums added in f64.
#include "octic_common.hpp"

namespace octic {
namespace {

__device__ __forceinline__ f32x4 seg_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr int SEG_FW_LD = 36;    // 32 k + 4: rows 16-byte aligned, a fragment read (16 rows x 4 k-quads) hits 64 banks
constexpr int SEG_FW_ROWS = 128;

// workgroup = 128 rows of X x 16 NT classes; wave w owns rows 16 RT w .. (RT x NT tiles of 16 x 16) and therefore whole logit
// rows: accumulator element e of tile (bt, ct) in lane (r, q) is logit[row 16 RT w + 16bt + 4q + e][class 16ct + r], a row
// lives in the 16 lanes of one q.  RT = 2 (4 waves) up to 160 classes, RT = 1 (8 waves) above: the accumulators of 2 x 16
// tiles and their chain partials do not fit the register file.
constexpr int seg_fw_threads(int NT) { return NT > 10 ? 512 : 256; }

template <int NT, bool PREDICT>
__global__ __launch_bounds__(seg_fw_threads(NT)) void seg_forward_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                          const float* __restrict__ W, const float* __restrict__ bias, int C,
                                                          const int* __restrict__ y, float* __restrict__ dlogits,
                                                          double* __restrict__ loss_part, int* __restrict__ pred) {
  __shared__ __attribute__((aligned(16))) float Xs[SEG_FW_ROWS * SEG_FW_LD];
  __shared__ __attribute__((aligned(16))) float Ws[NT * 16 * SEG_FW_LD];
  __shared__ double red[8];
  constexpr int LDD = NT * 16, NTHR = seg_fw_threads(NT), RT = 512 / NTHR, NW = NTHR / 64;
  constexpr int SROWS = NTHR / 8;                       // rows per staging pass (8 float4 per row)
  constexpr int XP = SEG_FW_ROWS / SROWS, WP = (LDD + SROWS - 1) / SROWS;
  const int64_t b0 = (int64_t)blockIdx.x * SEG_FW_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;   // staging: NTHR / 8 rows x 8 float4 per pass
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 fr[XP], wr[WP];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int64_t b = b0 + srow + SROWS * i;
      fr[i] = b < N ? *(const f32x4*)(X + b * ldx + k0 + sc4) : zero;
    }
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      const int c = srow + SROWS * i;
      wr[i] = c < C ? *(const f32x4*)(W + (int64_t)c * D + k0 + sc4) : zero;
    }
  };
  f32x4 acc[RT][NT], part[RT][NT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = part[i][j] = zero;
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += 32) {
    __syncthreads();                       // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < XP; ++i) *(f32x4*)(Xs + (srow + SROWS * i) * SEG_FW_LD + sc4) = fr[i];
#pragma unroll
    for (int i = 0; i < WP; ++i)
      if (srow + SROWS * i < LDD) *(f32x4*)(Ws + (srow + SROWS * i) * SEG_FW_LD + sc4) = wr[i];
    __syncthreads();
    if (k0 + 32 < D) fetch(k0 + 32);       // in flight under the products
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4 a4[RT];
#pragma unroll
      for (int bt = 0; bt < RT; ++bt) a4[bt] = *(const f32x4*)(Xs + (16 * RT * w + 16 * bt + r) * SEG_FW_LD + 16 * j + 4 * q);
#pragma unroll
      for (int h = 0; h < 2; ++h) {        // the class tiles in two halves: half the W fragments live at a time
        f32x4 b4[NT / 2];
#pragma unroll
        for (int ct = 0; ct < NT / 2; ++ct) b4[ct] = *(const f32x4*)(Ws + (16 * (ct + h * (NT / 2)) + r) * SEG_FW_LD + 16 * j + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int bt = 0; bt < RT; ++bt)
#pragma unroll
            for (int ct = 0; ct < NT / 2; ++ct)
              part[bt][ct + h * (NT / 2)] = seg_mfma16(a4[bt][e], b4[ct][e], part[bt][ct + h * (NT / 2)]);
      }
    }
    if (k0 & 32) {                         // D % 64 == 0: every chain is 64 long
#pragma unroll
      for (int bt = 0; bt < RT; ++bt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          acc[bt][ct] += part[bt][ct];
          part[bt][ct] = zero;
        }
    }
  }

  float bv[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) bv[ct] = 16 * ct + r < C ? bias[16 * ct + r] : 0.f;
  double lsum = 0.0;
#pragma unroll
  for (int bt = 0; bt < RT; ++bt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t row = b0 + 16 * RT * w + 16 * bt + 4 * q + e;
      const bool live = row < N;           // uniform over the 16 lanes of a row: the shuffles below stay inside them
      float x[NT];
      float m = -INFINITY;
      int am = 0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + r;
        x[ct] = c < C ? acc[bt][ct][e] + bv[ct] : -INFINITY;
        if (x[ct] > m) { m = x[ct]; am = c; }
      }
      if (PREDICT) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {   // first maximum wins, as numpy.argmax
          const float om = __shfl_xor(m, o);
          const int oa = __shfl_xor(am, o);
          if (om > m || (om == m && oa < am)) { m = om; am = oa; }
        }
        if (live && r == 0) pred[row] = am;
        continue;
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
      float s = 0.f;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) s += expf(x[ct] - m);   // exp(-inf) = 0 for the padded classes
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
      const float ls = logf(s);
      int lab = live ? y[row] : -1;
      if (lab < 0 || lab >= C) lab = -1;   // not a class index: the row contributes nothing
      float* drow = dlogits + row * LDD;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + r;
        float d = 0.f;
        if (lab >= 0 && c < C) {
          d = expf((x[ct] - m) - ls);
          if (c == lab) {
            d -= 1.f;
            lsum += (double)((m + ls) - x[ct]);
          }
        }
        if (live) drow[c] = d;
      }
    }
  if (PREDICT) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
  if (lane == 0) red[w] = lsum;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) t += red[i];
    loss_part[blockIdx.x] = t;
  }
}

// one workgroup: strided f64 sums, then the 256 thread totals in index order
__global__ __launch_bounds__(256) void seg_value_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ value) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    value[0] = t;
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// workgroup = (column tile of DT, row slab): all 16 NT classes x DT columns; wave w owns columns (DT / 4) w .. and every
// class (NT x DT / 64 tiles).  A = dlogits^T (rows = classes), B = X, k = data rows, 4 per MFMA step in row order;
// accumulator element e of tile (ct, j) in lane (r, q) is g[class 16ct + 4q + e][column (DT / 4) w + 16 j + r].
// LDS rows are padded by 16 floats: the 4 data rows of a step land in 4 different groups of 16 banks.
constexpr int SEG_WG_ROWS = 32;     // data rows per staged chunk

template <int NT, int DT>
__global__ __launch_bounds__(256) void seg_wgrad_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                        const float* __restrict__ dl, int64_t slab_rows,
                                                        float* __restrict__ wpart, double* __restrict__ dbpart) {
  constexpr int LDD = NT * 16, DLD = LDD + 16, XLD = DT + 16, CW = DT / 64;
  constexpr int XQ = DT / 4;           // float4 per X row of the tile
  constexpr int XPASS = DT / 32;       // float4 per thread per chunk
  constexpr int DPASS = NT / 2;
  __shared__ __attribute__((aligned(16))) float Xs[SEG_WG_ROWS * XLD];
  __shared__ __attribute__((aligned(16))) float Ds[SEG_WG_ROWS * DLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int d0 = blockIdx.x * DT;
  const int64_t n0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t n1 = n0 + slab_rows < N ? n0 + slab_rows : N;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int xrow = tid / XQ, xc4 = (tid % XQ) * 4;   // X pass p: row xrow + (256 / XQ) p
  f32x4 xr[XPASS], dr[DPASS];
  auto fetch = [&](int64_t nb) {
#pragma unroll
    for (int p = 0; p < XPASS; ++p) {
      const int64_t n = nb + xrow + (256 / XQ) * p;
      xr[p] = n < n1 ? *(const f32x4*)(X + n * ldx + d0 + xc4) : zero;
    }
#pragma unroll
    for (int p = 0; p < DPASS; ++p) {
      const int idx = tid + 256 * p;                 // float4 index in the contiguous 32 x LDD chunk
      const int64_t n = nb + idx / (LDD / 4);
      dr[p] = n < n1 ? *(const f32x4*)(dl + nb * LDD + (int64_t)idx * 4) : zero;
    }
  };
  f32x4 acc[NT][CW];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < CW; ++j) acc[i][j] = zero;
  const bool do_bias = blockIdx.x == 0 && tid < LDD;
  double gb = 0.0;
  if (n0 < n1) fetch(n0);
  for (int64_t nb = n0; nb < n1; nb += SEG_WG_ROWS) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < XPASS; ++p) *(f32x4*)(Xs + (xrow + (256 / XQ) * p) * XLD + xc4) = xr[p];
#pragma unroll
    for (int p = 0; p < DPASS; ++p) {
      const int idx = tid + 256 * p;
      *(f32x4*)(Ds + (idx / (LDD / 4)) * DLD + (idx % (LDD / 4)) * 4) = dr[p];
    }
    __syncthreads();
    if (nb + SEG_WG_ROWS < n1) fetch(nb + SEG_WG_ROWS);
    if (do_bias) {
#pragma unroll 8
      for (int b = 0; b < SEG_WG_ROWS; ++b) gb += (double)Ds[b * DLD + tid];   // row order, f64
    }
#pragma unroll 2
    for (int s = 0; s < SEG_WG_ROWS / 4; ++s) {
      float a[NT], b[CW];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) a[ct] = Ds[(4 * s + q) * DLD + 16 * ct + r];
#pragma unroll
      for (int j = 0; j < CW; ++j) b[j] = Xs[(4 * s + q) * XLD + (DT / 4) * w + 16 * j + r];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int j = 0; j < CW; ++j) acc[ct][j] = seg_mfma16(a[ct], b[j], acc[ct][j]);
    }
  }
  float* out = wpart + (int64_t)blockIdx.y * LDD * D;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int j = 0; j < CW; ++j) {
      const f32x4 v = acc[ct][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(int64_t)(16 * ct + 4 * q + e) * D + d0 + (DT / 4) * w + 16 * j + r] = v[e];
    }
  if (do_bias) dbpart[(int64_t)blockIdx.y * LDD + tid] = gb;
}

// one thread per element of dW (and the first C threads of the last block row for db): slab order, f64
__global__ __launch_bounds__(256) void seg_wgrad_finish_kernel(const float* __restrict__ wpart, const double* __restrict__ dbpart,
                                                               int slabs, int ldd, int C, int D, const float* __restrict__ W,
                                                               double scale, double lambda, float* __restrict__ dW,
                                                               float* __restrict__ db) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)C * D;
  if (i < total) {
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += (double)wpart[(int64_t)k * ldd * D + i];
    dW[i] = (float)(scale * s + lambda * (double)W[i]);
  } else if (i < total + C) {
    const int c = (int)(i - total);
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += dbpart[(int64_t)k * ldd + c];
    db[c] = (float)(scale * s);
  }
}

// ------------------------------------------------------------------------------------------------ column statistics
// workgroup = 64 columns x one row slab; thread = 4 columns (one float4), 16 threads share a column quad and take rows
// slab + rl, + 16, ...  Sums of (x - x[0, col]) and its square in f64 (the shift keeps the one-pass variance free of
// cancellation), the 16 row lanes added in index order through LDS.
__global__ __launch_bounds__(256) void seg_colstats_kernel(const float* __restrict__ X, int64_t ldx, int64_t N,
                                                           int64_t slab_rows, int D, double* __restrict__ part) {
  __shared__ double red[16][16][8];
  const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cq;
  const int64_t n0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t n1 = n0 + slab_rows < N ? n0 + slab_rows : N;
  const f32x4 k4 = *(const f32x4*)(X + col);
  double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
  int64_t n = n0 + rl;
  for (; n + 48 < n1; n += 64) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(X + (n + 16 * u) * ldx + col);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)v[u][j] - (double)k4[j];
        s[j] += d;
        ss[j] += d * d;
      }
  }
  for (; n < n1; n += 16) {
    const f32x4 v = *(const f32x4*)(X + n * ldx + col);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)v[j] - (double)k4[j];
      s[j] += d;
      ss[j] += d * d;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[rl][cq][j] = s[j]; red[rl][cq][4 + j] = ss[j]; }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c = threadIdx.x >> 3, j = threadIdx.x & 7;   // column quad c, statistic j
    double t = 0.0;
    for (int i = 0; i < 16; ++i) t += red[i][c][j];
    part[((int64_t)blockIdx.y * 2 + (j >> 2)) * D + blockIdx.x * 64 + 4 * c + (j & 3)] = t;
  }
}

__global__ __launch_bounds__(256) void seg_colstats_finish_kernel(const double* __restrict__ part, int slabs, int D, int64_t N,
                                                                  const float* __restrict__ X, double* __restrict__ mean,
                                                                  double* __restrict__ var) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  double s = 0.0, ss = 0.0;
  for (int k = 0; k < slabs; ++k) {
    s += part[((int64_t)k * 2) * D + d];
    ss += part[((int64_t)k * 2 + 1) * D + d];
  }
  const double m = s / (double)N;
  mean[d] = (double)X[d] + m;
  const double v = ss / (double)N - m * m;
  var[d] = v > 0.0 ? v : 0.0;
}

// x = float(float(double(x) - mean) / scale): the two roundings of StandardScaler.transform on an f32 array
__global__ __launch_bounds__(256) void seg_standardize_kernel(float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                              const double* __restrict__ mean, const double* __restrict__ scale) {
  const int dq = D / 4;
  const int64_t total = N * dq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / dq;
    const int c = (int)(i - n * dq) * 4;
    float* p = X + n * ldx + c;
    f32x4 v = *(const f32x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = (float)((double)v[j] - mean[c + j]);
      v[j] = (float)((double)t / scale[c + j]);
    }
    *(f32x4*)p = v;
  }
}

// ------------------------------------------------------------------------------------------------ labels
template <typename T>
__device__ __forceinline__ int seg_label(const void* p, int64_t i) { return (int)((const T*)p)[i] & 255; }
__device__ __forceinline__ int seg_label_at(const void* p, int esize, int64_t i) {
  return esize == 1 ? seg_label<uint8_t>(p, i) : esize == 2 ? seg_label<int16_t>(p, i)
       : esize == 4 ? seg_label<int32_t>(p, i) : seg_label<int64_t>(p, i);
}

// one wave per patch row: a 256-bin LDS histogram (integer LDS atomics), then the largest count, smallest value on a tie
__global__ __launch_bounds__(256) void seg_mode_kernel(const void* __restrict__ labels, int esize, int64_t R, int L,
                                                       int* __restrict__ mode) {
  __shared__ int hist[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < R; row += (int64_t)gridDim.x * 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[w][lane + 64 * j] = 0;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < L; i += 64) atomicAdd(&hist[w][seg_label_at(labels, esize, row * L + i)], 1);
    __builtin_amdgcn_wave_barrier();
    int best = -1, val = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // ascending values: a strict > keeps the smallest
      const int c = hist[w][lane + 64 * j];
      if (c > best) { best = c; val = lane + 64 * j; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ob = __shfl_xor(best, o), ov = __shfl_xor(val, o);
      if (ob > best || (ob == best && ov < val)) { best = ob; val = ov; }
    }
    if (lane == 0) mode[row] = val;
    __builtin_amdgcn_wave_barrier();
  }
}

// one wave per patch row: histogram of the row's pixel labels, then counts[label][pred[row]] += n for the labels that are
// not ignored (64-bit integer atomics: exact and order-free)
__global__ __launch_bounds__(256) void seg_confusion_kernel(const void* __restrict__ labels, int esize, int64_t R, int L,
                                                            const int* __restrict__ pred, const uint8_t* __restrict__ ignore,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ int hist[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < R; row += (int64_t)gridDim.x * 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[w][lane + 64 * j] = 0;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < L; i += 64) atomicAdd(&hist[w][seg_label_at(labels, esize, row * L + i)], 1);
    __builtin_amdgcn_wave_barrier();
    const int p = pred[row] & 255;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = lane + 64 * j;
      const int c = hist[w][t];
      if (c > 0 && !ignore[t]) atomicAdd(&counts[t * 256 + p], (unsigned long long)c);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline int seg_check(const void* X, int64_t ldx, int64_t N, int D, int C) {
  if (!X) return OCTIC_ENULL;
  if (N < 1 || D < 64 || D % 64 || C < 2 || C > 256 || ldx < D) return OCTIC_ESHAPE;
  if ((N + SEG_FW_ROWS - 1) / SEG_FW_ROWS > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if ((((uintptr_t)X) & 15) || (ldx & 3)) return OCTIC_EALIGN;
  return OCTIC_OK;
}
inline int seg_ldd(int C) { return 32 * ((C + 31) / 32); }
inline int seg_dt(int D, int C) { return (D % 256 == 0 && seg_ldd(C) <= 160) ? 256 : (D % 128 == 0 ? 128 : 64); }
inline int seg_slabs(int64_t N, int D, int C) {
  const int64_t chunks = (N + SEG_WG_ROWS - 1) / SEG_WG_ROWS;
  int64_t s = device_cus() / (D / seg_dt(D, C));
  // a slab's partial tile is as large as ldd rows of X: keep the workspace below a quarter of X (and the finish launch
  // below the MFMA work) when N is small
  const int64_t cap = N / (4 * seg_ldd(C));
  if (s > cap) s = cap;
  if (s > chunks) s = chunks;
  if (s < 1) s = 1;
  return (int)s;
}
inline int64_t seg_slab_rows(int64_t N, int slabs) {
  const int64_t per = (N + slabs - 1) / slabs;
  return (per + SEG_WG_ROWS - 1) / SEG_WG_ROWS * SEG_WG_ROWS;
}
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
struct SegWs { int64_t loss, db, w, total; };
inline SegWs seg_ws(int64_t N, int D, int C) {
  SegWs r;
  const int slabs = seg_slabs(N, D, C), ldd = seg_ldd(C);
  r.loss = 0;
  r.db = align256(8 * ((N + SEG_FW_ROWS - 1) / SEG_FW_ROWS));
  r.w = r.db + align256(8ll * slabs * ldd);
  r.total = r.w + align256(4ll * slabs * ldd * D);
  return r;
}
inline int cs_slabs(int64_t N, int D) {
  int64_t s = 4ll * device_cus() / (D / 64);
  if (s < 1) s = 1;
  const int64_t most = (N + 63) / 64;
  return (int)(s > most ? most : s);
}

#define SEG_NT_SWITCH(nt, CALL)                                                                        \
  switch (nt) {                                                                                        \
    case 2: CALL(2); break;   case 4: CALL(4); break;   case 6: CALL(6); break;   case 8: CALL(8); break; \
    case 10: CALL(10); break; case 12: CALL(12); break; case 14: CALL(14); break; default: CALL(16); break; \
  }

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_seg_ldd(int C) { return (C < 2 || C > 256) ? OCTIC_ESHAPE : seg_ldd(C); }

int octic_seg_slabs(int64_t N, int D, int C) {
  if (N < 1 || D < 64 || D % 64 || C < 2 || C > 256) return OCTIC_ESHAPE;
  return seg_slabs(N, D, C);
}

int64_t octic_seg_workspace_bytes(int64_t N, int D, int C) {
  if (N < 1 || D < 64 || D % 64 || C < 2 || C > 256) return OCTIC_ESHAPE;
  return seg_ws(N, D, C).total;
}

int octic_seg_value_dlogits(const float* X, int64_t ldx, int64_t N, int D, const float* W, const float* b, int C,
                            const int32_t* y, float* dlogits, double* value, void* workspace, void* stream) {
  if (int e = seg_check(X, ldx, N, D, C)) return e;
  if (!W || !b || !y || !dlogits || !value || !workspace) return OCTIC_ENULL;
  if ((((uintptr_t)W) & 15) || (((uintptr_t)dlogits) & 15) || (((uintptr_t)workspace) & 255)) return OCTIC_EALIGN;
  const int64_t nblk = (N + SEG_FW_ROWS - 1) / SEG_FW_ROWS;
  double* loss_part = (double*)workspace;
  const hipStream_t st = (hipStream_t)stream;
#define SEG_CALL(NT_) seg_forward_kernel<NT_, false><<<dim3((unsigned)nblk), seg_fw_threads(NT_), 0, st>>>(X, ldx, N, D, W, b, C, y, dlogits, loss_part, nullptr)
  SEG_NT_SWITCH(seg_ldd(C) / 16, SEG_CALL)
#undef SEG_CALL
  seg_value_kernel<<<1, 256, 0, st>>>(loss_part, nblk, value);
  return launch_status();
}

int octic_seg_predict(const float* X, int64_t ldx, int64_t N, int D, const float* W, const float* b, int C, int32_t* pred,
                      void* stream) {
  if (int e = seg_check(X, ldx, N, D, C)) return e;
  if (!W || !b || !pred) return OCTIC_ENULL;
  if (((uintptr_t)W) & 15) return OCTIC_EALIGN;
  const int64_t nblk = (N + SEG_FW_ROWS - 1) / SEG_FW_ROWS;
  const hipStream_t st = (hipStream_t)stream;
#define SEG_CALL(NT_) seg_forward_kernel<NT_, true><<<dim3((unsigned)nblk), seg_fw_threads(NT_), 0, st>>>(X, ldx, N, D, W, b, C, nullptr, nullptr, nullptr, pred)
  SEG_NT_SWITCH(seg_ldd(C) / 16, SEG_CALL)
#undef SEG_CALL
  return launch_status();
}

int octic_seg_wgrad(const float* X, int64_t ldx, int64_t N, int D, const float* dlogits, int C, const float* W, double scale,
                    double lambda, float* dW, float* db, void* workspace, void* stream) {
  if (int e = seg_check(X, ldx, N, D, C)) return e;
  if (!dlogits || !W || !dW || !db || !workspace) return OCTIC_ENULL;
  if ((((uintptr_t)dlogits) & 15) || (((uintptr_t)workspace) & 255)) return OCTIC_EALIGN;
  const SegWs ws = seg_ws(N, D, C);
  const int slabs = seg_slabs(N, D, C), ldd = seg_ldd(C), dt = seg_dt(D, C);
  const int64_t slab_rows = seg_slab_rows(N, slabs);
  double* dbpart = (double*)((char*)workspace + ws.db);
  float* wpart = (float*)((char*)workspace + ws.w);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(D / dt), (unsigned)slabs);
#define SEG_CALL_DT(NT_, DT_) seg_wgrad_kernel<NT_, DT_><<<grid, 256, 0, st>>>(X, ldx, N, D, dlogits, slab_rows, wpart, dbpart)
#define SEG_CALL_LO(NT_) do { if (dt == 256) SEG_CALL_DT(NT_, 256); else if (dt == 128) SEG_CALL_DT(NT_, 128); else SEG_CALL_DT(NT_, 64); } while (0)
#define SEG_CALL_HI(NT_) do { if (dt == 128) SEG_CALL_DT(NT_, 128); else SEG_CALL_DT(NT_, 64); } while (0)
  switch (ldd / 16) {
    case 2: SEG_CALL_LO(2); break;
    case 4: SEG_CALL_LO(4); break;
    case 6: SEG_CALL_LO(6); break;
    case 8: SEG_CALL_LO(8); break;
    case 10: SEG_CALL_LO(10); break;
    case 12: SEG_CALL_HI(12); break;
    case 14: SEG_CALL_HI(14); break;
    default: SEG_CALL_HI(16); break;
  }
#undef SEG_CALL_HI
#undef SEG_CALL_LO
#undef SEG_CALL_DT
  const int64_t total = (int64_t)C * D + C;
  seg_wgrad_finish_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(wpart, dbpart, slabs, ldd, C, D, W, scale, lambda,
                                                                                 dW, db);
  return launch_status();
}

int64_t octic_seg_colstats_workspace_bytes(int64_t N, int D) {
  if (N < 1 || D < 64 || D % 64) return OCTIC_ESHAPE;
  return 16ll * cs_slabs(N, D) * D;
}

int octic_seg_colstats(const float* X, int64_t ldx, int64_t N, int D, double* mean, double* var, void* workspace, void* stream) {
  if (int e = seg_check(X, ldx, N, D, 2)) return e;
  if (!mean || !var || !workspace) return OCTIC_ENULL;
  const int slabs = cs_slabs(N, D);
  int64_t slab_rows = (N + slabs - 1) / slabs;
  slab_rows = (slab_rows + 15) / 16 * 16;
  const hipStream_t st = (hipStream_t)stream;
  seg_colstats_kernel<<<dim3((unsigned)(D / 64), (unsigned)slabs), 256, 0, st>>>(X, ldx, N, slab_rows, D, (double*)workspace);
  seg_colstats_finish_kernel<<<dim3((unsigned)((D + 255) / 256)), 256, 0, st>>>((const double*)workspace, slabs, D, N, X, mean, var);
  return launch_status();
}

int octic_seg_standardize(float* X, int64_t ldx, int64_t N, int D, const double* mean, const double* scale, void* stream) {
  if (int e = seg_check(X, ldx, N, D, 2)) return e;
  if (!mean || !scale) return OCTIC_ENULL;
  int64_t blocks = (N * (D / 4) + 255) / 256;
  const int64_t cap = 32ll * device_cus();
  if (blocks > cap) blocks = cap;
  seg_standardize_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(X, ldx, N, D, mean, scale);
  return launch_status();
}

static int seg_label_check(const void* labels, int esize, int64_t R, int L) {
  if (!labels) return OCTIC_ENULL;
  if (R < 1 || L < 1) return OCTIC_ESHAPE;
  if (esize != 1 && esize != 2 && esize != 4 && esize != 8) return OCTIC_EDTYPE;
  if (((uintptr_t)labels) & (esize - 1)) return OCTIC_EALIGN;
  return OCTIC_OK;
}

int octic_seg_patch_mode(const void* labels, int esize, int64_t R, int L, int32_t* mode, void* stream) {
  if (int e = seg_label_check(labels, esize, R, L)) return e;
  if (!mode) return OCTIC_ENULL;
  int64_t blocks = (R + 3) / 4;
  const int64_t cap = 32ll * device_cus();
  if (blocks > cap) blocks = cap;
  seg_mode_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(labels, esize, R, L, mode);
  return launch_status();
}

int octic_seg_confusion(const void* labels, int esize, int64_t R, int L, const int32_t* pred, const uint8_t* ignore,
                        int64_t* counts, void* stream) {
  if (int e = seg_label_check(labels, esize, R, L)) return e;
  if (!pred || !ignore || !counts) return OCTIC_ENULL;
  int64_t blocks = (R + 3) / 4;
  const int64_t cap = 32ll * device_cus();
  if (blocks > cap) blocks = cap;
  seg_confusion_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(labels, esize, R, L, pred, ignore,
                                                                               (unsigned long long*)counts);
  return launch_status();
}

}  // extern "C"
