// Linear-probe evaluation of a frozen backbone (dinov2/eval/linear.py): the grid of nn.Linear(out_dim, C) classifiers that
// setup_linear_classifiers builds (linear.py:237-258) trained together by SGD with momentum (linear.py:344-366, 519-521), as
// four launches over ALL classifiers, driven by a device table of octic_probe_head entries:
//   1. probe_features_kernel : F[B, (n+1) D] = [cls(L-n) | ... | cls(L-1) | mean patch(L-1)]  (create_linear_input,
//                              linear.py:173-185: every classifier's input is a column range of this row - no torch.cat)
//   2. probe_forward_kernel  : logits[h] = F[:, col0 : col0 + K] W_h^T + b_h                  (LinearClassifier.forward)
//   3. probe_ce_kernel       : row log-sum-exp, loss, dlogits = (softmax - onehot) / B, rank of the label; then
//      probe_ce_finish_kernel: per-classifier mean loss and top-1 / top-5 counters, accumulated on the device
//   4. probe_sgd_kernel      : per 64 x 64 tile of W_h: g = dlogits^T F over the B rows in registers, buf = mu buf + g,
//                              W -= lr buf.  The gradient never reaches HBM: 16 B / parameter instead of 28.
// Exact f32 throughout (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain), no atomics, every sum in a fixed order: a graph
// replay equals the eager step bit for bit.  Kernel 4 is a stream over W and its momentum (each lane owns 64 contiguous
// bytes of a row, a row of the tile is 256 contiguous bytes, all eight 16-byte loads of a lane are issued before the
// products start); the B x 64 slices of F and dlogits a tile needs come from L2 through LDS.
#include "octic_common.hpp"

namespace octic {

typedef octic_probe_head ProbeHead;

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ 1. features
struct FeatArgs {
  const void* cls[4];
  int64_t cls_ld[4];
  const void* patch;
  int64_t ld_b, ld_t;
  int n, P, D;
  float* F;
  int64_t ldf;
};

template <typename T>
__device__ __forceinline__ f32x4 load4(const T* p);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float* p) { return *(const f32x4*)p; }
template <>
__device__ __forceinline__ f32x4 load4<bf16>(const bf16* p) {
  const bf16x4 a = *(const bf16x4*)p;
  return f32x4{(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
}

// one thread = 4 columns of one image; the patch mean is an f32 sum in token order (compensated) times 1/P, rounded to the token dtype
// (what torch.mean returns for it) before the widening .float()
template <typename T>
__global__ __launch_bounds__(256) void probe_features_kernel(FeatArgs a) {
  const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t b = blockIdx.y;
  if (col >= a.D) return;
  float* Fr = a.F + b * a.ldf;
  for (int i = 0; i < a.n; ++i)
    *(f32x4*)(Fr + (int64_t)i * a.D + col) = load4<T>((const T*)a.cls[i] + b * a.cls_ld[i] + col);
  const T* x = (const T*)a.patch + b * a.ld_b + col;
  // token order, compensated (Kahan): the sum of up to ~1400 tokens stays within an ulp of the exact one
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, comp = {0.f, 0.f, 0.f, 0.f};
  auto add = [&](f32x4 v) {
    const f32x4 y = v - comp;
    const f32x4 u = s + y;
    comp = (u - s) - y;
    s = u;
  };
  int t = 0;
  for (; t + 8 <= a.P; t += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = load4<T>(x + (int64_t)(t + u) * a.ld_t);
#pragma unroll
    for (int u = 0; u < 8; ++u) add(v[u]);
  }
  for (; t < a.P; ++t) add(load4<T>(x + (int64_t)t * a.ld_t));
  const float inv = 1.0f / (float)a.P;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float m = s[j] * inv;
    if (sizeof(T) == 2) m = (float)(bf16)m;
    s[j] = m;
  }
  *(f32x4*)(Fr + (int64_t)a.n * a.D + col) = s;
}

// ------------------------------------------------------------------------------------------------ 2. forward
constexpr int FW_LD = 36;   // 32 k + 4: rows 16-byte aligned, the 16 rows x 4 k-quads of a fragment read hit 64 banks

// workgroup = 128 rows of F x 64 classes, k in chunks of 32 through LDS; wave w owns rows 32w .. 32w+31 (2 x 4 tiles of
// 16 x 16).  A lane takes 4 consecutive k of its row with one ds_read_b128 and feeds them to 4 MFMA steps, so step e sums
// k = 4q + e (q = lane >> 4) - the same permutation on both operands, a fixed order.
__global__ __launch_bounds__(256) void probe_forward_kernel(const ProbeHead* __restrict__ heads, const float* __restrict__ F,
                                                            int64_t ldf, int B, int C, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float Fs[128 * FW_LD];
  __shared__ __attribute__((aligned(16))) float Ws[64 * FW_LD];
  const ProbeHead h = heads[blockIdx.y];
  const int c0 = blockIdx.x * 64, b0 = blockIdx.z * 128;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const float* Fb = F + h.col0;
  // staging map: F chunk = 128 rows x 8 float4 (4 per thread), W chunk = 64 rows x 8 float4 (2 per thread)
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  f32x4 fr[4], wr[2];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = b0 + srow + 32 * i;
      fr[i] = b < B ? *(const f32x4*)(Fb + (int64_t)b * ldf + k0 + sc4) : zero;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = c0 + srow + 32 * i;
      wr[i] = c < C ? *(const f32x4*)(h.w + (int64_t)c * h.K + k0 + sc4) : zero;
    }
  };
  // Each 32-wide k chunk is its own fmaf chain from zero; the chunk sums are added with a compensated (Kahan) sum, so
  // the rounding error does not grow with K (a single chain over K = 6400 is several times further from the exact
  // product than a blocked library GEMM).
  f32x4 acc[2][4], comp[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = comp[i][j] = zero;
  fetch(0);
  for (int k0 = 0; k0 < h.K; k0 += 32) {
    __syncthreads();                       // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) *(f32x4*)(Fs + (srow + 32 * i) * FW_LD + sc4) = fr[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *(f32x4*)(Ws + (srow + 32 * i) * FW_LD + sc4) = wr[i];
    __syncthreads();
    if (k0 + 32 < h.K) fetch(k0 + 32);     // in flight under the products
    f32x4 part[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4 a4[2], b4[4];
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) a4[bt] = *(const f32x4*)(Fs + (32 * w + 16 * bt + r) * FW_LD + 16 * j + 4 * q);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) b4[ct] = *(const f32x4*)(Ws + (16 * ct + r) * FW_LD + 16 * j + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
          for (int ct = 0; ct < 4; ++ct)
            part[bt][ct] = mfma16(a4[bt][e], b4[ct][e], (j == 0 && e == 0) ? zero : part[bt][ct]);
    }
#pragma unroll
    for (int bt = 0; bt < 2; ++bt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f32x4 y = part[bt][ct] - comp[bt][ct];
        const f32x4 u = acc[bt][ct] + y;
        comp[bt][ct] = (u - acc[bt][ct]) - y;
        acc[bt][ct] = u;
      }
  }
  float* out = logits + (int64_t)blockIdx.y * B * C;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int c = c0 + 16 * ct + r;
    if (c >= C) continue;
    const float bias = h.b[c];
#pragma unroll
    for (int bt = 0; bt < 2; ++bt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = b0 + 32 * w + 16 * bt + 4 * q + e;
        if (b < B) out[(int64_t)b * C + c] = acc[bt][ct][e] + bias;
      }
  }
}

// ------------------------------------------------------------------------------------------------ 3. cross entropy
__device__ __forceinline__ float ce_block_sum(float v, float* red) {   // fixed order: wave totals, then waves 0..3
  v = wave_total(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

// one workgroup per logit row (classifier h, image b).  rank = number of logits strictly greater than the label's.
__global__ __launch_bounds__(256) void probe_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       int B, int C, float* __restrict__ dlogits,
                                                       float* __restrict__ rowloss, int* __restrict__ rowrank) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const int b = (int)(row % B);
  const float* x = logits + row * C;
  const int64_t lab64 = labels[b];
  const bool valid = lab64 >= 0 && lab64 < C;
  const int lab = valid ? (int)lab64 : -1;
  const float xl = valid ? x[lab] : INFINITY;
  float m = -INFINITY;
  int gt = 0;
  for (int j = threadIdx.x; j < C; j += 256) {
    const float v = x[j];
    m = fmaxf(m, v);
    gt += v > xl ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o));
    gt += __shfl_xor(gt, o);
  }
  __shared__ int redi[4];
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = m; redi[threadIdx.x >> 6] = gt; }
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  gt = redi[0] + redi[1] + redi[2] + redi[3];
  __syncthreads();
  float s = 0.f;
  for (int j = threadIdx.x; j < C; j += 256) s += expf(x[j] - m);
  s = ce_block_sum(s, red);
  const float ls = logf(s);
  if (threadIdx.x == 0) {
    rowloss[row] = valid ? (m + ls) - xl : 0.f;
    rowrank[row] = valid ? gt : C;
  }
  if (dlogits) {
    float* d = dlogits + row * C;
    const float invB = 1.0f / (float)B;
    for (int j = threadIdx.x; j < C; j += 256) {
      const float p = expf((x[j] - m) - ls);
      d[j] = valid ? (p - (j == lab ? 1.f : 0.f)) * invB : 0.f;
    }
  }
}

// one wave per classifier: the B row losses in lane-strided order, then the wave total
__global__ __launch_bounds__(64) void probe_ce_finish_kernel(const float* __restrict__ rowloss, const int* __restrict__ rowrank,
                                                             int B, float* __restrict__ loss_mean,
                                                             float* __restrict__ loss_sum, int* __restrict__ topk) {
  const int h = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  int c1 = 0, c5 = 0;
  for (int b = lane; b < B; b += 64) {
    s += rowloss[(int64_t)h * B + b];
    const int rk = rowrank[(int64_t)h * B + b];
    c1 += rk < 1 ? 1 : 0;
    c5 += rk < 5 ? 1 : 0;
  }
  s = wave_total(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c1 += __shfl_xor(c1, o);
    c5 += __shfl_xor(c5, o);
  }
  if (lane == 0) {
    if (loss_mean) loss_mean[h] = s / (float)B;
    if (loss_sum) loss_sum[h] += s;
    if (topk) { topk[2 * h] += c1; topk[2 * h + 1] += c5; }
  }
}

// ------------------------------------------------------------------------------------------------ 4. gradient + SGD
constexpr int SG_LD = 80;   // 64 + 16: the 4 batch rows of an MFMA step land in 4 different groups of 16 banks

// workgroup = 64 classes x 64 columns of one W_h; wave w owns classes 16w .. 16w+15 and all 64 columns (4 tiles).
// Product orientation: A = F^T (rows = columns k of W), B = dlogits (columns = classes), so a result register quad is 4
// columns of ONE class.  Tile t takes k = 4 i + t for its row i: lane (r, q) reads F[b][4r .. 4r+3] with one
// ds_read_b128 for the 4 tiles, and ends up holding g[class 16w + r][16q + 4 reg + t] = acc[t][reg] - 16 consecutive
// columns, i.e. 64 contiguous bytes of the W row.  The batch is walked 4 rows per MFMA step in order: one fmaf chain
// per 32 rows, the chains added in row order.
__global__ __launch_bounds__(256) void probe_sgd_kernel(const ProbeHead* __restrict__ heads, int nheads,
                                                        const float* __restrict__ F, int64_t ldf,
                                                        const float* __restrict__ dlogits, int B, int C,
                                                        const float* __restrict__ lr_t, float mu) {
  __shared__ __attribute__((aligned(16))) float Fs[64 * SG_LD];
  __shared__ __attribute__((aligned(16))) float Ds[64 * SG_LD];
  const int kt = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  // the table entry of this k-tile: the last one with tile0 <= kt.  64 entries per round, one load per lane and a ballot (a
  // serial walk is a chain of dependent L2 loads - tens of microseconds in front of every tile)
  int hi = -1;
  for (int base = 0; base < nheads; base += 64) {
    const int i = base + lane;
    const bool le = i < nheads && heads[i].tile0 <= kt;
    hi += __popcll(__ballot(le));
  }
  hi = __builtin_amdgcn_readfirstlane(hi);
  const ProbeHead h = heads[hi];
  const int k0 = (kt - h.tile0) * 64, c0 = blockIdx.y * 64;
  const float lr = lr_t[h.lr_index];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // the stream: this lane's 64 bytes of W and of the momentum, requested before anything else
  const int cw = c0 + 16 * w + r;
  const bool own = cw < C;
  const int64_t woff = (int64_t)cw * h.K + k0 + 16 * q;
  f32x4 wv[4], mv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    wv[e] = own ? *(const f32x4*)(h.w + woff + 4 * e) : zero;
    mv[e] = own ? *(const f32x4*)(h.mw + woff + 4 * e) : zero;
  }

  const float* Fb = F + h.col0 + k0;
  const float* Db = dlogits + (int64_t)hi * B * C;
  const bool cvec = (C & 3) == 0;
  const int srow = tid >> 4, sc4 = (tid & 15) * 4;   // staging: 64 rows x 16 float4, 4 per thread
  const bool do_bias = k0 == 0 && tid < 64 && c0 + tid < C;
  float gb = 0.f, gbc = 0.f;
  f32x4 acc[4] = {zero, zero, zero, zero};
  for (int b0 = 0; b0 < B; b0 += 64) {
    f32x4 fr[4], dr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = b0 + srow + 16 * i;
      fr[i] = b < B ? *(const f32x4*)(Fb + (int64_t)b * ldf + sc4) : zero;
      const int c = c0 + sc4;
      dr[i] = zero;
      if (b < B) {
        const float* dp = Db + (int64_t)b * C + c;
        if (cvec) {
          if (c < C) dr[i] = *(const f32x4*)dp;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < C) dr[i][e] = dp[e];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(f32x4*)(Fs + (srow + 16 * i) * SG_LD + sc4) = fr[i];
      *(f32x4*)(Ds + (srow + 16 * i) * SG_LD + sc4) = dr[i];
    }
    __syncthreads();
    if (do_bias) {
      const int nb = min(64, B - b0);
      for (int b = 0; b < nb; ++b) {                    // row order, compensated
        const float y = Ds[b * SG_LD + tid] - gbc;
        const float u = gb + y;
        gbc = (u - gb) - y;
        gb = u;
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {             // 32 batch rows = one fmaf chain from zero, then added to the total
      f32x4 part[4] = {zero, zero, zero, zero};
#pragma unroll 4
      for (int s = 8 * half; s < 8 * half + 8; ++s) {
        const f32x4 a4 = *(const f32x4*)(Fs + (4 * s + q) * SG_LD + 4 * r);
        const float dv = Ds[(4 * s + q) * SG_LD + 16 * w + r];
#pragma unroll
        for (int t = 0; t < 4; ++t) part[t] = mfma16(a4[t], dv, part[t]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] += part[t];
    }
  }
  if (own) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f32x4 m = mv[e], p = wv[e];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        m[t] = __fmul_rn(mu, m[t]) + acc[t][e];        // buf.mul_(mu).add_(g): two roundings, as torch.optim.SGD
        p[t] = __builtin_fmaf(-lr, m[t], p[t]);        // p.add_(buf, alpha=-lr)
      }
      *(f32x4*)(h.mw + woff + 4 * e) = m;
      *(f32x4*)(h.w + woff + 4 * e) = p;
    }
  }
  if (do_bias) {
    const int c = c0 + tid;
    const float m = __fmul_rn(mu, h.mb[c]) + gb;
    h.mb[c] = m;
    h.b[c] = __builtin_fmaf(-lr, m, h.b[c]);
  }
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_probe_features(const void* const* cls, const int64_t* cls_ld, int n, const void* patch, int64_t patch_ld_b,
                         int64_t patch_ld_t, int dtype, int64_t B, int P, int D, float* F, int64_t ldf, void* stream) {
  if (!cls || !cls_ld || !patch || !F) return OCTIC_ENULL;
  if (n < 1 || n > 4 || B <= 0 || B > 65535 || P <= 0 || D <= 0 || D % 64 || ldf < (int64_t)(n + 1) * D) return OCTIC_ESHAPE;
  if (dtype != OCTIC_F32 && dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  FeatArgs a;
  for (int i = 0; i < 4; ++i) { a.cls[i] = nullptr; a.cls_ld[i] = 0; }
  for (int i = 0; i < n; ++i) {
    if (!cls[i]) return OCTIC_ENULL;
    if ((((uintptr_t)cls[i]) & 15) || (cls_ld[i] & 7)) return OCTIC_EALIGN;
    a.cls[i] = cls[i];
    a.cls_ld[i] = cls_ld[i];
  }
  if ((((uintptr_t)patch) & 15) || (((uintptr_t)F) & 15) || (patch_ld_b & 7) || (patch_ld_t & 7) || (ldf & 3)) return OCTIC_EALIGN;
  a.patch = patch; a.ld_b = patch_ld_b; a.ld_t = patch_ld_t;
  a.n = n; a.P = P; a.D = D; a.F = F; a.ldf = ldf;
  const dim3 grid((unsigned)((D / 4 + 255) / 256), (unsigned)B);
  if (dtype == OCTIC_BF16)
    probe_features_kernel<bf16><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else
    probe_features_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

static int probe_check(const void* heads, int nheads, const float* F, int64_t ldf, int B, int C) {
  if (!heads || !F) return OCTIC_ENULL;
  if (nheads <= 0 || nheads > 65535 || B <= 0 || C <= 0 || ldf <= 0) return OCTIC_ESHAPE;
  if ((int64_t)nheads * B * C > 0x7FFFFFFFll * 4) return OCTIC_ESHAPE;
  if ((((uintptr_t)F) & 15) || (ldf & 3)) return OCTIC_EALIGN;
  return OCTIC_OK;
}

int octic_probe_forward(const octic_probe_head* heads, int nheads, const float* F, int64_t ldf, int B, int C, float* logits,
                        void* stream) {
  if (int e = probe_check(heads, nheads, F, ldf, B, C)) return e;
  if (!logits) return OCTIC_ENULL;
  const dim3 grid((unsigned)((C + 63) / 64), (unsigned)nheads, (unsigned)((B + 127) / 128));
  if (grid.z > 65535) return OCTIC_ESHAPE;
  probe_forward_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(heads, F, ldf, B, C, logits);
  return launch_status();
}

int octic_probe_ce(const float* logits, const int64_t* labels, int nheads, int B, int C, float* dlogits, float* rowloss,
                   int* rowrank, float* loss_mean, float* loss_sum, int* topk, void* stream) {
  if (!logits || !labels || !rowloss || !rowrank) return OCTIC_ENULL;
  if (nheads <= 0 || B <= 0 || C <= 0 || (int64_t)nheads * B > 0x7FFFFFFF) return OCTIC_ESHAPE;
  probe_ce_kernel<<<dim3((unsigned)(nheads * B)), 256, 0, (hipStream_t)stream>>>(logits, labels, B, C, dlogits, rowloss, rowrank);
  probe_ce_finish_kernel<<<dim3((unsigned)nheads), 64, 0, (hipStream_t)stream>>>(rowloss, rowrank, B, loss_mean, loss_sum, topk);
  return launch_status();
}

int octic_probe_sgd(const octic_probe_head* heads, int nheads, int total_ktiles, const float* F, int64_t ldf,
                    const float* dlogits, int B, int C, const float* lr, float momentum, void* stream) {
  if (int e = probe_check(heads, nheads, F, ldf, B, C)) return e;
  if (!dlogits || !lr) return OCTIC_ENULL;
  if (total_ktiles < nheads) return OCTIC_ESHAPE;
  if ((C % 4) == 0 && (((uintptr_t)dlogits) & 15)) return OCTIC_EALIGN;
  const dim3 grid((unsigned)total_ktiles, (unsigned)((C + 63) / 64));
  if (grid.y > 65535) return OCTIC_ESHAPE;
  probe_sgd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(heads, nheads, F, ldf, dlogits, B, C, lr, momentum);
  return launch_status();
}

}  // extern "C"
