// Row kernels of the DINOv2 objective on the prototype axis (K = 65 536 in the recipe): the teacher's centred softmax
// (dinov2/loss/dino_clstoken_loss.py:43-51, ibot_patch_loss.py:63-77) and the soft-target cross entropy
// -sum_k t_k log_softmax(s / temp)_k with its gradient (dino_clstoken_loss.py:78-92, ibot_patch_loss.py:26-34).
// HBM-bound by construction: the eager composition walks the [rows, K] logits nine times in f32 (subtract, divide, softmax,
// divide, log_softmax, multiply, sum, and the two backward passes); here the teacher's probabilities cost one read (+ one
// re-read that hits L2 / MALL) and one write, the cross entropy ONE read of the student logits and the probabilities, its
// gradient one read of each and one write.  One workgroup per row, 16-byte loads, online max / sum (no second pass for the
// log-sum-exp), f32 arithmetic throughout (expf / logf of the device library, not the fast intrinsics); the student logits are taken in their storage dtype (bf16 under autocast: the
// reference divides by the temperature in bf16 first - this path skips that rounding).  The teacher's other centering, the
// Sinkhorn-Knopp targets (dino_clstoken_loss.py:53-76, ibot_patch_loss.py:79-116), is the second half of this file.
#include "octic_common.hpp"

namespace octic {

constexpr int SL_THREADS = 512;

struct MaxSum { float m, e; };
__device__ __forceinline__ void ms_add8(MaxSum& a, const float v[8]) {
  float mx = v[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) mx = fmaxf(mx, v[i]);
  if (mx > a.m) { a.e *= expf(a.m - mx); a.m = mx; }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += expf(v[i] - a.m);
  a.e += s;
}
// workgroup-wide combine of per-thread (max, sum of exp relative to it); every thread gets the result.  scale: the maxima are
// in units of 1 / scale of the exponent (the Sinkhorn passes keep them as logits; 1 elsewhere, where x * 1.f is x)
__device__ __forceinline__ MaxSum ms_block(MaxSum a, float* red, float scale = 1.f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = SL_THREADS / 64;
  float m = a.m;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  const float e = wave_total(a.e * (a.m == -INFINITY ? 0.f : expf((a.m - m) * scale)));
  if (lane == 0) { red[2 * w] = m; red[2 * w + 1] = e; }
  __syncthreads();
  float M = red[0];
  for (int i = 1; i < nw; ++i) M = fmaxf(M, red[2 * i]);
  float E = 0.f;
  for (int i = 0; i < nw; ++i) E += red[2 * i + 1] * (red[2 * i] == -INFINITY ? 0.f : expf((red[2 * i] - M) * scale));
  __syncthreads();
  return MaxSum{M, E};
}
__device__ __forceinline__ float sum_block(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = SL_THREADS / 64;
  v = wave_total(v);
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < nw; ++i) s += red[i];
  __syncthreads();
  return s;
}

// out[r, :] = softmax((t[r, :] - center) * inv_temp)
template <typename TS>
__global__ __launch_bounds__(SL_THREADS) void softmax_center_kernel(const TS* __restrict__ t, int64_t ldt,
                                                                     const float* __restrict__ center, float inv_temp,
                                                                     float* __restrict__ out, int K) {
  __shared__ float red[2 * SL_THREADS / 64];
  const int64_t r = blockIdx.x;
  const TS* tr = t + r * ldt;
  float* o = out + r * (int64_t)K;
  MaxSum a{-INFINITY, 0.f};
  for (int k = threadIdx.x * 8; k < K; k += SL_THREADS * 8) {
    float v[8], c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    load8<TS>(tr + k, v);
    if (center) load8<float>(center + k, c);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (v[i] - c[i]) * inv_temp;
    ms_add8(a, v);
  }
  const MaxSum A = ms_block(a, red);
  const float inv = 1.0f / A.e;
  for (int k = threadIdx.x * 8; k < K; k += SL_THREADS * 8) {
    float v[8], c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    load8<TS>(tr + k, v);
    if (center) load8<float>(center + k, c);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = expf((v[i] - c[i]) * inv_temp - A.m) * inv;
    store8<float>(o + k, v);
  }
}

// loss[r] = tsum lse - sum_k t_k z_k,  z = s[r, :] * inv_temp,  lse = log sum exp z,  t = tprob[r % t_rows, :]
template <typename TS>
__global__ __launch_bounds__(SL_THREADS) void soft_ce_fwd_kernel(const TS* __restrict__ s, int64_t lds_,
                                                                  const float* __restrict__ tprob, int64_t t_rows,
                                                                  float inv_temp, float* __restrict__ loss,
                                                                  float* __restrict__ lse, float* __restrict__ tsum, int K) {
  __shared__ float red[2 * SL_THREADS / 64];
  const int64_t r = blockIdx.x;
  const TS* sr = s + r * lds_;
  const float* tr = tprob + (r % t_rows) * (int64_t)K;
  MaxSum a{-INFINITY, 0.f};
  float dot = 0.f, ts = 0.f;
  for (int k = threadIdx.x * 8; k < K; k += SL_THREADS * 8) {
    float v[8], t[8];
    load8<TS>(sr + k, v);
    load8<float>(tr + k, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] *= inv_temp;
      dot = __builtin_fmaf(t[i], v[i], dot);
      ts += t[i];
    }
    ms_add8(a, v);
  }
  const MaxSum A = ms_block(a, red);
  dot = sum_block(dot, red);
  ts = sum_block(ts, red);
  if (threadIdx.x == 0) {
    const float l = A.m + logf(A.e);
    lse[r] = l;
    tsum[r] = ts;
    loss[r] = ts * l - dot;
  }
}

// ds[r, k] = g[r] inv_temp (exp(z_k - lse[r]) tsum[r] - t_k)
template <typename TS>
__global__ __launch_bounds__(SL_THREADS) void soft_ce_bwd_kernel(const TS* __restrict__ s, int64_t lds_,
                                                                  const float* __restrict__ tprob, int64_t t_rows,
                                                                  float inv_temp, const float* __restrict__ g,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ tsum, TS* __restrict__ ds,
                                                                  int64_t ldd, int K) {
  const int64_t r = blockIdx.x;
  const TS* sr = s + r * lds_;
  const float* tr = tprob + (r % t_rows) * (int64_t)K;
  TS* dr = ds + r * ldd;
  const float gr = g[r] * inv_temp, l = lse[r], ts = tsum[r];
  for (int k = threadIdx.x * 8; k < K; k += SL_THREADS * 8) {
    float v[8], t[8];
    load8<TS>(sr + k, v);
    load8<float>(tr + k, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = gr * (expf(v[i] * inv_temp - l) * ts - t[i]);
    store8<TS>(dr + k, v);
  }
}

static int sl_check(int64_t rows, int K, int64_t ld) {
  if (rows < 0 || K <= 0) return OCTIC_ESHAPE;
  if (K % 8 || ld % 8 || ld < K) return OCTIC_ESHAPE;
  if (rows > 0x7FFFFFFF) return OCTIC_ESHAPE;
  return OCTIC_OK;
}

// ---- Sinkhorn-Knopp teacher targets (dinov2/loss/dino_clstoken_loss.py:53-76, ibot_patch_loss.py:79-116) --------------------
// With E[b, k] = exp((x[b, k] - mx[b]) * inv_temp) (mx[b] the row's own maximum logit: a per-row factor of E is absorbed by
// v[b] below; the subtraction comes first, in the logits' own scale, where it is exact or nearly so - x * inv_temp alone is
// rounded at its full magnitude, 1e-5 of exp() at a few hundred), every state of the reference's Q is E[b, k] u[k] v[b], so Q
// is never stored:
//   r[k] = sum_b E[b, k] v[b]   (first round: v[b] = exp((mx[b] - m) inv_temp), m the maximum over all rows of all ranks: the
//                                reference's exp(x / temp) up to a constant; the caller all-reduces r)  sinkhorn_protos_kernel
//   u[k] = 1 / r[k],  c[b] = sum_k E[b, k] u[k],  v[b] = 1 / c[b]                                     sinkhorn_rows_kernel
//   out[b, k] = E[b, k] u[k] / c[b]  (c of the last round is summed by the same workgroup)            sinkhorn_final_kernel
// The reference's division by the total sum and its constants K and B cancel in out and are not applied.  No atomics: the row
// sum over samples is per-slab partials in a fixed order plus sinkhorn_finish_kernel, so two calls are bitwise equal.
constexpr int SK_THREADS = 256;              // prototype-sum pass: 8 columns a thread, SK_COLS columns a workgroup
constexpr int SK_COLS = SK_THREADS * 8;
constexpr int SK_SLAB_ROWS = 32;             // rows of one slab, until the slab count reaches SK_MAX_SLABS
constexpr int SK_MAX_SLABS = 256;

struct SkPlan { int slabs; int64_t rows_per_slab; };
static SkPlan sk_plan(int64_t rows) {
  int64_t rps = (rows + SK_MAX_SLABS - 1) / SK_MAX_SLABS;
  if (rps < SK_SLAB_ROWS) rps = SK_SLAB_ROWS;
  return SkPlan{(int)((rows + rps - 1) / rps), rps};
}

// dst[slab, k] = sum over the slab's rows b of weight[b] exp((x[b, k] - shift[b]) inv_temp)
template <typename TS>
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_protos_kernel(const TS* __restrict__ x, int64_t ld, float inv_temp,
                                                                      const float* __restrict__ shift,
                                                                      const float* __restrict__ weight,
                                                                      float* __restrict__ dst, int64_t rows,
                                                                      int64_t rows_per_slab, int K) {
  const int k = (blockIdx.x * SK_THREADS + threadIdx.x) * 8;
  if (k >= K) return;
  const int64_t r0 = blockIdx.y * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
  for (int64_t r = r0; r < r1; ++r) {
    float v[8];
    load8<TS>(x + r * ld + k, v);
    const float sh = shift[r], w = weight[r];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(w, expf((v[i] - sh) * inv_temp), acc[i]);
  }
  store8<float>(dst + blockIdx.y * (int64_t)K + k, acc);
}

// r[k] = sum_s part[s, k], slabs in index order
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_finish_kernel(const float* __restrict__ part, int slabs,
                                                                      float* __restrict__ r, int K) {
  const int k = blockIdx.x * SK_THREADS + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int i = 0; i < slabs; ++i) s += part[i * (int64_t)K + k];
  r[k] = s;
}

// one row: (mx = max_k x_k, sum_k u_k exp((x_k - mx) inv_temp)), u = 1 where it is null; every thread gets the result
template <typename TS>
__device__ __forceinline__ MaxSum sk_row_stats(const TS* __restrict__ xr, float inv_temp, const float* __restrict__ u, int K,
                                               float* red) {
  MaxSum a{-INFINITY, 0.f};
  for (int k = threadIdx.x * 8; k < K; k += SL_THREADS * 8) {
    float v[8], w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    load8<TS>(xr + k, v);
    if (u) load8<float>(u + k, w);
    float mx = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) mx = fmaxf(mx, v[i]);
    if (mx > a.m) { a.e *= expf((a.m - mx) * inv_temp); a.m = mx; }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = __builtin_fmaf(w[i], expf((v[i] - a.m) * inv_temp), s);
    a.e += s;
  }
  return ms_block(a, red, inv_temp);      // the maxima are logits: the partial sums meet at exp((m_i - M) inv_temp)
}

template <typename TS>
__global__ __launch_bounds__(SL_THREADS) void sinkhorn_rows_kernel(const TS* __restrict__ x, int64_t ld, float inv_temp,
                                                                    const float* __restrict__ u, float* __restrict__ rowmax,
                                                                    float* __restrict__ c, int K) {
  __shared__ float red[2 * SL_THREADS / 64];
  const int64_t r = blockIdx.x;
  const MaxSum A = sk_row_stats<TS>(x + r * ld, inv_temp, u, K, red);
  if (threadIdx.x == 0) {
    rowmax[r] = A.m;
    c[r] = A.e;
  }
}

template <typename TS>
__global__ __launch_bounds__(SL_THREADS) void sinkhorn_final_kernel(const TS* __restrict__ x, int64_t ld, float inv_temp,
                                                                     const float* __restrict__ u, float* __restrict__ out,
                                                                     int K) {
  __shared__ float red[2 * SL_THREADS / 64];
  const int64_t r = blockIdx.x;
  const TS* xr = x + r * ld;
  float* o = out + r * (int64_t)K;
  const MaxSum A = sk_row_stats<TS>(xr, inv_temp, u, K, red);
  const float inv = 1.0f / A.e;
  for (int k = threadIdx.x * 8; k < K; k += SL_THREADS * 8) {
    float v[8], w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    load8<TS>(xr + k, v);
    if (u) load8<float>(u + k, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = expf((v[i] - A.m) * inv_temp) * w[i] * inv;
    store8<float>(o + k, v);
  }
}

static bool sk_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
// the logits of every Sinkhorn pass: x non-null, f32 / bf16, rows >= 1, K % 8 == 0, rows of ld >= K elements on 16-byte
// boundaries
static int sk_check(const void* x, int dtype, int64_t ld, float inv_temp, int64_t rows, int K) {
  if (!x) return OCTIC_ENULL;
  if (dtype != OCTIC_BF16 && dtype != OCTIC_F32) return OCTIC_EDTYPE;
  if (rows < 1 || rows > 0x7FFFFFFF || K <= 0 || K % 8 || ld < K) return OCTIC_ESHAPE;
  if (!(inv_temp > 0.f)) return OCTIC_ESHAPE;          // the row maximum of x is the row maximum of x * inv_temp
  if (sk_misaligned(x) || ((ld * elem_size(dtype)) & 15)) return OCTIC_EALIGN;
  return OCTIC_OK;
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_softmax_center(const void* t, int t_dtype, int64_t ldt, const float* center, float inv_temp, float* out,
                         int64_t rows, int K, void* stream) {
  if (rows == 0) return OCTIC_OK;
  if (!t || !out) return OCTIC_ENULL;
  if (int e = sl_check(rows, K, ldt)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (t_dtype == OCTIC_BF16)
    softmax_center_kernel<bf16><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const bf16*)t, ldt, center, inv_temp, out, K);
  else if (t_dtype == OCTIC_F32)
    softmax_center_kernel<float><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const float*)t, ldt, center, inv_temp, out, K);
  else
    return OCTIC_EDTYPE;
  return launch_status();
}

int octic_soft_ce_fwd(const void* s, int s_dtype, int64_t lds, const float* tprob, int64_t t_rows, float inv_temp,
                      float* loss, float* lse, float* tsum, int64_t rows, int K, void* stream) {
  if (rows == 0) return OCTIC_OK;
  if (!s || !tprob || !loss || !lse || !tsum) return OCTIC_ENULL;
  if (int e = sl_check(rows, K, lds)) return e;
  if (t_rows <= 0) return OCTIC_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (s_dtype == OCTIC_BF16)
    soft_ce_fwd_kernel<bf16><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const bf16*)s, lds, tprob, t_rows, inv_temp, loss, lse, tsum, K);
  else if (s_dtype == OCTIC_F32)
    soft_ce_fwd_kernel<float><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const float*)s, lds, tprob, t_rows, inv_temp, loss, lse, tsum, K);
  else
    return OCTIC_EDTYPE;
  return launch_status();
}

int octic_soft_ce_bwd(const void* s, int s_dtype, int64_t lds, const float* tprob, int64_t t_rows, float inv_temp,
                      const float* g, const float* lse, const float* tsum, void* ds, int64_t ldd, int64_t rows, int K,
                      void* stream) {
  if (rows == 0) return OCTIC_OK;
  if (!s || !tprob || !g || !lse || !tsum || !ds) return OCTIC_ENULL;
  if (int e = sl_check(rows, K, lds)) return e;
  if (int e = sl_check(rows, K, ldd)) return e;
  if (t_rows <= 0) return OCTIC_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (s_dtype == OCTIC_BF16)
    soft_ce_bwd_kernel<bf16><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const bf16*)s, lds, tprob, t_rows, inv_temp, g, lse, tsum, (bf16*)ds, ldd, K);
  else if (s_dtype == OCTIC_F32)
    soft_ce_bwd_kernel<float><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const float*)s, lds, tprob, t_rows, inv_temp, g, lse, tsum, (float*)ds, ldd, K);
  else
    return OCTIC_EDTYPE;
  return launch_status();
}

int octic_sinkhorn_slabs(int64_t rows) {
  if (rows < 1 || rows > 0x7FFFFFFF) return OCTIC_ESHAPE;
  return sk_plan(rows).slabs;
}

int octic_sinkhorn_protos(const void* x, int x_dtype, int64_t ldx, float inv_temp, const float* shift, const float* weight,
                          float* partials, float* r, int64_t rows, int K, void* stream) {
  if (int e = sk_check(x, x_dtype, ldx, inv_temp, rows, K)) return e;
  const SkPlan p = sk_plan(rows);
  if (!shift || !weight || !r || (p.slabs > 1 && !partials)) return OCTIC_ENULL;
  if (sk_misaligned(r) || (p.slabs > 1 && sk_misaligned(partials))) return OCTIC_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  float* dst = p.slabs > 1 ? partials : r;
  const dim3 grid((unsigned)((K + SK_COLS - 1) / SK_COLS), (unsigned)p.slabs);
  if (x_dtype == OCTIC_BF16)
    sinkhorn_protos_kernel<bf16><<<grid, dim3(SK_THREADS), 0, st>>>((const bf16*)x, ldx, inv_temp, shift, weight, dst, rows, p.rows_per_slab, K);
  else
    sinkhorn_protos_kernel<float><<<grid, dim3(SK_THREADS), 0, st>>>((const float*)x, ldx, inv_temp, shift, weight, dst, rows, p.rows_per_slab, K);
  if (p.slabs > 1)
    sinkhorn_finish_kernel<<<dim3((unsigned)((K + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS), 0, st>>>(partials, p.slabs, r, K);
  return launch_status();
}

int octic_sinkhorn_rows(const void* x, int x_dtype, int64_t ldx, float inv_temp, const float* u, float* rowmax, float* c,
                        int64_t rows, int K, void* stream) {
  if (int e = sk_check(x, x_dtype, ldx, inv_temp, rows, K)) return e;
  if (!rowmax || !c) return OCTIC_ENULL;
  if (sk_misaligned(u)) return OCTIC_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == OCTIC_BF16)
    sinkhorn_rows_kernel<bf16><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const bf16*)x, ldx, inv_temp, u, rowmax, c, K);
  else
    sinkhorn_rows_kernel<float><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const float*)x, ldx, inv_temp, u, rowmax, c, K);
  return launch_status();
}

int octic_sinkhorn_final(const void* x, int x_dtype, int64_t ldx, float inv_temp, const float* u, float* out, int64_t rows,
                         int K, void* stream) {
  if (int e = sk_check(x, x_dtype, ldx, inv_temp, rows, K)) return e;
  if (!out) return OCTIC_ENULL;
  if (sk_misaligned(u) || sk_misaligned(out)) return OCTIC_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == OCTIC_BF16)
    sinkhorn_final_kernel<bf16><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const bf16*)x, ldx, inv_temp, u, out, K);
  else
    sinkhorn_final_kernel<float><<<dim3((unsigned)rows), dim3(SL_THREADS), 0, st>>>((const float*)x, ldx, inv_temp, u, out, K);
  return launch_status();
}

}  // extern "C"
