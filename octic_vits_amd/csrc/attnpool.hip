// Attentive-probe evaluation (dinov2/eval/segmentation/eval_classification.py): the grid of AttnPoolClassifier heads - one
// learned query token, kv = nn.Linear(D, 2D) over all B x N patch tokens, SDPA with D / 64 heads of 64, nn.Linear(D, C) -
// trained together on a frozen backbone.  The query is ONE token, so keys and values are never formed: with Wk = kv.weight[:D],
// Wv = kv.weight[D:], head h owning rows 64h .. 64h+63 and scale = 1/8,
//   U[gH+h, :]  = scale sum_j q_g[64h+j] Wk_g[64h+j, :]          ap_fold_kernel      (the query folded through Wk)
//   S           = X U^T                                           octic_dense_f32_nt  (all classifiers in one product)
//   P[b, :, c]  = softmax over the N tokens of image b            ap_softmax_kernel   (the key bias is constant in n: it cancels)
//   Z[b, c, :]  = sum_n P[b, n, c] X[b, n, :]                     ap_gemm_kernel      (batched TN per image)
//   pooled[b, g, 64h+j] = Wv_g[64h+j, :] . Z[b, gH+h, :] + bv_g   ap_gemm_kernel      (grouped, GH groups)
// and the backward has the same shapes.  Per-classifier operands come from DEVICE arrays of G pointers (the classifiers'
// parameters and gradients are views of flat buffers; the host cannot see the arrays, so their contents are the caller's to
// keep 16-byte aligned).  Exact f32 throughout (v_mfma_f32_16x16x4_f32), no atomics, every sum in a fixed order.
#include "octic_common.hpp"

namespace octic {

__device__ __forceinline__ f32x4 ap_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ the one GEMM kernel
// C_z[m, n] = alpha sum_k A_z[m, k] B_z[k, n] (+ bias_z[n]) for z = z1 Z2 + z2: every operand is a base (a pointer, or entry
// z1 of a device pointer array) plus z1 / z2 offsets, with element strides per index, so NT, NN, TN, batched and grouped
// products are one kernel.  Workgroup = 64 x 64 of C, k in chunks of 16 through LDS (both tiles k-contiguous, rows of 20
// floats); wave w owns rows 16w .. 16w+15.  A lane reads 4 consecutive k of its row and feeds them to 4 MFMA steps: an
// element of C is ONE chain from +0 over k in chunks of 16 ascending, step e of a chunk adding k = e, 4 + e, 8 + e, 12 + e -
// a function of K alone, so a row of C does not depend on M, on its tile or on the other rows.  Global loads follow the
// operand's unit-stride axis (4 elements per thread, one 16-byte load where the address allows it); everything past an M, N
// or K edge is read as zero and never written.
constexpr int AP_LD = 20;

struct ApGemm {
  const float* A; const float* const* Atab; int64_t a_z1, a_z2, a_m, a_k;
  const float* B; const float* const* Btab; int64_t b_z1, b_z2, b_k, b_n;
  float* C; float* const* Ctab; int64_t c_z1, c_z2, c_m;
  const float* const* biastab; int64_t bias_z2;
  int M, N, K, Z2;
  float alpha;
};

// 4 elements of a 64 x 16 tile for this thread: `kc` = the k axis has unit stride (thread = row i, k kk .. kk+3), otherwise
// thread = k kk, rows i .. i+3 with stride s_i
__device__ __forceinline__ void ap_fetch(const float* base, bool kc, int64_t s_i, int64_t s_k, int i, int kk, int I, int K,
                                         float v[4]) {
  const float* p = base + (int64_t)i * s_i + (int64_t)kk * s_k;
  if (kc) {
    if (i < I && kk + 3 < K && !(((uintptr_t)p) & 15)) {
      const f32x4 t = *(const f32x4*)p;
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (i < I && kk + e < K) ? p[e] : 0.f;
    }
  } else {
    if (s_i == 1 && kk < K && i + 3 < I && !(((uintptr_t)p) & 15)) {
      const f32x4 t = *(const f32x4*)p;
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (kk < K && i + e < I) ? p[(int64_t)e * s_i] : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void ap_gemm_kernel(ApGemm a) {
  __shared__ __attribute__((aligned(16))) float As[64 * AP_LD];
  __shared__ __attribute__((aligned(16))) float Bs[64 * AP_LD];
  const int z = blockIdx.z, z1 = z / a.Z2, z2 = z - z1 * a.Z2;
  const float* A = (a.Atab ? a.Atab[z1] : a.A) + z1 * a.a_z1 + z2 * a.a_z2;
  const float* B = (a.Btab ? a.Btab[z1] : a.B) + z1 * a.b_z1 + z2 * a.b_z2;
  float* C = (a.Ctab ? a.Ctab[z1] : a.C) + z1 * a.c_z1 + z2 * a.c_z2;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const bool akc = a.a_k == 1, bkc = a.b_k == 1;
  const int ai = akc ? tid >> 2 : (tid & 15) * 4, ak = akc ? (tid & 3) * 4 : tid >> 4;
  const int bi = bkc ? tid >> 2 : (tid & 15) * 4, bk = bkc ? (tid & 3) * 4 : tid >> 4;
  float ar[4], br[4];
  auto fetch = [&](int k0) {
    ap_fetch(A + (int64_t)m0 * a.a_m + (int64_t)k0 * a.a_k, akc, a.a_m, a.a_k, ai, ak, a.M - m0, a.K - k0, ar);
    ap_fetch(B + (int64_t)n0 * a.b_n + (int64_t)k0 * a.b_k, bkc, a.b_n, a.b_k, bi, bk, a.N - n0, a.K - k0, br);
  };
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero, zero, zero, zero};
  fetch(0);
  for (int k0 = 0; k0 < a.K; k0 += 16) {
    __syncthreads();                       // the previous chunk's reads are done
    if (akc) *(f32x4*)(As + ai * AP_LD + ak) = f32x4{ar[0], ar[1], ar[2], ar[3]};
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) As[(ai + e) * AP_LD + ak] = ar[e];
    }
    if (bkc) *(f32x4*)(Bs + bi * AP_LD + bk) = f32x4{br[0], br[1], br[2], br[3]};
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) Bs[(bi + e) * AP_LD + bk] = br[e];
    }
    __syncthreads();
    if (k0 + 16 < a.K) fetch(k0 + 16);     // in flight under the products
    const f32x4 a4 = *(const f32x4*)(As + (16 * w + r) * AP_LD + 4 * q);
    f32x4 b4[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) b4[ct] = *(const f32x4*)(Bs + (16 * ct + r) * AP_LD + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = ap_mfma16(a4[e], b4[ct][e], acc[ct]);
  }
  const float* bias = a.biastab ? a.biastab[z1] + z2 * a.bias_z2 : nullptr;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int n = n0 + 16 * ct + r;
    if (n >= a.N) continue;
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + 16 * w + 4 * q + e;
      if (m < a.M) C[(int64_t)m * a.c_m + n] = bias ? a.alpha * acc[ct][e] + bv : a.alpha * acc[ct][e];
    }
  }
}

static int ap_launch(const ApGemm& a, int64_t Z, void* stream) {
  const int64_t gx = (a.N + 63) / 64, gy = (a.M + 63) / 64;
  if (gy > 65535 || Z > 65535 || gx > 0x7FFFFFFF) return OCTIC_ESHAPE;
  ap_gemm_kernel<<<dim3((unsigned)gx, (unsigned)gy, (unsigned)Z), 256, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

static ApGemm ap_args() {
  ApGemm a;
  a.A = nullptr; a.Atab = nullptr; a.a_z1 = a.a_z2 = 0; a.a_m = a.a_k = 0;
  a.B = nullptr; a.Btab = nullptr; a.b_z1 = a.b_z2 = 0; a.b_k = a.b_n = 0;
  a.C = nullptr; a.Ctab = nullptr; a.c_z1 = a.c_z2 = 0; a.c_m = 0;
  a.biastab = nullptr; a.bias_z2 = 0;
  a.M = a.N = a.K = 0; a.Z2 = 1; a.alpha = 1.0f;
  return a;
}

// ------------------------------------------------------------------------------------------------ fold / unfold
// U[gH+h, d] = scale sum_j q_g[64h+j] Wk_g[64h+j, d], j ascending, one fmaf chain; rows GH .. rows-1 are written as zero (the
// padding of GH to the multiple of 4 the scores product needs).  Reads every Wk once.
__global__ __launch_bounds__(256) void ap_fold_kernel(const float* const* __restrict__ q, const float* const* __restrict__ wk,
                                                      int GH, int H, int D, float* __restrict__ U) {
  const int row = blockIdx.x, d = blockIdx.y * 256 + threadIdx.x;
  if (d >= D) return;
  float u = 0.f;
  if (row < GH) {
    const int g = row / H, h = row - g * H;
    const float* qg = q[g] + 64 * h;
    const float* w = wk[g] + (int64_t)64 * h * D + d;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) u = fmaf(qg[j], w[(int64_t)j * D], u);
    u *= 0.125f;
  }
  U[(int64_t)row * D + d] = u;
}

// one workgroup per row r = 64h+j of classifier g: dWk_g[r, :] = scale q_g[r] dU[gH+h, :], dq_g[r] = scale Wk_g[r, :] . dU[gH+h, :]
// (per thread d = t, t + 256, ... ascending, then the wave totals, then waves 0 .. 3), dbk_g[r] = 0.
__global__ __launch_bounds__(256) void ap_unfold_kernel(const float* const* __restrict__ q, const float* const* __restrict__ wk,
                                                        const float* __restrict__ dU, int H, int D, float* const* __restrict__ dq,
                                                        float* const* __restrict__ dwk, float* const* __restrict__ dbk) {
  __shared__ float red[4];
  const int g = blockIdx.x / D, r = blockIdx.x - g * D;
  const float* du = dU + ((int64_t)g * H + (r >> 6)) * D;
  const float* w = wk[g] + (int64_t)r * D;
  float* dw = dwk[g] + (int64_t)r * D;
  const float qs = 0.125f * q[g][r];
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float v = du[d];
    dw[d] = qs * v;
    s = fmaf(w[d], v, s);
  }
  s = wave_total(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    dq[g][r] = 0.125f * (((red[0] + red[1]) + red[2]) + red[3]);
    dbk[g][r] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ token softmax
// workgroup = 64 columns of one image x 4 token lanes (lane y takes tokens y, y + 4, ...); maxima and sums meet in LDS in
// lane order.  exp2 domain, maximum subtracted: finite for any finite scores; N = 1 gives exp2(0) / 1 = 1 exactly.
constexpr float AP_LOG2E = 1.44269504088896340736f;

__global__ __launch_bounds__(256) void ap_softmax_kernel(float* __restrict__ S, int64_t lds, int N, int GH) {
  __shared__ float red[4][64];
  const int cx = threadIdx.x & 63, y = threadIdx.x >> 6, c = blockIdx.x * 64 + cx;
  const bool live = c < GH, pad = c >= GH && c < lds;
  float* s = S + (int64_t)blockIdx.y * N * lds + c;
  float m = -INFINITY;
  if (live)
    for (int n = y; n < N; n += 4) m = fmaxf(m, s[(int64_t)n * lds]);
  red[y][cx] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][cx], red[1][cx]), fmaxf(red[2][cx], red[3][cx]));
  __syncthreads();
  float sum = 0.f;
  if (live)
    for (int n = y; n < N; n += 4) sum += exp2f((s[(int64_t)n * lds] - m) * AP_LOG2E);
  red[y][cx] = sum;
  __syncthreads();
  sum = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
  if (live)
    for (int n = y; n < N; n += 4) s[(int64_t)n * lds] = exp2f((s[(int64_t)n * lds] - m) * AP_LOG2E) / sum;
  else if (pad)
    for (int n = y; n < N; n += 4) s[(int64_t)n * lds] = 0.f;
}

// dS = P (dP - sum_n P dP), in place on dP; same workgroup shape and summation order as the forward
__global__ __launch_bounds__(256) void ap_softmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, int64_t lds,
                                                             int N, int GH) {
  __shared__ float red[4][64];
  const int cx = threadIdx.x & 63, y = threadIdx.x >> 6, c = blockIdx.x * 64 + cx;
  const bool live = c < GH, pad = c >= GH && c < lds;
  const int64_t base = (int64_t)blockIdx.y * N * lds + c;
  const float* p = P + base;
  float* d = dP + base;
  float t = 0.f;
  if (live)
    for (int n = y; n < N; n += 4) t = fmaf(p[(int64_t)n * lds], d[(int64_t)n * lds], t);
  red[y][cx] = t;
  __syncthreads();
  t = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
  if (live)
    for (int n = y; n < N; n += 4) d[(int64_t)n * lds] = p[(int64_t)n * lds] * (d[(int64_t)n * lds] - t);
  else if (pad)
    for (int n = y; n < N; n += 4) d[(int64_t)n * lds] = 0.f;
}

// dst_g[c] = alpha sum_r src[g group_stride + r ld + c], r ascending
__global__ __launch_bounds__(256) void ap_colsum_kernel(const float* __restrict__ src, int64_t group_stride, int64_t ld, int rows,
                                                        int cols, float alpha, float* const* __restrict__ dst) {
  const int c = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  if (c >= cols) return;
  const float* s = src + (int64_t)g * group_stride + c;
  float t = 0.f;
  for (int r = 0; r < rows; ++r) t += s[(int64_t)r * ld];
  dst[g][c] = alpha * t;
}

static inline bool ap_mis(const void* p) { return (((uintptr_t)p) & 15) != 0; }
static inline bool ap_dims(int64_t B, int64_t G, int64_t D) {
  return B >= 1 && B <= 65535 && G >= 1 && G <= 1024 && D >= 64 && D % 64 == 0 && D <= 16384;
}

}  // namespace octic

using namespace octic;

int octic_attnpool_fold(const float* const* q, const float* const* wk, int G, int D, float* U, int64_t rows, void* stream) {
  if (!q || !wk || !U) return OCTIC_ENULL;
  if (!ap_dims(1, G, D) || rows < (int64_t)G * (D / 64) || rows > (int64_t)G * (D / 64) + 3) return OCTIC_ESHAPE;
  if (ap_mis(q) || ap_mis(wk) || ap_mis(U)) return OCTIC_EALIGN;
  ap_fold_kernel<<<dim3((unsigned)rows, (unsigned)((D + 255) / 256)), 256, 0, (hipStream_t)stream>>>(q, wk, G * (D / 64), D / 64, D, U);
  return launch_status();
}

int octic_attnpool_softmax(float* S, int64_t lds, int64_t B, int N, int GH, void* stream) {
  if (!S) return OCTIC_ENULL;
  if (B < 1 || B > 65535 || N < 1 || GH < 1 || lds < GH || lds > (int64_t)1 << 20 || B * N * lds > (int64_t)1 << 40) return OCTIC_ESHAPE;
  if (ap_mis(S) || (lds & 3)) return OCTIC_EALIGN;
  ap_softmax_kernel<<<dim3((unsigned)((lds + 63) / 64), (unsigned)B), 256, 0, (hipStream_t)stream>>>(S, lds, N, GH);
  return launch_status();
}

int octic_attnpool_pool(const float* P, int64_t ldp, const float* X, int64_t ldx, int64_t B, int N, int D, int GH, float* Z,
                        void* stream) {
  if (!P || !X || !Z) return OCTIC_ENULL;
  if (!ap_dims(B, 1, D) || N < 1 || GH < 1 || ldp < GH || ldx < D) return OCTIC_ESHAPE;
  if (ap_mis(P) || ap_mis(X) || ap_mis(Z) || (ldp & 3) || (ldx & 3)) return OCTIC_EALIGN;
  ApGemm a = ap_args();
  a.A = P; a.a_z1 = (int64_t)N * ldp; a.a_m = 1; a.a_k = ldp;
  a.B = X; a.b_z1 = (int64_t)N * ldx; a.b_k = ldx; a.b_n = 1;
  a.C = Z; a.c_z1 = (int64_t)GH * D; a.c_m = D;
  a.M = GH; a.N = D; a.K = N;
  return ap_launch(a, B, stream);
}

int octic_attnpool_value(const float* Z, const float* const* wv, const float* const* bv, int B, int G, int D, float* pooled,
                         int64_t ldo, void* stream) {
  if (!Z || !wv || !bv || !pooled) return OCTIC_ENULL;
  if (!ap_dims(B, G, D) || ldo < (int64_t)G * D) return OCTIC_ESHAPE;
  if (ap_mis(Z) || ap_mis(wv) || ap_mis(bv) || ap_mis(pooled) || (ldo & 3)) return OCTIC_EALIGN;
  const int H = D / 64;
  ApGemm a = ap_args();
  a.A = Z; a.a_z1 = (int64_t)H * D; a.a_z2 = D; a.a_m = (int64_t)G * H * D; a.a_k = 1;
  a.Btab = wv; a.b_z2 = (int64_t)64 * D; a.b_k = 1; a.b_n = D;
  a.C = pooled; a.c_z1 = D; a.c_z2 = 64; a.c_m = ldo;
  a.biastab = bv; a.bias_z2 = 64;
  a.M = B; a.N = 64; a.K = D; a.Z2 = H;
  return ap_launch(a, (int64_t)G * H, stream);
}

int octic_attnpool_dinput(const float* dlogits, const float* const* w, int G, int B, int C, int D, float alpha, float* dF,
                          int64_t ldd, void* stream) {
  if (!dlogits || !w || !dF) return OCTIC_ENULL;
  if (!ap_dims(B, G, D) || C < 1 || ldd < (int64_t)G * D) return OCTIC_ESHAPE;
  if (ap_mis(dlogits) || ap_mis(w) || ap_mis(dF) || (ldd & 3)) return OCTIC_EALIGN;
  ApGemm a = ap_args();
  a.A = dlogits; a.a_z1 = (int64_t)B * C; a.a_m = C; a.a_k = 1;
  a.Btab = w; a.b_k = D; a.b_n = 1;
  a.C = dF; a.c_z1 = D; a.c_m = ldd;
  a.M = B; a.N = D; a.K = C; a.alpha = alpha;
  return ap_launch(a, G, stream);
}

int octic_attnpool_dweight(const float* dlogits, const float* F, int64_t ldf, int64_t col0, int64_t col_stride, int G, int B,
                           int C, int K, float alpha, float* const* dw, void* stream) {
  if (!dlogits || !F || !dw) return OCTIC_ENULL;
  if (!ap_dims(B, G, 64) || C < 1 || K < 1 || col0 < 0 || col_stride < 0 || ldf < col0 + (G - 1) * col_stride + K) return OCTIC_ESHAPE;
  if (ap_mis(dlogits) || ap_mis(F) || ap_mis(dw) || (ldf & 3) || (col0 & 3) || (col_stride & 3)) return OCTIC_EALIGN;
  ApGemm a = ap_args();
  a.A = dlogits; a.a_z1 = (int64_t)B * C; a.a_m = 1; a.a_k = C;
  a.B = F + col0; a.b_z1 = col_stride; a.b_k = ldf; a.b_n = 1;
  a.Ctab = dw; a.c_m = K;
  a.M = C; a.N = K; a.K = B; a.alpha = alpha;
  return ap_launch(a, G, stream);
}

int octic_attnpool_colsum(const float* src, int64_t group_stride, int64_t ld, int G, int rows, int cols, float alpha,
                          float* const* dst, void* stream) {
  if (!src || !dst) return OCTIC_ENULL;
  if (G < 1 || G > 65535 || rows < 1 || cols < 1 || ld < cols || group_stride < 0) return OCTIC_ESHAPE;
  if (ap_mis(src) || ap_mis(dst)) return OCTIC_EALIGN;
  ap_colsum_kernel<<<dim3((unsigned)((cols + 255) / 256), (unsigned)G), 256, 0, (hipStream_t)stream>>>(src, group_stride, ld, rows, cols,
                                                                                                      alpha, dst);
  return launch_status();
}

int octic_attnpool_dz(const float* dpooled, int64_t ldd, const float* const* wv, int B, int G, int D, float* dZ, void* stream) {
  if (!dpooled || !wv || !dZ) return OCTIC_ENULL;
  if (!ap_dims(B, G, D) || ldd < (int64_t)G * D) return OCTIC_ESHAPE;
  if (ap_mis(dpooled) || ap_mis(wv) || ap_mis(dZ) || (ldd & 3)) return OCTIC_EALIGN;
  const int H = D / 64;
  ApGemm a = ap_args();
  a.A = dpooled; a.a_z1 = D; a.a_z2 = 64; a.a_m = ldd; a.a_k = 1;
  a.Btab = wv; a.b_z2 = (int64_t)64 * D; a.b_k = D; a.b_n = 1;
  a.C = dZ; a.c_z1 = (int64_t)H * D; a.c_z2 = D; a.c_m = (int64_t)G * H * D;
  a.M = B; a.N = D; a.K = 64; a.Z2 = H;
  return ap_launch(a, (int64_t)G * H, stream);
}

int octic_attnpool_dwv(const float* dpooled, int64_t ldd, const float* Z, int B, int G, int D, float* const* dwv, void* stream) {
  if (!dpooled || !Z || !dwv) return OCTIC_ENULL;
  if (!ap_dims(B, G, D) || ldd < (int64_t)G * D) return OCTIC_ESHAPE;
  if (ap_mis(dpooled) || ap_mis(Z) || ap_mis(dwv) || (ldd & 3)) return OCTIC_EALIGN;
  const int H = D / 64;
  ApGemm a = ap_args();
  a.A = dpooled; a.a_z1 = D; a.a_z2 = 64; a.a_m = 1; a.a_k = ldd;
  a.B = Z; a.b_z1 = (int64_t)H * D; a.b_z2 = D; a.b_k = (int64_t)G * H * D; a.b_n = 1;
  a.Ctab = dwv; a.c_z2 = (int64_t)64 * D; a.c_m = D;
  a.M = 64; a.N = D; a.K = B; a.Z2 = H;
  return ap_launch(a, (int64_t)G * H, stream);
}

int octic_attnpool_dscores(const float* X, int64_t ldx, const float* dZ, const float* P, int64_t ldp, int64_t B, int N, int D,
                           int GH, float* dS, void* stream) {
  if (!X || !dZ || !P || !dS) return OCTIC_ENULL;
  if (!ap_dims(B, 1, D) || N < 1 || GH < 1 || ldp < GH || ldp > (int64_t)1 << 20 || ldx < D || P == dS) return OCTIC_ESHAPE;
  if (ap_mis(X) || ap_mis(dZ) || ap_mis(P) || ap_mis(dS) || (ldp & 3) || (ldx & 3)) return OCTIC_EALIGN;
  ApGemm a = ap_args();
  a.A = X; a.a_z1 = (int64_t)N * ldx; a.a_m = ldx; a.a_k = 1;
  a.B = dZ; a.b_z1 = (int64_t)GH * D; a.b_k = 1; a.b_n = D;
  a.C = dS; a.c_z1 = (int64_t)N * ldp; a.c_m = ldp;
  a.M = N; a.N = GH; a.K = D;
  if (int e = ap_launch(a, B, stream)) return e;
  ap_softmax_bwd_kernel<<<dim3((unsigned)((ldp + 63) / 64), (unsigned)B), 256, 0, (hipStream_t)stream>>>(P, dS, ldp, N, GH);
  return launch_status();
}

int octic_attnpool_unfold(const float* const* q, const float* const* wk, const float* dU, int G, int D, float* const* dq,
                          float* const* dwk, float* const* dbk, void* stream) {
  if (!q || !wk || !dU || !dq || !dwk || !dbk) return OCTIC_ENULL;
  if (!ap_dims(1, G, D)) return OCTIC_ESHAPE;
  if (ap_mis(q) || ap_mis(wk) || ap_mis(dU) || ap_mis(dq) || ap_mis(dwk) || ap_mis(dbk)) return OCTIC_EALIGN;
  ap_unfold_kernel<<<dim3((unsigned)(G * D)), 256, 0, (hipStream_t)stream>>>(q, wk, dU, D / 64, D, dq, dwk, dbk);
  return launch_status();
}
