// Float32 dense GEMMs of the standard half (nn.Linear of deit/vit.py:14-56, dinov2/layers/{mlp,swiglu_ffn,attention}.py) on
// the exact-f32 MFMA (v_mfma_f32_16x16x4_f32): forward NT, input gradient NN, weight gradient TN, and the f32 GELU backward.
// ONE kernel body serves the three products.  A workgroup of 4 waves (2 x 2) owns a 128 x 128 output tile; wave (wi, wj) owns
// 64 x 64 of it as 4 x 4 accumulators of 16 x 16 (16 independent chains per wave: the 40-cycle dependent latency of the
// instruction never shows).  The reduction runs in chunks of 32: both operand tiles go global -> registers -> LDS (the next
// chunk's loads are in flight under the products), in one of two images:
//   reduction-contiguous operand (A and W of NT, G of NN):   [128 rows][32 r], row stride 36 floats, fragments by ds_read_b128
//   reduction-major operand (W of NN, G and X of TN):        [32 r][128 columns], row stride 132, fragments by ds_read_b32
// W is read as stored in all three products: no transposed copy exists.  Both strides keep the fragment reads of a 32-lane
// half on distinct banks (36: as knn_common.hpp; 132: lanes of one half differ by 4 rows = 528 words = 16 banks).
// ORDER OF AN ELEMENT'S SUM: one fmaf chain from +0 over the reduction index in chunks of 16 ascending, inside a chunk
// e, 4 + e, 8 + e, 12 + e for e = 0 .. 3 (the instruction sums its 4 k in lane-group order), then + bias.  It depends on the
// reduction length alone - not on M, the row's position or the tile - and a row of the result reads only that row of the left
// operand: NT and NN results are independent of batch mates, bitwise.  Tails are zero-filled in LDS (x + 0 * 0 = x).
// TN reduces over the M token rows: row slabs (blockIdx.z) write f32 partial tiles to the workspace and a second launch adds
// them in slab order; the slab count is a function of (M, N, K) alone.  The column sums of G ride along in the workgroups of
// the first K tile (sequential over a slab's rows from the LDS image, then slab order).  No floating-point atomics anywhere.
#include "octic_common.hpp"

namespace octic {
namespace {

constexpr int DF_BM = 128, DF_BN = 128, DF_BK = 32;
constexpr int DF_LDK = 36, DF_LDT = 132;
constexpr int DF_IMG = DF_BM * DF_LDK;            // floats of one operand image (the reduction-major one needs 32 * 132 <= this)
constexpr int DF_MAX_SLABS = 64;
enum { DF_NT = 0, DF_NN = 1, DF_TN = 2 };
enum { EPI_PLAIN = 0, EPI_GELU = 1, EPI_SLAB = 2 };

struct DfPlan {
  int slabs, slab_rows, wgs;
};

struct DfArgs {
  const float *P, *Q, *bias;    // P: the operand of the output rows, Q: of the output columns; bias over the columns
  float *out, *h, *db;
  int64_t ldp, ldq, ldo, ldh, slab_out, slab_db;
  int I, J, R, slab_rows;       // out is [I, J], the reduction has R terms; slab_rows: terms per blockIdx.z (EPI_SLAB)
};

// (op, M, N, K, ld_max) -> accepted? and the launch shape.  The launchers call this and nothing else for shape decisions.
inline int df_plan(int op, int64_t M, int64_t N, int64_t K, int64_t ld_max, DfPlan* p) {
  if (op < DF_NT || op > DF_TN || M < 1 || N < 4 || K < 4 || (N & 3) || (K & 3) || ld_max < 0) return OCTIC_ESHAPE;
  const int64_t longest_row = N > K ? N : K;                      // every op has an operand with rows of N and one of K
  if (ld_max && ld_max < longest_row) return OCTIC_ESHAPE;        // that operand's stride is below its row length
  const int64_t ld = ld_max > longest_row ? ld_max : longest_row;
  const int64_t rows = M > longest_row ? M : longest_row;
  if (rows * ld >= ((int64_t)1 << 31)) return OCTIC_ESHAPE;       // element offsets of an operand stay below 2^31
  const int64_t I = op == DF_TN ? N : M, J = op == DF_NT ? N : K;
  const int64_t tiles = ((I + DF_BM - 1) / DF_BM) * ((J + DF_BN - 1) / DF_BN);
  int64_t slabs = 1, slab_rows = 0;
  if (op == DF_TN) {
    // about four workgroups per CU of a 256-CU device (they are co-resident: the last round's imbalance shrinks with their
    // number), slabs of at least 256 rows; a function of (M, N, K) only
    int64_t want = 1024 / tiles, most = M / 256;
    slabs = want < most ? want : most;
    slabs = slabs < 1 ? 1 : (slabs > DF_MAX_SLABS ? DF_MAX_SLABS : slabs);
    slab_rows = ((M + slabs - 1) / slabs + DF_BK - 1) / DF_BK * DF_BK;
    slabs = (M + slab_rows - 1) / slab_rows;
  }
  if (tiles * slabs >= ((int64_t)1 << 31) || (J + DF_BN - 1) / DF_BN > 65535) return OCTIC_ESHAPE;
  if (p) {
    p->slabs = (int)slabs;
    p->slab_rows = (int)slab_rows;
    p->wgs = (int)(tiles * slabs);
  }
  return OCTIC_OK;
}

inline int64_t df_ws_bytes(int op, int64_t N, int64_t K, const DfPlan& p) {
  const int64_t need = (op == DF_TN && p.slabs > 1) ? (int64_t)p.slabs * (N * K + N) * 4 : 0;
  return need < 256 ? 256 : (need + 255) / 256 * 256;
}

__device__ __forceinline__ f32x4 df_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Rows [row0, row0 + 128) x reduction terms [r0, r0 + 32) of one operand into 4 float4 registers per thread (zeros past an edge).
template <bool RED_MAJOR>
__device__ __forceinline__ void df_fetch(f32x4 v[4], const float* __restrict__ p, int64_t ld, int row0, int nrows, int r0, int rend) {
  const int tid = threadIdx.x;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (!RED_MAJOR) {
    const int k = r0 + (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + (tid >> 3) + 32 * i;
      v[i] = (row < nrows && k < rend) ? *(const f32x4*)(p + (int64_t)row * ld + k) : zero;
    }
  } else {
    const int c = row0 + (tid & 31) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = r0 + (tid >> 5) + 8 * i;
      v[i] = (rr < rend && c < nrows) ? *(const f32x4*)(p + (int64_t)rr * ld + c) : zero;
    }
  }
}
template <bool RED_MAJOR>
__device__ __forceinline__ void df_stage(float* img, const f32x4 v[4]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!RED_MAJOR) *(f32x4*)(img + ((tid >> 3) + 32 * i) * DF_LDK + (tid & 7) * 4) = v[i];
    else *(f32x4*)(img + ((tid >> 5) + 8 * i) * DF_LDT + (tid & 31) * 4) = v[i];
  }
}
// The fragment of 16-row block `blk` (rows base .. base + 15, lane r owns row base + r) for reduction terms 16 jj + 4 q + e.
template <bool RED_MAJOR>
__device__ __forceinline__ f32x4 df_frag(const float* img, int base, int r, int q, int jj) {
  if (!RED_MAJOR) return *(const f32x4*)(img + (base + r) * DF_LDK + 16 * jj + 4 * q);
  const float* c = img + (16 * jj + 4 * q) * DF_LDT + base + r;
  f32x4 v = {c[0], c[DF_LDT], c[2 * DF_LDT], c[3 * DF_LDT]};
  return v;
}

template <bool PT, bool QT, int EPI>
__global__ __launch_bounds__(256) void dense_f32_kernel(DfArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * DF_IMG];
  float* Ps = lds;
  float* Qs = lds + DF_IMG;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int wi = w >> 1, wj = w & 1;
  const int i0 = blockIdx.x * DF_BM, j0 = blockIdx.y * DF_BN;
  int rbeg = 0, rend = a.R;
  if (EPI == EPI_SLAB) {
    rbeg = blockIdx.z * a.slab_rows;
    rend = rbeg + a.slab_rows < a.R ? rbeg + a.slab_rows : a.R;
  }
  const bool colsum = EPI == EPI_SLAB && a.db && blockIdx.y == 0 && tid < DF_BM;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4][4];
#pragma unroll
  for (int bt = 0; bt < 4; ++bt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[bt][ct] = zero;
  float dbsum = 0.f;

  f32x4 pr[4], qr[4];
  df_fetch<PT>(pr, a.P, a.ldp, i0, a.I, rbeg, rend);
  df_fetch<QT>(qr, a.Q, a.ldq, j0, a.J, rbeg, rend);
  for (int r0 = rbeg; r0 < rend; r0 += DF_BK) {
    __syncthreads();                         // the previous chunk's fragment reads are done
    df_stage<PT>(Ps, pr);
    df_stage<QT>(Qs, qr);
    __syncthreads();
    if (r0 + DF_BK < rend) {                 // in flight under the products
      df_fetch<PT>(pr, a.P, a.ldp, i0, a.I, r0 + DF_BK, rend);
      df_fetch<QT>(qr, a.Q, a.ldq, j0, a.J, r0 + DF_BK, rend);
    }
    if (EPI == EPI_SLAB && PT && colsum) {   // column tid of G's image, rows in order (zero rows past the slab's end)
#pragma unroll 8
      for (int rr = 0; rr < DF_BK; ++rr) dbsum += Ps[rr * DF_LDT + tid];
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      f32x4 pv[4], qv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        pv[t] = df_frag<PT>(Ps, 64 * wi + 16 * t, r, q, jj);
        qv[t] = df_frag<QT>(Qs, 64 * wj + 16 * t, r, q, jj);
      }
      // the Q fragment is the instruction's A operand: accumulator register e of lane (r, q) is out[i + r][j + 4 q + e],
      // four consecutive columns - the epilogue stores 16 bytes per lane
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt)
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[bt][ct] = df_mfma(qv[ct][e], pv[bt][e], acc[bt][ct]);
    }
  }

  float* out = a.out;
  if (EPI == EPI_SLAB) out += (int64_t)blockIdx.z * a.slab_out;
#pragma unroll
  for (int bt = 0; bt < 4; ++bt) {
    const int i = i0 + 64 * wi + 16 * bt + r;
    if (i >= a.I) continue;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int j = j0 + 64 * wj + 16 * ct + 4 * q;
      if (j >= a.J) continue;
      f32x4 v = acc[bt][ct];
      if (EPI != EPI_SLAB && a.bias) v += *(const f32x4*)(a.bias + j);
      if (EPI == EPI_GELU) {
        *(f32x4*)(a.h + (int64_t)i * a.ldh + j) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_exact(v[e]);
      }
      *(f32x4*)(out + (int64_t)i * a.ldo + j) = v;
    }
  }
  if (EPI == EPI_SLAB && colsum && i0 + tid < a.I) a.db[(int64_t)blockIdx.z * a.slab_db + i0 + tid] = dbsum;
}

// out[n, k] = sum over slabs, in slab order, of the partial tiles; db likewise.  One float4 (or one db column) per thread.
__global__ __launch_bounds__(256) void dense_f32_tn_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ dbws,
                                                                  int slabs, int N, int K, float* __restrict__ out, int64_t ldo,
                                                                  float* __restrict__ db) {
  const int64_t k4 = K / 4, nk4 = (int64_t)N * k4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < nk4) {
    f32x4 s = *(const f32x4*)(ws + idx * 4);
    for (int z = 1; z < slabs; ++z) s += *(const f32x4*)(ws + ((int64_t)z * nk4 + idx) * 4);
    *(f32x4*)(out + (idx / k4) * ldo + (idx % k4) * 4) = s;
  } else if (db && idx - nk4 < N) {
    const int64_t n = idx - nk4;
    float s = dbws[n];
    for (int z = 1; z < slabs; ++z) s += dbws[(int64_t)z * N + n];
    db[n] = s;
  }
}

// ------------------------------------------------------------------------------------------ GELU backward, f32
// The f32 twin of dense_gelu_bwd_kernel (dense.hip): dh = gelu'(h) * g on dense [rows, d] and per-row-block column sums of dh.
// 64 column chunks of 4 floats x 4 row phases per workgroup; exact erff / expf (what ATen's f32 GeluBackward evaluates).
__device__ __forceinline__ float gelu_grad_f32(float x) {     // cdf + x pdf, in the order ATen's kernel evaluates it
  const float cdf = 0.5f * (1.0f + erff(x * kSqrt1Over2));
  const float pdf = expf(-0.5f * x * x) * kInvSqrt2Pi;
  return cdf + x * pdf;
}
constexpr int kGeluF32RowBlocks = 256;       // = octic_dense_gelu_blocks(): one partials shape for both dtypes
__global__ __launch_bounds__(256) void dense_gelu_bwd_f32_kernel(const float* __restrict__ h, const float* __restrict__ g,
                                                                 float* __restrict__ dh, float* __restrict__ partials,
                                                                 int64_t rows, int d) {
  __shared__ float red[4][64][4];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cl) * 4;
  const int64_t per = (rows + kGeluF32RowBlocks - 1) / kGeluF32RowBlocks;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (col < d) {
    for (int64_t r = r0 + ph; r < r1; r += 4) {
      const f32x4 hv = *(const f32x4*)(h + r * d + col), gv = *(const f32x4*)(g + r * d + col);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = gelu_grad_f32(hv[e]) * gv[e];
      acc += o;
      *(f32x4*)(dh + r * d + col) = o;
    }
  }
  if (!partials) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) red[ph][cl][e] = acc[e];
  __syncthreads();
  if (ph == 0 && col < d) {
    float* out = partials + (int64_t)blockIdx.y * d + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = (red[0][cl][e] + red[1][cl][e]) + (red[2][cl][e] + red[3][cl][e]);
  }
}
// db[j] = sum_b partials[b][j] in the order of dense_finish_kernel (16 groups of every 16th block, then the groups in order)
__global__ __launch_bounds__(256) void dense_f32_colsum_finish_kernel(const float* __restrict__ partials, int nblocks, int d,
                                                                      float* __restrict__ db) {
  __shared__ float red[16][17];
  const int cx = threadIdx.x & 15, gy = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + cx;
  float s = 0.f;
  if (j < d)
    for (int b = gy; b < nblocks; b += 16) s += partials[(int64_t)b * d + j];
  red[gy][cx] = s;
  __syncthreads();
  if (gy == 0 && j < d) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cx];
    db[j] = t;
  }
}

inline bool misaligned(const void* p) { return ((uintptr_t)p) & 15; }

template <bool PT, bool QT, int EPI>
inline void df_launch(const DfArgs& a, int slabs, hipStream_t s) {
  const dim3 grid((a.I + DF_BM - 1) / DF_BM, (a.J + DF_BN - 1) / DF_BN, slabs);
  hipLaunchKernelGGL((dense_f32_kernel<PT, QT, EPI>), grid, dim3(256), 0, s, a);
}

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_dense_f32_plan(int op, int64_t M, int64_t N, int64_t K, int64_t ld_max, int out[4]) {
  DfPlan p;
  const int rc = df_plan(op, M, N, K, ld_max, &p);
  if (rc != OCTIC_OK) return rc;
  if (out) {
    out[0] = DF_BM;
    out[1] = DF_BN;
    out[2] = p.slabs;
    out[3] = p.wgs;
  }
  return OCTIC_OK;
}

int64_t octic_dense_f32_workspace_bytes(int op, int64_t M, int64_t N, int64_t K) {
  DfPlan p;
  const int rc = df_plan(op, M, N, K, 0, &p);
  return rc != OCTIC_OK ? rc : df_ws_bytes(op, N, K, p);
}

int octic_dense_f32_nt(const float* A, const float* W, const float* bias, int64_t M, int64_t N, int64_t K, int64_t lda,
                       int64_t ldw, float* C, int64_t ldc, int gelu, float* H, int64_t ldh, void* stream) {
  if (!A || !W || !C || (gelu && !H)) return OCTIC_ENULL;
  int64_t ldm = lda > ldw ? lda : ldw;
  ldm = ldc > ldm ? ldc : ldm;
  if (gelu && ldh > ldm) ldm = ldh;
  DfPlan p;
  const int rc = df_plan(DF_NT, M, N, K, ldm, &p);
  if (rc != OCTIC_OK) return rc;
  if (lda < K || ldw < K || ldc < N || (gelu && ldh < N)) return OCTIC_ESHAPE;
  if (misaligned(A) || misaligned(W) || misaligned(C) || misaligned(bias) || (gelu && misaligned(H)) ||
      ((lda | ldw | ldc | (gelu ? ldh : 0)) & 3))
    return OCTIC_EALIGN;
  DfArgs a = {};
  a.P = A; a.Q = W; a.bias = bias; a.out = C; a.h = H;
  a.ldp = lda; a.ldq = ldw; a.ldo = ldc; a.ldh = ldh;
  a.I = (int)M; a.J = (int)N; a.R = (int)K;
  if (gelu) df_launch<false, false, EPI_GELU>(a, 1, (hipStream_t)stream);
  else df_launch<false, false, EPI_PLAIN>(a, 1, (hipStream_t)stream);
  return launch_status();
}

int octic_dense_f32_nn(const float* G, const float* W, int64_t M, int64_t N, int64_t K, int64_t ldg, int64_t ldw, float* DX,
                       int64_t ldx, void* stream) {
  if (!G || !W || !DX) return OCTIC_ENULL;
  int64_t ldm = ldg > ldw ? ldg : ldw;
  ldm = ldx > ldm ? ldx : ldm;
  DfPlan p;
  const int rc = df_plan(DF_NN, M, N, K, ldm, &p);
  if (rc != OCTIC_OK) return rc;
  if (ldg < N || ldw < K || ldx < K) return OCTIC_ESHAPE;
  if (misaligned(G) || misaligned(W) || misaligned(DX) || ((ldg | ldw | ldx) & 3)) return OCTIC_EALIGN;
  DfArgs a = {};
  a.P = G; a.Q = W; a.out = DX;
  a.ldp = ldg; a.ldq = ldw; a.ldo = ldx;
  a.I = (int)M; a.J = (int)K; a.R = (int)N;
  df_launch<false, true, EPI_PLAIN>(a, 1, (hipStream_t)stream);
  return launch_status();
}

int octic_dense_f32_tn(const float* G, const float* X, int64_t M, int64_t N, int64_t K, int64_t ldg, int64_t ldx, float* DW,
                       int64_t ldw, float* db, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!G || !X || !DW) return OCTIC_ENULL;
  int64_t ldm = ldg > ldx ? ldg : ldx;
  ldm = ldw > ldm ? ldw : ldm;
  DfPlan p;
  const int rc = df_plan(DF_TN, M, N, K, ldm, &p);
  if (rc != OCTIC_OK) return rc;
  if (ldg < N || ldx < K || ldw < K) return OCTIC_ESHAPE;
  if (misaligned(G) || misaligned(X) || misaligned(DW) || misaligned(workspace) || ((ldg | ldx | ldw) & 3)) return OCTIC_EALIGN;
  if (p.slabs > 1) {
    if (!workspace) return OCTIC_ENULL;
    if (workspace_bytes < df_ws_bytes(DF_TN, N, K, p)) return OCTIC_EWORKSPACE;
  }
  DfArgs a = {};
  a.P = G; a.Q = X;
  a.ldp = ldg; a.ldq = ldx;
  a.I = (int)N; a.J = (int)K; a.R = (int)M;
  a.slab_rows = p.slab_rows;
  if (p.slabs == 1) {
    a.out = DW; a.ldo = ldw; a.db = db;
    df_launch<true, true, EPI_SLAB>(a, 1, (hipStream_t)stream);
    return launch_status();
  }
  float* ws = (float*)workspace;
  float* dbws = ws + (int64_t)p.slabs * N * K;
  a.out = ws; a.ldo = K; a.slab_out = N * K;
  a.db = db ? dbws : nullptr; a.slab_db = N;
  df_launch<true, true, EPI_SLAB>(a, p.slabs, (hipStream_t)stream);
  const int64_t items = N * (K / 4) + (db ? N : 0);
  hipLaunchKernelGGL(dense_f32_tn_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws,
                     dbws, p.slabs, (int)N, (int)K, DW, ldw, db);
  return launch_status();
}

int octic_dense_gelu_bwd_f32(const float* h, const float* g, float* dh, float* partials, float* db, int64_t rows, int d,
                             void* stream) {
  if (rows == 0 && !db) return OCTIC_OK;
  if (!h || !g || !dh || (db && !partials)) return OCTIC_ENULL;
  if (rows < 0 || d <= 0 || (d & 3) || rows * (int64_t)d >= ((int64_t)1 << 40)) return OCTIC_ESHAPE;
  if (misaligned(h) || misaligned(g) || misaligned(dh) || misaligned(partials)) return OCTIC_EALIGN;
  hipLaunchKernelGGL(dense_gelu_bwd_f32_kernel, dim3((d / 4 + 63) / 64, kGeluF32RowBlocks), dim3(256), 0, (hipStream_t)stream, h,
                     g, dh, db ? partials : nullptr, rows, d);
  if (db)
    hipLaunchKernelGGL(dense_f32_colsum_finish_kernel, dim3((d + 15) / 16), dim3(256), 0, (hipStream_t)stream, partials,
                       kGeluF32RowBlocks, d, db);
  return launch_status();
}

}  // extern "C"
