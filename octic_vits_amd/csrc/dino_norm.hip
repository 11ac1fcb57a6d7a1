// The two normalisations of the DINO / iBOT head (dinov2/layers/dino_head.py:36-41) as row kernels.
//   * F.normalize(x, dim=-1, p=2, eps) and its backward: one wave per row, the row in registers as 16-byte chunks (chunk c of a
//     row belongs to lane c % 64, slot c / 64), the sum of squares in f32 - a lane adds its elements in ascending order, the
//     wave total is the DPP butterfly of octic_common.hpp - so the order is fixed by D alone and a row never sees its batch mates.
//   * nn.utils.weight_norm of the prototype layer: from f32 v [N, K] and g [N] the bf16 operand W = g v / ||v||_row, its
//     transpose W^T [K, N] (the operand of the input-gradient GEMM) through an LDS tile so that the stores run along N, and the
//     f32 row norms, in one pass over v; and (dv, dg) from the f32 weight gradient.  The f32 weight never exists.
// No atomics.  Per-row scalars (inv, norms, dg) are stored by lane 0 of the row's wave with an ordinary vector store.
#include "octic_common.hpp"

namespace octic {

constexpr int DN_THREADS = 256;               // 4 waves = 4 rows in flight a workgroup
constexpr int DN_WAVES = DN_THREADS / 64;
constexpr int DN_MAX_D = 4096;                // 8 chunks of 8 elements per lane
constexpr int WN_MAX_K = 2048;                // 8 chunks of 4 floats per lane
constexpr int WN_LDS_BYTES = 65536;
// bf16 elements behind a tile row: a row is then TN / 2 + 1 dwords, an odd number, instead of a multiple of the 64 banks' 32.
// The transposed write of a row of v is four 2-byte stores a lane, lane l at k = 4 l + j: the lanes of one store are
// 4 (TN / 2 + 1) dwords apart, i.e. 4 banks apart mod 64 (TN = 64) - 16 distinct banks over the wave, a 4-way conflict; without
// the pad all 64 lanes would meet on one bank.  Four k a lane make the lane stride a multiple of 4 dwords whatever the pad, so
// the conflict cannot be padded away (measured, it does not show: the variant without the transposed operand is no faster per
// byte - NOTES).  The read-back after the barrier is 16 contiguous bytes a thread.
constexpr int WN_PAD = 2;
typedef unsigned __attribute__((may_alias)) u32_alias;       // the bf16 tile read back as dwords

// ------------------------------------------------------------------------------------------------------- L2 normalisation
// NCH = chunk slots per lane (1, 2, 4, 8): D <= 512 NCH.
template <typename TI, typename TO, int NCH>
__global__ __launch_bounds__(DN_THREADS) void l2norm_fwd_kernel(const TI* __restrict__ x, int64_t ldx, int64_t rows, int chunks,
                                                                float eps, TO* __restrict__ y, int64_t ldy,
                                                                float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TI* xr = x + row * ldx;
  float v[NCH][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      load8<TI>(xr + 8 * c, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
  const float nrm = sqrtf(wave_total(ss));
  const float d = nrm < eps ? eps : nrm;                     // clamp_min: a NaN norm stays NaN (fmaxf would hide it)
  TO* yr = y + row * ldy;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = v[i][j] / d;
      store8<TO>(yr + 8 * c, o);
    }
  }
  if (lane == 0) inv[row] = 1.0f / d;
}

// dx = inv (g - yh (yh . g)) with yh = x inv where ||x|| >= eps (clamp_min passes the gradient there), g inv below it.  The norm
// is summed again in the forward's order, so the branch is the forward's.
template <typename TG, typename TX, typename TD, int NCH>
__global__ __launch_bounds__(DN_THREADS) void l2norm_bwd_kernel(const TG* __restrict__ g, int64_t ldg, const TX* __restrict__ x,
                                                                int64_t ldx, const float* __restrict__ inv, int64_t rows,
                                                                int chunks, float eps, TD* __restrict__ dx, int64_t lddx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TX* xr = x + row * ldx;
  const TG* gr = g + row * ldg;
  const float rinv = inv[row];
  float xv[NCH][8], gv[NCH][8];
  float ss = 0.f, dot = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      load8<TX>(xr + 8 * c, xv[i]);
      load8<TG>(gr + 8 * c, gv[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ss += xv[i][j] * xv[i][j];
        xv[i][j] *= rinv;                       // yh
        dot += xv[i][j] * gv[i][j];
      }
    }
  }
  const float nrm = sqrtf(wave_total(ss));
  dot = wave_total(dot);
  const bool clamped = nrm < eps;               // (a NaN norm is not clamped: NaN flows through the projection as in torch)
  TD* dr = dx + row * lddx;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = clamped ? gv[i][j] * rinv : rinv * (gv[i][j] - xv[i][j] * dot);
      store8<TD>(dr + 8 * c, o);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ weight norm
// A workgroup owns TN consecutive rows of v; wave w takes rows w, w + 4, ... of the tile, one at a time, the row in registers as
// 4-float chunks (chunk c: lane c % 64, slot c / 64).  W is stored row by row (8 bytes a lane, contiguous over the wave); with
// WT the bf16 values also go to tile[k][n] in LDS and, after the barrier, leave as 16-byte pieces of W^T rows: the TN values of
// one k are TN * 2 contiguous bytes of W^T.
template <int NCH, bool WT>
__global__ __launch_bounds__(DN_THREADS) void weight_norm_prep_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                                      int N, int K, int TN, bf16* __restrict__ W,
                                                                      bf16* __restrict__ Wt, float* __restrict__ norms) {
  extern __shared__ __align__(16) unsigned char wn_smem[];
  bf16* tile = (bf16*)wn_smem;                  // [K][TN + WN_PAD]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * TN;
  const int chunks = K / 4;
  const int lds_ld = TN + WN_PAD;
  for (int r = wave; r < TN; r += DN_WAVES) {
    const int n = n0 + r;
    if (n >= N) break;                          // (wave-uniform; the barrier below is outside the loop)
    const float* vr = v + (int64_t)n * K;
    f32x4 x[NCH];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < chunks) {
        x[i] = *(const f32x4*)(vr + 4 * c);
        ss += x[i][0] * x[i][0];
        ss += x[i][1] * x[i][1];
        ss += x[i][2] * x[i][2];
        ss += x[i][3] * x[i][3];
      }
    }
    const float nrm = sqrtf(wave_total(ss));
    const float rn = 1.0f / nrm, gn = g[n];
    bf16* wr = W + (int64_t)n * K;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < chunks) {
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f2bf(gn * x[i][j] * rn);
        *(bf16x4*)(wr + 4 * c) = o;
        if (WT) {
#pragma unroll
          for (int j = 0; j < 4; ++j) tile[(4 * c + j) * lds_ld + r] = o[j];
        }
      }
    }
    if (lane == 0) norms[n] = nrm;
  }
  if (!WT) return;
  __syncthreads();
  const int per_k = TN / 8;                     // 16-byte pieces of one k
  const int pieces = K * per_k;
  for (int p = threadIdx.x; p < pieces; p += DN_THREADS) {
    const int k = p / per_k, q = p - k * per_k;
    const int n = n0 + 8 * q;
    if (n >= N) continue;                       // (N % 8 == 0: a piece lies inside or outside as a whole)
    const u32_alias* src = (const u32_alias*)(tile + k * lds_ld + 8 * q);   // 4-byte aligned: lds_ld and 8 q are even
    u32x4 o = {src[0], src[1], src[2], src[3]};
    *(u32x4*)(Wt + (int64_t)k * N + n) = o;
  }
}

// One wave per row, f32: with r = 1 / ||v|| and s = dW . v:  dg = s r,  dv = g (r dW - r^3 s v).
template <int NCH>
__global__ __launch_bounds__(DN_THREADS) void weight_norm_bwd_kernel(const float* __restrict__ dW, const float* __restrict__ v,
                                                                     const float* __restrict__ g, const float* __restrict__ norms,
                                                                     int N, int K, float* __restrict__ dv, float* __restrict__ dg) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const int chunks = K / 4;
  const float* wr = dW + (int64_t)n * K;
  const float* vr = v + (int64_t)n * K;
  f32x4 a[NCH], b[NCH];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      a[i] = *(const f32x4*)(wr + 4 * c);
      b[i] = *(const f32x4*)(vr + 4 * c);
      s += a[i][0] * b[i][0];
      s += a[i][1] * b[i][1];
      s += a[i][2] * b[i][2];
      s += a[i][3] * b[i][3];
    }
  }
  s = wave_total(s);
  const float r = 1.0f / norms[n], gn = g[n];
  const float r3s = r * r * r * s;
  float* dr = dv + (int64_t)n * K;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = gn * (r * a[i][j] - r3s * b[i][j]);
      *(f32x4*)(dr + 4 * c) = o;
    }
  }
  if (lane == 0) dg[n] = s * r;
}

static inline int slots_for(int chunks) {       // chunk slots per lane: 1, 2, 4 or 8
  const int per = (chunks + 63) / 64;
  return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : 8;
}

static inline int wn_tile_rows(int K) {         // rows of v a prep workgroup owns: the widest of 64 .. 8 whose LDS tile fits
  for (int tn = 64; tn >= 8; tn >>= 1)
    if ((int64_t)K * (tn + WN_PAD) * 2 <= WN_LDS_BYTES) return tn;
  return 0;
}

static inline bool wn_shape_ok(int64_t N, int64_t K) {
  return N >= 1 && N <= 0x7FFFFFFFll / 4 && K >= 8 && K <= WN_MAX_K && K % 8 == 0 && N * K < (1ll << 40);
}

template <typename TI, typename TO>
static void l2_fwd_launch(int nch, dim3 grid, hipStream_t st, const void* x, int64_t ldx, int64_t rows, int chunks, float eps,
                          void* y, int64_t ldy, float* inv) {
#define OCTIC_L2F(N_) l2norm_fwd_kernel<TI, TO, N_><<<grid, dim3(DN_THREADS), 0, st>>>((const TI*)x, ldx, rows, chunks, eps, (TO*)y, ldy, inv)
  if (nch == 1) OCTIC_L2F(1);
  else if (nch == 2) OCTIC_L2F(2);
  else if (nch == 4) OCTIC_L2F(4);
  else OCTIC_L2F(8);
#undef OCTIC_L2F
}

template <typename TG, typename TX, typename TD>
static void l2_bwd_launch(int nch, dim3 grid, hipStream_t st, const void* g, int64_t ldg, const void* x, int64_t ldx,
                          const float* inv, int64_t rows, int chunks, float eps, void* dx, int64_t lddx) {
#define OCTIC_L2B(N_) l2norm_bwd_kernel<TG, TX, TD, N_><<<grid, dim3(DN_THREADS), 0, st>>>((const TG*)g, ldg, (const TX*)x, ldx, inv, rows, chunks, eps, (TD*)dx, lddx)
  if (nch == 1) OCTIC_L2B(1);
  else if (nch == 2) OCTIC_L2B(2);
  else if (nch == 4) OCTIC_L2B(4);
  else OCTIC_L2B(8);
#undef OCTIC_L2B
}

static inline int l2_check(const void* p, int dtype, int64_t ld, int64_t D) {
  if (!p) return OCTIC_ENULL;
  if (dtype != OCTIC_BF16 && dtype != OCTIC_F32) return OCTIC_EDTYPE;
  if (ld < D) return OCTIC_ESHAPE;
  if ((((uintptr_t)p) & 15) || ((ld * elem_size(dtype)) & 15)) return OCTIC_EALIGN;
  return OCTIC_OK;
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_l2norm_ok(int64_t rows, int64_t D) {
  return rows >= 1 && rows <= 0x7FFFFFFFll && D >= 8 && D <= DN_MAX_D && D % 8 == 0;
}

int octic_l2norm_rows_fwd(const void* x, int x_dtype, int64_t ldx, int64_t rows, int64_t D, float eps, void* y, int y_dtype,
                          int64_t ldy, float* inv, void* stream) {
  if (!x || !y || !inv) return OCTIC_ENULL;
  if (!octic_l2norm_ok(rows, D)) return OCTIC_ESHAPE;
  int e = l2_check(x, x_dtype, ldx, D);
  if (e == OCTIC_OK) e = l2_check(y, y_dtype, ldy, D);
  if (e != OCTIC_OK) return e;
  const int chunks = (int)(D / 8), nch = slots_for(chunks);
  const dim3 grid((unsigned)((rows + DN_WAVES - 1) / DN_WAVES));
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == OCTIC_BF16 && y_dtype == OCTIC_BF16) l2_fwd_launch<bf16, bf16>(nch, grid, st, x, ldx, rows, chunks, eps, y, ldy, inv);
  else if (x_dtype == OCTIC_BF16) l2_fwd_launch<bf16, float>(nch, grid, st, x, ldx, rows, chunks, eps, y, ldy, inv);
  else if (y_dtype == OCTIC_BF16) l2_fwd_launch<float, bf16>(nch, grid, st, x, ldx, rows, chunks, eps, y, ldy, inv);
  else l2_fwd_launch<float, float>(nch, grid, st, x, ldx, rows, chunks, eps, y, ldy, inv);
  return launch_status();
}

int octic_l2norm_rows_bwd(const void* g, int g_dtype, int64_t ldg, const void* x, int x_dtype, int64_t ldx, const float* inv,
                          int64_t rows, int64_t D, float eps, void* dx, int64_t lddx, void* stream) {
  if (!g || !x || !inv || !dx) return OCTIC_ENULL;
  if (!octic_l2norm_ok(rows, D)) return OCTIC_ESHAPE;
  int e = l2_check(g, g_dtype, ldg, D);
  if (e == OCTIC_OK) e = l2_check(x, x_dtype, ldx, D);
  if (e == OCTIC_OK) e = l2_check(dx, x_dtype, lddx, D);       // dx has x's dtype
  if (e != OCTIC_OK) return e;
  const int chunks = (int)(D / 8), nch = slots_for(chunks);
  const dim3 grid((unsigned)((rows + DN_WAVES - 1) / DN_WAVES));
  hipStream_t st = (hipStream_t)stream;
  if (g_dtype == OCTIC_BF16 && x_dtype == OCTIC_BF16) l2_bwd_launch<bf16, bf16, bf16>(nch, grid, st, g, ldg, x, ldx, inv, rows, chunks, eps, dx, lddx);
  else if (g_dtype == OCTIC_BF16) l2_bwd_launch<bf16, float, float>(nch, grid, st, g, ldg, x, ldx, inv, rows, chunks, eps, dx, lddx);
  else if (x_dtype == OCTIC_BF16) l2_bwd_launch<float, bf16, bf16>(nch, grid, st, g, ldg, x, ldx, inv, rows, chunks, eps, dx, lddx);
  else l2_bwd_launch<float, float, float>(nch, grid, st, g, ldg, x, ldx, inv, rows, chunks, eps, dx, lddx);
  return launch_status();
}

int octic_weight_norm_prep(const float* v, const float* g, int64_t N, int64_t K, void* W, void* Wt, float* norms, void* stream) {
  if (!v || !g || !W || !norms) return OCTIC_ENULL;
  if (!wn_shape_ok(N, K) || (Wt && N % 8)) return OCTIC_ESHAPE;
  if ((((uintptr_t)v) & 15) || (((uintptr_t)W) & 15) || (((uintptr_t)Wt) & 15)) return OCTIC_EALIGN;
  const int tn = wn_tile_rows((int)K);
  if (tn < 8) return OCTIC_ESHAPE;
  const int nch = slots_for((int)(K / 4));
  const dim3 grid((unsigned)((N + tn - 1) / tn));
  const size_t lds = Wt ? (size_t)K * (tn + WN_PAD) * 2 : 0;
  hipStream_t st = (hipStream_t)stream;
#define OCTIC_WNP(N_, T_) weight_norm_prep_kernel<N_, T_><<<grid, dim3(DN_THREADS), lds, st>>>(v, g, (int)N, (int)K, tn, (bf16*)W, (bf16*)Wt, norms)
  if (Wt) {
    if (nch == 1) OCTIC_WNP(1, true);
    else if (nch == 2) OCTIC_WNP(2, true);
    else if (nch == 4) OCTIC_WNP(4, true);
    else OCTIC_WNP(8, true);
  } else {
    if (nch == 1) OCTIC_WNP(1, false);
    else if (nch == 2) OCTIC_WNP(2, false);
    else if (nch == 4) OCTIC_WNP(4, false);
    else OCTIC_WNP(8, false);
  }
#undef OCTIC_WNP
  return launch_status();
}

int octic_weight_norm_bwd(const float* dW, const float* v, const float* g, const float* norms, int64_t N, int64_t K, float* dv,
                          float* dg, void* stream) {
  if (!dW || !v || !g || !norms || !dv || !dg) return OCTIC_ENULL;
  if (!wn_shape_ok(N, K)) return OCTIC_ESHAPE;
  if ((((uintptr_t)dW) & 15) || (((uintptr_t)v) & 15) || (((uintptr_t)dv) & 15)) return OCTIC_EALIGN;
  const int nch = slots_for((int)(K / 4));
  const dim3 grid((unsigned)((N + DN_WAVES - 1) / DN_WAVES));
  hipStream_t st = (hipStream_t)stream;
#define OCTIC_WNB(N_) weight_norm_bwd_kernel<N_><<<grid, dim3(DN_THREADS), 0, st>>>(dW, v, g, norms, (int)N, (int)K, dv, dg)
  if (nch == 1) OCTIC_WNB(1);
  else if (nch == 2) OCTIC_WNB(2);
  else if (nch == 4) OCTIC_WNB(4);
  else OCTIC_WNB(8);
#undef OCTIC_WNB
  return launch_status();
}

}  // extern "C"
