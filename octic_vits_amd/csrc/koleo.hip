// KoLeo regularizer of the DINOv2 step (dinov2/loss/koleo_loss.py:18-48) as one forward and one backward launch over G
// independent groups of n consecutive rows (the two global crops of the recipe), instead of the eager composition's ~50
// launches (normalize, an n x n mm on the BLAS library, a strided diagonal fill, max, gather, PairwiseDistance, log, mean and
// the autograd backward of each).  Per row i of a group, all in f32 after one widening of the input:
//   inv_i = 1 / max(||x_i||, eps),  xh_i = x_i inv_i
//   I(i)  = the row j != i of the group with the largest xh_i . xh_j
//   d_i   = ||xh_i - xh_I(i) + 1e-8||   (nn.PairwiseDistance adds its eps to every element),   term_i = -log(d_i + eps)
// TOTAL ORDER of the neighbour search, as in knn_common.hpp: (dot, row index) - the larger dot first, on equal dots the lower
// index; a dot that is NaN counts as -inf; the row itself is excluded (the reference's "-1 on the diagonal" as an exclusion,
// not as a value).  torch.max leaves ties unspecified; this rule is ours.
// One workgroup per row.  Forward: xh_i sits in LDS, every wave takes the rows j = wave, wave + 8, ... of the group and
// forms sum_k xh_i[k] x_j[k] and sum_k x_j[k]^2 in ONE read of x_j (the dot is the first times inv_j; a row whose squared norm
// overflows has inv_j = 0, xh_j = 0 and the dot 0, as the eager arm has).  Backward: G_i = c_i e_i - sum_{j: I(j) = i} c_j e_j
// with c = -gterm / (d + eps), e = (xh - xh_I + 1e-8) / d, the rows j gathered in ascending order by the workgroup that owns
// row i - no atomics (index_select's backward scatters with them) - then autograd's F.normalize:
// dx_i = (G_i - xh_i (xh_i . G_i)) inv_i where ||x_i|| >= eps, G_i / eps below it.
// DETERMINISM: every sum is a fixed-order chain - 8 consecutive elements per lane at a stride of 512, the DPP wave tree, the
// waves in index order - that depends on D alone, and inv_j is formed by the same routine wherever it is needed.  A row's
// results depend on the rows of its own group, n and D only: not on G, the group's position, the row strides or the rest of
// the batch; two calls are bitwise equal.
#include "octic_common.hpp"

#pragma clang fp contract(off)      // xh_j = x_j inv_j is ROUNDED before it is subtracted, in both kernels alike

namespace octic {

constexpr int KL_THREADS = 512;              // 8 waves; 8 elements a thread cover KL_DMAX in one step
constexpr int KL_WAVES = KL_THREADS / 64;
constexpr int KL_NMAX = 256;
constexpr int KL_DMAX = KL_THREADS * 8;
constexpr float KL_PDIST_EPS = 1e-8f;        // nn.PairwiseDistance(2, eps=1e-8) of the reference's constructor

static bool kl_ok(int64_t groups, int64_t n, int64_t D) {
  if (groups < 1 || n < 2 || n > KL_NMAX) return false;
  if (D < 8 || D > KL_DMAX || D % 8) return false;
  return groups <= 0x7FFFFFFFll / n;
}

// one wave: sum_k x[k]^2 (every lane gets it)
template <typename T>
__device__ __forceinline__ float kl_sumsq(const T* __restrict__ xr, int D, int lane) {
  float q = 0.f;
  for (int k = lane * 8; k < D; k += 512) {
    float v[8];
    load8<T>(xr + k, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) q = __builtin_fmaf(v[e], v[e], q);
  }
  return wave_total(q);
}
__device__ __forceinline__ float kl_inv(float q, float eps) { return 1.0f / fmaxf(sqrtf(q), eps); }

// workgroup sum, waves in index order; every thread gets it
__device__ __forceinline__ float kl_block_sum(float v, float* red) {
  v = wave_total(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < KL_WAVES; ++i) s += red[i];
  __syncthreads();
  return s;
}

template <typename T>
__global__ __launch_bounds__(KL_THREADS) void koleo_fwd_kernel(const T* __restrict__ x, int64_t ldx, int n, int D, float eps,
                                                                float* __restrict__ term, int* __restrict__ nn,
                                                                float* __restrict__ inv, float* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float xh[KL_DMAX];
  __shared__ float red[KL_WAVES], best_v[KL_WAVES], best_inv[KL_WAVES];
  __shared__ int best_j[KL_WAVES];
  const int64_t row = blockIdx.x, g = row / n;
  const int i = (int)(row - g * n), lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T* xg = x + g * n * ldx;
  const T* xi = xg + i * ldx;
  const float inv_i = kl_inv(kl_sumsq<T>(xi, D, lane), eps);
  const int k0 = threadIdx.x * 8;
  if (k0 < D) {
    float v[8];
    load8<T>(xi + k0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= inv_i;
    store8<float>(xh + k0, v);
  }
  __syncthreads();

  float bv = -INFINITY, binv = 0.f;
  int bj = 0x7FFFFFFF;
  for (int j = w; j < n; j += KL_WAVES) {      // ascending inside a wave: a later row needs a strictly larger dot
    if (j == i) continue;
    const T* xj = xg + j * ldx;
    float s = 0.f, q = 0.f;
    for (int k = lane * 8; k < D; k += 512) {
      float v[8], a[8];
      load8<T>(xj + k, v);
      load8<float>(xh + k, a);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s = __builtin_fmaf(a[e], v[e], s);
        q = __builtin_fmaf(v[e], v[e], q);
      }
    }
    s = wave_total(s);
    q = wave_total(q);
    const float ij = kl_inv(q, eps);
    float d = ij > 0.f ? s * ij : 0.f;         // ij == 0: ||x_j||^2 overflowed, xh_j is the zero row
    if (!(d == d)) d = -INFINITY;
    if (d > bv || bj == 0x7FFFFFFF) { bv = d; bj = j; binv = ij; }
  }
  if (lane == 0) { best_v[w] = bv; best_j[w] = bj; best_inv[w] = binv; }
  __syncthreads();
  bv = best_v[0]; bj = best_j[0]; binv = best_inv[0];
#pragma unroll
  for (int u = 1; u < KL_WAVES; ++u) {         // a wave without rows holds (-inf, INT_MAX) and loses every tie
    const float v = best_v[u];
    const int j = best_j[u];
    if (v > bv || (v == bv && j < bj)) { bv = v; bj = j; binv = best_inv[u]; }
  }

  float acc = 0.f;
  if (k0 < D) {
    float v[8], a[8];
    load8<T>(xg + bj * ldx + k0, v);
    load8<float>(xh + k0, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float df = (a[e] - v[e] * binv) + KL_PDIST_EPS;
      acc = __builtin_fmaf(df, df, acc);
    }
  }
  const float d = sqrtf(kl_block_sum(acc, red));
  if (threadIdx.x == 0) {
    term[row] = -logf(d + eps);
    nn[row] = bj;
    inv[row] = inv_i;
    dist[row] = d;
  }
}

template <typename T>
__global__ __launch_bounds__(KL_THREADS) void koleo_bwd_kernel(const T* __restrict__ x, int64_t ldx, int n, int D, float eps,
                                                                const float* __restrict__ gterm, const int* __restrict__ nn,
                                                                const float* __restrict__ inv, const float* __restrict__ dist,
                                                                T* __restrict__ dx, int64_t lddx) {
  __shared__ int snn[KL_NMAX];
  __shared__ float red[KL_WAVES];
  const int64_t row = blockIdx.x, g = row / n, base = g * n;
  const int i = (int)(row - base), lane = threadIdx.x & 63;
  const T* xg = x + base * ldx;
  const T* xi = xg + i * ldx;
  for (int j = threadIdx.x; j < n; j += KL_THREADS) snn[j] = nn[base + j];
  const float nrm = sqrtf(kl_sumsq<T>(xi, D, lane));      // which side of the clamp the row is on, as the forward saw it
  const float inv_i = inv[row];
  const int k0 = threadIdx.x * 8;
  const bool act = k0 < D;
  float xhi[8] = {0, 0, 0, 0, 0, 0, 0, 0}, G[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (act) {
    load8<T>(xi + k0, xhi);
#pragma unroll
    for (int e = 0; e < 8; ++e) xhi[e] *= inv_i;
  }
  {
    int I = nn[row];
    I = I < 0 ? 0 : (I >= n ? n - 1 : I);                  // indices are the forward's; a foreign value must not leave the group
    const float d = dist[row], c = -gterm[row] / (d + eps), inv_I = inv[base + I];
    if (act) {
      float v[8];
      load8<T>(xg + I * ldx + k0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) G[e] = c * (((xhi[e] - v[e] * inv_I) + KL_PDIST_EPS) / d);
    }
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {                            // the rows whose neighbour is row i, ascending
    if (snn[j] != i) continue;
    const float d = dist[base + j], c = -gterm[base + j] / (d + eps), inv_j = inv[base + j];
    if (act) {
      float v[8];
      load8<T>(xg + j * ldx + k0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) G[e] = G[e] - c * (((v[e] * inv_j - xhi[e]) + KL_PDIST_EPS) / d);
    }
  }
  float p = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) p = __builtin_fmaf(xhi[e], G[e], p);
  p = kl_block_sum(p, red);
  if (act) {
    float o[8];
    if (nrm >= eps) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (G[e] - xhi[e] * p) * inv_i;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = G[e] / eps;
    }
    store8<T>(dx + row * lddx + k0, o);
  }
}

static bool kl_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static int kl_check(const void* x, int dtype, int64_t ldx, int64_t groups, int64_t n, int64_t D) {
  if (!x) return OCTIC_ENULL;
  if (dtype != OCTIC_BF16 && dtype != OCTIC_F32) return OCTIC_EDTYPE;
  if (!kl_ok(groups, n, D) || ldx < D) return OCTIC_ESHAPE;
  if (kl_misaligned(x) || ((ldx * elem_size(dtype)) & 15)) return OCTIC_EALIGN;
  return OCTIC_OK;
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_koleo_ok(int64_t groups, int64_t n, int64_t D) { return kl_ok(groups, n, D) ? 1 : 0; }

int octic_koleo_fwd(const void* x, int x_dtype, int64_t ldx, int64_t groups, int64_t n, int64_t D, float eps, float* term,
                    int32_t* nn, float* inv, float* dist, void* stream) {
  if (!term || !nn || !inv || !dist) return OCTIC_ENULL;
  if (int e = kl_check(x, x_dtype, ldx, groups, n, D)) return e;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(groups * n));
  if (x_dtype == OCTIC_BF16)
    koleo_fwd_kernel<bf16><<<grid, dim3(KL_THREADS), 0, st>>>((const bf16*)x, ldx, (int)n, (int)D, eps, term, nn, inv, dist);
  else
    koleo_fwd_kernel<float><<<grid, dim3(KL_THREADS), 0, st>>>((const float*)x, ldx, (int)n, (int)D, eps, term, nn, inv, dist);
  return launch_status();
}

int octic_koleo_bwd(const void* x, int x_dtype, int64_t ldx, int64_t groups, int64_t n, int64_t D, float eps,
                    const float* gterm, const int32_t* nn, const float* inv, const float* dist, void* dx, int64_t lddx,
                    void* stream) {
  if (!gterm || !nn || !inv || !dist || !dx) return OCTIC_ENULL;
  if (int e = kl_check(x, x_dtype, ldx, groups, n, D)) return e;
  if (lddx < D) return OCTIC_ESHAPE;
  if (kl_misaligned(dx) || ((lddx * elem_size(x_dtype)) & 15)) return OCTIC_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(groups * n));
  if (x_dtype == OCTIC_BF16)
    koleo_bwd_kernel<bf16><<<grid, dim3(KL_THREADS), 0, st>>>((const bf16*)x, ldx, (int)n, (int)D, eps, gterm, nn, inv, dist,
                                                             (bf16*)dx, lddx);
  else
    koleo_bwd_kernel<float><<<grid, dim3(KL_THREADS), 0, st>>>((const float*)x, ldx, (int)n, (int)D, eps, gterm, nn, inv, dist,
                                                              (float*)dx, lddx);
  return launch_status();
}

}  // extern "C"
