// The two orbit-based invariant maps (reference: octic_vits/d8_invariantization.py:142-210 MaxFilteringInvariant, :212-280
// CanonizationInvariant) without anything eightfold in HBM.
// The eight action matrices of D8 on the 8-tuple are signed permutations: the four one-dimensional irreps keep their place and
// change sign, the two E copies (x4, x5) and (x6, x7) transform alike - in place for e, rr, m, mrr and swapped for r, rrr, mr,
// mrrr.  The eight matrices touch 12 (i, j) pairs, so all eight products of a (row, reference) pair are signed sums of 12 dot
// products of length c.  With E_a = [x(4+a) | x(6+a)] (the packed E row a) and refE_b = [ref(4+b) | ref(6+b)] the 8 E partials
// pair up into the four dots Q_ab = E_a . refE_b of length 2c, so a tile holds 8 accumulators per element:
//   prod_g = ((((s0 P0 + s1 P1) + s2 P2) + s3 P3) + s4 Q[0][swap_g]) + s5 Q[1][1 - swap_g],   P_u = x_u . ref_u
// in the group order e, r, rr, rrr, m, mr, mrr, mrrr; the max keeps the lowest index among equals and the first NaN.
// Operands are the compute dtype T (bf16 on v_mfma_f32_16x16x32_bf16, f32 on the exact v_mfma_f32_16x16x4_f32); partials,
// signed sums and comparisons are f32.  A workgroup of 4 waves owns a 64 x 64 tile, wave w the 16 left-operand rows 16 w ..;
// the reduction runs in chunks of 32 through LDS images [64][32] (row stride 40 bf16 / 36 f32), tails zero-filled.
//   forward    rows x references, reduction over c:  x and the prepared component planes [8][R][c] are both reduction-contiguous
//   backward x rows x channels,   reduction over R:  the signed cotangent g * A_idx[i, j] is formed while its image is staged,
//              the planes are transposed into LDS; one pass per (i, j) pair (E rows: two passes of width 2c each)
//   backward references  references x channels, reduction over the M rows in row slabs: f32 partials [slab][R][8c] in the
//              workspace, then a fixed-order sum over the slabs that also writes the [R, c, 8] layout.  No atomics.
// A row of out / idx / dx reads only that row of x and g: results do not depend on batch mates or position.
// Canonization is a row kernel pair (one wave per row): 8 partial dots with reference[8c], the same signed sums and winner
// rule, then out = A_idx x as a signed copy; the backward is the inverse signed permutation of the cotangent.
#include "octic_common.hpp"

namespace octic {
namespace {

constexpr int OI_T = 64, OI_BK = 32;
constexpr int OI_MAX_SLABS = 8, OI_SLAB_MIN = 256;

// bit 8 u + g set: the sign of unit u (0 .. 3: x0 .. x3, 4: E row 0, 5: E row 1) under group element g is negative
constexpr unsigned long long kOrbitNeg = 0x0000CC965AAAF000ull;
constexpr unsigned kOrbitSwap = 0xAA;      // bit g: the element exchanges the two rows of an E copy
__device__ __forceinline__ bool orbit_neg(int u, int g) { return (kOrbitNeg >> (8 * u + g)) & 1; }
__device__ __forceinline__ bool orbit_swap(int g) { return (kOrbitSwap >> g) & 1; }
__device__ __forceinline__ float orbit_sign(int u, int g) { return orbit_neg(u, g) ? -1.f : 1.f; }

template <typename T> struct Tr;
template <> struct Tr<bf16> {
  typedef bf16x8 vec;
  static constexpr int VE = 8, LD = 40;
};
template <> struct Tr<float> {
  typedef f32x4 vec;
  static constexpr int VE = 4, LD = 36;
};

// acc += A-block (16 rows of `a` from a_row: register e of lane (r, q) is row 4 q + e) x B-block (lane r is row b_row + r)
__device__ __forceinline__ f32x4 oi_mma(const bf16* a, const bf16* b, int q, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(a + 8 * q), *(const bf16x8*)(b + 8 * q), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4 oi_mma(const float* a, const float* b, int q, f32x4 acc) {
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const f32x4 av = *(const f32x4*)(a + 16 * jj + 4 * q), bv = *(const f32x4*)(b + 16 * jj + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc, 0, 0, 0);
  }
  return acc;
}

// One image [64][32] from a reduction-contiguous source: src(row, k) is the address of 16 bytes or nullptr (zeros).
template <typename T, typename F>
__device__ __forceinline__ void oi_stage_rows(T* img, F src) {
  typedef typename Tr<T>::vec vec;
  constexpr int VE = Tr<T>::VE, VPR = OI_BK / VE, NV = OI_T * VPR / 256;
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    const int v = threadIdx.x + 256 * h, row = v / VPR, k = (v % VPR) * VE;
    const T* p = src(row, k);
    vec val = {};
    if (p) val = *(const vec*)p;
    *(vec*)(img + row * Tr<T>::LD + k) = val;
  }
}
// One image [64][32] from a reduction-major source: src(k, col) is the address of 16 bytes (VE consecutive columns) or nullptr.
template <typename T, typename F>
__device__ __forceinline__ void oi_stage_cols(T* img, F src) {
  typedef typename Tr<T>::vec vec;
  constexpr int VE = Tr<T>::VE, VPC = OI_T / VE, NV = OI_BK * VPC / 256;
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    const int v = threadIdx.x + 256 * h, k = v / VPC, col = (v % VPC) * VE;
    const T* p = src(k, col);
    vec val = {};
    if (p) val = *(const vec*)p;
#pragma unroll
    for (int e = 0; e < VE; ++e) img[(col + e) * Tr<T>::LD + k] = val[e];
  }
}

// x: address of element k of unit u (0 .. 3, 4 = E row 0, 5 = E row 1) of row t
template <typename T>
__device__ __forceinline__ const T* oi_x(const View& v, int64_t t, int u, int k, int c) {
  return u < 4 ? (const T*)v.p[u] + t * v.ld[u] + k : (const T*)v.p[4] + t * v.ld[4] + (u - 4) * 2 * c + k;
}
// planes [8][R][c]: address of element k of unit u of reference d (E units: [ref(4 + b) | ref(6 + b)])
template <typename T>
__device__ __forceinline__ const T* oi_ref(const T* planes, int64_t d, int u, int k, int64_t R, int c) {
  int plane = u;
  if (u >= 4 && k >= c) {
    plane = u + 2;
    k -= c;
  }
  return planes + ((int64_t)plane * R + d) * c + k;
}

__device__ __forceinline__ void orbit_pick(const float p[8], float& best, int& bi) {
  best = p[0];
  bi = 0;
#pragma unroll
  for (int g = 1; g < 8; ++g)
    if (best == best && (p[g] > best || p[g] != p[g])) {
      best = p[g];
      bi = g;
    }
}
// the 8 signed sums of (P0 .. P3, Q[a][b]): q_swap[a] is the E partial row a takes under a swapping element
__device__ __forceinline__ void orbit_sums(const float P[4], const float q_keep[2], const float q_swap[2], float prod[8]) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const bool sw = (kOrbitSwap >> g) & 1;
    float s = orbit_sign(0, g) * P[0];
    s += orbit_sign(1, g) * P[1];
    s += orbit_sign(2, g) * P[2];
    s += orbit_sign(3, g) * P[3];
    s += orbit_sign(4, g) * (sw ? q_swap[0] : q_keep[0]);
    s += orbit_sign(5, g) * (sw ? q_swap[1] : q_keep[1]);
    prod[g] = s;
  }
}

// ------------------------------------------------------------------------------------------ MaxFiltering
template <typename T>
__global__ __launch_bounds__(256) void max_filter_prep_kernel(const float* __restrict__ ref, T* __restrict__ planes, int64_t R,
                                                              int c) {
  const int64_t n = R * c * 8, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i & 7);
  const int64_t dc = i >> 3;                   // d * c + cc
  planes[(int64_t)j * R * c + dc] = (T)ref[i];
}

template <typename T, typename TO>
__global__ __launch_bounds__(256) void max_filter_fwd_kernel(View x, const T* __restrict__ planes, TO* __restrict__ out,
                                                             uint8_t* __restrict__ idx, int64_t M, int64_t R, int c, int vec4) {
  constexpr int LD = Tr<T>::LD;
  __shared__ __attribute__((aligned(16))) T lds[4 * OI_T * LD];
  T* Xs[2] = {lds, lds + OI_T * LD};
  T* Rs[2] = {lds + 2 * OI_T * LD, lds + 3 * OI_T * LD};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * OI_T, d0 = (int64_t)blockIdx.y * OI_T;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 P[4][4], Q[2][2][4];                     // [unit][reference block], [E row of x][E row of ref][reference block]
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int b = 0; b < 4; ++b) P[u][b] = zero;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int k = 0; k < 4; ++k) Q[a][b][k] = zero;

#pragma unroll
  for (int ph = 0; ph < 3; ++ph) {               // units (0, 1), (2, 3), (E row 0, E row 1)
    const int K = ph < 2 ? c : 2 * c;
    for (int k0 = 0; k0 < K; k0 += OI_BK) {
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int u = 2 * ph + s;
        oi_stage_rows<T>(Xs[s], [&](int row, int k) -> const T* {
          return (t0 + row < M && k0 + k < K) ? oi_x<T>(x, t0 + row, u, k0 + k, c) : nullptr;
        });
        oi_stage_rows<T>(Rs[s], [&](int row, int k) -> const T* {
          return (d0 + row < R && k0 + k < K) ? oi_ref<T>(planes, d0 + row, u, k0 + k, R, c) : nullptr;
        });
      }
      __syncthreads();
      const T* xb[2] = {Xs[0] + (16 * w + r) * LD, Xs[1] + (16 * w + r) * LD};
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const T* ra[2] = {Rs[0] + (16 * b + r) * LD, Rs[1] + (16 * b + r) * LD};
        if (ph < 2) {
          P[2 * ph][b] = oi_mma(ra[0], xb[0], q, P[2 * ph][b]);
          P[2 * ph + 1][b] = oi_mma(ra[1], xb[1], q, P[2 * ph + 1][b]);
        } else {
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) Q[a][bb][b] = oi_mma(ra[bb], xb[a], q, Q[a][bb][b]);
        }
      }
    }
  }

  const int64_t t = t0 + 16 * w + r;
  if (t >= M) return;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int64_t db = d0 + 16 * b + 4 * q;
    if (db >= R) continue;
    TO ov[4];
    uint8_t iv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p4[4] = {P[0][b][e], P[1][b][e], P[2][b][e], P[3][b][e]};
      const float keep[2] = {Q[0][0][b][e], Q[1][1][b][e]}, swp[2] = {Q[0][1][b][e], Q[1][0][b][e]};
      float prod[8], best;
      int bi;
      orbit_sums(p4, keep, swp, prod);
      orbit_pick(prod, best, bi);
      ov[e] = (TO)best;
      iv[e] = (uint8_t)bi;
    }
    if (vec4) {                                  // R % 4 == 0 and aligned bases: the lane's four references are one store each
      typedef TO __attribute__((ext_vector_type(4))) to4;
      const to4 o4 = {ov[0], ov[1], ov[2], ov[3]};
      *(to4*)(out + t * R + db) = o4;
      *(unsigned*)(idx + t * R + db) = iv[0] | (iv[1] << 8) | (iv[2] << 16) | ((unsigned)iv[3] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (db + e < R) {
          out[t * R + db + e] = ov[e];
          idx[t * R + db + e] = iv[e];
        }
    }
  }
}

// 8 cotangents g[t, d .. d + 7] with their winners, signed for `unit` and kept where the winner's swap bit equals want_swap
// (want_swap < 0: every winner), as T into dst[8]; zeros behind row M - 1 / reference R - 1.
template <typename T>
__device__ __forceinline__ void oi_signed_g8(const T* __restrict__ g, const uint8_t* __restrict__ idx, int64_t t, int64_t d,
                                             int64_t M, int64_t R, int unit, int want_swap, T dst[8]) {
  float gv[8];
  unsigned char iv[8];
  const int64_t off = t * R + d;
  if (t < M && d + 8 <= R && !(R & 7)) {
    load8<T>(g + off, gv);
    const uint2 pk = *(const uint2*)(idx + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) iv[e] = (unsigned char)(((e < 4 ? pk.x : pk.y) >> (8 * (e & 3))) & 0xFF);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = t < M && d + e < R;
      gv[e] = in ? (float)g[off + e] : 0.f;
      iv[e] = in ? idx[off + e] : 0;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int gi = iv[e] & 7;
    const bool keep = want_swap < 0 || (int)orbit_swap(gi) == want_swap;
    dst[e] = (T)(keep ? (orbit_neg(unit, gi) ? -gv[e] : gv[e]) : 0.f);
  }
}
template <typename T>
__device__ __forceinline__ void oi_store8_lds(T* p, const T v[8]);
template <>
__device__ __forceinline__ void oi_store8_lds<bf16>(bf16* p, const bf16 v[8]) {
  bf16x8 a;
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = v[e];
  *(bf16x8*)p = a;
}
template <>
__device__ __forceinline__ void oi_store8_lds<float>(float* p, const float v[8]) {
  const f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  *(f32x4*)p = a;
  *(f32x4*)(p + 4) = b;
}

// blockIdx.y -> (unit, first column of the tile inside the unit); the unit is c (u < 4) or 2c (E rows) wide
__device__ __forceinline__ void oi_unit_of(int y, int c, int& u, int& col0) {
  const int t1 = (c + OI_T - 1) / OI_T, t2 = (2 * c + OI_T - 1) / OI_T;
  if (y < 4 * t1) {
    u = y / t1;
    col0 = (y % t1) * OI_T;
  } else {
    y -= 4 * t1;
    u = 4 + y / t2;
    col0 = (y % t2) * OI_T;
  }
}
inline int oi_unit_tiles(int c) { return 4 * ((c + OI_T - 1) / OI_T) + 2 * ((2 * c + OI_T - 1) / OI_T); }

template <typename T>
__global__ __launch_bounds__(256) void max_filter_bwd_x_kernel(const T* __restrict__ g, const uint8_t* __restrict__ idx,
                                                               const T* __restrict__ planes, View dx, int64_t M, int64_t R, int c) {
  constexpr int LD = Tr<T>::LD;
  __shared__ __attribute__((aligned(16))) T lds[2 * OI_T * LD];
  T* Gs = lds;
  T* Ws = lds + OI_T * LD;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * OI_T;
  int u, col0;
  oi_unit_of(blockIdx.y, c, u, col0);
  const int W = u < 4 ? c : 2 * c, passes = u < 4 ? 1 : 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero, zero, zero, zero};
  for (int p = 0; p < passes; ++p) {
    const int ru = u < 4 ? u : 4 + p;                           // the reference unit this pass multiplies by
    const int want = u < 4 ? -1 : (p ^ (u - 4));                // E row a reads refE_p under the winners with swap == (p != a)
    for (int64_t k0 = 0; k0 < R; k0 += OI_BK) {
      __syncthreads();
      {
        const int row = threadIdx.x >> 2, kk = (threadIdx.x & 3) * 8;
        T v8[8];
        oi_signed_g8<T>(g, idx, t0 + row, k0 + kk, M, R, u, want, v8);
        oi_store8_lds<T>(Gs + row * LD + kk, v8);
      }
      oi_stage_cols<T>(Ws, [&](int k, int col) -> const T* {
        return (k0 + k < R && col0 + col < W) ? oi_ref<T>(planes, k0 + k, ru, col0 + col, R, c) : nullptr;
      });
      __syncthreads();
      const T* gb = Gs + (16 * w + r) * LD;
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = oi_mma(Ws + (16 * b + r) * LD, gb, q, acc[b]);
    }
  }
  const int64_t t = t0 + 16 * w + r;
  if (t >= M) return;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int col = col0 + 16 * b + 4 * q;
    if (col >= W) continue;                                     // W is a multiple of 8: four columns are in or out together
    T* dst = (T*)oi_x<T>(dx, t, u, col, c);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = (T)acc[b][e];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void max_filter_bwd_ref_kernel(const T* __restrict__ g, const uint8_t* __restrict__ idx, View x,
                                                                 float* __restrict__ ws, int64_t M, int64_t R, int c,
                                                                 int slab_rows) {
  constexpr int LD = Tr<T>::LD;
  __shared__ __attribute__((aligned(16))) T lds[2 * OI_T * LD];
  T* Gs = lds;                                                  // [64 references][32 rows]
  T* Xs = lds + OI_T * LD;                                      // [64 channels][32 rows]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int64_t d0 = (int64_t)blockIdx.x * OI_T;
  int u, col0;
  oi_unit_of(blockIdx.y, c, u, col0);
  const int W = u < 4 ? c : 2 * c, passes = u < 4 ? 1 : 2;
  const int64_t rbeg = (int64_t)blockIdx.z * slab_rows, rend = rbeg + slab_rows < M ? rbeg + slab_rows : M;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero, zero, zero, zero};
  for (int p = 0; p < passes; ++p) {
    const int xu = u < 4 ? u : 4 + p;                           // refE_b sums E row a = p under the winners with swap == (a != b)
    const int want = u < 4 ? -1 : (p ^ (u - 4));
    for (int64_t k0 = rbeg; k0 < rend; k0 += OI_BK) {
      __syncthreads();
      {
        const int k = threadIdx.x >> 3, dd = (threadIdx.x & 7) * 8;   // 32 rows x 8 groups of 8 references
        T v8[8];
        oi_signed_g8<T>(g, idx, k0 + k, d0 + dd, rend, R, xu, want, v8);
#pragma unroll
        for (int e = 0; e < 8; ++e) Gs[(dd + e) * LD + k] = v8[e];
      }
      oi_stage_cols<T>(Xs, [&](int k, int col) -> const T* {
        return (k0 + k < rend && col0 + col < W) ? oi_x<T>(x, k0 + k, xu, col0 + col, c) : nullptr;
      });
      __syncthreads();
      const T* gb = Gs + (16 * w + r) * LD;
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = oi_mma(Xs + (16 * b + r) * LD, gb, q, acc[b]);
    }
  }
  const int64_t d = d0 + 16 * w + r;
  if (d >= R) return;
  float* dst = ws + ((int64_t)blockIdx.z * R + d) * (8 * c) + (u < 4 ? u * c : 4 * c + (u - 4) * 2 * c);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int col = col0 + 16 * b + 4 * q;
    if (col >= W) continue;
    *(f32x4*)(dst + col) = acc[b];
  }
}

// dref[d, cc, j] = sum over the slabs, in slab order, of ws[slab][d][slot(j) c + cc]   (slots: x0 x1 x2 x3 x4 x6 x5 x7)
__global__ __launch_bounds__(256) void max_filter_bwd_ref_finish_kernel(const float* __restrict__ ws, float* __restrict__ dref,
                                                                        int64_t R, int c, int slabs) {
  const int64_t n = R * c * 8, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i & 7);
  const int64_t dc = i >> 3, d = dc / c;
  const int cc = (int)(dc - d * c);
  const int slot = j < 4 ? j : (j == 4 ? 4 : (j == 5 ? 6 : (j == 6 ? 5 : 7)));
  const int64_t src = d * (8 * c) + slot * c + cc, stride = R * 8 * c;
  float s = ws[src];
  for (int z = 1; z < slabs; ++z) s += ws[z * stride + src];
  dref[i] = s;
}

struct OiSlabs {
  int slabs, slab_rows;
};
inline OiSlabs oi_slabs(int64_t M, int64_t R, int c) {
  const int64_t tiles = ((R + OI_T - 1) / OI_T) * oi_unit_tiles(c);
  int64_t want = 1024 / tiles, most = (M + OI_SLAB_MIN - 1) / OI_SLAB_MIN;
  if (most > OI_MAX_SLABS) most = OI_MAX_SLABS;
  int64_t slabs = want < most ? want : most;
  if (slabs < 1) slabs = 1;
  const int64_t rows = ((M + slabs - 1) / slabs + OI_BK - 1) / OI_BK * OI_BK;
  OiSlabs s = {(int)((M + rows - 1) / rows), (int)rows};
  return s;
}
inline int oi_check_shape(int64_t M, int64_t R, int c) {
  if (M < 1 || R < 1 || check_c(c) != OCTIC_OK) return OCTIC_ESHAPE;
  if (M >= ((int64_t)1 << 31) - OI_T || R * 8 * c >= ((int64_t)1 << 31) || (R + OI_T - 1) / OI_T > 65535 ||
      oi_unit_tiles(c) > 65535 || M * R >= ((int64_t)1 << 40))
    return OCTIC_ESHAPE;
  return OCTIC_OK;
}
inline bool oi_misaligned(const void* p) { return ((uintptr_t)p) & 15; }

// ------------------------------------------------------------------------------------------ Canonization
// One wave per row.  reference is i-major [8c]: dot_g = sum_i s_g[i] x_perm_g(i) . reference_i, so the E partials are
// Q[a][b] = E_a . refE_b with row a of x against row b of the reference - a swapping element reads Q[1][0] and Q[0][1].
template <typename T>
__device__ __forceinline__ float oi_round(float v);
template <>
__device__ __forceinline__ float oi_round<float>(float v) { return v; }
template <>
__device__ __forceinline__ float oi_round<bf16>(float v) { return (float)(bf16)v; }

template <typename T, typename TO>
__global__ __launch_bounds__(256) void canonize_fwd_kernel(View x, const float* __restrict__ ref, TO* __restrict__ out,
                                                           uint8_t* __restrict__ idx, int64_t M, int c) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= M) return;
  const T* xp[8];                                               // component j of the row
#pragma unroll
  for (int j = 0; j < 8; ++j) xp[j] = j < 4 ? oi_x<T>(x, t, j, 0, c) : oi_x<T>(x, t, 4 + (j & 1), (j >> 1) == 3 ? c : 0, c);
  float P[4] = {0.f, 0.f, 0.f, 0.f}, Q[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int cc = lane; cc < c; cc += 64) {
    float xv[8], rv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xv[j] = (float)xp[j][cc];
      rv[j] = oi_round<T>(ref[j * c + cc]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) P[u] = fmaf(xv[u], rv[u], P[u]);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) Q[a][b] = fmaf(xv[6 + a], rv[6 + b], fmaf(xv[4 + a], rv[4 + b], Q[a][b]));
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) P[u] = wave_total(P[u]);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) Q[a][b] = wave_total(Q[a][b]);
  const float keep[2] = {Q[0][0], Q[1][1]}, swp[2] = {Q[1][0], Q[0][1]};
  float prod[8], best;
  int bi;
  orbit_sums(P, keep, swp, prod);
  orbit_pick(prod, best, bi);
  if (lane == 0) idx[t] = (uint8_t)bi;
  const bool sw = orbit_swap(bi);
  TO* o = out + t * (8 * (int64_t)c);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int u = i < 4 ? i : 4 + (i & 1);
    const T* src = xp[(i >= 4 && sw) ? (i ^ 1) : i];
    const bool neg = orbit_neg(u, bi);
    for (int cc = lane; cc < c; cc += 64) {
      const float v = (float)src[cc];
      o[i * c + cc] = (TO)(neg ? -v : v);
    }
  }
}

template <typename T, typename TG>
__global__ __launch_bounds__(256) void canonize_bwd_kernel(const TG* __restrict__ g, const uint8_t* __restrict__ idx, View dx,
                                                           int64_t M, int c) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= M) return;
  const int bi = idx[t] & 7;
  const bool sw = orbit_swap(bi);
  const TG* gr = g + t * (8 * (int64_t)c);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int u = i < 4 ? i : 4 + (i & 1), j = (i >= 4 && sw) ? (i ^ 1) : i;   // out_i = s_i x_j, so dx_j = s_i g_i
    T* dst = (T*)(j < 4 ? oi_x<T>(dx, t, j, 0, c) : oi_x<T>(dx, t, 4 + (j & 1), (j >> 1) == 3 ? c : 0, c));
    const bool neg = orbit_neg(u, bi);
    for (int cc = lane; cc < c; cc += 64) {
      const float v = (float)gr[i * c + cc];
      dst[cc] = (T)(neg ? -v : v);
    }
  }
}

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_max_filter_prep(const float* references, void* planes, int64_t R, int c, int dtype, void* stream) {
  if (!references || !planes) return OCTIC_ENULL;
  if (dtype != OCTIC_F32 && dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  const int rc = oi_check_shape(1, R, c);
  if (rc != OCTIC_OK) return rc;
  if (oi_misaligned(references) || oi_misaligned(planes)) return OCTIC_EALIGN;
  const unsigned blocks = (unsigned)((R * c * 8 + 255) / 256);
  if (dtype == OCTIC_F32)
    hipLaunchKernelGGL(max_filter_prep_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, references, (float*)planes, R, c);
  else
    hipLaunchKernelGGL(max_filter_prep_kernel<bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, references, (bf16*)planes, R, c);
  return launch_status();
}

int octic_max_filter_fwd(const octic_view* x, const void* planes, void* out, uint8_t* idx, int64_t M, int64_t R, int c, int dtype,
                         int out_dtype, void* stream) {
  if (!x || !planes || !out || !idx) return OCTIC_ENULL;
  if ((dtype != OCTIC_F32 && dtype != OCTIC_BF16) || (out_dtype != OCTIC_F32 && out_dtype != OCTIC_BF16)) return OCTIC_EDTYPE;
  int rc = oi_check_shape(M, R, c);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(x, c, dtype)) != OCTIC_OK) return rc;
  if (oi_misaligned(planes)) return OCTIC_EALIGN;
  const dim3 grid((unsigned)((M + OI_T - 1) / OI_T), (unsigned)((R + OI_T - 1) / OI_T));
  hipStream_t s = (hipStream_t)stream;
  const int vec4 = !(R & 3) && !oi_misaligned(out) && !(((uintptr_t)idx) & 3);
  if (dtype == OCTIC_F32) {
    const View v = make_view<float>(x);
    if (out_dtype == OCTIC_F32)
      hipLaunchKernelGGL((max_filter_fwd_kernel<float, float>), grid, dim3(256), 0, s, v, (const float*)planes, (float*)out, idx, M, R, c, vec4);
    else
      hipLaunchKernelGGL((max_filter_fwd_kernel<float, bf16>), grid, dim3(256), 0, s, v, (const float*)planes, (bf16*)out, idx, M, R, c, vec4);
  } else {
    const View v = make_view<bf16>(x);
    if (out_dtype == OCTIC_F32)
      hipLaunchKernelGGL((max_filter_fwd_kernel<bf16, float>), grid, dim3(256), 0, s, v, (const bf16*)planes, (float*)out, idx, M, R, c, vec4);
    else
      hipLaunchKernelGGL((max_filter_fwd_kernel<bf16, bf16>), grid, dim3(256), 0, s, v, (const bf16*)planes, (bf16*)out, idx, M, R, c, vec4);
  }
  return launch_status();
}

int octic_max_filter_bwd_x(const void* g, const uint8_t* idx, const void* planes, const octic_view* dx, int64_t M, int64_t R, int c,
                           int dtype, void* stream) {
  if (!g || !idx || !planes || !dx) return OCTIC_ENULL;
  if (dtype != OCTIC_F32 && dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  int rc = oi_check_shape(M, R, c);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(dx, c, dtype)) != OCTIC_OK) return rc;
  if (oi_misaligned(planes) || oi_misaligned(g) || (((uintptr_t)idx) & 7)) return OCTIC_EALIGN;
  const dim3 grid((unsigned)((M + OI_T - 1) / OI_T), (unsigned)oi_unit_tiles(c));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OCTIC_F32)
    hipLaunchKernelGGL(max_filter_bwd_x_kernel<float>, grid, dim3(256), 0, s, (const float*)g, idx, (const float*)planes,
                       make_view<float>(dx), M, R, c);
  else
    hipLaunchKernelGGL(max_filter_bwd_x_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)g, idx, (const bf16*)planes,
                       make_view<bf16>(dx), M, R, c);
  return launch_status();
}

int octic_max_filter_bwd_ref_plan(int64_t M, int64_t R, int c, int out[4]) {
  const int rc = oi_check_shape(M, R, c);
  if (rc != OCTIC_OK) return rc;
  if (out) {
    const OiSlabs p = oi_slabs(M, R, c);
    out[0] = p.slabs;
    out[1] = p.slab_rows;
    out[2] = OI_T;
    out[3] = (int)((R + OI_T - 1) / OI_T) * oi_unit_tiles(c);
  }
  return OCTIC_OK;
}

int64_t octic_max_filter_bwd_ref_workspace_bytes(int64_t M, int64_t R, int c) {
  const int rc = oi_check_shape(M, R, c);
  if (rc != OCTIC_OK) return rc;
  return (int64_t)oi_slabs(M, R, c).slabs * R * 8 * c * 4;
}

int octic_max_filter_bwd_ref(const void* g, const uint8_t* idx, const octic_view* x, float* dref, void* workspace,
                             int64_t workspace_bytes, int64_t M, int64_t R, int c, int dtype, void* stream) {
  if (!g || !idx || !x || !dref || !workspace) return OCTIC_ENULL;
  if (dtype != OCTIC_F32 && dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  int rc = oi_check_shape(M, R, c);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(x, c, dtype)) != OCTIC_OK) return rc;
  if (oi_misaligned(g) || (((uintptr_t)idx) & 7) || oi_misaligned(dref) || oi_misaligned(workspace)) return OCTIC_EALIGN;
  const OiSlabs p = oi_slabs(M, R, c);
  if (workspace_bytes < (int64_t)p.slabs * R * 8 * c * 4) return OCTIC_EWORKSPACE;
  const dim3 grid((unsigned)((R + OI_T - 1) / OI_T), (unsigned)oi_unit_tiles(c), (unsigned)p.slabs);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OCTIC_F32)
    hipLaunchKernelGGL(max_filter_bwd_ref_kernel<float>, grid, dim3(256), 0, s, (const float*)g, idx, make_view<float>(x),
                       (float*)workspace, M, R, c, p.slab_rows);
  else
    hipLaunchKernelGGL(max_filter_bwd_ref_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)g, idx, make_view<bf16>(x),
                       (float*)workspace, M, R, c, p.slab_rows);
  hipLaunchKernelGGL(max_filter_bwd_ref_finish_kernel, dim3((unsigned)((R * c * 8 + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, dref, R, c, p.slabs);
  return launch_status();
}

int octic_canonize_fwd(const octic_view* x, const float* reference, void* out, uint8_t* idx, int64_t M, int c, int dtype,
                       int out_dtype, void* stream) {
  if (!x || !reference || !out || !idx) return OCTIC_ENULL;
  if ((dtype != OCTIC_F32 && dtype != OCTIC_BF16) || (out_dtype != OCTIC_F32 && out_dtype != OCTIC_BF16)) return OCTIC_EDTYPE;
  int rc = oi_check_shape(M, 1, c);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(x, c, dtype)) != OCTIC_OK) return rc;
  const dim3 grid((unsigned)((M + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OCTIC_F32) {
    const View v = make_view<float>(x);
    if (out_dtype == OCTIC_F32) hipLaunchKernelGGL((canonize_fwd_kernel<float, float>), grid, dim3(256), 0, s, v, reference, (float*)out, idx, M, c);
    else hipLaunchKernelGGL((canonize_fwd_kernel<float, bf16>), grid, dim3(256), 0, s, v, reference, (bf16*)out, idx, M, c);
  } else {
    const View v = make_view<bf16>(x);
    if (out_dtype == OCTIC_F32) hipLaunchKernelGGL((canonize_fwd_kernel<bf16, float>), grid, dim3(256), 0, s, v, reference, (float*)out, idx, M, c);
    else hipLaunchKernelGGL((canonize_fwd_kernel<bf16, bf16>), grid, dim3(256), 0, s, v, reference, (bf16*)out, idx, M, c);
  }
  return launch_status();
}

int octic_canonize_bwd(const void* g, int g_dtype, const uint8_t* idx, const octic_view* dx, int64_t M, int c, int dtype,
                       void* stream) {
  if (!g || !idx || !dx) return OCTIC_ENULL;
  if ((dtype != OCTIC_F32 && dtype != OCTIC_BF16) || (g_dtype != OCTIC_F32 && g_dtype != OCTIC_BF16)) return OCTIC_EDTYPE;
  int rc = oi_check_shape(M, 1, c);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(dx, c, dtype)) != OCTIC_OK) return rc;
  const dim3 grid((unsigned)((M + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OCTIC_F32) {
    const View v = make_view<float>(dx);
    if (g_dtype == OCTIC_F32) hipLaunchKernelGGL((canonize_bwd_kernel<float, float>), grid, dim3(256), 0, s, (const float*)g, idx, v, M, c);
    else hipLaunchKernelGGL((canonize_bwd_kernel<float, bf16>), grid, dim3(256), 0, s, (const bf16*)g, idx, v, M, c);
  } else {
    const View v = make_view<bf16>(dx);
    if (g_dtype == OCTIC_F32) hipLaunchKernelGGL((canonize_bwd_kernel<bf16, float>), grid, dim3(256), 0, s, (const float*)g, idx, v, M, c);
    else hipLaunchKernelGGL((canonize_bwd_kernel<bf16, bf16>), grid, dim3(256), 0, s, (const bf16*)g, idx, v, M, c);
  }
  return launch_status();
}

}  // extern "C"
