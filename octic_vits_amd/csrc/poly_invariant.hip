// The two polynomial invariant maps (reference: octic_vits/d8_invariantization.py:66-112 PolynomialInvariant, 32 generators of
// degree <= 5, and :114-141 ThirdOrderInvariant, 15 generators of degree 3) as one forward and one backward row kernel.
// The maps are element-wise over (row, column): a thread that holds x0 .. x7 of W adjacent columns of one row writes all P
// planes of those columns (forward) or, with the P cotangents, all eight input gradients (backward).  Nothing but x is read
// besides the cotangent; no atomics, no workspace, no LDS.
// Arithmetic.  The generators are the monomial strings of the Python tables, parsed at compile time ("356+347" = x3 x5 x6 +
// x3 x4 x7); a generator is evaluated with the expression tree of the Python composition: every monomial is the left-to-right
// product of its digits (the "0" prefix of the third-order degree-2 block first), terms are added / subtracted in table order,
// and every multiply and add is rounded on its own - contraction is OFF for this file, hipcc would otherwise fuse
// a*b + c*d into an fma.  The f32 output is therefore bit-identical to the composition on f32 inputs and the bf16 output is
// its round-to-nearest-even.  The digit order of the tables makes every generator invariant under the eight group elements
// bit for bit (see d8_invariantization.py); the strings below must stay equal to the Python ones, a host test compares them.
// Backward.  dx_i = sum_k g_k dp_k/dx_i, recomputed from x in registers.  The accumulation order is fixed: generators in
// plane order, the terms of a generator in table order, the distinct digits of a term in order of first appearance.  A term
// that holds x_i with multiplicity m adds  +-((prod of the term's digits with the first x_i removed, left to right) * m) * g_k
// to dx_i (the factor m only where m > 1): at most 3 + 1 + 1 rounded multiplies and one rounded add per term.
// Work split: item = (row, group of W columns), one item per thread, items of a row adjacent: the lanes of a wave store
// 64 W contiguous elements of a plane (less at a row end).  Offsets are 64-bit; the grid is not capped.  W = 4 forward
// (74 / 76 VGPRs polynomial f32 / bf16 output, 50 / 48 third order) and W = 2 backward (122 / 121 and 90 / 72 VGPRs): the
// backward keeps 8 W inputs, 8 W accumulators and the shared sub-products of ~170 terms alive; at W = 4 the polynomial
// backward needs 246 - 256 VGPRs (1 - 2 waves per SIMD) and measured 89 us against 55 us at W = 2 with a bf16 cotangent.
#include "octic_common.hpp"

#pragma clang fp contract(off)

namespace octic {
namespace {

// columns per thread, forward / backward: the choice and the register counts behind it are in NOTES, "Polynomial invariants"
constexpr int PI_WF = 4, PI_WB = 2;
constexpr int PI_MAX_TERMS = 2, PI_MAX_DEG = 5;

struct PiTerm {
  int sign, n;
  int d[PI_MAX_DEG];
};
struct PiGen {
  int nt;
  PiTerm t[PI_MAX_TERMS];
};

constexpr PiGen pi_parse(const char* prefix, const char* s) {
  PiGen g = {};
  int k = 0;
  while (*s) {
    PiTerm t = {};
    t.sign = 1;
    if (*s == '+') ++s;
    else if (*s == '-') {
      t.sign = -1;
      ++s;
    }
    for (const char* p = prefix; *p; ++p) t.d[t.n++] = *p - '0';
    while (*s >= '0' && *s <= '9') t.d[t.n++] = *s++ - '0';
    g.t[k++] = t;
  }
  g.nt = k;
  return g;
}

// MAP 0: PolynomialInvariant  [x0 | deg 2 (6) | deg 3 (8) | deg 4, 5 (17)];  MAP 1: ThirdOrderInvariant  [x0^3 | x0 deg 2 | deg 3]
template <int MAP> struct PiMap;
template <> struct PiMap<OCTIC_POLY_POLYNOMIAL> { static constexpr int P = 32; };
template <> struct PiMap<OCTIC_POLY_THIRD_ORDER> { static constexpr int P = 15; };

template <int MAP>
constexpr PiGen pi_gen(int k) {
  const char* const deg2[6] = {"66+77", "46+57", "44+55", "33", "22", "11"};
  // the strings of d8_invariantization._DEG2 / _DEG3 / _DEG4, digit for digit: the order of the digits is the order of the
  // multiplies, chosen there so that every generator is bitwise invariant under the eight group elements
  const char* const deg3[8] = {"673", "356+347", "453", "266-277", "246-257", "244-255", "156-147", "123"};
  const char* const deg4[17] = {"6666+7777", "4666+5777", "4466+5577", "4446+5557", "4444+5555", "2356-2347", "1366-1377",
                                "1346-1357", "1344-1355", "6712", "1256+1247", "4512", "16667-17776", "15666-14777",
                                "14566-15477", "14456-15547", "14445-15554"};
  if (k == 0) return pi_parse("", MAP == OCTIC_POLY_POLYNOMIAL ? "0" : "000");
  if (k < 7) return pi_parse(MAP == OCTIC_POLY_POLYNOMIAL ? "" : "0", deg2[k - 1]);
  if (k < 15) return pi_parse("", deg3[k - 7]);
  return pi_parse("", deg4[k - 15]);
}

template <typename T, int W> struct PiVec;
template <int W> struct PiVec<float, W> { typedef float __attribute__((ext_vector_type(W))) type; };
template <int W> struct PiVec<bf16, W> { typedef __bf16 __attribute__((ext_vector_type(W))) type; };

template <typename T, int W>
__device__ __forceinline__ void pi_load(const T* p, float (&v)[W]) {
  const typename PiVec<T, W>::type a = *(const typename PiVec<T, W>::type*)p;
#pragma unroll
  for (int e = 0; e < W; ++e) v[e] = (float)a[e];
}
template <typename T, int W>
__device__ __forceinline__ void pi_store(T* p, const float (&v)[W]) {
  typename PiVec<T, W>::type a;
#pragma unroll
  for (int e = 0; e < W; ++e) a[e] = (T)v[e];
  *(typename PiVec<T, W>::type*)p = a;
}

// element offset of component j (8-tuple index) of row m inside its view pointer; the packed E row is [x4 | x6 | x5 | x7]
__device__ __forceinline__ float* pi_x(const View& v, int64_t m, int j, int c) {
  return j < 4 ? (float*)v.p[j] + m * v.ld[j] : (float*)v.p[4] + m * v.ld[4] + (j & 1) * 2 * c + ((j - 4) >> 1) * c;
}

template <int W>
__device__ __forceinline__ void pi_load_x(const View& x, int64_t m, int col, int c, float (&xv)[8][W]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) pi_load<float, W>(pi_x(x, m, j, c) + col, xv[j]);
}

template <int MAP, int K, typename TO, int W>
__device__ __forceinline__ void pi_fwd_planes(const float (&xv)[8][W], TO* o, int c) {
  if constexpr (K < PiMap<MAP>::P) {
    constexpr PiGen G = pi_gen<MAP>(K);
    float r[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      float out = 0.f;
#pragma unroll
      for (int t = 0; t < G.nt; ++t) {
        float term = xv[G.t[t].d[0]][e];
#pragma unroll
        for (int j = 1; j < G.t[t].n; ++j) term = term * xv[G.t[t].d[j]][e];
        out = t == 0 ? term : (G.t[t].sign > 0 ? out + term : out - term);   // the first term of every generator is positive
      }
      r[e] = out;
    }
    pi_store<TO, W>(o + (int64_t)K * c, r);
    pi_fwd_planes<MAP, K + 1, TO, W>(xv, o, c);
  }
}

template <int MAP, typename TO>
__global__ __launch_bounds__(256) void poly_invariant_fwd_kernel(View x, TO* __restrict__ out, int64_t M, int c) {
  constexpr int W = PI_WF;
  const int cw = c / W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * cw) return;
  const int64_t m = idx / cw;
  const int col = (int)(idx - m * cw) * W;
  float xv[8][W];
  pi_load_x<W>(x, m, col, c, xv);
  pi_fwd_planes<MAP, 0, TO, W>(xv, out + m * ((int64_t)PiMap<MAP>::P * c) + col, c);
}

template <int MAP, int K, typename TG, int W>
__device__ __forceinline__ void pi_bwd_planes(const float (&xv)[8][W], const TG* g, int c, float (&acc)[8][W]) {
  if constexpr (K < PiMap<MAP>::P) {
    constexpr PiGen G = pi_gen<MAP>(K);
    float gv[W];
    pi_load<TG, W>(g + (int64_t)K * c, gv);
#pragma unroll
    for (int t = 0; t < G.nt; ++t) {
#pragma unroll
      for (int j = 0; j < G.t[t].n; ++j) {
        const int i = G.t[t].d[j];
        bool first = true;
        int mult = 0;
#pragma unroll
        for (int jj = 0; jj < G.t[t].n; ++jj) {
          if (G.t[t].d[jj] == i) {
            ++mult;
            if (jj < j) first = false;
          }
        }
        if (!first) continue;
#pragma unroll
        for (int e = 0; e < W; ++e) {
          float v = 1.f;
          bool any = false;
#pragma unroll
          for (int jj = 0; jj < G.t[t].n; ++jj) {
            if (jj == j) continue;
            v = any ? v * xv[G.t[t].d[jj]][e] : xv[G.t[t].d[jj]][e];
            any = true;
          }
          if (mult > 1) v = v * (float)mult;
          v = any ? v * gv[e] : gv[e];
          acc[i][e] = G.t[t].sign > 0 ? acc[i][e] + v : acc[i][e] - v;
        }
      }
    }
    pi_bwd_planes<MAP, K + 1, TG, W>(xv, g, c, acc);
  }
}

template <int MAP, typename TG>
__global__ __launch_bounds__(256) void poly_invariant_bwd_kernel(const TG* __restrict__ g, View x, View dx, int64_t M, int c) {
  constexpr int W = PI_WB;
  const int cw = c / W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * cw) return;
  const int64_t m = idx / cw;
  const int col = (int)(idx - m * cw) * W;
  float xv[8][W], acc[8][W];
  pi_load_x<W>(x, m, col, c, xv);
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int e = 0; e < W; ++e) acc[j][e] = 0.f;
  pi_bwd_planes<MAP, 0, TG, W>(xv, g + m * ((int64_t)PiMap<MAP>::P * c) + col, c, acc);
#pragma unroll
  for (int j = 0; j < 8; ++j) pi_store<float, W>(pi_x(dx, m, j, c) + col, acc[j]);
}

inline int pi_check(int64_t M, int c, int map) {
  if (M < 1 || check_c(c) != OCTIC_OK || (map != OCTIC_POLY_POLYNOMIAL && map != OCTIC_POLY_THIRD_ORDER)) return OCTIC_ESHAPE;
  // one thread per item in a 1-d grid of 256-thread blocks: fewer than 2^31 items, and M * P * c far inside int64
  constexpr int wmin = PI_WF < PI_WB ? PI_WF : PI_WB;
  if (M > (((int64_t)1 << 31) - 1) / (c / wmin)) return OCTIC_ESHAPE;
  return OCTIC_OK;
}
inline dim3 pi_grid(int64_t M, int c, int w) { return dim3((unsigned)((M * (c / w) + 255) / 256)); }

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_poly_invariant_fwd(const octic_view* x, void* out, int64_t M, int c, int map, int out_dtype, void* stream) {
  if (!x || !out) return OCTIC_ENULL;
  if (out_dtype != OCTIC_F32 && out_dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  int rc = pi_check(M, c, map);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(x, c, OCTIC_F32)) != OCTIC_OK) return rc;
  if (((uintptr_t)out) & 15) return OCTIC_EALIGN;
  const View v = make_view<float>(x);
  const dim3 grid = pi_grid(M, c, PI_WF);
  hipStream_t s = (hipStream_t)stream;
  if (map == OCTIC_POLY_POLYNOMIAL) {
    if (out_dtype == OCTIC_F32) hipLaunchKernelGGL((poly_invariant_fwd_kernel<OCTIC_POLY_POLYNOMIAL, float>), grid, dim3(256), 0, s, v, (float*)out, M, c);
    else hipLaunchKernelGGL((poly_invariant_fwd_kernel<OCTIC_POLY_POLYNOMIAL, bf16>), grid, dim3(256), 0, s, v, (bf16*)out, M, c);
  } else {
    if (out_dtype == OCTIC_F32) hipLaunchKernelGGL((poly_invariant_fwd_kernel<OCTIC_POLY_THIRD_ORDER, float>), grid, dim3(256), 0, s, v, (float*)out, M, c);
    else hipLaunchKernelGGL((poly_invariant_fwd_kernel<OCTIC_POLY_THIRD_ORDER, bf16>), grid, dim3(256), 0, s, v, (bf16*)out, M, c);
  }
  return launch_status();
}

int octic_poly_invariant_bwd(const void* g, int g_dtype, const octic_view* x, const octic_view* dx, int64_t M, int c, int map,
                             void* stream) {
  if (!g || !x || !dx) return OCTIC_ENULL;
  if (g_dtype != OCTIC_F32 && g_dtype != OCTIC_BF16) return OCTIC_EDTYPE;
  int rc = pi_check(M, c, map);
  if (rc != OCTIC_OK) return rc;
  if ((rc = check_view(x, c, OCTIC_F32)) != OCTIC_OK || (rc = check_view(dx, c, OCTIC_F32)) != OCTIC_OK) return rc;
  if (((uintptr_t)g) & 15) return OCTIC_EALIGN;
  const View vx = make_view<float>(x), vd = make_view<float>(dx);
  const dim3 grid = pi_grid(M, c, PI_WB);
  hipStream_t s = (hipStream_t)stream;
  if (map == OCTIC_POLY_POLYNOMIAL) {
    if (g_dtype == OCTIC_F32) hipLaunchKernelGGL((poly_invariant_bwd_kernel<OCTIC_POLY_POLYNOMIAL, float>), grid, dim3(256), 0, s, (const float*)g, vx, vd, M, c);
    else hipLaunchKernelGGL((poly_invariant_bwd_kernel<OCTIC_POLY_POLYNOMIAL, bf16>), grid, dim3(256), 0, s, (const bf16*)g, vx, vd, M, c);
  } else {
    if (g_dtype == OCTIC_F32) hipLaunchKernelGGL((poly_invariant_bwd_kernel<OCTIC_POLY_THIRD_ORDER, float>), grid, dim3(256), 0, s, (const float*)g, vx, vd, M, c);
    else hipLaunchKernelGGL((poly_invariant_bwd_kernel<OCTIC_POLY_THIRD_ORDER, bf16>), grid, dim3(256), 0, s, (const bf16*)g, vx, vd, M, c);
  }
  return launch_status();
}

}  // extern "C"
