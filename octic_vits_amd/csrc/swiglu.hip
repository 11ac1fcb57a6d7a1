// The gate of DINOv2's SwiGLU FFN (dinov2/layers/swiglu_ffn.py: x1, x2 = w12(x).chunk(2, -1); hidden = silu(x1) * x2) and
// its backward, as two bf16 row kernels with f32 arithmetic.  x12 is the [rows, 2H] output of the w12 GEMM: columns
// [0, H) are the gate x1, [H, 2H) the value x2.  Both kernels are HBM-bound (forward 6 bytes per element of a, backward
// 10) and follow dense_gelu_bwd_kernel (csrc/dense.hip): a workgroup is 64 column chunks (8 columns = 16 bytes each) x 4
// row phases and walks a strip of rows two at a time, so a lane has four (forward) or six (backward) independent 16-byte
// loads in flight.  The backward leaves, on the side, the column sums of dx12 (the bias gradient of w12) as slabs in a
// fixed order, summing the STORED bf16 values - what the GEMMs downstream see.
#include "octic_common.hpp"

namespace octic {

constexpr int kSwigluRowBlocks = 256;    // x 8 column blocks at H = 4096: 8 waves per SIMD's worth of work in flight

// sigmoid through 1 / (1 + exp(-x)): exp overflows to +inf for x < -88.7 (rcp(inf) = 0) and underflows to 0 for large x
// (rcp(1) = 1) - never inf / inf.  For x >= 17 the sum rounds to 1 and the result is exactly 1.
__device__ __forceinline__ float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

__device__ __forceinline__ bf16x8 swiglu_gate(bf16x8 x1, bf16x8 x2) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = (float)x1[e];
    o[e] = (bf16)((a * sigmoidf(a)) * (float)x2[e]);
  }
  return o;
}

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const bf16* __restrict__ x12, long ld12, bf16* __restrict__ a,
                                                         long lda, long rows, int H) {
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cl) * 8;
  const long per = (rows + kSwigluRowBlocks - 1) / kSwigluRowBlocks;
  const long r0 = (long)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  if (col >= H) return;
  long r = r0 + ph;
  for (; r + 4 < r1; r += 8) {            // two rows per trip: four 16-byte loads in flight per lane
    const bf16* p0 = x12 + r * ld12 + col;
    const bf16* p1 = x12 + (r + 4) * ld12 + col;
    const bf16x8 g0 = *(const bf16x8*)p0, v0 = *(const bf16x8*)(p0 + H);
    const bf16x8 g1 = *(const bf16x8*)p1, v1 = *(const bf16x8*)(p1 + H);
    *(bf16x8*)(a + r * lda + col) = swiglu_gate(g0, v0);
    *(bf16x8*)(a + (r + 4) * lda + col) = swiglu_gate(g1, v1);
  }
  for (; r < r1; r += 4) {
    const bf16* p0 = x12 + r * ld12 + col;
    *(bf16x8*)(a + r * lda + col) = swiglu_gate(*(const bf16x8*)p0, *(const bf16x8*)(p0 + H));
  }
}

// One 8-column chunk of one row: dx1 = ga * x2 * silu'(x1) with silu'(x) = s (1 + x (1 - s)), dx2 = ga * silu(x1); the
// stored values are added to the lane's column sums.
__device__ __forceinline__ void swiglu_grad(bf16x8 x1, bf16x8 x2, bf16x8 ga, bf16x8& d1, bf16x8& d2, float acc[16]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = (float)x1[e], g = (float)ga[e];
    const float s = sigmoidf(a);
    d1[e] = (bf16)(g * ((float)x2[e] * (s * (1.0f + a * (1.0f - s)))));     // ga last: inf * 0 cannot arise from a huge ga
    d2[e] = (bf16)(g * (a * s));
    acc[e] += (float)d1[e];
    acc[8 + e] += (float)d2[e];
  }
}

__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const bf16* __restrict__ x12, long ld12, const bf16* __restrict__ ga,
                                                         long ldg, bf16* __restrict__ dx12, long ldd,
                                                         float* __restrict__ partials, long rows, int H) {
  __shared__ float red[4][64][16];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cl) * 8;
  const long per = (rows + kSwigluRowBlocks - 1) / kSwigluRowBlocks;
  const long r0 = (long)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  float acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (col < H) {
    long r = r0 + ph;
    for (; r + 4 < r1; r += 8) {          // two rows per trip: six 16-byte loads in flight per lane
      const bf16* p0 = x12 + r * ld12 + col;
      const bf16* p1 = x12 + (r + 4) * ld12 + col;
      const bf16x8 g0 = *(const bf16x8*)p0, v0 = *(const bf16x8*)(p0 + H), c0 = *(const bf16x8*)(ga + r * ldg + col);
      const bf16x8 g1 = *(const bf16x8*)p1, v1 = *(const bf16x8*)(p1 + H), c1 = *(const bf16x8*)(ga + (r + 4) * ldg + col);
      bf16x8 a0, b0, a1, b1;
      swiglu_grad(g0, v0, c0, a0, b0, acc);
      swiglu_grad(g1, v1, c1, a1, b1, acc);
      bf16* q0 = dx12 + r * ldd + col;
      bf16* q1 = dx12 + (r + 4) * ldd + col;
      *(bf16x8*)q0 = a0;
      *(bf16x8*)(q0 + H) = b0;
      *(bf16x8*)q1 = a1;
      *(bf16x8*)(q1 + H) = b1;
    }
    for (; r < r1; r += 4) {
      const bf16* p0 = x12 + r * ld12 + col;
      bf16x8 a0, b0;
      swiglu_grad(*(const bf16x8*)p0, *(const bf16x8*)(p0 + H), *(const bf16x8*)(ga + r * ldg + col), a0, b0, acc);
      bf16* q0 = dx12 + r * ldd + col;
      *(bf16x8*)q0 = a0;
      *(bf16x8*)(q0 + H) = b0;
    }
  }
  if (!partials) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) red[ph][cl][e] = acc[e];
  __syncthreads();
  if (ph == 0 && col < H) {               // slab [2H]: dx1 sums at col, dx2 sums at H + col - w12.bias order
    float* out = partials + (long)blockIdx.y * 2 * H + col;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      out[e] = (red[0][cl][e] + red[1][cl][e]) + (red[2][cl][e] + red[3][cl][e]);
      out[H + e] = (red[0][cl][8 + e] + red[1][cl][8 + e]) + (red[2][cl][8 + e] + red[3][cl][8 + e]);
    }
  }
}

// rows of H columns behind every (pointer, row stride) pair: 16-byte chunks need H, the strides and the bases on 8 elements
inline int swiglu_check(int64_t rows, int H) { return (rows < 0 || H <= 0 || (H & 7)) ? OCTIC_ESHAPE : OCTIC_OK; }

}  // namespace octic

using namespace octic;

extern "C" {

int octic_swiglu_blocks(void) { return kSwigluRowBlocks; }

int octic_swiglu_fwd(const void* x12, int64_t ld12, void* a, int64_t lda, int64_t rows, int H, void* stream) {
  if (rows == 0) return OCTIC_OK;
  if (!x12 || !a) return OCTIC_ENULL;
  if (int e = swiglu_check(rows, H)) return e;
  if (ld12 < 2 * (int64_t)H || lda < H) return OCTIC_ESHAPE;
  if (((ld12 | lda) & 7) || ((((uintptr_t)x12) | ((uintptr_t)a)) & 15)) return OCTIC_EALIGN;
  swiglu_fwd_kernel<<<dim3((H / 8 + 63) / 64, kSwigluRowBlocks), dim3(256), 0, (hipStream_t)stream>>>(
      (const bf16*)x12, (long)ld12, (bf16*)a, (long)lda, (long)rows, H);
  return launch_status();
}

int octic_swiglu_bwd(const void* x12, int64_t ld12, const void* ga, int64_t ldg, void* dx12, int64_t ldd, float* partials,
                     int64_t rows, int H, void* stream) {
  if (rows == 0) return OCTIC_OK;
  if (!x12 || !ga || !dx12) return OCTIC_ENULL;
  if (int e = swiglu_check(rows, H)) return e;
  if (ld12 < 2 * (int64_t)H || ldg < H || ldd < 2 * (int64_t)H) return OCTIC_ESHAPE;
  if (((ld12 | ldg | ldd) & 7) || ((((uintptr_t)x12) | ((uintptr_t)ga) | ((uintptr_t)dx12)) & 15)) return OCTIC_EALIGN;
  if (((uintptr_t)partials) & 3) return OCTIC_EALIGN;
  swiglu_bwd_kernel<<<dim3((H / 8 + 63) / 64, kSwigluRowBlocks), dim3(256), 0, (hipStream_t)stream>>>(
      (const bf16*)x12, (long)ld12, (const bf16*)ga, (long)ldg, (bf16*)dx12, (long)ldd, partials, (long)rows, H);
  return launch_status();
}

}  // extern "C"
