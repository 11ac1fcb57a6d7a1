// Linear depth head of the DINOv2 hub (dinov2/hub/depthers.py:36-67, hub/depth/decode_heads.py: BNHead + depth_pred) at patch
// resolution.  The reference concatenates [patch | class token] channels of 1 or 4 layers, upsamples that [B, 2 D layers, h, w]
// tensor u = 4 times bilinearly, projects it to 256 bins with a 1x1 convolution and takes relu + 0.1, the normalised
// expectation over the bins.  The projection and the resize are both linear and bilinear weights sum to 1 (clamped borders
// too), so conv(up(x)) = up(conv(x)), and the class-token half of the channels is one bias vector per image:
//   1. depth_cls_kernel    : cb[b, k] = bias[k] + sum_l cls_l[b, :] . Wc_l[k, :]            (one wave per (image, bin))
//   2. depth_logits_kernel : Lo[b, p, k] = sum_l P_l[b, p, :] . Wp_l[k, :] + cb[b, k]       (exact-f32 MFMA, 128 rows x 256 bins
//                            per workgroup, a workgroup never leaves its image; the token rows are read where the backbone
//                            left them: batch / row strides, no permute, no cat)
//   3. depth_expect_kernel : depth[b, y, x] = clamp(sum_k bins[k] z_k / sum_k z_k), z = relu(bilinear(Lo)) + 0.1
//                            (one wave per block of up to u^2 pixels between the same four cells, 4 bins per lane;
//                            [B, 256, u h, u w] never exists)
// Rounding (the header's arithmetic contract): cb is 64 per-lane fmaf chains (lane i takes the float4 columns i, i + 64, ... of
// layer 0, then of layer 1, ...) added by a butterfly (offsets 32, 16, 8, 4, 2, 1), plus the bias; a logit is layers * D / 64
// fmaf chains of 64 products each started from zero (layer by layer, ascending columns) added in that order, plus cb.  Both
// depend on (layers, D) alone.  No atomics.  All offsets are 64-bit.
#include "octic_common.hpp"

namespace octic {
namespace {

__device__ __forceinline__ f32x4 depth_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr int DEPTH_BINS = 256;
constexpr int DEPTH_ROWS = 128;   // patch rows per workgroup of the logits launch
constexpr int DEPTH_LD = 36;      // 32 k + 4: rows 16-byte aligned, a fragment read (16 rows x 4 k-quads) hits 64 banks
constexpr int DEPTH_NT = DEPTH_BINS / 16;

struct DepthLayers {
  const float* patch[4];
  int64_t ldb[4], ldr[4];   // batch and row strides of the patch rows, in floats
  const float* cls[4];
  int64_t cls_ldb[4];
};

// one wave per (image, bin), four per workgroup
__global__ __launch_bounds__(256) void depth_cls_kernel(DepthLayers L, int layers, int D, int64_t B, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ cb) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= B * DEPTH_BINS) return;                    // wave-uniform
  const int64_t b = item / DEPTH_BINS;
  const int k = (int)(item - b * DEPTH_BINS);
  const int64_t ldw = 2ll * D * layers;
  float s = 0.f;
  for (int l = 0; l < layers; ++l) {
    const float* c = L.cls[l] + b * L.cls_ldb[l];
    const float* wr = W + k * ldw + (2ll * l + 1) * D;   // the class-token half of layer l
    for (int d = 4 * lane; d < D; d += 256) {
      const f32x4 cv = *(const f32x4*)(c + d), wv = *(const f32x4*)(wr + d);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(cv[j], wv[j], s);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) cb[item] = s + bias[k];
}

// workgroup = 128 patch rows of ONE image x all 256 bins, 8 waves; wave v owns rows 16 v .. 16 v + 15 and every bin (16 tiles
// of 16 x 16): accumulator element e of tile ct in lane (r, q) is Lo[row 16 v + 4 q + e][bin 16 ct + r].  The staging is
// csrc/segeval.hip's seg_forward_kernel<16>: 32 columns per chunk through LDS, the next chunk's loads in flight under the MFMAs.
__global__ __launch_bounds__(512) void depth_logits_kernel(DepthLayers L, int layers, int D, int64_t hw, int tiles,
                                                           const float* __restrict__ W, const float* __restrict__ cb,
                                                           float* __restrict__ Lo) {
  __shared__ __attribute__((aligned(16))) float Xs[DEPTH_ROWS * DEPTH_LD];
  __shared__ __attribute__((aligned(16))) float Ws[DEPTH_BINS * DEPTH_LD];
  constexpr int NT = DEPTH_NT, SROWS = 64;               // rows per staging pass (512 threads, 8 float4 per row)
  constexpr int XP = DEPTH_ROWS / SROWS, WP = DEPTH_BINS / SROWS;
  const int64_t b = blockIdx.x / tiles;
  const int64_t p0 = (int64_t)(blockIdx.x - b * tiles) * DEPTH_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6, r = lane & 15, q = lane >> 4;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  const int64_t ldw = 2ll * D * layers;
  const int KT = layers * D;                             // the patch-half columns, layer after layer
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 fr[XP], wr[WP];
  auto fetch = [&](int kk) {
    const int l = kk / D, k0 = kk - l * D;
    const float* X = L.patch[l] + b * L.ldb[l] + k0 + sc4;
    const int64_t ldr = L.ldr[l];
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int64_t p = p0 + srow + SROWS * i;
      fr[i] = p < hw ? *(const f32x4*)(X + p * ldr) : zero;
    }
    const float* Wl = W + 2ll * l * D + k0 + sc4;
#pragma unroll
    for (int i = 0; i < WP; ++i) wr[i] = *(const f32x4*)(Wl + (int64_t)(srow + SROWS * i) * ldw);
  };
  f32x4 acc[NT], part[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = part[j] = zero;
  fetch(0);
  for (int kk = 0; kk < KT; kk += 32) {
    __syncthreads();                       // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < XP; ++i) *(f32x4*)(Xs + (srow + SROWS * i) * DEPTH_LD + sc4) = fr[i];
#pragma unroll
    for (int i = 0; i < WP; ++i) *(f32x4*)(Ws + (srow + SROWS * i) * DEPTH_LD + sc4) = wr[i];
    __syncthreads();
    if (kk + 32 < KT) fetch(kk + 32);      // in flight under the products
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const f32x4 a4 = *(const f32x4*)(Xs + (16 * v + r) * DEPTH_LD + 16 * j + 4 * q);
#pragma unroll
      for (int h = 0; h < 2; ++h) {        // the bin tiles in two halves: half the W fragments live at a time
        f32x4 b4[NT / 2];
#pragma unroll
        for (int ct = 0; ct < NT / 2; ++ct) b4[ct] = *(const f32x4*)(Ws + (16 * (ct + h * (NT / 2)) + r) * DEPTH_LD + 16 * j + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int ct = 0; ct < NT / 2; ++ct) part[ct + h * (NT / 2)] = depth_mfma16(a4[e], b4[ct][e], part[ct + h * (NT / 2)]);
      }
    }
    if (kk & 32) {                         // D % 64 == 0: every chain is 64 long and stays inside its layer
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        acc[ct] += part[ct];
        part[ct] = zero;
      }
    }
  }
  const float* cbb = cb + b * DEPTH_BINS;
  float* out = Lo + b * hw * DEPTH_BINS;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const float cv = cbb[16 * ct + r];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t p = p0 + 16 * v + 4 * q + e;
      if (p < hw) out[p * DEPTH_BINS + 16 * ct + r] = acc[ct][e] + cv;
    }
  }
}

// torch's upsample_bilinear2d source index for align_corners = False and an output of u n: src = (dst + 0.5) / u - 0.5,
// clamped below at 0; i0 = floor(src), i1 = min(i0 + 1, n - 1), l1 = src - i0 (u = 1, 2, 4: every step is exact in f32)
__device__ __forceinline__ void depth_source(int dst, float inv_u, int n, int& i0, int& i1, float& l1) {
  float src = inv_u * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  l1 = src - (float)i0;
}

// One wave per block of output pixels that lie between the same four source cells: block row by holds the rows
// u by - u / 2 .. u by - u / 2 + u - 1 that exist (h + 1 block rows for u = 2 | 4 - the first and the last are the clamped
// borders - and h for u = 1), columns alike, so the four cells - whole 1 KiB rows of Lo, lane i holds bins 4 i .. 4 i + 3 - are
// read once for up to u^2 pixels.  Per pixel the two sums share their butterfly: after the offset-32 exchange lanes 0 .. 31
// carry sum z and lanes 32 .. 63 carry sum bins z (each value still adds its partners at offsets 32, 16, 8, 4, 2, 1 in that
// order).  Pixel n of the block waits in lane n and the block is stored at the end.
__global__ __launch_bounds__(256) void depth_expect_kernel(const float* __restrict__ Lo, int64_t B, int h, int w, int u,
                                                           const float* __restrict__ bins, float lo, float hi,
                                                           float* __restrict__ depth) {
  const int lane = threadIdx.x & 63;
  const int H = u * h, Wd = u * w, half = u / 2;
  const int bh = u == 1 ? h : h + 1, bw = u == 1 ? w : w + 1;
  const int64_t per_image = (int64_t)bh * bw, total = B * per_image;
  const float inv_u = 1.f / (float)u;
  const f32x4 bv = *(const f32x4*)(bins + 4 * lane);
  for (int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < total; blk += (int64_t)gridDim.x * 4) {
    const int64_t b = blk / per_image;
    const int64_t rem = blk - b * per_image;
    const int by = (int)(rem / bw), bx = (int)(rem - (int64_t)by * bw);
    const int y0 = u * by - half < 0 ? 0 : u * by - half, y1 = u * by - half + u > H ? H : u * by - half + u;
    const int x0 = u * bx - half < 0 ? 0 : u * bx - half, x1 = u * bx - half + u > Wd ? Wd : u * bx - half + u;
    const int nx = x1 - x0;
    int i0, i1, j0, j1;
    float hl1, wl1;
    depth_source(y0, inv_u, h, i0, i1, hl1);             // every row of the block has these cells, only the weight moves
    depth_source(x0, inv_u, w, j0, j1, wl1);
    const float* base = Lo + b * h * w * DEPTH_BINS + 4 * lane;
    const f32x4 a00 = *(const f32x4*)(base + ((int64_t)i0 * w + j0) * DEPTH_BINS);
    const f32x4 a01 = *(const f32x4*)(base + ((int64_t)i0 * w + j1) * DEPTH_BINS);
    const f32x4 a10 = *(const f32x4*)(base + ((int64_t)i1 * w + j0) * DEPTH_BINS);
    const f32x4 a11 = *(const f32x4*)(base + ((int64_t)i1 * w + j1) * DEPTH_BINS);
    float mine = 0.f;
    int n = 0;
    for (int y = y0; y < y1; ++y) {
      int ti0, ti1;
      depth_source(y, inv_u, h, ti0, ti1, hl1);
      const float hl0 = 1.f - hl1;
      for (int x = x0; x < x1; ++x, ++n) {
        depth_source(x, inv_u, w, ti0, ti1, wl1);
        const float wl0 = 1.f - wl1;
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float val = hl0 * (wl0 * a00[j] + wl1 * a01[j]) + hl1 * (wl0 * a10[j] + wl1 * a11[j]);
          const float z = (val < 0.f ? 0.f : val) + 0.1f;    // NaN stays NaN, as torch.relu
          s += z;
          t = fmaf(bv[j], z, t);
        }
        const bool low = lane < 32;
        float r = (low ? s : t) + __shfl_xor(low ? t : s, 32);   // lanes 0 .. 31: s + s', lanes 32 .. 63: t + t'
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) r += __shfl_xor(r, o);
        float d = __shfl(r, 32) / __shfl(r, 0);
        d = d < lo ? lo : (d > hi ? hi : d);                 // torch.clamp: NaN passes through
        if (lane == n) mine = d;
      }
    }
    if (lane < n) depth[(b * H + y0 + lane / nx) * Wd + x0 + lane % nx] = mine;
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool depth_ok(int D, int layers, int n_bins, int upsample) {
  return D >= 64 && D <= 4096 && D % 64 == 0 && layers >= 1 && layers <= 4 && n_bins == DEPTH_BINS &&
         (upsample == 1 || upsample == 2 || upsample == 4);
}
inline int64_t depth_tiles(int64_t hw) { return (hw + DEPTH_ROWS - 1) / DEPTH_ROWS; }
inline bool depth_grid_ok(int64_t B, int h, int w, int upsample) {
  if (B < 1 || h < 1 || w < 1) return false;
  const int64_t hw = (int64_t)h * w;
  if (hw > 0x7FFFFFFFll / (upsample * upsample)) return false;          // an image's output pixels are an int
  if (B > 0x7FFFFFFFll / depth_tiles(hw)) return false;                  // workgroups of the logits launch
  if (B > 0x7FFFFFFFll / DEPTH_BINS * 4) return false;                   // workgroups of the class-token launch
  return true;
}
inline int64_t depth_expect_blocks(int64_t B, int h, int w, int upsample) {
  const int64_t waves = B * (upsample == 1 ? h : h + 1) * (upsample == 1 ? w : w + 1);   // one per pixel block
  const int64_t blocks = (waves + 3) / 4, cap = 32ll * device_cus();
  return blocks > cap ? cap : blocks;
}

}  // namespace
}  // namespace octic

using namespace octic;

extern "C" {

int octic_depth_ok(int D, int layers, int n_bins, int upsample) { return depth_ok(D, layers, n_bins, upsample) ? 1 : 0; }

int octic_depth_plan(int64_t B, int h, int w, int D, int layers, int n_bins, int upsample, int out[4]) {
  if (!out) return OCTIC_ENULL;
  if (!depth_ok(D, layers, n_bins, upsample) || !depth_grid_ok(B, h, w, upsample)) return OCTIC_ESHAPE;
  out[0] = DEPTH_ROWS;
  out[1] = (int)(B * depth_tiles((int64_t)h * w));
  out[2] = layers * D / 64;
  out[3] = (int)depth_expect_blocks(B, h, w, upsample);
  return OCTIC_OK;
}

int octic_depth_logits(const float* const* patch, const int64_t* patch_ldb, const int64_t* patch_ldr, const float* const* cls,
                       const int64_t* cls_ldb, int layers, int64_t B, int h, int w, int D, const float* W, const float* bias,
                       int n_bins, float* image_bias, float* Lo, void* stream) {
  if (!patch || !patch_ldb || !patch_ldr || !cls || !cls_ldb || !W || !bias || !image_bias || !Lo) return OCTIC_ENULL;
  if (!depth_ok(D, layers, n_bins, 1) || !depth_grid_ok(B, h, w, 1)) return OCTIC_ESHAPE;
  const int64_t hw = (int64_t)h * w;
  DepthLayers L = {};
  for (int l = 0; l < layers; ++l) {
    if (!patch[l] || !cls[l]) return OCTIC_ENULL;
    if (patch_ldr[l] < D || (B > 1 && (patch_ldb[l] < 0 || cls_ldb[l] < 0))) return OCTIC_ESHAPE;
    if ((((uintptr_t)patch[l]) & 15) || (((uintptr_t)cls[l]) & 15) || (patch_ldb[l] & 3) || (patch_ldr[l] & 3) || (cls_ldb[l] & 3))
      return OCTIC_EALIGN;
    L.patch[l] = patch[l]; L.ldb[l] = patch_ldb[l]; L.ldr[l] = patch_ldr[l];
    L.cls[l] = cls[l]; L.cls_ldb[l] = cls_ldb[l];
  }
  if ((((uintptr_t)W) & 15) || (((uintptr_t)Lo) & 15) || (((uintptr_t)image_bias) & 3) || (((uintptr_t)bias) & 3)) return OCTIC_EALIGN;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = depth_tiles(hw);
  depth_cls_kernel<<<dim3((unsigned)((B * DEPTH_BINS + 3) / 4)), 256, 0, st>>>(L, layers, D, B, W, bias, image_bias);
  depth_logits_kernel<<<dim3((unsigned)(B * tiles)), 512, 0, st>>>(L, layers, D, hw, (int)tiles, W, image_bias, Lo);
  return launch_status();
}

int octic_depth_expect(const float* Lo, int64_t B, int h, int w, int n_bins, int upsample, const float* bins, float min_depth,
                       float max_depth, float* depth, void* stream) {
  if (!Lo || !bins || !depth) return OCTIC_ENULL;
  if (!depth_ok(64, 1, n_bins, upsample) || !depth_grid_ok(B, h, w, upsample)) return OCTIC_ESHAPE;
  if ((((uintptr_t)Lo) & 15) || (((uintptr_t)bins) & 15) || (((uintptr_t)depth) & 3)) return OCTIC_EALIGN;
  depth_expect_kernel<<<dim3((unsigned)depth_expect_blocks(B, h, w, upsample)), 256, 0, (hipStream_t)stream>>>(
      Lo, B, h, w, upsample, bins, min_depth, max_depth, depth);
  return launch_status();
}

}  // extern "C"
