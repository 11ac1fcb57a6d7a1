// Device-side 3-Augment of the DeiT-III recipe on uint8 batches (deit/augment.py:90-123 behind the crop: horizontal flip, one of
// grayscale / solarize / Gaussian blur, ColorJitter, ToTensor, Normalize).  As in mixup.hip the host draws the per-sample
// parameters (octic_vits_amd/augment.py) and uploads them as one DEVICE table of octic_aug_row entries; the kernel reads nothing
// else about the draw, so one captured launch serves every replay.
//
// The arithmetic is PIL's, rounding for rounding (every stage rounds to uint8 where PIL does; the contract is spelled out in
// include/octic_hip.h and restated with numpy in tests/golden/augment_numpy.py):
//   load   : src[y][flip ? W-1-x : x], then grayscale (all channels = L) or solarize, per pixel
//   blur   : three extended-box passes along x, then three along y, 24-bit fixed point, uint8 between the passes; the box
//            constants r <= 1, ww, fw come from the table (the kernel is integer only), so three passes reach 6 pixels
//   jitter : up to three blends deg + f (v - deg) in table order, product and sum rounded separately (no FMA), clipped and
//            truncated.  Contrast blends towards the rounded mean of L over the WHOLE image as it is at that point of the chain
//   store  : uint8 [B,H,W,3], or f32 [B,3,H,W] = (v / 255 - mean[c]) / std[c] with two correctly rounded f32 divisions
//
// One kernel, instantiated twice.  A workgroup owns a 32 x 64 tile of one image (rows of 192 contiguous source bytes, 256
// contiguous output bytes per channel row); a blurred sample loads the tile with a 6-pixel halo into LDS (one dword per pixel:
// R | G << 8 | B << 16) and runs the six passes there between two buffers, clamping neighbours at the IMAGE border exactly as
// PIL does, so any H, W >= 1 works, lines shorter than the halo included.  The statistics instance replays the chain up to the
// contrast op and leaves sum(L) of its tile in partials[b][tile] (uint32; workgroups of samples without a contrast op leave at
// once); the output instance adds the partials of its image in index order (integers: exact) and finishes the chain.  No
// atomics; an eager call and a graph replay agree bit for bit.
#include "octic_common.hpp"

namespace octic {

typedef octic_aug_row AugRow;

constexpr int AT_H = 32, AT_W = 64, A_HALO = 6, A_THREADS = 256;
constexpr int AL_H = AT_H + 2 * A_HALO, AL_W = AT_W + 2 * A_HALO;

__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) outside [0, 1]: f32, separate product and sum, clip, truncate
__device__ __forceinline__ int aug_blend(float deg, int v, float f) {
  const float t = __fadd_rn(deg, __fmul_rn(f, (float)v - deg));
  return (int)fminf(fmaxf(t, 0.f), 255.f);
}

// the row of sample b with everything made safe: an unknown op (or a blur whose box radius is not 0 or 1) means "no op", a
// jitter entry that is no op or repeats an earlier one is skipped
__device__ __forceinline__ AugRow aug_row(const AugRow* __restrict__ table, int b) {
  AugRow r = table[b];
  if (r.op < 0 || r.op > 3 || (r.op == 3 && (r.blur_r < 0 || r.blur_r > 1))) r.op = 0;
  int seen = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int o = r.order[k];
    if (o < 0 || o > 2 || (seen >> o & 1)) r.order[k] = -1;
    else seen |= 1 << o;
  }
  return r;
}

__device__ __forceinline__ int aug_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one box pass over the whole LDS region; ALONG_X: neighbours along x, else along y.  (gx0, gy0) = image coordinates of the
// region's corner, rw x rh its size.  Neighbours are clamped to the image (PIL's edge rule), then to the region (only values
// that never reach the tile's interior are affected: the halo shrinks by r + 1 <= 2 per pass).
template <bool ALONG_X>
__device__ __forceinline__ void aug_box_pass(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int gx0, int gy0, int rw,
                                             int rh, int H, int W, int r, uint32_t ww, uint32_t fw) {
  for (int idx = threadIdx.x; idx < rw * rh; idx += A_THREADS) {
    const int ly = idx / rw, lx = idx - ly * rw;
    const int gy = gy0 + ly, gx = gx0 + lx;
    uint32_t o = 0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int g = ALONG_X ? gx : gy, g0 = ALONG_X ? gx0 : gy0, n = ALONG_X ? W : H, ln = ALONG_X ? rw : rh;
      uint32_t s0 = 0, s1 = 0, s2 = 0, e0 = 0, e1 = 0, e2 = 0;
#pragma unroll
      for (int d = -2; d <= 2; ++d) {
        if (d < -r - 1 || d > r + 1) continue;
        const int l = aug_clamp(aug_clamp(g + d, 0, n - 1) - g0, 0, ln - 1);
        const uint32_t p = in[ALONG_X ? ly * AL_W + l : l * AL_W + lx];
        if (d == -r - 1 || d == r + 1) {
          e0 += p & 255u; e1 += (p >> 8) & 255u; e2 += (p >> 16) & 255u;
        } else {
          s0 += p & 255u; s1 += (p >> 8) & 255u; s2 += (p >> 16) & 255u;
        }
      }
      const uint32_t o0 = (ww * s0 + fw * e0 + (1u << 23)) >> 24;
      const uint32_t o1 = (ww * s1 + fw * e1 + (1u << 23)) >> 24;
      const uint32_t o2 = (ww * s2 + fw * e2 + (1u << 23)) >> 24;
      o = (o0 & 255u) | ((o1 & 255u) << 8) | ((o2 & 255u) << 16);
    }
    out[ly * AL_W + lx] = o;
  }
}

__device__ __forceinline__ uint64_t aug_block_sum(uint64_t v, uint64_t* red) {   // every thread ends with the total
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// grid: B x tiles workgroups, tile t of sample b = blockIdx.x; tiles = tiles_y x tiles_x
template <bool STATS, bool OUT_U8>
__global__ __launch_bounds__(A_THREADS) void augment_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst,
                                                            const AugRow* __restrict__ table, float m0, float m1, float m2,
                                                            float d0, float d1, float d2, int H, int W, int tiles_x, int tiles,
                                                            uint32_t* __restrict__ partials) {
  __shared__ uint32_t buf[2][AL_H * AL_W];
  __shared__ uint64_t red[4];
  const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const AugRow row = aug_row(table, b);
  // the jitter ops this instance runs: all of them, or those in front of the contrast op
  int contrast_at = -1;
#pragma unroll
  for (int k = 3; k >= 0; --k)
    if (row.order[k] == 1) contrast_at = k;
  if (STATS && contrast_at < 0) return;
  const int nj = STATS ? contrast_at : 4;
  float mean_l = 0.f;
  if (!STATS && contrast_at >= 0) {
    uint64_t s = 0;
    for (int i = threadIdx.x; i < tiles; i += A_THREADS) s += partials[(int64_t)b * tiles + i];
    s = aug_block_sum(s, red);
    const uint64_t n = (uint64_t)H * (uint64_t)W;
    mean_l = (float)(int)((2 * s + n) / (2 * n));          // PIL: int(mean + 0.5)
  }

  const int halo = row.op == 3 ? A_HALO : 0;
  const int y0 = ty * AT_H, x0 = tx * AT_W;
  const int gy0 = y0 - halo, gx0 = x0 - halo, rh = AT_H + 2 * halo, rw = AT_W + 2 * halo;
  const uint8_t* img = src + (int64_t)b * H * W * 3;
  for (int idx = threadIdx.x; idx < rw * rh; idx += A_THREADS) {
    const int ly = idx / rw, lx = idx - ly * rw;
    const int gy = gy0 + ly, gx = gx0 + lx;
    uint32_t p = 0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const uint8_t* s = img + ((int64_t)gy * W + (row.flip ? W - 1 - gx : gx)) * 3;
      int r = s[0], g = s[1], bl = s[2];
      if (row.op == 1) {
        r = g = bl = aug_luma(r, g, bl);
      } else if (row.op == 2) {
        r = r < 128 ? r : 255 - r;
        g = g < 128 ? g : 255 - g;
        bl = bl < 128 ? bl : 255 - bl;
      }
      p = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)bl << 16);
    }
    buf[0][ly * AL_W + lx] = p;
  }
  __syncthreads();
  int cur = 0;
  if (row.op == 3) {
    const uint32_t ww = (uint32_t)row.blur_ww, fw = (uint32_t)row.blur_fw;
#pragma unroll 1
    for (int pass = 0; pass < 6; ++pass) {
      if (pass < 3) aug_box_pass<true>(buf[cur], buf[cur ^ 1], gx0, gy0, rw, rh, H, W, row.blur_r, ww, fw);
      else aug_box_pass<false>(buf[cur], buf[cur ^ 1], gx0, gy0, rw, rh, H, W, row.blur_r, ww, fw);
      cur ^= 1;
      __syncthreads();
    }
  }

  const float mean[3] = {m0, m1, m2}, sd[3] = {d0, d1, d2};
  uint32_t acc = 0;
  for (int idx = threadIdx.x; idx < AT_H * AT_W; idx += A_THREADS) {
    const int oy = idx / AT_W, ox = idx - oy * AT_W;
    const int gy = y0 + oy, gx = x0 + ox;
    if (gy >= H || gx >= W) continue;
    const uint32_t p = buf[cur][(oy + halo) * AL_W + ox + halo];
    int v[3] = {(int)(p & 255u), (int)((p >> 8) & 255u), (int)((p >> 16) & 255u)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = row.order[k];
      if (k >= nj || o < 0) continue;
      const float f = o == 0 ? row.brightness : (o == 1 ? row.contrast : row.saturation);
      const float deg = o == 0 ? 0.f : (o == 1 ? mean_l : (float)aug_luma(v[0], v[1], v[2]));
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = aug_blend(deg, v[c], f);
    }
    if (STATS) {
      acc += (uint32_t)aug_luma(v[0], v[1], v[2]);
    } else if (OUT_U8) {
      uint8_t* d = (uint8_t*)dst + (((int64_t)b * H + gy) * W + gx) * 3;
      d[0] = (uint8_t)v[0];
      d[1] = (uint8_t)v[1];
      d[2] = (uint8_t)v[2];
    } else {
      float* d = (float*)dst + (((int64_t)b * 3) * H + gy) * W + gx;
#pragma unroll
      for (int c = 0; c < 3; ++c) d[(int64_t)c * H * W] = ((float)v[c] / 255.0f - mean[c]) / sd[c];
    }
  }
  if (STATS) {
    const uint64_t s = aug_block_sum(acc, red);
    if (threadIdx.x == 0) partials[(int64_t)b * tiles + t] = (uint32_t)s;   // <= 2048 x 255
  }
}

static bool aug_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

static int64_t aug_tiles(int H, int W) { return (int64_t)((H + AT_H - 1) / AT_H) * ((W + AT_W - 1) / AT_W); }

}  // namespace octic

using namespace octic;

extern "C" {

int64_t octic_augment_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return OCTIC_ESHAPE;
  return aug_tiles(H, W) * B * 4;
}

int octic_augment_u8(const uint8_t* src, void* dst, int dtype_out, const octic_aug_row* table, float mean0, float mean1,
                     float mean2, float std0, float std1, float std2, int B, int H, int W, void* workspace, void* stream) {
  if (!src || !dst || !table || !workspace) return OCTIC_ENULL;
  if (B <= 0 || H <= 0 || W <= 0) return OCTIC_ESHAPE;
  if (dtype_out != OCTIC_F32 && dtype_out != OCTIC_U8) return OCTIC_EDTYPE;
  const int64_t n = (int64_t)H * W * 3;
  if (n >= 0x80000000ll) return OCTIC_ESHAPE;
  const int es = dtype_out == OCTIC_F32 ? 4 : 1;
  if ((((uintptr_t)dst) & (es - 1)) || (((uintptr_t)table) & 3) || (((uintptr_t)workspace) & 3)) return OCTIC_EALIGN;
  if (aug_overlap(src, n * B, dst, n * B * es)) return OCTIC_ESHAPE;
  const int64_t tiles = aug_tiles(H, W);
  if (tiles * B > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  const int tiles_x = (W + AT_W - 1) / AT_W;
  const dim3 grid((unsigned)(tiles * B));
  const hipStream_t st = (hipStream_t)stream;
  uint32_t* partials = (uint32_t*)workspace;
  augment_kernel<true, false><<<grid, A_THREADS, 0, st>>>(src, nullptr, table, mean0, mean1, mean2, std0, std1, std2, H, W,
                                                          tiles_x, (int)tiles, partials);
  if (dtype_out == OCTIC_U8)
    augment_kernel<false, true><<<grid, A_THREADS, 0, st>>>(src, dst, table, mean0, mean1, mean2, std0, std1, std2, H, W, tiles_x,
                                                            (int)tiles, partials);
  else
    augment_kernel<false, false><<<grid, A_THREADS, 0, st>>>(src, dst, table, mean0, mean1, mean2, std0, std1, std2, H, W,
                                                             tiles_x, (int)tiles, partials);
  return launch_status();
}

}  // extern "C"
