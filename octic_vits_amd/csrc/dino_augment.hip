// DINOv2's multi-crop augmentation (dinov2/data/augmentations.py: DataAugmentationDINO) on the device, from a ragged batch of
// decoded uint8 images: bicubic RandomResizedCrop, flip, ColorJitter with hue, grayscale, the 9 x 9 Gaussian blur, solarize,
// ToTensor and Normalize.  As in augment.hip the host draws everything (octic_vits_amd/dino_augment.py) and uploads one
// octic_dino_row per crop plus the integer resampling coefficients; the kernels read nothing else about the draw.
//
// The arithmetic is Pillow's and torchvision's, rounding for rounding (the contract is in include/octic_hip.h and restated
// with numpy in tests/golden/dino_augment_numpy.py).  Four kernels per crop size, uint8 crops between them:
//   dino_resize_kernel      one workgroup per crop and 16 output rows: the horizontal pass of the source rows those need goes
//                           to LDS as uint8 (mirrored when the crop is flipped), the vertical pass reads them from there.
//                           Rows that do not fit the LDS at once are done in chunks of output rows.
//   dino_jitter_kernel<1>   replays ColorJitter up to its contrast op and leaves sum(L) of 2048 pixels in partials[n][tile]
//   dino_jitter_kernel<0>   adds the partials of its crop in index order (integers: exact), runs ColorJitter and grayscale
//   dino_finish_kernel      blur (16 x 64 tile with a 4-pixel reflected halo in LDS, separable, f32, fma in tap order, no
//                           rounding between the passes), rint, solarize, then uint8 NHWC or normalised f32 NCHW
// No atomics and no float sums across threads: bitwise reproducible, and a crop's result does not depend on its place in the
// batch.  Every index taken from a table is clamped or checked, so a malformed table gives wrong pixels, never a stray access.
#include "octic_common.hpp"

namespace octic {

typedef octic_dino_row DinoRow;

constexpr int DN_THREADS = 256;
constexpr int DR_ROWS = 16, DR_LDS = 49152;                  // resize: output rows per workgroup, bytes of uint8 rows in LDS
constexpr int DJ_PIX = 2048;                                 // jitter: pixels per workgroup
constexpr int DF_H = 16, DF_W = 64, DF_HALO = 4;             // finish: tile and halo
constexpr int DF_RH = DF_H + 2 * DF_HALO, DF_RW = DF_W + 2 * DF_HALO;

__device__ __forceinline__ int dn_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int dn_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
__device__ __forceinline__ int dn_blend(float deg, int v, float f) {   // Image.blend outside [0, 1], as augment.hip
  const float t = __fadd_rn(deg, __fmul_rn(f, (float)v - deg));
  return (int)fminf(fmaxf(t, 0.f), 255.f);
}
__device__ __forceinline__ int dn_clip8(int v) { return dn_clamp(v, 0, 255); }

// Pillow's rgb2hsv / hsv2rgb (libImaging/Convert.c) around H += shift (mod 256)
__device__ __forceinline__ void dn_hue(int* v, int shift) {
  const int r = v[0], g = v[1], b = v[2];
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = maxc;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = __fsub_rn(bc, gc);
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    H = dn_clip8((int)((double)h * 255.0));
    S = dn_clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    v[0] = v[1] = v[2] = V;
    return;
  }
  const double hf = (double)(float)H * 6.0 / 255.0;
  const double fl = floor(hf);
  const float f = (float)(hf - fl);
  const float fs = (float)((double)(float)S / 255.0);
  const double vd = (double)V, fd = (double)f, fsd = (double)fs;
  const int p = dn_clip8((int)round(vd * (1.0 - fsd)));
  const int q = dn_clip8((int)round(vd * (1.0 - fsd * fd)));
  const int t = dn_clip8((int)round(vd * (1.0 - fsd * (1.0 - fd))));
  switch ((int)fl % 6) {
    case 0: v[0] = V; v[1] = t; v[2] = p; break;
    case 1: v[0] = q; v[1] = V; v[2] = p; break;
    case 2: v[0] = p; v[1] = V; v[2] = t; break;
    case 3: v[0] = p; v[1] = q; v[2] = V; break;
    case 4: v[0] = t; v[1] = p; v[2] = V; break;
    default: v[0] = V; v[1] = p; v[2] = q; break;
  }
}

// ------------------------------------------------------------------------------------------------ resized crop
// grid: N x tiles workgroups; coefficient block of one crop and axis: bounds[S][2] = (xmin, count), then k[S][taps]
__global__ __launch_bounds__(DN_THREADS) void dino_resize_kernel(const uint8_t* __restrict__ data, int64_t data_bytes,
                                                                 const DinoRow* __restrict__ rows,
                                                                 const int32_t* __restrict__ coef, int64_t coef_len, int S,
                                                                 int tiles, uint8_t* __restrict__ out) {
  __shared__ uint8_t lds[DR_LDS];
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const DinoRow r = rows[n];
  const int y0 = t * DR_ROWS, y1 = min(y0 + DR_ROWS, S);
  uint8_t* dst = out + (int64_t)n * S * S * 3;
  const int64_t need_h = 2 * (int64_t)S + (int64_t)S * r.htaps, need_v = 2 * (int64_t)S + (int64_t)S * r.vtaps;
  const bool ok = r.src_h >= 1 && r.src_w >= 1 && r.src_h <= (1 << 24) && r.src_w <= (1 << 24) && r.top >= 0 && r.left >= 0 && r.h >= 1 && r.w >= 1 &&
                  (int64_t)r.top + r.h <= r.src_h && (int64_t)r.left + r.w <= r.src_w && r.src_offset >= 0 &&
                  r.src_offset + (int64_t)r.src_h * r.src_w * 3 <= data_bytes && r.htaps >= 1 && r.vtaps >= 1 && r.hcoef >= 0 &&
                  r.vcoef >= 0 && (int64_t)r.hcoef + need_h <= coef_len && (int64_t)r.vcoef + need_v <= coef_len;
  if (!ok) {
    for (int i = threadIdx.x; i < (y1 - y0) * S * 3; i += DN_THREADS) dst[(int64_t)y0 * S * 3 + i] = 0;
    return;
  }
  const int32_t* hb = coef + r.hcoef;
  const int32_t* hk = hb + 2 * S;
  const int32_t* vb = coef + r.vcoef;
  const int32_t* vk = vb + 2 * S;
  const int cap = DR_LDS / (S * 3);
  const uint8_t* src = data + r.src_offset + ((int64_t)r.top * r.src_w + r.left) * 3;
  int y = y0;
  while (y < y1) {
    // the chunk [y, ye) of output rows whose source rows [first, first + nrows) fit the LDS
    const int first = dn_clamp(vb[2 * y], 0, r.h - 1);
    int ye = y, nrows = 0;
    for (; ye < y1; ++ye) {
      const int lo = dn_clamp(vb[2 * ye], 0, r.h - 1);
      const int end = lo + dn_clamp(vb[2 * ye + 1], 0, min(r.vtaps, r.h - lo));
      if (end - first > cap) break;
      nrows = max(nrows, end - first);
    }
    if (ye == y) {                                          // one output row alone exceeds the LDS: the host refuses such tap
      ye = y + 1;                                           // counts (octic_dino_resize_max_taps), a malformed table loses taps
      nrows = cap;
    }
    nrows = min(nrows, r.h - first);
    // horizontal pass of the source rows into LDS
    for (int idx = threadIdx.x; idx < nrows * S; idx += DN_THREADS) {
      const int rr = idx / S, x = idx - rr * S;
      const int lo = dn_clamp(hb[2 * x], 0, r.w - 1);
      const int c = dn_clamp(hb[2 * x + 1], 0, min(r.htaps, r.w - lo));
      const uint8_t* p = src + ((int64_t)(first + rr) * r.src_w + lo) * 3;
      const int32_t* k = hk + (int64_t)x * r.htaps;
      uint32_t a0 = 1u << 21, a1 = 1u << 21, a2 = 1u << 21;
      for (int j = 0; j < c; ++j) {
        const uint32_t kj = (uint32_t)k[j];
        a0 += kj * p[3 * j];
        a1 += kj * p[3 * j + 1];
        a2 += kj * p[3 * j + 2];
      }
      uint8_t* o = lds + (rr * S + (r.flip ? S - 1 - x : x)) * 3;
      o[0] = (uint8_t)dn_clip8((int32_t)a0 >> 22);
      o[1] = (uint8_t)dn_clip8((int32_t)a1 >> 22);
      o[2] = (uint8_t)dn_clip8((int32_t)a2 >> 22);
    }
    __syncthreads();
    // vertical pass
    for (int idx = threadIdx.x; idx < (ye - y) * S; idx += DN_THREADS) {
      const int yr = idx / S, x = idx - yr * S, yy = y + yr;
      const int lo = dn_clamp(vb[2 * yy], 0, r.h - 1);
      const int c = dn_clamp(vb[2 * yy + 1], 0, min(r.vtaps, r.h - lo));
      const int32_t* k = vk + (int64_t)yy * r.vtaps;
      uint32_t a0 = 1u << 21, a1 = 1u << 21, a2 = 1u << 21;
      for (int j = 0; j < c; ++j) {
        const int rr = lo + j - first;
        if (rr < 0 || rr >= nrows) continue;
        const uint32_t kj = (uint32_t)k[j];
        const uint8_t* p = lds + (rr * S + x) * 3;
        a0 += kj * p[0];
        a1 += kj * p[1];
        a2 += kj * p[2];
      }
      uint8_t* o = dst + ((int64_t)yy * S + x) * 3;
      o[0] = (uint8_t)dn_clip8((int32_t)a0 >> 22);
      o[1] = (uint8_t)dn_clip8((int32_t)a1 >> 22);
      o[2] = (uint8_t)dn_clip8((int32_t)a2 >> 22);
    }
    __syncthreads();
    y = ye;
  }
}

// ------------------------------------------------------------------------------------------------ ColorJitter and grayscale
__device__ __forceinline__ uint64_t dn_block_sum(uint64_t v, uint64_t* red) {   // every thread ends with the total
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// grid: N x tiles workgroups over the H W pixels of a crop.  src and dst may be the same buffer (a pixel depends on itself
// and on the partials only, which the STATS launch finished before).
template <bool STATS>
__global__ __launch_bounds__(DN_THREADS) void dino_jitter_kernel(const uint8_t* src, uint8_t* dst,
                                                                 const DinoRow* __restrict__ rows, int npix, int tiles,
                                                                 uint32_t* __restrict__ partials) {
  __shared__ uint64_t red[4];
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const DinoRow row = rows[n];
  int order[4], seen = 0, contrast_at = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int o = row.order[k];
    if (o < 0 || o > 3 || (seen >> o & 1)) order[k] = -1;
    else {
      order[k] = o;
      seen |= 1 << o;
      if (o == 1) contrast_at = k;
    }
  }
  if (STATS && contrast_at < 0) return;
  const int nj = STATS ? contrast_at : 4;
  float mean_l = 0.f;
  if (!STATS && contrast_at >= 0) {
    uint64_t s = 0;
    for (int i = threadIdx.x; i < tiles; i += DN_THREADS) s += partials[(int64_t)n * tiles + i];
    s = dn_block_sum(s, red);
    const uint64_t np = (uint64_t)npix;
    mean_l = (float)(int)((2 * s + np) / (2 * np));         // PIL: int(mean + 0.5)
  }
  const uint8_t* in = src + (int64_t)n * npix * 3;
  uint32_t acc = 0;
#pragma unroll 1
  for (int i = 0; i < DJ_PIX / DN_THREADS; ++i) {
    const int pix = t * DJ_PIX + i * DN_THREADS + threadIdx.x;
    if (pix >= npix) break;
    const uint8_t* s = in + (int64_t)pix * 3;
    int v[3] = {s[0], s[1], s[2]};
#pragma unroll 1
    for (int k = 0; k < nj; ++k) {
      const int o = order[k];
      if (o < 0) continue;
      if (o == 3) {
        dn_hue(v, row.hue_shift & 255);
      } else {
        const float f = o == 0 ? row.brightness : (o == 1 ? row.contrast : row.saturation);
        const float deg = o == 0 ? 0.f : (o == 1 ? mean_l : (float)dn_luma(v[0], v[1], v[2]));
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = dn_blend(deg, v[c], f);
      }
    }
    if (STATS) {
      acc += (uint32_t)dn_luma(v[0], v[1], v[2]);
    } else {
      if (row.gray) v[0] = v[1] = v[2] = dn_luma(v[0], v[1], v[2]);
      uint8_t* d = dst + ((int64_t)n * npix + pix) * 3;
      d[0] = (uint8_t)v[0];
      d[1] = (uint8_t)v[1];
      d[2] = (uint8_t)v[2];
    }
  }
  if (STATS) {
    const uint64_t s = dn_block_sum(acc, red);
    if (threadIdx.x == 0) partials[(int64_t)n * tiles + t] = (uint32_t)s;   // <= 2048 x 255
  }
}

// ------------------------------------------------------------------------------------------------ blur, solarize, output
__device__ __forceinline__ int dn_reflect(int i, int n) {    // torch's reflect padding (pad 4 < n), then made safe
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return dn_clamp(i, 0, n - 1);
}

// grid: N x tiles workgroups, tiles = tiles_y x tiles_x
template <bool OUT_U8>
__global__ __launch_bounds__(DN_THREADS) void dino_finish_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst,
                                                                 const DinoRow* __restrict__ rows, float m0, float m1, float m2,
                                                                 float d0, float d1, float d2, int H, int W, int tiles_x,
                                                                 int tiles) {
  __shared__ uint32_t in[DF_RH * DF_RW];
  __shared__ float hb[DF_RH * DF_W * 3];
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const DinoRow row = rows[n];
  const int y0 = ty * DF_H, x0 = tx * DF_W;
  const uint8_t* img = src + (int64_t)n * H * W * 3;
  const bool blur = row.blur != 0;
  if (blur) {
    for (int idx = threadIdx.x; idx < DF_RH * DF_RW; idx += DN_THREADS) {
      const int ly = idx / DF_RW, lx = idx - ly * DF_RW;
      const int gy = dn_reflect(y0 - DF_HALO + ly, H), gx = dn_reflect(x0 - DF_HALO + lx, W);
      const uint8_t* s = img + ((int64_t)gy * W + gx) * 3;
      in[idx] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < DF_RH * DF_W; idx += DN_THREADS) {
      const int ly = idx / DF_W, lx = idx - ly * DF_W;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const uint32_t p = in[ly * DF_RW + lx + j];
        const float w = row.blur_w[j];
        a0 = fmaf(w, (float)(p & 255u), a0);
        a1 = fmaf(w, (float)((p >> 8) & 255u), a1);
        a2 = fmaf(w, (float)((p >> 16) & 255u), a2);
      }
      hb[idx * 3] = a0;
      hb[idx * 3 + 1] = a1;
      hb[idx * 3 + 2] = a2;
    }
    __syncthreads();
  }
  const float mean[3] = {m0, m1, m2}, sd[3] = {d0, d1, d2};
  for (int idx = threadIdx.x; idx < DF_H * DF_W; idx += DN_THREADS) {
    const int oy = idx / DF_W, ox = idx - oy * DF_W;
    const int gy = y0 + oy, gx = x0 + ox;
    if (gy >= H || gx >= W) continue;
    int v[3];
    if (blur) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) a = fmaf(row.blur_w[j], hb[((oy + j) * DF_W + ox) * 3 + c], a);
        v[c] = (int)fminf(fmaxf(rintf(a), 0.f), 255.f);
      }
    } else {
      const uint8_t* s = img + ((int64_t)gy * W + gx) * 3;
      v[0] = s[0];
      v[1] = s[1];
      v[2] = s[2];
    }
    if (row.solarize) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = v[c] < 128 ? v[c] : 255 - v[c];
    }
    if (OUT_U8) {
      uint8_t* d = (uint8_t*)dst + (((int64_t)n * H + gy) * W + gx) * 3;
      d[0] = (uint8_t)v[0];
      d[1] = (uint8_t)v[1];
      d[2] = (uint8_t)v[2];
    } else {
      float* d = (float*)dst + (((int64_t)n * 3) * H + gy) * W + gx;
#pragma unroll
      for (int c = 0; c < 3; ++c) d[(int64_t)c * H * W] = ((float)v[c] / 255.0f - mean[c]) / sd[c];
    }
  }
}

static bool dn_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

static int64_t dn_jitter_tiles(int64_t npix) { return (npix + DJ_PIX - 1) / DJ_PIX; }
static int64_t dn_partial_bytes(int N, int64_t npix) { return (dn_jitter_tiles(npix) * N * 4 + 255) / 256 * 256; }

}  // namespace octic

using namespace octic;

extern "C" {

// HOST code: Pillow's precompute_coeffs / normalize_coeffs_8bpc for the bicubic filter, float64, no contraction
int octic_dino_resize_coeffs(int n, int S, int taps, int32_t* bounds, int32_t* k) {
#pragma clang fp contract(off)
  if (!bounds || !k) return OCTIC_ENULL;
  if (n < 1 || S < 1) return OCTIC_ESHAPE;
  if (n == S) {                                             // Pillow skips the pass: one tap of 2^22
    if (taps != 1) return OCTIC_ESHAPE;
    for (int x = 0; x < S; ++x) {
      bounds[2 * x] = x;
      bounds[2 * x + 1] = 1;
      k[x] = 1 << 22;
    }
    return 0;
  }
  const double scale = (double)n / S, fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs, a = -0.5;
  if (taps != (int)ceil(support) * 2 + 1) return OCTIC_ESHAPE;
  for (int x = 0; x < S; ++x) {
    const double center = (x + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    const int c = hi - lo;
    double w[2048], ww = 0.0;
    if (c > 2048 || c > taps) return OCTIC_ESHAPE;
    for (int j = 0; j < c; ++j) {
      double t = (j + lo - center + 0.5) / fs;
      if (t < 0.0) t = -t;
      w[j] = t < 1.0 ? ((a + 2.0) * t - (a + 3.0)) * t * t + 1 : (t < 2.0 ? (((t - 5) * t + 8) * t - 4) * a : 0.0);
      ww += w[j];
    }
    bounds[2 * x] = lo;
    bounds[2 * x + 1] = c;
    int32_t* kx = k + (int64_t)x * taps;
    for (int j = 0; j < taps; ++j) {
      if (j >= c) {
        kx[j] = 0;
        continue;
      }
      const double v = ww != 0.0 ? w[j] / ww : w[j];
      kx[j] = v < 0 ? (int32_t)(v * (double)(1 << 22) - 0.5) : (int32_t)(v * (double)(1 << 22) + 0.5);
    }
  }
  return 0;
}

int octic_dino_resize_max_taps(int S) {
  if (S < 5 || S > 4096) return OCTIC_ESHAPE;
  return DR_LDS / (S * 3);
}

int64_t octic_dino_color_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H < 5 || W < 5) return OCTIC_ESHAPE;
  const int64_t npix = (int64_t)H * W;
  if (npix * 3 >= 0x80000000ll) return OCTIC_ESHAPE;
  return dn_partial_bytes(N, npix) + npix * 3 * N;
}

int octic_dino_resize_u8(const uint8_t* data, int64_t data_bytes, const octic_dino_row* rows, const int32_t* coef,
                         int64_t coef_len, int N, int S, uint8_t* crops, void* stream) {
  if (!data || !rows || !coef || !crops) return OCTIC_ENULL;
  if (N <= 0 || S < 5 || S > 4096 || data_bytes <= 0 || coef_len <= 0) return OCTIC_ESHAPE;
  if ((((uintptr_t)rows) & 7) || (((uintptr_t)coef) & 3)) return OCTIC_EALIGN;
  const int64_t tiles = (S + DR_ROWS - 1) / DR_ROWS;
  if (tiles * N > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if (dn_overlap(data, data_bytes, crops, (int64_t)N * S * S * 3)) return OCTIC_ESHAPE;
  dino_resize_kernel<<<dim3((unsigned)(tiles * N)), DN_THREADS, 0, (hipStream_t)stream>>>(data, data_bytes, rows, coef, coef_len,
                                                                                         S, (int)tiles, crops);
  return launch_status();
}

int octic_dino_color_u8(const uint8_t* crops, void* dst, int dtype_out, const octic_dino_row* rows, float mean0, float mean1,
                        float mean2, float std0, float std1, float std2, int N, int H, int W, void* workspace, void* stream) {
  if (!crops || !dst || !rows || !workspace) return OCTIC_ENULL;
  if (N <= 0 || H < 5 || W < 5) return OCTIC_ESHAPE;
  if (dtype_out != OCTIC_F32 && dtype_out != OCTIC_U8) return OCTIC_EDTYPE;
  const int64_t npix = (int64_t)H * W, n = npix * 3;
  if (n >= 0x80000000ll) return OCTIC_ESHAPE;
  const int es = dtype_out == OCTIC_F32 ? 4 : 1;
  if ((((uintptr_t)dst) & (es - 1)) || (((uintptr_t)rows) & 7) || (((uintptr_t)workspace) & 3)) return OCTIC_EALIGN;
  const int64_t ws_bytes = dn_partial_bytes(N, npix) + n * N;
  if (dn_overlap(crops, n * N, dst, n * N * es) || dn_overlap(workspace, ws_bytes, dst, n * N * es) ||
      dn_overlap(workspace, ws_bytes, crops, n * N))
    return OCTIC_ESHAPE;
  const int64_t jt = dn_jitter_tiles(npix);
  const int tiles_x = (W + DF_W - 1) / DF_W;
  const int64_t ft = (int64_t)((H + DF_H - 1) / DF_H) * tiles_x;
  if (jt * N > 0x7FFFFFFFll || ft * N > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  const hipStream_t st = (hipStream_t)stream;
  uint32_t* partials = (uint32_t*)workspace;
  uint8_t* tmp = (uint8_t*)workspace + dn_partial_bytes(N, npix);
  const dim3 jgrid((unsigned)(jt * N)), fgrid((unsigned)(ft * N));
  dino_jitter_kernel<true><<<jgrid, DN_THREADS, 0, st>>>(crops, nullptr, rows, (int)npix, (int)jt, partials);
  dino_jitter_kernel<false><<<jgrid, DN_THREADS, 0, st>>>(crops, tmp, rows, (int)npix, (int)jt, partials);
  if (dtype_out == OCTIC_U8)
    dino_finish_kernel<true><<<fgrid, DN_THREADS, 0, st>>>(tmp, dst, rows, mean0, mean1, mean2, std0, std1, std2, H, W, tiles_x,
                                                           (int)ft);
  else
    dino_finish_kernel<false><<<fgrid, DN_THREADS, 0, st>>>(tmp, dst, rows, mean0, mean1, mean2, std0, std1, std2, H, W, tiles_x,
                                                            (int)ft);
  return launch_status();
}

}  // extern "C"
