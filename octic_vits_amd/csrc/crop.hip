// The crops and the evaluation resize of the DeiT-III pipeline on the device, from a ragged batch of decoded uint8 images:
// timm's RandomResizedCropAndInterpolation (bicubic), the --src crop (Resize + RandomCrop(padding=4, reflect)), the evaluation
// transform (Resize + CenterCrop) and the quarter turns / mirror of --rot-eval / --flop-eval (deit/augment.py:90-108,
// deit/datasets.py:91-132).  One kernel: a window of the reflect-padded, bicubically resized box of a source, turned and
// mirrored, as uint8 NHWC or as the normalised f32 NCHW batch.  The host draws everything (octic_vits_amd/crop.py) and uploads
// one octic_crop_row per output image plus the integer coefficients of octic_dino_resize_coeffs; the arithmetic is Pillow's,
// rounding for rounding (the contract is in include/octic_hip.h, restated with numpy in tests/golden/crop_numpy.py).
//
//   crop_resize_kernel   one workgroup per image and CR_ROWS rows of the window.  Only what the window touches is computed:
//                        the source rows its resized rows need and, of those, the bytes its resized columns need.  Those
//                        row segments go to LDS with aligned dword loads, the horizontal pass reads them from there and leaves uint8
//                        rows in LDS in OUTPUT column order (reflected, mirrored), the vertical pass reads one dword (four
//                        bytes of a row: it does not care about channels) per tap and row and stores dwords.  Rows that do not
//                        fit the LDS at once are done in chunks of window rows, segments in batches of source rows.
// Integer sums only, no atomics: bitwise reproducible, and an image's result does not depend on its place in the batch.  Every
// bound read from device memory is clamped, and a row that does not describe a window inside its data gives an all-zero image.
#include "octic_common.hpp"

namespace octic {

typedef octic_crop_row CropRow;

constexpr int CR_THREADS = 256;
constexpr int CR_ROWS = 16;                                  // window rows per workgroup
constexpr int CR_LDS = 49152;                                // bytes of horizontally resampled uint8 rows in LDS
constexpr int CR_STAGE = 12288;                              // bytes of staged source row segments in LDS

__device__ __forceinline__ int cr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int cr_clip8(int v) { return cr_clamp(v, 0, 255); }
__device__ __forceinline__ int cr_reflect(int i, int n) {    // numpy.pad(mode="reflect") with pad < n, then made safe
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return cr_clamp(i, 0, n - 1);
}
__host__ __device__ __forceinline__ int cr_stride(int W) { return (W * 3 + 3) / 4 * 4; }   // bytes of one LDS row of W pixels

// A coefficient times a pixel on the 24-bit multiplier (v_mad_i32_i24: full rate, where the 32-bit multiply runs at a quarter
// of it and was most of this kernel's time).  Exact for |k| < 2^23: Pillow's coefficients are below 2^22 (1 + the side lobes),
// and the host checks it; another pool gives wrong pixels, no stray access.
__device__ __forceinline__ uint32_t cr_mul(uint32_t k, uint32_t v) { return (uint32_t)__mul24((int)k, (int)v); }

// acc[c] = 2^21 + sum_j k[j] s[3 j + c] over the taps j0 <= j < j1 of one output pixel
__device__ __forceinline__ void cr_taps(const uint8_t* __restrict__ s, const int32_t* __restrict__ k, int j0, int j1,
                                        uint32_t (&acc)[3]) {
  acc[0] = acc[1] = acc[2] = 1u << 21;
#pragma unroll 4
  for (int j = j0; j < j1; ++j) {
    const uint32_t kj = (uint32_t)k[j];
    acc[0] += cr_mul(kj, s[3 * j]);
    acc[1] += cr_mul(kj, s[3 * j + 1]);
    acc[2] += cr_mul(kj, s[3 * j + 2]);
  }
}

// grid: N x tiles workgroups, tiles = ceil(OH / CR_ROWS).  A coefficient block is bounds[S][2] = (xmin, count), then k[S][taps].
template <bool OUT_U8>
__global__ __launch_bounds__(CR_THREADS) void crop_resize_kernel(const uint8_t* __restrict__ data, int64_t data_bytes,
                                                                 const CropRow* __restrict__ rows,
                                                                 const int32_t* __restrict__ coef, int64_t coef_len, int OH,
                                                                 int OW, int tiles, void* __restrict__ out, float m0, float m1,
                                                                 float m2, float d0, float d1, float d2) {
  __shared__ uint32_t hrows32[CR_LDS / 4];
  __shared__ uint32_t stage32[CR_STAGE / 4];
  __shared__ float lut[OUT_U8 ? 1 : 768];
  const uint8_t* hrows = (const uint8_t*)hrows32;
  const uint8_t* stage = (const uint8_t*)stage32;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const CropRow r = rows[n];
  const int wy0 = t * CR_ROWS, wy1 = min(wy0 + CR_ROWS, OH);
  const int64_t img = (int64_t)n * OH * OW * 3;              // elements in front of this image, either format
  const int64_t need_h = 2 * (int64_t)r.rw + (int64_t)r.rw * r.htaps, need_v = 2 * (int64_t)r.rh + (int64_t)r.rh * r.vtaps;
  const bool ok = r.src_h >= 1 && r.src_w >= 1 && r.src_h <= (1 << 24) && r.src_w <= (1 << 24) && r.top >= 0 && r.left >= 0 &&
                  r.h >= 1 && r.w >= 1 && (int64_t)r.top + r.h <= r.src_h && (int64_t)r.left + r.w <= r.src_w && r.src_offset >= 0 &&
                  r.src_offset + (int64_t)r.src_h * r.src_w * 3 <= data_bytes && r.rh >= 1 && r.rw >= 1 && r.rh <= (1 << 24) &&
                  r.rw <= (1 << 24) && r.htaps >= 1 && r.vtaps >= 1 && r.hcoef >= 0 && r.vcoef >= 0 &&
                  (int64_t)r.hcoef + need_h <= coef_len && (int64_t)r.vcoef + need_v <= coef_len && r.pad >= 0 &&
                  (r.pad == 0 || r.pad < min(r.rh, r.rw)) && r.rot >= 0 && r.rot <= 3 && (!(r.rot & 1) || OH == OW) &&
                  r.win_top >= 0 && r.win_left >= 0 && (int64_t)r.win_top + OH <= (int64_t)r.rh + 2 * r.pad &&
                  (int64_t)r.win_left + OW <= (int64_t)r.rw + 2 * r.pad;
  if (!ok) {                                                 // (the tiles of an image cover it whatever its orientation)
    const int cnt = (wy1 - wy0) * OW;
    if (OUT_U8) {
      uint8_t* dst = (uint8_t*)out + img + (int64_t)wy0 * OW * 3;
      for (int i = threadIdx.x; i < cnt * 3; i += CR_THREADS) dst[i] = 0;
    } else {
      for (int i = threadIdx.x; i < cnt * 3; i += CR_THREADS) {
        const int c = i / cnt, o = i - c * cnt;
        ((float*)out)[img + ((int64_t)c * OH + wy0) * OW + o] = 0.f;
      }
    }
    return;
  }
  if (!OUT_U8) {                                             // ToTensor + Normalize of the 256 values, two divisions each
    const float mean[3] = {m0, m1, m2}, sd[3] = {d0, d1, d2};
    for (int i = threadIdx.x; i < 768; i += CR_THREADS) lut[i] = ((float)(i & 255) / 255.0f - mean[i >> 8]) / sd[i >> 8];
    __syncthreads();
  }
  // orientation: LDS column p of a row holds window column (xm ? OW-1-p : p).  rot 0 / 2: window row -> output row (reversed
  // for rot 2), p = output x.  rot 1 / 3 (OH == OW): p = output y, the window row gives output x.
  const bool odd = r.rot & 1, flip = r.flip != 0;
  const bool xm = r.rot == 0 ? flip : (r.rot == 2 ? !flip : r.rot == 1);
  const int hstride = cr_stride(OW), hwords = hstride / 4, cap = CR_LDS / hstride;
  const int32_t* hb = coef + r.hcoef;
  const int32_t* hk = hb + 2 * (int64_t)r.rw;
  const int32_t* vb = coef + r.vcoef;
  const int32_t* vk = vb + 2 * (int64_t)r.rh;
  // the resized columns the window reads: [a, b] inside, 1 .. -a left of it, 2 (rw - 1) - b .. rw - 2 right of it
  const int a = r.win_left - r.pad, b = a + OW - 1;
  int rx0 = max(a, 0), rx1 = min(b, r.rw - 1);
  if (a < 0) {
    rx0 = min(rx0, 1);
    rx1 = max(rx1, -a);
  }
  if (b > r.rw - 1) {
    rx0 = min(rx0, 2 * (r.rw - 1) - b);
    rx1 = max(rx1, r.rw - 2);
  }
  rx0 = cr_clamp(rx0, 0, r.rw - 1);                          // (a window that lies in the padding alone reads a subset)
  rx1 = cr_clamp(rx1, rx0, r.rw - 1);
  // ... and the source columns [c0, c1) of the box those need (bounds grow with x)
  const int c0 = cr_clamp(hb[2 * rx0], 0, r.w - 1);
  const int cl = cr_clamp(hb[2 * rx1], 0, r.w - 1);
  const int c1 = max(cl + cr_clamp(hb[2 * rx1 + 1], 0, min(r.htaps, r.w - cl)), c0);
  const int segbytes = (c1 - c0) * 3;
  const int sstride = (segbytes + 6) / 4 * 4;                // an aligned segment starts up to 3 bytes early
  const bool staged = sstride <= CR_STAGE;                   // wider sources are read from memory directly
  const int batch = staged ? CR_STAGE / sstride : cap;
  const uint8_t* const data_end = data + data_bytes;
  const int64_t src0 = r.src_offset + ((int64_t)r.top * r.src_w + r.left + c0) * 3;   // byte (row 0, column c0) of the box
  int y = wy0;
  while (y < wy1) {
    // the chunk [y, ye) of window rows whose source rows [first, first + nrows) fit the LDS
    int first = 0x7fffffff, last = 0, ye = y;
    for (; ye < wy1; ++ye) {
      const int ry = cr_reflect(r.win_top + ye - r.pad, r.rh);
      const int lo = cr_clamp(vb[2 * ry], 0, r.h - 1);
      const int end = lo + cr_clamp(vb[2 * ry + 1], 0, min(r.vtaps, r.h - lo));
      const int f = min(first, lo), l = max(last, end);
      if (l - f > cap) break;
      first = f;
      last = l;
    }
    if (ye == y) {                                          // one window row alone exceeds the LDS: the host refuses such tap
      const int ry = cr_reflect(r.win_top + y - r.pad, r.rh);   // counts (octic_crop_resize_max_taps), a malformed table loses taps
      first = cr_clamp(vb[2 * ry], 0, r.h - 1);
      last = first + cap;
      ye = y + 1;
    }
    const int nrows = min(last - first, r.h - first);
    for (int r0 = 0; r0 < nrows; r0 += batch) {
      const int nb = min(batch, nrows - r0);
      if (staged) {                                         // source row segments -> LDS, aligned dwords
        const int sw = sstride / 4;
        for (int idx = threadIdx.x; idx < nb * sw; idx += CR_THREADS) {
          const int rr = idx / sw, d = idx - rr * sw;
          const uint8_t* p = data + src0 + (int64_t)(first + r0 + rr) * r.src_w * 3;
          const int shift = (int)((uintptr_t)p & 3);
          if (d * 4 >= shift + segbytes) continue;
          const uint8_t* q = p - shift + d * 4;
          uint32_t v;
          if (q >= data && q + 4 <= data_end) {
            v = *(const uint32_t*)q;
          } else {                                          // the dword leaves the buffer: its bytes inside, one by one
            v = 0;
            for (int i = 0; i < 4; ++i)
              if (q + i >= data && q + i < data_end) v |= (uint32_t)q[i] << (8 * i);
          }
          stage32[rr * sw + d] = v;
        }
        __syncthreads();
      }
      // horizontal pass of these source rows into LDS, in output column order
      for (int idx = threadIdx.x; idx < nb * OW; idx += CR_THREADS) {
        const int rr = idx / OW, p = idx - rr * OW;
        const int rx = cr_reflect(r.win_left + (xm ? OW - 1 - p : p) - r.pad, r.rw);
        const int lo = cr_clamp(hb[2 * rx], 0, r.w - 1);
        const int c = cr_clamp(hb[2 * rx + 1], 0, min(r.htaps, r.w - lo));
        const int j0 = max(c0 - lo, 0), j1 = min(c, c1 - lo);   // (all of 0 .. c for bounds that grow with x)
        const int32_t* k = hk + (int64_t)rx * r.htaps;
        const uint8_t* g = data + src0 + (int64_t)(first + r0 + rr) * r.src_w * 3;
        uint32_t acc[3];
        if (staged) cr_taps(stage + rr * sstride + (int)((uintptr_t)g & 3) + (lo - c0) * 3, k, j0, j1, acc);
        else cr_taps(g + (int64_t)(lo - c0) * 3, k, j0, j1, acc);
        uint8_t* o = (uint8_t*)hrows32 + (r0 + rr) * hstride + p * 3;
        o[0] = (uint8_t)cr_clip8((int32_t)acc[0] >> 22);
        o[1] = (uint8_t)cr_clip8((int32_t)acc[1] >> 22);
        o[2] = (uint8_t)cr_clip8((int32_t)acc[2] >> 22);
      }
      __syncthreads();
    }
    // vertical pass: four bytes of a row per thread
    for (int idx = threadIdx.x; idx < (ye - y) * hwords; idx += CR_THREADS) {
      const int yr = idx / hwords, i = idx - yr * hwords, wy = y + yr;
      const int ry = cr_reflect(r.win_top + wy - r.pad, r.rh);
      const int lo = cr_clamp(vb[2 * ry], 0, r.h - 1);
      const int c = cr_clamp(vb[2 * ry + 1], 0, min(r.vtaps, r.h - lo));
      const int32_t* k = vk + (int64_t)ry * r.vtaps;
      const int j0 = max(first - lo, 0), j1 = min(c, first + nrows - lo);   // the taps whose rows are in LDS (all, but for a
      const uint32_t* col = hrows32 + (lo - first) * hwords + i;          // malformed table)
      uint32_t acc[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
#pragma unroll 4
      for (int j = j0; j < j1; ++j) {
        const uint32_t kj = (uint32_t)k[j];
        const uint32_t w = col[j * hwords];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += cr_mul(kj, (w >> (8 * q)) & 255u);
      }
      uint32_t v[4], packed = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = (uint32_t)cr_clip8((int32_t)acc[q] >> 22);
        packed |= v[q] << (8 * q);
      }
      const int nbytes = min(4, OW * 3 - 4 * i);             // (the last dword of a row may be short)
      if (!odd) {
        const int oy = r.rot == 2 ? OH - 1 - wy : wy;
        if (OUT_U8) {
          uint8_t* d = (uint8_t*)out + img + (int64_t)oy * OW * 3 + 4 * i;
          if (nbytes == 4 && ((uintptr_t)d & 3) == 0) {
            *(uint32_t*)d = packed;
          } else {
            for (int q = 0; q < nbytes; ++q) d[q] = (uint8_t)v[q];
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int bq = 4 * i + q, px = bq / 3, ch = bq - px * 3;
            if (q < nbytes) ((float*)out)[img + ((int64_t)ch * OH + oy) * OW + px] = lut[ch * 256 + v[q]];
          }
        }
      } else {
        const int ox = (r.rot == 1) == flip ? OW - 1 - wy : wy;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int bq = 4 * i + q, oy = bq / 3, ch = bq - oy * 3;
          if (q >= nbytes) continue;
          if (OUT_U8) ((uint8_t*)out)[img + ((int64_t)oy * OW + ox) * 3 + ch] = (uint8_t)v[q];
          else ((float*)out)[img + ((int64_t)ch * OH + oy) * OW + ox] = lut[ch * 256 + v[q]];
        }
      }
    }
    __syncthreads();
    y = ye;
  }
}

static bool cr_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_crop_resize_max_taps(int OW) {
  if (OW < 5 || OW > 4096) return OCTIC_ESHAPE;
  return CR_LDS / cr_stride(OW);
}

int octic_crop_resize_rows(void) { return CR_ROWS; }

int octic_crop_resize_u8(const uint8_t* data, int64_t data_bytes, const octic_crop_row* rows, const int32_t* coef,
                         int64_t coef_len, int N, int OH, int OW, void* dst, int dtype_out, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, void* stream) {
  if (!data || !rows || !coef || !dst) return OCTIC_ENULL;
  if (N <= 0 || OH < 5 || OH > 4096 || OW < 5 || OW > 4096 || data_bytes <= 0 || coef_len <= 0) return OCTIC_ESHAPE;
  if (dtype_out != OCTIC_F32 && dtype_out != OCTIC_U8) return OCTIC_EDTYPE;
  const int es = dtype_out == OCTIC_F32 ? 4 : 1;
  if ((((uintptr_t)rows) & 7) || (((uintptr_t)coef) & 3) || (((uintptr_t)dst) & (es - 1))) return OCTIC_EALIGN;
  const int64_t tiles = (OH + CR_ROWS - 1) / CR_ROWS;
  if (tiles * N > 0x7FFFFFFFll) return OCTIC_ESHAPE;
  if (cr_overlap(data, data_bytes, dst, (int64_t)N * OH * OW * 3 * es)) return OCTIC_ESHAPE;
  const dim3 grid((unsigned)(tiles * N));
  if (dtype_out == OCTIC_U8)
    crop_resize_kernel<true><<<grid, CR_THREADS, 0, (hipStream_t)stream>>>(data, data_bytes, rows, coef, coef_len, OH, OW, (int)tiles,
                                                                          dst, mean0, mean1, mean2, std0, std1, std2);
  else
    crop_resize_kernel<false><<<grid, CR_THREADS, 0, (hipStream_t)stream>>>(data, data_bytes, rows, coef, coef_len, OH, OW, (int)tiles,
                                                                           dst, mean0, mean1, mean2, std0, std1, std2);
  return launch_status();
}

}  // extern "C"
