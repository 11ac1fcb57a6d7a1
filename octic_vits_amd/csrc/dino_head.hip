// Input rows of a DINO / iBOT head call (dinov2/train/ssl_meta_arch.py:226-267): up to four row segments - the class tokens of
// each crop set, the masked patch tokens through an int64 index - gathered into one [rows_out, D] buffer whose uncovered rows
// are +0 (the padding up to `upperbound`), in ONE launch instead of new_zeros + index_select + copy_ + cat; and the scatter of the
// cotangent rows back to their sources with plain stores (the indices are distinct, as mask_indices_list is: no atomics, no sum
// is reordered).  Rows move as 16-byte chunks, one wave per output row; a row's bytes do not depend on the row count, the row's
// position or its neighbours.
#include "octic_common.hpp"

namespace octic {

constexpr int DH_THREADS = 256;               // 4 waves = 4 rows a workgroup
constexpr int DH_WAVES = DH_THREADS / 64;
constexpr int HR_MAX_SEGMENTS = 4;

// One wave per output row.  The segment that covers the row is looked up in the table (at most four entries); a row no
// segment covers - or whose source row lies outside [0, src_rows) - is written as +0 by the gather and left alone by the
// scatter.
template <bool SCATTER>
__global__ __launch_bounds__(DH_THREADS) void head_rows_kernel(const octic_head_segment* __restrict__ segs, int nseg,
                                                               int64_t rows_out, int chunks, char* __restrict__ out,
                                                               int64_t ldo_bytes, int esize) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * DH_WAVES + (threadIdx.x >> 6);
  if (row >= rows_out) return;
  char* src = nullptr;
  for (int s = 0; s < nseg; ++s) {
    const octic_head_segment sg = segs[s];
    const int64_t r = row - sg.out_row0;
    if (r < 0 || r >= sg.n) continue;
    const int64_t j = sg.idx ? sg.idx[r] : r;
    if (j < 0 || j >= sg.src_rows || sg.inner < 1) break;
    src = (char*)sg.base + ((j / sg.inner) * sg.outer_ld + (j % sg.inner) * sg.inner_ld) * esize;
    break;
  }
  u32x4* o = (u32x4*)(out + row * ldo_bytes);
  if (SCATTER) {
    if (!src) return;
    for (int c = lane; c < chunks; c += 64) ((u32x4*)src)[c] = o[c];
  } else {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int c = lane; c < chunks; c += 64) o[c] = src ? ((const u32x4*)src)[c] : zero;
  }
}

}  // namespace octic

using namespace octic;

extern "C" {

int octic_head_rows(const octic_head_segment* segments_dev, int n_segments, int64_t rows_out, int64_t D, int dtype, void* out,
                    int64_t ldo, int scatter, void* stream) {
  if (!segments_dev || !out) return OCTIC_ENULL;
  if (dtype != OCTIC_BF16 && dtype != OCTIC_F32) return OCTIC_EDTYPE;
  if (n_segments < 1 || n_segments > HR_MAX_SEGMENTS || rows_out < 1 || rows_out > 0x7FFFFFFFll || D < 8 || D % 8 ||
      D > (1 << 20) || ldo < D)
    return OCTIC_ESHAPE;
  const int es = elem_size(dtype);
  if ((((uintptr_t)out) & 15) || ((ldo * es) & 15) || ((D * es) & 15)) return OCTIC_EALIGN;
  const dim3 grid((unsigned)((rows_out + DH_WAVES - 1) / DH_WAVES)), block(DH_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)(D * es / 16);
  if (scatter)
    head_rows_kernel<true><<<grid, block, 0, st>>>(segments_dev, n_segments, rows_out, chunks, (char*)out, ldo * es, es);
  else
    head_rows_kernel<false><<<grid, block, 0, st>>>(segments_dev, n_segments, rows_out, chunks, (char*)out, ldo * es, es);
  return launch_status();
}

}  // extern "C"
