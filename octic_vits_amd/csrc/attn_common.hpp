// Shared pieces of the attention kernels (csrc/attention.hip: generic shapes; csrc/attn80.hip: the persistent
// head_dim-80 kernels): argument structs, head-vector addressing on packed LinearD8 rows, accumulator helpers.
#pragma once
#include "octic_common.hpp"

namespace octic {

typedef __attribute__((ext_vector_type(16))) float f32x16;

struct AttnArgs {
  const bf16* q; const bf16* k; const bf16* v;   // element (b,h,t,d) at base + b*sB + h*sH + t*sT + d
  int64_t sB, sH, sT;
  bf16* o; int64_t oB, oH, oT;
  float* lse;            // [B,H,T] log2-domain log-sum-exp of the scaled scores
  int H, T, hd;
  float scale_log2;      // softmax scale * log2(e)
  // packed mode (cv_in > 0): q == k == v is the packed LinearD8 output [B,T,3*8c] (row stride sT, sH = 0), o the packed
  // [B,T,8c] input of the output projection; cv = irrep block width of a row (3c / c), c = channels per irrep.
  int cv_in, cv_out, c;
  int dbg = 0;           // developer probes (csrc/attn80.hip): 1 = K / V descriptors with zero records (their DMA is dropped)
  // nullable, [B] f32: the factor the caller multiplies sample b's branch output with (stochastic depth).  Exactly 0.0f = the
  // sample is dropped: a kernel may skip it - it then writes +0 to the sample's o rows and lse and reads none of its operands
  // (include/octic_hip.h, octic_attn_*_skip)
  const float* sample_scale = nullptr;
};

// ---- head-vector addressing ------------------------------------------------------------------------------------------
// Plain (cv == 0): the hd elements of (b,h,t) are contiguous.  Packed: the head vector of tensor s, head h is six pieces
// of the token row - w = c/H channels of each one-dimensional irrep and 2w of each row of E (reference
// d8_layers.py:631-643, 650-656) - so AttentionD8 needs no pack / unpack passes.  The dot products do not care about the
// order of the hd elements as long as q, k (and v, o) agree, so the pieces are visited in an order that keeps 16-byte
// groups inside a piece where possible (w = 10, hd = 80 = ten groups of 8): groups 0-3 = first 8 channels of A1, A2, B1,
// B2; groups 4-7 = E0[0:8], E0[8:16], E1[0:8], E1[8:16]; group 8 = the four 2-channel remainders of the 1-D pieces;
// group 9 = the two 4-channel remainders of the E pieces.  Pieces start on 4-byte boundaries (20 h bytes).
struct HeadMap { int cv, bs; };        // bs = s*c + h*w
typedef unsigned u32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int hm_off8(const HeadMap m, int g) {
  return g < 4 ? g * m.cv + m.bs : (4 + 2 * ((g - 4) >> 1)) * m.cv + 2 * m.bs + ((g - 4) & 1) * 8;
}
__device__ __forceinline__ u32x4 hm_load16(const bf16* row, int c, const HeadMap m) {
  if (m.cv == 0) return *(const u32x4*)(row + c * 8);
  if (c < 8) return *(const u32x4_u*)(row + hm_off8(m, c));
  if (c == 8) {
    const bf16* p = row + m.bs + 8;
    return u32x4{*(const unsigned*)p, *(const unsigned*)(p + m.cv), *(const unsigned*)(p + 2 * m.cv),
                 *(const unsigned*)(p + 3 * m.cv)};
  }
  const bf16* p = row + 4 * m.cv + 2 * m.bs + 16;
  const u32x2_u e0 = *(const u32x2_u*)p, e1 = *(const u32x2_u*)(p + 2 * m.cv);
  return u32x4{e0[0], e0[1], e1[0], e1[1]};
}
__device__ __forceinline__ void hm_store16(bf16* row, int c, const u32x4 v, const HeadMap m) {
  if (m.cv == 0) { *(u32x4*)(row + c * 8) = v; return; }
  if (c < 8) { *(u32x4_u*)(row + hm_off8(m, c)) = v; return; }
  if (c == 8) {
    bf16* p = row + m.bs + 8;
    *(unsigned*)p = v[0]; *(unsigned*)(p + m.cv) = v[1]; *(unsigned*)(p + 2 * m.cv) = v[2]; *(unsigned*)(p + 3 * m.cv) = v[3];
    return;
  }
  bf16* p = row + 4 * m.cv + 2 * m.bs + 16;
  *(u32x2_u*)p = u32x2_u{v[0], v[1]};
  *(u32x2_u*)(p + 2 * m.cv) = u32x2_u{v[2], v[3]};
}
// four consecutive elements: half `sub` of group g
__device__ __forceinline__ void hm_store8(bf16* row, int g, int sub, const u32x2 v, const HeadMap m) {
  if (m.cv == 0) { *(u32x2*)(row + g * 8 + sub * 4) = v; return; }
  if (g < 8) { *(u32x2_u*)(row + hm_off8(m, g) + sub * 4) = u32x2_u{v[0], v[1]}; return; }
  if (g == 8) {
    bf16* p = row + 2 * sub * m.cv + m.bs + 8;
    *(unsigned*)p = v[0]; *(unsigned*)(p + m.cv) = v[1];
    return;
  }
  *(u32x2_u*)(row + (4 + 2 * sub) * m.cv + 2 * m.bs + 16) = u32x2_u{v[0], v[1]};
}
// the head maps of one (b, h): tensor s of the packed projection output / the packed single-tensor rows
struct HeadMaps { HeadMap q, k, v, o; };
template <typename A>
__device__ __forceinline__ HeadMaps head_maps(const A& a, int h) {
  HeadMaps m;
  const int w = a.cv_in > 0 ? a.c / a.H : 0;
  m.q = HeadMap{a.cv_in, h * w};
  m.k = HeadMap{a.cv_in, a.c + h * w};
  m.v = HeadMap{a.cv_in, 2 * a.c + h * w};
  m.o = HeadMap{a.cv_out, h * w};
  return m;
}
// Workgroup / work-item index -> (b, h) unit.  When the heads of a token share cache lines (packed rows: 20-byte pieces;
// the standard block's fused [B,T,3,H,hd] projection: 160-byte pieces) the units are dealt so that each XCD works on
// whole batches: the lines a head leaves partly used are consumed by its neighbours out of the same L2 instead of
// being fetched once per XCD.  Bijective for any unit count.
__device__ __forceinline__ int unit_of(int idx, int units, bool shared_rows) {
  if (!shared_rows) return idx;
  const int xcd = idx & 7, local = idx >> 3, q8 = units >> 3, r8 = units & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + local;
}

// element e of the head vector -> element offset in the row (scalar accesses of the merge paths)
__device__ __forceinline__ int hm_elem(int e, const HeadMap m) {
  if (m.cv == 0) return e;
  const int g = e >> 3, j = e & 7;
  if (g < 8) return hm_off8(m, g) + j;
  if (g == 8) return (j >> 1) * m.cv + m.bs + 8 + (j & 1);
  return (4 + 2 * (j >> 2)) * m.cv + 2 * m.bs + 16 + (j & 3);
}

__device__ inline int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// +0 to the T head vectors (nc 16-byte chunks each) of one (b, h) of a tensor, by all `nthr` threads of the workgroup:
// the store of a unit whose sample the stochastic-depth mask drops (AttnArgs::sample_scale)
__device__ __forceinline__ void zero_head_rows(bf16* base, int64_t row_stride, int T, int nc, const HeadMap m, int tid, int nthr) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int i = tid; i < T * nc; i += nthr) {
    const int row = i / nc;
    hm_store16(base + (int64_t)row * row_stride, i - row * nc, z, m);
  }
}
__device__ __forceinline__ void zero_stats(float* p, int T, int tid, int nthr) {
  for (int i = tid; i < T; i += nthr) p[i] = 0.f;
}

__device__ inline bf16x8 pack8(const float* p) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (bf16)p[i];
  return r;
}

// V^T (or any row-major [key][col] LDS image) fragment of the A operand for  Y = A X  where X is an accumulator tile:
// lane (r = lane&31 -> column c0 + r, half) gets, for k-step s, keys 16s + 4*half + {0..3} and + 8 + {0..3}.
__device__ inline bf16x8 tr_frag(const char* img, int row_bytes, int key0, int c0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int q4 = i >> 2, p = i & 3, half = g >> 1;
  const char* a = img + (size_t)(key0 + 4 * half + q4) * row_bytes + (c0 + (g & 1) * 16 + 4 * p) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)a);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a + 8 * row_bytes));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

constexpr int kPartPad = 4;    // f32 row pad of the partial-result images (conflict-free 16-byte accesses)

struct AttnBwdArgs {
  const bf16* q; const bf16* k; const bf16* v; int64_t sB, sH, sT;      // inputs
  const bf16* o; const bf16* dout; int64_t oB, oH, oT;                   // forward output and its cotangent
  const float* lse; float* delta;                                         // [B,H,T] f32
  bf16* dq; bf16* dk; bf16* dv; int64_t gB, gH, gT;                     // gradients
  int H, T, hd;
  float scale, scale_log2;
  int cv_in, cv_out, c;                                                   // packed mode, see AttnArgs
  const float* sample_scale = nullptr;                                    // see AttnArgs: a skipped sample gets +0 in dq, dk, dv, delta
};


// accumulator tile set -> bf16 rows of the output (lane r = row `row`, 4 consecutive columns per store)
template <int DT>
__device__ __forceinline__ void store_rows(bf16* row, const f32x16 (&acc)[DT], float f, int hd, int half,
                                           const HeadMap m = HeadMap{0, 0}) {
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const int g = d * 4 + k4;                  // elements 8 g + 4 half .. + 3
      if (g * 8 < hd) {
        bf16x4 ov = {(bf16)(acc[d][4 * k4] * f), (bf16)(acc[d][4 * k4 + 1] * f), (bf16)(acc[d][4 * k4 + 2] * f),
                     (bf16)(acc[d][4 * k4 + 3] * f)};
        hm_store8(row, g, half, __builtin_bit_cast(u32x2, ov), m);
      }
    }
}

// 16-byte row stores (head_dim % 16 == 0): a lane holds elements 8 g + 4 half .. + 3 of group g; exchanging halves
// between the two half-waves (v_permlane32_swap) gives lanes 0-31 the whole even group and lanes 32-63 the whole odd
// group of a pair - one 16-byte store per lane and pair instead of two 8-byte ones (the store tail of these kernels is
// bound by the number of store instructions, not by bytes: MI355X guide, T21).
template <int DT>
__device__ __forceinline__ void store_rows_wide(bf16* row, const f32x16 (&acc)[DT], float f, int hd, int half,
                                                const HeadMap m = HeadMap{0, 0}) {
#pragma unroll
  for (int pr = 0; pr < DT * 2; ++pr) {                // groups (2 pr, 2 pr + 1)
    if (pr * 16 < hd) {
      u32x2 a, b;
      {
        const int g = 2 * pr, d = g >> 2, k4 = g & 3;
        const bf16x4 v = {(bf16)(acc[d][4 * k4] * f), (bf16)(acc[d][4 * k4 + 1] * f), (bf16)(acc[d][4 * k4 + 2] * f), (bf16)(acc[d][4 * k4 + 3] * f)};
        a = __builtin_bit_cast(u32x2, v);
      }
      {
        const int g = 2 * pr + 1, d = g >> 2, k4 = g & 3;
        const bf16x4 v = {(bf16)(acc[d][4 * k4] * f), (bf16)(acc[d][4 * k4 + 1] * f), (bf16)(acc[d][4 * k4 + 2] * f), (bf16)(acc[d][4 * k4 + 3] * f)};
        b = __builtin_bit_cast(u32x2, v);
      }
      const auto r0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);   // lanes 32-63 of a <-> lanes 0-31 of b
      const auto r1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
      hm_store16(row, 2 * pr + half, u32x4{r0[0], r1[0], r0[1], r1[1]}, m);
    }
  }
}

template <int DT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[DT]) {
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[d][i] = 0.f;
}


// ---- per-wave row fragments shared by the resident-K/V kernels (csrc/attention.hip) and the streaming ones
// (csrc/attn_stream.hip)
// lane (r, half) holds Q[query][16 ks + 8 half .. +7] = B operand of K Q^T
template <int KS>
__device__ __forceinline__ void load_rows8(bf16x8 (&f)[KS], const bf16* base, int64_t st, int tile, int T, int lane,
                                           const HeadMap m = HeadMap{0, 0}) {
  const int r = lane & 31, half = lane >> 5;
  const int i = tile * 32 + r;
  const int ic = i < T ? i : T - 1;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    f[ks] = __builtin_bit_cast(bf16x8, hm_load16(base + (int64_t)ic * st, 2 * ks + half, m));
}

// per-query operands of the dq kernel for one query tile: Q and dO fragments, log-sum-exp, delta = <dO, O>
template <int KS>
struct DqRows {
  bf16x8 qf[KS], dof[KS], of[KS];
  float lse, delta;
};
// issue the loads only: the staging loads follow right behind, so the two memory round trips overlap ...
template <int KS>
__device__ __forceinline__ void load_dq_rows(DqRows<KS>& R, const AttnBwdArgs& a, int64_t in_off, int64_t o_off,
                                             int64_t stat_off, int qtile, int lane, const HeadMaps& hm) {
  const int T = a.T;
  const int r = lane & 31, half = lane >> 5;
  const int qi = qtile * 32 + r;
  const int qc = qi < T ? qi : T - 1;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    R.qf[ks] = __builtin_bit_cast(bf16x8, hm_load16(a.q + in_off + (int64_t)qc * a.sT, 2 * ks + half, hm.q));
    R.dof[ks] = __builtin_bit_cast(bf16x8, hm_load16(a.dout + o_off + (int64_t)qc * a.oT, 2 * ks + half, hm.o));
    R.of[ks] = __builtin_bit_cast(bf16x8, hm_load16(a.o + o_off + (int64_t)qc * a.oT, 2 * ks + half, hm.o));
  }
  R.lse = a.lse[stat_off + qc];
}
// ... and delta = <dO, O> once everything has landed
template <int KS>
__device__ __forceinline__ void finish_dq_rows(DqRows<KS>& R, const AttnBwdArgs& a, int64_t stat_off, int qtile,
                                               int lane, bool write_delta) {
  const int r = lane & 31, half = lane >> 5;
  const int qi = qtile * 32 + r;
  float delta = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) delta += (float)R.dof[ks][j] * (float)R.of[ks][j];
  delta += __shfl_xor(delta, 32, 64);
  R.delta = delta;
  if (write_delta && qi < a.T && half == 0) a.delta[stat_off + qi] = delta;
}

// the wave's key rows: lane (r, half) holds K[key][16 ks + 8 half ..] and V[key][..] = B operands (key on the lane)
template <int KS>
struct KvRows {
  bf16x8 kf[KS], vf[KS];
};
template <int KS>
__device__ __forceinline__ void load_kv_rows(KvRows<KS>& R, const AttnBwdArgs& a, int64_t in_off, int ktile, int lane,
                                             const HeadMaps& hm) {
  const int r = lane & 31, half = lane >> 5;
  const int ki = ktile * 32 + r;
  const int kcl = ki < a.T ? ki : a.T - 1;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    R.kf[ks] = __builtin_bit_cast(bf16x8, hm_load16(a.k + in_off + (int64_t)kcl * a.sT, 2 * ks + half, hm.k));
    R.vf[ks] = __builtin_bit_cast(bf16x8, hm_load16(a.v + in_off + (int64_t)kcl * a.sT, 2 * ks + half, hm.v));
  }
}


// A workgroup that owns ONE (b, h) of a backward launch and whose sample is dropped: +0 to the unit's dq, dk, dv rows and its
// delta, before any load - the caller returns right after.  nc = head_dim / 8.
__device__ __forceinline__ void zero_bwd_unit(const AttnBwdArgs& a, int64_t g_off, int64_t stat_off, const HeadMaps& hm, int nc,
                                              int tid, int nthr) {
  zero_head_rows(a.dq + g_off, a.gT, a.T, nc, hm.q, tid, nthr);
  zero_head_rows(a.dk + g_off, a.gT, a.T, nc, hm.k, tid, nthr);
  zero_head_rows(a.dv + g_off, a.gT, a.T, nc, hm.v, tid, nthr);
  zero_stats(a.delta + stat_off, a.T, tid, nthr);
}

// Block index -> (b, h) of a one-unit-per-workgroup backward launch with a stochastic-depth mask: the units of the KEPT samples
// come first - dealt by unit_of over n_kept H units, so the kept work fills whole rounds of workgroups evenly over the XCDs
// (dealing all B H units and leaving the dropped ones early made an XCD with many kept samples the tail of the launch:
// E max_x Binomial(8, 1/2) = 6.3 of its 8 samples at batch 64) - and the dropped samples' units after them.  Every wave works
// the mapping out for itself from the B factors, 64 samples per ballot word, in registers: no LDS, no barrier.
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int n, int lane) {
  const bool hit = ((m >> lane) & 1ull) && __builtin_popcountll(m & ((1ull << lane) - 1ull)) == n;
  return __builtin_ctzll(__builtin_amdgcn_ballot_w64(hit));
}
__device__ __forceinline__ void skip_unit(const float* scale, int B, int H, int idx, bool shared_rows, int lane, int& b, int& h,
                                          bool& dropped) {
  int nk = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const bool kept = b0 + lane < B && scale[b0 + lane] != 0.f;
    nk += __builtin_popcountll(__builtin_amdgcn_ballot_w64(kept));
  }
  const int uk = nk * H;
  dropped = idx >= uk;
  // (the dropped units too: the heads of a sample share cache lines, and a line zero-filled from one XCD's L2 is written once)
  const int u = dropped ? unit_of(idx - uk, B * H - uk, shared_rows) : unit_of(idx, uk, shared_rows);
  int want = u / H;                                  // ordinal among the kept (dropped) samples
  h = u - want * H;
  b = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const bool in = b0 + lane < B;
    const bool kept = in && scale[b0 + lane] != 0.f;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(dropped ? in && !kept : kept);
    const int cnt = __builtin_popcountll(m);
    if (want < cnt) { b = b0 + nth_set_bit(m, want, lane); break; }
    want -= cnt;
  }
  b = __builtin_amdgcn_readfirstlane(b);
  h = __builtin_amdgcn_readfirstlane(h);
}

// ---- LDS row images: bytes per row, shared by the resident and the streaming kernels -------------------------------
inline int attn_rsk(int hd) { return hd * 2 + 16; }                       // K image (odd # of 16-B slots)
inline int attn_rsv(int dp) { int r = dp * 2; return ((r / 4) % 32 == 0) ? r + 64 : r; }   // V image, dp = DT * 32 columns
// backward images, read both by rows (ds_read_b128) and transposed (ds_read_b64_tr_b16): rows are padded so the b128 reads
// are conflict-free, the transposed reads then see at most 2-way conflicts.  The tr fragments reach DT * 32 columns, so
// rows must hold that many (the pad columns meet zero accumulator columns / are discarded).
inline int attn_rs(int hd) { return (hd + 31) / 32 * 32 * 2 + 16; }

constexpr int kAttnMaxT = 16384;                   // longest sequence of the entry points
constexpr int kAttnWaves = 8;                      // resident backward: eight waves own tiles 0-7 and share a ninth
constexpr int kStreamWaves = 4;                    // csrc/attn_stream.hip: waves per workgroup
constexpr int kStreamRows = kStreamWaves * 32;     // own rows per workgroup
constexpr int kStreamBlk = 64;                     // streamed rows per LDS block
constexpr int kStreamThreads = kStreamWaves * 64;

// ---- which kernels an attention call runs -------------------------------------------------------------------------------
// attn_plan (csrc/attention.hip) is the ONE place that decides; octic_attn_plan reports it, the entry points launch it.  The
// launchers take every workgroup size and dynamic-LDS byte count from the plan: the number that decided is the number launched.
struct AttnPlan {
  int fwd, fwd_waves;          // OCTIC_ATTN_FWD_*
  size_t fwd_lds;
  int fwd_dbg;                 // developer probe of the head_dim-80 forward (OCTIC_ROUTE_ATTN_ONLINE >> 4)
  int bwd, bwd_waves;          // OCTIC_ATTN_BWD_*: what a phase-3 call runs
  size_t bwd_lds;              // SINGLE only
  int pair, pair_waves;        // phases 1 and 2 (and phase 3 unless bwd is SINGLE): OCTIC_ATTN_BWD_PAIR | STREAM | F32
  size_t dq_lds, dkv_lds;
  // Stochastic depth (AttnArgs::sample_scale): which of the planned kernels SKIP a sample whose factor is 0, i.e. read none of
  // its operands and store +0 - the others compute the sample.  fwd_skip_max_b: the forward skips in launches of up to that
  // many samples (0: never); bwd_skips / pair_skips: the phase-3 kernel / the phase-1 + phase-2 pair.  octic_attn_skip_plan.
  int fwd_skip_max_b;
  bool bwd_skips, pair_skips;
};
// Pure host arithmetic, no HIP call.  ld_*: token strides in elements of q/k/v, o/dout, dq/dk/dv (0: hd).  OCTIC_ESHAPE for
// the (T, hd) no kernel takes - the shape check of every attention entry point.
int attn_plan(int dtype, int T, int hd, int64_t ld_in, int64_t ld_out, int64_t ld_grad, AttnPlan* plan);

// KS = hd / 16 k-steps of the score product, DT = ceil(hd / 32) d-tiles of the output: f(KsDt<KS, DT>{})
template <int KS_, int DT_>
struct KsDt { static constexpr int KS = KS_, DT = DT_; };
template <typename F>
inline int attn_dispatch(int hd, F&& f) {
  switch (hd / 16) {
    case 1: return f(KsDt<1, 1>{});
    case 2: return f(KsDt<2, 1>{});
    case 3: return f(KsDt<3, 2>{});
    case 4: return f(KsDt<4, 2>{});
    case 5: return f(KsDt<5, 3>{});
    case 6: return f(KsDt<6, 3>{});
    case 7: return f(KsDt<7, 4>{});
    default: return f(KsDt<8, 4>{});
  }
}

// dynamic-LDS opt-in (up to the CU's 160 KiB) of a launcher's kernels, once per device
template <typename... K>
inline void attn_lds_optin(DeviceOnce& once, K... kernels) {
  if (!once.first()) return;
  ((void)hipFuncSetAttribute((const void*)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), ...);
  (void)hipGetLastError();
}

// csrc/attn80.hip: persistent head_dim-80 forwards (all operands by LDS-DMA, one head ahead), one-shot or online softmax
int attn80_fwd_launch(const AttnArgs& a, int64_t B, const AttnPlan& p, hipStream_t s);
// csrc/attn80_bwd.hip: single-pass backward (dq, dk, dv from ONE recomputation of P) for head_dim 80
int attn80_bwd_launch(const AttnBwdArgs& a, int64_t B, const AttnPlan& p, hipStream_t s);
// csrc/attn_stream.hip: K / V (Q / dO) streamed through LDS in blocks, any T
int attn_stream_fwd_launch(const AttnArgs& a, int64_t B, const AttnPlan& p, hipStream_t s);
int attn_stream_bwd_launch(const AttnBwdArgs& a, int64_t B, int phase, const AttnPlan& p, hipStream_t s);
// csrc/attn_f32.hip: dynamic LDS of its three kernels
size_t attn_f32_lds(int hd);

}  // namespace octic
