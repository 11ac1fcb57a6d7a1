// Softmax attention for long sequences (320 < T <= 16384; every T under OCTIC_ROUTE_ATTN_STREAM = 1), bf16, head_dim a
// multiple of 16 up to 128.  The kernels of csrc/attention.hip hold the whole K and V of a head in LDS, which caps T
// at 320; here K / V (forward, dq) or Q / dO (dkv) stream through LDS in blocks of 64 rows, double-buffered:
//
//   * one workgroup = 4 waves = 128 rows of its own dimension (queries: forward, dq; keys: dkv), one wave per 32;
//     the operand rows of the wave stay in registers for the whole walk;
//   * the arithmetic is that of attention.hip: swapped X = K Q^T on v_mfma_f32_32x32x16_bf16 (query on the lane),
//     P straight from the accumulators as the B operand of O^T = V^T P, V^T fragments by ds_read_b64_tr_b16, online
//     softmax in the exp2 domain; the backward recomputes P from the saved log-sum-exp (no T x T storage);
//   * staging is split (T14): block j + 1 is requested into registers before the products of block j and written to
//     the other LDS buffer after them, one barrier per block;
//   * keys of the last block beyond T are masked to -inf (forward) / P = 0 (backward); rows beyond T are staged as
//     zeros so that P = 0 never meets a non-finite operand;
//   * every gradient element is written once by one workgroup, in a fixed order: no atomics, bitwise repeatable.
// Packed rows (AttentionD8, head_dim 64 / 80) are gathered with HeadMap exactly as in the resident kernels.
#include "attn_common.hpp"

namespace octic {

// (kStreamWaves = 4 waves per workgroup, kStreamRows = 128 own rows, kStreamBlk = 64 streamed rows per LDS block: attn_common.hpp)

// One block of rows of two tensors in flight through registers: thread (row t0 + it * tstep, 16-byte chunk c).
template <int KS>
struct StreamStage {
  static constexpr int kc = 2 * KS;                          // 16-byte chunks of a head vector
  static constexpr int tstep = kStreamThreads / kc;          // rows per pass of the workgroup
  static constexpr int NR = (kStreamBlk + tstep - 1) / tstep;
  u32x4 a[NR], b[NR];
  float st;                                                  // dkv kernel: lse (threads 0-63) or delta (64-127)
};

template <int KS>
__device__ __forceinline__ void stream_request(StreamStage<KS>& R, const bf16* srcA, int64_t stA, const HeadMap mA,
                                               const bf16* srcB, int64_t stB, const HeadMap mB, int row0, int T, int tid) {
  using S = StreamStage<KS>;
  const int t0 = tid / S::kc, c = tid - t0 * S::kc;
#pragma unroll
  for (int it = 0; it < S::NR; ++it) {
    const int t = t0 + it * S::tstep, row = row0 + t;
    R.a[it] = u32x4{0, 0, 0, 0};
    R.b[it] = u32x4{0, 0, 0, 0};
    if (t0 < S::tstep && t < kStreamBlk && row < T) {
      R.a[it] = hm_load16(srcA + (int64_t)row * stA, c, mA);
      R.b[it] = hm_load16(srcB + (int64_t)row * stB, c, mB);
    }
  }
}

// rows >= T of the block are written as zeros; chunks >= kc of a row (the pad columns) are never touched here
template <int KS>
__device__ __forceinline__ void stream_write(const StreamStage<KS>& R, char* imgA, int rsA, char* imgB, int rsB, int tid) {
  using S = StreamStage<KS>;
  const int t0 = tid / S::kc, c = tid - t0 * S::kc;
  if (t0 >= S::tstep) return;
#pragma unroll
  for (int it = 0; it < S::NR; ++it) {
    const int t = t0 + it * S::tstep;
    if (t < kStreamBlk) {
      *(u32x4*)(imgA + (size_t)t * rsA + c * 16) = R.a[it];
      *(u32x4*)(imgB + (size_t)t * rsB + c * 16) = R.b[it];
    }
  }
}

// zero the pad chunks [kc, rs / 16) of every row of an image (read by the transposing fragments, never staged)
__device__ __forceinline__ void zero_pad_cols(char* img, int rs, int kc, int tid) {
  const int pc = rs / 16 - kc;
  for (int q = tid; q < kStreamBlk * pc; q += kStreamThreads) {
    const int t = q / pc, c = kc + (q - t * pc);
    *(u32x4*)(img + (size_t)t * rs + c * 16) = u32x4{0, 0, 0, 0};
  }
}

// (workgroup) -> (b, h, tile of the own dimension); the tiles of a head are dealt to one XCD (unit_of), so the streamed
// operand of a head is fetched into one L2
struct StreamUnit { int b, h, tile; };
__device__ __forceinline__ StreamUnit stream_unit(int H, int ntile) {
  const int u = unit_of(blockIdx.x, gridDim.x, true);
  const int bh = u / ntile;
  StreamUnit s;
  s.tile = u - bh * ntile;
  s.b = bh / H;
  s.h = bh - s.b * H;
  return s;
}

// ---- forward ---------------------------------------------------------------------------------------------------
// the key tiles (32 keys) of one block starting at key k0 against the wave's query fragments; state updated in place
template <int KS, int DT>
__device__ __forceinline__ void fwd_stream_block(const AttnArgs& a, const char* Ks, const char* Vs, int rsk, int rsv,
                                                 const bf16x8 (&qf)[KS], int k0, int lane, float& m, float& l,
                                                 f32x16 (&ot)[DT]) {
  const int T = a.T;
  const int r = lane & 31, half = lane >> 5;
#pragma unroll
  for (int j = 0; j < kStreamBlk / 32; ++j) {
    const int kbase = k0 + j * 32;
    if (kbase >= T) break;                             // block-uniform: every processed tile has a real key
    f32x16 x;
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = 0.f;
    const char* krow = Ks + (size_t)(j * 32 + r) * rsk + half * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(krow + ks * 32), qf[ks], x, 0, 0, 0);
    if (kbase + 32 > T) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (kbase + acc_row(i, half) >= T) x[i] = -INFINITY;
    }
    float mx = fmaxf(fmaxf(x[0], x[1]), x[2]);
#pragma unroll
    for (int i = 3; i < 15; i += 2) mx = fmaxf(fmaxf(mx, x[i]), x[i + 1]);
    mx = fmaxf(mx, x[15]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx * a.scale_log2);
    if (__builtin_amdgcn_ballot_w64(m_new > m)) {
      const float alpha = __builtin_amdgcn_exp2f(m - m_new);
      l *= alpha;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[d][i] *= alpha;
      m = m_new;
    }
    float ps[16];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      ps[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(x[i], a.scale_log2, -m));
      sum += ps[i];
    }
    l += sum;
    const bf16x8 pb0 = pack8(ps), pb1 = pack8(ps + 8);
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Vs, rsv, j * 32, d * 32, lane), pb0, ot[d], 0, 0, 0);
      ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Vs, rsv, j * 32 + 16, d * 32, lane), pb1, ot[d], 0, 0, 0);
    }
  }
}

// grid: ceil(T / 128) query tiles x B H heads; LDS: two buffers of {K image [64][rsk], V image [64][rsv]}.  Two waves
// per SIMD up to head_dim 80 (a register cap of 256); wider heads would spill under that cap and keep one.
template <int KS, int DT>
__global__ __launch_bounds__(kStreamThreads, KS <= 5 ? 2 : 1) void attn_fwd_stream_kernel(AttnArgs a, int rsk, int rsv, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T = a.T, hd = a.hd;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const StreamUnit su = stream_unit(a.H, nqt);
  const int64_t in_off = su.b * a.sB + su.h * a.sH;
  const HeadMaps hm = head_maps(a, su.h);
  const size_t kimg = (size_t)kStreamBlk * rsk, buf = kimg + (size_t)kStreamBlk * rsv;
  const int qtile = su.tile * kStreamWaves + wid;
  const bool active = qtile * 32 < T;                 // wave-uniform; an idle wave still stages and meets the barriers

  bf16x8 qf[KS];
  load_rows8<KS>(qf, a.q + in_off, a.sT, qtile, T, lane, hm.q);
  StreamStage<KS> R;
  stream_request<KS>(R, a.k + in_off, a.sT, hm.k, a.v + in_off, a.sT, hm.v, 0, T, tid);
  for (int i = 0; i < 2; ++i) {
    zero_pad_cols(smem + i * buf, rsk, 2 * KS, tid);
    zero_pad_cols(smem + i * buf + kimg, rsv, 2 * KS, tid);
  }
  stream_write<KS>(R, smem, rsk, smem + kimg, rsv, tid);
  __syncthreads();

  f32x16 ot[DT];
  zero_acc<DT>(ot);
  float m = -INFINITY, l = 0.f;
  const int nkb = (T + kStreamBlk - 1) / kStreamBlk;
  for (int kb = 0; kb < nkb; ++kb) {
    char* cur = smem + (kb & 1) * buf;
    char* nxt = smem + ((kb + 1) & 1) * buf;
    const bool more = kb + 1 < nkb;
    if (more) stream_request<KS>(R, a.k + in_off, a.sT, hm.k, a.v + in_off, a.sT, hm.v, (kb + 1) * kStreamBlk, T, tid);
    if (active) fwd_stream_block<KS, DT>(a, cur, cur + kimg, rsk, rsv, qf, kb * kStreamBlk, lane, m, l, ot);
    if (more) stream_write<KS>(R, nxt, rsk, nxt + kimg, rsv, tid);   // nxt was last read before the previous barrier
    __syncthreads();
  }
  if (!active) return;
  l += __shfl_xor(l, 32, 64);
  const int qi = qtile * 32 + r;
  if (qi < T) {
    if (half == 0 && a.lse) a.lse[((int64_t)su.b * a.H + su.h) * T + qi] = m + log2f(l);
    store_rows_wide<DT>(a.o + su.b * a.oB + su.h * a.oH + (int64_t)qi * a.oT, ot, 1.0f / l, hd, half, hm.o);
  }
}

// ---- backward, phase 1: dQ (and delta) per query tile; K and V stream ---------------------------------------------
template <int KS, int DT>
__device__ __forceinline__ void dq_stream_block(const AttnBwdArgs& a, const char* Ks, const char* Vs, int rs,
                                                const DqRows<KS>& R, int k0, int lane, f32x16 (&dqt)[DT]) {
  const int T = a.T;
  const int r = lane & 31, half = lane >> 5;
#pragma unroll
  for (int j = 0; j < kStreamBlk / 32; ++j) {
    const int kbase = k0 + j * 32;
    if (kbase >= T) break;
    f32x16 x, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { x[i] = 0.f; dp[i] = 0.f; }
    const char* krow = Ks + (size_t)(j * 32 + r) * rs + half * 16;
    const char* vrow = Vs + (size_t)(j * 32 + r) * rs + half * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(krow + ks * 32), R.qf[ks], x, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(vrow + ks * 32), R.dof[ks], dp, 0, 0, 0);
    }
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float p = __builtin_amdgcn_exp2f(x[i] * a.scale_log2 - R.lse);
      if (kbase + 32 > T && kbase + acc_row(i, half) >= T) p = 0.f;
      ds[i] = p * (dp[i] - R.delta);
    }
    const bf16x8 b0 = pack8(ds), b1 = pack8(ds + 8);
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      dqt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Ks, rs, j * 32, d * 32, lane), b0, dqt[d], 0, 0, 0);
      dqt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Ks, rs, j * 32 + 16, d * 32, lane), b1, dqt[d], 0, 0, 0);
    }
  }
}

// grid: ceil(T / 128) query tiles x B H heads; LDS: two buffers of {K image, V image}, both [64][rs].  Two waves per
// SIMD up to head_dim 64 (head_dim 80 spills under that cap).
template <int KS, int DT>
__global__ __launch_bounds__(kStreamThreads, KS <= 4 ? 2 : 1) void attn_bwd_dq_stream_kernel(AttnBwdArgs a, int rs, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T = a.T, hd = a.hd;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const StreamUnit su = stream_unit(a.H, nqt);
  const int64_t in_off = su.b * a.sB + su.h * a.sH, o_off = su.b * a.oB + su.h * a.oH;
  const int64_t stat_off = ((int64_t)su.b * a.H + su.h) * T;
  const HeadMaps hm = head_maps(a, su.h);
  const size_t img = (size_t)kStreamBlk * rs, buf = 2 * img;
  const int qtile = su.tile * kStreamWaves + wid;
  const bool active = qtile * 32 < T;

  DqRows<KS> mine;
  load_dq_rows<KS>(mine, a, in_off, o_off, stat_off, qtile, lane, hm);
  StreamStage<KS> R;
  stream_request<KS>(R, a.k + in_off, a.sT, hm.k, a.v + in_off, a.sT, hm.v, 0, T, tid);
  for (int i = 0; i < 4; ++i) zero_pad_cols(smem + i * img, rs, 2 * KS, tid);
  finish_dq_rows<KS>(mine, a, stat_off, qtile, lane, true);           // delta = <dO, O>, written for phase 2
  stream_write<KS>(R, smem, rs, smem + img, rs, tid);
  __syncthreads();

  f32x16 dqt[DT];
  zero_acc<DT>(dqt);
  const int nkb = (T + kStreamBlk - 1) / kStreamBlk;
  for (int kb = 0; kb < nkb; ++kb) {
    char* cur = smem + (kb & 1) * buf;
    char* nxt = smem + ((kb + 1) & 1) * buf;
    const bool more = kb + 1 < nkb;
    if (more) stream_request<KS>(R, a.k + in_off, a.sT, hm.k, a.v + in_off, a.sT, hm.v, (kb + 1) * kStreamBlk, T, tid);
    if (active) dq_stream_block<KS, DT>(a, cur, cur + img, rs, mine, kb * kStreamBlk, lane, dqt);
    if (more) stream_write<KS>(R, nxt, rs, nxt + img, rs, tid);
    __syncthreads();
  }
  const int qi = qtile * 32 + r;
  if (active && qi < T)
    store_rows_wide<DT>(a.dq + su.b * a.gB + su.h * a.gH + (int64_t)qi * a.gT, dqt, a.scale, hd, half, hm.q);
}

// ---- backward, phase 2: dK, dV per key tile; Q, dO, lse and delta stream -------------------------------------------
template <int KS, int DT>
__device__ __forceinline__ void dkv_stream_block(const AttnBwdArgs& a, const char* Qs, const char* Ds, const float* lse_s,
                                                 const float* del_s, int rs, const KvRows<KS>& R, int q0, int lane,
                                                 f32x16 (&dkt)[DT], f32x16 (&dvt)[DT]) {
  const int r = lane & 31, half = lane >> 5;
#pragma unroll
  for (int j = 0; j < kStreamBlk / 32; ++j) {
    if (q0 + j * 32 >= a.T) break;                    // padded queries of a partial tile meet lse = +inf: P = 0
    f32x16 x, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { x[i] = 0.f; dp[i] = 0.f; }
    const char* qrow = Qs + (size_t)(j * 32 + r) * rs + half * 16;
    const char* drow = Ds + (size_t)(j * 32 + r) * rs + half * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(qrow + ks * 32), R.kf[ks], x, 0, 0, 0);    // X'[q][key]
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(drow + ks * 32), R.vf[ks], dp, 0, 0, 0);  // dP[q][key]
    }
    float ps[16], ds[16];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int qq = j * 32 + 8 * g4 + 4 * half;           // accumulator rows 4 g4 .. 4 g4 + 3 are queries qq .. qq + 3
      const f32x4 l4 = *(const f32x4*)(lse_s + qq), d4 = *(const f32x4*)(del_s + qq);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int i = 4 * g4 + jj;
        const float p = __builtin_amdgcn_exp2f(x[i] * a.scale_log2 - l4[jj]);
        ps[i] = p;
        ds[i] = p * (dp[i] - d4[jj]);
      }
    }
    const bf16x8 p0 = pack8(ps), p1 = pack8(ps + 8), s0 = pack8(ds), s1 = pack8(ds + 8);
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      dvt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Ds, rs, j * 32, d * 32, lane), p0, dvt[d], 0, 0, 0);
      dvt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Ds, rs, j * 32 + 16, d * 32, lane), p1, dvt[d], 0, 0, 0);
      dkt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Qs, rs, j * 32, d * 32, lane), s0, dkt[d], 0, 0, 0);
      dkt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Qs, rs, j * 32 + 16, d * 32, lane), s1, dkt[d], 0, 0, 0);
    }
  }
}

// grid: ceil(T / 128) key tiles x B H heads; LDS: two buffers of {Q image, dO image [64][rs], lse [64], delta [64]}
template <int KS, int DT>
__global__ __launch_bounds__(kStreamThreads) void attn_bwd_dkv_stream_kernel(AttnBwdArgs a, int rs, int nkt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T = a.T, hd = a.hd;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const StreamUnit su = stream_unit(a.H, nkt);
  const int64_t in_off = su.b * a.sB + su.h * a.sH, o_off = su.b * a.oB + su.h * a.oH;
  const int64_t stat_off = ((int64_t)su.b * a.H + su.h) * T;
  const HeadMaps hm = head_maps(a, su.h);
  const size_t img = (size_t)kStreamBlk * rs, buf = 2 * img + 2 * kStreamBlk * sizeof(float);
  const int ktile = su.tile * kStreamWaves + wid;
  const bool active = ktile * 32 < T;

  KvRows<KS> kv;
  load_kv_rows<KS>(kv, a, in_off, ktile, lane, hm);
  StreamStage<KS> R;
  auto request = [&](int q0) {
    stream_request<KS>(R, a.q + in_off, a.sT, hm.q, a.dout + o_off, a.oT, hm.o, q0, T, tid);
    const int t = tid & (kStreamBlk - 1), qi = q0 + t;
    R.st = tid < kStreamBlk ? INFINITY : 0.f;         // padded queries: P = exp2(x - inf) = 0, delta 0
    if (tid < 2 * kStreamBlk && qi < T) R.st = tid < kStreamBlk ? a.lse[stat_off + qi] : a.delta[stat_off + qi];
  };
  auto write = [&](char* b) {
    stream_write<KS>(R, b, rs, b + img, rs, tid);
    if (tid < 2 * kStreamBlk) ((float*)(b + 2 * img))[tid] = R.st;   // lse [64] | delta [64]
  };
  request(0);
  for (int i = 0; i < 2; ++i) {
    zero_pad_cols(smem + i * buf, rs, 2 * KS, tid);
    zero_pad_cols(smem + i * buf + img, rs, 2 * KS, tid);
  }
  write(smem);
  __syncthreads();

  f32x16 dkt[DT], dvt[DT];
  zero_acc<DT>(dkt);
  zero_acc<DT>(dvt);
  const int nqb = (T + kStreamBlk - 1) / kStreamBlk;
  for (int qb = 0; qb < nqb; ++qb) {
    char* cur = smem + (qb & 1) * buf;
    char* nxt = smem + ((qb + 1) & 1) * buf;
    const bool more = qb + 1 < nqb;
    if (more) request((qb + 1) * kStreamBlk);
    if (active) {
      const float* st = (const float*)(cur + 2 * img);
      dkv_stream_block<KS, DT>(a, cur, cur + img, st, st + kStreamBlk, rs, kv, qb * kStreamBlk, lane, dkt, dvt);
    }
    if (more) write(nxt);
    __syncthreads();
  }
  const int ki = ktile * 32 + r;
  if (active && ki < T) {
    store_rows_wide<DT>(a.dk + su.b * a.gB + su.h * a.gH + (int64_t)ki * a.gT, dkt, a.scale, hd, half, hm.k);
    store_rows_wide<DT>(a.dv + su.b * a.gB + su.h * a.gH + (int64_t)ki * a.gT, dvt, 1.0f, hd, half, hm.v);
  }
}

// ---- launchers: the dynamic LDS comes with the plan (attn_plan, csrc/attention.hip) ------------------------------------
int attn_stream_fwd_launch(const AttnArgs& a, int64_t B, const AttnPlan& p, hipStream_t s) {
  const int nqt = (a.T + kStreamRows - 1) / kStreamRows;
  const int64_t grid = (int64_t)nqt * B * a.H;
  if (grid > 0x7FFFFFFF) return OCTIC_ESHAPE;
  return attn_dispatch(a.hd, [&](auto c) {
    constexpr int KS = decltype(c)::KS, DT = decltype(c)::DT;
    static DeviceOnce once;
    attn_lds_optin(once, attn_fwd_stream_kernel<KS, DT>);
    attn_fwd_stream_kernel<KS, DT><<<(int)grid, kStreamThreads, p.fwd_lds, s>>>(a, attn_rsk(a.hd), attn_rsv(DT * 32), nqt);
    return launch_status();
  });
}

int attn_stream_bwd_launch(const AttnBwdArgs& a, int64_t B, int phase, const AttnPlan& p, hipStream_t s) {
  const int rs = attn_rs(a.hd), ntile = (a.T + kStreamRows - 1) / kStreamRows;
  const int64_t grid = (int64_t)ntile * B * a.H;
  if (grid > 0x7FFFFFFF) return OCTIC_ESHAPE;
  return attn_dispatch(a.hd, [&](auto c) {
    constexpr int KS = decltype(c)::KS, DT = decltype(c)::DT;
    static DeviceOnce once;
    attn_lds_optin(once, attn_bwd_dq_stream_kernel<KS, DT>, attn_bwd_dkv_stream_kernel<KS, DT>);
    if (phase & 1) attn_bwd_dq_stream_kernel<KS, DT><<<(int)grid, kStreamThreads, p.dq_lds, s>>>(a, rs, ntile);
    if (phase & 2) attn_bwd_dkv_stream_kernel<KS, DT><<<(int)grid, kStreamThreads, p.dkv_lds, s>>>(a, rs, ntile);
    return launch_status();
  });
}

}  // namespace octic
