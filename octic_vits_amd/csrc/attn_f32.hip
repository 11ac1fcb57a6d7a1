// Softmax attention on float32 operands, forward and backward, any 0 < T <= 16384, head_dim a multiple of 16 up to 128.
// Every product runs on v_mfma_f32_16x16x4_f32, which is bit-for-bit a k-ordered fmaf chain: exact f32, no reduced
// precision anywhere.  One streaming design covers every T (the structure of csrc/attn_stream.hip):
//
//   * one workgroup = 4 waves = 128 rows of its own dimension (queries: forward, dq; keys: dkv), one wave per 32 = two
//     16-row tiles; the wave's own rows stay in registers for the whole walk.  Lane (c = lane & 15, g = lane >> 4) holds
//     elements [g hd/4, (g + 1) hd/4) of row c of a tile: the k index of an MFMA step is only a summation order, so step
//     s of a product over the head vector takes element g hd/4 + s from both operands (16-byte loads on both sides);
//   * the other operand streams through LDS in blocks of 32 rows, double-buffered with split staging: block j + 1 is
//     requested into registers before the products of block j and written to the other buffer after them, one barrier
//     per block.  LDS rows are padded to hd + 4 floats: the 16-byte row reads and the 4-byte column reads below are
//     both bank-conflict free;
//   * swapped product X = K Q^T: the accumulator of a 16 x 16 tile has its query on lane & 15 and keys 4 g + reg in its
//     four registers.  O^T = V^T P^T takes accumulator register `reg` as the B operand of step `reg` as it stands,
//     with the A operand of that step read from V row 4 g + reg: P never goes through LDS.  The backward is the same
//     shape three more times (dQ^T = K^T dS^T; key-owned: dV^T = dO^T P, dK^T = Q^T dS);
//   * online softmax in the exp2 domain on f32 statistics; row max and sum reduce over lanes l, l+16, l+32, l+48 in a
//     fixed order.  lse = m + log2(l) is the log2-domain log-sum-exp; the backward recomputes P = exp2(x scale log2e -
//     lse) and uses delta = rowsum(dO o O) (written by the query-owned phase, summed in the order of the dP entries);
//     a last block of at most 16 rows runs a one-tile instantiation of the block body;
//   * keys of the last block beyond T are masked to -inf (forward) / P = 0 (backward); rows beyond T are staged as zeros
//     so that P = 0 never meets a non-finite operand; no address beyond row T - 1 of any operand is read;
//   * every output element is written once by one lane, in a fixed order: no atomics, bitwise repeatable.
#include "attn_common.hpp"

namespace octic {

constexpr int kF32Waves = 4;                       // waves per workgroup
constexpr int kF32Rows = kF32Waves * 32;           // own rows per workgroup
constexpr int kF32Blk = 32;                        // streamed rows per LDS block
constexpr int kF32Threads = kF32Waves * 64;

struct AttnF32Args {
  const float* q; const float* k; const float* v; int64_t sB, sH, sT;   // element (b,h,t,d) at base + b*sB + h*sH + t*sT + d
  const float* o; const float* dout; float* out; int64_t oB, oH, oT;    // forward: out; backward: o and dout
  float* lse; float* delta;                                              // [B,H,T]
  float* dq; float* dk; float* dv; int64_t gB, gH, gT;
  int H, T, hd;
  float scale, scale_log2;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// x * s - m with the product rounded before the subtraction (no fma): where x is the row's own maximum and m its rounded
// scaled value - a one-hot row, T = 1 - the exponent is exactly 0 and P exactly 1, as in a softmax over rounded scores
__device__ __forceinline__ float scaled_minus(float x, float s, float m) {
#pragma clang fp contract(off)
  const float t = x * s;
  return t - m;
}

// rows row0 .. row0 + 31 of a tensor as the register operand of a wave: f[rt][i] = element g hd/4 + i of row rt*16 + c
template <int KC>
__device__ __forceinline__ void load_own(float (&f)[2][4 * KC], const float* base, int64_t st, int row0, int T, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int row = row0 + rt * 16 + c;
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (row < T) x = *(const f32x4*)(base + (int64_t)row * st + g * 4 * KC + 4 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j) f[rt][4 * i + j] = x[j];
    }
  }
}

// One block of rows of two tensors in flight through registers: chunk q = tid + it * 256 is (row q / kc, 16 bytes q % kc)
template <int KC>
struct F32Stage {
  static constexpr int kc = 4 * KC;                                  // 16-byte chunks of a head vector
  static constexpr int NR = (kF32Blk * kc + kF32Threads - 1) / kF32Threads;
  f32x4 a[NR], b[NR];
  float st;                                                          // dkv kernel: lse (threads 0-31) or delta (32-63)
};

template <int KC>
__device__ __forceinline__ void f32_request(F32Stage<KC>& R, const float* srcA, int64_t stA, const float* srcB, int64_t stB,
                                            int row0, int T, int tid) {
  using S = F32Stage<KC>;
#pragma unroll
  for (int it = 0; it < S::NR; ++it) {
    const int q = tid + it * kF32Threads, t = q / S::kc, ch = q - t * S::kc, row = row0 + t;
    R.a[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    R.b[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < kF32Blk && row < T) {
      R.a[it] = *(const f32x4*)(srcA + (int64_t)row * stA + ch * 4);
      R.b[it] = *(const f32x4*)(srcB + (int64_t)row * stB + ch * 4);
    }
  }
}

// rows >= T of the block are written as zeros; the 4 pad floats of a row are never read
template <int KC>
__device__ __forceinline__ void f32_write(const F32Stage<KC>& R, float* imgA, float* imgB, int rs, int tid) {
  using S = F32Stage<KC>;
#pragma unroll
  for (int it = 0; it < S::NR; ++it) {
    const int q = tid + it * kF32Threads, t = q / S::kc, ch = q - t * S::kc;
    if (t < kF32Blk) {
      *(f32x4*)(imgA + t * rs + ch * 4) = R.a[it];
      *(f32x4*)(imgB + t * rs + ch * 4) = R.b[it];
    }
  }
}

// x[st][rt] = (rows st*16 .. st*16 + 15 of the LDS image) (own rows of tile rt)^T, summed over the head vector:
// accumulator register reg of lane (c, g) is (streamed row st*16 + 4 g + reg, own row rt*16 + c).  NS = streamed 16-row
// tiles of the block that hold a real row (2; 1 in a last block of at most 16 rows): 2 NS independent accumulators.
template <int KC, int NS>
__device__ __forceinline__ void f32_scores(const float* img, int rs, const float (&own)[2][4 * KC], f32x4 (&x)[NS][2], int lane) {
  const float* r0 = img + (lane & 15) * rs + (lane >> 4) * 4 * KC;
#pragma unroll
  for (int st = 0; st < NS; ++st) x[st][0] = x[st][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < KC; ++i) {
    f32x4 av[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) av[st] = *(const f32x4*)(r0 + st * 16 * rs + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int st = 0; st < NS; ++st) {
        x[st][0] = mfma4(av[st][j], own[0][4 * i + j], x[st][0]);
        x[st][1] = mfma4(av[st][j], own[1][4 * i + j], x[st][1]);
      }
  }
}

// acc[rt][dt] (head columns dt*16 + 4 g + reg, own row rt*16 + c) += sum over the streamed rows of
// img[row][column] * w[st][rt][row]: step `reg` takes accumulator register reg of w as the B operand and image row
// 4 g + reg as the A operand
template <int KC, int NS>
__device__ __forceinline__ void f32_accumulate(const float* img, int rs, const f32x4 (&w)[NS][2], f32x4 (&acc)[2][KC], int lane) {
  const float* base = img + (4 * (lane >> 4)) * rs + (lane & 15);
#pragma unroll
  for (int st = 0; st < NS; ++st)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float* row = base + (st * 16 + reg) * rs;
#pragma unroll
      for (int dt = 0; dt < KC; ++dt) {
        const float a = row[dt * 16];
        acc[0][dt] = mfma4(a, w[st][0][reg], acc[0][dt]);
        acc[1][dt] = mfma4(a, w[st][1][reg], acc[1][dt]);
      }
    }
}

template <int KC>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[2][KC]) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int dt = 0; dt < KC; ++dt) acc[rt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// accumulators -> rows of a [.., T, hd] tensor: lane (c, g) writes columns dt*16 + 4 g .. + 3 of row rt*16 + c
template <int KC>
__device__ __forceinline__ void store_own(float* base, int64_t st, const f32x4 (&acc)[2][KC], float m0, float m1, int row0,
                                          int T, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int row = row0 + rt * 16 + c;
    const float mul = rt ? m1 : m0;
    if (row < T) {
#pragma unroll
      for (int dt = 0; dt < KC; ++dt) *(f32x4*)(base + (int64_t)row * st + dt * 16 + 4 * g) = acc[rt][dt] * mul;
    }
  }
}

struct F32Unit { int b, h, tile; };
__device__ __forceinline__ F32Unit f32_unit(int H, int ntile) {
  const int bh = blockIdx.x / ntile;
  F32Unit u;
  u.tile = blockIdx.x - bh * ntile;
  u.b = bh / H;
  u.h = bh - u.b * H;
  return u;
}

__device__ __forceinline__ float sum4lanes(float x) {
  x += __shfl_xor(x, 16, 64);
  x += __shfl_xor(x, 32, 64);
  return x;
}

// LDS: two buffers of {image A [32][rs], image B [32][rs], stats [64]} floats
__host__ __device__ inline int f32_buf_floats(int rs) { return 2 * kF32Blk * rs + 2 * kF32Blk; }

// ---- forward ---------------------------------------------------------------------------------------------------
// the NS key tiles of the block at key k0 against the wave's query rows; softmax state and O^T updated in place
template <int KC, int NS>
__device__ __forceinline__ void f32_fwd_block(const AttnF32Args& a, const float* Ks, const float* Vs, int rs,
                                              const float (&qf)[2][4 * KC], int k0, int lane, float (&m)[2], float (&l)[2],
                                              f32x4 (&ot)[2][KC]) {
  const int g = lane >> 4;
  f32x4 x[NS][2];
  f32_scores<KC, NS>(Ks, rs, qf, x, lane);
  if (k0 + NS * 16 > a.T) {
#pragma unroll
    for (int st = 0; st < NS; ++st)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (k0 + st * 16 + 4 * g + reg >= a.T) { x[st][0][reg] = -INFINITY; x[st][1][reg] = -INFINITY; }
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    float mx = fmaxf(fmaxf(x[0][rt][0], x[0][rt][1]), fmaxf(x[0][rt][2], x[0][rt][3]));
    if (NS == 2) mx = fmaxf(mx, fmaxf(fmaxf(x[NS - 1][rt][0], x[NS - 1][rt][1]), fmaxf(x[NS - 1][rt][2], x[NS - 1][rt][3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m[rt], mx * a.scale_log2);   // every block holds a real key: m_new is finite
    const float alpha = __builtin_amdgcn_exp2f(m[rt] - m_new);
    m[rt] = m_new;
#pragma unroll
    for (int dt = 0; dt < KC; ++dt) ot[rt][dt] *= alpha;
    float sum = 0.f;
#pragma unroll
    for (int st = 0; st < NS; ++st)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float p = __builtin_amdgcn_exp2f(scaled_minus(x[st][rt][reg], a.scale_log2, m_new));
        x[st][rt][reg] = p;
        sum += p;
      }
    l[rt] = __builtin_fmaf(l[rt], alpha, sum);
  }
  f32_accumulate<KC, NS>(Vs, rs, x, ot, lane);
}

// grid: ceil(T / 128) query tiles x B H heads
template <int KC>
__global__ __launch_bounds__(kF32Threads) void attn_f32_fwd_kernel(AttnF32Args a, int nqt) {
  extern __shared__ __attribute__((aligned(16))) float smem_f32[];
  const int T = a.T, rs = a.hd + 4;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
  const F32Unit u = f32_unit(a.H, nqt);
  const float* qb = a.q + u.b * a.sB + u.h * a.sH;
  const float* kb = a.k + u.b * a.sB + u.h * a.sH;
  const float* vb = a.v + u.b * a.sB + u.h * a.sH;
  const int row0 = u.tile * kF32Rows + wid * 32;
  const bool active = row0 < T;                       // wave-uniform; an idle wave still stages and meets the barriers
  const int img = kF32Blk * rs, buf = f32_buf_floats(rs);

  float qf[2][4 * KC];
  load_own<KC>(qf, qb, a.sT, row0, T, lane);
  F32Stage<KC> R;
  f32_request<KC>(R, kb, a.sT, vb, a.sT, 0, T, tid);
  f32_write<KC>(R, smem_f32, smem_f32 + img, rs, tid);
  __syncthreads();

  f32x4 ot[2][KC];
  zero_acc<KC>(ot);
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  const int nkb = (T + kF32Blk - 1) / kF32Blk;
  for (int blk = 0; blk < nkb; ++blk) {
    float* cur = smem_f32 + (blk & 1) * buf;
    float* nxt = smem_f32 + ((blk + 1) & 1) * buf;
    const bool more = blk + 1 < nkb;
    if (more) f32_request<KC>(R, kb, a.sT, vb, a.sT, (blk + 1) * kF32Blk, T, tid);
    if (active) {
      const int k0 = blk * kF32Blk;
      if (k0 + 16 < T) f32_fwd_block<KC, 2>(a, cur, cur + img, rs, qf, k0, lane, m, l, ot);
      else f32_fwd_block<KC, 1>(a, cur, cur + img, rs, qf, k0, lane, m, l, ot);
    }
    if (more) f32_write<KC>(R, nxt, nxt + img, rs, tid);   // nxt was last read before the previous barrier
    __syncthreads();
  }
  if (!active) return;
  const float l0 = sum4lanes(l[0]), l1 = sum4lanes(l[1]);
  if (g == 0 && a.lse) {
    float* lse = a.lse + ((int64_t)u.b * a.H + u.h) * T;
    if (row0 + c < T) lse[row0 + c] = m[0] + log2f(l0);
    if (row0 + 16 + c < T) lse[row0 + 16 + c] = m[1] + log2f(l1);
  }
  store_own<KC>(a.out + u.b * a.oB + u.h * a.oH, a.oT, ot, 1.0f / l0, 1.0f / l1, row0, T, lane);
}

// ---- backward, phase 1: delta and dQ per query tile; K and V stream ---------------------------------------------
template <int KC, int NS>
__device__ __forceinline__ void f32_dq_block(const AttnF32Args& a, const float* Ks, const float* Vs, int rs,
                                             const float (&qf)[2][4 * KC], const float (&dof)[2][4 * KC],
                                             const float (&lse)[2], const float (&delta)[2], int k0, int lane,
                                             f32x4 (&dqt)[2][KC]) {
  const int g = lane >> 4;
  f32x4 x[NS][2], dp[NS][2];
  f32_scores<KC, NS>(Ks, rs, qf, x, lane);
  f32_scores<KC, NS>(Vs, rs, dof, dp, lane);
#pragma unroll
  for (int st = 0; st < NS; ++st)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float p = __builtin_amdgcn_exp2f(scaled_minus(x[st][rt][reg], a.scale_log2, lse[rt]));
        if (k0 + st * 16 + 4 * g + reg >= a.T) p = 0.f;
        x[st][rt][reg] = p * (dp[st][rt][reg] - delta[rt]);
      }
  f32_accumulate<KC, NS>(Ks, rs, x, dqt, lane);
}

template <int KC>
__global__ __launch_bounds__(kF32Threads) void attn_f32_dq_kernel(AttnF32Args a, int nqt) {
  extern __shared__ __attribute__((aligned(16))) float smem_f32[];
  const int T = a.T, rs = a.hd + 4;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
  const F32Unit u = f32_unit(a.H, nqt);
  const int64_t in_off = u.b * a.sB + u.h * a.sH, o_off = u.b * a.oB + u.h * a.oH;
  const int64_t stat_off = ((int64_t)u.b * a.H + u.h) * T;
  const float* kb = a.k + in_off;
  const float* vb = a.v + in_off;
  const int row0 = u.tile * kF32Rows + wid * 32;
  const bool active = row0 < T;
  const int img = kF32Blk * rs, buf = f32_buf_floats(rs);

  F32Stage<KC> R;
  f32_request<KC>(R, kb, a.sT, vb, a.sT, 0, T, tid);
  float qf[2][4 * KC], dof[2][4 * KC];
  load_own<KC>(qf, a.q + in_off, a.sT, row0, T, lane);
  load_own<KC>(dof, a.dout + o_off, a.oT, row0, T, lane);
  // delta = rowsum(dO o O) as the diagonal of the MFMA product O dO^T: the same fmaf chain, in the same order, as the
  // dP = V dO^T entries it is subtracted from, so that dP - delta cancels exactly where a row of P is one-hot
  float lse[2], delta[2];
  {
    float of[2][4 * KC];
    load_own<KC>(of, a.o + o_off, a.oT, row0, T, lane);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4 * KC; ++i) d = mfma4(of[rt][i], dof[rt][i], d);
      // element (row 4 g + reg, column c): the diagonal entry of query c sits in lane c + 16 (c >> 2), register c & 3
      const int reg = c & 3;
      float mine = d[0];
      if (reg == 1) mine = d[1];
      if (reg == 2) mine = d[2];
      if (reg == 3) mine = d[3];
      delta[rt] = __shfl(mine, c + 16 * (c >> 2), 64);
      const int row = row0 + rt * 16 + c;
      lse[rt] = row < T ? a.lse[stat_off + row] : INFINITY;       // rows beyond T: P = exp2(0 - inf) = 0
      if (g == 0 && row < T) a.delta[stat_off + row] = delta[rt];   // for phase 2
    }
  }
  f32_write<KC>(R, smem_f32, smem_f32 + img, rs, tid);
  __syncthreads();

  f32x4 dqt[2][KC];
  zero_acc<KC>(dqt);
  const int nkb = (T + kF32Blk - 1) / kF32Blk;
  for (int blk = 0; blk < nkb; ++blk) {
    float* cur = smem_f32 + (blk & 1) * buf;
    float* nxt = smem_f32 + ((blk + 1) & 1) * buf;
    const bool more = blk + 1 < nkb;
    if (more) f32_request<KC>(R, kb, a.sT, vb, a.sT, (blk + 1) * kF32Blk, T, tid);
    if (active) {
      const int k0 = blk * kF32Blk;
      if (k0 + 16 < T) f32_dq_block<KC, 2>(a, cur, cur + img, rs, qf, dof, lse, delta, k0, lane, dqt);
      else f32_dq_block<KC, 1>(a, cur, cur + img, rs, qf, dof, lse, delta, k0, lane, dqt);
    }
    if (more) f32_write<KC>(R, nxt, nxt + img, rs, tid);
    __syncthreads();
  }
  if (active) store_own<KC>(a.dq + u.b * a.gB + u.h * a.gH, a.gT, dqt, a.scale, a.scale, row0, T, lane);
}

// ---- backward, phase 2: dK, dV per key tile; Q, dO, lse and delta stream -------------------------------------------
// padded queries of a partial tile meet lse = +inf: P = 0
template <int KC, int NS>
__device__ __forceinline__ void f32_dkv_block(const AttnF32Args& a, const float* Qs, const float* Ds, const float* stats,
                                              int rs, const float (&kf)[2][4 * KC], const float (&vf)[2][4 * KC], int lane,
                                              f32x4 (&dkt)[2][KC], f32x4 (&dvt)[2][KC]) {
  const int g = lane >> 4;
  f32x4 x[NS][2], dp[NS][2];
  f32_scores<KC, NS>(Qs, rs, kf, x, lane);            // X[query][key]
  f32_scores<KC, NS>(Ds, rs, vf, dp, lane);           // dP[query][key]
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const f32x4 l4 = *(const f32x4*)(stats + st * 16 + 4 * g), d4 = *(const f32x4*)(stats + kF32Blk + st * 16 + 4 * g);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float p = __builtin_amdgcn_exp2f(scaled_minus(x[st][rt][reg], a.scale_log2, l4[reg]));
        x[st][rt][reg] = p;
        dp[st][rt][reg] = p * (dp[st][rt][reg] - d4[reg]);
      }
  }
  f32_accumulate<KC, NS>(Ds, rs, x, dvt, lane);
  f32_accumulate<KC, NS>(Qs, rs, dp, dkt, lane);
}

template <int KC>
__global__ __launch_bounds__(kF32Threads) void attn_f32_dkv_kernel(AttnF32Args a, int nkt) {
  extern __shared__ __attribute__((aligned(16))) float smem_f32[];
  const int T = a.T, rs = a.hd + 4;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4;
  const F32Unit u = f32_unit(a.H, nkt);
  const int64_t in_off = u.b * a.sB + u.h * a.sH, o_off = u.b * a.oB + u.h * a.oH, g_off = u.b * a.gB + u.h * a.gH;
  const int64_t stat_off = ((int64_t)u.b * a.H + u.h) * T;
  const float* qb = a.q + in_off;
  const float* db = a.dout + o_off;
  const int row0 = u.tile * kF32Rows + wid * 32;
  const bool active = row0 < T;
  const int img = kF32Blk * rs, buf = f32_buf_floats(rs);

  F32Stage<KC> R;
  auto request = [&](int q0) {
    f32_request<KC>(R, qb, a.sT, db, a.oT, q0, T, tid);
    const int qi = q0 + (tid & (kF32Blk - 1));
    R.st = tid < kF32Blk ? INFINITY : 0.f;            // padded queries: P = exp2(x - inf) = 0, delta 0
    if (tid < 2 * kF32Blk && qi < T) R.st = tid < kF32Blk ? a.lse[stat_off + qi] : a.delta[stat_off + qi];
  };
  auto write = [&](float* b) {
    f32_write<KC>(R, b, b + img, rs, tid);
    if (tid < 2 * kF32Blk) b[2 * img + tid] = R.st;   // lse [32] | delta [32]
  };
  request(0);
  float kf[2][4 * KC], vf[2][4 * KC];
  load_own<KC>(kf, a.k + in_off, a.sT, row0, T, lane);
  load_own<KC>(vf, a.v + in_off, a.sT, row0, T, lane);
  write(smem_f32);
  __syncthreads();

  f32x4 dkt[2][KC], dvt[2][KC];
  zero_acc<KC>(dkt);
  zero_acc<KC>(dvt);
  const int nqb = (T + kF32Blk - 1) / kF32Blk;
  for (int blk = 0; blk < nqb; ++blk) {
    float* cur = smem_f32 + (blk & 1) * buf;
    float* nxt = smem_f32 + ((blk + 1) & 1) * buf;
    const bool more = blk + 1 < nqb;
    if (more) request((blk + 1) * kF32Blk);
    if (active) {
      if (blk * kF32Blk + 16 < T) f32_dkv_block<KC, 2>(a, cur, cur + img, cur + 2 * img, rs, kf, vf, lane, dkt, dvt);
      else f32_dkv_block<KC, 1>(a, cur, cur + img, cur + 2 * img, rs, kf, vf, lane, dkt, dvt);
    }
    if (more) write(nxt);
    __syncthreads();
  }
  if (active) {
    store_own<KC>(a.dk + g_off, a.gT, dkt, a.scale, a.scale, row0, T, lane);
    store_own<KC>(a.dv + g_off, a.gT, dvt, 1.0f, 1.0f, row0, T, lane);
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------
size_t attn_f32_lds(int hd) { return 2 * (size_t)f32_buf_floats(hd + 4) * sizeof(float); }   // <= 66.5 KiB

// dynamic-LDS opt-in of a kernel on the current device (head_dim 128 needs 66.5 KiB); a failure is reported as the
// positive hipError_t and tried again by the next call
template <typename K>
static int f32_lds_optin(K kernel, DeviceOnce& once) {
  if (!once.first()) return OCTIC_OK;
  const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_f32_lds(128));
  if (e == hipSuccess) return OCTIC_OK;
  (void)hipGetLastError();
  once.mask = 0;
  return (int)e;
}

template <int KC>
static int f32_fwd(const AttnF32Args& a, int64_t B, const AttnPlan& p, hipStream_t s) {
  const int nqt = (a.T + kF32Rows - 1) / kF32Rows;
  const int64_t grid = (int64_t)nqt * B * a.H;
  if (grid > 0x7FFFFFFF) return OCTIC_ESHAPE;
  static DeviceOnce once;
  if (const int rc = f32_lds_optin(attn_f32_fwd_kernel<KC>, once)) return rc;
  attn_f32_fwd_kernel<KC><<<(int)grid, kF32Threads, p.fwd_lds, s>>>(a, nqt);
  return launch_status();
}

template <int KC>
static int f32_bwd(const AttnF32Args& a, int64_t B, int phase, const AttnPlan& p, hipStream_t s) {
  const int ntile = (a.T + kF32Rows - 1) / kF32Rows;
  const int64_t grid = (int64_t)ntile * B * a.H;
  if (grid > 0x7FFFFFFF) return OCTIC_ESHAPE;
  static DeviceOnce once_dq, once_dkv;
  if (const int rc = f32_lds_optin(attn_f32_dq_kernel<KC>, once_dq)) return rc;
  if (const int rc = f32_lds_optin(attn_f32_dkv_kernel<KC>, once_dkv)) return rc;
  if (phase & 1) attn_f32_dq_kernel<KC><<<(int)grid, kF32Threads, p.dq_lds, s>>>(a, ntile);
  if (phase & 2) attn_f32_dkv_kernel<KC><<<(int)grid, kF32Threads, p.dkv_lds, s>>>(a, ntile);
  return launch_status();
}

static bool f32_rows_aligned(int64_t x) { return (x & 3) == 0; }   // 16-byte rows = 4 floats
// the -inf masking and the running maximum work on x * scale: the scale must be positive and finite
static bool f32_scale_ok(float scale) { return scale > 0.f && scale < INFINITY; }

}  // namespace octic

using namespace octic;

extern "C" {

int octic_attn_fwd_f32(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int H, int T, int hd,
                       int64_t sB, int64_t sH, int64_t sT, int64_t oB, int64_t oH, int64_t oT, float scale, void* stream) {
  if (!q || !k || !v || !o) return OCTIC_ENULL;
  AttnPlan p;
  if (B <= 0 || H <= 0 || attn_plan(OCTIC_F32, T, hd, sT, oT, 0, &p)) return OCTIC_ESHAPE;
  if (!f32_scale_ok(scale)) return OCTIC_ESHAPE;
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o)) & 15) return OCTIC_EALIGN;
  if (!f32_rows_aligned(sB | sH | sT | oB | oH | oT)) return OCTIC_EALIGN;
  AttnF32Args a = {};
  a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v; a.sB = sB; a.sH = sH; a.sT = sT;
  a.out = (float*)o; a.oB = oB; a.oH = oH; a.oT = oT;
  a.lse = lse;
  a.H = H; a.T = T; a.hd = hd;
  a.scale = scale;
  a.scale_log2 = scale * 1.4426950408889634f;
  hipStream_t s = (hipStream_t)stream;
  return attn_dispatch(hd, [&](auto c) { return f32_fwd<decltype(c)::KS>(a, B, p, s); });
}

int octic_attn_bwd_f32(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       float* delta, void* dq, void* dk, void* dv, int64_t B, int H, int T, int hd, int64_t sB, int64_t sH,
                       int64_t sT, int64_t oB, int64_t oH, int64_t oT, int64_t gB, int64_t gH, int64_t gT, float scale,
                       int phase, void* stream) {
  if (!q || !k || !v || !o || !dout || !lse || !delta || !dq || !dk || !dv) return OCTIC_ENULL;
  if (phase < 1 || phase > 3) return OCTIC_ESHAPE;
  AttnPlan p;
  if (B <= 0 || H <= 0 || attn_plan(OCTIC_F32, T, hd, sT, oT, 0, &p)) return OCTIC_ESHAPE;
  if (!f32_scale_ok(scale)) return OCTIC_ESHAPE;
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o) | ((uintptr_t)dout) | ((uintptr_t)dq) |
       ((uintptr_t)dk) | ((uintptr_t)dv)) & 15)
    return OCTIC_EALIGN;
  if (!f32_rows_aligned(sB | sH | sT | oB | oH | oT | gB | gH | gT)) return OCTIC_EALIGN;
  AttnF32Args a = {};
  a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v; a.sB = sB; a.sH = sH; a.sT = sT;
  a.o = (const float*)o; a.dout = (const float*)dout; a.oB = oB; a.oH = oH; a.oT = oT;
  a.lse = const_cast<float*>(lse); a.delta = delta;
  a.dq = (float*)dq; a.dk = (float*)dk; a.dv = (float*)dv; a.gB = gB; a.gH = gH; a.gT = gT;
  a.H = H; a.T = T; a.hd = hd;
  a.scale = scale;
  a.scale_log2 = scale * 1.4426950408889634f;
  hipStream_t s = (hipStream_t)stream;
  return attn_dispatch(hd, [&](auto c) { return f32_bwd<decltype(c)::KS>(a, B, phase, p, s); });
}

}  // extern "C"
