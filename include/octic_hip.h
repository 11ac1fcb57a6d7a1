/*
 * octic_hip.h — C ABI of the MI355X (gfx950) octic-ViT block engine.
 *
 * The reference (davnords/octic-vits) is pure Python; its replaceable surface for the hot path
 * is the set of torch modules in octic_vits/d8_layers.py and the one custom-op boundary
 * TritonGeluD8Function (octic_vits/d8_gelu.py:456-478).  This header is the boundary a
 * maintainer binds instead (ctypes stub in INTEGRATION.md): plain pointers, sizes and a HIP
 * stream — no torch types.  Every entry point cites the reference code it replaces.
 *
 * Conventions
 *  - All pointers are DEVICE pointers.  Nothing here allocates, frees or synchronises; work is
 *    enqueued on `stream` (a hipStream_t passed as void*), so calls are graph-capturable.
 *  - Return value: 0 on success, a negative OCTIC_E* code on a rejected argument, or the positive
 *    hipError_t of a failed launch.  octic_strerror() renders either.
 *  - An octic feature of M token rows and D = 8c channels is a 5-tuple (A1,A2,B1,B2:[M,c];
 *    E:[M,2,2c]) exactly as in the reference (d8_layers.py:64-81,111-112).  It is passed as an
 *    octic_view: five base pointers plus five row strides (in elements).  Two layouts matter:
 *      tuple  : five separate contiguous tensors            ld = {c,c,c,c,4c}
 *      packed : one [M, 8c] row  [A1|A2|B1|B2|E_row0|E_row1]  ptr[i] = base + i*c (i<4),
 *               ptr[4] = base + 4c, ld = {8c,...}  — the engine's native HBM layout
 *               ("(B, tokens, irrep, channel)"): one token = one contiguous row.
 *    Row r of E for token m starts at ptr[4] + m*ld[4] + r*2c.  E[..,r,0:c] / E[..,r,c:2c] are the
 *    two E copies (8-tuple entries x(4+r) / x(6+r), d8_utils.py:358-385).
 *  - c must be a multiple of 8 (16-byte vectors in bf16); every base pointer and row stride
 *    must keep rows 16-byte aligned.  Violations return OCTIC_EALIGN/OCTIC_ESHAPE — they are never
 *    silently routed to a slower path.
 *  - dtype codes: OCTIC_F32 (exact f32 MFMA path, used for the reference's fp32 equivariance
 *    tolerances) and OCTIC_BF16 (bf16 operands, f32 accumulate — the training path).
 */
#ifndef OCTIC_HIP_H
#define OCTIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCTIC_ABI_VERSION 20

enum { OCTIC_F32 = 0, OCTIC_BF16 = 1, OCTIC_U8 = 2 /* octic_augment_u8's pixel output only */ };

enum {
  OCTIC_OK = 0,
  OCTIC_ESHAPE = -1,   /* c not a multiple of 8, non-positive sizes, heads not dividing c ... */
  OCTIC_EALIGN = -2,   /* pointer or row stride breaks 16-byte row alignment */
  OCTIC_EDTYPE = -3,   /* unsupported dtype combination */
  OCTIC_ENULL = -4,    /* required pointer is NULL */
  OCTIC_EWORKSPACE = -5 /* workspace too small (see the *_workspace_bytes query) */
};

typedef struct {
  void* ptr[5];   /* A1, A2, B1, B2, E */
  int64_t ld[5];  /* row stride in ELEMENTS (E: stride between tokens, the 2 rows are adjacent) */
} octic_view;

int octic_abi_version(void);
const char* octic_strerror(int code);

/* ---- routing overrides (measurement / tests) --------------------------------------------------
 * Every entry point chooses its kernel and tiling from the shapes alone.  The alternatives it chooses between are all
 * shipped; this ONE call forces a choice so that an A/B or a test can run the other kernel on the same operands.
 * Parity-tested under a forced value (tests/): DENSE_TILE, WGRAD_TILE, LINEAR_RING, DENSE_IMAGE, DENSE_CLS2, ATTN_STREAM
 * and the three attention knobs ATTN_LEGACY, ATTN_ONLINE, ATTN_BWD_PAIR (tests/test_attn_resident_gpu.py).  NOT set by
 * any test: DENSE_SPLIT, WGRAD_SLABS and RING_EVEN - the tests reach those alternatives only where the automatic
 * choice picks them; the forced values are exercised by the A/B tools (tools/ab_dense_tile.py, tools/bench_tn.py,
 * tools/wreg_check.py) alone.
 * It is the library's only process-global mutable state: not thread-safe against concurrent launches,
 * value 0 = automatic (the default), returns the previous value (OCTIC_ESHAPE for an unknown knob).              */
enum {
  OCTIC_ROUTE_DENSE_TILE = 0,      /* octic_dense_gemm_nt plain mode: 4 = 256 x 256 tile, 5 = 256 x 320 tile; + 16 / + 32 =
                                      octic_dense_gemm_nt_tokens_adaptive always runs the 320- / the 256-wide tile          */
  OCTIC_ROUTE_DENSE_SPLIT = 1,     /* octic_dense_gemm_nt: n = K-split of the last partial round (1 = unsplit, in front)  */
  OCTIC_ROUTE_WGRAD_SLABS = 2,     /* octic_dense_wgrad_tn: number of row slabs                                           */
  OCTIC_ROUTE_WGRAD_TILE = 3,      /* octic_dense_wgrad_tn: 256 | 320 = tile width along K                                */
  OCTIC_ROUTE_LINEAR_RING = 4,     /* octic_linear_d8_fwd: 1 = ring kernel for every shape (no W-stationary kernel)       */
  OCTIC_ROUTE_RING_EVEN = 5,       /* octic_linear_d8_fwd ring kernel: 1 = even item spread instead of the planned order  */
  OCTIC_ROUTE_ATTN_LEGACY = 6,     /* octic_attn_*: 1 = the two-kernel online-softmax family for every shape              */
  OCTIC_ROUTE_ATTN_ONLINE = 7,     /* octic_attn_fwd*: 1 = persistent online-softmax forward instead of the one-shot one  */
  OCTIC_ROUTE_ATTN_BWD_PAIR = 8,   /* octic_attn_bwd*: 1 = the dq + dkv kernel pair instead of the single-pass backward   */
  OCTIC_ROUTE_DENSE_IMAGE = 9,     /* octic_dense_gemm_nt_tokens: 1 = per-image panels wherever legal, 2 = never, 3 = plain only;
                                      octic_dense_gemm_nt_tokens_image: + 4 = per-image panels wherever it can take the launch,
                                      + 8 = class-token rows in a launch of their own, + 16 = never (the former call)           */
  OCTIC_ROUTE_DENSE_CLS2 = 10,     /* class-token rows of per-image launches as two launches (K split): 1 = never, 2 = wherever legal */
  OCTIC_ROUTE_ATTN_STREAM = 11,    /* octic_attn_*: 1 = the streaming (K / V through LDS in blocks) kernels for every T too   */
  OCTIC_ROUTE_COUNT = 12
};
int octic_route_override(int knob, int value);

/* ---- D8 GELU -------------------------------------------------------------------------------
 * Replaces d8_gelu_fwd / d8_gelu_bwd (Triton, d8_gelu.py:104-196, 210-331, 333-453) and the
 * torch twin GeluD8 (d8_layers.py:98-102): per (row, channel j) gather the 8 isotypic
 * components, iso->regular butterfly, exact-erf GELU, regular->iso.  Arithmetic is f32 in
 * registers for both dtypes (the reference's bf16 path does the butterflies in bf16,
 * d8_gelu.py:11-26; f32 is strictly more accurate).  y may alias x.                       */
int octic_gelu_d8_fwd(const octic_view* x, const octic_view* y, int64_t M, int c, int dtype, void* stream);
/* gin = F( gelu'(F^-1 x) * F^-1 g )   (d8_gelu.py:283-321) */
int octic_gelu_d8_bwd(const octic_view* g, const octic_view* x, const octic_view* gin, int64_t M, int c,
                      int dtype, void* stream);
/* The same two with the stochastic-depth factor of the branch they sit in: sample_scale[M / rows_per_sample] (f32, device),
 * one entry per sample of rows_per_sample consecutive token rows; NULL = the plain call.  CONTRACT, for every kernel the
 * entry points can launch (four or eight channels per thread, bf16 and f32): for a sample whose factor is exactly 0 the
 * kernel reads NONE of its input rows (x; g and x in the backward) and writes +0 to every element of its output rows (y;
 * gin) - the caller may hand over rows that were never written, and may rely on the zeros.  Every other row is bit for bit
 * what the plain call writes.  Same launch shape as the plain call (nothing depends on the mask's values on the host).
 * OCTIC_ESHAPE when the mask is given and rows_per_sample <= 0 or M % rows_per_sample != 0.                              */
int octic_gelu_d8_fwd_skip(const octic_view* x, const octic_view* y, int64_t M, int c, int dtype,
                           const float* sample_scale, int64_t rows_per_sample, void* stream);
int octic_gelu_d8_bwd_skip(const octic_view* g, const octic_view* x, const octic_view* gin, int64_t M, int c, int dtype,
                           const float* sample_scale, int64_t rows_per_sample, void* stream);

/* ---- LayerNormD8 (+AffineD8) -----------------------------------------------------------------
 * Replaces LayerNormD8.forward (d8_layers.py:166-186): per-segment mean removal, one shared
 * std = (sqrt2/4)*sqrt(sum_1D var + mean_rows var_E + eps), then alpha (and beta on A1).
 * x is f32 (the residual stream); y is out_dtype.  alpha[i] may be NULL as a group (=> no affine,
 * elementwise_affine=False); beta may be NULL.  stats (optional, [M,8] f32: 6 means, rstd, 0) is
 * what the backward needs.                                                                     */
int octic_layernorm_d8_fwd(const octic_view* x, const octic_view* y, const float* const alpha[5],
                           const float* beta, float* stats, int64_t M, int c, float eps, int out_dtype,
                           void* stream);
/* dx = (dres ? dres : 0) + LN'(g).  g is g_dtype, x/dx/dres are f32.  Column sums for the affine
 * parameters are written as per-block partial slabs into `partials` ([nblk, 2, 8c] f32,
 * nblk = octic_layernorm_d8_bwd_blocks(M)); reduce them with octic_layernorm_d8_bwd_finish.     */
int octic_layernorm_d8_bwd_blocks(int64_t M);
int octic_layernorm_d8_bwd(const octic_view* g, const octic_view* x, const float* stats,
                           const float* const alpha[5], const octic_view* dres, const octic_view* dx,
                           float* partials, int64_t M, int c, int g_dtype, void* stream);
/* octic_layernorm_d8_bwd_cast: octic_layernorm_d8_bwd for a bf16 cotangent on packed rows with c in {32,...,160}
 * (other arguments: OCTIC_ESHAPE, call the two kernels), which also stores gcast[row] = bf16(rs[row / rows_per_sample] *
 * dx[row]) (packed rows of 8c, rs may be NULL): the drop-path-scaled bf16 cotangent that the backward of the
 * residual-fused LinearD8 in front of this norm needs (d8_layers.py:698-707 chained over two branches) - what
 * octic_cast_rowscale makes of dx in a pass of its own.                                                          */
int octic_layernorm_d8_bwd_cast(const octic_view* g, const octic_view* x, const float* stats, const float* const alpha[5],
                                const octic_view* dres, const octic_view* dx, float* partials, int64_t M, int c,
                                const float* rs, int64_t rows_per_sample, void* gcast, void* stream);
/* octic_layernorm_d8_bwd_skip / octic_layernorm_d8_bwd_cast_skip: the two above with the stochastic-depth factor of the
 * branch this norm OPENS as a sample mask (sample_scale: one f32 per rows_per_sample rows, NULL = the calls above;
 * rows_per_sample <= 0 or M % rows_per_sample != 0 with a mask: OCTIC_ESHAPE).  sample_scale[b] == 0 PROMISES that the rows
 * of g of sample b are zero - the branch's first GEMM stores exact zeros for a dropped sample - and the kernel may then leave
 * those rows of g, x and stats unread: dx = dres (zeros without dres), gcast = bf16(rs * dres), nothing added to the
 * partials.  With the promise kept and x finite every output equals the unmasked call, up to the sign of an exact zero
 * (which no comparison of values sees).  Honoured by the bf16 kernel for packed rows with c <= 160; every other route
 * reads all rows.                                                                                                   */
int octic_layernorm_d8_bwd_skip(const octic_view* g, const octic_view* x, const float* stats, const float* const alpha[5],
                                const octic_view* dres, const octic_view* dx, float* partials, int64_t M, int c, int g_dtype,
                                const float* sample_scale, int64_t rows_per_sample, void* stream);
int octic_layernorm_d8_bwd_cast_skip(const octic_view* g, const octic_view* x, const float* stats,
                                     const float* const alpha[5], const octic_view* dres, const octic_view* dx,
                                     float* partials, int64_t M, int c, const float* rs, int64_t rows_per_scale, void* gcast,
                                     const float* sample_scale, int64_t rows_per_sample, void* stream);
/* octic_layernorm_d8_bwd_cast_inplace: octic_layernorm_d8_bwd_cast_skip where dres and dx are ONE buffer (`dx`: on entry the
 * residual cotangent, on return the stream cotangent).  sample_scale is required (NULL: OCTIC_ENULL), packed rows, c = 32 ...
 * 160 in steps of 32 (else OCTIC_ESHAPE).  Which rows of `dx` are touched:
 *   sample_scale != 0 (live row):            read, then written with LN'(g) + dres by the lane that read each address;
 *   sample_scale == 0, rs != 0 (or rs NULL): read only (dx = dres is what the buffer holds; gcast = bf16(rs * dres));
 *   sample_scale == 0, rs == 0:              neither read nor written; gcast is an exact zero row.
 * The promise of sample_scale is that of the _skip calls.  gcast is written for every row; partials, slabs and the order of
 * every sum are those of octic_layernorm_d8_bwd_cast_skip, and so is every value, up to the sign of an exact zero.       */
int octic_layernorm_d8_bwd_cast_inplace(const octic_view* g, const octic_view* x, const float* stats,
                                        const float* const alpha[5], const octic_view* dx, float* partials, int64_t M, int c,
                                        const float* rs, int64_t rows_per_scale, void* gcast, const float* sample_scale,
                                        int64_t rows_per_sample, void* stream);
int octic_layernorm_d8_bwd_finish(const float* partials, int nblk, int c, float* const dalpha[5], float* dbeta,
                                  void* stream);
/* njobs of the reductions above in ceil(njobs / 48) launches, bit-identical to njobs calls (see octic_dense_finish_batch). */
typedef struct octic_ln_finish_job {
  const float* partials; /* [nblk][2][8c] */
  float* dalpha[5];      /* each may be NULL */
  float* dbeta;          /* may be NULL */
  int nblk;
  int c;
} octic_ln_finish_job;
int octic_layernorm_d8_bwd_finish_batch(const octic_ln_finish_job* jobs, int njobs, void* stream);

/* Sample blocks between a full batch and a compacted one (the opt-in batch compaction of stochastic depth, drop_path_d8 of
 * d8_layers.py:249-270 computed on the kept samples only): scatter == 0: dst[i] = src[idx[i]], scatter != 0: dst[idx[i]] =
 * src[i], i < n; a block = block_bytes (multiple of 16) = one sample's token rows; idx int64 on the device, distinct.        */
int octic_sample_blocks(const void* src, void* dst, const int64_t* idx, int64_t n, int64_t block_bytes, int scatter,
                        void* stream);

/* ---- LinearD8 (irrep-blocked GEMM on MFMA) ----------------------------------------------------
 * Replaces LinearD8.forward (d8_layers.py:124-127) = five nn.Linear calls, as ONE launch:
 *     y_g[m, n] = resid_g[m, n] + rs[token(m)/rows_per_sample] * cs_g[n] * ( sum_k x_g[m,k] W_g[n,k] + bias[n] (g==A1) )
 * W_g: [cout_g, cin_g] row-major in `dtype` (nn.Linear layout), g = A1,A2,B1,B2 (c wide) and E
 * (2c wide, shared by both E rows, d8_layers.py:127).  resid (out_dtype view), rs (f32 per
 * sample: drop-path mask/keep-prob, d8_layers.py:256-270), cs (f32 per channel: AffineD8 /
 * LayerScaleD8 gamma, d8_layers.py:147-158,205-212) and bias (f32 [cout]) are each optional
 * (NULL) — together they fuse `x + drop_path(gamma * linear(h))` (d8_layers.py:704-707) into
 * the GEMM epilogue.  The same entry point computes the input gradient when given the
 * transposed weights (dX = dY W  ==  linear with W^T).  x and W are `dtype`; y/resid are
 * out_dtype.  Supported (dtype,out_dtype): (F32,F32), (BF16,BF16), (BF16,F32).             */
int octic_linear_d8_fwd(const octic_view* x, const void* const w[5], const float* bias, const octic_view* y,
                        const octic_view* resid, const float* rs, int64_t rows_per_sample,
                        const float* const cs[5], int64_t M, int cin, int cout, int dtype, int out_dtype,
                        void* stream);
/* The same with the stochastic-depth factor of the branch the GEMM sits in: sample_scale[M / skip_rows_per_sample] (f32,
 * device), one entry per sample of skip_rows_per_sample consecutive token rows; NULL = the plain call.  CONTRACT: a factor of
 * exactly 0 says that NOBODY will read the output rows of that sample; the kernel may leave those rows unwritten and the sample's
 * input rows unread.  Every row of a sample whose factor is not 0 is bit for bit what the unmasked launch writes.  The W-stationary
 * kernel honours the mask per 32-row tile (a tile is left out iff every token row it covers belongs to samples with factor 0)
 * and deals the remaining tiles evenly over its workgroups; a launch the plan routes to the ring or the register-staged kernel
 * computes every row, as does one with more than 4096 row tiles in an irrep group - the contract allows both.  The plan
 * (octic_linear_d8_plan) and the launch shape do not depend on the mask.  OCTIC_ESHAPE for a masked call that also carries a
 * residual, rs or a non-NULL cs array (a fused tail writes the stream itself: every row has a reader), or with
 * skip_rows_per_sample <= 0 or M % skip_rows_per_sample != 0.                                                              */
int octic_linear_d8_fwd_skip(const octic_view* x, const void* const w[5], const float* bias, const octic_view* y,
                             const octic_view* resid, const float* rs, int64_t rows_per_sample,
                             const float* const cs[5], int64_t M, int cin, int cout, int dtype, int out_dtype,
                             const float* sample_scale, int64_t skip_rows_per_sample, void* stream);
/* The same with a mask of another kind: dropped[M / dropped_rows_per_sample] (f32, device; a factor of exactly 0 = the sample is
 * dropped by stochastic depth; NULL = the plain call).  Where _skip says "nobody reads those rows", this says "those rows are
 * known": the caller promises what makes the dropped samples' work void, and every output row is still defined.  CONTRACT:
 *   plain launch (no resid / rs / cs): bias must be NULL, and the caller promises that EVERY INPUT ROW of a dropped sample is zero.
 *     The kernel may leave those rows unread and writes +0 to every output row of a dead tile (a 128-row tile all of whose
 *     tokens belong to dropped samples).  Kept samples' rows are bit for bit the unmasked launch's; dropped samples' rows
 *     compare equal to it (zeros either way).
 *   fused launch: needs resid and rs, and dropped_rows_per_sample == rows_per_sample; the caller promises rs[b] == 0 wherever
 *     dropped[b] == 0 (the same array will do).  A dead tile's output rows are its resid rows copied, x unread.
 *   OCTIC_ESHAPE: a plain masked launch with a bias; a fused one without resid or rs or with unequal row counts;
 *     dropped_rows_per_sample <= 0 or M % dropped_rows_per_sample != 0; a mask with the lift addressing.
 * Ignoring the mask is always correct under this contract: only the ring kernel's SKIP instantiation (bf16 operands,
 * linear_d8_ring_kernel<.., SKIP>, at most 1024 row tiles per irrep group) honours it - it runs the live items first, dealt evenly
 * over the XCDs, and a dead item neither loads nor multiplies; the W-stationary and register-staged kernels and f32 operands
 * compute every row.  The plan (octic_linear_d8_plan) and the launch shape do not depend on the mask.                          */
int octic_linear_d8_fwd_dropped(const octic_view* x, const void* const w[5], const float* bias, const octic_view* y,
                                const octic_view* resid, const float* rs, int64_t rows_per_sample,
                                const float* const cs[5], int64_t M, int cin, int cout, int dtype, int out_dtype,
                                const float* dropped, int64_t dropped_rows_per_sample, void* stream);

/* Compute-dtype copies of the f32 master weights in ONE launch per layer: wb = [W_A1|W_A2|W_B1|W_B2|W_E]
 * (forward), wt = each matrix transposed with the layer-scale folded in, wt_g[k][n] = cs_g[n] W_g[n][k]
 * (input gradient dX = dY diag(cs) W).  Either output may be NULL; cs may be NULL.                 */
int octic_linear_d8_prep(const float* const w32[5], const float* const cs[5], int cin, int cout, void* wb, void* wt,
                         int dtype, void* stream);
/* The same for many layers in ONE launch (after an optimizer step).  items_dev: device array sorted by block_begin;
 * item i owns workgroups [block_begin, block_begin + block_count) of the total_blocks launched, with block_count =
 * octic_linear_d8_prep_batch_blocks(cin, cout) (one 64 x 64 tile of one irrep's matrix each); wb / wt / cs[] entries
 * may be NULL as in octic_linear_d8_prep.                                                              */
typedef struct octic_prep_item {
  const float* w[5];
  const float* cs[5];
  void* wb;
  void* wt;
  int32_t cin, cout;
  int32_t block_begin, block_count;
} octic_prep_item;
int octic_linear_d8_prep_batch_blocks(int cin, int cout);
int octic_linear_d8_prep_batch(const octic_prep_item* items_dev, int n_items, int total_blocks, int dtype, void* stream);

/* Output-tile width (32*NT) the launcher picks for this problem; the kernel instantiation that runs is
 * linear_d8_kernel<TIN, TOUT, NT> — exposed so profilers/benchmarks can name it.                 */
int octic_linear_d8_tile_n(int64_t M, int cin, int cout);
/* Host-only query (no device call): what octic_linear_d8_fwd runs for this problem, as decided by the one routing function
 * of the library (linear_plan, csrc/gemm.hip) under the current octic_route_override table.  fused: whether the call passes a
 * residual, a per-sample scale or column scales.  out[0] = kernel (OCTIC_LINEAR_*), out[1] = columns per output tile (0 for
 * the W-stationary kernel, which sizes its column chunks per irrep), out[2] = 1 when the fused-epilogue instantiation runs,
 * out[3] = 0.  OCTIC_ESHAPE / OCTIC_EDTYPE exactly where the entry point returns them for (M, cin, cout, dtype, out_dtype). */
enum {
  OCTIC_LINEAR_WREG = 0,     /* csrc/gemm_wreg.hip linear_d8_wreg_kernel<TOUT, fused>: bf16, cin a multiple of 32 in 32 .. 160 */
  OCTIC_LINEAR_RING = 1,     /* linear_d8_ring_kernel<TIN, TOUT, fused, ..>: cin a multiple of 32 (bf16) | 16 (f32); tile 80 | 160 */
  OCTIC_LINEAR_CLASSIC = 2   /* linear_d8_kernel<TIN, TOUT, NT>: register-staged, tile 32 NT, any legal cin                  */
};
int octic_linear_d8_plan(int64_t M, int cin, int cout, int dtype, int out_dtype, int fused, int out[4]);
/* Host-only query (no device call): the workgroup -> item order of a long-K ("ring") launch.  A launch is `ngroups` (<= 5)
 * item classes, class g with items[g] items of ksteps[g] K-steps each (class 0 = the long one, the E irrep); workgroups are
 * dispatched in blockIdx order round-robin over the 8 XCDs to slots_per_xcd slots each, so the order is a schedule.
 * out_group / out_item (sum(items) entries each) receive, per workgroup, the item it runs.  Returns 1 if the planned order
 * applies, 0 for the even spread, negative on bad arguments.                                                            */
int octic_linear_d8_ring_order(int ngroups, const int* items, const int* ksteps, int slots_per_xcd, int* out_group,
                               int* out_item);
/* The same for a masked ring launch (octic_linear_d8_fwd_dropped), through the kernel's own mapping function: class g has
 * items[g] row tiles of n_chunks[g] column chunks each (n_chunks NULL = 1 each; classes 1.. must be equal), dead_long[items[0]] /
 * dead_short[items[1]] flag the dead row tiles (non-zero = dead; the short classes cover the same rows).  out_group / out_item /
 * out_dead (nullable), sum(items * n_chunks) entries each: per workgroup the class, the item (row tile * n_chunks + chunk) and
 * whether it is dead.  In every XCD's dispatch order (workgroups x, x + 8, ..) live long items come first, then live short
 * ones, then dead ones; live items are shared evenly over the XCDs; the chunks of a long row tile are consecutive workgroups
 * of one XCD where the launch has ceil(items[0] / 8) * n_chunks[0] rounds.  Returns the number of workgroups, OCTIC_ESHAPE for
 * a launch the masked kernel does not take (unequal short classes, more than 1024 row tiles).                              */
int octic_linear_d8_ring_order_dropped(int ngroups, const int* items, const int* ksteps, int slots_per_xcd, const int* n_chunks,
                                       const unsigned char* dead_long, const unsigned char* dead_short, int* out_group,
                                       int* out_item, int* out_dead);

/* Weight gradient  G_g[n,k] = sum_rows dy_g[row,n] x_g[row,k]  (E: both rows).  Reduction over the
 * M (2M) rows is split over `splits` row ranges whose f32 partial slabs go to `workspace`
 * (octic_linear_d8_wgrad_workspace_bytes).  The finish kernel sums the slabs in a fixed order
 * (bitwise reproducible) and applies the layer-scale chain rule when cs != NULL:
 *     dW_g[n,k] = cs_g[n] * G_g[n,k]
 *     dcs_g[n]  = sum_k W_g[n,k] G_g[n,k]  + (g==A1 ? bias[n]*dysum[n] : 0)
 *     dbias[n]  = cs_A1[n] * dysum[n]          with dysum = column sums of dy_A1
 * which is the gradient of  y = resid + rs*cs*(xW^T+b)  w.r.t. W, cs, b when dy = rs*dL/dy.
 * w32 (f32 master weights) and bias are only read when cs != NULL.                            */
/* octic_linear_d8_wgrad_has_colsum: 1 if the wgrad launch for this shape also leaves the column sums of the invariant
 * irrep's dY (the bias gradient) in the workspace; _finish then takes them when called with dysum == NULL and
 * octic_colsum_a1 is not needed.                                                                       */
int octic_linear_d8_wgrad_has_colsum(int cin, int cout, int dtype);
/* Host-only query: what octic_linear_d8_wgrad runs for this problem (wgrad_plan, csrc/wgrad.hip).  out[0] = kernel
 * (OCTIC_WGRAD_*), out[1] = tile width (32 TT; 160 on every ring shape), out[2] = the `splits` to pass, out[3] = 1 when the
 * launch leaves the A1 column sums in the workspace.  _has_colsum, _splits and _tile below are its single answers. */
enum {
  OCTIC_WGRAD_RING = 0,      /* wgrad_ring_kernel: bf16, cin and cout multiples of 160 */
  OCTIC_WGRAD_TILED = 1      /* wgrad_kernel<TIN, TT>                                  */
};
int octic_linear_d8_wgrad_plan(int64_t M, int cin, int cout, int dtype, int out[4]);
int64_t octic_linear_d8_wgrad_workspace_bytes(int cin, int cout, int splits);
int octic_linear_d8_wgrad_splits(int64_t M, int cin, int cout);
int octic_linear_d8_wgrad_tile(int64_t M, int cin, int cout);   /* tile width 32*TT of wgrad_kernel<TIN, TT> */
int octic_linear_d8_wgrad(const octic_view* x, const octic_view* dy, int64_t M, int cin, int cout, int dtype,
                          float* workspace, int splits, void* stream);
/* octic_linear_d8_wgrad under the stochastic-depth mask of the branch: sample_scale = one f32 factor per sample of
 * rows_per_sample token rows (M % rows_per_sample == 0, else OCTIC_ESHAPE; a pointer off 4 bytes: OCTIC_EALIGN), or NULL.
 * sample_scale[b] == 0 PROMISES that every dy row of sample b is zero.  A bf16 launch on the ring kernel whose groups have at
 * most 4096 steps of 32 rows then reads only the LIVE steps - those with a token row of a kept sample - and deals them evenly:
 * of a group's L live steps, split s of S sums those of rank [L s / S, L (s + 1) / S) in ascending order; a split left
 * without steps stores zeros.  Plan, workspace, `splits` and grid are those of the plain entry; the f32 slab sums are grouped
 * differently, so the gradients agree with the plain entry's as two summation orders of the same f32 terms do (bit for bit
 * where those sums are exact).  Without the promise the dropped rows are simply left out.  NULL, f32 operands, the tiled
 * kernel and longer groups launch exactly what octic_linear_d8_wgrad launches, which forwards NULL.                    */
int octic_linear_d8_wgrad_skip(const octic_view* x, const octic_view* dy, int64_t M, int cin, int cout, int dtype,
                               float* workspace, int splits, const float* sample_scale, int rows_per_sample, void* stream);
/* Host-only query: the steps a masked launch walks, through the kernel's own liveness and share rules.  sample_scale is a HOST
 * array here.  Writes (group in launch order: E first, then A1 A2 B1 B2; split; step) for every step walked, groups and
 * splits ascending and the steps of a split in the order it takes them, `cap` entries at most.  Returns their number, or
 * OCTIC_ESHAPE for a launch that would run unmasked (f32, the tiled kernel, more than 4096 steps) or a cap too small. */
int octic_linear_d8_wgrad_order_dropped(int64_t M, int cin, int cout, int dtype, int splits, const float* sample_scale,
                                        int rows_per_sample, int cap, int* out_group, int* out_split, int* out_step);
int octic_linear_d8_wgrad_finish(const float* workspace, int splits, int cin, int cout,
                                 const float* const w32[5], const float* const cs[5], const float* bias,
                                 const float* dysum, float* const dw[5], float* const dcs[5], float* dbias,
                                 void* stream);
/* njobs of the finishes above in ceil(njobs / 8) launches, bit-identical to njobs calls (see octic_dense_finish_batch);
 * has_cs = 0 stands for cs == NULL (w32, cs, dcs ignored).                                                          */
typedef struct octic_wgrad_finish_job {
  const float* workspace;
  const float* w32[5];
  const float* cs[5];
  const float* bias;
  const float* dysum;
  float* dw[5];
  float* dcs[5];
  float* dbias;
  int splits, cin, cout, has_cs;
} octic_wgrad_finish_job;
int octic_linear_d8_wgrad_finish_batch(const octic_wgrad_finish_job* jobs, int njobs, void* stream);

/* Column sums of the A1 block of dy (bias gradient, bias exists on A1 only: d8_layers.py:117-122).
 * out[n] = sum_m dy_A1[m,n]; `partials` holds octic_colsum_blocks(M) * c floats.               */
int octic_colsum_blocks(int64_t M);
int octic_colsum_a1(const octic_view* dy, int64_t M, int c, int dtype, float* partials, float* out, void* stream);

/* y = rs[token/rows_per_sample] * x, converted f32 -> out_dtype (cotangent entering a fused
 * residual branch: dL/d(branch) = drop-path mask * dL/dx_out).  rs may be NULL (pure cast).     */
int octic_cast_rowscale(const octic_view* x, const octic_view* y, const float* rs, int64_t rows_per_sample,
                        int64_t M, int c, int out_dtype, void* stream);

/* ---- attention head packing (d8_layers.py:631-643, 650-656) ------------------------------------
 * pack:  qkv view (3*8c channels: per irrep [q|k|v] thirds) -> q,k,v  [B,H,T,8w], w = c/H, per-head
 *        vector [A1 w|A2 w|B1 w|B2 w|E_row0 2w|E_row1 2w].  qkv_out = 3 consecutive [B,H,T,8w] arrays.
 * unpack: o [B,H,T,8w] -> view with 8c channels.  Each is the other's adjoint (n_s = 3 / 1).
 * heads[s] (s < n_s) are n_s separately allocated [B,H,T,8w] arrays (q, k, v — or their gradients, which
 * autograd hands back as three unrelated tensors).                                              */
int octic_attn_pack_heads(const octic_view* qkv, void* const heads[3], int64_t B, int64_t T, int H, int c, int n_s,
                          int dtype, void* stream);
int octic_attn_unpack_heads(void* const heads[3], const octic_view* y, int64_t B, int64_t T, int H, int c, int n_s,
                            int dtype, void* stream);

/* ---- attention core (bf16) ---------------------------------------------------------------------
 * o = softmax(scale * q k^T) v per (batch, head); replaces F.scaled_dot_product_attention in AttentionD8
 * (d8_layers.py:645-648) and the standard blocks (deit/vit.py:41-45).  Element (b,h,t,d) of q/k/v is at
 * base + b*sB + h*sH + t*sT + d (one stride set for the three, so [B,H,T,hd] and the [B,T,3,H,hd] views of a
 * fused qkv tensor both work); o likewise with oB/oH/oT.  lse ([B,H,T] f32, may be NULL) receives the
 * log2-domain log-sum-exp needed by the backward.  T <= 16384, hd a multiple of 16 (<= 128); otherwise
 * OCTIC_ESHAPE (callers keep torch SDPA for such shapes).  T <= 320 keeps K and V of a head resident in LDS; longer
 * sequences (and every T under OCTIC_ROUTE_ATTN_STREAM = 1) stream them through LDS in blocks.       */
int octic_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int H, int T, int hd,
                   int64_t sB, int64_t sH, int64_t sT, int64_t oB, int64_t oH, int64_t oT, float scale, void* stream);

/* Backward of octic_attn_fwd (P recomputed from q, k and lse; nothing T x T is stored).  o / dout share the stride
 * set (oB,oH,oT); dq/dk/dv share (gB,gH,gT).  delta: [B,H,T] f32 (row sums of dout*o).  phase bit 0: query-owned
 * kernel (writes delta and dq); bit 1: key-owned kernel (reads delta, writes dk and dv); 3 = both, in that order. */
int octic_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   float* delta, void* dq, void* dk, void* dv, int64_t B, int H, int T, int hd, int64_t sB, int64_t sH,
                   int64_t sT, int64_t oB, int64_t oH, int64_t oT, int64_t gB, int64_t gH, int64_t gT, float scale,
                   int phase, void* stream);

/* ---- attention core (float32) ------------------------------------------------------------------
 * octic_attn_fwd / octic_attn_bwd on float32 operands (q, k, v, o, dout, dq, dk, dv all f32; every stride in f32
 * elements, rows 16-byte aligned = strides multiples of 4).  Same argument lists, stride sets, lse / delta / phase
 * meaning and rejections (OCTIC_ENULL, OCTIC_ESHAPE for T outside 1..16384, hd % 16 != 0, hd > 128, non-positive
 * B / H; OCTIC_EALIGN), all before any launch; scale must be positive and finite (the masking and the running maximum
 * work on scaled scores): anything else is OCTIC_ESHAPE too.  Arithmetic contract:
 *  - every product is a chain of v_mfma_f32_16x16x4_f32 = a k-ordered f32 fmaf chain, one rounding per product, no
 *    reduced precision; scores sum over the head vector in the order d = g hd/4 + s (g = 0..3 the MFMA k index, s the
 *    step), P V and the gradient products over the rows of a 32-row block in the order 4 g + reg, blocks in
 *    ascending order;
 *  - online softmax in the exp2 domain: p = exp2(fl(x scale log2(e)) - m) - the product is rounded before the subtraction,
 *    no fma, so the exponent of a row's own maximum is exactly 0 - with the running row max m updated once per 32-key
 *    block, f32 statistics, row sums reduced over the four lanes of a row in a fixed order; lse = m + log2(l); the
 *    backward recomputes p = exp2(fl(x scale log2(e)) - lse) and uses delta = rowsum(dout * o), summed as the diagonal
 *    of an MFMA product in the order of the dP entries it is subtracted from;
 *  - keys beyond T in the last block are masked (-inf forward, p = 0 backward), rows beyond T are staged as zeros, no
 *    address beyond row T - 1 of any operand is read;
 *  - every output element is written once, no atomics: results are bitwise repeatable and independent of the strides.
 * One streaming design for every T: 128 own rows per workgroup, 32 streamed rows per LDS block (csrc/attn_f32.hip). */
int octic_attn_fwd_f32(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int H, int T, int hd,
                       int64_t sB, int64_t sH, int64_t sT, int64_t oB, int64_t oH, int64_t oT, float scale, void* stream);
int octic_attn_bwd_f32(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       float* delta, void* dq, void* dk, void* dv, int64_t B, int H, int T, int hd, int64_t sB, int64_t sH,
                       int64_t sT, int64_t oB, int64_t oH, int64_t oT, int64_t gB, int64_t gH, int64_t gT, float scale,
                       int phase, void* stream);

/* AttentionD8 straight on packed rows - reference octic_vits/d8_layers.py:631-656 (head split of the five-irrep
 * projection output, F.scaled_dot_product_attention, re-assembly of the irreps) WITHOUT the pack / unpack copies:
 * qkv = LinearD8 output [B, T, 3*8c] (row stride ld_qkv elements), o = packed [B, T, 8c] input of the output
 * projection.  c / H must be 10 (head_dim 80) or 8 (head_dim 64), bf16, T <= 16384.  lse [B,H,T] as in octic_attn_fwd. */
int octic_attn_fwd_packed(const void* qkv, void* o, float* lse, int64_t B, int H, int T, int c, int64_t ld_qkv,
                          int64_t ld_o, float scale, void* stream);
/* Backward of octic_attn_fwd_packed (autograd of d8_layers.py:631-656): dqkv packed like qkv (row stride ld_g)
 * receives dq | dk | dv, dout packed like o; phase as in octic_attn_bwd. */
int octic_attn_bwd_packed(const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                          int64_t B, int H, int T, int c, int64_t ld_qkv, int64_t ld_o, int64_t ld_g, float scale,
                          int phase, void* stream);

/* What the attention entry points run for a shape, without touching the GPU: the answer of the one routing function of
 * the library (attn_plan, csrc/attention.hip), under the current octic_route_override table.  dtype: OCTIC_BF16 | OCTIC_F32;
 * ld_in / ld_out / ld_grad: token strides in elements of q/k/v, of o/dout and of dq/dk/dv (the sT / oT / gT of the entry
 * points, ld_qkv / ld_o / ld_g of the packed ones; 0 = hd, contiguous heads).  out[0] = forward kernel (OCTIC_ATTN_FWD_*),
 * out[1] = its waves per workgroup, out[2] = what a backward call with phase 3 runs (OCTIC_ATTN_BWD_*), out[3] = its waves.
 * OCTIC_ESHAPE exactly where the entry points return it for (T, hd). */
enum {
  OCTIC_ATTN_FWD_PERSIST = 0,      /* attn_fwd_persist_kernel: one workgroup per CU walks over its heads                   */
  OCTIC_ATTN_FWD_A80_ONESHOT = 1,  /* csrc/attn80.hip, head_dim 80: fwd_os_kernel / fwd_oss_kernel<n>, one-shot softmax     */
  OCTIC_ATTN_FWD_A80_ONLINE = 2,   /* csrc/attn80.hip, head_dim 80: fwd_kernel, online softmax                              */
  OCTIC_ATTN_FWD_RESIDENT = 3,     /* attn_fwd_kernel<.., 512 | 640>: one workgroup per head, one wave per query tile       */
  OCTIC_ATTN_FWD_STREAM = 4,       /* csrc/attn_stream.hip: K / V through LDS in blocks                                     */
  OCTIC_ATTN_FWD_F32 = 5           /* csrc/attn_f32.hip                                                                     */
};
enum {
  OCTIC_ATTN_BWD_SINGLE = 0,       /* csrc/attn80_bwd.hip: dq, dk, dv from one recomputation of P                           */
  OCTIC_ATTN_BWD_PAIR = 1,         /* attn_bwd_dq_kernel + attn_bwd_dkv_kernel, K / V (Q / dO) of a head resident in LDS    */
  OCTIC_ATTN_BWD_STREAM = 2,       /* the streaming dq + dkv pair                                                           */
  OCTIC_ATTN_BWD_F32 = 3           /* the float32 dq + dkv pair                                                             */
};
int octic_attn_plan(int dtype, int T, int hd, int64_t ld_in, int64_t ld_out, int64_t ld_grad, int out[4]);
/* The same query for stochastic depth: which of the planned kernels SKIP a sample whose sample_scale is 0 - read none of its
 * operands (q, k, v, and o, dout in the backward) and store +0 - as opposed to computing it, which the contract of the *_skip
 * entry points also allows.  A caller that leaves operand rows of a dropped sample unwritten needs the former.  out[0] = the
 * largest batch B at which the forward skips (0: it never does; fwd_os_kernel alone, up to its 512-sample order table),
 * out[1] = 1 when a backward call with phase 3 skips, out[2] = 1 when the phase-1 + phase-2 pair skips, out[3] = 0.          */
int octic_attn_skip_plan(int dtype, int T, int hd, int64_t ld_in, int64_t ld_out, int64_t ld_grad, int out[4]);

/* ---- attention core: samples dropped by stochastic depth ------------------------------------------
 * The four bf16 entry points with one more argument in front of `stream`: sample_scale, nullable, B floats on the
 * device - the per-sample factor the CALLER multiplies this attention branch's output with (x + scale * f(x)); exactly
 * 0.0f for a sample whose branch is dropped.  The existing entry points are these with sample_scale = NULL.
 * Contract: for a sample with sample_scale[b] == 0 a kernel MAY skip the sample.  If it does, it writes +0 to every
 * element of that sample's o rows and lse (forward), of its dq, dk, dv rows and delta (backward), and reads none of the
 * sample's operands.  The caller guarantees that the branch output is multiplied by the same factor, so the skipped o never
 * reaches the result and dout is zero for those samples (dq = dk = dv = 0 is then what the full computation gives).  A
 * kernel that does not skip computes the sample as without the argument.  NULL, or factors that are all non-zero, give
 * the results of the plain entry points bit for bit.  Which kernels skip: the persistent one-shot
 * forward at 257 / 258 tokens, head_dim 80 (up to 512 samples per launch), and the single-pass backward for head_dim 80
 * (257, 193 .. 256 and <= 64 tokens); every other route ignores the argument.  sample_scale must be 4-byte aligned
 * (OCTIC_EALIGN); all other rejections as in the plain entry points.                                                    */
int octic_attn_fwd_skip(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int H, int T, int hd,
                        int64_t sB, int64_t sH, int64_t sT, int64_t oB, int64_t oH, int64_t oT, float scale,
                        const float* sample_scale, void* stream);
int octic_attn_bwd_skip(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                        float* delta, void* dq, void* dk, void* dv, int64_t B, int H, int T, int hd, int64_t sB, int64_t sH,
                        int64_t sT, int64_t oB, int64_t oH, int64_t oT, int64_t gB, int64_t gH, int64_t gT, float scale,
                        int phase, const float* sample_scale, void* stream);
int octic_attn_fwd_packed_skip(const void* qkv, void* o, float* lse, int64_t B, int H, int T, int c, int64_t ld_qkv,
                               int64_t ld_o, float scale, const float* sample_scale, void* stream);
int octic_attn_bwd_packed_skip(const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                               int64_t B, int H, int T, int c, int64_t ld_qkv, int64_t ld_o, int64_t ld_g, float scale,
                               int phase, const float* sample_scale, void* stream);

/* ---- octic -> standard hand-off (model.py:196-200) ---------------------------------------------
 * hybrid:    dense[m, :] = cat(A1,A2,B1,B2, E[0,:c], E[1,:c], E[0,c:], E[1,c:])   (8-tuple order,
 *            d8_utils.py:370-385; the following standard blocks' weights depend on it)
 * invariant: dense[m, :] = cat(A1,|A2|,|B1|,|B2|, sqrt(E[0]^2+E[1]^2))  [6c]  (PowerSpectrumInvariant,
 *            d8_invariantization.py:49-64)
 * x is f32 (residual stream); dense is out_dtype.  The *_bwd forms take dense f32 gradients.    */
int octic_handoff_cat_fwd(const octic_view* x, void* dense, int64_t M, int c, int out_dtype, void* stream);
int octic_handoff_cat_bwd(const float* ddense, const octic_view* dx, int64_t M, int c, void* stream);
int octic_power_spectrum_fwd(const octic_view* x, void* dense, int64_t M, int c, int out_dtype, void* stream);
int octic_power_spectrum_bwd(const float* ddense, const octic_view* x, const octic_view* dx, int64_t M, int c,
                             void* stream);

/* ---- lift patch embedding (d8_layers.py:284-486, model.py:172-181) -----------------------------
 * im2col: img [B,Cin,Himg,Wimg] f32 -> patches [B*G*G, Kpad] `dtype`, column = (ch, py, px), zero
 * padded to Kpad (a multiple of 8 >= Cin*p*p).  The conv with stride = kernel is then one GEMM
 * against the symmetry-expanded weights; use octic_lift_gemm: out_packed[b, tok0 + n, :] =
 * patches[b*G*G + n, :] W^T + bias + pos[n, :]  with W:[8c, Kpad] rows in packed channel order and
 * pos:[G*G, 8c] f32 (unfolded positional embedding, may be NULL); rows [0,tok0) of every sample
 * are left untouched (cls token).  out is f32 [B, tok0+G*G, 8c].                               */
int octic_im2col_patches(const float* img, void* patches, int64_t B, int Cin, int Himg, int Wimg, int p,
                         int Kpad, int dtype, void* stream);
int octic_lift_gemm(const void* patches, const void* w, const float* bias, const float* pos, float* out,
                    int64_t B, int64_t n_patches, int tok0, int Kpad, int D, int dtype, void* stream);
/* dW[n,k] = sum_rows dout[row, n] patches[row, k]  with dout the [rows, D] cotangent of the patch
 * tokens in `dtype` (cls rows removed by the caller); f32 result, split-row slabs like wgrad.
 * (bias here is a full [D] vector, zero outside the A1 block.)                                   */
int64_t octic_lift_wgrad_workspace_bytes(int Kpad, int D, int splits);
int octic_lift_wgrad(const void* patches, const void* dout, float* dw, float* workspace, int splits, int64_t rows,
                     int Kpad, int D, int dtype, void* stream);

/* ---- fused multi-tensor LAMB + EMA ----------------------------------------------------------------
 * One optimizer step of the reference recipe (apex FusedLAMB via timm create_optimizer 'fusedlamb',
 * experiments/train_deit.py:42; timm ModelEma, deit/main.py:344-351) over ALL tensors in five launches:
 * global grad-norm clip to max_grad_norm, Adam moments with bias correction, + wd*p, per-tensor trust ratio
 * |p|/|u| (only where wd != 0), p -= lr*ratio*u, ema += (1-decay)(p-ema).  The gradient buffers are
 * overwritten (they hold the update between the two passes).  Tables are device arrays: per-tensor
 * pointers p,g,m,v,ema (ema may be NULL), per-tensor weight decay, and a chunk list
 * (tensor id, element offset, length) with tensor_chunk_begin[ntensors+1] giving each tensor's chunk
 * range.  workspace: octic_lamb_workspace_floats() f32, zero-initialised by the caller once; after the call
 * workspace[1] = global grad norm (the number deit/engine.py:84 logs), workspace[2] = 1 if the step was SKIPPED
 * because that norm is not finite (parameters, moments, EMA and bf16 copies untouched: the reference exits
 * before optimizer.step() on a non-finite loss, deit/engine.py:67-71), workspace[3] = applied steps,
 * workspace[6] = skipped steps so far.  step > 0: the bias-correction step t given by the host; step == 0: t is
 * the device-side counter workspace[3] (+1 per applied step), so a hipGraph capture of the call replays
 * correctly.  bf16_shadow (may be NULL; entries may be NULL): per-tensor bf16
 * buffers that receive a rounded copy of the updated parameter in the same pass - the compute-dtype weights
 * torch.autocast would otherwise re-cast at every use.                                              */
int64_t octic_lamb_workspace_floats(int ntensors, int nchunks);
int octic_lamb_step(void* const* p, void* const* g, void* const* m, void* const* v, void* const* ema, const float* wd,
                    const int* chunk_tensor, const int64_t* chunk_off, const int* chunk_len,
                    const int* tensor_chunk_begin, int ntensors, int nchunks, float* workspace, float lr, float beta1,
                    float beta2, float eps, float max_grad_norm, int step, float ema_decay, void* const* bf16_shadow,
                    void* stream);
/* The same fused step WITHOUT the layer-wise trust ratio: AdamW with decoupled weight decay, p -= lr (mhat / (sqrt(vhat) +
 * eps) + wd p) - torch.optim.AdamW as the DINOv2 recipe builds it (dinov2/train/train.py:60-61), with clip_grad_norm_ of the
 * tensors of this call to max_grad_norm (train.py:274-279: one call per sub-model) and the teacher's EMA (`ema` = the
 * teacher's parameters, ema_decay = the momentum of the step: ssl_meta_arch.py:356-367) in the same two passes.           */
int octic_adamw_step(void* const* p, void* const* g, void* const* m, void* const* v, void* const* ema, const float* wd,
                     const int* chunk_tensor, const int64_t* chunk_off, const int* chunk_len,
                     const int* tensor_chunk_begin, int ntensors, int nchunks, float* workspace, float lr, float beta1,
                     float beta2, float eps, float max_grad_norm, int step, float ema_decay, void* const* bf16_shadow,
                     void* stream);
/* The same two steps with the schedule-driven hyper-parameters read from DEVICE memory (same kernels, same arithmetic):
 * lr = [ntensors] f32, the absolute learning rate of each tensor (read once per chunk, like wd); ema_decay = ONE f32 (may
 * be NULL when ema is NULL), the EMA weight 1 - decay is formed on the device in f32.  A hipGraph that captured the call
 * follows whatever the host copies into those buffers between replays (timm / DINOv2 schedules, layer-wise lr decay).
 * With every lr[i] = x and *ema_decay = d the results equal octic_lamb_step / octic_adamw_step(lr = x, ema_decay = d)
 * bit for bit.                                                                                                           */
int octic_lamb_step_hp(void* const* p, void* const* g, void* const* m, void* const* v, void* const* ema, const float* wd,
                       const int* chunk_tensor, const int64_t* chunk_off, const int* chunk_len,
                       const int* tensor_chunk_begin, int ntensors, int nchunks, float* workspace, const float* lr,
                       float beta1, float beta2, float eps, float max_grad_norm, int step, const float* ema_decay,
                       void* const* bf16_shadow, void* stream);
int octic_adamw_step_hp(void* const* p, void* const* g, void* const* m, void* const* v, void* const* ema, const float* wd,
                        const int* chunk_tensor, const int64_t* chunk_off, const int* chunk_len,
                        const int* tensor_chunk_begin, int ntensors, int nchunks, float* workspace, const float* lr,
                        float beta1, float beta2, float eps, float max_grad_norm, int step, const float* ema_decay,
                        void* const* bf16_shadow, void* stream);

/* ---- standard (non-equivariant) half of the hybrid: row kernels around the library GEMMs ----------------
 * The reference's standard blocks (deit/models_v2.py Layer_scale_init_Block, used for the second half of the
 * depth by octic_vits/model.py:130-150) are  x = x + drop_path(gamma * f(LayerNorm(x))).  The four projections
 * stay on the BLAS library; these entry points replace the eager chain around them.  Rows are dense
 * [rows, d] with d % 4 == 0, d <= 2048; x / residual stream / statistics are f32, branch tensors `dtype`.
 *
 * octic_dense_layernorm_fwd: y = (x-mean)*rstd*w + b (w, b may be NULL), stats[rows,2] = (mean, rstd).
 * octic_dense_layernorm_bwd: dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) + dres with g = gy*w (dres = cotangent
 *   of the residual path, may be NULL); partials (may be NULL) receives octic_dense_blocks(rows) slabs [2][d]
 *   holding sum gy*xhat and sum gy; octic_dense_finish reduces them into dw / db.
 * octic_scale_residual_fwd: out = x + rs[row / rows_per_scale] * gamma[col] * y  (rs, gamma may be NULL).
 * octic_scale_residual_bwd: gy = rs*gamma*gout in y's dtype; slabs [2][d] of sum rs*gout*y (= d gamma) and
 *   sum rs*gout (times gamma = bias gradient of the projection that produced y).
 * octic_dense_finish: out0[j] = sum_b slab[b][0][j];  out1[j] = scale1[j] * sum_b slab[b][1][j]
 *   (out0, out1, scale1 may each be NULL).                                                              */
int octic_dense_blocks(int64_t rows);
/* octic_dense_resid_layernorm_fwd: xout = x + rs[row / rows_per_scale] * gamma * yb (the tail of one branch of
 * Layer_scale_init_Block, deit/vit.py:131-134) and y = LayerNorm(xout) (the norm that opens the next branch,
 * deit/vit.py:132-133) in one row pass; stats[rows,2] = (mean, rstd) of xout.  Same arithmetic as
 * octic_scale_residual_fwd followed by octic_dense_layernorm_fwd.                                            */
int octic_dense_resid_layernorm_fwd(const float* x, const void* yb, int yb_dtype, const float* gamma, const float* rs,
                                    int64_t rows_per_scale, float* xout, void* y, int y_dtype, const float* w,
                                    const float* b, float* stats, int64_t rows, int d, float eps, void* stream);
/* octic_dense_resid_layernorm_fwd_skip: the same call (rs required: NULL is OCTIC_ENULL) that leaves the rows of yb unread
 * where rs[row / rows_per_scale] == 0: zeros stand in, xout = x + 0.  xout, y and stats are written for every row.  With yb
 * finite every output equals the plain call, up to the sign of an exact zero.                                          */
int octic_dense_resid_layernorm_fwd_skip(const float* x, const void* yb, int yb_dtype, const float* gamma, const float* rs,
                                         int64_t rows_per_scale, float* xout, void* y, int y_dtype, const float* w,
                                         const float* b, float* stats, int64_t rows, int d, float eps, void* stream);
int octic_dense_layernorm_fwd(const float* x, void* y, int y_dtype, const float* w, const float* b, float* stats,
                              int64_t rows, int d, float eps, void* stream);
int octic_dense_layernorm_bwd(const void* gy, int g_dtype, const float* x, const float* w, const float* stats,
                              const float* dres, float* dx, float* partials, int64_t rows, int d, void* stream);
int octic_dense_finish(const float* partials, int nblocks, int d, float* out0, float* out1, const float* scale1,
                       void* stream);
/* octic_dense_finish_batch: njobs reductions of the kind above in ceil(njobs / 64) launches, bit-identical to njobs calls of
 * octic_dense_finish (same summation order).  For callers that can postpone the parameter-gradient reductions of a backward
 * pass to its end (nothing reads them before the optimizer): 96 five-microsecond launches per ViT-H step become two.       */
typedef struct octic_finish_job {
  const float* partials; /* [nblocks][2][d] slabs */
  float* out0;           /* [d] or NULL */
  float* out1;           /* [d] or NULL */
  const float* scale1;   /* [d] or NULL */
  int nblocks;
  int d;
} octic_finish_job;
int octic_dense_finish_batch(const octic_finish_job* jobs, int njobs, void* stream);
/* octic_dense_layernorm_bwd_tail: octic_dense_layernorm_bwd (bf16 gy) followed by octic_scale_residual_bwd on its result,
 * one row pass for d = 256, 512, ... 1280 (other d: OCTIC_ESHAPE, call the two): dx as above; gyb = rs*gamma*dx in bf16
 * (cotangent of the bf16 branch output yb whose residual add produced the normalised stream); partials / partials2:
 * octic_dense_blocks(rows) slabs [2][d] each, as the two kernels leave them (both may be NULL).  The autograd of
 * `x = x + drop_path(gamma * f(norm(x)))` chained over two branches (deit/vit.py:131-134).                       */
int octic_dense_layernorm_bwd_tail(const void* gy, const float* x, const float* w, const float* stats, const float* dres,
                                   float* dx, float* partials, const void* yb, const float* gamma, const float* rs,
                                   int64_t rows_per_scale, void* gyb, float* partials2, int64_t rows, int d, void* stream);
/* octic_dense_layernorm_bwd_tail_skip: the same with the stochastic-depth factor of the branch this norm OPENS as a sample
 * mask (sample_scale: one f32 per rows_per_sample rows, NULL = the call above; rows_per_sample <= 0 or rows %
 * rows_per_sample != 0 with a mask: OCTIC_ESHAPE).  sample_scale[b] == 0 PROMISES that the rows of gy of sample b are zero -
 * the branch's first GEMM stores exact zeros for a dropped sample - and the kernel may then leave those rows of gy, x and
 * stats unread: dx = dres (zeros without dres), nothing added to `partials`.  Under a mask the rows with rs == 0 (the factor
 * of the branch that ENDS here) leave yb unread as well; their zero gyb rows are still stored.  With the promise kept and x
 * finite every output equals the unmasked call, up to the sign of an exact zero (which no comparison of values sees). */
int octic_dense_layernorm_bwd_tail_skip(const void* gy, const float* x, const float* w, const float* stats,
                                        const float* dres, float* dx, float* partials, const void* yb, const float* gamma,
                                        const float* rs, int64_t rows_per_scale, void* gyb, float* partials2, int64_t rows,
                                        int d, const float* sample_scale, int64_t rows_per_sample, void* stream);
/* octic_dense_layernorm_bwd_tail_inplace: octic_dense_layernorm_bwd_tail_skip where dres and dx are ONE buffer (`dx`: on
 * entry the residual cotangent, on return the stream cotangent).  sample_scale is required (NULL: OCTIC_ENULL).  Which rows
 * of `dx` are touched:
 *   sample_scale != 0 (live row):            read, then written with LN'(gy) + dres by the lane that read each address;
 *   sample_scale == 0, rs != 0 (or rs NULL): read only (dx = dres is what the buffer holds; gyb = rs * gamma * dres);
 *   sample_scale == 0, rs == 0:              neither read nor written; gyb is an exact zero row, yb stays unread.
 * The promise of sample_scale is that of the _skip call.  gyb is written for every row; slabs and the order of every sum
 * are those of octic_dense_layernorm_bwd_tail_skip, and so is every value, up to the sign of an exact zero.             */
int octic_dense_layernorm_bwd_tail_inplace(const void* gy, const float* x, const float* w, const float* stats, float* dx,
                                           float* partials, const void* yb, const float* gamma, const float* rs,
                                           int64_t rows_per_scale, void* gyb, float* partials2, int64_t rows, int d,
                                           const float* sample_scale, int64_t rows_per_sample, void* stream);
/* octic_dense_gelu_bwd: dh = gelu'(h) * g (exact erf GELU, bf16 [rows, d], d % 8 == 0) and, when partials != NULL,
 * octic_dense_gelu_blocks() slabs [d] of column sums of dh (bias gradient of the projection that produced h;
 * reduce with octic_dense_finish(partials, blocks, d/2, out, out + d/2, NULL)).  Replaces GeluBackward + the
 * bias-gradient reduction of the standard MLP (deit/vit.py Mlp).                                          */
int octic_dense_gelu_blocks(void);
int octic_dense_gelu_bwd(const void* h, const void* g, void* dh, float* partials, int64_t rows, int d, void* stream);
/* octic_dense_colsum: octic_dense_gelu_blocks() slabs [d] of f32 column sums of a bf16 [rows, d] tensor (row stride ld
 * elements, d % 8 == 0), in a fixed order; reduce with octic_dense_finish as above.  The bias gradient of the fused-qkv
 * projection (autograd of deit/vit.py:33: grad.sum(0) over the token rows).                                      */
int octic_dense_colsum(const void* g, int64_t rows, int d, int64_t ld, float* partials, void* stream);
/* octic_dense_colsum_skip: sample_scale[b] == 0 (one f32 per rows_per_sample rows; NULL = the call above; rows_per_sample
 * <= 0 or rows % rows_per_sample != 0 with a mask: OCTIC_ESHAPE) promises that the rows of sample b are zero; they are not
 * read and zeros take their place in the same sums.                                                                  */
int octic_dense_colsum_skip(const void* g, int64_t rows, int d, int64_t ld, float* partials, const float* sample_scale,
                            int64_t rows_per_sample, void* stream);
/* The gate of DINOv2's SwiGLU FFN (dinov2/layers/swiglu_ffn.py:29-33: x1, x2 = w12(x).chunk(2, -1); silu(x1) * x2), bf16 with
 * f32 arithmetic.  x12: [rows, 2H], row stride ld12 elements - columns [0, H) the gate x1, [H, 2H) the value x2.
 * octic_swiglu_fwd: a[r, j] = bf16(silu(x12[r, j]) * x12[r, H + j]), j < H; a: [rows, H], row stride lda.
 * octic_swiglu_bwd: with s = sigmoid(x1) and ga [rows, H] (row stride ldg) the cotangent of a,
 *   dx12[r, j] = bf16(ga * x2 * s * (1 + x1 * (1 - s))),  dx12[r, H + j] = bf16(ga * x1 * s)   (dx12: row stride ldd)
 *   and, when partials != NULL, octic_swiglu_blocks() slabs [2H] of f32 column sums of the STORED bf16 dx12 (what the GEMMs
 *   downstream see), in a fixed order: reduce with octic_dense_finish(partials, blocks, H, db, db + H, NULL) - the bias
 *   gradient of w12, in w12.bias order.
 * Refused before any launch: H <= 0, H % 8 != 0 or a row stride shorter than its row (OCTIC_ESHAPE); a row stride that is
 * no multiple of 8 or a base pointer off 16 bytes (OCTIC_EALIGN); a NULL operand (OCTIC_ENULL).  rows == 0: OCTIC_OK, no
 * launch.  sigmoid is 1 / (1 + exp(-x)): finite inputs anywhere in bf16's range give finite or correctly infinite results,
 * never NaN; for x1 >= 17 it is exactly 1, so a == bf16(x1 * x2), dx1 == bf16(ga * x2), dx2 == bf16(ga * x1) bit for bit. */
int octic_swiglu_blocks(void);
int octic_swiglu_fwd(const void* x12, int64_t ld12, void* a, int64_t lda, int64_t rows, int H, void* stream);
int octic_swiglu_bwd(const void* x12, int64_t ld12, const void* ga, int64_t ldg, void* dx12, int64_t ldd, float* partials,
                     int64_t rows, int H, void* stream);
int octic_scale_residual_fwd(const float* x, const void* y, int y_dtype, const float* gamma, const float* rs,
                             int64_t rows_per_scale, float* out, int64_t rows, int d, void* stream);
int octic_scale_residual_bwd(const float* gout, const void* y, int y_dtype, const float* gamma, const float* rs,
                             int64_t rows_per_scale, void* gy, float* partials, int64_t rows, int d, void* stream);

/* The same four row kernels with a ROW MAP (int32 [rows]): the compact rows 0..rows-1 of a branch correspond to rows
 * rowmap[r] of a larger f32 tensor - the residual stream (or its cotangent) of which the branch sees only the kept samples:
 * DINOv2's batch-subset stochastic depth (dinov2/layers/block.py:113-140: x[brange] in, index_add back) without the gather
 * and scatter passes.  _fwd_rows reads x[rowmap[r]] (and, xcopy != NULL, leaves the rows as read in a compact copy: what the
 * backward needs once the stream has been edited in place); scale_residual_fwd_rows writes out[rowmap[r]] = x[r] + rs gamma
 * y[r]; scale_residual_bwd_rows reads gout[rowmap[r]]; layernorm_bwd_rows reads dres[rowmap[r]] and writes dx[rowmap[r]]
 * (dres == dx edits the stream's cotangent in place).  rowmap == NULL: the plain kernels.  Rows of a map must be distinct. */
int octic_dense_layernorm_fwd_rows(const float* x, void* y, int y_dtype, const float* w, const float* b, float* stats,
                                   int64_t rows, int d, float eps, const int* rowmap, float* xcopy, void* stream);
int octic_dense_layernorm_bwd_rows(const void* gy, int g_dtype, const float* x, const float* w, const float* stats,
                                   const float* dres, float* dx, float* partials, int64_t rows, int d, const int* rowmap,
                                   void* stream);
int octic_scale_residual_fwd_rows(const float* x, const void* y, int y_dtype, const float* gamma, const float* rs,
                                  int64_t rows_per_scale, float* out, int64_t rows, int d, const int* rowmap, void* stream);
int octic_scale_residual_bwd_rows(const float* gout, const void* y, int y_dtype, const float* gamma, const float* rs,
                                  int64_t rows_per_scale, void* gy, float* partials, int64_t rows, int d, const int* rowmap,
                                  void* stream);

/* bf16 operand copies of nn.Linear weights [N,K] for octic_dense_gemm_nt, all layers in one launch (what autocast's
 * per-use weight casts amount to, deit/engine.py:56): wb = bf16(src) [N,K] (may be NULL) and wt = bf16(src)^T [K,N]
 * (the input-gradient GEMM dX = dY W is then an NT problem too).  src is the f32 master or an existing bf16 copy
 * (src_dtype).  block_begin = running sum of octic_dense_prep_batch_blocks(N, K) over the items.            */
typedef struct octic_dense_prep_item {
  const void* src;
  void* wb;
  void* wt;
  int32_t N, K;
  int32_t block_begin, pad;
} octic_dense_prep_item;
int octic_dense_prep_batch_blocks(int N, int K);
int octic_dense_prep_batch(const octic_dense_prep_item* items_dev, int n_items, int total_blocks, int src_dtype, void* stream);

/* ---- hand-written dense bf16 GEMMs of the standard half -------------------------------------
 * The four projections of the reference's standard block (deit/vit.py:14-56 Attention.qkv / .proj, timm Mlp fc1 / fc2
 * used by Layer_scale_init_Block, deit/vit.py:90-134) and their input gradients are "NT" problems
 *     C[M,N] = A[M,K] . B[N,K]^T          A, B bf16 with K contiguous (lda, ldb = row strides in elements),
 * M token rows, f32 accumulation on v_mfma_f32_16x16x32_bf16.  Taken: K % 64 == 0 with K >= 128 (two K-tiles of 64), N % 8 == 0,
 * lda, ldb, ldc % 8 == 0 (the epilogues move 16 bytes = 8 bf16 of a row of C / C2 / H per lane: a smaller ldc would misalign
 * them), A and B 16-byte aligned, M * lda and N * ldb below 2^30 elements (32-bit buffer offsets); anything else is
 * OCTIC_ESHAPE / OCTIC_EALIGN before any launch.  X / OUT of mode 2 and the colsum slabs are dense (row stride N).
 * `mode` selects the fused tail:
 *   0 PLAIN : C = acc + bias                                   (qkv forward; input gradients: bias = NULL)
 *   1 GELU  : C = acc + bias (pre-activation, kept for backward), C2 = gelu(C) exact erf (fc1 + nn.GELU, vit.py:131-134)
 *   2 RESID : C = acc + bias (branch output, kept for d gamma),  OUT = X + rs[row / rows_per_sample] * gamma * C
 *             = x + drop_path(gamma * f(x)) of deit/vit.py:131-134 with f32 residual stream X / OUT [M,N] dense
 *   3 DGELU : C = gelu'(H) * acc   with H the saved pre-activation (fc2 input gradient fused with GELU backward);
 *             colsum (may be NULL): octic_dense_gemm_colsum_rows(M,N,K) slabs [N] f32 whose sum over slabs is the column
 *             sum of C (= fc1's bias gradient), every element written by each launch, fixed order -> octic_dense_finish
 *   4 GELUF : like 1, but C = gelu'(acc + bias) rounded to bf16 - the factor the backward multiplies by - instead of the
 *             pre-activation itself (gelu and gelu' share one erf evaluation in the epilogue);  C2 = gelu(acc + bias)
 *   5 DFACT : like 3 with H = the factor stored by mode 4: C = H * acc, no transcendental in the epilogue (one more bf16
 *             rounding of the factor than mode 1 + 3; same column sums)
 *   6 GELUO : C = gelu(acc + bias) only (the value mode 1 leaves in C2): passes that never run a backward - inference, the
 *             DINOv2 teacher - write half the bytes
 * C / C2 / H are bf16 [M,N] with row stride ldc.  bias, gamma [N] f32 and rs f32 may be NULL.  workspace:
 * octic_dense_gemm_workspace_bytes(M,N,K) bytes (split-K slabs of the last partial round of tiles + counters), ZEROED once
 * by the caller when it is allocated (the kernels re-arm their counters; calls sharing a workspace must be stream-ordered). */
int64_t octic_dense_gemm_workspace_bytes(int M, int N, int K);
int octic_dense_gemm_colsum_rows(int M, int N, int K);
/* Output tile width the kernel will use for this problem and mode: 256 (256 x 256 tile) or 320 (256 x 320 tile: plain mode,
 * N % 320 == 0, chosen where it makes the launch ONE round of workgroups - the N = 1280 problems of ViT-H).  Informational
 * (profilers see two kernel symbols: dense_nt_kernel<mode, 4> and <0, 5>). */
int octic_dense_gemm_tile(int M, int N, int K, int mode);
int octic_dense_gemm_nt(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int mode, void* C,
                        void* C2, int64_t ldc, const float* bias, const float* gamma, const float* rs,
                        int64_t rows_per_sample, const float* X, float* OUT, const void* H, float* colsum,
                        void* workspace, void* stream);
/* The same GEMM for token rows that are whole images: A / C / C2 / H rows are [B, tokens, .] flattened (M = B * tokens), as every
 * projection of deit/vit.py's blocks sees them (x: [B, N, C], vit.py:31-32).  tokens = 257 (ViT-H/14 at 224 x 224: one class
 * token + 256 patches) lets the launch take per-image row panels - panel b = the 256 patch rows of image b, so M = 64 x 257
 * is 64 full panels instead of 64 + a 64-row last panel whose tiles are split along K - and run the B class-token rows
 * (row stride tokens * lda) as a skinny [B, K] x [K, N] launch of their own, wherever the launch model says that is shorter
 * (all modes but 2; K % 128 == 0).  Same results up to the f32 summation order of the class-token rows (bitwise reproducible
 * from launch to launch).  tokens = 0 (or any other value): exactly octic_dense_gemm_nt.  The column-sum slabs of modes 3 / 5
 * then have octic_dense_gemm_plan()'s out[1] rows.  Workspace: octic_dense_gemm_workspace_bytes covers both plans. */
int octic_dense_gemm_nt_tokens(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int mode, void* C,
                               void* C2, int64_t ldc, const float* bias, const float* gamma, const float* rs,
                               int64_t rows_per_sample, const float* X, float* OUT, const void* H, float* colsum,
                               void* workspace, int tokens, void* stream);
/* What octic_dense_gemm_nt_tokens will do for this problem: out[0] = output tile width (256 | 320), out[1] = rows of the
 * column-sum slabs of modes 3 / 5, out[2] = 1 when the launch uses per-image panels + the class-token kernel, out[3] =
 * workgroups of the main launch. */
int octic_dense_gemm_plan(int M, int N, int K, int mode, int tokens, int* out4);
/* The same launch under a stochastic-depth mask.  sample_scale: [M / rows_per_sample] f32 on the device, may be NULL (then
 * exactly octic_dense_gemm_nt_tokens); it comes with rows_per_sample.  A factor of 0 means the caller and every reader of the
 * output accept, for that sample's rows, EITHER the computed result OR +0 - the choice is per tile.  A row panel all of whose
 * samples have factor 0 is dead: the kernel may leave the rows of A (and of H in modes 3 / 5) that only dead tiles cover unread,
 * stores every output of a dead tile (C, C2; rows below M, columns below N, row stride ldc) as +0 and, in modes 3 / 5, the
 * tile's two column-sum slab rows as +0 - outputs are never left unwritten, so they are finite whatever the buffers held.  A
 * live tile is computed by exactly the code, K range and plan of the unmasked launch (same grid, workspace, tile width, panels
 * and split-K front; octic_dense_gemm_plan_dropped reports it): kept samples' rows are bit for bit those of the unmasked launch.
 * Only which workgroup takes which full tile changes: dead tiles first, then the live ones dealt evenly over the XCDs
 * (octic_dense_gemm_order_dropped is the kernel's own mapping on the host).  Mode 2 and launches of more than 1024 row panels
 * compute every row, which the contract allows.  The class-token launch of per-image panels computes all its rows.
 * rows_per_sample <= 0 or M % rows_per_sample != 0 with a mask: OCTIC_ESHAPE. */
int octic_dense_gemm_nt_tokens_skip(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int mode, void* C,
                                    void* C2, int64_t ldc, const float* bias, const float* gamma, const float* rs,
                                    int64_t rows_per_sample_rs, const float* X, float* OUT, const void* H, float* colsum,
                                    const float* sample_scale, int rows_per_sample, void* workspace, int tokens,
                                    void* stream);
/* octic_dense_gemm_plan for a masked launch (today identical to it; OCTIC_ESHAPE for a bad rows_per_sample). */
int octic_dense_gemm_plan_dropped(int M, int N, int K, int mode, int tokens, int rows_per_sample, int* out4);
/* Host query of the masked launch's item map: sample_scale is a HOST array.  Per workgroup in blockIdx order: out_tm / out_tn
 * the tile (-1 = padding workgroup), out_part its K part, out_split 1 for an item of the split-K front, out_dead 1 for a dead
 * tile (each nullable, `cap` entries).  Returns the number of workgroups, or OCTIC_ESHAPE for a launch the masked kernel does
 * not take (mode 2, more than 1024 panels, bad rows_per_sample) or cap too small. */
int octic_dense_gemm_order_dropped(int M, int N, int K, int mode, int tokens, const float* sample_scale, int rows_per_sample,
                                   int cap, int* out_tm, int* out_tn, int* out_part, int* out_split, int* out_dead);
/* octic_dense_gemm_nt_tokens_skip with the tile width of one kind of launch chosen on the device.  A masked plain-mode launch
 * whose plan is per-image panels on the 320-wide tile, nothing split, ONE round of tiles (ViT-H: the N = 1280 launches at batch
 * 64) lasts as long as one live tile however many panels the mask kills.  Cut 256 wide, its tiles are shorter and still one
 * round while live panels * (N / 256) <= CUs; the kernel counts the live panels and takes the 256-wide tile body exactly then,
 * the 320-wide one otherwise (grid = the larger tile count; the workgroups past the chosen width's tiles return).  Either
 * width gives every output element the same MFMA sequence over K: the contract and the bits of kept rows are those of
 * octic_dense_gemm_nt_tokens_skip.  Eligible: mask given, mode 0, that plan, N % 256 == 0, at most 1024 panels - anything else
 * IS octic_dense_gemm_nt_tokens_skip.  OCTIC_ROUTE_DENSE_TILE + 16 / + 32 forces the wide / the narrow choice (tests, A/B). */
int octic_dense_gemm_nt_tokens_adaptive(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int mode,
                                        void* C, void* C2, int64_t ldc, const float* bias, const float* gamma, const float* rs,
                                        int64_t rows_per_sample_rs, const float* X, float* OUT, const void* H, float* colsum,
                                        const float* sample_scale, int rows_per_sample, void* workspace, int tokens,
                                        void* stream);
/* What it does with a masked launch of this problem: out[0] = 1 if the adaptive kernel takes it, out[1] = workgroups of the
 * main launch, out[2] / out[3] = the two tile widths (320, 256), out[4] = the largest live-panel count that runs the 256-wide
 * tile under the rule (-1 where 256 does not divide N).  OCTIC_ESHAPE for a bad rows_per_sample. */
int octic_dense_gemm_plan_adaptive(int M, int N, int K, int mode, int tokens, int rows_per_sample, int* out5);
/* Host query of the adaptive launch's item map (sample_scale is a HOST array), by the kernel's own functions.  Per workgroup
 * in blockIdx order: out_tm / out_tn the tile at the chosen width (-1 = the workgroup returns), out_dead 1 for a dead tile
 * (each nullable, `cap` entries); *out_width = 256 | 320.  Returns the number of workgroups, or OCTIC_ESHAPE for a launch the
 * adaptive kernel does not take or cap too small. */
int octic_dense_gemm_order_adaptive(int M, int N, int K, int mode, int tokens, const float* sample_scale, int rows_per_sample,
                                    int cap, int* out_tm, int* out_tn, int* out_dead, int* out_width);
/* octic_dense_gemm_nt_tokens_adaptive with the launch's class-token rows inside the main launch.  The adaptive launch leaves the
 * CUs of its dead tiles idle for most of its length while the class-token rows wait behind it for one or two latency-bound
 * launches of their own.  With fold_cls != 0, a launch the adaptive kernel takes whose K is at most 16 slices of 320 becomes ONE
 * launch: the adaptive launch's workgroups, workgroup for workgroup, followed at the END of the grid by class-token workgroups
 * (512 threads; an item = 16 class-token rows x 16 columns, computed inside one workgroup: a slice of 320 per wave as ten MFMAs
 * from a zero accumulator, f32 partial tiles summed in slice order from slice 0, bias in f32, one rounding - the arithmetic
 * and the bits of the stand-alone class-token kernels).  Every class-token row is written; the mask does not apply to them.
 * fold_cls == 0, or any other launch: exactly octic_dense_gemm_nt_tokens_adaptive.  When few CUs are free the class-token
 * workgroups run behind the live tiles, so callers fold where the mask is expected to drop enough samples
 * (functional.DENSE_CLS_FOLD_MIN_DROP). */
int octic_dense_gemm_nt_tokens_adaptive_cls(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int mode,
                                            void* C, void* C2, int64_t ldc, const float* bias, const float* gamma, const float* rs,
                                            int64_t rows_per_sample_rs, const float* X, float* OUT, const void* H, float* colsum,
                                            const float* sample_scale, int rows_per_sample, void* workspace, int tokens,
                                            int fold_cls, void* stream);
/* What it does (fold_cls != 0) with a masked launch of this problem: out[0] = 1 if the folded kernel takes it, out[1] = workgroups
 * of the launch, out[2] = class-token workgroups among them (the last ones), out[3] = class-token items of the busiest of those,
 * out[4] = tile workgroups in front (= out[1] of octic_dense_gemm_plan_adaptive).  OCTIC_ESHAPE for a bad rows_per_sample. */
int octic_dense_gemm_plan_adaptive_cls(int M, int N, int K, int mode, int tokens, int rows_per_sample, int* out5);
/* Host query of the folded launch's item map (sample_scale is a HOST array), by the kernel's own functions.  out_tm / out_tn /
 * out_dead / out_width: as octic_dense_gemm_order_adaptive, one entry per workgroup of the launch (-1 / -1 / 0 for a class-token
 * workgroup).  out_cls_rt / out_cls_ct: row tile and column tile (of 16) of the class-token items, out[3] entries per
 * class-token workgroup in the order it takes them, -1 = none (each nullable, `cls_cap` entries).  Returns the number of
 * workgroups, or OCTIC_ESHAPE for a launch the folded kernel does not take or a cap too small. */
int octic_dense_gemm_order_adaptive_cls(int M, int N, int K, int mode, int tokens, const float* sample_scale, int rows_per_sample,
                                        int cap, int* out_tm, int* out_tn, int* out_dead, int* out_width, int cls_cap,
                                        int* out_cls_rt, int* out_cls_ct);

/* octic_dense_gemm_nt_tokens_adaptive_cls for a launch under the stochastic-depth mask of a branch that drops each sample with
 * probability `drop`.  With 257 tokens a classic panel of 256 consecutive rows straddles two images and is dead only when both are
 * dropped (live share 1 - drop^2); a per-image panel dies with its image (1 - drop).  A masked launch of mode 0 / 5 (mode 4 too
 * under OCTIC_ROUTE_DENSE_IMAGE + 4; by itself it stays classic, see csrc/dense_gemm.hip kDgImageKeep) that the
 * former call keeps on classic panels (sample_scale per image: rows_per_sample == tokens == 257, K % 128 == 0, N % 16 == 0) runs
 * on per-image panels of the 256-wide tile - full tiles only, nothing split along K - where the modelled expected launch is a
 * tenth shorter (the model: csrc/dense_gemm.hip dense_plan_image).  Its class-token rows are computed by workgroups at the END of
 * the grid (K at most 16 slices of 320; the arithmetic and bits of dense_cls_kernel: a slice per wave, partial tiles summed in
 * slice order, the mode's epilogue; mode 5 leaves their column sums in slab rows 2 * images onward), else by the class-token
 * launch behind the main one.  The grid depends on the problem and `drop` only, never on the mask's values.  Kept rows: the bits
 * of the unmasked per-image launch with nothing split; rows of a dropped sample: those or +0, tile by tile; every class-token row
 * is computed.  drop <= 0, sample_scale NULL, or any launch it does not take (the N = 1280 launches among them): exactly
 * octic_dense_gemm_nt_tokens_adaptive_cls. */
int octic_dense_gemm_nt_tokens_image(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb, int mode,
                                     void* C, void* C2, int64_t ldc, const float* bias, const float* gamma, const float* rs,
                                     int64_t rows_per_sample_rs, const float* X, float* OUT, const void* H, float* colsum,
                                     const float* sample_scale, int rows_per_sample, void* workspace, int tokens,
                                     int fold_cls, double drop, void* stream);
/* What it does with a launch of this problem (masked != 0: with a sample_scale): out[0] = 1 if it leaves the former call's plan
 * for per-image panels, out[1] = workgroups of the main launch, out[2] = class-token workgroups among them (the last ones; 0 = a
 * launch of their own, or not taken), out[3] = class-token items (16 rows x 16 columns) of the busiest of those, out[4] = tile
 * workgroups in front, out[5] = tile width of the plan in force (256 | 320), out[6] = colsum slab rows of modes 3 / 5 under the
 * plan in force, out[7] = 1 if the plan in force is per-image panels.  OCTIC_ESHAPE for a bad shape or rows_per_sample. */
int octic_dense_gemm_plan_image(int M, int N, int K, int mode, int tokens, int rows_per_sample, int masked, double drop, int* out8);
/* Host query of a taken launch's item map (sample_scale is a HOST array), by the kernel's own functions.  Per workgroup in blockIdx
 * order: out_tm / out_tn the tile (-1 for a class-token workgroup), out_dead 1 for a dead tile (each nullable, `cap` entries);
 * out_cls_rt / out_cls_ct as octic_dense_gemm_order_adaptive_cls.  Returns the number of workgroups, or OCTIC_ESHAPE for a launch
 * not taken or a cap too small. */
int octic_dense_gemm_order_image(int M, int N, int K, int mode, int tokens, const float* sample_scale, int rows_per_sample, double drop,
                                 int cap, int* out_tm, int* out_tn, int* out_dead, int cls_cap, int* out_cls_rt, int* out_cls_ct);

/* Weight gradient of an nn.Linear of the standard half (the autograd of deit/vit.py:33,46 and of timm Mlp.fc1 / fc2):
 *     dW[N,K] = dY[M,N]^T . X[M,K]     f32, nn.Linear layout
 * dY, X bf16 row-major (ldy, ldx row strides in elements), N % 256 == 0, K % 256 == 0 or K % 320 == 0, at most 1024
 * output tiles, M * ld * 2 < 2^31.  The reduction over the M token rows is cut into row slabs (one workgroup per slab and
 * 256 x 256 or 256 x 320 tile, all tiles of a slab walking the same rows in lockstep); the f32 partial tiles are summed in slab order by the
 * last workgroup of a tile (bitwise reproducible).  Shapes those tiles do not divide with N % 64 == 0 and K % 64 == 0 (the
 * narrow DeiT-III blocks, D = 192 / 384) take 64 x 64 tiles: row slabs of f32 partial tiles summed in slab order by a
 * second launch (also bitwise reproducible).  workspace: octic_dense_wgrad_workspace_bytes(M,N,K) bytes, zeroed
 * once at allocation.                                                                                                 */
int64_t octic_dense_wgrad_workspace_bytes(int M, int N, int K);
/* Tile width along K the launch will use: 256 (256 x 256 tiles, whenever K % 256 == 0) or 320 (256 x 320 tiles: K % 320 == 0
 * only), 64 on the narrow path, 0 for a shape no path takes.  Informational (profilers see dense_tn_kernel<4, ..> / <5, ..>). */
int octic_dense_wgrad_tile(int M, int N, int K);
/* Host-only query: the accept-and-plan function of the TN launchers (dw_route, csrc/dense_wgrad.hip).  One problem (N1 = 0) or
 * the pair [N0 | N1] of octic_dense_wgrad_tn_pair; ld_max = the largest operand row stride in elements (0 = not known: the
 * stride bound is not checked).  out[0] = tile width (64 | 256 | 320), out[1] = output tiles, out[2] = row slabs, out[3] = 0.
 * OCTIC_ESHAPE for what the launchers refuse by shape or stride bound (pointer alignment and ld % 8 are theirs to check). */
int octic_dense_wgrad_plan(int M, int N0, int N1, int K, int64_t ld_max, int out[4]);
int octic_dense_wgrad_tn(const void* dY, const void* X, int M, int N, int K, int64_t ldy, int64_t ldx, float* dW,
                         void* workspace, void* stream);
/* Two weight gradients that share the token rows M and K as ONE launch (tile list = [problem 0 | problem 1], row slabs chosen
 * for the sum): the qkv and proj weight gradients of a standard block (deit/vit.py:33-45).  Results bit-identical to two
 * octic_dense_wgrad_tn calls whenever the joint launch picks the slab counts those would (each tile sums its slabs in slab
 * order); workspace: octic_dense_wgrad_pair_workspace_bytes.                                                            */
int64_t octic_dense_wgrad_pair_workspace_bytes(int M, int N0, int N1, int K);
int octic_dense_wgrad_tn_pair(const void* dY0, const void* X0, int N0, int64_t ldy0, int64_t ldx0, float* dW0,
                              const void* dY1, const void* X1, int N1, int64_t ldy1, int64_t ldx1, float* dW1, int M, int K,
                              void* workspace, void* stream);
/* The same two launches inside a block with stochastic depth (timm DropPath in deit/vit.py: x + drop_path(gamma * f(norm(x)))).
 * sample_scale: NULL (= the plain call) or the [M / rows_per_sample] f32 factors (0 or 1 / keep) the block multiplies the
 * branch with, sample b owning token rows [b rows_per_sample, (b + 1) rows_per_sample); for the pair ONE mask for both
 * problems.  CONTRACT: sample_scale[b] == 0 promises that every dY row of sample b (dY0 and dY1 of the pair) is zero.  The
 * 256- / 320-wide kernel may then leave those rows of dY and X unread: it walks only the 64-row reduction steps that touch a
 * sample with a non-zero factor, inside the same row slabs and with the same slab order in the final sum.  The mask is a hint
 * only: with the promise kept the result is what the unmasked launch writes (the 64 x 64 path ignores it; so does a launch
 * whose slabs exceed 16 384 steps).  OCTIC_ESHAPE when the mask is given and rows_per_sample <= 0 or M % rows_per_sample != 0.
 * Workspace and plan queries: those of the plain calls.                                                                  */
int octic_dense_wgrad_tn_skip(const void* dY, const void* X, int M, int N, int K, int64_t ldy, int64_t ldx, float* dW,
                              const float* sample_scale, int rows_per_sample, void* workspace, void* stream);
int octic_dense_wgrad_tn_pair_skip(const void* dY0, const void* X0, int N0, int64_t ldy0, int64_t ldx0, float* dW0,
                                   const void* dY1, const void* X1, int N1, int64_t ldy1, int64_t ldx1, float* dW1, int M, int K,
                                   const float* sample_scale, int rows_per_sample, void* workspace, void* stream);

/* ---- float32 dense GEMMs of the standard half (csrc/dense_f32.hip) -------------------------------------------------------
 * The nn.Linear of a standard block (deit/vit.py:14-56; dinov2/layers/mlp.py, swiglu_ffn.py, attention.py) when the model runs
 * in float32: forward, input gradient, weight gradient (+ bias gradient) and the GELU backward.  Everything is f32 row-major:
 *     octic_dense_f32_nt   C[M,N]  = A[M,K] . W[N,K]^T (+ bias[N]);  gelu != 0: H = that, C = gelu(H) (exact erf GELU, nn.GELU())
 *     octic_dense_f32_nn   DX[M,K] = G[M,N] . W[N,K]                 (W as stored: no transposed copy)
 *     octic_dense_f32_tn   DW[N,K] = G[M,N]^T . X[M,K],  db[N] = column sums of G when db != NULL
 *     octic_dense_gelu_bwd_f32   dh = gelu'(h) * g on dense [rows, d];  db != NULL: db[d] = column sums of dh
 * Limits: M >= 1, N % 4 == 0, K % 4 == 0, every row stride (elements) a multiple of 4 and >= its row length, pointers 16-byte
 * aligned, (largest of M, N, K) * (largest row stride) < 2^31.  Shape violations: OCTIC_ESHAPE; alignment: OCTIC_EALIGN; a
 * missing operand: OCTIC_ENULL; a short TN workspace: OCTIC_EWORKSPACE - all before any launch.  Every M / N / K tail is
 * handled inside the kernel: nothing past an edge is read or written.
 * ARITHMETIC CONTRACT.  Products run on v_mfma_f32_16x16x4_f32: exact f32 inputs, one rounding per product, f32 accumulate.
 * An element of an NT / NN result is ONE fmaf chain from +0 over the reduction index (K for NT, N for NN) - blocks of 16
 * ascending, inside a block e, 4 + e, 8 + e, 12 + e for e = 0 .. 3 - then one addition of the bias.  No split of the reduction
 * over workgroups; the order depends on the reduction length alone, not on M, the row's position or its tile, and a result
 * row reads that row of A / G, W and the bias only: a sample's rows are bitwise independent of its batch mates.
 * TN reduces over the M token rows in row slabs (multiples of 32 rows): each slab is one such chain per element into an f32
 * partial tile in the workspace, and a second launch adds the partials in slab order.  db: sequential over a slab's rows, then
 * slab order.  The slab count is a function of (M, N, K) alone (octic_dense_f32_plan out[2]); with one slab the result goes
 * straight to DW.  The GELU backward sums 256 row blocks (octic_dense_gelu_blocks()) in the order of octic_dense_finish.
 * No floating-point atomics: every result is bitwise repeatable.  Subnormals are kept.
 * op of the queries: 0 = NT, 1 = NN, 2 = TN. */
#define OCTIC_DENSE_F32_NT 0
#define OCTIC_DENSE_F32_NN 1
#define OCTIC_DENSE_F32_TN 2
/* Host-only query: the accept-and-plan function the three launchers call.  ld_max = the largest operand row stride in
 * elements (0 = not known: only the shape is judged).  out[0] = tile rows, out[1] = tile columns of the output, out[2] = row
 * slabs (1 for NT / NN), out[3] = workgroups of the main launch.  OCTIC_ESHAPE exactly where the launchers refuse by shape or
 * stride bound: N or K no multiple of 4, M < 1, ld_max below the longest operand row, the 2^31 offset bound (per-operand
 * strides, ld % 4 and pointer alignment are theirs to check). */
int octic_dense_f32_plan(int op, int64_t M, int64_t N, int64_t K, int64_t ld_max, int out[4]);
/* bytes of the workspace of octic_dense_f32_tn (slab partials; 256 where the plan has one slab, and for op NT / NN);
 * OCTIC_ESHAPE for a shape the plan refuses.  The workspace needs no initialisation. */
int64_t octic_dense_f32_workspace_bytes(int op, int64_t M, int64_t N, int64_t K);
/* bias nullable; H / ldh are used with gelu != 0 only. */
int octic_dense_f32_nt(const float* A, const float* W, const float* bias, int64_t M, int64_t N, int64_t K, int64_t lda,
                       int64_t ldw, float* C, int64_t ldc, int gelu, float* H, int64_t ldh, void* stream);
int octic_dense_f32_nn(const float* G, const float* W, int64_t M, int64_t N, int64_t K, int64_t ldg, int64_t ldw, float* DX,
                       int64_t ldx, void* stream);
/* DW may be any [N,K] view with row stride ldw (a gradient-bucket view); db nullable; workspace nullable where the plan has one
 * slab. */
int octic_dense_f32_tn(const float* G, const float* X, int64_t M, int64_t N, int64_t K, int64_t ldg, int64_t ldx, float* DW,
                       int64_t ldw, float* db, void* workspace, int64_t workspace_bytes, void* stream);
/* partials: [octic_dense_gelu_blocks(), d] f32, required with db (both nullable together: no column sums); d % 4 == 0. */
int octic_dense_gelu_bwd_f32(const float* h, const float* g, float* dh, float* partials, float* db, int64_t rows, int d,
                             void* stream);

/* ---- row kernels of the DINOv2 objective over the prototype axis (K % 8 == 0, row strides % 8 == 0) -----
 * octic_softmax_center: out[r, :] = softmax((t[r, :] - center) * inv_temp) in f32 - the teacher's centred, sharpened
 * probabilities (dinov2/loss/dino_clstoken_loss.py:43-51, ibot_patch_loss.py:63-77); center may be NULL; t f32 or bf16.
 * octic_soft_ce_fwd: loss[r] = -sum_k t_k log_softmax(s[r, :] * inv_temp)_k with t = tprob[r % t_rows, :] (several student
 * crops against the same teacher rows: dino_clstoken_loss.py:78-92; the masked patch tokens: ibot_patch_loss.py:26-34), plus
 * the row statistics the gradient needs (lse[r], tsum[r] = sum_k t_k).  octic_soft_ce_bwd: ds[r, k] = g[r] inv_temp
 * (softmax(s inv_temp)_k tsum[r] - t_k) in s's dtype.  s is read in its storage dtype (bf16 under autocast), arithmetic f32. */
int octic_softmax_center(const void* t, int t_dtype, int64_t ldt, const float* center, float inv_temp, float* out,
                         int64_t rows, int K, void* stream);
int octic_soft_ce_fwd(const void* s, int s_dtype, int64_t lds, const float* tprob, int64_t t_rows, float inv_temp,
                      float* loss, float* lse, float* tsum, int64_t rows, int K, void* stream);
int octic_soft_ce_bwd(const void* s, int s_dtype, int64_t lds, const float* tprob, int64_t t_rows, float inv_temp,
                      const float* g, const float* lse, const float* tsum, void* ds, int64_t ldd, int64_t rows, int K,
                      void* stream);

/* ---- Sinkhorn-Knopp teacher targets of the DINO / iBOT terms (dinov2/loss/dino_clstoken_loss.py:53-76,
 * ibot_patch_loss.py:79-116) without the K x B matrix Q: with E[b, k] = exp((x[b, k] - rowmax[b]) * inv_temp), rowmax[b] the
 * largest logit of row b, every state of Q is E[b, k] u[k] v[b].  One round is  r = protos(shift = rowmax, weight = v);
 * [all-reduce r over ranks];  u = 1 / r;  c = rows(u);  v = 1 / c;  the first round's weight is exp((rowmax[b] - m) *
 * inv_temp) with m the maximum of rowmax over all ranks (rowmax from octic_sinkhorn_rows with u = NULL), the last round ends
 * in octic_sinkhorn_final, which sums its own c.  The reference's total sum and its constants K and B cancel in the result
 * and are not applied; the result is finite where the reference's exp(x / temp) overflows.  x is f32 or bf16 [rows, K] with
 * row stride ldx >= K, 16-byte aligned rows; K % 8 == 0; inv_temp > 0; rows >= 1 (rows == 0 is OCTIC_ESHAPE: there is no
 * round to run); u, r, partials, out 16-byte aligned f32.  No atomics and fixed summation orders: bitwise reproducible.
 * octic_sinkhorn_slabs: the row slabs of the prototype-sum pass for this row count (OCTIC_ESHAPE for rows < 1).
 * octic_sinkhorn_protos: r[k] = sum_b weight[b] exp((x[b, k] - shift[b]) inv_temp); partials is a [slabs, K] f32 workspace,
 *   nullable where slabs == 1.  octic_sinkhorn_rows: rowmax[b] = max_k x[b, k], c[b] = sum_k u[k] E[b, k] (u nullable: 1).
 *   octic_sinkhorn_final: out[b, k] = u[k] E[b, k] / sum_k' u[k'] E[b, k'], contiguous [rows, K] f32 (u nullable: 1). */
int octic_sinkhorn_slabs(int64_t rows);
int octic_sinkhorn_protos(const void* x, int x_dtype, int64_t ldx, float inv_temp, const float* shift, const float* weight,
                          float* partials, float* r, int64_t rows, int K, void* stream);
int octic_sinkhorn_rows(const void* x, int x_dtype, int64_t ldx, float inv_temp, const float* u, float* rowmax, float* c,
                        int64_t rows, int K, void* stream);
int octic_sinkhorn_final(const void* x, int x_dtype, int64_t ldx, float inv_temp, const float* u, float* out, int64_t rows,
                         int K, void* stream);

/* ---- KoLeo regularizer of the DINOv2 objective (dinov2/loss/koleo_loss.py:18-48), one forward and one backward launch ------
 * x is [groups * n, D] f32 or bf16 with element stride 1, row stride ldx >= D and 16-byte aligned rows, read as `groups`
 * independent groups of n consecutive rows (the recipe: the two global crops).  All arithmetic is f32 after one widening.  Per
 * row i of a group: inv[i] = 1 / max(||x_i||, eps), xh_i = x_i inv[i]; nn[i] = the group-local index of the row j != i with the
 * largest xh_i . xh_j - on equal dots the LOWEST j (torch.max leaves ties unspecified: this rule is ours), a NaN dot counts as
 * -inf, the row itself is excluded; dist[i] = ||xh_i - xh_nn[i] + 1e-8|| (nn.PairwiseDistance adds its eps to every element);
 * term[i] = -log(dist[i] + eps).  The loss of a group is the mean of its terms, taken by the caller.
 * octic_koleo_bwd: from gterm = d loss / d term and the saved x, nn, inv, dist: G_i = c_i e_i - sum over the j with nn[j] == i
 * (ascending, gathered by the workgroup of row i: no atomics) of c_j e_j, c = -gterm / (dist + eps), e = (xh - xh_nn + 1e-8) /
 * dist; then autograd's F.normalize: dx_i = (G_i - xh_i (xh_i . G_i)) inv[i] where ||x_i|| >= eps, G_i / eps below it; dx in
 * x's dtype, rounded once, row stride lddx >= D, 16-byte aligned rows.
 * A row's nn, term and dx depend on the rows of its own group, n and D only - not on groups, the group's position, the row
 * strides or the rest of the batch - and two calls are bitwise equal (fixed summation orders).
 * octic_koleo_ok: 1 where the kernels take the shape, else 0 - the only place the range lives: groups >= 1, 2 <= n <= 256,
 * 8 <= D <= 4096, D % 8 == 0, groups * n < 2^31.  The entry points return OCTIC_ENULL, OCTIC_EDTYPE, OCTIC_ESHAPE (a shape
 * octic_koleo_ok refuses, ldx or lddx < D) and OCTIC_EALIGN before any launch. */
int octic_koleo_ok(int64_t groups, int64_t n, int64_t D);
int octic_koleo_fwd(const void* x, int x_dtype, int64_t ldx, int64_t groups, int64_t n, int64_t D, float eps, float* term,
                    int32_t* nn, float* inv, float* dist, void* stream);
int octic_koleo_bwd(const void* x, int x_dtype, int64_t ldx, int64_t groups, int64_t n, int64_t D, float eps,
                    const float* gterm, const int32_t* nn, const float* inv, const float* dist, void* dx, int64_t lddx,
                    void* stream);

/* ---- input rows of a DINO / iBOT head call (dinov2/train/ssl_meta_arch.py:226-267) ----------------------------------------
 * octic_head_rows: segments_dev is a DEVICE table of 1 .. 4 octic_head_segment.  Row r < n of a segment is source row
 * j = idx ? idx[r] : r, which sits at base + (j / inner) * outer_ld + (j % inner) * inner_ld elements (the class tokens
 * x_norm[:, 0]: inner 1, outer_ld = T D; the masked patch tokens x_norm[:, 1 + R:].flatten(0, 1)[idx]: inner = the patches of an
 * image, outer_ld = T D, inner_ld = D, base at the first patch token), and belongs to row out_row0 + r of out [rows_out, D]
 * (dtype OCTIC_F32 / OCTIC_BF16, element stride 1, row stride ldo >= D).  scatter == 0: the source rows are copied to out and
 * every row of out that no segment covers is written as +0 (the padding up to `upperbound`).  scatter != 0: the rows of out
 * (cotangents) are written back to their sources with plain stores - indices are distinct, as mask_indices_list is; the caller
 * zero-fills the destination once.  A row whose j lies outside [0, src_rows) is +0 in the gather and skipped by the scatter.
 * Rows move as 16-byte chunks: the bytes of a row do not depend on the row count, the row's position or its neighbours; no
 * atomics.  The host cannot see the table: 16-byte aligned source rows and segments that do not overlap in out are the
 * caller's to keep.  8 <= D <= 2^20, D % 8 == 0, 1 <= rows_out < 2^31, 1 <= n_segments <= 4.  OCTIC_ENULL, OCTIC_EDTYPE,
 * OCTIC_ESHAPE (also ldo < D) and OCTIC_EALIGN (out or its row stride off 16 bytes) are returned before any launch. */
typedef struct octic_head_segment {
  const void* base;      /* first source row (dtype elements)                                  */
  const int64_t* idx;    /* [n] source row indices on the device, or NULL = 0 .. n-1            */
  int64_t n;             /* rows of the segment                                                 */
  int64_t inner;         /* source rows per outer step (>= 1)                                   */
  int64_t outer_ld;      /* elements between outer steps                                        */
  int64_t inner_ld;      /* elements between the rows of one outer step                         */
  int64_t out_row0;      /* first row of out the segment owns                                   */
  int64_t src_rows;      /* addressable source rows: j outside [0, src_rows) is never touched   */
} octic_head_segment;
int octic_head_rows(const octic_head_segment* segments_dev, int n_segments, int64_t rows_out, int64_t D, int dtype, void* out,
                    int64_t ldo, int scatter, void* stream);

/* ---- the normalisations of the DINO / iBOT head (dinov2/layers/dino_head.py:36-41) -----------------------------------------
 * F.normalize(x, dim=-1, p=2, eps) over the rows of x [rows, D] (OCTIC_F32 / OCTIC_BF16, element stride 1, row stride ldx >=
 * D, 16-byte aligned rows).  octic_l2norm_rows_fwd: the sum of squares in f32 after one widening, n = sqrt(sum),
 * d = n < eps ? eps : n (clamp_min: a NaN norm stays NaN), y = x / d rounded once to y_dtype, inv[row] = 1 / d (f32 [rows]).
 * octic_l2norm_rows_bwd: from the cotangent g of y, x and the saved inv: with yh = x inv (f32) and the norm summed again in
 * the forward's order, dx = inv (g - yh (yh . g)) where n >= eps (or NaN) and dx = g inv where n < eps - clamp_min passes no
 * gradient there, as autograd has it; dx has x's dtype, rounded once.  One wave per row; a lane adds the elements of its 16-byte
 * chunks (chunk c: lane c % 64) in ascending order and the 64 lane sums meet in a fixed butterfly: the order depends on D
 * alone, a row's bytes do not depend on the row count, its position or its neighbours (a NaN row stays alone), no atomics, two
 * calls are bitwise equal.  octic_l2norm_ok: 1 where the kernels take the shape - 1 <= rows < 2^31, 8 <= D <= 4096,
 * D % 8 == 0 - else 0.  OCTIC_ENULL, OCTIC_ESHAPE (also a row stride < D), OCTIC_EDTYPE and OCTIC_EALIGN come before any launch.
 *
 * nn.utils.weight_norm(nn.Linear(K, N, bias=False)) (dim 0) without the f32 weight.  octic_weight_norm_prep: from v [N, K] and
 * g [N] (f32, dense, 16-byte aligned) in one pass: norms[n] = ||v[n]|| (f32 sum in a fixed order that depends on K alone),
 * W[n, k] = bf16(g[n] v[n, k] (1 / norms[n])) dense [N, K] - torch._weight_norm's arithmetic, rounded once - and, where Wt is
 * not NULL, the same values as Wt [K, N] (N % 8 == 0 then), staged through LDS so that its stores run along N; Wt == NULL
 * writes nothing but W and norms.  octic_weight_norm_bwd: from the f32 gradient dW [N, K] of that weight, v, g and norms: with
 * r = 1 / norms[n] and s = dW[n] . v[n]:  dg[n] = s r,  dv[n, k] = g[n] (r dW[n, k] - r^3 s v[n, k])  (autograd of
 * torch._weight_norm), f32 throughout, one wave per row.  1 <= N < 2^29, 8 <= K <= 2048, K % 8 == 0.  OCTIC_ENULL,
 * OCTIC_ESHAPE and OCTIC_EALIGN come before any launch. */
int octic_l2norm_ok(int64_t rows, int64_t D);
int octic_l2norm_rows_fwd(const void* x, int x_dtype, int64_t ldx, int64_t rows, int64_t D, float eps, void* y, int y_dtype,
                          int64_t ldy, float* inv, void* stream);
int octic_l2norm_rows_bwd(const void* g, int g_dtype, int64_t ldg, const void* x, int x_dtype, int64_t ldx, const float* inv,
                          int64_t rows, int64_t D, float eps, void* dx, int64_t lddx, void* stream);
int octic_weight_norm_prep(const float* v, const float* g, int64_t N, int64_t K, void* W, void* Wt, float* norms, void* stream);
int octic_weight_norm_bwd(const float* dW, const float* v, const float* g, const float* norms, int64_t N, int64_t K, float* dv,
                          float* dg, void* stream);

/* ---- linear-probe evaluation of a frozen backbone (dinov2/eval/linear.py) ----------------------------------------------
 * The grid of nn.Linear(K_h, C) classifiers of setup_linear_classifiers (linear.py:237-258) as one launch per stage over
 * all classifiers.  Every classifier reads a column range [col0, col0 + K) of one f32 feature row
 * F = [cls(L-n) | ... | cls(L-1) | mean patch(L-1)] (create_linear_input, linear.py:173-185) and is described by one entry of
 * a DEVICE table; tile0 is the running sum of K / 64 over the entries before it (the table is in tile0 order).  K % 64 == 0,
 * col0 % 4 == 0, w / mw 16-byte aligned, W is [C, K] row-major (nn.Linear's layout); the host cannot see the table, so
 * these are the caller's to keep.  Exact f32 (f32-input MFMA), no atomics, fixed summation orders: bitwise reproducible. */
typedef struct {
  float* w;       /* [C, K] weight           */
  float* b;       /* [C]    bias             */
  float* mw;      /* [C, K] momentum of w    */
  float* mb;      /* [C]    momentum of b    */
  int32_t col0;   /* first feature column    */
  int32_t K;      /* input width             */
  int32_t lr_index; /* index into the device learning-rate buffer of octic_probe_sgd */
  int32_t tile0;  /* sum of K / 64 over the entries before this one */
} octic_probe_head;
/* F[b, i D : (i+1) D] = float(cls[i][b, :]) for i < n (n <= 4; cls[i] + b cls_ld[i] is image b's class token of the i-th
 * normed block output), F[b, n D : (n+1) D] = the mean of the P patch tokens patch[b, t, :] (strides patch_ld_b /
 * patch_ld_t in elements) of the last one: f32 sum in token order, times 1/P, rounded to the token dtype as torch.mean
 * rounds it.  cls and cls_ld are HOST arrays of n entries; tokens f32 or bf16; D % 64 == 0.                              */
int octic_probe_features(const void* const* cls, const int64_t* cls_ld, int n, const void* patch, int64_t patch_ld_b,
                         int64_t patch_ld_t, int dtype, int64_t B, int P, int D, float* F, int64_t ldf, void* stream);
/* logits[h][B, C] = F[:, col0_h : col0_h + K_h] W_h^T + b_h for every table entry (LinearClassifier.forward,
 * linear.py:201-203; AllClassifiers.forward, linear.py:212-213).  B and C arbitrary; logits is [nheads, B, C] contiguous.  */
int octic_probe_forward(const octic_probe_head* heads, int nheads, const float* F, int64_t ldf, int B, int C, float* logits,
                        void* stream);
/* Per logit row: the cross entropy against labels[b] (int64 class indices in [0, C)), rowloss / rowrank (rank = number of
 * logits strictly greater than the label's; both [nheads, B] scratch) and, when dlogits is not NULL, dlogits =
 * (softmax - onehot) / B (the gradient of nn.CrossEntropyLoss(), linear.py:357).  Then per classifier, each optional:
 * loss_mean[h] = the batch mean, loss_sum[h] += the batch sum, topk[2h] += rows with rank < 1, topk[2h+1] += rows with
 * rank < 5 (the MEAN_ACCURACY top-1 / top-5 of evaluate_linear_classifiers, linear.py:262-312) - device accumulators.    */
int octic_probe_ce(const float* logits, const int64_t* labels, int nheads, int B, int C, float* dlogits, float* rowloss,
                   int* rowrank, float* loss_mean, float* loss_sum, int* topk, void* stream);
/* Weight gradient and torch.optim.SGD(momentum, weight_decay=0) step in one pass (linear.py:361-365, 519): per 64 x 64 tile
 * of W_h, g = dlogits_h^T F[:, col0_h + ...] summed over b = 0 .. B-1 in order, mw = momentum mw + g, w -= lr[lr_index_h] mw;
 * the same for the bias with the column sums of dlogits_h.  Zero momentum buffers reproduce SGD's first step.  lr is a
 * device f32 buffer.  total_ktiles = sum of K_h / 64.                                                                  */
int octic_probe_sgd(const octic_probe_head* heads, int nheads, int total_ktiles, const float* F, int64_t ldf,
                    const float* dlogits, int B, int C, const float* lr, float momentum, void* stream);

/* ---- attentive-probe evaluation of a frozen backbone (dinov2/eval/segmentation/eval_classification.py; csrc/attnpool.hip) ----
 * The grid of G AttnPoolClassifier heads (one query token, kv = nn.Linear(D, 2D), SDPA with H = D / 64 heads of 64,
 * nn.Linear(D, C)) on f32 patch tokens X [B, N, D] (row stride ldx), without keys or values: with Wk = kv.weight[:D],
 * Wv = kv.weight[D:], scale = 1/8, GH = G H and c = g H + h,
 *     U[c, :] = scale sum_j q_g[64h+j] Wk_g[64h+j, :];   S = X U^T (octic_dense_f32_nt);   P[b, :, c] = softmax_n S[b, :, c];
 *     Z[b, c, :] = sum_n P[b, n, c] X[b, n, :];          pooled[b, g D + 64h+j] = Wv_g[64h+j, :] . Z[b, c, :] + bv_g[64h+j]
 * (the key bias adds a constant over n and cancels in the softmax; sum_n P = 1 carries the value bias through).  The linear
 * layer and the loss are octic_probe_forward / octic_probe_ce on pooled as [B, G D] with col0 = g D.
 * Arguments of type `const float* const*` / `float* const*` are DEVICE arrays of G pointers, one per classifier; the host
 * cannot see them, so 16-byte alignment of the pointers in them is the caller's to keep (the array itself is checked).
 * Limits: D % 64 == 0, 64 <= D <= 16384, 1 <= B <= 65535, 1 <= G <= 1024, N, C >= 1, row strides multiples of 4 and no
 * shorter than their rows: OCTIC_ESHAPE / OCTIC_EALIGN, OCTIC_ENULL for a missing operand, all before any launch.  Every
 * token, column and batch tail is handled inside the kernels.
 * ARITHMETIC CONTRACT.  The products (pool, value, dinput, dweight, dz, dwv and the first pass of dscores) run on
 * v_mfma_f32_16x16x4_f32: an element is ONE chain from +0 over its reduction index in chunks of 16 ascending, step e of a
 * chunk adding indices e, 4 + e, 8 + e, 12 + e; then one multiplication by alpha and one addition of the bias where there
 * is one.  The order depends on the reduction length alone, and everything that belongs to image b reads image b only: a
 * sample's rows are bitwise independent of its batch mates.  Token reductions of the softmax and its backward: token lanes
 * y = n mod 4 sequentially, then lanes 0 .. 3.  No floating-point atomics: every result is bitwise repeatable. */
/* U [rows, D] dense, rows in GH .. GH + 3: rows >= GH are written as zero (the padding octic_dense_f32_nt's N % 4 needs). */
int octic_attnpool_fold(const float* const* q, const float* const* wk, int G, int D, float* U, int64_t rows, void* stream);
/* In place on S [B N, lds]: columns < GH become the softmax over the N rows of each image (exp2 domain, maximum subtracted:
 * finite for finite scores, exactly 1 for N = 1), columns GH .. lds-1 become zero. */
int octic_attnpool_softmax(float* S, int64_t lds, int64_t B, int N, int GH, void* stream);
/* Z [B, GH, D] dense from P [B N, ldp] and X [B N, ldx]. */
int octic_attnpool_pool(const float* P, int64_t ldp, const float* X, int64_t ldx, int64_t B, int N, int D, int GH, float* Z,
                        void* stream);
/* pooled [B, ldo >= G D] from Z; wv[g] = Wv_g [D, D] row-major, bv[g] = its bias [D]. */
int octic_attnpool_value(const float* Z, const float* const* wv, const float* const* bv, int B, int G, int D, float* pooled,
                         int64_t ldo, void* stream);
/* The backward of G nn.Linear(K, C) layers whose logit gradients are dlogits [G, B, C] dense (octic_probe_ce's):
 * dinput:  dF[b, g D + d] = alpha sum_c dlogits[g, b, c] w[g][c, d]                     (w[g] [C, D] row-major);
 * dweight: dw[g][c, k] = alpha sum_b dlogits[g, b, c] F[b, col0 + g col_stride + k]     (dw[g] [C, K] dense; K any);
 * colsum:  dst[g][c] = alpha sum_r src[g group_stride + r ld + c], r ascending          (bias gradients). */
int octic_attnpool_dinput(const float* dlogits, const float* const* w, int G, int B, int C, int D, float alpha, float* dF,
                          int64_t ldd, void* stream);
int octic_attnpool_dweight(const float* dlogits, const float* F, int64_t ldf, int64_t col0, int64_t col_stride, int G, int B,
                           int C, int K, float alpha, float* const* dw, void* stream);
int octic_attnpool_colsum(const float* src, int64_t group_stride, int64_t ld, int G, int rows, int cols, float alpha,
                          float* const* dst, void* stream);
/* dZ[b, c, :] = sum_j dpooled[b, g D + 64h+j] Wv_g[64h+j, :];   dwv[g][64h+j, :] = sum_b dpooled[b, g D + 64h+j] Z[b, c, :]. */
int octic_attnpool_dz(const float* dpooled, int64_t ldd, const float* const* wv, int B, int G, int D, float* dZ, void* stream);
int octic_attnpool_dwv(const float* dpooled, int64_t ldd, const float* Z, int B, int G, int D, float* const* dwv, void* stream);
/* dS [B N, ldp] = P (dP - sum_n P dP) with dP[b, n, c] = X[b, n, :] . dZ[b, c, :]: two launches, dP lives in dS between them
 * (dS must not be P); columns GH .. ldp-1 of dS become zero.  dU = dS^T X is octic_dense_f32_tn. */
int octic_attnpool_dscores(const float* X, int64_t ldx, const float* dZ, const float* P, int64_t ldp, int64_t B, int N, int D,
                           int GH, float* dS, void* stream);
/* dq[g][64h+j] = scale Wk_g[64h+j, :] . dU[c, :];  dwk[g][64h+j, :] = scale q_g[64h+j] dU[c, :];  dbk[g][:] = 0 exactly (the
 * key bias cannot change any output).  dU [GH (+ padding), D] dense. */
int octic_attnpool_unfold(const float* const* q, const float* const* wk, const float* dU, int G, int D, float* const* dq,
                          float* const* dwk, float* const* dbk, void* stream);

/* ---- linear segmentation evaluation of a frozen backbone (dinov2/eval/segmentation/eval_segmentation.py) --------------
 * Multinomial logistic regression (LogregClassifier, :281-337) on standardised f32 patch features X [N, D] (row stride ldx
 * elements, 16-byte aligned rows) resident in device memory; W is [C, D] row-major, contiguous.  Supported: 2 <= C <= 256,
 * D % 64 == 0, N >= 1 (anything else: OCTIC_ESHAPE before any launch).  Exact f32 (f32-input MFMA), no floating-point
 * atomics, fixed summation orders: bitwise reproducible.  All row and element offsets are 64-bit.
 * octic_seg_ldd: the row stride of dlogits, 32 ceil(C / 32) floats (columns C .. ldd-1 are written as zero).
 * octic_seg_slabs: row slabs the weight gradient cuts N into (informational).
 * octic_seg_workspace_bytes: one workspace (256-byte aligned) serves octic_seg_value_dlogits and octic_seg_wgrad.       */
int octic_seg_ldd(int C);
int octic_seg_slabs(int64_t N, int D, int C);
int64_t octic_seg_workspace_bytes(int64_t N, int D, int C);
/* value[0] (DEVICE f64) = sum_n CE(X_n W^T + b, y_n) and dlogits [N, ldd] = softmax - onehot; y holds int32 class indices,
 * a row whose y is outside [0, C) contributes nothing.  The logits never reach memory.                                  */
int octic_seg_value_dlogits(const float* X, int64_t ldx, int64_t N, int D, const float* W, const float* b, int C,
                            const int32_t* y, float* dlogits, double* value, void* workspace, void* stream);
/* pred[n] = argmax_c (X_n W^T + b)_c, the first maximum (LogisticRegression.predict before the classes_ lookup).        */
int octic_seg_predict(const float* X, int64_t ldx, int64_t N, int D, const float* W, const float* b, int C, int32_t* pred,
                      void* stream);
/* dW [C, D] = scale dlogits^T X + lambda W and db [C] = scale colsum(dlogits): N cut into row slabs over all CUs, f32 partial
 * tiles summed in slab order (f64) by a finish launch.  X is read once, dlogits D / tile-width times.                    */
int octic_seg_wgrad(const float* X, int64_t ldx, int64_t N, int D, const float* dlogits, int C, const float* W, double scale,
                    double lambda, float* dW, float* db, void* workspace, void* stream);
/* StandardScaler (segmentation/utils.py:566-573): per-column mean and population variance over the N rows accumulated in f64
 * (mean, var: DEVICE f64 [D]), and the transform in place, x = float(float(x - mean) / scale).                          */
int64_t octic_seg_colstats_workspace_bytes(int64_t N, int D);
int octic_seg_colstats(const float* X, int64_t ldx, int64_t N, int D, double* mean, double* var, void* workspace, void* stream);
int octic_seg_standardize(float* X, int64_t ldx, int64_t N, int D, const double* mean, const double* scale, void* stream);
/* mode[r] = the most frequent of the L pixel labels labels[r, :] (integers of esize 1, 2, 4 or 8 bytes, values 0 .. 255),
 * the smallest on a tie, as torch.mode (Classifier.fit, eval_segmentation.py:83; LogregClassifier._fit :331).           */
int octic_seg_patch_mode(const void* labels, int esize, int64_t R, int L, int32_t* mode, void* stream);
/* counts[t * 256 + pred[r]] += number of pixels of row r with label t, for every t with ignore[t] == 0 (ignore: DEVICE
 * uint8 [256]; counts: DEVICE int64 [256 * 256], accumulated): the confusion matrix behind accuracy / mIoU (:50-61).     */
int octic_seg_confusion(const void* labels, int esize, int64_t R, int L, const int32_t* pred, const uint8_t* ignore,
                        int64_t* counts, void* stream);

/* ---- the k-NN classifier of the segmentation evaluation (KNNClassifier, eval_segmentation.py:172-278) ------------------
 * For each of n query rows Q [n, D] (row stride ldq) the kmax nearest of M key rows K [M, D] (row stride ldk, so a
 * sub-sampled training set is a stride) under the SQUARED L2 distance (|a|^2 + |b|^2) - 2 a.b, the cosine distance
 * 1 - a.b / (|a| |b|), or both from one pass (metrics: 1 = L2, 2 = cosine, 3 = both).  The distance matrix never reaches
 * memory.  qnorm [n] / knorm [M] are the squared row norms octic_seg_rownorms writes; skip (nullable, DEVICE uint8 [M]) marks
 * key rows that must not be listed.
 * TOTAL ORDER: (distance, key row index): the smaller distance first, on equal distance the lower index.  A NaN distance
 * counts as +inf; a key at distance +inf is never listed, so a query with fewer than kmax listable keys ends on (+inf, -1).
 * The distance of a pair is a function of the two rows alone (one fmaf chain over D in a fixed order): idx and dist are bitwise
 * equal for every split count and every query order or batching.  Exact f32 (f32-input MFMA), no floating-point atomics, 64-bit
 * row offsets.  Limits: D % 64 == 0, 1 <= kmax <= 32, kmax <= M < 2^31, 0 <= splits <= 64 (anything else: OCTIC_ESHAPE before
 * any launch; the caller checks that at least kmax keys are not skipped - the skip array lives on the device).
 * octic_seg_knn_plan: out[0] = key-axis splits of an automatic launch (1 once the query tiles fill the device), out[1] / out[2]
 * = query rows / keys per tile, out[3] = workspace class (0: the workspace is not read, 1: it holds the splits' partial lists).
 * octic_seg_knn_workspace_bytes: for `splits` as passed to octic_seg_knn (0 = the plan's); 256-byte aligned.
 * idx_* int32 / dist_* f32 are [n, kmax] with row stride ldo >= kmax, sorted; columns kmax .. ldo-1 are not written.  The pair
 * of a metric that is not asked for may be NULL.                                                                          */
int octic_seg_knn_plan(int64_t n, int64_t M, int D, int kmax, int metrics, int* out);
int64_t octic_seg_knn_workspace_bytes(int64_t n, int64_t M, int D, int kmax, int metrics, int splits);
int octic_seg_rownorms(const float* X, int64_t ldx, int64_t N, int D, float* norms, void* stream);
int octic_seg_knn(const float* Q, int64_t ldq, int64_t n, const float* K, int64_t ldk, int64_t M, int D, const float* qnorm,
                  const float* knorm, const uint8_t* skip, int kmax, int metrics, int splits, int32_t* idx_l2, float* dist_l2,
                  int32_t* idx_cos, float* dist_cos, int64_t ldo, void* workspace, void* stream);
/* The same search on rows of bf16 (the reference's `classifiers_kwargs: {knn: {dtype: bfloat16}}`, eval_config.yaml; the casts
 * of KNNClassifier._fit / _predict_batch, eval_segmentation.py:207, :248).  X, Q and K hold bf16 values the caller rounded ONCE
 * (round to nearest even, torch's cast); strides are in elements and rows are 16-byte aligned (ldx, ldq, ldk % 8 == 0).
 * Everything after that cast is f32: octic_seg_rownorms_bf16 sums the squares of the rounded values in f32 in a fixed order;
 * octic_seg_knn_bf16 forms the dot products on the bf16 MFMA (16x16x32) with f32 accumulation - one accumulator chain over D in
 * ascending channel order per pair - and then the SAME ordering keys, TOTAL ORDER, NaN and skip rules as octic_seg_knn; dist_*
 * are those f32 values.  Both distances come from the one pass: no second, normalised-then-rounded copy of the keys exists.
 * The list ordered by the f32 distance of the rounded operands is one valid answer to the reference's bf16 problem (whose
 * 8-bit distances tie in bulk, and torch.topk leaves ties open), and a reproducible one: bitwise equal for every split count
 * and every query order or batching.  Same limits, error codes, tiles, plan and workspace as octic_seg_knn:
 * octic_seg_knn_plan and octic_seg_knn_workspace_bytes answer for both element types.                                        */
int octic_seg_rownorms_bf16(const void* X, int64_t ldx, int64_t N, int D, float* norms, void* stream);
int octic_seg_knn_bf16(const void* Q, int64_t ldq, int64_t n, const void* K, int64_t ldk, int64_t M, int D, const float* qnorm,
                       const float* knorm, const uint8_t* skip, int kmax, int metrics, int splits, int32_t* idx_l2,
                       float* dist_l2, int32_t* idx_cos, float* dist_cos, int64_t ldo, void* workspace, void* stream);
/* out [nk, n, L] (uint8): out[i, r, l] = the most frequent of labels[idx[r, 0 .. ks[i]-1], l], the smallest value on a tie
 * (torch.mode), over the raw label values (an ignored value can win).  idx has row stride ldi; labels is [R, L] of esize-byte
 * integers (values 0 .. 255) and an index outside [0, R) casts no vote.  ks: HOST array of nk <= 8 ascending values 1 .. 32.  */
int octic_seg_knn_vote(const int32_t* idx, int64_t ldi, int64_t n, const void* labels, int esize, int64_t R, int L, const int* ks,
                       int nk, uint8_t* out, void* stream);

/* ---- the k-NN classification evaluation (KnnModule, dinov2/eval/knn.py:100-185) --------------------------------------------
 * octic_knn_topk: for each of n query rows Q [n, D] (row stride ldq) the kmax key rows of K [M, D] (row stride ldk) with the
 * LARGEST inner product (the reference's torch.mm + topk(max_k) on L2-normalised class tokens; nothing here normalises).  The
 * similarity matrix never reaches memory.
 * TOTAL ORDER: (similarity descending, key row index ascending): the larger similarity first, on equal similarity the lower
 * index.  torch.topk leaves ties open; this rule is ours, the mirror of octic_seg_knn's.  A NaN similarity counts as -inf; a
 * key at -inf is never listed, so a query with fewer than kmax listable keys ends on (-inf, -1).
 * The similarity of a pair is a function of the two rows alone (one fmaf chain over D in a fixed order, the channel order of
 * octic_seg_knn): idx and sim are bitwise equal for every split count and every query order or batching.  Exact f32 (f32-input
 * MFMA), no floating-point atomics, 64-bit row offsets.  Limits: D % 64 == 0, 1 <= kmax <= OCTIC_KNN_KMAX, kmax <= M < 2^31,
 * 0 <= splits <= 64 (anything else: OCTIC_ESHAPE before any launch).
 * octic_knn_topk_plan: out[0] = key-axis splits of an automatic launch (1 once the query tiles fill the device), out[1] / out[2]
 * = query rows / keys per tile, out[3] = workspace class (0: the workspace is not read, 1: it holds the splits' partial lists).
 * octic_knn_topk_workspace_bytes: for `splits` as passed to octic_knn_topk (0 = the plan's); 256-byte aligned.
 * idx int32 / sim f32 are [n, kmax] with row stride ldo >= kmax, sorted; columns kmax .. ldo-1 are not written.             */
#define OCTIC_KNN_KMAX 256
int octic_knn_topk_plan(int64_t n, int64_t M, int D, int kmax, int* out);
int64_t octic_knn_topk_workspace_bytes(int64_t n, int64_t M, int D, int kmax, int splits);
int octic_knn_topk(const float* Q, int64_t ldq, int64_t n, const float* K, int64_t ldk, int64_t M, int D, int kmax, int splits,
                   int32_t* idx, float* sim, int64_t ldo, void* workspace, void* stream);
/* The vote of KnnModule.forward (knn.py:179-184) on the lists above.  sim / idx are [n, kmax] (row stride ldi), labels DEVICE
 * int64 [M] (the class of every key row), C >= 5 classes, inv_T = 1 / temperature (positive, finite), ks a HOST array of nk <= 8
 * strictly ascending values in 1 .. kmax.  probas f32 [nk, n, C], every element written:
 *   probas[i, r, c] = sum over j < ks[i] with labels[idx[r, j]] == c of w[r, j],   w[r, :] = softmax(sim[r, :kmax] * inv_T)
 * The softmax runs over ALL kmax entries (max-subtracted, f32) and each k sums a prefix, so for k < kmax a row does not sum to 1.
 * Every sum runs in rank order j = 0, 1, ...; no floating-point atomics.  An entry with index outside [0, M) or with a label
 * outside [0, C) casts no vote (its weight is 0 in every sum over classes; its similarity still stands in the softmax's
 * denominator, where an unlisted entry's -inf adds nothing).
 * targets (nullable, DEVICE int64 [n]) with counters (DEVICE int64 [nk, 2]): the same launch ADDS, for each ks[i], the rows
 * whose target class ranks first / among the first five to counters[i, 0] / counters[i, 1] (integer atomics).  The class
 * ranking orders by proba descending, then class index ascending.  A target outside [0, C) counts no hit.                  */
int octic_knn_vote(const float* sim, const int32_t* idx, int64_t ldi, int64_t n, int kmax, const int64_t* labels, int64_t M,
                   int C, float inv_T, const int* ks, int nk, float* probas, const int64_t* targets, int64_t* counters,
                   void* stream);

/* ---- top-k accuracy counters of the evaluations (dinov2/eval/metrics.py; csrc/topk_metric.hip) ------------------------------
 * MulticlassAccuracy(average = micro | macro | none, top_k = k), ImageNetReaLAccuracy and the class mapping of
 * LinearPostprocessor (linear.py:219-230: preds[:, class_mapping]) on f32 score rows scores[g, r, :] - G groups of n rows of C
 * columns at scores + g ld_g + r ld_r (element strides, >= C where there is more than one row / group): the [classifiers, B, C]
 * logits of octic_probe_forward and the [nk, n, C] probas of octic_knn_vote both fit without a copy.
 * octic_topk_rank: class_map is a nullable DEVICE int32 [Cm] (NULL: identity, Cm must equal C); candidate j < Cm is class j with
 * score s_j = scores[g, r, class_map[j]].  The host cannot see the mapping: the caller guarantees entries in [0, C) (an entry
 * outside reads nothing and scores -inf).  targets is DEVICE int64 [n, A], 1 <= A <= OCTIC_TOPK_MAX_TARGETS, shared by all
 * groups; a value outside [0, Cm) is an undefined target (the reference pads with -1).  rank int32 [G, n, A], every element
 * written: for a defined target t the number of candidates that come before candidate t, for an undefined one Cm.
 *   order 0: j comes before t iff s_j > s_t                              (octic_probe_ce's rank: a tied target is a hit)
 *   order 1: j comes before t iff s_j > s_t or (s_j == s_t and j < t)    (octic_knn_vote's ranking: index ascending on ties)
 * A NaN score counts as -inf.  One wave per (group, row), one pass over the candidates for all A targets.
 * octic_topk_count ADDS the ranks of one update to DEVICE int64 counters (64-bit integer atomics: the counters do not depend on
 * the launch shape or on how the rows were split into calls).  ks: HOST array of nk <= 8 strictly ascending values >= 1.
 *   OCTIC_TOPK_ANY   counters [G, 1 + nk]:     [g, 0] += rows with at least one defined target, [g, 1 + i] += rows where some
 *                                              defined target has rank < ks[i]            (micro accuracy; ReaL with A > 1)
 *   OCTIC_TOPK_CLASS counters [G, Cm, 1 + nk]: A must be 1 and targets (the same [n]) is read again: [g, c, 0] += rows whose
 *                                              target is c, [g, c, 1 + i] += those of them with rank < ks[i]
 * Limits, refused with OCTIC_ESHAPE before any launch: G, n >= 1, G n A < 2^31, 1 <= C < 2^31, 1 <= Cm < 2^31, order 0 | 1,
 * strides as above; OCTIC_ENULL / OCTIC_EALIGN (4-byte scores, map and ranks, 8-byte targets and counters) likewise.          */
#define OCTIC_TOPK_MAX_TARGETS 32
#define OCTIC_TOPK_ANY 0
#define OCTIC_TOPK_CLASS 1
int octic_topk_rank(const float* scores, int64_t ld_g, int64_t ld_r, int64_t G, int64_t n, int64_t C, const int32_t* class_map,
                    int64_t Cm, const int64_t* targets, int A, int order, int32_t* rank, void* stream);
int octic_topk_count(const int32_t* rank, int64_t G, int64_t n, int A, int64_t Cm, const int64_t* targets, int mode, const int* ks,
                     int nk, int64_t* counters, void* stream);

/* ---- Mixup / CutMix and the BCE loss of the DeiT-III recipe (timm/data/mixup.py; deit/engine.py:47-59) -----------------
 * The host draws the per-sample parameters and uploads them as a DEVICE table of B rows; the kernels take everything about
 * the draw from it (never from arguments), so one captured launch serves every replay.  A row whose partner is outside
 * [0, B) or whose lam is outside [0, 1) means "not mixed".  f32 arithmetic, no atomics, fixed summation orders.          */
typedef struct {
  int32_t partner; /* the sample this one is mixed with (timm: B - 1 - i)                     */
  float lam;       /* weight of the sample itself; 1 = not mixed                              */
  int32_t cut;     /* != 0: CutMix (the box is pasted), 0: Mixup (the images are blended)     */
  int32_t yl, yh;  /* box rows    [yl, yh)                                                    */
  int32_t xl, xh;  /* box columns [xl, xh)                                                    */
  int32_t pad;
} octic_mix_row;
/* dst[i] (f32 [B, C, H, W], out of place) = src[partner] inside sample i's box, bit for bit; elsewhere src[i] bit for bit
 * when the row is a cut or lam == 1, else lam src[i] + (1 - lam) src[partner] (Mixup._mix_batch / _mix_elem / _mix_pair).
 * Any W: 16-byte accesses along W when W % 4 == 0 and both pointers are 16-byte aligned, element accesses otherwise; boxes
 * start and end at any column.  C H W < 2^31 - 4.  src and dst must not overlap (OCTIC_ESHAPE).                       */
int octic_mix_images(const float* src, float* dst, const octic_mix_row* table, int B, int C, int H, int W, void* stream);
/* targets [rows, num_classes] (f32, contiguous) for the batch rows row0 .. row0 + rows - 1 (mixup_target):
 * t = lam onehot(labels[b], on, off) + (1 - lam) onehot(labels[partner], on, off) with timm's three f32 roundings, and
 * t = (t > 0) when binarize != 0 (deit/engine.py:53-54).  labels: int64 [B] - partners are indexed in the WHOLE batch.  A
 * label outside [0, num_classes) gives an all-`off` one-hot row and is counted nowhere else.  rows <= 65535.            */
int octic_mix_targets(const int64_t* labels, const octic_mix_row* table, int B, int row0, int rows, int num_classes, float on,
                      float off, int binarize, float* targets, void* stream);
/* nn.BCEWithLogitsLoss(reduction="mean") of logits [rows, num_classes] (f32 or bf16, row stride ldl elements) against the
 * targets octic_mix_targets would write for the same arguments, without materialising them: per element
 * max(x, 0) - x t + log1p(exp(-|x|)) in f32, summed in f64 in a fixed order.  Each output is optional (not both NULL):
 * loss[0] (DEVICE f32) = the mean, needs workspace (rows doubles, 8-byte aligned);
 * dlogits (the logits' dtype, row stride ldd) = gscale[0] (sigmoid(x) - t) / (rows num_classes), gscale a DEVICE f32 (the
 * incoming gradient; NULL = 1).                                                                                      */
int octic_mix_bce(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B, int row0,
                  int rows, int num_classes, float on, float off, int binarize, float* loss, const float* gscale,
                  void* dlogits, int64_t ldd, void* workspace, void* stream);
/* The soft-target cross entropy of the reference loop without --bce-loss (timm's SoftTargetCrossEntropy, deit/main.py:372-374)
 * of logits [rows, num_classes] (f32 or bf16, row stride ldl >= num_classes) against the NON-binarised targets t that
 * octic_mix_targets would write for the same arguments, without materialising them; labels, table, B, row0, rows as for
 * octic_mix_bce.  With the identity table (partner = the row itself, lam = 1) and on = 1 - s + s / C, off = s / C it is timm's
 * LabelSmoothingCrossEntropy(s), at s = 0 nn.CrossEntropyLoss (main.py:375-378).  Per row, m = max x, se = sum expf(x - m),
 * S = sum t, and   row = S (m + log se) - sum t x:   the exponentials and targets in f32, the sums over the row and the row
 * value in f64 in a fixed order that depends on num_classes and the dtype only (not on ldl, alignment or rows) - so finite logits
 * of any size the dtype holds give a finite row value; a non-finite logit gives a non-finite loss.  Each output is optional (not both
 * NULL):  loss[0] (DEVICE f32) = the mean of the row values over rows, needs workspace (rows doubles, 8-byte aligned);
 * dlogits (the logits' dtype, row stride ldd) = gscale[0] (S expf(x - m) / se - t) / rows, gscale a DEVICE f32 (NULL = 1).
 * One workgroup per row.  num_classes >= 2, any value: up to 24576 the row is read from memory once and kept in registers (two
 * instantiations: up to 2048, up to 24576); above that every pass re-reads it (three reads, one for a loss-only or two for a
 * gradient-only call less).  16-byte accesses where the operand's base and row stride are multiples of 16 bytes, element
 * accesses otherwise and at a row's ragged end; nothing outside [row start, row start + num_classes) is touched.          */
int octic_mix_ce(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B, int row0,
                 int rows, int num_classes, float on, float off, float* loss, const float* gscale, void* dlogits, int64_t ldd,
                 void* workspace, void* stream);
/* The loss of --cosub (deit/engine.py:50-65): logits [2 rows, num_classes] (f32 or bf16, row stride ldl) - row r is the first
 * pass of batch sample row0 + r, row rows + r its second pass; a, b = the two halves.  With t as for octic_mix_bce (binarised when
 * binarize != 0) and bce(x, t) its per-element expression:
 *   loss[0] = 0.25 [ mean bce(a, t) + mean bce(b, t) + mean bce(a, sigmoid(b)) + mean bce(b, sigmoid(a)) ],
 * each mean over rows num_classes elements, the sigmoid targets constants (`.detach()`); f64 sums in a fixed order.
 *   dlogits [2 rows, num_classes] (row stride ldd): da = gscale[0] 0.25 / (rows num_classes) [ (sigmoid(a) - t) + (sigmoid(a) -
 *   sigmoid(b)) ], db its mirror image.
 * One launch reads both halves once and writes both gradients; exchanging the halves exchanges the gradients and keeps the loss,
 * bit for bit.  Outputs, gscale and workspace (rows doubles) as for octic_mix_bce.  num_classes >= 2.                     */
int octic_cosub_bce(const void* logits, int dtype, int64_t ldl, const int64_t* labels, const octic_mix_row* table, int B, int row0,
                    int rows, int num_classes, float on, float off, int binarize, float* loss, const float* gscale, void* dlogits,
                    int64_t ldd, void* workspace, void* stream);

/* ---- 3-Augment of the DeiT-III recipe on uint8 batches (deit/augment.py:90-123 behind the crop) ---------------------------
 * RandomHorizontalFlip, RandomChoice(grayscale, solarize, Gaussian blur), ColorJitter(brightness, contrast, saturation),
 * ToTensor and Normalize as one call on the decoded, cropped batch.  As for the mix the host draws the per-sample parameters
 * and uploads them as a DEVICE table of B rows; the kernels take everything about the draw from it.  A row whose op is not
 * 0..3, or a blur row whose box radius is not 0 or 1, gets no op; a jitter entry outside 0..2, or one that repeats an earlier
 * entry, is skipped.  The arithmetic is PIL's (Pillow's ImageOps / ImageFilter / ImageEnhance), rounding for rounding, with a
 * uint8 image between all stages:
 *   flip       x -> W-1-x
 *   grayscale  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in all three channels
 *   solarize   v < 128 ? v : 255 - v
 *   blur       three passes along x, then three along y, per channel, of
 *              out[x] = (ww sum_{|d| <= r} in[clamp(x+d)] + fw (in[clamp(x-r-1)] + in[clamp(x+r+1)]) + (1 << 23)) >> 24,
 *              clamp to the line.  The host computes the constants in FLOAT32, one rounding per operation, from the radius:
 *              s2 = radius radius / 3, L = sqrtf(12 s2 + 1), l = floorf((L - 1) / 2),
 *              a = (2l + 1)(l (l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)), fr = l + a; r = (int)fr,
 *              ww = (uint32)((float)(1 << 24) / (fr 2 + 1)), fw = ((1 << 24) - (2r + 1) ww) / 2.  radius <= 2 gives r <= 1.
 *   jitter     order[0..3] in turn: v = trunc(clip(deg + f (v - deg), 0, 255)) in f32, product and sum rounded separately;
 *              brightness: deg = 0; saturation: deg = the pixel's L; contrast: deg = (2 S + N) / (2 N) in integers, S = the sum
 *              of L over the whole image as it is at that point of the chain, N = H W
 *   output     (v / 255 - mean[c]) / std[c], two correctly rounded f32 divisions                                          */
typedef struct {
  int32_t flip;                            /* != 0: mirrored along x                                       */
  int32_t op;                              /* 0 none, 1 grayscale, 2 solarize, 3 Gaussian blur             */
  int32_t blur_r, blur_ww, blur_fw;        /* the box pass constants (op 3)                                */
  int32_t order[4];                        /* jitter ops in application order: 0 brightness, 1 contrast, 2 saturation, -1 skip */
  float brightness, contrast, saturation;  /* the blend factors                                            */
  int32_t pad[4];
} octic_aug_row;
/* bytes of the workspace of octic_augment_u8 (per-tile sums of L for the contrast op); OCTIC_ESHAPE for non-positive sizes */
int64_t octic_augment_workspace_bytes(int B, int H, int W);
/* src: uint8 [B, H, W, 3] (a decoder's layout, and PIL's), left untouched.  dst, by dtype_out: OCTIC_F32 - f32 [B, 3, H, W],
 * the normalised batch the model takes; OCTIC_U8 - uint8 [B, H, W, 3], the augmented pixels in front of ToTensor.  Any
 * H, W >= 1 with H W 3 < 2^31.  workspace: octic_augment_workspace_bytes(B, H, W) bytes, 4-byte aligned, always required (the
 * table decides on the device whether a sample has a contrast op).  src and dst must not overlap (OCTIC_ESHAPE).  Integer
 * sums only, no atomics: bitwise reproducible.                                                                         */
int octic_augment_u8(const uint8_t* src, void* dst, int dtype_out, const octic_aug_row* table, float mean0, float mean1,
                     float mean2, float std0, float std1, float std2, int B, int H, int W, void* workspace, void* stream);

/* ---- DINOv2's multi-crop augmentation on ragged uint8 images (dinov2/data/augmentations.py: DataAugmentationDINO) ---------
 * Bicubic RandomResizedCrop, RandomHorizontalFlip, RandomApply(ColorJitter with hue), RandomGrayscale, torchvision's
 * GaussianBlur(9), RandomSolarize, ToTensor and Normalize.  The host draws everything and uploads one row per crop (all crops
 * of one call have one output size) plus a pool of integer resampling coefficients; the kernels take everything about the
 * draw from them.  Apart from the blur the arithmetic is Pillow's, rounding for rounding, with a uint8 image between all stages:
 *   resize     img.crop(box).resize((S, S), BICUBIC), Pillow's 8-bit two-pass resample.  Per axis, crop length n: scale = n / S,
 *              fs = max(scale, 1), support = 2 fs, taps = 2 ceil(support) + 1; for output x: center = (x + 0.5) scale,
 *              xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), n),
 *              w_j = bicubic((j + xmin - center + 0.5) / fs), a = -0.5: ((a+2)t - (a+3)) t t + 1 for t < 1,
 *              (((t-5)t + 8)t - 4) a for t < 2; float64, normalised by their sum; k_j = (int)(w_j 2^22 +- 0.5), away from
 *              zero.  out = clamp((sum_j k_j p[xmin + j] + 2^21) >> 22, 0, 255) in int32.  Horizontal pass first, to uint8, the
 *              vertical pass on that.  A pass with n == S is the identity (the host gives it one tap of 2^22).  The HOST
 *              computes xmin, the count and k; per crop and axis the pool holds int32 bounds[S][2] = (xmin, count) and then
 *              k[S][taps] at the row's offset.  The kernels do integer sums only; bounds are clamped to the crop.
 *   flip       x -> S-1-x (on the resized crop)
 *   jitter     order[0..3] in turn; -1, an entry outside 0..3 or a repeated one is skipped.  0 brightness, 1 contrast,
 *              2 saturation: v = trunc(clip(deg + f (v - deg), 0, 255)) in f32, product and sum rounded separately, deg = 0,
 *              (2 S + N) / (2 N) in integers (S = the sum of L over the whole crop as it is at that point, N its pixels), the
 *              pixel's L.  3 hue: Pillow's convert("HSV"), H = (H + hue_shift) & 255, convert("RGB"), with
 *              RGB->HSV: V = max; max == min: H = S = 0; else in f32 cr = max - min, s = cr / max, rc, gc, bc = (max - c) / cr,
 *                h = bc - gc (f32) if r == max, else (float)(2.0 + rc - bc) if g == max, else (float)(4.0 + gc - rc) (double),
 *                h = (float)fmod(h / 6.0 + 1.0, 1.0) (double), H = clip8((int)(h 255.0)), S = clip8((int)(s 255.0)) (double)
 *              HSV->RGB: S == 0: grey V; else hf = (float)H 6.0 / 255.0 (double), i = floor(hf), f = (float)(hf - i),
 *                fs = (float)(S / 255.0), p = round(V (1 - fs)), q = round(V (1 - fs f)), t = round(V (1 - fs (1 - f))) in
 *                double with C round(), clip8; i % 6 selects (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q)
 *   grayscale  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in all three channels
 *   blur       torchvision's gaussian_blur(9, sigma) of a uint8 image: f32, reflect padding 4, the host's nine f32 weights
 *              blur_w (x = linspace(-4, 4, 9), pdf = exp(-0.5 (x / sigma)^2), pdf / pdf.sum(), all f32, computed as
 *              torchvision does).  Separable: a = 0, then a = fmaf(blur_w[j], p[x - 4 + j], a) for j = 0..8 along x, the f32
 *              results unrounded, the same along y over those, then rintf (half to even) and clip8.  (torchvision's own
 *              summation order is its convolution library's; the results agree wherever the exact sum is not within the f32
 *              accumulation error, about 1.2e-3, of a rounding tie.)
 *   solarize   v < 128 ? v : 255 - v
 *   output     (v / 255 - mean[c]) / std[c], two correctly rounded f32 divisions                                          */
typedef struct {
  int64_t src_offset;                      /* byte offset of the source image [src_h, src_w, 3] in `data`  */
  int32_t src_h, src_w;
  int32_t top, left, h, w;                 /* the crop box inside the source                               */
  int32_t flip;                            /* != 0: mirrored along x                                       */
  int32_t hcoef, htaps, vcoef, vtaps;      /* offsets (int32 words) of the two coefficient blocks in the pool, taps per output */
  int32_t order[4];                        /* ColorJitter's ops in application order: 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 skip */
  float brightness, contrast, saturation;  /* the blend factors                                            */
  int32_t hue_shift;                       /* (uint8)(int)(hue_factor 255)                                 */
  int32_t gray, blur, solarize;            /* != 0: applied                                                */
  float blur_w[9];                         /* the 1-D Gaussian weights (blur)                              */
  int32_t pad[7];
} octic_dino_row;                          /* 160 bytes */
/* HOST code, no launch: the coefficient block of one axis as stated above, crop length n -> S: bounds[S][2] and k[S][taps]
 * (unused taps 0).  taps must be 1 for n == S and 2 ceil(2 max(n / S, 1)) + 1 otherwise (at most 2048), else OCTIC_ESHAPE.   */
int octic_dino_resize_coeffs(int n, int S, int taps, int32_t* bounds, int32_t* k);
/* the most taps per output the resize kernel holds for output size S (its uint8 rows live in LDS); OCTIC_ESHAPE unless
 * 5 <= S <= 4096.  The host refuses sources whose 2 ceil(2 max(n / S, 1)) + 1 exceeds it.                               */
int octic_dino_resize_max_taps(int S);
/* crops [N, S, S, 3] (uint8) = the resized, flipped crops of the rows.  data: the uint8 source images back to back
 * (data_bytes in all), left untouched; coef: the pool (coef_len int32 words).  A row whose image, box or coefficient blocks do
 * not lie inside data / the source / the pool gives an all-zero crop.  rows 8-byte aligned.  Bitwise reproducible.        */
int octic_dino_resize_u8(const uint8_t* data, int64_t data_bytes, const octic_dino_row* rows, const int32_t* coef,
                         int64_t coef_len, int N, int S, uint8_t* crops, void* stream);
/* bytes of the workspace of octic_dino_color_u8 (per-tile sums of L, and the jittered uint8 crops); OCTIC_ESHAPE for N < 1,
 * H or W < 5 (the blur's reflect padding) or H W 3 >= 2^31                                                                */
int64_t octic_dino_color_workspace_bytes(int N, int H, int W);
/* The chain behind the resize and flip on uint8 crops [N, H, W, 3], left untouched: jitter, grayscale, blur, solarize, output.
 * The geometry fields of the rows are not read.  dst, by dtype_out: OCTIC_F32 - f32 [N, 3, H, W], normalised; OCTIC_U8 - uint8
 * [N, H, W, 3], the pixels in front of ToTensor.  crops, dst and workspace must not overlap (OCTIC_ESHAPE).  Integer sums
 * across pixels, no atomics: bitwise reproducible, and independent of a crop's place in the batch.                        */
int octic_dino_color_u8(const uint8_t* crops, void* dst, int dtype_out, const octic_dino_row* rows, float mean0, float mean1,
                        float mean2, float std0, float std1, float std2, int N, int H, int W, void* workspace, void* stream);

/* ---- the DeiT-III crops and evaluation resize on ragged uint8 images (deit/augment.py:90-108, deit/datasets.py:91-132) -------
 * timm's RandomResizedCropAndInterpolation(bicubic), the --src crop (Resize + RandomCrop(padding, reflect)), the evaluation
 * transform (Resize(bicubic) + CenterCrop) and the quarter turns / mirror of --rot-eval / --flop-eval, as ONE windowed resample:
 * an OH x OW window of the reflect-padded, resized box of a source, turned and mirrored.  The host draws everything and uploads
 * one row per output image plus the coefficient pool of octic_dino_resize_coeffs (a block per image and axis, w -> rw and
 * h -> rh, layout as above).  Output pixel (y, x) of image n:
 *   orientation  undo the mirror (flip != 0: x -> OW-1-x), then the rot quarter turns COUNTER-CLOCKWISE, to get the position
 *                (wy, wx) in the window: rot 0 (y, x); 1 (x, OH-1-y); 2 (OH-1-y, OW-1-x); 3 (OW-1-x, y).  This is
 *                ImageOps.mirror(img.rotate(90 rot)) of Pillow (rotate turns counter-clockwise and takes its exact transpose
 *                path for quarter turns of a square image; checked against Pillow 12), numpy.rot90(window, rot)[:, ::-1].
 *                rot 1 and 3 need OH == OW.
 *   window       (ry, rx) = (win_top + wy - pad, win_left + wx - pad), reflected into [0, rh) x [0, rw) as
 *                numpy.pad(mode="reflect") does: i < 0 -> -i, i >= n -> 2 (n - 1) - i (no edge repeat; pad < min(rh, rw)).
 *   resize       pixel (ry, rx) of img.crop(box).resize((rw, rh), BICUBIC): Pillow's 8-bit two-pass resample exactly as stated
 *                for octic_dino_resize_u8 - horizontal pass to uint8, the vertical pass on that, a pass of equal lengths the
 *                identity.  Only the resized rows and columns the window touches are computed.  The products k_j p run on
 *                the 24-bit multiplier: exact for |k_j| < 2^23, which Pillow's coefficients (at most 2^22 (1 + the side lobes))
 *                are; the host checks it.
 *   output       OCTIC_U8: the pixel; OCTIC_F32: (v / 255 - mean[c]) / std[c], two correctly rounded f32 divisions          */
typedef struct {                           /* one output image; 8-byte aligned, 80 bytes                   */
  int64_t src_offset;                      /* byte offset of the source image [src_h, src_w, 3] in `data`  */
  int32_t src_h, src_w;
  int32_t top, left, h, w;                 /* the box that is resampled                                    */
  int32_t rh, rw;                          /* the size the box is resampled to                             */
  int32_t pad;                             /* reflect padding round the resized image                      */
  int32_t win_top, win_left;               /* the OH x OW window in the padded resized image               */
  int32_t rot, flip;                       /* rot in 0..3: quarter turns counter-clockwise, then (flip != 0) mirrored along x */
  int32_t hcoef, htaps, vcoef, vtaps;      /* offsets (int32 words) of the two coefficient blocks in the pool (w -> rw: bounds[rw][2],
                                              k[rw][htaps]; h -> rh likewise), taps per output               */
  int32_t reserved;
} octic_crop_row;
/* the most taps per output of the VERTICAL pass the kernel holds for windows OW wide (its uint8 rows live in LDS);
 * OCTIC_ESHAPE unless 5 <= OW <= 4096.  The host refuses boxes whose 2 ceil(2 max(h / rh, 1)) + 1 exceeds it.             */
int octic_crop_resize_max_taps(int OW);
/* window rows per workgroup of octic_crop_resize_u8 (what its tests put their output heights around)                        */
int octic_crop_resize_rows(void);
/* dst, by dtype_out: OCTIC_U8 - uint8 [N, OH, OW, 3]; OCTIC_F32 - f32 [N, 3, OH, OW], normalised.  data: the uint8 source
 * images back to back (data_bytes in all), left untouched; coef: the pool (coef_len int32 words).  5 <= OH, OW <= 4096.  A row
 * whose source, box, coefficient blocks or window do not lie inside data / the source / the pool / the padded resized image,
 * whose rot is outside 0..3 (or odd with OH != OW) or whose pad is negative or >= min(rh, rw) gives an all-zero image (f32: 0.0),
 * never a stray access; every bound read from the pool is clamped.  rows 8-byte aligned; data and dst must not overlap
 * (OCTIC_ESHAPE).  Integer sums only, no atomics: bitwise reproducible, and independent of an image's place in the batch.  */
int octic_crop_resize_u8(const uint8_t* data, int64_t data_bytes, const octic_crop_row* rows, const int32_t* coef,
                         int64_t coef_len, int N, int OH, int OW, void* dst, int dtype_out, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, void* stream);

/* ---- linear depth head of the DINOv2 hub (dinov2/hub/depthers.py:36-67; hub/depth/decode_heads.py: BNHead, depth_pred;
 *      csrc/depth.hip) -------------------------------------------------------------------------------------------------
 * The reference upsamples the [patch | class token] channels of 1 or 4 layers u = 4 times and projects the large tensor to
 * 256 bins.  Projection and bilinear resize commute and the class-token half is one bias vector per image, so the engine
 * projects at patch resolution (octic_depth_logits) and resizes, normalises and takes the expectation in one pass
 * (octic_depth_expect); neither the concatenated nor the upsampled tensor exists.
 * Limits (octic_depth_ok / octic_depth_plan are the only place they live): D % 64 == 0, 64 <= D <= 4096, layers 1 .. 4,
 * n_bins == 256, upsample 1 | 2 | 4 (the scale is exact in f32), B, h, w >= 1, h w upsample^2 < 2^31, fewer than 2^31
 * workgroups.  Strides are multiples of 4 floats, operand rows 16-byte aligned.  OCTIC_ENULL, OCTIC_ESHAPE and OCTIC_EALIGN are
 * returned before any launch.  All offsets are 64-bit.  No atomics: results are bitwise reproducible and an image's map does
 * not depend on its batch mates or its place in the batch.
 * octic_depth_ok: 1 where the kernels take (D, layers, n_bins, upsample), else 0.
 * octic_depth_plan: out[0] = patch rows per workgroup of the logits launch (a workgroup never leaves its image), out[1] = its
 * workgroups = B ceil(h w / out[0]), out[2] = summation chains per logit = layers D / 64, out[3] = workgroups of the
 * expectation launch.  OCTIC_ESHAPE exactly where the launchers refuse by shape.                                            */
int octic_depth_ok(int D, int layers, int n_bins, int upsample);
int octic_depth_plan(int64_t B, int h, int w, int D, int layers, int n_bins, int upsample, int out[4]);
/* Lo [B, h w, 256] dense f32: Lo[b, p, k] = sum_l patch_l[b, p, :] . W[k, 2 D l : 2 D l + D]
 *                                          + (bias[k] + sum_l cls_l[b, :] . W[k, 2 D l + D : 2 D l + 2 D]).
 * patch / patch_ldb / patch_ldr / cls / cls_ldb: HOST arrays of `layers` entries - the patch-token rows of layer l start at
 * patch[l], image b at + b patch_ldb[l], row p at + p patch_ldr[l] floats (>= D); the class token of image b at
 * cls[l] + b cls_ldb[l]: the views out[:, 1 + R:] and out[:, 0] of a [B, T, D] block output, read in place.  W: DEVICE f32
 * [256, 2 D layers] contiguous in the reference's channel order (per layer the patch half, then the class-token half);
 * bias DEVICE f32 [256]; image_bias: DEVICE f32 [B, 256] workspace, on return the per-image term in brackets above.
 * Arithmetic contract (exact-f32 MFMA = fmaf): the per-image term is 64 fmaf chains - chain i takes the column quads
 * 4 i + 256 j (j ascending) of layer 0, then of layer 1, ... - added by a butterfly over offsets 32, 16, 8, 4, 2, 1, plus
 * bias[k]; a logit is layers D / 64 fmaf chains of 64 consecutive columns, each started from zero, added in ascending
 * (layer, column) order to a zero accumulator, plus the per-image term.  Both orders depend on (layers, D) alone.           */
int octic_depth_logits(const float* const* patch, const int64_t* patch_ldb, const int64_t* patch_ldr, const float* const* cls,
                       const int64_t* cls_ldb, int layers, int64_t B, int h, int w, int D, const float* W, const float* bias,
                       int n_bins, float* image_bias, float* Lo, void* stream);
/* depth [B, upsample h, upsample w] f32 from Lo: per output pixel the up-to-four source cells under torch's
 * upsample_bilinear2d weights for align_corners = False (src = (dst + 0.5) / upsample - 0.5 clamped below at 0,
 * i0 = floor(src), i1 = min(i0 + 1, n - 1), upper weight src - i0; horizontal pairs first, then the vertical pair), per bin
 * z = (v < 0 ? 0 : v) + 0.1f (NaN stays NaN, as torch.relu), depth = sum_k bins[k] z_k / sum_k z_k clamped to
 * [min_depth, max_depth] (NaN passes, as torch.clamp).  bins: DEVICE f32 [256], 16-byte aligned (the host's torch.linspace).
 * Sums: lane i adds bins 4 i .. 4 i + 3 in order, the 64 lane sums by a butterfly over offsets 32 .. 1.                     */
int octic_depth_expect(const float* Lo, int64_t B, int h, int w, int n_bins, int upsample, const float* bins, float min_depth,
                       float max_depth, float* depth, void* stream);

/* ---- orbit invariants: MaxFilteringInvariant / CanonizationInvariant (d8_invariantization.py:142-280) -----------------------
 * The eight action matrices of D8 on the 8-tuple are signed permutations that touch 12 (i, j) pairs, so the eight products
 * of a (row, reference) pair are signed sums of 12 dot products of length c (the 8 E dots pair up into 4 of length 2c).
 * dtype is the operand dtype of x / dx / planes / g (OCTIC_BF16: bf16 MFMA; OCTIC_F32: exact-f32 MFMA); partials, signed
 * sums and comparisons are f32.  Group order e, r, rr, rrr, m, mr, mrr, mrrr; the winner is the lowest index among equal
 * products and the first NaN product.  No address behind row M - 1, reference R - 1 or column c - 1 is read.
 * Nothing of M x 8 x R or M x 8 x 8c elements is written anywhere.                                                          */
/* references [R, c, 8] f32 (component innermost) -> planes [8][R][c] in dtype (R c 8 elements, 16-byte aligned). */
int octic_max_filter_prep(const float* references, void* planes, int64_t R, int c, int dtype, void* stream);
/* out [M, R] dense (out_dtype) = max_g, idx [M, R] uint8 = argmax_g of x[t] . (A_g references[d]). */
int octic_max_filter_fwd(const octic_view* x, const void* planes, void* out, uint8_t* idx, int64_t M, int64_t R, int c, int dtype,
                         int out_dtype, void* stream);
/* dx_i[t, :] = sum_j sum_d (g[t, d] A_idx[t, d][i, j]) ref_j[d, :]; g [M, R] dense in dtype (16-byte aligned), idx 8-byte aligned. */
int octic_max_filter_bwd_x(const void* g, const uint8_t* idx, const void* planes, const octic_view* dx, int64_t M, int64_t R, int c,
                           int dtype, void* stream);
/* The row slabs of octic_max_filter_bwd_ref, a function of (M, R, c) alone: out = {slabs, rows per slab, tile edge, workgroups per slab}. */
int octic_max_filter_bwd_ref_plan(int64_t M, int64_t R, int c, int out[4]);
int64_t octic_max_filter_bwd_ref_workspace_bytes(int64_t M, int64_t R, int c);
/* dref [R, c, 8] f32: dref_j[d, :] = sum_i sum_t (g[t, d] A_idx[t, d][i, j]) x_i[t, :].  f32 partials per row slab in the
 * workspace, then summed in slab order; no atomics. */
int octic_max_filter_bwd_ref(const void* g, const uint8_t* idx, const octic_view* x, float* dref, void* workspace,
                             int64_t workspace_bytes, int64_t M, int64_t R, int c, int dtype, void* stream);
/* reference [8c] f32, i-major.  idx [M] uint8 = argmax_g of reference . (A_g x[t]); out [M, 8c] dense (out_dtype), i-major
 * [x'0 | ... | x'7] = A_idx x[t]: a signed copy of the row's values.  One wave per row. */
int octic_canonize_fwd(const octic_view* x, const float* reference, void* out, uint8_t* idx, int64_t M, int c, int dtype,
                       int out_dtype, void* stream);
/* dx = the inverse signed permutation of g [M, 8c] dense (g_dtype). */
int octic_canonize_bwd(const void* g, int g_dtype, const uint8_t* idx, const octic_view* dx, int64_t M, int c, int dtype,
                       void* stream);

/* ---- polynomial invariants: PolynomialInvariant / ThirdOrderInvariant (d8_invariantization.py:66-141) ----------------------
 * Element-wise over (row, column).  x, dx: float32 views.  out / g: dense [M, P c], generator k at columns [k c, (k + 1) c),
 * P = 32 (OCTIC_POLY_POLYNOMIAL) or 15 (OCTIC_POLY_THIRD_ORDER), in the plane order of the Python modules; 16-byte aligned.
 * Forward: every generator in f32 with the expression tree of the Python composition (monomials as left-to-right products of
 * their digits, terms in table order, every multiply and add rounded on its own: no fma), so the f32 output equals the
 * composition bit for bit and the bf16 output is its round-to-nearest-even.
 * Backward: dx_i = sum_k g_k dp_k/dx_i recomputed from x; f32 sums in a fixed order (generators in plane order, terms in table
 * order, the distinct digits of a term in order of first appearance); no atomics, no workspace.
 * One thread per group of 4 (forward) / 2 (backward) adjacent columns of a row in an uncapped grid: M c / 2 must stay below
 * 2^31 (else -1).                                                                                                          */
enum { OCTIC_POLY_POLYNOMIAL = 0, OCTIC_POLY_THIRD_ORDER = 1 };
int octic_poly_invariant_fwd(const octic_view* x, void* out, int64_t M, int c, int map, int out_dtype, void* stream);
int octic_poly_invariant_bwd(const void* g, int g_dtype, const octic_view* x, const octic_view* dx, int64_t M, int c, int map,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCTIC_HIP_H */
