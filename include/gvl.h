/*
 * gvl.h — C-ABI of libgvl, the MI355X (gfx950) kernel library behind the
 * gpt2-vision-language drop-in modules.
 *
 * The reference (theophile-lt/gpt2-vision-language) is pure Python/PyTorch: its
 * operator boundary is the ATen op set its nn.Modules call.  Each
 * entry point below replaces one or more of those ATen calls; the reference call
 * site it stands in for is cited as file:line into /root/reference.
 *
 * Conventions (all entry points):
 *   - plain device pointers + int64 sizes/strides (in ELEMENTS), no torch types;
 *   - bf16 tensors are raw 16-bit words; fp32 where stated;
 *   - `stream` is a hipStream_t (the caller's torch.cuda.current_stream());
 *   - return 0 on success, -1 on a rejected argument (shape/alignment),
 *     -2 on a HIP launch error; gvl_last_error() returns the thread-local text;
 *   - the library allocates nothing: every buffer and workspace is owned by the
 *     caller (sizes from the *_workspace_size queries); no entry point
 *     synchronises the device, so every call is capturable into a hipGraph.
 */
#ifndef GVL_H_
#define GVL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVL_ABI_VERSION 14

/* Dropout seeds: every dropout mask is rng(seed_eff, element index) with
 * seed_eff = seed when seed_ptr is NULL or *seed_ptr == 0, else seed ^ mix64(*seed_ptr).
 * A training step captured into a hipGraph keeps its host seeds frozen; advancing the
 * device-side offset once per replay gives every step fresh masks (forward and backward
 * of one step read the same offset, so they agree). */

typedef void* gvl_stream_t;

const char* gvl_last_error(void);
int gvl_abi_version(void);
/* Measurement hook (bench.py roofline): arm a (start, stop) pair of timing-enabled
 * hipEvent_t for the calling thread; the main kernel of the next gvl_gemm / gvl_attn_fwd /
 * gvl_attn_bwd call on this thread is launched with hipExtLaunchKernelGGL bound to them, so
 * hipEventElapsedTime gives that kernel's execution time as its dispatch records it.  Not
 * for use under hipGraph capture. */
int gvl_set_launch_events(void* start, void* stop);

/* ------------------------------------------------------------------------- */
/* GEMM on bf16 MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate, fused epilogue.
 *   C[m][n] = epi( alpha * sum_k opA[m][k] * opB[k][n] )
 *   opA: a_mn=0 -> A stored [M][K] (row stride lda);  a_mn=1 -> A stored [K][M].
 *   opB: b_mn=0 -> B stored [N][K] (nn.Linear weight); b_mn=1 -> B stored [K][N].
 * Epilogue order: *alpha_ptr, +bias[n], *dgelu(pre_in), {pre_out=v; v=gelu(v)},
 *   (with gate and no act, pre_out receives the un-gated branch),
 *   dropout(p, seed, index m*N+n), *tanh(*gate), +residual, store (bf16 or fp32).
 * Replaces: nn.Linear forward/backward (addmm/mm) at source/gpt2/train_gpt2.py:26-27,
 *   50-58,96-97; gpt2_linear/model.py:125-129,172; gpt2_cross-att/model.py:39-41,81;
 *   gpt2_q_former/model.py:119-130,151 and the gelu/dropout/residual adds around them. */
typedef struct gvl_gemm_desc {
  const void* a;
  const void* b;
  void* c;
  int64_t m, n, k;
  int64_t lda, ldb, ldc;
  int32_t a_mn, b_mn;
  float alpha;
  const float* alpha_ptr; /* optional fp32 device scalar multiplied into alpha */
  const void* bias;       /* optional bf16 [N] */
  int32_t act;            /* 0 none, 1 gelu-tanh, 2 gelu-erf (pre_out <- x);
                             3 gelu-tanh, 4 gelu-erf with pre_out <- gelu'(x) (ABI v4);
                             5 quick-GELU x sigmoid(1.702 x), needs bias, no pre_out, no dact
                             (ABI v14: the frozen CLIP tower's fc1, gvl/clip.py) */
  int32_t dact;           /* 0 none, 1 dgelu-tanh, 2 dgelu-erf (of pre_in = x);
                             3: multiply by pre_in = gelu'(x) as stored by act 3/4 (ABI v4) */
  void* pre_out;          /* optional bf16 [M][ldp]: value before activation */
  const void* pre_in;     /* bf16 [M][ldp]: pre-activation for dact */
  int64_t ldp;
  const void* residual;   /* optional bf16 [M][ldr], may alias c */
  int64_t ldr;
  const void* gate;       /* optional bf16 scalar g: branch *= tanh(g) */
  float drop_p;           /* dropout probability on the branch (0 = off) */
  uint64_t seed;
  int32_t c_fp32;         /* 1: C is fp32 */
  void* workspace;        /* optional fp32 scratch for split-K (few output tiles, long K) */
  int64_t workspace_bytes;
  const uint64_t* seed_ptr; /* optional device step offset re-keying `seed` (see below) */
  /* ABI v5: optional arrival tickets for the in-launch two-way split-K combine (the two
   * K-halves of an output tile meet inside one launch; no separate reduce kernel).  The
   * caller allocates them zero-filled once; every call leaves them zero again.  Needs
   * ticket_count >= 8 * output tiles of the split GEMM; fewer -> the two-kernel path. */
  uint32_t* tickets;
  int64_t ticket_count;
} gvl_gemm_desc;
int gvl_gemm(const gvl_gemm_desc* d, gvl_stream_t stream);
/* count (<= 16) GEMMs of one shape and layout that differ only in a, b, c (and residual,
 * which is null for all or equal to c for all: C += AB) as ONE persistent launch: the
 * weight gradients of the 12 GPT-2 blocks of a micro-step (source/gpt2/train_gpt2.py:471,
 * loss.backward() -> the nn.Linear weight grads of every Block), each of which alone is too
 * few output tiles to fill the chip.  Other epilogues / shapes run one by one. */
int gvl_gemm_batched(const gvl_gemm_desc* d, int32_t count, gvl_stream_t stream);
/* As gvl_gemm_batched for weight gradients (a_mn = b_mn = 1, residual == c) that also add
 * each problem's bias gradient: dbias[i] (bf16 [m]) += row sums of A_i^T over k, i.e. the
 * column sums of dY — the nn.Linear bias grad beside its weight grad, computed from the same
 * operand tiles (no second pass over dY).  Returns -1 when the batch cannot run fused and
 * nothing was launched (the caller then uses gvl_gemm_batched + gvl_colsum_batched); any other
 * non-zero return is a launch failure after the GEMM may have added into C (fatal). */
int gvl_gemm_batched_dbias(const gvl_gemm_desc* d, void* const* dbias, int32_t count,
                           gvl_stream_t stream);
/* ABI v9: weight gradients of DIFFERENT shapes in one launch — the Q-Former bridge's deferred
 * nn.Linear weight grads of one backward (source/gpt2_q_former/model.py:114-168, the
 * out_proj / MLP Linears' grads that loss.backward() produces, each too few output tiles to
 * fill the chip alone): each problem a_mn = b_mn = 1, residual == c (C += dY^T X), the same
 * alpha; dbias[i] (bf16 [m], may be null; the array may be null) += column sums of dY_i.
 * count <= 48 (round 4: also every GPT-2 block's four weight grads of one LM backward flush,
 * train_gpt2.py:55-59,71-74, sizes and strides < 2^30).
 * ABI v11: a problem's alpha_ptr may be set (the tied lm_head's weight grad, scaled by the
 * device scalar dloss / count, train_gpt2.py:469 + the reference's loss scaling): every non-null
 * alpha_ptr of one call must be the same pointer; those problems get alpha * *alpha_ptr, the
 * others alpha.
 * Returns 0 when launched, -1 when the problems do not qualify and nothing was launched. */
int gvl_gemm_grouped(const gvl_gemm_desc* d, void* const* dbias, int32_t count,
                     gvl_stream_t stream);
/* Process-wide GEMM implementation knob (benchmarking / A-B tests):
 * impl 3 (default) = persistent ping-pong 256x256 kernel (split-K for few tiles) where
 * the work items fill the chip, else the 128x128 LDS-DMA ring; 2 = ring / non-persistent
 * ping-pong family; 1 = LDS-DMA v2 (K % 64 == 0); 0 = register-staged kernel always.
 * cfg -1 = pick by shape; otherwise forces a tile config of the family (impl 2: 0 = 256x256,
 * 1 = 256x128, 2 = 128x128, 3 = 256x256/5 slots, 4/5 = ping-pong, 6 = 64x128); impl 3:
 * cfg 3 forces the persistent kernel, 10 the four-wave narrow-output kernels (192x128 /
 * 128x128 tiles, direct-A where K % 384 == 0) where they apply, 11 = default routing without
 * them (and without the AGPR four-wave kernel), 12 (ABI v8, round 4) the AGPR four-wave kernel
 * (gemm_w4x.hip: 256 x 192 / 128 x 192 tiles, K-contiguous A, plain or bias + residual) where
 * it applies; 13 (ABI v10) = cfg 11 with the persistent kernel's in-launch two-way combine
 * enabled for single GEMMs (tests; otherwise never, since the callers' tickets are passed
 * to every gvl_gemm by gvl.kernels); other cfg values route as -1.  impl 4 (the removed 64-deep quadrant-phase
 * kernel) is rejected. */
int gvl_gemm_tune(int32_t impl, int32_t cfg);
/* Name of the kernel template instance gvl_gemm would launch for d (profiling: lets a
 * caller attribute event timings to the rocprofv3 kernel-trace rows). */
int gvl_gemm_kernel_name(const gvl_gemm_desc* d, char* buf, int32_t len);
/* ABI v7: name of the kernel instance the calling thread's last gvl_gemm_batched /
 * gvl_gemm_batched_dbias call launched as one batched launch ("" when it ran the problems one
 * by one through gvl_gemm): the bench attributes the batched weight-gradient launches too. */
int gvl_gemm_batched_kernel_name(char* buf, int32_t len);
/* (ABI v8-v9 had gvl_gemm_lib_route: plain N = 768 GEMMs handed to hipBLASLt.  Removed in
 * ABI v10: every GEMM runs on libgvl's own kernels; libgvl links no vendor BLAS.) */

/* ------------------------------------------------------------------------- */
/* LayerNorm over the last dim (eps given; reference uses 1e-5).
 * Replaces nn.LayerNorm at source/gpt2/train_gpt2.py:66,68,94 (ln_1/ln_2/ln_f),
 * gpt2_cross-att/model.py:91 (ln_x), gpt2_q_former/model.py:118-125. */
int gvl_layernorm_fwd(const void* x, int64_t ldx, const void* w, const void* b,
                      void* y, int64_t ldy, float* mean, float* rstd,
                      int64_t rows, int64_t cols, float eps, gvl_stream_t stream);
/* dx (bf16) = LN'(dy); if accumulate_dx, dx += result (residual-stream grad).
 * dw/db (bf16, optional) get column sums; they need workspace
 * gvl_layernorm_bwd_workspace_size(rows, cols) bytes. accumulate_wb adds into dw/db. */
int64_t gvl_layernorm_bwd_workspace_size(int64_t rows, int64_t cols);
int gvl_layernorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx,
                      const void* w, const float* mean, const float* rstd,
                      void* dx, int64_t lddx, int32_t accumulate_dx,
                      void* dw, void* db, int32_t accumulate_wb, void* workspace,
                      int64_t rows, int64_t cols, gvl_stream_t stream);
/* ABI v12: accumulate_wb bit 1 (value 2 | accumulate) defers the dw / db column sums: the
 * per-block partials stay in `workspace` (gvl_layernorm_bwd_blocks(rows) blocks of 2 * cols
 * floats) and dw / db are left untouched; one gvl_layernorm_bwd_finalize_batched launch later
 * reduces up to 64 such workspaces of one width into their dw[i] / db[i] (either may be null),
 * adding into them when accumulate_wb bit 0 is set — the end-of-backward flush of every
 * LayerNorm weight grad of a GPT-2 micro-step (train_gpt2.py:66,68,94) in one launch instead
 * of 25. */
int32_t gvl_layernorm_bwd_blocks(int64_t rows);
int gvl_layernorm_bwd_finalize_batched(const float* const* ws, const int32_t* nblk, int32_t count,
                                       int64_t cols, void* const* dw, void* const* db,
                                       int32_t accumulate_wb, gvl_stream_t stream);
/* dx = res + LayerNorm backward (the residual-stream gradient of a pre-LN block:
 * source/gpt2/train_gpt2.py:72-73, x + attn(ln_1(x)) / x + mlp(ln_2(x))) with the residual
 * read from its own buffer, so the caller needs no copy of it; otherwise as above. */
int gvl_layernorm_bwd_res(const void* dy, int64_t lddy, const void* x, int64_t ldx,
                          const void* w, const float* mean, const float* rstd,
                          const void* res, int64_t ldr, void* dx, int64_t lddx,
                          void* dw, void* db, int32_t accumulate_wb, void* workspace,
                          int64_t rows, int64_t cols, gvl_stream_t stream);
/* Wide rows: 1024 < cols <= 2048, cols % 8 == 0 (GPT-2 large / XL, n_embd 1280 / 1600); the
 * entry points above keep their cols <= 1024 contract and refuse these widths.  Same leading-
 * dimension and alignment rules, same outputs, same workspace size and block count
 * (gvl_layernorm_bwd_workspace_size / gvl_layernorm_bwd_blocks serve both).
 * gvl_layernorm_fwd_wide: gvl_layernorm_fwd's arguments (mean / rstd optional).
 * gvl_layernorm_bwd_wide: one entry for gvl_layernorm_bwd and gvl_layernorm_bwd_res: with
 * accumulate_dx set, dx = res + LN'(dy), where res is a separate operand, dx itself, or null
 * (= dx); with it clear res is not read.  accumulate_wb as above, bit 1 included.
 * gvl_layernorm_bwd_finalize_batched_wide: gvl_layernorm_bwd_finalize_batched for the
 * partials of gvl_layernorm_bwd_wide. */
int gvl_layernorm_fwd_wide(const void* x, int64_t ldx, const void* w, const void* b,
                           void* y, int64_t ldy, float* mean, float* rstd,
                           int64_t rows, int64_t cols, float eps, gvl_stream_t stream);
int gvl_layernorm_bwd_wide(const void* dy, int64_t lddy, const void* x, int64_t ldx,
                           const void* w, const float* mean, const float* rstd,
                           const void* res, int64_t ldr, void* dx, int64_t lddx,
                           int32_t accumulate_dx, void* dw, void* db, int32_t accumulate_wb,
                           void* workspace, int64_t rows, int64_t cols, gvl_stream_t stream);
int gvl_layernorm_bwd_finalize_batched_wide(const float* const* ws, const int32_t* nblk,
                                            int32_t count, int64_t cols, void* const* dw,
                                            void* const* db, int32_t accumulate_wb,
                                            gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Fused attention, head dim 64, bf16 in/out, fp32 online softmax.
 * q/k/v/o element (b,t,h,d) at ptr + b*s_b + t*s_t + h*s_h + d, so the packed
 * c_attn output [B,T,3C] is consumed in place and o is written as [B,T,C]
 * (the transpose(1,2).contiguous() of the reference is fused away).
 * Replaces F.scaled_dot_product_attention at source/gpt2/train_gpt2.py:40 (causal),
 * gpt2_cross-att/model.py:55 (non-causal bridge cross-attention) and the
 * nn.MultiheadAttention core at gpt2_q_former/model.py:135,140 (attention-prob
 * dropout p; need_weights output is discarded by the reference and not produced). */
typedef struct gvl_attn_desc {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse; /* fp32 [B][H][Tq], natural-log row logsumexp of scale*q.k */
  int64_t B, H, Tq, Tk;
  int64_t q_sb, q_st, q_sh;
  int64_t k_sb, k_st, k_sh;
  int64_t v_sb, v_st, v_sh;
  int64_t o_sb, o_st, o_sh;
  int32_t causal;
  float scale;
  float drop_p;
  uint64_t seed;
  const uint64_t* seed_ptr; /* optional device step offset re-keying `seed` */
} gvl_attn_desc;
int gvl_attn_fwd(const gvl_attn_desc* d, gvl_stream_t stream);
/* Backward: dO has the layout of o (do_* strides); dq/dk/dv the layouts of q/k/v
 * (dq_*, dk_*, dv_* strides).  workspace: gvl_attn_bwd_workspace_size bytes. */
typedef struct gvl_attn_bwd_desc {
  const void* dout;
  int64_t do_sb, do_st, do_sh;
  void* dq;
  int64_t dq_sb, dq_st, dq_sh;
  void* dk;
  int64_t dk_sb, dk_st, dk_sh;
  void* dv;
  int64_t dv_sb, dv_st, dv_sh;
  void* workspace;
} gvl_attn_bwd_desc;
int64_t gvl_attn_bwd_workspace_size(const gvl_attn_desc* d);
int gvl_attn_bwd(const gvl_attn_desc* d, const gvl_attn_bwd_desc* g, gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Row-wise cross-entropy over bf16 logits (fp32 math), fused softmax gradient.
 * Logits row for target r: (r / rows_per_group) * group_stride + row_offset + r % rows_per_group
 * (lets the caption loss read logits[:, M:M+T] in place).  targets int64 with
 * ignore_index=-100; optional uint8 mask weights rows (cross-att masked mean).
 * `vocab` need not be a multiple of 8 (GPTConfig()'s 50257): ldl / ldd are multiples of 8
 * >= vocab rounded up to 8, and the pad columns read as -inf and get dlogits 0.  A
 * target outside [0, vocab) (other than -100) gives row_loss NaN, never an out-of-row read.
 * Writes row_loss[r] (fp32), dlogits[r] = softmax - onehot (bf16, unscaled, 0 for
 * ignored rows, row stride ldd) and out[0]=mean loss, out[1]=1/count (count
 * clamped to >=1 when mask_mode, torch 0/0 semantics otherwise).
 * Replaces F.cross_entropy at source/gpt2/train_gpt2.py:124, gpt2_linear/model.py:206-210,
 * gpt2_cross-att/model.py:170-185. */
int gvl_cross_entropy(const void* logits, int64_t ldl, int64_t rows, int64_t vocab,
                      int64_t rows_per_group, int64_t group_stride, int64_t row_offset,
                      const int64_t* targets, const uint8_t* mask, int32_t mask_mode,
                      float* row_loss, void* dlogits, int64_t ldd, float* out,
                      gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Token + position embedding gather: out[row(r)] = wte[idx[r]] + wpe[r % T],
 * row(r) = (r / T) * out_rows_per_seq + out_offset + r % T  (caption models write the
 * text embeddings after the M image tokens).  `vocab` = rows of wte: an id outside
 * [0, vocab) is never dereferenced (it embeds as row 0 / is dropped from the scatter);
 * callers check ids on the host first, as nn.Embedding raises on them (ABI v3).
 * Replaces nn.Embedding x2 + add (+cat) at source/gpt2/train_gpt2.py:114-117,
 * gpt2_linear/model.py:187-200, gpt2_cross-att/model.py:155-158. */
int gvl_embedding_fwd(const int64_t* idx, const void* wte, const void* wpe, void* out,
                      int64_t n_tokens, int64_t T, int64_t C, int64_t vocab,
                      int64_t out_rows_per_seq, int64_t out_offset, gvl_stream_t stream);
/* One token per sequence, each at its own position (a decode step over prompts of different
 * lengths): out[r] = wte[idx[r]] + wpe[pos[r]] for r < n_tokens, out rows contiguous
 * (C elements apart), pos int32 [n_tokens] on the device, n_pos = rows of wpe.  The same sums
 * and rounding as gvl_embedding_fwd: row r holds the bits of gvl_embedding_fwd called on token r
 * alone with T = 1 and wpe + pos[r]*C.  A position outside [0, n_pos) is treated as an id
 * outside [0, vocab) is: never dereferenced, it reads row 0; callers check both on the host.
 * C % 8 == 0.  Added at ABI v14 without a version bump: a new symbol, nothing existing changes. */
int gvl_embedding_fwd_pos(const int64_t* idx, const int32_t* pos, const void* wte,
                          const void* wpe, void* out, int64_t n_tokens, int64_t C, int64_t vocab,
                          int64_t n_pos, gvl_stream_t stream);
/* Backward: fp32 scatter-add into dwte_acc [V][C] and dwpe_acc [T][C] (caller zeroes). */
int gvl_embedding_bwd(const int64_t* idx, const void* dout, float* dwte_acc, float* dwpe_acc,
                      int64_t n_tokens, int64_t T, int64_t C, int64_t vocab,
                      int64_t out_rows_per_seq, int64_t out_offset, gvl_stream_t stream);
/* ABI v6: deterministic embedding backward accumulated IN PLACE into bf16 gradients:
 * dwte[v] += sum of dout[row(r)] over the tokens r with idx[r] == v (summed in fp32 in token
 * order, one bf16 read-modify-write per touched row — no atomics, bit-identical run to run);
 * dwpe[t] += sum over sequences of dout[row(seq, t)].  Either pointer may be NULL.  The tied
 * wte's gradient is the lm_head weight gradient plus this (train_gpt2.py:114-117, :108 tying);
 * both accumulate into one arena gradient.  `keys`: uint32 scratch of
 * gvl_embedding_bwd_workspace(n_tokens) entries.  C % 8 == 0, C <= 1024, vocab < 2^18 - 1,
 * n_tokens % T == 0; ids outside [0, vocab) contribute nothing. */
/* ABI v6: grouped bf16 row copy: for g < G and t < T, dst row (g*dst_rows + dst_off + t) =
 * src row (g*src_rows + src_off + t) (src_rows = 0 broadcasts one block of T rows to every
 * group); with zero_rest the other dst_rows - T rows of each group are zeroed.  Replaces the
 * caption path's torch.cat of image tokens before the text embeddings
 * (gpt2_linear/model.py:191), query_tokens.expand (gpt2_q_former/model.py:160-161) and the
 * zero-filled [B, S, C] gradient around the text-row lm_head gradient (model.py:219-230). */
int gvl_copy_rows(const void* src, int64_t ld_src, int64_t src_rows, int64_t src_off, void* dst,
                  int64_t ld_dst, int64_t dst_rows, int64_t dst_off, int64_t T, int64_t G,
                  int64_t cols, int32_t zero_rest, gvl_stream_t stream);
int64_t gvl_embedding_bwd_workspace(int64_t n_tokens);
int gvl_embedding_bwd_det(const int64_t* idx, const void* dout, void* dwte, void* dwpe,
                          int64_t n_tokens, int64_t T, int64_t C, int64_t vocab,
                          int64_t out_rows_per_seq, int64_t out_offset, uint32_t* keys,
                          int64_t keys_count, gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* CLIP token pooling: [CLS] + adaptive_avg_pool2d(side x side -> 4 x 8) + L2 normalise
 * (eps 1e-12).  in: [B][1+side*side][D] (fp32 or bf16), out: [B][33][D] (fp32 or bf16).
 * Replaces pool_clip_197_to_33_avg_with_cls, gpt2_linear/model.py:240-254. */
int gvl_pool_clip(const void* in, int32_t in_fp32, void* out, int32_t out_fp32,
                  int64_t B, int64_t L, int64_t D, gvl_stream_t stream);
/* As gvl_pool_clip with the L2 normalisation optional (ABI v3): the pixel-input path pools
 * CLIP's layer-normed hidden states BEFORE the (linear, bias-free) visual projection — the
 * average commutes with it — so the projection runs on 33 tokens instead of 257, then
 * normalises with gvl_l2_normalize_rows (F.normalize(dim=-1, eps=1e-12), D <= 1024). */
int gvl_pool_clip_ex(const void* in, int32_t in_fp32, void* out, int32_t out_fp32, int64_t B,
                     int64_t L, int64_t D, int32_t normalize, gvl_stream_t stream);
int gvl_l2_normalize_rows(const void* in, void* out, int32_t fp32, int64_t rows, int64_t D,
                          gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Optimizer path over flat bf16 arenas (params / grads / exp_avg / exp_avg_sq).
 * gvl_grad_norm: out[0] = ||g||_2 (fp32), out[1] = clip coefficient
 *   min(1, max_norm / (norm + 1e-6)) — torch.nn.utils.clip_grad_norm_ at
 *   source/gpt2/train_gpt2.py:472.  workspace: gvl_grad_norm_workspace_size(n).
 * gvl_adamw: decoupled weight decay on elements [0, n_decay), none after; grads are
 *   multiplied by *grad_scale (the clip coefficient) on the fly; bias corrections use
 *   `step` (1-based) — torch.optim.AdamW(fused=True) at train_gpt2.py:140-143, :476. */
int64_t gvl_grad_norm_workspace_size(int64_t n);
int gvl_grad_norm(const void* g, int64_t n, float max_norm, void* workspace, float* out,
                  gvl_stream_t stream);
int gvl_adamw(void* p, const void* g, void* m, void* v, int64_t n, int64_t n_decay,
              float lr, float beta1, float beta2, float eps, float weight_decay,
              int64_t step, const float* grad_scale, gvl_stream_t stream);
/* As gvl_adamw with lr and the 1-based step read on the device from hyper[0], hyper[1]
 * (fp32): a step captured into a hipGraph stays correct across replays when the caller
 * advances `hyper` (param_groups[i]['lr'] written before each step, train_gpt2.py:474-476). */
int gvl_adamw_dev(void* p, const void* g, void* m, void* v, int64_t n, int64_t n_decay,
                  const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                  const float* grad_scale, gvl_stream_t stream);

/* Mixed-precision form (gvl.optim.AdamW default): fp32 master weights p_master and fp32
 * moments m/v are updated; the bf16 compute copy p the model reads is written from the
 * new master (28 B/param).  Same math and device-side {lr, step} as gvl_adamw_dev.  Keeps
 * sub-ulp updates (LayerNorm gains ~1.0: bf16 ulp 2^-7 >> lr) that a bf16-only step
 * rounds away, so training follows the reference's fp32 path (ABI v3). */
int gvl_adamw_master_dev(void* p, float* p_master, const void* g, float* m, float* v, int64_t n,
                         int64_t n_decay, const float* hyper, float beta1, float beta2, float eps,
                         float weight_decay, const float* grad_scale, gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Incremental decoding (ABI v3).  gvl_attn_decode: one new query per sequence attends all Tk
 * cached keys (non-causal over the cache = causal for the newest position); q element
 * (b, h, d) at q + b*q_sb + h*64 + d, key t at k + b*k_sb + t*k_st + h*64 (same for v),
 * output o + b*o_sb + h*64.  Tk <= 4096.  Replaces the full-sequence recompute of the
 * reference's decode loops (train_gpt2.py:440-449, gpt2_linear/data.py:111-127) with a KV cache.
 * gvl_sample: per row, softmax(logits / temperature), keep the top_k largest (0 = all), then
 * the reference's top-p set (sorted cumulative probability before the token <= top_p, 1 =
 * all; gpt2_linear/data.py:117-122), and draw with the caller's uniform u[row] in [0, 1) by
 * inverse CDF in token-index order.  V <= 65536; out int64 [rows]. */
int gvl_attn_decode(const void* q, int64_t q_sb, const void* k, int64_t k_sb, int64_t k_st,
                    const void* v, int64_t v_sb, int64_t v_st, void* o, int64_t o_sb, int64_t B,
                    int64_t H, int64_t Tk, float scale, gvl_stream_t stream);
int gvl_sample(const void* logits, int64_t ld, int32_t logits_fp32, int64_t rows, int64_t V,
               float temperature, int32_t top_k, float top_p, const float* u, int64_t* out,
               gvl_stream_t stream);

/* Beam-search decoding.  Added at ABI v14 without a version bump: both entry points are new
 * symbols and nothing existing changes, so a v14 caller keeps working against this library.
 *
 * gvl_attn_decode_beam: gvl_attn_decode with cache indirection.  Sequence r reads cached
 * position t from physical cache row src[r*src_ld + t] (int32, each in [0, B); the kernel
 * clamps an entry outside that range so a bad table cannot read outside the cache): its key is
 * at k + row*k_sb + t*k_st + h*64, likewise v.  q and o are indexed by r as before.  Same
 * limits (Tk <= 4096, 16-byte-aligned rows), arithmetic and accumulation order as
 * gvl_attn_decode: on a cache gathered by src the two give the same bits (both are the one
 * function body attn_decode_body, csrc/attn_decode.h; only the address of a key differs).  A
 * beam step only rewrites the small src table instead of copying reordered cache rows.
 *
 * gvl_beam_step: one beam-search step for B items x K beams (1 <= K <= 8, K <= V <= 65536),
 * row r = b*K + j.  logits [B*K, V] bf16 or fp32 (row stride ld); score_in [B*K] fp32 is the
 * raw sum of log-probabilities (-inf: empty slot); flen_in [B*K] int32 is 0 for a live row, else
 * the number of generated tokens of a finished one (its end token included); len_norm[n] (fp32,
 * at least step + 2 entries, positive) multiplies the raw score of an n-token hypothesis; step
 * counts from 0; eos = -1: no end token; t0 = cache position of the first generated token.
 *   candidates: a live row r offers (r, v) for every v < V with raw = score_in[r] + logp(v)
 *     (fp32 log-softmax with max subtraction) and length step + 1, finished (flen = step + 1)
 *     when v == eos; a finished row offers only (r, eos) with its own raw and flen; an empty
 *     row offers nothing.
 *   selection: key = raw * len_norm[length] in fp32; the K largest keys of the item win, ties
 *     to the lower parent slot, then to the lower token id.  Output slot i holds the i-th best:
 *     tok_out int64, parent_out int32 (slot within the item), score_out = raw, flen_out.  Slots
 *     past the last candidate are empty: score -inf, tok eos (0 without one), parent = own
 *     slot, flen 0.
 *   src_out[r'][t] = src_in[b*K + parent][t] for t < t0 + step and src_out[r'][t0 + step] = r'
 *     (the new token's K/V go into its own cache row at the next decoder step).  src_in and
 *     src_out are distinct int32 [B*K, src_ld] tables, src_ld > t0 + step.
 * workspace: gvl_beam_step_workspace_size(B, K) bytes.  Two launches, no synchronisation. */
int gvl_attn_decode_beam(const void* q, int64_t q_sb, const void* k, int64_t k_sb, int64_t k_st,
                         const void* v, int64_t v_sb, int64_t v_st, void* o, int64_t o_sb,
                         int64_t B, int64_t H, int64_t Tk, float scale, const int32_t* src,
                         int64_t src_ld, gvl_stream_t stream);
int64_t gvl_beam_step_workspace_size(int64_t B, int32_t K);
int gvl_beam_step(const void* logits, int64_t ld, int32_t logits_fp32, int64_t B, int32_t K,
                  int64_t V, const float* score_in, const int32_t* flen_in, const float* len_norm,
                  int32_t step, int32_t eos, int64_t t0, const int32_t* src_in, int64_t src_ld,
                  int64_t* tok_out, int32_t* parent_out, float* score_out, int32_t* flen_out,
                  int32_t* src_out, void* workspace, gvl_stream_t stream);

/* Decoding a batch of prompts of different lengths.  Added at ABI v14 without a version bump,
 * like the beam entry points: a new symbol, nothing existing changes.
 *
 * gvl_attn_decode_ragged: gvl_attn_decode_beam (src may be null: then the plain layout of
 * gvl_attn_decode, key t of sequence r in cache row r) that leaves out, per sequence r, the
 * keys of the range [gap_lo[r], gap_hi): gap_lo int32 [B] on the device, one entry per sequence
 * (per row of q), gap_hi the same for all.  The cache stays time-aligned: right-padded prompts
 * are prefilled into columns [0, gap_hi) and every sequence's i-th generated token goes to
 * column gap_hi + i, so sequence r, whose prefix has gap_lo[r] real columns, attends
 * [0, gap_lo[r]) and [gap_hi, Tk).
 *   A key inside the gap is never loaded, neither k nor v, and takes no part in the maximum, the
 *   sum or the accumulation: whatever those cache entries hold, a NaN or an infinity included,
 *   no output bit depends on it.
 *   The kernel clamps gap_lo[r] into [0, gap_hi], so a bad table cannot misbehave.
 *   A sequence with every key inside the gap (gap_lo[r] <= 0 and gap_hi == Tk) writes zeros.
 *   Every key and value outside the gap is handled by the thread, and summed in the place, it
 *   has in gvl_attn_decode: with an empty gap (gap_lo[r] == gap_hi) the output has the bits of
 *   gvl_attn_decode (src null) or gvl_attn_decode_beam (src given).  (All of them are the one
 *   function body attn_decode_body, csrc/attn_decode.h; the gap only skips loop iterations.)
 * Limits as there (Tk in 1..4096, 16-byte-aligned rows, B <= 65535; src_ld >= Tk when src is
 * given), and 0 <= gap_hi <= Tk, gap_lo non-null: checked on the host before the launch (-1 and
 * gvl_last_error naming the argument). */
int gvl_attn_decode_ragged(const void* q, int64_t q_sb, const void* k, int64_t k_sb, int64_t k_st,
                           const void* v, int64_t v_sb, int64_t v_st, void* o, int64_t o_sb,
                           int64_t B, int64_t H, int64_t Tk, float scale, const int32_t* src,
                           int64_t src_ld, const int32_t* gap_lo, int64_t gap_hi,
                           gvl_stream_t stream);

/* Speculative decoding: draft a few tokens per sequence, verify all of them in one KV-cached
 * decoder pass.  Added at ABI v14 without a version bump, like the beam and ragged entry points:
 * new symbols, nothing existing changes.
 *
 * gvl_attn_decode_multi: Q (1..8) new queries per sequence at per-sequence cache lengths, with
 * the K/V append fused.  qkv is this step's contiguous c_attn output [B, Q, 3C] (C = H*64; q at
 * columns [0, C), k at [C, 2C), v at [2C, 3C)), cache the packed per-layer cache [B, Tmax, 3C]
 * (rows 3C apart, sequences cache_sb apart), kv_len int32 [B] on the device, o [B*Q, C] with rows
 * o_ld apart.  With L = kv_len[b] clamped into [0, min(Tmax, 4096) - Q], query j of sequence b
 * sits at position L + j and attends positions [0, L + j]: a key or value at t < L is read from
 * cache[b, t], one at t >= L from qkv[b, t - L].  The launch also copies the k and v columns of
 * qkv[b, j] into cache[b, L + j] for every j < Q.
 *   Bit property: query j's output has exactly the bits of gvl_attn_decode with Tk = L + j + 1 on
 *   a cache that holds the same values: every key keeps its thread and every value its thread
 *   group and place in the sums.  (Both are the one function body attn_decode_body,
 *   csrc/attn_decode.h; only the address of a key or value differs.)
 *   Nothing in the launch reads the cache at or past L, so the append races with no load and no
 *   separate scatter is needed.  Cache columns from L + Q on, the q columns of the cache and,
 *   for query j, the qkv rows of later queries are never loaded: a NaN there reaches no output
 *   bit.  Cache elements outside the k and v columns of [L, L + Q) are never written.
 * Callers keep kv_len[b] + Q <= min(Tmax, 4096); the clamp only makes a bad table harmless.
 *
 * gvl_ngram_draft ("prompt lookup"): sequence b is s = prompt[b, :plen[b]] (int64 [B, P], rows
 * prompt_ld apart; plen int32 [B], clamped into [0, P]) followed by its n[b] emitted tokens
 * emitted[b, :n[b]] (int64, rows emitted_ld >= n_new apart; n int32 [B]); L = plen[b] + n[b],
 * P + n_new <= 4096.  For g = ngram, ngram - 1, ..., 1 (1 <= ngram <= 4) find the largest i with
 * i + g <= L - 1 and s[i..i+g) == s[L-g..L); the first g with a match wins and
 * draft[b, j] = s[i + g + j] for j < D (1 <= D <= 7) while i + g + j < L.  Every other entry is
 * -1: no guess.  Slot j guesses emitted[b, n[b] + j], the token after next for j = 1 and so on.
 * given (optional int64 [B, n_new], rows given_ld apart) overrides: where n[b] + j < n_new and
 * given[b, n[b] + j] >= 0, that is the draft for slot j.  A sequence with n[b] >= n_new (done)
 * gets -1 throughout.  Ids are compared as int32.  draft is int64 [B, D], contiguous.
 *
 * gvl_spec_accept: x int64 [B, Q] holds the token chosen from each of the Q logits rows of a
 * sequence (row j: after feeding [last, draft[0..j))), draft int64 [B, Q - 1] (null with Q = 1).
 * State, all on the device: n, kv_len, pos, lengths int32 [B]; last int64 [B] (the next token to
 * feed); out int64 [B, n_new] (rows out_ld apart).  eos < 0: no end token.  For n[b] < n_new:
 *   a = the count of leading j < Q - 1 with draft[b, j] == x[b, j]; m = min(a + 1, n_new - n[b]);
 *   if x[b, e] == eos for some e < m, the first such e gives m = e + 1, lengths[b] = n[b] + m,
 *   out[b, n[b] + m ..) = eos and n[b] = n_new (done); else n[b] += m.  In both cases
 *   out[b, n[b] .. n[b] + m) = x[b, :m] (the old n), kv_len[b] += m, pos[b] += m and
 *   last[b] = x[b, m - 1].  drafted[b] += the count of draft[b, j] >= 0, accepted[b] += m - 1
 *   (the drafted tokens that reached the output); either may be null.
 * A sequence with n[b] >= n_new keeps every bit of its state.  One thread per sequence, no host
 * involvement.  All three check their arguments on the host before the launch (-1 and
 * gvl_last_error naming the argument). */
int gvl_attn_decode_multi(const void* qkv, void* cache, int64_t cache_sb, int64_t Tmax,
                          const int32_t* kv_len, void* o, int64_t o_ld, int64_t B, int64_t H,
                          int64_t Q, float scale, gvl_stream_t stream);
int gvl_ngram_draft(const int64_t* prompt, int64_t prompt_ld, int64_t P, const int32_t* plen,
                    const int64_t* emitted, int64_t emitted_ld, const int32_t* n, int64_t n_new,
                    const int64_t* given, int64_t given_ld, int64_t B, int32_t ngram, int32_t D,
                    int64_t* draft, gvl_stream_t stream);
int gvl_spec_accept(const int64_t* x, const int64_t* draft, int64_t B, int32_t Q, int32_t* n,
                    int32_t* kv_len, int32_t* pos, int32_t* lengths, int64_t* last, int64_t* out,
                    int64_t out_ld, int64_t n_new, int64_t eos, int32_t* drafted,
                    int32_t* accepted, gvl_stream_t stream);

/* Logits processors: repetition penalty, no-repeat n-gram, end-token and bad-token bans, applied
 * in place between a decoder step and gvl_sample / gvl_beam_step.  Added at ABI v14 without a
 * version bump, like the beam entry points: a new symbol, nothing existing changes.
 *
 * logits [R, V] bf16 or fp32 (row stride ld >= V, 1 <= V <= 65536).  Row r's token sequence s is
 * its item's prompt, prompt[(r / rows_per_item)*prompt_ld + 0..P) (int64, prompt_ld >= P; null
 * with P = 0), then its n_hist generated tokens g_i = hist[i*hist_ld + row_i] (int64, step-major: one step's
 * tok_out of gvl_beam_step or out of gvl_sample is one row of it; hist_ld >= R), where row_i = r
 * when src is null, else src[r*src_ld + t0 + i] (the beam table, int32, src_ld >= t0 + n_hist;
 * the kernel clamps an entry into [0, R), so a bad table cannot read outside hist).
 * L = P + n_hist <= 4096; rows_per_item >= 1 divides R.  Ids are compared as int32 (one past
 * int32 saturates); an id outside [0, V) takes part in n-gram matching as a value and never
 * indexes logits.
 *   skipped: a row with flen != null and flen[r] > 0 (a finished beam) keeps every bit.
 *   repetition penalty (rep_penalty = p != 1; p finite, > 0): for each distinct v of s inside
 *     [0, V), once however often it occurs, x = logits[r][v] as fp32 becomes x < 0 ? x * p : x / p
 *     (a correctly rounded fp32 division), stored as is (fp32) or with one round-to-nearest-even
 *     (bf16): the Hugging Face rule, bit for bit.
 *   no-repeat n-gram (ngram = n, 0 <= n <= 16, 0 = off): n == 1 bans every token of s; n >= 2
 *     and L >= n: for every i in [0, L - n] with s[i + j] == s[L - n + 1 + j] for all j < n - 1,
 *     s[i + n - 1] is banned; L < n bans nothing.
 *   end token: ban_eos != 0 bans eos when 0 <= eos < V (a minimum length).
 *   bad tokens: bad[0..n_bad) (int32) are banned; ids outside [0, V) are ignored.
 * A ban stores -inf and wins over the penalty; gvl_sample and gvl_beam_step give a -inf logit
 * probability 0.  Columns [V, ld), other rows and every logit not named above are never written.
 * O(L + n_bad) logits touched per row; one launch (none when R == 0 or every control is off:
 * p == 1, n == 0, ban_eos == 0, n_bad == 0), no workspace, no synchronisation.  Arguments are
 * checked on the host before the launch (-1 and gvl_last_error naming the argument). */
int gvl_logits_process(void* logits, int64_t ld, int32_t logits_fp32, int64_t R, int64_t V,
                       const int64_t* hist, int64_t hist_ld, int32_t n_hist, const int32_t* src,
                       int64_t src_ld, int64_t t0, const int64_t* prompt, int64_t prompt_ld,
                       int32_t P, int32_t rows_per_item, float rep_penalty, int32_t ngram,
                       int32_t eos, int32_t ban_eos, const int32_t* bad, int32_t n_bad,
                       const int32_t* flen, gvl_stream_t stream);

/* Device-stepped decoding: the entry points a decode step needs so that one token's work can be
 * captured once as a graph and replayed (gvl.decode.GraphedGenerate / GraphedBeamSearch).  What a
 * host-stepped launch takes as an argument that changes every token (the cache column, Tk, n_hist,
 * ban_eos, step) is read from one int32 in device memory instead, which the graph itself
 * advances.  Added at ABI v14 without a version bump, like the beam, logits and scoring entry
 * points: new symbols, nothing existing changes.  Each shares its device code with the
 * host-stepped instance, so the bit properties below hold by construction.
 *
 * gvl_attn_decode_step: one new query per sequence, the K/V append fused, the column read on the
 * device.  qkv is this step's contiguous c_attn output [R, 3C] (C = H*64; q | k | v), cache the
 * packed per-layer cache [R, Tmax, 3C] (rows 3C apart, sequences cache_sb apart, Tmax <= 4096),
 * t one int32 on the device: the time-aligned column tc = *t of this step, o [R, C] with rows o_ld
 * apart.  The workgroup of (sequence r, head h) copies that head's k and v of qkv[r] into
 * cache[r, tc] and attends positions [0, tc]: position t' < tc is read from cache row r, or from
 * row src[r*src_ld + t'] when src (int32, src_ld >= Tmax, entries clamped into [0, R)) is given;
 * position tc is the row's own new key / value, read from qkv.  With gap_lo (int32 [R], clamped
 * into [0, gap_hi]; 0 <= gap_hi <= Tmax) the positions [gap_lo[r], gap_hi) are left out as in
 * gvl_attn_decode_ragged.
 *   Bit property: o has exactly the bits of gvl_attn_decode (src and gap_lo null),
 *   gvl_attn_decode_beam (src), or gvl_attn_decode_ragged (gap_lo, with or without src) at
 *   Tk = tc + 1 on a cache whose column tc holds the new k / v (and, with src, src[r][tc] = r).
 *   (All are the one function body attn_decode_body, csrc/attn_decode.h.)
 *   Nothing in the launch loads the cache at or past column tc, the q columns of the cache or a
 *   position inside the gap; nothing but the k and v columns of cache[:, tc] is written.
 *   tc outside [0, Tmax) makes the launch a no-op: neither o nor the cache is written, so a
 *   counter that ran away cannot write outside the cache.
 *
 * gvl_logits_process_dev: gvl_logits_process with n_hist = clamp(*step, 0, hist_cap) and the end
 * token banned while *step < min_new; step is one int32 on the device.  hist holds at least
 * hist_cap steps, src_ld >= t0 + hist_cap, P + hist_cap <= 4096; every other argument and every
 * rule is gvl_logits_process's, bit for bit (one kernel body).  No launch when R == 0 or no control
 * can ever act (p == 1, n == 0, min_new <= 0, n_bad == 0).
 *
 * gvl_beam_step_dev: gvl_beam_step with step = *step read on the device (one int32) and a host
 * bound max_steps >= 1: len_norm has at least max_steps + 1 entries and src_ld >= t0 + max_steps.
 * *step outside [0, max_steps) writes nothing; otherwise all five outputs have the bits of
 * gvl_beam_step at that step (one pair of kernel bodies).
 * All three check on the host what the host can see (-1 and gvl_last_error naming the argument). */
int gvl_attn_decode_step(const void* qkv, void* cache, int64_t cache_sb, int64_t Tmax,
                         const int32_t* t, void* o, int64_t o_ld, int64_t R, int64_t H, float scale,
                         const int32_t* src, int64_t src_ld, const int32_t* gap_lo, int64_t gap_hi,
                         gvl_stream_t stream);
int gvl_logits_process_dev(void* logits, int64_t ld, int32_t logits_fp32, int64_t R, int64_t V,
                           const int64_t* hist, int64_t hist_ld, const int32_t* step,
                           int32_t hist_cap, const int32_t* src, int64_t src_ld, int64_t t0,
                           const int64_t* prompt, int64_t prompt_ld, int32_t P,
                           int32_t rows_per_item, float rep_penalty, int32_t ngram, int32_t eos,
                           int32_t min_new, const int32_t* bad, int32_t n_bad, const int32_t* flen,
                           gvl_stream_t stream);
int gvl_beam_step_dev(const void* logits, int64_t ld, int32_t logits_fp32, int64_t B, int32_t K,
                      int64_t V, const float* score_in, const int32_t* flen_in,
                      const float* len_norm, const int32_t* step, int32_t max_steps, int32_t eos,
                      int64_t t0, const int32_t* src_in, int64_t src_ld, int64_t* tok_out,
                      int32_t* parent_out, float* score_out, int32_t* flen_out, int32_t* src_out,
                      void* workspace, gvl_stream_t stream);

/* Scoring of given tokens (the HellaSwag evaluation of train_gpt2.py:190-202, 394-426, caption
 * reranking, perplexity).  Added at ABI v14 without a version bump, like the beam and logits
 * entry points: new symbols, nothing existing changes.
 *
 * gvl_token_logprobs: per row r of logits [rows, V] bf16 or fp32 (row stride ld >= V in elements,
 * 1 <= V <= 65536, V any value; columns [V, ld) never count as logits; rows whose address and
 * stride are 16-byte aligned are read with 16-byte loads, others element by element) and its
 * target t = targets[r] (int64), in fp32:
 *   lse[r]    = max + log(sum_v exp(x[v] - max));
 *   logp[r]   = x[t] - lse[r];
 *   argmax[r] = the lowest v with x[v] == max (torch.argmax's tie-break), int32;
 *   rank[r]   = #{v: x[v] > x[t]} + #{v < t: x[v] == x[t]}, int32: 0 iff t is the argmax.
 * Each of the four outputs may be null.  mask: optional uint8 [rows].
 *   skipped: a row with t == -100 or mask[r] == 0; its logits are not read; logp = 0, lse = 0,
 *     argmax = -1, rank = -1.
 *   t outside [0, V) and not -100: nothing outside the row is read; logp = NaN, rank = -1 (the
 *     convention of gvl_cross_entropy); lse and argmax are the row's.
 *   x[t] = -inf in a row with a finite maximum (a banned token): logp = -inf exactly.
 * One launch, one workgroup per row, no workspace, no synchronisation.
 *
 * gvl_sequence_score: logp fp32 [N, T] (row-major, as written by gvl_token_logprobs), mask
 * optional uint8 [N, T], group in 1..16 dividing N.  Per sequence n, over the positions with
 * mask != 0 (all without a mask): sum_nll[n] = sum of -logp in fp32 in a fixed order, count[n]
 * (int32), mean_nll[n] = sum_nll / count (0 / 0 = NaN).  Per example g = `group` consecutive
 * sequences: pred_norm[g] = the first argmin of mean_nll, pred[g] = the first argmin of sum_nll
 * (int32, index within the example); both -1 when a sequence of the example has count 0.
 * One launch, one workgroup per example, no workspace, no synchronisation.
 * Both check their arguments on the host before the launch (-1 and gvl_last_error naming the
 * argument). */
int gvl_token_logprobs(const void* logits, int64_t ld, int32_t logits_fp32, int64_t rows,
                       int64_t V, const int64_t* targets, const uint8_t* mask, float* logp,
                       float* lse, int32_t* argmax, int32_t* rank, gvl_stream_t stream);
int gvl_sequence_score(const float* logp, const uint8_t* mask, int64_t N, int64_t T,
                       int32_t group, float* sum_nll, int32_t* count, float* mean_nll,
                       int32_t* pred_norm, int32_t* pred, gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Small fused elementwise helpers on the hot path. */
/* Column sums of a bf16 [rows][cols] matrix (row stride ld) -> bf16 out[cols]
 * (bias gradients); accumulate adds into out. workspace: gvl_colsum_workspace_size. */
int64_t gvl_colsum_workspace_size(int64_t rows, int64_t cols);
int gvl_colsum(const void* x, int64_t rows, int64_t cols, int64_t ld, void* out,
               int32_t accumulate, void* workspace, gvl_stream_t stream);
/* count (<= 16) column sums of one shape in one launch pair: out[i] (+)= colsum(x[i]) — the
 * deferred bias gradients of the 12 GPT-2 blocks (train_gpt2.py:471, nn.Linear bias grads).
 * workspace: gvl_colsum_batched_workspace_size(count, rows, cols) bytes. */
int64_t gvl_colsum_batched_workspace_size(int32_t count, int64_t rows, int64_t cols);
int gvl_colsum_batched(const void* const* x, void* const* out, int32_t count, int64_t rows,
                       int64_t cols, int64_t ld, int32_t accumulate, void* workspace,
                       gvl_stream_t stream);
/* out[r][c] = in[r][c] * keep(seed, r*cols+c) / (1-p) — dropout backward, with the
 * same counter-based mask the GEMM epilogue applies. */
int gvl_dropout_mask_apply(const void* in, int64_t ld_in, void* out, int64_t ld_out,
                           int64_t rows, int64_t cols, float p, uint64_t seed,
                           const uint64_t* seed_ptr, gvl_stream_t stream);
/* out[i] = tanh(*gate) * in[i] and gate_grad (fp32 scalar, accumulated) +=
 * (1 - tanh^2) * sum_i in[i] * y[i] — backward of x + tanh(g) * y
 * (gpt2_cross-att/model.py:101). */
int gvl_gate_bwd(const void* dx, const void* y, const void* gate, void* dy, float* gate_grad,
                 int64_t n, void* workspace, gvl_stream_t stream);
int64_t gvl_gate_bwd_workspace_size(int64_t n);
/* ABI v13: as gvl_gate_bwd, the gate gradient added into the bf16 scalar gate_grad (the gate
 * parameter's own .grad): gate_grad = bf16(gate_grad + bf16(dgate)), the roundings of
 * autograd's AccumulateGrad on a bf16 parameter — no fp32 scalar, zero-fill or conversion. */
int gvl_gate_bwd_acc_bf16(const void* dx, const void* y, const void* gate, void* dy,
                          void* gate_grad, int64_t n, void* workspace, gvl_stream_t stream);
/* fp32 -> bf16 conversion with optional accumulate into the bf16 destination. */
int gvl_f32_to_bf16(const float* in, void* out, int64_t n, int32_t accumulate,
                    gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Int8 weight-only decoding (csrc/linear_w8.hip).  Format: one fp32 scale per row n of an
 * nn.Linear weight [N][K], symmetric, no zero point: scale[n] = absmax_n / 127 (one correctly
 * rounded fp32 division), q[n][k] = clamp(rint(fp32(w[n][k]) / scale[n]), -127, 127) (correctly
 * rounded division, ties to even); a row of zeros has scale 0 and q 0.  A non-finite weight
 * makes its row's scale non-finite (the caller checks the scales once).  The dequantised
 * weight is bf16_rne(fp32(q) * scale[n]).
 * All three replace the nn.Linear forward inside the reference's decode loops
 * (source/gpt2/train_gpt2.py:440-449, gpt2_linear/data.py:111-127: model(x) per new token,
 * whose Linears read every weight once per token). */
/* bf16 w [N][K] (row stride ldw) -> int8 q [N][K] (ldq), fp32 scale [N]; one launch, 3 bytes of
 * HBM traffic per weight.  K, ldw, ldq multiples of 8; w, q, scale 16-byte aligned. */
int gvl_quantize_rows_i8(const void* w, int64_t ldw, int64_t n, int64_t k, void* q, int64_t ldq,
                         float* scale, gvl_stream_t stream);
/* int8 q [N][K] (ldq), fp32 scale [N] -> bf16 out [N][K] (ldo).  K, ldq, ldo multiples of 8;
 * q, scale, out 16-byte aligned. */
int gvl_dequantize_rows_i8(const void* q, int64_t ldq, const float* scale, int64_t n, int64_t k,
                           void* out, int64_t ldo, gvl_stream_t stream);
/* Linear on a few rows: c[m][n] = epi(scale[n] * sum_k x[m][k] * w[n][k]), x bf16 [M][K], w int8
 * [N][K] with scale fp32 [N]; scale == NULL: w is a bf16 [N][K] weight, same kernel body, no
 * conversion and no scale.  The int8 values enter the bf16 MFMA exactly, the sum is fp32 (K in
 * 64-wide chunks dealt to the 8 waves of a workgroup, 32-deep MFMA steps, the waves' partials
 * added in wave order), the scale is applied once in fp32, then gemm_common.h's epilogue in its
 * order: +bias, tanh-GELU (act 1), *tanh(*gate), +residual, one rounding to bf16.  Accepted
 * epilogues: plain; bias; bias + act 1; bias + residual; bias + gate + residual (anything else
 * is refused).  residual may alias c.
 * The bits of c[m][n] depend only on row m of x, row n of w, scale[n] and that element's
 * epilogue operands: not on M, other rows, ldc, or the grid; no atomics, no workspace.
 * K % 64 == 0, N % 8 == 0, 1 <= M <= GVL_LINEAR_W8_MAX_ROWS (64 rows per pass over w); ldx % 8,
 * ldw % 16 (int8) or % 8 (bf16), ldc % 4, ldr % 4 == 0, ldc >= N; every operand 16-byte aligned. */
#define GVL_LINEAR_W8_MAX_ROWS 256
typedef struct gvl_linear_w8_desc {
  const void* x;        /* bf16 [M][ldx] */
  const void* w;        /* int8 [N][ldw] (scale given) or bf16 [N][ldw] (scale NULL) */
  const float* scale;   /* fp32 [N] or NULL */
  void* c;              /* bf16 [M][ldc] */
  int64_t m, n, k;
  int64_t ldx, ldw, ldc;
  const void* bias;     /* optional bf16 [N] */
  int32_t act;          /* 0 none, 1 gelu-tanh */
  const void* residual; /* optional bf16 [M][ldr], may alias c */
  int64_t ldr;
  const void* gate;     /* optional bf16 scalar g: branch *= tanh(g) */
} gvl_linear_w8_desc;
int gvl_linear_w8(const gvl_linear_w8_desc* d, gvl_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Int8 KV cache for decoding (csrc/attn_decode_q8.hip).  New symbols at ABI v14 without a version
 * bump, like the beam, ragged, step and w8 entry points.  The format is gvl_quantize_rows_i8's
 * with one "row" being one head's 64-wide key or value vector at one position: scale = absmax /
 * 127, q = clamp(rint(x / scale), -127, 127), a zero vector has scale 0 and q 0, a non-finite
 * element makes the scale non-finite.  A layer's cache is two tensors, C = H*64:
 *   kv8 int8 [R][Tmax][2C] (rows 2C apart, sequences kv8_sb apart): the k heads, then the v heads;
 *   kvs fp32 [R][Tmax][2H] (rows 2H apart, sequences kvs_sb apart): the k scales, then the v scales.
 * The q third of a c_attn row is not stored.
 *
 * gvl_kv_quantize_i8 (the prefill): the k and v thirds of qkv[b][s] (bf16 [B][S][3C], sequences
 * qkv_sb apart, positions qkv_st apart) go to column col0 + s of sequence b, for all B * S
 * positions in one launch.  Nothing else is written.  0 <= col0, col0 + S <= 4096; kv8_sb and
 * kvs_sb at least col0 + S rows; kv8 16-byte aligned.
 *
 * gvl_attn_decode_q8 (a step): append + attend.  qkv is this step's contiguous c_attn output
 * [R][3C]; the column of the step is tc = *t_dev when t_dev (one int32 on the device: graph replay)
 * is given, else t.  The workgroup of (sequence r, head h) quantises that head's new k and v of
 * qkv[r], stores the 64 + 64 bytes and the two scales to column tc of row r, and attends positions
 * [0, tc]: position t' < tc from cache row r, or from row src[r*src_ld + t'] when src (int32,
 * src_ld >= Tmax, entries clamped into [0, R)) is given; position tc is its own quantised vectors,
 * kept on chip.  With gap_lo (int32 [R], clamped into [0, gap_hi]; 0 <= gap_hi <= Tmax) positions
 * [gap_lo[r], gap_hi) are left out as in gvl_attn_decode_ragged: neither their bytes nor their
 * scales are loaded, and a sequence with every position skipped writes zeros.
 *   Semantics: the attention sees, for every position including the step's own, fp32(q8) * scale;
 *   nothing else differs from gvl_attn_decode_step.  score_t = ks[t] * sum_d qs[d] * fp32(kq[t][d])
 *   (the sum in fp32, the scale applied once after it), the value pass accumulates
 *   (p_t * vs[t]) * fp32(vq[t][d]); max, sum, skip and the final division are attn_decode_body's.
 *   Bit properties (one kernel body, four (src, gap) instances): the bytes and scales appended
 *   equal what gvl_kv_quantize_i8 writes for the same qkv; src = identity and an empty gap each
 *   give the bits of the instance without them; t_dev gives the bits of the same column passed as t.
 *   Every load of the cache is at a position below tc, every store at tc.  tc outside
 *   [0, Tmax) makes the call a no-op: neither o nor the cache is written.  1 <= Tmax <= 4096.
 * Both check on the host what the host can see (-1 and gvl_last_error naming the argument) and are
 * capturable: no allocation, no synchronisation. */
int gvl_kv_quantize_i8(const void* qkv, int64_t qkv_sb, int64_t qkv_st, void* kv8, int64_t kv8_sb,
                       float* kvs, int64_t kvs_sb, int64_t B, int64_t S, int64_t H, int64_t col0,
                       gvl_stream_t stream);
int gvl_attn_decode_q8(const void* qkv, void* kv8, int64_t kv8_sb, float* kvs, int64_t kvs_sb,
                       int64_t Tmax, int64_t t, const int32_t* t_dev, void* o, int64_t o_ld,
                       int64_t R, int64_t H, float scale, const int32_t* src, int64_t src_ld,
                       const int32_t* gap_lo, int64_t gap_hi, gvl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GVL_H_ */
