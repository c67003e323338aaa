/*
 * peneo_hip.h — C ABI of libpeneo_hip.so, the MI355X (gfx950) device library behind the
 * PEneo forward/backward hot path.
 *
 * The upstream reference (ZeningLin/PEneo) is pure Python; it has no FFI.  The boundary a
 * maintainer swaps is the nn.Module contract of model/modeling_peneo.py:108-175 and
 * model/peneo_decoder.py:338-443.  Each entry point below names the reference code whose
 * device work it replaces.  INTEGRATION.md shows the ctypes stub that binds them.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - sizes are explicit; no hidden allocation: workspaces are passed in by the caller;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *   - return 0 on success, a negative PENEO_ERR_* otherwise; peneo_last_error() gives the
 *     (thread-local) message;
 *   - "dtype" selects the storage type of activations/weights: PENEO_BF16 (MFMA bf16 inputs,
 *     fp32 accumulate; the throughput mode) or PENEO_F32 (exact fp32 MFMA; the parity mode).
 *     Gradients of parameters, losses, logits, LayerNorm statistics and softmax
 *     log-sum-exps are always fp32.
 */
#ifndef PENEO_HIP_H
#define PENEO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PENEO_OK 0
#define PENEO_ERR_INVALID (-1)
#define PENEO_ERR_LAUNCH (-2)

#define PENEO_F32 0
#define PENEO_BF16 1

#define PENEO_ACT_NONE 0
#define PENEO_ACT_GELU 1 /* exact erf GELU (transformers RobertaIntermediate) */
#define PENEO_ACT_SILU 2 /* nn.SiLU (model/peneo_decoder.py:217,220,235) */

#define PENEO_MAX_HEADS 8 /* pair-classifier heads (the reference has 5) */

typedef void* peneo_stream_t;

int peneo_version(void);
const char* peneo_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Dense contraction:  C[m,n] = epilogue( alpha * sum_k A(m,k) * B(n,k) )
 *   a_kmajor != 0 : A is [M, K] row-major (leading dim lda >= K)   else A is [K, M] (lda >= M)
 *   b_kmajor != 0 : B is [N, K] row-major (ldb >= K)               else B is [K, N] (ldb >= N)
 * so  forward  y = x W^T      -> (a_kmajor=1, b_kmajor=1)            [nn.Linear everywhere]
 *     dgrad    dx = dy W      -> (1, 0)
 *     wgrad    dW = dy^T x    -> (0, 0)
 * Epilogue order:  v = alpha*acc (+bias[n]) ; preact <- v ; v = act(v) ; v *= act'(grad_src[m,n]) ;
 *                  dropout ; v += residual[m,n] ; v += C[m,n] if accumulate ; C <- v
 * Kernel choice for bf16 operands that meet the LDS-DMA conditions (16-byte aligned bases and rows): (1, *) the persistent launch or the
 * 8-wave big tiles where their rules pick the problem, else 128 x 128 tiles; (0, 0) a wgrad whose C is fp32 and made of whole
 * 384 x 192 tiles, with no epilogue option beyond accumulate, no a_colsum, K % 64 == 0 and K >= 65536 runs tiles x split_k
 * one-per-CU workgroups on 384 x 192 tiles (the pair heads' dW1; peneo_gemm_set_nn384_mode below), every other one 128 x 128 tiles.
 * A split reduction sums its slices in slice order on every path.
 * Replaces torch.nn.Linear / F.linear call sites: modeling_layoutlmv3.py:292-294,335-360,
 * RobertaSelfOutput/Intermediate/Output, peneo_decoder.py:126,213-222 and their autograd.
 * ------------------------------------------------------------------------------------------ */
struct peneo_pair_dz_args;
typedef struct peneo_gemm_epilogue {
  const float* bias;        /* [N] fp32 or NULL */
  int act;                  /* PENEO_ACT_* applied after bias */
  void* preact;             /* optional [M, ld_preact] (dtype c_dtype): value before act */
  int64_t ld_preact;
  const void* grad_src;     /* optional [M, ld_grad] (dtype c_dtype): multiply by act'(grad_src) */
  int64_t ld_grad;
  int grad_act;             /* which act' */
  const void* residual;     /* optional [M, ld_res] (dtype c_dtype) added last */
  int64_t ld_res;
  float alpha;              /* 0 is read as 1 */
  int accumulate;           /* C += result (c_dtype must be PENEO_F32) */
  float drop_p;             /* dropout probability (0 = off); keep mask = f(drop_seed, m*N+n) */
  uint32_t drop_seed;
  /* pair-head backward fusion (K12 bwd): when set, the tile is the first-layer pre-activation z = acc + bias of
   * rows = pairs, columns = [head, hidden]; the epilogue stores dz (see peneo_pair_dz) instead of z and adds the
   * dW2 / db1 partial sums to `pair_dz_ws` (same workspace layout as peneo_pair_dz, row = m-tile index mod 256).
   * No other epilogue option may be combined with it; split_k must be 1. */
  const struct peneo_pair_dz_args* pair_dz;
  float* pair_dz_ws;
  /* wgrad fusion (a_kmajor = 0, b_kmajor = 0, bf16): a_colsum[m] += sum_k A(m, k) -- with A = dy [tokens, M] this is the
   * bias gradient db = dy^T 1 of the same nn.Linear (autograd of modeling_layoutlmv3.py:292-294 and the Roberta dense
   * layers), taken from the A tiles the weight-gradient product already holds in LDS (one extra MFMA against a ones
   * operand in the workgroups of the first tile column; fp32 atomics, one per row and split slice).  [M] fp32 or NULL. */
  float* a_colsum;
} peneo_gemm_epilogue;

/* Workspace: peneo_gemm_workspace_bytes(M, N, K, split_k) bytes, 16-byte aligned, used by one call at a time (the next call on the
 * same stream may reuse it).  It holds the fp32 partials of a split reduction, and the flags and fp32 slabs of a persistent launch
 * whose ranges cut tiles (stream-k; large bf16 problems with k-major A and B, few tiles and a deep K), so it may be non-zero with
 * split_k == 1.  Its size follows peneo_gemm_set_sk_mode.  A stream-k launch zeroes its flags on `stream` before it starts, so a
 * call captured into a graph runs the same kernels as an eager one and replays with the workspace it was captured with.  A call
 * that needs the workspace and gets a null, smaller or misaligned one returns PENEO_ERR_INVALID. */
size_t peneo_gemm_workspace_bytes(int M, int N, int K, int split_k);
int peneo_gemm(int dtype, int a_kmajor, int b_kmajor, int M, int N, int K,
               const void* A, int64_t lda, const void* B, int64_t ldb,
               void* C, int64_t ldc, int c_dtype, const peneo_gemm_epilogue* ep,
               int split_k, void* workspace, size_t workspace_bytes, peneo_stream_t stream);

/* Up to 4 independent bf16 GEMMs C_i = op(A_i) op(B_i) of ONE operand layout in ONE launch (tiles of all problems side by
 * side, full K per tile, no split-k, no epilogue besides fp32 accumulate).  Operands must satisfy the LDS-DMA conditions
 * of peneo_gemm's bf16 path (16-byte aligned bases and row strides).  Used for the four weight gradients
 * dW = dy^T x of an encoder layer (autograd of the nn.Linear calls at modeling_layoutlmv3.py:292-294,335-360). */
typedef struct peneo_gemm_problem {
  int M, N, K;
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc;
  int accumulate;           /* C += A B (c_dtype must be PENEO_F32) */
  const peneo_gemm_epilogue* ep;   /* optional fused epilogue of THIS problem (bias, activation, pre-activation store, x act'(src),
                                    * dropout, residual: as for peneo_gemm; no pair_dz, no a_colsum); NULL = none.  Round 4: LiLT's
                                    * text and layout streams (modeling_lilt.py:269-429, H = 768 and H / 4 = 192) run each pair of
                                    * same-role Linear layers as one launch -- a [4096, 192] x [192, 576] GEMM alone is all fixed cost */
} peneo_gemm_problem;
int peneo_gemm_group(int dtype, int a_kmajor, int b_kmajor, int c_dtype, const peneo_gemm_problem* problems, int n,
                     peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise plumbing
 * ------------------------------------------------------------------------------------------ */
int peneo_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, peneo_stream_t stream);
/* Many contiguous fp32 -> bf16 casts in one launch: the bf16 working copies of the fp32 master weights that every nn.Linear of
 * the reference would read (modeling_layoutlmv3.py:292-294,335-360), refreshed after an optimizer step.  `table_dev` and the
 * two chunk maps (chunk c = elements [chunk_index[c] * peneo_cast_multi_chunk_elems(), ...) of item chunk_item[c]) live in
 * device memory and are built once per set of tensors. */
typedef struct peneo_cast_item { const float* src; void* dst; int64_t numel; } peneo_cast_item;
int peneo_cast_multi_chunk_elems(void);
int peneo_cast_multi(const peneo_cast_item* table_dev, const int32_t* chunk_item_dev, const int32_t* chunk_index_dev, int n_chunks,
                     peneo_stream_t stream);
/* dst[r, c] = src[r, c] for a strided 2-D block (row strides in elements), with optional dropout */
int peneo_copy2d(int dtype, const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                 float drop_p, uint32_t drop_seed, peneo_stream_t stream);
/* batched variant: logical row r of side X lives at (r / X_rpb) * X_bstride + (r % X_rpb) * ld_X elements
 * (X_rpb = 0: r * ld_X).  Used for the CLS / visual-token crop of model/modeling_peneo.py:138-163. */
int peneo_copy_rows(int dtype, const void* src, int64_t src_rpb, int64_t src_bstride, int64_t ld_src,
                    void* dst, int64_t dst_rpb, int64_t dst_bstride, int64_t ld_dst, int64_t rows, int64_t cols,
                    float drop_p, uint32_t drop_seed, peneo_stream_t stream);
/* LiLT (modeling_lilt.py:269-429) sums text and layout attention scores (BiACM).  With per-head concatenation
 *   out[r, h*(da+db) + c] = c < da ? scale_a * a[r, h*da + c] : scale_b * b[r, h*db + (c - da)]
 * of q (pre-scaled by 1/sqrt(d), 1/sqrt(d_l)), k and v, one attention call over head dim da+db yields both
 * context streams; peneo_head_split is the inverse (used for the context and for dq/dk/dv). */
int peneo_head_concat(int dtype, const void* a, int64_t lda, int da, float scale_a, const void* b, int64_t ldb, int db,
                      float scale_b, void* out, int64_t ldo, int64_t rows, int nh, peneo_stream_t stream);
int peneo_head_split(int dtype, const void* in, int64_t ldi, void* a, int64_t lda, int da, float scale_a, void* b,
                     int64_t ldb, int db, float scale_b, int64_t rows, int nh, peneo_stream_t stream);
/* out[n] (+)= sum_m x[m, n]   (bias gradients) */
int peneo_colsum(int dtype, const void* x, int64_t ldx, int64_t M, int64_t N, float* out, int accumulate,
                 peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (modeling_layoutlmv3.py:225,930,1113; Roberta*Output.LayerNorm).
 * Row r of the logical [rows, H] matrix lives at  (r / rpb) * bstride + (r % rpb) * H  elements
 * (rpb = 0 means contiguous), separately for input and output, so that sub-ranges of a
 * [B, T, H] buffer can be normalised in place.
 * ------------------------------------------------------------------------------------------ */
int peneo_layernorm_fwd(int dtype, const void* x, int64_t x_rpb, int64_t x_bstride,
                        void* y, int64_t y_rpb, int64_t y_bstride,
                        const float* gamma, const float* beta, float eps,
                        float* mean, float* rstd, int64_t rows, int H,
                        float drop_p, uint32_t drop_seed, peneo_stream_t stream);
/* dx may alias dy.  dgamma/dbeta (fp32, [H]) are accumulated into.
 * dx_dropped (may be NULL): a second, contiguous [rows, H] output = dx through the dropout mask (drop2_p, drop2_seed,
 * element index r*H + c) of the GEMM that produced this LayerNorm's input — the gradient that GEMM's dgrad/wgrad need,
 * without a separate masking pass.
 * dx_colsum (may be NULL; fp32 [H], accumulated into): the column sums over the rows of dx_dropped (of dx when dx_dropped is
 * NULL), summed in fp32 before the rounding to the output dtype = the BIAS gradient of the Linear that produced the
 * LayerNorm's input (modeling_layoutlmv3.py:482-529: dense -> dropout -> + residual -> LayerNorm), without a column-sum launch. */
int peneo_layernorm_bwd(int dtype, const void* dy, int64_t dy_rpb, int64_t dy_bstride,
                        const void* x, int64_t x_rpb, int64_t x_bstride,
                        void* dx, int64_t dx_rpb, int64_t dx_bstride,
                        const float* gamma, const float* mean, const float* rstd,
                        float* dgamma, float* dbeta, int64_t rows, int H,
                        float drop_p, uint32_t drop_seed, void* dx_dropped, float drop2_p, uint32_t drop2_seed,
                        float* dx_colsum, peneo_stream_t stream);
/* The same backward with the parameter gradients left as per-workgroup partial sums, partials[P][2][H] (fp32; row 0 of a
 * pair = gamma, row 1 = beta), P = peneo_layernorm_bwd_partial_rows(dtype, rows, H); 0 means this dtype / row length has
 * no such form (use peneo_layernorm_bwd).  The caller reduces them with peneo_colsum over [P, 2H] whenever it likes (the
 * model does it on its weight-gradient stream): no same-address atomics at the end of the kernel, one row per half-wave.
 * All row bases 16-byte aligned. */
int64_t peneo_layernorm_bwd_partial_rows(int dtype, int64_t rows, int H);
int peneo_layernorm_bwd_partial(int dtype, const void* dy, int64_t dy_rpb, int64_t dy_bstride,
                                const void* x, int64_t x_rpb, int64_t x_bstride,
                                void* dx, int64_t dx_rpb, int64_t dx_bstride,
                                const float* gamma, const float* mean, const float* rstd,
                                float* partials, int64_t partial_rows, int64_t rows, int H,
                                float drop_p, uint32_t drop_seed, void* dx_dropped, float drop2_p, uint32_t drop2_seed,
                                peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K1 — text embeddings (modeling_layoutlmv3.py:131-227, modeling_lilt.py:75-130,160-210)
 * ------------------------------------------------------------------------------------------ */
/* RoBERTa position ids: cumsum(ids != pad) * (ids != pad) + pad   (:164-181) */
int peneo_position_ids(const int64_t* input_ids, int B, int S, int64_t pad_id, int32_t* pos_ids,
                       peneo_stream_t stream);
/* out[b,s,:] = word[ids] + type0 + pos[pid] (+ cat(x[l],y[t],x[r],y[b],h[b-t],w[r-l]) if spatial) ;
 * returns PENEO_ERR_INVALID through `status` (device int, may be NULL) when a coordinate is outside
 * [0, max_2d) — the reference raises IndexError (:133,138-141).
 * clip_hw != 0 clips the h/w lookups to [0, max_2d-1] (LayoutLMv3); LiLT does not clip.         */
typedef struct peneo_embed_tables {
  const float* word;   /* [vocab, H] */
  const float* type0;  /* [H] row 0 of token_type_embeddings */
  const float* pos;    /* [max_pos, H] */
  const float* x; const float* y; const float* h; const float* w; /* [max_2d, coord|shape]; NULL = no spatial part */
  int coord_size; int shape_size; int max_2d; int vocab; int max_pos;
} peneo_embed_tables;
int peneo_embed_text_fwd(int dtype, const int64_t* input_ids, const int32_t* pos_ids, const int64_t* bbox,
                         const peneo_embed_tables* tab, int B, int S, int H, int clip_hw,
                         void* out, int64_t out_rpb, int64_t out_bstride, int32_t* status, peneo_stream_t stream);
/* scatter-add of d_out into fp32 table gradients (dense, like nn.Embedding(sparse=False));
 * rows equal to pad_id are skipped for word/pos (padding_idx semantics). */
typedef struct peneo_embed_grads {
  float* word; float* type0; float* pos; float* x; float* y; float* h; float* w;
} peneo_embed_grads;
int peneo_embed_text_bwd(int dtype, const void* d_out, int64_t rpb, int64_t bstride,
                         const int64_t* input_ids, const int32_t* pos_ids, const int64_t* bbox,
                         const peneo_embed_grads* g, int coord_size, int shape_size, int max_2d,
                         int B, int S, int H, int clip_hw, int64_t pad_id, peneo_stream_t stream);
/* spatial-only embedding for LiLT: out[b,s,:] = cat(x[l],y[t],x[r],y[b],h[b-t],w[r-l]) */

/* ------------------------------------------------------------------------------------------
 * K2 — patch embedding (modeling_layoutlmv3.py:51-84, 910-931)
 * ------------------------------------------------------------------------------------------ */
/* image [B, C, Hi, Wi] fp32 -> patches [B * (Hi/16) * (Wi/16), C*256] (k = c*256 + py*16 + px) */
int peneo_im2col_patch16(int dtype, const float* image, int B, int C, int Hi, int Wi, void* patches,
                         peneo_stream_t stream);
/* vis[b,0,:] = cls + pos[0]; vis[b,1+p,:] = proj[b*np+p,:] + pos[1+p]  */
int peneo_visual_assemble_fwd(int dtype, const void* proj, const float* cls, const float* pos, int B, int np, int H,
                              void* vis, peneo_stream_t stream);
/* d_proj <- d_vis[:,1:]; d_cls += sum_b d_vis[b,0]; d_pos += sum_b d_vis[b] */
int peneo_visual_assemble_bwd(int dtype, const void* d_vis, int B, int np, int H, void* d_proj, float* d_cls,
                              float* d_pos, peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K4 — relative-position bias (modeling_layoutlmv3.py:586-676), computed once per forward.
 * lut[|delta|] holds the *unsigned* part of relative_position_bucket (the host fills it with
 * the reference's own fp32 formula so bucket indices are bit-exact); the sign adds nb/2.
 * ------------------------------------------------------------------------------------------ */
/* Per-token inputs of peneo_relpos_buckets and the attention key mask over the concatenated text + visual sequence
 * (T = S + nv; modeling_layoutlmv3.py:1052-1080, 586-676): one launch.  int32 [B, T] outputs, each may be NULL;
 * attention_mask int64 [B, S] (NULL = all ones), bbox int64 [B, S, 4], vx / vy int32 [nv] grid coordinates of the patches. */
int peneo_relpos_inputs(const int64_t* attention_mask, const int64_t* bbox, const int32_t* vx, const int32_t* vy, int B, int S,
                        int nv, int32_t* key_mask, int32_t* pos, int32_t* xs, int32_t* ys, peneo_stream_t stream);
int peneo_relpos_buckets(const int32_t* pos, const int32_t* xs, const int32_t* ys, int B, int T,
                         const uint8_t* lut1, int lut1_len, int half1,
                         const uint8_t* lut2, int lut2_len, int half2,
                         uint8_t* bk1, uint8_t* bkx, uint8_t* bky, peneo_stream_t stream);
/* Packed ("varlen") inference, the row movers (version 113; csrc/rows_pack.hip).  Every buffer is the caller's; nothing is allocated.
 * peneo_pack_plan: order-preserving compaction of key_mask int32 [B, T] (peneo_relpos_inputs; holes allowed), per document:
 *   lens [B] = number of non-zero entries of row b; cu_rows [B + 1] = their exclusive prefix sum (cu_rows[B] = all live rows);
 *   live_t [B, T]: live_t[b, i] = position of the i-th non-zero entry of row b, ascending, and -1 for i >= lens[b].
 *   One launch, no atomics, no workspace.
 * peneo_rows_pack: gathers rows of `row_bytes` bytes (a multiple of 4; contiguous rows) out of src [B, T, row_bytes]:
 *   cu_rows given: dst row cu_rows[b] + i = src row (b, live_t[b, i]) for i < min(lens[b], Tm) (dst has dst_rows rows; a row outside
 *     it is not written; rows of dst that belong to no live token are left alone);
 *   cu_rows NULL: the per-document layout dst [B, Tm, row_bytes], dst_rows = B * Tm: row (b, i) as above for i < lens[b], zeros from
 *     lens[b] on - every row is written (the int32 pos / xs / ys inputs of peneo_relpos_buckets at T = Tm).
 * peneo_rows_unpack: the inverse of the cu_rows layout: writes EVERY row of dst [B, T, row_bytes] - row (b, live_t[b, i]) = src row
 *   cu_rows[b] + i (src has src_rows rows), all other rows zeros.  live_t rows must be ascending, as peneo_pack_plan writes them.
 * Rows move as 16-byte pieces when row_bytes and both base pointers are multiples of 16, else as dwords (4-byte alignment is required). */
int peneo_pack_plan(const int32_t* key_mask, int B, int T, int32_t* lens, int32_t* cu_rows, int32_t* live_t, peneo_stream_t stream);
int peneo_rows_pack(const void* src, const int32_t* live_t, const int32_t* lens, const int32_t* cu_rows, int B, int T, int Tm,
                    int64_t row_bytes, void* dst, int64_t dst_rows, peneo_stream_t stream);
int peneo_rows_unpack(const void* src, int64_t src_rows, const int32_t* live_t, const int32_t* lens, const int32_t* cu_rows, int B, int T,
                      int64_t row_bytes, void* dst, peneo_stream_t stream);
/* bias[b,h,i,j] = scale * (w1[h,bk1] + wx[h,bkx] + wy[h,bky]); any of the three may be NULL.
 * Output layout [B, nh, T, Tp] with Tp = peneo_attn_padded_len(T); columns j >= T and keys with
 * key_mask[b,j] == 0 (may be NULL) hold -1e30, which is how the attention kernels see the padding mask. */
int peneo_relpos_bias_fwd(int dtype, const uint8_t* bk1, const uint8_t* bkx, const uint8_t* bky,
                          const float* w1, int bins1, const float* wx, const float* wy, int bins2,
                          float scale, int B, int nh, int T, int Tp, const int32_t* key_mask, void* bias,
                          peneo_stream_t stream);
/* dw*[h,bin] += scale * sum_{b,i,j in bin} g[b,h,i,j]   (g rows have stride ldg >= T) */
/* Bias-table gradients from L per-layer bf16 dS^T buffers (layout of peneo_attn_bwd's ds_out, `layer_stride`
 * elements apart): dS is summed over the layers in fp32, then binned.  The bucket maps are the TRANSPOSED ones,
 * bkT[b, j, i] = bucket(i, j) (peneo_relpos_buckets on negated positions yields exactly that), stored with row
 * stride Tp: uint8 [B, T, Tp] (columns >= T are ignored), so that 8 buckets are one aligned 8-byte load. */
int peneo_relpos_bias_bwd_layers(const void* ds, int L, int64_t layer_stride, const uint8_t* bk1_t, const uint8_t* bkx_t,
                                 const uint8_t* bky_t, float* dw1, int bins1, float* dwx, float* dwy, int bins2,
                                 float scale, int B, int nh, int T, int Tp, peneo_stream_t stream);
int peneo_relpos_bias_bwd(const float* g, int64_t ldg, const uint8_t* bk1, const uint8_t* bkx, const uint8_t* bky,
                          float* dw1, int bins1, float* dwx, float* dwy, int bins2,
                          float scale, int B, int nh, int T, peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K6 — attention core (modeling_layoutlmv3.py:365-404; the "cogview" softmax :308-321 is exactly
 * softmax).  q/k/v are rows of a [B*T, ld] matrix, head h at columns h*d..;
 *   scores = scale * q.k + bias[b,h,i,j] + key_bias[b,j]      (both optional; -1e30 = masked key)
 * Operands whose reduction index must be contiguous are passed as per-head transposed copies
 * [B, nh, DP, Tp] (DP = peneo_attn_padded_dim(d), Tp = peneo_attn_padded_len(T)) made by
 * peneo_head_transpose: vt for the forward; kt, qt and dot (= d_out transposed) for the backward.
 * `lse` [B, nh, T] fp32 is the per-row log-sum-exp in log2 units (an opaque forward->backward buffer).
 *
 * Dropout on the attention probabilities (modeling_layoutlmv3.py:396-399): the keep bits of one call are made by
 * peneo_attn_drop_words - a pure function of (seed, word index), Bernoulli(1 - p) per bit with p realised to 2^-17 - into
 * `words`, uint32 [B * nh][n_query_blocks][n_key_slots] (peneo_attn_drop_words_dims), and handed to the
 * forward and to the backward of that call (`drop_words`; NULL with drop_p = 0).  One dword holds the 32 queries of a
 * block for one key; the key slots of a 32-key block are ordered as the forward kernel's accumulator registers see them,
 * so the kernels read whole select masks instead of hashing per element (csrc/attention.hip, top).
 * ------------------------------------------------------------------------------------------ */
int peneo_attn_padded_len(int T);
int peneo_attn_padded_dim(int d);
int peneo_head_transpose(int dtype, const void* src, int64_t ld, int B, int nh, int T, int d, void* dst,
                         peneo_stream_t stream);
/* v / vt: bf16 takes V in place (row stride ld_qk, like q and k) and reads V^T with the hardware transpose read, vt may
 * be NULL; fp32 needs vt, the per-head transposed copy from peneo_head_transpose (v is then ignored). */
/* bias_ld: peneo_attn_padded_len(T); since version 113 the forward also takes a larger row stride that is a multiple of 8 (the rows
 * of one document cut out of a bias tensor built for a longer one): the kernels read columns below peneo_attn_padded_len(T) only. */
int peneo_attn_fwd(int dtype, const void* q, const void* k, const void* v, int64_t ld_qk, const void* vt,
                   int B, int nh, int T, int d, float scale, const void* bias, int64_t bias_ld,
                   const float* key_bias, void* out, int64_t ld_out, float* lse, float drop_p, const uint32_t* drop_words,
                   peneo_stream_t stream);
/* Per-document-length ("varlen") form of the forward for packed inference (version 113; csrc/attn_fwd_pipe.hip).  It covers the
 * shape the pipelined kernel covers: bf16, d = 64, bias tensor present, V row-major, no dropout, no key_bias.
 *   lens int32 [B], cu_rows int32 [B + 1] (peneo_pack_plan); Tm: the extent the grid, bias and lse are laid out for (>= max lens).
 *   q / k / v / out: `rows` rows in all; the rows of document b are cu_rows[b] .. cu_rows[b] + n_b - 1, n_b = min(lens[b], Tm).
 *   bias [B, nh, Tm, bias_ld] (bias_ld a multiple of 8, >= Tm rounded up to 32); lse fp32 [B, nh, Tm] (may be NULL).
 * For every document, out and lse rows below n_b hold what peneo_attn_fwd writes for that document alone (B = 1, T = n_b, its slice of
 * the bias with the same bias_ld), bit for bit; keys from n_b on are never read into the softmax, whatever the bias holds there.  Rows
 * from n_b on in lse, and every row of out that belongs to no document, are NOT written.  lens[b] <= 0 is legal: nothing is written for
 * that document.  A document whose rows do not lie inside [0, rows) is skipped whole (nothing read, nothing written).
 * peneo_attn_fwd_varlen_supported is a host-side question (no GPU call): 1 for (PENEO_BF16, 64), 0 for everything else.  An unsupported
 * pair, a NULL operand / bias / lens / cu_rows, operands that are not 16-byte aligned or whose row strides are not whole 16-byte
 * pieces, or a bias_ld too small return PENEO_ERR_INVALID with a peneo_last_error text, nothing launched - never a fallback. */
int peneo_attn_fwd_varlen_supported(int dtype, int d);
int peneo_attn_fwd_varlen(int dtype, const void* q, const void* k, const void* v, int64_t ld_qk, int64_t rows, const int32_t* lens,
                          const int32_t* cu_rows, int B, int nh, int Tm, int d, float scale, const void* bias, int64_t bias_ld,
                          void* out, int64_t ld_out, float* lse, peneo_stream_t stream);
void peneo_attn_drop_words_dims(int T, int* n_query_blocks, int* n_key_slots);
int64_t peneo_attn_drop_words_count(int B, int nh, int T);   /* = B * nh * n_query_blocks * n_key_slots */
int peneo_attn_drop_words(uint32_t* words, int B, int nh, int T, float drop_p, uint32_t seed, peneo_stream_t stream);
/* dq/dk/dv share the q/k/v layout (ld_dqkv).  g_bias (fp32 [B, nh, T, bias_ld], may be NULL) is
 * accumulated with dS so the bias-table gradient can be reduced once per step.
 * `delta` is a [B, nh, T] fp32 scratch.
 * Implementations: with dtype bf16 and `ds_out` and/or `dq_accum` the single-pass kernel runs (S / dP computed once,
 * dK / dV in registers; kt / qt / dot are not read and may be NULL).  dQ then comes from a second kernel that multiplies
 * the stored dS^T slab with K (ds_out given, dq_accum NULL: the faster form) or from fp32 atomics into `dq_accum`
 * (fp32 scratch [B*T, nh*d], overwritten).  Otherwise (fp32, or both NULL) the dQ kernel + the dK/dV kernel run and
 * need the per-head transposed copies kt / qt / dot from peneo_head_transpose.
 * ds_out (single-pass only, may be NULL): bf16 [B, nh, T keys, Tp queries] receives this layer's dS^T (key-major,
 * unscaled); with one such buffer per layer the bias-table gradient is reduced once per step by
 * peneo_relpos_bias_bwd_layers instead of a read-modify-write of g_bias in every layer. */
int peneo_attn_bwd(int dtype, const void* q, const void* k, const void* v, int64_t ld_qkv,
                   const void* kt, const void* qt, const void* dot,
                   const void* out, const void* d_out, int64_t ld_out, const float* lse,
                   int B, int nh, int T, int d, float scale, const void* bias, int64_t bias_ld, const float* key_bias,
                   void* dq, void* dk, void* dv, int64_t ld_dqkv, float* g_bias, float* delta, float* dq_accum,
                   void* ds_out, float drop_p, const uint32_t* drop_words, peneo_stream_t stream);

/* Two-stream attention forward (version 103): LiLT's attention (modeling_lilt.py:269-429) as ONE call - two operand streams
 * (text a, layout b), one shared softmax, two outputs - without the packed copies of peneo_head_concat / peneo_head_split:
 *   scores[b,h,i,j] = (scale_a * q_a) . k_a + (scale_b * q_b) . k_b + key_bias[b,j]
 *   P = softmax over the keys j < T;   out_a = P . v_a,   out_b = P . v_b
 * q_a / k_a / v_a are rows of a [B*T, ld_a] matrix with head h at columns h*d_a.., q_b / k_b / v_b rows of a [B*T, ld_b] matrix with
 * head h at columns h*d_b.. (e.g. column slices of the two fused QKV buffers); out_a / out_b likewise with ld_out_a / ld_out_b.
 * scale_a * q_a and scale_b * q_b are rounded to bf16 before the products, which is what peneo_head_concat writes (exact for powers
 * of two), so the results equal peneo_head_concat x 2 -> peneo_attn_fwd(d = d_a + d_b, scale 1, no bias tensor, key_bias) ->
 * peneo_head_split bit for bit.  key_bias: fp32 [B, Tp], Tp = peneo_attn_padded_len(T), additive (0 / -1e30), may be NULL; keys
 * j >= T are masked by the kernel itself and nothing is promised about, or read from, its padding columns [T, Tp).  A query row
 * whose keys are all masked gives zeros and lse = -1e30, as peneo_attn_fwd does.  lse: fp32 [B, nh, T] in log2 units, the format of
 * peneo_attn_fwd (so that a backward can use it); may be NULL.  No workspace, no allocation, no dropout.
 * peneo_attn2_supported is a host-side question (no GPU call): 1 for (PENEO_BF16, 64, 16), 0 for everything else.
 * peneo_attn2_fwd returns PENEO_ERR_INVALID (with a peneo_last_error text, nothing launched, never a silent fallback) for an
 * unsupported triple, B / nh / T below 1, a null operand or output, an operand or output pointer that is not 16-byte aligned, a row
 * stride whose byte size is not a multiple of 16 or is too small for nh heads, and strides or T whose tile offsets do not fit the
 * kernel's 32-bit lane offsets. */
int peneo_attn2_supported(int dtype, int d_a, int d_b);
int peneo_attn2_fwd(int dtype, const void* q_a, const void* k_a, const void* v_a, int64_t ld_a,
                    const void* q_b, const void* k_b, const void* v_b, int64_t ld_b,
                    int B, int nh, int T, int d_a, int d_b, float scale_a, float scale_b, const float* key_bias,
                    void* out_a, int64_t ld_out_a, void* out_b, int64_t ld_out_b, float* lse, peneo_stream_t stream);

/* Two-stream attention for training (version 104): the forward with attention dropout, and the backward.
 * peneo_attn2_fwd_dropout is peneo_attn2_fwd plus (drop_p, drop_words): drop_words is ONE set of peneo_attn_drop_words in the format
 * peneo_attn_fwd takes; both value streams share the mask; kept probabilities are scaled by 1 / (1 - p) once, on the accumulators;
 * lse stays the pre-dropout log-sum-exp.  drop_p == 0 with NULL words gives the bits of peneo_attn2_fwd; drop_p > 0 with NULL words
 * is PENEO_ERR_INVALID.  With dropout it equals the concat path (peneo_attn_fwd at d_a + d_b with the same words) bit for bit.
 *
 * peneo_attn2_bwd writes the gradients of that contract with respect to the UNSCALED q_a, k_a, v_a, q_b, k_b, v_b (dq_a carries
 * scale_a, dq_b scale_b: what peneo_head_split(dcat, .., scale_a, scale_b) delivers on the concat path, bit for bit for power-of-two
 * scales).  out_a / d_out_a are rows of [B*T, ld_out_a] matrices, out_b / d_out_b of [B*T, ld_out_b]; lse is the forward's;
 * dq_a / dk_a / dv_a are rows of a [B*T, ld_da] matrix with head h at columns h*d_a.., dq_b / dk_b / dv_b of a [B*T, ld_db] matrix
 * (e.g. the column thirds of two fused dqkv buffers).  drop_p / drop_words: what the forward took.
 * workspace: peneo_attn2_bwd_workspace_bytes(B, nh, T) bytes (0 for sizes below 1), 16-byte aligned, owned by the caller: delta
 * (fp32 [B, nh, T]) then the dS^T slab (bf16 [B, nh, T keys, Tp queries]).  It needs no initialisation, carries no state between
 * calls and may be reused by the next call on the same stream; nothing is allocated, so the call is safe under graph capture.
 * Three launches (delta; dK, dV and the slab; dQ from the slab).  PENEO_ERR_INVALID (peneo_last_error names the function, nothing is
 * launched, never a silent fallback) for an unsupported triple, sizes below 1, a null or misaligned operand, output or workspace,
 * row strides that are not multiples of 16 bytes or too small for nh heads, strides or T beyond the kernels' 32-bit lane offsets,
 * and drop_p > 0 without words. */
int peneo_attn2_fwd_dropout(int dtype, const void* q_a, const void* k_a, const void* v_a, int64_t ld_a,
                            const void* q_b, const void* k_b, const void* v_b, int64_t ld_b,
                            int B, int nh, int T, int d_a, int d_b, float scale_a, float scale_b, const float* key_bias,
                            void* out_a, int64_t ld_out_a, void* out_b, int64_t ld_out_b, float* lse,
                            float drop_p, const uint32_t* drop_words, peneo_stream_t stream);
size_t peneo_attn2_bwd_workspace_bytes(int B, int nh, int T);
int peneo_attn2_bwd(int dtype,
                    const void* q_a, const void* k_a, const void* v_a, int64_t ld_a,
                    const void* q_b, const void* k_b, const void* v_b, int64_t ld_b,
                    const void* out_a, const void* d_out_a, int64_t ld_out_a,
                    const void* out_b, const void* d_out_b, int64_t ld_out_b,
                    const float* lse, int B, int nh, int T, int d_a, int d_b, float scale_a, float scale_b,
                    const float* key_bias,
                    void* dq_a, void* dk_a, void* dv_a, int64_t ld_da,
                    void* dq_b, void* dk_b, void* dv_b, int64_t ld_db,
                    void* workspace, float drop_p, const uint32_t* drop_words, peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K11 + K12 (+ K13) — handshaking + the pair-classifier heads + class-weighted CE, fused
 * (model/peneo_decoder.py:149-177, 231-292, 315-336, 355-428; model/custom_loss.py:189-202).
 *
 * ab [B, N, 2D]: a_i = W_c[:, :D] h_i  (cols 0..D) and b_j = W_c[:, D:] h_j + bias_c (cols D..2D),
 * so that  combine_fc(cat(h_i, h_j)) = a_i + b_j.  For every packed upper-triangular pair
 * p(i,j) = i*N - i(i-1)/2 + (j-i):  x = SiLU(a_i + b_j);  per head: SiLU(W1_h x + b1_h) -> W2_h . + b2_h.
 * ------------------------------------------------------------------------------------------ */
typedef struct peneo_pair_heads_desc {
  int num_heads;                       /* <= PENEO_MAX_HEADS */
  int D;                               /* decoder hidden size (multiple of 32) */
  int classes[PENEO_MAX_HEADS];        /* 2,3,3,3,3 */
  const void* w_packed;                /* from peneo_pair_heads_pack (both layers, MFMA fragment order) */
  const float* b1;                     /* [num_heads * D] */
  const float* b2;                     /* [sum classes] */
  float drop_p;                        /* K12 dropout between the two classifier layers (model/peneo_decoder.py:261); 0 = off.
                                          keep(b, p, n) is a pure function of (drop_seed, document, pair, hidden column):
                                          the backward entry points regenerate it from the same two numbers.  Realised as
                                          round(p * 2^16) / 2^16 with the matching 1 / (1 - p) scale */
  uint32_t drop_seed;
} peneo_pair_heads_desc;

/* Host-side query (no GPU call, version 108): 1 where peneo_pair_heads_pack + peneo_pair_heads_fwd have a kernel for
 * (dtype, D, num_heads), else 0.  D <= 512: D / 16 in {2, 4, 6, 8, 12, 16, 24, 32}, fp32 and bf16.  512 < D <= 1024: bf16 only, D a
 * multiple of 64 (pair_heads_wide.hip: four waves of 32 pairs, a ring of two weight slabs; five heads fit at D = 1024, eight up to
 * D = 960).  Everything else - fp32 above 512 among it - makes the two calls return PENEO_ERR_INVALID (and packed_bytes 0 above 512);
 * a caller that needs such a width materialises the pair activations (peneo_pair_x_fwd + peneo_gemm). */
int peneo_pair_heads_supported(int dtype, int D, int num_heads);
size_t peneo_pair_heads_packed_bytes(int dtype, int num_heads, int D);
/* w1[h] : [D, D] row-major fp32 (nn.Linear weight), w2[h] : [classes[h], D] fp32;
 * w1 / w2 / classes are HOST arrays (of device pointers / ints) with num_heads entries */
int peneo_pair_heads_pack(int dtype, const float* const* w1, const float* const* w2, const int* classes,
                          int num_heads, int D, void* packed, peneo_stream_t stream);

typedef struct peneo_pair_loss {
  const int64_t* tags[PENEO_MAX_HEADS];   /* [B, P] label maps (data/collator.py:170-204); NULL = no loss */
  const float* class_weight[PENEO_MAX_HEADS]; /* [classes[h]] fp32 device */
  float* partials;                        /* [peneo_pair_loss_partials(B, N)][32] fp32 workspace: one row per workgroup =
                                             sum_p w[tag]*nll [8] | sum_p w[tag] [8] | sum_p dlogits [16]; reduced by
                                             peneo_loss_finish (deterministic, no atomics) */
  float* dlogits[PENEO_MAX_HEADS];        /* optional [B, P, classes[h]] fp32: w[tag] * (softmax - onehot) (unnormalised) */
} peneo_pair_loss;
int64_t peneo_pair_loss_partials(int B, int N);

/* logits[h] : [B, P, classes[h]] fp32, contiguous, P = N (N + 1) / 2 (may be NULL when only the loss is wanted) */
int peneo_pair_heads_fwd(int dtype, const void* ab, int B, int N, const peneo_pair_heads_desc* desc,
                         float* const* logits /* host array of num_heads device pointers, or NULL */,
                         const peneo_pair_loss* loss, peneo_stream_t stream);

/* Length-aware inference form (version 111, opt-in): peneo_pair_heads_fwd that skips the pairs touching a document's padding.
 * lens [B] int32 on the device, clamped to [0, N] by the kernels; n_b = the clamped length of document b, P_b = n_b (n_b + 1) / 2.
 * WALK: document b is walked as the n_b-token document it is - workgroup x owns its local pairs q in [256 x, 256 x + 256), (i, j) is
 *   pair q of an n_b-token triangle, live while q < P_b - and everything indexed by the pair (logits, tags) keeps the N-packed index
 *   p(i, j) above; ab keeps its [B, N, 2D] strides.  The grid stays (ceil(P / 256), B): the lengths are never read by the host.  A
 *   workgroup without a live pair leaves at once, storing a zero row of loss partials.  With n_b = N the walk is peneo_pair_heads_fwd's.
 * LIVE PAIRS (j < n_b): everything of peneo_pair_heads_fwd holds - the packed weights of peneo_pair_heads_pack, the widths and dtypes
 *   of peneo_pair_heads_supported, and the logits bit for bit (the arithmetic of a pair does not depend on where it is walked).
 * PADDED PAIRS (j >= n_b) hold the background row in every requested map: class 0 = 0.0f, every other class = PENEO_PAIR_PAD_LOGIT.
 *   Their argmax is tag 0 with score 1, so peneo_spots_compact* and every other consumer of the [B, P, C] maps work unchanged.  (A fill
 *   launch of the same call, ahead of the main kernel on the stream: every element of every requested map is defined after the call.)
 * LOSS (`loss` may be NULL; loss->dlogits[h] must be NULL): the peneo_pair_loss_partials(B, N) partial rows sum w nll, w and the class
 *   sums over the LIVE PAIRS ONLY; rows of workgroups without a live pair are zero.  The rows of document b are, row by row, the
 *   bits peneo_pair_heads_fwd writes for that document cropped to n_b tokens.  peneo_loss_finish over them is therefore A DIFFERENT
 *   NUMBER from the reference's loss and from peneo_pair_heads_fwd's, which average over the padded pairs (label 0) as well: it is the
 *   class-weighted mean over the pairs of real tokens.  (With no live pair in the whole batch the mean is 0 / 0.)
 * Returns PENEO_ERR_INVALID with a peneo_last_error() text, nothing launched, for desc->drop_p != 0, a NULL lens, a non-NULL dlogits
 * and an unsupported (dtype, D, heads).  No workspace, no allocation, no host synchronisation; safe under graph capture; nothing
 * order-dependent is launched.
 * peneo_pair_lens_from_mask: lens[b] = 1 + the last index j < N with mask[b * ld + j] != 0, 0 if there is none, N for a NULL mask (one
 * launch; mask int64 on the device, row stride ld >= N).  A mask that is not a prefix yields a superset of its tokens, never a subset. */
#define PENEO_PAIR_PAD_LOGIT (-1e30f)
int peneo_pair_lens_from_mask(const int64_t* mask /* [B, ld] or NULL */, int64_t ld, int B, int N,
                              int32_t* lens, peneo_stream_t stream);
int peneo_pair_heads_fwd_lens(int dtype, const void* ab, int B, int N, const int32_t* lens,
                              const peneo_pair_heads_desc* desc, float* const* logits,
                              const peneo_pair_loss* loss, peneo_stream_t stream);

/* The same launch for a train step whose backward is peneo_pair_bwd_saved (bf16, D = 384: peneo_pair_save_supported).  It walks the
 * pairs in the backward's blocks of 8 rows i x 16 columns j and leaves what the backward would otherwise rebuild:
 *   act    [peneo_pair_save_bytes(B, N, num_heads, D)]: per document, block, 32-unit slab of the num_heads * D hidden units and
 *          group of 32 pairs one 2 KiB record: the classifiers' pre-activations z = W1_h x + b1_h as f16 [32 pairs][32 units], a
 *          unit the K12 dropout drops stored as -30000 (SiLU and SiLU' of that are 0: the backward needs no mask and runs no dropout
 *          chain) - what autograd under autocast saves of model/peneo_decoder.py:253-271, 2 bytes per pair and hidden unit;
 *   x_rows [B * peneo_pair_bwd_rows(N), D] bf16: x = SiLU(a_i + b_j) in block order (the B operand of dW1 = dz^T x).
 * Logits, loss partial rows and dlogits are those of peneo_pair_heads_fwd bit for bit (same arithmetic per pair, indexed by the
 * packed pair index); `loss->partials` has peneo_pair_loss_partials_save(B, N) rows here.  16-byte aligned buffers.
 * RANGE: z is stored as f16 and a dropped unit as -30000 + W1 x, so the saved form assumes |W1 x + b1| < 30000 for every pair and
 * hidden unit (then a dropped z stays below -20 where SiLU and SiLU' are 0 in f16, and nothing reaches the f16 limit 65504: an
 * overflow to -inf would give -inf * 0 = NaN in peneo_pair_bwd_saved).  With LayerNorm-ed inputs and initializer_range-scale
 * weights |z| is O(10); a caller that cannot bound it runs peneo_pair_heads_fwd + peneo_pair_bwd_fused (the recomputing form has
 * no such limit; PEneoDecoder.save_pair_act = False / PENEO_PAIR_SAVE=0). */
int peneo_pair_save_supported(int dtype, int D, int num_heads);
size_t peneo_pair_save_bytes(int B, int N, int num_heads, int D);
int64_t peneo_pair_loss_partials_save(int B, int N);
int peneo_pair_heads_fwd_save(int dtype, const void* ab, int B, int N, const peneo_pair_heads_desc* desc,
                              float* const* logits, const peneo_pair_loss* loss, void* act, void* x_rows,
                              peneo_stream_t stream);

/* The e4m3 form of the saved activations (version 109, opt-in): the same launch - same walk, same arithmetic, same K12 dropout; logits,
 * loss partial rows, dlogits and x_rows are the bytes peneo_pair_heads_fwd_save writes - with one byte per pair and hidden unit in `act`:
 *   act    [peneo_pair_save_e4m3_bytes(B, N, num_heads, D)] = half of peneo_pair_save_bytes: per document, block, 32-unit slab and
 *          group of 32 pairs (the order of the f16 form) one 1 KiB record of 32 x 32 e4m3fn bytes.
 * VALUE: each byte is e4m3fn(RNE(clamp(v, -448, 448))) of the f16 value v peneo_pair_heads_fwd_save stores for that pair and unit (a
 *   conversion of the f16 value, not of the fp32 accumulator: no double rounding to allow for).  The clamp is explicit in the kernel.  A
 *   dropped unit (-30000 + W1 x in the f16 form) is therefore -448: sigmoid(-448) is exactly 0 in the backward's fp32 arithmetic (exp2
 *   overflows to +inf, its reciprocal is 0), so y = 0 and SiLU' = 0 with no mask, as in the f16 form.
 * RANGE: a kept |z| above 448 saturates to +-448: the backward's result for that unit is finite and off by the excess, never NaN.
 *   Pre-activations are O(10) with LayerNorm-ed inputs; the f16 form's bound (|W1 x + b1| < 30000) applies unchanged.
 * LAYOUT of a record: [16 rows][64 bytes].  Pair p = 8 qd + 4 h + e of the group (qd = 0..3, h = 0..1, e = 0..3) is in row
 *   8 (qd >> 1) + 4 h + 2 (qd & 1) + (e >> 1); a row holds, per hidden unit, the two bytes (pair with e even, pair with e odd), and the
 *   32 units of the slab stand in the row as eight-byte quads: units 8 G + 4 f + 0..3 (G = 0..3, f = 0..1) at byte 16 (2 (G >> 1) + f)
 *   + 8 (G & 1).  (The backward's transposing LDS read moves 16-bit elements: a two-pair element per unit gives every lane eight pairs
 *   of its unit per read, and the four rows a read touches are 256 consecutive bytes.)
 * peneo_pair_save_e4m3_supported: host-side query (no GPU call), 1 exactly where peneo_pair_save_supported is 1 (bf16, D = 384).
 * Returns PENEO_ERR_INVALID with a peneo_last_error() text for an unsupported (dtype, D, heads), a NULL act / x_rows or a buffer that is
 * not 16-byte aligned.  The MXFP8 train forward (peneo_pair_heads_fwd_mxfp8_save) keeps writing f16 records. */
int peneo_pair_save_e4m3_supported(int dtype, int D, int num_heads);
size_t peneo_pair_save_e4m3_bytes(int B, int N, int num_heads, int D);
int peneo_pair_heads_fwd_save_e4m3(int dtype, const void* ab, int B, int N, const peneo_pair_heads_desc* desc,
                                   float* const* logits, const peneo_pair_loss* loss, void* act, void* x_rows,
                                   peneo_stream_t stream);

/* MXFP8 inference form of the same heads (pair_heads_mx.hip; eval only: no dropout, no dlogits, no backward).
 * Both first-layer operands, the rows of W1cat [num_heads * D, D] and every pair's x = SiLU(a_i + b_j) (fp32 from the bf16 `ab`),
 * are quantized to OCP MX v1.0 MXFP8: per block of 32 consecutive elements along D, scale 2^e with e = floor(log2(amax)) - 8
 * clamped to the E8M0 range [-127, 127] (an all-zero block: e = -127), elements e4m3fn(RNE(clamp(v / 2^e, -448, 448))).
 * z = W1_h x accumulates in fp32 on the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4); + b1, SiLU, then the second layer and
 * the loss of peneo_pair_heads_fwd (y as bf16, W2 bf16, fp32 accumulate, + b2).  256 pairs per workgroup as there:
 * `loss->partials` has peneo_pair_loss_partials(B, N) rows.
 *
 * peneo_mxfp8_quantize_rows: src [rows, cols] fp32 row-major (cols % 32 == 0, 16-byte aligned) -> q [rows, cols] e4m3 bytes and
 * scales [rows, cols / 32] E8M0 bytes, both caller-owned; the quantizer the pack and the kernel apply.
 * peneo_pair_mxfp8_supported: host-side query (no GPU call): 1 when D % 64 == 0, 64 <= D <= 512, 1 <= num_heads <= PENEO_MAX_HEADS
 * and the weight ring fits in LDS, else 0.
 * peneo_pair_heads_pack_mxfp8: w1 / w2 / classes as for peneo_pair_heads_pack -> `packed` [peneo_pair_heads_mxfp8_packed_bytes]
 * (16-byte aligned; 0 bytes = unsupported shape): per 32-row slab the e4m3 first-layer fragments, their E8M0 scales and the bf16
 * second-layer fragments, in fragment order.  Once per weight version.
 * peneo_pair_heads_fwd_mxfp8: ab [B, N, 2D] bf16; `desc` as for peneo_pair_heads_fwd with w_packed from the pack above and
 * drop_p == 0; `loss` (may be NULL) with every dlogits[h] NULL.  Other arguments give PENEO_ERR_INVALID. */
int peneo_mxfp8_quantize_rows(const float* src, int64_t rows, int64_t cols, void* q_e4m3, void* scales_e8m0,
                              peneo_stream_t stream);
int peneo_pair_mxfp8_supported(int D, int num_heads);
size_t peneo_pair_heads_mxfp8_packed_bytes(int num_heads, int D);
int peneo_pair_heads_pack_mxfp8(const float* const* w1, const float* const* w2, const int* classes, int num_heads, int D,
                                void* packed, peneo_stream_t stream);
int peneo_pair_heads_fwd_mxfp8(const void* ab, int B, int N, const peneo_pair_heads_desc* desc,
                               float* const* logits /* host array of num_heads device pointers, or NULL */,
                               const peneo_pair_loss* loss, peneo_stream_t stream);

/* MXFP8 inference form of the heads at decoder widths 512 < D <= 1024 (version 112; pair_heads_mx_wide.hip): the contract of
 * peneo_pair_heads_fwd_mxfp8 above, word for word - the same quantizer on both first-layer operands, the scaled MFMAs in the same
 * k-step order, + b1, SiLU, the bf16 second layer, + b2, fp32 logits, the loss rows of 256 pairs (`loss->partials` has
 * peneo_pair_loss_partials(B, N) rows; single-writer, no atomics, no workspace, no allocation) - on a kernel of its own: four waves
 * that hold two groups of 32 pairs each, so that 256 pairs share one pass over every weight slab.  The narrow entry points keep
 * answering exactly as before (0 / PENEO_ERR_INVALID above D = 512).
 * peneo_pair_mxfp8_wide_supported: host-side query (no GPU call): 1 when D % 64 == 0, 512 < D <= 1024, 1 <= num_heads <=
 * PENEO_MAX_HEADS and the ring of three weight slabs + the b1 table fit in 160 KiB of LDS (true for every such D up to 8 heads), else 0.
 * peneo_pair_heads_pack_mxfp8_wide: as peneo_pair_heads_pack_mxfp8 -> `packed` [peneo_pair_heads_mxfp8_wide_packed_bytes]
 * (16-byte aligned; 0 bytes = unsupported shape): the same slab contents at a stride of a whole number of 4 KiB.  The two packs are
 * not interchangeable; a pointer carries no size, so a wrong one is NOT detectable.
 * peneo_pair_heads_fwd_mxfp8_wide: the arguments of peneo_pair_heads_fwd_mxfp8 with w_packed from the pack above.  PENEO_ERR_INVALID
 * with a peneo_last_error() text naming the argument: drop_p != 0, a non-NULL dlogits[h], a (D, num_heads) the query refuses. */
int peneo_pair_mxfp8_wide_supported(int D, int num_heads);
size_t peneo_pair_heads_mxfp8_wide_packed_bytes(int num_heads, int D);
int peneo_pair_heads_pack_mxfp8_wide(const float* const* w1, const float* const* w2, const int* classes, int num_heads, int D,
                                     void* packed, peneo_stream_t stream);
int peneo_pair_heads_fwd_mxfp8_wide(const void* ab, int B, int N, const peneo_pair_heads_desc* desc,
                                    float* const* logits /* host array of num_heads device pointers, or NULL */,
                                    const peneo_pair_loss* loss, peneo_stream_t stream);

/* MXFP8 train forward of the same heads (version 105): the first layer of peneo_pair_heads_fwd_mxfp8 - same quantizer, same scaled
 * MFMAs in the same order - on the walk of peneo_pair_heads_fwd_save, leaving what peneo_pair_bwd_saved reads.
 * peneo_pair_mxfp8_save_supported: host-side query (no GPU call): 1 exactly when peneo_pair_save_supported(PENEO_BF16, D, num_heads)
 * and peneo_pair_mxfp8_supported(D, num_heads) are both 1 (D = 384), else 0.
 * peneo_pair_heads_fwd_mxfp8_save: ab [B, N, 2D] bf16; `desc` as for peneo_pair_heads_fwd with w_packed from
 * peneo_pair_heads_pack_mxfp8 and drop_p in [0, 1); act / x_rows as for peneo_pair_heads_fwd_save (both required, 16-byte aligned);
 * `loss` (may be NULL) may carry dlogits; `loss->partials` has peneo_pair_loss_partials_save(B, N) rows.  Per pair:
 *   x = SiLU(a_i + b_j) in fp32; x_rows receives bf16(x), the bytes peneo_pair_heads_fwd_save writes;
 *   z = Q(W1) Q(x) + b1, Q the MXFP8 quantizer above (with drop_p = 0 the logits are those of peneo_pair_heads_fwd_mxfp8 bit for bit);
 *   the K12 dropout mask of (drop_seed, drop_p) is the one the bf16 forwards draw; the record holds f16(z) of a kept unit and
 *   -30000 of a dropped one, in the layout of peneo_pair_heads_fwd_save; y = bf16(SiLU(z)), 0 where dropped;
 *   logits = s (W2 y) + b2, s = 65536 / (65536 - round(drop_p 2^16)); loss rows and dlogits as peneo_pair_heads_fwd defines them.
 * Pairs of a block outside the triangle compute finite values that nobody reads; nothing is written for the absent second block of
 * the last workgroup.  The RANGE note of peneo_pair_heads_fwd_save applies (|z| < 30000).
 * GRADIENT: peneo_pair_bwd_saved on these buffers gives straight-through gradients: du = dz W1 and dW1 = dz^T x use the bf16 weights
 * and the bf16 x, while SiLU' and the loss are taken at this forward's quantized z.
 * Other arguments give PENEO_ERR_INVALID: an unsupported (D, num_heads), a NULL act / x_rows, a misaligned buffer, drop_p outside
 * [0, 1).  A w_packed that came from peneo_pair_heads_pack (the bf16 pack) is NOT detectable: the call takes a pointer without a
 * size; its slabs would be read at the MXFP8 stride (in bounds: the bf16 pack is the larger one) and give meaningless logits. */
int peneo_pair_mxfp8_save_supported(int D, int num_heads);
int peneo_pair_heads_fwd_mxfp8_save(const void* ab, int B, int N, const peneo_pair_heads_desc* desc,
                                    float* const* logits /* host array of num_heads device pointers, or NULL */,
                                    const peneo_pair_loss* loss, void* act, void* x_rows, peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Block-scaled (OCP MX v1.0) FP8 GEMM:  C[m, n] = epilogue( sum_k A^(m, k) * B^(n, k) ),  x^ = e4m3 element * 2^(E8M0 byte - 127)
 * Both operands are k-major, as every forward nn.Linear (y = x W^T): A_q [M, K] e4m3 bytes with A_s [M, K / 32] E8M0 bytes, B_q [N, K]
 * with B_s [N, K / 32], all contiguous, in the format peneo_mxfp8_quantize_rows writes (blocks of 32 consecutive k).  fp32 accumulation
 * on v_mfma_scale_f32_32x32x64_f8f6f4; no split-k, no workspace, no allocation.  C [M, ldc] is bf16 or fp32 (`c_dtype`).
 * Epilogue (`ep` may be NULL):  v = alpha * acc (+ bias[n]) ; v = act(v) (PENEO_ACT_NONE or PENEO_ACT_GELU; the erf form, evaluated as
 * peneo_gemm does for the same c_dtype) ; v += residual[m, n] (dtype c_dtype) ; C <- v.  Any other field of `ep` being set (preact,
 * grad_src, drop_p > 0, accumulate, pair_dz, a_colsum, another act) is PENEO_ERR_INVALID.
 * MX output (C_q, C_s both non-NULL or both NULL): C_q [M, N] e4m3 and C_s [M, N / 32] E8M0 receive the quantization, along n, of the
 * value AS ROUNDED TO bf16 -- byte for byte peneo_mxfp8_quantize_rows_bf16 of a bf16 C -- so that the next GEMM (FFN1 -> FFN2) reads
 * it without a quantizer launch; C may then be NULL and is not written.
 * Alignment: A_q, B_q, C, bias, residual 16 bytes; A_s, B_s, C_q 4 bytes; ldc and ld_res multiples of 4 and >= N.
 * Rows of A past M and of B past N are neither read as data nor written.
 * peneo_gemm_mxfp8_supported: host-side query (no GPU call): 1 when M >= 1 (ceil(M / 128) * ceil(N / 128) < 2^31), N >= 32 with N % 32 == 0 and
 * K >= 128 with K % 128 == 0 (a K stage of the kernel is 128 deep and holds one dword of scales per row), else 0.
 * peneo_mxfp8_quantize_rows_bf16: peneo_mxfp8_quantize_rows for a bf16 source [rows, ld] (ld >= cols, ld % 8 == 0, 16-byte aligned);
 * q [rows, cols] and scales [rows, cols / 32] contiguous.  A bf16 value gives exactly the bytes its fp32 image gives there.
 * ------------------------------------------------------------------------------------------ */
int peneo_mxfp8_quantize_rows_bf16(const void* src, int64_t rows, int64_t cols, int64_t ld, void* q_e4m3, void* scales_e8m0,
                                   peneo_stream_t stream);
/* peneo_layernorm_fwd (bf16, contiguous [rows, H] x and y, no dropout) that also writes the MX copy of y: y, mean, rstd bit for bit those
 * of peneo_layernorm_fwd, and y_q [rows, H] / y_s [rows, H / 32] byte for byte peneo_mxfp8_quantize_rows_bf16(y), in one launch.
 * x, y, gamma, beta 16-byte aligned, y_q 8-byte aligned.  peneo_layernorm_mxfp8_supported (host-only): H % 256 == 0 and H <= 1024. */
int peneo_layernorm_mxfp8_supported(int H);
int peneo_layernorm_fwd_mxfp8(const void* x, void* y, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                              int64_t rows, int H, void* y_q, void* y_s, peneo_stream_t stream);
int peneo_gemm_mxfp8_supported(int M, int N, int K);
int peneo_gemm_mxfp8(int M, int N, int K, const void* A_q, const void* A_s, const void* B_q, const void* B_s,
                     void* C, int64_t ldc, int c_dtype, const peneo_gemm_epilogue* ep, void* C_q, void* C_s,
                     peneo_stream_t stream);

/* --- building blocks of the chunked backward (rows i0..i1 of the pair triangle = pairs
 *     p(i0,i0) .. p(i1,i1)-1 of one document) ------------------------------------------- */
/* x[p - p0, :] = SiLU(a_i + b_j)  [npairs, D];  pre (may be NULL) receives a_i + b_j itself, the `grad_src` that lets the
 * dx GEMM epilogue apply SiLU' (peneo_gemm_epilogue.grad_src / grad_act) */
int peneo_pair_x_fwd(int dtype, const void* ab_doc, int N, int D, int i0, int i1, void* x, void* pre, peneo_stream_t stream);
/* du = dx * SiLU'(a_i + b_j)  (or du = dx when `premultiplied`: the GEMM epilogue already applied the factor);
 * d_ab_doc[i, :D] += sum_j du ; d_ab_doc[j, D:] += sum_i du   (fp32 [N, 2D]) */
int peneo_pair_x_bwd(int dtype, const void* ab_doc, int N, int D, int i0, int i1, const void* dx, float* d_ab_doc,
                     int premultiplied, peneo_stream_t stream);
/* For the [npairs, nh*D] pre-activations z of all heads' first layers (in place):
 *   y = SiLU(z);  dy[p, h*D+k] = sum_c scale_h * dlogits_h[p, c] * w2_h[c, k];  dz = dy * SiLU'(z)  (written over z)
 * and the reductions over pairs needed by the parameter gradients are accumulated into `workspace`
 * [peneo_pair_dz_workspace_bytes / (16 * nh*D)][4 * nh*D] fp32 (zero it once per step; sum its rows with peneo_colsum at the end):
 *   row block c (c = 0..2): sum_p scale_h*dlogits_h[p,c] * y[p, :]   -> dW2_h[c, :] = block[c][h*D : (h+1)*D]
 *   row block 3            : sum_p dz[p, :]                          -> db1
 * scale[h] (= d(loss) * loss_ratio_h / den_h) is a device vector. */
typedef struct peneo_pair_dz_args {
  int num_heads; int D; int classes[PENEO_MAX_HEADS];
  const float* dlogits[PENEO_MAX_HEADS];  /* [npairs, classes[h]] (already offset to the chunk) */
  const float* w2[PENEO_MAX_HEADS];       /* [classes[h], D] fp32 */
  const float* scale;                     /* [num_heads] device fp32 */
  float drop_p;                           /* the forward's K12 dropout (peneo_pair_heads_desc): y and dz are masked and scaled */
  uint32_t drop_seed;
  int drop_doc;                           /* chunked entry points: document index b and packed index p of the chunk's first */
  int64_t drop_pair0;                     /* pair, i.e. what the forward hashed (peneo_pair_bwd_fused walks all of them itself) */
} peneo_pair_dz_args;
size_t peneo_pair_dz_workspace_bytes(int num_heads, int D);
int peneo_pair_dz(int dtype, void* z_inout, int64_t npairs, const peneo_pair_dz_args* args, float* workspace,
                  peneo_stream_t stream);

/* dz of the pairs of rows i0..i1 of one document WITHOUT x or z in memory (bf16 only): x = SiLU(a_i + b_j) is rebuilt in
 * registers, z = x W1cat^T + b1 comes off the matrix cores with lane = hidden column, and the same kernel turns it into
 * dz [npairs, nh*D] and adds the dW2 / db1 column sums to `workspace` (layout of peneo_pair_dz; only its first 256 rows
 * are touched, as by the pair_dz epilogue of peneo_gemm: 256 rows suffice for a workspace these two share).  `w_packed` is the
 * fragment-packed weight buffer of peneo_pair_heads_pack (its second-layer fragments are not used here).
 * With x_out / pre_out it also leaves x = SiLU(a_i + b_j) and a_i + b_j for the dW1 / dx GEMMs (no peneo_pair_x_fwd pass).
 * Replaces peneo_pair_x_fwd + the first-layer GEMM + peneo_pair_dz of the chunked backward
 * (the autograd graph through model/peneo_decoder.py:269-336).
 * Widths: D / 16 in {2, 4, 6, 8, 12, 16, 24, 32} (eight waves, 256 pairs a workgroup), and since version 110 512 < D <= 1024 with
 * D % 64 == 0 (four waves, one per SIMD, the same 256 pairs in two rounds of 128; the packed image of peneo_pair_heads_pack for these
 * widths; same arguments, same checks, same workspace rows).  peneo_pair_dz_fused_supported says where a kernel exists. */
int peneo_pair_dz_fused(int dtype, const void* ab_doc, int N, int D, int i0, int i1, const void* w_packed, const float* b1,
                        const peneo_pair_dz_args* args, void* dz, float* workspace,
                        void* x_out /* optional [npairs, D]: what peneo_pair_x_fwd would write */,
                        void* pre_out /* given together with x_out */, peneo_stream_t stream);
/* 1 exactly where peneo_pair_dz_fused has a kernel (version 110; host only, no GPU call): bf16 with the widths above, 1..8 heads,
 * LDS permitting; 0 for everything else (fp32, other widths, no heads). */
int peneo_pair_dz_fused_supported(int dtype, int D, int num_heads);

/* Decoder backward through the pair space in ONE kernel (bf16; D / 16 in {2, 4, 8, 24, 32}): for all pairs (i, j), i <= j, of
 * all B documents it rebuilds x = SiLU(a_i + b_j) in registers, computes z = x W1cat^T + b1 and dz (as peneo_pair_dz_fused),
 * du = dz W1cat on the matrix cores with the accumulator kept in registers over all hidden units, and
 *   d_ab[b, i, :D] = sum_j du * SiLU'(a_i + b_j),  d_ab[b, j, D:] = sum_i du * SiLU'(a_i + b_j)   (fp32, overwritten; per-block
 *   partial rows + one reduction launch, no atomics),
 * plus the dW2 / db1 column sums into `workspace` (layout of peneo_pair_dz, first 256 rows).  It leaves dz [B * rows, nh*D]
 * and x [B * rows, D] (bf16) for the one remaining GEMM dW1cat = dz^T x.  rows = peneo_pair_bwd_rows(N): the pairs are
 * walked in blocks of 8 rows i x 16 columns j of the triangle (blocks on the diagonal / the last row of blocks carry
 * pairs outside it: their dz rows are zero, their x rows finite), both buffers in that block order.
 * args->dlogits[h] is the whole [B, P, classes[h]] map, args->scale the device vector of peneo_loss_finish.
 * Replaces, per document, peneo_pair_x_fwd + peneo_pair_dz_fused + the du GEMM (grad_src epilogue) + peneo_pair_x_bwd:
 * the autograd graph through model/peneo_decoder.py:149-177 and :231-292 except the first-layer weight gradient.
 * `w_packed`: peneo_pair_bwd_pack (per 32-unit slab the B-operand fragments of both products).
 * peneo_pair_bwd_supported: 1 when the fused launch exists for (dtype, D) AND its LDS image fits `num_heads` heads (the per-column
 * table grows with the head count: D = 512 holds 5 heads, not 6); num_heads <= 0 asks about (dtype, D) only.  On 0 a caller runs
 * the per-document chain (peneo_pair_x_fwd / peneo_pair_dz_fused / peneo_gemm / peneo_pair_x_bwd). */
int peneo_pair_bwd_supported(int dtype, int D, int num_heads);
int64_t peneo_pair_bwd_rows(int N);
size_t peneo_pair_bwd_packed_bytes(int num_heads, int D);
int peneo_pair_bwd_pack(const float* const* w1 /* host array of num_heads device pointers to [D, D] fp32 */, int num_heads, int D,
                        void* packed, peneo_stream_t stream);
size_t peneo_pair_bwd_partial_bytes(int B, int N, int D);   /* `partials`: per-block partial rows of d_a / d_b (scratch) */
int peneo_pair_bwd_fused(int dtype, const void* ab, int B, int N, int D, const void* w_packed, const float* b1,
                         const peneo_pair_dz_args* args, void* dz, void* x, float* d_ab, float* workspace,
                         float* partials, peneo_stream_t stream);

/* peneo_pair_bwd_fused for a forward that ran as peneo_pair_heads_fwd_save (bf16, D = 384): `act` holds the pre-activation z of
 * every pair and hidden unit (dropout applied), so this launch computes y = SiLU(z) and dz = (g W2 / (1 - p)) SiLU'(z) from it, runs
 * neither the first-layer product (24 of the 51 MFMAs per 32 pairs x 32 units) nor a dropout chain, and leaves the same dz
 * [B * rows, nh*D], d_ab and workspace sums (x_rows was written by the forward).  `w_packed`: peneo_pair_bwd_pack.  Results differ
 * from peneo_pair_bwd_fused by the f16 rounding of the saved z (what autograd under autocast would have saved; 5e-4 relative on dz). */
int peneo_pair_bwd_saved(int dtype, const void* ab, int B, int N, int D, const void* w_packed,
                         const peneo_pair_dz_args* args, const void* act, void* dz, float* d_ab, float* workspace,
                         float* partials, peneo_stream_t stream);

/* peneo_pair_bwd_saved on the 1 KiB e4m3 records of peneo_pair_heads_fwd_save_e4m3 (version 109): the same launch with one LDS-DMA piece
 * per slab and group instead of two and a 16 KiB record ring instead of 32.  A value is decoded e4m3 -> fp32 (exact) and then goes
 * through the statements the f16 form runs on its f16 -> fp32 value: on records that hold the same values the two give the same dz and
 * d_ab bit for bit.  Same arguments, same workspace rows (peneo_pair_bwd_workspace_rows), same deterministic mode: a row per workgroup
 * under peneo_set_deterministic(1 / 2), and in the default mode the call counts in peneo_order_dependent_launches as the f16 form does. */
int peneo_pair_bwd_saved_e4m3(int dtype, const void* ab, int B, int N, int D, const void* w_packed,
                              const peneo_pair_dz_args* args, const void* act, void* dz, float* d_ab, float* workspace,
                              float* partials, peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K13 — loss finish: reduces the per-workgroup partial rows of peneo_pair_heads_fwd:
 *   loss_h = num_h / den_h ; total = sum_h ratio_h * loss_h ; scale_h = ratio_h / den_h (the factor the
 *   backward applies to the un-normalised dlogits) ; dl_sum[c] = sum_p dlogits[p, c] (second-layer bias grads).
 * out: [num_heads + 1] = per-head losses then the total.  (model/peneo_decoder.py:315-336,375-428)
 * inv_den (optional, [num_heads]) = 1 / den_h: the factor for a gradient arriving on a per-head loss itself.
 * ------------------------------------------------------------------------------------------ */
int peneo_loss_finish(const float* partials, int64_t n_partials, const float* ratio, int num_heads, int total_classes,
                      float* out, float* scale, float* dl_sum, float* inv_den, peneo_stream_t stream);
/* K13, OHEM branch ("next" row f.3): CrossEntropyLossOHEM.forward with num_hard_positive / num_hard_negative != -1
 * (model/custom_loss.py:204-288) as executed by the reference, over the n = B*P flattened pairs of one head:
 * per-pair weighted CE, positives (tag != 0) and negatives sorted by descending loss (stable: equal losses keep the
 * flattened order), k = min(count, num_hard); k <= 0 or k == count keeps every element of the class, otherwise the kept
 * elements are sorted[idx[:k]] (the reference indexes the sorted array with unsorted positions; reproduced).
 * out8 = [loss, sum of kept losses, k_pos + k_neg, n_pos, n_neg, k_pos, k_neg, 0]; dlogits (optional, [n, C], the
 * un-normalised w_y (softmax - onehot) written by peneo_pair_heads_fwd) is zeroed on the dropped pairs in place and
 * dl_sum[C] receives its column sums.  Everything stays on the device (no host read-back of the counts).
 * Workspace: peneo_ohem_workspace_bytes(n) bytes, 256-byte aligned. */
size_t peneo_ohem_workspace_bytes(int64_t n);
int peneo_ohem_ce(const float* logits, const int64_t* tags, const float* class_weight, int64_t n, int C,
                  int num_hard_positive, int num_hard_negative, float* dlogits, float* out8, float* dl_sum,
                  void* workspace, size_t workspace_bytes, peneo_stream_t stream);
/* per-head out8 rows [num_heads, 8] -> out[num_heads + 1] (losses, then sum_h ratio_h loss_h), scale_h = ratio_h / den_h,
 * inv_den_h = 1 / den_h: the OHEM counterpart of peneo_loss_finish */
int peneo_ohem_finish(const float* out8, const float* ratio, int num_heads, float* out, float* scale, float* inv_den,
                      peneo_stream_t stream);
/* stand-alone weighted CE on materialised logits [rows, C] (used by the unfused parity path) */
int peneo_weighted_ce(const float* logits, const int64_t* tags, const float* class_weight, int64_t rows, int C,
                      float* num, float* den, float* dlogits, peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K14 — decode front end (model/peneo_decoder.py:98-114): softmax -> argmax/max -> compaction of
 * the non-zero tags of one [P, C] map into (i, j, tag, score) spots in increasing p order.
 * count: device int (number found, may exceed max_spots; only max_spots are stored).
 * ------------------------------------------------------------------------------------------ */
/* ------------------------------------------------------------------------------------------
 * Optimizer step ("next" row f.4): fused multi-tensor AdamW with per-tensor learning rate and weight decay,
 * i.e. the four parameter groups of PEneoTrainer.create_optimizer (pipeline/trainer.py:275-330: decoder
 * parameters at lr x peneo_downstream_speedup_ratio, no decay on biases / LayerNorm) in ONE launch.
 * Arithmetic of torch.optim.AdamW (decoupled decay, bias-corrected moments).  The table and the two chunk maps
 * (chunk c covers elements [chunk_index[c] * peneo_adamw_chunk_elems(), ...) of tensor chunk_tensor[c]) live in
 * device memory and are built once.  `step` counts from 1; a tensor whose own count differs (state resumed from a
 * checkpoint with per-parameter steps, a parameter that joined later) carries the difference in `step_offset`:
 * its bias corrections use step + step_offset (which must be >= 1).
 * ------------------------------------------------------------------------------------------ */
typedef struct peneo_adamw_tensor {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  int64_t numel; float lr; float weight_decay;
  int32_t step_offset; int32_t reserved;
} peneo_adamw_tensor;
int peneo_adamw_chunk_elems(void);
int peneo_adamw_step(const peneo_adamw_tensor* table_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                     int n_chunks, float beta1, float beta2, float eps, int step, peneo_stream_t stream);
/* Global gradient-norm clipping inside the step (the reference trains through HF Trainer.train(), start/run_rfund.py:307-321,
 * whose default max_grad_norm = 1.0 clips every step with torch.nn.utils.clip_grad_norm_): peneo_grad_sqnorm leaves
 * sum_t |grad_t|^2 over all tensors of the table as peneo_grad_sqnorm_slots() partial sums in sqnorm_dev (device fp64 array,
 * zeroed by the call, stream-ordered, no host sync; their sum is the squared norm); peneo_adamw_step_clip then uses
 * grad * min(1, max_grad_norm / (sqrt(sum) + 1e-6)) in place of grad.  The gradient tensors are not modified.
 * sqnorm_dev == NULL: no clipping (== peneo_adamw_step). */
int peneo_grad_sqnorm_slots(void);
int peneo_grad_sqnorm(const peneo_adamw_tensor* table_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                      int n_chunks, double* sqnorm_dev, peneo_stream_t stream);
int peneo_adamw_step_clip(const peneo_adamw_tensor* table_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                          int n_chunks, float beta1, float beta2, float eps, int step, const double* sqnorm_dev,
                          float max_grad_norm, peneo_stream_t stream);
/* The step that also writes the parameters' working copies: peneo_adamw_step_clip, and for every element the UPDATED
 * parameter value additionally goes to dst[i] of each emission record of its tensor -- the bf16 (or fp32) copies that the
 * forward would otherwise rebuild with peneo_cast / peneo_cast_multi in a second pass over the memory this kernel has just
 * streamed.  A record names a tensor of the AdamW table, a destination and its dtype (PENEO_BF16 / PENEO_F32); bf16 is
 * rounded exactly as peneo_cast rounds, so dst equals a cast of the stored parameter bit for bit.  dst is a contiguous run
 * of the tensor's numel elements that may sit anywhere inside a larger buffer (a row block of a stacked [3H, H] QKV
 * matrix, a slice of a concatenated bias vector): it only needs the alignment of its element type, the kernel picks vector
 * or element stores per record.  Layout: `emits_dev` holds the records sorted by tensor, `emit_first_dev` has one entry per
 * tensor of the table plus one: the records of tensor k are emits_dev[emit_first_dev[k] .. emit_first_dev[k + 1]) -- none,
 * one or any number per tensor (`tensor` repeats k; it is what a builder sorts by).  Both arrays live in device memory.
 * Parameters and moments come out bit-identical to peneo_adamw_step_clip.  emits_dev == emit_first_dev == NULL: no
 * emission (== peneo_adamw_step_clip). */
typedef struct peneo_adamw_emit { void* dst; int32_t tensor; int32_t dtype; } peneo_adamw_emit;
int peneo_adamw_step_emit(const peneo_adamw_tensor* table_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                          int n_chunks, float beta1, float beta2, float eps, int step, const double* sqnorm_dev,
                          float max_grad_norm, const peneo_adamw_emit* emits_dev, const int32_t* emit_first_dev,
                          peneo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Composite stages: ONE call enqueues every kernel of an encoder layer (bf16 path) -- the per-kernel entry points above
 * called back to back from C++ (csrc/stages.hip), so that a layer costs the host one FFI call instead of 7 (forward) or
 * ~25 (backward).  Replaces LayoutLMv3Layer.forward and its autograd (modeling_layoutlmv3.py:482-529, :335-404; Roberta
 * SelfOutput / Intermediate / Output).  Every buffer is the caller's; rows = B * T; all matrices contiguous:
 *   x, att, h1, a, h2, out [rows, H]; qkv [rows, 3H] (q | k | v); zi, inter [rows, I]; lse [B, nh, T]; m*, r* [rows] (LayerNorm
 *   statistics); Wqkv [3H, H], Wo [H, H], Wi [I, H], Wo2 [H, I] bf16 working copies; biases / LayerNorm parameters fp32.
 * zi (GELU pre-activation) may be NULL in a forward that no backward follows.  Dropout: p_hidden with seed_o / seed_o2 on the
 * two dense + residual sites (mask = f(seed, element), regenerated by the backward), p_attn with `drop_words`
 * (peneo_attn_drop_words).  bias / key_bias as for peneo_attn_fwd.
 * ------------------------------------------------------------------------------------------ */
typedef struct peneo_encoder_layer {
  const void* Wqkv; const float* bqkv; const void* Wo; const float* bo; const float* g1; const float* b1;
  const void* Wi; const float* bi; const void* Wo2; const float* bo2; const float* g2; const float* b2;
  const void* bias; int64_t bias_ld; const float* key_bias; const uint32_t* drop_words;
  const void* x; void* qkv; void* att; float* lse; void* h1; float* m1; float* r1; void* a; void* zi; void* inter; void* h2;
  float* m2; float* r2;
  int32_t B, T, H, nh, I;
  int32_t wgrad_last;       /* backward only: != 0 marks the layer whose backward the caller issues last (layer 0); read under
                             * peneo_gemm_group_set_nn384_mode(2) alone.  (The field was `reserved`: the struct's size is unchanged.) */
  float eps, attn_scale, p_hidden, p_attn;
  uint32_t seed_o, seed_o2;
} peneo_encoder_layer;
/* Backward: gradients of the activations (caller's scratch, all written) and of the parameters.  d_dense1 / d_dense2 are
 * only used with p_hidden > 0.  dw* fp32 [out, in] are overwritten; db*, dg* fp32 are ACCUMULATED into (zero them first);
 * ds_out bf16 [B, nh, T, Tp] receives this layer's dS^T (peneo_attn_bwd); delta [B, nh, T] fp32 scratch. */
typedef struct peneo_encoder_layer_grads {
  const void* d_out; void* d_x;
  void* d_h2; void* d_dense2; void* d_zi; void* d_a; void* d_h1; void* d_dense1; void* d_att; void* dqkv; float* delta; void* ds_out;
  float* dwqkv; float* dbqkv; float* dwo; float* dbo; float* dg1; float* db1; float* dwi; float* dbi; float* dwo2; float* dbo2;
  float* dg2; float* db2;
} peneo_encoder_layer_grads;
/* sizeof of the structs shared with a binding: 0 peneo_gemm_epilogue, 1 peneo_encoder_layer, 2 peneo_encoder_layer_grads,
 * 3 peneo_encoder_layer_mxfp8, 4 peneo_adamw_emit */
size_t peneo_struct_bytes(int which);
/* workspace of the layer's GEMMs (as peneo_gemm_workspace_bytes): which = 0 forward, 1 backward main stream (dgrads), 2 backward
 * side stream (wgrads) */
size_t peneo_encoder_layer_workspace_bytes(int rows, int H, int I, int which);
int peneo_encoder_layer_fwd(const peneo_encoder_layer* layer, void* out, void* workspace, size_t workspace_bytes,
                            peneo_stream_t stream);
/* Packed inference form of peneo_encoder_layer_fwd (version 113; no backward): the same chain over the `rows` live rows of a batch
 * whose tokens were packed to the front (peneo_pack_plan, peneo_rows_pack) - every GEMM and LayerNorm at M = rows, the attention
 * peneo_attn_fwd_varlen with lens / cu_rows.  `layer` as above with these readings: T is Tm, the extent of bias [B, nh, Tm, bias_ld] and
 * lse [B, nh, Tm]; x, qkv, att, h1, a, inter, h2, out and m*, r* have `rows` rows; 1 <= rows <= B * T.  It requires p_hidden == p_attn ==
 * 0, zi == NULL, a bias tensor, no key_bias and head dim 64, else PENEO_ERR_INVALID with nothing launched.  Workspace:
 * peneo_encoder_layer_workspace_bytes(rows, H, I, 0).  With every lens[b] == T (rows = B * T) the result equals peneo_encoder_layer_fwd
 * bit for bit. */
int peneo_encoder_layer_fwd_packed(const peneo_encoder_layer* layer, const int32_t* lens, const int32_t* cu_rows, int rows, void* out,
                                   void* workspace, size_t workspace_bytes, peneo_stream_t stream);
/* MXFP8 inference form of peneo_encoder_layer_fwd (no backward): the four nn.Linear products run on peneo_gemm_mxfp8, attention and
 * the two LayerNorms stay bf16.  `layer` as above, except that Wqkv / Wo / Wi / Wo2, inter and zi are not used (zi must be NULL) and
 * p_hidden == p_attn == 0; `mx` carries the weights quantized with peneo_mxfp8_quantize_rows (W*_q [out, in] e4m3, W*_s [out, in / 32]
 * E8M0) and the caller's MX scratch: x_q / att_q / a_q [rows, H], inter_q [rows, I], each with its scales [rows, cols / 32].  Every
 * shape must pass peneo_gemm_mxfp8_supported: (rows, 3H, H), (rows, H, H), (rows, I, H), (rows, H, I).  The call is the composition
 * of the public entry points, in this order: quantize x; QKV product + bias; peneo_attn_fwd; quantize att; output projection + bias +
 * residual x -> h1; peneo_layernorm_fwd -> a; quantize a; FFN1 + bias + GELU -> inter_q / inter_s only (the bf16 `inter` is not
 * written); FFN2 + bias + residual a -> h2; peneo_layernorm_fwd -> out.  Where peneo_layernorm_mxfp8_supported(H), "LayerNorm, then
 * quantize" is the single call peneo_layernorm_fwd_mxfp8 (the same bytes).  No workspace.
 * Chaining layers: with out_q / out_s non-NULL the last LayerNorm also leaves the MX copy of `out` there ([rows, H], [rows, H / 32]:
 * byte for byte the quantization of `out`); with x_prequantized != 0 the call takes x_q / x_s as the valid MX copy of x (the out_q /
 * out_s of the layer before) and skips its first quantizer. */
typedef struct peneo_encoder_layer_mxfp8 {
  const void* Wqkv_q; const void* Wqkv_s; const void* Wo_q; const void* Wo_s;
  const void* Wi_q; const void* Wi_s; const void* Wo2_q; const void* Wo2_s;
  void* x_q; void* x_s; void* att_q; void* att_s; void* a_q; void* a_s; void* inter_q; void* inter_s;
  void* out_q; void* out_s;          /* optional, both or neither */
  int32_t x_prequantized, reserved;
} peneo_encoder_layer_mxfp8;
int peneo_encoder_layer_mxfp8_supported(int rows, int H, int I);
int peneo_encoder_layer_fwd_mxfp8(const peneo_encoder_layer* layer, const peneo_encoder_layer_mxfp8* mx, void* out,
                                  peneo_stream_t stream);
/* The activation-gradient chain runs on `stream`; the parameter-gradient work (weight-gradient GEMMs, bias column sums) on
 * `side_stream` behind HIP events recorded on `stream` (the FFN / output-projection part starts with the attention backward,
 * the QKV part behind it).  The call does NOT join the two streams: the caller waits for `side_stream` before anything
 * reads dw* / db* (side_stream NULL or == stream: everything in order on one stream). */
int peneo_encoder_layer_bwd(const peneo_encoder_layer* layer, const peneo_encoder_layer_grads* grads, void* ws_main,
                            size_t ws_main_bytes, void* ws_side, size_t ws_side_bytes, peneo_stream_t stream,
                            peneo_stream_t side_stream);

/* K13 input side ("next" row f.2): dense label maps [B, P] int64 from n sparse spots (b, i, j, tag) — replaces the
 * host loop of HandshakingTaggingScheme.spots2shaking_tag4batch (model/peneo_decoder.py:35-73, called per head by
 * data/collator.py:156-204) and the 5.2 MB/document host-to-device copy of its result.  Last spot wins, like the
 * host loop; *status is set to 1 when a spot lies outside [0, B) x [0, N)^2. */
int peneo_spots_to_tags(const int32_t* spots_bijt, int n_spots, int B, int N, int64_t* tags, int32_t* status,
                        peneo_stream_t stream);
int peneo_spots_compact(const float* logits, int64_t P, int C, int N, int32_t* spots_ijt, float* scores,
                        int32_t* count, int max_spots, peneo_stream_t stream);

/* K14, batched: every map of a batch in ONE call (two stream-ordered launches: count, then write; csrc/spots.hip) — replaces one
 * peneo_spots_compact launch and one host read of its count per document and head (HandshakingTaggingScheme.
 * get_spots_from_shaking_tag, model/peneo_decoder.py:76-115, called 5 x B times per batch by pipeline/decode.py).
 * Map m is fp32 logits [B, P, classes[m]] (classes[m] >= 2) or an int64 label map [B, P] (classes[m] == 0); P = N (N + 1) / 2,
 * the same B and N for every map.  Per (map, document), exactly peneo_spots_compact: tag = first maximum under strict > (ties to
 * the lower class, a NaN never wins), score = 1 / sum_c exp(l_c - max) (the same bits), a pair is a spot iff tag != 0, spots come
 * out in increasing p; a label map's spot is value != 0 (the int64 value) with tag = value and score 1.0; labels are expected in the int32
 * range: a value outside it is still a spot, its tag is the low 32 bits (1 where those are zero).
 *   records [num_maps][B][max_spots] of 16 bytes {int32 i, int32 j, int32 tag, float score}, 16-byte aligned;
 *   counts  [num_maps][B] int32: the TRUE number of spots, which may exceed max_spots; only the first max_spots in p order are
 *           stored and nothing is written behind a (map, document)'s min(count, max_spots) records.
 * workspace: peneo_spots_compact_batch_workspace_bytes(num_maps, B, N) bytes (the per-segment counts; 0 = shape out of range),
 * 4-byte aligned, used by one call at a time.  The caller owns every buffer; no allocation and no host synchronisation inside.
 * PENEO_ERR_INVALID, with nothing launched: a NULL map / records / counts, num_maps outside 1 .. PENEO_MAX_HEADS, classes[m] == 1
 * or < 0, a NULL or short workspace, max_spots < 0, B < 1 or B > 65535 (documents are one grid dimension), N < 1 or N > 65535 (P must stay below 2^31).  records may be
 * NULL when max_spots == 0 (count only). */
typedef struct peneo_spots_batch_desc {
  int num_maps;                          /* <= PENEO_MAX_HEADS */
  int classes[PENEO_MAX_HEADS];          /* >= 2: fp32 logits [B, P, classes[m]]; 0: int64 label map [B, P] */
  const void* maps[PENEO_MAX_HEADS];
} peneo_spots_batch_desc;
size_t peneo_spots_compact_batch_workspace_bytes(int num_maps, int B, int N);
int peneo_spots_compact_batch(const peneo_spots_batch_desc* desc, int B, int N, void* records, int32_t* counts,
                              int max_spots, void* workspace, size_t workspace_bytes, peneo_stream_t stream);

/* ---- diagnostics: NOT part of the thread-safety contract -------------------------------------------------------------
 * Process-wide switch of the forward GEMM tile choice (gemm_big.hip): 0 = always the 128 x 128 kernel, 1 = the calibrated
 * choice (default; also set by PENEO_GEMM_BIG), 256 / 384 / 128 = force one big-tile shape where its constraints hold.  A plain
 * global: set it while no peneo_gemm call is in flight on any thread.  Used by the kernel tests and tools/ only. */
void peneo_gemm_set_big_mode(int mode);
int peneo_gemm_big_mode(void);            /* the mode in force (tests restore what they found) */
/* The same for weight gradients with A = [K, M] and B = [K, N] (gemm_big.hip, 384 x 192 tiles x split_k one-per-CU workgroups whose
 * fp32 partials the split-k reduce sums in slice order).  The rule: bf16 operands, fp32 C, no epilogue option beyond accumulate,
 * no a_colsum, M % 384 == 0, N % 192 == 0, K % 8 == 0, 16-byte aligned operands, and K >= 65536 (the pair heads' dW1; every
 * other caller keeps the 128 x 128 kernel).  0 = off, 1 = that rule (default; also set by PENEO_GEMM_NN384), 2 = the rule without
 * its bound on K (tests, tools).  PENEO_GEMM_BIG = 0 / peneo_gemm_set_big_mode(0) switches it off as well.
 * Diagnostics like the setter above (process-wide plain globals, not thread-safe, for tests, tools and the decoder's split choice):
 * peneo_gemm_nn384_mode: the mode in force (0 while big tiles are off).  peneo_gemm_nn384_launches: how many peneo_gemm calls of
 * this process took the path (the 128 x 128 kernel sums the same k-steps in the same order, so a result cannot tell which ran).
 * peneo_gemm_nn384_shape_ok: 1 if the SHAPE part of the rule holds for (M, N, K) under the mode in force - the library's one copy of
 * 384 / 192 / 8 / 65536; a call with that shape still keeps the 128 x 128 kernel when its layouts, C type, epilogue or the
 * alignment of an operand (16-byte bases, lda % 8, ldb % 8, ldc % 4, 64 rows of A or B below 2 GiB) are outside the rule. */
void peneo_gemm_set_nn384_mode(int mode);
int peneo_gemm_nn384_mode(void);
uint64_t peneo_gemm_nn384_launches(void);
int peneo_gemm_nn384_shape_ok(int M, int N, int K);
/* The same tile for peneo_gemm_group: ONE launch walks the 384 x 192 tiles of all problems of the call, each workgroup the whole K of
 * its tile (no split, no workspace, no atomics: the same bits on every run, and the bits of the 128 x 128 group).  Taken when EVERY
 * problem passes: bf16 operands, a_kmajor == b_kmajor == 0, fp32 C, no epilogue option beyond accumulate, M % 384 == 0, N % 192 == 0,
 * K % 8 == 0 (a ragged last k-tile requests only the rows below K), 16-byte aligned A / B / C bases, lda % 8, ldb % 8, ldc % 4, 64 rows
 * of A or B below 2 GiB; otherwise the whole call keeps the 128 x 128 kernel.  Mode: 0 = off, 1 = on (default), 2 = on except in the
 * peneo_encoder_layer_bwd call whose layer has wgrad_last != 0; also set by PENEO_WGRAD_NN384; off while big tiles are off.
 * peneo_gemm_group_nn384_launches: how many peneo_gemm_group calls of this process took the path. */
void peneo_gemm_group_set_nn384_mode(int mode);
int peneo_gemm_group_nn384_mode(void);
uint64_t peneo_gemm_group_nn384_launches(void);
/* The same for the persistent launch (gemm_sk.hip; first choice of peneo_gemm for large bf16 problems with k-major A and B):
 * 0 = off (the tiled kernels above), 1 = the measured rules (default; also set by PENEO_GEMM_SK), F * 1000 + BN = force ranges of
 * whole 32 F x BN tiles, + 100000 = force ranges that cut tiles (stream-k), wherever the kernel's constraints hold (B k-major among
 * them; elsewhere the tiled kernels run).  Instantiated tiles: F = 4 .. 8 with BN = 128, F = 4 .. 6 with BN = 256 (e.g. 5128, 4256,
 * 105128); any other forced mode makes peneo_gemm return PENEO_ERR_INVALID.  Size workspaces under the mode they are used with. */
void peneo_gemm_set_sk_mode(int mode);
/* tools/ only.  peneo_gemm_sk_set_prof: device buffer of [1024][16] uint64 that receives one lane's s_memrealtime stamps (100 MHz) at
 * the stations of every workgroup's range of a persistent launch (0 start, 1 stream primed, 2 first unit landed, 3 / 4 slab publish,
 * 5 / 6 / 7 flag wait and acquire, 8 / 9 last whole-tile epilogue, 10 / 11 finisher epilogue, 12 stores drained); NULL = off.
 * peneo_gemm_sk_set_max_groups: at most this many workgroups per persistent launch (a multiple of 8; 0 = one per CU). */
void peneo_gemm_sk_set_prof(void* stamps);
void peneo_gemm_sk_set_max_groups(int n);

/* ---- deterministic mode: bit-reproducible training steps ----------------------------------------------------------------
 * Process-wide like the switches above: a plain global, set while no call of this library is in flight on any thread.
 *   0  off (default): every launcher picks the kernels it always picked.
 *   1  every launcher that has an order-independent form uses it; the others run as before.
 *   2  strict: 1, and a call that would still take an order-dependent accumulation path (same-address float atomics from many
 *      workgroups) returns PENEO_ERR_INVALID, nothing launched, with a peneo_last_error() message that names the entry point.
 * PENEO_DETERMINISTIC = 0 / 1 / 2 sets the initial value.  Under modes 1 and 2 two executions of the same calls on the same inputs,
 * in one process on one device, give the same bits.  Nothing is claimed across devices, processes, ranks, batch sizes or builds.
 * Forms: peneo_colsum, peneo_layernorm_bwd and peneo_embed_text_bwd switch to single-writer kernels inside their
 * launchers (no workspace; peneo_encoder_layer_bwd follows through them); peneo_pair_bwd_fused / peneo_pair_bwd_saved(_e4m3) give every
 * workgroup a workspace row of its own, and so does peneo_pair_dz_fused; peneo_pair_x_bwd runs one workgroup per row; the
 * relative-position tables and the gradient norm take a workspace through the _ws entry points below.  Order-dependent in every
 * mode (counted; refused under 2): peneo_gemm with a_colsum or pair_dz, peneo_attn_bwd with dq_accum, peneo_ohem_ce,
 * peneo_weighted_ce, peneo_relpos_bias_bwd(_layers) and peneo_grad_sqnorm without workspace.
 * peneo_order_dependent_launches: how many calls of this process took an order-dependent accumulation path, in any mode (a result
 * cannot tell which kernel ran: the tests read this as proof of routing). */
void peneo_set_deterministic(int mode);
int peneo_deterministic(void);
uint64_t peneo_order_dependent_launches(void);
/* Workspace rows of peneo_pair_bwd_fused / peneo_pair_bwd_saved(_e4m3) under the mode in force: [rows][4 * num_heads * D] fp32, zeroed by
 * the caller, summed afterwards with peneo_colsum.  Mode 0: 256.  Modes 1 / 2: one row per workgroup of the launch, B * (blocks of
 * the pair triangle) = B * peneo_pair_bwd_rows(N) / 128 - at 8 x 511 tokens 8 448 rows x 4 * 5 * 384 floats = 260 MB.  Size the
 * workspace under the mode the call runs with. */
int64_t peneo_pair_bwd_workspace_rows(int B, int N);
/* The same for peneo_pair_dz_fused (the chunked decoder backward, widths without the fused kernel): rows of its workspace for
 * launches of up to `npairs` pairs.  Mode 0: 256.  Modes 1 / 2: one row per workgroup of a launch (npairs / 256, at least 256); the
 * launches of a backward add into the rows one after the other on one stream.  The four-wave kernel of the widths above 512 walks
 * a workgroup's 256 pairs in two rounds and adds twice to each address of its row: both adds come from the same lane of the same
 * wave, in program order, so the row still has a single writer in a fixed order and the call is not counted as order-dependent
 * under modes 1 / 2 either.  peneo_pair_x_bwd runs one workgroup per row / column of the triangle under the mode (no workspace). */
int64_t peneo_pair_dz_fused_workspace_rows(int64_t npairs);
/* peneo_relpos_bias_bwd_layers / peneo_relpos_bias_bwd with the deterministic fold: under modes 1 / 2 the per-workgroup bin sums go
 * to 64-bit fixed-point accumulators in `workspace` (2^-32 units, |sum of a bin over the launch| < 2^31) with integer atomics, and
 * one more launch adds every bin to dw1 / dwx / dwy.  workspace: peneo_relpos_bwd_workspace_bytes(nh, bins1, bins2) bytes (0 under
 * mode 0, where the calls equal the plain ones and workspace may be NULL), 8-byte aligned, cleared inside, one call at a time. */
size_t peneo_relpos_bwd_workspace_bytes(int nh, int bins1, int bins2);
int peneo_relpos_bias_bwd_layers_ws(const void* ds, int L, int64_t layer_stride, const uint8_t* bk1_t, const uint8_t* bkx_t,
                                    const uint8_t* bky_t, float* dw1, int bins1, float* dwx, float* dwy, int bins2, float scale,
                                    int B, int nh, int T, int Tp, void* workspace, size_t workspace_bytes, peneo_stream_t stream);
int peneo_relpos_bias_bwd_ws(const float* g, int64_t ldg, const uint8_t* bk1, const uint8_t* bkx, const uint8_t* bky, float* dw1,
                             int bins1, float* dwx, float* dwy, int bins2, float scale, int B, int nh, int T, void* workspace,
                             size_t workspace_bytes, peneo_stream_t stream);
/* peneo_grad_sqnorm with the deterministic sum: under modes 1 / 2 every chunk's sum is stored to `workspace` and one workgroup
 * adds them in chunk order; the total lands in slot 0 of sqnorm_dev and the other slots are cleared, so peneo_adamw_step_clip /
 * _emit read it unchanged.  workspace: peneo_grad_sqnorm_workspace_bytes(n_chunks) bytes (0 under mode 0: the plain call),
 * 8-byte aligned. */
size_t peneo_grad_sqnorm_workspace_bytes(int n_chunks);
int peneo_grad_sqnorm_ws(const peneo_adamw_tensor* table_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                         int n_chunks, double* sqnorm_dev, void* workspace, size_t workspace_bytes, peneo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PENEO_HIP_H */
