/*
 * mapfed.h — C ABI of the MI355X-native federated MaPLe hot path (libmapfed.so, gfx950).
 *
 * The reference (tahaspc82442/federated_multi_modal) is pure Python on PyTorch: its "kernels" are
 * implicit torch ops and it has no FFI below Python.  Each entry point
 * below replaces the torch op(s) the reference calls at the cited file:line; INTEGRATION.md shows
 * the ctypes binding and the Python module API (trainers/maple.py, trainers/maple_fed.py mirror)
 * that sit on top.
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (kernels never allocate or free).
 *   - `stream` is a hipStream_t (void* so the header needs no HIP include); all work is enqueued
 *     asynchronously on it; nothing synchronises the host.  Safe to capture in a hipGraph.
 *   - fp16 tensors are IEEE binary16, row-major; `ld*` are leading dimensions in elements.
 *   - Return value: 0 on success, non-zero on argument or launch error; the message is in
 *     mf_last_error() (thread-local).
 */
#ifndef MAPFED_H_
#define MAPFED_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* mf_last_error(void);
int mf_abi_version(void);

/* ---- dense projections (GEMM, MFMA) ------------------------------------------------------
 * C[M,N] = epilogue(A[M,K] . B[N,K]^T), fp32 accumulate.  K % 64 == 0, N % 4 == 0.
 * epilogue: 0 none | 1 +bias | 2 +bias then +aux_in residual | 3 +bias, aux_out = pre-activation (the
 *           backward's operand; null: not stored, the forward-only eval engine), C = QuickGELU | 4 C = QuickGELU'(fp16(acc), aux_in) | 5 fp32 store | 6 +aux_in residual
 * tile: 0 auto (latency picks), -1 auto for a product of the tower off the step's critical path (tiles chosen for
 *       work per CU-second; the engine passes it for the text tower at c4, the vision tower at C5), 1 128x128,
 *       2 128x64, 3 64x64, 10 160x128, 15 96x128, 16 160x64, 20 256x256 8-wave (gemm8s, the A/B baseline of 40),
 *       26 96x64, 31 64x64 and 33 32x64 with a 4-stage ring, 40 256x256 8-wave full-line (gemm8f), 50 small-M
 *       (gemm_sm: M <= 64, K <= 3072).
 * Replaces: nn.Linear / addmm inside nn.MultiheadAttention in_proj + out_proj, mlp.c_fc, QuickGELU,
 * mlp.c_proj and the residual adds (clip/model.py:274-280,303-305,350-351), the patch-embed conv as
 * im2col GEMM (clip/model.py:514), the tower heads (clip/model.py:570, trainers/maple.py:76) and all
 * of their autograd dX/dW products.                                                             */
int mf_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
               const void* bias, const void* aux_in, void* aux_out, int64_t ld_aux, int epilogue, int tile,
               void* stream);
/* General layouts: C[M,N] = epilogue(op(A) . op(B)^T) with
 *   a_kmajor = 0: A[m][k] at A[m*lda + k]  |  1: A[k*lda + m]   (e.g. dY^T of a weight gradient)
 *   b_kmajor = 0: B[n][k] at B[n*ldb + k]  |  1: B[k*ldb + n]   (e.g. nn.Linear W [out][in] in dX = dY . W)
 * K-major operands need rows % 8 == 0; K % 64 == 0 unless both operands are K-major (then any K: the
 * tail reads as zero).  Replaces the autograd dX / dW products of every nn.Linear on the path
 * (torch.mm(grad, W), torch.mm(grad^T, X)) without materialising a transpose.                      */
int mf_gemm(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C, int64_t ldc,
            int M, int N, int K, const void* bias, const void* aux_in, void* aux_out, int64_t ld_aux, int epilogue,
            int tile, void* stream);
/* Split-K plain product (no epilogue) for few output tiles and a long K, e.g. the weight gradients
 * dW = dY^T X with K = tokens (autograd's torch.mm(grad.t(), x) of nn.Linear, clip/model.py:274-280):
 * `splits` 128x128-tile workgroups per tile each reduce a K slice into an fp32 plane of ws, then the
 * planes are summed in a fixed order into C (fp16 if out_f16, else fp32).  splits <= 0: automatic.
 * ws: mf_gemm_splitk_ws_floats(M, N, K, splits) floats.  Layout flags as mf_gemm; N % 8 == 0.     */
int mf_gemm_splitk(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C,
                   int64_t ldc, int M, int N, int K, float* ws, int64_t ws_floats, int splits, int out_f16,
                   void* stream);
int mf_gemm_splitk_ws_floats(int M, int N, int K, int splits);
/* mf_gemm_splitk with a promise about A: its k-rows with k % L_full >= L_live are exact zeros (+0 or -0) in the
 * output rows m < m_live (A's columns >= m_live are ordinary data; B is only finite).  The 64-row K-tiles that
 * hold no live k-row are skipped by the workgroups below m_live; slices, planes and both summation orders are
 * mf_gemm_splitk's, so C is bit for bit its result (the class-row block's weight gradients, K = N images x L
 * tokens with one live row per image).  Both operands K-major (anything else is an error), 0 < L_live <= L_full,
 * K % L_full == 0; workspace as mf_gemm_splitk.                                                              */
int mf_gemm_splitk_live(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C,
                        int64_t ldc, int M, int N, int K, float* ws, int64_t ws_floats, int splits, int out_f16,
                        int L_live, int L_full, int m_live, void* stream);

/* ---- LayerNorm (fp16 io, fp32 math; clip/model.py:153-159) --------------------------------
 * row_index (optional, int32): output row i normalises input row row_index[i]
 * (ln_post on class tokens clip/model.py:567, ln_final + EOT gather trainers/maple.py:72-76).    */
int mf_layernorm_fwd(const void* x, int64_t ldx, const int* row_index, const float* gamma, const float* beta,
                     void* y, int64_t ldy, float* mean, float* rstd, int rows, int D, void* stream);
/* mf_prompt_inject_fwd(x, prompt, rows / L, L, row0, nrows, D) then mf_layernorm_fwd(x, ...), in one
 * pass (bit-identical): the deep prompts injected at the start of a block and that block's ln_1
 * (clip/model.py:320-349, 153-159).  x is written (the injected rows).                            */
int mf_layernorm_fwd_inject(void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                            float* mean, float* rstd, int rows, int D, const float* prompt, int L, int row0,
                            int nrows, void* stream);
/* dx = fp16(dres + fp16(LN'(dy)))  (dres optional; dx may alias dres); dgamma/dbeta written or
 * accumulated (accumulate != 0).  workspace: 2 * mf_layernorm_bwd_blocks(rows) * D floats.        */
int mf_layernorm_bwd_blocks(int rows);
int mf_layernorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const int* row_index,
                     const float* gamma, const float* mean, const float* rstd, const void* dres, int64_t ldres,
                     void* dx, int64_t lddx, float* dgamma, float* dbeta, float* workspace, int rows, int D,
                     int accumulate, void* stream);

/* Partials-only LayerNorm backward with the deep-prompt injection backward fused in: rows row0..row0+
 * nrows-1 of each L-row sequence store their dx as fp32 partials inj_part[rows/L][nrows][D] (the prompt
 * gradient = their sum over sequences, via mf_col_reduce_batch) and a zero dx row.  Replaces
 * mf_layernorm_bwd + mf_prompt_inject_bwd(zero_rows) on the same rows (clip/model.py:153-159,320-349). */
int mf_layernorm_bwd_inject(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                            const float* mean, const float* rstd, const void* dres, int64_t ldres, void* dx,
                            int64_t lddx, float* workspace, int rows, int D, float* inj_part, int L, int row0,
                            int nrows, void* stream);

/* Partials-only LayerNorm backward of a tower stored as the first L_live rows of each of its seqs L_full-row
 * sequences (the EOT-truncated text tower: every later row has exactly zero gradient).  The compact rows are
 * processed as rows t < L_live of the full tower, so the block partials (workspace: 2 *
 * mf_layernorm_bwd_blocks(seqs * L_full) * D floats) -- and dgamma / dbeta -- are bit for bit those of
 * mf_layernorm_bwd over all seqs * L_full rows.  inj_part (optional): the injection backward of
 * mf_layernorm_bwd_inject (L = L_live).  clip/model.py:153-159 under the causal mask of :679-685.        */
int mf_layernorm_bwd_live(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                          const float* mean, const float* rstd, const void* dres, int64_t ldres, void* dx,
                          int64_t lddx, float* workspace, int seqs, int L_live, int L_full, int D, float* inj_part,
                          int row0, int nrows, void* stream);

/* dgamma == dbeta == NULL: write the per-block partials only; their reduction is deferred to one
 * mf_col_reduce_batch over all LayerNorms of a backward pass.  desc = {const float* part; void* out;
 * int nblk, C, accumulate, out_f16} (mf_col_reduce_desc_bytes() bytes each, device memory):
 * out[c] (=|+=) sum_b part[b*C + c], fixed order; out is fp32, or fp16 when out_f16 (the deferred bias
 * gradients: mf_colsum_f16 with out == NULL leaves the partials, and this sum is bit for bit its own).  */
int mf_col_reduce_desc_bytes(void);
int mf_col_reduce_batch(const void* descs, int n, int max_cols, void* stream);

/* ---- attention (head_dim 64, L <= 512: one-pass kernels up to 256 rows, the caption path's growing
 * vision sequences of 257..512 rows on the two-pass forward / dK-dV + dQ backward; SDPA inside
 * nn.MultiheadAttention, clip/model.py:303-305, causal mask clip/model.py:679-685)
 * — qkv [N*L, 3*H*64], out [N*L, H*64], lse [N*H, ld_lse]                                         */
int mf_attention_fwd(const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out, float* lse, int ld_lse, int N,
                     int L, int H, int causal, void* stream);
/* The first q_rows query rows of every head only (K / V of all L <= 256 rows; each computed row bit-identical to
 * mf_attention_fwd's): the forward-only engine's last vision block, whose output ln_post reads only at the class
 * token (clip/model.py:567), attends query row 0 (r06).                                              */
int mf_attention_fwd_rows(const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out, float* lse, int ld_lse, int N,
                          int L, int H, int causal, int q_rows, void* stream);
/* The in-projection and the attention forward in one launch: qkv = fp16(x w^T + bias) (w = in_proj_weight
 * [3D, D], bias [3D]; bit-identical to mf_gemm_nt's EPI_BIAS) is written to qkv [N*L, 3D] and attended
 * as mf_attention_fwd does (bit-identical out / lse).  Shapes: the vision blocks (D = 768, 193..208
 * tokens) and the text blocks (D = 512, causal, 65..80 tokens); x_rows = rows of the x buffer (>= N*L).
 * Replaces the in_proj + SDPA of nn.MultiheadAttention (clip/model.py:303-305).                      */
int mf_qkv_attention_fwd(const void* x, int64_t ld_x, int x_rows, const void* w, const void* bias, void* qkv,
                         int64_t ld_qkv, void* out, int64_t ld_out, float* lse, int ld_lse, int N, int L, int H,
                         int causal, void* stream);
int mf_qkv_attention_supported(int N, int L, int H, int causal);
/* dqkv [N*L, 3*H*64]; dq_dot_ws: N*H*ld_lse floats of workspace                                   */
int mf_attention_bwd(const void* qkv, int64_t ld_qkv, const void* out, int64_t ld_out, const void* dout,
                     int64_t ld_dout, const float* lse, float* dq_dot_ws, int ld_lse, void* dqkv, int64_t ld_dqkv,
                     int N, int L, int H, int causal, void* stream);
/* mf_attention_bwd for a dout that is zero at query rows >= q_rows of every sequence (the training step's last
 * vision block: ln_post reads the class token only, so one row of dO per image is live).  Rows >= q_rows of dout,
 * out and lse are not read and may hold anything; qkv is read, and dqkv written, at every row.  dqkv is bit for bit
 * mf_attention_bwd's for that dout (+0 in dQ at the other query rows).  Non-causal, L <= 224 only (the fused
 * one-workgroup-per-head kernel); a causal mask or a longer sequence is an error -- there is no detour through the
 * full path, which would read the rows this entry leaves alone.                                      */
int mf_attention_bwd_rows(const void* qkv, int64_t ld_qkv, const void* out, int64_t ld_out, const void* dout,
                          int64_t ld_dout, const float* lse, int ld_lse, void* dqkv, int64_t ld_dqkv, int N, int L,
                          int H, int causal, int q_rows, void* stream);

/* ---- token assembly / prompt injection (clip/model.py:514-538,320-349; trainers/maple.py:54,152-166) */
/* Refused (nonzero, mf_last_error(), nothing launched) unless the stated preconditions hold; empty work (a batch
 * or row count of 0) returns 0 and launches nothing.
 * mf_im2col_patch: R % P == 0, P % 8 == 0, img and out 16-byte aligned.
 * mf_vision_assemble / mf_text_assemble: D % 4 == 0; the fp16 operands (patch, shared_ctx, x / prefix, ctx, suffix,
 *   x) 8-byte aligned (they are accessed 4 elements at a time); cls and pos need only their natural alignment.
 * mf_prompt_inject_fwd / _bwd: 0 <= row0 and row0 + nrows <= L; N == 0 or nrows == 0 is empty work.  _bwd: D % 4 == 0
 *   and dx 8-byte aligned.                                                                                          */
int mf_im2col_patch(const void* img, int img_is_f32, void* out, int B, int R, int P, void* stream);
int mf_vision_assemble(const void* patch, const float* cls, const float* pos, const void* shared_ctx, void* x,
                       int B, int G2, int n_ctx, int D, void* stream);
int mf_text_assemble(const void* prefix, const void* ctx, const void* suffix, const float* pos, void* x, int K,
                     int L, int n_ctx, int D, void* stream);
int mf_prompt_inject_fwd(void* x, const float* prompt, int N, int L, int row0, int nrows, int D, void* stream);
/* out[r,:] (=|+=) sum_n dx[n*L+row0+r,:] (fp32 accumulate, fp16 or fp32 out); zero_rows clears them  */
int mf_prompt_inject_bwd(void* dx, int N, int L, int row0, int nrows, int D, void* out, int out_f16, int accumulate,
                         int zero_rows, void* stream);

/* ---- helpers for the backward products ------------------------------------------------------ */
/* ---- caption-conditioned visual prompts (K19; clip/model.py:457-476, 550-561; trainers/maple.py:307-322) */
/* The growing vision sequence of a prompted layer: dst [N, Lp+ncap, D] = src rows 0..Lp-n_ctx-1 | cap    */
/* [ncap, D] (fp16, shared by every sequence) | fp16(prompt [n_ctx, D] fp32); replaces the torch.cat of   */
/* clip/model.py:324-330 fed with cat(projected captions, deep prompt) (:558-559).  Both directions need   */
/* D % 8 == 0, 0 <= n_ctx <= Lp, ncap >= 0 and 16-byte aligned fp16 operands (8 elements per access).      */
int mf_seq_grow(const void* src, void* dst, const void* cap, const float* prompt, int N, int Lp, int ncap, int n_ctx,
                int D, void* stream);
/* its backward into the previous output: dsrc [N, Lp, D] = ddst rows 0..Lp-n_ctx-1, zeros for the dropped */
/* previous prompt rows                                                                                     */
int mf_seq_grow_bwd(const void* ddst, void* dsrc, int N, int Lp, int ncap, int n_ctx, int D, void* stream);
/* AttentionPooling (clip/model.py:464-476) of B captions from their token ids [B, T] (int32), the fp32     */
/* token-embedding table [vocab, D] and the fp16 weight vector w [D]: pooled [B, D] fp16.  An id outside    */
/* [0, vocab) reads nothing and makes its caption's pooled row NaN (the step's loss check then raises)      */
int mf_caption_pool(const int* tokens, int B, int T, const float* table, int vocab, const void* w, int D,
                    void* pooled, void* stream);
/* out [C, R] = in [R, C]^T; ld_in >= C and ld_out >= R (refused otherwise).  Any alignment: 16-byte tile accesses
 * are used only when both pointers are 16-byte aligned and both leading dimensions are multiples of 8.       */
int mf_transpose_f16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int R, int C, void* stream);
/* dst row n*L_full + t = src row n*L_live + t (t < L_live; other dst rows untouched), C % 8 == 0 columns: the
 * EOT-truncated text tower's block-11 weight-gradient operands in the full tower's row layout              */
int mf_seq_scatter(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int N, int L_live, int L_full, int C,
                   void* stream);
int mf_colsum_blocks(int R);
/* out[c] = sum_r in[r,c]; workspace: mf_colsum_blocks(R) * C floats.  out == NULL: only the partials
 * workspace[mf_colsum_blocks(R)][C] are written, for a later mf_col_reduce_batch (nblk = mf_colsum_blocks(R)).
 * Refused unless C % 4 == 0, ld % 4 == 0, ld >= C, in is 8-byte aligned (4 fp16 per load) and workspace is non-null
 * and 16-byte aligned (4 floats per store); mf_colsum_f16_live likewise.                                         */
int mf_colsum_f16(const void* in, int64_t ld, int R, int C, void* out, int out_f16, float* workspace, void* stream);
/* mf_colsum_f16 for an `in` whose rows r with r % L_full >= L_live are exact zeros: the 64-row chunks without a
 * live row store +0 partials and read nothing; bit for bit mf_colsum_f16's result.  R % L_full == 0.          */
int mf_colsum_f16_live(const void* in, int64_t ld, int R, int C, void* out, int out_f16, float* workspace,
                       int L_live, int L_full, void* stream);
int mf_cast_f16_f32(const void* in, float* out, int64_t n, void* stream);

/* ---- prompt-learner linears, M <= 16 rows (trainers/maple.py:111-131,194-215) --------------- */
int mf_small_linear_fwd(const void* X, const void* W, const void* b, void* Y, int M, int I, int O, int is_f16,
                        void* stream);
/* dX, dW and db may each be null; db is written by the dW kernel, so a null dW leaves db untouched (in the batched
 * form too).                                                                                                     */
int mf_small_linear_bwd(const void* dY, const void* X, const void* W, void* dX, void* dW, void* db, int M, int I,
                        int O, int is_f16, int accumulate_dx, void* stream);

/* Batched form: every Linear of the prompt learner in one launch per direction.  descs: device array
 * of n descriptors of mf_small_linear_desc_bytes() bytes {const void *X, *W, *b; void *Y; const void* dY;
 * void *dX, *dW, *db; int M, I, O, is_f16, accumulate_dx, pad} (b / dX / dW / db may be null);
 * max_* bound the grid over the descriptors (M*O, M, I, O*I).                                         */
int mf_small_linear_desc_bytes(void);
int mf_small_linear_fwd_batch(const void* descs, int n, int max_mo, void* stream);
int mf_small_linear_bwd_batch(const void* descs, int n, int max_m, int max_i, int max_oi, void* stream);

/* ---- cosine-logit head + loss (trainers/maple.py:325,340-378) -------------------------------- */
int mf_clip_head_fwd(const void* img, const void* txt, int B, int K, int D, const float* logit_scale, void* img_n,
                     void* txt_n, float* norms, void* mm, void* logits, void* stream);
int mf_clip_loss_fwd_bwd(const void* img, const void* txt, const void* img_n, const void* txt_n, const float* norms,
                         const void* logits, const int64_t* label, int B, int K, int D, const float* logit_scale,
                         void* dmm, float* cos_ws, float* loss_out, void* dimg_n, void* dtxt_n, void* dimg,
                         void* dtxt, void* stream);
/* Soft (float) labels q [B,K] fp32 (trainers/maple.py:356-360): KL(q.clamp(1e-8) || softmax) batchmean
 * (fp32) + 0.5 (1 - mean cos(img_n, fp16(q) @ txt_n)); loss_out[0] is the fp32 total.  soft_ws: 2*B*D
 * fp16 of workspace.  The reference's `label @ text_features` multiplies fp32 by fp16 and raises in its
 * fp16 configuration; the label is taken in the features' dtype (what torch.autocast computes).       */
int mf_clip_loss_soft_fwd_bwd(const void* img, const void* txt, const void* img_n, const void* txt_n,
                              const float* norms, const void* logits, const float* label_probs, int B, int K, int D,
                              const float* logit_scale, void* dmm, float* cos_ws, void* soft_ws, float* loss_out,
                              void* dimg_n, void* dtxt_n, void* dimg, void* dtxt, void* stream);

/* eval predictions (trainers/maple.py:674-677): pred[b] = argmax_k logits (first max; NaN is the max);
 * acc[0] += #correct, acc[1] += B (device-side accuracy counters, read once per test pass)           */
int mf_argmax_correct(const void* logits, int B, int K, const int64_t* label, int64_t* pred, float* acc, void* stream);

/* ---- optimizer / federated averaging (trainers/maple.py:592-598; trainers/maple_fed.py:309-325) */
int mf_optim_chunk_bytes(void);
int mf_optim_chunk_elems(void);
int mf_clip_grad_norm(const void* g16, const float* g32, const void* chunks, int nchunks, float max_norm,
                      float* part, float* out, void* stream);
/* coef: the clip output (coef at [1]); hyper (device): {lr, momentum, weight_decay, first_step,    */
/* halt}; halt != 0 skips the update (a non-finite loss, trainers/maple.py:375-376)               */
int mf_sgd_step(void* p, void* g, void* buf, int64_t n, int is16, const float* coef, const float* hyper,
                void* stream);
/* The optimizer step in three launches (clip partial sums, coefficient + halt latch, SGD over both flat
 * buffers): mf_clip_grad_norm + mf_sgd_step(fp16) + mf_sgd_step(fp32), with hyper[4] = max(hyper[4], *halt_src,
 * *input_flag) (the step's non-finite-loss flag and its non-finite-input flag, input_flag nullable) folded into
 * the coefficient launch.  Bit-identical to those calls.                                                     */
int mf_optimizer_step(void* p16, void* g16, void* b16, int64_t n16, float* p32, float* g32, float* b32, int64_t n32,
                      const void* chunks, int nchunks, float max_norm, float* part, float* out, float* hyper,
                      const float* halt_src, const int* input_flag, void* stream);
/* FedProx local step (Li, Sahu, Zaheer, Sanjabi, Talwalkar, Smith: "Federated Optimization in Heterogeneous
 * Networks", MLSys 2020): mf_sgd_step with the proximal gradient mu * (p - pglob) added after clipping, in the
 * optimizer, as weight decay is.  hyper (device) has 6 floats here: {lr, momentum, weight_decay, first_step, halt,
 * mu}.  Per element, every line rounded to the buffer's dtype T: g = gc = T(g * coef) (the stored gradient stays
 * the clipped model gradient); d = T(p - pglob); gp = T(gc + mu * d); d_p = T(gp + wd * p); momentum and parameter
 * update as mf_sgd_step.  mu == 0 (or pglob == p element-wise) gives mf_sgd_step's result bit for bit.  pglob
 * (n elements of T, the last global weights) is only read and must not overlap p, g or buf.               */
int mf_sgd_prox_step(void* p, void* g, void* buf, const void* pglob, int64_t n, int is16, const float* coef,
                     const float* hyper, void* stream);
/* mf_optimizer_step with the proximal SGD launch (three launches; the clip norm is the model gradient's): its
 * arguments plus the global copies of the two flat buffers.  Bit-identical to mf_clip_grad_norm + the halt latch +
 * mf_sgd_prox_step(fp16) + mf_sgd_prox_step(fp32).                                                           */
int mf_optimizer_step_prox(void* p16, void* g16, void* b16, int64_t n16, float* p32, float* g32, float* b32,
                           int64_t n32, const void* chunks, int nchunks, float max_norm, float* part, float* out,
                           float* hyper, const float* halt_src, const int* input_flag, const void* glob16,
                           const float* glob32, void* stream);
/* FedDyn local step (Acar, Zhao, Matas Navarro, Mattina, Whatmough, Saligrama: "Federated Learning Based on Dynamic
 * Regularization", ICLR 2021): the local objective gains -<lam, w> + (alpha/2) ||w - w_global||^2.  hyper (device):
 * {lr, momentum, weight_decay, first_step, halt, alpha}, alpha in the slot mf_sgd_prox_step reads mu from.  lam: the
 * client's linear correction, n fp32 elements whatever the buffer's dtype T (it accumulates alpha * (w - w_global)
 * over the rounds, increments an fp16 accumulator would round away), read only.  Per element, every line rounded to T,
 * the scalars fp32, no fused multiply-add:
 *   g = gc = T(g * coef);  d = T(p - pglob);  gp = T(gc + alpha * d);  gl = T(gp - lam)   (one fp32 subtraction,
 *   then the rounding to T);  d_p = T(gl + wd * p);  momentum and parameter update as mf_sgd_step.
 * lam == 0 gives mf_sgd_prox_step's result at mu = alpha bit for bit.  halt != 0 leaves p, g and buf untouched.
 * pglob and lam must not overlap p, g or buf.                                                                */
int mf_sgd_dyn_step(void* p, void* g, void* buf, const void* pglob, const float* lam, int64_t n, int is16,
                    const float* coef, const float* hyper, void* stream);
/* mf_optimizer_step_prox with the dynamic SGD launch (three launches): its arguments plus lam, n16 + n32 fp32
 * elements in the bucket's order [fp16 trainables | fp32 trainables]: the fp16 buffer's step reads lam[0:n16], the fp32
 * buffer's lam[n16:].  Bit-identical to mf_clip_grad_norm + the halt latch + mf_sgd_dyn_step(fp16, lam) +
 * mf_sgd_dyn_step(fp32, lam + n16); 8 elements per thread under mf_optimizer_step_prox's rule with lam 32-byte
 * aligned (lam + n16 then is exactly when n16 % 8 == 0).                                                      */
int mf_optimizer_step_dyn(void* p16, void* g16, void* b16, int64_t n16, float* p32, float* g32, float* b32,
                          int64_t n32, const void* chunks, int nchunks, float max_norm, float* part, float* out,
                          float* hyper, const float* halt_src, const int* input_flag, const void* glob16,
                          const float* glob32, const float* lam, void* stream);
/* Sample-weighted FedAvg (McMahan, Moore, Ramage, Hampson, Aguera y Arcas: "Communication-Efficient Learning of
 * Deep Networks from Decentralized Data", AISTATS 2017): w_global = sum_k n_k w_k / sum_k n_k.  The weight travels
 * in the bucket, n = n16 + n32: pack writes n + 2 floats, bucket[0:n] = fp32(weight) * float(p) (0 if
 * *invalid_flag), bucket[n] = weight (0 if invalid), bucket[n+1] = the vote (1 valid / 0 invalid); weight must be
 * finite and > 0.  After the sum over the clients (mf_fedavg_reduce_ordered or an all-reduce) unpack writes
 * fp16(bucket[i] / bucket[n]) into every trainable and into g16/g32; a vote count bucket[n+1] == 0 restores the
 * trainables from g16/g32, as mf_fedavg_unpack does.  The product is rounded to fp32 before the sum (no fused
 * multiply-add across pack and reduce), so equal power-of-two weights give mf_fedavg_pack/unpack's result bit for
 * bit.                                                                                                         */
int mf_fedavg_pack_weighted(const void* p16, int64_t n16, const float* p32, int64_t n32, const int* invalid_flag,
                            float weight, float* bucket, void* stream);
int mf_fedavg_unpack_weighted(const float* bucket, void* p16, int64_t n16, float* p32, int64_t n32, void* g16,
                              float* g32, void* stream);
/* bucket[0:n16+n32] = this client's trainables as fp32 (0 if *invalid_flag), bucket[n16+n32] = its vote
 * (1 valid / 0 invalid); after an all-reduce(SUM) of the n16+n32+1 floats, unpack writes
 * fp16(sum / n_valid) into every trainable and into the global copy g16/g32, n_valid read from
 * bucket[n16+n32] on the device; n_valid == 0 (every client failed) restores the trainables from g16/g32.
 * Replaces: safe_average_weights + broadcast_weights' load_state_dict (trainers/maple_fed.py:309-315,327-331). */
int mf_fedavg_pack(const void* p16, int64_t n16, const float* p32, int64_t n32, const int* invalid_flag,
                   float* bucket, void* stream);
int mf_fedavg_unpack(const float* bucket, void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32,
                     void* stream);
/* FedOpt server optimizers, applied to the summed bucket in mf_fedavg_unpack's place: FedAvgM (Hsu, Qi, Brown:
 * "Measuring the Effects of Non-Identical Data Distribution for Federated Visual Classification", 2019) and
 * FedAdagrad / FedAdam / FedYogi (Reddi et al.: "Adaptive Federated Optimization", ICLR 2021, Algorithm 2; no bias
 * correction).  opt: 1 fedavgm, 2 fedadagrad, 3 fedadam, 4 fedyogi.  bucket is the sum over the clients in the
 * plain layout (weighted = 0: n floats, then the vote count) or the weighted one (weighted = 1: n floats, the summed
 * weights, the vote count), n = n16 + n32.  x, m, v: the server's fp32 master copy of the trainables and its two
 * moments, n floats each in the bucket's order [fp16 trainables | fp32 trainables]; v is neither read nor written
 * by fedavgm (may be null).  Rounding points: per element every binary operation below is one IEEE fp32 operation
 * (round to nearest even, no fused multiply-add); beta1, beta2, tau, eta are fp32 and 1 - beta1, 1 - beta2 are fp32
 * differences formed in the kernel; division and sqrtf are correctly rounded:
 *   d = bucket[n];  mean = bucket[i] / d;  delta = mean - x
 *   fedavgm:    m = beta1*m + delta;                                upd = m
 *   adaptive:   m = beta1*m + (1-beta1)*delta;  s = delta*delta
 *     fedadagrad: v = v + s
 *     fedadam:    v = beta2*v + (1-beta2)*s
 *     fedyogi:    v = v - ((1-beta2)*s) * sign(v - s),  sign(0) = 0
 *                                                                   upd = m / (sqrtf(v) + tau)
 *   x = x + eta*upd;  val = fp16(x);  p16 = g16 = val;  p32 = g32 = float(val)
 * so the clients receive what a `.half()` state dict would hold (mf_fedavg_unpack's contract, the fp32 LayerNorm
 * parameters and logit_scale included) and only x is fp32.  A vote count of 0 restores the trainables from g16 / g32
 * and leaves x, m, v untouched.  An x outside the fp16 range is delivered as +-inf.  8 elements per thread when
 * n16 % 8 == n32 % 8 == 0 and the pointers are 32-byte aligned (16 for p16 / g16), one per thread otherwise; the
 * same bits either way.  x, m, v, the bucket and the weight buffers must not overlap.  Errors: negative sizes, an
 * unknown opt, a non-finite hyper-parameter, tau <= 0 for an adaptive optimizer, a null state pointer.            */
int mf_fedopt_step(const float* bucket, int weighted, int opt, float beta1, float beta2, float tau, float eta,
                   float* x, float* m, float* v, void* p16, int64_t n16, float* p32, int64_t n32, void* g16,
                   float* g32, void* stream);
/* val = fp16(x) into another client's trainables and global copy (p16 = g16 = val, p32 = g32 = float(val)): the
 * second and later clients of a rank after mf_fedopt_step wrote the first.  Changes no state.                    */
int mf_fedopt_deliver(const float* x, void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32,
                      void* stream);
/* FedDyn's round end (Acar et al., ICLR 2021, Algorithm 1), one launch per local client in mf_fedavg_unpack's place
 * on the summed plain bucket [sum over the valid clients | votes], n = n16 + n32.  h: the server's state, the mean of
 * the N = num_clients clients' lam, n fp32 elements in the bucket's order; lam: this client's correction, the same
 * shape; flag: the client's device flag (non-zero: invalid or failed, it did not take part).  Per element i, with
 * w = float(p_i) the client's local weight and q = float(g_i) the round's starting weight (its global copy), both
 * read before anything is written, every binary operation one IEEE fp32 operation, no fused multiply-add;
 * frac = votes / (float)N and af = alpha * frac are formed once in the kernel:
 *   votes == 0:   p = g;  h and lam untouched
 *   client:       if *flag == 0:  lam = lam - alpha * (w - q)
 *   server:       mean = sum / votes;  h = h - af * (mean - q)             (mf_feddyn_step only)
 *   both:         mean = sum / votes;  x = mean - h / alpha  (the stepped h);
 *                 val = fp16(x);  p16 = g16 = val;  p32 = g32 = float(val)
 * An absent client keeps its lam (the paper's rule for a device that did not take part) and reaches h through frac.
 * mf_feddyn_deliver serves the rank's second and later clients: it reads the stepped h and the same bucket, so it
 * recomputes the same x (no fp32 copy of x is kept), and updates that client's own lam from its own p and g.
 * 8 elements per thread when n16 % 8 == n32 % 8 == 0 and bucket, h, lam, p32, g32 are 32-byte aligned (p16 / g16:
 * 16), one per thread otherwise; the same bits either way.  h, lam, the bucket and the weight buffers must not
 * overlap.  Errors: negative sizes, alpha not finite and > 0, num_clients < 1, a null pointer.                     */
int mf_feddyn_step(const float* bucket, float alpha, int num_clients, float* h, float* lam, const int* flag,
                   void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32, void* stream);
int mf_feddyn_deliver(const float* bucket, float alpha, const float* h, float* lam, const int* flag, void* p16,
                      int64_t n16, float* p32, int64_t n32, void* g16, float* g32, void* stream);
/* FedAvg in client order (trainers/maple_fed.py:311-314: torch.stack over the clients, then mean):   */
/* out[i] = sum_c gathered[c * stride + i] accumulated c = 0, 1, ... in fp32, for i < n; gathered    */
/* holds every client's packed bucket (an all-gather of mf_fedavg_pack outputs)                      */
int mf_fedavg_reduce_ordered(const float* gathered, int nclients, int64_t stride, int64_t n, float* out,
                             void* stream);
/* Robust aggregation: the coordinate-wise median and beta-trimmed mean of Yin, Chen, Ramchandran, Bartlett
 * ("Byzantine-Robust Distributed Learning: Towards Optimal Statistical Rates", ICML 2018) over the image
 * mf_fedavg_reduce_ordered sums (gathered[c * stride + i], c < nclients <= 64, i < n).  Per coordinate i, with the
 * nclients fp32 values v_c:
 *   - a NaN of any sign or payload marks client c absent; m = the number of present values (+-Inf are present);
 *   - the present values are sorted ascending in the IEEE total order (-0 before +0): s_0 <= ... <= s_{m-1};
 *   - k = min(trim_k, (m - 1) / 2) (integer division; k = 0 when m = 0): a trim that would leave nothing degrades to
 *     the median, so a large trim_k is the median (for even m the fp32 mean of the two middle values);
 *   - acc = s_k; acc += s_j for j = k + 1 .. m - 1 - k in ascending order, one IEEE fp32 add each (no fused
 *     multiply-add; a lone -0 stays -0);
 *   - out[i] = acc / float(m - 2k), correctly rounded; m = 0 gives +0;
 *   - out[count_pos] = float(m) instead (count_pos < 0: no such element).
 * A sum in sorted order depends on neither the client order nor on how the clients are laid out over the ranks.
 * gathered and out must not overlap.  16-byte loads when stride % 4 == 0 and both pointers are 16-byte aligned
 * (up to 16 clients), 4-byte loads otherwise and on the ragged tail; the same bits either way.
 * Errors: nclients < 1 or > 64, trim_k < 0, n < 0 or stride < n, count_pos >= n.                               */
int mf_fedavg_reduce_trimmed(const float* gathered, int nclients, int64_t stride, int64_t n, int trim_k,
                             int64_t count_pos, float* out, void* stream);
/* The bucket of the robust aggregation, n + 2 floats (n = n16 + n32): mf_fedavg_pack_weighted's layout at weight 1,
 * [float(trainables) | 1 | 1], and an invalid client writes the quiet NaN 0x7fc00000 (absent) into all of them.
 * Reduced by mf_fedavg_reduce_trimmed with count_pos at the last element it reads [statistic | 1 | m], which
 * mf_fedavg_unpack_weighted and mf_fedopt_step / mf_fedopt_deliver (weighted = 1) consume as they are.          */
int mf_fedavg_pack_robust(const void* p16, int64_t n16, const float* p32, int64_t n32, const int* invalid_flag,
                          float* bucket, void* stream);
/* ---- Multi-Krum (Blanchard, El Mhamdi, Guerraoui, Stainer: "Machine Learning with Adversaries: Byzantine Tolerant
 * Gradient Descent", NeurIPS 2017; keeping the m best: El Mhamdi, Guerraoui, Rouault, ICML 2018): whole clients are
 * kept or dropped by their squared L2 distances to their nearest peers, over the image mf_fedavg_reduce_trimmed reads
 * (gathered[c * stride + t], c < nclients <= 64, t < n; an absent client is NaN everywhere).  Every argument check
 * returns before any launch; plain vector stores, no float atomics.
 *
 * The distances, two launches, no host synchronisation, bit-identical run to run:
 *   D[i][j] = sum_t (double)(x_i[t] - x_j[t])^2 for i <= j, mirrored to D[j][i]: one fp32 subtract, the square and
 *   the sum in fp64 (the square of an fp32 value is exact in fp64, so a fused multiply-add gives mul + add's bits).
 *   The diagonal is computed like any pair: +0 for a present client, NaN for an absent one, which is how absence is
 *   read later.  All n coordinates take part; a difference of +-inf gives +inf.  Never formed from a Gram matrix.
 *   Order of summation: a workgroup owns a chunk of mf_krum_chunk_elems() coordinates and an 8 x 8 tile of client
 *   pairs; thread t of 256 adds the groups of 4 coordinates t, t + 256, ... of the chunk in ascending order (one
 *   16-byte load per client when stride % 4 == 0 and gathered is 16-byte aligned, 4-byte loads otherwise and on the
 *   ragged tail: the same bits either way), the 64 lanes of a wave are added by an xor butterfly (32, 16, .., 1), the 4
 *   waves in order, and the second launch adds the chunk partials in chunk order (16 contiguous runs, then the runs in
 *   order).  So D is a fixed function of (nclients, n, stride) and the values; the number of workgroups does not depend
 *   on the device.  n = 0 writes the all-zero matrix.
 * ws: mf_krum_ws_bytes(nclients, n) bytes, 8-byte aligned (-1 for nclients outside 1..64 or n < 0); dist: nclients^2
 * doubles, row-major.  Errors: nclients outside 1..64, n < 0 or stride < n, a null or misaligned ws / dist, a null
 * gathered with n > 0.                                                                                            */
int64_t mf_krum_ws_bytes(int nclients, int64_t n);
int mf_krum_chunk_elems(void);
int mf_krum_pairwise(const float* gathered, int nclients, int64_t stride, int64_t n, void* ws, double* dist,
                     void* stream);
/* The selection, one workgroup, a deterministic function of (parts, f, m).  parts: [nparts][nclients^2] doubles, the
 * distance matrices of the coordinate shards:
 *   - D = parts[0] + parts[1] + ... + parts[nparts - 1] per entry, sequential fp64 adds starting from part 0;
 *   - client i is present when D[i][i] is not NaN; p = the number of present clients; p = 0 selects nothing;
 *   - f' = max(min(f, (p - 3) div 2), 0): an f the present clients cannot carry degrades;
 *   - q = max(p - f' - 2, 0); score_i = the sum of the q smallest D[i][j] over present j != i, the terms taken in
 *     ascending (value, j) order, sequential fp64 adds starting from the first term (q = 0: +0);
 *   - m' = p - f' when m = 0 (Multi-Krum), else min(m, p - f') (m = 1: Krum);
 *   - the m' present clients lowest in (score, index) are selected.
 * selected[c] = 0 or 1; scores[c] = score_c, the quiet NaN 0x7ff8000000000000 for an absent client; counts =
 * {p, f', m'}.  Errors: nparts < 1, nclients outside 1..64, f < 0, m < 0, a null pointer.                        */
int mf_krum_select(const double* parts, int nparts, int nclients, int f, int m, int* selected, double* scores,
                   int* counts, void* stream);
/* The mean of the selected clients in mf_fedavg_reduce_trimmed's place.  selected (nclients ints, non-zero =
 * selected) is read on the device; m' = their number.  Per coordinate t < n:
 *   - acc = the first selected client's value; acc += the next one's, in client order, one IEEE fp32 add each;
 *   - out[t] = acc / float(m'), correctly rounded; m' = 0 gives +0;
 *   - an unselected client is skipped by a select, never multiplied by 0: an absent client's NaNs do not leak;
 *   - out[count_pos] = float(the number of non-NaN values at that coordinate over all clients) instead (count_pos
 *     < 0: no such element), as mf_fedavg_reduce_trimmed counts, so the reduced robust bucket reads
 *     [statistic | 1 | p].
 * gathered and out must not overlap.  16-byte loads when stride % 4 == 0 and both pointers are 16-byte aligned,
 * 4-byte loads otherwise and on the ragged tail; the same bits either way.
 * Errors: nclients < 1 or > 64, n < 0 or stride < n, count_pos >= n, a null pointer with n > 0.                  */
int mf_fedavg_reduce_selected(const float* gathered, int nclients, int64_t stride, int64_t n, const int* selected,
                              int64_t count_pos, float* out, void* stream);
/* ---- DP-FedAvg (McMahan, Ramage, Talwar, Zhang: "Learning Differentially Private Recurrent Language Models",
 * ICLR 2018): per-client update clipping and Gaussian noise on the sum.  Every fp32 operation named below is one
 * IEEE operation rounded on its own (no fused multiply-add), no float atomics, logf / sqrtf / sinf / cosf are the
 * library functions, and every argument check returns before any launch.
 *
 * The update's L2 norm and the clip scale, two launches, no host synchronisation, bit-identical run to run:
 *   d_i   = float(p_i) - float(g_i), one fp32 subtract, over [p16 | p32] against [g16 | g32];
 *   norm  = sqrt(sum_i d_i * d_i): per chunk of 8192 elements of either buffer an fp32 partial sum (16-byte loads over
 *           the middle that is 16-byte aligned in p and g alike, element loads for the ragged ends or throughout), then
 *           one block adds the partial sums in chunk order in fp64 and rounds the square root to fp32;
 *   out[0] = norm;  out[1] = scale = clip / norm (one fp32 divide) when norm > clip, else exactly 1.0f -- also for a
 *           NaN norm, whose client the validity flag excludes;  out[2] = 1.0f when clipped, else 0.
 * ws: mf_dp_update_ws_floats(n16, n32) floats (-1 for a negative size).  Errors: a negative size, clip not > 0, a
 * null ws / out, a null buffer of a non-zero size.                                                               */
int64_t mf_dp_update_ws_floats(int64_t n16, int64_t n32);
int mf_dp_update_scale(const void* p16, const void* g16, int64_t n16, const float* p32, const float* g32, int64_t n32,
                       float clip, float* ws, float* out, void* stream);
/* The bucket of a clipped client.  layout 0: mf_fedavg_pack's [y | 1]; 1: mf_fedavg_pack_weighted's
 * [w * y | w | 1]; 2: mf_fedavg_pack_robust's [y | 1 | 1] (weight unread).  An invalid client writes zeros in layouts
 * 0 and 1 and the quiet NaN 0x7fc00000 in layout 2, everywhere.  With s = *scale_ptr read on the device
 * (mf_dp_update_scale's out + 1), per element x = float(p), g = float(global copy):
 *   s >= 1:  y = x (a select: the bits of the three entry points above);
 *   else:    y = g + s * (x - g): d = x - g, sd = s * d, y = g + sd, three fp32 operations;
 * then the layout's w * y.  The bucket keeps holding weights: the sum over m valid clients is m * g + sum s_k d_k, so
 * every reduce, unpack and server step consumes it unchanged.  ||y - g||_2 <= clip up to the rounding of g + sd, about
 * sqrt(n) * 2^-24 * max|y|.  Errors: a negative size, layout outside 0..2, layout 1 with a weight outside (0, inf), a
 * null scale_ptr, bucket, or buffer of a non-zero size.                                                           */
int mf_fedavg_pack_clipped(const void* p16, int64_t n16, const float* p32, int64_t n32, const void* g16,
                           const float* g32, const int* invalid_flag, const float* scale_ptr, float weight, int layout,
                           float* bucket, void* stream);
/* buf[j] = buf[j] + std * z(offset + j) for j in [0, n): one fp32 multiply and one fp32 add.  z(i), the standard
 * normal of global coordinate i, depends on (seed, round, i) alone:
 *   q = i >> 2, lane = i & 3;
 *   (x0, x1, x2, x3) = Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC 2011; multipliers 0xD2511F53, 0xCD9E8D57, key
 *     increments 0x9E3779B9, 0xBB67AE85) of the counter (q_lo, q_hi, round, 0) under the key (seed_lo, seed_hi);
 *   u(x) = float(((x >> 9) << 1) | 1) * 2^-24, an odd multiple of 2^-24 in (0, 1), exact in fp32;
 *   lanes 0, 1 take (a, b) = (x0, x1), lanes 2, 3 (x2, x3);  r = sqrtf(-2 * logf(u(a))), theta = 6.2831855f * u(b);
 *   an even lane gives r * cosf(theta), an odd one r * sinf(theta).
 * So any split of a coordinate range over calls, ranks or shards gives the same bits.  One thread owns one counter;
 * a counter wholly inside the call at a 16-byte aligned address takes one 16-byte load and store, any other element
 * accesses, with the same arithmetic; nothing outside buf[0, n) is touched.  std = 0 (or n = 0) launches nothing, so
 * the buffer keeps its bits.  Errors: n < 0, offset < 0, offset + n > INT64_MAX, std negative or not finite, a null
 * or misaligned buf.                                                                                             */
int mf_dp_add_noise(float* buf, int64_t n, int64_t offset, uint64_t seed, uint32_t round, float std, void* stream);
/* ---- int8 compression of the FedAvg uplink with error feedback (QSGD: Alistarh, Grubic, Li, Tomioka, Vojnovic, NeurIPS
 * 2017; error feedback: Seide et al. 2014, Karimireddy, Rebjock, Stich, Jaggi, ICML 2019).  Every fp32 operation named
 * below is one IEEE operation rounded on its own (no fused multiply-add), no float atomics, plain vector stores only, and
 * every argument check returns before any launch.
 *
 * Coordinates i in [0, n), n = n16 + n32, run over [fp16 trainables | fp32 trainables], the bucket's order.  The
 * quantisation block is B = 256 consecutive coordinates; a block may straddle the fp16 / fp32 boundary, and coordinates
 * >= n of the padded bucket [0, world * S) count as u = 0.  S, the shard length, is a multiple of 256.
 *
 * Quantise (x the client's weights, g the global copy, e its fp32 residual):
 *   d_i = float(x_i) - float(g_i);  u_i = d_i + e_i (two fp32 operations; e_in == e_out == null: error feedback off,
 *         e is neither read nor written and u_i = d_i);
 *   per block: amax = max |u_i| (order-independent, exact), scale = amax / 127.0f (one divide); amax == 0 gives scale 0,
 *         all codes 0 and e'_i = u_i;
 *   t = u_i / scale (one divide), f = floorf(t);
 *   rounding 0 (nearest):    q = rintf(t);
 *   rounding 1 (stochastic): p = t - f (exact), q = f + (r_i < p ? 1 : 0), r_i = float(w >> 8) * 2^-24 in [0, 1), w the
 *         word i & 3 of Philox4x32-10 (mf_dp_add_noise's generator) on the counter (c_lo, c_hi, round,
 *         0x80000000 | client), c = i >> 2, under the key (seed_lo, seed_hi): the counter's last word keeps these streams
 *         apart from the noise streams, client is the global client index, and the bits depend on (seed, round, client, i)
 *         alone;
 *   q = fminf(fmaxf(q, -127), 127) (amax / (amax / 127) can round above 127; a NaN becomes -127, so only finite values
 *         are converted), stored as int8;
 *   e'_i = u_i - scale * q (one multiply, one subtract), written to e_out, a second buffer (e_in is only read, so a
 *         repeated call gives the same codes).
 * A client whose *invalid_flag is set (read on the device) writes codes 0, scales 0, weight 0 and vote 0 and copies e to
 * e' unchanged; no weight of it is read.
 *
 * Wire chunk per (destination rank r, client), mf_compress_chunk_bytes(S) = S + S / 64 + 8 bytes (-1 unless S is a
 * positive multiple of 256): [S int8 codes | S / 256 fp32 scales | fp32 weight | fp32 vote], the codes and scales of the
 * coordinates [r * S, r * S + S); weight = `weight` (1 for the plain and the robust layout), 0 if invalid; vote = 1, 0 if
 * invalid; the two are replicated into every chunk.  mf_compress_quantize writes the `world` chunks of one client
 * at image + r * rank_stride (bytes; image 4-byte aligned, rank_stride a multiple of 4): the exchange's send image
 * [destination rank][local client][chunk] is written in place.  One wave64 per block, four coordinates per lane (one
 * Philox counter), the max a wave reduction, the four codes one 32-bit store; 8- or 16-byte loads and stores wherever
 * an address allows, element accesses otherwise, the same bits either way.  Errors: negative sizes, S not a positive
 * multiple of 256, world < 1, world * S < n, an unknown rounding, a weight outside (0, inf), client >= 2^31, a null or
 * misaligned image, a null flag, a null buffer of a non-zero size, one residual pointer without the other or both the
 * same.
 *
 * Decode: nclients chunks at image + c * chunk_stride (bytes) into out + c * out_stride (floats), S floats each: chunk
 * c holds the coordinates i = first + c * first_step + j, j < S (first_step 0: every client's shard `first` of a
 * received image; first_step S with chunk_stride the rank stride: one client's whole bucket).  It writes the fp32 image
 * mf_fedavg_reduce_ordered / _trimmed read, in layout 0 (mf_fedavg_pack), 1 (mf_fedavg_pack_weighted) or 2
 * (mf_fedavg_pack_robust):
 *   i < n:       y = float(g_i) + scale * q (one multiply, one add), then w * y (layout 1) or y (0, 2);
 *   i == n:      the vote (0) or the weight (1, 2);   i == n + 1: the vote (1, 2);   beyond: +0;
 *   a chunk whose vote is 0: zeros everywhere (0, 1) or the quiet NaN 0x7fc00000 everywhere (2)
 * -- the bits those pack kernels write for an invalid client, and for a valid one for the weights g + scale * q.
 * Errors: negative sizes, first or first_step, S not a positive multiple of 256, nclients outside 1..65535, an unknown
 * layout, a null or misaligned image or out, a null global copy of a non-zero size, a stride below its element.      */
int64_t mf_compress_chunk_bytes(int64_t S);
int mf_compress_quantize(const void* x16, const void* g16, int64_t n16, const float* x32, const float* g32, int64_t n32,
                         const float* e_in, float* e_out, const int* invalid_flag, float weight, int rounding,
                         uint64_t seed, uint32_t round, uint32_t client, void* image, int64_t rank_stride, int64_t S,
                         int world, void* stream);
int mf_compress_decode(const void* image, int64_t chunk_stride, int nclients, int64_t S, int64_t first,
                       int64_t first_step, const void* g16, int64_t n16, const float* g32, int64_t n32, int layout,
                       float* out, int64_t out_stride, void* stream);
/* ---- block-wise top-k sparsification of the FedAvg uplink with error feedback (Aji & Heafield, EMNLP 2017; Stich,
 * Cordonnier, Jaggi, NeurIPS 2018; Lin et al., ICLR 2018; Sattler et al. 2019): the second codec of the same exchange.
 * What the int8 pair states above holds here unchanged and is written once in the code (csrc/compress.hip): the
 * coordinates, the blocks of B = 256 and the padding; the update u_i = d_i + e_i, or d_i without a residual; the
 * residual's two buffers; the invalid client (an all-zero payload, weight 0, vote 0, e' = e, no weight read); the
 * {weight, vote} tail that closes every chunk and the `world` chunks at image + r * rank_stride; the decode's chunks,
 * strides, first and first_step, its elements at n, n + 1 and beyond; and the rules (one IEEE operation at a time, no
 * float atomics, plain vector stores, every check before any launch).  Only the following is this codec's.
 * 1 <= k <= 64.
 *
 * Select: mag_i = the bits of u_i with the sign bit cleared, as an unsigned integer (a total order that places inf and
 * NaN too).  Within a block a precedes b iff mag_a > mag_b, or mag_a == mag_b and a has the lower index; the first k
 * are kept (an all-zero block, or one past n: the indices 0 .. k - 1 with value 0).  The kept entries travel in ascending
 * index order, each as (uint8 index within the block, fp32 u_i with its sign).  e'_i = +0 for a kept coordinate, u_i for
 * the others, written to e_out for i < n.
 *
 * Wire chunk, nb = S / 256 blocks: [nb * k fp32 values | nb * k uint8 indices | zero bytes up to a multiple of 4 | the
 * tail], block b's entries at b * k .. b * k + k - 1 of either region: mf_topk_chunk_bytes(S, k) = 4 nb k +
 * 4 ceil(nb k / 4) + 8 bytes (-1 unless S is a positive multiple of 256 and 1 <= k <= 64).  One wave64 per block, four
 * coordinates per lane; the k-th largest of the 39-bit keys (mag << 8) | (255 - index) is found most significant bit
 * first, each step a count by ballot and popcount across the wave; a kept coordinate's position is the count of kept
 * coordinates before it.  Errors: those of mf_compress_quantize (no rounding, no client), and k outside 1..64.
 *
 * Decode: s_i = the entry's value if i is a kept coordinate, +0 otherwise (with a repeated index any one of its entries
 * wins; an index is a byte and cannot leave its block);  y = float(g_i) + s_i, always the one fp32 add, then w * y
 * (layout 1) or y (layout 0).  Layouts 0 and 1 only, so a chunk whose vote is 0 decodes to zeros.  One wave per block
 * per chunk, the entries scattered through a 1 KB tile of LDS.  Errors: those of mf_compress_decode, layout 2, and k
 * outside 1..64.  In either pair a codec's own arguments (rounding and client; k) are checked ahead of the shared
 * ones.                                                                                                            */
int64_t mf_topk_chunk_bytes(int64_t S, int k);
int mf_topk_select(const void* x16, const void* g16, int64_t n16, const float* x32, const float* g32, int64_t n32,
                   const float* e_in, float* e_out, const int* invalid_flag, float weight, int k, void* image,
                   int64_t rank_stride, int64_t S, int world, void* stream);
int mf_topk_decode(const void* image, int64_t chunk_stride, int nclients, int64_t S, int64_t first, int64_t first_step,
                   const void* g16, int64_t n16, const float* g32, int64_t n32, int layout, float* out,
                   int64_t out_stride, int k, void* stream);
int mf_nonfinite_flag(const void* x, int64_t n, int is16, int* flag, void* stream);

/* ---- image transforms (data step before the path) ---------------------
 * Replaces the CPU transform workers the reference builds from configs/trainers/MaPLeFederated/
 * *.yaml:8-13 (Dassl build_transform -> torchvision RandomResizedCrop / RandomHorizontalFlip /
 * Resize + CenterCrop / ToTensor / Normalize on Pillow images, bicubic) and the fp16 cast at
 * trainers/maple.py:336.  Per image b, geom_host[b*11 ..] = {H, W, y0, x0, ch, cw, RH, RW, oy, ox,
 * flip} (HOST memory): crop [y0, y0+ch) x [x0, x0+cw) of the HxWx3 uint8 image at src + src_off[b],
 * resample it Pillow-exactly (interp 0 bicubic, 1 bilinear; 22-bit fixed-point taps, uint8
 * intermediate) to RH x RW, keep the out_h x out_w window at (oy, ox), flip it horizontally when
 * flip != 0, and store (u/255 - mean_c)/std_c as fp16 (out_f16) or fp32, planar [B][3][out_h][out_w].
 * src_off_host / src_off: the same byte offsets on the host (validated) and on the device.
 * ws: device workspace of mf_augment_ws_bytes(B, out_h, out_w, max crop height) bytes.         */
int64_t mf_augment_ws_bytes(int B, int out_h, int out_w, int max_rows);
int mf_augment(const void* src, int64_t src_bytes, const int64_t* src_off_host, const int64_t* src_off,
               const int* geom_host, int B, int out_h, int out_w, int interp, float mean0, float mean1, float mean2,
               float std0, float std1, float std2, void* out, int out_f16, void* ws, int64_t ws_bytes,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPFED_H_ */
