/*
 * madeleine_amd.h -- C ABI of libmadeleine_amd.so (gfx950 / MI355X).
 *
 * The reference (mahmoodlab/MADELEINE) has no FFI / operator registry: its hot path is plain
 * PyTorch modules.  This header is therefore the boundary the reference's *call sites* would bind
 * if the path were native; every entry point names the reference code it replaces (file:line are
 * relative to the reference checkout).  The Python mirror of the reference classes
 * (madeleine_amd/{model,abmil,loss,trainer}.py) calls these through ctypes with raw device pointers
 * (see INTEGRATION.md for the binding stub).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the CALLER allocates all
 *     inputs, outputs and workspaces.  Kernels never allocate, free or keep global state; they are
 *     re-entrant.
 *   - launches are asynchronous on the caller-provided hipStream_t (passed as void*); no internal
 *     synchronisation.
 *   - return value: 0 on success; a positive hipError_t if a launch failed; a negative MDL_E_* code
 *     for argument validation.  Nothing throws across the boundary.
 *   - row strides (ldE, ldx, ldy, lddx, lddy, ldc in elements; rsb, a_rsb, b_rsb, e_rsb in bytes): any value that is at least the row
 *     width, keeps every row 16-byte aligned (fp32: a multiple of 4 elements, bf16: of 8 -- 4 on the pooling entry points, whose lanes
 *     load 4 elements; bytes: of 16) and stays within the entry point's upper limit.  The limits exist where a kernel adds
 *     (row inside its tile) x stride + column bytes in 32 bits; each is stated beside the argument as that expression, which must not
 *     exceed 2^31 - 1.  Below the width or misaligned: MDL_E_ARG (the bf16 Linears: MDL_E_UNSUPPORTED for a stride that is not a
 *     multiple of 8); above the limit: MDL_E_UNSUPPORTED.  All of it is checked before anything is launched, empty problems included.
 *     A strided operand may be a column slice of a wider buffer: no kernel reads or writes the bytes between the end of a row and
 *     the start of the next.
 *   - fp32 values everywhere.  Contractions come in three engines: the *_split entry points (the DEFAULT of the Python
 *     mirror: every fp32 operand as an fp16 hi + lo image under a power-of-two scale, three v_mfma_f32_32x32x16_f16 products
 *     per logical product, fp32 accumulation -- error below an fp32 fmaf chain), the plain entry points (exact fp32,
 *     v_mfma_f32_32x32x2_f32; MADELEINE_GEMM=fp32) and the *_bf16 entry points at the end of this header (the reference's
 *     `precision: bfloat16` mode: bf16 activation storage and bf16 MFMA operands, fp32 accumulation / epilogues / parameters).
 *
 * Entry points by row of SURVEY.md section 8:  A2 mdl_abmil_gate_*  |  A3 mdl_abmil_pool_*  |  A2+A3 fused backward
 * mdl_abmil_attnpool_bwd  |  L1 mdl_infonce_*  |  G0-G3 mdl_got_*  |  N1 mdl_linear_*, mdl_ln_gelu_drop_*  |  bf16 mode *_bf16.
 *
 * Internal activation layout ("head-major"): the reference interleaves heads as channel j = e*H + c
 * (rearrange 'b t (e c) -> b t e c', Model.py:396).  Our encoder emits the same numbers with the
 * channel axis permuted to j' = c*512 + e by permuting the rows of pre_attn.8 / LayerNorm 9 and the
 * columns of token_projector / projector on the host (madeleine_amd/model.py) -- zero-cost, and every
 * kernel below then reads contiguous 2 KiB head rows.  H (heads) <= 8, hidden = 512 fixed
 * (Model.py:71).
 */
#ifndef MADELEINE_AMD_H
#define MADELEINE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_HIDDEN 512
#define MDL_MAX_HEADS 8

#define MDL_OK 0
#define MDL_E_ARG (-1)      /* bad size / null pointer */
#define MDL_E_ALIGN (-2)    /* pointer not 16-byte aligned */
#define MDL_E_UNSUPPORTED (-3)

/* library / build info: returns a static string "madeleine_amd <ver> gfx950" */
const char* mdl_version(void);

/* ABI revision of this header: bumped whenever an entry point's argument list changes.  A binding compares
 * mdl_abi_version() with the MDL_ABI_VERSION it was written against BEFORE calling anything else, so that a stale
 * shared object fails loudly instead of being called with shifted arguments. */
#define MDL_ABI_VERSION 26
int mdl_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * A2 -- gated attention scores.  Replaces BatchedABMIL.forward (madeleine/models/abmil.py:41-68)
 * for all H heads at once (the reference loops H module instances, Model.py:406-409).
 *
 *   s[t,c] = bc[c] + sum_j wc[c,j] * drop(tanh(E[t,c,:].Wa[c,j,:] + ba[c,j])) * drop(sigmoid(E[t,c,:].Wb[c,j,:] + bb[c,j]))
 *
 * E      [T, H*512]  head-major token embeddings (row stride ldE floats, >= H*512, % 4 == 0, 127 * 4 ldE + 48 <= 2^31 - 1)
 * Wa,Wb  [H,512,512] torch Linear layout [out,in];  ba,bb [H,512];  wc [H,512];  bc [H]
 * scores [T,H]       raw (pre-softmax) attention, == raw_attention of Model.py:406-411
 * act_a, act_b [T,H,512]  tanh / sigmoid activations BEFORE dropout, saved for backward (may be NULL
 *                    when no backward is needed: inference)
 * dropout: p_drop in [0,1). keep_a/keep_b (uint8 [T,H,512], 1 = keep) inject explicit masks (parity
 *          tests); when NULL and p_drop > 0 a counter-based hash of (seed, element index) decides.
 *          p_drop == 0 (module.eval()) => identity.
 * ws     workspace of mdl_abmil_gate_fwd_ws_bytes(T,H) bytes (K-major copy of the weights + score partials per
 *        128-wide j tile).
 * Refusals of every gate entry point -- the forwards and backwards here, in the bf16 mode and on the split engine, mdl_abmil_attnpool_bwd
 * (_phases) included -- come in one order: (1) MDL_E_ARG: a required pointer is NULL, one of act_a / act_b (forward) or of keep_a / keep_b
 * is, the pooling term is incomplete, phases, terms, T < 0, H outside 1 .. MDL_MAX_HEADS, a stride below the row width or off its
 * alignment, p_drop outside [0,1); (2) MDL_E_ALIGN: E, Wa, Wb, wc, act_a, act_b, dE or ws is not 16-byte aligned; (3) MDL_E_UNSUPPORTED:
 * H not in {1,2,4,8}, a stride above its 32-bit limit; (4) a forward with T == 0 returns MDL_OK before any launch (an empty backward
 * still zeroes its gradients); (5) MDL_E_UNSUPPORTED: a launch grid above 2^31 - 1.
 */
int64_t mdl_abmil_gate_fwd_ws_bytes(int64_t T, int H);
int mdl_abmil_gate_fwd(const float* E, int64_t ldE, const float* Wa, const float* ba, const float* Wb,
                       const float* bb, const float* wc, const float* bc, float* scores, float* act_a,
                       float* act_b, int64_t T, int H, float p_drop, uint64_t seed,
                       const uint8_t* keep_a, const uint8_t* keep_b, void* ws, void* stream);

/* Backward of the above.  d_scores [T,H] incoming gradient.
 * dE [T,H*512] (row stride ldE, the SAME stride as E: one argument serves both; 15 * 4 ldE + 1020 <= 2^31 - 1 in the backward entry
 *    points, mdl_abmil_attnpool_bwd(_phases) included): gradient wrt the token embeddings through the gates; written when
 *    accumulate == 0, added to the existing contents when accumulate != 0.
 * dWa,dWb [H,512,512]; dba,dbb,dwc [H,512]; dbc [H] (may be NULL)  -- all overwritten.
 * ws: mdl_abmil_gate_bwd_ws_bytes(T,H) bytes: d(za)|d(zb) [T+16,H,1024] (computed once, then both GEMMs are pure
 *     LDS-DMA contractions) + split-K slabs + column-sum partials. */
int64_t mdl_abmil_gate_bwd_ws_bytes(int64_t T, int H);
int mdl_abmil_gate_bwd(const float* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc,
                       const float* act_a, const float* act_b, const float* d_scores, float* dE,
                       int accumulate, float* dWa, float* dWb, float* dba, float* dbb, float* dwc,
                       float* dbc, int64_t T, int H, float p_drop, uint64_t seed, const uint8_t* keep_a,
                       const uint8_t* keep_b, void* ws, void* stream);

/* Materialises the keep-mask the two calls above derive from (seed, p_drop) when keep_a/keep_b are NULL:
 * keep uint8 [T,H,512], which = 0 (tanh branch) or 1 (sigmoid branch).  For reproducibility / tests. */
int mdl_abmil_gate_dropout_mask(uint8_t* keep, int64_t T, int H, int which, float p_drop, uint64_t seed,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * A3 -- softmax over patches + weighted pooling.  Replaces F.softmax(A, dim=1) (abmil.py:55) and
 * `(embeddings * attention).sum(dim=1)` (Model.py:416-417) without materialising E*attention.
 *
 *   pooled[b,c,e] = sum_t softmax_t(scores[b,:,c])[t] * E[b,t,c,e]
 *
 * Bags: dense (cu_seqlens == NULL: bag b = tokens [b*N, (b+1)*N)) or ragged (cu_seqlens int64
 * [n_bags+1] device array of token offsets into the packed E / scores; max_len = longest bag).
 * An empty bag pools to 0.
 * E [T,H*512] (stride ldE >= H*512, % 4 == 0 for fp32 and bf16 E alike, no upper limit: the pooling kernels form 64-bit row addresses;
 * the backward's dE shares ldE with E), scores [T,H], pooled [n_bags,H*512],
 * stat_m, stat_l [n_bags,H]: softmax max / sum-of-exp per bag and head (saved for backward).
 * ws: mdl_abmil_pool_ws_bytes(n_bags,max_len,H).
 */
int64_t mdl_abmil_pool_ws_bytes(int64_t n_bags, int64_t max_len, int H);
int mdl_abmil_pool_fwd(const float* E, int64_t ldE, const float* scores, float* pooled, float* stat_m,
                       float* stat_l, int64_t n_bags, int64_t N, const int64_t* cu_seqlens,
                       int64_t max_len, int H, void* ws, void* stream);

/* Backward.  d_pooled [n_bags,H*512].  Outputs: dE [T,H*512] (stride ldE; written or accumulated as
 * above) and d_scores [T,H] (gradient wrt the RAW scores through the softmax; written, or added to
 * existing contents when accumulate_scores != 0 -- used when raw attention also feeds a loss). */
int mdl_abmil_pool_bwd(const float* E, int64_t ldE, const float* scores, const float* pooled,
                       const float* stat_m, const float* stat_l, const float* d_pooled, float* dE,
                       int accumulate, float* d_scores, int accumulate_scores, int64_t n_bags, int64_t N,
                       const int64_t* cu_seqlens, int64_t max_len, int H, void* stream);

/* Weighted pooling WITHOUT the softmax: pooled[b,c,:] = sum_t weights[t,c] E[t,c,:] -- the 'relu' / 'leaky_relu' / 'sigmoid'
 * attention activations of BatchedABMIL (madeleine/models/abmil.py:56-61) pooled as Model.py:416-417 does.  weights [T,H] are the
 * ACTIVATED scores (the elementwise activation and its derivative stay with the caller); same geometry arguments and workspace
 * as mdl_abmil_pool_fwd; scratch_m / scratch_l [n_bags,H] are overwritten.  Backward: dE[t,c,:] (+)= weights[t,c] d_pooled[b,c,:],
 * d_weights[t,c] = <E[t,c,:], d_pooled[b,c,:]>. */
int mdl_abmil_wpool_fwd(const float* E, int64_t ldE, const float* weights, float* pooled, float* scratch_m, float* scratch_l,
                        int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H, void* ws, void* stream);
int mdl_abmil_wpool_bwd(const float* E, int64_t ldE, const float* weights, const float* d_pooled, float* dE, int accumulate,
                        float* d_weights, int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H, void* stream);
int mdl_abmil_wpool_fwd_bf16(const uint16_t* E, int64_t ldE, const float* weights, float* pooled, float* scratch_m, float* scratch_l,
                             int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H, void* ws, void* stream);
int mdl_abmil_wpool_bwd_bf16(const uint16_t* E, int64_t ldE, const float* weights, const float* d_pooled, uint16_t* dE, int accumulate,
                             float* d_weights, int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H,
                             void* stream);

/* Views: the intra-modality path pools two random half-bags per bag with the raw scores
 * re-softmaxed over the subset (Model.py:419-440).  A view is a DENSE bag of N tokens restricted to the index list
 * token_idx int32 [n_idx] (the same list for every bag: logical token i of bag b is row b*N + token_idx[i]); the kernels
 * gather the 8-KiB token rows in place -- no index_select copies of E.  ws: mdl_abmil_pool_ws_bytes(n_bags, n_idx, H).
 * The backward ACCUMULATES into dE (rows of the view) and/or d_scores; either may be NULL: d_scores == NULL is a dE-only pass
 * that does not read E (dE[t,c,:] += w[t,c] d_pooled[b,c,:]). */
int mdl_abmil_pool_view_fwd(const float* E, int64_t ldE, const float* scores, float* pooled, float* stat_m, float* stat_l,
                            int64_t n_bags, int64_t N, const int32_t* token_idx, int64_t n_idx, int H, void* ws, void* stream);
int mdl_abmil_pool_view_bwd(const float* E, int64_t ldE, const float* scores, const float* pooled, const float* stat_m,
                            const float* stat_l, const float* d_pooled, float* dE, float* d_scores, int64_t n_bags, int64_t N,
                            const int32_t* token_idx, int64_t n_idx, int H, void* stream);

/* Ragged views (ABI 26): the same two half-bag views on PACKED bags of unequal length (MADELEINE.forward_ragged with n_views = 3).
 * perm int32 [T]: absolute rows of the packed E / scores, each bag's rows shuffled within its own range; vcu int64 [2*n_bags + 1]:
 * prefix over positions in perm -- segment s = 2*b + v (view v in {0, 1} of bag b) is the rows perm[vcu[s] .. vcu[s+1]).  With the
 * reference's per-bag draw (idx = shuffle(arange(N_b)), mid = N_b // 2) view 0 is idx[:mid], view 1 idx[mid:].  pooled [2*n_bags, H*512]
 * and stat_m, stat_l [2*n_bags, H] are in segment order.  An empty segment (a 1-token bag's first view) pools to exact zeros and gets
 * zero gradients.  max_view_len >= every segment's length (it sizes the grid); ws: mdl_abmil_pool_ws_bytes(2*n_bags, max_view_len, H).
 * Every perm entry must be a row of E (< T) and perm a permutation of the rows it covers.  Bags of any length >= 1 take part (an absent
 * stain's 2-token zero bag included: the caller decides which outputs a loss reads).  Backward: as mdl_abmil_pool_view_bwd, it
 * ACCUMULATES into dE and / or d_scores (either may be NULL; d_scores == NULL does not read E); the segments write disjoint rows. */
int mdl_abmil_pool_rview_fwd(const float* E, int64_t ldE, const float* scores, float* pooled, float* stat_m, float* stat_l,
                             int64_t n_bags, const int32_t* perm, const int64_t* vcu, int64_t max_view_len, int H, void* ws, void* stream);
int mdl_abmil_pool_rview_bwd(const float* E, int64_t ldE, const float* scores, const float* pooled, const float* stat_m,
                             const float* stat_l, const float* d_pooled, float* dE, float* d_scores, int64_t n_bags, const int32_t* perm,
                             const int64_t* vcu, int64_t max_view_len, int H, void* stream);
int mdl_abmil_pool_rview_fwd_bf16(const uint16_t* E, int64_t ldE, const float* scores, float* pooled, float* stat_m, float* stat_l,
                                  int64_t n_bags, const int32_t* perm, const int64_t* vcu, int64_t max_view_len, int H, void* ws,
                                  void* stream);
int mdl_abmil_pool_rview_bwd_bf16(const uint16_t* E, int64_t ldE, const float* scores, const float* pooled, const float* stat_m,
                                  const float* stat_l, const float* d_pooled, uint16_t* dE, float* d_scores, int64_t n_bags,
                                  const int32_t* perm, const int64_t* vcu, int64_t max_view_len, int H, void* stream);

/* Fused backward of A2 + A3 ("abmil_attnpool_bwd").  Call sequence:
 *   1. mdl_abmil_pool_bwd(..., dE = NULL, ...)   -> d_scores only (one read of E; dE may be NULL in that call)
 *   2. mdl_abmil_attnpool_bwd(...)               -> dE, dWa, dWb, dba, dbb, dwc, dbc
 * Step 2 = mdl_abmil_gate_bwd whose dX epilogue adds the pooling term  w[t,c] * d_pooled[bag(t), c, :]
 * (w = exp(scores - stat_m) / stat_l) while writing dE once -- instead of the pooling backward writing dE and the gate
 * backward reading it back to accumulate (saves one write + one read of |E|).  row_bag int32 [T] gives the bag of
 * every token row (ragged bags); row_bag == NULL means dense bags of N tokens (bag = t / N).  ws as mdl_abmil_gate_bwd.
 * accumulate != 0: dE already holds another consumer's gradient of E (the token_projector's dX, Model.py:140) and the epilogue
 * adds to it -- the read-modify-write rides under the MFMA-bound contraction instead of a separate 3 x |E| add pass. */
int mdl_abmil_attnpool_bwd(const float* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc,
                           const float* act_a, const float* act_b, const float* d_scores, float* dE, int accumulate,
                           float* dWa, float* dWb, float* dba, float* dbb, float* dwc, float* dbc, int64_t T, int H, float p_drop,
                           uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b, const float* scores,
                           const float* stat_m, const float* stat_l, const float* d_pooled, const int32_t* row_bag,
                           int64_t N, void* ws, void* stream);

/* Profiling form of mdl_abmil_attnpool_bwd: `phases` bit 0 = the HBM-bound dz pass (+ the bias / wc column-sum reduction), bit 1 = the
 * MFMA-bound dX / dW contractions (+ the dW slab reduction); 3 = what mdl_abmil_attnpool_bwd runs.  Calling it with 1 and then 2 on
 * the same arguments and workspace gives the same results and lets the caller time the two halves with its own events (bench.py's
 * roofline_mfma counts the contractions only). */
int mdl_abmil_attnpool_bwd_phases(const float* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc,
                                  const float* act_a, const float* act_b, const float* d_scores, float* dE, int accumulate,
                                  float* dWa, float* dWb, float* dba, float* dbb, float* dwc, float* dbc, int64_t T, int H,
                                  float p_drop, uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b,
                                  const float* scores, const float* stat_m, const float* stat_l, const float* d_pooled,
                                  const int32_t* row_bag, int64_t N, void* ws, void* stream, int phases);
int mdl_abmil_attnpool_bwd_phases_bf16(const uint16_t* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc,
                                       const uint16_t* act_a, const uint16_t* act_b, const float* d_scores, uint16_t* dE,
                                       int accumulate, float* dWa, float* dWb, float* dba, float* dbb, float* dwc, float* dbc,
                                       int64_t T, int H, float p_drop, uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b,
                                       const float* scores, const float* stat_m, const float* stat_l, const float* d_pooled,
                                       const int32_t* row_bag, int64_t N, void* ws, void* stream, int phases);

/* ------------------------------------------------------------------------------------------------
 * N1 -- fused LayerNorm -> GELU(erf) -> Dropout of the pre-attention MLP.  Replaces the
 * nn.LayerNorm / nn.GELU / nn.Dropout(0.1) triple that follows each Linear (madeleine/models/Model.py:352-354,
 * :356-358, :360-362) and its autograd, in one HBM pass each way.
 * x, y, dy, dx [rows, W] contiguous; W in {256, 512, 2048}; gamma, beta [W]; mean, rstd [rows] (saved for
 * backward); LayerNorm: biased variance, rstd = 1/sqrt(var + eps).  Dropout as in the gate kernels: keep (uint8
 * [rows,W]) injects a mask, else a counter hash of (seed, element index) -- regenerated in backward.
 * dgamma, dbeta [W] are overwritten.  ws: mdl_ln_gelu_drop_bwd_ws_bytes(rows, W).
 * bias [W] (may be NULL): the bias of the preceding Linear, added to x before the LayerNorm (y = f(x + bias)) so the
 * GEMM runs bias-free; dbias [W] (may be NULL) receives its gradient = the column sums of dx, saving the separate
 * reduction pass over dx that autograd's Linear backward would launch.
 */
int mdl_ln_gelu_drop_fwd(const float* x, const float* bias, const float* gamma, const float* beta, float* y,
                         float* mean, float* rstd, int64_t rows, int W, float eps, float p_drop, uint64_t seed,
                         const uint8_t* keep, void* stream);
int64_t mdl_ln_gelu_drop_bwd_ws_bytes(int64_t rows, int W);
int mdl_ln_gelu_drop_bwd(const float* x, const float* bias, const float* gamma, const float* beta, const float* mean,
                         const float* rstd, const float* dy, float* dx, float* dgamma, float* dbeta, float* dbias,
                         int64_t rows, int W, float p_drop, uint64_t seed, const uint8_t* keep, void* ws,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * L1 -- InfoNCE with in-batch negatives.  Replaces InfoNCE.info_nce, negative_keys=None branch
 * (madeleine/utils/loss.py:92,111-127) for S independent problems in one launch (the reference
 * calls it once per stain from trainer.py:33).
 *
 * Q,P [S,Kmax,D] padded row blocks (problem s uses rows [0,cnt[s])); cnt int32 [S] device array.  D >= 8 and a multiple of 32
 *          (MDL_E_ARG otherwise, from the workspace query too): a narrower embedding is passed with zero columns behind it, which change
 *          neither the norms nor the products.
 * loss [S]: mean-reduced cross entropy of Q_hat P_hat^T / temperature against the diagonal
 *           (symmetric != 0: 0.5*rows + 0.5*columns, loss.py:120-123).  cnt[s] == 0 => loss 0.
 * ws: mdl_infonce_ws_bytes(S,Kmax,D): normalised rows, inverse norms, logits, LSEs (kept for bwd).
 */
int64_t mdl_infonce_ws_bytes(int S, int Kmax, int D);
/* row_loss (NULL, or [S,Kmax]): the per-sample losses of reduction='none' (loss.py:58 -> F.cross_entropy(..., reduction); symmetric:
 * 0.5 CE_i + 0.5 CE'_i); rows >= cnt[s] are zeroed. */
int mdl_infonce_fwd(const float* Q, const float* P, const int32_t* cnt, float* loss, float* row_loss, int S, int Kmax,
                    int D, float temperature, int symmetric, void* ws, void* stream);
/* Q,P: the forward's inputs (the fused path keeps no normalised copies).  d_loss [S] incoming gradient of the mean losses -- or, when
 * d_row_loss [S,Kmax] != NULL, the gradients of the per-sample losses (d_loss is then ignored and may be NULL); dQ,dP [S,Kmax,D] (rows
 * >= cnt[s] are zeroed).  ws must be the forward's.
 * Default: staged launches (normalise | similarity | log-sum-exp | loss ; coefficients | products | normalize backward), all stains per
 * launch.  Switch MDL_SW_INFONCE_FUSED ("Behaviour switches" below; the same value for a forward and its backward) with Kmax <= 256
 * and D <= 512: ONE launch forward and ONE backward producing the same bits
 * (measured slower on MI355X: the problem is latency-bound and fusing gives up wave-level parallelism; csrc/infonce.hip). */
int mdl_infonce_bwd(const float* Q, const float* P, const float* d_loss, const float* d_row_loss, const int32_t* cnt, float* dQ,
                    float* dP, int S, int Kmax, int D, float temperature, int symmetric, void* ws, void* stream);

/* L1 with explicit negatives (ABI 26, additive).  Replaces InfoNCE.info_nce, negative_keys branch (madeleine/utils/loss.py:93-110):
 * logits [q_hat.p_hat | q_hat.n_hat^T] / temperature with the target in column 0.  The reference branch builds them and then returns
 * None; the loss computed here is the cross entropy its in-batch branch applies to such logits,
 * F.cross_entropy(logits / temperature, labels, reduction) (loss.py:125).  x_hat = x / max(|x|, 1e-12) for every row.  `symmetric`
 * plays no part (the reference branch never reads it).
 *
 * Q,P [N,Dq] with Dq = D rounded up to 32, zero-padded columns (16-byte aligned); Neg [M,D] (paired == 0: one bank for every row) or
 * [N,M,D] (paired != 0: row i against Neg[i]), contiguous, any D >= 1 (read in place; NULL only when M == 0).
 * loss (NULL, or [1]): mean of the N row losses (N == 0 => 0); row_loss (NULL, or [N]): per-row losses (reduction='none').  At least
 * one of the two.  M == 0 gives loss 0 and zero gradients (a one-class cross entropy).
 * ws: mdl_infonce_neg_ws_bytes(N,M,D,paired): normalised Q,P, logits, norms, LSE partials, split partials (kept for bwd).
 * Returns MDL_E_UNSUPPORTED past the launch-grid limits (unpaired: N or Dq above 2,097,120, M above 67,107,840; paired: M above
 * 4,194,240). */
int64_t mdl_infonce_neg_ws_bytes(int N, int M, int D, int paired);
int mdl_infonce_neg_fwd(const float* Q, const float* P, const float* Neg, float* loss, float* row_loss, int N, int M, int D, int paired,
                        float temperature, void* ws, void* stream);
/* d_loss [1] incoming gradient of the mean -- or, when d_row_loss [N] != NULL, of the row losses (d_loss may then be NULL).
 * dQ,dP [N,Dq] (padding columns get the gradient of their zeros, 0 up to rounding); dNeg (NULL: skipped entirely, no kernel touches it)
 * same shape as Neg.  ws must be the forward's.  No atomics: splits over M are merged in a fixed order (same bits run to run). */
int mdl_infonce_neg_bwd(const float* Neg, const float* d_loss, const float* d_row_loss, float* dQ, float* dP, float* dNeg, int N, int M,
                        int D, int paired, float temperature, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N1 -- every Linear of the encoder as an exact-fp32 contraction in hand-written kernels: the three
 * Linears of the pre-attention MLP (madeleine/models/Model.py:351, :355, :359; bias = NULL there: the bias and its gradient
 * are handled by mdl_ln_gelu_drop_*), the token_projector Linear(2048, 128) (Model.py:140) and the slide projector
 * Linear(2048, 512) on the pooled embeddings (Model.py:145).
 * X [T,K] (row stride ldx), W [N,K] contiguous (torch's Linear.weight), bias [N] or NULL, Y [T,N] (row stride ldy); the backward's dY
 * has row stride ldy, dX row stride lddx.  Strides % 4 == 0.  Upper limits (for every T):
 *   mdl_linear_fwd: R * 4 ldx + 48 <= 2^31 - 1 with R = 127 (N % 256 == 0) or 255 (the tall tile); 3 * 4 ldy + 1020 <= 2^31 - 1
 *   mdl_linear_bwd: 127 * 4 ldy + 48 and 15 * 4 ldy + 4 N <= 2^31 - 1; 15 * 4 ldx + 4 K <= 2^31 - 1; 3 * 4 lddx + 1020 <= 2^31 - 1
 * Supported (MDL_E_UNSUPPORTED otherwise):
 *   T > 256 : N % 256 == 0 with K % 32 == 0 -- matrix-core tile engine, 128 x 256 tile; dX (output width K) runs the
 *             ragged-column variant of the tile when K % 256 != 0 (config 5: K = 768 + 32 stain channels);
 *             N % 256 == 128 with K % 256 == 0 -- the 256 x 128 "tall" geometry (token_projector);
 *   T <= 256: K % 4 == 0, N % 4 == 0 -- LDS-tiled fp32 FMA kernel (the slide projector's 64 rows).
 *   mdl_linear_fwd : Y = X W^T (+ bias)
 *   mdl_linear_bwd : dW [N,K] = dY^T X  (always);  dX [T,K] = dY W  when dX != NULL;  dbias [N] = column sums of dY when != NULL
 */
int64_t mdl_linear_fwd_ws_bytes(int64_t T, int N, int K);
int mdl_linear_fwd(const float* X, int64_t ldx, const float* W, const float* bias, float* Y, int64_t ldy, int64_t T, int N, int K,
                   void* ws, void* stream);
int64_t mdl_linear_bwd_ws_bytes(int64_t T, int N, int K);
int mdl_linear_bwd(const float* X, int64_t ldx, const float* W, const float* dY, int64_t ldy, float* dX, int64_t lddx,
                   float* dW, float* dbias, int64_t T, int N, int K, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * G0-G3 -- Graph Optimal Transport.  Replaces GOT (madeleine/utils/loss.py:278-302) =
 * cost_matrix_batch_torch (:162-176) + global-threshold ReLU (:288-292) + IPOT Wasserstein
 * (:179-207, 30 iterations, beta .5) + Gromov-Wasserstein (:236-275, 5 x 20 IPOT iterations,
 * beta .1) with cos_batch_torch intra costs (:210-233).  Called from trainer.py:42-45.
 *
 * V,Q [k,n,d]: the (already sub-sampled, loss.py:281-284) token sets of k cases; n <= 512, d <= 128
 * (n <= 256 -- what trainer.py:44 produces -- keeps the transport plans in registers / one matrix-core panel; 256 < n <= 512 keeps
 * them in the workspace and walks 256 x 256 output blocks).
 * out [2]: out[0] = sum_b WD_b, out[1] = sum_b GWD_b   (GOT returns out[1] + out[0], a SUM over cases).
 * Thresholds thr = min + .1 (max - min): the reference takes min/max over the WHOLE batch tensor for each of
 * the three cost tensors (cross, intra-V, intra-Q).  minmax_out float[6] (may be NULL) receives this call's
 * extrema (cross min,max | Cs min,max | Ct min,max).  When minmax_in (float[6], device) is non-NULL those
 * values are used INSTEAD -- the data-parallel driver all-gathers per-rank extrema so that every rank
 * thresholds with the global-batch values nn.DataParallel would see.
 * ws: mdl_got_ws_bytes(k,n,d) bytes: cost matrices + the per-iteration plans T_t and scaling vectors that
 * the reverse sweep replays (the same tensors the reference's autograd tape holds).  The backward calls
 * must receive the forward's workspace untouched.
 * ABI 23: for 128 < n <= 256 and 2 * (cases of the launch) <= compute units of the device, every IPOT sweep runs as TWO workgroups per
 * case and branch (row halves) that exchange their column sums once per iteration through 8-byte {value, tag} granules in the workspace
 * (device-scope stores / polls; csrc/got_resident.hip, Xch); the switch MDL_SW_GOT_NOSPLIT ("Behaviour switches" below; one value for all
 * stages of a call) keeps the one-workgroup sweeps.  Same results up to the
 * association of the column sums; bit-reproducible.  The workspace's global region ends with four floats {pass generation (uint32 bits),
 * exchange time-out flag (0 = none; non-zero voids the pass), 0, 0}, followed by the 64 bytes of padding mdl_got_ws_bytes adds.
 * A voided pass says so in its results: out[0..1] of the forward and dV / dQ of the backward are NaN when the flag is up (a sweep waited
 * ~1 s for a partner workgroup that never became resident -- the device was shared with work the launch did not know about, e.g. a
 * second training process; run those with MDL_SW_GOT_NOSPLIT set).  The flag is cleared by the extrema kernel of every forward.
 *
 * Return codes of every launching mdl_got_* function below (the four families: mdl_got_*, mdl_got_*_multi, mdl_got_tiled_*,
 * mdl_got_tiled_rect_*), in one order, each step over all problems of a call before the next step:
 *   1. MDL_E_ARG: np outside [1, MDL_GOT_MAX_BATCH] or a NULL array of a _multi form; k, n or m < 0, d < 1; an empty problem (k or n = 0)
 *      of a _multi form.
 *   2. MDL_E_UNSUPPORTED: a size beyond the class (n <= 512, d <= 128; a _multi problem n <= 256; tiled n, m, d <= 4096).
 *   3. MDL_E_ARG: ws NULL; out (_fwd), minmax_out (_extrema), d_out (_bwd_begin, _bwd) NULL; _extrema of an empty problem; V, Q (_fwd,
 *      _extrema, _bwd_finish, _bwd) or dV, dQ (_bwd_finish, _bwd) NULL while the tensor has elements -- a tensor of k n d = 0 elements
 *      (Q, dQ: k m d = 0) may be NULL.
 *   4. MDL_E_ALIGN: ws is not 16-byte aligned.
 *   5. An empty problem (k, n or m = 0) is MDL_OK and launches nothing: out = (0, 0), d_minmax = 0 where it is given, dV and dQ cleared
 *      where they have elements.
 * The combined _bwd functions are refused on a fault of either stage before the first stage is launched.  The *_ws_bytes queries answer
 * steps 1 and 2 for their sizes.
 */
int64_t mdl_got_ws_bytes(int k, int n, int d);
int mdl_got_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in,
                int k, int n, int d, void* ws, void* stream);
/* Only the first stage of the forward (normalise, raw costs, extrema): minmax_out [6] for this batch.  The
 * data-parallel driver calls it on every rank, reduces min/max over ranks, then runs mdl_got_fwd with minmax_in. */
int mdl_got_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int d, void* ws, void* stream);
/* Backward: d_out [2] = incoming gradients of (WD sum, GWD sum); dV,dQ [k,n,d] are written.  Gradient flows
 * through every unrolled IPOT iteration, the GW outer loop, the ReLU masks and the threshold extrema (to the
 * arg-min / arg-max elements, split evenly over ties like torch's min()/max() backward). */
int mdl_got_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int d,
                void* ws, void* stream);
/* The same in two steps, for the data-parallel path: _begin runs the reverse sweeps and reports the gradient
 * wrt the six threshold extrema in d_minmax [6] (may be NULL); the caller sums it over ranks; _finish routes
 * d_minmax_total [6] (NULL = this call's own) to the local elements that attain the extrema and writes dV,dQ. */
int mdl_got_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int d, void* ws, void* stream);
int mdl_got_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total,
                       int k, int n, int d, void* ws, void* stream);
/* Several GOT problems in ONE launch sequence (round 4).  The reference calls GOT once per stain (trainer.py:40-49); a data-parallel
 * rank used to run the stains' chains on one HIP stream each, and a process has four hardware queues: the first stream that is not
 * ours (a prefetcher's, RCCL's) made two chains share a queue and run one after the other.  Here every launch covers all problems
 * (a workgroup finds its problem from blockIdx), on the caller's stream alone.  1 <= np <= MDL_GOT_MAX_BATCH, every problem
 * non-empty (k >= 1, n >= 1) with n <= 256 (MDL_E_UNSUPPORTED above), one d for all; arrays of np entries: V[p], Q[p] [k[p], n[p], d],
 * ws[p] = mdl_got_ws_bytes(k[p], n[p], d) kept from _fwd_multi to _bwd_finish_multi, out[p] [2], minmax / d_minmax entries [6].
 * The kernels of the largest problem's size class run every problem: results of a problem equal its single-problem call bit for
 * bit when it is in that class itself, and to fp32 rounding otherwise (another reduction order). */
#define MDL_GOT_MAX_BATCH 4
int mdl_got_extrema_multi(int np, const float* const* V, const float* const* Q, float* const* minmax_out, const int* k, const int* n,
                          int d, void* const* ws, void* stream);
int mdl_got_fwd_multi(int np, const float* const* V, const float* const* Q, float* const* out, const float* const* minmax_in,
                      const int* k, const int* n, int d, void* const* ws, void* stream);
int mdl_got_bwd_begin_multi(int np, const float* const* d_out, float* const* d_minmax, const int* k, const int* n, int d,
                            void* const* ws, void* stream);
int mdl_got_bwd_finish_multi(int np, const float* const* V, const float* const* Q, float* const* dV, float* const* dQ,
                             const float* const* d_minmax_total, const int* k, const int* n, int d, void* const* ws, void* stream);

/* Tiled class of GOT: the same arguments, return codes (the order above), semantics and workspace contract as the six mdl_got_* entry
 * points above, for 1 <= n <= 4096 and 1 <= d <= 4096 at any k.  The shapes
 * of the resident classes are included, so the two can be compared.  Many workgroups share one case and meet only at kernel
 * boundaries (csrc/got_tiled.hip): the IPOT sweeps run as panels of 16 rows per workgroup with the column sums of an iteration merged
 * by the next launch (two launches per iteration), the products on 128 x 128 matrix-core tiles.  Deterministic (fixed-order merges, no
 * atomics).  The workspace holds the same tape as the resident classes, ~151 n^2 floats per case (0.6 GB at n = 1024, 10 GB at
 * n = 4096). */
int64_t mdl_got_tiled_ws_bytes(int k, int n, int d);
int mdl_got_tiled_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in,
                      int k, int n, int d, void* ws, void* stream);
int mdl_got_tiled_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int d, void* ws, void* stream);
int mdl_got_tiled_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int d, void* ws, void* stream);
int mdl_got_tiled_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total,
                             int k, int n, int d, void* ws, void* stream);
int mdl_got_tiled_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int d,
                      void* ws, void* stream);
/* The tiled class between token sets of different sizes: V [k, n, d], Q and dQ [k, m, d], sizes in the order (k, n, m, d), everything
 * else as in the six functions above, which are the m = n case of these (same code, same bits).  1 <= n, m <= 4096 and 1 <= d <= 4096
 * (MDL_E_UNSUPPORTED beyond, for each of them); k = 0, n = 0 or m = 0 gives zero outputs and zero gradients (dV and dQ are cleared).
 * The cross cost and every transport plan are n x m, the intra costs n x n and m x m; IPOT uses sigma_0 = 1/m,
 * delta_i = 1 / (n sum_j Q_ij sigma_j), sigma_j = 1 / (m sum_i Q_ij delta_i); Gromov-Wasserstein gamma_0 = 1/(n m), p = 1/n, q = 1/m.
 * GOT(V, Q) != GOT(Q, V).  The sweeps' row panels run over n: a shape with n << m uses few workgroups per case.  Workspace per case:
 * ~144 n up4(m) floats (the tape and the n x m intermediates) + 3 n up4(n) + 4 m up4(m) (1.5 GB at n = 4096, m = 512 against 10 GB at
 * n = m = 4096). */
int64_t mdl_got_tiled_rect_ws_bytes(int k, int n, int m, int d);
int mdl_got_tiled_rect_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in,
                           int k, int n, int m, int d, void* ws, void* stream);
int mdl_got_tiled_rect_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int m, int d, void* ws, void* stream);
int mdl_got_tiled_rect_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int m, int d, void* ws, void* stream);
int mdl_got_tiled_rect_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total,
                                  int k, int n, int m, int d, void* ws, void* stream);
int mdl_got_tiled_rect_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int m, int d,
                           void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 mode -- the reference's `precision: bfloat16` runs (torch autocast around the forward,
 * madeleine/utils/trainer.py:101-103, scripts/launch_pretrain_withStainEncodings.sh): activations are STORED in
 * bf16 (uint16_t bit patterns of torch.bfloat16: E, the gate activations, dE, the LayerNorm input/output), the
 * contractions run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, every epilogue / reduction / statistic is
 * fp32, parameters and their gradients stay fp32.  Same argument meaning as the fp32 entry points above; ldE counts
 * bf16 elements and must be a multiple of 8 on the gate entry points (16-byte LDS-DMA granules) and of 4 on the pooling entry points
 * (mdl_abmil_pool_*_bf16, _wpool_, _pool_view_, _pool_rview_: 8-byte loads), MDL_E_ARG otherwise.  Upper limits:
 * mdl_abmil_gate_fwd_bf16 255 * 2 ldE + 112 <= 2^31 - 1; mdl_abmil_gate_bwd_bf16 / mdl_abmil_attnpool_bwd(_phases)_bf16
 * 63 * 2 ldE + 496 <= 2^31 - 1 (dE shares ldE with E; any ldE >= H*512 within these rules: the backward reads E in place).
 * The fp32 entry points remain the parity path (1e-3 rel of the reference's fp32 results); this mode is held to
 * the reference-under-autocast accuracy (tests/test_bf16_gpu.py).
 */
int mdl_ln_gelu_drop_fwd_bf16(const uint16_t* x, const float* bias, const float* gamma, const float* beta, uint16_t* y,
                              float* mean, float* rstd, int64_t rows, int W, float eps, float p_drop, uint64_t seed,
                              const uint8_t* keep, void* stream);
int mdl_ln_gelu_drop_bwd_bf16(const uint16_t* x, const float* bias, const float* gamma, const float* beta, const float* mean,
                              const float* rstd, const uint16_t* dy, uint16_t* dx, float* dgamma, float* dbeta, float* dbias,
                              int64_t rows, int W, float p_drop, uint64_t seed, const uint8_t* keep, void* ws, void* stream);
/* Grouped LayerNorm-GELU-Dropout (ABI 24) for the engines whose GEMM epilogue adds no bias (exact fp32: no suffix; bf16): rows
 * [cu_groups[g], cu_groups[g + 1]) of group g (int64 [G + 1] on the device, G <= 2048, rows of a group contiguous) take the bias row
 * group_bias[g][W] -- the preceding Linear's bias + the bag's stain-encoding row times the encoding columns of the first weight
 * (Model.py:125-132, :351: [x | e_g] W^T = x Wx^T + e_g We^T), so the [T, D + 32] concatenation never exists.  The backward returns
 * dgroup_bias [G][W] = per-group column sums of dx (merged in a fixed order).  W in {256, 512, 1024}.
 * ws of the backward: mdl_ln_gelu_drop_bwd_groups_ws_bytes(rows, W, G). */
int mdl_ln_gelu_drop_fwd_groups(const float* x, const float* group_bias, const float* gamma, const float* beta, float* y, float* mean,
                                float* rstd, int64_t rows, int W, float eps, float p_drop, uint64_t seed, const uint8_t* keep,
                                const int64_t* cu_groups, int G, void* stream);
int mdl_ln_gelu_drop_fwd_groups_bf16(const uint16_t* x, const float* group_bias, const float* gamma, const float* beta, uint16_t* y,
                                     float* mean, float* rstd, int64_t rows, int W, float eps, float p_drop, uint64_t seed,
                                     const uint8_t* keep, const int64_t* cu_groups, int G, void* stream);
int mdl_ln_gelu_drop_bwd_groups(const float* x, const float* group_bias, const float* gamma, const float* beta, const float* mean,
                                const float* rstd, const float* dy, float* dx, float* dgamma, float* dbeta, float* dgroup_bias,
                                int64_t rows, int W, float p_drop, uint64_t seed, const uint8_t* keep, const int64_t* cu_groups, int G,
                                void* ws, void* stream);
int mdl_ln_gelu_drop_bwd_groups_bf16(const uint16_t* x, const float* group_bias, const float* gamma, const float* beta,
                                     const float* mean, const float* rstd, const uint16_t* dy, uint16_t* dx, float* dgamma,
                                     float* dbeta, float* dgroup_bias, int64_t rows, int W, float p_drop, uint64_t seed,
                                     const uint8_t* keep, const int64_t* cu_groups, int G, void* ws, void* stream);
int mdl_abmil_pool_fwd_bf16(const uint16_t* E, int64_t ldE, const float* scores, float* pooled, float* stat_m,
                            float* stat_l, int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H,
                            void* ws, void* stream);
int mdl_abmil_pool_bwd_bf16(const uint16_t* E, int64_t ldE, const float* scores, const float* pooled, const float* stat_m,
                            const float* stat_l, const float* d_pooled, uint16_t* dE, int accumulate, float* d_scores,
                            int accumulate_scores, int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len,
                            int H, void* stream);
int mdl_abmil_pool_view_fwd_bf16(const uint16_t* E, int64_t ldE, const float* scores, float* pooled, float* stat_m, float* stat_l,
                                 int64_t n_bags, int64_t N, const int32_t* token_idx, int64_t n_idx, int H, void* ws, void* stream);
int mdl_abmil_pool_view_bwd_bf16(const uint16_t* E, int64_t ldE, const float* scores, const float* pooled, const float* stat_m,
                                 const float* stat_l, const float* d_pooled, uint16_t* dE, float* d_scores, int64_t n_bags,
                                 int64_t N, const int32_t* token_idx, int64_t n_idx, int H, void* stream);
/* N1 Linears in the bf16 mode (madeleine/models/Model.py:351, :355, :359 pre-attention MLP, :140 token_projector under
 * `precision: bfloat16`, trainer.py:101-103): X, Y, dY, dX bf16; W [N,K], bias [N], dW, dbias fp32.  v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation; dW through the ds_read_b64_tr_b16 "TN" engine (no transposed copies of X / dY).
 * Supported (mdl_linear_bf16_supported; MDL_E_UNSUPPORTED otherwise): N % 128 == 0 and K % 32 == 0 (forward and
 * backward).  Leading dimensions multiples of 8 (MDL_E_UNSUPPORTED otherwise).  Same argument meaning as mdl_linear_fwd / mdl_linear_bwd.
 * Upper limits: mdl_linear_fwd_bf16 255 * 2 ldx + 112 <= 2^31 - 1, 7 * 2 ldy + 510 <= 2^31 - 1; mdl_linear_bwd_bf16
 * 255 * 2 lddy + 112 <= 2^31 - 1, 63 * 2 ldx + 496 <= 2^31 - 1, 7 * 2 lddx + 510 <= 2^31 - 1. */
int mdl_linear_bf16_supported(int64_t N, int64_t K, int backward);
int64_t mdl_linear_fwd_bf16_ws_bytes(int64_t T, int64_t N, int64_t K);
int mdl_linear_fwd_bf16(const uint16_t* X, int64_t ldx, const float* W, const float* bias, uint16_t* Y, int64_t ldy, int64_t T,
                        int64_t N, int64_t K, void* ws, void* stream);
int64_t mdl_linear_bwd_bf16_ws_bytes(int64_t T, int64_t N, int64_t K);
int mdl_linear_bwd_bf16(const uint16_t* X, int64_t ldx, const float* W, const uint16_t* dY, int64_t lddy, uint16_t* dX, int64_t lddx,
                        float* dW, float* dbias, int64_t T, int64_t N, int64_t K, void* ws, void* stream);

int64_t mdl_abmil_gate_fwd_bf16_ws_bytes(int64_t T, int H);
int mdl_abmil_gate_fwd_bf16(const uint16_t* E, int64_t ldE, const float* Wa, const float* ba, const float* Wb,
                            const float* bb, const float* wc, const float* bc, float* scores, uint16_t* act_a,
                            uint16_t* act_b, int64_t T, int H, float p_drop, uint64_t seed, const uint8_t* keep_a,
                            const uint8_t* keep_b, void* ws, void* stream);
int64_t mdl_abmil_gate_bwd_bf16_ws_bytes(int64_t T, int H);
int mdl_abmil_gate_bwd_bf16(const uint16_t* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc,
                            const uint16_t* act_a, const uint16_t* act_b, const float* d_scores, uint16_t* dE,
                            int accumulate, float* dWa, float* dWb, float* dba, float* dbb, float* dwc, float* dbc,
                            int64_t T, int H, float p_drop, uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b,
                            void* ws, void* stream);
int mdl_abmil_attnpool_bwd_bf16(const uint16_t* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc,
                                const uint16_t* act_a, const uint16_t* act_b, const float* d_scores, uint16_t* dE,
                                int accumulate, float* dWa, float* dWb, float* dba, float* dbb, float* dwc, float* dbc, int64_t T,
                                int H, float p_drop, uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b,
                                const float* scores, const float* stat_m, const float* stat_l, const float* d_pooled,
                                const int32_t* row_bag, int64_t N, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Split-fp16 contraction engine (round 3; csrc/split_engine.hpp): the fp32 contractions of the path -- nn.Linear of
 * madeleine/models/Model.py:351, :355, :359, :140 and the gate products of madeleine/models/abmil.py:49-52 -- with fp32-level accuracy
 * on v_mfma_f32_32x32x16_f16: every operand value as two fp16 planes hi + lo of (power-of-two scale) x value, every product as
 * ah bh + ah bl + al bh accumulated in fp32 (measured error below a plain fp32 fmaf chain, tools/micro/split_lab.hip).
 * SPLIT IMAGE of X [rows, K], K % 32 == 0: uint16 [rows][K / 32][2][32] -- the hi and the lo plane of every 32-column block side
 * by side (128 B = the bytes of the fp32 block); row stride rsb bytes (>= 4 K, % 16 == 0).  scale: device float[2] = {scale, absmax}.
 * Upper limits of an image's row stride where it is an OPERAND (none where mdl_split_image / _rows write it, nor on their ldx, nor on the
 * ldx of mdl_split_tile_absmax, nor on the e_rsb of mdl_abmil_pool_fwd_img / _dscores_img: 64-bit addresses): mdl_split_gemm_nt(_group_bias)
 * 256 a_rsb and 256 b_rsb <= 2^31 - 1 (512 a_rsb and 128 b_rsb on the narrow-output tile: N <= 128, M > 256, no row_gate / group_bias),
 * 4 ldc <= 2^31 - 1; mdl_split_gemm_tn 32 a_rsb, 32 b_rsb <= 2^31 - 1; mdl_abmil_gate_fwd_split 256 e_rsb <= 2^31 - 1;
 * mdl_abmil_attnpool_bwd_split 32 e_rsb <= 2^31 - 1 and 4 ldE <= 2^31 - 1.
 *   mdl_split_image   : image of a fp32 tensor (exact absmax -> scale with max |scale x| in [2^13, 2^14)), + pad_rows zero rows
 *   mdl_split_gemm_nt : C [M,N] (+)= sum_k A[m][k] B[n][k] (+ bias[n])   A, B images with K columns (rows m, n)
 *   mdl_split_gemm_tn : out [N][Mi] = sum_t B[t][n] A[t][m]              A, B images with T rows (contraction = rows); B must be
 *                       followed by >= 32 all-zero rows; ws = mdl_split_gemm_tn_ws_bytes (token-split slabs, reduced in fixed order)
 */
/* A3 on the image of E (the split GEMM mode keeps E as the image its LayerNorm kernel wrote, nothing else): mdl_abmil_pool_fwd with
 * E_img = split image [T][H*512] (row stride e_rsb bytes, scale e_scale[0]); mdl_abmil_pool_dscores_img = the score gradients of
 * mdl_abmil_pool_bwd (d_scores (+)= ...; the dE term is part of mdl_abmil_attnpool_bwd_split's dX epilogue). */
int mdl_abmil_pool_fwd_img(const void* E_img, int64_t e_rsb, const float* e_scale, const float* scores, float* pooled, float* stat_m,
                           float* stat_l, int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H, void* ws,
                           void* stream);
int mdl_abmil_pool_dscores_img(const void* E_img, int64_t e_rsb, const float* e_scale, const float* scores, const float* pooled,
                               const float* stat_m, const float* stat_l, const float* d_pooled, float* d_scores, int accumulate_scores,
                               int64_t n_bags, int64_t N, const int64_t* cu_seqlens, int64_t max_len, int H, void* stream);
/* Dispatch timer of the A3 forward (measurement only; bench.py's roofline.achieved).  mdl_pool_timer_arm(slot), 0 <= slot < 64 (negative:
 * disarm): the NEXT mdl_abmil_pool_fwd / _bf16 / _img call on this process launches its two kernels through hipExtLaunchKernel with
 * start / stop events on the caller's stream, i.e. the begin / end timestamps of the dispatches themselves (what rocprofv3
 * --kernel-trace reports) instead of the distance between two markers in a busy stream.  Nothing waits at launch;
 * mdl_pool_timer_read(slot, ms[3]) blocks until that slot's launches finished and returns {pool_partial, pool_combine, start of the
 * first to end of the second} in milliseconds (MDL_E_ARG for a slot that was never used).  Process-wide state, one training thread. */
int mdl_pool_timer_arm(int slot);
int mdl_pool_timer_read(int slot, float* ms);
/* A HIP stream restricted to a subset of the compute units (hipExtStreamCreateWithCUMask): mask = n_words x 32 bits, bit i = CU i may run
 * this stream's kernels.  For partitioning the chip between a matrix-core-bound and an HBM-bound chain that run concurrently (the dW
 * products of the backward beside the LayerNorm / dz passes).  *stream_out receives the hipStream_t; mdl_stream_destroy releases it. */
int mdl_stream_create_cu_mask(uint32_t n_words, const uint32_t* mask, void** stream_out);
int mdl_stream_destroy(void* stream);
int mdl_split_image(const float* X, int64_t ldx, int64_t rows, int K, void* img, int64_t rsb, int64_t pad_rows, float* scale,
                    void* stream);
/* ROW-SCALED image (round 4): row r of X is scaled by its own power of two s_r (max_k |s_r X[r][k]| in [2^13, 2^14); an all-zero
 * row has no scale: its image row is zero and row_inv = 0 -- do NOT divide by row_inv) -- for the tensor whose rows a CALLER controls, the patch features (Model.py:113, :351): with one common scale a patch 2^20 times
 * larger than the others would cost them their low bits (fp32 nn.Linear has no such coupling between rows).  row_inv (device
 * float[rows]) receives 1 / s_r (0 for an all-zero row: it contributes nothing to any product), scale = {1, max |X|}; scale may be NULL
 * (no bookkeeping launches: the image is ONE kernel -- the weights' images, built every forward; pass a constant {1, .} as its scale).  Consumers: mdl_split_gemm_nt(A = this image, a_row_mul = row_inv) -- the row
 * factor is undone in the epilogue, exactly; mdl_split_gemm_tn pairs it with a gradient image written with row_mul = row_inv
 * (mdl_ln_gelu_drop_bwd_split), so that the row factors cancel inside the contraction over rows. */
int mdl_split_image_rows(const float* X, int64_t ldx, int64_t rows, int K, void* img, int64_t rsb, int64_t pad_rows, float* row_inv,
                         float* scale, void* stream);
/* row_gate (device float[ceil(M / 256)], may be NULL; only with accumulate != 0 and bias == NULL): output tiles whose entry is 0 are
 * skipped -- mdl_split_tile_absmax(X, ...) fills it with the per-256-row maxima of |X| for A = image(X), and chunk_max (float
 * [ceil(rows / 32)], may be NULL) with the per-32-row maxima that mdl_split_gemm_tn's b_chunk_max takes. */
int mdl_split_tile_absmax(const float* X, int64_t ldx, int64_t rows, int K, float* gate, float* chunk_max, void* stream);
/* terms (round 4; 3 everywhere by default, anything but 2 / 3 is MDL_E_ARG): 3 = ah bh + ah bl + al bh, the fp32-class product.  2 = the
 * operand that is NOT a gradient enters with its hi plane only (11 significant bits): mdl_split_gemm_nt drops ah bl (B = the weight of
 * dX = dY W), mdl_split_gemm_tn drops al bh (A = the activations of dW = dY^T X), mdl_abmil_attnpool_bwd_split does both for the gate's
 * dX / dW -- 4 instead of 6 MFMA sets per 32-k block, results at ~2^-12 relative.  Only ever selected for BACKWARD products, by
 * madeleine_amd.functional.set_gradient_terms(2); the forward (every value the losses see) always runs with 3.
 * a_row_mul (device float[M], may be NULL): row m of the product is multiplied by a_row_mul[m] before bias / accumulation (the
 * 1 / s_r of a row-scaled A image, or the s_r that undoes a row_mul folded into a gradient image).  b_col_mul (device float[N], N % 4
 * == 0, may be NULL): the same per output column = per row of a row-scaled B image (a weight matrix W [N, K]: nn.Linear's rows). */
int mdl_split_gemm_nt(const void* A, int64_t a_rsb, const float* a_scale, const void* B, int64_t b_rsb, const float* b_scale, float* C,
                      int64_t ldc, int64_t M, int N, int K, const float* bias, int accumulate, float* absmax_out, const float* row_gate,
                      const float* a_row_mul, const float* b_col_mul, int terms, void* stream);
/* (round 5) The same product with a bias row per GROUP of output rows: C[m][:] += group_bias[row_group[m]][:]; group_bias [G][N]
 * contiguous fp32, row_group device int32 [M] with values in [0, G).  MADELEINE's stain encoding (Model.py:125-132) concatenates ONE
 * 32-vector per bag to every patch feature before the first Linear (:351): [x | e_g] W^T = x Wx^T + e_g We^T, so the concat never has to
 * exist -- the bag's row e_g We^T enters here, and mdl_ln_gelu_drop_bwd_split_groups returns its gradient. */
int mdl_split_gemm_nt_group_bias(const void* A, int64_t a_rsb, const float* a_scale, const void* B, int64_t b_rsb, const float* b_scale,
                                 float* C, int64_t ldc, int64_t M, int N, int K, const float* bias, const float* a_row_mul,
                                 const float* b_col_mul, const float* group_bias, const int32_t* row_group, int terms, void* stream);
int64_t mdl_split_gemm_tn_ws_bytes(int64_t T, int Mi, int N);
/* b_chunk_max (float [ceil(T / 32)], may be NULL): per-32-row maxima of |X| for B = image(X) (mdl_split_tile_absmax) -- chunks whose
 * entry is 0 are skipped (the token_projector's dW: the local loss reads the first <= 256 tokens of a bag, the rest of d_tok is zero). */
int mdl_split_gemm_tn(const void* A, int64_t a_rsb, const float* a_scale, int Mi, const void* B, int64_t b_rsb, const float* b_scale,
                      int N, float* out, int64_t T, const float* b_chunk_max, void* ws, int terms, void* stream);

/* N1 producers that write split images directly (csrc/preattn_act.hip): mdl_ln_gelu_drop_fwd / _bwd with the output tensor as an
 * image -- the pre-attention activations and their gradients are consumed by contractions only, so no fp32 copy is written (the
 * forward also writes y when y != NULL: E, which the pooling kernels read).  Scales from rigorous bounds (no pass over the data):
 *   forward  |y|  <= (max|gamma| sqrt(W-1) + max|beta|) / (1-p)
 *   backward |dx| <= rstd_max 1.13 max|gamma| max|dy| (2 + sqrt(W)) / (1-p);  dy_absmax = device float with max |dy| (from the producing
 *            kernel's epilogue) or NULL (one extra pass over dy).  The dx image is followed by 32 zero rows; ws as mdl_ln_gelu_drop_bwd. */
/* row_mul / rstd_max (forward, both may be NULL): rstd_max (device float) receives max_r rstd[r] * row_mul[r] (row_mul NULL: max rstd) --
 * handed to the backward it replaces that call's pass over rstd. */
int mdl_ln_gelu_drop_fwd_split(const float* x, const float* bias, const float* gamma, const float* beta, float* y, void* img, float* scale,
                               float* mean, float* rstd, int64_t rows, int W, float eps, float p_drop, uint64_t seed, const uint8_t* keep,
                               const float* row_mul, float* rstd_max, void* stream);
/* row_mul (device float[rows], may be NULL): the dx image holds row_mul[r] dx[r][:] (bound through max_r rstd[r] row_mul[r]); dgamma,
 * dbeta, dbias are unaffected.  For the first pre_attn block, whose input image is row-scaled (mdl_split_image_rows): row_mul = row_inv.
 * rstd_max (device float, may be NULL): the forward's max_r rstd[r] * row_mul[r] for THE SAME row_mul; with it and dy_absmax the call
 * issues no bookkeeping launch but the bound kernel. */
int mdl_ln_gelu_drop_bwd_split(const float* x, const float* bias, const float* gamma, const float* beta, const float* mean,
                               const float* rstd, const float* dy, const float* dy_absmax, void* dx_img, float* dx_scale, float* dgamma,
                               float* dbeta, float* dbias, int64_t rows, int W, float p_drop, uint64_t seed, const uint8_t* keep,
                               const float* row_mul, const float* rstd_max, void* ws, void* stream);
/* (round 5) mdl_ln_gelu_drop_bwd_split for a pre-LN tensor whose rows carry a per-group bias row (see mdl_split_gemm_nt_group_bias): the
 * rows of a group are contiguous, cu_groups = device int64 [G + 1] row offsets, G <= 2048.  Additionally dgroup_bias [G][W] = the sum
 * of dx over the rows of each group.  ws: mdl_ln_gelu_drop_bwd_groups_ws_bytes(rows, W, G). */
int64_t mdl_ln_gelu_drop_bwd_groups_ws_bytes(int64_t rows, int W, int G);
int mdl_ln_gelu_drop_bwd_split_groups(const float* x, const float* bias, const float* gamma, const float* beta, const float* mean,
                                      const float* rstd, const float* dy, const float* dy_absmax, void* dx_img, float* dx_scale,
                                      float* dgamma, float* dbeta, float* dbias, int64_t rows, int W, float p_drop, uint64_t seed,
                                      const uint8_t* keep, const float* row_mul, const float* rstd_max, const int64_t* cu_groups, int G,
                                      float* dgroup_bias, void* ws, void* stream);

/* A2 on the split engine (csrc/abmil_gate_split.hip): mdl_abmil_gate_fwd / mdl_abmil_attnpool_bwd(_phases) with E given as a split
 * image (rows of e_rsb bytes holding the H*512 head-major channels, scale e_scale) -- everything else (parameters, scores, saved
 * activations, gradients, dropout, pooling term, `accumulate`) as in the fp32 entry points.  scores == NULL in the backward: no
 * pooling term (plain gate backward).  dE_absmax (device float, may be NULL, zeroed by the caller) is raised to max |dE|.
 * phases of mdl_abmil_attnpool_bwd_split (bit mask, 1 .. 15): 1 = the dz pass (+ bias / wc column sums), 2 = both contractions,
 * 4 = the dX contraction alone, 8 = the dW contraction alone (dWa, dWb) -- the two contractions only read what the dz pass wrote into
 * `ws`, so a caller may queue 8 on another stream behind an event recorded after 1 while 4 and the rest of the backward proceed
 * (measured null on MI355X; the Python mirror issues 3, functional.gate_bwd_raw(phases=...) issues any
 * sequence -- tests/test_split_gpu.py holds 1, 4, 8 == 3 bit for bit). */
int64_t mdl_abmil_gate_fwd_split_ws_bytes(int64_t T, int H);
int mdl_abmil_gate_fwd_split(const void* E_img, int64_t e_rsb, const float* e_scale, const float* Wa, const float* ba, const float* Wb,
                             const float* bb, const float* wc, const float* bc, float* scores, float* act_a, float* act_b, int64_t T,
                             int H, float p_drop, uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b, void* ws, void* stream);
int64_t mdl_abmil_gate_bwd_split_ws_bytes(int64_t T, int H);
int mdl_abmil_attnpool_bwd_split(const void* E_img, int64_t e_rsb, const float* e_scale, const float* Wa, const float* Wb, const float* wc,
                                 const float* act_a, const float* act_b, const float* d_scores, float* dE, int64_t ldE, int accumulate,
                                 float* dWa, float* dWb, float* dba, float* dbb, float* dwc, float* dbc, int64_t T, int H, float p_drop,
                                 uint64_t seed, const uint8_t* keep_a, const uint8_t* keep_b, const float* scores, const float* stat_m,
                                 const float* stat_l, const float* d_pooled, const int32_t* row_bag, int64_t N, float* dE_absmax, void* ws,
                                 void* stream, int phases, int terms);

/* Dispatch plan (ABI 25): what the launcher of `product` chooses for a problem of T tokens (GOT: T = cases k of the launch), WITHOUT
 * launching anything -- host only, no device, no device memory.  Every answer comes from the launcher's own selection functions
 * (splits_for and the per-product split / tile / persistence predicates, the GOT class selection), under the switch values the
 * calling thread's launches would see ("Behaviour switches" below).  `cus`: compute units of the device the plan is for (only the GOT sweeps depend on it;
 * the gate / Linear launchers are sized for the 256 CUs of an MI355X).  out[0 .. n_out) receives up to MDL_PLAN_FIELDS fields
 * (the rest set to 0); returns MDL_E_ARG for an unknown product, bad sizes or n_out < 1, MDL_E_UNSUPPORTED where the launcher
 * would refuse the geometry.
 *
 *   product                      a, b        [VARIANT]                                 [PERSIST]                [EXTRA]
 *   MDL_PLAN_GATE_FP32_BWD       H, -        0                                         0                        0
 *   MDL_PLAN_GATE_SPLIT_FWD      H, -        0                                         persistent mode (0,1,2)  0
 *   MDL_PLAN_GATE_SPLIT_BWD      H, -        0                                         0                        0
 *   MDL_PLAN_GATE_BF16_FWD       H, -        token tile 128 | 256                      persistent mode (0,1,2)  0
 *   MDL_PLAN_GATE_BF16_BWD       H, -        dW tile 128 | 256                         0                        dX token tile 128 | 256
 *   MDL_PLAN_SPLIT_TN            Mi, N       0                                         0                        0
 *   MDL_PLAN_LINEAR_FP32_BWD     N, K        0 small-T | 1 wide (N % 256) | 2 swapped  0                        0
 *   MDL_PLAN_LINEAR_BF16_FWD     N, K        2 (128-col) | 4 (256-col) | 256 (256x256) tiles per workgroup       0
 *   MDL_PLAN_LINEAR_BF16_BWD     N, K        dW tile 128 | 256                         dX tiles per workgroup   dX: 4 (128x256) | 256
 *   MDL_PLAN_GOT                 n, -        size class 64 | 128 | 192 | 256 | 512     row-half products        split sweeps: 0 off,
 *                                                                                                               1 (2k WGs), 2 (+ 4k)
 *   MDL_PLAN_INFONCE_NEG         M, D        1: 16-byte loads of Neg (D % 4 == 0)      0                        LSE partials per row
 *                                            0: 4-byte loads
 *   MDL_PLAN_GOT_TILED           n, d        rows per sweep panel (16)                 0                        launches per IPOT
 *                                                                                                               iteration (2)
 *   MDL_PLAN_GOT_TILED_RECT      n, m        as MDL_PLAN_GOT_TILED                     0                        as MDL_PLAN_GOT_TILED
 * [SPLITS] token splits S of the dW-type contraction (1, with TPS = CHUNK = 0, where there are none), [TPS] tokens per split, [EMPTY] splits that hold no
 * token ((s * tps >= T)), [CHUNK] tokens per chunk of the contraction's main loop (tps is a multiple of it).
 * MDL_PLAN_INFONCE_NEG (T = N rows): [SPLITS] splits over M of the unpaired dQ contraction (1024 negatives each), [CHUNK] waves per row
 * of the paired kernels (64 negatives each); MDL_E_UNSUPPORTED where the unpaired launcher would refuse the geometry.
 * MDL_PLAN_GOT_TILED (T = cases k): [SPLITS] row panels per case (sweep workgroups per case and branch), [TPS] output tile edge of the
 * products (128), [EMPTY] product tiles per case of an n x n product, [CHUNK] columns per sweep chunk (256); MDL_E_UNSUPPORTED for
 * n > 4096 or d > 4096.  MDL_PLAN_GOT_TILED_RECT (a = n tokens of V, b = m tokens of Q): the same fields with [SPLITS] = ceil(n / 16)
 * and [EMPTY] = ceil(n / 128) ceil(m / 128), the tiles of an n x m product; MDL_E_UNSUPPORTED for n > 4096 or m > 4096. */
#define MDL_PLAN_GATE_FP32_BWD 1
#define MDL_PLAN_GATE_SPLIT_FWD 2
#define MDL_PLAN_GATE_SPLIT_BWD 3
#define MDL_PLAN_GATE_BF16_FWD 4
#define MDL_PLAN_GATE_BF16_BWD 5
#define MDL_PLAN_SPLIT_TN 6
#define MDL_PLAN_LINEAR_FP32_BWD 7
#define MDL_PLAN_LINEAR_BF16_FWD 8
#define MDL_PLAN_LINEAR_BF16_BWD 9
#define MDL_PLAN_GOT 10
#define MDL_PLAN_INFONCE_NEG 11
#define MDL_PLAN_GOT_TILED 12
#define MDL_PLAN_GOT_TILED_RECT 13
#define MDL_PLAN_VARIANT 0
#define MDL_PLAN_PERSIST 1
#define MDL_PLAN_SPLITS 2
#define MDL_PLAN_TPS 3
#define MDL_PLAN_EMPTY 4
#define MDL_PLAN_CHUNK 5
#define MDL_PLAN_EXTRA 6
#define MDL_PLAN_FIELDS 7
int mdl_dispatch_plan(int product, int64_t T, int a, int b, int cus, int64_t* out_host, int n_out);

/* Behaviour switches (additive, ABI 26): the A/B and opt-in switches of the launchers, one table (csrc/switches.hip).  Each has an id
 * below, a process-wide value and, per thread, an optional override.  The library reads the environment ONCE, on the first access to any
 * switch (the first launch, plan or mdl_switch_* call of the process), and never again: setting a variable afterwards changes nothing.
 * To change a switch later call mdl_switch_set (the process value) or mdl_switch_set_thread / mdl_switch_clear_thread (the calling
 * thread's override, which wins over the process value for launches issued by that thread).  No value is range-checked; what a number
 * means is decided where the launcher uses it.  All five calls are host only and thread-safe.
 *
 * Two kinds at the first read.  PRESENCE: 1 when the variable exists, whatever its text ("" and "0" included: =0 still means ON), else 0;
 * a launcher tests value != 0.  INTEGER: atoll of the text when the variable exists ("abc" gives 0), else the default.
 *
 *   id                           variable                         kind      default  meaning
 *   MDL_SW_INFONCE_FUSED         MADELEINE_INFONCE_FUSED          presence  0        the one-launch InfoNCE kernels (Kmax <= 256, D <= 512)
 *   MDL_SW_BF16_GATE128          MADELEINE_BF16_GATE128           presence  0        bf16 gate forward on the 128 x 256 tile throughout
 *   MDL_SW_DROP_16BIT            MADELEINE_DROP_16BIT             presence  0        one 16-bit hash per element where p allows the byte hash
 *   MDL_SW_GOT_NO192             MADELEINE_GOT_NO192              presence  0        GOT: 128 < n <= 192 runs in the 256 class
 *   MDL_SW_GOT_NOSPLIT           MADELEINE_GOT_NOSPLIT            presence  0        GOT: one-workgroup IPOT sweeps (no exchange)
 *   MDL_SW_GOT_NO_HALF_PRODUCTS  MADELEINE_GOT_NO_HALF_PRODUCTS   presence  0        GOT: forward C_gamma products as one workgroup per case
 *   MDL_SW_BF16_GATE_PERSIST     MADELEINE_BF16_GATE_PERSIST      integer   1        persistent mode 0 | 1 | 2 of the bf16 256-tile gate forward
 *   MDL_SW_GATE_PERSIST          MADELEINE_GATE_PERSIST           integer   0        persistent mode 0 | 1 | 2 of the split gate forward
 *   MDL_SW_BF16_LIN_PERSIST      MADELEINE_BF16_LIN_PERSIST       integer   1        0: bf16 Linear 256-tile, one column tile per workgroup
 *   MDL_SW_BF16_LIN256_MINK      MADELEINE_BF16_LIN256_MINK       integer   512      smallest contraction of the bf16 Linear 256-tile
 *   MDL_SW_BF16_TN256            MADELEINE_BF16_TN256             integer   1        0: bf16 dW products on the 128 x 256 x 32 tile
 *   MDL_SW_SPLIT_TOKENS          MADELEINE_SPLIT_TOKENS           integer   32768    tokens per split of the dW-type contractions
 *   MDL_SW_SP_NT_STAGES          MADELEINE_SP_NT_STAGES           integer   3        2: the two-stage NT loop of the split engine
 *   MDL_SW_SP_TN_STAGES          MADELEINE_SP_TN_STAGES           integer   3        other than 3: the two-stage TN loop of the split engine
 *   MDL_SW_BF16_STAGES           MADELEINE_BF16_STAGES            integer   3        2: the two-stage loops of the bf16 gate products
 *   MDL_SW_BF16_LIN_STAGES       MADELEINE_BF16_LIN_STAGES        integer   31       2 | 3 | 31 (NT only) | 32 (TN only): bf16 Linear loops
 *
 * Precondition (it held before the table as well): calls that share a workspace run under the same switch values -- a *_ws_bytes query
 * and the launches it sizes, a forward and its backward (mdl_infonce_fwd / _bwd; mdl_abmil_* forward / backward with dropout), and the
 * stages of one GOT call (_extrema, _fwd, _bwd_begin, _bwd_finish).  Nothing checks it: change a switch between steps, not inside one.
 *
 * mdl_switch_get: *value = what the calling thread sees.  mdl_switch_name: the variable's name (a static string), NULL for an id outside
 * 0 .. MDL_SW_COUNT - 1.  The others return MDL_E_ARG for such an id (mdl_switch_get also for value == NULL), MDL_OK otherwise. */
#define MDL_SW_INFONCE_FUSED 0
#define MDL_SW_BF16_GATE128 1
#define MDL_SW_DROP_16BIT 2
#define MDL_SW_GOT_NO192 3
#define MDL_SW_GOT_NOSPLIT 4
#define MDL_SW_GOT_NO_HALF_PRODUCTS 5
#define MDL_SW_BF16_GATE_PERSIST 6
#define MDL_SW_GATE_PERSIST 7
#define MDL_SW_BF16_LIN_PERSIST 8
#define MDL_SW_BF16_LIN256_MINK 9
#define MDL_SW_BF16_TN256 10
#define MDL_SW_SPLIT_TOKENS 11
#define MDL_SW_SP_NT_STAGES 12
#define MDL_SW_SP_TN_STAGES 13
#define MDL_SW_BF16_STAGES 14
#define MDL_SW_BF16_LIN_STAGES 15
#define MDL_SW_COUNT 16
int mdl_switch_get(int id, int64_t* value);
int mdl_switch_set(int id, int64_t value);
int mdl_switch_set_thread(int id, int64_t value);
int mdl_switch_clear_thread(int id);
const char* mdl_switch_name(int id);

/* ------------------------------------------------------------------------------------------------
 * O1 -- multi-tensor fp32 AdamW that skips a step with a non-finite gradient and clips by the global gradient norm in-stream.
 * Replaces optim.AdamW(ssl_model.parameters(), lr=args.lr) (setup_components.py:196) together with the host-side guards that usually
 * surround it (`if not torch.isfinite(loss): continue`, clip_grad_norm_): nothing is read back, copied to the device or allocated.
 *
 * One step of the caller, for each set of nt <= MDL_ADAMW_MAX_TENSORS tensors (a parameter group is one or more sets):
 *   1. mdl_adamw_grad_stats  (only with MDL_ADAMW_GUARD or MDL_ADAMW_CLIP; statistics launch `slot` of the step's `stat_launches`)
 *   2. mdl_adamw_update      after EVERY statistics launch of the step: the verdict and the norm are global over all sets
 *   3. mdl_adamw_commit      after the set's update; MDL_ADAMW_FINAL on the step's last commit
 * The number of launches does not depend on the outcome.  The *_host arguments are HOST arrays of nt device pointers / sizes, read
 * during the call and passed to the kernels by value (gradient addresses may change every step).  Every tensor is fp32 and dense;
 * p, g and the moments need 4-byte alignment only (16-byte accesses where a tensor's pointers allow them).  A tensor of zero
 * elements is accepted (its step still advances); step[i] is torch's per-parameter `step`, one fp32 value on the device.
 *
 * Update of an applied step, per element, t = step[i] + 1:   p *= 1 - lr wd;  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),   g' = g min(1, max_norm / (norm + 1e-6)) with MDL_ADAMW_CLIP,
 *   else g.  g is never written.  lr, beta1, beta2, eps, weight_decay and max_norm are passed as the BIT PATTERNS of doubles
 *   (*_bits): every derived scalar is formed in double on the device and rounded to fp32 once, as torch.optim.AdamW does on the host.
 * With MDL_ADAMW_GUARD a step in which any gradient element of any set is inf or NaN (decided per element) is void: update and
 * commit write nothing except, in the FINAL commit, grad_norm and skipped[0] += 1.
 *
 * ws: mdl_adamw_ws_bytes(stat_launches) bytes, 16-byte aligned, shared by all calls of one step: MDL_ADAMW_STAT_BLOCKS partial
 * {sum of squares, non-finite} pairs per statistics launch, every one of them rewritten by its launch and merged in a fixed order
 * (no float atomics: two runs give the same bits).  May be NULL with neither GUARD nor CLIP.  grad_norm [1] (the global norm, written
 * by the FINAL commit when statistics ran) and skipped [1] belong to the caller and persist between steps. */
#define MDL_ADAMW_MAX_TENSORS 48
#define MDL_ADAMW_STAT_BLOCKS 512
#define MDL_ADAMW_MAX_STAT_LAUNCHES 64
#define MDL_ADAMW_GUARD 1
#define MDL_ADAMW_CLIP 2
#define MDL_ADAMW_FINAL 4
int64_t mdl_adamw_ws_bytes(int64_t stat_launches);
int mdl_adamw_grad_stats(int nt, const float* const* g_host, const int64_t* numel_host, void* ws, int64_t slot, int64_t stat_launches,
                         void* stream);
int mdl_adamw_update(int nt, float* const* p_host, const float* const* g_host, float* const* exp_avg_host,
                     float* const* exp_avg_sq_host, const float* const* step_host, const int64_t* numel_host, uint64_t lr_bits,
                     uint64_t beta1_bits, uint64_t beta2_bits, uint64_t eps_bits, uint64_t weight_decay_bits, uint64_t max_norm_bits,
                     int flags, const void* ws, int64_t stat_launches, void* stream);
int mdl_adamw_commit(int nt, float* const* step_host, int flags, const void* ws, int64_t stat_launches, float* grad_norm,
                     int64_t* skipped, void* stream);

/* ------------------------------------------------------------------------------------------------
 * S1 -- draw and gather a whole batch of bags from a device-resident feature store, in one launch (ABI 26, additive).
 * Replaces the input side of the reference (madeleine/datasets/wsi_dataset.py): SlideDataset.sample_n (:42-50), the 2-token zero bag
 * of an absent stain (:66) and collate's stack (:86-99) -- without the h5 re-reads, the host draw and the per-step host-to-device copy.
 *
 * store: T_total rows of D elements, row_stride ELEMENTS apart (>= D), stored as dtype = MDL_STORE_F32 / _F16 / _BF16; 16-byte
 *   aligned.  off [n_bags + 1] (int64, ascending): bag g is rows off[g] .. off[g + 1] - 1.  All of it is only read.
 * bag [R] (int32): the stored bag of output row r, or -1 for an absent stain.  key_id [R] (int64) names row r's random stream: the draw
 *   of row r is a pure function of (seed, counter, key_id[r]) and of the bag's length -- not of R, of r or of the other rows.
 *   key_id == NULL stands for key_id[r] = bag[r].
 * out [R, N, D] fp32, dense, 16-byte aligned; every element is written.  idx_out [R, N] (int32) or NULL: the chosen row of the bag
 *   (0-based inside the bag), -1 in the rows of an absent stain.
 *
 * With n = off[bag + 1] - off[bag] (sample_n's semantics, in distribution -- the bits are this kernel's own, not torch's generators'):
 *   n >= N      N distinct rows: a uniformly random N-subset in uniformly random order (randperm(n)[:N]); a permutation at n == N
 *   1 <= n < N  N rows drawn independently and uniformly, with replacement (randint(0, n, (N,)))
 *   bag == -1   N x D zeros (what collate stacks for the dataset's zero bag).  A bag index outside [0, n_bags), an empty bag, a bag
 *               of more than 2^31 - 1 rows or one that leaves [0, T_total) is written as an absent stain: the kernel never reads
 *               outside the store.
 * Rows are copied bit for bit from an fp32 store and converted exactly from fp16 / bf16.  Any D >= 1: 16-byte accesses when D and
 * row_stride are multiples of 4 (fp32) / 8 (16-bit stores) elements, element-wise accesses otherwise.  No workspace.
 * MDL_E_UNSUPPORTED: R * N or the grid R * ceil(N / 64) beyond int32. */
#define MDL_STORE_F32 0
#define MDL_STORE_F16 1
#define MDL_STORE_BF16 2
int mdl_bag_sample(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                   const int32_t* bag, const int64_t* key_id, int64_t R, int N, int D, uint64_t seed, uint64_t counter, float* out,
                   int32_t* idx_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * S2 -- pack a batch of bags of DIFFERENT lengths from the store of S1 into one dense token tensor, in one launch (ABI 26, additive).
 * Replaces, for ragged batches (MADELEINE.forward_ragged; the reference can only stack equal-N bags, wsi_dataset.py:89-92), the
 * torch.cat of the bags, the zero bags of absent stains (wsi_dataset.py:66) and the per-token bag map, and bounds a bag by a draw
 * without replacement on the device.
 *
 * store, dtype, row_stride, T_total, off, n_bags, bag [R], key_id [R] or NULL, seed, counter: as in S1.
 * cu [R + 1] (int64, device, ascending, cu[0] = 0 and cu[R] = T_out): output bag r is rows cu[r] .. cu[r + 1] - 1 of out; its length
 *   L = cu[r + 1] - cu[r] is the caller's choice (the store passes min(n, max_tokens), and 2 for an absent stain).
 * chunk_cu [R + 1] (int64, device): the prefix sum of ceil(L_r / 64), chunk_cu[0] = 0; n_chunks = chunk_cu[R] is the grid (one
 *   workgroup per 64 rows of a bag; the workgroup finds its bag by binary search in chunk_cu).
 * out [T_out, D] fp32, dense, 16-byte aligned.  row_bag [T_out] (int32) or NULL: r on every row of bag r.  idx_out [T_out] (int32) or
 *   NULL: the row inside the stored bag, -1 where zeros were written.
 *
 * Per output bag r, with n = off[bag + 1] - off[bag]:
 *   bag absent or invalid by S1's rule   L rows of zeros, idx -1
 *   L >= n   the bag taken whole: rows t < n are stored rows t in stored order; rows t >= n (inconsistent tables only) zeros, idx -1
 *   L <  n   row t is the stored row that mdl_bag_sample draws for token t with N = L under the same (seed, counter, key_id[r]) --
 *            the same bits: L distinct rows, a uniformly random L-subset in uniformly random order
 * Rows are copied bit for bit from an fp32 store and converted exactly from fp16 / bf16; access widths as in S1.  With consistent
 * tables every element of out, row_bag and idx_out is written.  With inconsistent ones nothing outside the store is read and nothing at
 * or beyond row T_out is written (a (bag, chunk) the tables do not agree on writes nothing).  No workspace, no atomics.
 * MDL_E_UNSUPPORTED: R, T_out or n_chunks beyond int32.  R == 0, T_out == 0 or n_chunks == 0: nothing is launched. */
int mdl_bag_pack(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                 const int32_t* bag, const int64_t* key_id, const int64_t* cu, const int64_t* chunk_cu, int64_t R, int64_t n_chunks,
                 int64_t T_out, int D, uint64_t seed, uint64_t counter, float* out, int32_t* row_bag, int32_t* idx_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * S3, S4 -- S1 and S2 over a store in TWO TIERS (ABI 26, additive): rows [0, T_dev) of the store in device memory at `store`, rows
 * [T_dev, T_total) in pinned host memory at `store_host`, read by the kernel over PCIe.  For a cohort that does not fit in HBM.
 *
 * store: the device tier, T_dev rows (NULL allowed when T_dev == 0).  store_host: the host tier, T_total - T_dev rows, as the HOST
 *   address of registered (pinned) host memory -- hipHostMalloc or hipHostRegister -- or a device address (NULL allowed when T_dev ==
 *   T_total).  Both tiers share dtype and row_stride; 16-byte aligned.  off, n_bags and bag keep addressing rows of [0, T_total): a
 *   valid bag g with off[g + 1] <= T_dev is read at store + off[g] * row_stride, one with off[g] >= T_dev at store_host + (off[g] -
 *   T_dev) * row_stride, and a bag on both sides of T_dev falls under S1's bounds rule (zeros, idx -1; no address is formed from it).
 * host_wgs: the grid of the host-tier pass, 0 for the built-in default (64).  The work items (output row x 64-token chunk, pack chunk)
 *   whose bag is in the host tier are walked by host_wgs persistent workgroups in a launch of their own; the items of resident bags
 *   and of absent stains keep the one-workgroup-per-item grid of S1 / S2 in another.  Both go to `stream`.
 * Every other argument, the three draw regimes, the whole-bag rule of S2, access widths, exact widening, the bounds on the store and
 *   on the output side and the refusals are S1's and S2's: the kernels share their code, and with T_dev == T_total the outputs are
 *   bit-equal to S1 / S2.  A bag's draw does not depend on its tier.
 * Before any launch the entry points ask the runtime what store_host is (hipPointerGetAttributes on its first and last byte, the
 *   allocation's extent where hipMemGetAddressRange reports one) and resolve its device-visible address (hipHostGetDevicePointer).
 *   MDL_E_ARG for pageable, managed or unknown memory, for a tier that leaves its allocation, for T_dev outside [0, T_total] and for
 *   host_wgs < 0: no kernel is ever launched on a pointer the device cannot read. */
int mdl_bag_sample_tiered(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev,
                          const int64_t* off, int64_t n_bags, const int32_t* bag, const int64_t* key_id, int64_t R, int N, int D,
                          uint64_t seed, uint64_t counter, float* out, int32_t* idx_out, int host_wgs, void* stream);
int mdl_bag_pack_tiered(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev,
                        const int64_t* off, int64_t n_bags, const int32_t* bag, const int64_t* key_id, const int64_t* cu,
                        const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int64_t T_out, int D, uint64_t seed, uint64_t counter,
                        float* out, int32_t* row_bag, int32_t* idx_out, int host_wgs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * S5 -- the column means of whole stored bags: one vector per slide without the features leaving the store (ABI 26, additive).
 * Replaces, for a cohort held in the store of S1 / S3, the loop of bin/extract_mean_embs.py (h5 read, feats.mean(0) per slide): the
 * mean patch embedding that bin/run_linear_probing.py names as the baseline of every probe.
 *
 * store, dtype, row_stride, T_total, off, n_bags, bag [R]: as in S1; store_host, T_dev, host_wgs (mdl_bag_mean_tiered): as in S3.
 * out [R, D] fp32, dense, 16-byte aligned: out[r, :] is the mean over ALL rows of stored bag bag[r]; a row of zeros (the mean of the
 *   dataset's zero bag) for bag[r] == -1 and for a bag that is invalid by S1's bounds rule.
 * chunk_cu [R + 1] (int64, device): the prefix sum of ceil(n_r / MDL_BAG_MEAN_ROWS), n_r the rows of bag[r] (0 for an absent stain),
 *   chunk_cu[0] = 0; n_chunks = chunk_cu[R].  The same kind of table as S2's, with MDL_BAG_MEAN_ROWS for 64.
 * ws: n_chunks * D floats (mdl_bag_mean_ws_bytes), 16-byte aligned, contents need no initialisation.
 *
 * Two launches, no atomics.  A work item is (output row r, chunk c): rows c * MDL_BAG_MEAN_ROWS .. of the bag, a contiguous range of
 * the store.  One workgroup of MDL_BAG_MEAN_THREADS threads per item; a thread owns MDL_BAG_MEAN_COLS adjacent columns (16-byte loads
 * when D and row_stride are multiples of 4 (fp32) / 8 (16-bit stores) elements, element-wise loads otherwise; fp16 / bf16 widened
 * exactly) in one of G row groups,
 *     G = MDL_BAG_MEAN_THREADS / min(MDL_BAG_MEAN_THREADS, next_pow2(ceil(D / MDL_BAG_MEAN_COLS)))
 * and adds rows grp, grp + G, grp + 2 G, .. of the chunk in that order in fp32; the G sums are added in group order through LDS and
 * the item's partial [D] goes to ws.  The second launch adds a bag's partials in chunk order, divides by n and writes out[r].
 * Tiered: the items with a row at or beyond T_dev are walked by host_wgs persistent workgroups in a launch of their own, the others
 * keep the one-workgroup-per-item grid; the tier is chosen per ROW, so a bag on both sides of T_dev is served like any other.
 *
 * Bit contract.  The bits of out[r] depend only on the rows of bag bag[r] (their values as stored), on D and on MDL_BAG_MEAN_ROWS
 * (with _THREADS and _COLS): not on R, on the other bags or their order, on the tier of any row, on host_wgs or on row_stride (the
 * 16-byte and the element-wise loads feed the same additions).  Addition depth: an element of out[r] of a bag of len rows has passed
 * through at most
 *     h(len) = ceil(min(len, MDL_BAG_MEAN_ROWS) / G) + (G - 1) + (ceil(len / MDL_BAG_MEAN_ROWS) - 1)
 * fp32 additions (its row group's, the merge of the groups, the chunks), each of them rounded once, and one fp32 division.
 *
 * MDL_E_ARG: store / off / bag / chunk_cu / out / ws NULL, R, n_chunks, T_total or n_bags < 0, D < 1, row_stride < D, unknown dtype,
 * (tiered) T_dev outside [0, T_total], host_wgs < 0 or a host tier the device cannot read.  MDL_E_ALIGN: store, out or ws not 16-byte
 * aligned, a table misaligned for its type.  MDL_E_UNSUPPORTED: R or n_chunks beyond int32.  R == 0 or n_chunks == 0: MDL_OK, nothing
 * is launched and nothing written (n_chunks == 0 with R > 0 means every bag is absent: the zeros are the caller's).  With inconsistent
 * tables nothing outside the store is read and nothing outside out [R, D] and ws is written: a (bag, chunk) that chunk_cu and off do
 * not agree on writes no partial, and a bag whose chunk range disagrees with its length is a row of zeros. */
#define MDL_BAG_MEAN_ROWS 1024
#define MDL_BAG_MEAN_THREADS 256
#define MDL_BAG_MEAN_COLS 8
int64_t mdl_bag_mean_ws_bytes(int64_t n_chunks, int D);
int mdl_bag_mean(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags, const int32_t* bag,
                 const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int D, float* out, void* ws, void* stream);
int mdl_bag_mean_tiered(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev,
                        const int64_t* off, int64_t n_bags, const int32_t* bag, const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int D,
                        float* out, void* ws, int host_wgs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * P1-P3 -- the few-shot linear probe: P independent L2-regularised logistic fits over one embedding matrix, the decision values of
 * every case under every fit, and confusion matrix + AUC per fit (ABI 26, additive).  Replaces, for all (task, k, fold) problems of an
 * evaluation at once, bin/run_linear_probing.py:150-170: LogisticRegression(C=1, max_iter=10000).fit / .predict / .predict_proba
 * (:150-155), roc_auc_score (:46, :49) and the counts behind balanced_accuracy_score / cohen_kappa_score (:50, :163-164).
 *
 * X [S, d] fp32, row stride ldX >= d ELEMENTS, any d >= 1; only read.  C classes, 2 <= C <= MDL_PROBE_MAX_CLASSES; cols = 1 for C == 2
 * (sklearn's binary form), cols = C otherwise (multinomial).
 * y (int32): the label vector of problem p is y[p * ldy .. p * ldy + S); ldy == 0 shares one vector among all problems (several tasks
 *   of equal C go through one call with ldy = S).  Labels are 0 .. C-1; any other value (the reference's -1) marks an unlabeled case,
 *   which is in neither the training nor the test set.
 * train_idx [P, n_max] (int32), n_train [P] (int32): problem p trains on cases train_idx[p, 0 .. n_train[p]); the rest of the row is
 *   never read.  1 <= n_train[p] <= n_max <= MDL_PROBE_MAX_TRAIN.  Every labeled case that is not a training case is a test case.
 *
 * mdl_probe_fit minimises, per problem,
 *   C == 2:  cost * sum_i softplus(-(2 y_i - 1)(w . x_i + b)) + 1/2 |w|^2
 *   C  > 2:  cost * sum_i CE(softmax(W x_i + b), y_i)        + 1/2 |W|_F^2      (b unpenalised; returned with zero mean)
 * by Newton-CG in the span of the training rows (W = A^T X_train, Gram matrix in the workspace): one Gram launch, then one workgroup
 * per problem.  No workgroup waits on another; every loop is bounded (max_iter Newton steps, MDL_PROBE_CG_MAX CG steps each,
 * MDL_PROBE_LS_MAX step halvings).  A problem has converged when the inf-norm of the primal gradient (with respect to W and b, evaluated
 * in fp32 from W itself) is <= gtol; it stops after max_iter steps at the latest.  Once below gtol the iteration goes on only while a
 * step still halves that norm and it is above 0.03 gtol: stopping at the first value below gtol would leave the decision values of the
 * smallest problems more than 1e-3 off the optimum.
 * W_out [P, cols, d], b_out [P, cols]; info_out [P, 4] fp32: Newton steps taken, converged (1 / 0), the final inf-norm of the gradient,
 * CG steps in all.  A problem with n_train outside [1, n_max], a training index outside [0, S) or an unlabeled training case writes
 * NaN to its W, b and residual and converged = 0; the others are unaffected.  Results depend on the problem alone (not on P or p).
 *
 * mdl_probe_scores: z_out [P, S, cols] = X W_p^T + b_p for ALL S cases.  Prediction: z > 0 for C == 2 (z == 0 is class 0), argmax with
 * the lowest index on ties otherwise.
 *
 * mdl_probe_metrics, over the test cases of problem p: confusion_out [P, C, C] int32 (row = truth, column = prediction) and auc_out [P]
 * fp32 = roc_auc_score: the Mann-Whitney statistic with ties counted 1/2 -- C == 2: cases ranked by z; C > 2: one-vs-rest macro average,
 * class c ranked by log_softmax(z)[c] evaluated in fp64.  NaN where a class has no test case (C == 2: either class).  Exact pair
 * counting in integers, S <= MDL_PROBE_MAX_CASES; the order of the atomic additions cannot change a bit of the result.
 *
 * Workspaces: 16-byte aligned, sizes from the *_ws_bytes queries, contents need no initialisation.
 * Refusals, in this order, all before any launch and before any device pointer is touched (one check for every entry point that takes
 * the problem list: P1, P3, L1, L2, S1, S2 and B2, B3 of madeleine_amd_stats.h).
 *   (1) MDL_E_ARG: a NULL pointer; P, n_max or S < 1; d < 1 or ldX < d; max_iter < 0, cost not > 0, gtol not >= 0; ldy neither 0 nor >= S.
 *   (2) MDL_E_UNSUPPORTED: n_max > MDL_PROBE_MAX_TRAIN, C outside [2, MDL_PROBE_MAX_CLASSES], S > MDL_PROBE_MAX_CASES (metrics); S, P,
 *       P * n_max, P * cols * d or a launch grid beyond int32.
 *   (3) MDL_E_ALIGN: ws not 16-byte aligned.
 * A call with a fault of (2) and one of (3) is answered with (2).  (While every entry point carried its own checks, the fits and the
 * metrics of P, L and S looked at the alignment before the int32 bounds of their grids and answered such a call MDL_E_ALIGN; a call with
 * one fault gets what it always got.)
 * mdl_probe_scores takes no problem list and follows the same three steps. */
#define MDL_PROBE_MAX_TRAIN 256
#define MDL_PROBE_MAX_CLASSES 8
#define MDL_PROBE_MAX_CASES 16384
#define MDL_PROBE_CG_MAX 400
#define MDL_PROBE_LS_MAX 24
int64_t mdl_probe_fit_ws_bytes(int64_t P, int n_max, int d, int C);
int mdl_probe_fit(const float* X, int64_t ldX, int64_t S, int d, const int32_t* y, int64_t ldy, const int32_t* train_idx,
                  const int32_t* n_train, int64_t P, int n_max, int C, float cost, float gtol, int max_iter, float* W_out, float* b_out,
                  float* info_out, void* ws, void* stream);
int mdl_probe_scores(const float* X, int64_t ldX, int64_t S, int d, const float* W, const float* b, int64_t P, int C, float* z_out,
                     void* stream);
int64_t mdl_probe_metrics_ws_bytes(int64_t P, int64_t S, int C);
int mdl_probe_metrics(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train, int64_t P,
                      int n_max, int64_t S, int C, int32_t* confusion_out, float* auc_out, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L1-L2 -- the full-label linear probe: the fits of P1 with any number of training rows, and the metrics of P3 over problem tables
 * of that width (ABI 26, additive).  For the cross-validated linear probe trained on all labels (K folds of a cohort): n > d, where the
 * n x n Gram matrix of P1 is the wrong form.  X, y, ldy, train_idx, n_train, cost, gtol, max_iter, W_out, b_out, info_out mean what
 * they mean in P1-P3, with 1 <= n_train[p] <= n_max <= MDL_LOGIT_MAX_TRAIN and 1 <= d <= MDL_LOGIT_MAX_DIM.  The decision values between
 * the two calls come from mdl_probe_scores.
 *
 * mdl_logit_fit minimises the objective of mdl_probe_fit in the primal unknowns (W [cols, d], b [cols]) by Newton-CG, one workgroup
 * per problem, one launch.  Every product with X is one sweep over the training rows (n d 4 bytes): a wave takes a few rows into
 * registers, dots them with the vector in LDS, applies the row's loss Hessian (or residual) and accumulates x_i u_i^T in wave-private
 * registers; the waves are added through LDS in a fixed order.  The row -> wave assignment is a function of n alone.  One sweep per CG
 * step, one for the gradient and the decision values of every Newton step -- always from W itself, so the stop rule sees the gradient
 * of what is returned --, one for the change of the decision values along the step; the step length halves on the directional
 * derivative along the line, O(n cols) per trial.  No workgroup waits on another, no floating-point atomic, every sum in a fixed order;
 * every loop is bounded (max_iter Newton steps, MDL_LOGIT_CG_MAX CG steps each, MDL_LOGIT_LS_MAX step halvings).  Stop rule, meaning of
 * gtol and of `converged`, info_out [P, 4] and the zero-mean multinomial intercept: as mdl_probe_fit.  A problem with n_train outside
 * [1, n_max], a training index outside [0, S) or an unlabeled training case writes NaN to its W, b and residual and converged = 0 and
 * reads nothing of X; the others are unaffected.  A problem's bits depend on that problem alone (not on P, p, n_max or the others' sizes).
 * ws: mdl_logit_fit_ws_bytes = P * (3 * n4 * cols + d * nc) * 4 bytes with n4 = n_max rounded up to a multiple of 4 and nc = 1, 4 or 8
 * (cols rounded up to a width the kernel is built for): the decision values, the Hessian weights and the change of the decision values
 * along the step of every training row (n cols 4 bytes each: 512 KiB at n = 16384, cols = 8, more than the LDS holds), and W during the
 * iteration.
 *
 * mdl_logit_metrics: mdl_probe_metrics (the same three kernels, the same workspace size) for n_max <= MDL_LOGIT_MAX_TRAIN.
 *
 * Workspaces: 16-byte aligned, contents need no initialisation.  MDL_E_UNSUPPORTED: n_max > MDL_LOGIT_MAX_TRAIN, d > MDL_LOGIT_MAX_DIM
 * (fit), C outside [2, MDL_PROBE_MAX_CLASSES], S > MDL_PROBE_MAX_CASES (metrics), a launch grid or an output index beyond int32.
 * MDL_E_ARG, MDL_E_ALIGN: as P1-P3, and in the three steps of P1-P3: (1) MDL_E_ARG, (2) every MDL_E_UNSUPPORTED, (3) MDL_E_ALIGN.  All of
 * it is checked before anything is launched. */
#define MDL_LOGIT_MAX_TRAIN 16384
#define MDL_LOGIT_MAX_DIM 1024
#define MDL_LOGIT_CG_MAX 400
#define MDL_LOGIT_LS_MAX 24
int64_t mdl_logit_fit_ws_bytes(int64_t P, int n_max, int d, int C);
int mdl_logit_fit(const float* X, int64_t ldX, int64_t S, int d, const int32_t* y, int64_t ldy, const int32_t* train_idx,
                  const int32_t* n_train, int64_t P, int n_max, int C, float cost, float gtol, int max_iter, float* W_out, float* b_out,
                  float* info_out, void* ws, void* stream);
int64_t mdl_logit_metrics_ws_bytes(int64_t P, int64_t S, int C);
int mdl_logit_metrics(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train, int64_t P,
                      int n_max, int64_t S, int C, int32_t* confusion_out, float* auc_out, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A-map -- the attention read-out: per bag and head the softmax of the raw scores with its statistics, an exact stable descending
 * order, percentile ranks and the k best rows, for all bags of a pack in one launch sequence (ABI 26, additive).  Replaces, for the
 * raw scores MADELEINE.forward(..., return_attention=True) returns (Model.py:205-216), the per-bag, per-head host loop of
 * softmax / argsort / scipy.stats.rankdata(scores, 'average') / n * 100 that a heatmap is coloured by.
 *
 * scores [T, H] fp32, row stride ld >= H ELEMENTS; only read.  cu [R + 1] (int64, device): bag r is rows cu[r] .. cu[r + 1] - 1, n =
 *   cu[r + 1] - cu[r] of them.  H in {1, 2, 4, 8}; T and R within int32.  A SEGMENT is one (bag, head) pair.
 * ws: mdl_attn_map_ws_bytes(T, R, H) bytes for either call, 16-byte aligned, contents need no initialisation.
 *
 * mdl_attn_softmax: attn [T, H] (dense), m [R, H], l [R, H].  m is the exact maximum of the segment (fmaxf: a NaN is passed over
 *   unless every score is one), l = sum expf(s - m), attn = expf(s - m) / l (one fp32 division).  An empty bag writes m = -inf, l = 0
 *   and no attn.  A chunk is MDL_ATTN_ROWS consecutive rows of a segment and one workgroup of 256 threads: thread t adds its rows t,
 *   t + 256, .. in row order, the 64 lanes of a wave are added by xor butterflies, the four waves as (0 + 1) + (2 + 3), and one thread
 *   adds a segment's chunk partials in chunk order.  No atomics.  Addition depth: l of a segment of n rows has passed through at most
 *       h(n) = (MDL_ATTN_ROWS / 256 - 1) + 6 + 2 + (ceil(n / MDL_ATTN_ROWS) - 1)
 *   fp32 additions, each rounded once.
 *   Bit contract: the bits of a segment's attn, m and l depend on its own scores only -- not on R, on the other bags or their
 *   order, on where the bag lies in the pack or on ld.  Six launches.
 *
 * mdl_attn_rank: an exact, stable segmented sort of the raw scores.
 *   Comparison rule: ordinary float order; -0.0 equals +0.0; every NaN ties with every other NaN and ranks above +inf.  The result
 *   is therefore defined for any bit pattern.
 *   order [H, T] (int32): order[h, cu[r] + j] is the row INSIDE bag r (0-based) of its j-th highest score in head h; ties are broken
 *     by the lower row.
 *   pct [T, H] (dense fp32) or NULL: with L the count of the segment's scores strictly below this one and E the count equal to it,
 *     itself included, pct = (float)(100.0 * (2 L + E + 1) / (2.0 * n)), evaluated in double and rounded once: scipy's
 *     rankdata(scores, 'average') / n * 100.
 *   topk_idx [R, H, k] (int32), topk_val [R, H, k] (fp32), k >= 0 (both may be NULL for k == 0): the first min(k, n) entries of the
 *     segment's order and their raw scores (bit for bit), padded with -1 and -inf.
 *   An LSD radix sort on a 32-bit key (the usual float-to-unsigned transform after canonicalising -0 and NaN, inverted, so that the
 *   ascending stable sort gives the descending order with ties in row order), 8-bit digits, four passes of three launches: per-chunk
 *   digit counts (MDL_ATTN_SORT_KEYS keys per workgroup, a chunk never crosses a segment), a per-segment exclusive scan (digit-major,
 *   chunk-minor), a stable scatter (one wave per chunk, 64 keys a round, the rank among equal digits from 64-bit ballot matches).
 *   pct finds the run of equal keys by binary search in the sorted segment.  1 + 1 + 12 + (pct) 1 + (k > 0) 1 launches, whatever R
 *   and T.  The results are exact, so they depend on the segment's scores alone.
 *
 * No workgroup waits on another (launch order is the only dependency), no float atomics, no library sort.
 * Refusals, in this order.  MDL_E_ARG: scores / cu / ws or a required output NULL, T < 0, R < 0, ld < H, k < 0.  MDL_E_UNSUPPORTED:
 * H outside {1, 2, 4, 8}, T or R beyond int32, a launch grid (T / MDL_ATTN_SORT_KEYS + R chunks, R * H segments, R * H * k / 256)
 * beyond int32.  MDL_E_ALIGN: ws not 16-byte aligned, cu not 8-byte, a float / int32 buffer not 4-byte aligned.  R == 0 or T == 0:
 * MDL_OK, nothing is launched and nothing written.
 * With a cu that is not monotone or that leaves [0, T], nothing outside the given buffers is read or written: a bag with cu[r] < 0,
 * cu[r + 1] < cu[r] or cu[r + 1] > T is served as an empty bag (and bags that overlap write each other's rows). */
#define MDL_ATTN_ROWS 1024
#define MDL_ATTN_SORT_KEYS 1024
int64_t mdl_attn_map_ws_bytes(int64_t T, int64_t R, int H);
int mdl_attn_softmax(const float* scores, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int H, float* attn, float* m, float* l,
                     void* ws, void* stream);
int mdl_attn_rank(const float* scores, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int H, int64_t k, int32_t* order, float* pct,
                  int32_t* topk_idx, float* topk_val, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * R1 -- the smooth rank: exp(entropy of the normalised singular values) of an embedding matrix, on the device (ABI 26, additive).
 * Replaces smooth_rank_measure (madeleine/utils/utils.py:180-201): S = svd(E), p = S / |S|_1 + eps, p = p[:d], exp(-sum p ln p) --
 * the model-selection criterion of bin/pretrain.py:69-72, returned by train_loop and run_inference.
 *
 * E [n, d] fp32, row stride ldE >= d ELEMENTS (any such value: every offset into E is formed in 64 bits, there is no 32-bit limit;
 *   a column slice of a wider buffer is fine), 4-byte aligned; only read.  k = min(n, d) <= MDL_RANK_MAX_K; n, d <= 2^31 - 1.
 * eps_bits: the bit pattern of the fp64 eps (the header has no double; as mdl_adamw_update's scalars).
 * sigma [k] fp64 (8-byte aligned): the singular values, descending, >= 0.  out [2] fp64: exp(H) (unrounded; the reference rounds it to
 *   2 decimals) and H = -sum_i p_i ln p_i, p_i = sigma_i / sum(sigma) + eps over all k values.
 * ws: mdl_smooth_rank_ws_bytes(n, d) bytes, 16-byte aligned, contents need no initialisation ((chunks + 1) k^2 + 4 k doubles).
 *
 * Arithmetic, all fp64:
 *   1. Gram matrix G = E^T E (n >= d) or E E^T (n < d), k x k.  The fp32 inputs are widened first, so every product is exact and only
 *      the additions round.  The contraction (length L = max(n, d)) is cut into chunks of MDL_RANK_GRAM_ROWS rows -- or, beyond
 *      MDL_RANK_GRAM_MAX_CHUNKS of those, into that many equal chunks (a multiple of 16 rows each); a workgroup adds one chunk's
 *      rows in order into a MDL_RANK_GRAM_TILE-square tile of that chunk's partial, and a second launch adds the partials in chunk
 *      order.  Tiles on or below the diagonal are formed, the others mirrored: G is symmetric bit for bit.
 *   2. Householder reduction to tridiagonal form: k - 2 steps, each a launch for p = beta A v and a launch for the symmetric rank-2
 *      update of the trailing block, over blocks of MDL_RANK_TRI_ROWS rows.  Every workgroup rebuilds the step's reflector (and
 *      p^T v) from the k numbers involved, in the same fixed order.
 *   3. Every eigenvalue of the tridiagonal matrix by Sturm-count bisection from the Gershgorin interval: one thread each, 64 halvings,
 *      pivots inside (-pivmin, pivmin) taken as -pivmin, pivmin = DBL_MIN max(1, max e^2) (LAPACK dstebz).
 *   4. One workgroup: sigma_i = sqrt(max(lambda_i, 0)), their sum, p, H, in a fixed order.
 *   The tridiagonalisation perturbs G by O(k 2^-52) lambda_max: relative error of a singular value that is not tiny against sigma_max
 *   ~1e-13; singular values that are exactly zero come out as noise of at most sqrt(k 2^-52) sigma_max.
 *   Launches: 2 k (k >= 2; 4 for k == 1), a function of (n, d) alone.  No atomics, no host read, no workgroup waits on another, every
 *   loop's trip count is a function of (n, d).
 *   Bit contract: sigma and out depend on (E, n, d, ldE, eps) alone.
 * Edge values: an all-zero E gives sigma = 0 and out = NaN (0 / 0, as the reference).  A NaN or Inf anywhere in E gives NaN in out (and
 * in sigma); the call returns normally.  Squares of G's entries must stay finite in fp64 (|E| sqrt(L) below 1e37 is enough).
 *
 * Refusals, in this order, before any launch.  MDL_E_ARG: n < 1, d < 1, ldE < d, a NULL pointer.  MDL_E_ALIGN: E not 4-byte, sigma /
 * out not 8-byte, ws not 16-byte aligned.  MDL_E_UNSUPPORTED: k > MDL_RANK_MAX_K, n or d beyond int32, n * ldE beyond 2^61.
 * mdl_smooth_rank_ws_bytes returns the same negative codes for its sizes.
 *
 * mdl_smooth_rank_marked: the same call, which also records four caller-created hipEvent_t (marks_host [4], a HOST array of event
 * handles) on the stream: before the Gram launches, after them, after the tridiagonalisation and after the finish -- the stage times
 * of tools/exp_rank.py.  MDL_E_ARG for a NULL array or handle. */
#define MDL_RANK_MAX_K 1024
#define MDL_RANK_GRAM_ROWS 512
#define MDL_RANK_GRAM_MAX_CHUNKS 16
#define MDL_RANK_GRAM_TILE 64
#define MDL_RANK_TRI_ROWS 16
int64_t mdl_smooth_rank_ws_bytes(int64_t n, int64_t d);
int mdl_smooth_rank(const float* E, int64_t ldE, int64_t n, int64_t d, uint64_t eps_bits, void* sigma, void* out, void* ws, void* stream);
int mdl_smooth_rank_marked(const float* E, int64_t ldE, int64_t n, int64_t d, uint64_t eps_bits, void* sigma, void* out, void* ws,
                           void* const* marks_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * X1 -- cross-stain retrieval: pair ranks and top-k neighbours over embedding matrices, on the device (ABI 26, additive).
 * The label-free measure of what the contrastive loss optimises: at which rank does the embedding of a case's own IHC slide come back
 * among all the others, given its H&E embedding -- and the "most similar slides" query over the same matrices.
 *
 * Q [n, d] queries, K [m, d] gallery: fp32, row strides ldq, ldk >= d ELEMENTS (every offset is formed in 64 bits), 4-byte aligned,
 *   only read; Q and K may be the same pointer.  metric MDL_RETR_COSINE: rows scaled by 1 / max(|x|_2, 1e-12) (InfoNCE's rule);
 *   MDL_RETR_DOT: rows as they are.  The similarities s_ij come from the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) with fp32
 *   accumulation, in tiles that are consumed where they are produced: the [n, m] matrix is never written to memory.
 * ws: mdl_retrieval_ws_bytes(n, m, d, k, col_chunks) bytes, 16-byte aligned, contents need no initialisation: the scaled, zero-padded
 *   copies of Q and K (rows to multiples of MDL_RETR_ROW_BLOCK / MDL_RETR_COL_TILE, columns to a multiple of 32) and, per column
 *   chunk, two int32 counts and k 8-byte list entries per query row.  O((n + m) d + n k chunks), never O(n m).
 * col_chunks: the gallery's MDL_RETR_COL_TILE-row tiles are cut into this many equal column ranges, each streamed by its own workgroup
 *   per block of MDL_RETR_ROW_BLOCK queries (at most one chunk per tile); 0: enough of them for MDL_RETR_TARGET_WGS workgroups.
 *   No output depends on it.
 *
 * Bits depend on the two rows alone.  s_ij is one fmaf chain over the d products (zero-padded to a multiple of 32, in an order fixed
 *   by that length) of row i of Q and row j of K, each scaled by a factor computed from that row and d alone: not a function of n, m,
 *   the strides, the tile or chunk geometry or the position of either row.  Two identical gallery rows give bit-identical
 *   similarities: ties are real ties.
 * Order.  Every comparison is made on an ordered 32-bit key of the similarity: descending by value, -0 = +0, and every NaN is one
 *   key BELOW -inf, so a NaN similarity is never retrieved ahead of a number (the opposite of mdl_attn_rank's choice, deliberately:
 *   a model that emits NaN must score worst).  Ties are broken by the lower gallery index.  A total order: every output is
 *   independent of scheduling and of col_chunks.
 * paired = 1 (n <= m; the partner of query i is gallery row i):
 *   pair_sim [n] fp32   s_ii, from the same tile code as every other similarity
 *   greater  [n] int32  #{j != i : key(s_ij) before key(s_ii)}
 *   equal    [n] int32  #{j != i : key(s_ij) == key(s_ii)}
 *   A NaN s_ii gives greater = m - 1, equal = 0.  The rank of the partner is 1 + greater (optimistic) .. 1 + greater + equal.
 * k >= 1: topk_idx [n, k] int32 and topk_val [n, k] fp32, the first k gallery rows of every query in the order above with their
 *   similarities (-0 as +0, a NaN as the canonical quiet NaN); with exclude_diag = 1 (neighbours inside one cohort, Q is K) column i is
 *   skipped for row i.  Entries past the number of candidates are -1 / -inf.  k = 0 skips it.
 * Output pointers of a mode that is off may be NULL (greater / equal / pair_sim with paired = 0, topk_* with k = 0).
 * Three launches (scale, stream, finish) on the caller's stream; no allocation, no atomics, no host read, no workgroup waits on another.
 *
 * Refusals, in this order, before any launch.  MDL_E_ARG: Q, K, ws or an output of a mode that is on NULL; n, m or d < 1; ldq or
 *   ldk < d; k < 0; col_chunks < 0; an unknown metric; paired or exclude_diag not 0 / 1; both of them set; paired with n > m; neither
 *   paired nor k >= 1.  MDL_E_ALIGN: Q, K or an output not 4-byte, ws not 16-byte aligned.  MDL_E_UNSUPPORTED: n or m above
 *   MDL_RETR_MAX_ROWS, d above MDL_RETR_MAX_D, k above MDL_RETR_MAX_K, col_chunks above MDL_RETR_MAX_CHUNKS, n * ldq or m * ldk
 *   beyond 2^61.  mdl_retrieval_ws_bytes returns the same negative codes for its sizes. */
#define MDL_RETR_COSINE 0
#define MDL_RETR_DOT 1
#define MDL_RETR_MAX_ROWS 1048576
#define MDL_RETR_MAX_D 2048
#define MDL_RETR_MAX_K 64
#define MDL_RETR_MAX_CHUNKS 64
#define MDL_RETR_ROW_BLOCK 128
#define MDL_RETR_COL_TILE 128
#define MDL_RETR_TARGET_WGS 512
int64_t mdl_retrieval_ws_bytes(int64_t n, int64_t m, int64_t d, int k, int col_chunks);
int mdl_retrieval(const float* Q, int64_t ldq, const float* K, int64_t ldk, int64_t n, int64_t m, int64_t d, int metric, int paired,
                  int exclude_diag, int k, int col_chunks, int32_t* greater, int32_t* equal, float* pair_sim, int32_t* topk_idx,
                  float* topk_val, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * S1-S2 -- the survival probe: P independent ridge-penalised Cox proportional-hazards fits over one embedding matrix and, per fit,
 * Harrell's concordance index and a median-split log-rank statistic over the held-out cases (ABI 26, additive).  The reference names
 * patient stratification and prognostic prediction as uses of a slide embedding and ships no code for them; all problems of a
 * protocol (cross-validation folds x repeats x endpoints) go through one launch sequence.  The decision values between the two calls
 * come from mdl_probe_scores with C = 2 and a zero intercept: z [P, S] = X W_p^T for ALL S cases.
 *
 * X [S, d] fp32, row stride ldX >= d ELEMENTS, any d >= 1; only read.
 * time (fp32), event (int32): the vectors of problem p are time[p * ldt .. p * ldt + S) and event[p * lde .. p * lde + S); a stride of 0
 *   shares one vector among all problems (several endpoints go through one call with strides S).  event: 1 = event, 0 = censored, any
 *   other value (-1) = no follow-up: such a case is in neither the training nor the test set.
 * train_idx [P, n_max] (int32), n_train [P] (int32): problem p trains on cases train_idx[p, 0 .. n_train[p]); the rest of the row is
 *   never read.  1 <= n_train[p] <= n_max <= MDL_COX_MAX_TRAIN.  Every case with event 0 / 1 that is not a training case is a test case.
 *
 * mdl_cox_fit minimises, per problem, with Breslow ties, no intercept and the risk set R_i = {j in training : t_j >= t_i},
 *   F(w) = cost * sum_{i : event_i = 1} [ log sum_{j in R_i} exp(x_j . w) - x_i . w ] + 1/2 |w|^2
 * by Newton-CG in the span of the training rows (w = X_t^T a).  Three launches: an order kernel checks every training list and sorts it
 * by (time descending, case index ascending) -- a total order, so the result's bits do not depend on the order of the caller's list --,
 * a Gram kernel forms G = X_t X_t^T over the sorted rows in the workspace, and one workgroup per problem iterates; after the sort the
 * risk-set sums are prefix sums read at the end of a row's tie group, the sums over event times suffix sums read at its start.  The
 * decision values of every Newton step are formed from w itself, G only serves the Hessian-vector products.  No workgroup waits on
 * another; every loop is bounded (max_iter Newton steps, MDL_COX_CG_MAX CG steps each, MDL_COX_LS_MAX step halvings).
 * Stop rule, relative: with g0 the inf-norm of the primal gradient at w = 0, a problem has converged when that norm at w (evaluated in
 * fp32 from w itself) is <= gtol * g0.  The iteration aims at 0.03 gtol g0 and, once below gtol g0, goes on only while a step still
 * halves the norm; it stops after max_iter steps at the latest.  (The fp32 floor of the norm grows with cost and n; no absolute bound
 * fits all problems.)  A training list without an event has g0 = 0 and the optimum w = 0: zeros, converged = 1.
 * Range of the decision values: the exponentials are shifted by the maximum over ALL training rows, so no exp overflows; but the
 * risk-set sum of an event whose whole risk set lies more than ~87 below that maximum underflows to 0 in fp32.  Along the line search
 * that only halves the step; at an accepted iterate it ends the fit with a NaN residual and converged = 0 (never a wrong result reported
 * as converged).  Decision values of a ridge fit on embeddings span a few units, far from it; there is no per-risk-set shift.
 * W_out [P, d]; thr_out [P]: the median of the training rows' final decision values (the mean of the two middle values for even n,
 * in fp32) -- formed in the summation order of mdl_probe_scores, so it is the median of that call's z over the training rows bit for bit;
 * info_out [P, 4] fp32: Newton steps taken, converged (1 / 0), the final inf-norm of the gradient (absolute), CG steps in all.
 * A problem is refused -- NaN in its W, threshold and residual, converged = 0, the others unaffected -- when n_train is outside
 * [1, n_max], a training index is outside [0, S) or repeated, a training case has an event other than 0 / 1 or a time that is NaN,
 * infinite or negative.  Results depend on the problem alone (not on P, p, n_max or the order of its list).
 *
 * mdl_surv_metrics, over the test cases of problem p, from z [P, S] and thr [P] (only read).  Here n_train[p] = 0 is legal too (no
 * training list: every case with follow-up is a test case); a value outside [0, n_max] is clamped into it, and training indices
 * outside [0, S) are passed over:
 *   concordance: the pair (i, j) is comparable iff event_i = 1 and (t_i < t_j, or t_i = t_j and event_j = 0); it counts 2 if z_i > z_j,
 *     1 if z_i = z_j.  c_index_out [P] fp64 = count / (2 comparable), NaN without a comparable pair.
 *   stratification: a test case is high risk iff z > thr[p].  With, per test event case i, n_i = #{test j : t_j >= t_i}, h_i the same
 *     count inside the high group and d_i = #{test events j : t_j = t_i}:  O - E = sum_i [1(i high) - h_i / n_i],
 *     V = sum_{i : n_i > 1} (h_i / n_i)(1 - h_i / n_i)(n_i - d_i) / (n_i - 1) -- the log-rank sums over distinct event times, written
 *     per individual -- and chi2_out [P] fp64 = (O - E)^2 / V, NaN when V = 0.  One degree of freedom: p = erfc(sqrt(chi2 / 2)).
 *   counts_out [P, 6] int32: concordance numerator, comparable pairs, test cases, high-group size, events in the low group, events in
 *     the high group.
 *   All counting is exact, in integers (S <= MDL_PROBE_MAX_CASES keeps every count inside int32); one integer atomic per workgroup, whose
 *   order cannot change a bit.  The two sums run in double in a fixed order.  A NaN thr[p] (a refused fit) gives NaN in both doubles.
 *   c_index_out and chi2_out are fp64 arrays (the header has no double), 8-byte aligned.
 *
 * Workspaces: 16-byte aligned, sizes from the *_ws_bytes queries, contents need no initialisation.
 * MDL_E_UNSUPPORTED: n_max > MDL_COX_MAX_TRAIN, S > MDL_PROBE_MAX_CASES (metrics), a launch grid or an output index beyond int32.
 * MDL_E_ARG: null pointers, ldX < d, sizes < 1, ldt / lde not 0 or >= S, max_iter < 0, cost <= 0, gtol < 0.  MDL_E_ALIGN: ws not
 * 16-byte, c_index_out / chi2_out not 8-byte aligned.  All of it is checked before anything is launched, in the three steps of P1-P3:
 * (1) every MDL_E_ARG, (2) every MDL_E_UNSUPPORTED, the int32 bounds of the launch grids included, (3) MDL_E_ALIGN. */
#define MDL_COX_MAX_TRAIN 1024
#define MDL_COX_CG_MAX 400
#define MDL_COX_LS_MAX 24
int64_t mdl_cox_order_fit_ws_bytes(int64_t P, int n_max, int d);
int mdl_cox_fit(const float* X, int64_t ldX, int64_t S, int d, const float* time, int64_t ldt, const int32_t* event, int64_t lde,
                const int32_t* train_idx, const int32_t* n_train, int64_t P, int n_max, float cost, float gtol, int max_iter,
                float* W_out, float* thr_out, float* info_out, void* ws, void* stream);
int64_t mdl_surv_metrics_ws_bytes(int64_t P, int64_t S);
int mdl_surv_metrics(const float* z, const float* time, int64_t ldt, const int32_t* event, int64_t lde, const int32_t* train_idx,
                     const int32_t* n_train, int64_t P, int n_max, int64_t S, const float* thr, void* c_index_out, void* chi2_out,
                     int32_t* counts_out, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADELEINE_AMD_H */
