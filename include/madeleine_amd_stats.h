/*
 * madeleine_amd_stats.h -- the statistics side of libmadeleine_amd.so (gfx950 / MI355X): what turns the decision values of the probes
 * of madeleine_amd.h into confidence intervals and paired comparisons.  A third header of the same library, the same conventions and
 * the same strict grammar (madeleine_amd.h, top): extern "C", plain pointers and sizes, device pointers, caller-allocated buffers,
 * asynchronous launches on the caller's stream, 0 / positive hipError_t / negative MDL_E_* as the return value.  It declares entry
 * points only; the MDL_E_* codes, MDL_ABI_VERSION and the MDL_PROBE_* / MDL_LOGIT_* / MDL_COX_* limits are those of madeleine_amd.h,
 * and adding to THIS header does not change that revision: a binding checks every name below against the loaded library by itself.
 *
 * B1-B3 -- the test-set bootstrap of the probes' metrics.  The cohort's S cases are resampled R times with replacement; every problem
 * (fold, arm, task) recomputes its counts under the resample of its GROUP, so that all problems of one group see the same resample:
 * differences between arms and means over folds are paired by construction.  The contract is EXACT INTEGER ARITHMETIC: a numpy model
 * (tests/_resample_ref.py) equals the device bit for bit, and the bits of a (problem, replicate) depend on that problem's rows, its
 * group, seed, r and S alone -- not on P, p, n_max, R or how the replicates are spread over workgroups.
 *
 * Weights.  The weight vector of replicate r of group g is the count vector of S draws from [0, S), a function of (seed, g, r, S).
 * With mix32 of the dropout counter hash (x ^= x >> 16; x = lo24(x) * 0x58E58A + x; x ^= x >> 13; x = lo24(x) * 0xCA6D40 + x;
 * x ^= x >> 16), key(seed) = lo32((seed * 0x9E3779B97F4A7C15) >> 32) ^ lo32(seed) and all arithmetic mod 2^32:
 *     a      = mix32(key(seed) ^ lo32(g * 0x9E3779B9))                 g: the int32 group id, taken mod 2^32
 *     b      = mix32(a + r)                                            r = 1 .. R
 *     h_j    = mix32(mix32(b ^ j) + lo32(j * 0x9E3779B9))              j = 0 .. S - 1
 *     draw_j = (h_j * S) >> 32                                         a 64-bit product
 *     w[s]   = #{j : draw_j == s}
 * Replicate 0 is the sample itself: w = 1 everywhere.  Two rounds of mix32 per draw: with one the counts are under-dispersed (variance
 * 0.992-0.997 where 1 - 1/S is expected; two rounds: 0.9987-1.0011 at S = 1100).  The multiply-high map sends floor(2^32 / S) or that
 * plus one hash values to each index: a bias of at most S / 2^32 per index (3.8e-6 at S = 16384), left as it is.
 *
 * mdl_boot_weights (B1) writes w_out [G, R + 1, S] uint16 for the groups group[0 .. G): for tests and for users who resample on their
 * own.  S <= MDL_PROBE_MAX_CASES, so a count fits 16 bits.
 *
 * mdl_boot_class_counts (B2).  z [P, S, cols] fp32, y, ldy, train_idx [P, n_max], n_train [P], P, n_max, S, C mean what they mean for
 * mdl_probe_metrics / mdl_logit_metrics (n_max <= MDL_LOGIT_MAX_TRAIN, S <= MDL_PROBE_MAX_CASES), and the test-set rule, the
 * prediction rule and the scores are exactly theirs: a labeled case outside the training list is a test case, the prediction is z > 0
 * (C == 2) or the first maximum, the score of class c is z (C == 2, class 1) or the fp64 log_softmax(z)[c] (C > 2, one-vs-rest).
 * group [P] int32: the group of every problem.  Per problem p and replicate r, with w the weights of (seed, group[p], r, S):
 *   confusion_out [P, R + 1, C, C] int32: cell (t, q) = sum of w over the test cases of truth t and prediction q.
 *   auc_num_out [P, R + 1, cols] int64 (cols = 1 for C == 2, class 1; else one per class):
 *       sum over test cases i in the class and j outside it of w_i w_j (2 [s_i > s_j] + [s_i == s_j]),
 *     so that the weighted AUC of the class is num / (2 pos neg) with pos and neg from the row sums of the confusion matrix.  Replicate
 *     0 gives the confusion matrix and the pair counts of mdl_probe_metrics.  A problem whose test scores hold a NaN has -1 in all its
 *     auc_num_out entries; its confusion counts are written as usual.
 * Kernels (csrc/resample.hip): boot_prepare (a workgroup per problem: test class and prediction of every case, fp64 scores, test-set
 * size, NaN flag), boot_rank (O(S^2) counting once per problem and class: every test case's position in the total order (score, case
 * index) -- -0 == +0 -- with the bounds of its tie group), boot_class (a workgroup per problem and MDL_BOOT_REP_BLOCK replicates: the
 * S draws as integer LDS atomics on uint16 pairs, the weighted confusion, per class a workgroup prefix sum of the outside weights along
 * the order and, per case of the class, w (2 below + tied)).  The weights never reach global memory.  Integer sums only, no float
 * atomics, no workgroup waits on another, every loop is bounded by an argument or a constant.  LDS: 4 ceil(S / 2) + 4 ceil((S + 1) / 2)
 * bytes of dynamic LDS; the launcher raises the kernel's limit above 48 KiB, i.e. from S = 12288 on.
 *
 * mdl_boot_surv_counts (B3).  z [P, S], time, ldt, event, lde, train_idx, n_train, P, n_max, S mean what they mean for mdl_surv_metrics
 * (n_max <= MDL_COX_MAX_TRAIN; n_train = 0 is legal), and comparability, the 2 / 1 scoring and the test-set rule are its own.
 *   counts_out [P, R + 1, 2] int64: sum over ordered pairs of test cases (i, j) of w_i w_j [comparable(i, j)] (2 [z_i > z_j] +
 *     [z_i == z_j]), and the same sum of w_i w_j [comparable(i, j)].  A case drawn twice pairs with its own copy under the same rule:
 *     equal times and both events (or no event), so never comparable.  Replicate 0 equals counts_out[:, 0:2] of mdl_surv_metrics.
 * Pairs are counted per replicate (a workgroup per problem and MDL_BOOT_REP_BLOCK replicates, the problem's cases in LDS), which caps
 * the cohort: the test set is known on the device only, so the cap is on its bound S <= MDL_BOOT_SURV_MAX_TEST.  No workspace.
 *
 * Refusals, in this order, all before any launch and before any device pointer is touched (the order of every entry point that takes
 * a problem list: P1-P3 of madeleine_amd.h state it for the probes).
 *   (1) MDL_E_ARG: a NULL pointer; G, P, n_max or S < 1; R < 0; ldy / ldt / lde neither 0 nor >= S.
 *   (2) MDL_E_UNSUPPORTED: S > MDL_PROBE_MAX_CASES (B3: S > MDL_BOOT_SURV_MAX_TEST); n_max > MDL_LOGIT_MAX_TRAIN (B3: MDL_COX_MAX_TRAIN);
 *       C outside [2, MDL_PROBE_MAX_CLASSES]; G, P, P * n_max, R + 1 or a launch grid beyond int32.  Within these limits no count can
 *       leave its type: a confusion cell is at most S, a numerator at most 2 S^2 < 2^30, and every index is formed in 64 bits.
 *   (3) MDL_E_ALIGN: ws not 16-byte aligned; auc_num_out / counts_out not 8-byte, w_out not 2-byte, another array not 4-byte aligned.
 * R == 0 is legal and gives replicate 0 alone.  mdl_boot_class_ws_bytes returns the byte count, or the codes of (1) and (2) for its
 * sizes; the workspace needs no initialisation.
 */
#ifndef MADELEINE_AMD_STATS_H
#define MADELEINE_AMD_STATS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_BOOT_REP_BLOCK 8
#define MDL_BOOT_SURV_MAX_TEST 4096
#define MDL_BOOT_LDS_RAISE_FROM 12288
int mdl_boot_weights(uint64_t seed, const int32_t* group, int64_t G, int64_t R, int64_t S, uint16_t* w_out, void* stream);
int64_t mdl_boot_class_ws_bytes(int64_t P, int64_t S, int C);
int mdl_boot_class_counts(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train, int64_t P,
                          int n_max, int64_t S, int C, const int32_t* group, uint64_t seed, int64_t R, int32_t* confusion_out,
                          int64_t* auc_num_out, void* ws, void* stream);
int mdl_boot_surv_counts(const float* z, const float* time, int64_t ldt, const int32_t* event, int64_t lde, const int32_t* train_idx,
                         const int32_t* n_train, int64_t P, int n_max, int64_t S, const int32_t* group, uint64_t seed, int64_t R,
                         int64_t* counts_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MADELEINE_AMD_STATS_H */
