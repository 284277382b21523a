/*
 * madeleine_amd_regress.h -- the regression probe of libmadeleine_amd.so (gfx950 / MI355X): batched ridge fits of continuous targets
 * on slide embeddings, and Pearson, Spearman, R^2, MAE and RMSE over every fit's held-out cases.  A fifth header of the same library,
 * the same conventions and the same strict grammar (madeleine_amd.h, top): extern "C", plain pointers and sizes, device pointers,
 * caller-allocated buffers, asynchronous launches on the caller's stream, 0 / positive hipError_t / negative MDL_E_* as the return
 * value.  It declares entry points only; the MDL_E_* codes, MDL_ABI_VERSION and MDL_PROBE_MAX_CASES are those of madeleine_amd.h, and
 * adding to THIS header does not change that revision: a binding checks every name below against the loaded library by itself.
 *
 * Inputs (P1-P3 of madeleine_amd.h for X and the problem table):
 *   X         [S, d] float, row stride ldX >= d.
 *   train_idx [P, n_max] int32, n_train [P] int32: the training cases of problem p are train_idx[p, 0 .. n_train[p] - 1].  An index may
 *             repeat: the case then counts as often as it is listed.
 *   Y         [S, T] float, row stride ldY >= T, shared by all problems of a call.  A NaN is "no value".
 *   alphas    [A] float ON THE HOST, read before the call returns.  Every alpha must be finite and > 0.
 * A case i is a TEST case of (p, t) when Y[i, t] is finite and i is not in row p of train_idx.
 *
 * R1 -- mdl_ridge_fit.  For every (problem p, penalty a, target t) the minimiser of
 *     sum_i (y_it - w . x_i - b)^2 + alpha_a |w|^2        over the training rows of p, the intercept b unpenalised
 * (scikit-learn's Ridge(alpha)).  W_out [P, A, T, d] and b_out [P, A, T] float; info_out [P, A, 2] float: [0] 1 when the factorisation
 * succeeded, else 0; [1] the smallest pivot over the largest diagonal entry of the factorised matrix.
 *   Method, all in double from the widened float rows: the training means of X (per column, rows in list order) and of each target;
 *   the system K = Xc Xc^T (n x n, the Gram form) when n_train[p] <= d, else K = Xc^T Xc (d x d, the covariance form), Xc the centred
 *   rows -- the form is a function of n_train[p] and d alone.  Each entry of K is one FMA chain in ascending order of the summed index.
 *   Per (p, a): K + alpha I = L L^T by a right-looking blocked Cholesky (panels of 32 columns), one workgroup per factorisation.  Then
 *   L L^T c = r for every target, r = y - ybar (Gram form; W = Xc^T c, a chain in list order) or r = Xc^T (y - ybar) (covariance form;
 *   W = c, a chain in list order).  b = ybar - xbar . W with W before its rounding to float.  No atomics; no workgroup waits on
 *   another; the bits of a (p, a, t) result depend on that problem's rows, alpha_a and column t of Y alone -- not on P, p, n_max, T or A.
 *   Failures, each touching its own outputs only: a NaN among the training targets of (p, t) -> W, b of (p, ., t) NaN; n_train[p] outside
 *   [1, n_max] or an index outside [0, S) -> W, b of p NaN and info = {0, NaN}; a pivot that is not > 0 -> W, b of (p, a) NaN, info[0] = 0.
 *   n_train[p] = 1 is valid: W = 0, b = y.
 *   Limits: min(n_max, d) <= MDL_RIDGE_MAX_SYS, n_max <= MDL_RIDGE_MAX_TRAIN, T <= MDL_RIDGE_MAX_TARGETS, A <= MDL_RIDGE_MAX_ALPHAS,
 *   P * A <= 65535.
 *   ws: mdl_ridge_fit_ws_bytes(P, n_max, d, T, A) bytes.
 *
 * R2 -- mdl_ridge_scores.  Z [P, A, T, S] float, Z[p, a, t, i] = x_i . W[p, a, t] + b[p, a, t]: one float FMA chain from 0 over
 * k = 0 .. d - 1, then one addition of b.  Every (p, a, t) list is contiguous.  W is read as L = P * A * T rows; no workspace.
 *
 * R3 -- mdl_regress_metrics.  Over the test cases of (p, t), for every a: metrics_out [P, A, T, 6] double,
 *   MDL_REG_NTEST the number of test cases; MDL_REG_PEARSON r from two-pass sums in double; MDL_REG_SPEARMAN rho; MDL_REG_R2
 *   1 - sum (y - z)^2 / sum (y - ybar_test)^2; MDL_REG_MAE; MDL_REG_RMSE.
 *   n_test < 2: NaN for all but n_test.  All y of the test cases equal: r, rho and R^2 NaN; all z equal: r and rho NaN.  A NaN among
 *   the test cases' z: NaN for all but n_test.
 *   Spearman from exact integers: R_i = 2 #less + #equal + 1 among the test cases (#equal counts the case itself; -0 = +0), for z and
 *   for y (the y ranks once per (p, t)).  sums_out [P, A, T, 6] int64, may be NULL: n, sum Rz, sum Ry, sum Rz^2, sum Ry^2, sum Rz Ry;
 *   rho = (n sum Rz Ry - sum Rz sum Ry) / sqrt((n sum Rz^2 - (sum Rz)^2) (n sum Ry^2 - (sum Ry)^2)), the three differences exact in
 *   int64 (S <= MDL_PROBE_MAX_CASES).  The double sums: thread i of 256 adds its cases i, i + 256, .. in that order, then a fixed tree.
 *   ws: mdl_regress_metrics_ws_bytes(P, S, T) bytes.
 *
 * Workspaces are 16-byte aligned and need no initialisation.
 *
 * Refusals, in this order, all before any launch and before any device pointer is touched (csrc/probe_host.hpp: probe_check, for all
 * three entry points and both queries).
 *   (1) MDL_E_ARG: a NULL pointer (sums_out may be NULL); P, n_max, S, d, T or A < 1; ldX < d; ldY < T; one of the A alphas not finite or not > 0
 *       (all A are read, also where A is beyond the limit).
 *   (2) MDL_E_UNSUPPORTED: the limits above; S > MDL_PROBE_MAX_CASES (R3); P, S, P * n_max, a launch grid or a row count beyond int32.
 *   (3) MDL_E_ALIGN: ws not 16-byte aligned; metrics_out or sums_out not 8-byte aligned; any other pointer not 4-byte aligned.
 * The *_ws_bytes queries return the byte count, or the codes of (1) and (2) for their sizes.
 */
#ifndef MADELEINE_AMD_REGRESS_H
#define MADELEINE_AMD_REGRESS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_RIDGE_MAX_SYS 1024
#define MDL_RIDGE_MAX_TRAIN 16384
#define MDL_RIDGE_MAX_TARGETS 4096
#define MDL_RIDGE_MAX_ALPHAS 16
#define MDL_REG_NTEST 0
#define MDL_REG_PEARSON 1
#define MDL_REG_SPEARMAN 2
#define MDL_REG_R2 3
#define MDL_REG_MAE 4
#define MDL_REG_RMSE 5
int64_t mdl_ridge_fit_ws_bytes(int64_t P, int n_max, int d, int64_t T, int A);
int mdl_ridge_fit(const float* X, int64_t ldX, int64_t S, int d, const float* Y, int64_t ldY, int64_t T, const int32_t* train_idx,
                  const int32_t* n_train, int64_t P, int n_max, const float* alphas, int A, float* W_out, float* b_out, float* info_out,
                  void* ws, void* stream);
int mdl_ridge_scores(const float* X, int64_t ldX, int64_t S, int d, const float* W, const float* b, int64_t L, float* Z, void* stream);
int64_t mdl_regress_metrics_ws_bytes(int64_t P, int64_t S, int64_t T);
int mdl_regress_metrics(const float* Z, const float* Y, int64_t ldY, int64_t T, const int32_t* train_idx, const int32_t* n_train,
                        int64_t P, int n_max, int64_t S, int A, void* metrics_out, int64_t* sums_out, void* ws, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MADELEINE_AMD_REGRESS_H */
