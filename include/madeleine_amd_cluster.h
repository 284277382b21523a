/*
 * madeleine_amd_cluster.h -- morphological prototypes of libmadeleine_amd.so (gfx950 / MI355X): Lloyd's k-means with k-means++ seeding
 * over the rows of a device-resident feature store, read where they lie, and the per-bag histogram of the labels.  A sixth header of
 * the same library, the same conventions and the same strict grammar (madeleine_amd.h, top): extern "C", plain pointers and sizes,
 * device pointers, caller-allocated buffers, asynchronous launches on the caller's stream, 0 / positive hipError_t / negative MDL_E_*
 * as the return value.  It declares entry points only; the MDL_E_* codes, MDL_STORE_* and MDL_ABI_VERSION are those of madeleine_amd.h,
 * and adding to THIS header does not change that revision: a binding checks every name below against the loaded library by itself.
 *
 * The row source (K1-K3), S5's of madeleine_amd.h with one more table:
 *   store, dtype, row_stride, T_total, off [n_bags + 1], n_bags, bag [R]: as in S1 (resident tier only); fp16 / bf16 rows are widened
 *     exactly.  bag[r] == -1, a bag index outside [0, n_bags), an empty bag and a bag that leaves [0, T_total) contribute no rows.
 *   cu [R + 1] (int64, device): the prefix of the listed bags' lengths, cu[0] = 0, cu[R] = T.  Row i of bag bag[r] has CALL POSITION
 *     cu[r] + i: labels, dist and the seeds' positions are indexed by it.  T < 2^31.
 *   chunk_cu [R + 1] (int64, device; K1, K3): the prefix sum of ceil(n_r / MDL_KM_ROWS), n_r the rows of bag[r] (0 where it contributes
 *     none), chunk_cu[0] = 0; n_chunks = chunk_cu[R].  A chunk never straddles bags.
 *   A dense [T, D] matrix is the one-bag case: off = {0, T}, bag = {0}, cu = {0, T}, chunk_cu = {0, ceil(T / MDL_KM_ROWS)}.
 *   Bounds (S1's rule).  With inconsistent tables nothing outside the store is read and nothing outside the outputs is written: a bag
 *   whose positions cu[r] .. cu[r] + n_r - 1 leave [0, T), and a (bag, chunk) that chunk_cu and off do not agree on, is passed over.
 *
 * K1 -- mdl_kmeans_assign.  C [k, D] float, dense.  For every row t and centroid j
 *       v_tj = x_t . c_j - hn_j,      hn_j = 0.5 |c_j|^2
 *   x_t . c_j is ONE float fmaf chain from 0 on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) over the columns 0 .. dp - 1, dp = D
 *   rounded up to 32, in an order fixed by dp (within every 8: 0, 4, 1, 5, 2, 6, 3, 7; the zero padding leaves the value as it is);
 *   hn_j is a fmaf chain per lane of a wave (columns lane, lane + 64, ..), the xor butterfly and one halving; then one subtraction.
 *   Centroids are zero-padded into ws once per call; row tiles of MDL_KM_ROWS rows are read from the store in place; [T, k] is never
 *   written.
 *     labels [T] int32, IN and OUT: the argmax over j of v_tj (a NaN v counts as -inf), ties to the LOWEST j.
 *     dist   [T] float: |x_t|^2 - 2 v_{t, label}, |x_t|^2 a fmaf chain per 4 adjacent columns of every 32 and a fixed tree over the 8.
 *     stats  16 bytes, 8-byte aligned: [0] int64, the rows whose label differs from the one labels held on entry; [1] double, the
 *            inertia, sum of max(dist, 0): per-chunk double partials (a fixed tree over the chunk's rows) added in chunk order.
 *   A row with any non-finite element gets label -1 and dist NaN and takes no part in the count or the inertia.
 *   Bit contract: the bits of labels[t] and dist[t] depend on row t (its values, widened) and on C alone -- not on R, the other rows,
 *   row_stride, the chunk the row falls in or the store dtype beyond the exact widening.  No atomics.
 *   ws: mdl_kmeans_assign_ws_bytes(n_chunks, k, D): the padded centroids (k to 128, D to 32) and half-norms, 12 bytes per chunk.
 *
 * K2 -- mdl_kmeans_update.  C_out [k, D] float and counts [k] int64 from labels [T] (a label outside [0, k) belongs nowhere).
 *   A stable counting sort of the call positions by label, integers only: histograms per MDL_KM_SORT_ROWS positions (integer LDS
 *   counters), an exclusive scan over (label, chunk), a scatter that keeps ascending position inside a label.  Then the mean of every
 *   cluster's member rows in S5's scheme over its member list: one workgroup per MDL_KM_MEAN_ROWS members, a thread owns 8 adjacent
 *   columns in one of G row groups, G = 256 / min(256, next_pow2(ceil(D / 8))), and adds members grp, grp + G, .. of the chunk in that
 *   order in float; the G sums are added in group order; the chunks' partials are added in chunk order in DOUBLE, divided by the count
 *   in double and rounded to float once.  A cluster with no member keeps C_in[j] and reports count 0.  C_out may be C_in.
 *   Bit contract: the bits of C_out[j] depend on the member rows of j and their order alone.  No atomics on floats.
 *   Addition depth: an element of a cluster of len members has passed through at most
 *       h(len) = ceil(min(len, MDL_KM_MEAN_ROWS) / G) + (G - 1) + (ceil(len / MDL_KM_MEAN_ROWS) - 1)
 *   additions (the last term's in double).
 *   ws: mdl_kmeans_update_ws_bytes(T, k, D).
 *
 * K3 -- mdl_kmeans_seed.  k-means++ from u [k] doubles in [0, 1) on the device.  A row is FINITE when all its elements are; T_finite
 *   is their number.  Centre 0 is the finite row of rank floor(u[0] * T_finite) in call order.  For j >= 1: mind[t] is the minimum over
 *   the centres chosen so far of the float squared distance sum_i (x_ti - c_i)^2 (a fmaf chain per lane over columns lane, lane + 64, ..
 *   and the xor butterfly), 0 for a non-finite row; the double sums of mind per chunk (a fixed tree), per slice of ceil(n_chunks / 256)
 *   chunks (in chunk order) and their total (in slice order); centre j is the first call position whose inclusive double prefix (slices,
 *   then chunks, then rows, each in order) exceeds u[j] * total, and the finite row of rank floor(u[j] * T_finite) when total is 0.
 *   Two launches per centre, no host read.  pos_out [k] int64: the chosen call positions (-1 when there is no finite row);
 *   C_out [k, D]: those rows, widened.  T < k is MDL_E_ARG.
 *   ws: mdl_kmeans_seed_ws_bytes(n_chunks, T).
 *
 * K4 -- mdl_kmeans_hist.  counts [R, k] int32: counts[r, j] is the number of call positions cu[r] <= t < cu[r + 1] (inside [0, T))
 *   with labels[t] == j; a label outside [0, k) -- -1 included -- is counted nowhere.  Integer LDS counters.  No workspace
 *   (mdl_kmeans_hist_ws_bytes is 0).
 *
 * Refusals, all before any launch and before any device pointer is touched (csrc/kmeans.hip: km_check, for every entry point and query).
 *   (1) MDL_E_ARG: a NULL pointer; R, n_chunks, T_total or n_bags < 0; T < 1; D < 1; k < 1; row_stride < D; an unknown dtype; T < k (K3).
 *   (2) MDL_E_UNSUPPORTED: k > MDL_KM_MAX_K; R, T or n_chunks beyond int32.
 *   (3) MDL_E_ALIGN: store, C, C_in, C_out or ws not 16-byte aligned; off, cu, chunk_cu, counts (K2), pos_out, u or stats not 8-byte
 *       aligned; any other pointer not 4-byte aligned.
 * The *_ws_bytes queries return the byte count, or the codes of (1) and (2) for their sizes.  Workspaces need no initialisation.
 */
#ifndef MADELEINE_AMD_CLUSTER_H
#define MADELEINE_AMD_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_KM_MAX_K 1024
#define MDL_KM_ROWS 128
#define MDL_KM_SORT_ROWS 2048
#define MDL_KM_MEAN_ROWS 1024
int64_t mdl_kmeans_assign_ws_bytes(int64_t n_chunks, int k, int D);
int mdl_kmeans_assign(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                      const int32_t* bag, const int64_t* cu, const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int64_t T, int D,
                      const float* C, int k, int32_t* labels, float* dist, void* stats, void* ws, void* stream);
int64_t mdl_kmeans_update_ws_bytes(int64_t T, int k, int D);
int mdl_kmeans_update(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                      const int32_t* bag, const int64_t* cu, int64_t R, int64_t T, int D, const int32_t* labels, const float* C_in, int k,
                      float* C_out, int64_t* counts, void* ws, void* stream);
int64_t mdl_kmeans_seed_ws_bytes(int64_t n_chunks, int64_t T);
int mdl_kmeans_seed(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                    const int32_t* bag, const int64_t* cu, const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int64_t T, int D,
                    const void* u, int k, int64_t* pos_out, float* C_out, void* ws, void* stream);
int64_t mdl_kmeans_hist_ws_bytes(int64_t R, int k);
int mdl_kmeans_hist(const int32_t* labels, const int64_t* cu, int64_t R, int64_t T, int k, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MADELEINE_AMD_CLUSTER_H */
