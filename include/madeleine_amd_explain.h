/*
 * madeleine_amd_explain.h -- the explaining side of libmadeleine_amd.so (gfx950 / MI355X): which patches made a linear probe's decision.
 * A fourth header of the same library, the same conventions and the same strict grammar (madeleine_amd.h, top): extern "C", plain
 * pointers and sizes, device pointers, caller-allocated buffers, asynchronous launches on the caller's stream, 0 / positive hipError_t /
 * negative MDL_E_* as the return value.  It declares entry points only; the MDL_E_* codes, MDL_ABI_VERSION, MDL_HIDDEN and the probes'
 * class range are those of madeleine_amd.h, and adding to THIS header does not change that revision: a binding checks every name below
 * against the loaded library by itself.
 *
 * The identity.  The slide embedding is linear in the attention-weighted token embeddings (pooled = sum_t a[t] E[t], one Linear P on
 * top) and every probe of madeleine_amd.h is linear, so a decision value z_c = w_c . (P pooled + b_P) + b_c is, exactly,
 *     z_c = sum_t sum_h a[t, h] <U[c, h, :], E[t, h, :]> + (w_c . b_P + b_c)        U[c] = P_hm^T w_c
 * with P_hm the projector's weight with head-major columns.  X1 computes the terms, X2 sums them per bag.
 *
 * X1 -- mdl_attn_contrib.  W is the width of a head and must be MDL_HIDDEN.
 *   E        [T, H * W] head-major token embeddings, row stride ldE elements: (T - 1) * ldE + H * W elements.  e_dtype MDL_CONTRIB_E_F32:
 *            float; MDL_CONTRIB_E_BF16: bfloat16 (uint16 storage), widened exactly.
 *   attn     [T, H] float, row stride ldA: (T - 1) * ldA + H elements.
 *   U        [C, H * W] float, contiguous: C * H * W elements.
 *   per_head [T, H, C] float, contiguous: T * H * C elements; may be NULL.   per_head[t, h, c] = attn[t, h] * dot(t, h, c)
 *   total    [T, C] float, row stride ldO: (T - 1) * ldO + C elements; only the first C columns of a row are written.
 *            total[t, c] = ((per_head[t, 0, c] + per_head[t, 1, c]) + ...) + per_head[t, H - 1, c]: heads in ascending order.
 *   H in {1, 2, 4, 8}, 1 <= C <= MDL_CONTRIB_MAX_C.
 * Summation order of dot(t, h, c) = sum_e U[c, h W + e] E[t, h W + e], fixed.  A wave of 64 lanes owns one (row, head).  Lane l holds 8
 * elements: fp32 E: e = 4 l + j and 256 + 4 l + j (j = 0..3); bf16 E: e = 8 l + j (j = 0..7).  Its partial is the FMA chain
 * p = fma(E_e, U_e, p) from p = 0 over its elements in ascending e.  The 64 partials are added as the balanced binary tree over the lanes
 * in lane order: lanes 2 m and 2 m + 1 first, then the pairs (4 m, 4 m + 2), and so on up to the two halves of the wave.  The product
 * with attn[t, h] is one more fp32 rounding.
 * Row-local: the bits of row t depend on row t of E and attn, on U and on (H, C, e_dtype) alone -- not on T, the row's position, the
 * strides or the rest of the call; a NaN or Inf in row t reaches row t only.  No atomics, no workspace, one launch
 * (csrc/contrib.hip: ac_kernel; plain FMAs, two columns to a packed instruction, U in registers, E read once with 16-byte loads).
 *
 * X2 -- mdl_contrib_stats.  contrib [T, C] float, row stride ld >= C: (T - 1) * ld + C elements; cu [R + 1] int64: bag r is rows
 * cu[r] .. cu[r + 1] - 1 (a bag that is not inside [0, T] or runs backwards is an empty bag).  stats [R, 4, C] float, per bag and
 * column: MDL_CONTRIB_SUM the sum, MDL_CONTRIB_POS the sum of the positive terms, MDL_CONTRIB_NEG the sum of the negative terms,
 * MDL_CONTRIB_ABSMAX max |.|.  An empty bag gives zeros.
 *   Order: a bag is cut into chunks of MDL_CONTRIB_ROWS rows.  In a chunk, thread i of 256 adds rows i, 256 + i, 512 + i, 768 + i of the
 *   chunk in that order (a row past the bag's end adds +0), the 64 threads of a wave are added by xor butterflies of distance 32, 16, ..,
 *   1, the four waves as (w0 + w1) + (w2 + w3); the chunks of a bag are then added in ascending order by one thread.  No atomics; a
 *   bag's bits depend on the bag alone.
 *   NaN: a term belongs to the positive sum when its sign bit is clear and to the negative sum when it is set (the other sum gets +0
 *   for it), so a NaN reaches the sum, max |.| (which is NaN as soon as one term is) and the one signed sum its sign bit names.
 *   ws: mdl_contrib_stats_ws_bytes(T, R, C) bytes, 16-byte aligned, needs no initialisation.
 *
 * Refusals, in this order, all before any launch and before any device pointer is touched.
 *   (1) MDL_E_ARG: a NULL pointer (X1: E, attn and total may be NULL when T == 0, per_head in every call; X2: contrib when T == 0); a negative
 *       size; ldE < H * W, ldA < H, ldO < C, ld < C; e_dtype neither 0 nor 1; C < 1; H < 1; W < 1.
 *   (2) MDL_E_UNSUPPORTED: H outside {1, 2, 4, 8}, W != MDL_HIDDEN, C > MDL_CONTRIB_MAX_C; T or R or a launch grid beyond int32.
 *   (3) MDL_E_ALIGN: E or U not 16-byte aligned, ldE not a multiple of 4 (fp32) / 8 (bf16) elements; attn, per_head, total, contrib or
 *       stats not 4-byte aligned; cu not 8-byte aligned; ws not 16-byte aligned.
 * T == 0 or R == 0 returns MDL_OK with nothing launched.  mdl_contrib_stats_ws_bytes returns the byte count, or the codes of (1) and (2)
 * for its sizes.
 */
#ifndef MADELEINE_AMD_EXPLAIN_H
#define MADELEINE_AMD_EXPLAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_CONTRIB_MAX_C 8
#define MDL_CONTRIB_E_F32 0
#define MDL_CONTRIB_E_BF16 1
#define MDL_CONTRIB_ROWS 1024
#define MDL_CONTRIB_SUM 0
#define MDL_CONTRIB_POS 1
#define MDL_CONTRIB_NEG 2
#define MDL_CONTRIB_ABSMAX 3
int mdl_attn_contrib(const void* E, int64_t ldE, int e_dtype, const float* attn, int64_t ldA, const float* U, int64_t T, int H, int W,
                     int C, float* per_head, float* total, int64_t ldO, void* stream);
int64_t mdl_contrib_stats_ws_bytes(int64_t T, int64_t R, int C);
int mdl_contrib_stats(const float* contrib, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int C, float* stats, void* ws,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MADELEINE_AMD_EXPLAIN_H */
