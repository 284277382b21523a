// probe_common.hpp -- the device code that the probes (probe.hip, probe_primal.hip, survival.hip) and their bootstrap (resample.hip)
// share: the sizes derived from the class count, the CG constants, the workgroup reductions, the loss of one training row, the Gram tile
// product, the test-set rule and the prediction of a case.  Every helper is inlined into kernels that keep their names, signatures and
// launch geometry; what the metrics and their bootstrap must agree on bit for bit (test class, prediction, fp64 scores) is here once.
#pragma once
#include "common.hpp"

namespace mdl {

constexpr int PROBE_CMAX = MDL_PROBE_MAX_CLASSES;
constexpr float PROBE_CG_TOL2 = 1e-4f;     // CG stops at |residual|^2 <= 1e-4 |rhs|^2 (forcing term 1e-2)
constexpr float PROBE_TIGHT = 0.03f;       // a Newton iteration aims at PROBE_TIGHT * gtol; `converged` reports the residual against gtol
constexpr int GRAM_TILE = 64;              // Gram tile
constexpr int GRAM_KC = 32;                // Gram k-chunk

__host__ __device__ __forceinline__ int cols_of(int C) { return C == 2 ? 1 : C; }                         // decision values per case
__host__ __device__ constexpr int nc_of(int cols) { return cols == 1 ? 1 : (cols <= 4 ? 4 : 8); }         // columns a kernel is built for
__host__ __device__ __forceinline__ int64_t s16_of(int64_t S) { return (S + 15) / 16 * 16; }              // a row of per-case bytes

// ---- workgroup reductions ---------------------------------------------------------------------------------------------------------
// Sum of K per-thread values over the WAVES waves of the workgroup in one fixed order (xor butterflies, then the waves as a balanced
// tree: (0 + 1) + (2 + 3) for four); every thread returns the same bits.  The scratch: a row of LD >= K floats per wave.  Two barriers:
// it may be reused at once.
template <int K, int WAVES, int LD>
__device__ __forceinline__ void block_sum(float (&v)[K], float (*s_red)[LD]) {
    static_assert(K <= LD, "a wave's partials fit its row of the scratch");
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if ((tid & (WAVE - 1)) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) s_red[tid / WAVE][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float q[WAVES];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) q[w] = s_red[w][k];
#pragma unroll
        for (int span = WAVES / 2; span > 0; span >>= 1)
#pragma unroll
            for (int w = 0; w < span; ++w) q[w] = q[2 * w] + q[2 * w + 1];
        v[k] = q[0];
    }
    __syncthreads();
}

// Maximum of one value per thread over the workgroup, through column 0 of the same scratch.  A maximum is exact, so the order decides
// no bit of the result: four waves are paired and sixteen chained, as the kernels' code objects had it before the helper was shared.
template <int WAVES, int LD>
__device__ __forceinline__ float block_max(float v, float (*s_red)[LD]) {
    const int tid = threadIdx.x;
    v = wave_max(v);
    if ((tid & (WAVE - 1)) == 0) s_red[tid / WAVE][0] = v;
    __syncthreads();
    float m = s_red[0][0];
    if constexpr (WAVES == 4) {
        m = fmaxf(fmaxf(m, s_red[1][0]), fmaxf(s_red[2][0], s_red[3][0]));
    } else {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) m = fmaxf(m, s_red[w][0]);
    }
    __syncthreads();
    return m;
}

// ---- the logistic loss of one training row ----------------------------------------------------------------------------------------
// d loss / d f at decision values f (r = p - onehot) and what the Hessian needs: binary w[0] = p (1 - p), multinomial w = p.
template <int NC>
__device__ __forceinline__ void row_residual(const float (&f)[NC], int cols, int label, float (&r)[NC], float (&w)[NC]) {
    if (cols == 1) {
        const float s = label ? 1.f : -1.f;
        const float q = 1.f / (1.f + expf(s * f[0]));       // sigmoid(-s f): 0 when s f overflows
        r[0] = -s * q;
        w[0] = q * (1.f - q);
    } else {
        float m = f[0];
#pragma unroll
        for (int c = 1; c < NC; ++c)
            if (c < cols) m = fmaxf(m, f[c]);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            w[c] = c < cols ? expf(f[c] - m) : 0.f;
            sum += w[c];
        }
        const float inv = 1.f / sum;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            w[c] *= inv;
            r[c] = w[c] - (c == label ? 1.f : 0.f);
        }
    }
}

// (D q) of one row: the loss Hessian with respect to its decision values, applied to q
template <int NC>
__device__ __forceinline__ void row_hess(const float (&w)[NC], int cols, const float (&q)[NC], float (&out)[NC]) {
    if (cols == 1) {
        out[0] = w[0] * q[0];
    } else {
        float pq = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) pq = fmaf(w[c], q[c], pq);
#pragma unroll
        for (int c = 0; c < NC; ++c) out[c] = w[c] * (q[c] - pq);
    }
}

// ---- Gram tile ---------------------------------------------------------------------------------------------------------------------
// Tile (ti, tj) of G = X_t X_t^T by a workgroup of THREADS = 256: s_off [2][GRAM_TILE] holds the element offset in X of the tile's rows
// and of its columns' rows (-1: a zero row), sA / sB [GRAM_KC][GRAM_TILE + 1] are the caller's LDS.  Thread (ty, tx) owns the 4 x 4
// elements (ty + 16 u, tx + 16 v), each one fmaf chain over k = 0 .. d - 1.  The caller has a barrier behind its writes of s_off.
template <int THREADS>
__device__ __forceinline__ void gram_tile(const float* __restrict__ X, int d, const int64_t (*s_off)[GRAM_TILE],
                                          float (*sA)[GRAM_TILE + 1], float (*sB)[GRAM_TILE + 1], float* __restrict__ Gp, int ldg, int ti,
                                          int tj) {
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < d; k0 += GRAM_KC) {
#pragma unroll
        for (int q = 0; q < GRAM_TILE * GRAM_KC / THREADS; ++q) {
            const int e = q * THREADS + tid, r = e / GRAM_KC, kk = e % GRAM_KC;
            const bool in = k0 + kk < d;
            const int64_t oa = s_off[0][r], ob = s_off[1][r];
            sA[kk][r] = (in && oa >= 0) ? X[oa + k0 + kk] : 0.f;
            sB[kk][r] = (in && ob >= 0) ? X[ob + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < GRAM_KC; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = sA[kk][ty + 16 * u];
                b[u] = sB[kk][tx + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(a[u], b[v], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) Gp[(int64_t)(ti * GRAM_TILE + ty + 16 * u) * ldg + tj * GRAM_TILE + tx + 16 * v] = acc[u][v];
}

// ---- the test set and the prediction of a case -------------------------------------------------------------------------------------
// the class of a labeled case, -1 for an unlabeled one (a training case is struck out afterwards)
__device__ __forceinline__ int8_t probe_test_class(int label, int C) { return (label >= 0 && label < C) ? (int8_t)label : (int8_t)-1; }

// Strikes the training cases of problem p out of its per-case codes (-1: not a test case), by a workgroup of THREADS.  A count outside
// [0, n_max] is clamped and an index outside [0, S) skipped: a refused problem reads nothing out of bounds.  The caller has a barrier
// on either side.
template <int THREADS>
__device__ __forceinline__ void strike_training(int8_t* code, const int32_t* train_idx, const int32_t* n_train,
                                                int p, int n_max, int S) {
    int n = n_train[p];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const int idx = train_idx[(int64_t)p * n_max + i];
        if (idx >= 0 && idx < S) code[idx] = (int8_t)-1;
    }
}

// The prediction of one case from its decision values zs [cols].  cols == 1: z > 0.  Else the first maximum, and score[c * cstride] =
// log_softmax(zs)[c] in double.
__device__ __forceinline__ int probe_predict(const float* __restrict__ zs, int cols, double* __restrict__ score, int64_t cstride) {
    if (cols == 1) return zs[0] > 0.f ? 1 : 0;
    int pred = 0;
    float best = zs[0];
    for (int c = 1; c < cols; ++c)
        if (zs[c] > best) {                 // strictly greater: the lowest index wins a tie
            best = zs[c];
            pred = c;
        }
    double sum = 0.0;
    for (int c = 0; c < cols; ++c) sum += exp((double)zs[c] - (double)best);
    const double lse = (double)best + log(sum);
    for (int c = 0; c < cols; ++c) score[c * cstride] = (double)zs[c] - lse;
    return pred;
}

}  // namespace mdl
