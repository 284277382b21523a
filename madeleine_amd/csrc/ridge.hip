// ridge.hip -- the regression probe (R1-R3 of include/madeleine_amd_regress.h): P x A x T ridge fits of continuous targets over one
// embedding matrix by a direct solve in double, the decision values of every case under every fit, and per fit Pearson, Spearman, R^2,
// MAE and RMSE over the held-out cases.
//
//   rg_check_kernel    one workgroup per problem: the training list is within [1, n_max] x [0, S), or the problem is refused.
//   rg_mean_kernel     one thread per column of X and of Y: the training mean in double, rows in list order.
//   rg_system_kernel   one workgroup per 64 x 64 tile of the lower triangle of K: the Gram matrix of the centred rows (n <= d) or their
//                      covariance (n > d), every entry one fp64 FMA chain in ascending order of the summed index.
//   rg_rhs_kernel      covariance form only: r = Xc^T (y - ybar) per target, chains in list order (the Gram form's r is y - ybar itself).
//   rg_chol_kernel     one workgroup of 1024 per (p, a): K + alpha I = L L^T, right-looking, panels of 32 columns: the diagonal block in
//                      LDS, the panel by one thread per row, the trailing update in 128 x 128 blocks whose panel slices pass through LDS
//                      while the matrix itself stays in L2.  L is stored column-major with its transpose mirrored into the upper triangle,
//                      so that both substitutions read it along columns.
//   rg_solve_kernel    one workgroup per (p, a) and 8 targets: forward and back substitution with the right-hand sides in LDS, then W and b.
//   rg_scores_kernel   64 x 64 tiles of Z = W X^T + b in fp32.
//   rg_mask_kernel, rg_yrank_kernel, rg_metrics_kernel   the test set, the ranks of y among the test cases (once per (p, t)), and per
//                      list the ranks of z by exact pair counting, the six integer sums and the fp64 two-pass sums.
// No workgroup waits on another, there is no atomic, and every loop has a bound that is an argument or a constant of the header.
#include "probe_host.hpp"

#include "../../include/madeleine_amd_regress.h"

namespace mdl {
namespace {

constexpr int RG_SYS = MDL_RIDGE_MAX_SYS;
constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / WAVE;
constexpr int RG_TILE = 64;                // tile of K and of Z
constexpr int RG_KC = 16;                  // fp64 k-chunk of a K tile
constexpr int RG_NB = 32;                  // Cholesky panel width
constexpr int RG_CH_THREADS = 1024;
constexpr int RG_TB = 128;                 // trailing-update block
constexpr int RG_TK = 16;                  // panel columns per pass of a trailing block
constexpr int RG_TC = 8;                   // targets per solve workgroup
constexpr int RG_GRID_Y = 65535;           // problems ride on the second grid dimension
constexpr int RG_RT = 16;                  // targets per tile of the covariance right-hand sides
static_assert(RG_SYS % RG_NB == 0 && RG_CH_THREADS == RG_SYS && RG_CH_THREADS == RG_NB * RG_NB, "one thread per row and per block entry");

struct RidgeAlphas {
    double v[MDL_RIDGE_MAX_ALPHAS];
};

// workspace of the fit: status [P] (1: refused), fail [P A] (1: no factor), mean [P][d], ybar [P][T], K [P][ld][ld],
// L [P A][ld][ld] (column-major, ld >= min(n_max, d)), rhs [P][T][ld]
struct RidgeWs {
    int32_t* status;
    int32_t* fail;
    double* mean;
    double* ybar;
    double* K;
    double* L;
    double* rhs;
    int64_t ld;
};
inline int64_t ridge_ld(int n_max, int d) { return ((n_max < d ? n_max : d) + 1) / 2 * 2; }
inline int64_t ridge_ws_layout(RidgeWs* c, void* ws, int64_t P, int n_max, int d, int64_t T, int A) {
    const int64_t ld = ridge_ld(n_max, d);
    char* base = reinterpret_cast<char*>(ws);
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        char* at = base + o;
        o += up16(bytes);
        return at;
    };
    int32_t* status = reinterpret_cast<int32_t*>(take(P * 4));
    int32_t* fail = reinterpret_cast<int32_t*>(take(P * A * 4));
    double* mean = reinterpret_cast<double*>(take(P * d * 8));
    double* ybar = reinterpret_cast<double*>(take(P * T * 8));
    double* K = reinterpret_cast<double*>(take(P * ld * ld * 8));
    double* L = reinterpret_cast<double*>(take(P * A * ld * ld * 8));
    double* rhs = reinterpret_cast<double*>(take(P * T * ld * 8));
    if (c) *c = {status, fail, mean, ybar, K, L, rhs, ld};
    return o;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over a workgroup of RG_THREADS: xor butterflies, then the four waves as (0 + 1) + (2 + 3); every thread returns the same bits
template <class V>
__device__ __forceinline__ V rg_block_sum(V v, V* s_red) {
    if constexpr (std::is_floating_point<V>::value) {
        v = wave_sum_f64(v);
    } else {
        v = wave_sum_i64(v);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
    __syncthreads();
    const V out = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    __syncthreads();
    return out;
}

// ---- R1: check and means ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_check_kernel(const int32_t* __restrict__ train_idx, const int32_t* __restrict__ n_train,
                                                             int n_max, int S, RidgeWs c) {
    const int p = blockIdx.x, n = n_train[p];
    int bad = (n < 1 || n > n_max) ? 1 : 0;
    if (!bad)
        for (int i = threadIdx.x; i < n; i += RG_THREADS) {
            const int idx = train_idx[(int64_t)p * n_max + i];
            if (idx < 0 || idx >= S) bad = 1;
        }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) c.status[p] = bad;
}

// column col of [X | Y]: its mean over the training rows of p
__global__ __launch_bounds__(RG_THREADS) void rg_mean_kernel(const float* __restrict__ X, int64_t ldX, int d, const float* __restrict__ Y,
                                                            int64_t ldY, int T, const int32_t* __restrict__ train_idx,
                                                            const int32_t* __restrict__ n_train, int n_max, RidgeWs c) {
    const int p = blockIdx.y, col = blockIdx.x * RG_THREADS + threadIdx.x;
    if (c.status[p] || col >= d + T) return;
    const int n = n_train[p];
    const int32_t* idx = train_idx + (int64_t)p * n_max;
    const bool isx = col < d;
    const float* src = isx ? X + col : Y + (col - d);
    const int64_t ld = isx ? ldX : ldY;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += (double)src[(int64_t)idx[i] * ld];
    const double mean = sum / (double)n;
    if (isx) {
        c.mean[(int64_t)p * d + col] = mean;
    } else {
        c.ybar[(int64_t)p * T + (col - d)] = mean;
    }
}

// ---- R1: the system ---------------------------------------------------------------------------------------------------------------
// Tile (ti, tj), tj <= ti, of the lower triangle of K.  Thread (tx, ty) owns rows tx + 16 u and columns ty + 16 v.
__global__ __launch_bounds__(RG_THREADS) void rg_system_kernel(const float* __restrict__ X, int64_t ldX, int d,
                                                              const int32_t* __restrict__ train_idx, const int32_t* __restrict__ n_train,
                                                              int n_max, int tps, RidgeWs c) {
    const int p = blockIdx.y, ti = blockIdx.x / tps, tj = blockIdx.x % tps;
    if (c.status[p] || tj > ti) return;
    const int n = n_train[p];
    const bool gram = n <= d;
    const int M = gram ? n : d, len = gram ? d : n;      // order of the system, length of a chain
    if (ti * RG_TILE >= M) return;
    __shared__ double sA[RG_KC][RG_TILE + 1], sB[RG_KC][RG_TILE + 1];
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const int32_t* idx = train_idx + (int64_t)p * n_max;
    const double* mean = c.mean + (int64_t)p * d;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < len; k0 += RG_KC) {
#pragma unroll
        for (int q = 0; q < RG_TILE * RG_KC / RG_THREADS; ++q) {
            const int e = q * RG_THREADS + tid;
            // Gram: entry r = a training row, kk = a column of X (16 consecutive floats of a row); covariance: r = a column, kk = a row
            const int r = gram ? e / RG_KC : e % RG_TILE, kk = gram ? e % RG_KC : e / RG_TILE;
            const int k = k0 + kk, ra = ti * RG_TILE + r, rb = tj * RG_TILE + r;
            double a = 0.0, b = 0.0;
            if (k < len) {
                if (gram) {
                    if (ra < M) a = (double)X[(int64_t)idx[ra] * ldX + k] - mean[k];
                    if (rb < M) b = (double)X[(int64_t)idx[rb] * ldX + k] - mean[k];
                } else {
                    const int64_t row = (int64_t)idx[k] * ldX;
                    if (ra < M) a = (double)X[row + ra] - mean[ra];
                    if (rb < M) b = (double)X[row + rb] - mean[rb];
                }
            }
            sA[kk][r] = a;
            sB[kk][r] = b;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < RG_KC; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = sA[kk][tx + 16 * u];
                b[u] = sB[kk][ty + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
        __syncthreads();
    }
    double* Kp = c.K + (int64_t)p * c.ld * c.ld;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = ti * RG_TILE + tx + 16 * u, col = tj * RG_TILE + ty + 16 * v;
            if (row < M && col <= row) Kp[(int64_t)col * c.ld + row] = acc[u][v];
        }
}

// covariance form: rhs[p, t, j] = sum_i (x_ij - mean_j) (y_it - ybar_t), i in list order.  Thread (tj, tg): column j0 + tj, targets
// t0 + 4 tg .. + 3.
__global__ __launch_bounds__(RG_THREADS) void rg_rhs_kernel(const float* __restrict__ X, int64_t ldX, int d, const float* __restrict__ Y,
                                                           int64_t ldY, int T, const int32_t* __restrict__ train_idx,
                                                           const int32_t* __restrict__ n_train, int n_max, int jt, RidgeWs c) {
    const int p = blockIdx.y;
    if (c.status[p]) return;
    const int n = n_train[p];
    if (n <= d) return;                              // the Gram form takes y - ybar itself
    const int j0 = (blockIdx.x % jt) * RG_TILE, t0 = (blockIdx.x / jt) * RG_RT;
    constexpr int RC = 32;
    __shared__ double sX[RC][RG_TILE], sY[RC][RG_RT];
    const int tid = threadIdx.x, tj = tid % RG_TILE, tg = tid / RG_TILE;
    const int32_t* idx = train_idx + (int64_t)p * n_max;
    const double* mean = c.mean + (int64_t)p * d;
    const double* ybar = c.ybar + (int64_t)p * T;
    double acc[4] = {};
    for (int i0 = 0; i0 < n; i0 += RC) {
#pragma unroll
        for (int q = 0; q < RC * RG_TILE / RG_THREADS; ++q) {
            const int e = q * RG_THREADS + tid, kk = e / RG_TILE, r = e % RG_TILE;
            sX[kk][r] = (i0 + kk < n && j0 + r < d) ? (double)X[(int64_t)idx[i0 + kk] * ldX + j0 + r] - mean[j0 + r] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < RC * RG_RT / RG_THREADS; ++q) {
            const int e = q * RG_THREADS + tid, kk = e / RG_RT, r = e % RG_RT;
            sY[kk][r] = (i0 + kk < n && t0 + r < T) ? (double)Y[(int64_t)idx[i0 + kk] * ldY + t0 + r] - ybar[t0 + r] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < RC; ++kk) {
            const double a = sX[kk][tj];
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = fma(a, sY[kk][tg * 4 + v], acc[v]);
        }
        __syncthreads();
    }
    if (j0 + tj < d)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = t0 + tg * 4 + v;
            if (t < T) c.rhs[((int64_t)p * T + t) * c.ld + j0 + tj] = acc[v];
        }
}

// ---- R1: the factorisation ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_CH_THREADS) void rg_chol_kernel(int d, const int32_t* __restrict__ n_train, int A, RidgeAlphas alphas,
                                                               float* __restrict__ info, RidgeWs c) {
    __shared__ double sD[RG_NB][RG_NB + 1];          // the diagonal block, lower triangle; identity outside the matrix
    __shared__ double sPi[RG_TK][RG_TB], sPj[RG_TK][RG_TB];
    __shared__ double s_max[RG_CH_THREADS / WAVE];
    __shared__ double sInvD[RG_NB];
    const int tid = threadIdx.x, pa = blockIdx.x, p = pa / A, a = pa % A;
    const double nan = __builtin_nan("");
    if (c.status[p]) {
        if (tid == 0) {
            c.fail[pa] = 1;
            info[(int64_t)pa * 2] = 0.f;
            info[(int64_t)pa * 2 + 1] = __builtin_nanf("");
        }
        return;
    }
    const int n = n_train[p], M = n <= d ? n : d;
    const int64_t ld = c.ld;
    const double* Kp = c.K + (int64_t)p * ld * ld;
    double* Lp = c.L + (int64_t)pa * ld * ld;
    const double alpha = alphas.v[a];

    // L <- the lower triangle of K + alpha I; the largest diagonal entry
    double dmax = 0.0;
    for (int col = tid / RG_NB; col < M; col += RG_CH_THREADS / RG_NB)
        for (int row = col + tid % RG_NB; row < M; row += RG_NB) {
            double v = Kp[(int64_t)col * ld + row];
            if (row == col) {
                v += alpha;
                dmax = v > dmax ? v : dmax;          // a NaN never enters: the pivots below find it
            }
            Lp[(int64_t)col * ld + row] = v;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o, 64));
    if ((tid & (WAVE - 1)) == 0) s_max[tid / WAVE] = dmax;
    __syncthreads();
    dmax = s_max[0];
    for (int w = 1; w < RG_CH_THREADS / WAVE; ++w) dmax = fmax(dmax, s_max[w]);

    const int br = tid % RG_NB, bc = tid / RG_NB;    // this thread's entry of the diagonal block
    double minpiv = __builtin_inf();
    bool fail = false;
    for (int kb = 0; kb < M && !fail; kb += RG_NB) {
        const int nb = M - kb < RG_NB ? M - kb : RG_NB;
        sD[br][bc] = (br < nb && bc <= br) ? Lp[(int64_t)(kb + bc) * ld + kb + br] : (br == bc ? 1.0 : 0.0);
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            const double piv = sD[j][j];             // every thread reads the same value: the exit is uniform
            if (!(piv > 0.0)) {
                fail = true;
                break;
            }
            minpiv = piv < minpiv ? piv : minpiv;
            const double l = sqrt(piv);
            double upd = 0.0;
            const bool inner = bc > j && br >= bc;
            if (inner) upd = fma(-(sD[br][j] / l), sD[bc][j] / l, sD[br][bc]);
            __syncthreads();
            if (inner) sD[br][bc] = upd;
            if (bc == j && br >= j) sD[br][j] = br == j ? l : sD[br][j] / l;
            __syncthreads();
        }
        if (fail) break;
        if (bc == 0) sInvD[br] = 1.0 / sD[br][br];
        __syncthreads();
        if (br < nb && bc <= br) {                   // the block and its mirror
            Lp[(int64_t)(kb + bc) * ld + kb + br] = sD[br][bc];
            Lp[(int64_t)(kb + br) * ld + kb + bc] = sD[br][bc];
        }
        // the panel: row i of the rows below solves x L_kk^T = a, one thread per row, column by column with the diagonal's reciprocals
        const int i = kb + nb + tid;
        if (i < M) {
            double x[RG_NB];
#pragma unroll
            for (int q = 0; q < RG_NB; ++q) x[q] = q < nb ? Lp[(int64_t)(kb + q) * ld + i] : 0.0;
#pragma unroll 1       // unrolled, the 496 reads of the block are hoisted together and spill a thousand registers
            for (int k = 0; k < nb; ++k) {           // the pivot column's entry is x[0]; the rest moves down one register
                const double xk = x[0] * sInvD[k];
                Lp[(int64_t)(kb + k) * ld + i] = xk;
                Lp[(int64_t)i * ld + kb + k] = xk;
#pragma unroll
                for (int q = 0; q < RG_NB - 1; ++q) x[q] = k + 1 + q < RG_NB ? fma(-xk, sD[k + 1 + q][k], x[q + 1]) : 0.0;
            }
        }
        __syncthreads();                             // the panel is in memory for the whole workgroup
        // the trailing matrix, lower triangle, in RG_TB x RG_TB blocks: thread (tx, ty) owns rows tx + 32 u and columns ty + 32 v
        const int r0 = kb + nb, rest = M - r0, nblk = (rest + RG_TB - 1) / RG_TB;
        const int tx = tid % 32, ty = tid / 32;
        for (int bi = 0; bi < nblk; ++bi)
            for (int bj = 0; bj <= bi; ++bj) {
                const int i0 = r0 + bi * RG_TB, j0 = r0 + bj * RG_TB;
                double acc[4][4] = {};
                for (int kp = 0; kp < RG_NB; kp += RG_TK) {
#pragma unroll
                    for (int q = 0; q < RG_TK * RG_TB / RG_CH_THREADS; ++q) {
                        const int e = q * RG_CH_THREADS + tid, k = kp + e / RG_TB, r = e % RG_TB;
                        const bool in = k < nb;
                        sPi[e / RG_TB][r] = (in && i0 + r < M) ? Lp[(int64_t)(kb + k) * ld + i0 + r] : 0.0;
                        sPj[e / RG_TB][r] = (in && j0 + r < M) ? Lp[(int64_t)(kb + k) * ld + j0 + r] : 0.0;
                    }
                    __syncthreads();
#pragma unroll 4
                    for (int k = 0; k < RG_TK; ++k) {
                        double pi[4], pj[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            pi[u] = sPi[k][tx + 32 * u];
                            pj[u] = sPj[k][ty + 32 * u];
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int v = 0; v < 4; ++v) acc[u][v] = fma(pi[u], pj[v], acc[u][v]);
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int row = i0 + tx + 32 * u, col = j0 + ty + 32 * v;
                        if (row < M && col <= row) Lp[(int64_t)col * ld + row] -= acc[u][v];
                    }
            }
        __syncthreads();                             // the updated matrix is in memory before the next block is read
    }
    if (tid == 0) {
        c.fail[pa] = fail ? 1 : 0;
        info[(int64_t)pa * 2] = fail ? 0.f : 1.f;
        info[(int64_t)pa * 2 + 1] = (float)((fail ? nan : minpiv) / dmax);
    }
}

// ---- R1: the substitutions, W and b ------------------------------------------------------------------------------------------------
// The diagonal block kb of L into sD (lower triangle, identity outside the matrix) and the reciprocals of its diagonal
__device__ __forceinline__ void rg_load_block(const double* __restrict__ Lp, int64_t ld, int kb, int nb, double (*sD)[RG_NB + 1],
                                              double* sInv) {
#pragma unroll
    for (int q = 0; q < RG_NB * RG_NB / RG_THREADS; ++q) {
        const int e = q * RG_THREADS + threadIdx.x, r = e % RG_NB, col = e / RG_NB;
        const double v = (r < nb && col <= r) ? Lp[(int64_t)(kb + col) * ld + kb + r] : (r == col ? 1.0 : 0.0);
        sD[r][col] = v;
        if (r == col) sInv[r] = 1.0 / v;
    }
}

__global__ __launch_bounds__(RG_THREADS) void rg_solve_kernel(const float* __restrict__ X, int64_t ldX, int d, const float* __restrict__ Y,
                                                             int64_t ldY, int T, const int32_t* __restrict__ train_idx,
                                                             const int32_t* __restrict__ n_train, int n_max, int A,
                                                             float* __restrict__ W_out, float* __restrict__ b_out, RidgeWs c) {
    extern __shared__ double sC[];                   // [M][RG_TC]: the right-hand sides, then the solutions
    __shared__ double sD[RG_NB][RG_NB + 1];
    __shared__ double sInv[RG_NB];
    __shared__ double s_red[RG_WAVES];
    const int tid = threadIdx.x, pa = blockIdx.y, p = pa / A, t0 = blockIdx.x * RG_TC;
    const int nt = T - t0 < RG_TC ? T - t0 : RG_TC;
    float* Wp = W_out + ((int64_t)pa * T + t0) * d;
    float* bp = b_out + (int64_t)pa * T + t0;
    if (c.status[p] || c.fail[pa]) {
        const float nan = __builtin_nanf("");
        for (int64_t e = tid; e < (int64_t)nt * d; e += RG_THREADS) Wp[e] = nan;
        if (tid < nt) bp[tid] = nan;
        return;
    }
    const int n = n_train[p];
    const bool gram = n <= d;
    const int M = gram ? n : d;
    const int64_t ld = c.ld;
    const int32_t* idx = train_idx + (int64_t)p * n_max;
    const double* mean = c.mean + (int64_t)p * d;
    const double* ybar = c.ybar + (int64_t)p * T + t0;
    const double* Lp = c.L + (int64_t)pa * ld * ld;

    for (int e = tid; e < M * RG_TC; e += RG_THREADS) {
        const int i = e / RG_TC, v = e % RG_TC;
        double r = 0.0;
        if (v < nt) r = gram ? (double)Y[(int64_t)idx[i] * ldY + t0 + v] - ybar[v] : c.rhs[((int64_t)p * T + t0 + v) * ld + i];
        sC[e] = r;
    }
    __syncthreads();

    const int sr = tid % RG_NB, sv = tid / RG_NB;    // the diagonal solves: entry sr of target sv, in registers, by shuffles
    // L c' = r
    for (int kb = 0; kb < M; kb += RG_NB) {
        const int nb = M - kb < RG_NB ? M - kb : RG_NB;
        rg_load_block(Lp, ld, kb, nb, sD, sInv);
        __syncthreads();
        double val = sr < nb ? sC[(kb + sr) * RG_TC + sv] : 0.0;
        for (int k = 0; k < RG_NB; ++k) {
            const double ck = __shfl(val, k, RG_NB) * sInv[k];
            if (sr == k) val = ck;
            if (sr > k) val = fma(-sD[sr][k], ck, val);
        }
        if (sr < nb) sC[(kb + sr) * RG_TC + sv] = val;
        __syncthreads();
        for (int i = kb + nb + tid; i < M; i += RG_THREADS) {
            double acc[RG_TC];
#pragma unroll
            for (int v = 0; v < RG_TC; ++v) acc[v] = sC[i * RG_TC + v];
            for (int k = 0; k < nb; ++k) {
                const double l = Lp[(int64_t)(kb + k) * ld + i];
#pragma unroll
                for (int v = 0; v < RG_TC; ++v) acc[v] = fma(-l, sC[(kb + k) * RG_TC + v], acc[v]);
            }
#pragma unroll
            for (int v = 0; v < RG_TC; ++v) sC[i * RG_TC + v] = acc[v];
        }
        __syncthreads();
    }
    // L^T c = c': the blocks in descending order, L^T read from the mirror in the upper triangle
    for (int kb = (M - 1) / RG_NB * RG_NB; kb >= 0; kb -= RG_NB) {
        const int nb = M - kb < RG_NB ? M - kb : RG_NB;
        rg_load_block(Lp, ld, kb, nb, sD, sInv);
        __syncthreads();
        double val = sr < nb ? sC[(kb + sr) * RG_TC + sv] : 0.0;
        for (int k = RG_NB - 1; k >= 0; --k) {
            const double ck = __shfl(val, k, RG_NB) * sInv[k];
            if (sr == k) val = ck;
            if (sr < k) val = fma(-sD[k][sr], ck, val);
        }
        if (sr < nb) sC[(kb + sr) * RG_TC + sv] = val;
        __syncthreads();
        for (int i = tid; i < kb; i += RG_THREADS) {
            double acc[RG_TC];
#pragma unroll
            for (int v = 0; v < RG_TC; ++v) acc[v] = sC[i * RG_TC + v];
            for (int k = 0; k < nb; ++k) {
                const double l = Lp[(int64_t)(kb + k) * ld + i];
#pragma unroll
                for (int v = 0; v < RG_TC; ++v) acc[v] = fma(-l, sC[(kb + k) * RG_TC + v], acc[v]);
            }
#pragma unroll
            for (int v = 0; v < RG_TC; ++v) sC[i * RG_TC + v] = acc[v];
        }
        __syncthreads();
    }

    // W (Gram form: Xc^T c, a chain in list order) and the partial sums of xbar . W over this thread's columns, ascending
    double dot[RG_TC] = {};
    for (int j = tid; j < d; j += RG_THREADS) {
        double w[RG_TC];
        if (gram) {
#pragma unroll
            for (int v = 0; v < RG_TC; ++v) w[v] = 0.0;
            const double mj = mean[j];
            for (int i = 0; i < n; ++i) {
                const double x = (double)X[(int64_t)idx[i] * ldX + j] - mj;
#pragma unroll
                for (int v = 0; v < RG_TC; ++v) w[v] = fma(x, sC[i * RG_TC + v], w[v]);
            }
        } else {
#pragma unroll
            for (int v = 0; v < RG_TC; ++v) w[v] = sC[j * RG_TC + v];
        }
#pragma unroll
        for (int v = 0; v < RG_TC; ++v) {
            if (v < nt) Wp[(int64_t)v * d + j] = (float)w[v];
            dot[v] = fma(mean[j], w[v], dot[v]);
        }
    }
#pragma unroll
    for (int v = 0; v < RG_TC; ++v) {
        const double total = rg_block_sum(dot[v], s_red);
        if (tid == 0 && v < nt) bp[v] = (float)(ybar[v] - total);
    }
}

// ---- R2 ---------------------------------------------------------------------------------------------------------------------------
// Tile (tl, ts) of Z [L, S]: thread (tx, ty) owns lists ty + 16 u and cases tx + 16 v, each one fmaf chain over k = 0 .. d - 1, then + b
__global__ __launch_bounds__(RG_THREADS) void rg_scores_kernel(const float* __restrict__ X, int64_t ldX, int S, int d,
                                                              const float* __restrict__ W, const float* __restrict__ b, int64_t L,
                                                              int st, float* __restrict__ Z) {
    constexpr int KC = 32;
    __shared__ float sW[KC][RG_TILE + 1], sX[KC][RG_TILE + 1];
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const int64_t l0 = (int64_t)(blockIdx.x / st) * RG_TILE;
    const int i0 = (blockIdx.x % st) * RG_TILE;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < d; k0 += KC) {
#pragma unroll
        for (int q = 0; q < RG_TILE * KC / RG_THREADS; ++q) {
            const int e = q * RG_THREADS + tid, r = e / KC, kk = e % KC;
            const bool in = k0 + kk < d;
            sW[kk][r] = (in && l0 + r < L) ? W[(l0 + r) * d + k0 + kk] : 0.f;
            sX[kk][r] = (in && i0 + r < S) ? X[(int64_t)(i0 + r) * ldX + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < KC; ++kk) {
            float w[4], x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                w[u] = sW[kk][ty + 16 * u];
                x[u] = sX[kk][tx + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(x[v], w[u], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t l = l0 + ty + 16 * u;
        if (l >= L) continue;
        const float bl = b[l];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + tx + 16 * v;
            if (i < S) Z[l * S + i] = acc[u][v] + bl;
        }
    }
}

// ---- R3 ---------------------------------------------------------------------------------------------------------------------------
// workspace: mask [P][S16] int8 (0: outside the training list, -1: in it), ry [P T][S] int32 (the doubled rank of y, 0: no test case)
struct RegWs {
    int8_t* mask;
    int32_t* ry;
};
inline int64_t reg_ws_layout(RegWs* m, void* ws, int64_t P, int64_t S, int64_t T) {
    char* base = reinterpret_cast<char*>(ws);
    const int64_t mask_bytes = up16(P * s16_of(S));
    if (m) *m = {reinterpret_cast<int8_t*>(base), reinterpret_cast<int32_t*>(base + mask_bytes)};
    return mask_bytes + up16(P * T * S * 4);
}

__global__ __launch_bounds__(RG_THREADS) void rg_mask_kernel(const int32_t* __restrict__ train_idx, const int32_t* __restrict__ n_train,
                                                            int n_max, int S, int64_t S16, RegWs m) {
    const int p = blockIdx.x;
    int8_t* mask = m.mask + (int64_t)p * S16;
    for (int i = threadIdx.x; i < S; i += RG_THREADS) mask[i] = 0;
    __syncthreads();
    strike_training<RG_THREADS>(mask, train_idx, n_train, p, n_max, S);
}

// The doubled rank 2 #less + #equal + 1 of `mine` among the S values vals(j) (a NaN is no value: it is neither less nor equal), for the
// thread's own case of every slice handed to `sink(i, rank)`.  Staged through s_v in chunks of RG_THREADS.
template <class Vals, class Sink>
__device__ __forceinline__ void rg_ranks(int S, float* s_v, Vals vals, Sink sink) {
    const int tid = threadIdx.x;
    for (int i0 = 0; i0 < S; i0 += RG_THREADS) {
        const int i = i0 + tid;
        const float vi = i < S ? vals(i) : __builtin_nanf("");
        int less = 0, equal = 0;
        for (int j0 = 0; j0 < S; j0 += RG_THREADS) {
            s_v[tid] = j0 + tid < S ? vals(j0 + tid) : __builtin_nanf("");
            __syncthreads();
            const int lim = S - j0 < RG_THREADS ? S - j0 : RG_THREADS;
            for (int jj = 0; jj < lim; ++jj) {
                const float vj = s_v[jj];
                less += vj < vi ? 1 : 0;
                equal += vj == vi ? 1 : 0;
            }
            __syncthreads();
        }
        if (i < S) sink(i, 2 * less + equal + 1);
    }
}

__global__ __launch_bounds__(RG_THREADS) void rg_yrank_kernel(const float* __restrict__ Y, int64_t ldY, int T, int S, int64_t S16, RegWs m) {
    __shared__ float s_v[RG_THREADS];
    const int p = blockIdx.x / T, t = blockIdx.x % T;
    const int8_t* mask = m.mask + (int64_t)p * S16;
    int32_t* ry = m.ry + (int64_t)blockIdx.x * S;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    auto yval = [&](int i) {
        const float y = Y[(int64_t)i * ldY + t];
        return (mask[i] == 0 && y > -inf && y < inf) ? y : nan;      // a test case: finite and outside the training list
    };
    rg_ranks(S, s_v, yval, [&](int i, int rank) {
        const float y = yval(i);
        ry[i] = y == y ? rank : 0;
    });
}

__global__ __launch_bounds__(RG_THREADS) void rg_metrics_kernel(const float* __restrict__ Z, const float* __restrict__ Y, int64_t ldY, int T,
                                                               int A, int S, RegWs m, double* __restrict__ metrics,
                                                               int64_t* __restrict__ sums) {
    __shared__ float s_v[RG_THREADS];
    __shared__ double s_d[RG_WAVES];
    __shared__ long long s_i[RG_WAVES];
    const int tid = threadIdx.x;
    const int64_t l = blockIdx.x;                    // (p, a, t)
    const int p = (int)(l / ((int64_t)A * T)), t = (int)(l % T);
    const float* z = Z + l * S;
    const int32_t* ry = m.ry + ((int64_t)p * T + t) * S;
    const float nanf_ = __builtin_nanf("");
    long long cnt[6] = {};                           // n, sum Rz, sum Ry, sum Rz^2, sum Ry^2, sum Rz Ry
    long long znan = 0;
    rg_ranks(S, s_v, [&](int i) { return ry[i] > 0 ? z[i] : nanf_; }, [&](int i, int rank) {
        const long long rz = rank, r = ry[i];
        if (r == 0) return;
        if (z[i] != z[i]) znan = 1;
        cnt[0] += 1;
        cnt[1] += rz;
        cnt[2] += r;
        cnt[3] += rz * rz;
        cnt[4] += r * r;
        cnt[5] += rz * r;
    });
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[k] = rg_block_sum(cnt[k], s_i);
    znan = rg_block_sum(znan, s_i);
    const double nt = (double)cnt[0];
    // pass 1: the means; pass 2: the centred sums.  A thread's cases in case order.
    double sy = 0.0, sz = 0.0;
    for (int i = tid; i < S; i += RG_THREADS)
        if (ry[i] > 0) {
            sy += (double)Y[(int64_t)i * ldY + t];
            sz += (double)z[i];
        }
    const double my = rg_block_sum(sy, s_d) / nt, mz = rg_block_sum(sz, s_d) / nt;
    double q[5] = {};                                // Syy, Szz, Syz, sum (y - z)^2, sum |y - z|
    for (int i = tid; i < S; i += RG_THREADS)
        if (ry[i] > 0) {
            const double y = (double)Y[(int64_t)i * ldY + t], zi = (double)z[i];
            const double dy = y - my, dz = zi - mz, e = y - zi;
            q[0] = fma(dy, dy, q[0]);
            q[1] = fma(dz, dz, q[1]);
            q[2] = fma(dy, dz, q[2]);
            q[3] = fma(e, e, q[3]);
            q[4] += fabs(e);
        }
#pragma unroll
    for (int k = 0; k < 5; ++k) q[k] = rg_block_sum(q[k], s_d);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        const long long n = cnt[0];
        const long long num = n * cnt[5] - cnt[1] * cnt[2];      // exact: n sum Rz Ry < 2.9e17 at S <= 16384
        const long long vz = n * cnt[3] - cnt[1] * cnt[1], vy = n * cnt[4] - cnt[2] * cnt[2];      // 0: all values equal
        const bool any = n >= 2 && !znan;
        double* out = metrics + l * 6;
        out[MDL_REG_NTEST] = nt;
        out[MDL_REG_PEARSON] = (any && vz > 0 && vy > 0) ? q[2] / (sqrt(q[0]) * sqrt(q[1])) : nan;
        out[MDL_REG_SPEARMAN] = (any && vz > 0 && vy > 0) ? (double)num / (sqrt((double)vz) * sqrt((double)vy)) : nan;
        out[MDL_REG_R2] = (any && vy > 0) ? 1.0 - q[3] / q[0] : nan;
        out[MDL_REG_MAE] = any ? q[4] / nt : nan;
        out[MDL_REG_RMSE] = any ? sqrt(q[3] / nt) : nan;
        if (sums) {
#pragma unroll
            for (int k = 0; k < 6; ++k) sums[l * 6 + k] = cnt[k];
        }
    }
}

// the limits of the entry points: {n_max, d, S, fit, classes, min(n_max, d), T, A}
constexpr ProbeLimits RIDGE_FIT = {MDL_RIDGE_MAX_TRAIN, PROBE_NO_LIMIT, PROBE_NO_LIMIT, true, false, RG_SYS, MDL_RIDGE_MAX_TARGETS,
                                   MDL_RIDGE_MAX_ALPHAS};
constexpr ProbeLimits REG_METRICS = {MDL_RIDGE_MAX_TRAIN, PROBE_NO_LIMIT, MDL_PROBE_MAX_CASES, false, false, PROBE_NO_LIMIT,
                                     MDL_RIDGE_MAX_TARGETS, MDL_RIDGE_MAX_ALPHAS};

constexpr ProbeLimits RIDGE_SCORES = {PROBE_NO_LIMIT, PROBE_NO_LIMIT, PROBE_NO_LIMIT, true, false, PROBE_NO_LIMIT, PROBE_NO_LIMIT,
                                      PROBE_NO_LIMIT, false};      // L lists in the place of P problems; no table

inline ProbeTable ridge_table(const int32_t* train_idx, const int32_t* n_train, int64_t P, int n_max, int64_t S, int d, int64_t T, int A) {
    ProbeTable t = {train_idx, n_train, P, n_max, S, {}, 0, 0, d};
    t.T = T;
    t.A = A;
    return t;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_ridge_fit_ws_bytes(int64_t P, int n_max, int d, int64_t T, int A) {
    if (const int rc = probe_check(ridge_table(nullptr, nullptr, P, n_max, 1, d, T, A), RIDGE_FIT, nullptr)) return rc;
    return ridge_ws_layout(nullptr, nullptr, P, n_max, d, T, A);
}

extern "C" int mdl_ridge_fit(const float* X, int64_t ldX, int64_t S, int d, const float* Y, int64_t ldY, int64_t T, const int32_t* train_idx,
                             const int32_t* n_train, int64_t P, int n_max, const float* alphas, int A, float* W_out, float* b_out,
                             float* info_out, void* ws, void* stream) {
    const ProbeTable t = ridge_table(train_idx, n_train, P, n_max, S, d, T, A);
    RidgeAlphas al = {};
    bool values = ldY >= T;
    if (alphas)                                      // all A of them, whatever else is wrong with A: MDL_E_ARG comes first
        for (int a = 0; a < A; ++a) {
            if (a < MDL_RIDGE_MAX_ALPHAS) al.v[a] = (double)alphas[a];
            values = values && alphas[a] > 0.f && alphas[a] < __builtin_inff();      // a NaN fails the first comparison
        }
    const int64_t ld = ridge_ld(n_max, d), tps = ceil_div(ld, RG_TILE), cols = (int64_t)d + T;
    const int64_t jt = ceil_div(d, RG_TILE), tt = ceil_div(T, RG_RT);
    const bool grids = mul_i32(P, A, T) && i32(cols) && mul_i32(jt, tt) && P * (int64_t)A <= RG_GRID_Y;
    ProbeExtra extra = {all_given(X, Y, alphas, W_out, b_out, info_out, ws), grids,
                        host_aligned16(ws) && all_aligned(4, X, Y, W_out, b_out, info_out) && all_aligned(4, train_idx, n_train), 0, ldX, 0,
                        1.f, 0.f};
    extra.values = values;
    if (const int rc = probe_check(t, RIDGE_FIT, &extra)) return rc;
    RidgeWs c;
    ridge_ws_layout(&c, ws, P, n_max, d, T, A);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rg_check_kernel, dim3((unsigned)P), dim3(RG_THREADS), 0, s, train_idx, n_train, n_max, (int)S, c);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_mean_kernel, dim3((unsigned)ceil_div(cols, RG_THREADS), (unsigned)P), dim3(RG_THREADS), 0, s, X, ldX, d, Y, ldY,
                       (int)T, train_idx, n_train, n_max, c);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_system_kernel, dim3((unsigned)(tps * tps), (unsigned)P), dim3(RG_THREADS), 0, s, X, ldX, d, train_idx, n_train,
                       n_max, (int)tps, c);
    MDL_LAUNCH_CHECK();
    if (n_max > d) {                                 // some problem may take the covariance form
        hipLaunchKernelGGL(rg_rhs_kernel, dim3((unsigned)(jt * tt), (unsigned)P), dim3(RG_THREADS), 0, s, X, ldX, d, Y, ldY, (int)T,
                           train_idx, n_train, n_max, (int)jt, c);
        MDL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rg_chol_kernel, dim3((unsigned)(P * A)), dim3(RG_CH_THREADS), 0, s, d, n_train, A, al, info_out, c);
    MDL_LAUNCH_CHECK();
    const size_t lds = (size_t)ld * RG_TC * sizeof(double);
    if (lds > 32 * 1024) {                           // beside the static 9 KiB: the kernel's limit is raised to its largest need
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rg_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 RG_SYS * RG_TC * (int)sizeof(double));
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(rg_solve_kernel, dim3((unsigned)ceil_div(T, RG_TC), (unsigned)(P * A)), dim3(RG_THREADS), lds, s, X, ldX, d, Y, ldY,
                       (int)T, train_idx, n_train, n_max, A, W_out, b_out, c);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int mdl_ridge_scores(const float* X, int64_t ldX, int64_t S, int d, const float* W, const float* b, int64_t L, float* Z,
                                void* stream) {
    const int64_t lt = ceil_div(L, RG_TILE), st = ceil_div(S, RG_TILE);
    const ProbeExtra extra = {all_given(X, W, b, Z), mul_i32(lt, st), all_aligned(4, X, W, b, Z), 0, ldX, 0, 1.f, 0.f};
    if (const int rc = probe_check(ridge_table(nullptr, nullptr, L, 1, S, d, 1, 1), RIDGE_SCORES, &extra)) return rc;
    hipLaunchKernelGGL(rg_scores_kernel, dim3((unsigned)(lt * st)), dim3(RG_THREADS), 0, (hipStream_t)stream, X, ldX, (int)S, d, W, b, L,
                       (int)st, Z);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int64_t mdl_regress_metrics_ws_bytes(int64_t P, int64_t S, int64_t T) {
    if (const int rc = probe_check(ridge_table(nullptr, nullptr, P, 1, S, 0, T, 1), REG_METRICS, nullptr)) return rc;
    return reg_ws_layout(nullptr, nullptr, P, S, T);
}

extern "C" int mdl_regress_metrics(const float* Z, const float* Y, int64_t ldY, int64_t T, const int32_t* train_idx, const int32_t* n_train,
                                   int64_t P, int n_max, int64_t S, int A, void* metrics_out, int64_t* sums_out, void* ws, void* stream) {
    const ProbeTable t = ridge_table(train_idx, n_train, P, n_max, S, 0, T, A);
    ProbeExtra extra = {all_given(Z, Y, metrics_out, ws), mul_i32(P, T) && mul_i32(P, A, T),
                        host_aligned16(ws) && all_aligned(8, metrics_out) && all_aligned(8, sums_out) && all_aligned(4, Z, Y) &&
                            all_aligned(4, train_idx, n_train)};
    extra.values = ldY >= T;
    if (const int rc = probe_check(t, REG_METRICS, &extra)) return rc;
    RegWs m;
    reg_ws_layout(&m, ws, P, S, T);
    const int64_t S16 = s16_of(S);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rg_mask_kernel, dim3((unsigned)P), dim3(RG_THREADS), 0, s, train_idx, n_train, n_max, (int)S, S16, m);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_yrank_kernel, dim3((unsigned)(P * T)), dim3(RG_THREADS), 0, s, Y, ldY, (int)T, (int)S, S16, m);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_metrics_kernel, dim3((unsigned)(P * A * T)), dim3(RG_THREADS), 0, s, Z, Y, ldY, (int)T, A, (int)S, m,
                       reinterpret_cast<double*>(metrics_out), sums_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
