// probe_primal.hip -- the full-label linear probe (L1 of the header): P independent L2-regularised logistic fits of the objective of
// mdl_probe_fit with any number of training rows up to MDL_LOGIT_MAX_TRAIN, solved in the primal unknowns (W [cols, d], b [cols]).
//
//   logit_fit_kernel   one workgroup per problem, Newton-CG.  Everything that touches X is one SWEEP over the training rows: a wave
//                      takes LG rows at a time (row groups dealt to the four waves in turn, a function of n alone), keeps them in
//                      registers, dots them with the vector V in LDS (one DPP wave sum per row and column), applies the row's loss
//                      function and accumulates x_i u_i^T into wave-private registers (lane l owns the columns l, l + 64, ...); the four
//                      waves are added through LDS in the order ((0 + 1) + 2) + 3.  Three kinds of sweep:
//                        GRAD  V = W:  f_i = x_i . W + b, r_i and the Hessian weights of row i (to the workspace), sum x_i (cost r_i)^T
//                        HESS  V = p:  sum x_i (cost D_i (x_i . p + beta))^T with D_i from the stored weights: one CG step
//                        DOT   V = s:  df_i = x_i . s + beta (to the workspace): the decision values move linearly along the step
//                      The CG vectors live in registers (thread t owns the elements t, t + 256, ... of the flat [d, NC] array), the
//                      search direction in LDS where the sweep reads it.  The step length halves until the directional derivative,
//                      evaluated along the line from the stored f and df (O(n cols) per trial, no sweep), is no more than half as
//                      steep uphill as it was downhill at 0.
// No workgroup waits on another, no floating-point atomic, every sum in a fixed order; every loop has a bound that is an argument or a
// constant of the header.  The loss helpers and the reductions are those of probe_common.hpp.
#include "probe_host.hpp"

namespace mdl {
namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_WAVES = LG_THREADS / WAVE;
constexpr int LG_CMAX = PROBE_CMAX;
static_assert(LG_WAVES == 4, "the sweep's combine adds four waves");

__host__ __device__ __forceinline__ int64_t lg_npad_of(int n_max) { return ((int64_t)n_max + 3) / 4 * 4; }
// rows a wave holds in registers at a time, by the number of 64-column chunks of a row (and one row where the accumulators alone
// take 96 registers or more)
__host__ __device__ constexpr int lg_rows_of(int NC, int DK) { return NC * DK >= 96 ? 1 : (DK <= 2 ? 8 : (DK <= 8 ? 4 : 2)); }

enum { SW_GRAD = 0, SW_HESS = 1, SW_DOT = 2 };

struct LogitRows {              // the training rows of one problem and their state in the workspace ([n, cols] each)
    const float* X;
    int64_t ldX;
    const int32_t* tidx;        // train_idx of the problem
    const int32_t* y;           // label vector of the problem
    int n, d, cols;
    float* f;                   // decision values at W
    float* w;                   // Hessian weights at W
    float* df;                  // change of the decision values along the step
};

// One sweep over the training rows with V = s_v [d, NC] and intercept part beta (see the head of the file).  GRAD and HESS leave
// sum_i x_i u_i^T in s_out [d, NC] and return sum_i u_i in ub, the same bits in every thread; DOT writes rows.df only.  The caller
// has a barrier between its last write of s_v (and its last read of s_out) and the call; the sweep ends with one.
template <int NC, int DK, int MODE>
__device__ __forceinline__ void lg_sweep(const LogitRows& rows, float cost, const float* s_v, float* s_out, float (*s_red)[LG_CMAX + 3],
                                         const float (&beta)[NC], float (&ub)[NC]) {
    constexpr int LG = lg_rows_of(NC, DK);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int n = rows.n, d = rows.d, cols = rows.cols;
    float acc[DK][NC] = {};
    float us[NC] = {};
    for (int g = wave; g * LG < n; g += LG_WAVES) {
        float x[LG][DK];
#pragma unroll
        for (int q = 0; q < LG; ++q) {
            const int i = g * LG + q;
            const float* row = rows.X + (int64_t)rows.tidx[i < n ? i : n - 1] * rows.ldX;
#pragma unroll
            for (int k = 0; k < DK; ++k) {
                const int j = lane + WAVE * k;
                x[q][k] = (i < n && j < d) ? row[j] : 0.f;
            }
        }
        float s[LG][NC] = {};
#pragma unroll
        for (int k = 0; k < DK; ++k) {
            const int j = lane + WAVE * k;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float v = j < d ? s_v[j * NC + c] : 0.f;
#pragma unroll
                for (int q = 0; q < LG; ++q) s[q][c] = fmaf(x[q][k], v, s[q][c]);
            }
        }
#pragma unroll
        for (int q = 0; q < LG; ++q) {
            const int i = g * LG + q;
            if (i < n) {                            // uniform over the wave
                float z[NC], u[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) z[c] = wave_sum_dpp(s[q][c]) + beta[c];
                if (MODE == SW_DOT) {
                    if (lane == 0)
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            if (c < cols) rows.df[(int64_t)i * cols + c] = z[c];
                } else {
                    if (MODE == SW_GRAD) {
                        float r[NC], w[NC];
                        row_residual<NC>(z, cols, rows.y[rows.tidx[i]], r, w);
                        if (lane == 0)
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                if (c < cols) {
                                    rows.f[(int64_t)i * cols + c] = z[c];
                                    rows.w[(int64_t)i * cols + c] = w[c];
                                }
#pragma unroll
                        for (int c = 0; c < NC; ++c) u[c] = c < cols ? cost * r[c] : 0.f;
                    } else {
                        float w[NC], Dq[NC];
#pragma unroll
                        for (int c = 0; c < NC; ++c) w[c] = c < cols ? rows.w[(int64_t)i * cols + c] : 0.f;
                        row_hess<NC>(w, cols, z, Dq);
#pragma unroll
                        for (int c = 0; c < NC; ++c) u[c] = c < cols ? cost * Dq[c] : 0.f;
                    }
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        us[c] += u[c];
#pragma unroll
                        for (int k = 0; k < DK; ++k) acc[k][c] = fmaf(x[q][k], u[c], acc[k][c]);
                    }
                }
            }
        }
    }
    if (MODE == SW_DOT) {
        __syncthreads();
        return;
    }
    for (int wv = 0; wv < LG_WAVES; ++wv) {         // ((wave 0 + wave 1) + wave 2) + wave 3, element by element
        if (wave == wv) {
#pragma unroll
            for (int k = 0; k < DK; ++k) {
                const int j = lane + WAVE * k;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (j < d) s_out[j * NC + c] = wv == 0 ? acc[k][c] : s_out[j * NC + c] + acc[k][c];
            }
        }
        __syncthreads();
    }
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < NC; ++c) s_red[wave][c] = us[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) ub[c] = (s_red[0][c] + s_red[1][c]) + (s_red[2][c] + s_red[3][c]);
    __syncthreads();
}

// workspace of problem p: W [d, NC], then f, w, df, [npad, cols] fp32 each
template <int NC, int DK>
__global__ __launch_bounds__(LG_THREADS) void logit_fit_kernel(const float* __restrict__ X, int64_t ldX, int S, int d,
                                                               const int32_t* __restrict__ y, int64_t ldy,
                                                               const int32_t* __restrict__ train_idx, const int32_t* __restrict__ n_train,
                                                               int n_max, int C, float cost, float gtol, int max_iter,
                                                               float* __restrict__ W_out, float* __restrict__ b_out,
                                                               float* __restrict__ info, float* ws, int64_t npad) {
    constexpr int EM = (NC * DK * WAVE + LG_THREADS - 1) / LG_THREADS;      // elements of a [d, NC] vector per thread
    extern __shared__ float s_dyn[];
    __shared__ float s_red[LG_WAVES][LG_CMAX + 3];
    const int tid = threadIdx.x;
    const int p = blockIdx.x, cols = cols_of(C);
    const int L = d * NC;                           // vectors are [d, NC] in LDS and registers: element j * NC + c, zero at c >= cols
    float* s_v = s_dyn;
    float* s_out = s_dyn + L;
    float* Wp = W_out + (int64_t)p * cols * d;

    const int n = n_train[p];
    int bad = (n < 1 || n > n_max) ? 1 : 0;
    LogitRows rows;
    rows.X = X;
    rows.ldX = ldX;
    rows.tidx = train_idx + (int64_t)p * n_max;
    rows.y = y + (int64_t)p * ldy;
    rows.n = n;
    rows.d = d;
    rows.cols = cols;
    float* Ww = ws + (int64_t)p * (3 * npad * cols + (int64_t)L);       // W during the iteration, in the layout of the LDS vectors
    rows.f = Ww + L;
    rows.w = rows.f + npad * cols;
    rows.df = rows.w + npad * cols;
    if (!bad)
        for (int i = tid; i < n; i += LG_THREADS) {
            const int idx = rows.tidx[i];
            if (idx < 0 || idx >= S) {
                bad = 1;
            } else {
                const int label = rows.y[idx];
                if (label < 0 || label >= C) bad = 1;
            }
        }
    if (__syncthreads_or(bad)) {                    // refused: NaN, converged = 0; nothing of X is read
        const float nan = __builtin_nanf("");
        for (int e = tid; e < cols * d; e += LG_THREADS) Wp[e] = nan;
        if (tid < cols) b_out[(int64_t)p * cols + tid] = nan;
        if (tid < 4) info[(int64_t)p * 4 + tid] = tid == 2 ? nan : 0.f;
        return;
    }

    float xs[EM] = {}, rr[EM] = {};                 // the CG iterate and the CG residual: elements tid + 256 m; W itself is in Ww
    for (int e = tid; e < L; e += LG_THREADS) Ww[e] = 0.f;
    float b[NC] = {}, gb[NC], xb[NC], rb[NC], pb[NC], Hb[NC];
    float res = 0.f, prev = __builtin_inff();
    int it = 0, cg_total = 0;
    for (;;) {
        // decision values from W itself, and the gradient W + X_t^T (cost r), cost sum_i r_i
#pragma unroll
        for (int m = 0; m < EM; ++m)
            if (tid + LG_THREADS * m < L) s_v[tid + LG_THREADS * m] = Ww[tid + LG_THREADS * m];
        __syncthreads();
        lg_sweep<NC, DK, SW_GRAD>(rows, cost, s_v, s_out, s_red, b, gb);
        float gmax = 0.f;
#pragma unroll
        for (int m = 0; m < EM; ++m) {
            const int e = tid + LG_THREADS * m;
            const float g = e < L ? s_out[e] + s_v[e] : 0.f;
            gmax = fmaxf(gmax, fabsf(g));
            rr[m] = -g;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) gmax = fmaxf(gmax, fabsf(gb[c]));
        res = block_max<LG_WAVES>(gmax, s_red);
        // the stop rule of probe_fit_kernel: aim at PROBE_TIGHT * gtol, and below gtol end as soon as a step no longer halves the residual
        if (res <= PROBE_TIGHT * gtol || (res <= gtol && res >= 0.5f * prev)) break;
        if (it >= max_iter || !(res == res)) break;
        prev = res;

        // ---- CG on the Newton system, right-hand side (-g, -gb); the search direction (p, pb) has p in s_v ----
        float part[1] = {0.f};
#pragma unroll
        for (int m = 0; m < EM; ++m) {
            xs[m] = 0.f;
            part[0] = fmaf(rr[m], rr[m], part[0]);
            if (tid + LG_THREADS * m < L) s_v[tid + LG_THREADS * m] = rr[m];
        }
        block_sum<1, LG_WAVES>(part, s_red);               // its barriers also publish s_v
        float rho = part[0];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            xb[c] = 0.f;
            rb[c] = -gb[c];
            pb[c] = rb[c];
            rho = fmaf(rb[c], rb[c], rho);
        }
        const float rho0 = rho;
        for (int k = 0; k < MDL_LOGIT_CG_MAX && rho > 0.f; ++k) {
            lg_sweep<NC, DK, SW_HESS>(rows, cost, s_v, s_out, s_red, pb, Hb);
            part[0] = 0.f;
#pragma unroll
            for (int m = 0; m < EM; ++m) {
                const int e = tid + LG_THREADS * m;
                const float pe = e < L ? s_v[e] : 0.f;
                part[0] = fmaf(pe, e < L ? pe + s_out[e] : 0.f, part[0]);
            }
            block_sum<1, LG_WAVES>(part, s_red);
            float pHp = part[0];
#pragma unroll
            for (int c = 0; c < NC; ++c) pHp = fmaf(pb[c], Hb[c], pHp);
            if (!(pHp > 0.f)) break;
            const float alpha = rho / pHp;
            ++cg_total;
            part[0] = 0.f;
#pragma unroll
            for (int m = 0; m < EM; ++m) {
                const int e = tid + LG_THREADS * m;
                const float pe = e < L ? s_v[e] : 0.f;
                xs[m] = fmaf(alpha, pe, xs[m]);
                rr[m] = fmaf(-alpha, e < L ? pe + s_out[e] : 0.f, rr[m]);
                part[0] = fmaf(rr[m], rr[m], part[0]);
            }
            block_sum<1, LG_WAVES>(part, s_red);
            float rho_new = part[0];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                xb[c] = fmaf(alpha, pb[c], xb[c]);
                rb[c] = fmaf(-alpha, Hb[c], rb[c]);
                rho_new = fmaf(rb[c], rb[c], rho_new);
            }
            if (!(rho_new > PROBE_CG_TOL2 * rho0)) break;
            const float bt = rho_new / rho;
            rho = rho_new;
#pragma unroll
            for (int m = 0; m < EM; ++m) {
                const int e = tid + LG_THREADS * m;
                if (e < L) s_v[e] = fmaf(bt, s_v[e], rr[m]);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) pb[c] = fmaf(bt, pb[c], rb[c]);
            __syncthreads();
        }

        // ---- step length along (xs, xb): phi'(t) = sum_i cost r(f_i + t df_i) . df_i + <W, xs> + t <xs, xs> ----
        __syncthreads();
        float lin[2] = {0.f, 0.f};
#pragma unroll
        for (int m = 0; m < EM; ++m) {
            const int e = tid + LG_THREADS * m;
            if (e < L) s_v[e] = xs[m];
            lin[0] = fmaf(e < L ? Ww[e] : 0.f, xs[m], lin[0]);
            lin[1] = fmaf(xs[m], xs[m], lin[1]);
        }
        block_sum<2, LG_WAVES>(lin, s_red);
        lg_sweep<NC, DK, SW_DOT>(rows, cost, s_v, s_out, s_red, xb, Hb);
        auto line_term = [&](float t) {
            float acc[1] = {0.f};
            for (int i = tid; i < n; i += LG_THREADS) {
                float ft[NC], dfr[NC], rt[NC], wt[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    dfr[c] = c < cols ? rows.df[(int64_t)i * cols + c] : 0.f;
                    ft[c] = c < cols ? fmaf(t, dfr[c], rows.f[(int64_t)i * cols + c]) : 0.f;
                }
                row_residual<NC>(ft, cols, rows.y[rows.tidx[i]], rt, wt);
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < cols) acc[0] = fmaf(cost * rt[c], dfr[c], acc[0]);
            }
            block_sum<1, LG_WAVES>(acc, s_red);
            return acc[0];
        };
        const float dphi0 = line_term(0.f) + lin[0];
        if (!(dphi0 < 0.f)) break;                  // no descent left in fp32: stop here, unconverged
        float t = 1.f;
        for (int ls = 0; ls < MDL_LOGIT_LS_MAX; ++ls) {
            const float dphi = line_term(t) + lin[0] + t * lin[1];
            if (dphi <= -0.5f * dphi0) break;
            t *= 0.5f;
        }
#pragma unroll
        for (int m = 0; m < EM; ++m)
            if (tid + LG_THREADS * m < L) Ww[tid + LG_THREADS * m] = fmaf(t, xs[m], Ww[tid + LG_THREADS * m]);
#pragma unroll
        for (int c = 0; c < NC; ++c) b[c] = fmaf(t, xb[c], b[c]);
        ++it;
        __syncthreads();                            // the next GRAD sweep's s_v is written after every thread has left this step
    }
    for (int e = tid; e < L; e += LG_THREADS)
        if (e % NC < cols) Wp[(int64_t)(e % NC) * d + e / NC] = Ww[e];
    if (cols > 1) {                                  // the common shift of b is free: return the zero-mean one
        float mean = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) mean += c < cols ? b[c] : 0.f;
        mean /= (float)cols;
#pragma unroll
        for (int c = 0; c < NC; ++c) b[c] -= mean;
    }
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < cols) b_out[(int64_t)p * cols + c] = b[c];
        info[(int64_t)p * 4 + 0] = (float)it;
        info[(int64_t)p * 4 + 1] = res <= gtol ? 1.f : 0.f;
        info[(int64_t)p * 4 + 2] = res;
        info[(int64_t)p * 4 + 3] = (float)cg_total;
    }
}

struct LogitArgs {
    const float* X;
    int64_t ldX;
    int S, d;
    const int32_t* y;
    int64_t ldy;
    const int32_t* train_idx;
    const int32_t* n_train;
    int64_t P;
    int n_max, C;
    float cost, gtol;
    int max_iter;
    float *W, *b, *info, *ws;
    hipStream_t stream;
};

template <int NC, int DK>
int lg_launch(const LogitArgs& a) {
    const size_t lds = 2 * (size_t)NC * a.d * sizeof(float);
    if (lds > 48 * 1024) {                          // d = 1024 at NC = 8 takes 64 KiB beside the static 176 bytes: the kernel's limit is raised
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&logit_fit_kernel<NC, DK>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 2 * NC * MDL_LOGIT_MAX_DIM * (int)sizeof(float));
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((logit_fit_kernel<NC, DK>), dim3((unsigned)a.P), dim3(LG_THREADS), lds, a.stream, a.X, a.ldX, a.S, a.d, a.y, a.ldy,
                       a.train_idx, a.n_train, a.n_max, a.C, a.cost, a.gtol, a.max_iter, a.W, a.b, a.info, a.ws, lg_npad_of(a.n_max));
    static_assert(NC == nc_of(NC), "the kernels are built for the column counts lg_nc_of returns");
    return MDL_OK;
}

template <int NC>
int lg_launch_dk(const LogitArgs& a) {
    const int dk = (a.d + WAVE - 1) / WAVE;
    if (dk <= 1) return lg_launch<NC, 1>(a);
    if (dk <= 2) return lg_launch<NC, 2>(a);
    if (dk <= 4) return lg_launch<NC, 4>(a);
    if (dk <= 8) return lg_launch<NC, 8>(a);
    if (dk <= 12) return lg_launch<NC, 12>(a);
    return lg_launch<NC, 16>(a);
}

constexpr ProbeLimits LOGIT_FIT = {MDL_LOGIT_MAX_TRAIN, MDL_LOGIT_MAX_DIM, PROBE_NO_LIMIT, true, true};      // {n_max, d, S, fit, classes}

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_logit_fit_ws_bytes(int64_t P, int n_max, int d, int C) {
    if (const int rc = probe_check(probe_sizes(P, n_max, 1, C, d), LOGIT_FIT, nullptr)) return rc;
    const int cols = cols_of(C);
    return P * (3 * lg_npad_of(n_max) * cols + (int64_t)d * nc_of(cols)) * (int64_t)sizeof(float);
}

extern "C" int mdl_logit_fit(const float* X, int64_t ldX, int64_t S, int d, const int32_t* y, int64_t ldy, const int32_t* train_idx,
                             const int32_t* n_train, int64_t P, int n_max, int C, float cost, float gtol, int max_iter, float* W_out,
                             float* b_out, float* info_out, void* ws, void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{y, ldy}}, 1, C, d};
    const int cols = cols_of(C);
    const ProbeExtra extra = {all_given(X, W_out, b_out, info_out, ws), mul_i32(P, cols, d), host_aligned16(ws), 0, ldX, max_iter, cost, gtol};
    if (const int rc = probe_check(t, LOGIT_FIT, &extra)) return rc;
    const LogitArgs a = {X, ldX, (int)S, d, y, ldy, train_idx, n_train, P, n_max, C, cost, gtol, max_iter, W_out, b_out, info_out,
                         reinterpret_cast<float*>(ws), (hipStream_t)stream};
    if (const int rc = for_nc(cols, [&](auto nc) { return lg_launch_dk<decltype(nc)::value>(a); })) return rc;
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
