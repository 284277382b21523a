// probe.hip -- the few-shot linear probe (P1-P3 of the header): P independent L2-regularised logistic fits over one embedding matrix,
// the decision values of every case under every fit, and confusion matrix + AUC per fit.
//
//   probe_gram_kernel     one workgroup per 64 x 64 tile of a problem's Gram matrix G = X_t X_t^T (X_t: its n <= 256 training rows),
//                         written to the workspace with leading dimension ldg (n_max rounded up to 64); padding rows give zeros.
//   probe_fit_kernel      one workgroup per problem, thread i owns training row i: Newton-CG on (A, b) with W = A^T X_t.  Every outer
//                         step forms W (in W_out) and the decision values x_i . W + b FROM W -- not from G A, whose fp32 cancellation
//                         would put the fixed point 1e-3 away from the optimum -- so the stop rule sees the gradient of what is returned;
//                         G only serves the Hessian-vector products of CG, where its rounding costs a little convergence rate and nothing
//                         else.  CG runs on the primal Newton system in coefficient form: inner product <(a, beta), (a', beta')> =
//                         a^T G a' + beta . beta', operator (a, beta) -> (a + cost D (G a + beta), cost 1^T D (G a + beta)); one G product
//                         per step.  The step length halves until the directional derivative, evaluated along the line, is no more than
//                         half as steep uphill as it was downhill at 0 (the objective is convex along the line).
//   probe_scores_kernel   a wave per 4 cases: z = X W^T + b.
//   probe_prepare_kernel  one workgroup per problem: which cases are test cases (and of which class), the confusion matrix, for C > 2
//                         the fp64 log-softmax scores; zeroes the problem's pair counters.
//   probe_pairs_kernel    exact Mann-Whitney counting, 2 per (positive, negative) pair ranked right and 1 per tie, one integer atomic
//                         per workgroup: the sum is the same whatever the order.
//   probe_auc_kernel      a thread per problem: the counts to AUC, in double.
// mdl_logit_metrics (L2 of the header) is the same three metrics kernels behind a launcher that accepts problem tables of up to
// MDL_LOGIT_MAX_TRAIN columns; the fits of that width are in probe_primal.hip.
// No workgroup waits on another; every loop has a bound that is an argument or a constant of the header.
#include "probe_host.hpp"

namespace mdl {
namespace {

constexpr int PB_THREADS = 256;
constexpr int PB_WAVES = PB_THREADS / WAVE;
constexpr int PB_NMAX = MDL_PROBE_MAX_TRAIN;
constexpr int PB_CMAX = PROBE_CMAX;
static_assert(PB_NMAX == PB_THREADS, "the fit kernel gives one thread to each training row");

// ---- Gram -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB_THREADS) void probe_gram_kernel(const float* __restrict__ X, int64_t ldX, int S, int d,
                                                                const int32_t* __restrict__ train_idx,
                                                                const int32_t* __restrict__ n_train, int n_max, int ldg,
                                                                float* __restrict__ G) {
    const int tps = ldg / GRAM_TILE;
    const int p = blockIdx.x / (tps * tps), tile = blockIdx.x % (tps * tps);
    const int ti = tile / tps, tj = tile % tps;
    int n = n_train[p];
    if (n < 0 || n > n_max) n = 0;                    // a refused problem: the fit kernel never reads its G
    if (ti * GRAM_TILE >= n || tj * GRAM_TILE >= n) return;
    __shared__ float sA[GRAM_KC][GRAM_TILE + 1], sB[GRAM_KC][GRAM_TILE + 1];
    __shared__ int64_t s_off[2][GRAM_TILE];           // element offset of the tile's rows in X, -1: a zero row
    const int tid = threadIdx.x;
    if (tid < 2 * GRAM_TILE) {
        const int side = tid / GRAM_TILE, r = tid % GRAM_TILE;
        const int row = (side ? tj : ti) * GRAM_TILE + r;
        int64_t off = -1;
        if (row < n) {
            const int idx = train_idx[(int64_t)p * n_max + row];
            if (idx >= 0 && idx < S) off = (int64_t)idx * ldX;
        }
        s_off[side][r] = off;
    }
    __syncthreads();
    gram_tile<PB_THREADS>(X, d, s_off, sA, sB, G + (int64_t)p * ldg * ldg, ldg, ti, tj);
}

// ---- fit --------------------------------------------------------------------------------------------------------------------------
// out[c] (column j of X_t^T V) for the columns j = tid, tid + 256, ... handed to `sink`; V = s_v [n][NC]
template <int NC, class Sink>
__device__ __forceinline__ void xt_times(const float* __restrict__ X, const int64_t* s_off, int n, int d, const float* s_v, Sink sink) {
    for (int j = threadIdx.x; j < d; j += PB_THREADS) {
        float acc[NC] = {};
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const float x = X[s_off[i] + j];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = fmaf(x, s_v[i * NC + c], acc[c]);
        }
        sink(j, acc);
    }
}

template <int NC>
__global__ __launch_bounds__(PB_THREADS) void probe_fit_kernel(const float* __restrict__ X, int64_t ldX, int S, int d,
                                                               const int32_t* __restrict__ y, int64_t ldy,
                                                               const int32_t* __restrict__ train_idx, const int32_t* __restrict__ n_train,
                                                               int n_max, int C, float cost, float gtol, int max_iter, float* W_out,
                                                               float* __restrict__ b_out, float* __restrict__ info,
                                                               const float* __restrict__ G, int ldg) {
    __shared__ float s_v[PB_NMAX * NC];            // the vector every thread needs: input of G v and of X_t^T V
    __shared__ float s_f[PB_NMAX * NC];            // decision values of the training rows, from the waves that form them
    __shared__ int64_t s_off[PB_NMAX];
    __shared__ float s_red[PB_WAVES][PB_CMAX + 3];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int p = blockIdx.x, cols = cols_of(C);
    float* Wp = W_out + (int64_t)p * cols * d;
    const float* Gp = G + (int64_t)p * ldg * ldg;

    const int n = n_train[p];
    int bad = (n < 1 || n > n_max) ? 1 : 0;
    int label = 0;
    const bool row = !bad && tid < n;
    if (row) {
        const int idx = train_idx[(int64_t)p * n_max + tid];
        if (idx < 0 || idx >= S) {
            bad = 1;
        } else {
            s_off[tid] = (int64_t)idx * ldX;
            label = y[(int64_t)p * ldy + idx];
            if (label < 0 || label >= C) bad = 1;
        }
    }
    if (__syncthreads_or(bad)) {                    // refused: NaN, converged = 0; nothing of X is read
        const float nan = __builtin_nanf("");
        for (int e = tid; e < cols * d; e += PB_THREADS) Wp[e] = nan;
        if (tid < cols) b_out[(int64_t)p * cols + tid] = nan;
        if (tid < 4) info[(int64_t)p * 4 + tid] = tid == 2 ? nan : 0.f;
        return;
    }

    float a[NC] = {}, b[NC] = {}, f[NC] = {}, r[NC] = {}, w[NC] = {}, u[NC] = {};
    float res = 0.f, prev = __builtin_inff();
    int it = 0, cg_total = 0;
    for (;;) {
        // W = X_t^T A, into W_out
#pragma unroll
        for (int c = 0; c < NC; ++c) s_v[tid * NC + c] = a[c];
        __syncthreads();
        xt_times<NC>(X, s_off, n, d, s_v, [&](int j, const float (&acc)[NC]) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < cols) Wp[(int64_t)c * d + j] = acc[c];
        });
        __syncthreads();
        // f_i = x_i . W + b from W itself: a wave per row
        for (int i = wave; i < n; i += PB_WAVES) {
            float acc[NC] = {};
            const float* x = X + s_off[i];
            for (int j = lane; j < d; j += WAVE) {
                const float xv = x[j];
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < cols) acc[c] = fmaf(xv, Wp[(int64_t)c * d + j], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = wave_sum(acc[c]);
            if (lane == 0)
#pragma unroll
                for (int c = 0; c < NC; ++c) s_f[i * NC + c] = acc[c];
        }
        __syncthreads();
        float xw[NC] = {};                          // x_i . W = (G A)_i
        if (row) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                xw[c] = c < cols ? s_f[tid * NC + c] : 0.f;
                f[c] = xw[c] + b[c];
            }
            row_residual<NC>(f, cols, label, r, w);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                r[c] = c < cols ? r[c] : 0.f;
                u[c] = fmaf(cost, r[c], a[c]);
            }
        }
        // the primal gradient: X_t^T U with respect to W, cost sum_i r_i with respect to b
#pragma unroll
        for (int c = 0; c < NC; ++c) s_v[tid * NC + c] = u[c];
        __syncthreads();
        float gmax = 0.f;
        xt_times<NC>(X, s_off, n, d, s_v, [&](int, const float (&acc)[NC]) {
#pragma unroll
            for (int c = 0; c < NC; ++c) gmax = fmaxf(gmax, fabsf(acc[c]));
        });
        float gb[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) gb[c] = cost * r[c];
        block_sum<NC, PB_WAVES>(gb, s_red);                   // its barriers also free s_v
#pragma unroll
        for (int c = 0; c < NC; ++c) gmax = fmaxf(gmax, fabsf(gb[c]));
        res = block_max<PB_WAVES>(gmax, s_red);
        // The internal stop is tighter than gtol: Newton's last steps square the residual, and stopping at the first residual below
        // gtol leaves the decision values of a k = 1 problem 3e-3 (relative) off the optimum.  Below gtol the iteration also ends as
        // soon as a step no longer halves the residual (the fp32 floor).
        if (res <= PROBE_TIGHT * gtol || (res <= gtol && res >= 0.5f * prev)) break;
        if (it >= max_iter || !(res == res)) break;
        prev = res;

        // ---- CG on the Newton system, right-hand side (-U, -gb) ----
        float xa[NC] = {}, Gx[NC] = {}, xb[NC] = {};
        float ra[NC], rb[NC], pa[NC], pb[NC], Gr[NC], Gpd[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            ra[c] = -u[c];
            rb[c] = -gb[c];
        }
        auto g_times = [&](const float (&v)[NC], float (&out)[NC]) {      // out = (G V)_tid; G is symmetric: column tid, coalesced
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                s_v[tid * NC + c] = v[c];
                out[c] = 0.f;
            }
            __syncthreads();
            if (row) {
#pragma unroll 8
                for (int j = 0; j < n; ++j) {
                    const float g = Gp[(int64_t)j * ldg + tid];
#pragma unroll
                    for (int c = 0; c < NC; ++c) out[c] = fmaf(g, s_v[j * NC + c], out[c]);
                }
            }
            __syncthreads();
        };
        auto norm2 = [&](const float (&va)[NC], const float (&Gva)[NC], const float (&vb)[NC]) {
            float s[1] = {0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) s[0] = fmaf(va[c], Gva[c], s[0]);
            block_sum<1, PB_WAVES>(s, s_red);
#pragma unroll
            for (int c = 0; c < NC; ++c) s[0] = fmaf(vb[c], vb[c], s[0]);
            return s[0];
        };
        g_times(ra, Gr);
        float rho = norm2(ra, Gr, rb);
        const float rho0 = rho;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            pa[c] = ra[c];
            pb[c] = rb[c];
            Gpd[c] = Gr[c];
        }
        for (int k = 0; k < MDL_PROBE_CG_MAX && rho > 0.f; ++k) {
            float q[NC], Dq[NC], Ma[NC], red[NC + 1];
#pragma unroll
            for (int c = 0; c < NC; ++c) q[c] = (row && c < cols) ? Gpd[c] + pb[c] : 0.f;
            row_hess<NC>(w, cols, q, Dq);
            red[NC] = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                Dq[c] = (row && c < cols) ? Dq[c] : 0.f;
                Ma[c] = fmaf(cost, Dq[c], pa[c]);
                red[c] = Dq[c];
                red[NC] = fmaf(Gpd[c], Ma[c], red[NC]);
            }
            block_sum<NC + 1, PB_WAVES>(red, s_red);
            float pMp = red[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) pMp = fmaf(pb[c], cost * red[c], pMp);
            if (!(pMp > 0.f)) break;
            const float alpha = rho / pMp;
            ++cg_total;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                xa[c] = fmaf(alpha, pa[c], xa[c]);
                Gx[c] = fmaf(alpha, Gpd[c], Gx[c]);
                xb[c] = fmaf(alpha, pb[c], xb[c]);
                ra[c] = fmaf(-alpha, Ma[c], ra[c]);
                rb[c] = fmaf(-alpha, cost * red[c], rb[c]);
            }
            g_times(ra, Gr);
            const float rho_new = norm2(ra, Gr, rb);
            if (!(rho_new > PROBE_CG_TOL2 * rho0)) break;
            const float beta = rho_new / rho;
            rho = rho_new;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                pa[c] = fmaf(beta, pa[c], ra[c]);
                pb[c] = fmaf(beta, pb[c], rb[c]);
                Gpd[c] = fmaf(beta, Gpd[c], Gr[c]);
            }
        }

        // ---- step length along (xa, xb): phi'(t) = sum cost r(f + t df) . df + t xa^T G xa + xa^T G a ----
        float df[NC], lin[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            df[c] = (row && c < cols) ? Gx[c] + xb[c] : 0.f;
            lin[0] = fmaf(cost * r[c], df[c], lin[0]);
            lin[1] = fmaf(xa[c], xw[c], lin[1]);
            lin[2] = fmaf(xa[c], Gx[c], lin[2]);
        }
        block_sum<3, PB_WAVES>(lin, s_red);
        const float dphi0 = lin[0] + lin[1];
        if (!(dphi0 < 0.f)) break;                  // no descent left in fp32: stop here, unconverged
        float t = 1.f;
        for (int ls = 0; ls < MDL_PROBE_LS_MAX; ++ls) {
            float ft[NC], rt[NC], wt[NC], s[1] = {0.f};
            if (row) {
#pragma unroll
                for (int c = 0; c < NC; ++c) ft[c] = fmaf(t, df[c], f[c]);
                row_residual<NC>(ft, cols, label, rt, wt);
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < cols) s[0] = fmaf(cost * rt[c], df[c], s[0]);
            }
            block_sum<1, PB_WAVES>(s, s_red);
            const float dphi = s[0] + lin[1] + t * lin[2];
            if (dphi <= -0.5f * dphi0) break;
            t *= 0.5f;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            a[c] = fmaf(t, xa[c], a[c]);
            b[c] = fmaf(t, xb[c], b[c]);
        }
        ++it;
    }
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

// ---- decision values --------------------------------------------------------------------------------------------------------------
constexpr int SC_ROWS = 4;                           // cases per wave
template <int NC>
__global__ __launch_bounds__(PB_THREADS) void probe_scores_kernel(const float* __restrict__ X, int64_t ldX, int S, int d,
                                                                  const float* __restrict__ W, const float* __restrict__ b, int cols,
                                                                  int tiles, float* __restrict__ z) {
    const int p = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int s0 = (tile * PB_WAVES + wave) * SC_ROWS;
    if (s0 >= S) return;
    const float* Wp = W + (int64_t)p * cols * d;
    float acc[SC_ROWS][NC] = {};
    for (int j = lane; j < d; j += WAVE) {
        float wv[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) wv[c] = c < cols ? Wp[(int64_t)c * d + j] : 0.f;
#pragma unroll
        for (int q = 0; q < SC_ROWS; ++q) {
            const float x = s0 + q < S ? X[(int64_t)(s0 + q) * ldX + j] : 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[q][c] = fmaf(x, wv[c], acc[q][c]);
        }
    }
#pragma unroll
    for (int q = 0; q < SC_ROWS; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float v = wave_sum(acc[q][c]);
            if (lane == 0 && c < cols && s0 + q < S) z[((int64_t)p * S + s0 + q) * cols + c] = v + b[(int64_t)p * cols + c];
        }
}

// ---- metrics ----------------------------------------------------------------------------------------------------------------------
// workspace: tcls [P][S16] int8 (test class, -1: not a test case), cnt [P][PB_CMAX] uint64, score [P][C][S] double (C > 2 only)
struct MetricsWs {
    int8_t* tcls;
    unsigned long long* cnt;
    double* score;
};
inline MetricsWs metrics_ws(void* ws, int64_t P, int64_t S) {
    MetricsWs m;
    m.tcls = reinterpret_cast<int8_t*>(ws);
    m.cnt = reinterpret_cast<unsigned long long*>(m.tcls + P * s16_of(S));
    m.score = reinterpret_cast<double*>(m.cnt + P * PB_CMAX);
    return m;
}

__global__ __launch_bounds__(PB_THREADS) void probe_prepare_kernel(const float* __restrict__ z, const int32_t* __restrict__ y, int64_t ldy,
                                                                   const int32_t* __restrict__ train_idx,
                                                                   const int32_t* __restrict__ n_train, int n_max, int S, int C,
                                                                   int32_t* __restrict__ confusion, MetricsWs m, int64_t S8) {
    __shared__ int s_conf[PB_CMAX * PB_CMAX];
    const int tid = threadIdx.x, p = blockIdx.x, cols = cols_of(C);
    int8_t* tcls = m.tcls + (int64_t)p * S8;
    const int32_t* yp = y + (int64_t)p * ldy;
    if (tid < PB_CMAX) m.cnt[(int64_t)p * PB_CMAX + tid] = 0ull;
    if (tid < PB_CMAX * PB_CMAX) s_conf[tid] = 0;
    for (int s = tid; s < S; s += PB_THREADS) tcls[s] = probe_test_class(yp[s], C);
    __syncthreads();
    strike_training<PB_THREADS>(tcls, train_idx, n_train, p, n_max, S);
    __syncthreads();
    for (int s = tid; s < S; s += PB_THREADS) {
        const int t = tcls[s];
        if (t < 0) continue;
        const int pred = probe_predict(z + ((int64_t)p * S + s) * cols, cols, m.score + (int64_t)p * C * S + s, S);
        atomicAdd(&s_conf[t * C + pred], 1);
    }
    __syncthreads();
    if (tid < C * C) confusion[(int64_t)p * C * C + tid] = s_conf[tid];
}

__global__ __launch_bounds__(PB_THREADS) void probe_pairs_kernel(const float* __restrict__ z, int S, int C, int slices, MetricsWs m,
                                                                 int64_t S8) {
    __shared__ double s_sc[PB_THREADS];
    __shared__ int s_neg[PB_THREADS];
    __shared__ int s_cnt[PB_WAVES];
    const int tid = threadIdx.x;
    const int ncls = C == 2 ? 1 : C;
    const int slice = blockIdx.x % slices, rest = blockIdx.x / slices;
    const int ci = rest % ncls, p = rest / ncls;
    const int cpos = C == 2 ? 1 : ci;
    const int8_t* tcls = m.tcls + (int64_t)p * S8;
    const double* sc = m.score + ((int64_t)p * C + ci) * S;
    const float* zp = z + (int64_t)p * S;             // C == 2: cols = 1
    const int i = slice * PB_THREADS + tid;
    const bool pos = i < S && tcls[i] == cpos;
    if (!__syncthreads_or(pos ? 1 : 0)) return;
    const double mine = pos ? (C == 2 ? (double)zp[i] : sc[i]) : 0.0;
    int cnt = 0;
    for (int j0 = 0; j0 < S; j0 += PB_THREADS) {
        const int j = j0 + tid;
        int neg = 0;
        double v = 0.0;
        if (j < S) {
            const int t = tcls[j];
            neg = (t >= 0 && t != cpos) ? 1 : 0;
            if (neg) v = C == 2 ? (double)zp[j] : sc[j];
        }
        s_sc[tid] = v;
        s_neg[tid] = neg;
        __syncthreads();
        if (pos) {
            const int lim = S - j0 < PB_THREADS ? S - j0 : PB_THREADS;
            for (int jj = 0; jj < lim; ++jj)
                if (s_neg[jj]) cnt += mine > s_sc[jj] ? 2 : (mine == s_sc[jj] ? 1 : 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);      // at most 2 * 256 * 16384 per workgroup: fits an int
    if ((tid & (WAVE - 1)) == 0) s_cnt[tid / WAVE] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (total) atomicAdd(&m.cnt[(int64_t)p * PB_CMAX + ci], (unsigned long long)total);
    }
}

__global__ __launch_bounds__(PB_THREADS) void probe_auc_kernel(const int32_t* __restrict__ confusion, int P, int C, MetricsWs m,
                                                               float* __restrict__ auc) {
    const int p = blockIdx.x * PB_THREADS + threadIdx.x;
    if (p >= P) return;
    const int32_t* cf = confusion + (int64_t)p * C * C;
    double rows[PB_CMAX], total = 0.0;
    for (int t = 0; t < C; ++t) {
        rows[t] = 0.0;
        for (int q = 0; q < C; ++q) rows[t] += (double)cf[t * C + q];
        total += rows[t];
    }
    double out = 0.0;
    const int ncls = C == 2 ? 1 : C;
    for (int ci = 0; ci < ncls; ++ci) {
        const double npos = rows[C == 2 ? 1 : ci], nneg = total - npos;
        if (npos == 0.0 || nneg == 0.0) {
            out = __builtin_nan("");
            break;
        }
        out += 0.5 * (double)m.cnt[(int64_t)p * PB_CMAX + ci] / (npos * nneg);
    }
    auc[p] = (float)(out / (double)ncls);
}

// the limits of the entry points: {n_max, d, S, fit, classes}
constexpr ProbeLimits PROBE_FIT = {PB_NMAX, PROBE_NO_LIMIT, PROBE_NO_LIMIT, true, true};
constexpr ProbeLimits PROBE_METRICS = {PB_NMAX, PROBE_NO_LIMIT, MDL_PROBE_MAX_CASES, false, true};
constexpr ProbeLimits LOGIT_METRICS = {MDL_LOGIT_MAX_TRAIN, PROBE_NO_LIMIT, MDL_PROBE_MAX_CASES, false, true};

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_probe_fit_ws_bytes(int64_t P, int n_max, int d, int C) {
    if (const int rc = probe_check(probe_sizes(P, n_max, 1, C, d), PROBE_FIT, nullptr)) return rc;
    const int64_t ldg = gram_ld(n_max);
    return P * ldg * ldg * (int64_t)sizeof(float);
}

extern "C" int mdl_probe_fit(const float* X, int64_t ldX, int64_t S, int d, const int32_t* y, int64_t ldy, const int32_t* train_idx,
                             const int32_t* n_train, int64_t P, int n_max, int C, float cost, float gtol, int max_iter, float* W_out,
                             float* b_out, float* info_out, void* ws, void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{y, ldy}}, 1, C, d};
    const int64_t ldg = gram_ld(n_max), tps = ldg / GRAM_TILE;
    const int cols = cols_of(C);
    const ProbeExtra extra = {all_given(X, W_out, b_out, info_out, ws), mul_i32(P, tps, tps) && mul_i32(P, cols, d), host_aligned16(ws), 0,
                              ldX, max_iter, cost, gtol};
    if (const int rc = probe_check(t, PROBE_FIT, &extra)) return rc;
    float* G = reinterpret_cast<float*>(ws);
    hipLaunchKernelGGL(probe_gram_kernel, dim3((unsigned)(P * tps * tps)), dim3(PB_THREADS), 0, (hipStream_t)stream, X, ldX, (int)S, d,
                       train_idx, n_train, n_max, (int)ldg, G);
    MDL_LAUNCH_CHECK();
    for_nc(cols, [&](auto nc) {
        hipLaunchKernelGGL(probe_fit_kernel<decltype(nc)::value>, dim3((unsigned)P), dim3(PB_THREADS), 0, (hipStream_t)stream, X, ldX,
                           (int)S, d, y, ldy, train_idx, n_train, n_max, C, cost, gtol, max_iter, W_out, b_out, info_out, (const float*)G,
                           (int)ldg);
        return MDL_OK;
    });
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int mdl_probe_scores(const float* X, int64_t ldX, int64_t S, int d, const float* W, const float* b, int64_t P, int C,
                                float* z_out, void* stream) {
    if (!all_given(X, W, b, z_out)) return MDL_E_ARG;
    if (d < 1 || ldX < d || P < 1 || S < 1) return MDL_E_ARG;
    if (C < 2 || C > PB_CMAX) return MDL_E_UNSUPPORTED;
    const int cols = cols_of(C);
    const int64_t tiles = ceil_div(S, PB_WAVES * SC_ROWS);
    if (!i32(S) || !mul_i32(P, tiles) || !mul_i32(P, cols, d)) return MDL_E_UNSUPPORTED;
    for_nc(cols, [&](auto nc) {
        hipLaunchKernelGGL(probe_scores_kernel<decltype(nc)::value>, dim3((unsigned)(P * tiles)), dim3(PB_THREADS), 0, (hipStream_t)stream, X,
                           ldX, (int)S, d, W, b, cols, (int)tiles, z_out);
        return MDL_OK;
    });
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int64_t mdl_probe_metrics_ws_bytes(int64_t P, int64_t S, int C) {
    if (const int rc = probe_check(probe_sizes(P, 1, S, C, 0), PROBE_METRICS, nullptr)) return rc;
    return P * s16_of(S) + P * PB_CMAX * (int64_t)sizeof(unsigned long long) + (C > 2 ? P * C * S * (int64_t)sizeof(double) : 0);
}

// the three metrics launches behind mdl_probe_metrics and mdl_logit_metrics, which differ in the widest problem table they accept
static int launch_metrics(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train, int64_t P,
                          int n_max, const ProbeLimits& lim, int64_t S, int C, int32_t* confusion_out, float* auc_out, void* ws,
                          void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{y, ldy}}, 1, C, 0};
    const int ncls = cols_of(C);
    const int64_t slices = ceil_div(S, PB_THREADS);
    const ProbeExtra extra = {all_given(z, confusion_out, auc_out, ws), mul_i32(P, ncls, slices), host_aligned16(ws)};
    if (const int rc = probe_check(t, lim, &extra)) return rc;
    const MetricsWs m = metrics_ws(ws, P, S);
    const int64_t S16 = s16_of(S);
    hipLaunchKernelGGL(probe_prepare_kernel, dim3((unsigned)P), dim3(PB_THREADS), 0, (hipStream_t)stream, z, y, ldy, train_idx, n_train,
                       n_max, (int)S, C, confusion_out, m, S16);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(probe_pairs_kernel, dim3((unsigned)(P * ncls * slices)), dim3(PB_THREADS), 0, (hipStream_t)stream, z, (int)S, C,
                       (int)slices, m, S16);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(probe_auc_kernel, dim3((unsigned)((P + PB_THREADS - 1) / PB_THREADS)), dim3(PB_THREADS), 0, (hipStream_t)stream,
                       (const int32_t*)confusion_out, (int)P, C, m, auc_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int mdl_probe_metrics(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train,
                                 int64_t P, int n_max, int64_t S, int C, int32_t* confusion_out, float* auc_out, void* ws, void* stream) {
    return launch_metrics(z, y, ldy, train_idx, n_train, P, n_max, PROBE_METRICS, S, C, confusion_out, auc_out, ws, stream);
}

extern "C" int64_t mdl_logit_metrics_ws_bytes(int64_t P, int64_t S, int C) { return mdl_probe_metrics_ws_bytes(P, S, C); }

extern "C" int mdl_logit_metrics(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train,
                                 int64_t P, int n_max, int64_t S, int C, int32_t* confusion_out, float* auc_out, void* ws, void* stream) {
    return launch_metrics(z, y, ldy, train_idx, n_train, P, n_max, LOGIT_METRICS, S, C, confusion_out, auc_out, ws, stream);
}
