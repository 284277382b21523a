// survival.hip -- the survival probe (S1-S2 of the header): P independent ridge-penalised Cox proportional-hazards fits (Breslow ties, no
// intercept) over one embedding matrix, and per fit Harrell's concordance index and a median-split log-rank statistic over the held-out
// cases.  The decision values of every case under every fit come from mdl_probe_scores (C = 2, zero intercept).
//
//   cox_order_kernel    one workgroup per problem: checks the training list and sorts it into the workspace by (time descending, case
//                       index ascending) -- a total order, found by rank counting, so the fit does not depend on the caller's list order.
//   cox_gram_kernel     one workgroup per 64 x 64 tile of a problem's Gram matrix G = X_t X_t^T over the SORTED rows (the tiling of
//                       probe_gram_kernel, which is left as it is; leading dimension up to 1024).
//   cox_fit_kernel      one workgroup of 1024 threads per problem, thread i owns sorted row i: Newton-CG on the coefficients a with
//                       w = X_t^T a, as probe_fit_kernel.  With f = X_t w, e = exp(f - max f): S0_i = sum_{R_i} e is an inclusive prefix
//                       sum read at the END of row i's tie group, A_j = sum_{events i, t_i <= t_j} 1 / S0_i a suffix sum read at the START
//                       of row j's; the gradient in f is r = -event + e A, the Hessian (H u)_j = e_j (u_j A_j - B_j) with B a suffix sum
//                       over prefix sums of e u.  Every outer step forms w (in W_out) and f FROM w, so the stop rule sees the gradient of
//                       what is returned; G only serves CG's Hessian-vector products (one G product and two scans each).  The step length
//                       halves until the derivative along the line (two scans per trial) is at most half as steep uphill as it was
//                       downhill at 0.  It also writes the median of the training rows' decision values (rank counting).
//   surv_prepare_kernel one workgroup per problem: which cases are test cases, their event flag and risk group; zeroes the pair counter.
//   surv_pairs_kernel   O(S^2) tiles: per test event case the sizes of its risk set (all / high group) and of its tie group of events, and
//                       the concordance counts -- integers, one 64-bit integer atomic per workgroup: no sum depends on an order.
//   surv_finish_kernel  one workgroup per problem: the log-rank sums in double in a fixed order, c_index, chi2, the counts.
// No workgroup waits on another; every loop has a bound that is an argument or a constant of the header.
#include "probe_host.hpp"

namespace mdl {
namespace {

constexpr int CX_THREADS = 1024;
constexpr int CX_WAVES = CX_THREADS / WAVE;
constexpr int CX_NMAX = MDL_COX_MAX_TRAIN;
constexpr int CX_GRAM_THREADS = 256;
constexpr int SV_THREADS = 256;
constexpr int SV_WAVES = SV_THREADS / WAVE;
static_assert(CX_NMAX == CX_THREADS, "the fit kernel gives one thread to each training row");

// workspace of the fit: status [P] int32 (1: refused), order [P][n_max] int32 (the sorted case indices), G [P][ldg][ldg] fp32
struct CoxWs {
    int32_t* status;
    int32_t* order;
    float* G;
};
inline CoxWs cox_ws(void* ws, int64_t P, int n_max) {
    CoxWs c;
    char* base = reinterpret_cast<char*>(ws);
    c.status = reinterpret_cast<int32_t*>(base);
    c.order = reinterpret_cast<int32_t*>(base + up16(P * 4));
    c.G = reinterpret_cast<float*>(base + up16(P * 4) + up16(P * n_max * 4));
    return c;
}

// ---- order ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CX_THREADS) void cox_order_kernel(const float* __restrict__ time, int64_t ldt, const int32_t* __restrict__ event,
                                                              int64_t lde, int S, const int32_t* __restrict__ train_idx,
                                                              const int32_t* __restrict__ n_train, int n_max, CoxWs c) {
    __shared__ float s_t[CX_NMAX];
    __shared__ int s_idx[CX_NMAX];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int n = n_train[p];
    int bad = (n < 1 || n > n_max) ? 1 : 0;
    const bool row = !bad && tid < n;
    float t = 0.f;
    int idx = -1;
    if (row) {
        idx = train_idx[(int64_t)p * n_max + tid];
        if (idx < 0 || idx >= S) {
            bad = 1;
        } else {
            t = time[(int64_t)p * ldt + idx];
            const int ev = event[(int64_t)p * lde + idx];
            if ((ev != 0 && ev != 1) || !(t >= 0.f) || !(t < __builtin_inff())) bad = 1;      // NaN fails both comparisons
        }
        s_t[tid] = t;
        s_idx[tid] = idx;
    }
    bad = __syncthreads_or(bad);
    int rank = 0;
    if (!bad && row) {
        for (int j = 0; j < n; ++j) {
            const float tj = s_t[j];
            const int ij = s_idx[j];
            rank += (tj > t || (tj == t && ij < idx)) ? 1 : 0;
            if (ij == idx && j != tid) bad = 1;      // a repeated index
        }
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) c.status[p] = bad;
    if (!bad && row) c.order[(int64_t)p * n_max + rank] = idx;      // distinct keys: the ranks are a permutation of 0 .. n - 1
}

// ---- Gram -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CX_GRAM_THREADS) void cox_gram_kernel(const float* __restrict__ X, int64_t ldX, int d,
                                                                  const int32_t* __restrict__ n_train, int n_max, int ldg, CoxWs c) {
    const int tps = ldg / GRAM_TILE;
    const int p = blockIdx.x / (tps * tps), tile = blockIdx.x % (tps * tps);
    const int ti = tile / tps, tj = tile % tps;
    const int n = c.status[p] ? 0 : n_train[p];       // a refused problem: the fit kernel never reads its G
    if (ti * GRAM_TILE >= n || tj * GRAM_TILE >= n) return;
    __shared__ float sA[GRAM_KC][GRAM_TILE + 1], sB[GRAM_KC][GRAM_TILE + 1];
    __shared__ int64_t s_off[2][GRAM_TILE];           // element offset of the tile's rows in X, -1: a zero row
    const int tid = threadIdx.x;
    if (tid < 2 * GRAM_TILE) {
        const int side = tid / GRAM_TILE, r = tid % GRAM_TILE;
        const int row = (side ? tj : ti) * GRAM_TILE + r;
        s_off[side][r] = row < n ? (int64_t)c.order[(int64_t)p * n_max + row] * ldX : -1;      // the order kernel checked the range
    }
    __syncthreads();
    gram_tile<CX_GRAM_THREADS>(X, d, s_off, sA, sB, c.G + (int64_t)p * ldg * ldg, ldg, ti, tj);
}

// ---- fit --------------------------------------------------------------------------------------------------------------------------
// The LDS of the fit kernel.  v: the vector every thread needs (input of G v and of X_t^T v); f: decision values from the waves that
// form them, then the scans' results; off: element offset of each sorted row in X; red: the reductions' wave partials.
struct CoxLds {
    float v[CX_NMAX];
    float f[CX_NMAX];
    int64_t off[CX_NMAX];
    float red[CX_WAVES][2];
};

// Inclusive sum over the sorted positions 0 .. tid (REV: tid .. 1023), read at position `at`: within the wave by shuffles, the waves
// before (after) it added in position order.  A fixed order: the same bits whatever else runs.  Three barriers.
template <bool REV>
__device__ __forceinline__ float scan_at(float v, int at, CoxLds& s) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const float t = REV ? __shfl_down(v, o, WAVE) : __shfl_up(v, o, WAVE);
        if (REV ? lane + o < WAVE : lane >= o) v += t;
    }
    if (lane == (REV ? 0 : WAVE - 1)) s.red[wave][0] = v;
    __syncthreads();
    float base = 0.f;
    if (REV) {
        for (int w = CX_WAVES - 1; w > wave; --w) base += s.red[w][0];
    } else {
        for (int w = 0; w < wave; ++w) base += s.red[w][0];
    }
    s.f[tid] = v + base;
    __syncthreads();
    const float out = s.f[at];
    __syncthreads();
    return out;
}

// What a thread keeps of its sorted row between the steps
struct CoxRow {
    bool row;        // tid < n
    float ev;        // 1: event, 0: censored (or no row)
    int gs, ge;      // first and last position of the row's tie group
};

// At decision values f: e = exp(f - max f), inv = event / S0, A, and the gradient in f, r = -event + e A.  Rows that are none: all 0.
__device__ __forceinline__ float cox_residual(float f, const CoxRow& me, float& e, float& inv, float& A, CoxLds& s) {
    const float m = block_max<CX_WAVES>(me.row ? f : -__builtin_inff(), s.red);
    e = me.row ? expf(f - m) : 0.f;
    const float S0 = scan_at<false>(e, me.ge, s);
    inv = me.ev != 0.f ? 1.f / S0 : 0.f;
    A = scan_at<true>(inv, me.gs, s);
    return me.row ? fmaf(e, A, -me.ev) : 0.f;
}

// (H q) of the thread's row: the Hessian of the partial likelihood with respect to the decision values, applied to q
__device__ __forceinline__ float cox_hess(float q, const CoxRow& me, float e, float inv, float A, CoxLds& s) {
    const float inner = scan_at<false>(e * q, me.ge, s);
    const float B = scan_at<true>(inner * inv * inv, me.gs, s);
    return me.row ? e * (q * A - B) : 0.f;
}

// column j of X_t^T v for j = tid, tid + 1024, ... handed to `sink`; v = s.v [n]
template <class Sink>
__device__ __forceinline__ void xt_times(const float* __restrict__ X, const CoxLds& s, int n, int d, Sink sink) {
    for (int j = threadIdx.x; j < d; j += CX_THREADS) {
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < n; ++i) acc = fmaf(X[s.off[i] + j], s.v[i], acc);
        sink(j, acc);
    }
}

__global__ __launch_bounds__(CX_THREADS) void cox_fit_kernel(const float* __restrict__ X, int64_t ldX, int d, const float* __restrict__ time,
                                                            int64_t ldt, const int32_t* __restrict__ event, int64_t lde,
                                                            const int32_t* __restrict__ n_train, int n_max, float cost, float gtol,
                                                            int max_iter, float* W_out, float* __restrict__ thr_out,
                                                            float* __restrict__ info, CoxWs c, int ldg) {
    __shared__ CoxLds s;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int p = blockIdx.x;
    float* Wp = W_out + (int64_t)p * d;
    const float* Gp = c.G + (int64_t)p * ldg * ldg;

    if (c.status[p]) {                               // refused by the order kernel: NaN, converged = 0; nothing of X is read
        const float nan = __builtin_nanf("");
        for (int e = tid; e < d; e += CX_THREADS) Wp[e] = nan;
        if (tid == 0) thr_out[p] = nan;
        if (tid < 4) info[(int64_t)p * 4 + tid] = tid == 2 ? nan : 0.f;
        return;
    }
    const int n = n_train[p];
    CoxRow me;
    me.row = tid < n;
    me.ev = 0.f;
    me.gs = me.ge = tid;
    float t = -1.f;                                  // rows that are none: a time no training row has
    if (me.row) {
        const int idx = c.order[(int64_t)p * n_max + tid];
        s.off[tid] = (int64_t)idx * ldX;
        t = time[(int64_t)p * ldt + idx];
        me.ev = event[(int64_t)p * lde + idx] ? 1.f : 0.f;
    }
    s.v[tid] = t;
    __syncthreads();
    if (me.row) {                                    // times descend: the tie group is the positions with an equal time
        int above = 0, not_below = 0;
        for (int j = 0; j < n; ++j) {
            const float tj = s.v[j];
            above += tj > t ? 1 : 0;
            not_below += tj >= t ? 1 : 0;
        }
        me.gs = above;
        me.ge = not_below - 1;
    }
    __syncthreads();

    float a = 0.f, f = 0.f, e = 0.f, inv = 0.f, A = 0.f, r = 0.f, u = 0.f;
    float res = 0.f, prev = __builtin_inff(), g0 = 0.f;
    int it = 0, cg_total = 0;
    for (;;) {
        // w = X_t^T a, into W_out
        s.v[tid] = a;
        __syncthreads();
        xt_times(X, s, n, d, [&](int j, float acc) { Wp[j] = acc; });
        __syncthreads();
        // f_i = x_i . w from w itself: a wave per row, in the order of probe_scores_kernel (lane j, j + 64, ... as one fmaf chain, then
        // wave_sum), so that f equals the score mdl_probe_scores gives the row bit for bit and thr_out is the median of those scores
        for (int i = wave; i < n; i += CX_WAVES) {
            float acc = 0.f;
            const float* x = X + s.off[i];
            for (int j = lane; j < d; j += WAVE) acc = fmaf(x[j], Wp[j], acc);
            acc = wave_sum(acc);
            if (lane == 0) s.f[i] = acc;
        }
        __syncthreads();
        f = me.row ? s.f[tid] : 0.f;
        __syncthreads();
        r = cox_residual(f, me, e, inv, A, s);
        u = fmaf(cost, r, a);
        // the primal gradient X_t^T u
        s.v[tid] = u;
        __syncthreads();
        float gmax = 0.f;
        xt_times(X, s, n, d, [&](int, float acc) { gmax = fmaxf(gmax, fabsf(acc)); });
        res = block_max<CX_WAVES>(gmax, s.red);                   // its barriers also free s.v
        if (it == 0) g0 = res;                      // a = 0: the gradient at w = 0
        // Relative stop.  The internal target is tighter than gtol: Newton's last steps square the residual.  Below gtol g0 the
        // iteration also ends as soon as a step no longer halves the residual (the fp32 floor).
        if (res <= PROBE_TIGHT * gtol * g0 || (res <= gtol * g0 && res >= 0.5f * prev)) break;
        if (it >= max_iter || !(res == res)) break;
        prev = res;

        // ---- CG on the Newton system (I + cost H G) x = -u, inner product x^T G x' ----
        auto g_times = [&](float v) {                // (G v)_tid; G is symmetric: column tid, coalesced
            s.v[tid] = v;
            float out = 0.f;
            __syncthreads();
            if (me.row) {
#pragma unroll 8       // a deeper unroll was tried once and not found faster: DESIGN 3.15 has the run and what it does not show
                for (int j = 0; j < n; ++j) out = fmaf(Gp[(int64_t)j * ldg + tid], s.v[j], out);
            }
            __syncthreads();
            return out;
        };
        float xa = 0.f, Gx = 0.f;
        float ra = -u, Gr = g_times(ra);
        float red[1] = {ra * Gr};
        block_sum<1, CX_WAVES>(red, s.red);
        float rho = red[0];
        const float rho0 = rho;
        float pa = ra, Gpd = Gr;
        for (int k = 0; k < MDL_COX_CG_MAX && rho > 0.f; ++k) {
            const float Hq = cox_hess(me.row ? Gpd : 0.f, me, e, inv, A, s);
            const float Ma = fmaf(cost, Hq, pa);
            red[0] = Gpd * Ma;
            block_sum<1, CX_WAVES>(red, s.red);
            const float pMp = red[0];
            if (!(pMp > 0.f)) break;
            const float alpha = rho / pMp;
            ++cg_total;
            xa = fmaf(alpha, pa, xa);
            Gx = fmaf(alpha, Gpd, Gx);
            ra = fmaf(-alpha, Ma, ra);
            Gr = g_times(ra);
            red[0] = ra * Gr;
            block_sum<1, CX_WAVES>(red, s.red);
            const float rho_new = red[0];
            if (!(rho_new > PROBE_CG_TOL2 * rho0)) break;
            const float beta = rho_new / rho;
            rho = rho_new;
            pa = fmaf(beta, pa, ra);
            Gpd = fmaf(beta, Gpd, Gr);
        }

        // ---- step length along xa: phi'(t) = cost sum r(f + t df) df + xa^T G a + t xa^T G xa; (G a)_i = f_i ----
        const float df = me.row ? Gx : 0.f;
        float lin[2] = {cost * r * df, xa * f};
        block_sum<2, CX_WAVES>(lin, s.red);
        const float dphi0 = lin[0] + lin[1], xGa = lin[1];
        red[0] = xa * Gx;
        block_sum<1, CX_WAVES>(red, s.red);
        const float xGx = red[0];
        if (!(dphi0 < 0.f)) break;                  // no descent left in fp32: stop here, unconverged
        float tl = 1.f;
        for (int ls = 0; ls < MDL_COX_LS_MAX; ++ls) {
            float et, invt, At;
            const float rt = cox_residual(fmaf(tl, df, f), me, et, invt, At, s);
            red[0] = cost * rt * df;
            block_sum<1, CX_WAVES>(red, s.red);
            const float dphi = red[0] + xGa + tl * xGx;
            if (dphi <= -0.5f * dphi0) break;        // a NaN (an overflow along the line) halves too
            tl *= 0.5f;
        }
        a = fmaf(tl, xa, a);
        ++it;
    }

    // the median of the training rows' decision values (numpy's: the mean of the two middle values for even n), by rank counting
    s.v[tid] = f;
    if (tid < 2) s.red[0][tid] = __builtin_nanf("");
    __syncthreads();
    if (me.row) {
        int less = 0, equal = 0;
        for (int j = 0; j < n; ++j) {
            const float fj = s.v[j];
            less += fj < f ? 1 : 0;
            equal += fj == f ? 1 : 0;
        }
        const int lo = (n - 1) / 2, hi = n / 2;       // equal for odd n
        if (less <= lo && lo < less + equal) s.red[0][0] = f;      // every writer of a slot writes the same value
        if (less <= hi && hi < less + equal) s.red[0][1] = f;
    }
    __syncthreads();
    if (tid == 0) {
        thr_out[p] = 0.5f * (s.red[0][0] + s.red[0][1]);
        info[(int64_t)p * 4 + 0] = (float)it;
        info[(int64_t)p * 4 + 1] = res <= gtol * g0 ? 1.f : 0.f;
        info[(int64_t)p * 4 + 2] = res;
        info[(int64_t)p * 4 + 3] = (float)cg_total;
    }
}

// ---- metrics ----------------------------------------------------------------------------------------------------------------------
// workspace: cnt [P] uint64 (comparable pairs << 32 | concordance numerator), risk [3][P][S] int32 (n_i, h_i, d_i of the test event
// cases), tcls [P][S16] int8 (-1: not a test case; else bit 0 = event, bit 1 = high-risk group)
struct SurvWs {
    unsigned long long* cnt;
    int32_t* risk;
    int8_t* tcls;
};
inline SurvWs surv_ws(void* ws, int64_t P, int64_t S) {
    SurvWs m;
    char* base = reinterpret_cast<char*>(ws);
    m.cnt = reinterpret_cast<unsigned long long*>(base);
    m.risk = reinterpret_cast<int32_t*>(base + up16(P * 8));
    m.tcls = reinterpret_cast<int8_t*>(base + up16(P * 8) + up16(3 * P * S * 4));
    return m;
}

__global__ __launch_bounds__(SV_THREADS) void surv_prepare_kernel(const float* __restrict__ z, const int32_t* __restrict__ event, int64_t lde,
                                                                 const int32_t* __restrict__ train_idx,
                                                                 const int32_t* __restrict__ n_train, int n_max, int S,
                                                                 const float* __restrict__ thr, SurvWs m, int64_t S16) {
    const int tid = threadIdx.x, p = blockIdx.x;
    int8_t* tcls = m.tcls + (int64_t)p * S16;
    const int32_t* ep = event + (int64_t)p * lde;
    const float th = thr[p];
    if (tid == 0) m.cnt[p] = 0ull;
    for (int i = tid; i < S; i += SV_THREADS) {
        const int ev = ep[i];
        tcls[i] = (ev == 0 || ev == 1) ? (int8_t)(ev | (z[(int64_t)p * S + i] > th ? 2 : 0)) : (int8_t)-1;
    }
    __syncthreads();
    strike_training<SV_THREADS>(tcls, train_idx, n_train, p, n_max, S);
}

__global__ __launch_bounds__(SV_THREADS) void surv_pairs_kernel(const float* __restrict__ z, const float* __restrict__ time, int64_t ldt,
                                                               int S, int slices, SurvWs m, int64_t S16, int64_t P) {
    __shared__ float s_z[SV_THREADS], s_t[SV_THREADS];
    __shared__ int s_c[SV_THREADS];
    __shared__ int s_cnt[SV_WAVES][2];
    const int tid = threadIdx.x;
    const int slice = blockIdx.x % slices, p = blockIdx.x / slices;
    const int8_t* tcls = m.tcls + (int64_t)p * S16;
    const float* zp = z + (int64_t)p * S;
    const float* tp = time + (int64_t)p * ldt;
    const int i = slice * SV_THREADS + tid;
    const bool mine = i < S && tcls[i] >= 0 && (tcls[i] & 1);      // a test case with an event
    if (!__syncthreads_or(mine ? 1 : 0)) return;
    const float zi = mine ? zp[i] : 0.f, ti = mine ? tp[i] : 0.f;
    int num = 0, comp = 0, n_i = 0, h_i = 0, d_i = 0;
    for (int j0 = 0; j0 < S; j0 += SV_THREADS) {
        const int j = j0 + tid;
        const int cj = j < S ? tcls[j] : -1;
        s_c[tid] = cj;
        s_z[tid] = cj >= 0 ? zp[j] : 0.f;
        s_t[tid] = cj >= 0 ? tp[j] : 0.f;
        __syncthreads();
        if (mine) {
            const int lim = S - j0 < SV_THREADS ? S - j0 : SV_THREADS;
            for (int jj = 0; jj < lim; ++jj) {
                const int cls = s_c[jj];
                if (cls < 0) continue;
                const float tj = s_t[jj], zj = s_z[jj];
                if (tj >= ti) {
                    ++n_i;
                    h_i += cls >> 1;
                }
                if (tj == ti && (cls & 1)) ++d_i;
                if (ti < tj || (ti == tj && !(cls & 1))) {
                    ++comp;
                    num += zi > zj ? 2 : (zi == zj ? 1 : 0);
                }
            }
        }
        __syncthreads();
    }
    if (mine) {
        m.risk[((int64_t)0 * P + p) * S + i] = n_i;
        m.risk[((int64_t)1 * P + p) * S + i] = h_i;
        m.risk[((int64_t)2 * P + p) * S + i] = d_i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {               // at most 2 * 256 * 16384 per workgroup: fits an int
        num += __shfl_xor(num, o, 64);
        comp += __shfl_xor(comp, o, 64);
    }
    if ((tid & (WAVE - 1)) == 0) {
        s_cnt[tid / WAVE][0] = num;
        s_cnt[tid / WAVE][1] = comp;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long tn = (unsigned long long)((s_cnt[0][0] + s_cnt[1][0]) + (s_cnt[2][0] + s_cnt[3][0]));
        const unsigned long long tc = (unsigned long long)((s_cnt[0][1] + s_cnt[1][1]) + (s_cnt[2][1] + s_cnt[3][1]));
        if (tc) atomicAdd(&m.cnt[p], (tc << 32) + tn);      // both totals stay below 2^31 (S <= 16384): the halves never carry
    }
}

__global__ __launch_bounds__(SV_THREADS) void surv_finish_kernel(int S, const float* __restrict__ thr, SurvWs m, int64_t S16, int64_t P,
                                                                double* __restrict__ c_index, double* __restrict__ chi2,
                                                                int32_t* __restrict__ counts) {
    __shared__ double s_d[SV_THREADS][2];
    __shared__ int s_i[SV_THREADS][4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int8_t* tcls = m.tcls + (int64_t)p * S16;
    double oe = 0.0, var = 0.0;
    int n_test = 0, n_high = 0, ev_low = 0, ev_high = 0;
    for (int i = tid; i < S; i += SV_THREADS) {      // a thread's cases in case order
        const int cls = tcls[i];
        if (cls < 0) continue;
        const int high = cls >> 1;
        ++n_test;
        n_high += high;
        if (!(cls & 1)) continue;
        ev_high += high;
        ev_low += 1 - high;
        const double n_i = (double)m.risk[((int64_t)0 * P + p) * S + i], h_i = (double)m.risk[((int64_t)1 * P + p) * S + i];
        const double d_i = (double)m.risk[((int64_t)2 * P + p) * S + i];
        const double share = h_i / n_i;              // n_i >= 1: the case itself
        oe += (double)high - share;
        if (n_i > 1.0) var += share * (1.0 - share) * (n_i - d_i) / (n_i - 1.0);
    }
    s_d[tid][0] = oe;
    s_d[tid][1] = var;
    s_i[tid][0] = n_test;
    s_i[tid][1] = n_high;
    s_i[tid][2] = ev_low;
    s_i[tid][3] = ev_high;
    __syncthreads();
    for (int span = SV_THREADS / 2; span > 0; span >>= 1) {      // a fixed tree
        if (tid < span) {
            s_d[tid][0] += s_d[tid + span][0];
            s_d[tid][1] += s_d[tid + span][1];
#pragma unroll
            for (int k = 0; k < 4; ++k) s_i[tid][k] += s_i[tid + span][k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned long long cnt = m.cnt[p];
        const int num = (int)(cnt & 0xFFFFFFFFull), comp = (int)(cnt >> 32);
        const double nan = __builtin_nan("");
        const bool refused = thr[p] != thr[p];       // a refused fit: its scores are NaN too
        c_index[p] = (comp > 0 && !refused) ? (double)num / (2.0 * (double)comp) : nan;
        chi2[p] = (s_d[0][1] > 0.0 && !refused) ? s_d[0][0] * s_d[0][0] / s_d[0][1] : nan;
        int32_t* out = counts + (int64_t)p * 6;
        out[0] = num;
        out[1] = comp;
        out[2] = s_i[0][0];
        out[3] = s_i[0][1];
        out[4] = s_i[0][2];
        out[5] = s_i[0][3];
    }
}

// the limits of the entry points: {n_max, d, S, fit, classes}
constexpr ProbeLimits COX_FIT = {CX_NMAX, PROBE_NO_LIMIT, PROBE_NO_LIMIT, true, false};
constexpr ProbeLimits SURV_METRICS = {CX_NMAX, PROBE_NO_LIMIT, MDL_PROBE_MAX_CASES, false, false};

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_cox_order_fit_ws_bytes(int64_t P, int n_max, int d) {
    if (const int rc = probe_check(probe_sizes(P, n_max, 1, 0, d), COX_FIT, nullptr)) return rc;
    const int64_t ldg = gram_ld(n_max);
    return up16(P * 4) + up16(P * n_max * 4) + P * ldg * ldg * (int64_t)sizeof(float);
}

extern "C" int mdl_cox_fit(const float* X, int64_t ldX, int64_t S, int d, const float* time, int64_t ldt, const int32_t* event, int64_t lde,
                           const int32_t* train_idx, const int32_t* n_train, int64_t P, int n_max, float cost, float gtol, int max_iter,
                           float* W_out, float* thr_out, float* info_out, void* ws, void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{time, ldt}, {event, lde}}, 2, 0, d};
    const int64_t ldg = gram_ld(n_max), tps = ldg / GRAM_TILE;
    const ProbeExtra extra = {all_given(X, W_out, thr_out, info_out, ws), mul_i32(P, tps, tps) && mul_i32(P, d), host_aligned16(ws), 0,
                              ldX, max_iter, cost, gtol};
    if (const int rc = probe_check(t, COX_FIT, &extra)) return rc;
    const CoxWs c = cox_ws(ws, P, n_max);
    hipLaunchKernelGGL(cox_order_kernel, dim3((unsigned)P), dim3(CX_THREADS), 0, (hipStream_t)stream, time, ldt, event, lde, (int)S,
                       train_idx, n_train, n_max, c);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(cox_gram_kernel, dim3((unsigned)(P * tps * tps)), dim3(CX_GRAM_THREADS), 0, (hipStream_t)stream, X, ldX, d, n_train,
                       n_max, (int)ldg, c);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(cox_fit_kernel, dim3((unsigned)P), dim3(CX_THREADS), 0, (hipStream_t)stream, X, ldX, d, time, ldt, event, lde,
                       n_train, n_max, cost, gtol, max_iter, W_out, thr_out, info_out, c, (int)ldg);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int64_t mdl_surv_metrics_ws_bytes(int64_t P, int64_t S) {
    if (const int rc = probe_check(probe_sizes(P, 1, S, 0, 0), SURV_METRICS, nullptr)) return rc;
    return up16(P * 8) + up16(3 * P * S * 4) + P * s16_of(S);
}

extern "C" int mdl_surv_metrics(const float* z, const float* time, int64_t ldt, const int32_t* event, int64_t lde, const int32_t* train_idx,
                                const int32_t* n_train, int64_t P, int n_max, int64_t S, const float* thr, void* c_index_out,
                                void* chi2_out, int32_t* counts_out, void* ws, void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{time, ldt}, {event, lde}}, 2, 0, 0};
    const int64_t slices = ceil_div(S, SV_THREADS);
    const ProbeExtra extra = {all_given(z, thr, c_index_out, chi2_out, counts_out, ws), mul_i32(P, slices),
                              host_aligned16(ws) && all_aligned(8, c_index_out, chi2_out)};
    if (const int rc = probe_check(t, SURV_METRICS, &extra)) return rc;
    const SurvWs m = surv_ws(ws, P, S);
    const int64_t S16 = s16_of(S);
    hipLaunchKernelGGL(surv_prepare_kernel, dim3((unsigned)P), dim3(SV_THREADS), 0, (hipStream_t)stream, z, event, lde, train_idx, n_train,
                       n_max, (int)S, thr, m, S16);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(surv_pairs_kernel, dim3((unsigned)(P * slices)), dim3(SV_THREADS), 0, (hipStream_t)stream, z, time, ldt, (int)S,
                       (int)slices, m, S16, P);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(surv_finish_kernel, dim3((unsigned)P), dim3(SV_THREADS), 0, (hipStream_t)stream, (int)S, thr, m, S16, P,
                       reinterpret_cast<double*>(c_index_out), reinterpret_cast<double*>(chi2_out), counts_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
