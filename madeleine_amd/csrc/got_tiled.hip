// got_tiled.hip -- the TILED size class of GOT (1 <= n, m <= 4096 tokens, 1 <= d <= 4096): the same forward and reverse sweep as
// got_resident.hip (see its header for the algebra: IPOT, Gromov-Wasserstein, the one-matrix-per-iteration reverse with Y_t = gQ_t . Q_t),
// organised for shapes where one case holds more work than a workgroup -- or two -- can do.
//
// The two token sets may differ in size: V is [k, n, d], Q is [k, m, d] (mdl_got_tiled_rect_*; the square entry points pass m = n).
// The algebra with the sizes kept apart: C = 1 - V^ Q^T and every plan are n x m, Cs n x n, Ct m x m; IPOT has sigma_0 = 1/m,
// delta_i = 1 / (n sum_j Q_ij sigma_j), sigma_j = 1 / (m sum_i Q_ij delta_i), so the reverse carries -n delta^2 on the row side and
// -m sigma^2 on the column side; GW has gamma_0 = 1/(n m), rs = Cs^2 1/n, rt = Ct^2 1/m, C_gamma = rs 1^T + 1 rt^T - 2 Cs gamma Ct^T.
//
// Organisation: many workgroups share one case and meet only at kernel boundaries.
//   * SWEEPS (IPOT forward / reverse): a 256-thread workgroup owns a panel of RP = 16 rows of one case and branch (grid = panels x
//     cases x branches; the panels run over the n rows, whatever m is).  A row's reductions are wave-local (each wave owns 4 rows);
//     the column sums an iteration needs are written as per-panel partials [panel][m] and merged, in panel order, by the next launch.
//     Two launches per IPOT iteration: a row pass (reads A and the previous plan, writes the next plan into the tape, row scaling
//     delta, column partials) and a merge (column scaling sigma).  The forward fuses "write T_{t-1}" into the row pass of iteration t, so a pass reads A and T_{t-2} once
//     (re-read from L2 by the second phase of the pass, which needs the row sums of the first) and writes T_{t-1} once.
//     The reverse keeps the accumulator H = sum_t t W_t (+ iters Y_{iters+1}) in the workspace (read-modify-write per iteration) instead
//     of registers, and the per-row sums of Y in a workspace vector owned by the row's workgroup.
//   * PRODUCTS (the costs, C_gamma, their adjoints, the cost backward): 128 x 128 output tiles per 256-thread workgroup on
//     v_mfma_f32_32x32x2_f32 (each wave a 64 x 64 block of 2 x 2 accumulators), K-chunks of 16 staged through LDS with a register
//     prefetch of the next chunk; up to three independent products (jobs) per launch, up to three accumulated terms per product.
//   * No workgroup waits for another one of the same launch, no atomics: every cross-workgroup sum (column sums, extrema, tie counts,
//     threshold gradients, per-case distances) is written as partials and merged in a fixed order by a later launch -- two calls give
//     the same bits.
//   * Offsets are 64-bit: one case's tape at n = 4096 is ~2.5e9 floats.
// The WD and GW branches share the sweep launches where their iterations overlap (the Wasserstein IPOT runs beside the first GW IPOT
// in the forward, and its reverse beside the last GW reverse).  Cs and Ct are used with the reference's transposes applied literally.
#include "got_host.hpp"

namespace mdl {
namespace got_tiled {

constexpr int TMAXN = 4096;
constexpr int TMAXD = 4096;
constexpr int WD_ITERS = 30;
constexpr int GW_OUTER = 5;
constexpr int GW_INNER = 20;
constexpr float WD_INV_BETA = 2.0f;    // beta .5  (loss.py:179)
constexpr float GW_INV_BETA = 10.0f;   // lamda .1 (loss.py:269)
constexpr float THR_BETA = 0.1f;       // loss.py:288, :226

constexpr int NT = 256;        // threads of every kernel of this class (4 waves)
constexpr int RP = 16;         // rows of a sweep panel (4 per wave)
constexpr int CW = 256;        // columns of a sweep chunk (4 per lane)
constexpr int MT = 128;        // output tile edge of the products
constexpr int MK = 16;         // K-chunk of the products
constexpr int LDX = MT + 4;    // LDS row of a staged K-chunk ([k][128 + 4]: the row-major stores hit 64 distinct banks)

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }
__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------------------------------------
// workspace: k per-case regions, then the global partials.  V has n tokens, Q has m; a matrix with c columns has row stride up4(c)
// (16-byte rows).  Three matrix shapes: cross (n x m: C, the plans, the tapes), source (n x n: Cs) and target (m x m: Ct); vectors of
// length n (row quantities: delta, rs, Rv) and of length m (column quantities: sigma, rt, Cv, ga).  With m = n all of them coincide.
// ---------------------------------------------------------------------------------------------------------
struct Lay {
    int64_t ldn, ldm;            // row strides of matrices with n / m columns
    int64_t nm, nn, mm;          // elements of a cross / source / target matrix
    int64_t nvn, nvm;            // elements of a length-n / length-m vector
    int64_t P, PX;               // row panels over n (sweeps); over max(n, m) (kernels that walk all three cost matrices)
    int64_t tm;                  // product tile columns over m
    int64_t tiles[3], ext[3];    // product tiles per case of C0, Cs0, Ct0; global offsets of their extrema partials
    int64_t oVh, oQh, orV, orQ, oC0, oCs0, oCt0, oC, oCs, oCt, ors, ort, oAw, oAg, oWT, oWd, oWs, oCg, oGT, oGd, oGs, oP1, oP2, oP3,
        oG, ogT, ogCs, ogCt, ogC0, ogVh, ogQh, ogrs, ogrt, oRv, oCv, oga, ocp, ocpr;
    int64_t per_case;
    int64_t g_cnt, g_wd, g_gwd, g_gthr, g_thr, g_end;
};

__host__ __device__ inline Lay layout(int k, int n, int m, int d) {
    Lay L;
    L.ldn = up4(n);
    L.ldm = up4(m);
    L.nm = (int64_t)n * L.ldm;
    L.nn = (int64_t)n * L.ldn;
    L.mm = (int64_t)m * L.ldm;
    L.nvn = up4(n);
    L.nvm = up4(m);
    L.P = cdiv(n, RP);
    L.PX = cdiv(n > m ? n : m, RP);
    L.tm = cdiv(m, MT);
    const int64_t tn = cdiv(n, MT);
    L.tiles[0] = tn * L.tm;
    L.tiles[1] = tn * tn;
    L.tiles[2] = L.tm * L.tm;
    const int64_t nm = L.nm, nn = L.nn, mm = L.mm, nvn = L.nvn, nvm = L.nvm, cp = 2 * L.P * L.ldm;
    const int64_t ndn = up4((int64_t)n * d), ndm = up4((int64_t)m * d);
    int64_t o = 0;
    L.oVh = o; o += ndn;
    L.oQh = o; o += ndm;
    L.orV = o; o += nvn;
    L.orQ = o; o += nvm;
    L.oC0 = o; o += nm;                          // raw costs (masks and extremum routing of the backward)
    L.oCs0 = o; o += nn;
    L.oCt0 = o; o += mm;
    L.oC = o; o += nm;                           // thresholded costs
    L.oCs = o; o += nn;
    L.oCt = o; o += mm;
    L.ors = o; o += nvn;                         // Cst vectors
    L.ort = o; o += nvm;
    L.oAw = o; o += nm;                          // exp(-C / beta) of the Wasserstein IPOT
    L.oAg = o; o += nm;                          // ... of the GW IPOT in flight
    L.oWT = o; o += nm * WD_ITERS;               // tape: T_1..T_30
    L.oWd = o; o += nvn * WD_ITERS;              // delta_1..30
    L.oWs = o; o += nvm * (WD_ITERS + 1);        // sigma_0..30
    L.oCg = o; o += nm * GW_OUTER;               // C_gamma of every outer iteration
    L.oGT = o; o += nm * GW_OUTER * GW_INNER;
    L.oGd = o; o += nvn * GW_OUTER * GW_INNER;
    L.oGs = o; o += nvm * GW_OUTER * (GW_INNER + 1);
    L.oP1 = o; o += nm;                          // product intermediates (n x m); routed cost gradients in the backward finish:
    L.oP2 = o; o += nm > nn ? nm : nn;           //   P1 = d/dC0 (n x m), P2 = d/dCs0 (n x n), P3 = d/dCt0 (m x m)
    L.oP3 = o; o += mm;
    L.oG = o; o += nm;                           // d/dC_gamma (the GW reverse's H accumulator)
    L.ogT = o; o += nm;                          // d/dgamma
    L.ogCs = o; o += nn;
    L.ogCt = o; o += mm;
    L.ogC0 = o; o += nm;                         // d/dC (the WD reverse's H accumulator), then d/dC0
    L.ogVh = o; o += ndn;
    L.ogQh = o; o += ndm;
    L.ogrs = o; o += nvn;
    L.ogrt = o; o += nvm;
    L.oRv = o; o += 2 * nvn;                     // per branch: row sums of Y (reverse), column sums of Y, ga
    L.oCv = o; o += 2 * nvm;
    L.oga = o; o += 2 * nvm;
    L.ocp = o; o += 2 * cp;                      // per branch: two sets of per-panel column partials [P][ldm]
    L.ocpr = o; o += L.P * L.ldm;                // column partials of the GW products' Cst gradient
    L.per_case = o;
    int64_t g = (int64_t)k * L.per_case;
    for (int q = 0; q < 3; ++q) {                // per (kind, case, tile): (min, max)
        L.ext[q] = g;
        g += (int64_t)k * L.tiles[q] * 2;
    }
    g = up4(g);
    L.g_cnt = g; g += up4((int64_t)k * L.PX * 6);          // per (case, panel): tie counts of the six extrema
    L.g_wd = g; g += up4((int64_t)k * L.P);                // per (case, panel): Wasserstein distance partial
    L.g_gwd = g; g += up4((int64_t)k * L.tiles[0]);        // per (case, tile): GW distance partial
    L.g_gthr = g; g += up4((int64_t)k * L.PX * 3);         // per (case, panel): threshold-gradient partials
    L.g_thr = g; g += 32;   // [0..5] extrema used, [6..8] thresholds, [9..14] tie counts, [15..17] threshold gradients
    L.g_end = g;
    return L;
}

// ---------------------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 msk4(f32x4 v, int j, int n) {   // zero the columns >= n of a 4-column group
    f32x4 r;
    r.x = j < n ? v.x : 0.f;
    r.y = j + 1 < n ? v.y : 0.f;
    r.z = j + 2 < n ? v.z : 0.f;
    r.w = j + 3 < n ? v.w : 0.f;
    return r;
}
__device__ __forceinline__ float hsum4(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ f32x4 splat4(float s) {
    f32x4 r;
    r.x = r.y = r.z = r.w = s;
    return r;
}
// fixed-order sum over the workgroup: lane sums in order, a butterfly in the wave, the four waves in order
__device__ __forceinline__ float block_sum4(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// fixed-order sum of cnt floats with stride 1 (one workgroup): thread t adds elements t, t + NT, ... in order
__device__ __forceinline__ float block_sum_array(const float* src, int64_t cnt, int64_t stride, float* red) {
    float s = 0.f;
    for (int64_t e = threadIdx.x; e < cnt; e += NT) s += src[e * stride];
    return block_sum4(s, red);
}

// Walk of the RP x ld elements of a row panel by the workgroup, element e = r ld + j taken by thread e % NT in increasing e (the
// order the per-thread partial sums of tl_bwd_final_kernel are defined by), without a division per element.
struct PanelWalk {
    int e, r, j, ld;
    __device__ __forceinline__ PanelWalk(int64_t ld_) : e((int)threadIdx.x), ld((int)ld_) {
        r = e / ld;
        j = e - r * ld;
    }
    __device__ __forceinline__ bool in() const { return r < RP; }
    __device__ __forceinline__ void next() {
        e += NT;
        j += NT;
        while (j >= ld) {
            j -= ld;
            ++r;
        }
    }
};

// ---------------------------------------------------------------------------------------------------------
// K1: normalised tokens and their norms (one wave per token row)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void tl_norm_kernel(const float* __restrict__ V, const float* __restrict__ Q, float* ws, const Lay L,
                                                     int n, int m, int d) {
    const int64_t R = cdiv(n > m ? n : m, 4);
    const int64_t b = blockIdx.x / R;
    const int i = (int)(blockIdx.x % R) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    float* base = ws + b * L.per_case;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const int rows = s ? m : n;
        if (i >= rows) continue;   // wave-uniform; no barrier in this kernel
        const float* src = (s ? Q : V) + (b * rows + i) * (int64_t)d;
        float ss = 0.f;
        for (int e = lane; e < d; e += 64) ss += src[e] * src[e];
        ss = wave_sum(ss);
        const float nr = sqrtf(ss), sc = 1.f / (nr + 1e-12f);
        float* dst = base + (s ? L.oQh : L.oVh) + (int64_t)i * d;
        for (int e = lane; e < d; e += 64) dst[e] = src[e] * sc;
        if (lane == 0) base[(s ? L.orQ : L.orV) + i] = nr;
    }
}

// ---------------------------------------------------------------------------------------------------------
// K2: products on the matrix cores.  C[M x N] (per case) = epilogue(sum over terms of op(A_t) op(B_t)), op = transpose or not.
// A term operand with offset < 0 is the constant matrix (ca / cb): the uniform plan gamma_0 = 1/(n m) of the first GW iteration.
// The jobs of a launch may differ in shape (C0 is n x m, Cs0 n x n, Ct0 m x m): the grid covers the job with the most tiles and the
// workgroups beyond a job's own tiles leave at once.
// ---------------------------------------------------------------------------------------------------------
enum { GM_RAW = 0, GM_STORE = 1, GM_ACC = 2, GM_CG = 3, GM_GWD = 4 };
struct GTerm {
    int64_t oA, oB, lda, ldb;   // per-case offsets (< 0: constant operand); A(i,k) = ta ? A[k lda + i] : A[i lda + k]; B likewise
    float ca, cb;
    int ta, tb, K;
};
struct GJob {
    GTerm t[3];
    int nt, mode;
    int M, N, tn, tiles;        // output shape, tile columns, tiles per case
    float alpha;
    int64_t oC, ldc;            // output (per case)
    int64_t oX, oY, oZ;         // GM_CG / GM_GWD: rs, rt (vectors), gamma (GM_GWD)
    int64_t gpart;              // GM_RAW / GM_GWD: global offset of the per-(case, tile) partials
};
constexpr int GMAXJ = 3;
struct GArgs {
    float* ws;
    int64_t per_case;
    int k;
    GJob j[GMAXJ];
};

__global__ __launch_bounds__(NT) void tl_gemm_kernel(const GArgs g) {
    __shared__ float xs[MK * LDX];
    __shared__ float ys[MK * LDX];
    __shared__ float red[8];
    const GJob& J = g.j[blockIdx.y];
    const int64_t b = blockIdx.x / J.tiles;
    if (b >= g.k) return;   // workgroup-uniform, before any barrier
    const int tile = (int)(blockIdx.x % J.tiles);
    const int i0 = (tile / J.tn) * MT, j0 = (tile % J.tn) * MT;
    float* base = g.ws + b * g.per_case;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int bi0 = (wave >> 1) * 64, bj0 = (wave & 1) * 64;
    const int M = J.M, N = J.N;
    f32x16 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;
    constexpr int NP = MT * MK / NT;   // 8 elements per thread and operand per chunk
    float px[NP], py[NP];
#pragma unroll 1
    for (int term = 0; term < J.nt; ++term) {
        const GTerm T = J.t[term];
        const float* __restrict__ A = T.oA >= 0 ? base + T.oA : nullptr;
        const float* __restrict__ Bm = T.oB >= 0 ? base + T.oB : nullptr;
        const bool ta = T.ta, tb = T.tb;
        const int K = T.K;
        auto gload = [&](int k0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int idx = tid + NT * p;
                {
                    const int ii = ta ? (idx & 127) : (idx >> 4), kk = ta ? (idx >> 7) : (idx & 15);
                    const int i = i0 + ii, kx = k0 + kk;
                    const bool ok = i < M && kx < K;
                    px[p] = !ok ? 0.f : (A ? (ta ? A[(int64_t)kx * T.lda + i] : A[(int64_t)i * T.lda + kx]) : T.ca);
                }
                {
                    const int jj = tb ? (idx >> 4) : (idx & 127), kk = tb ? (idx & 15) : (idx >> 7);
                    const int j = j0 + jj, kx = k0 + kk;
                    const bool ok = j < N && kx < K;
                    py[p] = !ok ? 0.f : (Bm ? (tb ? Bm[(int64_t)j * T.ldb + kx] : Bm[(int64_t)kx * T.ldb + j]) : T.cb);
                }
            }
        };
        gload(0);
#pragma unroll 1
        for (int k0 = 0; k0 < K; k0 += MK) {
            __syncthreads();   // every wave is done with the previous chunk
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int idx = tid + NT * p;
                const int ii = ta ? (idx & 127) : (idx >> 4), ka = ta ? (idx >> 7) : (idx & 15);
                const int jj = tb ? (idx >> 4) : (idx & 127), kb = tb ? (idx & 15) : (idx >> 7);
                xs[ka * LDX + ii] = px[p];
                ys[kb * LDX + jj] = py[p];
            }
            __syncthreads();
            if (k0 + MK < K) gload(k0 + MK);   // next chunk in flight under this chunk's MFMAs
#pragma unroll
            for (int kk = 0; kk < MK; kk += 2) {
                const int kq = (kk + hi) * LDX;
                const float a0 = xs[kq + bi0 + l31], a1 = xs[kq + bi0 + 32 + l31];
                const float b0 = ys[kq + bj0 + l31], b1 = ys[kq + bj0 + 32 + l31];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    // epilogue: lane (l31, hi) of accumulator (u, v) holds rows (r & 3) + 8 (r >> 2) + 4 hi, column l31
    const int mode = J.mode;
    float* __restrict__ C = base + J.oC;
    const float* __restrict__ X = base + J.oX;
    const float* __restrict__ Y = base + J.oY;
    const float* __restrict__ Z = base + J.oZ;
    const int64_t ldc = J.ldc;
    const float alpha = J.alpha;
    float mn = INFINITY, mx = -INFINITY, sacc = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int j = j0 + bj0 + 32 * v + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + bi0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (i < M && j < N) {
                    const float a = acc[u][v][r];
                    const int64_t e = (int64_t)i * ldc + j;
                    if (mode == GM_RAW) {
                        const float x = 1.f - a;
                        C[e] = x;
                        mn = fminf(mn, x);
                        mx = fmaxf(mx, x);
                    } else if (mode == GM_STORE) {
                        C[e] = alpha * a;
                    } else if (mode == GM_ACC) {
                        C[e] += alpha * a;
                    } else if (mode == GM_CG) {
                        C[e] = (X[i] + Y[j]) - 2.f * a;
                    } else {
                        sacc += ((X[i] + Y[j]) - 2.f * a) * Z[e];
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    if (mode == GM_RAW) {
        mn = -wave_max(-mn);
        mx = wave_max(mx);
        __syncthreads();
        if (lane == 0) {
            red[wave] = mn;
            red[4 + wave] = mx;
        }
        __syncthreads();
        if (tid == 0) {
            float* o = g.ws + J.gpart + (b * J.tiles + tile) * 2;
            o[0] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
            o[1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        }
    } else if (mode == GM_GWD) {
        const float s = block_sum4(sacc, red);
        if (tid == 0) g.ws[J.gpart + b * J.tiles + tile] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// K3: extrema of the three raw cost tensors over the whole batch -> minmax_out; thresholds (minmax_in if given)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void tl_minmax_kernel(float* ws, const Lay L, int k, float* minmax_out, const float* minmax_in) {
    __shared__ float red[8];
    __shared__ float ext[6];
    const int tid = threadIdx.x;
    for (int m = 0; m < 3; ++m) {
        const int64_t cnt = (int64_t)k * L.tiles[m];
        const float* src = ws + L.ext[m];
        float a = INFINITY, z = -INFINITY;
        for (int64_t e = tid; e < cnt; e += NT) {
            a = fminf(a, src[2 * e]);
            z = fmaxf(z, src[2 * e + 1]);
        }
        a = -wave_max(-a);
        z = wave_max(z);
        __syncthreads();
        if ((tid & 63) == 0) {
            red[tid >> 6] = a;
            red[4 + (tid >> 6)] = z;
        }
        __syncthreads();
        if (tid == 0) {
            ext[2 * m] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
            ext[2 * m + 1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        }
    }
    __syncthreads();
    if (tid < 6) {
        if (minmax_out) minmax_out[tid] = ext[tid];
        ws[L.g_thr + tid] = minmax_in ? minmax_in[tid] : ext[tid];
    }
    if (tid < 3) {
        const float lo = minmax_in ? minmax_in[2 * tid] : ext[2 * tid], hi = minmax_in ? minmax_in[2 * tid + 1] : ext[2 * tid + 1];
        ws[L.g_thr + 6 + tid] = lo + THR_BETA * (hi - lo);
    }
}

// ---------------------------------------------------------------------------------------------------------
// K4: thresholded costs, tie counts of the six extrema, Cst vectors rs, rt (per panel)
// ---------------------------------------------------------------------------------------------------------
// one row of one cost matrix (this wave): dst = relu(src - thr), ties with the two extrema, sum of squares of the result
__device__ __forceinline__ float thr_row(const float* __restrict__ src, float* __restrict__ dst, int cols, float thr, float lo, float hi,
                                         float& clo, float& chi) {
    const int lane = threadIdx.x & 63;
    float sq = 0.f;
    for (int j = 4 * lane; j < cols; j += CW) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src + j);
        f32x4 c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool ok = j + q < cols;
            c[q] = ok ? fmaxf(x[q] - thr, 0.f) : 0.f;
            clo += ok && x[q] == lo;
            chi += ok && x[q] == hi;
            sq = __builtin_fmaf(c[q], c[q], sq);   // fused on purpose: the rounding of rs, rt must not depend on how the loop is compiled
        }
        *reinterpret_cast<f32x4*>(dst + j) = c;
    }
    return wave_sum(sq);
}

// grid: cases x panels over max(n, m) rows (C0 and Cs0 have n rows, Ct0 has m)
__global__ __launch_bounds__(NT) void tl_thr_kernel(float* ws, const Lay L, int n, int m) {
    __shared__ float red[4];
    const int64_t b = blockIdx.x / L.PX, panel = blockIdx.x % L.PX;
    float* base = ws + b * L.per_case;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ex[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) ex[q] = ws[L.g_thr + q];
    const float t0 = ws[L.g_thr + 6], t1 = ws[L.g_thr + 7], t2 = ws[L.g_thr + 8];
    float cnt[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int r = 0; r < RP / 4; ++r) {
        const int64_t i = panel * RP + wave + 4 * r;   // wave-uniform; no barrier until the loop ends
        if (i < n) {
            thr_row(base + L.oC0 + i * L.ldm, base + L.oC + i * L.ldm, m, t0, ex[0], ex[1], cnt[0], cnt[1]);
            const float as = thr_row(base + L.oCs0 + i * L.ldn, base + L.oCs + i * L.ldn, n, t1, ex[2], ex[3], cnt[2], cnt[3]);
            if (lane == 0) base[L.ors + i] = as / (float)n;   // rs_i = (1/n) sum_k Cs_ik^2  (loss.py:240)
        }
        if (i < m) {
            const float at = thr_row(base + L.oCt0 + i * L.ldm, base + L.oCt + i * L.ldm, m, t2, ex[4], ex[5], cnt[4], cnt[5]);
            if (lane == 0) base[L.ort + i] = at / (float)m;   // rt_j = (1/m) sum_l Ct_jl^2  (loss.py:241)
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const float s = block_sum4(cnt[q], red);
        if (threadIdx.x == 0) ws[L.g_cnt + (b * L.PX + panel) * 6 + q] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// IPOT sweeps.  A job = one branch of every case of the launch (grid.x = cases x panels, grid.y = job).
// ---------------------------------------------------------------------------------------------------------
struct SJob {
    int64_t oCm, oA, oT, od, os, ocp, oH, ogTin, oRv, oCv, oga;   // per-case offsets
    int64_t gpart;              // forward, last pass: global offset of the per-(case, panel) distance partials (< 0: none)
    const float* gscale;        // reverse seed: device scalar multiplying gT_in (nullptr: 1)
    int p, iters;               // forward: pass 1 .. iters + 1; reverse: iteration iters .. 1, iters + 1 = the seed
    float inv_beta;
};
struct SArgs {
    float* ws;
    int64_t per_case, ld, nm, nvn, nvm, P;   // ld = up4(m): the sweeps walk n x m matrices; rows and delta over n, columns and sigma over m
    int n, m;
    SJob j[2];
};

// Forward row pass p: T_{p-1} = delta_{p-1} (A . T_{p-2}) sigma_{p-1} is written to the tape (p >= 2; T_0 = 1); for p <= iters the pass
// continues with Q_p = A . T_{p-1}: delta_p,i = 1 / (n sum_j Q_p,ij sigma_{p-1,j}) (sigma_0 = 1/m) and the column partials sum_{i in panel} Q_p,ij delta_p,i.
// p == 1 forms A = exp(-C / beta) from the cost and stores it.  p == iters + 1 only writes T_iters (and the distance partial sum C . T).
__global__ __launch_bounds__(NT) void tl_fwd_row_kernel(const SArgs a) {
    __shared__ float red[4][CW];
    const SJob& J = a.j[blockIdx.y];
    const int64_t b = blockIdx.x / a.P, panel = blockIdx.x % a.P;
    const int n = a.n, m = a.m, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ld = a.ld, nm = a.nm, nvn = a.nvn, nvm = a.nvm;
    float* base = a.ws + b * a.per_case;
    const int p = J.p, iters = J.iters;
    const float fn = (float)n, inv_m = 1.f / (float)m, ib = J.inv_beta;
    float* __restrict__ A = base + J.oA;
    const float* __restrict__ Cm = base + J.oCm;
    const float* __restrict__ Tpp = base + J.oT + (int64_t)(p >= 3 ? p - 3 : 0) * nm;      // T_{p-2}
    float* __restrict__ Tw = base + J.oT + (int64_t)(p >= 2 ? p - 2 : 0) * nm;             // T_{p-1}
    const float* __restrict__ dprev = base + J.od + (int64_t)(p >= 2 ? p - 2 : 0) * nvn;   // delta_{p-1}
    const float* __restrict__ sprev = base + J.os + (int64_t)(p - 1) * nvm;                // sigma_{p-1}
    const bool rowpass = p <= iters;
    const bool dist = p == iters + 1 && J.gpart >= 0;
    // A and T_{p-1} at row i, columns j .. j + 3 (columns >= m read as 0)
    auto elem = [&](int64_t i, int j, float di, f32x4& Av, f32x4& Tv) {
        const int64_t e = i * ld + j;
        if (p == 1) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(Cm + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) Av[q] = expf(-c[q] * ib);
            Av = msk4(Av, j, m);
            Tv = msk4(splat4(1.f), j, m);
        } else {
            Av = msk4(*reinterpret_cast<const f32x4*>(A + e), j, m);
            const f32x4 tp = p >= 3 ? msk4(*reinterpret_cast<const f32x4*>(Tpp + e), j, m) : splat4(1.f);
            const f32x4 sq = msk4(*reinterpret_cast<const f32x4*>(sprev + j), j, m);
#pragma unroll
            for (int q = 0; q < 4; ++q) Tv[q] = di * (Av[q] * tp[q]) * sq[q];
        }
    };
    float dp[RP / 4], dl[RP / 4];
#pragma unroll
    for (int r = 0; r < RP / 4; ++r) {
        const int64_t i = panel * RP + wave + 4 * r;
        dp[r] = (p >= 2 && i < n) ? dprev[i] : 0.f;
        dl[r] = 0.f;
    }
    if (rowpass) {   // phase 1: row sums -> delta_p
#pragma unroll
        for (int r = 0; r < RP / 4; ++r) {
            const int64_t i = panel * RP + wave + 4 * r;
            if (i < n) {   // wave-uniform
                float s = 0.f;
                for (int j = 4 * lane; j < m; j += CW) {
                    f32x4 Av, Tv;
                    elem(i, j, dp[r], Av, Tv);
                    const f32x4 sq = p == 1 ? msk4(splat4(inv_m), j, m) : msk4(*reinterpret_cast<const f32x4*>(sprev + j), j, m);
#pragma unroll
                    for (int q = 0; q < 4; ++q) s += (Av[q] * Tv[q]) * sq[q];
                }
                s = wave_sum(s);
                dl[r] = 1.f / (fn * s);
                if (lane == 0) base[J.od + (int64_t)(p - 1) * nvn + i] = dl[r];
            }
        }
    }
    // phase 2: write A (p == 1) / T_{p-1} (p >= 2); column partials of Q_p delta_p
    float dsum = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < m; c0 += CW) {
        const int j = c0 + 4 * lane;
        f32x4 cacc = splat4(0.f);
        if (j < m) {
#pragma unroll
            for (int r = 0; r < RP / 4; ++r) {
                const int64_t i = panel * RP + wave + 4 * r;
                if (i < n) {
                    f32x4 Av, Tv;
                    elem(i, j, dp[r], Av, Tv);
                    const int64_t e = i * ld + j;
                    if (p == 1) *reinterpret_cast<f32x4*>(A + e) = Av;
                    else *reinterpret_cast<f32x4*>(Tw + e) = Tv;
                    if (rowpass) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) cacc[q] += (Av[q] * Tv[q]) * dl[r];
                    }
                    if (dist) {
                        const f32x4 c = msk4(*reinterpret_cast<const f32x4*>(Cm + e), j, m);
#pragma unroll
                        for (int q = 0; q < 4; ++q) dsum += c[q] * Tv[q];
                    }
                }
            }
        }
        if (rowpass) {
            *reinterpret_cast<f32x4*>(&red[wave][4 * lane]) = cacc;
            __syncthreads();
            const int jj = c0 + threadIdx.x;
            if (jj < m)
                base[J.ocp + panel * ld + jj] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
            __syncthreads();
        }
    }
    if (dist) {
        __shared__ float red2[4];
        const float s = block_sum4(dsum, red2);
        if (threadIdx.x == 0) a.ws[J.gpart + b * a.P + panel] = s;
    }
}

// merges of the column partials (grid.x = cases x column blocks, grid.y = job), panels summed in order
//   mode 0 (forward pass p): sigma_p,j = 1 / (m sum_panels)            (p == 1 also writes sigma_0 = 1/m)
//   mode 1 (reverse): seed: Cv = colsum(Y), ga = -m sigma_iters Cv;  iteration t: Cv += colsum(W_t), ga = -m so (so gsig + Cv)
//   (sigma = 1 / (m colsum), so d sigma / d colsum = -m sigma^2: the column side carries m where the row side carries n)
//   mode 2 (GW products): grt_j += sum_i G_ij
__global__ __launch_bounds__(NT) void tl_merge_kernel(const SArgs a, int mode) {
    const SJob& J = a.j[blockIdx.y];
    const int m = a.m;
    const int64_t R = cdiv(m, NT);
    const int64_t b = blockIdx.x / R;
    const int j = (int)(blockIdx.x % R) * NT + threadIdx.x;
    if (j >= m) return;
    float* base = a.ws + b * a.per_case;
    const int64_t ld = a.ld, nv = a.nvm, P = a.P;
    const float fm = (float)m;
    const float* cp = base + J.ocp;
    float s = 0.f;
    for (int64_t pp = 0; pp < P; ++pp) s += cp[pp * ld + j];
    if (mode == 0) {
        base[J.os + (int64_t)J.p * nv + j] = 1.f / (fm * s);
        if (J.p == 1) base[J.os + j] = 1.f / fm;
    } else if (mode == 1) {
        float* Cv = base + J.oCv;
        float* ga = base + J.oga;
        if (J.p == J.iters + 1) {
            Cv[j] = s;
            ga[j] = -fm * base[J.os + (int64_t)J.iters * nv + j] * s;
        } else {
            const float* cp2 = cp + P * ld;
            float cw = 0.f;
            for (int64_t pp = 0; pp < P; ++pp) cw += cp2[pp * ld + j];
            const float cv = Cv[j] + cw;
            Cv[j] = cv;
            const float so = base[J.os + (int64_t)(J.p - 1) * nv + j];
            ga[j] = -fm * so * (so * s + cv);
        }
    } else {
        base[J.oH + j] += s;
    }
}

// Reverse row pass (the one-matrix-per-iteration sweep of got_resident.hip, ipot_backward_h, with H in the workspace).
//   seed (p == iters + 1): Y = gscale gT_in . T_iters ; H = iters Y ; Rv = rowsum(Y) ; column partials of Y (set 1)
//   iteration t: Q_t = T_t / (delta_i sigma_j) ; gr_i = -n delta_i^2 (Rv_i / delta_i + sum_j Q ga) ; W = Q . (delta ga^T + gr so^T) ;
//                H += t W (t == 1: written as dL/dC = -(1/beta) H) ; Rv_i += delta_i (Q ga)_i + gr_i (Q so)_i ;
//                column partials of Q gr (set 1) and of W (set 2)
//   (delta = 1 / (n rowsum) gives the factor -n here; sigma = 1 / (m colsum) gives -m in tl_merge_kernel mode 1)
__global__ __launch_bounds__(NT) void tl_bwd_row_kernel(const SArgs a) {
    __shared__ float red[2][4][CW];
    const SJob& J = a.j[blockIdx.y];
    const int64_t b = blockIdx.x / a.P, panel = blockIdx.x % a.P;
    const int n = a.n, m = a.m, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ld = a.ld, nm = a.nm, nvn = a.nvn, nvm = a.nvm, P = a.P;
    float* base = a.ws + b * a.per_case;
    const int t = J.p, iters = J.iters;
    const float fn = (float)n;
    float* __restrict__ H = base + J.oH;
    float* __restrict__ Rv = base + J.oRv;
    const float* __restrict__ ga = base + J.oga;
    float* __restrict__ cp1 = base + J.ocp;
    float* __restrict__ cp2 = cp1 + P * ld;
    if (t == iters + 1) {
        const float gs = J.gscale ? *J.gscale : 1.f;
        const float* __restrict__ Tl = base + J.oT + (int64_t)(iters - 1) * nm;
        const float* __restrict__ gT = base + J.ogTin;
        float rs[RP / 4] = {};
#pragma unroll 1
        for (int c0 = 0; c0 < m; c0 += CW) {
            const int j = c0 + 4 * lane;
            f32x4 cacc = splat4(0.f);
            if (j < m) {
#pragma unroll
                for (int r = 0; r < RP / 4; ++r) {
                    const int64_t i = panel * RP + wave + 4 * r;
                    if (i < n) {
                        const int64_t e = i * ld + j;
                        const f32x4 gv = msk4(*reinterpret_cast<const f32x4*>(gT + e), j, m);
                        const f32x4 tl = msk4(*reinterpret_cast<const f32x4*>(Tl + e), j, m);
                        f32x4 y, h;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            y[q] = gs * gv[q] * tl[q];
                            h[q] = (float)iters * y[q];
                            rs[r] += y[q];
                            cacc[q] += y[q];
                        }
                        *reinterpret_cast<f32x4*>(H + e) = h;
                    }
                }
            }
            *reinterpret_cast<f32x4*>(&red[0][wave][4 * lane]) = cacc;
            __syncthreads();
            const int jj = c0 + threadIdx.x;
            if (jj < m)
                cp1[panel * ld + jj] = (red[0][0][threadIdx.x] + red[0][1][threadIdx.x]) + (red[0][2][threadIdx.x] + red[0][3][threadIdx.x]);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RP / 4; ++r) {
            const int64_t i = panel * RP + wave + 4 * r;
            const float s = wave_sum(rs[r]);
            if (lane == 0 && i < n) Rv[i] = s;
        }
        return;
    }
    const float* __restrict__ Tt = base + J.oT + (int64_t)(t - 1) * nm;
    const float* __restrict__ dlv = base + J.od + (int64_t)(t - 1) * nvn;
    const float* __restrict__ sg = base + J.os + (int64_t)t * nvm;
    const float* __restrict__ so = base + J.os + (int64_t)(t - 1) * nvm;
    const float ft = (float)t;
    auto colvec = [&](const float* v, int j) { return msk4(*reinterpret_cast<const f32x4*>(v + j), j, m); };
    auto rsg4 = [&](int j) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(sg + j);
        f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = j + q < m ? 1.f / s[q] : 0.f;
        return r;
    };
    float di[RP / 4], rdi[RP / 4], gr[RP / 4];
    // phase 1: row sums of Q_t against ga and sigma_{t-1}
#pragma unroll
    for (int r = 0; r < RP / 4; ++r) {
        const int64_t i = panel * RP + wave + 4 * r;
        di[r] = rdi[r] = gr[r] = 0.f;
        if (i < n) {   // wave-uniform
            di[r] = dlv[i];
            rdi[r] = 1.f / di[r];
            float s1 = 0.f, s2 = 0.f;
            for (int j = 4 * lane; j < m; j += CW) {
                const f32x4 tt = msk4(*reinterpret_cast<const f32x4*>(Tt + i * ld + j), j, m);
                const f32x4 rg = rsg4(j), gav = colvec(ga, j), sov = colvec(so, j);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float Qv = tt[q] * rdi[r] * rg[q];
                    s1 += Qv * gav[q];
                    s2 += Qv * sov[q];
                }
            }
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            const float Ri = Rv[i];
            gr[r] = -fn * di[r] * di[r] * (Ri * rdi[r] + s1);
            const float rnew = Ri + di[r] * s1 + gr[r] * s2;
            if (lane == 0) Rv[i] = rnew;
        }
    }
    // phase 2: W, H, column partials
    const float hs = t == 1 ? -J.inv_beta : 1.f;
#pragma unroll 1
    for (int c0 = 0; c0 < m; c0 += CW) {
        const int j = c0 + 4 * lane;
        f32x4 c1 = splat4(0.f), c2 = splat4(0.f);
        if (j < m) {
            const f32x4 rg = rsg4(j), gav = colvec(ga, j), sov = colvec(so, j);
#pragma unroll
            for (int r = 0; r < RP / 4; ++r) {
                const int64_t i = panel * RP + wave + 4 * r;
                if (i < n) {
                    const int64_t e = i * ld + j;
                    const f32x4 tt = msk4(*reinterpret_cast<const f32x4*>(Tt + e), j, m);
                    f32x4 h = *reinterpret_cast<const f32x4*>(H + e);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float Qv = tt[q] * rdi[r] * rg[q];
                        const float w = Qv * (di[r] * gav[q] + gr[r] * sov[q]);
                        h[q] = (h[q] + ft * w) * hs;
                        c1[q] += Qv * gr[r];
                        c2[q] += w;
                    }
                    *reinterpret_cast<f32x4*>(H + e) = h;
                }
            }
        }
        if (t > 1) {
            *reinterpret_cast<f32x4*>(&red[0][wave][4 * lane]) = c1;
            *reinterpret_cast<f32x4*>(&red[1][wave][4 * lane]) = c2;
            __syncthreads();
            const int jj = c0 + threadIdx.x, x = threadIdx.x;
            if (jj < m) {
                cp1[panel * ld + jj] = (red[0][0][x] + red[0][1][x]) + (red[0][2][x] + red[0][3][x]);
                cp2[panel * ld + jj] = (red[1][0][x] + red[1][1][x]) + (red[1][2][x] + red[1][3][x]);
            }
            __syncthreads();
        }
    }
}

// GW products: grs_i += sum_j G_ij (rows of the panel), column partials of G (merged by tl_merge_kernel mode 2 into grt)
__global__ __launch_bounds__(NT) void tl_rowcol_kernel(float* ws, const Lay L, int n, int m) {
    __shared__ float red[4][CW];
    const int64_t b = blockIdx.x / L.P, panel = blockIdx.x % L.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* base = ws + b * L.per_case;
    const int64_t ld = L.ldm;
    const float* G = base + L.oG;
    float rs[RP / 4] = {};
#pragma unroll 1
    for (int c0 = 0; c0 < m; c0 += CW) {
        const int j = c0 + 4 * lane;
        f32x4 cacc = splat4(0.f);
        if (j < m) {
#pragma unroll
            for (int r = 0; r < RP / 4; ++r) {
                const int64_t i = panel * RP + wave + 4 * r;
                if (i < n) {
                    const f32x4 g = msk4(*reinterpret_cast<const f32x4*>(G + i * ld + j), j, m);
                    rs[r] += hsum4(g);
#pragma unroll
                    for (int q = 0; q < 4; ++q) cacc[q] += g[q];
                }
            }
        }
        *reinterpret_cast<f32x4*>(&red[wave][4 * lane]) = cacc;
        __syncthreads();
        const int jj = c0 + threadIdx.x, x = threadIdx.x;
        if (jj < m) base[L.ocpr + panel * ld + jj] = (red[0][x] + red[1][x]) + (red[2][x] + red[3][x]);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RP / 4; ++r) {
        const int64_t i = panel * RP + wave + 4 * r;
        const float s = wave_sum(rs[r]);
        if (lane == 0 && i < n) base[L.ogrs + i] += s;
    }
}

// per-case distances -> out[2] (fixed order)
__global__ __launch_bounds__(NT) void tl_sum_kernel(float* ws, const Lay L, int k, float* out) {
    __shared__ float red[4];
    const float wd = block_sum_array(ws + L.g_wd, (int64_t)k * L.P, 1, red);
    const float gwd = block_sum_array(ws + L.g_gwd, (int64_t)k * L.tiles[0], 1, red);
    if (threadIdx.x == 0) {
        out[0] = wd;
        out[1] = gwd;
    }
}

// reverse seed of the GW branch: G = g1 gamma_5 (the final plan is detached, loss.py:248), zero the accumulated gradients
// (grid: cases x panels over max(n, m) rows)
__global__ __launch_bounds__(NT) void tl_gw_seed_kernel(float* ws, const Lay L, int n, int m, const float* __restrict__ d_out) {
    const int64_t b = blockIdx.x / L.PX, panel = blockIdx.x % L.PX;
    float* base = ws + b * L.per_case;
    const float g = d_out[1];
    const float* gam = base + L.oGT + (int64_t)(GW_OUTER * GW_INNER - 1) * L.nm;
    for (PanelWalk w(L.ldm); w.in(); w.next()) {
        const int64_t i = panel * RP + w.r;
        if (i >= n && i >= m) break;
        const int64_t x = panel * RP * L.ldm + w.e;
        if (i < n) base[L.oG + x] = g * gam[x];
        if (i < m) base[L.ogCt + x] = 0.f;
    }
    for (PanelWalk w(L.ldn); w.in(); w.next()) {
        if (panel * RP + w.r >= n) break;
        base[L.ogCs + panel * RP * L.ldn + w.e] = 0.f;
    }
    if (panel == 0) {
        for (int i = threadIdx.x; i < n; i += NT) base[L.ogrs + i] = 0.f;
        for (int i = threadIdx.x; i < m; i += NT) base[L.ogrt + i] = 0.f;
    }
}

// end of the reverse chain: dL/dC0 = relu mask of (g0 T_30 + WD reverse); dL/dCs0, dL/dCt0 = masks of (gCs + (2/n) Cs grs,
// gCt + (2/m) Ct grt); per-panel threshold-gradient partials (-sum of each masked gradient).  Grid: cases x panels over max(n, m) rows.
__global__ __launch_bounds__(NT) void tl_bwd_final_kernel(float* ws, const Lay L, int n, int m, const float* __restrict__ d_out) {
    __shared__ float red[4];
    const int64_t b = blockIdx.x / L.PX, panel = blockIdx.x % L.PX;
    float* base = ws + b * L.per_case;
    const float g0 = d_out[0], two_n = 2.f / (float)n, two_m = 2.f / (float)m;
    const float t0 = ws[L.g_thr + 6], t1 = ws[L.g_thr + 7], t2 = ws[L.g_thr + 8];
    const float* Tf = base + L.oWT + (int64_t)(WD_ITERS - 1) * L.nm;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (PanelWalk w(L.ldm); w.in(); w.next()) {
        const int64_t i = panel * RP + w.r;
        if (i >= n && i >= m) break;
        if (w.j >= m) continue;
        const int64_t x = panel * RP * L.ldm + w.e;
        if (i < n) {
            const float gc = g0 * Tf[x] + base[L.ogC0 + x];
            const float m0 = (base[L.oC0 + x] - t0 > 0.f) ? gc : 0.f;
            base[L.ogC0 + x] = m0;
            s0 -= m0;
        }
        if (i < m) {
            float at = base[L.ogCt + x] + two_m * base[L.oCt + x] * base[L.ogrt + i];
            at = (base[L.oCt0 + x] - t2 > 0.f) ? at : 0.f;
            base[L.ogCt + x] = at;
            s2 -= at;
        }
    }
    for (PanelWalk w(L.ldn); w.in(); w.next()) {
        const int64_t i = panel * RP + w.r;
        if (i >= n) break;
        if (w.j >= n) continue;
        const int64_t x = panel * RP * L.ldn + w.e;
        float as = base[L.ogCs + x] + two_n * base[L.oCs + x] * base[L.ogrs + i];
        as = (base[L.oCs0 + x] - t1 > 0.f) ? as : 0.f;
        base[L.ogCs + x] = as;
        s1 -= as;
    }
    s0 = block_sum4(s0, red);
    s1 = block_sum4(s1, red);
    s2 = block_sum4(s2, red);
    if (threadIdx.x == 0) {
        float* o = ws + L.g_gthr + (b * L.PX + panel) * 3;
        o[0] = s0;
        o[1] = s1;
        o[2] = s2;
    }
}

// threshold gradients -> d_minmax [6]; batch tie counts (fixed order)
__global__ __launch_bounds__(NT) void tl_thr_bwd_kernel(float* ws, const Lay L, int k, float* d_minmax) {
    __shared__ float red[4];
    const int64_t cnt = (int64_t)k * L.PX;
    for (int m = 0; m < 3; ++m) {
        const float s = block_sum_array(ws + L.g_gthr + m, cnt, 3, red);
        if (threadIdx.x == 0) {
            ws[L.g_thr + 15 + m] = s;
            if (d_minmax) {   // thr = min + beta (max - min)
                d_minmax[2 * m] = (1.f - THR_BETA) * s;
                d_minmax[2 * m + 1] = THR_BETA * s;
            }
        }
    }
    for (int m = 0; m < 6; ++m) {
        const float s = block_sum_array(ws + L.g_cnt + m, cnt, 6, red);
        if (threadIdx.x == 0) ws[L.g_thr + 9 + m] = s;
    }
}

// the extremum gradients, spread evenly over the local elements that attain them (torch's min()/max() backward) -> routed copies
// P1 = d/dC0, P2 = d/dCs0, P3 = d/dCt0 (the reverse chain's results stay untouched)
__global__ __launch_bounds__(NT) void tl_route_kernel(float* ws, const Lay L, int n, int m, const float* __restrict__ d_minmax_total) {
    const int64_t b = blockIdx.x / L.PX, panel = blockIdx.x % L.PX;   // panels over max(n, m) rows
    float* base = ws + b * L.per_case;
    float ex[6], sp[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        ex[q] = ws[L.g_thr + q];
        const float cnt = ws[L.g_thr + 9 + q];
        const float gthr = ws[L.g_thr + 15 + q / 2];
        const float gl = d_minmax_total ? d_minmax_total[q] : ((q & 1) ? THR_BETA * gthr : (1.f - THR_BETA) * gthr);
        sp[q] = cnt > 0.f ? gl / cnt : 0.f;
    }
    for (PanelWalk w(L.ldm); w.in(); w.next()) {
        const int64_t i = panel * RP + w.r;
        if (i >= n && i >= m) break;
        const int64_t x = panel * RP * L.ldm + w.e;
        if (i < n) {
            const float v0 = base[L.oC0 + x];
            float a = base[L.ogC0 + x];
            if (v0 == ex[0]) a += sp[0];
            if (v0 == ex[1]) a += sp[1];
            base[L.oP1 + x] = a;
        }
        if (i < m) {
            const float v2 = base[L.oCt0 + x];
            float z = base[L.ogCt + x];
            if (v2 == ex[4]) z += sp[4];
            if (v2 == ex[5]) z += sp[5];
            base[L.oP3 + x] = z;
        }
    }
    for (PanelWalk w(L.ldn); w.in(); w.next()) {
        const int64_t i = panel * RP + w.r;
        if (i >= n) break;
        const int64_t x = panel * RP * L.ldn + w.e;
        const float v1 = base[L.oCs0 + x];
        float s = base[L.ogCs + x];
        if (v1 == ex[2]) s += sp[2];
        if (v1 == ex[3]) s += sp[3];
        base[L.oP2 + x] = s;
    }
}

// x^ = x / (r + eps):  gx = s gx^ - (<x^, gx^> / r) x^   (one wave per token row)
__global__ __launch_bounds__(NT) void tl_norm_bwd_kernel(float* ws, const Lay L, int n, int m, int d, float* __restrict__ dV,
                                                         float* __restrict__ dQ) {
    const int64_t R = cdiv(n > m ? n : m, 4);
    const int64_t b = blockIdx.x / R;
    const int i = (int)(blockIdx.x % R) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float* base = ws + b * L.per_case;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const int rows = s ? m : n;
        if (i >= rows) continue;   // wave-uniform
        const float* gx = base + (s ? L.ogQh : L.ogVh) + (int64_t)i * d;
        const float* xh = base + (s ? L.oQh : L.oVh) + (int64_t)i * d;
        float dot = 0.f;
        for (int e = lane; e < d; e += 64) dot += xh[e] * gx[e];
        dot = wave_sum(dot);
        const float r = base[(s ? L.orQ : L.orV) + i];
        const float sc = 1.f / (r + 1e-12f);
        const float proj = r > 0.f ? dot / r : 0.f;
        float* out = (s ? dQ : dV) + (b * rows + i) * (int64_t)d;
        for (int e = lane; e < d; e += 64) out[e] = sc * gx[e] - proj * xh[e];
    }
}

// ---------------------------------------------------------------------------------------------------------
// launch sequences (a call gets here through got_run of got_host.hpp, which has checked it; they read their pointers from its record)
// ---------------------------------------------------------------------------------------------------------
struct Ctx {
    float* ws;
    Lay L;
    int k, n, m, d;
    hipStream_t s;
};
static Ctx ctx(const GotCall& g, hipStream_t s) {   // of the one problem of a call
    const GotProb& p = g.b.p[0];
    return Ctx{p.ws, layout(p.k, p.n, g.m, g.b.d), p.k, p.n, g.m, g.b.d, s};
}

static GTerm term(int K, int64_t oA, int64_t lda, bool ta, int64_t oB, int64_t ldb, bool tb, float ca = 0.f, float cb = 0.f) {
    GTerm t{};
    t.K = K;
    t.oA = oA;
    t.oB = oB;
    t.lda = lda;
    t.ldb = ldb;
    t.ca = ca;
    t.cb = cb;
    t.ta = ta;
    t.tb = tb;
    return t;
}
static GJob job(int mode, float alpha, int M, int N, int64_t oC, int64_t ldc) {
    GJob j{};
    j.mode = mode;
    j.alpha = alpha;
    j.M = M;
    j.N = N;
    j.tn = (int)cdiv(N, MT);
    j.tiles = (int)(cdiv(M, MT) * j.tn);
    j.oC = oC;
    j.ldc = ldc;
    return j;
}
static int gemm(const Ctx& c, const GJob* jobs, int nj) {
    GArgs g{};
    g.ws = c.ws;
    g.per_case = c.L.per_case;
    g.k = c.k;
    int tiles = 0;
    for (int i = 0; i < nj; ++i) {
        g.j[i] = jobs[i];
        tiles = jobs[i].tiles > tiles ? jobs[i].tiles : tiles;
    }
    hipLaunchKernelGGL(tl_gemm_kernel, dim3((unsigned)((int64_t)c.k * tiles), nj), dim3(NT), 0, c.s, g);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
static SArgs sargs(const Ctx& c) {
    SArgs a{};
    a.ws = c.ws;
    a.per_case = c.L.per_case;
    a.ld = c.L.ldm;
    a.nm = c.L.nm;
    a.nvn = c.L.nvn;
    a.nvm = c.L.nvm;
    a.P = c.L.P;
    a.n = c.n;
    a.m = c.m;
    return a;
}
static dim3 panels(const Ctx& c, int nj = 1) { return dim3((unsigned)((int64_t)c.k * c.L.P), nj); }      // rows of an n x m matrix
static dim3 xpanels(const Ctx& c) { return dim3((unsigned)((int64_t)c.k * c.L.PX)); }                    // rows of all three cost matrices
static dim3 colblocks(const Ctx& c, int nj = 1) { return dim3((unsigned)((int64_t)c.k * cdiv(c.m, NT)), nj); }
static dim3 tokrows(const Ctx& c) { return dim3((unsigned)((int64_t)c.k * cdiv(c.n > c.m ? c.n : c.m, 4))); }

// IPOT jobs of the two branches (forward and reverse use the same descriptor)
static SJob wd_job(const Ctx& c) {
    const Lay& L = c.L;
    SJob j{};
    j.oCm = L.oC;
    j.oA = L.oAw;
    j.oT = L.oWT;
    j.od = L.oWd;
    j.os = L.oWs;
    j.ocp = L.ocp;
    j.oH = L.ogC0;
    j.ogTin = L.oC;
    j.oRv = L.oRv;
    j.oCv = L.oCv;
    j.oga = L.oga;
    j.gpart = L.g_wd;
    j.iters = WD_ITERS;
    j.inv_beta = WD_INV_BETA;
    return j;
}
static SJob gw_job(const Ctx& c, int o) {
    const Lay& L = c.L;
    SJob j{};
    j.oCm = L.oCg + (int64_t)o * L.nm;
    j.oA = L.oAg;
    j.oT = L.oGT + (int64_t)o * GW_INNER * L.nm;
    j.od = L.oGd + (int64_t)o * GW_INNER * L.nvn;
    j.os = L.oGs + (int64_t)o * (GW_INNER + 1) * L.nvm;
    j.ocp = L.ocp + 2 * L.P * L.ldm;
    j.oH = L.oG;
    j.ogTin = L.ogT;
    j.oRv = L.oRv + L.nvn;
    j.oCv = L.oCv + L.nvm;
    j.oga = L.oga + L.nvm;
    j.gpart = -1;
    j.iters = GW_INNER;
    j.inv_beta = GW_INV_BETA;
    return j;
}

// forward sweeps of up to two jobs, each from pass 1 to iters + 1, aligned at pass 1
static int fwd_sweeps(const Ctx& c, const SJob* jobs, int nj) {
    int maxp = 0;
    for (int i = 0; i < nj; ++i) maxp = jobs[i].iters + 1 > maxp ? jobs[i].iters + 1 : maxp;
    for (int p = 1; p <= maxp; ++p) {
        SArgs a = sargs(c), m = sargs(c);
        int na = 0, nm = 0;
        for (int i = 0; i < nj; ++i) {
            if (p > jobs[i].iters + 1) continue;
            SJob j = jobs[i];
            j.p = p;
            a.j[na++] = j;
            if (p <= j.iters) m.j[nm++] = j;
        }
        hipLaunchKernelGGL(tl_fwd_row_kernel, panels(c, na), dim3(NT), 0, c.s, a);
        MDL_LAUNCH_CHECK();
        if (nm) {
            hipLaunchKernelGGL(tl_merge_kernel, colblocks(c, nm), dim3(NT), 0, c.s, m, 0);
            MDL_LAUNCH_CHECK();
        }
    }
    return MDL_OK;
}
// reverse sweeps of up to two jobs, each from its seed (iters + 1) down to 1, aligned at the seed
static int bwd_sweeps(const Ctx& c, const SJob* jobs, int nj, const float* gscale0) {
    int maxs = 0;
    for (int i = 0; i < nj; ++i) maxs = jobs[i].iters + 1 > maxs ? jobs[i].iters + 1 : maxs;
    for (int s = 0; s < maxs; ++s) {
        SArgs a = sargs(c), m = sargs(c);
        int na = 0, nm = 0;
        for (int i = 0; i < nj; ++i) {
            const int t = jobs[i].iters + 1 - s;
            if (t < 1) continue;
            SJob j = jobs[i];
            j.p = t;
            if (i == 0) j.gscale = gscale0;
            a.j[na++] = j;
            if (t > 1) m.j[nm++] = j;
        }
        hipLaunchKernelGGL(tl_bwd_row_kernel, panels(c, na), dim3(NT), 0, c.s, a);
        MDL_LAUNCH_CHECK();
        if (nm) {
            hipLaunchKernelGGL(tl_merge_kernel, colblocks(c, nm), dim3(NT), 0, c.s, m, 1);
            MDL_LAUNCH_CHECK();
        }
    }
    return MDL_OK;
}

// C_gamma of outer iteration o: P1 = gamma_{o-1} Ct^T (gamma_{-1} = 1/(n m)), then rs_i + rt_j - 2 Cs P1 (o == GW_OUTER: only the
// distance partials sum C_gamma . gamma_4).  Shapes: gamma n x m, Ct m x m, Cs n x n.
static int gw_cgamma(const Ctx& c, int o) {
    const Lay& L = c.L;
    const int n = c.n, m = c.m;
    const int64_t ldn = L.ldn, ldm = L.ldm;
    const float u = 1.f / ((float)n * (float)m);
    const int64_t og = o >= 1 ? L.oGT + ((int64_t)(o - 1) * GW_INNER + (GW_INNER - 1)) * L.nm : -1;
    GJob j1 = job(GM_STORE, 1.f, n, m, L.oP1, ldm);
    j1.t[0] = term(m, og, ldm, false, L.oCt, ldm, true, u);
    j1.nt = 1;
    int rc = gemm(c, &j1, 1);
    if (rc) return rc;
    GJob j2 = job(o < GW_OUTER ? GM_CG : GM_GWD, 1.f, n, m, o < GW_OUTER ? L.oCg + (int64_t)o * L.nm : 0, ldm);
    j2.t[0] = term(n, L.oCs, ldn, false, L.oP1, ldm, false);
    j2.nt = 1;
    j2.oX = L.ors;
    j2.oY = L.ort;
    j2.oZ = og;
    j2.gpart = L.g_gwd;
    return gemm(c, &j2, 1);
}

// M = Cs gam Ct^T with G = d/dC_gamma (C_gamma = Cst - 2 M):  gCs += -2 (G Ct) gam^T (n x n) ; gCt += -2 G^T (Cs gam) (m x m) ;
// d/dgam = -2 Cs^T (G Ct) (n x m, o >= 1);  Cst = rs 1^T + 1 rt^T: grs += rowsum(G), grt += colsum(G)
static int gw_bwd_products(const Ctx& c, int o) {
    const Lay& L = c.L;
    const int n = c.n, m = c.m;
    const int64_t ldn = L.ldn, ldm = L.ldm;
    const float u = 1.f / ((float)n * (float)m);
    const int64_t og = o >= 1 ? L.oGT + ((int64_t)(o - 1) * GW_INNER + (GW_INNER - 1)) * L.nm : -1;
    hipLaunchKernelGGL(tl_rowcol_kernel, panels(c), dim3(NT), 0, c.s, c.ws, L, n, m);
    MDL_LAUNCH_CHECK();
    {
        SArgs mg = sargs(c);
        mg.j[0].ocp = L.ocpr;
        mg.j[0].oH = L.ogrt;
        hipLaunchKernelGGL(tl_merge_kernel, colblocks(c), dim3(NT), 0, c.s, mg, 2);
        MDL_LAUNCH_CHECK();
    }
    GJob a[2];
    a[0] = job(GM_STORE, 1.f, n, m, L.oP1, ldm);   // P1 = G Ct
    a[0].t[0] = term(m, L.oG, ldm, false, L.oCt, ldm, false);
    a[0].nt = 1;
    a[1] = job(GM_STORE, 1.f, n, m, L.oP2, ldm);   // P2 = Cs gam
    a[1].t[0] = term(n, L.oCs, ldn, false, og, ldm, false, 0.f, u);
    a[1].nt = 1;
    int rc = gemm(c, a, 2);
    if (rc) return rc;
    GJob z[3];
    z[0] = job(GM_ACC, -2.f, n, n, L.ogCs, ldn);   // gCs += -2 P1 gam^T
    z[0].t[0] = term(m, L.oP1, ldm, false, og, ldm, true, 0.f, u);
    z[0].nt = 1;
    z[1] = job(GM_ACC, -2.f, m, m, L.ogCt, ldm);   // gCt += -2 G^T P2
    z[1].t[0] = term(n, L.oG, ldm, true, L.oP2, ldm, false);
    z[1].nt = 1;
    z[2] = job(GM_STORE, -2.f, n, m, L.ogT, ldm);  // d/dgam = -2 Cs^T P1
    z[2].t[0] = term(n, L.oCs, ldn, true, L.oP1, ldm, false);
    z[2].nt = 1;
    return gemm(c, z, o >= 1 ? 3 : 2);
}

static int launch_prep(const GotCall& g, hipStream_t s) {
    const Ctx c = ctx(g, s);
    const GotProb& p = g.b.p[0];
    const Lay& L = c.L;
    const int n = c.n, m = c.m, d = c.d;
    hipLaunchKernelGGL(tl_norm_kernel, tokrows(c), dim3(NT), 0, c.s, p.V, p.Q, c.ws, L, n, m, d);
    MDL_LAUNCH_CHECK();
    GJob j[3];
    const int64_t oa[3] = {L.oVh, L.oVh, L.oQh}, ob[3] = {L.oQh, L.oVh, L.oQh}, oc[3] = {L.oC0, L.oCs0, L.oCt0};
    const int64_t ldc[3] = {L.ldm, L.ldn, L.ldm};
    const int rows[3] = {n, n, m}, cols[3] = {m, n, m};
    for (int q = 0; q < 3; ++q) {   // raw costs 1 - <x^_i, y^_j> and per-tile extrema
        j[q] = job(GM_RAW, 1.f, rows[q], cols[q], oc[q], ldc[q]);
        j[q].t[0] = term(d, oa[q], d, false, ob[q], d, true);
        j[q].nt = 1;
        j[q].gpart = L.ext[q];
    }
    int rc = gemm(c, j, 3);
    if (rc) return rc;
    hipLaunchKernelGGL(tl_minmax_kernel, dim3(1), dim3(NT), 0, c.s, c.ws, L, c.k, p.mm_out, p.mm_in);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int launch_main(const GotCall& g, hipStream_t s) {
    const Ctx c = ctx(g, s);
    const Lay& L = c.L;
    hipLaunchKernelGGL(tl_thr_kernel, xpanels(c), dim3(NT), 0, c.s, c.ws, L, c.n, c.m);
    MDL_LAUNCH_CHECK();
    int rc = gw_cgamma(c, 0);
    if (rc) return rc;
    {   // the Wasserstein IPOT beside the first GW IPOT
        const SJob jobs[2] = {wd_job(c), gw_job(c, 0)};
        rc = fwd_sweeps(c, jobs, 2);
        if (rc) return rc;
    }
    for (int o = 1; o < GW_OUTER; ++o) {
        rc = gw_cgamma(c, o);
        if (rc) return rc;
        const SJob jg = gw_job(c, o);
        rc = fwd_sweeps(c, &jg, 1);
        if (rc) return rc;
    }
    rc = gw_cgamma(c, GW_OUTER);
    if (rc) return rc;
    hipLaunchKernelGGL(tl_sum_kernel, dim3(1), dim3(NT), 0, c.s, c.ws, L, c.k, g.b.p[0].out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int launch_bwd_begin(const GotCall& g, hipStream_t s) {
    const Ctx c = ctx(g, s);
    const float* d_out = g.b.p[0].d_out;
    const Lay& L = c.L;
    const int n = c.n, m = c.m;
    hipLaunchKernelGGL(tl_gw_seed_kernel, xpanels(c), dim3(NT), 0, c.s, c.ws, L, n, m, d_out);
    MDL_LAUNCH_CHECK();
    int rc;
    for (int o = GW_OUTER; o >= 0; --o) {
        rc = gw_bwd_products(c, o);
        if (rc) return rc;
        if (o == 0) break;
        if (o == GW_OUTER) {   // the Wasserstein reverse beside the last GW reverse
            const SJob jobs[2] = {wd_job(c), gw_job(c, o - 1)};
            rc = bwd_sweeps(c, jobs, 2, d_out);
        } else {
            const SJob jg = gw_job(c, o - 1);
            rc = bwd_sweeps(c, &jg, 1, nullptr);
        }
        if (rc) return rc;
    }
    hipLaunchKernelGGL(tl_bwd_final_kernel, xpanels(c), dim3(NT), 0, c.s, c.ws, L, n, m, d_out);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(tl_thr_bwd_kernel, dim3(1), dim3(NT), 0, c.s, c.ws, L, c.k, g.b.p[0].d_mm);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

// C0 = 1 - V^ Q^T (n x m), Cs0 = 1 - V^ V^T (n x n), Ct0 = 1 - Q^ Q^T (m x m):
//   gV^ = -(G0 Q^ + Gs V^ + Gs^T V^) (n x d) ;  gQ^ = -(G0^T V^ + Gt Q^ + Gt^T Q^) (m x d)
static int launch_bwd_finish(const GotCall& g, hipStream_t s) {
    const Ctx c = ctx(g, s);
    const GotProb& p = g.b.p[0];
    const Lay& L = c.L;
    const int n = c.n, m = c.m, d = c.d;
    const int64_t ldn = L.ldn, ldm = L.ldm;
    hipLaunchKernelGGL(tl_route_kernel, xpanels(c), dim3(NT), 0, c.s, c.ws, L, n, m, p.d_mm_total);
    MDL_LAUNCH_CHECK();
    GJob j[2];
    j[0] = job(GM_STORE, -1.f, n, d, L.ogVh, d);
    j[0].t[0] = term(m, L.oP1, ldm, false, L.oQh, d, false);
    j[0].t[1] = term(n, L.oP2, ldn, false, L.oVh, d, false);
    j[0].t[2] = term(n, L.oP2, ldn, true, L.oVh, d, false);
    j[0].nt = 3;
    j[1] = job(GM_STORE, -1.f, m, d, L.ogQh, d);
    j[1].t[0] = term(n, L.oP1, ldm, true, L.oVh, d, false);
    j[1].t[1] = term(m, L.oP3, ldm, false, L.oQh, d, false);
    j[1].t[2] = term(m, L.oP3, ldm, true, L.oQh, d, false);
    j[1].nt = 3;
    int rc = gemm(c, j, 2);
    if (rc) return rc;
    hipLaunchKernelGGL(tl_norm_bwd_kernel, tokrows(c), dim3(NT), 0, c.s, c.ws, L, n, m, d, p.dV, p.dQ);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int launch_fwd(const GotCall& g, hipStream_t s) {
    if (const int rc = launch_prep(g, s)) return rc;
    return launch_main(g, s);
}

static int64_t ws_floats(int k, int n, int m, int d) { return layout(k, n, m, d).g_end; }

// mdl_dispatch_plan products 12 (m = n) and 13 (dispatch_plan.hip)
static int plan(int, int n, int m, int, int64_t* o) {
    o[MDL_PLAN_VARIANT] = RP;                             // rows of a sweep panel
    o[MDL_PLAN_PERSIST] = 0;
    o[MDL_PLAN_SPLITS] = cdiv(n, RP);                     // row panels per case (sweep workgroups per case and branch)
    o[MDL_PLAN_TPS] = MT;                                 // output tile edge of the products
    o[MDL_PLAN_EMPTY] = cdiv(n, MT) * cdiv(m, MT);        // product tiles per case of an n x m product
    o[MDL_PLAN_CHUNK] = CW;                               // columns of a sweep chunk
    o[MDL_PLAN_EXTRA] = 2;                                // launches per IPOT iteration (row pass + column merge)
    return MDL_OK;
}

}  // namespace got_tiled

// the tiled row of the engine table (got_host.hpp): one problem per call, Q with a token count of its own
const GotEngine& got_tiled_engine() {
    using namespace got_tiled;
    static const GotEngine e = {TMAXN, TMAXN, TMAXD, 1, 0, ws_floats, {launch_prep, launch_fwd, launch_bwd_begin, launch_bwd_finish}, plan};
    return e;
}
}  // namespace mdl
