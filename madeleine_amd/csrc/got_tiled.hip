// got_tiled.hip -- the TILED size class of GOT (1 <= n <= 4096 tokens, 1 <= d <= 4096): the same forward and reverse sweep as
// got_impl.inc (see its header for the algebra: IPOT, Gromov-Wasserstein, the one-matrix-per-iteration reverse with Y_t = gQ_t . Q_t),
// organised for shapes where one case holds more work than a workgroup -- or two -- can do.
//
// Organisation: many workgroups share one case and meet only at kernel boundaries.
//   * SWEEPS (IPOT forward / reverse): a 256-thread workgroup owns a panel of RP = 16 rows of one case and branch (grid = panels x
//     cases x branches).  A row's reductions are wave-local (each wave owns 4 rows); the column sums an iteration needs are written as
//     per-panel partials [panel][n] and merged, in panel order, by the next launch.  Two launches per IPOT iteration: a row pass
//     (reads A and the previous plan, writes the next plan into the tape, row scaling delta, column partials) and a merge (column
//     scaling sigma).  The forward fuses "write T_{t-1}" into the row pass of iteration t, so a pass reads A and T_{t-2} once
//     (re-read from L2 by the second phase of the pass, which needs the row sums of the first) and writes T_{t-1} once.
//     The reverse keeps the accumulator H = sum_t t W_t (+ iters Y_{iters+1}) in the workspace (read-modify-write per iteration) instead
//     of registers, and the per-row sums of Y in a workspace vector owned by the row's workgroup.
//   * PRODUCTS (n x n x d costs, C_gamma, their adjoints, the cost backward): 128 x 128 output tiles per 256-thread workgroup on
//     v_mfma_f32_32x32x2_f32 (each wave a 64 x 64 block of 2 x 2 accumulators), K-chunks of 16 staged through LDS with a register
//     prefetch of the next chunk; up to three independent products (jobs) per launch, up to three accumulated terms per product.
//   * No workgroup waits for another one of the same launch, no atomics: every cross-workgroup sum (column sums, extrema, tie counts,
//     threshold gradients, per-case distances) is written as partials and merged in a fixed order by a later launch -- two calls give
//     the same bits.
//   * Offsets are 64-bit: one case's tape at n = 4096 is ~2.5e9 floats.
// The WD and GW branches share the sweep launches where their iterations overlap (the Wasserstein IPOT runs beside the first GW IPOT
// in the forward, and its reverse beside the last GW reverse).  Cs and Ct are used with the reference's transposes applied literally.
#include "common.hpp"

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
// workspace: k per-case regions, then the global partials.  Every n x n matrix has row stride ld = up4(n) (16-byte rows).
// ---------------------------------------------------------------------------------------------------------
struct Lay {
    int64_t ld, nn, nv, nd, P, tn, tiles;
    int64_t oVh, oQh, orV, orQ, oC0, oCs0, oCt0, oC, oCs, oCt, ors, ort, oAw, oAg, oWT, oWd, oWs, oCg, oGT, oGd, oGs, oP1, oP2, oP3,
        oG, ogT, ogCs, ogCt, ogC0, ogVh, ogQh, ogrs, ogrt, oRv, oCv, oga, ocp, ocpr;
    int64_t per_case;
    int64_t g_ext, g_cnt, g_wd, g_gwd, g_gthr, g_thr, g_end;
};

__host__ __device__ inline Lay layout(int k, int n, int d) {
    Lay L;
    L.ld = up4(n);
    L.nn = (int64_t)n * L.ld;
    L.nv = up4(n);
    L.nd = up4((int64_t)n * d);
    L.P = cdiv(n, RP);
    L.tn = cdiv(n, MT);
    L.tiles = L.tn * L.tn;
    const int64_t nn = L.nn, nv = L.nv, nd = L.nd, cp = 2 * L.P * L.ld;
    int64_t o = 0;
    L.oVh = o; o += nd;
    L.oQh = o; o += nd;
    L.orV = o; o += nv;
    L.orQ = o; o += nv;
    L.oC0 = o; o += nn;                          // raw costs (masks and extremum routing of the backward)
    L.oCs0 = o; o += nn;
    L.oCt0 = o; o += nn;
    L.oC = o; o += nn;                           // thresholded costs
    L.oCs = o; o += nn;
    L.oCt = o; o += nn;
    L.ors = o; o += nv;                          // Cst vectors
    L.ort = o; o += nv;
    L.oAw = o; o += nn;                          // exp(-C / beta) of the Wasserstein IPOT
    L.oAg = o; o += nn;                          // ... of the GW IPOT in flight
    L.oWT = o; o += nn * WD_ITERS;               // tape: T_1..T_30
    L.oWd = o; o += nv * WD_ITERS;               // delta_1..30
    L.oWs = o; o += nv * (WD_ITERS + 1);         // sigma_0..30
    L.oCg = o; o += nn * GW_OUTER;               // C_gamma of every outer iteration
    L.oGT = o; o += nn * GW_OUTER * GW_INNER;
    L.oGd = o; o += nv * GW_OUTER * GW_INNER;
    L.oGs = o; o += nv * GW_OUTER * (GW_INNER + 1);
    L.oP1 = o; o += nn;                          // product intermediates; routed cost gradients in the backward finish
    L.oP2 = o; o += nn;
    L.oP3 = o; o += nn;
    L.oG = o; o += nn;                           // d/dC_gamma (the GW reverse's H accumulator)
    L.ogT = o; o += nn;                          // d/dgamma
    L.ogCs = o; o += nn;
    L.ogCt = o; o += nn;
    L.ogC0 = o; o += nn;                         // d/dC (the WD reverse's H accumulator), then d/dC0
    L.ogVh = o; o += nd;
    L.ogQh = o; o += nd;
    L.ogrs = o; o += nv;
    L.ogrt = o; o += nv;
    L.oRv = o; o += 2 * nv;                      // per branch: row sums of Y (reverse), column sums of Y, ga
    L.oCv = o; o += 2 * nv;
    L.oga = o; o += 2 * nv;
    L.ocp = o; o += 2 * cp;                      // per branch: two sets of per-panel column partials [P][ld]
    L.ocpr = o; o += L.P * L.ld;                 // column partials of the GW products' Cst gradient
    L.per_case = o;
    int64_t g = (int64_t)k * L.per_case;
    L.g_ext = g; g += up4((int64_t)k * 3 * L.tiles * 2);   // per (kind, case, tile): (min, max)
    L.g_cnt = g; g += up4((int64_t)k * L.P * 6);           // per (case, panel): tie counts of the six extrema
    L.g_wd = g; g += up4((int64_t)k * L.P);                // per (case, panel): Wasserstein distance partial
    L.g_gwd = g; g += up4((int64_t)k * L.tiles);           // per (case, tile): GW distance partial
    L.g_gthr = g; g += up4((int64_t)k * L.P * 3);          // per (case, panel): threshold-gradient partials
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

// ---------------------------------------------------------------------------------------------------------
// K1: normalised tokens and their norms (one wave per token row)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void tl_norm_kernel(const float* __restrict__ V, const float* __restrict__ Q, float* ws, const Lay L,
                                                     int n, int d) {
    const int64_t R = cdiv(n, 4);
    const int64_t b = blockIdx.x / R;
    const int i = (int)(blockIdx.x % R) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;   // no barrier in this kernel
    float* base = ws + b * L.per_case;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const float* src = (s ? Q : V) + (b * n + i) * (int64_t)d;
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
// A term operand with offset < 0 is the constant matrix (ca / cb): the uniform plan gamma_0 = 1/n^2 of the first GW iteration.
// ---------------------------------------------------------------------------------------------------------
enum { GM_RAW = 0, GM_STORE = 1, GM_ACC = 2, GM_CG = 3, GM_GWD = 4 };
struct GTerm {
    int64_t oA, oB, lda, ldb;   // per-case offsets (< 0: constant operand); A(i,k) = ta ? A[k lda + i] : A[i lda + k]; B likewise
    float ca, cb;
    int ta, tb;
};
struct GJob {
    GTerm t[3];
    int nt, mode;
    float alpha;
    int64_t oC, ldc;            // output (per case)
    int64_t oX, oY, oZ;         // GM_CG / GM_GWD: rs, rt (vectors), gamma (GM_GWD)
    int64_t gpart;              // GM_RAW / GM_GWD: global offset of the per-(case, tile) partials
};
constexpr int GMAXJ = 3;
struct GArgs {
    float* ws;
    int64_t per_case;
    int M, N, K, tn, tiles;
    GJob j[GMAXJ];
};

__global__ __launch_bounds__(NT) void tl_gemm_kernel(const GArgs g) {
    __shared__ float xs[MK * LDX];
    __shared__ float ys[MK * LDX];
    __shared__ float red[8];
    const GJob& J = g.j[blockIdx.y];
    const int64_t b = blockIdx.x / g.tiles;
    const int tile = (int)(blockIdx.x % g.tiles);
    const int i0 = (tile / g.tn) * MT, j0 = (tile % g.tn) * MT;
    float* base = g.ws + b * g.per_case;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int bi0 = (wave >> 1) * 64, bj0 = (wave & 1) * 64;
    const int M = g.M, N = g.N, K = g.K;
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
            float* o = g.ws + J.gpart + (b * g.tiles + tile) * 2;
            o[0] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
            o[1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        }
    } else if (mode == GM_GWD) {
        const float s = block_sum4(sacc, red);
        if (tid == 0) g.ws[J.gpart + b * g.tiles + tile] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// K3: extrema of the three raw cost tensors over the whole batch -> minmax_out; thresholds (minmax_in if given)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void tl_minmax_kernel(float* ws, const Lay L, int k, float* minmax_out, const float* minmax_in) {
    __shared__ float red[8];
    __shared__ float ext[6];
    const int tid = threadIdx.x;
    const int64_t cnt = (int64_t)k * L.tiles;
    for (int m = 0; m < 3; ++m) {
        const float* src = ws + L.g_ext + (int64_t)m * cnt * 2;
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
__global__ __launch_bounds__(NT) void tl_thr_kernel(float* ws, const Lay L, int n) {
    __shared__ float red[4];
    const int64_t b = blockIdx.x / L.P, panel = blockIdx.x % L.P;
    float* base = ws + b * L.per_case;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ld = L.ld;
    float ex[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) ex[m] = ws[L.g_thr + m];
    const float t0 = ws[L.g_thr + 6], t1 = ws[L.g_thr + 7], t2 = ws[L.g_thr + 8];
    float cnt[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int r = 0; r < RP / 4; ++r) {
        const int i = (int)panel * RP + wave + 4 * r;
        if (i >= n) break;   // wave-uniform; no barrier until the loop ends
        float as = 0.f, at = 0.f;
        for (int j = 4 * lane; j < n; j += CW) {
            const int64_t e = i * ld + j;
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(base + L.oC0 + e);
            const f32x4 xs = *reinterpret_cast<const f32x4*>(base + L.oCs0 + e);
            const f32x4 xt = *reinterpret_cast<const f32x4*>(base + L.oCt0 + e);
            f32x4 c, cs, ct;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool ok = j + q < n;
                c[q] = ok ? fmaxf(x0[q] - t0, 0.f) : 0.f;
                cs[q] = ok ? fmaxf(xs[q] - t1, 0.f) : 0.f;
                ct[q] = ok ? fmaxf(xt[q] - t2, 0.f) : 0.f;
                cnt[0] += ok && x0[q] == ex[0];
                cnt[1] += ok && x0[q] == ex[1];
                cnt[2] += ok && xs[q] == ex[2];
                cnt[3] += ok && xs[q] == ex[3];
                cnt[4] += ok && xt[q] == ex[4];
                cnt[5] += ok && xt[q] == ex[5];
                as += cs[q] * cs[q];
                at += ct[q] * ct[q];
            }
            *reinterpret_cast<f32x4*>(base + L.oC + e) = c;
            *reinterpret_cast<f32x4*>(base + L.oCs + e) = cs;
            *reinterpret_cast<f32x4*>(base + L.oCt + e) = ct;
        }
        as = wave_sum(as);
        at = wave_sum(at);
        if (lane == 0) {
            base[L.ors + i] = as / (float)n;   // rs_i = (1/n) sum_k Cs_ik^2 ; rt_j = (1/n) sum_l Ct_jl^2  (loss.py:240-241)
            base[L.ort + i] = at / (float)n;
        }
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const float s = block_sum4(cnt[m], red);
        if (threadIdx.x == 0) ws[L.g_cnt + (b * L.P + panel) * 6 + m] = s;
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
    int64_t per_case, ld, nn, nv, P;
    int n;
    SJob j[2];
};

// Forward row pass p: T_{p-1} = delta_{p-1} (A . T_{p-2}) sigma_{p-1} is written to the tape (p >= 2; T_0 = 1); for p <= iters the pass
// continues with Q_p = A . T_{p-1}: delta_p,i = 1 / (n sum_j Q_p,ij sigma_{p-1,j}) and the column partials sum_{i in panel} Q_p,ij delta_p,i.
// p == 1 forms A = exp(-C / beta) from the cost and stores it.  p == iters + 1 only writes T_iters (and the distance partial sum C . T).
__global__ __launch_bounds__(NT) void tl_fwd_row_kernel(const SArgs a) {
    __shared__ float red[4][CW];
    const SJob& J = a.j[blockIdx.y];
    const int64_t b = blockIdx.x / a.P, panel = blockIdx.x % a.P;
    const int n = a.n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ld = a.ld, nn = a.nn, nv = a.nv;
    float* base = a.ws + b * a.per_case;
    const int p = J.p, iters = J.iters;
    const float fn = (float)n, inv_n = 1.f / fn, ib = J.inv_beta;
    float* __restrict__ A = base + J.oA;
    const float* __restrict__ Cm = base + J.oCm;
    const float* __restrict__ Tpp = base + J.oT + (int64_t)(p >= 3 ? p - 3 : 0) * nn;      // T_{p-2}
    float* __restrict__ Tw = base + J.oT + (int64_t)(p >= 2 ? p - 2 : 0) * nn;             // T_{p-1}
    const float* __restrict__ dprev = base + J.od + (int64_t)(p >= 2 ? p - 2 : 0) * nv;    // delta_{p-1}
    const float* __restrict__ sprev = base + J.os + (int64_t)(p - 1) * nv;                 // sigma_{p-1}
    const bool rowpass = p <= iters;
    const bool dist = p == iters + 1 && J.gpart >= 0;
    // A and T_{p-1} at row i, columns j .. j + 3 (columns >= n read as 0)
    auto elem = [&](int64_t i, int j, float di, f32x4& Av, f32x4& Tv) {
        const int64_t e = i * ld + j;
        if (p == 1) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(Cm + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) Av[q] = expf(-c[q] * ib);
            Av = msk4(Av, j, n);
            Tv = msk4(splat4(1.f), j, n);
        } else {
            Av = msk4(*reinterpret_cast<const f32x4*>(A + e), j, n);
            const f32x4 tp = p >= 3 ? msk4(*reinterpret_cast<const f32x4*>(Tpp + e), j, n) : splat4(1.f);
            const f32x4 sq = msk4(*reinterpret_cast<const f32x4*>(sprev + j), j, n);
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
                for (int j = 4 * lane; j < n; j += CW) {
                    f32x4 Av, Tv;
                    elem(i, j, dp[r], Av, Tv);
                    const f32x4 sq = p == 1 ? msk4(splat4(inv_n), j, n) : msk4(*reinterpret_cast<const f32x4*>(sprev + j), j, n);
#pragma unroll
                    for (int q = 0; q < 4; ++q) s += (Av[q] * Tv[q]) * sq[q];
                }
                s = wave_sum(s);
                dl[r] = 1.f / (fn * s);
                if (lane == 0) base[J.od + (int64_t)(p - 1) * nv + i] = dl[r];
            }
        }
    }
    // phase 2: write A (p == 1) / T_{p-1} (p >= 2); column partials of Q_p delta_p
    float dsum = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += CW) {
        const int j = c0 + 4 * lane;
        f32x4 cacc = splat4(0.f);
        if (j < n) {
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
                        const f32x4 c = msk4(*reinterpret_cast<const f32x4*>(Cm + e), j, n);
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
            if (jj < n)
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
//   mode 0 (forward pass p): sigma_p,j = 1 / (n sum_panels)            (p == 1 also writes sigma_0 = 1/n)
//   mode 1 (reverse): seed: Cv = colsum(Y), ga = -n sigma_iters Cv;  iteration t: Cv += colsum(W_t), ga = -n so (so gsig + Cv)
//   mode 2 (GW products): grt_j += sum_i G_ij
__global__ __launch_bounds__(NT) void tl_merge_kernel(const SArgs a, int mode) {
    const SJob& J = a.j[blockIdx.y];
    const int n = a.n;
    const int64_t R = cdiv(n, NT);
    const int64_t b = blockIdx.x / R;
    const int j = (int)(blockIdx.x % R) * NT + threadIdx.x;
    if (j >= n) return;
    float* base = a.ws + b * a.per_case;
    const int64_t ld = a.ld, nv = a.nv, P = a.P;
    const float fn = (float)n;
    const float* cp = base + J.ocp;
    float s = 0.f;
    for (int64_t pp = 0; pp < P; ++pp) s += cp[pp * ld + j];
    if (mode == 0) {
        base[J.os + (int64_t)J.p * nv + j] = 1.f / (fn * s);
        if (J.p == 1) base[J.os + j] = 1.f / fn;
    } else if (mode == 1) {
        float* Cv = base + J.oCv;
        float* ga = base + J.oga;
        if (J.p == J.iters + 1) {
            Cv[j] = s;
            ga[j] = -fn * base[J.os + (int64_t)J.iters * nv + j] * s;
        } else {
            const float* cp2 = cp + P * ld;
            float cw = 0.f;
            for (int64_t pp = 0; pp < P; ++pp) cw += cp2[pp * ld + j];
            const float cv = Cv[j] + cw;
            Cv[j] = cv;
            const float so = base[J.os + (int64_t)(J.p - 1) * nv + j];
            ga[j] = -fn * so * (so * s + cv);
        }
    } else {
        base[J.oH + j] += s;
    }
}

// Reverse row pass (the one-matrix-per-iteration sweep of got_impl.inc, ipot_backward_h, with H in the workspace).
//   seed (p == iters + 1): Y = gscale gT_in . T_iters ; H = iters Y ; Rv = rowsum(Y) ; column partials of Y (set 1)
//   iteration t: Q_t = T_t / (delta_i sigma_j) ; gr_i = -n delta_i^2 (Rv_i / delta_i + sum_j Q ga) ; W = Q . (delta ga^T + gr so^T) ;
//                H += t W (t == 1: written as dL/dC = -(1/beta) H) ; Rv_i += delta_i (Q ga)_i + gr_i (Q so)_i ;
//                column partials of Q gr (set 1) and of W (set 2)
__global__ __launch_bounds__(NT) void tl_bwd_row_kernel(const SArgs a) {
    __shared__ float red[2][4][CW];
    const SJob& J = a.j[blockIdx.y];
    const int64_t b = blockIdx.x / a.P, panel = blockIdx.x % a.P;
    const int n = a.n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ld = a.ld, nn = a.nn, nv = a.nv, P = a.P;
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
        const float* __restrict__ Tl = base + J.oT + (int64_t)(iters - 1) * nn;
        const float* __restrict__ gT = base + J.ogTin;
        float rs[RP / 4] = {};
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += CW) {
            const int j = c0 + 4 * lane;
            f32x4 cacc = splat4(0.f);
            if (j < n) {
#pragma unroll
                for (int r = 0; r < RP / 4; ++r) {
                    const int64_t i = panel * RP + wave + 4 * r;
                    if (i < n) {
                        const int64_t e = i * ld + j;
                        const f32x4 gv = msk4(*reinterpret_cast<const f32x4*>(gT + e), j, n);
                        const f32x4 tl = msk4(*reinterpret_cast<const f32x4*>(Tl + e), j, n);
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
            if (jj < n)
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
    const float* __restrict__ Tt = base + J.oT + (int64_t)(t - 1) * nn;
    const float* __restrict__ dlv = base + J.od + (int64_t)(t - 1) * nv;
    const float* __restrict__ sg = base + J.os + (int64_t)t * nv;
    const float* __restrict__ so = base + J.os + (int64_t)(t - 1) * nv;
    const float ft = (float)t;
    auto colvec = [&](const float* v, int j) { return msk4(*reinterpret_cast<const f32x4*>(v + j), j, n); };
    auto rsg4 = [&](int j) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(sg + j);
        f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = j + q < n ? 1.f / s[q] : 0.f;
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
            for (int j = 4 * lane; j < n; j += CW) {
                const f32x4 tt = msk4(*reinterpret_cast<const f32x4*>(Tt + i * ld + j), j, n);
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
    for (int c0 = 0; c0 < n; c0 += CW) {
        const int j = c0 + 4 * lane;
        f32x4 c1 = splat4(0.f), c2 = splat4(0.f);
        if (j < n) {
            const f32x4 rg = rsg4(j), gav = colvec(ga, j), sov = colvec(so, j);
#pragma unroll
            for (int r = 0; r < RP / 4; ++r) {
                const int64_t i = panel * RP + wave + 4 * r;
                if (i < n) {
                    const int64_t e = i * ld + j;
                    const f32x4 tt = msk4(*reinterpret_cast<const f32x4*>(Tt + e), j, n);
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
            if (jj < n) {
                cp1[panel * ld + jj] = (red[0][0][x] + red[0][1][x]) + (red[0][2][x] + red[0][3][x]);
                cp2[panel * ld + jj] = (red[1][0][x] + red[1][1][x]) + (red[1][2][x] + red[1][3][x]);
            }
            __syncthreads();
        }
    }
}

// GW products: grs_i += sum_j G_ij (rows of the panel), column partials of G (merged by tl_merge_kernel mode 2 into grt)
__global__ __launch_bounds__(NT) void tl_rowcol_kernel(float* ws, const Lay L, int n) {
    __shared__ float red[4][CW];
    const int64_t b = blockIdx.x / L.P, panel = blockIdx.x % L.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* base = ws + b * L.per_case;
    const int64_t ld = L.ld;
    const float* G = base + L.oG;
    float rs[RP / 4] = {};
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += CW) {
        const int j = c0 + 4 * lane;
        f32x4 cacc = splat4(0.f);
        if (j < n) {
#pragma unroll
            for (int r = 0; r < RP / 4; ++r) {
                const int64_t i = panel * RP + wave + 4 * r;
                if (i < n) {
                    const f32x4 g = msk4(*reinterpret_cast<const f32x4*>(G + i * ld + j), j, n);
                    rs[r] += hsum4(g);
#pragma unroll
                    for (int q = 0; q < 4; ++q) cacc[q] += g[q];
                }
            }
        }
        *reinterpret_cast<f32x4*>(&red[wave][4 * lane]) = cacc;
        __syncthreads();
        const int jj = c0 + threadIdx.x, x = threadIdx.x;
        if (jj < n) base[L.ocpr + panel * ld + jj] = (red[0][x] + red[1][x]) + (red[2][x] + red[3][x]);
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
    const float gwd = block_sum_array(ws + L.g_gwd, (int64_t)k * L.tiles, 1, red);
    if (threadIdx.x == 0) {
        out[0] = wd;
        out[1] = gwd;
    }
}

// reverse seed of the GW branch: G = g1 gamma_5 (the final plan is detached, loss.py:248), zero the accumulated gradients
__global__ __launch_bounds__(NT) void tl_gw_seed_kernel(float* ws, const Lay L, int n, const float* __restrict__ d_out) {
    const int64_t b = blockIdx.x / L.P, panel = blockIdx.x % L.P;
    float* base = ws + b * L.per_case;
    const float g = d_out[1];
    const float* gam = base + L.oGT + (int64_t)(GW_OUTER * GW_INNER - 1) * L.nn;
    for (int e = threadIdx.x; e < RP * L.ld; e += NT) {
        const int64_t i = panel * RP + e / L.ld;
        if (i >= n) break;
        const int64_t x = panel * RP * L.ld + e;
        base[L.oG + x] = g * gam[x];
        base[L.ogCs + x] = 0.f;
        base[L.ogCt + x] = 0.f;
    }
    if (panel == 0)
        for (int i = threadIdx.x; i < n; i += NT) {
            base[L.ogrs + i] = 0.f;
            base[L.ogrt + i] = 0.f;
        }
}

// end of the reverse chain: dL/dC0 = relu mask of (g0 T_30 + WD reverse); dL/dCs0, dL/dCt0 = masks of (gCs + (2/n) Cs grs, ...);
// per-panel threshold-gradient partials (-sum of each masked gradient)
__global__ __launch_bounds__(NT) void tl_bwd_final_kernel(float* ws, const Lay L, int n, const float* __restrict__ d_out) {
    __shared__ float red[4];
    const int64_t b = blockIdx.x / L.P, panel = blockIdx.x % L.P;
    float* base = ws + b * L.per_case;
    const float g0 = d_out[0], two_n = 2.f / (float)n;
    const float t0 = ws[L.g_thr + 6], t1 = ws[L.g_thr + 7], t2 = ws[L.g_thr + 8];
    const float* Tf = base + L.oWT + (int64_t)(WD_ITERS - 1) * L.nn;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int e = threadIdx.x; e < RP * L.ld; e += NT) {
        const int64_t i = panel * RP + e / L.ld;
        const int j = (int)(e % L.ld);
        if (i >= n) break;
        if (j >= n) continue;
        const int64_t x = panel * RP * L.ld + e;
        const float gc = g0 * Tf[x] + base[L.ogC0 + x];
        const float m0 = (base[L.oC0 + x] - t0 > 0.f) ? gc : 0.f;
        base[L.ogC0 + x] = m0;
        s0 -= m0;
        float as = base[L.ogCs + x] + two_n * base[L.oCs + x] * base[L.ogrs + i];
        float at = base[L.ogCt + x] + two_n * base[L.oCt + x] * base[L.ogrt + i];
        as = (base[L.oCs0 + x] - t1 > 0.f) ? as : 0.f;
        at = (base[L.oCt0 + x] - t2 > 0.f) ? at : 0.f;
        base[L.ogCs + x] = as;
        base[L.ogCt + x] = at;
        s1 -= as;
        s2 -= at;
    }
    s0 = block_sum4(s0, red);
    s1 = block_sum4(s1, red);
    s2 = block_sum4(s2, red);
    if (threadIdx.x == 0) {
        float* o = ws + L.g_gthr + (b * L.P + panel) * 3;
        o[0] = s0;
        o[1] = s1;
        o[2] = s2;
    }
}

// threshold gradients -> d_minmax [6]; batch tie counts (fixed order)
__global__ __launch_bounds__(NT) void tl_thr_bwd_kernel(float* ws, const Lay L, int k, float* d_minmax) {
    __shared__ float red[4];
    const int64_t cnt = (int64_t)k * L.P;
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
__global__ __launch_bounds__(NT) void tl_route_kernel(float* ws, const Lay L, int n, const float* __restrict__ d_minmax_total) {
    const int64_t b = blockIdx.x / L.P, panel = blockIdx.x % L.P;
    float* base = ws + b * L.per_case;
    float ex[6], sp[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        ex[m] = ws[L.g_thr + m];
        const float cnt = ws[L.g_thr + 9 + m];
        const float gthr = ws[L.g_thr + 15 + m / 2];
        const float gl = d_minmax_total ? d_minmax_total[m] : ((m & 1) ? THR_BETA * gthr : (1.f - THR_BETA) * gthr);
        sp[m] = cnt > 0.f ? gl / cnt : 0.f;
    }
    for (int e = threadIdx.x; e < RP * L.ld; e += NT) {
        const int64_t i = panel * RP + e / L.ld;
        if (i >= n) break;
        const int64_t x = panel * RP * L.ld + e;
        const float v0 = base[L.oC0 + x], v1 = base[L.oCs0 + x], v2 = base[L.oCt0 + x];
        float a = base[L.ogC0 + x], s = base[L.ogCs + x], z = base[L.ogCt + x];
        if (v0 == ex[0]) a += sp[0];
        if (v0 == ex[1]) a += sp[1];
        if (v1 == ex[2]) s += sp[2];
        if (v1 == ex[3]) s += sp[3];
        if (v2 == ex[4]) z += sp[4];
        if (v2 == ex[5]) z += sp[5];
        base[L.oP1 + x] = a;
        base[L.oP2 + x] = s;
        base[L.oP3 + x] = z;
    }
}

// x^ = x / (r + eps):  gx = s gx^ - (<x^, gx^> / r) x^   (one wave per token row)
__global__ __launch_bounds__(NT) void tl_norm_bwd_kernel(float* ws, const Lay L, int n, int d, float* __restrict__ dV,
                                                         float* __restrict__ dQ) {
    const int64_t R = cdiv(n, 4);
    const int64_t b = blockIdx.x / R;
    const int i = (int)(blockIdx.x % R) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* base = ws + b * L.per_case;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const float* gx = base + (s ? L.ogQh : L.ogVh) + (int64_t)i * d;
        const float* xh = base + (s ? L.oQh : L.oVh) + (int64_t)i * d;
        float dot = 0.f;
        for (int e = lane; e < d; e += 64) dot += xh[e] * gx[e];
        dot = wave_sum(dot);
        const float r = base[(s ? L.orQ : L.orV) + i];
        const float sc = 1.f / (r + 1e-12f);
        const float proj = r > 0.f ? dot / r : 0.f;
        float* out = (s ? dQ : dV) + (b * n + i) * (int64_t)d;
        for (int e = lane; e < d; e += 64) out[e] = sc * gx[e] - proj * xh[e];
    }
}

// ---------------------------------------------------------------------------------------------------------
// launch sequences
// ---------------------------------------------------------------------------------------------------------
struct Ctx {
    float* ws;
    Lay L;
    int k, n, d;
    hipStream_t s;
};

static GTerm term(int64_t oA, int64_t lda, bool ta, int64_t oB, int64_t ldb, bool tb, float ca = 0.f, float cb = 0.f) {
    GTerm t{};
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
static GJob job(int mode, float alpha, int64_t oC, int64_t ldc) {
    GJob j{};
    j.mode = mode;
    j.alpha = alpha;
    j.oC = oC;
    j.ldc = ldc;
    return j;
}
static int gemm(const Ctx& c, int M, int N, int K, const GJob* jobs, int nj) {
    GArgs g{};
    g.ws = c.ws;
    g.per_case = c.L.per_case;
    g.M = M;
    g.N = N;
    g.K = K;
    g.tn = (int)cdiv(N, MT);
    g.tiles = (int)(cdiv(M, MT) * g.tn);
    for (int i = 0; i < nj; ++i) g.j[i] = jobs[i];
    hipLaunchKernelGGL(tl_gemm_kernel, dim3((unsigned)((int64_t)c.k * g.tiles), nj), dim3(NT), 0, c.s, g);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
static SArgs sargs(const Ctx& c) {
    SArgs a{};
    a.ws = c.ws;
    a.per_case = c.L.per_case;
    a.ld = c.L.ld;
    a.nn = c.L.nn;
    a.nv = c.L.nv;
    a.P = c.L.P;
    a.n = c.n;
    return a;
}
static dim3 panels(const Ctx& c, int nj = 1) { return dim3((unsigned)((int64_t)c.k * c.L.P), nj); }
static dim3 colblocks(const Ctx& c, int nj = 1) { return dim3((unsigned)((int64_t)c.k * cdiv(c.n, NT)), nj); }

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
    j.oCm = L.oCg + (int64_t)o * L.nn;
    j.oA = L.oAg;
    j.oT = L.oGT + (int64_t)o * GW_INNER * L.nn;
    j.od = L.oGd + (int64_t)o * GW_INNER * L.nv;
    j.os = L.oGs + (int64_t)o * (GW_INNER + 1) * L.nv;
    j.ocp = L.ocp + 2 * L.P * L.ld;
    j.oH = L.oG;
    j.ogTin = L.ogT;
    j.oRv = L.oRv + L.nv;
    j.oCv = L.oCv + L.nv;
    j.oga = L.oga + L.nv;
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

// C_gamma of outer iteration o: P1 = gamma_{o-1} Ct^T (gamma_{-1} = 1/n^2), then rs_i + rt_j - 2 Cs P1 (o == GW_OUTER: only the distance
// partials sum C_gamma . gamma_4)
static int gw_cgamma(const Ctx& c, int o) {
    const Lay& L = c.L;
    const int n = c.n;
    const int64_t ld = L.ld;
    const float u = 1.f / ((float)n * (float)n);
    const int64_t og = o >= 1 ? L.oGT + ((int64_t)(o - 1) * GW_INNER + (GW_INNER - 1)) * L.nn : -1;
    GJob j1 = job(GM_STORE, 1.f, L.oP1, ld);
    j1.t[0] = term(og, ld, false, L.oCt, ld, true, u);
    j1.nt = 1;
    int rc = gemm(c, n, n, n, &j1, 1);
    if (rc) return rc;
    GJob j2 = job(o < GW_OUTER ? GM_CG : GM_GWD, 1.f, o < GW_OUTER ? L.oCg + (int64_t)o * L.nn : 0, ld);
    j2.t[0] = term(L.oCs, ld, false, L.oP1, ld, false);
    j2.nt = 1;
    j2.oX = L.ors;
    j2.oY = L.ort;
    j2.oZ = og;
    j2.gpart = L.g_gwd;
    return gemm(c, n, n, n, &j2, 1);
}

// M = Cs gam Ct^T with G = d/dC_gamma (C_gamma = Cst - 2 M):  gCs += -2 G Ct gam^T ; gCt += -2 G^T Cs gam ; d/dgam = -2 Cs^T G Ct
// (o >= 1);  Cst = rs 1^T + 1 rt^T: grs += rowsum(G), grt += colsum(G)
static int gw_bwd_products(const Ctx& c, int o) {
    const Lay& L = c.L;
    const int n = c.n;
    const int64_t ld = L.ld;
    const float u = 1.f / ((float)n * (float)n);
    const int64_t og = o >= 1 ? L.oGT + ((int64_t)(o - 1) * GW_INNER + (GW_INNER - 1)) * L.nn : -1;
    hipLaunchKernelGGL(tl_rowcol_kernel, panels(c), dim3(NT), 0, c.s, c.ws, L, n);
    MDL_LAUNCH_CHECK();
    {
        SArgs m = sargs(c);
        m.j[0].ocp = L.ocpr;
        m.j[0].oH = L.ogrt;
        hipLaunchKernelGGL(tl_merge_kernel, colblocks(c), dim3(NT), 0, c.s, m, 2);
        MDL_LAUNCH_CHECK();
    }
    GJob a[2];
    a[0] = job(GM_STORE, 1.f, L.oP1, ld);   // P1 = G Ct
    a[0].t[0] = term(L.oG, ld, false, L.oCt, ld, false);
    a[0].nt = 1;
    a[1] = job(GM_STORE, 1.f, L.oP2, ld);   // P2 = Cs gam
    a[1].t[0] = term(L.oCs, ld, false, og, ld, false, 0.f, u);
    a[1].nt = 1;
    int rc = gemm(c, n, n, n, a, 2);
    if (rc) return rc;
    GJob z[3];
    z[0] = job(GM_ACC, -2.f, L.ogCs, ld);   // gCs += -2 P1 gam^T
    z[0].t[0] = term(L.oP1, ld, false, og, ld, true, 0.f, u);
    z[0].nt = 1;
    z[1] = job(GM_ACC, -2.f, L.ogCt, ld);   // gCt += -2 G^T P2
    z[1].t[0] = term(L.oG, ld, true, L.oP2, ld, false);
    z[1].nt = 1;
    z[2] = job(GM_STORE, -2.f, L.ogT, ld);  // d/dgam = -2 Cs^T P1
    z[2].t[0] = term(L.oCs, ld, true, L.oP1, ld, false);
    z[2].nt = 1;
    return gemm(c, n, n, n, z, o >= 1 ? 3 : 2);
}

int launch_prep(const Ctx& c, float* minmax_out, const float* minmax_in, const float* V, const float* Q) {
    const Lay& L = c.L;
    const int n = c.n, d = c.d;
    hipLaunchKernelGGL(tl_norm_kernel, dim3((unsigned)((int64_t)c.k * cdiv(n, 4))), dim3(NT), 0, c.s, V, Q, c.ws, L, n, d);
    MDL_LAUNCH_CHECK();
    GJob j[3];
    const int64_t oa[3] = {L.oVh, L.oVh, L.oQh}, ob[3] = {L.oQh, L.oVh, L.oQh}, oc[3] = {L.oC0, L.oCs0, L.oCt0};
    for (int m = 0; m < 3; ++m) {   // raw costs 1 - <x^_i, y^_j> and per-tile extrema
        j[m] = job(GM_RAW, 1.f, oc[m], L.ld);
        j[m].t[0] = term(oa[m], d, false, ob[m], d, true);
        j[m].nt = 1;
        j[m].gpart = L.g_ext + (int64_t)m * c.k * L.tiles * 2;
    }
    int rc = gemm(c, n, n, d, j, 3);
    if (rc) return rc;
    hipLaunchKernelGGL(tl_minmax_kernel, dim3(1), dim3(NT), 0, c.s, c.ws, L, c.k, minmax_out, minmax_in);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

int launch_main(const Ctx& c, float* out) {
    const Lay& L = c.L;
    hipLaunchKernelGGL(tl_thr_kernel, panels(c), dim3(NT), 0, c.s, c.ws, L, c.n);
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
    hipLaunchKernelGGL(tl_sum_kernel, dim3(1), dim3(NT), 0, c.s, c.ws, L, c.k, out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

int launch_bwd_begin(const Ctx& c, const float* d_out, float* d_minmax) {
    const Lay& L = c.L;
    const int n = c.n;
    hipLaunchKernelGGL(tl_gw_seed_kernel, panels(c), dim3(NT), 0, c.s, c.ws, L, n, d_out);
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
    hipLaunchKernelGGL(tl_bwd_final_kernel, panels(c), dim3(NT), 0, c.s, c.ws, L, n, d_out);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(tl_thr_bwd_kernel, dim3(1), dim3(NT), 0, c.s, c.ws, L, c.k, d_minmax);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

// C0 = 1 - V^ Q^T, Cs0 = 1 - V^ V^T, Ct0 = 1 - Q^ Q^T:
//   gV^ = -(G0 Q^ + Gs V^ + Gs^T V^) ;  gQ^ = -(G0^T V^ + Gt Q^ + Gt^T Q^)
int launch_bwd_finish(const Ctx& c, const float* d_minmax_total, float* dV, float* dQ) {
    const Lay& L = c.L;
    const int n = c.n, d = c.d;
    const int64_t ld = L.ld;
    hipLaunchKernelGGL(tl_route_kernel, panels(c), dim3(NT), 0, c.s, c.ws, L, n, d_minmax_total);
    MDL_LAUNCH_CHECK();
    GJob j[2];
    j[0] = job(GM_STORE, -1.f, L.ogVh, d);
    j[0].t[0] = term(L.oP1, ld, false, L.oQh, d, false);
    j[0].t[1] = term(L.oP2, ld, false, L.oVh, d, false);
    j[0].t[2] = term(L.oP2, ld, true, L.oVh, d, false);
    j[0].nt = 3;
    j[1] = job(GM_STORE, -1.f, L.ogQh, d);
    j[1].t[0] = term(L.oP1, ld, true, L.oVh, d, false);
    j[1].t[1] = term(L.oP3, ld, false, L.oQh, d, false);
    j[1].t[2] = term(L.oP3, ld, true, L.oQh, d, false);
    j[1].nt = 3;
    int rc = gemm(c, n, d, n, j, 2);
    if (rc) return rc;
    hipLaunchKernelGGL(tl_norm_bwd_kernel, dim3((unsigned)((int64_t)c.k * cdiv(n, 4))), dim3(NT), 0, c.s, c.ws, L, n, d, dV, dQ);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

}  // namespace got_tiled

// mdl_dispatch_plan product 12 (dispatch_plan.hip)
int plan_got_tiled(int64_t k, int n, int d, int64_t* o) {
    if (k < 1 || n < 1 || d < 1 || k > 0x7fffffff) return MDL_E_ARG;
    if (n > got_tiled::TMAXN || d > got_tiled::TMAXD) return MDL_E_UNSUPPORTED;
    const int64_t P = got_tiled::cdiv(n, got_tiled::RP), tn = got_tiled::cdiv(n, got_tiled::MT);
    o[MDL_PLAN_VARIANT] = got_tiled::RP;      // rows of a sweep panel
    o[MDL_PLAN_PERSIST] = 0;
    o[MDL_PLAN_SPLITS] = P;                   // row panels per case (sweep workgroups per case and branch)
    o[MDL_PLAN_TPS] = got_tiled::MT;          // output tile edge of the products
    o[MDL_PLAN_EMPTY] = tn * tn;              // product tiles per case of an n x n product
    o[MDL_PLAN_CHUNK] = got_tiled::CW;        // columns of a sweep chunk
    o[MDL_PLAN_EXTRA] = 2;                    // launches per IPOT iteration (row pass + column merge)
    return MDL_OK;
}
}  // namespace mdl

using namespace mdl;

static int tl_check(int k, int n, int d) {
    if (k < 0 || n < 0 || d < 1) return MDL_E_ARG;
    if (n > got_tiled::TMAXN || d > got_tiled::TMAXD) return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

static got_tiled::Ctx tl_ctx(void* ws, int k, int n, int d, void* stream) {
    got_tiled::Ctx c;
    c.ws = (float*)ws;
    c.L = got_tiled::layout(k, n, d);
    c.k = k;
    c.n = n;
    c.d = d;
    c.s = (hipStream_t)stream;
    return c;
}

extern "C" int64_t mdl_got_tiled_ws_bytes(int k, int n, int d) {
    const int rc = tl_check(k, n, d);
    if (rc) return rc;
    return got_tiled::layout(k, n, d).g_end * 4 + 64;
}

extern "C" int mdl_got_tiled_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in, int k, int n,
                                 int d, void* ws, void* stream) {
    const int rc = tl_check(k, n, d);
    if (rc) return rc;
    if (!out || !ws) return MDL_E_ARG;
    if (!host_aligned16(ws)) return MDL_E_ALIGN;
    if (k == 0 || n == 0) {   // empty token tensors may have no storage
        const hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(float), (hipStream_t)stream);
        return e == hipSuccess ? MDL_OK : (int)e;
    }
    if (!V || !Q) return MDL_E_ARG;
    const got_tiled::Ctx c = tl_ctx(ws, k, n, d, stream);
    const int r = got_tiled::launch_prep(c, minmax_out, minmax_in, V, Q);
    if (r) return r;
    return got_tiled::launch_main(c, out);
}

extern "C" int mdl_got_tiled_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int d, void* ws, void* stream) {
    const int rc = tl_check(k, n, d);
    if (rc) return rc;
    if (!V || !Q || !minmax_out || !ws) return MDL_E_ARG;
    if (!host_aligned16(ws)) return MDL_E_ALIGN;
    if (k == 0 || n == 0) return MDL_E_ARG;   // extrema of an empty batch are undefined
    return got_tiled::launch_prep(tl_ctx(ws, k, n, d, stream), minmax_out, nullptr, V, Q);
}

extern "C" int mdl_got_tiled_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int d, void* ws, void* stream) {
    const int rc = tl_check(k, n, d);
    if (rc) return rc;
    if (!d_out || !ws) return MDL_E_ARG;
    if (!host_aligned16(ws)) return MDL_E_ALIGN;
    if (k == 0 || n == 0) {
        if (d_minmax) {
            const hipError_t e = hipMemsetAsync(d_minmax, 0, 6 * sizeof(float), (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
        }
        return MDL_OK;
    }
    return got_tiled::launch_bwd_begin(tl_ctx(ws, k, n, d, stream), d_out, d_minmax);
}

extern "C" int mdl_got_tiled_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total, int k, int n,
                                        int d, void* ws, void* stream) {
    const int rc = tl_check(k, n, d);
    if (rc) return rc;
    if (!ws) return MDL_E_ARG;
    if (!host_aligned16(ws)) return MDL_E_ALIGN;
    if (k == 0 || n == 0) return MDL_OK;   // empty token tensors may have no storage
    if (!V || !Q || !dV || !dQ) return MDL_E_ARG;
    return got_tiled::launch_bwd_finish(tl_ctx(ws, k, n, d, stream), d_minmax_total, dV, dQ);
}

extern "C" int mdl_got_tiled_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int d, void* ws,
                                 void* stream) {
    const int rc = mdl_got_tiled_bwd_begin(d_out, nullptr, k, n, d, ws, stream);
    if (rc) return rc;
    return mdl_got_tiled_bwd_finish(V, Q, dV, dQ, nullptr, k, n, d, ws, stream);
}
