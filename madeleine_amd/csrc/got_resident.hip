// got_resident.hip -- G0-G3: Graph Optimal Transport token alignment (forward + hand-written reverse sweep), the RESIDENT size class:
// its kernels, its launch sequences and its row of the engine table (got_host.hpp).  The C ABI is in got.hip.
//
// Replaces, for k cases with n sub-sampled tokens each (n <= 512, d <= 128; the reference's one call site passes subsample=256):
//   GOT                                (reference madeleine/utils/loss.py:278-302)
//   cost_matrix_batch_torch            (:162-176)   C0[b,i,j] = 1 - <v^_i, q^_j>,  x^ = x / (|x| + 1e-12)
//   global-threshold ReLU              (:288-292)   thr = min + .1 (max - min) over the WHOLE batch tensor
//   IPOT_torch_batch_uniform           (:179-193)   T <- delta * (A.T) * sigma^T, 30 it, beta .5   (Wasserstein)
//   IPOT_distance / batch_trace        (:196-207)   wd_b = sum_ij C_ij T_ij
//   cos_batch_torch                    (:210-233)   thresholded intra costs Cs, Ct
//   GW_torch_batch / GW_distance       (:236-275)   5 x [ C_g = Cst - 2 Cs g Ct^T ; g = IPOT(C_g, beta .1, 20 it) ]
// The reference back-propagates through every unrolled IPOT iteration (no detach: loss.py:204, :245-248
// detaches only the RETURNED gamma).  The backward here replays the iterations in reverse from the stored
// per-iteration plans T_t and scaling vectors (delta_t, sigma_t) -- the same tensors autograd's tape holds.
//
// Organisation: one 1024-thread workgroup (NW = 16 waves x 128 VGPRs: enough waves to hide the L2 latency of the per-iteration
// matrix passes; a 512-thread build with 256 VGPRs per wave measured slower at every n, see launch_fwd_sweep) per case and branch; the Wasserstein and the Gromov-Wasserstein branch of a case are independent and run as separate
// workgroups of the same launch.  For n <= 128 a branch's whole chain is one kernel; for n > 128 it is one launch per
// phase (thresholds | C_gamma | IPOT sweep | ...), so the register allocation of the sweeps is not shared with the
// matrix products' accumulators.  Round 6: the IPOT sweeps of those per-phase classes run as TWO workgroups per case and
// branch (row halves exchanging column sums once per iteration) whenever the launch fits the device -- see Xch below.
//   * IPOT iterations keep the running plan in REGISTERS: wave w owns rows w, w+NW, ..., lane l owns columns
//     l, l+64, ... (<= 16 x 4 elements per lane at n = 256).  Per iteration one read of A = exp(-C/beta) (L2
//     resident, n*n*4 B <= 256 KiB) and one write of T_t into the history; a row reduction is a 64-lane shuffle
//     reduce, a column reduction a per-lane accumulator merged across the waves through LDS.
//   * the n^3 products of the GW branch (and the n*n*d cost / cost-gradient products) run on the fp32 matrix cores
//     (v_mfma_f32_32x32x2_f32): K-chunks of 16 staged through LDS, each wave owns a 64x64 output panel.
// Cs and Ct are bitwise symmetric here (the same accumulation chain computes <x_i,x_j> and <x_j,x_i>), so the
// reference's transposes (:233, :240-247) are identities.
#include <atomic>

#include "got_host.hpp"
#include "switches.hpp"

namespace mdl {
namespace got1024 {   // (the workgroup size; the kernel symbols carry it, and the profiles key on them)

constexpr int GOT_REGN = 256;           // register / one-panel classes (the hot path: trainer.py:44 sub-samples to <= 256 tokens)
constexpr int GOT_BIGN = 512;           // "big" class (256 < n <= 512): plans and plan gradients in the workspace, blocked matrix products
constexpr int GOT_MAXD = 128;
constexpr int WD_ITERS = 30;
constexpr int GW_OUTER = 5;
constexpr int GW_INNER = 20;
constexpr float WD_INV_BETA = 2.0f;    // beta 0.5 (loss.py:179 default, GOT passes only the iteration count :294)
constexpr float GW_INV_BETA = 10.0f;   // lamda = 1e-1 (loss.py:269)
constexpr float THR_BETA = 0.1f;       // loss.py:288, :226

constexpr int GNT = 1024;              // threads per workgroup
constexpr int GNW = GNT / 64;          // 16 waves
constexpr int MM_KC = 16;              // K-chunk of the in-block matrix product
constexpr int MM_LDK = 288;            // k-major LDS tile [kk][256]: +32 floats so the two half-waves (k, k+1) hit disjoint banks
constexpr int MM_LDI = 17;             // row-major LDS tile [i][kk]: odd stride, conflict-free over 32 rows
constexpr int MM_TILE = MM_KC * MM_LDK;  // 4608 floats >= 256 * MM_LDI

// exchange area of one case: [branch 2][half 2][parity 2][XCH_SLOTS] 8-byte granules
constexpr int XCH_SLOTS = 512;
constexpr int XCH_FLOATS = 2 * 2 * 2 * XCH_SLOTS * 2;

struct GotWs {
    // per-case regions (float offsets from the case base)
    int64_t per_case;
    int64_t oVh, oQh, orV, orQ, oC0, oCs0, oCt0, oC, oWT, oWd, oWs, oCs, oCt, ors, ort, oCg, oGT, oGd, oGs, oP1, oP2, oP3,
        ogT, ogA, ogCs, ogCt, oG, ogC0, oA, oA2, ogVh, ogQh, ogrs, ogrt, oX;
    // global regions (float offsets from ws base)
    int64_t g_ext, g_thr, g_gthr, g_wd, g_gwd, g_cnt, g_gen, g_cases;
};

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

__host__ __device__ inline GotWs got_layout(int k, int n, int d) {
    GotWs w;
    const int64_t nn = up4((int64_t)n * n), nd = up4((int64_t)n * d), nv = up4(n);
    int64_t o = 0;
    w.oVh = o; o += nd;
    w.oQh = o; o += nd;
    w.orV = o; o += nv;
    w.orQ = o; o += nv;
    w.oC0 = o; o += nn;
    w.oCs0 = o; o += nn;
    w.oCt0 = o; o += nn;
    w.oC = o; o += nn;                       // thresholded cross cost
    w.oWT = o; o += nn * WD_ITERS;           // T_1..T_30
    w.oWd = o; o += nv * WD_ITERS;           // delta_1..30
    w.oWs = o; o += nv * (WD_ITERS + 1);     // sigma_0..30
    w.oCs = o; o += nn;
    w.oCt = o; o += nn;
    w.ors = o; o += nv;
    w.ort = o; o += nv;
    w.oCg = o; o += nn * GW_OUTER;           // C_gamma of every outer iteration
    w.oGT = o; o += nn * GW_OUTER * GW_INNER;
    w.oGd = o; o += nv * GW_OUTER * GW_INNER;
    w.oGs = o; o += nv * GW_OUTER * (GW_INNER + 1);
    w.oP1 = o; o += nn;
    w.oP2 = o; o += nn;
    w.oP3 = o; o += nn;
    w.ogT = o; o += nn;
    w.ogA = o; o += nn;                      // GW branch: accumulated dL/dA of the IPOT being reversed
    w.ogCs = o; o += nn;
    w.ogCt = o; o += nn;
    w.oG = o; o += nn;
    w.ogC0 = o; o += nn;                     // d/d(raw cross cost), written by the WD sweep, read by cost_bwd
    w.oA = o; o += nn;                       // exp(-C/beta) of the IPOT in flight (GW branch)
    w.oA2 = o; o += nn * 3;                  // the same for the WD branch (runs concurrently) + its gT, gA
    w.ogVh = o; o += nd;                     // d/d(normalised tokens)
    w.ogQh = o; o += nd;
    w.ogrs = o; o += nv;                     // gradients of the Cst vectors rs, rt (GW reverse chain)
    w.ogrt = o; o += nv;
    w.oX = o; o += XCH_FLOATS;               // exchange granules of the split sweeps (two workgroups per case and branch), see Xch
    w.per_case = o;
    int64_t g = (int64_t)k * w.per_case;
    w.g_cases = 0;
    w.g_ext = g; g += up4((int64_t)k * 6);   // per-case (min,max) x3
    w.g_thr = g; g += 32;                    // [0..5] extrema used, [6..8] thresholds, [9..14] tie counts, [15..17] gthr
    w.g_gthr = g; g += up4((int64_t)k * 3);  // per-case threshold-gradient partials
    w.g_wd = g; g += up4(k);
    w.g_gwd = g; g += up4(k);
    w.g_cnt = g; g += up4((int64_t)k * 6);   // per-case counts of elements equal to each extremum
    w.g_gen = g; g += 4;                     // [0] pass generation (uint32: the tag prefix of the split sweeps' granules), [1] exchange time-outs
    w.g_cases = g;                           // total floats
    return w;
}

// ---------------------------------------------------------------------------------------------------------
// block-wide helpers (GNT threads = GNW waves).  LDS scratch is passed in by the kernels.
// ---------------------------------------------------------------------------------------------------------
struct Ctx {
    int n, tid, lane, wave, cstride;
    float* colbuf;  // LDS [GNW][cstride]   (aliases the matrix-product tiles: never live at the same time)
    float* xs;      // LDS [MM_TILE]
    float* ys;      // LDS [MM_TILE]
    float* red;     // LDS [GNW * 2]
};

constexpr int GOT_SMEM = 2 * MM_TILE + 2 * GNW;  // floats; colbuf (GNW * 256 <= 4096) lives inside xs
// big class: colbuf [GNW][512] = 8192 floats spans xs and ys (contiguous)
static_assert(GNW * GOT_BIGN <= 2 * MM_TILE, "column buffer of the big class must fit the two matrix-product tiles");

__device__ __forceinline__ Ctx make_ctx(int n, float* smem) {
    const int tid = threadIdx.x;
    return Ctx{n, tid, tid & 63, tid >> 6, n > GOT_REGN ? GOT_BIGN : GOT_REGN, smem, smem, smem + MM_TILE, smem + 2 * MM_TILE};
}

// merge per-lane column accumulators of the GNW waves: f(j, sum_w cacc_w[j])
// The problem of this workgroup in a batched launch of `mult` * k_p blocks per problem (blocks of problem 0 first); bid becomes the block
// index within the problem.  Selected by compile-time indices: the batch stays in the kernel-argument segment.
__device__ __forceinline__ GotProb got_prob(const GotBatch& B, int pi) {
    GotProb P = B.p[0];
#pragma unroll
    for (int q = 1; q < GOT_MAXP; ++q)
        if (pi == q) P = B.p[q];
    return P;
}
__device__ __forceinline__ GotProb got_pick(const GotBatch& B, int mult, int& bid) {
    int pi = 0;
#pragma unroll
    for (int q = 0; q < GOT_MAXP - 1; ++q) {
        const int g = B.p[q].k * mult;
        if (pi == q && q < B.np - 1 && bid >= g) {
            bid -= g;
            pi = q + 1;
        }
    }
    return got_prob(B, pi);
}

template <int QC, class F>
__device__ __forceinline__ void col_finish(const Ctx& c, const float (&cacc)[QC], F&& f) {
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        const int j = c.lane + 64 * q;
        if (j < c.n) c.colbuf[c.wave * c.cstride + j] = cacc[q];
    }
    __syncthreads();
    if (c.tid < c.n) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < GNW; ++w) s += c.colbuf[w * c.cstride + c.tid];
        f(c.tid, s);
    }
    __syncthreads();
}

// the same for TWO accumulator sets in one barrier pair: f(j, sum_w a_w[j], sum_w b_w[j]).  The second set sits behind the first in the
// column buffer (2 x GNW x 256 floats <= the two matrix-product tiles the buffer aliases; not for the big class).
template <int QC, class F>
__device__ __forceinline__ void col_finish2(const Ctx& c, const float (&ca)[QC], const float (&cb)[QC], F&& f) {
    static_assert(2 * GNW * GOT_REGN <= 2 * MM_TILE, "two column buffers must fit the matrix-product tiles");
    // compile-time row stride: every access below is one base register + an immediate offset (with the runtime stride of Ctx the 2 x GNW
    // read addresses of the merge were hoisted out of the sweep's iteration loop and spilled)
    constexpr int CS = GOT_REGN;
    float* first = c.colbuf + c.wave * CS + c.lane;
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        if (c.lane + 64 * q < c.n) {
            first[64 * q] = ca[q];
            first[GNW * CS + 64 * q] = cb[q];
        }
    }
    __syncthreads();
    if (c.tid < c.n) {
        const float* col = c.colbuf + c.tid;
        float s = 0.f, z = 0.f;
#pragma unroll
        for (int w = 0; w < GNW; ++w) {
            s += col[w * CS];
            z += col[(GNW + w) * CS];
        }
        f(c.tid, s, z);
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// Split sweeps: TWO workgroups per case and branch (round 6).  A data-parallel rank's GOT launch holds k <= 128 cases, and four of the
// five Gromov-Wasserstein sweeps of a pass run alone -- k workgroups on 256 compute units; at n = 256 a lane of the one-workgroup sweep
// also holds 64 plan / accumulator elements, which spill.  Half h of a case owns the rows i = wave + GNW (2 r + h): 32 elements per lane
// (everything in registers, the forward keeps A = exp(-C / beta) there as well and never re-reads it); the only coupling between the
// halves is the COLUMN sums of an iteration (sigma_t in the forward; gsig / colsum(Y) in the reverse sweep), exchanged once per iteration:
// thread j publishes its partial as ONE 8-byte granule {float, tag} with a device-scope (sc1, write-through) store and polls the
// partner's granule with device-scope loads until the tag matches (MI355X_MICROARCH.md, hand-off price list: handoff-1to1).  Both halves
// add the two partials in the same order (half 0 + half 1), so the replicated column vectors agree bit for bit.
//   * tag = (generation << 10) | sequence number: the generation (ws[g_gen], bumped by the first kernel of every pass) keeps granules of
//     an earlier pass on the same workspace from ever matching; two parity slots, because a half may publish exchange e + 1 while its
//     partner still reads e (it cannot reach e + 2: that needs the partner's e + 1, published after the partner finished reading e).
//   * progress: a split launch holds at most as many workgroups as the device has compute units (checked on the host), each needs a
//     whole unit (1024 threads at 128 VGPRs): whenever a half waits for a partner that is not resident yet, a unit is free or held by a
//     workgroup that can finish -- no dispatch-order assumption.  Every poll loop is bounded all the same (XCH_LIMIT, then
//     ws[g_gen + 1] is raised and the pass's numbers are void: got_sum_kernel returns NaN distances and got_cost_bwd_kernel NaN
//     gradients -- e.g. two training processes sharing the GPU, each assuming it owns every compute unit; MADELEINE_GOT_NOSPLIT=1 is
//     the setting for that).
// ---------------------------------------------------------------------------------------------------------
constexpr int XCH_LIMIT = 1 << 20;
struct Xch {
    unsigned long long* mine;         // [2 parity][XCH_SLOTS]
    const unsigned long long* peer;
    float* err;                       // ws + g_gen + 1
    uint32_t tag0;                    // (generation << 10) | first sequence number of this launch
    int half;
    bool dead;                        // a poll of this thread timed out: stop waiting for the rest of the kernel
};
__device__ __forceinline__ Xch make_xch(float* ws, const GotWs& L, float* base, int branch, int half, int seq0) {
    unsigned long long* area = reinterpret_cast<unsigned long long*>(base + L.oX) + (int64_t)branch * 4 * XCH_SLOTS;
    const uint32_t gen = __float_as_uint(ws[L.g_gen]);
    return Xch{area + half * 2 * XCH_SLOTS, area + (1 - half) * 2 * XCH_SLOTS, ws + L.g_gen + 1, (gen << 10) | (uint32_t)seq0, half, false};
}
// this thread's partial `v` of exchange e, slot `slot` -> (half 0's partial) + (half 1's partial)
__device__ __forceinline__ float xch_add(Xch& x, int e, int slot, float v) {
    const uint32_t tag = x.tag0 + (uint32_t)e;
    const int at = (e & 1) * XCH_SLOTS + slot;
    __hip_atomic_store(x.mine + at, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long g = 0;
    if (!x.dead) {
        int spins = 0;
        for (;;) {
            g = __hip_atomic_load(x.peer + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)(g >> 32) == tag) break;
            if (++spins >= XCH_LIMIT) {
                x.dead = true;
                *x.err = 1.f;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    const float o = __uint_as_float((uint32_t)g);
    return x.half == 0 ? v + o : o + v;
}
// col_finish / col_finish2 of a split sweep: the workgroup's column partial, then the partner's (exchange e)
template <int QC, class F>
__device__ __forceinline__ void col_finish_x(const Ctx& c, Xch& x, int e, const float (&cacc)[QC], F&& f) {
    constexpr int CS = GOT_REGN;
    float* first = c.colbuf + c.wave * CS + c.lane;
#pragma unroll
    for (int q = 0; q < QC; ++q)
        if (c.lane + 64 * q < c.n) first[64 * q] = cacc[q];
    __syncthreads();
    if (c.tid < c.n) {
        const float* col = c.colbuf + c.tid;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < GNW; ++w) s += col[w * CS];
        f(c.tid, xch_add(x, e, c.tid, s));
    }
    __syncthreads();
}
template <int QC, class F>
__device__ __forceinline__ void col_finish2_x(const Ctx& c, Xch& x, int e, const float (&ca)[QC], const float (&cb)[QC], F&& f) {
    constexpr int CS = GOT_REGN;
    float* first = c.colbuf + c.wave * CS + c.lane;
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        if (c.lane + 64 * q < c.n) {
            first[64 * q] = ca[q];
            first[GNW * CS + 64 * q] = cb[q];
        }
    }
    __syncthreads();
    if (c.tid < c.n) {
        const float* col = c.colbuf + c.tid;
        float s = 0.f, z = 0.f;
#pragma unroll
        for (int w = 0; w < GNW; ++w) {
            s += col[w * CS];
            z += col[(GNW + w) * CS];
        }
        // both granules are in flight before the first poll
        const uint32_t tag = x.tag0 + (uint32_t)e;
        const int at = (e & 1) * XCH_SLOTS + c.tid;
        __hip_atomic_store(x.mine + at + GOT_REGN, ((unsigned long long)tag << 32) | __float_as_uint(z), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        const float st = xch_add(x, e, c.tid, s);
        unsigned long long g = 0;
        if (!x.dead) {
            int spins = 0;
            for (;;) {
                g = __hip_atomic_load(x.peer + at + GOT_REGN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((uint32_t)(g >> 32) == tag) break;
                if (++spins >= XCH_LIMIT) {
                    x.dead = true;
                    *x.err = 1.f;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        const float oz = __uint_as_float((uint32_t)g);
        f(c.tid, st, x.half == 0 ? z + oz : oz + z);
    }
    __syncthreads();
}
// block-wide sum over the workgroup, then over the two halves (exchange e, slot 0); the total is valid on thread 0
__device__ __forceinline__ float block_sum_x(const Ctx& c, Xch& x, int e, float v);

// block-wide sum of one value per thread (result valid on thread 0 after the call)
__device__ __forceinline__ float block_sum(const Ctx& c, float v, int slot = 0) {
    v = wave_sum(v);
    if (c.lane == 0) c.red[slot * GNW + c.wave] = v;
    __syncthreads();
    float s = 0.f;
    if (c.tid == 0)
        for (int w = 0; w < GNW; ++w) s += c.red[slot * GNW + w];
    return s;
}
__device__ __forceinline__ float block_sum_x(const Ctx& c, Xch& x, int e, float v) {
    float s = block_sum(c, v);
    if (c.tid == 0) s = xch_add(x, e, 0, s);
    return s;
}

// out(i,j) = sum_k Xop(i,k) Yop(k,j), i < M, j < N (both <= 256), k < K, on the fp32 matrix cores.
//   Xop(i,k) = TA ? X[k*ldx + i] : X[i*ldx + k]        Yop(k,j) = TB ? Y[j*ldy + k] : Y[k*ldy + j]
// K is walked in chunks of 16 staged through LDS (next chunk prefetched into registers while the current one is
// multiplied); wave w owns the 64x64 output panel (w/4, w%4).  epi(i, j, value) is called once per element.
// WIDE = false: wave w owns the 64 x 64 panel of a 4 x 4 grid -- 9 of 16 waves for M, N in (128, 192], and none on
// the SIMD that holds waves 3, 7, 11, 15.  WIDE = true (M, N <= 192): 12 waves own 32 x 96 strips (6 x 2 grid), three per
// SIMD: 9 instead of 12 tile-products on the busiest SIMD.  Every output element sees the same MFMA sequence over k in both layouts
// (same bits).
// LAY = 2 (round 6): M <= 128, N <= 256 -- a 4 x 4 grid of 32 x 64 panels, every wave busy on HALF the rows of a case (the
// forward C_gamma products split over two workgroups, gw_cgamma_half); LAY 0 / 1 = the layouts above (WIDE = LAY == 1).
template <bool TA, bool TB, int LAY, class Epi>
__device__ __forceinline__ void mm_impl(const Ctx& c, int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ Y,
                   int ldy, Epi&& epi) {
    constexpr bool WIDE = LAY == 1, HALF = LAY == 2;
    constexpr int UR = (WIDE || HALF) ? 1 : 2, VC = WIDE ? 3 : 2;   // 32-row / 32-column blocks per wave
    float* xs = c.xs;
    float* ys = c.ys;
    // opaque thread id per call: the address arithmetic of every inlined product would otherwise be hoisted to the
    // kernel entry and spilled
    int tid_ = c.tid;
    asm volatile("" : "+v"(tid_));
    const int tid = tid_, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int bi0 = WIDE ? (wave >> 1) * 32 : HALF ? (wave >> 2) * 32 : (wave >> 2) * 64;
    const int bj0 = WIDE ? (wave & 1) * 96 : (wave & 3) * 64;
    const bool active = bi0 < M && bj0 < N && (!WIDE || wave < 12);
    f32x16 acc[UR][VC];
#pragma unroll
    for (int a = 0; a < UR; ++a)
#pragma unroll
        for (int b = 0; b < VC; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    constexpr int NP = 256 * MM_KC / GNT;   // elements per thread and operand per chunk
    float px[NP], py[NP];
    auto gload = [&](int k0) {
        // opaque copies: keeps the compiler from hoisting the 2*NP loop-invariant bound masks of every inlined product
        // out of all loops (they would pin ~100 SGPR pairs across the whole kernel)
        int Mv = M, Nv = N, Kv = K;
        asm volatile("" : "+v"(Mv), "+v"(Nv), "+v"(Kv));
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int idx = tid + GNT * p;
            {
                const int kk = TA ? (idx >> 8) : (idx & 15), i = TA ? (idx & 255) : (idx >> 4);
                const bool ok = i < Mv && k0 + kk < Kv;
                px[p] = ok ? (TA ? X[(k0 + kk) * ldx + i] : X[i * ldx + k0 + kk]) : 0.f;
            }
            {
                const int kk = TB ? (idx & 15) : (idx >> 8), j = TB ? (idx >> 4) : (idx & 255);
                const bool ok = j < Nv && k0 + kk < Kv;
                py[p] = ok ? (TB ? Y[j * ldy + k0 + kk] : Y[(k0 + kk) * ldy + j]) : 0.f;
            }
        }
    };
    gload(0);
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += MM_KC) {
        __syncthreads();  // everyone is done reading the previous chunk (and colbuf users before the first)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int idx = tid + GNT * p;
            if (TA) xs[(idx >> 8) * MM_LDK + (idx & 255)] = px[p];
            else xs[(idx >> 4) * MM_LDI + (idx & 15)] = px[p];
            if (TB) ys[(idx >> 4) * MM_LDI + (idx & 15)] = py[p];
            else ys[(idx >> 8) * MM_LDK + (idx & 255)] = py[p];
        }
        __syncthreads();
        if (k0 + MM_KC < K) gload(k0 + MM_KC);
        if (active) {
#pragma unroll
            for (int kk = 0; kk < MM_KC; kk += 2) {
                const int kq = kk + hi;
                float a[UR], b[VC];
#pragma unroll
                for (int u = 0; u < UR; ++u) a[u] = TA ? xs[kq * MM_LDK + bi0 + 32 * u + l31] : xs[(bi0 + 32 * u + l31) * MM_LDI + kq];
#pragma unroll
                for (int v = 0; v < VC; ++v) b[v] = TB ? ys[(bj0 + 32 * v + l31) * MM_LDI + kq] : ys[kq * MM_LDK + bj0 + 32 * v + l31];
#pragma unroll
                for (int u = 0; u < UR; ++u)
#pragma unroll
                    for (int v = 0; v < VC; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[v], acc[u][v], 0, 0, 0);
            }
        }
    }
    if (active) {
#pragma unroll
        for (int u = 0; u < UR; ++u)
#pragma unroll
            for (int v = 0; v < VC; ++v) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = bi0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hi, j = bj0 + 32 * v + l31;
                    if (i < M && j < N) epi(i, j, acc[u][v][r]);
                }
                __builtin_amdgcn_sched_barrier(0);  // keep read-modify-write epilogues from hoisting 128 loads at once
            }
    }
    __syncthreads();
}

// WOK: the caller is one of the per-phase kernels (n > 128 classes), where the 12-wave layout pays; the fused n <= 128 kernels keep ONE
// inlined copy of the product (a second one costs them 260 more spilled registers).
template <bool TA, bool TB, bool WOK = false, class Epi>
__device__ __forceinline__ void mm(const Ctx& c, int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ Y,
                                   int ldy, Epi&& epi) {
#ifndef MDL_GOT_NO_WIDE_MM   // (A/B switch of tools/ab)
    if constexpr (WOK) {
        if (M <= 192 && N <= 192 && (M > 128 || N > 128)) {
            mm_impl<TA, TB, 1>(c, M, N, K, X, ldx, Y, ldy, epi);
            return;
        }
    }
#endif
    mm_impl<TA, TB, 0>(c, M, N, K, X, ldx, Y, ldy, epi);
}

// The same product for M, N up to GOT_BIGN: 256 x 256 output blocks, one mm() each (BIG = false: exactly mm()).
template <bool BIG, bool TA, bool TB, bool WOK = false, class Epi>
__device__ __forceinline__ void mmx(const Ctx& c, int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ Y,
                                    int ldy, Epi&& epi) {
    if constexpr (!BIG) {
        mm<TA, TB, WOK>(c, M, N, K, X, ldx, Y, ldy, epi);
    } else {
#pragma unroll 1
        for (int bi = 0; bi < M; bi += 256)
#pragma unroll 1
            for (int bj = 0; bj < N; bj += 256)
                mm<TA, TB>(c, M - bi < 256 ? M - bi : 256, N - bj < 256 ? N - bj : 256, K, TA ? X + bi : X + bi * ldx, ldx,
                           TB ? Y + bj * ldy : Y + bj, ldy, [&](int i, int j, float v) { epi(i + bi, j + bj, v); });
    }
}

// ---------------------------------------------------------------------------------------------------------
// IPOT forward (loss.py:179-193) on a materialised cost matrix Cm; stores T_1..T_iters, delta_1.., sigma_0..
// The plan lives in registers: T[r][q] = element (wave + GNW r, lane + 64 q).
// ---------------------------------------------------------------------------------------------------------
template <int RPW, int QC>
__device__ __forceinline__ void ipot_forward_t(const Ctx& c, const float* __restrict__ Cm, float inv_beta, int iters, float* __restrict__ Am,
                               float* __restrict__ Thist, float* __restrict__ dhist, float* __restrict__ shist, float* sig, float* del) {
    int tid_ = c.tid;
    asm volatile("" : "+v"(tid_));   // opaque per call (see mm)
    const int tid = tid_, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nn = (int)up4((int64_t)c.n * c.n);
    const int nv = (int)up4(c.n);
    const float fn = (float)c.n;
    for (int e = tid; e < c.n * c.n; e += GNT) Am[e] = expf(-Cm[e] * inv_beta);
    for (int j = tid; j < c.n; j += GNT) {
        sig[j] = 1.f / fn;
        shist[j] = 1.f / fn;
    }
    __syncthreads();
    float T[RPW][QC];
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int q = 0; q < QC; ++q) T[r][q] = 1.f;
    constexpr int RG = RPW < 4 ? RPW : 4;
#pragma unroll 1
    for (int t = 1; t <= iters; ++t) {
        // Bounds: rows are wave-uniform (scalar compares), columns need QC lane masks.  Loads are UNCONDITIONAL on clamped
        // indices and zeroed afterwards -- per-element predicates (RPW*QC exec masks) were what spilled.  n is re-derived
        // opaquely every iteration so that none of this is hoisted out of the loop.
        int n_ = c.n;
        asm volatile("" : "+v"(n_));
        const int n = __builtin_amdgcn_readfirstlane(n_);
        float* __restrict__ Tn = Thist + (t - 1) * nn;
        float cacc[QC], sq[QC];
        int jc[QC];
        bool jok[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            const int j = lane + 64 * q;
            jok[q] = j < n;
            jc[q] = jok[q] ? j : n - 1;
            cacc[q] = 0.f;
            sq[q] = jok[q] ? sig[j] : 0.f;
        }
        // Q = A . T_{t-1};  delta_t,i = 1 / (n sum_j Q_ij sigma_{t-1,j});  column partials a_j = sum_i Q_ij delta_t,i
#pragma unroll
        for (int r0 = 0; r0 < RPW; r0 += RG) {
            float a[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = wave + GNW * (r0 + g), ic = i < n ? i : n - 1;
                const float* __restrict__ Arow = Am + ic * n;   // scalar row base + 32-bit lane offset (saddr addressing)
#pragma unroll
                for (int q = 0; q < QC; ++q) a[g][q] = Arow[jc[q]];
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int r = r0 + g, i = wave + GNW * r;
                const bool iok = i < n;
                float rs = 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float Qv = (iok && jok[q]) ? a[g][q] * T[r][q] : 0.f;
                    T[r][q] = Qv;
                    rs += Qv * sq[q];
                }
                rs = wave_sum(rs);
                const float di = iok ? 1.f / (fn * rs) : 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) cacc[q] += T[r][q] * di;
                if (lane == 0 && iok) {
                    dhist[(t - 1) * nv + i] = di;
                    del[i] = di;
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the scheduler from hoisting every group's loads to the top (spills)
        }
        col_finish<QC>(c, cacc, [&](int j, float a) {
            const float s = 1.f / (fn * a);
            sig[j] = s;
            shist[t * nv + j] = s;
        });
#pragma unroll
        for (int q = 0; q < QC; ++q) sq[q] = jok[q] ? sig[lane + 64 * q] : 0.f;
        // T_t = delta_i Q_ij sigma_j
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = wave + GNW * r;
            if (i < n) {  // wave-uniform
                const float di = del[i];
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float Tv = di * T[r][q] * sq[q];
                    T[r][q] = Tv;
                    if (jok[q]) (Tn + i * n)[jc[q]] = Tv;
                }
            }
        }
    }
    __syncthreads();
}


// The same iterations on HALF of the rows (split sweeps, see Xch): rows i = wave + GNW (2 r + half), RPW of them per wave.  The plan AND
// A = exp(-C / beta) live in registers (2 x RPW x QC = 64 at n = 256), so an iteration reads nothing but sigma and writes its half of
// T_t; delta_t,i stays in a register of the wave that owns row i.  Same arithmetic per element as ipot_forward_t; the column sums are
// associated differently (RPW rows per wave, 16 waves, two halves), so the last bits differ from the one-workgroup sweep.
template <int RPW, int QC>
__device__ __forceinline__ void ipot_forward_split(const Ctx& c, Xch& x, const float* __restrict__ Cm, float inv_beta, int iters,
                                                   float* __restrict__ Thist, float* __restrict__ dhist, float* __restrict__ shist, float* sig) {
    int tid_ = c.tid;
    asm volatile("" : "+v"(tid_));   // opaque per call (see mm)
    const int tid = tid_, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = __builtin_amdgcn_readfirstlane(c.n);
    const int nn = (int)up4((int64_t)n * n);
    const int nv = (int)up4(n);
    const float fn = (float)n;
    for (int j = tid; j < n; j += GNT) {
        sig[j] = 1.f / fn;
        shist[j] = 1.f / fn;            // (both halves write the same value)
    }
    float T[RPW][QC], A[RPW][QC], dr[RPW];
    int jc[QC];
    bool jok[QC];
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        const int j = lane + 64 * q;
        jok[q] = j < n;
        jc[q] = jok[q] ? j : n - 1;
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int i = wave + GNW * (2 * r + x.half);
        const bool iok = i < n;
        const float* __restrict__ Crow = Cm + (iok ? i : n - 1) * n;
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            const float a = expf(-Crow[jc[q]] * inv_beta);
            A[r][q] = (iok && jok[q]) ? a : 0.f;     // zero outside the matrix: Q vanishes there without per-element predicates
            T[r][q] = 1.f;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 1; t <= iters; ++t) {
        float* __restrict__ Tn = Thist + (t - 1) * nn;
        float cacc[QC], sq[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            cacc[q] = 0.f;
            sq[q] = jok[q] ? sig[jc[q]] : 0.f;
        }
        // Q = A . T_{t-1};  delta_t,i = 1 / (n sum_j Q_ij sigma_{t-1,j});  column partials a_j = sum_i Q_ij delta_t,i
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = wave + GNW * (2 * r + x.half);
            const bool iok = i < n;   // wave-uniform
            float rs = 0.f;
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                const float Qv = A[r][q] * T[r][q];
                T[r][q] = Qv;
                rs += Qv * sq[q];
            }
            rs = wave_sum(rs);
            const float di = iok ? 1.f / (fn * rs) : 0.f;
            dr[r] = di;
#pragma unroll
            for (int q = 0; q < QC; ++q) cacc[q] += T[r][q] * di;
            if (lane == 0 && iok) dhist[(t - 1) * nv + i] = di;
        }
        col_finish_x<QC>(c, x, t - 1, cacc, [&](int j, float a) {
            const float s = 1.f / (fn * a);
            sig[j] = s;
            shist[t * nv + j] = s;
        });
#pragma unroll
        for (int q = 0; q < QC; ++q) sq[q] = jok[q] ? sig[jc[q]] : 0.f;
        // T_t = delta_i Q_ij sigma_j
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = wave + GNW * (2 * r + x.half);
            if (i < n) {  // wave-uniform
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float Tv = dr[r] * T[r][q] * sq[q];
                    T[r][q] = Tv;
                    if (jok[q]) (Tn + i * n)[jc[q]] = Tv;
                }
            }
        }
    }
    __syncthreads();
}

// The same iterations for n > 256: the running plan is the history entry itself (T_{t-1} is re-read from Thist, T_t written to it)
// -- 2 x 8 plan registers per row group instead of 32 x 8 per wave.  Two row passes per iteration: Q = A . T_{t-1} is recomputed in
// the second one (delta and the new sigma are known only after the first).
template <int QC>
__device__ __forceinline__ void ipot_forward_mem(const Ctx& c, const float* __restrict__ Cm, float inv_beta, int iters, float* __restrict__ Am,
                                                 float* __restrict__ Thist, float* __restrict__ dhist, float* __restrict__ shist, float* sig,
                                                 float* del) {
    const int tid = c.tid, lane = c.lane, wave = __builtin_amdgcn_readfirstlane(c.wave);
    const int n = c.n;
    const int nn = (int)up4((int64_t)n * n);
    const int nv = (int)up4(n);
    const float fn = (float)n;
    for (int e = tid; e < n * n; e += GNT) Am[e] = expf(-Cm[e] * inv_beta);
    for (int j = tid; j < n; j += GNT) {
        sig[j] = 1.f / fn;
        shist[j] = 1.f / fn;
    }
    __syncthreads();
    constexpr int RG = 2;
    int jc[QC];
    bool jok[QC];
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        const int j = lane + 64 * q;
        jok[q] = j < n;
        jc[q] = jok[q] ? j : n - 1;
    }
#pragma unroll 1
    for (int t = 1; t <= iters; ++t) {
        const float* __restrict__ Tp = (t >= 2) ? Thist + (t - 2) * nn : nullptr;   // T_0 = ones
        float* __restrict__ Tn = Thist + (t - 1) * nn;
        float cacc[QC], sq[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            cacc[q] = 0.f;
            sq[q] = jok[q] ? sig[jc[q]] : 0.f;
        }
        // delta_t,i = 1 / (n sum_j Q_ij sigma_{t-1,j});  column partials a_j = sum_i Q_ij delta_t,i
#pragma unroll 1
        for (int i0 = wave; i0 < n; i0 += GNW * RG) {
            float a[RG][QC], tp[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g, ic = i < n ? i : n - 1;
                const float* __restrict__ Arow = Am + ic * n;
                const float* __restrict__ Trow = Tp ? Tp + ic * n : nullptr;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    a[g][q] = Arow[jc[q]];
                    tp[g][q] = Trow ? Trow[jc[q]] : 1.f;
                }
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g;
                const bool iok = i < n;   // wave-uniform
                float rs = 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float Qv = (iok && jok[q]) ? a[g][q] * tp[g][q] : 0.f;
                    a[g][q] = Qv;
                    rs += Qv * sq[q];
                }
                rs = wave_sum(rs);
                const float di = iok ? 1.f / (fn * rs) : 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) cacc[q] += a[g][q] * di;
                if (lane == 0 && iok) {
                    dhist[(t - 1) * nv + i] = di;
                    del[i] = di;
                }
            }
        }
        col_finish<QC>(c, cacc, [&](int j, float a) {
            const float s = 1.f / (fn * a);
            sig[j] = s;
            shist[t * nv + j] = s;
        });
#pragma unroll
        for (int q = 0; q < QC; ++q) sq[q] = jok[q] ? sig[jc[q]] : 0.f;
        // T_t = delta_i Q_ij sigma_j
#pragma unroll 1
        for (int i0 = wave; i0 < n; i0 += GNW * RG) {
            float a[RG][QC], tp[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g, ic = i < n ? i : n - 1;
                const float* __restrict__ Arow = Am + ic * n;
                const float* __restrict__ Trow = Tp ? Tp + ic * n : nullptr;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    a[g][q] = Arow[jc[q]];
                    tp[g][q] = Trow ? Trow[jc[q]] : 1.f;
                }
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g;
                if (i < n) {   // wave-uniform
                    const float di = del[i];
#pragma unroll
                    for (int q = 0; q < QC; ++q)
                        if (jok[q]) (Tn + i * n)[jc[q]] = di * (a[g][q] * tp[g][q]) * sq[q];
                }
            }
        }
    }   // (a lane re-reads exactly the T_t elements it wrote; sig / del are ordered by the barriers of col_finish)
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// IPOT reverse sweep (round 5: ONE pass over one matrix per iteration, no matrix-sized state besides the accumulator H in registers).
// In: gT_in (n x n, gradient wrt the returned plan T_iters, times gscale), out: gC_out = dL/dC (n x n).
//
// Autograd's tape through  Q_t = A . T_{t-1};  delta_t = 1 / (n Q_t sigma_{t-1});  sigma_t = 1 / (n Q_t^T delta_t);  T_t = delta_t Q_t sigma_t
// gives per reversed iteration (dl = delta_t, sg = sigma_t, so = sigma_{t-1}, '.' elementwise):
//     gq = gT_t . Q_t ;  gdel_i = sum_j gq_ij sg_j ;  u_j = sum_i gq_ij dl_i ;  ga_j = -n sg_j^2 (gsig_j + u_j)
//     gr_i = -n dl_i^2 (gdel_i + sum_j Q_ij ga_j) ;  gsig_j <- sum_i Q_ij gr_i
//     gQ = gT_t dl sg + ga dl + gr so ;  gA += gQ . T_{t-1} ;  gT_{t-1} = gQ . A ;        dL/dC = -(1/beta) gA . A
// (rounds 1-4 ran exactly that: two passes over A, T_{t-1}, gT, gA per iteration = 9 matrix accesses, 4 + an LDS-resident gT for
// n <= 192).  With Y_t := gQ_t . Q_t the matrices drop out of the recurrence.  Since Q_{t+1} = A . T_t = A . (dl Q_t sg):
//     gq_t = gQ_{t+1} . A . Q_t = Y_{t+1} / (dl_i sg_j)   =>   gdel_i = rowsum(Y_{t+1})_i / dl_i ,   u_j = colsum(Y_{t+1})_j / sg_j
//     Y_t = Y_{t+1} + W_t ,   W_t = Q_t . (dl ga^T + gr so^T) ;   Y_{iters+1} = gT_in . T_iters
//     dL/dC = -(1/beta) sum_t gQ_t . Q_t = -(1/beta) H ,   H = iters Y_{iters+1} + sum_t t W_t
// so an iteration needs Q_t once (row sums against ga and so, then W_t), and only the row / column SUMS of Y travel between iterations
// (rowsum(W_t)_i = dl_i (Q_t ga)_i + gr_i (Q_t so)_i).  Q_t is rebuilt from the stored plan: Q_t = T_t / (dl_i sg_j) -- ONE matrix
// read per iteration (the forward writes one), no A, no gT / gA workspace traffic.  tools/got_reverse_check.py: the derivation against
// fp64 autograd (1e-15), and in fp32 arithmetic the same error as the two-pass sweep (2.8e-7 at n = 96).
// H: RPW x QC accumulators per lane (64 at n = 256): rows r < RPW - HLR in registers, the last HLR rows in lane-private LDS slots
// Hl[(r - (RPW - HLR)) * QC + q][tid] (conflict-free b32 accesses; 64 accumulators + the row operands do not fit the 128-VGPR budget of
// a 1024-thread workgroup: without the LDS rows the n = 256 class kept 46 of them in scratch).  LDS vectors: ga, Rv = rowsum(Y),
// Cv = colsum(Y).
// ---------------------------------------------------------------------------------------------------------
// load through a wave-uniform base + a 32-bit BYTE offset per lane: the `global_load_dword v, v_off, s[base:base+1]` form -- one offset
// register per column group instead of a 64-bit address pair per load
__device__ __forceinline__ float ld_soff(const float* __restrict__ sbase, uint32_t byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(sbase) + byte_off);
}
// NH = 2: the split sweep (see Xch) -- this workgroup owns the rows i = wave + GNW (2 r + x->half), RPW of them per wave, and merges its
// column sums with the partner's (exchange 0: the seed, exchange t' = iters + 1 - t: reversed iteration t).
template <int RPW, int QC, int HLR = 0, int NH = 1>
__device__ __forceinline__ void ipot_backward_h(const Ctx& c, float inv_beta, int iters, const float* __restrict__ Thist,
                                                const float* __restrict__ dhist, const float* __restrict__ shist,
                                                const float* __restrict__ gT_in, float gscale, float* __restrict__ gC_out, float* ga,
                                                float* Rv, float* Cv, float* Hl = nullptr, Xch* x = nullptr) {
    static_assert(NH == 1 || HLR == 0, "the split sweep keeps its whole accumulator block in registers");
    const int rhalf = NH == 2 ? x->half : 0;
    int tid_ = c.tid;
    asm volatile("" : "+v"(tid_));   // opaque per call (see mm)
    const int tid = tid_, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nn = (int)up4((int64_t)c.n * c.n);
    const int nv = (int)up4(c.n);
    const float fn = (float)c.n;
    constexpr int RREG = RPW - HLR;       // rows of H in registers
    float H[RREG > 0 ? RREG : 1][QC];
    float* __restrict__ hl = Hl + tid;    // this lane's LDS slots: hl[slot * GNT]
#ifndef MDL_GOT_H_RG
#define MDL_GOT_H_RG 4
#endif
#ifndef MDL_GOT_HLR3
#define MDL_GOT_HLR3 2
#endif
#ifndef MDL_GOT_HLR4
#define MDL_GOT_HLR4 7
#endif
    // rows of loads in flight per wave: a divisor of RPW (6 rows per wave in the split sweep of the n <= 192 class: 3)
    constexpr int RG = RPW % MDL_GOT_H_RG == 0 ? MDL_GOT_H_RG : (RPW < MDL_GOT_H_RG ? RPW : (RPW % 3 == 0 ? 3 : (RPW % 2 == 0 ? 2 : 1)));
    static_assert(RPW % RG == 0, "row groups must tile the wave's rows");
    {
        // Y_{iters+1} = gscale gT_in . T_iters : H = iters Y, row sums -> Rv, column sums -> Cv, first ga (gsig = 0)
        const int n = __builtin_amdgcn_readfirstlane(c.n);
        const float* __restrict__ Tl = Thist + (iters - 1) * nn;
        float cacc[QC];
        uint32_t jc[QC];   // unsigned: scalar row base + 32-bit lane offset (saddr addressing, no 64-bit address pairs)
        bool jok[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            const int j = lane + 64 * q;
            jok[q] = j < n;
            jc[q] = (uint32_t)(jok[q] ? j : n - 1) << 2;   // BYTE offset
            cacc[q] = 0.f;
        }
#pragma unroll
        for (int r0 = 0; r0 < RPW; r0 += RG) {
            float gv[RG][QC], tl[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = wave + GNW * (NH * (r0 + g) + rhalf), ic = i < n ? i : n - 1;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    gv[g][q] = ld_soff(gT_in + ic * n, jc[q]);
                    tl[g][q] = ld_soff(Tl + ic * n, jc[q]);
                }
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int r = r0 + g, i = wave + GNW * (NH * r + rhalf);
                const bool iok = i < n;
                float rs = 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float y = (iok && jok[q]) ? gscale * gv[g][q] * tl[g][q] : 0.f;
                    if (r < RREG) H[r < RREG ? r : 0][q] = (float)iters * y;
                    else hl[((r - RREG) * QC + q) * GNT] = (float)iters * y;
                    rs += y;
                    cacc[q] += y;
                }
                rs = wave_sum_dpp(rs);
                if (lane == 0 && iok) Rv[i] = rs;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const float* __restrict__ sg = shist + iters * nv;
        auto seed = [&](int j, float v) {
            Cv[j] = v;
            ga[j] = -fn * sg[j] * v;
        };
        if constexpr (NH == 2) col_finish_x<QC>(c, *x, 0, cacc, seed);
        else col_finish<QC>(c, cacc, seed);
    }
#pragma unroll 1
    for (int t = iters; t >= 1; --t) {
        int n_ = c.n;
        asm volatile("" : "+v"(n_));   // see ipot_forward_t: uniform row bounds, QC column masks, unconditional clamped loads
        const int n = __builtin_amdgcn_readfirstlane(n_);
        const float* __restrict__ Tt = Thist + (t - 1) * nn;
        const float* __restrict__ dl = dhist + (t - 1) * nv;
        const float* __restrict__ sg = shist + t * nv;
        const float* __restrict__ so = shist + (t - 1) * nv;
        const float ft = (float)t;
        float rsg[QC], soq[QC], gaq[QC], c1[QC], c2[QC];
        uint32_t jc[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            const int j = lane + 64 * q;
            const bool ok = j < n;
            const int jcl = ok ? j : n - 1;
            jc[q] = (uint32_t)jcl << 2;   // BYTE offset
            rsg[q] = ok ? __builtin_amdgcn_rcpf(ld_soff(sg, jc[q])) : 0.f;    // (1-ulp v_rcp_f32) zero outside the matrix: Q vanishes there
            soq[q] = ok ? ld_soff(so, jc[q]) : 0.f;
            gaq[q] = ok ? ga[jcl] : 0.f;
            c1[q] = 0.f;
            c2[q] = 0.f;
        }
#pragma unroll
        for (int r0 = 0; r0 < RPW; r0 += RG) {
            float tt[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = wave + GNW * (NH * (r0 + g) + rhalf), ic = i < n ? i : n - 1;
                const float* __restrict__ Trow = Tt + ic * n;   // scalar row base + 32-bit lane offset
#pragma unroll
                for (int q = 0; q < QC; ++q) tt[g][q] = ld_soff(Trow, jc[q]);
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int r = r0 + g, i = wave + GNW * (NH * r + rhalf);
                const bool iok = i < n;   // wave-uniform
                const float di = iok ? dl[i] : 0.f;
                const float rdi = iok ? __builtin_amdgcn_rcpf(di) : 0.f;
                float rs = 0.f, rs2 = 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float Qv = tt[g][q] * rdi * rsg[q];     // Q_t = T_t / (delta_t,i sigma_t,j)
                    tt[g][q] = Qv;
                    rs += Qv * gaq[q];
                    rs2 += Qv * soq[q];
                }
                rs = wave_sum_dpp(rs);
                rs2 = wave_sum_dpp(rs2);
                const float Ri = iok ? Rv[i] : 0.f;
                const float gri = -fn * di * di * (Ri * rdi + rs);
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float w = tt[g][q] * (di * gaq[q] + gri * soq[q]);
                    if (r < RREG) H[r < RREG ? r : 0][q] += ft * w;
                    else hl[((r - RREG) * QC + q) * GNT] += ft * w;
                    c1[q] += tt[g][q] * gri;
                    c2[q] += w;
                }
                if (lane == 0 && iok) Rv[i] = Ri + di * rs + gri * rs2;   // rowsum(Y_t); row i belongs to this wave alone
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // gsig_old_j = sum_i Q_ij gr_i ; colsum(Y_t) ; the ga of the next reversed iteration (its sigma_t is this one's sigma_{t-1})
        auto merge = [&](int j, float gs, float cw) {
            const float cv = Cv[j] + cw;
            Cv[j] = cv;
            const float s = so[j];
            ga[j] = -fn * s * (s * gs + cv);
        };
        if constexpr (NH == 2) col_finish2_x<QC>(c, *x, iters + 1 - t, c1, c2, merge);
        else col_finish2<QC>(c, c1, c2, merge);
    }
    {
        const int n = __builtin_amdgcn_readfirstlane(c.n);
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = wave + GNW * (NH * r + rhalf);
            if (i < n) {
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const int j = lane + 64 * q;
                    if (j < n) gC_out[i * n + j] = -inv_beta * (r < RREG ? H[r < RREG ? r : 0][q] : hl[((r - RREG) * QC + q) * GNT]);
                }
            }
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// IPOT reverse sweep of the BIG class (256 < n <= 512): the two-pass recurrences (see ipot_backward_h's header) with the plan gradient
// gT and the accumulator gA in the workspace (updated in place) -- n x n / 1024 = 256 accumulator registers per lane do not exist.
// Rows are walked by a dynamic loop (RG rows of loads in flight per wave), so the code stays small.
// ---------------------------------------------------------------------------------------------------------
template <int QC>
__device__ __forceinline__ void ipot_backward_mem(const Ctx& c, const float* __restrict__ Cm, float inv_beta, int iters,
                                                  float* __restrict__ Am, const float* __restrict__ Thist,
                                                  const float* __restrict__ dhist, const float* __restrict__ shist,
                                                  float* __restrict__ gT, float* __restrict__ gA, float* __restrict__ gC_out,
                                                  float* gsig, float* ga, float* gdel) {
    const int tid = c.tid, lane = c.lane, wave = __builtin_amdgcn_readfirstlane(c.wave);
    const int n = c.n;
    const int nn = (int)up4((int64_t)n * n);
    const int nv = (int)up4(n);
    const float fn = (float)n;
    for (int e = tid; e < n * n; e += GNT) {
        Am[e] = expf(-Cm[e] * inv_beta);
        gA[e] = 0.f;
    }
    for (int j = tid; j < n; j += GNT) gsig[j] = 0.f;
    __syncthreads();
    constexpr int RG = QC > 4 ? 1 : 2;   // 4 measured the same (7.2 vs 7.1 ms at n = 256) and starts to spill; QC = 8: one row
    int jc[QC];
    bool jok[QC];
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        const int j = lane + 64 * q;
        jok[q] = j < n;
        jc[q] = jok[q] ? j : n - 1;
    }
#pragma unroll 1
    for (int t = iters; t >= 1; --t) {
        const float* __restrict__ Tp = (t >= 2) ? Thist + (t - 2) * nn : nullptr;
        const float* __restrict__ dl = dhist + (t - 1) * nv;
        const float* __restrict__ sg = shist + t * nv;
        const float* __restrict__ so = shist + (t - 1) * nv;
        float sgq[QC], soq[QC], gaq[QC], cacc[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            sgq[q] = jok[q] ? sg[jc[q]] : 0.f;
            soq[q] = jok[q] ? so[jc[q]] : 0.f;
            cacc[q] = 0.f;
        }
        // P1: gdel_i = sum_j gT_ij Q_ij sig_j ; u_j = sum_i gT_ij del_i Q_ij ; ga_j = -m sig_j^2 (gsig_j + u_j)
#pragma unroll 1
        for (int i0 = wave; i0 < n; i0 += GNW * RG) {
            float a[RG][QC], tp[RG][QC], gv[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g, ic = i < n ? i : n - 1;
                const float* __restrict__ Arow = Am + ic * n;
                const float* __restrict__ Trow = Tp ? Tp + ic * n : nullptr;
                const float* __restrict__ Grow = gT + ic * n;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    a[g][q] = Arow[jc[q]];
                    tp[g][q] = Trow ? Trow[jc[q]] : 1.f;
                    gv[g][q] = Grow[jc[q]];
                }
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g;
                const bool iok = i < n;
                const float di = iok ? dl[i] : 0.f;
                float rs = 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    const float gq = (iok && jok[q]) ? gv[g][q] * (a[g][q] * tp[g][q]) : 0.f;
                    rs += gq * sgq[q];
                    cacc[q] += gq * di;
                }
                rs = wave_sum(rs);
                if (lane == 0 && iok) gdel[i] = rs;
            }
        }
        col_finish<QC>(c, cacc, [&](int j, float u) { ga[j] = -fn * sg[j] * sg[j] * (gsig[j] + u); });
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            gaq[q] = jok[q] ? ga[jc[q]] : 0.f;
            cacc[q] = 0.f;
        }
        // P2 (row): gdel_i += sum_j Q_ij ga_j ; gr_i = -n del_i^2 gdel_i
        // P3 (same row): gsig_old_j = sum_i Q_ij gr_i ; gQ = gT del sig + ga del + gr sig_old ; gA += gQ T_prev ; gT <- gQ A
#pragma unroll 1
        for (int i0 = wave; i0 < n; i0 += GNW * RG) {
            float a[RG][QC], tp[RG][QC], gv[RG][QC], gacc[RG][QC];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g, ic = i < n ? i : n - 1;
                const float* __restrict__ Arow = Am + ic * n;
                const float* __restrict__ Trow = Tp ? Tp + ic * n : nullptr;
                const float* __restrict__ Grow = gT + ic * n;
                const float* __restrict__ Crow = gA + ic * n;
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    a[g][q] = Arow[jc[q]];
                    tp[g][q] = Trow ? Trow[jc[q]] : 1.f;
                    gv[g][q] = Grow[jc[q]];
                    gacc[g][q] = Crow[jc[q]];
                }
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int i = i0 + GNW * g;
                const bool iok = i < n;   // wave-uniform
                const float di = iok ? dl[i] : 0.f;
                float rs = 0.f;
#pragma unroll
                for (int q = 0; q < QC; ++q) rs += (a[g][q] * tp[g][q]) * gaq[q];   // gaq is zero outside the matrix
                rs = wave_sum(rs);
                const float gri = iok ? -fn * di * di * (gdel[i] + rs) : 0.f;
                if (iok) {
#pragma unroll
                    for (int q = 0; q < QC; ++q) {
                        if (jok[q]) {
                            cacc[q] += a[g][q] * tp[g][q] * gri;
                            const float gQ = gv[g][q] * di * sgq[q] + gaq[q] * di + gri * soq[q];
                            (gA + i * n)[jc[q]] = gacc[g][q] + gQ * tp[g][q];
                            (gT + i * n)[jc[q]] = gQ * a[g][q];
                        }
                    }
                }
            }
        }
        col_finish<QC>(c, cacc, [&](int j, float v) { gsig[j] = v; });
    }
    // dL/dC = dL/dA * dA/dC = gA * (-1/beta) A
    for (int e = tid; e < n * n; e += GNT) gC_out[e] = -inv_beta * gA[e] * Am[e];
    __syncthreads();
}


// =========================================================================================================
// K1: normalise tokens, raw cost matrices (matrix cores), per-case extrema
// =========================================================================================================
template <bool BIG>
__global__ __launch_bounds__(GNT) void got_prep_kernel(const GotBatch B) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float ext[GNW][6];
    int b = blockIdx.x;
    const GotProb P = got_pick(B, 1, b);
    const float* __restrict__ V = P.V;
    const float* __restrict__ Q = P.Q;
    float* ws = P.ws;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    float* base = ws + (int64_t)b * L.per_case;
    float* Vh = base + L.oVh;
    float* Qh = base + L.oQh;
    // normalise: one wave per token row
    for (int r = c.wave; r < 2 * n; r += GNW) {
        const bool isq = r >= n;
        const int i = isq ? r - n : r;
        const float* src = (isq ? Q : V) + ((int64_t)b * n + i) * d;
        float ss = 0.f;
        for (int e = c.lane; e < d; e += 64) ss += src[e] * src[e];
        ss = wave_sum(ss);
        const float nr = sqrtf(ss);
        const float s = 1.f / (nr + 1e-12f);
        float* dst = (isq ? Qh : Vh) + i * d;
        for (int e = c.lane; e < d; e += 64) dst[e] = src[e] * s;
        if (c.lane == 0) (base + (isq ? L.orQ : L.orV))[i] = nr;
    }
    __syncthreads();
    // raw costs 1 - <x_i, y_j>, 3 matrices; running extrema per thread
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    mmx<BIG, false, true, !BIG>(c, n, n, d, Vh, d, Qh, d, [&](int i, int j, float v) {
        const float x = 1.f - v;
        base[L.oC0 + i * n + j] = x;
        mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
    });
    mmx<BIG, false, true, !BIG>(c, n, n, d, Vh, d, Vh, d, [&](int i, int j, float v) {
        const float x = 1.f - v;
        base[L.oCs0 + i * n + j] = x;
        mn[1] = fminf(mn[1], x); mx[1] = fmaxf(mx[1], x);
    });
    mmx<BIG, false, true, !BIG>(c, n, n, d, Qh, d, Qh, d, [&](int i, int j, float v) {
        const float x = 1.f - v;
        base[L.oCt0 + i * n + j] = x;
        mn[2] = fminf(mn[2], x); mx[2] = fmaxf(mx[2], x);
    });
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float a = mn[m], z = mx[m];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a = fminf(a, __shfl_xor(a, o, 64));
            z = fmaxf(z, __shfl_xor(z, o, 64));
        }
        if (c.lane == 0) {
            ext[c.wave][2 * m] = a;
            ext[c.wave][2 * m + 1] = z;
        }
    }
    __syncthreads();
    if (c.tid < 6) {
        float v = ext[0][c.tid];
        for (int w = 1; w < GNW; ++w) v = (c.tid & 1) ? fmaxf(v, ext[w][c.tid]) : fminf(v, ext[w][c.tid]);
        ws[L.g_ext + (int64_t)b * 6 + c.tid] = v;
    }
}

// K2: global extrema (local to this call) -> minmax_out; thresholds from minmax_in if given, else the local ones
__global__ __launch_bounds__(64) void got_minmax_kernel(const GotBatch B) {   // one block per problem
    const GotProb P = got_prob(B, blockIdx.x);
    float* ws = P.ws;
    float* __restrict__ minmax_out = P.mm_out;
    const float* __restrict__ minmax_in = P.mm_in;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const int tid = threadIdx.x;
    if (tid < 6) {
        float v = (tid & 1) ? -INFINITY : INFINITY;
        for (int b = 0; b < k; ++b) {
            const float x = ws[L.g_ext + (int64_t)b * 6 + tid];
            v = (tid & 1) ? fmaxf(v, x) : fminf(v, x);
        }
        if (minmax_out) minmax_out[tid] = v;
        ws[L.g_thr + tid] = minmax_in ? minmax_in[tid] : v;
    }
    __syncthreads();
    if (tid < 3) {
        const float lo = ws[L.g_thr + 2 * tid], hi = ws[L.g_thr + 2 * tid + 1];
        ws[L.g_thr + 6 + tid] = lo + THR_BETA * (hi - lo);
    }
    if (tid == 0) ws[L.g_gen + 1] = 0.f;   // exchange time-out flag of the split sweeps (Xch): defined in every size class from here on
}

// =========================================================================================================
// K3: Wasserstein branch forward (three phases: thresholds + tie counts | IPOT | distance)
// =========================================================================================================
__device__ __forceinline__ void wd_fwd_init(const Ctx& c, float* ws, const GotWs& L, int b) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const float thr = ws[L.g_thr + 6], e0 = ws[L.g_thr + 0], e1 = ws[L.g_thr + 1];
    float* C = base + L.oC;
    float c0 = 0.f, c1 = 0.f;
    for (int e = c.tid; e < n * n; e += GNT) {
        const float x = base[L.oC0 + e];
        C[e] = fmaxf(x - thr, 0.f);
        c0 += x == e0;
        c1 += x == e1;
    }
    c0 = block_sum(c, c0, 0);
    c1 = block_sum(c, c1, 1);
    if (c.tid == 0) {
        ws[L.g_cnt + (int64_t)b * 6 + 0] = c0;
        ws[L.g_cnt + (int64_t)b * 6 + 1] = c1;
    }
    __syncthreads();
}
template <int RPW, int QC>
__device__ __forceinline__ void wd_fwd_ipot(const Ctx& c, float* ws, const GotWs& L, int b, float* sig, float* del) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const float* C = base + L.oC;
    ipot_forward_t<RPW, QC>(c, C, WD_INV_BETA, WD_ITERS, base + L.oA2, base + L.oWT, base + L.oWd, base + L.oWs, sig, del);
    const float* T = base + L.oWT + (WD_ITERS - 1) * up4(n * n);
    float s = 0.f;
    for (int e = c.tid; e < n * n; e += GNT) s += C[e] * T[e];
    s = block_sum(c, s);
    if (c.tid == 0) ws[L.g_wd + b] = s;
}

// =========================================================================================================
// K4: Gromov-Wasserstein branch forward (phases: thresholds + Cst vectors | C_gamma(o) | IPOT(o) | distance)
// =========================================================================================================
template <bool BIG, bool WOK = false>
__device__ __forceinline__ void gw_cgamma(const Ctx& c, const float* __restrict__ Cs, const float* __restrict__ Ct,
                          const float* __restrict__ gamma /* nullptr => uniform 1/n^2 */, const float* rs, const float* rt,
                          float* __restrict__ P1, float* __restrict__ Cg) {
    const int n = c.n;
    if (gamma) {
        // P1 = gamma * Ct^T (= gamma * Ct, Ct symmetric);  Cg = rs_i + rt_j - 2 (Cs P1)_ij
        mmx<BIG, false, false, WOK>(c, n, n, n, gamma, n, Ct, n, [&](int i, int j, float v) { P1[i * n + j] = v; });
    } else {
        // gamma = 1/n^2 everywhere: (gamma Ct^T)_kj = (1/n^2) sum_l Ct_jl, the same for every k
        for (int j = c.wave; j < n; j += GNW) {
            float s = 0.f;
            for (int l = c.lane; l < n; l += 64) s += Ct[j * n + l];
            s = wave_sum(s) / ((float)n * (float)n);
            for (int kk = c.lane; kk < n; kk += 64) P1[kk * n + j] = s;
        }
    }
    __syncthreads();
    mmx<BIG, false, false, WOK>(c, n, n, n, Cs, n, P1, n, [&](int i, int j, float v) { Cg[i * n + j] = (rs[i] + rt[j]) - 2.f * v; });
}
// Rows [r0, r1) (at most 128 of them) of the same C_gamma by ONE of two workgroups of a case (round 6: a rank's launch holds k <= 128 cases
// -- with one workgroup per case the n^3 products of the forward ran on half of the chip).  No exchange between the halves: the chain is
// re-associated, Cg[rows] = rs + rt - 2 (Cs[rows, :] gamma) Ct, so a half needs only its own rows of the intermediate (P holds them at
// their global row positions; the two halves write disjoint rows).  gamma == nullptr (outer iteration 0): the column-constant gamma Ct^T
// is cheap -- every half builds its own full copy in P (the halves are handed different buffers) and multiplies as the one-workgroup form
// does (same bits for its rows).
__device__ __forceinline__ void gw_cgamma_half(const Ctx& c, const float* __restrict__ Cs, const float* __restrict__ Ct,
                                               const float* __restrict__ gamma, const float* rs, const float* rt, float* __restrict__ P,
                                               float* __restrict__ Cg, int r0, int r1) {
    const int n = c.n, m = r1 - r0;
    if (gamma) {
        mm_impl<false, false, 2>(c, m, n, n, Cs + (int64_t)r0 * n, n, gamma, n, [&](int i, int j, float v) { P[(r0 + i) * n + j] = v; });
        __syncthreads();
        mm_impl<false, false, 2>(c, m, n, n, P + (int64_t)r0 * n, n, Ct, n,
                                 [&](int i, int j, float v) { Cg[(r0 + i) * n + j] = (rs[r0 + i] + rt[j]) - 2.f * v; });
    } else {
        for (int j = c.wave; j < n; j += GNW) {
            float s = 0.f;
            for (int l = c.lane; l < n; l += 64) s += Ct[j * n + l];
            s = wave_sum(s) / ((float)n * (float)n);
            for (int kk = c.lane; kk < n; kk += 64) P[kk * n + j] = s;
        }
        __syncthreads();
        mm_impl<false, false, 2>(c, m, n, n, Cs + (int64_t)r0 * n, n, P, n,
                                 [&](int i, int j, float v) { Cg[(r0 + i) * n + j] = (rs[r0 + i] + rt[j]) - 2.f * v; });
    }
}

// thresholded intra costs, tie counts, rs/rt (to LDS and to the workspace)
__device__ __forceinline__ void gw_fwd_init(const Ctx& c, float* ws, const GotWs& L, int b, float* rs, float* rt) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const float thr_s = ws[L.g_thr + 7], thr_t = ws[L.g_thr + 8];
    const float e2 = ws[L.g_thr + 2], e3 = ws[L.g_thr + 3], e4 = ws[L.g_thr + 4], e5 = ws[L.g_thr + 5];
    float* Cs = base + L.oCs;
    float* Ct = base + L.oCt;
    float cn[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = c.tid; e < n * n; e += GNT) {
        const float x = base[L.oCs0 + e], y = base[L.oCt0 + e];
        Cs[e] = fmaxf(x - thr_s, 0.f);
        Ct[e] = fmaxf(y - thr_t, 0.f);
        cn[0] += x == e2; cn[1] += x == e3;
        cn[2] += y == e4; cn[3] += y == e5;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float v = block_sum(c, cn[m], m & 1);
        if (c.tid == 0) ws[L.g_cnt + (int64_t)b * 6 + 2 + m] = v;
        if (m & 1) __syncthreads();
    }
    __syncthreads();
    // rs_i = (1/n) sum_k Cs_ik^2 ; rt_j = (1/n) sum_l Ct_jl^2     (Cst = rs 1^T + 1 rt^T, loss.py:240-241)
    for (int i = c.wave; i < n; i += GNW) {
        float a = 0.f, z = 0.f;
        for (int j = c.lane; j < n; j += 64) {
            const float x = Cs[i * n + j], y = Ct[i * n + j];
            a += x * x;
            z += y * y;
        }
        a = wave_sum(a);
        z = wave_sum(z);
        if (c.lane == 0) {
            rs[i] = a / (float)n;
            rt[i] = z / (float)n;
            base[L.ors + i] = rs[i];
            base[L.ort + i] = rt[i];
        }
    }
    __syncthreads();
}
__device__ __forceinline__ void gw_load_rsrt(const Ctx& c, float* ws, const GotWs& L, int b, float* rs, float* rt) {
    const float* base = ws + (int64_t)b * L.per_case;
    for (int i = c.tid; i < c.n; i += GNT) {
        rs[i] = base[L.ors + i];
        rt[i] = base[L.ort + i];
    }
    __syncthreads();
}
__device__ __forceinline__ const float* gw_gamma_of(const float* base, const GotWs& L, int o, int nn) {  // plan of outer o
    return base + L.oGT + (o * GW_INNER + (GW_INNER - 1)) * nn;
}
// C_gamma of outer iteration o (o == GW_OUTER: the final one, written to P2 together with the distance)
template <bool BIG = false, bool WOK = false>
__device__ __forceinline__ void gw_fwd_cgamma(const Ctx& c, float* ws, const GotWs& L, int b, int o, const float* rs, const float* rt) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n);
    const float* gamma = (o >= 1) ? gw_gamma_of(base, L, o - 1, nn) : nullptr;
    float* dst = (o < GW_OUTER) ? base + L.oCg + o * nn : base + L.oP2;
    gw_cgamma<BIG, WOK>(c, base + L.oCs, base + L.oCt, gamma, rs, rt, base + L.oP1, dst);
    if (o == GW_OUTER) {  // gwd_b = sum C_gamma * gamma
        float s = 0.f;
        for (int e = c.tid; e < n * n; e += GNT) s += dst[e] * gamma[e];
        s = block_sum(c, s);
        if (c.tid == 0) ws[L.g_gwd + b] = s;
    }
}
template <int RPW, int QC>
__device__ __forceinline__ void gw_fwd_ipot(const Ctx& c, float* ws, const GotWs& L, int b, int o, float* sig, float* del) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n);
    const int nv = (int)up4(n);
    ipot_forward_t<RPW, QC>(c, base + L.oCg + o * nn, GW_INV_BETA, GW_INNER, base + L.oA, base + L.oGT + o * GW_INNER * nn,
                            base + L.oGd + o * GW_INNER * nv, base + L.oGs + o * (GW_INNER + 1) * nv, sig, del);
}

// fused chain: blocks [0,k): Wasserstein branch of case b; blocks [k,2k): Gromov-Wasserstein branch of case b - k
template <int RPW, int QC>
__global__ __launch_bounds__(GNT) void got_main_kernel(const GotBatch B) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float sig[GOT_REGN], del[GOT_REGN], rs[GOT_REGN], rt[GOT_REGN];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, 2, bid);
    float* ws = P.ws;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    if (bid < k) {
        wd_fwd_init(c, ws, L, bid);
        wd_fwd_ipot<RPW, QC>(c, ws, L, bid, sig, del);
    } else {
        const int b = bid - k;
        gw_fwd_init(c, ws, L, b, rs, rt);
#pragma unroll 1
        for (int o = 0; o < GW_OUTER; ++o) {
            gw_fwd_cgamma(c, ws, L, b, o, rs, rt);
            gw_fwd_ipot<RPW, QC>(c, ws, L, b, o, sig, del);
        }
        gw_fwd_cgamma(c, ws, L, b, GW_OUTER, rs, rt);
    }
}

// The same chain as one launch per phase (n > 128): each phase is its own kernel, so the register allocation of the
// IPOT sweeps (the plan lives in registers) is not shared with the matrix products' 128 accumulator registers.
//   STAGE 0: thresholds (2k blocks)   1: C_gamma(o) (k blocks)   2: IPOT(o) (k blocks, + k Wasserstein blocks when o == 0)
//   STAGE 4: C_gamma(o), o < GW_OUTER, by row halves (2k blocks; round 6)
//   BIG (256 < n <= 512): the plan lives in the history (ipot_forward_mem), blocked matrix products
template <int RPW, int QC, int STAGE, bool BIG = false>
__global__ __launch_bounds__(GNT) void got_fwd_stage_kernel(const GotBatch B, int o, int mult) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float va[BIG ? GOT_BIGN : GOT_REGN], vb[BIG ? GOT_BIGN : GOT_REGN];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, mult, bid);
    float* ws = P.ws;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    if constexpr (STAGE == 0) {
        if (bid < k) wd_fwd_init(c, ws, L, bid);
        else gw_fwd_init(c, ws, L, bid - k, va, vb);
        if constexpr (!BIG) {
            // split sweeps (Xch): clear this branch's exchange granules (tag 0 never matches), start a new pass generation
            float* xb = ws + (int64_t)(bid < k ? bid : bid - k) * L.per_case + L.oX + (bid < k ? XCH_FLOATS / 2 : 0);
            for (int e = c.tid; e < XCH_FLOATS / 2; e += GNT) xb[e] = 0.f;
            if (bid == 0 && c.tid == 0) {
                ws[L.g_gen] = __uint_as_float(__float_as_uint(ws[L.g_gen]) + 1u);
                ws[L.g_gen + 1] = 0.f;
            }
        }
    } else if constexpr (STAGE == 1) {
        gw_load_rsrt(c, ws, L, bid, va, vb);
        gw_fwd_cgamma<BIG, !BIG>(c, ws, L, bid, o, va, vb);
    } else if constexpr (STAGE == 4) {
        // C_gamma(o), o < GW_OUTER, as TWO workgroups per case (2k blocks): rows [0, 128) | [128, n) (gw_cgamma_half)
        const int half = bid >= k ? 1 : 0, b = bid - half * k;
        const int r0 = half ? 128 : 0, r1 = half ? n : (n < 128 ? n : 128);
        if (r1 <= r0) return;   // block-uniform: a case of a smaller problem of the batch has no second half
        gw_load_rsrt(c, ws, L, b, va, vb);
        float* base = ws + (int64_t)b * L.per_case;
        const int nn = (int)up4((int64_t)n * n);
        const float* gamma = (o >= 1) ? gw_gamma_of(base, L, o - 1, nn) : nullptr;
        gw_cgamma_half(c, base + L.oCs, base + L.oCt, gamma, va, vb, (gamma || !half) ? base + L.oP1 : base + L.oP2, base + L.oCg + o * nn, r0,
                       r1);
    } else {
        // ONE inlined copy of the sweep serves both branches (two call sites = two copies = spills): select the operands
        const bool wd = bid >= k;
        const int b = wd ? bid - k : bid;
        float* base = ws + (int64_t)b * L.per_case;
        const int nn = (int)up4((int64_t)n * n), nv = (int)up4(n);
        const float* Cm = wd ? base + L.oC : base + L.oCg + o * nn;
        if constexpr (BIG)
            ipot_forward_mem<QC>(c, Cm, wd ? WD_INV_BETA : GW_INV_BETA, wd ? WD_ITERS : GW_INNER, wd ? base + L.oA2 : base + L.oA,
                                 wd ? base + L.oWT : base + L.oGT + o * GW_INNER * nn,
                                 wd ? base + L.oWd : base + L.oGd + o * GW_INNER * nv,
                                 wd ? base + L.oWs : base + L.oGs + o * (GW_INNER + 1) * nv, va, vb);
        else
        ipot_forward_t<RPW, QC>(c, Cm, wd ? WD_INV_BETA : GW_INV_BETA, wd ? WD_ITERS : GW_INNER, wd ? base + L.oA2 : base + L.oA,
                                wd ? base + L.oWT : base + L.oGT + o * GW_INNER * nn,
                                wd ? base + L.oWd : base + L.oGd + o * GW_INNER * nv,
                                wd ? base + L.oWs : base + L.oGs + o * (GW_INNER + 1) * nv, va, vb);
        if (wd) {  // wd_b = sum C * T_final
            const float* T = base + L.oWT + (WD_ITERS - 1) * nn;
            float s = 0.f;
            for (int e = c.tid; e < n * n; e += GNT) s += Cm[e] * T[e];
            s = block_sum(c, s);
            if (c.tid == 0) ws[L.g_wd + b] = s;
        }
    }
}

// STAGE 2 as a SPLIT sweep (see Xch): two workgroups per case and branch.  mode 0: 2k blocks, the Gromov-Wasserstein sweep of outer
// iteration o;  mode 1: 4k blocks, [0, 2k) the same and [2k, 4k) the Wasserstein sweep;  mode 2: 2k blocks, the Wasserstein sweep alone.
// RPW = rows per wave of ONE half (8 at n <= 256, 6 at n <= 192).
template <int RPW, int QC>
__global__ __launch_bounds__(GNT) void got_fwd_sweep_split_kernel(const GotBatch B, int o, int mode) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float va[GOT_REGN];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, mode == 1 ? 4 : 2, bid);
    float* ws = P.ws;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    const int half = bid & 1, u = bid >> 1;
    const bool wd = mode == 2 || (mode == 1 && u >= k);
    const int b = (mode == 1 && wd) ? u - k : u;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n), nv = (int)up4(n);
    Xch x = make_xch(ws, L, base, wd ? 1 : 0, half, wd ? 200 : 1 + 32 * o);
    const float* Cm = wd ? base + L.oC : base + L.oCg + o * nn;
    ipot_forward_split<RPW, QC>(c, x, Cm, wd ? WD_INV_BETA : GW_INV_BETA, wd ? WD_ITERS : GW_INNER,
                                wd ? base + L.oWT : base + L.oGT + o * GW_INNER * nn,
                                wd ? base + L.oWd : base + L.oGd + o * GW_INNER * nv,
                                wd ? base + L.oWs : base + L.oGs + o * (GW_INNER + 1) * nv, va);
    if (wd) {  // wd_b = sum C * T_final: this half's rows (every lane re-reads the plan elements it wrote), then the partner's partial
        const float* T = base + L.oWT + (WD_ITERS - 1) * nn;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = c.wave + GNW * (2 * r + half);
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                const int j = c.lane + 64 * q;
                if (i < n && j < n) s += Cm[i * n + j] * T[i * n + j];
            }
        }
        s = block_sum_x(c, x, WD_ITERS, s);
        if (c.tid == 0 && half == 0) ws[L.g_wd + b] = s;
    }
}

__global__ __launch_bounds__(64) void got_sum_kernel(const GotBatch B) {   // one block per problem
    const GotProb P = got_prob(B, blockIdx.x);
    const float* ws = P.ws;
    float* __restrict__ out = P.out;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    if (threadIdx.x < 2) {
        const float* src = ws + (threadIdx.x ? L.g_gwd : L.g_wd);
        float s = 0.f;
        for (int b = 0; b < k; ++b) s += src[b];
        // a split sweep gave up waiting for its partner (Xch: the device was shared with work this launch did not know about): the
        // pass's numbers are void -- say so in the value itself instead of in a flag nobody reads: NaN distances, NaN gradients
        out[threadIdx.x] = (ws[L.g_gen + 1] != 0.f) ? __builtin_nanf("") : s;
    }
}

// =========================================================================================================
// backward K6: Wasserstein branch.  wd_b = sum C*T(C):  gC = g (T + dT/dC^T [C]);  masked to the raw-cost
// gradient (ogC0), plus this case's threshold-gradient partial.
// =========================================================================================================
template <int RPW, int QC>
__device__ __forceinline__ void got_wd_bwd(const Ctx& c, float* ws, const GotWs& L, int b, const float* __restrict__ d_out, float* gsig,
                           float* ga, float* gdel) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n);
    const float g = d_out[0];
    const float* C = base + L.oC;
    const float* Tf = base + L.oWT + (WD_ITERS - 1) * nn;
    float* gC = base + L.ogC0;
    // seed of the Wasserstein reverse: gT = g C (formed inside the sweep: gT_in = C, gscale = g)
    ipot_backward_h<RPW, QC>(c, WD_INV_BETA, WD_ITERS, base + L.oWT, base + L.oWd, base + L.oWs, C, g, gC, ga, gdel, gsig);
    // total dL/dC = g T_final + (through IPOT) ; mask by relu ; accumulate -sum as threshold gradient
    const float thr = ws[L.g_thr + 6];
    float s = 0.f;
    for (int e = c.tid; e < n * n; e += GNT) {
        const float gc = g * Tf[e] + gC[e];
        const float m = (base[L.oC0 + e] - thr > 0.f) ? gc : 0.f;
        gC[e] = m;
        s -= m;
    }
    s = block_sum(c, s);
    if (c.tid == 0) ws[L.g_gthr + (int64_t)b * 3 + 0] = s;
}

// =========================================================================================================
// backward K7: Gromov-Wasserstein branch -> gCs, gCt (wrt thresholded intra costs), then masked to raw costs.
// Phases: seed | per outer iteration o = 5..0: products (gw_bwd_products) then the IPOT sweep of o-1 | Cst terms + masks.
// The Cst-vector gradients grs, grt live in the workspace (they persist across the per-phase launches).
// =========================================================================================================
__device__ __forceinline__ void gw_bwd_init(const Ctx& c, float* ws, const GotWs& L, int b, const float* __restrict__ d_out) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n);
    const int N2 = n * n;
    const float g = d_out[1];
    float* gCs = base + L.ogCs;
    float* gCt = base + L.ogCt;
    float* G = base + L.oG;     // gradient wrt the current C_gamma
    // seed: gwd = sum C_gamma_final * gamma5 (gamma5 detached as a factor) => G = g * gamma5
    const float* gamma5 = gw_gamma_of(base, L, GW_OUTER - 1, nn);
    for (int e = c.tid; e < N2; e += GNT) {
        gCs[e] = 0.f;
        gCt[e] = 0.f;
        G[e] = g * gamma5[e];
    }
    for (int i = c.tid; i < n; i += GNT) {
        base[L.ogrs + i] = 0.f;
        base[L.ogrt + i] = 0.f;
    }
    __syncthreads();
}

// C_gamma^{(o)} = rs_i + rt_j - 2 (Cs gam Ct)_ij with gam = gamma^{(o-1)} (uniform for o == 0): from G = d/dC_gamma^{(o)}
// accumulate the Cst-vector, gCs, gCt gradients and write gT = d/d gamma^{(o-1)} (o >= 1).
// part: -1 = everything (the fused kernels); the per-phase launches give every case TWO workgroups for o >= 1 -- 0: Cst sums, G Ct,
// gCs, gT (three products), 1: Cs gam, gCt (two) -- the halves write disjoint arrays and only read G, Cs, Ct, gam.
template <bool BIG = false, int QC = 4, bool WOK = false>
__device__ __forceinline__ void gw_bwd_products(const Ctx& c, float* ws, const GotWs& L, int b, int o, float* ga, float* gdel,
                                                int part = -1) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n);
    const int N2 = n * n;
    const float* Cs = base + L.oCs;
    const float* Ct = base + L.oCt;
    float* gCs = base + L.ogCs;
    float* gCt = base + L.ogCt;
    float* grs = base + L.ogrs;
    float* grt = base + L.ogrt;
    float* G = base + L.oG;
    float* P1 = base + L.oP1;
    float* P2 = base + L.oP2;
    float* gT = base + L.ogT;
    const float* gam = (o >= 1) ? gw_gamma_of(base, L, o - 1, nn) : nullptr;
    // Cst gradient: grs_i += sum_j G_ij ; grt_j += sum_i G_ij
    if (part != 1) {
        float cacc[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) cacc[q] = 0.f;
        for (int i = c.wave; i < n; i += GNW) {
            float r = 0.f;
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                const int j = c.lane + 64 * q;
                if (j < n) {
                    const float v = G[i * n + j];
                    r += v;
                    cacc[q] += v;
                }
            }
            r = wave_sum(r);
            if (c.lane == 0) grs[i] += r;
        }
        col_finish<QC>(c, cacc, [&](int j, float v) { grt[j] += v; });
    }
    // M = Cs gam Ct:  gCs += -2 G (gam Ct)^T = -2 G Ct gam^T ; gCt += -2 G^T (Cs gam) ; ggam = -2 Cs G Ct
    if (gam) {
        if (part != 1) {
            mmx<BIG, false, false, WOK>(c, n, n, n, G, n, Ct, n, [&](int i, int j, float v) { P1[i * n + j] = v; });          // G Ct
            mmx<BIG, false, true, WOK>(c, n, n, n, P1, n, gam, n, [&](int i, int j, float v) { gCs[i * n + j] -= 2.f * v; });  // (G Ct) gam^T
        }
        if (part != 0) {
            mmx<BIG, false, false, WOK>(c, n, n, n, Cs, n, gam, n, [&](int i, int j, float v) { P2[i * n + j] = v; });        // Cs gam
            mmx<BIG, true, false, WOK>(c, n, n, n, G, n, P2, n, [&](int i, int j, float v) { gCt[i * n + j] -= 2.f * v; });    // G^T (Cs gam)
        }
        if (part != 1)
            mmx<BIG, false, false, WOK>(c, n, n, n, Cs, n, P1, n, [&](int i, int j, float v) { gT[i * n + j] = -2.f * v; });   // Cs (G Ct)
    } else if (part != 1) {
        // gam = 1/n^2 (constant): (G Ct gam^T)_ik = (1/n^2) sum_l (G Ct)_il ; (G^T Cs gam)_jl = (1/n^2) sum_i G_ij sum_k Cs_ik
        const float inv = 1.f / ((float)n * (float)n);
        mmx<BIG, false, false, WOK>(c, n, n, n, G, n, Ct, n, [&](int i, int j, float v) { P1[i * n + j] = v; });
        for (int i = c.wave; i < n; i += GNW) {
            float r = 0.f, cs = 0.f;
            for (int j = c.lane; j < n; j += 64) {
                r += P1[i * n + j];
                cs += Cs[i * n + j];
            }
            r = wave_sum(r) * inv;
            cs = wave_sum(cs) * inv;
            for (int kk = c.lane; kk < n; kk += 64) gCs[i * n + kk] -= 2.f * r;
            if (c.lane == 0) gdel[i] = cs;  // (Cs gam)_i* = cs (constant along columns)
        }
        __syncthreads();
        // gCt_jl += -2 sum_i G_ij (Cs gam)_il = -2 sum_i G_ij cs_i   (same for every l)
        float cacc[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) cacc[q] = 0.f;
        for (int i = c.wave; i < n; i += GNW) {
            const float w = gdel[i];
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                const int j = c.lane + 64 * q;
                if (j < n) cacc[q] += G[i * n + j] * w;
            }
        }
        col_finish<QC>(c, cacc, [&](int j, float v) { ga[j] = -2.f * v; });
        for (int e = c.tid; e < N2; e += GNT) gCt[e] += ga[(int)(e / n)];
        __syncthreads();
    }
}
// gT holds d/d gamma^{(oo)}; back through the IPOT of outer oo -> gradient wrt C_gamma^{(oo)} into G
template <int RPW, int QC>
__device__ __forceinline__ void gw_bwd_ipot(const Ctx& c, float* ws, const GotWs& L, int b, int oo, float* gsig, float* ga, float* gdel) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n);
    const int nv = (int)up4(n);
    ipot_backward_h<RPW, QC>(c, GW_INV_BETA, GW_INNER, base + L.oGT + oo * GW_INNER * nn, base + L.oGd + oo * GW_INNER * nv,
                             base + L.oGs + oo * (GW_INNER + 1) * nv, base + L.ogT, 1.f, base + L.oG, ga, gdel, gsig);
}
// Cst terms: rs_i = (1/n) sum_k Cs_ik^2  => gCs_ik += (2/n) Cs_ik grs_i ; same for Ct; ReLU masks; threshold partials
__device__ __forceinline__ void gw_bwd_final(const Ctx& c, float* ws, const GotWs& L, int b) {
    const int n = c.n;
    float* base = ws + (int64_t)b * L.per_case;
    const int N2 = n * n;
    const float* Cs = base + L.oCs;
    const float* Ct = base + L.oCt;
    float* gCs = base + L.ogCs;
    float* gCt = base + L.ogCt;
    const float* grs = base + L.ogrs;
    const float* grt = base + L.ogrt;
    const float thr_s = ws[L.g_thr + 7], thr_t = ws[L.g_thr + 8];
    float ss = 0.f, st = 0.f;
    for (int e = c.tid; e < N2; e += GNT) {
        const int i = (int)(e / n);
        float a = gCs[e] + (2.f / (float)n) * Cs[e] * grs[i];
        float z = gCt[e] + (2.f / (float)n) * Ct[e] * grt[i];
        a = (base[L.oCs0 + e] - thr_s > 0.f) ? a : 0.f;
        z = (base[L.oCt0 + e] - thr_t > 0.f) ? z : 0.f;
        gCs[e] = a;  // now gradients wrt the RAW intra costs
        gCt[e] = z;
        ss -= a;
        st -= z;
    }
    ss = block_sum(c, ss, 0);
    st = block_sum(c, st, 1);
    if (c.tid == 0) {
        ws[L.g_gthr + (int64_t)b * 3 + 1] = ss;
        ws[L.g_gthr + (int64_t)b * 3 + 2] = st;
    }
}

// fused reverse chain
template <int RPW, int QC>
__global__ __launch_bounds__(GNT) void got_main_bwd_kernel(const GotBatch B) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float gsig[GOT_REGN], ga[GOT_REGN], gdel[GOT_REGN];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, 2, bid);
    float* ws = P.ws;
    const float* __restrict__ d_out = P.d_out;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    // the GW sweeps are ~4x longer than the WD sweep: schedule them first
    if (bid < k) {
        const int b = bid;
        gw_bwd_init(c, ws, L, b, d_out);
#pragma unroll 1
        for (int o = GW_OUTER; o >= 0; --o) {
            gw_bwd_products(c, ws, L, b, o, ga, gdel);
            if (o >= 1) gw_bwd_ipot<RPW, QC>(c, ws, L, b, o - 1, gsig, ga, gdel);
        }
        gw_bwd_final(c, ws, L, b);
    } else {
        got_wd_bwd<RPW, QC>(c, ws, L, bid - k, d_out, gsig, ga, gdel);
    }
}

// per-phase launches of the reverse chain (n > 128), see got_fwd_stage_kernel.
//   STAGE 0: seed (k blocks)   1: products(o) (k)   2: IPOT sweep of outer o (k, + k whole Wasserstein reverses on the first)
//   3: Cst terms + masks (k)
template <int RPW, int QC, int STAGE, bool BIG = false>
__global__ __launch_bounds__(GNT) void got_bwd_stage_kernel(const GotBatch B, int o, int mult /* 2: blocks >= k = Wasserstein reverses */) {
    __shared__ float smem[GOT_SMEM];
    constexpr int VN = BIG ? GOT_BIGN : GOT_REGN;
    __shared__ float gsig[VN], ga[VN], gdel[VN];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, mult, bid);
    float* ws = P.ws;
    const float* __restrict__ d_out = P.d_out;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    if constexpr (STAGE == 0) {
        gw_bwd_init(c, ws, L, bid, d_out);
        if (!BIG && bid == 0 && c.tid == 0) ws[L.g_gen] = __uint_as_float(__float_as_uint(ws[L.g_gen]) + 1u);   // new pass generation (Xch)
    } else if constexpr (STAGE == 1) {
        // mult == 2 (o >= 1): blocks [0, k) take part 0 of case bid, blocks [k, 2k) part 1 of case bid - k
        gw_bwd_products<BIG, QC, !BIG>(c, ws, L, bid >= k ? bid - k : bid, o, ga, gdel, mult == 2 ? (bid >= k ? 1 : 0) : -1);
    } else if constexpr (STAGE == 2) {
        // one inlined copy of the reverse sweep for both branches (see got_fwd_stage_kernel)
        const bool wd = bid >= k;
        const int b = wd ? bid - k : bid;
        float* base = ws + (int64_t)b * L.per_case;
        const int nn = (int)up4((int64_t)n * n), nv = (int)up4(n);
        static_assert(BIG, "the n <= 256 classes run the sweep in got_bwd_sweep_kernel");
        float* A2 = base + L.oA2;
        if (wd) {  // seed of the Wasserstein reverse: gT = g * C
            const float g = d_out[0];
            for (int e = c.tid; e < n * n; e += GNT) A2[nn + e] = g * base[L.oC + e];
            __syncthreads();
        }
        const float* Cm = wd ? base + L.oC : base + L.oCg + o * nn;
        ipot_backward_mem<QC>(c, Cm, wd ? WD_INV_BETA : GW_INV_BETA, wd ? WD_ITERS : GW_INNER, wd ? A2 : base + L.oA,
                              wd ? base + L.oWT : base + L.oGT + o * GW_INNER * nn,
                              wd ? base + L.oWd : base + L.oGd + o * GW_INNER * nv,
                              wd ? base + L.oWs : base + L.oGs + o * (GW_INNER + 1) * nv, wd ? A2 + nn : base + L.ogT,
                              wd ? A2 + 2 * nn : base + L.ogA, wd ? base + L.ogC0 : base + L.oG, gsig, ga, gdel);
        if (wd) {  // total dL/dC = g T_final + (through IPOT); ReLU mask; threshold partial  (= the tail of got_wd_bwd)
            const float g = d_out[0], thr = ws[L.g_thr + 6];
            const float* Tf = base + L.oWT + (WD_ITERS - 1) * nn;
            float* gC = base + L.ogC0;
            float s = 0.f;
            for (int e = c.tid; e < n * n; e += GNT) {
                const float gc = g * Tf[e] + gC[e];
                const float m = (base[L.oC0 + e] - thr > 0.f) ? gc : 0.f;
                gC[e] = m;
                s -= m;
            }
            s = block_sum(c, s);
            if (c.tid == 0) ws[L.g_gthr + (int64_t)b * 3 + 0] = s;
        }
    } else {
        gw_bwd_final(c, ws, L, bid);
    }
}


// STAGE 2 of the reverse chain for 128 < n <= 256 as its own kernel: the one-pass IPOT sweep (ipot_backward_h) with the last HLR rows of
// every lane's accumulator block in LDS.  blocks [0, k): the Gromov-Wasserstein sweep of outer iteration o; blocks [k, 2k) (mult == 2):
// the whole Wasserstein reverse of case bid - k (seed gT = g C formed inside the sweep; tail = ReLU mask + threshold partial).
template <int RPW, int QC, int HLR>
__global__ __launch_bounds__(GNT) void got_bwd_sweep_kernel(const GotBatch B, int o, int mult) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float ga[GOT_REGN], Rv[GOT_REGN], Cv[GOT_REGN];
    __shared__ float Hl[(HLR > 0 ? HLR * QC : 1) * GNT];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, mult, bid);
    float* ws = P.ws;
    const float* __restrict__ d_out = P.d_out;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    const bool wd = bid >= k;
    const int b = wd ? bid - k : bid;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n), nv = (int)up4(n);
    // one inlined copy of the sweep for both branches (see got_fwd_stage_kernel)
    ipot_backward_h<RPW, QC, HLR>(c, wd ? WD_INV_BETA : GW_INV_BETA, wd ? WD_ITERS : GW_INNER,
                                  wd ? base + L.oWT : base + L.oGT + o * GW_INNER * nn,
                                  wd ? base + L.oWd : base + L.oGd + o * GW_INNER * nv,
                                  wd ? base + L.oWs : base + L.oGs + o * (GW_INNER + 1) * nv, wd ? base + L.oC : base + L.ogT,
                                  wd ? d_out[0] : 1.f, wd ? base + L.ogC0 : base + L.oG, ga, Rv, Cv, Hl);
    if (wd) {  // total dL/dC = g T_final + (through IPOT); ReLU mask; threshold partial  (= the tail of got_wd_bwd)
        const float g = d_out[0], thr = ws[L.g_thr + 6];
        const float* Tf = base + L.oWT + (WD_ITERS - 1) * nn;
        float* gC = base + L.ogC0;
        float s = 0.f;
        for (int e = c.tid; e < n * n; e += GNT) {
            const float gc = g * Tf[e] + gC[e];
            const float m = (base[L.oC0 + e] - thr > 0.f) ? gc : 0.f;
            gC[e] = m;
            s -= m;
        }
        s = block_sum(c, s);
        if (c.tid == 0) ws[L.g_gthr + (int64_t)b * 3 + 0] = s;
    }
}

// The same sweep SPLIT over two workgroups per case and branch (see Xch; modes as in got_fwd_sweep_split_kernel): 32 accumulators per
// lane at n = 256, all in registers -- no LDS rows, no scratch.
template <int RPW, int QC>
__global__ __launch_bounds__(GNT) void got_bwd_sweep_split_kernel(const GotBatch B, int o, int mode) {
    __shared__ float smem[GOT_SMEM];
    __shared__ float ga[GOT_REGN], Rv[GOT_REGN], Cv[GOT_REGN];
    int bid = blockIdx.x;
    const GotProb P = got_pick(B, mode == 1 ? 4 : 2, bid);
    float* ws = P.ws;
    const float* __restrict__ d_out = P.d_out;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    const int half = bid & 1, u = bid >> 1;
    const bool wd = mode == 2 || (mode == 1 && u >= k);
    const int b = (mode == 1 && wd) ? u - k : u;
    float* base = ws + (int64_t)b * L.per_case;
    const int nn = (int)up4((int64_t)n * n), nv = (int)up4(n);
    Xch x = make_xch(ws, L, base, wd ? 1 : 0, half, wd ? 200 : 1 + 32 * o);
    ipot_backward_h<RPW, QC, 0, 2>(c, wd ? WD_INV_BETA : GW_INV_BETA, wd ? WD_ITERS : GW_INNER,
                                   wd ? base + L.oWT : base + L.oGT + o * GW_INNER * nn,
                                   wd ? base + L.oWd : base + L.oGd + o * GW_INNER * nv,
                                   wd ? base + L.oWs : base + L.oGs + o * (GW_INNER + 1) * nv, wd ? base + L.oC : base + L.ogT,
                                   wd ? d_out[0] : 1.f, wd ? base + L.ogC0 : base + L.oG, ga, Rv, Cv, nullptr, &x);
    if (wd) {  // total dL/dC = g T_final + (through IPOT); ReLU mask; threshold partial -- this half's rows, then the partner's partial
        const float g = d_out[0], thr = ws[L.g_thr + 6];
        const float* Tf = base + L.oWT + (WD_ITERS - 1) * nn;
        float* gC = base + L.ogC0;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int i = c.wave + GNW * (2 * r + half);
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                const int j = c.lane + 64 * q;
                if (i < n && j < n) {
                    const int e = i * n + j;
                    const float gc = g * Tf[e] + gC[e];
                    const float m = (base[L.oC0 + e] - thr > 0.f) ? gc : 0.f;
                    gC[e] = m;
                    s -= m;
                }
            }
        }
        s = block_sum_x(c, x, WD_ITERS + 1, s);
        if (c.tid == 0 && half == 0) ws[L.g_gthr + (int64_t)b * 3 + 0] = s;
    }
}

// K8: threshold gradients -> extrema gradients; tie counts for the local extrema (counted per case in the forward)
__global__ __launch_bounds__(64) void got_thr_bwd_kernel(const GotBatch B) {   // one block per problem
    const GotProb P = got_prob(B, blockIdx.x);
    float* ws = P.ws;
    float* __restrict__ d_minmax = P.d_mm;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const int tid = threadIdx.x;
    if (tid < 3) {
        float s = 0.f;
        for (int b = 0; b < k; ++b) s += ws[L.g_gthr + (int64_t)b * 3 + tid];
        ws[L.g_thr + 15 + tid] = s;
        // thr = min + beta (max - min): d/dmin = (1-beta) gthr ; d/dmax = beta gthr
        if (d_minmax) {
            d_minmax[2 * tid] = (1.f - THR_BETA) * s;
            d_minmax[2 * tid + 1] = THR_BETA * s;
        }
    }
    // LOCAL elements equal to each extremum (torch's min()/max() backward spreads the gradient evenly over ties)
    if (tid >= 8 && tid < 14) {
        const int m = tid - 8;
        float s = 0.f;
        for (int b = 0; b < k; ++b) s += ws[L.g_cnt + (int64_t)b * 6 + m];
        ws[L.g_thr + 9 + m] = s;
    }
}

// K9: raw-cost gradients (+ extrema routing) -> normalised-token gradients (matrix cores) -> dV, dQ
template <bool BIG>
__global__ __launch_bounds__(GNT) void got_cost_bwd_kernel(const GotBatch B) {
    __shared__ float smem[GOT_SMEM];
    // two workgroups per case: blocks [0, k) the V side (G0, Gs -> dV), blocks [k, 2k) the Q side (G0, Gt -> dQ).  Both need the routed
    // cross-cost gradient G0: each writes ITS copy into a scratch matrix (P1 / P2, free after the reverse chain), nobody touches G0
    int b = blockIdx.x;
    const GotProb P = got_pick(B, 2, b);
    const bool qside = b >= P.k;
    if (qside) b -= P.k;
    const float* __restrict__ V = P.V;
    const float* __restrict__ Q = P.Q;
    float* ws = P.ws;
    float* __restrict__ dV = P.dV;
    float* __restrict__ dQ = P.dQ;
    const float* __restrict__ d_minmax_in = P.d_mm_total;
    const int k = P.k, n = P.n, d = B.d;
    const GotWs L = got_layout(k, n, d);
    const Ctx c = make_ctx(n, smem);
    float* base = ws + (int64_t)b * L.per_case;
    const int N2 = n * n;
    const bool void_pass = ws[L.g_gen + 1] != 0.f;  // exchange time-out in the forward or the reverse sweeps (Xch): NaN gradients
    const float* G0in = base + L.ogC0;              // d/dC0
    float* G0 = base + (qside ? L.oP2 : L.oP1);     // this side's routed copy
    float* Gs = base + L.ogCs;    // d/dCs0
    float* Gt = base + L.ogCt;    // d/dCt0
    {
        // gradient of the six extrema, spread evenly over the (local) elements that attain them.  In global mode
        // (thresholds supplied by the caller) an extremum owned by another rank matches no local element.
        float gex[6], ex[6], cnt[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            ex[m] = ws[L.g_thr + m];
            cnt[m] = ws[L.g_thr + 9 + m];
            const float gthr = ws[L.g_thr + 15 + m / 2];
            const float gloc = (m & 1) ? THR_BETA * gthr : (1.f - THR_BETA) * gthr;
            gex[m] = d_minmax_in ? d_minmax_in[m] : gloc;
        }
        for (int e = c.tid; e < N2; e += GNT) {
            const float v0 = base[L.oC0 + e], v1 = base[L.oCs0 + e], v2 = base[L.oCt0 + e];
            float a = G0in[e];
            if (v0 == ex[0] && cnt[0] > 0.f) a += gex[0] / cnt[0];
            if (v0 == ex[1] && cnt[1] > 0.f) a += gex[1] / cnt[1];
            G0[e] = a;
            if (!qside) {
                float s = Gs[e];
                if (v1 == ex[2] && cnt[2] > 0.f) s += gex[2] / cnt[2];
                if (v1 == ex[3] && cnt[3] > 0.f) s += gex[3] / cnt[3];
                Gs[e] = s;
            } else {
                float t = Gt[e];
                if (v2 == ex[4] && cnt[4] > 0.f) t += gex[4] / cnt[4];
                if (v2 == ex[5] && cnt[5] > 0.f) t += gex[5] / cnt[5];
                Gt[e] = t;
            }
        }
        __syncthreads();
    }
    // C0_ij = 1 - <v^_i,q^_j>; Cs0_ij = 1 - <v^_i,v^_j>; Ct0_ij = 1 - <q^_i,q^_j>
    //   gv^_i = - sum_j G0_ij q^_j - sum_j (Gs_ij + Gs_ji) v^_j ;  gq^_j = - sum_i G0_ij v^_i - sum_i (Gt_ji + Gt_ij) q^_i
    const float* Vh = base + L.oVh;
    const float* Qh = base + L.oQh;
    float* gVh = base + L.ogVh;
    float* gQh = base + L.ogQh;
    if (!qside) {   // block-uniform
        mmx<BIG, false, false, !BIG>(c, n, d, n, G0, n, Qh, d, [&](int i, int e, float v) { gVh[i * d + e] = -v; });
        mmx<BIG, false, false, !BIG>(c, n, d, n, Gs, n, Vh, d, [&](int i, int e, float v) { gVh[i * d + e] -= v; });
        mmx<BIG, true, false, !BIG>(c, n, d, n, Gs, n, Vh, d, [&](int i, int e, float v) { gVh[i * d + e] -= v; });
    } else {
        mmx<BIG, true, false, !BIG>(c, n, d, n, G0, n, Vh, d, [&](int i, int e, float v) { gQh[i * d + e] = -v; });
        mmx<BIG, false, false, !BIG>(c, n, d, n, Gt, n, Qh, d, [&](int i, int e, float v) { gQh[i * d + e] -= v; });
        mmx<BIG, true, false, !BIG>(c, n, d, n, Gt, n, Qh, d, [&](int i, int e, float v) { gQh[i * d + e] -= v; });
    }
    // x^ = x / (r + eps):  gx = s gx^ - (<x^, gx^> / r) x^   (r = |x|, s = 1/(r+eps); r == 0 -> s gx^)
    for (int i = c.wave; i < n; i += GNW) {
        const bool isq = qside;
        const float* gx = (isq ? gQh : gVh) + i * d;
        const float* xh = (isq ? Qh : Vh) + i * d;
        float acc[2], dot = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = c.lane + 64 * u;
            acc[u] = (e < d) ? gx[e] : 0.f;
            if (e < d) dot += xh[e] * acc[u];
        }
        dot = wave_sum(dot);
        const float r = (base + (isq ? L.orQ : L.orV))[i];
        const float s = 1.f / (r + 1e-12f);
        const float proj = (r > 0.f) ? dot / r : 0.f;
        float* out = (isq ? dQ : dV) + ((int64_t)b * n + i) * d;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = c.lane + 64 * u;
            if (e < d) out[e] = void_pass ? __builtin_nanf("") : s * acc[u] - proj * xh[e];
        }
    }
}


// ---------------------------------------------------------------------------------------------------------
// launch sequences (a call gets here through got_run of got_host.hpp, which has checked it)
// ---------------------------------------------------------------------------------------------------------
// Every launch covers all problems of the batch: `mult` * sum_p k_p blocks (mult = blocks per case), one block per problem for the
// bookkeeping kernels.  The size class is the class of the LARGEST n in the batch (a class runs every smaller n).
static inline int batch_cases(const GotBatch& B) {
    int K = 0;
    for (int p = 0; p < B.np; ++p) K += B.p[p].k;
    return K;
}
static inline int batch_nmax(const GotBatch& B) {
    int n = 0;
    for (int p = 0; p < B.np; ++p) n = B.p[p].n > n ? B.p[p].n : n;
    return n;
}

static int launch_prep(const GotCall& call, hipStream_t s) {
    const GotBatch& B = call.b;
    const int K = batch_cases(B), n = batch_nmax(B);
    if (n > GOT_REGN) hipLaunchKernelGGL(got_prep_kernel<true>, dim3(K), dim3(GNT), 0, s, B);
    else hipLaunchKernelGGL(got_prep_kernel<false>, dim3(K), dim3(GNT), 0, s, B);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(got_minmax_kernel, dim3(B.np), dim3(64), 0, s, B);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

// the IPOT sweep launches of the per-phase classes (128 < n <= 256): blocks [0, K) the Gromov-Wasserstein sweep of outer iteration o,
// blocks [K, 2K) (mult == 2) the Wasserstein sweep.  n <= 192: 12 x 3 elements per lane (16 waves) -- no fourth, empty column group.
// (Round-5 null: the same sweeps as 512-thread workgroups -- 8 waves x 256 VGPRs, a lane's 32 x 4 accumulator block in registers --
// spill more, not less (616 B of scratch per lane against 288) and run slower: k = 32, n = 256 forward 3.85 vs 3.09 ms, backward 5.65 vs
// 4.65 ms.  What the 16-wave sweep of the 256 class still waits for is its scratch reloads: every one is an s_waitcnt vmcnt(0) in front
// of the plan rows in flight.)
// split sweeps (see Xch): only while every workgroup of the launch can be resident at once -- 2 K (4 K) workgroups <= compute units
// (of the calling thread's current device; cached per ordinal: 0 = not asked yet, -1 = the query failed)
static int device_cus() {
    constexpr int MAX_DEV = 64;
    static std::atomic<int> cache[MAX_DEV];
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return -1;
    int cus = cache[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        cus = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : -1;
        cache[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}
// size class of the launch chain for the largest n of a batch: 64 | 128 (one fused kernel), 192 | 256 (per-phase launches; the IPOT
// sweeps of 192 on 12 x 3 plan registers per lane), 512 (the workspace-resident class, n > GOT_REGN)
static int got_class(int n) {
    if (n <= 64) return 64;
    if (n <= 128) return 128;
    if (n > GOT_REGN) return 512;
    return (n <= 192 && !sw(MDL_SW_GOT_NO192)) ? 192 : 256;
}
static bool split_sweeps(int K, int cus) { return 2 * K <= cus && !sw(MDL_SW_GOT_NOSPLIT); }
static bool split_sweep_4k(int K, int cus) { return 4 * K <= cus; }   // both sweeps of a two-sweep step in ONE launch
static bool half_products(int K, int cus) { return 2 * K <= cus && !sw(MDL_SW_GOT_NO_HALF_PRODUCTS); }
template <class K3, class K4>
static void launch_split(K3 k3, K4 k4, const GotBatch& B, int K, int n, int o, int mult, hipStream_t s) {
    auto go = [&](int blocks, int mode) {
        if (n <= 192) hipLaunchKernelGGL(k3, dim3(blocks), dim3(GNT), 0, s, B, o, mode);
        else hipLaunchKernelGGL(k4, dim3(blocks), dim3(GNT), 0, s, B, o, mode);
    };
    if (mult == 1) go(2 * K, 0);
    else if (split_sweep_4k(K, device_cus())) go(4 * K, 1);
    else {          // both branches would not be resident together: the Wasserstein sweep as its own launch
        go(2 * K, 2);
        go(2 * K, 0);
    }
}
static int launch_fwd_sweep(const GotBatch& B, int o, int mult, hipStream_t s) {
    const int K = batch_cases(B), n = batch_nmax(B);
    constexpr int R = 256 / GNW, R3 = 192 / GNW;
    if (split_sweeps(K, device_cus())) {
        launch_split(got_fwd_sweep_split_kernel<R3 / 2, 3>, got_fwd_sweep_split_kernel<R / 2, 4>, B, K, n, o, mult, s);
        MDL_LAUNCH_CHECK();
        return MDL_OK;
    }
    if (got_class(n) == 192)
        hipLaunchKernelGGL((got_fwd_stage_kernel<R3, 3, 2>), dim3(mult * K), dim3(GNT), 0, s, B, o, mult);
    else
        hipLaunchKernelGGL((got_fwd_stage_kernel<R, 4, 2>), dim3(mult * K), dim3(GNT), 0, s, B, o, mult);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
static int launch_bwd_sweep(const GotBatch& B, int o, int mult, hipStream_t s) {
    const int K = batch_cases(B), n = batch_nmax(B);
    constexpr int R = 256 / GNW, R3 = 192 / GNW;
    if (split_sweeps(K, device_cus())) {
        launch_split(got_bwd_sweep_split_kernel<R3 / 2, 3>, got_bwd_sweep_split_kernel<R / 2, 4>, B, K, n, o, mult, s);
        MDL_LAUNCH_CHECK();
        return MDL_OK;
    }
    // accumulator rows in LDS: 2 of 12 (n <= 192), 7 of 16 (n <= 256)
    if (got_class(n) == 192)
        hipLaunchKernelGGL((got_bwd_sweep_kernel<R3, 3, MDL_GOT_HLR3>), dim3(mult * K), dim3(GNT), 0, s, B, o, mult);
    else
        hipLaunchKernelGGL((got_bwd_sweep_kernel<R, 4, MDL_GOT_HLR4>), dim3(mult * K), dim3(GNT), 0, s, B, o, mult);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int launch_main(const GotCall& call, hipStream_t s) {
    const GotBatch& B = call.b;
    const int K = batch_cases(B), c = got_class(batch_nmax(B));
    if (c == 64) {
        hipLaunchKernelGGL((got_main_kernel<64 / GNW, 1>), dim3(2 * K), dim3(GNT), 0, s, B);
    } else if (c == 128) {
        hipLaunchKernelGGL((got_main_kernel<128 / GNW, 2>), dim3(2 * K), dim3(GNT), 0, s, B);
    } else if (c == 512) {  // big class: one launch per phase, plans in the workspace
        hipLaunchKernelGGL((got_fwd_stage_kernel<1, 8, 0, true>), dim3(2 * K), dim3(GNT), 0, s, B, 0, 2);
        for (int o = 0; o < GW_OUTER; ++o) {
            hipLaunchKernelGGL((got_fwd_stage_kernel<1, 8, 1, true>), dim3(K), dim3(GNT), 0, s, B, o, 1);
            hipLaunchKernelGGL((got_fwd_stage_kernel<1, 8, 2, true>), dim3(o == 0 ? 2 * K : K), dim3(GNT), 0, s, B, o, o == 0 ? 2 : 1);
        }
        hipLaunchKernelGGL((got_fwd_stage_kernel<1, 8, 1, true>), dim3(K), dim3(GNT), 0, s, B, GW_OUTER, 1);
    } else {  // one launch per phase; the IPOT sweeps of n <= 192 on 12 x 3 plan registers per lane (no fourth column group)
        constexpr int R = 256 / GNW, R3 = 192 / GNW;
        hipLaunchKernelGGL((got_fwd_stage_kernel<R, 4, 0>), dim3(2 * K), dim3(GNT), 0, s, B, 0, 2);
        // the C_gamma products by row halves while two workgroups per case still fit the device (no exchange between the halves, so
        // unlike the split sweeps nothing depends on residency; MADELEINE_GOT_NO_HALF_PRODUCTS=1: A/B switch)
        const bool halves = half_products(K, device_cus());
        for (int o = 0; o < GW_OUTER; ++o) {
            if (halves) hipLaunchKernelGGL((got_fwd_stage_kernel<R, 4, 4>), dim3(2 * K), dim3(GNT), 0, s, B, o, 2);
            else hipLaunchKernelGGL((got_fwd_stage_kernel<R, 4, 1>), dim3(K), dim3(GNT), 0, s, B, o, 1);
            const int rc = launch_fwd_sweep(B, o, o == 0 ? 2 : 1, s);
            if (rc) return rc;
        }
        hipLaunchKernelGGL((got_fwd_stage_kernel<R, 4, 1>), dim3(K), dim3(GNT), 0, s, B, GW_OUTER, 1);
    }
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(got_sum_kernel, dim3(B.np), dim3(64), 0, s, B);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int launch_bwd_begin(const GotCall& call, hipStream_t s) {
    const GotBatch& B = call.b;
    const int K = batch_cases(B), c = got_class(batch_nmax(B));
    if (c == 64) {
        hipLaunchKernelGGL((got_main_bwd_kernel<64 / GNW, 1>), dim3(2 * K), dim3(GNT), 0, s, B);
    } else if (c == 128) {
        hipLaunchKernelGGL((got_main_bwd_kernel<128 / GNW, 2>), dim3(2 * K), dim3(GNT), 0, s, B);
    } else if (c == 512) {  // big class
        hipLaunchKernelGGL((got_bwd_stage_kernel<1, 8, 0, true>), dim3(K), dim3(GNT), 0, s, B, 0, 1);
        for (int o = GW_OUTER; o >= 0; --o) {
            hipLaunchKernelGGL((got_bwd_stage_kernel<1, 8, 1, true>), dim3(o >= 1 ? 2 * K : K), dim3(GNT), 0, s, B, o, o >= 1 ? 2 : 1);
            if (o >= 1) {
                const int with_wd = (o == GW_OUTER) ? 1 : 0;
                hipLaunchKernelGGL((got_bwd_stage_kernel<1, 8, 2, true>), dim3(with_wd ? 2 * K : K), dim3(GNT), 0, s, B, o - 1, with_wd ? 2 : 1);
            }
        }
        hipLaunchKernelGGL((got_bwd_stage_kernel<1, 8, 3, true>), dim3(K), dim3(GNT), 0, s, B, 0, 1);
    } else {  // one launch per phase
        constexpr int R = 256 / GNW, R3 = 192 / GNW;
        hipLaunchKernelGGL((got_bwd_stage_kernel<R, 4, 0>), dim3(K), dim3(GNT), 0, s, B, 0, 1);
        for (int o = GW_OUTER; o >= 0; --o) {
            hipLaunchKernelGGL((got_bwd_stage_kernel<R, 4, 1>), dim3(o >= 1 ? 2 * K : K), dim3(GNT), 0, s, B, o, o >= 1 ? 2 : 1);   // two halves per case
            if (o >= 1) {
                const int with_wd = (o == GW_OUTER) ? 1 : 0;
                const int mult = with_wd ? 2 : 1;
                const int rc = launch_bwd_sweep(B, o - 1, mult, s);
                if (rc) return rc;
            }
        }
        hipLaunchKernelGGL((got_bwd_stage_kernel<R, 4, 3>), dim3(K), dim3(GNT), 0, s, B, 0, 1);
    }
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(got_thr_bwd_kernel, dim3(B.np), dim3(64), 0, s, B);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int launch_bwd_finish(const GotCall& call, hipStream_t s) {
    const GotBatch& B = call.b;
    const int K = batch_cases(B), n = batch_nmax(B);
    if (n > GOT_REGN) hipLaunchKernelGGL(got_cost_bwd_kernel<true>, dim3(2 * K), dim3(GNT), 0, s, B);   // V side | Q side of every case
    else hipLaunchKernelGGL(got_cost_bwd_kernel<false>, dim3(2 * K), dim3(GNT), 0, s, B);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

static int64_t ws_floats(int k, int n, int, int d) { return got_layout(k, n, d).g_cases; }

// mdl_dispatch_plan (dispatch_plan.hip): the class, row-half products and split sweeps launch_main / launch_bwd_begin choose for K cases
// of largest size n on a device of `cus` compute units
static int plan(int K, int n, int, int cus, int64_t* o) {
    const int c = got_class(n);
    const bool phased = c == 192 || c == 256;
    o[MDL_PLAN_VARIANT] = c;
    o[MDL_PLAN_PERSIST] = phased && half_products(K, cus) ? 1 : 0;
    o[MDL_PLAN_EXTRA] = phased && split_sweeps(K, cus) ? (split_sweep_4k(K, cus) ? 2 : 1) : 0;
    o[MDL_PLAN_SPLITS] = 1;
    return MDL_OK;
}

static int launch_fwd(const GotCall& call, hipStream_t s) {
    if (const int rc = launch_prep(call, s)) return rc;
    return launch_main(call, s);
}
}  // namespace got1024

// the resident row of the engine table (got_host.hpp): Q has the n tokens of V; a _multi call stays within the register classes
const GotEngine& got_resident_engine() {
    using namespace got1024;
    static const GotEngine e = {GOT_BIGN, GOT_BIGN, GOT_MAXD, GOT_MAXP, GOT_REGN, ws_floats,
                                {launch_prep, launch_fwd, launch_bwd_begin, launch_bwd_finish}, plan};
    return e;
}
}  // namespace mdl
