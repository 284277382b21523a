// resample.hip -- the test-set bootstrap of the probes' metrics (B1-B3 of include/madeleine_amd_stats.h): resampling weights from the
// counter hash, and per (problem, replicate) the weighted confusion matrix, the weighted Mann-Whitney numerators and the weighted
// concordance counts.  Exact integer arithmetic throughout: the sums are the same whatever the order of the atomic additions.
//
//   boot_weights_kernel   one workgroup per (group, replicate): the S draws as LDS atomics on uint16 pairs, then the counts to global.
//   boot_prepare_kernel   one workgroup per problem: test class and prediction of every case in one byte, for C > 2 the fp64 log-softmax
//                         scores (probe_common.hpp: the code of probe_prepare_kernel), the test-set size and the NaN flag.
//   boot_rank_kernel      O(S^2) counting once per problem and class, a thread per test case: lt = #{score below}, eq = #{score equal},
//                         and the case's position lt + #{equal, lower case index} in the total order; writes the order and the bounds
//                         [lt, lt + eq) of the tie group at that position.
//   boot_class_kernel     one workgroup per (problem, BT_RB replicates).  Per replicate: the draws, the weighted confusion matrix as LDS
//                         atomics, and per class a prefix sum of the outside weights along the order (a contiguous run of positions per
//                         thread, a wave scan, the four wave totals), then per case of the class w (2 below + tied) read from the prefix.
//   boot_surv_kernel      one workgroup per (problem, BT_RB replicates), the problem's cases in LDS: per replicate the draws and the
//                         O(S^2) weighted pair count of mdl_surv_metrics' rule.
// No workgroup waits on another; every loop has a bound that is an argument or a constant of the headers.
#include "probe_host.hpp"

#include "../../include/madeleine_amd_stats.h"

namespace mdl {
namespace {

constexpr int BT_THREADS = 256;
constexpr int BT_WAVES = BT_THREADS / WAVE;
constexpr int BT_RB = MDL_BOOT_REP_BLOCK;
constexpr int BT_CMAX = PROBE_CMAX;
constexpr int BT_SURV = MDL_BOOT_SURV_MAX_TEST;
constexpr uint32_t BT_GOLDEN = 0x9E3779B9U;
constexpr size_t BT_LDS_DEFAULT = 48 * 1024;       // dynamic LDS a kernel may ask for without raising its limit
static_assert(MDL_PROBE_MAX_CASES < 65536, "a count has to fit half a word");
static_assert(BT_CMAX == 8, "class and prediction share a byte, three bits each");

__host__ __device__ __forceinline__ int words_of(int S) { return (S + 1) / 2; }
inline uint32_t key_of(uint64_t seed) { return (uint32_t)(seed * 0x9E3779B97F4A7C15ULL >> 32) ^ (uint32_t)seed; }
// dynamic LDS of boot_class_kernel: the count words and the uint16 prefix over S + 1 positions
inline size_t class_lds(int S) { return 4 * (size_t)words_of(S) + 4 * (size_t)words_of(S + 1); }
static_assert(4 * ((MDL_BOOT_LDS_RAISE_FROM - 1 + 1) / 2) + 4 * ((MDL_BOOT_LDS_RAISE_FROM + 1) / 2) == BT_LDS_DEFAULT &&
                  4 * ((MDL_BOOT_LDS_RAISE_FROM + 1) / 2) + 4 * ((MDL_BOOT_LDS_RAISE_FROM + 2) / 2) > BT_LDS_DEFAULT,
              "MDL_BOOT_LDS_RAISE_FROM is the first S whose dynamic LDS exceeds the default limit");

__device__ __forceinline__ uint32_t group_key(uint32_t key, int32_t g) { return mix32(key ^ ((uint32_t)g * BT_GOLDEN)); }
__device__ __forceinline__ uint32_t weight_of(const uint32_t* s_cnt, int s) { return (s_cnt[s >> 1] >> ((s & 1) << 4)) & 0xFFFFu; }

// The weights of replicate r into s_cnt (uint16 pairs; words_of(S) words): all ones for r == 0, else the counts of the S draws.  Fields
// cannot carry: a count is at most S < 65536.  Ends on a barrier.
__device__ __forceinline__ void fill_weights(uint32_t* s_cnt, int S, uint32_t a, uint32_t r) {
    const int tid = threadIdx.x, words = words_of(S);
    for (int w = tid; w < words; w += BT_THREADS) s_cnt[w] = r == 0 ? 0x00010001u : 0u;
    __syncthreads();
    if (r != 0) {
        const uint32_t b = mix32(a + r);
        for (int j = tid; j < S; j += BT_THREADS) {
            const uint32_t h = mix32(mix32(b ^ (uint32_t)j) + (uint32_t)j * BT_GOLDEN);
            const uint32_t draw = (uint32_t)(((uint64_t)h * (uint32_t)S) >> 32);        // < S
            atomicAdd(&s_cnt[draw >> 1], 1u << ((draw & 1) << 4));
        }
        __syncthreads();
    }
}

// sum of one 64-bit value per thread over the workgroup; thread 0 holds it.  One barrier; s_red is free again after the caller's next one.
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(BT_THREADS) void boot_weights_kernel(uint32_t key, const int32_t* __restrict__ group, int reps, int S,
                                                                  uint16_t* __restrict__ w_out) {
    extern __shared__ uint32_t s_dyn[];
    const int g = blockIdx.x / reps, r = blockIdx.x % reps;
    fill_weights(s_dyn, S, group_key(key, group[g]), (uint32_t)r);
    uint16_t* out = w_out + (int64_t)blockIdx.x * S;
    for (int s = threadIdx.x; s < S; s += BT_THREADS) out[s] = (uint16_t)weight_of(s_dyn, s);
}

// ---- classification ---------------------------------------------------------------------------------------------------------------
// workspace: score [P][C][S] double (C > 2 only), ord [P][ncls][S] uint32 (case index | in-class << 15 at every position of the order),
// bnd [P][ncls][S] uint32 (tie group [lo, hi) of the position: lo | hi << 16), meta [P][2] int32 (test cases, NaN flag), code [P][S16]
// int8 (-1: not a test case; else class | prediction << 3)
struct BootWs {
    double* score;
    uint32_t* ord;
    uint32_t* bnd;
    int32_t* meta;
    int8_t* code;
};
inline int64_t boot_ws_bytes(int64_t P, int64_t S, int C, BootWs* m, void* ws) {
    const int64_t ncls = cols_of(C);
    const int64_t b_score = C > 2 ? P * C * S * 8 : 0, b_ord = up16(P * ncls * S * 4), b_meta = up16(P * 8);
    if (m) {
        char* base = reinterpret_cast<char*>(ws);
        m->score = reinterpret_cast<double*>(base);
        m->ord = reinterpret_cast<uint32_t*>(base + b_score);
        m->bnd = reinterpret_cast<uint32_t*>(base + b_score + b_ord);
        m->meta = reinterpret_cast<int32_t*>(base + b_score + 2 * b_ord);
        m->code = reinterpret_cast<int8_t*>(base + b_score + 2 * b_ord + b_meta);
    }
    return up16(b_score) + 2 * b_ord + b_meta + P * s16_of(S);
}

__global__ __launch_bounds__(BT_THREADS) void boot_prepare_kernel(const float* __restrict__ z, const int32_t* __restrict__ y, int64_t ldy,
                                                                  const int32_t* __restrict__ train_idx,
                                                                  const int32_t* __restrict__ n_train, int n_max, int S, int C, BootWs m,
                                                                  int64_t S16) {
    __shared__ int s_meta[2];
    const int tid = threadIdx.x, p = blockIdx.x, cols = cols_of(C);
    int8_t* code = m.code + (int64_t)p * S16;
    const int32_t* yp = y + (int64_t)p * ldy;
    if (tid < 2) s_meta[tid] = 0;
    for (int s = tid; s < S; s += BT_THREADS) code[s] = probe_test_class(yp[s], C);
    __syncthreads();
    strike_training<BT_THREADS>(code, train_idx, n_train, p, n_max, S);
    __syncthreads();
    int n_test = 0, nan = 0;
    for (int s = tid; s < S; s += BT_THREADS) {
        const int t = code[s];
        if (t < 0) continue;
        const float* zs = z + ((int64_t)p * S + s) * cols;
        double* sc = m.score + (int64_t)p * C * S + s;
        const int pred = probe_predict(zs, cols, sc, S);
        if (cols == 1) {
            nan |= zs[0] != zs[0];
        } else {
            for (int c = 0; c < cols; ++c) nan |= sc[(int64_t)c * S] != sc[(int64_t)c * S];
        }
        code[s] = (int8_t)(t | (pred << 3));
        ++n_test;
    }
    if (n_test) atomicAdd(&s_meta[0], n_test);
    if (nan) atomicOr(&s_meta[1], 1);
    __syncthreads();
    if (tid < 2) m.meta[(int64_t)p * 2 + tid] = s_meta[tid];
}

__global__ __launch_bounds__(BT_THREADS) void boot_rank_kernel(const float* __restrict__ z, int S, int C, int slices, BootWs m, int64_t S16) {
    __shared__ double s_sc[BT_THREADS];
    __shared__ int s_ok[BT_THREADS];
    const int tid = threadIdx.x;
    const int ncls = cols_of(C);
    const int slice = blockIdx.x % slices, rest = blockIdx.x / slices;
    const int ci = rest % ncls, p = rest / ncls;
    if (m.meta[(int64_t)p * 2 + 1]) return;            // a NaN among the test scores: no order, and nobody reads one
    const int cpos = C == 2 ? 1 : ci;
    const int8_t* code = m.code + (int64_t)p * S16;
    const double* sc = m.score + ((int64_t)p * C + ci) * S;
    const float* zp = z + (int64_t)p * S;              // C == 2: cols = 1
    const int i = slice * BT_THREADS + tid;
    const bool mine = i < S && code[i] >= 0;
    if (!__syncthreads_or(mine ? 1 : 0)) return;
    const double my = mine ? (C == 2 ? (double)zp[i] : sc[i]) : 0.0;
    int lt = 0, eq = 0, eqb = 0;
    for (int j0 = 0; j0 < S; j0 += BT_THREADS) {
        const int j = j0 + tid;
        const int ok = (j < S && code[j] >= 0) ? 1 : 0;
        s_sc[tid] = ok ? (C == 2 ? (double)zp[j] : sc[j]) : 0.0;
        s_ok[tid] = ok;
        __syncthreads();
        if (mine) {
            const int lim = S - j0 < BT_THREADS ? S - j0 : BT_THREADS;
            for (int jj = 0; jj < lim; ++jj) {
                if (!s_ok[jj]) continue;
                const double v = s_sc[jj];
                const int e = v == my ? 1 : 0;          // -0 == +0
                lt += v < my ? 1 : 0;
                eq += e;
                eqb += (e && j0 + jj < i) ? 1 : 0;
            }
        }
        __syncthreads();
    }
    if (mine) {                                          // no NaN: (score, case index) is a total order, pos a permutation of [0, n_test)
        const int64_t at = ((int64_t)p * ncls + ci) * S + lt + eqb;
        m.ord[at] = (uint32_t)i | (((code[i] & 7) == cpos ? 1u : 0u) << 15);
        m.bnd[at] = (uint32_t)lt | ((uint32_t)(lt + eq) << 16);
    }
}

__global__ __launch_bounds__(BT_THREADS) void boot_class_kernel(int S, int C, const int32_t* __restrict__ group, uint32_t key, int reps,
                                                                int nblk, BootWs m, int64_t S16, int32_t* __restrict__ confusion,
                                                                int64_t* __restrict__ auc_num) {
    extern __shared__ uint32_t s_dyn[];
    __shared__ int s_conf[BT_CMAX * BT_CMAX];
    __shared__ uint32_t s_wtot[BT_WAVES];
    __shared__ unsigned long long s_red[BT_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int p = blockIdx.x / nblk, r0 = (blockIdx.x % nblk) * BT_RB;
    const int r1 = r0 + BT_RB < reps ? r0 + BT_RB : reps;
    const int ncls = cols_of(C);
    uint32_t* s_cnt = s_dyn;
    uint16_t* s_pre = reinterpret_cast<uint16_t*>(s_dyn + words_of(S));      // S + 1 entries: a prefix is at most the sum of w = S
    const int8_t* code = m.code + (int64_t)p * S16;
    const int n = m.meta[(int64_t)p * 2], nan = m.meta[(int64_t)p * 2 + 1];
    const uint32_t a = group_key(key, group[p]);
    const int chunk = (n + BT_THREADS - 1) / BT_THREADS;
    const int lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    for (int r = r0; r < r1; ++r) {
        if (tid < BT_CMAX * BT_CMAX) s_conf[tid] = 0;
        fill_weights(s_cnt, S, a, (uint32_t)r);
        for (int s = tid; s < S; s += BT_THREADS) {
            const int c = code[s];
            if (c < 0) continue;
            const uint32_t w = weight_of(s_cnt, s);
            if (w) atomicAdd(&s_conf[(c & 7) * C + (c >> 3)], (int)w);
        }
        int64_t* out = auc_num + ((int64_t)p * reps + r) * ncls;
        for (int ci = 0; ci < ncls; ++ci) {
            if (nan) {
                if (tid == 0) out[ci] = -1;
                continue;
            }
            const uint32_t* ord = m.ord + ((int64_t)p * ncls + ci) * S;
            const uint32_t* bnd = m.bnd + ((int64_t)p * ncls + ci) * S;
            uint32_t local = 0;
            for (int q = lo; q < hi; ++q) {
                const uint32_t o = ord[q];
                local += (o >> 15) ? 0u : weight_of(s_cnt, (int)(o & 0x7FFFu));
            }
            uint32_t inc = local;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (lane == WAVE - 1) s_wtot[wave] = inc;
            __syncthreads();
            uint32_t run = inc - local;
            for (int w = 0; w < wave; ++w) run += s_wtot[w];
            for (int q = lo; q < hi; ++q) {
                const uint32_t o = ord[q];
                s_pre[q] = (uint16_t)run;
                run += (o >> 15) ? 0u : weight_of(s_cnt, (int)(o & 0x7FFFu));
            }
            if (tid == BT_THREADS - 1) s_pre[n] = (uint16_t)run;       // the last thread's run ends at n, or is empty and starts there
            __syncthreads();
            unsigned long long acc = 0;
            for (int q = tid; q < n; q += BT_THREADS) {
                const uint32_t o = ord[q];
                if (!(o >> 15)) continue;
                const uint32_t b = bnd[q];
                const uint32_t below = s_pre[b & 0xFFFFu], tied = (uint32_t)s_pre[b >> 16] - below;
                acc += (unsigned long long)weight_of(s_cnt, (int)(o & 0x7FFFu)) * (2u * below + tied);
            }
            acc = block_sum_u64(acc, s_red);
            if (tid == 0) out[ci] = (int64_t)acc;
        }
        __syncthreads();
        if (tid < C * C) confusion[((int64_t)p * reps + r) * C * C + tid] = s_conf[tid];
        __syncthreads();
    }
}

// ---- survival ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT_THREADS) void boot_surv_kernel(const float* __restrict__ z, const float* __restrict__ time, int64_t ldt,
                                                               const int32_t* __restrict__ event, int64_t lde,
                                                               const int32_t* __restrict__ train_idx, const int32_t* __restrict__ n_train,
                                                               int n_max, int S, const int32_t* __restrict__ group, uint32_t key, int reps,
                                                               int nblk, int64_t* __restrict__ counts) {
    __shared__ float s_z[BT_SURV], s_t[BT_SURV];
    __shared__ uint32_t s_cnt[BT_SURV / 2];
    __shared__ int8_t s_c[BT_SURV];                      // -1: not a test case, else the event flag
    __shared__ unsigned long long s_red[2][BT_WAVES];
    const int tid = threadIdx.x;
    const int p = blockIdx.x / nblk, r0 = (blockIdx.x % nblk) * BT_RB;
    const int r1 = r0 + BT_RB < reps ? r0 + BT_RB : reps;
    const int32_t* ep = event + (int64_t)p * lde;
    const float* tp = time + (int64_t)p * ldt;
    for (int i = tid; i < S; i += BT_THREADS) {
        const int ev = ep[i];
        s_c[i] = (ev == 0 || ev == 1) ? (int8_t)ev : (int8_t)-1;
        s_z[i] = z[(int64_t)p * S + i];
        s_t[i] = tp[i];
    }
    __syncthreads();
    strike_training<BT_THREADS>(s_c, train_idx, n_train, p, n_max, S);
    __syncthreads();
    const uint32_t a = group_key(key, group[p]);
    for (int r = r0; r < r1; ++r) {
        fill_weights(s_cnt, S, a, (uint32_t)r);
        unsigned long long num = 0, comp = 0;
        for (int i = tid; i < S; i += BT_THREADS) {
            if (s_c[i] != 1) continue;                   // a test case with an event
            const uint32_t wi = weight_of(s_cnt, i);
            if (!wi) continue;
            const float zi = s_z[i], ti = s_t[i];
            uint32_t ln = 0, lc = 0;                      // at most 2 S and S
            for (int j = 0; j < S; ++j) {
                const int cj = s_c[j];
                if (cj < 0) continue;
                const float tj = s_t[j], zj = s_z[j];
                if (ti < tj || (ti == tj && !cj)) {
                    const uint32_t wj = weight_of(s_cnt, j);
                    lc += wj;
                    ln += wj * (zi > zj ? 2u : (zi == zj ? 1u : 0u));
                }
            }
            num += (unsigned long long)wi * ln;
            comp += (unsigned long long)wi * lc;
        }
        num = block_sum_u64(num, s_red[0]);
        comp = block_sum_u64(comp, s_red[1]);
        if (tid == 0) {
            counts[((int64_t)p * reps + r) * 2] = (int64_t)num;
            counts[((int64_t)p * reps + r) * 2 + 1] = (int64_t)comp;
        }
        __syncthreads();
    }
}

// the limits of the entry points: {n_max, d, S, fit, classes}
constexpr ProbeLimits BOOT_CLASS = {MDL_LOGIT_MAX_TRAIN, PROBE_NO_LIMIT, MDL_PROBE_MAX_CASES, false, true};
constexpr ProbeLimits BOOT_SURV = {MDL_COX_MAX_TRAIN, PROBE_NO_LIMIT, BT_SURV, false, false};

inline int64_t rep_blocks(int64_t R) { return R / BT_RB + 1; }      // ceil((R + 1) / BT_RB) workgroups per problem, for any R >= 0

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int mdl_boot_weights(uint64_t seed, const int32_t* group, int64_t G, int64_t R, int64_t S, uint16_t* w_out, void* stream) {
    if (!all_given(group, w_out)) return MDL_E_ARG;
    if (G < 1 || S < 1 || R < 0) return MDL_E_ARG;
    if (R > 0x7FFFFFFE || S > MDL_PROBE_MAX_CASES || !mul_i32(G, R + 1)) return MDL_E_UNSUPPORTED;
    if (!aligned_to(group, 4) || !aligned_to(w_out, 2)) return MDL_E_ALIGN;
    const int64_t reps = R + 1;
    hipLaunchKernelGGL(boot_weights_kernel, dim3((unsigned)(G * reps)), dim3(BT_THREADS), 4 * (size_t)words_of((int)S), (hipStream_t)stream,
                       key_of(seed), group, (int)reps, (int)S, w_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int64_t mdl_boot_class_ws_bytes(int64_t P, int64_t S, int C) {
    if (const int rc = probe_check(probe_sizes(P, 1, S, C, 0), BOOT_CLASS, nullptr)) return rc;
    return boot_ws_bytes(P, S, C, nullptr, nullptr);
}

extern "C" int mdl_boot_class_counts(const float* z, const int32_t* y, int64_t ldy, const int32_t* train_idx, const int32_t* n_train,
                                     int64_t P, int n_max, int64_t S, int C, const int32_t* group, uint64_t seed, int64_t R,
                                     int32_t* confusion_out, int64_t* auc_num_out, void* ws, void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{y, ldy}}, 1, C, 0};
    const int ncls = cols_of(C);
    const int64_t slices = ceil_div(S, BT_THREADS), nblk = rep_blocks(R);
    const ProbeExtra extra = {all_given(z, group, confusion_out, auc_num_out, ws), mul_i32(P, ncls, slices) && mul_i32(P, nblk),
                              host_aligned16(ws) && aligned_to(auc_num_out, 8) && all_aligned(4, z, y, train_idx, n_train, group, confusion_out),
                              R};
    if (const int rc = probe_check(t, BOOT_CLASS, &extra)) return rc;
    const int64_t reps = R + 1;
    const size_t lds = class_lds((int)S);
    if (lds > BT_LDS_DEFAULT) {                          // S >= MDL_BOOT_LDS_RAISE_FROM: the kernel's limit is raised to its largest need
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&boot_class_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)class_lds(MDL_PROBE_MAX_CASES));
        if (e != hipSuccess) return (int)e;
    }
    BootWs m;
    boot_ws_bytes(P, S, C, &m, ws);
    const int64_t S16 = s16_of(S);
    hipLaunchKernelGGL(boot_prepare_kernel, dim3((unsigned)P), dim3(BT_THREADS), 0, (hipStream_t)stream, z, y, ldy, train_idx, n_train, n_max,
                       (int)S, C, m, S16);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(boot_rank_kernel, dim3((unsigned)(P * ncls * slices)), dim3(BT_THREADS), 0, (hipStream_t)stream, z, (int)S, C,
                       (int)slices, m, S16);
    MDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(boot_class_kernel, dim3((unsigned)(P * nblk)), dim3(BT_THREADS), lds, (hipStream_t)stream, (int)S, C, group,
                       key_of(seed), (int)reps, (int)nblk, m, S16, confusion_out, auc_num_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int mdl_boot_surv_counts(const float* z, const float* time, int64_t ldt, const int32_t* event, int64_t lde,
                                    const int32_t* train_idx, const int32_t* n_train, int64_t P, int n_max, int64_t S, const int32_t* group,
                                    uint64_t seed, int64_t R, int64_t* counts_out, void* stream) {
    const ProbeTable t = {train_idx, n_train, P, n_max, S, {{time, ldt}, {event, lde}}, 2, 0, 0};
    const int64_t nblk = rep_blocks(R);
    const ProbeExtra extra = {all_given(z, group, counts_out), mul_i32(P, nblk),
                              aligned_to(counts_out, 8) && all_aligned(4, z, time, event, train_idx, n_train, group), R};
    if (const int rc = probe_check(t, BOOT_SURV, &extra)) return rc;
    const int64_t reps = R + 1;
    hipLaunchKernelGGL(boot_surv_kernel, dim3((unsigned)(P * nblk)), dim3(BT_THREADS), 0, (hipStream_t)stream, z, time, ldt, event, lde,
                       train_idx, n_train, n_max, (int)S, group, key_of(seed), (int)reps, (int)nblk, counts_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
