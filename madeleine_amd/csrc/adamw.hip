// adamw.hip -- multi-tensor fp32 AdamW with a device-side non-finite guard and in-stream gradient-norm clipping (O1 of the header).
//
// One optimiser step is a fixed sequence of launches per set of <= MDL_ADAMW_MAX_TENSORS tensors, whatever the outcome:
//   adamw_stats_kernel   (only with the guard or clipping)  reads every gradient once; workgroup b writes {sum of squares, "saw a
//                        non-finite element"} to slot b of the launch's MDL_ADAMW_STAT_BLOCKS slots -- every slot, every time.
//   adamw_update_kernel  every workgroup merges ALL slots of the step (all launches, all parameter groups) in one fixed order, so every
//                        workgroup of every launch holds the same bits: the verdict and the clip coefficient.  Void step: return.
//                        Otherwise p, exp_avg, exp_avg_sq are updated; the gradients and `step` are only read.
//   adamw_commit_kernel  one thread per tensor: step += 1 unless the step is void.  A launch of its own, so that no workgroup of the
//                        update can still be reading the old value.  The last commit of the step also writes the global norm and bumps
//                        the skipped-step counter.
// The tensors' addresses travel BY VALUE in the kernel arguments (2.3 KB for 48 tensors): gradient addresses change every step under
// zero_grad(set_to_none=True), and a device-resident table would need an upload per step.
// Hyperparameters arrive as the bit patterns of doubles and every derived scalar (1 - lr wd, 1 - beta, the bias corrections) is formed
// in double and rounded to fp32 ONCE, as torch does on the host: 1 - fl32(0.999) is 4.7e-5 off 1 - 0.999.
#include "common.hpp"

namespace mdl {
namespace {

constexpr int AW_MAXT = MDL_ADAMW_MAX_TENSORS;
constexpr int AW_THREADS = 256;
constexpr int AW_VEC = 4;                                   // 16-byte accesses per thread and pass
constexpr int AW_CHUNK = AW_THREADS * 4 * AW_VEC;           // 4096 elements: one workgroup pass
constexpr int AW_STAT_BLOCKS = MDL_ADAMW_STAT_BLOCKS;
constexpr int AW_MAX_BLOCKS = 2048;                         // update grid cap; further chunks are grid-strided
static_assert(AW_THREADS >= AW_MAXT, "the commit kernel gives one thread to each tensor");

struct StatTable {
    const float* g[AW_MAXT];
    int64_t numel[AW_MAXT];
};
struct UpdTable {
    float* p[AW_MAXT];
    const float* g[AW_MAXT];
    float* m[AW_MAXT];
    float* v[AW_MAXT];
    const float* step[AW_MAXT];
    int64_t numel[AW_MAXT];
};
struct StepTable {
    float* step[AW_MAXT];
};
struct Hyper {
    uint64_t lr, beta1, beta2, eps, wd, max_norm;   // bit patterns of doubles
};

__host__ __device__ __forceinline__ int64_t chunks_of(int64_t numel) { return (numel + AW_CHUNK - 1) / AW_CHUNK; }
__device__ __forceinline__ double as_double(uint64_t bits) { return __builtin_bit_cast(double, bits); }

// Chunk c of the launch's chunk sequence (tensor 0's chunks, then tensor 1's, ...): advances the cursor (ti, first chunk of ti) to the
// tensor that holds it.  c only grows inside a workgroup, so the cursor never moves back.  False past the last chunk; tensors of zero
// elements own no chunk and are stepped over.
template <class Table>
__device__ __forceinline__ bool seek(const Table& tab, int nt, int64_t c, int& ti, int64_t& first) {
    while (ti < nt) {
        const int64_t nch = chunks_of(tab.numel[ti]);
        if (c < first + nch) return true;
        first += nch;
        ++ti;
    }
    return false;
}

__device__ __forceinline__ void stat_acc(float x, float& acc, uint32_t& mx) {
    acc = fmaf(x, x, acc);
    const uint32_t a = __builtin_bit_cast(uint32_t, x) & 0x7FFFFFFFu;   // |x| as an integer: inf and every NaN are >= 0x7F800000
    mx = a > mx ? a : mx;
}

__global__ __launch_bounds__(AW_THREADS) void adamw_stats_kernel(StatTable tab, int nt, float2* __restrict__ part) {
    const int tid = threadIdx.x;
    float acc = 0.f;
    uint32_t mx = 0;
    int ti = 0;
    int64_t first = 0;
    for (int64_t c = blockIdx.x; seek(tab, nt, c, ti, first); c += gridDim.x) {
        const int64_t base = (c - first) * AW_CHUNK;
        const int64_t left = tab.numel[ti] - base;
        const int cnt = left < AW_CHUNK ? (int)left : AW_CHUNK;
        const float* g = tab.g[ti] + base;      // base is a multiple of 4096 elements: the chunk is aligned as the tensor is
        if (aligned16(g)) {
            if (cnt == AW_CHUNK) {
                f32x4 x[AW_VEC];
#pragma unroll
                for (int u = 0; u < AW_VEC; ++u) x[u] = ld4(g + (u * AW_THREADS + tid) * 4);
#pragma unroll
                for (int u = 0; u < AW_VEC; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) stat_acc(x[u][j], acc, mx);
            } else {
                for (int e = tid * 4; e < cnt; e += AW_THREADS * 4) {
                    if (e + 4 <= cnt) {
                        const f32x4 x = ld4(g + e);
#pragma unroll
                        for (int j = 0; j < 4; ++j) stat_acc(x[j], acc, mx);
                    } else {
                        for (int j = e; j < cnt; ++j) stat_acc(g[j], acc, mx);
                    }
                }
            }
        } else {                                 // 4-byte alignment is all a gradient view promises
            if (cnt == AW_CHUNK) {
                float x[4 * AW_VEC];
#pragma unroll
                for (int u = 0; u < 4 * AW_VEC; ++u) x[u] = g[u * AW_THREADS + tid];
#pragma unroll
                for (int u = 0; u < 4 * AW_VEC; ++u) stat_acc(x[u], acc, mx);
            } else {
                for (int e = tid; e < cnt; e += AW_THREADS) stat_acc(g[e], acc, mx);
            }
        }
    }
    // fixed-order workgroup sum: xor butterflies inside the wave, then the four waves left to right
    __shared__ float s_acc[AW_THREADS / WAVE];
    __shared__ uint32_t s_mx[AW_THREADS / WAVE];
    acc = wave_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((tid & (WAVE - 1)) == 0) {
        s_acc[tid / WAVE] = acc;
        s_mx[tid / WAVE] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        float s = s_acc[0];
        uint32_t m = s_mx[0];
#pragma unroll
        for (int w = 1; w < AW_THREADS / WAVE; ++w) {
            s += s_acc[w];
            m = s_mx[w] > m ? s_mx[w] : m;
        }
        part[blockIdx.x] = make_float2(s, m >= 0x7F800000u ? 1.f : 0.f);
    }
}

// Every slot of the step, merged in one fixed order by a whole workgroup: thread t takes slots t, t + 256, ... in double, xor butterflies,
// then the four waves left to right.  Every thread returns the same (sum of squares, verdict); the same bits in every workgroup.
__device__ __forceinline__ void merge_partials(const float2* __restrict__ part, int np, double& sumsq, bool& bad) {
    __shared__ double s_sum[AW_THREADS / WAVE];
    __shared__ int s_bad[AW_THREADS / WAVE];
    const int tid = threadIdx.x;
    double s = 0.0;
    int b = 0;
    for (int i = tid; i < np; i += AW_THREADS) {
        const float2 x = part[i];
        s += (double)x.x;
        b |= (x.y != 0.f) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        b |= __shfl_xor(b, o, 64);
    }
    if ((tid & (WAVE - 1)) == 0) {
        s_sum[tid / WAVE] = s;
        s_bad[tid / WAVE] = b;
    }
    __syncthreads();
    sumsq = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    bad = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) != 0;
}

// clip_grad_norm_'s coefficient, in fp32 as torch forms it from its fp32 total norm
__device__ __forceinline__ float clip_coef(double sumsq, double max_norm) {
    const float norm = (float)sqrt(sumsq);
    return fminf(1.f, (float)max_norm / (norm + 1e-6f));
}

// base^k for an integer k >= 0 by squaring, in double (a few ulp of a double, far below the fp32 rounding that follows)
__device__ __forceinline__ double powi(double base, uint32_t k) {
    double r = 1.0;
    while (k) {
        if (k & 1u) r *= base;
        base *= base;
        k >>= 1;
    }
    return r;
}

struct Coef {
    float clip, decay, omb1, beta2, omb2, eps, step_size, bc2_sqrt;
};

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const Coef& k) {
    g *= k.clip;
    p *= k.decay;
    m = fmaf(k.omb1, g - m, m);
    v = fmaf(k.omb2 * g, g, v * k.beta2);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = fmaf(-k.step_size, m / denom, p);
}

__device__ __forceinline__ void adamw_elem4(f32x4& p, f32x4 g, f32x4& m, f32x4& v, const Coef& k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adamw_elem(pj, g[j], mj, vj, k);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
    }
}

__device__ __forceinline__ f32x4 ld4_any(const float* q, bool vec) {
    if (vec) return ld4(q);
    f32x4 r;
    r[0] = q[0];
    r[1] = q[1];
    r[2] = q[2];
    r[3] = q[3];
    return r;
}

__global__ __launch_bounds__(AW_THREADS) void adamw_update_kernel(UpdTable tab, int nt, Hyper h, int flags,
                                                                  const float2* __restrict__ part, int np) {
    const int tid = threadIdx.x;
    Coef k;
    k.clip = 1.f;
    if (flags & (MDL_ADAMW_GUARD | MDL_ADAMW_CLIP)) {
        double sumsq;
        bool bad;
        merge_partials(part, np, sumsq, bad);
        if ((flags & MDL_ADAMW_GUARD) && bad) return;          // void step: nothing is written, by any workgroup of any launch
        if (flags & MDL_ADAMW_CLIP) k.clip = clip_coef(sumsq, as_double(h.max_norm));
    }
    const double lr = as_double(h.lr), beta1 = as_double(h.beta1), beta2 = as_double(h.beta2);
    k.decay = (float)(1.0 - lr * as_double(h.wd));
    k.omb1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.omb2 = (float)(1.0 - beta2);
    k.eps = (float)as_double(h.eps);
    k.step_size = 0.f;
    k.bc2_sqrt = 1.f;

    int ti = 0, cur = -1;
    int64_t first = 0;
    for (int64_t c = blockIdx.x; seek(tab, nt, c, ti, first); c += gridDim.x) {
        if (ti != cur) {                         // t = step + 1 is the tensor's own: a parameter without a gradient does not advance
            cur = ti;
            const uint32_t t = (uint32_t)tab.step[ti][0] + 1u;
            k.step_size = (float)(lr / (1.0 - powi(beta1, t)));
            k.bc2_sqrt = (float)sqrt(1.0 - powi(beta2, t));
        }
        const int64_t base = (c - first) * AW_CHUNK;
        const int64_t left = tab.numel[ti] - base;
        const int cnt = left < AW_CHUNK ? (int)left : AW_CHUNK;
        float* p = tab.p[ti] + base;
        const float* g = tab.g[ti] + base;
        float* m = tab.m[ti] + base;
        float* v = tab.v[ti] + base;
        if (aligned16(p) && aligned16(m) && aligned16(v)) {
            const bool gvec = aligned16(g);      // FlatGradSync: aligned parameters and moments, gradient views at odd offsets
            if (cnt == AW_CHUNK) {
                f32x4 xp[AW_VEC], xg[AW_VEC], xm[AW_VEC], xv[AW_VEC];
#pragma unroll
                for (int u = 0; u < AW_VEC; ++u) {
                    const int e = (u * AW_THREADS + tid) * 4;
                    xg[u] = ld4_any(g + e, gvec);
                    xp[u] = ld4(p + e);
                    xm[u] = ld4(m + e);
                    xv[u] = ld4(v + e);
                }
#pragma unroll
                for (int u = 0; u < AW_VEC; ++u) {
                    const int e = (u * AW_THREADS + tid) * 4;
                    adamw_elem4(xp[u], xg[u], xm[u], xv[u], k);
                    st4(p + e, xp[u]);
                    st4(m + e, xm[u]);
                    st4(v + e, xv[u]);
                }
            } else {
                for (int e = tid * 4; e < cnt; e += AW_THREADS * 4) {
                    if (e + 4 <= cnt) {
                        f32x4 xp = ld4(p + e), xm = ld4(m + e), xv = ld4(v + e);
                        const f32x4 xg = ld4_any(g + e, gvec);
                        adamw_elem4(xp, xg, xm, xv, k);
                        st4(p + e, xp);
                        st4(m + e, xm);
                        st4(v + e, xv);
                    } else {
                        for (int j = e; j < cnt; ++j) adamw_elem(p[j], g[j], m[j], v[j], k);
                    }
                }
            }
        } else {
            for (int e = tid; e < cnt; e += AW_THREADS) adamw_elem(p[e], g[e], m[e], v[e], k);
        }
    }
}

__global__ __launch_bounds__(AW_THREADS) void adamw_commit_kernel(StepTable tab, int nt, int flags, const float2* __restrict__ part, int np,
                                                                  float* __restrict__ grad_norm, int64_t* __restrict__ skipped) {
    const int tid = threadIdx.x;
    double sumsq = 0.0;
    bool bad = false;
    const bool stats = (flags & (MDL_ADAMW_GUARD | MDL_ADAMW_CLIP)) != 0;
    if (stats) merge_partials(part, np, sumsq, bad);
    const bool is_void = (flags & MDL_ADAMW_GUARD) && bad;
    if (tid < nt && !is_void) tab.step[tid][0] += 1.f;
    if (tid == 0 && (flags & MDL_ADAMW_FINAL)) {
        if (stats) grad_norm[0] = (float)sqrt(sumsq);
        if (is_void) skipped[0] += 1;
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The partial slots of a step that ran `stat_launches` statistics launches; 0 where the flags ask for none.
inline int check_ws(int flags, const void* ws, int64_t stat_launches, int* np) {
    *np = 0;
    if (!(flags & (MDL_ADAMW_GUARD | MDL_ADAMW_CLIP))) return MDL_OK;
    if (ws == nullptr || stat_launches < 1 || stat_launches > MDL_ADAMW_MAX_STAT_LAUNCHES) return MDL_E_ARG;
    if (!host_aligned16(ws)) return MDL_E_ALIGN;
    *np = (int)(stat_launches * AW_STAT_BLOCKS);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_adamw_ws_bytes(int64_t stat_launches) {
    if (stat_launches < 0) return MDL_E_ARG;
    if (stat_launches > MDL_ADAMW_MAX_STAT_LAUNCHES) return MDL_E_UNSUPPORTED;
    return stat_launches * AW_STAT_BLOCKS * (int64_t)sizeof(float2);
}

extern "C" int mdl_adamw_grad_stats(int nt, const float* const* g_host, const int64_t* numel_host, void* ws, int64_t slot,
                                    int64_t stat_launches, void* stream) {
    if (nt < 0 || (nt > 0 && (g_host == nullptr || numel_host == nullptr))) return MDL_E_ARG;
    if (nt > AW_MAXT) return MDL_E_UNSUPPORTED;
    if (ws == nullptr || stat_launches < 1 || stat_launches > MDL_ADAMW_MAX_STAT_LAUNCHES || slot < 0 || slot >= stat_launches)
        return MDL_E_ARG;
    if (!host_aligned16(ws)) return MDL_E_ALIGN;
    StatTable tab = {};
    for (int i = 0; i < nt; ++i) {
        if (numel_host[i] < 0 || (numel_host[i] > 0 && g_host[i] == nullptr)) return MDL_E_ARG;
        if (!aligned4(g_host[i])) return MDL_E_ALIGN;
        tab.g[i] = g_host[i];
        tab.numel[i] = numel_host[i];
    }
    float2* part = reinterpret_cast<float2*>(ws) + slot * AW_STAT_BLOCKS;
    // always the full grid: a workgroup without a chunk still writes its (zero) slot, so every slot the update reads is written
    hipLaunchKernelGGL(adamw_stats_kernel, dim3(AW_STAT_BLOCKS), dim3(AW_THREADS), 0, (hipStream_t)stream, tab, nt, part);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int mdl_adamw_update(int nt, float* const* p_host, const float* const* g_host, float* const* exp_avg_host,
                                float* const* exp_avg_sq_host, const float* const* step_host, const int64_t* numel_host,
                                uint64_t lr_bits, uint64_t beta1_bits, uint64_t beta2_bits, uint64_t eps_bits, uint64_t weight_decay_bits,
                                uint64_t max_norm_bits, int flags, const void* ws, int64_t stat_launches, void* stream) {
    if (nt < 0 || (flags & ~(MDL_ADAMW_GUARD | MDL_ADAMW_CLIP))) return MDL_E_ARG;
    if (nt > 0 && (!p_host || !g_host || !exp_avg_host || !exp_avg_sq_host || !step_host || !numel_host)) return MDL_E_ARG;
    if (nt > AW_MAXT) return MDL_E_UNSUPPORTED;
    int np = 0;
    if (const int rc = check_ws(flags, ws, stat_launches, &np)) return rc;
    UpdTable tab = {};
    int64_t chunks = 0;
    for (int i = 0; i < nt; ++i) {
        const int64_t n = numel_host[i];
        if (n < 0 || step_host[i] == nullptr) return MDL_E_ARG;
        if (n > 0 && (!p_host[i] || !g_host[i] || !exp_avg_host[i] || !exp_avg_sq_host[i])) return MDL_E_ARG;
        if (!aligned4(p_host[i]) || !aligned4(g_host[i]) || !aligned4(exp_avg_host[i]) || !aligned4(exp_avg_sq_host[i]) ||
            !aligned4(step_host[i]))
            return MDL_E_ALIGN;
        tab.p[i] = p_host[i];
        tab.g[i] = g_host[i];
        tab.m[i] = exp_avg_host[i];
        tab.v[i] = exp_avg_sq_host[i];
        tab.step[i] = step_host[i];
        tab.numel[i] = n;
        chunks += chunks_of(n);
    }
    if (chunks == 0) return MDL_OK;           // only empty tensors: nothing to update (their steps advance in the commit)
    const Hyper h = {lr_bits, beta1_bits, beta2_bits, eps_bits, weight_decay_bits, max_norm_bits};
    const int grid = (int)(chunks < AW_MAX_BLOCKS ? chunks : AW_MAX_BLOCKS);
    hipLaunchKernelGGL(adamw_update_kernel, dim3(grid), dim3(AW_THREADS), 0, (hipStream_t)stream, tab, nt, h, flags,
                       reinterpret_cast<const float2*>(ws), np);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int mdl_adamw_commit(int nt, float* const* step_host, int flags, const void* ws, int64_t stat_launches, float* grad_norm,
                                int64_t* skipped, void* stream) {
    if (nt < 0 || (flags & ~(MDL_ADAMW_GUARD | MDL_ADAMW_CLIP | MDL_ADAMW_FINAL))) return MDL_E_ARG;
    if (nt > 0 && step_host == nullptr) return MDL_E_ARG;
    if (nt > AW_MAXT) return MDL_E_UNSUPPORTED;
    if ((flags & MDL_ADAMW_FINAL) && (grad_norm == nullptr || skipped == nullptr)) return MDL_E_ARG;
    int np = 0;
    if (const int rc = check_ws(flags, ws, stat_launches, &np)) return rc;
    StepTable tab = {};
    for (int i = 0; i < nt; ++i) {
        if (step_host[i] == nullptr) return MDL_E_ARG;
        if (!aligned4(step_host[i])) return MDL_E_ALIGN;
        tab.step[i] = step_host[i];
    }
    hipLaunchKernelGGL(adamw_commit_kernel, dim3(1), dim3(AW_THREADS), 0, (hipStream_t)stream, tab, nt, flags,
                       reinterpret_cast<const float2*>(ws), np, grad_norm, skipped);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}
