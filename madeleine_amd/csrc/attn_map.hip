// attn_map.hip -- the attention read-out (section A-map of the header): per (bag, head) segment of raw scores [T, H] the softmax with
// its statistics, an exact stable descending order, percentile ranks and the k best rows.  All segments of a call share every launch;
// the number of launches depends on neither R nor T.
//
//   am_plan_kernel      one workgroup: cu -> the segment table (first row, rows, first chunk of every bag).  A bag that is not inside
//                       [0, T], runs backwards or would push the chunk count past the launch grid is an EMPTY bag: nothing of it is
//                       read or written by any later kernel.
//   softmax             am_chunk_max -> am_seg_max (m) -> am_chunk_sum -> am_seg_sum (l) -> am_normalise (attn).  A chunk is
//                       MDL_ATTN_ROWS rows of one segment; a segment's chunks are merged in chunk order by one thread.
//   rank                am_keys (score -> inverted 32-bit key, row index) and four LSD radix passes of 8 bits, each am_hist (per-chunk
//                       digit counts) -> am_scan (per segment, digit-major, chunk-minor exclusive offsets) -> am_scatter (one wave per
//                       chunk: 64 keys a round in row order, the rank among equal digits from __ballot matches, so the pass is stable);
//                       then am_pct (runs of equal keys by binary search in the sorted segment) and am_topk.
// No workgroup waits on another: launch order is the only dependency.  The only atomics are integer LDS counts inside am_hist (their
// order cannot change a count).  Every loop is bounded by an argument.
#include "common.hpp"

namespace mdl {
namespace {

constexpr int AM_C = MDL_ATTN_SORT_KEYS;        // keys of a sort chunk == rows of a softmax chunk: one chunk table serves both
constexpr int AM_THREADS = 256;
constexpr int AM_PER = AM_C / AM_THREADS;       // rows per thread of a chunk
constexpr int AM_RADIX = 256;
static_assert(MDL_ATTN_ROWS == MDL_ATTN_SORT_KEYS, "the softmax and the sort share the chunk table");
static_assert(AM_C % AM_THREADS == 0 && AM_C % WAVE == 0 && AM_THREADS == AM_RADIX, "chunk geometry");


// The workspace, carved in one place for the size query and both entry points.
struct Ws {
    int32_t *seg_start, *seg_n, *chunk_cu;      // [R], [R], [R + 1]
    uint32_t *key_a, *key_b;                    // [H, T] each
    int32_t* val_b;                             // [H, T]
    uint32_t* hist;                             // [H, NC, 256]
    float *pm, *pl;                             // [H, NC] each
    int64_t bytes;
};
inline int64_t max_chunks(int64_t T, int64_t R) { return T / AM_C + R; }       // sum ceil(n_r / C) <= floor(T / C) + R
inline Ws carve(void* base, int64_t T, int64_t R, int H) {
    char* p = reinterpret_cast<char*>(base);
    int64_t o = 0;
    const int64_t NC = max_chunks(T, R);
    const auto take = [&](int64_t bytes) { char* q = p + o; o += up16(bytes); return q; };
    Ws w;
    w.seg_start = reinterpret_cast<int32_t*>(take(R * 4));
    w.seg_n = reinterpret_cast<int32_t*>(take(R * 4));
    w.chunk_cu = reinterpret_cast<int32_t*>(take((R + 1) * 4));
    w.key_a = reinterpret_cast<uint32_t*>(take(H * T * 4));
    w.key_b = reinterpret_cast<uint32_t*>(take(H * T * 4));
    w.val_b = reinterpret_cast<int32_t*>(take(H * T * 4));
    w.hist = reinterpret_cast<uint32_t*>(take(H * NC * AM_RADIX * 4));
    w.pm = reinterpret_cast<float*>(take(H * NC * 4));
    w.pl = reinterpret_cast<float*>(take(H * NC * 4));
    w.bytes = o;
    return w;
}

// What every kernel knows of the call: the segment table and the sizes.
struct Plan {
    const int32_t *seg_start, *seg_n, *chunk_cu;
    int R, T, H, NC;
};

// ---- the segment table --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AM_THREADS) void am_plan_kernel(const int64_t* __restrict__ cu, int R, int T, int NC,
                                                             int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_n,
                                                             int32_t* __restrict__ chunk_cu) {
    __shared__ int64_t s_scan[AM_THREADS];
    __shared__ int64_t s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_carry = 0;
        chunk_cu[0] = 0;
    }
    __syncthreads();
    for (int r0 = 0; r0 < R; r0 += AM_THREADS) {
        const int r = r0 + tid;
        int64_t a = 0, n = 0;
        if (r < R) {
            a = cu[r];
            const int64_t b = cu[r + 1];
            if (a >= 0 && a <= b && b <= (int64_t)T) n = b - a;
        }
        const int64_t cnt = (n + AM_C - 1) / AM_C;
        s_scan[tid] = cnt;
        __syncthreads();
        for (int o = 1; o < AM_THREADS; o <<= 1) {            // inclusive scan of the tile's chunk counts
            const int64_t add = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const int64_t incl = s_carry + s_scan[tid];
        if (r < R) {
            const bool fits = incl <= (int64_t)NC;            // always, with a consistent cu
            seg_start[r] = (int32_t)(n > 0 && fits ? a : 0);
            seg_n[r] = (int32_t)(fits ? n : 0);
            chunk_cu[r + 1] = (int32_t)(fits ? incl : (int64_t)NC);
        }
        __syncthreads();
        if (tid == AM_THREADS - 1) s_carry = incl <= (int64_t)NC ? incl : (int64_t)NC + 1;     // saturates: no overflow, stays "past NC"
        __syncthreads();
    }
}

struct Seg {
    int r, start, n, c;      // bag, first row, rows, chunk inside the segment
};

// The segment of chunk `chunk` (uniform over the workgroup); false where the chunk holds no row.
__device__ __forceinline__ bool find_seg(const Plan& p, int chunk, Seg& s) {
    if (chunk >= p.chunk_cu[p.R]) return false;
    int lo = 0, hi = p.R - 1;
    while (lo < hi) {                                         // the first r with chunk_cu[r + 1] > chunk
        const int mid = (lo + hi) >> 1;
        if (p.chunk_cu[mid + 1] <= chunk) lo = mid + 1;
        else hi = mid;
    }
    s.r = lo;
    s.start = p.seg_start[lo];
    s.n = p.seg_n[lo];
    s.c = chunk - p.chunk_cu[lo];
    return s.c >= 0 && (int64_t)s.c * AM_C < s.n;
}

__device__ __forceinline__ int chunks_of(int n) { return (n + AM_C - 1) / AM_C; }

// Workgroup reductions in one fixed order: xor butterflies inside a wave, then the four waves as (0 + 1) + (2 + 3).
__device__ __forceinline__ float wg_sum(float v, float* s_red) {
    v = wave_sum(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
__device__ __forceinline__ float wg_max(float v, float* s_red) {
    v = wave_max(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// ---- softmax ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AM_THREADS) void am_chunk_max_kernel(Plan p, const float* __restrict__ scores, int64_t ld,
                                                                  float* __restrict__ pm) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    __shared__ float s_red[AM_THREADS / WAVE];
    const int h = blockIdx.y;
    float v = -INFINITY;
#pragma unroll
    for (int q = 0; q < AM_PER; ++q) {
        const int i = s.c * AM_C + q * AM_THREADS + threadIdx.x;
        if (i < s.n) v = fmaxf(v, scores[(int64_t)(s.start + i) * ld + h]);
    }
    v = wg_max(v, s_red);
    if (threadIdx.x == 0) pm[(int64_t)h * p.NC + blockIdx.x] = v;
}

// One thread per segment: the segment's chunks in chunk order.  SUM = false: m = max of the chunk maxima; SUM = true: l = their sum.
template <bool SUM>
__global__ __launch_bounds__(AM_THREADS) void am_seg_kernel(Plan p, const float* __restrict__ part, float* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * AM_THREADS + threadIdx.x;
    if (g >= (int64_t)p.R * p.H) return;
    const int r = (int)(g / p.H), h = (int)(g % p.H);
    const int nch = chunks_of(p.seg_n[r]);
    const float* q = part + (int64_t)h * p.NC + p.chunk_cu[r];
    float v = SUM ? 0.f : -INFINITY;
    if (nch > 0) {
        v = q[0];
        for (int c = 1; c < nch; ++c) v = SUM ? v + q[c] : fmaxf(v, q[c]);
    }
    out[g] = v;
}

__global__ __launch_bounds__(AM_THREADS) void am_chunk_sum_kernel(Plan p, const float* __restrict__ scores, int64_t ld,
                                                                  const float* __restrict__ m, float* __restrict__ pl) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    __shared__ float s_red[AM_THREADS / WAVE];
    const int h = blockIdx.y;
    const float mm = m[(int64_t)s.r * p.H + h];
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < AM_PER; ++q) {                        // a thread's rows in row order; a row past the end adds +0, exactly
        const int i = s.c * AM_C + q * AM_THREADS + threadIdx.x;
        acc += i < s.n ? expf(scores[(int64_t)(s.start + i) * ld + h] - mm) : 0.f;
    }
    acc = wg_sum(acc, s_red);
    if (threadIdx.x == 0) pl[(int64_t)h * p.NC + blockIdx.x] = acc;
}

__global__ __launch_bounds__(AM_THREADS) void am_normalise_kernel(Plan p, const float* __restrict__ scores, int64_t ld,
                                                                  const float* __restrict__ m, const float* __restrict__ l,
                                                                  float* __restrict__ attn) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    const int h = blockIdx.y;
    const float mm = m[(int64_t)s.r * p.H + h], ll = l[(int64_t)s.r * p.H + h];
#pragma unroll
    for (int q = 0; q < AM_PER; ++q) {
        const int i = s.c * AM_C + q * AM_THREADS + threadIdx.x;
        if (i < s.n) attn[(int64_t)(s.start + i) * p.H + h] = expf(scores[(int64_t)(s.start + i) * ld + h] - mm) / ll;
    }
}

// ---- rank ---------------------------------------------------------------------------------------------------------------------------
// The sort key of a score: ascending unsigned order of the key is DESCENDING order of the scores under the header's comparison rule
// (-0 == +0, all NaNs equal and above +inf), so a stable ascending sort leaves ties in row order.
__device__ __forceinline__ uint32_t sort_key(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0x7FC00000u;     // every NaN: one positive quiet NaN, above +inf
    if (u == 0x80000000u) u = 0u;                             // -0 is +0
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

__global__ __launch_bounds__(AM_THREADS) void am_keys_kernel(Plan p, const float* __restrict__ scores, int64_t ld,
                                                             uint32_t* __restrict__ key, int32_t* __restrict__ val) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    const int h = blockIdx.y;
#pragma unroll
    for (int q = 0; q < AM_PER; ++q) {
        const int i = s.c * AM_C + q * AM_THREADS + threadIdx.x;
        if (i < s.n) {
            const int64_t at = (int64_t)h * p.T + s.start + i;
            key[at] = sort_key(scores[(int64_t)(s.start + i) * ld + h]);
            val[at] = i;
        }
    }
}

__global__ __launch_bounds__(AM_THREADS) void am_hist_kernel(Plan p, const uint32_t* __restrict__ key, int shift,
                                                             uint32_t* __restrict__ hist) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    __shared__ uint32_t s_hist[AM_RADIX];
    const int h = blockIdx.y;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < AM_PER; ++q) {
        const int i = s.c * AM_C + q * AM_THREADS + threadIdx.x;
        if (i < s.n) atomicAdd(&s_hist[(key[(int64_t)h * p.T + s.start + i] >> shift) & (AM_RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[((int64_t)h * p.NC + blockIdx.x) * AM_RADIX + threadIdx.x] = s_hist[threadIdx.x];
}

// One workgroup per segment, thread d = digit d: the counts become exclusive offsets inside the segment, digit-major and chunk-minor.
__global__ __launch_bounds__(AM_RADIX) void am_scan_kernel(Plan p, uint32_t* __restrict__ hist) {
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int nch = chunks_of(p.seg_n[r]);
    if (nch == 0) return;
    __shared__ uint32_t s_scan[AM_RADIX];
    const int d = threadIdx.x;
    uint32_t* q = hist + ((int64_t)h * p.NC + p.chunk_cu[r]) * AM_RADIX + d;
    uint32_t total = 0;
    for (int c = 0; c < nch; ++c) total += q[(int64_t)c * AM_RADIX];
    s_scan[d] = total;
    __syncthreads();
    for (int o = 1; o < AM_RADIX; o <<= 1) {
        const uint32_t add = d >= o ? s_scan[d - o] : 0u;
        __syncthreads();
        s_scan[d] += add;
        __syncthreads();
    }
    uint32_t run = s_scan[d] - total;
    for (int c = 0; c < nch; ++c) {
        const uint32_t v = q[(int64_t)c * AM_RADIX];
        q[(int64_t)c * AM_RADIX] = run;
        run += v;
    }
}

// One wave per chunk.  A round places 64 consecutive keys: a key goes to (offset of its digit so far) + (earlier lanes of the round with
// the same digit), which keeps equal digits in input order.
__global__ __launch_bounds__(WAVE) void am_scatter_kernel(Plan p, const uint32_t* __restrict__ key_in, const int32_t* __restrict__ val_in,
                                                          int shift, const uint32_t* __restrict__ offs, uint32_t* __restrict__ key_out,
                                                          int32_t* __restrict__ val_out) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    __shared__ uint32_t s_base[AM_RADIX];
    const int h = blockIdx.y, lane = threadIdx.x;
    for (int d = lane; d < AM_RADIX; d += WAVE) s_base[d] = offs[((int64_t)h * p.NC + blockIdx.x) * AM_RADIX + d];
    __syncthreads();
    const int64_t seg0 = (int64_t)h * p.T + s.start;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int round = 0; round < AM_C / WAVE; ++round) {
        const int i = s.c * AM_C + round * WAVE + lane;
        if (s.c * AM_C + round * WAVE >= s.n) break;          // uniform
        const bool active = i < s.n;
        const uint32_t k = active ? key_in[seg0 + i] : 0u;
        const int32_t v = active ? val_in[seg0 + i] : 0;
        const uint32_t d = (k >> shift) & (AM_RADIX - 1);
        uint64_t same = __ballot(active);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t vote = __ballot(bit);
            same &= bit ? vote : ~vote;
        }
        const uint32_t before = (uint32_t)__popcll(same & below), count = (uint32_t)__popcll(same);
        if (active) {
            const uint32_t at = s_base[d] + before;
            if (at < (uint32_t)s.n) {                         // always, when the offsets are this pass's own
                key_out[seg0 + at] = k;
                val_out[seg0 + at] = v;
            }
        }
        __syncthreads();
        if (active && before == 0) s_base[d] += count;
        __syncthreads();
    }
}

// key [H, T] sorted ascending inside every segment, order [H, T] the rows in that order.  L = rows strictly below = those after the
// run of equal keys, E = the run.
__global__ __launch_bounds__(AM_THREADS) void am_pct_kernel(Plan p, const uint32_t* __restrict__ key, const int32_t* __restrict__ order,
                                                            float* __restrict__ pct) {
    Seg s;
    if (!find_seg(p, blockIdx.x, s)) return;
    const int h = blockIdx.y;
    const uint32_t* ks = key + (int64_t)h * p.T + s.start;
#pragma unroll
    for (int q = 0; q < AM_PER; ++q) {
        const int i = s.c * AM_C + q * AM_THREADS + threadIdx.x;
        if (i >= s.n) continue;
        const uint32_t k = ks[i];
        int lo = 0, hi = i;                                   // the first position holding k
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ks[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        const int first = lo;
        lo = i + 1;
        hi = s.n;                                             // the first position holding more than k
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ks[mid] <= k) lo = mid + 1;
            else hi = mid;
        }
        const int64_t E = lo - first, L = s.n - lo;
        const int row = order[(int64_t)h * p.T + s.start + i];
        if (row >= 0 && row < s.n)
            pct[(int64_t)(s.start + row) * p.H + h] = (float)(100.0 * (double)(2 * L + E + 1) / (2.0 * (double)s.n));
    }
}

__global__ __launch_bounds__(AM_THREADS) void am_topk_kernel(Plan p, const float* __restrict__ scores, int64_t ld,
                                                             const int32_t* __restrict__ order, int k, int64_t total,
                                                             int32_t* __restrict__ topk_idx, float* __restrict__ topk_val) {
    const int64_t g = (int64_t)blockIdx.x * AM_THREADS + threadIdx.x;
    if (g >= total) return;
    const int j = (int)(g % k);
    const int64_t seg = g / k;
    const int h = (int)(seg % p.H), r = (int)(seg / p.H);
    const int n = p.seg_n[r], start = p.seg_start[r];
    int32_t idx = -1;
    float v = -INFINITY;
    if (j < n) {
        const int row = order[(int64_t)h * p.T + start + j];
        if (row >= 0 && row < n) {
            idx = row;
            v = scores[(int64_t)(start + row) * ld + h];
        }
    }
    topk_idx[g] = idx;
    topk_val[g] = v;
}


// The refusals the two entry points share, in the header's order; `grid` is the widest launch the call needs beyond the chunk grid.
int check_call(const float* scores, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int H, const void* ws) {
    if (!scores || !cu || !ws || T < 0 || R < 0 || ld < H) return MDL_E_ARG;
    if (H != 1 && H != 2 && H != 4 && H != 8) return MDL_E_UNSUPPORTED;
    if (!i32(T) || !i32(R) || !i32(max_chunks(T, R)) || !i32(R * H)) return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

Plan plan_of(const Ws& w, int64_t T, int64_t R, int H) { return Plan{w.seg_start, w.seg_n, w.chunk_cu, (int)R, (int)T, H, (int)max_chunks(T, R)}; }

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_attn_map_ws_bytes(int64_t T, int64_t R, int H) {
    if (T < 0 || R < 0) return MDL_E_ARG;
    if (H != 1 && H != 2 && H != 4 && H != 8) return MDL_E_UNSUPPORTED;
    if (!i32(T) || !i32(R) || !i32(max_chunks(T, R)) || !i32(R * H)) return MDL_E_UNSUPPORTED;
    return carve(nullptr, T, R, H).bytes;
}

#define AM_LAUNCH(kernel, grid, block, ...)                                                     \
    do {                                                                                        \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);     \
        MDL_LAUNCH_CHECK();                                                                     \
    } while (0)

extern "C" int mdl_attn_softmax(const float* scores, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int H, float* attn, float* m,
                                float* l, void* ws, void* stream) {
    if (!attn || !m || !l) return MDL_E_ARG;
    if (const int rc = check_call(scores, ld, cu, T, R, H, ws)) return rc;
    if (!host_aligned16(ws) || !aligned_to(cu, 8) || !aligned_to(scores, 4) || !aligned_to(attn, 4) || !aligned_to(m, 4) ||
        !aligned_to(l, 4))
        return MDL_E_ALIGN;
    if (R == 0 || T == 0) return MDL_OK;
    const Ws w = carve(ws, T, R, H);
    const Plan p = plan_of(w, T, R, H);
    const dim3 chunks((unsigned)p.NC, (unsigned)H), segs((unsigned)((R * H + AM_THREADS - 1) / AM_THREADS));
    AM_LAUNCH(am_plan_kernel, dim3(1), AM_THREADS, cu, p.R, p.T, p.NC, w.seg_start, w.seg_n, w.chunk_cu);
    AM_LAUNCH(am_chunk_max_kernel, chunks, AM_THREADS, p, scores, ld, w.pm);
    AM_LAUNCH(am_seg_kernel<false>, segs, AM_THREADS, p, (const float*)w.pm, m);
    AM_LAUNCH(am_chunk_sum_kernel, chunks, AM_THREADS, p, scores, ld, (const float*)m, w.pl);
    AM_LAUNCH(am_seg_kernel<true>, segs, AM_THREADS, p, (const float*)w.pl, l);
    AM_LAUNCH(am_normalise_kernel, chunks, AM_THREADS, p, scores, ld, (const float*)m, (const float*)l, attn);
    return MDL_OK;
}

extern "C" int mdl_attn_rank(const float* scores, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int H, int64_t k, int32_t* order,
                             float* pct, int32_t* topk_idx, float* topk_val, void* ws, void* stream) {
    if (!order || k < 0 || (k > 0 && (!topk_idx || !topk_val))) return MDL_E_ARG;
    if (const int rc = check_call(scores, ld, cu, T, R, H, ws)) return rc;
    if (!i32(k) || (k > 0 && R * H > 0x7FFFFFFFLL * AM_THREADS / k)) return MDL_E_UNSUPPORTED;      // the top-k grid
    if (!host_aligned16(ws) || !aligned_to(cu, 8) || !aligned_to(scores, 4) || !aligned_to(order, 4) || !aligned_to(pct, 4) ||
        !aligned_to(topk_idx, 4) || !aligned_to(topk_val, 4))
        return MDL_E_ALIGN;
    if (R == 0 || T == 0) return MDL_OK;
    const Ws w = carve(ws, T, R, H);
    const Plan p = plan_of(w, T, R, H);
    const dim3 chunks((unsigned)p.NC, (unsigned)H);
    AM_LAUNCH(am_plan_kernel, dim3(1), AM_THREADS, cu, p.R, p.T, p.NC, w.seg_start, w.seg_n, w.chunk_cu);
    AM_LAUNCH(am_keys_kernel, chunks, AM_THREADS, p, scores, ld, w.key_a, order);
    uint32_t *k_in = w.key_a, *k_out = w.key_b;
    int32_t *v_in = order, *v_out = w.val_b;
    for (int pass = 0; pass < 4; ++pass) {                    // an even number of passes: the result lands in (key_a, order)
        AM_LAUNCH(am_hist_kernel, chunks, AM_THREADS, p, (const uint32_t*)k_in, 8 * pass, w.hist);
        AM_LAUNCH(am_scan_kernel, dim3((unsigned)(R * H)), AM_RADIX, p, w.hist);
        AM_LAUNCH(am_scatter_kernel, chunks, WAVE, p, (const uint32_t*)k_in, (const int32_t*)v_in, 8 * pass, (const uint32_t*)w.hist, k_out,
                  v_out);
        uint32_t* tk = k_in; k_in = k_out; k_out = tk;
        int32_t* tv = v_in; v_in = v_out; v_out = tv;
    }
    if (pct) AM_LAUNCH(am_pct_kernel, chunks, AM_THREADS, p, (const uint32_t*)w.key_a, (const int32_t*)order, pct);
    if (k > 0) {
        const int64_t total = R * H * k;
        AM_LAUNCH(am_topk_kernel, dim3((unsigned)((total + AM_THREADS - 1) / AM_THREADS)), AM_THREADS, p, scores, ld,
                  (const int32_t*)order, (int)k, total, topk_idx, topk_val);
    }
    return MDL_OK;
}
