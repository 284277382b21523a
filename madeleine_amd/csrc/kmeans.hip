// kmeans.hip -- K1-K4 of include/madeleine_amd_cluster.h: Lloyd's k-means with k-means++ seeding over the rows of a device-resident
// feature store, read where they lie (any store dtype, widened exactly), and the per-bag histogram of the labels.
//
//   K1  km_prep_kernel     centroids -> zero-padded Cp [kp, dp] (kp = k to 128, dp = D to 32) and half-norms hn [kp], once per call
//       km_assign_kernel   workgroup w owns one chunk of KM_ROWS = 128 rows of one bag (found by binary search in chunk_cu, as S2 / S5)
//                          and streams the 128-centroid tiles of Cp past it: a tile is a 128 x 128 x dp product on the exact-fp32 MFMA
//                          (v_mfma_f32_32x32x2_f32; operand tiles, thread maps and the contraction order are retrieval.hip's), the row
//                          operand loaded from the store in place.  Wave w holds rows 32 w .. 32 w + 31; the finished tile is consumed
//                          in its accumulators: v = acc - hn, a lane's best of its 4 columns, a butterfly over the 32 lanes that hold
//                          a row's columns, and the running best over the tiles.  (value, index) under "greater value, then lower
//                          index" is a total order (a NaN v is made -inf first), so neither the butterfly nor the tiling shows.
//       km_assign_finish   one workgroup adds the chunks' counts and, in chunk order, their double inertia partials
//   K2  km_sort_hist / km_sort_scan / km_sort_scatter   the stable counting sort of call positions by label (integers only)
//       km_mean_partial / km_mean_combine               S5's scheme over a cluster's member list, the chunk partials combined in double
//   K3  km_seed_dist / km_seed_pick                     k-means++: two launches per centre, the pick by one workgroup
//   K4  km_hist_kernel     one workgroup per bag, integer LDS counters
//
// Bounds.  Every chunk is placed by place_chunk: r out of a search over [0, R), the bag's rows by bag_extent inside [0, T_total), its
// call positions inside [0, T); a chunk the tables do not agree on reads and writes nothing but its own (zero) partials.  Launch order
// is the only dependency between workgroups; no atomics on floats; no host read.
#include "common.hpp"

#include "../../include/madeleine_amd_cluster.h"

namespace mdl {
namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_ROWS = MDL_KM_ROWS;           // rows per chunk: 4 waves x 32
constexpr int KM_BN = 128;                     // centroids per tile: 4 MFMA column blocks per wave
constexpr int KM_BK = 32;                      // contraction per LDS stage
constexpr int KM_LDT = KM_BK + 4;              // LDS row stride (floats): retrieval.hip's, conflict-free 16-byte reads down a column of rows
constexpr int KM_SORT = MDL_KM_SORT_ROWS;
constexpr int KM_MEAN = MDL_KM_MEAN_ROWS;
constexpr int KM_SLICES = 256;                 // slices of the chunk list in the seeds' pick
static_assert(KM_ROWS == 128 && KM_THREADS == 256, "the thread maps below are written for these");

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// The row source of a call (the header's tables).  Bases are untyped: the checks know no element type.
struct Src {
    const void* store;
    int64_t row_stride, T_total;
    const int64_t* off;
    int64_t n_bags;
    const int32_t* bag;
    const int64_t* cu;
    const int64_t* chunk_cu;
    int R;
    int64_t n_chunks, T;
    int D;
};

template <class V>
__device__ __forceinline__ V table(const V* p, int64_t i) {
    return ((const __attribute__((address_space(4))) V*)p)[i];
}

// stored bag g: its length with `base` its first row of [0, T_total), or 0 where it contributes no rows (S1's bounds rule)
__device__ __forceinline__ int64_t bag_extent(const Src& s, int g, int64_t& base) {
    int64_t n = 0;
    base = 0;
    if (g >= 0 && g < s.n_bags) {
        base = table(s.off, g);
        n = table(s.off, g + 1) - base;
        if (base < 0 || n < 1 || n > 0x7FFFFFFF || base > s.T_total - n) n = base = 0;
    }
    return n;
}

// the last r of [0, R) with tab[r] <= w
__device__ __forceinline__ int search_le(const int64_t* tab, int R, int64_t w) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table(tab, mid) <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Chunk w of the call: `first` its first store row, `p0` its first call position, the return value its rows (1 .. KM_ROWS), or 0 for a
// chunk the tables do not place: then nothing of the store may be read and no position written.
__device__ __forceinline__ int place_chunk(const Src& s, int64_t w, int64_t& first, int64_t& p0) {
    const int r = search_le(s.chunk_cu, s.R, w);
    const int64_t c = w - table(s.chunk_cu, r);
    int64_t base;
    const int64_t n = bag_extent(s, table(s.bag, r), base);
    if (c < 0 || c >= (n + KM_ROWS - 1) / KM_ROWS) return 0;
    const int64_t q = table(s.cu, r);
    if (q < 0 || q > s.T - n) return 0;                        // its positions q .. q + n - 1 lie inside [0, T)
    first = base + c * KM_ROWS;
    p0 = q + c * KM_ROWS;
    return n - c * KM_ROWS < KM_ROWS ? (int)(n - c * KM_ROWS) : KM_ROWS;
}

// The store row of call position p, or -1 where the tables place none.
__device__ __forceinline__ int64_t place_position(const Src& s, int64_t p) {
    if (s.R < 1) return -1;
    const int r = search_le(s.cu, s.R, p);
    const int64_t i = p - table(s.cu, r);
    int64_t base;
    const int64_t n = bag_extent(s, table(s.bag, r), base);
    return (i >= 0 && i < n) ? base + i : -1;
}

__device__ __forceinline__ float up(float x) { return x; }
__device__ __forceinline__ float up(_Float16 x) { return (float)x; }
__device__ __forceinline__ float up(bf16_t x) { return (float)x; }
__device__ __forceinline__ f32x4 km_ld4(const float* p) { return ld4(p); }
__device__ __forceinline__ f32x4 km_ld4(const bf16_t* p) { return ld4(p); }
__device__ __forceinline__ f32x4 km_ld4(const _Float16* p) { return __builtin_convertvector(*reinterpret_cast<const f16x4*>(p), f32x4); }

// columns col .. col + 3 of a store row, widened exactly; columns at or beyond D read as 0.  VEC: D and row_stride are multiples of 4
// and the store is 16-byte aligned, so the four are whole and 16- (fp32) / 8-byte (16-bit stores) aligned.  Both forms give the same values.
template <class T, bool VEC>
__device__ __forceinline__ f32x4 load4(const T* __restrict__ row, int col, int D) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (col < D) v = km_ld4(row + col);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col + j < D) v[j] = up(row[col + j]);
    }
    return v;
}

__device__ __forceinline__ bool km_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }
__device__ __forceinline__ float nanf32() { return __uint_as_float(0x7fc00000u); }

// ---- K1: assign -------------------------------------------------------------------------------------------------------------------
// one wave per padded centroid row
__global__ __launch_bounds__(64) void km_prep_kernel(const float* __restrict__ C, int k, int D, int dp, float* __restrict__ Cp,
                                                     float* __restrict__ hn) {
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x;
    float* __restrict__ dst = Cp + (int64_t)j * dp;
    if (j >= k) {
        for (int c = lane; c < dp; c += 64) dst[c] = 0.f;
        if (lane == 0) hn[j] = 0.f;
        return;
    }
    const float* __restrict__ src = C + (int64_t)j * D;
    float ss = 0.f;
    for (int c = lane; c < dp; c += 64) {
        const float x = c < D ? src[c] : 0.f;
        ss = fmaf(x, x, ss);
        dst[c] = x;
    }
    ss = wave_sum(ss);
    if (lane == 0) hn[j] = 0.5f * ss;
}

__device__ __forceinline__ int km_acc_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// (v, j) <- the better of (v, j) and (v2, j2): the greater value, then the lower index
__device__ __forceinline__ void km_better(float& v, int& j, float v2, int j2) {
    const bool take = v2 > v || (v2 == v && j2 < j);
    v = take ? v2 : v;
    j = take ? j2 : j;
}

template <class T, bool VEC>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(Src s, const float* __restrict__ Cp, const float* __restrict__ hn, int dp,
                                                               int k, int col_tiles, int32_t* __restrict__ labels,
                                                               float* __restrict__ dist, int32_t* __restrict__ pchg,
                                                               double* __restrict__ pin) {
    __shared__ __attribute__((aligned(16))) float ops[2 * KM_ROWS * KM_LDT];      // row tile | centroid tile
    __shared__ float s_xn[KM_ROWS], s_d[KM_ROWS];
    __shared__ int s_bad[KM_ROWS], s_chg[KM_ROWS];
    const int tid = (int)threadIdx.x, lane = tid & 63, l32 = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t w = blockIdx.x;
    int64_t first, p0;
    const int rows = place_chunk(s, w, first, p0);
    if (rows == 0) {                                           // uniform: nothing read, its partials are zero
        if (tid == 0) {
            pchg[w] = 0;
            pin[w] = 0.0;
        }
        return;
    }
    const int D = s.D, nkb = dp / KM_BK;
    // operand loads: thread -> rows (tid >> 3) + 32 p, floats (tid & 7) * 4 .. + 3 of the stage
    const int lr = tid >> 3, lc = (tid & 7) * 4;
    const T* __restrict__ arow[4];
    bool alive[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        alive[p] = lr + 32 * p < rows;
        arow[p] = static_cast<const T*>(s.store) + (first + (alive[p] ? lr + 32 * p : 0)) * s.row_stride;
    }
    const int64_t pstride = (int64_t)32 * dp;
    f32x4 pa[4], pb[4];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#define KM_FETCH(tile, kb)                                                                       \
    do {                                                                                         \
        const float* __restrict__ bsrc = Cp + ((int64_t)(tile)*KM_BN + lr) * dp + lc + (kb)*KM_BK; \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                          \
            pa[p] = alive[p] ? load4<T, VEC>(arow[p], (kb)*KM_BK + lc, D) : zero4;               \
            pb[p] = ld4(bsrc + p * pstride);                                                     \
        }                                                                                        \
    } while (0)
    KM_FETCH(0, 0);

    const float* As = ops + (wave * 32 + l32) * KM_LDT + kh * 4;
    const float* Bs = ops + KM_ROWS * KM_LDT + l32 * KM_LDT + kh * 4;
    float xn[4] = {0.f, 0.f, 0.f, 0.f};
    int bad[4] = {0, 0, 0, 0};
    float bv[16];
    int bj[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        bv[r] = -INFINITY;
        bj[r] = 0x7fffffff;
    }

#pragma unroll 1
    for (int t = 0; t < col_tiles; ++t) {
        f32x16 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
#pragma unroll 1
        for (int kb = 0; kb < nkb; ++kb) {
            __syncthreads();      // the previous stage has been read
            if (t == 0) {         // uniform: the rows' squared norms and finiteness, from the first pass over the row tile
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        xn[p] = fmaf(pa[p][i], pa[p][i], xn[p]);
                        bad[p] |= km_finite(pa[p][i]) ? 0 : 1;
                    }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                st4(ops + (lr + 32 * p) * KM_LDT + lc, pa[p]);
                st4(ops + KM_ROWS * KM_LDT + (lr + 32 * p) * KM_LDT + lc, pb[p]);
            }
            __syncthreads();
            if (kb + 1 < nkb) KM_FETCH(t, kb + 1);
            else if (t + 1 < col_tiles) KM_FETCH(t + 1, 0);
#pragma unroll
            for (int k8 = 0; k8 < KM_BK / 8; ++k8) {
                const f32x4 a = ld4(As + k8 * 8);
                f32x4 b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) b[u] = ld4(Bs + u * 32 * KM_LDT + k8 * 8);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[u][i], acc[u], 0, 0, 0);
            }
        }
        // the finished tile, where it lies: acc[u][r] is row km_acc_row(r, kh) of the wave, column 128 t + 32 u + l32
        float h[4];
        int cj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cj[u] = t * KM_BN + u * 32 + l32;
            h[u] = hn[cj[u]];                                   // cj < kp
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = -INFINITY;
            int j = 0x7fffffff;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float vu = acc[u][r] - h[u];
                if (vu != vu) vu = -INFINITY;
                if (cj[u] < k) km_better(v, j, vu, cj[u]);
            }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {                  // over the 32 lanes of this half: the row's other columns
                const float v2 = __shfl_xor(v, o, 64);
                const int j2 = __shfl_xor(j, o, 64);
                km_better(v, j, v2, j2);
            }
            km_better(bv[r], bj[r], v, j);
        }
    }
#undef KM_FETCH
    // a row's norm: the chains of the 8 threads that loaded it, by a fixed tree
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            xn[p] += __shfl_xor(xn[p], o, 64);
            bad[p] |= __shfl_xor(bad[p], o, 64);
        }
        if ((tid & 7) == 0) {
            s_xn[lr + 32 * p] = xn[p];
            s_bad[lr + 32 * p] = bad[p];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (l32 == r) {                                         // every lane of the half holds the row's result; lane r writes it
            const int row = wave * 32 + km_acc_row(r, kh);
            int chg = 0;
            float dpos = 0.f;
            if (row < rows) {
                const int64_t p = p0 + row;
                const bool b = s_bad[row] != 0;
                const int lab = b ? -1 : bj[r];
                const float d = b ? nanf32() : s_xn[row] - 2.f * bv[r];
                chg = (!b && labels[p] != lab) ? 1 : 0;
                dpos = b ? 0.f : fmaxf(d, 0.f);
                labels[p] = lab;
                dist[p] = d;
            }
            s_chg[row] = chg;
            s_d[row] = dpos;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double a = (double)s_d[lane] + (double)s_d[lane + 64];
        int c = s_chg[lane] + s_chg[lane + 64];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            c += __shfl_xor(c, o, 64);
        }
        if (lane == 0) {
            pchg[w] = c;
            pin[w] = a;
        }
    }
}

// stats = {sum of pchg (int64), sum of pin in chunk order (double)}.  One workgroup.
__global__ __launch_bounds__(KM_THREADS) void km_assign_finish(const int32_t* __restrict__ pchg, const double* __restrict__ pin,
                                                               int64_t n_chunks, int64_t* __restrict__ stats) {
    __shared__ double s_in[KM_THREADS];
    __shared__ int64_t s_c[KM_THREADS];
    const int tid = (int)threadIdx.x;
    double total = 0.0;
    int64_t mine = 0;
    for (int64_t b = 0; b < n_chunks; b += KM_THREADS) {
        const int64_t i = b + tid;
        s_in[tid] = i < n_chunks ? pin[i] : 0.0;
        if (i < n_chunks) mine += pchg[i];
        __syncthreads();
        if (tid == 0) {
            const int cnt = n_chunks - b < KM_THREADS ? (int)(n_chunks - b) : KM_THREADS;
            for (int e = 0; e < cnt; ++e) total += s_in[e];
        }
        __syncthreads();
    }
    s_c[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int64_t c = 0;
        for (int e = 0; e < KM_THREADS; ++e) c += s_c[e];
        stats[0] = c;
        stats[1] = __double_as_longlong(total);
    }
}

// ---- K2: update -------------------------------------------------------------------------------------------------------------------
// cnt [k, nsc]: the labels of positions c * KM_SORT .. of sort chunk c
__global__ __launch_bounds__(KM_THREADS) void km_sort_hist(const int32_t* __restrict__ labels, int64_t T, int k, int nsc,
                                                           int32_t* __restrict__ cnt) {
    __shared__ int hist[MDL_KM_MAX_K];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    for (int j = tid; j < k; j += KM_THREADS) hist[j] = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)c * KM_SORT;
    for (int e = tid; e < KM_SORT; e += KM_THREADS) {
        const int64_t p = p0 + e;
        if (p < T) {
            const int l = labels[p];
            if (l >= 0 && l < k) atomicAdd(&hist[l], 1);
        }
    }
    __syncthreads();
    for (int j = tid; j < k; j += KM_THREADS) cnt[(int64_t)j * nsc + c] = hist[j];
}

// cnt -> its exclusive prefix in (label, chunk) order, in place; counts [k], cstart [k], item_cu [k + 1] (the prefix of
// ceil(count / KM_MEAN)).  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void km_sort_scan(int32_t* __restrict__ cnt, int k, int nsc, int64_t* __restrict__ counts,
                                                      int32_t* __restrict__ cstart, int32_t* __restrict__ item_cu) {
    __shared__ int s_sum[1024];
    __shared__ int s_total;
    const int tid = (int)threadIdx.x;
    const int64_t N = (int64_t)k * nsc, per = (N + 1023) / 1024;
    const int64_t a = tid * per < N ? tid * per : N, b = a + per < N ? a + per : N;
    int sum = 0;
    for (int64_t e = a; e < b; ++e) sum += cnt[e];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int e = 0; e < 1024; ++e) {
            const int v = s_sum[e];
            s_sum[e] = run;
            run += v;
        }
        s_total = run;
    }
    __syncthreads();
    int run = s_sum[tid];
    for (int64_t e = a; e < b; ++e) {
        const int v = cnt[e];
        cnt[e] = run;
        run += v;
    }
    __threadfence_block();
    __syncthreads();
    for (int j = tid; j < k; j += 1024) {
        const int st = cnt[(int64_t)j * nsc];
        const int en = j + 1 < k ? cnt[(int64_t)(j + 1) * nsc] : s_total;
        cstart[j] = st;
        counts[j] = en - st;
        s_sum[j] = (en - st + KM_MEAN - 1) / KM_MEAN;
    }
    __syncthreads();
    if (tid == 0) {
        int it = 0;
        for (int j = 0; j < k; ++j) {
            item_cu[j] = it;
            it += s_sum[j];
        }
        item_cu[k] = it;
    }
}

// mrow [T]: the store rows of the call positions, sorted by label and, inside a label, by position (-1: a position the tables do not place)
__global__ __launch_bounds__(KM_THREADS) void km_sort_scatter(Src s, const int32_t* __restrict__ labels, int k, int nsc,
                                                              const int32_t* __restrict__ offs, int64_t* __restrict__ mrow) {
    __shared__ int base[MDL_KM_MAX_K];
    __shared__ int s_lab[KM_THREADS];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    for (int j = tid; j < k; j += KM_THREADS) base[j] = offs[(int64_t)j * nsc + c];
    const int64_t p0 = (int64_t)c * KM_SORT;
    for (int sb = 0; sb < KM_SORT; sb += KM_THREADS) {
        const int64_t p = p0 + sb + tid;
        int l = -1;
        if (p < s.T) {
            l = labels[p];
            if (l < 0 || l >= k) l = -1;
        }
        __syncthreads();                                        // base is set; the previous sub-block's s_lab has been read
        s_lab[tid] = l;
        __syncthreads();
        int before = 0, after = 0;
        if (l >= 0) {
            for (int e = 0; e < KM_THREADS; ++e) {
                const int same = s_lab[e] == l ? 1 : 0;
                before += e < tid ? same : 0;
                after += e > tid ? same : 0;
            }
            const int dest = base[l] + before;
            if (dest >= 0 && dest < s.T) mrow[dest] = place_position(s, p);
        }
        __syncthreads();
        if (l >= 0 && after == 0) base[l] += before + 1;        // the label's last position of the sub-block moves its base
    }
}

// lanes that cover one member row: a power of two, a function of D alone (S5's)
__device__ __forceinline__ int km_lanes_per_row(int D) {
    const int ns = (D + 7) / 8;
    int lpr = 1;
    while (lpr < ns && lpr < KM_THREADS) lpr <<= 1;
    return lpr;
}

// item w = (cluster j, member chunk c): the float partial column sums of members c * KM_MEAN .. of j -> part [w, D]
template <class T, bool VEC>
__global__ __launch_bounds__(KM_THREADS) void km_mean_partial(Src s, int k, const int64_t* __restrict__ counts,
                                                              const int32_t* __restrict__ cstart, const int32_t* __restrict__ item_cu,
                                                              const int64_t* __restrict__ mrow, float* __restrict__ part) {
    __shared__ float s_part[KM_THREADS * 8];
    const int tid = (int)threadIdx.x, D = s.D;
    const int w = (int)blockIdx.x;
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (item_cu[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const int j = lo, c = w - item_cu[j];
    const int64_t cntj = counts[j];
    if (c < 0 || c >= (cntj + KM_MEAN - 1) / KM_MEAN) return;   // uniform: not an item (the grid is an upper bound)
    const int64_t m0 = (int64_t)cstart[j] + (int64_t)c * KM_MEAN;
    const int rows = cntj - (int64_t)c * KM_MEAN < KM_MEAN ? (int)(cntj - (int64_t)c * KM_MEAN) : KM_MEAN;
    if (m0 < 0 || m0 + rows > s.T) return;
    const int lpr = km_lanes_per_row(D), G = KM_THREADS / lpr, grp = tid / lpr, s0 = tid - grp * lpr;
    const int ns = (D + 7) / 8;
    const T* __restrict__ store = static_cast<const T*>(s.store);
    float* __restrict__ out = part + (int64_t)w * D;
    for (int sb = 0; sb < ns; sb += lpr) {                      // one pass unless D > 2048
        const int sl = sb + s0, col = sl * 8;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        f32x4 a0 = z, a1 = z;
        if (sl < ns) {
            for (int t0 = grp; t0 < rows; t0 += 4 * G) {
                f32x4 v0[4], v1[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int t = t0 + q * G;
                    v0[q] = z;
                    v1[q] = z;
                    if (t < rows) {
                        const int64_t a = mrow[m0 + t];
                        if (a >= 0 && a < s.T_total) {
                            const T* row = store + a * s.row_stride;
                            v0[q] = load4<T, VEC>(row, col, D);
                            v1[q] = load4<T, VEC>(row, col + 4, D);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (t0 + q * G < rows) {                    // in member order
                        a0 += v0[q];
                        a1 += v1[q];
                    }
            }
        }
        st4(s_part + tid * 8, a0);
        st4(s_part + tid * 8 + 4, a1);
        __syncthreads();
        for (int e = tid; e < lpr * 8; e += KM_THREADS) {       // column sb * 8 + e: its G group sums, in group order
            if (sb * 8 + e < D) {
                float sum = s_part[e];
                for (int gg = 1; gg < G; ++gg) sum += s_part[gg * lpr * 8 + e];
                out[sb * 8 + e] = sum;
            }
        }
        __syncthreads();
    }
}

// C_out[j] = (the partials of cluster j, added in chunk order in double) / count, rounded once; C_in[j] for a cluster of no member
__global__ __launch_bounds__(KM_THREADS) void km_mean_combine(int D, const int64_t* __restrict__ counts, const int32_t* __restrict__ item_cu,
                                                              const float* __restrict__ part, const float* C_in, float* C_out) {
    const int j = (int)blockIdx.x;
    const int64_t n = counts[j];
    const int i0 = item_cu[j], nc = (int)((n + KM_MEAN - 1) / KM_MEAN);
    for (int col = (int)threadIdx.x; col < D; col += KM_THREADS) {
        float o = C_in[(int64_t)j * D + col];
        if (n > 0) {
            double sum = 0.0;
            for (int c = 0; c < nc; ++c) sum += (double)part[(int64_t)(i0 + c) * D + col];
            o = (float)(sum / (double)n);
        }
        C_out[(int64_t)j * D + col] = o;
    }
}

// ---- K3: seed ---------------------------------------------------------------------------------------------------------------------
struct SeedWs {
    float* mind;             // [T]
    uint8_t* fin;            // [T]
    double* csum;            // [n_chunks]
    int32_t* ccnt;           // [n_chunks]
};

// FIRST: fin, ccnt and mind = 0.  Otherwise: mind <- min(mind, |x - c|^2) (taken == 1: mind <- the distance) and csum.  A wave per row.
template <class T, bool FIRST>
__global__ __launch_bounds__(KM_THREADS) void km_seed_dist(Src s, SeedWs ws, const float* __restrict__ cen, int taken) {
    __shared__ float s_m[KM_ROWS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t w = blockIdx.x;
    int64_t first, p0;
    const int rows = place_chunk(s, w, first, p0);
    if (rows == 0) {
        if (tid == 0) {
            if (FIRST) ws.ccnt[w] = 0; else ws.csum[w] = 0.0;
        }
        return;
    }
    const int D = s.D;
    for (int i = 0; i < 32; ++i) {
        const int row = wave * 32 + i;                          // uniform in the wave
        float m = 0.f;
        if (row < rows) {
            const T* __restrict__ x = static_cast<const T*>(s.store) + (first + row) * s.row_stride;
            if (FIRST) {
                int bad = 0;
                for (int c = lane; c < D; c += 64) bad |= km_finite(up(x[c])) ? 0 : 1;
                const bool f = __ballot(bad != 0) == 0;
                if (lane == 0) {
                    ws.fin[p0 + row] = f ? 1 : 0;
                    ws.mind[p0 + row] = 0.f;
                }
                m = f ? 1.f : 0.f;
            } else if (ws.fin[p0 + row]) {
                float d = 0.f;
                for (int c = lane; c < D; c += 64) {
                    const float e = up(x[c]) - cen[c];
                    d = fmaf(e, e, d);
                }
                d = wave_sum(d);
                m = taken == 1 ? d : fminf(ws.mind[p0 + row], d);
                if (!(m >= 0.f)) m = 0.f;                        // a NaN distance (a non-finite centre cannot be chosen, an overflow can)
                if (lane == 0) ws.mind[p0 + row] = m;
            }
        }
        if (lane == 0) s_m[row] = m;
    }
    __syncthreads();
    if (wave == 0) {
        double a = (double)s_m[lane] + (double)s_m[lane + 64];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) {
            if (FIRST) ws.ccnt[w] = (int)a; else ws.csum[w] = a;
        }
    }
}

// centre j: its call position -> pos_out[j], its row -> C_out[j].  One workgroup; thread 0 walks slices, chunks and rows in order.
template <class T>
__global__ __launch_bounds__(KM_THREADS) void km_seed_pick(Src s, SeedWs ws, const double* __restrict__ u, int j, int64_t* __restrict__ pos_out,
                                                           float* __restrict__ C_out) {
    __shared__ double s_sum[KM_SLICES];
    __shared__ int64_t s_cnt[KM_SLICES];
    __shared__ int64_t s_row;
    const int tid = (int)threadIdx.x;
    const int64_t nch = s.n_chunks, per = (nch + KM_SLICES - 1) / KM_SLICES;
    const int64_t a = tid * per < nch ? tid * per : nch, b = a + per < nch ? a + per : nch;
    double sum = 0.0;
    int64_t cnt = 0;
    for (int64_t c = a; c < b; ++c) {
        if (j > 0) sum += ws.csum[c];
        cnt += ws.ccnt[c];
    }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        int64_t tfin = 0;
        for (int e = 0; e < KM_SLICES; ++e) {
            total += s_sum[e];
            tfin += s_cnt[e];
        }
        const double uj = u[j];
        int64_t pos = -1, srow = -1;
        if (j > 0 && total > 0.0) {                             // D^2 sampling: the first position whose inclusive prefix exceeds target
            const double target = uj * total;
            double run = 0.0;
            int sl = -1, lastp = -1;
            for (int e = 0; e < KM_SLICES; ++e) {
                if (s_sum[e] > 0.0) lastp = e;
                if (run + s_sum[e] > target) {
                    sl = e;
                    break;
                }
                run += s_sum[e];
            }
            bool fallback = sl < 0;                             // rounding only: the last position of positive mind
            if (fallback) sl = lastp;
            const int64_t ca = sl * per, cb = ca + per < nch ? ca + per : nch;
            int64_t ch = -1, lastc = -1;
            for (int64_t c = ca; c < cb; ++c) {
                const double v = ws.csum[c];
                if (v > 0.0) lastc = c;
                if (!fallback && run + v > target) {
                    ch = c;
                    break;
                }
                run += v;
            }
            if (ch < 0) {
                fallback = true;
                ch = lastc;
            }
            int64_t first, p0;
            const int rows = ch >= 0 ? place_chunk(s, ch, first, p0) : 0;
            int hit = -1, lastr = -1;
            for (int i = 0; i < rows; ++i) {
                const float m = ws.mind[p0 + i];
                if (m > 0.f) lastr = i;
                run += (double)m;
                if (!fallback && run > target) {
                    hit = i;
                    break;
                }
            }
            if (hit < 0) hit = lastr;
            if (hit >= 0) {
                pos = p0 + hit;
                srow = first + hit;
            }
        } else if (tfin > 0) {                                   // the finite row of rank floor(u * T_finite)
            int64_t rank = (int64_t)(uj * (double)tfin);
            if (rank < 0) rank = 0;
            if (rank > tfin - 1) rank = tfin - 1;
            int sl = 0;
            while (sl < KM_SLICES - 1 && rank >= s_cnt[sl]) rank -= s_cnt[sl++];
            const int64_t ca = sl * per, cb = ca + per < nch ? ca + per : nch;
            int64_t ch = ca;
            while (ch < cb - 1 && rank >= ws.ccnt[ch]) rank -= ws.ccnt[ch++];
            int64_t first, p0;
            const int rows = place_chunk(s, ch, first, p0);
            for (int i = 0; i < rows; ++i) {
                if (ws.fin[p0 + i]) {
                    if (rank == 0) {
                        pos = p0 + i;
                        srow = first + i;
                        break;
                    }
                    --rank;
                }
            }
        }
        s_row = srow;
        pos_out[j] = pos;
    }
    __syncthreads();
    const int64_t srow = s_row;
    float* __restrict__ o = C_out + (int64_t)j * s.D;
    for (int c = tid; c < s.D; c += KM_THREADS)
        o[c] = srow >= 0 ? up(static_cast<const T*>(s.store)[srow * s.row_stride + c]) : nanf32();
}

// ---- K4: hist ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KM_THREADS) void km_hist_kernel(const int32_t* __restrict__ labels, const int64_t* __restrict__ cu, int64_t T,
                                                             int k, int32_t* __restrict__ counts) {
    __shared__ int hist[MDL_KM_MAX_K];
    const int tid = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    for (int j = tid; j < k; j += KM_THREADS) hist[j] = 0;
    __syncthreads();
    int64_t a = cu[r], b = cu[r + 1];
    if (a < 0) a = 0;
    if (b > T) b = T;
    for (int64_t p = a + tid; p < b; p += KM_THREADS) {
        const int l = labels[p];
        if (l >= 0 && l < k) atomicAdd(&hist[l], 1);
    }
    __syncthreads();
    for (int j = tid; j < k; j += KM_THREADS) counts[r * k + j] = hist[j];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
inline int64_t pad256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// The one check of the sizes of every entry point and query (the header's (1) and (2)); a size a call does not have is passed as 1 / 0.
int km_check_sizes(int64_t R, int64_t n_chunks, int64_t T, int64_t D, int64_t k) {
    if (R < 0 || n_chunks < 0 || T < 1 || D < 1 || k < 1) return MDL_E_ARG;
    if (k > MDL_KM_MAX_K || !i32(R) || !i32(T) || !i32(n_chunks) || D > 0x7FFFFFFF - KM_BK) return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

// The row source of K1-K3: the header's (1), (2), (3) in that order.
int km_check(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags, const int32_t* bag,
             const int64_t* cu, const int64_t* chunk_cu, bool chunked, int64_t R, int64_t n_chunks, int64_t T, int D, int k, Src& s) {
    if (!store || !off || !bag || !cu || (chunked && !chunk_cu) || T_total < 0 || n_bags < 0 || row_stride < D) return MDL_E_ARG;
    if (dtype != MDL_STORE_F32 && dtype != MDL_STORE_F16 && dtype != MDL_STORE_BF16) return MDL_E_ARG;
    if (const int rc = km_check_sizes(R, n_chunks, T, D, k)) return rc;
    if (!host_aligned16(store) || !aligned_to(off, 8) || !aligned_to(cu, 8) || !aligned_to(chunk_cu, 8) || !aligned_to(bag, 4))
        return MDL_E_ALIGN;
    s = Src{store, row_stride, T_total, off, n_bags, bag, cu, chunk_cu, (int)R, n_chunks, T, D};
    return MDL_OK;
}

inline bool vec_ok(const Src& s) { return s.D % 4 == 0 && s.row_stride % 4 == 0; }

struct AssignWs {
    float *Cp, *hn;
    int32_t* pchg;
    double* pin;
    int64_t bytes;
    int kp, dp;
};
inline AssignWs carve_assign(void* ws, int64_t n_chunks, int k, int D) {
    AssignWs a;
    a.kp = (k + KM_BN - 1) / KM_BN * KM_BN;
    a.dp = (D + KM_BK - 1) / KM_BK * KM_BK;
    char* base = (char*)ws;
    int64_t o = 0;
    a.Cp = (float*)(base + o);
    o += pad256((int64_t)a.kp * a.dp * 4);
    a.hn = (float*)(base + o);
    o += pad256((int64_t)a.kp * 4);
    a.pin = (double*)(base + o);
    o += pad256(n_chunks * 8);
    a.pchg = (int32_t*)(base + o);
    o += pad256(n_chunks * 4);
    a.bytes = o;
    return a;
}

struct UpdateWs {
    int32_t *cnt, *cstart, *item_cu;
    int64_t* mrow;
    float* part;
    int64_t bytes;
    int nsc, max_items;
};
inline UpdateWs carve_update(void* ws, int64_t T, int k, int D) {
    UpdateWs a;
    a.nsc = (int)((T + KM_SORT - 1) / KM_SORT);
    a.max_items = (int)(T / KM_MEAN) + k;
    char* base = (char*)ws;
    int64_t o = 0;
    a.cnt = (int32_t*)(base + o);
    o += pad256((int64_t)k * a.nsc * 4);
    a.cstart = (int32_t*)(base + o);
    o += pad256((int64_t)k * 4);
    a.item_cu = (int32_t*)(base + o);
    o += pad256((int64_t)(k + 1) * 4);
    a.mrow = (int64_t*)(base + o);
    o += pad256(T * 8);
    a.part = (float*)(base + o);
    o += pad256((int64_t)a.max_items * D * 4);
    a.bytes = o;
    return a;
}

inline SeedWs carve_seed(void* ws, int64_t n_chunks, int64_t T, int64_t& bytes) {
    SeedWs a;
    char* base = (char*)ws;
    int64_t o = 0;
    a.csum = (double*)(base + o);
    o += pad256(n_chunks * 8);
    a.ccnt = (int32_t*)(base + o);
    o += pad256(n_chunks * 4);
    a.mind = (float*)(base + o);
    o += pad256(T * 4);
    a.fin = (uint8_t*)(base + o);
    o += pad256(T);
    bytes = o;
    return a;
}

#define KM_LAUNCH(kernel, grid, block, ...)                                                     \
    do {                                                                                        \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);     \
        MDL_LAUNCH_CHECK();                                                                     \
    } while (0)
// the element type (and, where the kernel has the two forms, the access width) of a call
#define KM_BY_DTYPE(dtype, CALL)                  \
    do {                                          \
        if ((dtype) == MDL_STORE_F32) CALL(float);  \
        else if ((dtype) == MDL_STORE_F16) CALL(_Float16); \
        else CALL(bf16_t);                        \
    } while (0)

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_kmeans_assign_ws_bytes(int64_t n_chunks, int k, int D) {
    if (const int rc = km_check_sizes(0, n_chunks, 1, D, k)) return rc;
    return carve_assign(nullptr, n_chunks, k, D).bytes;
}

extern "C" int mdl_kmeans_assign(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                                 const int32_t* bag, const int64_t* cu, const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int64_t T,
                                 int D, const float* C, int k, int32_t* labels, float* dist, void* stats, void* ws, void* stream) {
    if (!C || !labels || !dist || !stats || !ws) return MDL_E_ARG;
    Src s;
    if (const int rc = km_check(store, dtype, row_stride, T_total, off, n_bags, bag, cu, chunk_cu, true, R, n_chunks, T, D, k, s)) return rc;
    if (!host_aligned16(C) || !host_aligned16(ws) || !aligned_to(stats, 8) || !aligned_to(labels, 4) || !aligned_to(dist, 4))
        return MDL_E_ALIGN;
    const AssignWs a = carve_assign(ws, n_chunks, k, D);
    if (R > 0 && n_chunks > 0) {
        KM_LAUNCH(km_prep_kernel, dim3((unsigned)a.kp), 64, C, k, D, a.dp, a.Cp, a.hn);
        const dim3 grid((unsigned)n_chunks);
        const int col_tiles = a.kp / KM_BN;
#define KM_ASSIGN(T_)                                                                                                              \
    do {                                                                                                                           \
        if (vec_ok(s))                                                                                                             \
            KM_LAUNCH((km_assign_kernel<T_, true>), grid, KM_THREADS, s, (const float*)a.Cp, (const float*)a.hn, a.dp, k, col_tiles, \
                      labels, dist, a.pchg, a.pin);                                                                                \
        else                                                                                                                       \
            KM_LAUNCH((km_assign_kernel<T_, false>), grid, KM_THREADS, s, (const float*)a.Cp, (const float*)a.hn, a.dp, k, col_tiles, \
                      labels, dist, a.pchg, a.pin);                                                                                \
    } while (0)
        KM_BY_DTYPE(dtype, KM_ASSIGN);
#undef KM_ASSIGN
    }
    KM_LAUNCH(km_assign_finish, dim3(1), KM_THREADS, (const int32_t*)a.pchg, (const double*)a.pin, R > 0 ? n_chunks : 0, (int64_t*)stats);
    return MDL_OK;
}

extern "C" int64_t mdl_kmeans_update_ws_bytes(int64_t T, int k, int D) {
    if (const int rc = km_check_sizes(0, 0, T, D, k)) return rc;
    return carve_update(nullptr, T, k, D).bytes;
}

extern "C" int mdl_kmeans_update(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                                 const int32_t* bag, const int64_t* cu, int64_t R, int64_t T, int D, const int32_t* labels,
                                 const float* C_in, int k, float* C_out, int64_t* counts, void* ws, void* stream) {
    if (!labels || !C_in || !C_out || !counts || !ws) return MDL_E_ARG;
    Src s;
    if (const int rc = km_check(store, dtype, row_stride, T_total, off, n_bags, bag, cu, nullptr, false, R, 0, T, D, k, s)) return rc;
    if (!host_aligned16(C_in) || !host_aligned16(C_out) || !host_aligned16(ws) || !aligned_to(counts, 8) || !aligned_to(labels, 4))
        return MDL_E_ALIGN;
    const UpdateWs a = carve_update(ws, T, k, D);
    KM_LAUNCH(km_sort_hist, dim3((unsigned)a.nsc), KM_THREADS, labels, T, k, a.nsc, a.cnt);
    KM_LAUNCH(km_sort_scan, dim3(1), 1024, a.cnt, k, a.nsc, counts, a.cstart, a.item_cu);
    KM_LAUNCH(km_sort_scatter, dim3((unsigned)a.nsc), KM_THREADS, s, labels, k, a.nsc, (const int32_t*)a.cnt, a.mrow);
#define KM_MEAN_CALL(T_)                                                                                                            \
    do {                                                                                                                            \
        if (vec_ok(s))                                                                                                              \
            KM_LAUNCH((km_mean_partial<T_, true>), dim3((unsigned)a.max_items), KM_THREADS, s, k, (const int64_t*)counts,           \
                      (const int32_t*)a.cstart, (const int32_t*)a.item_cu, (const int64_t*)a.mrow, a.part);                         \
        else                                                                                                                        \
            KM_LAUNCH((km_mean_partial<T_, false>), dim3((unsigned)a.max_items), KM_THREADS, s, k, (const int64_t*)counts,          \
                      (const int32_t*)a.cstart, (const int32_t*)a.item_cu, (const int64_t*)a.mrow, a.part);                         \
    } while (0)
    KM_BY_DTYPE(dtype, KM_MEAN_CALL);
#undef KM_MEAN_CALL
    KM_LAUNCH(km_mean_combine, dim3((unsigned)k), KM_THREADS, D, (const int64_t*)counts, (const int32_t*)a.item_cu, (const float*)a.part,
              C_in, C_out);
    return MDL_OK;
}

extern "C" int64_t mdl_kmeans_seed_ws_bytes(int64_t n_chunks, int64_t T) {
    if (const int rc = km_check_sizes(0, n_chunks, T, 1, 1)) return rc;
    int64_t bytes;
    carve_seed(nullptr, n_chunks, T, bytes);
    return bytes;
}

extern "C" int mdl_kmeans_seed(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                               const int32_t* bag, const int64_t* cu, const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int64_t T,
                               int D, const void* u, int k, int64_t* pos_out, float* C_out, void* ws, void* stream) {
    if (!u || !pos_out || !C_out || !ws) return MDL_E_ARG;
    Src s;
    if (const int rc = km_check(store, dtype, row_stride, T_total, off, n_bags, bag, cu, chunk_cu, true, R, n_chunks, T, D, k, s)) return rc;
    if (T < k || R < 1 || n_chunks < 1) return MDL_E_ARG;
    if (!host_aligned16(C_out) || !host_aligned16(ws) || !aligned_to(u, 8) || !aligned_to(pos_out, 8)) return MDL_E_ALIGN;
    int64_t bytes;
    const SeedWs a = carve_seed(ws, n_chunks, T, bytes);
    const dim3 grid((unsigned)n_chunks);
    const double* ud = (const double*)u;
#define KM_SEED(T_)                                                                                                     \
    do {                                                                                                                \
        KM_LAUNCH((km_seed_dist<T_, true>), grid, KM_THREADS, s, a, (const float*)C_out, 0);                            \
        KM_LAUNCH((km_seed_pick<T_>), dim3(1), KM_THREADS, s, a, ud, 0, pos_out, C_out);                                \
        for (int j = 1; j < k; ++j) {                                                                                   \
            KM_LAUNCH((km_seed_dist<T_, false>), grid, KM_THREADS, s, a, (const float*)(C_out + (int64_t)(j - 1) * D), j); \
            KM_LAUNCH((km_seed_pick<T_>), dim3(1), KM_THREADS, s, a, ud, j, pos_out, C_out);                            \
        }                                                                                                               \
    } while (0)
    KM_BY_DTYPE(dtype, KM_SEED);
#undef KM_SEED
    return MDL_OK;
}

extern "C" int64_t mdl_kmeans_hist_ws_bytes(int64_t R, int k) {
    if (const int rc = km_check_sizes(R, 0, 1, 1, k)) return rc;
    return 0;
}

extern "C" int mdl_kmeans_hist(const int32_t* labels, const int64_t* cu, int64_t R, int64_t T, int k, int32_t* counts, void* stream) {
    if (!labels || !cu || !counts) return MDL_E_ARG;
    if (const int rc = km_check_sizes(R, 0, T, 1, k)) return rc;
    if (!aligned_to(cu, 8) || !aligned_to(labels, 4) || !aligned_to(counts, 4)) return MDL_E_ALIGN;
    if (R > 0) KM_LAUNCH(km_hist_kernel, dim3((unsigned)R), KM_THREADS, labels, cu, T, k, counts);
    return MDL_OK;
}
