// bag_sample.hip -- draw and gather one batch of bags from a device-resident feature store (S1 of the header): SlideDataset.sample_n,
// the zero bag of an absent stain and collate's stack in ONE launch, with no host draw and no host-to-device copy of features.
//
// Work split.  Workgroup (r, c) owns tokens c * 64 .. c * 64 + 63 of output row r.  Wave 0 draws: lane l computes the bag row of token
// c * 64 + l -- ONCE per output row, by one lane -- and leaves it in LDS (and in idx_out).  After the barrier the four waves copy the
// 64 rows: a row is read by min(64, next_pow2(16-byte vectors per row)) adjacent lanes, BS_INFLIGHT rows in flight per lane.
//
// The draw is a pure function of (seed, counter, key_id[r], n): two 32-bit row keys are hashed from the three 64-bit words with mix32
// (common.hpp); nothing depends on R, on r or on the other rows of the launch.
//   n < N   (with replacement)  token t takes row (h * n) >> 32 with h = mix32(mix32(t ^ ka) + kb).
//   n >= N, n <= 64             random-key sort inside wave 0: lane i < n hashes its index, its rank among the n hashes (ties by lane)
//                               is its position, and positions < N are kept.  A uniformly random order of the bag, cut at N.
//                               (A Feistel network cannot serve these: halves of 1-3 bits do not mix, its statistics fail at n = 5.)
//   n >= N, n > 64              a keyed bijection F of [0, 2^b), b the smallest even width with 2^b >= n (so 2^b < 4 n): a balanced
//                               Feistel network of FEISTEL_ROUNDS rounds, round function mix32 under per-round keys.  Token t < N <= n
//                               takes y = F(t), and while y >= n, y = F(y) (cycle walking).  t -> y is then a bijection of [0, n):
//                               distinct tokens take distinct rows, with no memory and no host.
// Termination of the walk.  F is a permutation of the finite set [0, 2^b), so the orbit t, F(t), F(F(t)), ... is a cycle that returns
// to its start t.  t lies in [0, n); the walk stops at the first element of the cycle inside [0, n), and t itself is one: it stops
// after at most (cycle length) <= 2^b steps, 2^b / n < 4 in expectation.  There is deliberately no iteration cap -- cutting a walk
// short would map two tokens to one row.
//
// Bounds.  A bag index outside [0, n_bags), an empty or over-long bag and a bag that leaves [0, T_total) are written as absent stains
// (zeros, idx -1): whatever the tables hold, no address outside the store is formed.
#include "common.hpp"

namespace mdl {
namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_TOK = 64;                  // tokens per workgroup = lanes of the drawing wave
constexpr int BS_WAVES = BS_THREADS / WAVE;
constexpr int FEISTEL_ROUNDS = 6;
static_assert(BS_TOK == WAVE, "wave 0 draws one token per lane, and the random-key sort of a small bag needs the whole bag in one wave");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

struct RowKey {
    uint32_t a, b;
};

// two 32-bit keys from (seed, counter, key_id): a chain of mix32 over the six words, from two different starts
__device__ __forceinline__ RowKey row_key(uint64_t seed, uint64_t counter, uint64_t key_id) {
    const uint32_t w[6] = {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)key_id,
                           (uint32_t)(key_id >> 32)};
    RowKey k = {0x243F6A88u, 0x85A308D3u};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        k.a = mix32(k.a ^ w[i]) + 0x9E3779B9u;
        k.b = mix32(k.b + w[i]) ^ 0x7F4A7C15u;
    }
    k.a = mix32(k.a);
    k.b = mix32(k.b ^ k.a);
    return k;
}

__device__ __forceinline__ uint32_t token_hash(uint32_t t, RowKey k) { return mix32(mix32(t ^ k.a) + k.b); }

// F: one pass of the balanced Feistel network over 2 * half bits
__device__ __forceinline__ uint32_t feistel(uint32_t x, int half, RowKey k) {
    const uint32_t mask = (1u << half) - 1u;
    uint32_t L = x >> half, Rr = x & mask;
#pragma unroll
    for (int i = 0; i < FEISTEL_ROUNDS; ++i) {
        const uint32_t rk = k.a + (uint32_t)i * 0x9E3779B9u;
        const uint32_t f = mix32(mix32(Rr ^ rk) + k.b) & mask;
        const uint32_t nl = Rr;
        Rr = L ^ f;
        L = nl;
    }
    return (L << half) | Rr;
}

#ifndef BS_INFLIGHT
#define BS_INFLIGHT 4                       // rows a lane has in flight in the 16-byte copy loop (1 / 2 / 4 / 8 measured: DESIGN 3.10)
#endif

// 16 bytes of a store row <-> the fp32 values they hold
template <class T>
struct Vec;
template <>
struct Vec<float> {
    static constexpr int E = 4;      // elements per 16-byte access of the store
    typedef f32x4 Raw;
    static __device__ __forceinline__ Raw ld(const float* src) { return ld4(src); }
    static __device__ __forceinline__ void st(float* dst, Raw v) { st4(dst, v); }
    static __device__ __forceinline__ float up(float x) { return x; }
};
template <>
struct Vec<_Float16> {
    static constexpr int E = 8;
    typedef f16x8 Raw;
    static __device__ __forceinline__ Raw ld(const _Float16* src) { return *reinterpret_cast<const f16x8*>(src); }
    static __device__ __forceinline__ void st(float* dst, Raw raw) {
        const f32x8 v = __builtin_convertvector(raw, f32x8);
        st4(dst, v.lo);
        st4(dst + 4, v.hi);
    }
    static __device__ __forceinline__ float up(_Float16 x) { return (float)x; }
};
template <>
struct Vec<bf16_t> {
    static constexpr int E = 8;
    typedef bf16x8 Raw;
    static __device__ __forceinline__ Raw ld(const bf16_t* src) { return *reinterpret_cast<const bf16x8*>(src); }
    static __device__ __forceinline__ void st(float* dst, Raw raw) {
        const f32x8 v = __builtin_convertvector(raw, f32x8);
        st4(dst, v.lo);
        st4(dst + 4, v.hi);
    }
    static __device__ __forceinline__ float up(bf16_t x) { return (float)x; }
};

// VEC: D and row_stride are multiples of Vec<T>::E and both bases are 16-byte aligned, so every row of both sides is.
template <class T, bool VEC>
__global__ __launch_bounds__(BS_THREADS) void bag_sample_kernel(const T* __restrict__ store, int64_t row_stride, int64_t T_total,
                                                                const int64_t* __restrict__ off, int64_t n_bags,
                                                                const int32_t* __restrict__ bag, const int64_t* __restrict__ key_id,
                                                                int N, int D, int chunks, uint64_t seed, uint64_t counter,
                                                                float* __restrict__ out, int32_t* __restrict__ idx_out) {
    __shared__ int32_t s_idx[BS_TOK];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int r = blockIdx.x / chunks, t0 = (blockIdx.x - r * chunks) * BS_TOK;
    const int cnt = N - t0 < BS_TOK ? N - t0 : BS_TOK;        // tokens of this workgroup, >= 1

    const int g = bag[r];
    int64_t base = 0, n64 = 0;
    if (g >= 0 && g < n_bags) {
        base = off[g];
        n64 = off[g + 1] - base;
        if (base < 0 || n64 < 1 || n64 > 0x7FFFFFFF || base > T_total - n64) n64 = 0;
    }
    const uint32_t n = (uint32_t)n64;                           // 0: an absent stain
    float* orow = out + ((int64_t)r * N + t0) * D;

    if (n == 0) {                                               // uniform over the workgroup
        const int64_t total = (int64_t)cnt * D;
        if (VEC) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            for (int64_t e = (int64_t)tid * 4; e < total; e += BS_THREADS * 4) st4(orow + e, z);
        } else {
            for (int64_t e = tid; e < total; e += BS_THREADS) orow[e] = 0.f;
        }
        if (idx_out != nullptr && tid < cnt) idx_out[(int64_t)r * N + t0 + tid] = -1;
        return;
    }

    if (wave == 0) {
        const RowKey k = row_key(seed, counter, key_id != nullptr ? (uint64_t)key_id[r] : (uint64_t)(int64_t)g);
        const uint32_t t = (uint32_t)(t0 + lane);
        if (n < (uint32_t)N) {                                  // with replacement
            s_idx[lane] = (int32_t)(((uint64_t)token_hash(t, k) * n) >> 32);
        } else if (n <= (uint32_t)WAVE) {                       // N <= n <= 64: one chunk (t0 == 0), random-key sort in the wave
            const uint32_t h = token_hash((uint32_t)lane, k);
            int rank = 0;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t hj = (uint32_t)__shfl((int)h, (int)j, WAVE);
                rank += (hj < h || (hj == h && j < (uint32_t)lane)) ? 1 : 0;
            }
            if ((uint32_t)lane < n && rank < N) s_idx[rank] = lane;      // ranks of lanes < n are a permutation of 0 .. n-1
        } else {                                                // N <= n, n > 64: keyed bijection of [0, n)
            int bits = 32 - __builtin_clz(n - 1);              // 2^bits >= n, bits >= 7
            bits += bits & 1;
            const int half = bits >> 1;
            uint32_t y = t;
            if (lane < cnt) {
                do {
                    y = feistel(y, half, k);
                } while (y >= n);                               // terminates: see the header comment
            }
            s_idx[lane] = (int32_t)y;
        }
    }
    __syncthreads();
    if (idx_out != nullptr && tid < cnt) idx_out[(int64_t)r * N + t0 + tid] = s_idx[tid];

    const T* bag_rows = store + base * row_stride;
    if (VEC) {
        constexpr int E = Vec<T>::E;
        const int dv = D / E;                                   // 16-byte accesses of the store per row
        int lpr = 1;                                            // lanes per row: a power of two, <= 64
        while (lpr < dv && lpr < WAVE) lpr <<= 1;
        const int sub = lane / lpr, c0 = lane - sub * lpr;
        const int step = BS_WAVES * (WAVE / lpr);               // rows the workgroup covers per pass
        for (int row0 = wave * (WAVE / lpr) + sub; row0 < cnt; row0 += BS_INFLIGHT * step) {
            const T* src[BS_INFLIGHT];
            float* dst[BS_INFLIGHT];
#pragma unroll
            for (int j = 0; j < BS_INFLIGHT; ++j) {
                const int row = row0 + j * step;
                const int safe = row < cnt ? row : row0;          // a row past the chunk: addresses of a valid one, never used
                src[j] = bag_rows + (int64_t)s_idx[safe] * row_stride;
                dst[j] = orow + (int64_t)safe * D;
            }
            for (int c = c0; c < dv; c += lpr) {
                typename Vec<T>::Raw v[BS_INFLIGHT];
#pragma unroll
                for (int j = 0; j < BS_INFLIGHT; ++j)
                    if (row0 + j * step < cnt) v[j] = Vec<T>::ld(src[j] + c * E);
#pragma unroll
                for (int j = 0; j < BS_INFLIGHT; ++j)
                    if (row0 + j * step < cnt) Vec<T>::st(dst[j] + c * E, v[j]);
            }
        }
    } else {                                                    // any D, any stride: element-wise
        for (int row = wave; row < cnt; row += BS_WAVES) {
            const T* sa = bag_rows + (int64_t)s_idx[row] * row_stride;
            float* da = orow + (int64_t)row * D;
            for (int c = lane; c < D; c += WAVE) da[c] = Vec<T>::up(sa[c]);
        }
    }
}

template <class T>
int launch(const void* store, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags, const int32_t* bag,
           const int64_t* key_id, int64_t R, int N, int D, int chunks, uint64_t seed, uint64_t counter, float* out, int32_t* idx_out,
           hipStream_t stream) {
    const bool vec = D % Vec<T>::E == 0 && row_stride % Vec<T>::E == 0;
    const dim3 grid((unsigned)(R * chunks)), block(BS_THREADS);
    if (vec)
        hipLaunchKernelGGL((bag_sample_kernel<T, true>), grid, block, 0, stream, reinterpret_cast<const T*>(store), row_stride, T_total, off,
                           n_bags, bag, key_id, N, D, chunks, seed, counter, out, idx_out);
    else
        hipLaunchKernelGGL((bag_sample_kernel<T, false>), grid, block, 0, stream, reinterpret_cast<const T*>(store), row_stride, T_total,
                           off, n_bags, bag, key_id, N, D, chunks, seed, counter, out, idx_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int mdl_bag_sample(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                              const int32_t* bag, const int64_t* key_id, int64_t R, int N, int D, uint64_t seed, uint64_t counter,
                              float* out, int32_t* idx_out, void* stream) {
    if (store == nullptr || off == nullptr || bag == nullptr || out == nullptr) return MDL_E_ARG;
    if (R < 0 || N < 1 || D < 1 || T_total < 0 || n_bags < 0 || row_stride < D) return MDL_E_ARG;
    if (dtype != MDL_STORE_F32 && dtype != MDL_STORE_F16 && dtype != MDL_STORE_BF16) return MDL_E_ARG;
    if (!host_aligned16(store) || !host_aligned16(out)) return MDL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(off) & 7u) || (reinterpret_cast<uintptr_t>(bag) & 3u) || (reinterpret_cast<uintptr_t>(key_id) & 7u) ||
        (reinterpret_cast<uintptr_t>(idx_out) & 3u))
        return MDL_E_ALIGN;
    const int chunks = (N + BS_TOK - 1) / BS_TOK;
    if (R > 0x7FFFFFFF / (int64_t)N || R * chunks > 0x7FFFFFFF) return MDL_E_UNSUPPORTED;
    if (R == 0) return MDL_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case MDL_STORE_F32:
            return launch<float>(store, row_stride, T_total, off, n_bags, bag, key_id, R, N, D, chunks, seed, counter, out, idx_out, s);
        case MDL_STORE_F16:
            return launch<_Float16>(store, row_stride, T_total, off, n_bags, bag, key_id, R, N, D, chunks, seed, counter, out, idx_out, s);
        default:
            return launch<bf16_t>(store, row_stride, T_total, off, n_bags, bag, key_id, R, N, D, chunks, seed, counter, out, idx_out, s);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// bag_pack (S2 of the header) -- the variable-length form of the gather above: every bag at its own length L_r = cu[r + 1] - cu[r],
// packed back to back into out [T_out, D], in ONE launch.  A bag that fits (L_r >= n) is taken whole and in stored order; a longer one
// (L_r < n) is cut to L_r rows by exactly the draw of bag_sample_kernel with N := L_r -- the same keys, the same in-wave sort for
// n <= 64, the same Feistel walk above -- so the rows and idx are bit-equal to mdl_bag_sample(N = L_r) under the same (seed, counter,
// key_id).  The with-replacement regime cannot occur: a bag is never asked for more rows than it has.
//
// Work split.  chunk_cu [R + 1] is the prefix sum of ceil(L_r / 64): workgroup w finds its bag r, the last one with chunk_cu[r] <= w,
// by binary search (wave-uniform, ceil(log2 R) reads of a table that stays in L2), owns rows 64 c .. 64 c + 63 of that bag with
// c = w - chunk_cu[r], and then runs bag_sample's scheme: wave 0 leaves the 64 source rows in LDS, the four waves copy them.
//
// Bounds.  The store side is bag_sample's: a bag the tables cannot place inside [0, T_total) is written as an absent stain.  The output
// side: a workgroup writes packed rows cu[r] + 64 c + i only, and only those inside [0, T_out); a (bag, chunk) that the two tables do
// not agree on (cu[r] < 0, cu[r + 1] <= cu[r], c outside the bag) writes nothing.  r comes out of a search over [0, R), so every table
// is read inside its R (+ 1) entries whatever chunk_cu holds.
namespace mdl {
namespace {

// rows [0, ncopy) of the chunk from the store rows s_idx names (the copy loops of bag_sample_kernel), rows [ncopy, cnt) zeros
template <class T, bool VEC>
__device__ __forceinline__ void pack_rows(const T* __restrict__ bag_rows, int64_t row_stride, const int32_t* s_idx, int ncopy, int cnt, int D,
                                          float* __restrict__ orow, int tid, int lane, int wave) {
    if (VEC) {
        constexpr int E = Vec<T>::E;
        const int dv = D / E;                                   // 16-byte accesses of the store per row
        int lpr = 1;                                            // lanes per row: a power of two, <= 64
        while (lpr < dv && lpr < WAVE) lpr <<= 1;
        const int sub = lane / lpr, c0 = lane - sub * lpr;
        const int step = BS_WAVES * (WAVE / lpr);               // rows the workgroup covers per pass
        for (int row0 = wave * (WAVE / lpr) + sub; row0 < ncopy; row0 += BS_INFLIGHT * step) {
            const T* src[BS_INFLIGHT];
            float* dst[BS_INFLIGHT];
#pragma unroll
            for (int j = 0; j < BS_INFLIGHT; ++j) {
                const int row = row0 + j * step;
                const int safe = row < ncopy ? row : row0;        // a row past the chunk: addresses of a valid one, never used
                src[j] = bag_rows + (int64_t)s_idx[safe] * row_stride;
                dst[j] = orow + (int64_t)safe * D;
            }
            for (int c = c0; c < dv; c += lpr) {
                typename Vec<T>::Raw v[BS_INFLIGHT];
#pragma unroll
                for (int j = 0; j < BS_INFLIGHT; ++j)
                    if (row0 + j * step < ncopy) v[j] = Vec<T>::ld(src[j] + c * E);
#pragma unroll
                for (int j = 0; j < BS_INFLIGHT; ++j)
                    if (row0 + j * step < ncopy) Vec<T>::st(dst[j] + c * E, v[j]);
            }
        }
    } else {                                                    // any D, any stride: element-wise
        for (int row = wave; row < ncopy; row += BS_WAVES) {
            const T* sa = bag_rows + (int64_t)s_idx[row] * row_stride;
            float* da = orow + (int64_t)row * D;
            for (int c = lane; c < D; c += WAVE) da[c] = Vec<T>::up(sa[c]);
        }
    }
    float* zrow = orow + (int64_t)ncopy * D;
    const int64_t total = (int64_t)(cnt - ncopy) * D;
    if (VEC) {                                                  // D is a multiple of 4 and out is 16-byte aligned: so is every row
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int64_t e = (int64_t)tid * 4; e < total; e += BS_THREADS * 4) st4(zrow + e, z);
    } else {
        for (int64_t e = tid; e < total; e += BS_THREADS) zrow[e] = 0.f;
    }
}

template <class T, bool VEC>
__global__ __launch_bounds__(BS_THREADS) void bag_pack_kernel(const T* __restrict__ store, int64_t row_stride, int64_t T_total,
                                                              const int64_t* __restrict__ off, int64_t n_bags,
                                                              const int32_t* __restrict__ bag, const int64_t* __restrict__ key_id,
                                                              const int64_t* __restrict__ cu, const int64_t* __restrict__ chunk_cu, int R,
                                                              int64_t T_out, int D, uint64_t seed, uint64_t counter,
                                                              float* __restrict__ out, int32_t* __restrict__ row_bag,
                                                              int32_t* __restrict__ idx_out) {
    __shared__ int32_t s_idx[BS_TOK];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t w = blockIdx.x;
    int lo = 0, hi = R - 1;                                     // the last r of [0, R) with chunk_cu[r] <= w (bags of no rows are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_cu[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const int r = lo;
    const int64_t p0 = cu[r], p1 = cu[r + 1], c = w - chunk_cu[r];
    if (p0 < 0 || p0 >= T_out || p1 <= p0 || c < 0 || c > (T_out >> 6)) return;      // uniform over the workgroup, as all that follows
    const int64_t L = p1 - p0, t0 = c * BS_TOK;                 // no overflow: 0 <= p0 < p1, 0 <= t0 <= T_out < 2^31
    int64_t lim = L - t0;
    if (T_out - p0 - t0 < lim) lim = T_out - p0 - t0;
    if (lim < 1) return;
    const int cnt = lim < BS_TOK ? (int)lim : BS_TOK;           // packed rows of this workgroup, all inside [0, T_out)

    const int g = bag[r];
    int64_t base = 0, n64 = 0;
    if (g >= 0 && g < n_bags) {
        base = off[g];
        n64 = off[g + 1] - base;
        if (base < 0 || n64 < 1 || n64 > 0x7FFFFFFF || base > T_total - n64) n64 = 0;
    }
    const uint32_t n = (uint32_t)n64;                           // 0: an absent stain
    const int64_t prow = p0 + t0;

    int ncopy = 0;                                              // rows of the chunk that come from the store; the others are zeros
    if (n != 0 && L >= n64) {                                   // the bag taken whole: row t is stored row t
        const int64_t left = n64 - t0;
        ncopy = left < 0 ? 0 : left < cnt ? (int)left : cnt;
        if (wave == 0) s_idx[lane] = (int32_t)t0 + lane;
    } else if (n != 0) {                                        // L < n: bag_sample_kernel's draw without replacement, N = L
        ncopy = cnt;
        if (wave == 0) {
            const RowKey k = row_key(seed, counter, key_id != nullptr ? (uint64_t)key_id[r] : (uint64_t)(int64_t)g);
            const int N = (int)L;
            if (n <= (uint32_t)WAVE) {                          // L < n <= 64: one chunk (t0 == 0), random-key sort in the wave
                const uint32_t h = token_hash((uint32_t)lane, k);
                int rank = 0;
                for (uint32_t j = 0; j < n; ++j) {
                    const uint32_t hj = (uint32_t)__shfl((int)h, (int)j, WAVE);
                    rank += (hj < h || (hj == h && j < (uint32_t)lane)) ? 1 : 0;
                }
                if ((uint32_t)lane < n && rank < N) s_idx[rank] = lane;
            } else {                                            // keyed bijection of [0, n), cycle walking
                int bits = 32 - __builtin_clz(n - 1);
                bits += bits & 1;
                const int half = bits >> 1;
                uint32_t y = (uint32_t)t0 + (uint32_t)lane;
                if (lane < cnt) {
                    do {
                        y = feistel(y, half, k);
                    } while (y >= n);                           // terminates: see the comment at the head of the file
                }
                s_idx[lane] = (int32_t)y;
            }
        }
    }
    __syncthreads();
    if (tid < cnt) {
        if (idx_out != nullptr) idx_out[prow + tid] = tid < ncopy ? s_idx[tid] : -1;
        if (row_bag != nullptr) row_bag[prow + tid] = r;
    }
    pack_rows<T, VEC>(store + base * row_stride, row_stride, s_idx, ncopy, cnt, D, out + prow * D, tid, lane, wave);
}

template <class T>
int launch_pack(const void* store, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags, const int32_t* bag,
                const int64_t* key_id, const int64_t* cu, const int64_t* chunk_cu, int R, int64_t n_chunks, int64_t T_out, int D,
                uint64_t seed, uint64_t counter, float* out, int32_t* row_bag, int32_t* idx_out, hipStream_t stream) {
    const bool vec = D % Vec<T>::E == 0 && row_stride % Vec<T>::E == 0;
    const dim3 grid((unsigned)n_chunks), block(BS_THREADS);
    if (vec)
        hipLaunchKernelGGL((bag_pack_kernel<T, true>), grid, block, 0, stream, reinterpret_cast<const T*>(store), row_stride, T_total, off,
                           n_bags, bag, key_id, cu, chunk_cu, R, T_out, D, seed, counter, out, row_bag, idx_out);
    else
        hipLaunchKernelGGL((bag_pack_kernel<T, false>), grid, block, 0, stream, reinterpret_cast<const T*>(store), row_stride, T_total, off,
                           n_bags, bag, key_id, cu, chunk_cu, R, T_out, D, seed, counter, out, row_bag, idx_out);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_bag_pack(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                            const int32_t* bag, const int64_t* key_id, const int64_t* cu, const int64_t* chunk_cu, int64_t R,
                            int64_t n_chunks, int64_t T_out, int D, uint64_t seed, uint64_t counter, float* out, int32_t* row_bag,
                            int32_t* idx_out, void* stream) {
    if (store == nullptr || off == nullptr || bag == nullptr || cu == nullptr || chunk_cu == nullptr || out == nullptr) return MDL_E_ARG;
    if (R < 0 || n_chunks < 0 || T_out < 0 || D < 1 || T_total < 0 || n_bags < 0 || row_stride < D) return MDL_E_ARG;
    if (dtype != MDL_STORE_F32 && dtype != MDL_STORE_F16 && dtype != MDL_STORE_BF16) return MDL_E_ARG;
    if (!host_aligned16(store) || !host_aligned16(out)) return MDL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(off) & 7u) || (reinterpret_cast<uintptr_t>(bag) & 3u) || (reinterpret_cast<uintptr_t>(key_id) & 7u) ||
        (reinterpret_cast<uintptr_t>(cu) & 7u) || (reinterpret_cast<uintptr_t>(chunk_cu) & 7u) ||
        (reinterpret_cast<uintptr_t>(row_bag) & 3u) || (reinterpret_cast<uintptr_t>(idx_out) & 3u))
        return MDL_E_ALIGN;
    if (R > 0x7FFFFFFF || T_out > 0x7FFFFFFF || n_chunks > 0x7FFFFFFF) return MDL_E_UNSUPPORTED;
    if (R == 0 || T_out == 0 || n_chunks == 0) return MDL_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case MDL_STORE_F32:
            return launch_pack<float>(store, row_stride, T_total, off, n_bags, bag, key_id, cu, chunk_cu, (int)R, n_chunks, T_out, D, seed,
                                      counter, out, row_bag, idx_out, s);
        case MDL_STORE_F16:
            return launch_pack<_Float16>(store, row_stride, T_total, off, n_bags, bag, key_id, cu, chunk_cu, (int)R, n_chunks, T_out, D, seed,
                                         counter, out, row_bag, idx_out, s);
        default:
            return launch_pack<bf16_t>(store, row_stride, T_total, off, n_bags, bag, key_id, cu, chunk_cu, (int)R, n_chunks, T_out, D, seed,
                                       counter, out, row_bag, idx_out, s);
    }
}
