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
//
// One kernel, one launcher.  A call is described by three records: the Store (both tiers and the bag table), the Draw (which bag under
// which keys) and one job, SampleJob (S1, S3) or PackJob (S2, S4).  gather_item, overloaded on the job, is the whole work of one
// (output row, 64-token chunk) item; the draw (row_key, token_hash, feistel, draw_distinct), the placement of a bag (locate_bag) and
// the copy loops (copy_rows, zero_rows) are device functions under it.  bag_gather_kernel<T, VEC, PASS, Job> is the only __global__
// function of the gathers and launch() the only place that launches it, so the four entry points draw and copy with the same code; they
// differ in the records they fill and in the passes they ask for (PASS_ALL, or PASS_DEV then PASS_HOST: the tiered forms, further down).
// The per-bag column means (S5, further down) are a third job of the same kernel and launcher, followed by a combine kernel.
#include "common.hpp"
#include <type_traits>

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

// Which items a kernel owns.  PASS_ALL: every item, the store is one device tensor (S1, S2).  The tiered entry points split a launch
// in two: PASS_DEV owns the items of resident bags and of absent stains, PASS_HOST those of the bags in the host tier.
enum { PASS_ALL = 0, PASS_DEV = 1, PASS_HOST = 2 };

// The store: rows [0, T_dev) at `dev`, rows [T_dev, T_total) at `host` (their device-visible address), D elements of the call's
// dtype per row, row_stride elements from one row to the next in both tiers; bag g is rows off[g] .. off[g + 1] - 1.  The resident
// store (S1, S2) is the case host == NULL, T_dev == T_total.  The bases are untyped so that the argument checks, which know no
// element type, read the same record as the kernels.
struct Store {
    const void* dev;
    const void* host;
    int64_t T_dev, row_stride, T_total;
    const int64_t* off;                     // [n_bags + 1]
    int64_t n_bags;
    int D;
};

// The draw: output row (bag) r takes stored bag bag[r] under the keys of (seed, counter, key_id[r]); key_id NULL: key_id[r] = bag[r].
struct Draw {
    const int32_t* bag;
    const int64_t* key_id;
    uint64_t seed, counter;
};

// The dense gather (S1, S3): item w is tokens 64 c .. 64 c + 63 of output row r, w = r * chunks + c; out [R, N, D], idx_out [R, N] or NULL.
struct SampleJob {
    int N, chunks;
    int64_t items;                          // R * chunks <= 2^31 - 1: the grid of every pass but the host pass, which walks them
    float* out;
    int32_t* idx_out;
};

// The pack (S2, S4): item w is one 64-row chunk of the output bag that chunk_cu places it in; out [T_out, D], row_bag and idx_out
// [T_out] or NULL.
struct PackJob {
    const int64_t* cu;                      // [R + 1]
    const int64_t* chunk_cu;                // [R + 1]
    int R;
    int64_t T_out;
    int64_t items;                          // n_chunks <= 2^31 - 1
    float* out;
    int32_t* row_bag;
    int32_t* idx_out;
};

// One entry of a table of the call (off, bag, key_id, cu, chunk_cu).  No kernel of this file writes a table, but they arrive inside
// records, where __restrict__ cannot say so.  The constant address space says it: these wave-uniform reads then stay scalar loads in
// the host pass's loop as well, past the barrier and the stores of the items before (without it they become one vector load per lane).
template <class V>
__device__ __forceinline__ V table(const V* p, int64_t i) {
    return ((const __attribute__((address_space(4))) V*)p)[i];
}

// Where the tables place stored bag g: returns n, its length, with `base` its first row of [0, T_total), or 0 (and base 0) for an
// absent stain, by the table or by the bounds rule of the header comment.  A bag with n != 0 lies inside [0, T_total).
__device__ __forceinline__ int64_t bag_extent(const Store& st, int g, int64_t& base) {
    int64_t n64 = 0;
    base = 0;
    if (g >= 0 && g < st.n_bags) {
        base = table(st.off, g);
        n64 = table(st.off, g + 1) - base;
        if (base < 0 || n64 < 1 || n64 > 0x7FFFFFFF || base > st.T_total - n64) n64 = base = 0;
    }
    return n64;
}

// The rows of stored bag g: returns n, its length, or 0 for an absent stain (by the table or by the bounds rule of the header comment);
// `rows` is its first row (the tier's base when n == 0: never read).  Tiered (PASS != PASS_ALL): a bag on both sides of T_dev is an
// absent stain; on_host says which pass owns the item.
template <class T, int PASS>
__device__ __forceinline__ uint32_t locate_bag(const Store& st, int g, const T*& rows, bool& on_host) {
    int64_t base;
    int64_t n64 = bag_extent(st, g, base);
    on_host = false;
    if (PASS != PASS_ALL && n64 != 0) {
        if (base >= st.T_dev) {                                 // wholly in the host tier: T_dev <= base, base + n <= T_total
            on_host = true;
            rows = static_cast<const T*>(st.host) + (base - st.T_dev) * st.row_stride;
            return (uint32_t)n64;
        }
        if (base > st.T_dev - n64) n64 = base = 0;              // on both sides of T_dev: no address is formed from it
    }
    rows = static_cast<const T*>(st.dev) + base * st.row_stride;
    return (uint32_t)n64;
}

// Wave 0, N <= n: the bag rows of tokens t0 .. t0 + 63 of a draw of N distinct rows out of n -> s_idx (see the header comment).
__device__ __forceinline__ void draw_distinct(RowKey k, uint32_t n, int N, uint32_t t0, int lane, int cnt, int32_t* s_idx) {
    if (n <= (uint32_t)WAVE) {                                  // N <= n <= 64: one chunk (t0 == 0), random-key sort in the wave
        const uint32_t h = token_hash((uint32_t)lane, k);
        int rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t hj = (uint32_t)__shfl((int)h, (int)j, WAVE);
            rank += (hj < h || (hj == h && j < (uint32_t)lane)) ? 1 : 0;
        }
        if ((uint32_t)lane < n && rank < N) s_idx[rank] = lane;          // ranks of lanes < n are a permutation of 0 .. n-1
    } else {                                                    // N <= n, n > 64: keyed bijection of [0, n)
        int bits = 32 - __builtin_clz(n - 1);                  // 2^bits >= n, bits >= 7
        bits += bits & 1;
        const int half = bits >> 1;
        uint32_t y = t0 + (uint32_t)lane;
        if (lane < cnt) {
            do {
                y = feistel(y, half, k);
            } while (y >= n);                                   // terminates: see the header comment
        }
        s_idx[lane] = (int32_t)y;
    }
}

// The four waves copy rows [0, ncopy) of a chunk from the bag rows s_idx names to orow, INFLIGHT rows in flight per lane.
// VEC: D and row_stride are multiples of Vec<T>::E and both bases are 16-byte aligned, so every row of both sides is.
template <class T, bool VEC, int INFLIGHT>
__device__ __forceinline__ void copy_rows(const T* __restrict__ bag_rows, int64_t row_stride, const int32_t* s_idx, int ncopy, int D,
                                          float* __restrict__ orow, int lane, int wave) {
    if (VEC) {
        constexpr int E = Vec<T>::E;
        const int dv = D / E;                                   // 16-byte accesses of the store per row
        int lpr = 1;                                            // lanes per row: a power of two, <= 64
        while (lpr < dv && lpr < WAVE) lpr <<= 1;
        const int sub = lane / lpr, c0 = lane - sub * lpr;
        const int step = BS_WAVES * (WAVE / lpr);               // rows the workgroup covers per pass
        for (int row0 = wave * (WAVE / lpr) + sub; row0 < ncopy; row0 += INFLIGHT * step) {
            const T* src[INFLIGHT];
            float* dst[INFLIGHT];
#pragma unroll
            for (int j = 0; j < INFLIGHT; ++j) {
                const int row = row0 + j * step;
                const int safe = row < ncopy ? row : row0;        // a row past the chunk: addresses of a valid one, never used
                src[j] = bag_rows + (int64_t)s_idx[safe] * row_stride;
                dst[j] = orow + (int64_t)safe * D;
            }
            for (int c = c0; c < dv; c += lpr) {
                typename Vec<T>::Raw v[INFLIGHT];
#pragma unroll
                for (int j = 0; j < INFLIGHT; ++j)
                    if (row0 + j * step < ncopy) v[j] = Vec<T>::ld(src[j] + c * E);
#pragma unroll
                for (int j = 0; j < INFLIGHT; ++j)
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
}

// `count` rows of zeros from zrow on (VEC: D is a multiple of 4 and out is 16-byte aligned, so every row is)
template <bool VEC>
__device__ __forceinline__ void zero_rows(float* __restrict__ zrow, int count, int D, int tid) {
    const int64_t total = (int64_t)count * D;
    if (VEC) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int64_t e = (int64_t)tid * 4; e < total; e += BS_THREADS * 4) st4(zrow + e, z);
    } else {
        for (int64_t e = tid; e < total; e += BS_THREADS) zrow[e] = 0.f;
    }
}

// Item w = (output row r, chunk c) of the dense gather: the whole of S1's work for tokens 64 c .. 64 c + 63 of row r.  Uniform over the
// workgroup, the early returns included; a caller that loops over items puts a barrier between two of them (s_idx is reused).
template <class T, bool VEC, int PASS, int INFLIGHT>
__device__ __forceinline__ void gather_item(const Store& st, const Draw& dr, const SampleJob& job, int64_t item, int32_t* s_idx) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int w = (int)item, N = job.N, D = st.D;               // items <= 2^31 - 1
    const int r = w / job.chunks, t0 = (w - r * job.chunks) * BS_TOK;
    const int cnt = N - t0 < BS_TOK ? N - t0 : BS_TOK;        // tokens of this item, >= 1

    const int g = table(dr.bag, r);
    const T* bag_rows;
    bool on_host;
    const uint32_t n = locate_bag<T, PASS>(st, g, bag_rows, on_host);    // 0: absent
    if (PASS != PASS_ALL && on_host != (PASS == PASS_HOST)) return;      // the other pass's item
    float* orow = job.out + ((int64_t)r * N + t0) * D;
    int32_t* idx_out = job.idx_out;

    if (n == 0) {                                               // uniform over the workgroup
        zero_rows<VEC>(orow, cnt, D, tid);
        if (idx_out != nullptr && tid < cnt) idx_out[(int64_t)r * N + t0 + tid] = -1;
        return;
    }

    if (wave == 0) {
        const RowKey k = row_key(dr.seed, dr.counter, dr.key_id != nullptr ? (uint64_t)table(dr.key_id, r) : (uint64_t)(int64_t)g);
        if (n < (uint32_t)N)                                    // with replacement
            s_idx[lane] = (int32_t)(((uint64_t)token_hash((uint32_t)(t0 + lane), k) * n) >> 32);
        else
            draw_distinct(k, n, N, (uint32_t)t0, lane, cnt, s_idx);
    }
    __syncthreads();
    if (idx_out != nullptr && tid < cnt) idx_out[(int64_t)r * N + t0 + tid] = s_idx[tid];
    copy_rows<T, VEC, INFLIGHT>(bag_rows, st.row_stride, s_idx, cnt, D, orow, lane, wave);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// bag_pack (S2 of the header) -- the variable-length form of the gather above: every bag at its own length L_r = cu[r + 1] - cu[r],
// packed back to back into out [T_out, D], in ONE launch.  A bag that fits (L_r >= n) is taken whole and in stored order; a longer one
// (L_r < n) is cut to L_r rows by exactly the draw of the dense gather with N := L_r -- the same keys, the same in-wave sort for
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

// Item w = (output bag r, chunk c) of the pack: the whole of S2's work for packed rows cu[r] + 64 c .. + 63.  Uniform over the workgroup,
// the early returns included; a caller that loops over items puts a barrier between two of them (s_idx is reused).
template <class T, bool VEC, int PASS, int INFLIGHT>
__device__ __forceinline__ void gather_item(const Store& st, const Draw& dr, const PackJob& job, int64_t w, int32_t* s_idx) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int D = st.D;
    const int64_t T_out = job.T_out;
    int lo = 0, hi = job.R - 1;                                 // the last r of [0, R) with chunk_cu[r] <= w (bags of no rows are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table(job.chunk_cu, mid) <= w) lo = mid; else hi = mid - 1;
    }
    const int r = lo;
    const int64_t p0 = table(job.cu, r), p1 = table(job.cu, r + 1), c = w - table(job.chunk_cu, r);
    if (p0 < 0 || p0 >= T_out || p1 <= p0 || c < 0 || c > (T_out >> 6)) return;      // uniform over the workgroup, as all that follows
    const int64_t L = p1 - p0, t0 = c * BS_TOK;                 // no overflow: 0 <= p0 < p1, 0 <= t0 <= T_out < 2^31
    int64_t lim = L - t0;
    if (T_out - p0 - t0 < lim) lim = T_out - p0 - t0;
    if (lim < 1) return;
    const int cnt = lim < BS_TOK ? (int)lim : BS_TOK;           // packed rows of this item, all inside [0, T_out)

    const int g = table(dr.bag, r);
    const T* bag_rows;
    bool on_host;
    const uint32_t n = locate_bag<T, PASS>(st, g, bag_rows, on_host);    // 0: absent
    if (PASS != PASS_ALL && on_host != (PASS == PASS_HOST)) return;      // the other pass's item
    const int64_t n64 = n, prow = p0 + t0;

    int ncopy = 0;                                              // rows of the chunk that come from the store; the others are zeros
    if (n != 0 && L >= n64) {                                   // the bag taken whole: row t is stored row t
        const int64_t left = n64 - t0;
        ncopy = left < 0 ? 0 : left < cnt ? (int)left : cnt;
        if (wave == 0) s_idx[lane] = (int32_t)t0 + lane;
    } else if (n != 0) {                                        // L < n: the dense gather's draw without replacement, N = L
        ncopy = cnt;
        if (wave == 0)
            draw_distinct(row_key(dr.seed, dr.counter, dr.key_id != nullptr ? (uint64_t)table(dr.key_id, r) : (uint64_t)(int64_t)g), n, (int)L,
                          (uint32_t)t0, lane, cnt, s_idx);
    }
    __syncthreads();
    if (tid < cnt) {
        if (job.idx_out != nullptr) job.idx_out[prow + tid] = tid < ncopy ? s_idx[tid] : -1;
        if (job.row_bag != nullptr) job.row_bag[prow + tid] = r;
    }
    float* orow = job.out + prow * D;
    copy_rows<T, VEC, INFLIGHT>(bag_rows, st.row_stride, s_idx, ncopy, D, orow, lane, wave);
    zero_rows<VEC>(orow + (int64_t)ncopy * D, cnt - ncopy, D, tid);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The tiered forms (S3, S4 of the header): rows [0, T_dev) of the store in device memory, rows [T_dev, T_total) in pinned host memory
// that the kernel reads over PCIe.  The items are those of S1 / S2 and so is every bit written (gather_item); what changes is who runs
// an item.  Two launches of the one kernel below on the stream, each skipping the other's items:
//   device pass  PASS_DEV: one workgroup per item, the chip-wide grid of S1 / S2: the items of resident bags and of absent stains (a
//                bag on both sides of T_dev is one).  An item of the host tier returns after three table reads.
//   host pass    PASS_HOST: a NARROW PERSISTENT grid: host_wgs workgroups walk all items with a grid stride, skip those that are not
//                the host tier's and run the same draw-then-copy on the others.  A 63 GB/s link is saturated by a few hundred KB in
//                flight (host_wgs x 256 lanes x BS_HOST_INFLIGHT x 16 B); a chip-wide grid would hold wave slots and registers of
//                every CU for the milliseconds the link needs, in front of the step's kernels that run beside a prefetching gather.
// Two launches rather than one kernel that branches per item: one grid cannot be both chip-wide and narrow.
#ifndef BS_HOST_INFLIGHT
#define BS_HOST_INFLIGHT 4                  // rows a lane has in flight over PCIe
#endif
#ifndef BS_HOST_WGS
#define BS_HOST_WGS 64                      // the host pass's grid when the caller passes host_wgs = 0
#endif

// ------------------------------------------------------------------------------------------------------------------------------------
// bag_mean (S5 of the header) -- the column means of whole stored bags, the mean-embedding baseline of a cohort: a reduction over the
// same store, through the same records, passes and launcher, followed by one small combine launch.  No atomics.
//
// Work split.  chunk_cu [R + 1] is the prefix sum of ceil(n_r / BM_ROWS): item w is chunk c = w - chunk_cu[r] of output row r (found
// by the pack's binary search), rows c * BM_ROWS .. of stored bag bag[r] -- a CONTIGUOUS range of the store.  Inside the workgroup a
// thread owns one slot of BM_COLS adjacent columns (one 16-byte load of a 16-bit store, two of an fp32 store; element-wise loads where
// D or the stride forbid them) in one row group: lpr = min(256, next_pow2(ceil(D / BM_COLS))) adjacent lanes cover a row and the G =
// 256 / lpr row groups take the chunk's rows t = grp, grp + G, grp + 2 G, ...  Each thread adds its rows in that order in fp32
// (BM_INFLIGHT loads in flight, the additions in row order), the groups' sums are merged through LDS in the order 0, 1, .. G - 1, and
// the fp32 partial [D] of the item goes to ws[w].  D > 256 * BM_COLS: the slots are walked in passes of 256.
// bag_mean_combine_kernel then adds a bag's partials in chunk order, divides by n and writes out[r]; a bag the tables do not place
// (absent, invalid, or chunk_cu disagreeing with off about its chunks) is a row of zeros.
//
// The order of the additions of a column is a function of (n, D, BM_ROWS) alone: lpr and G depend on D only -- not on the element
// type, on the copy path (VEC or not: the stride), on the pass that served the chunk, on its grid or on the other bags.
//
// Tiers.  The split is per ROW: row a of [0, T_total) is read from the device tier when a < T_dev and from the host tier otherwise, so a
// bag on both sides of T_dev is served like any other.  A chunk with a row at or beyond T_dev is the host pass's item, every other
// chunk the device pass's.
//
// Bounds.  r comes out of a search over [0, R); the bag's rows are bag_extent's, inside [0, T_total); a chunk index outside the bag
// writes nothing; ws is written at item w < n_chunks only and read at chunk_cu[r] .. chunk_cu[r + 1] - 1 only when that range lies in
// [0, n_chunks) and has the length off gives; out is written at rows r < R.
constexpr int BM_ROWS = MDL_BAG_MEAN_ROWS;
constexpr int BM_COLS = MDL_BAG_MEAN_COLS;
constexpr int BM_INFLIGHT = 8;              // rows a lane has in flight, both passes (16 for the 16-bit stores measured the same)
static_assert(BS_THREADS == MDL_BAG_MEAN_THREADS && BM_COLS == 8, "the header's h(len) and the slot loads are written for these");

struct MeanJob {
    const int64_t* chunk_cu;                // [R + 1]
    int R;
    int64_t items;                          // n_chunks <= 2^31 - 1
    float* ws;                              // [n_chunks, D]: one partial per item
    float* out;                             // [R, D]
};

// lanes that cover one row: a power of two, a function of D alone
__device__ __forceinline__ int mean_lanes_per_row(int D) {
    const int ns = (D + BM_COLS - 1) / BM_COLS;
    int lpr = 1;
    while (lpr < ns && lpr < BS_THREADS) lpr <<= 1;
    return lpr;
}

// columns col .. col + 7 of a store row, widened exactly; columns at or beyond D read as 0 (col < D)
template <class T, bool VEC>
__device__ __forceinline__ f32x8 load_slot(const T* __restrict__ row, int col, int D) {
    f32x8 v;
    if constexpr (VEC && Vec<T>::E == BM_COLS) {                // D % 8 == 0: the slot is whole
        v = __builtin_convertvector(Vec<T>::ld(row + col), f32x8);
    } else if constexpr (VEC) {                                 // fp32, D % 4 == 0
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        v.lo = Vec<T>::ld(row + col);
        v.hi = col + 4 < D ? Vec<T>::ld(row + col + 4) : z;
    } else {
#pragma unroll
        for (int j = 0; j < BM_COLS; ++j) v[j] = col + j < D ? Vec<T>::up(row[col + j]) : 0.f;
    }
    return v;
}

// Item w = (output row r, chunk c) of the mean: the partial column sums of rows c * BM_ROWS .. of bag bag[r] -> ws[w].  Uniform over the
// workgroup, the early returns included; a caller that loops over items puts a barrier between two of them (s_part is reused).
template <class T, bool VEC, int PASS, int INFLIGHT>
__device__ __forceinline__ void gather_item(const Store& st, const Draw& dr, const MeanJob& job, int64_t w, int32_t*) {
    __shared__ float s_part[BS_THREADS * BM_COLS];
    const int tid = threadIdx.x, D = st.D;
    int lo = 0, hi = job.R - 1;                                 // the last r of [0, R) with chunk_cu[r] <= w (bags of no chunks are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table(job.chunk_cu, mid) <= w) lo = mid; else hi = mid - 1;
    }
    const int r = lo;
    const int64_t c = w - table(job.chunk_cu, r);
    int64_t base;
    const int64_t n = bag_extent(st, table(dr.bag, r), base);  // 0: absent
    if (c < 0 || c >= (n + BM_ROWS - 1) / BM_ROWS) return;      // not a chunk of this bag (n == 0 included): nothing is read or written
    const int64_t t_first = c * BM_ROWS, first = base + t_first;     // no overflow: c * BM_ROWS < n + BM_ROWS <= 2^31 + BM_ROWS
    const int rows = n - t_first < BM_ROWS ? (int)(n - t_first) : BM_ROWS;         // >= 1, all inside the bag
    if (PASS != PASS_ALL && (first + rows > st.T_dev) != (PASS == PASS_HOST)) return;     // the other pass's item

    const int lpr = mean_lanes_per_row(D), G = BS_THREADS / lpr, grp = tid / lpr, s0 = tid - grp * lpr;
    const int ns = (D + BM_COLS - 1) / BM_COLS;
    const T* dev = static_cast<const T*>(st.dev);
    const T* host = static_cast<const T*>(st.host);
    const int64_t stride = st.row_stride, T_dev = st.T_dev;
    float* part = job.ws + w * D;
    for (int sb = 0; sb < ns; sb += lpr) {                      // one pass unless D > 256 * BM_COLS
        const int s = sb + s0, col = s * BM_COLS;
        f32x8 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (s < ns) {
            for (int t0 = grp; t0 < rows; t0 += BM_INFLIGHT * G) {
                f32x8 v[BM_INFLIGHT];
#pragma unroll
                for (int j = 0; j < BM_INFLIGHT; ++j) {
                    const int t = t0 + j * G;
                    if (t < rows) {
                        const int64_t a = first + t;            // the row of [0, T_total)
                        const T* row = (PASS == PASS_HOST && a >= T_dev) ? host + (a - T_dev) * stride : dev + a * stride;
                        v[j] = load_slot<T, VEC>(row, col, D);
                    }
                }
#pragma unroll
                for (int j = 0; j < BM_INFLIGHT; ++j)
                    if (t0 + j * G < rows) acc += v[j];           // in row order
            }
        }
        st4(s_part + tid * BM_COLS, acc.lo);
        st4(s_part + tid * BM_COLS + 4, acc.hi);
        __syncthreads();
        for (int e = tid; e < lpr * BM_COLS; e += BS_THREADS) {  // column sb * 8 + e of the pass: its G group sums, in group order
            if (sb * BM_COLS + e < D) {
                float sum = s_part[e];
                for (int gg = 1; gg < G; ++gg) sum += s_part[gg * lpr * BM_COLS + e];
                part[sb * BM_COLS + e] = sum;
            }
        }
        __syncthreads();                                        // the next pass overwrites s_part
    }
}

// out[r] = (the partials of bag bag[r], added in chunk order) / n; zeros for a bag the tables do not place.  One workgroup per row.
__global__ __launch_bounds__(BS_THREADS) void bag_mean_combine_kernel(Store st, Draw dr, MeanJob job) {
    const int r = blockIdx.x, D = st.D;
    int64_t base;
    const int64_t n = bag_extent(st, table(dr.bag, r), base);
    const int64_t nc = (n + BM_ROWS - 1) / BM_ROWS, p0 = table(job.chunk_cu, r), p1 = table(job.chunk_cu, r + 1);
    const bool placed = n > 0 && p0 >= 0 && p1 >= p0 && p1 <= job.items && p1 - p0 == nc;
    const float* __restrict__ part = job.ws + (placed ? p0 : 0) * D;
    float* __restrict__ o = job.out + (int64_t)r * D;
    const float len = (float)n;
    for (int col = threadIdx.x; col < D; col += BS_THREADS) {
        float sum = 0.f;
        if (placed) {
            sum = part[col];
            for (int64_t k = 1; k < nc; ++k) sum += part[k * D + col];
            sum /= len;
        }
        o[col] = sum;
    }
}

// The kernel of every pass of this file: Job (SampleJob, PackJob or MeanJob) selects gather_item and names the work in a kernel trace
// (for a MeanJob the item is a reduction, and bag_mean_combine_kernel above follows the passes).  PASS_ALL and
// PASS_DEV: the grid is job.items, workgroup w runs item w.  PASS_HOST: any grid, the workgroups share the items out by grid stride.
template <class T, bool VEC, int PASS, class Job>
__global__ __launch_bounds__(BS_THREADS) void bag_gather_kernel(Store st, Draw dr, Job job) {
    __shared__ int32_t s_idx[BS_TOK];
    if (PASS != PASS_HOST) {
        gather_item<T, VEC, PASS, BS_INFLIGHT>(st, dr, job, (int64_t)blockIdx.x, s_idx);
    } else {
        for (int64_t w = blockIdx.x; w < job.items; w += gridDim.x) {
            gather_item<T, VEC, PASS, BS_HOST_INFLIGHT>(st, dr, job, w, s_idx);
            __syncthreads();                                    // the next item's draw overwrites s_idx
        }
    }
}

// What the runtime knows about the host tier [p, p + bytes): MDL_OK and its device-visible address when both ends lie in registered
// (pinned) host memory or both in device memory, and -- where the runtime reports the allocation's extent -- inside one allocation.
// Anything else (pageable, managed, unknown to the runtime) is MDL_E_ARG: no kernel is launched on it.
int device_view_of_tier(const void* p, int64_t bytes, const void** dev) {
    const char* first = static_cast<const char*>(p);
    const char* ends[2] = {first, first + (bytes - 1)};
    hipMemoryType type[2];
    for (int i = 0; i < 2; ++i) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, ends[i]) != hipSuccess) {
            (void)hipGetLastError();                            // pageable memory on runtimes that answer with an error
            return MDL_E_ARG;
        }
        type[i] = attr.type;
        if (attr.isManaged) return MDL_E_ARG;
    }
    if (type[0] != type[1] || (type[0] != hipMemoryTypeHost && type[0] != hipMemoryTypeDevice)) return MDL_E_ARG;
    void* d = const_cast<void*>(p);
    if (type[0] == hipMemoryTypeHost && hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) {
        (void)hipGetLastError();
        return MDL_E_ARG;
    }
    if (d == nullptr) return MDL_E_ARG;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d) == hipSuccess) {
        // hipHostMalloc and hipMalloc report base and size; for hipHostRegister-ed memory the runtime reports the registration's size
        // and a NULL base: the tier must then fit the size, and its place inside the registration rests on the two ends above
        const uintptr_t b = reinterpret_cast<uintptr_t>(base), a = reinterpret_cast<uintptr_t>(d);
        if ((uint64_t)bytes > size) return MDL_E_ARG;
        if (base != nullptr && (a < b || a - b > size - (uint64_t)bytes)) return MDL_E_ARG;
    } else {
        (void)hipGetLastError();                                // no extent reported for this kind of memory: the two ends stand
    }
    *dev = d;
    return MDL_OK;
}

// arguments common to S3 and S4: MDL_OK with *host_dev resolved (NULL without a host tier) and *wgs the host pass's grid (0: no pass)
int check_tiers(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev, int D, int host_wgs,
                int64_t items, const void** host_dev, int* wgs) {
    if (T_total < 0 || T_dev < 0 || T_dev > T_total || host_wgs < 0 || D < 1 || row_stride < D) return MDL_E_ARG;
    if (dtype != MDL_STORE_F32 && dtype != MDL_STORE_F16 && dtype != MDL_STORE_BF16) return MDL_E_ARG;
    if ((T_dev > 0 && store == nullptr) || (T_dev < T_total && store_host == nullptr)) return MDL_E_ARG;
    if (!host_aligned16(store) || !host_aligned16(store_host)) return MDL_E_ALIGN;
    *host_dev = nullptr;
    *wgs = 0;
    if (T_dev == T_total || items == 0) return MDL_OK;
    const int64_t esz = dtype == MDL_STORE_F32 ? 4 : 2, rows = T_total - T_dev;
    if (rows > INT64_MAX / esz / row_stride) return MDL_E_ARG;
    const int rc = device_view_of_tier(store_host, ((rows - 1) * row_stride + D) * esz, host_dev);
    if (rc != MDL_OK) return rc;
    if (!host_aligned16(*host_dev)) return MDL_E_ALIGN;
    const int64_t want = host_wgs > 0 ? host_wgs : BS_HOST_WGS;
    *wgs = (int)(want < items ? want : items);
    return MDL_OK;
}

// The sizes and the output side of a call as its entry point received them, before anything is narrowed to int.  A dense gather
// (S1, S3) states N and brings no table; a pack (S2, S4) states n_chunks and T_out and brings cu, chunk_cu and row_bag.  A mean (S5)
// is checked as a pack of no rows whose one table, chunk_cu, stands for both, and brings a workspace.
struct Call {
    bool pack;
    int64_t R;
    int N;
    int64_t n_chunks, T_out;
    const int64_t *cu, *chunk_cu;
    float* out;
    int32_t *row_bag, *idx_out;
    const void* ws;                         // S5's partials, NULL for the gathers
};

inline bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

// The refusals all entry points share, in one order for all of them: NULL / range / dtype (MDL_E_ARG), then alignment
// (MDL_E_ALIGN), then the int32 launch geometry (MDL_E_UNSUPPORTED).  An optional pointer that is NULL is aligned.  Which of the store's
// two bases may be NULL differs between the resident and the tiered forms and is the entry point's to say, before this.
int check_call(const Store& st, const Draw& dr, const Call& c, int dtype) {
    if (st.off == nullptr || dr.bag == nullptr || c.out == nullptr) return MDL_E_ARG;
    if (c.pack ? (c.cu == nullptr || c.chunk_cu == nullptr || c.n_chunks < 0 || c.T_out < 0) : c.N < 1) return MDL_E_ARG;
    if (c.R < 0 || st.D < 1 || st.T_total < 0 || st.n_bags < 0 || st.row_stride < st.D) return MDL_E_ARG;
    if (dtype != MDL_STORE_F32 && dtype != MDL_STORE_F16 && dtype != MDL_STORE_BF16) return MDL_E_ARG;
    if (!host_aligned16(st.dev) || !host_aligned16(st.host) || !host_aligned16(c.out) || !host_aligned16(c.ws)) return MDL_E_ALIGN;
    if (misaligned(st.off, 8) || misaligned(dr.key_id, 8) || misaligned(c.cu, 8) || misaligned(c.chunk_cu, 8)) return MDL_E_ALIGN;
    if (misaligned(dr.bag, 4) || misaligned(c.row_bag, 4) || misaligned(c.idx_out, 4)) return MDL_E_ALIGN;
    // the output rows are indexed in int32, and with them the items: a dense gather has R * ceil(N / 64) <= R * N of them
    if (c.pack ? (c.R > 0x7FFFFFFF || c.T_out > 0x7FFFFFFF || c.n_chunks > 0x7FFFFFFF) : c.R > 0x7FFFFFFF / (int64_t)c.N)
        return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

// How a call's items are shared out: one PASS_ALL launch (the resident store), or a PASS_DEV launch followed, when host_wgs > 0, by a
// PASS_HOST launch of host_wgs workgroups.
struct Passes {
    bool tiered;
    int host_wgs;
};

// The one launcher: the dtype dispatch, the choice of the copy path and every launch of this file.
template <class Job>
int launch(const Store& st, const Draw& dr, const Job& job, Passes passes, int dtype, hipStream_t stream) {
    const auto run = [&](auto elem, auto vec16) -> int {        // the launches of one element type and one copy path
        using T = decltype(elem);
        constexpr bool VEC = decltype(vec16)::value;
        const dim3 grid((unsigned)job.items), narrow((unsigned)passes.host_wgs), block(BS_THREADS);
        if (!passes.tiered) {
            hipLaunchKernelGGL((bag_gather_kernel<T, VEC, PASS_ALL, Job>), grid, block, 0, stream, st, dr, job);
            MDL_LAUNCH_CHECK();
            return MDL_OK;
        }
        hipLaunchKernelGGL((bag_gather_kernel<T, VEC, PASS_DEV, Job>), grid, block, 0, stream, st, dr, job);
        MDL_LAUNCH_CHECK();
        if (passes.host_wgs == 0) return MDL_OK;                // no host tier
        hipLaunchKernelGGL((bag_gather_kernel<T, VEC, PASS_HOST, Job>), narrow, block, 0, stream, st, dr, job);
        MDL_LAUNCH_CHECK();
        return MDL_OK;
    };
    const auto typed = [&](auto elem) -> int {                  // 16-byte copies when every row of both sides is 16-byte aligned
        constexpr int E = Vec<decltype(elem)>::E;
        const bool vec = st.D % E == 0 && st.row_stride % E == 0;
        return vec ? run(elem, std::true_type()) : run(elem, std::false_type());
    };
    switch (dtype) {
        case MDL_STORE_F32:
            return typed(float());
        case MDL_STORE_F16:
            return typed(_Float16());
        default:
            return typed(bf16_t());
    }
}

inline int chunks_of(int N) { return (N + BS_TOK - 1) / BS_TOK; }

// S5's second launch: one workgroup per output row, after the pass(es) that wrote the partials, on the same stream
int mean_combine(const Store& st, const Draw& dr, const MeanJob& job, hipStream_t stream) {
    hipLaunchKernelGGL(bag_mean_combine_kernel, dim3((unsigned)job.R), dim3(BS_THREADS), 0, stream, st, dr, job);
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

// The four entry points fill the records, say what is theirs alone -- which store base may be NULL, and for S3 / S4 the tiers' ranges --
// and then go through the same steps: check_call, nothing to do (MDL_OK), [tiered: the runtime's view of store_host], launch.
// check_tiers is the safety code in front of a kernel that reads host memory and stays whole: it states the tiers' rules again,
// none of which can fail by then, before it asks the runtime.

extern "C" int mdl_bag_sample(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                              const int32_t* bag, const int64_t* key_id, int64_t R, int N, int D, uint64_t seed, uint64_t counter,
                              float* out, int32_t* idx_out, void* stream) {
    const Store st = {store, nullptr, T_total, row_stride, T_total, off, n_bags, D};
    const Draw dr = {bag, key_id, seed, counter};
    const Call call = {false, R, N, 0, 0, nullptr, nullptr, out, nullptr, idx_out};
    if (store == nullptr) return MDL_E_ARG;
    const int rc = check_call(st, dr, call, dtype);
    if (rc != MDL_OK) return rc;
    if (R == 0) return MDL_OK;
    const SampleJob job = {N, chunks_of(N), R * chunks_of(N), out, idx_out};
    return launch(st, dr, job, Passes{false, 0}, dtype, (hipStream_t)stream);
}

extern "C" int mdl_bag_pack(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                            const int32_t* bag, const int64_t* key_id, const int64_t* cu, const int64_t* chunk_cu, int64_t R,
                            int64_t n_chunks, int64_t T_out, int D, uint64_t seed, uint64_t counter, float* out, int32_t* row_bag,
                            int32_t* idx_out, void* stream) {
    const Store st = {store, nullptr, T_total, row_stride, T_total, off, n_bags, D};
    const Draw dr = {bag, key_id, seed, counter};
    const Call call = {true, R, 0, n_chunks, T_out, cu, chunk_cu, out, row_bag, idx_out};
    if (store == nullptr) return MDL_E_ARG;
    const int rc = check_call(st, dr, call, dtype);
    if (rc != MDL_OK) return rc;
    if (R == 0 || T_out == 0 || n_chunks == 0) return MDL_OK;
    const PackJob job = {cu, chunk_cu, (int)R, T_out, n_chunks, out, row_bag, idx_out};
    return launch(st, dr, job, Passes{false, 0}, dtype, (hipStream_t)stream);
}

extern "C" int mdl_bag_sample_tiered(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev,
                                     const int64_t* off, int64_t n_bags, const int32_t* bag, const int64_t* key_id, int64_t R, int N, int D,
                                     uint64_t seed, uint64_t counter, float* out, int32_t* idx_out, int host_wgs, void* stream) {
    Store st = {store, store_host, T_dev, row_stride, T_total, off, n_bags, D};
    const Draw dr = {bag, key_id, seed, counter};
    const Call call = {false, R, N, 0, 0, nullptr, nullptr, out, nullptr, idx_out};
    if (T_dev < 0 || T_dev > T_total || host_wgs < 0) return MDL_E_ARG;
    if ((T_dev > 0 && store == nullptr) || (T_dev < T_total && store_host == nullptr)) return MDL_E_ARG;      // a tier of no rows has no base
    int rc = check_call(st, dr, call, dtype);
    if (rc != MDL_OK) return rc;
    if (R == 0) return MDL_OK;
    const SampleJob job = {N, chunks_of(N), R * chunks_of(N), out, idx_out};
    Passes passes = {true, 0};
    rc = check_tiers(store, store_host, dtype, row_stride, T_total, T_dev, D, host_wgs, job.items, &st.host, &passes.host_wgs);
    if (rc != MDL_OK) return rc;
    return launch(st, dr, job, passes, dtype, (hipStream_t)stream);
}

extern "C" int mdl_bag_pack_tiered(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev,
                                   const int64_t* off, int64_t n_bags, const int32_t* bag, const int64_t* key_id, const int64_t* cu,
                                   const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int64_t T_out, int D, uint64_t seed, uint64_t counter,
                                   float* out, int32_t* row_bag, int32_t* idx_out, int host_wgs, void* stream) {
    Store st = {store, store_host, T_dev, row_stride, T_total, off, n_bags, D};
    const Draw dr = {bag, key_id, seed, counter};
    const Call call = {true, R, 0, n_chunks, T_out, cu, chunk_cu, out, row_bag, idx_out};
    if (T_dev < 0 || T_dev > T_total || host_wgs < 0) return MDL_E_ARG;
    if ((T_dev > 0 && store == nullptr) || (T_dev < T_total && store_host == nullptr)) return MDL_E_ARG;      // a tier of no rows has no base
    int rc = check_call(st, dr, call, dtype);
    if (rc != MDL_OK) return rc;
    if (R == 0 || T_out == 0 || n_chunks == 0) return MDL_OK;
    const PackJob job = {cu, chunk_cu, (int)R, T_out, n_chunks, out, row_bag, idx_out};
    Passes passes = {true, 0};
    rc = check_tiers(store, store_host, dtype, row_stride, T_total, T_dev, D, host_wgs, job.items, &st.host, &passes.host_wgs);
    if (rc != MDL_OK) return rc;
    return launch(st, dr, job, passes, dtype, (hipStream_t)stream);
}

// S5: the partial sums go through the same steps with a MeanJob, then the combine kernel is launched on the same stream.
extern "C" int64_t mdl_bag_mean_ws_bytes(int64_t n_chunks, int D) {
    if (n_chunks < 0 || D < 1) return MDL_E_ARG;
    if (n_chunks > 0x7FFFFFFF) return MDL_E_UNSUPPORTED;
    return n_chunks * (int64_t)D * (int64_t)sizeof(float);
}

extern "C" int mdl_bag_mean(const void* store, int dtype, int64_t row_stride, int64_t T_total, const int64_t* off, int64_t n_bags,
                            const int32_t* bag, const int64_t* chunk_cu, int64_t R, int64_t n_chunks, int D, float* out, void* ws,
                            void* stream) {
    const Store st = {store, nullptr, T_total, row_stride, T_total, off, n_bags, D};
    const Draw dr = {bag, nullptr, 0, 0};
    const Call call = {true, R, 0, n_chunks, 0, chunk_cu, chunk_cu, out, nullptr, nullptr, ws};
    if (store == nullptr || ws == nullptr) return MDL_E_ARG;
    int rc = check_call(st, dr, call, dtype);
    if (rc != MDL_OK) return rc;
    if (R == 0 || n_chunks == 0) return MDL_OK;
    const MeanJob job = {chunk_cu, (int)R, n_chunks, static_cast<float*>(ws), out};
    rc = launch(st, dr, job, Passes{false, 0}, dtype, (hipStream_t)stream);
    return rc != MDL_OK ? rc : mean_combine(st, dr, job, (hipStream_t)stream);
}

extern "C" int mdl_bag_mean_tiered(const void* store, const void* store_host, int dtype, int64_t row_stride, int64_t T_total, int64_t T_dev,
                                   const int64_t* off, int64_t n_bags, const int32_t* bag, const int64_t* chunk_cu, int64_t R,
                                   int64_t n_chunks, int D, float* out, void* ws, int host_wgs, void* stream) {
    Store st = {store, store_host, T_dev, row_stride, T_total, off, n_bags, D};
    const Draw dr = {bag, nullptr, 0, 0};
    const Call call = {true, R, 0, n_chunks, 0, chunk_cu, chunk_cu, out, nullptr, nullptr, ws};
    if (T_dev < 0 || T_dev > T_total || host_wgs < 0 || ws == nullptr) return MDL_E_ARG;
    if ((T_dev > 0 && store == nullptr) || (T_dev < T_total && store_host == nullptr)) return MDL_E_ARG;      // a tier of no rows has no base
    int rc = check_call(st, dr, call, dtype);
    if (rc != MDL_OK) return rc;
    if (R == 0 || n_chunks == 0) return MDL_OK;
    const MeanJob job = {chunk_cu, (int)R, n_chunks, static_cast<float*>(ws), out};
    Passes passes = {true, 0};
    rc = check_tiers(store, store_host, dtype, row_stride, T_total, T_dev, D, host_wgs, job.items, &st.host, &passes.host_wgs);
    if (rc != MDL_OK) return rc;
    rc = launch(st, dr, job, passes, dtype, (hipStream_t)stream);
    return rc != MDL_OK ? rc : mean_combine(st, dr, job, (hipStream_t)stream);
}
