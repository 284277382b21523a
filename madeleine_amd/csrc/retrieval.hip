// retrieval.hip -- X1: cross-stain retrieval over embedding matrices (include/madeleine_amd.h, X1).  Queries Q [n, d] against a gallery
// K [m, d]: the rank of every query's partner among all gallery rows (exact integer counts) and / or the k best gallery rows of every
// query, from similarity tiles that are consumed where they are produced.  The [n, m] matrix is never written to memory.
//
//   1. rt_normalize_kernel: one wave per row writes x / max(|x|, 1e-12) (cosine; InfoNCE's rule) or x (dot) into zero-padded copies
//      Qn [n_pad, dp], Kn [m_pad, dp] (rows to a multiple of the tile, columns to a multiple of RT_BK), so the product needs no bounds.
//   2. rt_stream_kernel: workgroup (row block, column chunk) owns RT_BM query rows and streams the chunk's RT_BN-column gallery tiles
//      past them.  A tile is a 128 x 128 x dp product on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) from LDS operand tiles; wave w
//      holds rows 32 w .. 32 w + 31 of it, so a row's state belongs to ONE wave: lane r of the wave keeps the partner key, the two
//      counts and the k-th best key of row r, and the row's sorted top-k list lies in LDS.  The finished tile goes through LDS (the
//      operand buffer, reused) and is read back a row at a time, a lane per column: two ballots count, a third finds the columns that
//      beat the k-th best, and only those are inserted.  In paired mode the tile that holds the partners is computed first.
//   3. rt_finish_kernel: one wave per query adds the chunk counts (integers) and merges the chunk lists.
//
// s_ij is ONE fmaf chain over k = 0 .. dp - 1 in an order fixed by dp (within every 8: 0, 4, 1, 5, 2, 6, 3, 7), on the normalised rows,
// whose bits are a function of the row alone: the bits of s_ij depend on row i of Q and row j of K and nothing else.  The trailing zeros
// of the padding leave the chain's value as it is.  Every comparison is made on rt_key (descending value, -0 = +0, every NaN one key
// below -inf), ties by the lower gallery index: a total order, so no output depends on the chunking or on scheduling.
// Launch order is the only dependency between workgroups; no atomics, no host read.
#include "common.hpp"

namespace mdl {
namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_BM = MDL_RETR_ROW_BLOCK;      // query rows per workgroup: 4 waves x 32
constexpr int RT_BN = MDL_RETR_COL_TILE;       // gallery rows per tile: 4 MFMA column blocks per wave
constexpr int RT_BK = 32;                      // contraction per LDS stage
constexpr int RT_LDT = RT_BK + 4;              // LDS row stride (floats): 16-byte rows, conflict-free 16-byte reads down a column of rows
constexpr int RT_PASS = 64;                    // columns of the finished tile handed to the row pass at a time (a lane each)
static_assert(RT_BM == 128 && RT_BN == 128 && RT_THREADS == 256, "the thread maps below are written for these");
static_assert(4 * 32 * RT_PASS <= 2 * RT_BM * RT_LDT, "the row pass reuses the operand buffer");

struct Geo {
    int64_t n_pad, m_pad;
    int dp, row_blocks, col_tiles, tiles_per_chunk, chunks;
};
// col_chunks == 0: enough chunks for MDL_RETR_TARGET_WGS workgroups, at most one per tile and MDL_RETR_MAX_CHUNKS.  A function of the
// sizes alone, so the workspace query and the call agree.
inline Geo geometry(int64_t n, int64_t m, int64_t d, int col_chunks) {
    Geo g;
    g.row_blocks = (int)((n + RT_BM - 1) / RT_BM);
    g.col_tiles = (int)((m + RT_BN - 1) / RT_BN);
    g.n_pad = (int64_t)g.row_blocks * RT_BM;
    g.m_pad = (int64_t)g.col_tiles * RT_BN;
    g.dp = (int)((d + RT_BK - 1) / RT_BK * RT_BK);
    int c = col_chunks > 0 ? col_chunks : (MDL_RETR_TARGET_WGS + g.row_blocks - 1) / g.row_blocks;
    if (c > MDL_RETR_MAX_CHUNKS) c = MDL_RETR_MAX_CHUNKS;
    if (c > g.col_tiles) c = g.col_tiles;
    if (c < 1) c = 1;
    g.tiles_per_chunk = (g.col_tiles + c - 1) / c;
    g.chunks = (g.col_tiles + g.tiles_per_chunk - 1) / g.tiles_per_chunk;
    return g;
}

struct Ws {
    float *Qn, *Kn;          // [n_pad, dp], [m_pad, dp]
    uint64_t* lists;         // [chunks, n_pad, k]   (key << 32 | ~index), descending; 0 = no entry
    int32_t *pg, *pe;        // [chunks, n_pad]
    int64_t bytes;
};
inline Ws carve(void* ws, const Geo& g, int k) {
    char* base = (char*)ws;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char* p = base + off;
        off += (bytes + 255) & ~(int64_t)255;
        return p;
    };
    Ws w;
    w.Qn = (float*)take(g.n_pad * g.dp * 4);
    w.Kn = (float*)take(g.m_pad * g.dp * 4);
    w.lists = (uint64_t*)take((int64_t)g.chunks * g.n_pad * k * 8);
    w.pg = (int32_t*)take((int64_t)g.chunks * g.n_pad * 4);
    w.pe = (int32_t*)take((int64_t)g.chunks * g.n_pad * 4);
    w.bytes = off;
    return w;
}

// ---- the order ------------------------------------------------------------------------------------------------------------------
// A larger key is retrieved earlier.  Numbers: the usual monotone map of the fp32 bits (-0 first made +0), from 0x007fffff (-inf)
// upwards; every NaN: 1; 0 is kept for "no entry".
__device__ __forceinline__ uint32_t rt_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (v != v) return 1u;
    if (v == 0.f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rt_value(uint32_t key) {
    if (key == 1u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
__device__ __forceinline__ uint64_t rt_entry(uint32_t key, uint32_t col) { return ((uint64_t)key << 32) | (uint32_t)~col; }

__device__ __forceinline__ uint64_t rt_readlane64(uint64_t v, int l) {      // l uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
// lane i <- lane i - 1 over the whole wave on the DPP network (wave_shr:1); lane 0 keeps its own value
__device__ __forceinline__ uint32_t rt_wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false);
}
// L: a descending list, one entry per lane.  Puts c (uniform) where it belongs; the last lane's entry falls off.  Whole wave.
__device__ __forceinline__ void rt_insert(uint64_t& L, uint64_t c, int lane) {
    const int pos = __popcll(__ballot(L > c));
    const uint64_t up = ((uint64_t)rt_wave_shr1((uint32_t)(L >> 32)) << 32) | rt_wave_shr1((uint32_t)L);
    L = lane < pos ? L : (lane == pos ? c : up);
}

// ---- 1. normalise ---------------------------------------------------------------------------------------------------------------
// Block b < n_pad: row b of Q, else row b - n_pad of K.  The sum of squares is one fmaf chain per lane (columns lane, lane + 64, ..)
// and the xor butterfly: a function of the row and d alone.
__global__ __launch_bounds__(64) void rt_normalize_kernel(const float* __restrict__ Q, int64_t ldq, int64_t n, int64_t n_pad,
                                                          const float* __restrict__ K, int64_t ldk, int64_t m, int d, int dp, int cosine,
                                                          float* __restrict__ Qn, float* __restrict__ Kn) {
    const int64_t b = blockIdx.x;
    const bool gal = b >= n_pad;
    const int64_t r = gal ? b - n_pad : b, rows = gal ? m : n;
    const int lane = (int)threadIdx.x;
    float* __restrict__ dst = (gal ? Kn : Qn) + r * dp;
    if (r >= rows) {
        for (int c = lane; c < dp; c += 64) dst[c] = 0.f;
        return;
    }
    const float* __restrict__ src = gal ? K + r * ldk : Q + r * ldq;
    float inv = 1.f;
    if (cosine) {
        float ss = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float x = src[c];
            ss = fmaf(x, x, ss);
        }
        ss = wave_sum(ss);
        inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    }
    for (int c = lane; c < dp; c += 64) dst[c] = c < d ? (cosine ? src[c] * inv : src[c]) : 0.f;
}

// ---- 2. stream ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rt_acc_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// KCAP: entries of a row's list in LDS (0: no top-k), k <= KCAP.  grid (row_blocks, chunks).
template <int KCAP>
__global__ __launch_bounds__(RT_THREADS) void rt_stream_kernel(const float* __restrict__ Qn, const float* __restrict__ Kn, int dp, int64_t n,
                                                               int64_t m, int64_t n_pad, int paired, int exclude_diag, int k,
                                                               int tiles_per_chunk, int col_tiles, float* __restrict__ pair_sim,
                                                               int32_t* __restrict__ pg, int32_t* __restrict__ pe,
                                                               uint64_t* __restrict__ pl) {
    __shared__ __attribute__((aligned(16))) float ops[2 * RT_BM * RT_LDT];      // A tile | B tile; the finished tile after the product
    __shared__ uint64_t lists[RT_BM * (KCAP ? KCAP : 1)];
    const int tid = (int)threadIdx.x, lane = tid & 63, l32 = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = (int)blockIdx.x, chunk = (int)blockIdx.y;
    const int64_t i0 = (int64_t)rb * RT_BM;
    const int t0 = chunk * tiles_per_chunk, t1 = t0 + tiles_per_chunk < col_tiles ? t0 + tiles_per_chunk : col_tiles;
    const int lead = paired ? 1 : 0, ntiles = (t1 - t0) + lead, nkb = dp / RT_BK;
    if (KCAP)
        for (int e = tid; e < RT_BM * KCAP; e += RT_THREADS) lists[e] = 0;

    // lane r < 32 of wave w: the state of row 32 w + r of the block
    uint32_t pk = 0;
    int cg = 0, ce = 0;
    uint64_t thr = 0;

    // operand loads: thread -> rows (tid >> 3) + 32 p, floats (tid & 7) * 4 .. + 3 of the stage
    const int lr = tid >> 3, lc = (tid & 7) * 4;
    const int64_t pstride = (int64_t)32 * dp;
    const float* __restrict__ asrc = Qn + (i0 + lr) * dp + lc;
    f32x4 pa[4], pb[4];
#define RT_TILE_OF(s) ((paired && (s) == 0) ? rb : t0 + (s)-lead)
#define RT_FETCH(s, kb)                                                                          \
    do {                                                                                         \
        const float* __restrict__ bsrc = Kn + ((int64_t)RT_TILE_OF(s) * RT_BN + lr) * dp + lc;   \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                          \
            pa[p] = ld4(asrc + p * pstride + (kb)*RT_BK);                                        \
            pb[p] = ld4(bsrc + p * pstride + (kb)*RT_BK);                                        \
        }                                                                                        \
    } while (0)
    RT_FETCH(0, 0);

    const float* As = ops + (wave * 32 + l32) * RT_LDT + kh * 4;
    const float* Bs = ops + RT_BM * RT_LDT + l32 * RT_LDT + kh * 4;
    float* sc = ops + wave * (32 * RT_PASS);

#pragma unroll 1
    for (int s = 0; s < ntiles; ++s) {
        f32x16 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
#pragma unroll 1
        for (int kb = 0; kb < nkb; ++kb) {
            __syncthreads();      // the previous stage (or the row pass) has been read
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                st4(ops + (lr + 32 * p) * RT_LDT + lc, pa[p]);
                st4(ops + RT_BM * RT_LDT + (lr + 32 * p) * RT_LDT + lc, pb[p]);
            }
            __syncthreads();
            if (kb + 1 < nkb) RT_FETCH(s, kb + 1);
            else if (s + 1 < ntiles) RT_FETCH(s + 1, 0);
#pragma unroll
            for (int k8 = 0; k8 < RT_BK / 8; ++k8) {
                const f32x4 a = ld4(As + k8 * 8);
                f32x4 b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) b[u] = ld4(Bs + u * 32 * RT_LDT + k8 * 8);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[u][i], acc[u], 0, 0, 0);
            }
        }
        // the finished tile, RT_PASS columns at a time: accumulators -> this wave's rows in LDS -> a row per trip, a lane per column
        const int jt = RT_TILE_OF(s);
        const bool partner_tile = paired && s == 0;
#pragma unroll      // the accumulators are indexed by `pass`: unrolled, they stay in registers
        for (int pass = 0; pass < RT_BN / RT_PASS; ++pass) {
            __syncthreads();
#pragma unroll
            for (int u2 = 0; u2 < 2; ++u2)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[rt_acc_row(r, kh) * RT_PASS + u2 * 32 + l32] = acc[pass * 2 + u2][r];
            __syncthreads();
            if (partner_tile) {      // row 32 w + r meets its partner in column 32 w + r of the tile
                if ((wave >> 1) == pass && lane < 32) {
                    const float v = sc[lane * RT_PASS + (wave & 1) * 32 + lane];
                    pk = rt_key(v);
                    const int64_t row = i0 + wave * 32 + lane;
                    if (chunk == 0 && row < n) pair_sim[row] = v;
                }
                continue;
            }
            const int64_t col = (int64_t)jt * RT_BN + pass * RT_PASS + lane;
            const bool live = col < m;
#pragma unroll 1
            for (int rr = 0; rr < 32; ++rr) {
                const int64_t row = i0 + wave * 32 + rr;
                if (row >= n) break;      // uniform
                const uint32_t key = rt_key(sc[rr * RT_PASS + lane]);
                if (paired) {
                    const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pk, rr);
                    const bool other = live && col != row;
                    const int g = __popcll(__ballot(other && key > p)), e = __popcll(__ballot(other && key == p));
                    if (lane == rr) {
                        cg += g;
                        ce += e;
                    }
                }
                if (KCAP) {
                    const uint64_t cand = rt_entry(key, (uint32_t)col);
                    uint64_t tt = rt_readlane64(thr, rr);
                    uint64_t hits = __ballot(live && !(exclude_diag && col == row) && cand > tt);
                    if (hits) {      // uniform
                        uint64_t* Lp = lists + (wave * 32 + rr) * (KCAP ? KCAP : 1);
                        uint64_t L = lane < k ? Lp[lane] : 0;
                        while (hits) {
                            const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)hits) - 1);
                            hits &= hits - 1;
                            const uint64_t c = rt_readlane64(cand, src);
                            if (c > tt) {
                                rt_insert(L, c, lane);
                                tt = rt_readlane64(L, k - 1);
                            }
                        }
                        if (lane < k) Lp[lane] = L;
                        if (lane == rr) thr = tt;
                    }
                }
            }
        }
    }
#undef RT_FETCH
#undef RT_TILE_OF
    if (paired && lane < 32) {
        const int64_t o = (int64_t)chunk * n_pad + i0 + wave * 32 + lane;
        pg[o] = cg;
        pe[o] = ce;
    }
    if (KCAP) {
        __syncthreads();
        for (int e = tid; e < RT_BM * k; e += RT_THREADS) {
            const int row = e / k, q = e - row * k;
            pl[((int64_t)chunk * n_pad + i0 + row) * k + q] = lists[row * (KCAP ? KCAP : 1) + q];
        }
    }
}

// ---- 3. finish ------------------------------------------------------------------------------------------------------------------
// One wave per query: the chunk counts added as integers, a NaN partner ranked last, the chunk lists merged (each is sorted, so a
// chunk is left at its first entry that does not make the list).
__global__ __launch_bounds__(RT_THREADS) void rt_finish_kernel(int64_t n, int64_t n_pad, int64_t m, int chunks, int paired, int k,
                                                               const int32_t* __restrict__ pg, const int32_t* __restrict__ pe,
                                                               const uint64_t* __restrict__ pl, const float* __restrict__ pair_sim,
                                                               int32_t* __restrict__ greater, int32_t* __restrict__ equal,
                                                               int32_t* __restrict__ topk_idx, float* __restrict__ topk_val) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (RT_THREADS / 64) + ((int)threadIdx.x >> 6);
    if (row >= n) return;      // uniform in the wave
    if (paired) {
        int g = 0, e = 0;
        for (int c = lane; c < chunks; c += 64) {
            g += pg[(int64_t)c * n_pad + row];
            e += pe[(int64_t)c * n_pad + row];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            g += __shfl_xor(g, o, 64);
            e += __shfl_xor(e, o, 64);
        }
        if (lane == 0) {
            const float ps = pair_sim[row];
            if (ps != ps) {
                g = (int)(m - 1);
                e = 0;
            }
            greater[row] = g;
            equal[row] = e;
        }
    }
    if (k > 0) {
        uint64_t L = lane < k ? pl[row * k + lane] : 0;
        for (int c = 1; c < chunks; ++c) {
            const uint64_t C = lane < k ? pl[((int64_t)c * n_pad + row) * k + lane] : 0;
            uint64_t tt = rt_readlane64(L, k - 1);
            for (int e = 0; e < k; ++e) {
                const uint64_t cnd = rt_readlane64(C, e);
                if (cnd <= tt) break;      // uniform
                rt_insert(L, cnd, lane);
                tt = rt_readlane64(L, k - 1);
            }
        }
        if (lane < k) {
            topk_idx[row * k + lane] = L ? (int32_t)~(uint32_t)L : -1;
            topk_val[row * k + lane] = L ? rt_value((uint32_t)(L >> 32)) : -INFINITY;
        }
    }
}


int check_sizes(int64_t n, int64_t m, int64_t d, int k, int col_chunks) {
    if (n < 1 || m < 1 || d < 1 || k < 0 || col_chunks < 0) return MDL_E_ARG;
    if (n > MDL_RETR_MAX_ROWS || m > MDL_RETR_MAX_ROWS || d > MDL_RETR_MAX_D || k > MDL_RETR_MAX_K || col_chunks > MDL_RETR_MAX_CHUNKS)
        return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

#define RT_LAUNCH(kernel, grid, block, ...)                                                     \
    do {                                                                                        \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);     \
        MDL_LAUNCH_CHECK();                                                                     \
    } while (0)

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_retrieval_ws_bytes(int64_t n, int64_t m, int64_t d, int k, int col_chunks) {
    if (const int rc = check_sizes(n, m, d, k, col_chunks)) return rc;
    return carve(nullptr, geometry(n, m, d, col_chunks), k).bytes;
}

extern "C" int mdl_retrieval(const float* Q, int64_t ldq, const float* K, int64_t ldk, int64_t n, int64_t m, int64_t d, int metric,
                             int paired, int exclude_diag, int k, int col_chunks, int32_t* greater, int32_t* equal, float* pair_sim,
                             int32_t* topk_idx, float* topk_val, void* ws, void* stream) {
    if (!Q || !K || !ws || n < 1 || m < 1 || d < 1 || ldq < d || ldk < d || k < 0 || col_chunks < 0) return MDL_E_ARG;
    if ((metric != MDL_RETR_COSINE && metric != MDL_RETR_DOT) || (paired != 0 && paired != 1) || (exclude_diag != 0 && exclude_diag != 1))
        return MDL_E_ARG;
    if ((paired && exclude_diag) || (paired && n > m) || (!paired && k == 0)) return MDL_E_ARG;
    if (paired && (!greater || !equal || !pair_sim)) return MDL_E_ARG;
    if (k > 0 && (!topk_idx || !topk_val)) return MDL_E_ARG;
    if (!aligned_to(Q, 4) || !aligned_to(K, 4) || !aligned_to(greater, 4) || !aligned_to(equal, 4) || !aligned_to(pair_sim, 4) ||
        !aligned_to(topk_idx, 4) || !aligned_to(topk_val, 4) || !host_aligned16(ws))
        return MDL_E_ALIGN;
    if (const int rc = check_sizes(n, m, d, k, col_chunks)) return rc;
    // every offset into Q and K is formed in 64 bits
    if (ldq > (0x7fffffffffffffffLL / 4 - d) / n || ldk > (0x7fffffffffffffffLL / 4 - d) / m) return MDL_E_UNSUPPORTED;
    const Geo g = geometry(n, m, d, col_chunks);
    const Ws w = carve(ws, g, k);
    RT_LAUNCH(rt_normalize_kernel, dim3((unsigned)(g.n_pad + g.m_pad)), 64, Q, ldq, n, g.n_pad, K, ldk, m, (int)d, g.dp,
              metric == MDL_RETR_COSINE ? 1 : 0, w.Qn, w.Kn);
    const dim3 grid((unsigned)g.row_blocks, (unsigned)g.chunks);
#define RT_STREAM(KCAP)                                                                                                                \
    RT_LAUNCH(rt_stream_kernel<KCAP>, grid, RT_THREADS, (const float*)w.Qn, (const float*)w.Kn, g.dp, n, m, g.n_pad, paired, exclude_diag, \
              k, g.tiles_per_chunk, g.col_tiles, pair_sim, w.pg, w.pe, w.lists)
    if (k == 0) RT_STREAM(0);
    else if (k <= 16) RT_STREAM(16);
    else RT_STREAM(64);
#undef RT_STREAM
    RT_LAUNCH(rt_finish_kernel, dim3((unsigned)((n + RT_THREADS / 64 - 1) / (RT_THREADS / 64))), RT_THREADS, n, g.n_pad, m, g.chunks, paired, k,
              (const int32_t*)w.pg, (const int32_t*)w.pe, (const uint64_t*)w.lists, (const float*)pair_sim, greater, equal, topk_idx,
              topk_val);
    return MDL_OK;
}
