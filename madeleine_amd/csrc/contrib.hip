// contrib.hip -- patch contributions of a linear probe's decision (include/madeleine_amd_explain.h, X1 and X2).
//
//   ac_kernel           out[t, h, c] = attn[t, h] * <U[c, h, :], E[t, h, :]> and total[t, c] = the heads added in ascending order.  HBM-bound
//                       by design: E (2 KiB per row and head in fp32) is read once with 16-byte non-temporal loads.  A wave owns one head
//                       for the whole launch and keeps its 512 x C slice of U in registers (8 C VGPRs), so the only traffic besides E is
//                       attn and the outputs; plain FMAs, two columns to an instruction (v_pk_fma_f32; at C = 8: 32 a lane per row and
//                       head), the 64 partials of all columns added in one transposed butterfly (wave_sum8).  A workgroup is max(4, H)
//                       waves = max(4, H) / H row slots x H heads; a wave takes 4 (fp32) or 8 (bf16) rows per round (all loads of the
//                       round are issued before the first FMA), leaves its products in LDS and, after the round's one barrier, the first
//                       threads add the heads of every row.  Two LDS buffers: a wave can be at most one round ahead of the reader.
//   cs_plan_kernel      one workgroup: cu -> the segment table (first row, rows, first chunk of every bag), as the attention read-out's.
//   cs_chunk_kernel     a workgroup per chunk of MDL_CONTRIB_ROWS rows and per column: the four partial statistics of the chunk.
//   cs_seg_kernel       a thread per (bag, statistic, column): the bag's chunks in ascending order.
// No atomics, no workgroup waits on another, every loop is bounded by an argument.
#include "common.hpp"

#include "../../include/madeleine_amd_explain.h"

namespace mdl {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

constexpr int AC_MAX_GRID = 2048;               // 8 workgroups a CU: more than are resident (3-7 waves a SIMD), so no CU idles
constexpr int CS_C = MDL_CONTRIB_ROWS;
constexpr int CS_THREADS = 256;
constexpr int CS_PER = CS_C / CS_THREADS;
static_assert(HID == 512 && CS_C % CS_THREADS == 0, "a head row is 8 elements a lane; chunk geometry");

// The 8 elements of lane `lane` of a head row (header: fp32 e = 4 l + j and 256 + 4 l + j; bf16 e = 8 l + j), in ascending e.
__device__ __forceinline__ f32x8 load8(const float* head, int lane) {
    const f32x4 a = ld4_nt(head + 4 * lane), b = ld4_nt(head + HID / 2 + 4 * lane);
    return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ bf16x8 load8(const bf16_t* head, int lane) {
    return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(head + 8 * lane));
}
// A loaded head row slice stays as it was stored until its FMAs (bf16: 4 registers instead of 8, which is what lets a wave take 8 rows
// a round); widening is exact.
__device__ __forceinline__ f32x8 widen(f32x8 v) { return v; }
__device__ __forceinline__ f32x8 widen(bf16x8 v) { return __builtin_convertvector(v, f32x8); }
template <typename TE> struct Stored { typedef f32x8 type; };
template <> struct Stored<bf16_t> { typedef bf16x8 type; };
// rows of a wave per round: 8 KiB of E in flight a wave for either storage type
template <typename TE> constexpr int rows_per_round() { return sizeof(TE) == 4 ? 4 : 8; }
// U is read where E is: the slice of a lane follows the element order of the storage type.
template <typename TE>
__device__ __forceinline__ f32x8 load_u(const float* head, int lane) {
    if constexpr (sizeof(TE) == 4) {
        const f32x4 a = ld4(head + 4 * lane), b = ld4(head + HID / 2 + 4 * lane);
        return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    } else {
        const f32x4 a = ld4(head + 8 * lane), b = ld4(head + 8 * lane + 4);
        return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    }
}

// 8 values a lane -> their 8 sums over the wave, one a lane: the lanes whose low three bits are (b0, b1, b2) end with the sum of value
// b2 + 2 b1 + 4 b0.  Three exchange stages (lane ^ 1, ^ 2, ^ 4) in which a lane keeps one half of its values and adds the partner's copy
// of them, then lane ^ 8, ^ 16, ^ 32 on the one value left: every value is added as the balanced binary tree over the lanes in lane
// order (addition commutes exactly, so who holds a partial does not matter), at 27 instructions instead of 8 x 11.
template <int PATTERN>
__device__ __forceinline__ float swizzle(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), PATTERN));
}
__device__ __forceinline__ float wave_sum8(const float (&p)[8], int lane) {
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    float q[4], r[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (b0 ? p[i + 4] : p[i]) + dpp_mov<0xB1>(b0 ? p[i] : p[i + 4]);         // quad_perm [1,0,3,2]
#pragma unroll
    for (int i = 0; i < 2; ++i) r[i] = (b1 ? q[i + 2] : q[i]) + dpp_mov<0x4E>(b1 ? q[i] : q[i + 2]);         // quad_perm [2,3,0,1]
    float s = (b2 ? r[1] : r[0]) + swizzle<0x101F>(b2 ? r[0] : r[1]);                                        // lane ^ 4
    s += dpp_mov<0x128>(s);                                                                                  // row_ror:8 = lane ^ 8
    s += swizzle<0x401F>(s);                                                                                 // lane ^ 16
    s += __shfl_xor(s, 32, 64);
    return s;
}

template <typename TE, int C, int NW>
__global__ __launch_bounds__(NW* WAVE) void ac_kernel(const TE* __restrict__ E, int64_t ldE, const float* __restrict__ attn, int64_t ldA,
                                                      const float* __restrict__ U, int T, int H, float* __restrict__ per_head,
                                                      float* __restrict__ total, int64_t ldO, int ntiles) {
    constexpr int AC_RW = rows_per_round<TE>();
    __shared__ float s_part[2][NW * AC_RW][MDL_CONTRIB_MAX_C];      // [buffer][row slot x head][column]
    constexpr int C2 = (C + 1) / 2;                                 // columns go in pairs: one packed FMA serves two of them
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);      // uniform: the row addresses are scalar arithmetic
    const int h = wave % H, slot = wave / H, slots = NW / H;
    const int tile_rows = slots * AC_RW;
    const int col = ((lane >> 2) & 1) | (lane & 2) | ((lane & 1) << 2);      // the column lane < 8 ends with (wave_sum8)
    f32x2 u[C2][8];
#pragma unroll
    for (int c = 0; c < C2; ++c) {
        const f32x8 lo = load_u<TE>(U + ((int64_t)(2 * c) * H + h) * HID, lane);
        f32x8 hi = f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (2 * c + 1 < C) hi = load_u<TE>(U + ((int64_t)(2 * c + 1) * H + h) * HID, lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) u[c][j] = f32x2{lo[j], hi[j]};
    }

    int buf = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1) {      // uniform over the workgroup
        const int64_t row0 = (int64_t)tile * tile_rows + slot * AC_RW;
        typename Stored<TE>::type e[AC_RW];
        float a[AC_RW];
#pragma unroll
        for (int i = 0; i < AC_RW; ++i) {
            const int64_t row = row0 + i;                                          // uniform over the wave
            if (row < T) {
                e[i] = load8(E + (int64_t)row * ldE + (int64_t)h * HID, lane);
                a[i] = attn[(int64_t)row * ldA + h];
            } else {
                e[i] = typename Stored<TE>::type{};
                a[i] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < AC_RW; ++i) {
            const int64_t row = row0 + i;
            float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const f32x8 ei = widen(e[i]);
#pragma unroll
            for (int c = 0; c < C2; ++c) {
                f32x2 acc = f32x2{0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 8; ++j) acc = __builtin_elementwise_fma(f32x2{ei[j], ei[j]}, u[c][j], acc);
                p[2 * c] = acc[0];
                p[2 * c + 1] = acc[1];
            }
            const float mine = a[i] * wave_sum8(p, lane);
            if (lane < 8 && col < C) {
                s_part[buf][(slot * AC_RW + i) * H + h][col] = mine;
                if (per_head != nullptr && row < T) per_head[((int64_t)row * H + h) * C + col] = mine;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < tile_rows * C) {
            const int r = threadIdx.x / C, c = threadIdx.x % C;
            const int64_t row = (int64_t)tile * tile_rows + r;
            if (row < T) {
                float t = s_part[buf][r * H][c];
                for (int hh = 1; hh < H; ++hh) t += s_part[buf][r * H + hh][c];
                total[(int64_t)row * ldO + c] = t;
            }
        }
    }
}

template <typename TE, int NW>
void ac_launch(int C, dim3 grid, hipStream_t stream, const TE* E, int64_t ldE, const float* attn, int64_t ldA, const float* U, int T, int H,
               float* per_head, float* total, int64_t ldO, int ntiles) {
#define AC_CASE(c)                                                                                                                   \
    case c:                                                                                                                          \
        hipLaunchKernelGGL((ac_kernel<TE, c, NW>), grid, dim3(NW* WAVE), 0, stream, E, ldE, attn, ldA, U, T, H, per_head, total, ldO, \
                           ntiles);                                                                                                  \
        break
    switch (C) {
        AC_CASE(1);
        AC_CASE(2);
        AC_CASE(3);
        AC_CASE(4);
        AC_CASE(5);
        AC_CASE(6);
        AC_CASE(7);
        AC_CASE(8);
    }
#undef AC_CASE
}

// ---- X2: the segment table (the plan of csrc/attn_map.hip, for chunks of MDL_CONTRIB_ROWS rows) -------------------------------------------
struct Ws {
    int32_t *seg_start, *seg_n, *chunk_cu;      // [R], [R], [R + 1]
    float* part;                                // [NC, 4, C]
    int64_t bytes;
};
inline int64_t max_chunks(int64_t T, int64_t R) { return T / CS_C + R; }       // sum ceil(n_r / CS_C) <= floor(T / CS_C) + R
inline Ws carve(void* base, int64_t T, int64_t R, int C) {
    char* p = reinterpret_cast<char*>(base);
    int64_t o = 0;
    const auto take = [&](int64_t bytes) { char* q = p + o; o += up16(bytes); return q; };
    Ws w;
    w.seg_start = reinterpret_cast<int32_t*>(take(R * 4));
    w.seg_n = reinterpret_cast<int32_t*>(take(R * 4));
    w.chunk_cu = reinterpret_cast<int32_t*>(take((R + 1) * 4));
    w.part = reinterpret_cast<float*>(take(max_chunks(T, R) * 4 * C * 4));
    w.bytes = o;
    return w;
}

__global__ __launch_bounds__(CS_THREADS) void cs_plan_kernel(const int64_t* __restrict__ cu, int R, int T, int NC,
                                                             int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_n,
                                                             int32_t* __restrict__ chunk_cu) {
    __shared__ int64_t s_scan[CS_THREADS];
    __shared__ int64_t s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_carry = 0;
        chunk_cu[0] = 0;
    }
    __syncthreads();
    for (int r0 = 0; r0 < R; r0 += CS_THREADS) {
        const int r = r0 + tid;
        int64_t a = 0, n = 0;
        if (r < R) {
            a = cu[r];
            const int64_t b = cu[r + 1];
            if (a >= 0 && a <= b && b <= (int64_t)T) n = b - a;
        }
        s_scan[tid] = (n + CS_C - 1) / CS_C;
        __syncthreads();
        for (int o = 1; o < CS_THREADS; o <<= 1) {            // inclusive scan of the tile's chunk counts
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
        if (tid == CS_THREADS - 1) s_carry = incl <= (int64_t)NC ? incl : (int64_t)NC + 1;
        __syncthreads();
    }
}

// max |.| that keeps a NaN: fmaxf alone would drop it.
__device__ __forceinline__ float nan_max(float m, float v) { return (m != m || v != v) ? __builtin_nanf("") : fmaxf(m, v); }

template <bool MAX>
__device__ __forceinline__ float cs_wg(float v, float* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = MAX ? nan_max(v, w) : v + w;
    }
    __syncthreads();                                          // s_red is reused by the four reductions of a chunk
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return MAX ? nan_max(nan_max(s_red[0], s_red[1]), nan_max(s_red[2], s_red[3])) : (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(CS_THREADS) void cs_chunk_kernel(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_n,
                                                              const int32_t* __restrict__ chunk_cu, int R, int C,
                                                              const float* __restrict__ contrib, int64_t ld, float* __restrict__ part) {
    const int chunk = blockIdx.x, c = blockIdx.y;
    if (chunk >= chunk_cu[R]) return;
    int lo = 0, hi = R - 1;
    while (lo < hi) {                                         // the first r with chunk_cu[r + 1] > chunk
        const int mid = (lo + hi) >> 1;
        if (chunk_cu[mid + 1] <= chunk) lo = mid + 1;
        else hi = mid;
    }
    const int start = seg_start[lo], n = seg_n[lo], k = chunk - chunk_cu[lo];
    if (k < 0 || (int64_t)k * CS_C >= n) return;
    __shared__ float s_red[CS_THREADS / WAVE];
    float sum = 0.f, pos = 0.f, neg = 0.f, amax = 0.f;
#pragma unroll
    for (int q = 0; q < CS_PER; ++q) {
        const int i = k * CS_C + q * CS_THREADS + threadIdx.x;
        const float v = i < n ? contrib[(int64_t)(start + i) * ld + c] : 0.f;
        const bool minus = (__builtin_bit_cast(uint32_t, v) >> 31) != 0;
        sum += v;
        pos += minus ? 0.f : v;
        neg += minus ? v : 0.f;
        amax = nan_max(amax, fabsf(v));
    }
    sum = cs_wg<false>(sum, s_red);
    pos = cs_wg<false>(pos, s_red);
    neg = cs_wg<false>(neg, s_red);
    amax = cs_wg<true>(amax, s_red);
    if (threadIdx.x == 0) {
        float* q = part + (int64_t)chunk * 4 * C + c;
        q[MDL_CONTRIB_SUM * C] = sum;
        q[MDL_CONTRIB_POS * C] = pos;
        q[MDL_CONTRIB_NEG * C] = neg;
        q[MDL_CONTRIB_ABSMAX * C] = amax;
    }
}

__global__ __launch_bounds__(CS_THREADS) void cs_seg_kernel(const int32_t* __restrict__ seg_n, const int32_t* __restrict__ chunk_cu, int R,
                                                            int C, const float* __restrict__ part, float* __restrict__ stats) {
    const int64_t g = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x;
    if (g >= (int64_t)R * 4 * C) return;
    const int r = (int)(g / (4 * C)), sc = (int)(g % (4 * C));      // sc = statistic * C + column
    const int nch = (seg_n[r] + CS_C - 1) / CS_C;
    const float* q = part + (int64_t)chunk_cu[r] * 4 * C + sc;
    float v = 0.f;
    if (nch > 0) {
        v = q[0];
        for (int k = 1; k < nch; ++k) {
            const float w = q[(int64_t)k * 4 * C];
            v = sc / C == MDL_CONTRIB_ABSMAX ? nan_max(v, w) : v + w;
        }
    }
    stats[g] = v;
}

int stats_sizes(int64_t T, int64_t R, int C) {
    if (T < 0 || R < 0 || C < 1) return MDL_E_ARG;
    if (C > MDL_CONTRIB_MAX_C || !i32(T) || !i32(R) || !i32(max_chunks(T, R))) return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

#define CT_LAUNCH(kernel, grid, block, ...)                                                     \
    do {                                                                                        \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);     \
        MDL_LAUNCH_CHECK();                                                                     \
    } while (0)

extern "C" int mdl_attn_contrib(const void* E, int64_t ldE, int e_dtype, const float* attn, int64_t ldA, const float* U, int64_t T, int H,
                                int W, int C, float* per_head, float* total, int64_t ldO, void* stream) {
    if (T < 0 || H < 1 || W < 1 || C < 1 || !U) return MDL_E_ARG;
    if (T > 0 && (!E || !attn || !total)) return MDL_E_ARG;
    if (ldE < (int64_t)H * W || ldA < H || ldO < C || (e_dtype != MDL_CONTRIB_E_F32 && e_dtype != MDL_CONTRIB_E_BF16)) return MDL_E_ARG;
    if ((H != 1 && H != 2 && H != 4 && H != 8) || W != HID || C > MDL_CONTRIB_MAX_C || !i32(T)) return MDL_E_UNSUPPORTED;
    if (!host_aligned16(E) || !host_aligned16(U) || ldE % (e_dtype == MDL_CONTRIB_E_F32 ? 4 : 8) != 0 || !aligned_to(attn, 4) ||
        !aligned_to(per_head, 4) || !aligned_to(total, 4))
        return MDL_E_ALIGN;
    if (T == 0) return MDL_OK;
    const int nw = H > 4 ? H : 4;
    const int tile_rows = nw / H * (e_dtype == MDL_CONTRIB_E_F32 ? rows_per_round<float>() : rows_per_round<bf16_t>());
    const int ntiles = (int)((T + tile_rows - 1) / tile_rows);
    const dim3 grid((unsigned)(ntiles < AC_MAX_GRID ? ntiles : AC_MAX_GRID));
    hipStream_t s = (hipStream_t)stream;
    if (e_dtype == MDL_CONTRIB_E_F32) {
        const float* e = reinterpret_cast<const float*>(E);
        if (nw == 4) ac_launch<float, 4>(C, grid, s, e, ldE, attn, ldA, U, (int)T, H, per_head, total, ldO, ntiles);
        else ac_launch<float, 8>(C, grid, s, e, ldE, attn, ldA, U, (int)T, H, per_head, total, ldO, ntiles);
    } else {
        const bf16_t* e = reinterpret_cast<const bf16_t*>(E);
        if (nw == 4) ac_launch<bf16_t, 4>(C, grid, s, e, ldE, attn, ldA, U, (int)T, H, per_head, total, ldO, ntiles);
        else ac_launch<bf16_t, 8>(C, grid, s, e, ldE, attn, ldA, U, (int)T, H, per_head, total, ldO, ntiles);
    }
    MDL_LAUNCH_CHECK();
    return MDL_OK;
}

extern "C" int64_t mdl_contrib_stats_ws_bytes(int64_t T, int64_t R, int C) {
    if (const int rc = stats_sizes(T, R, C)) return rc;
    return carve(nullptr, T, R, C).bytes;
}

extern "C" int mdl_contrib_stats(const float* contrib, int64_t ld, const int64_t* cu, int64_t T, int64_t R, int C, float* stats, void* ws,
                                 void* stream) {
    if (!cu || !stats || !ws || (T > 0 && !contrib) || ld < C) return MDL_E_ARG;
    if (const int rc = stats_sizes(T, R, C)) return rc;
    if (!i32(R * 4 * C)) return MDL_E_UNSUPPORTED;
    if (!host_aligned16(ws) || !aligned_to(cu, 8) || !aligned_to(contrib, 4) || !aligned_to(stats, 4)) return MDL_E_ALIGN;
    if (R == 0 || T == 0) return MDL_OK;
    const Ws w = carve(ws, T, R, C);
    const int NC = (int)max_chunks(T, R);
    CT_LAUNCH(cs_plan_kernel, dim3(1), CS_THREADS, cu, (int)R, (int)T, NC, w.seg_start, w.seg_n, w.chunk_cu);
    CT_LAUNCH(cs_chunk_kernel, dim3((unsigned)NC, (unsigned)C), CS_THREADS, (const int32_t*)w.seg_start, (const int32_t*)w.seg_n,
              (const int32_t*)w.chunk_cu, (int)R, C, contrib, ld, w.part);
    CT_LAUNCH(cs_seg_kernel, dim3((unsigned)((R * 4 * C + CS_THREADS - 1) / CS_THREADS)), CS_THREADS, (const int32_t*)w.seg_n,
              (const int32_t*)w.chunk_cu, (int)R, C, (const float*)w.part, stats);
    return MDL_OK;
}
