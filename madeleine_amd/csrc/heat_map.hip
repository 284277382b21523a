// heat_map.hip -- attention heatmaps (section V1 of include/madeleine_amd_view.h): patch coordinates and per-patch values of a packed
// set of bags become level / covered / RGBA planes by exact integer arithmetic.  All bags and channels of a call share every launch.
//
//   hv_plan_kernel        one workgroup: the per-bag records -> the tile table (first tile of every canvas).  A record that does not
//                         hold (canvas_ok) or that would push the tile count past the launch grid is an EMPTY canvas: no later kernel
//                         reads or writes anything of it.
//   hv_accumulate_kernel  a group of `lanes` lanes per patch walks the clipped footprint row-major and adds (1 << 40) + q into the packed
//                         word of every pixel, once per channel: the lanes of one atomic instruction touch consecutive words of a row.
//   hv_blur_rows_kernel   one tile with a halo of r columns through LDS: S1, N1.
//   hv_blur_cols_kernel   one tile with a halo of r rows through LDS: S2, N2, then level, covered and the colour.
// No workgroup waits on another: launch order is the only dependency.  The only atomics are 64-bit integer adds (their order cannot
// change a sum).  Every loop is bounded by an argument or a validated record.
#include "common.hpp"

#include "../../include/madeleine_amd_view.h"

namespace mdl {
namespace {

constexpr int HV_THREADS = 256;
constexpr int HV_TILE = MDL_HEAT_TILE;
constexpr int HV_MAX_R = MDL_HEAT_MAX_R;
constexpr int HV_SPAN = HV_TILE + 2 * HV_MAX_R;       // a tile with both halos
constexpr int HV_PER = HV_TILE * HV_TILE / HV_THREADS;      // pixels per thread of a tile
constexpr int HV_COUNT_SHIFT = 40;
constexpr uint64_t HV_SUM_MASK = (1ull << HV_COUNT_SHIFT) - 1ull;
constexpr int64_t HV_MAX_T = 1ll << 24;               // N < 2^24 and S < 2^24 * 65535 < 2^40: both fields of the packed word exact
constexpr int64_t HV_MAX_PS = 1ll << 24;
static_assert(HV_TILE * HV_TILE % HV_THREADS == 0 && HV_THREADS % HV_TILE == 0, "tile geometry");
static_assert(MDL_HEAT_WS_PER_PLANE_PIXEL == 3 * 8, "acc, S1, N1");

struct Taps {
    int32_t t[2 * HV_MAX_R + 1];
};

struct Canvas {
    int64_t ps, ox, oy, off;
    int W, H;
};

__host__ __device__ __forceinline__ int tiles_of(int n) { return (n + HV_TILE - 1) / HV_TILE; }

// 0: the record holds; MDL_E_ARG / MDL_E_UNSUPPORTED as the header states.  The host refuses the call with it, the device serves the
// canvas as an empty one.
__host__ __device__ __forceinline__ int canvas_check(const int64_t* rec, int64_t P, Canvas& c) {
    const int64_t ps = rec[MDL_HEAT_PS], ox = rec[MDL_HEAT_OX], oy = rec[MDL_HEAT_OY], W = rec[MDL_HEAT_W], H = rec[MDL_HEAT_H],
                  off = rec[MDL_HEAT_OFF];
    if (ps < 1 || W < 1 || H < 1 || off < 0) return MDL_E_ARG;
    if (W > MDL_HEAT_MAX_SIDE || H > MDL_HEAT_MAX_SIDE || ps > HV_MAX_PS) return MDL_E_UNSUPPORTED;
    if (ox < -0x7FFFFFFFLL || ox > 0x7FFFFFFFLL || oy < -0x7FFFFFFFLL || oy > 0x7FFFFFFFLL) return MDL_E_UNSUPPORTED;
    if (off > P || W * H > P - off) return MDL_E_ARG;
    c.ps = ps;
    c.ox = ox;
    c.oy = oy;
    c.off = off;
    c.W = (int)W;
    c.H = (int)H;
    return MDL_OK;
}

__host__ __device__ __forceinline__ int64_t floor_div(int64_t a, int64_t d) {      // d >= 1
    const int64_t q = a / d;
    return (a % d != 0 && a < 0) ? q - 1 : q;
}

// The workspace, carved in one place for the size query and the entry point.
struct Ws {
    int32_t* tile_cu;                 // [R + 1]
    uint64_t *acc, *s1, *n1;          // [C * P] each
    int64_t bytes;
};
inline Ws carve(void* base, int64_t P, int64_t R, int C) {
    char* p = reinterpret_cast<char*>(base);
    int64_t o = 0;
    const auto take = [&](int64_t bytes) { char* q = p + o; o += up16(bytes); return q; };
    Ws w;
    w.tile_cu = reinterpret_cast<int32_t*>(take((R + 1) * 4));
    w.acc = reinterpret_cast<uint64_t*>(take(C * P * 8));
    w.s1 = reinterpret_cast<uint64_t*>(take(C * P * 8));
    w.n1 = reinterpret_cast<uint64_t*>(take(C * P * 8));
    w.bytes = o;
    return w;
}

// ---- the tile table ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HV_THREADS) void hv_plan_kernel(const int64_t* __restrict__ bag, int R, int64_t P, int NT,
                                                             int32_t* __restrict__ tile_cu) {
    __shared__ int64_t s_scan[HV_THREADS];
    __shared__ int64_t s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_carry = 0;
        tile_cu[0] = 0;
    }
    __syncthreads();
    for (int b0 = 0; b0 < R; b0 += HV_THREADS) {
        const int b = b0 + tid;
        int64_t cnt = 0;
        if (b < R) {
            Canvas c;
            if (canvas_check(bag + (int64_t)b * MDL_HEAT_REC, P, c) == MDL_OK) cnt = (int64_t)tiles_of(c.W) * tiles_of(c.H);
        }
        s_scan[tid] = cnt;
        __syncthreads();
        for (int o = 1; o < HV_THREADS; o <<= 1) {            // inclusive scan of the slice's tile counts
            const int64_t add = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const int64_t incl = s_carry + s_scan[tid];
        if (b < R) tile_cu[b + 1] = (int32_t)(incl <= (int64_t)NT ? incl : (int64_t)NT);      // equal to NT at the end, with a record that
        __syncthreads();                                                                      // agrees with bag_host
        if (tid == HV_THREADS - 1) s_carry = incl <= (int64_t)NT ? incl : (int64_t)NT + 1;    // saturates: stays "past NT"
        __syncthreads();
    }
}

struct Tile {
    Canvas c;
    int x0, y0;      // the tile's first pixel
};

// The canvas and position of tile `tile` (uniform over the workgroup); false where the tile belongs to no canvas.
__device__ __forceinline__ bool find_tile(const int32_t* __restrict__ tile_cu, const int64_t* __restrict__ bag, int R, int64_t P, int tile,
                                          Tile& t) {
    if (tile >= tile_cu[R]) return false;
    int lo = 0, hi = R - 1;
    while (lo < hi) {                                         // the first b with tile_cu[b + 1] > tile
        const int mid = (lo + hi) >> 1;
        if (tile_cu[mid + 1] <= tile) lo = mid + 1;
        else hi = mid;
    }
    if (canvas_check(bag + (int64_t)lo * MDL_HEAT_REC, P, t.c) != MDL_OK) return false;
    const int local = tile - tile_cu[lo], tx = tiles_of(t.c.W);
    if (local < 0 || local >= tx * tiles_of(t.c.H)) return false;      // a canvas cut short by the saturated table
    t.x0 = (local % tx) * HV_TILE;
    t.y0 = (local / tx) * HV_TILE;
    return true;
}

// ---- steps 1 - 3 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HV_THREADS) void hv_accumulate_kernel(const int32_t* __restrict__ xy, const int64_t* __restrict__ cu,
                                                                   const float* __restrict__ values, int64_t ld, int T, int R, int C,
                                                                   const int64_t* __restrict__ bag, int64_t P, int ds, int lane_shift,
                                                                   uint64_t* __restrict__ acc) {
    const int64_t g = (int64_t)blockIdx.x * HV_THREADS + threadIdx.x;
    const int64_t i = g >> lane_shift;
    const int lanes = 1 << lane_shift, sub = (int)(g & (lanes - 1));
    if (i >= T) return;
    int lo = 0, hi = R - 1;
    while (lo < hi) {                                         // the first b with cu[b + 1] > i
        const int mid = (lo + hi) >> 1;
        if (cu[mid + 1] <= i) lo = mid + 1;
        else hi = mid;
    }
    const int64_t first = cu[lo], end = cu[lo + 1];
    if (!(first >= 0 && first <= i && i < end && end <= (int64_t)T)) return;      // a cu that is not monotone or leaves [0, T]
    Canvas c;
    if (canvas_check(bag + (int64_t)lo * MDL_HEAT_REC, P, c) != MDL_OK) return;
    const int64_t dx = (int64_t)xy[2 * i] - c.ox, dy = (int64_t)xy[2 * i + 1] - c.oy;
    int64_t x0 = floor_div(dx, ds), x1 = floor_div(dx + c.ps - 1, ds), y0 = floor_div(dy, ds), y1 = floor_div(dy + c.ps - 1, ds);
    x0 = x0 < 0 ? 0 : x0;
    y0 = y0 < 0 ? 0 : y0;
    x1 = x1 > c.W - 1 ? c.W - 1 : x1;
    y1 = y1 > c.H - 1 ? c.H - 1 : y1;
    if (x0 > x1 || y0 > y1) return;
    const int fw = (int)(x1 - x0 + 1), n = fw * (int)(y1 - y0 + 1);      // n <= 2^30
    const int64_t plane = (int64_t)c.W * c.H;
    for (int ch = 0; ch < C; ++ch) {
        const float v = values[i * ld + ch];
        if (v != v) continue;
        const uint32_t q = !(v > 0.f) ? 0u : v >= 1.f ? 65535u : (uint32_t)rintf(v * 65535.f);
        const uint64_t word = (1ull << HV_COUNT_SHIFT) + q;
        uint64_t* dst = acc + (int64_t)C * c.off + ch * plane;
        for (int k = sub; k < n; k += lanes)
            atomicAdd(reinterpret_cast<unsigned long long*>(dst + (y0 + k / fw) * c.W + (x0 + k % fw)), (unsigned long long)word);
    }
}

// ---- step 4, the row pass ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HV_THREADS) void hv_blur_rows_kernel(const int32_t* __restrict__ tile_cu, const int64_t* __restrict__ bag,
                                                                  int R, int C, int64_t P, Taps taps, int r,
                                                                  const uint64_t* __restrict__ acc, uint64_t* __restrict__ s1,
                                                                  uint64_t* __restrict__ n1) {
    Tile t;
    if (!find_tile(tile_cu, bag, R, P, blockIdx.x, t)) return;
    __shared__ uint64_t s_word[HV_TILE][HV_SPAN];
    const int ch = blockIdx.y, W = t.c.W, H = t.c.H, span = HV_TILE + 2 * r;
    const int64_t base = (int64_t)C * t.c.off + (int64_t)ch * W * H;
    for (int idx = threadIdx.x; idx < HV_TILE * span; idx += HV_THREADS) {
        const int ly = idx / span, lx = idx % span, gx = t.x0 + lx - r, gy = t.y0 + ly;
        s_word[ly][lx] = (gx >= 0 && gx < W && gy < H) ? acc[base + (int64_t)gy * W + gx] : 0ull;
    }
    __syncthreads();
    const int lx = threadIdx.x % HV_TILE;
#pragma unroll
    for (int j = 0; j < HV_PER; ++j) {
        const int ly = threadIdx.x / HV_TILE + j * (HV_THREADS / HV_TILE);
        uint64_t s = 0, n = 0;
        for (int k = 0; k <= 2 * r; ++k) {
            const uint64_t w = s_word[ly][lx + k], tap = (uint64_t)taps.t[k];
            s += tap * (w & HV_SUM_MASK);
            n += tap * (w >> HV_COUNT_SHIFT);
        }
        const int gx = t.x0 + lx, gy = t.y0 + ly;
        if (gx < W && gy < H) {
            s1[base + (int64_t)gy * W + gx] = s;
            n1[base + (int64_t)gy * W + gx] = n;
        }
    }
}

// ---- step 4, the column pass, and steps 5 - 6 --------------------------------------------------------------------------------------
__global__ __launch_bounds__(HV_THREADS) void hv_blur_cols_kernel(const int32_t* __restrict__ tile_cu, const int64_t* __restrict__ bag,
                                                                  int R, int C, int64_t P, Taps taps, int r,
                                                                  const uint64_t* __restrict__ acc, const uint64_t* __restrict__ s1,
                                                                  const uint64_t* __restrict__ n1, const uint8_t* __restrict__ lut,
                                                                  const uint8_t* __restrict__ under, int alpha,
                                                                  uint16_t* __restrict__ level, uint8_t* __restrict__ covered,
                                                                  uint32_t* __restrict__ rgba) {
    Tile t;
    if (!find_tile(tile_cu, bag, R, P, blockIdx.x, t)) return;
    __shared__ uint64_t s_s[HV_SPAN][HV_TILE];
    __shared__ uint64_t s_n[HV_SPAN][HV_TILE];
    const int ch = blockIdx.y, W = t.c.W, H = t.c.H, span = HV_TILE + 2 * r;
    const int64_t base = (int64_t)C * t.c.off + (int64_t)ch * W * H;
    for (int idx = threadIdx.x; idx < span * HV_TILE; idx += HV_THREADS) {
        const int ly = idx / HV_TILE, lx = idx % HV_TILE, gx = t.x0 + lx, gy = t.y0 + ly - r;
        const bool in = gx < W && gy >= 0 && gy < H;
        s_s[ly][lx] = in ? s1[base + (int64_t)gy * W + gx] : 0ull;
        s_n[ly][lx] = in ? n1[base + (int64_t)gy * W + gx] : 0ull;
    }
    __syncthreads();
    const int lx = threadIdx.x % HV_TILE;
#pragma unroll
    for (int j = 0; j < HV_PER; ++j) {
        const int ly = threadIdx.x / HV_TILE + j * (HV_THREADS / HV_TILE);
        const int gx = t.x0 + lx, gy = t.y0 + ly;
        if (gx >= W || gy >= H) continue;
        uint64_t s = 0, n = 0;
        for (int k = 0; k <= 2 * r; ++k) {
            const uint64_t tap = (uint64_t)taps.t[k];
            s += tap * s_s[ly + k][lx];
            n += tap * s_n[ly + k][lx];
        }
        const int64_t at = base + (int64_t)gy * W + gx;
        const bool cov = (acc[at] >> HV_COUNT_SHIFT) != 0ull && n != 0ull;      // n >= centre^2 * N > 0 with taps the host has checked
        const uint32_t m = cov ? (uint32_t)(s / n) : 0u;
        uint32_t R8 = 0, G8 = 0, B8 = 0, A8 = 0;
        if (under) {
            const uint8_t* u = under + 3 * (t.c.off + (int64_t)gy * W + gx);
            R8 = u[0];
            G8 = u[1];
            B8 = u[2];
            A8 = 255;
        }
        if (cov) {
            const uint32_t idx = (m * 255u + 32767u) / 65535u;
            const uint8_t* e = lut + 4 * (idx > 255u ? 255u : idx);
            const uint32_t a = ((uint32_t)e[3] * (uint32_t)alpha + 127u) / 255u;
            if (under) {
                R8 = (e[0] * a + R8 * (255u - a) + 127u) / 255u;
                G8 = (e[1] * a + G8 * (255u - a) + 127u) / 255u;
                B8 = (e[2] * a + B8 * (255u - a) + 127u) / 255u;
            } else {
                R8 = e[0];
                G8 = e[1];
                B8 = e[2];
                A8 = a;
            }
        }
        level[at] = (uint16_t)(m > 65535u ? 65535u : m);
        covered[at] = cov ? 1 : 0;
        rgba[at] = R8 | (G8 << 8) | (B8 << 16) | (A8 << 24);
    }
}


// The refusals of the three sizes the query and the entry point share.
int check_sizes(int64_t P, int64_t R, int C) {
    if (P < 0 || R < 0 || C < 1) return MDL_E_ARG;
    if (!i32(P) || !i32(R) || C > 65535 || !i32((int64_t)C * P)) return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_heat_ws_bytes(int64_t P, int64_t R, int C) {
    if (const int rc = check_sizes(P, R, C)) return rc;
    return carve(nullptr, P, R, C).bytes;
}

#define HV_LAUNCH(kernel, grid, ...)                                                                   \
    do {                                                                                               \
        hipLaunchKernelGGL(kernel, grid, dim3(HV_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);       \
        MDL_LAUNCH_CHECK();                                                                            \
    } while (0)

#define HV_MARK(i)                                                                              \
    do {                                                                                        \
        if (marks) {                                                                            \
            const hipError_t _e = hipEventRecord((hipEvent_t)marks[i], (hipStream_t)stream);    \
            if (_e != hipSuccess) return (int)_e;                                               \
        }                                                                                       \
    } while (0)

// marks: NULL, or MDL_HEAT_MARKS events recorded before the memset, after the tile table, after the accumulation, after the row pass
// and after the column pass.
static int heat_render(const int32_t* xy, const int64_t* cu, const float* values, int64_t ld, int64_t T, int64_t R, int C,
                       const int64_t* bag_host, const int64_t* bag, int64_t P, int ds, const int32_t* taps_host, int r,
                       const uint8_t* lut, const uint8_t* base, int alpha, uint16_t* level, uint8_t* covered, uint8_t* rgba, void* ws,
                       void* const* marks, void* stream) {
    if (((!xy || !values) && T != 0) || !cu || !bag_host || !bag || !taps_host || !lut || !level || !covered || !rgba || !ws) return MDL_E_ARG;
    if (T < 0 || R < 0 || C < 1 || P < 0 || ld < C || ds < 1 || r < 0 || alpha < 0 || alpha > 255) return MDL_E_ARG;
    if (r > HV_MAX_R || T >= HV_MAX_T) return MDL_E_UNSUPPORTED;
    if (const int rc = check_sizes(P, R, C)) return rc;
    Taps taps = {};
    int64_t tap_sum = 0;
    for (int k = 0; k <= 2 * r; ++k) {
        if (taps_host[k] < 0 || taps_host[k] != taps_host[2 * r - k]) return MDL_E_ARG;
        taps.t[k] = taps_host[k];
        tap_sum += taps_host[k];
    }
    if (tap_sum != MDL_HEAT_TAP_SUM || taps_host[r] <= 0) return MDL_E_ARG;
    int64_t n_tiles = 0, widest = 1;
    for (int64_t b = 0; b < R; ++b) {
        Canvas c;
        if (const int rc = canvas_check(bag_host + b * MDL_HEAT_REC, P, c)) return rc;
        n_tiles += (int64_t)tiles_of(c.W) * tiles_of(c.H);
        int64_t fw = (c.ps - 1) / ds + 2;                    // the widest footprint a patch of this bag can have, before clipping
        fw = fw > c.W ? c.W : fw;
        int64_t fh = (c.ps - 1) / ds + 2;
        fh = fh > c.H ? c.H : fh;
        widest = fw * fh > widest ? fw * fh : widest;
    }
    if (!i32(n_tiles)) return MDL_E_UNSUPPORTED;
    if (!host_aligned16(ws) || !aligned_to(cu, 8) || !aligned_to(bag, 8) || !aligned_to(bag_host, 8) || !aligned_to(xy, 4) ||
        !aligned_to(values, 4) || !aligned_to(taps_host, 4) || !aligned_to(rgba, 4) || !aligned_to(level, 2))
        return MDL_E_ALIGN;
    if (R == 0 || P == 0) return MDL_OK;
    int lane_shift = 0;
    while (lane_shift < 6 && (1ll << lane_shift) < widest) ++lane_shift;
    const Ws w = carve(ws, P, R, C);
    HV_MARK(0);
    const hipError_t e = hipMemsetAsync(w.acc, 0, (size_t)C * (size_t)P * 8, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    HV_LAUNCH(hv_plan_kernel, dim3(1), bag, (int)R, P, (int)n_tiles, w.tile_cu);
    HV_MARK(1);
    if (T > 0) {
        const int64_t blocks = ((T << lane_shift) + HV_THREADS - 1) / HV_THREADS;      // T < 2^24, at most 64 lanes a patch: within int32
        HV_LAUNCH(hv_accumulate_kernel, dim3((unsigned)blocks), xy, cu, values, ld, (int)T, (int)R, C, bag, P, ds, lane_shift, w.acc);
    }
    HV_MARK(2);
    if (n_tiles > 0) {
        const dim3 tiles((unsigned)n_tiles, (unsigned)C);
        HV_LAUNCH(hv_blur_rows_kernel, tiles, (const int32_t*)w.tile_cu, bag, (int)R, C, P, taps, r, (const uint64_t*)w.acc, w.s1, w.n1);
        HV_MARK(3);
        HV_LAUNCH(hv_blur_cols_kernel, tiles, (const int32_t*)w.tile_cu, bag, (int)R, C, P, taps, r, (const uint64_t*)w.acc,
                  (const uint64_t*)w.s1, (const uint64_t*)w.n1, lut, base, alpha, level, covered, reinterpret_cast<uint32_t*>(rgba));
    } else {
        HV_MARK(3);
    }
    HV_MARK(4);
    return MDL_OK;
}

extern "C" int mdl_heat_render(const int32_t* xy, const int64_t* cu, const float* values, int64_t ld, int64_t T, int64_t R, int C,
                               const int64_t* bag_host, const int64_t* bag, int64_t P, int ds, const int32_t* taps_host, int r,
                               const uint8_t* lut, const uint8_t* base, int alpha, uint16_t* level, uint8_t* covered, uint8_t* rgba,
                               void* ws, void* stream) {
    return heat_render(xy, cu, values, ld, T, R, C, bag_host, bag, P, ds, taps_host, r, lut, base, alpha, level, covered, rgba, ws, nullptr,
                       stream);
}

extern "C" int mdl_heat_render_marked(const int32_t* xy, const int64_t* cu, const float* values, int64_t ld, int64_t T, int64_t R, int C,
                                      const int64_t* bag_host, const int64_t* bag, int64_t P, int ds, const int32_t* taps_host, int r,
                                      const uint8_t* lut, const uint8_t* base, int alpha, uint16_t* level, uint8_t* covered,
                                      uint8_t* rgba, void* ws, void* const* marks_host, void* stream) {
    if (!marks_host) return MDL_E_ARG;
    for (int i = 0; i < MDL_HEAT_MARKS; ++i)
        if (!marks_host[i]) return MDL_E_ARG;
    return heat_render(xy, cu, values, ld, T, R, C, bag_host, bag, P, ds, taps_host, r, lut, base, alpha, level, covered, rgba, ws, marks_host,
                       stream);
}
