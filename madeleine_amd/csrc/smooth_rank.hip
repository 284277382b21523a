// smooth_rank.hip -- R1: exp(entropy of the normalised singular values) of an embedding matrix, entirely on the device
// (include/madeleine_amd.h, R1).  E [n, d] fp32 -> the k = min(n, d) singular values in fp64 and exp(H), H.
//
//   1. Gram matrix in fp64, G = E^T E (n >= d) or E E^T (n < d): fp32 inputs widened first, so every product is exact (48 bits) and
//      only the additions round.  The contraction is cut into row chunks; a workgroup forms one 64 x 64 tile of one chunk's partial
//      Gram and a second kernel adds the partials in chunk order.  Only tiles on or below the diagonal are formed; the combine writes
//      both halves, so G is symmetric bit for bit.
//   2. Householder reduction to tridiagonal form, k - 2 steps of two launches (matrix-vector product, symmetric rank-2 update) over
//      blocks of SR_TRI_ROWS rows of the trailing block.  Every workgroup rebuilds the step's reflector, and the update also p^T v,
//      from the k numbers involved: nothing is exchanged inside a launch.  The update keeps the matrix symmetric bit for bit.
//   3. All k eigenvalues of the tridiagonal matrix by Sturm-count bisection from the Gershgorin interval: one thread per eigenvalue,
//      64 halvings, dstebz's pivot floor.
//   4. One workgroup: sigma = sqrt(max(lambda, 0)) descending, p = sigma / sum(sigma) + eps, H = -sum p ln p.
//
// 2 + 2 (k - 2) + 2 launches for k >= 2, 4 for k == 1: a function of (n, d) alone.  No atomics, no host read, no workgroup waits
// on another, and every loop's trip count is a function of (n, d), so a NaN cannot hang a kernel.
#include <float.h>

#include "common.hpp"

namespace mdl {
namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_TILE = MDL_RANK_GRAM_TILE;       // 64 x 64 outputs per workgroup, 4 x 4 per thread
constexpr int SR_KSTEP = 16;                      // contraction rows staged in LDS per step
constexpr int SR_TRI_ROWS = MDL_RANK_TRI_ROWS;    // rows of the trailing block per workgroup: 4 waves x 4 rows
constexpr int SR_BISECT_THREADS = 64;
constexpr int SR_HALVINGS = 64;
static_assert(SR_TILE == 64 && SR_THREADS == 256 && SR_TRI_ROWS == 16, "the thread maps below are written for these");
static_assert(MDL_RANK_GRAM_ROWS % SR_KSTEP == 0, "a chunk is a whole number of LDS stages");

// The contraction (length L = max(n, d)) in C equal chunks of `rows` rows, rows a multiple of SR_KSTEP: chunks of MDL_RANK_GRAM_ROWS
// until there would be more than MDL_RANK_GRAM_MAX_CHUNKS of them, then that many longer ones.  A function of L alone.
struct Chunks {
    int64_t rows;
    int count;
};
inline Chunks chunks_of(int64_t L) {
    int64_t c = (L + MDL_RANK_GRAM_ROWS - 1) / MDL_RANK_GRAM_ROWS;
    if (c <= MDL_RANK_GRAM_MAX_CHUNKS) return Chunks{MDL_RANK_GRAM_ROWS, (int)c};
    int64_t rows = (L + MDL_RANK_GRAM_MAX_CHUNKS - 1) / MDL_RANK_GRAM_MAX_CHUNKS;
    rows = (rows + SR_KSTEP - 1) / SR_KSTEP * SR_KSTEP;
    return Chunks{rows, (int)((L + rows - 1) / rows)};
}

struct Ws {
    double* G;        // [k, k]  the Gram matrix, tridiagonalised in place
    double* part;     // [chunks, k, k]
    double* p;        // [k]     the step's matrix-vector product
    double* diag;     // [k]     diagonal of the tridiagonal matrix (entries 0 .. k-3; the last two stay in G)
    double* off;      // [k]     its off-diagonal: off[j] couples j and j + 1
    double* lam;      // [k]     eigenvalues, ascending
    int64_t bytes;
};
inline Ws carve(void* ws, int64_t L, int k) {
    const int64_t kk = (int64_t)k * k, vec = ((int64_t)k + 1) / 2 * 2;      // vectors keep 16-byte alignment
    double* base = (double*)ws;
    Ws w;
    w.G = base;
    w.part = w.G + kk;
    w.p = w.part + kk * chunks_of(L).count;
    w.diag = w.p + vec;
    w.off = w.diag + vec;
    w.lam = w.off + vec;
    w.bytes = (int64_t)sizeof(double) * ((w.lam + vec) - base);
    return w;
}

// ---- sums in a fixed order: lane partials by xor butterflies, the waves of the workgroup in wave order ---------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Every thread of the workgroup gets the total.  `red` holds one double per wave; the trailing barrier lets it be reused at once.
template <int THREADS>
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// ---- 1. Gram ------------------------------------------------------------------------------------------------------------------
// X(r, i), r in [0, L) the contraction index, i in [0, k): E[r, i] when TR == false (G = E^T E), E[i, r] when TR == true (G = E E^T).
// blockIdx.x enumerates the tile pairs (ti >= tj) row by row, blockIdx.y the chunk.
template <bool TR>
__global__ __launch_bounds__(SR_THREADS) void sr_gram_kernel(const float* __restrict__ E, int64_t ldE, int64_t L, int k, int64_t chunk_rows,
                                                             double* __restrict__ part) {
    __shared__ double As[SR_KSTEP][SR_TILE + 1], Bs[SR_KSTEP][SR_TILE + 1];
    int ti = 0, rest = (int)blockIdx.x;
    while (rest > ti) {      // at most k / SR_TILE = 16 rounds
        rest -= ti + 1;
        ++ti;
    }
    const int tj = rest, t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows, r1 = (r0 + chunk_rows < L) ? r0 + chunk_rows : L;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

    for (int64_t s0 = r0; s0 < r1; s0 += SR_KSTEP) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // lanes run along the unit-stride direction of E: the columns i when TR == false, the contraction index r when TR == true
            const int rr = TR ? (t & 15) : (t >> 6) + 4 * q, ii = TR ? (t >> 4) + 16 * q : (t & 63);
            const int64_t r = s0 + rr;
            const int ia = ti * SR_TILE + ii, ib = tj * SR_TILE + ii;
            float va = 0.f, vb = 0.f;
            if (r < r1) {
                if (ia < k) va = TR ? E[(int64_t)ia * ldE + r] : E[r * ldE + ia];
                if (ib < k) vb = TR ? E[(int64_t)ib * ldE + r] : E[r * ldE + ib];
            }
            As[rr][ii] = (double)va;
            Bs[rr][ii] = (double)vb;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SR_KSTEP; ++s) {
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = As[s][ty + 16 * q];
                b[q] = Bs[s][tx + 16 * q];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);      // the product is exact: one rounding, of the sum
        }
        __syncthreads();
    }
    double* out = part + (int64_t)blockIdx.y * k * k;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int i = ti * SR_TILE + ty + 16 * x;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int j = tj * SR_TILE + tx + 16 * y;
            if (i < k && j < k) out[(int64_t)i * k + j] = acc[x][y];
        }
    }
}

// G[i, j] = the chunk partials added in chunk order, for the tiles on or below the diagonal; tiles below it are mirrored.
__global__ __launch_bounds__(SR_THREADS) void sr_gram_combine_kernel(const double* __restrict__ part, int k, int chunks, double* __restrict__ G) {
    const int64_t kk = (int64_t)k * k, g = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x;
    if (g >= kk) return;
    const int i = (int)(g / k), j = (int)(g % k);
    if (i / SR_TILE < j / SR_TILE) return;
    double s = part[g];
    for (int c = 1; c < chunks; ++c) s += part[c * kk + g];
    G[g] = s;
    if (i / SR_TILE != j / SR_TILE) G[(int64_t)j * k + i] = s;
}

// ---- 2. tridiagonalisation ------------------------------------------------------------------------------------------------------
// The reflector of step j, from row j of the (symmetric) matrix: x = A[j, j+1 .. k-1], m = k - 1 - j numbers.
//   H = I - beta v v^T,  H x = alpha e_1,  alpha = -sign(x_0) |x|,  v = x - alpha e_1,  beta = 2 / v^T v.
// x already a multiple of e_1: beta = 0, alpha = x_0 (the step leaves the matrix as it is, with the same launches).
// On return v[0 .. m) holds v.  Every workgroup of both launches of the step calls this on the same numbers and gets the same bits.
struct Reflector {
    double alpha, beta;
};
__device__ __forceinline__ Reflector reflector(const double* __restrict__ A, int k, int j, double* v, double* red) {
    const int m = k - 1 - j, t = (int)threadIdx.x;
    const double* x = A + (int64_t)j * k + j + 1;
    double tail = 0.0;
    for (int l = t; l < m; l += SR_THREADS) {
        const double xl = x[l];
        v[l] = xl;
        if (l > 0) tail = fma(xl, xl, tail);
    }
    __syncthreads();
    tail = block_sum_f64<SR_THREADS>(tail, red);
    const double x0 = v[0];
    Reflector h{x0, 0.0};
    double v0 = x0;
    if (!(tail == 0.0)) {                                // a NaN comes here and stays one
        const double norm = sqrt(fma(x0, x0, tail));
        h.alpha = x0 > 0.0 ? -norm : norm;
        v0 = x0 - h.alpha;
        h.beta = 2.0 / fma(v0, v0, tail);
    }
    __syncthreads();                                     // everyone has read x0
    if (t == 0) v[0] = v0;
    __syncthreads();
    return h;
}

// p = beta A22 v over the trailing block A22 = A[j+1 .., j+1 ..].  A workgroup takes SR_TRI_ROWS rows, a wave four of them; a row's
// sum is 64 lane partials (columns lane, lane + 64, ..) added by the butterfly.
__global__ __launch_bounds__(SR_THREADS) void sr_tri_matvec_kernel(const double* __restrict__ A, int k, int j, double* __restrict__ p,
                                                                   double* __restrict__ diag, double* __restrict__ off) {
    __shared__ double v[MDL_RANK_MAX_K], red[SR_THREADS / 64];
    const int m = k - 1 - j, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const Reflector h = reflector(A, k, j, v, red);
    if (blockIdx.x == 0 && t == 0) {
        diag[j] = A[(int64_t)j * k + j];
        off[j] = h.alpha;
    }
    const double* A22 = A + (int64_t)(j + 1) * k + (j + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = (int)blockIdx.x * SR_TRI_ROWS + wave * 4 + q;      // uniform in the wave
        if (i >= m) continue;
        const double* row = A22 + (int64_t)i * k;
        double s = 0.0;
        for (int l = lane; l < m; l += 64) s = fma(row[l], v[l], s);
        s = wave_sum_f64(s);
        if (lane == 0) p[i] = h.beta * s;
    }
}

// A22 <- A22 - v w^T - w v^T,  w = p - (beta / 2)(p^T v) v.  Entry (i, l) subtracts round(v_i w_l) + round(w_i v_l): products and
// sum are rounded separately (no FMA contraction), so entries (i, l) and (l, i) get the same bits and the matrix stays symmetric.
__global__ __launch_bounds__(SR_THREADS) void sr_tri_update_kernel(double* __restrict__ A, int k, int j, const double* __restrict__ p) {
    __shared__ double v[MDL_RANK_MAX_K], w[MDL_RANK_MAX_K], red[SR_THREADS / 64];
    const int m = k - 1 - j, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const Reflector h = reflector(A, k, j, v, red);
    double pv = 0.0;
    for (int l = t; l < m; l += SR_THREADS) {
        const double pl = p[l];
        w[l] = pl;
        pv = fma(pl, v[l], pv);
    }
    pv = block_sum_f64<SR_THREADS>(pv, red);             // its first barrier also publishes w
    const double K = 0.5 * h.beta * pv;
    for (int l = t; l < m; l += SR_THREADS) w[l] = fma(-K, v[l], w[l]);      // thread t's own entries
    __syncthreads();
    double* A22 = A + (int64_t)(j + 1) * k + (j + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = (int)blockIdx.x * SR_TRI_ROWS + wave * 4 + q;
        if (i >= m) continue;
        double* row = A22 + (int64_t)i * k;
        const double vi = v[i], wi = w[i];
        for (int l = lane; l < m; l += 64) row[l] = __dsub_rn(row[l], __dadd_rn(__dmul_rn(vi, w[l]), __dmul_rn(wi, v[l])));
    }
}

// ---- 3. bisection -------------------------------------------------------------------------------------------------------------
// The tridiagonal matrix: diag / off hold entries 0 .. k-3 (written by the matvec launches), the last 2 x 2 block is still in A.
__device__ __forceinline__ double tri_diag(const double* A, const double* diag, int k, int i) {
    return i < k - 2 ? diag[i] : A[(int64_t)i * k + i];
}
__device__ __forceinline__ double tri_off(const double* A, const double* off, int k, int i) {      // i in [0, k - 1)
    return i < k - 2 ? off[i] : A[(int64_t)(i + 1) * k + i];
}

// Thread g finds eigenvalue g (ascending): the least x with at least g + 1 eigenvalues below it, by SR_HALVINGS halvings of the
// widened Gershgorin interval.  count(x) = negative pivots of the LDL^T of T - x, a pivot inside (-pivmin, pivmin) taken as -pivmin
// (dstebz / dlaebz).  Two threads follow the same midpoints until their decisions differ, and the lower index always takes the lower
// half first: lam is ascending whatever count() rounds to.  A non-finite entry gives NaN; an all-zero matrix gives exact zeros (so
// that the finish divides 0 by 0 as the reference does).
__global__ __launch_bounds__(SR_BISECT_THREADS) void sr_bisect_kernel(const double* __restrict__ A, const double* __restrict__ diag,
                                                                      const double* __restrict__ off, int k, double* __restrict__ lam) {
    __shared__ double d[MDL_RANK_MAX_K], e2[MDL_RANK_MAX_K];
    const int t = (int)threadIdx.x, g = (int)blockIdx.x * SR_BISECT_THREADS + t;
    for (int i = t; i < k; i += SR_BISECT_THREADS) {
        d[i] = tri_diag(A, diag, k, i);
        const double e = i < k - 1 ? tri_off(A, off, k, i) : 0.0;
        e2[i] = e * e;                                   // e2[i] couples i and i + 1; e2[k - 1] = 0
    }
    __syncthreads();
    double gl = d[0], gu = d[0], emax2 = 0.0, prev = 0.0;
    bool bad = false;
    for (int i = 0; i < k; ++i) {
        const double here = sqrt(e2[i]), r = prev + here;
        bad = bad || !(fabs(d[i]) <= DBL_MAX) || !(e2[i] <= DBL_MAX);
        gl = fmin(gl, d[i] - r);
        gu = fmax(gu, d[i] + r);
        emax2 = fmax(emax2, e2[i]);
        prev = here;
    }
    if (g >= k) return;
    if (bad) {
        lam[g] = __builtin_nan("");
        return;
    }
    if (gl == 0.0 && gu == 0.0) {
        lam[g] = 0.0;
        return;
    }
    const double pivmin = DBL_MIN * fmax(1.0, emax2), tnorm = fmax(fabs(gl), fabs(gu));
    const double widen = 2.1 * tnorm * DBL_EPSILON * k + 4.2 * pivmin;
    double lo = gl - widen, hi = gu + widen;
    for (int it = 0; it < SR_HALVINGS; ++it) {
        const double x = 0.5 * (lo + hi);
        double q = d[0] - x;
        if (fabs(q) < pivmin) q = -pivmin;
        int count = q < 0.0;
        for (int i = 1; i < k; ++i) {
            q = d[i] - x - e2[i - 1] / q;
            if (fabs(q) < pivmin) q = -pivmin;
            count += q < 0.0;
        }
        if (count >= g + 1) hi = x;
        else lo = x;
    }
    lam[g] = 0.5 * (lo + hi);
}

// ---- 4. finish ----------------------------------------------------------------------------------------------------------------
// One workgroup.  sigma descending; s and H are sums of per-thread partials (entries t, t + 256, ..) in the fixed order of block_sum.
__global__ __launch_bounds__(SR_THREADS) void sr_finish_kernel(const double* __restrict__ lam, int k, double eps, double* __restrict__ sigma,
                                                               double* __restrict__ out) {
    __shared__ double sg[MDL_RANK_MAX_K], red[SR_THREADS / 64];
    const int t = (int)threadIdx.x;
    double s = 0.0;
    for (int i = t; i < k; i += SR_THREADS) {
        const double l = lam[k - 1 - i], v = sqrt(l > 0.0 ? l : (l == l ? 0.0 : l));      // max(l, 0) that keeps a NaN
        sg[i] = v;
        sigma[i] = v;
        s += v;
    }
    s = block_sum_f64<SR_THREADS>(s, red);
    double h = 0.0;
    for (int i = t; i < k; i += SR_THREADS) {
        const double p = sg[i] / s + eps;
        h -= p * log(p);
    }
    h = block_sum_f64<SR_THREADS>(h, red);
    if (t == 0) {
        out[0] = exp(h);
        out[1] = h;
    }
}


int check_sizes(int64_t n, int64_t d) {
    if (n < 1 || d < 1) return MDL_E_ARG;
    if ((n < d ? n : d) > MDL_RANK_MAX_K) return MDL_E_UNSUPPORTED;
    if (n > 0x7fffffffLL || d > 0x7fffffffLL) return MDL_E_UNSUPPORTED;
    return MDL_OK;
}

#define SR_LAUNCH(kernel, grid, block, ...)                                                     \
    do {                                                                                        \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);     \
        MDL_LAUNCH_CHECK();                                                                     \
    } while (0)
#define SR_MARK(i)                                                                              \
    do {                                                                                        \
        if (marks) {                                                                            \
            const hipError_t _e = hipEventRecord((hipEvent_t)marks[i], (hipStream_t)stream);    \
            if (_e != hipSuccess) return (int)_e;                                               \
        }                                                                                       \
    } while (0)

// marks: NULL, or four events recorded before the Gram, after it, after the tridiagonalisation and after the finish.
int smooth_rank(const float* E, int64_t ldE, int64_t n, int64_t d, uint64_t eps_bits, void* sigma, void* out, void* ws, void* const* marks,
                void* stream) {
    if (n < 1 || d < 1 || ldE < d || !E || !sigma || !out || !ws) return MDL_E_ARG;
    if (!aligned_to(E, 4) || !aligned_to(sigma, 8) || !aligned_to(out, 8) || !host_aligned16(ws)) return MDL_E_ALIGN;
    if (const int rc = check_sizes(n, d)) return rc;
    // every offset into E is formed in 64 bits, and (rows - 1) * ldE + d has to stay inside them
    if (ldE > (0x7fffffffffffffffLL / 4 - d) / n) return MDL_E_UNSUPPORTED;
    const bool tr = n < d;
    const int k = (int)(tr ? n : d);
    const int64_t L = tr ? d : n;
    const Chunks ch = chunks_of(L);
    const Ws w = carve(ws, L, k);
    double eps;
    __builtin_memcpy(&eps, &eps_bits, sizeof eps);
    const int nt = (k + SR_TILE - 1) / SR_TILE;
    const dim3 gram((unsigned)(nt * (nt + 1) / 2), (unsigned)ch.count);
    const unsigned cells = (unsigned)(((int64_t)k * k + SR_THREADS - 1) / SR_THREADS);

    SR_MARK(0);
    if (tr) SR_LAUNCH(sr_gram_kernel<true>, gram, SR_THREADS, E, ldE, L, k, ch.rows, w.part);
    else SR_LAUNCH(sr_gram_kernel<false>, gram, SR_THREADS, E, ldE, L, k, ch.rows, w.part);
    SR_LAUNCH(sr_gram_combine_kernel, dim3(cells), SR_THREADS, (const double*)w.part, k, ch.count, w.G);
    SR_MARK(1);
    for (int j = 0; j + 2 < k; ++j) {
        const dim3 blocks((unsigned)((k - 1 - j + SR_TRI_ROWS - 1) / SR_TRI_ROWS));
        SR_LAUNCH(sr_tri_matvec_kernel, blocks, SR_THREADS, (const double*)w.G, k, j, w.p, w.diag, w.off);
        SR_LAUNCH(sr_tri_update_kernel, blocks, SR_THREADS, w.G, k, j, (const double*)w.p);
    }
    SR_MARK(2);
    SR_LAUNCH(sr_bisect_kernel, dim3((unsigned)((k + SR_BISECT_THREADS - 1) / SR_BISECT_THREADS)), SR_BISECT_THREADS, (const double*)w.G,
              (const double*)w.diag, (const double*)w.off, k, w.lam);
    SR_LAUNCH(sr_finish_kernel, dim3(1), SR_THREADS, (const double*)w.lam, k, eps, (double*)sigma, (double*)out);
    SR_MARK(3);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_smooth_rank_ws_bytes(int64_t n, int64_t d) {
    if (const int rc = check_sizes(n, d)) return rc;
    return carve(nullptr, n < d ? d : n, (int)(n < d ? n : d)).bytes;
}

extern "C" int mdl_smooth_rank(const float* E, int64_t ldE, int64_t n, int64_t d, uint64_t eps_bits, void* sigma, void* out, void* ws,
                               void* stream) {
    return smooth_rank(E, ldE, n, d, eps_bits, sigma, out, ws, nullptr, stream);
}

extern "C" int mdl_smooth_rank_marked(const float* E, int64_t ldE, int64_t n, int64_t d, uint64_t eps_bits, void* sigma, void* out,
                                      void* ws, void* const* marks_host, void* stream) {
    if (!marks_host || !marks_host[0] || !marks_host[1] || !marks_host[2] || !marks_host[3]) return MDL_E_ARG;
    return smooth_rank(E, ldE, n, d, eps_bits, sigma, out, ws, marks_host, stream);
}
