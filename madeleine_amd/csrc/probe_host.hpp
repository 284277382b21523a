// probe_host.hpp -- host side shared by the entry points that take a problem table (probe.hip, probe_primal.hip, survival.hip,
// resample.hip, ridge.hip): the record of the table, the limits of an entry point and the one function that refuses a call.  No kernel and no
// device function lives here.
#pragma once
#include <type_traits>

#include "probe_common.hpp"

namespace mdl {

// ---- the record: train_idx [P, n_max] and n_train [P] over S cases, with up to two per-case columns of row stride 0 (shared by all
// problems) or >= S (y; time and event), the class count and the width of X
struct ProbeColumn {
    const void* ptr;
    int64_t ld;
};
struct ProbeTable {
    const int32_t* train_idx;
    const int32_t* n_train;
    int64_t P;
    int n_max;
    int64_t S;
    ProbeColumn col[2];   // an unused column: {nullptr, 0}
    int ncol;
    int C;                // 0 where there are no classes
    int d;                // 0 where there is no X
    int64_t T = 1;        // target columns of a shared Y [S, T] (the regression probe), 1 elsewhere
    int A = 1;            // penalties per problem (the regression probe), 1 elsewhere
};
// the sizes alone, for a *_ws_bytes query (a size the query does not take: 1)
inline ProbeTable probe_sizes(int64_t P, int n_max, int64_t S, int C, int d) { return {nullptr, nullptr, P, n_max, S, {}, 0, C, d}; }

// ---- the limits of an entry point, stated once: its launcher and its *_ws_bytes query read the same row
constexpr int PROBE_NO_LIMIT = 0x7FFFFFFF;   // what an int32 holds: every S and d are held to it
struct ProbeLimits {
    int n_max;      // MDL_PROBE_MAX_TRAIN, MDL_LOGIT_MAX_TRAIN or MDL_COX_MAX_TRAIN
    int d;          // MDL_LOGIT_MAX_DIM or none
    int S;          // MDL_PROBE_MAX_CASES, MDL_BOOT_SURV_MAX_TEST or none
    bool fit;       // takes X [S, d]: d >= 1
    bool classes;   // takes C in 2 .. MDL_PROBE_MAX_CLASSES
    int sys = PROBE_NO_LIMIT;   // MDL_RIDGE_MAX_SYS: the order min(n_max, d) of a direct solve, or none
    int T = PROBE_NO_LIMIT;     // MDL_RIDGE_MAX_TARGETS or none
    int A = PROBE_NO_LIMIT;     // MDL_RIDGE_MAX_ALPHAS or none
    bool table = true;          // takes train_idx and n_train (false: a scoring call over P lists, n_max = 1)
};

// ---- what an entry point adds to its table.  The caller states facts; probe_check alone decides what is refused and in which order.
struct ProbeExtra {
    bool pointers;       // every pointer the entry point needs besides the table's is there
    bool grids;          // every launch grid and element count beyond the table's is within int32 (mul_i32)
    bool aligned;        // ws to 16 bytes and the 8 / 4 / 2-byte alignments the header states
    int64_t R = 0;       // bootstrap replicates
    int64_t ldX = 0;     // row stride of X and the solver's arguments (fit entry points)
    int max_iter = 0;
    float cost = 0.f, gtol = 0.f;
    bool values = true;  // every further argument the entry point states is in its range (ldY >= T, each alpha finite and > 0)
};

// a * b * c within int32, with every factor within int32 (so no 64-bit product can overflow on the way)
inline bool mul_i32(int64_t a, int64_t b = 1, int64_t c = 1) { return i32(a) && i32(b) && i32(a * b) && i32(c) && i32(a * b * c); }
inline int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }      // no a + b - 1 that could overflow
inline int64_t gram_ld(int64_t n_max) { return ceil_div(n_max, GRAM_TILE) * GRAM_TILE; }      // leading dimension of a problem's Gram matrix
template <class... Ptr>
inline bool all_given(const Ptr*... p) { return ((p != nullptr) && ...); }
template <class... Ptr>
inline bool all_aligned(uintptr_t bytes, const Ptr*... p) { return (aligned_to(p, bytes) && ...); }

// The only place that refuses a call of this family, before any launch and before a device pointer is touched:
//   1. MDL_E_ARG: a NULL pointer; P, n_max or S < 1; d < 1 or ldX < d; max_iter < 0, cost not > 0, gtol not >= 0; R < 0; a column
//      stride neither 0 nor >= S; T or A < 1, or a further argument outside the range its entry point states
//   2. MDL_E_UNSUPPORTED: n_max, d, S, min(n_max, d), T or A beyond the entry point's row of limits, C outside
//      2 .. MDL_PROBE_MAX_CLASSES; R + 1 beyond int32;
//      S, P, P * n_max or one of the entry point's grids and element counts beyond int32
//   3. MDL_E_ALIGN.
// extra == nullptr is a *_ws_bytes query: the sizes it takes, the row of limits and P within int32.
inline int probe_check(const ProbeTable& t, const ProbeLimits& lim, const ProbeExtra* extra) {
    if (extra && ((lim.table && (!t.train_idx || !t.n_train)) || !extra->pointers)) return MDL_E_ARG;
    if (t.P < 1 || t.n_max < 1 || t.S < 1 || (lim.fit && t.d < 1) || t.T < 1 || t.A < 1) return MDL_E_ARG;
    if (extra) {
        if (!extra->values) return MDL_E_ARG;
        if (lim.fit && (extra->ldX < t.d || extra->max_iter < 0 || !(extra->cost > 0.f) || !(extra->gtol >= 0.f))) return MDL_E_ARG;
        if (extra->R < 0) return MDL_E_ARG;
        for (int c = 0; c < t.ncol; ++c)
            if (!t.col[c].ptr || (t.col[c].ld != 0 && t.col[c].ld < t.S)) return MDL_E_ARG;
    }
    if (t.n_max > lim.n_max || t.d > lim.d || t.S > lim.S || !i32(t.P)) return MDL_E_UNSUPPORTED;
    if ((t.n_max < t.d ? t.n_max : t.d) > lim.sys || t.T > lim.T || t.A > lim.A) return MDL_E_UNSUPPORTED;
    if (lim.classes && (t.C < 2 || t.C > PROBE_CMAX)) return MDL_E_UNSUPPORTED;
    if (!extra) return MDL_OK;
    if (extra->R > 0x7FFFFFFE || !mul_i32(t.P, t.n_max) || !extra->grids) return MDL_E_UNSUPPORTED;
    return extra->aligned ? MDL_OK : MDL_E_ALIGN;
}

// the kernel template built for `cols` decision values per case: f(std::integral_constant<int, NC>) with NC = nc_of(cols)
template <class F>
inline int for_nc(int cols, F f) {
    if (cols == 1) return f(std::integral_constant<int, 1>());
    if (cols <= 4) return f(std::integral_constant<int, 4>());
    return f(std::integral_constant<int, 8>());
}

}  // namespace mdl
