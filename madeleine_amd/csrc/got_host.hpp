// got_host.hpp -- host side shared by the two size classes of GOT (got_resident.hip, got_tiled.hip) and by the C ABI (got.hip): the
// record of a call, the engine table, the one function that refuses a call and the one that runs it.  No kernel and no device function
// lives here.
#pragma once
#include "common.hpp"
#include "got_batch.hpp"

namespace mdl {

static_assert(GOT_MAXP == MDL_GOT_MAX_BATCH, "the batch the kernels take by value is the batch the header publishes");

// ---- the stages of a call: bits, so that a combined backward is checked as the set {begin, finish} before its first launch ----
enum GotStage { GOT_EXTREMA = 0, GOT_FWD, GOT_BWD_BEGIN, GOT_BWD_FINISH, GOT_STAGES };
constexpr int got_bit(GotStage s) { return 1 << s; }

// ---- the record of a call.  GotBatch goes to the resident kernels by value and keeps its layout, so what only the host reads lives
// beside it: the stream, m (the tokens of Q of problem 0: a rectangular call is never batched; Q of a batched problem has n tokens) and
// whether the call came through a _multi entry point.
struct GotCall {
    GotBatch b;
    int m;
    bool multi;
    hipStream_t s;
};
static inline int got_m(const GotCall& c, int p) { return c.multi ? c.b.p[p].n : c.m; }

// ---- the engine table: one row per size class, its limits stated once ----
struct GotEngine {
    int max_n, max_m, max_d;   // tokens of V, of Q, channels
    int max_np;                // problems of a call
    int max_n_batched;         // tokens of a problem of a _multi call
    int64_t (*ws_floats)(int k, int n, int m, int d);
    int (*launch[GOT_STAGES])(const GotCall&, hipStream_t);
    int (*plan)(int k, int n, int m, int cus, int64_t* o);   // mdl_dispatch_plan: what the launchers choose for k cases
};
// The rows are handed out by functions: a table at namespace scope would be emitted into the device code as well.
const GotEngine& got_resident_engine();   // got_resident.hip: m == n, plans in registers (n <= 256) or in the workspace (n <= 512)
const GotEngine& got_tiled_engine();      // got_tiled.hip: many workgroups per case

static inline bool got_sizes_bad(int k, int n, int m, int d) { return k < 0 || n < 0 || m < 0 || d < 1; }
static inline bool got_sizes_over(const GotEngine& e, int n, int m, int d) { return n > e.max_n || m > e.max_m || d > e.max_d; }

// The only place that refuses a GOT call.  Each step runs over all problems before the next one begins:
//   1. MDL_E_ARG: np outside [1, MDL_GOT_MAX_BATCH] (a _multi wrapper passes np = 0 for a NULL array), k, n, m < 0, d < 1, an empty
//      problem of a _multi call   2. MDL_E_UNSUPPORTED: a size beyond the engine's limits   3. MDL_E_ARG: ws, or a pointer a stage
//      cannot do without, is NULL (out | minmax_out | d_out; V, Q, dV, dQ only while the tensor has elements), extrema of an empty
//      problem   4. MDL_E_ALIGN: ws off 16 bytes   5. the empty problem (k, n or m == 0) is MDL_OK with *empty set: the caller zeroes the
//      stages' outputs and launches nothing.
static inline int got_check(const GotEngine& e, int stages, const GotCall& c, bool* empty) {
    const GotBatch& b = c.b;
    *empty = false;
    if (b.np < 1 || b.np > GOT_MAXP) return MDL_E_ARG;
    for (int p = 0; p < b.np; ++p)
        if (got_sizes_bad(b.p[p].k, b.p[p].n, got_m(c, p), b.d) || (c.multi && (b.p[p].k < 1 || b.p[p].n < 1))) return MDL_E_ARG;
    if (b.np > e.max_np) return MDL_E_UNSUPPORTED;
    for (int p = 0; p < b.np; ++p)
        if (got_sizes_over(e, b.p[p].n, got_m(c, p), b.d) || (c.multi && b.p[p].n > e.max_n_batched)) return MDL_E_UNSUPPORTED;
    const bool tokens = stages & (got_bit(GOT_EXTREMA) | got_bit(GOT_FWD) | got_bit(GOT_BWD_FINISH));
    for (int p = 0; p < b.np; ++p) {
        const GotProb& q = b.p[p];
        const int m = got_m(c, p);
        const bool none = q.k == 0 || q.n == 0 || m == 0, hasV = q.k && q.n, hasQ = q.k && m;   // (d >= 1)
        if (!q.ws || ((stages & got_bit(GOT_FWD)) && !q.out) || ((stages & got_bit(GOT_EXTREMA)) && (!q.mm_out || none)) ||
            ((stages & got_bit(GOT_BWD_BEGIN)) && !q.d_out))
            return MDL_E_ARG;
        if (tokens && ((hasV && !q.V) || (hasQ && !q.Q))) return MDL_E_ARG;
        if ((stages & got_bit(GOT_BWD_FINISH)) && ((hasV && !q.dV) || (hasQ && !q.dQ))) return MDL_E_ARG;
        *empty |= none;
    }
    for (int p = 0; p < b.np; ++p)
        if (!host_aligned16(b.p[p].ws)) return MDL_E_ALIGN;
    return MDL_OK;
}

// what a stage of an empty problem leaves: out = (0, 0), d_minmax = 0 where it is given, dV / dQ = 0 where they have elements
static inline int got_zero(GotStage st, const GotCall& c) {
    const GotProb& q = c.b.p[0];   // (a _multi call has no empty problem)
    const size_t bv = (size_t)q.k * q.n * c.b.d * sizeof(float), bq = (size_t)q.k * c.m * c.b.d * sizeof(float);
    hipError_t err = hipSuccess;
    if (st == GOT_FWD) err = hipMemsetAsync(q.out, 0, 2 * sizeof(float), c.s);
    if (st == GOT_BWD_BEGIN && q.d_mm) err = hipMemsetAsync(q.d_mm, 0, 6 * sizeof(float), c.s);
    if (st == GOT_BWD_FINISH && bv) err = hipMemsetAsync(q.dV, 0, bv, c.s);
    if (st == GOT_BWD_FINISH && bq && err == hipSuccess) err = hipMemsetAsync(q.dQ, 0, bq, c.s);
    return (int)err;
}

// A call: every stage of `stages` is checked before the first one runs; then they run in the order of the enum.
static inline int got_run(const GotEngine& e, int stages, const GotCall& c) {
    bool empty;
    if (const int rc = got_check(e, stages, c, &empty)) return rc;
    for (int st = 0; st < GOT_STAGES; ++st)
        if (stages & (1 << st))
            if (const int rc = empty ? got_zero((GotStage)st, c) : e.launch[st](c, c.s)) return rc;
    return MDL_OK;
}

// a *_ws_bytes query: the engine's workspace and 64 bytes of padding, or the refusal of the sizes
static inline int64_t got_ws_bytes(const GotEngine& e, int k, int n, int m, int d) {
    if (got_sizes_bad(k, n, m, d)) return MDL_E_ARG;
    if (got_sizes_over(e, n, m, d)) return MDL_E_UNSUPPORTED;
    return e.ws_floats(k, n, m, d) * 4 + 64;
}

}  // namespace mdl
