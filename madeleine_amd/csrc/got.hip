// got.hip -- C ABI of Graph Optimal Transport (G0-G3, reference madeleine/utils/loss.py:162-302): the 22 entry points of the two size
// classes (resident: got_resident.hip; tiled: got_tiled.hip) and their dispatch plans.  An entry point fills the record of its call and
// hands it to got_run (got_host.hpp) with its engine's row; nothing here refuses a call or launches a kernel.
#include "got_host.hpp"

using namespace mdl;

namespace mdl {
// mdl_dispatch_plan (dispatch_plan.hip): k cases in one launch sequence (the batched entry points: the sum of the problems' k and the
// largest n)
static int got_plan(const GotEngine& e, int64_t k, int n, int m, int d, int cus, int64_t* o) {
    if (k < 1 || n < 1 || m < 1 || d < 1 || k > 0x7fffffff) return MDL_E_ARG;
    if (got_sizes_over(e, n, m, d)) return MDL_E_UNSUPPORTED;
    return e.plan((int)k, n, m, cus, o);
}
int plan_got(int64_t k, int n, int cus, int64_t* o) { return got_plan(got_resident_engine(), k, n, n, 1, cus, o); }
int plan_got_tiled(int64_t k, int n, int m, int d, int64_t* o) { return got_plan(got_tiled_engine(), k, n, m, d, 0, o); }
}  // namespace mdl

namespace {
// ---- one problem: V [k, n, d], Q [k, m, d] ----
struct Sizes {
    int k, n, m, d;
    void *ws, *stream;
};
GotCall one(const Sizes& z) {
    GotCall c{};
    c.b.np = 1;
    c.b.d = z.d;
    c.b.p[0].ws = (float*)z.ws;
    c.b.p[0].k = z.k;
    c.b.p[0].n = z.n;
    c.m = z.m;
    c.s = (hipStream_t)z.stream;
    return c;
}
int fwd(const GotEngine& e, const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in, const Sizes& z) {
    GotCall c = one(z);
    GotProb& p = c.b.p[0];
    p.V = V, p.Q = Q, p.out = out, p.mm_out = minmax_out, p.mm_in = minmax_in;
    return got_run(e, got_bit(GOT_FWD), c);
}
int extrema(const GotEngine& e, const float* V, const float* Q, float* minmax_out, const Sizes& z) {
    GotCall c = one(z);
    GotProb& p = c.b.p[0];
    p.V = V, p.Q = Q, p.mm_out = minmax_out;
    return got_run(e, got_bit(GOT_EXTREMA), c);
}
// begin (d_out, d_minmax), finish (V, Q, dV, dQ, d_minmax_total) or, for the combined backward, both: checked together, run in order
int bwd(const GotEngine& e, int stages, const float* V, const float* Q, const float* d_out, float* d_minmax, float* dV, float* dQ,
               const float* d_minmax_total, const Sizes& z) {
    GotCall c = one(z);
    GotProb& p = c.b.p[0];
    p.V = V, p.Q = Q, p.d_out = d_out, p.d_mm = d_minmax, p.dV = dV, p.dQ = dQ, p.d_mm_total = d_minmax_total;
    return got_run(e, stages, c);
}
constexpr int BEGIN = got_bit(GOT_BWD_BEGIN), FINISH = got_bit(GOT_BWD_FINISH);
}  // namespace

extern "C" int64_t mdl_got_ws_bytes(int k, int n, int d) { return got_ws_bytes(got_resident_engine(), k, n, n, d); }
extern "C" int mdl_got_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in, int k, int n, int d,
                           void* ws, void* stream) {
    return fwd(got_resident_engine(), V, Q, out, minmax_out, minmax_in, {k, n, n, d, ws, stream});
}
extern "C" int mdl_got_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int d, void* ws, void* stream) {
    return extrema(got_resident_engine(), V, Q, minmax_out, {k, n, n, d, ws, stream});
}
extern "C" int mdl_got_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int d, void* ws, void* stream) {
    return bwd(got_resident_engine(), BEGIN, nullptr, nullptr, d_out, d_minmax, nullptr, nullptr, nullptr, {k, n, n, d, ws, stream});
}
extern "C" int mdl_got_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total, int k, int n, int d,
                                  void* ws, void* stream) {
    return bwd(got_resident_engine(), FINISH, V, Q, nullptr, nullptr, dV, dQ, d_minmax_total, {k, n, n, d, ws, stream});
}
extern "C" int mdl_got_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int d, void* ws,
                           void* stream) {
    return bwd(got_resident_engine(), BEGIN | FINISH, V, Q, d_out, nullptr, dV, dQ, nullptr, {k, n, n, d, ws, stream});
}

// The tiled class, rectangular: sizes in the order (k, n, m, d).  The square entry points below are their m = n case.
extern "C" int64_t mdl_got_tiled_rect_ws_bytes(int k, int n, int m, int d) { return got_ws_bytes(got_tiled_engine(), k, n, m, d); }
extern "C" int mdl_got_tiled_rect_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in, int k,
                                      int n, int m, int d, void* ws, void* stream) {
    return fwd(got_tiled_engine(), V, Q, out, minmax_out, minmax_in, {k, n, m, d, ws, stream});
}
extern "C" int mdl_got_tiled_rect_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int m, int d, void* ws,
                                          void* stream) {
    return extrema(got_tiled_engine(), V, Q, minmax_out, {k, n, m, d, ws, stream});
}
extern "C" int mdl_got_tiled_rect_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int m, int d, void* ws, void* stream) {
    return bwd(got_tiled_engine(), BEGIN, nullptr, nullptr, d_out, d_minmax, nullptr, nullptr, nullptr, {k, n, m, d, ws, stream});
}
extern "C" int mdl_got_tiled_rect_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total, int k,
                                             int n, int m, int d, void* ws, void* stream) {
    return bwd(got_tiled_engine(), FINISH, V, Q, nullptr, nullptr, dV, dQ, d_minmax_total, {k, n, m, d, ws, stream});
}
extern "C" int mdl_got_tiled_rect_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int m,
                                      int d, void* ws, void* stream) {
    return bwd(got_tiled_engine(), BEGIN | FINISH, V, Q, d_out, nullptr, dV, dQ, nullptr, {k, n, m, d, ws, stream});
}

extern "C" int64_t mdl_got_tiled_ws_bytes(int k, int n, int d) { return mdl_got_tiled_rect_ws_bytes(k, n, n, d); }
extern "C" int mdl_got_tiled_fwd(const float* V, const float* Q, float* out, float* minmax_out, const float* minmax_in, int k, int n,
                                 int d, void* ws, void* stream) {
    return mdl_got_tiled_rect_fwd(V, Q, out, minmax_out, minmax_in, k, n, n, d, ws, stream);
}
extern "C" int mdl_got_tiled_extrema(const float* V, const float* Q, float* minmax_out, int k, int n, int d, void* ws, void* stream) {
    return mdl_got_tiled_rect_extrema(V, Q, minmax_out, k, n, n, d, ws, stream);
}
extern "C" int mdl_got_tiled_bwd_begin(const float* d_out, float* d_minmax, int k, int n, int d, void* ws, void* stream) {
    return mdl_got_tiled_rect_bwd_begin(d_out, d_minmax, k, n, n, d, ws, stream);
}
extern "C" int mdl_got_tiled_bwd_finish(const float* V, const float* Q, float* dV, float* dQ, const float* d_minmax_total, int k, int n,
                                        int d, void* ws, void* stream) {
    return mdl_got_tiled_rect_bwd_finish(V, Q, dV, dQ, d_minmax_total, k, n, n, d, ws, stream);
}
extern "C" int mdl_got_tiled_bwd(const float* V, const float* Q, const float* d_out, float* dV, float* dQ, int k, int n, int d, void* ws,
                                 void* stream) {
    return mdl_got_tiled_rect_bwd(V, Q, d_out, dV, dQ, k, n, n, d, ws, stream);
}

// ---- several problems in one launch sequence (got_batch.hpp), resident class: arrays of np entries.  An array a stage has no use for
// is NULL here; one it may do without (minmax_in, d_minmax, d_minmax_total) may be NULL in the call.  A NULL array that the stage needs,
// or an np that the arrays cannot be read with, leaves np = 0 in the record, which got_check refuses first.
namespace {
struct Arrays {
    const float* const *V, *const *Q;
    float* const *dV, *const *dQ, *const *out, *const *mm_out;
    const float* const* mm_in;
    const float* const* d_out;
    float* const* d_mm;
    const float* const* d_mm_total;
};
int multi(GotStage st, int np, const Arrays& a, const int* k, const int* n, int d, void* const* ws, void* stream) {
    GotCall c{};
    c.b.d = d;
    c.multi = true;
    c.s = (hipStream_t)stream;
    const bool tokens = st != GOT_BWD_BEGIN, finish = st == GOT_BWD_FINISH;
    const bool arrays = k && n && ws && (!tokens || (a.V && a.Q)) && (!finish || (a.dV && a.dQ)) && (st != GOT_FWD || a.out) &&
                        (st != GOT_EXTREMA || a.mm_out) && (st != GOT_BWD_BEGIN || a.d_out);
    c.b.np = arrays && np >= 1 && np <= GOT_MAXP ? np : 0;
    for (int p = 0; p < c.b.np; ++p) {
        auto at = [p](auto* arr) { return arr ? arr[p] : nullptr; };
        c.b.p[p] = GotProb{(float*)ws[p], at(a.V), at(a.Q), at(a.dV), at(a.dQ), at(a.out), at(a.mm_out), at(a.mm_in), at(a.d_out),
                           at(a.d_mm), at(a.d_mm_total), k[p], n[p]};
    }
    return got_run(got_resident_engine(), got_bit(st), c);
}
}  // namespace

extern "C" int mdl_got_extrema_multi(int np, const float* const* V, const float* const* Q, float* const* minmax_out, const int* k,
                                     const int* n, int d, void* const* ws, void* stream) {
    return multi(GOT_EXTREMA, np, {V, Q, nullptr, nullptr, nullptr, minmax_out}, k, n, d, ws, stream);
}
extern "C" int mdl_got_fwd_multi(int np, const float* const* V, const float* const* Q, float* const* out, const float* const* minmax_in,
                                 const int* k, const int* n, int d, void* const* ws, void* stream) {
    return multi(GOT_FWD, np, {V, Q, nullptr, nullptr, out, nullptr, minmax_in}, k, n, d, ws, stream);
}
extern "C" int mdl_got_bwd_begin_multi(int np, const float* const* d_out, float* const* d_minmax, const int* k, const int* n, int d,
                                       void* const* ws, void* stream) {
    return multi(GOT_BWD_BEGIN, np, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_out, d_minmax}, k, n, d, ws, stream);
}
extern "C" int mdl_got_bwd_finish_multi(int np, const float* const* V, const float* const* Q, float* const* dV, float* const* dQ,
                                        const float* const* d_minmax_total, const int* k, const int* n, int d, void* const* ws,
                                        void* stream) {
    return multi(GOT_BWD_FINISH, np, {V, Q, dV, dQ, nullptr, nullptr, nullptr, nullptr, nullptr, d_minmax_total}, k, n, d, ws, stream);
}
