// gate_host.hpp -- host side shared by the three gated-attention engines (abmil_gate.hip fp32, abmil_gate_bf16.hip, abmil_gate_split.hip):
// the argument records the extern "C" wrappers fill, the engine table, the two functions that refuse a call, the run-time -> compile-time
// dispatch, the workspace layouts, the grids and the phase structure of the backward.  No kernel and no device function lives here.
#pragma once
#include <type_traits>
#include "gate_common.hpp"

namespace mdl {

// launchers of the reduction / finalize kernels defined in abmil_gate.hip (shared by the three engines)
int gate_launch_finalize(const float* part, const float* bc, float* scores, int64_t n, int H, hipStream_t s);
int gate_launch_reduce_w(const float* slabW, float* dWa, float* dWb, int H, int S, hipStream_t s);
int gate_launch_reduce_v(const float* slabV, float* dba, float* dbb, float* dwc, float* dbc, int H, int S, hipStream_t s);

// ---- the records of a call ----
struct GateParams { const float *Wa, *ba, *Wb, *bb, *wc, *bc; };   // [H,512,512] Wa, Wb; [H,512] ba, bb, wc; [H] bc.  A backward reads Wa, Wb, wc
struct GateSrc { const void* p; int64_t ld; const float* scale; };  // E: a tensor (ld in elements), or a split image (ld in bytes, scale)
template <class V>                  // the saved activations [T,H,512] in E's element type (fp32 on the split engine).  V = void: a forward
struct GateActs { V *a, *b; };      // writes them (both or neither); const void: a backward reads them
struct GateDrop { float p; uint64_t seed; const uint8_t *keep_a, *keep_b; };   // keep_*: explicit masks (both or neither), else the counter hash
struct GateGrads { float *dWa, *dWb, *dba, *dbb, *dwc, *dbc; };              // dbc may be NULL
struct GateDE { void* p; int64_t ld; int accumulate; float* absmax; };        // ld in elements; absmax (split, may be NULL): raised to max |dE|
struct GateProblem { int64_t T; int H, phases, terms; };                      // phases, terms: backward only
struct GateFwdCall {
    GateSrc src; GateParams par; float* scores; GateActs<void> act; GateDrop drop; GateProblem pb; void* ws; hipStream_t s;
};
struct GateBwdCall {
    GateSrc src; GateParams par; GateActs<const void> act; const float* d_scores; GateDE de; GateGrads g; GateDrop drop; PoolTerm pt;
    bool pool;   // the entry point cannot do without the pooling term (on the split engine pt.scores decides)
    GateProblem pb; void* ws; hipStream_t s;
};

// ---- the engine table: what differs between the engines in how a call is refused ----
struct StrideFit {   // stride_fits32(stride, elem_bytes, rows, col_bytes) of the kernel expression that is narrowest
    int64_t rows, col_bytes;
};
struct GateEngine {
    bool image;        // E is a split image: src.scale is required, dE has a stride of its own (fp32 elements)
    int elem_bytes;    // of a unit of E's stride (an image's stride counts bytes)
    int stride_unit;   // E's stride is a multiple of this many units = 16 bytes, the LDS-DMA granule
    int head_units;    // stride units of one head's 512 channels
    StrideFit fwd, bwd;
    int max_phases;    // 3: bit 0 dz pass, bit 1 both contractions; 15: also bit 2 dX alone, bit 3 dW alone
    int64_t (*fwd_max_grid)(int64_t T, int H);               // the widest launch of a forward
    int64_t (*bwd_max_grid)(int64_t T, int H, int phases);   // ... of the phases of a backward
};
// Addressed in 16-byte units by every engine (NULL counts as aligned).  Forward: E (LDS-DMA), Wa, Wb (the weight-image kernels), wc and
// act_a / act_b (vector load / stores of the forward epilogue), ws.  Backward: E, dE (the dX epilogue's vector store), Wa, Wb, act_a, act_b
// and wc (the dz pass), ws.
template <class... P>
static inline bool gate_aligned16(const P*... p) { return (host_aligned16(p) && ...); }
static inline bool gate_heads_ok(int H) { return H == 1 || H == 2 || H == 4 || H == 8; }   // xcd_head: 8 / H shares per head

static inline bool gate_ranges_ok(const GateEngine& e, const GateSrc& src, const GateProblem& pb, const GateDrop& d) {
    return (d.keep_a == nullptr) == (d.keep_b == nullptr) && pb.T >= 0 && pb.H >= 1 && pb.H <= MDL_MAX_HEADS &&
           src.ld >= (int64_t)pb.H * e.head_units && src.ld % e.stride_unit == 0 && d.p >= 0.f && d.p < 1.f;
}

// The only two places that refuse a gate call, in one order:
//   1. MDL_E_ARG: a required pointer or one of a pair is NULL, an incomplete pooling term, phases, terms, T, H, a stride below the row
//      width or off its alignment, p_drop   2. MDL_E_ALIGN   3. MDL_E_UNSUPPORTED: H not in {1,2,4,8}, a stride above its 32-bit limit
//   4. forwards: T == 0 is MDL_OK before any launch (*empty; a backward still zeroes its gradients)   5. MDL_E_UNSUPPORTED: a grid above
//      2^31 - 1
static inline int gate_check_fwd(const GateEngine& e, const GateFwdCall& c, bool* empty) {
    const GateParams& p = c.par;
    *empty = c.pb.T == 0;
    if (!c.src.p || (e.image && !c.src.scale) || !p.Wa || !p.ba || !p.Wb || !p.bb || !p.wc || !p.bc || !c.scores || !c.ws) return MDL_E_ARG;
    if ((c.act.a == nullptr) != (c.act.b == nullptr) || !gate_ranges_ok(e, c.src, c.pb, c.drop)) return MDL_E_ARG;
    if (!gate_aligned16(c.src.p, p.Wa, p.Wb, p.wc, c.act.a, c.act.b, c.ws)) return MDL_E_ALIGN;
    if (!gate_heads_ok(c.pb.H) || !stride_fits32(c.src.ld, e.elem_bytes, e.fwd.rows, e.fwd.col_bytes)) return MDL_E_UNSUPPORTED;
    if (*empty) return MDL_OK;
    return e.fwd_max_grid(c.pb.T, c.pb.H) > 0x7fffffff ? MDL_E_UNSUPPORTED : MDL_OK;
}
static inline int gate_check_bwd(const GateEngine& e, const GateBwdCall& c) {
    const GateParams& p = c.par;
    const GateGrads& g = c.g;
    const PoolTerm& pt = c.pt;
    if (!c.src.p || (e.image && !c.src.scale) || !p.Wa || !p.Wb || !p.wc || !c.act.a || !c.act.b || !c.d_scores || !c.de.p || !g.dWa ||
        !g.dWb || !g.dba || !g.dbb || !g.dwc || !c.ws)
        return MDL_E_ARG;
    if ((c.pool || pt.scores) && (!pt.scores || !pt.stat_m || !pt.stat_l || !pt.d_pooled || (!pt.row_bag && pt.N < 1))) return MDL_E_ARG;
    if (c.pb.phases < 1 || c.pb.phases > e.max_phases || (c.pb.terms != 2 && c.pb.terms != 3) || !gate_ranges_ok(e, c.src, c.pb, c.drop))
        return MDL_E_ARG;
    if (e.image && (c.de.ld < (int64_t)c.pb.H * HID || (c.de.ld & 3))) return MDL_E_ARG;
    if (!gate_aligned16(c.src.p, c.de.p, p.Wa, p.Wb, c.act.a, c.act.b, p.wc, c.ws)) return MDL_E_ALIGN;
    if (!gate_heads_ok(c.pb.H) || !stride_fits32(c.src.ld, e.elem_bytes, e.bwd.rows, e.bwd.col_bytes)) return MDL_E_UNSUPPORTED;
    if (e.image && !stride_fits32(c.de.ld, 4, 1, 0)) return MDL_E_UNSUPPORTED;   // the dX epilogue's 32-bit row pitch ld4 = ldE * 4
    return e.bwd_max_grid(c.pb.T, c.pb.H, c.pb.phases) > 0x7fffffff ? MDL_E_UNSUPPORTED : MDL_OK;
}

// ---- run-time value -> compile-time value: f(std::integral_constant<int, V>) for the V of the list that equals v, the last V for any
// other v.  A kernel launch is written once, inside f, for all of its template arguments.
template <int V, int... Rest, class F>
static inline int gate_pick(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : gate_pick<Rest...>(v, f);
}
// the dropout modes of gate_keep2_fwd (gate_drop_mode: 0 off, 1 hash with 16-bit fields, 3 hash with byte fields, 2 explicit masks)
template <class F>
static inline int gate_pick_dm(const DropCfg& d, F&& f) { return gate_pick<0, 1, 3, 2>(gate_drop_mode(d), f); }
// a forward kernel's <DM, SAVE>: f(dm, save), save = 1 where the activations are stored
template <class F>
static inline int gate_pick_fwd(const DropCfg& d, bool save, F&& f) {
    return gate_pick_dm(d, [&](auto dm) { return gate_pick<1, 0>(save, [&](auto sv) { return f(dm, sv); }); });
}
// one launch of any gate kernel; its status
template <class... P, class... A>
static inline int gate_launch(void (*kernel)(P...), dim3 grid, int threads, hipStream_t s, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, s, static_cast<P>(args)...);
    return (int)hipGetLastError();
}
static inline DropCfg make_drop(const GateDrop& d) { return make_drop(d.p, d.seed, d.keep_a, d.keep_b); }

// ---- grids ----
static inline int64_t gate_tiles(int64_t T, int tile) { return (T + tile - 1) / tile; }
struct GateFwdGeom {
    int tile;        // token rows of a tile
    int64_t n_tt;    // token tiles
    int pmode;       // 0: a workgroup per (token tile, column tile); 1: a workgroup runs the GATE_JT column tiles of a token tile; 2: `pt`
    int64_t grid;    //    token tiles of one column tile
};
// the forward's grid for token tiles of `tile` rows under persistence mode pmode (pt: token tiles per workgroup in mode 2)
static inline GateFwdGeom gate_fwd_grid(int64_t T, int H, int tile, int pmode, int pt) {
    GateFwdGeom g{tile, gate_tiles(T, tile), pmode, 0};
    const int64_t tiles = xcd_head_grid(g.n_tt, GATE_JT, H), per_share = (g.n_tt + 8 / H - 1) / (8 / H);
    g.grid = pmode == 1 ? tiles / GATE_JT : pmode == 2 ? 8 * ((per_share + pt - 1) / pt) * GATE_JT : tiles;
    return g;
}
// MADELEINE_*_PERSIST asks for mode `asked`; kept only where gate_persist_pays for the grid of tile workgroups
static inline int gate_pmode(int asked, int64_t T, int H, int tile, double gain, int pt) {
    const int64_t tiles = gate_fwd_grid(T, H, tile, 0, pt).grid;
    if (asked == 1 && !gate_persist_pays(tiles, gain)) return 0;
    if (asked == 2 && !gate_persist_pays(tiles, gain, pt)) return 0;
    return asked == 1 || asked == 2 ? asked : 0;   // any other value of the switch runs a workgroup per tile, as it always did
}
struct GateBwdGeom {
    // stated by the engine, by name:
    int S;                     // token splits of the dW contraction
    int chunk, min_chunks;     // a split is whole chunks of `chunk` tokens, at least min_chunks of them
    int pad;                   // zero rows behind dz, the token tail of the dW contraction
    int dz_rows;               // token rows per workgroup of the dz pass
    int dx_tile, dw_tile;      // token rows of a dX tile; the dW kernel (128 | 256) with dw_per output tiles per head and split
    int dw_per;
    // derived by gate_bwd_grid:
    int64_t tps, nblk, dx_grid, dw_grid;   // tokens per split, workgroups of the dz pass, dX over token tiles x 2 column halves, dW
};
static inline GateBwdGeom gate_bwd_grid(GateBwdGeom g, int64_t T, int H) {
    g.tps = ((T + g.S - 1) / g.S + g.chunk - 1) / g.chunk * g.chunk;
    if (g.tps < (int64_t)g.min_chunks * g.chunk) g.tps = (int64_t)g.min_chunks * g.chunk;
    g.nblk = gate_tiles(T, g.dz_rows);
    g.dx_grid = xcd_head_grid(gate_tiles(T, g.dx_tile), 2, H);
    g.dw_grid = xcd_head_grid(g.S, g.dw_per, H);
    return g;
}
// the widest launch of the phases: the dz pass (counted as nblk * H), and the dX grid where it runs; the dW grid is S-bound, far below
static inline int64_t gate_bwd_max_grid(const GateBwdGeom& g, int H, int phases) {
    const int64_t dz = g.nblk * H, dx = (phases & (2 | 4)) ? g.dx_grid : 0;
    return dz > dx ? dz : dx;
}
static inline void plan_splits(int64_t* o, int64_t T, const GateBwdGeom& g) { plan_splits(o, T, g.S, g.tps, g.chunk); }

// ---- workspace layouts: byte offsets and the total, read by the *_ws_bytes queries and by the launchers ----
struct WsCursor {
    int64_t o = 0;
    int64_t take(int64_t bytes) { const int64_t at = o; o += (bytes + 15) & ~(int64_t)15; return at; }
};
struct GateFwdWs { int64_t oW, opart, osc, total; };   // weight image [H][1024 x 512] | score partials [T][H][4] fp32 | scale floats (split)
static inline GateFwdWs gate_fwd_ws(int64_t T, int H, int w_elem_bytes, int sc_bytes) {
    WsCursor c;   // (a braced list is evaluated left to right)
    GateFwdWs w{c.take((int64_t)H * HID * 1024 * w_elem_bytes), c.take(T * H * GATE_JT * 4), c.take(sc_bytes), 0};
    w.total = c.o + 64;
    return w;
}
// weight image WN (bf16, split) | dz [T + pad][H][1024] | slabW [S][H][512][1024] fp32 | slabV [nblk][H][4][512] fp32 | scale floats (split)
struct GateBwdWs { int64_t oWN, odz, oslabW, oslabV, osc, total; };
static inline GateBwdWs gate_bwd_ws(int64_t T, int H, const GateBwdGeom& g, int wn_elem_bytes, int dz_elem_bytes, int sc_bytes) {
    WsCursor c;
    GateBwdWs w{c.take((int64_t)H * HID * 1024 * wn_elem_bytes), c.take((T + g.pad) * H * 1024 * dz_elem_bytes),
                c.take((int64_t)g.S * H * HID * 1024 * 4), c.take(g.nblk * H * 4 * HID * 4), c.take(sc_bytes), 0};
    w.total = c.o + 64;
    return w;
}
template <class Ws>   // a *_ws_bytes query: the total of the engine's layout, or the refusal of its sizes
static inline int64_t gate_ws_bytes(int64_t T, int H, Ws (*layout)(int64_t, int)) {
    return (T < 0 || H < 1 || H > MDL_MAX_HEADS) ? (int64_t)MDL_E_ARG : layout(T, H).total;
}
static inline int gate_zero_pad_rows(char* dz, int64_t T, int H, const GateBwdGeom& g, int dz_elem_bytes, hipStream_t s) {
    return (int)hipMemsetAsync(dz + T * H * 1024 * dz_elem_bytes, 0, (size_t)g.pad * H * 1024 * dz_elem_bytes, s);
}

// ---- the phases of a backward, spelled once.  Bit 0: set-up (the zero pad rows of dz, the engine's scales), the dz pass, the reduction of
// its column sums; bit 1 | 2: the dX half (weight image, contraction); bit 1 | 3: the dW half and the reduction of its slabs.  An empty
// problem runs everything but the dz pass and the dX half: the reductions zero the gradients.  The engines supply the steps.
template <class Setup, class Dz, class Dx, class Dw>
static inline int gate_bwd_phases(const GateBwdCall& c, const GateBwdGeom& g, float* slabW, float* slabV, Setup&& setup, Dz&& dz, Dx&& dx,
                                  Dw&& dw) {
    const GateProblem& pb = c.pb;
    if (pb.phases & 1) {
        if (const int rc = setup()) return rc;
        if (pb.T > 0)
            if (const int rc = dz()) return rc;
        if (const int rc = gate_launch_reduce_v(slabV, c.g.dba, c.g.dbb, c.g.dwc, c.g.dbc, pb.H, (int)g.nblk, c.s)) return rc;
    }
    if ((pb.phases & (2 | 4)) && pb.T > 0)
        if (const int rc = dx()) return rc;
    if (pb.phases & (2 | 8)) {
        if (const int rc = dw()) return rc;
        return gate_launch_reduce_w(slabW, c.g.dWa, c.g.dWb, pb.H, g.S, c.s);
    }
    return MDL_OK;
}

// ---- the wrappers' records: the 24 arguments every backward entry point of the tensor engines shares, in the header's order ----
template <class IO>
static inline GateBwdCall gate_bwd_call(const IO* E, int64_t ldE, const float* Wa, const float* Wb, const float* wc, const IO* act_a,
                                        const IO* act_b, const float* d_scores, IO* dE, int accumulate, float* dWa, float* dWb, float* dba,
                                        float* dbb, float* dwc, float* dbc, int64_t T, int H, float p_drop, uint64_t seed,
                                        const uint8_t* keep_a, const uint8_t* keep_b, void* ws, void* stream) {
    return {{E, ldE, nullptr}, {Wa, nullptr, Wb, nullptr, wc, nullptr}, {act_a, act_b}, d_scores, {dE, ldE, accumulate, nullptr},
            {dWa, dWb, dba, dbb, dwc, dbc}, {p_drop, seed, keep_a, keep_b}, {nullptr, nullptr, nullptr, nullptr, nullptr, 1}, false,
            {T, H, 3, 3}, ws, (hipStream_t)stream};
}
static inline GateBwdCall with_pool(GateBwdCall c, const PoolTerm& pt, int phases = 3) {
    c.pt = pt, c.pool = true, c.pb.phases = phases;
    return c;
}

}  // namespace mdl
