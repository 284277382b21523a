"""Every strided kernel at its stride limit and past element 2^31, on a device (the case table and the method: tests/_wide_cases.py).

tests/test_strides_cpu.py proves that a launcher refuses the first stride above its limit; nothing there shows that the limit is the
one the kernels need.  Here every stride argument with a 32-bit limit runs AT the largest stride its launcher accepts (Part A), and
every stride argument the headers call limit-free runs with rows past element 2^31 (Part B), on the shapes, the runners, the fp64
references and the bounds of the twin tests (tests/test_strides_gpu.py and the families' own files).  Every case asserts
  (a) the valid region of every output equals, bit for bit, the same call on contiguous copies;
  (b) no byte of the 12.5 GiB arena outside the valid slices changed, no input slice changed, and the small padded buffers of the
      operands that are not wide pass Lay's check;
  (c) the outputs pass the twin's check against its fp64 reference, with the twin's bound.
No case runs a call its launcher does not accept under the header, and none is meant to fault: a 32-bit offset that wraps can only
lower an address, and the first wide row lies 2^31 bytes into the arena, so a wrong kernel reads fill (NaN) or another row and fails
(a).  What is still not run: the exact edge of the kernels in _wide_cases.ARGUED, and the tiered store entry points."""
import pytest
import torch

from tests import _wide_cases as W
from tests._wide_cases import WideLay
from tests.test_dispatch_edges_gpu import _expect_plan
from tests import test_strides_gpu as S
from tests.test_strides_gpu import BF, F32, Lay, _strided_vs_contiguous

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena(dev):
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(dev)
    if free < W.MIN_FREE_BYTES:
        pytest.skip("%.1f GiB of %.1f GiB device memory free; the %.1f GiB arena is only taken with %d GiB free"
                    % (free / 2 ** 30, total / 2 ** 30, W.ARENA_BYTES / 2 ** 30, W.MIN_FREE_BYTES >> 30))
    mem = torch.empty(W.ARENA_BYTES, dtype=torch.uint8, device=dev)
    yield mem
    del mem
    torch.cuda.empty_cache()


def _runner(dev, c):
    """(run, check) of a case: the runner of the twin test on the twin's data."""
    p = dict(c.params)
    if c.family == "gate":
        bf16, H, fwd, T = p.pop("bf16"), p.pop("H"), p["forward"], c.T
        case = S._gate_case(T, H, 0.0, bf16)
        check = S._check_gate_b16 if bf16 else S._check_gate_f32
        return (lambda lay: S._run_gate(dev, lay, case, BF if bf16 else F32, T, H, 0.0, **p)), (lambda got: check(case, T, got, fwd))
    if c.family == "gate_split":
        H, fwd, T = p.pop("H"), p["forward"], c.T
        case = S._gate_case(T, H, 0.0, False)
        return (lambda lay: S._run_gate_split(dev, lay, case, T, H, **p)), (lambda got: S._check_gate_split(case, got, fwd))
    if c.family == "linear":
        bf16, N, K, T = p.pop("bf16"), p.pop("N"), p.pop("K"), c.T
        case = S._lin_case(T, N, K, bf16)
        check = S._check_linear_b16 if bf16 else S._check_linear_f32
        return (lambda lay: S._run_linear(dev, lay, case, BF if bf16 else F32, T, N, K, **p)), (lambda got: check(case, got, **p))
    return {"split_nt": S._split_nt_runner, "split_tn": S._split_tn_runner, "pool": S._pool_runner, "pool_views": S._pool_views_runner,
            "pool_img": S._pool_img_runner, "split_image": S._split_image_runner, "store": _store_runner, "attn": _attn_runner,
            "rank": _rank_runner, "retrieval": _retrieval_runner, "probe": _probe_runner, "cox": _cox_runner,
            "heat": _heat_runner}[c.family](dev, **p)


# ============================================================================================ the runners of the newer families (Part B)
# Each places its strided operand with lay.inp (a contiguous copy under Lay('contig'), a slice of the arena under WideLay), calls the
# entry points through the functional wrappers where these pass stride(0) on and through MF._call where they take contiguous input
# only, and hands the outputs to the checks of the family's own test file.
def _place(lay, x, k, dev):
    """x as operand k of the layout when k goes wide; otherwise a plain contiguous tensor (one label row per problem: Lay fills its
    padding with NaN and keeps rows 16 bytes apart, which integer rows and rows of 330 floats do not allow)."""
    if k in getattr(lay, "target", ()):
        return lay.inp(x, k)
    return x.to(dev).contiguous()


def _store_runner(dev, dtype):
    """bag_sample, bag_pack (whole bags and bags cut to 70 rows) and bag_mean on a resident store of test_store_gpu's bags."""
    from madeleine_amd import functional as MF
    from tests import test_store_embed_gpu as TE
    from tests import test_store_gpu as TS
    from tests import test_store_pack_gpu as TP
    dtype, D, lens = getattr(torch, dtype), 32, TS.LENS
    rows = TS._rows(sum(lens), D, D).to(dtype)
    mean_bag = list(range(len(lens)))
    mean_bag.insert(4, -1)
    caps = (None, 70)

    def tables():
        off, bag, key = TS._tables(lens, dev)
        return off, bag, key, [TP._cu(TP._out_lens(bag, lens, cap), dev) for cap in caps]

    def run(lay):
        store = lay.inp(rows)
        off, bag, key, packs = tables()
        out = {}
        smp, idx = MF.bag_sample(store, off, bag, key, 70, seed=5, counter=1, return_indices=True)
        out.update(sample=smp.reshape(bag.numel(), -1), sample_idx=idx)
        for cap, (cu, ch, T, n_chunks) in zip(caps, packs):
            tok, row_bag, pidx = MF.bag_pack(store, off, bag, key, cu, ch, T, n_chunks, seed=5, counter=1, return_indices=True)
            out.update({"pack%s" % cap: tok, "pack%s_row_bag" % cap: row_bag.view(1, -1), "pack%s_idx" % cap: pidx.view(1, -1)})
        off_m, bag_m, ch_m, n_m = TE._tables(lens, mean_bag, dev)
        out["mean"] = MF.bag_mean(store, off_m, bag_m, ch_m, n_m)
        return out

    def check(got):
        off, bag, key = (t.cpu() for t in TS._tables(lens, torch.device("cpu")))
        TS._check_gather(rows, off, bag, got["sample"].view(bag.numel(), 70, D), got["sample_idx"])
        TS._check_draw(got["sample_idx"], lens, bag, 70)
        for cap in caps:
            TP._check_pack(rows, off, bag, lens, TP._out_lens(bag, lens, cap), got["pack%s" % cap], got["pack%s_row_bag" % cap].view(-1),
                           got["pack%s_idx" % cap].view(-1))
        TE.check_mean(rows, off, got["mean"], lens, mean_bag)
    return run, check


def _attn_runner(dev, name, H):
    """attn_softmax and attn_rank (k = 0, 16 and past the longest bag) on the score sets of test_attention_gpu."""
    from madeleine_amd import functional as MF
    from tests import test_attention_gpu as TA
    import numpy as np
    s = torch.from_numpy(np.array(TA.scores_of(name, H)))
    ks = (0, 16, TA.KMAX)

    def run(lay):
        sd, cu = lay.inp(s), torch.from_numpy(TA.cu_of(TA.LENS)).to(dev)
        attn, m, l_ = MF.attn_softmax(sd, cu)
        out = dict(attn=attn, m=m, l=l_)
        for k in ks:
            order, pct, ti, tv = MF.attn_rank(sd, cu, k=k)
            out.update({"order%d" % k: order, "pct%d" % k: pct})
            if k:
                out.update({"topk_idx%d" % k: ti.reshape(len(TA.LENS), -1), "topk_val%d" % k: tv.reshape(len(TA.LENS), -1)})
        return out

    def check(got):
        TA.check_softmax(name, H, got["attn"], got["m"], got["l"])
        for k in ks:
            ti = got["topk_idx%d" % k].view(len(TA.LENS), H, k) if k else None
            tv = got["topk_val%d" % k].view(len(TA.LENS), H, k) if k else None
            TA.check_rank(name, H, k, got["order%d" % k], got["pct%d" % k], ti, tv)
    return run, check


def _rank_runner(dev, n, d):
    """mdl_smooth_rank and mdl_smooth_rank_marked on the matrix of test_rank_gpu.test_row_stride_keeps_the_bits."""
    from madeleine_amd import functional as MF
    from tests import _rank_ref as RR
    from tests import test_rank_gpu as TR
    E = RR.gauss(n, d + 24, 7)[:, :d].copy()

    def run(lay):
        Ev = lay.inp(torch.from_numpy(E))
        out, sigma = MF._rank_call(Ev, RR.EPS)
        rank_m, sigma_m, _ = MF.smooth_rank_stages(Ev, RR.EPS)
        return dict(out=out.view(1, -1), sigma=sigma.view(1, -1), marked_rank=rank_m.view(1, 1), marked_sigma=sigma_m.view(1, -1))

    def check(got):
        out, sigma = got["out"].view(-1), got["sigma"].view(-1)
        assert out.dtype == sigma.dtype == torch.float64
        TR.check_result(E, float(out[0]), float(out[1]), sigma.numpy(), RR.RANK_TOL[RR.FULL], "slice %dx%d" % (n, d))
        assert torch.equal(got["marked_rank"].view(-1), out[:1]) and torch.equal(got["marked_sigma"].view(-1), sigma), "the marked call"
    return run, check


def _retrieval_runner(dev, n, m, d, noise, k):
    from madeleine_amd import functional as MF
    from tests import test_retrieval_gpu as TQ
    Q, K, _, _ = TQ.cosine_case(n, m, d, noise)

    def place(lay, x, i):      # (d = 77: Lay's 16-byte row pitch does not exist for it; the other operand gets the twin's ld = d + 24)
        if lay.mode == "contig":
            return torch.from_numpy(x).to(dev)
        if i in lay.target:
            return lay.inp(torch.from_numpy(x), i)
        buf = torch.full((x.shape[0], d + 24), float("nan"), device=dev)
        buf[:, :d] = torch.from_numpy(x).to(dev)
        return buf[:, :d]

    def run(lay):
        Qv, Kv = place(lay, Q, 0), place(lay, K, 1)
        assert lay.mode == "contig" or not (Qv.is_contiguous() or Kv.is_contiguous())
        res = MF.retrieval(Qv, Kv, k=k)
        return dict(greater=res.greater.view(1, -1), equal=res.equal.view(1, -1), pair_sim=res.pair_sim.view(1, -1), topk_idx=res.topk_idx,
                    topk_val=res.topk_val)

    def check(got):
        TQ.check_cosine_result(n, m, d, noise, k, (got["greater"].view(-1).numpy(), got["equal"].view(-1).numpy(),
                                                    got["pair_sim"].view(-1).numpy(), got["topk_idx"].numpy(), got["topk_val"].numpy()))
    return run, check


def _probe_runner(dev, mod, cohort):
    """mdl_probe_fit / mdl_logit_fit, mdl_probe_scores and mdl_probe_metrics / mdl_logit_metrics on a cohort of the family's file, by
    MF._call: X is operand 0; operand 1 is the label matrix [P, S], one row per problem (the wrappers take it contiguous only).  A
    cohort of fewer than 10 problems repeats its first ones: ten rows keep the span inside the arena."""
    from madeleine_amd import functional as MF
    if mod == "probe":
        from tests import test_probe_gpu as TP
        co = dict(TP.R.cohort(cohort))
    else:
        from tests import test_probe_cv_gpu as TP
        co = dict(TP.V.cohort(cohort))
    while len(co["problems"]) < 10:
        co["problems"] = (co["problems"] * 2)[:10]
    C, cols = co["C"], 1 if co["C"] == 2 else co["C"]
    fit, metrics = ("mdl_probe_fit", "mdl_probe_metrics") if mod == "probe" else ("mdl_logit_fit", "mdl_logit_metrics")

    def run(lay):
        table, n_train = TP._table([p["idx"] for p in co["problems"]])
        P, n_max = table.shape
        X = lay.inp(co["X"].float(), 0)
        S_, d = X.shape
        y = _place(lay, co["y"].to(torch.int32).unsqueeze(0).expand(P, S_).contiguous(), 1, dev)
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        W, b, info, z, auc = nan(P, cols, d), nan(P, cols), nan(P, 4), nan(P, S_, cols), nan(P)
        conf = torch.full((P, C, C), -7, dtype=torch.int32, device=dev)
        MF._call(fit, X, X.stride(0), S_, d, y, y.stride(0), table, n_train, P, n_max, C, 1.0, TP.GTOL, 100, W, b, info,
                 MF._ws_for(fit + "_ws_bytes", dev, P, n_max, d, C), MF._stream())
        MF._call("mdl_probe_scores", X, X.stride(0), S_, d, W, b, P, C, z, MF._stream())
        MF._call(metrics, z, y, y.stride(0), table, n_train, P, n_max, S_, C, conf, auc, MF._ws_for(metrics + "_ws_bytes", dev, P, S_, C),
                 MF._stream())
        return dict(W=W.view(P, -1), b=b, info=info, z=z.view(P, -1), conf=conf.view(P, -1), auc=auc.view(1, -1))

    def check(got):
        P = len(co["problems"])
        S_, d = co["X"].shape
        out = dict(W=got["W"].view(P, cols, d), b=got["b"], info=got["info"], z=got["z"].view(P, S_, cols), conf=got["conf"].view(P, C, C),
                   auc=got["auc"].view(-1))
        TP._optimality(cohort, co, out)
        TP._decision_values(cohort, co, out)
        TP._metrics_against_fp64_optimum(cohort, co, out)
    return run, check


def _cox_runner(dev, cohort):
    """mdl_cox_fit, mdl_probe_scores and mdl_surv_metrics on a cohort of test_survival_gpu, by MF._call: X is operand 0, the follow-up
    times [P, S] operand 1, the event flags [P, S] operand 2, one row per problem; the cohort's 7 problems are made 10."""
    from madeleine_amd import functional as MF
    from tests import test_survival_gpu as TS
    co = dict(TS.R.cohort(cohort))
    while len(co["problems"]) < 10:
        co["problems"] = (co["problems"] * 2)[:10]

    def run(lay):
        table, n_train = TS._table([p["idx"] for p in co["problems"]])
        P, n_max = table.shape
        X = lay.inp(co["X"].float(), 0)
        S_, d = X.shape
        tm = _place(lay, co["time"].float().unsqueeze(0).expand(P, S_).contiguous(), 1, dev)
        ev = _place(lay, co["event"].to(torch.int32).unsqueeze(0).expand(P, S_).contiguous(), 2, dev)
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        W, thr, info, z = nan(P, d), nan(P), nan(P, 4), nan(P, S_, 1)
        c_index, chi2 = torch.full((P,), float("nan"), dtype=torch.float64, device=dev), torch.full((P,), float("nan"), dtype=torch.float64, device=dev)
        counts = torch.full((P, 6), -7, dtype=torch.int32, device=dev)
        MF._call("mdl_cox_fit", X, X.stride(0), S_, d, tm, tm.stride(0), ev, ev.stride(0), table, n_train, P, n_max, float(co["cost"]), TS.GTOL,
                 100, W, thr, info, MF._ws_for("mdl_cox_order_fit_ws_bytes", dev, P, n_max, d), MF._stream())
        MF._call("mdl_probe_scores", X, X.stride(0), S_, d, W.unsqueeze(1), torch.zeros(P, 1, device=dev), P, 2, z, MF._stream())
        z = z.squeeze(2)
        MF._call("mdl_surv_metrics", z, tm, tm.stride(0), ev, ev.stride(0), table, n_train, P, n_max, S_, thr, c_index, chi2, counts,
                 MF._ws_for("mdl_surv_metrics_ws_bytes", dev, P, S_), MF._stream())
        return dict(W=W, thr=thr.view(1, -1), info=info, z=z, c=c_index.view(1, -1), chi2=chi2.view(1, -1), counts=counts)

    def check(got):
        out = dict(got, thr=got["thr"].view(-1), c=got["c"].view(-1), chi2=got["chi2"].view(-1))
        for rule in (TS._optimality, TS._decision_values, TS._metrics_equal_the_host_recount, TS._metrics_against_fp64_optimum):
            rule(cohort, co, out)
    return run, check


def _heat_runner(dev, C):
    """mdl_heat_render and mdl_heat_render_marked on the bags of test_heatmap_gpu.test_channels_and_row_stride."""
    import numpy as np
    from madeleine_amd import functional as MF
    from tests import _heat_ref as HR
    from tests import test_heatmap_gpu as TH
    rng = np.random.default_rng(8 + C)
    xy = rng.integers(0, 500, (700, 2))
    v = rng.random((700, C), dtype=np.float32)
    cu, canv, ds, taps = [0, 300, 700], [(32, 0, 0, 67, 67), (32, 10, 10, 33, 70)], 8, TH.box_taps(2)

    def run(lay):
        vd = lay.inp(torch.from_numpy(v))
        out = {}
        for b, (level, covered, rgba) in enumerate(TH.device_render(dev, xy, cu, vd, canv, ds, taps, TH.GRAY, 255)):
            out.update({"level%d" % b: level.view(torch.int16).reshape(C, -1), "covered%d" % b: covered.reshape(C, -1), "rgba%d" % b: rgba.reshape(C, -1)})
        rec, P = TH.records_of(canv)
        level, covered, rgba, _ = MF.heat_render_stages(torch.from_numpy(xy.astype(np.int32)).to(dev), torch.tensor(cu, device=dev), vd, rec, P, ds,
                                                        torch.tensor(taps, dtype=torch.int32), torch.from_numpy(TH.GRAY).to(dev), 255)
        out.update(marked_level=level.view(torch.int16).view(1, -1), marked_covered=covered.view(1, -1), marked_rgba=rgba)
        return out

    def check(got):
        want = HR.render(xy, cu, v, canv, ds, taps, TH.GRAY, 255, None)
        for b, (w, (ps, ox, oy, Wd, Hd)) in enumerate(zip(want, canv)):
            TH.same_bits((got["level%d" % b].view(C, Hd, Wd), got["covered%d" % b].view(C, Hd, Wd), got["rgba%d" % b].view(C, Hd, Wd, 4)), w,
                         "of bag %d" % b)
        assert torch.equal(got["marked_level"].view(-1), torch.cat([got["level%d" % b].reshape(-1) for b in range(len(canv))])), "the marked call"
        assert torch.equal(got["marked_covered"].view(-1), torch.cat([got["covered%d" % b].reshape(-1) for b in range(len(canv))]))
        assert torch.equal(got["marked_rgba"].view(-1), torch.cat([got["rgba%d" % b].reshape(-1) for b in range(len(canv))]))
    return run, check


def _run_wide(dev, arena, c, ld):
    assert c_span(c) * ld * c.elem + W.LEAD <= arena.numel(), "the span and the lead do not fit the arena"
    run, check = _runner(dev, c)
    lay = WideLay(arena, c.target, ld, c.elem, Lay("pad", dev))
    _strided_vs_contiguous(dev, "wide", run, check, lay=lay)
    assert lay.slices, "the case has no wide operand"
    assert max(s["rows"] for s in lay.slices) == c_span(c), "the table's row count is not the one the runner uses"
    return lay


def c_span(c):
    return c.span_rows if isinstance(c, W.A) else c.R


@pytest.mark.parametrize("c", W.PART_A, ids=lambda c: c.id)
def test_at_the_limit(dev, arena, c):
    """Part A: the largest aligned stride the launcher accepts (kind 'ii': the largest that fits the arena, on the limiting kernel)."""
    for product, T, a, b, want in c.plan:
        _expect_plan(product, T, a, b, want)
    ld = c.ld
    if c.kind != "ii":
        assert c.rows * ld * c.elem + c.col <= W.LIM < c.rows * (ld + c.align) * c.elem + c.col
    lay = _run_wide(dev, arena, c, ld)
    assert c.capped or lay.far_rows(1 << 32) >= 1, "no valid row starts 2^32 bytes from the operand's base"


@pytest.mark.parametrize("c", W.PART_B, ids=lambda c: c.id)
def test_far(dev, arena, c):
    """Part B: a stride without a limit, with the last max(2, R // 8) rows past element 2^31 (byte 2^32 for a stride in bytes)."""
    lay = _run_wide(dev, arena, c, c.ld)
    assert lay.far_rows(c.mark * c.elem) >= max(2, c.far_rows), "fewer than two rows start past the mark"


def test_peak_memory(dev, arena):
    """Runs last in the file: reports the peak of the device allocator (the arena, one scan mask and the operands of a case)."""
    peak = torch.cuda.max_memory_allocated(dev)
    print("peak device memory allocated: %.2f GiB" % (peak / 2 ** 30))
    assert peak >= arena.numel()
