"""Every kernel that draws dropout from the counter hash draws the mask the host model states (tests/_drop_ref.py, written from the
specification of mix32 / the seed key / the threshold / the row key and calling nothing of the library).

The chain that carries the hash mode to the fp64 references:
  (a), (b)  mdl_abmil_gate_dropout_mask == the model, bit for bit (both field widths, thr 0 and 65535, 64-bit seeds, and (b) on both sides
            of element index 2^32).  tests/test_gate_kinds_gpu.py (iv) and tests/test_dispatch_edges_gpu.py already hold the gate's hash
            calls to the same calls fed these exported masks, and the mask calls to fp64: the export was the one link nothing stated.
  (c)       every LayerNorm-GELU-Dropout entry point that draws: the call with (p, seed, keep = NULL) equals the call with (p, 0, keep =
            the model's mask) in every output, as bytes.  The mask path is held to fp64 by tests/test_hip_kernels.py::
            test_ln_gelu_drop_vs_torch / ::test_ln_gelu_drop_groups_vs_torch (and tests/test_ln_kinds_gpu.py ties the split entries to the
            plain ones in mask mode), so equality to the bit carries the hash path -- the one training runs -- to the same reference.
            The two calls run the same arithmetic; only the source of the multiplier differs (DM 1 against 2).
  (d)       the fp32 forward's y is y(p = 0) * inv(p) exactly where the model keeps and an exact zero where it drops: the mask is read off
            the hash call itself, without the mask path.
  (e)       through ABMILEmbedder / MADELEINE in train mode on every engine: the step run from recorded seeds equals, in the loss and in
            every gradient as bytes, the step run from the model's masks of those seeds injected in the layout _drop_cfg / _gate_dropout
            expect -- the seed reaches forward and backward alike, and the hash mask relates to the injected layout as the Python side assumes.
  (f)       one fresh seed per dropout site and forward, reproducible under torch.manual_seed, none in eval mode, none in a backward.

Result on the device: every pair of (c) and every engine of (e) is equal to the bit; no pair needed the fallback to its fp64 bound, and
(d) excluded no element (the inputs have no exact zero: tests/test_dropout_hash_cpu.py::test_ln_case_inputs_tell_kept_from_dropped).
(b) found the export itself wrong past 2^32 elements: it launched one thread per element, a launch carries its work-items per dimension
in 32 bits, and T = 2^20 + 8 at H = 8 wrote its first 32768 bytes and nothing else, without an error (fixed: the kernel strides).

Mutations of a scratch build, none committed: `lo4 + 2u` -> `lo4 + 1u` in act_keep4_t fails the bf16 and split cases of (c), (d), (e); the
two fields of a pair swapped in act_keep4 fails the fp32 cases of (c), (d), (e); `>` for `>=` on the byte fields of drop_keep2 (the
export's form) fails (a) and (b), the same in gate_keep2_hash (the kernels' form) fails every case of (e); both row keys without their
high-word term fail (b) and nothing else.

Not covered, because the operands would be tens of GB: the gate forward / backward kernels and every LayerNorm kernel above element index
2^32 (drop_row_key in the epilogues, act_row_key).  Dropping the high-word term there makes no test fail; for the gate only (b), the
export, sees it.  tests/test_stride_limits_gpu.py does not change this: it runs the gates with rows of E and dE past byte 2^32 and
element 2^31 of their buffers (wide row strides, at the launchers' limits), which holds their ADDRESSES to 64 bits, but the hash index
is token * H * 512 + column, a function of T and not of the stride, and T stays a few hundred there."""
import numpy as np
import pytest
import torch

from tests import _drop_ref as D
from tests import test_ln_kinds_gpu as K
from tests._switches import switch  # noqa: F401  (a fixture)
from tests._util import MODS5, t
from tests.test_ln_kinds_gpu import ln_bwd, ln_bwd_split, ln_fwd, ln_fwd_split, same_bits

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2 ** 62 - 1, 2 ** 63 + 5)
LN_DRAWS = [(p, seed) for p in (0.1, 0.25) for seed in (1234, 2 ** 63 + 5)]
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _export(T, H, which, p, seed, dev, out=None):
    from madeleine_amd import functional as MF
    m = torch.empty(T, H, D.HID, dtype=torch.uint8, device=dev) if out is None else out
    MF._call("mdl_abmil_gate_dropout_mask", m, T, H, which, float(p), seed, MF._stream())
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) exported gate masks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5, 0.1, 0.3, 1e-6, 0.99999])
@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_exported_gate_mask_equals_the_model(dev, switch, H, p):
    switch("MADELEINE_DROP_16BIT", 0)
    for T in (1, 130):
        for seed in SEEDS:
            want = [D.gate_keep(T, H, which, p, seed) for which in (0, 1)]
            for which in (0, 1):
                got = _export(T, H, which, p, seed, dev).cpu().numpy()
                assert np.array_equal(got, want[which]), (T, H, which, p, seed, int((got != want[which]).sum()))
            if p == 1e-6:
                assert want[0].all() and want[1].all()              # threshold 0: everything is kept
            if p == 0.99999:
                assert want[0].mean() < 1e-3                        # threshold 65535: a field survives only at 0xFFFF


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_exported_gate_mask_with_the_byte_fields_switched_off(dev, switch, H):
    """p = 0.25 under MADELEINE_DROP_16BIT=1: the 16-bit rule, another mask than the byte rule gives."""
    for T in (1, 130):
        for seed in SEEDS:
            for which in (0, 1):
                switch("MADELEINE_DROP_16BIT", 1)
                got16 = _export(T, H, which, 0.25, seed, dev).cpu().numpy()
                switch("MADELEINE_DROP_16BIT", 0)
                got8 = _export(T, H, which, 0.25, seed, dev).cpu().numpy()
                assert np.array_equal(got16, D.gate_keep(T, H, which, 0.25, seed, force16=True)), (T, H, which, seed)
                assert np.array_equal(got8, D.gate_keep(T, H, which, 0.25, seed)), (T, H, which, seed)
                assert T == 1 and H == 1 or not np.array_equal(got16, got8)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the high word of the element index
# ---------------------------------------------------------------------------------------------------------------------------------
def test_exported_gate_mask_across_index_2_pow_32(dev, switch):
    """T = 2^20 + 8 tokens at H = 8: 2^32 + 32768 elements (4.3 GB of uint8), the smallest shape whose indices cross 2^32 -- token 2^20
    starts exactly there.  Token rows [0, 8) and [2^20 - 8, 2^20 + 8) against the model at p = 0.1 (16-bit fields) and, into the same
    buffer, p = 0.25 (byte fields), both masks.  This is the only test that executes drop_row_key's high-word term: the gate forward /
    backward kernels and the LayerNorm kernels (act_row_key) are not run there -- their operands would be tens of GB -- so a wrong high
    word in those is not seen by any test (the wide strides of tests/test_stride_limits_gpu.py move addresses past 2^32, not the hash
    index, which depends on T alone)."""
    switch("MADELEINE_DROP_16BIT", 0)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 6 * 2 ** 30:
        pytest.skip("needs one 4.3 GB buffer: %.1f GB of device memory are free, 6 GB asked for" % (free / 2 ** 30))
    T, H, seed = 2 ** 20 + 8, 8, 2 ** 63 + 5
    rows = np.concatenate([np.arange(8), np.arange(2 ** 20 - 8, 2 ** 20 + 8)])
    rows_d = torch.from_numpy(rows).to(dev)
    buf = torch.empty(T, H, D.HID, dtype=torch.uint8, device=dev)
    assert buf.numel() > 2 ** 32
    for p in (0.1, 0.25):
        for which in (0, 1):
            got = _export(T, H, which, p, seed, dev, out=buf).index_select(0, rows_d).cpu().numpy()
            want = D.gate_keep(T, H, which, p, seed, rows=rows)
            assert np.array_equal(got, want), (p, which, [int(r) for r in rows[(got != want).reshape(len(rows), -1).any(1)]])
            # the rows past 2^32 are not the rows a 32-bit index would give them
            low = D.gate_keep(T, H, which, p, seed, rows=rows[-8:] - 2 ** 20)
            assert not np.array_equal(want[-8:], low)
    del buf


# ---------------------------------------------------------------------------------------------------------------------------------
# (c), (d) the LayerNorm-GELU-Dropout family
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def draw(monkeypatch):
    """The call helpers of tests/test_ln_kinds_gpu.py take (p, seed, keep) from their module's drop_args: here from the inputs."""
    monkeypatch.setattr(K, "drop_args", lambda inp, mode: (0.0, 0, None) if mode == "off" else
                        (inp["p"], inp["seed"], None) if mode == "hash" else (inp["p"], 0, inp["keep"]))


_CASES = {}


def _case(dev, W, rows, dtype=torch.float32):
    """The inputs of tests/_drop_ref.py:ln_case_inputs on the device (built once per shape and type, never written)."""
    key = (W, rows, dtype)
    if key not in _CASES:
        inp = {k: torch.from_numpy(v).to(dev) for k, v in D.ln_case_inputs(W, rows).items()}
        inp["x"], inp["dy"] = inp["x"].to(dtype), inp["dy"].to(dtype)
        assert all(v.is_contiguous() for v in inp.values())
        _CASES[key] = inp
    return dict(_CASES[key])


def _with_draw(inp, p, seed, dev):
    rows, W = inp["x"].shape
    return dict(inp, p=p, seed=seed, keep=torch.from_numpy(D.ln_keep(rows, W, p, seed)).to(dev))


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), what + (k, int((a[k].contiguous().view(torch.uint8) != b[k].contiguous().view(torch.uint8)).sum()))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W,rows", D.LN_SHAPES)
def test_ln_hash_call_equals_mask_call_with_the_models_mask(dev, draw, W, rows, dtype):
    """mdl_ln_gelu_drop_fwd / _bwd and their _bf16 forms: y, mean, rstd; dx, dgamma, dbeta, dbias."""
    for p, seed in LN_DRAWS:
        inp = _with_draw(_case(dev, W, rows, dtype), p, seed, dev)
        fh, fm = ln_fwd(inp, "hash"), ln_fwd(inp, "mask")
        _assert_same(fh, fm, (p, seed, "forward"))
        _assert_same(ln_bwd(inp, fh, "hash"), ln_bwd(inp, fm, "mask"), (p, seed, "backward"))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W,rows", D.LN_GROUP_SHAPES)
def test_ln_grouped_hash_call_equals_mask_call_with_the_models_mask(dev, draw, W, rows, dtype):
    """mdl_ln_gelu_drop_fwd_groups / _bwd_groups and their _bf16 forms, three groups of which the middle one is empty: y, mean, rstd; dx,
    dgamma, dbeta, dgroup_bias."""
    cu = torch.tensor(D.ln_case_groups(rows), dtype=torch.int64, device=dev)
    base = _case(dev, W, rows, dtype)
    base["bias"] = torch.stack([base["bias"], -base["bias"], 0.5 * base["bias"]]).contiguous()      # one bias row per group
    for p, seed in LN_DRAWS:
        inp = _with_draw(base, p, seed, dev)
        fh, fm = ln_fwd(inp, "hash", cu), ln_fwd(inp, "mask", cu)
        _assert_same(fh, fm, (p, seed, "forward"))
        bh, bm = ln_bwd(inp, fh, "hash", cu), ln_bwd(inp, fm, "mask", cu)
        assert "dgroup_bias" in bh
        _assert_same(bh, bm, (p, seed, "backward"))


@pytest.mark.parametrize("W,rows", D.LN_SHAPES)
def test_ln_split_hash_call_equals_mask_call_with_the_models_mask(dev, draw, W, rows):
    """mdl_ln_gelu_drop_fwd_split with y requested and image-only (y, image bytes, scale, mean, rstd, rstd_max), mdl_ln_gelu_drop_bwd_split
    and _bwd_split_groups (dx image bytes with its 32 zero rows, dx scale, dgamma, dbeta, dbias, dgroup_bias)."""
    cu = torch.tensor(D.ln_case_groups(rows), dtype=torch.int64, device=dev)
    for p, seed in LN_DRAWS:
        inp = _with_draw(_case(dev, W, rows), p, seed, dev)
        for want_y in (True, False):
            fh, fm = (ln_fwd_split(inp, mode, want_y, want_rstd_max=True) for mode in ("hash", "mask"))
            assert ("y" in fh) == want_y and "rstd_max" in fh
            _assert_same(fh, fm, (p, seed, "forward, y requested" if want_y else "forward, image only"))
        _assert_same(ln_bwd_split(inp, fh, "hash"), ln_bwd_split(inp, fm, "mask"), (p, seed, "backward"))
        gh, gm = ln_bwd_split(inp, fh, "hash", cu=cu), ln_bwd_split(inp, fm, "mask", cu=cu)
        assert "dgroup_bias" in gh
        _assert_same(gh, gm, (p, seed, "grouped backward"))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W,rows", D.LN_SHAPES)
def test_ln_forward_keeps_what_the_model_keeps_and_scales_by_inv(dev, draw, W, rows, dtype):
    """(d), and the mask read off the hash call itself: y != 0 wherever the p = 0 call of the same inputs is non-zero.  fp32: a kept element
    is y(p = 0) * inv(p) exactly (the kernel forms gelu * kp with kp = inv or 0), a dropped one an exact zero.  bf16: the same mask (the
    product is rounded once more, so only the mask is compared).  At most 1e-5 of a case may be left out for an exact zero at p = 0."""
    base = _case(dev, W, rows, dtype)
    y0 = ln_fwd(base, "off")["y"]
    live = y0 != 0
    assert float((~live).float().mean()) <= 1e-5
    for p, seed in LN_DRAWS:
        inp = _with_draw(base, p, seed, dev)
        y, keep = ln_fwd(inp, "hash")["y"], inp["keep"].bool()
        assert torch.equal((y != 0) & live, keep & live), (p, seed, int((((y != 0) != keep) & live).sum()))
        assert not bool((y[~keep] != 0).any()), "dropped elements are exact zeros"
        if dtype == torch.float32:
            want = y0 * float(D.inv(p))           # (an fp32 product: the scalar is a float32 value)
            assert same_bits(torch.where(keep, y, torch.zeros_like(y)), torch.where(keep, want, torch.zeros_like(y))), (p, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# (e), (f) through the model
# ---------------------------------------------------------------------------------------------------------------------------------
class _Seeds:
    """Stands in for functional.new_dropout_seed: hands out `fixed` in order, or passes the library's own draws through; records both."""

    def __init__(self, real, fixed=None):
        self.real, self.fixed, self.drawn = real, fixed, []

    def __call__(self):
        s = self.fixed[len(self.drawn)] if self.fixed is not None else self.real()
        self.drawn.append(s)
        return s


FIXED_SEEDS = [2 ** 63 + 5, 1234, 2 ** 62 - 1, 77]         # the three pre-attention blocks, then the gates (c_uint64 takes the first)
D_IN = 64


def _model(dev, H, stain):
    from tests.test_heads_gpu import _build
    model, _ = _build(MODS5[:2], D_IN, "drophash%d" % H, dev, H, stain_encoding=stain)
    return model.train()


def _masks_from_seeds(model, seeds, lead, dev):
    """The masks of the model's four dropout sites for `seeds`, in the layout _injected_keep takes: pre[blk] [*lead, W] in the reference's
    channel order -- the kernel draws block 2 in head-major order j' and _drop_cfg hands it keep[..., perm], so the injected mask is the
    kernel's under the inverse permutation -- and gate[c] = (ka, kb) [*lead, 512] of head c."""
    emb = model.wsi_embedders
    H, T = emb.n_heads, int(np.prod(lead))
    p_pre, p_gate = float(emb.pre_attn[3].p), emb.attn[0].dropout_p()
    assert (p_pre, p_gate) == (0.1, 0.25)
    inv_perm = emb._inv_perm.cpu().numpy()
    pre = [D.ln_keep(T, 512, p_pre, seeds[0]), D.ln_keep(T, 512, p_pre, seeds[1]), D.ln_keep(T, 512 * H, p_pre, seeds[2])[:, inv_perm]]
    ka, kb = (D.gate_keep(T, H, which, p_gate, seeds[3]) for which in (0, 1))
    dv = lambda a, w: torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(*lead, w)      # noqa: E731
    return {"pre": [dv(m, m.shape[-1]) for m in pre], "gate": [(dv(ka[:, c], 512), dv(kb[:, c], 512)) for c in range(H)]}


def _step(model, run, leaves):
    """loss and every gradient (parameters, then inputs) of one forward + backward of a scalar loss."""
    model.zero_grad(set_to_none=True)
    fresh = [x.detach().clone().requires_grad_() for x in leaves]
    embs, toks = run(fresh)
    loss = sum((embs[k].float() * (1.0 + 0.1 * i)).square().sum() + 0.01 * toks[k].float().sum() for i, k in enumerate(sorted(embs)))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    grads.update({"input%d" % i: x.grad.detach().clone() for i, x in enumerate(fresh) if x.grad is not None})
    return loss.detach().reshape(1).clone(), grads


ENGINES = ("split", "fp32", "bf16")
MODEL_CASES = [(e, 4, "dense") for e in ENGINES] + [(e, 1, "dense") for e in ENGINES] + [(e, 4, "stain") for e in ENGINES] + \
    [(e, 4, "ragged") for e in ENGINES]


@pytest.mark.parametrize("engine,H,kind", MODEL_CASES, ids=["%s-H%d-%s" % c for c in MODEL_CASES])
def test_model_step_from_seeds_equals_step_from_the_models_masks(dev, monkeypatch, switch, engine, H, kind):
    """(e): 'split' = the split engine (the default; more than 256 token rows), 'fp32' = the exact-fp32 engine, 'bf16' = under autocast;
    'stain' = with stain encodings (the grouped LayerNorm path; on the split engine the per-group bias and the split-grouped backward),
    'ragged' = forward_ragged on packed bags of unequal lengths."""
    from madeleine_amd import functional as MF
    switch("MADELEINE_DROP_16BIT", 0)
    monkeypatch.setattr(MF, "GEMM_MODE", "fp32" if engine == "fp32" else "split")
    model = _model(dev, H, kind == "stain")
    if kind == "ragged":
        lens = [[70, 200], [130, 97]]
        leaves = [t((n, D_IN), "drophash:bag%d" % n).to(dev) for row in lens for n in row]
        lead = (sum(sum(row) for row in lens), 1)
        call = lambda xs: model.forward_ragged([xs[0:2], xs[2:4]], dev, n_loss_tokens=64)      # noqa: E731
    else:
        B, M, N = 2, 2, 160
        leaves = [t((B, M, N, D_IN), "drophash:feats").to(dev)]
        lead = (B * M, N)
        call = lambda xs: model({"feats": xs[0]}, device=dev, train=True)      # noqa: E731

    def run(xs):
        with torch.autocast(device_type="cuda", dtype=BF, enabled=engine == "bf16"):
            return call(xs)

    rec = _Seeds(MF.new_dropout_seed, FIXED_SEEDS)
    monkeypatch.setattr(MF, "new_dropout_seed", rec)
    loss_h, grads_h = _step(model, run, leaves)
    assert rec.drawn == FIXED_SEEDS, "three blocks, then the gates; nothing drawn in the backward"
    model.wsi_embedders._injected_keep = _masks_from_seeds(model, rec.drawn, lead, dev)
    loss_m, grads_m = _step(model, run, leaves)
    assert len(rec.drawn) == 4, "injected masks draw no seed"
    assert torch.isfinite(loss_h) and same_bits(loss_h, loss_m), (float(loss_h), float(loss_m))
    assert grads_h.keys() == grads_m.keys() and len(grads_h) >= 12 + 5 * H
    assert any(k.startswith("input") for k in grads_h)
    differ = [k for k in grads_h if not same_bits(grads_h[k], grads_m[k])]
    assert not differ, differ
    # and the masks matter: other seeds give another step
    model.wsi_embedders._injected_keep = None
    monkeypatch.setattr(MF, "new_dropout_seed", _Seeds(None, [s + 1 for s in FIXED_SEEDS]))
    assert not same_bits(loss_h, _step(model, run, leaves)[0])


def test_seeds_are_fresh_reproducible_and_reused_by_the_backward(dev, monkeypatch):
    """(f)"""
    from madeleine_amd import functional as MF
    model = _model(dev, 4, False)
    feats = t((2, 2, 160, D_IN), "drophash:feats").to(dev)
    rec = _Seeds(MF.new_dropout_seed)
    monkeypatch.setattr(MF, "new_dropout_seed", rec)

    def forward():
        embs, toks = model({"feats": feats}, device=dev, train=True)
        return sum(e.square().sum() for e in embs.values()) + sum(x.sum() for x in toks.values())

    torch.manual_seed(3)
    loss = forward()
    first = list(rec.drawn)
    assert len(first) == 4 and len(set(first)) == 4, "one seed per dropout site: three blocks and the gates"
    assert all(isinstance(s, int) and 0 <= s < 2 ** 64 for s in first)
    loss.backward()
    torch.cuda.synchronize()
    assert rec.drawn == first, "the backward reuses the forward's seeds"
    forward()
    second = rec.drawn[4:]
    assert len(second) == 4 and not set(second) & set(first), "a second forward draws new ones"
    torch.manual_seed(3)
    del rec.drawn[:]
    forward()
    forward()
    assert rec.drawn == first + second, "torch.manual_seed fixes the list"
    model.eval()
    del rec.drawn[:]
    with torch.no_grad():
        model({"feats": feats}, device=dev, train=True)
        model({"feats": feats[:, :1]}, device=dev, train=False)
    assert rec.drawn == [], "eval mode draws none"
