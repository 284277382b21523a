"""The ways of describing the same gate to the gated-attention kernels agree to the bit (csrc/abmil_gate*.hip, csrc/gate_host.hpp), on
the three engines (fp32, bf16, split), through the C ABI so that every output of an entry point is looked at:
 (i)   a forward with and without saved activations: the same scores;
 (ii)  mdl_abmil_gate_bwd against mdl_abmil_attnpool_bwd with d_pooled == 0 (split: scores == NULL against scores given): the same dE and
       six gradients -- the dX epilogue's fmaf(w, 0, v) is v for a finite softmax weight w (torch.equal takes -0 for +0);
 (iii) mdl_abmil_attnpool_bwd against _phases 1 then 2 on one workspace (split: phases 3 against 1, 4, 8), with a pooling term;
 (iv)  the counter hash against the same call with the masks that mdl_abmil_gate_dropout_mask exports passed as keep_a / keep_b, for both
       field widths of the hash: scores, activations, dE and gradients.
Shapes: T = 1 (less than a tile) and 130 (a full 128-row tile and a tail of 2) with 1 and 4 heads and every dropout mode (off; the
16-bit hash, p = 0.1; the byte hash, p = 0.25; explicit masks); T = 4100 and 16390 with one head and the byte hash, which cross to the
256-row bf16 forward / dX tiles (from 4096 tokens) and to the wide bf16 dW kernel (from 16384) -- asserted through mdl_dispatch_plan.

Levels: measured on the library before gate_host.hpp and the same after: every comparison of (i) - (iv) is equal to the bit at every
shape, engine and mode (1156 whole tensors over the 54 cases; the kernels of a pair differ in a template argument or in the launch
sequence, never in the order of a floating-point operation), so every assertion is torch.equal."""

import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = {"off": 0.0, "hash16": 0.1, "bytes": 0.25, "mask": 0.25}
SEED = 4321
CASES = ([(e, T, H, m) for e in ("fp32", "bf16", "split") for T in (1, 130) for H in (1, 4) for m in MODES] +
         [(e, T, 1, "bytes") for e in ("fp32", "bf16", "split") for T in (4100, 16390)])
GRADS = ("dE", "dWa", "dWb", "dba", "dbb", "dwc", "dbc")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Gate:
    """The gate entry points of one library (lib: a loaded libmadeleine_amd, default the package's) on one engine."""

    def __init__(self, engine, lib=None):
        from madeleine_amd import _native
        self.engine, self.lib = engine, lib if lib is not None else _native.lib()
        self.sfx = {"fp32": "", "bf16": "_bf16", "split": "_split"}[engine]

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
        assert rc == 0, (name, rc)

    def ws(self, query, T, H, dev):
        return torch.empty(max(int(getattr(self.lib, query)(T, H)), 16), dtype=torch.uint8, device=dev)

    def src(self, inp):
        if self.engine == "split":
            img = inp["img"]
            return (img.data, img.K * 4, img.scale)
        return (inp["E"], inp["E"].stride(0))

    def fwd(self, inp, p, keep=(None, None), save=True):
        T, H, dev = inp["T"], inp["H"], inp["E"].device
        stream = torch.cuda.current_stream().cuda_stream
        scores = torch.empty(T, H, device=dev)
        adt = torch.bfloat16 if self.engine == "bf16" else torch.float32
        a, b = (torch.empty(T, H, 512, device=dev, dtype=adt), torch.empty(T, H, 512, device=dev, dtype=adt)) if save else (None, None)
        self.call("mdl_abmil_gate_fwd" + self.sfx, *self.src(inp), inp["Wa"], inp["ba"], inp["Wb"], inp["bb"], inp["wc"], inp["bc"], scores, a,
                  b, T, H, p, SEED, *keep, self.ws("mdl_abmil_gate_fwd%s_ws_bytes" % self.sfx, T, H, dev), stream)
        return dict(scores=scores, act_a=a, act_b=b)

    def bwd(self, inp, act, p, keep=(None, None), pool=None, phases=None):
        """pool = (scores, stat_m, stat_l, d_pooled, row_bag, N) or None; phases: a sequence of masks on one workspace, or None for the
        entry point without phases (split: 3).  -> dE, the six gradients, and dE_absmax on the split engine."""
        T, H, E = inp["T"], inp["H"], inp["E"]
        stream = torch.cuda.current_stream().cuda_stream
        out = dict(dE=torch.empty_like(E), dWa=torch.empty_like(inp["Wa"]), dWb=torch.empty_like(inp["Wb"]), dba=torch.empty_like(inp["ba"]),
                   dbb=torch.empty_like(inp["bb"]), dwc=torch.empty_like(inp["wc"]), dbc=torch.empty_like(inp["bc"]))
        ws = self.ws("mdl_abmil_gate_bwd%s_ws_bytes" % self.sfx, T, H, E.device)
        split = self.engine == "split"
        args = (inp["Wa"], inp["Wb"], inp["wc"], act["act_a"], act["act_b"], inp["ds"], out["dE"]) + ((out["dE"].stride(0),) if split else ()) + (
            0, *[out[k] for k in GRADS[1:]], T, H, p, SEED, *keep)
        if split:
            out["dE_absmax"] = torch.zeros(1, device=E.device)
            for ph in phases or (3,):
                self.call("mdl_abmil_attnpool_bwd_split", *self.src(inp), *args, *(pool or (None,) * 5 + (0,)), out["dE_absmax"], ws, stream, ph, 3)
        elif pool is None:
            assert phases is None
            self.call("mdl_abmil_gate_bwd" + self.sfx, *self.src(inp), *args, ws, stream)
        elif phases is None:
            self.call("mdl_abmil_attnpool_bwd" + self.sfx, *self.src(inp), *args, *pool, ws, stream)
        else:
            for ph in phases:
                self.call("mdl_abmil_attnpool_bwd_phases" + self.sfx, *self.src(inp), *args, *pool, ws, stream, ph)
        return out

    def masks(self, inp, p):
        T, H = inp["T"], inp["H"]
        keep = [torch.empty(T, H, 512, device=inp["E"].device, dtype=torch.uint8) for _ in range(2)]
        for which in (0, 1):
            self.call("mdl_abmil_gate_dropout_mask", keep[which], T, H, which, p, SEED, torch.cuda.current_stream().cuda_stream)
        return tuple(keep)


def make_inputs(dev, engine, T, H, ragged=False):
    """E [T, H*512] in the engine's storage type (split: fp32 and its image), the gate parameters, d_scores, a pooling term over one
    dense bag (ragged: bags of uneven length through row_bag) with its true softmax statistics, and random keep masks."""
    from madeleine_amd import functional as MF
    gen = torch.Generator(device=dev).manual_seed(100 * T + H)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)      # noqa: E731
    E = rnd(T, H * 512).to(torch.bfloat16 if engine == "bf16" else torch.float32)
    inp = dict(T=T, H=H, E=E, Wa=rnd(H, 512, 512) * 0.05, Wb=rnd(H, 512, 512) * 0.05, ba=rnd(H, 512) * 0.1, bb=rnd(H, 512) * 0.1,
               wc=rnd(H, 512) * 0.1, bc=rnd(H) * 0.1, ds=rnd(T, H))
    if engine == "split":
        inp["img"] = MF.split_image(E)
    scores = rnd(T, H)
    if ragged:
        cuts = sorted({0, T} | {int(x) for x in torch.randint(1, T, (3,), device=dev, generator=gen).tolist()})
        row_bag = torch.cat([torch.full((b - a,), i, dtype=torch.int32, device=dev) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))])
        nb, N = len(cuts) - 1, 0
    else:
        row_bag, nb, N = None, 1, T
    bag = row_bag.long() if ragged else torch.zeros(T, dtype=torch.long, device=dev)
    m = torch.full((nb, H), -1e30, device=dev).scatter_reduce(0, bag[:, None].expand(T, H), scores, "amax")
    l = torch.zeros(nb, H, device=dev).index_add_(0, bag, torch.exp(scores - m[bag]))
    inp["pool"] = (scores, m, l, rnd(nb, H * 512), row_bag, N)
    inp["pool0"] = (scores, m, l, torch.zeros(nb, H * 512, device=dev), row_bag, N)
    inp["keep"] = tuple((torch.rand(T, H, 512, device=dev, generator=gen) < 0.75).to(torch.uint8) for _ in range(2))
    return inp


def same(x, y, what):
    for k in x:
        assert (x[k] is None and y[k] is None) or torch.equal(x[k], y[k]), (what, k)
    return len(x)


def run_case(gate, dev, T, H, mode):
    """The comparisons (i) - (iv) on one library; -> the number of tensors compared."""
    inp = make_inputs(dev, gate.engine, T, H)
    p = MODES[mode]
    keep = inp["keep"] if mode == "mask" else (None, None)
    n = 0
    act = gate.fwd(inp, p, keep)
    n += same(dict(scores=act["scores"]), dict(scores=gate.fwd(inp, p, keep, save=False)["scores"]), "(i) saved activations")
    plain = gate.bwd(inp, act, p, keep)
    n += same(plain, gate.bwd(inp, act, p, keep, pool=inp["pool0"]), "(ii) d_pooled == 0")
    whole = gate.bwd(inp, act, p, keep, pool=inp["pool"])
    assert not torch.equal(whole["dE"], plain["dE"]), "the pooling term reaches dE"
    n += same(whole, gate.bwd(inp, act, p, keep, pool=inp["pool"], phases=(1, 4, 8) if gate.engine == "split" else (1, 2)), "(iii) phases")
    if mode in ("hash16", "bytes"):
        masks = gate.masks(inp, p)
        act_m = gate.fwd(inp, p, masks)
        n += same(act, act_m, "(iv) forward, exported masks")
        n += same(whole, gate.bwd(inp, act_m, p, masks, pool=inp["pool"]), "(iv) backward, exported masks")
        kept = float(masks[0].float().mean())
        assert T * H * 512 < 4096 or abs(kept - (1 - p)) < 0.05, kept
    return n


@pytest.mark.parametrize("engine,T,H,mode", CASES, ids=["%s-T%d-H%d-%s" % c for c in CASES])
def test_gate_kinds_agree(dev, engine, T, H, mode):
    from madeleine_amd import _native
    assert mode != "bytes" or not _native.switch_get("MADELEINE_DROP_16BIT"), "the byte-field hash is switched off: p = 0.25 would run the 16-bit one"
    assert run_case(Gate(engine), dev, T, H, mode) > 0


def test_shapes_take_their_kernels():
    """The small shapes run the 128-row bf16 kernels, 4100 tokens the 256-row forward and dX tiles, 16390 the wide dW kernel too."""
    from madeleine_amd import _native
    wide_fwd = not _native.switch_get("MADELEINE_BF16_GATE128")
    wide_dw = _native.switch_get("MADELEINE_BF16_TN256") != 0
    for T in sorted({c[1] for c in CASES}):
        fwd, bwd = _native.dispatch_plan("gate_bf16_fwd", T, 1), _native.dispatch_plan("gate_bf16_bwd", T, 1)
        assert fwd["variant"] == (256 if T >= 4096 and wide_fwd else 128), (T, fwd)
        assert bwd["extra"] == (256 if T >= 4096 else 128), (T, bwd)
        assert bwd["variant"] == (256 if T >= 16384 and wide_dw else 128), (T, bwd)
        assert _native.dispatch_plan("gate_split_bwd", T, 1)["chunk"] == 32 and _native.dispatch_plan("gate_fp32_bwd", T, 1)["chunk"] == 16
