"""CPU-only checks of the product's host side: the C-ABI library loads and exports every symbol the
header declares (no compute calls), module construction / state_dict contract, argument validation,
the calculate_losses host logic (with the oracle's loss callables injected), and loud failure on CPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from oracle import restatement as R
from tests._util import MODS5, ROOT, golden, t


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "madeleine_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mdl_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    from madeleine_amd import _native
    names = _header_symbols()
    assert len(names) >= 14
    assert set(names) == set(_native.SIGNATURES), (set(names) ^ set(_native.SIGNATURES))
    lib = _native.lib()                       # builds with hipcc if missing; raises if impossible
    raw = ctypes.CDLL(_native.lib_path())
    for n in names:
        assert hasattr(raw, n), n
    assert b"gfx950" in lib.mdl_version()
    # host-only queries are safe without a GPU
    assert lib.mdl_abmil_gate_fwd_ws_bytes(1000, 4) >= 1000 * 4 * 4 * 4
    assert lib.mdl_abmil_pool_ws_bytes(64, 4096, 4) >= 64 * 32 * 2048 * 4
    assert lib.mdl_infonce_ws_bytes(4, 32, 512) > 0
    assert lib.mdl_abmil_gate_fwd_ws_bytes(-1, 4) < 0 and lib.mdl_abmil_pool_ws_bytes(1, 1, 99) < 0


def test_derived_signatures_equal_hand_written_ones():
    """The binding is parsed from the header; these six are typed here by hand from the same declarations.  Between them: every scalar
    type (int, int64_t, uint64_t, uint32_t, float), pointers of every kind, the char* return and (void)."""
    from madeleine_amd import _native
    p, i32, i64, u32, u64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
    expected = {
        "mdl_version": (ctypes.c_char_p, []),
        "mdl_abmil_gate_fwd": (i32, [p, i64, p, p, p, p, p, p, p, p, p, i64, i32, f32, u64, p, p, p, p]),
        "mdl_split_gemm_nt": (i32, [p, i64, p, p, i64, p, p, i64, i64, i32, i32, p, i32, p, p, p, p, i32, p]),
        "mdl_got_tiled_rect_fwd": (i32, [p, p, p, p, p, i32, i32, i32, i32, p, p]),
        "mdl_stream_create_cu_mask": (i32, [u32, p, p]),
        "mdl_dispatch_plan": (i32, [i32, i64, i32, i32, i32, p, i32]),
        "mdl_abmil_gate_fwd_ws_bytes": (i64, [i64, i32]),
    }
    for name, (res, args) in expected.items():
        got_res, got_args = _native.SIGNATURES[name]
        assert got_res is res and got_args == args, name


@pytest.mark.parametrize("text, message", [
    ("int mdl_a(const float* x, size_t n);", "unknown type 'size_t n' in the declaration of mdl_a"),
    ("double mdl_a(int n);", "unknown type 'double' in the declaration of mdl_a"),
    ("void* mdl_a(int n);", "unknown type 'void*' in the declaration of mdl_a"),
    ("int mdl_a(int);", "unknown type 'int' in the declaration of mdl_a"),
    ("int mdl_a(const float*);", "unknown type 'const float*' in the declaration of mdl_a"),
    ("int mdl_a(int n, const float *);", "unknown type 'const float *' in the declaration of mdl_a"),
    ("int mdl_a(float x[4]);", "unknown type 'float x[4]' in the declaration of mdl_a"),
    ("int mdl_a(int64_t int);", "unknown type 'int64_t int' in the declaration of mdl_a"),
    ("int mdl_a(int n);\nint mdl_b(void);\nint mdl_a(int n);", "declares mdl_a twice"),
    ("int mdl_a(int n, float x;\nint mdl_b(void);", "cannot read the header declaration 'int mdl_a(int n, float x'"),
    ("int mdl_a(int n) { return n; }", "cannot read the header declaration"),
    ("/* int mdl_a(int n); */\n#define MDL_ABI_VERSION 26\n", "declares no entry point"),
    ("", "declares no entry point"),
])
def test_header_parser_is_strict(text, message):
    """A header the parser cannot read completely is an error that names the declaration -- never a guessed type."""
    from madeleine_amd import _native
    with pytest.raises(ValueError, match=re.escape(message)):
        _native._parse_header(text)


def test_header_parser_reads_what_it_should():
    from madeleine_amd import _native
    sigs, defines = _native._parse_header(
        "#ifdef __cplusplus\nextern \"C\" {\n#endif\n#define MDL_E_X (-7) /* why */\n#define MDL_N 3\n"
        "/* int mdl_gone(int n); */\nconst char* mdl_v(void);\nint64_t mdl_w(const float* const* V, void** out,\n"
        "              uint64_t seed, float p);\n#ifdef __cplusplus\n}\n#endif\n")
    assert sigs == {"mdl_v": (ctypes.c_char_p, []),
                    "mdl_w": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_float])}
    assert defines == {"MDL_E_X": -7, "MDL_N": 3}


def test_constants_come_from_the_header_defines():
    """ABI_VERSION, the error codes, PLAN_PRODUCTS and the PLAN_FIELDS indices against this test's own reading of the #defines."""
    from madeleine_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "madeleine_amd.h")).read(), flags=re.S)
    defs = {k: int(v.strip("()")) for k, v in re.findall(r"^#define\s+(MDL_\w+)\s+(\(?-?\d+\)?)\s*$", src, flags=re.M)}
    assert _native.ABI_VERSION == defs["MDL_ABI_VERSION"] == 26
    errs = {k: v for k, v in defs.items() if k.startswith("MDL_E_")}
    assert sorted(_native._ERR) == sorted(errs.values()) == [-3, -2, -1]
    for k, v in errs.items():
        assert _native._ERR[v].startswith(k)
        with pytest.raises(RuntimeError, match=k):
            _native.check(v, "mdl_x")
    assert _native._E_UNSUPPORTED == defs["MDL_E_UNSUPPORTED"]
    assert defs["MDL_PLAN_FIELDS"] == len(_native.PLAN_FIELDS) == 7
    for i, f in enumerate(_native.PLAN_FIELDS):
        assert defs["MDL_PLAN_" + f.upper()] == i
    fields = {"MDL_PLAN_" + f.upper() for f in _native.PLAN_FIELDS} | {"MDL_PLAN_FIELDS"}
    products = {k[len("MDL_PLAN_"):].lower(): v for k, v in defs.items() if k.startswith("MDL_PLAN_") and k not in fields}
    assert _native.PLAN_PRODUCTS == products and len(products) == 13
    assert _native.PLAN_PRODUCTS["gate_fp32_bwd"] == 1 and _native.PLAN_PRODUCTS["got_tiled_rect"] == 13


def _cfg(mods, d_in=64):
    return SimpleNamespace(MODALITIES=list(mods), wsi_encoder="abmil", patch_embedding_dim=d_in,
                           wsi_encoder_hidden_dim=512, activation="softmax", n_heads=4)


@pytest.mark.parametrize("stain_encoding", [False, True])
def test_state_dict_contract(stain_encoding):
    from madeleine_amd import MADELEINE
    m = MADELEINE(_cfg(MODS5, 512), stain_encoding=stain_encoding)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == R.param_shapes(5, 512, 4, stain_encoding)
    n = sum(p.numel() for p in m.parameters())
    assert n == (4_996_740 + 16_544 if stain_encoding else 4_996_740)   # SURVEY.md section 8(a) row A0 [probed]


@pytest.mark.parametrize("H", [1, 2, 8])
def test_state_dict_contract_other_head_counts(H):
    """MADELEINE(n_heads=H) has the reference's state_dict keys, order and shapes (heads.npz holds the reference's list)."""
    from madeleine_amd import MADELEINE
    g = golden("heads")
    M, D = int(g["shape"][1]), int(g["shape"][3])
    cfg = _cfg(MODS5[:M], D)
    cfg.n_heads = H
    shapes = [(k, tuple(v.shape)) for k, v in MADELEINE(cfg).state_dict().items()]
    ref = [(str(k), tuple(int(d) for d in s if d >= 0)) for k, s in zip(g[f"h{H}/state_keys"], g[f"h{H}/state_shapes"])]
    assert shapes == ref
    assert dict(shapes) == R.param_shapes(M, D, H)


@pytest.mark.parametrize("H", [3, 16])
def test_unsupported_head_counts_raise_at_construction(H):
    """The kernels are instantiated for 1, 2, 4 and 8 heads: any other count fails when the model is built, naming those values."""
    from madeleine_amd import MADELEINE
    from madeleine_amd.model import ABMILEmbedder
    cfg = _cfg(MODS5[:2])
    cfg.n_heads = H
    with pytest.raises(ValueError, match=r"n_heads must be one of \(1, 2, 4, 8\)"):
        MADELEINE(cfg)
    with pytest.raises(ValueError, match="got %d" % H):
        ABMILEmbedder({"input_dim": 64, "hidden_dim": 512},
                      {"model": "ABMIL", "params": {"input_dim": 512, "hidden_dim": 512, "dropout": True, "activation": "softmax",
                                                    "n_heads": H, "n_classes": 1}})


def test_no_cpu_fallback_and_errors():
    from madeleine_amd import BatchedABMIL, InfoNCE, MADELEINE
    m = MADELEINE(_cfg(MODS5[:2]))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m({"feats": torch.zeros(1, 2, 8, 64)}, "cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        InfoNCE()(torch.zeros(4, 32), torch.zeros(4, 32))
    with pytest.raises(NotImplementedError):
        BatchedABMIL(input_dim=1024, hidden_dim=256)(torch.zeros(1, 4, 1024))
    bad = _cfg(MODS5[:2])
    bad.wsi_encoder = "vit"
    with pytest.raises(ValueError):
        MADELEINE(bad)
    crit = InfoNCE()
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4), torch.zeros(3, 4))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4), torch.zeros(2, 8))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(2, 3, 4))


def test_calculate_losses_host_logic_against_golden():
    """Our calculate_losses (host logic) with the ORACLE's loss callables reproduces the reference's numbers:
    mask/gate logic, [global, local] order, local weight, k<=1 skip, sentinel."""
    from madeleine_amd import calculate_losses
    g = golden("calculate_losses")
    B, M, N = 6, 5, 12
    stains = MODS5[1:]
    he_e, he_t = t((B, 1, 512), "cl:he_e"), t((B, N, 128), "cl:he_t")
    wsi = {"HE": he_e.unsqueeze(3).repeat(1, 1, 1, M - 1)}
    tok = {"HE": he_t.unsqueeze(3).repeat(1, 1, 1, M - 1)}
    for s in stains:
        wsi[s] = t((B, 1, 512), f"cl:e{s}") + 0.1 * he_e
        tok[s] = t((B, N, 128), f"cl:t{s}") + 0.6 * he_t
    labels = torch.from_numpy(g["labels"])
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=0.7)
    nce = lambda query, positive_key, symmetric=False: R.info_nce(query, positive_key, 0.001, symmetric)  # noqa: E731
    torch.manual_seed(5)
    loss, flag = calculate_losses(stains, nce, R.got, None, wsi, tok, labels[:, 1:], args)
    assert flag and abs(float(loss) - float(g["full/loss"])) < 1e-5 * abs(float(g["full/loss"]))
    l0 = torch.zeros(B, M)
    l0[:, 0] = 1
    l0[2, 3] = 1
    loss_s, flag_s = calculate_losses(stains, nce, R.got, None, wsi, tok, l0[:, 1:], args)
    assert loss_s == -1 and flag_s is False


def test_utils_mirror():
    from madeleine_amd.utils import set_model_precision, smooth_rank_measure
    assert set_model_precision("bfloat16") is torch.bfloat16 and set_model_precision("float32") is torch.float32
    with pytest.raises(ValueError):
        set_model_precision("int8")
    r = smooth_rank_measure(torch.eye(8))
    assert abs(r - 8.0) < 0.05


def test_checkpoint_and_pretrained_dir_round_trip(tmp_path):
    """N3 host glue: load_checkpoint (utils.py:92-121, incl. a DataParallel-style 'module.' state dict) and
    create_model_from_pretrained on a local checkpoint directory (factory.py:29-41: model_config.json + model.pt)."""
    import json
    from types import SimpleNamespace
    from madeleine_amd import MADELEINE, create_model_from_pretrained, load_checkpoint
    cfgd = dict(MODALITIES=["HE", "ER"], wsi_encoder="abmil", patch_embedding_dim=64, wsi_encoder_hidden_dim=512,
                activation="softmax", n_heads=4, precision="bfloat16")
    src = MADELEINE(SimpleNamespace(**cfgd))
    torch.save({"module." + k: v for k, v in src.state_dict().items()}, tmp_path / "model.pt")
    (tmp_path / "model_config.json").write_text(json.dumps(cfgd))
    dst = load_checkpoint(SimpleNamespace(RESULS_SAVE_PATH=str(tmp_path)), MADELEINE(SimpleNamespace(**cfgd)))
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    model, precision = create_model_from_pretrained(str(tmp_path), device="cpu")
    assert precision is torch.bfloat16
    for k, v in src.state_dict().items():
        assert torch.equal(v, model.state_dict()[k]), k


def test_dataset_collate_contract():
    """N4: item / collate contract of wsi_dataset.py (fixed-N resample, zero bag for an absent stain, stacking)."""
    import pandas as pd
    from madeleine_amd.data import SlideDataset, SyntheticSlideDataset, collate
    df = pd.DataFrame({"slide_id": ["a", "b"], "HE": [1, 1], "ER": [1, 0], "split": ["train", "val"]})
    seen = []

    def loader(path):
        seen.append(path)
        return torch.arange(10 * 4, dtype=torch.float32).view(10, 4) if path.endswith("a_HE.h5") else torch.ones(3, 4)

    ds = SlideDataset("x", None, "/feats", ["HE", "ER"], embedding_size=4, sample=6, feature_loader=loader, dataframe=df)
    a, b = ds[0], ds[1]
    assert [f.shape for f in a["feats"]] == [torch.Size([6, 4])] * 2 and a["modality_labels"] == [1, 1]
    assert len(set(map(tuple, a["feats"][0].tolist()))) == 6            # randperm: no replacement when the bag is long enough
    assert float(b["feats"][1].abs().sum()) == 0.0 and b["feats"][1].shape == (6, 4)   # absent stain -> resampled zero bag
    assert seen == ["/feats/a_HE.h5", "/feats/a_ER.h5", "/feats/b_HE_val.h5"]            # split suffix, absent file not read
    batch = collate([a, b])
    assert batch["feats"].shape == (2, 2, 6, 4) and batch["modality_labels"].tolist() == [[1, 1], [1, 0]]
    assert batch["slide_ids"] == ["a", "b"]
    syn = SyntheticSlideDataset(5, MODS5, 8, 16, seed=1)
    item = syn[3]
    assert len(item["feats"]) == 5 and item["feats"][0].shape == (8, 16) and item["modality_labels"][0] == 1
    for m, lab in enumerate(item["modality_labels"]):
        assert (float(item["feats"][m].abs().sum()) == 0.0) == (lab == 0)


def test_h5_feature_files_without_h5py(tmp_path):
    """N4: `load_features` (wsi_dataset.py:14-19) reads the chunked / resizable `features` datasets save_hdf5 writes
    (conch_patch_embedder.py:16-66) through the ctypes binding of the system's libhdf5, and SlideDataset + collate produce the
    reference's batch contract from real .h5 files (present stain -> file, absent stain -> zero bag, fixed-N resample)."""
    import numpy as np
    import pandas as pd
    from madeleine_amd import h5io
    from madeleine_amd.data import SlideDataset, collate, load_features
    rng = np.random.default_rng(0)
    D = 32
    feats = {("c0", "HE"): rng.standard_normal((50, 1, D)).astype(np.float32),      # [N,1,D]: squeezed by the loader
             ("c0", "ER"): rng.standard_normal((7, D)).astype(np.float32),           # shorter than `sample`: randint resample
             ("c1", "HE"): rng.standard_normal((40, D)).astype(np.float32)}
    for (cid, m), a in feats.items():
        h5io.write_datasets(str(tmp_path / f"{cid}_{m}.h5"), {"features": a, "coords": np.zeros((a.shape[0], 2), np.float32)})
    got = load_features(str(tmp_path / "c0_HE.h5"))
    assert got.dtype == torch.float32 and tuple(got.shape) == (50, D)
    assert torch.equal(got, torch.from_numpy(feats[("c0", "HE")].squeeze()))
    with pytest.raises(KeyError):
        h5io.read_dataset(str(tmp_path / "c0_HE.h5"), "nope")
    df = pd.DataFrame({"slide_id": ["c0", "c1"], "HE": [1, 1], "ER": [1, 0], "split": ["train", "train"]})
    ds = SlideDataset("toy", None, str(tmp_path), ["HE", "ER"], embedding_size=D, sample=16, train=True, dataframe=df)
    torch.manual_seed(0)
    batch = collate([ds[0], ds[1]])
    assert tuple(batch["feats"].shape) == (2, 2, 16, D) and batch["slide_ids"] == ["c0", "c1"]
    assert torch.equal(batch["modality_labels"], torch.tensor([[1.0, 1.0], [1.0, 0.0]]))
    assert float(batch["feats"][1, 1].abs().max()) == 0.0                             # absent stain -> zero bag
    rows = {tuple(r.tolist()) for r in torch.from_numpy(feats[("c0", "ER")])}
    assert all(tuple(r.tolist()) in rows for r in batch["feats"][0, 1])               # resampled rows come from the file


def test_simple_dataset_for_extraction(tmp_path):
    """N3/N4: the extraction-side dataset (wsi_dataset.py:102-125): one item per .h5 file = (features [N,D], slide id), batch 1
    through simple_collate -> the (feats [1,N,D], [slide_id]) pairs run_inference consumes."""
    import numpy as np
    from torch.utils.data import DataLoader
    from madeleine_amd import h5io
    from madeleine_amd.data import SimpleDataset, simple_collate
    rng = np.random.default_rng(1)
    arrs = {"s_b": rng.standard_normal((9, 16)).astype(np.float32), "s_a": rng.standard_normal((5, 1, 16)).astype(np.float32)}
    for k, a in arrs.items():
        h5io.write_datasets(str(tmp_path / f"{k}.h5"), {"features": a})
    (tmp_path / "notes.txt").write_text("not a feature file")
    ds = SimpleDataset(str(tmp_path))
    assert len(ds) == 2
    seen = {}
    for feats, ids in DataLoader(ds, batch_size=1, collate_fn=simple_collate):
        assert feats.dim() == 3 and feats.shape[0] == 1 and len(ids) == 1
        seen[ids[0]] = feats[0]
    assert set(seen) == {"s_a", "s_b"}
    assert torch.equal(seen["s_a"], torch.from_numpy(arrs["s_a"].squeeze())) and torch.equal(seen["s_b"], torch.from_numpy(arrs["s_b"]))



def test_bench_gpus_n_relaunches_itself_under_torchrun():
    """`python bench.py --gpus 2` with no launcher in the environment must start 2 ranks under torch.distributed.run by itself
    (the bare form used to die on a WORLD_SIZE assertion).  Without a GPU every rank then stops at bench.py's own
    'needs a GPU' check -- reached only after the relaunch, the rendezvous and init_process_group(gloo) worked."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MADELEINE_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                        "--no-extra-legs"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    if torch.cuda.is_available():      # (this file also runs on the GPU box: there the two gloo ranks share the GPU and finish)
        assert r.returncode == 0, r.stderr[-2000:]
        return
    assert r.returncode != 0
    assert "WORLD_SIZE" not in r.stderr, r.stderr[-2000:]
    assert r.stderr.count("bench.py needs a GPU") >= 2, r.stderr[-2000:]


def test_bench_compact_line_fits_the_driver_record():
    """BENCH_r05.parsed was null because bench.py printed one 22-KB line and the driver keeps an ~8-KB tail.  The
    contract line is now built by bench.compact_line: <= 4 KB whatever the detail record holds, every contract key + roofline + cpu_baseline
    present.  Fed with round 5's own 22-KB record (profiles/r05fin2_bench_default.json) and with a pathologically bloated one."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    rec = json.load(open(os.path.join(ROOT, "profiles", "r05fin2_bench_default.json")))
    assert len(json.dumps(rec)) > 16000
    rec["dtype_short"], rec["detail_path"] = "f32 (3-term split-fp16 MFMA products, fp32 accumulate)", "gpurun_out/bench_detail.json"
    for bloat in (0, 400):
        r = json.loads(json.dumps(rec))
        for i in range(bloat):    # many more kernel families / legs than any real run has: the optional objects are shed, the contract stays
            r["kernel_roofline"]["k%03d" % i] = {"bound": "hbm", "avg_ms": 1.0, "achieved": 1.0, "unit": "GB/s", "peak": 8000.0, "frac": 0.5}
        r["cpu_baseline"]["sample"] = r["cpu_baseline"]["sample"] * (1 + bloat)
        line = bench.compact_line(r)
        assert len(line) <= bench.COMPACT_MAX == 4096 and "\n" not in line
        out = json.loads(line)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert k in out, k
        assert out["config"]["workload"].startswith("c2:") and "model" not in out["config"]
        assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(out["roofline"])
        assert {"value", "unit", "cores", "kind", "sample"} <= set(out["cpu_baseline"])
        assert ("kernels" in out) == (bloat == 0)


def test_numa_pin_helper_is_harmless_without_topology():
    """distributed.pin_to_gpu_numa: cpulist parsing, and no change of the affinity mask when the GPU / sysfs topology is unavailable."""
    import os
    from madeleine_amd import distributed as DP
    assert DP._parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}
    assert DP._parse_cpulist("") == set()
    before = os.sched_getaffinity(0)
    assert DP.pin_to_gpu_numa(0, sysfs="/nonexistent") is None
    assert os.sched_getaffinity(0) == before
