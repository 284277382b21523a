"""The library's switch table (include/madeleine_amd.h, "Behaviour switches"; csrc/switches.hip) without a GPU: ids and names, the one
read of the environment at first use with the parsing the scattered getenv sites had, the process-wide setter against a start with the
variable, the per-thread override, and distributed._fan_out leaving the environment alone.  A child here is a fresh interpreter that
loads the shared object with ctypes alone (no torch), so that its first access to the table happens under the environment it was given."""
import ctypes
import json
import os
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor
from unittest import mock

import pytest

from madeleine_amd import _native
from tests._switches import SWITCHES, switch  # noqa: F401  (switch: a fixture)

E_ARG = -1
TEXTS = (None, "", "0", "00", "1", "2", "abc")      # None: the variable does not exist
GOT_PLAN = ("got", 64, 193, 0)                      # 64 cases of n = 193 on 256 CUs: split sweeps 2 (2k and 4k workgroups fit), 0 when off

# argv: library, then `product T a b` groups.  Prints {"switches": {name: value}, "plans": [[7 fields], ...]}.
CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.mdl_switch_name.restype = ctypes.c_char_p
lib.mdl_switch_get.argtypes = [ctypes.c_int, ctypes.c_void_p]
lib.mdl_dispatch_plan.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
values, i, v = {}, 0, ctypes.c_int64()
while lib.mdl_switch_name(i):
    assert lib.mdl_switch_get(i, ctypes.addressof(v)) == 0
    values[lib.mdl_switch_name(i).decode()] = v.value
    i += 1
plans, out, a = [], (ctypes.c_int64 * 7)(), [int(x) for x in sys.argv[2:]]
for j in range(0, len(a), 4):
    assert lib.mdl_dispatch_plan(a[j], a[j + 1], a[j + 2], a[j + 3], 256, ctypes.addressof(out), 7) == 0
    plans.append(list(out))
print(json.dumps({"switches": values, "plans": plans}))
"""


def _child(env_changes, plans=()):
    """A fresh process with `env_changes` ({name: text, or None for absent}) on top of an environment that names no library switch."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for k, v in env_changes.items():
        if v is not None:
            env[k] = v
    args = [str(x) for p in plans for x in (_native.PLAN_PRODUCTS[p[0]],) + tuple(p[1:])]
    _native.lib()      # (built, if it was not)
    r = subprocess.run([sys.executable, "-c", CHILD, os.environ.get("MADELEINE_LIB") or _native.lib_path()] + args, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def _plan_fields(p):
    return [_native.dispatch_plan(p[0], p[1], p[2], p[3])[f] for f in _native.PLAN_FIELDS]


def test_ids_and_names():
    lib = _native.lib()
    names = [lib.mdl_switch_name(i) for i in range(_native.SWITCH_COUNT)]
    assert all(names) and len(set(names)) == len(names)
    assert sorted(n.decode() for n in names) == sorted(SWITCHES) and tuple(n.decode() for n in names) == _native.switch_names()
    out = ctypes.c_int64(-5)
    for bad in (-1, _native.SWITCH_COUNT, 1 << 20):
        assert lib.mdl_switch_name(bad) is None
        assert lib.mdl_switch_get(bad, ctypes.addressof(out)) == E_ARG and out.value == -5
        assert lib.mdl_switch_set(bad, 1) == E_ARG and lib.mdl_switch_set_thread(bad, 1) == E_ARG and lib.mdl_switch_clear_thread(bad) == E_ARG
    assert lib.mdl_switch_get(0, None) == E_ARG
    with pytest.raises(KeyError):
        _native.switch_get("MADELEINE_GEMM")      # read in Python: not a library switch


def _expected(kind, default, text):
    """The rules, by hand: presence = the variable exists; integer = atoll(text) when it exists ("" and "abc" give 0), else the default."""
    if kind == "presence":
        return 0 if text is None else 1
    return default if text is None else {"": 0, "0": 0, "00": 0, "1": 1, "2": 2, "abc": 0}[text]


def test_read_at_start_keeps_the_old_parsing():
    """One fresh process per (variable, text): the variable reads by its kind's rule, every other switch keeps its default."""
    defaults = {n: d for n, (_, d) in SWITCHES.items()}
    assert _child({})["switches"] == defaults
    cases = [(n, text) for n in SWITCHES for text in TEXTS if text is not None]
    with ThreadPoolExecutor(max_workers=8) as ex:
        got = list(ex.map(lambda c: _child({c[0]: c[1]})["switches"], cases))
    for (name, text), values in zip(cases, got):
        kind, default = SWITCHES[name]
        assert values == dict(defaults, **{name: _expected(kind, default, text)}), (name, text)


@pytest.mark.parametrize("name,text,value,plan,field,changed,pinned", [
    ("MADELEINE_BF16_TN256", "0", 0, ("linear_bf16_bwd", 16384, 256, 512), "variant", 128, 256),
    ("MADELEINE_SPLIT_TOKENS", "4096", 4096, ("gate_split_bwd", 262144, 4, 0), "splits", 64, 8),
    ("MADELEINE_GOT_NOSPLIT", "", 1, GOT_PLAN, "extra", 0, 2),
], ids=["BF16_TN256", "SPLIT_TOKENS", "GOT_NOSPLIT"])
def test_start_up_value_equals_setter_value(switch, name, text, value, plan, field, changed, pinned):
    """A process started with the variable plans what this one plans after switch_set to the same value; back at the default the plan is
    the one tests/test_dispatch_plan_cpu.py pins."""
    at_start = _child({name: text}, [plan])
    assert at_start["switches"][name] == value
    index = _native.PLAN_FIELDS.index(field)
    for n, (_, default) in SWITCHES.items():
        switch(n, default)
    assert _plan_fields(plan)[index] == pinned
    switch(name, value)
    assert _plan_fields(plan) == at_start["plans"][0] and _plan_fields(plan)[index] == changed
    switch(name, SWITCHES[name][1])
    assert _plan_fields(plan)[index] == pinned and _plan_fields(plan) == _child({}, [plan])["plans"][0]


def test_thread_scope(switch):
    name = "MADELEINE_GOT_NOSPLIT"
    extra = lambda: _native.dispatch_plan(*GOT_PLAN[:3], cus=256)["extra"]      # noqa: E731
    switch(name, 0)
    seen = {}

    def other():
        seen["inside"] = (_native.switch_get(name), extra())
        _native.switch_set(name, 7)
        seen["after_set"] = _native.switch_get(name)

    assert extra() == 2
    with _native.switch_override(name, 1):
        assert _native.switch_get(name) == 1 and extra() == 0
        th = threading.Thread(target=other)
        th.start()
        th.join()
        assert seen == {"inside": (0, 2), "after_set": 7}
        assert _native.switch_get(name) == 1 and extra() == 0      # this thread still sees its override
    assert _native.switch_get(name) == 7 and extra() == 0          # the override is gone: the other thread's process-wide value
    switch(name, 0)
    assert extra() == 2


def test_the_environment_is_not_read_again(monkeypatch):
    """The rule: the environment counts once, at the library's first use.  Setting a variable afterwards changes nothing."""
    plan = ("linear_bf16_bwd", 16384, 256, 512)
    before, plan_before = _native.switch_get("MADELEINE_BF16_TN256"), _plan_fields(plan)
    monkeypatch.setenv("MADELEINE_BF16_TN256", "1" if before == 0 else "0")
    assert _native.switch_get("MADELEINE_BF16_TN256") == before and _plan_fields(plan) == plan_before
    monkeypatch.delenv("MADELEINE_BF16_TN256")
    assert _native.switch_get("MADELEINE_BF16_TN256") == before


def test_fan_out_leaves_the_environment_alone(monkeypatch, switch):
    """distributed._fan_out on a (mocked) device: inside, this thread's launches see MADELEINE_GOT_NOSPLIT = 1; os.environ is the same
    bytes before, inside and after, and so is the process value."""
    import torch

    from madeleine_amd import distributed as D
    name = "MADELEINE_GOT_NOSPLIT"
    switch(name, 0)
    monkeypatch.setattr(D, "_SIDE_STREAMS", {})
    for attr in ("Stream", "Event", "current_stream"):
        monkeypatch.setattr(torch.cuda, attr, mock.MagicMock())
    env = dict(os.environb)
    seen = {}
    with D._fan_out("cuda:0", 3) as lanes:
        assert dict(os.environb) == env
        assert _native.switch_get(name) == 1 and _native.dispatch_plan(*GOT_PLAN[:3], cus=256)["extra"] == 0
        th = threading.Thread(target=lambda: seen.update(other=_native.switch_get(name)))
        th.start()
        th.join()
        assert lanes(0) is not None
    assert seen == {"other": 0}
    assert dict(os.environb) == env and _native.switch_get(name) == 0
    with D._fan_out("cpu", 3):                                       # CPU tensors: no fan-out, no override
        assert _native.switch_get(name) == 0
