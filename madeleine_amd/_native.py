"""ctypes binding of libmadeleine_amd.so (the C ABI of include/madeleine_amd.h, include/madeleine_amd_view.h,
include/madeleine_amd_stats.h, include/madeleine_amd_explain.h, include/madeleine_amd_regress.h and include/madeleine_amd_cluster.h).

Single backend: there is no CPU / eager fallback.  `lib()` raises if the shared object cannot be
loaded (it is built in-tree by `python -m madeleine_amd._build` / __graft_entry__.build(); if it is
missing or stale and hipcc is present it is rebuilt once), and every op raises RuntimeError on a
non-zero return code.
"""
import contextlib
import ctypes
import os
import re
import threading

from . import _build

_LOCK = threading.Lock()
_LIB = None

# The header's scalar types; every pointer is passed as an address (c_void_p).  Anything else is an error, never a guess.
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float}
_POINTEES = frozenset(_SCALARS) | {"void", "char", "uint8_t", "uint16_t", "int32_t"}
_DECL = re.compile(r"(?P<ret>[\w\s*]+?)\b(?P<name>\w+)\s*\((?P<args>[^()]*)\)")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)


def _ctype(text, decl, named):
    """ctypes type of one parameter (`named`: the last word is its name) or of a return type."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if named:      # the last word must be the parameter's name: `const float*` or `float x[4]` is not read as a float
        if not (len(words) >= 2 and words[-1].isidentifier() and words[-1] not in _POINTEES):
            raise ValueError("madeleine_amd: unknown type %r in the declaration of %s" % (" ".join(text.split()), decl))
        words = words[:-1]
    if len(words) == 1 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    if named and len(words) >= 2 and words[0] in _POINTEES and set(words[1:]) == {"*"}:
        return ctypes.c_void_p
    if not named and words == ["char", "*"]:      # the version string
        return ctypes.c_char_p
    raise ValueError("madeleine_amd: unknown type %r in the declaration of %s" % (" ".join(text.split()), decl))


def _parse_header(text):
    """(SIGNATURES, integer #defines) of the C header `text`.  Strict: every statement must read as `ret name(args);` with types
    from the tables above, names must be unique and at least one declaration must be found -- a header this cannot read is an
    import error, not a kernel launched with shifted arguments."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2)) for m in _DEFINE.finditer(text)}
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)      # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    sigs = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = _DECL.fullmatch(stmt)
        if m is None:
            raise ValueError("madeleine_amd: cannot read the header declaration %r" % stmt[:80])
        name, args = m.group("name"), m.group("args").strip()
        if name in sigs:
            raise ValueError("madeleine_amd: the header declares %s twice" % name)
        argtypes = [] if args == "void" else [_ctype(a, name, True) for a in args.split(",")]
        sigs[name] = (_ctype(m.group("ret"), name, False), argtypes)
    if not sigs:
        raise ValueError("madeleine_amd: the header declares no entry point")
    return sigs, defines


# name -> (restype, argtypes), and the header's integer #defines: include/madeleine_amd.h is the only source of both
with open(_build.HEADER) as _f:
    SIGNATURES, _DEFINES = _parse_header(_f.read())
ABI_VERSION = _DEFINES["MDL_ABI_VERSION"]
# the second header (include/madeleine_amd_view.h: the heatmap entry points) is read the same way into a table of its own: SIGNATURES
# stays exactly the main header's set, and the revision above is the main header's alone
with open(_build.VIEW_HEADER) as _f:
    VIEW_SIGNATURES, VIEW_DEFINES = _parse_header(_f.read())
if set(VIEW_SIGNATURES) & set(SIGNATURES) or set(VIEW_DEFINES) & set(_DEFINES):
    raise ImportError("madeleine_amd: %s repeats a name of %s" % (_build.VIEW_HEADER, _build.HEADER))
# the third header (include/madeleine_amd_stats.h: the bootstrap entry points), the same way: a table of its own, no name of the other two
with open(_build.STATS_HEADER) as _f:
    STATS_SIGNATURES, STATS_DEFINES = _parse_header(_f.read())
if (set(STATS_SIGNATURES) & (set(SIGNATURES) | set(VIEW_SIGNATURES))) or (set(STATS_DEFINES) & (set(_DEFINES) | set(VIEW_DEFINES))):
    raise ImportError("madeleine_amd: %s repeats a name of %s or %s" % (_build.STATS_HEADER, _build.HEADER, _build.VIEW_HEADER))
# the fourth header (include/madeleine_amd_explain.h: the patch contributions of a probe's decision), the same way again
with open(_build.EXPLAIN_HEADER) as _f:
    EXPLAIN_SIGNATURES, EXPLAIN_DEFINES = _parse_header(_f.read())
if (set(EXPLAIN_SIGNATURES) & (set(SIGNATURES) | set(VIEW_SIGNATURES) | set(STATS_SIGNATURES))) or \
        (set(EXPLAIN_DEFINES) & (set(_DEFINES) | set(VIEW_DEFINES) | set(STATS_DEFINES))):
    raise ImportError("madeleine_amd: %s repeats a name of %s, %s or %s"
                      % (_build.EXPLAIN_HEADER, _build.HEADER, _build.VIEW_HEADER, _build.STATS_HEADER))
# the fifth header (include/madeleine_amd_regress.h: the regression probe), the same way again: no name of the other four
with open(_build.REGRESS_HEADER) as _f:
    REGRESS_SIGNATURES, REGRESS_DEFINES = _parse_header(_f.read())
if (set(REGRESS_SIGNATURES) & (set(SIGNATURES) | set(VIEW_SIGNATURES) | set(STATS_SIGNATURES) | set(EXPLAIN_SIGNATURES))) or \
        (set(REGRESS_DEFINES) & (set(_DEFINES) | set(VIEW_DEFINES) | set(STATS_DEFINES) | set(EXPLAIN_DEFINES))):
    raise ImportError("madeleine_amd: %s repeats a name of the other four headers" % _build.REGRESS_HEADER)
# the sixth header (include/madeleine_amd_cluster.h: k-means over the slide store), the same way again: no name of the other five
with open(_build.CLUSTER_HEADER) as _f:
    CLUSTER_SIGNATURES, CLUSTER_DEFINES = _parse_header(_f.read())
if (set(CLUSTER_SIGNATURES) & (set(SIGNATURES) | set(VIEW_SIGNATURES) | set(STATS_SIGNATURES) | set(EXPLAIN_SIGNATURES) |
                               set(REGRESS_SIGNATURES))) or \
        (set(CLUSTER_DEFINES) & (set(_DEFINES) | set(VIEW_DEFINES) | set(STATS_DEFINES) | set(EXPLAIN_DEFINES) | set(REGRESS_DEFINES))):
    raise ImportError("madeleine_amd: %s repeats a name of the other five headers" % _build.CLUSTER_HEADER)


def lib_path() -> str:
    return _build.LIB


def lib():
    """Load (once) and return the ctypes handle.  Raises RuntimeError if unavailable."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        override = os.environ.get("MADELEINE_LIB")   # a library built elsewhere (A/B of two builds); the ABI check below still applies
        path = override or lib_path()
        if not override and not _build.is_fresh():
            try:
                _build.build()
            except _build.HipccMissing as e:
                # no compiler on this machine: a prebuilt library may still be used, guarded by the ABI check below
                if not os.path.exists(path):
                    raise RuntimeError(
                        "madeleine_amd: libmadeleine_amd.so is missing and could not be built (%s). "
                        "There is no fallback path: run `python -m madeleine_amd._build`." % e) from e
            except Exception as e:
                # sources newer than the library and the rebuild FAILED: never dlopen the stale object -- its entry points
                # would be called with this file's (newer) signatures
                raise RuntimeError("madeleine_amd: libmadeleine_amd.so is stale and the rebuild failed: %s" % e) from e
        try:
            handle = ctypes.CDLL(path)
        except OSError as e:
            raise RuntimeError("madeleine_amd: cannot load %s: %s" % (path, e)) from e
        try:
            abi = handle.mdl_abi_version
        except AttributeError:
            raise RuntimeError("madeleine_amd: %s predates the ABI-version check; rebuild it "
                               "(`python -m madeleine_amd._build --force`)" % path) from None
        abi.restype, abi.argtypes = SIGNATURES["mdl_abi_version"]
        if abi() != ABI_VERSION:
            raise RuntimeError("madeleine_amd: %s implements ABI revision %d, this binding expects %d; rebuild it "
                               "(`python -m madeleine_amd._build --force`)" % (path, abi(), ABI_VERSION))
        for name, (res, args) in list(SIGNATURES.items()) + list(VIEW_SIGNATURES.items()) + list(STATS_SIGNATURES.items()) + \
                list(EXPLAIN_SIGNATURES.items()) + list(REGRESS_SIGNATURES.items()) + list(CLUSTER_SIGNATURES.items()):
            try:
                fn = getattr(handle, name)
            except AttributeError:
                raise RuntimeError("madeleine_amd: %s does not export %s (header / library mismatch)" % (path, name)) from None
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
        return _LIB


_E_UNSUPPORTED = _DEFINES["MDL_E_UNSUPPORTED"]
_ERR_TEXT = {"MDL_E_ARG": "MDL_E_ARG (bad size / null pointer)", "MDL_E_ALIGN": "MDL_E_ALIGN (pointer not 16-byte aligned)"}
_ERR = {v: _ERR_TEXT.get(k, k) for k, v in _DEFINES.items() if k.startswith("MDL_E_")}


def check(rc: int, what: str):
    if rc != 0:
        msg = _ERR.get(rc, "hipError_t %d" % rc)
        raise RuntimeError("madeleine_amd: %s failed: %s" % (what, msg))


# mdl_dispatch_plan: the fields of an answer, in the order of their MDL_PLAN_<FIELD> indices, and the products (every other MDL_PLAN_*)
PLAN_FIELDS = ("variant", "persist", "splits", "tps", "empty", "chunk", "extra")
if _DEFINES["MDL_PLAN_FIELDS"] != len(PLAN_FIELDS) or any(_DEFINES["MDL_PLAN_" + f.upper()] != i for i, f in enumerate(PLAN_FIELDS)):
    raise ImportError("madeleine_amd: PLAN_FIELDS does not match the MDL_PLAN_* field indices of %s" % _build.HEADER)
PLAN_PRODUCTS = {k[len("MDL_PLAN_"):].lower(): v for k, v in _DEFINES.items()
                 if k.startswith("MDL_PLAN_") and k[len("MDL_PLAN_"):].lower() not in PLAN_FIELDS + ("fields",)}


def dispatch_plan(product: str, T: int, a: int, b: int = 0, cus: int = 256) -> dict:
    """What the launcher of `product` chooses for T tokens (GOT: T = cases) and sizes a, b on a device of `cus` compute units: a dict
    over PLAN_FIELDS.  Host only (no device needed)."""
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    check(lib().mdl_dispatch_plan(PLAN_PRODUCTS[product], T, a, b, cus, ctypes.addressof(out), len(PLAN_FIELDS)),
          "mdl_dispatch_plan(%s, T=%d, %d, %d)" % (product, T, a, b))
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


# The library's behaviour switches (include/madeleine_amd.h, "Behaviour switches"), by their environment names.  The library reads the
# environment once, at its first use; these calls are how a switch changes afterwards.
SWITCH_COUNT = _DEFINES["MDL_SW_COUNT"]
_SWITCH_IDS = {}


def switch_names() -> tuple:
    """The environment names of the switches, in the order of their ids."""
    return tuple(lib().mdl_switch_name(i).decode() for i in range(SWITCH_COUNT))


def _switch_id(name: str) -> int:
    if not _SWITCH_IDS:
        _SWITCH_IDS.update({n: i for i, n in enumerate(switch_names())})
    try:
        return _SWITCH_IDS[name]
    except KeyError:
        raise KeyError("madeleine_amd: %r is not a library switch (%s)" % (name, ", ".join(_SWITCH_IDS))) from None


def switch_get(name: str) -> int:
    """The value the calling thread's launches see: its override if it holds one, the process value otherwise."""
    out = ctypes.c_int64()
    check(lib().mdl_switch_get(_switch_id(name), ctypes.addressof(out)), "mdl_switch_get(%s)" % name)
    return out.value


def switch_set(name: str, value: int) -> None:
    """Set the process value (every thread without an override of its own sees it from its next launch on)."""
    check(lib().mdl_switch_set(_switch_id(name), int(value)), "mdl_switch_set(%s)" % name)


@contextlib.contextmanager
def switch_override(name: str, value: int):
    """Within the block the launches the calling thread issues see `value`; other threads and the process value are untouched -- autograd's
    device thread included, which issues the launches of a `.backward()`.  The exit clears the thread's override: blocks for one switch do
    not nest."""
    sid = _switch_id(name)
    check(lib().mdl_switch_set_thread(sid, int(value)), "mdl_switch_set_thread(%s)" % name)
    try:
        yield
    finally:
        check(lib().mdl_switch_clear_thread(sid), "mdl_switch_clear_thread(%s)" % name)
