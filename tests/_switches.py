"""The library's behaviour switches for the tests (include/madeleine_amd.h, "Behaviour switches"): the defaults as INTEGRATION.md documents
them, written out by hand, and a fixture that sets a switch process-wide for one test."""
import pytest

# environment name -> (kind, default)
SWITCHES = {
    "MADELEINE_INFONCE_FUSED": ("presence", 0),
    "MADELEINE_BF16_GATE128": ("presence", 0),
    "MADELEINE_DROP_16BIT": ("presence", 0),
    "MADELEINE_GOT_NO192": ("presence", 0),
    "MADELEINE_GOT_NOSPLIT": ("presence", 0),
    "MADELEINE_GOT_NO_HALF_PRODUCTS": ("presence", 0),
    "MADELEINE_BF16_GATE_PERSIST": ("integer", 1),
    "MADELEINE_GATE_PERSIST": ("integer", 0),
    "MADELEINE_BF16_LIN_PERSIST": ("integer", 1),
    "MADELEINE_BF16_LIN256_MINK": ("integer", 512),
    "MADELEINE_BF16_TN256": ("integer", 1),
    "MADELEINE_SPLIT_TOKENS": ("integer", 32768),
    "MADELEINE_SP_NT_STAGES": ("integer", 3),
    "MADELEINE_SP_TN_STAGES": ("integer", 3),
    "MADELEINE_BF16_STAGES": ("integer", 3),
    "MADELEINE_BF16_LIN_STAGES": ("integer", 31),
}


def non_default():
    """{name: value} of the switches that the calling thread sees away from their defaults."""
    from madeleine_amd import _native
    return {n: _native.switch_get(n) for n, (_, d) in SWITCHES.items() if _native.switch_get(n) != d}


@pytest.fixture
def switch():
    """switch(name, value): mdl_switch_set for the rest of the test; every switch it touched gets its earlier value back afterwards."""
    from madeleine_amd import _native
    was = {}

    def set_(name, value):
        was.setdefault(name, _native.switch_get(name))
        _native.switch_set(name, value)

    yield set_
    for name, value in was.items():
        _native.switch_set(name, value)
