"""Host-side checks of the two-stream attention entry points (no GPU needed)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    return ctypes.CDLL(hip.LIB_PATH)


def test_attn2_symbols_are_declared_and_exported(lib):
    from peneo_amd import hip
    for name in ("peneo_attn2_supported", "peneo_attn2_fwd"):
        assert name in hip.SIGNATURES
        assert hasattr(lib, name)
    assert lib.peneo_version() >= 103


def test_attn2_support_query_accepts_lilt_widths(lib):
    from peneo_amd import hip
    assert lib.peneo_attn2_supported(hip.BF16, 64, 16) == 1


@pytest.mark.parametrize("dtype,d_a,d_b", [("F32", 64, 16), ("BF16", 48, 12), ("BF16", 80, 0), ("BF16", 64, 32), ("BF16", 0, 16),
                                           ("BF16", -64, 16)])
def test_attn2_support_query_refuses_everything_else(lib, dtype, d_a, d_b):
    from peneo_amd import hip
    assert lib.peneo_attn2_supported(getattr(hip, dtype), d_a, d_b) == 0
