"""Host-side checks of the MXFP8 pair-heads entry points (no GPU needed)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    return ctypes.CDLL(hip.LIB_PATH)


def test_mxfp8_symbols_are_declared_and_exported(lib):
    from peneo_amd import hip
    for name in ("peneo_mxfp8_quantize_rows", "peneo_pair_mxfp8_supported", "peneo_pair_heads_mxfp8_packed_bytes",
                 "peneo_pair_heads_pack_mxfp8", "peneo_pair_heads_fwd_mxfp8"):
        assert name in hip.SIGNATURES
        assert hasattr(lib, name)
    assert lib.peneo_version() >= 101


def test_mxfp8_support_query_accepts_the_shipped_widths(lib):
    assert lib.peneo_pair_mxfp8_supported(384, 5) == 1
    assert lib.peneo_pair_mxfp8_supported(512, 5) == 1


@pytest.mark.parametrize("D,nh", [(96, 5), (400, 5), (1024, 5), (0, 5), (384, 0), (384, 9), (-64, 5)])
def test_mxfp8_support_query_refuses_what_the_kernel_cannot_hold(lib, D, nh):
    assert lib.peneo_pair_mxfp8_supported(D, nh) == 0
    lib.peneo_pair_heads_mxfp8_packed_bytes.restype = ctypes.c_size_t
    assert lib.peneo_pair_heads_mxfp8_packed_bytes(nh, D) == 0
