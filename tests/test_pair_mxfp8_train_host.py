"""Host-side checks of the MXFP8 train forward of the pair heads (no GPU needed): exports, signatures, version, support query,
and the block-count parities the GPU tests rely on."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    return ctypes.CDLL(hip.LIB_PATH)


def test_symbols_are_declared_and_exported(lib):
    from peneo_amd import hip
    for name, nargs in (("peneo_pair_mxfp8_save_supported", 2), ("peneo_pair_heads_fwd_mxfp8_save", 9)):
        assert name in hip.SIGNATURES
        assert len(hip.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    # the loaded library carries the ctypes signatures
    fn = hip.lib().peneo_pair_heads_fwd_mxfp8_save
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert len(hip.lib().peneo_pair_mxfp8_save_supported.argtypes) == 2
    assert lib.peneo_version() >= 105


def test_python_entry_points_exist():
    from peneo_amd import ops
    from peneo_amd.model import PEneoModel
    assert callable(ops.pair_mxfp8_save_supported) and callable(ops.pair_heads_fwd_mxfp8_save)
    assert callable(PEneoModel.set_pair_heads_train_format)


@pytest.mark.parametrize("D,nh,want", [(384, 5, 1), (512, 5, 0), (320, 5, 0), (384, 0, 0)])
def test_support_query(lib, D, nh, want):
    assert lib.peneo_pair_mxfp8_save_supported(D, nh) == want
    # exactly the conjunction of the two queries it is defined by (PENEO_BF16 = 1)
    from peneo_amd import hip
    both = lib.peneo_pair_save_supported(hip.BF16, D, nh) and lib.peneo_pair_mxfp8_supported(D, nh)
    assert bool(both) == bool(want)


def pb_num_tiles(N):
    """common.h: blocks of 8 rows x 16 columns that touch the triangle i <= j < N"""
    def before(ti):
        m = ti >> 1
        return ti * ((N + 15) // 16) - (m * (m - 1) + (m if ti & 1 else 0))
    return before((N + 7) // 8)


@pytest.mark.parametrize("N,odd", [(33, True), (97, True), (48, False), (16, False)])
def test_block_count_parities_of_the_gpu_shapes(N, odd):
    """the kernel tests want both an absent second block in the last workgroup (odd count) and none (even count)"""
    n = pb_num_tiles(N)
    brute = sum(1 for ti in range((N + 7) // 8) for tj in range((N + 15) // 16) if 16 * tj + 15 >= 8 * ti)
    assert n == brute
    assert (n % 2 == 1) == odd
    from peneo_amd import hip
    rows = hip.lib().peneo_pair_bwd_rows(N)
    assert rows == 128 * n
