"""MXFP8 pair heads at decoder widths 512 < D <= 1024 (peneo_pair_heads_fwd_mxfp8_wide), host side (no GPU): the four entry points
in header, exports and ctypes table, the host-side query and packed size, that the narrow entry points answer as before, and the
decoder's switch - set_pair_heads_format("mxfp8", wide=True) - with the route it gives."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
NAMES = ("peneo_pair_mxfp8_wide_supported", "peneo_pair_heads_mxfp8_wide_packed_bytes", "peneo_pair_heads_pack_mxfp8_wide",
         "peneo_pair_heads_fwd_mxfp8_wide")
WIDTHS = (576, 640, 704, 768, 832, 896, 960, 1024)
REFUSED = [(384, 5), (512, 5), (800, 5), (1088, 5), (0, 5), (-64, 5), (768, 0), (768, 9), (1024, 0), (1024, 9)]


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    lb = ctypes.CDLL(hip.LIB_PATH)
    for name in ("peneo_pair_heads_mxfp8_wide_packed_bytes", "peneo_pair_heads_mxfp8_packed_bytes"):
        getattr(lb, name).restype = ctypes.c_size_t
    return lb


def _decoder(D=768):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig
    from peneo_amd.model.peneo_decoder import PEneoDecoder
    cfg = dict(peneo_config("layoutlmv3-base", layoutlmv3_config("tiny")), peneo_decoder_shrink=False)
    return PEneoDecoder(config=PEneoConfig(**cfg), input_size=D)


def test_entry_points_are_declared_exported_bound_and_wrapped(lib):
    from peneo_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    declared = set(re.findall(r"\b(peneo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/peneo_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hip.SIGNATURES, f"{name} is missing from the ctypes table"
    assert sorted(hip.SIGNATURES) == sorted(declared)
    assert lib.peneo_version() >= 112
    for name in ("pair_mxfp8_wide_supported", "pair_heads_pack_mxfp8_wide", "pair_heads_fwd_mxfp8_wide"):
        assert callable(getattr(ops, name)), name


@pytest.mark.parametrize("D", WIDTHS)
def test_query_accepts_the_eight_widths_with_five_heads(lib, D):
    from peneo_amd import ops
    assert lib.peneo_pair_mxfp8_wide_supported(D, 5) == 1
    assert ops.pair_mxfp8_wide_supported(D, 5) is True
    # a slab is a whole number of 4 KiB (one 1 KiB DMA piece per wave of the four) that holds D / 64 fragments of 2 KiB, the scale
    # words and the two second-layer fragments; one slab per 32 hidden units of the 5 D
    nbytes = lib.peneo_pair_heads_mxfp8_wide_packed_bytes(5, D)
    nslab = 5 * D // 32
    payload = (D // 64) * 2048 + -(-(D // 64) // 4) * 256 + 2048
    assert nbytes == nslab * (-(-payload // 4096) * 4096)


@pytest.mark.parametrize("D,nh", REFUSED)
def test_query_refuses_and_the_packed_size_is_zero_exactly_there(lib, D, nh):
    assert lib.peneo_pair_mxfp8_wide_supported(D, nh) == 0
    assert lib.peneo_pair_heads_mxfp8_wide_packed_bytes(nh, D) == 0


def test_packed_size_is_nonzero_exactly_where_the_query_is_one(lib):
    for D in range(-64, 1216, 32):
        for nh in range(0, 10):
            assert (lib.peneo_pair_heads_mxfp8_wide_packed_bytes(nh, D) != 0) == (lib.peneo_pair_mxfp8_wide_supported(D, nh) == 1), (D, nh)
    # by the real LDS need: the ring of three slabs and the b1 table of eight heads still fit at every width
    assert all(lib.peneo_pair_mxfp8_wide_supported(D, 8) == 1 for D in WIDTHS)


@pytest.mark.parametrize("D", [768, 1024])
def test_the_narrow_entry_points_answer_as_before(lib, D):
    assert lib.peneo_pair_mxfp8_supported(D, 5) == 0
    assert lib.peneo_pair_heads_mxfp8_packed_bytes(5, D) == 0
    assert lib.peneo_pair_mxfp8_save_supported(D, 5) == 0
    assert lib.peneo_pair_mxfp8_supported(512, 5) == 1 and lib.peneo_pair_mxfp8_supported(384, 5) == 1


def test_decoder_switch_at_768(monkeypatch):
    from peneo_amd.model.peneo_decoder import PairRoute, pair_route
    for var in ("PENEO_SKIP_PADDED_PAIRS", "PENEO_PAIR_WIDE"):
        monkeypatch.delenv(var, raising=False)
    dec = _decoder(768)
    with pytest.raises(ValueError, match="D = 768") as err:
        dec.set_pair_heads_format("mxfp8")                       # without wide=True: refused as before ...
    assert "wide=True" in str(err.value)                         # ... with a pointer to the switch
    assert dec.pair_heads_format == "bf16"
    dec.set_pair_heads_format("mxfp8", wide=True)
    assert dec.pair_heads_format == "mxfp8"
    with pytest.raises(ValueError):
        dec.set_pair_heads_train_format("mxfp8")                 # no saved backward at this width
    assert dec.pair_heads_train_format == "bf16"
    # the route of a forward without gradients, with labels and without; pair_wide (the bf16 A/B arm) is not consulted
    for pair_wide in (True, False):
        dec.pair_wide = pair_wide
        assert pair_route(dec, BF16, 768, False, True, 0.0) == PairRoute("mxfp8_eval")
        assert pair_route(dec, BF16, 768, False, False, 0.0, has_mask=True) == PairRoute("mxfp8_eval")
    dec.pair_wide = True
    # the length-aware walk and "mxfp8" keep refusing each other, either way round
    with pytest.raises(ValueError, match="mxfp8"):
        dec.set_skip_padded_pairs(True)
    assert dec.skip_padded_pairs is False
    dec.set_pair_heads_format("bf16")
    dec.set_skip_padded_pairs(True)
    with pytest.raises(ValueError, match="length-aware"):
        dec.set_pair_heads_format("mxfp8", wide=True)
    assert dec.pair_heads_format == "bf16"
    dec.set_skip_padded_pairs(False)
    dec.set_pair_heads_format("mxfp8", wide=True)
    # a forward with gradients is refused before anything runs (host tensors: no kernel could)
    B, N = 1, 4
    labels = [torch.zeros(B, N * (N + 1) // 2, dtype=torch.int64) for _ in range(5)]
    with pytest.raises(ValueError, match="inference-only"):
        dec(torch.zeros(B, N, 768, dtype=BF16, requires_grad=True), None, *labels)
    with torch.no_grad(), pytest.raises(ValueError, match="bfloat16"):
        dec(torch.zeros(B, N, 768, dtype=torch.float32), None, *labels)


def test_wide_changes_nothing_up_to_512_and_refuses_what_no_kernel_holds():
    from peneo_amd.model.peneo_decoder import PairRoute, pair_route
    dec = _decoder(384)
    dec.set_pair_heads_format("mxfp8", wide=True)
    assert dec.pair_heads_format == "mxfp8" and pair_route(dec, BF16, 384, False, True, 0.0) == PairRoute("mxfp8_eval")
    for D in (800, 1088):                                        # not a multiple of 64; above 1024
        dec = _decoder(D)
        for wide in (False, True):
            with pytest.raises(ValueError, match=f"D = {D}") as err:
                dec.set_pair_heads_format("mxfp8", wide=wide)
            assert "wide=True" not in str(err.value)
        assert dec.pair_heads_format == "bf16"


def test_route_up_to_512_asks_in_the_old_order():
    """widths the narrow MXFP8 kernel holds but no fused bf16 kernel does: the format is accepted and the step stays on the
    materialising path, as before"""
    from peneo_amd import ops
    from peneo_amd.model.peneo_decoder import PairRoute, pair_route
    for D in (320, 448):
        assert ops.pair_mxfp8_supported(D, 5) and not ops.pair_heads_supported(BF16, D, 5)
        for wide in (False, True):
            dec = _decoder(D)
            dec.set_pair_heads_format("mxfp8", wide=wide)
            assert pair_route(dec, BF16, D, False, True, 0.0) == PairRoute("generic")


def test_model_setter_passes_wide_on():
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    bcfg = dict(layoutlmv3_config("base"), num_hidden_layers=1, vocab_size=1000)
    pcfg = dict(peneo_config("layoutlmv3-base", bcfg), peneo_decoder_shrink=False)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    with pytest.raises(ValueError, match="bfloat16"):
        m.set_pair_heads_format("mxfp8", wide=True)              # fp32 compute
    m.set_compute_dtype(BF16)
    with pytest.raises(ValueError, match="D = 768"):
        m.set_pair_heads_format("mxfp8")
    assert m.set_pair_heads_format("mxfp8", wide=True) is m and m.peneo_decoder.pair_heads_format == "mxfp8"
    with pytest.raises(ValueError):
        m.set_pair_heads_train_format("mxfp8")
    m.set_pair_heads_format("bf16")
    assert m.peneo_decoder.pair_heads_format == "bf16"
