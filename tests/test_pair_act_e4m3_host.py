"""Host-side checks of the e4m3 form of the saved pair activations (no GPU needed): exports, signatures, version, the support and
size queries against the f16 form's, and the validation of PEneoModel.set_pair_act_format."""
import ctypes

import pytest
import torch

NEW = (("peneo_pair_save_e4m3_supported", 3), ("peneo_pair_save_e4m3_bytes", 4), ("peneo_pair_heads_fwd_save_e4m3", 10),
       ("peneo_pair_bwd_saved_e4m3", 13))


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    return hip.lib()


def test_symbols_are_declared_and_exported(lib):
    import os
    from peneo_amd import hip
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "peneo_hip.h")).read()
    for name, nargs in NEW:
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs
        assert hasattr(raw, name)
        assert name + "(" in header
        assert len(getattr(lib, name).argtypes) == nargs
    # the e4m3 entry points take the arguments of the f16 ones
    assert hip.SIGNATURES["peneo_pair_heads_fwd_save_e4m3"] == hip.SIGNATURES["peneo_pair_heads_fwd_save"]
    assert hip.SIGNATURES["peneo_pair_bwd_saved_e4m3"] == hip.SIGNATURES["peneo_pair_bwd_saved"]
    assert lib.peneo_pair_save_e4m3_bytes.restype is ctypes.c_size_t
    assert lib.peneo_version() >= 109


def test_python_entry_points_exist():
    from peneo_amd import ops
    from peneo_amd.model import PEneoDecoder, PEneoModel
    assert callable(ops.pair_save_e4m3_supported) and callable(ops.pair_save_e4m3_bytes)
    assert callable(PEneoModel.set_pair_act_format) and callable(PEneoDecoder.set_pair_act_format)
    with pytest.raises(ValueError):
        ops.pair_heads_fwd(torch.zeros(1, 2, 64), None, None, None, [2], save=True, save_format="fp8")
    with pytest.raises(ValueError):
        ops.pair_bwd_saved(torch.zeros(1, 2, 64), None, None, None, None, None, None, act_format="fp8")


def test_support_query(lib):
    from peneo_amd import hip
    assert lib.peneo_pair_save_e4m3_supported(hip.BF16, 384, 5) == 1
    for dtype, D, nh in ((hip.F32, 384, 5), (hip.BF16, 512, 5), (hip.BF16, 384, 0), (hip.BF16, 96, 5)):
        assert lib.peneo_pair_save_e4m3_supported(dtype, D, nh) == 0, (dtype, D, nh)
    # exactly where the f16 form is supported, and the old predicates answer as before
    for dtype in (hip.F32, hip.BF16):
        for D in (32, 96, 128, 384, 512, 768, 1024):
            for nh in (0, 1, 5, 8, 9):
                assert lib.peneo_pair_save_e4m3_supported(dtype, D, nh) == lib.peneo_pair_save_supported(dtype, D, nh)
    assert lib.peneo_pair_save_supported(hip.BF16, 384, 5) == 1 and lib.peneo_pair_save_supported(hip.BF16, 512, 5) == 0
    assert lib.peneo_pair_save_supported(hip.F32, 384, 5) == 0
    assert lib.peneo_pair_mxfp8_save_supported(384, 5) == 1 and lib.peneo_pair_mxfp8_save_supported(512, 5) == 0
    assert lib.peneo_pair_bwd_supported(hip.BF16, 512, 5) == 1 and lib.peneo_pair_bwd_supported(hip.BF16, 512, 6) == 0


def test_size_query(lib):
    from peneo_amd import ops
    assert lib.peneo_pair_save_bytes(8, 511, 5, 384) == 8 * 1056 * 60 * 4 * 2048
    for B, N in ((8, 511), (1, 9)):
        full = lib.peneo_pair_save_bytes(B, N, 5, 384)
        assert full > 0 and full % 2 == 0
        assert lib.peneo_pair_save_e4m3_bytes(B, N, 5, 384) == full // 2 == ops.pair_save_e4m3_bytes(B, N, 5, 384)
    assert lib.peneo_pair_save_e4m3_bytes(0, 511, 5, 384) == 0
    assert lib.peneo_pair_save_e4m3_bytes(1, 0, 5, 384) == 0 and lib.peneo_pair_save_e4m3_bytes(1, 9, 0, 384) == 0


def _mk(width="base", **over):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    bc = dict(layoutlmv3_config(width), num_hidden_layers=1, vocab_size=100)
    pcfg = dict(peneo_config("layoutlmv3-base", bc), **over)
    return PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))


def test_setter_validation():
    m = _mk().set_compute_dtype(torch.bfloat16)
    dec = m.peneo_decoder
    assert dec.pair_act_format == "f16"                                   # the default
    with pytest.raises(ValueError):
        m.set_pair_act_format("fp8")                                      # an unknown name
    with pytest.raises(ValueError):
        m.set_pair_act_format("bf16")
    m.set_compute_dtype(torch.float32)
    with pytest.raises(ValueError):
        m.set_pair_act_format("e4m3")                                     # fp32 compute
    m.set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError):
        _mk(peneo_classifier_num_layers=3).set_compute_dtype(torch.bfloat16).set_pair_act_format("e4m3")
    with pytest.raises(ValueError):
        _mk("tiny").set_compute_dtype(torch.bfloat16).set_pair_act_format("e4m3")      # a width without the saved backward
    for attr in ("save_pair_act", "fused_bwd"):                           # the saved backward switched off
        setattr(dec, attr, False)
        with pytest.raises(ValueError):
            m.set_pair_act_format("e4m3")
        setattr(dec, attr, True)
    assert dec.pair_act_format == "f16"                                   # none of the refused calls changed it
    # not together with the MXFP8 train forward, in either order
    m.set_pair_heads_train_format("mxfp8")
    with pytest.raises(ValueError):
        m.set_pair_act_format("e4m3")
    m.set_pair_heads_train_format("bf16")
    assert m.set_pair_act_format("e4m3") is m and dec.pair_act_format == "e4m3"
    with pytest.raises(ValueError):
        m.set_pair_heads_train_format("mxfp8")
    assert dec.pair_heads_train_format == "bf16"
    assert m.set_pair_act_format("f16") is m and dec.pair_act_format == "f16"
    m.set_pair_heads_train_format("mxfp8")                                # ... and fine again once the records are f16
