"""Packed encoder for inference, host side (no GPU): the six entry points in header, exports, ctypes table and ops; the
host-side `supported` query; encoder_route over its whole condition table; the refusals at set time; the environment default."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("peneo_pack_plan", "peneo_rows_pack", "peneo_rows_unpack", "peneo_attn_fwd_varlen_supported", "peneo_attn_fwd_varlen",
         "peneo_encoder_layer_fwd_packed")
WRAPPERS = ("pack_plan", "rows_pack", "rows_unpack", "attn_fwd_varlen_supported", "attn_fwd_varlen", "encoder_layer_fwd_packed")


def _peneo(backbone="lmv3"):
    from seeded import layoutlmv3_config, lilt_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    if backbone == "lmv3":
        pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("tiny"))
    else:
        pcfg = peneo_config("lilt-roberta-en-base", lilt_config("tiny"))
    return PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))


def test_entry_points_are_declared_exported_bound_and_wrapped():
    from peneo_amd import hip, ops
    from peneo_amd.model import PEneoModel
    from peneo_amd.model.modeling_layoutlmv3 import LayoutLMv3Model
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    declared = set(re.findall(r"\b(peneo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = hip.load_library()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/peneo_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hip.SIGNATURES, f"{name} is missing from the ctypes table"
    assert sorted(hip.SIGNATURES) == sorted(declared)
    assert lib.peneo_version() >= 113
    for name in WRAPPERS:
        assert callable(getattr(ops, name)), name
    assert callable(PEneoModel.set_skip_padded_tokens) and callable(LayoutLMv3Model.set_skip_padded_tokens)


def test_supported_query_is_one_for_bf16_at_64_only():
    from peneo_amd import hip, ops
    lib = hip.load_library()
    for dtype, d in itertools.product((hip.F32, hip.BF16, 2, -1), (0, 16, 32, 63, 64, 65, 96, 128)):
        assert lib.peneo_attn_fwd_varlen_supported(dtype, d) == int(dtype == hip.BF16 and d == 64), (dtype, d)
    assert ops.attn_fwd_varlen_supported(BF16, 64) is True
    assert ops.attn_fwd_varlen_supported(F32, 64) is False and ops.attn_fwd_varlen_supported(BF16, 32) is False


def test_unsupported_varlen_call_is_an_error_with_a_text_never_a_fallback():
    """(refused on the host before anything is launched: no GPU is touched)"""
    from peneo_amd import hip
    lib = hip.load_library()
    for dtype, d in ((hip.F32, 64), (hip.BF16, 32)):
        rc = lib.peneo_attn_fwd_varlen(dtype, 16, 16, 16, 64, 1, 16, 16, 1, 1, 1, d, 1.0, 16, 64, 16, 64, None, None)
        assert rc == -1                                                   # PENEO_ERR_INVALID
        text = lib.peneo_last_error().decode()
        assert "peneo_attn_fwd_varlen" in text and "no fallback" in text, text


ON = dict(switch=True, grad_enabled=False, training=False, dtype=BF16, has_mask=True, stage_calls=True, head_dim=64, has_bias=True,
          encoder_format="bf16")
OFF_VALUES = dict(switch=False, grad_enabled=True, training=True, dtype=F32, has_mask=False, stage_calls=False, head_dim=32, has_bias=False,
                  encoder_format="mxfp8")


def test_route_over_the_whole_condition_table():
    from peneo_amd.model.modeling_layoutlmv3 import encoder_route
    assert sorted(ON) == sorted(OFF_VALUES)
    assert encoder_route(**ON) == "packed"
    # every subset of violated conditions: packed only when none is violated
    keys = sorted(ON)
    for n in range(1, len(keys) + 1):
        for bad in itertools.combinations(keys, n):
            args = dict(ON, **{k: OFF_VALUES[k] for k in bad})
            assert encoder_route(**args) == "padded", bad
    # other head dims: none is packed
    for d in (16, 48, 96, 128):
        assert encoder_route(**dict(ON, head_dim=d)) == "padded"


def test_refusals_at_set_time():
    m = _peneo("lmv3").set_compute_dtype(BF16)
    assert m.backbone.skip_padded_tokens is False
    assert m.set_skip_padded_tokens(True) is m and m.backbone.skip_padded_tokens is True
    with pytest.raises(ValueError, match="skip_padded_tokens"):           # the MXFP8 encoder after the switch
        m.set_encoder_format("mxfp8")
    assert m.backbone.encoder_format == "bf16"
    assert m.set_skip_padded_tokens(False) is m and m.backbone.skip_padded_tokens is False
    # the switch after the MXFP8 encoder (set on the backbone directly: the base-width query needs no GPU, the tiny widths have no
    # MXFP8 form)
    m.backbone.encoder_format = "mxfp8"
    with pytest.raises(ValueError, match="mxfp8"):
        m.set_skip_padded_tokens(True)
    with pytest.raises(ValueError, match="mxfp8"):
        m.backbone.set_skip_padded_tokens(True)
    assert m.backbone.skip_padded_tokens is False
    m.backbone.encoder_format = "bf16"
    # a LiLT backbone
    lilt = _peneo("lilt")
    with pytest.raises(ValueError, match="LiLT"):
        lilt.set_skip_padded_tokens(True)
    assert lilt.set_skip_padded_tokens(False) is lilt
    # the two inference switches are independent, and the MXFP8 pair heads are not refused beside this one
    m.set_skip_padded_tokens(True).set_skip_padded_pairs(True)
    assert m.backbone.skip_padded_tokens and m.peneo_decoder.skip_padded_pairs
    m.set_skip_padded_pairs(False)
    assert m.backbone.skip_padded_tokens and not m.peneo_decoder.skip_padded_pairs


@pytest.mark.parametrize("env,want", [(None, False), ("0", False), ("1", True)])
def test_switch_is_off_by_default_and_follows_the_environment(env, want, monkeypatch):
    if env is None:
        monkeypatch.delenv("PENEO_SKIP_PADDED_TOKENS", raising=False)
    else:
        monkeypatch.setenv("PENEO_SKIP_PADDED_TOKENS", env)
    m = _peneo("lmv3")
    assert m.backbone.skip_padded_tokens is want
    m.set_skip_padded_tokens(not want)
    assert m.backbone.skip_padded_tokens is (not want)


def test_docstrings_state_the_host_read_and_the_zero_rows():
    from peneo_amd.model import PEneoModel
    from peneo_amd.model.modeling_layoutlmv3 import LayoutLMv3Model
    doc = " ".join(LayoutLMv3Model.set_skip_padded_tokens.__doc__.split())
    assert "ONE device-to-host read" in doc and "ZEROS" in doc and "set_skip_padded_pairs(True)" in doc
    assert "set_skip_padded_pairs(True)" in " ".join(PEneoModel.set_skip_padded_tokens.__doc__.split())
