"""Host-side checks of the two-stream attention training entry points (no GPU needed)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    lib.peneo_attn2_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.peneo_attn2_bwd_workspace_bytes.argtypes = [ctypes.c_int] * 3
    return lib


def test_training_symbols_are_declared_and_exported(lib):
    from peneo_amd import hip
    for name in ("peneo_attn2_fwd_dropout", "peneo_attn2_bwd_workspace_bytes", "peneo_attn2_bwd"):
        assert name in hip.SIGNATURES
        assert hasattr(lib, name)
    assert lib.peneo_version() >= 104
    # the backward's argument list: dtype, 6 operands + 2 strides, 4 outputs of the forward + 2 strides, lse, 5 sizes, 2 scales, key bias,
    # 6 gradients + 2 strides, workspace, drop_p, words, stream
    assert len(hip.SIGNATURES["peneo_attn2_bwd"][1]) == 36
    assert len(hip.SIGNATURES["peneo_attn2_fwd_dropout"][1]) == len(hip.SIGNATURES["peneo_attn2_fwd"][1]) + 2


def test_workspace_holds_delta_and_the_slab(lib):
    assert lib.peneo_attn2_bwd_workspace_bytes(2, 3, 97) >= 2 * 3 * 97 * 4 + 2 * 3 * 97 * 128 * 2
    assert lib.peneo_attn2_bwd_workspace_bytes(8, 12, 512) >= 8 * 12 * 512 * 4 + 8 * 12 * 512 * 512 * 2
    for B, nh, T in ((0, 3, 97), (2, 0, 97), (2, 3, 0), (-1, 3, 97), (2, 3, -5)):
        assert ctypes.c_ssize_t(lib.peneo_attn2_bwd_workspace_bytes(B, nh, T)).value <= 0


def _lilt_cfg(size="base"):
    from seeded import lilt_config
    from peneo_amd.model.configuration_peneo import LiltConfig
    return LiltConfig(**{k: v for k, v in lilt_config(size).items() if k != "model_type"})


@pytest.mark.parametrize("value,on", [(None, False), ("0", False), ("", False), ("1", True)])
def test_training_switch_is_off_unless_set_to_one(monkeypatch, value, on):
    from peneo_amd.model.modeling_lilt import lilt_route
    if value is None:
        monkeypatch.delenv("PENEO_LILT_ATTN2_TRAIN", raising=False)
    else:
        monkeypatch.setenv("PENEO_LILT_ATTN2_TRAIN", value)
    train = SimpleNamespace(p_attn=0.1)
    assert (lilt_route(_lilt_cfg(), torch.bfloat16, train, True).attention == "attn2_train") is on


def test_training_switch_needs_bf16_the_widths_and_a_training_forward(monkeypatch):
    from peneo_amd.model.modeling_lilt import lilt_route
    monkeypatch.setenv("PENEO_LILT_ATTN2_TRAIN", "1")
    monkeypatch.delenv("PENEO_LILT_ATTN2", raising=False)
    train, evals = SimpleNamespace(p_attn=0.1), SimpleNamespace(p_attn=0.0)
    base, tiny = _lilt_cfg(), _lilt_cfg("tiny")                                                  # head dims 64 + 16, 48 + 12
    assert lilt_route(base, torch.bfloat16, evals, True).attention == "attn2_train"             # autograd alone is enough
    assert lilt_route(base, torch.float32, train, True).attention != "attn2_train"
    assert lilt_route(tiny, torch.bfloat16, train, True).attention != "attn2_train"
    assert lilt_route(base, torch.bfloat16, train, False).attention == "attn2_train"            # attention dropout alone is enough
    assert lilt_route(base, torch.bfloat16, evals, False).attention == "attn2_eval"             # an eval forward
