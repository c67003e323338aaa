"""peneo_pair_dz_fused at decoder widths 512 < D <= 1024, host side (no GPU): the width query in header, exports, ctypes table and
ops and its answers; the workspace rows the four-wave kernel keeps; the decoder's switch."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def hip():
    """the binding module, with the deterministic mode it found restored afterwards"""
    from peneo_amd import hip as h
    h.load_library()
    before = h.deterministic_mode()
    yield h
    h.set_deterministic(before)


def test_query_is_declared_exported_bound_and_wrapped(hip):
    from peneo_amd import ops
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    declared = set(re.findall(r"\b(peneo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    name = "peneo_pair_dz_fused_supported"
    lib = hip.lib()
    assert name in declared, f"{name} is not declared in include/peneo_hip.h"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in hip.SIGNATURES, f"{name} is missing from the ctypes table"
    assert sorted(hip.SIGNATURES) == sorted(declared)
    assert lib.peneo_version() >= 110
    assert callable(ops.pair_dz_fused_supported)


def test_query_answers_without_a_gpu(hip):
    from peneo_amd import ops
    f32, bf16 = torch.float32, torch.bfloat16
    for D in (768, 960, 1024):
        assert ops.pair_dz_fused_supported(bf16, D, 5) is True, D
    for D in (384, 512, 96):
        assert ops.pair_dz_fused_supported(bf16, D, 5) is True, D
    for D in (800, 320, 1088):
        assert ops.pair_dz_fused_supported(bf16, D, 5) is False, D
    for D in (32, 96, 384, 512, 768, 800, 960, 1024, 1088):
        assert ops.pair_dz_fused_supported(f32, D, 5) is False, D
    for D in (96, 384, 768, 1024):
        assert ops.pair_dz_fused_supported(bf16, D, 0) is False, D
    # the whole families: the narrow list, and every multiple of 64 above 512 up to 1024
    for D in (32, 64, 96, 128, 192, 256, 384, 512, 576, 640, 704, 768, 832, 896, 960, 1024):
        assert ops.pair_dz_fused_supported(bf16, D, 5), D
    for D in (0, -64, 48, 160, 448, 544, 992, 1056, 2048):
        assert not ops.pair_dz_fused_supported(bf16, D, 5), D
    assert not ops.pair_dz_fused_supported(bf16, 768, 9)


def test_workspace_rows_are_what_they_were(hip):
    """The four-wave kernel keeps 256 pairs a workgroup: the answers test_deterministic_host.py pins."""
    lib = hip.lib()
    hip.set_deterministic(0)
    assert lib.peneo_pair_dz_fused_workspace_rows(1) == 256 and lib.peneo_pair_dz_fused_workspace_rows(1 << 18) == 256
    for mode in (1, 2):
        hip.set_deterministic(mode)
        assert lib.peneo_pair_dz_fused_workspace_rows(1) == 256 and lib.peneo_pair_dz_fused_workspace_rows(256 * 256) == 256
        assert lib.peneo_pair_dz_fused_workspace_rows(256 * 256 + 1) == 257 and lib.peneo_pair_dz_fused_workspace_rows(1 << 18) == 1024
    hip.set_deterministic(0)
    assert lib.peneo_pair_dz_fused_workspace_rows(0) == 0


@pytest.mark.parametrize("env,want", [(None, False), ("0", False), ("1", True)])
def test_switch_is_off_by_default_and_follows_the_environment(env, want, monkeypatch):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig
    from peneo_amd.model.peneo_decoder import PEneoDecoder
    if env is None:
        monkeypatch.delenv("PENEO_DZ_FUSED_WIDE", raising=False)
    else:
        monkeypatch.setenv("PENEO_DZ_FUSED_WIDE", env)
    bcfg = layoutlmv3_config("tiny")
    cfg = PEneoConfig(**dict(peneo_config("layoutlmv3-base", bcfg), peneo_decoder_shrink=False))
    dec = PEneoDecoder(config=cfg, input_size=bcfg["hidden_size"])
    assert dec.fused_dz_wide is want
    assert dec.fused_dz is True          # (the switch it depends on keeps its default)
