"""Length-aware pair heads (peneo_pair_heads_fwd_lens), host side (no GPU): the two entry points in header, exports, ctypes table
and ops; the model switch and what pair_route answers with it; and the compact walk restated in Python, checked exhaustively."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("peneo_pair_heads_fwd_lens", "peneo_pair_lens_from_mask")


def _decoder(D=384, kcls=2, ohem=False):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig
    from peneo_amd.model.peneo_decoder import PEneoDecoder
    over = dict(peneo_decoder_shrink=False, peneo_classifier_num_layers=kcls)
    if ohem:
        over.update(peneo_ohem_num_positive=8, peneo_ohem_num_negative=8)
    return PEneoDecoder(config=PEneoConfig(**dict(peneo_config("layoutlmv3-base", layoutlmv3_config("tiny")), **over)), input_size=D)


def test_entry_points_are_declared_exported_bound_and_wrapped():
    from peneo_amd import hip, ops
    from peneo_amd.model import PEneoModel
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    declared = set(re.findall(r"\b(peneo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = hip.load_library()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/peneo_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hip.SIGNATURES, f"{name} is missing from the ctypes table"
    assert sorted(hip.SIGNATURES) == sorted(declared)
    assert lib.peneo_version() >= 111
    assert re.search(r"#define\s+PENEO_PAIR_PAD_LOGIT\s+\(-1e30f\)", src)
    assert ops.PAIR_PAD_LOGIT == -1e30
    assert callable(ops.pair_heads_fwd_lens) and callable(ops.pair_lens_from_mask)
    assert callable(PEneoModel.set_skip_padded_pairs)


def test_header_says_the_loss_is_not_the_reference_loss():
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    at = src.index("Length-aware inference form")
    text = " ".join(src[at:src.index("#define PENEO_PAIR_PAD_LOGIT")].replace("\n *", " ").split())
    assert "A DIFFERENT NUMBER from the reference's loss" in text and "LIVE PAIRS ONLY" in text


@pytest.mark.parametrize("env,want", [(None, False), ("0", False), ("1", True)])
def test_switch_is_off_by_default_and_follows_the_environment(env, want, monkeypatch):
    if env is None:
        monkeypatch.delenv("PENEO_SKIP_PADDED_PAIRS", raising=False)
    else:
        monkeypatch.setenv("PENEO_SKIP_PADDED_PAIRS", env)
    dec = _decoder()
    assert dec.skip_padded_pairs is want
    dec.set_skip_padded_pairs(not want)
    assert dec.skip_padded_pairs is (not want)


def test_route_with_the_switch(monkeypatch):
    from peneo_amd.model.peneo_decoder import PairRoute, pair_route
    for var in ("PENEO_SKIP_PADDED_PAIRS", "PENEO_DZ_FUSED", "PENEO_BWD_FUSED", "PENEO_PAIR_SAVE", "PENEO_PAIR_WIDE"):
        monkeypatch.delenv(var, raising=False)
    assert PairRoute("bf16") == PairRoute("bf16", lens=False)            # the new field's default keeps every existing route equal
    assert PairRoute("bf16", lens=True) != PairRoute("bf16")
    for dt, D in ((BF16, 384), (BF16, 512), (BF16, 64), (F32, 64), (BF16, 768)):
        dec = _decoder(D)
        plain = {k: pair_route(dec, dt, D, k[0], k[1], 0.0, has_mask=True) for k in ((False, False), (False, True), (True, True), (True, False))}
        assert not any(r.lens for r in plain.values())                   # off: nothing moves, mask or not
        dec.set_skip_padded_pairs(True)
        # eval without gradients and with a mask: the length-aware route, labels or not
        assert pair_route(dec, dt, D, False, True, 0.0, has_mask=True) == PairRoute("bf16", lens=True)
        assert pair_route(dec, dt, D, False, False, 0.0, has_mask=True) == PairRoute("bf16", lens=True)
        # without a mask: today's
        assert pair_route(dec, dt, D, False, True, 0.0, has_mask=False) == plain[(False, True)] == PairRoute("bf16")
        assert pair_route(dec, dt, D, False, True, 0.0) == PairRoute("bf16")
        # with gradients: today's route, with labels and without
        for has_tags in (True, False):
            assert pair_route(dec, dt, D, True, has_tags, 0.0, has_mask=True) == plain[(True, has_tags)]
            assert pair_route(dec, dt, D, True, has_tags, 0.1, has_mask=True) == pair_route(_decoder(D), dt, D, True, has_tags, 0.1)
    # the materialising path (3-layer classifiers) and OHEM losses keep the plain launch
    dec = _decoder(384, kcls=3)
    dec.set_skip_padded_pairs(True)
    assert pair_route(dec, BF16, 384, False, True, 0.0, has_mask=True) == PairRoute("generic")
    dec = _decoder(384, ohem=True)
    dec.set_skip_padded_pairs(True)
    assert pair_route(dec, BF16, 384, False, True, 0.0, has_mask=True) == PairRoute("bf16")
    assert pair_route(dec, BF16, 384, False, False, 0.0, has_mask=True) == PairRoute("bf16", lens=True)


def test_switch_and_mxfp8_refuse_each_other(monkeypatch):
    monkeypatch.delenv("PENEO_SKIP_PADDED_PAIRS", raising=False)
    dec = _decoder(384)
    dec.set_pair_heads_format("mxfp8")
    with pytest.raises(ValueError, match="mxfp8"):
        dec.set_skip_padded_pairs(True)
    assert dec.skip_padded_pairs is False
    dec.set_skip_padded_pairs(False)                                     # switching off is always fine
    dec.set_pair_heads_format("bf16")
    dec.set_skip_padded_pairs(True)
    with pytest.raises(ValueError, match="length-aware"):
        dec.set_pair_heads_format("mxfp8")
    assert dec.pair_heads_format == "bf16"


def test_model_setter_reaches_the_decoder(monkeypatch):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    monkeypatch.delenv("PENEO_SKIP_PADDED_PAIRS", raising=False)
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("tiny"))
    model = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    assert model.peneo_decoder.skip_padded_pairs is False
    assert model.set_skip_padded_pairs(True) is model and model.peneo_decoder.skip_padded_pairs is True
    model.set_compute_dtype(BF16)
    with pytest.raises(ValueError):
        model.set_pair_heads_format("mxfp8")
    model.set_skip_padded_pairs(False)
    assert model.peneo_decoder.skip_padded_pairs is False


def test_ops_refuse_host_tensors_by_name():
    from peneo_amd import ops
    from peneo_amd.hip import PeneoHipError
    with pytest.raises(PeneoHipError, match="pair_lens_from_mask"):
        ops.pair_lens_from_mask(torch.ones(2, 6, dtype=torch.int64), 6)
    with pytest.raises(PeneoHipError, match="pair_heads_fwd_lens"):
        ops.pair_heads_fwd_lens(torch.zeros(2, 4, 64), torch.tensor([4, 4]), None, None, None, [2])          # int64 lens


# ---- the compact walk, restated: workgroup x of document b owns local pairs q in [256 x, 256 x + 256) of the n_b-token triangle ----
def _row_start(i, n):
    return i * n - i * (i - 1) // 2


def _decode(q, n):
    """pair q of an n-token triangle -> (i, j): the largest i with row_start(i) <= q"""
    i = 0
    while i + 1 < n and _row_start(i + 1, n) <= q:
        i += 1
    return i, i + q - _row_start(i, n)


def _walk(n_raw, N, wg_pairs=256):
    """what one document's launch touches: the N-packed indices the main kernel writes, and the workgroups that leave at once"""
    n = min(max(n_raw, 0), N)
    P, Pb = N * (N + 1) // 2, n * (n + 1) // 2
    written, idle = [], []
    for x in range(-(-P // wg_pairs)):                       # the grid stays ceil(P / 256)
        if x * wg_pairs >= Pb:
            idle.append(x)
            continue
        for q in range(x * wg_pairs, min((x + 1) * wg_pairs, Pb)):
            i, j = _decode(q, n)
            assert 0 <= i <= j < n
            written.append(_row_start(i, N) + (j - i))
    return written, idle


def test_compact_walk_hits_every_live_pair_once_and_no_other():
    N = 40
    P = N * (N + 1) // 2
    for n in range(0, N + 1):
        written, idle = _walk(n, N)
        live = sorted(_row_start(i, N) + (j - i) for i in range(n) for j in range(i, n))
        assert len(written) == len(set(written)) == n * (n + 1) // 2, n
        assert sorted(written) == live, n
        assert all(0 <= p < P for p in written)
        # the fill covers the rest: pairs with j >= n, decoded at N
        padded = [p for p in range(P) if _decode(p, N)[1] >= n]
        assert sorted(padded + written) == list(range(P)), n
        assert idle == list(range(-(-(n * (n + 1) // 2) // 256), -(-P // 256))), n
    # a full document is the present walk, pair for pair and workgroup for workgroup; lengths are clamped to [0, N]
    assert _walk(N, N) == (list(range(P)), [])
    assert _walk(N + 7, N) == _walk(N, N) and _walk(-3, N) == _walk(0, N) == ([], [0, 1, 2, 3])
