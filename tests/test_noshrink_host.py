"""peneo_decoder_shrink = False, host side (no GPU): the oracle's shrink-off branch against the fixture the real reference wrote
(tests/golden/make_golden_noshrink.py), and the new width query in header, exports, ctypes table and ops."""
import os
import re

import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")


def test_oracle_shrink_off_reproduces_the_reference_fixture():
    """LayoutLMv3-base widths, one layer, shrink off (decoder width 768): weights regenerated from the seed, batch from its
    arguments; logits and losses within 1e-5 of the reference's, the same argmax everywhere."""
    from oracle import peneo_oracle as O
    from seeded import seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    from peneo_amd.model import PEneoConfig, PEneoModel
    fx = load_golden("lmv3_h768_noshrink")
    pcfg = fx["config"]
    assert pcfg["peneo_decoder_shrink"] is False
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    assert m.peneo_decoder.decoder_hidden_size == 768 and not hasattr(m.peneo_decoder, "shrink_projection")
    sd = seeded_fill_(m.state_dict(), fx["seed"])
    batch = synthetic_rfund_batch(**fx["batch_args"])
    with torch.no_grad():
        ref = O.peneo_forward({k: v.detach().clone() for k, v in sd.items()}, pcfg, batch)
    for h in HEADS:
        got, want = ref[h + "_shaking_outputs"], fx["logits"][h]
        assert got.shape == want.shape == (2, 1128, 2 if h == "line_extraction" else 3)
        err = float((got - want).abs().max())
        assert err <= 1e-5, (h, err)
        assert torch.equal(got.argmax(-1), want.argmax(-1)), h
        assert abs(float(ref[h + "_loss"]) - float(fx["losses"][h + "_loss"])) <= 1e-5, h
    assert abs(float(ref["loss"]) - float(fx["losses"]["loss"])) <= 1e-5
    # what the GPU test compares gradients with: every parameter's norm, the tensors under 64 KiB in full
    names = {n for n, _ in m.named_parameters()}
    assert set(fx["grad_norms"]) <= names and set(fx["grads_full"]) <= set(fx["grad_norms"]) and len(fx["grads_full"]) >= 20
    assert all(g.numel() * 4 < 64 * 1024 for g in fx["grads_full"].values())


def test_width_query_is_declared_exported_bound_and_wrapped():
    from peneo_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    declared = set(re.findall(r"\b(peneo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    name = "peneo_pair_heads_supported"
    lib = hip.load_library()
    assert name in declared, f"{name} is not declared in include/peneo_hip.h"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in hip.SIGNATURES, f"{name} is missing from the ctypes table"
    assert sorted(hip.SIGNATURES) == sorted(declared)
    assert lib.peneo_version() >= 108
    assert callable(ops.pair_heads_supported)


def test_width_query_answers_without_a_gpu():
    """The kernels' widths: D / 16 in {2, 4, 6, 8, 12, 16, 24, 32} in both dtypes; above 512 bf16 only, multiples of 64 up to 1024."""
    from peneo_amd import ops
    f32, bf16 = torch.float32, torch.bfloat16
    for D in (32, 64, 96, 128, 192, 256, 384, 512):
        assert ops.pair_heads_supported(f32, D, 5) and ops.pair_heads_supported(bf16, D, 5), D
    for D in (160, 320, 448, 480):
        assert not ops.pair_heads_supported(f32, D, 5) and not ops.pair_heads_supported(bf16, D, 5), D
    for D in (576, 640, 704, 768, 832, 896, 960, 1024):
        assert ops.pair_heads_supported(bf16, D, 5) and not ops.pair_heads_supported(f32, D, 5), D
    for D in (544, 800, 992, 1056, 1088, 2048, 0, -64, 48):
        assert not ops.pair_heads_supported(bf16, D, 5), D
    assert not ops.pair_heads_supported(bf16, 768, 0) and not ops.pair_heads_supported(bf16, 768, 9)
    assert ops.pair_heads_supported(bf16, 896, 8) and not ops.pair_heads_supported(bf16, 1024, 8)   # (LDS: ring + b1 table)
    # a width without a kernel has no packed image above 512
    from peneo_amd import hip
    lib = hip.lib()
    assert lib.peneo_pair_heads_packed_bytes(hip.F32, 5, 768) == 0
    assert lib.peneo_pair_heads_packed_bytes(hip.BF16, 5, 768) == 5 * 768 // 32 * 52 * 1024
    assert lib.peneo_pair_heads_packed_bytes(hip.BF16, 5, 1024) == 5 * 1024 // 32 * 68 * 1024
