"""The fused pair-heads forward at decoder widths 512 < D <= 1024 (pair_heads_wide.hip; bf16 only), op level: what
test_pair_heads_fwd_and_loss, test_pair_heads_fwd_classifier_dropout and test_pair_heads_fwd_hand_kernel_is_repeatable_at_size
(test_gpu_kernels.py) ask of the narrower kernels, at
    (33, 768)   P = 561: a ragged last block of pairs (and a workgroup whose second round is empty or partial)
    (130, 768)  many full blocks, both documents
    (71, 960)   KS = 60, not a power-of-two multiple
    (70, 1024)  the register and LDS ceiling
The reference is the fp32 torch computation on bf16-rounded operands, computed once per case."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = torch.bfloat16
CLASSES = [2, 3, 3, 3, 3]
CASES = [(33, 768), (130, 768), (71, 960), (70, 1024)]
P_DROP = 0.1


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


TOL_BF16 = 2e-2      # tol(bf16) of test_gpu_kernels.py


@functools.lru_cache(maxsize=None)
def _case(N, D):
    """inputs, the packed weights' sources and the fp32 references (plain and with the K12 mask) of one case; never modified"""
    from dropout_ref import k12_keep, k12_scale
    B = 2
    g = torch.Generator().manual_seed(N + D)
    ab = torch.randn(B, N, 2 * D, generator=g).to(DEV).to(DT)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    b1 = [0.1 * torch.randn(D, generator=g).to(DEV) for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).to(DEV) for c in CLASSES]
    b2 = [0.1 * torch.randn(c, generator=g).to(DEV) for c in CLASSES]
    P = N * (N + 1) // 2
    tags = [torch.randint(0, c, (B, P), generator=g).to(DEV) for c in CLASSES]
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device=DEV) for c in CLASSES]
    seed = 0xC0FFEE + N
    rd = lambda t: t.to(DT).float()
    ii, jj = torch.triu_indices(N, N, device=DEV)
    x = F.silu(ab.float()[:, ii, :D] + ab.float()[:, jj, D:])
    xq = x.to(DT).float()                                     # the kernel keeps x as bf16 fragments
    keep = torch.stack([k12_keep(seed, b, 0, P, len(CLASSES) * D, P_DROP) for b in range(B)]).to(DEV)   # [B, P, nh * D]
    ref, ref_drop = [], []
    for h, (a, b_, c, d) in enumerate(zip(w1, b1, w2, b2)):
        y = F.silu(F.linear(x, rd(a), b_))
        ref.append(F.linear(y, rd(c), d))
        yd = F.silu(F.linear(xq, rd(a), b_)) * keep[:, :, h * D:(h + 1) * D] * k12_scale(P_DROP)
        ref_drop.append(F.linear(yd, rd(c), d))
    keep_rate = float(keep.float().mean())
    return dict(B=B, P=P, ab=ab, w1=w1, b1=torch.cat(b1), w2=w2, b2=torch.cat(b2), tags=tags, cw=cw, seed=seed, ref=ref,
                ref_drop=ref_drop, keep_rate=keep_rate, keep_numel=keep.numel())


def test_width_query_on_the_device_box(ops):
    for D in (768, 960, 1024):
        assert ops.pair_heads_supported(DT, D, 5) and not ops.pair_heads_supported(torch.float32, D, 5)
    for D in (384, 512):
        assert ops.pair_heads_supported(DT, D, 5) and ops.pair_heads_supported(torch.float32, D, 5)


def test_fp32_above_512_is_refused_with_the_limit_named(ops):
    from peneo_amd.hip import PeneoHipError
    D = 768
    w1 = [torch.zeros(D, D, device=DEV) for _ in CLASSES]
    w2 = [torch.zeros(c, D, device=DEV) for c in CLASSES]
    with pytest.raises(PeneoHipError, match="D=768 not supported"):
        ops.pair_heads_pack(torch.float32, w1, w2)
    # the forward itself: a packed image of the bf16 kind, fp32 activations
    wp = ops.pair_heads_pack(DT, w1, w2)
    ab = torch.zeros(1, 8, 2 * D, device=DEV)
    with pytest.raises(PeneoHipError, match="D=768 not supported.*512"):
        ops.pair_heads_fwd(ab, wp, torch.zeros(5 * D, device=DEV), torch.zeros(14, device=DEV), CLASSES)


@pytest.mark.parametrize("N,D", CASES)
def test_pair_heads_wide_fwd_and_loss(ops, N, D):
    c = _case(N, D)
    wp = ops.pair_heads_pack(DT, c["w1"], c["w2"])
    logits, partials, dlog = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES, tags=c["tags"], class_weights=c["cw"],
                                                want_dlogits=True)
    assert partials.shape == (c["B"] * ((c["P"] + 255) // 256), 32)
    tot = partials.sum(0)
    num, den = tot[:5], tot[8:13]
    out, scale, dls = ops.loss_finish(partials, torch.ones(5, device=DEV), 14)
    for h in range(5):
        err = rel_err(logits[h], c["ref"][h])
        print(f"N={N} D={D} head {h}: logits rel_err {err:.3e}")
        assert err < TOL_BF16, (h, err)
        lr = logits[h].clone().requires_grad_(True)
        loss_sum = F.cross_entropy(lr.view(-1, CLASSES[h]), c["tags"][h].view(-1), weight=c["cw"][h], reduction="sum")
        loss_sum.backward()
        wsum = c["cw"][h][c["tags"][h].view(-1)].sum()
        assert abs(float(num[h]) - float(loss_sum)) / float(loss_sum) < 1e-4
        assert abs(float(den[h]) - float(wsum)) / float(wsum) < 1e-5
        assert rel_err(dlog[h], lr.grad) < 1e-4
    assert rel_err(dls, torch.cat([d.sum((0, 1)) for d in dlog])) < 1e-3
    assert abs(float(out[5]) - float((num / den).sum())) < 1e-4 and rel_err(scale[0], 1.0 / den) < 1e-5 and rel_err(scale[1], 1.0 / den) < 1e-5
    # loss-only call (no logits written) agrees
    _, part2, _ = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES, want_logits=False, tags=c["tags"], class_weights=c["cw"])
    assert rel_err(part2.sum(0)[:5], num) < 1e-5


@pytest.mark.parametrize("N,D", CASES)
def test_pair_heads_wide_classifier_dropout(ops, N, D):
    """The K12 mask inside the wide kernel is the function of (seed, document, pair, hidden column) that tests/dropout_ref.py
    restates and peneo_pair_dz regenerates in the chunked backward."""
    c = _case(N, D)
    assert abs(c["keep_rate"] - (1 - 6554 / 65536)) < 4 / math.sqrt(c["keep_numel"])
    wp = ops.pair_heads_pack(DT, c["w1"], c["w2"])
    logits, _, _ = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES, drop_p=P_DROP, drop_seed=c["seed"])
    plain, _, _ = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES)
    for h in range(5):
        err = rel_err(logits[h], c["ref_drop"][h])
        print(f"N={N} D={D} head {h}: dropout logits rel_err {err:.3e}, undropped against it {rel_err(plain[h], c['ref_drop'][h]):.3f}")
        assert err < TOL_BF16, (h, err)
        assert rel_err(plain[h], c["ref_drop"][h]) > 0.1              # the mask really changes the result
    again, _, _ = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES, drop_p=P_DROP, drop_seed=c["seed"])
    other, _, _ = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES, drop_p=P_DROP, drop_seed=c["seed"] + 1)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(logits, again)) and not torch.equal(logits[1], other[1])


@pytest.mark.parametrize("N,D", CASES)
def test_pair_heads_wide_train_launches_are_repeatable(ops, N, D):
    """Three launches of the train-mode call on the same inputs agree bit for bit in the loss partials and the dlogits."""
    c = _case(N, D)
    wp = ops.pair_heads_pack(DT, c["w1"], c["w2"])
    first = None
    for _ in range(3):
        _, partials, dlog = ops.pair_heads_fwd(c["ab"], wp, c["b1"], c["b2"], CLASSES, want_logits=False, tags=c["tags"],
                                               class_weights=c["cw"], want_dlogits=True, drop_p=P_DROP, drop_seed=77)
        torch.cuda.synchronize()
        cur = [partials.clone()] + [d.clone() for d in dlog]
        if first is None:
            first = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(cur, first))
