"""MXFP8 pair heads at decoder widths 512 < D <= 1024 (pair_heads_mx_wide.hip): the fused kernel against the torch emulation of
the numeric contract it shares with peneo_pair_heads_fwd_mxfp8 (tests/test_gpu_pair_mxfp8.py: the emulation, the cases and the
bounds are that file's), the loss rows, repeatability and the refusals of the C entry points.  B = 2 throughout."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_pair_mxfp8 import CLASSES, DEV, check_close, emulate_logits, make_case

pytestmark = pytest.mark.gpu

# (22: P = 253, one partly filled workgroup; 23: P = 276, a second workgroup with 20 live pairs; 33 / 130: several workgroups, the
# last partly filled; then one case at each of the eight widths)
SHAPES = [(22, 768), (23, 768), (33, 768), (130, 768), (71, 960), (70, 1024)] + \
         [(70, D) for D in (576, 640, 704, 768, 832, 896, 960)]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _case(N, D, wide=False):
    """(inputs, packed weights) of a shape, made once"""
    from peneo_amd import ops as o
    case = make_case(N, D, N * 7 + D, wide=wide)
    return case, o.pair_heads_pack_mxfp8_wide(case[1], case[2])


@pytest.mark.parametrize("N,D", SHAPES)
def test_fused_kernel_matches_the_emulation(ops, N, D):
    (ab, w1, w2, b1, b2), wp = _case(N, D)
    logits, _, _ = ops.pair_heads_fwd_mxfp8_wide(ab, wp, b1, b2, CLASSES)
    P = N * (N + 1) // 2
    assert [tuple(l.shape) for l in logits] == [(2, P, c) for c in CLASSES]
    check_close(logits, emulate_logits(ab, w1, b1, w2, b2))


@pytest.mark.parametrize("D", [960, 1024])
def test_fused_kernel_with_wide_channel_range(ops, D):
    """15 and 16 k-steps: a partly filled and a full last scale word, every scale-byte selector in use; with channels spanning five
    decades the block scales differ, so a wrong block-to-scale pairing shows"""
    (ab, w1, w2, b1, b2), wp = _case(70, D, wide=True)
    logits, _, _ = ops.pair_heads_fwd_mxfp8_wide(ab, wp, b1, b2, CLASSES)
    check_close(logits, emulate_logits(ab, w1, b1, w2, b2), rel_to_max=True)


def test_loss_partials_match_cross_entropy_on_the_kernels_logits(ops):
    N, D = 130, 768
    (ab, w1, w2, b1, b2), wp = _case(N, D)
    P = N * (N + 1) // 2
    g = torch.Generator().manual_seed(9)
    tags = [torch.randint(0, c, (2, P), generator=g).to(DEV) for c in CLASSES]
    tags[1][0, :5] = -100                                                   # ignored labels carry no weight
    tags[3][1, -3:] = -100                                                  # ... in the last, partly filled workgroup too
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device=DEV) for c in CLASSES]
    logits, partials, _ = ops.pair_heads_fwd_mxfp8_wide(ab, wp, b1, b2, CLASSES, tags=tags, class_weights=cw)
    assert partials.shape == (ops.lib().peneo_pair_loss_partials(2, N), 32)
    tot = partials.double().sum(0)
    for h in range(len(CLASSES)):
        want = F.cross_entropy(logits[h].reshape(-1, CLASSES[h]).double(), tags[h].reshape(-1), weight=cw[h].double(),
                               reduction="sum", ignore_index=-100)
        den = cw[h].double()[tags[h][tags[h] >= 0]].sum()
        assert abs(float(tot[h]) - float(want)) <= 1e-4 * abs(float(want))
        assert abs(float(tot[8 + h]) - float(den)) <= 1e-4 * float(den)
    none, partials2, _ = ops.pair_heads_fwd_mxfp8_wide(ab, wp, b1, b2, CLASSES, want_logits=False, tags=tags, class_weights=cw)
    assert none is None and torch.equal(partials, partials2)
    # peneo_loss_finish reads the rows unchanged
    out, _, _ = ops.loss_finish(partials, torch.ones(len(CLASSES), device=DEV), sum(CLASSES))
    for h in range(len(CLASSES)):
        assert abs(float(out[h]) - float(tot[h] / tot[8 + h])) <= 1e-5 * abs(float(tot[h] / tot[8 + h]))


def test_three_launches_are_bit_identical(ops):
    N, D = 130, 768
    (ab, w1, w2, b1, b2), wp = _case(N, D)
    P = N * (N + 1) // 2
    g = torch.Generator().manual_seed(1)
    tags = [torch.randint(0, c, (2, P), generator=g).to(DEV) for c in CLASSES]
    ref = None
    for _ in range(3):
        logits, partials, _ = ops.pair_heads_fwd_mxfp8_wide(ab, wp, b1, b2, CLASSES, tags=tags)
        cur = [partials.clone()] + [l.clone() for l in logits]
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(cur, ref))


def _raw_fwd(entry, ab, wp, b1, b2, drop_p=0.0, loss=None):
    """a forward entry point through the C ABI directly: (return code, peneo_last_error)"""
    from peneo_amd import hip
    B, N, D2 = ab.shape
    desc = hip.PairHeadsDesc()
    desc.num_heads, desc.D = len(CLASSES), D2 // 2
    for h, c in enumerate(CLASSES):
        desc.classes[h] = c
    desc.w_packed, desc.b1, desc.b2 = hip.ptr(wp), hip.ptr(b1), hip.ptr(b2)
    desc.drop_p, desc.drop_seed = drop_p, 1
    pl = None
    if loss is not None:
        tags, dlog, partials = loss
        pl = hip.PairLoss()
        for h in range(len(CLASSES)):
            pl.tags[h] = hip.ptr(tags[h])
            pl.dlogits[h] = hip.ptr(dlog[h]) if dlog is not None else None
        pl.partials = hip.ptr(partials)
    rc = getattr(hip.lib(), entry)(hip.ptr(ab), B, N, ctypes.byref(desc), None, ctypes.byref(pl) if pl is not None else None,
                                   hip.stream())
    return rc, (hip.lib().peneo_last_error() or b"").decode()


def test_unsupported_arguments_are_refused(ops):
    WIDE, NARROW = "peneo_pair_heads_fwd_mxfp8_wide", "peneo_pair_heads_fwd_mxfp8"
    N = 22
    (ab, w1, w2, b1, b2), wp = _case(N, 768)
    P = N * (N + 1) // 2
    tags = [torch.zeros((2, P), dtype=torch.int64, device=DEV) for _ in CLASSES]
    dlog = [torch.empty((2, P, c), dtype=torch.float32, device=DEV) for c in CLASSES]
    partials = torch.empty((ops.lib().peneo_pair_loss_partials(2, N), 32), dtype=torch.float32, device=DEV)
    rc, msg = _raw_fwd(WIDE, ab, wp, b1, b2, drop_p=0.1)
    assert rc == -1 and "drop_p" in msg, (rc, msg)                      # PENEO_ERR_INVALID
    rc, msg = _raw_fwd(WIDE, ab, wp, b1, b2, loss=(tags, dlog, partials))
    assert rc == -1 and "dlogits" in msg, (rc, msg)
    rc, msg = _raw_fwd(WIDE, ab, wp, b1, b2, loss=(tags, None, partials))  # the same call without them is accepted
    torch.cuda.synchronize()
    assert rc == 0, msg
    # widths: 512 and 1088 handed to the wide entry point, 768 to the narrow one (nothing is launched: the buffers are not read)
    for D in (512, 1088):
        bad = torch.zeros(2, N, 2 * D, dtype=torch.bfloat16, device=DEV)
        rc, msg = _raw_fwd(WIDE, bad, wp, b1, b2)
        assert rc == -1 and f"D={D}" in msg and "peneo_pair_mxfp8_wide_supported" in msg, (rc, msg)
    rc, msg = _raw_fwd(NARROW, ab, wp, b1, b2)
    assert rc == -1 and "D=768" in msg, (rc, msg)
    # the wrappers: a pack of another shape, a width without a kernel
    with pytest.raises(ValueError):
        ops.pair_heads_fwd_mxfp8_wide(ab, wp[:-4096], b1, b2, CLASSES)
    with pytest.raises(ValueError):
        ops.pair_heads_pack_mxfp8_wide([w[:512, :512].contiguous() for w in w1], [w[:, :512].contiguous() for w in w2])
    with pytest.raises(ValueError):
        ops.pair_heads_pack_mxfp8(w1, w2)
