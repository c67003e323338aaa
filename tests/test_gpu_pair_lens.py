"""peneo_pair_heads_fwd_lens / peneo_pair_lens_from_mask on the GPU, op level.

Shape: N = 40 (P = 820: four workgroups of 256 pairs a document), B = 5 with lens = [40, 23, 1, 0, 37], i.e. P_b = 820, 276, 1, 0,
703: a full document, one workgroup plus a ragged second, a single pair, an empty document and a ragged last workgroup.  Five heads
with classes 2, 3, 3, 3, 3.  Kernels: the generic one ((bf16, 64), (fp32, 64)), the hand-interleaved one ((bf16, 384), (bf16, 512))
and the four-wave one ((bf16, 768)).  The reference is ops.pair_heads_fwd on the same inputs (bit for bit), computed once per case."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
CLASSES = [2, 3, 3, 3, 3]
N, LENS = 40, [40, 23, 1, 0, 37]
B, P = len(LENS), N * (N + 1) // 2
WG = 256                                       # pairs per workgroup == per row of loss partials
G = -(-P // WG)
KERNELS = [(BF16, 64), (F32, 64), (BF16, 384), (BF16, 512), (BF16, 768)]
IDS = [f"{'bf16' if dt == BF16 else 'fp32'}-{D}" for dt, D in KERNELS]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


def _row_start(i, n):
    return i * n - i * (i - 1) // 2


def _packed(n):
    """N-packed indices of the pairs of an n-token document, in the order of its own triangle (q = 0 .. n (n + 1) / 2 - 1)"""
    ii, jj = torch.triu_indices(n, n)
    return (ii * N - ii * (ii - 1) // 2 + (jj - ii)).to(DEV)


def _live_mask():
    """[B, P] bool: pair (i, j) of document b has j < lens[b]"""
    jj = torch.triu_indices(N, N)[1]
    return (jj[None, :] < torch.tensor(LENS)[:, None]).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(dtype, D):
    """inputs and the plain call's results of one case; never modified"""
    from peneo_amd import ops
    g = torch.Generator().manual_seed(1000 + D + (1 if dtype == F32 else 0))
    ab = torch.randn(B, N, 2 * D, generator=g).to(DEV).to(dtype)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    b1 = torch.cat([0.1 * torch.randn(D, generator=g).to(DEV) for _ in CLASSES])
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).to(DEV) for c in CLASSES]
    b2 = torch.cat([0.1 * torch.randn(c, generator=g).to(DEV) for c in CLASSES])
    tags = [torch.randint(0, c, (B, P), generator=g).to(DEV) for c in CLASSES]
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device=DEV) for c in CLASSES]
    wp = ops.pair_heads_pack(dtype, w1, w2)
    logits, partials, _ = ops.pair_heads_fwd(ab, wp, b1, b2, CLASSES, tags=tags, class_weights=cw)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    return dict(ab=ab, wp=wp, b1=b1, b2=b2, tags=tags, cw=cw, logits=logits, partials=partials, lens=lens, live=_live_mask())


def _nan_maps():
    return [torch.full((B, P, c), float("nan"), dtype=torch.float32, device=DEV) for c in CLASSES]


@pytest.mark.parametrize("dtype,D", KERNELS, ids=IDS)
def test_live_pairs_are_the_plain_logits_and_the_padding_is_background(ops, dtype, D):
    c = _case(dtype, D)
    live = c["live"]
    assert live.sum(1).tolist() == [n * (n + 1) // 2 for n in LENS]
    out = _nan_maps()                                        # an element the call leaves unwritten stays NaN
    logits, partials, dlog = ops.pair_heads_fwd_lens(c["ab"], c["lens"], c["wp"], c["b1"], c["b2"], CLASSES, logits_out=out)
    assert partials is None and dlog is None
    pad = torch.tensor(ops.PAIR_PAD_LOGIT, dtype=torch.float32, device=DEV)
    for h, k in enumerate(CLASSES):
        assert logits[h] is out[h]
        assert bool(torch.isfinite(logits[h]).all()), f"head {h}: an element was left unwritten"
        assert torch.equal(logits[h][live], c["logits"][h][live]), f"head {h}: live logits differ from pair_heads_fwd"
        bg = torch.cat([torch.zeros(1, device=DEV), pad.expand(k - 1)])
        padded = logits[h][~live]
        assert padded.shape[0] == B * P - int(live.sum()) and torch.equal(padded, bg.expand_as(padded)), f"head {h}: padding"
    # fresh maps (no caller buffer) carry the same bits, with the loss requested beside them too
    again, _, _ = ops.pair_heads_fwd_lens(c["ab"], c["lens"], c["wp"], c["b1"], c["b2"], CLASSES, tags=c["tags"], class_weights=c["cw"])
    for h in range(len(CLASSES)):
        assert torch.equal(again[h], logits[h])


@pytest.mark.parametrize("dtype,D", KERNELS, ids=IDS)
def test_full_lengths_are_the_plain_call_bit_for_bit(ops, dtype, D):
    c = _case(dtype, D)
    for full in (N, N + 9):                                  # lengths above N are clamped to N
        lens = torch.full((B,), full, dtype=torch.int32, device=DEV)
        logits, partials, _ = ops.pair_heads_fwd_lens(c["ab"], lens, c["wp"], c["b1"], c["b2"], CLASSES, tags=c["tags"],
                                                      class_weights=c["cw"], logits_out=_nan_maps())
        for h in range(len(CLASSES)):
            assert torch.equal(logits[h], c["logits"][h]), h
        assert partials.shape == c["partials"].shape == (B * G, 32)
        assert torch.equal(partials, c["partials"])


@pytest.mark.parametrize("dtype,D", KERNELS, ids=IDS)
def test_loss_rows_are_those_of_the_cropped_documents(ops, dtype, D):
    """The compact walk of document b is the plain walk of that document cropped to n_b tokens: partial rows equal row by row."""
    c = _case(dtype, D)
    parts = []
    for want_logits in (False, True):
        _, partials, _ = ops.pair_heads_fwd_lens(c["ab"], c["lens"], c["wp"], c["b1"], c["b2"], CLASSES, want_logits=want_logits,
                                                 tags=c["tags"], class_weights=c["cw"])
        assert partials.shape == (ops.lib().peneo_pair_loss_partials(B, N), 32) == (B * G, 32)
        parts.append(partials)
    assert torch.equal(parts[0], parts[1])
    partials = parts[0]
    assert bool(torch.isfinite(partials).all())
    cropped = []
    for b, n in enumerate(LENS):
        rows = partials[b * G:(b + 1) * G]
        used = -(-(n * (n + 1) // 2) // WG)
        if n > 0:
            idx = _packed(n)
            tags_n = [t[b:b + 1, idx].contiguous() for t in c["tags"]]
            _, ref, _ = ops.pair_heads_fwd(c["ab"][b:b + 1, :n].contiguous(), c["wp"], c["b1"], c["b2"], CLASSES, want_logits=False,
                                           tags=tags_n, class_weights=c["cw"])
            assert ref.shape == (used, 32)
            assert torch.equal(rows[:used], ref), f"document {b} (n = {n})"
            cropped.append(ref)
        assert float(rows[used:].abs().max() if used < G else 0.0) == 0.0, f"document {b}: rows of idle workgroups"
        assert torch.equal(rows[used:], torch.zeros_like(rows[used:]))
    ratio = torch.ones(len(CLASSES), device=DEV)
    got, _, _ = ops.loss_finish(partials, ratio, sum(CLASSES))
    want, _, _ = ops.loss_finish(torch.cat(cropped).contiguous(), ratio, sum(CLASSES))
    rel = ((got - want).abs() / want.abs()).max()
    print(f"loss_finish lens vs cropped: {got.tolist()} vs {want.tolist()}, rel {float(rel):.3e}")
    assert float(rel) < 1e-5
    # and they are the live-pair losses: a float64 class-weighted CE over the pairs with j < n_b
    for h, k in enumerate(CLASSES):
        lg, tg = c["logits"][h][c["live"]].double(), c["tags"][h][c["live"]]
        w = c["cw"][h].double()[tg]
        nll = torch.logsumexp(lg, -1) - lg.gather(-1, tg[:, None])[:, 0]
        ref64 = float((w * nll).sum() / w.sum())
        assert abs(float(got[h]) - ref64) < 1e-4 * max(1.0, abs(ref64)), (h, float(got[h]), ref64)


def test_lens_from_mask(ops):
    rows = [[1, 1, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]]
    mask = torch.tensor(rows, dtype=torch.int64, device=DEV)
    lens = ops.pair_lens_from_mask(mask, 6)
    assert lens.dtype == torch.int32 and lens.device == mask.device and lens.shape == (5,)
    assert lens.tolist() == [4, 0, 6, 3, 1]                  # a mask with a hole: a superset of its tokens, never a subset
    assert ops.pair_lens_from_mask(mask, 3).tolist() == [2, 0, 3, 3, 1]          # positions from N on are not looked at
    # a cropped view of a wider mask (the decoder's case: row stride above N), other integer dtypes and bool
    wide = torch.zeros(5, 9, dtype=torch.int64, device=DEV)
    wide[:, 1:7] = mask
    wide[:, 7:] = 1
    assert ops.pair_lens_from_mask(wide[:, 1:7], 6).tolist() == [4, 0, 6, 3, 1]
    assert ops.pair_lens_from_mask(mask.to(torch.int32), 6).tolist() == [4, 0, 6, 3, 1]
    assert ops.pair_lens_from_mask(mask.bool(), 6).tolist() == [4, 0, 6, 3, 1]
    # more than one pass of the 256 threads, the last token in the last position, and a single early one
    long = torch.zeros(3, 700, dtype=torch.int64, device=DEV)
    long[0, :513] = 1
    long[1, 699] = 1
    long[2, 5] = 1
    assert ops.pair_lens_from_mask(long, 700).tolist() == [513, 700, 6]
    # no mask: every length is N
    assert ops.pair_lens_from_mask(None, 40, B=3, device=DEV).tolist() == [40, 40, 40]


def _raw_call(ops, c, D, *, drop_p=0.0, dlogits=False, lens="ok", dtype_code=None, heads=None):
    """peneo_pair_heads_fwd_lens through the C ABI itself (what ops.pair_heads_fwd_lens cannot ask for)"""
    from peneo_amd import hip
    nh = len(CLASSES) if heads is None else heads
    desc = hip.PairHeadsDesc()
    desc.num_heads, desc.D = nh, D
    for h, k in enumerate(CLASSES):
        desc.classes[h] = k
    desc.w_packed, desc.b1, desc.b2 = hip.ptr(c["wp"]), hip.ptr(c["b1"]), hip.ptr(c["b2"])
    desc.drop_p, desc.drop_seed = drop_p, 7
    maps = _nan_maps()
    arr = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    loss, keep = None, []
    if dlogits:
        loss = hip.PairLoss()
        partials = torch.empty((B * G, 32), dtype=torch.float32, device=DEV)
        dl = [torch.empty((B, P, k), dtype=torch.float32, device=DEV) for k in CLASSES]
        for h in range(len(CLASSES)):
            loss.tags[h], loss.class_weight[h] = hip.ptr(c["tags"][h]), hip.ptr(c["cw"][h])
        loss.dlogits[len(CLASSES) - 1] = hip.ptr(dl[-1])     # one is enough
        loss.partials = hip.ptr(partials)
        keep = [partials, dl]
    rc = hip.lib().peneo_pair_heads_fwd_lens(hip.dtype_code(c["ab"].dtype) if dtype_code is None else dtype_code, hip.ptr(c["ab"]), B, N,
                                             hip.ptr(c["lens"]) if lens == "ok" else None, C.byref(desc), arr,
                                             C.byref(loss) if loss is not None else None, hip.stream())
    torch.cuda.synchronize()
    del keep
    return rc, maps


def test_refusals_name_the_function_and_launch_nothing(ops):
    from peneo_amd import hip
    from peneo_amd.hip import PeneoHipError
    D = 64
    c = _case(BF16, D)
    for kw, text in ((dict(drop_p=0.1), "drop_p"), (dict(dlogits=True), "dlogits"), (dict(lens=None), "lens"),
                     (dict(dtype_code=5), "peneo_pair_heads_fwd_lens"), (dict(heads=9), "heads")):
        rc, maps = _raw_call(ops, c, D, **kw)
        assert rc == -1, kw                                  # PENEO_ERR_INVALID
        with pytest.raises(PeneoHipError, match="peneo_pair_heads_fwd_lens.*" + text):
            hip.check(rc, "peneo_pair_heads_fwd_lens")
        assert all(bool(torch.isnan(m).all()) for m in maps), f"{kw}: something was launched"
    # an unsupported width: D = 320 has no kernel (bf16 ab of that width, weights never read)
    ab = torch.zeros(B, N, 2 * 320, dtype=BF16, device=DEV)
    with pytest.raises(PeneoHipError, match="peneo_pair_heads_fwd_lens.*D=320"):
        ops.pair_heads_fwd_lens(ab, c["lens"], c["wp"], torch.zeros(5 * 320, device=DEV), c["b2"], CLASSES)
    # ... and the same call that is in order goes through
    rc, maps = _raw_call(ops, c, D)
    assert rc == 0 and all(bool(torch.isfinite(m).all()) for m in maps)
    # lens of the wrong dtype, device, shape: refused by ops before anything is launched
    for bad in (c["lens"].long(), c["lens"].cpu(), c["lens"][:3].contiguous(), c["lens"].float(), LENS):
        with pytest.raises(PeneoHipError, match="pair_heads_fwd_lens"):
            ops.pair_heads_fwd_lens(c["ab"], bad, c["wp"], c["b1"], c["b2"], CLASSES)


def test_launches_nothing_order_dependent_and_survives_graph_capture(ops):
    """No allocation, no synchronisation, no workspace: the call (lens from a mask included) can be captured and replayed."""
    from peneo_amd import hip
    D = 64
    c = _case(BF16, D)
    before = hip.order_dependent_launches()
    mask = (torch.arange(N, device=DEV)[None, :] < c["lens"][:, None]).long()
    lens = torch.zeros(B, dtype=torch.int32, device=DEV)
    maps = _nan_maps()
    desc = hip.PairHeadsDesc()
    desc.num_heads, desc.D = len(CLASSES), D
    for h, k in enumerate(CLASSES):
        desc.classes[h] = k
    desc.w_packed, desc.b1, desc.b2 = hip.ptr(c["wp"]), hip.ptr(c["b1"]), hip.ptr(c["b2"])
    arr = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip.check(hip.lib().peneo_pair_lens_from_mask(hip.ptr(mask), mask.stride(0), B, N, hip.ptr(lens), hip.stream()))
            hip.check(hip.lib().peneo_pair_heads_fwd_lens(hip.BF16, hip.ptr(c["ab"]), B, N, hip.ptr(lens), C.byref(desc), arr, None,
                                                          hip.stream()))
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert lens.tolist() == LENS
    want, _, _ = ops.pair_heads_fwd_lens(c["ab"], c["lens"], c["wp"], c["b1"], c["b2"], CLASSES)
    for h in range(len(CLASSES)):
        assert torch.equal(maps[h], want[h])
    assert hip.order_dependent_launches() == before
