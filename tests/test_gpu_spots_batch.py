"""Batched spot decode (peneo_spots_compact_batch, csrc/spots.hip) against the per-map kernel it stands beside:
records and counts must equal ``ops.spots_compact`` on every [P, C] slice bit for bit, scores included, and nothing may be
written behind a (map, document)'s stored records."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = -7          # fill of records / counts before a launch: no record field and no count is ever -7


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


def make_logits(B, N, classes, seed):
    """randn with +4.0 on class 0 (about 0.5 % spots) and a planted spot at p = 0 and at p = P - 1 of every map and document."""
    P = N * (N + 1) // 2
    g = torch.Generator().manual_seed(seed)
    maps = []
    for C in classes:
        l = torch.randn(B, P, C, generator=g)
        l[..., 0] += 4.0
        l[:, 0, 1] = 9.0
        l[:, P - 1, C - 1] = 9.5
        maps.append(l.to(DEV))
    return maps


def launch(ops, maps, N, max_spots):
    """guard-filled outputs -> (records [M, B, max_spots, 4] int32, counts [M, B]) on the host"""
    M, B = len(maps), maps[0].shape[0]
    records = torch.full((M, B, max(max_spots, 1), 4), GUARD, dtype=torch.int32, device=DEV)
    counts = torch.full((M, B), GUARD, dtype=torch.int32, device=DEV)
    ops.spots_compact_batch_launch(maps, N, max_spots, records=records, counts=counts)
    return records.cpu(), counts.cpu()


def check_against_per_map(ops, maps, N, records, counts, max_spots):
    for m, lg in enumerate(maps):
        for b in range(lg.shape[0]):
            spots, scores = ops.spots_compact(lg[b], N, max_spots=max_spots)
            n = spots.shape[0]
            assert int(counts[m, b]) == n, (m, b)
            k = min(n, max_spots)
            assert torch.equal(records[m, b, :k, :3], spots.cpu()[:k]), (m, b)
            assert torch.equal(records[m, b, :k, 3], scores.cpu().view(torch.int32)[:k]), (m, b)     # the same bits
            assert bool((records[m, b, k:] == GUARD).all()), (m, b)


@pytest.mark.parametrize("classes", [(2, 3, 3, 3, 3), (5,), (3,) * 8], ids=["heads", "one5", "eight"])
@pytest.mark.parametrize("B,N", [(1, 1), (1, 2), (2, 63), (3, 91), (2, 130), (2, 511)])
def test_batch_equals_the_per_map_kernel(ops, B, N, classes):
    maps = make_logits(B, N, classes, seed=B * 1000 + N)
    records, counts = launch(ops, maps, N, 4096)
    P = N * (N + 1) // 2
    assert int(counts.min()) >= 1 and int(counts.max()) <= 4096
    for m in range(len(maps)):                                   # the planted spots are first and last
        for b in range(B):
            n = int(counts[m, b])
            assert records[m, b, 0, :3].tolist() == ([0, 0, 1] if P > 1 else [0, 0, classes[m] - 1])
            assert records[m, b, n - 1, :3].tolist() == [N - 1, N - 1, classes[m] - 1]
    check_against_per_map(ops, maps, N, records, counts, 4096)


def test_dense_map_is_ordered_across_every_segment(ops):
    """N = 130 with every pair a spot: the full ordered list, then a cap of 100."""
    B, N = 2, 130
    P = N * (N + 1) // 2
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(B, P, 3, generator=g)
    lg[..., 0] -= 30.0                                           # class 0 never wins
    maps = [lg.to(DEV)]
    records, counts = launch(ops, maps, N, P)
    assert counts.tolist() == [[P, P]]
    iu = torch.triu_indices(N, N)                                # row-major upper triangle = increasing p
    want_tag = (lg[..., 1:].argmax(-1) + 1).int()
    for b in range(B):
        assert torch.equal(records[0, b, :, 0], iu[0].int()) and torch.equal(records[0, b, :, 1], iu[1].int())
        assert torch.equal(records[0, b, :, 2], want_tag[b])
    check_against_per_map(ops, maps, N, records, counts, P)
    records, counts = launch(ops, maps, N, 100)
    assert counts.tolist() == [[P, P]]
    full, _ = launch(ops, maps, N, P)
    assert torch.equal(records[:, :, :100], full[:, :, :100])
    # a buffer longer than the cap stays untouched behind it.  (In the [M][B][max_spots] layout a write just past document 0's cap
    # lands in document 1's records, not behind the buffer: that is caught by the comparison with the full run above and below.)
    big = torch.full((1, B, 160, 4), GUARD, dtype=torch.int32, device=DEV)
    cnt = torch.full((1, B), GUARD, dtype=torch.int32, device=DEV)
    ops.spots_compact_batch_launch(maps, N, 100, records=big.view(-1)[:B * 100 * 4].view(1, B, 100, 4), counts=cnt)
    big = big.cpu().view(-1)
    assert torch.equal(big[:B * 100 * 4].view(1, B, 100, 4), full[:, :, :100]) and bool((big[B * 100 * 4:] == GUARD).all())


def test_empty_map_writes_nothing(ops):
    B, N = 2, 91
    P = N * (N + 1) // 2
    lg = torch.zeros(B, P, 3)
    lg[..., 0] = 1.0
    records, counts = launch(ops, [lg.to(DEV), torch.zeros(B, P, dtype=torch.int64, device=DEV)], N, 64)
    assert counts.tolist() == [[0, 0], [0, 0]] and bool((records == GUARD).all())


def test_ties_and_nan_follow_the_per_map_kernel(ops):
    N = 4
    P = N * (N + 1) // 2
    nan = float("nan")
    rows = [[1.0, 1.0, 1.0],      # all equal: class 0 keeps it, no spot
            [0.0, 2.0, 2.0],      # classes 1 and 2 tie above class 0: tag 1
            [2.0, 2.0, 0.0],      # class 0 ties with class 1: no spot
            [nan, 5.0, 1.0],      # NaN in class 0: nothing is > NaN, no spot
            [0.0, nan, 3.0],      # a NaN never wins: tag 2
            [0.0, 3.0, nan],      # tag 1 (its score is NaN, as in the per-map kernel)
            [0.0, -1.0, nan],     # no spot
            [nan, nan, nan],
            [-1.0, 0.0, 0.5],
            [3.0, 0.0, 0.5]]
    assert len(rows) == P
    lg = torch.tensor([rows, rows[::-1]], dtype=torch.float32).to(DEV)
    records, counts = launch(ops, [lg], N, 16)
    assert records[0, 0, :int(counts[0, 0]), 2].tolist() == [1, 2, 1, 2]
    iu = torch.triu_indices(N, N)
    assert records[0, 0, :4, :2].tolist() == [[int(iu[0, p]), int(iu[1, p])] for p in (1, 4, 5, 8)]
    check_against_per_map(ops, [lg], N, records, counts, 16)


def test_label_maps_and_a_mixed_call(ops):
    B, N = 3, 91
    P = N * (N + 1) // 2
    g = torch.Generator().manual_seed(11)
    tags = [(torch.rand(B, P, generator=g) < 0.02).long() * torch.randint(1, 3, (B, P), generator=g) for _ in range(2)]
    tags[1][:, 0] = 2
    tags[1][:, P - 1] = 1
    logit_maps = make_logits(B, N, (2, 3), seed=12)
    maps = [logit_maps[0], tags[0].to(DEV), logit_maps[1], tags[1].to(DEV)]
    records, counts = launch(ops, maps, N, 512)
    iu = torch.triu_indices(N, N)
    one = torch.tensor(1.0).view(torch.int32)
    for m, t in ((1, tags[0]), (3, tags[1])):
        for b in range(B):
            p = torch.nonzero(t[b])[:, 0]
            n = p.numel()
            assert int(counts[m, b]) == n and 0 < n < 512
            want = torch.stack([iu[0][p].int(), iu[1][p].int(), t[b][p].int(), one.expand(n)], 1)
            assert torch.equal(records[m, b, :n], want)
            assert bool((records[m, b, n:] == GUARD).all())
    check_against_per_map(ops, [maps[0], maps[2]], N, records[[0, 2]], counts[[0, 2]], 512)
    # label maps alone give the same records
    rec2, cnt2 = launch(ops, [maps[1], maps[3]], N, 512)
    assert torch.equal(rec2, records[[1, 3]]) and torch.equal(cnt2, counts[[1, 3]])


def test_wide_label_values_are_spots_and_a_zero_cap_only_counts(ops):
    """spot iff the int64 value != 0: a non-zero multiple of 2^32 is a spot (tag 1: its low 32 bits are zero), other wide values
    keep their low 32 bits; max_spots == 0 needs no records buffer and returns the true counts."""
    B, N = 1, 5
    P = N * (N + 1) // 2
    t = torch.zeros(B, P, dtype=torch.int64)
    t[0, 2], t[0, 7], t[0, 9], t[0, 14] = 1 << 32, (1 << 32) + 2, -1, 3 << 33
    records, counts = launch(ops, [t.to(DEV)], N, 8)
    assert counts.tolist() == [[4]]
    iu = torch.triu_indices(N, N)
    assert records[0, 0, :4, :3].tolist() == [[int(iu[0, p]), int(iu[1, p]), tag] for p, tag in ((2, 1), (7, 2), (9, -1), (14, 1))]
    assert bool((records[0, 0, 4:] == GUARD).all())
    maps = make_logits(2, 63, (2, 3), seed=8)
    _, want = launch(ops, maps, 63, 4096)
    rec0, cnt0 = ops.spots_compact_batch_launch(maps, 63, 0)
    assert rec0.numel() == 0 and torch.equal(cnt0.cpu(), want)


def test_three_launches_are_bit_identical(ops):
    maps = make_logits(2, 511, (2, 3, 3, 3, 3), seed=21)
    runs = [launch(ops, maps, 511, 4096) for _ in range(3)]
    for r, c in runs[1:]:
        assert torch.equal(r, runs[0][0]) and torch.equal(c, runs[0][1])


def test_bad_arguments_are_refused_and_nothing_is_written(ops):
    from peneo_amd import hip
    lib = hip.lib()
    B, N, cap = 2, 20, 32
    P = N * (N + 1) // 2
    lg = make_logits(B, N, (3,), seed=4)[0]
    one_class = torch.zeros(B, P, 1, device=DEV)
    records = torch.full((1, B, cap, 4), GUARD, dtype=torch.int32, device=DEV)
    counts = torch.full((1, B), GUARD, dtype=torch.int32, device=DEV)
    need = lib.peneo_spots_compact_batch_workspace_bytes(1, B, N)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)

    def call(num_maps=1, ptr0=lg.data_ptr(), classes0=3, b=B, n=N, max_spots=cap, wsp=ws.data_ptr(), wsb=need):
        d = hip.SpotsBatchDesc()
        d.num_maps = num_maps
        d.classes[0] = classes0
        d.maps[0] = ptr0
        for m in range(1, hip.MAX_HEADS):
            d.classes[m], d.maps[m] = 3, lg.data_ptr()
        return lib.peneo_spots_compact_batch(ctypes.byref(d), b, n, records.data_ptr(), counts.data_ptr(), max_spots, wsp, wsb,
                                             hip.stream())

    bad = {"null map": dict(ptr0=None), "no maps": dict(num_maps=0), "too many maps": dict(num_maps=hip.MAX_HEADS + 1),
           "one class": dict(ptr0=one_class.data_ptr(), classes0=1), "negative classes": dict(classes0=-1),
           "short workspace": dict(wsb=need - 1), "null workspace": dict(wsp=None), "negative cap": dict(max_spots=-1),
           "B = 0": dict(b=0), "N = 0": dict(n=0)}
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"peneo_spots_compact_batch" in lib.peneo_last_error(), what
    torch.cuda.synchronize()
    assert bool((records == GUARD).all()) and bool((counts == GUARD).all()) and bool((ws == 0x5A).all())
    assert call() == 0                                                       # the same call with nothing wrong
    torch.cuda.synchronize()
    check_against_per_map(ops, [lg], N, records.cpu(), counts.cpu(), cap)


def test_python_layers_regrow_and_match_the_per_document_call(ops):
    from peneo_amd.model import HandshakingTaggingScheme as H
    B, N = 2, 63
    maps = make_logits(B, N, (2, 3), seed=31)
    rec, cnt = ops.spots_compact_batch(maps, N, max_spots=4)                 # forces the repeat with the largest count
    assert not rec.is_cuda and not cnt.is_cuda and int(cnt.max()) > 4 and rec.shape == (int(cnt.sum()), 4)
    at = 0
    for m, lg in enumerate(maps):                                            # packed: (map, document) after (map, document)
        for b in range(B):
            spots, scores = ops.spots_compact(lg[b], N)
            n = int(cnt[m, b])
            assert n == spots.shape[0]
            assert torch.equal(rec[at:at + n, :3], spots.cpu()) and torch.equal(rec[at:at + n, 3], scores.cpu().view(torch.int32))
            at += n
    tags = (torch.rand(B, N * (N + 1) // 2) < 0.05).long().to(DEV) * 2
    ftags = torch.zeros(B, 6, device=DEV)                                    # a floating label map (N = 3): 0.5 is a spot with tag 0
    ftags[:, 1], ftags[:, 4] = 0.5, 2.0
    assert H.get_spots_from_shaking_tags_batch([ftags], 3) == [[[(0, 1, 0, 1.0), (1, 2, 2, 1.0)]] * B]
    every = maps + [tags, tags.int().unsqueeze(-1)]
    got = H.get_spots_from_shaking_tags_batch(every, N)
    want = [[H.get_spots_from_shaking_tag(m[b], seq_len=N) for b in range(B)] for m in every]
    assert got == want and all(len(w) > 0 for per_map in want for w in per_map)
