"""Host side of the batched spot decode (no GPU): the C ABI entries are bound, the workspace query behaves, and the graph walk
takes already compacted spot lists in place of score maps."""
import ctypes
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")


def test_batch_symbols_are_bound_and_the_descriptor_mirrors_the_header():
    from peneo_amd import hip
    for name in ("peneo_spots_compact_batch_workspace_bytes", "peneo_spots_compact_batch"):
        assert name in hip.SIGNATURES
    lib = hip.load_library()
    assert lib.peneo_spots_compact_batch.argtypes[0] == ctypes.POINTER(hip.SpotsBatchDesc)
    # int num_maps; int classes[8]; (4 bytes of padding) const void* maps[8]
    assert ctypes.sizeof(hip.SpotsBatchDesc) == 4 + 4 * hip.MAX_HEADS + 4 + 8 * hip.MAX_HEADS
    assert hip.SpotsBatchDesc.maps.offset == 40


def test_workspace_query_is_positive_and_non_decreasing():
    from peneo_amd import hip
    ws = hip.load_library().peneo_spots_compact_batch_workspace_bytes
    sizes = (1, 2, 63, 91, 130, 511, 1221)
    for m in range(1, hip.MAX_HEADS + 1):
        for b in (1, 2, 8, 64):
            prev = 0
            for n in sizes:
                v = ws(m, b, n)
                assert v > 0 and v >= prev, (m, b, n, v)
                prev = v
                if m > 1:
                    assert v >= ws(m - 1, b, n)
                if b > 1:
                    assert v >= ws(m, b // 2, n)
    # one int32 per (map, document, segment): at least one segment per 130 816 pairs, at most one per pair
    assert 5 * 8 * 4 <= ws(5, 8, 511) <= 5 * 8 * 130816 * 4
    # out of range: nothing to size
    assert ws(0, 1, 5) == 0 and ws(hip.MAX_HEADS + 1, 1, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 1, 0) == 0


def test_spot_lists_pass_through_the_tagging_scheme():
    from peneo_amd.model import HandshakingTaggingScheme as H
    spots = [(0, 3, 1, 0.75), (2, 2, 2, 0.5)]
    assert H.get_spots_from_shaking_tag(spots, seq_len=5) is spots
    assert H.get_spots_from_shaking_tag([], seq_len=5) == []
    # host tensors: the batch form is the per-document form, map by map
    g = torch.Generator().manual_seed(3)
    n = 9
    P = n * (n + 1) // 2
    logits = torch.randn(2, P, 3, generator=g)
    tags = torch.randint(0, 3, (2, P), generator=g)
    got = H.get_spots_from_shaking_tags_batch([logits, tags], n)
    assert got == [[H.get_spots_from_shaking_tag(m[b], seq_len=n) for b in range(2)] for m in (logits, tags)]
    assert H.get_spots_from_shaking_tags_batch([], n) == []


def test_decode_takes_the_reference_spot_lists_in_place_of_score_maps():
    """``sample_decode_peneo`` fed the reference's own spot lists of the two-page fixture returns the reference's decode."""
    from peneo_amd.model import HandshakingTaggingScheme
    from peneo_amd.pipeline.decode import decode_peneo, sample_decode_peneo
    fx = torch.load(os.path.join(HERE, "golden", "rfund_plumbing.pt"), weights_only=False)
    ev = fx["eval"]
    tagger = HandshakingTaggingScheme()
    for b in range(2):
        lists = [[tuple(s) for s in ev["spots"][h][b]] for h in HEADS]
        assert all(isinstance(l, list) for l in lists)
        got = sample_decode_peneo(tagger, fx["batch"]["text"][b], *lists, seq_len=511, decode_gt=False)
        assert got == ev["decode"]["pred"][b], b
    assert sum(len(p[0]) for p in ev["decode"]["pred"]) > 0
    # the batch form, spot lists on both sides (predictions as ground truth: decode_gt keeps the first successor)
    per_head = [[[tuple(s) for s in ev["spots"][h][b]] for b in range(2)] for h in HEADS]
    preds, gts, ids = decode_peneo(tagger, fx["batch"]["text"], *per_head, *per_head, [[0] * 511] * 2, ["a", "b"])
    assert preds == list(ev["decode"]["pred"]) and ids == ["a", "b"] and len(gts) == 2
