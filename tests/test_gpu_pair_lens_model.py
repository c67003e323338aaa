"""PEneoModel.set_skip_padded_pairs: an eval forward with the switch on against the default path on the same batch - the
maps on the live pairs, the background elsewhere, the decoded spots, the live-pair losses; forwards with gradients untouched in every
bit; LiLT; and prediction_loop on the two-page fixture.  The 2-layer base-width models of the MXFP8 tests (decoder width 384: the
hand-interleaved kernel), bf16, B = 4 at 48 tokens (N = 47) with the mask tails zeroed to decoder lengths N, N - 1, 28 and 1."""
import pytest
import torch

from test_gpu_pair_mxfp8 import OUT_KEYS, _model
from test_rfund_plumbing import _dataset, fx, tok  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SEQ = 48
N = SEQ - 1
LENS = [N, N - 1, 28, 1]
P = N * (N + 1) // 2
CLASSES = (2, 3, 3, 3, 3)
TAG_KEYS = ("line_extraction_shaking_tag", "ent_linking_head_rel_shaking_tag", "ent_linking_tail_rel_shaking_tag",
            "line_grouping_head_rel_shaking_tag", "line_grouping_tail_rel_shaking_tag")
LOSS_KEYS = ["line_extraction_loss", "ent_linking_h2h_loss", "ent_linking_t2t_loss", "line_grouping_h2h_loss", "line_grouping_t2t_loss"]
PAD = -1e30


def _batch(pcfg, backbone):
    from peneo_amd.data import synthetic_rfund_batch
    b = synthetic_rfund_batch(len(LENS), SEQ, 10, pcfg["backbone_config"]["vocab_size"], seed=6)
    if backbone == "lilt":
        b.pop("image", None)
    assert b["attention_mask"].shape == (len(LENS), SEQ) and bool(b["attention_mask"].all())
    for k, n in enumerate(LENS):                             # position 0 is the CLS token the model crops
        b["attention_mask"][k, n + 1:] = 0
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def _live():
    """[B, P] bool on the device: pair (i, j) of document b has j < LENS[b]"""
    jj = torch.triu_indices(N, N)[1]
    return (jj[None, :] < torch.tensor(LENS)[:, None]).cuda()


def _maps(out):
    return [out[k + "_shaking_outputs"] for k in OUT_KEYS]


def _check_maps(on, off, live):
    for k, a, b in zip(CLASSES, on, off):
        assert a.shape == b.shape == (len(LENS), P, k) and a.dtype == torch.float32
        assert torch.equal(a[live], b[live])
        bg = torch.tensor([0.0] + [PAD] * (k - 1), dtype=torch.float32, device=a.device)
        assert torch.equal(a[~live], bg.expand(int((~live).sum()), k))


@pytest.fixture
def calls(monkeypatch):
    from peneo_amd import ops
    seen = {"pair_heads_fwd": 0, "pair_heads_fwd_lens": 0}
    for name in seen:
        real = getattr(ops, name)

        def counting(*a, _real=real, _name=name, **kw):
            seen[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counting)
    return seen


def test_eval_forward_with_the_switch_on(calls):
    from peneo_amd.model.peneo_decoder import HandshakingTaggingScheme as S
    m, pcfg = _model("lmv3")
    batch = _batch(pcfg, "lmv3")
    live = _live()
    with torch.no_grad():
        off = m(**batch)
    assert calls == {"pair_heads_fwd": 1, "pair_heads_fwd_lens": 0}
    spots_off = S.get_spots_from_shaking_tags_batch(_maps(off), N)
    # guard: the default path decodes something in the live region and something in the padding, or nothing below is tested
    flat = [(b, sp) for per_map in spots_off for b, doc in enumerate(per_map) for sp in doc]
    assert any(sp[1] < LENS[b] for b, sp in flat) and any(sp[1] >= LENS[b] for b, sp in flat)
    assert m.set_skip_padded_pairs(True) is m
    with torch.no_grad():
        on = m(**batch)
    assert calls == {"pair_heads_fwd": 1, "pair_heads_fwd_lens": 1}
    _check_maps(_maps(on), _maps(off), live)
    # decoded spots: exactly the default path's with j < n_b, records and scores bit for bit
    spots_on = S.get_spots_from_shaking_tags_batch(_maps(on), N)
    for per_on, per_off in zip(spots_on, spots_off):
        for b, (doc_on, doc_off) in enumerate(zip(per_on, per_off)):
            assert doc_on == [sp for sp in doc_off if sp[1] < LENS[b]], b
    # the returned losses are the live-pair losses: float64 class-weighted CE of the returned maps over the pairs with j < n_b
    dec = m.peneo_decoder
    ratio = dec.loss_ratio if dec.loss_ratio is not None else [1.0] * 5
    total = 0.0
    for h, (key, tag_key) in enumerate(zip(LOSS_KEYS, TAG_KEYS)):
        lg, tg = _maps(on)[h][live].double(), batch[tag_key][live]
        w = (dec.le_loss.weight if h == 0 else dec.link_loss.weight).double()[tg]
        nll = torch.logsumexp(lg, -1) - lg.gather(-1, tg[:, None])[:, 0]
        want = float((w * nll).sum() / w.sum())
        total += ratio[h] * want
        print(f"{key}: live-pair {float(on[key]):.6f} (float64 {want:.6f}), all pairs {float(off[key]):.6f}")
        assert abs(float(on[key]) - want) <= 1e-4, key
    assert abs(float(on["loss"]) - total) <= 1e-4
    # a forward without a mask is today's: the plain launch, the default path's maps in every bit
    nomask = dict(batch, attention_mask=None)
    with torch.no_grad():
        ref = m.set_skip_padded_pairs(False)(**nomask)
        got = m.set_skip_padded_pairs(True)(**nomask)
    assert calls == {"pair_heads_fwd": 3, "pair_heads_fwd_lens": 1}
    for a, b in zip(_maps(got), _maps(ref)):
        assert torch.equal(a, b)
    assert float(got["loss"]) == float(ref["loss"])


def _grad_step(m, batch):
    """eval mode (dropout off), gradients enabled: loss, maps, every gradient"""
    m.zero_grad(set_to_none=True)
    out = m(**batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return out, grads


def test_forward_with_gradients_is_untouched_in_every_bit(calls):
    import peneo_amd
    m, pcfg = _model("lmv3")
    batch = _batch(pcfg, "lmv3")
    with peneo_amd.deterministic(1):                         # (order-independent sums: two runs of one step agree bit for bit)
        off, g_off = _grad_step(m, batch)
        m.set_skip_padded_pairs(True)
        on, g_on = _grad_step(m, batch)
    assert calls == {"pair_heads_fwd": 2, "pair_heads_fwd_lens": 0}
    assert torch.equal(on["loss"], off["loss"])
    for k in LOSS_KEYS:
        assert torch.equal(on[k], off[k]), k
    for a, b in zip(_maps(on), _maps(off)):
        assert torch.equal(a, b)
    assert g_on.keys() == g_off.keys() and len(g_on) > 50
    for n in g_on:
        assert torch.equal(g_on[n], g_off[n]), n


def test_lilt_maps_agree_the_same_way(calls):
    m, pcfg = _model("lilt")
    batch = _batch(pcfg, "lilt")
    with torch.no_grad():
        off = m(**batch)
        on = m.set_skip_padded_pairs(True)(**batch)
    assert calls == {"pair_heads_fwd": 1, "pair_heads_fwd_lens": 1}
    _check_maps(_maps(on), _maps(off), _live())


def test_prediction_loop_on_the_two_page_fixture(fx, tok):  # noqa: F811
    """compact_spots=True with the switch on: the switch-off metrics of the spots outside the padding (all of them, if none is in it)"""
    from torch.utils.data import DataLoader
    from peneo_amd.data import DataCollatorForPEneo
    from peneo_amd.model import PEneoConfig, PEneoModel
    from peneo_amd.pipeline import make_compute_metrics, prediction_loop
    dev = torch.device("cuda:0")
    ds, info = _dataset(tok, "dev", "layoutlmv3-base")
    coll = DataCollatorForPEneo(tokenizer=tok, image_processor=info.image_processor(), max_length=info.max_token_len,
                                require_image=info.image_processor is not None, add_cls_token=info.add_cls_token,
                                add_sep_token=info.add_sep_token)
    model = PEneoModel(PEneoConfig(**{k: v for k, v in fx["config"].items() if k != "model_type"}))
    model.load_state_dict(fx["state_dict"], strict=True)
    model.to(dev).set_compute_dtype(torch.float32).eval()
    mask = coll([ds[0], ds[1]])["attention_mask"][:, 1:]
    lens = [int(r.nonzero().max()) + 1 for r in mask]
    assert len(ds) == 2 and min(lens) < mask.shape[1]         # (at least one page has padding)
    plain = make_compute_metrics()
    dropped = []

    def filtered(pred, epoch):
        maps, rest, file_ids = pred
        kept = tuple([[sp for sp in doc if sp[1] < lens[b]] for b, doc in enumerate(per_map)] for per_map in maps)
        dropped.append(sum(len(doc) for per_map in maps for doc in per_map) - sum(len(doc) for per_map in kept for doc in per_map))
        return plain((kept, rest, file_ids), epoch)

    loader = lambda: DataLoader(ds, batch_size=2, shuffle=False, collate_fn=coll)
    off = prediction_loop(model, loader(), plain, compact_spots=True)
    want = prediction_loop(model, loader(), filtered, compact_spots=True)
    model.set_skip_padded_pairs(True)
    on = prediction_loop(model, loader(), plain, compact_spots=True)
    on_dense = prediction_loop(model, loader(), plain)
    print(f"lengths {lens}, predicted spots in the padding with the switch off: {dropped}")
    scores = [k for k in want if not k.endswith("loss")]
    assert scores and all(on[k] == want[k] == on_dense[k] for k in scores), (on, want)
    if dropped == [0]:
        assert all(on[k] == off[k] for k in scores)
    assert all(k in on and on[k] == on[k] for k in off)      # every loss is reported, none is NaN
