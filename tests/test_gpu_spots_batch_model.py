"""``prediction_loop(..., compact_spots=True)`` on the two-page RFUND fixture of test_rfund_plumbing.py: the same metrics as the
default mode (the reference's), from spot lists instead of tensors, with dense and with sparse labels."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "golden", "rfund")
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")


@pytest.fixture(scope="module")
def setup():
    from transformers import PreTrainedTokenizerFast
    from peneo_amd.data import DataCollatorForPEneo, RFUNDDataset
    from peneo_amd.model import PEneoConfig, PEneoModel
    from peneo_amd.model.backbone_mapping import BACKBONE_MAPPING
    fx = torch.load(os.path.join(HERE, "golden", "rfund_plumbing.pt"), weights_only=False)
    tok = PreTrainedTokenizerFast(tokenizer_file=os.path.join(ROOT, "tokenizer", "tokenizer.json"), bos_token="<s>",
                                  eos_token="</s>", cls_token="<s>", sep_token="</s>", pad_token="<pad>", unk_token="<unk>",
                                  mask_token="<mask>")
    info = BACKBONE_MAPPING["layoutlmv3-base"]
    ds = RFUNDDataset(data_root=ROOT, split="dev", language="en", tokenizer=tok, tokenizer_fetcher=info.tokenizer_fetcher,
                      max_token_len=info.max_token_len, add_cls_token=info.add_cls_token, add_sep_token=info.add_sep_token)
    collators = {sparse: DataCollatorForPEneo(tokenizer=tok, image_processor=info.image_processor(), max_length=info.max_token_len,
                                              require_image=True, add_cls_token=True, add_sep_token=True, sparse_tags=sparse)
                 for sparse in (False, True)}
    model = PEneoModel(PEneoConfig(**{k: v for k, v in fx["config"].items() if k != "model_type"}))
    model.load_state_dict(fx["state_dict"], strict=True)
    model.to(torch.device("cuda:0")).set_compute_dtype(torch.float32).eval()
    return fx, ds, collators, model


def _spot_lists_only(inner, seen):
    """a compute_metrics that checks what it is handed: per head and document a list of (i, j, tag, score), no tensor"""
    def compute_metrics(p, epoch=0):
        predictions, label_ids, _ = p
        for per_head in list(predictions) + list(label_ids[:5]):
            assert isinstance(per_head, list) and len(per_head) == 2
            for spots in per_head:
                assert isinstance(spots, list) and not torch.is_tensor(spots)
                assert all(isinstance(s, tuple) and len(s) == 4 and not any(torch.is_tensor(v) for v in s) for s in spots)
        seen["predictions"] = predictions
        seen["calls"] = seen.get("calls", 0) + 1
        return inner(p, epoch)
    return compute_metrics


@pytest.mark.parametrize("sparse", [False, True], ids=["dense_labels", "sparse_labels"])
def test_compact_loop_gives_the_reference_metrics(setup, sparse):
    from torch.utils.data import DataLoader
    from peneo_amd.pipeline import make_compute_metrics, prediction_loop
    fx, ds, collators, model = setup
    ev = fx["eval"]
    loader = DataLoader(ds, batch_size=2, shuffle=False, collate_fn=collators[sparse])
    seen, detail = {}, {}
    metrics = prediction_loop(model, loader, _spot_lists_only(make_compute_metrics(detail_eval=True, on_detail=detail.update), seen),
                              compact_spots=True)
    assert seen["calls"] == 1
    for k, want in ev["detail_metric"].items():
        assert metrics["eval_" + k] == want, k
    assert detail["kv_pair"] == ev["detail_metric_detail"]["kv_pair"]
    assert [s["detail"] for s in detail["detail"]] == [s["detail"] for s in ev["detail_metric_detail"]["detail"]]
    assert abs(metrics["eval_loss"] - float(ev["losses"]["loss"])) <= 1e-4
    # the spot lists themselves are the reference's (indices exact, scores as the existing end-to-end test asks)
    for h, name in enumerate(HEADS):
        for b in range(2):
            got, want = seen["predictions"][h][b], ev["spots"][name][b]
            assert [tuple(g[:3]) for g in got] == [tuple(w[:3]) for w in want], (name, b)
            assert all(abs(g[3] - w[3]) <= 1e-4 for g, w in zip(got, want))
    # the plain metric, and the default mode beside it
    m1 = prediction_loop(model, loader, make_compute_metrics(), compact_spots=True)
    m0 = prediction_loop(model, loader, make_compute_metrics())
    for k, want in ev["metric"].items():
        assert m1["eval_" + k] == want and m0["eval_" + k] == want, k
    assert set(m1) == set(m0)
