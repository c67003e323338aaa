"""LiLT's attention on one box, interleaved A/B:

  parent   the concat path: two ``head_concat`` launches build the packed q | k | v copy (text 64 + layout 16 per head),
           ``attn_fwd`` runs at head dim 80 (the register-staged kernel at DP = 96), ``head_split`` writes the two context streams;
  attn2    ``attn2_fwd``: one launch of the pipelined two-stream kernel, no copies.

(a) One layer's attention at B = 8, nh = 12, T = 512 on seeded bf16 operands with a ragged key bias, device events around REPS
    back-to-back calls of each arm (outputs preallocated where the op allows it; the parent's ``cat`` / ``attc`` buffers are
    allocated once, outside the timing).  The two arms' outputs are compared bit for bit first.
(b) The eval forward of a seeded LiLT-base PEneo model (12 layers, bf16 compute, ``torch.no_grad()``) on 8 synthetic documents of
    512 tokens with PENEO_LILT_ATTN2=0 (the parent commit's path) and =1, device events around REPS forwards, for the backbone
    alone and for the whole model; the five score maps of both settings are compared bit for bit first.
ROUNDS interleaved rounds after a warm-up, every round printed, then medians and spreads (max - min).
Results: profiles/lilt_attention2.txt."""
import math, os, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import ops
from seeded import lilt_config, peneo_config, seeded_fill_
from peneo_amd.model import PEneoConfig, PEneoModel
from peneo_amd.data import synthetic_rfund_batch

ROUNDS = int(os.environ.get("ROUNDS", 5))
REPS = int(os.environ.get("REPS", 20))
B, S, NH, DA, DB = 8, 512, 12, 64, 16
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def event_us(fn, reps=REPS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def med_spread(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def ab(name, unit, scale, parent, new):
    for f in (parent, new):
        event_us(f, 3)
    rows = []
    for _ in range(ROUNDS):
        rows.append((event_us(parent) * scale, event_us(new) * scale))
        print(f"{name}: parent {rows[-1][0]:.3f} {unit}  attn2 {rows[-1][1]:.3f} {unit}")
    (pa, sa), (pb, sb) = med_spread([r[0] for r in rows]), med_spread([r[1] for r in rows])
    print(f"{name} median: parent {pa:.3f} {unit} (spread {sa:.3f})  attn2 {pb:.3f} {unit} (spread {sb:.3f})  ({pa / pb:.2f}x)  "
          f"attn2 below parent in every round: {all(r[1] < r[0] for r in rows)}")
    sys.stdout.flush()


def one_layer():
    H, Hl, dc, R = NH * DA, NH * DB, DA + DB, B * S
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(R, 3 * H, generator=g).to(torch.bfloat16).cuda()
    lqkv = torch.randn(R, 3 * Hl, generator=g).to(torch.bfloat16).cuda()
    kb = torch.zeros(B, ops.attn_padded_len(S), dtype=torch.float32)
    for b in range(B):
        kb[b, S - 37 * b:S] = -1.0e30                   # ragged documents
    kb = kb.cuda()
    sa, sb = 1.0 / math.sqrt(DA), 1.0 / math.sqrt(DB)
    cat = torch.empty((R, 3 * NH * dc), dtype=torch.bfloat16, device="cuda")
    attc = torch.empty((R, NH * dc), dtype=torch.bfloat16, device="cuda")
    att, latt = torch.empty((R, H), dtype=torch.bfloat16, device="cuda"), torch.empty((R, Hl), dtype=torch.bfloat16, device="cuda")
    att2, latt2 = torch.empty_like(att), torch.empty_like(latt)
    lse, lse2 = (torch.empty((B, NH, S), dtype=torch.float32, device="cuda") for _ in range(2))

    def parent():
        ops.head_concat(qkv[:, :H], lqkv[:, :Hl], NH, cat[:, :NH * dc], sa, sb)
        ops.head_concat(qkv[:, H:], lqkv[:, Hl:], 2 * NH, cat[:, NH * dc:])
        ops.attn_fwd(cat[:, :NH * dc], cat[:, NH * dc:2 * NH * dc], cat[:, 2 * NH * dc:], B, NH, S, dc, 1.0, None, kb, out=attc, lse=lse)
        ops.head_split(attc, NH, att, latt)

    def core():
        ops.attn_fwd(cat[:, :NH * dc], cat[:, NH * dc:2 * NH * dc], cat[:, 2 * NH * dc:], B, NH, S, dc, 1.0, None, kb, out=attc, lse=lse)

    def new():
        ops.attn2_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], lqkv[:, :Hl], lqkv[:, Hl:2 * Hl], lqkv[:, 2 * Hl:], B, NH, S, sa, sb, kb,
                      out_a=att2, out_b=latt2, lse=lse2)

    parent(); new()
    torch.cuda.synchronize()
    print(f"(a) one layer's attention, B = {B}, nh = {NH}, T = {S}, head dims {DA} + {DB}: outputs identical: "
          f"{torch.equal(att, att2) and torch.equal(latt, latt2) and torch.equal(lse, lse2)}")
    ab("(a) attention of one layer", "us", 1.0, parent, new)
    event_us(core, 3)
    ts = [event_us(core) for _ in range(ROUNDS)]
    md, sp = med_spread(ts)
    print(f"(a) the parent's attn_fwd launch alone (head dim 80, no copies): {' '.join(f'{t:.1f}' for t in ts)} us; median {md:.1f} us (spread {sp:.1f})")


def eval_forward():
    pcfg = peneo_config("lilt-roberta-en-base", lilt_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 13)
    m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
    m.backbone.check_inputs = False
    batch = synthetic_rfund_batch(B, S, 128, pcfg["backbone_config"]["vocab_size"], seed=0, ragged=True, with_image=False)
    batch = {k: v.cuda() for k, v in batch.items()}
    enc = {k: batch[k] for k in ("input_ids", "bbox", "attention_mask")}

    def run(switch, fn):
        def go():
            os.environ["PENEO_LILT_ATTN2"] = switch
            with torch.no_grad():
                return fn()
        return go

    whole_off, whole_on = run("0", lambda: m(**batch)), run("1", lambda: m(**batch))
    bb_off, bb_on = run("0", lambda: m.backbone(**enc)), run("1", lambda: m.backbone(**enc))
    a, b = whole_off(), whole_on()
    same = all(torch.equal(a[h + "_shaking_outputs"], b[h + "_shaking_outputs"]) for h in HEADS)
    print(f"(b) LiLT-base eval forward, {B} documents x {S} tokens, bf16: score maps identical with the switch off and on: {same}")
    ab("(b) backbone eval forward", "ms", 1e-3, bb_off, bb_on)
    ab("(b) whole-model eval forward", "ms", 1e-3, whole_off, whole_on)
    os.environ.pop("PENEO_LILT_ATTN2", None)


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, {REPS} calls per timing")
    print(clocks())
    one_layer()
    eval_forward()
    print(clocks())


if __name__ == "__main__":
    main()
