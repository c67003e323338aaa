"""Length-aware pair heads (set_skip_padded_pairs / peneo_pair_heads_fwd_lens) against the default on one box, interleaved A/B
(profiles/pair_lens.txt), at 8 x 511 tokens, bf16, D = 384 (the hand-interleaved kernel) and D = 768 (the four-wave kernel), for three
length sets - all full, the lengths of synthetic_rfund_batch(ragged=True), all at half length - each with its pair fraction
sum_b P_b / (B P) beside the times:
(a) the pair-head launch alone, as an eval forward calls it (logits and loss): peneo_pair_heads_fwd against peneo_pair_lens_from_mask +
    peneo_pair_heads_fwd_lens (fill launch included);
(b) the eval forward per 8 documents (LayoutLMv3-base; the decoder shrink on: D = 384, and off: D = 768), switch off against on;
(c) with --parent DIR (a checkout of the parent commit, built): the off arm of (a) and (b) at full lengths in fresh processes of this
    tree and of DIR, alternating - the default path did not move.
Every child process runs under its own time limit and a failed one ends the run (no retries).
    python tools/run_pair_lens.py [--parent DIR]"""
import argparse, json, math, os, subprocess, sys
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--root", default=HERE, help="(child) the tree whose package runs")
ap.add_argument("--child", action="store_true", help="(child) the off arm at full lengths in a fresh process -> one JSON line")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import ops  # noqa: E402
from seeded import layoutlmv3_config, peneo_config, seeded_fill_  # noqa: E402
from peneo_amd.model import PEneoConfig, PEneoModel  # noqa: E402
from peneo_amd.data import synthetic_rfund_batch  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", 5))
CLASSES = [2, 3, 3, 3, 3]
B, N = 8, 511
P = N * (N + 1) // 2
WIDTHS = (384, 768)
HAS_LENS = hasattr(ops, "pair_heads_fwd_lens")             # (the parent's package has only the plain launch)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def ab(label, frac, fa, fb, reps):
    """interleaved rounds of off (fa) and on (fb); -> (median off, median on)"""
    for f in (fa, fb):
        timed(f, 3)
    rows = [(timed(fa, reps), timed(fb, reps)) for _ in range(ROUNDS)]
    for a, b in rows:
        print(f"{label}: off {a:.3f} ms  on {b:.3f} ms")
    a, b = [r[0] for r in rows], [r[1] for r in rows]
    gap, sa, sb = med(a) - med(b), max(a) - min(a), max(b) - min(b)
    verdict = "established" if abs(gap) > max(sa, sb) else "not established"
    print(f"{label} median: off {med(a):.3f} ms (spread {sa:.3f})  on {med(b):.3f} ms (spread {sb:.3f})  gap {gap:+.3f} ms: {verdict}; "
          f"on / off {med(b) / med(a):.3f} at pair fraction {frac:.3f} (short of it by {med(b) / med(a) - frac:+.3f} of the off arm)")
    sys.stdout.flush()
    return med(a), med(b)


def length_sets():
    """name -> decoder lengths [B] (of the N = 511 cropped positions)"""
    mask = synthetic_rfund_batch(B, N + 1, 128, 50265, seed=0, ragged=True)["attention_mask"][:, 1:]
    return {"full": [N] * B, "ragged": [int(r.sum()) for r in mask], "half": [N // 2] * B}


def fraction(lens):
    return sum(n * (n + 1) // 2 for n in lens) / (B * P)


def kernel_closures(D):
    """-> (off, on(mask)) launches at width D, as an eval forward with labels calls them"""
    g = torch.Generator().manual_seed(D)
    abt = torch.randn(B, N, 2 * D, generator=g).cuda().to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).cuda() for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).cuda() for c in CLASSES]
    b1, b2 = (0.1 * torch.randn(5 * D, generator=g)).cuda(), torch.zeros(14, device="cuda")
    tags = [torch.randint(0, c, (B, P), generator=g).cuda() for c in CLASSES]
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device="cuda") for c in CLASSES]
    wp = ops.pair_heads_pack(torch.bfloat16, w1, w2)
    off = lambda: ops.pair_heads_fwd(abt, wp, b1, b2, CLASSES, tags=tags, class_weights=cw)

    def on(mask):
        return lambda: ops.pair_heads_fwd_lens(abt, ops.pair_lens_from_mask(mask, N), wp, b1, b2, CLASSES, tags=tags, class_weights=cw)
    return off, on


def mask_of(lens):
    return (torch.arange(N)[None, :] < torch.tensor(lens)[:, None]).long().cuda()


def eval_model(D):
    """LayoutLMv3-base in eval mode, bf16; D = 384: the decoder shrink on, D = 768: off.  -> (model, batch(lens))"""
    pcfg = dict(peneo_config("layoutlmv3-base", layoutlmv3_config("base")), peneo_decoder_shrink=(D == 384))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 13)
    m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
    m.backbone.check_inputs = False
    assert m.peneo_decoder.decoder_hidden_size == D
    base = {k: v.cuda() for k, v in synthetic_rfund_batch(B, N + 1, 128, pcfg["backbone_config"]["vocab_size"], seed=0).items()}

    def batch(lens):
        full = torch.ones(B, N + 1, dtype=torch.int64, device="cuda")
        full[:, 1:] = mask_of(lens)
        return dict(base, attention_mask=full)
    return m, batch


def forward_of(m, batch, on):
    def go():
        if HAS_LENS:
            m.set_skip_padded_pairs(on)
        with torch.no_grad():
            return m(**batch)["loss"]
    return go


def child():
    """the off arm at full lengths: the plain launch and the eval forward, both widths"""
    res = {"root": ROOT}
    for D in WIDTHS:
        off, _ = kernel_closures(D)
        timed(off, 3)
        res[f"kernel_{D}_ms"] = med([timed(off, 10) for _ in range(3)])
        del off
        torch.cuda.empty_cache()
        m, batch = eval_model(D)
        go = forward_of(m, batch([N] * B), False)
        timed(go, 3)
        res[f"forward_{D}_ms"] = med([timed(go, 10) for _ in range(3)])
        del m, batch, go
        torch.cuda.empty_cache()
    print(json.dumps(res))


def run_child(root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--child"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child {root} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, B={B} N={N} (P = {P}: {-(-P // 256)} workgroups a document) bf16")
    print(clocks())
    sets = length_sets()
    for name, lens in sets.items():
        print(f"lengths {name}: {lens}  pair fraction {fraction(lens):.3f}")
    table = []
    for D in WIDTHS:
        off, on = kernel_closures(D)
        for name, lens in sets.items():
            a, b = ab(f"(a) pair-head launch alone, D = {D}, {name}", fraction(lens), off, on(mask_of(lens)), 10)
            table.append((f"launch D={D}", name, fraction(lens), a, b))
        del off, on
        torch.cuda.empty_cache()
    for D in WIDTHS:
        m, batch = eval_model(D)
        for name, lens in sets.items():
            bt = batch(lens)
            a, b = ab(f"(b) eval forward of 8 documents, D = {D}, {name}", fraction(lens), forward_of(m, bt, False), forward_of(m, bt, True), 5)
            table.append((f"forward D={D}", name, fraction(lens), a, b))
        m.set_skip_padded_pairs(False)
        del m, batch
        torch.cuda.empty_cache()
    print("summary (medians, ms):   what, lengths, pair fraction, off, on, on / off")
    for what, name, frac, a, b in table:
        print(f"  {what:<16} {name:<7} {frac:.3f}  {a:8.3f}  {b:8.3f}  {b / a:.3f}")
    if ARGS.parent:
        rows = []
        for _ in range(ROUNDS):
            rows.append((run_child(os.path.abspath(ARGS.parent)), run_child(HERE)))
            print("(c) off arm, full lengths, fresh processes: " + "  ".join(
                f"{k[:-3]} parent {rows[-1][0][k]:.3f} this tree {rows[-1][1][k]:.3f} ms" for k in sorted(rows[-1][0]) if k.endswith("_ms")))
            sys.stdout.flush()
        for k in sorted(rows[0][0]):
            if k.endswith("_ms"):
                a, b = [r[0][k] for r in rows], [r[1][k] for r in rows]
                gap, sa, sb = med(b) - med(a), max(a) - min(a), max(b) - min(b)
                verdict = "established" if abs(gap) > max(sa, sb) else "not established"
                print(f"(c) {k} median: parent {med(a):.3f} (spread {sa:.3f})  this tree {med(b):.3f} (spread {sb:.3f})  gap {gap:+.3f} ms: {verdict}")
    print(clocks())


if __name__ == "__main__":
    if ARGS.child:
        child()
    else:
        main()
