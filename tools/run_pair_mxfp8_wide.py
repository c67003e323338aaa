"""Wide MXFP8 against bf16 pair heads with the decoder shrink off, on one box, interleaved A/B, 8 x 511 tokens, bf16:
(i)   the pair-head launch alone at D = 768 and D = 1024: peneo_pair_heads_fwd_mxfp8_wide against peneo_pair_heads_fwd (the four-wave
      bf16 kernel of pair_heads_wide.hip);
(ii)  the eval forward of 8 documents of a shrink-off LayoutLMv3-base model, set_pair_heads_format("mxfp8", wide=True) against the
      default;
(iii) with --parent-tree DIR (a built checkout of the parent commit): the default arm of (ii) against that checkout's, one fresh
      process per arm and round, interleaved.
A gain is established only where the gap between the medians exceeds both arms' spreads (max - min over the rounds).
Results: profiles/pair_mxfp8_wide.txt."""
import argparse, math, os, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUNDS = int(os.environ.get("ROUNDS", 5))
CLASSES = [2, 3, 3, 3, 3]


def imports(root):
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests", "golden"))


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def verdict(name, rows, a_name, b_name):
    for a, b in rows:
        print(f"{name}: {a_name} {a:.3f} ms  {b_name} {b:.3f} ms")
    med = lambda v: sorted(v)[len(v) // 2]
    A, B = [r[0] for r in rows], [r[1] for r in rows]
    gap, sa, sb = med(A) - med(B), max(A) - min(A), max(B) - min(B)
    word = "established" if abs(gap) > max(sa, sb) else "not established"
    print(f"{name} median: {a_name} {med(A):.3f} ms (spread {sa:.3f})  {b_name} {med(B):.3f} ms (spread {sb:.3f})  "
          f"gap {gap:+.3f} ms, {med(A) / med(B):.2f}x: {word}")
    sys.stdout.flush()


def kernel_ab(B, N, D):
    from peneo_amd import ops
    g = torch.Generator().manual_seed(0)
    ab = torch.randn(B, N, 2 * D, generator=g).cuda().to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).cuda() for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).cuda() for c in CLASSES]
    b1, b2 = torch.zeros(5 * D, device="cuda"), torch.zeros(14, device="cuda")
    wp16, wpmx = ops.pair_heads_pack(torch.bfloat16, w1, w2), ops.pair_heads_pack_mxfp8_wide(w1, w2)
    f16 = lambda: ops.pair_heads_fwd(ab, wp16, b1, b2, CLASSES)
    fmx = lambda: ops.pair_heads_fwd_mxfp8_wide(ab, wpmx, b1, b2, CLASSES)
    for f in (f16, fmx):
        timed(f, 3)
    return [(timed(f16, 10), timed(fmx, 10)) for _ in range(ROUNDS)]


def eval_model():
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    from peneo_amd.data import synthetic_rfund_batch
    pcfg = dict(peneo_config("layoutlmv3-base", layoutlmv3_config("base")), peneo_decoder_shrink=False)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})).cuda().set_compute_dtype(torch.bfloat16).eval()
    m.backbone.check_inputs = False
    bs = [{k: v.cuda() for k, v in synthetic_rfund_batch(8, 512, 128, 50265, seed=s).items()} for s in range(3)]

    def run():
        for b in bs:
            m(**b)
    return m, run


def eval_ab():
    m, run = eval_model()
    rows = []
    with torch.no_grad():
        for wide in (False, True):
            m.set_pair_heads_format("mxfp8" if wide else "bf16", wide=wide)
            timed(run, 2)
        for _ in range(ROUNDS):
            m.set_pair_heads_format("bf16")
            a = timed(run, 3) / 3
            m.set_pair_heads_format("mxfp8", wide=True)
            rows.append((a, timed(run, 3) / 3))
    return rows


def eval_default_once():
    """one arm, one round of (iii): the default eval forward per 8 documents of whichever checkout is first on sys.path"""
    _, run = eval_model()
    with torch.no_grad():
        timed(run, 2)
        print(f"DEFAULT_MS {timed(run, 5) / 3:.4f}")


def parent_ab(parent):
    def one(root):
        env = dict(os.environ, PENEO_TREE=root)
        env.pop("PENEO_HIP_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--default-once"], env=env, capture_output=True, text=True,
                             timeout=600, check=True).stdout
        return float([l for l in out.splitlines() if l.startswith("DEFAULT_MS")][0].split()[1])
    return [(one(parent), one(ROOT)) for _ in range(ROUNDS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--default-once", action="store_true")
    args = ap.parse_args()
    imports(os.environ.get("PENEO_TREE", ROOT))
    if args.default_once:
        return eval_default_once()
    print(f"device: {torch.cuda.get_device_name(0)}")
    for D in (768, 1024):
        verdict(f"(i) pair-head launch B=8 N=511 D={D}", kernel_ab(8, 511, D), "bf16 wide", "mxfp8 wide")
    verdict("(ii) eval forward per 8 documents, shrink-off LayoutLMv3-base", eval_ab(), "default", "mxfp8 wide")
    if args.parent_tree:
        verdict("(iii) default eval forward per 8 documents", parent_ab(os.path.abspath(args.parent_tree)), "parent", "this tree")


if __name__ == "__main__":
    main()
