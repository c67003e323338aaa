"""MXFP8 against bf16 pair heads on one box, interleaved A/B: the eval kernel alone at (B, N, D) = (8, 511, 384) and (2, 1023, 512),
the whole bf16 eval forward of a base LayoutLMv3 model per 8 documents in both pair-head formats, and the accuracy figures of the
model-level tests (tests/test_gpu_pair_mxfp8.py: the same functions): random-init cosines per logit map for LayoutLMv3 and LiLT, and
the trained-batch spot agreement.  Results: profiles/pair_mxfp8.txt."""
import math, os, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from peneo_amd import ops
from seeded import layoutlmv3_config, peneo_config
from peneo_amd.model import PEneoConfig, PEneoModel
from peneo_amd.data import synthetic_rfund_batch

ROUNDS = int(os.environ.get("ROUNDS", 5))
CLASSES = [2, 3, 3, 3, 3]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernel_ab(B, N, D):
    g = torch.Generator().manual_seed(0)
    ab = torch.randn(B, N, 2 * D, generator=g).cuda().to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).cuda() for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).cuda() for c in CLASSES]
    b1, b2 = torch.zeros(5 * D, device="cuda"), torch.zeros(14, device="cuda")
    wp16, wpmx = ops.pair_heads_pack(torch.bfloat16, w1, w2), ops.pair_heads_pack_mxfp8(w1, w2)
    f16 = lambda: ops.pair_heads_fwd(ab, wp16, b1, b2, CLASSES)
    fmx = lambda: ops.pair_heads_fwd_mxfp8(ab, wpmx, b1, b2, CLASSES)
    for f in (f16, fmx):
        timed(f, 3)
    rows = []
    for _ in range(ROUNDS):
        rows.append((timed(f16, 10), timed(fmx, 10)))
    return rows


def eval_ab():
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})).cuda().set_compute_dtype(torch.bfloat16).eval()
    m.backbone.check_inputs = False
    bs = [{k: v.cuda() for k, v in synthetic_rfund_batch(8, 512, 128, 50265, seed=s).items()} for s in range(3)]
    def run(fmt):
        m.set_pair_heads_format(fmt)
        def f():
            for b in bs:
                m(**b)
        return f
    rows = []
    with torch.no_grad():
        for fmt in ("bf16", "mxfp8"):
            timed(run(fmt), 2)
        for _ in range(ROUNDS):
            rows.append((timed(run("bf16"), 3) / 3, timed(run("mxfp8"), 3) / 3))
    return rows


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(clocks())
    for B, N, D in ((8, 511, 384), (2, 1023, 512)):
        rows = kernel_ab(B, N, D)
        for a, b in rows:
            print(f"kernel B={B} N={N} D={D}: bf16 {a:.3f} ms  mxfp8 {b:.3f} ms")
        a = sorted(r[0] for r in rows)[len(rows) // 2]; b = sorted(r[1] for r in rows)[len(rows) // 2]
        print(f"kernel B={B} N={N} D={D} median: bf16 {a:.3f} ms  mxfp8 {b:.3f} ms  ({a / b:.2f}x)")
        sys.stdout.flush()
    rows = eval_ab()
    for a, b in rows:
        print(f"eval forward per 8 documents: bf16 {a:.3f} ms  mxfp8 {b:.3f} ms")
    a = sorted(r[0] for r in rows)[len(rows) // 2]; b = sorted(r[1] for r in rows)[len(rows) // 2]
    print(f"eval forward per 8 documents median: bf16 {a:.3f} ms  mxfp8 {b:.3f} ms  ({a / b:.2f}x)")
    print(clocks())
    sys.stdout.flush()
    from test_gpu_pair_mxfp8 import TRAIN_LR, TRAIN_STEPS, random_init_cosines, trained_spot_agreement
    for bb in ("lmv3", "lilt"):
        cos = random_init_cosines(bb)
        print(f"random init, {bb}, 2 layers, B = 2, S = 512: cosine mxfp8 / bf16 per map: "
              + " ".join(f"{k} {v:.5f}" for k, v in cos.items()))
    res = trained_spot_agreement()
    print(f"trained batch (lmv3, 2 layers, B = 2, S = 512, {TRAIN_STEPS} steps, lr {TRAIN_LR:g}): loss after {res.pop('loss_after'):.5f}")
    for k, v in res.items():
        print(f"  {k}: " + ", ".join(f"{n} {x:.5g}" if isinstance(x, float) else f"{n} {x}" for n, x in v.items()))


if __name__ == "__main__":
    main()
