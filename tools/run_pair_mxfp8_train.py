"""MXFP8 train forward of the pair heads against the bf16 saving forward on one box, interleaved A/B (profiles/pair_mxfp8_train.txt):
(a) the launch alone at B = 8, N = 511, D = 384, drop_p = 0.1 with loss and dlogits, as a train step calls it: peneo_pair_heads_fwd_save
    against peneo_pair_heads_fwd_mxfp8_save; the weight packs of the two formats on their own (a train step repacks after every
    optimizer step);
(b) the LayoutLMv3-base train step (8 documents x 512 tokens, bf16, dropout on, FusedAdamW step included, so every step repacks the
    weights of its format) with set_pair_heads_train_format("bf16") and ("mxfp8")."""
import math, os, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import ops
from seeded import layoutlmv3_config, peneo_config, seeded_fill_
from peneo_amd.model import PEneoConfig, PEneoModel
from peneo_amd.data import synthetic_rfund_batch
from peneo_amd.optim import FusedAdamW, peneo_param_groups

ROUNDS = int(os.environ.get("ROUNDS", 5))
CLASSES = [2, 3, 3, 3, 3]
B, N, D, DROP = 8, 511, 384, 0.1


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def ab(label, unit, fa, fb, reps):
    for f in (fa, fb):
        timed(f, 3)
    rows = [(timed(fa, reps), timed(fb, reps)) for _ in range(ROUNDS)]
    for a, b in rows:
        print(f"{label}: bf16 {a:.3f} {unit}  mxfp8 {b:.3f} {unit}")
    a, b = sorted(r[0] for r in rows), sorted(r[1] for r in rows)
    lower = all(y < x for x, y in rows)
    print(f"{label} median: bf16 {a[len(a) // 2]:.3f} {unit} (spread {a[-1] - a[0]:.3f})  mxfp8 {b[len(b) // 2]:.3f} {unit} "
          f"(spread {b[-1] - b[0]:.3f})  ratio {a[len(a) // 2] / b[len(b) // 2]:.3f}x  mxfp8 lower in every round: {lower}")
    sys.stdout.flush()


def launch_alone():
    g = torch.Generator().manual_seed(0)
    P = N * (N + 1) // 2
    abt = torch.randn(B, N, 2 * D, generator=g).cuda().to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).cuda() for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).cuda() for c in CLASSES]
    b1, b2 = (0.1 * torch.randn(5 * D, generator=g)).cuda(), torch.zeros(14, device="cuda")
    tags = [torch.randint(0, c, (B, P), generator=g).cuda() for c in CLASSES]
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device="cuda") for c in CLASSES]
    wp16, wpmx = ops.pair_heads_pack(torch.bfloat16, w1, w2), ops.pair_heads_pack_mxfp8(w1, w2)
    bufs = (torch.empty(ops.pair_save_bytes(B, N, 5, D), dtype=torch.uint8, device="cuda"),
            torch.empty(B * ops.pair_bwd_rows(N), D, dtype=torch.bfloat16, device="cuda"))
    kw = dict(want_logits=False, tags=tags, class_weights=cw, want_dlogits=True, drop_p=DROP, drop_seed=5, save_buffers=bufs)
    f16 = lambda: ops.pair_heads_fwd(abt, wp16, b1, b2, CLASSES, save=True, **kw)
    fmx = lambda: ops.pair_heads_fwd_mxfp8_save(abt, wpmx, b1, b2, CLASSES, **kw)
    ab(f"(a) saving forward alone, B={B} N={N} D={D} drop_p={DROP}", "ms", f16, fmx, 10)
    ab("(a) weight pack alone (once per optimizer step)", "ms", lambda: ops.pair_heads_pack(torch.bfloat16, w1, w2),
       lambda: ops.pair_heads_pack_mxfp8(w1, w2), 20)


def train_step():
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 13)
    m = m.cuda().set_compute_dtype(torch.bfloat16).train()
    m.backbone.check_inputs = False
    batch = {k: v.cuda() for k, v in synthetic_rfund_batch(B, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=0, ragged=True).items()}
    opt = FusedAdamW(peneo_param_groups(m, 1e-7, 0.01, 30.0), max_grad_norm=1.0)

    def step(fmt):
        def go():
            m.set_pair_heads_train_format(fmt)
            for p_ in m.parameters():
                p_.grad = None
            out = m(**batch)
            out["loss"].backward()
            opt.step()
            return out["loss"]
        return go
    l16, lmx = float(step("bf16")().detach()), float(step("mxfp8")().detach())
    print(f"(b) LayoutLMv3-base train step, {B} documents x 512 tokens, bf16, dropout on, optimizer step included: "
          f"loss bf16 {l16:.5f}  mxfp8 {lmx:.5f}")
    ab("(b) train step (forward + loss + backward + optimizer)", "ms", step("bf16"), step("mxfp8"), 10)
    m.set_pair_heads_train_format("bf16")


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds")
    print(clocks())
    launch_alone()
    train_step()
    print(clocks())


if __name__ == "__main__":
    main()
