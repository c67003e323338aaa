"""The fused pair-heads forward at decoder width 768 (peneo_decoder_shrink = False on a base backbone; pair_heads_wide.hip) against
the materialising per-document path (PEneoDecoder.pair_wide = False, i.e. PENEO_PAIR_WIDE=0) on one box, interleaved A/B
(profiles/pair_wide.txt).  The decoder stage alone, bf16, 8 documents x 511 tokens (P = 130 816 pairs each):
(a) the eval forward (no gradients; the five logit maps and the loss),
(b) a train step of the stage (train mode, the classifier dropout on: forward + loss + backward; the fused arm's backward is the
    chunked one, the materialising arm's the per-document one)."""
import os, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from seeded import layoutlmv3_config, peneo_config, seeded_fill_
from peneo_amd.model import PEneoConfig
from peneo_amd.model.peneo_decoder import PEneoDecoder, TAG_KWARGS

ROUNDS = int(os.environ.get("ROUNDS", 5))
B, N, D = 8, 511, 768


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def ab(label, fa, fb, reps):
    for f in (fa, fb):
        timed(f, 2)
    rows = [(timed(fa, reps), timed(fb, reps)) for _ in range(ROUNDS)]
    for a, b in rows:
        print(f"{label}: fused {a:.3f} ms  materialising {b:.3f} ms")
    a, b = sorted(r[0] for r in rows), sorted(r[1] for r in rows)
    lower = all(x < y for x, y in rows)
    print(f"{label} median: fused {a[len(a) // 2]:.3f} ms (spread {a[-1] - a[0]:.3f})  materialising {b[len(b) // 2]:.3f} ms "
          f"(spread {b[-1] - b[0]:.3f})  ratio {b[len(b) // 2] / a[len(a) // 2]:.3f}x  fused lower in every round: {lower}")
    sys.stdout.flush()
    return lower


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, B={B} N={N} D={D} bf16")
    print(clocks())
    pcfg = dict(peneo_config("layoutlmv3-base", layoutlmv3_config("base")), peneo_decoder_shrink=False)
    dec = PEneoDecoder(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}), D)
    seeded_fill_({"peneo_decoder." + k: v for k, v in dec.state_dict().items()}, 13)
    dec = dec.cuda()
    assert dec.decoder_hidden_size == D
    g = torch.Generator().manual_seed(0)
    seq = torch.randn(B, N, D, generator=g).cuda().to(torch.bfloat16)
    P = N * (N + 1) // 2
    tags = {k: (torch.rand(B, P, generator=g) < 0.01).long().cuda() * (1 + (i % 2) * (i > 0)) for i, k in enumerate(TAG_KWARGS)}

    def forward(wide):
        def go():
            dec.pair_wide = wide
            with torch.no_grad():
                return dec(seq, **tags)["loss"]
        return go

    def step(wide):
        def go():
            dec.pair_wide = wide
            for p_ in dec.parameters():
                p_.grad = None
            out = dec(seq, **tags)
            out["loss"].backward()
            return out["loss"]
        return go
    dec.eval()
    print(f"(a) eval loss: fused {float(forward(True)()):.5f}  materialising {float(forward(False)()):.5f}")
    fwd_lower = ab("(a) eval forward of the decoder stage", forward(True), forward(False), 3)
    dec.train()
    print(f"(b) train loss (each arm draws its own dropout masks): fused {float(step(True)().detach()):.5f}  "
          f"materialising {float(step(False)().detach()):.5f}")
    step_lower = ab("(b) train step of the decoder stage (forward + loss + backward)", step(True), step(False), 3)
    dec.pair_wide = True
    print(f"fused below the materialising arm in every round: eval forward {fwd_lower}, train step {step_lower}")
    print(clocks())


if __name__ == "__main__":
    main()
