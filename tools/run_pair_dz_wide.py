"""The four-wave peneo_pair_dz_fused (pair_dz_wide.hip) in the chunked decoder backward at width 768 (peneo_decoder_shrink = False on a
base backbone) against the parent chain (peneo_pair_x_fwd -> z GEMM -> peneo_pair_dz), on one box, interleaved
(profiles/pair_dz_wide.txt).  The decoder stage alone, bf16, 8 documents x 511 tokens (130 816 pairs each), train mode:
(a) the stage's train step (forward + loss + backward) with PEneoDecoder.fused_dz_wide off / on / on with the kernel writing x and
    a_i + b_j itself (dz_wide_writes_x: no peneo_pair_x_fwd launch), peak device memory of each arm,
(b) the worst gradient cosine and norm ratio between the arms on the same dropout masks,
(c) one document's dz alone: the new launch against the z GEMM + peneo_pair_dz (train) and the GEMM's pair_dz epilogue (eval)."""
import os, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from seeded import layoutlmv3_config, peneo_config, seeded_fill_
from peneo_amd import ops
from peneo_amd.model import PEneoConfig
from peneo_amd.model.engine import DropoutSeeds
from peneo_amd.model.peneo_decoder import HEAD_CLASSES, PEneoDecoder, TAG_KWARGS

ROUNDS = int(os.environ.get("ROUNDS", 5))
REPS = int(os.environ.get("REPS", 3))
B, N, D = 8, 511, 768
ARMS = (("parent", False, False), ("wide dz", True, False), ("wide dz + x", True, True))


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def compare(label, fns, reps):
    """fns: [(name, callable)], the first is the parent; interleaved rounds; prints the verdict per arm against the parent"""
    for _, f in fns:
        timed(f, 2)
    rows = [[timed(f, reps) for _, f in fns] for _ in range(ROUNDS)]
    for r in rows:
        print(f"{label}: " + "  ".join(f"{n} {t:.3f} ms" for (n, _), t in zip(fns, r)))
    cols = [sorted(r[i] for r in rows) for i in range(len(fns))]
    for i, (n, _) in enumerate(fns):
        c = cols[i]
        line = f"{label} [{n}]: median {c[len(c) // 2]:.3f} ms  min {c[0]:.3f}  max {c[-1]:.3f}"
        if i:
            lower = all(r[i] < r[0] for r in rows)
            gap = cols[0][len(cols[0]) // 2] - c[len(c) // 2]
            clear = lower and gap > max(c[-1] - c[0], cols[0][-1] - cols[0][0])
            line += (f"  parent / this {cols[0][len(cols[0]) // 2] / c[len(c) // 2]:.3f}x  lower in every round: {lower}  gap {gap:.3f} ms "
                     f"above both spreads: {clear}  -> {'established' if clear else 'not established'}")
        print(line)
    sys.stdout.flush()


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, {REPS} calls per timing, B={B} N={N} D={D} bf16, train mode")
    print(clocks())
    pcfg = dict(peneo_config("layoutlmv3-base", layoutlmv3_config("base")), peneo_decoder_shrink=False)
    dec = PEneoDecoder(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}), D)
    seeded_fill_({"peneo_decoder." + k: v for k, v in dec.state_dict().items()}, 13)
    dec = dec.cuda()
    assert dec.decoder_hidden_size == D and ops.pair_dz_fused_supported(torch.bfloat16, D, len(HEAD_CLASSES))
    g = torch.Generator().manual_seed(0)
    seq = torch.randn(B, N, D, generator=g).cuda().to(torch.bfloat16)
    P = N * (N + 1) // 2
    tags = {k: (torch.rand(B, P, generator=g) < 0.01).long().cuda() * (1 + (i % 2) * (i > 0)) for i, k in enumerate(TAG_KWARGS)}

    def step(wide, writes_x, seed_step=None):
        def go():
            dec.fused_dz_wide, dec.dz_wide_writes_x = wide, writes_x
            if seed_step is not None:
                DropoutSeeds._step = seed_step
            for p_ in dec.parameters():
                p_.grad = None
            out = dec(seq, **tags)
            out["loss"].backward()
            return out["loss"]
        return go
    dec.train()

    # (b) first: the same masks in every arm
    grads = {}
    for name, wide, wx in ARMS:
        loss = step(wide, wx, seed_step=7000)()
        torch.cuda.synchronize()
        grads[name] = {n: p.grad.detach().clone() for n, p in dec.named_parameters() if p.grad is not None}
        print(f"(b) train loss [{name}]: {float(loss.detach()):.6f}")
    ref = grads["parent"]
    gmax = max(float(v.double().norm()) for v in ref.values())
    for name in ("wide dz", "wide dz + x"):
        cos, nr = 1.0, 0.0
        for n, r in ref.items():
            a, r = grads[name][n].double().flatten(), r.double().flatten()
            if float(r.norm()) <= 1e-6 * gmax:
                continue
            cos = min(cos, float(torch.dot(a, r) / (a.norm() * r.norm())))
            nr = max(nr, abs(float(a.norm() / r.norm()) - 1))
        print(f"(b) gradients [{name}] against [parent], {len(ref)} tensors: worst cosine {cos:.7f}  worst |norm ratio - 1| {nr:.3e}")
    del grads, ref

    # (a) the train step, interleaved, and the peak memory of each arm
    compare("(a) train step of the decoder stage", [(n, step(w, x)) for n, w, x in ARMS], REPS)
    for name, wide, wx in ARMS:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step(wide, wx)()
        torch.cuda.synchronize()
        print(f"(a) peak device memory of a step [{name}]: {torch.cuda.max_memory_allocated() / 2**20:.1f} MiB")
    dec.fused_dz_wide, dec.dz_wide_writes_x = False, False

    # (c) one document's dz alone (what the chunk loop runs per document: 130 816 pairs are one chunk)
    dt, nh = torch.bfloat16, len(HEAD_CLASSES)
    names = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
    sd = dict(dec.named_parameters())
    w1 = [sd[f"{n}_fc.0.weight"].detach() for n in names]
    w2 = [sd[f"{n}_fc.3.weight"].detach().float().contiguous() for n in names]
    b1cat = torch.cat([sd[f"{n}_fc.0.bias"].detach() for n in names]).float().contiguous()
    w1cat = torch.cat(w1).to(dt)
    wp = ops.pair_heads_pack(dt, w1, w2)
    ab = torch.randn(N, 2 * D, generator=g).cuda().to(dt)
    dl = [(0.01 * torch.randn(P, c, generator=g)).cuda() for c in HEAD_CLASSES]
    scale = torch.ones(nh, device="cuda")
    x, pre = torch.empty(P, D, dtype=dt, device="cuda"), torch.empty(P, D, dtype=dt, device="cuda")
    z = torch.empty(P, nh * D, dtype=dt, device="cuda")
    ws = ops.pair_dz_workspace(nh, D, "cuda")
    for label, drop in (("train, drop_p 0.1", dict(drop_p=0.1, drop_seed=5, drop_doc=0, drop_pair0=0)), ("eval", {})):
        dza = ops.pair_dz_args(D, HEAD_CLASSES, dl, w2, scale, **drop)

        def parent():
            ops.pair_x_fwd(ab, 0, N, x, pre)
            if drop:
                ops.gemm(x, w1cat, bias=b1cat, out=z)
                ops.pair_dz(z, P, D, HEAD_CLASSES, None, None, ws, None, args=dza)
            else:
                ops.gemm(x, w1cat, bias=b1cat, out=z, pair_dz=dza, pair_dz_ws=ws)

        def wide():
            ops.pair_x_fwd(ab, 0, N, x, pre)
            ops.pair_dz_fused(ab, 0, N, wp, b1cat, dza, z, ws)

        def wide_x():
            ops.pair_dz_fused(ab, 0, N, wp, b1cat, dza, z, ws, x, pre)

        def x_only():
            ops.pair_x_fwd(ab, 0, N, x, pre)
        compare(f"(c) x / pre and dz of one document ({label})",
                [("pair_x_fwd + z GEMM + pair_dz" if drop else "pair_x_fwd + z GEMM with the pair_dz epilogue", parent),
                 ("pair_x_fwd + wide dz", wide), ("wide dz writing x / pre", wide_x)], REPS)
        print(f"(c) pair_x_fwd alone: {timed(x_only, 5):.3f} ms;  first layer of one document: {2 * P * nh * D * D / 1e9:.0f} GFLOP")
    print(clocks())


if __name__ == "__main__":
    main()
