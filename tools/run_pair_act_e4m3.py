"""e4m3 against f16 records of the saved pair activations on one box, interleaved A/B (profiles/pair_act_e4m3.txt), at 8 x 511 tokens,
D = 384, drop_p = 0.1:
(a) peneo_pair_heads_fwd_save against peneo_pair_heads_fwd_save_e4m3 alone (loss and dlogits on, as a train step calls it);
(b) peneo_pair_bwd_saved against peneo_pair_bwd_saved_e4m3 alone;
(c) the LayoutLMv3-base train iteration (8 documents x 512 tokens, bf16, dropout on, FusedAdamW step included) with
    set_pair_act_format("f16") and ("e4m3"), and the lowest gradient cosine of the e4m3 step against the f16 step;
(d) peak device memory of that iteration, one fresh process per format (the step-sized buffers are kept between steps, so one
    process that ran both formats holds the larger one);
(e) with --parent DIR (a checkout of the parent commit, built): the f16 arm of (a) - (c) in fresh processes of this tree and of DIR,
    alternating - the default path did not move.
    python tools/run_pair_act_e4m3.py [--parent DIR]"""
import argparse, gc, json, math, os, subprocess, sys
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--root", default=HERE, help="(child) the tree whose package runs")
ap.add_argument("--child", default=None, choices=["f16", "e4m3"], help="(child) one format in a fresh process -> one JSON line")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import ops  # noqa: E402
from seeded import layoutlmv3_config, peneo_config, seeded_fill_  # noqa: E402
from peneo_amd.model import PEneoConfig, PEneoModel  # noqa: E402
from peneo_amd.data import synthetic_rfund_batch  # noqa: E402
from peneo_amd.optim import FusedAdamW, peneo_param_groups  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", 5))
CLASSES = [2, 3, 3, 3, 3]
B, N, D, DROP = 8, 511, 384, 0.1
HAS_E4M3 = hasattr(ops, "pair_save_e4m3_bytes")           # (the parent's package has only the f16 form)


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


def ab(label, fa, fb, reps):
    for f in (fa, fb):
        timed(f, 3)
    rows = [(timed(fa, reps), timed(fb, reps)) for _ in range(ROUNDS)]
    for a, b in rows:
        print(f"{label}: f16 {a:.3f} ms  e4m3 {b:.3f} ms")
    a, b = [r[0] for r in rows], [r[1] for r in rows]
    gap, sa, sb = med(a) - med(b), max(a) - min(a), max(b) - min(b)
    verdict = "established" if abs(gap) > max(sa, sb) else "not established"
    print(f"{label} median: f16 {med(a):.3f} ms (spread {sa:.3f})  e4m3 {med(b):.3f} ms (spread {sb:.3f})  gap {gap:+.3f} ms: {verdict}")
    sys.stdout.flush()


def kernel_closures(fmt):
    """-> (forward, backward) launches of one format on buffers of their own"""
    g = torch.Generator().manual_seed(0)
    P = N * (N + 1) // 2
    abt = torch.randn(B, N, 2 * D, generator=g).cuda().to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).cuda() for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).cuda() for c in CLASSES]
    b1, b2 = (0.1 * torch.randn(5 * D, generator=g)).cuda(), torch.zeros(14, device="cuda")
    tags = [torch.randint(0, c, (B, P), generator=g).cuda() for c in CLASSES]
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device="cuda") for c in CLASSES]
    wp, wp2 = ops.pair_heads_pack(torch.bfloat16, w1, w2), ops.pair_bwd_pack(w1)
    nbytes = ops.pair_save_e4m3_bytes(B, N, 5, D) if fmt == "e4m3" else ops.pair_save_bytes(B, N, 5, D)
    bufs = (torch.empty(nbytes, dtype=torch.uint8, device="cuda"),
            torch.empty(B * ops.pair_bwd_rows(N), D, dtype=torch.bfloat16, device="cuda"))
    kw = dict(want_logits=False, tags=tags, class_weights=cw, want_dlogits=True, drop_p=DROP, drop_seed=5, save=True, save_buffers=bufs)
    fkw, bkw = (dict(save_format=fmt), dict(act_format=fmt)) if HAS_E4M3 else ({}, {})
    fwd = lambda: ops.pair_heads_fwd(abt, wp, b1, b2, CLASSES, **kw, **fkw)
    dl = fwd()[2]
    dz = torch.empty(B * ops.pair_bwd_rows(N), 5 * D, dtype=torch.bfloat16, device="cuda")
    d_ab = torch.empty(B, N, 2 * D, device="cuda")
    ws = ops.pair_bwd_workspace(B, N, 5, D, "cuda")
    args = ops.pair_dz_args(D, CLASSES, dl, w2, torch.ones(5, device="cuda"), drop_p=DROP, drop_seed=5)
    keep = (dl, w2)   # noqa: F841  (args holds raw pointers)
    bwd = lambda: (keep, ops.pair_bwd_saved(abt, wp2, args, bufs[0], dz, d_ab, ws, **bkw))
    return fwd, bwd


def model_step():
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 13)
    m = m.cuda().set_compute_dtype(torch.bfloat16).train()
    m.backbone.check_inputs = False
    batch = {k: v.cuda() for k, v in synthetic_rfund_batch(B, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=0, ragged=True).items()}
    opt = FusedAdamW(peneo_param_groups(m, 1e-7, 0.01, 30.0), max_grad_norm=1.0)

    def step(fmt, optimizer=True):
        def go():
            if HAS_E4M3:
                m.set_pair_act_format(fmt)
            for p_ in m.parameters():
                p_.grad = None
            out = m(**batch)
            out["loss"].backward()
            if optimizer:
                opt.step()
            return out["loss"]
        return go
    return m, step


def kernels_alone(fmt):
    """the two launches of one format; its buffers (records, x rows, dz, workspace: ~10 GB) die with this frame"""
    fwd, bwd = kernel_closures(fmt)
    timed(fwd, 3)
    timed(bwd, 3)
    return {"fwd_ms": med([timed(fwd, 10) for _ in range(3)]), "bwd_ms": med([timed(bwd, 10) for _ in range(3)])}


def child(fmt):
    res = {"fmt": fmt, "root": ROOT, **kernels_alone(fmt)}
    gc.collect()
    torch.cuda.empty_cache()
    res["held_before_model_gb"] = torch.cuda.memory_allocated() / 1e9          # (nothing of the kernel measurement is left: ~0)
    m, step = model_step()
    go = step(fmt)
    timed(go, 3)
    torch.cuda.reset_peak_memory_stats()
    res["step_ms"] = med([timed(go, 10) for _ in range(3)])
    res["peak_gb"] = torch.cuda.max_memory_allocated() / 1e9
    print(json.dumps(res))


def run_child(root, fmt):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--child", fmt], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child {root} {fmt} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, B={B} N={N} D={D} drop_p={DROP}")
    print(clocks())
    print(f"records: f16 {ops.pair_save_bytes(B, N, 5, D) / 1e9:.3f} GB  e4m3 {ops.pair_save_e4m3_bytes(B, N, 5, D) / 1e9:.3f} GB")
    (f16, b16), (f8, b8) = kernel_closures("f16"), kernel_closures("e4m3")
    ab("(a) saving forward alone", f16, f8, 10)
    ab("(b) saved backward alone", b16, b8, 10)
    del f16, b16, f8, b8
    torch.cuda.empty_cache()
    m, step = model_step()
    # gradients of one step per format, same seeds (no optimizer step in between)
    from peneo_amd.model.engine import DropoutSeeds
    grads = {}
    for fmt in ("f16", "e4m3"):
        DropoutSeeds._step, m._step = 40, 40
        loss = step(fmt, optimizer=False)()
        torch.cuda.synchronize()
        grads[fmt] = (float(loss.detach()), {n: p.grad.detach().double().flatten().clone() for n, p in m.named_parameters() if p.grad is not None})
    cos = {n: float(torch.dot(a, grads["f16"][1][n]) / (a.norm() * grads["f16"][1][n].norm()))
           for n, a in grads["e4m3"][1].items() if float(grads["f16"][1][n].norm()) > 0}
    # (attention key biases: an analytically zero gradient, rounding noise in both formats - listed apart)
    low = sorted(((n, c) for n, c in cos.items() if not n.endswith("key.bias")), key=lambda kv: kv[1])[:5]
    keyb = sorted(c for n, c in cos.items() if n.endswith("key.bias"))
    print(f"(c) one step, same seeds: loss f16 {grads['f16'][0]:.6f}  e4m3 {grads['e4m3'][0]:.6f}; lowest gradient cosines e4m3 vs f16: {low}; "
          f"key biases (noise): {keyb[0]:.3f} .. {keyb[-1]:.3f}")
    del grads
    ab("(c) train iteration (forward + loss + backward + optimizer)", step("f16"), step("e4m3"), 10)
    m.set_pair_act_format("f16")
    del m, step
    torch.cuda.empty_cache()
    for fmt in ("f16", "e4m3"):
        r = run_child(HERE, fmt)
        print(f"(d) fresh process, {fmt}: peak device memory of the train iteration {r['peak_gb']:.2f} GB (step {r['step_ms']:.3f} ms; "
              f"{r['held_before_model_gb']:.3f} GB allocated before the model was built)")
    if ARGS.parent:
        rows = []
        for _ in range(ROUNDS):
            rows.append((run_child(os.path.abspath(ARGS.parent), "f16"), run_child(HERE, "f16")))
            print(f"(e) f16 arm, fresh processes: parent fwd {rows[-1][0]['fwd_ms']:.3f} bwd {rows[-1][0]['bwd_ms']:.3f} step {rows[-1][0]['step_ms']:.3f} ms"
                  f"  this tree fwd {rows[-1][1]['fwd_ms']:.3f} bwd {rows[-1][1]['bwd_ms']:.3f} step {rows[-1][1]['step_ms']:.3f} ms")
            sys.stdout.flush()
        for k in ("fwd_ms", "bwd_ms", "step_ms"):
            a, b = [r[0][k] for r in rows], [r[1][k] for r in rows]
            print(f"(e) {k} median: parent {med(a):.3f} (spread {max(a) - min(a):.3f})  this tree {med(b):.3f} (spread {max(b) - min(b):.3f})")
    print(clocks())


if __name__ == "__main__":
    if ARGS.child:
        child(ARGS.child)
    else:
        main()
