"""Cost of the deterministic mode, interleaved A/B on one box: the LayoutLMv3-base and the LiLT-base train iteration at
8 x 512 tokens (forward + backward + FusedAdamW.step() with clip, every dropout site on).

  arm (a)  mode 0 of this tree against an older tree (default ./_old: `git worktree add _old <commit>` and build it there, as for
           tools/ab_old_new.sh): one fresh process per measurement, ROUNDS rounds old / new / old / new ...: the default path must
           not have moved beyond the two arms' spreads.
  arm (b)  mode 2 against mode 0 of this tree, alternating inside ONE process per model (the mode is a run-time switch): ms per
           iteration, order-dependent launches per iteration under mode 0 (= the launches the mode reroutes), cost per such launch,
           peak device memory under each mode.

    python tools/ab_deterministic.py [--old-root _old] [--rounds 5] [--steps 10] [--warmup 3] [--models lmv3,lilt] [--skip-a]

The parent process never touches the GPU; every measurement runs in a child that ends before the next one starts."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from seeded import layoutlmv3_config, lilt_config, peneo_config, seeded_fill_
    from peneo_amd import hip
    from peneo_amd.data import synthetic_rfund_batch
    from peneo_amd.model import PEneoConfig, PEneoModel
    from peneo_amd.model.engine import DropoutSeeds
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    lilt = args.child == "lilt"
    pcfg = peneo_config("lilt-roberta-en-base", lilt_config("base")) if lilt else peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    torch.manual_seed(20251003)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 11)
    m = m.cuda().set_compute_dtype(torch.bfloat16).train()
    b = synthetic_rfund_batch(8, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=1008, ragged=lilt)
    if lilt:
        b.pop("image", None)
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    opt = FusedAdamW(peneo_param_groups(m, 1e-5, 0.01, 30.0), max_grad_norm=1.0)
    has_mode = hasattr(hip, "set_deterministic")
    counter = hip.order_dependent_launches if has_mode else (lambda: 0)

    def step():
        opt.zero_grad(set_to_none=True)
        m(**batch)["loss"].backward()
        opt.step()
    out = []
    for mode in [int(x) for x in args.modes.split(",")]:
        if has_mode:
            hip.set_deterministic(mode)
        elif mode:
            raise SystemExit("this tree has no deterministic mode")
        DropoutSeeds._step = m._step = 100
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        c0 = counter()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.steps):
            step()
        t1.record()
        torch.cuda.synchronize()
        out.append(dict(mode=mode, ms=t0.elapsed_time(t1) / args.steps, counted=(counter() - c0) / args.steps,
                        peak_mb=torch.cuda.max_memory_allocated() / 2 ** 20))
    print("RESULT " + json.dumps(out))


def run_child(model, root, modes, args):
    env = {k: v for k, v in os.environ.items() if k != "PENEO_DETERMINISTIC"}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", model, "--root", root, "--modes", modes, "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(line[-1][len("RESULT "):])


def spread(xs):
    return f"median {statistics.median(xs):.3f}  min {min(xs):.3f}  max {max(xs):.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--modes", default="0")
    ap.add_argument("--old-root", default=os.path.join(ROOT, "_old"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="lmv3,lilt")
    ap.add_argument("--skip-a", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for model in args.models.split(","):
        print(f"== {model}-base, 8 x 512 tokens, train iteration with FusedAdamW + clip: ms per iteration over {args.steps} iterations")
        if not args.skip_a:
            old, new = [], []
            for r in range(args.rounds):
                old.append(run_child(model, args.old_root, "0", args)[0]["ms"])
                new.append(run_child(model, ROOT, "0", args)[0]["ms"])
                print(f"   (a) round {r}: old {old[-1]:.3f}  new mode 0 {new[-1]:.3f}", flush=True)
            print(f"(a) old tree      : {spread(old)}")
            print(f"(a) this tree, 0  : {spread(new)}")
        res = run_child(model, ROOT, ",".join(["0", "2"] * args.rounds), args)
        m0 = [x for x in res if x["mode"] == 0]
        m2 = [x for x in res if x["mode"] == 2]
        for r, (a, b) in enumerate(zip(m0, m2)):
            print(f"   (b) round {r}: mode 0 {a['ms']:.3f}  mode 2 {b['ms']:.3f}")
        t0, t2 = statistics.median(x["ms"] for x in m0), statistics.median(x["ms"] for x in m2)
        n = m0[0]["counted"]
        print(f"(b) mode 0        : {spread([x['ms'] for x in m0])}   order-dependent launches per iteration {n:.0f}   peak {m0[-1]['peak_mb']:.0f} MiB")
        print(f"(b) mode 2        : {spread([x['ms'] for x in m2])}   order-dependent launches per iteration {m2[0]['counted']:.0f}   peak {m2[-1]['peak_mb']:.0f} MiB")
        print(f"(b) cost          : {t2 - t0:+.3f} ms per iteration ({100 * (t2 - t0) / t0:+.1f} %), {1000 * (t2 - t0) / max(n, 1):+.1f} us per rerouted launch, "
              f"{m2[-1]['peak_mb'] - m0[-1]['peak_mb']:+.0f} MiB peak device memory", flush=True)


if __name__ == "__main__":
    main()
