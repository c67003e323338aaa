"""Whole training iterations with FusedAdamW, emission of the working copies off (every copy re-cast by the next forward)
against on (written by the optimizer kernel): bench.py's synthetic batch, bf16, train mode, LayoutLMv3-base and LiLT-base at
8 x 512 tokens with 128 lines.  The two arms alternate on one box, one process: per round and arm 3 warm-up iterations, then
`--iters` timed ones; reported per round: the median ms of an iteration (zero_grad + forward + loss + backward + step(), HIP
events at the iteration boundaries, so the host runs ahead as in training) and the median ms of step() alone (HIP events
around it), then each arm's spread over the rounds.  One model, one optimizer per arm (each with its own moments).

    python tools/run_adamw_emit.py [--rounds 5] [--iters 20] [--out profiles/adamw_emit.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from bench import build_model  # noqa: E402  (also puts tests/golden on the path)


def run_backbone(backbone, rounds, iters, warmup, say):
    from peneo_amd.data import synthetic_rfund_batch
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model, pcfg = build_model("base", torch.bfloat16, backbone)
    model = model.to(dev).set_compute_dtype(torch.bfloat16).train()
    model.backbone.check_inputs = "deferred"
    vocab = pcfg["backbone_config"]["vocab_size"]
    batches = []
    for s in range(4):
        b = synthetic_rfund_batch(8, 512, 128, vocab, seed=s)
        if backbone == "lilt":
            b.pop("image", None)
        batches.append({k: v.to(dev) for k, v in b.items()})
    arms = {"off": FusedAdamW(peneo_param_groups(model, 5e-5, 0.01, 30.0), max_grad_norm=1.0),
            "on": FusedAdamW(peneo_param_groups(model, 5e-5, 0.01, 30.0), max_grad_norm=1.0, emit_into=model)}

    def iterate(opt, n):
        """n iterations -> (ms per iteration, ms per step()): events only, no host sync inside"""
        marks, steps = [], []
        for i in range(n):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)
            opt.zero_grad(set_to_none=True)
            model(**batches[i % len(batches)])["loss"].backward()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opt.step()
            z.record()
            steps.append((a, z))
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)
        torch.cuda.synchronize()
        return [marks[i].elapsed_time(marks[i + 1]) for i in range(n)], [a.elapsed_time(z) for a, z in steps]

    med = {k: {"iter": [], "step": []} for k in arms}
    for r in range(rounds):
        for name, opt in arms.items():
            iterate(opt, warmup)
            it, st = iterate(opt, iters)
            med[name]["iter"].append(statistics.median(it))
            med[name]["step"].append(statistics.median(st))
            say(f"{backbone} round {r} emit {name:3s}: iteration median {med[name]['iter'][-1]:.3f} ms (min {min(it):.3f} max {max(it):.3f}), "
                f"step() median {med[name]['step'][-1]:.3f} ms (min {min(st):.3f} max {max(st):.3f})")
    n_emit = len(arms["on"].emitted_keys())
    say(f"{backbone}: {n_emit} cache entries written by the step, {arms['on']._emit.n_records} records")
    for what in ("iter", "step"):
        off, on = med["off"][what], med["on"][what]
        gap = statistics.median(off) - statistics.median(on)
        spread = max(max(off) - min(off), max(on) - min(on))
        verdict = "established" if abs(gap) > spread else "not established"
        say(f"{backbone} {what:4s}: off median-of-rounds {statistics.median(off):.3f} ms (spread {max(off) - min(off):.3f}), "
            f"on {statistics.median(on):.3f} ms (spread {max(on) - min(on):.3f}); off - on = {gap:+.3f} ms: {verdict} "
            f"(the gap {'exceeds' if abs(gap) > spread else 'does not exceed'} both arms' spreads)")
    del arms, model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--backbones", default="layoutlmv3,lilt")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.cuda.set_stream(torch.cuda.Stream(device=torch.device("cuda", 0), priority=-1))     # as bench.py runs the step
    p = torch.cuda.get_device_properties(0)
    say(f"box: {p.name}, {p.multi_processor_count} CUs, torch {torch.__version__}, hip {torch.version.hip}, "
        f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
    say(f"arms interleaved per round; rounds {args.rounds}, warm-up {args.warmup}, timed iterations {args.iters}; 8 x 512 tokens, 128 lines, bf16, train mode")
    for bb in args.backbones.split(","):
        run_backbone(bb, args.rounds, args.iters, args.warmup, say)


if __name__ == "__main__":
    main()
