"""The decode front end (score maps on the device -> spot lists on the host) on one box, interleaved A/B:

  parent   one ``get_spots_from_shaking_tag`` per document and head: B x 5 single-workgroup launches, three host reads each;
  batched  ``get_spots_from_shaking_tags_batch``: two launches and two device-to-host copies for the whole batch.

Workload: the five score maps of one eval forward of a seeded LayoutLMv3-base PEneo model (bf16 compute) on 8 synthetic documents
of 512 tokens (N = 511, P = 130 816).  A randomly initialised model calls about two thirds of all pairs a spot, which no decode
ever sees, so the class-0 bias of every head is raised until about 0.5 % of the pairs stay spots (a trained model's density, and
the one the kernel tests use); the density reached is printed.  Each timing is a host clock around work that starts from
synchronised device tensors and ends in the host-side spot lists - the synchronisations are part of what is measured - REPS calls
per timing, ROUNDS interleaved rounds after a warm-up, every round printed, then medians and spreads (max - min).  The two new
kernels' device time comes from events around the bare launches.  Last, the peak device memory of ``prediction_loop`` over 8, 16, 32
and 64 synthetic documents in both modes (``torch.cuda.max_memory_allocated`` above what is allocated before the loop).
Results: profiles/decode_front_end.txt."""
import os, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import ops
from seeded import layoutlmv3_config, peneo_config
from peneo_amd.model import HandshakingTaggingScheme as H, PEneoConfig, PEneoModel
from peneo_amd.data import synthetic_rfund_batch
from peneo_amd.pipeline import prediction_loop

ROUNDS = int(os.environ.get("ROUNDS", 5))
REPS = int(os.environ.get("REPS", 5))
B, S = 8, 512
N = S - 1
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
DENSITY = 0.005


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(REPS):
        fn()
    return (time.perf_counter() - t) * 1e3 / REPS


def med_spread(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def build_model(batch):
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    torch.manual_seed(0)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})).cuda().set_compute_dtype(torch.bfloat16).eval()
    m.backbone.check_inputs = False
    with torch.no_grad():
        out = m(**batch)
        for h in HEADS:                                   # class-0 bias up to the margin that leaves DENSITY of the pairs as spots
            lg = getattr(out, h + "_shaking_outputs").float()
            margin = (lg[..., 1:].max(-1).values - lg[..., 0]).flatten()
            thr = margin.topk(int(DENSITY * margin.numel())).values[-1]
            getattr(m.peneo_decoder, h + "_fc")[3].bias[0] += thr
    return m


def front_end(m, batch):
    with torch.no_grad():
        out = m(**batch)
    maps = [getattr(out, h + "_shaking_outputs") for h in HEADS]
    P = maps[0].shape[1]
    parent = lambda: [[H.get_spots_from_shaking_tag(mp[b], seq_len=N) for b in range(B)] for mp in maps]
    batched = lambda: H.get_spots_from_shaking_tags_batch(maps, N)
    a, b = parent(), batched()
    n = [sum(len(d) for d in per_map) for per_map in b]
    print(f"maps: {[tuple(mp.shape) for mp in maps]}  spots per map over {B} documents: {n}  "
          f"(density {sum(n) / (5 * B * P):.4%})  lists identical: {a == b}")
    for f in (parent, batched):
        host_ms(f)
    rows = []
    for _ in range(ROUNDS):
        rows.append((host_ms(parent), host_ms(batched)))
        print(f"front end, {B} documents x 5 maps -> host spot lists: parent {rows[-1][0]:.3f} ms  batched {rows[-1][1]:.3f} ms")
    (pa, sa), (pb, sb) = med_spread([r[0] for r in rows]), med_spread([r[1] for r in rows])
    print(f"front end median: parent {pa:.3f} ms (spread {sa:.3f})  batched {pb:.3f} ms (spread {sb:.3f})  ({pa / pb:.1f}x)")
    print(f"bar (batched median below parent median by more than both spreads): {pa - pb:.3f} ms > {sa + sb:.3f} ms: {pa - pb > sa + sb}")
    # the two kernels alone
    fmaps = [mp.float().contiguous() for mp in maps]
    rec = torch.empty((5, B, 4096, 4), dtype=torch.int32, device="cuda")
    cnt = torch.empty((5, B), dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.spots_batch_workspace_bytes(5, B, N), dtype=torch.uint8, device="cuda")
    launch = lambda: ops.spots_compact_batch_launch(fmaps, N, 4096, records=rec, counts=cnt, workspace=ws)
    launch()
    ts = []
    for _ in range(ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            launch()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / 20)
    md, sp = med_spread(ts)
    byt = 2 * sum(mp.numel() * 4 for mp in fmaps)
    print(f"count + write kernels, device events, 20 launches per timing: {' '.join(f'{t:.1f}' for t in ts)} us; "
          f"median {md:.1f} us (spread {sp:.1f}), {byt / 1e6:.0f} MB read -> {byt / md / 1e6:.2f} TB/s")
    old = lambda: ops.lib().peneo_spots_compact(ops.ptr(fmaps[1][0]), P, 3, N, ops.ptr(rec), ops.ptr(rec[1]), ops.ptr(cnt), 4096, ops.stream())
    old()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        old()
    e.record()
    torch.cuda.synchronize()
    print(f"per-map kernel, one [P, 3] map, device events: {s.elapsed_time(e) * 1e3 / 20:.1f} us (x {5 * B} maps per batch)")


def loop_memory(m, batch):
    host = {k: v.cpu() for k, v in batch.items()}
    host.update(text=[["x"] * N for _ in range(B)], relations=[[] for _ in range(B)], fname=[f"doc{i}" for i in range(B)])
    nothing = lambda p, epoch=0: {}
    sizes = (8, 16, 32, 64)
    for compact in (False, True):
        peaks = []
        for docs in sizes:
            torch.cuda.synchronize(); torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            prediction_loop(m, [host] * (docs // B), nothing, compact_spots=compact)
            peaks.append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        print(f"prediction_loop compact_spots={compact}: peak device memory above the model at {sizes} documents: "
              + " ".join(f"{p:.0f}" for p in peaks) + f" MiB (growth 8 -> 64: {peaks[-1] - peaks[0]:+.0f} MiB)")


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, {REPS} calls per timing")
    print(clocks())
    batch = {k: v.cuda() for k, v in synthetic_rfund_batch(B, S, 128, 50265, seed=0).items()}
    m = build_model(batch)
    front_end(m, batch)
    sys.stdout.flush()
    loop_memory(m, batch)
    print(clocks())


if __name__ == "__main__":
    main()
