"""MXFP8 against bf16 encoder layers on one box, interleaved A/B within one process per step (ROUNDS rounds, medians, warm-up first):
  gemm      per forward shape of the base (R = 5672) and the large (R = 2442) layer, peneo_gemm bf16 against peneo_gemm_mxfp8 with the same
            epilogue (operands already quantized), and the row quantizer of the activation that feeds it;
  layer     one encoder layer forward, peneo_encoder_layer_fwd against peneo_encoder_layer_fwd_mxfp8 (quantizers included);
  eval      the eval forward of a base LayoutLMv3 PEneo model per 8 documents (8 x 512 tokens, 128 lines) in the four combinations
            encoder bf16 / mxfp8 x pair heads bf16 / mxfp8;
  accuracy  the figures of the model-level tests (tests/test_gpu_encoder_mxfp8.py: the same functions).
Without arguments the steps run one after the other, each in a process of its own under its own time limit; nothing is started after a
step that failed.  Clocks are read (read-only query) before and after every step.  Results: profiles/encoder_mxfp8.txt."""
import math, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"gemm": 240, "layer": 180, "eval": 420, "accuracy": 600}   # per-step time limit, seconds


def driver():
    for step, limit in STEPS.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step]).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__" and len(sys.argv) < 2:
    sys.exit(driver())

import torch
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, os.path.join(ROOT, "tests"))
from peneo_amd import hip, ops
from peneo_amd.hip import ACT_GELU, ACT_NONE

ROUNDS = int(os.environ.get("ROUNDS", 5))
DEV = "cuda"
median = lambda xs: sorted(xs)[len(xs) // 2]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def ab(label, fns, reps, unit=1e3, suffix="us", nd=1):
    """fns: {name: callable}; interleaved rounds, every round printed, then the medians and the spread of each arm"""
    for f in fns.values():
        timed(f, 3)
    rows = [{n: timed(f, reps) * unit for n, f in fns.items()} for _ in range(ROUNDS)]
    for r in rows:
        print(f"{label}: " + "  ".join(f"{n} {v:.{nd}f} {suffix}" for n, v in r.items()))
    med = {n: median([r[n] for r in rows]) for n in fns}
    spread = {n: max(r[n] for r in rows) - min(r[n] for r in rows) for n in fns}
    print(f"{label} median: " + "  ".join(f"{n} {med[n]:.{nd}f} {suffix} (spread {spread[n]:.{nd}f})" for n in fns), flush=True)
    return med


def step_gemm():
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, R, H, I in (("base", 5672, 768, 3072), ("large", 2442, 1024, 4096)):
        roles = (("qkv", 3 * H, H, {}), ("attn-out", H, H, {"residual": True}), ("ffn1", I, H, {"act": ACT_GELU}), ("ffn2", H, I, {"residual": True}))
        for role, N, K, opt in roles:
            a = torch.randn((R, K), device=DEV, generator=g).to(torch.bfloat16)
            w = (torch.randn((N, K), device=DEV, generator=g) * 0.03)
            w16 = w.to(torch.bfloat16)
            bias = torch.randn(N, device=DEV, generator=g) * 0.1
            res = torch.randn((R, N), device=DEV, generator=g).to(torch.bfloat16) if opt.get("residual") else None
            aq, as_ = ops.mxfp8_quantize_rows_bf16(a)
            wq, ws = ops.mxfp8_quantize_rows(w)
            out = torch.empty((R, N), dtype=torch.bfloat16, device=DEV)
            kw = dict(bias=bias, act=opt.get("act", ACT_NONE), residual=res, out=out)
            med = ab(f"gemm {name} {role} M={R} N={N} K={K}", {
                "bf16": lambda: ops.gemm(a, w16, **kw),
                "mxfp8": lambda: ops.gemm_mxfp8(aq, as_, wq, ws, **kw),
                "quantize-A": lambda: ops.mxfp8_quantize_rows_bf16(a, aq, as_)}, 20)
            fl = 2.0 * R * N * K
            print(f"gemm {name} {role}: bf16 {fl / med['bf16'] / 1e6:.0f} TFLOP/s  mxfp8 {fl / med['mxfp8'] / 1e6:.0f} TFLOP/s  "
                  f"speed-up {med['bf16'] / med['mxfp8']:.2f}x, with the quantizer {med['bf16'] / (med['mxfp8'] + med['quantize-A']):.2f}x", flush=True)


def step_layer():
    from test_gpu_encoder_mxfp8 import LayerCase
    import ctypes as C
    for name, B, T, H, nh, I in (("base", 8, 709, 768, 12, 3072), ("large", 2, 1221, 1024, 16, 4096)):
        case = LayerCase(ops, B, T, H, nh, I, key_bias=True)
        R = B * T
        # the bf16 composite on the dequantized weights
        deq = lambda q, s: (q.view(torch.float8_e4m3fn).float().reshape(q.shape[0], -1, 32) * torch.exp2(s.float() - 127.0).unsqueeze(-1)
                            ).reshape(q.shape).to(torch.bfloat16)
        w16 = [deq(q, s) for q, s in case.w]
        bf = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=DEV)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
        keep = dict(qkv=bf(R, 3 * H), att=bf(R, H), h1=bf(R, H), a=bf(R, H), h2=bf(R, H), inter=bf(R, I), lse=f32(B, nh, T), m1=f32(R),
                    r1=f32(R), m2=f32(R), r2=f32(R), out=bf(R, H))
        L = hip.EncoderLayer()
        L.Wqkv, L.Wo, L.Wi, L.Wo2 = (t.data_ptr() for t in w16)
        L.bqkv, L.bo, L.bi, L.bo2 = (t.data_ptr() for t in case.b)
        L.g1, L.b1, L.g2, L.b2 = (t.data_ptr() for t in case.ln)
        L.key_bias, L.x = case.kb.data_ptr(), case.x.data_ptr()
        for n in ("qkv", "att", "h1", "a", "h2", "inter", "lse", "m1", "r1", "m2", "r2"):
            setattr(L, n, keep[n].data_ptr())
        L.B, L.T, L.H, L.nh, L.I = B, T, H, nh, I
        L.eps, L.attn_scale = case.eps, case.scale
        wsb = int(hip.lib().peneo_encoder_layer_workspace_bytes(R, H, I, 0))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)

        def f16():
            hip.check(hip.lib().peneo_encoder_layer_fwd(C.byref(L), keep["out"].data_ptr(), ws.data_ptr(), wsb, hip.stream()), "layer")
        Lm, Xm, got = case.describe()
        fmx = lambda: ops.encoder_layer_fwd_mxfp8(Lm, Xm, got["out"])
        fmx()
        f16()
        cos = float(torch.nn.functional.cosine_similarity(got["out"].flatten().double(), keep["out"].flatten().double(), dim=0))
        med = ab(f"layer {name} B={B} T={T} H={H} I={I}", {"bf16": f16, "mxfp8": fmx}, 10)
        print(f"layer {name}: speed-up {med['bf16'] / med['mxfp8']:.2f}x; cosine of out, mxfp8 against bf16 on the dequantized weights {cos:.5f}", flush=True)


def step_eval():
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    from peneo_amd.data import synthetic_rfund_batch
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})).cuda().set_compute_dtype(torch.bfloat16).eval()
    m.backbone.check_inputs = False
    bs = [{k: v.cuda() for k, v in synthetic_rfund_batch(8, 512, 128, 50265, seed=s).items()} for s in range(3)]

    def run(enc, heads):
        def f():
            m.set_encoder_format(enc).set_pair_heads_format(heads)
            for b in bs:
                m(**b)
        return f
    import time
    with torch.no_grad():
        fns = {f"enc-{e}+heads-{h}": run(e, h) for h in ("bf16", "mxfp8") for e in ("bf16", "mxfp8")}
        ab("eval forward per 8 documents", {n: (lambda f=f: f()) for n, f in fns.items()}, 3, unit=1.0 / 3, suffix="ms", nd=3)
        # the host's share: time to ENQUEUE a forward (no synchronise inside the window; the queue is empty at its start)
        for n, f in fns.items():
            ts = []
            for _ in range(ROUNDS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts.append((time.perf_counter() - t0) / 3 * 1e3)
                torch.cuda.synchronize()
            print(f"host enqueue time per forward, {n}: median {median(ts):.3f} ms (min {min(ts):.3f})", flush=True)


def step_accuracy():
    from test_gpu_encoder_mxfp8 import COSINE_FLOOR, TRAIN_LR, TRAIN_STEPS, random_init_accuracy, trained_spot_agreement
    res = random_init_accuracy()
    print(f"random init, 12 layers, base width, B = 2, S = 512, encoder mxfp8 against bf16: cosine of last_hidden_state "
          f"{res['cosine_last_hidden_state']:.5f} (floor {COSINE_FLOOR}), relative error {res['relative_error_last_hidden_state']:.4f}; "
          "logit maps: " + " ".join(f"{k} {v:.5f}" for k, v in res["cosine_logit_maps"].items()), flush=True)
    res = trained_spot_agreement()
    print(f"trained batch (2 layers, B = 2, S = 512, {TRAIN_STEPS} steps, lr {TRAIN_LR:g}): loss after {res.pop('loss_after'):.5f}")
    for k, v in res.items():
        print(f"  {k}: bf16 spots {v.pop('spots_bf16')}")
        for setting, r in v.items():
            print(f"    {setting}: " + ", ".join(f"{n} {x:.5g}" if isinstance(x, float) else f"{n} {x}" for n, x in r.items()))


if __name__ == "__main__":
    step = sys.argv[1]
    print(f"==== {step}: device {torch.cuda.get_device_name(0)}, {ROUNDS} rounds")
    print(clocks(), flush=True)
    {"gemm": step_gemm, "layer": step_layer, "eval": step_eval, "accuracy": step_accuracy}[step]()
    print(clocks(), flush=True)
