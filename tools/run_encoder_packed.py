"""Packed encoder for inference (set_skip_padded_tokens / peneo_encoder_layer_fwd_packed) against the default on one box,
interleaved A/B (profiles/encoder_packed.txt), at 8 x 512 tokens with an image (T = 709), bf16, LayoutLMv3-base, for three length sets -
all full, the lengths of synthetic_rfund_batch(ragged=True), all at half length - each with its row fraction R / (B T) beside the times:
(a) one encoder layer alone: peneo_encoder_layer_fwd at B T rows against peneo_encoder_layer_fwd_packed at R rows;
(b) the bias build: buckets + bias at [B, nh, T, Tp] against plan + host read + three per-document packs + buckets + bias at Tm;
(c) the whole eval forward per 8 documents, switch off against on, set_skip_padded_pairs(True) in both arms;
(d) what the switch itself costs at full lengths: plan, host read, pack and unpack of the hidden rows, one by one;
(e) with --parent DIR (a checkout of the parent commit, built): the off arm of (c) at full lengths in fresh processes of this tree and
    of DIR, alternating - the default path did not move.
Every child process runs under its own time limit and a failed one ends the run (no retries).
    python tools/run_encoder_packed.py [--parent DIR]"""
import argparse, ctypes as C, json, math, os, subprocess, sys
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--root", default=HERE, help="(child) the tree whose package runs")
ap.add_argument("--child", action="store_true", help="(child) the off arm at full lengths in a fresh process -> one JSON line")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import hip, ops  # noqa: E402
from seeded import layoutlmv3_config, peneo_config, seeded_fill_  # noqa: E402
from peneo_amd.model import PEneoConfig, PEneoModel  # noqa: E402
from peneo_amd.data import synthetic_rfund_batch  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", 5))
B, S, NV = 8, 512, 197
T = S + NV
H, NH, I = 768, 12, 3072
HAS_PACKED = hasattr(ops, "encoder_layer_fwd_packed")       # (the parent's package has only the default path)
BF16 = torch.bfloat16


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


def ab(label, frac, fa, fb, reps):
    """interleaved rounds of off (fa) and on (fb); -> (median off, median on)"""
    for f in (fa, fb):
        timed(f, 3)
    rows = [(timed(fa, reps), timed(fb, reps)) for _ in range(ROUNDS)]
    for a, b in rows:
        print(f"{label}: off {a:.3f} ms  on {b:.3f} ms")
    a, b = [r[0] for r in rows], [r[1] for r in rows]
    gap, sa, sb = med(a) - med(b), max(a) - min(a), max(b) - min(b)
    verdict = "established" if abs(gap) > max(sa, sb) else "not established"
    print(f"{label} median: off {med(a):.3f} ms (spread {sa:.3f})  on {med(b):.3f} ms (spread {sb:.3f})  gap {gap:+.3f} ms: {verdict}; "
          f"on / off {med(b) / med(a):.3f} at row fraction {frac:.3f}")
    sys.stdout.flush()
    return med(a), med(b)


def length_sets():
    """name -> text lengths [B] (of the S positions, the CLS token among them)"""
    mask = synthetic_rfund_batch(B, S, 128, 50265, seed=0, ragged=True)["attention_mask"]
    return {"full": [S] * B, "ragged": [int(r.sum()) for r in mask], "half": [S // 2] * B}


def fraction(lens):
    return sum(n + NV for n in lens) / (B * T)


def text_mask(lens):
    return (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long().cuda()


def key_mask(lens):
    km = torch.ones((B, T), dtype=torch.int32, device="cuda")
    km[:, :S] = text_mask(lens).to(torch.int32)
    return km


def layer_closures():
    """-> fn(lens) -> (off, on): one layer call on random weights, at B T rows and at the packed rows of `lens`"""
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s, std=1.0: torch.randn(s, device="cuda", generator=g) * std
    w = [rn(n, k, std=0.03).to(BF16) for n, k in ((3 * H, H), (H, H), (I, H), (H, I))]
    bs = [rn(n, std=0.1) for n in (3 * H, H, I, H)]
    ln = [1.0 + rn(H, std=0.1), rn(H, std=0.1), 1.0 + rn(H, std=0.1), rn(H, std=0.1)]
    x = rn(B * T, H).to(BF16)

    def describe(R, Tm):
        bf = lambda *s: torch.empty(s, dtype=BF16, device="cuda")
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        keep = dict(qkv=bf(R, 3 * H), att=bf(R, H), h1=bf(R, H), a=bf(R, H), inter=bf(R, I), h2=bf(R, H), lse=f32(B, NH, Tm), m1=f32(R),
                    r1=f32(R), m2=f32(R), r2=f32(R), out=bf(R, H))
        keep["bias"] = (rn(B, NH, Tm, ops.attn_padded_len(Tm))).to(BF16)
        L = hip.EncoderLayer()
        L.Wqkv, L.Wo, L.Wi, L.Wo2 = (t.data_ptr() for t in w)
        L.bqkv, L.bo, L.bi, L.bo2 = (t.data_ptr() for t in bs)
        L.g1, L.b1, L.g2, L.b2 = (t.data_ptr() for t in ln)
        L.bias, L.bias_ld = keep["bias"].data_ptr(), keep["bias"].shape[-1]
        L.x = x.data_ptr()
        for name in ("qkv", "att", "h1", "a", "inter", "h2", "lse", "m1", "r1", "m2", "r2"):
            setattr(L, name, keep[name].data_ptr())
        L.B, L.T, L.H, L.nh, L.I = B, Tm, H, NH, I
        L.eps, L.attn_scale, L.p_hidden, L.p_attn = 1e-5, 1.0 / math.sqrt(H // NH), 0.0, 0.0
        wsb = int(hip.lib().peneo_encoder_layer_workspace_bytes(R, H, I, 0))
        keep["ws"] = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        return L, keep, wsb

    def make(lens):
        L0, k0, wsb0 = describe(B * T, T)
        off = lambda: hip.check(hip.lib().peneo_encoder_layer_fwd(C.byref(L0), k0["out"].data_ptr(), k0["ws"].data_ptr() if wsb0 else None,
                                                                  wsb0, hip.stream()), "peneo_encoder_layer_fwd")
        tot = [n + NV for n in lens]
        R, Tm = sum(tot), max(tot)
        L1, k1, wsb1 = describe(R, Tm)
        ln_d = torch.tensor(tot, dtype=torch.int32, device="cuda")
        cu_d = torch.tensor([sum(tot[:b]) for b in range(B + 1)], dtype=torch.int32, device="cuda")
        on = lambda: ops.encoder_layer_fwd_packed(L1, ln_d, cu_d, R, k1["out"], k1["ws"] if wsb1 else None)
        return off, on, (k0, k1)
    return make


def eval_model():
    """LayoutLMv3-base in eval mode, bf16, the length-aware pair heads on.  -> (model, batch(lens))"""
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 13)
    m = m.cuda().set_compute_dtype(BF16).eval()
    m.backbone.check_inputs = False
    m.set_skip_padded_pairs(True)
    base = {k: v.cuda() for k, v in synthetic_rfund_batch(B, S, 128, pcfg["backbone_config"]["vocab_size"], seed=0).items()}
    assert base["image"] is not None
    return m, lambda lens: dict(base, attention_mask=text_mask(lens))


def forward_of(m, batch, on):
    def go():
        if HAS_PACKED:
            m.set_skip_padded_tokens(on)
        with torch.no_grad():
            return m(**batch)["loss"]
    return go


def bias_closures(m, batch):
    """the K4 part of the forward alone, as the two paths run it, on the model's own tables -> (off, on)"""
    bb, cfg = m.backbone, m.backbone.config
    dev = torch.device("cuda")
    vx, vy = bb.visual_xy(dev, NV)
    lut1, lut2 = bb.lut("1d", cfg.rel_pos_bins, cfg.max_rel_pos, dev), bb.lut("2d", cfg.rel_2d_pos_bins, cfg.max_rel_2d_pos, dev)
    w1, wx, wy = (t.weight.detach() for t in (bb.encoder.rel_pos_bias, bb.encoder.rel_pos_x_bias, bb.encoder.rel_pos_y_bias))
    km, pos, xs, ys = ops.relpos_inputs(batch["attention_mask"], batch["bbox"].contiguous(), vx, vy, B, S, NV, True, True)
    scale = 1.0 / math.sqrt(H // NH)

    def off():
        bk = ops.relpos_buckets(pos, xs, ys, B, T, lut1, cfg.rel_pos_bins // 2, lut2, cfg.rel_2d_pos_bins // 2)
        return ops.relpos_bias_fwd(BF16, bk[0], bk[1], bk[2], w1, wx, wy, scale, B, NH, T, key_mask=km)

    def on():
        lens, cu, live = ops.pack_plan(km)
        Tm = max(lens.tolist())
        pk = [ops.rows_pack(t, live, lens, None, Tm) for t in (pos, xs, ys)]
        bk = ops.relpos_buckets(pk[0], pk[1], pk[2], B, Tm, lut1, cfg.rel_pos_bins // 2, lut2, cfg.rel_2d_pos_bins // 2)
        return ops.relpos_bias_fwd(BF16, bk[0], bk[1], bk[2], w1, wx, wy, scale, B, NH, Tm)
    return off, on


def switch_cost():
    """(d) at full lengths: the launches the switch adds, one by one (medians of ROUNDS x 20 calls)"""
    km = key_mask([S] * B)
    x = torch.randn((B, T, H), device="cuda").to(BF16)
    lens, cu, live = ops.pack_plan(km)
    packed = ops.rows_pack(x, live, lens, cu, T, rows=B * T)
    parts = {"plan": ("peneo_pack_plan", lambda: ops.pack_plan(km)),
             "read": ("plan + the host read of lens (stream otherwise idle)", lambda: ops.pack_plan(km)[0].tolist()),
             "pack": ("pack of the hidden rows (8 x 709 x 1536 B)", lambda: ops.rows_pack(x, live, lens, cu, T, out=packed)),
             "pack4": ("per-document pack of one int32 array (three per forward)", lambda: ops.rows_pack(km, live, lens, None, T)),
             "unpack": ("unpack of the hidden rows", lambda: ops.rows_unpack(packed, live, lens, cu, out=x))}
    got = {}
    for key, (name, fn) in parts.items():
        timed(fn, 3)
        v = [timed(fn, 20) for _ in range(ROUNDS)]
        got[key] = med(v)
        print(f"(d) {name}: median {med(v) * 1e3:.1f} us (spread {(max(v) - min(v)) * 1e3:.1f} us)")
    total = got["read"] + got["pack"] + 3 * got["pack4"] + got["unpack"]
    print(f"(d) sum per forward (plan + host read, hidden pack, three int32 packs, unpack): {total * 1e3:.1f} us")


def child():
    """the off arm at full lengths: the eval forward"""
    m, batch = eval_model()
    go = forward_of(m, batch([S] * B), False)
    timed(go, 3)
    print(json.dumps({"root": ROOT, "forward_ms": med([timed(go, 10) for _ in range(3)])}))


def run_child(root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--child"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child {root} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, B={B} S={S} + {NV} visual tokens (T = {T}) bf16, H={H}")
    print(clocks())
    sets = length_sets()
    for name, lens in sets.items():
        print(f"lengths {name}: {lens}  rows {sum(n + NV for n in lens)} of {B * T}: row fraction {fraction(lens):.3f}, Tm {max(lens) + NV}")
    table = []
    make = layer_closures()
    for name, lens in sets.items():
        off, on, keep = make(lens)
        a, b = ab(f"(a) one encoder layer, {name}", fraction(lens), off, on, 10)
        table.append(("layer", name, fraction(lens), a, b))
        del off, on, keep
        torch.cuda.empty_cache()
    del make
    m, batch = eval_model()
    for name, lens in sets.items():
        off, on = bias_closures(m, batch(lens))
        a, b = ab(f"(b) bias build, {name}", fraction(lens), off, on, 10)
        table.append(("bias build", name, fraction(lens), a, b))
    for name, lens in sets.items():
        bt = batch(lens)
        a, b = ab(f"(c) eval forward of 8 documents, {name}", fraction(lens), forward_of(m, bt, False), forward_of(m, bt, True), 5)
        table.append(("forward", name, fraction(lens), a, b))
    m.set_skip_padded_tokens(False)
    del m, batch
    torch.cuda.empty_cache()
    switch_cost()
    print("summary (medians, ms):   what, lengths, row fraction, off, on, on / off")
    for what, name, frac, a, b in table:
        print(f"  {what:<12} {name:<7} {frac:.3f}  {a:8.3f}  {b:8.3f}  {b / a:.3f}")
    if ARGS.parent:
        rows = []
        for _ in range(ROUNDS):
            rows.append((run_child(os.path.abspath(ARGS.parent)), run_child(HERE)))
            print(f"(e) off arm, full lengths, fresh processes: forward parent {rows[-1][0]['forward_ms']:.3f} this tree "
                  f"{rows[-1][1]['forward_ms']:.3f} ms")
            sys.stdout.flush()
        a, b = [r[0]["forward_ms"] for r in rows], [r[1]["forward_ms"] for r in rows]
        gap, sa, sb = med(b) - med(a), max(a) - min(a), max(b) - min(b)
        verdict = "established" if abs(gap) > max(sa, sb) else "not established"
        print(f"(e) forward_ms median: parent {med(a):.3f} (spread {sa:.3f})  this tree {med(b):.3f} (spread {sb:.3f})  gap {gap:+.3f} ms: {verdict}")
    print(clocks())


if __name__ == "__main__":
    if ARGS.child:
        child()
    else:
        main()
