"""FusedAdamW(emit_into=model): the step writes the declarative working copies of the weights and stamps them current.
Every emitted entry must hold exactly what its builder makes from the current parameters, the next forward must not
rebuild it, everything else must stay lazy, and the model must compute what a freshly built model computes."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
LAZY = ("dec.ab", "dec.pack", "dec.pack2", "dec.pack_mxfp8")      # re-packs, a quantiser, a column split: never emitted


def build_model(pcfg, state_dict, dtype):
    from peneo_amd.model import PEneoConfig, PEneoModel
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    m.load_state_dict(state_dict, strict=True)
    return m.cuda().set_compute_dtype(dtype).eval()                # eval: dropout off, every forward deterministic


def setup(name, dtype, emit=True, freeze=None, max_grad_norm=1.0):
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    fx = load_golden(name)
    m = build_model(fx["config"], fx["state_dict"], dtype)
    if freeze is not None:
        freeze(m).requires_grad_(False)
    b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in fx["batch"].items()}
    opt = FusedAdamW(peneo_param_groups(m, 2e-3, 0.01, fx["config"]["peneo_downstream_speedup_ratio"]), max_grad_norm=max_grad_norm,
                     emit_into=m if emit else None)
    return fx, m, b, opt


def caches(m):
    from peneo_amd.model.engine import WeightCache
    out = []
    for mod in m.modules():
        wc = getattr(mod, "weight_cache", None)
        if isinstance(wc, WeightCache) and all(wc is not o for o in out):
            out.append(wc)
    assert len(out) == 2                                           # the backbone's and the decoder's
    return out


def builds(m):
    return {(i, k): n for i, wc in enumerate(caches(m)) for k, n in wc.builds.items()}


def fwd_bwd(m, b, opt):
    opt.zero_grad(set_to_none=True)
    m(**b)["loss"].backward()


def eval_loss(m, b):
    with torch.no_grad():
        return float(m(**b)["loss"])


def fresh_loss(fx, m, b, dtype):
    ref = build_model(fx["config"], {k: v.detach().clone() for k, v in m.state_dict().items()}, dtype)
    return eval_loss(ref, b)


def emitted(m, opt):
    cs = caches(m)
    return {([c is wc for c in cs].index(True), key) for wc, key in opt.emitted_keys()}


def check_emitted_entries(m, opt):
    """every entry the step wrote == its own builder, run in a fresh cache on the current parameters; stamped current"""
    from peneo_amd.model.engine import WeightCache
    assert opt.emitted_keys()
    for wc, key in opt.emitted_keys():
        name, args = wc.builder_of(key)
        assert name in ("cast", "cat_rows", "cat_vec")
        want = getattr(WeightCache(), name)(*args)
        stamp, have = wc._store[key]
        assert have.dtype == want.dtype and have.shape == want.shape and torch.equal(have, want), key
        assert key[0] not in LAZY and key[-1] != "mxfp8"
        assert wc.is_current(key, [p for p in (args[1] if isinstance(args[1], list) else [args[1]]) if p is not None]), key


def check_step(fx, m, b, opt, dtype, n_lazy=2, loss_rtol=0.0):
    """after an emitting step: contents, no rebuild of an emitted entry by the next forward (or backward), lazy ones rebuilt,
    and the loss of a freshly built model"""
    check_emitted_entries(m, opt)
    em, before = emitted(m, opt), builds(m)
    loss = eval_loss(m, b)
    after = builds(m)
    assert all(after[k] == before[k] for k in em), [k for k in em if after[k] != before[k]]
    lazy = [k for k in before if k[1][0] in ("dec.ab", "dec.pack") and k[1][1] == dtype]
    assert len(lazy) == n_lazy and all(after[k] == before[k] + 1 for k in lazy), lazy
    ref = fresh_loss(fx, m, b, dtype)
    print("loss", loss, "fresh model", ref)
    assert abs(loss - ref) <= loss_rtol * abs(ref), (loss, ref)       # (rtol 0: the same float)
    fwd_bwd(m, b, opt)                                             # (the backward's own entries, dec.w1cat, are hits too)
    assert all(builds(m)[k] == before[k] for k in em)
    return em


@pytest.mark.parametrize("name,dtype", [("lmv3_tiny", BF), ("lilt_tiny", BF), ("lmv3_tiny", F32)], ids=["lmv3-bf16", "lilt-bf16", "lmv3-fp32"])
def test_three_emitting_steps(name, dtype):
    fx, m, b, opt = setup(name, dtype)
    fwd_bwd(m, b, opt)
    for it in range(3):
        opt.step()
        em = check_step(fx, m, b, opt, dtype)                       # (leaves the gradients of the next iteration)
        names = {k[1][0] for k in em}
        bufs = {wc._store[key][1].dtype for wc, key in opt.emitted_keys()}
        assert {"L0.qkv", "L0.bqkv", "dec.bab", "dec.b1", "dec.b2", "dec.w1cat"} <= names, names
        if dtype == F32:
            assert bufs == {F32} and "L0.o" not in names            # fp32 compute: the casts are the parameters themselves
        elif name == "lilt_tiny":
            assert bufs == {BF, F32}
            assert {"L0.lqkv", "L0.blqkv", "L0.t.o", "L0.t.i", "L0.t.o2", "L0.l.o", "L0.l.i", "L0.l.o2", "boxlin"} <= names, names
        else:
            assert bufs == {BF, F32}
            assert {"L0.o", "L0.i", "L0.o2", "L1.qkv", "patch_proj", "dec.s0", "dec.s3"} <= names, names


@pytest.mark.parametrize("name,k", [("lmv3_tiny_cls1", 1), ("lmv3_tiny_cls3", 3)])
def test_other_classifier_depths(name, k):
    """1- and 3-layer classifiers run the per-head path: one cast per head and layer, no packed form"""
    fx, m, b, opt = setup(name, BF)
    fwd_bwd(m, b, opt)
    for _ in range(2):
        opt.step()
        # The per-head path sums its loss with fp32 atomics, so two forwards of ONE model with the same weights already differ in
        # the last bits (the 2-layer goldens above do not: there the loss must be the same float).  Bound: reordering a sum of n
        # fp32 partials moves it by at most (n - 1) * 2^-24 relative; 1e-5 covers ~160 partials per head.  A working copy left
        # stale by a step would show at the scale of the step itself: at these learning rates the loss moves by tens of percent.
        names = {key[1][0] for key in check_step(fx, m, b, opt, BF, n_lazy=1, loss_rtol=1e-5)}      # (lazy: dec.ab only)
        assert {f"dec.h{h}.{l}" for h in range(5) for l in range(k)} <= names, names
        assert {"L0.qkv", "L0.bqkv", "dec.bab", "dec.s0"} <= names and "dec.b1" not in names


def test_foreign_writes_still_invalidate():
    from peneo_amd.model.engine import bump_param_epoch
    fx, m, b, opt = setup("lmv3_tiny", BF)
    fwd_bwd(m, b, opt)
    opt.step()
    l0 = eval_loss(m, b)
    w = m.backbone.encoder.layer[1].intermediate.dense.weight
    with torch.no_grad():
        w.mul_(1.5)                                                # versioned in-place update
    l1 = eval_loss(m, b)
    assert l1 != l0 and l1 == fresh_loss(fx, m, b, BF)
    w.data.mul_(1.25)                                              # unversioned writes + the epoch bump
    m.peneo_decoder.ent_linking_h2h_fc[0].weight.data.mul_(0.5)
    bump_param_epoch()
    l2 = eval_loss(m, b)
    assert l2 != l1 and l2 == fresh_loss(fx, m, b, BF)
    fwd_bwd(m, b, opt)                                             # the rebuilt (re-allocated) entries are re-pointed
    opt.step()
    check_step(fx, m, b, opt, BF)


def test_entry_with_a_frozen_source_stays_lazy():
    fx, m, b, opt = setup("lmv3_tiny", BF, freeze=lambda m: m.backbone.encoder.layer[0].attention.self.key.weight)
    fwd_bwd(m, b, opt)
    for _ in range(2):
        before = builds(m)
        opt.step()
        em = check_step(fx, m, b, opt, BF)
        assert (0, ("L0.qkv", BF)) not in em and (0, ("L0.o", BF)) in em and (0, ("L1.qkv", BF)) in em
        assert builds(m)[(0, ("L0.qkv", BF))] == before[(0, ("L0.qkv", BF))] + 1


def test_state_dict_round_trip_and_a_parameter_that_joins_late():
    fx, m, b, opt = setup("lmv3_tiny", BF)
    late = m.backbone.encoder.layer[0].output.dense.weight         # the one source of L0.o2
    fwd_bwd(m, b, opt)
    late.grad = None                                               # no gradient in this step: not in the step's table
    opt.step()
    em = check_step(fx, m, b, opt, BF)
    assert (0, ("L0.o2", BF)) not in em and (0, ("L0.o", BF)) in em
    opt.step()                                                     # now it has one: the tables are rebuilt with it
    em = check_step(fx, m, b, opt, BF)
    assert (0, ("L0.o2", BF)) in em
    opt.load_state_dict(opt.state_dict())
    opt.step()
    assert (0, ("L0.o2", BF)) in check_step(fx, m, b, opt, BF)
    assert [int(float(opt.state_dict()["state"][i]["step"])) for i in (0, 1)] == [3, 3]


def test_switching_the_compute_dtype():
    fx, m, b, opt = setup("lmv3_tiny", BF)
    fwd_bwd(m, b, opt)
    opt.step()
    check_step(fx, m, b, opt, BF)
    m.set_compute_dtype(F32)
    fwd_bwd(m, b, opt)
    opt.step()                                                     # (still writes the bf16 copies the last bf16 forward used)
    check_step(fx, m, b, opt, F32)
    opt.step()
    em = check_step(fx, m, b, opt, F32)
    assert (0, ("L0.o", BF)) not in em and (0, ("L0.qkv", F32)) in em   # the bf16 copies are no longer written
    m.set_compute_dtype(BF)
    fwd_bwd(m, b, opt)
    opt.step()
    check_step(fx, m, b, opt, BF)
    opt.step()
    em = check_step(fx, m, b, opt, BF)
    assert (0, ("L0.o", BF)) in em and (0, ("L0.qkv", F32)) not in em


@pytest.mark.parametrize("name", ["lmv3_tiny", "lilt_tiny"])
def test_without_emission_every_entry_is_rebuilt_each_iteration(name):
    """the default: one build of every entry per iteration, as before the emitting mode existed"""
    fx, m, b, opt = setup(name, BF, emit=False)
    assert opt.emitted_keys() == []
    counts = []
    for _ in range(3):
        fwd_bwd(m, b, opt)
        opt.step()
        counts.append(builds(m))
    assert opt.emitted_keys() == [] and len(counts[0]) > 10
    assert set(counts[0]) == set(counts[2])
    for k in counts[0]:
        assert (counts[0][k], counts[1][k], counts[2][k]) == (1, 2, 3), k
    assert eval_loss(m, b) == fresh_loss(fx, m, b, BF)
