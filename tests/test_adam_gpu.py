"""GPU: clip + Adam / AdamW on the device.  ssc_adam_step against the float64 restatement (tests/adamref.py) within the derived
first-order bound of its fp32 evaluation; TrainEngine.clip_adam_step with the freeze schedule against torch.optim.Adam / AdamW fed
the device's own gradients; the optimiser spec through train_step and SelfCritical.step; the state in torch.optim.Adam's layout."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import adamref as R
import oracle
from goldenlib import group, load
from gpuutil import dev, engine_from
from ssc_runtime import lib as L
from ssc_runtime.engine import OptimSpec

pytestmark = pytest.mark.gpu
GUARD = 8
SENTINEL = -7.0


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def raw_step(p, g, m, v, sq, gscale, max_norm, lr, b1, b2, eps, wd, decoupled, step, n=None):
    lib = L.load()
    n = p.numel() if n is None else n
    rc = lib._raw_ssc_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, L.ptr(sq), gscale, max_norm, lr, b1, b2, eps, wd,
                                int(decoupled), step, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def guarded(values, off):
    """values (fp32, CPU) placed `off` elements into a 16-byte aligned device buffer between sentinel guards -> (buffer, slice)."""
    n = values.numel()
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32)
    buf[GUARD + off:GUARD + off + n] = values
    buf = buf.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + off:GUARD + off + n]


def guards_intact(buf, off, n):
    return bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all())


def inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 0.3
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.02
    quiet = torch.rand(n, generator=g) < 0.1            # elements with g = 0, m = v = 0
    if n >= 5:
        quiet[n // 2] = True
    grad[quiet] = 0
    m[quiet] = 0
    v[quiet] = 0
    return p, grad, m, v, quiet


WORST = {"p": 0.0, "m": 0.0, "v": 0.0}


def check_against_bound(got, want, tag):
    """|device - restatement| <= the first-order bound of adamref.step (operation counts: its docstring), per element."""
    for k in ("p", "m", "v"):
        err = np.abs(got[k].double().cpu().numpy() - want[k])
        bound = want["E" + k]
        frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        WORST[k] = max(WORST[k], frac)
        assert (err <= bound).all(), (tag, k, frac)
    return WORST


HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.001)
COMBOS = list(itertools.product((1, 2, 1000), (False, True), (True, False), (1.0, 0.5)))   # step, decoupled, clip active, gscale


def one_call(n, offs, seed, step, decoupled, clip, gscale):
    p, grad, m, v, quiet = inputs(n, seed)
    sq = (grad * grad).sum().reshape(1)
    norm = float(sq.sqrt()) * gscale
    max_norm = norm * (0.5 if clip else 2.0) if norm > 0 else 1.0
    bufs = [guarded(x, o) for x, o in zip((p, grad, m, v), offs)]
    h = HYPER
    rc = raw_step(*(s for _, s in bufs), sq.cuda(), gscale, max_norm, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], decoupled, step)
    assert rc == 0
    for (buf, _), o in zip(bufs, offs):
        assert guards_intact(buf, o, n), "a write outside the slice"
    assert torch.equal(bufs[1][1].cpu(), grad)                      # the gradient is read only
    want = R.step(p.double().numpy(), grad.double().numpy(), m.double().numpy(), v.double().numpy(), float(sq), gscale, R.f32(max_norm),
                  h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], decoupled, step)
    got = {"p": bufs[0][1], "m": bufs[2][1], "v": bufs[3][1]}
    check_against_bound(got, want, (n, offs, step, decoupled, clip, gscale))
    q = quiet.numpy()
    if decoupled:                                                 # g = m = v = 0 under AdamW: the moments stay exactly 0
        assert (got["m"].cpu().numpy()[q] == 0).all() and (got["v"].cpu().numpy()[q] == 0).all()
    return got


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 1027, 262151])
def test_kernel_matches_the_restatement_within_the_derived_bound(n, off):
    for i, (step, decoupled, clip, gscale) in enumerate(COMBOS):
        one_call(n, (off,) * 4, 1000 * n + 10 * off + i, step, decoupled, clip, gscale)
    print("largest error / bound so far:", {k: round(x, 4) for k, x in WORST.items()})


@pytest.mark.parametrize("n", [5, 1027, 262151])
def test_kernel_with_mixed_offsets_takes_the_scalar_path(n):
    for i, (step, decoupled, clip, gscale) in enumerate(COMBOS[::5]):
        one_call(n, (0, 1, 2, 3), 77 * n + i, step, decoupled, clip, gscale)
        one_call(n, (3, 3, 1, 3), 78 * n + i, step, decoupled, clip, gscale)
    print("largest error / bound so far:", {k: round(x, 4) for k, x in WORST.items()})


@pytest.mark.parametrize("decoupled", [False, True])
def test_five_steps_fed_back_no_drift_and_two_runs_bit_identical(decoupled):
    n, off, h = 1027, 1, HYPER
    runs = []
    for _ in range(2):
        p, grad0, m, v, _q = inputs(n, 31)
        (bp, sp), (bm, sm), (bv, sv) = guarded(p, off), guarded(m, off), guarded(v, off)
        gen = torch.Generator().manual_seed(32)
        for step in range(1, 6):
            grad = torch.randn(n, generator=gen) * 0.3
            bg, sg = guarded(grad, off)
            sq = (grad * grad).sum().reshape(1)
            before = [x.double().cpu().numpy() for x in (sp, sg, sm, sv)]     # the device's own state goes into the restatement
            assert raw_step(sp, sg, sm, sv, sq.cuda(), 1.0, 2.0, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], decoupled, step) == 0
            want = R.step(*before, float(sq), 1.0, 2.0, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], decoupled, step)
            check_against_bound({"p": sp, "m": sm, "v": sv}, want, ("fed back", step, decoupled))
        runs.append((bp.clone(), bm.clone(), bv.clone()))
    for a, b in zip(*runs):
        assert same_bits(a, b)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("off", [0, 2])
def test_all_zero_elements_stay_exactly_zero(decoupled, off):
    """What the padding columns of the flat layout hold: p = g = m = v = 0, with weight decay on, under both kinds."""
    n = 1027
    p, grad, m, v, _q = inputs(n, 41)
    pad = torch.arange(n) % 7 == 3
    for x in (p, grad, m, v):
        x[pad] = 0
    sq = (grad * grad).sum().reshape(1).cuda()
    bufs = [guarded(x, off) for x in (p, grad, m, v)]
    for step in (1, 2, 3):
        assert raw_step(*(s for _, s in bufs), sq, 1.0, 0.5, 1e-3, 0.9, 0.999, 1e-8, 0.1, decoupled, step) == 0
        for k in (0, 2, 3):
            x = bufs[k][1].cpu()
            assert same_bits(x[pad], torch.zeros(int(pad.sum()))), (k, step)     # +0, not even -0
            assert bool((x[~pad] != 0).any())


def test_refused_calls_launch_nothing_and_n0_succeeds():
    n = 37
    p, grad, m, v, _q = inputs(n, 51)
    bufs = [guarded(x, 0) for x in (p, grad, m, v)]
    keep = [b.clone() for b, _ in bufs]
    sq = (grad * grad).sum().reshape(1).cuda()
    sl = [s for _, s in bufs]
    ok = dict(gscale=1.0, max_norm=1.0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, decoupled=0, step=1)
    lib = L.load()

    def call(ptrs, sqp, a, count=n):
        rc = lib._raw_ssc_adam_step(*ptrs, count, sqp, a["gscale"], a["max_norm"], a["lr"], a["b1"], a["b2"], a["eps"], a["wd"],
                                    a["decoupled"], a["step"], L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    ptrs = [L.ptr(s) for s in sl]
    for k in range(4):
        assert call(ptrs[:k] + [None] + ptrs[k + 1:], L.ptr(sq), ok) == -1
    assert call(ptrs, None, ok) == -1
    for bad in (dict(step=0), dict(step=-1), dict(b1=1.0), dict(b1=-0.5), dict(b2=1.0), dict(b2=1.5), dict(b1=float("nan")),
                dict(eps=0.0), dict(eps=-1.0), dict(lr=-1e-3), dict(wd=-0.01)):
        assert call(ptrs, L.ptr(sq), dict(ok, **bad)) == -1, bad
    assert call(ptrs, L.ptr(sq), ok, count=0) == 0
    odd = [C.c_void_p(x.data_ptr() + 2) for x in sl]                 # no multiple of 4: no float pointer, SSC_EALIGN
    for k in range(4):
        assert call(ptrs[:k] + [odd[k]] + ptrs[k + 1:], L.ptr(sq), ok, count=n - 1) == -2
    for (b, _), k in zip(bufs, keep):
        assert same_bits(b, k)                                       # nothing was launched: every buffer is as it was
    assert call(ptrs, L.ptr(sq), ok) == 0 and not same_bits(bufs[0][0], keep[0])


# ---- engine -----------------------------------------------------------------------------------------------------------------
# lr, betas, eps, weight decay and the clip norm are exact in fp32: torch (float64 scalars) and the device (fp32 arguments) then
# apply the same numbers, and what is left between them is the fp32 evaluation the bound describes
ENG = dict(lr=2.0 ** -10, betas=(0.875, 1 - 2.0 ** -9), eps=2.0 ** -27, wd=2.0 ** -10, max_norm=0.5)


@functools.lru_cache(maxsize=None)
def toy():
    d, cfgd = load("g1_train_sv1")
    cfg = oracle.OracleConfig(**cfgd)
    assert cfg.sentiment_vae == 1
    ins = group(d, "in/")
    batch = (dev(ins["feats"]), dev(ins["caps"]), dev(ins["sentiment"]), dev(ins["eps"]))
    return cfg, group(d, "param/"), batch


def unpad(flat, store, name):
    """Tensor `name` out of a flat buffer laid out as `store` (offsets / shapes; rows of 2-D weights padded to 4 floats)."""
    o, cnt = store.offsets[name]
    shp = store.shapes[name]
    if len(shp) == 2 and shp[0] > 1:
        return flat[o:o + cnt].view(shp[0], cnt // shp[0])[:, :shp[1]]
    return flat[o:o + shp[-1]].view(*shp)


def padding_mask(store):
    mask = torch.ones(store.numel, dtype=torch.bool, device=store.flat.device)
    for n in store.shapes:
        unpad(mask, store, n).fill_(False)
    return mask


def upstream(B, kld_weight=750.0):
    return torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * kld_weight), device="cuda")


def four_iterations(kind, check=True):
    """Decoder LSTM frozen on iterations 1-2, trained on 3-4; torch.optim on CPU float64 gets the device's own gradients."""
    cfg, params, batch = toy()
    eng = engine_from(cfg, params)
    names = list(eng.params.shapes)
    ref = {n: torch.nn.Parameter(eng.params.views[n].detach().double().cpu().clone()) for n in names}
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    opt = cls([ref[n] for n in names], lr=ENG["lr"], betas=ENG["betas"], eps=ENG["eps"], weight_decay=ENG["wd"])
    errs = {n: (0.0, 0.0, 0.0) for n in names}
    gl, gk = upstream(batch[1].size(0))
    clipped = 0
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for it in range(1, 5):
        frozen = it <= 2
        eng.forward(*batch)
        eng.backward(gl, gk, skip=eng.decoder_names if frozen else ())
        live = [n for n in names if not (frozen and n in eng.decoder_names)]
        for n in names:
            ref[n].grad = unpad(eng.grads.flat, eng.grads, n).detach().double().cpu().clone() if n in live else None
        sq = float(sum((ref[n].grad ** 2).sum() for n in live))
        clipped += np.sqrt(sq) > ENG["max_norm"]
        lo, hi = eng.trainable_range(frozen)
        before = {n: (ref[n].detach().numpy().copy(),) + tuple(
            opt.state[ref[n]][k].numpy().copy() if ref[n] in opt.state else np.zeros(ref[n].shape) for k in ("exp_avg", "exp_avg_sq"))
            for n in live}
        grads = {n: ref[n].grad.numpy().copy() for n in live}
        torch.nn.utils.clip_grad_norm_([ref[n] for n in live], ENG["max_norm"])
        opt.step()
        eng.clip_adam_step(ENG["lr"], ENG["betas"], ENG["eps"], ENG["wd"], kind == "adamw", ENG["max_norm"], frozen)
        torch.cuda.synchronize()
        if not check:
            continue
        for n in live:
            step = int(opt.state[ref[n]]["step"])
            assert step == (it - 2 if n in eng.decoder_names else it)
            b = R.step(before[n][0], grads[n], before[n][1], before[n][2], sq, 1.0, ENG["max_norm"], ENG["lr"], *ENG["betas"], ENG["eps"],
                       ENG["wd"], kind == "adamw", step, err_in=errs[n], sq_rel_err=R.sq_norm_rel_err(hi - lo))
            errs[n] = (b["Ep"], b["Em"], b["Ev"])
            st = opt.state[ref[n]]
            # the restatement follows torch (1e-12), so the bound it carries is the bound around torch's values
            assert np.abs(b["p"] - ref[n].detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(b["p"]).max())
            for k, flat, want in (("p", eng.params.flat, ref[n].detach()), ("m", eng.exp_avg, st["exp_avg"]), ("v", eng.exp_avg_sq, st["exp_avg_sq"])):
                err = (unpad(flat, eng.params, n).double().cpu() - want).abs().numpy()
                frac = float((err / np.maximum(b["E" + k], 1e-300)).max())
                worst[k] = max(worst[k], frac)
                assert (err <= b["E" + k]).all(), (kind, it, n, k, frac)
    if check:
        print(f"{kind}: clip active on {clipped} of 4 iterations; largest error / accumulated bound:", {k: round(x, 4) for k, x in worst.items()})
        assert clipped >= 1, "the clip was never active: the toy gradients are smaller than ENG['max_norm']"
    return eng, names, ref, opt


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_engine_follows_torch_through_the_freeze_schedule(kind):
    eng, names, ref, opt = four_iterations(kind)
    assert eng.adam_steps == [4, 2] and eng.steps_done == 4
    spec = OptimSpec(kind, betas=ENG["betas"], eps=ENG["eps"])
    sd = eng.optimizer_state_dict([(n, None) for n in names], ENG["lr"], 0.9, ENG["wd"], 4, spec)
    for i, n in enumerate(names):
        assert float(sd["state"][i]["step"]) == (2 if n in eng.decoder_names else 4), n
        assert sd["state"][i]["step"].dtype == torch.float32 and tuple(sd["state"][i]["exp_avg"].shape) == tuple(eng.params.shapes[n])
    pad = padding_mask(eng.params)
    assert int(pad.sum()) > 0
    for flat in (eng.params.flat, eng.exp_avg, eng.exp_avg_sq):
        assert same_bits(flat[pad], torch.zeros(int(pad.sum())))


def test_decoder_before_its_first_step_has_no_state_entry():
    cfg, params, batch = toy()
    eng = engine_from(cfg, params)
    gl, gk = upstream(batch[1].size(0))
    eng.forward(*batch)
    eng.backward(gl, gk, skip=eng.decoder_names)
    dec0 = eng.params.flat[eng.params.range_of(eng.decoder_names)[0]:].clone()
    eng.clip_adam_step(1e-3, decoder_frozen=True)
    names = list(eng.params.shapes)
    sd = eng.optimizer_state_dict([(n, None) for n in names], 1e-3, 0.9, 0.0, 1, OptimSpec("adam"))
    assert sorted(sd["state"]) == [i for i, n in enumerate(names) if n not in eng.decoder_names]
    assert same_bits(eng.params.flat[eng.params.range_of(eng.decoder_names)[0]:], dec0)       # frozen: not touched


HP = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=12.5)


def test_optim_none_is_todays_sgd_step_bit_for_bit():
    cfg, params, batch = toy()
    a, b, c = (engine_from(cfg, params) for _ in range(3))
    gl, gk = upstream(batch[1].size(0), HP["kld_weight"])
    for it, frozen in enumerate((True, False, False)):
        la, ka = a.train_step(*batch, decoder_frozen=frozen, optim=None, **HP)
        lc, kc = c.train_step(*batch, decoder_frozen=frozen, optim=OptimSpec("sgd"), **HP)      # the spec's SGD: the call's arguments
        lb, kb = b.forward(*batch)
        b.backward(gl, gk, skip=b.decoder_names if frozen else ())
        b.clip_sgd_step(HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"], frozen)
        assert torch.equal(la, lb) and torch.equal(ka, kb) and torch.equal(lc, lb)
        for x in (a, c):
            assert same_bits(x.params.flat, b.params.flat) and same_bits(x.momentum, b.momentum)
        assert a.exp_avg is None and a.adam_steps == [0, 0]
    # a spec's own momentum / weight decay go into the step AND into the state dict's param group
    own = OptimSpec("sgd", momentum=0.5, weight_decay=0.0)
    d, e = engine_from(cfg, params), engine_from(cfg, params)
    d.train_step(*batch, optim=own, **HP)
    e.forward(*batch)
    e.backward(gl, gk)
    e.clip_sgd_step(HP["lr"], 0.5, 0.0, HP["max_norm"], False)
    assert same_bits(d.params.flat, e.params.flat) and not same_bits(d.params.flat, a.params.flat)
    names = [(n, None) for n in d.params.shapes]
    grp = d.optimizer_state_dict(names, HP["lr"], HP["momentum"], HP["weight_decay"], 1, own)["param_groups"][0]
    assert grp["momentum"] == 0.5 and grp["weight_decay"] == 0.0
    grp = d.optimizer_state_dict(names, HP["lr"], HP["momentum"], HP["weight_decay"], 1)["param_groups"][0]
    assert grp["momentum"] == HP["momentum"] and grp["weight_decay"] == HP["weight_decay"]


@pytest.mark.parametrize("frozen", [False, True])
def test_self_critical_step_with_optim_none_is_todays_sgd_step_bit_for_bit(frozen):
    """SelfCritical.step(optim=None) and backward_update(optim=None) with the advantage-weighted upstream against rollout + forward +
    backward + clip_sgd_step composed by hand: parameters and momentum, two steps; no Adam state appears."""
    from test_scst_gpu import SEED, fresh, setup
    s = setup(1, 0)
    a, sa = fresh(s)
    b, sb = fresh(s)
    c, sc = fresh(s)
    for k in range(2):
        loss, kld, stats = sa.step(s["feats"], [0, 1, 2], s["senti"], seed=SEED + k, decoder_frozen=frozen, optim=None, **HP)
        ro = sb.rollout(s["feats"], [0, 1, 2], s["senti"], SEED + k, kld_weight=HP["kld_weight"])
        lb, kb = b.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
        b.backward(ro.gl, ro.gk, skip=b.decoder_names if frozen else ())
        b.clip_sgd_step(HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"], frozen)
        ro = sc.rollout(s["feats"], [0, 1, 2], s["senti"], SEED + k, kld_weight=HP["kld_weight"])
        c.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
        c.backward_update(ro.gl, ro.gk, HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"], frozen, optim=None)
        assert torch.equal(loss, lb) and torch.equal(kld, kb) and torch.equal(stats, ro.stats)
        for x in (a, c):
            assert same_bits(x.params.flat, b.params.flat) and same_bits(x.momentum, b.momentum)
            assert x.exp_avg is None and x.exp_avg_sq is None and x.adam_steps == [0, 0]
    assert not torch.equal(a.params.flat, s["eng"].params.flat)     # (the steps moved the parameters)


def test_train_step_with_an_adam_spec_is_its_hand_composition():
    cfg, params, batch = toy()
    a, b = engine_from(cfg, params), engine_from(cfg, params)
    gl, gk = upstream(batch[1].size(0), HP["kld_weight"])
    spec = OptimSpec("adamw", betas=(0.8, 0.99), eps=1e-6, weight_decay=0.02)
    for frozen in (True, False):
        a.train_step(*batch, lr=1e-3, decoder_frozen=frozen, optim=spec)
        b.forward(*batch)
        b.backward(gl, gk, skip=b.decoder_names if frozen else ())
        b.clip_adam_step(1e-3, (0.8, 0.99), 1e-6, 0.02, True, 12.5, frozen)
        for x, y in ((a.params.flat, b.params.flat), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
            assert same_bits(x, y)
    assert a.adam_steps == [2, 1] and a.momentum is None


def test_state_dict_loads_into_torch_and_into_a_fresh_engine():
    from test_module_gpu import build_model
    eng, names, ref, opt = four_iterations("adam", check=False)
    cfg, params, batch = toy()
    model = build_model(cfg, params, beam=1)
    named = list(model.named_parameters())
    spec = OptimSpec("adam", betas=ENG["betas"], eps=ENG["eps"])
    sd = eng.optimizer_state_dict(named, ENG["lr"], 0.9, ENG["wd"], 4, spec)
    topt = torch.optim.Adam(model.parameters())
    topt.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    assert topt.param_groups[0]["betas"] == ENG["betas"] and topt.param_groups[0]["weight_decay"] == ENG["wd"]
    for (n, p) in named:
        assert float(topt.state[p]["step"]) == (2 if n in eng.decoder_names else 4)
        assert same_bits(topt.state[p]["exp_avg"], unpad(eng.exp_avg, eng.params, n))
    # (torch advances `step` in place: a dict that an optimiser has loaded is not reused)
    sd = eng.optimizer_state_dict(named, ENG["lr"], 0.9, ENG["wd"], 4, spec)
    other = engine_from(cfg, eng.state_dict())
    other.load_optimizer_state_dict(named, sd, spec)
    assert other.adam_steps == [4, 2]
    gl, gk = upstream(batch[1].size(0))
    for x in (eng, other):
        x.forward(*batch)
        x.backward(gl, gk)
        x.clip_adam_step(ENG["lr"], ENG["betas"], ENG["eps"], ENG["wd"], False, ENG["max_norm"], False)
    for x, y in ((eng.params.flat, other.params.flat), (eng.exp_avg, other.exp_avg), (eng.exp_avg_sq, other.exp_avg_sq)):
        assert same_bits(x, y)
    # the other kind's state is refused by name, both ways
    with pytest.raises(ValueError, match=r"'adam'.*'sgd'"):
        other.load_optimizer_state_dict(named, sd)
    sgd = engine_from(cfg, params)
    sgd.forward(*batch)
    sgd.backward(gl, gk)
    sgd.clip_sgd_step(0.015)
    with pytest.raises(ValueError, match=r"'sgd'.*'adam'"):
        other.load_optimizer_state_dict(named, sgd.optimizer_state_dict(named, 0.015, 0.9, 0.001, 1), spec)


def test_self_critical_step_with_adam_is_its_hand_composition():
    from test_scst_gpu import SEED, fresh, setup
    s = setup(1, 0)
    a, sa = fresh(s)
    b, sb = fresh(s)
    spec = OptimSpec("adam", betas=(0.9, 0.999), eps=1e-8)
    for k, frozen in enumerate((True, False)):
        loss, kld, stats = sa.step(s["feats"], [0, 1, 2], s["senti"], lr=5e-5, seed=SEED + k, decoder_frozen=frozen, weight_decay=0.0,
                                   optim=spec)
        ro = sb.rollout(s["feats"], [0, 1, 2], s["senti"], SEED + k)
        lb, kb = b.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
        b.backward_update(ro.gl, ro.gk, 5e-5, weight_decay=0.0, decoder_frozen=frozen, optim=spec)
        assert torch.equal(loss, lb) and torch.equal(kld, kb)
        for x, y in ((a.params.flat, b.params.flat), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
            assert same_bits(x, y)
    assert a.adam_steps == [2, 1] and not torch.equal(a.params.flat, s["eng"].params.flat)
    # ... and backward_update(optim=adam) is backward + clip_adam_step
    c, sc = fresh(s)
    ro = sc.rollout(s["feats"], [0, 1, 2], s["senti"], SEED)
    c.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
    c.backward(ro.gl, ro.gk, skip=c.decoder_names)
    c.clip_adam_step(5e-5, (0.9, 0.999), 1e-8, 0.0, False, 12.5, True)
    d, sd_ = fresh(s)
    sd_.step(s["feats"], [0, 1, 2], s["senti"], lr=5e-5, seed=SEED, decoder_frozen=True, weight_decay=0.0, optim=spec)
    assert same_bits(c.params.flat, d.params.flat) and same_bits(c.exp_avg_sq, d.exp_avg_sq)


def test_module_scst_step_passes_the_spec_on():
    from test_module_gpu import build_model
    from test_scst_gpu import N_, P_, SEED, fresh, setup
    s = setup(1, 0)
    spec = OptimSpec("adamw", weight_decay=0.01)
    m = build_model(s["cfg"], s["params"], beam=1)
    m.train()
    loss, kld, stats = m.scst_step(s["feats"], [0, 1, 2], s["senti"].view(P_, 1), references=s["references"], seed=SEED, n_samples=N_,
                                   lr=5e-5, optim=spec)
    a, sa = fresh(s)
    la, ka, st = sa.step(s["feats"], [0, 1, 2], s["senti"], lr=5e-5, seed=SEED, optim=spec)
    assert torch.equal(loss, la) and torch.equal(kld, ka)
    sd = m.state_dict()
    for k, v in a.state_dict().items():
        assert same_bits(sd[k], v), k
    assert m._engine().adam_steps == [1, 1] and same_bits(m._engine().exp_avg, a.exp_avg)
