"""GPU: KL annealing and the free-bits floor of the train step.  Kernel level: ssc_latent_fwd_fb / ssc_latent_fb_finish /
ssc_latent_bwd_fb against the float64 reference (tests/freebitsref.py) from the same fp32 inputs, at the shapes that cross every
boundary of the two forward forms.  Train step: ssc_train_fwd_opts / ssc_train_bwd_opts (the floor in ssc_train_opts) against the CPU oracle, whose
per-step mean / log_var / prior_mean stay in the autograd graph and become the floored KL through freebitsref; off and saturated
floors, determinism, the phased backward, the module and its neighbours, scripts/train.py.

Every test picks its floor from the reference (freebitsref.pick_lambda: the midpoint of the widest gap of what the mode compares,
between the 30th and 70th percentile) and asserts on the CPU that both gate states occur and that half the gap is at least ten
times the bound then put on the device's KL, so no gate can differ between fp32 and float64.

Bounds.  kld_b is a sum of n <= T Z terms of one sign (a KL element is >= 0 up to the 1e-5 of the denominator): lane-strided
partial sums (<= ceil(Z / 64) additions), the wave tree (6), the waves of a row (<= 4), the steps (T) - any term passes through at
most 4 + 6 + 4 + T <= 30 fp32 roundings of partial sums no larger than the total: 30 * 2^-24 = 1.8e-6 of |ref|, next to a few
2^-24 per element for expf / logf and the bracket.  kl_tol = 1e-4 + 1e-5 max|ref| (the bound tests/test_train_gpu.py puts on kld)
covers it five times over, the absolute part the train step's own error in mean / log_var.  Gradients: the element-wise formulas, a
handful of roundings of their operands - grad_tol = 1e-4 max(max|ref|, 1e-3) + 2e-6, the project's bound for gradients."""
import ctypes as C
import functools
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import freebitsref as fr
import oracle
from gpuutil import dev, engine_from, maxdiff
from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 1e30
MODE_NAME = {1: "element", 2: "step", 3: "dim"}
P_CELL = "_updown_cell."


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def kl_tol(ref):
    return 1e-4 + 1e-5 * float(ref.detach().abs().max())


def grad_tol(ref):
    return 1e-4 * max(float(ref.detach().abs().max()), 1e-3) + 2e-6


def r4(x):
    return (x + 3) // 4 * 4


def P(t):
    return None if t is None else t.data_ptr()


def floor_for(k, w, mode, select=None):
    """(lam, kld, gate, K) of the reference at the floor picked for `mode`; asserts the two conditions every test needs.
    select: a mask over what the mode compares (the train step never looks at rows without weight)."""
    vals = fr.compared(k, w, mode)
    lam, half = fr.pick_lambda(vals if select is None else vals[select])
    kld, gate, K = fr.floored(k, w, lam, mode)
    g = gate if select is None else gate[select]
    assert bool(g.any()) and not bool(g.all()), "both gate states must occur"
    assert half >= 10 * kl_tol(kld), (half, kl_tol(kld))
    return lam, kld, gate, K


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------
T_K = 4
# (B, Z, nslab, kld_mode, per-element prior mean and its gradient): a lane round; the 8-slab unroll; rows that do not fill the
# block's four waves; the many-slab form at one wave per row width and at four; a width that form declines; that form at two waves
# per row width, where each of its two parts of 20 slabs completes a full round of 16 loads and then a remainder
KSHAPES = [(1, 5, 1, 0, False), (3, 64, 3, 1, False), (5, 100, 9, 1, False), (2, 64, 17, 0, False), (4, 200, 20, 2, True),
           (4, 150, 20, 2, False), (3, 128, 40, 1, False)]


@functools.lru_cache(maxsize=None)
def kcase(B, Z, nslab, kmode, has_pm, mode):
    """Inputs of T_K steps of one shape, made so that what `mode` compares falls into two groups (terms near 0 and terms above 1)
    with the gap between them inside the percentile window, and their float64 references.  Shared, changed by none."""
    g = torch.Generator().manual_seed(7000 + 131 * B + 17 * Z + nslab + 5 * mode)
    T = T_K
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    tt, bb, jj = torch.meshgrid(torch.arange(T), torch.arange(B), torch.arange(Z), indexing="ij")
    w = ((tt[:, :, 0] + 2 * bb[:, :, 0]) % 3 != 2).float()                     # zeros in every column of B (B = 1: step 2)
    flag = {1: rnd(T, B, Z) < 0.5, 2: (tt + bb) % 2 == 0, 3: jj % 2 == 0}[mode]
    sign = lambda: torch.where(rnd(T, B, Z) < 0.5, -1.0, 1.0).double()
    delta = torch.where(flag, sign() * (1.5 + rnd(T, B, Z)), 0.15 * (2 * rnd(T, B, Z) - 1))
    lv_t = torch.where(flag, sign() * (0.5 + 0.5 * rnd(T, B, Z)), 0.1 * (2 * rnd(T, B, Z) - 1))
    prior_var = 1.0 if kmode == 0 else 0.8
    sent = torch.randint(-1, 2, (B,), generator=g).float()
    pm = (torch.randn(T, B, Z, generator=g) * 0.3) if has_pm else None
    prior_mean = torch.zeros(T, B, Z, dtype=torch.float64) if kmode == 0 else (
        pm.double() if has_pm else (0.5 * sent.double()).view(1, B, 1).expand(T, B, Z))
    bmu, blv = torch.randn(Z, generator=g) * 0.1, torch.randn(Z, generator=g) * 0.1
    slabs = torch.randn(T, nslab, B, 2 * Z, generator=g) * 0.3
    target = torch.cat([prior_mean + delta - bmu.double(), lv_t - blv.double()], -1)
    slabs[:, -1] = (target - slabs[:, :-1].double().sum(1)).float()
    eps = torch.randn(T, B, Z, generator=g)
    # float64 reference from the fp32 inputs
    tot = slabs.double().sum(1)
    m, l = tot[..., :Z] + bmu.double(), tot[..., Z:] + blv.double()
    z = eps.double() * (0.5 * l).exp() + m
    k = fr.k_elem(m, l, prior_mean, prior_var, kmode)
    lam, kld, gate, K = floor_for(k, w, mode)
    dz = torch.randn(T, 2, B, r4(Z), generator=g)                              # two split-K slabs of dz per step
    gk = torch.tensor([0.7, -1.3, 0.25, 0.9, -0.4])[:B]
    dmu_k, dlv_k, dpm_k = fr.dlatent(m, l, prior_mean, prior_var, kmode, w, gk, gate)
    dzs = dz.double().sum(1)[..., :Z]
    want_dmu = dzs + dmu_k
    want_dlv = dzs * eps.double() * 0.5 * (0.5 * l).exp() + dlv_k
    return dict(B=B, Z=Z, nslab=nslab, kmode=kmode, has_pm=has_pm, mode=mode, w=w, sent=sent, pm=pm, prior_var=prior_var,
                prior_mean=prior_mean, bmu=bmu,
                blv=blv, slabs=slabs, eps=eps, m=m, l=l, z=z, k=k, lam=lam, kld=kld, raw=fr.raw(k, w), gate=gate, K=K, dz=dz, gk=gk,
                dmu=want_dmu, dlv=want_dlv, dpm=dpm_k)


def run_kernels(c, lam, plain=False, zero_dz=False):
    """T_K forward steps (+ the finish of mode 3) and T_K backward steps on fresh device buffers with poisoned padding."""
    lib = L.load()
    B, Z, T, mode = c["B"], c["Z"], T_K, c["mode"]
    ldz, lddim, ldd, ldpm = r4(Z) + 4, r4(Z) + 4, 2 * Z + 3, r4(Z)
    st = L.stream_ptr()
    slabs, eps, w, sent = dev(c["slabs"]), dev(c["eps"]), dev(c["w"]), dev(c["sent"])
    bmu, blv, gk = dev(c["bmu"]), dev(c["blv"]), dev(c["gk"])
    pm = None
    if c["has_pm"]:
        pm = torch.full((T, B, ldpm), POISON, device="cuda")
        pm[:, :, :Z] = dev(c["pm"])
    mu, lv, z = (torch.full((T, B, ldz), POISON, device="cuda") for _ in range(3))
    kld, raw = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    gate_step = torch.full((T, B), float("nan"), device="cuda")
    acc = torch.full((B, lddim), POISON, device="cuda")
    acc[:, :Z] = 0
    kdim, gate_dim = torch.full((Z + 2,), POISON, device="cuda"), torch.full((Z + 2,), POISON, device="cuda")
    dz = torch.zeros_like(c["dz"]).cuda() if zero_dz else dev(c["dz"])
    dmulv = torch.full((T, B, ldd), POISON, device="cuda")
    dpm = torch.full((T, B, ldpm + 4), POISON, device="cuda")

    def fbdesc(t):
        fb = L.FreeBits()
        fb.lambda_, fb.mode = lam, mode
        fb.kld_raw, fb.gate_step, fb.dim_acc, fb.lddim, fb.gate_dim = P(raw), P(gate_step[t]), P(acc), lddim, P(gate_dim)
        return fb

    for t in range(T):
        d = L.LatentFwdDesc()
        d.B, d.Z = B, Z
        d.mulv, d.ldmulv, d.nslab, d.slab_stride = P(slabs[t]), 2 * Z, c["nslab"], B * 2 * Z
        d.bmu, d.blv, d.eps, d.ldeps = P(bmu), P(blv), P(eps[t]), Z
        d.kld_mode, d.sent, d.pm_scale, d.prior_var = c["kmode"], P(sent) if c["kmode"] and not c["has_pm"] else None, 0.5, c["prior_var"]
        d.w, d.mu, d.lv, d.z, d.ldz, d.kld_acc = P(w[t]), P(mu[t]), P(lv[t]), P(z[t]), ldz, P(kld)
        if pm is not None:
            d.pm, d.ldpm = P(pm[t]), ldpm
        if plain:
            lib.ssc_latent_fwd(C.byref(d), st)
        else:
            fb = fbdesc(t)
            lib.ssc_latent_fwd_fb(C.byref(d), C.byref(fb), st)
    if not plain and mode == 3 and lam > 0:
        lib.ssc_latent_fb_finish(P(acc), lddim, B, Z, lam, P(kdim), P(gate_dim), P(kld), st)
    for t in range(T):
        d = L.LatentBwdDesc()
        d.B, d.Z = B, Z
        d.dz, d.lddz, d.nslab, d.slab_stride = P(dz[t]), r4(Z), 2, B * r4(Z)
        d.eps, d.ldeps, d.mu, d.lv, d.ldz = P(eps[t]), Z, P(mu[t]), P(lv[t]), ldz
        d.kld_mode, d.sent, d.pm_scale, d.prior_var = c["kmode"], P(sent) if c["kmode"] and not c["has_pm"] else None, 0.5, c["prior_var"]
        d.w, d.gk, d.dmulv, d.lddmulv = P(w[t]), P(gk), P(dmulv[t]), ldd
        if pm is not None:
            d.pm, d.ldpm, d.dpm, d.lddpm = P(pm[t]), ldpm, P(dpm[t]), ldpm + 4
        if plain:
            lib.ssc_latent_bwd(C.byref(d), st)
        else:
            fb = fbdesc(t)
            lib.ssc_latent_bwd_fb(C.byref(d), C.byref(fb), st)
    torch.cuda.synchronize()
    return dict(mu=mu, lv=lv, z=z, kld=kld, raw=raw, gate_step=gate_step, acc=acc, kdim=kdim, gate_dim=gate_dim, dmulv=dmulv, dpm=dpm)


def device_gate(c, out):
    """The gates the device used, in the shape of the reference's (mode 1 keeps none: None)."""
    if c["mode"] == 2:
        return out["gate_step"].cpu() != 0
    if c["mode"] == 3:
        return out["gate_dim"][:c["Z"]].cpu() != 0
    return None


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("B,Z,nslab,kmode,has_pm", KSHAPES)
def test_kernels_match_float64(B, Z, nslab, kmode, has_pm, mode):
    c = kcase(B, Z, nslab, kmode, has_pm, mode)
    out = run_kernels(c, c["lam"])
    base = run_kernels(c, 0.0, plain=True)
    for name in ("mu", "lv", "z"):                                             # the plain kernel's bits, padding untouched
        assert torch.equal(bits(out[name]), bits(base[name])), name
        assert bool((out[name][:, :, Z:] == POISON).all()), name
        assert maxdiff(out[name][:, :, :Z], c[{"mu": "m", "lv": "l", "z": "z"}[name]]) <= 1e-5
    assert torch.equal(bits(out["raw"]), bits(base["kld"]))                    # the raw KL is the plain kernel's, bit for bit
    dm, dl = out["dmulv"][:, :, :Z].cpu(), out["dmulv"][:, :, Z:2 * Z].cpu()
    print(f"B={B} Z={Z} nslab={nslab} kld_mode={kmode} mode={mode} lam={c['lam']:.4g}: kld err {maxdiff(out['kld'], c['kld']):.3e} "
          f"(tol {kl_tol(c['kld']):.3e}), raw err {maxdiff(out['raw'], c['raw']):.3e}, dmu err {maxdiff(dm, c['dmu']):.3e} "
          f"(tol {grad_tol(c['dmu']):.3e}), dlv err {maxdiff(dl, c['dlv']):.3e} (tol {grad_tol(c['dlv']):.3e})")
    assert maxdiff(out["kld"], c["kld"]) <= kl_tol(c["kld"])
    assert maxdiff(out["raw"], c["raw"]) <= kl_tol(c["raw"])
    got_gate = device_gate(c, out)
    if got_gate is not None:
        assert torch.equal(got_gate, c["gate"])
    if mode == 3:
        assert maxdiff(out["kdim"][:Z], c["K"]) <= kl_tol(c["K"])
        assert maxdiff(out["kld"].mean(), torch.where(c["K"] > c["lam"], c["K"], torch.tensor(c["lam"], dtype=torch.float64)).sum()) \
            <= kl_tol(c["kld"])
        assert bool((out["kdim"][Z:] == POISON).all()) and bool((out["gate_dim"][Z:] == POISON).all())
        assert bool((out["acc"][:, Z:] == POISON).all())
    assert maxdiff(dm, c["dmu"]) <= grad_tol(c["dmu"])
    assert maxdiff(dl, c["dlv"]) <= grad_tol(c["dlv"])
    assert bool((out["dmulv"][:, :, 2 * Z:] == POISON).all())
    if has_pm:
        print(f"  dpm err {maxdiff(out['dpm'][:, :, :Z], c['dpm']):.3e} (tol {grad_tol(c['dpm']):.3e})")
        assert maxdiff(out["dpm"][:, :, :Z], c["dpm"]) <= grad_tol(c["dpm"])
        assert bool((out["dpm"][:, :, Z:] == POISON).all())
    # without a reparameterisation gradient nothing is left where the gate is closed: exactly 0
    zero = run_kernels(c, c["lam"], zero_dz=True)
    closed = ~fr.gate_full(c["gate"], (T_K, B, Z))
    assert bool(closed.any())
    assert bool((zero["dmulv"][:, :, :Z].cpu()[closed] == 0).all()) and bool((zero["dmulv"][:, :, Z:2 * Z].cpu()[closed] == 0).all())
    if has_pm:
        assert bool((zero["dpm"][:, :, :Z].cpu()[closed] == 0).all())
    live = (~closed) & (c["w"] > 0).unsqueeze(-1) & (c["gk"] != 0).view(1, B, 1)
    assert bool((zero["dmulv"][:, :, :Z].cpu()[live] != 0).all())              # (and the open ones did get their KL gradient)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("B,Z,nslab,kmode,has_pm", [KSHAPES[1], KSHAPES[4]])
def test_kernels_with_lambda_zero_are_the_plain_kernels(B, Z, nslab, kmode, has_pm, mode):
    c = kcase(B, Z, nslab, kmode, has_pm, mode)
    a, b = run_kernels(c, 0.0), run_kernels(c, 0.0, plain=True)
    for name in ("mu", "lv", "z", "kld", "dmulv", "dpm"):
        assert torch.equal(bits(a[name]), bits(b[name])), name
    assert bool((a["raw"] == 0).all()) and bool(torch.isnan(a["gate_step"]).all())      # nothing of the struct is written


@pytest.mark.parametrize("B,Z,nslab,kmode,has_pm", KSHAPES)
def test_plain_kernels_match_float64(B, Z, nslab, kmode, has_pm):
    """ssc_latent_fwd / ssc_latent_bwd against the reference with every gate open: the raw KL and its whole gradient."""
    c = kcase(B, Z, nslab, kmode, has_pm, 1)
    out = run_kernels(c, 0.0, plain=True)
    for name in ("mu", "lv", "z"):
        assert bool((out[name][:, :, Z:] == POISON).all()), name
        assert maxdiff(out[name][:, :, :Z], c[{"mu": "m", "lv": "l", "z": "z"}[name]]) <= 1e-5
    every = torch.ones(T_K, B, Z, dtype=torch.bool)
    dmu_k, dlv_k, dpm_k = fr.dlatent(c["m"], c["l"], c["prior_mean"], c["prior_var"], kmode, c["w"], c["gk"], every)
    dzs = c["dz"].double().sum(1)[..., :Z]
    want_dmu, want_dlv = dzs + dmu_k, dzs * c["eps"].double() * 0.5 * (0.5 * c["l"]).exp() + dlv_k
    dm, dl = out["dmulv"][:, :, :Z].cpu(), out["dmulv"][:, :, Z:2 * Z].cpu()
    print(f"B={B} Z={Z} nslab={nslab} kld_mode={kmode} plain: kld err {maxdiff(out['kld'], c['raw']):.3e} (tol {kl_tol(c['raw']):.3e}), "
          f"dmu err {maxdiff(dm, want_dmu):.3e} (tol {grad_tol(want_dmu):.3e}), dlv err {maxdiff(dl, want_dlv):.3e} "
          f"(tol {grad_tol(want_dlv):.3e})")
    assert maxdiff(out["kld"], c["raw"]) <= kl_tol(c["raw"])
    assert maxdiff(dm, want_dmu) <= grad_tol(want_dmu)
    assert maxdiff(dl, want_dlv) <= grad_tol(want_dlv)
    assert bool((out["dmulv"][:, :, 2 * Z:] == POISON).all())
    if has_pm:
        print(f"  dpm err {maxdiff(out['dpm'][:, :, :Z], dpm_k):.3e} (tol {grad_tol(dpm_k):.3e})")
        assert maxdiff(out["dpm"][:, :, :Z], dpm_k) <= grad_tol(dpm_k)
        assert bool((out["dpm"][:, :, Z:] == POISON).all())
    assert bool((out["raw"] == 0).all()) and bool(torch.isnan(out["gate_step"]).all())  # (the plain entries take no struct)


# ---- 2. train step ----------------------------------------------------------------------------------------------------------
# the fixtures of tests/test_train_gpu.py: two of test_train_matches_oracle_medium (SENTIMENT_VAE 0 and 1) and the one of
# test_train_sv2_matches_oracle_medium
MEDIUM = {0: (5, 10, dict(V=777, E=100, H=130, A=70, F=260, Z=30, L=9), 5, 17),
          1: (6, 7, dict(V=451, E=300, H=64, A=48, F=128, Z=16, L=6), 5, 17),
          2: (24, 9, dict(V=600, E=128, H=192, A=96, F=256, Z=150, L=6), 6, 23)}
# (weights, biases) of fc_mean / fc_log_var are multiplied by the first pair at which the reference's values leave the margin the
# floor needs (module docstring); with small weights and large biases the elements of a dimension gather around its own value
SCALES = [(1.0, 1.0), (4.0, 4.0), (0.05, 8.0), (0.02, 16.0), (0.01, 32.0)]
TRAIN_CASES = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 3)]


def _fixture(sv):
    B, R, dims, pseed, iseed = MEDIUM[sv]
    kw = dict(prior_std=0.8) if sv == 2 else dict(senti_prior_multip=0.5)
    cfg = oracle.OracleConfig(vocab_size=dims["V"], image_feature_size=dims["F"], embedding_size=dims["E"], hidden_size=dims["H"],
                              attention_projection_size=dims["A"], z_space=dims["Z"], max_caption_length=dims["L"], sentiment_vae=sv, **kw)
    params = oracle.init_params(cfg, seed=pseed)
    g = torch.Generator().manual_seed(iseed)
    L_, T = dims["L"], dims["L"] + 1
    feats = torch.randn(B, R, dims["F"], generator=g)
    feats[0, R - 3:] = 0
    obj = None
    if sv == 2:
        obj = torch.randn(B, R, 150, generator=g) * 0.5
        obj[0, R - 3:] = 0
        obj[3, 2] = 0
    caps = torch.zeros(B, L_, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(3, L_ + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(2, dims["V"], (n,), generator=g)
    if sv == 2:
        caps[1, 1] = 0
    senti = None if sv == 2 else torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(T, B, dims["Z"], generator=g)
    return cfg, params, feats, caps, senti, eps, obj


def _oracle_latents(cfg, p, feats, caps, senti, eps, obj):
    out = oracle.train_forward(p, cfg, feats, caps, senti, eps, return_steps=True, obj_atts=obj)
    stack = lambda key: torch.stack([s[key] for s in out["steps"]], 0)
    w = (out["tokens"][:, 1:] != cfg.pad_index).t().double()
    k = fr.k_elem(stack("mean"), stack("log_var"), stack("prior_mean"), cfg.prior_std ** 2, 0 if cfg.sentiment_vae == 0 else 1)
    return out, k, w


@functools.lru_cache(maxsize=None)
def medium(sv, mode):
    """The fixture with its fc parameters scaled (SCALES), the floor, and the oracle's floored objective differentiated by autograd
    through oracle.train_forward and freebitsref: mean(loss) + mean(kld_floored) / kld_weight."""
    cfg, params, feats, caps, senti, eps, obj = _fixture(sv)
    for ws, bs in SCALES:
        scaled = dict(params)
        for n in ("fc_mean", "fc_log_var"):
            scaled[P_CELL + n + ".weight"] = params[P_CELL + n + ".weight"] * ws
            scaled[P_CELL + n + ".bias"] = params[P_CELL + n + ".bias"] * bs
        p = {k: v.clone().requires_grad_(True) for k, v in scaled.items()}
        out, k, w = _oracle_latents(cfg, p, feats, caps, senti, eps, obj)
        select = None if mode == 3 else w.bool()
        try:
            lam, kld, gate, K = floor_for(k, w, mode, select)
        except AssertionError:
            continue
        break
    else:
        raise AssertionError(f"no scale of fc_mean / fc_log_var leaves the floor its margin (SENTIMENT_VAE {sv}, mode {mode})")
    assert maxdiff(fr.raw(k, w), out["kld"]) <= kl_tol(out["kld"])             # (freebitsref at no floor is the oracle's kld)
    (out["loss"].double().mean() + kld.mean() / cfg.kld_weight).backward()
    grads = {n: v.grad.clone() for n, v in p.items()}
    return dict(cfg=cfg, params=scaled, feats=feats, caps=caps, senti=senti, eps=eps, obj=obj, lam=lam, mode=mode, kld=kld.detach(),
                raw=out["kld"].detach(), loss=out["loss"].detach(), gate=gate, K=K, w=w, grads=grads, B=feats.size(0), select=select)


def inputs(m):
    return (dev(m["feats"]), dev(m["caps"]), dev(m["senti"]) if m["senti"] is not None else None, dev(m["eps"]),
            dev(m["obj"]) if m["obj"] is not None else None)


def upstream(m):
    B = m["B"]
    return torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * m["cfg"].kld_weight), device="cuda")


def grads_of(eng):
    return {k: v.clone() for k, v in eng.grad_dict().items()}


@pytest.mark.parametrize("sv,mode", TRAIN_CASES)
def test_train_step_matches_oracle_with_floored_kl(sv, mode):
    m = medium(sv, mode)
    eng = engine_from(m["cfg"], m["params"])
    args, name = inputs(m), MODE_NAME[mode]
    loss_off, kld_off = (t.clone() for t in eng.forward(*args))
    loss, kld = eng.forward(*args, free_bits=m["lam"], free_bits_mode=name)
    print(f"SENTIMENT_VAE {sv} mode {name} lam {m['lam']:.4g}: kld err {maxdiff(kld, m['kld']):.3e} (tol {kl_tol(m['kld']):.3e}), "
          f"raw err {maxdiff(eng.kld_raw(), m['raw']):.3e}")
    assert torch.equal(bits(loss), bits(loss_off))                              # z and the cross-entropy do not depend on the floor
    assert torch.equal(bits(eng.kld_raw()), bits(kld_off))                      # the raw KL is the KL of the forward without it
    assert maxdiff(kld, m["kld"]) <= kl_tol(m["kld"])
    assert maxdiff(kld, kld_off) > 10 * kl_tol(m["kld"])                        # (the floor did move the value)
    if mode == 2:
        sel = m["select"]
        assert torch.equal((eng.free_bits_view("gate_step").cpu() != 0)[sel], m["gate"][sel])
    if mode == 3:
        assert torch.equal(eng.free_bits_view("gate_dim").cpu() != 0, m["gate"])
        assert maxdiff(eng.free_bits_view("kdim"), m["K"]) <= kl_tol(m["K"])
    gl, gk = upstream(m)
    eng.backward(gl, gk)
    got = grads_of(eng)
    for k, v in m["grads"].items():
        if k in eng.frozen_names:
            continue
        print(f"  {k}: err {maxdiff(got[k], v):.3e} tol {grad_tol(v):.3e}")
        assert maxdiff(got[k], v) <= grad_tol(v), (k, maxdiff(got[k], v), grad_tol(v))
    # the phased backward reads the same cfg and the same gates: the same gradients, bit for bit
    eng.forward(*args, free_bits=m["lam"], free_bits_mode=name)
    eng.backward_phased(gl, gk, (16, 32, 64, 8, 4, 128))
    for k, v in eng.grad_dict().items():
        assert k in eng.frozen_names or torch.equal(bits(v), bits(got[k])), k


# ---- 3. off and saturated; 4. determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_zero_floor_is_the_step_without_the_arguments(mode):
    m = medium(1, mode)
    eng = engine_from(m["cfg"], m["params"])
    args = inputs(m)
    gl, gk = upstream(m)
    a = [t.clone() for t in eng.forward(*args)]
    eng.backward(gl, gk)
    ga = grads_of(eng)
    b = [t.clone() for t in eng.forward(*args, free_bits=0.0, free_bits_mode=MODE_NAME[mode])]
    assert eng.kld_raw() is not None and torch.equal(bits(eng.kld_raw()), bits(b[1]))
    eng.backward(gl, gk)
    gb = grads_of(eng)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    for k in ga:
        assert torch.equal(bits(ga[k]), bits(gb[k])), k
    # ... and the fused step with beta 1 and no floor is the fused step of before
    e1, e2 = engine_from(m["cfg"], m["params"]), engine_from(m["cfg"], m["params"])
    step = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=0.5)
    e1.train_step(*args[:4], obj_atts=args[4], **step)
    e2.train_step(*args[:4], obj_atts=args[4], kl_beta=1.0, free_bits=0.0, free_bits_mode=MODE_NAME[mode], **step)
    assert torch.equal(bits(e1.params.flat), bits(e2.params.flat))


@pytest.mark.parametrize("sv,mode", [(0, 1), (1, 2), (2, 3)])
def test_floor_above_every_value_leaves_no_kl_gradient(sv, mode):
    m = medium(sv, mode)
    eng = engine_from(m["cfg"], m["params"])
    args = inputs(m)
    gl, gk = upstream(m)
    eng.forward(*args)
    eng.backward(gl, torch.zeros_like(gk))
    want = grads_of(eng)
    loss, kld = eng.forward(*args, free_bits=1e6, free_bits_mode=MODE_NAME[mode])
    eng.backward(gl, gk)
    got = grads_of(eng)
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    Z, n = m["cfg"].z_space, m["w"].sum(0)
    per_row = {1: n * Z, 2: n, 3: torch.full_like(n, Z)}[mode] * 1e6          # every term at the floor
    assert maxdiff(kld, per_row) <= kl_tol(per_row)


def test_beta_zero_is_legal_and_scales_the_kl_gradient():
    m = medium(1, 3)
    args = inputs(m)
    step = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=1e9)
    a, b = engine_from(m["cfg"], m["params"]), engine_from(m["cfg"], m["params"])
    a.train_step(*args[:4], kl_beta=0.0, **step)
    gl, _ = upstream(m)
    b.forward(*args)
    b.backward_update(gl, torch.zeros_like(gl), **{k: v for k, v in step.items() if k != "kld_weight"})
    assert torch.equal(bits(a.params.flat), bits(b.params.flat))
    gk_buf = a._upstream[1]
    a.train_step(*args[:4], kl_beta=0.25, **step)
    assert a._upstream[1] is gk_buf and maxdiff(gk_buf, torch.full((m["B"],), 0.25 / (m["B"] * 750.0))) <= 1e-12   # refilled in place
    a.train_step(*args[:4], **step)
    assert torch.equal(bits(gk_buf), bits(torch.full((m["B"],), 1.0 / (m["B"] * 750.0))))
    with pytest.raises(ValueError, match="kl_beta"):
        a.train_step(*args[:4], kl_beta=-0.1, **step)


def test_two_dim_mode_steps_are_bit_equal():
    m = medium(2, 3)
    args = inputs(m)
    gl, gk = upstream(m)
    res = []
    for _ in range(2):
        eng = engine_from(m["cfg"], m["params"])
        loss, kld = eng.forward(*args, free_bits=m["lam"], free_bits_mode="dim")
        eng.backward(gl, gk)
        res.append([loss.clone(), kld.clone(), eng.kld_raw().clone(), eng.free_bits_view("gate_dim").clone(),
                    eng.free_bits_view("kdim").clone(), eng.grads.flat.clone()])
    for x, y in zip(*res):
        assert torch.equal(bits(x), bits(y))


# ---- 5. phased (overlapped) backward on one rank ----------------------------------------------------------------------------
def _rccl_worker(port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    m = medium(1, 3)
    eng = engine_from(m["cfg"], m["params"])
    eng.dp_force = True
    args = inputs(m)
    gl, gk = upstream(m)
    eng.forward(*args, free_bits=m["lam"], free_bits_mode="dim")
    eng.backward(gl, gk)
    plain = eng.grads.flat.clone()
    eng.grads.flat.zero_()
    eng.forward(*args, free_bits=m["lam"], free_bits_mode="dim")
    world = eng.backward_overlapped(gl, gk)
    torch.cuda.synchronize()
    same = torch.equal(bits(eng.grads.flat), bits(plain))
    eng.forward(*args)
    eng.backward(gl, gk)
    moved = not torch.equal(bits(eng.grads.flat), bits(plain))
    ret.put((world, same, moved))
    dist.destroy_process_group()


def test_overlapped_backward_honours_the_floor_on_one_rank():
    from test_dp_gpu import _join_then_get
    ctx = mp.get_context("spawn")
    ret = ctx.SimpleQueue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = ctx.Process(target=_rccl_worker, args=(port, ret))
    p.start()
    world, same, moved = _join_then_get([p], ret)
    assert world == 1 and same and moved


# ---- 6. module and neighbours -----------------------------------------------------------------------------------------------
def build_model(cfg, params, free_bits, mode, beam=5):
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    mod = UpDownCaptioner(Vocabulary.synthetic(cfg.vocab_size), cfg.image_feature_size, cfg.embedding_size, cfg.hidden_size,
                          cfg.attention_projection_size, max_caption_length=cfg.max_caption_length, beam_size=beam,
                          use_cbs=cfg.tied, z_space=cfg.z_space, prior_std=cfg.prior_std, simple_vae=cfg.simple_vae,
                          latent_embedding="glove", sentiment_vae=cfg.sentiment_vae, senti_prior_multip=cfg.senti_prior_multip,
                          device=torch.device("cuda"), free_bits=free_bits, free_bits_mode=mode)
    mod.load_state_dict(dict(params))
    return mod.cuda()


def test_module_training_forward_returns_the_floored_kl_and_its_gradients():
    m = medium(0, 3)                                                            # (E = 100: no GloVe table to load)
    eng = engine_from(m["cfg"], m["params"])
    feats, caps, senti, eps, _ = inputs(m)
    loss, kld = eng.forward(feats, caps, senti, eps, free_bits=m["lam"], free_bits_mode="dim")
    mod = build_model(m["cfg"], m["params"], m["lam"], "dim")
    mod.train()
    mod._eps_override = m["eps"]
    out = mod(feats, None, None, caps, senti)
    assert torch.equal(bits(out["loss"]), bits(loss)) and torch.equal(bits(out["kld"]), bits(kld))
    assert maxdiff(mod._engine().kld_raw(), m["raw"]) <= kl_tol(m["raw"])
    (out["loss"].mean() + out["kld"].mean() / m["cfg"].kld_weight).backward()
    named = dict(mod.named_parameters())
    for k, v in m["grads"].items():
        assert maxdiff(named[k].grad, v) <= grad_tol(v), k


def test_posterior_and_likelihood_scores_never_floor():
    m = medium(0, 3)                                                            # (E = 100: no GloVe table to load)
    feats, caps, senti, eps, _ = inputs(m)
    res = []
    for fb in (0.0, m["lam"]):
        mod = build_model(m["cfg"], m["params"], fb, "dim")
        mod.train()
        mod._eps_override = m["eps"]
        out = mod(feats, None, None, caps, senti)                                # leaves the engine's cfg at this captioner's floor
        post = mod._engine().posterior_forward(feats, caps, senti, eps)
        torch.manual_seed(3)                                                     # (both score calls draw their noise from it)
        sc = mod.score_captions(feats, caps, senti, n_samples=2)
        ps = mod.posterior_score_captions(feats, caps, senti, n_samples=1, eps=eps)
        res.append((out["kld"].detach().clone(), [t.clone() for t in post], sc, ps))
    (k0, p0, s0, q0), (k1, p1, s1, q1) = res
    assert not torch.equal(k0, k1)                                              # (the training forwards did differ)
    for x, y in zip(p0, p1):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(bits(p1[1]), bits(k0))                                   # its kld is the raw KL
    assert torch.equal(bits(s0.log_probs), bits(s1.log_probs)) and torch.equal(bits(s0.marginal), bits(s1.marginal))
    for f in ("log_w", "kld", "elbo"):
        assert torch.equal(bits(getattr(q0, f)), bits(getattr(q1, f))), f
    assert torch.equal(q0.kl_dim, q1.kl_dim)


def test_self_critical_step_never_floors():
    """A captioner built with a floor - and fresh from a floored training forward - takes the self-critical step of one built
    without, bit for bit (the smallest fixture of tests/test_scst_gpu.py)."""
    from test_scst_gpu import HP, N_, P_, SEED, setup
    s = setup(1, 0)
    cfg = s["cfg"]
    res = []
    for fb in (0.0, 0.05):
        mod = build_model(cfg, s["params"], fb, "element", beam=1)
        mod.train()
        ro = s["ro"]
        mod._eps_override = ro.train_eps
        out = mod(ro.feats, None, None, ro.caps, ro.sentiment.view(-1, 1))
        mod._eps_override = None
        loss, kld, stats = mod.scst_step(s["feats"], [0, 1, 2], s["senti"].view(P_, 1), references=s["references"], seed=SEED,
                                         n_samples=N_, decoder_frozen=False, **HP)
        res.append((out["kld"].detach().clone(), loss.clone(), kld.clone(), stats.clone(), mod._eng.params.flat.clone()))
    a, b = res
    assert not torch.equal(a[0], b[0])                                          # (the training forwards did differ)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x.cpu().contiguous().view(torch.uint8), y.cpu().contiguous().view(torch.uint8))


# ---- 7. script --------------------------------------------------------------------------------------------------------------
def _train(tmp_path, name, extra, stop=4):
    from test_scripts_gpu import YAML
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    out = tmp_path / name
    args = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--fused-optimizer", "--zero-eps", "--serialization-dir", str(out), "--stop-after", str(stop),
            "--checkpoint-every", "2"] + extra
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out, [json.loads(x) for x in open(out / "scalars.jsonl")]


def test_train_script_anneals_floors_and_resumes(tmp_path):
    keys = ["--config-override", "OPTIM.KL_ANNEAL", "linear", "OPTIM.KL_ANNEAL_ITERS", "4", "OPTIM.FREE_BITS", "0.05",
            "OPTIM.FREE_BITS_MODE", "dim"]
    out, log = _train(tmp_path, "fb", keys)
    assert [rec["iteration"] for rec in log] == [1, 2, 3, 4]
    assert [rec["kl_beta"] for rec in log] == [0.0, 0.25, 0.5, 0.75]          # beta of iteration i is kl_beta(i - 1, "linear", 4)
    for rec in log:
        assert rec["kld_free"] >= rec["2kld_loss"] > 0 and 0 <= rec["active_dims"] <= 16
        want = rec["1reconstr_loss"] + rec["kl_beta"] * rec["kld_free"] / 750
        assert abs(rec["3loss"] - want) <= 1e-5 * abs(want)
    text = open(out / "config.yml").read()
    assert "KL_ANNEAL: linear" in text and "FREE_BITS: 0.05" in text
    plain_out, plain = _train(tmp_path, "plain", [])
    assert all(rec["kl_beta"] == 1.0 and "kld_free" not in rec and "active_dims" not in rec for rec in plain)
    # the first step's raw KL is the plain run's KL (same parameters, same batch, zero noise); the parameters then part ways
    assert abs(log[0]["2kld_loss"] - plain[0]["2kld_loss"]) <= 1e-6 * abs(plain[0]["2kld_loss"])
    a = torch.load(out / "checkpoint_4.pth", map_location="cpu", weights_only=True)["model"]
    b = torch.load(plain_out / "checkpoint_4.pth", map_location="cpu", weights_only=True)["model"]
    assert any(not torch.equal(a[k], b[k]) for k in a)
    # a run resumed at the checkpoint of iteration 2 continues the schedule at iteration 3
    res_out, res = _train(tmp_path, "resumed", keys + ["--start-from-checkpoint", str(out / "checkpoint_2.pth")])
    assert [rec["iteration"] for rec in res] == [3, 4] and [rec["kl_beta"] for rec in res] == [0.5, 0.75]
    c = torch.load(res_out / "checkpoint_4.pth", map_location="cpu", weights_only=True)["model"]
    for k in a:
        assert torch.equal(a[k], c[k]), k
