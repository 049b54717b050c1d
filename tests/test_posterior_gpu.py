"""GPU: posterior scoring of given captions - ssc_posterior_rows against its float64 restatement, TrainEngine.posterior_forward /
posterior_score_captions against the float64 oracle (tests/posteriorref.py), the decode kernels against the train kernels at the
same z, non-interference with a training step in flight, chunking, the module method and scripts/train.py --val-posterior-samples."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import posteriorref as PR
from gpuutil import engine_from
from ssc_runtime import lib as L
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.inference import plan_posterior_chunks, posterior_score_captions, score_captions
from ssc_runtime.vocab import Vocabulary
from test_score_gpu import YAML, base_params
from var_updown.models import UpDownCaptioner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def r4(x):
    return (x + 3) // 4 * 4


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def padded(x, ld, dead):
    """(T, B, Z) -> device (T * B, ld) with NaN in the pad columns and in every row of `dead` (T, B)."""
    T, B, Z = x.shape
    out = torch.full((T * B, ld), float("nan"))
    out[:, :Z] = x.reshape(T * B, Z)
    out[dead.reshape(-1)] = float("nan")
    return out.cuda()


def kernel_case(T, B, Z, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(T, B, Z, generator=g)
    lv = torch.randn(T, B, Z, generator=g) * 1.5 - 1
    lv.view(-1)[:: 7] = -30.0
    lv.view(-1)[3:: 11] = 5.0
    eps = torch.randn(T, B, Z, generator=g)
    z = eps * torch.exp(lv / 2) + mu                       # formed in float32, as the forward forms it
    pm = torch.randn(T, B, Z, generator=g) * 0.5
    sent = torch.randint(-1, 2, (B,), generator=g).float()
    n_live = torch.randint(1, T + 1, (B,), generator=g)     # w = 1 on a prefix of the steps, as the train forward leaves it
    n_live[B // 2] = 0                                      # one row with no live step
    n_live[0] = T
    w = (torch.arange(T).view(T, 1) < n_live.view(1, B)).float()
    return mu, lv, z, eps, pm, sent, w


def run_rows(lib, mu, lv, z, eps, w, pm, sent, pm_scale, kld_mode, pv, optional=True):
    T, B, Z = mu.shape
    ldz, lde, ldp, ld = r4(Z) + 4, Z + 1, r4(Z) + 8, Z + 3
    dead = w == 0
    bufs = [padded(x, l, dead) for x, l in ((mu, ldz), (lv, ldz), (z, ldz), (eps, lde))]
    pmd = padded(pm, ldp, dead) if pm is not None else None
    wd = w.reshape(-1).cuda()
    sd = sent.cuda() if sent is not None else None
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out = {"log_ratio": nan(B), "kl": nan(B)}
    if optional:
        out.update(kl_dim=nan(B, ld), step_kl=nan(T, B), step_ratio=nan(T, B))
    d = L.PosteriorRowsDesc()
    d.T, d.B, d.Z, d.ldz, d.ldeps, d.ld = T, B, Z, ldz, lde, ld
    d.mu, d.lv, d.z, d.eps = (b.data_ptr() for b in bufs)
    d.w = wd.data_ptr()
    if pmd is not None:
        d.pm, d.ldpm = pmd.data_ptr(), ldp
    d.kld_mode, d.pm_scale, d.prior_var = kld_mode, pm_scale, pv
    d.sent = sd.data_ptr() if sd is not None else None
    for k, v in out.items():
        setattr(d, k, v.data_ptr())
    lib.ssc_posterior_rows(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    if optional:
        assert torch.isnan(res["kl_dim"][:, Z:]).all()   # (pad columns of the output are not written)
        res["kl_dim"] = res["kl_dim"][:, :Z]
    return res, d, (bufs, pmd, wd, sd, out)


@pytest.mark.parametrize("prior", ["mode0", "mode1", "pm"])
@pytest.mark.parametrize("T,B,Z", [(3, 5, 1), (3, 5, 8), (3, 5, 65), (3, 5, 150), (21, 150, 128)])
def test_posterior_rows_against_the_restatement(T, B, Z, prior):
    """The same float32 inputs through the kernel and through posteriorref.posterior_rows: every output within 1e-5 + 5e-6 S, S the
    sum of the absolute parts of the terms behind it (each fp32 term a few ulp off, plus at most T ceil(Z / 64) + 6 <= 69
    roundings of a running sum, times 6e-8); ldz = round4(Z) + 4 with NaN in the pad columns and in every (t, b) with w = 0; dead
    rows and steps exactly 0; a second run, and one without the optional outputs, the same bits."""
    lib = L.load()
    pv = 0.49
    mu, lv, z, eps, pm, sent, w = kernel_case(T, B, Z, seed=100 * Z + T)
    if prior == "mode0":
        kw = dict(pm=None, sent=None, pm_scale=0.0, kld_mode=0)
        ref_pm = None
    elif prior == "mode1":
        kw = dict(pm=None, sent=sent, pm_scale=0.5, kld_mode=1)
        ref_pm = 0.5 * sent
    else:
        kw = dict(pm=pm, sent=None, pm_scale=0.0, kld_mode=2)
        ref_pm = pm
    want = PR.posterior_rows(mu, lv, z, eps, w, ref_pm, kw["kld_mode"], np.float32(pv))
    got, _, _ = run_rows(lib, mu, lv, z, eps, w, kw["pm"], kw["sent"], kw["pm_scale"], kw["kld_mode"], pv)
    for name in ("log_ratio", "kl", "kl_dim", "step_kl", "step_ratio"):
        err = (got[name].double() - want[name]).abs()
        bound = 1e-5 + 5e-6 * want["abs_" + name]
        print(f"{prior} T {T} B {B} Z {Z} {name}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, "
              f"|ref| up to {float(want[name].abs().max()):.1f}")
        assert (err <= bound).all(), name
    dead_row = B // 2
    assert float(got["log_ratio"][dead_row]) == 0 and float(got["kl"][dead_row]) == 0 and (got["kl_dim"][dead_row] == 0).all()
    assert (got["step_kl"][w == 0] == 0).all() and (got["step_ratio"][w == 0] == 0).all()
    again, _, _ = run_rows(lib, mu, lv, z, eps, w, kw["pm"], kw["sent"], kw["pm_scale"], kw["kld_mode"], pv)
    assert all(torch.equal(got[k], again[k]) for k in got)
    bare, _, _ = run_rows(lib, mu, lv, z, eps, w, kw["pm"], kw["sent"], kw["pm_scale"], kw["kld_mode"], pv, optional=False)
    assert torch.equal(bare["log_ratio"], got["log_ratio"]) and torch.equal(bare["kl"], got["kl"])


def test_posterior_rows_bad_arguments():
    """Every bad-argument case returns SSC_EINVAL (-1) through _raw_, with device pointers in place."""
    lib = L.load()
    mu, lv, z, eps, pm, sent, w = kernel_case(3, 5, 8, seed=1)
    _, d, keep = run_rows(lib, mu, lv, z, eps, w, pm, None, 0.0, 1, 0.49)
    assert lib._raw_ssc_posterior_rows(C.byref(d), L.stream_ptr()) == 0
    some = d.mu
    for bad in (dict(mu=None), dict(lv=None), dict(z=None), dict(eps=None), dict(w=None), dict(log_ratio=None), dict(kl=None),
                dict(T=0), dict(B=0), dict(Z=0), dict(T=-2), dict(ldz=7), dict(ldeps=7), dict(ldpm=7), dict(ld=7), dict(prior_var=0.0),
                dict(prior_var=-0.49), dict(kld_mode=-1), dict(kld_mode=3), dict(kld_mode=2, pm=None)):
        saved = {k: getattr(d, k) for k in bad}
        for k, v in bad.items():
            setattr(d, k, v)
        assert lib._raw_ssc_posterior_rows(C.byref(d), L.stream_ptr()) == -1, bad
        for k, v in saved.items():
            setattr(d, k, v)
    assert d.mu == some and lib._raw_ssc_posterior_rows(C.byref(d), L.stream_ptr()) == 0
    torch.cuda.synchronize()


# ---- the full path -------------------------------------------------------------------------------------------------------------------
def full_bound(ref):
    """The bound tests/test_train_gpu.py holds for loss and kld."""
    return 1e-4 + 1e-5 * float(torch.as_tensor(ref).abs().max())


@functools.lru_cache(maxsize=None)
def mode0_params():
    cfg = oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32, attention_projection_size=16,
                              z_space=8, max_caption_length=9, sentiment_vae=0, prior_std=0.8, beam_size=1)
    return cfg, oracle.init_params(cfg, seed=5)


def params_of(kind):
    return mode0_params() if kind == "mode0" else base_params(kind)


@functools.lru_cache(maxsize=None)
def engine_of(kind):
    cfg, params = params_of(kind)
    return engine_from(cfg, params)


@functools.lru_cache(maxsize=None)
def path_case(kind):
    """nimg 2, C 2, K 3, L 6, R 5: one short caption, one of full length, one in between, slot (1, 0) absent; explicit noise over
    all slots.  -> the inputs and the float64 oracle's result over the rows of the present captions (computed once, read only)."""
    cfg, params = params_of(kind)
    nimg, Cc, K, L0, R = 2, 2, 3, 6, 5
    g = torch.Generator().manual_seed(41)
    caps = torch.zeros(nimg, Cc, L0, dtype=torch.int64)
    for (i, c), n in {(0, 0): 2, (0, 1): 6, (1, 1): 4}.items():
        caps[i, c, :n] = torch.randint(2, cfg.vocab_size, (n,), generator=g)
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g)
    senti = torch.randint(-1, 2, (nimg,), generator=g).float() if cfg.sentiment_vae == 1 else None
    obj = torch.randn(nimg, R, cfg.z_space, generator=g) * 0.3 if cfg.sentiment_vae == 2 else None
    eps = torch.randn(L0 + 1, nimg * Cc * K, cfg.z_space, generator=g)
    slots = [0, 1, 3]
    rows = torch.tensor([s * K + k for s in slots for k in range(K)])
    img = rows // (Cc * K)
    want = PR.posterior_forward(params, cfg, feats[img], caps.view(nimg * Cc, L0)[rows // K], senti[img].view(-1, 1) if senti is not None
                                else None, eps[:, rows], obj[img] if obj is not None else None)
    return dict(cfg=cfg, caps=caps, feats=feats, senti=senti, obj=obj, eps=eps, K=K, slots=slots, want=want)


def score(kind, **kw):
    c = path_case(kind)
    dv = lambda x: x.cuda() if x is not None else None
    return posterior_score_captions(engine_of(kind), c["feats"].cuda(), dv(c["senti"]), c["caps"], c["K"], eps=c["eps"].cuda(),
                                    obj_means=dv(c["obj"]), want_steps=True, **kw)


@pytest.mark.parametrize("kind", ["toy", "sv2"])
def test_full_path_against_the_float64_oracle(kind):
    """nll, kld, log_ratio, log_w, elbo, iwae, token_kl within 1e-4 + 1e-5 max|ref| of the float64 oracle (the float32 CPU oracle
    stays within 7e-5 of it at a medium width where |ref| is about 490); kl_dim.sum() against kld.sum() at the same bound; the
    absent slot zeros."""
    c = path_case(kind)
    want, K, slots = c["want"], c["K"], c["slots"]
    s = score(kind)
    nimg, Cc, L0 = c["caps"].shape
    assert s.n_tokens.cpu().tolist() == [[3, 7], [0, 5]] and s.n_steps == 15 * K
    pick = lambda t: t.reshape(nimg * Cc, K, *t.shape[3:])[slots].cpu().double()
    for name, ref in (("nll", want["nll"]), ("kld", want["kld"]), ("log_ratio", want["log_ratio"]), ("log_w", want["log_w"])):
        got = pick(getattr(s, name)).reshape(-1)
        print(f"{kind} {name}: max err {float((got - ref).abs().max()):.3e}, bound {full_bound(ref):.3e}, |ref| up to {float(ref.abs().max()):.1f}")
        assert (got - ref).abs().max() <= full_bound(ref), name
    elbo, iwae, ess = PR.bounds(want["log_w"].view(len(slots), K))
    for name, ref in (("elbo", elbo), ("iwae", iwae)):
        got = getattr(s, name).reshape(-1)[slots].cpu().double()
        print(f"{kind} {name}: max err {float((got - ref).abs().max()):.3e}, bound {full_bound(ref):.3e}")
        assert (got - ref).abs().max() <= full_bound(ref), name
    assert (s.iwae >= s.elbo - 1e-5).all()
    tk = want["step_kl"].t().reshape(len(slots), K, L0 + 1)
    assert (pick(s.token_kl) - tk).abs().max() <= full_bound(tk)
    tr = want["step_ratio"].t().reshape(len(slots), K, L0 + 1)
    assert (pick(s.token_ratio) - tr).abs().max() <= full_bound(tr)
    assert abs(float(s.kl_dim.sum()) - float(want["kld"].sum())) <= full_bound(want["kld"].sum())
    assert (s.kl_dim - want["kl_dim"].sum(0)).abs().max() <= full_bound(want["kl_dim"].sum(0))
    for t in (s.log_w, s.nll, s.log_ratio, s.kld, s.token_kl, s.token_ratio):
        assert (t[1, 0] == 0).all()
    assert float(s.elbo[1, 0]) == float(s.iwae[1, 0]) == float(s.ess[1, 0]) == 0
    summ = s.summary()
    assert summ["n_captions"] == 3 and summ["n_tokens"] == 15 and summ["iwae_nll_per_token"] <= summ["elbo_nll_per_token"] + 1e-6
    assert summ["kl_per_token"] == pytest.approx(float(want["kld"].view(len(slots), K).mean(1).sum()) / 15, abs=1e-4)


@pytest.mark.parametrize("kind", ["mode0", "toy"])
def test_decode_path_against_train_path_at_the_same_z(kind):
    """score_captions fed eps_steps = (z_t - pm) / sqrt(pv) with the z of posterior_forward: its log_probs (the decode cells and
    tables) equal -nll of the train forward (the train cells) within twice the bound of the full-path test."""
    cfg, params = params_of(kind)
    eng = engine_of(kind)
    dec = DecodeEngine(eng.dims, eng.params.c_struct, "cuda")
    nimg, Cc, K, L0, R = 2, 2, 2, 6, 5
    g = torch.Generator().manual_seed(9)
    caps = torch.zeros(nimg, Cc, L0, dtype=torch.int64)
    for k, n in enumerate((3, 6, 1, 5)):
        caps[k // Cc, k % Cc, :n] = torch.randint(2, cfg.vocab_size, (n,), generator=g)
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g).cuda()
    senti = torch.randint(-1, 2, (nimg,), generator=g).float().cuda()
    G = nimg * Cc * K
    img = torch.arange(G, device="cuda") // (Cc * K)
    eps = torch.randn(L0 + 1, G, cfg.z_space, generator=g).cuda()
    nll = eng.posterior_forward(feats[img].contiguous(), caps.view(nimg * Cc, L0).repeat_interleave(K, 0).cuda(), senti[img], eps)[0]
    z = eng.posterior_view("z")
    assert eng.posterior_view("w").sum(0).cpu().tolist() == [float(n) for n in (4, 4, 7, 7, 2, 2, 6, 6)]
    assert (z - (eps * torch.exp(eng.posterior_view(8) / 2) + eng.posterior_view(7))).abs().max() < 1e-5   # (the stored z)
    pm = (eng.dims.pm_scale * senti[img]).view(1, G, 1)
    steps = [((z[t] - pm[0]) / float(np.sqrt(eng.dims.prior_var))).contiguous() for t in range(L0 + 1)]
    got = score_captions(dec, feats, senti, caps, K, cfg.boundary_index, "padded", eps_steps=steps)
    ref = -nll.cpu().double()
    err = (got.log_probs.reshape(-1).cpu().double() - ref).abs().max()
    print(f"{kind}: max |decode log_probs + train nll| {float(err):.3e}, bound {2 * full_bound(ref):.3e}, |ref| up to {float(ref.abs().max()):.1f}")
    assert err <= 2 * full_bound(ref)
    assert got.n_tokens.cpu().tolist() == [[4, 7], [2, 6]]


def test_posterior_forward_does_not_disturb_a_training_step():
    """forward, posterior_forward on other data (another shape), backward: gradients bit-equal to forward, backward; nll() and
    fwd_version unchanged."""
    cfg, _ = params_of("toy")
    eng = engine_of("toy")
    g = torch.Generator().manual_seed(2)
    B, R, Lc = 6, 5, 7
    feats = torch.randn(B, R, cfg.image_feature_size, generator=g).cuda()
    caps = torch.zeros(B, Lc, dtype=torch.int64)
    for b in range(B):
        caps[b, : b + 1] = torch.randint(2, cfg.vocab_size, (b + 1,), generator=g)
    caps = caps.cuda()
    senti = torch.randint(-1, 2, (B,), generator=g).float().cuda()
    eps = torch.randn(Lc + 1, B, cfg.z_space, generator=g).cuda()
    gl, gk = torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1e-3, device="cuda")
    eng.forward(feats, caps, senti, eps, label_smoothing=0.1)
    eng.backward(gl, gk)
    want = eng.grads.flat.clone()
    eng.grads.flat.zero_()
    loss, kld = eng.forward(feats, caps, senti, eps, label_smoothing=0.1)
    nll0, version = eng.nll().clone(), eng.fwd_version
    out = eng.posterior_forward(feats[:4, :3].contiguous() * 2, caps[:4, :5].contiguous(), senti[:4].contiguous(),
                                torch.randn(6, 4, cfg.z_space, generator=g).cuda())
    assert out[0].shape == (4,) and out[4].shape == (4, cfg.z_space) and out[5].shape == (6, 4)
    assert eng.fwd_version == version and torch.equal(eng.nll(), nll0) and float(eng._cfg.label_smoothing) == pytest.approx(0.1)
    eng.backward(gl, gk)
    assert torch.equal(eng.grads.flat, want)
    # with label_smoothing 0 the posterior forward's nll and kld are the training forward's own
    loss0, kld0 = eng.forward(feats, caps, senti, eps)
    p = eng.posterior_forward(feats, caps, senti, eps)
    assert torch.equal(p[0], loss0) and torch.equal(p[1], kld0)


def test_chunking_and_explicit_noise_rows():
    """max_rows = K (one caption per forward, each trimmed to its own length) against the default (one forward) within the bound of
    the full-path test; with an absent slot in the call the rows of eps still map to (image, caption, sample): every present
    caption alone, with its slice of the noise, gives the scores it has in the whole call."""
    c = path_case("toy")
    K = c["K"]
    whole, single = score("toy"), score("toy", max_rows=K)
    assert len(plan_posterior_chunks([2, 6, 0, 4], K, K)) == 3
    for name in ("log_w", "nll", "log_ratio", "kld", "elbo", "iwae", "token_kl"):
        a, b = getattr(whole, name).cpu().double(), getattr(single, name).cpu().double()
        assert (a - b).abs().max() <= full_bound(a), name
    assert (whole.kl_dim - single.kl_dim).abs().max() <= full_bound(whole.kl_dim) and whole.n_steps == single.n_steps
    with pytest.raises(ValueError, match="max_rows"):
        score("toy", max_rows=K - 1)
    eng = engine_of("toy")
    nimg, Cc, L0 = c["caps"].shape
    for slot in c["slots"]:
        i, cc = divmod(slot, Cc)
        one = posterior_score_captions(eng, c["feats"][i: i + 1].cuda(), c["senti"][i: i + 1].cuda(), c["caps"][i: i + 1, cc: cc + 1], K,
                                       eps=c["eps"][:, slot * K: (slot + 1) * K].cuda())
        a, b = one.log_w.view(-1).cpu().double(), whole.log_w[i, cc].cpu().double()
        assert (a - b).abs().max() <= full_bound(b), slot
    bad = c["caps"].clone()
    bad[0, 1, 2] = c["cfg"].vocab_size

    class NoLaunch:
        dims = eng.dims
    with pytest.raises(ValueError, match="outside the vocabulary"):
        posterior_score_captions(NoLaunch(), c["feats"].cuda(), c["senti"].cuda(), bad, K)
    # the default noise: one draw of the global CPU generator, the same seed the same scores
    torch.manual_seed(5)
    a = posterior_score_captions(eng, c["feats"].cuda(), c["senti"].cuda(), c["caps"], K)
    after = torch.rand(1)
    torch.manual_seed(5)
    b = posterior_score_captions(eng, c["feats"].cuda(), c["senti"].cuda(), c["caps"], K)
    torch.manual_seed(5)
    torch.randint(0, 2 ** 62, (1,))
    assert torch.equal(a.log_w, b.log_w) and torch.equal(after, torch.rand(1)) and not torch.equal(a.log_w, whole.log_w)


# ---- the module and the script ---------------------------------------------------------------------------------------------------------
def small_module(seed):
    torch.manual_seed(seed)
    return UpDownCaptioner(Vocabulary.synthetic(120), 64, 40, 48, 32, max_caption_length=8, beam_size=1, z_space=16, sentiment_vae=1,
                           senti_prior_multip=0.5, device=torch.device("cuda")).cuda()


def test_module_method_in_both_modes_and_between_optimizer_steps():
    m = small_module(3).train()
    g = torch.Generator().manual_seed(1)
    B, R, Lc, K = 5, 5, 8, 2
    feats = torch.randn(B, R, 64, generator=g).cuda()
    caps = torch.zeros(B, Lc, dtype=torch.int64)
    for b in range(B):
        caps[b, : b + 2] = torch.randint(2, 120, (b + 2,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float().cuda()
    eps = torch.randn(Lc + 1, B * K, 16, generator=g).cuda()
    before = m.posterior_score_captions(feats, caps, sentiment=senti, n_samples=K, eps=eps)
    assert m.training and before.log_w.shape == (B, 1, K) and before.n_tokens.view(-1).tolist() == [3, 4, 5, 6, 7]
    in_eval = m.eval().posterior_score_captions(feats, caps, sentiment=senti, n_samples=K, eps=eps)
    assert not m.training and torch.equal(in_eval.log_w, before.log_w) and torch.equal(in_eval.kld, before.kld)
    m.train()
    fn = posterior_score_captions(m._engine(), feats, senti.reshape(B), caps.unsqueeze(1), K, eps=eps)
    assert torch.equal(fn.log_w, before.log_w) and torch.equal(fn.kl_dim, before.kl_dim)
    assert m.posterior_score_captions(feats, caps, sentiment=senti).log_w.shape == (B, 1, 1)
    eng = m._engine()
    eng.train_step(feats, caps.cuda(), senti, torch.randn(Lc + 1, B, 16, generator=g).cuda(), lr=0.5)
    after = m.posterior_score_captions(feats, caps, sentiment=senti, n_samples=K, eps=eps)
    fresh = small_module(99)
    fresh.load_state_dict(m.state_dict())
    want = fresh.eval().posterior_score_captions(feats, caps, sentiment=senti, n_samples=K, eps=eps)
    assert (after.log_w - want.log_w).abs().max() < 1e-5
    assert (after.log_w - before.log_w).abs().min() > 0


def test_train_script_posterior_validation_does_not_change_training(tmp_path):
    """scripts/train.py --val-posterior-samples 2: the four scalars in every validation record; the training scalars (all but the
    wall-clock field), the other validation scalars and the final checkpoint are those of the same run without the flag, bit for
    bit."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    g = torch.Generator().manual_seed(5)
    caps = torch.zeros(6, 8, dtype=torch.int64)
    for b in range(6):
        caps[b, : b + 1] = torch.randint(2, 150, (b + 1,), generator=g)
    val = tmp_path / "val.pt"
    torch.save({"image_features": torch.randn(6, 5, 64, generator=g), "caption_tokens": caps,
                "sentiment": torch.randint(-1, 2, (6, 1), generator=g).float()}, val)
    base = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--checkpoint-every", "5", "--val-tensors", str(val), "--val-every", "3"]
    logs = {}
    for name, extra in (("plain", []), ("post", ["--val-posterior-samples", "2"])):
        r = subprocess.run([sys.executable] + base + extra + ["--serialization-dir", str(tmp_path / name)], cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        logs[name] = [json.loads(x) for x in open(tmp_path / name / "scalars.jsonl")]
    new = {"val_elbo_nll_per_token", "val_iwae_nll_per_token", "val_kl_per_token", "val_active_units"}
    vals = [r for r in logs["post"] if "val_nll_per_token" in r]
    assert [r["iteration"] for r in vals] == [3, 5]
    for r in vals:
        assert new <= set(r) and 0 < r["val_iwae_nll_per_token"] <= r["val_elbo_nll_per_token"] + 1e-9
        assert r["val_kl_per_token"] >= 0 and 0 <= r["val_active_units"] <= 16 and isinstance(r["val_active_units"], int)
    assert not any(new & set(r) for r in logs["plain"])
    strip = lambda rows: [{k: v for k, v in r.items() if k != "elapsed_s" and k not in new} for r in rows]
    assert strip(logs["post"]) == strip(logs["plain"]) and len(logs["plain"]) == 7
    a = torch.load(tmp_path / "plain" / "checkpoint_5.pth", weights_only=True)
    b = torch.load(tmp_path / "post" / "checkpoint_5.pth", weights_only=True)
    assert set(a["model"]) == set(b["model"]) and all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    for k, st in a["optimizer"]["state"].items():
        assert torch.equal(st["momentum_buffer"], b["optimizer"]["state"][k]["momentum_buffer"])
