"""CPU: posterior scoring - the float64 definitions (tests/posteriorref.py) against torch.distributions, the properties of the
bounds, the Monte-Carlo KL on a fixed seed, the chunk planner, PosteriorScores.summary on hand-made numbers, the new flag of
scripts/train.py and the argument checks of ssc_posterior_rows that need no GPU."""
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch
from torch.distributions import Normal

import posteriorref as PR
from ssc_runtime import lib as L
from ssc_runtime.inference import PosteriorScores, plan_posterior_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_case(T, B, Z, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(T, B, Z, generator=g, dtype=dtype)
    lv = torch.randn(T, B, Z, generator=g, dtype=dtype) * 1.5 - 1
    eps = torch.randn(T, B, Z, generator=g, dtype=dtype)
    pm = torch.randn(T, B, Z, generator=g, dtype=dtype) * 0.5
    w = (torch.rand(T, B, generator=g) < 0.7).to(dtype)
    return mu, lv, eps * (lv / 2).exp() + mu, eps, w, pm


@pytest.mark.parametrize("kld_mode", [0, 1, 2])
def test_reference_agrees_with_normal_log_prob(kld_mode):
    """log_ratio / step_ratio = sum of Normal(pm, sqrt(pv)).log_prob(z) - Normal(mu, exp(lv / 2)).log_prob(z) over the live steps to
    1e-10 in float64; the KL of modes 1 and 2 is torch's kl_divergence up to the 1e-5 in its denominator, mode 0 is against N(0, 1)."""
    T, B, Z, pv = 4, 5, 7, 0.49
    mu, lv, z, eps, w, pm = random_case(T, B, Z, seed=kld_mode)
    out = PR.posterior_rows(mu, lv, z, eps, w, pm, kld_mode, pv)
    diff = (Normal(pm, math.sqrt(pv)).log_prob(z) - Normal(mu, (lv / 2).exp()).log_prob(z)) * w.unsqueeze(-1)
    assert (out["step_ratio"] - diff.sum(-1)).abs().max() < 1e-10
    assert (out["log_ratio"] - diff.sum((0, 2))).abs().max() < 1e-10
    q = Normal(mu, (lv / 2).exp())
    if kld_mode == 0:
        kl = torch.distributions.kl_divergence(q, Normal(torch.zeros_like(mu), torch.ones_like(mu)))
        assert (out["kl_dim"] - (kl * w.unsqueeze(-1)).sum(0)).abs().max() < 1e-10
    else:
        kl = torch.distributions.kl_divergence(q, Normal(pm, math.sqrt(pv)))
        assert (out["kl_dim"] - (kl * w.unsqueeze(-1)).sum(0)).abs().max() < 1e-3   # (pv + 1e-5 in the training formula)
        exact = PR.kl_closed_form(mu, lv, pm, pv)
        assert (exact - kl.sum(-1)).abs().max() < 1e-10
    assert (out["kl"] - out["kl_dim"].sum(1)).abs().max() < 1e-10 and (out["kl"] - out["step_kl"].sum(0)).abs().max() < 1e-10
    assert (out["abs_log_ratio"] >= out["log_ratio"].abs() - 1e-12).all() and (out["abs_kl"] >= out["kl"].abs() - 1e-12).all()
    # a dead step contributes nothing, whatever it holds; a per-row prior mean is broadcast
    mu2, z2 = mu.clone(), z.clone()
    mu2[w == 0] = float("nan")
    z2[w == 0] = float("nan")
    again = PR.posterior_rows(mu2, lv, z2, eps, w, pm, kld_mode, pv)
    assert all(torch.equal(out[k], again[k]) for k in out)
    row = torch.linspace(-1, 1, B, dtype=torch.float64)
    a = PR.posterior_rows(mu, lv, z, eps, w, row, kld_mode, pv)
    b = PR.posterior_rows(mu, lv, z, eps, w, row.view(1, B, 1).expand(T, B, Z), kld_mode, pv)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_bounds_properties():
    """iwae >= elbo always; K identical samples give iwae == elbo == log_w and ess = K; one dominant weight gives ess -> 1."""
    g = torch.Generator().manual_seed(3)
    lw = torch.randn(50, 6, generator=g, dtype=torch.float64) * 20 - 100
    elbo, iwae, ess = PR.bounds(lw)
    assert (iwae >= elbo - 1e-12).all() and (ess >= 1 - 1e-12).all() and (ess <= 6 + 1e-12).all()
    same = torch.full((3, 5), -42.25, dtype=torch.float64)
    elbo, iwae, ess = PR.bounds(same)
    assert (elbo == -42.25).all() and (iwae - elbo).abs().max() < 1e-12 and (ess - 5).abs().max() < 1e-12
    _, _, ess = PR.bounds(torch.tensor([[0.0, -800.0, -900.0]], dtype=torch.float64))
    assert abs(float(ess) - 1) < 1e-12
    # the product's float32 reductions agree with the float64 ones; absent slots are zero
    lw32 = lw.float()
    e, i, s = PosteriorScores.reduce(lw32, torch.tensor([True] * 49 + [False]))
    e64, i64, s64 = PR.bounds(lw32)
    assert (e[:49].double() - e64[:49]).abs().max() < 1e-4 and (i[:49].double() - i64[:49]).abs().max() < 1e-4
    assert (s[:49].double() - s64[:49]).abs().max() < 1e-4 and float(e[49]) == float(i[49]) == float(s[49]) == 0.0


def test_monte_carlo_kl_on_a_fixed_seed():
    """4096 eps draws of one step (seed 11): -mean(step_ratio) within 4 standard errors (computed here) of the closed-form
    KL(q || N(pm, pv))."""
    n, Z, pv = 4096, 8, 0.49
    g = torch.Generator().manual_seed(11)
    mu = (torch.randn(Z, generator=g, dtype=torch.float64) * 0.8).expand(1, n, Z)
    lv = (torch.randn(Z, generator=g, dtype=torch.float64) - 0.5).expand(1, n, Z)
    pm = (torch.randn(Z, generator=g, dtype=torch.float64) * 0.3).expand(1, n, Z)
    eps = torch.randn(1, n, Z, generator=g, dtype=torch.float64)
    out = PR.posterior_rows(mu, lv, eps * (lv / 2).exp() + mu, eps, torch.ones(1, n, dtype=torch.float64), pm, 1, pv)
    est = -out["step_ratio"][0]
    want = float(PR.kl_closed_form(mu[0, 0], lv[0, 0], pm[0, 0], pv))
    se = float(est.std(unbiased=True)) / math.sqrt(n)
    print(f"MC KL {float(est.mean()):.5f} closed form {want:.5f} standard error {se:.5f}")
    assert se > 0 and abs(float(est.mean()) - want) < 4 * se


def test_chunk_planner():
    """Whole captions per chunk, absent slots dropped, every present slot exactly once and in order, each chunk trimmed to its
    longest caption; n_samples > max_rows raises."""
    words = [3, 0, 5, 1, 0, 0, 7, 2, 4]
    chunks = plan_posterior_chunks(words, 3, max_rows=7)       # two captions (6 rows) per forward
    assert chunks == [([0, 2], 5), ([3, 6], 7), ([7, 8], 4)]
    assert plan_posterior_chunks(words, 3, max_rows=3) == [([i], words[i]) for i in (0, 2, 3, 6, 7, 8)]
    assert plan_posterior_chunks(words, 2) == [([0, 2, 3, 6, 7, 8], 7)]
    assert plan_posterior_chunks([0, 0], 2) == []
    for slots, length in plan_posterior_chunks(list(range(40)), 5, max_rows=64):
        assert 1 <= len(slots) * 5 <= 64 and length == max(slots) and 0 not in slots
    with pytest.raises(ValueError, match="max_rows"):
        plan_posterior_chunks(words, 8, max_rows=7)
    with pytest.raises(ValueError):
        plan_posterior_chunks(words, 0)


def hand_scores():
    # two images x two slots x K = 2; slot (1, 1) is absent
    log_w = torch.tensor([[[-10.0, -12.0], [-6.0, -6.0]], [[-20.0, -20.0], [0.0, 0.0]]])
    nll = torch.tensor([[[8.0, 9.0], [5.0, 5.5]], [[18.0, 17.0], [0.0, 0.0]]])
    log_ratio = log_w + nll
    kld = torch.tensor([[[3.0, 3.0], [1.0, 1.0]], [[2.0, 4.0], [0.0, 0.0]]])
    n_tokens = torch.tensor([[4, 2], [4, 0]])
    elbo, iwae, ess = PosteriorScores.reduce(log_w, n_tokens > 0)
    kl_dim = torch.tensor([0.3, 0.19, 6.0, 0.21], dtype=torch.float64)
    return PosteriorScores(log_w, nll, log_ratio, kld, n_tokens, elbo, iwae, ess, kl_dim, n_steps=20)


def test_summary_on_hand_made_numbers():
    s = hand_scores().summary()
    lse = math.log(math.exp(-10) + math.exp(-12)) - math.log(2)
    assert s["n_captions"] == 3 and s["n_tokens"] == 10
    assert s["elbo_nll_per_token"] == pytest.approx((11 + 6 + 20) / 10, abs=1e-6)
    assert s["iwae_nll_per_token"] == pytest.approx((-lse + 6 + 20) / 10, abs=1e-6)
    assert s["recon_nll_per_token"] == pytest.approx((8.5 + 5.25 + 17.5) / 10, abs=1e-6)
    assert s["kl_per_token"] == pytest.approx((3 + 1 + 3) / 10, abs=1e-6)
    assert s["kl_mc_per_token"] == pytest.approx(s["elbo_nll_per_token"] - s["recon_nll_per_token"], abs=1e-6)
    w = torch.tensor([1.0, math.exp(-2)])
    assert s["ess_mean"] == pytest.approx((float(w.sum() ** 2 / (w ** 2).sum()) + 2 + 2) / 3, abs=1e-5)
    assert s["active_units"] == 3                      # 0.3 / 20 > 0.01, 0.19 / 20 is not, 6 / 20, 0.21 / 20
    assert s["iwae_nll_per_token"] <= s["elbo_nll_per_token"]
    both = PosteriorScores.concat([hand_scores(), hand_scores()])
    assert both.log_w.shape == (4, 2, 2) and both.n_steps == 40 and torch.equal(both.kl_dim, 2 * hand_scores().kl_dim)
    s2 = both.summary()
    assert s2["n_tokens"] == 20 and s2["elbo_nll_per_token"] == pytest.approx(s["elbo_nll_per_token"], abs=1e-6)
    assert s2["active_units"] == 3
    empty = hand_scores()
    empty.n_tokens = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError):
        empty.summary()


def test_train_script_flag_parses(monkeypatch):
    """--val-posterior-samples K; off - and absent from the namespace - unless given."""
    import sys
    monkeypatch.setattr(sys, "path", list(sys.path))
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    spec = importlib.util.spec_from_file_location("ssc_train_script_posterior", os.path.join(ROOT, "scripts", "train.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    a = t.parser.parse_args(["--config", "c", "--gpu-ids", "0"])
    assert getattr(a, "val_posterior_samples", 0) == 0 and "val_posterior_samples" not in vars(a)
    a = t.parser.parse_args(["--config", "c", "--gpu-ids", "0", "--val-tensors", "v.pt", "--val-posterior-samples", "8"])
    assert a.val_posterior_samples == 8 and a.val_tensors == "v.pt"
    with pytest.raises(SystemExit):
        t.parser.parse_args(["--config", "c", "--gpu-ids", "0", "--val-posterior-samples", "many"])
    assert callable(t.validate_posterior)


def test_posterior_rows_rejects_bad_arguments_without_a_gpu():
    """Every bad-argument case of ssc_posterior_rows is SSC_EINVAL (-1) before anything is launched or read (host memory here)."""
    lib = L.load()
    T, B, Z, ldz = 2, 3, 5, 8
    buf = (C.c_float * (T * B * ldz))()
    a = C.addressof(buf)

    def desc(**kw):
        d = L.PosteriorRowsDesc()
        d.T, d.B, d.Z, d.ldz, d.ldeps, d.ldpm, d.ld = T, B, Z, ldz, ldz, ldz, ldz
        d.mu = d.lv = d.z = d.eps = d.w = d.log_ratio = d.kl = a
        d.kld_mode, d.prior_var = 1, 0.49
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [dict(mu=None), dict(lv=None), dict(z=None), dict(eps=None), dict(w=None), dict(log_ratio=None), dict(kl=None),
           dict(T=0), dict(B=0), dict(Z=0), dict(B=-1), dict(Z=513), dict(ldz=Z - 1), dict(ldeps=Z - 1), dict(pm=a, ldpm=Z - 1),
           dict(kl_dim=a, ld=Z - 1), dict(prior_var=0.0), dict(prior_var=-1.0), dict(prior_var=float("nan")), dict(kld_mode=-1),
           dict(kld_mode=3), dict(kld_mode=2)]
    for kw in bad:
        assert lib._raw_ssc_posterior_rows(C.byref(desc(**kw)), None) == -1, kw
    assert lib._raw_ssc_posterior_rows(None, None) == -1
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    bt = L.Batch(2, 3, 4, a, a, None, a, None)
    assert lib._raw_ssc_train_posterior(C.byref(cfg), C.byref(bt), None, 0, a, a, a, None, 0, None, None, None) == -1
    assert lib._raw_ssc_train_posterior(C.byref(cfg), C.byref(bt), a, 16, a, a, a, None, 0, None, None, None) == -4   # SSC_EWORKSPACE
    assert lib._raw_ssc_train_posterior(C.byref(cfg), C.byref(bt), a, 16, None, a, a, None, 0, None, None, None) == -1
