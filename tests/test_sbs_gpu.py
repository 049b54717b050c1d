"""GPU: the stochastic beam search (ssc_beam_first_gumbel / ssc_beam_step_gumbel, ssc_decode_stochastic_beam,
DecodeEngine.stochastic_beam, diverse_decode / UpDownCaptioner / scripts/inference.py with the Gumbel sampler) against the
reference's own GumbelSampler + BeamSearch (tests/golden/g18_stochastic_beam.npz), the float64 restatement (tests/sbsref.py), the
multinomial word sampler at beam 1 and the CPU oracle."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import sbsref as R
from oracle.seqcvae_oracle import zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from test_sampling_gpu import ROOT, chi2_pvalue, inputs, model, run_child

pytestmark = pytest.mark.gpu


class Steps:
    """The stand-alone selection entries on device buffers for B entries of k beams, n candidates per beam."""

    def __init__(self, B, k, n, V, T, seed, end=R.END):
        self.B, self.k, self.n, self.V, self.end = B, k, n, V, end
        self.s = sampling.GumbelSampler(T).desc(seed)
        dev = "cuda"
        self.pred = torch.empty(B, k, dtype=torch.int64, device=dev)
        self.lp = torch.empty(B, k, dtype=torch.float32, device=dev)
        self.G = torch.empty(B, k, dtype=torch.float32, device=dev)
        self.bp = torch.empty(B, k, dtype=torch.int64, device=dev)
        self.sval = torch.empty(2 * B * k * max(n, k), dtype=torch.float32, device=dev)
        self.sidx = torch.empty(B * k * max(n, k), dtype=torch.int64, device=dev)

    def desc(self, scores):
        d = L.BeamDesc()
        d.scores, d.ld, d.raw_logits = L.ptr(scores), self.V, 1
        d.dims = L.FsmDims(0, 1, self.V, 0, 1)
        d.B, d.beam, d.per_node, d.end_index = self.B, self.k, self.n, self.end
        d.pred, d.lp_out, d.backptr = L.ptr(self.pred), L.ptr(self.lp), L.ptr(self.bp)
        d.scratch_val, d.scratch_idx = L.ptr(self.sval), L.ptr(self.sidx)
        return d

    def first(self, rows):
        rows = torch.as_tensor(rows).cuda().contiguous()
        L.load().ssc_beam_first_gumbel(self.desc(rows), self.s, L.ptr(self.G), L.stream_ptr())
        torch.cuda.synchronize()
        return self.pred.cpu().numpy(), self.lp.cpu().numpy().astype(np.float64), self.G.cpu().numpy().astype(np.float64)

    def step(self, rows, t, last_pred, last_lp, g_last):
        rows = torch.as_tensor(rows).cuda().contiguous()
        last = torch.as_tensor(np.asarray(last_pred, dtype=np.int64)).cuda().contiguous()
        phi = torch.as_tensor(np.asarray(last_lp, dtype=np.float32)).cuda().contiguous()
        gl = torch.as_tensor(np.asarray(g_last, dtype=np.float32)).cuda().contiguous()
        d = self.desc(rows)
        d.last_pred, d.last_lp, d.step_index = L.ptr(last), L.ptr(phi), t
        L.load().ssc_beam_step_gumbel(d, self.s, L.ptr(gl), L.ptr(self.G), L.stream_ptr())
        torch.cuda.synchronize()
        return (self.pred.cpu().numpy(), self.lp.cpu().numpy().astype(np.float64), self.G.cpu().numpy().astype(np.float64),
                self.bp.cpu().numpy())

    def candidates(self, rows_n):
        """the row kernel's own output of the last call: (tokens, G, summed log-probs) (rows, n)."""
        m = rows_n * self.n
        sv = self.sval.cpu().numpy()
        return self.sidx.cpu().numpy()[:m].reshape(-1, self.n), sv[:m].reshape(-1, self.n), sv[m: 2 * m].reshape(-1, self.n)


def _finite_gap(x):
    x = np.sort(x[np.isfinite(x)])
    return np.diff(x).min() if x.size > 1 else np.inf


def _check(what, gap, tok, lp, G, rtok, rlp, rG, bp=None, rbp=None):
    ok = gap > 1e-5
    np.testing.assert_array_equal(tok[ok], rtok[ok], err_msg=str(what))
    if bp is not None:
        np.testing.assert_array_equal(bp[ok], rbp[ok], err_msg=str(what))
    np.testing.assert_allclose(lp[ok], rlp[ok], atol=1e-5, rtol=0, err_msg=str(what))
    np.testing.assert_allclose(G[ok], rG[ok], rtol=1e-5, atol=1e-6, err_msg=str(what))
    return int(ok.sum())


def test_reference_parity():
    """Every g18 case, each step teacher-forced on the reference's own selections: tokens and back-pointers equal wherever the
    entry's margin exceeds 1e-5, log-probs within 1e-5, G within 1e-5 relative."""
    fx, cases = R.load_fixture()
    checked = total = 0
    for c in cases:
        rec = fx[c["name"]]
        st = Steps(c["B"], c["k"], c["n"], c["V"], c["T"], R.SEED)
        for t, rows in R.replay(c, rec):
            total += c["B"]
            if t == 0:
                tok, lp, G = st.first(rows)
                checked += _check((c["name"], t), rec["gap"][t], tok, lp, G, rec["tok"][t], rec["lp_t"][t], rec["G"][t])
            else:
                tok, lp, G, bp = st.step(rows, t, rec["tok"][t - 1].reshape(-1), rec["lp_t"][t - 1].reshape(-1),
                                         rec["G"][t - 1].reshape(-1))
                checked += _check((c["name"], t), rec["gap"][t], tok, lp, G, rec["tok"][t], rec["lp_t"][t], rec["G"][t], bp,
                                  rec["bp"][t])
    assert checked > 0.9 * total


@pytest.mark.parametrize("V", [50, 10000, 40000])
def test_row_kernel_against_the_restatement(V):
    """Random rows (ended rows mixed in), T in {0.7, 1, 1.6}, n in {1, 2, 5}: the row kernel's candidates and the merged step
    against the float64 restatement, margin-aware; G within 1e-5 relative.  V 40 000 takes the global-memory form."""
    rng = np.random.default_rng(V)
    B, k = 6, 5
    for T in (0.7, 1.0, 1.6):
        for n in (1, 2, 5):
            logits = (rng.standard_normal((B * k, V)) * 2.5).astype(np.float32)
            lsm = logits.astype(np.float64) - np.log(np.exp(logits.astype(np.float64)).sum(1, keepdims=True))
            last = rng.integers(0, V, B * k)
            last[rng.random(B * k) < 0.3] = R.END
            phi = rng.uniform(-12, -1, B * k).astype(np.float32)
            Gp = (phi + rng.uniform(0, 2, B * k)).astype(np.float32)
            st = Steps(B, k, n, V, T, seed=1000 + n)
            tok, lp, G, bp = st.step(logits, 3, last, phi, Gp)
            ctok, cG, cL = st.candidates(B * k)
            rtok, rG, rL = R.row_candidates(lsm, last, phi.astype(np.float64), Gp.astype(np.float64), n, T, 1000 + n, 3)
            # margin of each row's decisions: the g of its (n)-th and (n+1)-th tokens, in float64
            lpT = R._lsm(lsm / T) if T != 1.0 else lsm
            g = np.sort(R.perturbed(phi[:, None].astype(np.float64) + lpT, R.uniforms(V, 1000 + n, 3, np.arange(B * k))), 1)[:, ::-1]
            rgap = np.diff(-g[:, : n + 1], axis=1).min(1)
            rgap[last == R.END] = np.inf
            ok = rgap > 1e-5
            assert ok.mean() > 0.8
            np.testing.assert_array_equal(ctok[ok], rtok[ok], err_msg=str((V, T, n)))
            fin = ok[:, None] & np.isfinite(rG)
            np.testing.assert_allclose(cG[fin], rG[fin], rtol=1e-5, atol=1e-5, err_msg=str((V, T, n)))
            np.testing.assert_allclose(cL[fin], rL[fin], atol=1e-5, err_msg=str((V, T, n)))
            assert np.isneginf(cG[~np.isfinite(rG)]).all()
            mt, ml, mG, msel = R.merge(rtok, rG, rL, B, k)
            egap = np.minimum(rgap.reshape(B, k).min(1), [_finite_gap(rG.reshape(B, -1)[e]) for e in range(B)])
            egap = np.minimum(egap, [_finite_gap(ml[e]) for e in range(B)])
            _check((V, T, n), egap, tok, lp, G, mt, ml, mG, bp, msel // n)


def test_step0_frequencies_follow_softmax():
    """k = 1 at step 0 over 65 536 rows of one V = 50 row (distinct row ids): chi-square of the tokens against softmax(lp)."""
    rng = np.random.default_rng(8)
    lp = rng.standard_normal(50) * 1.5
    lp -= np.log(np.exp(lp).sum())
    n = 65536
    st = Steps(n, 1, 1, 50, 1.0, seed=4242)
    tok, _, _ = st.first(torch.from_numpy(lp.astype(np.float32)).view(1, 50).expand(n, 50).contiguous())
    counts = np.bincount(tok.reshape(-1), minlength=50).astype(np.float64)
    exp = np.exp(lp) * n
    big = exp >= 5
    obs_b, exp_b = counts[big], exp[big]
    if (~big).any():   # (the rare tokens pooled)
        obs_b, exp_b = np.append(obs_b, counts[~big].sum()), np.append(exp_b, exp[~big].sum())
    x = ((obs_b - exp_b) ** 2 / exp_b).sum()
    assert chi2_pvalue(x, len(obs_b) - 1) > 1e-3, x


def _entry_inputs(cfg, nimg, ns, R_, k, seed, steps=None):
    """inputs() with the latent noise of the later steps repeated over the k beams of each entry."""
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R_, seed, steps)
    return feats, senti, eps0, eps.repeat_interleave(k, dim=1)


def test_beam1_equals_multinomial():
    """k = n = 1, T = 1: every step is argmax(logit + g_v) with the multinomial sampler's noise - the captions of ssc_decode_sample
    with MultinomialSampler(1.0) and the same seed, log-probs within 1e-5."""
    cfg, _, _, dec = model(False)
    nimg, ns, R_ = 3, 4, 7
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R_, seed=31)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    L_ = cfg.max_caption_length
    a, alp = dec.stochastic_beam(ctx, sent_b, ns, 1, 1, L_, cfg.boundary_index, eps0.cuda(), eps.cuda(), sampling.GumbelSampler(),
                                 seed=55)
    b, blp = dec.sample(ctx, sent_b, ns, L_, cfg.boundary_index, eps0.cuda(), eps.cuda(), sampling.MultinomialSampler(1.0), seed=55)
    assert torch.equal(a[:, 0, :].cpu(), b.cpu())
    assert (alp[:, 0].cpu() - blp.cpu()).abs().max() <= 1e-5


def test_full_width_against_the_oracle():
    """H 1200, V 10 000, R 36, 8 images x 20 samples, k 5, n 2, 12 steps: every returned beam, teacher-forced through
    oracle.decode_step with its entry's noise, gives its log-prob within 1e-4; each entry's captions are pairwise distinct and
    sorted by log-prob; ended captions are padded with the end token."""
    cfg, params, _, dec = model(True)
    nimg, ns, R_, k, n, steps = 8, 20, 36, 5, 2, 12
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=41, steps=steps)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B)
    pred, lps = dec.stochastic_beam(ctx, sent_b.cuda(), ns, k, n, steps, cfg.boundary_index, eps0.cuda(), eps.cuda(),
                                    sampling.GumbelSampler(1.0), seed=2024)
    pred, lps = pred.cpu(), lps.cpu()
    assert pred.shape[:2] == (B, k)
    assert (lps[:, :-1] >= lps[:, 1:]).all()
    for b in range(B):
        assert len({tuple(x) for x in pred[b].tolist()}) == k
    end = cfg.boundary_index
    ended = (pred == end).cumsum(-1) > 0
    assert (pred[ended] == end).all()
    rows = B * k
    fr = feats.unsqueeze(1).expand(nimg, ns * k, R_, feats.size(2)).reshape(rows, R_, -1)
    se = sent_b.view(B, 1).repeat_interleave(k, 0)
    pm, pv = oracle.prior_from_sentiment(cfg, se, rows, fr)
    states = zero_states(rows, cfg.hidden_size, fr)
    flat = pred.reshape(rows, -1)
    tokens = torch.full((rows,), end, dtype=torch.long)
    total = torch.zeros(rows, dtype=torch.float64)
    alive = torch.ones(rows, dtype=torch.bool)
    with torch.no_grad():
        for t in range(flat.size(1)):
            e = eps0.repeat_interleave(k, 0) if t == 0 else eps[t - 1]
            lp, states, _, _, _ = oracle.decode_step(params, cfg, fr, tokens, states, False, se, pm, pv, e)
            tok = flat[:, t]
            total += torch.where(alive, lp.double().gather(1, tok.view(-1, 1)).view(-1), torch.zeros(rows, dtype=torch.float64))
            alive &= tok != end
            tokens = tok.clone()
    assert (total - lps.reshape(rows).double()).abs().max() < 1e-4


def test_seeds_and_stopping():
    cfg, _, _, dec = model(False)
    nimg, ns, R_, k = 3, 4, 7, 4
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=5)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(-1).cuda()
    s = sampling.GumbelSampler(1.3)
    L_ = cfg.max_caption_length
    run = lambda seed, **kw: dec.stochastic_beam(ctx, sent_b, ns, k, 2, L_, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed,
                                                 **kw)
    a, b, c = run(123), run(123), run(124)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])
    # without early stop: the same captions, surplus columns hold the end token, the log-probs are unchanged
    full = run(123, early_stop=False)
    steps = a[0].size(-1)
    assert torch.equal(full[0][..., :steps], a[0]) and (full[0][..., steps:] == cfg.boundary_index).all()
    assert torch.equal(full[1], a[1])
    # an overwhelming end token at k = 1: one column
    cfg2, _, _, dec2 = model(False, boundary_bias=60.0)
    ctx2 = dec2.prepare(feats.cuda())
    p, lp = dec2.stochastic_beam(ctx2, sent_b, ns, 1, 1, L_, cfg2.boundary_index, eps0.cuda(), eps[:, ::k].contiguous().cuda(), s, 9)
    assert p.shape == (nimg * ns, 1, 1) and (p == cfg2.boundary_index).all()


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", {seed!r}, "MODEL.STOCHASTIC_BEAM_SEARCH", "True", "MODEL.BEAM_SIZE", "5",
                            "MODEL.IMAGE_FEATURE_SIZE", "64", "MODEL.EMBEDDING_SIZE", "40", "MODEL.HIDDEN_SIZE", "48",
                            "MODEL.ATTENTION_PROJECTION_SIZE", "32", "MODEL.Z_SPACE", "16", "DATA.MAX_CAPTION_LENGTH", "8"])
torch.manual_seed(C.RANDOM_SEED)
m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                sampler=sampling.from_config(C.MODEL)).cuda().eval()
g = torch.Generator().manual_seed(0)
feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
out = m(feats)["predictions"]
print(json.dumps(out.cpu().tolist()))
"""


def test_module_and_script():
    outs = {}
    for seed in ("3", "3", "4"):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"), seed=seed)
        outs.setdefault(seed, []).append(json.loads(run_child(["-c", src]).strip().splitlines()[-1]))
    a, b = outs["3"]
    assert a == b and len(a) == 8 and all(0 < len(c) <= 8 for c in a)
    assert outs["4"][0] != a
    # a sampler with constraints is refused
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    m = UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=3, z_space=4, sampler=sampling.GumbelSampler()).cuda().eval()
    m._use_cbs = True
    with pytest.raises(ValueError, match="USE_CBS"):
        m(torch.randn(2, 3, 16, device="cuda"), fsm=torch.ones(2, 1, 1, 50, dtype=torch.uint8))
    cfg, _, _, dec = model(False)
    with pytest.raises(ValueError, match="constraints"):
        diverse_decode(dec, torch.randn(2, 3, cfg.image_feature_size).cuda(), None, 2, 3, 5, cfg.boundary_index,
                       fsm=torch.ones(2, 1, 1, cfg.vocab_size, dtype=torch.uint8).cuda(), sampler=sampling.GumbelSampler())


def test_inference_script_with_stochastic_beam_search(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
                   "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
                   "  BEAM_SIZE: 5\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
                   "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n")
    out = tmp_path / "pred.json"
    run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4",
               "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--config-override",
               "MODEL.STOCHASTIC_BEAM_SEARCH", "True", "MODEL.BEAM_SIZE", "5"])
    caps = json.load(open(out))
    assert len(caps) == 4 * 5 and all(isinstance(c["caption"], str) for c in caps)
