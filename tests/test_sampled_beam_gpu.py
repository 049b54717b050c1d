"""GPU: the sampled-node beam search (ssc_beam_step_sampled, ssc_decode_sampled_beam, DecodeEngine.sampled_beam, diverse_decode /
UpDownCaptioner / scripts/inference.py with MODEL.SAMPLED_BEAM_SEARCH) against the reference's own BeamSearch with its word
samplers (tests/golden/g19_sampled_beam.npz), the float64 restatement (tests/sampledbeamref.py), ssc_sample_rows, the beam search
and the CPU oracle."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import sampledbeamref as R
from oracle.seqcvae_oracle import zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from test_sampling_gpu import ROOT, chi2_pvalue, inputs, model, run_child, sample_rows

pytestmark = pytest.mark.gpu

SAMPLERS = {"multinomial": lambda T, rep, k, p: sampling.MultinomialSampler(T, with_replacement=rep),
            "top-k": lambda T, rep, k, p: sampling.TopKSampler(k=k, temperature=T, with_replacement=rep),
            "top-p": lambda T, rep, k, p: sampling.TopPSampler(p=p, temperature=T, with_replacement=rep)}


class Steps:
    """The stand-alone step (and ssc_beam_first_fsm for step 0) on device buffers: B entries of k beams, n candidates per beam."""

    def __init__(self, B, k, n, V, sampler, seed, end=R.END):
        self.B, self.k, self.n, self.V, self.end = B, k, n, V, end
        self.sampler = sampler
        self.s = sampler.desc(seed)
        dev = "cuda"
        self.pred = torch.empty(B, k, dtype=torch.int64, device=dev)
        self.lp = torch.empty(B, k, dtype=torch.float32, device=dev)
        self.bp = torch.empty(B, k, dtype=torch.int64, device=dev)
        self.sval = torch.empty(B * k * n, dtype=torch.float32, device=dev)
        self.sidx = torch.empty(B * k * n, dtype=torch.int64, device=dev)

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
        L.load().ssc_beam_first_fsm(self.desc(rows), L.stream_ptr())
        torch.cuda.synchronize()
        return self.pred.cpu().numpy(), self.lp.cpu().numpy().astype(np.float64)

    def step(self, rows, t, last_pred, last_lp):
        rows = torch.as_tensor(rows).cuda().contiguous()
        last = torch.as_tensor(np.asarray(last_pred, dtype=np.int64)).cuda().contiguous()
        phi = torch.as_tensor(np.asarray(last_lp, dtype=np.float32)).cuda().contiguous()
        d = self.desc(rows)
        d.last_pred, d.last_lp, d.step_index = L.ptr(last), L.ptr(phi), t
        L.load().ssc_beam_step_sampled(d, self.s, 1 if self.sampler.with_replacement else 0, L.stream_ptr())
        torch.cuda.synchronize()
        return self.pred.cpu().numpy(), self.lp.cpu().numpy().astype(np.float64), self.bp.cpu().numpy()

    def candidates(self):
        """the row kernel's own output of the last step: (tokens, summed log-probs) (rows, n)."""
        return self.sidx.cpu().numpy().reshape(-1, self.n), self.sval.cpu().numpy().reshape(-1, self.n)


def _case_sampler(c):
    return SAMPLERS[c["kind"]](c["T"], c["rep"], c["top_k"], c["top_p"])


def test_reference_parity():
    """Every g19 case, each step teacher-forced on the reference's own selections: tokens and back-pointers equal wherever the
    entry's margin exceeds 1e-5, summed log-probs within 1e-5.  Includes V 40 003 (the global-memory form)."""
    fx, cases = R.load_fixture()
    checked = total = 0
    for c in cases:
        rec = fx[c["name"]]
        st = Steps(c["B"], c["k"], c["n"], c["V"], _case_sampler(c), R.SEED)
        for t, rows in R.replay(c, rec):
            total += c["B"]
            ok = rec["gap"][t] > 1e-5
            what = (c["name"], t)
            if t == 0:
                tok, lp = st.first(rows)
            else:
                tok, lp, bp = st.step(rows, t, rec["tok"][t - 1].reshape(-1), rec["lp_t"][t - 1].reshape(-1))
                np.testing.assert_array_equal(bp[ok], rec["bp"][t][ok], err_msg=str(what))
            np.testing.assert_array_equal(tok[ok], rec["tok"][t][ok], err_msg=str(what))
            np.testing.assert_allclose(lp[ok], rec["lp_t"][t][ok], atol=1e-5, rtol=0, err_msg=str(what))
            checked += int(ok.sum())
    assert checked > 0.9 * total


@pytest.mark.parametrize("V", [51, 10000, 40000])
def test_row_kernel_against_the_restatement(V):
    """Random rows (ended rows mixed in), every kind, both replacement modes, n in {1, 2, 5}: the row kernel's candidates equal the
    float64 restatement's wherever the row's margin exceeds 1e-5, summed log-probs within 1e-6 (+ 1e-6 relative)."""
    rng = np.random.default_rng(V)
    B, k = 4, 5
    for kind in R.KINDS:
        for rep in (False, True):
            for n, T in ((1, 1.0), (2, 0.7), (5, 1.6)):
                logits = (rng.standard_normal((B * k, V)) * 2.5).astype(np.float32)
                last = rng.integers(0, V, B * k)
                last[rng.random(B * k) < 0.3] = R.END
                phi = rng.uniform(-12, -1, B * k).astype(np.float32)
                s = SAMPLERS[kind](T, rep, 7, 0.7)
                st = Steps(B, k, n, V, s, seed=1000 + n)
                st.step(logits, 3, last, phi)
                ctok, cL = st.candidates()
                kid, top_k, top_p, _ = R.sampler_args(dict(kind=kind, top_k=7, top_p=0.7, T=T))
                rtok, rL, gap = R.row_candidates(logits, last, phi.astype(np.float64), n, kind, top_k, top_p, T, rep, 1000 + n, 3)
                ok = gap > 1e-5
                assert ok.mean() > 0.8, (kind, rep, n)
                what = (V, kind, rep, n, T)
                np.testing.assert_array_equal(ctok[ok], rtok[ok], err_msg=str(what))
                fin = ok[:, None] & np.isfinite(rL)
                np.testing.assert_allclose(cL[fin], rL[fin], atol=1e-6, rtol=1e-6, err_msg=str(what))
                assert np.isneginf(cL[ok[:, None] & ~np.isfinite(rL)]).all()


@pytest.mark.parametrize("rep", [False, True])
def test_beam1_equals_sample_rows(rep):
    """k = n = 1: one step draws ssc_sample_rows' token for the same row id and step, with its log-prob, bit for bit."""
    rng = np.random.default_rng(7)
    for kind, V in (("multinomial", 50), ("top-k", 1001), ("top-p", 10000), ("top-p", 40000)):
        B = 64
        logits = torch.from_numpy((rng.standard_normal((B, V)) * 2).astype(np.float32)).cuda()
        s = SAMPLERS[kind](0.8, rep, 10, 0.9)
        st = Steps(B, 1, 1, V, s, seed=99)
        phi = rng.uniform(-5, 0, B).astype(np.float32)
        tok, lp, bp = st.step(logits, 4, np.full(B, R.END + 1), phi)
        row_lp = torch.from_numpy(phi).cuda()
        stok, _, _ = sample_rows(logits, s, 99, step=4, row_lp=row_lp, end_index=R.END)
        assert np.array_equal(tok[:, 0], stok.cpu().numpy()), kind
        assert np.array_equal(lp[:, 0].astype(np.float32), row_lp.cpu().numpy()), kind
        assert (bp == 0).all()


def test_ended_beams_duplicate_with_replacement():
    """An ended beam is one-hot at the end token: with replacement each of its n draws is the end token at phi, so the merge can
    keep a finished caption twice (as the reference does); without replacement it offers it once."""
    V, k, n = 50, 3, 2
    logits = np.random.default_rng(1).standard_normal((k, V)).astype(np.float32)
    last = np.array([R.END, 7, 9])
    phi = np.array([-0.1, -50.0, -60.0], np.float32)
    for rep, ends in ((True, 2), (False, 1)):
        st = Steps(1, k, n, V, sampling.MultinomialSampler(with_replacement=rep), seed=3)
        tok, lp, bp = st.step(logits, 2, last, phi)
        assert (tok[0, :ends] == R.END).all() and (bp[0, :ends] == 0).all() and (lp[0, :ends] == np.float32(-0.1)).all()
        assert tok[0, ends] != R.END and bp[0, ends] == 1
        assert (lp[0, :-1] >= lp[0, 1:]).all()


@pytest.mark.parametrize("rep", [False, True])
def test_node_pair_frequencies(rep):
    """n = 2 over 65 536 rows of one V = 6 row: the ordered pairs drawn follow Plackett-Luce p_a p_b / (1 - p_a) without
    replacement, p_a p_b with replacement (chi-square)."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(6) * 1.2).astype(np.float32)
    p = np.exp(x.astype(np.float64) - x.max())
    p /= p.sum()
    rows = 65536
    st = Steps(rows, 1, 2, 6, sampling.MultinomialSampler(with_replacement=rep), seed=31337)
    st.step(torch.from_numpy(x).view(1, 6).expand(rows, 6).contiguous(), 1, np.full(rows, R.END + 1), np.zeros(rows))
    ctok, _ = st.candidates()
    counts = np.zeros((6, 6))
    np.add.at(counts, (ctok[:, 0], ctok[:, 1]), 1)
    exp = p[:, None] * p[None, :] * rows
    if not rep:
        exp = exp / (1 - p)[:, None]
        np.fill_diagonal(exp, 0)
        assert np.trace(counts) == 0
    cells = exp > 0
    obs, e = counts[cells], exp[cells]
    big = e >= 5
    obs_b, e_b = np.append(obs[big], obs[~big].sum()), np.append(e[big], e[~big].sum())
    if e_b[-1] == 0:
        obs_b, e_b = obs_b[:-1], e_b[:-1]
    xs = ((obs_b - e_b) ** 2 / e_b).sum()
    assert chi2_pvalue(xs, len(obs_b) - 1) > 1e-3, xs


def _entry_inputs(cfg, nimg, ns, R_, k, seed, steps=None):
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R_, seed, steps)
    return feats, senti, eps0, eps.repeat_interleave(k, dim=1)


@pytest.mark.parametrize("sampler", [sampling.TopKSampler(k=2), sampling.TopPSampler(p=0.0)])
def test_deterministic_limits_equal_beam_search(sampler):
    """TopKSampler(k = n) and TopPSampler(p = 0) without replacement draw the top n tokens of every beam: at full width (H 1200,
    V 10 000, R 36, 8 images x 20 samples, beam 5, per_node 2, 8 steps) the captions are the beam search's, log-probs within
    1e-5 (+ two fp32 ulps of the sum: the searches sum in a different order).  Entries whose final beam-search log-probs come
    within 2e-4 of a tie are left out of the caption comparison - a proxy for the per-step selection margin, stricter than it
    where a step's margin is wide but the final beams end up close (it can only leave out comparable entries)."""
    cfg, _, _, dec = model(True)
    nimg, ns, R_, k, n, steps = 8, 20, 36, 5, 2, 8
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=23, steps=steps)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    beams, blp = dec.search(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0.cuda(), eps.cuda(), skip_dead=True)
    pred, slp = dec.sampled_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0.cuda(), eps.cuda(), sampler, seed=77)
    beams, blp, pred, slp = beams[:, 0].cpu(), blp.reshape(B, k).cpu(), pred.cpu(), slp.cpu()
    assert pred.shape == beams.shape, (pred.shape, beams.shape)
    d = blp[:, :-1] - blp[:, 1:]
    ok = (d > 2e-4).all(1)
    assert ok.float().mean() > 0.8
    assert torch.equal(pred[ok], beams[ok])
    assert ((slp - blp).abs() <= 1e-5 + 3e-7 * blp.abs()).all()   # (+ two fp32 ulps of a sum near -72)


@pytest.mark.parametrize("kind,rep", [("top-k", False), ("top-p", True), ("multinomial", False)])
def test_full_width_against_the_oracle(kind, rep):
    """H 1200, V 10 000, R 36, 8 images x 20 samples, k 5, n 2, 10 steps: every beam, teacher-forced through oracle.decode_step
    with its entry's noise, gives its log-prob within 1e-4; every sampled token lies in the oracle's kept set (margin-aware at the
    cut); log-probs are sorted."""
    cfg, params, _, dec = model(True)
    nimg, ns, R_, k, n, steps = 8, 20, 36, 5, 2, 10
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=41, steps=steps)
    B = nimg * ns
    s = SAMPLERS[kind](0.9, rep, 12, 0.8)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B)
    pred, lps = dec.sampled_beam(ctx, sent_b.cuda(), ns, k, n, steps, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed=2024)
    pred, lps = pred.cpu(), lps.cpu()
    assert pred.shape[:2] == (B, k)
    assert (lps[:, :-1] >= lps[:, 1:]).all()
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
            lpd = lp.double()
            mine = lpd.gather(1, tok.view(-1, 1)).view(-1)
            if t > 0:   # (step 0 is the top k)
                srt = lpd.sort(1, descending=True).values
                if kind == "top-k":
                    inside = mine >= srt[:, s.k - 1] - 1e-4
                elif kind == "top-p":
                    q = torch.softmax(lpd / s.temperature, 1)
                    ahead = (q * (q > q.gather(1, tok.view(-1, 1)) + 1e-6)).sum(1)
                    inside = ahead < s.p + 1e-4
                else:
                    inside = torch.isfinite(mine)
                assert bool((inside | ~alive).all()), (kind, t)
            total += torch.where(alive, mine, torch.zeros(rows, dtype=torch.float64))
            alive &= tok != end
            tokens = tok.clone()
    assert (total - lps.reshape(rows).double()).abs().max() < 1e-4


def test_seeds_and_stopping():
    cfg, _, _, dec = model(False)
    nimg, ns, R_, k = 3, 4, 7, 4
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=5)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(-1).cuda()
    s = sampling.TopPSampler(p=0.9, temperature=1.3)
    L_ = cfg.max_caption_length
    run = lambda seed, **kw: dec.sampled_beam(ctx, sent_b, ns, k, 2, L_, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed, **kw)
    a, b, c = run(123), run(123), run(124)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])
    full = run(123, early_stop=False)
    steps = a[0].size(-1)
    assert torch.equal(full[0][..., :steps], a[0]) and (full[0][..., steps:] == cfg.boundary_index).all()
    assert torch.equal(full[1], a[1])
    # an overwhelming end token: every beam ends at step 0 and the search stops there
    cfg2, _, _, dec2 = model(False, boundary_bias=60.0)
    ctx2 = dec2.prepare(feats.cuda())
    p, lp = dec2.sampled_beam(ctx2, sent_b, ns, 1, 1, L_, cfg2.boundary_index, eps0.cuda(), eps[:, ::k].contiguous().cuda(), s, 9)
    assert p.shape == (nimg * ns, 1, 1) and (p == cfg2.boundary_index).all()


def test_diverse_decode_sampled_beam():
    cfg, _, _, dec = model(False)
    feats = torch.randn(3, 7, cfg.image_feature_size).cuda()
    senti = torch.tensor([1.0, 0.0, -1.0]).cuda()
    s = sampling.TopKSampler(k=6, with_replacement=True)
    torch.manual_seed(0)
    a, steps = diverse_decode(dec, feats, senti, 4, 5, cfg.max_caption_length, cfg.boundary_index, sampler=s, sampled_beam=True)
    torch.manual_seed(0)
    b, _ = diverse_decode(dec, feats, senti, 4, 5, cfg.max_caption_length, cfg.boundary_index, sampler=s, sampled_beam=True)
    assert a.shape == (3, 4, steps) and torch.equal(a, b)
    with pytest.raises(ValueError, match="word sampling draws one word per row"):   # without the keyword: beam 1 only, as before
        diverse_decode(dec, feats, senti, 4, 5, cfg.max_caption_length, cfg.boundary_index, sampler=s)
    with pytest.raises(ValueError, match="constraints"):
        diverse_decode(dec, feats, senti, 2, 3, 5, cfg.boundary_index, sampler=s, sampled_beam=True,
                       fsm=torch.ones(3, 1, 1, cfg.vocab_size, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="word sampler"):
        diverse_decode(dec, feats, senti, 2, 3, 5, cfg.boundary_index, sampler=sampling.GumbelSampler(), sampled_beam=True)


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", {seed!r}, "MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", "0.9",
                            "MODEL.SAMPLED_BEAM_SEARCH", "True", "MODEL.BEAM_SIZE", "5",
                            "MODEL.IMAGE_FEATURE_SIZE", "64", "MODEL.EMBEDDING_SIZE", "40", "MODEL.HIDDEN_SIZE", "48",
                            "MODEL.ATTENTION_PROJECTION_SIZE", "32", "MODEL.Z_SPACE", "16", "DATA.MAX_CAPTION_LENGTH", "8"])
torch.manual_seed(C.RANDOM_SEED)
m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                sampler=sampling.from_config(C.MODEL)).cuda().eval()
assert m.sampled_beam
g = torch.Generator().manual_seed(0)
feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
out = m(feats)["predictions"]
print(json.dumps(out.cpu().tolist()))
"""


def test_module_forward():
    outs = {}
    for seed in ("3", "3", "4"):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"), seed=seed)
        outs.setdefault(seed, []).append(json.loads(run_child(["-c", src]).strip().splitlines()[-1]))
    a, b = outs["3"]
    assert a == b and len(a) == 8 and all(0 < len(c) <= 8 for c in a)
    assert outs["4"][0] != a
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    with pytest.raises(ValueError, match="BEAM_SIZE"):   # the word sampler at beam > 1 without sampled_beam: refused as before
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=3, z_space=4, sampler=sampling.TopKSampler(k=4))
    m = UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=3, z_space=4, sampler=sampling.TopKSampler(k=4),
                        sampled_beam=True).cuda().eval()
    m._use_cbs = True
    with pytest.raises(ValueError, match="USE_CBS"):
        m(torch.randn(2, 3, 16, device="cuda"), fsm=torch.ones(2, 1, 1, 50, dtype=torch.uint8))


def test_inference_script_with_sampled_beam_search(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
                   "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
                   "  BEAM_SIZE: 5\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
                   "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n")
    out = tmp_path / "pred.json"
    run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4",
               "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--config-override",
               "MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", "True", "MODEL.BEAM_SIZE", "5"])
    caps = json.load(open(out))
    assert len(caps) == 4 * 5 and all(isinstance(c["caption"], str) for c in caps)
