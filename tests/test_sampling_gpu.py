"""GPU: the word samplers (ssc_sample_rows, ssc_decode_sample, DecodeEngine.sample, diverse_decode(sampler=...), the module's
eval forward and scripts/inference.py with MODEL.DECODE_SAMPLER) against the reference's own distributions
(tests/golden/g17_samplers.npz), the NumPy restatement of the draw (tests/samplerref.py), the beam-1 search and the CPU oracle."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import samplerref as S
from gpuutil import engine_from
from oracle.seqcvae_oracle import zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.inference import diverse_decode
from test_attention_trace_gpu import R_, STEPS, VARIANTS, entry_inputs, medium

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture():
    return S.load_fixture()


def make(kind, k, p, T):
    if kind == "multinomial":
        return sampling.MultinomialSampler(temperature=T)
    if kind == "top-k":
        return sampling.TopKSampler(k=k, temperature=T)
    return sampling.TopPSampler(p=p, temperature=T)


def sample_rows(logits, sampler, seed, step=0, row_ids=None, last_pred=None, row_lp=None, end_index=0, probs=False):
    lib = L.load()
    logits = logits.cuda().contiguous()
    rows, V = logits.shape
    pred = torch.empty(rows, dtype=torch.int64, device="cuda")
    lp = torch.empty(rows, dtype=torch.float32, device="cuda")
    po = torch.empty(rows, V, dtype=torch.float32, device="cuda") if probs else None
    d = sampler.desc(seed)
    lib.ssc_sample_rows(L.ptr(logits), V, rows, V, d, L.ptr(row_ids), step, L.ptr(last_pred), L.ptr(row_lp), end_index, L.ptr(pred),
                        L.ptr(lp), L.ptr(po), L.stream_ptr())
    torch.cuda.synchronize()
    return pred.cpu(), lp.cpu(), (po.cpu() if probs else None)


def test_filtered_distributions_match_the_reference():
    """ssc_sample_rows(probs_out=...) on the fixture rows against the reference's distributions (samplerref.check_against_reference:
    kept sets equal except within 1e-6 of p, and the tail the reference's fp32 cumsum drops at p = 1; probabilities within 1e-6)."""
    d, cfg = fixture()
    for V in cfg["vs"]:
        lp = torch.from_numpy(d[f"lp_V{V}"])
        for si, (kind, k, p, T) in enumerate(cfg["settings"]):
            key = f"dist_V{V}_s{si}"
            if key not in d:
                continue
            _, _, po = sample_rows(lp, make(kind, k, p, T), seed=11, probs=True)
            for r in range(lp.size(0)):
                ref = d[key][r].astype(np.float64)
                got = po[r].double().numpy()
                _, ahead = S.filter_dist(d[f"lp_V{V}"][r], kind, k, p, T)
                S.check_against_reference(got, ref, ahead, kind, p, (V, kind, k, p, T, r))
                assert abs(got.sum() - 1.0) < 1e-4


@pytest.mark.parametrize("V", [50, 9973, 10000, 30000, 40000])
def test_draws_equal_the_numpy_restatement(V):
    """The drawn token is argmax of logit / T + Gumbel(Philox) over the kept set: equal to the NumPy restatement wherever the top
    two perturbed scores differ by more than 1e-5; the step log-prob is the untempered log_softmax at the token (1e-6).  Odd V
    (9973) and V above the LDS-resident size (40000: the multi-pass form) included."""
    g = torch.Generator().manual_seed(V)
    rows = 24
    logits = torch.randn(rows, V, generator=g) * 2.0
    logits[::3] = (logits[::3] * 2).round() / 2   # exact ties
    row_ids = torch.arange(1000, 1000 + rows, dtype=torch.int64)
    lse = torch.logsumexp(logits.double(), dim=1)
    for sampler in (sampling.MultinomialSampler(temperature=0.8), sampling.TopKSampler(k=min(40, V), temperature=1.3),
                    sampling.TopPSampler(p=0.7, temperature=0.6)):
        seed = 0x0123_4567_89AB_CDEF + V
        tok, lp, po = sample_rows(logits, sampler, seed, step=5, row_ids=row_ids.cuda(), probs=True)
        checked = 0
        for r in range(rows):
            kept = po[r].numpy() > 0
            want, sc = S.draw(logits[r].numpy(), kept, sampler.temperature, seed, 5, int(row_ids[r]))
            top2 = np.sort(sc[np.isfinite(sc)])[-2:]
            if len(top2) == 2 and top2[1] - top2[0] <= 1e-5:
                continue
            assert int(tok[r]) == want, (sampler, r)
            assert kept[int(tok[r])]
            assert abs(float(lp[r]) - (float(logits[r, want]) - float(lse[r]))) < 1e-6
            checked += 1
        assert checked >= rows - 2


def chi2_pvalue(x, k):
    # Wilson-Hilferty: (X / k)^(1/3) is close to normal
    z = ((x / k) ** (1 / 3) - (1 - 2 / (9 * k))) / math.sqrt(2 / (9 * k))
    return 0.5 * math.erfc(z / math.sqrt(2))


@pytest.mark.parametrize("si_row", [(("multinomial", 0, 1.0, 1.7), 0), (("top-k", 5, 1.0, 1.3), 2), (("top-p", 0, 0.9, 0.7), 1),
                                    (("top-p", 0, 0.5, 1.3), 2)])
def test_draw_frequencies_follow_the_reference_distribution(si_row):
    """One launch of 65 536 copies of one fixture row (V = 50) with distinct row ids: chi-square of the token counts against the
    reference's distribution, p > 1e-3 (fixed seed: deterministic)."""
    (setting, r) = si_row
    d, cfg = fixture()
    si = cfg["settings"].index(setting)
    ref = d[f"dist_V50_s{si}"][r].astype(np.float64)
    n = 65536
    logits = torch.from_numpy(d["lp_V50"][r]).view(1, 50).expand(n, 50).contiguous()
    tok, _, _ = sample_rows(logits, make(*setting), seed=20251015, step=2)
    counts = np.bincount(tok.numpy(), minlength=50).astype(np.float64)
    assert counts[ref == 0].sum() == 0
    exp = ref * n
    big = exp >= 5
    obs_b = np.append(counts[big], counts[~big & (ref > 0)].sum())
    exp_b = np.append(exp[big], exp[~big & (ref > 0)].sum())
    keep = exp_b > 0
    x = (((obs_b - exp_b) ** 2)[keep] / exp_b[keep]).sum()
    dof = max(int(keep.sum()) - 1, 1)
    assert chi2_pvalue(x, dof) > 1e-3, (setting, x, dof)


def test_ended_rows_and_running_log_probs():
    """A row whose previous token is end_index emits end_index at log-prob 0 (its logits are not read: NaN here) and keeps its
    running log-prob; the others draw and add their step log-prob."""
    g = torch.Generator().manual_seed(3)
    V, rows, end = 300, 8, 1
    logits = torch.randn(rows, V, generator=g)
    logits[1::2] = float("nan")
    last = torch.tensor([5, end, 7, end, 9, end, 11, end], dtype=torch.int64).cuda()
    run = torch.full((rows,), -2.0, device="cuda")
    tok, lp, _ = sample_rows(logits, sampling.TopPSampler(p=0.9), seed=1, step=3, last_pred=last, row_lp=run, end_index=end)
    assert (tok[1::2] == end).all() and (lp[1::2] == 0).all()
    assert torch.isfinite(lp[0::2]).all() and (lp[0::2] < 0).all()
    want = -2.0 + lp
    assert torch.equal(run.cpu(), want)


# ---- the sampled decode ---------------------------------------------------------------------------------------------------
def model(full, seed=4, boundary_bias=0.0):
    if full:
        cfg = oracle.OracleConfig(vocab_size=10000, image_feature_size=2048, embedding_size=1000, hidden_size=1200,
                                  attention_projection_size=768, z_space=128, max_caption_length=20, sentiment_vae=1,
                                  senti_prior_multip=0.5, beam_size=1)
    else:
        cfg = oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32,
                                  attention_projection_size=16, z_space=8, max_caption_length=9, sentiment_vae=1,
                                  senti_prior_multip=0.5, beam_size=1)
    params = oracle.init_params(cfg, seed=seed)
    params["_output_layer.bias"][cfg.boundary_index] += boundary_bias
    eng = engine_from(cfg, params)
    return cfg, params, eng, DecodeEngine(eng.dims, eng.params.c_struct, "cuda")


def inputs(cfg, nimg, ns, R, seed, steps=None):
    g = torch.Generator().manual_seed(seed)
    steps = steps or cfg.max_caption_length
    B = nimg * ns
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g)
    senti = torch.randint(-1, 2, (nimg,), generator=g).float()
    eps0 = torch.randn(B, cfg.z_space, generator=g)
    eps = torch.randn(steps - 1, B, cfg.z_space, generator=g)
    return feats, senti, eps0, eps


@pytest.mark.parametrize("full", [False, True, "table"])
def test_top1_sampling_equals_beam1_search(full):
    """TopKSampler(k=1) through ssc_decode_sample draws the argmax: the beam-1 search's captions (the steps are formed alike, so
    the logits are the same) and its caption log-probs within 1e-5 (+ one fp32 ulp of the sum).  Toy width and full width (H 1200, V 10 000, R 36, 8 images x
    20 samples); "table": toy width at 2 images x 256 samples - 512 rows, 256 per image, the smallest extents at which both calls
    take the attended-feature-table form (formed by the call's first step, read by the later ones through the parent list)."""
    cfg, _, _, dec = model(full is True)
    nimg, ns, R = {False: (3, 4, 7), True: (8, 20, 36), "table": (2, 256, 7)}[full]
    L_ = cfg.max_caption_length
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R, seed=17)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    beams, blp = dec.search(ctx, sent_b, ns, 1, 1, L_, cfg.boundary_index, eps0.cuda(), eps.cuda(), skip_dead=True)
    pred, slp = dec.sample(ctx, sent_b, ns, L_, cfg.boundary_index, eps0.cuda(), eps.cuda(), sampling.TopKSampler(k=1), seed=5)
    assert torch.equal(pred.cpu(), beams[:, 0, 0, :].cpu())
    # (the two sum the same step log-probs, whose log-sum-exps are formed in different orders: 1e-5, plus one fp32 ulp of a sum
    # near -180 at full width)
    assert ((slp.cpu() - blp.view(B).cpu()).abs() <= 1e-5 + 1.2e-7 * blp.view(B).cpu().abs()).all()
    # diverse_decode(sampler=...) draws the latent noise exactly as the beam-1 call does
    torch.manual_seed(99)
    a, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), ns, 1, L_, cfg.boundary_index)
    torch.manual_seed(99)
    b, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), ns, 1, L_, cfg.boundary_index, sampler=sampling.TopKSampler(k=1))
    assert torch.equal(a.cpu(), b.cpu())
    with pytest.raises(ValueError, match="beam"):
        diverse_decode(dec, feats.cuda(), senti.cuda(), ns, 2, L_, cfg.boundary_index, sampler=sampling.TopKSampler(k=1))


@pytest.mark.parametrize("setting", [("multinomial", 0, 1.0, 1.0), ("top-k", 20, 1.0, 0.8), ("top-p", 0, 0.9, 1.2)])
def test_full_width_sampled_decode_against_the_oracle(setting):
    """Full width, each sampler: the GPU's sampled tokens, teacher-forced through oracle.decode_step with the same noise, give each
    caption's summed log-prob within 1e-4, and every sampled token lies in the oracle's kept set (margin-aware at the cut)."""
    cfg, params, _, dec = model(True)
    kind, k, p, T = setting
    nimg, ns, R, steps = 2, 10, 36, 12
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R, seed=23, steps=steps)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B)
    pred, slp = dec.sample(ctx, sent_b.cuda(), ns, steps, cfg.boundary_index, eps0.cuda(), eps.cuda(), make(*setting), seed=77)
    pred, slp = pred.cpu(), slp.cpu()
    fr = feats.unsqueeze(1).expand(nimg, ns, R, feats.size(2)).reshape(B, R, -1)
    se = sent_b.view(B, 1)
    pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
    states = zero_states(B, cfg.hidden_size, fr)
    tokens = torch.full((B,), cfg.boundary_index, dtype=torch.long)
    total = torch.zeros(B, dtype=torch.float64)
    alive = torch.ones(B, dtype=torch.bool)
    with torch.no_grad():
        for t in range(pred.size(1)):
            e = eps0 if t == 0 else eps[t - 1]
            lp, states, _, _, _ = oracle.decode_step(params, cfg, fr, tokens, states, False, se, pm, pv, e)
            for b in range(B):
                if not alive[b]:
                    assert int(pred[b, t]) == cfg.boundary_index
                    continue
                tok = int(pred[b, t])
                row = lp[b].double().numpy()
                total[b] += row[tok]
                _, ahead = S.filter_dist(row, kind, k, p, T)
                if kind == "top-k":
                    assert row[tok] >= np.sort(row)[-k] - 1e-5, (b, t)
                elif kind == "top-p" and p < 1:
                    assert ahead[tok] < p + 1e-5 or row[tok] >= row.max() - 1e-5, (b, t, ahead[tok])
            alive &= pred[:, t] != cfg.boundary_index
            tokens = pred[:, t].clone()
    assert (total - slp.double()).abs().max() < 1e-4


def test_same_seed_same_captions_other_seed_other_captions():
    cfg, _, _, dec = model(False)
    nimg, ns, R = 3, 8, 7
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R, seed=5)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(-1).cuda()
    s = sampling.TopPSampler(p=0.95, temperature=1.5)
    a = dec.sample(ctx, sent_b, ns, cfg.max_caption_length, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed=123)
    b = dec.sample(ctx, sent_b, ns, cfg.max_caption_length, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed=123)
    c = dec.sample(ctx, sent_b, ns, cfg.max_caption_length, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed=124)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])


def test_end_handling_and_early_stop():
    """@@BOUNDARY@@ made overwhelmingly likely: every row draws it at step 0, the device notes the stop (ctl[0] = 1), the call
    returns 1 column; without early stop the surplus steps emit @@BOUNDARY@@ at log-prob 0.  A bias that lets the first draw pass
    ends every row at step 1 at the latest (ssc_sample_rows ended-row handling, test_ended_rows_and_running_log_probs)."""
    cfg, _, _, dec = model(False, boundary_bias=60.0)
    nimg, ns, R = 2, 6, 7
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R, seed=9)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(-1).cuda()
    s = sampling.MultinomialSampler(temperature=1.0)
    pred, lp = dec.sample(ctx, sent_b, ns, cfg.max_caption_length, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed=1)
    assert pred.shape == (nimg * ns, 1) and (pred == cfg.boundary_index).all()
    full, lp2 = dec.sample(ctx, sent_b, ns, cfg.max_caption_length, cfg.boundary_index, eps0.cuda(), eps.cuda(), s, seed=1,
                           early_stop=False)
    assert full.shape == (nimg * ns, cfg.max_caption_length) and (full == cfg.boundary_index).all()
    assert torch.equal(lp, lp2)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sample_opts_off_paths_are_the_plain_call(variant):
    """The medium model, 3 images x 2 samples, the three samplers: ssc_decode_sample, ssc_decode_sample_opts with opts NULL, with
    four NULL fields, with bytes = sizeof(size_t), and with all three off descriptors present (rules with every control off, a kind-0
    truncation, a contrast with alpha = beta = 0) give the same predictions and the same log-probs, bit for bit.  So does an active
    min-p truncation behind `bytes` - a field that is not wholly inside the caller's size is not read -, which changes the log-probs
    once `bytes` covers it."""
    cfg, _, _, dec = medium(variant)
    nimg, ns = 3, 2
    feats, senti, eps0, eps = entry_inputs(cfg, nimg, ns, R_, 17, STEPS)
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(-1).cuda() if senti is not None else None
    ctx = dec.prepare(feats.cuda())
    lib, cfgp = dec.lib, C.byref(dec._cfg)
    Opts, full = L.SampleOpts, C.sizeof(L.SampleOpts)
    off_rules, _keep = sampling.LogitRules().desc(ns)
    off_trunc, off_contrast = sampling.Truncation().desc(), L.Contrast()
    minp = sampling.MinPTruncation(0.3).desc()
    bits = lambda x: x.view(torch.int32)

    def run(sdesc, opts, plain=False):
        o = C.byref(opts) if opts is not None else None
        if plain:
            nbytes, call = lib.ssc_decode_sample_workspace_bytes, lambda p, sd, ws: lib.ssc_decode_sample(cfgp, C.byref(p), C.byref(sd), C.byref(sdesc), *ws)
        else:
            nbytes = lambda c, sd: lib.ssc_decode_sample_opts_workspace_bytes(c, sd, o)
            call = lambda p, sd, ws: lib.ssc_decode_sample_opts(cfgp, C.byref(p), C.byref(sd), C.byref(sdesc), o, *ws)
        return dec._one_call(ctx, sent_b, ns, 1, 1, 1, STEPS, cfg.boundary_index, eps0.cuda(), eps.cuda(), True, True, (nimg * ns,), nbytes, call)

    for smp in (sampling.MultinomialSampler(1.0), sampling.TopKSampler(k=3), sampling.TopPSampler(p=0.9, temperature=1.2)):
        sdesc = smp.desc(13)
        pred0, lp0 = run(sdesc, None, plain=True)
        cases = {"opts NULL": None, "four NULL fields": Opts(bytes=full), "bytes = sizeof(size_t)": Opts(bytes=C.sizeof(C.c_size_t)),
                 "three off descriptors": Opts(bytes=full, rules=C.pointer(off_rules), trunc=C.pointer(off_trunc),
                                               contrast=C.pointer(off_contrast)),
                 "min-p behind bytes": Opts(bytes=Opts.trunc.offset, trunc=C.pointer(minp))}
        for name, opts in cases.items():
            pred, lp = run(sdesc, opts)
            assert torch.equal(pred, pred0) and torch.equal(bits(lp), bits(lp0)), (variant, smp, name)
        _, lp_cut = run(sdesc, Opts(bytes=full, trunc=C.pointer(minp)))
        assert not torch.equal(bits(lp_cut), bits(lp0)), (variant, smp)   # (the same descriptor, once it is read)


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", {seed!r}, "MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", "0.9",
                            "MODEL.SAMPLER_TEMPERATURE", "1.3", "MODEL.BEAM_SIZE", "1", "MODEL.IMAGE_FEATURE_SIZE", "64",
                            "MODEL.EMBEDDING_SIZE", "40", "MODEL.HIDDEN_SIZE", "48", "MODEL.ATTENTION_PROJECTION_SIZE", "32",
                            "MODEL.Z_SPACE", "16", "DATA.MAX_CAPTION_LENGTH", "8"])
torch.manual_seed(C.RANDOM_SEED)
m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                sampler=sampling.from_config(C.MODEL)).cuda().eval()
g = torch.Generator().manual_seed(0)
feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()   # one image, 8 latent samples
out = m(feats)["predictions"]
print(json.dumps(out.cpu().tolist()))
"""


def run_child(args, timeout=300):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_module_forward_with_a_sampler():
    outs = {}
    for seed in ("3", "3", "4"):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"), seed=seed)
        outs.setdefault(seed, []).append(json.loads(run_child(["-c", src]).strip().splitlines()[-1]))
    a, b = outs["3"]
    assert a == b                                        # same RANDOM_SEED: the same captions
    assert len(a) == 8 and all(0 < len(c) <= 8 for c in a)
    assert len({tuple(c) for c in a}) > 1                # the latent samples (and the words) differ
    assert outs["4"][0] != a


def test_module_sampler_rejects_beam_and_cbs():
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    with pytest.raises(ValueError, match="BEAM_SIZE"):
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=3, z_space=4, sampler=sampling.TopPSampler())
    m = UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=1, z_space=4, sampler=sampling.TopPSampler()).cuda().eval()
    m._use_cbs = True   # (CBS needs the frozen GloVe table; the check comes first)
    with pytest.raises(ValueError, match="USE_CBS"):
        m(torch.randn(2, 3, 16, device="cuda"), fsm=torch.ones(2, 1, 1, 50, dtype=torch.uint8))


def test_inference_script_with_a_sampler(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
                   "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
                   "  BEAM_SIZE: 5\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
                   "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n")
    caps = []
    for i in range(2):
        out = tmp_path / f"pred{i}.json"
        run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4",
                   "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--config-override",
                   "MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", "0.9", "MODEL.BEAM_SIZE", "1"])
        caps.append(json.load(open(out)))
    assert caps[0] == caps[1] and len(caps[0]) == 4 * 5
    per_image = {}
    for c in caps[0]:
        assert isinstance(c["caption"], str)
        per_image.setdefault(c["image_id"], []).append(c["caption"])
    assert any(len(set(v)) > 1 for v in per_image.values())
