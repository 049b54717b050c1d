"""GPU: scoring given captions under the model - ssc_score_rows, ssc_decode_score (DecodeEngine.score), score_captions, the module's
score_captions and the scripts' validation / likelihood re-ranking - against the float64 restatement and the teacher-forced CPU
oracle (tests/scoreref.py) and against the log-probs the decoders report for their own captions."""
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
import scoreref as SR
from gpuutil import engine_from
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.inference import score_captions
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lp_bound(ref):
    """The bound tests/test_sampling_gpu.py holds for a step log-prob and for a sum of them: 1e-5, plus one fp32 ulp of the value."""
    return 1e-5 + 1.2e-7 * np.abs(ref)


# ---- ssc_score_rows ------------------------------------------------------------------------------------------------------------
def rows_case(V, seed):
    """-> (logits (rows, V) float32 with NaN in the rows that must not be read, target, last_target, end_index)."""
    g = torch.Generator().manual_seed(seed)
    end = 0 if V == 1 else 1
    rows = 12
    x = torch.randn(rows, V, generator=g) * 3
    x[1] = 1e4 + (torch.rand(V, generator=g) * 160 - 80)              # a spread of +-80 around 1e4: the maximum must be subtracted
    x[2] = (x[2] * 2).round() / 2                                      # exact ties
    x[3, torch.randperm(V, generator=g)[: max(V // 2, 1)]] = x[3].max()   # duplicated maxima
    x[4] = -1e20
    x[4, torch.randperm(V, generator=g)[: max(V // 8, 1)]] = torch.randn(max(V // 8, 1), generator=g)
    x[5] = 1e4 - 80.0                                                  # the target far below one peak
    x[5, V - 1] = 1e4 + 80.0
    target = torch.randint(0, V, (rows,), generator=g)
    target[3] = int((x[3] == x[3].max()).nonzero()[-1])                # the LAST of the equal maxima: rank = their number - 1
    target[5] = 0
    target[6] = V - 1
    target[7] = 0
    last = torch.full((rows,), 12345, dtype=torch.int64)               # (never an index; != end: the row has not ended)
    last[8] = end                                                      # ended by its previous token
    target[9] = -1                                                     # ended by a negative target
    target[10] = V                                                     # ids that must never be used as an index
    target[11] = 2 ** 40
    x[8:] = float("nan")
    return x, target, last, end


@pytest.mark.parametrize("V", [1, 5, 90, 1027, 10000])
def test_score_rows_against_the_restatement(V):
    """The same float32 logits through the kernel and through scoreref.score_rows: lp within 1e-5 + 1.2e-7 |lp|, ranks EQUAL,
    row_lp = its start + lp in fp32, ended rows untouched and never read (NaN), ids >= V at -inf.  Two layouts: an unaligned base
    with ld = V + 3 (scalar loads) and a 16-byte aligned one with ld = V + 4 (16-byte loads where V % 4 == 0)."""
    lib = L.load()
    x, target, last, end = rows_case(V, seed=V)
    rows = x.size(0)
    ref_lp, ref_rank, _ = SR.score_rows(x.numpy(), target.numpy(), last.numpy(), end)
    live = ref_rank >= 0
    assert live.sum() == 8 and np.isneginf(ref_lp[10:]).all() and (ref_lp[8:10] == 0).all()
    assert ref_rank[3] == int((x[3] == x[3].max()).sum()) - 1 and (V == 1 or ref_lp[5] == pytest.approx(-160.0, abs=1e-3))
    xc = x.cuda()
    for off, pad in ((1, 3), (0, 4)):
        ld = V + pad
        buf = torch.full((off + rows * ld,), float("nan"), device="cuda")
        view = buf[off:].view(rows, ld)
        view[:, :V] = x.cuda()
        assert (view.data_ptr() % 16 == 0) == (off == 0)
        run = torch.full((rows,), -2.0, device="cuda")
        lp = torch.full((rows,), 7.0, device="cuda")
        rank = torch.full((rows,), 99, dtype=torch.int32, device="cuda")
        tg, la = target.cuda(), last.cuda()
        lib.ssc_score_rows(C.c_void_p(view.data_ptr()), ld, rows, V, L.ptr(tg), L.ptr(la), end, L.ptr(run), L.ptr(lp), L.ptr(rank),
                           L.stream_ptr())
        torch.cuda.synchronize()
        got = lp.cpu().double().numpy()
        print(f"V {V} layout {(off, pad)}: max |lp - ref| {np.abs(got[live] - ref_lp[live]).max():.3e}")
        assert (np.abs(got[live] - ref_lp[live]) <= lp_bound(ref_lp[live])).all(), (got, ref_lp)
        assert (got[8:10] == 0).all() and np.isneginf(got[10:]).all()
        assert (rank.cpu().numpy() == ref_rank).all(), (rank.cpu().numpy(), ref_rank)
        want_run = torch.full((rows,), -2.0) + lp.cpu()
        want_run[8:10] = -2.0
        assert torch.equal(run.cpu(), want_run)
        # optional outputs left out; no row ended by its previous token
        lp2 = torch.empty(rows, device="cuda")
        lib.ssc_score_rows(C.c_void_p(view.data_ptr()), ld, 8, V, L.ptr(tg), None, end, None, L.ptr(lp2), None, L.stream_ptr())
        assert torch.equal(lp2[:8].cpu(), lp[:8].cpu())   # (no atomics, a fixed order: the same bits)
    for bad in (dict(ld=V - 1), dict(rows=-1), dict(end=V), dict(end=-1), dict(logits=None), dict(target=None), dict(lp=None)):
        a = dict(logits=L.ptr(xc), ld=V, rows=2, end=end, target=L.ptr(tg), lp=L.ptr(lp))
        a.update(bad)
        rc = lib._raw_ssc_score_rows(a["logits"], a["ld"], a["rows"], V, a["target"], L.ptr(la), a["end"], None, a["lp"], None, L.stream_ptr())
        assert rc == -1, bad


# ---- the scoring call ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_params(kind):
    if kind == "full":
        cfg = oracle.OracleConfig(vocab_size=10000, image_feature_size=2048, embedding_size=1000, hidden_size=1200,
                                  attention_projection_size=768, z_space=128, max_caption_length=20, sentiment_vae=1,
                                  senti_prior_multip=0.5, beam_size=1)
    elif kind == "toy":
        cfg = oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32,
                                  attention_projection_size=16, z_space=8, max_caption_length=9, sentiment_vae=1,
                                  senti_prior_multip=0.5, beam_size=1)
    else:   # SENTIMENT_VAE = 2 at toy width (the pooled prior conditions the language LSTMs on 150 columns: Z_SPACE 150)
        cfg = oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32,
                                  attention_projection_size=16, z_space=150, max_caption_length=9, sentiment_vae=2, prior_std=0.9,
                                  beam_size=1)
    return cfg, oracle.init_params(cfg, seed=4)


@functools.lru_cache(maxsize=None)
def model(kind, boundary_bias=0.0):
    cfg, params = base_params(kind)
    params = {k: v.clone() for k, v in params.items()}
    params["_output_layer.bias"][cfg.boundary_index] += boundary_bias
    eng = engine_from(cfg, params)
    return cfg, params, eng, DecodeEngine(eng.dims, eng.params.c_struct, "cuda")


def inputs(cfg, nimg, rows_per_image, R, seed, steps):
    g = torch.Generator().manual_seed(seed)
    G = nimg * rows_per_image
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g)
    senti = torch.randint(-1, 2, (nimg,), generator=g).float()
    eps0 = torch.randn(G, cfg.z_space, generator=g)
    eps = torch.randn(steps - 1, G, cfg.z_space, generator=g)
    return feats, senti, eps0, eps


def per_row(senti, nimg, rpi):
    return senti.view(nimg, 1).expand(nimg, rpi).reshape(nimg * rpi)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("decoder", ["top-1", "multinomial"])
def test_scoring_a_decoders_captions_reproduces_its_log_probs(full, decoder):
    """The captions ssc_decode_sample returns, scored with C = its n_samples, N = 1 and the same noise: its own log-probs within
    1e-5 + 1.2e-7 |lp| - with the arg-max decoder (top-k, k = 1) every scored token has rank 0; with multinomial draws and a raised
    END bias the rows end at different steps.  n_tokens = the caption's words + its END, capped at the number of steps."""
    # (multinomial: END raised to about a quarter of the mass of the near-uniform start distribution of a fresh model)
    bias = 0.0 if decoder == "top-1" else round(float(np.log((10000 if full else 90) / 4)), 2)
    cfg, _, _, dec = model("full" if full else "toy", bias)
    nimg, ns, R = (8, 20, 36) if full else (3, 4, 7)
    steps, end = cfg.max_caption_length, cfg.boundary_index
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R, seed=17, steps=steps)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = per_row(senti, nimg, ns).cuda()
    smp = sampling.TopKSampler(k=1) if decoder == "top-1" else sampling.MultinomialSampler(temperature=1.0)
    pred, slp = dec.sample(ctx, sent_b, ns, steps, end, eps0.cuda(), eps.cuda(), smp, seed=5)
    n = pred.size(1)
    lps, ntok, tlp, trk = dec.score(ctx, sent_b, pred.view(nimg, ns, n), 1, end, eps0.cuda(), eps.cuda()[: n - 1] if n > 1 else None,
                                    want_tokens=True, want_ranks=True)
    slp, lps = slp.cpu().double().numpy(), lps.cpu().double().numpy()
    print(f"{decoder} full={full}: steps {n}, max |score - decoder| {np.abs(lps - slp).max():.3e}, |lp| up to {np.abs(slp).max():.1f}")
    assert (np.abs(lps - slp) <= lp_bound(slp)).all()
    is_end = (pred == end).cpu()
    words = torch.where(is_end.any(-1), is_end.float().argmax(-1), torch.full((B,), n))
    assert torch.equal(ntok.cpu().view(B).long(), (words + 1).clamp(max=n))
    trk, tlp = trk.cpu(), tlp.cpu()
    scored = torch.arange(n).view(1, n) < ntok.cpu().view(B, 1)
    assert ((trk >= 0) == scored).all() and (tlp[~scored] == 0).all() and (tlp[scored] < 0).all()
    if decoder == "top-1":
        assert (trk[scored] == 0).all()
    else:
        assert len(set(words.tolist())) > 2, words   # the rows end at different steps
        assert (trk[scored] > 0).any()
    # the caption's log-prob is the fp32 running sum of its token log-probs: half an ulp of the sum per step
    assert (np.abs(tlp.double().sum(1).numpy() - lps) <= n * 6e-8 * np.abs(lps) + 1e-6).all()


def oracle_case(kind):
    """8 images x 4 captions x 16 samples = 512 rows, 64 per image (the large-call forms of the step: attended-feature table,
    parent lists, skipped rows), L 11: random captions of 1 .. 10 words + END, one absent slot, one of 11 words (no room for END)."""
    cfg, params, _, dec = model(kind, 0.0)
    nimg, Cc, N, R, Lc = 8, 4, 16, 36 if kind == "full" else 7, 11
    g = torch.Generator().manual_seed(31)
    caps = torch.full((nimg, Cc, Lc), cfg.boundary_index, dtype=torch.int64)
    for k in range(nimg * Cc):
        n = k % 10 + 1
        caps[k // Cc, k % Cc, :n] = torch.randint(2, cfg.vocab_size, (n,), generator=g)
    caps[2, 1, 0] = -1                                                              # absent
    caps[5, 3] = torch.randint(2, cfg.vocab_size, (Lc,), generator=g)              # no room for END
    feats, senti, eps0, eps = inputs(cfg, nimg, Cc * N, R, seed=23, steps=Lc)
    obj = torch.randn(nimg, R, cfg.z_space, generator=g) * 0.3 if cfg.sentiment_vae == 2 else None
    return cfg, params, dec, caps, N, feats, (None if cfg.sentiment_vae == 2 else senti), eps0, eps, obj


@pytest.mark.parametrize("kind", ["full", "sv2"])
def test_scoring_call_against_the_oracle_on_the_large_call_forms(kind):
    """Full width (H 1200, V 10 000, R 36) and, at toy width, SENTIMENT_VAE = 2: every token's log-prob against the teacher-forced
    oracle within 1e-4, every caption's sum within 1e-4, ranks margin-aware: #{oracle lp > x + 2e-4} <= rank <= #{oracle lp >= x -
    2e-4}; n_tokens, the absent slot and the steps after a caption's end exactly."""
    cfg, params, dec, caps, N, feats, senti, eps0, eps, obj = oracle_case(kind)
    nimg, Cc, Lc = caps.shape
    G = nimg * Cc * N
    want = SR.score_captions(params, cfg, feats, senti, caps, N, eps0, eps, obj_atts=obj)
    ctx = dec.prepare(feats.cuda(), obj.cuda() if obj is not None else None)
    sent_g = per_row(senti, nimg, Cc * N).cuda() if senti is not None else None
    lps, ntok, tlp, trk = dec.score(ctx, sent_g, caps, N, cfg.boundary_index, eps0.cuda(), eps.cuda(), want_tokens=True, want_ranks=True)
    lps, tlp, trk = lps.cpu().double().numpy(), tlp.cpu().double().numpy(), trk.cpu().numpy()
    assert (ntok.cpu().numpy() == want["n_tokens"]).all() and want["n_tokens"][2, 1] == 0 and want["n_tokens"][5, 3] == Lc
    scored = want["token_rank"] >= 0
    assert ((trk >= 0) == scored).all() and (tlp[~scored] == 0).all()
    print(f"{kind}: max token |lp - oracle| {np.abs(tlp - want['token_lp']).max():.3e}, "
          f"max caption |sum - oracle| {np.abs(lps - want['log_probs']).max():.3e}")
    assert np.abs(tlp - want["token_lp"]).max() < 1e-4
    assert np.abs(lps - want["log_probs"]).max() < 1e-4
    tgt = np.clip(SR.prepare_targets(caps, N, cfg.vocab_size, cfg.boundary_index)[0], 0, None)
    for t in range(Lc):
        lp = want["step_lp"][t]
        x = lp[np.arange(G), tgt[t]][:, None]
        lo, hi = (lp > x + 2e-4).sum(1), (lp >= x - 2e-4).sum(1)
        s = scored[:, t]
        assert ((lo <= trk[:, t]) & (trk[:, t] <= hi))[s].all(), t


def test_row_order_and_sharing():
    """(C captions, N samples) in one call == every (image, caption, sample) as a call of its own with its slice of the noise, 1e-5:
    the row order is (image, caption, sample) and the rows of a call do not see each other."""
    cfg, _, _, dec = model("toy", 0.0)
    nimg, Cc, N, R, Lc = 2, 3, 2, 7, 6
    g = torch.Generator().manual_seed(3)
    caps = torch.full((nimg, Cc, Lc), cfg.boundary_index, dtype=torch.int64)
    for k in range(nimg * Cc):
        caps[k // Cc, k % Cc, : k + 1] = torch.randint(2, cfg.vocab_size, (k + 1,), generator=g)
    feats, senti, eps0, eps = inputs(cfg, nimg, Cc * N, R, seed=8, steps=Lc)
    ctx = dec.prepare(feats.cuda())
    lps, ntok, _, _ = dec.score(ctx, per_row(senti, nimg, Cc * N).cuda(), caps, N, cfg.boundary_index, eps0.cuda(), eps.cuda())
    lps = lps.cpu()
    assert ntok.cpu().view(-1).tolist() == [2, 3, 4, 5, 6, 6]
    for i in range(nimg):
        one = dec.prepare(feats[i: i + 1].cuda())
        for c in range(Cc):
            for n in range(N):
                r = (i * Cc + c) * N + n
                lp1, nt1, _, _ = dec.score(one, senti[i: i + 1].cuda(), caps[i: i + 1, c: c + 1], 1, cfg.boundary_index,
                                           eps0[r: r + 1].cuda(), eps[:, r: r + 1].cuda())
                assert abs(float(lp1[0]) - float(lps[r])) < 1e-5, (i, c, n)
                assert int(nt1[0, 0]) == int(ntok[i, c])


def test_bad_descriptions_and_ids():
    cfg, _, eng, dec = model("toy", 0.0)
    lib = L.load()
    nimg, Cc, N, R, Lc = 2, 2, 2, 7, 4
    G = nimg * Cc * N
    feats, senti, eps0, eps = inputs(cfg, nimg, Cc * N, R, seed=2, steps=Lc)
    ctx = dec.prepare(feats.cuda())
    caps = torch.randint(2, cfg.vocab_size, (nimg, Cc, Lc)).cuda()
    sent = per_row(senti, nimg, Cc * N).cuda()
    e0, e = eps0.cuda(), eps.cuda()
    out = torch.empty(G, device="cuda")
    ntok = torch.empty(nimg, Cc, dtype=torch.int32, device="cuda")

    def desc(**kw):
        d = L.ScoreDesc()
        d.nimg, d.R, d.n_captions, d.n_samples, d.max_len, d.end_index = nimg, R, Cc, N, Lc, cfg.boundary_index
        d.feats, d.imgbuf, d.sentiment, d.targets = ctx.feats.data_ptr(), ctx.buf.data_ptr(), sent.data_ptr(), caps.data_ptr()
        d.eps0, d.eps, d.log_probs, d.n_tokens = e0.data_ptr(), e.data_ptr(), out.data_ptr(), ntok.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    nbytes = lib.ssc_decode_score_workspace_bytes(C.byref(dec._cfg), C.byref(desc()))
    assert nbytes > 0 and lib.ssc_decode_score_workspace_bytes(C.byref(dec._cfg), C.byref(desc(n_samples=0))) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = eng.params.c_struct()

    def call(d, nb=nbytes):
        return lib._raw_ssc_decode_score(C.byref(dec._cfg), C.byref(p), C.byref(d), L.ptr(ws), nb, L.stream_ptr())
    assert call(desc()) == 0
    for bad in (dict(n_samples=0), dict(n_captions=-1), dict(max_len=0), dict(end_index=cfg.vocab_size), dict(end_index=-1),
                dict(targets=None), dict(eps=None), dict(eps0=None), dict(log_probs=None), dict(n_tokens=None), dict(sentiment=None),
                dict(imgbuf=None)):
        assert call(desc(**bad)) == -1, bad                       # SSC_EINVAL
    assert call(desc(), nbytes - 256) == -4                       # SSC_EWORKSPACE
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        dec.score(ctx, sent, caps, N, cfg.vocab_size, e0, e)
    # ids outside the vocabulary: ValueError on the host before anything is launched (a stand-in engine that cannot launch)
    class NoLaunch:
        dims = dec.dims
    for layout, bad in (("decoded", cfg.vocab_size), ("decoded", -3), ("padded", cfg.vocab_size), ("padded", -1)):
        c2 = caps.cpu().clone()
        c2[1, 0, 2] = bad
        with pytest.raises(ValueError, match="outside the vocabulary"):
            score_captions(NoLaunch(), feats.cuda(), senti.cuda(), c2, N, cfg.boundary_index, layout)
    with pytest.raises(ValueError, match="layout"):
        score_captions(NoLaunch(), feats.cuda(), senti.cuda(), caps.cpu(), N, cfg.boundary_index, "auto")


def test_score_captions_layouts_and_noise():
    """score_captions: the training layout (0-padded, END appended here) and the decoders' layout give the same scores for the same
    captions; the call is trimmed to the longest caption; it consumes ONE draw of the global CPU generator, and the same seed
    gives the same scores; marginal = logsumexp_n - log N; against the oracle with explicit noise."""
    cfg, params, _, dec = model("toy", 0.0)
    end = cfg.boundary_index
    nimg, Cc, N, R, L0 = 2, 3, 3, 7, 8
    g = torch.Generator().manual_seed(6)
    padded = torch.zeros(nimg, Cc, L0, dtype=torch.int64)
    for k, n in enumerate((3, 5, 0, 1, 4, 2)):   # (slot 2 is absent)
        padded[k // Cc, k % Cc, :n] = torch.randint(2, cfg.vocab_size, (n,), generator=g)
    decoded = torch.where(padded == 0, torch.full_like(padded, end), padded)
    decoded[0, 2, 0] = -1
    feats, senti, _, _ = inputs(cfg, nimg, Cc * N, R, seed=12, steps=2)
    G = nimg * Cc * N
    eps = [torch.randn(G, cfg.z_space, generator=g) for _ in range(L0 + 1)]
    a = score_captions(dec, feats.cuda(), senti.cuda(), padded, N, end, "padded", eps_steps=eps, want_tokens=True, want_ranks=True)
    b = score_captions(dec, feats.cuda(), senti.cuda(), decoded, N, end, "decoded", eps_steps=eps, want_tokens=True, want_ranks=True)
    assert a.token_lp.shape == (nimg, Cc, N, 6) and torch.equal(a.log_probs, b.log_probs) and torch.equal(a.token_rank, b.token_rank)
    assert a.n_tokens.cpu().tolist() == [[4, 6, 0], [2, 5, 3]] and torch.equal(a.n_tokens, b.n_tokens)
    assert torch.allclose(a.marginal, torch.logsumexp(a.log_probs, -1) - float(np.log(N)), atol=1e-6) and float(a.marginal[0, 2]) == 0
    tg = torch.cat([decoded, torch.full((nimg, Cc, 1), end)], -1)[..., :6]
    want = SR.score_captions(params, cfg, feats, senti, tg, N, eps[0], torch.stack(eps[1:6]))
    assert np.abs(a.log_probs.cpu().double().numpy().reshape(-1) - want["log_probs"]).max() < 1e-4
    s = a.summary()
    assert s["n_tokens"] == 20 and s["nll_per_token"] == pytest.approx(-want["log_probs"].reshape(-1, N).mean(1).sum() / 20, abs=1e-4)
    torch.manual_seed(77)
    c = score_captions(dec, feats.cuda(), senti.cuda(), padded, N, end, "padded")
    after = torch.rand(1)
    torch.manual_seed(77)
    d = score_captions(dec, feats.cuda(), senti.cuda(), padded, N, end, "padded")
    torch.manual_seed(77)
    torch.randint(0, 2 ** 62, (1,))
    assert torch.equal(c.log_probs, d.log_probs) and torch.equal(after, torch.rand(1))
    assert not torch.equal(c.log_probs, a.log_probs)


# ---- the module --------------------------------------------------------------------------------------------------------------------
def small_module(seed):
    torch.manual_seed(seed)
    return UpDownCaptioner(Vocabulary.synthetic(120), 64, 40, 48, 32, max_caption_length=8, beam_size=1, z_space=16, sentiment_vae=1,
                           senti_prior_multip=0.5, device=torch.device("cuda")).cuda()


def test_module_scores_between_optimizer_steps():
    """UpDownCaptioner.score_captions after one clip + SGD step == a freshly built model holding the updated state_dict (1e-6), and
    != the score before the step: nothing derived from the old weights is reused."""
    m = small_module(3).train()
    g = torch.Generator().manual_seed(1)
    B, R, Lc, N = 6, 5, 8, 2
    feats = torch.randn(B, R, 64, generator=g).cuda()
    caps = torch.zeros(B, Lc, dtype=torch.int64)
    for b in range(B):
        caps[b, : b + 2] = torch.randint(2, 120, (b + 2,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float().cuda()
    eps = [torch.randn(B * N, 16, generator=g) for _ in range(Lc + 1)]
    before = m.score_captions(feats, caps, sentiment=senti, n_samples=N, eps_steps=eps)
    assert before.log_probs.shape == (B, 1, N) and before.n_tokens.view(-1).tolist() == [3, 4, 5, 6, 7, 8] and m.training
    eng = m._engine()
    eng.train_step(feats, caps.cuda(), senti, torch.randn(Lc + 1, B, 16, generator=g).cuda(), lr=0.5)
    after = m.score_captions(feats, caps, sentiment=senti, n_samples=N, eps_steps=eps)
    fresh = small_module(99)
    fresh.load_state_dict(m.state_dict())
    want = fresh.eval().score_captions(feats, caps, sentiment=senti, n_samples=N, eps_steps=eps)
    assert (after.log_probs - want.log_probs).abs().max() < 1e-6
    assert (after.log_probs - before.log_probs).abs().min() > 0
    assert m.score_captions(feats, caps, sentiment=senti).log_probs.shape == (B, 1, 1)   # (a model built without a config: 1 sample)


# ---- the scripts -------------------------------------------------------------------------------------------------------------------
YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n  IMAGE_FEATURE_SIZE: 64\n"
        "  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n  BEAM_SIZE: 3\n  USE_CBS: False\n"
        "  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n  SIMPLE_VAE: False\n"
        "  N_Z_SAMPLES: 4\nOPTIM:\n  BATCH_SIZE: 8\n  NUM_ITERATIONS: 5\n  BEFORE_UPDATE_DECODER_EVERY: 2\n"
        "  EPOCH_START_DECODER_TRAINING: 3\n")


def run_child(args):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout[-2000:] + r.stderr[-4000:]


def test_train_script_validation_does_not_change_training(tmp_path):
    """scripts/train.py --val-tensors: the four val_* scalars at every --val-every-th iteration and at the last one; the training
    scalars (all but the wall-clock field) and the final checkpoint are those of the same run without validation, bit for bit;
    more than one rank is refused."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    g = torch.Generator().manual_seed(5)
    caps = torch.zeros(10, 8, dtype=torch.int64)
    for b in range(10):
        caps[b, : b % 7 + 1] = torch.randint(2, 150, (b % 7 + 1,), generator=g)
    val = tmp_path / "val.pt"
    torch.save({"image_features": torch.randn(10, 5, 64, generator=g), "caption_tokens": caps,
                "sentiment": torch.randint(-1, 2, (10, 1), generator=g).float()}, val)
    base = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--checkpoint-every", "5"]
    runs = {"plain": [], "val": ["--val-tensors", str(val), "--val-every", "2", "--val-samples", "3", "--val-images", "7"]}
    logs = {}
    for name, extra in runs.items():
        rc, out = run_child(base + extra + ["--serialization-dir", str(tmp_path / name)])
        assert rc == 0, out
        logs[name] = [json.loads(x) for x in open(tmp_path / name / "scalars.jsonl")]
    vals = [r for r in logs["val"] if "val_nll_per_token" in r]
    assert [r["iteration"] for r in vals] == [2, 4, 5]
    for r in vals:
        assert set(r) == {"iteration", "val_nll_per_token", "val_perplexity", "val_marginal_nll_per_token", "val_top1"}
        assert r["val_perplexity"] == pytest.approx(np.exp(r["val_nll_per_token"]), rel=1e-9) and 0 <= r["val_top1"] <= 1
        assert 0 < r["val_marginal_nll_per_token"] <= r["val_nll_per_token"] + 1e-9
    strip = lambda rows: [{k: v for k, v in r.items() if k != "elapsed_s"} for r in rows if "val_nll_per_token" not in r]
    assert strip(logs["val"]) == strip(logs["plain"]) and len(strip(logs["plain"])) == 5
    a = torch.load(tmp_path / "plain" / "checkpoint_5.pth", weights_only=True)
    b = torch.load(tmp_path / "val" / "checkpoint_5.pth", weights_only=True)
    assert set(a["model"]) == set(b["model"]) and all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    for k, st in a["optimizer"]["state"].items():
        assert torch.equal(st["momentum_buffer"], b["optimizer"]["state"][k]["momentum_buffer"])
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable] + base + runs["val"] + ["--serialization-dir", str(tmp_path / "w2")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "one GPU only" in r.stderr


def test_inference_script_likelihood_reranking(tmp_path):
    """scripts/inference.py --likelihood-samples 3 --likelihood-output: one entry per image whose pick holds the largest of the listed
    marginals (and the per-token pick the largest marginal / n_tokens); the same RANDOM_SEED gives the same file."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    files = []
    for i in range(2):
        out, lik = tmp_path / f"pred{i}.json", tmp_path / f"lik{i}.json"
        rc, log = run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "5",
                             "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--images-per-call", "3",
                             "--likelihood-samples", "3", "--likelihood-output", str(lik)])
        assert rc == 0, log
        files.append((json.load(open(out)), open(lik).read()))
    assert files[0][1] == files[1][1]
    preds, lik = files[0][0], json.loads(files[0][1])
    assert len(lik) == 5 and [e["image_id"] for e in lik] == sorted({p["image_id"] for p in preds})
    for e in lik:
        caps = [p["caption"] for p in preds if p["image_id"] == e["image_id"]]
        m, n = np.array(e["marginal"]), np.array(e["n_tokens"])
        assert len(caps) == len(m) == len(n) == 4 and (m < 0).all() and (n >= 1).all()
        assert e["pick"] == int(m.argmax()) and e["caption"] == caps[e["pick"]]
        assert e["pick_per_token"] == int((m / n).argmax()) and e["caption_per_token"] == caps[e["pick_per_token"]]
        assert all(len(c.split()) in (k - 1, k) for c, k in zip(caps, n) if c)   # words + END (no END: all 8 steps)
