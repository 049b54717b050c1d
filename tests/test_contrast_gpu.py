"""GPU: contrastive decoding for the word samplers (include/ssc.h: ssc_contrast_rows, ssc_contrast).  The row kernel against the
float64 restatement (tests/contrastref.py) on inputs the restatement calls decidable; the sampled decode with an amateur stream
(ssc_sample_opts.contrast, DecodeEngine.sample(contrast=)) against the same decode driven step by step over two DecodeEngine.step
streams, against the call without it and against the CPU oracle; what the plausibility cut does to the draws; diverse_decode, the
module and scripts/inference.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import contrastref as R
import oracle
from gpuutil import engine_from
from oracle.seqcvae_oracle import cell_step, embed, output_logits, zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.contrast import Contrast, amateur_features
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.inference import diverse_decode
from ssc_runtime.prefix import DecodePrefix
from test_attention_trace_gpu import R_, SEEDS, STEPS, VARIANTS, entry_inputs, medium, medium_params
from test_latent_guide_gpu import bits, make_guide, step_prior
from test_logit_rules_gpu import GUARD, SENTINEL, decode_inputs, padded, placed, yardstick_rules
from test_sampling_gpu import inputs as wide_inputs
from test_sampling_gpu import run_child
from test_truncation_gpu import NIMG, NS, SAMPLERS, guarded, padded_stats, sharp_wide_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = R.END
LP_TOL = 1e-4           # the project's parity tolerance of a log-prob
DIVERGENCE_TOL = 1e-4   # ... and of a row statistic (test_truncation_gpu.ENTROPY_TOL)


def value_tol(alpha):
    """the edit scales lp_e by 1 + alpha and lp_a by alpha, each within LP_TOL"""
    return (1 + 2 * alpha) * LP_TOL


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def run_contrast(view_e, ld, view_a, lda, rows, V, alpha, beta, last_d, kept=None, div=None):
    L.load().ssc_contrast_rows(view_e.data_ptr(), ld, view_a.data_ptr() if view_a is not None else None, lda, rows, V, alpha, beta,
                               L.ptr(last_d), END, L.ptr(kept), L.ptr(div), L.stream_ptr())
    torch.cuda.synchronize()


def device_log_softmax(x, V):
    """ssc_log_softmax of the first V columns of x (rows, ld) float32 numpy -> (rows, V) tensor on the device"""
    x_d = torch.from_numpy(np.ascontiguousarray(x[:, :V])).cuda()
    out = torch.empty_like(x_d)
    L.load().ssc_log_softmax(L.ptr(x_d), V, x_d.size(0), V, L.ptr(out), V, L.stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("V,ld,off,lda,offa", R.SHAPES)
def test_rows_kernel_against_the_restatement(V, ld, off, lda, offa):
    """Per alpha in {0, 0.5, 1, 2} and beta in {0, 0.1, 0.5}: the restatement finds no undecidable token in the inputs (asserted
    first); then the kept set is EQUAL to its own, the finite values are within (1 + 2 alpha) 1e-4 of it, `kept` is exact and
    `divergence` within 1e-4.  Exact: with alpha = 0, and in the row whose amateur equals its expert at every alpha, the kept
    entries are bit-equal to ssc_log_softmax(x_e); with beta = 0 nothing is dropped; the amateur's buffer, the NaN pad columns, the
    guard words of all four buffers and the ended row (NaN) are untouched; two calls are bit-equal; NULL outputs change nothing; a
    NULL amateur at alpha = 0 gives the bits of the call with one; both knobs 0 change nothing at all.  V = 1024: the 16-byte path
    and the scalar paths (either row misaligned) give the same bits."""
    xe, xa, last = R.rows_case(V, ld, lda, R.row_seed(V))
    live = [r for r in range(R.N_ROWS) if last[r] != END]
    lsm = device_log_softmax(xe[live], V)
    last_d = torch.from_numpy(last).cuda()
    flat_a, view_a = placed(xa, offa)
    before_a = flat_a.clone()
    flat, view = placed(xe, off)
    before = flat.clone()
    kept_buf, kept = guarded(R.N_ROWS, torch.int32, -99)
    div_buf, div = guarded(R.N_ROWS, torch.float32, SENTINEL)
    lo, hi = GUARD + off, GUARD + off + xe.size
    for beta in R.BETAS:
        for alpha in R.ALPHAS:
            tag = (V, ld, off, lda, offa, alpha, beta)
            want, kept_ref, kl_ref, _, und = R.edit_rows(xe, xa, V, alpha, beta, last, END)
            assert und == [], (tag, und[:5])
            outs = []
            for _ in range(2):   # two calls on equal inputs
                flat.copy_(before)
                kept_buf.fill_(-99)
                div_buf.fill_(SENTINEL)
                run_contrast(view, ld, view_a, lda, R.N_ROWS, V, alpha, beta, last_d, kept, div)
                outs.append((flat.clone(), kept_buf.clone(), div_buf.clone()))
            for a, b in zip(outs[0], outs[1]):
                assert torch.equal(bits(a), bits(b)), tag
            got_flat, kept_got, div_got = outs[0]
            assert torch.equal(bits(flat_a), bits(before_a)), tag                       # the amateur and its guards
            if alpha == 0 and beta == 0:   # off: no launch, nothing written
                assert torch.equal(bits(got_flat), bits(before)), tag
                assert bool((kept_got == -99).all()) and bool((div_got == SENTINEL).all()), tag
                continue
            assert torch.equal(bits(got_flat[:lo]), bits(before[:lo])) and torch.equal(bits(got_flat[hi:]), bits(before[hi:])), tag
            assert bool((kept_got[:GUARD] == -99).all()) and bool((kept_got[-GUARD:] == -99).all()), tag
            assert bool((div_got[:GUARD] == SENTINEL).all()) and bool((div_got[-GUARD:] == SENTINEL).all()), tag
            got_d = got_flat[lo:hi].view(R.N_ROWS, ld)
            b4 = before[lo:hi].view(R.N_ROWS, ld)
            assert torch.equal(bits(got_d[:, V:]), bits(b4[:, V:])), tag                # the pad columns
            assert torch.equal(bits(got_d[4]), bits(b4[4])), tag                        # the ended row
            got = got_d.cpu().numpy().astype(np.float64)
            fin_got, fin_want = np.isfinite(got[live, :V]), np.isfinite(want[live, :V])
            assert (fin_got == fin_want).all(), (tag, np.argwhere(fin_got != fin_want)[:5].tolist())
            assert not np.isnan(got[live, :V]).any() and (got[live, :V][~fin_got] == -np.inf).all(), tag
            err = np.abs(got[live, :V][fin_got] - want[live, :V][fin_want]).max()
            kl_got = div_got[GUARD: GUARD + R.N_ROWS].cpu().numpy().astype(np.float64)
            kl_err = np.abs(kl_got - kl_ref).max()
            print(f"{tag}: kept {kept_got[GUARD: GUARD + R.N_ROWS].tolist()}, max |y - float64| {err:.2e} (bound {value_tol(alpha):.1e}), "
                  f"max |KL - float64| {kl_err:.2e}")
            assert err <= value_tol(alpha), (tag, err)
            assert kept_got[GUARD: GUARD + R.N_ROWS].tolist() == kept_ref.tolist(), tag
            assert kl_err <= DIVERGENCE_TOL, (tag, kl_got, kl_ref)
            assert kl_got[2] == 0.0 and kl_got[4] == 0.0 and kept_got[GUARD + 4] == 0, tag
            if beta == 0:
                assert fin_got.all(), tag
            keep_d = torch.isfinite(got_d[live][:, :V])
            same = [live.index(2)] if alpha != 0 else list(range(len(live)))   # rows whose kept entries are the expert's log-probs
            for i in same:
                assert torch.equal(bits(got_d[live[i], :V][keep_d[i]]), bits(lsm[i][keep_d[i]])), (tag, i)
            flat.copy_(before)
            run_contrast(view, ld, view_a, lda, R.N_ROWS, V, alpha, beta, last_d)    # no statistics asked for
            assert torch.equal(bits(flat), bits(got_flat)), tag
            if alpha == 0:   # the plausibility cut alone takes no amateur
                flat.copy_(before)
                div_buf.fill_(SENTINEL)
                run_contrast(view, ld, None, 0, R.N_ROWS, V, alpha, beta, last_d, kept, div)
                assert torch.equal(bits(flat), bits(got_flat)) and torch.equal(kept_buf, kept_got), tag
                assert bool((div == 0).all()), tag
            if V == 1024:   # both rows on a 16-byte boundary: the vector path
                xa0 = np.full((R.N_ROWS, 1024), np.nan, dtype=np.float32)
                xa0[:, :V] = xa[:, :V]
                xe0 = np.full((R.N_ROWS, 1024), np.nan, dtype=np.float32)
                xe0[:, :V] = xe[:, :V]
                _, va0 = placed(xa0, 0)
                _, ve0 = placed(xe0, 0)
                run_contrast(ve0, 1024, va0, 1024, R.N_ROWS, V, alpha, beta, last_d, kept, div)
                assert torch.equal(bits(ve0[live]), bits(got_d[live][:, :V])), tag
                assert torch.equal(kept_buf, kept_got) and torch.equal(bits(div_buf), bits(div_got)), tag


# ---- the decode ---------------------------------------------------------------------------------------------------------------------------
ALPHA, BETA = 1.0, 0.1
AMATEURS = ("features", "params", "zero-noise", "sentiment", "cut-only")


@functools.lru_cache(maxsize=None)
def second_engine(variant):
    """Another parameter set of the variant's configuration: a checkpoint of the same dims, sharpened as the first."""
    cfg, params = medium_params(variant)
    other = {k: v.clone() for k, v in oracle.init_params(cfg, seed=SEEDS[variant][0] + 7).items()}
    other["_updown_cell._butd_attention._attention_layer.weight"] *= 8.0
    if not VARIANTS[variant][0]:
        other["_output_layer.weight"] *= 8.0
        other["_output_layer.bias"][cfg.boundary_index] += 1.2
    eng = engine_from(cfg, other)
    dec = DecodeEngine(eng.dims, eng.params.c_struct, "cuda")
    if VARIANTS[variant][2]:
        dec._cfg.gemm_mode = VARIANTS[variant][2]
    return other, eng, dec


def make_contrast(kind, variant, alpha=ALPHA, beta=BETA, **kw):
    if kind == "features":
        return Contrast(alpha, beta, features="mean", **kw)
    if kind == "params":
        return Contrast(alpha, beta, engine=second_engine(variant)[2], **kw)
    if kind == "zero-noise":
        return Contrast(alpha, beta, latent="mean", **kw)
    if kind == "sentiment":
        return Contrast(alpha, beta, sentiment=-1.0, **kw)
    return Contrast(0.0, 0.5, **kw)


class ForcedOff(Contrast):
    """A contrast with both knobs at 0 that DecodeEngine.sample hands to ssc_decode_sample_opts (as its contrast) all the same"""
    active = True


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_off_path_is_the_call_without_a_contrast(variant):
    """contrast=None, an inactive Contrast and a descriptor with both knobs at 0 handed to ssc_decode_sample_opts itself give
    the predictions and the log-probs of the call without the argument, bit for bit - alone, under active logit rules and under a
    truncation."""
    cfg, _, _, dec = medium(variant)
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    ctx = dec.prepare(feats)
    rules = yardstick_rules(cfg.vocab_size, NIMG)
    for name, smp in SAMPLERS.items():
        args = (ctx, sent_b, NS, STEPS, cfg.boundary_index, eps0, eps, smp, 13)
        for kw in (dict(), dict(logit_rules=rules), dict(truncation=sampling.MinPTruncation(0.05))):
            pred0, lp0 = dec.sample(*args, **kw)
            for c in (None, Contrast(0.0, 0.0), ForcedOff(0.0, 0.0, features="mean")):
                pred, lp = dec.sample(*args, contrast=c, **kw)
                assert torch.equal(pred, pred0) and torch.equal(bits(lp), bits(lp0)), (variant, name, c, list(kw))


def amateur_of(contrast, dec, ctx, sent_b, eps0, eps):
    """-> what the amateur stream of `contrast` steps with: (engine, image context, sentiment (B) or None, eps0, eps)"""
    a_dec = contrast.engine if contrast.engine is not None else dec
    a_ctx = contrast.ctx if contrast.ctx is not None else ctx
    a_sent = sent_b
    if contrast.sentiment is not None and sent_b is not None:
        a_sent = torch.full_like(sent_b, float(contrast.sentiment))
    if contrast.latent == "mean":
        eps0, eps = torch.zeros_like(eps0), torch.zeros_like(eps)
    return a_dec, a_ctx, a_sent, eps0, eps


def start_states(dec, start, B, V, end):
    tokens = start.tokens.clone()
    tokens[(tokens < 0) | (tokens >= V)] = end
    state = dec.zero_states(B)
    state.update(h1=start.h1, c1=start.c1, h_decoder=start.hd, c_decoder=start.cd)
    return tokens, state


def drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, sampler, seed, contrast=None, trunc=None, rules=None, guide=None, start=None,
          probe_beta=None, forced=None):
    """The sampled decode driven from Python: per step DecodeEngine.step of the expert, DecodeEngine.step of the amateur (fed the same
    words, on its own states), ssc_contrast_rows, ssc_logit_rules_rows, ssc_truncate_rows, ssc_sample_rows.  probe_beta: the
    plausibility cut applied to a COPY of every step's expert logits - was the step's token inside the expert's plausible set?
    forced (B, steps): the tokens are given instead of drawn.
    -> (tokens (B, steps), log-probs (B), kept (B, steps), divergence (B, steps), inside (B, steps))"""
    lib = L.load()
    V = dec.dims.V
    T = float(sampler.temperature)
    sdesc = sampler.desc(seed)
    rd = rules.desc(ns) if rules is not None else None
    run = torch.zeros(B, device="cuda")
    hist = torch.full((steps, B), -1, dtype=torch.int64, device="cuda")
    kept = torch.zeros(steps, B, dtype=torch.int32, device="cuda")
    div = torch.zeros(steps, B, device="cuda")
    inside = torch.ones(steps, B, dtype=torch.bool, device="cuda")
    two = contrast is not None and contrast.alpha != 0
    if start is None:
        tokens, state = torch.full((B,), end, dtype=torch.int64, device="cuda"), None
        state_a = None
    else:
        tokens, state = start_states(dec, start, B, V, end)
        state_a = start_states(dec, contrast.start, B, V, end)[1] if two else None
    if two:
        a_dec, a_ctx, a_sent, a_eps0, a_eps = amateur_of(contrast, dec, ctx, sent_b, eps0, eps)
        a_guide = guide if contrast.guide == "shared" else None
    last = None
    for t in range(steps):
        pm, pv = step_prior(guide, t, B, 1, sent_b, dec.dims)
        logits, state, _ = dec.step(ctx, tokens, state, sent_b, eps0 if t == 0 else eps[t - 1], raw_logits=True, prior_mean=pm, prior_var=pv)
        copy = None
        if probe_beta is not None:
            copy = logits.clone()
            lib.ssc_contrast_rows(L.ptr(copy), V, None, 0, B, V, 0.0, probe_beta, L.ptr(last), end, None, None, L.stream_ptr())
        if contrast is not None:
            logits_a = None
            if two:
                pm_a, pv_a = step_prior(a_guide, t, B, 1, a_sent, dec.dims)
                logits_a, state_a, _ = a_dec.step(a_ctx, tokens, state_a, a_sent, a_eps0 if t == 0 else a_eps[t - 1], raw_logits=True,
                                                  prior_mean=pm_a, prior_var=pv_a)
            lib.ssc_contrast_rows(L.ptr(logits), V, L.ptr(logits_a), V, B, V, contrast.alpha, contrast.beta, L.ptr(last), end,
                                  L.ptr(kept[t]), L.ptr(div[t]), L.stream_ptr())
        if rd is not None:
            lib.ssc_logit_rules_rows(L.ptr(logits), V, B, V, C.byref(rd[0]), L.ptr(hist), B, t, end, L.stream_ptr())
        if trunc is not None:
            td = trunc.desc(None, None)
            lib.ssc_truncate_rows(L.ptr(logits), V, B, V, C.byref(td), T, L.ptr(last), end, L.stream_ptr())
        if forced is None:
            slp = torch.empty(B, device="cuda")
            lib.ssc_sample_rows(L.ptr(logits), V, B, V, C.byref(sdesc), None, t, L.ptr(last), L.ptr(run), end, L.ptr(hist[t]), L.ptr(slp), None,
                                L.stream_ptr())
        else:
            hist[t] = forced[:, t]
        if copy is not None:
            inside[t] = torch.isfinite(copy.gather(1, hist[t].view(B, 1)).view(B))
            if last is not None:
                inside[t] |= last == end
        last = tokens = hist[t]
    return hist.t().contiguous(), run, kept.t().contiguous(), div.t().contiguous(), inside.t().contiguous()


@pytest.mark.parametrize("amateur", AMATEURS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_contrastive_decode_against_the_stepwise_driver(variant, amateur):
    """The one call gives the tokens, the log-probs and both statistics blocks of the same decode driven step by step over two
    DecodeEngine.step streams, bit for bit: each sampler; the amateur by other features, by another parameter set, by zero noise, by
    another sentiment, and the plausibility cut alone; alone with skip_dead / early_stop on and off and an attention trace, with
    active logit rules under a latent guide in both guide modes, and with rules and a truncation from a prefix start state."""
    cfg, _, _, dec = medium(variant)
    end, V = cfg.boundary_index, cfg.vocab_size
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    B = NIMG * NS
    rules = yardstick_rules(V, NIMG)
    guide = make_guide("var+len", B, cfg.z_space, STEPS, 5)
    tr = sampling.MinPTruncation(0.05)
    g = torch.Generator().manual_seed(3)
    prefix = torch.full((NIMG, 2), -1, dtype=torch.int64)
    prefix[1, :1] = torch.randint(2, V, (1,), generator=g)
    prefix[2, :2] = torch.randint(2, V, (2,), generator=g)
    peps = torch.randn(2, B, cfg.z_space, generator=g).cuda()
    flags = ((True, True, False), (False, False, False), (True, False, True), (False, True, False))
    moved = False
    for name, smp in SAMPLERS.items():
        for what, kw, gmode, runs in (("alone", dict(), "shared", flags),
                                      ("rules+guide", dict(rules=rules, guide=guide), "shared", flags[:2]),
                                      ("rules+guide-prior", dict(rules=rules, guide=guide), "prior", flags[:1]),
                                      ("rules+trunc+prefix", dict(rules=rules, trunc=tr, start=True), "shared", flags[:1])):
            ctx = dec.prepare(feats)
            c = make_contrast(amateur, variant, guide=gmode).prepare(dec, ctx.feats)
            dkw = dict(kw)
            if dkw.get("start"):
                dkw["start"] = dec.prime(ctx, sent_b, NS, DecodePrefix(prefix), end, peps)
                if c.steps_amateur:
                    a_dec, a_ctx, a_sent, _, _ = amateur_of(c, dec, ctx, sent_b, eps0, eps)
                    c.start = a_dec.prime(a_ctx, a_sent, NS, DecodePrefix(prefix), end, peps)
            want = drive(dec, ctx, sent_b, B, NS, STEPS, end, eps0, eps, smp, 13, contrast=c, **dkw)
            plain = drive(dec, ctx, sent_b, B, NS, STEPS, end, eps0, eps, smp, 13, **dkw)
            moved |= not torch.equal(want[0], plain[0])
            skw = {{"rules": "logit_rules", "trunc": "truncation"}.get(k, k): v for k, v in dkw.items()}
            for skip_dead, early_stop, attention in runs:
                out = dec.sample(ctx, sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=early_stop, attention=attention,
                                 skip_dead=skip_dead, contrast=c, contrast_stats=True, **skw)
                pred, lp, (kept, div) = out[0], out[1], out[-1]
                tag = (variant, amateur, name, what, skip_dead, early_stop, attention)
                assert kept.shape == div.shape == pred.shape, tag
                assert torch.equal(padded(pred, STEPS, end), want[0]), tag
                assert torch.equal(bits(lp), bits(want[1])), (tag, (lp - want[1]).abs().max().item())
                assert torch.equal(padded_stats(kept, STEPS), want[2]), tag
                assert torch.equal(bits(padded_stats(div, STEPS)), bits(want[3])), tag
                if attention:
                    assert dec.attention(out[2]).top_region.shape == (B, STEPS)
            live = want[2] > 0
            assert bool(live[:, 0].all()) and bool((want[2][live] <= V).all()) and bool((want[3][~live] == 0).all())
            # (another sentiment: -1 is what some images have anyway, and a model without a sentiment reads none - such streams are
            # equal, divergence 0, unless the amateur leaves the guide)
            equal = not c.steps_amateur or (amateur == "sentiment" and sent_b is None and gmode == "shared")
            if equal:
                assert bool((want[3] == 0).all())
            elif amateur != "sentiment":
                assert bool((want[3][live] > 0).all()), "an amateur that differs from the expert has a positive divergence"
            else:
                assert bool((want[3][live] > 0).any()) and bool((want[3][live] >= 0).all())
            if not VARIANTS[variant][0]:   # (the tied heads are not sharpened: nearly uniform rows, every word plausible)
                assert bool((want[2][live] < V).any()), "the plausibility cut dropped nothing"
    if not VARIANTS[variant][0]:
        assert moved, "the contrast changed no caption"


@pytest.mark.parametrize("amateur", ["zero-noise", "features"])
def test_contrastive_decode_with_the_attended_feature_table(amateur):
    """2 images x 256 samples - 512 rows, 256 per image, the smallest extents at which the steps of both streams take the
    attended-feature-table form: the one call against the stepwise driver, bit for bit, for an amateur that shares the expert's
    image context (its own table decision forms the shared table once more) and for one with a context of its own."""
    cfg, _, _, dec = medium("untied-sv1")
    end = cfg.boundary_index
    nimg, ns = 2, 256
    B = nimg * ns
    feats, sent_b, eps0, eps = decode_inputs(cfg, seed=23, nimg=nimg, ns=ns)
    smp = SAMPLERS["multinomial"]
    ctx = dec.prepare(feats)
    c = make_contrast(amateur, "untied-sv1").prepare(dec, ctx.feats)
    want = drive(dec, ctx, sent_b, B, ns, STEPS, end, eps0, eps, smp, 13, contrast=c)
    assert ctx.att_table_ready and (c.ctx is None or c.ctx.att_table_ready)      # the stepwise streams took the table form
    for skip_dead in (True, False):
        pred, lp, (kept, div) = dec.sample(ctx, sent_b, ns, STEPS, end, eps0, eps, smp, 13, early_stop=False, skip_dead=skip_dead, contrast=c,
                                           contrast_stats=True)
        assert torch.equal(pred, want[0]) and torch.equal(bits(lp), bits(want[1])), (amateur, skip_dead)
        assert torch.equal(kept, want[2]) and torch.equal(bits(div), bits(want[3])), (amateur, skip_dead)
    assert bool((want[3][want[2] > 0] > 0).all())


# ---- against the CPU oracle -----------------------------------------------------------------------------------------------------------------
def oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, smp, contrast, a_params, a_feats, seed=77):
    """The device's tokens teacher-forced through the oracle's decode step under both contexts - the expert's (params, feats) and the
    amateur's (a_params, a_feats) - with the same noise; the restatement's edit on the oracle's two logits rows.
    -> (max over the captions of |summed edited log-prob, oracle - device|, undecidable tokens over all live rows, device tokens
    among them, max |divergence, oracle - device|).  Asserts that every other device token lies in the oracle-side kept set."""
    B = nimg * ns
    end = cfg.boundary_index
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B) if senti is not None else None
    ctx = dec.prepare(feats.cuda())
    contrast.prepare(dec, ctx.feats)
    pred, slp, (_, div) = dec.sample(ctx, sent_b.cuda() if sent_b is not None else None, ns, steps, end, eps0.cuda(), eps.cuda(), smp, seed,
                                     early_stop=False, contrast=contrast, contrast_stats=True)
    pred, slp, div = pred.cpu(), slp.cpu(), div.cpu().double().numpy()
    se = sent_b.view(B, 1) if sent_b is not None else None
    streams = []
    for p, f in ((params, feats), (a_params, a_feats)):
        fr = f.unsqueeze(1).expand(nimg, ns, f.size(1), f.size(2)).reshape(B, f.size(1), -1)
        pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
        streams.append([p, fr, pm, pv, zero_states(B, cfg.hidden_size, fr)])
    tokens = torch.full((B,), end, dtype=torch.long)
    total = np.zeros(B)
    alive = np.ones(B, dtype=bool)
    undecidable = exempt = 0
    kl_err = 0.0
    alpha, beta = contrast.alpha, contrast.beta
    with torch.no_grad():
        for t in range(steps):
            e = eps0 if t == 0 else eps[t - 1]
            rows = []
            for s in streams:
                p, fr, pm, pv, states = s
                h_dec, s[4], _, _, _, _ = cell_step(p, cfg, fr, embed(p, cfg, tokens), states, False, se, pm, pv, e, None, None, True)
                rows.append(output_logits(p, cfg, h_dec).float().numpy())
            for b in range(B):
                tok = int(pred[b, t])
                if not alive[b]:
                    assert tok == end
                    continue
                c = R.contrast_row(rows[0][b], rows[1][b], alpha, beta)
                kl_err = max(kl_err, abs(c.kl - div[b, t]))
                undecidable += len(c.undecidable)
                if tok in c.undecidable:
                    exempt += 1
                    continue
                assert c.kept[tok], (b, t, tok)
                total[b] += R.log_softmax(c.y)[tok]
            alive &= (pred[:, t] != end).numpy()
            tokens = pred[:, t].clone()
    return float(np.abs(total - slp.double().numpy()).max()), undecidable, exempt, kl_err


ORACLE_TOL = (1 + 2 * ALPHA) * 1e-4   # test_truncation_gpu.ORACLE_TOL times the factor by which the edit scales the streams' errors
# (variant, amateur) -> the seed of the inputs: one at which the restatement finds no undecidable token on the oracle's logits
ORACLE_SEEDS = {("untied-sv1", "features"): 18, ("untied-sv0-fp32", "params"): 18}   # (seed 17, the default: one token within the band there)
ORACLE_VARIANTS = ("untied-sv1", "untied-sv0-fp32")   # (the tied heads are not sharpened: nearly uniform rows)


@pytest.mark.parametrize("amateur", ["features", "params"])
@pytest.mark.parametrize("variant", ORACLE_VARIANTS)
def test_contrastive_decode_against_the_oracle(variant, amateur):
    """Toy width (the medium model), multinomial, alpha = 1, beta = 0.1, the amateur by features and by parameter set: the
    restatement finds no undecidable token on the oracle's logits for the chosen seeds (asserted), every device token lies in the
    oracle-side kept set (exact) and each caption's summed edited log-prob is within 3e-4 of the oracle's."""
    cfg, params = medium_params(variant)
    _, _, _, dec = medium(variant)
    seed = ORACLE_SEEDS.get((variant, amateur), 17)
    feats, senti, eps0, eps = entry_inputs(cfg, NIMG, NS, R_, seed, STEPS)
    a_params = second_engine(variant)[0] if amateur == "params" else params
    a_feats = amateur_features(feats, "mean") if amateur == "features" else feats
    c = make_contrast(amateur, variant)
    worst, und, exempt, kl_err = oracle_check(cfg, params, dec, feats, senti, NIMG, NS, STEPS, eps0, eps, SAMPLERS["multinomial"], c,
                                              a_params, a_feats)
    print(f"{variant} {amateur} seed {seed}: max |summed edited log-prob, oracle - device| {worst:.3e}, undecidable {und} (drawn {exempt}), "
          f"max |divergence, oracle - device| {kl_err:.3e}")
    assert und == 0 and exempt == 0, (variant, amateur, seed, und, exempt)
    assert worst <= ORACLE_TOL, (variant, amateur, worst)


WIDE_SEED = 359   # (test_truncation_gpu.WIDE_SEED; the restatement finds no undecidable token in the 36 rows of either stream's logits)


def test_full_width_contrastive_decode_against_the_oracle():
    """Full width on the sharpened model (H 1200, V 10 000, R 36; 2 images x 3 samples, 6 steps), the amateur by mean features: the
    same three checks."""
    cfg, params, _, dec = sharp_wide_model()
    nimg, ns, R36, steps = 2, 3, 36, 6
    feats, senti, eps0, eps = wide_inputs(cfg, nimg, ns, R36, seed=WIDE_SEED, steps=steps)
    c = Contrast(ALPHA, BETA, features="mean")
    worst, und, exempt, kl_err = oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, sampling.MultinomialSampler(1.0), c,
                                              params, amateur_features(feats, "mean"))
    print(f"full width seed {WIDE_SEED}: max |summed edited log-prob, oracle - device| {worst:.3e}, undecidable {und} (drawn {exempt}), "
          f"max |divergence, oracle - device| {kl_err:.3e}")
    assert und == 0 and exempt == 0, (und, exempt)
    assert worst <= ORACLE_TOL, worst


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_plausibility_cut_confines_the_draws_where_the_plain_decode_leaves_the_set():
    """Multinomial sampling on the sharpened full-width model with a fixed seed: the call without a contrast draws at least one token
    outside its step's plausible set of the expert (beta = 0.5; asserted, so that the check is not vacuous), the contrastive call
    (alpha = 1 against mean features) none."""
    cfg, _, _, dec = sharp_wide_model()
    end = cfg.boundary_index
    nimg, ns, steps = 2, 8, 8
    B = nimg * ns
    feats, senti, eps0, eps = wide_inputs(cfg, nimg, ns, 36, seed=29, steps=steps)
    feats, eps0, eps = feats.cuda(), eps0.cuda(), eps.cuda()
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    smp = sampling.MultinomialSampler(1.0)
    ctx = dec.prepare(feats)
    args = (ctx, sent_b, ns, steps, end, eps0, eps, smp, 41)
    plain, _ = dec.sample(*args, early_stop=False)
    tok, _, _, _, inside = drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, smp, 41, probe_beta=0.5)
    assert torch.equal(tok, plain)
    outside = int((~inside).sum())
    print(f"plain call: {outside} of {int((plain != end).sum()) + B} drawn tokens lie outside the expert's plausible set")
    assert outside >= 1
    c = Contrast(1.0, 0.5, features="mean").prepare(dec, ctx.feats)
    cut, lp, (kept, div) = dec.sample(*args, early_stop=False, contrast=c, contrast_stats=True)
    _, _, _, _, inside = drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, smp, 41, probe_beta=0.5, forced=cut)
    assert bool(inside.all()) and bool(torch.isfinite(lp).all())
    live = kept > 0
    print(f"contrastive call: mean kept {float(kept[live].float().mean()):.1f} of {cfg.vocab_size}, mean divergence "
          f"{float(div[live].mean()):.3f} nats")
    assert bool(live[:, 0].all()) and bool((kept[live] < cfg.vocab_size).all()) and bool((div[live] > 0).all())


# ---- the interface --------------------------------------------------------------------------------------------------------------------------
def test_diverse_decode_takes_a_contrast():
    cfg, _, _, dec = medium("untied-sv1")
    feats, senti, _, _ = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    end = cfg.boundary_index
    kw = dict(sampler=sampling.MultinomialSampler(1.0), sample_seed=9)

    def run(**more):
        torch.manual_seed(3)
        return diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, **{**kw, **more})

    plain, _ = run()
    off, _ = run(contrast=Contrast(0.0, 0.0, features="mean"))
    assert torch.equal(plain, off)
    flat = lambda p: padded(p.reshape(NIMG * NS, -1), STEPS, end)
    outs = {}
    for name, c in (("mean", Contrast(1.0, 0.1, features="mean")), ("noise", Contrast(1.0, 0.1, features="noise:0.5")),
                    ("latent", Contrast(1.0, 0.1, latent="mean")), ("sentiment", Contrast(1.0, 0.1, sentiment=0.0)),
                    ("engine", Contrast(1.0, 0.1, engine=second_engine("untied-sv1")[2]))):
        caps, k = run(contrast=c)
        again, _ = run(contrast=c)
        assert caps.shape[:2] == (NIMG, NS) and caps.size(-1) == k and torch.equal(caps, again), name
        outs[name] = flat(caps)
        assert not torch.equal(outs[name], flat(plain)), name
    # the call's amateur is the one DecodeEngine.sample is handed directly
    ctx = dec.prepare(feats.cuda())
    c = Contrast(1.0, 0.1, features="mean").prepare(dec, ctx.feats)
    assert c.ctx is not None and torch.equal(c.ctx.feats, amateur_features(feats.cuda(), "mean"))
    # greedy contrastive decoding is the top-k sampler with k = 1: no randomness of the draw is left
    g1, _ = run(contrast=Contrast(1.0, 0.1, features="mean"), sampler=sampling.TopKSampler(k=1), sample_seed=9)
    g2, _ = run(contrast=Contrast(1.0, 0.1, features="mean"), sampler=sampling.TopKSampler(k=1), sample_seed=10)
    assert torch.equal(g1, g2)
    # composes with logit rules, a truncation, a prefix and an attention trace
    rules = sampling.LogitRules(no_repeat_ngram=1, min_length=3)
    prefix = DecodePrefix(torch.tensor([[5, 6], [7, -1], [-1, -1]]))
    caps, _ = run(contrast=Contrast(1.0, 0.1, features="mean"), truncation=sampling.EtaTruncation(0.01), logit_rules=rules, prefix=prefix)
    assert caps[0, :, :2].tolist() == [[5, 6]] * NS and caps[1, :, 0].tolist() == [7] * NS
    out = run(contrast=Contrast(1.0, 0.1, latent="mean"), logit_rules=rules, attention="summary")
    assert out[-1].top_region.shape[:2] == (NIMG, NS)
    for more, name in ((dict(sampler=None), "not the beam search"), (dict(sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                       (dict(sampled_beam=True), "sampled-node beam search"),
                       (dict(sampler=None, diverse_beam=sampling.DiverseBeam(1, 0.5)), "diverse beam search")):
        with pytest.raises(ValueError, match="contrast belongs to the word samplers.*" + name):
            diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, contrast=Contrast(1.0), **{**kw, **more})


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.contrast import Contrast
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", 3, "MODEL.DECODE_SAMPLER", "top-k", "MODEL.BEAM_SIZE", 1, "MODEL.SAMPLER_TOP_K", 3,
                            "MODEL.IMAGE_FEATURE_SIZE", 64, "MODEL.EMBEDDING_SIZE", 40, "MODEL.HIDDEN_SIZE", 48,
                            "MODEL.ATTENTION_PROJECTION_SIZE", 32, "MODEL.Z_SPACE", 16, "DATA.MAX_CAPTION_LENGTH", 8] + {keys!r})
def run(contrast="config"):
    torch.manual_seed(C.RANDOM_SEED)
    m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                    sampler=sampling.from_config(C.MODEL)).cuda().eval()
    with torch.no_grad():
        m._output_layer.weight.mul_(8.0)
    if contrast != "config":
        m.contrast(contrast)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
    return m(feats)["predictions"].cpu().tolist()
print(json.dumps([run(), run(None), run(Contrast(1.5, 0.2, features="mean"))]))
"""


def test_module_reads_the_keys_and_takes_a_contrast_in_a_child_process():
    """The eval forward of a top-k (k = 3) module: with the keys at their defaults it is the forward without a contrast; with
    MODEL.CONTRAST_ALPHA 1.5, CONTRAST_BETA 0.2 and CONTRAST_AMATEUR mean-features it is the forward under contrast(Contrast(1.5, 0.2,
    features="mean")); contrast(None) switches the keys' contrast off again."""
    pkg = os.path.join(ROOT, "style-seqcvae_amd")
    outs = {}
    for name, keys in (("off", []),
                       ("on", ["MODEL.CONTRAST_ALPHA", 1.5, "MODEL.CONTRAST_BETA", 0.2, "MODEL.CONTRAST_AMATEUR", "mean-features"])):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=pkg, keys=keys)
        outs[name] = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    plain, plain_none, plain_set = outs["off"]
    keyed, keyed_none, keyed_set = outs["on"]
    assert plain == plain_none == keyed_none
    assert keyed != plain
    assert keyed == plain_set == keyed_set


SCRIPT_YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
               "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
               "  BEAM_SIZE: 1\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
               "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n  DECODE_SAMPLER: top-k\n  SAMPLER_TOP_K: 4\n")


def test_inference_script_with_the_contrast_flags(tmp_path):
    """scripts/inference.py: --contrast 1:0.1 --contrast-amateur prior-mean changes the captions of the run without the flags, writes
    the bytes of the run with the MODEL.CONTRAST_* keys and, with --contrast-output, the per-word divergence of every returned
    caption.  (--contrast 0 and the refusals are decided by check_contrast_args: tests/test_contrast_cpu.py.)"""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(SCRIPT_YAML)
    script = os.path.join(ROOT, "scripts", "inference.py")
    base = [script, "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4", "--vocab-size", "150", "--num-boxes", "5"]

    def run(name, *extra):
        out = tmp_path / (name + ".json")
        run_child(base + ["--output-path", str(out)] + list(extra))
        return out.read_bytes()

    plain = run("plain")
    div_path = tmp_path / "div.json"
    on = run("on", "--contrast", "1:0.1", "--contrast-amateur", "prior-mean", "--contrast-output", str(div_path))
    assert on != plain and len(json.loads(on)) == 4 * 5
    assert on == run("keys", "--config-override", "MODEL.CONTRAST_ALPHA", "1.0", "MODEL.CONTRAST_BETA", "0.1", "MODEL.CONTRAST_AMATEUR",
                     "prior-mean")
    rows = json.loads(div_path.read_text())
    caps = json.loads(on)
    assert len(rows) == len(caps)
    for row, cap in zip(rows, caps):
        assert row["image_id"] == cap["image_id"] and len(row["divergence"]) >= 1
        assert all(isinstance(v, float) and v >= 0 for v in row["divergence"])
    assert any(v > 0 for row in rows for v in row["divergence"])
