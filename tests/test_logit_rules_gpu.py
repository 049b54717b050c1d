"""GPU: the logit rules of the word samplers (include/ssc.h: ssc_logit_rules).  The kernel (ssc_logit_rules_rows) bit for bit against
the NumPy restatement (tests/logitrulesref.py); the sampled decode under rules (ssc_sample_opts.rules, DecodeEngine.sample) against
the same decode driven step by step, against the rules themselves and against the CPU oracle; the module and scripts/inference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import logitrulesref as R
import oracle
from oracle.seqcvae_oracle import cell_step, embed, output_logits, zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from test_attention_trace_gpu import R_, STEPS, VARIANTS, entry_inputs, medium, medium_params
from test_latent_guide_gpu import bits, make_guide, step_prior
from test_sampling_gpu import inputs as wide_inputs
from test_sampling_gpu import model as wide_model
from test_sampling_gpu import run_child

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1
GUARD = 8        # floats in front of and behind every buffer
SENTINEL = 12345.0


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def placed(x, off):
    """x (numpy, 2-D float32) on the device inside a buffer of sentinels, its first element `off` floats past a 16-byte boundary, GUARD
    words on either side.  -> (the whole buffer, the view of x)"""
    flat = torch.full((GUARD + off + x.size + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = flat[GUARD + off: GUARD + off + x.size].view(*x.shape)
    view.copy_(torch.from_numpy(x))
    assert (view.data_ptr() % 16) == 4 * (off % 4)
    return flat, view


def rules_struct(r, bias_d=None, ld_bias=0, bias_row_d=None):
    d = L.LogitRules()
    d.no_repeat_ngram, d.min_length, d.n_suppress = r.no_repeat_ngram, r.min_length, len(r.suppress)
    for i, v in enumerate(r.suppress):
        d.suppress[i] = v
    d.repetition_penalty, d.presence_penalty, d.frequency_penalty = (float(r.repetition_penalty), float(r.presence_penalty),
                                                                     float(r.frequency_penalty))
    if bias_d is not None:
        d.bias, d.ld_bias, d.n_bias = bias_d.data_ptr(), ld_bias, r.bias.shape[0]
        d.bias_row = bias_row_d.data_ptr() if bias_row_d is not None else None
    return d


def run_rules(logits_view, ld, rows, V, d, hist_d, t):
    L.load().ssc_logit_rules_rows(logits_view.data_ptr(), ld, rows, V, C.byref(d), L.ptr(hist_d), rows, t, END, L.stream_ptr())
    torch.cuda.synchronize()


def history(rng, V, rows, t):
    """(max(t, 1), rows) int64 over an alphabet of 4 ids, so that n-grams repeat.  Row 0 repeats ONE id: for every n <= t its last
    n - 1 tokens have occurred before, followed by that id - an n-gram ban is certain.  Every fourth row has ended (last token END);
    one row of the larger cases holds an id outside the vocabulary."""
    alphabet = rng.choice(np.arange(2, V), size=4, replace=False)
    h = rng.choice(alphabet, size=(max(t, 1), rows)).astype(np.int64)
    h[:, 0] = alphabet[0]
    if t >= 1:
        h[t - 1, 3::4] = END
        if rows > 4:
            h[0, 1] = V + 5
        if rows > 5 and t >= 2:
            h[0, 5] = -7
    return h, alphabet


#            n   theta pres  freq  n_sup  m(t)                   bias
SETTINGS = [(0,  1.0,  0.0,  0.0,  0,     lambda t: 0,           None),                 # only checked to change nothing (inactive)
            (1,  1.0,  0.0,  0.0,  0,     lambda t: 0,           None),
            (2,  1.3,  0.0,  0.0,  8,     lambda t: t + 1,       None),
            (3,  1.0,  0.5,  0.25, 0,     lambda t: t,           None),
            (64, 1.3,  0.5,  0.25, 8,     lambda t: t + 1,       None),
            (0,  1.0,  0.0,  0.0,  0,     lambda t: 0,           ("shared", "pad3", 0)),
            (2,  1.3,  0.5,  0.0,  8,     lambda t: t,           ("shared", "same", 1)),   # both rows one float off 16 bytes: the 16-byte path
            (3,  1.0,  0.0,  0.25, 0,     lambda t: t + 1,       ("rows", "pad3", 1)),
            (1,  1.3,  0.5,  0.25, 8,     lambda t: t + 1,       ("rows", "same", 0)),     # aligned alike at offset 0
            (2,  1.3,  0.5,  0.25, 0,     lambda t: 0,           ("rows", "same", (1, 2)))]  # aligned differently: the scalar path


def one_case(rng, V, ld, rows, t, setting):
    """-> the number of n-gram bans that fired; asserts bit-equality of every buffer with the restatement's"""
    n, theta, pres, freq, n_sup, m_of, bias_mode = setting
    hist, alphabet = history(rng, V, rows, t)
    free = np.setdiff1d(np.arange(2, V), alphabet)
    suppress = tuple(int(v) for v in rng.choice(free, size=n_sup, replace=False))
    x = (rng.standard_normal((rows, ld)) * 3).astype(np.float32)
    x[:, alphabet[1]] = 0.0                       # a logit of exactly 0 under theta
    x[:, V:] = np.nan                             # the pad column is poisoned
    live = np.ones(rows, dtype=bool)
    if t >= 1:
        live = hist[t - 1] != END
        x[~live] = np.nan                         # ended rows are neither read nor written
    bias = bias_row = None
    off_x = off_b = 0
    ld_bias = 0
    if bias_mode is not None:
        kind, ldk, offs = bias_mode
        off_x, off_b = offs if isinstance(offs, tuple) else (offs, offs)
        n_bias = 1 if kind == "shared" else 3
        ld_bias = V + 3 if ldk == "pad3" else ld
        bias_full = np.full((n_bias, ld_bias), np.nan, dtype=np.float32)
        bias_full[:, :V] = rng.standard_normal((n_bias, V)).astype(np.float32)
        bias_full[:, :V][rng.random((n_bias, V)) < 0.05] = -np.inf
        bias = bias_full[:, :V]
        if kind == "rows":
            bias_row = [i % n_bias for i in range(rows)]
            if rows > 1:   # (a single row keeps its bias)
                bias_row[-1] = -1
                bias_row[1] = n_bias + 2
    r = R.Rules(n, m_of(t), suppress, theta, pres, freq, bias, bias_row)
    want = R.edit_rows(x, V, hist, t, r, END)
    fired = sum(len(R.ngram_bans([int(hist[j, i]) for j in range(t)], n, V, END)) for i in range(rows) if live[i])
    flat, view = placed(x, off_x)
    before = flat.clone()
    hist_d = torch.from_numpy(hist).cuda()
    bias_flat = bias_d = bias_row_d = None
    if bias is not None:
        bias_flat, bias_d = placed(bias_full, off_b)
        bias_before = bias_flat.clone()
        bias_row_d = torch.tensor(bias_row, dtype=torch.int32, device="cuda") if bias_row is not None else None
    d = rules_struct(r, bias_d, ld_bias, bias_row_d)
    expect = before.clone()
    expect[GUARD + off_x: GUARD + off_x + x.size] = torch.from_numpy(want).reshape(-1).cuda()
    outs = []
    for _ in range(2):   # two calls on equal inputs
        flat.copy_(before)
        run_rules(view, ld, rows, V, d, hist_d if t >= 1 else None, t)
        outs.append(flat.clone())
    tag = (V, ld, rows, t, setting[:5], bias_mode)
    assert torch.equal(bits(outs[0]), bits(outs[1])), tag
    if not torch.equal(bits(outs[0]), bits(expect)):
        got = outs[0][GUARD + off_x: GUARD + off_x + x.size].view(rows, ld).cpu().numpy()
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        i, v = bad[0]
        raise AssertionError(f"{tag}: {len(bad)} elements differ, first at row {i} column {v}: got {got[i, v]!r}, want {want[i, v]!r}, "
                             f"input {x[i, v]!r}; guards intact: {torch.equal(bits(outs[0][:GUARD]), bits(before[:GUARD]))}")
    assert torch.equal(hist_d.cpu(), torch.from_numpy(hist))
    if bias is not None:
        assert torch.equal(bits(bias_flat), bits(bias_before)), tag   # the bias matrix is never written
    if not sampling.LogitRules(n, m_of(t), suppress, theta, pres, freq).active and bias is None:
        assert torch.equal(bits(outs[0]), bits(before))
    return fired


@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("V,ld", [(37, 37), (451, 452), (1000, 1000), (10000, 10000)])
def test_rows_kernel_is_bit_equal_to_the_restatement(V, ld, rows):
    """Every edited row bit-equal to the restatement; guard words, the poisoned pad column, ended rows (NaN), the history and the bias
    bit-equal to their inputs; two calls bit-equal; all controls off changes nothing.  Steps 0, 1, 2, 7, 20 (and 63 from V 451
    on); n in {0, 1, 2, 3, 64}; theta, presence and frequency on and off; 0 and 8 suppressed ids; min_length on either side of t;
    no bias, one shared row, per-row indices with a -1 and an out-of-range value, entries of -inf, ld_bias = V + 3 (the scalar
    path), both rows aligned alike at offsets 0 and 1 (16-byte accesses where ld allows) and aligned differently."""
    rng = np.random.default_rng(V * 131 + rows)
    ts = [0, 1, 2, 7, 20] + ([63] if V >= 451 else [])
    cases = 0
    for t in ts:
        for setting in SETTINGS:
            n = setting[0]
            if V <= t + setting[4] + 1:
                continue
            fired = one_case(rng, V, ld, rows, t, setting)
            if n >= 1 and t >= n:
                assert fired >= 1, (V, rows, t, n)   # at least one n-gram ban fired
            cases += 1
    assert cases >= len(ts) * (len(SETTINGS) - 3)


def test_a_bias_that_leaves_two_tokens_confines_every_sampler():
    """All but two tokens banned through the bias (-inf), then the row sampler of each kind on the edited rows: every drawn token is
    one of the two, and its log-prob is that of a two-token distribution."""
    V, rows = 451, 70
    rng = np.random.default_rng(5)
    x = torch.from_numpy((rng.standard_normal((rows, V)) * 2).astype(np.float32)).cuda()
    keep = (17, 300)
    bias = torch.full((1, V), float("-inf"), device="cuda")
    bias[0, list(keep)] = 0.0
    d = L.LogitRules()
    d.repetition_penalty = 1.0
    d.bias, d.ld_bias, d.n_bias = bias.data_ptr(), V, 1
    run_rules(x, V, rows, V, d, None, 0)
    lse = torch.logsumexp(x[:, list(keep)].double(), dim=1).cpu()
    for sampler in (sampling.MultinomialSampler(1.0), sampling.TopKSampler(k=5, temperature=1.3), sampling.TopPSampler(p=0.9)):
        pred = torch.empty(rows, dtype=torch.int64, device="cuda")
        lp = torch.empty(rows, device="cuda")
        sd = sampler.desc(21)
        L.load().ssc_sample_rows(L.ptr(x), V, rows, V, C.byref(sd), None, 0, None, None, END, L.ptr(pred), L.ptr(lp), None, L.stream_ptr())
        torch.cuda.synchronize()
        pred, lp = pred.cpu(), lp.cpu()
        assert set(pred.tolist()) <= set(keep), sampler
        if sampler.kind == 0:
            assert set(pred.tolist()) == set(keep)   # 70 rows: both tokens are drawn
        want = x.cpu()[torch.arange(rows), pred].double() - lse
        assert (lp.double() - want).abs().max() < 1e-5


# ---- the decode -------------------------------------------------------------------------------------------------------------------------
SAMPLERS = {"multinomial": sampling.MultinomialSampler(1.0), "top-k": sampling.TopKSampler(k=3), "top-p": sampling.TopPSampler(p=0.9, temperature=1.2)}
NIMG, NS = 3, 2


class ForcedRules(sampling.LogitRules):
    """Inactive rules that DecodeEngine.sample hands to ssc_decode_sample_opts (as its rules) all the same"""
    active = True


def decode_inputs(cfg, seed=17, nimg=NIMG, ns=NS, steps=STEPS):
    feats, senti, eps0, eps = entry_inputs(cfg, nimg, ns, R_, seed, steps)
    B = nimg * ns
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda() if senti is not None else None
    return feats.cuda(), sent_b, eps0.cuda(), eps.cuda()


def image_bias(V, nimg, seed, banned=()):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(nimg, V, generator=g) * 1.5
    for i, v in enumerate(banned):
        b[i % nimg, v] = float("-inf")
    return b


def yardstick_rules(V, nimg):
    return sampling.LogitRules(no_repeat_ngram=2, min_length=4, suppress=(0,), repetition_penalty=1.3, presence_penalty=0.2,
                               frequency_penalty=0.1, bias=image_bias(V, nimg, 3, banned=(7, 9, 11)).cuda())


def stepwise_sample_rules(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, guide, sampler, seed, rules):
    """The sampled decode driven from Python: DecodeEngine.step, ssc_logit_rules_rows, ssc_sample_rows per step."""
    lib = L.load()
    V = dec.dims.V
    sdesc = sampler.desc(seed)
    rd, _keep = rules.desc(ns)
    run = torch.zeros(B, device="cuda")
    tokens = torch.full((B,), end, dtype=torch.int64, device="cuda")
    hist = torch.full((steps, B), -1, dtype=torch.int64, device="cuda")
    state, last = None, None
    for t in range(steps):
        pm, pv = step_prior(guide, t, B, 1, sent_b, dec.dims)
        logits, state, _ = dec.step(ctx, tokens, state, sent_b, eps0 if t == 0 else eps[t - 1], raw_logits=True, prior_mean=pm, prior_var=pv)
        lib.ssc_logit_rules_rows(L.ptr(logits), V, B, V, C.byref(rd), L.ptr(hist), B, t, end, L.stream_ptr())
        slp = torch.empty(B, device="cuda")
        lib.ssc_sample_rows(L.ptr(logits), V, B, V, C.byref(sdesc), None, t, L.ptr(last), L.ptr(run), end, L.ptr(hist[t]), L.ptr(slp), None,
                            L.stream_ptr())
        last = tokens = hist[t]
    return hist.t().contiguous(), run


def padded(pred, steps, end):
    return torch.nn.functional.pad(pred, (0, steps - pred.size(1)), value=end)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_off_path_is_the_plain_sampled_decode(variant):
    """logit_rules=None and rules with every control off - handed to DecodeEngine.sample, and handed to ssc_decode_sample_opts
    itself - give the predictions and the log-probs of the call without the argument, bit for bit."""
    cfg, _, _, dec = medium(variant)
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    ctx = dec.prepare(feats)
    for name, smp in SAMPLERS.items():
        args = (ctx, sent_b, NS, STEPS, cfg.boundary_index, eps0, eps, smp, 13)
        pred0, lp0 = dec.sample(*args)
        for lr in (None, sampling.LogitRules(), ForcedRules()):
            pred, lp = dec.sample(*args, logit_rules=lr)
            assert torch.equal(pred, pred0) and torch.equal(bits(lp), bits(lp0)), (variant, name, lr)


@pytest.mark.parametrize("kind", list(SAMPLERS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ruled_decode_against_the_stepwise_driver(variant, kind):
    """Active rules (n = 2, m = 4, theta 1.3, presence 0.2, frequency 0.1, token 0 suppressed, a per-image bias with -inf entries):
    the one call gives the tokens and the log-probs of the same decode driven step by step - DecodeEngine.step, ssc_logit_rules_rows,
    ssc_sample_rows - bit for bit, with skip_dead / early_stop on and off, under a latent guide and with an attention trace.  The
    rules change the captions.  Measured on one MI355X: the same bits in all 96 runs."""
    cfg, _, _, dec = medium(variant)
    end, V = cfg.boundary_index, cfg.vocab_size
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    B = NIMG * NS
    smp = SAMPLERS[kind]
    rules = yardstick_rules(V, NIMG)
    for guide in (None, make_guide("var+len", B, cfg.z_space, STEPS, 5)):
        want_pred, want_lp = stepwise_sample_rules(dec, dec.prepare(feats), sent_b, B, NS, STEPS, end, eps0, eps, guide, smp, 13, rules)
        for skip_dead, early_stop, attention in ((True, True, False), (False, False, False), (True, False, True), (False, True, False)):
            out = dec.sample(dec.prepare(feats), sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=early_stop, attention=attention,
                             guide=guide, logit_rules=rules, skip_dead=skip_dead)
            pred, lp = out[0], out[1]
            tag = (variant, kind, guide is not None, skip_dead, early_stop, attention)
            assert torch.equal(padded(pred, STEPS, end), want_pred), tag
            assert torch.equal(bits(lp), bits(want_lp)), (tag, (lp - want_lp).abs().max().item())
            if attention:
                tr = dec.attention(out[2])
                first_end = (want_pred == end).int().argmax(1)
                for b in range(B):   # every word up to the caption's END has a trace
                    n_words = int(first_end[b]) + 1 if bool((want_pred[b] == end).any()) else STEPS
                    assert (tr.top_region[b, :n_words] >= 0).all() and (tr.top_region[b, n_words:] == -1).all()
        if guide is None:
            plain, _ = dec.sample(dec.prepare(feats), sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=False)
            assert not torch.equal(plain, want_pred), "the rules changed nothing"


def violations(pred, end, n, m, forbidden):
    """-> (captions that repeat an n-gram, captions that end before m words, captions that hold a forbidden word (per image))"""
    rep = short = bad = 0
    for b, cap in enumerate(pred.tolist()):
        words = cap[: cap.index(end)] if end in cap else cap
        grams = [tuple(words[i: i + n]) for i in range(len(words) - n + 1)]
        rep += len(set(grams)) != len(grams)
        short += end in cap and len(words) < m
        bad += any(w in forbidden(b) for w in words)
    return rep, short, bad


def test_the_rules_hold_where_the_plain_decode_breaks_them():
    """Top-k (k = 3) sampling of 32 captions of up to 16 words: the call without rules repeats a bigram, ends before 4 words and emits
    the two words picked from its own output (one suppressed, one biased to -inf for every image) - each at least once, so that
    the check is not vacuous; the ruled call on the same seed does none of these."""
    cfg, _, _, dec = medium("untied-sv1")
    end, V = cfg.boundary_index, cfg.vocab_size
    nimg, ns, steps, n, m = 4, 8, 16, 2, 4
    feats, sent_b, eps0, eps = decode_inputs(cfg, seed=29, nimg=nimg, ns=ns, steps=steps)
    smp = sampling.TopKSampler(k=3)
    args = (dec.prepare(feats), sent_b, ns, steps, end, eps0, eps, smp, 41)
    plain, _ = dec.sample(*args, early_stop=False)
    words, counts = np.unique(plain[plain != end].cpu().numpy(), return_counts=True)
    order = words[np.argsort(-counts, kind="stable")]
    sup, neg = int(order[0]), int(order[1])      # the plain call's two most frequent words
    forbidden = lambda b: (sup, neg)
    rep, short, bad = violations(plain, end, n, m, forbidden)
    print(f"plain call: {rep} captions repeat a bigram, {short} end before {m} words, {bad} hold word {sup} or {neg}")
    assert rep >= 1 and short >= 1 and bad >= 1
    bias = torch.zeros(nimg, V)
    bias[:, neg] = float("-inf")
    rules = sampling.LogitRules(no_repeat_ngram=n, min_length=m, suppress=(sup,), bias=bias.cuda())
    ruled, lp = dec.sample(*args, early_stop=False, logit_rules=rules)
    assert violations(ruled, end, n, m, forbidden) == (0, 0, 0)
    assert torch.isfinite(lp).all()


def oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, smp, rules, ref_rules):
    """The GPU's tokens teacher-forced through the oracle's decode step (cell_step and output_logits, as oracle.decode_step calls
    them, keeping the raw logits) with the same noise; the restatement's rules on the oracle's logits.
    -> max over the captions of |summed edited log-prob, oracle - device|; asserts that no GPU token is banned on the oracle's side."""
    B = nimg * ns
    end, V = cfg.boundary_index, cfg.vocab_size
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B) if senti is not None else None
    pred, slp = dec.sample(dec.prepare(feats.cuda()), sent_b.cuda() if sent_b is not None else None, ns, steps, end, eps0.cuda(), eps.cuda(),
                           smp, 77, early_stop=False, logit_rules=rules)
    pred, slp = pred.cpu(), slp.cpu()
    fr = feats.unsqueeze(1).expand(nimg, ns, feats.size(1), feats.size(2)).reshape(B, feats.size(1), -1)
    se = sent_b.view(B, 1) if sent_b is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
    states = zero_states(B, cfg.hidden_size, fr)
    tokens = torch.full((B,), end, dtype=torch.long)
    total = np.zeros(B)
    alive = np.ones(B, dtype=bool)
    with torch.no_grad():
        for t in range(steps):
            e = eps0 if t == 0 else eps[t - 1]
            h_dec, states, _, _, _, _ = cell_step(params, cfg, fr, embed(params, cfg, tokens), states, False, se, pm, pv, e, None, None, True)
            logits = output_logits(params, cfg, h_dec).float().numpy()
            for b in range(B):
                tok = int(pred[b, t])
                if not alive[b]:
                    assert tok == end
                    continue
                hist = [int(v) for v in pred[b, :t]]
                assert tok not in R.banned(V, hist, ref_rules, end, row=b), (b, t, tok)
                row = R.edit_row(logits[b], V, hist, ref_rules, end, row=b).astype(np.float64)
                mx = row.max()
                total[b] += row[tok] - (mx + np.log(np.exp(row - mx).sum()))
            alive &= (pred[:, t] != end).numpy()
            tokens = pred[:, t].clone()
    return float(np.abs(total - slp.double().numpy()).max())


def reference_rules(rules, ns):
    bias = rules.bias.cpu().numpy() if rules.bias is not None else None
    rows = None if bias is None or bias.shape[0] == 1 else [b // ns for b in range(bias.shape[0] * ns)]
    return R.Rules(rules.no_repeat_ngram, rules.min_length, rules.suppress, rules.repetition_penalty, rules.presence_penalty,
                   rules.frequency_penalty, bias, rows)


ORACLE_TOL = 1e-4 * 1.3   # the sampled decode's 1e-4 against the oracle, scaled by max(theta, 1 / theta): the edit multiplies a logit
#                           error by at most that factor (the additive edits carry it over unchanged)


@pytest.mark.parametrize("kind", list(SAMPLERS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ruled_decode_against_the_oracle(variant, kind):
    """Toy width (the medium model): each caption's summed edited log-prob within 1e-4 * max(theta, 1 / theta) of the oracle's under
    the restatement's rules, and no device token banned on the oracle's side (exact).
    Measured on one MI355X: at most 5.2e-6 over the 12 cases."""
    cfg, params = medium_params(variant)
    _, _, _, dec = medium(variant)
    feats, senti, eps0, eps = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    rules = yardstick_rules(cfg.vocab_size, NIMG)
    worst = oracle_check(cfg, params, dec, feats, senti, NIMG, NS, STEPS, eps0, eps, SAMPLERS[kind], rules, reference_rules(rules, NS))
    print(f"{variant} {kind}: max |summed edited log-prob, oracle - device| {worst:.3e}")
    assert worst <= ORACLE_TOL, (variant, kind, worst)


def test_full_width_ruled_decode_against_the_oracle():
    """Full width (H 1200, V 10 000, R 36; 2 images x 3 samples, 6 steps), top-p: the same two checks.
    Measured on one MI355X: 4.6e-6."""
    cfg, params, _, dec = wide_model(True)
    nimg, ns, R, steps = 2, 3, 36, 6
    feats, senti, eps0, eps = wide_inputs(cfg, nimg, ns, R, seed=23, steps=steps)
    rules = yardstick_rules(cfg.vocab_size, nimg)
    worst = oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, sampling.TopPSampler(p=0.9, temperature=1.2), rules,
                         reference_rules(rules, ns))
    print(f"full width top-p: max |summed edited log-prob, oracle - device| {worst:.3e}")
    assert worst <= ORACLE_TOL, worst


def test_diverse_decode_takes_logit_rules():
    cfg, _, _, dec = medium("untied-sv1")
    feats, senti, _, _ = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    smp = sampling.TopKSampler(k=3)
    rules = sampling.LogitRules(no_repeat_ngram=1, min_length=3)
    kw = dict(sampler=smp, sample_seed=9)
    torch.manual_seed(3)
    plain, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, cfg.boundary_index, **kw)
    torch.manual_seed(3)
    off, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, cfg.boundary_index, logit_rules=sampling.LogitRules(), **kw)
    torch.manual_seed(3)
    ruled, k = diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, cfg.boundary_index, logit_rules=rules, **kw)
    assert torch.equal(plain, off)
    assert ruled.shape[:2] == (NIMG, NS) and ruled.size(-1) == k
    assert violations(padded(ruled.view(NIMG * NS, -1), STEPS, cfg.boundary_index), cfg.boundary_index, 1, 3, lambda b: ())[:2] == (0, 0)


# ---- module and script ----------------------------------------------------------------------------------------------------------------
MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", 3, "MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", 3, "MODEL.BEAM_SIZE", 1,
                            "MODEL.IMAGE_FEATURE_SIZE", 64, "MODEL.EMBEDDING_SIZE", 40, "MODEL.HIDDEN_SIZE", 48,
                            "MODEL.ATTENTION_PROJECTION_SIZE", 32, "MODEL.Z_SPACE", 16, "DATA.MAX_CAPTION_LENGTH", 8] + {keys!r})
def run(rules="config"):
    torch.manual_seed(C.RANDOM_SEED)
    m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                    sampler=sampling.from_config(C.MODEL)).cuda().eval()
    if rules != "config":
        m.logit_rules(rules)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
    return m(feats)["predictions"].cpu().tolist()
bias = torch.zeros(8, 120, device="cuda")
bias[:, 5] = float("-inf")
print(json.dumps([run(), run(None), run(sampling.LogitRules(no_repeat_ngram=1, min_length=8, bias=bias))]))
"""


def words_of(cap, end):
    return cap[: cap.index(end)] if end in cap else cap


def test_module_reads_the_keys_and_takes_rules_in_a_child_process():
    """The eval forward of a top-k module: with the keys at their defaults it is the forward without rules; with
    MODEL.SAMPLER_NO_REPEAT_NGRAM 1 and SAMPLER_MIN_LENGTH 5 no caption repeats a word or ends before 5; logit_rules(None) switches the
    keys' rules off again and logit_rules(rules) sets others (a per-image bias included)."""
    pkg = os.path.join(ROOT, "style-seqcvae_amd")
    outs = {}
    for name, keys in (("off", []), ("on", ["MODEL.SAMPLER_NO_REPEAT_NGRAM", 1, "MODEL.SAMPLER_MIN_LENGTH", 5])):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=pkg, keys=keys)
        outs[name] = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    plain, plain_none, set_rules = outs["off"]
    keyed, keyed_none, _ = outs["on"]
    assert plain == plain_none == keyed_none
    assert keyed != plain
    for cap in keyed:
        w = words_of(cap, END)
        assert len(set(w)) == len(w) and (len(w) >= 5 or END not in cap)
    for cap in set_rules:   # min_length = the caption length: no END at all, no word twice, never word 5
        assert END not in cap and len(set(cap)) == len(cap) == 8 and 5 not in cap


SCRIPT_YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
               "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
               "  BEAM_SIZE: 1\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
               "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n  DECODE_SAMPLER: top-k\n  SAMPLER_TOP_K: 4\n")


def test_inference_script_with_the_keys_and_a_word_bias(tmp_path):
    """scripts/inference.py: a --word-bias of zeros (the rules run, the logits keep their values) writes the bytes of the run
    without the flag; with the keys and a bias that bans two words no caption repeats a word, ends before 4 words or holds a
    banned word; the flag without a word sampler is refused."""
    import subprocess
    import sys
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(SCRIPT_YAML)
    script = os.path.join(ROOT, "scripts", "inference.py")
    base = [script, "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4", "--vocab-size", "150", "--num-boxes", "5"]

    def run(name, *extra):
        out = tmp_path / (name + ".json")
        run_child(base + ["--output-path", str(out)] + list(extra))
        return out.read_bytes()

    plain = run("plain")
    zeros = tmp_path / "zeros.json"
    zeros.write_text(json.dumps({"w7": 0.0, "w9": 0}))
    assert run("zeros", "--word-bias", str(zeros)) == plain
    used = sorted({w for c in json.loads(plain) for w in c["caption"].split()})
    assert len(used) >= 2
    ban = tmp_path / "ban.json"
    ban.write_text(json.dumps({used[0]: "-inf", used[1]: "-inf", "w3": 0.5}))
    ruled = json.loads(run("ruled", "--word-bias", str(ban), "--config-override", "MODEL.SAMPLER_NO_REPEAT_NGRAM", "1",
                           "MODEL.SAMPLER_MIN_LENGTH", "4", "MODEL.SAMPLER_REPETITION_PENALTY", "1.2"))
    assert len(ruled) == 4 * 5
    for c in ruled:
        w = c["caption"].split()
        assert len(set(w)) == len(w) and len(w) >= 4 and used[0] not in w and used[1] not in w, c
    r = subprocess.run([sys.executable] + base + ["--output-path", str(tmp_path / "x.json"), "--word-bias", str(ban), "--config-override",
                                                  "MODEL.DECODE_SAMPLER", "beam"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--word-bias needs a word sampler" in r.stderr, r.stderr[-2000:]
    unknown = tmp_path / "unknown.json"
    unknown.write_text(json.dumps({"zebra": 1.0}))
    r = subprocess.run([sys.executable] + base + ["--output-path", str(tmp_path / "x.json"), "--word-bias", str(unknown)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "'zebra' is not in the vocabulary" in r.stderr, r.stderr[-2000:]
