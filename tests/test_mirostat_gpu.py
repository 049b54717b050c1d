"""GPU: Mirostat 2.0 for the word samplers (include/ssc.h: ssc_mirostat).  The kernels (ssc_mirostat_rows, ssc_mirostat_update) against
the float64 restatement (tests/mirostatref.py) on inputs the restatement calls decidable; the sampled decode under Mirostat
(ssc_decode_sample_mirostat, DecodeEngine.sample) against the call without it, against the same decode driven step by step and
against the CPU oracle; the property the cut exists for; diverse_decode, the module and scripts/inference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import mirostatref as R
import oracle
from oracle.seqcvae_oracle import cell_step, embed, output_logits, zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from ssc_runtime.prefix import DecodePrefix
from test_attention_trace_gpu import R_, STEPS, VARIANTS, entry_inputs, medium, medium_params
from test_contrast_gpu import amateur_of, make_contrast, start_states
from test_latent_guide_gpu import bits, make_guide, step_prior
from test_logit_rules_gpu import GUARD, SENTINEL, decode_inputs, padded, placed, yardstick_rules
from test_sampling_gpu import run_child
from test_truncation_gpu import N_ROWS, NIMG, NS, SAMPLERS, SHAPES, TEMPS, guarded, padded_stats, rows_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1
TOL = 1e-4      # the project's parity tolerance: norm, surprise and mu' against float64
INF = float("inf")


def f32(v):
    """the value the library reads: the float32 nearest to v"""
    return float(np.float32(v))


# ---- the kernels --------------------------------------------------------------------------------------------------------------------------
MUS = ("below", "mid", "above")


def row_mus(x, V, T, which):
    """Per row the float32 threshold: below every surprise (only the top word stays), above every surprise (every finite entry
    stays), or mid-range - the midpoint of the widest gap between neighbouring surprises in the middle half of the row's sorted
    surprises (a flat row has no gap: a quarter nat below its one surprise).  A choice made from the inputs alone, in float64."""
    mu = np.full(N_ROWS, 1.0, dtype=np.float32)
    for r in range(N_ROWS):
        c = R.cut_row(x[r, :V], INF, T)
        if not c.live:
            continue
        s = np.sort(-c.logq[np.isfinite(c.logq)])
        if which == "below":
            mu[r] = s[0] - 0.5
        elif which == "above":
            mu[r] = s[-1] + 0.5
        else:
            mid = s[len(s) // 4: max(3 * len(s) // 4, len(s) // 4 + 2)]
            gaps = np.diff(mid)
            i = int(np.argmax(gaps)) if gaps.size and gaps.max() > 0 else -1
            mu[r] = 0.5 * (mid[i] + mid[i + 1]) if i >= 0 else s[0] - 0.25
    return mu


def run_rows(view, ld, rows, V, T, mu_d, last_d, kept, norm):
    L.load().ssc_mirostat_rows(view.data_ptr(), ld, rows, V, T, L.ptr(mu_d), L.ptr(last_d), END, L.ptr(kept), L.ptr(norm), L.stream_ptr())
    torch.cuda.synchronize()


def run_update(view, ld, rows, V, T, tau, eta, norm, pred_d, last_d, mu_d, mu_out, sur):
    L.load().ssc_mirostat_update(view.data_ptr(), ld, rows, V, T, tau, eta, L.ptr(norm), L.ptr(pred_d), L.ptr(last_d), END, L.ptr(mu_d),
                                 L.ptr(mu_out), L.ptr(sur), L.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", MUS)
@pytest.mark.parametrize("V,ld,off", SHAPES)
def test_kernels_against_the_restatement(V, ld, off, which):
    """Per temperature in {0.7, 1, 1.3}: the restatement finds no undecidable token in the inputs (asserted first); then the whole
    buffer is bit-equal to the restatement's edit - kept entries keep their bits, the others are -inf, the ended row (NaN), the row
    without a finite entry, the poisoned pad columns and the guard words are untouched -, `kept` is exact, `norm` within 1e-4 and
    left alone for the rows that pass through; two calls are bit-equal; a NULL kept changes nothing.  The update on the edited rows:
    mu' and the surprise within 1e-4 of the restatement for a kept word per row; a token outside [0, V), a dropped word, the ended
    and the empty row pass through (mu' = mu bit for bit, surprise 0); a NULL surprise changes nothing; in place (mu_out = mu_in)
    gives the same bits.  V = 1024: the 16-byte path (offset 0) gives the bits of the scalar path (offset 1)."""
    tau, eta = f32(2.0), f32(0.3)
    for T in TEMPS:
        x, last = rows_case(V, ld, 0, T, 1000 * V + int(T * 10))
        mu = row_mus(x, V, T, which)
        want, kept_ref, norm_ref, und = R.cut_rows(x, V, mu, T, last, END)
        tag = (V, ld, off, which, T)
        assert und == [], (tag, und[:5])
        live = [r for r in range(N_ROWS) if kept_ref[r] > 0]
        assert live == [0, 1, 2, 3, 4], tag
        fin = np.isfinite(x[:5, :V]).sum(1)
        if which == "below":
            assert kept_ref[:5].tolist() == [1] * 5, tag
        elif which == "above":
            assert kept_ref[:5].tolist() == fin.tolist(), tag
        else:
            assert all(1 <= kept_ref[r] < fin[r] for r in (0, 3, 4)), (tag, kept_ref)
        flat, view = placed(x, off)
        before = flat.clone()
        last_d = torch.from_numpy(last).cuda()
        mu_d = torch.from_numpy(mu).cuda()
        kept_buf, kept = guarded(N_ROWS, torch.int32, -99)
        norm_buf, norm = guarded(2 * N_ROWS, torch.float32, SENTINEL)
        expect = before.clone()
        expect[GUARD + off: GUARD + off + x.size] = torch.from_numpy(want).reshape(-1).cuda()
        outs = []
        for _ in range(2):   # two calls on equal inputs
            flat.copy_(before)
            kept_buf.fill_(-99)
            norm_buf.fill_(SENTINEL)
            run_rows(view, ld, N_ROWS, V, T, mu_d, last_d, kept, norm)
            outs.append((flat.clone(), kept_buf.clone(), norm_buf.clone()))
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(bits(a), bits(b)), tag
        got = outs[0][0]
        if not torch.equal(bits(got), bits(expect)):
            g = got[GUARD + off: GUARD + off + x.size].view(N_ROWS, ld).cpu().numpy()
            bad = np.argwhere(g.view(np.int32) != want.view(np.int32))
            i, v = bad[0]
            c = R.cut_row(x[i, :V], mu[i], T)
            raise AssertionError(f"{tag}: {len(bad)} elements differ, first at row {i} column {v}: got {g[i, v]!r}, want {want[i, v]!r}, "
                                 f"input {x[i, v]!r}, surprise {-c.logq[v] if v < V else None!r} at mu {mu[i]!r}; "
                                 f"guards intact: {torch.equal(bits(got[:GUARD]), bits(before[:GUARD]))}")
        assert bool((outs[0][1][:GUARD] == -99).all()) and bool((outs[0][1][-GUARD:] == -99).all()), tag
        assert bool((outs[0][2][:GUARD] == SENTINEL).all()) and bool((outs[0][2][-GUARD:] == SENTINEL).all()), tag
        kept_got = outs[0][1][GUARD: GUARD + N_ROWS].cpu().numpy()
        norm_got = outs[0][2][GUARD: GUARD + 2 * N_ROWS].view(2, N_ROWS).cpu().numpy().astype(np.float64)
        assert kept_got.tolist() == kept_ref.tolist(), tag
        assert (norm_got[:, 5:] == SENTINEL).all(), tag                      # the ended and the empty row: norm is left alone
        err_norm = np.abs(norm_got[:, :5] - norm_ref[:, :5]).max()
        assert err_norm <= TOL and (norm_got[0, :5] == norm_ref[0, :5]).all(), (tag, err_norm)
        flat.copy_(before)
        run_rows(view, ld, N_ROWS, V, T, mu_d, last_d, None, norm)             # no count asked for
        assert torch.equal(bits(flat), bits(expect)) and torch.equal(bits(norm_buf), bits(outs[0][2])), tag
        # ---- the update on the edited rows: a kept word other than the top one where there is one; then the rows that pass through
        kept_mask = np.isfinite(want[:, :V])
        pred = np.zeros(N_ROWS, dtype=np.int64)
        for r in range(5):
            ids = np.nonzero(kept_mask[r])[0]
            first = int(np.argmax(np.where(np.isfinite(x[r, :V]), x[r, :V], -np.inf)))
            others = ids[ids != first]
            pred[r] = int(others[len(others) // 2]) if others.size else first
        pred[5], pred[6] = 3, 3
        odd = pred.copy()
        odd[0], odd[1] = V, -1                                               # outside [0, V): checked on the device
        dropped = np.nonzero(np.isfinite(x[3, :V]) & ~kept_mask[3])[0]
        if dropped.size:
            odd[3] = int(dropped[0])                                         # a word the cut dropped: x_w = -inf
        sur_buf, sur = guarded(N_ROWS, torch.float32, SENTINEL)
        out_buf, mu_out = guarded(N_ROWS, torch.float32, SENTINEL)
        worst = 0.0
        for p in (pred, odd):
            mu_ref, sur_ref = R.update_rows(x, V, T, tau, eta, p, mu.astype(np.float64), last, END)
            for r in range(N_ROWS):   # (the restatement reads the row as it ARRIVED; a dropped word passes through on the device)
                if r < 5 and 0 <= p[r] < V and not kept_mask[r, p[r]]:
                    mu_ref[r], sur_ref[r] = mu[r], 0.0
            p_d = torch.from_numpy(p).cuda()
            res = []
            for _ in range(2):
                sur_buf.fill_(SENTINEL)
                out_buf.fill_(SENTINEL)
                run_update(view, ld, N_ROWS, V, T, tau, eta, norm, p_d, last_d, mu_d, mu_out, sur)
                res.append((sur_buf.clone(), out_buf.clone()))
            assert torch.equal(bits(res[0][0]), bits(res[1][0])) and torch.equal(bits(res[0][1]), bits(res[1][1])), tag
            assert torch.equal(bits(flat), bits(expect)), tag                # the update writes no logit
            for b, fill in ((res[0][0], SENTINEL), (res[0][1], SENTINEL)):
                assert bool((b[:GUARD] == fill).all()) and bool((b[-GUARD:] == fill).all()), tag
            sur_got = res[0][0][GUARD: GUARD + N_ROWS].cpu().numpy()
            mu_got = res[0][1][GUARD: GUARD + N_ROWS].cpu().numpy()
            passes = [r for r in range(N_ROWS) if sur_ref[r] == 0.0 and mu_ref[r] == mu[r]]
            assert set(passes) >= {5, 6}, tag
            for r in passes:
                assert sur_got[r] == 0.0 and mu_got[r].view(np.int32) == mu[r].view(np.int32), (tag, r)
            worst = max(worst, np.abs(sur_got - sur_ref).max(), np.abs(mu_got - mu_ref).max())
            out_buf.fill_(SENTINEL)
            run_update(view, ld, N_ROWS, V, T, tau, eta, norm, p_d, last_d, mu_d, mu_out, None)     # no surprise asked for
            assert torch.equal(bits(out_buf), bits(res[0][1])), tag
            inplace = mu_d.clone()
            run_update(view, ld, N_ROWS, V, T, tau, eta, norm, p_d, last_d, inplace, inplace, None)  # mu_out = mu_in
            assert torch.equal(bits(inplace), bits(mu_out)), tag
        print(f"{tag}: kept {kept_got.tolist()}, max |log Z - float64| {err_norm:.2e}, max |surprise, mu' - float64| {worst:.2e}")
        assert worst <= TOL, (tag, worst)
        if V == 1024:
            flat0, view0 = placed(x, 0)
            run_rows(view0, ld, N_ROWS, V, T, mu_d, last_d, kept, norm)
            assert torch.equal(bits(view0), bits(got[GUARD + off: GUARD + off + x.size].view(N_ROWS, ld))), tag
            assert torch.equal(kept_buf, outs[0][1]) and torch.equal(bits(norm_buf), bits(outs[0][2])), tag


# ---- the decode ---------------------------------------------------------------------------------------------------------------------------
# nats: the returned blocks are the device's own bits.  The medium model's rows hold 300 words (log 300 = 5.7 nats; the top word of a
# sharpened head carries about 4): a target of 5 nats from a start of 6 cuts the tail of the first steps' rows and then follows the
# drawn words - a start below the top word's surprise would leave the top word alone at every step
MIRO = sampling.Mirostat(5.0, 0.3, mu0=6.0, unit="nats")


class ForcedOff(sampling.Mirostat):
    """A Mirostat with tau = 0 that DecodeEngine.sample hands to ssc_decode_sample_mirostat all the same"""
    active = True


class Spy:
    """The library, noting which of the sampled decode's two entries is called"""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        if name in ("ssc_decode_sample_opts", "ssc_decode_sample_mirostat"):
            self._seen.append(name)
        return getattr(self._lib, name)


def drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, sampler, seed, miro=None, contrast=None, trunc=None, rules=None, guide=None,
          start=None, forced=None):
    """The sampled decode driven from Python: per step DecodeEngine.step of the expert (and of a contrast's amateur),
    ssc_contrast_rows, ssc_logit_rules_rows, ssc_truncate_rows, ssc_mirostat_rows, ssc_sample_rows, ssc_mirostat_update.  forced
    (B, steps): the tokens are given instead of drawn.
    -> (tokens (B, steps), log-probs (B), mu (B, steps + 1), surprise (B, steps), kept (B, steps), the logits (steps, B, V) as they
    ARRIVED at the Mirostat cut)"""
    lib = L.load()
    V = dec.dims.V
    T = float(sampler.temperature)
    sdesc = sampler.desc(seed)
    rd = rules.desc(ns) if rules is not None else None
    run = torch.zeros(B, device="cuda")
    hist = torch.full((steps, B), -1, dtype=torch.int64, device="cuda")
    mu = torch.zeros(steps + 1, B, device="cuda")
    sur = torch.zeros(steps, B, device="cuda")
    kept = torch.zeros(steps, B, dtype=torch.int32, device="cuda")
    norm = torch.zeros(2, B, device="cuda")
    arrived = torch.zeros(steps, B, V, device="cuda")
    if miro is not None:
        md = miro.desc()
        mu[0] = md.mu0
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
        if contrast is not None:
            logits_a = None
            if two:
                pm_a, pv_a = step_prior(a_guide, t, B, 1, a_sent, dec.dims)
                logits_a, state_a, _ = a_dec.step(a_ctx, tokens, state_a, a_sent, a_eps0 if t == 0 else a_eps[t - 1], raw_logits=True,
                                                  prior_mean=pm_a, prior_var=pv_a)
            lib.ssc_contrast_rows(L.ptr(logits), V, L.ptr(logits_a), V, B, V, contrast.alpha, contrast.beta, L.ptr(last), end, None, None,
                                  L.stream_ptr())
        if rd is not None:
            lib.ssc_logit_rules_rows(L.ptr(logits), V, B, V, C.byref(rd[0]), L.ptr(hist), B, t, end, L.stream_ptr())
        if trunc is not None:
            td = trunc.desc(None, None)
            lib.ssc_truncate_rows(L.ptr(logits), V, B, V, C.byref(td), T, L.ptr(last), end, L.stream_ptr())
        arrived[t] = logits
        if miro is not None:
            lib.ssc_mirostat_rows(L.ptr(logits), V, B, V, T, L.ptr(mu[t]), L.ptr(last), end, L.ptr(kept[t]), L.ptr(norm), L.stream_ptr())
        if forced is None:
            slp = torch.empty(B, device="cuda")
            lib.ssc_sample_rows(L.ptr(logits), V, B, V, C.byref(sdesc), None, t, L.ptr(last), L.ptr(run), end, L.ptr(hist[t]), L.ptr(slp), None,
                                L.stream_ptr())
        else:
            hist[t] = forced[:, t]
        if miro is not None:
            lib.ssc_mirostat_update(L.ptr(logits), V, B, V, T, md.tau, md.eta, L.ptr(norm), L.ptr(hist[t]), L.ptr(last), end, L.ptr(mu[t]),
                                    L.ptr(mu[t + 1]), L.ptr(sur[t]), L.stream_ptr())
        last = tokens = hist[t]
    return hist.t().contiguous(), run, mu.t().contiguous(), sur.t().contiguous(), kept.t().contiguous(), arrived


def first_max(x):
    """x (..., V) -> the lowest index at which each row holds its maximum"""
    V = x.size(-1)
    idx = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


def live_columns(tok, end):
    """tok (B, steps) -> (B, steps) bool: the row had not ended in front of the step"""
    live = torch.ones_like(tok, dtype=torch.bool)
    live[:, 1:] = (tok[:, :-1] != end).int().cummin(1).values.bool()
    return live


def check_obeys(tag, tok, mu, sur, arrived, end):
    """The exact property, from the blocks and the stepwise logits: every drawn token of a live row has surprise <= mu or is its
    row's lowest-index maximum.  -> the number of (row, step) pairs checked, and of those only the top-word exception covers."""
    B, steps = tok.shape
    first = first_max(arrived).t()                      # (B, steps)
    livecol = live_columns(tok, end)
    over = sur > mu[:, :steps]
    bad = livecol & over & (tok != first)
    assert not bool(bad.any()), (tag, bad.nonzero()[:5].tolist())
    assert bool((sur[~livecol] == 0).all()), tag
    return int(livecol.sum()), int((livecol & over).sum())


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mirostat_decode_against_the_stepwise_driver(variant):
    """The one call gives the tokens, the log-probs and the three blocks of the same decode driven step by step, bit for bit: each
    sampler, alone with skip_dead / early_stop on and off and an attention trace, with active logit rules and a truncation under a
    latent guide, with a contrast, and with rules from a prefix start state.  Every drawn token obeys the cut."""
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
    cut_any = proper = False
    for name, smp in SAMPLERS.items():
        ctx = dec.prepare(feats)
        con = make_contrast("features", variant).prepare(dec, ctx.feats)
        for what, kw, runs in (("alone", dict(), flags), ("rules+trunc+guide", dict(rules=rules, trunc=tr, guide=guide), flags[:2]),
                               ("contrast", dict(contrast=con), flags[:2]), ("rules+prefix", dict(rules=rules, start=True), flags[:1])):
            dkw = dict(kw)
            if dkw.get("start"):
                dkw["start"] = dec.prime(ctx, sent_b, NS, DecodePrefix(prefix), end, peps)
            want = drive(dec, ctx, sent_b, B, NS, STEPS, end, eps0, eps, smp, 13, miro=MIRO, **dkw)
            skw = {{"rules": "logit_rules", "trunc": "truncation"}.get(k, k): v for k, v in dkw.items()}
            for skip_dead, early_stop, attention in runs:
                out = dec.sample(ctx, sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=early_stop, attention=attention,
                                 skip_dead=skip_dead, mirostat=MIRO, mirostat_stats=True, **skw)
                pred, lp, (mu, sur, kept) = out[0], out[1], out[-1]
                tag = (variant, name, what, skip_dead, early_stop, attention)
                n = pred.size(1)
                assert mu.shape == sur.shape == kept.shape == pred.shape, tag
                assert torch.equal(padded(pred, STEPS, end), want[0]), tag
                assert torch.equal(bits(lp), bits(want[1])), (tag, (lp - want[1]).abs().max().item())
                assert torch.equal(bits(mu), bits(want[2][:, :n])), tag
                assert torch.equal(bits(padded_stats(sur, STEPS)), bits(want[3])), tag
                assert torch.equal(padded_stats(kept, STEPS), want[4]), tag
                if attention:
                    assert dec.attention(out[2]).top_region.shape == (B, STEPS)
            assert bool((want[2][:, 0] == MIRO.mu0_nats).all()), (variant, name, what)   # under a prefix too: mu0 at the continuation
            check_obeys((variant, name, what), want[0], want[2], want[3], want[5], end)
            live = want[4] > 0
            assert bool(live[:, 0].all()) and bool((want[4][live] <= V).all())
            finite = torch.isfinite(want[5]).sum(-1).t()
            cut_any |= bool((want[4][live] < finite[live]).any())
            proper |= bool(((want[4][live] < finite[live]) & (want[4][live] > 1)).any())
    assert cut_any, "Mirostat dropped nothing"
    if not VARIANTS[variant][0]:   # (the tied heads are not sharpened: the surprises of a nearly uniform row lie within a few hundredths)
        assert proper, "no cut between the top word alone and the whole row"


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_off_path_is_the_call_without_mirostat(variant):
    """mirostat=None, an inactive object and tau = 0 handed to ssc_decode_sample_mirostat itself give the predictions and the
    log-probs of ssc_decode_sample_opts, bit for bit - alone, under active logit rules, under a truncation and under a contrast."""
    cfg, _, _, dec = medium(variant)
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    ctx = dec.prepare(feats)
    rules = yardstick_rules(cfg.vocab_size, NIMG)
    con = make_contrast("features", variant).prepare(dec, ctx.feats)
    lib, seen = dec.lib, []
    dec.lib = Spy(lib, seen)
    try:
        for name, smp in SAMPLERS.items():
            args = (ctx, sent_b, NS, STEPS, cfg.boundary_index, eps0, eps, smp, 13)
            for kw in (dict(), dict(logit_rules=rules), dict(truncation=sampling.MinPTruncation(0.05)), dict(contrast=con)):
                pred0, lp0 = dec.sample(*args, **kw)
                for m, entry in ((None, "ssc_decode_sample_opts"), (sampling.Mirostat(0.0), "ssc_decode_sample_opts"),
                                 (ForcedOff(0.0), "ssc_decode_sample_mirostat")):
                    del seen[:]
                    pred, lp = dec.sample(*args, mirostat=m, **kw)
                    assert seen == [entry], (seen, entry)     # (without an active Mirostat the engine still makes the old call)
                    assert torch.equal(pred, pred0) and torch.equal(bits(lp), bits(lp0)), (variant, name, m, list(kw))
    finally:
        dec.lib = lib


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
ORACLE_TOL = 1e-4
ORACLE_MIRO = MIRO
# variant -> the seed of the inputs: one at which the restatement finds no undecidable token at band(t) on the oracle's logits
ORACLE_SEEDS = {"untied-sv1": 18, "untied-sv0-fp32": 18}   # (seeds 17 .. 24 tried; 17, the default: one token within the band on either)
ORACLE_VARIANTS = ("untied-sv1", "untied-sv0-fp32")   # (the tied heads are not sharpened: nearly uniform rows)


def oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, smp, m, seed=77):
    """The GPU's tokens teacher-forced through the oracle's decode step with the same noise; the restatement's control loop on the
    oracle's logits.  -> (max |summed edited log-prob, oracle - device|, max over t of |mu_t, oracle - device| / (1 + eta t),
    undecidable tokens over all live rows, the live (row, step) pairs cut between the top word alone and the whole row).  Asserts that every device token lies in the oracle-side kept set."""
    B = nimg * ns
    end = cfg.boundary_index
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B) if senti is not None else None
    pred, slp, (mu_d, _, _) = dec.sample(dec.prepare(feats.cuda()), sent_b.cuda() if sent_b is not None else None, ns, steps, end,
                                         eps0.cuda(), eps.cuda(), smp, seed, early_stop=False, mirostat=m, mirostat_stats=True)
    pred, slp, mu_d = pred.cpu(), slp.cpu(), mu_d.cpu().double().numpy()
    fr = feats.unsqueeze(1).expand(nimg, ns, feats.size(1), feats.size(2)).reshape(B, feats.size(1), -1)
    se = sent_b.view(B, 1) if sent_b is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
    states = zero_states(B, cfg.hidden_size, fr)
    tokens = torch.full((B,), end, dtype=torch.long)
    total = np.zeros(B)
    alive = np.ones(B, dtype=bool)
    undecidable = proper = 0
    T = float(smp.temperature)
    tau, eta = m.tau_nats, f32(m.eta)
    mu = np.full(B, m.mu0_nats, dtype=np.float64)
    worst_mu = 0.0
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
                worst_mu = max(worst_mu, abs(mu[b] - mu_d[b, t]) / (1 + eta * t))
                c = R.cut_row(logits[b], mu[b], T, R.band(t, eta))
                undecidable += len(c.undecidable)
                proper += int(1 < int(c.kept.sum()) < cfg.vocab_size)
                assert c.kept[tok] or tok in c.undecidable, (b, t, tok)
                row = np.where(c.kept, logits[b].astype(np.float64), -np.inf)
                mx = row.max()
                total[b] += row[tok] - (mx + np.log(np.exp(row - mx).sum()))
                mu[b] = mu[b] - eta * (-c.logq[tok] - tau)
            alive &= (pred[:, t] != end).numpy()
            tokens = pred[:, t].clone()
    return float(np.abs(total - slp.double().numpy()).max()), worst_mu, undecidable, proper


@pytest.mark.parametrize("variant", ORACLE_VARIANTS)
def test_mirostat_decode_against_the_oracle(variant):
    """Toy width (the medium model), multinomial: the restatement finds no undecidable token at band(t) on the oracle's logits for
    the chosen seeds (asserted), every device token lies in the oracle-side kept set (exact), |mu_t - oracle| <= (1 + eta t) 1e-4 and
    each caption's summed edited log-prob is within 1e-4 of the oracle's."""
    cfg, params = medium_params(variant)
    _, _, _, dec = medium(variant)
    seed = ORACLE_SEEDS.get(variant, 17)
    feats, senti, eps0, eps = entry_inputs(cfg, NIMG, NS, R_, seed, STEPS)
    worst, worst_mu, und, cut = oracle_check(cfg, params, dec, feats, senti, NIMG, NS, STEPS, eps0, eps, SAMPLERS["multinomial"], ORACLE_MIRO)
    print(f"{variant} seed {seed}: max |summed edited log-prob, oracle - device| {worst:.3e}, max |mu_t, oracle - device| / (1 + eta t) "
          f"{worst_mu:.3e}, undecidable {und}, proper cuts {cut}")
    assert und == 0, (variant, seed, und)
    assert cut > 0, "no proper cut on the oracle's side"
    assert worst_mu <= ORACLE_TOL, (variant, worst_mu)
    assert worst <= ORACLE_TOL, (variant, worst)


def test_mirostat_confines_the_draws_where_the_plain_decode_exceeds_the_threshold():
    """Multinomial sampling of 32 captions of up to 16 words on a fixed seed: the call without Mirostat draws tokens whose surprise
    exceeds the Mirostat run's mu_t at the same row and step (asserted, so that the check is not vacuous); the Mirostat call draws
    none such beyond the top-word exception."""
    cfg, _, _, dec = medium("untied-sv1")
    end, V = cfg.boundary_index, cfg.vocab_size
    nimg, ns, steps = 4, 8, 16
    B = nimg * ns
    feats, sent_b, eps0, eps = decode_inputs(cfg, seed=29, nimg=nimg, ns=ns, steps=steps)
    smp = sampling.MultinomialSampler(1.0)
    ctx = dec.prepare(feats)
    args = (ctx, sent_b, ns, steps, end, eps0, eps, smp, 41)
    plain, _ = dec.sample(*args, early_stop=False)
    tok, _, _, _, _, arrived = drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, smp, 41)
    assert torch.equal(tok, plain)
    cut, lp, (mu, sur, kept) = dec.sample(*args, early_stop=False, mirostat=MIRO, mirostat_stats=True)
    # the plain tokens' surprise under the plain run's own rows, against the Mirostat run's thresholds
    plain_sur = -torch.log_softmax(arrived.double(), -1).gather(2, plain.t().unsqueeze(-1)).squeeze(-1).t()
    live = live_columns(plain, end)
    first = first_max(arrived).t()
    outside = int((live & (plain_sur > mu.double()) & (plain != first)).sum())
    print(f"plain call: {outside} of {int(live.sum())} drawn tokens are more surprising than the Mirostat run's mu_t")
    assert outside >= 1
    got = drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, smp, 41, miro=MIRO, forced=cut)
    assert torch.equal(bits(got[2][:, :steps]), bits(mu)) and torch.equal(bits(got[3]), bits(sur))
    n, top_only = check_obeys("confine", cut, got[2], sur, got[5], end)
    print(f"Mirostat call: 0 of {n} drawn tokens above mu_t beyond the top-word exception ({top_only} by it); mean kept "
          f"{float(kept[kept > 0].float().mean()):.1f} of {V}, mean surprise {float(sur[kept > 0].mean()):.3f} nats at tau {MIRO.tau}")
    assert bool(torch.isfinite(lp).all()) and top_only < n, "every draw fell under the top-word exception"


# ---- the interface --------------------------------------------------------------------------------------------------------------------------
def test_diverse_decode_takes_a_mirostat():
    cfg, _, _, dec = medium("untied-sv1")
    feats, senti, _, _ = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    end = cfg.boundary_index
    kw = dict(sampler=sampling.MultinomialSampler(1.0), sample_seed=9)

    def run(**more):
        torch.manual_seed(3)
        return diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, **kw, **more)

    plain, _ = run()
    off, _ = run(mirostat=sampling.Mirostat(0.0))
    wide, _ = run(mirostat=sampling.Mirostat(1000.0, 0.0))           # a fixed cut above every surprise keeps every word
    greedy, k = run(mirostat=sampling.Mirostat(1.0, 0.0, mu0=-100.0))  # ... below every surprise: only the top word is left
    assert torch.equal(plain, off) and torch.equal(plain, wide)
    torch.manual_seed(3)
    top1, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, sampler=sampling.TopKSampler(k=1), sample_seed=9)
    assert torch.equal(greedy, top1) and greedy.size(-1) == k
    # the statistics in the object's unit: bits = nats / ln 2, the same bits of the device's blocks
    mb, mn = sampling.Mirostat(3.0, 0.1), sampling.Mirostat(3.0 * R.LN2, 0.1, mu0=6.0 * R.LN2, unit="nats")
    assert (mb.tau_nats, mb.mu0_nats) == (mn.tau_nats, mn.mu0_nats)
    cb, kb, (mu_b, sur_b, kept_b) = run(mirostat=mb, mirostat_stats=True)
    cn, _, (mu_n, sur_n, kept_n) = run(mirostat=mn, mirostat_stats=True)
    assert torch.equal(cb, cn) and torch.equal(kept_b, kept_n) and mu_b.shape == (NIMG, NS, kb) == sur_b.shape == kept_b.shape
    assert torch.equal(mu_b, mu_n / R.LN2) and torch.equal(sur_b, sur_n / R.LN2) and bool((mu_b[:, :, 0] == mu_n[:, :, 0] / R.LN2).all())
    assert float((mu_b[:, :, 0] - 6.0).abs().max()) < 1e-6
    # composes with logit rules, a truncation, a contrast, a guide, a prefix and an attention trace
    rules = sampling.LogitRules(no_repeat_ngram=1, min_length=3)
    prefix = DecodePrefix(torch.tensor([[5, 6], [7, -1], [-1, -1]]))
    caps, _ = run(mirostat=MIRO, logit_rules=rules, truncation=sampling.EtaTruncation(0.01), prefix=prefix)
    assert caps[0, :, :2].tolist() == [[5, 6]] * NS and caps[1, :, 0].tolist() == [7] * NS
    out = run(mirostat=MIRO, mirostat_stats=True, logit_rules=rules, attention="summary", contrast=make_contrast("features", "untied-sv1"),
              contrast_stats=True, guide=make_guide("var+len", NIMG * NS, cfg.z_space, STEPS, 5))
    assert out[2].top_region.shape[:2] == (NIMG, NS) and len(out[3]) == 2 and len(out[4]) == 3 and out[4][0].shape == out[0].shape
    for more, name in ((dict(sampler=None), "not the beam search"), (dict(sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                       (dict(sampled_beam=True), "sampled-node beam search"),
                       (dict(sampler=None, diverse_beam=sampling.DiverseBeam(1, 0.5)), "diverse beam search")):
        with pytest.raises(ValueError, match="Mirostat belongs to the word samplers.*" + name):
            diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, mirostat=MIRO, **{**kw, **more})


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", 3, "MODEL.DECODE_SAMPLER", "top-k", "MODEL.BEAM_SIZE", 1,
                            "MODEL.IMAGE_FEATURE_SIZE", 64, "MODEL.EMBEDDING_SIZE", 40, "MODEL.HIDDEN_SIZE", 48,
                            "MODEL.ATTENTION_PROJECTION_SIZE", 32, "MODEL.Z_SPACE", 16, "DATA.MAX_CAPTION_LENGTH", 8] + {keys!r})
def run(mirostat="config"):
    torch.manual_seed(C.RANDOM_SEED)
    m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                    sampler=sampling.from_config(C.MODEL)).cuda().eval()
    if mirostat != "config":
        m.mirostat(mirostat)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
    return m(feats)["predictions"].cpu().tolist()
print(json.dumps([run(), run(None), run(sampling.Mirostat(1.0, 0.0, mu0=-100.0)), run(sampling.Mirostat(1000.0, 0.0))]))
"""


def test_module_reads_the_keys_and_takes_a_mirostat_in_a_child_process():
    """The eval forward of a top-k (k = 3) module: with the keys at their defaults it is the forward without Mirostat; with
    MODEL.SAMPLER_MIROSTAT_TAU set it differs; mirostat(None) switches the keys' control off again; a fixed cut below every surprise
    leaves the most probable word of every step - the forward of a k = 1 module -, one above every surprise changes nothing."""
    pkg = os.path.join(ROOT, "style-seqcvae_amd")
    outs = {}
    for name, keys in (("off", ["MODEL.SAMPLER_TOP_K", 3]),
                       ("on", ["MODEL.SAMPLER_TOP_K", 3, "MODEL.SAMPLER_MIROSTAT_TAU", 0.25, "MODEL.SAMPLER_MIROSTAT_ETA", 1.0]),
                       ("k1", ["MODEL.SAMPLER_TOP_K", 1])):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=pkg, keys=keys)
        outs[name] = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    plain, plain_none, plain_low, plain_high = outs["off"]
    keyed, keyed_none, keyed_low, _ = outs["on"]
    greedy = outs["k1"][0]
    assert plain == plain_none == keyed_none == plain_high
    assert keyed != plain
    assert plain_low == keyed_low == greedy


SCRIPT_YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
               "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
               "  BEAM_SIZE: 1\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
               "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n  DECODE_SAMPLER: top-k\n  SAMPLER_TOP_K: 4\n")


def test_inference_script_with_the_mirostat_flags(tmp_path):
    """scripts/inference.py: --mirostat 1000:0 (the kernels run, a fixed cut that keeps every word) writes the bytes of the run
    without the flag; --mirostat-output writes per caption the mu and surprise traces in bits; the keys stand in for the flag; the
    flag without a word sampler is refused."""
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
    trace = tmp_path / "trace.json"
    assert run("wide", "--mirostat", "1000:0", "--mirostat-output", str(trace)) == plain
    recs = json.loads(trace.read_text())
    caps = json.loads(plain)
    assert len(recs) == len(caps) == 4 * 5 and [r["caption"] for r in recs] == [c["caption"] for c in caps]
    for r in recs:
        n = len(r["caption"].split())
        assert len(r["mu"]) == len(r["surprise"]) == min(n + 1, 8) and all(abs(v - 2000.0) < 1e-3 for v in r["mu"]) and all(v > 0 for v in r["surprise"])
    on = run("on", "--mirostat", "0.5:1")
    assert on != plain and len(json.loads(on)) == 4 * 5
    assert on == run("keys", "--config-override", "MODEL.SAMPLER_MIROSTAT_TAU", "0.5", "MODEL.SAMPLER_MIROSTAT_ETA", "1.0")
    r = subprocess.run([sys.executable] + base + ["--output-path", str(tmp_path / "x.json"), "--mirostat", "3", "--config-override",
                                                  "MODEL.DECODE_SAMPLER", "beam"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--mirostat needs a word sampler" in r.stderr, r.stderr[-2000:]
