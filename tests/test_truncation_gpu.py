"""GPU: the truncation of the word samplers (include/ssc.h: ssc_truncation).  The kernel (ssc_truncate_rows) against the float64
restatement (tests/truncationref.py) on inputs the restatement calls decidable; the distribution the draw is then made from; the
sampled decode under a truncation (ssc_sample_opts.trunc, DecodeEngine.sample) against the call without it, against the same
decode driven step by step and against the CPU oracle; diverse_decode, the module and scripts/inference.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import oracle
import truncationref as R
from gpuutil import engine_from
from oracle.seqcvae_oracle import cell_step, embed, output_logits, zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.inference import diverse_decode
from ssc_runtime.prefix import DecodePrefix
from test_attention_trace_gpu import R_, STEPS, VARIANTS, entry_inputs, medium, medium_params
from test_latent_guide_gpu import bits, make_guide, step_prior
from test_logit_rules_gpu import GUARD, SENTINEL, decode_inputs, padded, placed, yardstick_rules
from test_sampling_gpu import chi2_pvalue, fixture, run_child, sample_rows
from test_sampling_gpu import inputs as wide_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1
ENTROPY_TOL = 1e-4      # the project's parity tolerance
KINDS = {"typical": 1, "min-p": 2, "eta": 3, "epsilon": 4}


def f32(v):
    """the value the library reads: the float32 nearest to v"""
    return float(np.float32(v))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
ROWS_VALUE = {1: 0.87654, 2: 0.05, 3: 3e-4, 4: 3e-4}   # (tau such that tau * V is no integer for any V below: a flat row is decidable)
SHAPES = [(37, 37, 0), (451, 452, 1), (1024, 1028, 1), (2003, 2004, 0), (10000, 10000, 0), (32768, 32768, 0), (32769, 32772, 1),
          (40000, 40000, 0)]   # (V, ld, offset in floats past a 16-byte boundary); 32768 is the last V of the LDS form
TEMPS = (0.7, 1.0, 1.3)
N_ROWS = 7
LIVE = (0, 1, 2, 3, 4)
# per (V, kind, T): the first seed offset at which the restatement finds no undecidable token (found on the CPU with rows_case alone)
ROW_SEEDS = {(451, 1, 0.7): 3, (1024, 1, 0.7): 5, (2003, 1, 0.7): 1, (2003, 1, 1.0): 1, (2003, 1, 1.3): 1, (32768, 3, 1.3): 3,
             (32769, 1, 1.0): 2, (32769, 1, 1.3): 2, (32769, 4, 1.0): 1, (40000, 1, 0.7): 3, (40000, 1, 1.0): 1, (40000, 3, 1.3): 2}


def rows_case(V, ld, kind, T, seed):
    """Seven rows: random; peaked (one token holds nearly all the mass); flat; values on a grid of 0.5 with the maximum three times
    - exact ties at the cut and at the top; 30 % of the entries -inf; an ended row full of NaN; a row without a finite entry.  The
    pad columns are NaN.  -> (x (7, ld) float32, last_pred (7,) int64)"""
    rng = np.random.default_rng(seed)
    x = np.full((N_ROWS, ld), np.nan, dtype=np.float32)
    x[0, :V] = rng.standard_normal(V) * 3
    x[1, :V] = rng.standard_normal(V)
    x[1, V // 3] = 25.0
    x[2, :V] = -1.25
    x[3, :V] = np.round(rng.standard_normal(V) * 3 * 2) / 2
    x[3, [1, V // 2, V - 1]] = x[3, :V].max() + 0.5
    x[4, :V] = rng.standard_normal(V) * 3
    x[4, :V][rng.random(V) < 0.3] = -np.inf
    x[6, :V] = -np.inf
    last = np.full(N_ROWS, 7, dtype=np.int64)
    last[5] = END
    return x, last


def row_seed(V, kind, T):
    return 1000 * V + 10 * kind + int(T * 10) * 100000 + ROW_SEEDS.get((V, kind, T), 0) * 7919


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD: GUARD + n]


def run_truncate(view, ld, rows, V, kind, value, T, last_d, ent=None, kept=None):
    t = L.Truncation(kind, value, ent.data_ptr() if ent is not None else None, kept.data_ptr() if kept is not None else None)
    L.load().ssc_truncate_rows(view.data_ptr(), ld, rows, V, C.byref(t), T, L.ptr(last_d), END, L.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("V,ld,off", SHAPES)
def test_rows_kernel_against_the_restatement(V, ld, off, kind):
    """Per temperature in {0.7, 1, 1.3}: the restatement finds no undecidable token in the inputs (asserted first); then the kept sets
    are EQUAL to its own - the whole buffer is bit-equal to the restatement's edit: kept entries keep their bits, the others are -inf,
    the ended row (NaN), the row without a finite entry, the poisoned pad columns and the guard words are untouched -, `kept` is
    exact, `entropy` within 1e-4, the guards of both statistics intact; two calls are bit-equal; NULL outputs change nothing;
    kind 0 changes nothing at all.  V = 1024: the 16-byte path (offset 0) gives the bits of the scalar path (offset 1)."""
    k = KINDS[kind]
    value = f32(ROWS_VALUE[k])
    for T in TEMPS:
        x, last = rows_case(V, ld, k, T, row_seed(V, k, T))
        want, ent_ref, kept_ref, und = R.edit_rows(x, V, k, value, T, last, END)
        tag = (V, ld, off, kind, T)
        assert und == [], (tag, und[:5])
        cut_row = R.truncate_row(x[3, :V], k, value, T)
        if k == 1 and V >= 451:   # the cut of the grid row falls inside a run of equal values: the index rule decides
            same = x[3, :V] == x[3, cut_row.cut]
            assert cut_row.kept[same].any() and not cut_row.kept[same].all(), tag
        flat, view = placed(x, off)
        before = flat.clone()
        last_d = torch.from_numpy(last).cuda()
        ent_buf, ent = guarded(N_ROWS, torch.float32, SENTINEL)
        kept_buf, kept = guarded(N_ROWS, torch.int32, -99)
        expect = before.clone()
        expect[GUARD + off: GUARD + off + x.size] = torch.from_numpy(want).reshape(-1).cuda()
        outs = []
        for _ in range(2):   # two calls on equal inputs
            flat.copy_(before)
            ent_buf.fill_(SENTINEL)
            kept_buf.fill_(-99)
            run_truncate(view, ld, N_ROWS, V, k, value, T, last_d, ent, kept)
            outs.append((flat.clone(), ent_buf.clone(), kept_buf.clone()))
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(bits(a), bits(b)), tag
        got = outs[0][0]
        if not torch.equal(bits(got), bits(expect)):
            g = got[GUARD + off: GUARD + off + x.size].view(N_ROWS, ld).cpu().numpy()
            bad = np.argwhere(g.view(np.int32) != want.view(np.int32))
            i, v = bad[0]
            c = R.truncate_row(x[i, :V], k, value, T)
            raise AssertionError(f"{tag}: {len(bad)} elements differ, first at row {i} column {v}: got {g[i, v]!r}, want {want[i, v]!r}, "
                                 f"input {x[i, v]!r}, d or log q {c.d[v] if v < V else None!r} (cut {c.cut}: {c.d[c.cut] if c.cut >= 0 else None!r}); "
                                 f"guards intact: {torch.equal(bits(got[:GUARD]), bits(before[:GUARD]))}")
        assert bool((outs[0][1][:GUARD] == SENTINEL).all()) and bool((outs[0][1][-GUARD:] == SENTINEL).all()), tag
        assert bool((outs[0][2][:GUARD] == -99).all()) and bool((outs[0][2][-GUARD:] == -99).all()), tag
        kept_got = outs[0][2][GUARD: GUARD + N_ROWS].cpu().numpy()
        ent_got = outs[0][1][GUARD: GUARD + N_ROWS].cpu().numpy().astype(np.float64)
        assert kept_got.tolist() == kept_ref.tolist(), tag
        err = np.abs(ent_got - ent_ref)
        print(f"{tag}: kept {kept_got.tolist()}, max |entropy - float64| {err.max():.2e}")
        assert err.max() <= ENTROPY_TOL, (tag, err)
        assert ent_got[5] == 0.0 and ent_got[6] == 0.0
        flat.copy_(before)
        run_truncate(view, ld, N_ROWS, V, k, value, T, last_d)            # no statistics asked for
        assert torch.equal(bits(flat), bits(expect)), tag
        flat.copy_(before)
        ent_buf.fill_(SENTINEL)
        run_truncate(view, ld, N_ROWS, V, 0, value, T, last_d, ent, kept)   # off
        assert torch.equal(bits(flat), bits(before)) and bool((ent_buf == SENTINEL).all()), tag
        if V == 1024:
            flat0, view0 = placed(x, 0)
            run_truncate(view0, ld, N_ROWS, V, k, value, T, last_d, ent, kept)
            assert torch.equal(bits(view0), bits(got[GUARD + off: GUARD + off + x.size].view(N_ROWS, ld))), tag
            assert torch.equal(bits(ent_buf), bits(outs[0][1])) and torch.equal(kept_buf, outs[0][2]), tag


# ---- the distribution the draw is made from -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_truncated_rows_give_the_renormalised_distribution(kind):
    """ssc_sample_rows (multinomial, probs_out) on truncated rows against the float64 distribution renormalised over the
    restatement's kept set: rtol 3e-6 / atol 1e-6, samplerref's tolerances."""
    k = KINDS[kind]
    value = f32(ROWS_VALUE[k])
    for V in (451, 10000):
        for T in TEMPS:
            x, _ = rows_case(V, V, k, T, row_seed(V, k, T))
            x = x[list(LIVE)]
            cuts = [R.truncate_row(x[r], k, value, T) for r in range(len(LIVE))]
            assert all(c.undecidable == [] for c in cuts), (V, kind, T)
            x_d = torch.from_numpy(x).cuda()
            run_truncate(x_d, V, len(LIVE), V, k, value, T, None)
            _, _, po = sample_rows(x_d, sampling.MultinomialSampler(temperature=T), seed=5, probs=True)
            for r, c in enumerate(cuts):
                want = R.renormalised(x[r], c.kept, T)
                np.testing.assert_allclose(po[r].double().numpy(), want, rtol=3e-6, atol=1e-6, err_msg=str((V, kind, T, r)))


CHI_VALUE = {1: 0.7, 2: 0.1, 3: 0.05, 4: 0.02}


@pytest.mark.parametrize("kind,r", [("typical", 1), ("min-p", 2), ("eta", 2), ("epsilon", 1)])
def test_draw_frequencies_follow_the_truncated_distribution(kind, r):
    """65 536 copies of one fixture row (V = 50) with distinct row ids, truncated, then drawn (multinomial): chi-square of the token
    counts against the float64 renormalised distribution, p > 1e-3 (fixed seed: deterministic) - the procedure and the bound of
    test_draw_frequencies_follow_the_reference_distribution.  The cut is a proper one: more than one token kept, not all."""
    k = KINDS[kind]
    value = f32(CHI_VALUE[k])
    d, _ = fixture()
    row = d["lp_V50"][r]
    c = R.truncate_row(row, k, value, 1.0)
    assert c.undecidable == [] and 1 < int(c.kept.sum()) < 50, (kind, int(c.kept.sum()))
    ref = R.renormalised(row, c.kept, 1.0)
    n = 65536
    logits = torch.from_numpy(row).view(1, 50).expand(n, 50).contiguous().cuda()
    run_truncate(logits, 50, n, 50, k, value, 1.0, None)
    tok, _, _ = sample_rows(logits, sampling.MultinomialSampler(1.0), seed=20251015, step=2)
    counts = np.bincount(tok.numpy(), minlength=50).astype(np.float64)
    assert counts[ref == 0].sum() == 0
    exp = ref * n
    big = exp >= 5
    obs_b = np.append(counts[big], counts[~big & (ref > 0)].sum())
    exp_b = np.append(exp[big], exp[~big & (ref > 0)].sum())
    keep = exp_b > 0
    x2 = (((obs_b - exp_b) ** 2)[keep] / exp_b[keep]).sum()
    dof = max(int(keep.sum()) - 1, 1)
    assert chi2_pvalue(x2, dof) > 1e-3, (kind, x2, dof)


# ---- the decode ---------------------------------------------------------------------------------------------------------------------------
SAMPLERS = {"multinomial": sampling.MultinomialSampler(1.0), "top-k": sampling.TopKSampler(k=3), "top-p": sampling.TopPSampler(p=0.9, temperature=1.2)}
TRUNCATIONS = {"typical": sampling.TypicalTruncation(0.9), "min-p": sampling.MinPTruncation(0.05), "eta": sampling.EtaTruncation(0.01),
               "epsilon": sampling.EpsilonTruncation(0.01)}
NIMG, NS = 3, 2


class ForcedOff(sampling.Truncation):
    """A kind-0 truncation that DecodeEngine.sample hands to ssc_decode_sample_opts (as its trunc) all the same"""
    active = True


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_off_path_is_the_call_without_a_truncation(variant):
    """truncation=None and kind 0 - handed to DecodeEngine.sample, and handed to ssc_decode_sample_opts itself - give the predictions
    and the log-probs of the call without the argument, bit for bit; so does the kind-0 descriptor under active logit rules against
    the call with those rules alone."""
    cfg, _, _, dec = medium(variant)
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    ctx = dec.prepare(feats)
    rules = yardstick_rules(cfg.vocab_size, NIMG)
    for name, smp in SAMPLERS.items():
        args = (ctx, sent_b, NS, STEPS, cfg.boundary_index, eps0, eps, smp, 13)
        for kw in (dict(), dict(logit_rules=rules)):
            pred0, lp0 = dec.sample(*args, **kw)
            for tr in (None, sampling.Truncation(), ForcedOff()):
                pred, lp = dec.sample(*args, truncation=tr, **kw)
                assert torch.equal(pred, pred0) and torch.equal(bits(lp), bits(lp0)), (variant, name, tr, list(kw))


def drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, sampler, seed, trunc=None, rules=None, guide=None, start=None, probe=None,
          forced=None):
    """The sampled decode driven from Python: DecodeEngine.step, ssc_logit_rules_rows, ssc_truncate_rows, ssc_sample_rows per step.
    probe: a truncation applied to a COPY of every step's logits - was the step's token inside its kept set?  forced (B, steps): the
    tokens are given instead of drawn.  -> (tokens (B, steps), log-probs (B), entropy (B, steps), kept (B, steps), inside (B, steps))"""
    lib = L.load()
    V = dec.dims.V
    T = float(sampler.temperature)
    sdesc = sampler.desc(seed)
    rd = rules.desc(ns) if rules is not None else None
    run = torch.zeros(B, device="cuda")
    hist = torch.full((steps, B), -1, dtype=torch.int64, device="cuda")
    ent = torch.zeros(steps, B, device="cuda")
    kept = torch.zeros(steps, B, dtype=torch.int32, device="cuda")
    inside = torch.ones(steps, B, dtype=torch.bool, device="cuda")
    if start is None:
        tokens, state = torch.full((B,), end, dtype=torch.int64, device="cuda"), None
    else:
        tokens = start.tokens.clone()
        tokens[(tokens < 0) | (tokens >= V)] = end
        state = dec.zero_states(B)
        state.update(h1=start.h1, c1=start.c1, h_decoder=start.hd, c_decoder=start.cd)
    last = None
    for t in range(steps):
        pm, pv = step_prior(guide, t, B, 1, sent_b, dec.dims)
        logits, state, _ = dec.step(ctx, tokens, state, sent_b, eps0 if t == 0 else eps[t - 1], raw_logits=True, prior_mean=pm, prior_var=pv)
        if rd is not None:
            lib.ssc_logit_rules_rows(L.ptr(logits), V, B, V, C.byref(rd[0]), L.ptr(hist), B, t, end, L.stream_ptr())
        copy = None
        if probe is not None:
            copy = logits.clone()
            pd = probe.desc()
            lib.ssc_truncate_rows(L.ptr(copy), V, B, V, C.byref(pd), T, L.ptr(last), end, L.stream_ptr())
        if trunc is not None:
            td = trunc.desc(ent[t], kept[t])
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
    return hist.t().contiguous(), run, ent.t().contiguous(), kept.t().contiguous(), inside.t().contiguous()


def padded_stats(s, steps):
    return torch.nn.functional.pad(s, (0, steps - s.size(1)), value=0)


@pytest.mark.parametrize("kind", list(TRUNCATIONS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_truncated_decode_against_the_stepwise_driver(variant, kind):
    """The one call gives the tokens, the log-probs and both statistics blocks of the same decode driven step by step -
    DecodeEngine.step, ssc_logit_rules_rows, ssc_truncate_rows, ssc_sample_rows - bit for bit: each sampler, alone with skip_dead /
    early_stop on and off and an attention trace, with active logit rules under a latent guide, and with them from a prefix start
    state.  On the sharpened (untied) heads the truncation drops entries in every configuration."""
    cfg, _, _, dec = medium(variant)
    end, V = cfg.boundary_index, cfg.vocab_size
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    B = NIMG * NS
    tr = TRUNCATIONS[kind]
    rules = yardstick_rules(V, NIMG)
    guide = make_guide("var+len", B, cfg.z_space, STEPS, 5)
    g = torch.Generator().manual_seed(3)
    prefix = torch.full((NIMG, 2), -1, dtype=torch.int64)
    prefix[1, :1] = torch.randint(2, V, (1,), generator=g)
    prefix[2, :2] = torch.randint(2, V, (2,), generator=g)
    peps = torch.randn(2, B, cfg.z_space, generator=g).cuda()
    flags = ((True, True, False), (False, False, False), (True, False, True), (False, True, False))
    for name, smp in SAMPLERS.items():
        for what, kw, runs in (("alone", dict(), flags), ("rules+guide", dict(rules=rules, guide=guide), flags[:2]),
                               ("rules+prefix", dict(rules=rules, start=True), flags[:1])):
            ctx = dec.prepare(feats)
            dkw = dict(kw)
            if dkw.get("start"):
                dkw["start"] = dec.prime(ctx, sent_b, NS, DecodePrefix(prefix), end, peps)
            want = drive(dec, ctx, sent_b, B, NS, STEPS, end, eps0, eps, smp, 13, trunc=tr, **dkw)
            skw = {("logit_rules" if k == "rules" else k): v for k, v in dkw.items()}
            for skip_dead, early_stop, attention in runs:
                out = dec.sample(ctx, sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=early_stop, attention=attention,
                                 skip_dead=skip_dead, truncation=tr, truncation_stats=True, **skw)
                pred, lp, (ent, kept) = out[0], out[1], out[-1]
                tag = (variant, kind, name, what, skip_dead, early_stop, attention)
                assert ent.shape == kept.shape == pred.shape, tag
                assert torch.equal(padded(pred, STEPS, end), want[0]), tag
                assert torch.equal(bits(lp), bits(want[1])), (tag, (lp - want[1]).abs().max().item())
                assert torch.equal(bits(padded_stats(ent, STEPS)), bits(want[2])), tag
                assert torch.equal(padded_stats(kept, STEPS), want[3]), tag
                if attention:
                    assert dec.attention(out[2]).top_region.shape == (B, STEPS)
            live = want[3] > 0
            assert bool(live[:, 0].all()) and bool((want[3][live] <= V).all()) and bool((want[2][~live] == 0).all())
            if not VARIANTS[variant][0]:   # (the tied heads are not sharpened: eta and epsilon keep their nearly uniform rows whole)
                assert bool((want[3][live] < V).any()), "the truncation dropped nothing"


def oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, smp, tr, seed=77):
    """The GPU's tokens teacher-forced through the oracle's decode step with the same noise; the restatement's truncation on the
    oracle's logits.  -> (max over the captions of |summed edited log-prob, oracle - device|, undecidable tokens over all live rows,
    device tokens among them).  Asserts that every other device token lies in the oracle-side kept set."""
    B = nimg * ns
    end = cfg.boundary_index
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B) if senti is not None else None
    pred, slp = dec.sample(dec.prepare(feats.cuda()), sent_b.cuda() if sent_b is not None else None, ns, steps, end, eps0.cuda(), eps.cuda(),
                           smp, seed, early_stop=False, truncation=tr)
    pred, slp = pred.cpu(), slp.cpu()
    fr = feats.unsqueeze(1).expand(nimg, ns, feats.size(1), feats.size(2)).reshape(B, feats.size(1), -1)
    se = sent_b.view(B, 1) if sent_b is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
    states = zero_states(B, cfg.hidden_size, fr)
    tokens = torch.full((B,), end, dtype=torch.long)
    total = np.zeros(B)
    alive = np.ones(B, dtype=bool)
    undecidable = exempt = 0
    value, T = f32(tr.value), float(smp.temperature)
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
                c = R.truncate_row(logits[b], tr.kind, value, T)
                undecidable += len(c.undecidable)
                if tok in c.undecidable:
                    exempt += 1
                    continue
                assert c.kept[tok], (b, t, tok)
                row = np.where(c.kept, logits[b].astype(np.float64), -np.inf)
                mx = row.max()
                total[b] += row[tok] - (mx + np.log(np.exp(row - mx).sum()))
            alive &= (pred[:, t] != end).numpy()
            tokens = pred[:, t].clone()
    return float(np.abs(total - slp.double().numpy()).max()), undecidable, exempt


ORACLE_TOL = 1e-4   # the sampled decode's tolerance against the oracle: the edit only removes entries, it scales no error
# (variant, kind) -> the seed of the inputs: one at which the restatement finds no undecidable token on the oracle's logits
ORACLE_SEEDS = {("untied-sv0-fp32", "min-p"): 19}   # (seed 17, the default: one token within the band there)
ORACLE_VARIANTS = ("untied-sv1", "untied-sv0-fp32")   # (the tied heads are not sharpened: nearly uniform rows, every cut undecidable)


@pytest.mark.parametrize("kind", list(TRUNCATIONS))
@pytest.mark.parametrize("variant", ORACLE_VARIANTS)
def test_truncated_decode_against_the_oracle(variant, kind):
    """Toy width (the medium model), multinomial: the restatement finds no undecidable token on the oracle's logits for the chosen
    seeds (asserted), every device token lies in the oracle-side kept set (exact) and each caption's summed edited log-prob is
    within 1e-4 of the oracle's."""
    cfg, params = medium_params(variant)
    _, _, _, dec = medium(variant)
    seed = ORACLE_SEEDS.get((variant, kind), 17)
    feats, senti, eps0, eps = entry_inputs(cfg, NIMG, NS, R_, seed, STEPS)
    worst, und, exempt = oracle_check(cfg, params, dec, feats, senti, NIMG, NS, STEPS, eps0, eps, SAMPLERS["multinomial"], TRUNCATIONS[kind])
    print(f"{variant} {kind} seed {seed}: max |summed edited log-prob, oracle - device| {worst:.3e}, undecidable {und} (drawn {exempt})")
    assert und == 0 and exempt == 0, (variant, kind, seed, und, exempt)
    assert worst <= ORACLE_TOL, (variant, kind, worst)


# The output layer scaled by 32 and input seed 359: the first of the seeds 100 .. 1299 at which the restatement finds no undecidable
# token in the 36 rows (measured on one MI355X: 3 such seeds in 858 tried, 5.1 undecidable tokens per seed on average; at a scale of
# 8 none in 1200, 9.7 on average)
WIDE_SHARP = 32.0
WIDE_SEED = 359


@functools.lru_cache(maxsize=None)
def sharp_wide_model(sharp=WIDE_SHARP):
    """Full width with the output layer scaled (as initialised the rows are nearly uniform over 10 000 words: every cut undecidable)"""
    cfg = oracle.OracleConfig(vocab_size=10000, image_feature_size=2048, embedding_size=1000, hidden_size=1200,
                              attention_projection_size=768, z_space=128, max_caption_length=20, sentiment_vae=1,
                              senti_prior_multip=0.5, beam_size=1)
    params = {k: v.clone() for k, v in oracle.init_params(cfg, seed=4).items()}
    params["_output_layer.weight"] *= sharp
    eng = engine_from(cfg, params)
    return cfg, params, eng, DecodeEngine(eng.dims, eng.params.c_struct, "cuda")


def test_full_width_truncated_decode_against_the_oracle():
    """Full width (H 1200, V 10 000, R 36; 2 images x 3 samples, 6 steps), typical: the same three checks."""
    cfg, params, _, dec = sharp_wide_model()
    nimg, ns, R36, steps = 2, 3, 36, 6
    feats, senti, eps0, eps = wide_inputs(cfg, nimg, ns, R36, seed=WIDE_SEED, steps=steps)
    worst, und, exempt = oracle_check(cfg, params, dec, feats, senti, nimg, ns, steps, eps0, eps, sampling.MultinomialSampler(1.0),
                                      sampling.TypicalTruncation(0.9))
    print(f"full width typical seed {WIDE_SEED}: max |summed edited log-prob, oracle - device| {worst:.3e}, undecidable {und} (drawn {exempt})")
    assert und == 0 and exempt == 0, (und, exempt)
    assert worst <= ORACLE_TOL, worst


def test_typical_truncation_confines_the_draws_where_the_plain_decode_leaves_the_set():
    """Multinomial sampling of 32 captions of up to 16 words on a fixed seed: the call without a truncation draws at least one token
    outside its step's typical set (tau = 0.9; asserted, so that the check is not vacuous), the truncated call none; its mean
    `kept` over the live steps is below V."""
    cfg, _, _, dec = medium("untied-sv1")
    end, V = cfg.boundary_index, cfg.vocab_size
    nimg, ns, steps = 4, 8, 16
    B = nimg * ns
    feats, sent_b, eps0, eps = decode_inputs(cfg, seed=29, nimg=nimg, ns=ns, steps=steps)
    smp, tr = sampling.MultinomialSampler(1.0), sampling.TypicalTruncation(0.9)
    ctx = dec.prepare(feats)
    args = (ctx, sent_b, ns, steps, end, eps0, eps, smp, 41)
    plain, _ = dec.sample(*args, early_stop=False)
    tok, _, _, _, inside = drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, smp, 41, probe=tr)
    assert torch.equal(tok, plain)
    outside = int((~inside).sum())
    print(f"plain call: {outside} of {int((plain != end).sum()) + B} drawn tokens lie outside their step's typical set")
    assert outside >= 1
    cut, lp, (ent, kept) = dec.sample(*args, early_stop=False, truncation=tr, truncation_stats=True)
    _, _, _, _, inside = drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, smp, 41, probe=tr, forced=cut)
    assert bool(inside.all()) and bool(torch.isfinite(lp).all())
    live = kept > 0
    mean_kept = float(kept[live].float().mean())
    print(f"truncated call: mean kept {mean_kept:.1f} of {V}, mean entropy {float(ent[live].mean()):.3f} nats")
    assert bool(live[:, 0].all()) and mean_kept < V and bool((ent[live] > 0).all())


# ---- the interface --------------------------------------------------------------------------------------------------------------------------
def test_diverse_decode_takes_a_truncation():
    cfg, _, _, dec = medium("untied-sv1")
    feats, senti, _, _ = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    end = cfg.boundary_index
    kw = dict(sampler=sampling.MultinomialSampler(1.0), sample_seed=9)

    def run(**more):
        torch.manual_seed(3)
        return diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, **kw, **more)

    plain, _ = run()
    off, _ = run(truncation=sampling.Truncation())
    one, _ = run(truncation=sampling.TypicalTruncation(1.0))     # tau = 1 keeps every word
    greedy, k = run(truncation=sampling.MinPTruncation(1.0))     # only the most probable word is left
    assert torch.equal(plain, off) and torch.equal(plain, one)
    assert greedy.shape[:2] == (NIMG, NS) and greedy.size(-1) == k and not torch.equal(padded(greedy.view(NIMG * NS, -1), STEPS, end),
                                                                                       padded(plain.view(NIMG * NS, -1), STEPS, end))
    torch.manual_seed(3)
    top1, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, sampler=sampling.TopKSampler(k=1), sample_seed=9)
    assert torch.equal(greedy, top1)
    # composes with logit rules, a prefix and an attention trace
    rules = sampling.LogitRules(no_repeat_ngram=1, min_length=3)
    prefix = DecodePrefix(torch.tensor([[5, 6], [7, -1], [-1, -1]]))
    caps, _ = run(truncation=sampling.EtaTruncation(0.01), logit_rules=rules, prefix=prefix)
    assert caps[0, :, :2].tolist() == [[5, 6]] * NS and caps[1, :, 0].tolist() == [7] * NS
    out = run(truncation=sampling.EpsilonTruncation(0.01), logit_rules=rules, attention="summary")
    assert out[-1].top_region.shape[:2] == (NIMG, NS)
    for more, name in ((dict(sampler=None), "not the beam search"), (dict(sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                       (dict(sampled_beam=True), "sampled-node beam search"),
                       (dict(sampler=None, diverse_beam=sampling.DiverseBeam(1, 0.5)), "diverse beam search")):
        with pytest.raises(ValueError, match="truncation belongs to the word samplers.*" + name):
            diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, truncation=sampling.TypicalTruncation(),
                           **{**kw, **more})


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
def run(truncation="config"):
    torch.manual_seed(C.RANDOM_SEED)
    m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                    sampler=sampling.from_config(C.MODEL)).cuda().eval()
    if truncation != "config":
        m.truncation(truncation)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
    return m(feats)["predictions"].cpu().tolist()
print(json.dumps([run(), run(None), run(sampling.MinPTruncation(1.0))]))
"""


def test_module_reads_the_keys_and_takes_a_truncation_in_a_child_process():
    """The eval forward of a top-k (k = 3) module: with the keys at their defaults it is the forward without a truncation; with
    MODEL.SAMPLER_TRUNCATION min-p at value 1 only the most probable word of every step is left - the forward of a k = 1 module;
    truncation(None) switches the keys' truncation off again and truncation(t) sets another."""
    pkg = os.path.join(ROOT, "style-seqcvae_amd")
    outs = {}
    for name, keys in (("off", ["MODEL.SAMPLER_TOP_K", 3]),
                       ("on", ["MODEL.SAMPLER_TOP_K", 3, "MODEL.SAMPLER_TRUNCATION", "min-p", "MODEL.SAMPLER_TRUNCATION_VALUE", 1.0]),
                       ("k1", ["MODEL.SAMPLER_TOP_K", 1])):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=pkg, keys=keys)
        outs[name] = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    plain, plain_none, plain_set = outs["off"]
    keyed, keyed_none, _ = outs["on"]
    greedy = outs["k1"][0]
    assert plain == plain_none == keyed_none
    assert keyed != plain
    assert keyed == plain_set == greedy


SCRIPT_YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
               "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
               "  BEAM_SIZE: 1\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
               "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n  DECODE_SAMPLER: top-k\n  SAMPLER_TOP_K: 4\n")


def test_inference_script_with_the_truncation_flag(tmp_path):
    """scripts/inference.py: --truncation typical:1 (the kernel runs, every word is kept) writes the bytes of the run without the
    flag; --truncation min-p:1 writes those of a top-1 run; the flag without a word sampler is refused."""
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
    assert run("tau1", "--truncation", "typical:1") == plain
    greedy = run("minp1", "--truncation", "min-p:1")
    assert greedy != plain and len(json.loads(greedy)) == 4 * 5
    assert greedy == run("top1", "--config-override", "MODEL.SAMPLER_TOP_K", "1")
    assert greedy == run("keys", "--config-override", "MODEL.SAMPLER_TRUNCATION", "min-p", "MODEL.SAMPLER_TRUNCATION_VALUE", "1.0")
    r = subprocess.run([sys.executable] + base + ["--output-path", str(tmp_path / "x.json"), "--truncation", "typical:0.9", "--config-override",
                                                  "MODEL.DECODE_SAMPLER", "beam"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--truncation needs a word sampler" in r.stderr, r.stderr[-2000:]
