"""GPU: the beam search under the decode rules - n-gram blocking, minimum length, suppressed tokens, length penalty
(ssc_beam_first_rules / ssc_beam_step_rules, ssc_decode_rules_beam, DecodeEngine.rules_beam, diverse_decode / UpDownCaptioner /
scripts/inference.py with MODEL.NO_REPEAT_NGRAM and its sister keys) against the numpy float32 restatement of its definition
(tests/rulesref.py: bit-exact), the plain beam search (rules off), a search driven step by step from Python, and the CPU oracle's
decode step."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import oracle
import rulesref as R
from oracle.seqcvae_oracle import zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from test_dbs_gpu import MARGIN, ORACLE_CASES, _entry_inputs, device_log_softmax, make_rows, same_bits, same_values, sharp_model
from test_sampling_gpu import ROOT, inputs, model, run_child

pytestmark = pytest.mark.gpu

F = np.float32
WORDS = np.arange(2, 8)   # the 6 distinct words the fed histories are drawn from, so that n-grams do repeat


def desc_of(rules):
    """rulesref.Rules -> the C struct"""
    d = L.RulesDesc()
    d.no_repeat_ngram, d.min_length, d.n_suppress = rules.n, rules.m, len(rules.suppress)
    for i, v in enumerate(rules.suppress):
        d.suppress[i] = v
    for i, v in enumerate(rules.table):
        d.length_penalty[i] = float(v)
    return d


class Steps:
    """The two stand-alone steps on device buffers: B entries of k beams, n candidates per beam.  Every output starts from a fill
    value, so that a refused call can be seen to have written nothing."""

    def __init__(self, B, k, n, V, raw, end=R.END, ld=None, ld_hist=64):
        self.B, self.k, self.n, self.V, self.end, self.raw, self.ld, self.ld_hist = B, k, n, V, end, raw, ld or V, ld_hist
        dev = "cuda"
        self.pred = torch.full((B, k), -7, dtype=torch.int64, device=dev)
        self.lp = torch.full((B, k), 7.0, dtype=torch.float32, device=dev)
        self.bp = torch.full((B, k), -7, dtype=torch.int64, device=dev)
        self.hist = torch.full((B, k, ld_hist), -7, dtype=torch.int32, device=dev)
        self.len = torch.full((B, k), -7, dtype=torch.int32, device=dev)
        self.score = torch.full((B, k), 7.0, dtype=torch.float32, device=dev)
        m = max(k, n)
        self.sval = torch.empty(B * k * m, dtype=torch.float32, device=dev)
        self.sidx = torch.empty(B * k * m, dtype=torch.int64, device=dev)
        self.ctl, self.max_steps = None, 0   # early stop: off unless a test sets them

    def untouched(self):
        return bool((self.pred == -7).all() and (self.lp == 7.0).all() and (self.bp == -7).all() and (self.hist == -7).all()
                    and (self.len == -7).all() and (self.score == 7.0).all())

    def desc(self, scores):
        d = L.BeamDesc()
        d.scores, d.ld, d.raw_logits = L.ptr(scores), self.ld, 1 if self.raw else 0
        d.dims = L.FsmDims(0, 1, self.V, 0, 1)
        d.B, d.beam, d.per_node, d.end_index = self.B, self.k, self.n, self.end
        d.pred, d.lp_out, d.backptr = L.ptr(self.pred), L.ptr(self.lp), L.ptr(self.bp)
        d.scratch_val, d.scratch_idx = L.ptr(self.sval), L.ptr(self.sidx)
        d.ctl, d.max_steps = L.ptr(self.ctl), self.max_steps
        return d

    def state(self, hist=None, lens=None):
        s = L.RulesState()
        s.hist, s.len = L.ptr(hist), L.ptr(lens)
        s.hist_out, s.len_out, s.score_out, s.ld_hist = L.ptr(self.hist), L.ptr(self.len), L.ptr(self.score), self.ld_hist
        return s

    def outputs(self, t):
        return (self.pred.cpu().numpy(), self.lp.cpu().numpy(), self.bp.cpu().numpy(), self.len.cpu().numpy(),
                self.score.cpu().numpy(), self.hist[:, :, :t + 1].cpu().numpy())

    def first(self, rows, rules):
        rows = torch.as_tensor(rows).cuda().contiguous()
        L.load().ssc_beam_first_rules(self.desc(rows), desc_of(rules), self.state(), L.stream_ptr())
        torch.cuda.synchronize()
        return self.outputs(0)

    def step(self, rows, t, last_pred, last_lp, hist, lens, rules):
        rows = torch.as_tensor(rows).cuda().contiguous()
        last = torch.as_tensor(np.asarray(last_pred, dtype=np.int64)).cuda().contiguous()
        phi = torch.as_tensor(np.asarray(last_lp, dtype=np.float32)).cuda().contiguous()
        h = torch.zeros(self.B, self.k, self.ld_hist, dtype=torch.int32, device="cuda")
        h[:, :, :t] = torch.as_tensor(np.asarray(hist, dtype=np.int32)[:, :, :t]).cuda()
        ln = torch.as_tensor(np.asarray(lens, dtype=np.int32)).cuda().contiguous()
        d = self.desc(rows)
        d.last_pred, d.last_lp, d.step_index = L.ptr(last), L.ptr(phi), t
        L.load().ssc_beam_step_rules(d, desc_of(rules), self.state(h, ln), L.stream_ptr())
        torch.cuda.synchronize()
        return self.outputs(t)


def rows_of(rng, rows, V, ties):
    """test_dbs_gpu.make_rows at half its scale (exact ties and the grid survive a factor of 1/2): the largest of 40 003 logits
    then lies near 5, so that +10 on a banned token makes it the row's arg-max whatever it was before."""
    return (make_rows(rng, rows, V, ties) * F(0.5)).astype(F)


def fed_state(rng, B, k, t, end=R.END):
    """Histories of t tokens drawn from 6 distinct words, a quarter of the beams ended (END from some earlier position on, the
    length saying where) -> histories (B, k, t) int32, last tokens (B, k) int64, lengths (B, k) int32."""
    hist = rng.choice(WORDS, size=(B, k, t)).astype(np.int32)
    lens = np.full((B, k), t, dtype=np.int32)
    ended = rng.random((B, k)) < 0.25
    for b, j in zip(*np.nonzero(ended)):
        lens[b, j] = rng.integers(1, t + 1)
        hist[b, j, lens[b, j] - 1:] = end
    return hist, hist[:, :, t - 1].astype(np.int64), lens


def promote_banned(rng, x, hist, last, t, k, rules, stats, end=R.END):
    """For every live row whose rules ban something, with probability 1/2: +10 on the logit of one banned token - the ban then
    decides the row.  stats: [rows with a ban, of those the rows whose unruled arg-max is banned]."""
    V = x.shape[1]
    for r in range(x.shape[0]):
        b, j = divmod(r, k)
        if last[b, j] == end:
            continue
        ban = R.banned(V, hist[b, j], t, rules, end)
        if not ban.any():
            continue
        if rng.random() < 0.5:
            x[r, rng.choice(np.nonzero(ban)[0])] += F(10)
        stats[0] += 1
        stats[1] += bool(ban[np.argmax(x[r])])


def step_cases(V, shape):
    """The settings of one (V, shape) case: every later step t crossed with every n; minimum lengths on both sides of t, suppress
    lists of 0, 1 and 8 ids, the three penalty tables, given log-probs and raw logits, plain rows and rows with exact ties."""
    rng = np.random.default_rng(V * 7 + sum(shape))
    i = 0
    for t in (1, 2, 5, 19, 63):
        for n in (0, 1, 2, 3, 4):
            m = (0, t, t + 1)[i % 3]
            ns = (0, 1, 8)[(i // 3 + i) % 3]
            sup = tuple(int(v) for v in rng.choice(np.r_[0, 2:12], size=ns, replace=False))   # words of the histories among them
            alpha = (0.0, 0.7, 1.0)[(i // 5 + i // 2) % 3]
            yield dict(t=t, n=n, m=m, sup=sup, alpha=alpha, raw=bool((i // 2 + i // 7) % 2), ties=bool((i + i // 4) % 2))
            i += 1


def test_the_step_cases_cover_every_setting():
    cs = list(step_cases(90, (3, 5, 2)))
    assert {c["t"] for c in cs} == {1, 2, 5, 19, 63} and {c["n"] for c in cs} == {0, 1, 2, 3, 4}
    assert {len(c["sup"]) for c in cs} == {0, 1, 8} and {c["alpha"] for c in cs} == {0.0, 0.7, 1.0}
    assert {c["raw"] for c in cs} == {False, True} and {c["ties"] for c in cs} == {False, True}
    assert {np.sign(c["m"] - c["t"]) for c in cs if c["m"]} == {0, 1} and any(c["m"] == 0 for c in cs)
    for v in ({(c["n"], c["raw"]) for c in cs}, {(c["n"], c["ties"]) for c in cs}):
        assert len(v) == 10   # every n on given log-probs and on logits, on plain rows and on tied rows


def check_steps(V, shape, cases):
    B, k, per = shape
    rng = np.random.default_rng(V * 100 + B * 7 + k * 3 + per)
    stats = [0, 0]
    phi = None
    for c in cases:
        rules = R.Rules(c["n"], c["m"], c["sup"], R.penalty_table(c["alpha"]))
        st = Steps(B, k, per, V, c["raw"])
        what = (V, shape, c)
        if phi is None or phi.shape != (B, k) or c["t"] == 1:
            # step 0 under the same rules; its sums start the chain
            x0 = rows_of(rng, B, V, c["ties"])
            given0 = x0 if c["raw"] else (x0 - F(9.0))   # (raw_logits 0: scores are taken as they are)
            lp0 = device_log_softmax(x0) if c["raw"] else given0
            tok, phi, _, lens, score, hist = st.first(given0, rules)
            rtok, rphi, rlens, rscore, rhist, _ = R.first_step(lp0, k, rules)
            assert same_values(tok, rtok) and same_values(phi, rphi) and same_values(score, rscore), what
            assert same_values(lens, rlens) and same_values(hist, rhist), what
        t = c["t"]
        hist_in, last, lens_in = fed_state(rng, B, k, t)
        x = rows_of(rng, B * k, V, c["ties"])
        promote_banned(rng, x, hist_in, last, t, k, rules, stats)
        given = x if c["raw"] else (x - F(9.0))
        lpr = device_log_softmax(x) if c["raw"] else given
        tok, lp, bp, lens, score, hist = st.step(given, t, last, phi, hist_in, lens_in, rules)
        rtok, rlp, rbp, rlens, rscore, rhist, _ = R.next_step(lpr, last, phi, hist_in, lens_in, t, B, k, per, rules)
        assert same_values(tok, rtok), what
        assert same_values(bp, rbp), what
        assert same_values(lp, rlp), what
        assert same_values(lens, rlens), what
        assert same_values(score, rscore), what
        assert same_values(hist, rhist), what
        phi = lp   # the next step runs on the device's own sums
    return stats


@pytest.mark.parametrize("V", [90, 1000, 10000])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 2), (2, 32, 32), (70, 4, 3)])
def test_steps_bit_exact_against_the_restatement(V, shape):
    """Step 0 and later steps at t in {1, 2, 5, 19, 63}, chained on the device's own sums, with fed histories over 6 words and a
    quarter of the beams ended; n in 0..4 at every t, minimum lengths on both sides of t, 0 / 1 / 8 suppressed ids, the penalty
    tables of alpha 0 / 0.7 / 1, given log-probs (raw_logits 0) and logits (raw_logits 1: the restatement is fed ssc_log_softmax
    of the same logits), plain rows and rows with exact ties.  Tokens, back-pointers, sums, lengths, scores and histories are
    equal bit for bit.  Half of the rows whose rules ban something get +10 on a banned token; the test asserts that at least a
    quarter of them have their unruled arg-max banned, without which its inputs would prove nothing."""
    stats = check_steps(V, shape, step_cases(V, shape))
    print(f"V {V} shape {shape}: {stats[1]} of {stats[0]} rows with a ban have their unruled arg-max banned")
    assert stats[0] > 0 and stats[1] >= 0.25 * stats[0]


def test_large_vocabulary_takes_the_global_memory_form():
    """V = 40 003 (beyond the register form): the same bit-exact agreement, at every n and both raw settings."""
    V, shape = 40003, (2, 6, 2)
    cases = [dict(t=t, n=n, m=m, sup=sup, alpha=alpha, raw=raw, ties=ties)
             for t, n, m, sup, alpha, raw, ties in ((1, 1, 2, (0,), 1.0, True, True), (2, 2, 0, (), 0.7, True, False),
                                                    (5, 3, 5, (0, 2, 3, 4, 5, 6, 7, 9), 1.0, False, True),
                                                    (19, 4, 20, (3,), 0.0, True, False), (63, 0, 64, (), 0.7, True, True),
                                                    (5, 1, 0, (), 0.0, False, False))]
    stats = check_steps(V, shape, cases)
    assert stats[0] > 0 and stats[1] >= 0.25 * stats[0]


# ---- rules off ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [90, 10000])
def test_rules_off_is_the_beam_search_bit_for_bit(V):
    """No rule and every penalty 1.0f: ssc_beam_first_fsm / ssc_beam_step_fsm with the trivial machine on the same logits."""
    rng = np.random.default_rng(V)
    B, k, n = 4, 5, 2
    st = Steps(B, k, n, V, True)
    lib = L.load()
    x0 = torch.from_numpy(make_rows(rng, B, V, True)).cuda()
    tok, lp, _, lens, score, hist = st.first(x0, R.Rules())
    bpred = torch.empty(B, k, dtype=torch.int64, device="cuda")
    blp = torch.empty(B, k, dtype=torch.float32, device="cuda")
    bbp = torch.empty(B, k, dtype=torch.int64, device="cuda")
    sval = torch.empty(B * k * k, dtype=torch.float32, device="cuda")
    sidx = torch.empty(B * k * k, dtype=torch.int64, device="cuda")
    d = st.desc(x0)
    d.pred, d.lp_out, d.backptr = L.ptr(bpred), L.ptr(blp), L.ptr(bbp)
    d.scratch_val, d.scratch_idx = L.ptr(sval), L.ptr(sidx)
    lib.ssc_beam_first_fsm(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(tok, bpred.cpu().numpy()) and same_bits(lp, blp.cpu().numpy()) and same_bits(score, lp)
    assert (lens == 1).all() and np.array_equal(hist[:, :, 0], tok)
    last = tok.copy()
    last[1, 3] = last[2, 0] = R.END
    hist_in = last[:, :, None].astype(np.int32)
    x = torch.from_numpy(make_rows(rng, B * k, V, False)).cuda()
    tok1, lp1, bp1, lens1, score1, hist1 = st.step(x, 1, last, lp, hist_in, lens, R.Rules())
    lastd, phid = torch.from_numpy(last).cuda(), torch.from_numpy(lp).cuda()
    d = st.desc(x)
    d.pred, d.lp_out, d.backptr = L.ptr(bpred), L.ptr(blp), L.ptr(bbp)
    d.scratch_val, d.scratch_idx = L.ptr(sval), L.ptr(sidx)
    d.last_pred, d.last_lp, d.step_index = L.ptr(lastd), L.ptr(phid), 1
    lib.ssc_beam_step_fsm(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(tok1, bpred.cpu().numpy()) and same_bits(bp1, bbp.cpu().numpy()) and same_bits(lp1, blp.cpu().numpy())
    assert same_bits(score1, lp1)


def test_one_call_with_rules_off_is_the_one_call_beam_search():
    """ssc_decode_rules_beam with every rule off against ssc_decode_search at a call below 512 rows (logits, no records):
    predictions and log-probs bit-equal, scores equal to the log-probs, lengths = first END + 1."""
    cfg, _, _, dec = model(False, boundary_bias=1.0)
    nimg, ns, R_, k, n = 3, 4, 7, 5, 2
    steps = cfg.max_caption_length
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=5)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    pred, lps, scores, lens = dec.rules_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, sampling.DecodeRules())
    want, want_lp = dec.search(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps)
    assert torch.equal(pred, want.view(B, k, -1))
    assert same_bits(lps.cpu().numpy(), want_lp.view(B, k).cpu().numpy()) and same_bits(scores.cpu().numpy(), lps.cpu().numpy())
    check_lengths(pred.cpu().numpy(), lens.cpu().numpy(), cfg.boundary_index, steps)


def check_lengths(pred, lens, end, max_steps):
    """len = the index of the first END plus one, or max_steps (a search cut by early stop returns fewer columns: every beam had
    ended)."""
    for cap, n in zip(pred.reshape(-1, pred.shape[-1]).tolist(), lens.reshape(-1).tolist()):
        assert n == (cap.index(end) + 1 if end in cap else max_steps), (cap, n)


# ---- robustness --------------------------------------------------------------------------------------------------------------------

ALL_ON = R.Rules(3, 3, (0, 4), R.penalty_table(1.0))


def test_two_calls_are_bit_identical():
    V, k, n, B, t = 3000, 12, 2, 5, 6
    rng = np.random.default_rng(2)
    st = Steps(B, k, n, V, True)
    x = rows_of(rng, B * k, V, True)
    hist, last, lens = fed_state(rng, B, k, t)
    phi = rng.uniform(-9, -1, (B, k)).astype(F)
    a = [v.copy() for v in st.step(x, t, last, phi, hist, lens, ALL_ON)]
    b = st.step(x, t, last, phi, hist, lens, ALL_ON)
    assert all(same_bits(u, v) for u, v in zip(a, b))


def test_a_step_after_the_stop_moves_nothing():
    """ctl[0] = 3 and a step at t = 5 (queued by a host that polled late): END from the same beam for every slot, the history
    with END appended, and sum, length and score as they were - the score recomputed from them has the bits it had."""
    V, k, n, B, t, steps = 90, 4, 2, 3, 5, 9
    rng = np.random.default_rng(11)
    st = Steps(B, k, n, V, True)
    st.ctl = torch.zeros(2 + 2 * steps, dtype=torch.int32, device="cuda")
    st.ctl[0] = 3
    st.max_steps = steps
    hist, last, lens = fed_state(rng, B, k, t)
    phi = rng.uniform(-9, -1, (B, k)).astype(F)
    phi[0, 1] = -np.inf   # (an empty slot of an earlier step)
    tok, lp, bp, lens_out, score, hist_out = st.step(rows_of(rng, B * k, V, False), t, last, phi, hist, lens, ALL_ON)
    assert (tok == R.END).all() and (bp == np.arange(k)[None]).all()
    assert same_bits(lp, phi) and same_bits(lens_out, lens)
    assert same_bits(score, (phi / ALL_ON.table[lens - 1]).astype(F))
    assert np.array_equal(hist_out[:, :, :t], hist) and (hist_out[:, :, t] == R.END).all()
    assert int(st.ctl[0]) == 3


@pytest.mark.parametrize("V,raw", [(90, True), (1000, False), (40003, True)])
def test_the_scores_are_never_written(V, raw):
    """Bans do not touch the logits: rows with a leading dimension beyond V and guard values in the surplus columns are the same
    bytes after a first and a later step as before."""
    k, n, B, t, ld = 4, 3, 3, 5, V + 13
    rng = np.random.default_rng(V)
    st = Steps(B, k, n, V, raw, ld=ld)
    buf = np.full((B * k, ld), 1e30, dtype=F)
    buf[:, :V] = rows_of(rng, B * k, V, False)
    hist, last, lens = fed_state(rng, B, k, t)
    dev = torch.from_numpy(buf).cuda()
    st.first(dev, ALL_ON)
    phi = rng.uniform(-9, -1, (B, k)).astype(F)
    out = st.step(dev, t, last, phi, hist, lens, ALL_ON)
    assert same_bits(dev.cpu().numpy(), buf)
    rows = np.ascontiguousarray(buf[:, :V])
    ref = R.next_step(device_log_softmax(rows) if raw else rows, last, phi, hist, lens, t, B, k, n, ALL_ON)
    assert all(same_values(u, v) for u, v in zip(out, ref[:6]))   # (the surplus columns played no part)


def test_bad_descriptors_launch_nothing():
    V, B = 90, 2
    x = torch.randn(B * 33, V, device="cuda")
    lib = L.load()

    def refused(k=6, n=2, t=1, rules=None, machine=False, ld_hist=64, calls=("first", "step")):
        st = Steps(B, k, n, V, True, ld_hist=ld_hist)
        d = st.desc(x)
        if machine:
            d.dims = L.FsmDims(B, 2, V, 0, 1)
        r = desc_of(R.Rules(3, 2, (0,), R.penalty_table(1.0))) if rules is None else rules
        for call in calls:
            s = st.state()
            if call == "step":
                last = torch.full((B, k), 3, dtype=torch.int64, device="cuda")
                phi = torch.zeros(B, k, device="cuda")
                h = torch.zeros(B, k, 64, dtype=torch.int32, device="cuda")
                ln = torch.ones(B, k, dtype=torch.int32, device="cuda")
                d.last_pred, d.last_lp, d.step_index = L.ptr(last), L.ptr(phi), t
                s = st.state(h, ln)
            with pytest.raises(L.SscError, match="SSC_EINVAL"):
                getattr(lib, f"ssc_beam_{call}_rules")(C.byref(d), C.byref(r), C.byref(s), L.stream_ptr())
        torch.cuda.synchronize()
        assert st.untouched()

    def rules_with(**kw):
        r = desc_of(R.Rules(3, 2, (0,), R.penalty_table(1.0)))
        for key, v in kw.items():
            if key == "suppress0":
                r.suppress[0] = v
            elif key.startswith("penalty"):
                r.length_penalty[int(key[7:])] = v
            else:
                setattr(r, key, v)
        return r

    refused(machine=True)
    refused(k=33)
    refused(n=33, calls=("step",))   # (step 0 takes no per_node)
    refused(t=0, calls=("step",))
    refused(t=64, calls=("step",))
    refused(t=7, ld_hist=7, calls=("step",))
    refused(rules=rules_with(no_repeat_ngram=65))
    refused(rules=rules_with(no_repeat_ngram=-1))
    refused(rules=rules_with(min_length=-1))
    refused(rules=rules_with(n_suppress=9))
    refused(rules=rules_with(suppress0=V))
    refused(rules=rules_with(suppress0=R.END))
    refused(rules=rules_with(penalty63=0.0))
    refused(rules=rules_with(penalty5=float("nan")))
    refused(rules=rules_with(penalty0=float("inf")))
    # the one-call search refuses the same
    cfg, _, _, dec = model(False)
    feats, senti, eps0, eps = inputs(cfg, 2, 2, 5, seed=1)
    ctx = dec.prepare(feats.cuda())
    bad = sampling.DecodeRules(3, 2, 1.0, (0,))
    bad.no_repeat_ngram = 65
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        dec.rules_beam(ctx, None, 2, 6, 1, 4, cfg.boundary_index, eps0, eps.repeat_interleave(6, 1)[:3], bad)
    with pytest.raises(ValueError, match="boundary"):
        dec.rules_beam(ctx, None, 2, 6, 1, 4, cfg.boundary_index, eps0, eps.repeat_interleave(6, 1)[:3],
                       sampling.DecodeRules(suppress=(cfg.boundary_index,)))
    with pytest.raises(ValueError, match="per_node"):
        dec.rules_beam(ctx, None, 2, 33, 1, 4, cfg.boundary_index, eps0, eps.repeat_interleave(33, 1)[:3], sampling.DecodeRules(3))


# ---- the whole search ----------------------------------------------------------------------------------------------------------

def stepwise_search(dec, ctx, sent_b, B, k, n, rules, steps, end, eps0, eps, early_stop=False, skip_dead=False):
    """The search driven from Python: DecodeEngine.step (raw logits) + ssc_beam_first_rules / ssc_beam_step_rules, the states
    re-ordered by back-pointer as cbs_search does.  -> (predictions (B, k, steps'), sums, scores, lengths (B, k), the final history
    generation (B, k, steps'), per-step record, ctl[0] or None)."""
    lib = L.load()
    dev = "cuda"
    V = dec.dims.V
    r = desc_of(rules)
    preds = torch.empty(steps, B, k, dtype=torch.int64, device=dev)
    backs = torch.empty(max(steps - 1, 1), B, k, dtype=torch.int64, device=dev)
    m = max(k, n)
    sval = torch.empty(B * k * m, dtype=torch.float32, device=dev)
    sidx = torch.empty(B * k * m, dtype=torch.int64, device=dev)
    hist = [torch.zeros(B, k, steps, dtype=torch.int32, device=dev) for _ in range(2)]
    lens = [torch.zeros(B, k, dtype=torch.int32, device=dev) for _ in range(2)]
    score = [torch.zeros(B, k, dtype=torch.float32, device=dev) for _ in range(2)]
    ctl = None
    if early_stop:
        ctl = torch.zeros(2 + 2 * steps, dtype=torch.int32, device=dev)
        ctl[0] = steps
    last_lp = torch.empty(B, k, dtype=torch.float32, device=dev)
    logits, states, _ = dec.step(ctx, torch.full((B,), end, dtype=torch.int64, device=dev), None, sent_b, eps0.cuda(), raw_logits=True)
    d = L.BeamDesc()
    d.raw_logits = 1
    d.dims = L.FsmDims(0, 1, V, 0, 1)
    d.B, d.beam, d.per_node, d.end_index = B, k, n, end
    d.ctl, d.max_steps = L.ptr(ctl), steps
    d.scratch_val, d.scratch_idx = L.ptr(sval), L.ptr(sidx)
    d.scores, d.ld = L.ptr(logits), logits.stride(0)
    d.pred, d.lp_out = L.ptr(preds[0]), L.ptr(last_lp)
    s = L.RulesState()
    s.ld_hist = steps
    s.hist_out, s.len_out, s.score_out = L.ptr(hist[0]), L.ptr(lens[0]), L.ptr(score[0])
    lib.ssc_beam_first_rules(C.byref(d), C.byref(r), C.byref(s), L.stream_ptr())
    a = 0
    rec = {"lp": [last_lp], "len": [lens[0].clone()], "score": [score[0].clone()]}
    states = {key: v.repeat_interleave(k, 0).contiguous() for key, v in states.items() if not key.startswith("_")}
    states["_parent"] = torch.zeros(B, k, dtype=torch.int64, device=dev)
    sent_rows = sent_b.repeat_interleave(k) if sent_b is not None else None
    ran = 1
    for t in range(1, steps):
        if ctl is not None and int(ctl[0]) <= t:
            break
        last = preds[t - 1].reshape(B * k)
        if skip_dead:
            states["_skip"] = (last_lp, end)
        logits, states, _ = dec.step(ctx, last, states, sent_rows, eps[t - 1].cuda(), raw_logits=True)
        new_lp = torch.empty_like(last_lp)
        d.scores, d.ld = L.ptr(logits), logits.stride(0)
        d.last_pred, d.last_lp = L.ptr(last), L.ptr(last_lp)
        d.pred, d.lp_out, d.backptr = L.ptr(preds[t]), L.ptr(new_lp), L.ptr(backs[t - 1])
        d.step_index = t
        s.hist, s.len = L.ptr(hist[a]), L.ptr(lens[a])
        s.hist_out, s.len_out, s.score_out = L.ptr(hist[1 - a]), L.ptr(lens[1 - a]), L.ptr(score[1 - a])
        lib.ssc_beam_step_rules(C.byref(d), C.byref(r), C.byref(s), L.stream_ptr())
        a = 1 - a
        last_lp = new_lp
        rec["lp"].append(new_lp)
        rec["len"].append(lens[a].clone())
        rec["score"].append(score[a].clone())
        idx = (torch.arange(B, device=dev).view(B, 1) * k + backs[t - 1]).reshape(-1)
        states = {key: v[idx].contiguous() for key, v in states.items() if not key.startswith("_")}
        states["_parent"] = backs[t - 1]
        ran = t + 1
    out = torch.empty(B, k, ran, dtype=torch.int64, device=dev)
    lib.ssc_beam_backtrace(L.ptr(preds), L.ptr(backs), ran, B, k, L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    nsteps = int(ctl[0]) if ctl is not None else ran
    record = {"tok": [preds[t].cpu().numpy() for t in range(ran)], "lp": [x.cpu().numpy() for x in rec["lp"]],
              "bp": [None] + [backs[t].cpu().numpy() for t in range(ran - 1)], "len": [x.cpu().numpy() for x in rec["len"]],
              "score": [x.cpu().numpy() for x in rec["score"]]}
    return (out[:, :, :nsteps].cpu(), last_lp.cpu(), score[a].cpu(), lens[a].cpu(), hist[a][:, :, :nsteps].cpu(), record,
            nsteps if ctl is not None else None)


SEARCH_RULES = sampling.DecodeRules(no_repeat_ngram=2, min_length=3, length_alpha=1.0, suppress=(0,))


def ref_rules(rules):
    return R.Rules(rules.no_repeat_ngram, rules.min_length, rules.suppress, rules.table())


@pytest.mark.parametrize("early_stop,skip_dead", [(False, False), (True, True), (True, False), (False, True)])
def test_one_call_search_equals_the_stepwise_search(early_stop, skip_dead):
    """ssc_decode_rules_beam with every rule on against the same search driven step by step from Python, bit for bit; the final
    history generation is the back-traced prediction."""
    cfg, _, _, dec = model(False, boundary_bias=2.0)
    nimg, ns, R_, k, n = 3, 4, 7, 5, 2
    steps = cfg.max_caption_length
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=5)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    pred, lps, scores, lens = dec.rules_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, SEARCH_RULES,
                                             early_stop=early_stop, skip_dead=skip_dead)
    want, want_lp, want_score, want_len, hist, _, _ = stepwise_search(dec, ctx, sent_b, B, k, n, ref_rules(SEARCH_RULES), steps,
                                                                      cfg.boundary_index, eps0, eps, early_stop=early_stop,
                                                                      skip_dead=skip_dead)
    assert pred.shape == want.shape
    assert torch.equal(pred.cpu(), want)
    assert same_bits(lps.cpu().numpy(), want_lp.numpy()) and same_bits(scores.cpu().numpy(), want_score.numpy())
    assert torch.equal(lens.cpu(), want_len)
    assert torch.equal(hist.long(), want)
    ended = (pred == cfg.boundary_index).cumsum(-1) > 0
    assert (pred[ended] == cfg.boundary_index).all()


def test_search_stops_when_every_beam_has_ended():
    """An overwhelming end token once the minimum length allows it: ctl[0] < max_steps, the call returns ctl[0] columns, and
    without early stop the surplus columns hold end_index while sums, scores and lengths stay what they were."""
    cfg, params, _, dec = model(False, boundary_bias=6.0)
    nimg, ns, R_, k, n = 2, 3, 5, 4, 2
    steps = cfg.max_caption_length
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=8)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    a, alp, asc, alen = dec.rules_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, SEARCH_RULES)
    want, want_lp, want_score, want_len, _, _, nsteps = stepwise_search(dec, ctx, sent_b, B, k, n, ref_rules(SEARCH_RULES), steps,
                                                                        cfg.boundary_index, eps0, eps, early_stop=True)
    assert SEARCH_RULES.min_length < nsteps < steps and a.size(-1) == nsteps
    assert torch.equal(a.cpu(), want) and same_bits(alp.cpu().numpy(), want_lp.numpy())
    assert same_bits(asc.cpu().numpy(), want_score.numpy()) and torch.equal(alen.cpu(), want_len)
    full, flp, fsc, flen = dec.rules_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, SEARCH_RULES, early_stop=False)
    assert full.size(-1) == steps and torch.equal(full[..., :nsteps], a) and (full[..., nsteps:] == cfg.boundary_index).all()
    assert torch.equal(flp, alp) and torch.equal(fsc, asc) and torch.equal(flen, alen)


# `sharp` scales the output layer (test_dbs_gpu.sharp_model): at 12 the toy model's plain beam search repeats words
PROPERTY_CASE = dict(sharp=12.0, seed=5)


@pytest.mark.parametrize("n", [1, 2])
def test_properties_of_the_whole_search(n):
    """A model whose PLAIN beam search repeats an n-gram in at least one caption (asserted on DecodeEngine.search's output) decoded
    under the rules: no caption holds a repeated n-gram before its END, none ends before min_length, no suppressed id appears,
    scores == log_probs / table[len - 1] bit for bit, scores descend along the beam axis, len = first END + 1 or max_steps.  With
    sharp 12 and seed 5 the oracle's plain search, on the CPU, repeats a word in 60 of 60 captions and a bigram in 53 of 60."""
    c = PROPERTY_CASE
    cfg, _, dec, _eng = sharp_model(False, c["sharp"])
    nimg, ns, R_, k, per = 3, 4, 7, 5, 2
    steps = cfg.max_caption_length
    end = cfg.boundary_index
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=c["seed"])
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    plain, _ = dec.search(ctx, sent_b, ns, k, per, steps, end, eps0, eps, early_stop=False)
    plain = plain.view(B * k, -1).cpu().numpy()
    assert any(R.repeated_ngram(cap, n, end) for cap in plain), "the plain search repeats nothing: the test proves nothing"
    for alpha in (0.0, 0.7, 1.0):
        word = next(int(w) for w in plain[:, 0] if w not in (0, end))   # a word the plain search starts a caption with
        rules = sampling.DecodeRules(no_repeat_ngram=n, min_length=4, length_alpha=alpha, suppress=(0, word))
        pred, lps, scores, lens = dec.rules_beam(ctx, sent_b, ns, k, per, steps, end, eps0, eps, rules, early_stop=False)
        pred, lps, scores, lens = pred.cpu().numpy(), lps.cpu().numpy(), scores.cpu().numpy(), lens.cpu().numpy()
        table = rules.table()
        fin = np.isfinite(lps)
        assert fin.any()
        for cap, lp in zip(pred.reshape(B * k, -1), lps.reshape(-1)):
            if not np.isfinite(lp):
                continue   # (an empty slot: END at -inf)
            words = cap.tolist()
            words = words[:words.index(end)] if end in words else words
            assert not R.repeated_ngram(cap, n, end), cap
            assert len(words) >= 4, cap
            assert not set(words) & set(rules.suppress), cap
        check_lengths(pred, lens, end, steps)
        assert same_bits(scores, (lps / table[lens - 1]).astype(F))
        assert (np.diff(scores, axis=1) <= 0).all()


# ---- against the CPU oracle ------------------------------------------------------------------------------------------------------

def oracle_search(cfg, params, feats, senti, eps0, eps, nimg, ns, k, n, rules, steps):
    """tests/rulesref.search driven by the oracle's eval decode step -> its record (per-step tokens, sums, back-pointers, lengths,
    scores, histories and selection margins)."""
    B = nimg * ns
    R_ = feats.size(1)
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B, 1)
    end = cfg.boundary_index
    t_of = {"t": 0}

    def step(tokens, states):
        rows = tokens.shape[0]
        per = rows // nimg
        fr = feats.unsqueeze(1).expand(nimg, per, R_, feats.size(2)).reshape(rows, R_, -1)
        se = sent_b.repeat_interleave(rows // B, 0)
        pm, pv = oracle.prior_from_sentiment(cfg, se, rows, fr)
        st = zero_states(rows, cfg.hidden_size, fr) if states is None else {k_: torch.from_numpy(np.ascontiguousarray(v)) for k_, v in states.items()}
        t = t_of["t"]
        e = eps0 if t == 0 else eps[t - 1]
        t_of["t"] = t + 1
        with torch.no_grad():
            lp, st, _, _, _ = oracle.decode_step(params, cfg, fr, torch.from_numpy(tokens), st, False, se, pm, pv, e)
        return lp.numpy().astype(F), {k_: v.numpy() for k_, v in st.items()}

    return R.search(step, None, B, k, n, rules, steps, end=end, early_stop=False)[2]


def compare_with_oracle(rec, dev, B):
    """-> (entries compared to the end, entries in all, largest difference of a sum).  An entry is followed up to the first step
    at which its selection has a sub-margin gap, and then counts as cut short."""
    alive = np.ones(B, dtype=bool)
    worst = 0.0
    for t in range(len(rec["tok"])):
        alive &= rec["margin"][t] > MARGIN
        if not alive.any():
            break
        assert np.array_equal(dev["tok"][t][alive], rec["tok"][t][alive]), t
        assert np.array_equal(dev["len"][t][alive], rec["len"][t][alive]), t
        if t > 0:
            assert np.array_equal(dev["bp"][t][alive], rec["bp"][t][alive]), t
        fin = np.isfinite(rec["lp"][t][alive])
        diff = np.abs(dev["lp"][t][alive][fin].astype(np.float64) - rec["lp"][t][alive][fin])
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
    return int(alive.sum()), B, worst


# beam, per_node and seed of the oracle comparison, picked on the CPU (the oracle side alone) for the cap on entries cut short
ORACLE_SEEDS = {False: dict(seed=5, k=3, per=1), True: dict(seed=10, k=3, per=1)}


@pytest.mark.parametrize("gemm_mode", [0, 2])
@pytest.mark.parametrize("full", [False, True])
def test_against_the_cpu_oracle(full, gemm_mode):
    """tests/rulesref.py driven by the oracle's eval decode step, against the device search driven step by step, k = 3, per_node
    1, n = 2, min_length = 3, alpha = 1, suppress [0]: toy width (3 images x 4 samples, 9 steps) and full width (H 1200,
    V 10 000, R 36, 2 images x 3 samples, 6 steps), in the engine's default GEMM mode and in gemm_mode 2 (exact fp32).  Sums within
    1e-4, the project's decode tolerance (with alpha >= 0 every divisor is >= 1: the key's error is no larger); tokens,
    back-pointers and lengths identical at every (entry, step) whose oracle selection margin exceeds 2e-4; an entry is followed
    up to its first sub-margin step.  At most 10 % of the entries may be cut short that way.  The oracle side alone, on the CPU,
    cuts short 0 of 12 entries at toy width (seed 5, smallest margin 2.8e-4) and 0 of 6 at full width (seed 10, smallest margin
    3.8e-4); wider beams put more keys next to each other - at k = 6, per_node 2 the same seeds cut 9 of 12 and 6 of 6."""
    c = dict(ORACLE_CASES[full], **ORACLE_SEEDS[full])
    cfg, params, dec, _eng = sharp_model(full, c["sharp"])
    if gemm_mode:
        dec._cfg.gemm_mode = gemm_mode   # (what an engine-wide ModelDims.gemm_mode sets)
    nimg, ns, k, n, steps = c["nimg"], c["ns"], c["k"], c["per"], c["steps"]
    rules = ref_rules(SEARCH_RULES)
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, c["R_"], k, seed=c["seed"], steps=steps)
    B = nimg * ns
    rec = oracle_search(cfg, params, feats, senti, eps0, eps, nimg, ns, k, n, rules, steps)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    dev = stepwise_search(dec, ctx, sent_b, B, k, n, rules, steps, cfg.boundary_index, eps0, eps)[5]
    whole, entries, worst = compare_with_oracle(rec, dev, B)
    print(f"oracle parity full={full} gemm_mode={gemm_mode}: {entries - whole} of {entries} entries cut short, max |dlp| {worst:.3g}")
    assert worst < 1e-4
    assert entries - whole <= 0.1 * entries


# ---- the public interface ------------------------------------------------------------------------------------------------------

def test_diverse_decode_with_rules():
    cfg, _, _, dec = model(False)
    feats = torch.randn(3, 7, cfg.image_feature_size).cuda()
    senti = torch.tensor([1.0, 0.0, -1.0]).cuda()
    rules = sampling.DecodeRules(no_repeat_ngram=2, min_length=3, length_alpha=1.0, suppress=(0,))
    L_ = cfg.max_caption_length
    torch.manual_seed(0)
    best, steps = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index, rules=rules)
    assert best.shape == (3, 4, steps) and best.dtype == torch.int64
    # beam 0 of the engine's own output, on the noise the call drew
    torch.manual_seed(0)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    B = 12
    eps0 = torch.randn(B, cfg.z_space, device="cuda", generator=gen)
    eps = torch.randn(max(L_ - 1, 1), B * 6, cfg.z_space, device="cuda", generator=gen)
    ctx = dec.prepare(feats)
    beams, lps, scores, lens = dec.rules_beam(ctx, senti.view(3, 1).expand(3, 4).reshape(B), 4, 6, 3, L_, cfg.boundary_index, eps0,
                                              eps, rules)
    assert torch.equal(best.view(B, -1), beams[:, 0, :])
    assert lps.shape == scores.shape == lens.shape == (B, 6) and lens.dtype == torch.int32
    # rules with every control off, and no rules: the beam search's captions
    torch.manual_seed(0)
    off, _ = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index, rules=sampling.DecodeRules())
    torch.manual_seed(0)
    beam, _ = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index)
    assert torch.equal(off, beam)
    with pytest.raises(ValueError, match="sampler"):
        diverse_decode(dec, feats, senti, 2, 6, 5, cfg.boundary_index, rules=rules, sampler=sampling.TopKSampler(k=3))
    with pytest.raises(ValueError, match="diverse_beam"):
        diverse_decode(dec, feats, senti, 2, 6, 5, cfg.boundary_index, rules=rules, diverse_beam=sampling.DiverseBeam(3, 0.5))
    with pytest.raises(ValueError, match="constraints"):
        diverse_decode(dec, feats, senti, 2, 6, 5, cfg.boundary_index, rules=rules,
                       fsm=torch.ones(3, 1, 1, cfg.vocab_size, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="boundary"):
        diverse_decode(dec, feats, senti, 2, 6, 5, cfg.boundary_index, rules=sampling.DecodeRules(suppress=(cfg.boundary_index,)))


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", "3", "MODEL.NO_REPEAT_NGRAM", "2", "MODEL.MIN_CAPTION_LENGTH", "3",
                            "MODEL.LENGTH_PENALTY_ALPHA", "1.0", "MODEL.SUPPRESS_UNKNOWN", "True", "MODEL.BEAM_SIZE", "6",
                            "MODEL.IMAGE_FEATURE_SIZE", "64", "MODEL.EMBEDDING_SIZE", "40", "MODEL.HIDDEN_SIZE", "48",
                            "MODEL.ATTENTION_PROJECTION_SIZE", "32", "MODEL.Z_SPACE", "16", "DATA.MAX_CAPTION_LENGTH", "8"])
torch.manual_seed(C.RANDOM_SEED)
m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                sampler=sampling.from_config(C.MODEL)).cuda().eval()
r = m.decode_rules
assert r is not None and (r.no_repeat_ngram, r.min_length, r.length_alpha, r.suppress) == (2, 3, 1.0, (0,))
g = torch.Generator().manual_seed(0)
feats = torch.randn(8, 6, 64, generator=g).cuda()
out = m(feats)["predictions"]
print(json.dumps(out.cpu().tolist()))
"""


def test_module_forward():
    src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"))
    a, b = (json.loads(run_child(["-c", src]).strip().splitlines()[-1]) for _ in range(2))
    assert a == b and len(a) == 8 and all(0 < len(c) <= 8 for c in a)
    for cap in a:
        words = cap[:cap.index(1)] if 1 in cap else cap
        assert len(words) >= 3 and 0 not in words and not R.repeated_ngram(cap, 2, 1), cap
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    rules = sampling.DecodeRules(no_repeat_ngram=3)
    with pytest.raises(ValueError, match="DECODE_SAMPLER"):
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4, decode_rules=rules, sampler=sampling.GumbelSampler())
    with pytest.raises(ValueError, match="DIVERSE_BEAM_SEARCH"):
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4, decode_rules=rules,
                        diverse_beam=sampling.DiverseBeam(3, 0.5))
    with pytest.raises(ValueError, match="boundary"):
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4, decode_rules=sampling.DecodeRules(suppress=(1,)))
    assert UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4,
                           decode_rules=sampling.DecodeRules()).decode_rules is None   # every control off: no rules
    m = UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4, decode_rules=rules).cuda().eval()
    m._use_cbs = True
    with pytest.raises(ValueError, match="USE_CBS"):
        m(torch.randn(2, 3, 16, device="cuda"), fsm=torch.ones(2, 1, 1, 50, dtype=torch.uint8))


def test_inference_script_with_decode_rules(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 12\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
                   "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
                   "  BEAM_SIZE: 6\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
                   "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 2\n")
    out = tmp_path / "pred.json"
    run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4",
               "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--config-override",
               "MODEL.NO_REPEAT_NGRAM", "3", "MODEL.LENGTH_PENALTY_ALPHA", "1.0", "MODEL.SUPPRESS_UNKNOWN", "True"])
    caps = json.load(open(out))
    assert len(caps) == 4 * 2 and all(isinstance(c["caption"], str) for c in caps)
    for c in caps:
        words = c["caption"].split()
        grams = [tuple(words[i:i + 3]) for i in range(len(words) - 2)]
        assert len(grams) == len(set(grams)), c
        assert "@@UNKNOWN@@" not in words, c
