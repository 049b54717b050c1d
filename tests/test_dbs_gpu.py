"""GPU: the diverse beam search (ssc_beam_first_diverse / ssc_beam_step_diverse, ssc_decode_diverse_beam,
DecodeEngine.diverse_beam, diverse_decode / UpDownCaptioner / scripts/inference.py with MODEL.DIVERSE_BEAM_SEARCH) against the
numpy float32 restatement of its definition (tests/dbsref.py: bit-exact), the beam search (one group), a search driven step by
step from Python, and the CPU oracle's decode step."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dbsref as R
import oracle
from oracle.seqcvae_oracle import zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from test_sampling_gpu import ROOT, inputs, model, run_child

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(6, 3, 1), (6, 2, 3), (20, 20, 1), (32, 4, 4), (5, 1, 2)]   # (k, Gr, n)


def list_len(k, Gr, n, V):
    return min(n + k - k // Gr, V)


class Steps:
    """The two stand-alone steps on device buffers: B entries of k beams in Gr groups, n candidates per beam."""

    def __init__(self, B, k, Gr, n, V, lam, raw, end=R.END):
        self.B, self.k, self.Gr, self.n, self.V, self.end, self.raw = B, k, Gr, n, V, end, raw
        self.s = L.DiverseDesc(Gr, lam)
        dev = "cuda"
        self.pred = torch.full((B, k), -7, dtype=torch.int64, device=dev)
        self.lp = torch.full((B, k), 7.0, dtype=torch.float32, device=dev)
        self.bp = torch.full((B, k), -7, dtype=torch.int64, device=dev)
        m = k + n   # (>= every list length: min(n + k - k / Gr, V) at a later step, k at step 0)
        self.sval = torch.empty(B * k * m, dtype=torch.float32, device=dev)
        self.sidx = torch.empty(B * k * m, dtype=torch.int64, device=dev)

    def desc(self, scores):
        d = L.BeamDesc()
        d.scores, d.ld, d.raw_logits = L.ptr(scores), self.V, 1 if self.raw else 0
        d.dims = L.FsmDims(0, 1, self.V, 0, 1)
        d.B, d.beam, d.per_node, d.end_index = self.B, self.k, self.n, self.end
        d.pred, d.lp_out, d.backptr = L.ptr(self.pred), L.ptr(self.lp), L.ptr(self.bp)
        d.scratch_val, d.scratch_idx = L.ptr(self.sval), L.ptr(self.sidx)
        return d

    def first(self, rows):
        rows = torch.as_tensor(rows).cuda().contiguous()
        L.load().ssc_beam_first_diverse(self.desc(rows), self.s, L.stream_ptr())
        torch.cuda.synchronize()
        return self.pred.cpu().numpy(), self.lp.cpu().numpy()

    def step(self, rows, t, last_pred, last_lp):
        rows = torch.as_tensor(rows).cuda().contiguous()
        last = torch.as_tensor(np.asarray(last_pred, dtype=np.int64)).cuda().contiguous()
        phi = torch.as_tensor(np.asarray(last_lp, dtype=np.float32)).cuda().contiguous()
        d = self.desc(rows)
        d.last_pred, d.last_lp, d.step_index = L.ptr(last), L.ptr(phi), t
        L.load().ssc_beam_step_diverse(d, self.s, L.stream_ptr())
        torch.cuda.synchronize()
        return self.pred.cpu().numpy(), self.lp.cpu().numpy(), self.bp.cpu().numpy()


def device_log_softmax(x):
    x = torch.as_tensor(x).cuda().contiguous()
    out = torch.empty_like(x)
    L.load().ssc_log_softmax(L.ptr(x), x.size(1), x.size(0), x.size(1), L.ptr(out), x.size(1), L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def make_rows(rng, rows, V, ties):
    """raw logits; `ties`: quantised to a 1/4 grid, and half of every row duplicated from its other half - exact ties"""
    x = (rng.standard_normal((rows, V)) * 2.5).astype(F)
    if ties:
        x = np.round(x * 4) / F(4)
        h = V // 2
        x[:, h:2 * h] = x[:, :h]
    return x.astype(F)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == F else a,
                                                                        b.view(np.int32) if b.dtype == F else b)


def same_values(a, b):
    """bit-equal, +0 and -0 taken as the same value"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("V", [90, 1000, 10000])
@pytest.mark.parametrize("shape", SHAPES)
def test_steps_bit_exact_against_the_restatement(V, shape):
    """Step 0 and two later steps, chained on the device's own outputs with ended beams mixed in, for strength 0 / 0.5 / 4, on
    given log-probs (raw_logits 0) and on logits (raw_logits 1: the restatement is fed ssc_log_softmax of the same logits); plain
    rows and rows with exact ties.  Tokens, back-pointers and log-probs are equal bit for bit."""
    k, Gr, n = shape
    rng = np.random.default_rng(V * 100 + k * 3 + Gr)
    B = 3
    for lam in (0.0, 0.5, 4.0):
        for raw in (False, True):
            for ties in (False, True):
                what = (V, shape, lam, raw, ties)
                st = Steps(B, k, Gr, n, V, lam, raw)
                x0 = make_rows(rng, B, V, ties)
                given0 = x0 if raw else (x0 - F(9.0))   # (raw_logits 0: scores are taken as they are)
                lp0 = device_log_softmax(x0) if raw else given0
                tok, lp = st.first(given0)
                rtok, rlp, _ = R.first_step(lp0, k, Gr, lam)
                assert same_values(tok, rtok) and same_values(lp, rlp), what
                for t in (1, 2):
                    last, phi = tok.copy(), lp.copy()
                    ended = rng.random((B, k)) < 0.25
                    last[ended] = R.END
                    x = make_rows(rng, B * k, V, ties)
                    given = x if raw else (x - F(9.0))
                    lpr = device_log_softmax(x) if raw else given
                    tok, lp, bp = st.step(given, t, last, phi)
                    rtok, rlp, rbp, _ = R.next_step(lpr, last, phi, B, k, Gr, n, lam)
                    assert same_values(tok, rtok), (what, t)
                    assert same_values(bp, rbp), (what, t)
                    assert same_values(lp, rlp), (what, t)


def test_large_vocabulary_takes_the_global_memory_form():
    """V = 40 003 (beyond the register form): the same bit-exact agreement."""
    V, k, Gr, n, B = 40003, 6, 3, 2, 2
    rng = np.random.default_rng(5)
    st = Steps(B, k, Gr, n, V, 0.5, True)
    x0 = make_rows(rng, B, V, True)
    tok, lp = st.first(x0)
    rtok, rlp, _ = R.first_step(device_log_softmax(x0), k, Gr, 0.5)
    assert same_values(tok, rtok) and same_values(lp, rlp)
    x = make_rows(rng, B * k, V, False)
    last = tok.copy()
    last[0, 2] = R.END
    tok1, lp1, bp1 = st.step(x, 1, last, lp)
    rtok, rlp, rbp, _ = R.next_step(device_log_softmax(x), last, lp, B, k, Gr, n, 0.5)
    assert same_values(tok1, rtok) and same_values(bp1, rbp) and same_values(lp1, rlp)


@pytest.mark.parametrize("V", [90, 10000])
def test_one_group_is_the_beam_search_bit_for_bit(V):
    """Gr = 1, any strength: ssc_beam_first_fsm / ssc_beam_step_fsm with the trivial machine on the same logits."""
    rng = np.random.default_rng(V)
    B, k, n = 4, 5, 2
    st = Steps(B, k, 1, n, V, 3.0, True)
    lib = L.load()
    x0 = torch.from_numpy(make_rows(rng, B, V, True)).cuda()
    tok, lp = st.first(x0)
    bpred = torch.empty(B, k, dtype=torch.int64, device="cuda")
    blp = torch.empty(B, k, dtype=torch.float32, device="cuda")
    bbp = torch.empty(B, k, dtype=torch.int64, device="cuda")
    d = st.desc(x0)
    d.pred, d.lp_out, d.backptr = L.ptr(bpred), L.ptr(blp), L.ptr(bbp)
    sval = torch.empty(B * k * n, dtype=torch.float32, device="cuda")
    sidx = torch.empty(B * k * n, dtype=torch.int64, device="cuda")
    d.scratch_val, d.scratch_idx = L.ptr(sval), L.ptr(sidx)
    lib.ssc_beam_first_fsm(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(tok, bpred.cpu().numpy()) and same_bits(lp, blp.cpu().numpy())
    last = tok.copy()
    last[1, 3] = last[2, 0] = R.END
    x = torch.from_numpy(make_rows(rng, B * k, V, False)).cuda()
    tok1, lp1, bp1 = st.step(x, 1, last, lp)
    lastd, phid = torch.from_numpy(last).cuda(), torch.from_numpy(lp).cuda()
    d = st.desc(x)
    d.pred, d.lp_out, d.backptr = L.ptr(bpred), L.ptr(blp), L.ptr(bbp)
    d.scratch_val, d.scratch_idx = L.ptr(sval), L.ptr(sidx)
    d.last_pred, d.last_lp, d.step_index = L.ptr(lastd), L.ptr(phid), 1
    lib.ssc_beam_step_fsm(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(tok1, bpred.cpu().numpy()) and same_bits(bp1, bbp.cpu().numpy()) and same_bits(lp1, blp.cpu().numpy())


def test_strong_penalty_gives_pairwise_distinct_tokens():
    """k' = 1, n = 1, strength 1e4 (far above the spread of a row's log-probs): the live beams of an entry pick pairwise distinct
    tokens at a step, even when every row prefers the same token."""
    V, k, B = 500, 20, 3
    rng = np.random.default_rng(9)
    st = Steps(B, k, k, 1, V, 1e4, True)
    x0 = make_rows(rng, B, V, False)
    tok, lp = st.first(x0)
    assert all(len(set(r)) == k for r in tok.tolist())
    x = make_rows(rng, B * k, V, False)
    x[:, 17] += 30.0   # every row's favourite
    last = tok.copy()
    last[0, 5] = last[1, 0] = R.END
    tok1, lp1, bp1 = st.step(x, 1, last, lp)
    for b in range(B):
        live = [t for t, l in zip(tok1[b].tolist(), last[b].tolist()) if l != R.END]
        assert len(set(live)) == len(live) and live.count(17) == 1
    assert (bp1 == np.arange(k)[None]).all()


def test_two_calls_are_bit_identical():
    V, k, Gr, n, B = 3000, 12, 4, 2, 5
    rng = np.random.default_rng(2)
    st = Steps(B, k, Gr, n, V, 0.5, True)
    x = make_rows(rng, B * k, V, True)
    last = rng.integers(2, V, (B, k))
    phi = rng.uniform(-9, -1, (B, k)).astype(F)
    a = [v.copy() for v in st.step(x, 1, last, phi)]
    b = st.step(x, 1, last, phi)
    assert all(same_bits(u, v) for u, v in zip(a, b))


def test_bad_descriptors_launch_nothing():
    V, B = 90, 2
    x = torch.randn(B * 33, V, device="cuda")
    lib = L.load()

    def refused(k, Gr, lam, machine=False, n=1, calls=("first", "step")):
        st = Steps(B, k, Gr, n, V, lam, True)
        d = st.desc(x)
        if machine:
            d.dims = L.FsmDims(B, 2, V, 0, 1)
        for call in calls:
            if call == "step":
                last = torch.full((B, k), 3, dtype=torch.int64, device="cuda")
                phi = torch.zeros(B, k, device="cuda")
                d.last_pred, d.last_lp, d.step_index = L.ptr(last), L.ptr(phi), 1
            with pytest.raises(L.SscError, match="SSC_EINVAL"):
                getattr(lib, f"ssc_beam_{call}_diverse")(C.byref(d), C.byref(st.s), L.stream_ptr())
        torch.cuda.synchronize()
        assert (st.pred == -7).all() and (st.lp == 7.0).all() and (st.bp == -7).all()

    refused(6, 4, 0.5)
    refused(6, 0, 0.5)
    refused(6, 3, -0.5)
    refused(6, 3, float("inf"))
    refused(6, 3, float("nan"))
    refused(6, 3, 0.5, machine=True)
    refused(33, 3, 0.5)
    refused(6, 3, 0.5, n=33, calls=("step",))   # (step 0 takes no per_node)
    # the one-call search refuses the same
    cfg, _, _, dec = model(False)
    feats, senti, eps0, eps = inputs(cfg, 2, 2, 5, seed=1)
    ctx = dec.prepare(feats.cuda())
    with pytest.raises(ValueError, match="multiple"):
        dec.diverse_beam(ctx, None, 2, 6, 1, 4, cfg.boundary_index, eps0, eps.repeat_interleave(6, 1)[:3], sampling.DiverseBeam(4, 0.5))
    bad = sampling.DiverseBeam(3, 0.5)
    bad.strength = -1.0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        dec.diverse_beam(ctx, None, 2, 6, 1, 4, cfg.boundary_index, eps0, eps.repeat_interleave(6, 1)[:3], bad)


# ---- the whole search ----------------------------------------------------------------------------------------------------------

def _entry_inputs(cfg, nimg, ns, R_, k, seed, steps=None):
    feats, senti, eps0, eps = inputs(cfg, nimg, ns, R_, seed, steps)
    return feats, senti, eps0, eps.repeat_interleave(k, dim=1)


def stepwise_search(dec, ctx, sent_b, B, k, Gr, n, lam, steps, end, eps0, eps, early_stop=False, skip_dead=False):
    """The search driven from Python: DecodeEngine.step (raw logits) + ssc_beam_first_diverse / ssc_beam_step_diverse, the states
    re-ordered by back-pointer as cbs_search does.  -> (predictions (B, k, steps'), log-probs (B, k), per-step tokens / log-probs
    / back-pointers, ctl[0] or None)."""
    lib = L.load()
    dev = "cuda"
    V = dec.dims.V
    m = max(list_len(k, Gr, n, V), k)
    s = L.DiverseDesc(Gr, lam)
    preds = torch.empty(steps, B, k, dtype=torch.int64, device=dev)
    backs = torch.empty(max(steps - 1, 1), B, k, dtype=torch.int64, device=dev)
    sval = torch.empty(B * k * m, dtype=torch.float32, device=dev)
    sidx = torch.empty(B * k * m, dtype=torch.int64, device=dev)
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
    lib.ssc_beam_first_diverse(C.byref(d), C.byref(s), L.stream_ptr())
    lps = [last_lp]
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
        lib.ssc_beam_step_diverse(C.byref(d), C.byref(s), L.stream_ptr())
        last_lp = new_lp
        lps.append(new_lp)
        idx = (torch.arange(B, device=dev).view(B, 1) * k + backs[t - 1]).reshape(-1)
        states = {key: v[idx].contiguous() for key, v in states.items() if not key.startswith("_")}
        states["_parent"] = backs[t - 1]
        ran = t + 1
    out = torch.empty(B, k, ran, dtype=torch.int64, device=dev)
    lib.ssc_beam_backtrace(L.ptr(preds), L.ptr(backs), ran, B, k, L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    nsteps = int(ctl[0]) if ctl is not None else ran
    rec = {"tok": [preds[t].cpu().numpy() for t in range(ran)], "lp": [x.cpu().numpy() for x in lps],
           "bp": [None] + [backs[t].cpu().numpy() for t in range(ran - 1)]}
    return out[:, :, :nsteps].cpu(), last_lp.cpu(), rec, nsteps if ctl is not None else None


@pytest.mark.parametrize("early_stop,skip_dead", [(False, False), (True, True), (True, False), (False, True)])
def test_one_call_search_equals_the_stepwise_search(early_stop, skip_dead):
    """ssc_decode_diverse_beam against the same search driven step by step from Python, bit for bit."""
    cfg, _, _, dec = model(False, boundary_bias=2.0)
    nimg, ns, R_, k, Gr, n, lam = 3, 4, 7, 6, 3, 1, 0.5
    steps = cfg.max_caption_length
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=5)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    div = sampling.DiverseBeam(Gr, lam)
    pred, lps = dec.diverse_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, div, early_stop=early_stop,
                                 skip_dead=skip_dead)
    want, want_lp, _, _ = stepwise_search(dec, ctx, sent_b, B, k, Gr, n, lam, steps, cfg.boundary_index, eps0, eps,
                                          early_stop=early_stop, skip_dead=skip_dead)
    assert pred.shape == want.shape
    assert torch.equal(pred.cpu(), want)
    assert same_bits(lps.cpu().numpy(), want_lp.numpy())
    ended = (pred == cfg.boundary_index).cumsum(-1) > 0
    assert (pred[ended] == cfg.boundary_index).all()


def test_search_stops_when_every_beam_has_ended():
    """An overwhelming end token from step 1 on: ctl[0] < max_steps, the call returns ctl[0] columns, and without early stop the
    surplus columns hold end_index."""
    cfg, params, _, dec = model(False, boundary_bias=6.0)
    nimg, ns, R_, k, Gr, n, lam = 2, 3, 5, 4, 2, 1, 0.5
    steps = cfg.max_caption_length
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R_, k, seed=8)
    B = nimg * ns
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    div = sampling.DiverseBeam(Gr, lam)
    a, alp = dec.diverse_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, div)
    want, want_lp, _, nsteps = stepwise_search(dec, ctx, sent_b, B, k, Gr, n, lam, steps, cfg.boundary_index, eps0, eps,
                                               early_stop=True)
    assert nsteps < steps and a.size(-1) == nsteps
    assert torch.equal(a.cpu(), want) and same_bits(alp.cpu().numpy(), want_lp.numpy())
    full, flp = dec.diverse_beam(ctx, sent_b, ns, k, n, steps, cfg.boundary_index, eps0, eps, div, early_stop=False)
    assert full.size(-1) == steps and torch.equal(full[..., :nsteps], a) and (full[..., nsteps:] == cfg.boundary_index).all()
    assert torch.equal(flp, alp)


def oracle_search(cfg, params, feats, senti, eps0, eps, nimg, ns, k, Gr, n, lam, steps):
    """tests/dbsref.search driven by the oracle's eval decode step -> its record (per-step tokens, log-probs, back-pointers and
    selection margins)."""
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

    return R.search(step, None, B, k, Gr, n, lam, steps, end=end, early_stop=False)[2]


MARGIN = 2e-4   # the selection margin beyond which a 1e-4 log-prob tolerance cannot flip a choice
# `sharp` scales the output layer of the randomly initialised model: as initialised its distributions are nearly uniform and the
# best tokens of a row lie ~1e-4 apart, so that hardly any selection could be compared
ORACLE_CASES = {False: dict(nimg=3, ns=4, R_=7, steps=9, seed=5, sharp=8.0), True: dict(nimg=2, ns=3, R_=36, steps=6, seed=1, sharp=4.0)}


def sharp_model(full, sharp):
    """test_sampling_gpu.model with the output layer's weights scaled by `sharp` -> (cfg, params, DecodeEngine)."""
    from gpuutil import engine_from
    from ssc_runtime.decode import DecodeEngine
    cfg, params, _, _ = model(full)
    params = {k_: v.clone() for k_, v in params.items()}
    params["_output_layer.weight"] *= sharp
    eng = engine_from(cfg, params)
    return cfg, params, DecodeEngine(eng.dims, eng.params.c_struct, "cuda"), eng


def compare_with_oracle(rec, dev, B, Gr, k):
    """-> (pairs compared to the end, pairs in all, largest log-prob difference).  Group g of an entry depends on the groups
    before it (their selections are its counts) and on no later one, so the pair (entry, g) is compared up to the first step at
    which a selection of one of the entry's groups 0 .. g has a sub-margin gap, and then counts as cut short."""
    kp = k // Gr
    alive = np.ones((B, Gr), dtype=bool)
    worst = 0.0
    for t in range(len(rec["tok"])):
        alive &= np.logical_and.accumulate(rec["margin"][t] > MARGIN, axis=1)
        if not alive.any():
            break
        sel = np.repeat(alive, kp, axis=1)   # (B, k): the beams of the pairs still compared
        assert np.array_equal(dev["tok"][t][sel], rec["tok"][t][sel]), t
        if t > 0:
            assert np.array_equal(dev["bp"][t][sel], rec["bp"][t][sel]), t
        fin = np.isfinite(rec["lp"][t][sel])
        diff = np.abs(dev["lp"][t][sel][fin].astype(np.float64) - rec["lp"][t][sel][fin])
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
    return int(alive.sum()), B * Gr, worst


@pytest.mark.parametrize("gemm_mode", [0, 2])
@pytest.mark.parametrize("full", [False, True])
def test_against_the_cpu_oracle(full, gemm_mode):
    """tests/dbsref.py driven by the oracle's eval decode step, against the device search driven step by step, k = 6, Gr = 3,
    n = 1, strength 0.5: toy width (3 images x 4 samples, 9 steps) and full width (H 1200, V 10 000, R 36, 2 images x 3 samples,
    6 steps), in the engine's default GEMM mode and in gemm_mode 2 (exact fp32).  Log-probs within 1e-4; tokens and
    back-pointers identical at every (entry, step, group) whose oracle selection margins exceed 2e-4; a pair (entry, group) is
    followed up to its first sub-margin step.  At most 10 % of the pairs may be cut short that way.  The oracle side alone, on
    the CPU, cuts short 0 of 36 pairs at toy width (seed 5, smallest margin 4.7e-4) and 0 of 18 at full width (seed 1, smallest
    margin 5.2e-4)."""
    c = ORACLE_CASES[full]
    cfg, params, dec, _eng = sharp_model(full, c["sharp"])
    if gemm_mode:
        dec._cfg.gemm_mode = gemm_mode   # (what an engine-wide ModelDims.gemm_mode sets)
    nimg, ns, k, Gr, n, lam, steps = c["nimg"], c["ns"], 6, 3, 1, 0.5, c["steps"]
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, c["R_"], k, seed=c["seed"], steps=steps)
    B = nimg * ns
    rec = oracle_search(cfg, params, feats, senti, eps0, eps, nimg, ns, k, Gr, n, lam, steps)
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    _, _, dev, _ = stepwise_search(dec, ctx, sent_b, B, k, Gr, n, lam, steps, cfg.boundary_index, eps0, eps)
    whole, pairs, worst = compare_with_oracle(rec, dev, B, Gr, k)
    print(f"oracle parity full={full} gemm_mode={gemm_mode}: {pairs - whole} of {pairs} pairs cut short, max |dlp| {worst:.3g}")
    assert worst < 1e-4
    assert pairs - whole <= 0.1 * pairs


# ---- the public interface ------------------------------------------------------------------------------------------------------

def test_diverse_decode_both_return_forms():
    cfg, _, _, dec = model(False)
    feats = torch.randn(3, 7, cfg.image_feature_size).cuda()
    senti = torch.tensor([1.0, 0.0, -1.0]).cuda()
    div = sampling.DiverseBeam(3, 0.5)
    L_ = cfg.max_caption_length
    torch.manual_seed(0)
    best, steps = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index, diverse_beam=div)
    torch.manual_seed(0)
    groups, steps2, glp = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index, diverse_beam=div, return_groups=True)
    assert best.shape == (3, 4, steps) and groups.shape == (3, 4, 3, steps) and glp.shape == (3, 4, 3) and steps == steps2
    pick = glp.argmax(-1)
    assert torch.equal(best, groups.gather(2, pick.view(3, 4, 1, 1).expand(3, 4, 1, steps)).squeeze(2))
    # the group's best is the arg-max inside the group of the engine's own output
    torch.manual_seed(0)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    B = 12
    eps0 = torch.randn(B, cfg.z_space, device="cuda", generator=gen)
    eps = torch.randn(max(L_ - 1, 1), B * 6, cfg.z_space, device="cuda", generator=gen)
    ctx = dec.prepare(feats)
    beams, lps = dec.diverse_beam(ctx, senti.view(3, 1).expand(3, 4).reshape(B), 4, 6, div.per_node(6), L_, cfg.boundary_index,
                                  eps0, eps, div)
    gi = lps.view(B, 3, 2).argmax(-1)
    want = beams.view(B, 3, 2, -1).gather(2, gi.view(B, 3, 1, 1).expand(B, 3, 1, beams.size(-1))).squeeze(2)
    assert torch.equal(groups.view(B, 3, -1), want)
    assert torch.equal(glp.view(B, 3), lps.view(B, 3, 2).max(-1).values)
    # one group: the beam search's captions
    torch.manual_seed(0)
    one, _ = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index, diverse_beam=sampling.DiverseBeam(1, 0.5))
    torch.manual_seed(0)
    beam, _ = diverse_decode(dec, feats, senti, 4, 6, L_, cfg.boundary_index)
    assert torch.equal(one, beam)
    with pytest.raises(ValueError, match="sampler"):
        diverse_decode(dec, feats, senti, 2, 6, 5, cfg.boundary_index, diverse_beam=div, sampler=sampling.TopKSampler(k=3))
    with pytest.raises(ValueError, match="constraints"):
        diverse_decode(dec, feats, senti, 2, 6, 5, cfg.boundary_index, diverse_beam=div,
                       fsm=torch.ones(3, 1, 1, cfg.vocab_size, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="multiple"):
        diverse_decode(dec, feats, senti, 2, 5, 5, cfg.boundary_index, diverse_beam=div)
    with pytest.raises(ValueError, match="return_groups"):
        diverse_decode(dec, feats, senti, 2, 5, 5, cfg.boundary_index, return_groups=True)


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", {seed!r}, "MODEL.DIVERSE_BEAM_SEARCH", "True", "MODEL.DIVERSE_BEAM_GROUPS", "3",
                            "MODEL.DIVERSE_BEAM_STRENGTH", "0.5", "MODEL.BEAM_SIZE", "6",
                            "MODEL.IMAGE_FEATURE_SIZE", "64", "MODEL.EMBEDDING_SIZE", "40", "MODEL.HIDDEN_SIZE", "48",
                            "MODEL.ATTENTION_PROJECTION_SIZE", "32", "MODEL.Z_SPACE", "16", "DATA.MAX_CAPTION_LENGTH", "8"])
torch.manual_seed(C.RANDOM_SEED)
m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                sampler=sampling.from_config(C.MODEL),
                                diverse_beam=sampling.diverse_beam_from_config(C.MODEL)).cuda().eval()
assert m.diverse_beam is not None and m.diverse_beam.groups == 3
g = torch.Generator().manual_seed(0)
feats = torch.randn(8, 6, 64, generator=g).cuda()
out = m(feats)["predictions"]
print(json.dumps(out.cpu().tolist()))
"""


def test_module_forward():
    outs = {}
    for seed in ("3", "3"):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"), seed=seed)
        outs.setdefault(seed, []).append(json.loads(run_child(["-c", src]).strip().splitlines()[-1]))
    a, b = outs["3"]
    assert a == b and len(a) == 8 and all(0 < len(c) <= 8 for c in a)
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    with pytest.raises(ValueError, match="BEAM_SIZE"):
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=5, z_space=4, diverse_beam=sampling.DiverseBeam(3, 0.5))
    with pytest.raises(ValueError, match="DIVERSE_BEAM_SEARCH"):
        UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4, diverse_beam=sampling.DiverseBeam(3, 0.5),
                        sampler=sampling.GumbelSampler())
    m = UpDownCaptioner(Vocabulary.synthetic(50), 16, 8, 16, 8, beam_size=6, z_space=4,
                        diverse_beam=sampling.DiverseBeam(3, 0.5)).cuda().eval()
    m._use_cbs = True
    with pytest.raises(ValueError, match="USE_CBS"):
        m(torch.randn(2, 3, 16, device="cuda"), fsm=torch.ones(2, 1, 1, 50, dtype=torch.uint8))


def test_inference_script_with_diverse_beam_search(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
                   "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
                   "  BEAM_SIZE: 6\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
                   "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 2\n")
    outs = []
    for i in range(2):
        out = tmp_path / f"pred{i}.json"
        run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4",
                   "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--config-override",
                   "MODEL.DIVERSE_BEAM_SEARCH", "True", "MODEL.DIVERSE_BEAM_GROUPS", "3", "MODEL.DIVERSE_BEAM_STRENGTH", "0.5"])
        outs.append(json.load(open(out)))
    caps = outs[0]
    assert len(caps) == 4 * 2 * 3 and all(isinstance(c["caption"], str) for c in caps)
    assert outs[0] == outs[1]   # a fixed RANDOM_SEED: the same captions
