"""GPU: ensemble decoding - ssc_ensemble_combine_rows against ssc_log_softmax and the float64 restatement (tests/ensembleref.py),
ssc_decode_search_ensemble (EnsembleDecodeEngine.search) against the single-model search, against the same search driven step by
step from Python and against the CPU oracle, and the public interface (CaptionerEnsemble, scripts/inference.py)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import dbsref
import ensembleref as E
import oracle
from goldenlib import load_raw, unpack_fsm
from gpuutil import engine_from
from ssc_runtime import lib as L
from ssc_runtime.decode import CompiledFsm, DecodeEngine, EnsembleDecodeEngine
from ssc_runtime.inference import diverse_decode
from test_dbs_gpu import MARGIN, _entry_inputs, compare_with_oracle, device_log_softmax, make_rows, same_bits
from test_sampling_gpu import ROOT, model, run_child

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 7.25


# ---- the kernel ------------------------------------------------------------------------------------------------------------------

def combine_dev(xs, logw, mode, V=None, last_pred=None, row_lp=None, end=0, out=None, check=True):
    """ssc_ensemble_combine_rows over device tensors xs[m] (rows, >= V) with leading dimension xs[m].stride(0) -> (rc, out)."""
    lib = L.load()
    M = len(xs)
    rows = xs[0].size(0)
    V = V or xs[0].size(1)
    if out is None:
        out = torch.full((rows, V), SENTINEL, dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * M)(*[x.data_ptr() for x in xs])
    lw = (C.c_float * M)(*[float(v) for v in logw])
    d = L.EnsembleRowsDesc(M, ptrs, xs[0].stride(0), lw, mode)
    rc = lib._raw_ssc_ensemble_combine_rows(C.byref(d), rows, V, L.ptr(last_pred), L.ptr(row_lp), end, L.ptr(out), out.stride(0),
                                            L.stream_ptr())
    torch.cuda.synchronize()
    assert not check or rc == 0, rc
    return rc, out


ROWS = 300
WEIGHTS = np.array([5.0, 1.0, 3.0, 2.0, 0.5, 4.0, 1.5, 0.25])   # uneven


@functools.lru_cache(maxsize=None)
def kernel_case(V):
    """Member logits (8, ROWS, V) float32, made once per V and left unchanged: the odd rows with exact ties (a 1/4 grid, half of the
    row a copy of the other half), member 1 with a logit at -1e30 in rows 2 and 200; the float64 log-softmax of every member row;
    ssc_log_softmax of the same rows (the parent commit's kernel).  Its error against float64 is taken by log_softmax_error over
    exactly the members and rows a call reads."""
    rng = np.random.default_rng(V)
    x = np.stack([np.where((np.arange(ROWS) % 2 == 1)[:, None], make_rows(rng, ROWS, V, True), make_rows(rng, ROWS, V, False))
                  for _ in range(8)]).astype(F)
    x[1, 2, 5] = x[1, 200, V - 1] = F(-1e30)
    ref = E.log_softmax64(x)
    dev = np.stack([device_log_softmax(x[m]) for m in range(8)])
    return x, ref, dev


def log_softmax_error(ref, dev, M, rows):
    """ssc_log_softmax's largest error against float64 on members 0 .. M - 1, rows 0 .. rows - 1: the ordinary entries (the -1e30
    logit is compared relatively: one fp32 ulp of 1e30 is 7.6e22)."""
    r, d = ref[:M, :rows], dev[:M, :rows].astype(np.float64)
    ordinary = np.abs(r) < 1e6
    assert np.all(np.abs(d - r)[~ordinary] <= 2.0 ** -23 * np.abs(r[~ordinary]))
    return float(np.abs(d - r)[ordinary].max())


def check_against_ref(got, want, M, err_ls, what):
    """(M + 2) x the log-softmax's own error: one such reduction per member, the sum and - mode 1 - the renormalisation.  An entry
    whose exact value is huge (mode 1 next to the -1e30 logit: ~ -1e29) cannot be nearer than its own fp32 rounding, so such
    entries get the same factor on 2^-23 of their magnitude."""
    got = got.astype(np.float64)
    ordinary = np.abs(want) < 1e6
    worst = float(np.abs(got - want)[ordinary].max())
    print(f"{what}: ssc_log_softmax max error {err_ls:.3g}, combine max error {worst:.3g}, allowed {(M + 2) * err_ls:.3g}")
    assert worst <= (M + 2) * err_ls
    if (~ordinary).any():
        assert np.all(np.abs(got - want)[~ordinary] <= (M + 2) * 2.0 ** -23 * np.abs(want[~ordinary]))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("V", [90, 1000, 10000])
def test_combine_against_float64(V, M, mode):
    """rows 7 and 300 of the case of `V` (ties, a -1e30 logit, uneven weights), M members.  M = 1, mode 0: bit-equal to
    ssc_log_softmax.  Otherwise within (M + 2) x ssc_log_softmax's own largest error against float64 on the M members and the
    rows of that call, measured here (check_against_ref prints both).  Observed on one MI355X: ssc_log_softmax's error between
    5.86e-7 (V 90, M 1, 7 rows) and 1.87e-6 (V 10 000, 300 rows); the combine's largest error per V 2.25e-6 (V 90, M 8, mode 1, 300
    rows; allowed 1.17e-5), 3.37e-6 (V 1000, M 2, mode 1, 300 rows; allowed 6.37e-6), 4.21e-6 (V 10 000, M 2, mode 1, 300 rows;
    allowed 7.44e-6); nearest to its bound: 3.09e-6 of 5.23e-6 allowed (V 10 000, M 2, mode 1, 7 rows); mode 0 stays below 2.8e-6
    everywhere."""
    x, ref, dev = kernel_case(V)
    w = E.normalise(WEIGHTS[:M], M)
    logw = np.log(w).astype(F)
    want = E.combine_log_probs(ref[:M], np.exp(logw.astype(np.float64)), mode)
    for rows in (7, ROWS):
        xs = [torch.from_numpy(x[m, :rows]).cuda() for m in range(M)]
        _, out = combine_dev(xs, logw, mode)
        got = out.cpu().numpy()
        if M == 1 and mode == 0:
            assert same_bits(got, dev[0, :rows])
        else:
            check_against_ref(got, want[:rows], M, log_softmax_error(ref, dev, M, rows), f"V {V} M {M} mode {mode} rows {rows}")
        _, again = combine_dev(xs, logw, mode)
        assert same_bits(again.cpu().numpy(), got)   # two calls: the same bits


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V,ld,ldo", [(90, 92, 92), (1000, 1004, 1000), (1000, 1001, 1003), (10000, 10004, 10004)])
def test_combine_leading_dimensions(V, ld, ldo, mode):
    """ld > V: 16-byte rows with a scalar tail (90 in 92), 16-byte rows (1000 in 1004), rows that are not 16-byte aligned (1001) -
    the same bits as the packed call, and nothing written behind a row's V entries."""
    x, _, _ = kernel_case(V)
    M, rows = 3, 7
    logw = np.log(E.normalise(WEIGHTS[:M], M)).astype(F)
    packed = [torch.from_numpy(x[m, :rows]).cuda() for m in range(M)]
    _, want = combine_dev(packed, logw, mode)
    wide = []
    for m in range(M):
        t = torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")
        t[:, :V] = packed[m]
        wide.append(t)
    out = torch.full((rows, ldo), SENTINEL, dtype=torch.float32, device="cuda")
    combine_dev(wide, logw, mode, V=V, out=out)
    assert same_bits(out[:, :V].cpu().numpy(), want.cpu().numpy())
    assert bool((out[:, V:] == SENTINEL).all())


@pytest.mark.parametrize("mode", [0, 1])
def test_combine_skips_ended_and_dead_rows(mode):
    """Rows whose last token is end_index or whose running log-prob is <= -1e19 keep the sentinel the output was filled with (their
    inputs hold NaNs: a read would show); the live rows are those of the call without the lists.  Either list may be missing."""
    V, M, rows, end = 1000, 2, 12, 3
    x, _, _ = kernel_case(V)
    logw = np.log(E.normalise(WEIGHTS[:M], M)).astype(F)
    last = torch.tensor([0, end, 5, 5, end, 7, 8, 9, end, 2, 2, 2], dtype=torch.int64, device="cuda")
    lp = torch.tensor([-1.0, -2.0, -1e20, -3.0, -1e20, 0.0, -1e19, -5.0, -1.0, -9e18, -2.0, -float("inf")], device="cuda")
    xs = [torch.from_numpy(x[m, :rows]).cuda() for m in range(M)]
    _, full = combine_dev(xs, logw, mode)
    for use_last, use_lp in ((True, True), (True, False), (False, True)):
        skipped = torch.zeros(rows, dtype=torch.bool, device="cuda")
        if use_last:
            skipped |= last == end
        if use_lp:
            skipped |= lp <= -1e19
        poisoned = [t.clone() for t in xs]
        for t in poisoned:
            t[skipped] = float("nan")
        _, out = combine_dev(poisoned, logw, mode, last_pred=last if use_last else None, row_lp=lp if use_lp else None, end=end)
        assert 0 < int(skipped.sum()) < rows
        assert bool((out[skipped] == SENTINEL).all())
        assert same_bits(out[~skipped].cpu().numpy(), full[~skipped].cpu().numpy())
        assert not bool((out[~skipped] == SENTINEL).any())


@pytest.mark.parametrize("mode", [0, 1])
def test_a_nan_logit_makes_the_row_nan(mode):
    """A NaN in one member's row: that member's log-sum-exp is NaN, as under ssc_log_softmax, and the whole output row is NaN -
    M = 1 / mode 0 has ssc_log_softmax's NaN pattern; the other rows are those of the call without the NaN."""
    V, rows = 1000, 7
    x, _, _ = kernel_case(V)
    for M in (1, 2):
        logw = np.log(E.normalise(WEIGHTS[:M], M)).astype(F)
        xs = [torch.from_numpy(x[m, :rows]).cuda() for m in range(M)]
        _, clean = combine_dev(xs, logw, mode)
        xs[M - 1][3, 17] = float("nan")
        _, out = combine_dev(xs, logw, mode)
        assert bool(torch.isnan(out[3]).all())
        keep = [r for r in range(rows) if r != 3]
        assert same_bits(out[keep].cpu().numpy(), clean[keep].cpu().numpy())
        if M == 1:
            assert np.array_equal(np.isnan(device_log_softmax(xs[0].cpu().numpy())), torch.isnan(out).cpu().numpy())


def test_combine_bad_descriptors_leave_the_output_untouched():
    V, rows = 90, 7
    x, _, _ = kernel_case(V)
    xs = [torch.from_numpy(x[m, :rows]).cuda() for m in range(2)]
    ok = np.log([0.5, 0.5]).astype(F)
    lib = L.load()

    def rc(M=2, ld=V, logw=ok, mode=0, V_=V, null=False, ldo=V):
        out = torch.full((rows, V), SENTINEL, dtype=torch.float32, device="cuda")
        n = max(M, 1)
        ptrs = (C.c_void_p * n)(*[(xs[m % 2].data_ptr() if not (null and m == n - 1) else None) for m in range(n)])
        lw = (C.c_float * n)(*[float(logw[m % 2]) for m in range(n)])
        d = L.EnsembleRowsDesc(M, ptrs, ld, lw, mode)
        r = lib._raw_ssc_ensemble_combine_rows(C.byref(d), rows, V_, None, None, 0, L.ptr(out), ldo, L.stream_ptr())
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        return r

    assert rc(M=0) == -1 and rc(M=9) == -1
    assert rc(null=True) == -1
    assert rc(V_=0) == -1
    assert rc(ld=V - 1) == -1
    assert rc(ldo=V - 1) == -1
    assert rc(mode=2) == -1
    assert rc(logw=np.array([0.0, np.nan], dtype=F)) == -1
    assert rc(logw=np.array([-np.inf, 0.0], dtype=F)) == -1


# ---- the driver ------------------------------------------------------------------------------------------------------------------

def toy_members(seeds=(4, 5, 6), boundary_bias=0.0, sharp=1.0, full=False, V=None):
    """test_sampling_gpu.model(full) per seed (the output layer's weights scaled by `sharp`, V other than the model's 90 on request)
    -> (cfg, [params], [DecodeEngine], keep-alive)."""
    if V is None and sharp == 1.0:
        got = [model(full, seed=s, boundary_bias=boundary_bias) for s in seeds]
        return got[0][0], [g[1] for g in got], [g[3] for g in got], [g[2] for g in got]
    cfg = model_cfg(full)
    if V is not None:
        cfg.vocab_size = V
    plist, decs, engs = [], [], []
    for s in seeds:
        params = oracle.init_params(cfg, seed=s)
        params["_output_layer.bias"][cfg.boundary_index] += boundary_bias
        params["_output_layer.weight"] *= sharp
        eng = engine_from(cfg, params)
        plist.append(params)
        engs.append(eng)
        decs.append(DecodeEngine(eng.dims, eng.params.c_struct, "cuda"))
    return cfg, plist, decs, engs


def stepwise_ensemble(decs, ctxs, weights, mode, sent_b, B, k, n, steps, end, eps0, eps, early_stop=False, skip_dead=False,
                      fsm=None, compiled=None):
    """The ensemble search driven from Python: DecodeEngine.step (raw logits) per member -> ssc_ensemble_combine_rows ->
    ssc_beam_first_fsm / ssc_beam_step_fsm (raw_logits 0) -> every member's states re-ordered by back-pointer.
    -> (predictions (B, S, k, steps'), log-probs (B, S, k), per-step record, ctl[0] or None)."""
    lib = L.load()
    dev = "cuda"
    M = len(decs)
    V = decs[0].dims.V
    S = 1 if fsm is None else fsm.size(1)
    SB = S * k
    logw = np.log(E.normalise(weights, M)).astype(F)
    preds = torch.empty(steps, B, SB, dtype=torch.int64, device=dev)
    backs = torch.empty(max(steps - 1, 1), B, SB, dtype=torch.int64, device=dev)
    sval = torch.empty(B * S * SB * n, dtype=torch.float32, device=dev)
    sidx = torch.empty(B * S * SB * n, dtype=torch.int64, device=dev)
    ctl = None
    if early_stop:
        ctl = torch.zeros(2 + 2 * steps, dtype=torch.int32, device=dev)
        ctl[0] = steps
    last_lp = torch.empty(B, S, k, dtype=torch.float32, device=dev)
    start = torch.full((B,), end, dtype=torch.int64, device=dev)
    outs = [d.step(c, start, None, sent_b, eps0.cuda(), raw_logits=True) for d, c in zip(decs, ctxs)]
    _, lp = combine_dev([o[0] for o in outs], logw, E.MODES[mode])
    bd = L.BeamDesc()
    bd.raw_logits = 0
    bd.fsm = L.ptr(fsm)
    bd.tables = L.ptr(compiled.tables) if compiled is not None else None
    bd.dims = compiled.dims if compiled is not None else L.FsmDims(B, S, V, 0, 1)
    bd.B, bd.beam, bd.per_node, bd.end_index = B, k, n, end
    bd.ctl, bd.max_steps = L.ptr(ctl), steps
    bd.scratch_val, bd.scratch_idx = L.ptr(sval), L.ptr(sidx)
    bd.scores, bd.ld = L.ptr(lp), lp.stride(0)
    bd.pred, bd.lp_out = L.ptr(preds[0]), L.ptr(last_lp)
    lib.ssc_beam_first_fsm(C.byref(bd), L.stream_ptr())
    bd.skip_dead = 1 if (skip_dead and compiled is not None) else 0
    lps = [last_lp]
    states = []
    for o in outs:
        st = {key: v.repeat_interleave(SB, 0).contiguous() for key, v in o[1].items() if not key.startswith("_")}
        st["_parent"] = torch.zeros(B, SB, dtype=torch.int64, device=dev)
        states.append(st)
    sent_rows = sent_b.repeat_interleave(SB) if sent_b is not None else None
    ran = 1
    for t in range(1, steps):
        if ctl is not None and int(ctl[0]) <= t:
            break
        last = preds[t - 1].reshape(B * SB)
        logits = []
        for m, (d, c) in enumerate(zip(decs, ctxs)):
            if skip_dead:
                states[m]["_skip"] = (last_lp, end)
            lg, states[m], _ = d.step(c, last, states[m], sent_rows, eps[t - 1].cuda(), raw_logits=True)
            logits.append(lg)
        _, lp = combine_dev(logits, logw, E.MODES[mode], last_pred=last if skip_dead else None,
                            row_lp=last_lp if skip_dead else None, end=end)
        new_lp = torch.empty_like(last_lp)
        bd.scores, bd.ld = L.ptr(lp), lp.stride(0)
        bd.last_pred, bd.last_lp = L.ptr(last), L.ptr(last_lp)
        bd.pred, bd.lp_out, bd.backptr = L.ptr(preds[t]), L.ptr(new_lp), L.ptr(backs[t - 1])
        bd.step_index = t
        lib.ssc_beam_step_fsm(C.byref(bd), L.stream_ptr())
        last_lp = new_lp
        lps.append(new_lp)
        idx = (torch.arange(B, device=dev).view(B, 1) * SB + backs[t - 1]).reshape(-1)
        for m in range(M):
            states[m] = {key: v[idx].contiguous() for key, v in states[m].items() if not key.startswith("_")}
            states[m]["_parent"] = backs[t - 1]
        ran = t + 1
    out = torch.empty(B, SB, ran, dtype=torch.int64, device=dev)
    lib.ssc_beam_backtrace(L.ptr(preds), L.ptr(backs), ran, B, SB, L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    nsteps = int(ctl[0]) if ctl is not None else ran
    rec = {"tok": [preds[t].cpu().numpy() for t in range(ran)], "lp": [x.view(B, SB).cpu().numpy() for x in lps],
           "bp": [None] + [backs[t].cpu().numpy() for t in range(ran - 1)]}
    return out[:, :, :nsteps].view(B, S, k, nsteps).cpu(), last_lp.cpu(), rec, nsteps if ctl is not None else None


NIMG, NS, R_, K, N = 3, 4, 7, 3, 2   # the driver tests' extents: 3 images x 4 samples, beam 3, per_node 2


def search_inputs(cfg, nimg=NIMG, ns=NS, R__=R_, k=K, seed=5, S=1, steps=None):
    feats, senti, eps0, eps = _entry_inputs(cfg, nimg, ns, R__, k * S, seed=seed, steps=steps)
    B = nimg * ns
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda()
    return feats.cuda(), sent_b, eps0, eps


def test_one_member_is_the_single_model_search():
    """(a) M = 1: the predictions and log-probs of DecodeEngine.search, bit for bit (the combine of one member at weight 1 is
    ssc_log_softmax, which is what the selection takes from raw logits)."""
    cfg, _, decs, _keep = toy_members(seeds=(4,))
    feats, sent_b, eps0, eps = search_inputs(cfg)
    L_, end = cfg.max_caption_length, cfg.boundary_index
    for early_stop, skip_dead in ((True, False), (False, True)):
        want, want_lp = decs[0].search(decs[0].prepare(feats), sent_b, NS, K, N, L_, end, eps0, eps, early_stop=early_stop,
                                       skip_dead=skip_dead)
        ens = EnsembleDecodeEngine(decs)
        got, got_lp = ens.search(ens.prepare(feats), sent_b, NS, K, N, L_, end, eps0, eps, early_stop=early_stop, skip_dead=skip_dead)
        assert torch.equal(got, want) and same_bits(got_lp.cpu().numpy(), want_lp.cpu().numpy())


@pytest.mark.parametrize("early_stop,skip_dead", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_one_call_equals_the_stepwise_search(mode, early_stop, skip_dead):
    """(b) M = 3: ssc_decode_search_ensemble against the same search driven step by step from Python, bit for bit."""
    cfg, _, decs, _keep = toy_members(boundary_bias=2.0)
    feats, sent_b, eps0, eps = search_inputs(cfg)
    L_, end = cfg.max_caption_length, cfg.boundary_index
    weights = [0.5, 0.3, 0.2]
    ens = EnsembleDecodeEngine(decs, weights, mode)
    ctx = ens.prepare(feats)
    got, got_lp = ens.search(ctx, sent_b, NS, K, N, L_, end, eps0, eps, early_stop=early_stop, skip_dead=skip_dead)
    want, want_lp, _, _ = stepwise_ensemble(decs, ctx.ctxs, weights, mode, sent_b, NIMG * NS, K, N, L_, end, eps0, eps,
                                            early_stop=early_stop, skip_dead=skip_dead)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert same_bits(got_lp.cpu().numpy(), want_lp.numpy())
    ended = (got == end).cumsum(-1) > 0
    assert (got[ended] == end).all()


@pytest.mark.parametrize("nimg,ns,ungathered", [(2, 256, False), (8, 64, True)])
def test_table_and_ungathered_form(nimg, ns, ungathered):
    """(c) 2 images x 256 samples: 512 batch entries, the smallest extent at which the call's first step forms the attended-feature
    tables (one per member) and every step reads them.  8 images x 64 samples: the fewest images at which the later steps also read
    their states un-gathered, through the back-pointers (ssc_decode_ungathered_ok), every member's alike.  M = 2 against the
    stepwise driver, which re-orders the states: predictions identical, log-probs within the 1e-5 of
    test_top1_sampling_equals_beam1_search."""
    cfg, _, decs, _keep = toy_members(seeds=(4, 5))
    feats, sent_b, eps0, eps = search_inputs(cfg, nimg, ns, seed=17)
    L_, end = cfg.max_caption_length, cfg.boundary_index
    ens = EnsembleDecodeEngine(decs, [0.6, 0.4])
    ctx = ens.prepare(feats)
    assert decs[0]._att_table_fits(ctx.ctxs[0], nimg * ns, ns)
    assert decs[0].ungathered_ok(ctx.ctxs[0], nimg * ns * K, K) == ungathered
    got, got_lp = ens.search(ctx, sent_b, ns, K, N, L_, end, eps0, eps, skip_dead=True)
    ctx2 = ens.prepare(feats)
    want, want_lp, _, _ = stepwise_ensemble(decs, ctx2.ctxs, [0.6, 0.4], "prob", sent_b, nimg * ns, K, N, L_, end, eps0, eps,
                                            early_stop=True, skip_dead=True)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    diff = (got_lp.cpu() - want_lp).abs()
    print(f"table / un-gathered form: max |dlp| {float(diff.max()):.3g}")
    assert bool((diff <= 1e-5 + 1.2e-7 * want_lp.abs()).all())


_G12 = load_raw("g12_cbs")


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_machine_dense_and_compiled(mode):
    """(d) The machines of g12_cbs case 2 (3 entries, S = 4, V = 97) through the dense scans and through the compiled form with
    skip_dead: bit-identical predictions and log-probs - under skip_dead the predictions wherever a beam is finite
    (ssc_beam_desc.skip_dead: only the tokens of beams at <= -1e19 may differ) -, and equal to the stepwise driver over the dense
    machine."""
    key = "search/case2"
    B, S, V, beam, per_node, steps = (int(x) for x in _G12[key + "/dims"])
    assert (S, V) == (4, 97)
    fsm = unpack_fsm(_G12[key + "/fsm_bits"], B, S, V).cuda().contiguous()
    cfg, _, decs, _keep = toy_members(seeds=(4, 5), V=V, boundary_bias=1.0)
    feats, sent_b, eps0, eps = search_inputs(cfg, B, 1, k=beam, S=S, seed=3, steps=steps)
    end = cfg.boundary_index
    ens = EnsembleDecodeEngine(decs, [2.0, 1.0], mode)
    ctx = ens.prepare(feats)
    dense, dense_lp = ens.search(ctx, sent_b, 1, beam, per_node, steps, end, eps0, eps, fsm=fsm, early_stop=False)
    comp = CompiledFsm(fsm, max_exceptions=V, fill=8)
    for skip in (False, True):
        got, got_lp = ens.search(ctx, sent_b, 1, beam, per_node, steps, end, eps0, eps, fsm=fsm, compiled=comp, skip_dead=skip,
                                 early_stop=False)
        assert same_bits(got_lp.cpu().numpy(), dense_lp.cpu().numpy())
        if skip:   # (ssc_beam_desc.skip_dead: only the tokens of beams at <= -1e19 may differ)
            finite = dense_lp > -1e19
            assert bool(finite.any()) and torch.equal(got[finite], dense[finite])
        else:
            assert torch.equal(got, dense)
    want, want_lp, _, _ = stepwise_ensemble(decs, ctx.ctxs, [2.0, 1.0], mode, sent_b, B, beam, per_node, steps, end, eps0, eps, fsm=fsm)
    assert torch.equal(dense.cpu(), want) and same_bits(dense_lp.cpu().numpy(), want_lp.numpy())


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_member_order_changes_no_prediction(mode):
    """(e) The members permuted together with their weights: the same captions (the sums run in another order: the log-probs may
    differ in their last bits)."""
    cfg, _, decs, _keep = toy_members()
    feats, sent_b, eps0, eps = search_inputs(cfg)
    L_, end = cfg.max_caption_length, cfg.boundary_index
    weights = [0.5, 0.3, 0.2]
    outs = []
    for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        ens = EnsembleDecodeEngine([decs[i] for i in perm], [weights[i] for i in perm], mode)
        outs.append(ens.search(ens.prepare(feats), sent_b, NS, K, N, L_, end, eps0, eps))
    for pred, lp in outs[1:]:
        assert torch.equal(pred, outs[0][0])
        assert float((lp - outs[0][1]).abs().max()) < 1e-5


def test_search_stops_when_every_beam_has_ended():
    """(f) boundary_bias 6: every beam ends early - ctl[0] < max_steps, the call returns ctl[0] columns; without early stop the
    surplus columns hold end_index."""
    cfg, _, decs, _keep = toy_members(boundary_bias=6.0)
    feats, sent_b, eps0, eps = search_inputs(cfg, seed=8)
    L_, end = cfg.max_caption_length, cfg.boundary_index
    ens = EnsembleDecodeEngine(decs)
    ctx = ens.prepare(feats)
    a, alp = ens.search(ctx, sent_b, NS, K, N, L_, end, eps0, eps)
    nsteps = a.size(-1)
    assert nsteps < L_
    full, flp = ens.search(ctx, sent_b, NS, K, N, L_, end, eps0, eps, early_stop=False)
    assert full.size(-1) == L_ and torch.equal(full[..., :nsteps], a) and bool((full[..., nsteps:] == end).all())
    assert torch.equal(flp, alp)


def test_unsupported_decodes_name_the_feature():
    cfg, _, decs, _keep = toy_members(seeds=(4, 5))
    feats, sent_b, eps0, eps = search_inputs(cfg)
    ens = EnsembleDecodeEngine(decs)
    with pytest.raises(NotImplementedError, match="attention"):
        ens.search(ens.prepare(feats), sent_b, NS, K, N, cfg.max_caption_length, cfg.boundary_index, eps0, eps, attention=True)
    from ssc_runtime import sampling
    with pytest.raises(NotImplementedError, match="ensemble"):
        diverse_decode(ens, feats, None, 2, 1, 5, cfg.boundary_index, sampler=sampling.TopKSampler(k=3))


# ---- against the CPU oracle ------------------------------------------------------------------------------------------------------

# (seeds of the members, seed of the inputs, `sharp`: test_dbs_gpu.sharp_model's scale of the output layer)
ORACLE_CASES = {False: dict(nimg=3, ns=4, R_=7, steps=9, members=(4, 5), seed=5, sharp=8.0),
                True: dict(nimg=2, ns=3, R_=36, steps=6, members=(4, 5), seed=1, sharp=4.0)}


def oracle_record(cfg, plist, weights, c):
    """tests/dbsref.search (one group, strength 0: the plain beam search, with its selection margins) driven by the oracle's decode
    step under every member (tests/ensembleref.oracle_step_fn) -> its record."""
    feats, senti, eps0, eps = _entry_inputs(cfg, c["nimg"], c["ns"], c["R_"], K, seed=c["seed"], steps=c["steps"])
    step = E.oracle_step_fn(cfg, plist, weights, 0, feats, senti, eps0, eps, c["nimg"], c["ns"])
    return dbsref.search(step, None, c["nimg"] * c["ns"], K, 1, N, 0.0, c["steps"], end=cfg.boundary_index, early_stop=False)[2]


@pytest.mark.parametrize("gemm_mode", [0, 2])
@pytest.mark.parametrize("full", [False, True])
def test_against_the_cpu_oracle(full, gemm_mode):
    """M = 2, mode "prob", weights (0.6, 0.4), beam 3, per_node 2: the oracle's ensemble search on the CPU against the device search
    driven step by step (which test_one_call_equals_the_stepwise_search ties to the one call), toy width (3 images x 4 samples, 9
    steps) and full width (H 1200, V 10 000, R 36, 2 images x 3 samples, 6 steps), in the engine's default GEMM mode and in
    gemm_mode 2.  Log-probs within 1e-4; tokens and back-pointers identical at every step whose oracle margin exceeds 2e-4; an
    entry is followed to its first sub-margin step; at most 10 % of the entries may be cut short.  The oracle side alone, on the
    CPU (oracle_margins() below), cuts short 0 of 12 entries at toy width (members 4 and 5, inputs 5, smallest margin 3.1e-4) and
    0 of 6 at full width (members 4 and 5, inputs 1, smallest margin 2.3e-4).  Observed on one MI355X: 0 of 12 / 0 of 6 cut short
    in both GEMM modes, max |dlp| 5.7e-6 / 3.8e-6 at toy width (default mode / mode 2) and 7.6e-6 / 1.1e-5 at full width."""
    c = ORACLE_CASES[full]
    cfg, plist, decs, _keep = toy_members(seeds=c["members"], sharp=c["sharp"], full=full)
    if gemm_mode:
        for d in decs:
            d._cfg.gemm_mode = gemm_mode
    weights = [0.6, 0.4]
    rec = oracle_record(cfg, plist, weights, c)
    feats, senti, eps0, eps = _entry_inputs(cfg, c["nimg"], c["ns"], c["R_"], K, seed=c["seed"], steps=c["steps"])
    B = c["nimg"] * c["ns"]
    sent_b = senti.view(c["nimg"], 1).expand(c["nimg"], c["ns"]).reshape(B).cuda()
    ctxs = [d.prepare(feats.cuda()) for d in decs]
    want, want_lp, dev, _ = stepwise_ensemble(decs, ctxs, weights, "prob", sent_b, B, K, N, c["steps"], cfg.boundary_index, eps0, eps)
    # ... and the one call at this width and in this GEMM mode: the stepwise driver's captions and log-probs, bit for bit
    ens = EnsembleDecodeEngine(decs, weights)
    got, got_lp = ens.search(ens.prepare(feats.cuda()), sent_b, c["ns"], K, N, c["steps"], cfg.boundary_index, eps0, eps,
                             early_stop=False)
    assert torch.equal(got.cpu(), want) and same_bits(got_lp.cpu().numpy(), want_lp.numpy())
    whole, entries, worst = compare_with_oracle(rec, dev, B, 1, K)
    print(f"oracle parity full={full} gemm_mode={gemm_mode}: {entries - whole} of {entries} entries cut short, max |dlp| {worst:.3g}")
    assert worst < 1e-4
    assert entries - whole <= 0.1 * entries


def test_full_width_one_call_with_state_planes():
    """Full width (H 1200, V 10 000, R 36), M = 2, 8 images x 22 samples x beam 3 = 528 rows per step, the default 2xFP16
    numerics (gemm_mode 3): the extent at which the later steps read every member's states un-gathered and each member carries
    its own two generations of fp16 state pieces (ensemble_layout).  Against the stepwise driver, which re-orders the states and
    lets every step split them again: predictions identical, log-probs within the 1e-5 (+ one fp32 ulp of the sum) of
    test_top1_sampling_equals_beam1_search (observed on one MI355X: the same bits).  The exact-fp32 numerics (gemm_mode 2) have no
    step of 512 rows or more with shared parents - their products take no row lists -, for one model as for several; full width
    in that mode, M = 2, is the one call of test_against_the_cpu_oracle."""
    c = ORACLE_CASES[True]
    cfg, _, decs, _keep = toy_members(seeds=c["members"], sharp=c["sharp"], full=True)
    nimg, ns, steps = 8, 22, 4
    feats, sent_b, eps0, eps = search_inputs(cfg, nimg, ns, c["R_"], seed=3, steps=steps)
    end = cfg.boundary_index
    weights = [0.6, 0.4]
    ens = EnsembleDecodeEngine(decs, weights)
    ctx = ens.prepare(feats)
    assert decs[0].ungathered_ok(ctx.ctxs[0], nimg * ns * K, K)
    got, got_lp = ens.search(ctx, sent_b, ns, K, N, steps, end, eps0, eps, skip_dead=True, early_stop=False)
    ctx2 = ens.prepare(feats)
    want, want_lp, _, _ = stepwise_ensemble(decs, ctx2.ctxs, weights, "prob", sent_b, nimg * ns, K, N, steps, end, eps0, eps,
                                            skip_dead=True)
    diff = (got_lp.cpu() - want_lp).abs()
    print(f"full width one call: max |dlp| {float(diff.max()):.3g}, "
          f"{int((got.cpu() != want).any(-1).sum())} of {got.numel() // steps} captions differ")
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert bool((diff <= 1e-5 + 1.2e-7 * want_lp.abs()).all())


def oracle_margins():
    """The oracle side alone (CPU): how many entries of every ORACLE_CASES case have a sub-margin step, and the smallest margin."""
    for full, c in ORACLE_CASES.items():
        cfg = model_cfg(full)
        plist = []
        for s in c["members"]:
            p = oracle.init_params(cfg, seed=s)
            p["_output_layer.weight"] *= c["sharp"]
            plist.append(p)
        rec = oracle_record(cfg, plist, [0.6, 0.4], c)
        m = np.stack(rec["margin"])   # (steps, B, 1)
        print(f"full={full}: {int((m.min(0) <= MARGIN).sum())} of {m.shape[1]} entries cut short, smallest margin {m.min():.3g}")


def model_cfg(full):
    """The configuration of test_sampling_gpu.model(full), without an engine (for the CPU-only oracle_margins)."""
    if full:
        return oracle.OracleConfig(vocab_size=10000, image_feature_size=2048, embedding_size=1000, hidden_size=1200,
                                   attention_projection_size=768, z_space=128, max_caption_length=20, sentiment_vae=1,
                                   senti_prior_multip=0.5, beam_size=1)
    return oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32, attention_projection_size=16,
                               z_space=8, max_caption_length=9, sentiment_vae=1, senti_prior_multip=0.5, beam_size=1)


# ---- the public interface --------------------------------------------------------------------------------------------------------

MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.vocab import Vocabulary
from var_updown.models import CaptionerEnsemble, UpDownCaptioner
members = []
for seed in (1, 2, 3):
    torch.manual_seed(seed)
    members.append(UpDownCaptioner(Vocabulary.synthetic(120), 64, 40, 48, 32, max_caption_length=8, beam_size=3, z_space=16,
                                   sentiment_vae=1, senti_prior_multip=0.5, device=torch.device("cuda")).cuda())
ens = CaptionerEnsemble(members, weights=[3, 2, 1], mode={mode!r})
assert not ens.training
g = torch.Generator().manual_seed(0)
feats = torch.randn(6, 5, 64, generator=g).cuda()
senti = torch.randint(-1, 2, (6, 1), generator=g).float().cuda()
torch.manual_seed(11)
out = ens(feats, sentiment=senti)["predictions"]
torch.manual_seed(11)
lead = members[0]
eps0 = lead._draw_eps(1, 6, feats.device)[0]
eps = lead._draw_eps(7, 6 * 3, feats.device)
eng = ens.engine()
beams, lps = eng.search(eng.prepare(feats), senti.reshape(6), 1, 3, 1, 8, lead._boundary_index, eps0, eps)
single = members[0](feats, sentiment=senti)["predictions"]
try:
    ens.train()
    raised = False
except RuntimeError:
    raised = True
print(json.dumps({{"forward": out.cpu().tolist(), "search": beams[:, 0, 0, :].cpu().tolist(), "train_raises": raised,
                  "shape_like_single": out.dim() == single.dim() and out.size(0) == single.size(0)}}))
"""


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_captioner_ensemble_forward(mode):
    """CaptionerEnsemble's eval forward (in a child process): the captions of EnsembleDecodeEngine.search on the same inputs and
    noise, in the shape of UpDownCaptioner's eval forward; training mode raises."""
    src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"), mode=mode)
    got = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    assert got["forward"] == got["search"] and len(got["forward"]) == 6 and all(0 < len(c) <= 8 for c in got["forward"])
    assert got["train_raises"] and got["shape_like_single"]


def test_inference_script_with_an_ensemble(tmp_path):
    """scripts/inference.py --synthetic 4 --ensemble-checkpoints: predictions are written; the same checkpoint given twice writes
    the single-checkpoint predictions (the mean of two equal distributions is that distribution up to its last bits; the
    checkpoints' output layers are scaled by 8 so that no selection hangs on those)."""
    from ssc_runtime.config import Config
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
                   "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
                   "  BEAM_SIZE: 3\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
                   "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 3\n")
    conf = Config(str(cfg), [])
    cks = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        m = UpDownCaptioner.from_config(conf, vocabulary=Vocabulary.synthetic(150), device=torch.device("cpu"))
        with torch.no_grad():
            m._output_layer.weight *= 8.0
        cks.append(str(tmp_path / f"ck{seed}.pt"))
        torch.save({"model": m.state_dict()}, cks[-1])

    def run(name, extra):
        out = tmp_path / name
        run_child([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4",
                   "--vocab-size", "150", "--num-boxes", "5", "--output-path", str(out), "--checkpoint-path", cks[0]] + extra)
        return json.load(open(out))

    single = run("single.json", [])
    twice = run("twice.json", ["--ensemble-checkpoints", cks[0]])
    both = run("both.json", ["--ensemble-checkpoints", cks[1], "--ensemble-weights", "2", "1", "--ensemble-mode", "logprob"])
    assert len(single) == 4 * 3 and twice == single
    assert len(both) == 4 * 3 and all(isinstance(c["caption"], str) for c in both)
    assert [c["image_id"] for c in both] == [c["image_id"] for c in single]
