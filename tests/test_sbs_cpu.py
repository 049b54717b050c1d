"""CPU: the stochastic beam search's sampler, config key and argument checks, and the float64 restatement the GPU tests compare
against - checked against the reference's own GumbelSampler + BeamSearch (tests/golden/g18_stochastic_beam.npz)."""
import ctypes as C

import numpy as np
import pytest

import sbsref as R
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config


def test_gumbel_sampler_and_desc():
    for t in (0.0, -1.0):
        with pytest.raises(ValueError):
            sampling.GumbelSampler(temperature=t)
    s = sampling.GumbelSampler(0.7)
    assert s.beam_search and not sampling.MultinomialSampler().beam_search
    d = s.desc(-1)
    assert isinstance(d, L.GumbelDesc) and d.seed == 2 ** 64 - 1 and abs(d.temperature - 0.7) < 1e-7
    assert C.sizeof(L.GumbelDesc) == 16 and L.GumbelDesc.seed.offset == 8


def test_config_key():
    assert Config().MODEL.STOCHASTIC_BEAM_SEARCH is False
    s = sampling.from_config(Config(config_override=["MODEL.STOCHASTIC_BEAM_SEARCH", "True", "MODEL.SAMPLER_TEMPERATURE",
                                                     "1.6"]).MODEL)
    assert isinstance(s, sampling.GumbelSampler) and s.temperature == 1.6
    with pytest.raises(ValueError, match="STOCHASTIC_BEAM_SEARCH"):
        sampling.from_config(Config(config_override=["MODEL.STOCHASTIC_BEAM_SEARCH", "True", "MODEL.DECODE_SAMPLER",
                                                     "top-k", "MODEL.SAMPLER_TOP_K", "5"]).MODEL)
    with pytest.raises(ValueError, match="DECODE_SAMPLER"):
        sampling.from_config(Config(config_override=["MODEL.DECODE_SAMPLER", "gumbel"]).MODEL)


def _beam_desc(B, k, n, V):
    d = L.BeamDesc()
    d.scores, d.ld, d.raw_logits = C.c_void_p(256), V, 1
    d.dims = L.FsmDims(0, 1, V, 0, 1)
    d.B, d.beam, d.per_node, d.end_index = B, k, n, 1
    d.last_pred, d.last_lp, d.pred, d.lp_out, d.backptr = [C.c_void_p(256)] * 5
    d.scratch_val, d.scratch_idx = C.c_void_p(256), C.c_void_p(256)
    d.step_index = 1
    return d


def test_gumbel_calls_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    g = sampling.GumbelSampler().desc(1)
    buf = C.c_void_p(256)
    for B, k, n, V in ((2, 3, 4, 50),      # n > k
                       (2, 3, 2, 2),       # k > V (and n <= V)
                       (2, 33, 2, 100),    # past the 32-beam limit
                       (2, 3, 0, 50)):
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_beam_step_gumbel(C.byref(_beam_desc(B, k, n, V)), C.byref(g), buf, buf, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):   # n > V
        lib.ssc_beam_step_gumbel(C.byref(_beam_desc(2, 3, 3, 2)), C.byref(g), buf, buf, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):   # k > V at step 0
        lib.ssc_beam_first_gumbel(C.byref(_beam_desc(2, 8, 1, 5)), C.byref(g), buf, None)
    bad = L.GumbelDesc(0.0, 1)                            # temperature 0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_beam_step_gumbel(C.byref(_beam_desc(2, 3, 2, 50)), C.byref(bad), buf, buf, None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    sd = L.SearchDesc()
    sd.nimg, sd.R, sd.n_samples, sd.S, sd.beam, sd.per_node, sd.max_steps, sd.end_index = 2, 3, 4, 1, 3, 1, 5, 1
    assert lib.ssc_decode_stochastic_beam_workspace_bytes(C.byref(cfg), C.byref(sd)) > 0
    for beam, per_node, T in ((3, 1, 0.0), (3, 4, 1.0), (11, 1, 1.0)):   # T 0; per_node > beam; beam > V (10)
        sd.beam, sd.per_node = beam, per_node
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_decode_stochastic_beam(C.byref(cfg), C.byref(L.Params()), C.byref(sd), C.byref(L.GumbelDesc(T, 1)),
                                           C.c_void_p(256), 1 << 30, None)


def _check_step(what, rec, t, tok, lp, G, bp=None, tol_lp=1e-6, tol_g=1e-5):
    ok = rec["gap"][t] > 1e-5   # entries whose every decision at this step has a margin above 1e-5
    assert ok.any() or not len(ok), what
    np.testing.assert_array_equal(tok[ok], rec["tok"][t][ok], err_msg=what)
    if bp is not None:
        np.testing.assert_array_equal(bp[ok], rec["bp"][t][ok], err_msg=what)
    np.testing.assert_allclose(lp[ok], rec["lp_t"][t][ok], atol=tol_lp, rtol=tol_lp, err_msg=what)
    np.testing.assert_allclose(G[ok], rec["G"][t][ok], rtol=tol_g, atol=tol_g, err_msg=what)
    return int(ok.sum())


def test_restatement_reproduces_the_reference():
    fx, cases = R.load_fixture()
    checked = 0
    for c in cases:
        rec = fx[c["name"]]
        B, k, n = c["B"], c["k"], c["n"]
        for t, rows in R.replay(c, rec):   # teacher-forced on the reference's own selections
            if t == 0:
                tok, lp, G = R.first_step(rows, k, R.SEED)
                checked += _check_step((c["name"], t), rec, t, tok, lp, G)
            else:
                tok, lp, G, bp = R.next_step(rows, rec["tok"][t - 1], rec["lp_t"][t - 1].astype(np.float64),
                                             rec["G"][t - 1].astype(np.float64), B, k, n, c["T"], R.SEED, t)
                checked += _check_step((c["name"], t), rec, t, tok, lp, G, bp)
        # the reference's final output is the last step's, back-traced
        steps = rec["tok"].shape[0]
        assert rec["pred"].shape == (B, k, steps)
        np.testing.assert_array_equal(rec["pred"][:, :, -1], rec["tok"][-1])
        np.testing.assert_allclose(rec["lp"], rec["lp_t"][-1])
    assert checked > 0.9 * sum(fx[c["name"]]["gap"].size for c in cases)
    # the fixture covers what it is meant to: beams that end at different steps, and a search that ends at step 0 at k = 1
    ends = fx["ends"]["pred"]
    first_end = np.where((ends == R.END).any(-1), (ends == R.END).argmax(-1), ends.shape[-1])
    assert len(np.unique(first_end)) > 1
    assert fx["allend0"]["pred"].shape == (2, 1, 1) and (fx["allend0"]["pred"] == R.END).all()
    # k captions per entry are distinct
    for c in cases:
        p = fx[c["name"]]["pred"]
        for b in range(c["B"]):
            assert len({tuple(x) for x in p[b]}) == c["k"], c["name"]


def test_top_n_by_g_is_top_n_by_transform():
    rng = np.random.default_rng(3)
    for V, n, Tp in ((50, 5, 0.0), (10000, 2, -3.5), (10000, 32, -40.0)):
        lp = rng.standard_normal((8, V)) * 3
        phi = lp - np.log(np.exp(lp).sum(1, keepdims=True)) + rng.uniform(-20, 0, (8, 1))
        g = R.perturbed(phi, R.uniforms(V, 77, 1, np.arange(8)))
        G = R.transform(g, np.full(8, Tp))
        by_g, by_G = R.top_by(g, n), R.top_by(G, n + 1)
        for r in range(8):
            Gs = np.take_along_axis(G[r], by_G[r], 0)
            if (np.diff(Gs) < 0).all():   # wherever the transformed values differ, the orders agree
                np.testing.assert_array_equal(by_g[r], by_G[r][:n])
        assert (np.take_along_axis(G, by_g[:, :1], 1)[:, 0] == Tp).all()   # the maximum maps to the target exactly
