"""CPU: the word samplers' argument checks and config keys, and the NumPy restatements the GPU sampling tests compare against
(filters vs the reference's own distributions in tests/golden/g17_samplers.npz, Philox4x32-10 vs its published known answers)."""
import ctypes as C

import numpy as np
import pytest

import samplerref as S
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config
from test_attention_trace_cpu import model_cfg, sample_opts, search_desc


def test_sampler_argument_checks():
    with pytest.raises(ValueError):
        sampling.TopPSampler(p=-0.1)
    with pytest.raises(ValueError):
        sampling.TopPSampler(p=1.01)
    with pytest.raises(ValueError):
        sampling.TopKSampler(k=0)
    with pytest.raises(ValueError):
        sampling.TopKSampler(k=20).check_vocab(10)
    sampling.TopKSampler(k=10).check_vocab(10)
    for cls in (sampling.MultinomialSampler, sampling.TopKSampler, sampling.TopPSampler):
        with pytest.raises(ValueError):
            cls(temperature=-1.0)
    with pytest.raises(ValueError):
        sampling.MultinomialSampler(temperature=0.0)
    # temperature `or 1.0` for top-k / top-p (beam_search.py:173,233)
    assert sampling.TopKSampler(k=3, temperature=0).temperature == 1.0
    assert sampling.TopPSampler(p=0.5, temperature=0).temperature == 1.0
    s = sampling.TopPSampler(p=0.25, temperature=0.5, with_replacement=True)
    d = s.desc(2 ** 63 + 5)
    assert (d.kind, d.top_p, d.temperature, d.seed) == (2, 0.25, 0.5, 2 ** 63 + 5)
    d = sampling.TopKSampler(k=7, temperature=1.3).desc(3)
    assert (d.kind, d.top_k) == (1, 7) and abs(d.temperature - 1.3) < 1e-6
    assert sampling.MultinomialSampler().desc(0).kind == 0
    assert C.sizeof(L.SamplerDesc) == 24


def test_config_keys_and_defaults():
    c = Config()
    m = c.MODEL
    assert (m.DECODE_SAMPLER, m.SAMPLER_TOP_K, m.SAMPLER_TOP_P, m.SAMPLER_TEMPERATURE) == ("beam", 0, 1.0, 1.0)
    assert sampling.from_config(m) is None
    c = Config(config_override=["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", "0.9", "MODEL.SAMPLER_TEMPERATURE", "0.7"])
    s = sampling.from_config(c.MODEL)
    assert isinstance(s, sampling.TopPSampler) and s.p == 0.9 and s.temperature == 0.7
    c = Config(config_override=["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", "5"])
    s = sampling.from_config(c.MODEL)
    assert isinstance(s, sampling.TopKSampler) and s.k == 5
    assert isinstance(sampling.from_config(Config(config_override=["MODEL.DECODE_SAMPLER", "multinomial"]).MODEL),
                      sampling.MultinomialSampler)
    with pytest.raises(ValueError, match="DECODE_SAMPLER"):
        sampling.from_config(Config(config_override=["MODEL.DECODE_SAMPLER", "gumbel"]).MODEL)


def test_sample_calls_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    d = sampling.TopKSampler(k=5).desc(1)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):   # k > V
        lib.ssc_sample_rows(C.c_void_p(16), 4, 1, 4, C.byref(d), None, 0, None, None, 1, C.c_void_p(16), C.c_void_p(16), None, None)
    bad = L.SamplerDesc(0, 0, 1.0, 0.0, 1)                 # temperature 0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_sample_rows(C.c_void_p(16), 8, 1, 8, C.byref(bad), None, 0, None, None, 1, C.c_void_p(16), C.c_void_p(16), None, None)
    bad = L.SamplerDesc(2, 0, 1.5, 1.0, 1)                 # p > 1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_sample_rows(C.c_void_p(16), 8, 1, 8, C.byref(bad), None, 0, None, None, 1, C.c_void_p(16), C.c_void_p(16), None, None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    sd = L.SearchDesc()
    sd.nimg, sd.R, sd.n_samples, sd.S, sd.beam, sd.per_node, sd.max_steps, sd.end_index = 2, 3, 4, 1, 1, 1, 5, 1
    assert lib.ssc_decode_sample_workspace_bytes(C.byref(cfg), C.byref(sd)) > 0
    sd.beam = 2   # word sampling is beam 1 only
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_decode_sample(C.byref(cfg), C.byref(L.Params()), C.byref(sd), C.byref(sampling.MultinomialSampler().desc(1)),
                              C.c_void_p(16), 1 << 30, None)


def test_sample_opts_bytes_rule_without_a_gpu():
    """ssc_sample_opts.bytes (include/ssc.h): a size below sizeof(size_t), no multiple of the pointer size or above the library's own
    is SSC_EINVAL (-1) whatever else the call holds; a field is read only if it lies wholly inside `bytes` - a bad contrast is refused
    inside the size and not read behind it, where the call then wants the plain call's workspace (one byte short: SSC_EWORKSPACE, -4).
    ssc_decode_sample_opts_workspace_bytes is the plain call's without an amateur and grows by the amateur's blocks with one."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)   # (never read: every check comes before the launch)
    cfg, d, p, smp = model_cfg(), search_desc(a, beam=1, per_node=1), L.Params(), L.SamplerDesc(0, 0, 1.0, 1.0, 3)
    c_, dd = C.byref(cfg), C.byref(d)
    size = lambda o: lib.ssc_decode_sample_opts_workspace_bytes(c_, dd, C.byref(o) if o is not None else None)
    call = lambda o, n: lib._raw_ssc_decode_sample_opts(c_, C.byref(p), dd, C.byref(smp), C.byref(o) if o is not None else None, a, n, None)
    full, word = C.sizeof(L.SampleOpts), C.sizeof(C.c_size_t)
    assert full == 5 * C.sizeof(C.c_void_p) and L.SampleOpts.contrast.offset == full - C.sizeof(C.c_void_p)
    n0 = lib.ssc_decode_sample_workspace_bytes(c_, dd)
    assert n0 > 0 and size(None) == size(sample_opts()) == size(sample_opts(nbytes=word)) == n0
    assert call(None, n0 - 1) == call(sample_opts(), n0 - 1) == call(sample_opts(nbytes=word), n0 - 1) == -4
    for nbytes in (0, 4, 12, full + 8):
        assert call(sample_opts(nbytes=nbytes), n0) == -1 and call(sample_opts(nbytes=nbytes), n0 - 1) == -1, nbytes
        assert size(sample_opts(nbytes=nbytes)) == 0, nbytes
    bad = L.Contrast()
    bad.alpha, bad.beta = -1.0, 0.1
    assert call(sample_opts(contrast=bad), n0) == -1 and call(sample_opts(contrast=bad), n0 - 1) == -1
    cut = sample_opts(contrast=bad, nbytes=L.SampleOpts.contrast.offset)
    assert call(cut, n0 - 1) == -4 and size(cut) == n0
    # an amateur that is stepped: the number the contrast's own workspace function gave before this entry replaced it, read off the
    # commit before for this shape - V 50, H 8, R 5, B = 2 x 3, 6 steps
    good = L.Contrast()
    good.alpha, good.beta = 1.0, 0.1
    assert n0 == 67115776 and size(sample_opts(contrast=good)) == 134230016
    assert size(sample_opts(contrast=good, nbytes=L.SampleOpts.contrast.offset)) == n0


def test_filter_restatement_matches_the_reference_distributions():
    d, cfg = S.load_fixture()
    n = 0
    for V in cfg["vs"]:
        lp = d[f"lp_V{V}"]
        for si, (kind, k, p, T) in enumerate(cfg["settings"]):
            key = f"dist_V{V}_s{si}"
            if key not in d:
                assert kind == "top-k" and k > V
                continue
            for r in range(lp.shape[0]):
                probs, ahead = S.filter_dist(lp[r], kind, k, p, T)
                S.check_against_reference(probs, d[key][r], ahead, kind, p, (V, kind, k, p, T, r))
                n += 1
    assert n == 3 * (3 * 17 - 2)
    # the fixture covers the cases it is meant to: exact ties cut by top-k 5, p = 0 keeps one token
    lp = d["lp_V50"][2]
    assert (lp == lp.max()).sum() == 3
    si = cfg["settings"].index(("top-p", 0, 0.0, 0.7))
    assert ((d[f"dist_V10000_s{si}"] > 0).sum(-1) == 1).all()


def test_philox_known_answers():
    # Random123 known-answer vectors of philox4x32_10
    cases = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in cases:
        assert tuple(int(x) for x in S.philox4x32_10(np.array(ctr, dtype=np.uint32), key)) == want


def test_gumbel_noise_is_open_interval_and_gumbel_distributed():
    g = S.gumbel(400003, seed=0x1234_5678_9ABC_DEF0, step=3, b=17)
    assert np.isfinite(g).all() and g.dtype == np.float32
    # Gumbel(0, 1): mean = Euler-Mascheroni constant, variance = pi^2 / 6
    assert abs(g.mean() - 0.5772157) < 0.01 and abs(g.var() - np.pi ** 2 / 6) < 0.03
    # the counter words: other steps / rows / seeds give other noise, the same ones the same
    assert np.array_equal(g, S.gumbel(400003, 0x1234_5678_9ABC_DEF0, 3, 17))
    assert not np.array_equal(g[:100], S.gumbel(100, 0x1234_5678_9ABC_DEF0, 4, 17))
    assert not np.array_equal(g[:100], S.gumbel(100, 0x1234_5678_9ABC_DEF0, 3, 18))
    assert not np.array_equal(g[:100], S.gumbel(100, 0x1234_5678_9ABC_DEF1, 3, 17))


def test_gumbel_max_draw_follows_the_filtered_distribution():
    rng = np.random.default_rng(5)
    logits = rng.normal(size=12).astype(np.float32) * 1.5
    probs, _ = S.filter_dist(logits - np.log(np.exp(logits.astype(np.float64)).sum()), "top-p", p=0.8, T=0.9)
    counts = np.zeros(12)
    for b in range(20000):
        counts[S.draw(logits, probs > 0, 0.9, 99, 0, b)[0]] += 1
    assert counts[probs == 0].sum() == 0
    exp = probs[probs > 0] * 20000
    chi2 = (((counts[probs > 0] - exp) ** 2) / exp).sum()
    assert chi2 < 40, chi2   # (df <= 11: p ~ 1e-5)
