"""CPU: Mirostat 2.0 for the word samplers (include/ssc.h: ssc_mirostat) - the restatement (tests/mirostatref.py) against a
brute-force loop on hand-made rows, the control loop on synthetic Zipf rows, the unit conversion, the class, the config keys and
their refusals, the struct and the bindings against the header, every refusal of the four new symbols (no launch is reached: no GPU
needed), the workspace size, the runtime's refusals and those of scripts/inference.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mirostatref as R
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config
from ssc_runtime.decode import DecodeEngine, EnsembleDecodeEngine
from ssc_runtime.engine import ModelDims
from ssc_runtime.inference import diverse_decode
from ssc_runtime.vocab import Vocabulary
from test_attention_trace_cpu import CFG, header, model_cfg, sample_opts, search_desc, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1
INF = float("inf")
LN2 = math.log(2.0)


# ---- the restatement against a brute-force loop ---------------------------------------------------------------------------------------
def brute_force(x, mu, T):
    """The definition of include/ssc.h word for word, with Python lists and math.* in place of array operations."""
    V = len(x)
    fin = [v for v in range(V) if math.isfinite(x[v])]
    if not fin:
        return set(), {}
    mx = max(float(x[v]) for v in fin)
    Z = math.fsum(math.exp((float(x[v]) - mx) / T) for v in fin)
    sur = {v: math.log(Z) - (float(x[v]) - mx) / T for v in fin}
    first = min(v for v in fin if float(x[v]) == mx)
    return {v for v in fin if sur[v] <= mu} | {first}, sur


def kept_ids(c):
    return [int(v) for v in np.nonzero(c.kept)[0]]


def test_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(7)
    checked = 0
    for V in (5, 37, 200):
        for T in (0.7, 1.0, 1.3):
            x = (rng.standard_normal(V) * 3).astype(np.float32)
            x[rng.integers(0, V, 2)] = -INF
            _, sur = brute_force(x, 0.0, T)
            for mu in (min(sur.values()) - 0.5, float(np.median(list(sur.values()))) + 1e-3, max(sur.values()) + 0.5):
                c = R.cut_row(x, mu, T)
                kept, _ = brute_force(x, mu, T)
                assert c.undecidable == [], (V, T, mu)
                assert set(kept_ids(c)) == kept
                checked += 1
    assert checked == 27


def test_hand_made_rows():
    # a flat row of V = 37: every surprise is log 37 - all or only token 0
    flat = np.zeros(37, dtype=np.float32)
    assert kept_ids(R.cut_row(flat, math.log(37) + 0.1)) == list(range(37))
    assert kept_ids(R.cut_row(flat, math.log(37) - 0.1)) == [0]
    assert R.cut_row(flat, math.log(37) - 0.1).undecidable == [] and R.cut_row(flat, math.log(37)).undecidable == list(range(1, 37))
    for T in (0.7, 1.3):   # (a flat row is flat at any temperature)
        assert kept_ids(R.cut_row(flat + 3, math.log(37) + 0.1, T)) == list(range(37))
    # a peaked row: q = (0.9, 0.05, 0.03, 0.02): surprises 0.105, 3.0, 3.5, 3.9 nats
    peaked = np.log(np.array([0.9, 0.05, 0.03, 0.02])).astype(np.float32)
    assert kept_ids(R.cut_row(peaked, 0.01)) == [0]                  # mu below every surprise: the top word stays
    assert kept_ids(R.cut_row(peaked, 3.2)) == [0, 1]
    assert kept_ids(R.cut_row(peaked, 3.6)) == [0, 1, 2]
    assert kept_ids(R.cut_row(peaked, 10.0)) == [0, 1, 2, 3]
    assert kept_ids(R.cut_row(peaked, -5.0)) == [0]                  # a negative mu as well
    assert kept_ids(R.cut_row(peaked[::-1].copy(), 0.01)) == [3]
    # the maximum three times: below its surprise only the lowest index stays, above it all three
    tri = np.array([1.0, 4.0, 0.0, 4.0, 4.0, -2.0], dtype=np.float32)
    top = -R.cut_row(tri, 0.0).logq[1]
    assert kept_ids(R.cut_row(tri, top - 0.05)) == [1] and kept_ids(R.cut_row(tri, top + 0.05)) == [1, 3, 4]
    assert R.cut_row(tri, top + 1e-6).undecidable == [3, 4]          # (first itself is never undecidable)
    # -inf entries stay dropped and weigh nothing
    banned = np.array([-INF, 2.0, -INF, 2.0 + math.log(3.0)], dtype=np.float32)
    c = R.cut_row(banned, 100.0)
    assert kept_ids(c) == [1, 3] and math.exp(c.logq[3]) == pytest.approx(0.75) and c.first == 3
    assert kept_ids(R.cut_row(banned, 1.0)) == [3]
    none = R.cut_row(np.full(4, -INF, dtype=np.float32), 3.0)
    assert kept_ids(none) == [] and not none.live
    # an ended row, a row without a finite entry and the pad column come back as they were
    x = np.array([[0.0, 5.0, 0.0, 9.0], [np.nan, np.nan, np.nan, 7.0], [-INF, -INF, -INF, 1.0]], dtype=np.float32)
    out, kept, norm, und = R.cut_rows(x, 3, [0.5, 0.5, 0.5], 1.0, last_pred=[0, END, 0], end=END)
    assert out[0].tolist() == [-INF, 5.0, -INF, 9.0] and kept.tolist() == [1, 0, 0] and und == []
    assert np.isnan(out[1, :3]).all() and out[2].tolist() == [-INF, -INF, -INF, 1.0]
    assert norm[0, 0] == 5.0 and np.isnan(norm[:, 1:]).all()
    # the update: the surprise under the distribution BEFORE the cut; pass-through rows keep mu
    mu2, sur = R.update_rows(np.stack([peaked, peaked, peaked, peaked]), 4, 1.0, 1.0, 0.5, [1, 7, 2, 0], [3.2] * 4, last_pred=[0, 0, END, 0],
                             end=END)
    assert sur[0] == pytest.approx(-math.log(0.05), abs=1e-6) and mu2[0] == pytest.approx(3.2 - 0.5 * (-math.log(0.05) - 1.0), abs=1e-6)
    assert (sur[1], mu2[1], sur[2], mu2[2]) == (0.0, 3.2, 0.0, 3.2)
    assert mu2[3] > 3.2                                              # an unsurprising word raises mu
    edited = R.cut_rows(np.stack([peaked]), 4, [3.2], 1.0)[0]
    assert R.update_rows(edited, 4, 1.0, 1.0, 0.5, [3], [3.2])[1][0] == 0.0   # a dropped word: the row passes through


# ---- the control loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau_bits", [2.0, 4.0])
def test_control_loop_holds_the_surprise_closer_to_tau_than_plain_sampling(tau_bits):
    """Synthetic Zipf rows whose exponent changes from step to step (a fixed knob fits none of them): the mean observed surprise of
    steps 50 onward is closer to tau under the control than the uncontrolled multinomial sampler's on the same rows with the same
    uniform draws.  A comparison, not a threshold."""
    V, steps, eta = 1000, 200, 0.1
    rng = np.random.default_rng(2021)
    expo = rng.uniform(1.05, 1.6, steps)
    perm = [rng.permutation(V) for _ in range(steps)]
    u = rng.random(steps)
    rows = lambda t: (-expo[t] * np.log(np.arange(1, V + 1)))[perm[t]].astype(np.float32)
    draw = lambda t, q: min(int(np.searchsorted(np.cumsum(q), u[t] * q.sum(), side="right")), V - 1)
    tau = tau_bits * LN2
    _, mu, sur, kept = R.control_loop(rows, steps, tau, eta, 2 * tau, 1.0, draw)
    plain = np.zeros(steps)
    for t in range(steps):
        c = R.cut_row(rows(t), INF)
        plain[t] = -c.logq[draw(t, np.exp(c.logq))]
    err_on, err_off = abs(sur[50:].mean() - tau), abs(plain[50:].mean() - tau)
    assert err_on < err_off, (err_on / LN2, err_off / LN2)
    assert kept.min() >= 1 and (kept < V).any() and np.isfinite(mu).all()
    # every drawn word obeys the cut: its surprise is at most mu_t, or it is the top word
    for t in range(steps):
        assert sur[t] <= mu[t] or sur[t] == -R.cut_row(rows(t), INF).logq.max()


def test_eta_zero_is_a_fixed_surprise_cut():
    rows = lambda t: np.log(np.array([0.5, 0.3, 0.15, 0.05])).astype(np.float32)
    toks, mu, sur, kept = R.control_loop(rows, 10, 1.0, 0.0, 1.5, 1.0, lambda t, q: int(np.argmax(q > 0) if t % 2 else 1))
    assert (mu == 1.5).all() and (kept == 2).all() and set(toks) == {0, 1}


# ---- the class, the units and the config keys ----------------------------------------------------------------------------------------------
def test_mirostat_class_units_and_arguments():
    S = sampling
    m = S.Mirostat()
    assert (m.tau, m.eta, m.mu0, m.unit) == (3.0, 0.1, 6.0, "bits") and m.active
    f32 = lambda v: C.c_float(v).value
    assert m.tau_nats == f32(3.0 * LN2) and m.mu0_nats == f32(6.0 * LN2) and m.scale == LN2
    d = m.desc()
    assert (d.tau, d.mu0) == (f32(3.0 * LN2), f32(6.0 * LN2)) and d.eta == f32(0.1) and not d.mu and not d.surprise and not d.kept
    n = S.Mirostat(2.0, 0.25, mu0=5.0, unit="nats")
    assert (n.tau_nats, n.mu0_nats, n.desc().eta) == (2.0, 5.0, 0.25)
    assert S.Mirostat(4.0).mu0 == 8.0 and S.Mirostat(4.0, mu0=1.0).mu0 == 1.0 and S.Mirostat(1.0, mu0=-2.0).mu0 == -2.0
    assert not S.Mirostat(0.0).active and S.Mirostat(1.0, 0.0).active
    t = torch.tensor([LN2, 2 * LN2])
    assert torch.allclose(m.from_nats(t), torch.tensor([1.0, 2.0])) and n.from_nats(t) is t
    for kw in (dict(tau=-1.0), dict(tau=math.nan), dict(tau=INF), dict(eta=-0.1), dict(eta=math.nan), dict(eta=INF), dict(mu0=math.nan),
               dict(mu0=INF), dict(mu0=-INF), dict(unit="hartleys"), dict(tau="much")):
        with pytest.raises(ValueError, match="Mirostat"):
            S.Mirostat(**kw)


TOPP = ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", 0.95, "MODEL.BEAM_SIZE", 1]


def test_config_keys():
    c = Config()
    assert (c.MODEL.SAMPLER_MIROSTAT_TAU, c.MODEL.SAMPLER_MIROSTAT_ETA) == (0.0, 0.1)
    assert sampling.mirostat_from_config(c.MODEL) is None and sampling.mirostat_from_config(Config(config_override=TOPP).MODEL) is None
    # eta alone selects nothing
    assert sampling.mirostat_from_config(Config(config_override=TOPP + ["MODEL.SAMPLER_MIROSTAT_ETA", 0.5]).MODEL) is None
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_MIROSTAT_TAU", 2.5, "MODEL.SAMPLER_MIROSTAT_ETA", 0.2])
    m = sampling.mirostat_from_config(c.MODEL)
    assert (m.tau, m.eta, m.mu0, m.unit) == (2.5, 0.2, 5.0, "bits")
    assert isinstance(sampling.from_config(c.MODEL), sampling.TopPSampler)
    for other, match in (([], "needs MODEL.DECODE_SAMPLER"), (["MODEL.STOCHASTIC_BEAM_SEARCH", True], "needs MODEL.DECODE_SAMPLER"),
                         (["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLED_BEAM_SEARCH", True], "SAMPLED_BEAM_SEARCH exclude")):
        c = Config(config_override=["MODEL.SAMPLER_MIROSTAT_TAU", 3.0] + other)
        for read in (lambda: sampling.mirostat_from_config(c.MODEL), lambda: sampling.from_config(c.MODEL)):
            with pytest.raises(ValueError, match=match) as e:
                read()
            assert "MODEL.SAMPLER_MIROSTAT_TAU" in str(e.value)
    for override in (["MODEL.SAMPLER_MIROSTAT_TAU", -1.0], ["MODEL.SAMPLER_MIROSTAT_TAU", math.nan], ["MODEL.SAMPLER_MIROSTAT_TAU", INF],
                     ["MODEL.SAMPLER_MIROSTAT_ETA", -0.5], ["MODEL.SAMPLER_MIROSTAT_ETA", math.nan], ["MODEL.SAMPLER_MIROSTAT_ETA", INF]):
        with pytest.raises(ValueError, match=override[0].split(".")[1]):
            Config(config_override=TOPP + override)


def test_a_model_reads_the_keys_with_a_word_sampler_only():
    from var_updown.models import UpDownCaptioner
    small = ["MODEL.IMAGE_FEATURE_SIZE", 8, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
             "MODEL.Z_SPACE", 4]
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_MIROSTAT_TAU", 3.0] + small)
    vocab = Vocabulary.synthetic(40)
    m = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu")     # (no sampler: the keys are not read)
    assert m._mirostat is None
    with pytest.raises(ValueError, match="needs a word sampler"):
        m.mirostat(sampling.Mirostat())
    m.mirostat(None)
    s = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu", sampler=sampling.from_config(c.MODEL))
    assert isinstance(s._mirostat, sampling.Mirostat) and s._mirostat.tau == 3.0
    s.mirostat(sampling.Mirostat(0.0))             # inactive: off
    assert s._mirostat is None
    s.mirostat(sampling.Mirostat(2.0, unit="nats"))
    assert s._mirostat.unit == "nats"
    with pytest.raises(ValueError, match="Mirostat or None"):
        s.mirostat(sampling.TypicalTruncation())


# ---- the struct and the bindings against the header -----------------------------------------------------------------------------------------
NEW = ("ssc_mirostat_rows", "ssc_mirostat_update", "ssc_decode_sample_mirostat_workspace_bytes", "ssc_decode_sample_mirostat")


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
    return [a.strip() for a in m.group(1).split(",")]


def test_bindings_mirror_the_header():
    assert struct_fields("ssc_mirostat") == [f for f, _ in L.Mirostat._fields_] == ["tau", "eta", "mu0", "mu", "surprise", "kept"]
    assert C.sizeof(L.Mirostat) == 40
    cdll = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(cdll, name), name
        args = declaration(name)
        assert len(args) == len(L.SYMBOLS[name][1]), name
        for a, ct in zip(args, L.SYMBOLS[name][1]):   # scalars by type, everything else a pointer
            want = C.c_float if a.startswith("float ") else C.c_int if a.startswith("int ") else C.c_size_t if a.startswith("size_t ") else None
            assert (ct is want) if want is not None else ("*" in a and ct not in (C.c_float, C.c_int, C.c_size_t)), (name, a)
    # ssc_decode_sample_opts with one argument more, behind the opts
    plain, miro = L.SYMBOLS["ssc_decode_sample_opts"][1], L.SYMBOLS["ssc_decode_sample_mirostat"][1]
    assert miro[:5] == plain[:5] and miro[5] is C.POINTER(L.Mirostat) and miro[6:] == plain[5:]
    plain, miro = L.SYMBOLS["ssc_decode_sample_opts_workspace_bytes"][1], L.SYMBOLS["ssc_decode_sample_mirostat_workspace_bytes"][1]
    assert miro == plain + [C.POINTER(L.Mirostat)]
    # the descriptor travels BESIDE the opts: the struct and the version are what they were
    assert struct_fields("ssc_sample_opts") == [f for f, _ in L.SampleOpts._fields_] and C.sizeof(L.SampleOpts) == 5 * C.sizeof(C.c_void_p)
    assert L.load().ssc_version() == 4
    assert "mirostat.hip" in open(os.path.join(ROOT, "style-seqcvae_amd", "build.py")).read()


# ---- refusals, without a GPU ------------------------------------------------------------------------------------------------------------------
def test_rows_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    V = 50

    def call(logits=a, ld=V, rows=3, V=V, T=1.0, mu=a, last=a, end=END, kept=a, norm=a):
        return lib._raw_ssc_mirostat_rows(logits, ld, rows, V, T, mu, last, end, kept, norm, None)

    assert call(rows=0) == 0 and call(rows=0, last=None, end=-7, kept=None) == 0          # nothing to edit
    for kw in (dict(logits=None), dict(mu=None), dict(norm=None), dict(ld=49), dict(rows=-1), dict(V=0), dict(end=-1), dict(end=50),
               dict(T=0.0), dict(T=-1.0), dict(T=INF), dict(T=math.nan)):
        assert call(**kw) == -1, kw
        if "rows" not in kw:
            assert call(rows=0, **kw) == -1, kw     # (refused with nothing to edit as well)
    for kw in (dict(logits=a + 2), dict(mu=a + 1), dict(last=a + 2), dict(kept=a + 3), dict(norm=a + 2)):
        assert call(**kw) == -2, kw
    assert call(logits=a + 2, T=0.0) == -1      # SSC_EINVAL comes first


def test_update_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    V = 50

    def call(logits=a, ld=V, rows=3, V=V, T=1.0, tau=2.0, eta=0.1, norm=a, pred=a, last=a, end=END, mu_in=a, mu_out=a, sur=a):
        return lib._raw_ssc_mirostat_update(logits, ld, rows, V, T, tau, eta, norm, pred, last, end, mu_in, mu_out, sur, None)

    assert call(rows=0) == 0 and call(rows=0, last=None, end=-7, sur=None) == 0 and call(rows=0, tau=0.0, eta=0.0) == 0
    for kw in (dict(logits=None), dict(norm=None), dict(pred=None), dict(mu_in=None), dict(mu_out=None), dict(ld=49), dict(rows=-1),
               dict(V=0), dict(end=-1), dict(end=50), dict(T=0.0), dict(T=-1.0), dict(T=INF), dict(T=math.nan), dict(tau=-1.0),
               dict(tau=math.nan), dict(tau=INF), dict(eta=-0.1), dict(eta=math.nan), dict(eta=INF)):
        assert call(**kw) == -1, kw
    for kw in (dict(logits=a + 2), dict(norm=a + 1), dict(pred=a + 2), dict(last=a + 2), dict(mu_in=a + 3), dict(mu_out=a + 2),
               dict(sur=a + 1)):
        assert call(**kw) == -2, kw
    assert call(pred=a + 2, eta=-1.0) == -1     # SSC_EINVAL comes first


def miro(tau=2.0, eta=0.1, mu0=4.0, mu=None, surprise=None, kept=None):
    return L.Mirostat(tau, eta, mu0, mu, surprise, kept)


def test_decode_refuses_a_bad_mirostat_before_any_launch_and_sizes_its_workspace():
    """A descriptor that passes every check with a workspace one byte short: SSC_EWORKSPACE (-4) - it was accepted, nothing was
    launched; SSC_EINVAL / SSC_EALIGN for every bad one whatever the workspace.  Off (NULL or tau 0) the workspace is that of
    ssc_decode_sample_opts; on it is larger by 2 B floats rounded up to 256 bytes."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    d = search_desc(a, beam=1, per_node=1)
    c, dd = C.byref(cfg), C.byref(d)
    B = d.nimg * d.n_samples
    grow = (2 * B * 4 + 255) // 256 * 256
    trunc = L.Truncation(2, 0.1, None, None)
    contrast = L.Contrast()
    contrast.alpha, contrast.beta = 1.0, 0.1
    for o in (None, sample_opts(), sample_opts(trunc=trunc), sample_opts(contrast=contrast)):
        ob = C.byref(o) if o is not None else None
        n0 = lib.ssc_decode_sample_opts_workspace_bytes(c, dd, ob)
        assert n0 > 0 and n0 % 256 == 0
        assert lib.ssc_decode_sample_mirostat_workspace_bytes(c, dd, ob, None) == n0
        assert lib.ssc_decode_sample_mirostat_workspace_bytes(c, dd, ob, C.byref(miro(0.0))) == n0
        assert lib.ssc_decode_sample_mirostat_workspace_bytes(c, dd, ob, C.byref(miro(mu=a))) == n0 + grow
    bad_opts = sample_opts(nbytes=3)
    assert lib.ssc_decode_sample_mirostat_workspace_bytes(c, dd, C.byref(bad_opts), C.byref(miro(mu=a))) == 0
    n0 = lib.ssc_decode_sample_workspace_bytes(c, dd)
    n = n0 + grow
    p = L.Params()

    def call(m, nbytes, smp=None, opts=None):
        smp = smp or L.SamplerDesc(0, 0, 1.0, 1.0, 3)
        return lib._raw_ssc_decode_sample_mirostat(c, C.byref(p), dd, C.byref(smp), C.byref(opts) if opts is not None else None,
                                                   C.byref(m) if m is not None else None, a, nbytes, None)

    # off: the plain call's workspace is enough (one byte less is not); on: it takes the larger one
    assert call(None, n0 - 1) == -4 and call(miro(0.0), n0 - 1) == -4 and call(miro(0.0, math.nan, math.nan), n0 - 1) == -4
    assert call(miro(mu=a), n - 1) == -4 and call(miro(mu=a, surprise=a, kept=a), n - 1) == -4
    assert call(miro(eta=0.0, mu=a), n - 1) == -4 and call(miro(mu0=-3.0, mu=a), n - 1) == -4
    for m in (miro(-1.0, mu=a), miro(math.nan, mu=a), miro(INF, mu=a), miro(eta=-0.1, mu=a), miro(eta=math.nan, mu=a), miro(eta=INF, mu=a),
              miro(mu0=math.nan, mu=a), miro(mu0=INF, mu=a), miro(mu0=-INF, mu=a), miro(mu=None)):
        assert call(m, n) == -1 and call(m, n - 1) == -1, (m.tau, m.eta, m.mu0)
    assert call(miro(mu=a + 2), n) == -2 and call(miro(mu=a, surprise=a + 1), n) == -2 and call(miro(mu=a, kept=a + 3), n) == -2
    assert call(miro(-1.0, mu=a + 2), n) == -1      # SSC_EINVAL comes first
    # everything ssc_decode_sample_opts refuses stays refused
    assert call(miro(mu=a), n, smp=L.SamplerDesc(0, 0, 1.0, 0.0, 3)) == -1        # temperature 0
    assert call(miro(mu=a), n, smp=L.SamplerDesc(3, 0, 1.0, 1.0, 3)) == -1
    assert call(miro(mu=a), n, opts=bad_opts) == -1
    assert call(miro(mu=a), n, opts=sample_opts(trunc=L.Truncation(5, 0.5, None, None))) == -1
    assert call(miro(mu=a), n - 1, opts=sample_opts(trunc=trunc)) == -4
    d.beam = 2
    assert call(miro(mu=a), n) == -1
    d.beam = 1
    assert CFG["V"] == 50


# ---- the runtime ------------------------------------------------------------------------------------------------------------------------------
def dims(**kw):
    base = dict(V=50, E=8, H=8, A=8, F=8, Z=4, S=0, kld_mode=0, pm_scale=0.0, prior_var=1.0)
    base.update(kw)
    return ModelDims(**base)


def test_diverse_decode_takes_a_mirostat_with_a_word_sampler_only():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    feats = torch.zeros(2, 3, 8)
    base = dict(n_samples=3, max_steps=6, boundary_index=1, mirostat=sampling.Mirostat(3.0))
    for kw, name in ((dict(beam=2), "not the beam search"),
                     (dict(beam=2, sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                     (dict(beam=2, sampler=sampling.TopKSampler(k=5), sampled_beam=True), "sampled-node beam search"),
                     (dict(beam=2, diverse_beam=sampling.DiverseBeam(2, 0.5)), "diverse beam search"),
                     (dict(beam=2, rules=sampling.DecodeRules(2, 0, 1.0, ())), "beam search under decode rules")):
        with pytest.raises(ValueError, match="Mirostat belongs to the word samplers.*" + name):
            diverse_decode(dec, feats, None, **base, **kw)
    with pytest.raises(NotImplementedError, match="Mirostat.*ensemble"):
        diverse_decode(EnsembleDecodeEngine([dec]), feats, None, beam=1, sampler=sampling.TopKSampler(k=5), **base)
    # an inactive Mirostat is none: the beam search's own refusal of a word sampler at beam 2 is what is left
    with pytest.raises(ValueError, match="beam must be 1"):
        diverse_decode(dec, feats, None, 3, 2, 6, 1, sampler=sampling.TopKSampler(k=5), mirostat=sampling.Mirostat(0.0))
    with pytest.raises(ValueError, match="mirostat_stats needs an active mirostat"):
        diverse_decode(dec, feats, None, 3, 1, 6, 1, sampler=sampling.TopKSampler(k=5), mirostat_stats=True)
    with pytest.raises(ValueError, match="mirostat_stats needs an active mirostat"):
        dec.sample(None, None, 3, 6, 1, None, None, sampling.TopKSampler(k=5), 1, mirostat_stats=True)


# ---- the script's refusals ----------------------------------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script_mirostat", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_checks_the_mirostat_flags(tmp_path):
    mod = script_module()
    args = lambda *a: mod.parser.parse_args(BASE + list(a))
    assert mod.check_mirostat_args(args()) is None and mod.check_mirostat_args(args("--mirostat", "0")) is None
    m = mod.check_mirostat_args(args("--mirostat", "3:0.25"))
    assert (m.tau, m.eta, m.mu0, m.unit) == (3.0, 0.25, 6.0, "bits")
    assert mod.check_mirostat_args(args("--mirostat", "2.5")).eta == 0.1
    for flag, msg in (("-1", "tau must be finite"), ("3:-0.5", "eta must be finite"), ("much", "two numbers"), ("3:x", "two numbers")):
        with pytest.raises(SystemExit, match=msg):
            mod.check_mirostat_args(args("--mirostat=" + flag))
    f = tmp_path / "ck.pt"
    f.write_text("")
    with pytest.raises(SystemExit, match="not available with --ensemble-checkpoints"):
        mod.check_mirostat_args(args("--mirostat", "3", "--checkpoint-path", str(f), "--ensemble-checkpoints", str(f)))
    for override in ([], ["MODEL.STOCHASTIC_BEAM_SEARCH", True], ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", True]):
        with pytest.raises(SystemExit, match="needs a word sampler"):
            mod.check_mirostat_args(args("--mirostat", "3"), Config(config_override=override).MODEL)
    topp = Config(config_override=TOPP).MODEL
    assert mod.check_mirostat_args(args("--mirostat", "3"), topp).tau == 3.0 and mod.check_mirostat_args(args(), topp) is None
    with pytest.raises(SystemExit, match="--mirostat-output needs an active Mirostat"):
        mod.check_mirostat_args(args("--mirostat-output", "m.json"), topp)
    keys = Config(config_override=TOPP + ["MODEL.SAMPLER_MIROSTAT_TAU", 2.0, "MODEL.SAMPLER_MIROSTAT_ETA", 0.3]).MODEL
    m = mod.check_mirostat_args(args("--mirostat-output", "m.json"), keys)
    assert (m.tau, m.eta) == (2.0, 0.3) and mod.check_mirostat_args(args("--mirostat", "4"), keys).eta == 0.3
