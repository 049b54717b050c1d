"""CPU: contrastive decoding for the word samplers (include/ssc.h: ssc_contrast_rows, ssc_contrast) - the float64 restatement's own
invariants (tests/contrastref.py), the amateur's features, the MODEL keys, the runtime's and the script's refusals, and everything the
library refuses before any launch."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import contrastref as R
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config
from ssc_runtime.contrast import AMATEURS, Contrast, amateur_features, contrast_from_config, contrast_from_name
from ssc_runtime.decode import DecodeEngine, EnsembleDecodeEngine
from ssc_runtime.engine import ModelDims
from ssc_runtime.inference import diverse_decode
from ssc_runtime.vocab import Vocabulary
from test_attention_trace_cpu import CFG, RETIRED_SAMPLE_ENTRIES, header, model_cfg, sample_opts, search_desc, struct_fields
from truncationref import D_BAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def rows(V=200, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(V) * 3).astype(np.float32), (rng.standard_normal(V) * 2).astype(np.float32)


def test_the_edit_is_the_expert_sharpened_against_the_amateur():
    """softmax(y) over the kept set is proportional to p_e^(1 + alpha) / p_a^alpha - a brute-force restatement of the formula."""
    xe, xa = rows()
    pe, pa = np.exp(R.log_softmax(xe)), np.exp(R.log_softmax(xa))
    for alpha in R.ALPHAS:
        for beta in R.BETAS:
            e = R.contrast_row(xe, xa, alpha, beta)
            kept = pe >= np.float64(np.float32(beta)) * pe.max() if beta else np.ones_like(pe, dtype=bool)
            assert (e.kept == kept).all() and e.undecidable == []
            w = np.where(kept, pe ** (1 + alpha) / pa ** alpha, 0.0)
            np.testing.assert_allclose(np.exp(R.log_softmax(e.y)), w / w.sum(), rtol=1e-9, atol=1e-300)
            assert (e.y[~kept] == -np.inf).all() and np.isfinite(e.y[kept]).all()
            np.testing.assert_allclose(e.kl, (pe * (np.log(pe) - np.log(pa))).sum(), rtol=1e-9)
            assert e.kl > 0


def test_alpha_zero_and_an_equal_amateur_leave_the_experts_log_probs():
    xe, xa = rows()
    lp = R.log_softmax(xe)
    for beta in R.BETAS:
        a0 = R.contrast_row(xe, xa, 0.0, beta)
        none = R.contrast_row(xe, None, 0.0, beta)
        assert (a0.y[a0.kept] == lp[a0.kept]).all() and (none.y == a0.y).all() and none.kl == 0.0 and a0.kl > 0
        for alpha in R.ALPHAS:
            same = R.contrast_row(xe, xe, alpha, beta)
            assert (same.y[same.kept] == lp[same.kept]).all() and same.kl == 0.0 and (same.kept == a0.kept).all()
    with pytest.raises(ValueError):
        R.contrast_row(xe, None, 1.0, 0.1)


def test_the_plausible_set():
    """beta = 0 keeps everything; the set shrinks as beta grows; every maximal entry is kept at any beta; a peaked row keeps one."""
    xe, xa = rows()
    xe[[3, 77]] = xe.max() + 1.0
    sets = [R.contrast_row(xe, xa, 1.0, b).kept for b in (0.0, 0.01, 0.1, 0.5, 0.999)]
    assert sets[0].all()
    for big, small in zip(sets, sets[1:]):
        assert (big | ~small).all() and big.sum() >= small.sum()
    assert sets[-1][[3, 77]].all() and sets[-1].sum() == 2
    peaked = xe.copy()
    peaked[5] = 40.0
    assert R.contrast_row(peaked, xa, 1.0, 0.1).kept.sum() == 1


def test_undecidable_tokens_are_reported():
    """A token within D_BAND of the cut is reported, on either side of it; a maximal entry never is."""
    logb = R.logb_of(0.1)
    for shift, want in ((0.0, [1]), (0.4 * D_BAND, [1]), (-0.4 * D_BAND, [1]), (3 * D_BAND, []), (-3 * D_BAND, [])):
        x32 = np.array([2.0, 2.0 + logb + shift, 0.0, -1.0], dtype=np.float32)
        e = R.contrast_row(x32, None, 0.0, 0.1)
        assert e.undecidable == want, shift
        assert bool(e.kept[1]) == (e.lp_e[1] >= logb + e.lp_e.max())
    assert R.contrast_row(np.array([2.0, 2.0, 1.0], dtype=np.float32), None, 0.0, 0.999).undecidable == []
    assert R.logb_of(0.1) == float(np.float32(math.log(float(np.float32(0.1)))))


@pytest.mark.parametrize("V,ld,off,lda,offa", R.SHAPES)
def test_the_kernel_tests_inputs_are_decidable(V, ld, off, lda, offa):
    """What tests/test_contrast_gpu.py asserts first, checked here without a device: no undecidable token at any beta; the rows are
    what they are meant to be - the cut drops entries, the grid row keeps its three maxima, the ended row is left as it came."""
    xe, xa, last = R.rows_case(V, ld, lda, R.row_seed(V))
    for beta in R.BETAS:
        for alpha in R.ALPHAS:
            out, kept, kl, live, und = R.edit_rows(xe, xa, V, alpha, beta, last, R.END)
            assert und == [], (V, alpha, beta, und[:5])
            assert live.tolist() == [True] * 4 + [False] and kept[4] == 0 and kl[4] == 0 and np.isnan(out[4]).all()
            assert np.isnan(out[:, V:]).all()
            assert kl[2] == 0 and (kl[[0, 1, 3]] > 0).all()
            if beta == 0:
                assert kept[:4].tolist() == [V] * 4
            else:
                assert (kept[:4] < V).all() and (kept[:4] >= 1).all() and kept[1] == 1 and kept[3] >= 3


# ---- the amateur's features ---------------------------------------------------------------------------------------------------------------
def test_amateur_features_keep_the_region_mask():
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(3, 6, 8, generator=g)
    feats[0, 4:] = 0
    feats[2, 1] = 0
    mean = amateur_features(feats, "mean")
    for i in range(3):
        live = (feats[i] != 0).any(-1)
        assert torch.equal((mean[i] != 0).any(-1), live)
        want = feats[i][live].mean(0)
        for r in torch.nonzero(live).flatten():
            torch.testing.assert_close(mean[i, r], want)
    noisy = amateur_features(feats, "noise:0.5", torch.Generator().manual_seed(1))
    again = amateur_features(feats, "noise:0.5", torch.Generator().manual_seed(1))
    assert torch.equal(noisy, again) and not torch.equal(noisy, feats)
    assert torch.equal((noisy != 0).any(-1), (feats != 0).any(-1))
    full = amateur_features(feats, "noise:1", torch.Generator().manual_seed(1))
    assert abs(float(full[1].std()) / float(feats[1].std()) - 1) < 0.5       # pure noise at the image's own scale
    for bad in ("noise", "noise:0", "noise:1.5", "noise:x", "median"):
        with pytest.raises(ValueError, match="features must be"):
            amateur_features(feats, bad)


def test_contrast_checks_its_arguments():
    c = Contrast(1.0)
    assert (c.alpha, c.beta, c.active, c.steps_amateur, c.own_context) == (1.0, 0.1, True, True, False)
    assert not Contrast(0.0, 0.0, features="mean").active
    cut = Contrast(0.0, 0.5, features="mean")
    assert cut.active and not cut.steps_amateur
    for kw in (dict(alpha=-0.1), dict(alpha=INF), dict(alpha=math.nan), dict(alpha=1, beta=1.0), dict(alpha=1, beta=-0.1),
               dict(alpha=1, beta=math.nan), dict(alpha=1, features="median"), dict(alpha=1, features="noise:2"), dict(alpha=1, features=3),
               dict(alpha=1, latent="zero"), dict(alpha=1, guide="none")):
        with pytest.raises(ValueError, match="Contrast"):
            Contrast(**kw)
    for name in AMATEURS:
        c = contrast_from_name(1.5, 0.2, name, 0.25)
        assert (c.alpha, c.beta) == (1.5, 0.2)
    assert contrast_from_name(1, 0.1, "noise-features", 0.25).features == "noise:0.25"
    assert contrast_from_name(1, 0.1, "prior-mean").latent == "mean" and contrast_from_name(1, 0.1, "neutral-sentiment").sentiment == 0.0
    with pytest.raises(ValueError, match="amateur must be one of"):
        contrast_from_name(1, 0.1, "weak")


# ---- the configuration ----------------------------------------------------------------------------------------------------------------------
TOPP = ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", 0.95, "MODEL.BEAM_SIZE", 1]


def test_config_defaults_are_off():
    c = Config()
    assert (c.MODEL.CONTRAST_ALPHA, c.MODEL.CONTRAST_BETA, c.MODEL.CONTRAST_AMATEUR, c.MODEL.CONTRAST_NOISE) == (0.0, 0.1, "mean-features", 0.5)
    assert contrast_from_config(c.MODEL) is None
    # the other keys alone select nothing
    assert contrast_from_config(Config(config_override=TOPP + ["MODEL.CONTRAST_BETA", 0.5, "MODEL.CONTRAST_AMATEUR", "prior-mean"]).MODEL) is None


def test_the_keys_are_read_and_need_a_word_sampler():
    c = Config(config_override=TOPP + ["MODEL.CONTRAST_ALPHA", 1.5, "MODEL.CONTRAST_BETA", 0.2, "MODEL.CONTRAST_AMATEUR", "noise-features",
                                       "MODEL.CONTRAST_NOISE", 0.25])
    k = contrast_from_config(c.MODEL)
    assert (k.alpha, k.beta, k.features) == (1.5, 0.2, "noise:0.25")
    assert isinstance(sampling.from_config(c.MODEL), sampling.TopPSampler)
    for other, match in (([], "needs MODEL.DECODE_SAMPLER"), (["MODEL.STOCHASTIC_BEAM_SEARCH", True], "needs MODEL.DECODE_SAMPLER"),
                         (["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLED_BEAM_SEARCH", True], "SAMPLED_BEAM_SEARCH exclude")):
        c = Config(config_override=["MODEL.CONTRAST_ALPHA", 1.0] + other)
        for read in (lambda: contrast_from_config(c.MODEL), lambda: sampling.from_config(c.MODEL)):
            with pytest.raises(ValueError, match=match) as e:
                read()
            assert "MODEL.CONTRAST_ALPHA" in str(e.value)


@pytest.mark.parametrize("override,match", [
    (["MODEL.CONTRAST_ALPHA", -1.0], "CONTRAST_ALPHA"), (["MODEL.CONTRAST_ALPHA", "nan"], "CONTRAST_ALPHA"),
    (["MODEL.CONTRAST_ALPHA", "inf"], "CONTRAST_ALPHA"),
    (["MODEL.CONTRAST_BETA", 1.0], "CONTRAST_BETA"), (["MODEL.CONTRAST_BETA", -0.1], "CONTRAST_BETA"),
    (["MODEL.CONTRAST_NOISE", 0.0], "CONTRAST_NOISE"), (["MODEL.CONTRAST_NOISE", 1.5], "CONTRAST_NOISE"),
    (["MODEL.CONTRAST_AMATEUR", "weak"], "mean-features \\| noise-features"),
])
def test_config_validation(override, match):
    override = [float(v) if v in ("nan", "inf") else v for v in override]
    with pytest.raises(ValueError, match=match):
        Config(config_override=TOPP + override)
    Config(config_override=TOPP + ["MODEL.CONTRAST_ALPHA", 2, "MODEL.CONTRAST_BETA", 0, "MODEL.CONTRAST_NOISE", 1.0])


def test_a_model_reads_the_keys_with_a_word_sampler_only():
    from var_updown.models import UpDownCaptioner
    small = ["MODEL.IMAGE_FEATURE_SIZE", 8, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
             "MODEL.Z_SPACE", 4]
    c = Config(config_override=TOPP + ["MODEL.CONTRAST_ALPHA", 1.0, "MODEL.CONTRAST_AMATEUR", "prior-mean"] + small)
    vocab = Vocabulary.synthetic(40)
    m = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu")     # (scripts/train.py: no sampler, the keys are not read)
    assert m._contrast is None
    with pytest.raises(ValueError, match="needs a word sampler"):
        m.contrast(Contrast(1.0))
    m.contrast(None)
    s = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu", sampler=sampling.from_config(c.MODEL))
    assert isinstance(s._contrast, Contrast) and s._contrast.latent == "mean" and s._contrast.alpha == 1.0
    s.contrast(Contrast(0.0, 0.0))            # inactive: off
    assert s._contrast is None
    s.contrast(Contrast(2.0, features="mean"))
    assert s._contrast.alpha == 2.0
    with pytest.raises(ValueError, match="Contrast or None"):
        s.contrast(sampling.LogitRules())


# ---- the struct and the bindings against the header ---------------------------------------------------------------------------------------
def test_bindings_mirror_the_header():
    names = [f for f, _ in L.Contrast._fields_]
    assert struct_fields("ssc_contrast") == names == ["alpha", "beta", "params", "feats", "imgbuf", "sentiment", "eps0", "eps", "obj_atts",
                                                      "guide_mode", "start", "kept", "divergence"]
    assert C.sizeof(L.Contrast) == 96
    for name in ("ssc_contrast_rows", "ssc_decode_sample_opts_workspace_bytes", "ssc_decode_sample_opts"):
        assert name in L.SYMBOLS and name + "(" in header()
    assert len(L.SYMBOLS["ssc_contrast_rows"][1]) == 13
    # the sampled decode's options are one descriptor - the header's field order, the size and four pointers - behind one entry
    assert struct_fields("ssc_sample_opts") == [f for f, _ in L.SampleOpts._fields_] == ["bytes", "guide", "rules", "trunc", "contrast"]
    assert C.sizeof(L.SampleOpts) == 5 * C.sizeof(C.c_void_p) and L.SampleOpts._fields_[4][1] is C.POINTER(L.Contrast)
    cdll = C.CDLL(L.LIB_PATH)
    for name in RETIRED_SAMPLE_ENTRIES:
        assert name not in L.SYMBOLS and not hasattr(cdll, name) and name + "(" not in header(), name
    assert L.SYMBOLS["ssc_contrast_rows"][1][6] is C.c_float and L.SYMBOLS["ssc_contrast_rows"][1][7] is C.c_float
    assert L.load().ssc_version() == 4
    # the pinned structs keep their sizes
    assert (C.sizeof(L.SamplerDesc), C.sizeof(L.LogitRules), C.sizeof(L.Truncation)) == (24, 80, 24)


# ---- refusals, without a GPU ------------------------------------------------------------------------------------------------------------
BAD_KNOBS = [(-0.5, 0.1), (math.nan, 0.1), (INF, 0.1), (-INF, 0.1), (1.0, 1.0), (1.0, 1.5), (1.0, -0.1), (1.0, math.nan), (0.0, 1.0),
             (0.0, math.nan)]
GOOD_KNOBS = [(1.0, 0.1), (0.5, 0.0), (0.0, 0.5), (2.0, 0.999)]
END = 1


def test_rows_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    V = 50

    def call(alpha=1.0, beta=0.1, logits=a, ld=V, am=a, lda=V, rows=3, V=V, last=a, end=END, kept=None, div=None):
        return lib._raw_ssc_contrast_rows(logits, ld, am, lda, rows, V, alpha, beta, last, end, kept, div, None)

    assert call(0.0, 0.0) == 0 and call(0.0, 0.0, am=None, last=None, end=-7) == 0           # off: SSC_OK with no launch
    for al, be in GOOD_KNOBS:
        assert call(al, be, rows=0) == 0                                                     # nothing to edit
    assert call(0.0, 0.5, am=None, rows=0) == 0                                              # the cut alone takes no amateur
    assert call(logits=None) == -1 and call(am=None) == -1 and call(1e-3, 0.0, am=None) == -1
    for kw in (dict(ld=49), dict(lda=49), dict(rows=-1), dict(V=0), dict(end=-1), dict(end=50)):
        assert call(**kw) == -1, kw
        assert call(0.0, 0.0, **kw) == -1, kw            # (what does not depend on the knobs is refused with them off as well)
    assert call(0.0, 0.5, am=None, lda=0, rows=0) == 0   # (no amateur: its leading dimension is not read)
    for al, be in BAD_KNOBS:
        assert call(al, be) == -1, (al, be)
        assert call(al, be, rows=0) == -1, (al, be)
    # alignment: a pointer that is no multiple of 4
    assert call(logits=a + 2) == -2 and call(am=a + 1) == -2 and call(last=a + 3) == -2
    assert call(kept=a + 2) == -2 and call(div=a + 1) == -2 and call(0.0, 0.0, kept=a + 1) == -2
    assert call(1.0, 1.5, kept=a + 2) == -1              # SSC_EINVAL comes first


def contrast(alpha=1.0, beta=0.1, **kw):
    c = L.Contrast()
    c.alpha, c.beta = alpha, beta
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_decode_refuses_a_bad_contrast_before_any_launch():
    """A descriptor that passes every check with a workspace one byte short: SSC_EWORKSPACE (-4) without a contrast, with both knobs 0
    and with good ones - they were accepted, nothing was launched -, SSC_EINVAL / SSC_EALIGN for every bad one whatever the
    workspace.  A NULL contrast, both knobs 0 and the cut alone cost the workspace of ssc_decode_sample; an amateur that is stepped
    costs its states, alpha, logits and step workspace on top."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    d = search_desc(a, beam=1, per_node=1)
    c_, dd = C.byref(cfg), C.byref(d)
    n0 = lib.ssc_decode_sample_workspace_bytes(c_, dd)
    size = lambda c: lib.ssc_decode_sample_opts_workspace_bytes(c_, dd, C.byref(sample_opts(contrast=c)))
    assert n0 > 0 and size(None) == n0 == size(contrast(0.0, 0.0)) == size(contrast(0.0, 0.5))
    assert lib.ssc_decode_sample_opts_workspace_bytes(c_, dd, None) == n0
    n = size(contrast())
    B, H, V, Rr = 6, CFG["H"], CFG["V"], 5
    assert n >= n0 + 4 * (8 * B * H + B * Rr + B * V) + lib.ssc_decode_step_workspace_bytes(c_, B, Rr)
    assert n == size(contrast(2.0, 0.0, feats=a, imgbuf=a))
    p = L.Params()

    def call(c, nbytes, smp=None, rules=None, trunc=None, guide=None):
        smp = smp or L.SamplerDesc(0, 0, 1.0, 1.0, 3)
        return lib._raw_ssc_decode_sample_opts(c_, C.byref(p), dd, C.byref(smp), C.byref(sample_opts(guide, rules, trunc, c)), a, nbytes,
                                               None)

    assert call(None, n0 - 1) == -4 and call(contrast(0.0, 0.0), n0 - 1) == -4 and call(contrast(0.0, 0.5), n0 - 1) == -4
    for al, be in GOOD_KNOBS:
        c = contrast(al, be, kept=a, divergence=a)
        assert call(c, size(c) - 1) == -4, (al, be)
    assert call(contrast(), n0) == -4                      # (the amateur's blocks are wanted)
    good = contrast(feats=a, imgbuf=a, params=C.addressof(p), sentiment=a, eps0=a, eps=a, guide_mode=1)
    assert call(good, n - 1) == -4
    for al, be in BAD_KNOBS:
        assert call(contrast(al, be), n - 1) == -1 and call(contrast(al, be), n) == -1, (al, be)
    assert call(contrast(feats=a), n) == -1 and call(contrast(imgbuf=a), n) == -1          # both or neither
    assert call(contrast(params=C.addressof(p)), n) == -1                                  # params without its own context
    assert call(contrast(0.0, 0.0, feats=a), n) == -1                                      # (refused with the knobs off as well)
    assert call(contrast(guide_mode=2), n) == -1 and call(contrast(guide_mode=-1), n) == -1
    assert call(contrast(kept=a + 2), n) == -2 and call(contrast(divergence=a + 1), n) == -2
    assert call(contrast(1.0, 1.5, kept=a + 2), n) == -1                                   # SSC_EINVAL comes first
    # a start state on one side only, or an amateur's start with a NULL block
    st = L.StartState(a, a, a, a, a)
    half = L.StartState(a, a, None, a, a)
    no_tokens = L.StartState(a, a, a, a, None)
    assert call(contrast(start=C.pointer(st)), n) == -1
    d.start = C.pointer(st)
    assert call(contrast(), n) == -1 and call(contrast(start=C.pointer(half)), n) == -1
    assert call(contrast(start=C.pointer(st)), n - 1) == -4 and call(contrast(start=C.pointer(no_tokens)), n - 1) == -4
    assert call(contrast(0.0, 0.5), n0 - 1) == -4           # (an amateur that is not stepped reads no start state)
    d.start = None
    # everything the call refuses without a contrast stays refused: a bad sampler, bad rules, a bad truncation, a bad guide, a bad descriptor
    assert call(contrast(), n, smp=L.SamplerDesc(0, 0, 1.0, 0.0, 3)) == -1
    bad_rules = L.LogitRules()
    bad_rules.repetition_penalty = 0.0
    assert call(contrast(), n, rules=bad_rules) == -1
    assert call(contrast(), n, trunc=L.Truncation(1, 1.5, None, None)) == -1
    assert call(contrast(), n - 1, trunc=L.Truncation(2, 0.05, None, None)) == -4
    assert call(contrast(), n, guide=L.LatentGuideDesc(0, a, a, 4, a)) == -1
    assert call(contrast(guide_mode=1), n - 1, guide=L.LatentGuideDesc(3, a, a, 4, a)) == -4
    d.feats = None
    assert call(contrast(), n) == -1
    d.feats = a
    d.beam = 2
    assert call(contrast(), n) == -1
    d.beam = 1
    # NULL opts are the call with a NULL contrast: the same refusals and the same workspace
    assert lib._raw_ssc_decode_sample_opts(c_, C.byref(p), dd, C.byref(L.SamplerDesc(0, 0, 1.0, 1.0, 3)), None, a, n0 - 1, None) == -4


# ---- the runtime --------------------------------------------------------------------------------------------------------------------------
def dims(**kw):
    base = dict(V=50, E=8, H=8, A=8, F=8, Z=4, S=0, kld_mode=0, pm_scale=0.0, prior_var=1.0)
    base.update(kw)
    return ModelDims(**base)


def test_diverse_decode_takes_a_contrast_with_a_word_sampler_only():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    feats = torch.zeros(2, 3, 8)
    base = dict(n_samples=3, max_steps=6, boundary_index=1, contrast=Contrast(1.0))
    for kw, name in ((dict(beam=2), "not the beam search"),
                     (dict(beam=2, sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                     (dict(beam=2, sampler=sampling.TopKSampler(k=5), sampled_beam=True), "sampled-node beam search"),
                     (dict(beam=2, diverse_beam=sampling.DiverseBeam(2, 0.5)), "diverse beam search"),
                     (dict(beam=2, rules=sampling.DecodeRules(2, 0, 1.0, ())), "beam search under decode rules")):
        with pytest.raises(ValueError, match="contrast belongs to the word samplers.*" + name):
            diverse_decode(dec, feats, None, **base, **kw)
    with pytest.raises(NotImplementedError, match="contrast.*ensemble"):
        diverse_decode(EnsembleDecodeEngine([dec]), feats, None, beam=1, sampler=sampling.TopKSampler(k=5), **base)
    # an inactive contrast is no contrast: the beam search's own refusal of a word sampler at beam 2 is what is left
    with pytest.raises(ValueError, match="beam must be 1"):
        diverse_decode(dec, feats, None, 3, 2, 6, 1, sampler=sampling.TopKSampler(k=5), contrast=Contrast(0.0, 0.0))
    with pytest.raises(ValueError, match="contrast_stats needs an active contrast"):
        diverse_decode(dec, feats, None, 3, 1, 6, 1, sampler=sampling.TopKSampler(k=5), contrast_stats=True)
    with pytest.raises(ValueError, match="contrast_stats needs an active contrast"):
        dec.sample(None, None, 3, 6, 1, None, None, sampling.TopKSampler(k=5), 1, contrast_stats=True)
    # an amateur engine of other dims is refused; so are all-zero amateur features
    other = DecodeEngine(dims(H=16), lambda: L.Params(), "cuda")
    with pytest.raises(ValueError, match="dims of the expert"):
        Contrast(1.0, engine=other).prepare(dec, feats)
    with pytest.raises(ValueError, match="all zero"):
        Contrast(1.0, features="mean").prepare(dec, feats)
    with pytest.raises(ValueError, match="amateur's features are"):
        Contrast(1.0, features=torch.ones(2, 4, 8)).prepare(dec, torch.ones(2, 3, 8))
    assert Contrast(0.0, 0.5, features="mean").prepare(dec, feats).ctx is None      # the cut alone prepares nothing


# ---- the script's refusals ----------------------------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script_contrast", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_checks_the_contrast_flags(tmp_path):
    mod = script_module()
    args = lambda *a: mod.parser.parse_args(BASE + list(a))
    word = Config(config_override=TOPP).MODEL
    assert mod.check_contrast_args(args()) == (None, None, None)
    assert mod.check_contrast_args(args("--contrast", "1.5:0.2", "--contrast-amateur", "prior-mean")) == (1.5, 0.2, "prior-mean")
    assert mod.check_contrast_args(args("--contrast", "2")) == (2.0, None, None)
    for flag, msg in (("much", "ALPHA\\[:BETA\\]"), ("1:x", "ALPHA\\[:BETA\\]"), ("-1", "ALPHA must be"), ("inf", "ALPHA must be"),
                      ("1:1", "BETA must lie"), ("1:-0.5", "BETA must lie")):
        with pytest.raises(SystemExit, match=msg):
            mod.check_contrast_args(args("--contrast", flag))
    with pytest.raises(SystemExit, match="--contrast-amateur: one of mean-features"):
        mod.check_contrast_args(args("--contrast", "1", "--contrast-amateur", "weak"))
    with pytest.raises(SystemExit, match="--contrast-checkpoint: no such checkpoint"):
        mod.check_contrast_args(args("--contrast", "1", "--contrast-checkpoint", str(tmp_path / "none.pt")))
    # with the MODEL node: the keys fill the gaps; off without an ALPHA
    assert mod.check_contrast_args(args(), word) is None
    assert mod.check_contrast_args(args("--contrast", "0"), word) is None
    assert mod.check_contrast_args(args("--contrast", "0:0.5"), word) == (0.0, 0.5, "mean-features")
    assert mod.check_contrast_args(args("--contrast", "2"), word) == (2.0, 0.1, "mean-features")
    keyed = Config(config_override=TOPP + ["MODEL.CONTRAST_ALPHA", 1.5, "MODEL.CONTRAST_BETA", 0.3, "MODEL.CONTRAST_AMATEUR", "prior-mean"]).MODEL
    assert mod.check_contrast_args(args(), keyed) == (1.5, 0.3, "prior-mean")
    assert mod.check_contrast_args(args("--contrast", "0"), keyed) is None
    assert mod.check_contrast_args(args("--contrast-amateur", "neutral-sentiment"), keyed) == (1.5, 0.3, "neutral-sentiment")
    f = tmp_path / "ck.pt"
    f.write_text("")
    assert mod.check_contrast_args(args("--contrast", "1", "--contrast-checkpoint", str(f)), word) == (1.0, 0.1, None)
    assert mod.check_contrast_args(args("--contrast", "1", "--contrast-checkpoint", str(f), "--contrast-amateur", "prior-mean"),
                                   word) == (1.0, 0.1, "prior-mean")
    for extra, name in ((("--contrast-amateur", "prior-mean"), "--contrast-amateur"), (("--contrast-output", str(tmp_path / "d.json")), "--contrast-output"),
                        (("--contrast-checkpoint", str(f)), "--contrast-checkpoint")):
        with pytest.raises(SystemExit, match=name + " needs an active contrast"):
            mod.check_contrast_args(args(*extra), word)
    with pytest.raises(SystemExit, match="not available with --ensemble-checkpoints"):
        mod.check_contrast_args(args("--contrast", "1", "--checkpoint-path", str(f), "--ensemble-checkpoints", str(f)), word)
    for override in ([], ["MODEL.STOCHASTIC_BEAM_SEARCH", True], ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", True]):
        with pytest.raises(SystemExit, match="--contrast needs a word sampler"):
            mod.check_contrast_args(args("--contrast", "1"), Config(config_override=override).MODEL)
