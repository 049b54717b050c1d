"""CPU: the truncation of the word samplers (include/ssc.h: ssc_truncation) - the restatement (tests/truncationref.py) against a
brute-force sort and on hand-made rows, the classes, the config keys and their refusals, the struct and the bindings against the
header, every refusal of the three new symbols (no launch is reached: no GPU needed), the runtime's refusals and those of
scripts/inference.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import truncationref as R
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
VALUES = {1: (0.2, 0.5, 0.9, 1.0), 2: (0.01, 0.3, 1.0), 3: (3e-4, 0.05, 0.6), 4: (3e-4, 0.05, 0.6)}


# ---- the restatement against a brute-force sort ---------------------------------------------------------------------------------------
def brute_force(x, kind, value, T):
    """The definitions of include/ssc.h word for word, with Python lists and math.* in place of array operations."""
    V = len(x)
    fin = [v for v in range(V) if math.isfinite(x[v])]
    if not fin:
        return set(), 0.0
    mx = max(float(x[v]) for v in fin)
    e = {v: math.exp((float(x[v]) - mx) / T) for v in fin}
    Z = math.fsum(e.values())
    q = {v: e[v] / Z for v in fin}
    logq = {v: (float(x[v]) - mx) / T - math.log(Z) for v in fin}
    H = -math.fsum(q[v] * logq[v] for v in fin)
    first = min(v for v in fin if float(x[v]) == mx)
    if kind == 1:
        order = sorted(fin, key=lambda v: (abs(-logq[v] - H), v))
        kept, ahead = set(), 0.0
        for i, v in enumerate(order):
            if i == 0 or ahead < value or value >= 1.0:   # (tau = 1 keeps every finite entry)
                kept.add(v)
            ahead += q[v]
        return kept, H
    if kind == 2:
        return {v for v in fin if logq[v] >= math.log(value) + logq[first]}, H
    eta = min(value, math.sqrt(value) * math.exp(-H)) if kind == 3 else value
    return {v for v in fin if logq[v] >= math.log(eta)} | {first}, H


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_restatement_against_a_brute_force_sort(kind):
    rng = np.random.default_rng(100 + kind)
    checked = 0
    for case in range(120):
        V = int(rng.integers(2, 60))
        T = float(rng.choice([0.7, 1.0, 1.3]))
        x = (rng.standard_normal(V) * float(rng.choice([0.5, 2.0, 5.0]))).astype(np.float32)
        if rng.random() < 0.3:
            x[rng.random(V) < 0.3] = -np.inf
        if rng.random() < 0.3:   # duplicated values
            x[rng.integers(0, V, size=V // 2)] = x[int(rng.integers(0, V))]
        value = float(rng.choice(VALUES[kind]))
        c = R.truncate_row(x, kind, value, T)
        want, H = brute_force(x, kind, value, T)
        assert abs(c.H - H) < 1e-12, (case, c.H, H)
        if c.undecidable:    # a cumsum and an fsum may differ in the last place exactly there
            continue
        assert set(np.nonzero(c.kept)[0].tolist()) == want, (case, kind, value, T)
        checked += 1
    assert checked >= 90


# ---- hand-made rows -----------------------------------------------------------------------------------------------------------------------
def kept_ids(c):
    return np.nonzero(c.kept)[0].tolist()


def test_a_flat_row_keeps_the_lowest_indices_up_to_the_mass():
    c = R.truncate_row(np.zeros(37, dtype=np.float32), 1, 0.5)
    assert kept_ids(c) == list(range(19)) and c.undecidable == []   # 18 / 37 < 0.5 <= 19 / 37
    assert abs(c.H - math.log(37)) < 1e-12
    assert kept_ids(R.truncate_row(np.zeros(37, dtype=np.float32), 1, 1.0)) == list(range(37))
    # every other kind keeps a flat row whole (q = 1 / 37 against thresholds of at most 0.6 / 37 ... ) - or, for a large epsilon,
    # the lowest-index maximum alone
    assert kept_ids(R.truncate_row(np.zeros(37, dtype=np.float32), 2, 1.0)) == list(range(37))
    assert kept_ids(R.truncate_row(np.zeros(37, dtype=np.float32), 4, 0.01)) == list(range(37))
    assert kept_ids(R.truncate_row(np.zeros(37, dtype=np.float32), 4, 0.5)) == [0]
    # ... where eta adapts to the entropy: eta = min(0.5, sqrt(0.5) / 37) = 0.019 < 1 / 37
    assert kept_ids(R.truncate_row(np.zeros(37, dtype=np.float32), 3, 0.5)) == list(range(37))


def test_a_peaked_row_keeps_one_token():
    x = np.full(50, -3.0, dtype=np.float32)
    x[17] = 8.0     # q_17 = 0.9992
    for kind, value in ((1, 0.9), (2, 0.05), (3, 3e-4), (4, 3e-4)):
        c = R.truncate_row(x, kind, value)
        assert kept_ids(c) == [17], (kind, kept_ids(c))
    # the most probable word need not be typical: with mass on a broad shoulder the peak's surprise is far below the entropy
    y = np.zeros(200, dtype=np.float32)
    y[0] = 4.0      # q_0 = 0.215, s_0 = 1.54; the others s = 5.54; H = 4.68: the shoulder comes first
    c = R.truncate_row(y, 1, 0.5)
    assert 0 not in kept_ids(c) and kept_ids(c)[0] == 1


def test_duplicated_values_at_the_cut_go_by_the_index():
    x = np.array([2.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, -5.0], dtype=np.float32)
    st = R.row_stats(x, 1.0)
    q = st[1]
    c = R.truncate_row(x, 1, 0.5)
    # the order is by |s - H|; whatever it is, tokens of one value are taken lowest index first and the set is a prefix of it
    d = np.abs(-np.log(q) - st[3])
    order = np.lexsort((np.arange(8), d))
    n = len(kept_ids(c))
    assert sorted(order[:n].tolist()) == kept_ids(c)
    for val in (0.0, 1.0):
        same = [v for v in range(8) if x[v] == val]
        got = [v for v in same if c.kept[v]]
        assert got == same[: len(got)]
    assert c.undecidable == []     # duplicates of the cut's value are decided exactly
    # a cut that falls inside a run of duplicates: four tokens of q = 0.25 each, tau = 0.6 -> three of them (0.5 < 0.6 <= 0.75)
    assert kept_ids(R.truncate_row(np.array([1.0, 1.0, -INF, 1.0, 1.0], dtype=np.float32), 1, 0.6)) == [0, 1, 3]


def test_min_p_of_one_keeps_every_maximal_token():
    x = np.array([0.5, 3.0, -1.0, 3.0, 2.9999, 3.0], dtype=np.float32)
    for T in (0.7, 1.0, 1.3):
        assert kept_ids(R.truncate_row(x, 2, 1.0, T)) == [1, 3, 5]
    assert kept_ids(R.truncate_row(x, 2, 0.9)) == [1, 3, 4, 5]
    # eta and epsilon keep only the LOWEST-index maximum when nothing reaches the threshold
    y = np.zeros(10, dtype=np.float32)
    assert kept_ids(R.truncate_row(y, 4, 0.5)) == [0]


def test_a_row_with_banned_entries():
    x = np.array([-INF, 1.0, -INF, 1.0, 0.0, -INF], dtype=np.float32)
    for kind, value in ((1, 1.0), (2, 0.01), (3, 1e-3), (4, 1e-3)):
        c = R.truncate_row(x, kind, value)
        assert kept_ids(c) == [1, 3, 4], kind          # -inf stays dropped and weighs nothing
        z = 2 * math.e + 1
        assert abs(c.H - (math.log(z) - 2 * math.e / z)) < 1e-12
        assert np.isfinite(c.H)
    none = R.truncate_row(np.full(5, -INF, dtype=np.float32), 1, 0.9)
    assert kept_ids(none) == [] and none.H == 0.0
    out, ent, kept, und = R.edit_rows(np.array([[0.0, 5.0, 0.0, 9.0], [np.nan, np.nan, np.nan, 7.0]], dtype=np.float32), 3, 2, 0.5, 1.0,
                                      last_pred=[0, END], end=END)
    assert out[0].tolist() == [-INF, 5.0, -INF, 9.0] and kept.tolist() == [1, 0]     # the pad column is not touched
    assert np.isnan(out[1, :3]).all() and ent[1] == 0.0                            # an ended row comes back as it was


def test_undecidable_tokens_are_reported():
    # two tokens whose probabilities straddle epsilon by less than the band
    eps = 0.25
    x = np.log(np.array([0.5, 0.25 * (1 + 5e-6), 0.25 * (1 - 5e-6)])).astype(np.float32)
    c = R.truncate_row(x, 4, eps)
    assert set(c.undecidable) == {1, 2}
    far = R.truncate_row(np.log(np.array([0.5, 0.3, 0.2])).astype(np.float32), 4, eps)
    assert far.undecidable == [] and kept_ids(far) == [0, 1]
    # typical: a mass ahead within 1e-6 of tau
    c = R.truncate_row(np.zeros(4, dtype=np.float32), 1, 0.5)
    assert 2 in c.undecidable


# ---- the classes and the config keys --------------------------------------------------------------------------------------------------------
def test_truncation_classes_check_their_arguments():
    S = sampling
    assert (S.TypicalTruncation().kind, S.TypicalTruncation().value) == (1, 0.9)
    assert (S.MinPTruncation().kind, S.MinPTruncation().value) == (2, 0.05)
    assert (S.EtaTruncation().kind, S.EtaTruncation().value) == (3, 3e-4)
    assert (S.EpsilonTruncation().kind, S.EpsilonTruncation().value) == (4, 3e-4)
    assert not S.Truncation().active and S.Truncation(0, 7.0).kind == 0 and S.TypicalTruncation(1.0).active
    assert S.MinPTruncation(1.0).value == 1.0
    for make, bad in ((S.TypicalTruncation, (0.0, -0.1, 1.0001, math.nan, INF)), (S.MinPTruncation, (0.0, 1.5, math.nan)),
                      (S.EtaTruncation, (0.0, 1.0, -1.0, math.nan)), (S.EpsilonTruncation, (0.0, 1.0, 2.0, math.nan))):
        for v in bad:
            with pytest.raises(ValueError, match="truncation needs"):
                make(v)
    for kind in (-1, 5, 1.5, True):
        with pytest.raises(ValueError, match="kind"):
            S.Truncation(kind, 0.5)
    with pytest.raises(ValueError, match="number"):
        S.Truncation(1, "much")
    d = S.TypicalTruncation(0.75).desc()
    assert (d.kind, d.value) == (1, 0.75) and not d.entropy and not d.kept
    assert isinstance(S.truncation_from_name("Min-P", 0.1), S.MinPTruncation) and S.truncation_from_name("none") is None
    with pytest.raises(ValueError, match="one of none"):
        S.truncation_from_name("top-a")


TOPP = ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", 0.95, "MODEL.BEAM_SIZE", 1]


def test_config_defaults_are_off():
    c = Config()
    assert (c.MODEL.SAMPLER_TRUNCATION, c.MODEL.SAMPLER_TRUNCATION_VALUE) == ("none", 0.0)
    assert sampling.truncation_from_config(c.MODEL) is None
    assert sampling.truncation_from_config(Config(config_override=TOPP).MODEL) is None
    # a value alone selects nothing
    assert sampling.truncation_from_config(Config(config_override=TOPP + ["MODEL.SAMPLER_TRUNCATION_VALUE", 0.5]).MODEL) is None


@pytest.mark.parametrize("name,cls,default", [("typical", "TypicalTruncation", 0.9), ("min-p", "MinPTruncation", 0.05),
                                              ("eta", "EtaTruncation", 3e-4), ("epsilon", "EpsilonTruncation", 3e-4)])
def test_each_kind_is_read_from_the_keys_and_needs_a_word_sampler(name, cls, default):
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_TRUNCATION", name])
    t = sampling.truncation_from_config(c.MODEL)
    assert type(t).__name__ == cls and t.value == default and t.kind == sampling.TRUNCATION_KINDS[name]
    assert isinstance(sampling.from_config(c.MODEL), sampling.TopPSampler)      # the sampler's own keys are read as before
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_TRUNCATION", name, "MODEL.SAMPLER_TRUNCATION_VALUE", 0.25])
    assert sampling.truncation_from_config(c.MODEL).value == 0.25
    for other, match in (([], "needs MODEL.DECODE_SAMPLER"), (["MODEL.STOCHASTIC_BEAM_SEARCH", True], "needs MODEL.DECODE_SAMPLER"),
                         (["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLED_BEAM_SEARCH", True], "SAMPLED_BEAM_SEARCH exclude"),
                         (["MODEL.DIVERSE_BEAM_SEARCH", True, "MODEL.DIVERSE_BEAM_GROUPS", 1], "needs MODEL.DECODE_SAMPLER")):
        c = Config(config_override=["MODEL.SAMPLER_TRUNCATION", name] + other)
        for read in (lambda: sampling.truncation_from_config(c.MODEL), lambda: sampling.from_config(c.MODEL)):
            with pytest.raises(ValueError, match=match) as e:
                read()
            assert "MODEL.SAMPLER_TRUNCATION" in str(e.value)


@pytest.mark.parametrize("override,match", [
    (["MODEL.SAMPLER_TRUNCATION", "top-a"], "none \\| typical"), (["MODEL.SAMPLER_TRUNCATION", "typical", "MODEL.SAMPLER_TRUNCATION_VALUE", 1.5], "SAMPLER_TRUNCATION_VALUE"),
    (["MODEL.SAMPLER_TRUNCATION", "eta", "MODEL.SAMPLER_TRUNCATION_VALUE", 1.0], "SAMPLER_TRUNCATION_VALUE"),
    (["MODEL.SAMPLER_TRUNCATION", "min-p", "MODEL.SAMPLER_TRUNCATION_VALUE", -0.1], "SAMPLER_TRUNCATION_VALUE"),
    (["MODEL.SAMPLER_TRUNCATION", "epsilon", "MODEL.SAMPLER_TRUNCATION_VALUE", "nan"], "SAMPLER_TRUNCATION_VALUE"),
])
def test_config_validation(override, match):
    override = [float(v) if v == "nan" else v for v in override]
    with pytest.raises(ValueError, match=match):
        Config(config_override=TOPP + override)
    Config(config_override=TOPP + ["MODEL.SAMPLER_TRUNCATION", "typical", "MODEL.SAMPLER_TRUNCATION_VALUE", 1.0])


def test_a_model_reads_the_keys_with_a_word_sampler_only():
    from var_updown.models import UpDownCaptioner
    small = ["MODEL.IMAGE_FEATURE_SIZE", 8, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
             "MODEL.Z_SPACE", 4]
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_TRUNCATION", "min-p"] + small)
    vocab = Vocabulary.synthetic(40)
    m = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu")     # (scripts/train.py: no sampler, the keys are not read)
    assert m._truncation is None
    with pytest.raises(ValueError, match="needs a word sampler"):
        m.truncation(sampling.TypicalTruncation())
    m.truncation(None)
    s = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu", sampler=sampling.from_config(c.MODEL))
    assert isinstance(s._truncation, sampling.MinPTruncation)
    s.truncation(sampling.Truncation())            # inactive: off
    assert s._truncation is None
    s.truncation(sampling.EtaTruncation(0.01))
    assert s._truncation.kind == 3
    with pytest.raises(ValueError, match="Truncation or None"):
        s.truncation(sampling.LogitRules())


# ---- the struct and the bindings against the header ---------------------------------------------------------------------------------------
def test_bindings_mirror_the_header():
    assert struct_fields("ssc_truncation") == [f for f, _ in L.Truncation._fields_] == ["kind", "value", "entropy", "kept"]
    assert C.sizeof(L.Truncation) == 24
    for name in ("ssc_truncate_rows", "ssc_decode_sample_opts_workspace_bytes", "ssc_decode_sample_opts"):
        assert name in L.SYMBOLS and name + "(" in header()
    assert len(L.SYMBOLS["ssc_truncate_rows"][1]) == 9
    # the truncation is the fourth field of the sampled decode's options (the size and four pointers)
    assert struct_fields("ssc_sample_opts") == [f for f, _ in L.SampleOpts._fields_] and C.sizeof(L.SampleOpts) == 5 * C.sizeof(C.c_void_p)
    assert L.SampleOpts._fields_[3] == ("trunc", C.POINTER(L.Truncation))
    assert L.SYMBOLS["ssc_truncate_rows"][1][5] is C.c_float
    assert L.load().ssc_version() == 4
    # the pinned structs keep their sizes
    assert (C.sizeof(L.SamplerDesc), C.sizeof(L.LogitRules)) == (24, 80)


# ---- refusals, without a GPU ------------------------------------------------------------------------------------------------------------
BAD_VALUES = [(1, 0.0), (1, -0.5), (1, 1.0001), (1, math.nan), (1, INF), (2, 0.0), (2, 1.5), (2, math.nan), (3, 0.0), (3, 1.0),
              (3, math.nan), (3, -1e-3), (4, 0.0), (4, 1.0), (4, 2.0), (4, math.nan), (-1, 0.5), (5, 0.5), (99, 0.5)]
GOOD_VALUES = [(1, 0.9), (1, 1.0), (2, 1.0), (2, 1e-3), (3, 3e-4), (4, 0.999)]


def trunc(kind=1, value=0.9, entropy=None, kept=None):
    return L.Truncation(kind, value, entropy, kept)


def test_rows_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    V = 50

    def call(t, logits=a, ld=V, rows=3, V=V, T=1.0, last=a, end=END):
        return lib._raw_ssc_truncate_rows(logits, ld, rows, V, C.byref(t) if t is not None else None, T, last, end, None)

    assert call(trunc(0, 0.0)) == 0 and call(trunc(0, math.nan), last=None, end=-7) == 0    # off: SSC_OK with no launch
    for k, v in GOOD_VALUES:
        assert call(trunc(k, v), rows=0) == 0                                              # nothing to edit
    assert call(None) == -1 and call(trunc(), logits=None) == -1
    for kw in (dict(ld=49), dict(rows=-1), dict(V=0), dict(end=-1), dict(end=50), dict(T=0.0), dict(T=-1.0), dict(T=INF),
               dict(T=math.nan)):
        assert call(trunc(), **kw) == -1, kw
        assert call(trunc(0, 0.0), **kw) == -1, kw       # (what does not depend on the kind is refused with it off as well)
    for k, v in BAD_VALUES:
        assert call(trunc(k, v)) == -1, (k, v)
        assert call(trunc(k, v), rows=0) == -1, (k, v)
    # alignment: a pointer that is no multiple of 4
    assert call(trunc(), logits=a + 2) == -2 and call(trunc(), last=a + 1) == -2
    assert call(trunc(entropy=a + 2)) == -2 and call(trunc(kept=a + 3)) == -2 and call(trunc(0, 0.0, kept=a + 1)) == -2
    assert call(trunc(5, 0.5, entropy=a + 2)) == -1      # SSC_EINVAL comes first


def test_decode_refuses_a_bad_truncation_before_any_launch_and_costs_no_workspace():
    """A descriptor that passes every check with a workspace one byte short: SSC_EWORKSPACE (-4) without a truncation, with kind 0 and
    with good ones - they were accepted, nothing was launched -, SSC_EINVAL / SSC_EALIGN for every bad one whatever the workspace.
    The workspace is that of ssc_decode_sample."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    d = search_desc(a, beam=1, per_node=1)
    n = lib.ssc_decode_sample_opts_workspace_bytes(C.byref(cfg), C.byref(d), C.byref(sample_opts(trunc=trunc())))
    assert n > 0 and n == lib.ssc_decode_sample_workspace_bytes(C.byref(cfg), C.byref(d))
    p = L.Params()
    c, dd = C.byref(cfg), C.byref(d)

    def call(t, nbytes, smp=None, rules=None, guide=None):
        smp = smp or L.SamplerDesc(0, 0, 1.0, 1.0, 3)
        return lib._raw_ssc_decode_sample_opts(c, C.byref(p), dd, C.byref(smp), C.byref(sample_opts(guide, rules, t)), a, nbytes, None)

    assert call(None, n - 1) == -4 and call(trunc(0, 0.0), n - 1) == -4
    for k, v in GOOD_VALUES:
        assert call(trunc(k, v), n - 1) == -4 and call(trunc(k, v, a, a), n - 1) == -4
    for k, v in BAD_VALUES:
        assert call(trunc(k, v), n - 1) == -1 and call(trunc(k, v), n) == -1, (k, v)
    assert call(trunc(entropy=a + 2), n) == -2 and call(trunc(kept=a + 1), n) == -2
    # everything the call refuses without a truncation stays refused: a bad sampler, bad rules, a bad guide, a bad descriptor
    assert call(trunc(), n, smp=L.SamplerDesc(0, 0, 1.0, 0.0, 3)) == -1       # temperature 0
    assert call(trunc(), n, smp=L.SamplerDesc(3, 0, 1.0, 1.0, 3)) == -1       # sampler kind 3 does not exist
    bad_rules = L.LogitRules()
    bad_rules.repetition_penalty = 0.0
    assert call(trunc(), n, rules=bad_rules) == -1
    good_rules = L.LogitRules()
    good_rules.no_repeat_ngram, good_rules.repetition_penalty = 2, 1.3
    assert call(trunc(), n - 1, rules=good_rules) == -4
    assert call(trunc(), n, guide=L.LatentGuideDesc(0, a, a, 4, a)) == -1
    assert call(trunc(), n - 1, guide=L.LatentGuideDesc(3, a, a, 4, a)) == -4
    d.feats = None
    assert call(trunc(), n) == -1
    d.feats = a
    d.beam = 2
    assert call(trunc(), n) == -1
    d.beam = 1
    assert CFG["V"] == 50


# ---- the runtime --------------------------------------------------------------------------------------------------------------------------
def dims(**kw):
    base = dict(V=50, E=8, H=8, A=8, F=8, Z=4, S=0, kld_mode=0, pm_scale=0.0, prior_var=1.0)
    base.update(kw)
    return ModelDims(**base)


def test_diverse_decode_takes_a_truncation_with_a_word_sampler_only():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    feats = torch.zeros(2, 3, 8)
    tr = sampling.TypicalTruncation(0.9)
    base = dict(n_samples=3, max_steps=6, boundary_index=1, truncation=tr)
    for kw, name in ((dict(beam=2), "not the beam search"),
                     (dict(beam=2, sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                     (dict(beam=2, sampler=sampling.TopKSampler(k=5), sampled_beam=True), "sampled-node beam search"),
                     (dict(beam=2, diverse_beam=sampling.DiverseBeam(2, 0.5)), "diverse beam search"),
                     (dict(beam=2, rules=sampling.DecodeRules(2, 0, 1.0, ())), "beam search under decode rules")):
        with pytest.raises(ValueError, match="truncation belongs to the word samplers.*" + name):
            diverse_decode(dec, feats, None, **base, **kw)
    with pytest.raises(NotImplementedError, match="truncation.*ensemble"):
        diverse_decode(EnsembleDecodeEngine([dec]), feats, None, beam=1, sampler=sampling.TopKSampler(k=5), **base)
    # an inactive truncation is no truncation: the beam search's own refusal of a word sampler at beam 2 is what is left
    with pytest.raises(ValueError, match="beam must be 1"):
        diverse_decode(dec, feats, None, 3, 2, 6, 1, sampler=sampling.TopKSampler(k=5), truncation=sampling.Truncation())
    with pytest.raises(ValueError, match="truncation_stats needs an active truncation"):
        dec.sample(None, None, 3, 6, 1, None, None, sampling.TopKSampler(k=5), 1, truncation_stats=True)


# ---- the script's refusals ----------------------------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script_truncation", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_checks_the_truncation_flag(tmp_path):
    mod = script_module()
    args = lambda *a: mod.parser.parse_args(BASE + list(a))
    assert mod.check_truncation_args(args()) is None
    assert mod.check_truncation_args(args("--truncation", "none")) is None
    t = mod.check_truncation_args(args("--truncation", "typical:0.9"))
    assert isinstance(t, sampling.TypicalTruncation) and t.value == 0.9
    assert mod.check_truncation_args(args("--truncation", "eta")).value == 3e-4
    for flag, msg in (("typical:1.5", "value in \\(0, 1\\]"), ("top-a:0.5", "one of none"), ("epsilon:1", "epsilon in \\(0, 1\\)")):
        with pytest.raises(SystemExit, match=msg):
            mod.check_truncation_args(args("--truncation", flag))
    with pytest.raises((SystemExit, ValueError)):
        mod.check_truncation_args(args("--truncation", "typical:much"))
    f = tmp_path / "ck.pt"
    f.write_text("")
    with pytest.raises(SystemExit, match="not available with --ensemble-checkpoints"):
        mod.check_truncation_args(args("--truncation", "min-p:0.1", "--checkpoint-path", str(f), "--ensemble-checkpoints", str(f)))
    for override in ([], ["MODEL.STOCHASTIC_BEAM_SEARCH", True], ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", True]):
        with pytest.raises(SystemExit, match="needs a word sampler"):
            mod.check_truncation_args(args("--truncation", "typical:0.9"), Config(config_override=override).MODEL)
    assert mod.check_truncation_args(args("--truncation", "typical:0.9"), Config(config_override=TOPP).MODEL).kind == 1
