"""CPU: the logit rules of the word samplers (include/ssc.h: ssc_logit_rules) - the restatement (tests/logitrulesref.py) on hand cases
and against an independently written implementation of the same formulas, the struct and the bindings against the header, every
refusal of the three new symbols (no launch is reached: no GPU needed), the workspace size, the config keys and their refusals, the
runtime's refusals and those of scripts/inference.py."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import logitrulesref as R
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
F = np.float32
INF = float("inf")


# ---- the restatement on hand cases ----------------------------------------------------------------------------------------------------
def row(V=8, fill=1.0):
    return np.full(V, fill, dtype=np.float32)


def bans(x):
    return sorted(int(v) for v in np.nonzero(np.isneginf(x))[0])


def test_a_repeated_bigram_is_banned():
    # history a b c a b a: the bigrams that start with the last token a are (a, b) twice - b is banned; c, a and END are not
    out = R.edit_row(row(), 8, [2, 3, 4, 2, 3, 2], R.Rules(no_repeat_ngram=2), END)
    assert bans(out) == [3]
    # ... and after a b c a b: (b, c) occurred - c is banned
    assert bans(R.edit_row(row(), 8, [2, 3, 4, 2, 3], R.Rules(no_repeat_ngram=2), END)) == [4]
    # a trigram needs both of its first two tokens to match
    assert bans(R.edit_row(row(), 8, [2, 3, 4, 5, 3, 4], R.Rules(no_repeat_ngram=3), END)) == [5]
    assert bans(R.edit_row(row(), 8, [2, 3, 4, 5, 6, 4], R.Rules(no_repeat_ngram=3), END)) == []


def test_unigram_blocking_bans_every_used_word_but_never_end():
    out = R.edit_row(row(), 8, [5, 2, 5, END, 7], R.Rules(no_repeat_ngram=1), END)   # (a stand-alone history may hold an END inside)
    assert bans(out) == [2, 5, 7]


def test_a_history_shorter_than_the_prefix_bans_nothing():
    for hist in ([], [2], [2, 2]):
        assert bans(R.edit_row(row(), 8, hist, R.Rules(no_repeat_ngram=4), END)) == []
    assert bans(R.edit_row(row(), 8, [2, 2, 2], R.Rules(no_repeat_ngram=4), END)) == []   # n - 1 tokens: still no 4-gram to repeat
    assert bans(R.edit_row(row(), 8, [2, 2, 2, 2], R.Rules(no_repeat_ngram=4), END)) == [2]


def test_end_is_banned_below_the_minimum_length_only():
    r = R.Rules(min_length=3)
    assert bans(R.edit_row(row(), 8, [], r, END)) == [END]
    assert bans(R.edit_row(row(), 8, [4, 5], r, END)) == [END]
    assert bans(R.edit_row(row(), 8, [4, 5, 6], r, END)) == []


def test_repetition_penalty_divides_positive_and_multiplies_the_rest():
    x = np.array([0.0, 9.0, 3.0, -2.0, -0.0, 5.0], dtype=np.float32)
    out = R.edit_row(x, 6, [0, 2, 3, 4], R.Rules(repetition_penalty=1.5), 1)
    assert out[0] == 0.0 and not np.signbit(out[0])          # a logit of exactly 0 is "not positive": 0 * theta = 0
    assert out[2] == F(F(3.0) / F(1.5))
    assert out[3] == F(F(-2.0) * F(1.5))                     # a negative logit moves AWAY from zero
    assert out[4] == 0.0 and np.signbit(out[4])
    assert out[5] == F(5.0) and out[1] == F(9.0)             # words outside the history are untouched
    # theta < 1 rewards repetition
    assert R.edit_row(x, 6, [2], R.Rules(repetition_penalty=0.5), 1)[2] == F(6.0)


def test_presence_counts_once_and_frequency_per_occurrence():
    x = row(8, 2.0)
    out = R.edit_row(x, 8, [3, 5, 3, 3], R.Rules(presence_penalty=0.5, frequency_penalty=0.25), END)
    assert out[3] == F(F(2.0) - F(F(0.5) + F(F(0.25) * F(3.0))))   # a token three times
    assert out[5] == F(F(2.0) - F(F(0.5) + F(0.25)))
    assert out[2] == F(2.0)
    # theta first, then the subtraction
    both = R.edit_row(x, 8, [3, 3, 3], R.Rules(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25), END)
    assert both[3] == F(F(F(2.0) / F(1.3)) - F(F(0.5) + F(F(0.25) * F(3.0))))


def test_a_bias_of_minus_infinity_is_a_ban_and_rows_pick_their_bias():
    bias = np.zeros((2, 8), dtype=np.float32)
    bias[0, 4] = -INF
    bias[0, 5] = 0.75
    bias[1, 6] = -1.0
    r = R.Rules(bias=bias, bias_row=[0, 1, -1, 2], repetition_penalty=1.3, presence_penalty=0.2)
    x = row(8, 1.0)
    o0 = R.edit_row(x, 8, [4, 5], r, END, row=0)
    assert bans(o0) == [4]                                   # -inf stays -inf under the penalties
    assert o0[5] == F(F(F(1.75) / F(1.3)) - F(0.2))          # bias first, then the penalties on the biased logit
    o1 = R.edit_row(x, 8, [], r, END, row=1)
    assert o1[6] == F(0.0) and o1[4] == F(1.0)
    for k in (2, 3):                                         # an index outside [0, n_bias): no bias for that row
        assert np.array_equal(R.edit_row(x, 8, [], r, END, row=k), x)
    assert R.banned(8, [4, 5], r, END, row=0) == {4}


def test_ended_rows_pad_columns_and_foreign_ids():
    x = np.arange(10, dtype=np.float32)
    r = R.Rules(no_repeat_ngram=1, min_length=9, suppress=(0,), repetition_penalty=2.0, bias=np.ones((1, 8), dtype=np.float32))
    assert np.array_equal(R.edit_row(x, 8, [3, END], r, END), x)        # last token END: neither read nor written
    out = R.edit_row(x, 8, [3, 99, -4, 3], r, END)                      # ids outside [0, V) are skipped
    assert np.array_equal(out[8:], x[8:])                               # columns V .. ld - 1 are never touched
    assert bans(out) == [0, END, 3]
    # off: nothing changes
    assert np.array_equal(R.edit_row(x, 8, [3, 4], R.Rules(), END), x)


# ---- the restatement against an independent implementation ---------------------------------------------------------------------------------
def independent(x, V, hist, r, end, k):
    """The same three stages written another way: counts through np.unique, the n-gram rule through tuples of the history's windows."""
    x = x.copy()
    t = len(hist)
    if t and hist[-1] == end:
        return x
    if r.bias is not None:
        br = 0 if r.bias_row is None else r.bias_row[k]
        if 0 <= br < len(r.bias):
            x[:V] = (x[:V].astype(np.float32) + r.bias[br][:V]).astype(np.float32)
    ids, counts = np.unique(np.array([h for h in hist if 0 <= h < V], dtype=np.int64), return_counts=True)
    for c, n in zip(ids, counts):
        scaled = np.float32(x[c]) / r.repetition_penalty if x[c] > 0 else np.float32(x[c]) * r.repetition_penalty
        x[c] = np.float32(scaled) - np.float32(r.presence_penalty + np.float32(r.frequency_penalty * np.float32(n)))
    x[list(r.suppress)] = -np.inf
    if t < r.min_length:
        x[end] = -np.inf
    n = r.no_repeat_ngram
    if n >= 1 and t >= n:
        prefix = tuple(hist[t - n + 1:]) if n > 1 else ()
        for j in range(t - n + 1):
            if tuple(hist[j:j + n - 1]) == prefix:
                v = hist[j + n - 1]
                if v != end and 0 <= v < V:
                    x[v] = -np.inf
    return x


def test_restatement_against_an_independent_implementation():
    rng = np.random.default_rng(11)
    with np.errstate(all="ignore"):
        for case in range(300):
            V = int(rng.integers(6, 40))
            ld = V + int(rng.integers(0, 3))
            t = int(rng.integers(0, 12))
            alphabet = rng.choice(V, size=min(V, int(rng.integers(2, 5))), replace=False)
            hist = [int(v) for v in rng.choice(alphabet, size=t)]
            if t and rng.random() < 0.1:
                hist[int(rng.integers(0, t))] = int(rng.choice([-3, V, V + 7]))
            sup = tuple(int(v) for v in rng.choice([v for v in range(V) if v != END], size=int(rng.integers(0, 3)), replace=False))
            bias = None
            if rng.random() < 0.5:
                bias = rng.standard_normal((2, V)).astype(np.float32)
                bias[rng.random((2, V)) < 0.1] = -np.inf
            r = R.Rules(int(rng.integers(0, 5)), int(rng.integers(0, 8)), sup, float(rng.choice([1.0, 1.3, 0.7])),
                        float(rng.choice([0.0, 0.5])), float(rng.choice([0.0, 0.25])), bias, [1, 0, 5][: 3])
            x = (rng.standard_normal(ld) * 3).astype(np.float32)
            x[rng.random(ld) < 0.1] = 0.0
            k = int(rng.integers(0, 3))
            got, want = R.edit_row(x, V, hist, r, END, row=k), independent(x, V, hist, r, END, k)
            assert got.tobytes() == want.tobytes(), (case, hist, vars(r))
            assert R.banned(V, hist, r, END, row=k) <= set(bans(got)) or (t and hist[-1] == END)


# ---- the struct and the bindings against the header -------------------------------------------------------------------------------------
def test_bindings_mirror_the_header():
    declared = [re.sub(r"\[.*\]", "", f) for f in struct_fields("ssc_logit_rules")]   # (suppress[SSC_RULES_MAX_SUPPRESS])
    assert declared == [f for f, _ in L.LogitRules._fields_]
    assert L.LogitRules._fields_[3][1]._length_ == L.SSC_RULES_MAX_SUPPRESS == 8
    assert C.sizeof(L.LogitRules) == 80
    r = L.LogitRules()
    assert not r.bias and not r.bias_row and r.no_repeat_ngram == 0
    for name in ("ssc_logit_rules_rows", "ssc_decode_sample_opts_workspace_bytes", "ssc_decode_sample_opts"):
        assert name in L.SYMBOLS and name + "(" in header()
    assert len(L.SYMBOLS["ssc_logit_rules_rows"][1]) == 10
    # the rules are the third field of the sampled decode's options (the size and four pointers)
    assert struct_fields("ssc_sample_opts") == [f for f, _ in L.SampleOpts._fields_] and C.sizeof(L.SampleOpts) == 5 * C.sizeof(C.c_void_p)
    assert L.SampleOpts._fields_[2] == ("rules", C.POINTER(L.LogitRules))
    assert L.load().ssc_version() == 4
    # the pinned structs keep their sizes
    assert (C.sizeof(L.SamplerDesc), C.sizeof(L.RulesDesc)) == (24, 12 + 4 * 8 + 4 * 64)


# ---- refusals, without a GPU --------------------------------------------------------------------------------------------------------------
def rules_desc(a=None, **kw):
    r = L.LogitRules()
    r.no_repeat_ngram, r.min_length, r.repetition_penalty = 2, 1, 1.3
    if a is not None:
        r.bias, r.ld_bias, r.n_bias, r.bias_row = a, 50, 2, a
    for k, v in kw.items():
        if k == "suppress":
            r.n_suppress = len(v)
            for i, s in enumerate(v[: L.SSC_RULES_MAX_SUPPRESS]):
                r.suppress[i] = s
        else:
            setattr(r, k, v)
    return r


BAD_FIELDS = [dict(no_repeat_ngram=-1), dict(no_repeat_ngram=65), dict(min_length=-1), dict(n_suppress=-1), dict(n_suppress=9),
              dict(suppress=(50,)), dict(suppress=(-1,)), dict(suppress=(END,)), dict(repetition_penalty=0.0),
              dict(repetition_penalty=-1.0), dict(repetition_penalty=INF), dict(repetition_penalty=math.nan),
              dict(presence_penalty=INF), dict(presence_penalty=math.nan), dict(frequency_penalty=-INF),
              dict(frequency_penalty=math.nan)]
BAD_BIAS = [dict(ld_bias=49), dict(n_bias=0), dict(n_bias=-2)]


def test_rows_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    V = 50

    def call(r, logits=a, ld=V, rows=3, V=V, hist=a, ld_hist=3, t=2, end=END):
        return lib._raw_ssc_logit_rules_rows(logits, ld, rows, V, C.byref(r) if r is not None else None, hist, ld_hist, t, end, None)

    off = L.LogitRules()
    off.repetition_penalty = 1.0
    assert call(off) == 0                        # every control off and no bias: SSC_OK with no launch
    assert call(rules_desc(), rows=0) == 0       # nothing to edit
    assert call(None) == -1 and call(rules_desc(), logits=None) == -1
    assert call(rules_desc(), hist=None) == -1   # a history is needed from step 1 on
    for kw in (dict(ld=49), dict(ld_hist=2), dict(t=-1), dict(t=64), dict(rows=-1), dict(V=0), dict(end=-1), dict(end=50)):
        assert call(rules_desc(), **kw) == -1, kw
    for kw in BAD_FIELDS:
        assert call(rules_desc(**kw)) == -1, kw
        assert call(rules_desc(a, **kw)) == -1, kw
    for kw in BAD_BIAS:
        assert call(rules_desc(a, **kw)) == -1, kw
    # V > t + n_suppress + 1: the rules alone cannot empty a row
    assert call(rules_desc(), V=3, ld=3, t=2, end=1) == -1
    assert call(rules_desc(suppress=(2, 3)), V=12, ld=12, t=9) == -1
    # alignment: a pointer that is no multiple of 4
    for kw in (dict(logits=a + 2), dict(hist=a + 1)):
        assert call(rules_desc(), **kw) == -2, kw
    assert call(rules_desc(a, bias=a + 2)) == -2 and call(rules_desc(a, bias_row=a + 3)) == -2


def sample_rules_call(lib, a):
    smp = L.SamplerDesc(0, 0, 1.0, 1.0, 3)
    p = L.Params()
    return lambda c, d, r, g, n: lib._raw_ssc_decode_sample_opts(c, C.byref(p), d, C.byref(smp), C.byref(sample_opts(guide=g, rules=r)), a,
                                                                 n, None)


def test_decode_refuses_bad_rules_before_any_launch_and_costs_no_workspace():
    """A descriptor that passes every check with a workspace one byte short: SSC_EWORKSPACE (-4) without rules, with inactive ones
    and with good ones - the rules were accepted, nothing was launched -, SSC_EINVAL / SSC_EALIGN for every bad one whatever the
    workspace.  The workspace is that of ssc_decode_sample."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    d = search_desc(a, beam=1, per_node=1)
    n = lib.ssc_decode_sample_opts_workspace_bytes(C.byref(cfg), C.byref(d), C.byref(sample_opts(rules=rules_desc())))
    assert n > 0 and n == lib.ssc_decode_sample_workspace_bytes(C.byref(cfg), C.byref(d))
    call = sample_rules_call(lib, a)
    c, dd = C.byref(cfg), C.byref(d)
    assert call(c, dd, None, None, n - 1) == -4
    off = L.LogitRules()
    off.repetition_penalty = 1.0
    for good in (off, rules_desc(), rules_desc(a), rules_desc(a, bias_row=None), rules_desc(suppress=(0, 2, 3))):
        assert call(c, dd, good, None, n - 1) == -4
    for kw in BAD_FIELDS:
        for r in (rules_desc(**kw), rules_desc(a, **kw)):
            assert call(c, dd, r, None, n - 1) == -1, kw
            assert call(c, dd, r, None, n) == -1, kw
    for kw in BAD_BIAS:
        assert call(c, dd, rules_desc(a, **kw), None, n) == -1, kw
    assert call(c, dd, rules_desc(a, bias=a + 2), None, n) == -2
    assert call(c, dd, rules_desc(a, bias_row=a + 1), None, n) == -2
    # active rules: at most SSC_RULES_MAX_LEN steps, and a vocabulary the rules alone cannot empty
    d.max_steps = 65
    assert call(c, dd, rules_desc(), None, 1 << 40) == -1
    assert call(c, dd, off, None, 0) == -4            # inactive rules do not limit the steps
    d.max_steps = 46
    assert call(c, dd, rules_desc(suppress=(0, 2, 3, 4)), None, 1 << 40) == -1    # V = 50 <= 46 + 4
    assert call(c, dd, rules_desc(suppress=(0, 2, 3)), None, 0) == -4
    d.max_steps = 6
    # what the unruled call refuses stays refused
    d.feats = None
    assert call(c, dd, rules_desc(), None, n) == -1
    d.feats = a
    d.beam = 2
    assert call(c, dd, rules_desc(), None, n) == -1
    d.beam = 1
    bad_guide = L.LatentGuideDesc(0, a, a, 4, a)
    assert call(c, dd, rules_desc(), bad_guide, n) == -1
    assert call(c, dd, rules_desc(), L.LatentGuideDesc(3, a, a, 4, a), n - 1) == -4
    assert CFG["V"] == 50


# ---- the runtime --------------------------------------------------------------------------------------------------------------------------
def test_logit_rules_class_checks_its_arguments():
    LR = sampling.LogitRules
    assert not LR().active and LR(min_length=1).active and LR(suppress=(3,)).active and LR(frequency_penalty=0.1).active
    assert LR(repetition_penalty=1.2).active and LR(presence_penalty=-0.5).active and LR(no_repeat_ngram=3).active
    for kw, msg in ((dict(no_repeat_ngram=65), "no_repeat_ngram"), (dict(no_repeat_ngram=-1), "no_repeat_ngram"),
                    (dict(no_repeat_ngram=True), "no_repeat_ngram"), (dict(min_length=-1), "min_length"),
                    (dict(suppress=range(9)), "at most 8"), (dict(suppress=(2, 2)), "distinct"), (dict(suppress=(-1,)), "distinct"),
                    (dict(repetition_penalty=0), "positive"), (dict(repetition_penalty=-2.0), "positive"),
                    (dict(repetition_penalty=INF), "finite"), (dict(presence_penalty=math.nan), "finite"),
                    (dict(frequency_penalty=1e39), "finite"), (dict(bias=np.zeros(4)), "float32 tensor"),
                    (dict(bias=torch.zeros(4, dtype=torch.float64)), "float32 tensor"), (dict(bias=torch.zeros(2, 2, 2)), "float32 tensor")):
        with pytest.raises(ValueError, match=msg):
            LR(**kw)
    r = LR(no_repeat_ngram=2, min_length=3, suppress=(0, 5))
    r.check(50, END, 20, 4)
    for args, msg in (((50, END, 65, 4), "at most 64 steps"), ((5, END, 4, 4), "suppressed token"), ((50, 5, 20, 4), "boundary token"),
                      ((22, END, 20, 4), "must not empty a row")):
        with pytest.raises(ValueError, match=msg):
            r.check(*args)
    LR().check(5, 5, 1000, 1)   # inactive rules limit nothing
    d, keep = r.desc(3)
    assert (d.no_repeat_ngram, d.min_length, d.n_suppress, list(d.suppress)[:2]) == (2, 3, 2, [0, 5])
    assert d.repetition_penalty == 1.0 and not d.bias and not d.bias_row and keep == []
    b = LR(bias=torch.zeros(7))
    assert b.active and tuple(b.bias.shape) == (1, 7)
    with pytest.raises(ValueError, match="device tensor"):
        b.check(7, END, 3, 2)


def dims(**kw):
    base = dict(V=50, E=8, H=8, A=8, F=8, Z=4, S=0, kld_mode=0, pm_scale=0.0, prior_var=1.0)
    base.update(kw)
    return ModelDims(**base)


def test_diverse_decode_takes_logit_rules_with_a_word_sampler_only():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    feats = torch.zeros(2, 3, 8)
    lr = sampling.LogitRules(no_repeat_ngram=2)
    base = dict(n_samples=3, max_steps=6, boundary_index=1, logit_rules=lr)
    for kw in (dict(beam=2), dict(beam=2, sampler=sampling.GumbelSampler(1.0)), dict(beam=2, sampler=sampling.TopKSampler(k=5), sampled_beam=True),
               dict(beam=2, diverse_beam=sampling.DiverseBeam(2, 0.5)), dict(beam=2, rules=sampling.DecodeRules(2, 0, 1.0, ()))):
        with pytest.raises(ValueError, match="logit rules belong to the word samplers"):
            diverse_decode(dec, feats, None, **base, **kw)
    with pytest.raises(NotImplementedError, match="logit rules.*ensemble"):
        diverse_decode(EnsembleDecodeEngine([dec]), feats, None, beam=1, sampler=sampling.TopKSampler(k=5), **base)
    # rules= with a sampler keeps raising as before, with and without logit rules
    for extra in (dict(), dict(logit_rules=lr)):
        with pytest.raises(ValueError, match="decode rules belong to the deterministic beam search"):
            diverse_decode(dec, feats, None, 3, 1, 6, 1, sampler=sampling.TopKSampler(k=5), rules=sampling.DecodeRules(2, 0, 1.0, ()), **extra)


# ---- the config keys ----------------------------------------------------------------------------------------------------------------------
KEYS = ["SAMPLER_NO_REPEAT_NGRAM", "SAMPLER_MIN_LENGTH", "SAMPLER_SUPPRESS_UNKNOWN", "SAMPLER_REPETITION_PENALTY",
        "SAMPLER_PRESENCE_PENALTY", "SAMPLER_FREQUENCY_PENALTY"]
ON = {"SAMPLER_NO_REPEAT_NGRAM": 3, "SAMPLER_MIN_LENGTH": 4, "SAMPLER_SUPPRESS_UNKNOWN": True, "SAMPLER_REPETITION_PENALTY": 1.2,
      "SAMPLER_PRESENCE_PENALTY": 0.5, "SAMPLER_FREQUENCY_PENALTY": 0.25}
TOPK = ["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", 5, "MODEL.BEAM_SIZE", 1]


def test_defaults_are_off():
    c = Config()
    assert [getattr(c.MODEL, k) for k in KEYS] == [0, 0, False, 1.0, 0.0, 0.0]
    assert sampling.logit_rules_from_config(c.MODEL, Vocabulary.synthetic(20)) is None
    c = Config(config_override=TOPK)
    assert sampling.logit_rules_from_config(c.MODEL, Vocabulary.synthetic(20)) is None
    assert isinstance(sampling.from_config(c.MODEL), sampling.TopKSampler)


@pytest.mark.parametrize("key", KEYS)
def test_each_key_selects_the_rules_and_needs_a_word_sampler(key):
    c = Config(config_override=TOPK + ["MODEL." + key, ON[key]])
    r = sampling.logit_rules_from_config(c.MODEL, Vocabulary.synthetic(20))
    assert r is not None and r.active
    want = dict(no_repeat_ngram=0, min_length=0, suppress=(), repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    name = {"SAMPLER_NO_REPEAT_NGRAM": "no_repeat_ngram", "SAMPLER_MIN_LENGTH": "min_length", "SAMPLER_SUPPRESS_UNKNOWN": "suppress",
            "SAMPLER_REPETITION_PENALTY": "repetition_penalty", "SAMPLER_PRESENCE_PENALTY": "presence_penalty",
            "SAMPLER_FREQUENCY_PENALTY": "frequency_penalty"}[key]
    want[name] = (0,) if key == "SAMPLER_SUPPRESS_UNKNOWN" else ON[key]
    assert {k: getattr(r, k) for k in want} == want and r.bias is None
    assert isinstance(sampling.from_config(c.MODEL), sampling.TopKSampler)   # the sampler's own keys are read as before
    assert sampling.decode_rules_from_config(c.MODEL) is None                # ... and the beam search's rules stay off
    for other, match in (([], "needs MODEL.DECODE_SAMPLER"),
                         (["MODEL.STOCHASTIC_BEAM_SEARCH", True], "needs MODEL.DECODE_SAMPLER"),
                         (["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", True], "SAMPLED_BEAM_SEARCH exclude"),
                         (["MODEL.DIVERSE_BEAM_SEARCH", True, "MODEL.DIVERSE_BEAM_GROUPS", 1], "needs MODEL.DECODE_SAMPLER")):
        c = Config(config_override=["MODEL." + key, ON[key]] + other)
        for read in (lambda: sampling.logit_rules_from_config(c.MODEL), lambda: sampling.from_config(c.MODEL)):
            with pytest.raises(ValueError, match=match) as e:
                read()
            assert "MODEL." + key in str(e.value)   # the message names the key that asked for the rules


@pytest.mark.parametrize("override,match", [
    (["MODEL.SAMPLER_NO_REPEAT_NGRAM", 65], "SAMPLER_NO_REPEAT_NGRAM"), (["MODEL.SAMPLER_NO_REPEAT_NGRAM", -1], "SAMPLER_NO_REPEAT_NGRAM"),
    (["MODEL.SAMPLER_MIN_LENGTH", -2], "SAMPLER_MIN_LENGTH"), (["MODEL.SAMPLER_MIN_LENGTH", 20], "below DATA.MAX_CAPTION_LENGTH"),
    (["MODEL.SAMPLER_REPETITION_PENALTY", 0.0], "must be positive"), (["MODEL.SAMPLER_REPETITION_PENALTY", "inf"], "finite"),
    (["MODEL.SAMPLER_PRESENCE_PENALTY", "nan"], "finite"), (["MODEL.SAMPLER_FREQUENCY_PENALTY", "inf"], "finite"),
    (["MODEL.SAMPLER_SUPPRESS_UNKNOWN", 1], "True or False"),
    (["MODEL.SAMPLER_NO_REPEAT_NGRAM", 2, "DATA.MAX_CAPTION_LENGTH", 65], "MAX_CAPTION_LENGTH <= 64"),
])
def test_config_validation(override, match):
    override = [float(v) if v in ("inf", "nan") else v for v in override]
    with pytest.raises(ValueError, match=match):
        Config(config_override=override)


def test_a_model_without_a_sampler_never_reads_the_keys():
    """scripts/train.py builds its model without sampler=: the keys may be set in its config (with the decode's sampler) and are
    ignored; the eval forward of a beam-search model has no logit rules and refuses to be given some."""
    from var_updown.models import UpDownCaptioner
    c = Config(config_override=TOPK + ["MODEL.SAMPLER_NO_REPEAT_NGRAM", 3, "MODEL.IMAGE_FEATURE_SIZE", 8, "MODEL.EMBEDDING_SIZE", 8,
                                       "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8, "MODEL.Z_SPACE", 4])
    vocab = Vocabulary.synthetic(40)
    m = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu")
    assert m._logit_rules is None
    with pytest.raises(ValueError, match="needs a word sampler"):
        m.logit_rules(sampling.LogitRules(no_repeat_ngram=2))
    m.logit_rules(None)
    s = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu", sampler=sampling.from_config(c.MODEL))
    assert s._logit_rules is not None and s._logit_rules.no_repeat_ngram == 3
    s.logit_rules(sampling.LogitRules())          # inactive: off
    assert s._logit_rules is None
    with pytest.raises(ValueError, match="LogitRules or None"):
        s.logit_rules(sampling.DecodeRules(2, 0, 1.0, ()))
    with pytest.raises(ValueError, match="must not empty a row"):   # V = 24 <= MAX_CAPTION_LENGTH 20 + 4 suppressed
        small = UpDownCaptioner.from_config(c, vocabulary=Vocabulary.synthetic(24), device="cpu", sampler=sampling.from_config(c.MODEL))
        small.logit_rules(sampling.LogitRules(no_repeat_ngram=1, suppress=(2, 3, 4, 5)))


# ---- the script's refusals ----------------------------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script_logit_rules", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_checks_the_word_bias_flag(tmp_path):
    mod = script_module()
    f = tmp_path / "bias.json"
    f.write_text("{}")
    args = lambda *a: mod.parser.parse_args(BASE + list(a))
    mod.check_word_bias_args(args())                                   # no flag: nothing to check
    with pytest.raises(SystemExit, match="no such file"):
        mod.check_word_bias_args(args("--word-bias", str(f) + ".missing"))
    with pytest.raises(SystemExit, match="not available with --ensemble-checkpoints"):
        mod.check_word_bias_args(args("--word-bias", str(f), "--checkpoint-path", str(f), "--ensemble-checkpoints", str(f)))
    for override in ([], ["MODEL.STOCHASTIC_BEAM_SEARCH", True], ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", True]):
        with pytest.raises(SystemExit, match="needs a word sampler"):
            mod.check_word_bias_args(args("--word-bias", str(f)), Config(config_override=override).MODEL)
    mod.check_word_bias_args(args("--word-bias", str(f)), Config(config_override=TOPK).MODEL)


def test_inference_script_reads_word_bias_files(tmp_path):
    mod = script_module()
    vocab = Vocabulary.synthetic(12)
    f = tmp_path / "bias.json"
    f.write_text(json.dumps({"w3": 1.5, "w7": "-inf", "@@UNKNOWN@@": -2, "w4": "0.25"}))
    row = mod.load_word_bias(str(f), vocab)
    assert row.dtype == torch.float32 and tuple(row.shape) == (12,)
    assert row[3] == 1.5 and row[7] == -INF and row[0] == -2 and row[4] == 0.25 and int((row != 0).sum()) == 4
    for blob, msg in (('{"w3": 1, "zebra": 2}', "'zebra' is not in the vocabulary"), ('{"w3": "inf"}', "finite"), ('{"w3": "nan"}', "finite"),
                      ('{"w3": "much"}', "must be a number"), ('{"w3": null}', "must be a number"), ("{}", "non-empty"),
                      ("[1]", "non-empty"), ("{", "not JSON"), ('{"@@BOUNDARY@@": "-inf"}', "cannot be banned")):
        f.write_text(blob)
        with pytest.raises(SystemExit, match=msg):
            mod.load_word_bias(str(f), vocab)
