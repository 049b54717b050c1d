"""CPU: the decode rules of the beam search (n-gram blocking, minimum length, suppressed tokens, length penalty) - the config keys
and their exclusions, sampling.DecodeRules and its C struct, the refusals of the library that need no launch, and the numpy
restatement tests/rulesref.py against tests/dbsref.py (rules off) and against a brute-force check of its own outputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dbsref
import rulesref as R
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config
from ssc_runtime.vocab import Vocabulary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- config ------------------------------------------------------------------------------------------------------------------

def test_defaults_select_no_rules():
    c = Config()
    assert (c.MODEL.NO_REPEAT_NGRAM, c.MODEL.MIN_CAPTION_LENGTH, c.MODEL.LENGTH_PENALTY_ALPHA, c.MODEL.SUPPRESS_UNKNOWN) == (0, 0, 0.0, False)
    assert sampling.decode_rules_from_config(c.MODEL, Vocabulary.synthetic(20)) is None
    assert sampling.from_config(c.MODEL) is None
    assert not sampling.DecodeRules().active


@pytest.mark.parametrize("override,want", [
    (["MODEL.NO_REPEAT_NGRAM", "3"], (3, 0, 0.0, ())),
    (["MODEL.MIN_CAPTION_LENGTH", "5"], (0, 5, 0.0, ())),
    (["MODEL.LENGTH_PENALTY_ALPHA", "0.7"], (0, 0, 0.7, ())),
    (["MODEL.LENGTH_PENALTY_ALPHA", "1"], (0, 0, 1.0, ())),
    (["MODEL.SUPPRESS_UNKNOWN", "True"], (0, 0, 0.0, (0,))),
])
def test_any_non_default_key_selects_the_rules(override, want):
    c = Config(config_override=override)
    r = sampling.decode_rules_from_config(c.MODEL, Vocabulary.synthetic(20))
    assert r is not None and r.active
    assert (r.no_repeat_ngram, r.min_length, r.length_alpha, r.suppress) == want
    assert sampling.from_config(c.MODEL) is None   # still the deterministic beam search: no sampler


@pytest.mark.parametrize("override,match", [
    (["MODEL.NO_REPEAT_NGRAM", "65"], "NO_REPEAT_NGRAM"),
    (["MODEL.NO_REPEAT_NGRAM", "-1"], "NO_REPEAT_NGRAM"),
    (["MODEL.MIN_CAPTION_LENGTH", "-2"], "MIN_CAPTION_LENGTH"),
    (["MODEL.MIN_CAPTION_LENGTH", "20"], "MIN_CAPTION_LENGTH"),
    (["MODEL.LENGTH_PENALTY_ALPHA", "inf"], "LENGTH_PENALTY_ALPHA"),
    (["MODEL.NO_REPEAT_NGRAM", "3", "DATA.MAX_CAPTION_LENGTH", "65"], "MAX_CAPTION_LENGTH"),
])
def test_config_validation(override, match):
    if override[1] == "inf":
        override = [override[0], float("inf")]
    with pytest.raises(ValueError, match=match):
        Config(config_override=override)


@pytest.mark.parametrize("other,match", [
    (["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", "3", "MODEL.BEAM_SIZE", "1"], "DECODE_SAMPLER"),
    (["MODEL.STOCHASTIC_BEAM_SEARCH", "True"], "STOCHASTIC_BEAM_SEARCH"),
    (["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", "True"], "DECODE_SAMPLER"),
    (["MODEL.DIVERSE_BEAM_SEARCH", "True"], "DIVERSE_BEAM_SEARCH"),
    (["MODEL.USE_CBS", "True", "MODEL.EMBEDDING_SIZE", "300"], "USE_CBS"),
])
@pytest.mark.parametrize("key", [["MODEL.NO_REPEAT_NGRAM", "3"], ["MODEL.SUPPRESS_UNKNOWN", "True"]])
def test_the_rules_exclude_the_other_decodes(key, other, match):
    c = Config(config_override=key + other)
    with pytest.raises(ValueError, match=match) as e:
        sampling.from_config(c.MODEL)
    assert key[0] in str(e.value)   # the message names the key that asked for the rules


# ---- DecodeRules ---------------------------------------------------------------------------------------------------------------

def test_argument_checks():
    for kw in (dict(no_repeat_ngram=65), dict(no_repeat_ngram=-1), dict(no_repeat_ngram=1.5), dict(min_length=-1),
               dict(length_alpha=float("nan")), dict(length_alpha=float("inf")), dict(suppress=range(9)), dict(suppress=(3, 3)),
               dict(suppress=(-1,))):
        with pytest.raises(ValueError):
            sampling.DecodeRules(**kw)
    r = sampling.DecodeRules(3, 2, 1.0, (0, 7))
    r.check(50, 1, 20)
    with pytest.raises(ValueError, match="boundary"):
        sampling.DecodeRules(suppress=(1,)).check(50, 1, 20)
    with pytest.raises(ValueError, match="suppressed"):
        sampling.DecodeRules(suppress=(50,)).check(50, 1, 20)
    with pytest.raises(ValueError, match="64"):
        r.check(50, 1, 65)
    with pytest.raises(ValueError, match="finite and positive"):
        sampling.DecodeRules(length_alpha=40.0).check(50, 1, 20)   # 64 ** 40 is beyond float32


@pytest.mark.parametrize("alpha", [0.0, 0.7, 1.0, 2.0])
def test_desc_holds_the_rules_and_the_table(alpha):
    r = sampling.DecodeRules(3, 5, alpha, (0, 9))
    d = r.desc()
    assert (d.no_repeat_ngram, d.min_length, d.n_suppress) == (3, 5, 2) and list(d.suppress)[:2] == [0, 9]
    table = np.array(list(d.length_penalty), dtype=F)
    want = (np.arange(1, 65, dtype=np.float64) ** alpha).astype(F)   # float64 power, rounded to float32 once
    assert np.array_equal(table.view(np.int32), want.view(np.int32))
    assert np.array_equal(table, R.penalty_table(alpha)) and np.array_equal(table, r.table())
    if alpha == 0.0:
        assert (table == F(1)).all()
    if alpha == 1.0:
        assert np.array_equal(table, np.arange(1, 65, dtype=F))


def test_struct_layouts_match_the_header():
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    body = text[text.index("typedef struct {\n  int no_repeat_ngram;"):text.index("} ssc_rules_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:int|float)\s+(\w+)(?:\[\w+\])?;", body)
    assert fields == [f for f, _ in L.RulesDesc._fields_]
    assert re.search(r"#define SSC_RULES_MAX_LEN (\d+)", text).group(1) == str(L.SSC_RULES_MAX_LEN)
    assert re.search(r"#define SSC_RULES_MAX_SUPPRESS (\d+)", text).group(1) == str(L.SSC_RULES_MAX_SUPPRESS)
    assert C.sizeof(L.RulesDesc) == 4 * (3 + L.SSC_RULES_MAX_SUPPRESS + L.SSC_RULES_MAX_LEN)
    assert L.RulesDesc.length_penalty.offset == 4 * (3 + L.SSC_RULES_MAX_SUPPRESS)
    body = text[text.index("typedef struct {          /* running per-beam state"):text.index("} ssc_rules_state;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:int\*|float\*|int)\s+(\w+);", body)
    assert fields == [f for f, _ in L.RulesState._fields_]


# ---- refusals that need no launch ------------------------------------------------------------------------------------------------

def _descs(V=90, B=2, k=4, n=2, t=1):
    buf = (C.c_float * 4096)()   # host memory: never read, the checks come first
    a = C.addressof(buf)
    d = L.BeamDesc()
    d.scores, d.ld, d.raw_logits = a, V, 1
    d.dims = L.FsmDims(0, 1, V, 0, 1)
    d.B, d.beam, d.per_node, d.end_index = B, k, n, 1
    d.pred, d.lp_out, d.backptr, d.scratch_val, d.scratch_idx = a, a, a, a, a
    d.last_pred, d.last_lp, d.step_index = a, a, t
    s = L.RulesState()
    s.hist, s.len, s.hist_out, s.len_out, s.score_out, s.ld_hist = a, a, a + 2048, a + 2048, a, 64
    r = sampling.DecodeRules(3, 2, 1.0, (0,)).desc()
    return d, r, s, buf


def _refused(d, r, s, calls=("first", "step")):
    lib = L.load()
    for call in calls:
        rc = getattr(lib, f"_raw_ssc_beam_{call}_rules")(C.byref(d) if d else None, C.byref(r) if r else None,
                                                          C.byref(s) if s else None, None)
        assert rc == -1, call


def test_bad_descriptors_are_refused_before_any_launch():
    d, r, s, _ = _descs()
    _refused(None, r, s)
    _refused(d, None, s)
    _refused(d, r, None)
    for field in ("scores", "pred", "lp_out", "scratch_val", "scratch_idx"):
        d, r, s, _ = _descs()
        setattr(d, field, None)
        _refused(d, r, s)
    for field in ("hist_out", "len_out", "score_out"):
        d, r, s, _ = _descs()
        setattr(s, field, None)
        _refused(d, r, s)
    for field in ("last_pred", "last_lp", "backptr"):
        d, r, s, _ = _descs()
        setattr(d, field, None)
        _refused(d, r, s, calls=("step",))
    for field in ("hist", "len"):
        d, r, s, _ = _descs()
        setattr(s, field, None)
        _refused(d, r, s, calls=("step",))
    d, r, s, _ = _descs()
    d.dims = L.FsmDims(2, 2, 90, 0, 1)   # a machine
    _refused(d, r, s)
    d, r, s, _ = _descs()
    d.fsm = d.scores
    _refused(d, r, s)
    for k, n, V, B, calls in ((0, 2, 90, 2, ("first", "step")), (33, 2, 90, 2, ("first", "step")), (4, 0, 90, 2, ("step",)),
                              (4, 33, 90, 2, ("step",)), (8, 2, 6, 2, ("first", "step")), (4, 8, 6, 2, ("step",)),
                              (32, 2, 90, (1 << 19) + 1, ("first", "step"))):
        d, r, s, _ = _descs(V=V, B=B, k=k, n=n)
        _refused(d, r, s, calls=calls)
    for field, value in (("no_repeat_ngram", -1), ("no_repeat_ngram", 65), ("min_length", -1), ("n_suppress", -1), ("n_suppress", 9)):
        d, r, s, _ = _descs()
        setattr(r, field, value)
        _refused(d, r, s)
    for bad in (-1, 90, 1):   # outside [0, V), or the end token
        d, r, s, _ = _descs()
        r.suppress[0] = bad
        _refused(d, r, s)
    for at in (0, 17, 63):   # all 64 entries are checked, not only the ones a search of this length would use
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            d, r, s, _ = _descs()
            r.length_penalty[at] = bad
            _refused(d, r, s)
    for t in (0, -1, 64):
        d, r, s, _ = _descs(t=t)
        _refused(d, r, s, calls=("step",))
    d, r, s, _ = _descs(t=5)
    s.ld_hist = 5   # < step_index + 1
    _refused(d, r, s, calls=("step",))
    d, r, s, _ = _descs()
    s.hist_out = s.hist   # the two generations must differ
    _refused(d, r, s, calls=("step",))
    # the one-call search: NULL rules / outputs
    lib = L.load()
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    assert lib._raw_ssc_decode_rules_beam(C.byref(cfg), None, None, None, None, None, None, 0, None) == -1
    assert lib.ssc_decode_rules_beam_workspace_bytes(C.byref(cfg), None) == 0


def test_workspace_of_the_other_searches_is_unchanged_by_the_rules_fields():
    """The rules search takes the other searches' workspace plus its histories, lengths and scores (two generations each, every
    piece rounded up to 256 bytes); the plain search's size is what the same layout gives without them."""
    lib = L.load()
    cfg = L.ModelCfg(90, 24, 32, 16, 48, 8, 1, 0, 0, 0.5, 1.0, 0, 1, 0)
    sd = L.SearchDesc()
    sd.nimg, sd.R, sd.n_samples, sd.S, sd.beam, sd.per_node, sd.max_steps, sd.end_index = 3, 7, 4, 1, 5, 2, 9, 1
    plain = lib.ssc_decode_search_workspace_bytes(C.byref(cfg), C.byref(sd))
    rules = lib.ssc_decode_rules_beam_workspace_bytes(C.byref(cfg), C.byref(sd))
    G = 3 * 4 * 5

    def up(n):
        return (n + 255) // 256 * 256

    assert plain > 0 and rules == plain + 2 * (up(G * 9 * 4) + 2 * up(G * 4))


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def chain_model(V, seed, loop=4.0):
    """A first-order chain over V words whose favourite successors run in short cycles, so that a plain search repeats n-grams:
    step(tokens, states) -> (float32 log-probs (rows, V), states)."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((V, V)) * 0.7
    for v in range(2, V):
        W[v, 2 + (v - 2 + 1) % 3 + 3 * ((v - 2) // 3 % 2)] += loop   # cycles of three words
    W[:, R.END] -= 1.0
    W[R.END, 2:8] += 1.0

    def step(tokens, states):
        t = states["t"][0]
        x = W[tokens] + 0.15 * t * (np.arange(V) == R.END)   # END grows slowly more likely
        return dbsref.log_softmax64(x).astype(F), {"t": states["t"] + 1}

    return step


def test_rules_off_is_the_one_group_search_of_dbsref():
    V, B, k, n, steps = 40, 3, 5, 2, 10
    for seed in (0, 1):
        step = chain_model(V, seed)
        st = {"t": np.zeros(B, dtype=np.int64)}
        pred, lps, rec = R.search(step, st, B, k, n, R.Rules(), steps, early_stop=False)
        dpred, dlps, drec = dbsref.search(step, st, B, k, 1, n, 0.0, steps, early_stop=False)
        assert np.array_equal(pred, dpred) and np.array_equal(lps.view(np.int32), dlps.view(np.int32))
        for t in range(steps):
            assert np.array_equal(rec["tok"][t], drec["tok"][t])
            assert np.array_equal(rec["score"][t].view(np.int32), rec["lp"][t].view(np.int32))   # x / 1.0f is x
            if t:
                assert np.array_equal(rec["bp"][t], drec["bp"][t])
        # the final history generation is the back-traced prediction
        assert np.array_equal(rec["hist"][-1], pred)


def test_trigram_blocking_against_a_brute_force_check():
    V, B, k, n, steps = 40, 4, 5, 2, 14
    step = chain_model(V, 3)
    st = {"t": np.zeros(B, dtype=np.int64)}
    plain, _, _ = R.search(step, st, B, k, n, R.Rules(), steps, early_stop=False)
    assert any(R.repeated_ngram(c, 3) for c in plain.reshape(-1, steps)), "the chain repeats no trigram: the test proves nothing"
    rules = R.Rules(ngram=3, min_length=4, suppress=(0, 5), table=R.penalty_table(1.0))
    pred, lps, rec = R.search(step, st, B, k, n, rules, steps, early_stop=False)
    assert np.array_equal(rec["hist"][-1], pred)
    for b in range(B):
        for j in range(k):
            cap = [int(v) for v in pred[b, j]]
            words = cap[:cap.index(R.END)] if R.END in cap else cap
            grams = [tuple(words[i:i + 3]) for i in range(len(words) - 2)]   # brute force: every trigram at most once
            assert len(grams) == len(set(grams)), cap
            assert len(words) >= 4 or not np.isfinite(lps[b, j]), cap
            assert 0 not in words and 5 not in words
            L_ = rec["len"][-1][b, j]
            assert L_ == (len(words) + 1 if R.END in cap else steps)
            assert rec["score"][-1][b, j] == lps[b, j] / rules.table[L_ - 1]
    assert (np.diff(rec["score"][-1], axis=1) <= 0).all()   # sorted by key


def test_unigram_and_bigram_blocking_and_the_ban_mask():
    assert R.banned(10, [2, 3, 2], 3, R.Rules(ngram=2)).nonzero()[0].tolist() == [3]        # (2, 3) seen: 3 after 2 is banned
    assert R.banned(10, [2, 3, 4], 3, R.Rules(ngram=2)).nonzero()[0].tolist() == []
    assert R.banned(10, [2, 3, 2], 3, R.Rules(ngram=1)).nonzero()[0].tolist() == [2, 3]
    assert R.banned(10, [2, 3], 2, R.Rules(ngram=3)).nonzero()[0].tolist() == []            # fewer than n tokens: nothing
    assert R.banned(10, [2, 3, 4, 2, 3], 5, R.Rules(ngram=3)).nonzero()[0].tolist() == [4]
    assert R.banned(10, [2], 1, R.Rules(min_length=2, suppress=(0,))).nonzero()[0].tolist() == [0, R.END]
    assert R.banned(10, [2, 5], 2, R.Rules(min_length=2, suppress=(0,))).nonzero()[0].tolist() == [0]
