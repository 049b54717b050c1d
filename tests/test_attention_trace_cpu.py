"""CPU: attention traces (include/ssc.h: ssc_attn_record, ssc_attn_gather) - the restated ancestry on hand-built searches, the
bindings against the header, every refusal (no launch is reached: no GPU needed), the workspace sizes with and without a trace, and
the MODEL.DECODE_ATTENTION key."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import attnref as AR
from ssc_runtime import lib as L
from ssc_runtime.config import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1


# ---- the restated ancestry ---------------------------------------------------------------------------------------------------------
def test_crossing_ancestry():
    """Two beams that swap places at every step: word t of a final beam was produced by the row its ancestor stood in."""
    T, B, SB = 4, 1, 2
    words = np.array([[[5, 6]], [[7, 8]], [[9, 10]], [[11, 12]]])
    backs = np.array([[[1, 0]], [[1, 0]], [[1, 0]]])
    anc = AR.ancestry(words, backs, None, END)
    # final beam 0: place after step 3 = 0, after 2 = 1, after 1 = 0, after 0 = 1 -> rows b, 1, 0, 1
    assert anc.tolist() == [[0, 1, 0, 1], [0, 0, 1, 0]]
    # both children of ONE parent: the two captions share the rows of their common past
    backs[2] = [[1, 1]]
    # (both stood at place 1 after step 2, which stood at 0 after step 1 and at 1 after step 0)
    assert AR.ancestry(words, backs, None, END).tolist() == [[0, 1, 0, 1], [0, 1, 0, 1]]


def test_end_in_mid_chain_keeps_the_first_end_and_drops_the_forced_ones():
    words = np.array([[[5, 6]], [[END, 8]], [[END, 9]], [[END, END]]])
    backs = np.array([[[0, 1]], [[0, 1]], [[0, 1]]])
    anc = AR.ancestry(words, backs, None, END)
    assert anc.tolist() == [[0, 0, -1, -1], [0, 1, 1, 1]]   # (beam 1's END at step 3 is its first: real attention)


def test_stop_at_3_of_7_steps():
    T, B, SB = 7, 2, 2
    rng = np.random.default_rng(0)
    words = rng.integers(2, 9, (T, B, SB))
    backs = rng.integers(0, SB, (T - 1, B, SB))
    anc = AR.ancestry(words, backs, 3, END)
    assert (anc[:, 3:] == -1).all() and (anc[:, :3] >= 0).all()
    # the chain starts at step 2, not at step 6
    for b in range(B):
        for j in range(SB):
            p1 = backs[1][b, j]
            p0 = backs[0][b, p1]
            assert anc[b * SB + j].tolist()[:3] == [b, b * SB + p0, b * SB + p1]
    assert (AR.ancestry(words, backs, 0, END)[:, 1:] == -1).all()   # (ctl[0] is at least 1: the first step always runs)


def test_dead_beam_and_single_beam():
    words = np.array([[[5, 6, 7]], [[8, 9, 10]]])
    backs = np.array([[[2, 0, 1]]])
    lp = np.array([[-1.5, -1e20, -2.0]], dtype=np.float32)
    anc = AR.ancestry(words, backs, None, END, lp)
    assert anc.tolist() == [[0, 2], [-1, -1], [0, 1]]
    # SB = 1, no back-pointers (a row decode): the identity until the row has ended; negative words (a scoring call) read nothing
    words = np.array([[[5], [5], [-1]], [[END], [6], [-1]], [[END], [END], [-1]], [[END], [END], [-1]]])
    assert AR.ancestry(words, None, None, END).tolist() == [[0, 0, -1, -1], [1, 1, 1, -1], [-1, -1, -1, -1]]


def test_restated_gather():
    hist = np.zeros((2, 3, 4), dtype=np.float32)
    hist[0, 1] = [0.25, 0.5, 0.25, 0.0]
    hist[1, 2] = [0.4, 0.1, 0.4, 0.1]          # an exact tie: the lower index
    hist[1, 0] = np.nan                         # never read
    anc = np.array([[1, 2], [-1, 7]])
    maps, top, wgt, ent = AR.gather(hist, anc, [0, 1, 5, 0])
    assert top.tolist() == [[1, 0], [-1, -1], [-1, -1], [1, 0]] and wgt[0].tolist() == [0.5, np.float32(0.4)]
    assert ent[0, 0] == pytest.approx(1.5 * np.log(2)) and (maps[1:3] == 0).all() and (ent[1:3] == 0).all()
    assert np.array_equal(maps[3], maps[0]) and np.array_equal(maps[0, 0], hist[0, 1])


# ---- bindings against the header -----------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "ssc.h")).read()


def struct_fields(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = text[:text.index("} " + name + ";")]
    body = body[body.rindex("typedef struct {"):]
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?[A-Za-z_0-9]+\s*\**\s*", "", decl)
        fields += [n.strip().lstrip("*").strip() for n in decl.split(",")]
    return fields


def test_bindings_mirror_the_header():
    assert struct_fields("ssc_attn_record") == [f for f, _ in L.AttnRecord._fields_] == ["hist", "anc"]
    assert struct_fields("ssc_attn_gather_desc") == [f for f, _ in L.AttnGatherDesc._fields_]
    for c_name, cls in (("ssc_search_desc", L.SearchDesc), ("ssc_score_desc", L.ScoreDesc)):
        got = struct_fields(c_name)
        assert got[-1] == "attn" and cls._fields_[-1][0] == "attn" and cls._fields_[-1][1] is C.POINTER(L.AttnRecord)
        assert got == [f for f, _ in cls._fields_]
    assert "ssc_attn_gather" in L.SYMBOLS and "ssc_debug_decode_view" in L.DEBUG_SYMBOLS
    assert C.sizeof(L.AttnRecord) == 16 and C.sizeof(L.AttnGatherDesc) == 96
    lib = L.load()
    assert lib.ssc_version() == 4
    assert not L.SearchDesc().attn and not L.ScoreDesc().attn   # a zero-initialised descriptor: the trace is off


# ---- refusals, without a GPU ---------------------------------------------------------------------------------------------------------
def test_gather_refusals():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)   # (never read: every check comes before the launch)

    def desc(**kw):
        d = L.AttnGatherDesc(hist=a, rows=4, R=4, steps=2, anc=a, n_caps=4, sel=None, n_sel=4, maps=a, ld_maps=4, top_region=a,
                             top_weight=a, entropy=a)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = [dict(hist=None), dict(anc=None), dict(maps=None, top_region=None, top_weight=None, entropy=None), dict(ld_maps=3),
           dict(rows=0), dict(R=0), dict(steps=0), dict(n_caps=0), dict(n_sel=0), dict(rows=-1), dict(R=-3), dict(steps=-1),
           dict(n_caps=-2), dict(n_sel=-1), dict(n_sel=3)]
    for kw in bad:
        assert lib._raw_ssc_attn_gather(C.byref(desc(**kw)), None) == -1, kw
    assert lib._raw_ssc_attn_gather(None, None) == -1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_attn_gather(C.byref(desc(hist=None)), None)


CFG = dict(V=50, E=8, H=8, A=8, F=8, Z=4)


def model_cfg():
    return L.ModelCfg(CFG["V"], CFG["E"], CFG["H"], CFG["A"], CFG["F"], CFG["Z"], 0, 0, 0, 0.0, 1.0, 0, 1, 0)


def search_desc(a, beam=4, per_node=2):
    d = L.SearchDesc()
    d.nimg, d.R, d.n_samples, d.S, d.beam, d.per_node, d.max_steps, d.end_index = 2, 5, 3, 1, beam, per_node, 6, 1
    d.feats = d.imgbuf = d.eps0 = d.eps = d.predictions = d.log_probs = d.ctl = a
    return d


def sample_opts(guide=None, rules=None, trunc=None, contrast=None, nbytes=None):
    """-> an ssc_sample_opts over the given descriptors (ctypes structures, or None: a NULL field); bytes = its own size unless given."""
    o = L.SampleOpts(bytes=C.sizeof(L.SampleOpts) if nbytes is None else nbytes)
    for field, desc in (("guide", guide), ("rules", rules), ("trunc", trunc), ("contrast", contrast)):
        if desc is not None:
            setattr(o, field, C.pointer(desc))
    return o


# the per-feature entries of the sampled decode that ssc_sample_opts / ssc_decode_sample_opts replaced
RETIRED_SAMPLE_ENTRIES = ("ssc_decode_sample_guided", "ssc_decode_sample_rules", "ssc_decode_sample_rules_workspace_bytes",
                          "ssc_decode_sample_trunc", "ssc_decode_sample_trunc_workspace_bytes", "ssc_decode_sample_contrast",
                          "ssc_decode_sample_contrast_workspace_bytes")


def score_desc(a):
    d = L.ScoreDesc()
    d.nimg, d.R, d.n_captions, d.n_samples, d.max_len, d.end_index = 2, 5, 3, 2, 6, 1
    d.feats = d.imgbuf = d.eps0 = d.eps = d.targets = d.log_probs = d.n_tokens = a
    return d


def one_call_decodes(lib, a):
    """-> [(name, descriptor, bytes(cfg, desc), call(cfg, params, desc, workspace_bytes))] of every one-call decode, each with a
    descriptor that passes its checks (the pointers are one host buffer: no check reads through them)."""
    gum = L.GumbelDesc(1.0, 3)
    smp = L.SamplerDesc(0, 0, 1.0, 1.0, 3)
    div = L.DiverseDesc(2, 0.5)
    rul = L.RulesDesc()
    rul.no_repeat_ngram, rul.min_length = 2, 1
    for q in range(L.SSC_RULES_MAX_LEN):
        rul.length_penalty[q] = 1.0
    p = L.Params()
    ref = C.byref
    return [
        ("search", search_desc(a), lib.ssc_decode_search_workspace_bytes,
         lambda c, d, n: lib._raw_ssc_decode_search(c, ref(p), d, a, n, None)),
        ("stochastic", search_desc(a), lib.ssc_decode_stochastic_beam_workspace_bytes,
         lambda c, d, n: lib._raw_ssc_decode_stochastic_beam(c, ref(p), d, ref(gum), a, n, None)),
        ("sampled", search_desc(a), lib.ssc_decode_sampled_beam_workspace_bytes,
         lambda c, d, n: lib._raw_ssc_decode_sampled_beam(c, ref(p), d, ref(smp), 0, a, n, None)),
        ("diverse", search_desc(a), lambda c, d: lib.ssc_decode_diverse_beam_workspace_bytes(c, d, ref(div)),
         lambda c, d, n: lib._raw_ssc_decode_diverse_beam(c, ref(p), d, ref(div), a, n, None)),
        ("rules", search_desc(a), lib.ssc_decode_rules_beam_workspace_bytes,
         lambda c, d, n: lib._raw_ssc_decode_rules_beam(c, ref(p), d, ref(rul), a, a, a, n, None)),
        ("sample", search_desc(a, beam=1, per_node=1), lib.ssc_decode_sample_workspace_bytes,
         lambda c, d, n: lib._raw_ssc_decode_sample(c, ref(p), d, ref(smp), a, n, None)),
        ("score", score_desc(a), lib.ssc_decode_score_workspace_bytes,
         lambda c, d, n: lib._raw_ssc_decode_score(c, ref(p), d, a, n, None)),
    ]


def test_a_trace_without_its_buffers_is_refused_before_any_launch_and_costs_no_workspace():
    """Every one-call decode, with a descriptor that passes every check and a workspace one byte short: SSC_EWORKSPACE (-4) - the
    descriptor was accepted, nothing was launched - with the trace off and with a complete trace; SSC_EINVAL (-1) as soon as the
    trace lacks hist or anc.  *_workspace_bytes is the same number with the trace off and on."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    for name, d, nbytes, call in one_call_decodes(lib, a):
        off = nbytes(C.byref(cfg), C.byref(d))
        assert off > 0, name
        assert call(C.byref(cfg), C.byref(d), off - 1) == -4, name
        rec = L.AttnRecord(a, a)
        d.attn = C.pointer(rec)
        assert nbytes(C.byref(cfg), C.byref(d)) == off, name
        assert call(C.byref(cfg), C.byref(d), off - 1) == -4, name
        for hist, anc in ((None, a), (a, None), (None, None)):
            bad = L.AttnRecord(hist, anc)
            d.attn = C.pointer(bad)
            assert call(C.byref(cfg), C.byref(d), off - 1) == -1, (name, hist, anc)
            assert call(C.byref(cfg), C.byref(d), off) == -1, (name, hist, anc)
            assert nbytes(C.byref(cfg), C.byref(d)) == off, name


def test_debug_view_refuses_bad_arguments():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    d = search_desc(a)
    view = lib.ssc_debug_decode_view
    assert view(C.byref(cfg), C.byref(d), a, 0, 0) and view(C.byref(cfg), C.byref(d), a, 0, 1)
    assert view(C.byref(cfg), C.byref(d), a, 1, 0) and not view(C.byref(cfg), C.byref(d), a, 1, 1)
    assert not view(C.byref(cfg), C.byref(d), None, 0, 0) and not view(C.byref(cfg), C.byref(d), a, 2, 0)
    assert not view(C.byref(cfg), C.byref(d), a, 0, 2) and not view(None, C.byref(d), a, 0, 0)


# ---- the config key ------------------------------------------------------------------------------------------------------------------
def test_config_key_and_its_refusals():
    assert Config().MODEL.DECODE_ATTENTION == "none"
    for mode in ("none", "summary", "full"):
        assert Config(config_override=["MODEL.DECODE_ATTENTION", mode]).MODEL.DECODE_ATTENTION == mode
    for bad in ("all", "Full", ""):
        with pytest.raises(ValueError, match="DECODE_ATTENTION"):
            Config(config_override=["MODEL.DECODE_ATTENTION", bad])
    with pytest.raises(ValueError, match="DECODE_ATTENTION"):
        Config(config_override=["MODEL.DECODE_ATTENTION", 1])
