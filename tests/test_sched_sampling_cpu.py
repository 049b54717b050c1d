"""CPU: scheduled sampling - the restated forward (tests/schedsampref.py) against the oracle, the schedule and the seed
(ssc_runtime/schedule.py), the OPTIM.SCHEDULED_SAMPLING_* config keys, and the C ABI of ssc_sched_mix_rows and of
ssc_train_fwd_opts / ssc_train_bwd_opts with a `sched` descriptor: exported, mirrored in ctypes, and refusing bad arguments before anything is launched
(no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import oracle
import schedsampref as R
from ssc_runtime import lib as L
from ssc_runtime.config import Config
from ssc_runtime.schedule import ss_prob, ss_prob_from_config, ss_sampler_from_config, ss_seed
from ssc_runtime.scst import scst_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restated forward ---------------------------------------------------------------------------------------------------
def _case(sv, tied=False):
    cfg = oracle.OracleConfig(vocab_size=30, image_feature_size=12, embedding_size=8, hidden_size=10, attention_projection_size=6,
                              z_space=5, max_caption_length=4, sentiment_vae=sv, senti_prior_multip=0.5, prior_std=0.9, tied=tied)
    params = oracle.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(4)
    B, Rg, L_ = 3, 4, 4
    feats = torch.randn(B, Rg, 12, generator=g)
    caps = torch.tensor([[5, 0, 7, 9], [8, 9, 0, 0], [3, 4, 5, 6]])           # row 0: an in-caption id 0
    senti = torch.tensor([[1.0], [-1.0], [0.0]])
    eps = torch.randn(L_ + 1, B, 5, generator=g)
    return cfg, params, feats, caps, senti, eps


@pytest.mark.parametrize("sv,tied", [(0, False), (1, False), (1, True)])
def test_restated_forward_with_ground_truth_inputs_is_the_oracle(sv, tied):
    cfg, params, feats, caps, senti, eps = _case(sv, tied)
    tok, w = R.tokens_and_weights(cfg, caps)
    res = []
    for fed in (None, tok[:-1]):
        p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        out = (oracle.train_forward(p, cfg, feats, caps, senti, eps) if fed is None
               else R.train_forward_fed(p, cfg, feats, caps, senti, eps, fed))
        oracle.train_objective(out, cfg).backward()
        res.append((out, p))
    (a, pa), (b, pb) = res
    assert (a["loss"] - b["loss"]).abs().max().item() <= 1e-12 and (a["kld"] - b["kld"]).abs().max().item() <= 1e-12
    for k in pa:
        ga = pa[k].grad if pa[k].grad is not None else torch.zeros_like(pa[k])
        gb = pb[k].grad if pb[k].grad is not None else torch.zeros_like(pb[k])
        assert (ga - gb).abs().max().item() <= 1e-12, k
    # other inputs do move it - and the embedding gradient lands on the rows that were fed
    fed = tok[:-1].clone()
    fed[1, 2] = 17                                                              # (t = 1, b = 2): ground truth 3
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = R.train_forward_fed(p, cfg, feats, caps, senti, eps, fed)
    oracle.train_objective(out, cfg).backward()
    assert (out["loss"] - a["loss"]).abs().max().item() > 1e-6
    if not tied:
        ge = p["_embedding_layer.weight"].grad
        assert float(ge[17].abs().max()) > 0 and float(pa["_embedding_layer.weight"].grad[17].abs().max()) == 0
        assert float(ge[0].abs().max()) == 0                                    # id 0 (fed after the in-caption unknown) receives none


def test_decisions_eligibility_and_the_two_streams():
    seed = 0x1234_5678_9ABC_DEF0
    u = R.uniforms(seed, 6, 5)
    assert u.dtype == np.float32 and u.shape == (6, 5) and bool(((u > 0) & (u < 1)).all())
    assert np.array_equal(R.uniforms_step(seed, 4, 5), u[4])                    # row r of step t: counter (0, t, r, 1)
    assert np.array_equal(R.uniforms(seed, 6, 9)[:, :5], u)
    # counter word 3 = 1: not the word draws' block (0, t, b, 0)
    import samplerref as S
    ctr = np.array([[0, 4, 2, 0]], dtype=np.uint32)
    x0 = S.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[0, 0]
    u0 = np.float32(((int(x0) >> 9) * 2 + 1) * 2.0 ** -24)
    assert u0 != u[4, 2]
    w = np.array([[1, 1, 1], [1, 1, 0], [0, 1, 0], [1, 0, 0], [1, 0, 0]], dtype=np.float32)
    e = R.eligible(w)
    assert e.tolist() == [[False] * 3, [True, True, False], [False, True, False], [False, False, False], [True, False, False]]
    assert not R.fires(u[:5, :3], e, 0.0).any()
    assert np.array_equal(R.fires(u[:5, :3], e, 1.0), e)
    assert np.array_equal(R.fires(u[:5, :3], e, 0.5), e & (u[:5, :3] < np.float32(0.5)))


# ---- schedule and seed ------------------------------------------------------------------------------------------------------
def test_ss_prob_corners():
    kw = dict(start=100, every=10, increase=0.05, maximum=0.25)
    assert ss_prob(0, **kw) == 0.0 and ss_prob(99, **kw) == 0.0                # before start
    assert ss_prob(100, **kw) == 0.0 and ss_prob(109, **kw) == 0.0             # at start: (0 // every) increases so far
    assert ss_prob(110, **kw) == 0.05 and ss_prob(119, **kw) == 0.05           # at each increase
    assert ss_prob(120, **kw) == 0.05 * 2 and ss_prob(130, **kw) == 0.05 * 3 and ss_prob(140, **kw) == 0.05 * 4
    assert ss_prob(150, **kw) == 0.25 and ss_prob(10 ** 9, **kw) == 0.25       # at the cap
    for it in (0, 5, 10 ** 6):
        assert ss_prob(it, start=-1, every=1, increase=1.0, maximum=1.0) == 0.0   # start = -1: off
    assert ss_prob(0, start=0, every=1, increase=0.5, maximum=1.0) == 0.0 and ss_prob(1, 0, 1, 0.5, 1.0) == 0.5
    assert ss_prob(2, 0, 1, 0.5, 1.0) == 1.0 and ss_prob(3, 0, 1, 0.5, 1.0) == 1.0
    assert isinstance(ss_prob(110, **kw), float)
    want = {it: ss_prob(it, **kw) for it in range(90, 160)}
    for it in (159, 91, 120, 91, 150):                                          # a pure function of the iteration
        assert ss_prob(it, **kw) == want[it]
    for bad in (dict(every=0), dict(increase=-0.1), dict(increase=1.5), dict(maximum=1.1), dict(maximum=float("nan"))):
        args = dict(kw)
        args.update(bad)
        with pytest.raises(ValueError, match="ss_prob"):
            ss_prob(120, **args)


def test_ss_seed_is_its_own_stream():
    seen = set()
    for rs in (0, 1, 7):
        for it in (1, 2, 1000):
            for rank in (0, 1, 7):
                s = ss_seed(rs, it, rank)
                assert 0 <= s < 2 ** 64 and s != scst_seed(rs, it, rank)
                assert s == ss_seed(rs, it, rank)
                seen.add(s)
    assert len(seen) == 27                                                      # differs across seeds, iterations and ranks
    assert len({ss_seed(3, 10, r) for r in range(8)}) == 8


# ---- config -----------------------------------------------------------------------------------------------------------------
def test_config_keys_defaults_overrides_and_refusals():
    o = Config().OPTIM
    assert (o.SCHEDULED_SAMPLING_START, o.SCHEDULED_SAMPLING_INCREASE_EVERY, o.SCHEDULED_SAMPLING_INCREASE_PROB,
            o.SCHEDULED_SAMPLING_MAX_PROB, o.SCHEDULED_SAMPLING_SAMPLER, o.SCHEDULED_SAMPLING_TEMPERATURE) == (
        -1, 5000, 0.05, 0.25, "multinomial", 1.0)
    assert ss_prob_from_config(o, 10 ** 6) == 0.0 and ss_sampler_from_config(o) == (0, 0, 1.0, 1.0)
    c = Config(None, ["OPTIM.SCHEDULED_SAMPLING_START", "0", "OPTIM.SCHEDULED_SAMPLING_INCREASE_EVERY", "2",
                      "OPTIM.SCHEDULED_SAMPLING_INCREASE_PROB", "0.5", "OPTIM.SCHEDULED_SAMPLING_MAX_PROB", "1",
                      "OPTIM.SCHEDULED_SAMPLING_SAMPLER", "argmax", "OPTIM.SCHEDULED_SAMPLING_TEMPERATURE", "0.7"]).OPTIM
    assert [ss_prob_from_config(c, it) for it in range(6)] == [0.0, 0.0, 0.5, 0.5, 1.0, 1.0]
    assert ss_sampler_from_config(c) == (1, 1, 1.0, 1.0)                        # arg-max: top-k with k = 1
    m = Config(None, ["OPTIM.SCHEDULED_SAMPLING_TEMPERATURE", "0.7"]).OPTIM
    assert ss_sampler_from_config(m) == (0, 0, 1.0, 0.7)
    bad = [("SCHEDULED_SAMPLING_START", "-2"), ("SCHEDULED_SAMPLING_START", "True"), ("SCHEDULED_SAMPLING_INCREASE_EVERY", "0"),
           ("SCHEDULED_SAMPLING_INCREASE_EVERY", "-5"), ("SCHEDULED_SAMPLING_INCREASE_PROB", "-0.1"),
           ("SCHEDULED_SAMPLING_INCREASE_PROB", "1.5"), ("SCHEDULED_SAMPLING_MAX_PROB", "1.01"), ("SCHEDULED_SAMPLING_MAX_PROB", "-1"),
           ("SCHEDULED_SAMPLING_SAMPLER", "top-k"), ("SCHEDULED_SAMPLING_SAMPLER", "beam"), ("SCHEDULED_SAMPLING_TEMPERATURE", "0"),
           ("SCHEDULED_SAMPLING_TEMPERATURE", "-1.0")]
    for key, val in bad:
        with pytest.raises(ValueError, match="OPTIM." + key):
            Config(None, ["OPTIM." + key, val])
    with pytest.raises(ValueError):
        Config(None, ["OPTIM.SCHEDULED_SAMPLING_START", "1.5"])                 # not an integer: refused by type or by value


def test_engine_argument_check():
    from ssc_runtime import sampling
    from ssc_runtime.engine import check_sched_sampling
    assert check_sched_sampling(0.0) is None and check_sched_sampling(0, None, 5) is None
    ss = check_sched_sampling(0.25, None, 2 ** 64 - 1)
    assert (ss.prob, ss.sampler.kind, ss.sampler.temperature, ss.sampler.seed) == (0.25, 0, 1.0, 2 ** 64 - 1)
    ss = check_sched_sampling(1.0, sampling.TopKSampler(k=3, temperature=0.5), 9)
    assert (ss.sampler.kind, ss.sampler.top_k, ss.sampler.temperature, ss.sampler.seed) == (1, 3, 0.5, 9)
    ss = check_sched_sampling(0.5, (2, 0, 0.9, 1.5), 1)
    assert (ss.sampler.kind, round(ss.sampler.top_p, 6), ss.sampler.temperature) == (2, 0.9, 1.5)
    for bad in (-0.1, 1.1, float("nan"), "x", True):
        with pytest.raises(ValueError, match="ss_prob"):
            check_sched_sampling(bad)
    for bad in ((3, 0, 1.0, 1.0), (0, 0, 1.0, 0.0), (1, 0, 1.0, 1.0), (2, 0, 1.5, 1.0)):
        with pytest.raises(ValueError, match="ss_sampler"):
            check_sched_sampling(0.5, bad)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_and_bindings_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    body = text[text.index("typedef struct {\n  float prob;"):text.index("} ssc_sched_sampling;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(?:float|ssc_sampler_desc)\s+(\w+);", body) == [f for f, _ in L.SchedSampling._fields_] == ["prob", "sampler"]
    assert L.SchedSampling._fields_[1][1] is L.SamplerDesc
    assert C.sizeof(L.SchedSampling) == 8 + C.sizeof(L.SamplerDesc) and L.SchedSampling.sampler.offset == 8   # (the seed is 8-byte aligned)
    assert L.ModelCfg._fields_[-1] == ("label_smoothing", C.c_float)            # the cfg did not grow
    cdll = C.CDLL(L.LIB_PATH)
    for name in ("ssc_sched_mix_rows", "ssc_train_fwd_opts", "ssc_train_bwd_opts", "ssc_train_sched_view"):
        assert hasattr(cdll, name) and name in L.SYMBOLS
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ssc_sched_mix_rows", "ssc_train_fwd_opts", "ssc_train_bwd_opts"):
        decl = flat[flat.index("int " + name + "("):]
        nargs = decl[:decl.index(");")].count(",") + 1
        assert nargs == len(L.SYMBOLS[name][1]), name
    # the descriptor travels as a field of ssc_train_opts (its layout: tests/test_free_bits_cpu.py), a pointer to this struct
    assert dict(L.TrainOpts._fields_)["sched"] is C.POINTER(L.SchedSampling) and L.TrainOpts.sched.offset == 8
    lib = L.load()
    assert lib.ssc_version() == 4
    # the two new blocks sit behind every other one: views 13 / 14 of ssc_train_sched_view, offsets larger than any other view's
    # (the numbering of ssc_train_workspace_view itself stays 0..12)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    buf = (C.c_float * 16)()
    base = C.addressof(buf)
    ld = C.c_int(0)
    off = {w: lib.ssc_train_workspace_view(C.byref(cfg), 2, 3, 4, base, w, C.byref(ld)) - base for w in range(13)}
    for w in (13, 14):
        assert not lib.ssc_train_workspace_view(C.byref(cfg), 2, 3, 4, base, w, C.byref(ld))
        off[w] = lib.ssc_train_sched_view(C.byref(cfg), 2, 3, 4, base, w, C.byref(ld)) - base
        assert ld.value == 2
    for w in (0, 12, 15, -1):
        assert not lib.ssc_train_sched_view(C.byref(cfg), 2, 3, 4, base, w, C.byref(ld))
    assert not lib.ssc_train_sched_view(C.byref(cfg), 0, 3, 4, base, 13, C.byref(ld))
    assert off[13] > max(off[w] for w in range(13)) and off[14] > off[13]
    fb = [lib.ssc_train_free_bits_view(C.byref(cfg), 2, 3, 4, base, w, C.byref(ld)) - base for w in range(4)]
    assert off[13] > max(fb)
    assert off[14] + 4 * (5 * 2) <= lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4)


def _ss(prob=0.5, kind=0, top_k=0, top_p=1.0, temperature=1.0, seed=7):
    return L.SchedSampling(prob, L.SamplerDesc(kind, top_k, top_p, temperature, seed))


def test_mix_rows_refuses_bad_arguments_before_anything_is_launched():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    good = dict(logits=a, ld=8, rows=0, V=8, truth=a, w_prev=a, w_cur=a, table=a, ldt=4, E=4, step=1, ss=_ss(), tok_out=a, fed_out=a,
                emb_out=a, ldo=4)
    order = ["logits", "ld", "rows", "V", "truth", "w_prev", "w_cur", "table", "ldt", "E", "step", "ss", "tok_out", "fed_out", "emb_out",
             "ldo"]

    def call(**kw):
        d = dict(good)
        d.update(kw)
        args = [C.byref(d[k]) if k == "ss" and d[k] is not None else d[k] for k in order]
        return lib._raw_ssc_sched_mix_rows(*args, None)

    assert call() == 0                                                          # no rows: every check passed, nothing launched
    for name in ("logits", "truth", "w_prev", "w_cur", "table", "ss", "tok_out", "fed_out", "emb_out"):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None, "rows": 3}) == -1, name
    for rows in (0, 3):                                                         # refused whatever the row count: before a launch
        for prob in (-0.1, 1.0001, float("nan"), float("inf")):
            assert call(ss=_ss(prob=prob), rows=rows) == -1, prob
        assert call(ld=7, rows=rows) == -1 and call(step=0, rows=rows) == -1 and call(step=-3, rows=rows) == -1
        assert call(ldt=3, rows=rows) == -1 and call(ldo=3, rows=rows) == -1 and call(E=0, rows=rows) == -1 and call(V=0, rows=rows) == -1
        # the sampler limits of ssc_sample_rows
        assert call(ss=_ss(kind=3), rows=rows) == -1 and call(ss=_ss(kind=-1), rows=rows) == -1
        assert call(ss=_ss(temperature=0.0), rows=rows) == -1 and call(ss=_ss(temperature=float("nan")), rows=rows) == -1
        assert call(ss=_ss(temperature=float("inf")), rows=rows) == -1
        assert call(ss=_ss(kind=1, top_k=0), rows=rows) == -1 and call(ss=_ss(kind=1, top_k=9), rows=rows) == -1
        assert call(ss=_ss(kind=2, top_p=-0.1), rows=rows) == -1 and call(ss=_ss(kind=2, top_p=1.1), rows=rows) == -1
    assert call(rows=-1) == -1
    assert call(ss=_ss(prob=0.0)) == 0 and call(ss=_ss(prob=1.0)) == 0 and call(ss=_ss(kind=1, top_k=8)) == 0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_sched_mix_rows(a, 8, 3, 8, a, a, a, a, 4, 4, 0, C.byref(_ss()), a, a, a, 4, None)


def test_train_entries_refuse_bad_sampling_arguments():
    """Everything else is in order and the workspace is too small: arguments that pass end at SSC_EWORKSPACE (before any launch), bad
    ones at SSC_EINVAL."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    p = L.Params()
    for name, typ in L.Params._fields_:
        setattr(p, name, 4 if typ is C.c_int else a)
    bt = L.Batch(2, 3, 4, a, a, a, a, None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)

    def opts(ss, free_bits=0.0, mode=0, kd=None):
        return C.byref(L.TrainOpts(free_bits, mode, C.pointer(ss) if ss is not None else None, C.pointer(kd) if kd is not None else None))

    def fwd(ss, free_bits=0.0, mode=0, kd=None):
        return lib._raw_ssc_train_fwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, opts(ss, free_bits, mode, kd), None)

    def bwd(ss, phases=15, free_bits=0.0, mode=0, kd=None):
        return lib._raw_ssc_train_bwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), phases,
                                           opts(ss, free_bits, mode, kd), None)

    assert fwd(None) == -4 and fwd(_ss(0.0)) == -4 and fwd(_ss(0.25)) == -4 and fwd(_ss(1.0)) == -4
    assert fwd(_ss(0.5, kind=1, top_k=1)) == -4 and fwd(_ss(0.5, kind=1, top_k=10)) == -4 and fwd(_ss(0.5, kind=2, top_p=0.9)) == -4
    for prob in (-0.1, 1.5, float("nan")):
        assert fwd(_ss(prob)) == -1
    assert fwd(_ss(0.5, kind=1, top_k=11)) == -1 and fwd(_ss(0.5, kind=3)) == -1 and fwd(_ss(0.5, temperature=0.0)) == -1
    assert fwd(_ss(0.5), 0.1, 0) == -1 and fwd(_ss(0.5), 0.1, 3) == -4         # the free-bits checks are the same helper's
    # the backward is given the opts of its forward ("the forward fed its own words" is sched->prob > 0) and refuses every
    # descriptor the forward refuses, whatever the phases
    for phases in (15, 64, 2):
        assert bwd(None, phases) == -4 and bwd(_ss(0.0), phases) == -4 and bwd(_ss(0.5), phases) == -4 and bwd(_ss(1.0), phases) == -4
        assert bwd(_ss(0.5, kind=1, top_k=10), phases) == -4 and bwd(_ss(0.5, kind=2, top_p=0.9), phases) == -4
        for prob in (-0.1, 1.5, float("nan")):
            assert bwd(_ss(prob), phases) == -1, prob
        assert bwd(_ss(0.5, kind=3), phases) == -1 and bwd(_ss(0.5, kind=1, top_k=11), phases) == -1
        assert bwd(_ss(0.5, temperature=0.0), phases) == -1
        assert bwd(_ss(0.5), phases, 0.1, 0) == -1 and bwd(_ss(0.5), phases, 0.1, 3) == -4
    assert bwd(_ss(0.5), 0) == -1 and bwd(_ss(0.5), 256) == -1
    # scheduled sampling on together with distillation on: refused by both entries; either one off is in order
    kd = lambda alpha: L.Distill(a, 10, alpha, 2.0, a, None)
    for call in (fwd, bwd):
        assert call(_ss(0.5), kd=kd(0.5)) == -1 and call(_ss(1.0), kd=kd(1.0)) == -1
        assert call(_ss(0.0), kd=kd(0.5)) == -4 and call(_ss(0.5), kd=kd(0.0)) == -4 and call(None, kd=kd(0.5)) == -4
