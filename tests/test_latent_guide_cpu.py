"""CPU: latent-guided decoding (include/ssc.h: ssc_latent_guide) - the restatement (tests/guideref.py) against a direct float64
evaluation, the guide builders (LatentGuide.from_encoding / lerp), the Levenshtein reference on hand cases, the bindings against the
header, every refusal of the five new symbols (no launch is reached: no GPU needed), the workspace sizes, and the refusals of the
runtime and of the scripts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guideref as GR
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.decode import DecodeEngine, EnsembleDecodeEngine
from ssc_runtime.engine import ModelDims
from ssc_runtime.guide import Encoding, LatentGuide, caption_match, match_summary
from ssc_runtime.inference import diverse_decode
from test_attention_trace_cpu import model_cfg, sample_opts, score_desc, search_desc, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def rows_case(Z, B, rpe, steps, seed, ld=None):
    rng = np.random.default_rng(seed)
    ld = Z if ld is None else ld
    mean = rng.standard_normal((steps, B, ld)).astype(np.float32)
    var = (rng.random((steps, B, ld)) * 2).astype(np.float32)
    eps = rng.standard_normal((B * rpe, Z)).astype(np.float32)
    sent = rng.integers(-1, 2, B * rpe).astype(np.float32)
    return mean, var, eps, sent


@pytest.mark.parametrize("Z,B,rpe", [(1, 1, 1), (3, 5, 3), (8, 2, 6), (65, 3, 1)])
def test_restatement_against_float64(Z, B, rpe):
    """z = eps sqrt(var) + mean on guided entries, eps sqrt(prior_var) + pm_scale sent on the others: the float32 restatement within
    three roundings of the float64 one, element by element; var None gives the mean exactly; pad columns zero; what lies behind them
    is not written."""
    steps, t = 4, 2
    mean, var, eps, sent = rows_case(Z, B, rpe, steps, seed=Z)
    length = np.array([(b * 2) % (steps + 1) for b in range(B)])
    for ln in (None, length):
        for v in (var, None):
            args = (mean, v, ln, t, eps, sent, 0.5, 1.5, rpe)
            got = GR.guide_rows(*args, ldz=Z + 5)
            want = GR.guide_rows(*args, ldz=Z + 5, dtype=np.float64)
            guided = GR.guided_entries(steps, ln, t, B)
            for r in range(B * rpe):
                b = r // rpe
                if guided[b]:
                    direct = mean[t, b].astype(np.float64) + (eps[r].astype(np.float64) * np.sqrt(var[t, b].astype(np.float64)) if v is not None else 0)
                else:
                    direct = eps[r].astype(np.float64) * np.sqrt(1.5) + 0.5 * sent[r]
                assert np.allclose(want[r, :Z], direct, rtol=1e-15, atol=0)
                if guided[b] and v is None:
                    assert np.array_equal(got[r, :Z], mean[t, b])
            bound = GR.guide_bound(*args)
            assert (np.abs(got[:, :Z].astype(np.float64) - want[:, :Z]) <= 4e-7 * bound + 1e-300).all()
            r4 = (Z + 3) // 4 * 4
            assert (got[:, Z:r4] == 0).all() and np.isnan(got[:, r4:]).all()
    # past the guide's steps every entry is unguided, whatever its length
    assert not GR.guided_entries(steps, None, steps, B).any() and not GR.guided_entries(steps, length, steps + 3, B).any()


def test_restatement_never_reads_what_the_kernel_must_not():
    Z, B, rpe, steps, t = 5, 4, 2, 3, 1
    mean, var, eps, sent = rows_case(Z, B, rpe, steps, seed=9, ld=Z + 3)
    length = np.array([0, 1, 2, 3])                # entries 0, 1 unguided at t = 1
    mean[:, :, Z:] = np.nan
    var[:, :, Z:] = np.nan                         # pad columns of the guide
    mean[t, :2] = np.nan
    var[t, :2] = np.nan                            # the guide of unguided entries
    z = GR.guide_rows(mean, var, length, t, eps, sent, 0.5, 1.0, rpe)
    assert np.isfinite(z).all()
    eps2 = eps.copy()
    eps2[2 * rpe:] = np.nan                        # var None: the noise of guided rows
    z2 = GR.guide_rows(mean, None, length, t, eps2, sent, 0.5, 1.0, rpe)
    assert np.isfinite(z2).all() and np.array_equal(z2[: 2 * rpe], z[: 2 * rpe])


# ---- the caption comparison ------------------------------------------------------------------------------------------------------------
def test_levenshtein_hand_cases():
    lev = GR.levenshtein
    assert lev([], []) == 0 and lev([3, 4], []) == 2 and lev([], [5]) == 1
    assert lev([2, 3, 4], [2, 3, 4]) == 0
    assert lev([2, 3, 4], [2, 9, 4]) == 1            # a substitution
    assert lev([2, 3, 4], [2, 4]) == 1               # a deletion
    assert lev([2, 4], [2, 3, 4]) == 1               # an insertion
    assert lev([2, 3, 4, 5], [3, 4, 5, 2]) == 2      # a rotation: delete at the front, insert at the back
    assert lev([7, 7, 7], [8, 8, 8, 8]) == 4
    assert lev(list("kitten"), list("sitting")) == 3


def test_caption_match_reference_columns():
    pred = np.array([[2, 3, 4, END, 9], [END, 5, 5, 5, 5], [2, 3, -1, 4, 5], [2, 3, 4, 5, 6], [2, 3, 4, END, END]])
    ref = np.array([[2, 3, 4, END], [2, 3, END, END], [2, 3, END, 7], [2, 3, 4, 5], [2, 9, 4, 5]])
    got = GR.caption_match(pred, ref, END)
    assert got.tolist() == [[3, 3, 3, 1, 0],      # equal; what follows the END does not count
                            [0, 2, 0, 0, 2],      # an empty prediction
                            [2, 2, 2, 1, 0],      # a negative id ends the caption as an END does
                            [5, 4, 4, 0, 1],      # no END inside L: all L tokens
                            [3, 4, 2, 0, 2]]
    s = match_summary(torch.from_numpy(got))
    assert s["n_pairs"] == 5 and s["exact_rate"] == pytest.approx(2 / 5)
    assert s["token_accuracy"] == pytest.approx(11 / (3 + 2 + 2 + 5 + 4)) and s["wer"] == pytest.approx(5 / 15)


# ---- the builders ----------------------------------------------------------------------------------------------------------------------
def encoding(T=4, B=3, Z=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return Encoding(torch.randn(T, B, Z, generator=g), torch.randn(T, B, Z, generator=g), torch.randn(T, B, Z, generator=g) * 0.3,
                    torch.tensor([2, 4, 3][:B], dtype=torch.int32))


def test_from_encoding_shapes_and_corners():
    enc = encoding()
    g = LatentGuide.from_encoding(enc)
    assert (g.steps, g.B, g.Z) == (4, 3, 5) and g.var is None and torch.equal(g.mean, enc.z) and torch.equal(g.length, enc.length)
    g = LatentGuide.from_encoding(enc, jitter=0.5, repeat=2)
    assert (g.steps, g.B, g.Z) == (4, 6, 5)
    assert torch.equal(g.mean[:, 0], enc.z[:, 0]) and torch.equal(g.mean[:, 1], enc.z[:, 0]) and torch.equal(g.mean[:, 5], enc.z[:, 2])
    assert torch.allclose(g.var[:, 2], 0.25 * torch.exp(enc.lv[:, 1])) and g.length.tolist() == [2, 2, 4, 4, 3, 3]
    assert g.mean.dtype == torch.float32 and g.length.dtype == torch.int32
    for bad in (dict(jitter=-0.1), dict(jitter=float("nan")), dict(repeat=0)):
        with pytest.raises(ValueError, match="from_encoding"):
            LatentGuide.from_encoding(enc, **bad)
    with pytest.raises(ValueError, match="mean must be"):
        LatentGuide(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="var"):
        LatentGuide(torch.zeros(2, 3, 5), torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="length"):
        LatentGuide(torch.zeros(2, 3, 5), None, torch.zeros(4))
    with pytest.raises(ValueError, match="this call has"):
        LatentGuide(torch.zeros(2, 3, 5)).desc("cpu", 4, 5)
    d, keep = LatentGuide(torch.zeros(2, 3, 5), None, torch.tensor([1, 2, 0])).desc("cpu", 3, 5)
    assert (d.steps, d.ld) == (2, 5) and d.mean == keep[0].data_ptr() and not d.var and d.len == keep[2].data_ptr()


def test_lerp():
    a = LatentGuide.from_encoding(encoding(T=4, seed=1), jitter=1.0)
    b = LatentGuide.from_encoding(encoding(T=6, seed=2))          # no variance: standard deviation 0
    b.length = torch.tensor([6, 1, 3], dtype=torch.int32)
    m = LatentGuide.lerp(a, b, 0.25)
    assert (m.steps, m.B, m.Z) == (4, 3, 5) and m.length.tolist() == [2, 1, 3]
    assert torch.allclose(m.mean, 0.75 * a.mean + 0.25 * b.mean[:4]) and torch.allclose(m.var, (0.75 * a.var.sqrt()) ** 2)
    ends = LatentGuide.lerp(a, b, 0.0), LatentGuide.lerp(a, b, 1.0)
    assert torch.allclose(ends[0].mean, a.mean) and torch.allclose(ends[0].var, a.var)
    assert torch.allclose(ends[1].mean, b.mean[:4]) and float(ends[1].var.abs().max()) == 0.0
    plain = LatentGuide.lerp(LatentGuide(a.mean), LatentGuide(b.mean), 0.5)
    assert plain.var is None and plain.length is None and plain.steps == 4
    assert LatentGuide.lerp(LatentGuide(a.mean), b, 0.5).length.tolist() == [4, 1, 3]      # no length: all of the guide's steps
    with pytest.raises(ValueError, match="different extent"):
        LatentGuide.lerp(a, LatentGuide(torch.zeros(4, 2, 5)), 0.5)
    with pytest.raises(ValueError, match="finite"):
        LatentGuide.lerp(a, b, float("inf"))


# ---- bindings against the header -------------------------------------------------------------------------------------------------------
NEW = ("ssc_latent_guide_rows", "ssc_caption_match", "ssc_decode_search_guided", "ssc_decode_sample_opts", "ssc_decode_score_guided")


def test_bindings_mirror_the_header():
    assert struct_fields("ssc_latent_guide") == [f for f, _ in L.LatentGuideDesc._fields_] == ["steps", "mean", "var", "ld", "len"]
    assert C.sizeof(L.LatentGuideDesc) == 40
    lib = L.load()
    cdll = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(cdll, name), name
    # the guided calls are the plain ones plus the guide, in front of the workspace
    for plain in ("ssc_decode_search", "ssc_decode_score"):
        args, gargs = L.SYMBOLS[plain][1], L.SYMBOLS[plain + "_guided"][1]
        assert gargs[:-3] == args[:-3] + [C.POINTER(L.LatentGuideDesc)] and gargs[-3:] == args[-3:]
    # the sampled decode takes it as the first field behind the size of its options, which travel in the same place
    args, oargs = L.SYMBOLS["ssc_decode_sample"][1], L.SYMBOLS["ssc_decode_sample_opts"][1]
    assert oargs[:-3] == args[:-3] + [C.POINTER(L.SampleOpts)] and oargs[-3:] == args[-3:]
    assert struct_fields("ssc_sample_opts") == [f for f, _ in L.SampleOpts._fields_] and C.sizeof(L.SampleOpts) == 5 * C.sizeof(C.c_void_p)
    assert L.SampleOpts._fields_[1] == ("guide", C.POINTER(L.LatentGuideDesc))
    # the descriptors did not grow: the guide travels beside them
    assert struct_fields("ssc_search_desc")[-1] == "attn" and struct_fields("ssc_score_desc")[-1] == "attn"
    assert lib.ssc_version() == 4


# ---- refusals, without a GPU -----------------------------------------------------------------------------------------------------------
def guide_desc(a, **kw):
    g = L.LatentGuideDesc(steps=3, mean=a, var=a, ld=4, len=a)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


BAD_GUIDES = [dict(steps=0), dict(steps=-2), dict(mean=None), dict(ld=3), dict(ld=0), dict(mean="+1"), dict(var="+2"), dict(len="+3")]


def bad_guide(a, kw):
    return guide_desc(a, **{k: (a + int(v) if isinstance(v, str) else v) for k, v in kw.items()})


def test_guide_rows_refusals():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)   # (never read: every check comes before the launch)
    rows = lambda g, t=0, n=6, rpe=3, Z=4, eps=a, ldeps=4, z=a, ldz=4, sent=a: lib._raw_ssc_latent_guide_rows(
        C.byref(g) if g is not None else None, t, n, rpe, Z, eps, ldeps, sent, 0.5, 1.0, z, ldz, None)
    good = guide_desc(a)
    for kw in BAD_GUIDES:
        assert rows(bad_guide(a, kw)) == -1, kw
    for kw in (dict(t=-1), dict(n=0), dict(n=-6), dict(rpe=0), dict(rpe=4), dict(Z=0), dict(eps=None), dict(z=None), dict(ldeps=3), dict(ldz=3),
               dict(eps=a + 2), dict(z=a + 1), dict(sent=a + 3)):
        assert rows(good, **kw) == -1, kw
    # no guide, or a step past it: the checks of ssc_latent_prior_sample (a NULL eps is one of them)
    assert rows(None, eps=None) == -1 and rows(good, t=3, eps=None) == -1 and rows(guide_desc(a, steps=0), t=5) == -1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_latent_guide_rows(C.byref(guide_desc(a, mean=None)), 0, 6, 3, 4, a, 4, a, 0.5, 1.0, a, 4, None)


def test_caption_match_refusals():
    lib = L.load()
    buf = (C.c_int64 * 64)()
    a = C.addressof(buf)
    call = lambda pred=a, Lp=4, ref=a, Lr=4, n=3, end=1, out=a: lib._raw_ssc_caption_match(pred, Lp, ref, Lr, n, end, out, None)
    for kw in (dict(pred=None), dict(ref=None), dict(out=None), dict(n=-1), dict(Lp=0), dict(Lr=0), dict(Lp=129), dict(Lr=129), dict(Lr=1000),
               dict(end=-1)):
        assert call(**kw) == -1, kw
    assert call(n=0) == 0   # nothing to compare: no launch
    with pytest.raises(ValueError, match="widths"):
        caption_match(torch.zeros(2, 129, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="pred"):
        caption_match(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int64), 1)


def guided_calls(lib, a):
    """-> [(name, descriptor, bytes(cfg, desc), call(cfg, desc, guide (a LatentGuideDesc) or None, workspace_bytes))]"""
    smp = L.SamplerDesc(0, 0, 1.0, 1.0, 3)
    p = L.Params()
    ref = C.byref
    gref = lambda g: ref(g) if g is not None else None
    return [("search", search_desc(a), lib.ssc_decode_search_workspace_bytes,
             lambda c, d, g, n: lib._raw_ssc_decode_search_guided(c, ref(p), d, gref(g), a, n, None)),
            ("search-beam1", search_desc(a, beam=1, per_node=1), lib.ssc_decode_search_workspace_bytes,
             lambda c, d, g, n: lib._raw_ssc_decode_search_guided(c, ref(p), d, gref(g), a, n, None)),
            ("sample", search_desc(a, beam=1, per_node=1), lib.ssc_decode_sample_workspace_bytes,
             lambda c, d, g, n: lib._raw_ssc_decode_sample_opts(c, ref(p), d, ref(smp), ref(sample_opts(guide=g)), a, n, None)),
            ("score", score_desc(a), lib.ssc_decode_score_workspace_bytes,
             lambda c, d, g, n: lib._raw_ssc_decode_score_guided(c, ref(p), d, gref(g), a, n, None))]


def test_guided_decodes_refuse_a_bad_guide_before_any_launch_and_cost_no_workspace():
    """Each guided call, with a descriptor that passes every check and a workspace one byte short: SSC_EWORKSPACE (-4) without a
    guide and with a good one - the guide was accepted, nothing was launched -, SSC_EINVAL (-1) for every bad guide, whatever the
    workspace.  *_workspace_bytes is the unguided call's own function: the same number."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    for name, d, nbytes, call in guided_calls(lib, a):
        n = nbytes(C.byref(cfg), C.byref(d))
        assert n > 0, name
        assert call(C.byref(cfg), C.byref(d), None, n - 1) == -4, name
        for good in (guide_desc(a), guide_desc(a, var=None), guide_desc(a, len=None), guide_desc(a, ld=7, steps=1), guide_desc(a, steps=100)):
            assert call(C.byref(cfg), C.byref(d), good, n - 1) == -4, name
        for kw in BAD_GUIDES:
            g = bad_guide(a, kw)
            assert call(C.byref(cfg), C.byref(d), g, n - 1) == -1, (name, kw)
            assert call(C.byref(cfg), C.byref(d), g, n) == -1, (name, kw)
        # SENTIMENT_VAE = 2: out of scope, with every other input of that configuration in place
        sv2 = model_cfg()
        sv2.kld_mode, sv2.S = 2, 1
        d.obj_atts = a
        assert call(C.byref(sv2), C.byref(d), None, 0) == -4, name
        assert call(C.byref(sv2), C.byref(d), guide_desc(a), 1 << 40) == -1, name
        d.obj_atts = None
        # what the unguided call refuses stays refused
        d.feats = None
        assert call(C.byref(cfg), C.byref(d), guide_desc(a), n) == -1, name


# ---- the runtime's refusals ------------------------------------------------------------------------------------------------------------
def dims(**kw):
    base = dict(V=50, E=8, H=8, A=8, F=8, Z=4, S=0, kld_mode=0, pm_scale=0.0, prior_var=1.0)
    base.update(kw)
    return ModelDims(**base)


def test_decoders_without_guides_name_the_feature():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    g = LatentGuide(torch.zeros(2, 6, 4))
    a = (None, None, 3, 2, 1, 6, 1, None, None)
    for call in (lambda: dec.stochastic_beam(*a, sampling.GumbelSampler(1.0), 1, guide=g),
                 lambda: dec.sampled_beam(*a, sampling.TopKSampler(k=5), 1, guide=g),
                 lambda: dec.diverse_beam(*a, sampling.DiverseBeam(2, 0.5), guide=g),
                 lambda: dec.rules_beam(*a, sampling.DecodeRules(2, 0, 1.0, ()), guide=g),
                 lambda: EnsembleDecodeEngine([dec, DecodeEngine(dims(), lambda: L.Params(), "cuda")]).search(*a, guide=g)):
        with pytest.raises(NotImplementedError, match="latent guides"):
            call()
    sv2 = DecodeEngine(dims(kld_mode=2, S=1), lambda: L.Params(), "cuda")
    with pytest.raises(NotImplementedError, match="latent guides.*SENTIMENT_VAE = 2"):
        sv2._guide_desc(g, 6)
    with pytest.raises(ValueError, match="this call has"):
        dec._guide_desc(g, 4)


def test_diverse_decode_refuses_guides_where_the_decoder_takes_none():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    ens = EnsembleDecodeEngine([dec])
    g = LatentGuide(torch.zeros(2, 6, 4))
    feats = torch.zeros(2, 3, 8)
    base = dict(n_samples=3, beam=2, max_steps=6, boundary_index=1, guide=g)
    for kw in (dict(rules=sampling.DecodeRules(2, 0, 1.0, ())), dict(diverse_beam=sampling.DiverseBeam(2, 0.5)),
               dict(sampler=sampling.TopKSampler(k=5), sampled_beam=True), dict(sampler=sampling.GumbelSampler(1.0))):
        with pytest.raises(NotImplementedError, match="latent guides"):
            diverse_decode(dec, feats, None, **base, **kw)
    with pytest.raises(NotImplementedError, match="latent guides.*ensemble"):
        diverse_decode(ens, feats, None, **base)


# ---- the scripts' refusals -------------------------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script_guide", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("args,msg", [
    (["--exemplar-jitter", "0.5"], "needs --exemplar-tensors"),
    (["--exemplar-tensors", "{f}.missing"], "no such file"),
    (["--exemplar-tensors", "{f}", "--exemplar-jitter", "-1"], "finite standard-deviation factor"),
    (["--exemplar-tensors", "{f}", "--exemplar-jitter", "nan"], "finite standard-deviation factor"),
    (["--exemplar-tensors", "{f}", "--checkpoint-path", "{f}", "--ensemble-checkpoints", "{f}"], "not available with --ensemble-checkpoints"),
])
def test_inference_script_checks_its_exemplar_flags(tmp_path, args, msg):
    f = tmp_path / "ex.pt"
    f.write_bytes(b"")
    mod = script_module()
    with pytest.raises(SystemExit, match=msg):
        mod.check_exemplar_args(mod.parser.parse_args(BASE + [x.format(f=f) for x in args]))


def test_inference_script_reads_exemplar_files(tmp_path):
    mod = script_module()
    f = tmp_path / "ex.pt"
    torch.save({"image_id": [7, 3], "captions": torch.tensor([[2, 3, 0], [4, 0, 0]])}, f)
    assert mod.check_exemplar_args(mod.parser.parse_args(BASE + ["--exemplar-tensors", str(f)])) == 0.0
    assert mod.check_exemplar_args(mod.parser.parse_args(BASE + ["--exemplar-tensors", str(f), "--exemplar-jitter", "0.25"])) == 0.25
    assert mod.check_exemplar_args(mod.parser.parse_args(BASE)) == 0.0
    ex = mod.load_exemplars(str(f), 8)
    assert sorted(ex) == [3, 7] and ex[7].tolist() == [2, 3, 0] and ex[3].dtype == torch.int64
    with pytest.raises(SystemExit, match="MAX_CAPTION_LENGTH"):
        mod.load_exemplars(str(f), 2)
    torch.save({"captions": torch.zeros(2, 3, dtype=torch.int64)}, f)
    with pytest.raises(SystemExit, match="image_id"):
        mod.load_exemplars(str(f), 8)
    torch.save({"image_id": [1], "captions": torch.zeros(2, 3, dtype=torch.int64)}, f)
    with pytest.raises(SystemExit, match="captions must be"):
        mod.load_exemplars(str(f), 8)


def test_train_script_refuses_reconstruction_without_validation_tensors(tmp_path):
    import subprocess
    import sys
    from test_score_gpu import YAML
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0",
                        "--synthetic", "2", "--val-reconstruction"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--val-reconstruction needs --val-tensors" in r.stderr, r.stderr[-2000:]


# ---- the oracle's margins --------------------------------------------------------------------------------------------------------------
def test_oracle_seeds_have_clear_margins():
    """The seeds tests/test_latent_guide_gpu.py compares the guided searches with the oracle on: with the oracle alone, every
    selection of every search (first step, per-row candidates, merges) is decided by more than 2e-4."""
    import test_latent_guide_gpu as G
    from test_attention_trace_gpu import STEPS
    for (variant, name) in G.ORACLE_SEEDS:
        for kind in ("var+len", "short"):
            cfg, params, nimg, ns, beam, per_node, feats, senti, eps0, eps, guide, fsm = G.oracle_case(variant, name, kind)
            _, lp, margin = G.oracle_search(cfg, params, feats, senti, nimg, ns, beam, per_node, STEPS, eps0, eps, guide, fsm)
            assert margin > G.MARGIN, (variant, name, kind, margin)
            assert bool((lp > -1e19).any())
