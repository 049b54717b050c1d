"""CPU: ensemble decoding - the float64 restatement of the two combine modes (tests/ensembleref.py), the normalisation of the
weights, and the argument checks of ssc_ensemble_combine_rows / ssc_decode_search_ensemble (made before any launch, so they run
without a GPU), of EnsembleDecodeEngine, of CaptionerEnsemble and of scripts/inference.py's ensemble flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ensembleref as E
from ssc_runtime import lib as L
from ssc_runtime.decode import DecodeEngine, EnsembleDecodeEngine, ensemble_weights
from ssc_runtime.engine import ModelDims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def logsumexp(x):
    m = x.max(-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]


def rows(M, n, V, seed=0):
    return np.random.default_rng(seed).standard_normal((M, n, V)) * 3.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_both_modes_are_normalised(M, mode):
    x = rows(M, 5, 97, seed=M)
    x[0, 0, 3] = -1e30
    w = E.normalise(np.arange(1, M + 1), M)
    out = E.combine(x, w, mode)
    assert out.shape == (5, 97) and np.abs(logsumexp(out)).max() < 1e-12


@pytest.mark.parametrize("mode", [0, 1])
def test_one_member_is_log_softmax(mode):
    x = rows(1, 4, 50)
    assert np.abs(E.combine(x, [1.0], mode) - E.log_softmax64(x[0])).max() < 1e-12


def test_mode_0_with_equal_members_is_the_member():
    x = rows(1, 4, 50)
    out = E.combine(np.repeat(x, 3, axis=0), E.normalise([1, 2, 5], 3), 0)
    assert np.abs(out - E.log_softmax64(x[0])).max() < 1e-12


def test_mode_1_with_a_vanishing_weight_tends_to_member_0():
    x = rows(2, 4, 50)
    want = E.log_softmax64(x[0])
    err = [np.abs(E.combine(x, E.normalise([1.0, e], 2), 1) - want).max() for e in (1e-2, 1e-4, 1e-8)]
    assert err[0] > err[1] > err[2] and err[2] < 1e-6


def test_mode_0_is_the_log_of_the_mean_probability():
    x = rows(3, 4, 20)
    w = E.normalise([3, 1, 2], 3)
    p = np.exp(E.log_softmax64(x))
    assert np.abs(np.exp(E.combine(x, w, 0)) - (w.reshape(3, 1, 1) * p).sum(0)).max() < 1e-14


def test_weights_are_normalised():
    assert ensemble_weights(None, 4) == [0.25] * 4
    w = ensemble_weights([2, 6], 2)
    assert w == [0.25, 0.75] and np.allclose(E.normalise([2, 6], 2), w)
    x = rows(2, 3, 30)
    assert np.array_equal(E.combine(x, E.normalise([2, 6], 2), 0), E.combine(x, E.normalise([1, 3], 2), 0))
    for bad in ([1.0], [1.0, 0.0], [1.0, -1.0], [1.0, float("nan")], [1.0, float("inf")], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="ensemble"):
            ensemble_weights(bad, 2)


def dims(H=16):
    return ModelDims(V=50, E=8, H=H, A=8, F=16, Z=4, S=1, kld_mode=1, pm_scale=0.5, prior_var=1.0)


def test_engine_constructor_checks():
    mk = lambda d: DecodeEngine(d, lambda: L.Params(), "cuda")
    a, b = mk(dims()), mk(dims())
    e = EnsembleDecodeEngine([a, b], weights=[1, 3], mode="logprob")
    assert e.weights == [0.25, 0.75] and e.mode == "logprob" and e.dims == a.dims
    assert EnsembleDecodeEngine([a]).weights == [1.0]
    with pytest.raises(ValueError, match="architecture"):
        EnsembleDecodeEngine([a, mk(dims(H=32))])
    with pytest.raises(ValueError, match="mode"):
        EnsembleDecodeEngine([a, b], mode="mean")
    with pytest.raises(ValueError, match="members"):
        EnsembleDecodeEngine([mk(dims()) for _ in range(9)])
    with pytest.raises(ValueError, match="members"):
        EnsembleDecodeEngine([])
    for bad in ([1.0], [1.0, 0.0], [1.0, float("nan")]):
        with pytest.raises(ValueError, match="weights"):
            EnsembleDecodeEngine([a, b], weights=bad)
    for name in ("sample", "score", "stochastic_beam", "sampled_beam", "diverse_beam", "rules_beam", "attention"):
        with pytest.raises(NotImplementedError, match="ensemble"):
            getattr(e, name)()


def test_captioner_ensemble_checks():
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import CaptionerEnsemble, UpDownCaptioner
    mk = lambda V=50, H=16, **kw: UpDownCaptioner(Vocabulary.synthetic(V), 16, 8, H, 8, beam_size=3, z_space=4, **kw)
    a, b = mk(), mk()
    ens = CaptionerEnsemble([a, b], weights=[1, 1])
    assert not ens.training and not a.training and ens.weights == [0.5, 0.5]
    with pytest.raises(RuntimeError, match="eval"):
        ens.train()
    with pytest.raises(ValueError, match="vocabulary"):
        CaptionerEnsemble([a, mk(V=60)])
    with pytest.raises(ValueError, match="configuration"):
        CaptionerEnsemble([a, mk(H=32)])
    with pytest.raises(ValueError, match="configuration"):
        CaptionerEnsemble([a, mk(max_caption_length=7)])
    with pytest.raises(ValueError, match="mode"):
        CaptionerEnsemble([a, b], mode="x")
    with pytest.raises(ValueError, match="weights"):
        CaptionerEnsemble([a, b], weights=[1.0, -2.0])
    with pytest.raises(ValueError, match="at most 8"):
        CaptionerEnsemble([a] * 9)
    from ssc_runtime import sampling
    with pytest.raises(ValueError, match="beam search only"):
        CaptionerEnsemble([a, mk(diverse_beam=sampling.DiverseBeam(3, 0.5))])


def combine_rc(M=2, V=8, ld=8, ldo=8, logw=(-0.6931472, -0.6931472), mode=0, null_member=False, rows_=2):
    """ssc_ensemble_combine_rows on host buffers: every case here is rejected before a launch (or has no rows), so nothing is read."""
    lib = L.load()
    bufs = [(C.c_float * (rows_ * max(ld, 1) + 4))() for _ in range(max(M, 1))]
    ptrs = (C.c_void_p * max(M, 1))(*[C.addressof(b) for b in bufs])
    if null_member:
        ptrs[max(M, 1) - 1] = None
    lw = (C.c_float * max(M, 1))(*list(logw)[: max(M, 1)] + [0.0] * (max(M, 1) - len(logw)))
    out = (C.c_float * (rows_ * max(ldo, 1) + 4))()
    d = L.EnsembleRowsDesc(M, ptrs, ld, lw, mode)
    return lib._raw_ssc_ensemble_combine_rows(C.byref(d), rows_, V, None, None, 0, C.addressof(out), ldo, None)


def test_combine_rejects_bad_descriptors_without_a_gpu():
    assert combine_rc(rows_=0) == 0            # a valid descriptor over no rows: nothing to launch
    assert combine_rc(M=0) == -1
    assert combine_rc(M=9, logw=(0.0,) * 9) == -1
    assert combine_rc(null_member=True) == -1
    assert combine_rc(V=0) == -1
    assert combine_rc(V=8, ld=7) == -1
    assert combine_rc(V=8, ldo=7) == -1
    assert combine_rc(mode=2) == -1
    assert combine_rc(logw=(0.0, float("nan"))) == -1
    assert combine_rc(logw=(0.0, float("-inf"))) == -1
    lib = L.load()
    assert lib._raw_ssc_ensemble_combine_rows(None, 1, 8, None, None, 0, None, 8, None) == -1


def test_search_ensemble_rejects_bad_descriptors_without_a_gpu():
    """ssc_decode_search_ensemble: M out of range, a NULL member, bad weights, an unknown mode, d->imgbuf != imgbufs[0] and a set
    d->attn are SSC_EINVAL before any launch; the workspace size grows with the members."""
    lib = L.load()
    cfg = dims().cfg()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    sd = L.SearchDesc()
    sd.nimg, sd.R, sd.n_samples, sd.S, sd.beam, sd.per_node, sd.max_steps, sd.end_index = 1, 3, 2, 1, 2, 1, 4, 1
    sd.feats = sd.imgbuf = sd.sentiment = sd.eps0 = sd.eps = sd.predictions = sd.log_probs = sd.ctl = a
    p = L.Params()

    def desc(M=2, weights=(1.0, 1.0), mode=0, img0=a, null_param=False):
        n = max(M, 1)
        params = (C.POINTER(L.Params) * n)(*[C.pointer(p) for _ in range(n)])
        if null_param:
            params[n - 1] = C.POINTER(L.Params)()
        imgs = (C.c_void_p * n)(*([img0] + [a] * (n - 1)))
        w = (C.c_float * n)(*(list(weights) + [1.0] * n)[:n]) if weights is not None else None
        return L.EnsembleDesc(M, params, imgs, w, mode), (params, imgs, w)

    def rc(**kw):
        e, _keep = desc(**kw)
        return lib._raw_ssc_decode_search_ensemble(C.byref(cfg), C.byref(e), C.byref(sd), a, 1 << 40, None)

    one = lib.ssc_decode_search_workspace_bytes(C.byref(cfg), C.byref(sd))
    sizes = [lib.ssc_decode_search_ensemble_workspace_bytes(C.byref(cfg), C.byref(sd), C.byref(desc(M=m)[0])) for m in (1, 2, 3)]
    assert one < sizes[0] < sizes[1] < sizes[2] and sizes[2] - sizes[1] == sizes[1] - sizes[0]
    assert lib.ssc_decode_search_ensemble_workspace_bytes(C.byref(cfg), C.byref(sd), C.byref(desc(M=9)[0])) == 0
    assert rc(M=0) == -1 and rc(M=9) == -1
    assert rc(null_param=True) == -1
    assert rc(weights=(1.0, 0.0)) == -1 and rc(weights=(1.0, -1.0)) == -1 and rc(weights=(1.0, float("nan"))) == -1
    assert rc(mode=2) == -1
    assert rc(img0=a + 16) == -1
    rec = L.AttnRecord(a, a)
    sd.attn = C.pointer(rec)
    assert rc() == -1
    sd.attn = None
    e, _keep = desc()
    assert lib._raw_ssc_decode_search_ensemble(C.byref(cfg), C.byref(e), C.byref(sd), a, 16, None) == -4   # (valid, but no workspace)


SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("args,msg", [
    (["--ensemble-weights", "1", "2"], "need --ensemble-checkpoints"),
    (["--ensemble-mode", "logprob"], "need --ensemble-checkpoints"),
    (["--ensemble-checkpoints", "{ck}"], "needs --checkpoint-path"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints", "{ck}.missing"], "no such checkpoint"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints"] + ["{ck}"] * 8, "at most 8"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints", "{ck}", "--ensemble-weights", "1"], "2 positive finite weights"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints", "{ck}", "--ensemble-weights", "1", "0"], "2 positive finite weights"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints", "{ck}", "--ensemble-weights", "1", "nan"], "2 positive finite weights"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints", "{ck}", "--attention-output", "a.pt"], "beam search only"),
    (["--checkpoint-path", "{ck}", "--ensemble-checkpoints", "{ck}", "--likelihood-samples", "2", "--likelihood-output", "l.json"],
     "beam search only"),
])
def test_inference_script_checks_its_ensemble_flags(tmp_path, args, msg):
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"")
    mod = script_module()
    with pytest.raises(SystemExit, match=msg):
        mod.check_ensemble_args(mod.parser.parse_args(BASE + [x.format(ck=ck) for x in args]))


def test_inference_script_accepts_good_ensemble_flags(tmp_path):
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"")
    mod = script_module()
    ok = ["--checkpoint-path", str(ck), "--ensemble-checkpoints", str(ck), str(ck)]
    assert mod.check_ensemble_args(mod.parser.parse_args(BASE + ok)) == (None, "prob")
    got = mod.check_ensemble_args(mod.parser.parse_args(BASE + ok + ["--ensemble-weights", "1", "2", "3", "--ensemble-mode", "logprob"]))
    assert got == ([1.0, 2.0, 3.0], "logprob")
    assert mod.check_ensemble_args(mod.parser.parse_args(BASE)) == (None, "prob")
    with pytest.raises(SystemExit):   # (argparse: not one of prob | logprob)
        mod.parser.parse_args(BASE + ok + ["--ensemble-mode", "mean"])


def test_inference_script_checks_the_flags_before_anything_else(tmp_path):
    """The script itself: a bad ensemble flag ends it before the configuration is read or a device is touched."""
    r = subprocess.run([sys.executable, SCRIPT] + BASE + ["--ensemble-weights", "1", "2"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "need --ensemble-checkpoints" in r.stderr, r.stderr[-2000:]
