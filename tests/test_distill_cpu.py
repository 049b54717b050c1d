"""CPU: knowledge distillation.  The float64 restatement (tests/distillref.py) against torch's own F.kl_div + F.cross_entropy and
against autograd, its invariants (kd_row >= 0, 0 for a shifted copy, shift invariance of the teacher, q = 0 entries), the refusals
of the five C entry points before anything is launched (host buffers stand in for device memory: a call that got past its checks
would fail on the launch, not return -1), the runtime's refusals and the argument checks of scripts/train.py.  No GPU here."""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

import distillref
from ssc_runtime import lib as L
from ssc_runtime.engine import Distill, ModelDims, check_distill, check_distill_sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_, B_ = 3, 4
W = torch.tensor([[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0]])


def rand_case(V, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T_, B_, V, generator=g, dtype=dtype) * 3
    s = torch.randn(T_, B_, V, generator=g, dtype=dtype) * 3
    y = torch.randint(0, V, (T_, B_), generator=g)
    gl = torch.tensor([0.7, -1.3, 0.25, 0.0], dtype=dtype)
    return x, s, y, gl


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 90, 1000])
@pytest.mark.parametrize("alpha,tau,eps", [(0.5, 2.0, 0.1), (1.0, 1.0, 0.0), (0.3, 4.0, 0.0), (0.0, 2.0, 0.3)])
def test_reference_is_torchs_kl_div_and_cross_entropy(V, alpha, tau, eps):
    x, s, y, _ = rand_case(V, seed=V)
    row, kd = distillref.rows(x, s, y, eps, alpha, tau)
    want_kd = tau * tau * F.kl_div(torch.log_softmax(x / tau, -1), torch.softmax(s / tau, -1), reduction="none").sum(-1)
    want_ce = F.cross_entropy(x.view(-1, V), y.view(-1), reduction="none", label_smoothing=eps).view(T_, B_)
    assert float((kd - want_kd).abs().max()) <= 1e-12 * max(1.0, float(want_kd.abs().max()))
    want = (1 - alpha) * want_ce + alpha * want_kd
    assert float((row - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    loss, kd_b = distillref.loss(x, s, y, W, eps, alpha, tau)
    n = W.sum(0).double()
    assert float((loss - (W * want).sum(0) * n / (n + 1e-13)).abs().max()) <= 1e-12 * float(loss.abs().max())
    assert float((kd_b - (W * want_kd).sum(0) * n / (n + 1e-13)).abs().max()) <= 1e-12 * max(1.0, float(kd_b.abs().max()))


@pytest.mark.parametrize("alpha,tau,eps", [(0.5, 2.0, 0.1), (1.0, 1.0, 0.0), (0.3, 4.0, 0.2), (1.0, 4.0, 0.1)])
def test_closed_form_gradient_is_autograds(alpha, tau, eps):
    x, s, y, gl = rand_case(90, seed=3)
    s[0, 1, 5] = float("-inf")
    xr = x.clone().requires_grad_(True)
    sr = s.clone().requires_grad_(True)
    loss, _ = distillref.loss(xr, sr, y, W, eps, alpha, tau)
    (loss * gl).sum().backward()
    want = distillref.dlogits(x, s, y, W, gl, eps, alpha, tau)
    assert float((xr.grad - want).abs().max()) <= 1e-12
    assert sr.grad is None or float(sr.grad.abs().max()) == 0.0        # the teacher is a constant
    assert float(want[W == 0].abs().max()) == 0.0 and float(want[:, 3].abs().max()) == 0.0


def test_kd_row_is_nonnegative_and_zero_for_a_shifted_copy():
    x, s, y, gl = rand_case(200, seed=5)
    for tau in (1.0, 2.0, 4.0):
        assert float(distillref.kd_rows(x, s, tau).min()) >= 0.0
        kd = distillref.kd_rows(x, x + 123.0, tau)
        assert float(kd.abs().max()) <= 1e-10
        d = distillref.dlogits(x, x - 7.5, y, W, gl, 0.0, 1.0, tau)
        assert float(d.abs().max()) <= 1e-12
        # only differences within a teacher row matter: raw logits or log-probs, any shift per row
        shift = torch.randn(T_, B_, 1, dtype=torch.float64) * 50
        a = distillref.loss(x, s, y, W, 0.1, 0.5, tau)
        b = distillref.loss(x, s + shift, y, W, 0.1, 0.5, tau)
        c = distillref.loss(x, torch.log_softmax(s, -1), y, W, 0.1, 0.5, tau)
        for u, v in zip(a, b):
            assert float((u - v).abs().max()) <= 1e-9
        for u, v in zip(a, c):
            assert float((u - v).abs().max()) <= 1e-9


def test_entries_without_teacher_mass_contribute_nothing():
    x, s, y, gl = rand_case(50, seed=9)
    s[:, :, 10:20] = float("-inf")
    base = distillref.kd_rows(x, s, 2.0)
    x2 = x.clone()
    x2[:, :, 10:20] = -1e30                                            # whatever the student holds there ...
    keep = torch.ones(50, dtype=torch.bool)
    keep[10:20] = False
    # ... the row is the KL over the other entries, with the student renormalised over ALL entries
    logp = torch.log_softmax(x2 / 2.0, -1)[..., keep]
    logq = torch.log_softmax(s[..., keep] / 2.0, -1)
    want = 4.0 * (logq.exp() * (logq - logp)).sum(-1)
    got = distillref.kd_rows(x2, s, 2.0)
    assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 1e-10
    assert torch.isfinite(base).all()
    x3 = x.clone()
    x3[0, 0, 3] = float("-inf")                                        # a student entry at -inf under positive teacher mass
    assert float(distillref.kd_rows(x3, s, 2.0)[0, 0]) == float("inf")
    s4 = s.clone()
    s4[1, 1, 0] = float("nan")
    l, k = distillref.loss(x, s4, y, W, 0.0, 0.5, 2.0)
    assert torch.isnan(l[1]) and torch.isnan(k[1]) and torch.isfinite(l[[0, 2, 3]]).all()


def test_skipped_rows_are_never_read_by_the_reference():
    x, s, y, gl = rand_case(30, seed=11)
    a = distillref.loss(x, s, y, W, 0.1, 0.5, 2.0)
    x[W == 0] = float("nan")
    s[W == 0] = float("nan")
    b = distillref.loss(x, s, y, W, 0.1, 0.5, 2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(distillref.dlogits(x, s, y, W, gl, 0.1, 0.5, 2.0)).all()


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------------
NEW = ("ssc_ce_fwd_distill", "ssc_ce_bwd_distill", "ssc_train_fwd_opts", "ssc_train_bwd_opts")


def test_new_symbols_and_struct_mirror_the_header():
    lib = L.load()
    cdll = C.CDLL(L.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(cdll, name) and name in L.SYMBOLS
        decl = flat[flat.index("int " + name + "("):]
        assert decl[:decl.index(");")].count(",") + 1 == len(L.SYMBOLS[name][1]), name
    assert len(L.SYMBOLS["ssc_ce_fwd_distill"][1]) == len(L.SYMBOLS["ssc_ce_fwd_smooth"][1]) + 1
    assert len(L.SYMBOLS["ssc_ce_bwd_distill"][1]) == len(L.SYMBOLS["ssc_ce_bwd_smooth"][1]) + 1
    # the descriptor travels as a field of ssc_train_opts (its layout: tests/test_free_bits_cpu.py), a pointer to this struct
    assert dict(L.TrainOpts._fields_)["distill"] is C.POINTER(L.Distill) and L.TrainOpts.distill.offset == 16
    body = flat[:flat.index("} ssc_distill;")]
    body = body[body.rindex("typedef struct {"):]
    fields = re.findall(r"(?:const float\*|float\*|float|int)\s+(\w+);", body)
    assert fields == [f for f, _ in L.Distill._fields_] == ["teacher", "ldt", "alpha", "temperature", "rows", "kd"]
    assert C.sizeof(L.Distill) == 40
    assert lib.ssc_version() == 4
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    base = lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4)      # the scratch is the caller's: the workspace is what it was
    cfg.label_smoothing = 0.1
    assert lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4) == base > 0


def _bufs():
    T, B, V = 2, 2, 5
    f = (C.c_float * (3 * T * B * V))()          # the student's logits
    t = (C.c_float * (3 * T * B * V))()          # the teacher's scores: another buffer
    r = (C.c_float * (3 * T * B + B))()
    i = (C.c_int64 * (T * B))()
    return T, B, V, C.addressof(f), C.addressof(t), C.addressof(r), C.addressof(i), (f, t, r, i)


def _kd(teacher, rows, ldt=5, alpha=0.5, tau=2.0, kd=None):
    return L.Distill(teacher, ldt, alpha, tau, rows, kd)


def test_ce_entries_refuse_bad_arguments_before_anything_is_launched():
    lib = L.load()
    T, B, V, a, t, r, tg, keep = _bufs()

    def fwd(kd, logits=a, ldl=V, eps=0.1, T_=T, B_=B, V_=V, lse=a, loss=a, targets=tg, w=a, nvalid=a):
        return lib._raw_ssc_ce_fwd_distill(logits, ldl, targets, w, nvalid, T_, B_, V_, eps, C.byref(kd) if kd is not None else None,
                                           lse, loss, None, None)

    def bwd(kd, logits=a, ldl=V, eps=0.1, T_=T, B_=B, V_=V, lse=a, gl=a, targets=tg, w=a, nvalid=a):
        return lib._raw_ssc_ce_bwd_distill(logits, ldl, targets, w, nvalid, lse, gl, T_, B_, V_, eps,
                                           C.byref(kd) if kd is not None else None, None)

    good = _kd(t, r)
    for call in (fwd, bwd):
        # everything the plain calls refuse, with a descriptor in order, with alpha 0 and with none
        for kd in (good, _kd(t, r, alpha=0.0), None):
            for eps in (1.0, -0.1, float("nan"), 1.5, float("inf")):
                assert call(kd, eps=eps) == -1, (call.__name__, eps)
            assert call(kd, ldl=V - 1) == -1 and call(kd, logits=None) == -1
            assert call(kd, targets=None) == -1 and call(kd, w=None) == -1 and call(kd, nvalid=None) == -1 and call(kd, lse=None) == -1
            assert call(kd, T_=0) == -1 and call(kd, B_=0) == -1 and call(kd, V_=0) == -1
            assert call(kd, logits=a + 2) == -2
        for alpha in (-0.1, 1.0001, float("nan"), float("inf")):
            assert call(_kd(t, r, alpha=alpha)) == -1, alpha
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            assert call(_kd(t, r, tau=tau)) == -1, tau
            assert call(_kd(t, r, tau=tau, alpha=0.0)) == -1, tau       # refused whatever alpha is
        assert call(_kd(None, r)) == -1 and call(_kd(t, None)) == -1 and call(_kd(t, r, ldt=V - 1)) == -1
        # a teacher range that meets the logits range: the same matrix, one that starts inside it, one that ends inside it
        assert call(_kd(a, r)) == -1
        assert call(_kd(a + 4 * (T * B * V - 1), r)) == -1
        assert call(_kd(a - 4 * (T * B * V - 1), r)) == -1
        assert call(_kd(a, r, ldt=2 * V)) == -1
        assert call(_kd(t + 2, r)) == -2 and call(_kd(t, r + 1)) == -2 and call(_kd(t, r, kd=r + 3)) == -2
    assert fwd(good, loss=None) == -1 and bwd(good, gl=None) == -1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_ce_fwd_distill(a, V, tg, a, a, T, B, V, 0.1, C.byref(_kd(t, r, tau=0.0)), a, a, None, None)


def test_train_entries_refuse_bad_distill_arguments():
    """Everything else is in order and the workspace is too small: arguments that pass end at SSC_EWORKSPACE (before any launch), bad
    ones at SSC_EINVAL / SSC_EALIGN."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    p = L.Params()
    for name, typ in L.Params._fields_:
        setattr(p, name, 4 if typ is C.c_int else a)
    bt = L.Batch(2, 3, 4, a, a, a, a, None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    ref = lambda kd, fb=0.0, mode=0: C.byref(L.TrainOpts(fb, mode, None, C.pointer(kd) if kd is not None else None))
    calls = {
        "fwd": lambda kd, fb=0.0, mode=0: lib._raw_ssc_train_fwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, ref(kd, fb, mode), None),
        "bwd": lambda kd, fb=0.0, mode=0: lib._raw_ssc_train_bwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), 15,
                                                                      ref(kd, fb, mode), None),
        "phases": lambda kd, fb=0.0, mode=0: lib._raw_ssc_train_bwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), 16,
                                                                         ref(kd, fb, mode), None),
    }
    for name, call in calls.items():
        assert call(None) == -4 and call(_kd(a, a, ldt=10)) == -4 and call(_kd(None, None, alpha=0.0)) == -4, name
        assert call(_kd(a, a, ldt=12, alpha=1.0, tau=1.0, kd=a)) == -4, name
        for alpha in (-0.1, 1.5, float("nan")):
            assert call(_kd(a, a, ldt=10, alpha=alpha)) == -1, (name, alpha)
        for tau in (0.0, -2.0, float("nan"), float("inf")):
            assert call(_kd(a, a, ldt=10, tau=tau)) == -1 and call(_kd(a, a, ldt=10, tau=tau, alpha=0.0)) == -1, (name, tau)
        assert call(_kd(None, a, ldt=10)) == -1 and call(_kd(a, None, ldt=10)) == -1 and call(_kd(a, a, ldt=9)) == -1, name
        assert call(_kd(a + 2, a, ldt=10)) == -2 and call(_kd(a, a + 1, ldt=10)) == -2, name
        assert call(_kd(a, a, ldt=10), 0.1, 0) == -1 and call(_kd(a, a, ldt=10), 0.1, 3) == -4     # the free-bits checks are the same helper's
    bad_cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0, 1.5)
    assert lib._raw_ssc_train_fwd_opts(C.byref(bad_cfg), C.byref(p), C.byref(bt), a, 16, a, a, ref(_kd(a, a, ldt=10)), None) == -1
    for phases in (0, 256):
        assert lib._raw_ssc_train_bwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), phases,
                                           ref(_kd(a, a, ldt=10)), None) == -1


# ---- 3. the runtime --------------------------------------------------------------------------------------------------------------
def test_check_distill_and_the_distill_object():
    assert check_distill(0.5, 2) == (0.5, 2.0) and check_distill(0, 1.0) == (0.0, 1.0) and check_distill(1, 0.5) == (1.0, 0.5)
    for alpha in (-0.1, 1.1, float("nan"), "x", None, True):
        with pytest.raises(ValueError, match="distill_alpha"):
            check_distill(alpha, 1.0)
    for tau in (0.0, -1.0, float("nan"), float("inf"), "x", None, False):
        with pytest.raises(ValueError, match="distill_temperature"):
            check_distill(0.5, tau)
    d = Distill(torch.zeros(4, 8), 8, 0.25, 4)
    assert (d.ld, d.alpha, d.temperature) == (8, 0.25, 4.0)
    with pytest.raises(ValueError, match="distill_alpha"):
        Distill(torch.zeros(4, 8), 8, 2.0)
    with pytest.raises(ValueError, match="distill_temperature"):
        Distill(torch.zeros(4, 8), 8, 0.5, 0.0)


def test_distillation_with_scheduled_sampling_names_both():
    check_distill_sampling(0.0, 0.5)
    check_distill_sampling(0.5, 0.0)
    with pytest.raises(ValueError, match=r"(?s)distill.*scheduled sampling"):
        check_distill_sampling(0.5, 0.25)
    # TrainEngine.forward makes this check before it touches anything: no engine state (and no GPU) is needed to reach it
    from ssc_runtime.engine import TrainEngine
    eng = object.__new__(TrainEngine)
    with pytest.raises(ValueError, match=r"(?s)distill.*scheduled sampling"):
        TrainEngine.forward(eng, None, None, None, None, ss_prob=0.25, distill=Distill(torch.zeros(4, 8), 8, 0.5))


DIMS = ModelDims(V=50, E=8, H=8, A=8, F=8, Z=4)


def test_teacher_refuses_bad_members_weights_and_modes():
    from ssc_runtime.distill import DistillTeacher, same_architecture
    sd = {}
    t = DistillTeacher([(sd, DIMS)], student_dims=DIMS)
    assert t.weights == [1.0] and t.mode == "prob"
    t = DistillTeacher([(sd, DIMS), (sd, ModelDims(V=50, E=8, H=8, A=8, F=8, Z=4, gemm_mode=2, label_smoothing=0.1))], (3, 1), "logprob")
    assert t.weights == [0.75, 0.25] and t.mode == "logprob"
    t.check_student(DIMS)
    other = ModelDims(V=51, E=8, H=8, A=8, F=8, Z=4)
    assert not same_architecture(DIMS, other)
    with pytest.raises(ValueError, match="architecture or vocabulary"):
        DistillTeacher([(sd, other)], student_dims=DIMS)
    with pytest.raises(ValueError, match="architecture or vocabulary"):
        DistillTeacher([(sd, DIMS), (sd, ModelDims(V=50, E=8, H=16, A=8, F=8, Z=4))])
    with pytest.raises(ValueError, match="architecture or vocabulary"):
        t.check_student(ModelDims(V=50, E=8, H=8, A=8, F=8, Z=4, tied=True))
    with pytest.raises(ValueError, match="1 .. 8 teachers"):
        DistillTeacher([(sd, DIMS)] * 9)
    with pytest.raises(ValueError, match="1 .. 8 teachers"):
        DistillTeacher([])
    for weights in ((1.0,), (1.0, 0.0), (1.0, -2.0), (1.0, float("nan")), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="weights"):
            DistillTeacher([(sd, DIMS)] * 2, weights)
    with pytest.raises(ValueError, match="unknown mode"):
        DistillTeacher([(sd, DIMS)], mode="mean")
    for member in (sd, (sd,), (sd, "dims"), "checkpoint.pth", None):
        with pytest.raises(ValueError, match="neither a TrainEngine"):
            DistillTeacher([member])


def test_config_keys():
    from ssc_runtime.config import Config
    c = Config()
    assert (c.OPTIM.DISTILL_ALPHA, c.OPTIM.DISTILL_TEMPERATURE, c.OPTIM.DISTILL_MODE) == (0.0, 1.0, "prob")
    c = Config(None, ["OPTIM.DISTILL_ALPHA", "0.5", "OPTIM.DISTILL_TEMPERATURE", "2", "OPTIM.DISTILL_MODE", "logprob"])
    assert (c.OPTIM.DISTILL_ALPHA, c.OPTIM.DISTILL_TEMPERATURE, c.OPTIM.DISTILL_MODE) == (0.5, 2.0, "logprob")
    for key, val in (("OPTIM.DISTILL_ALPHA", "1.5"), ("OPTIM.DISTILL_ALPHA", "-0.1"), ("OPTIM.DISTILL_TEMPERATURE", "0"),
                     ("OPTIM.DISTILL_TEMPERATURE", "-1"), ("OPTIM.DISTILL_MODE", "mean")):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            Config(None, [key, val])


# ---- 4. the script ---------------------------------------------------------------------------------------------------------------
def _train_script(monkeypatch):
    """scripts/train.py as a module; what importing it leaves in the process is undone after the test."""
    import sys
    monkeypatch.setattr(sys, "path", list(sys.path))
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    spec = importlib.util.spec_from_file_location("ssc_train_script_distill", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_script_argument_checks(monkeypatch):
    from ssc_runtime.config import Config
    t = _train_script(monkeypatch)
    base = ["--config", "c", "--gpu-ids", "0"]
    plain = t.parser.parse_args(base)
    assert not hasattr(plain, "distill_checkpoints") and not hasattr(plain, "distill_weights")     # the namespace is what it was
    on = Config(None, ["OPTIM.DISTILL_ALPHA", "0.5", "OPTIM.DISTILL_TEMPERATURE", "2"])
    off = Config()
    assert t.distill_plan(plain, off) is None
    a = t.parser.parse_args(base + ["--distill-checkpoints", "a.pth", "b.pth", "--distill-weights", "0.7", "0.3"])
    assert t.distill_plan(a, on) == (["a.pth", "b.pth"], [0.7, 0.3], 0.5, 2.0, "prob")
    a = t.parser.parse_args(base + ["--distill-checkpoints", "a.pth"])
    assert t.distill_plan(a, on) == (["a.pth"], None, 0.5, 2.0, "prob")
    with pytest.raises(SystemExit, match="DISTILL_ALPHA"):
        t.distill_plan(a, off)                                          # teachers without a weight in the loss
    with pytest.raises(SystemExit, match="--distill-checkpoints"):
        t.distill_plan(plain, on)                                       # a weight without teachers
    with pytest.raises(SystemExit, match="--distill-checkpoints"):
        t.distill_plan(t.parser.parse_args(base + ["--distill-weights", "1"]), off)
    for weights in (["1"], ["1", "0"], ["1", "-1"], ["1", "nan"], ["1", "2", "3"]):
        with pytest.raises(SystemExit, match="--distill-weights"):
            t.distill_plan(t.parser.parse_args(base + ["--distill-checkpoints", "a.pth", "b.pth", "--distill-weights"] + weights), on)
    with pytest.raises(SystemExit, match="1 to 8"):
        t.distill_plan(t.parser.parse_args(base + ["--distill-checkpoints"] + ["a.pth"] * 9), on)
    ss = Config(None, ["OPTIM.DISTILL_ALPHA", "0.5", "OPTIM.SCHEDULED_SAMPLING_START", "0"])
    with pytest.raises(SystemExit, match=r"(?s)distillation.*scheduled sampling"):
        t.distill_plan(a, ss)
