"""CPU: token-level unlikelihood training.  The float64 restatement (tests/unlikelihoodref.py): its closed-form gradient against
autograd, its candidate sets on hand-made captions, alpha = 0 against tests/smoothref.py; the config key, the module constructor and
the runtime's refusals; the declarations against the ctypes table; the refusals of the two cross-entropy entries and of the two
train-step entries before anything is launched (host buffers stand in for device memory: a call that got past its checks would fail
on the launch, not return -1).  No GPU here."""
import ctypes as C
import os
import re

import pytest
import torch

import smoothref
import unlikelihoodref as ulref
from ssc_runtime import lib as L
from ssc_runtime.engine import check_unlikelihood, check_unlikelihood_distill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 1e-5
NEW = ("ssc_ce_fwd_unlike", "ssc_ce_bwd_unlike", "ssc_train_fwd_unlike", "ssc_train_bwd_unlike")


def rand_case(V, T=6, B=4, seed=0):
    """Captions over a small word range, so that repeats are everywhere; lengths T, T - 1, 2, 1 (cycled)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    y = torch.randint(0, min(V, 5), (T, B), generator=g)
    lengths = [T, T - 1, 2, 1]
    w = torch.tensor([[1.0 if t < lengths[b % 4] else 0.0 for b in range(B)] for t in range(T)], dtype=torch.float64)
    w[1, 0] = 0.0                                       # a position inside a caption that carries no loss
    gl = torch.tensor([0.7, -1.3, 0.25, 0.0], dtype=torch.float64)[:B]
    return x, y, w, gl


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [37, 451, 2003])
@pytest.mark.parametrize("alpha,eps", [(0.5, 0.0), (2.0, 0.1)])
def test_closed_form_gradient_is_autograds(V, alpha, eps):
    x, y, w, gl = rand_case(V)
    assert sum(len(c) for row in ulref.candidates(y, w) for c in row) >= 8
    want = ulref.dlogits_autograd(x, y, w, gl, eps, alpha, DELTA)
    got = ulref.dlogits(x, y, w, gl, eps, alpha, DELTA)
    assert (got - want).abs().max().item() <= 1e-12
    assert bool((got[w == 0] == 0).all()) and bool((got[:, 3] == 0).all())


def test_a_clamped_candidate_has_the_floor_and_no_gradient():
    x, y, w, gl = rand_case(37)
    c = ulref.candidates(y, w)[3][0][0]
    x[3, 0, c] = x[3, 0].max() + 40.0                   # p[c] = 1 - 4e-18 * (sum of the others): far below the clamp
    _, ul, G = ulref.rows(x, y, w, 0.0, 1.0, DELTA)
    others = [k for k in ulref.candidates(y, w)[3][0] if k != c]
    om = ulref.one_minus_p(x[3, 0])
    want = -torch.log(torch.tensor(DELTA, dtype=torch.float64)) - torch.log(om[others]).sum()
    assert abs(ul[3, 0].item() - want.item()) <= 1e-12
    p = torch.softmax(x[3, 0], -1)
    assert abs(G[3, 0].item() - (p[others] / om[others]).sum().item()) <= 1e-12      # the clamped one adds nothing to G
    want = ulref.dlogits_autograd(x, y, w, gl, 0.1, 2.0, DELTA)
    assert (ulref.dlogits(x, y, w, gl, 0.1, 2.0, DELTA) - want).abs().max().item() <= 1e-12
    smallest, clamped = ulref.check_margins(x, y, w, DELTA)
    assert clamped == 1 and smallest >= 0.05
    x[4, 0, ulref.candidates(y, w)[4][0][0]] = x[4, 0].max() + 8.0      # 1 - p of about 1e-3: inside the band float32 cannot decide
    with pytest.raises(AssertionError):
        ulref.check_margins(x, y, w, DELTA)


def test_hand_made_candidate_sets():
    #               b=0        b=1                      b=2                  b=3                       b=4
    # captions:     5 7 5 9    3 3 3 (target repeats)   4 [6: w = 0] 8 6     2 2 6 2 (dup in context)  1 (one word)
    y = torch.tensor([[5, 3, 4, 2, 1],
                      [7, 3, 6, 2, 0],
                      [5, 3, 8, 6, 0],
                      [9, 0, 6, 2, 0]])
    w = torch.tensor([[1, 1, 1, 1, 1],
                      [1, 1, 0, 1, 0],
                      [1, 1, 1, 1, 0],
                      [1, 0, 1, 1, 0]], dtype=torch.float64)
    c = ulref.candidates(y, w)
    assert c[0] == [[], [], [], [], []]                                 # step 0: empty
    assert c[1][0] == [5] and c[2][0] == [7] and c[3][0] == [5, 7]      # a repeat: at t = 2 the target 5 itself is excluded
    assert c[1][1] == [] and c[2][1] == []                              # a repeat of the current target only
    assert c[3][1] == []                                                # w = 0 row: no term
    assert c[1][2] == [] and c[2][2] == [4] and c[3][2] == [4, 8]       # the w = 0 position's 6 never becomes a candidate
    assert c[2][3] == [2] and c[3][3] == [6]                            # 2 twice in the context: once, and excluded as the target
    assert c[1][4] == c[2][4] == c[3][4] == []                          # padding
    V = 11
    x = torch.randn(4, 5, V, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    _, ul, G = ulref.rows(x, y, w, 0.0, 1.0, DELTA)
    p = torch.softmax(x, -1)
    assert abs(ul[3, 0].item() + (torch.log1p(-p[3, 0, 5]) + torch.log1p(-p[3, 0, 7])).item()) <= 1e-12
    assert abs(ul[2, 3].item() + torch.log1p(-p[2, 3, 2]).item()) <= 1e-12
    assert abs(G[2, 3].item() - (p[2, 3, 2] / (1 - p[2, 3, 2])).item()) <= 1e-12
    assert ul[0].abs().max().item() == 0 and ul[:, 1].abs().max().item() == 0 and ul[:, 4].abs().max().item() == 0
    m = ulref.margins(x, y, w)
    assert m.numel() == sum(len(k) for row in c for k in row) == 9


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_alpha_zero_is_smoothref(eps):
    x, y, w, gl = rand_case(90)
    l, ul = ulref.loss(x, y, w, eps, 0.0, DELTA)
    assert torch.equal(l, smoothref.loss(x, y, w, eps)) and float(ul.max()) > 0
    assert torch.equal(ulref.dlogits(x, y, w, gl, eps, 0.0, DELTA), smoothref.dlogits(x, y, w, gl, eps))
    la, _ = ulref.loss(x, y, w, eps, 0.5, DELTA)
    assert (la - (l + 0.5 * ul)).abs().max().item() <= 1e-12


def test_skipped_rows_are_never_read_by_the_reference():
    x, y, w, gl = rand_case(37)
    l0, u0 = ulref.loss(x, y, w, 0.1, 0.5, DELTA)
    x2 = x.clone()
    x2[w == 0] = float("nan")
    l1, u1 = ulref.loss(x2, y, w, 0.1, 0.5, DELTA)
    assert torch.equal(l0, l1) and torch.equal(u0, u1)
    assert torch.equal(ulref.dlogits(x2, y, w, gl, 0.1, 0.5, DELTA), ulref.dlogits(x, y, w, gl, 0.1, 0.5, DELTA))


# ---- 2. the ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_struct_mirror_the_header():
    lib = L.load()
    cdll = C.CDLL(L.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(cdll, name) and name in L.SYMBOLS
        decl = flat[flat.index("int " + name + "("):]
        assert decl[:decl.index(");")].count(",") + 1 == len(L.SYMBOLS[name][1]), name
    assert L.SYMBOLS["ssc_ce_fwd_unlike"][1][:9] == L.SYMBOLS["ssc_ce_fwd_distill"][1][:9]         # the argument order of the distilled entries
    assert L.SYMBOLS["ssc_ce_fwd_unlike"][1][10:] == L.SYMBOLS["ssc_ce_fwd_distill"][1][10:]
    assert L.SYMBOLS["ssc_ce_bwd_unlike"][1][:11] == L.SYMBOLS["ssc_ce_bwd_distill"][1][:11]
    assert L.SYMBOLS["ssc_ce_fwd_unlike"][1][9] is L.SYMBOLS["ssc_ce_bwd_unlike"][1][11] is C.POINTER(L.Unlikelihood)
    body = flat[:flat.index("} ssc_unlikelihood;")]
    body = body[body.rindex("typedef struct {"):]
    fields = re.findall(r"(?:float\*|float)\s+(\w+);", body)
    assert fields == [f for f, _ in L.Unlikelihood._fields_] == ["alpha", "min_one_minus", "rows", "ul"]
    assert C.sizeof(L.Unlikelihood) == 24
    # ssc_train_opts keeps its 24 bytes while the version is 4: the descriptor travels beside it, behind the opts of the two entries
    body = flat[:flat.index("} ssc_train_opts;")]
    body = body[body.rindex("typedef struct {"):]
    assert re.findall(r"(\w+);", body) == [f for f, _ in L.TrainOpts._fields_] and C.sizeof(L.TrainOpts) == 24
    for name, base in (("ssc_train_fwd_unlike", "ssc_train_fwd_opts"), ("ssc_train_bwd_unlike", "ssc_train_bwd_opts")):
        args, plain = L.SYMBOLS[name][1], L.SYMBOLS[base][1]
        assert args[:-2] == plain[:-1] and args[-2] is C.POINTER(L.Unlikelihood) and args[-1] is plain[-1], name
    assert lib.ssc_version() == 4


def _bufs():
    T, B, V = 2, 2, 5
    f = (C.c_float * (3 * T * B * V))()
    r = (C.c_float * (2 * T * B + B + 4))()
    i = (C.c_int64 * (T * B))()
    return T, B, V, C.addressof(f), C.addressof(r), C.addressof(i), (f, r, i)


def _ul(rows, alpha=0.5, delta=DELTA, ul=None):
    return L.Unlikelihood(alpha, delta, rows, ul)


def test_ce_entries_refuse_bad_arguments_before_anything_is_launched():
    lib = L.load()
    T, B, V, a, r, tg, keep = _bufs()

    def fwd(ul, logits=a, ldl=V, eps=0.1, T_=T, B_=B, V_=V, lse=a, loss=a, targets=tg, w=a, nvalid=a):
        return lib._raw_ssc_ce_fwd_unlike(logits, ldl, targets, w, nvalid, T_, B_, V_, eps, C.byref(ul) if ul is not None else None,
                                          lse, loss, None, None)

    def bwd(ul, logits=a, ldl=V, eps=0.1, T_=T, B_=B, V_=V, lse=a, gl=a, targets=tg, w=a, nvalid=a):
        return lib._raw_ssc_ce_bwd_unlike(logits, ldl, targets, w, nvalid, lse, gl, T_, B_, V_, eps,
                                          C.byref(ul) if ul is not None else None, None)

    good = _ul(r, ul=r + 4 * 2 * T * B)
    for call in (fwd, bwd):
        # everything the smoothed calls refuse, with a descriptor in order, with alpha 0 and with none
        for ul in (good, _ul(r, alpha=0.0), None):
            for eps in (1.0, -0.1, float("nan"), 1.5, float("inf")):
                assert call(ul, eps=eps) == -1, (call.__name__, eps)
            assert call(ul, ldl=V - 1) == -1 and call(ul, logits=None) == -1
            assert call(ul, targets=None) == -1 and call(ul, w=None) == -1 and call(ul, nvalid=None) == -1 and call(ul, lse=None) == -1
            assert call(ul, T_=0) == -1 and call(ul, B_=0) == -1 and call(ul, V_=0) == -1
            assert call(ul, logits=a + 2) == -2
        for alpha in (-0.1, float("nan"), float("inf"), -float("inf")):
            assert call(_ul(r, alpha=alpha)) == -1, alpha
        for delta in (0.0, 1.0, -1e-5, 1.5, float("nan"), float("inf")):
            assert call(_ul(r, delta=delta)) == -1, delta
            assert call(_ul(r, delta=delta, alpha=0.0)) == -1, delta          # refused whatever alpha is
        assert call(_ul(None)) == -1
        assert call(good, T_=257) == -1 and call(_ul(r, alpha=1e-3), T_=257) == -1        # one lane per context position
        assert call(_ul(r + 1)) == -2 and call(_ul(r, ul=r + 3)) == -2
    assert fwd(good, loss=None) == -1 and bwd(good, gl=None) == -1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_ce_fwd_unlike(a, V, tg, a, a, T, B, V, 0.1, C.byref(_ul(r, alpha=-1.0)), a, a, None, None)


def test_train_entries_refuse_bad_unlikelihood_arguments():
    """Everything else is in order and the workspace is too small: arguments that pass end at SSC_EWORKSPACE (before any launch), bad
    ones at SSC_EINVAL / SSC_EALIGN - both options on through ssc_train_fwd_unlike among them: that check precedes any device access."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    p = L.Params()
    for name, typ in L.Params._fields_:
        setattr(p, name, 4 if typ is C.c_int else a)
    bt = L.Batch(2, 3, 4, a, a, a, a, None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    kd_on = L.Distill(a, 10, 0.5, 2.0, a, None)
    kd_off = L.Distill(None, 0, 0.0, 1.0, None, None)
    ss_on = L.SchedSampling(0.5, L.SamplerDesc(0, 0, 1.0, 1.0, 7))

    def ref(ul, kd=None, ss=None):
        opts = L.TrainOpts(0.0, 0, C.pointer(ss) if ss is not None else None, C.pointer(kd) if kd is not None else None)
        return C.byref(opts), (C.byref(ul) if ul is not None else None)
    calls = {
        "fwd": lambda *o: lib._raw_ssc_train_fwd_unlike(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, *ref(*o), None),
        "bwd": lambda *o: lib._raw_ssc_train_bwd_unlike(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), 15, *ref(*o), None),
        "phases": lambda *o: lib._raw_ssc_train_bwd_unlike(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), 16, *ref(*o), None),
    }
    for name, call in calls.items():
        assert call(None) == -4 and call(_ul(a)) == -4 and call(_ul(a, ul=a)) == -4 and call(_ul(None, alpha=0.0)) == -4, name
        assert call(_ul(a), kd_off) == -4 and call(_ul(a, alpha=0.0), kd_on) == -4, name      # one of the two off: they do not meet
        assert call(_ul(a), None, ss_on) == -4, name                                        # composes with scheduled sampling
        assert call(_ul(a), kd_on) == -1, name                                              # both on
        for alpha in (-0.1, float("nan"), float("inf")):
            assert call(_ul(a, alpha=alpha)) == -1, (name, alpha)
        for delta in (0.0, 1.0, float("nan")):
            assert call(_ul(a, delta=delta)) == -1 and call(_ul(a, delta=delta, alpha=0.0)) == -1, (name, delta)
        assert call(_ul(None)) == -1 and call(_ul(a + 1)) == -2 and call(_ul(a, ul=a + 2)) == -2, name
    # the scratch is the caller's: the workspace is what it was
    assert lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4) > 0
    long_bt = L.Batch(2, 3, 256, a, a, a, a, None)             # T = L + 1 = 257 steps: refused with the term on, not without it
    assert lib._raw_ssc_train_fwd_unlike(C.byref(cfg), C.byref(p), C.byref(long_bt), a, 1 << 40, a, a, *ref(_ul(a)), None) == -1
    assert lib._raw_ssc_train_fwd_unlike(C.byref(cfg), C.byref(p), C.byref(long_bt), a, 16, a, a, *ref(_ul(a, alpha=0.0)), None) == -4
    for phases in (0, 256):
        assert lib._raw_ssc_train_bwd_unlike(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), phases, *ref(_ul(a)), None) == -1


# ---- 3. the runtime, the config, the module --------------------------------------------------------------------------------------
def test_check_unlikelihood():
    assert check_unlikelihood(0.5) == (0.5, 1e-5) and check_unlikelihood(0, 0.01) == (0.0, 0.01) and check_unlikelihood(3) == (3.0, 1e-5)
    for alpha in (-0.1, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match=r"unlikelihood must"):
            check_unlikelihood(alpha)
    for delta in (0.0, 1.0, -1e-5, float("nan"), "x", None, False):
        with pytest.raises(ValueError, match="unlikelihood_clamp"):
            check_unlikelihood(0.5, delta)
    check_unlikelihood_distill(0.5, 0.0)
    check_unlikelihood_distill(0.0, 0.5)
    with pytest.raises(ValueError, match=r"(?s)unlikelihood.*distill_alpha"):
        check_unlikelihood_distill(0.5, 0.5)


def test_config_key_and_its_refusals():
    from ssc_runtime.config import Config
    assert Config().OPTIM.UNLIKELIHOOD_ALPHA == 0.0
    assert Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", "0.5"]).OPTIM.UNLIKELIHOOD_ALPHA == 0.5
    assert Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", 2]).OPTIM.UNLIKELIHOOD_ALPHA == 2.0
    assert Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", "0.5", "OPTIM.LABEL_SMOOTHING", "0.1", "OPTIM.FREE_BITS", "0.05",
                         "OPTIM.SCHEDULED_SAMPLING_START", "0"]).OPTIM.UNLIKELIHOOD_ALPHA == 0.5
    for bad in ("-0.1", float("inf"), float("nan")):
        with pytest.raises(ValueError, match=r"OPTIM\.UNLIKELIHOOD_ALPHA"):
            Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", bad])
    with pytest.raises(ValueError):
        Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", "much"])
    with pytest.raises(ValueError, match=r"(?s)OPTIM\.UNLIKELIHOOD_ALPHA.*OPTIM\.DISTILL_ALPHA"):
        Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", "0.5", "OPTIM.DISTILL_ALPHA", "0.5"])
    assert Config(None, ["OPTIM.UNLIKELIHOOD_ALPHA", "0", "OPTIM.DISTILL_ALPHA", "0.5"]).OPTIM.DISTILL_ALPHA == 0.5


def test_captioner_takes_the_value():
    from ssc_runtime.config import Config
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    over = ["MODEL.IMAGE_FEATURE_SIZE", 16, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
            "MODEL.Z_SPACE", 4, "MODEL.USE_CBS", False, "MODEL.MIN_CONSTRAINTS_TO_SATISFY", 0, "DATA.CBS.MAX_GIVEN_CONSTRAINTS", 0]
    voc = Vocabulary.synthetic(20)
    m = UpDownCaptioner.from_config(Config(config_override=over + ["OPTIM.UNLIKELIHOOD_ALPHA", 0.5]), vocabulary=voc, device=None)
    assert (m.unlikelihood, m.unlikelihood_clamp) == (0.5, 1e-5)
    m = UpDownCaptioner.from_config(Config(config_override=over), vocabulary=voc, device=None)
    assert (m.unlikelihood, m.unlikelihood_clamp) == (0.0, 1e-5)
    m = UpDownCaptioner(voc, 16, 8, 8, 8, z_space=4, unlikelihood=1, unlikelihood_clamp=1e-3)
    assert (m.unlikelihood, m.unlikelihood_clamp) == (1.0, 1e-3)
    with pytest.raises(ValueError, match="unlikelihood must"):
        UpDownCaptioner(voc, 16, 8, 8, 8, z_space=4, unlikelihood=-1.0)
    with pytest.raises(ValueError, match="unlikelihood_clamp"):
        UpDownCaptioner(voc, 16, 8, 8, 8, z_space=4, unlikelihood=0.5, unlikelihood_clamp=1.0)
