"""CPU: label smoothing of the cross-entropy - the float64 reference of the GPU tests (tests/smoothref.py) against
torch.nn.functional.cross_entropy(label_smoothing=...), the OPTIM.LABEL_SMOOTHING config key, and the C ABI of ssc_ce_fwd_smooth /
ssc_ce_bwd_smooth: exported, mirrored in ctypes, and refusing bad arguments before anything touches memory (no GPU here)."""
import ctypes as C

import pytest
import torch

import smoothref
from ssc_runtime import lib as L
from ssc_runtime.config import Config


def _case(V, seed):
    g = torch.Generator().manual_seed(seed)
    T, B = 4, 3
    x = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 3.0
    y = torch.randint(0, V, (T, B), generator=g)
    y[0, 0], y[1, 0] = 0, V - 1
    w = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    gl = torch.tensor([0.7, -1.3, 0.25], dtype=torch.float64)
    return x, y, w, gl


@pytest.mark.parametrize("V", [5, 37])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_reference_equals_torch_cross_entropy_with_label_smoothing(eps, V):
    x, y, w, gl = _case(V, 100 + V)
    T, B, _ = x.shape
    xt = x.clone().requires_grad_(True)
    want_rows = torch.nn.functional.cross_entropy(xt.view(T * B, V), y.view(T * B), label_smoothing=eps, reduction="none").view(T, B)
    got_rows = smoothref.rows(x, y, eps)
    assert (got_rows - want_rows.detach()).abs().max().item() <= 1e-12
    n = w.sum(0)
    want_loss = n * ((w * want_rows).sum(0) / (n + 1e-13))
    got_loss = smoothref.loss(x, y, w, eps)
    assert (got_loss - want_loss.detach()).abs().max().item() <= 1e-12
    (gl * want_loss).sum().backward()
    got_grad = smoothref.dlogits(x, y, w, gl, eps)
    assert (got_grad - xt.grad).abs().max().item() <= 1e-12
    assert (got_grad[w == 0] == 0).all()
    # ... and the reference's own autograd agrees with its closed form (the train-step tests differentiate through it)
    xr = x.clone().requires_grad_(True)
    (gl * smoothref.loss(xr, y, w, eps)).sum().backward()
    assert (xr.grad - got_grad).abs().max().item() <= 1e-12


def test_reference_ignores_rows_without_weight():
    x, y, w, gl = _case(37, 7)
    bad = x.clone()
    bad[w == 0] = float("nan")
    assert torch.equal(smoothref.loss(bad, y, w, 0.1), smoothref.loss(x, y, w, 0.1))
    assert torch.equal(smoothref.dlogits(bad, y, w, gl, 0.1), smoothref.dlogits(x, y, w, gl, 0.1))


def test_config_key_default_override_and_refusal():
    assert Config().OPTIM.LABEL_SMOOTHING == 0.0
    assert Config(config_override=["OPTIM.LABEL_SMOOTHING", "0.1"]).OPTIM.LABEL_SMOOTHING == 0.1
    assert Config(config_override=["OPTIM.LABEL_SMOOTHING", 0]).OPTIM.LABEL_SMOOTHING == 0.0
    for bad in ("-0.1", "1.0", "1.5"):
        with pytest.raises(ValueError, match="OPTIM.LABEL_SMOOTHING"):
            Config(config_override=["OPTIM.LABEL_SMOOTHING", bad])


def test_captioner_takes_the_value_from_the_config():
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    over = ["MODEL.IMAGE_FEATURE_SIZE", 16, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
            "MODEL.Z_SPACE", 4, "MODEL.USE_CBS", False, "MODEL.MIN_CONSTRAINTS_TO_SATISFY", 0, "DATA.CBS.MAX_GIVEN_CONSTRAINTS", 0]
    voc = Vocabulary.synthetic(20)
    m = UpDownCaptioner.from_config(Config(config_override=over + ["OPTIM.LABEL_SMOOTHING", 0.1]), vocabulary=voc, device=None)
    assert m.label_smoothing == 0.1
    assert UpDownCaptioner.from_config(Config(config_override=over), vocabulary=voc, device=None).label_smoothing == 0.0
    with pytest.raises(ValueError, match="label_smoothing"):
        UpDownCaptioner(voc, 16, 8, 8, 8, z_space=4, label_smoothing=1.0)


def test_engine_dims_and_cfg_carry_the_field():
    from ssc_runtime.engine import ModelDims, check_label_smoothing
    d = ModelDims(V=10, E=4, H=4, A=4, F=4, Z=4)
    assert d.label_smoothing == 0.0 and d.cfg().label_smoothing == 0.0
    d.label_smoothing = 0.25
    assert d.cfg().label_smoothing == 0.25
    for bad in (-0.1, 1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="label_smoothing"):
            check_label_smoothing(bad)


def test_model_cfg_keeps_its_positional_construction():
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    assert cfg.label_smoothing == 0.0
    assert L.ModelCfg._fields_[-1] == ("label_smoothing", C.c_float)
    lib = L.load()
    base = lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4)
    cfg.label_smoothing = 0.1    # the workspace holds the third block and nll whatever the value
    assert lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4) == base > 0
    ld = C.c_int(0)
    buf = (C.c_float * 16)()
    assert lib.ssc_train_workspace_view(C.byref(cfg), 2, 3, 4, C.addressof(buf), 12, C.byref(ld)) and ld.value == 2
    assert not lib.ssc_train_workspace_view(C.byref(cfg), 2, 3, 4, C.addressof(buf), 13, C.byref(ld))


def test_new_symbols_are_exported_and_in_the_ctypes_table():
    lib = L.load()
    cdll = C.CDLL(L.LIB_PATH)
    for name in ("ssc_ce_fwd_smooth", "ssc_ce_bwd_smooth"):
        assert hasattr(cdll, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][1].count(C.c_float) == 1
    assert len(L.SYMBOLS["ssc_ce_fwd_smooth"][1]) == 13 and len(L.SYMBOLS["ssc_ce_bwd_smooth"][1]) == 12
    assert lib.ssc_version() == 4


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Host buffers stand in for device memory: a call that got past its checks would fail on the launch (no GPU), not return -1."""
    lib = L.load()
    T, B, V = 2, 2, 5
    f = (C.c_float * (3 * T * B * V))()
    i = (C.c_int64 * (T * B))()
    a, t = C.addressof(f), C.addressof(i)

    def fwd(logits=a, ldl=V, eps=0.1, T_=T, B_=B, V_=V, lse=a, loss=a, targets=t, w=a, nvalid=a):
        return lib._raw_ssc_ce_fwd_smooth(logits, ldl, targets, w, nvalid, T_, B_, V_, eps, lse, loss, None, None)

    def bwd(logits=a, ldl=V, eps=0.1, T_=T, B_=B, V_=V, lse=a, gl=a, targets=t, w=a, nvalid=a):
        return lib._raw_ssc_ce_bwd_smooth(logits, ldl, targets, w, nvalid, lse, gl, T_, B_, V_, eps, None)

    for call in (fwd, bwd):
        for eps in (1.0, -0.1, float("nan"), 1.5, float("inf")):
            assert call(eps=eps) == -1, (call.__name__, eps)
        assert call(ldl=V - 1) == -1
        assert call(logits=None) == -1
        assert call(targets=None) == -1 and call(w=None) == -1 and call(nvalid=None) == -1 and call(lse=None) == -1
        assert call(T_=0) == -1 and call(B_=0) == -1 and call(V_=0) == -1
        assert call(logits=None, eps=0.0) == -1 and call(ldl=V - 1, eps=0.0) == -1
    assert fwd(loss=None) == -1 and bwd(gl=None) == -1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_ce_fwd_smooth(a, V, t, a, a, T, B, V, 1.0, a, a, None, None)
