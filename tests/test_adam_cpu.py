"""CPU: the Adam / AdamW step's restatement (tests/adamref.py) against torch.optim on float64 tensors - it is pinned to the real
thing before it judges the device -, the ssc_adam_step declaration and binding, the OPTIM.* keys, and the optimiser state in
torch.optim.Adam's layout (packing helpers of ssc_runtime/engine.py on CPU tensors)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import adamref as R
from ssc_runtime import lib as L
from ssc_runtime.config import Config
from ssc_runtime.engine import (FlatStore, ModelDims, OptimSpec, check_optimizer_state_kind, optimizer_state_kind, pack_adam_state,
                                range_step_count, unpack_adam_state)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8      # taken in float64 on both sides (fp32_scalars=False)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("max_norm", [0.75, 1e4])             # clip active / inactive
@pytest.mark.parametrize("wd", [0.0, 0.001])
@pytest.mark.parametrize("decoupled", [False, True])
def test_restatement_is_torch_adam_and_adamw(decoupled, wd, max_norm):
    g = torch.Generator().manual_seed(11)
    shapes = [(7, 5), (13,), (3, 4)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    state = [(p.detach().numpy().copy(), np.zeros(s), np.zeros(s)) for p, s in zip(ps, shapes)]
    for step in range(1, 6):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
        sq = float(sum((x * x).sum() for x in grads))
        for p, x in zip(ps, grads):
            p.grad = x.clone()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        assert (np.sqrt(sq) > max_norm) == (max_norm < 1)
        for i, (p, x) in enumerate(zip(ps, grads)):
            out = R.step(*state[i][:1], x.numpy(), *state[i][1:], sq, 1.0, max_norm, LR, B1, B2, EPS, wd, decoupled, step,
                         fp32_scalars=False)
            state[i] = (out["p"], out["m"], out["v"])
            st = opt.state[p]
            assert rel(out["p"], p.detach().numpy()) <= 1e-12
            assert rel(out["m"], st["exp_avg"].numpy()) <= 1e-12 and rel(out["v"], st["exp_avg_sq"].numpy()) <= 1e-12
            assert float(st["step"]) == step


def test_restatement_with_a_parameter_frozen_for_two_steps():
    """torch does not count a step for a parameter without a gradient: the frozen one's `step` lags, and so must the caller's."""
    g = torch.Generator().manual_seed(12)
    ps = [torch.nn.Parameter(torch.randn(9, generator=g, dtype=torch.float64)) for _ in range(2)]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.001)
    state = [(p.detach().numpy().copy(), np.zeros(9), np.zeros(9)) for p in ps]
    counts = [0, 0]
    for it in range(1, 6):
        frozen = it <= 2
        grads = [torch.randn(9, generator=g, dtype=torch.float64) for _ in ps]
        live = [0] if frozen else [0, 1]
        ps[1].grad = None
        for i in live:
            ps[i].grad = grads[i].clone()
        sq = float(sum((grads[i] ** 2).sum() for i in live))
        torch.nn.utils.clip_grad_norm_([ps[i] for i in live], 0.5)
        opt.step()
        for i in live:
            counts[i] += 1
            out = R.step(state[i][0], grads[i].numpy(), state[i][1], state[i][2], sq, 1.0, 0.5, LR, B1, B2, EPS, 0.001, False, counts[i],
                         fp32_scalars=False)
            state[i] = (out["p"], out["m"], out["v"])
            assert rel(out["p"], ps[i].detach().numpy()) <= 1e-12
    assert counts == [5, 3] and float(opt.state[ps[0]]["step"]) == 5 and float(opt.state[ps[1]]["step"]) == 3


def test_bound_grows_with_every_error_source():
    z = np.zeros(4)
    base = R.step(z + 1, z + 1, z + 0.5, z + 0.25, 4.0, 1.0, 1.0, LR, B1, B2, EPS, 0.0, False, 3)
    worse = R.step(z + 1, z + 1, z + 0.5, z + 0.25, 4.0, 1.0, 1.0, LR, B1, B2, EPS, 0.0, False, 3, err_in=(1e-7, 1e-7, 1e-7),
                   sq_rel_err=1e-5)
    for k in ("Ep", "Em", "Ev"):
        assert (base[k] > 0).all() and (worse[k] > base[k]).all()
    assert (base["Em"] < 8 * R.U).all() and (base["Ep"] < 64 * R.U).all()     # a few u of values of order 1
    quiet = R.step(z, z, z, z, 4.0, 1.0, 1.0, LR, B1, B2, EPS, 0.5, False, 1)
    assert (quiet["p"] == 0).all() and (quiet["m"] == 0).all() and (quiet["v"] == 0).all()


def test_symbol_is_declared_and_bound_with_matching_types():
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+ssc_adam_step\s*\(([^)]*)\)\s*;", text)
    assert m, "ssc_adam_step is not declared in include/ssc.h"
    ctype = {"float*": C.c_void_p, "const float*": C.c_void_p, "void*": C.c_void_p, "size_t": C.c_size_t, "float": C.c_float, "int": C.c_int}
    want = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    res, args = L.SYMBOLS["ssc_adam_step"]
    assert res is C.c_int and args == want and len(args) == 16
    lib = L.load()
    assert lib.ssc_version() == 4
    assert hasattr(C.CDLL(L.LIB_PATH), "ssc_adam_step")
    # no GPU is needed to be refused: every check comes before the launch
    one = (C.c_float * 4)()
    ok = dict(p=one, g=one, m=one, v=one, n=4, sq=one, gscale=1.0, max_norm=1.0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, dec=0, step=1)
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(sq=None), dict(step=0), dict(step=-3), dict(b1=1.0),
                dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(eps=0.0), dict(eps=-1e-8), dict(lr=-1e-3), dict(wd=-0.1)):
        a = dict(ok, **bad)
        rc = lib._raw_ssc_adam_step(a["p"], a["g"], a["m"], a["v"], a["n"], a["sq"], a["gscale"], a["max_norm"], a["lr"], a["b1"], a["b2"],
                                    a["eps"], a["wd"], a["dec"], a["step"], None)
        assert rc == -1, bad
    # a pointer that is no multiple of 4 is no float pointer: SSC_EALIGN (-2), also before any launch
    odd = C.c_void_p(C.addressof(one) + 2)
    for k in "pgmv":
        a = dict(ok, **{k: odd})
        rc = lib._raw_ssc_adam_step(a["p"], a["g"], a["m"], a["v"], 2, a["sq"], 1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, None)
        assert rc == -2, k


def test_config_keys_defaults_and_refusals():
    c = Config()
    assert c.OPTIM.OPTIMIZER == "sgd" and list(c.OPTIM.ADAM_BETAS) == [0.9, 0.999] and c.OPTIM.ADAM_EPS == 1e-8
    assert c.OPTIM.LR == 0.015 and c.OPTIM.MOMENTUM == 0.9 and c.OPTIM.WEIGHT_DECAY == 0.001      # (untouched)
    c = Config(None, ["OPTIM.OPTIMIZER", "adamw", "OPTIM.ADAM_BETAS", "[0.8, 0.99]", "OPTIM.ADAM_EPS", "1e-6", "OPTIM.LR", "5e-5"])
    assert c.OPTIM.OPTIMIZER == "adamw" and list(c.OPTIM.ADAM_BETAS) == [0.8, 0.99] and c.OPTIM.ADAM_EPS == 1e-6
    with pytest.raises(ValueError, match="OPTIM.OPTIMIZER"):
        Config(None, ["OPTIM.OPTIMIZER", "lion"])
    with pytest.raises(ValueError, match="ADAM_BETAS"):
        Config(None, ["OPTIM.ADAM_BETAS", "[0.9, 1.0]"])
    with pytest.raises(ValueError, match="ADAM_EPS"):
        Config(None, ["OPTIM.ADAM_EPS", "0.0"])
    with pytest.raises(ValueError, match="kind"):
        OptimSpec(kind="lion")
    assert OptimSpec("adam").is_adam and OptimSpec("adamw").is_adam and not OptimSpec().is_adam


# ---- state-dict layout ------------------------------------------------------------------------------------------------------
DIMS = ModelDims(V=23, E=10, H=6, A=5, F=7, Z=3, S=1, kld_mode=1, pm_scale=0.5)       # odd widths: padded rows in the flat layout


def filled_state():
    """An engine-shaped Adam state on the CPU: flat moments (padding columns zero), the decoder LSTM two steps behind."""
    shapes = DIMS.param_shapes()
    store = FlatStore(shapes, "cpu")
    m, v = FlatStore(shapes, "cpu"), FlatStore(shapes, "cpu")
    g = torch.Generator().manual_seed(5)
    for n in shapes:
        m.views[n].copy_(torch.randn(*shapes[n], generator=g))
        v.views[n].copy_(torch.rand(*shapes[n], generator=g))
    names = list(shapes)
    steps = {n: (2 if "_decoder." in n else 4) for n in names}
    return store, m, v, names, steps


def test_state_dict_loads_into_torch_adam_and_round_trips():
    store, m, v, names, steps = filled_state()
    spec = OptimSpec("adam", betas=(0.8, 0.99), eps=1e-6)
    sd = pack_adam_state(names, store.offsets, store.shapes, m.flat, v.flat, steps, 3e-4, spec, 0.001, 17)
    assert sd["iteration"] == 17 and optimizer_state_kind(sd) == "adam"
    grp = sd["param_groups"][0]
    assert grp["betas"] == (0.8, 0.99) and grp["eps"] == 1e-6 and grp["weight_decay"] == 0.001 and grp["amsgrad"] is False
    assert grp["lr"] == 3e-4 and grp["params"] == list(range(len(names))) and grp["decoupled_weight_decay"] is False
    for i, n in enumerate(names):
        st = sd["state"][i]
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == steps[n]
        assert tuple(st["exp_avg"].shape) == tuple(store.shapes[n]) == tuple(st["exp_avg_sq"].shape)
        assert torch.equal(st["exp_avg"], m.views[n]) and torch.equal(st["exp_avg_sq"], v.views[n])
    # the pure round trip: pack -> unpack gives the buffers back bit for bit
    m3, v3 = FlatStore(store.shapes, "cpu"), FlatStore(store.shapes, "cpu")
    assert unpack_adam_state(names, store.offsets, store.shapes, m3.flat, v3.flat, sd) == steps
    assert torch.equal(m3.flat, m.flat) and torch.equal(v3.flat, v.flat)
    # torch accepts it, and steps from it (its step counts advance in place: `sd` is spent after this)
    ps = [torch.nn.Parameter(torch.zeros(*store.shapes[n])) for n in names]
    opt = torch.optim.Adam(ps)
    opt.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    assert opt.param_groups[0]["betas"] == (0.8, 0.99) and float(opt.state[ps[-1]]["step"]) == 2
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert float(opt.state[ps[0]]["step"]) == 5 and float(opt.state[ps[-1]]["step"]) == 3
    # ... and torch's own dict comes back into flat buffers: values, step counts, zero padding
    back = opt.state_dict()
    m2, v2 = FlatStore(store.shapes, "cpu"), FlatStore(store.shapes, "cpu")
    m2.flat.fill_(7.0)
    v2.flat.fill_(7.0)
    got = unpack_adam_state(names, store.offsets, store.shapes, m2.flat, v2.flat, back)
    assert got == {n: steps[n] + 1 for n in names}
    for i, n in enumerate(names):
        assert torch.equal(m2.views[n], back["state"][i]["exp_avg"]) and torch.equal(v2.views[n], back["state"][i]["exp_avg_sq"])
    probe = FlatStore(store.shapes, "cpu")
    for n in names:
        probe.views[n].fill_(1.0)
    pad = probe.flat == 0
    assert int(pad.sum()) > 0 and bool((m2.flat[pad] == 0).all()) and bool((v2.flat[pad] == 0).all())


def test_a_parameter_that_never_stepped_has_no_entry():
    store, m, v, names, steps = filled_state()
    steps = {n: (0 if "_decoder." in n else 3) for n in names}
    sd = pack_adam_state(names, store.offsets, store.shapes, m.flat, v.flat, steps, 1e-3, OptimSpec("adamw"), 0.01, 3)
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
    assert sorted(sd["state"]) == [i for i, n in enumerate(names) if "_decoder." not in n]
    ps = [torch.nn.Parameter(torch.zeros(*store.shapes[n])) for n in names]
    torch.optim.AdamW(ps).load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    m2, v2 = FlatStore(store.shapes, "cpu"), FlatStore(store.shapes, "cpu")
    m2.flat.fill_(7.0)
    assert unpack_adam_state(names, store.offsets, store.shapes, m2.flat, v2.flat, sd) == steps
    assert bool((m2.views[names[-1]] == 0).all())


def test_state_of_the_other_kind_is_refused_by_name():
    store, m, v, names, steps = filled_state()
    adam = pack_adam_state(names, store.offsets, store.shapes, m.flat, v.flat, steps, 1e-3, OptimSpec("adam"), 0.0, 1)
    p = [torch.nn.Parameter(torch.zeros(3))]
    sgd = torch.optim.SGD(p, lr=0.1, momentum=0.9)
    p[0].grad = torch.ones(3)
    sgd.step()
    sgd = sgd.state_dict()
    assert optimizer_state_kind(sgd) == "sgd" and optimizer_state_kind({"state": {}, "param_groups": []}) is None
    with pytest.raises(ValueError, match=r"'sgd'.*'adam'"):
        check_optimizer_state_kind(sgd, "adam")
    with pytest.raises(ValueError, match=r"'sgd'.*'adamw'"):
        check_optimizer_state_kind(sgd, "adamw")
    with pytest.raises(ValueError, match=r"'adam'.*'sgd'"):
        check_optimizer_state_kind(adam, "sgd")
    with pytest.raises(ValueError, match=r"'sgd'.*'adam'"):
        unpack_adam_state(["w"], {"w": (0, 4)}, {"w": (3,)}, torch.zeros(4), torch.zeros(4), sgd)
    check_optimizer_state_kind(adam, "adamw")       # Adam and AdamW keep the same state
    check_optimizer_state_kind(sgd, "sgd")
    check_optimizer_state_kind({"state": {}, "param_groups": []}, "adam")


def test_one_step_count_per_range_and_never_updated_parameters():
    """What load_optimizer_state_dict makes of a range's per-parameter counts: one count; a parameter torch never gave a gradient
    (no entry: 0) joins it; two different non-zero counts are refused with the way out named."""
    assert range_step_count([4, 4, 4]) == 4 and range_step_count([]) == 0 and range_step_count([0, 0]) == 0
    assert range_step_count([4, 0, 4]) == 4 and range_step_count(iter([0, 7])) == 7
    with pytest.raises(ValueError, match=r"\[3, 4\].*--reset-optimizer"):
        range_step_count([4, 3, 0])


def test_spec_overrides_are_resolved_in_one_place():
    assert OptimSpec("sgd").resolve(0.9, 0.001) == (0.9, 0.001)
    assert OptimSpec("sgd", momentum=0.5, weight_decay=0.0).resolve(0.9, 0.001) == (0.5, 0.0)
    assert OptimSpec("adamw", weight_decay=0.02).resolve(0.9, 0.001) == (0.9, 0.02)
