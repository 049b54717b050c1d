"""GPU: knowledge distillation in the cross-entropy train step.  Kernel level: ssc_ce_fwd_distill / ssc_ce_bwd_distill against the
float64 restatement (tests/distillref.py) computed from the same fp32 inputs, at row widths on every path of the kernels (scalar
throughout, 16-byte bulk with and without a tail, misaligned first rows, a teacher matrix laid out as the student's and otherwise),
with skipped rows full of NaN in both matrices, poisoned pad columns, teacher entries at -inf and a student row spread over +-80.
Train step: ssc_train_fwd_opts / ssc_train_bwd_opts (the descriptor in ssc_train_opts) against the CPU oracle, whose per-step logits stay in the autograd graph and are
turned into the distilled loss by distillref; the teachers are oracle parameter sets of other seeds run on the same noise.  Then the
fused step, DistillTeacher, the module and scripts/train.py.
Tolerances are the project's own (tests/test_train_gpu.py): loss and kd 1e-4 + 1e-5 max|ref|, gradients 1e-4 max(scale, 1e-3) + 2e-6."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distillref
import ensembleref
import oracle
import smoothref
from gpuutil import dev, engine_from, maxdiff
from ssc_runtime import lib as L
from ssc_runtime.distill import DistillTeacher
from ssc_runtime.engine import Distill, OptimSpec
from test_label_smoothing_gpu import B_, POISON, SHAPES, STEP, T_, bits, grad_tol, inputs, loss_tol, medium

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = T_ * B_
SENTINEL = 7.25          # what an output buffer holds before a call that must not write it

# ---- 1. kernels -------------------------------------------------------------------------------------------------------------
KSHAPES = SHAPES + [(10000, 10000, 0), (90, 92, 1)]
# the teacher matrix: laid out as the student's, or with a leading dimension and a misalignment of its own
LAYOUTS = ["same", "other"]
COMBOS = [(alpha, tau, eps) for alpha in (0.3, 1.0) for tau in (1.0, 2.0, 4.0) for eps in (0.0, 0.1)]


def teacher_layout(V, ld, off, layout):
    return (ld, off) if layout == "same" else (V + 3, (off + 2) % 4)


@functools.lru_cache(maxsize=None)
def case(V, ld, off):
    """Inputs of one shape - the w and gl patterns of tests/test_label_smoothing_gpu.py::case -; shared, changed by none."""
    g = torch.Generator().manual_seed(2000 + V + ld + off)
    w = torch.tensor([[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0]])          # caption lengths 3, 2, 3, 1
    x = torch.randn(T_, B_, V, generator=g) * 2.0
    x[1, 2] = torch.rand(V, generator=g) * 160.0 - 80.0                                             # spread over +-80: the running max moves
    x[1, 2, V // 2] = 80.0
    s = torch.randn(T_, B_, V, generator=g) * 2.0
    for t, b, v in ((0, 0, 1), (1, 2, 3), (2, 2, V - 1), (0, 1, V // 3)):                           # a few entries, never a whole row
        s[t, b, v] = float("-inf")
    y = torch.randint(0, V, (T_, B_), generator=g)
    y[0, 0], y[0, 1], y[1, 2] = 0, V - 1, V - 1
    gl = torch.tensor([0.7, -1.3, 0.25, 0.0])                                                       # mixed signs, one zero
    # eps = 0 only: one student entry at -1e30 where the teacher is -inf (anywhere else the reference itself is astronomically large)
    x0 = x.clone()
    x0[0, 0, 1] = -1e30
    return dict(V=V, ld=ld, off=off, w=w, y=y, gl=gl, nvalid=w.sum(0), x={0.0: x0, 0.1: x}, s=s)


def padded(c, m, ld, off):
    """The (T, B, V) matrix m as the device sees it: rows of ld floats from `off` on, skipped rows NaN, poison everywhere else."""
    md = m.clone()
    md[c["w"] == 0] = float("nan")
    buf = torch.full((ROWS * ld + 8,), POISON)
    buf[off:off + ROWS * ld].view(ROWS, ld)[:, :c["V"]] = md.view(ROWS, c["V"])
    return buf


def untouched(c, buf, ld, off, rows_too=None):
    """Everything outside the [0, V) columns of the rows still holds the poison; rows_too: the rows themselves hold these bits."""
    V = c["V"]
    b = buf.cpu()
    ok = bool((b[:off] == POISON).all()) and bool((b[off + ROWS * ld:] == POISON).all())
    ok = ok and bool((b[off:off + ROWS * ld].view(ROWS, ld)[:, V:] == POISON).all())
    if rows_too is not None:
        ok = ok and torch.equal(bits(b), bits(rows_too))
    return ok


def run_pair(c, x, s, ldt, offt, alpha, tau, eps, kd_null=False):
    """forward + in-place backward on fresh device copies -> dict of everything the calls wrote (and their return codes)."""
    lib = L.load()
    V, ld, off = c["V"], c["ld"], c["off"]
    xb, sb = padded(c, x, ld, off).cuda(), padded(c, s, ldt, offt).cuda()
    assert xb.data_ptr() % 16 == 0 and sb.data_ptr() % 16 == 0
    y, w, nv, gl = dev(c["y"]), dev(c["w"]), dev(c["nvalid"]), dev(c["gl"])
    lse = torch.full((3 * ROWS,), SENTINEL, device="cuda")
    loss = torch.full((B_,), SENTINEL, device="cuda")
    nll = torch.full((B_,), SENTINEL, device="cuda")
    rows = torch.full((3 * ROWS,), SENTINEL, device="cuda")
    kdb = torch.full((B_,), SENTINEL, device="cuda")
    d = L.Distill(sb[offt:].data_ptr(), ldt, alpha, tau, rows.data_ptr(), kdb.data_ptr())
    kd = None if kd_null else C.byref(d)
    st = L.stream_ptr()
    rc_f = lib._raw_ssc_ce_fwd_distill(L.ptr(xb[off:]), ld, L.ptr(y), L.ptr(w), L.ptr(nv), T_, B_, V, eps, kd, L.ptr(lse), L.ptr(loss),
                                       L.ptr(nll), st)
    rc_b = lib._raw_ssc_ce_bwd_distill(L.ptr(xb[off:]), ld, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(lse), L.ptr(gl), T_, B_, V, eps, kd, st)
    torch.cuda.synchronize()
    grad = xb[off:off + ROWS * ld].view(T_, B_, ld)[:, :, :V]
    return dict(rc=(rc_f, rc_b), xb=xb, sb=sb, sb0=padded(c, s, ldt, offt), lse=lse, loss=loss, nll=nll, rows=rows, kd=kdb, grad=grad)


def lse64(m, tau, live):
    r = torch.logsumexp(m.double() / tau, -1)
    return torch.where(live, r, torch.zeros((), dtype=torch.float64))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V,ld,off", KSHAPES)
def test_kernels_match_float64(V, ld, off, layout):
    c = case(V, ld, off)
    ldt, offt = teacher_layout(V, ld, off, layout)
    w, y, gl, s = c["w"], c["y"], c["gl"], c["s"]
    live = w != 0
    worst = dict(loss=0.0, kd=0.0, grad=0.0)
    for alpha, tau, eps in COMBOS:
        x = c["x"][eps]
        r = run_pair(c, x, s, ldt, offt, alpha, tau, eps)
        assert r["rc"] == (0, 0)
        want_loss, want_kd = distillref.loss(x, s, y, w, eps, alpha, tau)
        want_nll = smoothref.loss(x, y, w, 0.0)
        want_grad = distillref.dlogits(x, s, y, w, gl, eps, alpha, tau)
        got = r["grad"].cpu()
        e = dict(loss=maxdiff(r["loss"], want_loss) / loss_tol(want_loss), kd=maxdiff(r["kd"], want_kd) / loss_tol(want_kd),
                 grad=maxdiff(got, want_grad) / grad_tol(want_grad))
        print(f"V={V} ld={ld} off={off} ldt={ldt} offt={offt} alpha={alpha} tau={tau} eps={eps}: loss err {maxdiff(r['loss'], want_loss):.3e} "
              f"(tol {loss_tol(want_loss):.3e}), kd err {maxdiff(r['kd'], want_kd):.3e} (tol {loss_tol(want_kd):.3e}), nll err "
              f"{maxdiff(r['nll'], want_nll):.3e}, grad err {maxdiff(got, want_grad):.3e} (tol {grad_tol(want_grad):.3e})")
        worst = {k: max(worst[k], e[k]) for k in worst}
        for t in (r["loss"], r["nll"], r["kd"], got, r["lse"], r["rows"]):
            assert torch.isfinite(t).all()
        assert maxdiff(r["loss"], want_loss) <= loss_tol(want_loss)
        assert maxdiff(r["nll"], want_nll) <= loss_tol(want_nll)
        assert maxdiff(r["kd"], want_kd) <= loss_tol(want_kd)
        assert maxdiff(got, want_grad) <= grad_tol(want_grad)
        assert float(want_kd.min()) >= 0.0 and float(r["kd"].min()) >= -loss_tol(want_kd)
        # lse and the three blocks of `rows` against float64
        _, kd_row = distillref.rows(x, s, y, eps, alpha, tau)
        blocks = [(r["lse"][:ROWS], lse64(x, 1.0, live)), (r["rows"][:ROWS], lse64(x, tau, live)),
                  (r["rows"][ROWS:2 * ROWS], lse64(s, tau, live)), (r["rows"][2 * ROWS:], w.double() * kd_row)]
        for have, want in blocks:
            assert maxdiff(have.view(T_, B_), want) <= loss_tol(want), (alpha, tau, eps)
        assert maxdiff(r["lse"][2 * ROWS:].view(T_, B_), w.double() * smoothref.rows(x, y, 0.0)) <= loss_tol(want_nll)
        dead = ~live
        assert bool((bits(got[dead]) == 0).all())                         # skipped rows: exactly +0 over [0, V)
        assert bool((bits(got[:, 3]) == 0).all())                         # gl = 0: zero rows too
        assert bool((r["lse"].view(3, T_, B_).cpu()[:, dead] == 0).all()) and bool((r["rows"].view(3, T_, B_).cpu()[:, dead] == 0).all())
        assert untouched(c, r["xb"], ld, off)
        assert untouched(c, r["sb"], ldt, offt, rows_too=r["sb0"])        # the teacher matrix: not one bit moved
    print(f"V={V} {layout}: worst error / tolerance: loss {worst['loss']:.3f} kd {worst['kd']:.3f} grad {worst['grad']:.3f}")


@pytest.mark.parametrize("V,ld,off", [(37, 37, 0), (451, 452, 1), (1024, 1024, 0), (2003, 2004, 0)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_alpha_zero_and_no_descriptor_are_the_smoothed_entries(V, ld, off, eps):
    lib = L.load()
    c = case(V, ld, off)
    x, s = c["x"][0.1], c["s"]
    xb = padded(c, x, ld, off).cuda()
    y, w, nv, gl = dev(c["y"]), dev(c["w"]), dev(c["nvalid"]), dev(c["gl"])
    lse, loss, nll = torch.empty(3 * ROWS, device="cuda"), torch.empty(B_, device="cuda"), torch.empty(B_, device="cuda")
    st = L.stream_ptr()
    lib.ssc_ce_fwd_smooth(L.ptr(xb[off:]), ld, L.ptr(y), L.ptr(w), L.ptr(nv), T_, B_, V, eps, L.ptr(lse), L.ptr(loss), L.ptr(nll), st)
    lib.ssc_ce_bwd_smooth(L.ptr(xb[off:]), ld, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(lse), L.ptr(gl), T_, B_, V, eps, st)
    torch.cuda.synchronize()
    for kd_null, alpha in ((True, 0.5), (False, 0.0)):
        r = run_pair(c, x, s, ld, off, alpha, 2.0, eps, kd_null=kd_null)
        assert r["rc"] == (0, 0)
        for name, t in (("lse", lse), ("loss", loss), ("nll", nll), ("xb", xb)):
            assert torch.equal(bits(r[name]), bits(t)), (name, kd_null)
        assert bool((r["rows"] == SENTINEL).all()) and bool((r["kd"] == SENTINEL).all())     # nothing of kd is written
        assert torch.equal(bits(r["sb"]), bits(r["sb0"]))


@pytest.mark.parametrize("V,ld,off", [(37, 37, 0), (451, 452, 1), (10000, 10000, 0)])
@pytest.mark.parametrize("tau", [1.0, 2.0, 4.0])
def test_a_teacher_that_is_a_bit_copy_of_the_student_has_no_loss_and_no_gradient(V, ld, off, tau):
    c = case(V, ld, off)
    x = c["x"][0.1]
    for ldt, offt in (teacher_layout(V, ld, off, "same"), teacher_layout(V, ld, off, "other")):
        r = run_pair(c, x, x, ldt, offt, 1.0, tau, 0.0)
        assert r["rc"] == (0, 0)
        zeros = torch.zeros(T_, B_, V)
        print(f"V={V} tau={tau} ldt={ldt}: kd max {float(r['kd'].abs().max()):.3e}, |dx| max {float(r['grad'].abs().max()):.3e}")
        assert float(r["kd"].abs().max()) <= loss_tol(torch.zeros(1)) and float(r["loss"].abs().max()) <= loss_tol(torch.zeros(1))
        assert maxdiff(r["grad"], zeros) <= grad_tol(zeros)
        want_nll = smoothref.loss(x, c["y"], c["w"], 0.0)
        assert maxdiff(r["nll"], want_nll) <= loss_tol(want_nll)             # alpha = 1: the hard loss is still reported


@pytest.mark.parametrize("V,ld,off", [(37, 37, 0), (451, 452, 1), (2003, 2004, 0), (10000, 10000, 0)])
def test_two_calls_are_bit_equal(V, ld, off):
    c = case(V, ld, off)
    for layout in LAYOUTS:
        ldt, offt = teacher_layout(V, ld, off, layout)
        a = run_pair(c, c["x"][0.1], c["s"], ldt, offt, 0.3, 2.0, 0.1)
        b = run_pair(c, c["x"][0.1], c["s"], ldt, offt, 0.3, 2.0, 0.1)
        for k in ("lse", "loss", "nll", "rows", "kd", "grad"):
            assert torch.equal(bits(a[k]), bits(b[k])), k


def test_refused_calls_leave_every_output_untouched():
    c = case(451, 452, 0)
    x, s = c["x"][0.1], c["s"]
    clean = padded(c, x, 452, 0)
    for alpha, tau in ((1.5, 2.0), (-0.1, 2.0), (float("nan"), 2.0), (0.5, 0.0), (0.5, -1.0), (0.5, float("inf")), (0.5, float("nan"))):
        r = run_pair(c, x, s, 452, 0, alpha, tau, 0.1)
        assert r["rc"] == (-1, -1), (alpha, tau)
        for k in ("lse", "loss", "nll", "rows", "kd"):
            assert bool((r[k] == SENTINEL).all()), k
        assert torch.equal(bits(r["xb"]), bits(clean)) and torch.equal(bits(r["sb"]), bits(r["sb0"]))
    # a leading dimension below V, a teacher that IS the student's matrix, one that starts inside it
    lib = L.load()
    xb, sb = clean.cuda(), padded(c, s, 452, 0).cuda()
    y, w, nv = dev(c["y"]), dev(c["w"]), dev(c["nvalid"])
    for teacher, ldt in ((sb.data_ptr(), 450), (xb.data_ptr(), 452), (xb.data_ptr() + 4 * 452 * 5, 452)):
        out = torch.full((3 * ROWS + B_,), SENTINEL, device="cuda")
        rows = torch.full((3 * ROWS + B_,), SENTINEL, device="cuda")
        d = L.Distill(teacher, ldt, 0.5, 2.0, rows.data_ptr(), rows[3 * ROWS:].data_ptr())
        rc_f = lib._raw_ssc_ce_fwd_distill(L.ptr(xb), 452, L.ptr(y), L.ptr(w), L.ptr(nv), T_, B_, 451, 0.1, C.byref(d), L.ptr(out),
                                           L.ptr(out[3 * ROWS:]), None, L.stream_ptr())
        rc_b = lib._raw_ssc_ce_bwd_distill(L.ptr(xb), 452, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(out), L.ptr(nv), T_, B_, 451, 0.1,
                                           C.byref(d), L.stream_ptr())
        torch.cuda.synchronize()
        assert (rc_f, rc_b) == (-1, -1)
        assert bool((out == SENTINEL).all()) and bool((rows == SENTINEL).all()) and torch.equal(bits(xb), bits(clean))


# ---- 2. train step ----------------------------------------------------------------------------------------------------------
EPS = 0.1


@functools.lru_cache(maxsize=None)
def teacher_logits(name, seed):
    """(T, B, V) float32: the per-step logits of the oracle under the parameter set of `seed` on the student's minibatch and noise."""
    m = medium(name)
    params = oracle.init_params(m["cfg"], seed=seed)
    with torch.no_grad():
        out = oracle.train_forward(params, m["cfg"], m["feats"], m["caps"], m["senti"], m["eps"], return_steps=True)
    return params, torch.stack([s["logits"] for s in out["steps"]], 0).detach()


def step_weights(name):
    """(T, B) bool: the steps of the minibatch that have a target (the rows anybody reads)."""
    caps = medium(name)["caps"]              # the targets of a caption are its words and the boundary that closes it
    return torch.cat([torch.ones(1, caps.size(0), dtype=torch.bool), caps.t() != 0], 0)


@functools.lru_cache(maxsize=None)
def reference(name, alpha, tau, eps, scores_key):
    """The oracle's forward with its per-step logits in the graph, the distilled loss distillref makes of them against the scores
    SCORES[scores_key] (T, B, V), and the gradients of mean(loss) + mean(kld) / kld_weight."""
    m = medium(name)
    cfg = m["cfg"]
    p = {k: v.clone().requires_grad_(True) for k, v in m["params"].items()}
    out = oracle.train_forward(p, cfg, m["feats"], m["caps"], m["senti"], m["eps"], return_steps=True)
    logits = torch.stack([s["logits"] for s in out["steps"]], 0)
    targets = out["tokens"][:, 1:].t().contiguous()
    w = (targets != cfg.pad_index).double()
    loss, kd = distillref.loss(logits, SCORES[scores_key], targets, w, eps, alpha, tau)
    (loss.mean() + out["kld"].double().mean() / cfg.kld_weight).backward()
    return dict(loss=loss.detach(), kd=kd.detach(), kld=out["kld"].detach(), nll=out["loss"].detach(),
                grads={k: v.grad.clone() for k, v in p.items()})


SCORES = {}


def oracle_scores(name, seed=6):
    key = (name, "oracle", seed)
    if key not in SCORES:
        SCORES[key] = teacher_logits(name, seed)[1]
    return key


def upstream(m):
    B = m["B"]
    return torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * m["cfg"].kld_weight), device="cuda")


def check_against(eng, loss, kld, ref, gl, gk, what):
    print(f"{what}: loss err {maxdiff(loss, ref['loss']):.3e} (tol {loss_tol(ref['loss']):.3e}), kd err {maxdiff(eng.kd(), ref['kd']):.3e} "
          f"(tol {loss_tol(ref['kd']):.3e}), kld err {maxdiff(kld, ref['kld']):.3e}, nll err {maxdiff(eng.nll(), ref['nll']):.3e}")
    assert maxdiff(loss, ref["loss"]) <= loss_tol(ref["loss"])
    assert maxdiff(eng.kd(), ref["kd"]) <= loss_tol(ref["kd"])
    assert maxdiff(kld, ref["kld"]) <= loss_tol(ref["kld"])
    assert maxdiff(eng.nll(), ref["nll"]) <= loss_tol(ref["nll"])
    eng.backward(gl, gk)
    got = eng.grad_dict()
    for k, v in ref["grads"].items():
        if k in eng.frozen_names:      # the tied table is frozen: the engine forms no gradient for it
            continue
        print(f"  {k}: err {maxdiff(got[k], v):.3e} tol {grad_tol(v):.3e}")
        assert maxdiff(got[k], v) <= grad_tol(v), (k, maxdiff(got[k], v), grad_tol(v))
    return got


def scores_on_device(key):
    t = SCORES[key]
    return dev(t.reshape(-1, t.size(-1)).float()), t.size(-1)


@pytest.mark.parametrize("name", ["untied", "tied"])
@pytest.mark.parametrize("alpha,tau,eps", [(0.5, 2.0, EPS), (1.0, 1.0, 0.0)])
def test_train_step_matches_oracle_with_distilled_loss(name, alpha, tau, eps):
    m = medium(name)
    key = oracle_scores(name)
    ref = reference(name, alpha, tau, eps, key)
    eng = engine_from(m["cfg"], m["params"])
    args = inputs(m)
    gl, gk = upstream(m)
    # today's forward / backward: what distill=None and alpha = 0 must reproduce bit for bit
    loss_p, kld_p = (t.clone() for t in eng.forward(*args, label_smoothing=eps))
    eng.backward(gl, gk)
    grads_p = eng.grad_dict()
    sc, ld = scores_on_device(key)
    for off in (None, Distill(sc, ld, 0.0, tau)):
        loss_o, kld_o = (t.clone() for t in eng.forward(*args, label_smoothing=eps, distill=off))
        assert torch.equal(bits(loss_o), bits(loss_p)) and torch.equal(bits(kld_o), bits(kld_p))
        assert float(eng.kd().abs().max()) == 0.0
        eng.backward(gl, gk)
        for k, v in eng.grad_dict().items():
            assert torch.equal(bits(v), bits(grads_p[k])), k
    loss, kld = eng.forward(*args, label_smoothing=eps, distill=Distill(sc, ld, alpha, tau))
    assert torch.equal(bits(kld), bits(kld_p))                     # the latent path does not know about the teacher
    assert maxdiff(loss, loss_p) > 1e-3                            # (the teacher moved the loss)
    got = check_against(eng, loss, kld, ref, gl, gk, f"{name} alpha {alpha} tau {tau} eps {eps}")
    # the phased backward of the data-parallel path keeps the descriptor beside the cfg: the same gradients, bit for bit
    eng.forward(*args, label_smoothing=eps, distill=Distill(sc, ld, alpha, tau))
    eng.backward_phased(gl, gk, (16, 32, 64, 8, 4, 128))
    for k, v in eng.grad_dict().items():
        assert k in eng.frozen_names or torch.equal(bits(v), bits(got[k])), k
    # no state leaks: a forward with label smoothing only, after a distilled one, is the one before it
    loss_a, kld_a = eng.forward(*args, label_smoothing=eps)
    assert torch.equal(bits(loss_a), bits(loss_p)) and torch.equal(bits(kld_a), bits(kld_p))
    eng.backward(gl, gk)
    for k, v in eng.grad_dict().items():
        assert torch.equal(bits(v), bits(grads_p[k])), k


def test_train_entry_refuses_a_teacher_inside_the_workspace_and_sampling():
    m = medium("untied")
    eng = engine_from(m["cfg"], m["params"])
    args = inputs(m)
    loss_p, _ = (t.clone() for t in eng.forward(*args))
    own = eng.workspace_view(9)                                     # the student's own logits block as its teacher
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        eng.forward(*args, distill=Distill(own, own.stride(1), 0.5, 2.0))
    sc, ld = scores_on_device(oracle_scores("untied"))
    with pytest.raises(ValueError, match=r"(?s)distill.*scheduled sampling"):
        eng.forward(*args, ss_prob=0.5, distill=Distill(sc, ld, 0.5, 2.0))
    with pytest.raises(ValueError, match="fewer than"):
        eng.forward(*args, distill=Distill(sc.view(-1)[:-1].clone(), ld, 0.5, 2.0))
    loss_a, _ = eng.forward(*args)
    assert torch.equal(bits(loss_a), bits(loss_p))


def test_fused_step_matches_the_oracle_step_on_the_reference_gradients():
    m = medium("untied")
    key = oracle_scores("untied")
    ref = reference("untied", 0.5, 2.0, EPS, key)
    sc, ld = scores_on_device(key)
    eng = engine_from(m["cfg"], m["params"])
    eng.train_step(*inputs(m), label_smoothing=EPS, distill=Distill(sc, ld, 0.5, 2.0), **STEP)
    want, _, _ = oracle.sgd_clip_step(m["params"], ref["grads"], {}, STEP["lr"], STEP["momentum"], STEP["weight_decay"], STEP["max_norm"])
    sd = eng.state_dict()
    for k, v in want.items():
        assert maxdiff(sd[k], v) < 1e-5, (k, maxdiff(sd[k], v))      # the bound of tests/test_label_smoothing_gpu.py for its step
    plain = engine_from(m["cfg"], m["params"])
    plain.train_step(*inputs(m), label_smoothing=EPS, **STEP)
    assert not torch.equal(plain.params.flat, eng.params.flat)


def test_fused_adam_step_matches_torchs_adam_on_the_reference_gradients():
    """Adam divides the gradient by its own magnitude, so its first step is Lipschitz in the gradient with constant lr / eps: at
    lr = eps = 1e-3 an error delta in a gradient moves the parameter by at most delta - the 2e-6 floor of the gradient tolerance
    stays well inside the 1e-5 bound, and a term missing from the gradient (1e-3 and more here) would not."""
    m = medium("untied")
    key = oracle_scores("untied")
    ref = reference("untied", 0.5, 2.0, EPS, key)
    sc, ld = scores_on_device(key)
    spec = OptimSpec(kind="adam", betas=(0.9, 0.999), eps=1e-3)
    eng = engine_from(m["cfg"], m["params"])
    eng.train_step(*inputs(m), label_smoothing=EPS, distill=Distill(sc, ld, 0.5, 2.0), optim=spec,
                   **{**STEP, "lr": 1e-3})
    ps = {k: torch.nn.Parameter(v.clone().double()) for k, v in m["params"].items()}
    for k, p in ps.items():
        p.grad = ref["grads"][k].clone().double()
    torch.nn.utils.clip_grad_norm_(list(ps.values()), STEP["max_norm"])
    torch.optim.Adam(list(ps.values()), lr=1e-3, betas=spec.betas, eps=spec.eps, weight_decay=STEP["weight_decay"]).step()
    sd = eng.state_dict()
    for k, v in ps.items():
        assert maxdiff(sd[k], v) < 1e-5, (k, maxdiff(sd[k], v))
    assert maxdiff(sd["_output_layer.weight"], m["params"]["_output_layer.weight"]) > 1e-4       # (the step did move the parameters)


def teacher_engines(name, seeds=(6, 7)):
    m = medium(name)
    return [engine_from(m["cfg"], teacher_logits(name, s)[0]) for s in seeds]


def test_one_teacher_returns_its_own_logits_view():
    m = medium("untied")
    (member,) = teacher_engines("untied", (6,))
    t = DistillTeacher([member], student_dims=engine_from(m["cfg"], m["params"]).dims)
    args = inputs(m)
    sc, ld = t.scores(*args)
    view = member.workspace_view(9)
    assert sc.data_ptr() == view.data_ptr() and ld == view.stride(1) and tuple(sc.shape) == tuple(view.shape)
    w = step_weights("untied")
    want = teacher_logits("untied", 6)[1]
    assert maxdiff(sc.cpu()[w], want[w]) <= 1e-3                                 # the member's forward IS the teacher-forced forward
    member.forward(*args)
    assert torch.equal(bits(sc[dev(w)]), bits(member.workspace_view(9)[dev(w)]))


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_two_teachers_are_combined_by_the_ensemble_kernel(mode):
    lib = L.load()
    name = "untied"
    m = medium(name)
    members = teacher_engines(name)
    t = DistillTeacher(members, (0.7, 0.3), mode)
    args = inputs(m)
    sc, ld = t.scores(*args)
    T, B, V = sc.shape
    # a direct ssc_ensemble_combine_rows over the members' logits views: the same bits
    views = [e.workspace_view(9) for e in members]
    out = torch.empty(T * B, ld, device="cuda")
    ptrs = (L.vp * 2)(*[v.data_ptr() for v in views])
    logw = (C.c_float * 2)(math.log(0.7), math.log(0.3))
    d = L.EnsembleRowsDesc(2, ptrs, views[0].stride(1), logw, ensembleref.MODES[mode])
    lib.ssc_ensemble_combine_rows(C.byref(d), T * B, V, None, None, 0, L.ptr(out), ld, L.stream_ptr())
    w = step_weights(name)
    wd = dev(w)
    assert torch.equal(bits(sc[wd]), bits(out.view(T, B, ld)[:, :, :V][wd]))
    # the loss and the gradients against ensembleref + distillref in float64, from the members' own logits
    lg = np.stack([v.cpu().double().numpy().reshape(T * B, V) for v in views])
    lg[:, ~w.view(-1).numpy()] = 0.0                                            # (rows nobody reads may hold anything)
    mix = torch.from_numpy(ensembleref.combine(lg, ensembleref.normalise((0.7, 0.3), 2), ensembleref.MODES[mode])).view(T, B, V)
    assert maxdiff(sc.cpu()[w], mix[w]) <= 1e-4
    key = (name, "mix", mode)
    SCORES[key] = mix
    ref = reference(name, 0.5, 2.0, EPS, key)
    eng = engine_from(m["cfg"], m["params"])
    gl, gk = upstream(m)
    loss, kld = eng.forward(*args, label_smoothing=EPS, distill=t.distill(*args, 0.5, 2.0))
    check_against(eng, loss, kld, ref, gl, gk, f"two teachers, mode {mode}")
    assert t.distill(*args, 0.0, 2.0) is None


def test_composes_with_free_bits_and_label_smoothing():
    import freebitsref as fr
    import test_free_bits_gpu as fb
    m = fb.medium(1, 1)                                  # SENTIMENT_VAE 1, the element floor: its scaled parameters and its floor
    cfg = m["cfg"]
    teacher = oracle.init_params(cfg, seed=6)
    with torch.no_grad():
        tout = oracle.train_forward(teacher, cfg, m["feats"], m["caps"], m["senti"], m["eps"], return_steps=True)
    scores = torch.stack([s["logits"] for s in tout["steps"]], 0)
    p = {k: v.clone().requires_grad_(True) for k, v in m["params"].items()}
    out, k, w = fb._oracle_latents(cfg, p, m["feats"], m["caps"], m["senti"], m["eps"], m["obj"])
    kld, _, _ = fr.floored(k, w, m["lam"], 1)
    logits = torch.stack([s["logits"] for s in out["steps"]], 0)
    targets = out["tokens"][:, 1:].t().contiguous()
    loss, kd = distillref.loss(logits, scores, targets, w, EPS, 0.5, 2.0)
    (loss.mean() + kld.mean() / cfg.kld_weight).backward()
    ref = dict(loss=loss.detach(), kd=kd.detach(), kld=kld.detach(), nll=out["loss"].detach(), grads={n: v.grad.clone() for n, v in p.items()})
    eng = engine_from(cfg, m["params"])
    args = fb.inputs(m)
    gl, gk = fb.upstream(m)
    sc = dev(scores.reshape(-1, scores.size(-1)))
    got_loss, got_kld = eng.forward(*args, label_smoothing=EPS, free_bits=m["lam"], free_bits_mode="element",
                                    distill=Distill(sc, sc.size(1), 0.5, 2.0))
    check_against(eng, got_loss, got_kld, ref, gl, gk, "free bits + label smoothing + distillation")
    assert maxdiff(got_kld, m["raw"]) > 10 * fb.kl_tol(m["kld"])                # (the floor did move the KL)


# ---- 3. module and script ---------------------------------------------------------------------------------------------------
MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.distill import DistillTeacher
from ssc_runtime.engine import Distill
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
def build(seed):
    torch.manual_seed(seed)
    return UpDownCaptioner(Vocabulary.synthetic(120), 64, 40, 48, 32, max_caption_length=8, beam_size=3, z_space=16, sentiment_vae=1,
                           senti_prior_multip=0.5, device=torch.device("cuda")).cuda()
student, t1, t2 = build(1), build(2), build(3)
g = torch.Generator().manual_seed(0)
feats = torch.randn(6, 5, 64, generator=g).cuda()
caps = torch.randint(2, 120, (6, 8), generator=g).cuda()
caps[0, 5:] = 0
senti = torch.randint(-1, 2, (6, 1), generator=g).float().cuda()
eps = torch.randn(9, 6, 16, generator=g)
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32).tolist()
student.train()
student._eps_override = eps
off = student(feats, None, None, caps, senti)
teacher = DistillTeacher([t1._engine(), t2._engine()], (2, 1), "prob", student_dims=student._engine().dims)
student.distill(teacher, 0.5, 2.0)
out = student(feats, None, None, caps, senti)
(out["loss"].mean() + out["kld"].mean() / 750.0).backward()
grad = {{n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}}
# the engine driven by hand on the same inputs: the same loss, the same gradients
eng = student._engine()
d = teacher.distill(feats, caps, senti, eps.cuda(), 0.5, 2.0)
loss, kld = eng.forward(feats, caps, senti, eps.cuda(), distill=d)
B = 6
eng.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * 750.0), device="cuda"))
same_grads = all(torch.equal(grad[n], eng.grads.views[n]) for n in grad)
student.distill(None, 0.0)
again = student(feats, None, None, caps, senti)
try:
    student.distill(teacher, 0.5, 2.0)
    student.scheduled_sampling(0.5, 3)
    student(feats, None, None, caps, senti)
    raised = False
except ValueError as e:
    raised = "scheduled sampling" in str(e)
print(json.dumps({{"same_loss": bits(out["loss"]) == bits(loss), "same_kld": bits(out["kld"]) == bits(kld) == bits(off["kld"]),
                  "kd": out["kd"].tolist(), "moved": bits(out["loss"]) != bits(off["loss"]), "same_grads": same_grads, "n_grads": len(grad),
                  "off_again": bits(again["loss"]) == bits(off["loss"]) and "kd" not in again and "kd" not in off, "raised": raised}}))
"""


def run_child(args, timeout=300):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_module_autograd_path_distils():
    """UpDownCaptioner.distill (in a child process): the training forward returns the engine's distilled loss and kd, backward its
    gradients; off again it is the forward it was; with scheduled sampling it raises."""
    src = MODULE_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "style-seqcvae_amd"))
    got = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    assert got["same_loss"] and got["same_kld"] and got["moved"] and got["same_grads"] and got["n_grads"] > 10
    assert got["off_again"] and got["raised"]
    assert len(got["kd"]) == 6 and all(math.isfinite(v) and v > 0 for v in got["kd"])


def _train(tmp_path, name, extra, fused=True, stop=2, ok=True):
    from test_scripts_gpu import YAML
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    out = tmp_path / name
    args = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--zero-eps", "--serialization-dir", str(out), "--stop-after", str(stop), "--checkpoint-every", "1"] + (
                ["--fused-optimizer"] if fused else []) + extra
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-4000:]
    return out, r


def test_train_script_distils_logs_and_resumes(tmp_path):
    read = lambda d: [json.loads(x) for x in open(d / "scalars.jsonl")]
    t1, _ = _train(tmp_path, "t1", ["--config-override", "RANDOM_SEED", "11"])
    t2, _ = _train(tmp_path, "t2", ["--config-override", "RANDOM_SEED", "12"])
    kd = ["--distill-checkpoints", str(t1 / "checkpoint_2.pth"), str(t2 / "checkpoint_2.pth"), "--distill-weights", "0.7", "0.3"]
    keys = ["--config-override", "OPTIM.DISTILL_ALPHA", "0.5", "OPTIM.DISTILL_TEMPERATURE", "2.0"]
    out, _ = _train(tmp_path, "kd", kd + keys, stop=3)
    log = read(out)
    assert [rec["iteration"] for rec in log] == [1, 2, 3]
    for rec in log:
        assert math.isfinite(rec["kd"]) and rec["kd"] > 0 and math.isfinite(rec["nll"]) and rec["nll"] > 0
        assert abs(rec["nll"] - rec["1reconstr_loss"]) > 1e-6
    assert "DISTILL_ALPHA: 0.5" in open(out / "config.yml").read()
    plain = read(t1)
    assert "kd" not in plain[0] and "nll" not in plain[0]                        # a run without teachers logs what it logged
    # the checkpoint resumes (the teachers are loaded again, the student continues): the log line of iteration 3 again
    res, _ = _train(tmp_path, "resumed", kd + keys + ["--start-from-checkpoint", str(out / "checkpoint_2.pth")], stop=3)
    strip = lambda rec: {k: v for k, v in rec.items() if k != "elapsed_s"}
    assert [strip(rec) for rec in read(res)] == [strip(rec) for rec in log[2:]]
    # the autograd path distils too
    auto, _ = _train(tmp_path, "autograd", kd + keys, fused=False, stop=1)
    a = read(auto)[0]
    assert abs(a["kd"] - log[0]["kd"]) <= 1e-3 * max(1.0, abs(log[0]["kd"])) and abs(a["3loss"] - log[0]["3loss"]) < 1e-3
    # self-critical steps ignore the flags, with a notice; a configured scheduled sampling is an error that names both
    _, r = _train(tmp_path, "scst", kd + keys + ["--scst-references", "synthetic", "--scst-samples", "2", "--scst-max-steps", "8"], stop=1)
    assert "are ignored by the self-critical steps" in r.stdout and "--distill-checkpoints" in r.stdout
    _, r = _train(tmp_path, "ss", kd + keys + ["OPTIM.SCHEDULED_SAMPLING_START", "0"], stop=1, ok=False)
    assert "distillation" in r.stderr and "scheduled sampling" in r.stderr and "Traceback" not in r.stderr
