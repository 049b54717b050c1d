"""GPU: token-level unlikelihood training in the cross-entropy train step.  Kernel level: ssc_ce_fwd_unlike / ssc_ce_bwd_unlike against
the float64 reference (tests/unlikelihoodref.py) computed from the same fp32 logits, at row widths on every path of the kernels
(scalar throughout, 16-byte bulk with and without a tail, a misaligned first row), with repeats planted in the captions, a w = 0
position inside one, a candidate of large probability and a clamped one, skipped rows full of NaN, poisoned pad columns and guard
words around the descriptor's scratch.  Train step: TrainEngine.forward / backward with unlikelihood= against autograd of the
reference objective on the CPU oracle's logits, alone and composed with label smoothing, free bits and scheduled sampling.

The inputs keep every candidate's 1 - p either >= 0.05 or <= delta / 100 (unlikelihoodref.check_margins asserts it before any
comparison): inside that band float32 cannot decide the clamp.  Tolerances are the project's own, imported from
tests/test_label_smoothing_gpu.py: loss 1e-4 + 1e-5 max|ref|, gradients 1e-4 max(scale, 1e-3) + 2e-6."""
import ctypes as C
import functools

import pytest
import torch

import unlikelihoodref as ulref
from gpuutil import dev, dims_from_cfg, maxdiff
from ssc_runtime import lib as L
from ssc_runtime.engine import Distill, TrainEngine
from test_label_smoothing_gpu import EPS, POISON, STEP, bits, grad_tol, loss_tol
from test_label_smoothing_gpu import medium as smooth_medium

pytestmark = pytest.mark.gpu
DELTA = 1e-5
GUARD = 8
SENTINEL = -777.0
ALPHA = 0.5

# ---- 1. kernels -------------------------------------------------------------------------------------------------------------
T_, B_ = 7, 5
LENGTHS = (7, 6, 4, 1, 5)
# (V, ld, offset in floats of the first row from a 16-byte boundary)
SHAPES = [(37, 37, 0), (451, 452, 1), (1024, 1028, 1), (2003, 2004, 0), (10000, 10000, 0)]
WIDE = (70, 2, (70, 40))        # T, B, lengths: candidate lanes in both waves of a row's first 128 lanes


def _finish(V, ld, off, x, y, w, gl):
    T, B = y.shape
    rows = T * B
    xd = x.clone()
    xd[w == 0] = float("nan")                                                                       # skipped rows: never read
    buf = torch.full((rows * ld + 8,), POISON)
    buf[off:off + rows * ld].view(rows, ld)[:, :V] = xd.view(rows, V)
    margin = ulref.check_margins(x, y, w, DELTA)                                                    # the condition of the module docstring
    ref = {}
    for eps in (0.0, 0.1):
        nll = ulref.loss(x, y, w, 0.0, 0.0, DELTA)[0]
        for alpha in (0.5, 2.0):
            loss, ul = ulref.loss(x, y, w, eps, alpha, DELTA)
            _, ul_row, G = ulref.rows(x, y, w, eps, alpha, DELTA)
            ref[alpha, eps] = dict(loss=loss, ul=ul, nll=nll, G=G, wul=w * ul_row, grad=ulref.dlogits(x, y, w, gl, eps, alpha, DELTA))
    return dict(V=V, ld=ld, off=off, T=T, B=B, x=x, w=w.float(), y=y, gl=gl, nvalid=w.sum(0).float(), buf=buf, ref=ref, margin=margin,
                cands=ulref.candidates(y, w))


@functools.lru_cache(maxsize=None)
def case(V, ld, off):
    """Inputs of one shape and their float64 references at every (alpha, eps) the tests use; shared, changed by none."""
    g = torch.Generator().manual_seed(2000 + V + ld + off)
    x = torch.randn(T_, B_, V, generator=g) * 2.0
    y = torch.randint(0, V, (T_, B_), generator=g)
    w = torch.tensor([[1.0 if t < LENGTHS[b] else 0.0 for b in range(B_)] for t in range(T_)], dtype=torch.float64)
    y[2, 0], y[5, 0] = y[0, 0], y[0, 0]            # caption 0: its first word again at steps 2 and 5 (at both it is the target: excluded)
    y[6, 0] = y[1, 0]                              #            ... and the second word at the last step
    y[3, 1] = y[0, 1]                              # caption 1: a repeat; y[1, 1] twice more in the context of its later steps
    y[2, 1] = y[1, 1]
    y[3, 2] = y[1, 2]                              # caption 2: a repeat at its last step
    y[4, 4], y[2, 4] = y[0, 4], y[1, 4]            # caption 4: two repeats
    w[3, 0] = 0.0                                  # a position inside caption 0 without a loss: its word is nobody's candidate
    y[3, 0] = (int(y[4, 0]) + 1) % V if int(y[4, 0]) + 1 != int(y[0, 0]) else (int(y[4, 0]) + 2) % V
    big = int(y[1, 0])                             # a candidate of row (4, 0) raised by 6: its p is large
    x[4, 0, big] += 6.0
    clamp = int(y[0, 1])                           # a candidate of row (4, 1) at the row's maximum + 40: 1 - p is ~1e-17, clamped
    x[4, 1, clamp] = x[4, 1].max() + 40.0
    gl = torch.tensor([0.7, -1.3, 0.25, 0.0, 0.4])                                                  # mixed signs, one zero
    c = _finish(V, ld, off, x, y, w, gl)
    assert big in c["cands"][4][0] and clamp in c["cands"][4][1] and int(y[3, 0]) not in c["cands"][6][0]
    p_big = torch.softmax(x[4, 0].double(), -1)[big]
    assert float(p_big) > 100 * float(torch.softmax((x[4, 0] - 6.0 * torch.nn.functional.one_hot(torch.tensor(big), V)).double(), -1)[big])
    assert c["margin"][1] == 1                                                                      # exactly the planted one is clamped
    return c


@functools.lru_cache(maxsize=None)
def wide_case():
    """T = 70 steps at V = 37: the first 64 positions of the captions use 20 words, the later ones the other 17 as well, so words
    first seen at a position >= 64 are candidates - kept by lanes of the second wave."""
    T, B, lengths = WIDE
    V = 37
    g = torch.Generator().manual_seed(77)
    x = torch.randn(T, B, V, generator=g) * 2.0
    y = torch.randint(0, 20, (T, B), generator=g)
    y[64:] = torch.randint(0, V, (T - 64, B), generator=g)
    w = torch.tensor([[1.0 if t < lengths[b] else 0.0 for b in range(B)] for t in range(T)], dtype=torch.float64)
    w[10, 0] = 0.0
    c = _finish(V, V, 0, x, y, w, torch.tensor([0.7, -1.3]))
    first_seen_late = set(y[64:69, 0].tolist()) - set(y[:64, 0].tolist())
    assert first_seen_late and first_seen_late - {int(y[69, 0])} <= set(c["cands"][69][0])
    return c


def run_pair(c, alpha, eps, delta=DELTA, desc="on", entries="unlike"):
    """forward + in-place backward on a fresh device copy of the case.  desc: "on" | "null" (no descriptor) | "norows" (rows NULL);
    entries: "unlike" | "smooth" (ssc_ce_fwd_smooth / ssc_ce_bwd_smooth).  Every output starts as SENTINEL."""
    lib = L.load()
    V, ld, off, T, B = c["V"], c["ld"], c["off"], c["T"], c["B"]
    rows = T * B
    buf = c["buf"].cuda()
    assert buf.data_ptr() % 16 == 0
    view = buf[off:]
    y, w, nv, gl = dev(c["y"]), dev(c["w"]), dev(c["nvalid"]), dev(c["gl"])
    lse = torch.full((3 * rows,), SENTINEL, device="cuda")
    loss = torch.full((B,), SENTINEL, device="cuda")
    nll = torch.full((B,), SENTINEL, device="cuda")
    scratch = torch.full((GUARD + 2 * rows + B + GUARD,), SENTINEL, device="cuda")
    d = L.Unlikelihood(alpha, delta, None if desc == "norows" else scratch[GUARD:].data_ptr(), scratch[GUARD + 2 * rows:].data_ptr())
    ref = None if desc == "null" else C.byref(d)
    st = L.stream_ptr()
    if entries == "smooth":
        rc = (lib._raw_ssc_ce_fwd_smooth(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), T, B, V, eps, L.ptr(lse), L.ptr(loss), L.ptr(nll), st),
              lib._raw_ssc_ce_bwd_smooth(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(lse), L.ptr(gl), T, B, V, eps, st))
    else:
        rc = (lib._raw_ssc_ce_fwd_unlike(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), T, B, V, eps, ref, L.ptr(lse), L.ptr(loss),
                                         L.ptr(nll), st),
              lib._raw_ssc_ce_bwd_unlike(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(lse), L.ptr(gl), T, B, V, eps, ref, st))
    torch.cuda.synchronize()
    b = buf.cpu()
    body = b[off:off + rows * ld].view(rows, ld)
    outside = bool((b[:off] == POISON).all()) and bool((b[off + rows * ld:] == POISON).all()) and bool((body[:, V:] == POISON).all())
    s = scratch.cpu()
    return dict(rc=rc, buf=b, grad=body[:, :V].reshape(T, B, V), outside=outside, lse=lse.cpu(), loss=loss.cpu(), nll=nll.cpu(),
                G=s[GUARD:GUARD + rows].view(T, B), wul=s[GUARD + rows:GUARD + 2 * rows].view(T, B), ul=s[GUARD + 2 * rows:GUARD + 2 * rows + B],
                guards=torch.cat([s[:GUARD], s[GUARD + 2 * rows + B:]]), scratch=s)


def check_pair(c, alpha, eps, what):
    r = run_pair(c, alpha, eps)
    want = c["ref"][alpha, eps]
    assert r["rc"] == (0, 0)
    fig = {k: (maxdiff(r[k], want[k]), loss_tol(want[k])) for k in ("loss", "nll", "ul", "G", "wul")}
    fig["grad"] = (maxdiff(r["grad"], want["grad"]), grad_tol(want["grad"]))
    print(f"{what} alpha={alpha} eps={eps}: smallest unclamped 1 - p {c['margin'][0]:.3f}; " +
          ", ".join(f"{k} err {e:.3e} (tol {t:.3e}, {e / t:.4f} of it)" for k, (e, t) in fig.items()))
    for k in ("loss", "nll", "ul", "G", "wul", "grad", "lse"):
        assert torch.isfinite(r[k]).all(), k
    for k, (e, t) in fig.items():
        assert e <= t, (k, e, t)
    dead = c["w"] == 0
    assert bool((bits(r["grad"][dead]) == 0).all())                           # skipped rows: exactly +0 over [0, V)
    assert bool((bits(r["grad"][:, c["gl"] == 0]) == 0).all())                # gl = 0: zero rows too
    assert bool((r["lse"].view(3, c["T"], c["B"])[:, dead] == 0).all()) and bool((r["G"][dead] == 0).all()) and bool((r["wul"][dead] == 0).all())
    assert r["outside"] and bool((r["guards"] == SENTINEL).all())
    return r


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("alpha", [0.5, 2.0])
@pytest.mark.parametrize("V,ld,off", SHAPES)
def test_kernels_match_float64(V, ld, off, alpha, eps):
    c = case(V, ld, off)
    r = check_pair(c, alpha, eps, f"V={V} ld={ld} off={off}")
    want = c["ref"][alpha, eps]
    assert float(want["ul"][3]) == 0.0 and float(r["ul"][3]) == 0.0           # the one-word caption has no candidates
    assert float(want["wul"][4, 1]) > 11.5                                    # (the clamped one's -log(delta))


@pytest.mark.parametrize("alpha,eps", [(0.5, 0.1), (2.0, 0.0)])
def test_candidate_lanes_cross_a_wave_boundary(alpha, eps):
    check_pair(wide_case(), alpha, eps, "T=70 B=2 V=37")


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V,ld,off", [(37, 37, 0), (451, 452, 1), (2003, 2004, 0)])
def test_alpha_zero_and_no_descriptor_are_the_smoothed_entries(V, ld, off, eps):
    c = case(V, ld, off)
    want = run_pair(c, 0.0, eps, entries="smooth")
    for desc, alpha in (("on", 0.0), ("null", 0.5), ("norows", 0.0)):
        r = run_pair(c, alpha, eps, desc=desc)
        assert r["rc"] == (0, 0)
        for k in ("lse", "loss", "nll"):
            assert torch.equal(bits(r[k]), bits(want[k])), (desc, k)
        body = lambda t: t["buf"][off:off + T_ * B_ * ld].view(-1, ld)[:, :V][(c["w"] != 0).view(-1)]
        assert torch.equal(bits(body(r)), bits(body(want))) and r["outside"]
        assert bool((r["scratch"] == SENTINEL).all())                         # no buffer of the descriptor is written


@pytest.mark.parametrize("V,ld,off", [(37, 37, 0), (451, 452, 1), (10000, 10000, 0)])
def test_two_calls_are_bit_equal(V, ld, off):
    c = case(V, ld, off)
    a, b = run_pair(c, 2.0, 0.1), run_pair(c, 2.0, 0.1)
    for k in ("lse", "loss", "nll", "G", "wul", "ul"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    live = c["w"] != 0
    assert torch.equal(bits(a["grad"][live]), bits(b["grad"][live]))


def test_refused_calls_leave_every_output_untouched():
    c = case(451, 452, 1)
    clean = c["buf"]
    bad = [dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=0.5, delta=0.0), dict(alpha=0.5, delta=1.0),
           dict(alpha=0.5, delta=float("nan")), dict(alpha=0.0, delta=2.0), dict(alpha=0.5, desc="norows"), dict(alpha=0.5, eps=1.0)]
    for kw in bad:
        kw = dict(dict(eps=0.1), **kw)
        r = run_pair(c, **kw)
        assert r["rc"] == (-1, -1), kw
        for k in ("lse", "loss", "nll", "scratch"):
            assert bool((r[k] == SENTINEL).all()), (kw, k)
        assert torch.equal(bits(torch.nan_to_num(r["buf"], nan=3.0)), bits(torch.nan_to_num(clean, nan=3.0))), kw


# ---- 2. train step ----------------------------------------------------------------------------------------------------------
def with_repeats(caps):
    """A copy of the captions with earlier words written over later ones: the third word is the first again, the last the second."""
    caps = caps.clone()
    for b in range(caps.size(0)):
        n = int((caps[b] != 0).sum())
        if n >= 3:
            caps[b, 2] = caps[b, 0]
        if n >= 5:
            caps[b, n - 1] = caps[b, 1]
    return caps


@functools.lru_cache(maxsize=None)
def medium(name, alpha=ALPHA, eps=EPS):
    """The `medium` fixture of tests/test_label_smoothing_gpu.py with repeats in its captions, and the reference objective
    differentiated by autograd on the oracle's logits."""
    m = dict(smooth_medium(name))
    m["caps"] = with_repeats(m["caps"])
    ref = ulref.train_reference(m["cfg"], m["params"], m["feats"], m["caps"], m["senti"], m["eps"], eps, alpha, DELTA)
    assert float(ref["ul"].max()) > 1e-3                                       # the term moved the loss
    m.update(ref)
    return m


def engine(m, gemm_mode=0):
    d = dims_from_cfg(m["cfg"])
    d.gemm_mode = gemm_mode
    eng = TrainEngine(d, "cuda")
    eng.load_state_dict(m["params"])
    return eng


def inputs(m):
    return dev(m["feats"]), dev(m["caps"]), dev(m["senti"]), dev(m["eps"])


def upstream(m):
    B = m["B"]
    return torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * m["cfg"].kld_weight), device="cuda")


def check_against(eng, loss, kld, ref, gl, gk, what):
    print(f"{what}: loss err {maxdiff(loss, ref['loss']):.3e} (tol {loss_tol(ref['loss']):.3e}), ul err {maxdiff(eng.ul(), ref['ul']):.3e} "
          f"(tol {loss_tol(ref['ul']):.3e}), kld err {maxdiff(kld, ref['kld']):.3e}, nll err {maxdiff(eng.nll(), ref['nll']):.3e}")
    assert maxdiff(loss, ref["loss"]) <= loss_tol(ref["loss"])
    assert maxdiff(eng.ul(), ref["ul"]) <= loss_tol(ref["ul"])
    assert maxdiff(kld, ref["kld"]) <= loss_tol(ref["kld"])
    assert maxdiff(eng.nll(), ref["nll"]) <= loss_tol(ref["nll"])
    eng.backward(gl, gk)
    got = eng.grad_dict()
    worst = 0.0
    for k, v in ref["grads"].items():
        if k in eng.frozen_names:      # the tied table is frozen: the engine forms no gradient for it
            continue
        worst = max(worst, maxdiff(got[k], v) / grad_tol(v))
        assert maxdiff(got[k], v) <= grad_tol(v), (k, maxdiff(got[k], v), grad_tol(v))
    print(f"  largest gradient error: {worst:.4f} of grad_tol")
    return got


@pytest.mark.parametrize("gemm_mode", [0, 2])
@pytest.mark.parametrize("name", ["untied", "tied"])
def test_train_step_matches_autograd_of_the_reference_objective(name, gemm_mode):
    m = medium(name)
    eng = engine(m, gemm_mode)
    args = inputs(m)
    gl, gk = upstream(m)
    # today's forward / backward: what unlikelihood = 0 must reproduce bit for bit
    loss_p, kld_p = (t.clone() for t in eng.forward(*args, label_smoothing=EPS))
    eng.backward(gl, gk)
    grads_p = eng.grad_dict()
    loss_o, kld_o = (t.clone() for t in eng.forward(*args, label_smoothing=EPS, unlikelihood=0.0, unlikelihood_clamp=0.5))
    assert torch.equal(bits(loss_o), bits(loss_p)) and torch.equal(bits(kld_o), bits(kld_p)) and float(eng.ul().abs().max()) == 0.0
    eng.backward(gl, gk)
    for k, v in eng.grad_dict().items():
        assert torch.equal(bits(v), bits(grads_p[k])), k
    loss, kld = eng.forward(*args, label_smoothing=EPS, unlikelihood=ALPHA)
    assert torch.equal(bits(kld), bits(kld_p))                     # the latent path does not know about the term
    assert maxdiff(loss, loss_p) > 1e-3 * ALPHA                    # (it moved the loss)
    got = check_against(eng, loss, kld, m, gl, gk, f"{name} gemm_mode {gemm_mode}")
    # the phased backward of the data-parallel path keeps the descriptor beside the cfg: the same gradients, bit for bit
    eng.forward(*args, label_smoothing=EPS, unlikelihood=ALPHA)
    eng.backward_phased(gl, gk, (16, 32, 64, 8, 4, 128))
    for k, v in eng.grad_dict().items():
        assert k in eng.frozen_names or torch.equal(bits(v), bits(got[k])), k
    # no state leaks: a forward with label smoothing only, after one with the term, is the one before it
    loss_a, kld_a = eng.forward(*args, label_smoothing=EPS)
    assert torch.equal(bits(loss_a), bits(loss_p)) and float(eng.ul().abs().max()) == 0.0
    eng.backward(gl, gk)
    for k, v in eng.grad_dict().items():
        assert torch.equal(bits(v), bits(grads_p[k])), k


def test_composes_with_free_bits_and_label_smoothing():
    import freebitsref as fr
    import test_free_bits_gpu as fb
    m = fb.medium(1, 1)                                  # SENTIMENT_VAE 1, the element floor: its scaled parameters and its floor
    cfg = m["cfg"]
    p = {k: v.clone().requires_grad_(True) for k, v in m["params"].items()}
    out, k, w = fb._oracle_latents(cfg, p, m["feats"], m["caps"], m["senti"], m["eps"], m["obj"])
    kld, _, _ = fr.floored(k, w, m["lam"], 1)
    logits = torch.stack([s["logits"] for s in out["steps"]], 0)
    targets = out["tokens"][:, 1:].t().contiguous()
    ulref.check_margins(logits.detach(), targets, w, DELTA)
    loss, ul = ulref.loss(logits, targets, w, EPS, 2.0, DELTA)
    (loss.mean() + kld.mean() / cfg.kld_weight).backward()
    ref = dict(loss=loss.detach(), ul=ul.detach(), kld=kld.detach(), nll=out["loss"].detach(), grads={n: v.grad.clone() for n, v in p.items()})
    assert float(ref["ul"].max()) > 1e-3
    eng = TrainEngine(dims_from_cfg(cfg), "cuda")
    eng.load_state_dict(m["params"])
    got_loss, got_kld = eng.forward(*fb.inputs(m), label_smoothing=EPS, free_bits=m["lam"], free_bits_mode="element", unlikelihood=2.0)
    check_against(eng, got_loss, got_kld, ref, *fb.upstream(m), "free bits + label smoothing + unlikelihood")
    assert maxdiff(got_kld, m["raw"]) > 10 * fb.kl_tol(m["kld"])                # (the floor did move the KL)


def test_composes_with_scheduled_sampling():
    """Under scheduled sampling the candidates are the ground-truth targets, as the loss's targets are; the fed ids of the fixed
    seed are read back through input_tokens() and given to the restated forward."""
    import schedsampref as R
    import test_sched_sampling_gpu as ss
    m = ss.medium("untied")                                                     # (caption 1 holds an in-caption unknown: w = 0 there)
    seed = ss.pick_seed(m, 0.5)
    eng = ss.engine(m)
    args = ss.inputs(m)
    kw = dict(ss_prob=0.5, ss_sampler=ss.MULTI, ss_seed=seed)
    eng.forward(*args, **kw)
    fed_ids = eng.input_tokens().cpu().clone()
    assert bool(eng.fed_mask().any())
    loss, kld = eng.forward(*args, unlikelihood=ALPHA, **kw)
    assert torch.equal(eng.input_tokens().cpu(), fed_ids)                       # the term moves neither a logit nor a draw
    cfg = m["cfg"]
    p = {k: v.clone().requires_grad_(True) for k, v in m["params"].items()}
    out = R.train_forward_fed(p, cfg, m["feats"], m["caps"], m["senti"], m["eps"], fed_ids, return_steps=True)
    logits = out["logits"].transpose(0, 1)
    targets = out["tokens"][:, 1:].t().contiguous()
    w = (targets != cfg.pad_index).double()
    ulref.check_margins(logits.detach(), targets, w, DELTA)
    ref_loss, ul = ulref.loss(logits, targets, w, 0.0, ALPHA, DELTA)
    (ref_loss.mean() + out["kld"].double().mean() / cfg.kld_weight).backward()
    ref = dict(loss=ref_loss.detach(), ul=ul.detach(), kld=out["kld"].detach(), nll=out["loss"].detach(),
               grads={k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()})
    assert float(ref["ul"].max()) > 1e-3
    check_against(eng, loss, kld, ref, *ss.upstream(m), "scheduled sampling 0.5 + unlikelihood")


def test_refused_together_with_distillation_before_any_call_into_the_library():
    m = medium("untied")
    eng = engine(m)
    args = inputs(m)
    eng.forward(*args)
    version = eng.fwd_version
    T, B, V = m["cfg"].max_caption_length + 1, m["B"], m["cfg"].vocab_size
    scores = torch.zeros(T * B, V, device="cuda")
    with pytest.raises(ValueError, match=r"(?s)unlikelihood.*distill"):
        eng.forward(*args, unlikelihood=ALPHA, distill=Distill(scores, V, 0.5, 2.0))
    with pytest.raises(ValueError, match=r"(?s)unlikelihood.*distill"):
        eng.train_step(*args, unlikelihood=ALPHA, distill=Distill(scores, V, 0.5, 2.0), **STEP)
    with pytest.raises(ValueError, match="unlikelihood must"):
        eng.forward(*args, unlikelihood=-1.0)
    with pytest.raises(ValueError, match="unlikelihood_clamp"):
        eng.forward(*args, unlikelihood=ALPHA, unlikelihood_clamp=1.0)
    assert eng.fwd_version == version
    eng.forward(*args, unlikelihood=ALPHA, distill=Distill(scores, V, 0.0, 2.0))      # one of the two off: fine
    eng.forward(*args, unlikelihood=0.0, distill=Distill(scores, V, 0.5, 2.0))


def test_fused_step_is_forward_and_backward_update_and_zero_is_the_plain_step():
    m = medium("untied")
    args = inputs(m)
    gl, gk = upstream(m)
    kw = dict(label_smoothing=EPS, unlikelihood=ALPHA)
    a, b = engine(m), engine(m)
    loss_a, _ = a.train_step(*args, kl_beta=0.5, **STEP, **kw)
    loss_b, _ = b.forward(*args, **kw)
    b.backward_update(gl, 0.5 * gk, **{k: v for k, v in STEP.items() if k != "kld_weight"})
    assert torch.equal(bits(loss_a), bits(loss_b)) and torch.equal(bits(a.ul()), bits(b.ul()))
    assert torch.equal(bits(a.params.flat), bits(b.params.flat))
    plain, zero = engine(m), engine(m)
    plain.train_step(*args, label_smoothing=EPS, **STEP)
    zero.train_step(*args, label_smoothing=EPS, unlikelihood=0.0, **STEP)
    assert torch.equal(bits(plain.params.flat), bits(zero.params.flat)) and float(zero.ul().abs().max()) == 0.0
    assert not torch.equal(bits(plain.params.flat), bits(a.params.flat))


def test_self_critical_step_is_unaffected():
    """A captioner built with unlikelihood 0.5 - and fresh from a training forward with the term - takes the self-critical step of
    one built without, bit for bit (the smallest fixture of tests/test_scst_gpu.py)."""
    from test_label_smoothing_gpu import build_model
    from test_scst_gpu import HP, N_, P_, SEED, setup
    s = setup(1, 0)
    res = []
    for alpha in (0.0, 0.5):
        mod = build_model(s["cfg"], s["params"], 0.0, beam=1)
        mod.unlikelihood = alpha
        mod.train()
        ro = s["ro"]
        mod._eps_override = ro.train_eps
        out = mod(ro.feats, None, None, ro.caps, ro.sentiment.view(-1, 1))
        assert ("ul" in out) == (alpha > 0)
        mod._eps_override = None
        loss, kld, stats = mod.scst_step(s["feats"], [0, 1, 2], s["senti"].view(P_, 1), references=s["references"], seed=SEED,
                                         n_samples=N_, decoder_frozen=False, **HP)
        res.append((out["loss"].detach().clone(), loss.clone(), kld.clone(), stats.clone(), mod._eng.params.flat.clone(),
                    mod._eng.ul().clone()))
    a, b = res
    assert not torch.equal(a[0], b[0])                                          # (the training forwards did differ)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x.cpu().contiguous().view(torch.uint8), y.cpu().contiguous().view(torch.uint8))
    assert float(b[5].abs().max()) == 0.0                                       # the self-critical forward had the term off
