"""GPU: label smoothing in the cross-entropy train step.  Kernel level: ssc_ce_fwd_smooth / ssc_ce_bwd_smooth against the float64
reference (tests/smoothref.py) computed from the same fp32 logits, at row widths on every path of the kernels (scalar throughout,
16-byte bulk with and without a tail, a misaligned first row: head + bulk + tail), with skipped rows full of NaN and poisoned pad
columns.  Train step: ssc_train_fwd / ssc_train_bwd with cfg.label_smoothing against the CPU oracle, whose per-step logits stay in
the autograd graph and are turned into the smoothed loss by smoothref; the fused step, the module and the self-critical step.
Tolerances are the project's own (tests/test_train_gpu.py): loss 1e-4 + 1e-5 max|ref|, gradients 1e-4 max(scale, 1e-3) + 2e-6."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import oracle
import smoothref
from gpuutil import dev, engine_from, maxdiff
from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_, B_ = 3, 4
POISON = 1e30


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def loss_tol(ref):
    return 1e-4 + 1e-5 * float(ref.abs().max())


def grad_tol(ref):
    return 1e-4 * max(float(ref.abs().max()), 1e-3) + 2e-6


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------
# (V, ld, offset in floats of the first row from a 16-byte boundary)
SHAPES = [(37, 37, 0), (451, 452, 0), (777, 780, 0), (1024, 1024, 0), (2003, 2004, 0), (451, 452, 1), (1024, 1028, 1)]


@functools.lru_cache(maxsize=None)
def case(V, ld, off):
    """Inputs of one shape and their float64 references at every eps the tests use; shared, changed by none."""
    g = torch.Generator().manual_seed(1000 + V + ld + off)
    rows = T_ * B_
    w = torch.tensor([[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0]])          # caption lengths 3, 2, 3, 1
    x = torch.randn(T_, B_, V, generator=g) * 2.0
    x[1, 2] = torch.rand(V, generator=g) * 160.0 - 80.0                                             # spread over +-80: the running max moves
    x[1, 2, V // 2] = 80.0
    y = torch.randint(0, V, (T_, B_), generator=g)
    y[0, 0], y[0, 1], y[1, 2] = 0, V - 1, V - 1
    gl = torch.tensor([0.7, -1.3, 0.25, 0.0])                                                       # mixed signs, one zero
    nvalid = w.sum(0)
    xd = x.clone()
    xd[w == 0] = float("nan")                                                                       # skipped rows: never read
    buf = torch.full((rows * ld + 8,), POISON)
    buf[off:off + rows * ld].view(rows, ld)[:, :V] = xd.view(rows, V)
    ref = {}
    for eps in (0.0, 0.1, 0.3):
        ref[eps] = (smoothref.loss(x, y, w, eps), smoothref.dlogits(x, y, w, gl, eps))
    return dict(V=V, ld=ld, off=off, w=w, y=y, gl=gl, nvalid=nvalid, buf=buf, ref=ref)


def run_pair(c, eps, smooth=True):
    """forward + in-place backward on a fresh device copy of the case -> (whole buffer, lse blocks, loss, nll)."""
    lib = L.load()
    V, ld, off = c["V"], c["ld"], c["off"]
    rows = T_ * B_
    buf = c["buf"].cuda()
    assert buf.data_ptr() % 16 == 0
    view = buf[off:]
    y, w, nv, gl = dev(c["y"]), dev(c["w"]), dev(c["nvalid"]), dev(c["gl"])
    lse = torch.full(((3 if smooth else 2) * rows,), float("nan"), device="cuda")
    loss = torch.full((B_,), float("nan"), device="cuda")
    nll = torch.full((B_,), float("nan"), device="cuda")
    st = L.stream_ptr()
    if smooth:
        lib.ssc_ce_fwd_smooth(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), T_, B_, V, eps, L.ptr(lse), L.ptr(loss), L.ptr(nll), st)
        lib.ssc_ce_bwd_smooth(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(lse), L.ptr(gl), T_, B_, V, eps, st)
    else:
        lib.ssc_ce_fwd(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), T_, B_, V, L.ptr(lse), L.ptr(loss), st)
        lib.ssc_ce_bwd(L.ptr(view), ld, L.ptr(y), L.ptr(w), L.ptr(nv), L.ptr(lse), L.ptr(gl), T_, B_, V, st)
    torch.cuda.synchronize()
    return buf, lse, loss, nll


def untouched(c, buf):
    """Everything outside the [0, V) columns of the rows still holds the poison: pad columns, the floats before and behind."""
    V, ld, off = c["V"], c["ld"], c["off"]
    rows = T_ * B_
    b = buf.cpu()
    ok = bool((b[:off] == POISON).all()) and bool((b[off + rows * ld:] == POISON).all())
    return ok and bool((b[off:off + rows * ld].view(rows, ld)[:, V:] == POISON).all())


@pytest.mark.parametrize("eps", [0.1, 0.3])
@pytest.mark.parametrize("V,ld,off", SHAPES)
def test_kernels_match_float64(V, ld, off, eps):
    c = case(V, ld, off)
    rows = T_ * B_
    buf, lse, loss, nll = run_pair(c, eps)
    want_loss, want_grad = c["ref"][eps]
    want_nll = c["ref"][0.0][0]
    got = buf[off:off + rows * ld].view(T_, B_, ld)[:, :, :V].cpu()
    print(f"V={V} ld={ld} off={off} eps={eps}: loss err {maxdiff(loss, want_loss):.3e} (tol {loss_tol(want_loss):.3e}), "
          f"nll err {maxdiff(nll, want_nll):.3e}, grad err {maxdiff(got, want_grad):.3e} (tol {grad_tol(want_grad):.3e})")
    assert torch.isfinite(loss).all() and torch.isfinite(nll).all() and torch.isfinite(got).all() and torch.isfinite(lse).all()
    assert maxdiff(loss, want_loss) <= loss_tol(want_loss)
    assert maxdiff(nll, want_nll) <= loss_tol(want_nll)
    assert maxdiff(got, want_grad) <= grad_tol(want_grad)
    dead = c["w"] == 0
    assert bool((bits(got[dead]) == 0).all())                         # skipped rows: exactly +0 over [0, V)
    assert bool((bits(got[:, 3]) == 0).all())                         # gl = 0: zero rows too
    assert bool((lse.view(3, T_, B_).cpu()[:, dead] == 0).all())      # lse, w*row(eps), w*row(0) of a skipped row
    assert untouched(c, buf)


@pytest.mark.parametrize("V,ld,off", SHAPES)
def test_eps_zero_is_bit_equal_to_the_unsmoothed_entries(V, ld, off):
    c = case(V, ld, off)
    rows = T_ * B_
    b0, lse0, loss0, _ = run_pair(c, 0.0, smooth=False)
    b1, lse1, loss1, nll1 = run_pair(c, 0.0)
    assert torch.equal(bits(lse1[:2 * rows]), bits(lse0)) and torch.equal(bits(lse1[2 * rows:]), bits(lse0[rows:]))
    assert torch.equal(bits(loss1), bits(loss0)) and torch.equal(bits(nll1), bits(loss0))
    g0 = b0[off:off + rows * ld].view(rows, ld)[:, :V]
    g1 = b1[off:off + rows * ld].view(rows, ld)[:, :V]
    assert torch.equal(bits(g1), bits(g0))
    assert untouched(c, b1)
    want_loss, want_grad = c["ref"][0.0]
    assert maxdiff(loss1, want_loss) <= loss_tol(want_loss)
    assert maxdiff(g1.view(T_, B_, V), want_grad) <= grad_tol(want_grad)


@pytest.mark.parametrize("V,ld,off", [(37, 37, 0), (451, 452, 1), (2003, 2004, 0)])
def test_two_calls_are_bit_equal(V, ld, off):
    c = case(V, ld, off)
    a = run_pair(c, 0.1)
    b = run_pair(c, 0.1)
    rows = T_ * B_
    for x, y in zip(a, b):
        if x is a[0]:   # the buffer holds the NaN-free gradient over [0, V) and poison elsewhere
            x, y = x[off:off + rows * ld].view(rows, ld)[:, :V], y[off:off + rows * ld].view(rows, ld)[:, :V]
        assert torch.equal(bits(x), bits(y))


def test_nll_pointer_is_optional():
    lib = L.load()
    c = case(37, 37, 0)
    buf = c["buf"].cuda()
    y, w, nv = dev(c["y"]), dev(c["w"]), dev(c["nvalid"])
    lse = torch.empty(3 * T_ * B_, device="cuda")
    loss = torch.empty(B_, device="cuda")
    lib.ssc_ce_fwd_smooth(L.ptr(buf), 37, L.ptr(y), L.ptr(w), L.ptr(nv), T_, B_, 37, 0.1, L.ptr(lse), L.ptr(loss), None, L.stream_ptr())
    want = c["ref"][0.1][0]
    assert maxdiff(loss, want) <= loss_tol(want)


# ---- 2. train step ----------------------------------------------------------------------------------------------------------
EPS = 0.1
MEDIUM = {
    "untied": (0, 5, 10, dict(V=777, E=100, H=130, A=70, F=260, Z=30, L=9)),
    "tied": (1, 6, 7, dict(V=451, E=300, H=64, A=48, F=128, Z=16, L=6)),     # run with the tied head: frozen table, Linear + Tanh
}
STEP = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=0.5)


@functools.lru_cache(maxsize=None)
def medium(name):
    """The inputs of tests/test_train_gpu.py::test_train_matches_oracle_medium at this shape, the oracle's forward with its per-step
    logits in the graph, the smoothed loss smoothref makes of them and the gradients of mean(loss) + mean(kld) / kld_weight."""
    sv, B, R, dims = MEDIUM[name]
    cfg = oracle.OracleConfig(vocab_size=dims["V"], image_feature_size=dims["F"], embedding_size=dims["E"],
                              hidden_size=dims["H"], attention_projection_size=dims["A"], z_space=dims["Z"],
                              max_caption_length=dims["L"], sentiment_vae=sv, senti_prior_multip=0.5, tied=name == "tied")
    params = oracle.init_params(cfg, seed=5)
    g = torch.Generator().manual_seed(17)
    L_, T = dims["L"], dims["L"] + 1
    feats = torch.randn(B, R, dims["F"], generator=g)
    feats[0, R - 3:] = 0
    caps = torch.zeros(B, L_, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(3, L_ + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(2, dims["V"], (n,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(T, B, dims["Z"], generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = oracle.train_forward(p, cfg, feats, caps, senti, eps, return_steps=True)
    logits = torch.stack([s["logits"] for s in out["steps"]], 0)              # (T, B, V), in the autograd graph
    targets = out["tokens"][:, 1:].t().contiguous()
    w = (targets != cfg.pad_index).double()
    loss = smoothref.loss(logits, targets, w, EPS)
    (loss.mean() + out["kld"].double().mean() / cfg.kld_weight).backward()
    grads = {k: v.grad.clone() for k, v in p.items()}
    return dict(cfg=cfg, params=params, feats=feats, caps=caps, senti=senti, eps=eps, loss=loss.detach(), kld=out["kld"].detach(),
                nll=out["loss"].detach(), grads=grads, B=B)


def inputs(m):
    return dev(m["feats"]), dev(m["caps"]), dev(m["senti"]), dev(m["eps"])


@pytest.mark.parametrize("name", list(MEDIUM))
def test_train_step_matches_oracle_with_smoothed_loss(name):
    m = medium(name)
    cfg, B = m["cfg"], m["B"]
    eng = engine_from(cfg, m["params"])
    args = inputs(m)
    loss_plain, kld_plain = (t.clone() for t in eng.forward(*args))
    loss_zero, kld_zero = (t.clone() for t in eng.forward(*args, label_smoothing=0.0))
    assert torch.equal(bits(loss_zero), bits(loss_plain)) and torch.equal(bits(kld_zero), bits(kld_plain))
    assert torch.equal(bits(eng.nll()), bits(loss_plain))
    loss, kld = eng.forward(*args, label_smoothing=EPS)
    print(f"{name}: loss err {maxdiff(loss, m['loss']):.3e} (tol {loss_tol(m['loss']):.3e}), kld err {maxdiff(kld, m['kld']):.3e}, "
          f"nll err {maxdiff(eng.nll(), m['nll']):.3e}")
    assert maxdiff(loss, m["loss"]) <= loss_tol(m["loss"])
    assert maxdiff(kld, m["kld"]) <= loss_tol(m["kld"])
    assert torch.equal(bits(kld), bits(kld_plain))
    assert maxdiff(eng.nll(), m["nll"]) <= loss_tol(m["nll"])
    assert maxdiff(loss, loss_plain) > 1e-3                      # (smoothing moved the loss)
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * cfg.kld_weight), device="cuda")
    eng.backward(gl, gk)
    got = eng.grad_dict()
    for k, v in m["grads"].items():
        if k in eng.frozen_names:      # the tied table is frozen (updown_captioner.py:75): the engine forms no gradient for it
            continue
        print(f"  {k}: err {maxdiff(got[k], v):.3e} tol {grad_tol(v):.3e}")
        assert maxdiff(got[k], v) <= grad_tol(v), (k, maxdiff(got[k], v), grad_tol(v))
    # the phased backward of the data-parallel path reads the same cfg: the same gradients, bit for bit
    eng.forward(*args, label_smoothing=EPS)
    eng.backward_phased(gl, gk, (16, 32, 64, 8, 4, 128))
    for k, v in eng.grad_dict().items():
        assert k in eng.frozen_names or torch.equal(bits(v), bits(got[k])), k


def test_fused_step_matches_the_oracle_step_on_the_reference_gradients():
    m = medium("untied")
    eng = engine_from(m["cfg"], m["params"])
    eng.train_step(*inputs(m), label_smoothing=EPS, **STEP)
    want, _, _ = oracle.sgd_clip_step(m["params"], m["grads"], {}, STEP["lr"], STEP["momentum"], STEP["weight_decay"], STEP["max_norm"])
    sd = eng.state_dict()
    for k, v in want.items():
        assert maxdiff(sd[k], v) < 1e-5, (k, maxdiff(sd[k], v))      # the bound of tests/test_module_gpu.py for its steps
    plain = engine_from(m["cfg"], m["params"])
    plain.train_step(*inputs(m), **STEP)
    assert not torch.equal(plain.params.flat, eng.params.flat)


def build_model(cfg, params, label_smoothing, beam=5):
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    mod = UpDownCaptioner(Vocabulary.synthetic(cfg.vocab_size), cfg.image_feature_size, cfg.embedding_size, cfg.hidden_size,
                          cfg.attention_projection_size, max_caption_length=cfg.max_caption_length, beam_size=beam,
                          use_cbs=cfg.tied, z_space=cfg.z_space, prior_std=cfg.prior_std, simple_vae=cfg.simple_vae,
                          latent_embedding="glove", sentiment_vae=cfg.sentiment_vae, senti_prior_multip=cfg.senti_prior_multip,
                          device=torch.device("cuda"), label_smoothing=label_smoothing)
    mod.load_state_dict(dict(params))
    return mod.cuda()


def test_module_training_forward_returns_the_engine_loss_and_its_gradients():
    m = medium("untied")
    eng = engine_from(m["cfg"], m["params"])
    feats, caps, senti, eps = inputs(m)
    loss, kld = eng.forward(feats, caps, senti, eps, label_smoothing=EPS)
    mod = build_model(m["cfg"], m["params"], EPS)
    mod.train()
    mod._eps_override = m["eps"]
    out = mod(feats, None, None, caps, senti)
    assert torch.equal(bits(out["loss"]), bits(loss)) and torch.equal(bits(out["kld"]), bits(kld))
    (out["loss"].mean() + out["kld"].mean() / m["cfg"].kld_weight).backward()
    named = dict(mod.named_parameters())
    for k, v in m["grads"].items():
        assert maxdiff(named[k].grad, v) <= grad_tol(v), k
    # the stand-alone loss entry: the same kernel on logits of the caller's
    V = m["cfg"].vocab_size
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(3, 4, V, generator=g)
    tg = torch.randint(0, V, (3, 4), generator=g)
    mask = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]])
    want = smoothref.loss(lg.transpose(0, 1), tg.t(), mask.t().double(), 0.3)
    got = mod._get_loss(lg.cuda(), tg.cuda(), mask.cuda(), label_smoothing=0.3)
    assert maxdiff(got, want) <= loss_tol(want)
    assert torch.equal(bits(mod._get_loss(lg.cuda(), tg.cuda(), mask.cuda(), label_smoothing=0.0)),
                       bits(mod._get_loss(lg.cuda(), tg.cuda(), mask.cuda())))


def test_self_critical_step_never_smooths():
    """A captioner built with label_smoothing 0.1 - and fresh from a smoothed training forward - takes the self-critical step of one
    built with 0, bit for bit (the smallest fixture of tests/test_scst_gpu.py)."""
    from test_scst_gpu import HP, N_, P_, SEED, setup
    s = setup(1, 0)
    cfg = s["cfg"]
    res = []
    for ls in (0.0, 0.1):
        mod = build_model(cfg, s["params"], ls, beam=1)
        mod.train()
        ro = s["ro"]
        mod._eps_override = ro.train_eps
        out = mod(ro.feats, None, None, ro.caps, ro.sentiment.view(-1, 1))     # leaves the engine's cfg at this captioner's smoothing
        mod._eps_override = None
        loss, kld, stats = mod.scst_step(s["feats"], [0, 1, 2], s["senti"].view(P_, 1), references=s["references"], seed=SEED,
                                         n_samples=N_, decoder_frozen=False, **HP)
        res.append((out["loss"].detach().clone(), loss.clone(), kld.clone(), stats.clone(), mod._eng.params.flat.clone(),
                    mod._eng.nll().clone()))
    a, b = res
    assert not torch.equal(a[0], b[0])                                          # (the training forwards did differ)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x.cpu().contiguous().view(torch.uint8), y.cpu().contiguous().view(torch.uint8))
    assert torch.equal(bits(b[5]), bits(b[1]))                                  # nll of an unsmoothed forward is its loss


# ---- 3. script --------------------------------------------------------------------------------------------------------------
def test_train_script_smooths_and_logs_nll(tmp_path):
    from test_scripts_gpu import YAML
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    out = tmp_path / "run"
    args = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--fused-optimizer", "--serialization-dir", str(out), "--stop-after", "2",
            "--config-override", "OPTIM.LABEL_SMOOTHING", "0.1"]
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = [json.loads(x) for x in open(out / "scalars.jsonl")]
    assert [rec["iteration"] for rec in log] == [1, 2]
    for rec in log:
        assert "nll" in rec and rec["nll"] > 0 and rec["nll"] == rec["nll"] and abs(rec["nll"] - rec["1reconstr_loss"]) > 1e-6
    assert "LABEL_SMOOTHING: 0.1" in open(out / "config.yml").read()
