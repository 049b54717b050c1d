"""GPU: scheduled sampling in the cross-entropy train step (include/ssc.h: ssc_sched_sampling).

Kernel: ssc_sched_mix_rows against tests/schedsampref.py + tests/samplerref.py from the same fp32 logits - the fed mask bit for bit
(the decision is integer arithmetic and one exact float32 compare), the token of every fired row equal to ssc_sample_rows' token
for the same row, and equal to the NumPy draw wherever that is decided by more than float32 rounding (schedsampref.draw_row: the
margin tests/test_sampling_gpu.py uses), the gathered embedding rows bit for bit, guard words around every output.

Train step: the draws restated from the device's own logits rows; loss, kld and every gradient against the restated forward
(schedsampref.train_forward_fed) fed the device's input ids, under the project's bounds for the train step
(tests/test_free_bits_gpu.py): loss / kld 1e-4 + 1e-5 max|ref|, gradients 1e-4 max(max|ref|, 1e-3) + 2e-6."""
import ctypes as C
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import freebitsref as fr
import oracle
import schedsampref as R
import smoothref
from gpuutil import dev, dims_from_cfg, maxdiff
from ssc_runtime import lib as L
from ssc_runtime.engine import TrainEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = float(np.float32(1e30))   # (exact in float32: read back, it compares equal)
# (kind, top_k, top_p, temperature): multinomial at a temperature other than 1, arg-max (top-k with k = 1), top-k, top-p
SAMPLERS = {"multinomial": (0, 0, 1.0, 0.8), "argmax": (1, 1, 1.0, 1.0), "top-k": (1, 40, 1.0, 1.3), "top-p": (2, 0, 0.7, 0.6)}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def val_tol(ref):
    return 1e-4 + 1e-5 * float(ref.detach().abs().max())


def grad_tol(ref):
    return 1e-4 * max(float(ref.detach().abs().max()), 1e-3) + 2e-6


def sched(prob, sampler, seed):
    kind, k, p, T = sampler
    return L.SchedSampling(prob, L.SamplerDesc(kind, min(k, 10 ** 9), p, T, seed))


def sample_rows(logits, ld, V, sampler, seed, step):
    """ssc_sample_rows on (rows, ld) device logits with row r as batch entry r."""
    lib = L.load()
    rows = logits.size(0)
    pred = torch.empty(rows, dtype=torch.int64, device="cuda")
    lp = torch.empty(rows, dtype=torch.float32, device="cuda")
    kind, k, p, T = sampler
    d = L.SamplerDesc(kind, k, p, T, seed)
    lib.ssc_sample_rows(L.ptr(logits), ld, rows, V, C.byref(d), None, step, None, None, 0, L.ptr(pred), L.ptr(lp), None, L.stream_ptr())
    return pred.cpu()


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kcase(V, ld, rows):
    """Logits, ground-truth ids, weights and the table of one shape; shared, changed by none.  rows 5 and 70 hold ineligible rows of
    each kind (no previous target, no target, neither), whose logits are NaN; the pad column of ld > V is poisoned."""
    g = torch.Generator().manual_seed(1000 + V + 7 * rows)
    logits = torch.full((rows, ld), POISON)
    logits[:, :V] = torch.randn(rows, V, generator=g) * 2.0
    logits[::3, :V] = (logits[::3, :V] * 2).round() / 2                        # exact ties
    r = torch.arange(rows)
    w_prev = torch.ones(rows)
    w_cur = torch.ones(rows)
    if rows > 1:
        w_prev[(r % 7 == 1) | (r % 7 == 3)] = 0
        w_cur[(r % 7 == 2) | (r % 7 == 3)] = 0
    elig = (w_prev != 0) & (w_cur != 0)
    logits[~elig] = float("nan")
    truth = torch.randint(0, V, (rows,), generator=g)
    truth[0] = 0                                                                # the pad id: the table's row 0
    E, ldt = (10, 11) if rows == 5 else (12, 12)                                # rows off / on 16-byte boundaries
    table = torch.randn(V, ldt, generator=g)
    return dict(V=V, ld=ld, rows=rows, logits=logits, w_prev=w_prev, w_cur=w_cur, elig=elig.numpy(), truth=truth, E=E, ldt=ldt,
                table=table, dev=dict(logits=dev(logits), w_prev=dev(w_prev), w_cur=dev(w_cur), truth=dev(truth), table=dev(table)))


def run_mix(c, step, prob, sampler, seed):
    lib = L.load()
    rows, E, d = c["rows"], c["E"], c["dev"]
    ldo = E + 6
    tok = torch.full((rows + 2,), -7, dtype=torch.int64, device="cuda")
    fed = torch.full((rows + 2,), POISON, device="cuda")
    emb = torch.full((rows + 2, ldo), POISON, device="cuda")
    ss = sched(prob, sampler, seed)
    lib.ssc_sched_mix_rows(L.ptr(d["logits"]), c["ld"], rows, c["V"], L.ptr(d["truth"]), L.ptr(d["w_prev"]), L.ptr(d["w_cur"]),
                           L.ptr(d["table"]), c["ldt"], E, step, C.byref(ss), L.ptr(tok[1:]), L.ptr(fed[1:]), L.ptr(emb[1:]), ldo,
                           L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu(), fed.cpu(), emb.cpu()


def seed_with_both_states(c, prob, base):
    """The first seed from `base` on for which the restated decisions of steps 1 and 19 over the eligible rows hold both states."""
    for seed in range(base, base + 64):
        f = np.concatenate([R.fires(R.uniforms_step(seed, s, c["rows"]), c["elig"], prob)[c["elig"]] for s in (1, 19)])
        if f.any() and not f.all():
            return seed
    raise AssertionError("no seed with both decision states")


@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("V,ld", [(37, 37), (451, 452), (1000, 1000), (10000, 10000), (40003, 40004)])
def test_mix_rows_match_the_restatement(V, ld, rows):
    c = kcase(V, ld, rows)
    truth, table, E = c["truth"].numpy(), c["table"], c["E"]
    clean = torch.nan_to_num(c["logits"], nan=0.0).cuda()
    fired_total = sure_total = 0
    for name, sampler in SAMPLERS.items():
        kind, k, p, T = sampler
        sampler = (kind, min(k, V), p, T)
        for step in (1, 19):
            draws = {}                                                          # the draw of a row does not depend on prob
            for prob in (0.0, 0.25, 1.0):
                seed = seed_with_both_states(c, prob, 0x5EED0000 + V) if prob == 0.25 else 0x0123_4567_89AB_CDEF + V
                tok, fed, emb = run_mix(c, step, prob, sampler, seed)
                what = (name, step, prob)
                assert int(tok[0]) == -7 and int(tok[-1]) == -7 and float(fed[0]) == POISON and float(fed[-1]) == POISON, what
                assert bool((emb[0] == POISON).all()) and bool((emb[-1] == POISON).all()) and bool((emb[:, E:] == POISON).all()), what
                tok, fed, emb = tok[1:-1], fed[1:-1], emb[1:-1, :E]
                want_fed = R.fires(R.uniforms_step(seed, step, rows), c["elig"], prob)
                assert np.array_equal(fed.numpy(), want_fed.astype(np.float32)), what          # 1.0 / 0.0, bit for bit
                if prob == 0.0:
                    assert not want_fed.any()
                if prob == 1.0:
                    assert np.array_equal(want_fed, c["elig"])
                assert np.array_equal(tok.numpy()[~want_fed], truth[~want_fed]), what
                # a fired row: ssc_sample_rows' token for the same logits row, sampler, step, row id and seed - always
                lib_tok = sample_rows(clean, ld, V, sampler, seed, step).numpy()
                assert np.array_equal(tok.numpy()[want_fed], lib_tok[want_fed]), what
                for r in np.nonzero(want_fed)[0]:
                    key = (seed, int(r))
                    if key not in draws:
                        draws[key] = R.draw_row(c["logits"][r, :V].numpy(), *sampler, seed, step, int(r))
                    want, sure = draws[key]
                    fired_total += 1
                    sure_total += int(sure)
                    assert not sure or int(tok[r]) == want, (what, int(r))
                assert bool(((tok >= 0) & (tok < V)).all())
                assert torch.equal(bits(emb), bits(table[tok][:, :E])), what                     # the fed word's row, row 0 for id 0
                tok2, fed2, emb2 = run_mix(c, step, prob, sampler, seed)                         # two calls: the same bits
                assert torch.equal(tok2[1:-1], tok) and torch.equal(bits(fed2[1:-1]), bits(fed)) and torch.equal(bits(emb2[1:-1, :E]), bits(emb))
    assert fired_total > 0 and sure_total >= 0.9 * fired_total, (fired_total, sure_total)


def test_quarter_probability_seed_holds_both_states():
    c = kcase(1000, 1000, 70)
    seed = seed_with_both_states(c, 0.25, 0x5EED0000 + 1000)
    _, fed, _ = run_mix(c, 1, 0.25, SAMPLERS["multinomial"], seed)
    f = fed[1:-1].numpy()[c["elig"]]
    assert 0 < f.sum() < f.size                                                 # both states among the eligible rows of ONE launch
    assert not fed[1:-1].numpy()[~c["elig"]].any()


# ---- 2. the train step ------------------------------------------------------------------------------------------------------
MEDIUM = {"untied": (0, 5, 10, dict(V=777, E=100, H=130, A=70, F=260, Z=30, L=9), False),
          "tied": (1, 5, 7, dict(V=451, E=300, H=64, A=48, F=128, Z=16, L=6), True),
          "one": (1, 1, 6, dict(V=777, E=100, H=130, A=70, F=260, Z=30, L=9), False)}
STEP = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=0.5)
MULTI = (0, 0, 1.0, 1.0)
P_CELL = "_updown_cell."
SCALES = [(1.0, 1.0), (4.0, 4.0), (0.05, 8.0), (0.02, 16.0), (0.01, 32.0)]   # (as tests/test_free_bits_gpu.py)


@functools.lru_cache(maxsize=None)
def medium(name):
    sv, B, Rg, dims, tied = MEDIUM[name]
    cfg = oracle.OracleConfig(vocab_size=dims["V"], image_feature_size=dims["F"], embedding_size=dims["E"], hidden_size=dims["H"],
                              attention_projection_size=dims["A"], z_space=dims["Z"], max_caption_length=dims["L"], sentiment_vae=sv,
                              senti_prior_multip=0.5, tied=tied)
    params = oracle.init_params(cfg, seed=5)
    g = torch.Generator().manual_seed(17)
    L_, T = dims["L"], dims["L"] + 1
    feats = torch.randn(B, Rg, dims["F"], generator=g)
    feats[0, Rg - 3:] = 0
    caps = torch.zeros(B, L_, dtype=torch.long)
    for b in range(B):
        n = L_ if b == 0 else int(torch.randint(3, L_ + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(2, dims["V"], (n,), generator=g)
    if B > 1:
        caps[1, 1] = 0                                                          # an in-caption @@UNKNOWN@@ (id 0, the pad index)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(T, B, dims["Z"], generator=g)
    tok, w = R.tokens_and_weights(cfg, caps)
    return dict(cfg=cfg, params=params, feats=feats, caps=caps, senti=senti, eps=eps, B=B, T=T, V=dims["V"], tok=tok, w=w.numpy(),
                elig=R.eligible(w.numpy()))


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


def pick_seed(m, prob, base=100):
    """The first seed for which at least a third of the eligible positions fire (and, below prob 1, not all of them) - chosen on
    the CPU by the restated decisions."""
    for seed in range(base, base + 64):
        f = R.fires(R.uniforms(seed, m["T"], m["B"]), m["elig"], prob)[m["elig"]]
        if 3 * f.sum() >= f.size and (prob >= 1.0 or not f.all()):
            return seed
    raise AssertionError("no seed")


def check_draws(m, eng, prob, sampler, seed, logits):
    """input_tokens() / fed_mask() of the forward that just ran against the restatement run on the device's own logits rows
    (T, B, V).  Returns the device's fed ids (T, B) on the CPU."""
    T, B, V = m["T"], m["B"], m["V"]
    fed_ids, fed = eng.input_tokens().cpu(), eng.fed_mask().cpu().numpy()
    tok = m["tok"]
    assert fed_ids.dtype == torch.int64 and tuple(fed_ids.shape) == (T, B) and fed.dtype == np.bool_
    assert torch.equal(fed_ids[0], tok[0]) and not fed[0].any()                # step 0 never samples
    want_fed = R.fires(R.uniforms(seed, T, B), m["elig"], prob)
    assert np.array_equal(fed, want_fed)
    lg = logits.cpu()
    n_fired = n_sure = n_new = 0
    for t in range(1, T):
        rows = lg[t - 1].contiguous()
        want, f, sure = R.mix_rows(torch.nan_to_num(rows).numpy(), tok[t].numpy(), m["w"][t - 1], m["w"][t], t, prob, *sampler, seed)
        assert np.array_equal(f, want_fed[t])
        got = fed_ids[t].numpy()
        assert np.array_equal(got[~f], tok[t].numpy()[~f]), t                   # not eligible / not fired: the ground truth
        if f.any():
            lib_tok = sample_rows(torch.nan_to_num(rows).cuda(), V, V, sampler, seed, t).numpy()
            assert np.array_equal(got[f], lib_tok[f]), t
            assert np.array_equal(got[f & sure], want[f & sure]), t
        n_fired += int(f.sum())
        n_sure += int((f & sure).sum())
        n_new += int((f & (want != tok[t].numpy())).sum())
    n_elig = int(m["elig"].sum())
    # not vacuous: a third of the eligible positions fire, a third of those feed another word than the ground truth
    assert 3 * n_fired >= n_elig > 0 and 3 * n_new >= n_fired and n_sure >= 0.9 * n_fired, (n_elig, n_fired, n_new, n_sure)
    return fed_ids


def reference(m, fed_ids, label_smoothing=0.0, floor=None):
    """Loss, kld and the gradients of the mean objective of the restated forward fed `fed_ids` (floor: (lambda, mode) through
    freebitsref, label_smoothing through smoothref, as tests/test_free_bits_gpu.py and tests/test_label_smoothing_gpu.py do)."""
    cfg = m["cfg"]
    p = {k: v.clone().requires_grad_(True) for k, v in m["params"].items()}
    out = R.train_forward_fed(p, cfg, m["feats"], m["caps"], m["senti"], m["eps"], fed_ids, return_steps=True)
    loss, kld = out["loss"], out["kld"]
    if label_smoothing > 0:
        targets = out["tokens"][:, 1:].t().contiguous()
        loss = smoothref.loss(out["logits"].transpose(0, 1), targets, (targets != cfg.pad_index).double(), label_smoothing)
    if floor is not None:
        stack = lambda key: torch.stack([s[key] for s in out["steps"]], 0)
        k = fr.k_elem(stack("mean"), stack("log_var"), stack("prior_mean"), cfg.prior_std ** 2, 0 if cfg.sentiment_vae == 0 else 1)
        kld = fr.floored(k, torch.from_numpy(m["w"]).double(), floor[0], floor[1])[0]
    (loss.double().mean() + kld.double().mean() / cfg.kld_weight).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    return loss.detach(), kld.detach(), grads


def check_step(m, eng, loss, kld, ref, gl, gk, label=""):
    want_loss, want_kld, grads = ref
    print(f"{label}: loss err {maxdiff(loss, want_loss):.3e} (tol {val_tol(want_loss):.3e}), kld err {maxdiff(kld, want_kld):.3e} "
          f"(tol {val_tol(want_kld):.3e})")
    assert maxdiff(loss, want_loss) <= val_tol(want_loss) and maxdiff(kld, want_kld) <= val_tol(want_kld)
    eng.backward(gl, gk)
    got = {k: v.clone() for k, v in eng.grad_dict().items()}
    for k, v in grads.items():
        if k in eng.frozen_names:
            continue
        print(f"  {k}: err {maxdiff(got[k], v):.3e} tol {grad_tol(v):.3e}")
        assert maxdiff(got[k], v) <= grad_tol(v), (k, maxdiff(got[k], v), grad_tol(v))
    return got


@pytest.mark.parametrize("gemm_mode", [0, 2])
@pytest.mark.parametrize("name,prob,sampler", [("untied", 0.5, "multinomial"), ("tied", 0.5, "top-k"), ("one", 0.5, "multinomial"),
                                               ("untied", 1.0, "argmax"), ("tied", 1.0, "top-p")])
def test_train_step_draws_values_and_gradients(name, prob, sampler, gemm_mode):
    m = medium(name)
    sampler = SAMPLERS[sampler]
    seed = pick_seed(m, prob)
    eng = engine(m, gemm_mode)
    args = inputs(m)
    loss, kld = eng.forward(*args, ss_prob=prob, ss_sampler=sampler, ss_seed=seed)
    logits = eng.workspace_view(9).clone()                                      # (the backward overwrites the block)
    fed_ids = check_draws(m, eng, prob, sampler, seed, logits)
    if prob == 1.0:
        assert np.array_equal(eng.fed_mask().cpu().numpy(), m["elig"])          # every eligible position is fed by the model
    gl, gk = upstream(m)
    got = check_step(m, eng, loss, kld, reference(m, fed_ids), gl, gk, f"{name} prob {prob} gemm_mode {gemm_mode}")
    if not m["cfg"].tied:
        # the embedding table is what tells the fed ids from the targets: rows only the model's words touch have a gradient
        ge = got["_embedding_layer.weight"].cpu()
        only_fed = sorted(set(fed_ids[eng.fed_mask().cpu()].tolist()) - set(m["tok"][:-1].reshape(-1).tolist()) - {0})
        assert only_fed and all(float(ge[i].abs().max()) > 0 for i in only_fed)
        assert float(ge[0].abs().max()) == 0
    # the phased backward reads the same ids: the same gradients, bit for bit
    eng.forward(*args, ss_prob=prob, ss_sampler=sampler, ss_seed=seed)
    eng.backward_phased(gl, gk, (16, 32, 64, 8, 4, 128))
    for k, v in eng.grad_dict().items():
        assert k in eng.frozen_names or torch.equal(bits(v), bits(got[k])), k
    # determinism: the same seed twice gives the same bits; another seed feeds other ids
    loss2, kld2 = eng.forward(*args, ss_prob=prob, ss_sampler=sampler, ss_seed=seed)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(kld2), bits(kld))
    assert torch.equal(eng.input_tokens().cpu(), fed_ids)
    eng.backward(gl, gk)
    for k, v in eng.grad_dict().items():
        assert k in eng.frozen_names or torch.equal(bits(v), bits(got[k])), k
    if sampler[:2] != (1, 1):                                                   # (arg-max at prob 1 draws no noise)
        eng.forward(*args, ss_prob=prob, ss_sampler=sampler, ss_seed=seed + 1)
        assert not torch.equal(eng.input_tokens().cpu(), fed_ids)


@pytest.mark.parametrize("name", ["untied", "tied"])
def test_zero_probability_is_the_step_without_the_arguments(name):
    m = medium(name)
    args = inputs(m)
    gl, gk = upstream(m)
    res = []
    for kw in ({}, dict(ss_prob=0.0), dict(ss_prob=0.0, ss_sampler=SAMPLERS["top-k"], ss_seed=99)):
        eng = engine(m)
        loss, kld = eng.forward(*args, **kw)
        assert torch.equal(eng.input_tokens().cpu(), m["tok"][:-1]) and not bool(eng.fed_mask().any())
        nll = eng.nll().clone()
        eng.backward(gl, gk)
        grads = eng.grads.flat.clone()
        step = engine(m)
        step.train_step(*args, **STEP, **kw)
        res.append([loss.clone(), kld.clone(), nll, grads, step.params.flat.clone()])
    for other in res[1:]:
        for x, y in zip(res[0], other):
            assert torch.equal(bits(x), bits(y))
    # ... and a sampled forward does not leave anything behind that the next unsampled step reads
    eng = engine(m)
    eng.forward(*args, ss_prob=1.0, ss_seed=3)
    loss, kld = eng.forward(*args)
    eng.backward(gl, gk)
    assert torch.equal(bits(loss), bits(res[0][0])) and torch.equal(bits(eng.grads.flat), bits(res[0][3]))


def test_composes_with_label_smoothing_and_free_bits():
    base = medium("untied")
    seed = pick_seed(base, 0.5)
    args = inputs(base)
    gl, gk = upstream(base)
    w = torch.from_numpy(base["w"]).double()
    # the floor: picked from the restated latents of the forward the device runs (its fed ids), with the margin
    # tests/test_free_bits_gpu.py asks for - as there, fc_mean / fc_log_var are scaled by the first pair that leaves that margin
    for ws, bs in SCALES:
        m = dict(base)
        m["params"] = dict(base["params"])
        for n in ("fc_mean", "fc_log_var"):
            m["params"][P_CELL + n + ".weight"] = base["params"][P_CELL + n + ".weight"] * ws
            m["params"][P_CELL + n + ".bias"] = base["params"][P_CELL + n + ".bias"] * bs
        eng = engine(m)
        eng.forward(*args, ss_prob=0.5, ss_sampler=MULTI, ss_seed=seed)
        fed_ids = eng.input_tokens().cpu().clone()
        with torch.no_grad():
            out = R.train_forward_fed(m["params"], m["cfg"], m["feats"], m["caps"], m["senti"], m["eps"], fed_ids, return_steps=True)
        stack = lambda key: torch.stack([s_[key] for s_ in out["steps"]], 0)
        k = fr.k_elem(stack("mean"), stack("log_var"), stack("prior_mean"), m["cfg"].prior_std ** 2, 0)
        lam, half = fr.pick_lambda(fr.compared(k, w, 1)[w.bool()])
        kld_ref, gate, _ = fr.floored(k, w, lam, 1)
        if bool(gate[w.bool()].any()) and not bool(gate[w.bool()].all()) and half >= 10 * val_tol(kld_ref):
            break
    else:
        raise AssertionError("no scale of fc_mean / fc_log_var leaves the floor its margin")
    loss, kld = eng.forward(*args, label_smoothing=0.1, free_bits=lam, free_bits_mode="element", ss_prob=0.5, ss_sampler=MULTI,
                            ss_seed=seed)
    assert torch.equal(eng.input_tokens().cpu(), fed_ids)                       # neither option moves a logit or a draw
    ref = reference(m, fed_ids, label_smoothing=0.1, floor=(lam, 1))
    check_step(m, eng, loss, kld, ref, gl, gk, "smoothing 0.1 + element floor")
    plain = reference(m, fed_ids)
    assert maxdiff(loss, plain[0]) > 1e-3 and maxdiff(kld, plain[1]) > 10 * val_tol(plain[1])   # (both options did move the values)
    # the fused step: kl_beta rides along as before
    a, b = engine(m), engine(m)
    kw = dict(label_smoothing=0.1, free_bits=lam, free_bits_mode="element", ss_prob=0.5, ss_sampler=MULTI, ss_seed=seed)
    a.train_step(*args, kl_beta=0.5, **STEP, **kw)
    b.forward(*args, **kw)
    b.backward_update(gl, 0.5 * gk, **{k_: v for k_, v in STEP.items() if k_ != "kld_weight"})
    assert torch.equal(bits(a.params.flat), bits(b.params.flat))
    assert torch.equal(a.input_tokens().cpu(), fed_ids)


# ---- overlapped backward on one rank ----------------------------------------------------------------------------------------
def _rccl_worker(port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    m = medium("untied")
    seed = pick_seed(m, 0.5)
    eng = engine(m)
    eng.dp_force = True
    args = inputs(m)
    gl, gk = upstream(m)
    kw = dict(ss_prob=0.5, ss_sampler=MULTI, ss_seed=seed)
    eng.forward(*args, **kw)
    eng.backward(gl, gk)
    plain = eng.grads.flat.clone()
    eng.grads.flat.zero_()
    eng.forward(*args, **kw)
    world = eng.backward_overlapped(gl, gk)
    torch.cuda.synchronize()
    same = torch.equal(bits(eng.grads.flat), bits(plain))
    eng.forward(*args)
    eng.backward(gl, gk)
    moved = not torch.equal(bits(eng.grads.flat), bits(plain))
    ret.put((world, same, moved))
    dist.destroy_process_group()


def test_overlapped_backward_scatters_by_the_fed_ids_on_one_rank():
    from test_dp_gpu import _join_then_get
    ctx = mp.get_context("spawn")
    ret = ctx.SimpleQueue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = ctx.Process(target=_rccl_worker, args=(port, ret))
    p.start()
    world, same, moved = _join_then_get([p], ret)
    assert world == 1 and same and moved


# ---- neighbours, module -----------------------------------------------------------------------------------------------------
def build_model(cfg, params, beam=5):
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    mod = UpDownCaptioner(Vocabulary.synthetic(cfg.vocab_size), cfg.image_feature_size, cfg.embedding_size, cfg.hidden_size,
                          cfg.attention_projection_size, max_caption_length=cfg.max_caption_length, beam_size=beam,
                          use_cbs=cfg.tied, z_space=cfg.z_space, prior_std=cfg.prior_std, simple_vae=cfg.simple_vae,
                          latent_embedding="glove", sentiment_vae=cfg.sentiment_vae, senti_prior_multip=cfg.senti_prior_multip,
                          device=torch.device("cuda"))
    mod.load_state_dict(dict(params))
    return mod.cuda()


def test_module_autograd_path_samples_and_differentiates():
    m = medium("untied")                                                        # (E = 100: no GloVe table to load)
    seed = pick_seed(m, 0.5)
    feats, caps, senti, eps = inputs(m)
    eng = engine(m)
    loss, kld = eng.forward(feats, caps, senti, eps, ss_prob=0.5, ss_sampler=MULTI, ss_seed=seed)
    fed_ids = eng.input_tokens().cpu().clone()
    mod = build_model(m["cfg"], m["params"])
    mod.train()
    mod._eps_override = m["eps"]
    off = mod(feats, None, None, caps, senti)                                   # the default is off
    assert not bool(mod._engine().fed_mask().any())
    mod.scheduled_sampling(0.5, seed)
    out = mod(feats, None, None, caps, senti)
    assert torch.equal(bits(out["loss"]), bits(loss)) and torch.equal(bits(out["kld"]), bits(kld))
    assert not torch.equal(bits(out["loss"]), bits(off["loss"]))
    assert torch.equal(mod._engine().input_tokens().cpu(), fed_ids)
    (out["loss"].mean() + out["kld"].mean() / m["cfg"].kld_weight).backward()
    _, _, grads = reference(m, fed_ids)
    named = dict(mod.named_parameters())
    for k, v in grads.items():
        assert maxdiff(named[k].grad, v) <= grad_tol(v), k
    mod.scheduled_sampling(0.0)
    again = mod(feats, None, None, caps, senti)
    assert torch.equal(bits(again["loss"]), bits(off["loss"]))
    with pytest.raises(ValueError, match="ss_prob"):
        mod.scheduled_sampling(1.5)


def test_posterior_and_likelihood_scores_never_sample():
    m = medium("untied")
    seed = pick_seed(m, 0.5)
    feats, caps, senti, eps = inputs(m)
    res = []
    for prob in (0.0, 0.5):
        mod = build_model(m["cfg"], m["params"])
        mod.train()
        mod._eps_override = m["eps"]
        mod.scheduled_sampling(prob, seed)
        out = mod(feats, None, None, caps, senti)                                # leaves the engine at this captioner's setting
        post = mod._engine().posterior_forward(feats, caps, senti, eps)
        torch.manual_seed(3)                                                     # (both score calls draw their noise from it)
        sc = mod.score_captions(feats, caps, senti, n_samples=2)
        ps = mod.posterior_score_captions(feats, caps, senti, n_samples=1, eps=eps)
        res.append((out["loss"].detach().clone(), [t.clone() for t in post], sc, ps))
    (l0, p0, s0, q0), (l1, p1, s1, q1) = res
    assert not torch.equal(l0, l1)                                              # (the training forwards did differ)
    for x, y in zip(p0, p1):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(bits(p1[0]), bits(l0))                                   # its nll is the teacher-forced loss
    assert torch.equal(bits(s0.log_probs), bits(s1.log_probs)) and torch.equal(bits(s0.marginal), bits(s1.marginal))
    for f in ("log_w", "kld", "elbo"):
        assert torch.equal(bits(getattr(q0, f)), bits(getattr(q1, f))), f


def test_self_critical_step_never_samples():
    """A captioner with a schedule set - and fresh from a sampled training forward - takes the self-critical step of one without,
    bit for bit (the smallest fixture of tests/test_scst_gpu.py)."""
    from test_scst_gpu import HP, N_, P_, SEED, setup
    s = setup(1, 0)
    cfg = s["cfg"]
    res = []
    for prob in (0.0, 1.0):
        mod = build_model(cfg, s["params"], beam=1)
        mod.train()
        ro = s["ro"]
        mod._eps_override = ro.train_eps
        mod.scheduled_sampling(prob, 11)
        out = mod(ro.feats, None, None, ro.caps, ro.sentiment.view(-1, 1))
        mod._eps_override = None
        loss, kld, stats = mod.scst_step(s["feats"], [0, 1, 2], s["senti"].view(P_, 1), references=s["references"], seed=SEED,
                                         n_samples=N_, decoder_frozen=False, **HP)
        res.append((out["loss"].detach().clone(), loss.clone(), kld.clone(), stats.clone(), mod._eng.params.flat.clone()))
    a, b = res
    assert not torch.equal(a[0], b[0])                                          # (the training forwards did differ)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x.cpu().contiguous().view(torch.uint8), y.cpu().contiguous().view(torch.uint8))


# ---- full width -------------------------------------------------------------------------------------------------------------
def test_full_width_c2_step():
    """C2's widths (B = 64, V = 10 000, E = 1000, H = 1200) with captions cut to 3 tokens for the CPU restatement: the real kernel
    forms of the per-step 64 x 1200 x 10 000 head and the 64 x 1000 x 4800 gate block.  Draws, loss, kld, embedding gradient."""
    dims = dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=3)
    B, Rg = 64, 36
    cfg = oracle.OracleConfig(vocab_size=dims["V"], image_feature_size=dims["F"], embedding_size=dims["E"], hidden_size=dims["H"],
                              attention_projection_size=dims["A"], z_space=dims["Z"], max_caption_length=dims["L"], sentiment_vae=1,
                              senti_prior_multip=0.5)
    params = oracle.init_params(cfg, seed=11)
    g = torch.Generator().manual_seed(23)
    feats = torch.randn(B, Rg, dims["F"], generator=g)
    caps = torch.zeros(B, 3, dtype=torch.long)
    for b in range(B):
        n = 3 if b % 4 else 2
        caps[b, :n] = torch.randint(2, dims["V"], (n,), generator=g)
    caps[5, 1] = 0
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(4, B, dims["Z"], generator=g)
    tok, w = R.tokens_and_weights(cfg, caps)
    m = dict(cfg=cfg, params=params, feats=feats, caps=caps, senti=senti, eps=eps, B=B, T=4, V=dims["V"], tok=tok, w=w.numpy(),
             elig=R.eligible(w.numpy()))
    seed = pick_seed(m, 0.5)
    eng = engine(m)
    loss, kld = eng.forward(*inputs(m), ss_prob=0.5, ss_sampler=SAMPLERS["multinomial"], ss_seed=seed)
    logits = eng.workspace_view(9).clone()
    fed_ids = check_draws(m, eng, 0.5, SAMPLERS["multinomial"], seed, logits)
    prev = torch.get_num_threads()
    torch.set_num_threads(min(16, prev))
    try:
        want_loss, want_kld, grads = reference(m, fed_ids)
    finally:
        torch.set_num_threads(prev)
    assert maxdiff(loss, want_loss) <= val_tol(want_loss) and maxdiff(kld, want_kld) <= val_tol(want_kld)
    gl, gk = upstream(m)
    eng.backward(gl, gk)
    k = "_embedding_layer.weight"
    got = eng.grad_dict()[k]
    print(f"full width: loss err {maxdiff(loss, want_loss):.3e}, emb grad err {maxdiff(got, grads[k]):.3e} tol {grad_tol(grads[k]):.3e}")
    assert maxdiff(got, grads[k]) <= grad_tol(grads[k])


# ---- script -----------------------------------------------------------------------------------------------------------------
def _train(tmp_path, name, extra, fused=True, stop=4):
    from test_scripts_gpu import YAML
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    out = tmp_path / name
    args = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--zero-eps", "--serialization-dir", str(out), "--stop-after", str(stop),
            "--checkpoint-every", "2"] + (["--fused-optimizer"] if fused else []) + extra
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out, [json.loads(x) for x in open(out / "scalars.jsonl")]


def test_train_script_follows_the_schedule_and_resumes(tmp_path):
    keys = ["--config-override", "OPTIM.SCHEDULED_SAMPLING_START", "0", "OPTIM.SCHEDULED_SAMPLING_INCREASE_EVERY", "1",
            "OPTIM.SCHEDULED_SAMPLING_INCREASE_PROB", "0.25", "OPTIM.SCHEDULED_SAMPLING_MAX_PROB", "0.5"]
    out, log = _train(tmp_path, "ss", keys)
    assert [rec["iteration"] for rec in log] == [1, 2, 3, 4]
    assert [rec["ss_prob"] for rec in log] == [0.0, 0.25, 0.5, 0.5]            # iteration i: ss_prob(i - 1, 0, 1, 0.25, 0.5)
    assert log[0]["ss_fed_share"] == 0.0 and all(0.0 < rec["ss_fed_share"] < 1.0 for rec in log[1:])
    assert "SCHEDULED_SAMPLING_START: 0" in open(out / "config.yml").read()
    # a run resumed at the checkpoint of iteration 2 draws what the uninterrupted run drew: the same log lines
    _, res = _train(tmp_path, "resumed", keys + ["--start-from-checkpoint", str(out / "checkpoint_2.pth")])
    strip = lambda rec: {k: v for k, v in rec.items() if k != "elapsed_s"}
    assert [strip(r) for r in res] == [strip(r) for r in log[2:]]
    # the autograd path follows the same schedule with the same seeds
    _, auto = _train(tmp_path, "autograd", keys, fused=False)
    assert [rec["ss_prob"] for rec in auto] == [0.0, 0.25, 0.5, 0.5]
    assert auto[0]["ss_fed_share"] == 0.0 and all(0.0 < rec["ss_fed_share"] < 1.0 for rec in auto[1:])
    assert abs(auto[0]["3loss"] - log[0]["3loss"]) < 1e-3
