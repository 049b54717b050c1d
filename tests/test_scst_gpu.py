"""GPU: the self-critical training step.  ssc_scst_prepare (pack + advantage kernels) bit for bit against tests/scstref.py; the
rollout (DecodeEngine.sample -> ssc_eval_score -> ssc_scst_prepare) against its three legs called directly; every parameter
gradient of the advantage-weighted step against autograd on the CPU oracle; SelfCritical.step against its manual composition;
scripts/train.py --scst-references end to end, with resume."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import scstref as R
from gpuutil import dims_from_cfg, maxdiff
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.engine import TrainEngine
from ssc_runtime.evaluation import CaptionReferences
from ssc_runtime.scst import SelfCritical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1
OUTS = (("caps", torch.int64), ("lengths", torch.int32), ("reward", torch.float32), ("advantage", torch.float32),
        ("gl", torch.float32), ("gk", torch.float32), ("stats", torch.float64))


def bits(t):
    t = torch.as_tensor(t).cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def raw_prepare(pred, scores, base, L_, baseline, w, loss_scale, kld_scale, P=None, N=None):
    """ssc_scst_prepare on sentinel-filled outputs -> (return code, outputs): what a refused call leaves is visible."""
    lib = L.load()
    P = scores.shape[0] if P is None else P
    N = scores.shape[1] if N is None else N
    G, steps = pred.shape
    out = {"caps": torch.full((G, max(L_, 1)), -7, dtype=torch.int64, device="cuda")}
    out["lengths"] = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    for k in ("reward", "advantage", "gl", "gk"):
        out[k] = torch.full((G,), -7.0, dtype=torch.float32, device="cuda")
    out["stats"] = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    d = L.ScstDesc()
    d.P, d.N, d.steps, d.L, d.end_index, d.baseline = P, N, steps, L_, END, baseline
    d.predictions, d.scores, d.base_scores = pred.data_ptr(), scores.data_ptr(), base.data_ptr() if base is not None else None
    for k in range(6):
        d.reward_weights[k] = w[k]
    d.loss_scale, d.kld_scale = loss_scale, kld_scale
    for k, _ in OUTS:
        setattr(d, k, out[k].data_ptr())
    rc = lib._raw_ssc_scst_prepare(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def untouched(out):
    return all(bool((v == -7).all()) for v in out.values())


# ---- 1. pack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("PN", [(1, 1), (1, 5), (26, 5)])          # G = 1, 5, 130: one wave, one workgroup and a part, 33 workgroups
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("steps", [1, 7, 20])
def test_pack_matches_the_restatement(steps, extra, PN):
    P, N = PN
    G = P * N
    g = torch.Generator().manual_seed(100 * steps + 10 * extra + G)
    for shift in range(5):
        pred = torch.randint(2, 30, (G, steps), generator=g)
        pred[torch.rand(G, steps, generator=g) < 0.08] = END
        for r in range(G):
            kind = (r + shift) % 5
            if kind == 0:
                pred[r, 0] = END                                    # ends in column 0
            elif kind == 1:
                pred[r][pred[r] == END] = 3
                pred[r, steps - 1] = END                            # ends in the last column
            elif kind == 2:
                pred[r][pred[r] == END] = 4                         # never ends
            elif kind == 3:
                pred[r, steps // 2] = 0                             # holds id 0 (before or after its end)
                pred[r, 0] = 0 if steps > 1 else pred[r, 0]
        scores = torch.zeros(P, N, 6, dtype=torch.float64, device="cuda")
        rc, out = raw_prepare(pred.cuda(), scores, None, steps + extra, 0, (0,) * 5 + (1,), 1.0, 1.0)
        assert rc == 0
        caps, lengths = R.pack(pred.numpy(), END, steps + extra)
        assert torch.equal(out["caps"].cpu(), torch.from_numpy(caps)) and torch.equal(out["lengths"].cpu(), torch.from_numpy(lengths))
        share = float((lengths == steps).sum()) / G
        assert abs(float(out["stats"][3]) - share) <= 1e-12 * share
    rc, out = raw_prepare(pred.cuda(), scores, None, steps - 1, 0, (0,) * 5 + (1,), 1.0, 1.0)
    assert rc == -1 and untouched(out)                              # L < steps: SSC_EINVAL, nothing written


# ---- 2. advantage -----------------------------------------------------------------------------------------------------------
WEIGHTS = ((0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.1, 0.0, 0.3, 0.5, 0.25, 1.0), (1 / 3, 0.7, 0.0, 1e-3, 2.0, 0.6))


@pytest.mark.parametrize("P", [1, 3, 70])
@pytest.mark.parametrize("N", [1, 2, 5, 64, 65, 128])
def test_advantage_matches_the_restatement(N, P):
    g = np.random.default_rng(1000 * N + P)
    s = g.random((P, N, 6))
    s[..., 5] *= 10
    if N >= 2:
        s[0, 1] = s[0, 0]                                           # exact duplicates within an image
        s[0, N - 1] = s[0, 0]
    if P >= 3:
        s[1] = 0                                                    # an all-zero image (no references)
    base = g.random((P, 6))
    base[P - 1] = s[P - 1, 0]                                       # a baseline equal to a sample
    steps = 4
    pred = torch.randint(0, 6, (P * N, steps), generator=torch.Generator().manual_seed(N + P)).cuda()
    lengths = R.pack(pred.cpu().numpy(), END, steps)[1]
    sd, bd = torch.from_numpy(s).cuda(), torch.from_numpy(base).cuda()
    G = P * N
    for w in WEIGHTS[1:]:
        for baseline in (0, 1, 2):
            ls, ks = 1.0 / G, 1.0 / (G * 750.0)
            rc, out = raw_prepare(pred, sd, bd if baseline == 2 else None, steps, baseline, w, ls, ks)
            if baseline == 1 and N == 1:
                assert rc == -1 and untouched(out)                  # SSC_EINVAL: no other sample to average
                continue
            assert rc == 0
            want = R.advantage(s, base, w, baseline, ls, ks, lengths, steps)
            for k in ("reward", "advantage", "gl", "gk"):
                assert same_bits(out[k], torch.from_numpy(want[k])), (k, w, baseline)
            got = out["stats"].cpu().numpy()
            assert (np.abs(got - want["stats"]) <= 1e-12 * np.abs(want["stats"])).all(), (got, want["stats"])
            if baseline == 1 and N == 2:
                assert float(out["advantage"][0]) == 0.0 and float(out["advantage"][1]) == 0.0
            if baseline == 1 and P >= 3:
                assert bool((out["advantage"][N:2 * N] == 0).all()) and bool((out["reward"][N:2 * N] == 0).all())
    rc, out = raw_prepare(pred, sd, None, steps, 2, WEIGHTS[0], 1.0, 1.0)
    assert rc == -1 and untouched(out)                              # SSC_EINVAL: a given baseline without base_scores


# ---- 3. rollout ---------------------------------------------------------------------------------------------------------
P_, N_, R_, SEED = 3, 4, 5, 20261017


def toy_cfg(sv):
    return oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32, attention_projection_size=16,
                               z_space=8, max_caption_length=9, sentiment_vae=sv, senti_prior_multip=0.5, beam_size=1)


def engines(cfg, params, mode):
    dims = dims_from_cfg(cfg)
    dims.gemm_mode = mode
    eng = TrainEngine(dims, "cuda")
    eng.load_state_dict(params)
    return eng, DecodeEngine(eng.dims, eng.params.c_struct, "cuda")


def words_of(cfg):
    return ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, cfg.vocab_size)]


def caption(row, words):
    out = []
    for t in row.tolist():
        if t == END:
            break
        if t != 0:
            out.append(words[t])
    return out


@functools.lru_cache(maxsize=None)
def setup(sv, mode, baseline="loo"):
    """One model, its engines, references made from its own samples, and one rollout: shared by the tests below, changed by none."""
    cfg = toy_cfg(sv)
    params = oracle.init_params(cfg, seed=7)
    params["_output_layer.bias"][END] += 1.0
    eng, dec = engines(cfg, params, mode)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(P_, R_, cfg.image_feature_size, generator=g).cuda()
    senti = torch.tensor([1.0, -1.0, 0.0]).cuda()
    steps, G, Z = cfg.max_caption_length, P_ * N_, cfg.z_space
    # sample first (the rollout's noise: a device generator seeded with the rollout's seed), then make the references from the samples
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED)
    eps0 = torch.randn(G, Z, device="cuda", generator=gen)
    eps = torch.randn(steps - 1, G, Z, device="cuda", generator=gen)
    first, _ = dec.sample(dec.prepare(feats), senti.repeat_interleave(N_), N_, steps, END, eps0, eps, sampling.MultinomialSampler(), SEED)
    words = words_of(cfg)
    refs = {}
    for p in range(P_):
        a = caption(first[p * N_], words) or ["w2", "w3"]
        b = caption(first[p * N_ + 1], words) or ["w4", "w5", "w6"]
        b = [w if i % 2 == 0 else words[2 + (i * 7 + p) % 50] for i, w in enumerate(b)]     # every second word replaced
        refs[p] = [" ".join(a), " ".join(b)]
    references = CaptionReferences(refs)
    scst = SelfCritical(eng, dec, references, words, n_samples=N_, baseline=baseline, max_steps=steps)
    ro = scst.rollout(feats, [0, 1, 2], senti, SEED)
    return dict(cfg=cfg, params=params, eng=eng, dec=dec, feats=feats, senti=senti, first=first, words=words, references=references,
                scst=scst, ro=ro, steps=steps)


def padded_scores(references, pred3, words, ids):
    """CaptionReferences.score wants five captions per image (its top-5 statistics): the first caption is repeated up to five. A
    caption's scores do not depend on its neighbours, so the first N columns are the scores of the N captions."""
    P, N, _ = pred3.shape
    pad = torch.cat([pred3] + [pred3[:, :1]] * max(0, 5 - N), dim=1)
    res = references.score(pad, END, words, image_ids=ids)
    return res.bleu[:, :N], res.rouge[:, :N], res.cider[:, :N]


def test_rollout_equals_its_legs_called_directly():
    s = setup(1, 0)
    ro, dec, scst = s["ro"], s["dec"], s["scst"]
    G = P_ * N_
    assert torch.equal(ro.predictions, s["first"])
    again, _ = dec.sample(dec.prepare(s["feats"]), ro.sentiment, N_, s["steps"], END, ro.eps0, ro.eps, sampling.MultinomialSampler(),
                          ro.word_seed)
    assert torch.equal(ro.predictions, again)
    Lc = ro.predictions.size(1)
    _, _, cider = padded_scores(s["references"], ro.predictions.view(P_, N_, Lc), s["words"], [0, 1, 2])
    sc = ro.scores.cpu().numpy()
    assert np.array_equal(sc[:, :, 5].view(np.int64), cider.view(np.int64))
    assert same_bits(ro.reward, torch.from_numpy(cider.reshape(G).astype(np.float32)))
    want = R.advantage(sc, None, (0, 0, 0, 0, 0, 1), 1, 1.0 / G, 1.0 / (G * 750.0))
    # a condition on the INPUT, by the restatement alone: the rewards differ enough for the weighted gradient to mean something
    print("rollout |advantage|:", np.abs(want["advantage64"]).round(4).tolist())
    assert (np.abs(want["advantage64"]) > 1e-3).sum() >= G // 2
    caps, lengths = R.pack(ro.predictions.cpu().numpy(), END, Lc)
    assert torch.equal(ro.caps.cpu(), torch.from_numpy(caps)) and torch.equal(ro.lengths.cpu(), torch.from_numpy(lengths))
    for k in ("reward", "advantage", "gl", "gk"):
        assert same_bits(getattr(ro, k), torch.from_numpy(want[k])), k
    want = R.advantage(sc, None, (0, 0, 0, 0, 0, 1), 1, 1.0 / G, 1.0 / (G * 750.0), lengths, Lc)
    assert (np.abs(ro.stats.cpu().numpy() - want["stats"]) <= 1e-12 * np.abs(want["stats"])).all()
    assert tuple(ro.feats.shape) == (G, R_, 48) and torch.equal(ro.feats[N_ + 1], s["feats"][1])
    assert tuple(ro.train_eps.shape) == (Lc + 1, G, 8)
    # an image without references: reward 0, advantage 0
    ro2 = scst.rollout(s["feats"], [0, "nope", 2], s["senti"], SEED)
    assert bool((ro2.reward[N_:2 * N_] == 0).all()) and bool((ro2.advantage[N_:2 * N_] == 0).all())
    assert same_bits(ro2.reward[:N_], ro.reward[:N_]) and torch.equal(ro2.predictions, ro.predictions)


def test_rollout_greedy_baseline():
    s = setup(1, 0, "greedy")
    ro, dec = s["ro"], s["dec"]
    G, Z, steps = P_ * N_, 8, s["steps"]
    z0, zs = torch.zeros(P_, Z, device="cuda"), torch.zeros(steps - 1, P_, Z, device="cuda")
    want, _ = dec.sample(dec.prepare(s["feats"]), s["senti"], 1, steps, END, z0, zs, sampling.TopKSampler(k=1), 99)
    assert torch.equal(ro.base_predictions, want)
    assert torch.equal(ro.predictions, s["first"])                  # the samples do not depend on the baseline
    b = padded_scores(s["references"], want.view(P_, 1, -1), s["words"], [0, 1, 2])
    got = ro.base_scores.cpu().numpy()
    assert np.array_equal(got[:, 5].view(np.int64), b[2][:, 0].view(np.int64))
    ref = R.advantage(ro.scores.cpu().numpy(), got, (0, 0, 0, 0, 0, 1), 2, 1.0 / G, 1.0 / (G * 750.0))
    for k in ("reward", "advantage", "gl", "gk"):
        assert same_bits(getattr(ro, k), torch.from_numpy(ref[k])), k


def test_rollout_refuses_what_it_cannot_do():
    s = setup(1, 0)
    with pytest.raises(ValueError, match="image ids"):
        s["scst"].rollout(s["feats"], [0, 1], s["senti"], 1)
    s["dec"].weights_frozen = True
    try:
        with pytest.raises(ValueError, match="weights_frozen"):
            s["scst"].rollout(s["feats"], [0, 1, 2], s["senti"], 1)
    finally:
        s["dec"].weights_frozen = False
    with pytest.raises(ValueError, match="leave-one-out"):
        SelfCritical(s["eng"], s["dec"], s["references"], s["words"], n_samples=1)
    with pytest.raises(ValueError, match="words"):
        SelfCritical(s["eng"], s["dec"], s["references"], s["words"][:-1], n_samples=2)


# ---- 4. gradient parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sv,mode", [(1, 0), (1, 2), (0, 0), (0, 2)])     # SENTIMENT_VAE 1 / 0; default GEMM mode / exact fp32
def test_every_gradient_matches_autograd_of_the_weighted_objective(sv, mode):
    """Device backward with the rollout's gl / gk against autograd of sum gl loss + sum gk kld on oracle.train_forward with the same
    caps, eps and sentiment: every parameter, 1e-4 of the tensor's scale (the bound of
    test_train_gpu.test_full_size_c2_matches_oracle_every_gradient)."""
    s = setup(sv, mode)
    ro, eng, cfg = s["ro"], s["eng"], s["cfg"]
    G = P_ * N_
    adv = R.advantage(ro.scores.cpu().numpy(), None, (0, 0, 0, 0, 0, 1), 1, 1.0 / G, 1.0 / (G * 750.0))["advantage64"]
    assert (np.abs(adv) > 1e-3).sum() >= G // 2
    p = {k: v.clone().requires_grad_(True) for k, v in s["params"].items()}
    R.objective(p, cfg, ro.feats.cpu(), ro.caps.cpu(), ro.sentiment.cpu().view(G, 1), ro.train_eps.cpu(), ro.gl.cpu(),
                ro.gk.cpu()).backward()
    eng.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
    eng.backward(ro.gl, ro.gk)
    got = eng.grad_dict()
    worst = {}
    for k, v in p.items():
        scale = max(v.grad.abs().max().item(), 1e-6)
        worst[k] = maxdiff(got[k], v.grad) / scale
    print("gradient error / scale:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in p.items():
        scale = max(v.grad.abs().max().item(), 1e-6)
        assert maxdiff(got[k], v.grad) <= 1e-4 * scale + 1e-7, (k, maxdiff(got[k], v.grad), scale)


# ---- 5. step composition ----------------------------------------------------------------------------------------------------
HP = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=12.5)


def fresh(s, baseline="loo"):
    eng, dec = engines(s["cfg"], s["params"], 0)
    return eng, SelfCritical(eng, dec, s["references"], s["words"], n_samples=N_, baseline=baseline, max_steps=s["steps"])


def state(eng):
    return eng.params.flat.clone(), eng.momentum.clone()


@pytest.mark.parametrize("frozen", [False, True])
def test_step_equals_its_manual_composition(frozen):
    s = setup(1, 0)
    a, sa = fresh(s)
    b, sb = fresh(s)
    c, sc = fresh(s)
    loss, kld, stats = sa.step(s["feats"], [0, 1, 2], s["senti"], seed=SEED, decoder_frozen=frozen, **HP)
    ro = sb.rollout(s["feats"], [0, 1, 2], s["senti"], SEED, kld_weight=HP["kld_weight"])
    loss_b, kld_b = b.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
    b.backward(ro.gl, ro.gk, skip=b.decoder_names if frozen else ())
    b.clip_sgd_step(HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"], frozen)
    assert torch.equal(loss, loss_b) and torch.equal(kld, kld_b) and same_bits(stats, ro.stats)
    for x, y in zip(state(a), state(b)):
        assert same_bits(x, y)
    assert not torch.equal(a.params.flat, s["eng"].params.flat)    # (the step moved the parameters)
    sc.step(s["feats"], [0, 1, 2], s["senti"], seed=SEED, decoder_frozen=frozen, **HP)
    for x, y in zip(state(a), state(c)):
        assert same_bits(x, y)                                      # same state, same seed: the same bits
    # a second step from the moved parameters, another seed: the rollout reads the parameters as they are NOW
    sa.step(s["feats"], [0, 1, 2], s["senti"], seed=SEED + 1, decoder_frozen=frozen, **HP)
    ro = sb.rollout(s["feats"], [0, 1, 2], s["senti"], SEED + 1, kld_weight=HP["kld_weight"])
    b.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
    b.backward(ro.gl, ro.gk, skip=b.decoder_names if frozen else ())
    b.clip_sgd_step(HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"], frozen)
    for x, y in zip(state(a), state(b)):
        assert same_bits(x, y)


def test_train_step_equals_forward_backward_update_with_constant_upstream():
    s = setup(1, 0)
    ro = s["ro"]
    a, _ = fresh(s)
    b, _ = fresh(s)
    B = ro.caps.size(0)
    for it in range(2):
        la, ka = a.train_step(ro.feats, ro.caps, ro.sentiment, ro.train_eps, **HP)
        lb, kb = b.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
        b.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * HP["kld_weight"]), device="cuda"))
        b.clip_sgd_step(HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"], False)
        assert torch.equal(la, lb) and torch.equal(ka, kb)
        for x, y in zip(state(a), state(b)):
            assert same_bits(x, y)


# ---- 6. script and module ---------------------------------------------------------------------------------------------------
YAML = """
RANDOM_SEED: 2
DATA:
  MAX_CAPTION_LENGTH: 8
  CBS:
    MAX_GIVEN_CONSTRAINTS: 0
MODEL:
  IMAGE_FEATURE_SIZE: 64
  EMBEDDING_SIZE: 40
  HIDDEN_SIZE: 48
  ATTENTION_PROJECTION_SIZE: 32
  BEAM_SIZE: 3
  USE_CBS: False
  MIN_CONSTRAINTS_TO_SATISFY: 0
  Z_SPACE: 16
  SENTIMENT_VAE: 1
  SENTI_PRIOR_MULTIP: 0.5
  SIMPLE_VAE: False
  N_Z_SAMPLES: 4
OPTIM:
  BATCH_SIZE: 4
  NUM_ITERATIONS: 3
  BEFORE_UPDATE_DECODER_EVERY: 2
  EPOCH_START_DECODER_TRAINING: 2
"""


def run(args):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_train_script_runs_self_critical_steps_and_resumes(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    base = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "16", "--vocab-size", "60",
            "--num-boxes", "5", "--checkpoint-every", "1", "--scst-references", "synthetic", "--scst-samples", "4", "--scst-max-steps",
            "8", "--scst-sampler", "top-k", "--scst-top-k", "20", "--scst-reward", "0,0,0,0.5,0,1"]
    a, b = tmp_path / "a", tmp_path / "b"
    run(base + ["--serialization-dir", str(a)])
    log = [json.loads(x) for x in open(a / "scalars.jsonl")]
    assert [r["iteration"] for r in log] == [1, 2, 3]
    for r in log:
        assert r["5reward"] >= 0 and r["6baseline"] >= 0 and r["7abs_advantage"] >= 0 and 0 <= r["8no_end_share"] <= 1
        assert np.isfinite([r["1reconstr_loss"], r["2kld_loss"], r["3loss"]]).all()
    run(base + ["--serialization-dir", str(b), "--start-from-checkpoint", str(a / "checkpoint_2.pth")])
    want = torch.load(a / "checkpoint_3.pth", map_location="cpu", weights_only=True)
    got = torch.load(b / "checkpoint_3.pth", map_location="cpu", weights_only=True)
    assert set(want) == {"model", "optimizer"} == set(got) and got["optimizer"]["iteration"] == 3
    for k, v in want["model"].items():
        assert same_bits(got["model"][k], v), k
    for i, st in want["optimizer"]["state"].items():
        assert same_bits(got["optimizer"]["state"][i]["momentum_buffer"], st["momentum_buffer"]), i
    assert [json.loads(x) for x in open(b / "scalars.jsonl")][0]["5reward"] == log[2]["5reward"]


def test_module_scst_step_matches_the_engine_level_step():
    from test_module_gpu import build_model
    s = setup(1, 0)
    m = build_model(s["cfg"], s["params"], beam=1)
    m.train()
    loss, kld, stats = m.scst_step(s["feats"], [0, 1, 2], s["senti"].view(P_, 1), references=s["references"], seed=SEED, n_samples=N_,
                                   decoder_frozen=False, **HP)
    a, sa = fresh(s)
    la, ka, st = sa.step(s["feats"], [0, 1, 2], s["senti"], seed=SEED, **HP)
    assert torch.equal(loss, la) and torch.equal(kld, ka) and same_bits(stats, st)
    sd = m.state_dict()
    for k, v in a.state_dict().items():
        assert same_bits(sd[k], v), k
