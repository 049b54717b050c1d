"""GPU: ssc_eval_select (csrc/caption_select.hip) against the float64 restatement tests/selectref.py on the caption kernels
ssc_eval_set builds from the fixtures' token rows; the fallback and edge cases; determinism; the host layer (select_captions,
CaptionReferences.select, ConsensusBank.select, EvalResult.subset_summary) and both scripts with --select-k.

Bounds (tests/selectref.py): `gains` within selectref.TOL[method] x the image's largest gain - 10 x the float64
disagreement measured on the CPU (DPP: incremental against slogdet, 5.47e-15; MBR: ascending against descending sums, 9.03e-16;
MMR: 0, bit for bit); picks are compared as captions, position by position, by following the device's picks through the
restatement; a position whose best and second-best distinct caption lie within the bound is left out, at most 10 % of a fixture."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import selectref as R
from ssc_runtime import evaluation as E
from ssc_runtime import lib as L
from ssc_runtime.evaluation import CaptionReferences, ConsensusBank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345

_FX = {}


def device_fixture(P, N):
    """The fixture with its caption kernel from ssc_eval_set, computed once and shared: (fx, K on the device, K on the host)."""
    if (P, N) not in _FX:
        fx = R.fixture(P, N)
        _, (ref_off, tok_off, toks, W) = R.fixture_refs(fx)
        prep = E._Prepared.from_csr(ref_off, tok_off, toks, W, "cuda")
        id_map = torch.tensor([0, 0] + list(range(1, fx["V"] - 1)), dtype=torch.int32, device="cuda")
        pred = torch.from_numpy(fx["tokens"]).cuda()
        Kd = E._eval_set_call(pred, 1, fx["V"], prep, id_map, torch.zeros(P, dtype=torch.int32, device="cuda"))[2]
        Kh = Kd.cpu().numpy()
        want = R.fixture_kernel(fx)
        assert np.array_equal(Kh, Kh.transpose(0, 2, 1))
        assert np.abs(Kh - want).max() <= 1e-12           # (the set call's own bound: test_caption_set_gpu.py)
        _FX[P, N] = (fx, Kd, Kh)
    return _FX[P, N]


def raw_select(K, q, k, method, normalize=True, el=None, lam=0.5, theta=1.0, min_gain=1e-10):
    """One ssc_eval_select call on device tensors with the outputs pre-filled: -> (rc, picks, gains, n_primary) on the host."""
    P, N, _ = K.shape
    picks = torch.full((P, k), SENTINEL, dtype=torch.int32, device="cuda")
    gains = torch.full((P, k), float(SENTINEL), dtype=torch.float64, device="cuda")
    nprim = torch.full((P,), SENTINEL, dtype=torch.int32, device="cuda")
    d = L.EvalSelectDesc(P, N, k, method, L.ptr(K), L.ptr(q), int(normalize), lam, theta, min_gain, L.ptr(el), L.ptr(picks),
                         L.ptr(gains), L.ptr(nprim))
    lib = L.load()
    nbytes = lib.ssc_eval_select_workspace_bytes(C.byref(d))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib._raw_ssc_eval_select(C.byref(d), L.ptr(ws), nbytes, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, picks.cpu().numpy().astype(np.int64), gains.cpu().numpy(), nprim.cpu().numpy().astype(np.int64)


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


# ---- kernel against restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,N", R.SHAPES)
def test_kernel_against_restatement_on_caption_kernels(P, N):
    fx, Kd, Kh = device_fixture(P, N)
    q = dev(fx["quality"], torch.float64)
    eld = dev(fx["eligible"], torch.uint8)
    total = skipped = 0
    worst = {R.MBR: 0.0, R.MMR: 0.0, R.DPP: 0.0}
    for method, k, normalize, masked, kw in R.grid(N):
        rc, picks, gains, nprim = raw_select(Kd, q, k, method, normalize, eld if masked else None, **kw)
        assert rc == 0
        assert ((picks >= -1) & (picks < N)).all() and (nprim >= 0).all() and (nprim <= k).all()
        for p in range(P):
            el = fx["eligible"][p] if masked else None
            rule = R.make_rule(method, Kh[p], fx["quality"][p], el, normalize, **kw)
            n, s, dv = R.judge(rule, k, fx["caps"][p], R.TOL[method], picks[p], gains[p], nprim[p])
            got = picks[p][picks[p] >= 0]
            assert len(set(got.tolist())) == len(got)                            # no candidate twice
            if masked:
                assert fx["eligible"][p][got].all()
            total, skipped, worst[method] = total + n, skipped + s, max(worst[method], dv)
    print(f"P {P} N {N}: {total} positions, {skipped} within the margin; largest gain deviation / largest gain: "
          + ", ".join(f"{name} {worst[m]:.3g} (bound {R.TOL[m]:.3g})" for name, m in (("MBR", R.MBR), ("MMR", R.MMR), ("DPP", R.DPP))))
    assert skipped <= R.SKIP_CAP * total


def test_quality_null_for_mbr_and_dpp_with_theta_zero():
    fx, Kd, Kh = device_fixture(5, 20)
    for method, kw in ((R.MBR, {}), (R.DPP, dict(theta=0.0))):
        rc, picks, gains, nprim = raw_select(Kd, None, 20, method, True, None, **kw)
        assert rc == 0
        for p in range(5):
            rule = R.make_rule(method, Kh[p], None, None, True, **kw)
            R.judge(rule, 20, fx["caps"][p], R.TOL[method], picks[p], gains[p], nprim[p])
            if method == R.DPP:   # the fallback without a quality is the index order
                rest = picks[p][nprim[p]:]
                assert list(rest) == sorted(rest)


# ---- fallback and edge cases ------------------------------------------------------------------------------------------------------

def toy_kernel(caps, V=12):
    """(1, N, steps) predictions of the given token lists (ids 2..V-1, boundary 1) -> their kernel on the device."""
    N, steps = len(caps), max(2, max(len(c) for c in caps) + 1)
    pred = np.ones((1, N, steps), dtype=np.int64)
    for n, c in enumerate(caps):
        pred[0, n, :len(c)] = c
    refs = [[(2, 3, 4, 5)], [(6, 7, 8)], [(9, 10, 11, 2)]]
    ref_off, tok_off, toks = [0], [0], []
    for rs in refs:
        for r in rs:
            toks += [t - 1 for t in r]
            tok_off.append(len(toks))
        ref_off.append(len(tok_off) - 1)
    prep = E._Prepared.from_csr(ref_off, tok_off, toks, V - 1, "cuda")
    id_map = torch.tensor([0, 0] + list(range(1, V - 1)), dtype=torch.int32, device="cuda")
    return E._eval_set_call(torch.from_numpy(pred).cuda(), 1, V, prep, id_map, torch.zeros(1, dtype=torch.int32, device="cuda"))[2]


def test_all_identical_captions_dpp_keeps_one_and_falls_back_to_quality():
    K = toy_kernel([[2, 3, 4, 5, 6]] * 6)
    q = torch.tensor([[0.1, 0.9, 0.3, 0.9, -1.0, 0.2]], dtype=torch.float64, device="cuda")
    rc, picks, gains, nprim = raw_select(K, q, 6, R.DPP, True, None, theta=0.0)
    assert rc == 0 and nprim[0] == 1
    assert list(picks[0]) == [0, 1, 3, 2, 5, 4]
    assert gains[0, 0] == K[0, 0, 0].item() and not gains[0, 1:].any()
    # with the quality in the rule the first pick is the best duplicate (the lower index of the two best)
    rc, picks, gains, nprim = raw_select(K, q, 6, R.DPP, True, None, theta=1.0)
    assert rc == 0 and nprim[0] == 1 and list(picks[0]) == [1, 3, 2, 5, 0, 4]


def test_k_beyond_the_eligible_count_gives_minus_one_tails():
    fx, Kd, Kh = device_fixture(5, 20)
    el = np.zeros((5, 20), dtype=np.uint8)
    el[0, [3, 7, 9]] = 1
    el[1, 5] = 1            # one eligible candidate; images 2..4: none
    q = dev(fx["quality"], torch.float64)
    for method in (R.MBR, R.MMR, R.DPP):
        rc, picks, gains, nprim = raw_select(Kd, q, 6, method, True, dev(el, torch.uint8))
        assert rc == 0
        assert sorted(picks[0, :3]) == [3, 7, 9] and (picks[0, 3:] == -1).all() and not gains[0, 3:].any()
        assert picks[1, 0] == 5 and (picks[1, 1:] == -1).all()
        assert (picks[2:] == -1).all() and not gains[2:].any() and not nprim[2:].any()
        if method == R.MBR:
            assert gains[1, 0] == 0.0 and nprim[1] == 1 and nprim[0] == 3
        for p in range(5):
            R.judge(R.make_rule(method, Kh[p], fx["quality"][p], el[p], True), 6, fx["caps"][p], R.TOL[method], picks[p], gains[p],
                    nprim[p])


def test_non_finite_inputs_give_einval_and_that_images_picks_are_minus_one():
    fx, Kd, Kh = device_fixture(5, 20)
    el = np.ones((5, 20), dtype=np.uint8)
    el[3, 4] = 0
    qn = fx["quality"].copy()
    qn[1, 6] = np.nan                      # an eligible candidate: image 1 is refused
    qn[3, 4] = np.inf                      # not eligible: never read as a number
    for method in (R.MBR, R.MMR, R.DPP):
        for k in (5, 20):
            rc, picks, gains, nprim = raw_select(Kd, dev(qn, torch.float64), k, method, True, dev(el, torch.uint8))
            assert rc == -1                                                   # SSC_EINVAL
            assert (picks[1] == -1).all() and not gains[1].any() and nprim[1] == 0
            assert ((picks >= -1) & (picks < 20)).all()                       # every slot written, none out of range
            for p in (0, 2, 3, 4):                                            # the other images are what they would have been
                R.judge(R.make_rule(method, Kh[p], qn[p], el[p], True), k, fx["caps"][p], R.TOL[method], picks[p], gains[p], nprim[p])
    Kn = Kd.clone()
    Kn[2, 3, 8] = Kn[2, 8, 3] = float("inf")
    rc, picks, gains, nprim = raw_select(Kn, dev(fx["quality"], torch.float64), 5, R.DPP)
    assert rc == -1 and (picks[2] == -1).all() and ((picks >= -1) & (picks < 20)).all() and (picks[[0, 1, 3, 4]] >= 0).all()
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        E.select_captions(Kd, dev(qn, torch.float64), k=5, method="mmr", eligible=dev(el, torch.uint8))
    # a masked NaN is no error
    el[1, 6] = 0
    rc, picks, _, _ = raw_select(Kd, dev(qn, torch.float64), 5, R.MMR, True, dev(el, torch.uint8))
    assert rc == 0 and 6 not in picks[1] and (picks >= 0).all()


# ---- determinism -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,k", [(65, 65), (128, 16), (128, 40)])
def test_two_calls_and_permuted_images_are_bit_identical(N, k):
    fx, Kd, _ = device_fixture(5, N)
    q = dev(fx["quality"], torch.float64)
    el = dev(fx["eligible"], torch.uint8)
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    for method in (R.MBR, R.MMR, R.DPP):
        a = raw_select(Kd, q, k, method, True, el)
        b = raw_select(Kd, q, k, method, True, el)
        c = raw_select(Kd[perm].contiguous(), q[perm].contiguous(), k, method, True, el[perm].contiguous())
        assert a[0] == b[0] == c[0] == 0
        pm = perm.cpu().numpy()
        for x, y, z in zip(a[1:], b[1:], c[1:]):
            assert x.tobytes() == y.tobytes()
            assert x[pm].tobytes() == z.tobytes()


# ---- host layer ------------------------------------------------------------------------------------------------------------------

def toy_corpus(P=6, N=8, seed=11):
    rng = np.random.default_rng(seed)
    V = 26
    words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
    pred = np.ones((P, N, 9), dtype=np.int64)
    for p in range(P):
        for n in range(N):
            if n == 5:
                continue                                     # an empty caption
            if n in (3, 6):
                pred[p, n] = pred[p, n - 2]                  # duplicates
                continue
            L_ = int(rng.integers(2, 9))
            pred[p, n, :L_] = rng.integers(2, V, L_)
    refs = {900 + p: [" ".join(f"w{int(t)}" for t in rng.integers(2, V, int(rng.integers(3, 9)))) for _ in range(3)] for p in range(P)}
    bank_caps = [[" ".join(f"w{int(t)}" for t in rng.integers(2, V, int(rng.integers(3, 9)))) for _ in range(2)] for _ in range(10)]
    return words, pred, refs, bank_caps, rng


def test_references_and_bank_select_agree_with_select_captions_and_subset_summary():
    words, pred, refs, bank_caps, rng = toy_corpus()
    P, N, _ = pred.shape
    pt = torch.from_numpy(pred).cuda()
    qids = list(refs)
    cr = CaptionReferences(refs)
    full = cr.score(pt, 1, words, image_ids=qids, set_diversity=True)
    quality = torch.from_numpy(rng.normal(size=(P, N))).cuda()
    empty = pt[:, :, 0] == 1
    assert empty[:, 5].all()
    for method, kw in (("dpp", dict(theta=0.7)), ("mmr", dict(lam=0.6)), ("mbr", {})):
        got = cr.select(pt, 1, words, image_ids=qids, quality=quality, k=5, method=method, **kw)
        want = E.select_captions(torch.from_numpy(full.set_kernel).cuda(), quality, k=5, method=method, eligible=~empty, **kw)
        assert np.array_equal(got.picks, want.picks) and np.array_equal(got.gains, want.gains)
        assert np.array_equal(got.n_primary, want.n_primary) and got.method == method and got.k == 5
        assert not (got.picks == 5).any() and (got.picks >= 0).all()        # the empty caption is never picked
    # quality by name
    cons = E.ConsensusResult(quality.cpu().numpy(), None, None, None, None)
    a = cr.select(pt, 1, words, image_ids=qids, quality="consensus", consensus=cons, k=4)
    b = cr.select(pt, 1, words, image_ids=qids, quality="logprob", logprob=quality, k=4)
    c = cr.select(pt, 1, words, image_ids=qids, quality=quality, k=4)
    assert np.array_equal(a.picks, c.picks) and np.array_equal(b.picks, c.picks) and np.array_equal(a.gains, b.gains)
    with pytest.raises(ValueError, match="needs consensus"):
        cr.select(pt, 1, words, image_ids=qids, quality="consensus", k=4)
    with pytest.raises(ValueError, match="needs logprob"):
        cr.select(pt, 1, words, image_ids=qids, quality="logprob", k=4)
    # the bank: its own document frequencies
    bank = ConsensusBank(torch.randn(10, 16), list(range(10)), bank_caps)
    id_map = torch.tensor([bank.references.word_id.get(w, 0) for w in words], dtype=torch.int32, device="cuda")
    id_map[0] = 0
    Kb = E._eval_set_call(pt, 1, len(words), bank.prep, id_map, torch.zeros(P, dtype=torch.int32, device="cuda"))[2]
    assert not torch.equal(Kb, torch.from_numpy(full.set_kernel).cuda())
    for method in ("dpp", "mmr", "mbr"):
        got = bank.select(pt, 1, words, quality=quality, k=5, method=method)
        want = E.select_captions(Kb, quality, k=5, method=method, eligible=~empty)
        assert np.array_equal(got.picks, want.picks) and np.array_equal(got.gains, want.gains)
    # DPP never returns a duplicate while distinct captions are left (5 distinct non-empty captions per image, k = 5)
    sel = bank.select(pt, 1, words, quality=quality, k=5, method="dpp")
    for p in range(P):
        assert len(set(tuple(pred[p, n]) for n in sel.picks[p])) == 5 and sel.n_primary[p] == 5
    # subset_summary = the existing summaries of the gathered predictions
    gathered = sel.gather(pt, 1)
    assert tuple(gathered.shape) == (P, 5, pred.shape[2])
    for p in range(P):
        assert torch.equal(gathered[p], pt[p, torch.from_numpy(sel.picks[p]).cuda()])
    sub = cr.score(gathered, 1, words, image_ids=qids, set_diversity=True).summary()
    got = full.subset_summary(sel, "select")
    want = {"select subset Div-1": sub["Div-1"], "select subset Div-2": sub["Div-2"], "select subset distinct": 5.0,
            "select subset unique": sub["unique"], "select subset mBLEU-1": sub["mBLEU-1"], "select subset mBLEU-2": sub["mBLEU-2"],
            "select subset mBLEU-3": sub["mBLEU-3"], "select subset mBLEU-4": sub["mBLEU-4"], "select subset self-cider": sub["self-cider"],
            "select subset oracle cider": sub["cider"], "select subset mean cider": sub["mean cider"],
            "select subset oracle B4": sub["B4"], "select subset mean B4": sub["mean B4"]}
    assert got == want
    assert sub["cider"] <= full.summary()["cider"] + 1e-15            # an oracle over a subset cannot beat the oracle over all
    lines = E.format_summary({**full.summary(), **got})
    assert [x.split(":")[0] for x in lines if " subset " in x] == list(want)
    # a selection with k = 1 has no set numbers
    one = full.subset_summary(bank.select(pt, 1, words, quality=quality, k=1, method="mmr"), "best")
    assert sorted(one) == sorted(f"best subset {n}" for n in ("Div-1", "Div-2", "oracle cider", "mean cider", "oracle B4", "mean B4"))
    assert one["best subset oracle cider"] == one["best subset mean cider"]


# ---- scripts ---------------------------------------------------------------------------------------------------------------------

YAML = """
RANDOM_SEED: 3
DATA:
  MAX_CAPTION_LENGTH: 8
  CBS:
    MAX_GIVEN_CONSTRAINTS: 0
MODEL:
  IMAGE_FEATURE_SIZE: 64
  EMBEDDING_SIZE: 40
  HIDDEN_SIZE: 48
  ATTENTION_PROJECTION_SIZE: 32
  BEAM_SIZE: 2
  USE_CBS: False
  MIN_CONSTRAINTS_TO_SATISFY: 0
  Z_SPACE: 16
  SENTIMENT_VAE: 1
  SENTI_PRIOR_MULTIP: 0.5
  SIMPLE_VAE: False
  N_Z_SAMPLES: 6
"""


def _run(args, ok=True):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def test_scripts_write_select_output_that_round_trips(tmp_path):
    from ssc_runtime.data import SyntheticCaptionData
    from ssc_runtime.vocab import Vocabulary
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    V, R_, F = 40, 5, 64
    syn = SyntheticCaptionData(6, R_, F, 8, V, seed=4321)
    g = torch.Generator().manual_seed(1)
    pooled = torch.cat([syn.feats.mean(1), torch.randn(14, F, generator=g)])
    bcaps = [[" ".join(f"w{int(t)}" for t in torch.randint(2, V, (6,), generator=g)) for _ in range(2)] for _ in range(20)]
    bank_path = tmp_path / "bank.pt"
    ConsensusBank.write_file(str(bank_path), pooled, list(range(20)), bcaps)
    refs = {str(i): [" ".join(f"w{int(t)}" for t in torch.randint(2, V, (5,), generator=g)) for _ in range(3)] for i in range(5)}
    rp = tmp_path / "refs.json"
    rp.write_text(json.dumps(refs))
    out, picked = tmp_path / "pred.json", tmp_path / "picked.json"
    inf = [os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "6", "--vocab-size", str(V),
           "--num-boxes", str(R_), "--images-per-call", "4", "--references", str(rp)]
    o1 = _run(inf + ["--output-path", str(out), "--consensus-bank", str(bank_path), "--consensus-k", "5", "--select-k", "3", "--select-method", "dpp",
                     "--select-theta", "0.5", "--select-output", str(picked)])
    groups = E.load_predictions(str(out))
    sel = E.load_predictions(str(picked))                       # the prediction-file format
    assert list(sel) == list(groups) == list(range(6))
    for iid, caps in sel.items():
        assert 1 <= len(caps) <= 3 and all(c in groups[iid] and c for c in caps)
    lines1 = [x for x in o1.splitlines() if x.startswith("select subset")]
    names = [x.split(":")[0] for x in lines1]
    assert names[:2] == ["select subset Div-1", "select subset Div-2"] and "select subset oracle cider" in names
    assert "select subset mBLEU-4" in names and "wrote" in o1 and "selected captions (dpp, k = 3)" in o1
    # log-prob quality needs no bank: the kernel's document frequencies are the references'
    # (its own predictions file: scoring the captions draws from the run's random stream, so the later chunks decode differently)
    picked_lp = tmp_path / "picked_lp.json"
    inf += ["--output-path", str(tmp_path / "pred_lp.json")]
    o2 = _run(inf + ["--select-k", "2", "--select-method", "mmr", "--select-quality", "logprob", "--select-lambda", "0.7",
                     "--select-output", str(picked_lp)])
    sel_lp, groups_lp = E.load_predictions(str(picked_lp)), E.load_predictions(str(tmp_path / "pred_lp.json"))
    assert list(sel_lp) == list(range(6)) and all(1 <= len(c) <= 2 and all(x in groups_lp[i] for x in c) for i, c in sel_lp.items())
    assert any(x.startswith("select subset mean cider") for x in o2.splitlines())
    o3 = _run(inf + ["--select-k", "2", "--select-output", str(picked_lp)], ok=False)
    assert "--select-quality consensus needs --consensus-bank" in o3
    # evaluate.py: the same selection from the JSON, features from a query tensor file
    qt = tmp_path / "query.pt"
    torch.save({"caption_tokens": torch.zeros(6, 1, dtype=torch.long), "image_id": torch.arange(6), "image_features": syn.feats}, str(qt))
    picked2, summ = tmp_path / "picked2.json", tmp_path / "summary.json"
    ev = [os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp), "--gpu-ids", "0"]
    o5 = _run(ev + ["--consensus-bank", str(bank_path), "--query-tensors", str(qt), "--consensus-k", "5", "--select-k", "3",
                    "--select-method", "dpp", "--select-theta", "0.5", "--select-output", str(picked2), "--output-json", str(summ)])
    assert E.load_predictions(str(picked2)) == sel
    assert [x for x in o5.splitlines() if x.startswith("select subset")] == lines1
    assert "select subset oracle cider" in json.load(open(summ))
    o6 = _run(ev + ["--select-k", "3"], ok=False)
    assert "needs --consensus-bank" in o6
