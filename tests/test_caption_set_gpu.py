"""GPU: ssc_eval_set (csrc/caption_eval.hip: es_caption, es_pair, es_eigen) through ssc_runtime.evaluation against the float64
restatement tests/captionsetref.py: random corpora (small vocabularies with repeats, duplicate and empty captions, @@UNKNOWN@@,
reference words outside the vocabulary, images without references, one evaluated image, N = 128, 64-token captions), a full-scale
corpus, bit-level symmetry / duplicate rows / determinism, set_diversity=False left exactly as it was, SSC_EINVAL on bad inputs and
both scripts with --set-diversity.

Bounds: set statistics and distinct counts are integers and must be equal; K within relative 1e-12 (exact zeros
within 1e-15); eigenvalues within 2 N 1e-12 absolute (Weyl: |d lambda| <= ||dK||_F <= N 1e-12 max|K|, |K| <= 1, doubled for the
two eigen-solvers' own errors); a Self-CIDEr value within N (2 N 1e-12) / (2 sqrt(1e-6) lambda_1) - the eigenvalue bound carried
through d sqrt(l) = d l / (2 sqrt(l)) for the at most N kept eigenvalues l >= 1e-6 lambda_1, relative to sum sqrt(l) >= sqrt(lambda_1).
An image is left out of the Self-CIDEr comparison only when the RESTATEMENT finds an eigenvalue within a factor 10 of the cut-off
(the two sides may then keep different eigenvalues); at most 2 % of a test's images may be, which every test asserts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import captionsetref as S
from ssc_runtime import evaluation as E
from ssc_runtime import lib as L
from ssc_runtime.evaluation import CaptionReferences

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK_TOK = ("@@UNKNOWN@@",)   # a candidate token no reference holds, equal only to itself


def make_corpus(seed, I, N, V, max_refs=7, max_len=64, ref_len=(1, 20), small=None, unscored=2, long_share=0.2):
    """Vocabulary ['@@UNKNOWN@@', '@@BOUNDARY@@', 'w2', ...]; references for the first I of I + unscored prediction images;
    predictions (I + unscored, N, max_len + 1) with boundary 1 after each caption (a full-length caption has none)."""
    rng = np.random.default_rng(seed)
    words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
    pool = small or V
    refs = {}
    for i in range(I):
        rs = []
        for _ in range(int(rng.integers(1, max_refs + 1))):
            n = int(rng.integers(ref_len[0], ref_len[1] + 1))
            toks = [f"w{int(t)}" for t in rng.integers(2, pool, n)]
            if rng.random() < 0.3:
                toks[int(rng.integers(0, n))] = f"oov{int(rng.integers(0, 3))}"   # a reference word outside the vocabulary
            rs.append(" ".join(toks))
        refs[100 + i] = rs
    P = I + unscored
    pred = np.ones((P, N, max_len + 1), dtype=np.int64)
    for i in range(P):
        for n in range(N):
            if n % 4 == 3:
                pred[i, n] = pred[i, n - 1 - int(rng.integers(0, 3))]   # duplicate of an earlier caption
                continue
            L_ = int(rng.choice([0, 1, int(rng.integers(2, 12)), int(rng.integers(2, max_len + 1)), max_len],
                                p=[0.1, 0.1, 0.6 - long_share, 0.2, long_share]))
            ids = rng.integers(2, pool, L_)
            ids[rng.random(L_) < 0.05] = 0                        # @@UNKNOWN@@
            pred[i, n, :L_] = ids
    pred = pred[:, :, :max_len] if long_share >= 0.5 else pred    # rows with no boundary at all
    return words, refs, pred, list(refs) + [900 + k for k in range(unscored)]


def captions(words, pred, unk_as_word=False):
    out = []
    for img in pred:
        caps = []
        for row in img:
            row = list(row)
            cut = row.index(1) if 1 in row else len(row)
            caps.append([(words[0] if unk_as_word else UNK_TOK) if t == 0 else words[t] for t in row[:cut]])
        out.append(caps)
    return out


def restate(words, refs, pred, image_ids):
    scored = [p for p, i in enumerate(image_ids) if i in refs]
    return S.evaluate(captions(words, pred), [[r.split() for r in refs[image_ids[p]]] for p in scored], scored=scored)


def close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = np.where(b == 0, np.abs(a) <= 1e-15, np.abs(a - b) <= 1e-12 * np.abs(b))
    assert ok.all(), (a[~ok][:5], b[~ok][:5])


def check(res, per, s, image_ids, refs):
    P, N = res.set_stats.shape[:2]
    assert np.array_equal(res.set_stats, per["set_stats"])
    assert np.array_equal(res.distinct, per["distinct"])
    scored = [p for p, i in enumerate(image_ids) if i in refs]
    bounds, left_out = [], 0
    for at, p in enumerate(scored):
        close(res.set_kernel[p], per["kernel"][p])
        lam = per["eigenvalues"][p]
        err = np.abs(res.set_eigenvalues[p] - lam).max()
        print(f"image {p}: N {N} lambda_1 {lam[0]:.6g} eigenvalue error {err:.3g} (bound {2 * N * 1e-12:.3g})")
        assert err <= 2 * N * 1e-12
        if lam[0] <= 0:
            assert res.self_cider_values[at] == 0.0
            bounds.append(0.0)
            continue
        if S.near_cut(lam):
            left_out += 1
            continue
        bound = N * (2 * N * 1e-12) / (2 * np.sqrt(1e-6) * lam[0])
        d = abs(res.self_cider_values[at] - per["self_cider"][p])
        print(f"image {p}: self-cider {per['self_cider'][p]:.12g} error {d:.3g} (bound {bound:.3g})")
        assert d <= bound
        bounds.append(bound)
    for p in range(P):
        if p not in scored:
            assert not res.set_eigenvalues[p].any() and not res.set_kernel[p].any()
    assert left_out <= 0.02 * P, f"{left_out} of {P} images have an eigenvalue near the cut-off"
    assert res.degenerate_sets == per["degenerate"]
    got = res.summary()
    for k in ("mBLEU-1", "mBLEU-2", "mBLEU-3", "mBLEU-4", "unique"):
        assert got[k] == pytest.approx(s[k], rel=1e-10, abs=1e-15), k
    if left_out == 0:
        assert abs(got["self-cider"] - s["self-cider"]) <= float(np.mean(bounds)) + 1e-15
    return got


CASES = [dict(seed=1, I=9, N=8, V=40, small=8), dict(seed=2, I=12, N=6, V=300), dict(seed=3, I=1, N=5, V=30, small=6),
         dict(seed=4, I=20, N=11, V=60, small=12), dict(seed=5, I=3, N=128, V=50, small=10, unscored=1),
         dict(seed=6, I=6, N=7, V=80, small=16, long_share=0.5)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"seed{c['seed']}-N{c['N']}")
def test_random_corpora_against_restatement(case):
    words, refs, pred, ids = make_corpus(**case)
    cr = CaptionReferences(refs)
    pt = torch.from_numpy(pred).cuda()
    res = cr.score(pt, 1, words, image_ids=ids, set_diversity=True)
    per, s = restate(words, refs, pred, ids)
    check(res, per, s, ids, refs)
    # without references: the same statistics and distinct counts
    only = E.set_diversity(pt, 1, len(words))
    assert np.array_equal(only.set_stats, res.set_stats) and np.array_equal(only.distinct, res.distinct)
    assert only.set_kernel is None and "self-cider" not in only.summary()
    assert only.summary()["mBLEU-4"] == res.summary()["mBLEU-4"] and only.summary()["unique"] == res.summary()["unique"]
    # strings: the same captions as text give the same set numbers (other ids, the same words)
    caps = {iid: [" ".join(c) for c in img] for iid, img in zip(ids, captions(words, pred, unk_as_word=True))}
    res2 = cr.score_captions(caps, set_diversity=True)
    assert np.array_equal(res2.set_stats, res.set_stats) and np.array_equal(res2.distinct, res.distinct)
    assert res2.summary()["self-cider"] == pytest.approx(res.summary()["self-cider"], rel=1e-10, abs=1e-13)


def test_full_scale_against_restatement():
    rng = np.random.default_rng(5)
    I, N, V = 1000, 20, 10000
    words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
    zipf = np.minimum(rng.zipf(1.3, size=(I * 5 * 20 + I * N * 20)), V - 3) + 1   # frequent words repeat, as in captions
    it = iter(zipf)
    refs = {i: [" ".join(f"w{next(it)}" for _ in range(int(rng.integers(6, 17)))) for _ in range(5)] for i in range(I)}
    pred = np.ones((I, N, 20), dtype=np.int64)
    for i in range(I):
        for n in range(N):
            L_ = int(rng.integers(5, 21))   # up to the full 20 tokens: such a row holds no boundary
            pred[i, n, :L_] = [next(it) for _ in range(L_)]
    cr = CaptionReferences(refs)
    res = cr.score(torch.from_numpy(pred).cuda(), 1, words, set_diversity=True)
    per, s = restate(words, refs, pred, list(refs))
    got = check(res, per, s, list(refs), refs)
    print({k: got[k] for k in ("mBLEU-1", "mBLEU-4", "self-cider", "unique")})


def test_bitwise_symmetry_duplicates_determinism_and_untouched_scores():
    words, refs, pred, ids = make_corpus(11, 30, 10, 80, small=15)
    cr = CaptionReferences(refs, style_words={"w2", "w4"})
    pt = torch.from_numpy(pred).cuda()
    before = cr.score(pt, 1, words, image_ids=ids)
    a = cr.score(pt, 1, words, image_ids=ids, set_diversity=True)
    b = CaptionReferences(refs, style_words={"w2", "w4"}).score(pt, 1, words, image_ids=ids, set_diversity=True)
    after = cr.score(pt, 1, words, image_ids=ids)
    for x, y in ((a.set_stats, b.set_stats), (a.set_kernel, b.set_kernel), (a.set_eigenvalues, b.set_eigenvalues),
                 (a.distinct, b.distinct)):
        assert x.tobytes() == y.tobytes()
    K = a.set_kernel
    assert K.tobytes() == np.ascontiguousarray(K.transpose(0, 2, 1)).tobytes()
    dups = 0
    for p in range(pred.shape[0]):
        for i in range(pred.shape[1]):
            for j in range(i):
                if np.array_equal(pred[p, i], pred[p, j]):
                    assert K[p, i].tobytes() == K[p, j].tobytes() and a.set_stats[p, i].tobytes() == a.set_stats[p, j].tobytes()
                    dups += 1
    assert dups >= pred.shape[0]
    # set_diversity=False: exactly what it was, and no set fields
    assert before.set_stats is None and "mBLEU-1" not in before.summary() and "unique" not in before.summary()
    for r in (a, after):
        for x, y in ((before.bleu, r.bleu), (before.rouge, r.rouge), (before.cider, r.cider), (before.stats, r.stats),
                     (before.div_counts, r.div_counts), (before.top5, r.top5), (before.style_counts, r.style_counts)):
            assert x.tobytes() == y.tobytes()
    assert list(before.summary()) == list(after.summary()) == list(a.summary())[:len(before.summary())]


def test_bad_ids_and_lengths_return_einval():
    ok = torch.ones(2, 5, 4, dtype=torch.int64, device="cuda")
    ok[:, :, 0] = 2
    ok[1, 3, 1] = 3
    for bad in (7, -3):   # ids outside 0..V-1
        p = ok.clone()
        p[1, 2, 1] = bad
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            E.set_diversity(p, 1, 6)
    long = torch.full((2, 5, 70), 3, dtype=torch.int64, device="cuda")   # 70 tokens, no boundary
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        E.set_diversity(long, 1, 6)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):   # an image asks for references the call does not have
        E._eval_set(ok, 1, 6, None, None, torch.tensor([-1, 0], dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="captions per image"):
        E.set_diversity(ok[:, :1], 1, 6)
    res = E.set_diversity(ok, 1, 6)   # the library is still fine
    assert np.all(res.set_stats[:, :, 0] == [[1] * 5, [1, 1, 1, 2, 1]]) and list(res.distinct) == [1, 2]
    assert res.summary()["unique"] == pytest.approx(0.3)


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


def _run(args):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_scripts_print_the_same_set_lines_and_json_holds_the_restatement(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    rng = np.random.default_rng(9)
    # the synthetic data's image ids are 0..n-1; image 5 has no references (mBLEU / unique only)
    refs = {str(i): [" ".join(f"w{int(t)}" for t in rng.integers(2, 40, int(rng.integers(3, 9)))) for _ in range(3)]
            for i in range(5)}
    rp = tmp_path / "refs.json"
    rp.write_text(json.dumps(refs))
    out = tmp_path / "pred.json"
    o1 = _run([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "6",
               "--vocab-size", "40", "--num-boxes", "5", "--output-path", str(out), "--images-per-call", "4",
               "--references", str(rp), "--set-diversity"])
    summ = tmp_path / "summary.json"
    o2 = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp),
               "--gpu-ids", "0", "--output-json", str(summ), "--set-diversity"])
    lines1 = [x for x in o1.splitlines() if ":" in x and not x.startswith("wrote")]
    lines2 = [x for x in o2.splitlines() if ":" in x and not x.startswith(("input", "Total"))]
    assert lines1 == lines2
    tail = [x.split(":")[0] for x in lines1 if x.startswith(("mBLEU", "self-cider", "unique"))]
    assert tail == ["mBLEU-1", "mBLEU-2", "mBLEU-3", "mBLEU-4", "self-cider", "unique"]
    # without the flag neither script prints them
    o3 = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp), "--gpu-ids", "0"])
    assert not any(x.startswith(("mBLEU", "self-cider", "unique")) for x in o3.splitlines())
    groups = {}
    for e in json.load(open(out)):
        groups.setdefault(e["image_id"], []).append(e["caption"].split())
    from ssc_runtime.vocab_builder import caption_words
    scored = [p for p, i in enumerate(groups) if str(i) in refs]
    imgs = list(groups.values())
    ids = list(groups)
    per, s = S.evaluate(imgs, [[caption_words(c) for c in refs[str(ids[p])]] for p in scored], scored=scored)
    got = json.load(open(summ))
    for k in ("mBLEU-1", "mBLEU-2", "mBLEU-3", "mBLEU-4", "unique"):
        assert got[k] == pytest.approx(s[k], rel=1e-10, abs=1e-15), k
    N = len(imgs[0])
    assert not any(S.near_cut(per["eigenvalues"][p]) for p in scored)
    bound = np.mean([N * (2 * N * 1e-12) / (2 * np.sqrt(1e-6) * per["eigenvalues"][p][0]) if per["eigenvalues"][p][0] > 0 else 0.0
                     for p in scored])
    assert abs(got["self-cider"] - s["self-cider"]) <= bound + 1e-15
