"""GPU: ssc_eval_prepare_refs / ssc_eval_score (csrc/caption_eval.hip) through ssc_runtime.evaluation against the float64
restatement tests/captionevalref.py: random corpora (small vocabularies with repeats, ties and duplicate captions, 1-7 references,
candidate lengths 0..64, reference words outside the vocabulary, @@UNKNOWN@@ in candidates, one image), the g20 inputs, duplicate
captions, determinism, a full-scale corpus, the decode path through scripts/inference.py --references and scripts/evaluate.py, and
SSC_EINVAL on bad inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import captionevalref as R
from ssc_runtime import lib as L
from ssc_runtime.evaluation import CaptionReferences

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
UNK_TOK = ("@@UNKNOWN@@",)   # a candidate token no reference holds, equal only to itself


def make_corpus(seed, I, N, V, max_refs=7, max_len=64, ref_len=(1, 20), oov=True, small=None):
    """Vocabulary ['@@UNKNOWN@@', '@@BOUNDARY@@', 'w2', ...]; predictions (I, N, steps) with boundary 1 after each caption."""
    rng = np.random.default_rng(seed)
    words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
    pool = small or V
    refs = {}
    for i in range(I):
        rs = []
        for _ in range(int(rng.integers(1, max_refs + 1))):
            n = int(rng.integers(ref_len[0], ref_len[1] + 1))
            toks = [f"w{int(t)}" for t in rng.integers(2, pool, n)]
            if oov and rng.random() < 0.3:
                toks[int(rng.integers(0, n))] = f"oov{int(rng.integers(0, 3))}"   # a reference word outside the vocabulary
            rs.append(" ".join(toks))
        refs[100 + i] = rs
    steps = max_len + 1
    pred = np.ones((I, N, steps), dtype=np.int64)
    for i in range(I):
        for n in range(N):
            if n % 4 == 3 and n > 0:
                pred[i, n] = pred[i, n - 1]                       # duplicate caption
                continue
            L_ = int(rng.choice([0, 1, int(rng.integers(2, 12)), int(rng.integers(2, max_len + 1))], p=[0.1, 0.1, 0.6, 0.2]))
            ids = rng.integers(2, pool, L_)
            ids[rng.random(L_) < 0.05] = 0                        # @@UNKNOWN@@
            pred[i, n, :L_] = ids
    return words, refs, pred


def restate(words, refs, pred, image_ids, style=None):
    cands = []
    for i in range(pred.shape[0]):
        caps = []
        for n in range(pred.shape[1]):
            row = list(pred[i, n])
            cut = row.index(1) if 1 in row else len(row)
            caps.append([UNK_TOK if t == 0 else words[t] for t in row[:cut]])
        cands.append(caps)
    tr = [[r.split() for r in refs[i]] for i in image_ids]
    return R.evaluate(cands, tr, style_words=style)


def check(res, per, s, margin=1e-9):
    def close(a, b):
        a, b = np.asarray(a), np.asarray(b)
        ok = np.where(b == 0, np.abs(a) <= 1e-15, np.abs(a - b) <= 1e-12 * np.abs(b))
        assert ok.all(), (a[~ok][:5], b[~ok][:5])
    close(res.bleu, per["bleu"])
    close(res.rouge, per["rouge"])
    close(res.cider, per["cider"])
    assert np.array_equal(res.stats, per["stats"])
    for key, vals in (("B1", per["bleu"][:, :, 0]), ("B2", per["bleu"][:, :, 1]), ("B3", per["bleu"][:, :, 2]),
                      ("B4", per["bleu"][:, :, 3]), ("rouge", per["rouge"]), ("cider", per["cider"])):
        srt = np.sort(vals, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > margin
        assert np.array_equal(res.oracle[key][clear], per["oracle"][key][clear]), key
    c = per["cider"]
    for i in range(c.shape[0]):   # top-5 sets (equal where the 5th / 6th CIDEr values are apart)
        srt = np.sort(c[i])[::-1]
        if len(srt) == 5 or srt[4] - srt[5] > margin:
            assert set(res.top5[i]) == set(per["top5"][i])
    got = res.summary()
    for k, v in s.items():
        if isinstance(v, float) and np.isnan(v):
            assert np.isnan(got[k]), k
        else:
            assert got[k] == pytest.approx(v, rel=1e-10, abs=1e-15), k


@pytest.mark.parametrize("seed,I,N,V,small", [(1, 9, 8, 40, 8), (2, 12, 6, 300, None), (3, 1, 5, 30, 6), (4, 20, 11, 60, 12)])
def test_random_corpora_against_restatement(seed, I, N, V, small):
    words, refs, pred = make_corpus(seed, I, N, V, small=small)
    style = {"w2", "w3", "w5", "oov1"}
    cr = CaptionReferences(refs, style_words=style)
    ids = list(refs)
    res = cr.score(torch.from_numpy(pred).cuda(), 1, words)
    per, s = restate(words, refs, pred, ids, style)
    check(res, per, s)
    # strings: the same captions as text score the same
    caps = {iid: [" ".join("@@UNKNOWN@@" if t == 0 else words[t] for t in row[: list(row).index(1) if 1 in row else len(row)])
                  for row in pred[i]] for i, iid in enumerate(ids)}
    res2 = cr.score_captions(caps)
    assert np.array_equal(res2.cider, res.cider) and np.array_equal(res2.stats, res.stats)


def test_prediction_images_without_references_count_toward_div_only():
    words, refs, pred = make_corpus(7, 6, 5, 50, small=10)
    ids = list(refs)
    cr = CaptionReferences({k: refs[k] for k in ids[:4]})
    res = cr.score(torch.from_numpy(pred).cuda(), 1, words, image_ids=ids)
    cands_rest = [[[UNK_TOK if t == 0 else words[t] for t in row[: list(row).index(1) if 1 in row else len(row)]] for row in img]
                  for img in pred[4:]]
    per, s = R.evaluate([[[UNK_TOK if t == 0 else words[t] for t in row[: list(row).index(1) if 1 in row else len(row)]]
                          for row in img] for img in pred[:4]], [[r.split() for r in refs[k]] for k in ids[:4]],
                        div_only=cands_rest)
    check(res, per, s)
    assert res.image_ids == ids[:4]


def test_g20_inputs():
    g = np.load(os.path.join(HERE, "golden", "g20_caption_eval.npz"))
    words = [str(w) for w in g["words"]]
    cand = g["cand_ids"]
    I, N, Lc = cand.shape
    toks, lens, counts = g["ref_tokens"], g["ref_lengths"], g["ref_counts"]
    refs, at, r = {}, 0, 0
    for i in range(I):
        refs[i] = []
        for _ in range(counts[i]):
            refs[i].append(" ".join(words[t] for t in toks[at: at + lens[r]]))
            at += lens[r]
            r += 1
    vocab = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + words
    pred = np.where(cand >= 0, cand + 2, 1).astype(np.int64)
    cr = CaptionReferences(refs, style_words=set(str(w) for w in g["style_words"]))
    res = cr.score(torch.from_numpy(pred).cuda(), 1, vocab)
    s = res.summary()
    assert [s["Div-1"], s["Div-2"], s["top5 Div-1"], s["top5 Div-2"]] == pytest.approx(list(g["div"]), rel=1e-13)
    assert [s["senti_prec"], s["senti_rec"], s["has_anp"]] == pytest.approx(list(g["style"]), rel=1e-15)
    assert np.array_equal(res.top5, g["top5"])


def test_duplicate_captions_score_bit_equal_and_lowest_index_wins():
    refs = {1: ["a dog runs on the grass", "the dog is running"], 2: ["a cat sleeps", "a cat on a bed"]}
    cr = CaptionReferences(refs)
    vocab = ["@@UNKNOWN@@", "@@BOUNDARY@@", "a", "dog", "runs", "on", "the", "grass", "cat", "sleeps", "bed"]
    w = {x: i for i, x in enumerate(vocab)}
    caps = [["a dog runs"] * 3 + ["the dog"] * 3, ["a cat on the bed"] * 6]
    pred = np.ones((2, 6, 8), dtype=np.int64)
    for i in range(2):
        for n in range(6):
            t = [w[x] for x in caps[i][n].split()]
            pred[i, n, :len(t)] = t
    res = cr.score(torch.from_numpy(pred).cuda(), 1, vocab)
    for a, b in ((0, 1), (0, 2), (3, 4), (3, 5)):
        assert res.cider[0, a].tobytes() == res.cider[0, b].tobytes()
        assert res.bleu[0, a].tobytes() == res.bleu[0, b].tobytes()
    assert len(set(res.cider[1].tobytes()[k: k + 8] for k in range(0, 48, 8))) == 1
    assert res.oracle["cider"][1] == 0 and list(res.top5[1]) == [0, 1, 2, 3, 4]
    best = 0 if res.cider[0, 0] >= res.cider[0, 3] else 3
    assert res.oracle["cider"][0] == best


def test_two_calls_are_bit_identical():
    words, refs, pred = make_corpus(11, 30, 10, 80, small=15)
    cr = CaptionReferences(refs, style_words={"w2", "w4"})
    p = torch.from_numpy(pred).cuda()
    a = cr.score(p, 1, words)
    cr2 = CaptionReferences(refs, style_words={"w2", "w4"})   # a second preparation as well
    b = cr2.score(p, 1, words)
    for x, y in ((a.bleu, b.bleu), (a.rouge, b.rouge), (a.cider, b.cider), (a.stats, b.stats), (a.top5, b.top5),
                 (a.div_counts, b.div_counts), (a.style_counts, b.style_counts)):
        assert x.tobytes() == y.tobytes()


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
            L_ = int(rng.integers(5, 17))
            pred[i, n, :L_] = [next(it) for _ in range(L_)]
    cr = CaptionReferences(refs)
    res = cr.score(torch.from_numpy(pred).cuda(), 1, words)
    per, s = restate(words, refs, pred, list(refs))
    check(res, per, s)


def test_bad_ids_and_lengths_return_einval():
    refs = {1: ["a b c"], 2: ["b c d"]}
    cr = CaptionReferences(refs)
    vocab = ["@@UNKNOWN@@", "@@BOUNDARY@@", "a", "b", "c", "d"]
    ok = torch.ones(2, 5, 4, dtype=torch.int64, device="cuda")
    ok[:, :, 0] = 2
    for bad in (7, -3):   # ids outside 0..V-1
        p = ok.clone()
        p[1, 2, 1] = bad
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            cr.score(p, 1, vocab)
    long = torch.full((2, 5, 70), 3, dtype=torch.int64, device="cuda")   # 70 tokens, no boundary
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        cr.score(long, 1, vocab)
    res = cr.score(ok, 1, vocab)   # the library is still fine
    assert np.all(res.stats[:, :, 0] == 1)


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


def test_decode_path_script_and_json_agree(tmp_path):
    """scripts/inference.py --synthetic --references scores the device tensor of the decode; scripts/evaluate.py on the JSON it
    wrote prints the same lines, and they are the restatement's."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    rng = np.random.default_rng(9)
    # the synthetic data's image ids are 0..n-1; image 5 has no references (Div-n only)
    refs = {str(i): [" ".join(f"w{int(t)}" for t in rng.integers(2, 40, int(rng.integers(3, 9)))) for _ in range(3)]
            for i in range(5)}
    refs["0"].append("W3 w4, oov_word.")
    rp = tmp_path / "refs.json"
    rp.write_text(json.dumps(refs))
    tsv = tmp_path / "forms.tsv"
    tsv.write_text("a\tw3,w7\nb\tw11,w20\n")
    out = tmp_path / "pred.json"
    o1 = _run([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "6",
               "--vocab-size", "40", "--num-boxes", "5", "--output-path", str(out), "--images-per-call", "4",
               "--references", str(rp), "--style-wordforms", str(tsv)])
    summ = tmp_path / "summary.json"
    top = tmp_path / "top5.json"
    o2 = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp),
               "--style-wordforms", str(tsv), "--gpu-ids", "0", "--output-json", str(summ), "--top5-output", str(top)])
    lines1 = [x for x in o1.splitlines() if ":" in x and not x.startswith("wrote")]
    lines2 = [x for x in o2.splitlines() if ":" in x and not x.startswith(("input", "Total"))]
    assert lines1 == lines2 and any(x.startswith("mean cider:") for x in lines1)
    preds = json.load(open(out))
    groups = {}
    for e in preds:
        groups.setdefault(e["image_id"], []).append(e["caption"].split())
    ids = [i for i in groups if str(i) in refs]
    from ssc_runtime.vocab_builder import caption_words
    per, s = R.evaluate([groups[i] for i in ids], [[caption_words(c) for c in refs[str(i)]] for i in ids],
                        style_words={"w3", "w7", "w11", "w20"}, div_only=[groups[i] for i in groups if str(i) not in refs])
    got = json.load(open(summ))
    for k, v in s.items():
        if isinstance(v, float) and np.isnan(v):
            assert np.isnan(got[k]), k
        else:
            assert got[k] == pytest.approx(v, rel=1e-10, abs=1e-15), k
    assert len(json.load(open(top))) == 5 * len(ids)
