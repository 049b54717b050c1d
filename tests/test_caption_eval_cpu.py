"""CPU: the float64 restatement of the caption metrics (tests/captionevalref.py) against the worked example of the definitions,
property cases and the g20 fixture made from the reference's own eval.py functions; parsing of prediction / reference files;
argument validation of the ssc_eval_* entry points without a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import captionevalref as R
from ssc_runtime import lib as L
from ssc_runtime import evaluation as E

HERE = os.path.dirname(os.path.abspath(__file__))

REFS = [["a man riding a horse", "a person on a horse"], ["two dogs play in the grass"],
        ["a red bus on the street", "a bus parked on a street"]]
CANDS = ["a man on a horse", "two dogs in grass", "a bus"]


def test_worked_example():
    refs = [[r.split() for r in rs] for rs in REFS]
    cid = R.Cider(refs)
    got = [cid.score(c.split(), refs[i]) for i, c in enumerate(CANDS)]
    assert got == pytest.approx([3.390993428619308, 2.697607376530157, 1.6927870669162917], rel=1e-14)
    b0 = R.bleu_from_stats(*R.bleu_stats(CANDS[0].split(), refs[0]))
    assert b0 == pytest.approx([0.9999999996000004, 0.8660254034163782, 0.6299605246569553, 0.00010573712628898506], rel=1e-13)
    assert R.rouge_l(CANDS[0].split(), refs[0]) == pytest.approx(0.8, rel=1e-15)
    assert R.rouge_l(CANDS[1].split(), refs[1]) == pytest.approx(0.7721518987341772, rel=1e-15)
    assert R.bleu_from_stats(*R.bleu_stats(CANDS[2].split(), refs[2]))[0] == pytest.approx(0.13533528310127763, rel=1e-13)
    assert R.rouge_l(CANDS[2].split(), refs[2]) == pytest.approx(0.45864661654135336, rel=1e-15)


def test_property_cases():
    refs = [["a cat on a mat".split()]]
    # one image: log I = 0, every weight 0, every CIDEr-D 0
    assert R.Cider(refs).score("a cat".split(), refs[0]) == 0.0
    assert R.Cider(refs).score("a cat on a mat".split(), refs[0]) == 0.0
    # a candidate equal to its only reference: ROUGE-L 1
    assert R.rouge_l("a cat on a mat".split(), refs[0]) == pytest.approx(1.0, rel=1e-15)
    # closest-length ties go to the shorter reference
    assert R.bleu_stats("a b c d".split(), ["x y z".split(), "x y z w v".split()])[1] == 3
    assert R.bleu_stats("a b c d".split(), ["x y z w v".split(), "x y z".split()])[1] == 3
    # an empty candidate scores 0 everywhere
    refs2 = [["a b".split()], ["c d".split()]]
    assert R.rouge_l([], refs2[0]) == 0.0 and R.Cider(refs2).score([], refs2[0]) == 0.0
    assert max(R.bleu_from_stats(*R.bleu_stats([], refs2[0]))) == 0.0


def test_restatement_matches_reference_functions_g20():
    g = np.load(os.path.join(HERE, "golden", "g20_caption_eval.npz"))
    words = [str(w) for w in g["words"]]
    cand = g["cand_ids"]
    I, N, _ = cand.shape
    cands = [[[words[t] for t in cand[i, n] if t >= 0] for n in range(N)] for i in range(I)]
    toks, lens, counts = g["ref_tokens"], g["ref_lengths"], g["ref_counts"]
    refs, at, r = [], 0, 0
    for i in range(I):
        rs = []
        for _ in range(counts[i]):
            rs.append([words[t] for t in toks[at: at + lens[r]]])
            at += lens[r]
            r += 1
        refs.append(rs)
    per, s = R.evaluate(cands, refs, style_words=set(str(w) for w in g["style_words"]))
    assert [s["Div-1"], s["Div-2"], s["top5 Div-1"], s["top5 Div-2"]] == pytest.approx(list(g["div"]), rel=1e-13)
    assert [s["senti_prec"], s["senti_rec"], s["has_anp"]] == pytest.approx(list(g["style"]), rel=1e-15)
    assert np.array_equal(per["top5"], g["top5"])


def test_restatement_against_pycocoevalcap():
    pytest.importorskip("pycocoevalcap")
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.cider.cider import Cider
    from pycocoevalcap.rouge.rouge import Rouge
    gts = {i: rs for i, rs in enumerate(REFS)}
    res = {i: [c] for i, c in enumerate(CANDS)}
    refs = [[r.split() for r in rs] for rs in REFS]
    per, _ = R.evaluate([[c.split()] * 5 for c in CANDS], refs)
    _, b = Bleu(4).compute_score(gts, res, verbose=0)
    assert np.allclose(np.array(b).T, per["bleu"][:, 0], rtol=1e-12)
    assert np.allclose(Rouge().compute_score(gts, res)[1], per["rouge"][:, 0], rtol=1e-12)
    assert np.allclose(Cider().compute_score(gts, res)[1], per["cider"][:, 0], rtol=1e-12)


def test_parsing_of_prediction_and_reference_files(tmp_path):
    p = tmp_path / "pred.json"
    p.write_text(json.dumps([{"image_id": 5, "caption": "a b"}, {"image_id": 3, "caption": "c"}, {"image_id": 5, "caption": "d"}]))
    got = E.load_predictions(str(p))
    assert list(got.items()) == [(5, ["a b", "d"]), (3, ["c"])]
    coco = tmp_path / "coco.json"
    coco.write_text(json.dumps({"annotations": [{"image_id": 3, "caption": "A dog."}, {"image_id": 5, "caption": "x"},
                                                {"image_id": 3, "caption": "b"}]}))
    assert dict(E.load_references(str(coco))) == {3: ["A dog.", "b"], 5: ["x"]}
    plain = tmp_path / "plain.json"
    plain.write_text(json.dumps({"3": ["a"], "x7": ["b", "c"]}))
    assert dict(E.load_references(str(plain))) == {3: ["a"], "x7": ["b", "c"]}
    with pytest.raises(ValueError, match="list of caption strings"):
        E.load_references({"3": "a"})
    # references are tokenised as the vocabulary builder does: lower case, punctuation dropped
    refs = E.CaptionReferences({3: ["A dog, running."]}, device="cpu")
    assert refs.tokens[3] == [["a", "dog", "running"]]
    with pytest.raises(ValueError, match="tokens"):
        E.CaptionReferences({3: ["..."]}, device="cpu")
    with pytest.raises(ValueError, match="tokens"):
        E.CaptionReferences({3: [" ".join(["w"] * 65)]}, device="cpu")
    tsv = tmp_path / "forms.tsv"
    tsv.write_text("happy\thappy,happier\nsad\tsad\n")
    assert E.style_words_from_tsv(str(tsv)) == {"happy", "happier", "sad"}


def test_sample_count_errors():
    refs = E.CaptionReferences({1: ["a b"], 2: ["c d"]}, device="cpu")
    with pytest.raises(ValueError, match="same number of captions"):
        refs.score_captions({1: ["a"] * 5, 2: ["c"] * 6})
    with pytest.raises(ValueError, match="at least 5 captions"):
        refs.score_captions({1: ["a"] * 4, 2: ["c"] * 4})
    import torch
    with pytest.raises(ValueError, match="int64"):
        refs.score(torch.zeros(2, 5, 3, dtype=torch.int32), 1, ["@@UNKNOWN@@", "@@BOUNDARY@@", "a"])
    with pytest.raises(ValueError, match="image ids"):
        refs.score(torch.zeros(3, 5, 3, dtype=torch.int64), 1, ["@@UNKNOWN@@", "@@BOUNDARY@@", "a"])


def test_summary_lines_follow_eval_py():
    s = {k: 0.123456 for k in ("Div-1", "Div-2", "B1", "B2", "B3", "B4", "mean B1", "mean B2", "mean B3", "mean B4", "rouge",
                               "mean rouge", "cider", "mean cider", "top5 Div-1", "top5 Div-2")}
    lines = E.format_summary(s)
    assert "B1: 12.35" in lines and "mean cider: 12.35" in lines and lines[0] == "Div-1: 0.123456"
    assert any("meteor" in x and "not computed" in x for x in lines)


def test_eval_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    assert lib.ssc_eval_refs_bytes(0, 1, 1) == 0
    assert lib.ssc_eval_refs_bytes(2, 1, 5) == 0          # fewer references than images
    assert lib.ssc_eval_refs_bytes(2, 3, 2) == 0          # fewer tokens than references
    assert lib.ssc_eval_refs_bytes(2, 3, 10) > 0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_prepare_refs(None, None)
    fake = C.c_void_p(0x1000)
    r = L.EvalRefs(2, 3, 10, 70000, fake, fake, fake, None, fake, 1 << 20)   # W > 65535
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_prepare_refs(C.byref(r), None)
    r.W = 50
    r.state_bytes = 16
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_prepare_refs(C.byref(r), None)
    r.state_bytes = lib.ssc_eval_refs_bytes(2, 3, 10)
    d = L.EvalScoreDesc(fake, 2, 5, 8, 1, 100, fake, None, fake, fake, fake, fake, fake)
    assert lib.ssc_eval_score_workspace_bytes(C.byref(r), C.byref(d)) > 0
    for field, bad in (("N", 0), ("N", 129), ("P", 0), ("steps", 0), ("V", 0), ("V", 65536), ("id_map", None), ("scores", None)):
        good = getattr(d, field)
        setattr(d, field, bad)
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_eval_score(C.byref(r), C.byref(d), fake, 256, None)
        setattr(d, field, good)
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_score(C.byref(r), C.byref(d), fake, 4, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_score(None, C.byref(d), fake, 256, None)
