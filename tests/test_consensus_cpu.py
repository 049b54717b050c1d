"""CPU: the float64 restatement of consensus re-ranking (tests/consensusref.py) against hand-worked cases; the new symbols in the
header and the ctypes table; the argument checks that need no GPU; the bank file round trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import captionevalref as R
import consensusref as CR
from ssc_runtime import evaluation as E
from ssc_runtime import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ssc_eval_consensus", "ssc_eval_consensus_workspace_bytes", "ssc_knn_merge", "ssc_l2_normalize_rows"]

BANK = [[["a", "dog", "runs", "fast"], ["the", "dog", "runs"]],
        [["a", "cat", "sleeps", "on", "the", "mat"]],
        [["two", "birds", "fly", "over", "the", "sea"], ["birds", "fly"]],
        [["a", "man", "rides", "a", "horse"]]]


def test_equal_candidate_outranks_disjoint_and_duplicates_tie_to_the_lower_index():
    cands = [[["x", "y", "z"], ["a", "dog", "runs", "fast"], ["q"], ["a", "dog", "runs", "fast"]]]
    nb = np.array([[0, 2]])
    scores, pool, pick, order = CR.rerank(BANK, cands, nb)
    assert pool.tolist() == [4]
    assert scores[0, 1] > 0 and scores[0, 0] == 0 and scores[0, 2] == 0
    assert scores[0, 1] == scores[0, 3]            # a duplicate ties ...
    assert pick.tolist() == [1]                    # ... and the lower index wins
    assert order[0].tolist() == [1, 3, 0, 2]       # stable: the zeros keep their order


def test_one_neighbour_pool_is_the_images_cider():
    cands = [[["the", "dog", "runs", "fast"], ["birds", "fly", "over"], []]]
    for j in range(len(BANK)):
        scores, pool, _, _ = CR.rerank(BANK, cands, np.array([[j, -1, -1]]))
        cid = R.Cider(BANK)
        want = [cid.score(c, BANK[j]) for c in cands[0]]
        assert scores[0].tolist() == want and pool.tolist() == [len(BANK[j])]


def test_bank_document_frequencies_are_used():
    # "the" is in three of four bank images, "horse" in one: the rarer word weighs more
    cid = R.Cider(BANK)
    assert cid.df[("the",)] == 3 and cid.df[("horse",)] == 1 and cid.ref_len == np.log(4.0)
    scores, _, pick, _ = CR.rerank(BANK, [[["the"], ["horse"]]], np.array([[3, 1]]))
    assert pick.tolist() == [1] and scores[0, 1] > scores[0, 0]


def test_neighbours_order_ties_exclude_and_small_bank():
    bank = np.array([[1.0, 0.0], [2.0, 0.0], [0.0, 3.0], [1.0, 1.0], [0.0, 0.0]])
    q = np.array([[5.0, 0.0], [0.0, 0.0], [1.0, 1.0]])
    s = CR.cosine(q, bank)
    assert s.shape == (3, 5)
    assert s[0].tolist() == pytest.approx([1.0, 1.0, 0.0, np.sqrt(0.5), 0.0])
    assert not s[1].any() and not s[:, 4].any()                      # zero rows: similarity 0 to everything
    nb = CR.neighbours(s, 3)
    assert nb[0].tolist() == [0, 1, 3]                               # rows 0 and 1 tie: the lower row first
    assert nb[1].tolist() == [0, 1, 2]                               # all equal: by row
    assert nb[2].tolist() == [3, 0, 1]
    assert CR.neighbours(s, 3, exclude=[0, -1, 3])[0].tolist() == [1, 3, 2]
    assert CR.neighbours(s, 3, exclude=[0, -1, 3])[2].tolist() == [0, 1, 2]   # the self-match is gone
    assert CR.neighbours(s, 7)[0].tolist() == [0, 1, 3, 2, 4, -1, -1]


def test_new_symbols_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(ssc_[a-z0-9_]+)\s*\(", text))
    cdll = C.CDLL(L.LIB_PATH)
    for n in NEW:
        assert n in names and n in L.SYMBOLS and hasattr(cdll, n), n
    body = text[text.index("typedef struct {\n  const int64_t* predictions;", text.index("ssc_knn_merge")):text.index("} ssc_eval_consensus_desc;")]
    fields = [n.strip() for line in re.findall(r"(?:const )?(?:int64_t\*|int\*|double\*|int)\s+([\w, ]+);", body) for n in line.split(",")]
    assert fields == [f for f, _ in L.EvalConsensusDesc._fields_]
    assert L.load().ssc_version() == 4


def test_argument_checks_need_no_gpu():
    lib = L.load()
    one = C.c_void_p(16)   # never dereferenced: every call below is refused before any launch
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_l2_normalize_rows(None, 1, 4, 4, one, 4, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_l2_normalize_rows(one, 1, 8, 4, one, 8, None)        # ld < F
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_l2_normalize_rows(one, 0, 4, 4, one, 4, None)
    for args in ((None, 8, 1, 8, 0, 4, None, one, one), (one, 8, 1, 8, 0, 129, None, one, one), (one, 8, 1, 8, 0, 0, None, one, one),
                 (one, 4, 1, 8, 0, 4, None, one, one), (one, 8, 0, 8, 0, 4, None, one, one), (one, 8, 1, 8, -1, 4, None, one, one),
                 (one, 8, 1, 8, 0, 4, None, None, one), (one, 1 << 23, 1, 1 << 23, 0, 4, None, one, one)):
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_knn_merge(*args, None)
    refs = L.EvalRefs(2, 2, 4, 3, one, one, one, None, one, 1 << 20)

    def desc(**kw):
        f = dict(predictions=one, P=2, N=3, steps=5, boundary_index=1, V=10, id_map=one, neighbours=one, k=2, scores=one,
                 pool_refs=one, pick=one, order=one)
        f.update(kw)
        return L.EvalConsensusDesc(**f)
    assert lib.ssc_eval_consensus_workspace_bytes(C.byref(refs), C.byref(desc())) > 0
    bad = [dict(N=0), dict(N=129), dict(k=0), dict(k=129), dict(P=0), dict(steps=0), dict(V=0), dict(V=65536), dict(neighbours=None),
           dict(id_map=None), dict(scores=None), dict(pool_refs=None), dict(pick=None), dict(order=None), dict(predictions=None)]
    for kw in bad:
        assert lib.ssc_eval_consensus_workspace_bytes(C.byref(refs), C.byref(desc(**kw))) == 0, kw
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_eval_consensus(C.byref(refs), C.byref(desc(**kw)), one, 256, None)
    assert lib.ssc_eval_consensus_workspace_bytes(None, C.byref(desc())) == 0
    assert lib.ssc_eval_consensus_workspace_bytes(C.byref(refs), None) == 0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_consensus(None, C.byref(desc()), one, 256, None)
    small = L.EvalRefs(2, 2, 4, 3, one, one, one, None, one, 8)     # a state too small for its own sizes
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_consensus(C.byref(small), C.byref(desc()), one, 256, None)
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_consensus(C.byref(refs), C.byref(desc()), None, 0, None)


def test_bank_file_round_trip_weights_only(tmp_path):
    pooled = torch.randn(3, 6)
    caps = [["a dog runs", "the dog"], ["a cat"], ["two birds fly", "birds", "sea birds"]]
    path = str(tmp_path / "bank.pt")
    E.ConsensusBank.write_file(path, pooled, [7, 9, 11], caps)
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(d) == ["captions", "image_id", "pooled"]
    assert d["pooled"].dtype == torch.float32 and torch.equal(d["pooled"], pooled)
    assert d["image_id"].dtype == torch.int64 and d["image_id"].tolist() == [7, 9, 11] and d["captions"] == caps
    got = E.ConsensusBank.read_file(path)
    assert torch.equal(got[0], pooled) and got[1] == [7, 9, 11] and got[2] == caps
    E.ConsensusBank.write_file(path, pooled.numpy(), ["a", "b", "c"], caps)     # ids that are not integers: strings
    assert E.ConsensusBank.read_file(path)[1] == ["a", "b", "c"]
    with pytest.raises(ValueError, match="bank file"):
        E.ConsensusBank.write_file(path, pooled, [1, 2], caps)
    torch.save({"pooled": pooled}, path)
    with pytest.raises(ValueError, match="not a consensus bank"):
        E.ConsensusBank.read_file(path)


def test_summary_lines_without_consensus_are_unchanged():
    s = {k: 0.5 for k in ("Div-1", "Div-2", "B1", "B2", "B3", "B4", "mean B1", "mean B2", "mean B3", "mean B4", "rouge", "mean rouge",
                          "cider", "mean cider", "top5 Div-1", "top5 Div-2")}
    base = E.format_summary(s)
    assert not any("consensus" in x for x in base)
    s2 = dict(s)
    s2.update({"consensus B1": 0.25, "consensus B2": 0.25, "consensus B3": 0.25, "consensus B4": 0.25, "consensus rouge": 0.125,
               "consensus cider": 0.5, "consensus agreement": 0.75})
    more = E.format_summary(s2)
    at = more.index("mean cider: 50.0")
    assert more[at + 1: at + 8] == ["consensus B1: 25.0", "consensus B2: 25.0", "consensus B3: 25.0", "consensus B4: 25.0",
                                    "consensus rouge: 12.5", "consensus cider: 50.0", "consensus agreement: 0.75"]
    assert [x for x in more if "consensus" not in x] == base
