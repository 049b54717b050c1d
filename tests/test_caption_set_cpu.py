"""CPU: the float64 restatement of the caption-set diversity metrics (tests/captionsetref.py) against a worked example that can be
checked by hand and against the properties the definitions imply; the host reductions of ssc_runtime.evaluation on the same
numbers; format_summary with and without the new keys; keyword plumbing; argument validation of ssc_eval_set without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import captionsetref as S
from ssc_runtime import lib as L
from ssc_runtime import evaluation as E

# Three evaluated images whose references share no word with the captions: every df is 0, every weight is tf * log 3.
REFS = [[["x", "y"]], [["y", "z"]], [["z", "x"]]]
CAPS = ["a b c d".split(), "a b c d".split(), "e f".split()]


def test_worked_example():
    # set statistics: testlen, reflen, guess[4], correct[4]
    #   caption 0 against {a b c d, e f}: the duplicate at index 1 is a reference, so every n-gram is matched and the closest
    #   reference length is 4; caption 1 likewise; caption 2 (e f) against two copies of a b c d: nothing matches, closest length 4.
    st = S.set_stats(CAPS)
    assert st.tolist() == [[4, 4, 4, 3, 2, 1, 4, 3, 2, 1], [4, 4, 4, 3, 2, 1, 4, 3, 2, 1], [2, 4, 2, 1, 0, 0, 0, 0, 0, 0]]
    # kernel: captions 0 and 1 are equal (cosine 1 at every order), share nothing with caption 2; caption 2 has no 3- / 4-grams,
    # so its diagonal entry is (1 + 1 + 0 + 0) / 4
    df, n = S.reference_df(REFS)
    assert n == 3 and df[("x",)] == 2 and df[("x", "y")] == 1
    K = S.kernel_matrix(CAPS, df, n)
    assert K == pytest.approx(np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0.5]]), abs=1e-15)
    # eigenvalues of [[1, 1], [1, 1]] are 2 and 0; the third is 1/2
    lam = S.eigenvalues(K)
    assert lam == pytest.approx([2.0, 0.5, 0.0], abs=1e-14)
    want = -math.log(math.sqrt(2.0) / (math.sqrt(2.0) + math.sqrt(0.5))) / math.log(3.0)
    v, deg = S.self_cider(lam)
    assert v == pytest.approx(want, rel=1e-14) and not deg
    assert S.distinct(CAPS) == 2
    per, s = S.evaluate([CAPS], REFS[:1] + REFS[1:], scored=[0])
    assert s["self-cider"] == pytest.approx(want, rel=1e-14) and s["unique"] == pytest.approx(2.0 / 3.0, rel=1e-15)
    # mBLEU-1: samples 0 and 1 score r = (4 + 1e-15) / (4 + 1e-9) times BleuScorer's brevity penalty exp(1 - 1 / r) (its length
    # ratio is the same r < 1), sample 2 scores 1e-15 / 2 x exp(1 - 4 / 2)
    r0 = (4 + 1e-15) / (4 + 1e-9)
    b0 = r0 * math.exp(1 - 1 / r0)
    b2 = (1e-15 / (2 + 1e-9)) * math.exp(1 - 1 / ((2 + 1e-15) / (4 + 1e-9)))
    assert s["mBLEU-1"] == pytest.approx((2 * b0 + b2) / 3, rel=1e-14)
    # the runtime's host reductions give the same numbers from the same statistics and eigenvalues
    assert E.mbleu(st[None]) == pytest.approx([s[f"mBLEU-{k}"] for k in (1, 2, 3, 4)], rel=1e-14)
    assert E.self_cider(lam)[0] == pytest.approx(want, rel=1e-14)


def test_one_evaluated_image_is_degenerate():
    df, n = S.reference_df(REFS[:1])   # log I = 0: every weight is 0
    K = S.kernel_matrix(CAPS, df, n)
    assert not K.any()
    assert S.self_cider(S.eigenvalues(K)) == (0.0, True)
    assert E.self_cider(np.zeros(3)) == (0.0, True)
    assert S.self_cider(S.eigenvalues(S.kernel_matrix([[], [], []], *S.reference_df(REFS)))) == (0.0, True)


def test_restatement_properties():
    rng = np.random.default_rng(3)
    df, n = S.reference_df(REFS + [[["w1", "w2", "w3"]], [["w2", "w3"], ["w4"]]])
    for _ in range(20):
        N = int(rng.integers(2, 9))
        caps = [[f"w{int(t)}" for t in rng.integers(0, 7, int(rng.integers(0, 9)))] for _ in range(N)]
        K = S.kernel_matrix(caps, df, n)
        assert np.array_equal(K, K.T) or np.allclose(K, K.T, rtol=0, atol=1e-15)
        assert K.min() >= 0.0 and K.max() <= 1.0 + 1e-15
        assert S.eigenvalues(K).min() >= -1e-12
    # N identical captions: every pair matches in full, one nonzero eigenvalue
    same = ["a b c d e".split()] * 5
    per, s = S.evaluate([same, same], REFS, scored=[0, 1])
    assert s["self-cider"] == pytest.approx(0.0, abs=1e-12) and s["unique"] == pytest.approx(0.2)
    assert [s[f"mBLEU-{k}"] for k in (1, 2, 3, 4)] == pytest.approx([1.0] * 4, rel=1e-9)
    # pairwise word-disjoint captions of >= 4 words: K is the identity
    disjoint = [[f"c{i}_{t}" for t in range(4 + i)] for i in range(6)]
    per, s = S.evaluate([disjoint], REFS, scored=[0])
    assert per["kernel"][0] == pytest.approx(np.eye(6), abs=1e-15)
    assert s["self-cider"] == pytest.approx(1.0, rel=1e-12) and s["unique"] == 1.0
    assert [s[f"mBLEU-{k}"] for k in (1, 2, 3, 4)] == pytest.approx([0.0] * 4, abs=1e-12)
    # all empty captions are one caption; an empty caption is a reference of length 0
    assert S.distinct([[], [], ["a"]]) == 2
    assert S.set_stats([["a", "b"], [], ["a"]]).tolist() == [[2, 1, 2, 1, 0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0, 0, 0],
                                                             [1, 0, 1, 0, 0, 0, 1, 0, 0, 0]]   # tie |2 - 1| = |0 - 1|: the shorter
    # eigenvalues under the cut-off do not count
    assert S.self_cider([1.0, 1e-7, 0.0])[0] == 0.0 and S.self_cider([1.0, 1.0, 1e-7])[0] == pytest.approx(math.log(2) / math.log(3))
    assert S.near_cut([1.0, 3e-6, 0.0]) and not S.near_cut([1.0, 1e-3, 1e-9, 0.0])


KEYS = ("Div-1", "Div-2", "B1", "B2", "B3", "B4", "mean B1", "mean B2", "mean B3", "mean B4", "rouge", "mean rouge", "cider",
        "mean cider", "top5 Div-1", "top5 Div-2")


def test_format_summary_with_and_without_the_set_keys():
    s = {k: 0.123456 for k in KEYS}
    plain = E.format_summary(s)
    assert not any(x.startswith(("mBLEU", "self-cider", "unique")) for x in plain)
    s.update({"mBLEU-1": 0.654321, "mBLEU-2": 0.5, "mBLEU-3": 0.25, "mBLEU-4": 0.125, "self-cider": 0.87654321, "unique": 0.95})
    lines = E.format_summary(s)
    assert lines[:len(plain)] == plain
    assert lines[len(plain):] == ["mBLEU-1: 65.43", "mBLEU-2: 50.0", "mBLEU-3: 25.0", "mBLEU-4: 12.5", "self-cider: 0.8765",
                                  "unique: 0.95"]
    del s["self-cider"]   # no prediction image had references
    assert E.format_summary(s)[len(plain):] == ["mBLEU-1: 65.43", "mBLEU-2: 50.0", "mBLEU-3: 25.0", "mBLEU-4: 12.5", "unique: 0.95"]


def test_keyword_plumbing_errors():
    refs = E.CaptionReferences({1: ["a b"], 2: ["c d"]}, device="cpu")
    with pytest.raises(TypeError, match="set_diversity"):
        refs.score_captions({1: ["a"] * 5, 2: ["c"] * 5}, set_diversity="yes")
    with pytest.raises(TypeError, match="set_diversity"):
        refs.score(torch.zeros(2, 5, 3, dtype=torch.int64), 1, ["@@UNKNOWN@@", "@@BOUNDARY@@", "a"], set_diversity=1)
    with pytest.raises(ValueError, match="int64"):
        E.set_diversity(torch.zeros(2, 5, 3, dtype=torch.int32), 1, 10)
    with pytest.raises(ValueError, match="on the device"):
        E.set_diversity(torch.zeros(2, 5, 3, dtype=torch.int64), 1, 10)
    # without the keyword a result has no set fields and summary() no set keys
    r = E.EvalResult([1], np.zeros((1, 5, 6)), np.zeros((1, 5, 10), dtype=np.int64), np.ones((1, 9), dtype=np.int64), [0],
                     np.zeros((1, 5), dtype=np.int64), False)
    assert r.set_stats is None and r.set_eigenvalues is None and r.distinct is None and r.degenerate_sets is None
    assert sorted(r.summary()) == sorted(KEYS)
    sd = E.SetDiversity(S.set_stats(CAPS)[None], np.array([2]), np.zeros((1, 3, 3)), np.array([[2.0, 0.5, 0.0]]), [0])
    r = E.EvalResult([1], np.zeros((1, 5, 6)), np.zeros((1, 5, 10), dtype=np.int64), np.ones((1, 9), dtype=np.int64), [0],
                     np.zeros((1, 5), dtype=np.int64), False, sd)
    got = r.summary()
    assert set(KEYS) <= set(got)
    assert got["unique"] == pytest.approx(2 / 3) and got["self-cider"] == pytest.approx(S.self_cider([2.0, 0.5, 0.0])[0], rel=1e-14)
    assert r.degenerate_sets == 0 and r.set_eigenvalues.shape == (1, 3)


def test_eval_set_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    assert lib.ssc_version() == 4
    fake = C.c_void_p(0x1000)

    def desc():
        return L.EvalSetDesc(fake, 3, 5, 8, 1, 100, fake, fake, fake, None, fake, fake)

    d = desc()
    need = lib.ssc_eval_set_workspace_bytes(None, C.byref(d))
    assert need > 0
    for field, bad in (("N", 1), ("N", 129), ("P", 0), ("steps", 0), ("V", 0), ("V", 65536), ("predictions", None),
                       ("ref_image", None), ("set_counts", None), ("eigenvalues", None), ("distinct", None)):
        d = desc()
        setattr(d, field, bad)
        assert lib.ssc_eval_set_workspace_bytes(None, C.byref(d)) == 0, field
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_eval_set(None, C.byref(d), fake, 1 << 30, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_set(None, None, fake, 1 << 30, None)
    d = desc()
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_set(None, C.byref(d), fake, need - 1, None)
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_set(None, C.byref(d), None, need, None)
    # with references: the reference state is checked as ssc_eval_score checks it, id_map is needed, and a kernel matrix the
    # caller does not take lies in the workspace
    r = L.EvalRefs(2, 3, 10, 50, fake, fake, fake, None, fake, lib.ssc_eval_refs_bytes(2, 3, 10))
    with_refs = lib.ssc_eval_set_workspace_bytes(C.byref(r), C.byref(d))
    assert with_refs >= need + 3 * 5 * 5 * 8
    d.kernel = fake
    assert lib.ssc_eval_set_workspace_bytes(C.byref(r), C.byref(d)) == need
    d.id_map = None
    assert lib.ssc_eval_set_workspace_bytes(C.byref(r), C.byref(d)) == 0
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_set(C.byref(r), C.byref(d), fake, 1 << 30, None)
    assert lib.ssc_eval_set_workspace_bytes(None, C.byref(d)) == need   # no references: id_map is not read
    d = desc()
    r.W = 70000
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_set(C.byref(r), C.byref(d), fake, 1 << 30, None)
    r.W = 50
    r.state_bytes = 16
    with pytest.raises(L.SscError, match="SSC_EWORKSPACE"):
        lib.ssc_eval_set(C.byref(r), C.byref(d), fake, 1 << 30, None)
