"""CPU: the float64 restatement of the diverse subset selection (tests/selectref.py) - the incremental DPP rule against the
brute-force slogdet rule, the measured tolerances, the margin rule's cap on the fixtures, properties of the three rules -, the new
symbols in the header and the ctypes table, and every refusal of ssc_eval_select that needs no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import selectref as R
from ssc_runtime import evaluation as E
from ssc_runtime import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ssc_eval_select", "ssc_eval_select_workspace_bytes"]

_FX = {}


def fx_of(P, N):
    if (P, N) not in _FX:
        fx = R.fixture(P, N)
        _FX[P, N] = (fx, R.fixture_kernel(fx))
    return _FX[P, N]


# ---- the restatement against itself ---------------------------------------------------------------------------------------------

def test_fixtures_are_what_the_tests_need():
    for P, N in R.SHAPES:
        fx, K = fx_of(P, N)
        assert K.shape == (P, N, N) and np.array_equal(K, K.transpose(0, 2, 1)) and K.min() >= 0 and K.max() <= 1 + 1e-12
        assert 14 <= fx["V"] <= 32 and np.isfinite(fx["quality"]).all()
        for p in range(P):
            assert any(len(c) == 0 for c in fx["caps"][p]) and max(len(c) for c in fx["caps"][p]) <= 12
            if N >= 4:
                assert len(set(fx["caps"][p])) < N                   # duplicates
            assert not fx["eligible"][p][[len(c) == 0 for c in fx["caps"][p]]].any()


@pytest.mark.parametrize("P,N", R.SHAPES)
def test_incremental_dpp_against_brute_force_and_measured_tolerances(P, N):
    """The measurement behind selectref.TOL, made again: the largest deviation of a candidate's objective at any position, relative
    to the image's largest gain - DPP incremental against slogdet, MBR ascending against descending sums, MMR against itself."""
    fx, K = fx_of(P, N)
    dpp = mbr = 0.0
    for normalize in (True, False):
        theta = 1.0 if normalize else 0.1
        for el in (None, fx["eligible"]):
            for p in range(P):
                e = None if el is None else el[p]
                a = R.run(R.DppRule(K[p], fx["quality"][p], e, normalize, theta), N)
                b = R.run(R.DppBruteRule(K[p], fx["quality"][p], e, normalize, theta), N, forced=a["picks"])
                assert np.array_equal(a["picks"], b["picks"]) and a["n_primary"] == b["n_primary"]
                scale = np.abs(a["gains"]).max() or 1.0
                for t in range(a["n_primary"]):
                    oa, ob = a["steps"][t][0], b["steps"][t][0]
                    ok = ~np.isnan(oa)
                    assert np.array_equal(ok, ~np.isnan(ob))
                    dpp = max(dpp, float(np.abs(oa[ok] - ob[ok]).max() / scale))
                # the stop is not a near-tie: the refused gain is far below min_gain, the last accepted one far above
                if a["stop_value"] is not None:
                    assert a["stop_value"] < 1e-10 - R.TOL[R.DPP] * scale
                if a["n_primary"]:
                    assert a["gains"][a["n_primary"] - 1] > 1e-10 + R.TOL[R.DPP] * scale
                m1, m2 = R.MbrRule(K[p], None, e), R.MbrRule(K[p], None, e, reverse=True)
                mbr = max(mbr, float(np.abs(m1.s - m2.s).max() / (np.abs(m1.s).max() or 1.0)))
    print(f"P {P} N {N}: DPP incremental vs slogdet {dpp:.3g} (recorded {R.MEASURED_DPP:.3g}), MBR reversed sums {mbr:.3g} "
          f"(recorded {R.MEASURED_MBR:.3g}); bounds x{R.FACTOR:g}")
    assert dpp <= R.TOL[R.DPP] and mbr <= R.TOL[R.MBR]
    assert R.TOL == {R.MBR: 10 * R.MEASURED_MBR, R.MMR: 0.0, R.DPP: 10 * R.MEASURED_DPP}


@pytest.mark.parametrize("P,N", R.SHAPES)
def test_margin_rule_leaves_out_at_most_a_tenth_of_a_fixture(P, N):
    """The restatement judged against itself on the CPU kernel: it passes its own bounds, and the positions whose best and
    second-best distinct caption lie within the tolerance stay below the cap - the seeds are chosen so."""
    fx, K = fx_of(P, N)
    total = skipped = 0
    for method, k, normalize, masked, kw in R.grid(N):
        for p in range(P):
            el = fx["eligible"][p] if masked else None
            own = R.run(R.make_rule(method, K[p], fx["quality"][p], el, normalize, **kw), k)
            n, s, _ = R.judge(R.make_rule(method, K[p], fx["quality"][p], el, normalize, **kw), k, fx["caps"][p], R.TOL[method],
                              own["picks"], own["gains"], own["n_primary"])
            total, skipped = total + n, skipped + s
    print(f"P {P} N {N}: {skipped} of {total} positions within the margin")
    assert skipped <= R.SKIP_CAP * total


# ---- properties of the rules ------------------------------------------------------------------------------------------------------

def test_dpp_never_picks_a_duplicate_before_the_fallback():
    for P, N in ((1, 20), (5, 64)):
        fx, K = fx_of(P, N)
        for p in range(P):
            out = R.run(R.DppRule(K[p], fx["quality"][p], None, True, 1.0), N)
            prim = [fx["caps"][p][j] for j in out["picks"][: out["n_primary"]]]
            assert len(set(prim)) == len(prim) and () not in prim            # no caption twice, no empty caption
            assert out["n_primary"] <= len(set(fx["caps"][p])) - 1
            assert (out["gains"][out["n_primary"]:] == 0).all() and (out["picks"] >= 0).all()
            # the fallback is the quality order of what is left
            rest = out["picks"][out["n_primary"]:]
            assert list(rest) == sorted(rest, key=lambda j: (-fx["quality"][p][j], j))


def test_dpp_gains_are_determinant_ratios():
    fx, K = fx_of(1, 20)
    out = R.run(R.DppRule(K[0], fx["quality"][0], None, True, 0.5), 20)
    rule = R.DppRule(K[0], fx["quality"][0], None, True, 0.5)
    S = list(out["picks"][: out["n_primary"]])
    for t in range(len(S)):
        det = np.linalg.det(rule.L[np.ix_(S[: t + 1], S[: t + 1])]) / (np.linalg.det(rule.L[np.ix_(S[:t], S[:t])]) if t else 1.0)
        assert out["gains"][t] == pytest.approx(det, rel=1e-9, abs=1e-13)
    assert (np.diff(out["gains"][: len(S)]) <= 1e-12).all()                   # greedy gains of a PSD kernel do not grow


def test_mmr_with_lambda_one_is_the_quality_order():
    fx, K = fx_of(5, 20)
    for normalize in (True, False):
        picks, gains, nprim = R.select(R.MMR, K, fx["quality"], 20, None, normalize, lam=1.0)
        for p in range(5):
            q = fx["quality"][p]
            assert list(picks[p]) == sorted(range(20), key=lambda j: (-q[j], j))
            assert np.array_equal(gains[p], R.qhat(q, np.ones(20, dtype=bool), normalize)[picks[p]])
        assert (nprim == 20).all()


def test_mmr_first_pick_is_the_best_quality_whatever_lambda():
    fx, K = fx_of(1, 20)
    picks, gains, _ = R.select(R.MMR, K, fx["quality"], 3, None, True, lam=0.0)
    assert picks[0, 0] == int(np.argmax(fx["quality"][0])) and gains[0, 0] == 0.0
    assert gains[0, 1] == -K[0][picks[0, 1], picks[0, 0]]


def test_dpp_with_theta_zero_and_identity_kernel_has_unit_gains():
    K = np.eye(7)[None]
    picks, gains, nprim = R.select(R.DPP, K, None, 7, None, True, theta=0.0)
    assert list(picks[0]) == list(range(7)) and (gains == 1.0).all() and nprim[0] == 7
    q = np.linspace(-3, 2, 7)[None]
    picks, gains, nprim = R.select(R.DPP, K, q, 7, None, True, theta=0.0)
    assert list(picks[0]) == list(range(7)) and (gains == 1.0).all()


def test_mbr_ranks_an_outlier_last():
    rng = np.random.default_rng(3)
    N = 9
    K = 0.8 + 0.1 * rng.random((N, N))
    K = (K + K.T) / 2
    K[4, :] = K[:, 4] = 0.05
    np.fill_diagonal(K, 1.0)
    picks, gains, nprim = R.select(R.MBR, K[None], None, N)
    assert picks[0, -1] == 4 and nprim[0] == N and (np.diff(gains[0]) <= 0).all()
    assert gains[0, -1] == pytest.approx(0.05)
    # one eligible candidate: s = 0; none: all -1
    el = np.zeros((1, N), dtype=np.uint8)
    assert (R.select(R.MBR, K[None], None, 3, el)[0] == -1).all()
    el[0, 6] = 1
    picks, gains, nprim = R.select(R.MBR, K[None], None, 3, el)
    assert list(picks[0]) == [6, -1, -1] and not gains.any() and nprim[0] == 1


def test_all_identical_captions_dpp_picks_one_then_quality():
    K = np.full((1, 6, 6), 0.75)
    q = np.array([[0.1, 0.9, 0.3, 0.9, -1.0, 0.2]])
    picks, gains, nprim = R.select(R.DPP, K, q, 6, None, True, theta=0.0)
    assert nprim[0] == 1 and picks[0, 0] == 0 and gains[0, 0] == 0.75 and not gains[0, 1:].any()
    assert list(picks[0, 1:]) == [1, 3, 2, 5, 4]


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(ssc_[a-z0-9_]+)\s*\(", text))
    cdll = C.CDLL(L.LIB_PATH)
    for n in NEW:
        assert n in names and n in L.SYMBOLS and hasattr(cdll, n), n
    body = text[text.index("typedef struct {\n  int P, N, k;"):text.index("} ssc_eval_select_desc;")]
    fields = [n.strip() for line in re.findall(r"(?:const )?(?:uint8_t\*|double\*|int\*|double|int)\s+([\w, ]+);", body)
              for n in line.split(",")]
    assert fields == [f for f, _ in L.EvalSelectDesc._fields_]
    kinds = {"int": C.c_int, "double": C.c_double}
    for decl, names_ in re.findall(r"((?:const )?(?:uint8_t\*|double\*|int\*|double|int))\s+([\w, ]+);", body):
        for n in names_.split(","):
            want = C.c_void_p if decl.endswith("*") else kinds[decl]
            assert dict(L.EvalSelectDesc._fields_)[n.strip()] is want, n
    # the block closes the evaluation section: behind the consensus call, in front of the self-critical step
    assert text.index("ssc_eval_consensus(") < text.index("ssc_eval_select_desc;") < text.index("ssc_scst_desc;")
    assert len(L.SYMBOLS["ssc_eval_select"][1]) == 4 and len(L.SYMBOLS["ssc_eval_select_workspace_bytes"][1]) == 1
    assert re.search(r"int ssc_eval_select\(const ssc_eval_select_desc\* d, void\* workspace, size_t workspace_bytes, void\* stream\);",
                     text)
    assert re.search(r"size_t ssc_eval_select_workspace_bytes\(const ssc_eval_select_desc\* d\);", text)
    assert L.load().ssc_version() == 4


ONE = C.c_void_p(16)   # never dereferenced: every call below is refused before any launch


def desc(**kw):
    f = dict(P=2, N=6, k=3, method=3, kernel=ONE, quality=ONE, normalize=1, theta=1.0, min_gain=1e-10, eligible=None, picks=ONE,
             gains=ONE, n_primary=ONE)
    f["lambda"] = 0.5
    f.update(kw)
    return L.EvalSelectDesc(**f)


BAD = [dict(N=0), dict(N=129, k=5), dict(k=0), dict(k=7), dict(P=0), dict(method=0), dict(method=4), dict(normalize=2), dict(picks=None),
       dict(gains=None), dict(n_primary=None), dict(kernel=None), dict(quality=None), dict(quality=None, method=2),
       {"lambda": -0.01}, {"lambda": 1.01}, {"lambda": math.nan}, dict(theta=-1.0), dict(theta=math.inf), dict(theta=math.nan),
       dict(min_gain=-1e-300), dict(min_gain=math.nan), dict(P=1 << 20, N=128)]


def test_workspace_bytes_is_zero_for_bad_arguments():
    lib = L.load()
    assert lib.ssc_eval_select_workspace_bytes(None) == 0
    assert lib.ssc_eval_select_workspace_bytes(C.byref(desc())) > 0
    for kw in BAD:
        assert lib.ssc_eval_select_workspace_bytes(C.byref(desc(**kw))) == 0, kw
    # a NULL quality is fine where the rule does not read one
    for kw in (dict(quality=None, method=1), dict(quality=None, theta=0.0)):
        assert lib.ssc_eval_select_workspace_bytes(C.byref(desc(**kw))) > 0, kw
    # the DPP vectors beyond the LDS form are P x N x k doubles
    small = lib.ssc_eval_select_workspace_bytes(C.byref(desc(N=128, k=16)))
    big = lib.ssc_eval_select_workspace_bytes(C.byref(desc(N=128, k=17)))
    assert big - small == 2 * 128 * 17 * 8
    assert lib.ssc_eval_select_workspace_bytes(C.byref(desc(N=128, k=128, method=1))) == small
    assert lib.ssc_eval_select_workspace_bytes(C.byref(desc(N=128, k=128))) < (1 << 63)


def test_every_pre_launch_refusal_needs_no_gpu():
    lib = L.load()
    for kw in BAD:
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_eval_select(C.byref(desc(**kw)), ONE, 1 << 30, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_select(None, ONE, 1 << 30, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_select(C.byref(desc()), None, 1 << 30, None)
    need = lib.ssc_eval_select_workspace_bytes(C.byref(desc(N=128, k=40)))
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_select(C.byref(desc(N=128, k=40)), ONE, need - 1, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_eval_select(C.byref(desc()), ONE, 0, None)


def test_host_layer_refusals_need_no_gpu():
    import torch
    K = torch.zeros(2, 4, 4, dtype=torch.float64)
    for kw, msg in ((dict(method="best"), "method"), (dict(k=0), "k = 0"), (dict(k=5), "k = 5"), (dict(method="mmr"), "needs a quality"),
                    (dict(method="dpp"), "needs a quality")):
        with pytest.raises(ValueError, match=msg):
            E.select_captions(K, None, **{**dict(k=2), **kw})
    with pytest.raises(ValueError, match="float64"):
        E.select_captions(K.float(), None, k=2, method="mbr")
    with pytest.raises(ValueError, match=r"\(images, N, N\)"):
        E.select_captions(torch.zeros(2, 4, 3, dtype=torch.float64), None, k=2, method="mbr")
    sel = E.CaptionSelection(np.array([[2, 0], [1, -1]]), np.zeros((2, 2)), np.array([2, 1]), "dpp")
    pred = torch.arange(2 * 3 * 4).view(2, 3, 4)
    got = sel.gather(pred, boundary_index=-7)
    assert got.shape == (2, 2, 4) and torch.equal(got[0, 0], pred[0, 2]) and torch.equal(got[0, 1], pred[0, 0])
    assert torch.equal(got[1, 0], pred[1, 1]) and (got[1, 1] == -7).all()
    groups = {5: ["a", "b", "c"], 9: ["d", "e", "f"]}
    assert sel.captions(groups) == {5: ["c", "a"], 9: ["e"]}
    two = E.CaptionSelection.concat([sel, sel])
    assert two.picks.shape == (4, 2) and two.k == 2 and two.method == "dpp"


def test_summary_lines_without_a_subset_are_unchanged():
    s = {k: 0.5 for k in ("Div-1", "Div-2", "B1", "B2", "B3", "B4", "mean B1", "mean B2", "mean B3", "mean B4", "rouge", "mean rouge",
                          "cider", "mean cider", "top5 Div-1", "top5 Div-2")}
    base = E.format_summary(s)
    assert not any("subset" in x for x in base)
    s2 = dict(s)
    s2.update({"select subset Div-1": 0.31234567, "select subset distinct": 4.5, "select subset mBLEU-4": 0.25,
               "select subset oracle cider": 0.5, "select subset mean B4": 0.125})
    more = E.format_summary(s2)
    assert more[: len(base)] == base
    assert more[len(base):] == ["select subset Div-1: 0.3123", "select subset distinct: 4.5", "select subset mBLEU-4: 25.0",
                                "select subset oracle cider: 50.0", "select subset mean B4: 12.5"]
