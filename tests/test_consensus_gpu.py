"""GPU: consensus re-ranking (csrc/consensus.hip: l2n_rows, knn_merge, ec_score, ec_order) through ssc_runtime.evaluation against the
float64 restatement tests/consensusref.py.

Neighbours.  tau = 1e-4 is the project's parity bound for fp32 outputs, here on products of unit rows.  With the fp64 similarities s
and s_(k) the k-th largest of a query's admissible rows, a GPU list is accepted iff it holds k distinct admissible rows, every
returned row has s >= s_(k) - tau, every row with s > s_(k) + tau is returned, the returned similarities are within tau of fp64, and
the list is sorted by its own similarities with ties by bank row.  Every query of every fixture is checked.

Scores are computed from the RESTATEMENT's neighbour lists, so that test does not depend on the search: within relative 1e-12 of the
restatement, exact zeros within 1e-15 (the bound DESIGN.md 7e uses for the set kernel); pool sizes equal; the pick's restated score
within that bound of the best restated score; candidates whose GPU scores are bit-equal in index order."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import captionevalref as R
import consensusref as CR
from ssc_runtime import evaluation as E
from ssc_runtime import lib as L
from ssc_runtime.evaluation import CaptionReferences, ConsensusBank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 1e-4
UNK_TOK = ("@@UNKNOWN@@",)   # a candidate token no reference holds, equal only to itself


def dummy_caps(M):
    return [[f"w{j % 7} w{j % 5 + 7}"] for j in range(M)]


def check_lists(idx, sim, s64, k, exclude=None):
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    Q, M = s64.shape
    assert idx.shape == (Q, k) and sim.shape == (Q, k) and idx.dtype == np.int32 and sim.dtype == np.float32
    for p in range(Q):
        ok = np.ones(M, dtype=bool)
        if exclude is not None and exclude[p] >= 0:
            ok[exclude[p]] = False
        kk = min(k, int(ok.sum()))
        got = idx[p, :kk]
        assert (idx[p, kk:] == -1).all() and np.isneginf(sim[p, kk:]).all(), p
        assert (got >= 0).all() and (got < M).all() and ok[got].all() and len(set(got.tolist())) == kk, (p, got)
        cut = np.sort(s64[p, ok])[::-1][kk - 1]
        assert (s64[p, got] >= cut - TAU).all(), (p, s64[p, got].min(), cut)
        must = np.nonzero(ok & (s64[p] > cut + TAU))[0]
        assert set(must.tolist()) <= set(got.tolist()), p
        assert np.abs(sim[p, :kk].astype(np.float64) - s64[p, got]).max() <= TAU, p
        a, b = sim[p, :kk - 1], sim[p, 1:kk]
        assert ((a > b) | ((a == b) & (got[:-1] < got[1:]))).all(), p


@pytest.fixture
def gemm_mode():
    lib = L.load()
    prev = lib.ssc_set_gemm_mode(1)
    yield lib
    lib.ssc_set_gemm_mode(prev)


@pytest.mark.parametrize("mode", [1, 0], ids=["x3", "f32"])
def test_random_gaussian_neighbours_both_gemm_modes(gemm_mode, mode):
    gemm_mode.ssc_set_gemm_mode(mode)
    g = torch.Generator().manual_seed(3)
    M, F, Q = 4096, 2048, 37
    bank_x, q = torch.randn(M, F, generator=g), torch.randn(Q, F, generator=g)
    bank = ConsensusBank(bank_x, list(range(M)), dummy_caps(M))
    s64 = CR.cosine(q.numpy(), bank_x.numpy())
    for k in (1, 5, 60, 128):
        idx, sim = bank.neighbours(q, k=k)
        check_lists(idx, sim, s64, k)
    idx, sim = bank.neighbours(q, k=60, chunk_rows=1000)   # another chunking: the same acceptance
    check_lists(idx, sim, s64, 60)


def clustered(seed=5, C=12, k=8, F=128):
    """Unit centres (orthonormal) + 0.1 noise per component, exactly k bank rows per cluster, one query per cluster."""
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((F, C)))[0].T
    member = np.repeat(np.arange(C), k)
    rng.shuffle(member)
    bank_x = (centres[member] + 0.1 * rng.standard_normal((C * k, F))).astype(np.float32)
    q = (centres + 0.1 * rng.standard_normal((C, F))).astype(np.float32)
    return bank_x, q, member


def forced_sets(bank_x, q, member, k):
    """The fp64 similarities, and the assertion that lets the neighbour SET be compared exactly: every query's gap at the cut is
    more than 100 tau."""
    s64 = CR.cosine(q, bank_x)
    srt = np.sort(s64, axis=1)[:, ::-1]
    gap = srt[:, k - 1] - srt[:, k]
    print("gap at the cut: min", gap.min())
    assert (gap > 100 * TAU).all(), gap.min()
    want = CR.neighbours(s64, k)
    for c in range(q.shape[0]):
        assert set(want[c].tolist()) == set(np.nonzero(member == c)[0].tolist())
    return s64, want


def test_clustered_neighbour_sets_are_forced():
    k = 8
    bank_x, q, member = clustered(k=k)
    s64, want = forced_sets(bank_x, q, member, k)
    bank = ConsensusBank(bank_x, list(range(len(bank_x))), dummy_caps(len(bank_x)))
    idx, sim = bank.neighbours(q, k=k)
    check_lists(idx, sim, s64, k)
    got = idx.cpu().numpy()
    for c in range(q.shape[0]):
        assert set(got[c].tolist()) == set(want[c].tolist()), c


def test_odd_feature_sizes_one_query_small_bank_zero_rows_and_exclude():
    g = torch.Generator().manual_seed(9)
    for F, M, Q, k in ((100, 300, 5, 16), (50, 200, 1, 7), (37, 10, 3, 16), (2048, 33, 1, 128)):
        bank_x, q = torch.randn(M, F, generator=g), torch.randn(Q, F, generator=g)
        bank_x[M // 2] = 0.0          # a zero bank row: similarity 0 to everything
        if Q > 2:
            q[Q - 1] = 0.0        # a zero query row
        ids = [1000 + j for j in range(M)]
        bank = ConsensusBank(bank_x, ids, dummy_caps(M))
        s64 = CR.cosine(q.numpy(), bank_x.numpy())
        assert not s64[:, M // 2].any()
        idx, sim = bank.neighbours(q, k=k)
        check_lists(idx, sim, s64, k)   # M < k: the remaining slots are (-1, -inf)
        if Q > 2:
            assert idx[Q - 1, :min(k, M)].tolist() == list(range(min(k, M))) and not sim[Q - 1, :min(k, M)].any()
        # exclude: the query's own bank row (by image id) is skipped; an id the bank does not hold excludes nothing
        near = CR.neighbours(s64, 1)[:, 0]
        ex_ids = [ids[j] for j in near]
        ex_ids[0] = ids[near[0]] if Q == 1 else -5
        ex_rows = [bank.index.get(i, -1) for i in ex_ids]
        idx2, sim2 = bank.neighbours(q, k=k, exclude_ids=ex_ids)
        check_lists(idx2, sim2, s64, k, exclude=ex_rows)
        for p in range(Q):
            if ex_rows[p] >= 0:
                assert ex_rows[p] not in idx2[p].tolist()
    with pytest.raises(ValueError, match="neighbours are supported"):
        bank.neighbours(q, k=129)
    with pytest.raises(ValueError, match="queries must be"):
        bank.neighbours(torch.randn(2, 5), k=3)


def drive_merge(sims, k, chunk, exclude=None):
    lib = L.load()
    Q, M = sims.shape
    bs = torch.full((Q, k), float("-inf"), dtype=torch.float32, device="cuda")
    bi = torch.full((Q, k), -1, dtype=torch.int32, device="cuda")
    for off in range(0, M, chunk):
        mc = min(chunk, M - off)
        part = sims[:, off: off + mc].contiguous()
        lib.ssc_knn_merge(L.ptr(part), mc, Q, mc, off, k, L.ptr(exclude), L.ptr(bs), L.ptr(bi), L.stream_ptr())
    torch.cuda.synchronize()
    return bs.cpu().numpy(), bi.cpu().numpy()


def test_merge_is_exact_and_independent_of_the_chunk_size():
    g = torch.Generator().manual_seed(21)
    Q, M = 6, 40000
    sims = torch.randn(Q, M, generator=g)
    sims[1] = torch.round(sims[1] * 4) / 4            # many ties, also at the cut
    sims[2] = 0.5                                     # one value: the lowest rows win
    sims[3, ::3] = -0.0                               # -0 counts as +0
    sims[3, 1::3] = 0.0
    sims[4] = -torch.rand(M, generator=g)             # negative only
    ex = torch.tensor([-1, 17, 0, 39999, -1, 123456], dtype=torch.int32)
    dev = sims.cuda()
    canon = sims.numpy().astype(np.float64) + 0.0
    for k in (1, 60, 128):
        for excl in (None, ex):
            ref_s, ref_i = drive_merge(dev, k, M, excl.cuda() if excl is not None else None)
            for chunk in (1000, 16384, 777):
                s, i = drive_merge(dev, k, chunk, excl.cuda() if excl is not None else None)
                assert s.tobytes() == ref_s.tobytes() and i.tobytes() == ref_i.tobytes(), (k, chunk)
            for p in range(Q):                        # and they are the exact top-k: (similarity descending, row ascending)
                rows = np.lexsort((np.arange(M), -canon[p]))
                if excl is not None:
                    rows = rows[rows != int(excl[p])]
                assert ref_i[p].tolist() == rows[:k].tolist(), (k, p)
                assert np.array_equal(ref_s[p].astype(np.float64), canon[p, rows[:k]])


def test_normalize_rows():
    lib = L.load()
    g = torch.Generator().manual_seed(2)
    for rows, F, ld in ((7, 2048, 2048), (3, 5000, 5000), (5, 50, 52), (4, 33, 33), (2, 4100, 4104)):
        x = torch.randn(rows, ld, generator=g) * 3
        x[1, :F] = 0.0
        out = torch.full((rows, ld), 7.0, device="cuda")
        xd = x.cuda()
        lib.ssc_l2_normalize_rows(L.ptr(xd), rows, F, ld, L.ptr(out), ld, L.stream_ptr())
        got = out.cpu().numpy()
        x64 = x.numpy().astype(np.float64)[:, :F]
        n = np.sqrt((x64 * x64).sum(1, keepdims=True))
        want = np.where(n > 0, x64 / np.where(n > 0, n, 1), 0.0)
        assert np.abs(got[:, :F] - want).max() <= 1e-6 and not got[1, :F].any()
        assert (got[:, F:] == 7.0).all()              # nothing past the row is written
        out2 = torch.full((rows, ld), 7.0, device="cuda")
        lib.ssc_l2_normalize_rows(L.ptr(xd), rows, F, ld, L.ptr(out2), ld, L.stream_ptr())
        assert torch.equal(out, out2)


# ---- scores ---------------------------------------------------------------------------------------------------------------------

def make_case(seed, M, P, N, V, k, small=None, max_len=64, long_share=0.2, holes=0.2):
    """Vocabulary ['@@UNKNOWN@@', '@@BOUNDARY@@', 'w2', ...]; a bank of M images with 1..6 captions (some words outside the
    vocabulary); predictions (P, N, max_len + 1) with boundary 1 after each caption: duplicates, empty captions, @@UNKNOWN@@,
    full-length rows; neighbour lists from the restatement on random features, with some slots emptied."""
    rng = np.random.default_rng(seed)
    words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
    pool = small or V
    caps = []
    for _ in range(M):
        cs = []
        for _ in range(int(rng.integers(1, 7))):
            n = int(rng.choice([int(rng.integers(1, 20)), 64], p=[0.95, 0.05]))
            toks = [f"w{int(t)}" for t in rng.integers(2, pool, n)]
            if rng.random() < 0.3:
                toks[int(rng.integers(0, n))] = f"oov{int(rng.integers(0, 3))}"
            cs.append(" ".join(toks))
        caps.append(cs)
    pred = np.ones((P, N, max_len + 1), dtype=np.int64)
    for i in range(P):
        for n in range(N):
            if n % 4 == 3:
                pred[i, n] = pred[i, n - 1 - int(rng.integers(0, 3))]   # duplicate of an earlier caption
                continue
            L_ = int(rng.choice([0, 1, int(rng.integers(2, 12)), int(rng.integers(2, max_len + 1)), max_len],
                                p=[0.1, 0.1, 0.6 - long_share, 0.2, long_share]))
            if rng.random() < 0.3 and L_ > 1:   # a caption close to a bank caption, so that scores are not all tiny
                src = caps[int(rng.integers(0, M))][0].split()
                ids = np.array([int(w[1:]) if w.startswith("w") else 0 for w in src][:L_])
                L_ = len(ids)
            else:
                ids = rng.integers(2, pool, L_)
                ids[rng.random(L_) < 0.05] = 0                        # @@UNKNOWN@@
            pred[i, n, :L_] = ids
    F = 24
    bank_x = rng.standard_normal((M, F)).astype(np.float32)
    q = rng.standard_normal((P, F)).astype(np.float32)
    nb = CR.neighbours(CR.cosine(q, bank_x), k)
    for p in range(P):
        drop = rng.random(k) < holes
        drop[int(rng.integers(0, k))] = False     # at least one valid entry (and only valid bank rows where M < k)
        nb[p, drop & (np.arange(k) != int(np.argmax(nb[p] >= 0)))] = -1
    return words, caps, pred, bank_x, q, nb


def cand_tokens(words, pred):
    out = []
    for img in pred:
        cs = []
        for row in img:
            row = list(row)
            cut = row.index(1) if 1 in row else len(row)
            cs.append([UNK_TOK if t == 0 else words[t] for t in row[:cut]])
        out.append(cs)
    return out


def close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = np.where(b == 0, np.abs(a) <= 1e-15, np.abs(a - b) <= 1e-12 * np.abs(b))
    assert ok.all(), (a[~ok][:5], b[~ok][:5])


def check_scores(res, ref_scores, ref_pool, pred):
    P, N = ref_scores.shape
    close(res.scores, ref_scores)
    assert np.array_equal(res.pool_refs, ref_pool)
    for p in range(P):
        best = ref_scores[p].max()
        got = ref_scores[p, res.pick[p]]
        assert got >= best - 1e-12 * abs(best) - 1e-15, (p, got, best)
        order = res.order[p]
        assert sorted(order.tolist()) == list(range(N)) and order[0] == res.pick[p]
        gs = res.scores[p, order]
        assert (gs[:-1] >= gs[1:]).all()
        same = gs[:-1] == gs[1:]
        assert (order[:-1][same] < order[1:][same]).all()             # bit-equal scores: the lower index first
        rs = ref_scores[p, order]
        assert (rs[:-1] >= rs[1:] - 1e-12 * np.abs(rs[1:]) - 1e-15).all()
        for i in range(N):
            for j in range(i):
                if np.array_equal(pred[p, i], pred[p, j]):
                    assert res.scores[p, i] == res.scores[p, j]      # equal captions score bit-equal


CASES = [dict(seed=1, M=30, P=6, N=8, V=40, k=5, small=8), dict(seed=2, M=50, P=5, N=6, V=300, k=12),
         dict(seed=3, M=12, P=3, N=1, V=30, k=1, small=6, holes=0.0), dict(seed=4, M=200, P=3, N=128, V=60, k=128, small=12),
         dict(seed=5, M=40, P=4, N=7, V=80, k=9, small=16, long_share=0.5), dict(seed=6, M=5, P=4, N=5, V=30, k=8, small=6)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"seed{c['seed']}-N{c['N']}-k{c['k']}")
def test_scores_against_restatement(case):
    words, caps, pred, bank_x, q, nb = make_case(**case)
    M = len(caps)
    bank = ConsensusBank(bank_x, list(range(M)), caps)
    pt = torch.from_numpy(pred).cuda()
    res = bank.rerank(pt, 1, words, neighbours=nb)
    bank_refs = [[c.split() for c in cs] for cs in caps]
    ref_scores, ref_pool, _, _ = CR.rerank(bank_refs, cand_tokens(words, pred), nb)
    print("largest score", ref_scores.max(), "zeros", int((ref_scores == 0).sum()), "of", ref_scores.size)
    check_scores(res, ref_scores, ref_pool, pred)
    assert np.array_equal(res.neighbours, nb) and res.neighbour_sims is None
    again = bank.rerank(pt, 1, words, neighbours=nb)                  # two calls are bit-identical
    for x, y in ((res.scores, again.scores), (res.pick, again.pick), (res.order, again.order), (res.pool_refs, again.pool_refs)):
        assert x.tobytes() == y.tobytes()


def test_one_neighbour_pool_equals_the_reference_scorer():
    """A pool of one image is CIDEr-D against that image's references with the bank's document frequencies: what ssc_eval_score
    gives when the bank is its evaluated set."""
    words, caps, pred, bank_x, q, _ = make_case(7, 25, 25, 6, 50, 1, small=10)
    bank = ConsensusBank(bank_x, list(range(25)), caps)
    pt = torch.from_numpy(pred).cuda()
    nb = np.arange(25).reshape(25, 1)
    res = bank.rerank(pt, 1, words, neighbours=nb)
    direct = bank.references.score(pt, 1, words, image_ids=list(range(25)))
    assert res.scores.tobytes() == direct.cider.tobytes()
    assert np.array_equal(res.pick, direct.oracle["cider"])


def test_bad_ids_neighbours_and_lengths_return_einval():
    words, caps, pred, bank_x, q, nb = make_case(8, 20, 3, 5, 30, 4, small=8, max_len=10)
    bank = ConsensusBank(bank_x, list(range(20)), caps)
    pt = torch.from_numpy(pred).cuda()
    good = bank.rerank(pt, 1, words, neighbours=nb)
    for bad in (len(words), -3):                       # ids outside 0..V-1
        p = pt.clone()
        p[1, 2, 0] = bad
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            bank.rerank(p, 1, words, neighbours=nb)
    for bad in (20, -2, 1 << 30):                      # neighbour indices outside -1..M-1
        n2 = nb.copy()
        n2[2, 1] = bad
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            bank.rerank(pt, 1, words, neighbours=n2)
    n2 = nb.copy()
    n2[0] = -1                                         # a query without a neighbour
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        bank.rerank(pt, 1, words, neighbours=n2)
    long = torch.full((3, 5, 70), 3, dtype=torch.int64, device="cuda")   # 70 tokens, no boundary
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        bank.rerank(long, 1, words, neighbours=nb)
    with pytest.raises(ValueError, match="neighbours must be"):
        bank.rerank(pt, 1, words, neighbours=nb[:2])
    with pytest.raises(ValueError, match="pooled_queries or neighbours"):
        bank.rerank(pt, 1, words)
    after = bank.rerank(pt, 1, words, neighbours=nb)   # the library is still fine
    assert after.scores.tobytes() == good.scores.tobytes()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def clustered_corpus(k=8, N=6):
    """The clustered fixture with captions: cluster c's bank images talk about their own words, every query has one candidate
    per cluster-ish topic plus duplicates and an empty one."""
    bank_x, q, member = clustered(k=k)
    C = q.shape[0]
    rng = np.random.default_rng(17)
    V = 2 + 6 * C
    words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
    topic = lambda c: np.arange(2 + 6 * c, 8 + 6 * c)   # noqa: E731
    caps = [[" ".join(f"w{int(t)}" for t in rng.choice(np.concatenate([topic(member[j]), topic((member[j] + 1) % C)[:2]]),
                                                       int(rng.integers(4, 9)))) for _ in range(3)] for j in range(len(member))]
    pred = np.ones((C, N, 10), dtype=np.int64)
    for c in range(C):
        for n in range(N):
            if n == N - 1:
                continue                                  # an empty caption
            if n == 3:
                pred[c, n] = pred[c, 1]                   # a duplicate
                continue
            t = topic((c + n) % C) if n % 2 else topic(c)
            L_ = int(rng.integers(3, 9))
            pred[c, n, :L_] = rng.choice(t, L_)
    return bank_x, q, member, words, caps, pred


def test_rerank_end_to_end_and_consensus_summary(tmp_path):
    k, N = 8, 6
    bank_x, q, member, words, caps, pred = clustered_corpus(k, N)
    s64, want = forced_sets(bank_x, q, member, k)
    M, C = len(caps), q.shape[0]
    ids = [500 + j for j in range(M)]
    bank = ConsensusBank(bank_x, ids, caps)
    path = str(tmp_path / "bank.pt")
    bank.save(path)
    bank = ConsensusBank.load(path)                      # through the file
    pt = torch.from_numpy(pred).cuda()
    res = bank.rerank(pt, 1, words, q, k=k)
    for c in range(C):
        assert set(res.neighbours[c].tolist()) == set(want[c].tolist())
    check_lists(torch.from_numpy(res.neighbours.astype(np.int32)), torch.from_numpy(res.neighbour_sims), s64, k)
    bank_refs = [[c.split() for c in cs] for cs in caps]
    ref_scores, ref_pool, ref_pick, _ = CR.rerank(bank_refs, cand_tokens(words, pred), res.neighbours)
    check_scores(res, ref_scores, ref_pool, pred)
    assert (ref_scores.max(1) > 0).all()
    # the restatement end to end (its own neighbour order): the same pool as a set, so the same scores within the bound
    ref2, _, _, _ = CR.rerank(bank_refs, cand_tokens(words, pred), want)
    close(res.scores, ref2)
    # test references of the query images: the consensus lines are those of the picked captions
    rng = np.random.default_rng(3)
    test_refs = {900 + c: [" ".join(f"w{int(t)}" for t in rng.integers(2 + 6 * c, 8 + 6 * c, int(rng.integers(3, 9)))) for _ in range(2)]
                 for c in range(C)}
    cr = CaptionReferences(test_refs)
    qids = list(test_refs)
    before = cr.score(pt, 1, words, image_ids=qids)
    with_c = cr.score(pt, 1, words, image_ids=qids, consensus=res)
    s0, s1 = before.summary(), with_c.summary()
    assert list(s1)[:len(s0)] == list(s0) and all(s1[k_] == s0[k_] or (s1[k_] != s1[k_] and s0[k_] != s0[k_]) for k_ in s0)
    extra = list(s1)[len(s0):]
    assert extra == ["consensus B1", "consensus B2", "consensus B3", "consensus B4", "consensus rouge", "consensus cider",
                     "consensus agreement"]
    assert E.format_summary(s0) == [x for x in E.format_summary(s1) if not x.startswith("consensus")]
    assert before.consensus_pick is None and np.array_equal(with_c.consensus_pick, res.pick)
    cands = cand_tokens(words, pred)
    per, _ = R.evaluate(cands, [[r.split() for r in test_refs[i]] for i in qids])
    rows = np.arange(C)
    sel = per["stats"][rows, res.pick]
    bl = R.bleu_from_stats(sel[:, 0].sum(), sel[:, 1].sum(), sel[:, 2:6].sum(0), sel[:, 6:10].sum(0))
    for k_ in range(4):
        assert s1[f"consensus B{k_ + 1}"] == pytest.approx(bl[k_], rel=1e-10, abs=1e-15)
    assert s1["consensus rouge"] == pytest.approx(per["rouge"][rows, res.pick].mean(), rel=1e-10, abs=1e-15)
    assert s1["consensus cider"] == pytest.approx(per["cider"][rows, res.pick].mean(), rel=1e-10, abs=1e-15)
    assert s1["consensus agreement"] == float(np.mean(res.pick == with_c.oracle["cider"]))
    with pytest.raises(ValueError, match="consensus holds"):
        cr.score(pt[:, :5], 1, words, image_ids=qids, consensus=res)
    with pytest.raises(TypeError, match="ConsensusResult"):
        cr.score(pt, 1, words, image_ids=qids, consensus=res.pick)
    # exclude: a query that is a bank image is not its own neighbour
    own = bank.rerank(pt[:2], 1, words, bank_x[:2], k=k, exclude_ids=ids[:2])
    plain = bank.rerank(pt[:2], 1, words, bank_x[:2], k=k)
    for p in range(2):
        assert plain.neighbours[p, 0] == p and p not in own.neighbours[p].tolist()


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


def test_scripts_build_a_bank_and_rerank(tmp_path):
    from ssc_runtime.data import SyntheticCaptionData
    from ssc_runtime.vocab import Vocabulary
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    V, R_, F = 40, 5, 64
    vocab_dir = tmp_path / "vocab"
    Vocabulary.synthetic(V).save_to_files(str(vocab_dir))
    # training tensors: 20 images x 2 caption rows, ragged features; images 0..5 are the ones inference.py --synthetic 6 decodes
    # (the same generator seed), so their own rows must be excluded from their neighbours
    syn = SyntheticCaptionData(6, R_, F, 8, V, seed=4321)
    g = torch.Generator().manual_seed(1)
    feats = torch.cat([syn.feats, torch.randn(14, R_, F, generator=g)])
    nb = torch.tensor([R_] * 6 + [int(x) for x in torch.randint(2, R_ + 1, (14,), generator=g)])
    caps = torch.randint(2, V, (40, 8), generator=g)
    caps[:, 6:] = 0
    train = tmp_path / "train.pt"
    # (ragged files hold one feature block per ROW: repeat every image's block for its second caption row)
    blocks = [feats[i, : int(nb[i])] for i in range(20)]
    torch.save({"caption_tokens": caps, "image_id": torch.arange(20).repeat_interleave(2),
                "features": torch.cat([b for b in blocks for _ in range(2)]), "num_boxes": nb.repeat_interleave(2)}, str(train))
    bank_path = tmp_path / "bank.pt"
    o = _run([os.path.join(ROOT, "scripts", "build_consensus_bank.py"), "--train-tensors", str(train), "--vocabulary", str(vocab_dir),
              "--output", str(bank_path), "--gpu-ids", "0"])
    assert "wrote 20 images, 40 captions, 64 features" in o
    pooled, ids, bcaps = ConsensusBank.read_file(str(bank_path))
    assert ids == list(range(20)) and all(len(c) == 2 and all(len(x.split()) == 6 for x in c) for c in bcaps)
    want = np.stack([b.numpy().astype(np.float64).mean(0) for b in blocks])
    assert np.abs(pooled.numpy() - want).max() <= 1e-5
    refs = {str(i): [" ".join(f"w{int(t)}" for t in torch.randint(2, V, (5,), generator=g)) for _ in range(3)] for i in range(5)}
    rp = tmp_path / "refs.json"
    rp.write_text(json.dumps(refs))
    out, best = tmp_path / "pred.json", tmp_path / "best.json"
    o1 = _run([os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "6",
               "--vocab-size", str(V), "--num-boxes", str(R_), "--output-path", str(out), "--images-per-call", "4",
               "--references", str(rp), "--consensus-bank", str(bank_path), "--consensus-k", "5", "--consensus-output", str(best)])
    picked = json.load(open(best))
    groups = E.load_predictions(str(out))
    assert [e["image_id"] for e in picked] == list(groups) == list(range(6))
    assert all(e["caption"] in groups[e["image_id"]] for e in picked)
    lines1 = [x for x in o1.splitlines() if x.startswith("consensus")]
    assert [x.split(":")[0] for x in lines1] == ["consensus B1", "consensus B2", "consensus B3", "consensus B4", "consensus rouge",
                                                  "consensus cider", "consensus agreement"]
    # the picks are the restatement's: neighbours of the pooled synthetic features with the image's own row excluded
    bank_refs = [[c.split() for c in cs] for cs in bcaps]
    s64 = CR.cosine(syn.feats.numpy().astype(np.float64).mean(1), pooled.numpy())
    nbr = CR.neighbours(s64, 5, exclude=list(range(6)))
    srt = np.sort(np.where(np.eye(6, 20, dtype=bool), -np.inf, s64), axis=1)[:, ::-1]
    if ((srt[:, 4] - srt[:, 5]) > 100 * TAU).all():      # (only where the neighbour sets are forced)
        ref_scores, _, _, _ = CR.rerank(bank_refs, [[c.split() for c in caps_] for caps_ in groups.values()], nbr)
        for p, e in enumerate(picked):
            got = ref_scores[p, groups[p].index(e["caption"])]
            assert got >= ref_scores[p].max() * (1 - 1e-12) - 1e-15
    # evaluate.py: the same lines from the JSON, features from a query tensor file
    qt = tmp_path / "query.pt"
    torch.save({"caption_tokens": torch.zeros(6, 1, dtype=torch.long), "image_id": torch.arange(6), "image_features": syn.feats}, str(qt))
    summ, best2 = tmp_path / "summary.json", tmp_path / "best2.json"
    o2 = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp), "--gpu-ids", "0",
               "--consensus-bank", str(bank_path), "--query-tensors", str(qt), "--consensus-k", "5", "--output-json", str(summ),
               "--consensus-output", str(best2)])
    assert [x for x in o2.splitlines() if x.startswith("consensus")] == lines1
    assert json.load(open(best2)) == picked
    assert "consensus cider" in json.load(open(summ))
    # a prediction image without features is an error that names the id
    torch.save({"caption_tokens": torch.zeros(5, 1, dtype=torch.long), "image_id": torch.arange(5), "image_features": syn.feats[:5]}, str(qt))
    o3 = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp), "--gpu-ids", "0",
               "--consensus-bank", str(bank_path), "--query-tensors", str(qt)], ok=False)
    assert "prediction image 5" in o3
    # without the flags neither script prints the lines
    o4 = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--predictions", str(out), "--references", str(rp), "--gpu-ids", "0"])
    assert "consensus" not in o4
