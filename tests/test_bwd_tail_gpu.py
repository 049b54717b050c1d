"""GPU: the once-per-step kernels around the train step's time loops.

The small-row path of ssc_colsum, the weight-gradient work list with an identity-list member and with a second destination (op
level and on whole train steps), the one-pass ssc_feat_prep and ssc_prep_tokens_rows (tokens, loss weights and the row lists in
one launch).  Float64 references are numpy, stated here.

A sequential fp32 sum of n addends a_i is within (n - 1) * 2^-24 * sum|a_i| of the exact sum (first order); an addend that is
itself a rounded product w*x adds 2^-24 * |w x|.  The bounds below are (n + 2) * 2^-24 * sum|a_i|."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from gpuutil import dev, engine_from, maxdiff
from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("rows", [1, 9, 63])
def test_colsum_small_row_path(rows, N, weighted, accumulate):
    """ssc_colsum below 64 rows (eight loads in flight, summed in row order) against float64 at the bound above.  With
    accumulate the initial value is one more addend of the sum, so it is counted in sum|a_i| (the factor stays rows + 2)."""
    g = torch.Generator().manual_seed(rows * 7 + N)
    X = torch.randn(rows, N + 2, generator=g).cuda()
    w = torch.randn(rows, generator=g).cuda() if weighted else None
    base = torch.randn(N, 3, generator=g)
    out = base.clone().cuda()
    L.load().ssc_colsum(L.ptr(X), X.stride(0), rows, N, L.ptr(w) if weighted else None, L.ptr(out), 3, accumulate, L.stream_ptr())
    torch.cuda.synchronize()
    x = X.cpu().double().numpy()[:, :N]
    if weighted:
        x = w.cpu().double().numpy()[:, None] * x
    ref, mag = x.sum(0), np.abs(x).sum(0)
    if accumulate:
        b0 = base[:, 0].double().numpy()
        ref, mag = ref + b0, mag + np.abs(b0)
    err = np.abs(out.cpu()[:, 0].double().numpy() - ref)
    bound = (rows + 2) * U * mag
    print(f"rows={rows} N={N} weighted={weighted} accumulate={accumulate}: max error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert torch.equal(out.cpu()[:, 1:], base[:, 1:])           # the cells between the strided outputs


# ---- whole train steps ----------------------------------------------------------------------------------------------------------
def _tiny_step():
    cfg = oracle.OracleConfig(vocab_size=24, image_feature_size=16, embedding_size=8, hidden_size=8, attention_projection_size=8,
                              z_space=4, max_caption_length=4, sentiment_vae=1, senti_prior_multip=0.5)
    params = oracle.init_params(cfg, seed=23)
    g = torch.Generator().manual_seed(4)
    B, R, Lc = 5, 3, 4
    feats = torch.randn(B, R, 16, generator=g)
    caps = _tiny_caps()
    senti = torch.tensor([[1.0], [0.0], [-1.0], [1.0], [-1.0]])
    eps = torch.randn(Lc + 1, B, 4, generator=g)
    return cfg, params, feats, caps, senti, eps


def _tiny_caps():
    caps = torch.zeros(5, 4, dtype=torch.long)                  # row 0: empty
    caps[1] = torch.tensor([5, 9, 2, 17])                       # full
    caps[2, :3] = torch.tensor([6, 0, 11])                      # id 0 inside
    caps[3, :1] = 7
    caps[4, :2] = torch.tensor([3, 21])
    return caps


def _oracle_grads(cfg, params, feats, caps, senti, eps):
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = oracle.train_forward(p, cfg, feats, caps, senti, eps)
    oracle.train_objective(out, cfg).backward()
    return {k: v.grad.clone() for k, v in p.items()}


def _step_grads(cfg, params, feats, caps, senti, eps):
    """(one-call gradients, phased gradients) of one train step"""
    B = feats.size(0)
    eng = engine_from(cfg, params)
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * cfg.kld_weight), device="cuda")
    batch = (dev(feats), dev(caps), dev(senti), dev(eps))

    def grads(run):
        eng.forward(*batch)
        eng.grads.flat.fill_(NAN)
        run()
        torch.cuda.synchronize()
        return eng.grad_dict()

    return grads(lambda: eng.backward(gl, gk)), grads(lambda: eng.backward_phased(gl, gk, (16, 32, 64, 128, 4, 8)))


def _check_step(cfg, got, phased, want, tol):
    from ssc_runtime.engine import P_ATT, P_DEC
    E, F, H = cfg.embedding_size, cfg.image_feature_size, cfg.hidden_size
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(_bits(v), _bits(phased[k])), k
    # the two gradients that are one product: stored twice by the work list's tile epilogue (or copied), never recomputed
    assert torch.equal(_bits(got[P_ATT + "weight_hh"]), _bits(got[P_ATT + "weight_ih"][:, E + F:E + F + H]))
    assert torch.equal(_bits(got[P_DEC + "weight_hh"]), _bits(got[P_DEC + "weight_ih"][:, F + H:F + 2 * H]))
    for k, w in want.items():
        d, scale = maxdiff(got[k], w), tol(w)
        if k == P_ATT + "weight_ih":
            print(f"{k}: averaged-feature block, max difference to the oracle {maxdiff(got[k][:, E:E + F], w[:, E:E + F]):.3e}")
        assert d < scale, (k, d, scale)


def test_tiny_step_with_edge_captions_matches_oracle_and_phases():
    """B = 5, R = 3, L = 4, E = H = A = 8, F = 16, Z = 4, V = 24, SENTIMENT_VAE = 1; captions: an empty one, a full one, one with
    id 0 inside.  Every gradient against the CPU oracle as tests/test_train_gpu.py::test_edge_cases_match_oracle compares them
    (max |difference| < 1e-4); the phased backward (16, 32, 64, 128, 4, 8) equals the one-call backward bit for bit; dW_hh of the
    attention and decoder LSTMs are bit-equal to their blocks of dW_ih."""
    cfg, params, feats, caps, senti, eps = _tiny_step()
    got, phased = _step_grads(cfg, params, feats, caps, senti, eps)
    _check_step(cfg, got, phased, _oracle_grads(cfg, params, feats, caps, senti, eps), lambda w: 1e-4)


def test_work_list_sized_step_matches_oracle_and_phases():
    """At widths where the weight gradients run as the work list (B = 64: the K = B product of the per-row gate-gradient sums with
    the averaged features rides in it under the identity list, dW_hh leaves the tile epilogue as a second destination): every
    gradient within 1e-4 * max|gradient| of the CPU oracle (the bound of the full-size tests), phased = one call bit for bit."""
    cfg = oracle.OracleConfig(vocab_size=600, image_feature_size=256, embedding_size=128, hidden_size=160,
                              attention_projection_size=96, z_space=32, max_caption_length=6, sentiment_vae=1,
                              senti_prior_multip=0.5)
    params = oracle.init_params(cfg, seed=12)
    g = torch.Generator().manual_seed(6)
    B, R, Lc = 64, 5, 6
    feats = torch.randn(B, R, 256, generator=g)
    caps = torch.zeros(B, Lc, dtype=torch.long)
    for b in range(B):
        n = b % (Lc + 1)
        caps[b, :n] = torch.randint(2, 600, (n,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(Lc + 1, B, 32, generator=g)
    got, phased = _step_grads(cfg, params, feats, caps, senti, eps)
    _check_step(cfg, got, phased, _oracle_grads(cfg, params, feats, caps, senti, eps),
                lambda w: 1e-4 * max(w.abs().max().item(), 1e-6) + 1e-7)


# ---- the weight-gradient work list -----------------------------------------------------------------------------------------------
def _dw_desc(a, b, K, M, N, out, rows, cnt, out2=None):
    d = L.GemmDesc()
    d.nseg = 1
    d.seg[0].A, d.seg[0].B = a.data_ptr(), b.data_ptr()
    d.seg[0].lda, d.seg[0].ldb, d.seg[0].K = a.stride(0), b.stride(0), K
    d.M, d.N, d.a_kc, d.b_kc = M, N, 0, 0
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.splits = 1
    d.k_count, d.ka_rows, d.kb_rows = cnt.data_ptr(), rows.data_ptr(), rows.data_ptr()
    if out2 is not None:
        d.C2, d.ldc2 = out2.data_ptr(), out2.stride(0)
    return d


def _run_group(descs):
    arr = (C.POINTER(L.GemmDesc) * len(descs))(*[C.pointer(d) for d in descs])
    L.load().ssc_gemm_dw_group(arr, len(descs), L.stream_ptr())
    torch.cuda.synchronize()


def _check_product(got, a, b, rows, M, N, what):
    ad, bd = a.cpu().double().numpy()[rows][:, :M], b.cpu().double().numpy()[rows][:, :N]
    ref = ad.T @ bd
    bound = 2e-6 * (np.abs(ad).T @ np.abs(bd))                  # the bound of tests/test_gemm_gpu.py for 3xBF16 products
    err = np.abs(got.cpu().double().numpy()[:, :N] - ref)
    print(what, "max error / bound", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), what


@pytest.mark.parametrize("K", [1, 5, 64])
def test_work_list_member_with_an_identity_list(K):
    """A member whose k-row list is the identity list of K rows (the K = B product of the per-row gate-gradient sums with the
    averaged features) beside a member with a live list, M = 132, N = 260, through ssc_gemm_dw_group: both against float64 at
    2e-6 * sum|a||b|; the columns behind N stay untouched."""
    M, N, KL = 132, 260, 96
    torch.manual_seed(30 + K)
    a_id, b_id = torch.randn(K, M, device="cuda"), torch.randn(K, N + 4, device="cuda")[:, :N]
    a_lv, b_lv = torch.randn(KL, M, device="cuda"), torch.randn(KL, N, device="cuda")
    ident = torch.cat([torch.tensor([K, 0, 0, 0]), torch.arange(K)]).to(torch.int32).cuda()
    keep = torch.arange(KL)[torch.rand(KL, generator=torch.Generator().manual_seed(K)) < 0.6]
    live = torch.zeros(KL + 4, dtype=torch.int32)
    live[0] = keep.numel()
    live[4:4 + keep.numel()] = keep.to(torch.int32)
    live = live.cuda()
    out_id = torch.full((M, N + 8), NAN, device="cuda")
    out_lv = torch.full((M, N + 8), NAN, device="cuda")
    _run_group([_dw_desc(a_id, b_id, K, M, N, out_id, ident[4:], ident[:1]), _dw_desc(a_lv, b_lv, KL, M, N, out_lv, live[4:], live[:1])])
    _check_product(out_id, a_id, b_id, np.arange(K), M, N, f"identity list K={K}")
    _check_product(out_lv, a_lv, b_lv, keep.numpy(), M, N, f"live list beside K={K}")
    assert torch.isnan(out_id[:, N:]).all() and torch.isnan(out_lv[:, N:]).all()


@pytest.mark.parametrize("ldc2", [264, 261])                     # 16-byte rows, and rows the wide stores cannot take
def test_work_list_member_with_a_second_destination(ldc2):
    """A member with a second destination whose ld differs from the first's: both destinations bit-equal, the guard columns
    beside both untouched, the product within 2e-6 * sum|a||b| of float64."""
    M, N, K = 132, 260, 96
    torch.manual_seed(41)
    a, b = torch.randn(K, M, device="cuda"), torch.randn(K, N, device="cuda")
    keep = torch.arange(K)[torch.rand(K, generator=torch.Generator().manual_seed(3)) < 0.7]
    rows = torch.zeros(K, dtype=torch.int32)
    rows[:keep.numel()] = keep.to(torch.int32)
    rows, cnt = rows.cuda(), torch.tensor([keep.numel()], dtype=torch.int32).cuda()
    out = torch.full((M, N + 12), NAN, device="cuda")
    out2 = torch.full((M, ldc2), NAN, device="cuda")
    other = torch.full((M, N), NAN, device="cuda")
    _run_group([_dw_desc(a, b, K, M, N, out, rows, cnt, out2=out2), _dw_desc(a, b, K, M, N, other, rows, cnt)])
    assert torch.equal(_bits(out[:, :N]), _bits(out2[:, :N])) and torch.equal(_bits(out[:, :N]), _bits(other))
    assert torch.isnan(out[:, N:]).all() and torch.isnan(out2[:, N:]).all()
    _check_product(out, a, b, keep.numpy(), M, N, f"second destination ldc2={ldc2}")


# ---- per-sequence precompute ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,F", [(2, 3, 5), (3, 36, 260), (2, 9, 1030)])   # the last one: more columns than one sweep of a workgroup
def test_feat_prep_one_pass(B, R, F):
    """One all-zero region and one image whose regions are all zero: the mask is exact, avg is within
    (R + 2) * 2^-24 * sum_r |v_r| / max(n, 1e-8) of float64."""
    g = torch.Generator().manual_seed(B * 100 + R)
    feats = torch.randn(B, R, F, generator=g)
    feats[0, R // 2] = 0
    feats[B - 1] = 0
    fd = feats.cuda()
    mask = torch.full((B, R), NAN).cuda()
    avg = torch.full((B, F), NAN).cuda()
    L.load().ssc_feat_prep(L.ptr(fd), B, R, F, L.ptr(mask), L.ptr(avg), L.stream_ptr())
    torch.cuda.synchronize()
    v = feats.double().numpy()
    m = (np.abs(v).sum(2) > 0).astype(np.float64)
    n = np.maximum(m.sum(1), 1e-8)[:, None]
    assert np.array_equal(mask.cpu().numpy().astype(np.float64), m)
    assert m[0].sum() == R - 1 and m[B - 1].sum() == 0
    ref = (m[:, :, None] * v).sum(1) / n
    bound = (R + 2) * U * np.abs(v).sum(1) / n
    err = np.abs(avg.cpu().double().numpy() - ref)
    print(f"B={B} R={R} F={F}: max error / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert float(avg[B - 1].abs().max()) == 0.0


def _tokens_ref(caps, pad, boundary):
    """numpy restatement: boundary tokens (allennlp add_sentence_boundary_token_ids), loss weights, and the two row lists"""
    B, Lc = caps.shape
    T = Lc + 1
    tok = np.zeros((Lc + 2, B), dtype=np.int64)
    tok[0] = boundary
    tok[1:Lc + 1] = caps.T
    nb = (caps != pad).sum(1)
    tok[nb + 1, np.arange(B)] = boundary
    w = (tok[1:] != pad).astype(np.float32)
    nvalid = w.sum(0)
    on = w != 0
    later = np.flip(np.logical_or.accumulate(np.flip(on, 0), 0), 0)    # w = 1 at step t or at a later step of the caption
    lists = []
    for flags in (on, later):
        rows = np.nonzero(flags.reshape(-1))[0].astype(np.int32)
        full = np.zeros(T * B, dtype=np.int32)
        full[:rows.size] = rows
        lists.append((rows.size, full))
    return tok, w, nvalid, lists


def _random_caps(B, Lc, seed):
    g = torch.Generator().manual_seed(seed)
    caps = torch.zeros(B, Lc, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(0, Lc + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(1, 50, (n,), generator=g)
        if n > 2 and b % 3 == 0:
            caps[b, 1] = 0                                       # an in-caption id 0
    return caps


@pytest.mark.parametrize("case", ["tiny", "random", "beyond_lds"])
def test_prep_tokens_rows_equals_numpy(case):
    """B = 5, L = 4 with the captions of the train-step test; B = 65, L = 20 random; and more rows than the one-launch form keeps
    in LDS (it then runs as two launches).  tok, w, nvalid, both counts and both lists (the unused entries behind a count are 0)
    equal the numpy restatement exactly; the identity list is [B, -, -, -, 0 .. B-1] and nothing behind it is written."""
    caps = {"tiny": _tiny_caps(), "random": _random_caps(65, 20, 1), "beyond_lds": _random_caps(3000, 20, 2)}[case]
    B, Lc = caps.shape
    T, pad, boundary = Lc + 1, 0, 3
    cd = caps.cuda()
    tok = torch.full((Lc + 2, B), -7, dtype=torch.int64).cuda()
    w = torch.full((T, B), NAN).cuda()
    nvalid = torch.full((B,), NAN).cuda()
    act = torch.full((T * B + 4,), -7, dtype=torch.int32).cuda()
    live = torch.full((T * B + 4,), -7, dtype=torch.int32).cuda()
    ident = torch.full((B + 4 + 2,), -7, dtype=torch.int32).cuda()
    L.load().ssc_prep_tokens_rows(L.ptr(cd), B, Lc, pad, boundary, L.ptr(tok), L.ptr(w), L.ptr(nvalid), L.ptr(act), L.ptr(live),
                                  L.ptr(ident), L.stream_ptr())
    torch.cuda.synchronize()
    idn = ident.cpu().numpy()
    assert idn[0] == B and np.array_equal(idn[4:B + 4], np.arange(B)) and (idn[B + 4:] == -7).all()
    rtok, rw, rnv, lists = _tokens_ref(caps.numpy(), pad, boundary)
    assert np.array_equal(tok.cpu().numpy(), rtok)
    assert np.array_equal(w.cpu().numpy(), rw)
    assert np.array_equal(nvalid.cpu().numpy(), rnv)
    for name, got, (count, rows) in (("act", act, lists[0]), ("live", live, lists[1])):
        got = got.cpu().numpy()
        assert got[0] == count, name
        assert np.array_equal(got[4:], rows), name
    assert lists[1][0] > lists[0][0] or case == "tiny"          # in-caption zeros make the live list the longer one
