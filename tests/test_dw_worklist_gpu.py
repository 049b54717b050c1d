"""GPU: the weight gradients of a train step as one work list (ssc_gemm_dw_group: a persistent grid of the wave-specialised
128x128 TN kernel walks the tiles of every member).  Per output element the work list runs the operations of the single
product, so every result is compared BIT FOR BIT with the same product issued alone through ssc_gemm, and against a float64
product within the project's GEMM bound 2e-6 * sum|a||b| (tests/test_gemm_gpu.py)."""
import ctypes as C

import pytest
import torch

from gpuutil import gemm
from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu


def _row_list(n, frac, seed, count=None):
    """(padded int32 list on the device, its count on the device, the listed rows)"""
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(n, generator=g) < frac
    keep[0] = True
    idx = torch.nonzero(keep).flatten()
    if count is not None:
        idx = idx[:count]
    pad = torch.zeros(n, dtype=torch.int32)
    pad[: idx.numel()] = idx.to(torch.int32)
    return pad.cuda(), torch.tensor([idx.numel()], dtype=torch.int32).cuda(), idx


def _desc(a, b, K, M, N, out, lists, accumulate=0):
    rows_a, rows_b, cnt = lists
    d = L.GemmDesc()
    d.nseg = 1
    d.seg[0].A, d.seg[0].B = a.data_ptr(), b.data_ptr()
    d.seg[0].lda, d.seg[0].ldb, d.seg[0].K = a.stride(0), b.stride(0), K
    d.M, d.N, d.a_kc, d.b_kc = M, N, 0, 0
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.accumulate = accumulate
    d.splits = 1
    d.k_count, d.ka_rows, d.kb_rows = cnt.data_ptr(), rows_a.data_ptr(), rows_b.data_ptr()
    return d


def _run_group(descs):
    lib = L.load()
    arr = (C.POINTER(L.GemmDesc) * len(descs))(*[C.pointer(d) for d in descs])
    lib.ssc_gemm_dw_group(arr, len(descs), L.stream_ptr())
    torch.cuda.synchronize()


def _check(members, K, operands_a, operands_b, lists):
    """members: (M, N, ldc, index of the row lists, accumulate); operands_*: (K, width) device tensors by width"""
    outs, singles, descs = [], [], []
    g = torch.Generator().manual_seed(99)
    for M, N, ldc, li, acc in members:
        base = torch.randn(M, ldc, generator=g).cuda() if acc else torch.full((M, ldc), float("nan"), device="cuda")
        outs.append(base.clone())
        singles.append(base.clone())
    for (M, N, ldc, li, acc), out in zip(members, outs):
        descs.append(_desc(operands_a[M], operands_b[N], K, M, N, out, lists[li][:3], acc))
    _run_group(descs)
    for (M, N, ldc, li, acc), out, one in zip(members, outs, singles):
        rows_a, rows_b, cnt, idx = lists[li]
        a, b = operands_a[M], operands_b[N]
        gemm([(a, a.stride(0), b, b.stride(0), K)], M, N, 0, 0, one, accumulate=acc, splits=1,
             compact={"k_count": cnt, "ka_rows": rows_a, "kb_rows": rows_b})
        torch.cuda.synchronize()
        got, alone = out.cpu(), one.cpu()
        what = f"member M={M} N={N} ldc={ldc} list={li} accumulate={acc}"
        # bit for bit, the columns past N (never written: NaN or the initial values) included
        assert torch.equal(got.view(torch.int32), alone.view(torch.int32)), what
        ad, bd = a.cpu().double()[idx][:, :M], b.cpu().double()[idx][:, :N]
        ref = ad.T @ bd
        bound = 2e-6 * (ad.abs().T @ bd.abs())
        prod = got[:, :N].double()
        if not acc:   # (the caller checks an accumulating member: it knows the initial values)
            err = (prod - ref).abs()
            print(what, "max error / bound", (err / bound.clamp_min(1e-30)).max().item() if idx.numel() else 0.0)
            assert (err <= bound).all(), what
        if idx.numel() == 0 and not acc:
            assert torch.count_nonzero(prod).item() == 0, what
    return outs


def test_work_list_of_mixed_members_equals_single_products():
    """15 members: M 4800 / 768 / 256, N 128 / 152 / 1000 / 1200 / 2048, leading dimensions wider than N, K rows from two
    different device-side lists (a member's A and B lists are tensors of their own), one member with k_count = 0, one with
    accumulate."""
    K = 1344
    torch.manual_seed(21)
    A = {M: torch.randn(K, M, device="cuda") for M in (4800, 768, 256)}
    B = {N: torch.randn(K, N + 8, device="cuda")[:, :N] / K ** 0.5 for N in (128, 152, 1000, 1200, 2048)}   # ldb = N + 8
    r0, c0, i0 = _row_list(K, 0.7, 3)
    r1, c1, i1 = _row_list(K, 0.4, 8)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    lists = [(r0, r0.clone(), c0, i0), (r1, r1.clone(), c1, i1), (r0, r0.clone(), zero, i0[:0])]
    members = [
        (4800, 1000, 1000 + 2248, 0, 0), (4800, 1200, 5448, 0, 0), (4800, 1200, 5448, 1, 0), (4800, 2048, 2048 + 4, 0, 0),
        (4800, 128, 5448, 1, 0), (4800, 152, 152 + 12, 0, 0), (768, 1200, 1200, 1, 0), (768, 1000, 1004, 0, 0),
        (768, 2048, 2056, 1, 0), (256, 1200, 1208, 0, 0), (256, 128, 132, 1, 0), (256, 152, 152, 0, 0),
        (4800, 1200, 1200, 2, 0),      # no live row: an exact zero product
        (768, 152, 160, 0, 1),         # accumulate
        (256, 2048, 2048, 1, 0),
    ]
    outs = _check(members, K, A, B, lists)
    # the accumulating member against float64: initial values + product
    M, N, ldc, li, _ = members[13]
    g = torch.Generator().manual_seed(99)
    base = None
    for Mi, Ni, ldci, lii, acci in members:   # (the initial values were drawn in member order)
        if acci:
            base = torch.randn(Mi, ldci, generator=g)
    ad, bd = A[M].cpu().double()[i0], B[N].cpu().double()[i0]
    ref = base[:, :N].double() + ad.T @ bd
    bound = 2e-6 * (base[:, :N].double().abs() + ad.abs().T @ bd.abs())
    err = (outs[13].cpu()[:, :N].double() - ref).abs()
    print("accumulating member: max error / bound", (err / bound).max().item())
    assert (err <= bound).all()


def test_work_list_longer_than_twenty_rounds_and_shorter_than_one():
    """More tiles than 20 x compute units (every workgroup walks more than 20 tiles) and fewer tiles than compute units (most
    workgroups of the persistent grid have no tile and leave at once)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = 160
    torch.manual_seed(22)
    A = {M: torch.randn(K, M, device="cuda") for M in (4800, 256)}
    B = {N: torch.randn(K, N, device="cuda") / K ** 0.5 for N in (2048, 152)}
    r0, c0, i0 = _row_list(K, 0.6, 5)
    lists = [(r0, r0.clone(), c0, i0)]
    per = ((4800 + 127) // 128) * (2048 // 128)
    n = 20 * cus // per + 1
    assert n <= 20 and n * per > 20 * cus
    _check([(4800, 2048, 2048, 0, 0)] * n, K, A, B, lists)
    assert 2 * 2 < cus
    _check([(256, 152, 152, 0, 0)], K, A, B, lists)


def test_one_flush_backward_equals_the_phased_backward():
    """engine.backward (ssc_train_bwd: the weight gradients of the head and of every phase in ONE work list) against
    engine.backward_phased in a legal phase order (one flush per phase) and against the per-phase launches of the debug switch:
    every gradient bit for bit."""
    import oracle
    from gpuutil import engine_from
    lib = L.load()
    cfg = oracle.OracleConfig(vocab_size=1200, image_feature_size=512, embedding_size=256, hidden_size=320,
                              attention_projection_size=192, z_space=64, max_caption_length=9, sentiment_vae=1,
                              senti_prior_multip=0.5)
    eng = engine_from(cfg, oracle.init_params(cfg, seed=11))
    g = torch.Generator().manual_seed(5)
    B, R, Lc = 64, 12, 9
    feats = torch.randn(B, R, 512, generator=g).cuda()
    caps = torch.zeros(B, Lc, dtype=torch.long)
    for b in range(B):
        n = 2 + b % 8
        caps[b, :n] = torch.randint(2, 1200, (n,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float().cuda()
    eps = torch.randn(Lc + 1, B, 64, generator=g).cuda()
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * 750.0), device="cuda")

    def grads(run):
        eng.forward(feats, caps.cuda(), senti, eps)
        eng.grads.flat.fill_(float("nan"))
        run()
        torch.cuda.synchronize()
        return {n: v.clone() for n, v in eng.grads.views.items()}

    want = grads(lambda: eng.backward(gl, gk))
    assert all(torch.isfinite(v).all() for v in want.values())
    phased = grads(lambda: eng.backward_phased(gl, gk, (16, 32, 8, 4, 2)))
    lib.ssc_debug_set(b"dw_one_flush", 0)
    try:
        per_phase = grads(lambda: eng.backward(gl, gk))
    finally:
        lib.ssc_debug_set(b"dw_one_flush", 1)
    for name, other in (("phased", phased), ("dw_one_flush=0", per_phase)):
        bad = {n: (v - want[n]).abs().max().item() for n, v in other.items() if not torch.equal(v, want[n])}
        assert not bad, (name, bad)
