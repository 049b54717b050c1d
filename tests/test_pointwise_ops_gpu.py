"""GPU: the small kernels of csrc/pointwise.hip that ran only inside whole train steps, one by one.

ssc_colsum2 on its two-stage path (rows >= 64 with scratch: 64 row chunks of ceil(rows / 64) rows, then the chunks) and on the
one-pass kernel it takes without scratch; ssc_bias_tanh and ssc_tanh_bwd; the refusals of both tanh entries; and the three pure
data movers ssc_copy_strided, ssc_embed_gather and ssc_prep_tokens, bit for bit against numpy.

Bounds (U = 2^-24, half an ulp of 1):
  column sums  (rows + 2) * U * sum|a_i|: a sum of n fp32 addends in ANY order is within (n - 1) U sum|a_i| of the exact one (first
               order), an addend that is a rounded product adds U |a_i| (the derivation at the top of test_bwd_tail_gpu.py);
  tanh         U |x + bias| + 4 U: the rounding of the fp32 sum x + bias through a slope <= 1, then a 2-ulp tanhf and the store;
  tanh bwd     4 U |dy|: y*y, 1 - y*y and the product round once each, every one of them at most U |dy| of the result."""
import numpy as np
import pytest
import torch

from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
EINVAL = -1


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- column sums ----------------------------------------------------------------------------------------------------------------
def _colsum(X, rows, N, w, out, stride, out2, accumulate, scratch):
    L.load().ssc_colsum2(L.ptr(X), X.stride(0), rows, N, L.ptr(w), L.ptr(out), stride, L.ptr(out2), accumulate, L.ptr(scratch),
                         L.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 256, 257])
@pytest.mark.parametrize("rows", [64, 65, 127, 128, 1344, 4097])
def test_colsum2_two_stage_path(rows, N):
    """rows: the threshold, 65 and 127 (chunks of 2 rows: 31 resp. 0 empty trailing chunks and a last chunk of one row), 128, the
    train step's T*B = 1344, and 4097 (chunks of 65 = 8 x 8 + 1 rows).  N: around the 64 columns of a stage-2 workgroup and the 256
    of a stage-1 workgroup.  ldx = N + 3.  Every combination of wrow, out_stride 1 / 3, out2 and accumulate; the scratch starts as
    NaN.  Then the same sums without scratch (the one-pass kernel), and a second call for bit-identical results."""
    g = torch.Generator().manual_seed(rows * 31 + N)
    X = torch.randn(rows, N + 3, generator=g).cuda()
    w = torch.randn(rows, generator=g).cuda()
    base = torch.randn(N, 3, generator=g)
    x64 = X.cpu().double().numpy()[:, :N]
    worst = 0.0
    for weighted in (False, True):
        a = w.cpu().double().numpy()[:, None] * x64 if weighted else x64
        s, mag = a.sum(0), np.abs(a).sum(0)
        for stride in (1, 3):
            for with_out2 in (False, True):
                for accumulate in (0, 1):
                    b0 = base[:, 0].double().numpy()
                    ref, bound = (s + b0, (rows + 2) * U * (mag + np.abs(b0))) if accumulate else (s, (rows + 2) * U * mag)
                    for two_stage in (True, False):
                        out = base[:, :stride].clone().cuda()
                        out2 = base[:, 0].clone().cuda() if with_out2 else None
                        scratch = torch.full((64 * N,), NAN, device="cuda") if two_stage else None
                        _colsum(X, rows, N, w if weighted else None, out, stride, out2, accumulate, scratch)
                        err = np.abs(out.cpu()[:, 0].double().numpy() - ref)
                        worst = max(worst, float((err / bound).max()))
                        assert (err <= bound).all(), (weighted, stride, with_out2, accumulate, two_stage)
                        assert torch.equal(out.cpu()[:, 1:], base[:, 1:stride])     # the cells between the strided outputs
                        if with_out2:
                            assert torch.equal(_bits(out2), _bits(out[:, 0]))
                        if two_stage:
                            again = base[:, :stride].clone().cuda()
                            _colsum(X, rows, N, w if weighted else None, again, stride, None, accumulate, scratch)
                            assert torch.equal(_bits(again), _bits(out))
    print(f"colsum2 rows={rows} N={N}: max error / bound {worst:.3f}")


# ---- tanh -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("rows", [1, 5])
def test_bias_tanh_and_tanh_bwd(rows, N, with_bias):
    """x <- tanh(x + bias) in place, then dy <- dy * (1 - y^2) on its result, rows N + 3 floats apart with the pad columns left
    alone.  x spans the linear part and the saturated part of tanh (3 N(0,1))."""
    g = torch.Generator().manual_seed(rows * 1000 + N)
    ld = N + 3
    x0 = torch.full((rows, ld), NAN)
    x0[:, :N] = 3.0 * torch.randn(rows, N, generator=g)
    bias = torch.randn(N, generator=g) if with_bias else None
    x, bias_d = x0.cuda(), bias.cuda() if with_bias else None
    L.load().ssc_bias_tanh(L.ptr(x), ld, rows, N, L.ptr(bias_d), L.stream_ptr())
    torch.cuda.synchronize()
    y = x.cpu()
    s = x0[:, :N].double() + (bias.double() if with_bias else 0.0)
    err = (y[:, :N].double() - torch.tanh(s)).abs()
    bound = U * s.abs() + 4 * U
    print(f"bias_tanh rows={rows} N={N} bias={with_bias}: max error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.isnan(y[:, N:]).all()

    dy0 = torch.full((rows, ld), NAN)
    dy0[:, :N] = torch.randn(rows, N, generator=g)
    dy = dy0.cuda()
    L.load().ssc_tanh_bwd(L.ptr(dy), ld, L.ptr(x), ld, rows, N, L.stream_ptr())
    torch.cuda.synchronize()
    want = dy0[:, :N].double() * (1.0 - y[:, :N].double() ** 2)
    err = (dy.cpu()[:, :N].double() - want).abs()
    bound = 4 * U * dy0[:, :N].double().abs()
    print(f"tanh_bwd rows={rows} N={N}: max error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.isnan(dy.cpu()[:, N:]).all()
    assert torch.equal(_bits(x), _bits(y))                        # y is only read


def test_tanh_entries_refuse_short_rows_and_too_many_rows():
    """ssc_tanh_bwd refuses lddy < N and ldy < N as ssc_bias_tanh refuses ldx < N; both refuse more rows than the grid's second
    dimension takes (65535) instead of handing the runtime an invalid grid.  Nothing is launched: the buffers keep their bits."""
    lib = L.load()
    g = torch.Generator().manual_seed(1)
    rows, N = 3, 8
    a0, b0 = torch.randn(rows, N, generator=g), torch.randn(rows, N, generator=g)
    a, b = a0.cuda(), b0.cuda()
    assert lib._raw_ssc_bias_tanh(L.ptr(a), N - 1, rows, N, None, L.stream_ptr()) == EINVAL
    assert lib._raw_ssc_tanh_bwd(L.ptr(a), N - 1, L.ptr(b), N, rows, N, L.stream_ptr()) == EINVAL
    assert lib._raw_ssc_tanh_bwd(L.ptr(a), N, L.ptr(b), N - 1, rows, N, L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))
    big0 = torch.randn(65536, 1, generator=g)
    big, y = big0.cuda(), torch.tanh(big0).cuda()
    assert lib._raw_ssc_bias_tanh(L.ptr(big), 1, 65536, 1, None, L.stream_ptr()) == EINVAL
    assert lib._raw_ssc_tanh_bwd(L.ptr(big), 1, L.ptr(y), 1, 65536, 1, L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(_bits(big), _bits(big0))
    assert lib._raw_ssc_bias_tanh(L.ptr(big), 1, 65535, 1, None, L.stream_ptr()) == 0      # the most rows a call takes
    torch.cuda.synchronize()
    got = big.cpu()
    assert ((got[:65535].double() - torch.tanh(big0[:65535].double())).abs() <= U * big0[:65535].double().abs() + 4 * U).all()
    assert torch.equal(_bits(got[65535:]), _bits(big0[65535:]))


# ---- data movers, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 4801])
@pytest.mark.parametrize("n", [1, 256, 257])
def test_copy_strided_equals_numpy(n, stride):
    """dst[i] = src[i * stride]: one workgroup exactly full, and one element into the second; 4801 = the stride of one column of
    a (4H + 1)-wide weight"""
    g = torch.Generator().manual_seed(n + stride)
    src = torch.randn((n - 1) * stride + 1, generator=g)
    dst, src_d = torch.full((n + 8,), NAN, device="cuda"), src.cuda()
    L.load().ssc_copy_strided(L.ptr(src_d), stride, n, L.ptr(dst), L.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dst[:n]).numpy(), _bits(src).numpy()[::stride][:n])
    assert torch.isnan(dst[n:]).all()


@pytest.mark.parametrize("E", [1, 37, 1000])
@pytest.mark.parametrize("n", [1, 700])
def test_embed_gather_equals_numpy(n, E):
    """out[i, :E] = table[ids[i], :E] with ldt = E + 3 and ldo = E + 5: repeated ids, the first and the last row of the table; the
    table's pad columns hold NaN and the output's pad columns stay as they were"""
    V = 50
    g = torch.Generator().manual_seed(n * 7 + E)
    table = torch.full((V, E + 3), NAN)
    table[:, :E] = torch.randn(V, E, generator=g)
    ids = torch.randint(0, V, (n,), generator=g)
    ids[0] = V - 1
    if n > 4:
        ids[1], ids[2], ids[3], ids[n - 1] = 0, 7, 7, 0
    out, table_d, ids_d = torch.full((n, E + 5), -3.0, device="cuda"), table.cuda(), ids.cuda()
    L.load().ssc_embed_gather(L.ptr(table_d), E + 3, L.ptr(ids_d), n, E, L.ptr(out), E + 5, L.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[:, :E]).numpy(), _bits(table[:, :E]).numpy()[ids.numpy()])
    assert (out[:, E:] == -3.0).all()


def _caps(B, Lc, shift, pad):
    """caption b is of kind (b + shift) % 5: all pad, full length, pad in the middle, one word, a random length"""
    g = torch.Generator().manual_seed(B * 100 + Lc * 3 + shift)
    caps = torch.full((B, Lc), pad, dtype=torch.long)
    for b in range(B):
        kind = (b + shift) % 5
        n = {0: 0, 1: Lc, 2: max(Lc - 1, 1), 3: 1}.get(kind, int(torch.randint(0, Lc + 1, (1,), generator=g)))
        caps[b, :n] = torch.randint(1, 60, (n,), generator=g)
        if kind == 2 and n > 2:
            caps[b, n // 2] = pad
    return caps


def _tokens_ref(caps, pad, boundary):
    """allennlp add_sentence_boundary_token_ids, time-major: a boundary token in front, one behind the caption's non-pad count;
    w[t, b] = [token t + 1 of b is not pad]; nvalid = sum_t w"""
    B, Lc = caps.shape
    tok = np.zeros((Lc + 2, B), dtype=np.int64)
    tok[0] = boundary
    tok[1:Lc + 1] = caps.T
    tok[(caps != pad).sum(1) + 1, np.arange(B)] = boundary
    w = (tok[1:] != pad).astype(np.float32)
    return tok, w, w.sum(0)


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("Lc", [1, 4, 20])
@pytest.mark.parametrize("B", [1, 5])
def test_prep_tokens_equals_numpy_and_the_rows_form(B, Lc, shift):
    """ssc_prep_tokens: tokens_tm, w_tm and nvalid equal the numpy restatement and, bit for bit, what ssc_prep_tokens_rows writes
    into the same three outputs.  Captions that are all pad, full length and with a pad in the middle (with B = 1 the one caption
    is each of them in turn)."""
    pad, boundary = 0, 3
    caps = _caps(B, Lc, shift, pad)
    T = Lc + 1
    cd = caps.cuda()

    def outputs():
        return (torch.full((Lc + 2, B), -7, dtype=torch.int64).cuda(), torch.full((T, B), NAN).cuda(), torch.full((B,), NAN).cuda())

    tok, w, nv = outputs()
    L.load().ssc_prep_tokens(L.ptr(cd), B, Lc, pad, boundary, L.ptr(tok), L.ptr(w), L.ptr(nv), L.stream_ptr())
    tok2, w2, nv2 = outputs()
    act, live = (torch.full((T * B + 4,), -7, dtype=torch.int32).cuda() for _ in range(2))
    ident = torch.full((B + 4,), -7, dtype=torch.int32).cuda()
    L.load().ssc_prep_tokens_rows(L.ptr(cd), B, Lc, pad, boundary, L.ptr(tok2), L.ptr(w2), L.ptr(nv2), L.ptr(act), L.ptr(live),
                                  L.ptr(ident), L.stream_ptr())
    torch.cuda.synchronize()
    rtok, rw, rnv = _tokens_ref(caps.numpy(), pad, boundary)
    assert np.array_equal(tok.cpu().numpy(), rtok)
    assert np.array_equal(w.cpu().numpy(), rw)
    assert np.array_equal(nv.cpu().numpy(), rnv)
    assert torch.equal(tok, tok2) and torch.equal(_bits(w), _bits(w2)) and torch.equal(_bits(nv), _bits(nv2))
