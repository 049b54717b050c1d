"""GPU: the non-temporal stream policy (ssc_debug_set("stream_nt"), include/ssc_debug.h) changes cache-policy modifiers only -
every result is bit-identical with it off (0) and on, and as accurate as the existing tests ask of the same kernels.
Bit 2: the streams of ssc_sgd_step and ssc_sq_norm.  (Bit 1, non-temporal weight loads of the 64x256 minibatch GEMM kernels, and
bit 4, weight-gradient stores, are not built - DESIGN.md 6 - so there is no GEMM form to compare here.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from adamref import coef_of, sq_norm_rel_err
from goldenlib import group, load
from gpuutil import dev, engine_from
from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu


def _get(lib, key):
    v = C.c_int(-1)
    lib.ssc_debug_get(key, C.byref(v))
    return v.value


class _policy:
    """`with _policy(lib, mask):` - the switch is process-global: always put the library's default back"""

    def __init__(self, lib, mask):
        self.lib, self.mask = lib, mask

    def __enter__(self):
        self.prev = _get(self.lib, b"stream_nt")
        self.lib.ssc_debug_set(b"stream_nt", self.mask)

    def __exit__(self, *exc):
        self.lib.ssc_debug_set(b"stream_nt", self.prev)


def test_train_step_of_a_golden_is_bit_identical_under_every_policy():
    """Two train steps (forward, backward, clip, SGD with momentum) at the tiny dimensions of the g6_sgd fixture: loss, kld, every
    gradient and every updated parameter under stream_nt 0 and 7 (every bit of the mask, built or not)."""
    d, cfgd = load("g6_sgd")
    cfg = oracle.OracleConfig(**cfgd)
    ins = group(d, "in/")
    args = (dev(ins["feats"]), dev(ins["caps"]), dev(ins["sentiment"]), dev(ins["eps"]))
    lib = L.load()
    got = {}
    for mask in (0, 7):
        with _policy(lib, mask):
            eng = engine_from(cfg, group(d, "param/"))
            rec = []
            for it in (1, 2):
                loss, kld = eng.train_step(*args, lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=0.5,
                                           decoder_frozen=(it == 1))
                rec += [loss.clone(), kld.clone()] + list(eng.grad_dict().values()) + list(eng.state_dict().values())
            torch.cuda.synchronize()
        got[mask] = rec
    for i, (x, y) in enumerate(zip(got[0], got[7])):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y), i
    assert len(got[0]) == 2 * (2 + len(eng.grad_dict()) + len(eng.state_dict()))


@pytest.mark.parametrize("n", [4099, (1 << 20) + 3])
def test_sq_norm_and_sgd_streams_are_bit_identical_and_match_float64(n):
    """ssc_sq_norm and ssc_sgd_step on n elements (no multiple of the 16-byte vector width: bulk + tail), both policies: equal
    bit for bit, and equal to a float64 restatement of include/ssc.h's formulas - the squared norm within the bound of its
    fp32 two-pass reduction (adamref.sq_norm_rel_err), parameters and momentum within 1e-5 (test_module_gpu.py's bound for
    the fused clip + SGD)."""
    lib = L.load()
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g) * 0.1
    gr = torch.randn(n, generator=g) * 0.05
    b0 = torch.randn(n, generator=g) * 0.02
    gscale, max_norm, lr, mom, wd = 0.5, 0.5, 0.015, 0.9, 0.001
    sq64 = float((gr.double() ** 2).sum())
    res = {}
    for mask in (0, 2):
        with _policy(lib, mask):
            p, gd, buf = p0.cuda(), gr.cuda(), b0.cuda()
            scratch = torch.zeros(1025, device="cuda")
            sq = scratch[1024:1025]
            lib.ssc_sq_norm(L.ptr(gd), n, L.ptr(scratch), L.ptr(sq), L.stream_ptr())
            lib.ssc_sgd_step(L.ptr(p), L.ptr(gd), L.ptr(buf), n, L.ptr(sq), gscale, max_norm, lr, mom, wd, 0, L.stream_ptr())
            torch.cuda.synchronize()
        res[mask] = (sq.cpu().clone(), p.cpu(), buf.cpu(), gd.cpu())
        assert abs(float(sq) - sq64) <= sq_norm_rel_err(n) * sq64, (mask, float(sq), sq64)
        coef = coef_of(float(sq), gscale, max_norm)
        f = lambda x: float(np.float32(x))
        dd = gr.double() * coef + f(wd) * p0.double()
        b64 = f(mom) * b0.double() + dd
        p64 = p0.double() - f(lr) * b64
        assert (res[mask][2].double() - b64).abs().max().item() < 1e-5
        assert (res[mask][1].double() - p64).abs().max().item() < 1e-5
        assert torch.equal(res[mask][3], gr)   # the gradient is only read
    for x, y in zip(res[0], res[2]):
        assert torch.equal(x, y)
