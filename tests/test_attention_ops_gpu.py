"""GPU: the attention entry points one by one against the float64 reference of tests/attnstepref.py, at the shapes where the
kernels of csrc/attention.hip change form.

Backward (ssc_attn_bwd, ssc_attn_bwd_pool): the 4 waves x 5 regions batches of the region loop and their clamped tail loads, the
256-wide slices of A, the vector / scalar arms (A % 4, ldq % 4, the alignment of q, pv, wa and dpv_acc), both arms of the dalpha
kernel (F % 4, lddatt % 4, the alignment of datt) and its grid tail, the pooled addends with Da <= D, and what each buffer means:
dq written, dpv_acc and dwa_acc accumulated (dwa_acc per row g), scratch_dalpha left holding dalpha.  alpha is the float64
forward's, rounded to fp32, so the forward's error is not counted again.
Forward variants: ssc_attn_fwd_pool, ssc_attn_pool, ssc_attn_weights and ssc_attn_logits, bit-equal to ssc_attn_fwd where they
share a kernel and within its bound of float64.
ssc_attn_fwd_qslabs (q given as split-K slabs) has no public entry and stays with the train-step tests.

Bound, per output: max|got - ref| <= 2e-5 * max(1, max|ref|), the one of test_attention_forward_matches_float64: ssc_tanh_fast
(<= 2 ulp) and fp32 sums, with inputs scaled so that every output is of order 1.  Every case prints error / bound per output."""
import math

import pytest
import torch

import attnstepref as ref
from ssc_runtime import lib as L

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 2e-5
EINVAL = -1


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _place(t, off=0, ld=None, fill=NAN):
    """t (2-D, or any shape with ld None) on the device, its first element `off` floats behind a 16-byte boundary, rows `ld`
    floats apart; the floats around it hold `fill`.  -> (view, whole buffer)"""
    t = t.contiguous()
    if ld is None:
        buf = torch.full((off + t.numel() + 4,), fill, dtype=t.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + t.numel()].view(t.shape)
    else:
        rows, cols = t.shape
        buf = torch.full((off + rows * ld + 4,), fill, dtype=t.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return view, buf


def _check(name, got, want, report, scale_floor=1.0):
    """max|got - want| <= 2e-5 * max(1, max|want|); the ratio goes into `report`"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert torch.isfinite(got).all(), name
    err = (got - want).abs().max().item()
    bound = TOL * max(scale_floor, want.abs().max().item())
    report.append(f"{name} {err / bound:.3f}")
    assert err <= bound, (name, err, bound)


def _mask(n_img, R, full=None):
    mask = torch.ones(n_img, R)
    if R > 4:
        mask[0, R - 3:] = 0.0
        mask[-1, 1] = 0.0
    if full is not None:
        mask[full] = 0.0
    return mask


def _inputs(G, R, A, F, D=0, rpi=1, seed=0, full=None):
    """float32 CPU tensors: what the device is given is exactly what the reference is given"""
    g = torch.Generator().manual_seed(seed * 7919 + G * 131 + R * 17 + A + F)
    n_img = (G + rpi - 1) // rpi
    mask = _mask(n_img, R, full)
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"mask": mask, "q": r(G, A), "pv": r(n_img, R, A) * mask[:, :, None], "wa": 0.3 * r(A),
         "feats": r(n_img, R, F) * mask[:, :, None], "datt": r(G, F) / math.sqrt(F), "q2": r(G, A), "datt2": r(G, F) / math.sqrt(F),
         "dpv0": r(n_img, R, A), "dwa0": r(G, A)}
    if D:
        t["obj"] = r(n_img, R, D) * mask[:, :, None]
        t["dpa"] = r(G, D) / math.sqrt(D)
        t["dpb"] = r(G, D) / math.sqrt(D)
        t["wide"] = r(G, F + 11 + D + 3)     # the buffer datt and dpool_a are column views of (other columns: other gradients)
    return t


class _Bwd:
    """The device side of one backward case: buffers, the argument list, the call."""

    def __init__(self, t, G, R, A, F, ldq=None, q_off=0, pv_off=0, wa_off=0, dpv_off=0, lddatt=None, datt_off=0,
                 D=0, Da=0, with_b=False, view=False):
        self.G, self.R, self.A, self.F, self.D, self.Da = G, R, A, F, D, Da
        self.ldq = A if ldq is None else ldq
        self.lddq = A + 4
        self.q, _ = _place(t["q"], q_off, self.ldq)
        self.pv, _ = _place(t["pv"], pv_off)
        self.wa, _ = _place(t["wa"], wa_off)
        self.feats, _ = _place(t["feats"])
        self.dpa = self.dpb = self.obj = None
        self.lddpa = self.lddpb = 0
        if view:       # datt at column 0 and dpool_a at the odd column F + 11 of one wide buffer, as the train step's dx holds them
            wide = t["wide"].clone()
            wide[:, :F] = t["datt"]
            wide[:, F + 11:F + 11 + Da] = t["dpa"][:, :Da]
            self.wide = wide.cuda()
            self.lddatt = self.lddpa = wide.size(1)
            self.datt = self.wide[:, :F]
            self.dpa = self.wide[:, F + 11:]
        else:
            self.lddatt = F if lddatt is None else lddatt
            self.datt, _ = _place(t["datt"], datt_off, self.lddatt)
            if D:
                self.lddpa = max(Da, 1)
                self.dpa, _ = _place(t["dpa"][:, :max(Da, 1)], 0, self.lddpa)
        if D:
            self.obj, _ = _place(t["obj"])
            if with_b:
                self.lddpb = D + 2
                self.dpb, _ = _place(t["dpb"], 0, self.lddpb)
        self.dq = torch.full((G, self.lddq), NAN, device="cuda")
        self.dpv, _ = _place(t["dpv0"], dpv_off, fill=0.0)
        self.dwa = t["dwa0"].cuda()
        self.scratch = torch.full((G, R), NAN, device="cuda")
        self.alpha = None

    def args(self):
        p = lambda x: None if x is None else x.data_ptr()
        return {"datt": p(self.datt), "lddatt": self.lddatt, "q": p(self.q), "ldq": self.ldq, "pv": p(self.pv), "wa": p(self.wa),
                "alpha": p(self.alpha), "feats": p(self.feats), "G": self.G, "R": self.R, "A": self.A, "F": self.F, "dq": p(self.dq),
                "lddq": self.lddq, "dpv_acc": p(self.dpv), "dwa_acc": p(self.dwa), "scratch": p(self.scratch), "obj": p(self.obj),
                "D": self.D, "dpa": p(self.dpa), "lddpa": self.lddpa, "Da": self.Da, "dpb": p(self.dpb), "lddpb": self.lddpb}

    def call(self, pooled=None, **over):
        """-> the entry's return code (unchecked).  pooled None: ssc_attn_bwd_pool exactly when obj is set."""
        a = self.args()
        a.update(over)
        lib = L.load()
        base = [a[k] for k in ("datt", "lddatt", "q", "ldq", "pv", "wa", "alpha", "feats", "G", "R", "A", "F", "dq", "lddq", "dpv_acc",
                               "dwa_acc", "scratch")]
        if pooled is None:
            pooled = a["obj"] is not None
        if pooled:
            rc = lib._raw_ssc_attn_bwd_pool(*base, a["obj"], a["D"], a["dpa"], a["lddpa"], a["Da"], a["dpb"], a["lddpb"], L.stream_ptr())
        else:
            rc = lib._raw_ssc_attn_bwd(*base, L.stream_ptr())
        torch.cuda.synchronize()
        return rc


def _reference(t, D=0, Da=0, with_b=False, q="q", datt="datt"):
    if not D:
        return ref.backward(t[q], t["pv"], t["wa"], t["mask"], t["feats"], t[datt])
    return ref.backward(t[q], t["pv"], t["wa"], t["mask"], t["feats"], t[datt], t["obj"], t["dpa"][:, :Da],
                        t["dpb"] if with_b else None)


def _run_bwd(label, G, R, A, F, seed=0, full=None, D=0, Da=0, with_b=False, **place):
    """One call on poisoned / pre-filled buffers against the reference: every assertion on the buffers' meaning."""
    t = _inputs(G, R, A, F, D, seed=seed, full=full)
    want = _reference(t, D, Da, with_b)
    k = _Bwd(t, G, R, A, F, D=D, Da=Da, with_b=with_b, **place)
    k.alpha = want["alpha"].float().cuda()
    assert k.call() == 0
    report = []
    _check("dq", k.dq[:, :A], want["dq"], report)
    assert torch.isnan(k.dq[:, A:]).all()                         # the pad columns of a dq row are not written
    _check("dpv_acc", k.dpv, t["dpv0"].double() + want["dpv"], report)
    _check("dwa_acc[g]", k.dwa, t["dwa0"].double() + want["dwa_rows"], report)
    _check("sum_g dwa_acc", k.dwa.double().sum(0), t["dwa0"].double().sum(0) + want["dwa"], report)
    _check("dalpha", k.scratch, want["dalpha"], report)
    off = t["mask"] == 0
    if off.any():                                                 # dl is exactly 0 there: the row keeps its value
        assert torch.equal(k.dpv.cpu()[off], t["dpv0"][off])
    if full is not None:
        assert float(k.dq[full, :A].abs().max()) == 0.0
        assert float(want["dq"][full].abs().max()) == 0.0
    print(f"{label} G={G} R={R} A={A} F={F}" + (f" D={D} Da={Da} b={with_b}" if D else "") + ": error / bound " + ", ".join(report))
    return k, t, want


# ---- backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 4, 5, 19, 20, 21, 41])
def test_bwd_region_batches(R):
    """regions go in groups of 4 waves x 5: one wave only partly filled (1, 3), exactly one region per wave (4), a second one in
    wave 0 (5), one short of a group, a full group, one more (19, 20, 21), two groups and one (41); A = 260: a second slice of A
    with one float4 lane in use"""
    _run_bwd("regions", 3, R, 260, 260)


@pytest.mark.parametrize("R", [64, 65, 128, 129, 255, 256])
def test_bwd_softmax_row_lanes(R):
    """the row's c = sum_r alpha dalpha and dl walk R in strides of 64 lanes, up to the entry's limit of 256"""
    _run_bwd("lanes", 2, R, 8, 8)


def test_bwd_refuses_more_than_256_regions():
    G, R, A, F = 2, 257, 8, 8
    t = _inputs(G, R, A, F)
    k = _Bwd(t, G, R, A, F)
    k.alpha = torch.zeros(G, R, device="cuda")
    before = [_bits(x) for x in (k.dq, k.dpv, k.dwa, k.scratch)]
    assert k.call() == EINVAL
    assert all(torch.equal(b, _bits(x)) for b, x in zip(before, (k.dq, k.dpv, k.dwa, k.scratch)))


@pytest.mark.parametrize("A", [4, 252, 256, 260, 1024, 1028])
def test_bwd_slices_of_a(A):
    """one workgroup per 256-wide slice of A: a single float4, one short of a slice, a full slice, one float4 into the next, four
    slices, four and one float4"""
    _run_bwd("slices", 3, 7, A, 12)


@pytest.mark.parametrize("A", [37, 30])
def test_bwd_scalar_arm_by_width(A):
    """A % 4 != 0: the lane-contiguous scalar arm (A = 37 also makes every row of pv and dpv_acc start off a 16-byte boundary)"""
    _run_bwd("scalar", 3, 7, A, 12)


@pytest.mark.parametrize("variant", ["vector", "ldq263", "q", "pv", "wa", "dpv_acc"])
def test_bwd_vector_and_scalar_arm_on_the_same_inputs(variant):
    """A = 260 takes the vector arm; ldq = 263, or any one of q, pv, wa, dpv_acc one float off a 16-byte boundary, sends the same
    inputs (same seed) through the scalar arm.  Each result meets the bound."""
    place = {"vector": {}, "ldq263": {"ldq": 263}, "q": {"q_off": 1}, "pv": {"pv_off": 1}, "wa": {"wa_off": 1},
             "dpv_acc": {"dpv_off": 1}}[variant]
    k, _, _ = _run_bwd(variant, 3, 7, 260, 12, seed=5, **place)
    off = {"q": k.q, "pv": k.pv, "wa": k.wa, "dpv_acc": k.dpv}.get(variant)
    assert off is None or off.data_ptr() % 16 == 4


@pytest.mark.parametrize("F,pad,off", [(4, 0, 0), (256, 0, 0), (260, 0, 0), (2048, 0, 0), (101, 0, 0), (260, 4, 0), (260, 1, 0),
                                       (260, 0, 1), (2048, 4, 0), (2048, 1, 0)])
def test_bwd_dalpha_arms(F, pad, off):
    """attn_dalpha_kernel: 16-byte loads when F % 4 == 0, lddatt % 4 == 0 and datt is aligned (one float4 lane, a full 256-wide
    sweep, one lane into the second, eight sweeps), else one float per lane (F = 101, lddatt = F + 1, datt one float off)"""
    _run_bwd("dalpha", 3, 7, 12, F, lddatt=F + pad, datt_off=off)


@pytest.mark.parametrize("G,R", [(1, 1), (3, 3), (5, 7)])
def test_bwd_dalpha_grid_tail(G, R):
    """four (g, r) waves per workgroup of attn_dalpha_kernel: G * R = 1, 9, 35 leave the last workgroup partly idle"""
    _run_bwd("grid tail", G, R, 12, 12)


def test_bwd_fully_masked_image():
    """image 1 of 3 has no region: its alpha is 0, its dq exactly 0, its dpv_acc rows keep their values"""
    _run_bwd("masked image", 3, 21, 260, 260, full=1)


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("Da", ["D", 1, 0])
@pytest.mark.parametrize("D", [150, 5])
def test_bwd_pool_addends(D, Da, with_b):
    """ssc_attn_bwd_pool: dalpha += (dpool_a zero-extended from Da columns + dpool_b) . obj.  datt and dpool_a are column views of
    one wide buffer (dpool_a at the odd column F + 11, lddpa > Da, random values - other gradients - behind its Da columns), as the
    BPTT loop passes them; lddpb = D + 2.  The buffer is F + D + 14 floats wide: 176 (16-byte loads of datt) and 31 (scalar)."""
    Da = D if Da == "D" else Da
    _run_bwd("pool", 3, 7, 12, 12, D=D, Da=Da, with_b=with_b, view=True)


def test_bwd_pool_plain_buffers_and_masked_image():
    """the pooled form on buffers of their own (lddpa = Da), R in a second region group, an image without regions"""
    _run_bwd("pool plain", 3, 21, 260, 101, D=150, Da=150, with_b=True, full=2)


def test_bwd_two_calls_accumulate():
    """two steps in a row with different datt and q: dpv_acc and dwa_acc hold start + step 1 + step 2, dq and scratch_dalpha the
    second step's"""
    G, R, A, F = 3, 7, 260, 12
    t = _inputs(G, R, A, F, seed=9)
    w1, w2 = _reference(t), _reference(t, q="q2", datt="datt2")
    k = _Bwd(t, G, R, A, F)
    k.alpha = w1["alpha"].float().cuda()
    assert k.call() == 0
    k.q.copy_(t["q2"])
    k.datt.copy_(t["datt2"])
    k.alpha = w2["alpha"].float().cuda()
    assert k.call() == 0
    report = []
    _check("dq", k.dq[:, :A], w2["dq"], report)
    _check("dalpha", k.scratch, w2["dalpha"], report)
    _check("dpv_acc", k.dpv, t["dpv0"].double() + w1["dpv"] + w2["dpv"], report)
    _check("dwa_acc[g]", k.dwa, t["dwa0"].double() + w1["dwa_rows"] + w2["dwa_rows"], report)
    print("two calls: error / bound " + ", ".join(report))


@pytest.mark.parametrize("what", ["ldq", "lddq", "lddatt", "scratch", "Da>D", "lddpa", "lddpb", "dpool_a"])
def test_bwd_refusals_leave_the_outputs_alone(what):
    """each refused before any launch: non-zero, and dq, dpv_acc, dwa_acc and scratch_dalpha keep their bits"""
    G, R, A, F, D = 3, 7, 12, 12, 5
    t = _inputs(G, R, A, F, D)
    pooled = what in ("Da>D", "lddpa", "lddpb", "dpool_a")
    k = _Bwd(t, G, R, A, F, D=D if pooled else 0, Da=3 if pooled else 0, with_b=pooled)
    k.alpha = _reference(t)["alpha"].float().cuda()
    over = {"ldq": {"ldq": A - 1}, "lddq": {"lddq": A - 1}, "lddatt": {"lddatt": F - 1}, "scratch": {"scratch": None},
            "Da>D": {"Da": D + 1, "lddpa": D + 1}, "lddpa": {"lddpa": 2}, "lddpb": {"lddpb": D - 1}, "dpool_a": {"dpa": None}}[what]
    outs = (k.dq, k.dpv, k.dwa, k.scratch)
    before = [_bits(x) for x in outs]
    assert k.call(**over) != 0
    assert all(torch.equal(b, _bits(x)) for b, x in zip(before, outs))
    assert k.call() == 0                                          # (the same buffers with the argument put right are accepted)


# ---- forward variants -----------------------------------------------------------------------------------------------------------
def _fwd(t, G, R, A, F, rpi):
    """ssc_attn_fwd on the device copies of t -> (logits, alpha, att (G, F + 4) NaN-padded, device inputs)"""
    lib = L.load()
    d = {k: t[k].cuda() for k in ("q", "pv", "wa", "mask", "feats")}
    logits, alpha = torch.full((G, R), NAN, device="cuda"), torch.full((G, R), NAN, device="cuda")
    att = torch.full((G, F + 4), NAN, device="cuda")
    lib.ssc_attn_fwd(L.ptr(d["q"]), A, L.ptr(d["pv"]), L.ptr(d["wa"]), L.ptr(d["mask"]), L.ptr(d["feats"]), G, R, A, F, rpi,
                     L.ptr(logits), L.ptr(alpha), L.ptr(att), F + 4, L.stream_ptr())
    torch.cuda.synchronize()
    return logits, alpha, att, d


@pytest.mark.parametrize("D,ldpool,rpi,F", [(150, 152, 1, 260), (150, 256, 3, 101), (257, 260, 3, 260), (1, 1, 1, 101), (1, 4, 3, 260)])
def test_fwd_pool(D, ldpool, rpi, F):
    """ssc_attn_fwd_pool: logits, alpha and att are ssc_attn_fwd's bits; pool[:, :D] against float64; columns D .. ldpool-1 are 0;
    nothing behind the last row is written.  D = 257: a second pooled 256-column chunk; F = 101: the scalar arm of att."""
    G, R, A = 7, 9, 40
    t = _inputs(G, R, A, F, D, rpi=rpi)
    want = ref.forward(t["q"], t["pv"], t["wa"], t["mask"], t["feats"], t["obj"], rpi=rpi)
    lg0, al0, att0, d = _fwd(t, G, R, A, F, rpi)
    logits, alpha = torch.full((G, R), NAN, device="cuda"), torch.full((G, R), NAN, device="cuda")
    att = torch.full((G, F + 4), NAN, device="cuda")
    obj = t["obj"].cuda()
    buf = torch.full((G * ldpool + 64,), NAN, device="cuda")
    L.load().ssc_attn_fwd_pool(L.ptr(d["q"]), A, L.ptr(d["pv"]), L.ptr(d["wa"]), L.ptr(d["mask"]), L.ptr(d["feats"]), G, R, A, F, rpi,
                               L.ptr(logits), L.ptr(alpha), L.ptr(att), F + 4, L.ptr(obj), D, L.ptr(buf), ldpool, L.stream_ptr())
    torch.cuda.synchronize()
    for a, b in ((logits, lg0), (alpha, al0), (att, att0)):
        assert torch.equal(_bits(a), _bits(b))
    pool = buf[:G * ldpool].view(G, ldpool)
    report = []
    _check("pool", pool[:, :D], want["pool"], report)
    _check("att", att[:, :F], want["att"], report)
    assert torch.isnan(att[:, F:]).all()
    assert ldpool == D or float(pool[:, D:].abs().max()) == 0.0
    assert torch.isnan(buf[G * ldpool:]).all()
    print(f"fwd_pool D={D} ldpool={ldpool} rpi={rpi} F={F}: error / bound " + ", ".join(report))


@pytest.mark.parametrize("rpi", [1, 5])
@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("D", [150, 1, 129])
def test_attn_pool(D, pad, rpi):
    """ssc_attn_pool: out[g, :D] = sum_r alpha[g,r] x[img(g),r,:] from a given alpha, G = 7 rows (no multiple of rpi = 5).  Of the
    pad columns exactly those below roundup(D, 4) are zeroed; D = 129: a second 128-thread workgroup per row."""
    G, R = 7, 9
    ldo = D + pad
    t = _inputs(G, R, 8, 8, D, rpi=rpi)
    f = ref.forward(t["q"], t["pv"], t["wa"], t["mask"], t["feats"], rpi=rpi)
    alpha = f["alpha"].float()
    want = ref.pooled(alpha.double(), t["obj"].double(), rpi)
    buf, alpha_d, x_d = torch.full((G * ldo + 64,), NAN, device="cuda"), alpha.cuda(), t["obj"].cuda()
    L.load().ssc_attn_pool(L.ptr(alpha_d), L.ptr(x_d), G, R, D, rpi, L.ptr(buf), ldo, L.stream_ptr())
    torch.cuda.synchronize()
    out = buf[:G * ldo].view(G, ldo)
    report = []
    _check("out", out[:, :D], want, report)
    zeroed = min(ldo, (D + 3) // 4 * 4)
    assert zeroed == D or float(out[:, D:zeroed].abs().max()) == 0.0
    assert torch.isnan(out[:, zeroed:]).all() and torch.isnan(buf[G * ldo:]).all()
    print(f"attn_pool D={D} ldo={ldo} rpi={rpi}: error / bound " + ", ".join(report))


def _weights_and_logits(t, G, R, A, rpi, d):
    lib = L.load()
    lg1 = torch.full((G, R), NAN, device="cuda")
    lib.ssc_attn_logits(L.ptr(d["q"]), A, L.ptr(d["pv"]), L.ptr(d["wa"]), G, R, A, rpi, L.ptr(lg1), L.stream_ptr())
    lg2, al2 = torch.full((G, R), NAN, device="cuda"), torch.full((G, R), NAN, device="cuda")
    lib.ssc_attn_weights(L.ptr(d["q"]), A, L.ptr(d["pv"]), L.ptr(d["wa"]), L.ptr(d["mask"]), G, R, A, rpi, L.ptr(lg2), L.ptr(al2),
                         L.stream_ptr())
    torch.cuda.synchronize()
    return lg1, lg2, al2


@pytest.mark.parametrize("rpi", [1, 4])
@pytest.mark.parametrize("R", [8, 9])
@pytest.mark.parametrize("A", [1024, 1028, 4096])
def test_weights_and_logits(A, R, rpi):
    """ssc_attn_logits and ssc_attn_weights leave the bits ssc_attn_fwd leaves, and meet its bound of float64.  A = 1024 / 1028:
    with and without the pv rows prefetched into registers; A = 4096: the most q the kernel keeps in LDS; R = 8 / 9: one region
    group per row, and a second with one region; rpi = 4 with G = 6: rows sharing an image, the last image short of rows.
    Image 1 has no region: its alpha is 0."""
    G, F = 6, 8
    t = _inputs(G, R, A, F, rpi=rpi, full=1)
    want = ref.forward(t["q"], t["pv"], t["wa"], t["mask"], t["feats"], rpi=rpi)
    lg0, al0, _, d = _fwd(t, G, R, A, F, rpi)
    lg1, lg2, al2 = _weights_and_logits(t, G, R, A, rpi, d)
    assert torch.equal(_bits(lg1), _bits(lg0)) and torch.equal(_bits(lg2), _bits(lg0)) and torch.equal(_bits(al2), _bits(al0))
    report = []
    _check("logits", lg1, want["logits"], report)
    _check("alpha", al2, want["alpha"], report)
    rows = torch.arange(G) // rpi == 1
    assert float(al2.cpu()[rows].abs().max()) == 0.0
    print(f"weights A={A} R={R} rpi={rpi}: error / bound " + ", ".join(report))


def test_logits_refuse_more_than_4096_columns():
    G, R, A = 2, 3, 4100
    t = _inputs(G, R, A, 4)
    lib = L.load()
    d = {k: t[k].cuda() for k in ("q", "pv", "wa", "mask")}
    lg, al = torch.full((G, R), NAN, device="cuda"), torch.full((G, R), NAN, device="cuda")
    assert lib._raw_ssc_attn_logits(L.ptr(d["q"]), A, L.ptr(d["pv"]), L.ptr(d["wa"]), G, R, A, 1, L.ptr(lg), L.stream_ptr()) == EINVAL
    assert lib._raw_ssc_attn_weights(L.ptr(d["q"]), A, L.ptr(d["pv"]), L.ptr(d["wa"]), L.ptr(d["mask"]), G, R, A, 1, L.ptr(lg), L.ptr(al),
                                     L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(lg).all() and torch.isnan(al).all()


def test_rows_beyond_the_grid_limit_are_refused():
    """G rides on gridDim.y of the apply, pool and backward kernels: 65536 rows are SSC_EINVAL before any launch (the logits of
    ssc_attn_fwd included), not an invalid grid handed to the runtime"""
    G, R, A, F, D = 65536, 1, 4, 4, 1
    lib = L.load()
    z = lambda *s: torch.zeros(*s, device="cuda")
    n = lambda *s: torch.full(s, NAN, device="cuda")
    q, pv, wa, mask, feats, obj = z(G, A), z(G, R, A), z(A), torch.ones(G, R, device="cuda"), z(G, R, F), z(G, R, D)
    lg, al, att, pool, dq, dpv, dwa, scr = n(G, R), n(G, R), n(G, F), n(G, D), n(G, A), n(G, R, A), n(G, A), n(G, R)
    p, s = L.ptr, L.stream_ptr()
    rcs = {
        "fwd": lib._raw_ssc_attn_fwd(p(q), A, p(pv), p(wa), p(mask), p(feats), G, R, A, F, 1, p(lg), p(al), p(att), F, s),
        "weights": lib._raw_ssc_attn_weights(p(q), A, p(pv), p(wa), p(mask), G, R, A, 1, p(lg), p(al), s),
        "fwd_pool": lib._raw_ssc_attn_fwd_pool(p(q), A, p(pv), p(wa), p(mask), p(feats), G, R, A, F, 1, p(lg), p(al), p(att), F, p(obj), D,
                                               p(pool), D, s),
        "pool": lib._raw_ssc_attn_pool(p(mask), p(obj), G, R, D, 1, p(pool), D, s),
        "bwd": lib._raw_ssc_attn_bwd(p(att), F, p(q), A, p(pv), p(wa), p(mask), p(feats), G, R, A, F, p(dq), A, p(dpv), p(dwa), p(scr), s),
        "bwd_pool": lib._raw_ssc_attn_bwd_pool(p(att), F, p(q), A, p(pv), p(wa), p(mask), p(feats), G, R, A, F, p(dq), A, p(dpv), p(dwa),
                                               p(scr), p(obj), D, p(pool), D, D, None, 0, s),
    }
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in rcs.values()), rcs
    for x in (lg, al, att, pool, dq, dpv, dwa, scr):
        assert torch.isnan(x).all()
