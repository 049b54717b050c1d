"""GPU: every kernel form of the constrained / plain beam selection (decode.hip, fsm.hip over the shared core of beam_common.h)
against tests/cbsref.py, the numpy restatement that tests/test_cbs_ref_cpu.py pins to the oracle's search and to hand-worked tie
cases.  The stages are checked one at a time:
  rows stage   scratch_val / scratch_idx as the entry left them, against cbsref.rows (cbsref.rows_from_records for the records entry);
  merge stage  pred / lp_out / backptr against cbsref.merge applied to the DEVICE's scratch (one float32 add per key: always bit-equal).
Indices are exact everywhere, the slots at -inf and at the -1e20 fills included; nothing is masked out of a comparison.  Values of
the log-prob entries are bit-equal; values of the raw-logit entries (`*_logits`, raw_logits = 1, records) are held to the project's
tolerance statement (1e-4 + 1e-5 |x|) around the float64 log-sum-exp restatement, their -inf and fill slots bit-equal.

Inputs, all seeded: (a) values on a 1/4 grid (ties everywhere, the cut included - see grid(), asserted below; the only family of the raw-logit
index checks: grid values stay distinct, and equal ones equal, after one log-sum-exp is subtracted from the whole row), (b) continuous
values (log-prob entries only), (c) edge rows: entries at -inf, a constant row, a row of -inf only (log-prob entries), running
log-probs holding -inf and -1e20.  Every step call holds an ended beam (row G - 2) and a dead beam (-1e20, row G - 1); the grid and
continuous calls also hold a duplicated beam (rows 0 and 1), the edge calls a live beam whose row is one finite constant (row 1,
asserted on the CPU: edge_roles).  The end token, the (beam, per_node) widths, the machine and the input family turn
independently of each other, and the turn starts elsewhere for every V (turn()).

No NaN anywhere: NaN scores are outside the selection's contract (no candidate ranks `after` the previous pick or `better` than
none, a round then finds nothing and beam_merge_kernel would read sidx[-1]), so the tests do not feed any."""
import ctypes as C

import numpy as np
import pytest
import torch

import cbsref as R
from ssc_runtime import lib as L
from ssc_runtime.decode import CompiledFsm

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL = -1
SV, SI = F(-7777.0), -99          # what an output holds before the call
REG_MAX = 10240                   # 256 * BEAM_ROW_NV
ERRS = {}                         # group -> largest error / bound of the raw-logit value checks


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(ERRS):
        print(f"\n[beam-select] largest error/bound, {k}: {ERRS[k]:.4f}")


def _note(group, got, want):
    e = R.err_over_bound(got, want)
    ERRS[group] = max(ERRS.get(group, 0.0), e)
    print(f"[beam-select] {group}: error/bound {e:.4f}")
    assert e <= 1.0, (group, e)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def grid(rng, shape, cut=3):
    """Values on a 1/4 grid.  Equal values are everywhere, but at the very top of a row they thin out (about four rows in ten tie
    across a cut of 3 at V = 63), so every row of more than `cut` tokens also gets its cut-th best value planted on one more
    token, of random position outside the best `cut`: the cut itself is tied in every unmasked row."""
    x = (np.round(rng.standard_normal(shape) * 1.5 * 4) / 4).astype(F)
    if x.ndim == 2 and x.shape[1] > cut:
        for r in x:
            o = np.argsort(-r, kind="stable")
            r[o[rng.integers(cut, r.size)]] = r[o[cut - 1]]
    return x


def cont(rng, shape):
    return (rng.standard_normal(shape) * 3).astype(F)


def edge(rng, shape, norm):
    """Row 0 holds entries at -inf, row 1 is one finite constant, row 3 (log-prob entries only) is -inf everywhere.  In a step
    call rows 0 and 1 are live beams with finite running log-probs and row 3 is a beam at -1e20 whose row is still read (beams())."""
    x = grid(rng, shape)
    rows, V = shape
    x[0, rng.random(V) < 0.3] = -np.inf
    if norm and not np.isfinite(x[0]).any():
        x[0, V - 1] = F(0.5)
    if rows > 1:
        x[1] = F(-2.5)
    if rows > 3 and not norm:
        x[3] = -np.inf
    return x


def edge_roles(x, last_pred, last_lp, end, norm):
    """CPU check of an edge call: a live beam with a finite running log-prob whose row is one finite constant, a live row with
    entries at -inf, and (log-prob entries) a row of -inf only that is not the ended beam's."""
    tok, ll = last_pred.reshape(-1), last_lp.reshape(-1)
    live = (tok != end) & np.isfinite(ll) & (ll > -1e19)
    const = np.isfinite(x[:, 0]) & (x == x[:, :1]).all(1)
    assert (live & const).any()
    assert (live & np.isinf(x).any(1) & np.isfinite(x).any(1)).any() or x.shape[1] < 8
    if not norm:
        assert ((tok != end) & np.isinf(x).all(1)).any()
    assert np.isinf(ll).any() or ll.size < 5


def scores(fam, rng, shape, norm, cut=3):
    return grid(rng, shape, cut) if fam == "grid" else cont(rng, shape) if fam == "cont" else edge(rng, shape, norm)


def beams(fam, rng, B, S, beam, V, end):
    """last_pred (B, S, beam) and last_lp: the row before last has ended, the last one is dead, row 1 repeats row 0's log-prob;
    edge family with 5 rows or more: rows 2 and 3 at -inf and -1e20."""
    G = B * S * beam
    tok = rng.integers(0, V, G)
    tok[tok == end] = (end + 1) % V if V > 1 else 7     # (a one-token vocabulary: any other id; a beam's last token is only compared)
    ll = -np.abs(cont(rng, G) if fam == "cont" else grid(rng, G))
    if G >= 2:
        tok[G - 2] = end
    if G >= 3:
        ll[G - 1] = F(-1e20)
    if G >= 4:
        ll[1] = ll[0]
    if fam == "edge" and G >= 5:
        ll[2] = -np.inf
        ll[3] = F(-1e20)
    return tok.reshape(B, S, beam).astype(np.int64), ll.reshape(B, S, beam).astype(F)


def dense_machine(rng, M, S, V, density):
    fsm = (rng.random((M, S, S, V)) < density).astype(np.uint8)
    if density < 0.5 and S > 1:
        fsm[0, 0, 1] = 0                          # a target with no admitted token
        fsm[0, 1, 2] = 0
        fsm[0, 1, 2, V // 2] = 1                  # and one with a single one: fewer than any per_node used here
    return fsm


def ties_at_cut(x, cut):
    """how many rows of (rows, V) have equal values on both sides of the cut after `cut` entries of the descending order."""
    if x.shape[1] <= cut:
        return 0
    s = -np.sort(-x, axis=1, kind="stable")
    return int((s[:, cut - 1] == s[:, cut]).sum())


# ---- the entries ----------------------------------------------------------------------------------------------------------------------
def padded(x, pad=3):
    """rows with a leading dimension above V; a kernel that reads past V meets 1e30."""
    buf = np.full((x.shape[0], x.shape[1] + pad), 1e30, dtype=F)
    buf[:, :x.shape[1]] = x
    return dev(buf)


def run_first(x, fsm, beam, norm, desc=False, mach=None):
    lib = L.load()
    B, V = x.shape
    S = 1 if fsm is None else fsm.shape[1]
    d_x = padded(x)
    d_fsm = None if fsm is None else dev(fsm)
    d_mach = None if mach is None else dev(np.asarray(mach, dtype=np.int32))
    pred = torch.full((B, S, beam), SI, dtype=torch.int64, device="cuda")
    out = torch.full((B, S, beam), float(SV), device="cuda")
    if desc:
        d = L.BeamDesc()
        d.scores, d.ld, d.raw_logits, d.fsm, d.mach = L.ptr(d_x), d_x.stride(0), int(norm), L.ptr(d_fsm), L.ptr(d_mach)
        d.dims = L.FsmDims(1 if fsm is None else fsm.shape[0], S, V, 0, 1)
        d.B, d.beam, d.pred, d.lp_out = B, beam, L.ptr(pred), L.ptr(out)
        rc = lib._raw_ssc_beam_first_fsm(C.byref(d), L.stream_ptr())
    else:
        fn = lib._raw_ssc_beam_first_logits if norm else lib._raw_ssc_beam_first
        rc = fn(L.ptr(d_x), d_x.stride(0), L.ptr(d_fsm), B, S, V, beam, L.ptr(pred), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, pred.cpu().numpy(), out.cpu().numpy()


class Step:
    """One later step on the device.  entry: "plain" (ssc_beam_step / ssc_beam_step_logits), "desc" (ssc_beam_step_fsm; comp: a
    CompiledFsm for the compiled form) or "parts" (ssc_beam_step_parts from records)."""

    def __init__(self, x, fsm, last_pred, last_lp, end, per_node, norm, entry="desc", comp=None, mach=None, skip_dead=0, ctl=None,
                 step_index=0, max_steps=0, parts=None, V=None, S=None, d_fsm=None):
        lib = L.load()
        B, S0, beam = last_pred.shape
        S = S0 if S is None else S
        V = x.shape[1] if V is None else V
        n = B * S * S * beam * per_node
        self.sval = torch.full((n,), float(SV), device="cuda")
        self.sidx = torch.full((n,), SI, dtype=torch.int64, device="cuda")
        self.pred = torch.full((B, S, beam), SI, dtype=torch.int64, device="cuda")
        self.out = torch.full((B, S, beam), float(SV), device="cuda")
        self.back = torch.full((B, S, beam), SI, dtype=torch.int64, device="cuda")
        d_x = padded(x) if x is not None else None
        if d_fsm is None and fsm is not None:
            d_fsm = dev(fsm)
        d_mach = None if mach is None else dev(np.asarray(mach, dtype=np.int32))
        d_lp, d_ll = dev(last_pred), dev(last_lp)
        d_ctl = None if ctl is None else dev(np.asarray(ctl, dtype=np.int32))
        d_parts = None if parts is None else dev(parts)
        st = L.stream_ptr()
        if entry == "plain":
            assert comp is None and mach is None and ctl is None and not skip_dead
            fn = lib._raw_ssc_beam_step_logits if norm else lib._raw_ssc_beam_step
            self.rc = fn(L.ptr(d_x), d_x.stride(0), L.ptr(d_fsm), L.ptr(d_lp), L.ptr(d_ll), B, S, V, beam, per_node, end, L.ptr(self.pred),
                         L.ptr(self.out), L.ptr(self.back), L.ptr(self.sval), L.ptr(self.sidx), st)
        else:
            d = L.BeamDesc()
            if d_x is not None:
                d.scores, d.ld = L.ptr(d_x), d_x.stride(0)
            d.raw_logits, d.fsm, d.mach = int(norm), L.ptr(d_fsm), L.ptr(d_mach)
            d.tables = L.ptr(comp.tables) if comp is not None else None
            d.dims = comp.dims if comp is not None else L.FsmDims(1 if fsm is None else fsm.shape[0], S, V, 0, 1)
            d.B, d.beam, d.per_node, d.end_index = B, beam, per_node, end
            d.last_pred, d.last_lp, d.pred, d.lp_out, d.backptr = L.ptr(d_lp), L.ptr(d_ll), L.ptr(self.pred), L.ptr(self.out), L.ptr(self.back)
            d.scratch_val, d.scratch_idx, d.skip_dead = L.ptr(self.sval), L.ptr(self.sidx), int(skip_dead)
            d.ctl, d.step_index, d.max_steps = L.ptr(d_ctl), step_index, max_steps
            if entry == "parts":
                self.rc = lib._raw_ssc_beam_step_parts(C.byref(d), L.ptr(d_parts), st)
            else:
                self.rc = lib._raw_ssc_beam_step_fsm(C.byref(d), st)
        torch.cuda.synchronize()
        self.sval, self.sidx = self.sval.cpu().numpy(), self.sidx.cpu().numpy()
        self.pred, self.out, self.back = self.pred.cpu().numpy(), self.out.cpu().numpy(), self.back.cpu().numpy()
        self.ctl = None if d_ctl is None else d_ctl.cpu().numpy()
        self.dims = (B, S, beam, per_node)
        self._ll = last_lp

    def untouched(self):
        return bool((self.sval == SV).all() and (self.sidx == SI).all() and (self.pred == SI).all() and (self.out == SV).all()
                    and (self.back == SI).all())

    def check(self, want_v, want_i, norm, group, what):
        """rows stage against the restatement's (want_v, want_i); merge stage against cbsref.merge of the device's own scratch."""
        B, S, beam, per_node = self.dims
        assert self.rc == 0, (what, self.rc)
        assert np.array_equal(self.sidx, want_i.reshape(-1)), (what, "scratch_idx")
        if norm:
            _note(group, self.sval, want_v)
        else:
            assert _bits(self.sval, want_v.reshape(-1)), (what, "scratch_val")
        return self.check_merge(what)

    def check_merge(self, what, last_lp=None):
        B, S, beam, per_node = self.dims
        p, l, bp = R.merge(self.sval, self.sidx, self._ll if last_lp is None else last_lp, S, beam, per_node)
        assert np.array_equal(self.pred, p), (what, "pred")
        assert np.array_equal(self.back, bp), (what, "backptr")
        assert _bits(self.out, l), (what, "lp_out")
        return self


ALL_V = [2, 63, 64, 65, 255, 256, 257, 10240, 10241, 16384, 16385]


def ends_for(V):
    return sorted({e for e in (0, 1, 300, V - 1) if e < V})


WIDTHS = [(3, 3), (2, 3), (3, 2)]   # (beam, per_node) in turn: a back-pointer is c // per_node, not c // beam


def turn(V, ends, family, machine, extra=0):
    """(end_index, (beam, per_node)) of a call, from the positions of its input family and its machine in their loops: for one
    machine the families walk through every end token and every width pair, with different strides (1 and 2), and the walk
    starts elsewhere for every V, so that no machine, family or `extra` switch is tied to one end token or one width pair."""
    start = ALL_V.index(V) if V in ALL_V else V
    return ends[(start + family + machine) % len(ends)], WIDTHS[(start + 2 * family + machine + extra) % len(WIDTHS)]


def combos():
    """(family, raw logits?) of the dense tests: the continuous family feeds the log-prob entries only."""
    return [("grid", 0), ("grid", 1), ("cont", 0), ("edge", 0), ("edge", 1)]


# ---- the first step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", ALL_V)
def test_first_step_against_the_restatement(V):
    """ssc_beam_first / ssc_beam_first_logits / ssc_beam_first_fsm: the one-state machine and dense machines of density 0.9 / 0.1
    (0.1: state 1 is not reachable from state 0 - fewer admitted tokens than beams, all slots -inf in ascending token order)."""
    rng = np.random.default_rng(1000 + V)
    B, beam = 2, min(3, V)
    tied = rows = 0
    for fam, norm in combos():
        for density in (None, 0.9, 0.1):
            x = scores(fam, rng, (B, V), norm)
            fsm = None if density is None else dense_machine(rng, B, 3, V, density)
            want_p, want_l = R.first(x, fsm, beam, norm=bool(norm))
            if fam == "grid" and fsm is None:
                tied, rows = tied + ties_at_cut(x, beam), rows + B
            for desc in (False, True):
                rc, p, l = run_first(x, fsm, beam, norm, desc=desc)
                what = (V, fam, norm, density, desc)
                assert rc == 0, what
                assert np.array_equal(p, want_p), what
                if norm:
                    _note("first step, raw logits", l, want_l)
                else:
                    assert _bits(l, want_l), what
    if V >= 63:
        assert 2 * tied >= rows, (tied, rows)   # the grid rows do tie across the cut (V = 2 has no cut to straddle with 2 beams)
    # one machine shared by both entries through the index list
    x = grid(rng, (B, V))
    fsm = dense_machine(rng, 2, 3, V, 0.9)
    rc, p, l = run_first(x, fsm, beam, 0, desc=True, mach=[1, 1])
    want_p, want_l = R.first(x, fsm, beam, mach=[1, 1])
    assert rc == 0 and np.array_equal(p, want_p) and _bits(l, want_l)


# ---- later steps, dense machine ---------------------------------------------------------------------------------------------------------
def _dense_case(V, reg):
    lib = L.load()
    rng = np.random.default_rng(2000 + V + reg)
    B = 2
    ends = ends_for(V)
    tied = rows = 0
    seen = set()
    prev = C.c_int(1)
    lib.ssc_debug_get(b"beam_reg", C.byref(prev))
    lib.ssc_debug_set(b"beam_reg", reg)
    try:
        for ci, (fam, norm) in enumerate(combos()):
            for di, density in enumerate((None, 0.9, 0.1)):
                S = 1 if density is None else 3
                end, widths = turn(V, ends, ci, di, reg)
                beam, per_node = (min(w, V) for w in widths)
                seen |= {(di, "end", end), (di, "widths", widths)}
                x = scores(fam, rng, (B * S * beam, V), norm, cut=per_node)
                fsm = None if density is None else dense_machine(rng, B, S, V, density)
                last_pred, last_lp = beams(fam, rng, B, S, beam, V, end)
                if fam == "edge":
                    edge_roles(x, last_pred, last_lp, end, norm)
                else:
                    x[1] = x[0]      # the duplicated beam: same row, same running log-prob
                want_v, want_i = R.rows(x, fsm, last_pred, end, per_node, norm=bool(norm))
                if density == 0.1 and V >= 63:
                    admitted = fsm.sum(-1)
                    assert (admitted == 0).any() and ((admitted > 0) & (admitted < per_node)).any()
                if fam == "grid":
                    tied, rows = tied + ties_at_cut(x, per_node), rows + x.shape[0]
                group = "step, dense machine, raw logits"
                for entry in ("plain", "desc"):
                    Step(x, fsm, last_pred, last_lp, end, per_node, norm, entry=entry).check(want_v, want_i, norm, group,
                                                                                              (V, reg, fam, norm, density, end, entry))
    finally:
        lib.ssc_debug_set(b"beam_reg", prev.value)
    # every machine met every end token and every width pair
    assert len(seen) == 3 * (len(ends) + len(WIDTHS)), sorted(seen)
    if V >= 63:
        assert 2 * tied >= rows, (tied, rows)


@pytest.mark.parametrize("V", ALL_V)
def test_step_with_dense_machines_against_the_restatement(V):
    """ssc_beam_step, ssc_beam_step_logits and ssc_beam_step_fsm without tables: register form up to V = 10240, then the plain /
    LDS-staged form, then (raw logits above 16384) the row read from memory; end_index over {0, 1, 300, V - 1}."""
    _dense_case(V, 1)


@pytest.mark.parametrize("V", [v for v in ALL_V if v <= REG_MAX])
def test_step_with_dense_machines_without_the_register_form(V):
    _dense_case(V, 0)


def test_merge_with_more_candidates_than_lanes():
    """S * beam * per_node = 3 * 5 * 5 = 75 candidates per target: a lane of the merge's one wave holds two."""
    rng = np.random.default_rng(75)
    B, S, beam, per_node, V, end = 2, 3, 5, 5, 63, 1
    for fam in ("grid", "cont", "edge"):
        x = scores(fam, rng, (B * S * beam, V), 0)
        fsm = dense_machine(rng, B, S, V, 0.9)
        last_pred, last_lp = beams(fam, rng, B, S, beam, V, end)
        want_v, want_i = R.rows(x, fsm, last_pred, end, per_node)
        s = Step(x, fsm, last_pred, last_lp, end, per_node, 0).check(want_v, want_i, 0, "", fam)
        if fam == "grid":   # keys on the grid: the merge's own cut is tied
            key = (s.sval.reshape(B, S, S * beam, per_node) + last_lp.reshape(B, 1, S * beam, 1)).reshape(B * S, -1)
            assert ties_at_cut(key, beam) >= B * S // 2


# ---- later steps, compiled machine --------------------------------------------------------------------------------------------------------
def hand_machine(V):
    """Three states.  From 0: every token loops (default set {0}) but tokens 0, 1, 2, 5, which lead to state 1 - a reachable target
    OUTSIDE the default set whose fills must skip those lowest ids -, and state 2 cannot be reached at all.  From 1: default {1},
    tokens 3 and 7 lead to 2, token 4 to 0 and 2.  From 2: every token stays; 0 and 1 are unreachable."""
    fsm = np.zeros((1, 3, 3, V), dtype=np.uint8)
    fsm[0, 0, 0] = 1
    fsm[0, 0, 0, [0, 1, 2, 5]] = 0
    fsm[0, 0, 1, [0, 1, 2, 5]] = 1
    fsm[0, 1, 1] = 1
    fsm[0, 1, 1, [3, 4, 7]] = 0
    fsm[0, 1, 2, [3, 4, 7]] = 1
    fsm[0, 1, 0, 4] = 1
    fsm[0, 2, 2] = 1
    return fsm


def sparse_machine(rng, M, S, V, nexc):
    """Per from-state one default target set and `nexc` exception tokens with random target sets (token 0 among them)."""
    fsm = np.zeros((M, S, S, V), dtype=np.uint8)
    for m in range(M):
        for s in range(S):
            fsm[m, s, :, :] = (rng.random(S) < 0.6).astype(np.uint8)[:, None]
            tok = np.unique(np.concatenate([[0], rng.integers(0, V, nexc)]))
            fsm[m, s][:, tok] = (rng.random((S, tok.size)) < 0.5).astype(np.uint8)
    return fsm


@pytest.mark.parametrize("V", [63, 257, 10240, 10241])
def test_step_with_compiled_machines_against_the_restatement(V):
    """ssc_fsm_compile + ssc_beam_step_fsm, row in registers (V <= 10240) and not: a capacity that compiles every from-state, E = 0
    (the dense scans inside the compiled launch), the hand-made machine, skip_dead with garbage in the dead row, shared machines."""
    rng = np.random.default_rng(3000 + V)
    B, S = 2, 3
    ends = ends_for(V)
    seen = set()
    small = V <= 512
    machines = [("hand", hand_machine(V), [0, 0], 16, True),
                ("random, compiled", dense_machine(rng, 2, S, V, 0.9) if small else sparse_machine(rng, 2, S, V, 150), None, V if small else 512, True),
                ("random, E = 0", dense_machine(rng, 2, S, V, 0.1 if small else 0.9), [1, 0], 0, False),
                ("shared", sparse_machine(rng, 1, S, V, 20), [0, 0], 64, True)]
    for mi, (name, fsm, mach, E, compiled) in enumerate(machines):
        d_fsm = dev(fsm)
        comp = CompiledFsm(d_fsm, max_exceptions=E, fill=8)
        ok = comp.sparse_states().cpu().numpy()
        assert ok.all() if compiled else not ok.any(), (name, ok)
        if name == "hand":
            reach = fsm[0].any(-1)     # (from, target)
            assert not reach[0, 2] and reach[0, 1] and not fsm[0, 0, 1, 3:5].any()
        for ci, (fam, norm) in enumerate(combos()):
            for skip_dead in (0, 1):
                end, (beam, per_node) = turn(V, ends, ci, mi, skip_dead)
                seen |= {(mi, "end", end), (mi, "widths", (beam, per_node))}
                x = scores(fam, rng, (B * S * beam, V), norm, cut=per_node)
                last_pred, last_lp = beams(fam, rng, B, S, beam, V, end)
                if name == "hand":   # an ended beam in from-state 0 (entry 1, beam 0): see below
                    last_pred[1, 0, 0] = end
                if fam == "edge":
                    edge_roles(x, last_pred, last_lp, end, norm)
                else:
                    x[1] = x[0]
                if skip_dead:      # what a skipped decode step leaves behind: large finite garbage, never read
                    dead = (last_lp.reshape(-1) <= -1e19) & (last_pred.reshape(-1) != end)
                    assert dead.any()
                    x[dead] = (rng.choice([-3e38, 3e38, 1e30], (int(dead.sum()), V))).astype(F)
                want_v, want_i = R.rows(x, fsm, last_pred, end, per_node, last_lp=last_lp, skip_dead=bool(skip_dead), mach=mach,
                                        norm=bool(norm))
                if name == "hand":
                    # target 1 from state 0 admits tokens 0, 1, 2, 5 only and lies outside the default set: an ended beam there is
                    # worth -inf (or 0 at END) on those four and -1e20 on every other token, so its list holds fills, and the
                    # fills are the lowest ids that are NOT among the four
                    got = want_i[1, 1, 0, 0].tolist()
                    fills = [v for v in got if v not in (0, 1, 2, 5)]
                    assert fills == [3, 4, 6][:len(fills)] and len(fills) >= per_node - 1, got
                Step(x, fsm, last_pred, last_lp, end, per_node, norm, comp=comp, mach=mach, skip_dead=skip_dead, d_fsm=comp.fsm).check(
                    want_v, want_i, norm, "step, compiled machine, raw logits", (V, name, fam, norm, skip_dead, end))
    assert len(seen) == len(machines) * (len(ends) + len(WIDTHS)), sorted(seen)


# ---- later steps from records -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 127, 128, 129, 10000])
def test_step_from_records_against_the_restatement(V):
    """ssc_beam_step_parts from cbsref.records of grid and continuous rows: G = B * beam in {1, 3, 4, 5} (the last workgroup of four
    waves holds idle ones), per_node 1 and 2, ended rows with end_index 0 and 1."""
    rng = np.random.default_rng(4000 + V)
    for B, beam in ((1, 1), (1, 3), (2, 2), (1, 5)):
        for per_node in (1, 2):
            for fam in ("grid", "cont"):
                for end in (0, 1):
                    if end >= V:
                        continue
                    x = scores(fam, rng, (B * beam, V), 1, cut=per_node)
                    last_pred, last_lp = beams(fam, rng, B, 1, beam, V, end)
                    parts = R.records(x)
                    s = Step(None, None, last_pred, last_lp, end, per_node, 1, entry="parts", parts=parts, V=V)
                    what = (V, B, beam, per_node, fam, end)
                    if per_node > V:    # a one-token vocabulary has no second candidate
                        assert s.rc == EINVAL and s.untouched(), what
                        continue
                    want_v, want_i = R.rows_from_records(parts, V, last_pred, end, per_node)
                    s.check(want_v, want_i, 1, "step from records", what)
                    # and the records entry selects what the logits entries select: same tokens, values within the statement
                    full_v, full_i = R.rows(x, None, last_pred, end, per_node, norm=True)
                    assert np.array_equal(want_i, full_i), what
                    _note("step from records, against the logits restatement", s.sval, full_v)


def test_step_from_records_refuses_what_it_cannot_do():
    rng = np.random.default_rng(5)
    B, beam, V, end = 2, 2, 129, 1
    x = grid(rng, (B * beam, V))
    parts = R.records(x)
    last_pred, last_lp = beams("grid", rng, B, 1, beam, V, end)
    ok = Step(None, None, last_pred, last_lp, end, 2, 1, entry="parts", parts=parts, V=V)
    assert ok.rc == 0 and not ok.untouched()
    s = Step(None, None, last_pred, last_lp, end, 3, 1, entry="parts", parts=parts, V=V)                      # per_node = 3
    assert s.rc == EINVAL and s.untouched()
    lp3, ll3 = beams("grid", rng, B, 3, beam, V, end)
    s = Step(None, None, lp3, ll3, end, 2, 1, entry="parts", parts=np.concatenate([parts] * 3), V=V)          # S = 3
    assert s.rc == EINVAL and s.untouched()
    fsm = np.ones((B, 1, 1, V), dtype=np.uint8)
    s = Step(None, fsm, last_pred, last_lp, end, 2, 1, entry="parts", parts=parts, V=V)                       # a machine
    assert s.rc == EINVAL and s.untouched()
    comp = CompiledFsm(dev(fsm), max_exceptions=8, fill=8)
    s = Step(None, None, last_pred, last_lp, end, 2, 1, entry="parts", parts=parts, V=V, comp=comp)           # tables
    assert s.rc == EINVAL and s.untouched()


# ---- the early stop -------------------------------------------------------------------------------------------------------------------
def test_stopped_and_stopping_steps():
    """ssc_beam_desc.ctl: a step at or after ctl[0] re-emits END from the same beam (cbsref.merge_stopped); a step in which every
    beam of the call ends leaves ctl[0] = step_index + 1; one live beam leaves it alone."""
    rng = np.random.default_rng(6)
    B, S, beam, per_node, V, end, max_steps = 2, 3, 2, 2, 65, 1, 8
    fsm = dense_machine(rng, B, S, V, 0.9)
    x = grid(rng, (B * S * beam, V))
    last_pred, last_lp = beams("grid", rng, B, S, beam, V, end)
    for ctl0, si in ((2, 3), (3, 3)):
        ctl = np.zeros(2 + 2 * max_steps, dtype=np.int32)
        ctl[0] = ctl0
        s = Step(x, fsm, last_pred, last_lp, end, per_node, 0, ctl=ctl, step_index=si, max_steps=max_steps)
        p, l, bp = R.merge_stopped(last_lp, S, beam, end)
        assert s.rc == 0 and np.array_equal(s.pred, p) and np.array_equal(s.back, bp) and _bits(s.out, l)
        assert s.ctl[0] == ctl0 and s.ctl[2 + si] == 0 and s.ctl[2 + max_steps + si] == B * S
    # every beam ends: END is admitted everywhere and far above every other token
    fsm1 = np.ones((B, S, S, V), dtype=np.uint8)
    x_end = (grid(rng, (B * S * beam, V)) - F(60)).astype(F)
    x_end[:, end] = F(0)
    ll = -np.abs(grid(rng, (B, S, beam))) - F(1)
    ll.reshape(-1)[3] = F(-0.5)       # the best running log-prob of its group
    for live in (0, 1):
        xx = x_end.copy()
        if live:
            xx[3, end] = F(-200)          # one row whose best tokens are not END: its candidates still win a slot of its group
            xx[3, 7] = F(0)
        lp_ = last_pred.copy()
        lp_[lp_ == end] = 5
        ctl = np.zeros(2 + 2 * max_steps, dtype=np.int32)
        ctl[0] = max_steps
        s = Step(xx, fsm1, lp_, ll, end, per_node, 0, ctl=ctl, step_index=4, max_steps=max_steps)
        want_v, want_i = R.rows(xx, fsm1, lp_, end, per_node)
        s.check(want_v, want_i, 0, "", ("ctl", live))
        assert bool((s.pred == end).all()) == (not live)
        assert s.ctl[0] == R.ctl_after(max_steps, s.pred, end, 4) == (max_steps if live else 5)
        assert s.ctl[2 + 4] == int((s.pred != end).sum()) and s.ctl[2 + max_steps + 4] == B * S


# ---- back-trace and row gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 9])
def test_backtrace_against_the_restatement(steps):
    lib = L.load()
    rng = np.random.default_rng(7 + steps)
    for B, SB in ((1, 1), (1, 63), (2, 32), (5, 13), (2, 65)):          # B * SB = 1, 63, 64, 65, 130
        preds = rng.integers(0, 1000, (steps, B, SB)).astype(np.int64)
        backs = rng.integers(0, SB, (max(steps - 1, 1), B, SB)).astype(np.int64)
        d_p, d_b = dev(preds), dev(backs)
        out = torch.full((B, SB, steps), SI, dtype=torch.int64, device="cuda")
        rc = lib._raw_ssc_beam_backtrace(L.ptr(d_p), L.ptr(d_b) if steps > 1 else None, steps, B, SB, L.ptr(out), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(out.cpu().numpy(), R.backtrace(preds, backs if steps > 1 else None)), (B, SB)
        for ctl0 in sorted({0, 1, 4, steps, steps + 3}):
            d_ctl = dev(np.array([ctl0, 0], dtype=np.int32))
            out = torch.full((B, SB, steps), SI, dtype=torch.int64, device="cuda")
            rc = lib._raw_ssc_beam_backtrace_ctl(L.ptr(d_p), L.ptr(d_b) if steps > 1 else None, L.ptr(d_ctl), steps, B, SB, 3, L.ptr(out),
                                                 L.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0 and np.array_equal(out.cpu().numpy(), R.backtrace_ctl(preds, backs, ctl0, steps, 3)), (B, SB, ctl0)


@pytest.mark.parametrize("Wd", [1, 255, 256, 257])
def test_gather_rows_against_the_restatement(Wd):
    lib = L.load()
    rng = np.random.default_rng(8 + Wd)
    B, rpb, ld = 3, 5, Wd + 5
    src = cont(rng, (B * rpb, ld))
    bp = rng.integers(0, rpb, B * rpb).astype(np.int64)
    d_src, d_bp = dev(src), dev(bp)
    dst = torch.full((B * rpb, ld), float(SV), device="cuda")
    rc = lib._raw_ssc_gather_rows(L.ptr(d_src), ld, L.ptr(d_bp), B, rpb, Wd, L.ptr(dst), L.stream_ptr())
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert rc == 0 and _bits(got[:, :Wd], R.gather_rows(src, bp, rpb)[:, :Wd])
    assert bool((got[:, Wd:] == SV).all())                           # the padding columns are not written
    before = d_src.clone()
    assert lib._raw_ssc_gather_rows(L.ptr(d_src), ld, L.ptr(d_bp), B, rpb, Wd, L.ptr(d_src), L.stream_ptr()) == EINVAL   # in place
    torch.cuda.synchronize()
    assert torch.equal(before, d_src)


def test_gather_rows_refuses_more_rows_than_the_grid_holds():
    """The rows sit on the grid's second dimension: 65535 of them are served, 65536 are SSC_EINVAL before any launch."""
    lib = L.load()
    rng = np.random.default_rng(9)
    for rows, want_rc in ((65535, 0), (65536, EINVAL)):
        rpb = rows // 257 if rows % 257 == 0 else (rows // 256 if rows % 256 == 0 else 1)
        B = rows // rpb
        assert B * rpb == rows
        src = cont(rng, (rows, 1))
        bp = rng.integers(0, rpb, rows).astype(np.int64)
        d_src, d_bp = dev(src), dev(bp)
        dst = torch.full((rows, 1), float(SV), device="cuda")
        rc = lib._raw_ssc_gather_rows(L.ptr(d_src), 1, L.ptr(d_bp), B, rpb, 1, L.ptr(dst), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want_rc, rows
        got = dst.cpu().numpy()
        assert _bits(got, R.gather_rows(src, bp, rpb)) if rc == 0 else bool((got == SV).all())
