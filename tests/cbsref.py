"""One step of the constrained / plain beam search (ssc_beam_first*, ssc_beam_step*, ssc_beam_step_fsm, ssc_beam_step_parts,
ssc_beam_backtrace*, ssc_gather_rows of include/ssc.h; cbs.py:127-277 of the reference) restated in plain numpy: float32 values,
int64 indices, no torch, no device.  Every selection is "value descending, index ascending" and is made here by ONE stable sort of
the whole masked row (or of the whole candidate list), not by the k rounds of the kernels.

Shapes: B batch entries, S machine states, `beam` beams per (entry, state), rows g = (b, s, k) flattened, V tokens.
  fsm (M, S, S, V) uint8: fsm[m, s, i, v] != 0 <-> token v leads from state s to state i; None: the one-state machine.
  mach (B,) machine of every entry, or None: machine b.
  scratch layout of the rows stage: (b, i, s, k, n), i the TARGET state, n < per_node.
Values: a masked token of the first step is worth -inf; of a later step -1e20f (larger than -inf: an ended beam's forbidden tokens
rank before its allowed non-END ones, as in cbs.py:177-206 where the mask is applied after the forced end)."""
import numpy as np

F = np.float32
FILL = F(-1e20)
NEG = F(-np.inf)


def top_by(x, n):
    """indices of the n first of x (1-d) in the order value descending, index ascending."""
    return np.argsort(-np.asarray(x), kind="stable")[:n]


def lse64(x):
    """float64 log-sum-exp of every row of (rows, V); a row of -inf only gives -inf."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(x - m).sum(1, keepdims=True)))[:, 0]


def log_probs(x):
    """(rows, V) raw logits -> float32 log-probs: the row's log-sum-exp in float64, x - lse rounded to float32 once."""
    x = np.asarray(x, dtype=F)
    return (x.astype(np.float64) - lse64(x)[:, None]).astype(F)


def _dims(fsm):
    if fsm is None:
        return 1
    fsm = np.asarray(fsm)
    assert fsm.ndim == 4 and fsm.shape[1] == fsm.shape[2]
    return fsm.shape[1]


def _mask(fsm, mach, b, s, i, V):
    if fsm is None:
        return np.ones(V, dtype=bool)
    return np.asarray(fsm)[b if mach is None else int(mach[b]), s, i] != 0


def first(lp, fsm, beam, mach=None, norm=False):
    """First step from (B, V) scores -> pred (B, S, beam) int64, lp_out (B, S, beam) float32: per (b, state s) the `beam` best
    tokens of the row with every token that does not lead from state 0 to s at -inf.  norm: `lp` holds raw logits (log_probs)."""
    lp = log_probs(lp) if norm else np.asarray(lp, dtype=F)
    B, V = lp.shape
    S = _dims(fsm)
    pred = np.zeros((B, S, beam), dtype=np.int64)
    out = np.zeros((B, S, beam), dtype=F)
    for b in range(B):
        for s in range(S):
            y = np.where(_mask(fsm, mach, b, 0, s, V), lp[b], NEG)
            o = top_by(y, beam)
            pred[b, s], out[b, s] = o, y[o]
    return pred, out


def ended_row(V, end_index):
    x = np.full(V, NEG, dtype=F)
    x[end_index] = F(0)
    return x


def rows(lp, fsm, last_pred, end_index, per_node, last_lp=None, skip_dead=False, mach=None, norm=False):
    """Rows stage of a later step.  lp (B*S*beam, V) scores, last_pred (B, S, beam) -> sval float32, sidx int64, both
    (B, S, S, beam, per_node) in the scratch layout (b, i, s, k, n): per row and TARGET state i the per_node best tokens of the
    cleaned, masked row.  Cleaned: an ended beam's row is 0 at end_index and -inf elsewhere; with skip_dead a row that has not
    ended and has last_lp <= -1e19 is all zeros; any other row is lp (norm: log_probs(lp)).  Masked: -1e20f."""
    last_pred = np.asarray(last_pred)
    B, S, beam = last_pred.shape
    assert S == _dims(fsm)
    lp = np.asarray(lp, dtype=F)
    G, V = lp.shape
    assert G == B * S * beam and per_node <= V
    ended = last_pred.reshape(G) == end_index
    dead = np.zeros(G, dtype=bool)
    if skip_dead:
        dead = ~ended & (np.asarray(last_lp, dtype=F).reshape(G) <= F(-1e19))
    live = ~ended & ~dead
    x = np.zeros((G, V), dtype=F)
    if live.any():
        x[live] = log_probs(lp[live]) if norm else lp[live]
    x[ended] = ended_row(V, end_index)
    sval = np.zeros((B, S, S, beam, per_node), dtype=F)
    sidx = np.zeros((B, S, S, beam, per_node), dtype=np.int64)
    for b in range(B):
        for s in range(S):
            for i in range(S):
                m = _mask(fsm, mach, b, s, i, V)
                for k in range(beam):
                    y = np.where(m, x[(b * S + s) * beam + k], FILL)
                    o = top_by(y, per_node)
                    sval[b, i, s, k], sidx[b, i, s, k] = y[o], o
    return sval, sidx


def merge(sval, sidx, last_lp, S, beam, per_node):
    """Merge stage: per (b, target state i) the `beam` best of the C = S * beam * per_node candidates c = (s, k, n) by the key
    sval + last_lp[b, c // per_node] (one float32 add), ties to the lower c.  -> pred (B, S, beam) int64, lp_out float32,
    backptr int64 = c // per_node."""
    C = S * beam * per_node
    sval = np.asarray(sval, dtype=F).reshape(-1, S, C)
    sidx = np.asarray(sidx).reshape(-1, S, C)
    B = sval.shape[0]
    ll = np.asarray(last_lp, dtype=F).reshape(B, S * beam)
    pred = np.zeros((B, S, beam), dtype=np.int64)
    out = np.zeros((B, S, beam), dtype=F)
    back = np.zeros((B, S, beam), dtype=np.int64)
    src = np.arange(C) // per_node
    for b in range(B):
        for i in range(S):
            key = sval[b, i] + ll[b][src]          # float32 + float32
            assert key.dtype == F
            o = top_by(key, beam)
            pred[b, i], out[b, i], back[b, i] = sidx[b, i][o], key[o], src[o]
    return pred, out, back


def merge_stopped(last_lp, S, beam, end_index):
    """A step queued after the search had stopped (ctl[0] <= step_index): END from the same beam, nothing moves."""
    ll = np.asarray(last_lp, dtype=F).reshape(-1, S, beam)
    B = ll.shape[0]
    pred = np.full((B, S, beam), end_index, dtype=np.int64)
    back = np.broadcast_to(np.arange(S * beam, dtype=np.int64).reshape(1, S, beam), (B, S, beam)).copy()
    return pred, ll.copy(), back


def ctl_after(ctl0, pred, end_index, step_index):
    """Word 0 of ssc_beam_desc.ctl after a step that was not stopped: step_index + 1 once EVERY beam of the call has ended."""
    return min(ctl0, step_index + 1) if bool((np.asarray(pred) == end_index).all()) else ctl0


def backtrace(preds, backptrs):
    """preds (steps, B, SB), backptrs (steps - 1, B, SB) (None for one step) -> (B, SB, steps): beam j's tokens, followed backwards."""
    preds = np.asarray(preds)
    steps, B, SB = preds.shape
    out = np.zeros((B, SB, steps), dtype=np.int64)
    for b in range(B):
        for j in range(SB):
            idx = j
            for t in range(steps - 1, -1, -1):
                out[b, j, t] = preds[t, b, idx]
                if t > 0:
                    idx = int(backptrs[t - 1][b, idx])
    return out


def backtrace_ctl(preds, backptrs, ctl0, max_steps, end_index):
    """The back-trace of the first n = clamp(ctl0, 1, max_steps) steps; columns >= n hold END.  -> (B, SB, max_steps)."""
    preds = np.asarray(preds)
    n = min(max(int(ctl0), 1), max_steps)
    _, B, SB = preds.shape
    out = np.full((B, SB, max_steps), end_index, dtype=np.int64)
    out[:, :, :n] = backtrace(preds[:n], None if n == 1 else np.asarray(backptrs)[:n - 1])
    return out


def gather_rows(src, backptr, rows_per_batch):
    """dst[b * rpb + r] = src[b * rpb + backptr[b * rpb + r]] (cbs.py:236-250)."""
    src = np.asarray(src)
    bp = np.asarray(backptr).reshape(-1)
    r = np.arange(bp.size)
    return src[r // rows_per_batch * rows_per_batch + bp]


def records(x):
    """(rows, V) float32 -> (rows, ceil(V / 128), 6) float32 in the record layout of ssc_gemm_desc.topk_part: per 128-column tile
    its maximum, sum exp(x - maximum) (summed in float64, rounded once), best value, best column, second-best value, its column;
    the columns as int32 bits in the float; ties to the lower column; a tile of one column: second -inf at column -1."""
    x = np.asarray(x, dtype=F)
    R, V = x.shape
    ntn = (V + 127) // 128
    out = np.zeros((R, ntn, 6), dtype=F)
    col = out.view(np.int32)
    for t in range(ntn):
        tile = x[:, t * 128:min(V, t * 128 + 128)]
        mx = tile.max(1)
        out[:, t, 0] = mx
        with np.errstate(invalid="ignore"):
            e = np.exp(tile.astype(np.float64) - mx[:, None].astype(np.float64))
        out[:, t, 1] = np.where(np.isfinite(mx), e.sum(1), 0.0).astype(F)
        for r in range(R):
            o = top_by(tile[r], 2)
            out[r, t, 2], col[r, t, 3] = tile[r, o[0]], t * 128 + o[0]
            if o.size > 1:
                out[r, t, 4], col[r, t, 5] = tile[r, o[1]], t * 128 + o[1]
            else:
                out[r, t, 4], col[r, t, 5] = NEG, -1
    return out


def records_lse64(parts):
    """float64 log-sum-exp of every row from its tiles' (maximum, sum) pairs."""
    p = np.asarray(parts, dtype=F).astype(np.float64)
    mx = p[:, :, 0].max(1)
    with np.errstate(invalid="ignore"):
        w = np.where(p[:, :, 1] > 0, p[:, :, 1] * np.exp(p[:, :, 0] - mx[:, None]), 0.0)
    return mx + np.log(w.sum(1))


def rows_from_records(parts, V, last_pred, end_index, per_node):
    """`rows` for the one-state machine from records instead of logits: the candidates of a live row are its tiles' best two
    columns, ordered (value descending, column ascending) before the float64 log-sum-exp is subtracted and the difference rounded
    to float32.  last_pred (B, 1, beam) -> sval, sidx (B, 1, 1, beam, per_node)."""
    parts = np.asarray(parts, dtype=F)
    last_pred = np.asarray(last_pred)
    B, S, beam = last_pred.shape
    G = B * beam
    assert S == 1 and parts.shape[0] == G and per_node <= V
    lse = records_lse64(parts)
    col = parts.view(np.int32)
    sval = np.zeros((G, per_node), dtype=F)
    sidx = np.zeros((G, per_node), dtype=np.int64)
    for g in range(G):
        if last_pred.reshape(G)[g] == end_index:
            y = ended_row(V, end_index)
            o = top_by(y, per_node)
            sval[g], sidx[g] = y[o], o
            continue
        v = np.concatenate([parts[g, :, 2], parts[g, :, 4]])
        c = np.concatenate([col[g, :, 3], col[g, :, 5]]).astype(np.int64)
        v, c = v[c >= 0], c[c >= 0]
        o = np.lexsort((c, -v))[:per_node]
        sval[g], sidx[g] = (v[o].astype(np.float64) - lse[g]).astype(F), c[o]
    return sval.reshape(B, 1, 1, beam, per_node), sidx.reshape(B, 1, 1, beam, per_node)


# ---- the project's one tolerance statement for float32 log-probs formed on the device from raw logits ------------------------------
ABS_TOL, REL_TOL = 1e-4, 1e-5


def err_over_bound(got, want):
    """largest |got - want| / (1e-4 + 1e-5 |want|) over the finite entries above the fills; -inf, and the -1e20 fills (sums that
    hold one included), must be the same bits - returns inf where they are not."""
    got, want = np.asarray(got, dtype=F).reshape(-1), np.asarray(want, dtype=F).reshape(-1)
    exact = ~np.isfinite(want) | (want <= F(-1e19))
    if not np.array_equal(got[exact].view(np.int32), want[exact].view(np.int32)):
        return np.inf
    g, w = got[~exact].astype(np.float64), want[~exact].astype(np.float64)
    if g.size == 0:
        return 0.0
    if not np.isfinite(g).all():
        return np.inf
    return float((np.abs(g - w) / (ABS_TOL + REL_TOL * np.abs(w))).max())
