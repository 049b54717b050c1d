"""CPU: tests/cbsref.py (the numpy restatement of one constrained-beam-search step that tests/test_beam_select_gpu.py holds the
kernels to) against two independent things: the oracle's whole search on tie-free inputs (oracle.cbs_search, pinned to the
reference's cbs.py by g12_cbs), and hand-worked tie cases whose expected lists are written out here."""
import numpy as np
import pytest
import torch

import cbsref as R
import oracle

F = np.float32
INF = float("inf")
FILL = float(np.float32(-1e20))


def _search(lp_step, fsm, B, S, beam, per_node, steps, end=1):
    """first / rows / merge / gather_rows / backtrace driven step by step, as ssc_runtime.decode.cbs_search drives the entries."""
    start = torch.full((B,), end, dtype=torch.long)
    lp0, state = lp_step(start, None)
    pred, last_lp = R.first(lp0.numpy(), fsm, beam)
    SB = S * beam
    enlarge = lambda t: t.view(B, 1, 1, -1).expand(B, S, beam, t.size(-1)).reshape(B * SB, -1).numpy().copy()
    state = {k: enlarge(v) for k, v in state.items()}
    preds, backs = [pred.reshape(B, SB)], []
    for _ in range(1, steps):
        last = preds[-1].reshape(B, S, beam)
        lp, new = lp_step(torch.from_numpy(last.reshape(-1)), {k: torch.from_numpy(v) for k, v in state.items()})
        sval, sidx = R.rows(lp.numpy(), fsm, last, end, per_node)
        pred, last_lp, back = R.merge(sval, sidx, last_lp, S, beam, per_node)
        preds.append(pred.reshape(B, SB))
        backs.append(back.reshape(B, SB))
        state = {k: R.gather_rows(v.numpy(), backs[-1], SB) for k, v in new.items()}
    return R.backtrace(np.stack(preds), np.stack(backs)).reshape(B, S, beam, steps), last_lp


@pytest.mark.parametrize("S,V,beam,per_node,density", [(1, 300, 3, 2, 0.9), (3, 300, 3, 2, 0.5), (3, 1000, 2, 3, 0.15), (1, 64, 5, 5, 0.9),
                                                        (3, 64, 3, 1, 0.9)])
def test_restatement_matches_the_oracle_search_on_tie_free_inputs(S, V, beam, per_node, density):
    """Six steps with the step function of test_cbs_search_random_configs_match_oracle (continuous log-probs: no ties among finite
    values): predictions equal on every beam the oracle reaches, log-probs within the project's tolerance statement."""
    B, steps = 2, 6
    g = torch.Generator().manual_seed(V * 31 + S * 7 + beam)
    U = torch.randn(V, 12, generator=g)
    W = torch.randn(12, V, generator=g) * 1.5
    drift = torch.randn(5, V, generator=g) * 0.5
    endb = 2.5 if density > 0.4 else 0.5
    fsm = (torch.rand(B, S, S, V, generator=g) < density).to(torch.uint8)
    fsm[:, :, :, 1] = 1
    fsm[:, :, :, 2:6] = 1

    def step_cpu(tokens, state):
        G = tokens.numel()
        cnt = torch.zeros(G, 1) if state is None else state["cnt"]
        acc = torch.zeros(G, 2) if state is None else state["acc"]
        logits = U[tokens] @ W + drift[cnt.long().view(-1) % 5] + acc.sum(1, keepdim=True) * 0.02
        logits[:, 1] += endb
        new = {"cnt": cnt + 1, "acc": (acc + tokens.view(-1, 1).float() * torch.tensor([[1.0, 0.5]])) % 3.0}
        return torch.log_softmax(logits, dim=1), new

    start = torch.full((B,), 1, dtype=torch.long)
    want_p, want_lp = oracle.cbs_search(start, None, step_cpu, fsm, end_index=1, max_steps=steps, beam_size=beam,
                                        per_node_beam_size=per_node, early_stop=False)
    got_p, got_lp = _search(step_cpu, fsm.numpy(), B, S, beam, per_node, steps)
    assert got_p.shape == tuple(want_p.shape)
    finite = (torch.isfinite(want_lp) & (want_lp > -1e19)).numpy()
    assert finite.any()
    assert np.array_equal(got_p[finite], want_p.numpy()[finite])
    assert R.err_over_bound(got_lp[finite], want_lp.numpy()[finite]) <= 1.0


def _one(lp_row, masks, last_tok, end, per_node, last_lp=None, skip_dead=False):
    """rows() for one beam of one entry in from-state 0 of a machine whose row 0 of targets is `masks` (S, V); other from-states empty."""
    masks = np.asarray(masks, dtype=np.uint8)
    S, V = masks.shape
    fsm = np.zeros((1, S, S, V), dtype=np.uint8)
    fsm[0, 0] = masks
    lp = np.zeros((S, V), dtype=F)
    lp[0] = lp_row
    last = np.full((1, S, 1), last_tok, dtype=np.int64)
    ll = None if last_lp is None else np.full((1, S, 1), last_lp, dtype=F)
    sval, sidx = R.rows(lp, fsm, last, end, per_node, last_lp=ll, skip_dead=skip_dead)
    return [sval[0, i, 0, 0].tolist() for i in range(S)], [sidx[0, i, 0, 0].tolist() for i in range(S)]


def test_a_tie_at_the_cut_goes_to_the_lower_token():
    #       token: 0     1     2     3     4     5     6
    row = [-1.0, -0.5, -2.0, -0.5, -1.0, -0.5, -1.0]
    v, i = _one(row, [[1] * 7], 3, 1, 2)
    assert i == [[1, 3]] and v == [[-0.5, -0.5]]              # three tokens at -0.5: the cut falls between 3 and 5
    v, i = _one(row, [[1] * 7], 3, 1, 4)
    assert i == [[1, 3, 5, 0]] and v == [[-0.5, -0.5, -0.5, -1.0]]   # three tokens at -1.0: only token 0 is taken
    p, l = R.first(np.array([row], dtype=F), None, 5)
    assert p.tolist() == [[[1, 3, 5, 0, 4]]] and l.tolist() == [[[-0.5, -0.5, -0.5, -1.0, -1.0]]]


def test_fills_come_in_ascending_token_order_and_skip_only_admitted_tokens():
    #       token: 0     1     2     3     4     5     6     7
    row = [-3.0, -1.0, -0.25, -2.0, -0.5, -4.0, -0.75, -1.5]
    masks = [[0, 0, 1, 0, 0, 1, 0, 0],      # target 0 admits tokens 2 and 5 only: fewer than per_node = 4
             [0, 0, 0, 0, 0, 0, 0, 0],      # target 1 admits nothing
             [1, 0, 1, 1, 1, 1, 1, 1]]      # target 2 admits everything but token 1
    v, i = _one(row, masks, 3, 1, 4)
    assert i[0] == [2, 5, 0, 1] and v[0] == [-0.25, -4.0, FILL, FILL]   # the admitted -4.0 ranks before every fill; fills 0, 1 (2 is admitted)
    assert i[1] == [0, 1, 2, 3] and v[1] == [FILL] * 4
    assert i[2] == [2, 4, 6, 7] and v[2] == [-0.25, -0.5, -0.75, -1.5]
    v, i = _one(row, [[0, 1, 0, 1, 0, 0, 0, 0]], 3, 1, 4)
    assert i == [[1, 3, 0, 2]] and v == [[-1.0, -2.0, FILL, FILL]]     # fills 0, 2: tokens 1 and 3 are skipped, nothing else


def test_first_step_with_fewer_admitted_tokens_than_beams():
    row = np.array([[-1.0, -0.5, -2.0, -0.5, -1.0, -3.0]], dtype=F)
    fsm = np.zeros((1, 2, 2, 6), dtype=np.uint8)
    fsm[0, 0, 0] = [0, 0, 0, 1, 1, 0]       # state 0 -> 0 admits tokens 3 and 4
    p, l = R.first(row, fsm, 4)             # state 0 -> 1 admits nothing
    assert p.tolist() == [[[3, 4, 0, 1], [0, 1, 2, 3]]]          # masked tokens of the FIRST step are -inf, lowest tokens first
    assert l.tolist() == [[[-0.5, -1.0, -INF, -INF], [-INF] * 4]]


@pytest.mark.parametrize("end", [0, 6])
def test_an_ended_beam_emits_end_then_the_lowest_tokens(end):
    row = [0.5, 9.0, -1.0, 3.0, 2.0, 7.0, 1.0]              # V = 7; never looked at
    v, i = _one(row, [[1] * 7], end, end, 3)
    assert i == [[0, 1, 2]] if end == 0 else i == [[6, 0, 1]]
    assert v == [[0.0, -INF, -INF]]
    # under a mask the forbidden tokens (-1e20) rank before the allowed non-END ones (-inf), END itself included when it is forbidden
    m = [1, 0, 1, 1, 0, 1, 1]
    v, i = _one(row, [m], end, end, 3)
    assert i == [[end, 1, 4]] and v == [[0.0, FILL, FILL]]
    m[end] = 0
    v, i = _one(row, [m], end, end, 3)
    assert (i == [[0, 1, 4]] if end == 0 else i == [[1, 4, 6]]) and v == [[FILL] * 3]
    # the records form of the same row
    parts = R.records(np.array([row], dtype=F))
    sv, si = R.rows_from_records(parts, 7, np.full((1, 1, 1), end), end, 2)
    assert si.reshape(-1).tolist() == ([0, 1] if end == 0 else [6, 0]) and sv.reshape(-1).tolist() == [0.0, -INF]


def test_a_dead_row_is_scored_as_all_zero_log_probs_only_when_asked():
    row = [-3.0, -1.0, -0.25, -2.0, -0.5, -4.0]
    masks = [[0, 1, 1, 0, 1, 1]]
    assert _one(row, masks, 3, 1, 3, last_lp=-1e20, skip_dead=True) == ([[0.0, 0.0, 0.0]], [[1, 2, 4]])
    assert _one(row, masks, 3, 1, 3, last_lp=-1e20, skip_dead=False) == ([[-0.25, -0.5, -1.0]], [[2, 4, 1]])
    assert _one(row, masks, 3, 1, 3, last_lp=-5.0, skip_dead=True) == ([[-0.25, -0.5, -1.0]], [[2, 4, 1]])
    assert _one(row, masks, 1, 1, 3, last_lp=-1e20, skip_dead=True) == ([[0.0, FILL, FILL]], [[1, 0, 3]])   # ended comes first


def test_merge_keys_ties_and_back_pointers():
    # S = 1, beam = 3, per_node = 2: candidates c = 0 .. 5 of beams 0, 0, 1, 1, 2, 2
    sval = np.array([-1.0, -2.0, -0.5, -1.5, 0.0, -INF], dtype=F)
    sidx = np.array([10, 11, 20, 21, 30, 31])
    ll = np.array([-1.0, -1.5, -2.0], dtype=F)               # keys: -2, -3, -2, -3, -2, -inf
    p, l, bp = R.merge(sval, sidx, ll, 1, 3, 2)
    assert p.tolist() == [[[10, 20, 30]]] and l.tolist() == [[[-2.0, -2.0, -2.0]]] and bp.tolist() == [[[0, 1, 2]]]
    # a dead beam (-1e20) absorbs its row's values in float32: all its candidates tie and go by index; -inf beams come last
    ll = np.array([-INF, -1e20, -1e20], dtype=F)
    p, l, bp = R.merge(sval, sidx, ll, 1, 3, 2)
    assert p.tolist() == [[[20, 21, 30]]] and bp.tolist() == [[[1, 1, 2]]] and l.tolist() == [[[FILL] * 3]]
    p, l, bp = R.merge_stopped(np.array([-1.0, -2.0, -3.0, -INF], dtype=F), 2, 2, 7)
    assert p.tolist() == [[[7, 7], [7, 7]]] and bp.tolist() == [[[0, 1], [2, 3]]] and l.tolist() == [[[-1.0, -2.0], [-3.0, -INF]]]
    assert R.ctl_after(9, p, 7, 4) == 5 and R.ctl_after(3, p, 7, 4) == 3 and R.ctl_after(9, [[7, 2]], 7, 4) == 9


def test_backtrace_gather_and_the_filled_columns():
    preds = np.array([[[1, 2, 3]], [[4, 5, 6]], [[7, 8, 9]]])          # (steps 3, B 1, SB 3)
    backs = np.array([[[2, 0, 0]], [[1, 1, 2]]])
    assert R.backtrace(preds, backs).tolist() == [[[1, 5, 7], [1, 5, 8], [1, 6, 9]]]
    assert R.backtrace(preds[:1], None).tolist() == [[[1], [2], [3]]]
    assert R.backtrace_ctl(preds, backs, 2, 3, 0).tolist() == [[[3, 4, 0], [1, 5, 0], [1, 6, 0]]]
    assert R.backtrace_ctl(preds, backs, 0, 3, 0).tolist() == [[[1, 0, 0], [2, 0, 0], [3, 0, 0]]]      # clamped to one step
    assert np.array_equal(R.backtrace_ctl(preds, backs, 7, 3, 0), R.backtrace(preds, backs))           # clamped to max_steps
    src = np.arange(12, dtype=F).reshape(6, 2)
    assert R.gather_rows(src, [2, 2, 0, 1, 0, 0], 3)[:, 0].tolist() == [4.0, 4.0, 0.0, 8.0, 6.0, 6.0]


def test_records_layout_and_selection_from_records():
    g = np.random.default_rng(5)
    x = (np.round(g.standard_normal((4, 129)) * 6) / 4).astype(F)
    x[0, :5] = [1.0, 9.0, 9.0, 2.0, 9.0]
    p = R.records(x)
    assert p.shape == (4, 2, 6)
    col = p.view(np.int32)
    assert p[0, 0, 0] == 9.0 and p[0, 0, 2] == 9.0 and p[0, 0, 4] == 9.0 and col[0, 0, 3] == 1 and col[0, 0, 5] == 2   # ties: lower column
    assert col[:, 1, 3].tolist() == [128] * 4 and col[:, 1, 5].tolist() == [-1] * 4 and bool((p[:, 1, 1] == 1.0).all())
    assert np.allclose(R.records_lse64(p), R.lse64(x), rtol=0, atol=1e-6)
    last = np.full((2, 1, 2), 3)
    for per_node in (1, 2):
        a_v, a_i = R.rows_from_records(p, 129, last, 1, per_node)
        b_v, b_i = R.rows(x, None, last, 1, per_node, norm=True)
        assert np.array_equal(a_i, b_i) and R.err_over_bound(a_v, b_v) <= 1.0


def test_log_probs_keep_ties_and_minus_infinity():
    x = np.array([[0.25, -np.inf, 0.25, -1.0], [2.0, 2.0, 2.0, 2.0]], dtype=F)
    lp = R.log_probs(x)
    assert lp[0, 0] == lp[0, 2] and lp[0, 1] == -INF and lp.dtype == F and len(set(lp[1].tolist())) == 1
    assert abs(float(np.exp(lp[0].astype(np.float64)).sum()) - 1.0) < 1e-6
