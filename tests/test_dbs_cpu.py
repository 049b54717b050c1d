"""CPU: the diverse beam search's definition (tests/dbsref.py, the numpy float32 restatement of include/ssc.h: ssc_diverse_desc) -
a hand-worked case, its two limits (one group = beam search, strength 0 = independent groups), the top-m containment the device
kernels rely on, and the configuration keys."""
import itertools

import numpy as np
import pytest
import torch

import dbsref as R
import oracle
from goldenlib import cbs_table_step, load_raw
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config

F = np.float32


def test_hand_worked_case():
    """V = 6, k = 4 in two groups of two, n = 1, strength 2, END = 1; beam 1 ends at step 0.  Every number is a multiple of 1/4."""
    lp0 = np.array([[-4, -1, -0.5, -2, -3, -5]], dtype=F)
    tok, lp, _ = R.first_step(lp0, 4, 2, 2.0)
    # group 0: tokens 2 (-0.5) and 1 (-1); group 1 sees r = [-4, -3, -2.5, -2, -3, -5]: tokens 3 (-2) and 2 (true log-prob -0.5)
    assert tok.tolist() == [[2, 1, 3, 2]]
    assert lp.tolist() == [[-0.5, -1.0, -2.0, -0.5]]
    rows = np.array([[-1, -3, -2, -0.25, -4, -5],      # beam 0: token 3
                     [0, 0, 0, 0, 0, 0],               # beam 1 has ended: never read
                     [-0.5, -1, -3, -0.25, -4, -5],    # beam 2: token 3 costs 2 now (-2.25), token 0 wins
                     [-3, -2, -4, -0.5, -1.5, -5]],    # beam 3: token 3 at -2.5, token 4 (-1.5) wins
                    dtype=F)
    tok1, lp1, bp1, _ = R.next_step(rows, tok, lp, 1, 4, 2, 1, 2.0)
    assert tok1.tolist() == [[3, 1, 4, 0]]
    assert bp1.tolist() == [[0, 1, 3, 2]]
    assert lp1.tolist() == [[-0.75, -1.0, -2.0, -2.5]]   # the TRUE sums: no penalty inside
    # without the penalty both beams of group 1 would take token 3 as well
    tok_, _, _, _ = R.next_step(rows, tok, lp, 1, 4, 2, 1, 0.0)
    assert tok_.tolist() == [[3, 1, 3, 3]]


def _np_step(step):
    """A torch table step as dbsref.search wants it: numpy in, numpy out, the state a dict of arrays (None before step 0)."""
    def f(tokens, states):
        st = None if not states else {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in states.items()}
        lp, new = step(torch.from_numpy(tokens), st)
        return lp.numpy().astype(F), {k: v.numpy() for k, v in new.items()}
    return f


_G12 = load_raw("g12_cbs")
_TRIVIAL = [ci for ci in range(int(_G12["ncases"])) if int(_G12[f"search/case{ci}/dims"][1]) == 1]


def test_fixture_has_trivial_machine_cases():
    assert _TRIVIAL


@pytest.mark.parametrize("ci", _TRIVIAL)
def test_one_group_is_the_oracle_beam_search(ci):
    """Gr = 1 (any strength): the oracle's restatement of ConstrainedBeamSearch.search at S = 1 on the g12_cbs trivial-machine
    cases, exactly - tokens and float32 log-probs."""
    key = f"search/case{ci}"
    B, S, V, beam, per_node, steps = (int(x) for x in _G12[key + "/dims"])
    table, drift = torch.from_numpy(_G12[key + "/table"]), torch.from_numpy(_G12[key + "/drift"])
    step = cbs_table_step(table, drift)
    want_p, want_lp = oracle.cbs_search(torch.full((B,), 1, dtype=torch.long), None, step, torch.ones(B, 1, 1, V, dtype=torch.uint8),
                                        1, max_steps=steps, beam_size=beam, per_node_beam_size=per_node)
    for lam in (0.0, 3.0):
        pred, lp, _ = R.search(_np_step(step), None, B, beam, 1, per_node, lam, steps)
        assert np.array_equal(pred, want_p[:, 0].numpy())
        assert np.array_equal(lp, want_lp[:, 0].numpy())


def test_strength_zero_runs_the_groups_independently():
    """lambda = 0: every group is the beam-k' search on its own rows."""
    rng = np.random.default_rng(3)
    B, k, Gr, n, V = 3, 6, 3, 2, 40
    kp = k // Gr
    lp0 = R.log_softmax64(rng.standard_normal((B, V))).astype(F)
    tok, lp, _ = R.first_step(lp0, k, Gr, 0.0)
    t1, l1, _ = R.first_step(lp0, kp, 1, 0.0)
    for g in range(Gr):
        assert np.array_equal(tok[:, g * kp:(g + 1) * kp], t1) and np.array_equal(lp[:, g * kp:(g + 1) * kp], l1)
    rows = R.log_softmax64(rng.standard_normal((B * k, V)) * 2).astype(F)
    last = rng.integers(2, V, (B, k))
    last[0, 1] = last[2, 4] = R.END
    phi = rng.uniform(-6, -1, (B, k)).astype(F)
    tok, lp, bp, _ = R.next_step(rows, last, phi, B, k, Gr, n, 0.0)
    for g in range(Gr):
        sl = slice(g * kp, (g + 1) * kp)
        t1, l1, b1, _ = R.next_step(rows.reshape(B, k, V)[:, sl].reshape(-1, V), last[:, sl], phi[:, sl], B, kp, 1, n, 0.0)
        assert np.array_equal(tok[:, sl], t1) and np.array_equal(lp[:, sl], l1) and np.array_equal(bp[:, sl], b1 + g * kp)


def test_top_m_list_holds_the_penalised_top_n():
    """The claim the device kernels rest on, by brute force: with at most k - k' penalised tokens, a row's n best tokens under
    r = lp - lambda * c are its n best computed from its m = n + (k - k') best under lp alone - order and ties included.  Rows
    with heavy ties (a few levels), every (k, Gr, n) with k <= 8."""
    rng = np.random.default_rng(11)
    V = 14
    cases = 0
    for k in range(1, 9):
        for Gr in [g for g in range(1, k + 1) if k % g == 0]:
            kp = k // Gr
            for n in range(1, min(k, V) + 1):
                m = min(n + k - kp, V)
                for trial in range(12):
                    levels = rng.integers(2, 5)
                    lp = (rng.integers(0, levels, V) * F(-0.5)).astype(F)
                    c = np.zeros(V, dtype=F)
                    P = k - kp
                    if P:
                        hit = rng.choice(V, size=rng.integers(0, P + 1), replace=False)
                        # (the counts of all penalised tokens sum to at most P: each earlier beam selects one token)
                        for v in hit:
                            c[v] += 1
                        extra = P - len(hit)
                        if len(hit) and extra:
                            for v in rng.choice(hit, size=rng.integers(0, extra + 1)):
                                c[v] += 1
                    for lam in (0.0, 0.5, 4.0):
                        full = R.top_by(lp - (F(lam) * c), n).tolist()
                        assert R.top_n_from_list(lp, c, lam, n, m) == full, (k, Gr, n, lam, lp, c)
                        cases += 1
    assert cases > 3000


def test_top_m_list_is_tight():
    """m - 1 entries are not enough: the list length is what the argument needs, not slack."""
    lp = np.array([-1, -2, -3, -4, -5, -6], dtype=F)
    c = np.array([1, 1, 0, 0, 0, 0], dtype=F)   # k - k' = 2 penalised tokens, n = 1: m = 3
    assert R.top_n_from_list(lp, c, 10.0, 1, 3) == R.top_by(lp - F(10.0) * c, 1).tolist() == [2]
    assert R.top_n_from_list(lp, c, 10.0, 1, 2) != [2]


def _cfg(*override):
    return Config(config_override=list(override))


def test_config_keys_and_defaults():
    C = _cfg()
    assert C.MODEL.DIVERSE_BEAM_SEARCH is False and C.MODEL.DIVERSE_BEAM_GROUPS == 1 and C.MODEL.DIVERSE_BEAM_STRENGTH == 0.5
    assert sampling.diverse_beam_from_config(C.MODEL) is None and sampling.from_config(C.MODEL) is None
    C = _cfg("MODEL.DIVERSE_BEAM_SEARCH", "True", "MODEL.BEAM_SIZE", "20", "MODEL.DIVERSE_BEAM_GROUPS", "20",
             "MODEL.DIVERSE_BEAM_STRENGTH", "0.8")
    d = sampling.diverse_beam_from_config(C.MODEL)
    assert isinstance(d, sampling.DiverseBeam) and d.groups == 20 and d.strength == pytest.approx(0.8)
    assert sampling.from_config(C.MODEL) is None   # deterministic: no sampler
    assert d.per_node(20) == 1 and sampling.DiverseBeam(3, 0.5).per_node(12) == 2 and sampling.DiverseBeam(1, 0.5).per_node(5) == 2
    desc = d.desc()
    assert desc.groups == 20 and desc.strength == pytest.approx(0.8)


@pytest.mark.parametrize("override,key", [
    (("MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", "3"), "MODEL.DECODE_SAMPLER"),
    (("MODEL.STOCHASTIC_BEAM_SEARCH", "True"), "MODEL.STOCHASTIC_BEAM_SEARCH"),
    (("MODEL.BEAM_SIZE", "6", "MODEL.DIVERSE_BEAM_GROUPS", "4"), "MODEL.DIVERSE_BEAM_GROUPS"),
    (("MODEL.DIVERSE_BEAM_GROUPS", "0"), "MODEL.DIVERSE_BEAM_GROUPS"),
    (("MODEL.DIVERSE_BEAM_STRENGTH", "-1.0"), "MODEL.DIVERSE_BEAM_STRENGTH"),
    (("MODEL.USE_CBS", "True", "MODEL.EMBEDDING_SIZE", "300"), "MODEL.USE_CBS"),
])
def test_config_exclusions_name_the_key(override, key):
    C = _cfg("MODEL.DIVERSE_BEAM_SEARCH", "True", *override)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        sampling.diverse_beam_from_config(C.MODEL)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        sampling.from_config(C.MODEL)


def test_sampled_beam_search_excludes_it():
    C = _cfg("MODEL.DIVERSE_BEAM_SEARCH", "True", "MODEL.SAMPLED_BEAM_SEARCH", "True", "MODEL.DECODE_SAMPLER", "top-p")
    with pytest.raises(ValueError, match="MODEL.DIVERSE_BEAM_SEARCH"):
        sampling.diverse_beam_from_config(C.MODEL)
    C = _cfg("MODEL.DIVERSE_BEAM_SEARCH", "True", "MODEL.SAMPLED_BEAM_SEARCH", "True")
    with pytest.raises(ValueError, match="SAMPLED_BEAM_SEARCH"):
        sampling.from_config(C.MODEL)


def test_diverse_beam_value_checks():
    with pytest.raises(ValueError, match="groups"):
        sampling.DiverseBeam(0, 0.5)
    with pytest.raises(ValueError, match="strength"):
        sampling.DiverseBeam(2, -0.1)
    with pytest.raises(ValueError, match="strength"):
        sampling.DiverseBeam(2, float("inf"))
    with pytest.raises(ValueError, match="multiple"):
        sampling.DiverseBeam(4, 0.5).check_beam(6)


def test_library_declares_the_entry_points():
    import ctypes as C
    for name in ("ssc_beam_first_diverse", "ssc_beam_step_diverse", "ssc_decode_diverse_beam_workspace_bytes",
                 "ssc_decode_diverse_beam"):
        assert name in L.SYMBOLS
    assert [f for f, _ in L.DiverseDesc._fields_] == ["groups", "strength"]
    lib = L.load()
    # bad descriptors are refused before anything is launched (no GPU here)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_beam_first_diverse(None, None, None)
    d, s = L.BeamDesc(), L.DiverseDesc(2, 0.5)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_beam_step_diverse(C.byref(d), C.byref(s), None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    sd = L.SearchDesc()
    sd.nimg, sd.R, sd.n_samples, sd.S, sd.beam, sd.per_node, sd.max_steps = 1, 2, 1, 1, 6, 1, 3
    assert lib.ssc_decode_diverse_beam_workspace_bytes(C.byref(cfg), C.byref(sd), C.byref(L.DiverseDesc(3, 0.5))) > 0
    assert lib.ssc_decode_diverse_beam_workspace_bytes(C.byref(cfg), C.byref(sd), C.byref(L.DiverseDesc(4, 0.5))) == 0
