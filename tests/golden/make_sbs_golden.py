#!/usr/bin/env python3
"""Generate tests/golden/g18_stochastic_beam.npz from the REFERENCE's own stochastic beam search.

Run in the build container only, where the reference checkout is (``REF`` of make_golden.py):
    python tests/golden/make_sbs_golden.py

* Imports the reference's unmodified ``var_updown/modules/beam_search.py`` (BeamSearch + GumbelSampler, :294-432, :592-768) with
  the in-memory stand-ins of make_sampler_golden.import_reference_samplers.
* Patches ``torch.rand_like`` so that its call c (one per step: init_state at step 0, sample_nodes after) returns the Philox
  uniforms of step c for the call's rows in order (tests/sbsref.uniforms): the reference sees exactly the device's noise.
* Pins the order of ties as the device does, by a stable descending ``sort`` / ``topk`` (as make_sampler_golden.py does).
* The step function is tests/sbsref.step_rows: log-probs from the last token, the step and a per-row state that the reference's
  _update_state re-orders, so back-pointers matter.

Per case of sbsref.CASES it stores the predictions (B, k, steps) and log-probs (B, k), and per step the selected tokens,
summed log-probs, G states and back-pointers (steps, B, k), plus ``gap`` (steps, B): the smallest margin of any decision of the
entry at that step - each row's cut (the n-th vs the (n+1)-th G), the merge's cut (the k-th vs the (k+1)-th candidate G) and
the adjacent summed log-probs of the sort - for margin-aware comparisons.  The log-prob rows are not stored: sbsref.replay()
regenerates them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import sbsref  # noqa: E402
from make_sampler_golden import import_reference_samplers  # noqa: E402


def _adjacent_gap(x):
    """smallest difference between adjacent finite values of each row of x (sorted descending); inf if none."""
    x = np.sort(np.asarray(x, dtype=np.float64), axis=1)[:, ::-1]
    d = x[:, :-1] - x[:, 1:]
    d = np.where(np.isfinite(x[:, :-1]) & np.isfinite(x[:, 1:]), d, np.inf)
    return d.min(1) if d.shape[1] else np.full(x.shape[0], np.inf)


def _cut_gap(x, m):
    """x (rows, C): the m-th largest minus the (m+1)-th (inf where either is not finite or C <= m)."""
    x = np.sort(np.asarray(x, dtype=np.float64), axis=1)[:, ::-1]
    if x.shape[1] <= m:
        return np.full(x.shape[0], np.inf)
    a, b = x[:, m - 1], x[:, m]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(a) & np.isfinite(b), a - b, np.inf)


def run_case(bs, c):
    B, k, n, V, T = c["B"], c["k"], c["n"], c["V"], c["T"]
    calls = {"rand": 0}
    rec = {"Grow": [], "cand": [], "beams": [], "nodes": []}
    orig_rand_like = torch.rand_like

    def fake_rand_like(x, *a, **kw):
        rows = x.shape[0]
        u = sbsref.uniforms(x.shape[1], sbsref.SEED, calls["rand"], np.arange(rows))
        calls["rand"] += 1
        return torch.from_numpy(u)

    sampler = bs.GumbelSampler(temperature=T)
    orig_gwm, orig_nodes, orig_beams = sampler.gumbel_with_max, sampler.sample_nodes, sampler.sample_beams

    def gwm(phi, Tt):
        G = orig_gwm(phi, Tt)
        rec["Grow"].append(G.clone())
        return G

    def nodes(log_probs, per_node, state):
        out = orig_nodes(log_probs, per_node, state)
        rec["nodes"].append(out[1].clone())
        return out

    def beams(log_probs, beam_size, state):
        rec["cand"].append(state["G_phi_S"].reshape(log_probs.shape).clone())
        out = orig_beams(log_probs, beam_size, state)
        rec["beams"].append((out[0].clone(), out[1].clone(), out[2]["G_phi_S"].reshape(B, beam_size).clone()))
        return out

    sampler.gumbel_with_max, sampler.sample_nodes, sampler.sample_beams = gwm, nodes, beams
    search = bs.BeamSearch(sbsref.END, max_steps=c["steps"], beam_size=k, per_node_beam_size=n, sampler=sampler)

    def step(last, state, t):
        acc = state["acc"].numpy()
        lp = sbsref.step_rows(last.numpy(), t, acc, V, c["boost"])
        return torch.from_numpy(lp), {"acc": torch.from_numpy(sbsref.next_state(acc, last.numpy()))}

    torch.rand_like = fake_rand_like
    try:
        start = torch.full((B,), sbsref.END, dtype=torch.long)
        pred, lps = search.search(start, {"acc": torch.from_numpy(sbsref.start_state(B))}, step)
    finally:
        torch.rand_like = orig_rand_like
    steps = len(rec["beams"])
    out = {"pred": pred.numpy().astype(np.int64), "lp": lps.numpy().astype(np.float32)}
    tok = np.zeros((steps, B, k), np.int64)
    lpt = np.zeros((steps, B, k), np.float32)
    G = np.zeros((steps, B, k), np.float32)
    bp = np.zeros((steps, B, k), np.int64)
    gap = np.zeros((steps, B), np.float64)
    for t in range(steps):
        sl, si, sg = rec["beams"][t]
        lpt[t], G[t] = sl.numpy(), sg.numpy()
        m = k if t == 0 else n
        if t == 0:
            tok[t] = si.numpy()
        else:
            cand_tok = rec["nodes"][t - 1].reshape(B, k * n).numpy()
            tok[t] = np.take_along_axis(cand_tok, si.numpy(), 1)
            bp[t] = si.numpy() // n
        rows = _cut_gap(rec["Grow"][t].numpy(), m).reshape(B, -1).min(1)
        gap[t] = np.minimum(np.minimum(rows, _cut_gap(rec["cand"][t].numpy(), k)), _adjacent_gap(sl.numpy()))
    out.update(tok=tok, lp_t=lpt, G=G, bp=bp, gap=gap.astype(np.float32))
    return out


def main():
    from make_golden import REF
    bs = import_reference_samplers(REF)
    orig_sort, orig_topk, orig_tsort, orig_ttopk = torch.sort, torch.topk, torch.Tensor.sort, torch.Tensor.topk

    def stable_sort(x, dim=-1, descending=False, **kw):
        return orig_sort(x, dim=dim, descending=descending, stable=True)

    def stable_topk(x, k, dim=-1, largest=True, sorted=True):
        v, i = orig_sort(x, dim=dim, descending=largest, stable=True)
        return v.narrow(dim, 0, k), i.narrow(dim, 0, k)

    torch.sort, torch.topk, torch.Tensor.sort, torch.Tensor.topk = stable_sort, stable_topk, stable_sort, stable_topk
    out = {"cfg": np.array(repr({"cases": [c["name"] for c in sbsref.CASES], "seed": sbsref.SEED}))}
    try:
        for c in sbsref.CASES:
            for key, val in run_case(bs, c).items():
                out[c["name"] + "/" + key] = val
    finally:
        torch.sort, torch.topk, torch.Tensor.sort, torch.Tensor.topk = orig_sort, orig_topk, orig_tsort, orig_ttopk
    path = os.path.join(HERE, "g18_stochastic_beam.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
