#!/usr/bin/env python3
"""Generate tests/golden/g19_sampled_beam.npz from the REFERENCE's own sampled-node beam search.

Run in the build container only, where the reference checkout is (``REF`` of make_golden.py):
    python tests/golden/make_sampled_beam_golden.py

* Imports the reference's unmodified ``var_updown/modules/beam_search.py`` (BeamSearch + MultinomialSampler / TopKSampler /
  TopPSampler, :103-293, :592-768) with the in-memory stand-ins of make_sampler_golden.import_reference_samplers.
* Patches ``torch.multinomial`` so that its call c (one per step t = c + 1, on all B * k rows) makes the device's choice from the
  probabilities it is given: without replacement the n largest log(p) + Gumbel(u_v) (Gumbel-top-n, stable), with replacement
  draw d = argmax log(p) + Gumbel(u_v at noise word d), where u_v is the device's Philox uniform of the VOCABULARY token at each
  position (tests/sampledbeamref.uniforms).  TopKSampler and TopPSampler call it on permuted rows; the permutation is the one
  their ``topk`` / ``sort`` call just returned, recorded by wrapping those.
* Pins the order of ties as the device does, by a stable descending ``sort`` / ``topk`` (as make_sbs_golden.py does).
* The step function is tests/sbsref.step_rows: log-probs from the last token, the step and a per-row state that the reference's
  _update_state re-orders, so back-pointers matter.

Per case of sampledbeamref.CASES it stores the predictions (B, k, steps) and log-probs (B, k), and per step the selected tokens,
summed log-probs and back-pointers (steps, B, k), plus ``gap`` (steps, B): the smallest margin of any decision of the entry at
that step - the kept set's cut, each row's draws (the n-th vs (n+1)-th perturbed score, or each draw's best vs second), the
merge's cut (the k-th vs (k+1)-th summed log-prob) and the adjacent summed log-probs of the sort - for margin-aware comparisons.
The log-prob rows are not stored: sbsref.replay() regenerates them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import sampledbeamref as R  # noqa: E402
from make_sampler_golden import import_reference_samplers  # noqa: E402


# Margins.  Exact ties are decided the same way on both sides (lower index first: the values of one row come from the same
# float32 logits), so a margin is the distance to the nearest DIFFERENT value.
def _adjacent_gap(x):
    """smallest non-zero difference between adjacent finite values of each row of x; inf if none."""
    x = np.sort(np.asarray(x, dtype=np.float64), axis=1)[:, ::-1]
    d = x[:, :-1] - x[:, 1:]
    d = np.where(np.isfinite(x[:, :-1]) & np.isfinite(x[:, 1:]) & (d != 0), d, np.inf)
    return d.min(1) if d.shape[1] else np.full(x.shape[0], np.inf)


def _cut_gap(x, m):
    """x (rows, C): the margin of the cut after the m largest - the m-th largest minus the (m+1)-th, or where those are equal,
    the distance from their value to the nearest different finite value (inf where there is none or C <= m)."""
    x = np.sort(np.asarray(x, dtype=np.float64), axis=1)[:, ::-1]
    out = np.full(x.shape[0], np.inf)
    if x.shape[1] <= m:
        return out
    for r in range(x.shape[0]):
        a, b = x[r, m - 1], x[r, m]
        if not (np.isfinite(a) and np.isfinite(b)):
            continue
        if a != b:
            out[r] = a - b
        else:
            f = x[r][np.isfinite(x[r]) & (x[r] != a)]
            out[r] = np.abs(f - a).min() if f.size else np.inf
    return out


def run_case(bs, c, sorts):
    B, k, n, V, T = c["B"], c["k"], c["n"], c["V"], c["T"]
    calls = {"multinomial": 0}
    rec = {"beams": [], "nodes": [], "rowgap": []}
    orig_multinomial = torch.multinomial

    def fake_multinomial(probs, num, replacement=False, **kw):
        rows, C = probs.shape
        step = calls["multinomial"] + 1
        calls["multinomial"] += 1
        perm = sorts["last"] if c["kind"] != "multinomial" else None
        vocab = perm.numpy() if perm is not None else np.broadcast_to(np.arange(C), (rows, C))
        assert vocab.shape == (rows, C), (vocab.shape, probs.shape)
        with np.errstate(divide="ignore"):
            logp = np.log(probs.double().numpy())
        out = np.zeros((rows, num), np.int64)
        gap = np.full(rows, np.inf)
        for d in range(num if replacement else 1):
            u = R.uniforms(V, R.SEED, step, np.arange(rows), d)
            s = logp + R.gumbel(np.take_along_axis(u, vocab, 1)).astype(np.float64)
            o = np.argsort(-s, axis=1, kind="stable")
            if replacement:
                out[:, d] = o[:, 0]
                gap = np.minimum(gap, _cut_gap(s, 1))
            else:
                out[:] = o[:, :num]
                gap = np.minimum(gap, _cut_gap(s, num))
        rec["rowgap"].append(gap)
        return torch.from_numpy(out)

    if c["kind"] == "multinomial":
        sampler = bs.MultinomialSampler(temperature=T, with_replacement=c["rep"])
    elif c["kind"] == "top-k":
        sampler = bs.TopKSampler(k=c["top_k"], temperature=T, with_replacement=c["rep"])
    else:
        sampler = bs.TopPSampler(p=c["top_p"], temperature=T, with_replacement=c["rep"])
    orig_nodes, orig_beams = sampler.sample_nodes, sampler.sample_beams

    def nodes(log_probs, per_node, state):
        out = orig_nodes(log_probs, per_node, state)
        rec["nodes"].append(out[1].clone())
        # the margin of the kept set's cut, per row (live rows only: an ended row is one-hot)
        x = log_probs.double().numpy()
        m = np.full(x.shape[0], np.inf)
        for r in range(x.shape[0]):
            if np.isfinite(x[r]).sum() > 1:
                m[r] = R.kept_set(x[r], c["kind"], c["top_k"], c["top_p"], T, n, c["rep"])[1]
        rec["rowgap"][-1] = np.minimum(rec["rowgap"][-1], m)
        return out

    def beams(log_probs, beam_size, state):
        out = orig_beams(log_probs, beam_size, state)
        rec["beams"].append((out[0].clone(), out[1].clone(), log_probs.clone()))
        return out

    sampler.sample_nodes, sampler.sample_beams = nodes, beams
    search = bs.BeamSearch(R.END, max_steps=c["steps"], beam_size=k, per_node_beam_size=n, sampler=sampler)

    def step(last, state, t):
        acc = state["acc"].numpy()
        lp = R.sbsref.step_rows(last.numpy(), t, acc, V, c["boost"])
        return torch.from_numpy(lp), {"acc": torch.from_numpy(R.sbsref.next_state(acc, last.numpy()))}

    torch.multinomial = fake_multinomial
    try:
        start = torch.full((B,), R.END, dtype=torch.long)
        pred, lps = search.search(start, {"acc": torch.from_numpy(R.sbsref.start_state(B))}, step)
    finally:
        torch.multinomial = orig_multinomial
    steps = len(rec["beams"])
    out = {"pred": pred.numpy().astype(np.int64), "lp": lps.numpy().astype(np.float32)}
    tok = np.zeros((steps, B, k), np.int64)
    lpt = np.zeros((steps, B, k), np.float32)
    bp = np.zeros((steps, B, k), np.int64)
    gap = np.zeros((steps, B), np.float64)
    for t in range(steps):
        sl, si, cand = rec["beams"][t]
        lpt[t] = sl.numpy()
        if t == 0:
            tok[t] = si.numpy()
            rows = np.full(B, np.inf)
        else:
            cand_tok = rec["nodes"][t - 1].reshape(B, k * n).numpy()
            tok[t] = np.take_along_axis(cand_tok, si.numpy(), 1)
            bp[t] = si.numpy() // n
            rows = rec["rowgap"][t - 1].reshape(B, k).min(1)
        gap[t] = np.minimum(np.minimum(rows, _cut_gap(cand.numpy(), k)), _adjacent_gap(sl.numpy()))
    out.update(tok=tok, lp_t=lpt, bp=bp, gap=gap.astype(np.float32))
    return out


def main():
    from make_golden import REF
    bs = import_reference_samplers(REF)
    orig_sort, orig_topk, orig_tsort, orig_ttopk = torch.sort, torch.topk, torch.Tensor.sort, torch.Tensor.topk
    sorts = {"last": None}

    def stable_sort(x, dim=-1, descending=False, **kw):
        v, i = orig_sort(x, dim=dim, descending=descending, stable=True)
        sorts["last"] = i
        return v, i

    def stable_topk(x, k, dim=-1, largest=True, sorted=True):
        v, i = orig_sort(x, dim=dim, descending=largest, stable=True)
        v, i = v.narrow(dim, 0, k), i.narrow(dim, 0, k)
        sorts["last"] = i
        return v, i

    torch.sort, torch.topk, torch.Tensor.sort, torch.Tensor.topk = stable_sort, stable_topk, stable_sort, stable_topk
    out = {"cfg": np.array(repr({"cases": [c["name"] for c in R.CASES], "seed": R.SEED}))}
    try:
        for c in R.CASES:
            for key, val in run_case(bs, c, sorts).items():
                out[c["name"] + "/" + key] = val
    finally:
        torch.sort, torch.topk, torch.Tensor.sort, torch.Tensor.topk = orig_sort, orig_topk, orig_tsort, orig_ttopk
    path = os.path.join(HERE, "g19_sampled_beam.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
