#!/usr/bin/env python3
"""Generate tests/golden/g17_samplers.npz from the REFERENCE's own word samplers.

Run in the build container only, where the reference checkout is (``REF`` of make_golden.py):
    python tests/golden/make_sampler_golden.py

* Imports the reference's unmodified ``var_updown/modules/beam_search.py`` (MultinomialSampler, TopKSampler, TopPSampler,
  :103-293) with in-memory stand-ins for what it imports but never uses on the sampling path: ``overrides``,
  ``allennlp.common`` (FromParams, Registrable.register), ``allennlp.common.checks.ConfigurationError`` and
  ``allennlp.nn.util.min_value_of_dtype``.
* Wraps ``torch.multinomial`` to capture the distribution each sampler draws from, mapped back to vocabulary order (top-k:
  through the sampler's own ``topk`` indices, top-p: through its ``sort`` indices).
* The reference leaves the order of tied log-probs to torch's sort / topk; the fixture pins it to lower-index-first (what the
  device samplers do) by running the samplers under a stable descending ``torch.sort`` / ``Tensor.topk``.

Rows (float32 log-probs, per V in {50, 10000, 30000}): 0 peaked, 1 flat, 2 exact ties.  Settings: multinomial T in
{0.5, 1, 1.7}; top-k k in {1, 5, 100} x T in {0.7, 1.3}; top-p p in {0, 0.5, 0.9, 1} x T in {0.7, 1.3}.  A (V, setting) pair the
reference rejects (k > V) is left out.  Stored as value tables (encode()); tests/samplerref.load_fixture() rebuilds
lp_V{V} (3, V) and dist_V{V}_s{si} (3, V).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VS = (50, 10000, 30000)
SETTINGS = ([("multinomial", 0, 1.0, t) for t in (0.5, 1.0, 1.7)] +
            [("top-k", k, 1.0, t) for k in (1, 5, 100) for t in (0.7, 1.3)] +
            [("top-p", 0, p, t) for p in (0.0, 0.5, 0.9, 1.0) for t in (0.7, 1.3)])


def import_reference_samplers(ref):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Registrable:
        @classmethod
        def register(cls, name):
            return lambda c: c

    class ConfigurationError(Exception):
        pass

    def min_value_of_dtype(dtype):
        return torch.finfo(dtype).min

    mod("overrides", overrides=lambda f: f)
    mod("allennlp")
    mod("allennlp.common", FromParams=object, Registrable=Registrable)
    mod("allennlp.common.checks", ConfigurationError=ConfigurationError)
    mod("allennlp.nn")
    mod("allennlp.nn.util", min_value_of_dtype=min_value_of_dtype)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_beam_search",
                                                  os.path.join(ref, "var_updown", "var_updown", "modules", "beam_search.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def rows_for(V, g):
    # logits on coarse grids (1/16, 1/512): every row takes at most 256 distinct values (many tokens share one: ties everywhere,
    # cut by index), which is what lets the fixture be stored as value tables (see encode())
    peaked = (torch.randn(V, generator=g) * 16).round().clamp(-120, 120) / 16
    peaked[V // 3] += 8.0
    peaked[(2 * V) // 3] += 6.5
    flat = (0.05 * torch.randn(V, generator=g) * 512).round().clamp(-120, 120) / 512
    ties = torch.randint(0, 6, (V,), generator=g).float() * -0.75   # six distinct values, each shared by ~V/6 tokens
    ties[torch.randperm(V, generator=g)[:3]] = 1.5                   # a three-way tie at the top
    logits = torch.stack([peaked, flat, ties])
    return torch.log_softmax(logits, dim=-1)


def encode(out, V, lp, dists):
    """Stores the rows and the reference's distributions compactly, and checks the encoding is exact.
    lp_V{V}_vals (3, 256) float32 + lp_V{V}_idx (3, V) uint8: row r is vals[r][idx[r]].
    Per setting: keep_V{V}_s{si} (3,) int64, the number of tokens kept - always a prefix of the row in descending order, ties by
    index -, and prob_V{V}_s{si} (3, 256) float32, the reference's probability of a kept token of each value (in a row, the
    reference gives equal log-probs equal probabilities).  tests/samplerref.load_fixture() rebuilds the (3, V) arrays."""
    lpn = lp.numpy()
    vals = np.zeros((3, 256), dtype=np.float32)
    idx = np.zeros((3, V), dtype=np.uint8)
    order = np.argsort(-lpn, axis=1, kind="stable")
    for r in range(3):
        u, inv = np.unique(lpn[r], return_inverse=True)
        assert len(u) <= 256, len(u)
        vals[r, : len(u)] = u
        idx[r] = inv
    assert np.array_equal(np.take_along_axis(vals, idx.astype(np.int64), 1), lpn)
    out[f"lp_V{V}_vals"], out[f"lp_V{V}_idx"] = vals, idx
    for si, probs in dists.items():
        keep = np.zeros(3, dtype=np.int64)
        tab = np.zeros((3, 256), dtype=np.float32)
        for r in range(3):
            kept = probs[r] > 0
            n = int(kept.sum())
            assert kept[order[r, :n]].all(), "kept set is not a prefix of the descending order"
            keep[r] = n
            tab[r, idx[r][kept]] = probs[r][kept]
            rebuilt = np.where(kept, tab[r, idx[r]], 0).astype(np.float32)
            assert np.array_equal(rebuilt, probs[r]), "equal log-probs with different probabilities"
        out[f"keep_V{V}_s{si}"], out[f"prob_V{V}_s{si}"] = keep, tab


def main():
    sys.path.insert(0, HERE)
    from make_golden import REF
    bs = import_reference_samplers(REF)
    g = torch.Generator().manual_seed(1717)
    out = {"cfg": np.array(repr({"settings": SETTINGS, "vs": VS}))}
    captured = []
    orig_multinomial, orig_sort, orig_topk = torch.multinomial, torch.sort, torch.Tensor.topk

    def fake_multinomial(probs, n, replacement=False, **kw):
        captured.append(probs.clone())
        return orig_multinomial(probs, n, replacement=replacement, **kw)

    def stable_sort(x, dim=-1, descending=False, **kw):
        return orig_sort(x, dim=dim, descending=descending, stable=True)

    def stable_topk(x, k, dim=-1, largest=True, sorted=True):
        v, i = orig_sort(x, dim=dim, descending=largest, stable=True)
        return v.narrow(dim, 0, k), i.narrow(dim, 0, k)

    torch.multinomial, torch.sort, torch.Tensor.topk = fake_multinomial, stable_sort, stable_topk
    try:
        for V in VS:
            lp = rows_for(V, g)
            dists = {}
            for si, (kind, k, p, T) in enumerate(SETTINGS):
                if kind == "top-k" and k > V:
                    continue
                if kind == "multinomial":
                    s = bs.MultinomialSampler(temperature=T)
                elif kind == "top-k":
                    s = bs.TopKSampler(k=k, temperature=T)
                else:
                    s = bs.TopPSampler(p=p, temperature=T)
                captured.clear()
                s.sample_nodes(lp.clone(), 1, {})
                probs = captured[0]
                if kind == "top-k":
                    _, idx = stable_topk(lp, k)
                elif kind == "top-p":
                    _lp = torch.log_softmax(lp / T, dim=-1) if T != 1.0 else lp
                    _, idx = stable_sort(_lp, descending=True)
                else:
                    idx = None
                if idx is not None:
                    full = torch.zeros_like(lp)
                    full.scatter_(1, idx, probs)
                    probs = full
                dists[si] = probs.numpy().astype(np.float32)
            encode(out, V, lp, dists)
    finally:
        torch.multinomial, torch.sort, torch.Tensor.topk = orig_multinomial, orig_sort, orig_topk
    path = os.path.join(HERE, "g17_samplers.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
