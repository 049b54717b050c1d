#!/usr/bin/env python3
"""Cost of unlikelihood training at the C2 train step's cross-entropy shape (bench.py: T = 21, B = 64 - 1344 rows -, V = 10000, ld =
the train workspace's padded V; caption lengths uniform in [0.6 T, T], so about four fifths of the rows carry a target).
The ssc_ce_fwd_unlike + ssc_ce_bwd_unlike pair (alpha 0.5) against the ssc_ce_fwd_smooth + ssc_ce_bwd_smooth pair on the same rows:
by bytes both move 3 row-matrices (the forward reads one, the backward reads and writes one); the unlikelihood pair adds the look-back
over the caption's earlier targets and at most T - 1 gathered loads per row and pass.  Alternating rounds on one device, each a window
of many back-to-back pairs between two device events after a warm-up; medians and min / max over the rounds.  One process, ended by
its own alarm after --time-limit seconds.  A report, not a gate.
    python tools/unlikelihood_probe.py [--rounds N] [--pairs N] [--time-limit S]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime import lib as L


def med(v):
    return {"us": round(statistics.median(v), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}


def kernels(a):
    lib = L.load()
    c = bench.C2
    B, T, V = c["B"], c["L"] + 1, c["V"]
    rows, ld = T * B, (V + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randn(rows, ld, device="cuda", generator=g) * 3.0
    logits = torch.empty_like(src)
    tg = torch.randint(0, V, (T, B), device="cuda", generator=g)
    tg[5], tg[9] = tg[2], tg[3]                                       # every caption repeats two of its words
    w = (torch.arange(T, device="cuda").view(T, 1) < torch.randint(3 * T // 5, T + 1, (1, B), device="cuda", generator=g)).float().contiguous()
    nv = w.sum(0).contiguous()
    gl = torch.full((B,), 1.0 / B, device="cuda")
    lse = torch.empty(3 * rows, device="cuda")
    loss, nll = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    scratch = torch.empty(2 * rows + B, device="cuda")
    P = L.ptr
    live = int(w.sum().item())
    d = L.Unlikelihood(0.5, 1e-5, scratch.data_ptr(), scratch[2 * rows:].data_ptr())

    def smooth():
        st = L.stream_ptr()
        lib.ssc_ce_fwd_smooth(P(logits), ld, P(tg), P(w), P(nv), T, B, V, 0.1, P(lse), P(loss), P(nll), st)
        lib.ssc_ce_bwd_smooth(P(logits), ld, P(tg), P(w), P(nv), P(lse), P(gl), T, B, V, 0.1, st)

    def unlike():
        st = L.stream_ptr()
        lib.ssc_ce_fwd_unlike(P(logits), ld, P(tg), P(w), P(nv), T, B, V, 0.1, C.byref(d), P(lse), P(loss), P(nll), st)
        lib.ssc_ce_bwd_unlike(P(logits), ld, P(tg), P(w), P(nv), P(lse), P(gl), T, B, V, 0.1, C.byref(d), st)

    variants = {"smooth": smooth, "unlike": unlike}

    def window(fn):
        logits.copy_(src)
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.pairs):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.pairs * 1e3   # us per pair

    for fn in variants.values():   # warm-up: code objects, clocks
        window(fn)
    t = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            t[k].append(window(fn))
    nbytes = (3 * live + (rows - live)) * V * 4
    out = {"rows": rows, "V": V, "ld": ld, "live_rows": live, "rounds": a.rounds, "pairs_per_round": a.pairs, "bytes": nbytes}
    for k, v in t.items():
        out[k] = med(v)
        out[k]["GBps"] = round(nbytes / (out[k]["us"] * 1e-6) / 1e9, 1)
    out["unlike_over_smooth"] = round(out["unlike"]["us"] / out["smooth"]["us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--time-limit", type=int, default=120, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.alarm(max(1, a.time_limit))   # (no handler: the default action ends the process, whatever it waits in)
    print(json.dumps({"kernels": kernels(a)}))


if __name__ == "__main__":
    main()
