#!/usr/bin/env python3
"""Time of the vocabulary cross-entropy pair (forward + in-place backward) on the head of the C2 train step (bench.py's widths:
T * B = 1344 rows, V = 10000, ld = the train workspace's padded V): ssc_ce_fwd_smooth + ssc_ce_bwd_smooth at eps = 0 (the kernels
of ssc_ce_fwd / ssc_ce_bwd) and at eps = 0.1 (the single-scan forward and the 16-byte backward), in alternating rounds on the same
device, each round a window of many back-to-back pairs between two device events after a warm-up; medians and min / max over the
rounds.  The logits buffer is refilled before every window and is then overwritten pair after pair by its own gradients, the same
for every variant (the kernels' work does not depend on the values).  One third of the rows carry weight 0, as padded captions do.
--other LIB: another build's libssc_hip.so (tools/build_variant.py, or the library of another checkout) is loaded next to the
in-tree one and its ssc_ce_fwd + ssc_ce_bwd pair joins the rounds: the same-box A/B of the smoothed pair against that build's
plain pair (only those two symbols are taken from it, so a build from before the smoothing entries works).  A report, not a gate.
    python tools/smooth_probe.py [--rounds N] [--pairs N] [--eps X] [--other path/to/libssc_hip.so]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime import lib as L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--other", default="", help="another build's libssc_hip.so: its ssc_ce_fwd + ssc_ce_bwd pair is timed too")
    a = ap.parse_args()
    lib = L.load()
    c = bench.C2
    B, T, V = c["B"], c["L"] + 1, c["V"]
    rows, ld = T * B, (V + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randn(rows, ld, device="cuda", generator=g) * 3.0
    logits = torch.empty_like(src)
    tg = torch.randint(0, V, (T, B), device="cuda", generator=g)
    w = (torch.arange(T, device="cuda").view(T, 1) < torch.randint(T // 3, T + 1, (1, B), device="cuda", generator=g)).float().contiguous()
    nv = w.sum(0).contiguous()
    gl = torch.full((B,), 1.0 / B, device="cuda")
    lse = torch.empty(3 * rows, device="cuda")
    loss, nll = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    P = L.ptr

    def smooth(eps):
        def pair():
            st = L.stream_ptr()
            lib.ssc_ce_fwd_smooth(P(logits), ld, P(tg), P(w), P(nv), T, B, V, eps, P(lse), P(loss), P(nll), st)
            lib.ssc_ce_bwd_smooth(P(logits), ld, P(tg), P(w), P(nv), P(lse), P(gl), T, B, V, eps, st)
        return pair

    variants = {"eps0": smooth(0.0), "smooth": smooth(a.eps)}
    if a.other:
        other = C.CDLL(os.path.abspath(a.other))
        vp, i = C.c_void_p, C.c_int
        other.ssc_ce_fwd.restype = other.ssc_ce_bwd.restype = i
        other.ssc_ce_fwd.argtypes = [vp, i, vp, vp, vp, i, i, i, vp, vp, vp]
        other.ssc_ce_bwd.argtypes = [vp, i, vp, vp, vp, vp, vp, i, i, i, vp]

        def plain():
            st = L.stream_ptr()
            rc = other.ssc_ce_fwd(P(logits), ld, P(tg), P(w), P(nv), T, B, V, P(lse), P(loss), st)
            rc = rc or other.ssc_ce_bwd(P(logits), ld, P(tg), P(w), P(nv), P(lse), P(gl), T, B, V, st)
            if rc:
                raise RuntimeError(f"--other: ssc_ce_fwd / ssc_ce_bwd failed ({rc})")
        variants["other"] = plain

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
    out = {"rows": rows, "V": V, "ld": ld, "eps": a.eps, "rounds": a.rounds, "pairs_per_round": a.pairs,
           "live_rows": int(w.sum().item())}
    for k, v in t.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    out["smooth_over_eps0"] = round(out["smooth_us"] / out["eps0_us"], 3)
    if a.other:
        out["smooth_over_other"] = round(out["smooth_us"] / out["other_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
