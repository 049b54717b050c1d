#!/usr/bin/env python3
"""Two timings of posterior scoring, each a median over alternating rounds on the same device (a window of back-to-back calls
between two device events after a warm-up; min / max over the rounds next to the median):
  rows:    ssc_posterior_rows alone at T = 21, B = 256, Z = 128 with every optional output, next to a device-to-device copy of the
           bytes it reads (mu, lv, z, eps of the live steps and w) - what a kernel bound by its reads alone would take;
  forward: one TrainEngine.posterior_forward at 256 rows x 36 regions x L = 20 at the C2 widths of bench.py, next to
           TrainEngine.forward of the same rows - the train forward as it was before posterior scoring existed; the difference is
           ssc_train_posterior's two launches and the output allocations.
A report, not a gate.
    python tools/posterior_probe.py [--rounds N] [--calls N] [--forwards N]
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
from ssc_runtime.engine import ModelDims, TrainEngine


def window(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def rounds(variants, n_rounds, n_calls):
    for fn in variants.values():   # warm-up: code objects, clocks, allocations
        window(fn, max(n_calls // 4, 1))
    t = {k: [] for k in variants}
    for _ in range(n_rounds):
        for k, fn in variants.items():
            t[k].append(window(fn, n_calls))
    out = {}
    for k, v in t.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=2000, help="ssc_posterior_rows calls per window")
    ap.add_argument("--forwards", type=int, default=10, help="forwards per window")
    a = ap.parse_args()
    lib = L.load()
    P = L.ptr
    T, B, Z = 21, 256, 128
    g = torch.Generator(device="cuda").manual_seed(1)
    mu, lv, eps = (torch.randn(T * B, Z, device="cuda", generator=g) for _ in range(3))
    z = eps * torch.exp(lv / 2) + mu
    w = (torch.arange(T, device="cuda").view(T, 1) < torch.randint(9, T + 1, (1, B), device="cuda", generator=g)).float().contiguous()
    log_ratio, kl, kl_dim = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, Z, device="cuda")
    step_kl, step_ratio = torch.empty(T, B, device="cuda"), torch.empty(T, B, device="cuda")
    d = L.PosteriorRowsDesc()
    d.T, d.B, d.Z, d.ldz, d.ldeps, d.ld = T, B, Z, Z, Z, Z
    d.mu, d.lv, d.z, d.eps, d.w = mu.data_ptr(), lv.data_ptr(), z.data_ptr(), eps.data_ptr(), w.data_ptr()
    d.kld_mode, d.pm_scale, d.prior_var = 0, 0.0, 1.0
    d.log_ratio, d.kl, d.kl_dim, d.step_kl, d.step_ratio = (t.data_ptr() for t in (log_ratio, kl, kl_dim, step_kl, step_ratio))
    live = int(w.sum().item())
    read_bytes = live * Z * 4 * 4 + T * B * 4
    src = torch.empty(read_bytes // 4, device="cuda")
    dst = torch.empty_like(src)
    out = {"T": T, "B": B, "Z": Z, "live_steps": live, "read_bytes": read_bytes, "rounds": a.rounds}
    out.update(rounds({"rows": lambda: lib.ssc_posterior_rows(C.byref(d), L.stream_ptr()), "copy": lambda: dst.copy_(src)}, a.rounds, a.calls))
    out["rows_gbps"] = round(read_bytes / out["rows_us"] / 1e3, 1)

    c = bench.C2
    rows = 256
    eng = TrainEngine(ModelDims(V=c["V"], E=c["E"], H=c["H"], A=c["A"], F=c["F"], Z=c["Z"], S=1, kld_mode=1, pm_scale=0.5), "cuda")
    torch.manual_seed(0)
    eng.params.flat.copy_(torch.randn_like(eng.params.flat) * 0.02)
    feats, caps, senti, e = bench.synth_batch(3, rows, c["R"], c["F"], c["L"], c["V"], c["Z"], "cuda")
    fwd = rounds({"posterior_forward": lambda: eng.posterior_forward(feats, caps, senti, e),
                  "forward": lambda: eng.forward(feats, caps, senti, e)}, a.rounds, a.forwards)
    out.update({"forward_rows": rows, "R": c["R"], "L": c["L"], **fwd})
    out["posterior_over_forward"] = round(out["posterior_forward_us"] / out["forward_us"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
