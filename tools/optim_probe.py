#!/usr/bin/env python3
"""Time of the two optimiser kernels on the flat buffer of the C2 model (bench.py's widths): ssc_adam_step and ssc_sgd_step on the
whole trainable range, in alternating rounds on the same device, each round a window of many back-to-back calls between two device
events after a warm-up; medians over the rounds.  Each is also given as a share of an 8 TB/s stream of its own bytes: Adam reads
p, g, m, v and writes p, m, v (7 words per element), SGD reads p, g, buf and writes p, buf (5).  By the byte counts alone Adam
should take about 1.4x the SGD kernel's time.  The buffers (hundreds of MB each) do not fit any cache.  A report, not a gate.
    python tools/optim_probe.py [rounds] [calls per round]
Prints one JSON line."""
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

PEAK_BYTES_PER_S = 8e12


def window(fn, calls):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    c = bench.C2
    dims = ModelDims(V=c["V"], E=c["E"], H=c["H"], A=c["A"], F=c["F"], Z=c["Z"], S=1, kld_mode=1, pm_scale=0.5)
    eng = TrainEngine(dims, "cuda:0")
    lib = L.load()
    n = eng.params.numel
    g = torch.Generator(device="cuda").manual_seed(1)
    eng.params.flat.normal_(0, 0.05, generator=g)
    eng.grads.flat.normal_(0, 1e-3, generator=g)
    mom, m, v = (torch.zeros_like(eng.params.flat) for _ in range(3))
    sq = (eng.grads.flat.double() ** 2).sum().float().reshape(1)
    count = [0]

    def adam():
        count[0] += 1
        lib.ssc_adam_step(L.ptr(eng.params.flat), L.ptr(eng.grads.flat), L.ptr(m), L.ptr(v), n, L.ptr(sq), 1.0, 12.5, 5e-5, 0.9, 0.999,
                          1e-8, 0.0, 0, count[0], L.stream_ptr())

    def sgd():
        lib.ssc_sgd_step(L.ptr(eng.params.flat), L.ptr(eng.grads.flat), L.ptr(mom), n, L.ptr(sq), 1.0, 12.5, 1e-5, 0.9, 0.001, 0,
                         L.stream_ptr())

    t = {"adam": [], "sgd": []}
    for _ in range(rounds):
        t["adam"].append(window(adam, calls))
        t["sgd"].append(window(sgd, calls))
    out = {"elements": n, "rounds": rounds, "calls_per_round": calls}
    for k, words in (("adam", 7), ("sgd", 5)):
        ms = statistics.median(t[k])
        out[k + "_ms"] = round(ms, 4)
        out[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        out[k + "_share_of_8TBs"] = round(words * 4 * n / (ms * 1e-3) / PEAK_BYTES_PER_S, 3)
    out["adam_over_sgd"] = round(out["adam_ms"] / out["sgd_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
