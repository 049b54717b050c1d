#!/usr/bin/env python3
"""Time of ssc_ensemble_combine_rows alone at the decode bench's shape - 10 000 rows x V 10 000 -, M = 2 and 4 members, both modes:
microseconds per call and the achieved GB/s against M * rows * V * 4 bytes read + rows * V * 4 bytes written (one HBM pass over
every member and the output; the kernel's further passes over a row are meant to hit L2), next to a device copy of the same
number of bytes.
    python tools/ensemble_probe.py [rows] [V]
Prints one JSON line."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
import torch

from ssc_runtime import lib as L


def timed(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    dev = torch.device("cuda", 0)
    lib = L.load()
    torch.manual_seed(0)
    members = [torch.randn(rows, V, device=dev) * 3 for _ in range(4)]
    out_buf = torch.empty(rows, V, device=dev)
    out = {"rows": rows, "V": V}
    for M in (2, 4):
        ptrs = (C.c_void_p * M)(*[m.data_ptr() for m in members[:M]])
        logw = (C.c_float * M)(*([float(torch.log(torch.tensor(1.0 / M)))] * M))
        nbytes = (M + 1) * rows * V * 4
        for mode, name in ((0, "prob"), (1, "logprob")):
            d = L.EnsembleRowsDesc(M, ptrs, V, logw, mode)

            def run():
                lib.ssc_ensemble_combine_rows(C.byref(d), rows, V, None, None, 0, L.ptr(out_buf), V, L.stream_ptr())
            us = timed(run, 20) * 1e3
            out[f"M{M}_{name}"] = {"us": us, "GBps": nbytes / us / 1e3, "bytes": nbytes}
        # a device copy that moves the same number of bytes (half read, half written)
        n = (M + 1) * rows * V // 2
        src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
        us_copy = timed(lambda: dst.copy_(src), 20) * 1e3
        out[f"M{M}_copy_same_bytes"] = {"us": us_copy, "GBps": nbytes / us_copy / 1e3}
        del src, dst
    print(json.dumps(out))


if __name__ == "__main__":
    main()
