#!/usr/bin/env python3
"""Times the diverse subset selection ssc_eval_select (MBR, MMR, greedy DPP; ssc_runtime.evaluation.select_captions) at P = 1000
images x N = 100 candidates, k = 5 and k = 20, and - in the same run, as the yardstick - ssc_eval_set producing the caption kernels
the selection reads.   python tools/select_probe.py [--images P] [--samples N] [--repeats R]
Every call reads a device flag back, so events around a call cover its kernels and that read.  All shapes are warmed up first; the
timed rounds alternate between the calls, so a disturbance on the shared host hits all of them alike; median and minimum over the
rounds are printed, and the ratio selection / kernel building of the medians."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssc_runtime import evaluation as E  # noqa: E402
from ssc_runtime import lib as Lb  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--images", type=int, default=1000)
p.add_argument("--samples", type=int, default=100)
p.add_argument("--length", type=int, default=20)
p.add_argument("--vocab", type=int, default=10000)
p.add_argument("--ref-images", type=int, default=2000, help="images of the reference set the document frequencies come from")
p.add_argument("--repeats", type=int, default=20)
p.add_argument("--ks", type=int, nargs="+", default=[5, 20])
a = p.parse_args()

rng = np.random.default_rng(0)
P, N, V, Lmax = a.images, a.samples, a.vocab, a.length
dev = torch.device("cuda", 0)
zipf = lambda size: np.minimum(rng.zipf(1.3, size=size), V - 3) + 1   # noqa: E731  (word frequencies as in captions)
# references as compact ids (= token id - 1), 5 per image
ref_off, tok_off, toks = [0], [0], []
for _ in range(a.ref_images):
    for _ in range(5):
        toks += [int(t) - 1 for t in zipf(int(rng.integers(8, Lmax + 1)))]
        tok_off.append(len(toks))
    ref_off.append(len(tok_off) - 1)
prep = E._Prepared.from_csr(ref_off, tok_off, toks, V - 1, dev)
id_map = torch.tensor([0, 0] + list(range(1, V - 1)), dtype=torch.int32, device=dev)
# candidates: every fifth one repeats an earlier caption of its image (what a sampled decode returns)
pred = zipf((P, N, Lmax))
lens = rng.integers(8, Lmax + 1, size=(P, N, 1))
pred = np.where(np.arange(Lmax)[None, None, :] < lens, pred, 1).astype(np.int64)
pred[:, 4::5] = pred[:, 2::5][:, : pred[:, 4::5].shape[1]]
pt = torch.from_numpy(pred).to(dev)
quality = torch.from_numpy(rng.normal(size=(P, N))).to(dev)
ref_image = torch.zeros(P, dtype=torch.int32, device=dev)
lib = Lb.load()

cnt = torch.empty(P, N, 10, dtype=torch.int32, device=dev)
kern = torch.empty(P, N, N, dtype=torch.float64, device=dev)
eig = torch.empty(P, N, dtype=torch.float64, device=dev)
dist = torch.empty(P, dtype=torch.int32, device=dev)
sd = Lb.EvalSetDesc(Lb.ptr(pt), P, N, Lmax, 1, V, Lb.ptr(id_map), Lb.ptr(ref_image), Lb.ptr(cnt), Lb.ptr(kern), Lb.ptr(eig), Lb.ptr(dist))
set_bytes = lib.ssc_eval_set_workspace_bytes(ctypes.byref(prep.desc), ctypes.byref(sd))
set_ws = torch.empty(set_bytes, dtype=torch.uint8, device=dev)


def run_set():
    lib.ssc_eval_set(ctypes.byref(prep.desc), ctypes.byref(sd), Lb.ptr(set_ws), set_bytes, Lb.stream_ptr())


calls = {"ssc_eval_set (kernel + eigenvalues)": run_set}
keep = []
for k in a.ks:
    for name, method in (("mbr", 1), ("mmr", 2), ("dpp", 3)):
        picks = torch.empty(P, k, dtype=torch.int32, device=dev)
        gains = torch.empty(P, k, dtype=torch.float64, device=dev)
        nprim = torch.empty(P, dtype=torch.int32, device=dev)
        d = Lb.EvalSelectDesc(P, N, k, method, Lb.ptr(kern), Lb.ptr(quality), 1, 0.5, 1.0, 1e-10, None, Lb.ptr(picks), Lb.ptr(gains),
                              Lb.ptr(nprim))
        nbytes = lib.ssc_eval_select_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        keep.append((picks, gains, nprim, d, ws))
        calls[f"ssc_eval_select {name} k={k}"] = (lambda d=d, ws=ws, nbytes=nbytes:
                                                  lib.ssc_eval_select(ctypes.byref(d), Lb.ptr(ws), nbytes, Lb.stream_ptr()))

for fn in calls.values():   # warm-up: every shape once (the first also fills the kernel matrices the selections read)
    fn()
torch.cuda.synchronize()
ms = {name: [] for name in calls}
for _ in range(a.repeats):
    for name, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1))
print(f"{P} images x {N} candidates, captions <= {Lmax} words, V {V}; {a.repeats} alternating rounds; events around each call "
      f"(its kernels + the flag read)")
base = float(np.median(ms["ssc_eval_set (kernel + eigenvalues)"]))
for name, v in ms.items():
    print(f"{name}: median {np.median(v):.3f} ms, min {np.min(v):.3f} ms, ratio to ssc_eval_set {np.median(v) / base:.4f}")
npr = keep[-1][2].cpu().numpy()
print(f"dpp k={a.ks[-1]}: picks made by the rule itself per image: mean {npr.mean():.2f}, min {npr.min()}")
