#!/usr/bin/env python3
"""Cost of knowledge distillation at the C2 train step's widths (bench.py: T * B = 1344 rows, V = 10000, ld = the train
workspace's padded V; about four fifths of the rows carry a target).
Kernels: the ssc_ce_fwd_distill + ssc_ce_bwd_distill pair (alpha 0.5, at temperature 2 and at temperature 1) against the
ssc_ce_fwd_smooth + ssc_ce_bwd_smooth pair on the same student rows, and a device copy of the bytes each pair moves - by bytes
the smoothed pair moves 3 row-matrices (the forward reads one, the backward reads and writes one), the distilled pair 5 (each also
reads the teacher's); rows without a target cost one written row.  Alternating rounds on one device, each a window of many
back-to-back pairs between two device events after a warm-up; medians and min / max over the rounds.
Step: TrainEngine.train_step at C2 plain, and distilled from M = 1 and M = 2 frozen teachers of the same architecture
(DistillTeacher: M teacher forwards and, for M = 2, one ssc_ensemble_combine_rows per step, all inside the timed window).
A report, not a gate.
    python tools/distill_probe.py [--rounds N] [--pairs N] [--steps N] [--no-step]
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
from ssc_runtime.distill import DistillTeacher
from ssc_runtime.engine import ModelDims, TrainEngine


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
    teacher = torch.randn(rows, ld, device="cuda", generator=g) * 3.0
    tg = torch.randint(0, V, (T, B), device="cuda", generator=g)
    # caption lengths uniform in [0.6 T, T]: four fifths of the rows are live
    w = (torch.arange(T, device="cuda").view(T, 1) < torch.randint(3 * T // 5, T + 1, (1, B), device="cuda", generator=g)).float().contiguous()
    nv = w.sum(0).contiguous()
    gl = torch.full((B,), 1.0 / B, device="cuda")
    lse = torch.empty(3 * rows, device="cuda")
    loss, nll = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    scratch = torch.empty(3 * rows + B, device="cuda")
    P = L.ptr
    live = int(w.sum().item())
    dead = rows - live

    def smooth():
        st = L.stream_ptr()
        lib.ssc_ce_fwd_smooth(P(logits), ld, P(tg), P(w), P(nv), T, B, V, 0.1, P(lse), P(loss), P(nll), st)
        lib.ssc_ce_bwd_smooth(P(logits), ld, P(tg), P(w), P(nv), P(lse), P(gl), T, B, V, 0.1, st)

    def distill(tau):
        d = L.Distill(teacher.data_ptr(), ld, 0.5, tau, scratch.data_ptr(), scratch[3 * rows:].data_ptr())

        def pair():
            st = L.stream_ptr()
            lib.ssc_ce_fwd_distill(P(logits), ld, P(tg), P(w), P(nv), T, B, V, 0.1, C.byref(d), P(lse), P(loss), P(nll), st)
            lib.ssc_ce_bwd_distill(P(logits), ld, P(tg), P(w), P(nv), P(lse), P(gl), T, B, V, 0.1, C.byref(d), st)
        return pair

    nbytes = {"smooth": (3 * live + dead) * V * 4, "distill": (5 * live + dead) * V * 4}

    def copy_of(n):   # a device copy that moves n bytes: n / 2 read, n / 2 written
        a_, b_ = torch.empty(n // 8, device="cuda"), torch.empty(n // 8, device="cuda")
        return lambda: b_.copy_(a_)

    variants = {"smooth": smooth, "distill_tau2": distill(2.0), "distill_tau1": distill(1.0), "copy_smooth": copy_of(nbytes["smooth"]),
                "copy_distill": copy_of(nbytes["distill"])}

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
    out = {"rows": rows, "V": V, "ld": ld, "live_rows": live, "rounds": a.rounds, "pairs_per_round": a.pairs, "bytes": nbytes}
    for k, v in t.items():
        out[k] = med(v)
        out[k]["GBps"] = round(nbytes["smooth" if k.endswith("smooth") else "distill"] / (out[k]["us"] * 1e-6) / 1e9, 1)
    out["distill_tau2_over_smooth"] = round(out["distill_tau2"]["us"] / out["smooth"]["us"], 3)
    out["distill_tau1_over_smooth"] = round(out["distill_tau1"]["us"] / out["smooth"]["us"], 3)
    out["copy_distill_over_copy_smooth"] = round(out["copy_distill"]["us"] / out["copy_smooth"]["us"], 3)
    return out


def steps(a):
    c = bench.C2
    dims = ModelDims(V=c["V"], E=c["E"], H=c["H"], A=c["A"], F=c["F"], Z=c["Z"], S=1, kld_mode=1, pm_scale=0.5)
    engs = []
    for seed in (2, 3, 4):   # the student and two teachers: the same architecture, other weights
        torch.manual_seed(seed)
        e = TrainEngine(dims, "cuda")
        e.params.flat.copy_(torch.randn_like(e.params.flat) * 0.02)
        engs.append(e)
    student = engs[0]
    batches = [bench.synth_batch(1234 + 100 * i, c["B"], c["R"], c["F"], c["L"], c["V"], c["Z"], "cuda") for i in range(4)]
    teachers = {1: DistillTeacher(engs[1:2], student_dims=dims), 2: DistillTeacher(engs[1:3], (0.7, 0.3), "prob", student_dims=dims)}

    def step(i, M):
        feats, caps, senti, eps = batches[i % len(batches)]
        d = teachers[M].distill(feats, caps, senti, eps, 0.5, 2.0) if M else None
        student.train_step(feats, caps, senti, eps, lr=1e-4, label_smoothing=0.1, distill=d)

    def window(M):
        step(0, M)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.steps):
            step(i, M)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1e3   # us per step

    for M in (0, 1, 2):
        window(M)
    t = {M: [] for M in (0, 1, 2)}
    for _ in range(a.rounds):
        for M in t:
            t[M].append(window(M))
    out = {"steps_per_round": a.steps, "plain": med(t[0]), "one_teacher": med(t[1]), "two_teachers": med(t[2])}
    out["one_teacher_over_plain"] = round(out["one_teacher"]["us"] / out["plain"]["us"], 3)
    out["two_teachers_over_plain"] = round(out["two_teachers"]["us"] / out["plain"]["us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="the kernel pairs only")
    a = ap.parse_args()
    out = {"kernels": kernels(a)}
    if not a.no_step:
        out["step"] = steps(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
