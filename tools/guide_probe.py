#!/usr/bin/env python3
"""Cost of a latent guide at the bench's decode call (C4): 100 images x 20 latent samples x beam 5 (per-node 2) = 10 000 rows,
36 x 2048 features, V 10 000, H 1200, 20 steps, early stop off - the beam search (ssc_decode_search) without a guide, with a guide
that has no variance (z = mean, no noise read) and with one that has (z = eps sqrt(var) + mean), in alternating rounds on the same
device; medians and the rounds' spread.  One launch replaces one launch per step, so the expectation is parity.  A search's work
depends on its captions (beams that share a parent share products, ssc_decode_step_desc.parent), and a guide changes the captions;
the leg "guided_same_z" therefore hands the prior itself as the guide (mean = pm_scale * sentiment, var = prior_var): the same z
bit for bit, the same captions (checked), so its difference to the unguided call is the guide's own cost.  Also the latent launch
alone on the (10 000, Z) rows of a later step: ssc_latent_prior_sample against ssc_latent_guide_rows.
    python tools/guide_probe.py [calls per round] [rounds]
Prints one JSON line."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime import lib as L
from ssc_runtime.guide import LatentGuide
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner


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
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    c = dict(bench.C2)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lib = L.load()
    t0 = time.perf_counter()
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), c["F"], c["E"], c["H"], c["A"], max_caption_length=c["L"], beam_size=5,
                            z_space=c["Z"], sentiment_vae=1, senti_prior_multip=0.5, device=dev).to(dev).eval()
    model._engine()
    dec = model._dec
    dec.weights_frozen = True
    images, n_z, beam, per_node, steps, Z = 100, 20, 5, 2, c["L"], c["Z"]
    B, G = images * n_z, images * n_z * beam
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    feats = torch.randn(images, c["R"], c["F"], device=dev, generator=g)
    sent = torch.ones(B, device=dev)
    eps0 = torch.randn(B, Z, device=dev, generator=g)
    eps = torch.randn(steps - 1, G, Z, device=dev, generator=g)
    mean = torch.randn(steps, B, Z, device=dev, generator=g)
    var = torch.rand(steps, B, Z, device=dev, generator=g) + 0.5
    same = LatentGuide(torch.full((steps, B, Z), 0.5, device=dev), torch.ones(steps, B, Z, device=dev))   # the prior of this model and sentiment
    guides = {"unguided": None, "guided_same_z": same, "guided_mean": LatentGuide(mean), "guided_var": LatentGuide(mean, var)}
    ctx = dec.prepare(feats)
    run = {k: (lambda gd=gd: dec.search(ctx, sent, n_z, beam, per_node, steps, 1, eps0, eps, early_stop=False, guide=gd))
           for k, gd in guides.items()}
    pred = {k: run[k]()[0] for k in run}
    ms = {k: [] for k in run}
    for _ in range(rounds):
        for k in run:
            ms[k].append(timed(run[k], calls))
    out = {"calls_per_round": calls, "rounds": rounds, "images": images, "samples": n_z, "beam": beam, "rows": G, "steps": steps, "Z": Z}
    for k, v in ms.items():
        out[k] = {"ms_per_call": statistics.median(v), "min": min(v), "max": max(v)}
    for k in ("guided_same_z", "guided_mean", "guided_var"):
        out[k + "_over_unguided"] = out[k]["ms_per_call"] / out["unguided"]["ms_per_call"]
        out[k + "_captions_equal_unguided"] = bool(torch.equal(pred[k], pred["unguided"]))

    # the latent launch alone, on the rows of a later step
    Zp = (Z + 3) // 4 * 4
    z = torch.empty(G, Zp, device=dev)
    sent_rows = torch.ones(G, device=dev)
    gd = L.LatentGuideDesc(steps, L.ptr(mean), L.ptr(var), Z, None)
    gm = L.LatentGuideDesc(steps, L.ptr(mean), None, Z, None)
    st = L.stream_ptr()
    launch = {
        "prior_sample": lambda: lib.ssc_latent_prior_sample(L.ptr(eps[3]), Z, L.ptr(sent_rows), 0.5, 1.0, G, Z, L.ptr(z), Zp, st),
        "guide_rows_mean": lambda: lib.ssc_latent_guide_rows(C.byref(gm), 4, G, beam, Z, L.ptr(eps[3]), Z, L.ptr(sent_rows), 0.5, 1.0, L.ptr(z), Zp, st),
        "guide_rows_var": lambda: lib.ssc_latent_guide_rows(C.byref(gd), 4, G, beam, Z, L.ptr(eps[3]), Z, L.ptr(sent_rows), 0.5, 1.0, L.ptr(z), Zp, st),
    }
    us = {k: [] for k in launch}
    for _ in range(rounds):
        for k in launch:
            us[k].append(timed(launch[k], 50) * 1e3)
    out["latent_launch_us"] = {k: {"us": statistics.median(v), "min": min(v), "max": max(v)} for k, v in us.items()}
    out["wall_s"] = time.perf_counter() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
