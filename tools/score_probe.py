#!/usr/bin/env python3
"""Time of caption scoring: (a) the row kernel alone (score_rows_kernel through ssc_score_rows) on (10 000, 10 000) logits, as
microseconds and as the share of an 8 TB/s stream of its 400 MB, next to a device copy of the same bytes; (b) one whole scoring call
(ssc_decode_score) at the bench's decode shape - 100 images x 5 captions x 20 latent samples = 10 000 rows, 36 x 2048 features,
V 10 000, H 1200, 20 steps, captions of 20 words so that no row ends early - next to the sampled decode (ssc_decode_sample,
multinomial, early stop off) at the same rows and steps, which forms the same step products.  Alternating rounds on the same
device; medians.
    python tools/score_probe.py [calls per round] [rounds]
Prints one JSON line."""
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
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner

HBM_BYTES_PER_S = 8e12


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
    out = {"calls_per_round": calls, "rounds": rounds}

    # (a) the row kernel alone
    G, V = 10000, c["V"]
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    logits = torch.randn(G, V, device=dev, generator=g) * 3
    target = torch.randint(0, V, (G,), device=dev, generator=g)
    last = torch.zeros(G, dtype=torch.int64, device=dev)
    lp = torch.empty(G, device=dev)
    rank = torch.empty(G, dtype=torch.int32, device=dev)
    dst = torch.empty_like(logits)

    def rows(with_rank):
        lib.ssc_score_rows(L.ptr(logits), V, G, V, L.ptr(target), L.ptr(last), 1, None, L.ptr(lp), L.ptr(rank) if with_rank else None,
                           L.stream_ptr())
    us = {"lp": [], "lp_rank": [], "copy": []}
    for _ in range(rounds):
        us["lp"].append(timed(lambda: rows(False), 20) * 1e3)
        us["lp_rank"].append(timed(lambda: rows(True), 20) * 1e3)
        us["copy"].append(timed(lambda: dst.copy_(logits), 20) * 1e3)
    nbytes = G * V * 4
    out["row_kernel"] = {"rows": G, "V": V, "bytes": nbytes}
    for k in ("lp", "lp_rank"):
        m = statistics.median(us[k])
        out["row_kernel"][k] = {"us": m, "min": min(us[k]), "max": max(us[k]), "GBps": nbytes / m / 1e3,
                                "share_of_8TBps": nbytes / (m * 1e-6) / HBM_BYTES_PER_S}
    m = statistics.median(us["copy"])
    out["row_kernel"]["copy_read_write"] = {"us": m, "one_pass_GBps": 2 * nbytes / m / 1e3}
    del logits, dst

    # (b) one scoring call next to the sampled decode at the same rows and steps
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), c["F"], c["E"], c["H"], c["A"], max_caption_length=c["L"], beam_size=1,
                            z_space=c["Z"], sentiment_vae=1, senti_prior_multip=0.5, device=dev).to(dev).eval()
    model._engine()
    dec = model._dec
    dec.weights_frozen = True
    images, n_caps, n_z, steps = 100, 5, 20, c["L"]
    rpi = n_caps * n_z
    B = images * rpi
    gc = torch.Generator().manual_seed(4321)
    feats = torch.randn(images, c["R"], c["F"], generator=gc).to(dev)
    sent = torch.ones(B, device=dev)
    caps = torch.randint(2, V, (images, n_caps, steps), generator=gc).to(dev)   # 20 words, no END: every row runs every step
    eps0 = torch.randn(B, c["Z"], device=dev, generator=g)
    eps = torch.randn(steps - 1, B, c["Z"], device=dev, generator=g)
    ctx = dec.prepare(feats)
    smp = sampling.MultinomialSampler()
    run_score = lambda: dec.score(ctx, sent, caps, n_z, 1, eps0, eps)
    run_score_all = lambda: dec.score(ctx, sent, caps, n_z, 1, eps0, eps, want_tokens=True, want_ranks=True)
    run_sample = lambda: dec.sample(ctx, sent, rpi, steps, 1, eps0, eps, smp, seed=7, early_stop=False)
    ms = {"score": [], "score_tokens_ranks": [], "sample": []}
    for _ in range(rounds):
        ms["sample"].append(timed(run_sample, calls))
        ms["score"].append(timed(run_score, calls))
        ms["score_tokens_ranks"].append(timed(run_score_all, calls))
    pred, _ = run_sample()
    out["call"] = {"images": images, "captions": n_caps, "samples": n_z, "rows": B, "steps": steps,
                   "sampled_rows_that_ended": int((pred == 1).any(-1).sum().item())}
    for k, v in ms.items():
        out["call"][k] = {"ms_per_call": statistics.median(v), "min": min(v), "max": max(v)}
    out["call"]["score_over_sample"] = out["call"]["score"]["ms_per_call"] / out["call"]["sample"]["ms_per_call"]
    out["wall_s"] = time.perf_counter() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
