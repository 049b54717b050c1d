#!/usr/bin/env python3
"""Cost of contrastive decoding (ssc_contrast) at C4's word-sampling call - 100 images x 20 latent samples (2000 rows), 36 x 2048
features, V 10 000, H 1200, 20 steps, top-p 0.9, early stop off so every call runs all its steps: the time per call of
ssc_decode_sample without a contrast, under the plausibility cut alone (alpha 0, beta 0.1: one row pass per step, no amateur) and
with an amateur stream (alpha 1, beta 0.1: mean features, and z at the prior mean), the same noise and seed, in alternating rounds
on one device - medians with min and max -; then the kernel alone (ssc_contrast_rows) on (2000, V) logits restored before every
launch, the restoring copy's own time taken off, with its bytes (two reads, one write of a block) per second next to a device copy.
    python tools/contrast_probe.py [calls] [rounds]
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bench
from sample_probe import timed
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.contrast import Contrast
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    c = dict(bench.C2)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), c["F"], c["E"], c["H"], c["A"], max_caption_length=c["L"], beam_size=5,
                            z_space=c["Z"], sentiment_vae=1, senti_prior_multip=0.5, device=dev).to(dev).eval()
    model._engine()
    dec = model._dec
    dec.weights_frozen = True
    g = torch.Generator().manual_seed(4321)
    images, n_z, steps, V = 100, 20, c["L"], c["V"]
    B = images * n_z
    feats = torch.randn(images, c["R"], c["F"], generator=g).to(dev)
    sent_b = torch.ones(B, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    eps0 = torch.randn(B, c["Z"], device=dev, generator=gen)
    eps = torch.randn(steps - 1, B, c["Z"], device=dev, generator=gen)
    ctx = dec.prepare(feats)
    smp = sampling.TopPSampler(p=0.9)
    kinds = (("cut_only_b0.1", Contrast(0.0, 0.1)), ("mean_features_a1_b0.1", Contrast(1.0, 0.1, features="mean").prepare(dec, ctx.feats)),
             ("prior_mean_a1_b0.1", Contrast(1.0, 0.1, latent="mean")))
    run = lambda k: (lambda: dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, contrast=k))
    runs = (("sample", run(None)),) + tuple((name, run(k)) for name, k in kinds)
    out = {"images": images, "n_z": n_z, "rows": B, "max_steps": steps, "V": V, "calls_per_round": calls, "rounds": rounds,
           "rounds_ms": {name: [] for name, _ in runs}}
    for _ in range(rounds):
        for name, fn in runs:
            out["rounds_ms"][name].append(timed(fn, calls))
    for name, _ in runs:
        v = sorted(out["rounds_ms"][name])
        out[name] = {"median_ms_per_call": v[len(v) // 2], "min": v[0], "max": v[-1]}
    base = out["sample"]["median_ms_per_call"]
    out["ratio_to_sample"] = {name: out[name]["median_ms_per_call"] / base for name, _ in kinds}
    _, _, (kept, div) = dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, contrast=kinds[1][1], contrast_stats=True)
    live = kept > 0
    out["mean_features_stats"] = {"mean_kept": float(kept[live].float().mean()), "mean_divergence_nats": float(div[live].mean())}
    # the kernel alone: the expert's logits restored from a master copy before every launch (the edit is in place)
    lib = L.load()
    master = torch.randn(B, V, device=dev) * 3
    amateur = master * 0.5 + torch.randn(B, V, device=dev)
    logits = torch.empty_like(master)
    us_copy = timed(lambda: logits.copy_(master), 50) * 1e3
    block = B * V * 4
    out["kernel"] = {"rows": B, "V": V, "block_bytes": block, "restore_copy_us": us_copy, "copy_GBps": 2 * block / us_copy / 1e3}
    for name, alpha, beta, am, blocks in (("a1_b0.1", 1.0, 0.1, amateur, 3), ("a1_b0", 1.0, 0.0, amateur, 3), ("a0_b0.1_no_amateur", 0.0, 0.1, None, 2)):
        def both():
            logits.copy_(master)
            lib.ssc_contrast_rows(L.ptr(logits), V, L.ptr(am), V, B, V, alpha, beta, None, 1, None, None, L.stream_ptr())
        us = timed(both, 50) * 1e3 - us_copy
        out["kernel"][name] = {"us": us, "GBps": blocks * block / us / 1e3, "ratio_to_copy": us / us_copy}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
