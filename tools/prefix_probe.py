#!/usr/bin/env python3
"""Cost of prompted decoding at the bench's decode shape - 100 images x 20 latent samples per call, 36 x 2048 features, V 10 000,
H 1200, beam 5, 20 steps, early stop off so every call runs all its steps: one prefixed decode call (ssc_decode_prime of Lp words
on the 2000 rows, ssc_decode_search with the start state, ssc_prefix_join) against the same call without a prefix, in alternating
rounds on the same device and inputs, and priming alone.  The expectation from the code: Lp extra steps at 1 / (S * beam) of the
search's rows.
    python tools/prefix_probe.py [calls] [rounds] [Lp]
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime.prefix import join_prefix
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
    Lp = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    c = dict(bench.C2)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), c["F"], c["E"], c["H"], c["A"], max_caption_length=c["L"], beam_size=5,
                            z_space=c["Z"], sentiment_vae=1, senti_prior_multip=0.5, device=dev).to(dev).eval()
    model._engine()
    dec = model._dec
    dec.weights_frozen = True
    g = torch.Generator().manual_seed(4321)
    images, n_z, beam, per, steps = 100, 20, 5, 2, c["L"]
    B = images * n_z
    feats = torch.randn(images, c["R"], c["F"], generator=g).to(dev)
    sent_b = torch.ones(B, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    eps0 = torch.randn(B, c["Z"], device=dev, generator=gen)
    eps = torch.randn(steps - 1, B * beam, c["Z"], device=dev, generator=gen)
    peps = torch.randn(Lp, B, c["Z"], device=dev, generator=gen)
    prefix = torch.randint(2, c["V"], (images, Lp), generator=g).to(dev).repeat_interleave(n_z, 0)
    ctx = dec.prepare(feats)

    def plain():
        return dec.search(ctx, sent_b, n_z, beam, per, steps, 1, eps0, eps, skip_dead=True, early_stop=False)

    def prime():
        return dec.prime(ctx, sent_b, n_z, prefix, 1, peps)

    def prefixed():
        start = prime()
        pred, lps = dec.search(ctx, sent_b, n_z, beam, per, steps, 1, eps0, eps, skip_dead=True, early_stop=False, start=start)
        return join_prefix(prefix, start, pred.view(B, beam, -1), lps.view(B, beam), 1)

    out = {"images": images, "n_z": n_z, "beam": beam, "max_steps": steps, "Lp": Lp, "V": c["V"], "calls_per_round": calls,
           "plain_ms": [], "prefixed_ms": [], "prime_ms": []}
    for _ in range(rounds):
        out["plain_ms"].append(timed(plain, calls))
        out["prefixed_ms"].append(timed(prefixed, calls))
        out["prime_ms"].append(timed(prime, calls))
    med = lambda v: sorted(v)[len(v) // 2]
    for key in ("plain_ms", "prefixed_ms", "prime_ms"):
        v = out[key]
        out[key[:-3]] = {"median_ms_per_call": med(v), "min": min(v), "max": max(v)}
    out["prefix_cost_ms"] = out["prefixed"]["median_ms_per_call"] - out["plain"]["median_ms_per_call"]
    out["prefix_cost_percent"] = 100.0 * out["prefix_cost_ms"] / out["plain"]["median_ms_per_call"]
    out["expected_percent"] = 100.0 * Lp / (steps * beam)   # Lp steps at 1 / beam of the rows of a search step
    print(json.dumps(out))


if __name__ == "__main__":
    main()
