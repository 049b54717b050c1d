#!/usr/bin/env python3
"""Cost and effect of arithmetic sampling for the word samplers (ssc_arith) at C4's word-sampling call - 100 images x 20 latent
samples (2000 rows), 36 x 2048 features, V 10 000, H 1200, 20 steps, full width, early stop off so every call runs all its steps.
Per sampler kind (multinomial, top-k 50, top-p 0.9) a run of its own: the time per call of ssc_decode_sample with the sampler's own
draw and with the arithmetic draw along the lattice, the same noise and seed, in alternating rounds on one device - medians with min
and max, and their ratio (boxes differ by a few per cent: only the ratio inside one run means anything).
Then the diversity of the 20 captions per image - Unique and mBLEU-4 (ssc_eval_set) - with all samples of an image sharing one latent
(share_latent=True), along the lattice and along independent uniform codes (each caption the same exact draw, not stratified), at
temperatures low enough for the random-weight model's captions to repeat.
    python tools/arith_probe.py [calls] [rounds] [temperature ...]
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
from ssc_runtime import sampling
from ssc_runtime.evaluation import set_diversity
from ssc_runtime.inference import diverse_decode
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    temps = [float(t) for t in sys.argv[3:]] or [0.02, 0.01, 0.005]
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
    lattice = sampling.Arithmetic()
    out = {"images": images, "n_z": n_z, "rows": B, "max_steps": steps, "V": V, "calls_per_round": calls, "rounds": rounds, "timing": {}}
    samplers = (("multinomial", sampling.MultinomialSampler(1.0)), ("top-k_50", sampling.TopKSampler(k=50)),
                ("top-p_0.9", sampling.TopPSampler(p=0.9)))
    for name, smp in samplers:   # each sampler kind a run of its own
        run = lambda **kw: (lambda: dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, **kw))
        legs = (("plain", run()), ("arithmetic", run(arithmetic=lattice)))
        ms = {leg: [] for leg, _ in legs}
        for _ in range(rounds):
            for leg, fn in legs:
                ms[leg].append(timed(fn, calls))
        t = {leg: spread(v) for leg, v in ms.items()}
        t["ratio_arithmetic_to_plain"] = t["arithmetic"]["median"] / t["plain"]["median"]
        t["rounds_ms"] = ms
        out["timing"][name] = t
    # diversity of an image's 20 captions, one latent per image: the lattice against independent uniform codes
    senti = torch.ones(images, device=dev)
    out["diversity"] = {}
    for T in temps:
        smp = sampling.MultinomialSampler(T)
        cg = torch.Generator().manual_seed(99)
        iid = torch.randint(-2 ** 63, 2 ** 63 - 1, (B,), dtype=torch.int64, generator=cg).to(dev)
        rec = {}
        for leg, ar in (("lattice", sampling.Arithmetic(share_latent=True)), ("independent_codes", sampling.Arithmetic(iid, share_latent=True))):
            torch.manual_seed(5)
            pred, _ = diverse_decode(dec, feats, senti, n_z, 1, steps, 1, sampler=smp, sample_seed=7, arithmetic=ar)
            s = set_diversity(pred, 1, V).summary()
            rec[leg] = {"unique": s["unique"], "mBLEU-4": s["mBLEU-4"], "steps": int(pred.size(-1))}
        out["diversity"][f"T_{T}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
