#!/usr/bin/env python3
"""Cost of scheduled sampling in the C2 train step (bench.py's shapes: B 64, 36 x 2048 features, L 20, V 10 000, E 1000, H 1200):
the fused step (forward + backward + clip + SGD) at ss_prob 0 against ss_prob P on the same build, device, parameters and
batches, in alternating rounds, and the two forwards alone.  With sampling the vocabulary head, the mix kernel and the
B x E x 4H block of the attention LSTM's input product run once per step inside the time loop: T - 1 more streams of the head
weight and of W_ih^att[:, :E] at M = B, and T - 1 mix launches.
    python tools/ss_probe.py [prob] [steps per round] [rounds]
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime.schedule import ss_seed
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    prob = float(sys.argv[1]) if len(sys.argv) > 1 else 0.25
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    c = dict(bench.C2)
    device = torch.device("cuda", 0)
    torch.manual_seed(2)
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), image_feature_size=c["F"], embedding_size=c["E"], hidden_size=c["H"],
                            attention_projection_size=c["A"], max_caption_length=c["L"], beam_size=5, z_space=c["Z"], prior_std=1.0,
                            simple_vae=False, latent_embedding="glove", sentiment_vae=1, senti_prior_multip=0.5, device=device).to(device)
    eng = model._engine()
    batches = [bench.synth_batch(1234 + 100 * i, c["B"], c["R"], c["F"], c["L"], c["V"], c["Z"], device) for i in range(4)]
    hp = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=12.5, decoder_frozen=False)

    def step(p):
        def run(i):
            feats, caps, senti, eps = batches[i % len(batches)]
            kw = dict(ss_prob=p, ss_seed=ss_seed(2, i + 1, 0)) if p > 0 else {}
            eng.train_step(feats, caps, senti, eps, **hp, **kw)
        return run

    def fwd(p):
        def run(i):
            feats, caps, senti, eps = batches[i % len(batches)]
            kw = dict(ss_prob=p, ss_seed=ss_seed(2, i + 1, 0)) if p > 0 else {}
            eng.forward(feats, caps, senti, eps, **kw)
        return run

    for p in (0.0, prob):   # out of idle, every kernel form loaded
        timed(step(p), 30)
    res = {"step_off": [], "step_on": [], "fwd_off": [], "fwd_on": []}
    for _ in range(rounds):
        res["step_off"].append(timed(step(0.0), steps))
        res["step_on"].append(timed(step(prob), steps))
        res["fwd_off"].append(timed(fwd(0.0), steps))
        res["fwd_on"].append(timed(fwd(prob), steps))
    feats, caps, senti, eps = batches[0]
    eng.forward(feats, caps, senti, eps, ss_prob=prob, ss_seed=1)
    n_weighted = int((caps != 0).sum()) + caps.size(0)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"shape": "C2", "prob": prob, "steps_per_round": steps, "rounds": rounds,
           "fed_share": float(eng.fed_mask().sum()) / n_weighted}
    for k, v in res.items():
        out[k + "_ms"] = {"median": med(v), "min": min(v), "max": max(v)}
    out["step_cost_ms"] = med(res["step_on"]) - med(res["step_off"])
    out["fwd_cost_ms"] = med(res["fwd_on"]) - med(res["fwd_off"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
