#!/usr/bin/env python3
"""Time of one self-critical training step (ssc_runtime/scst.py) at C2 widths - 32 images x 5 samples = 160 rows, 36 x 2048
features, V 10 000, H 1200, up to 20 steps - split into its legs: the sampled decode (prepare + ssc_decode_sample), the reward
(ssc_eval_score), ssc_scst_prepare, and the train step (forward + backward + clip + SGD) on the sampled captions.  Next to it, in
alternating rounds on the same device, TrainEngine.train_step on the same 160 rows and captions: that entry point's kernels are
not touched by the self-critical step, so the same build stands for the commit before it.  The legs are timed with their inputs
held fixed; the parameters and momentum are put back after every timed round of a leg that updates them.  Medians.
    python tools/scst_probe.py [rounds] [calls per round]
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
from ssc_runtime import sampling
from ssc_runtime.evaluation import CaptionReferences, _eval_score
from ssc_runtime.scst import BASELINES, SelfCritical, scst_prepare
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner

HP = dict(lr=0.015, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=12.5)


def timed(fn, n, restore=None):
    fn()   # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    if restore is not None:
        restore()
    return e0.elapsed_time(e1) / n


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    c = dict(bench.C2)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    t0 = time.perf_counter()
    P, N, steps = 32, 5, c["L"]
    G = P * N
    vocabulary = Vocabulary.synthetic(c["V"])
    model = UpDownCaptioner(vocabulary, c["F"], c["E"], c["H"], c["A"], max_caption_length=steps, beam_size=1, z_space=c["Z"],
                            sentiment_vae=1, senti_prior_multip=0.5, device=dev).to(dev).train()
    eng = model._engine()
    dec = model._dec
    g = torch.Generator().manual_seed(4321)
    feats = torch.randn(P, c["R"], c["F"], generator=g).to(dev)
    senti = torch.randint(-1, 2, (P,), generator=g).float().to(dev)
    refs = {p: [" ".join(f"w{int(t)}" for t in torch.randint(2, c["V"], (12,), generator=g)) for _ in range(5)] for p in range(P)}
    scst = SelfCritical(eng, dec, CaptionReferences(refs, device=dev), vocabulary, n_samples=N, max_steps=steps)
    ids = list(range(P))
    params0 = eng.params.flat.clone()
    eng.momentum = torch.zeros_like(eng.params.flat)   # (what the first clip_sgd_step would create)
    mom0 = eng.momentum.clone()

    def restore():
        eng.params.flat.copy_(params0)
        eng.momentum.copy_(mom0)

    ro = scst.rollout(feats, ids, senti, 7)
    L = ro.predictions.size(1)
    smp = sampling.MultinomialSampler()

    def leg_decode():
        ctx = dec.prepare(feats)
        dec.sample(ctx, ro.sentiment, N, steps, scst.end_index, ro.eps0, ro.eps, smp, 7)

    def leg_reward():
        _eval_score(scst._prep, ro.predictions.view(P, N, L), scst.end_index, scst._V, scst._id_map, None, ro.ref_image)

    def leg_prepare():
        scst_prepare(ro.predictions, ro.scores, None, scst.end_index, L, BASELINES["loo"], scst.reward_weights, 1.0 / G,
                     1.0 / (G * HP["kld_weight"]))

    def leg_train():
        eng.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps)
        eng.backward_update(ro.gl, ro.gk, HP["lr"], HP["momentum"], HP["weight_decay"], HP["max_norm"])

    def whole_step():
        scst.step(feats, ids, senti, seed=7, **HP)

    def xe_step():
        eng.train_step(ro.feats, ro.caps, ro.sentiment, ro.train_eps, **HP)

    legs = {"decode": (leg_decode, None), "reward": (leg_reward, None), "scst_prepare": (leg_prepare, None),
            "train": (leg_train, restore), "scst_step": (whole_step, restore), "train_step_160_rows": (xe_step, restore)}
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, rs) in legs.items():
            ms[k].append(timed(fn, calls, rs))
    out = {"P": P, "N": N, "rows": G, "steps": steps, "columns_sampled": L, "rounds": rounds, "calls_per_round": calls,
           "rows_without_end": float(ro.stats[3].item())}
    for k, v in ms.items():
        out[k] = {"ms": statistics.median(v), "min": min(v), "max": max(v)}
    legsum = sum(out[k]["ms"] for k in ("decode", "reward", "scst_prepare", "train"))
    out["legs_sum_ms"] = legsum
    out["prepare_share_of_step"] = out["scst_prepare"]["ms"] / out["scst_step"]["ms"]
    out["step_over_train_step"] = out["scst_step"]["ms"] / out["train_step_160_rows"]["ms"]
    out["wall_s"] = time.perf_counter() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
