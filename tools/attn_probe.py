#!/usr/bin/env python3
"""Cost of the attention trace in the C4 decode call (bench.py --mode decode: 100 images x 20 latent samples x beam 5 = 10 000 rows,
36 x 2048 features, 20 steps, early stop off so that every round runs the same steps): diverse_decode with the trace off, with
attention="summary" and with attention="full" on the same build, device, parameters and images, in alternating rounds, medians.
Off and on issue the same decode steps - a traced step writes its attention weights to the caller's history instead of to the
workspace -; on adds the history's allocation (steps x rows x R floats), the ancestry kernel and one gather of the 2000 returned
captions.  "gather_all": the gather of ALL 10 000 captions of the last record, maps included, on its own.
    python tools/attn_probe.py [calls per round] [rounds] [images per call]
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime.inference import diverse_decode
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
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    images = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    c = dict(bench.C2)
    device = torch.device("cuda", 0)
    torch.manual_seed(2)
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), image_feature_size=c["F"], embedding_size=c["E"], hidden_size=c["H"],
                            attention_projection_size=c["A"], max_caption_length=c["L"], beam_size=5, z_space=c["Z"], prior_std=1.0,
                            simple_vae=False, latent_embedding="glove", sentiment_vae=1, senti_prior_multip=0.5, device=device).to(device)
    model.eval()
    model._engine()
    dec = model._dec
    dec.weights_frozen = True
    g = torch.Generator().manual_seed(4321)
    feats = [torch.randn(images, c["R"], c["F"], generator=g).to(device) for _ in range(2)]
    senti = torch.ones(images, device=device)
    n_z, beam = 20, 5

    def call(mode):
        def run(i):
            diverse_decode(dec, feats[i % len(feats)], senti, n_z, beam, c["L"], 1, early_stop=False, attention=mode)
        return run

    modes = {"off": None, "summary": "summary", "full": "full"}
    for mode in modes.values():   # out of idle, every kernel form loaded
        timed(call(mode), 4)
    res = {k: [] for k in modes}
    for _ in range(rounds):
        for k, mode in modes.items():
            res[k].append(timed(call(mode), calls))
    # the gather of every caption of one record, on its own
    ctx = dec.prepare(feats[0])
    B = images * n_z
    gen = torch.Generator(device=device)
    gen.manual_seed(1)
    eps0 = torch.randn(B, c["Z"], device=device, generator=gen)
    eps = torch.randn(c["L"] - 1, B * beam, c["Z"], device=device, generator=gen)
    _, _, rec = dec.search(ctx, senti.repeat_interleave(n_z), n_z, beam, 2, c["L"], 1, eps0, eps, early_stop=False, attention=True)
    dec.attention(rec)
    gather_all = [timed(lambda i: dec.attention(rec), 20) for _ in range(rounds)]
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"shape": "C4", "images_per_call": images, "rows": B * beam, "calls_per_round": calls, "rounds": rounds,
           "hist_MB": rec.hist.numel() * 4 / 1e6}
    for k, v in res.items():
        out[k + "_ms"] = {"median": med(v), "min": min(v), "max": max(v)}
    out["summary_cost_ms"] = med(res["summary"]) - med(res["off"])
    out["full_cost_ms"] = med(res["full"]) - med(res["off"])
    out["summary_cost_pct"] = 100.0 * out["summary_cost_ms"] / med(res["off"])
    out["full_cost_pct"] = 100.0 * out["full_cost_ms"] / med(res["off"])
    out["gather_all_ms"] = {"median": med(gather_all), "min": min(gather_all), "max": max(gather_all)}
    moved = rec.rows * rec.steps * (2 * rec.R + 4) * 4
    out["gather_all_GBps"] = moved / med(gather_all) / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
