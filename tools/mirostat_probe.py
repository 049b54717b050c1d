#!/usr/bin/env python3
"""Cost of Mirostat for the word samplers (ssc_mirostat) at C4's word-sampling call - 100 images x 20 latent samples (2000 rows),
36 x 2048 features, V 10 000, H 1200, 20 steps, top-p 0.9, early stop off so every call runs all its steps: the time per call of
ssc_decode_sample without Mirostat, under Mirostat (tau 3 bits, eta 0.1 - and tau 13 bits, which on the nearly uniform rows of weights
as initialised keeps every word, so that the captions are the plain call's and the difference is the launches alone) and under the
min-p truncation (0.05) for scale, the same noise and seed, in alternating rounds on one device - medians with min and max -; then
the kernels alone on (2000, V) logits restored before every launch, the restoring copy's own time taken off: the cut
(ssc_mirostat_rows) against ssc_truncate_rows min-p on the same rows, in alternating rounds, and the update (ssc_mirostat_update).
    python tools/mirostat_probe.py [calls] [rounds]
Prints one JSON line."""
import ctypes as C
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
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


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
    miro = sampling.Mirostat(3.0, 0.1)
    run = lambda **kw: (lambda: dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, **kw))
    runs = (("sample", run()), ("mirostat_3_0.1", run(mirostat=miro)), ("mirostat_13_0.1", run(mirostat=sampling.Mirostat(13.0, 0.1))),
            ("min_p_0.05", run(truncation=sampling.MinPTruncation(0.05))))
    out = {"images": images, "n_z": n_z, "rows": B, "max_steps": steps, "V": V, "calls_per_round": calls, "rounds": rounds,
           "rounds_ms": {name: [] for name, _ in runs}}
    for _ in range(rounds):
        for name, fn in runs:
            out["rounds_ms"][name].append(timed(fn, calls))
    for name, _ in runs:
        s = spread(out["rounds_ms"][name])
        out[name] = {"median_ms_per_call": s["median"], "min": s["min"], "max": s["max"]}
    base = out["sample"]["median_ms_per_call"]
    out["ratio_to_sample"] = {name: out[name]["median_ms_per_call"] / base for name, _ in runs[1:]}
    _, _, (mu, sur, kept) = dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, mirostat=miro, mirostat_stats=True)
    plain = dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False)[0]
    wide = dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, mirostat=sampling.Mirostat(13.0, 0.1))[0]
    out["mirostat_13_equals_sample"] = bool(torch.equal(plain, wide))
    live = kept > 0
    out["mirostat_stats"] = {"mean_kept": float(kept[live].float().mean()), "mean_surprise_bits": float(sur[live].mean()),
                             "mean_surprise_bits_last_half": float(sur[:, steps // 2:][live[:, steps // 2:]].mean()),
                             "mean_mu_bits": float(mu[live].mean()), "tau_bits": miro.tau}
    # the kernels alone: logits restored from a master copy before every launch (an edited row would be cheaper to edit again)
    lib = L.load()
    master = torch.randn(B, V, device=dev) * 3
    logits = torch.empty_like(master)
    mu_d = torch.full((B,), 6.0, device=dev)     # (about the median surprise of such rows: a proper cut)
    norm = torch.zeros(2, B, device=dev)
    pred = torch.zeros(B, dtype=torch.int64, device=dev)
    td = sampling.MinPTruncation(0.05).desc()

    def cut():
        logits.copy_(master)
        lib.ssc_mirostat_rows(L.ptr(logits), V, B, V, 1.0, L.ptr(mu_d), None, 1, None, L.ptr(norm), L.stream_ptr())

    def minp():
        logits.copy_(master)
        lib.ssc_truncate_rows(L.ptr(logits), V, B, V, C.byref(td), 1.0, None, 1, L.stream_ptr())

    k = {"copy": [], "mirostat_rows": [], "min_p": []}
    for _ in range(rounds):
        k["copy"].append(timed(lambda: logits.copy_(master), 50) * 1e3)
        k["mirostat_rows"].append(timed(cut, 50) * 1e3)
        k["min_p"].append(timed(minp, 50) * 1e3)
    us_copy = spread(k["copy"])["median"]
    out["kernel"] = {"rows": B, "V": V, "bytes_read_and_written": 2 * B * V * 4, "restore_copy_us": spread(k["copy"])}
    for name in ("mirostat_rows", "min_p"):
        s = spread([v - us_copy for v in k[name]])
        out["kernel"][name] = {"us": s, "GBps": 2 * B * V * 4 / s["median"] / 1e3}
    out["kernel"]["ratio_mirostat_rows_to_min_p"] = out["kernel"]["mirostat_rows"]["us"]["median"] / out["kernel"]["min_p"]["us"]["median"]
    cut()
    upd = lambda: lib.ssc_mirostat_update(L.ptr(logits), V, B, V, 1.0, 2.0, 0.1, L.ptr(norm), L.ptr(pred), None, 1, L.ptr(mu_d), L.ptr(mu_d), None,
                                          L.stream_ptr())
    out["kernel"]["mirostat_update_us"] = spread([timed(upd, 50) * 1e3 for _ in range(rounds)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
