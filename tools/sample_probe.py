#!/usr/bin/env python3
"""Time of the sampled decode (ssc_decode_sample) against the beam-1 and beam-5 searches (ssc_decode_search) at the bench's decode
shape - 100 images x 20 latent samples per call, 36 x 2048 features, V 10 000, H 1200, max 20 steps, early stop off so every call
runs all its steps -, the stochastic beam search at beam 5 (ssc_decode_stochastic_beam), the sampled-node beam search at beam 5,
per-node 2 for each word sampler with and without replacement (ssc_decode_sampled_beam), and of the selections alone
(sample_rows_kernel through ssc_sample_rows, ssc_beam_step_gumbel, ssc_beam_step_sampled) on (G, V) logits, with their logits
bytes / time against one HBM pass.
    python tools/sample_probe.py [calls]
    python tools/sample_probe.py diverse-beam [calls] [rounds]
    python tools/sample_probe.py rules-beam [calls] [rounds]
    python tools/sample_probe.py word-rules [calls] [rounds]
The diverse-beam leg alone: the time per call of ssc_decode_diverse_beam (k = 6 in 3 groups, per-node 1) next to ssc_decode_search
(k = 6, per-node 3: the logits path) on the same inputs, in alternating rounds on the same device, and the two selections alone
(ssc_beam_step_fsm, ssc_beam_step_diverse) on the same (G * 6, V) logits - their share of a step.
The rules-beam leg alone, at C4's shapes (beam 5, per-node 2): the time per call of ssc_decode_search (at this size its later steps
read per-tile records, not logits), of ssc_decode_rules_beam with every rule off and of ssc_decode_rules_beam with n = 3,
alpha = 1, min_length = 5, suppress = [0] (both on the (G, V) logits), in alternating rounds on the same device and inputs.
The word-rules leg alone, at C4's word-sampling call (2000 rows, top-p 0.9): the time per call of ssc_decode_sample, of the same call
under logit rules without a bias (n = 3, min_length = 5, theta = 1.2, presence 0.2, frequency 0.1, suppress = [0]: the sparse
kernel) and with a per-image bias as well (the streaming kernel), in alternating rounds on the same device and inputs; then the
bias kernel alone on (2000, V) logits next to a device copy that moves the same bytes (3 x rows x V x 4: two reads, one write).
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
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


def diverse_beam_leg(dec, feats, senti, images, n_z, steps, c, calls, rounds):
    """Alternating rounds of `calls` one-call searches each: beam search k 6 / per-node 3 and diverse beam search k 6 / 3 groups /
    per-node 1, early stop off (all steps run), the same noise; then the selection kernels alone."""
    dev = feats.device
    k, B = 6, images * n_z
    G = B * k
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    eps0 = torch.randn(B, c["Z"], device=dev, generator=gen)
    eps = torch.randn(steps - 1, G, c["Z"], device=dev, generator=gen)
    sent_b = senti.view(images, 1).expand(images, n_z).reshape(B).contiguous()
    ctx = dec.prepare(feats)
    div = sampling.DiverseBeam(3, 0.5)
    run_beam = lambda: dec.search(ctx, sent_b, n_z, k, 3, steps, 1, eps0, eps, skip_dead=True, early_stop=False)
    run_div = lambda: dec.diverse_beam(ctx, sent_b, n_z, k, 1, steps, 1, eps0, eps, div, skip_dead=True, early_stop=False)
    out = {"images": images, "n_z": n_z, "beam": k, "max_steps": steps, "V": c["V"], "calls_per_round": calls,
           "beam_search_ms": [], "diverse_beam_ms": []}
    for _ in range(rounds):
        out["beam_search_ms"].append(timed(run_beam, calls))
        out["diverse_beam_ms"].append(timed(run_div, calls))
    for key in ("beam_search_ms", "diverse_beam_ms"):
        v = out[key]
        out[key.replace("_ms", "")] = {"ms_per_call": sum(v) / len(v), "min": min(v), "max": max(v)}
    # the selections alone on the same logits: step 1 of a search whose beams are all live
    lib = L.load()
    V = c["V"]
    big = torch.randn(G, V, device=dev) * 3
    bd = L.BeamDesc()
    bd.scores, bd.ld, bd.raw_logits, bd.dims = L.ptr(big), V, 1, L.FsmDims(B, 1, V, 0, 1)
    bd.B, bd.beam, bd.end_index, bd.step_index = B, k, 1, 1
    m = 1 + k - k // 3
    bufs = [torch.zeros(G, dtype=torch.int64, device=dev), torch.full((G,), -5.0, device=dev), torch.empty(G, dtype=torch.int64, device=dev),
            torch.empty(G, device=dev), torch.empty(G, dtype=torch.int64, device=dev), torch.empty(G * max(m, 3), device=dev),
            torch.empty(G * max(m, 3), dtype=torch.int64, device=dev)]
    bd.last_pred, bd.last_lp, bd.pred, bd.lp_out, bd.backptr, bd.scratch_val, bd.scratch_idx = [L.ptr(b) for b in bufs]
    dd = div.desc()

    def beam_step():
        bd.per_node = 3
        lib.ssc_beam_step_fsm(bd, L.stream_ptr())

    def div_step():
        bd.per_node = 1
        lib.ssc_beam_step_diverse(bd, dd, L.stream_ptr())
    out["selection"] = {"G": G, "list": m}
    for _ in range(rounds):
        for name, fn in (("beam_step_us", beam_step), ("diverse_step_us", div_step)):
            out["selection"].setdefault(name, []).append(timed(fn, 20) * 1e3)
    out["selection"]["logits_bytes"] = G * V * 4
    return out


def rules_beam_leg(dec, feats, senti, images, n_z, steps, c, calls, rounds):
    """Alternating rounds of `calls` one-call searches each at beam 5 / per-node 2, early stop off (all steps run), the same noise:
    the beam search, the search under rules with every rule off, and with n-gram blocking, a minimum length, a suppressed token
    and a length penalty."""
    dev = feats.device
    k, n, B = 5, 2, images * n_z
    G = B * k
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    eps0 = torch.randn(B, c["Z"], device=dev, generator=gen)
    eps = torch.randn(steps - 1, G, c["Z"], device=dev, generator=gen)
    sent_b = senti.view(images, 1).expand(images, n_z).reshape(B).contiguous()
    ctx = dec.prepare(feats)
    off = sampling.DecodeRules()
    on = sampling.DecodeRules(no_repeat_ngram=3, min_length=5, length_alpha=1.0, suppress=(0,))
    runs = (("beam_search", lambda: dec.search(ctx, sent_b, n_z, k, n, steps, 1, eps0, eps, skip_dead=True, early_stop=False)),
            ("rules_off", lambda: dec.rules_beam(ctx, sent_b, n_z, k, n, steps, 1, eps0, eps, off, skip_dead=True, early_stop=False)),
            ("rules_on", lambda: dec.rules_beam(ctx, sent_b, n_z, k, n, steps, 1, eps0, eps, on, skip_dead=True, early_stop=False)))
    out = {"images": images, "n_z": n_z, "beam": k, "per_node": n, "rows_per_step": G, "max_steps": steps, "V": c["V"],
           "calls_per_round": calls, "rounds_ms": {name: [] for name, _ in runs}}
    for _ in range(rounds):
        for name, fn in runs:
            out["rounds_ms"][name].append(timed(fn, calls))
    for name, _ in runs:
        v = out["rounds_ms"][name]
        out[name] = {"ms_per_call": sum(v) / len(v), "min": min(v), "max": max(v)}
    base = out["beam_search"]["ms_per_call"]
    out["ratio_to_beam_search"] = {name: out[name]["ms_per_call"] / base for name in ("rules_off", "rules_on")}
    return out


def word_rules_leg(dec, feats, senti, images, n_z, steps, c, calls, rounds):
    """Alternating rounds of `calls` one-call sampled decodes each (top-p 0.9, early stop off, the same noise and seed): without
    rules, under rules without a bias, under rules with a per-image bias; then the bias kernel alone against a copy."""
    import ctypes as C
    dev = feats.device
    B, V = images * n_z, c["V"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    eps0 = torch.randn(B, c["Z"], device=dev, generator=gen)
    eps = torch.randn(steps - 1, B, c["Z"], device=dev, generator=gen)
    sent_b = senti.view(images, 1).expand(images, n_z).reshape(B).contiguous()
    ctx = dec.prepare(feats)
    smp = sampling.TopPSampler(p=0.9)
    kw = dict(no_repeat_ngram=3, min_length=5, suppress=(0,), repetition_penalty=1.2, presence_penalty=0.2, frequency_penalty=0.1)
    sparse = sampling.LogitRules(**kw)
    biased = sampling.LogitRules(bias=torch.randn(images, V, device=dev, generator=gen), **kw)
    run = lambda lr: (lambda: dec.sample(ctx, sent_b, n_z, steps, 1, eps0, eps, smp, 7, early_stop=False, logit_rules=lr))
    runs = (("sample", run(None)), ("rules_no_bias", run(sparse)), ("rules_image_bias", run(biased)))
    out = {"images": images, "n_z": n_z, "rows": B, "max_steps": steps, "V": V, "calls_per_round": calls,
           "rounds_ms": {name: [] for name, _ in runs}}
    for _ in range(rounds):
        for name, fn in runs:
            out["rounds_ms"][name].append(timed(fn, calls))
    for name, _ in runs:
        v = sorted(out["rounds_ms"][name])
        out[name] = {"median_ms_per_call": v[len(v) // 2], "min": v[0], "max": v[-1]}
    base = out["sample"]["median_ms_per_call"]
    out["ratio_to_sample"] = {name: out[name]["median_ms_per_call"] / base for name in ("rules_no_bias", "rules_image_bias")}
    # the bias kernel alone (step 0: no history) against a copy of the same bytes - x and the bias read, x written
    lib = L.load()
    logits = torch.randn(B, V, device=dev) * 3
    full = torch.randn(B, V, device=dev)
    rd, _keep = sampling.LogitRules(bias=full).desc(1)
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    rd.bias_row = rows.data_ptr()
    us = timed(lambda: lib.ssc_logit_rules_rows(L.ptr(logits), V, B, V, C.byref(rd), None, B, 0, 1, L.stream_ptr()), 50) * 1e3
    dst = torch.empty(3 * B * V // 2, device=dev)
    src = torch.randn(3 * B * V // 2, device=dev)
    us_copy = timed(lambda: dst.copy_(src), 50) * 1e3
    out["bias_kernel"] = {"rows": B, "V": V, "bytes": 3 * B * V * 4, "us": us, "GBps": 3 * B * V * 4 / us / 1e3,
                          "copy_same_bytes_us": us_copy, "ratio_to_copy": us / us_copy}
    return out


def main():
    leg = len(sys.argv) > 1 and sys.argv[1] in ("diverse-beam", "rules-beam", "word-rules") and sys.argv[1]
    if leg:
        del sys.argv[1]
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    c = dict(bench.C2)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = UpDownCaptioner(Vocabulary.synthetic(c["V"]), c["F"], c["E"], c["H"], c["A"], max_caption_length=c["L"], beam_size=5,
                            z_space=c["Z"], sentiment_vae=1, senti_prior_multip=0.5, device=dev).to(dev).eval()
    model._engine()
    dec = model._dec
    dec.weights_frozen = True
    g = torch.Generator().manual_seed(4321)
    images, n_z, steps = 100, 20, c["L"]
    feats = torch.randn(images, c["R"], c["F"], generator=g).to(dev)
    senti = torch.ones(images, device=dev)
    if leg == "word-rules":
        print(json.dumps(word_rules_leg(dec, feats, senti, images, n_z, steps, c, calls, int(sys.argv[2]) if len(sys.argv) > 2 else 3)))
        return
    if leg == "rules-beam":
        print(json.dumps(rules_beam_leg(dec, feats, senti, images, n_z, steps, c, calls, int(sys.argv[2]) if len(sys.argv) > 2 else 3)))
        return
    if leg:
        print(json.dumps(diverse_beam_leg(dec, feats, senti, images, n_z, steps, c, calls, int(sys.argv[2]) if len(sys.argv) > 2 else 3)))
        return
    out = {"images": images, "n_z": n_z, "max_steps": steps, "V": c["V"]}
    t0 = time.perf_counter()
    for name, beam, sampler in (("beam5", 5, None), ("beam1", 1, None), ("top_p_0.9", 1, sampling.TopPSampler(p=0.9)),
                                ("top_k_40", 1, sampling.TopKSampler(k=40)), ("multinomial", 1, sampling.MultinomialSampler()),
                                ("stochastic_beam5", 5, sampling.GumbelSampler())):
        ms = timed(lambda: diverse_decode(dec, feats, senti, n_z, beam, steps, 1, early_stop=False, sampler=sampler), calls)
        out[name] = {"ms_per_call": ms, "us_per_step": ms * 1e3 / steps}
    for name, mk in (("multinomial", lambda r: sampling.MultinomialSampler(with_replacement=r)),
                     ("top_k_40", lambda r: sampling.TopKSampler(k=40, with_replacement=r)),
                     ("top_p_0.9", lambda r: sampling.TopPSampler(p=0.9, with_replacement=r))):
        for r in (False, True):
            sampler = mk(r)
            ms = timed(lambda: diverse_decode(dec, feats, senti, n_z, 5, steps, 1, early_stop=False, sampler=sampler, sampled_beam=True),
                       calls)
            out[f"sampled_beam5_{name}_{'with' if r else 'without'}_replacement"] = {"ms_per_call": ms, "us_per_step": ms * 1e3 / steps}
    # the row sampler alone on (G, V) logits
    lib = L.load()
    G, V = images * n_z, c["V"]
    logits = torch.randn(G, V, device=dev) * 3
    pred = torch.empty(G, dtype=torch.int64, device=dev)
    lp = torch.empty(G, dtype=torch.float32, device=dev)
    out["row_kernel"] = {"G": G, "V": V}
    for name, s in (("multinomial", sampling.MultinomialSampler()), ("top_k_40", sampling.TopKSampler(k=40)),
                    ("top_p_0.9", sampling.TopPSampler(p=0.9))):
        d = s.desc(7)

        def run():
            lib.ssc_sample_rows(L.ptr(logits), V, G, V, d, None, 1, None, None, 1, L.ptr(pred), L.ptr(lp), None, L.stream_ptr())
        us = timed(run, 50) * 1e3
        out["row_kernel"][name] = {"us": us, "GBps": G * V * 4 / us / 1e3}
    # the stochastic beam search's selection alone (row kernel + merge, ssc_beam_step_gumbel) on (G * 5, V) logits, beam 5, per-node 2
    Gs, k, n = G * 5, 5, 2
    big = torch.randn(Gs, V, device=dev) * 3
    bd = L.BeamDesc()
    bd.scores, bd.ld, bd.raw_logits, bd.dims = L.ptr(big), V, 1, L.FsmDims(0, 1, V, 0, 1)
    bd.B, bd.beam, bd.per_node, bd.end_index, bd.step_index = G, k, n, 1, 1
    bufs = [torch.zeros(Gs, dtype=torch.int64, device=dev), torch.full((Gs,), -5.0, device=dev), torch.empty(Gs, dtype=torch.int64, device=dev),
            torch.empty(Gs, device=dev), torch.empty(Gs, dtype=torch.int64, device=dev), torch.empty(2 * Gs * n, device=dev),
            torch.empty(Gs * n, dtype=torch.int64, device=dev), torch.full((Gs,), -4.0, device=dev), torch.empty(Gs, device=dev)]
    bd.last_pred, bd.last_lp, bd.pred, bd.lp_out, bd.backptr, bd.scratch_val, bd.scratch_idx = [L.ptr(b) for b in bufs[:7]]
    gd = sampling.GumbelSampler().desc(7)
    us = timed(lambda: lib.ssc_beam_step_gumbel(bd, gd, L.ptr(bufs[7]), L.ptr(bufs[8]), L.stream_ptr()), 20) * 1e3
    out["row_kernel"]["stochastic_beam_step"] = {"G": Gs, "us": us, "GBps": Gs * V * 4 / us / 1e3}
    # the sampled-node beam search's selection alone (row kernel + merge, ssc_beam_step_sampled), same logits, beam 5, per-node 2
    for name, s, r in (("multinomial", sampling.MultinomialSampler(), 0), ("multinomial_with_replacement", sampling.MultinomialSampler(), 1),
                       ("top_k_40", sampling.TopKSampler(k=40), 0), ("top_p_0.9", sampling.TopPSampler(p=0.9), 0)):
        sd = s.desc(7)
        us = timed(lambda: lib.ssc_beam_step_sampled(bd, sd, r, L.stream_ptr()), 20) * 1e3
        out["row_kernel"][f"sampled_beam_step_{name}"] = {"G": Gs, "us": us, "GBps": Gs * V * 4 / us / 1e3}
    del big
    # one HBM pass over the same bytes (a device copy reads and writes them: half its time is the read)
    dst = torch.empty_like(logits)
    us_copy = timed(lambda: dst.copy_(logits), 50) * 1e3
    out["row_kernel"]["copy_read_write_us"] = us_copy
    out["row_kernel"]["one_pass_GBps_from_copy"] = 2 * G * V * 4 / us_copy / 1e3
    out["wall_s"] = time.perf_counter() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
