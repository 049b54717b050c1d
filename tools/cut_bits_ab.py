#!/usr/bin/env python3
"""Bit-equality of two builds of libssc_hip.so on the word samplers' row kernels - the A/B behind a change that must not move a bit:
the same seeded inputs through the in-tree library and through a variant (tools/build_variant.py, e.g. of the parent commit), each in
a child process of its own, every output tensor compared on its int32 view.
Kernel inputs: every (V, ld, offset) of tests/test_truncation_gpu.py's SHAPES with its seven rows (random, peaked, flat, tied, 30 %
-inf, ended, empty) at temperatures 0.7, 1 and 1.3 - ssc_truncate_rows kinds 1 to 4 (edited block, entropy, kept), ssc_mirostat_rows
(edited block, kept, norm) and ssc_mirostat_update on its result (mu', surprise), ssc_sample_rows kinds 0 to 2 (token, log-prob,
probs); ssc_beam_step_sampled at the shapes of tests/test_sampled_beam_gpu.py (V 51, 10 000, 40 000; every kind, both replacement
modes, n in {1, 2, 5}: candidates, tokens, log-probs, back-pointers).  One-call inputs on a small model: DecodeEngine.sample with a
truncation, Mirostat and a contrast all on (tokens, log-probs, every statistics block) and one scheduled-sampling train step (loss,
kld, fed ids, fed mask, every gradient).
    python tools/cut_bits_ab.py <variant dir under style-seqcvae_amd, e.g. _base>
Prints one JSON line: the tensors compared and the names of those that differ; exit code 1 if any does."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "style-seqcvae_amd")
SHAPES = [(37, 37, 0), (451, 452, 1), (1024, 1028, 0), (1024, 1028, 1), (2003, 2004, 0), (10000, 10000, 0), (32768, 32768, 0),
          (32769, 32772, 1), (40000, 40000, 0)]   # test_truncation_gpu.SHAPES, V = 1024 at both offsets
TEMPS = (0.7, 1.0, 1.3)
TRUNC_VALUE = {1: 0.87654, 2: 0.05, 3: 3e-4, 4: 3e-4}
END = 1


def rows_case(V, ld, seed):
    """the seven rows of test_truncation_gpu.rows_case"""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = np.full((7, ld), np.nan, dtype=np.float32)
    x[0, :V] = rng.standard_normal(V) * 3
    x[1, :V] = rng.standard_normal(V)
    x[1, V // 3] = 25.0
    x[2, :V] = -1.25
    x[3, :V] = np.round(rng.standard_normal(V) * 3 * 2) / 2
    x[3, [1, V // 2, V - 1]] = x[3, :V].max() + 0.5
    x[4, :V] = rng.standard_normal(V) * 3
    x[4, :V][rng.random(V) < 0.3] = -np.inf
    x[6, :V] = -np.inf
    last = np.full(7, 7, dtype=np.int64)
    last[5] = END
    return x, last


def dump(path):
    sys.path[:0] = [ROOT, PKG]
    import numpy as np
    import torch
    from ssc_runtime import lib as L
    from ssc_runtime import sampling
    from ssc_runtime.contrast import Contrast
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    lib = L.load()
    dev = "cuda"
    out = {}

    def keep(name, t):
        assert name not in out, name
        out[name] = t.detach().cpu().contiguous().view(-1).view(torch.int32).clone()

    # ---- the row kernels ------------------------------------------------------------------------------------------------------
    for V, ld, off in SHAPES:
        for T in TEMPS:
            tag = f"V{V}+{off}/T{T}"
            x, last = rows_case(V, ld, 1000 * V + int(T * 10))
            flat = torch.full((x.size + off + 4,), float("nan"), device=dev)
            master = torch.from_numpy(x).reshape(-1).to(dev)
            view = flat[off: off + x.size]
            last_d = torch.from_numpy(last).to(dev)
            for kind in (1, 2, 3, 4):
                view.copy_(master)
                ent = torch.full((7,), -7.0, device=dev)
                kept = torch.full((7,), -99, dtype=torch.int32, device=dev)
                t = L.Truncation(kind, float(np.float32(TRUNC_VALUE[kind])), ent.data_ptr(), kept.data_ptr())
                lib.ssc_truncate_rows(view.data_ptr(), ld, 7, V, C.byref(t), T, L.ptr(last_d), END, L.stream_ptr())
                keep(f"truncate/{tag}/kind{kind}/rows", flat)
                keep(f"truncate/{tag}/kind{kind}/entropy", ent)
                keep(f"truncate/{tag}/kind{kind}/kept", kept)
            view.copy_(master)
            mu = torch.tensor([2.0, 0.5, 20.0, 4.0, 6.0, 3.0, 3.0], device=dev)
            kept = torch.full((7,), -99, dtype=torch.int32, device=dev)
            norm = torch.full((2, 7), -7.0, device=dev)
            lib.ssc_mirostat_rows(view.data_ptr(), ld, 7, V, T, L.ptr(mu), L.ptr(last_d), END, L.ptr(kept), L.ptr(norm), L.stream_ptr())
            keep(f"mirostat_rows/{tag}/rows", flat)
            keep(f"mirostat_rows/{tag}/kept", kept)
            keep(f"mirostat_rows/{tag}/norm", norm)
            pred = torch.nan_to_num(view.view(7, ld)[:, :V], nan=-float("inf")).argmax(1)   # a kept word of every live row
            mu2 = torch.full((7,), -7.0, device=dev)
            sur = torch.full((7,), -7.0, device=dev)
            lib.ssc_mirostat_update(view.data_ptr(), ld, 7, V, T, 3.0, 0.1, L.ptr(norm), L.ptr(pred), L.ptr(last_d), END, L.ptr(mu), L.ptr(mu2),
                                    L.ptr(sur), L.stream_ptr())
            keep(f"mirostat_update/{tag}/mu", mu2)
            keep(f"mirostat_update/{tag}/surprise", sur)
            # (the draw is not made for rows of NaN: the five live rows, in place, with ld as the stride)
            for name, s in (("multinomial", sampling.MultinomialSampler(temperature=T)), ("top_k", sampling.TopKSampler(k=min(40, V), temperature=T)),
                            ("top_p", sampling.TopPSampler(p=0.9, temperature=T))):
                tok = torch.empty(5, dtype=torch.int64, device=dev)
                lp = torch.empty(5, device=dev)
                po = torch.empty(5, V, device=dev)
                view.copy_(master)
                lib.ssc_sample_rows(L.ptr(view), ld, 5, V, s.desc(7), None, 2, None, None, END, L.ptr(tok), L.ptr(lp), L.ptr(po), L.stream_ptr())
                keep(f"sample_rows/{tag}/{name}/tok", tok)
                keep(f"sample_rows/{tag}/{name}/lp", lp)
                keep(f"sample_rows/{tag}/{name}/probs", po)
    # ---- the sampled-node beam's step ---------------------------------------------------------------------------------------------
    B, k = 4, 5
    for V in (51, 10000, 40000):
        rng = np.random.default_rng(V)
        for kind, mk in (("multinomial", lambda T, r: sampling.MultinomialSampler(temperature=T, with_replacement=r)),
                         ("top_k", lambda T, r: sampling.TopKSampler(k=7, temperature=T, with_replacement=r)),
                         ("top_p", lambda T, r: sampling.TopPSampler(p=0.7, temperature=T, with_replacement=r))):
            for rep in (False, True):
                for n, T in ((1, 1.0), (2, 0.7), (5, 1.6)):
                    logits = torch.from_numpy((rng.standard_normal((B * k, V)) * 2.5).astype(np.float32)).to(dev)
                    last = rng.integers(0, V, B * k)
                    last[rng.random(B * k) < 0.3] = END
                    last_d = torch.from_numpy(last.astype(np.int64)).to(dev)
                    phi = torch.from_numpy(rng.uniform(-12, -1, B * k).astype(np.float32)).to(dev)
                    bufs = dict(pred=torch.empty(B, k, dtype=torch.int64, device=dev), lp=torch.empty(B, k, device=dev),
                                backptr=torch.empty(B, k, dtype=torch.int64, device=dev), cand_lp=torch.empty(B * k * n, device=dev),
                                cand_tok=torch.empty(B * k * n, dtype=torch.int64, device=dev))
                    d = L.BeamDesc()
                    d.scores, d.ld, d.raw_logits, d.dims = L.ptr(logits), V, 1, L.FsmDims(0, 1, V, 0, 1)
                    d.B, d.beam, d.per_node, d.end_index, d.step_index = B, k, n, END, 3
                    d.pred, d.lp_out, d.backptr = L.ptr(bufs["pred"]), L.ptr(bufs["lp"]), L.ptr(bufs["backptr"])
                    d.scratch_val, d.scratch_idx = L.ptr(bufs["cand_lp"]), L.ptr(bufs["cand_tok"])
                    d.last_pred, d.last_lp = L.ptr(last_d), L.ptr(phi)
                    lib.ssc_beam_step_sampled(d, mk(T, rep).desc(1000 + n), 1 if rep else 0, L.stream_ptr())
                    for name, t in bufs.items():
                        keep(f"beam_step_sampled/V{V}/{kind}/rep{int(rep)}/n{n}/{name}", t)
    # ---- the one-call decode and the train step on a small model ----------------------------------------------------------------------
    torch.manual_seed(0)
    V, F, E, H, A, Z, Lc = 1200, 64, 40, 48, 32, 16, 8
    model = UpDownCaptioner(Vocabulary.synthetic(V), F, E, H, A, max_caption_length=Lc, beam_size=1, z_space=Z, sentiment_vae=1,
                            senti_prior_multip=0.5, device=torch.device(dev)).to(dev)
    with torch.no_grad():
        model._output_layer.weight.mul_(24.0)   # (as initialised the rows are nearly uniform: no cut would drop a word)
    eng = model._engine()
    dec = model._dec
    g = torch.Generator().manual_seed(5)
    nimg, ns, R = 3, 4, 6
    Bd = nimg * ns
    feats = torch.randn(nimg, R, F, generator=g).to(dev)
    sent_b = torch.ones(Bd, device=dev)
    eps0 = torch.randn(Bd, Z, generator=g).to(dev)
    eps = torch.randn(Lc - 1, Bd, Z, generator=g).to(dev)
    ctx = dec.prepare(feats)
    res = dec.sample(ctx, sent_b, ns, Lc, END, eps0, eps, sampling.TopPSampler(p=0.9, temperature=1.2), 13, early_stop=False,
                     truncation=sampling.TypicalTruncation(0.9), truncation_stats=True, contrast=Contrast(1.0, 0.1, latent="mean"),
                     contrast_stats=True, mirostat=sampling.Mirostat(3.0, 0.1), mirostat_stats=True)
    flat = []
    for r in res:
        flat += list(r) if isinstance(r, (tuple, list)) else [r]
    for i, t in enumerate(flat):
        keep(f"decode_sample/out{i}", t)
    Bt = 6
    caps = torch.zeros(Bt, Lc, dtype=torch.long)
    for b in range(Bt):
        n = 3 + b % 5
        caps[b, :n] = torch.randint(2, V, (n,), generator=g)
    tf = torch.randn(Bt, R, F, generator=g).to(dev)
    senti = torch.randint(-1, 2, (Bt, 1), generator=g).float().to(dev)
    teps = torch.randn(Lc + 1, Bt, Z, generator=g).to(dev)
    loss, kld = eng.forward(tf, caps.to(dev), senti, teps, ss_prob=0.5, ss_sampler=sampling.TopPSampler(p=0.9), ss_seed=11)
    keep("sched_train/loss", loss)
    keep("sched_train/kld", kld)
    keep("sched_train/input_tokens", eng.input_tokens())
    keep("sched_train/fed_mask", eng.fed_mask().to(torch.int32))
    eng.backward(torch.full((Bt,), 1.0 / Bt, device=dev), torch.full((Bt,), 1.0 / (Bt * 750.0), device=dev))
    for name, t in sorted(eng.grad_dict().items()):
        keep(f"sched_train/grad/{name}", t)
    torch.cuda.synchronize()
    torch.save(out, path)


def compare(script, variant_dir):
    """The two-process driver (shared with tools/ce_bits_ab.py): `script --dump PATH` - which saves a dict name -> int32 tensor - runs
    once against the in-tree library and once against style-seqcvae_amd/<variant_dir>/libssc_hip.so, each a fresh child process; prints
    the JSON line and exits 1 if any tensor differs."""
    variant = os.path.join(PKG, variant_dir, "libssc_hip.so")
    assert os.path.exists(variant), variant
    import torch
    with tempfile.TemporaryDirectory() as td:
        got = {}
        for name, env in (("tree", {}), ("variant", {"SSC_DEBUG": "1", "SSC_LIB_PATH": variant})):
            path = os.path.join(td, name + ".pt")
            subprocess.run([sys.executable, os.path.abspath(script), "--dump", path], env={**os.environ, **env}, check=True, timeout=900)
            got[name] = torch.load(path)
    a, b = got["tree"], got["variant"]
    assert list(a) == list(b)
    differ = [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]
    groups = {}
    for k in a:
        groups[k.split("/")[0]] = groups.get(k.split("/")[0], 0) + 1
    print(json.dumps({"variant": variant_dir, "tensors": len(a), "words": int(sum(t.numel() for t in a.values())), "by_entry": groups,
                      "differ": differ}))
    sys.exit(1 if differ else 0)


def main(dump):
    if sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    compare(sys.argv[0], sys.argv[1])


if __name__ == "__main__":
    main(dump)
