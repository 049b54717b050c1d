#!/usr/bin/env python3
"""Times the device caption evaluation (ssc_runtime.evaluation: ssc_eval_prepare_refs, ssc_eval_score) on a synthetic corpus of
5 000 images x 20 samples x 5 references, captions of up to 20 words over a 10 000-word vocabulary, and the float64 CPU
restatement (tests/captionevalref.py) on a slice of the same input for comparison.   python tools/eval_probe.py [--cpu-images K]
With --set (default on) it also times the caption-set call ssc_eval_set (mBLEU / Self-CIDEr / Unique) on the same predictions and
once at --set-samples captions per image, its host reduction, and the set restatement (tests/captionsetref.py) on the same slice.
Both library calls read a device flag back, so wall-clock time around a call is its whole cost; the kernels' own time comes from
events around the launches of a second call."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssc_runtime.evaluation import CaptionReferences  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--images", type=int, default=5000)
p.add_argument("--samples", type=int, default=20)
p.add_argument("--refs", type=int, default=5)
p.add_argument("--length", type=int, default=20)
p.add_argument("--vocab", type=int, default=10000)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--cpu-images", type=int, default=100, help="images of the CPU restatement's timed slice (0: skip)")
p.add_argument("--set", type=int, default=1, help="1: also time ssc_eval_set (0: skip)")
p.add_argument("--set-samples", type=int, default=100, help="captions per image of the second ssc_eval_set timing (0: skip)")
a = p.parse_args()

rng = np.random.default_rng(0)
I, N, V, Lmax = a.images, a.samples, a.vocab, a.length
words = ["@@UNKNOWN@@", "@@BOUNDARY@@"] + [f"w{i}" for i in range(2, V)]
zipf = lambda n: np.minimum(rng.zipf(1.3, size=n), V - 3) + 1   # noqa: E731  (word frequencies as in captions)
refs = {i: [" ".join(f"w{t}" for t in zipf(int(rng.integers(8, Lmax + 1)))) for _ in range(a.refs)] for i in range(I)}
pred = np.ones((I, N, Lmax), dtype=np.int64)
for i in range(I):
    for n in range(N):
        L = int(rng.integers(8, Lmax + 1))
        pred[i, n, :L] = zipf(L)
dev = torch.device("cuda", 0)
pt = torch.from_numpy(pred).to(dev)

cr = CaptionReferences(refs, device=dev)
ids = list(refs)
cr.score(pt, 1, words)   # warm-up: prepares the reference set, loads the kernels
prep, score = [], []
for _ in range(a.repeats):
    cr._prepared.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cr.prepared(ids)
    prep.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    res = cr.score(pt, 1, words)
    score.append(time.perf_counter() - t0)
# the library call alone (no host conversions, no copies back): events around ssc_eval_score's two kernels + flag read
import ctypes  # noqa: E402
from ssc_runtime import lib as Lb  # noqa: E402
prepd = cr.prepared(ids)
lib = Lb.load()
id_map = torch.tensor([cr.word_id.get(w, 0) for w in words], dtype=torch.int32, device=dev)
id_map[0] = 0
ref_image = torch.arange(I, dtype=torch.int32, device=dev)
sc = torch.empty(I, N, 6, dtype=torch.float64, device=dev)
cn = torch.empty(I, N, 10, dtype=torch.int32, device=dev)
im = torch.empty(I, 9, dtype=torch.int32, device=dev)
t5 = torch.empty(I, 5, dtype=torch.int32, device=dev)
ws = torch.empty(256, dtype=torch.uint8, device=dev)
d = Lb.EvalScoreDesc(Lb.ptr(pt), I, N, Lmax, 1, V, Lb.ptr(id_map), None, Lb.ptr(ref_image), Lb.ptr(sc), Lb.ptr(cn), Lb.ptr(im),
                     Lb.ptr(t5))
call = []
for _ in range(a.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    lib.ssc_eval_score(ctypes.byref(prepd.desc), ctypes.byref(d), Lb.ptr(ws), 256, Lb.stream_ptr())
    e1.record()
    torch.cuda.synchronize()
    call.append(e0.elapsed_time(e1))
s = res.summary()
print(f"corpus: {I} images x {N} samples x {a.refs} refs, captions <= {Lmax} words, V {V}; "
      f"{prepd.ntok} reference tokens, {int((pred != 1).sum())} candidate tokens")
print(f"prepare_refs (host CSR build + upload + 3 kernels + flag read): median {np.median(prep) * 1e3:.1f} ms")
print(f"score (CaptionReferences.score: uploads, 2 kernels, copies back, host reductions excluded): median {np.median(score) * 1e3:.1f} ms")
print(f"ssc_eval_score alone (events, 2 kernels + flag read): median {np.median(call):.2f} ms, min {np.min(call):.2f} ms")
t0 = time.perf_counter()
res.summary()
print(f"host reductions (summary()): {(time.perf_counter() - t0) * 1e3:.1f} ms")
print("cider", s["cider"], "mean cider", s["mean cider"], "B4", s["B4"], "Div-2", s["Div-2"])
if a.cpu_images:
    import captionevalref as R
    K = a.cpu_images
    tr = [[r.split() for r in refs[i]] for i in ids]
    t0 = time.perf_counter()
    cid = R.Cider(tr)   # document frequencies over all images
    t_df = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(K):
        for n in range(N):
            row = list(pred[i, n])
            c = [words[t] for t in row[: row.index(1) if 1 in row else len(row)]]
            R.bleu_from_stats(*R.bleu_stats(c, tr[i]))
            R.rouge_l(c, tr[i])
            cid.score(c, tr[i])
    t = time.perf_counter() - t0
    print(f"CPU restatement (float64 Python, one thread): document frequencies {t_df * 1e3:.0f} ms; {K} images x {N} samples "
          f"scored in {t:.2f} s -> {t * I / K:.0f} s for all {I} images (linear extrapolation)")


def time_set(pred_t, prep_desc, idm, refimg, label):
    """ssc_eval_set alone: events around the call (3 kernels + flag read), the kernel matrix kept in the workspace."""
    P_, N_, steps = pred_t.shape
    cnt = torch.empty(P_, N_, 10, dtype=torch.int32, device=dev)
    eig = torch.empty(P_, N_, dtype=torch.float64, device=dev)
    dist = torch.empty(P_, dtype=torch.int32, device=dev)
    sd = Lb.EvalSetDesc(Lb.ptr(pred_t), P_, N_, steps, 1, V, Lb.ptr(idm), Lb.ptr(refimg), Lb.ptr(cnt), None, Lb.ptr(eig), Lb.ptr(dist))
    nbytes = lib.ssc_eval_set_workspace_bytes(ctypes.byref(prep_desc), ctypes.byref(sd))
    wsp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib.ssc_eval_set(ctypes.byref(prep_desc), ctypes.byref(sd), Lb.ptr(wsp), nbytes, Lb.stream_ptr())   # warm-up
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.ssc_eval_set(ctypes.byref(prep_desc), ctypes.byref(sd), Lb.ptr(wsp), nbytes, Lb.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(f"ssc_eval_set alone, {label} ({P_} x {N_}, events, 3 kernels + flag read, workspace {nbytes / 2**20:.0f} MiB): "
          f"median {np.median(ms):.2f} ms, min {np.min(ms):.2f} ms")


if a.set:
    from ssc_runtime import evaluation as E  # noqa: E402
    time_set(pt, prepd.desc, id_map, ref_image, "the corpus above")
    t0 = time.perf_counter()
    res = cr.score(pt, 1, words, set_diversity=True)
    t_all = time.perf_counter() - t0
    t0 = time.perf_counter()
    sd_ = E.SetDiversity(res.set_stats, res.distinct, res.set_kernel, res.set_eigenvalues, range(I))
    ss = sd_.summary()
    print(f"score(set_diversity=True) (both calls, uploads, copies back incl. the kernel matrices): {t_all * 1e3:.1f} ms; "
          f"host reduction of the set numbers (Self-CIDEr per image, mBLEU, unique): {(time.perf_counter() - t0) * 1e3:.1f} ms")
    print({k: round(v, 6) for k, v in ss.items()}, "degenerate sets", sd_.degenerate_sets)
    if a.set_samples:
        Ns = a.set_samples
        big = np.minimum(rng.zipf(1.3, size=(I, Ns, Lmax)), V - 3) + 1
        lens = rng.integers(8, Lmax + 1, size=(I, Ns, 1))
        big = np.where(np.arange(Lmax)[None, None, :] < lens, big, 1).astype(np.int64)
        time_set(torch.from_numpy(big).to(dev), prepd.desc, id_map, ref_image, f"N = {Ns}")
    if a.cpu_images:
        import captionsetref as S
        K = a.cpu_images
        caps = [[[words[t] for t in list(row)[: list(row).index(1) if 1 in row else len(row)]] for row in pred[i]] for i in range(K)]
        t0 = time.perf_counter()
        df, n_img = S.reference_df([[r.split() for r in refs[i]] for i in ids])   # document frequencies over all images
        t_df = time.perf_counter() - t0
        t0 = time.perf_counter()
        st = np.stack([S.set_stats(c) for c in caps])
        for c in caps:
            S.self_cider(S.eigenvalues(S.kernel_matrix(c, df, n_img)))
            S.distinct(c)
        S.mbleu(st)
        t = time.perf_counter() - t0
        print(f"CPU set restatement (float64 Python, one thread): document frequencies {t_df * 1e3:.0f} ms; {K} images x {N} samples "
              f"in {t:.2f} s -> {t * I / K:.0f} s for all {I} images (linear extrapolation)")
