#!/usr/bin/env python3
"""Times the stages of consensus re-ranking (csrc/consensus.hip + ssc_gemm) at a realistic size on synthetic data: a bank of
M = 113 287 images x F = 2048 with five 8-15 word captions each over V = 10 000 words, Q = 1000 query images of N = 100 candidates,
k = 60 neighbours.  Prints, per stage: normalise (bank, queries), GEMM and merge per bank chunk, consensus scoring + ordering; and
for comparison the same neighbours from torch.mm + torch.topk in fp32 on the same device.  Not a pass/fail gate.

    python tools/consensus_probe.py [--bank 113287] [--features 2048] [--queries 1000] [--samples 100] [--k 60] [--out DIR]

Every stage that uses the GPU is a child process under its own `timeout`; the first non-zero status ends the run."""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))

parser = argparse.ArgumentParser("consensus re-ranking stage times")
parser.add_argument("--bank", type=int, default=113287)
parser.add_argument("--features", type=int, default=2048)
parser.add_argument("--queries", type=int, default=1000)
parser.add_argument("--samples", type=int, default=100)
parser.add_argument("--k", type=int, default=60)
parser.add_argument("--vocab", type=int, default=10000)
parser.add_argument("--reps", type=int, default=3)
parser.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "consensus_probe"), help="directory for the neighbour lists the stages share")
parser.add_argument("--stage", default="", choices=["", "knn", "torch", "score"])
LIMITS = {"knn": 300, "torch": 240, "score": 420}   # seconds per stage


def data(a, torch):
    g = torch.Generator(device="cuda").manual_seed(11)
    bank = torch.randn(a.bank, a.features, generator=g, device="cuda")
    q = torch.randn(a.queries, a.features, generator=g, device="cuda")
    # queries near bank rows, as test images are near training images: neighbours that mean something
    q = 0.5 * q + bank[torch.randint(0, a.bank, (a.queries,), generator=g, device="cuda")]
    return bank, q


class Timer:
    def __init__(self, torch):
        self.torch, self.t = torch, {}

    def __call__(self, name, fn):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.t.setdefault(name, []).append((e0, e1))

    def report(self):
        self.torch.cuda.synchronize()
        out = {}
        for name, evs in self.t.items():
            out[name] = [a.elapsed_time(b) for a, b in evs]
        return out


def stage_knn(a):
    import numpy as np
    import torch
    from ssc_runtime import evaluation as E
    from ssc_runtime import lib as L
    lib = L.load()
    bank, q = data(a, torch)
    M, F, Q, k = a.bank, a.features, a.queries, a.k
    st = L.stream_ptr()
    bn, qn = torch.empty_like(bank), torch.empty_like(q)
    rows = min(M, E.SIM_BUFFER_BYTES // (4 * Q) // 4 * 4)
    sims = torch.empty(Q, rows, dtype=torch.float32, device="cuda")
    d = L.GemmDesc()
    d.nseg, d.M, d.a_kc, d.b_kc, d.splits = 1, Q, 1, 1, 1
    d.seg[0].A, d.seg[0].lda, d.seg[0].ldb, d.seg[0].K = qn.data_ptr(), F, F, F
    d.C, d.ldc = sims.data_ptr(), rows
    print(f"bank {M} x {F}, {Q} queries, k {k}: chunks of {rows} rows ({Q * rows * 4 / 2**20:.1f} MB of similarities)")
    for rep in range(a.reps + 1):   # the first pass warms up
        T = Timer(torch)
        T("normalise bank", lambda: lib.ssc_l2_normalize_rows(L.ptr(bank), M, F, F, L.ptr(bn), F, st))
        T("normalise queries", lambda: lib.ssc_l2_normalize_rows(L.ptr(q), Q, F, F, L.ptr(qn), F, st))
        bs = torch.full((Q, k), float("-inf"), dtype=torch.float32, device="cuda")
        bi = torch.full((Q, k), -1, dtype=torch.int32, device="cuda")
        for off in range(0, M, rows):
            mc = min(rows, M - off)
            d.N = mc
            d.seg[0].B = bn.data_ptr() + 4 * off * F
            T("gemm", lambda: lib.ssc_gemm(ctypes.byref(d), st))
            T("merge", lambda: lib.ssc_knn_merge(L.ptr(sims), rows, Q, mc, off, k, None, L.ptr(bs), L.ptr(bi), st))
        t = T.report()
        if rep == 0:
            continue
        print(f"pass {rep}: normalise bank {t['normalise bank'][0]:.3f} ms, queries {t['normalise queries'][0]:.3f} ms; "
              f"gemm per chunk {' '.join(f'{x:.3f}' for x in t['gemm'])} ms (sum {sum(t['gemm']):.3f}); "
              f"merge per chunk {' '.join(f'{x:.3f}' for x in t['merge'])} ms (sum {sum(t['merge']):.3f}); "
              f"search total {sum(t['gemm']) + sum(t['merge']) + t['normalise queries'][0]:.3f} ms")
    os.makedirs(a.out, exist_ok=True)
    np.save(os.path.join(a.out, "consensus_probe_idx.npy"), bi.cpu().numpy())
    np.save(os.path.join(a.out, "consensus_probe_sim.npy"), bs.cpu().numpy())


def stage_torch(a):
    import numpy as np
    import torch
    bank, q = data(a, torch)
    k = a.k
    for rep in range(a.reps + 1):
        T = Timer(torch)
        out = {}

        def norm():
            out["bn"] = torch.nn.functional.normalize(bank, dim=1)
            out["qn"] = torch.nn.functional.normalize(q, dim=1)

        def mm():
            out["s"] = torch.mm(out["qn"], out["bn"].T)

        def topk():
            out["v"], out["i"] = torch.topk(out["s"], k, dim=1)
        T("normalise", norm)
        T("mm", mm)
        T("topk", topk)
        t = T.report()
        if rep:
            print(f"torch pass {rep}: normalize {t['normalise'][0]:.3f} ms, mm {t['mm'][0]:.3f} ms, topk {t['topk'][0]:.3f} ms "
                  f"(mm + topk {t['mm'][0] + t['topk'][0]:.3f} ms)")
    path = os.path.join(a.out, "consensus_probe_idx.npy")
    if os.path.exists(path):
        mine, ms = np.load(path), np.load(os.path.join(a.out, "consensus_probe_sim.npy"))
        theirs, ts = out["i"].cpu().numpy(), out["v"].cpu().numpy()
        same = float((mine == theirs).all(1).mean())
        sets = float(np.mean([len(set(x) & set(y)) / k for x, y in zip(mine.tolist(), theirs.tolist())]))
        print(f"against torch.mm + torch.topk (fp32): identical lists for {same:.4f} of the queries, mean set overlap {sets:.6f}, "
              f"largest similarity difference {np.abs(ms - ts).max():.3g}")


def stage_score(a):
    import numpy as np
    import torch
    from ssc_runtime import evaluation as E
    from ssc_runtime import lib as L
    lib = L.load()
    rng = np.random.default_rng(5)
    M, V, P, N, k = a.bank, a.vocab, a.queries, a.samples, a.k
    nref = 5 * M
    lens = rng.integers(8, 16, nref)
    tok_off = np.concatenate([[0], np.cumsum(lens)])
    toks = np.minimum(rng.zipf(1.3, int(tok_off[-1])), V - 3) + 1          # compact ids 1..V-2: frequent words repeat, as in captions
    ref_off = np.arange(0, nref + 1, 5)
    t0 = time.time()
    prep = E._Prepared.from_csr(ref_off, tok_off, toks, V - 2, "cuda")
    torch.cuda.synchronize()
    print(f"prepare {M} images, {nref} captions, {len(toks)} tokens: {time.time() - t0:.3f} s")
    path = os.path.join(a.out, "consensus_probe_idx.npy")
    nb = np.load(path).astype(np.int32) if os.path.exists(path) else rng.integers(0, M, (P, k)).astype(np.int32)
    nb = nb[:P, :k]
    # candidates: a neighbour's caption with some words redrawn, 8-15 words; prediction id v is compact id v - 1 (ids 0, 1: no word)
    steps = 16
    pred = np.ones((P, N, steps), dtype=np.int64)
    for p in range(P):
        src = nb[p, rng.integers(0, nb.shape[1], N)] * 5 + rng.integers(0, 5, N)
        for n in range(N):
            w = toks[tok_off[src[n]]: tok_off[src[n] + 1]].copy()
            redo = rng.random(len(w)) < 0.3
            w[redo] = np.minimum(rng.zipf(1.3, int(redo.sum())), V - 3) + 1
            pred[p, n, :len(w)] = w + 1
    id_map = np.concatenate([[0, 0], np.arange(1, V - 1)]).astype(np.int32)
    dev = dict(device="cuda")
    pt, im, nbt = torch.from_numpy(pred).cuda(), torch.from_numpy(id_map).cuda(), torch.from_numpy(nb).cuda()
    scores = torch.empty(P, N, dtype=torch.float64, **dev)
    pool, pick = torch.empty(P, dtype=torch.int32, **dev), torch.empty(P, dtype=torch.int32, **dev)
    order = torch.empty(P, N, dtype=torch.int32, **dev)
    ws = torch.empty(256, dtype=torch.uint8, **dev)

    def call(pred_t, nb_t, kk):
        d = L.EvalConsensusDesc(L.ptr(pred_t), P, N, steps, 1, V, L.ptr(im), L.ptr(nb_t), kk, L.ptr(scores), L.ptr(pool), L.ptr(pick),
                                L.ptr(order))
        torch.cuda.synchronize()
        t = time.time()
        lib.ssc_eval_consensus(ctypes.byref(prep.desc), ctypes.byref(d), L.ptr(ws), 256, L.stream_ptr())   # (synchronises)
        return (time.time() - t) * 1e3
    full = [call(pt, nbt, nb.shape[1]) for _ in range(a.reps + 1)][1:]
    print(f"consensus scoring + ordering ({P} x {N} candidates, pools of {int(pool.float().mean())} captions): "
          f"{' '.join(f'{x:.3f}' for x in full)} ms; mean best score {float(scores.max(1).values.mean()):.4f}")
    empty = torch.ones_like(pt)
    one = nbt[:, :1].contiguous()
    low = [call(empty, one, 1) for _ in range(a.reps + 1)][1:]
    print(f"the same call with empty candidates and one neighbour (launches, flag read-back and the ordering kernel: an upper bound "
          f"of the ordering stage): {' '.join(f'{x:.3f}' for x in low)} ms")


def main():
    a = parser.parse_args()
    if a.stage:
        {"knn": stage_knn, "torch": stage_torch, "score": stage_score}[a.stage](a)
        return 0
    for stage in ("knn", "torch", "score"):
        cmd = ["timeout", "-k", "10", str(LIMITS[stage]), sys.executable, os.path.abspath(__file__), "--stage", stage] + sys.argv[1:]
        print(f"--- {stage} (limit {LIMITS[stage]} s)", flush=True)
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"stage {stage} ended with status {rc}: stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
