"""The definition of the self-critical step's glue (csrc/scst.hip: ssc_scst_prepare) restated in plain NumPy fp64, in the summation
order the header states - rewards in column order, an image's leave-one-out sum in sample order, one rounding to fp32 per output -
and the weighted objective the step minimises, on the CPU oracle's train_forward."""
import numpy as np

import oracle


def pack(predictions, end_index, L):
    """predictions (G, steps) int64 -> (caps (G, L) int64: the row's tokens before its first end_index (all of them where it has
    none), then 0; lengths (G) int32).  Ids are copied as they are."""
    pred = np.asarray(predictions, dtype=np.int64)
    G, steps = pred.shape
    assert L >= steps
    caps = np.zeros((G, L), dtype=np.int64)
    lengths = np.zeros(G, dtype=np.int32)
    for g in range(G):
        n = steps
        for c in range(steps):
            if pred[g, c] == end_index:
                n = c
                break
        caps[g, :n] = pred[g, :n]
        lengths[g] = n
    return caps, lengths


def rewards(scores, weights):
    """r = sum_k w_k score_k in fp64, in column order."""
    s = np.asarray(scores, dtype=np.float64)
    r = np.zeros(s.shape[:-1], dtype=np.float64)
    for k in range(6):
        r = r + np.float64(weights[k]) * s[..., k]
    return r


def advantage(scores, base_scores, weights, baseline, loss_scale, kld_scale, lengths=None, steps=None):
    """scores (P, N, 6) fp64; base_scores (P, 6) for baseline 2.  baseline: 0 none, 1 leave-one-out, 2 given per image.
    -> dict: reward / advantage / gl / gk (G,) fp32 (one rounding each), reward64 / baseline64 / advantage64 (P, N) fp64, stats (4,)
    fp64 (mean reward, mean baseline, mean |advantage|, share of rows whose length is `steps`)."""
    s = np.asarray(scores, dtype=np.float64)
    P, N, _ = s.shape
    r = rewards(s, weights)
    if baseline == 1:
        assert N >= 2
        S = np.zeros(P, dtype=np.float64)
        for i in range(N):
            S = S + r[:, i]
        b = (S[:, None] - r) / np.float64(N - 1)
    elif baseline == 2:
        b = np.broadcast_to(rewards(base_scores, weights).reshape(P, 1), (P, N)).copy()
    else:
        b = np.zeros((P, N), dtype=np.float64)
    adv = r - b
    G = P * N
    no_end = 0.0 if lengths is None else float((np.asarray(lengths).reshape(-1) == steps).sum())
    stats = np.array([r.sum() / G, b.sum() / G, np.abs(adv).sum() / G, no_end / G], dtype=np.float64)
    return {"reward": r.reshape(G).astype(np.float32), "advantage": adv.reshape(G).astype(np.float32),
            "gl": (np.float64(loss_scale) * adv).reshape(G).astype(np.float32),
            "gk": np.full(G, np.float64(kld_scale)).astype(np.float32),
            "reward64": r, "baseline64": b, "advantage64": adv, "stats": stats}


def objective(params, cfg, feats, caps, sentiment, eps, gl, gk, obj_atts=None):
    """sum_g gl_g loss_g + sum_g gk_g kld_g with loss_g, kld_g of oracle.train_forward on the (sampled) captions."""
    out = oracle.train_forward(params, cfg, feats, caps, sentiment, eps, obj_atts=obj_atts)
    return (gl * out["loss"]).sum() + (gk * out["kld"]).sum()
