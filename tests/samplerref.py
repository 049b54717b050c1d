"""NumPy restatements of the word samplers (ssc_sample_rows, include/ssc.h) for the sampling tests: the three filters in float64,
Philox4x32-10 and the Gumbel-max draw in the device's float32 arithmetic."""
import ast

import numpy as np

import goldenlib

KIND = {"multinomial": 0, "top-k": 1, "top-p": 2}


def filter_dist(lp, kind, k=0, p=1.0, T=1.0):
    """lp (V,) log-probs -> (probs (V,) float64 over the kept set, ahead (V,) tempered mass strictly ahead of each token in the
    descending order (ties: lower index first))."""
    lp = np.asarray(lp, dtype=np.float64)
    V = lp.shape[0]
    order = np.argsort(-lp, kind="stable")
    z = lp / T
    q = np.exp(z - z.max())
    q /= q.sum()
    ahead = np.empty(V)
    ahead[order] = np.cumsum(q[order]) - q[order]
    kept = np.ones(V, dtype=bool)
    if kind == "top-k" and k < V:
        kept[:] = False
        kept[order[:k]] = True
    elif kind == "top-p" and p < 1.0:
        kept = ahead < p
        kept[order[0]] = True
    w = np.where(kept, q, 0.0)
    return w / w.sum(), ahead


M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4) uint32, key (2,) uint32 -> (..., 4) uint32."""
    c = [np.asarray(ctr[..., i], dtype=np.uint32) for i in range(4)]
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0 = np.uint32(k0 + W0)
            k1 = np.uint32(k1 + W1)
    return np.stack(c, axis=-1)


def gumbel(V, seed, step, b):
    """The draw's noise g_v (float32) of row (batch entry) b at `step`: counter (v / 4, step, b, 0), key = seed, word v % 4."""
    nj = (V + 3) // 4
    ctr = np.zeros((nj, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nj, dtype=np.uint32)
    ctr[:, 1] = step
    ctr[:, 2] = b
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:V]
    u = (((x >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)
    return -np.log(-np.log(u))


def draw(logits, kept, T, seed, step, b):
    """-> (token, perturbed scores (V,) float32 with -inf outside the kept set)."""
    x = np.asarray(logits, dtype=np.float32)
    s = x / np.float32(T) + gumbel(x.shape[0], seed, step, b)
    s = np.where(kept, s, np.float32(-np.inf))
    return int(np.argmax(s)), s


def load_fixture(name="g17_samplers"):
    """-> (arrays, cfg): lp_V{V} (3, V) float32 rows and dist_V{V}_s{si} (3, V) float32, the reference's distributions in
    vocabulary order, rebuilt from the value tables tests/golden/make_sampler_golden.py stores."""
    z = goldenlib.load_raw(name)
    cfg = ast.literal_eval(str(z["cfg"]))
    d = {}
    for V in cfg["vs"]:
        idx = z[f"lp_V{V}_idx"].astype(np.int64)
        lp = np.take_along_axis(z[f"lp_V{V}_vals"], idx, 1)
        d[f"lp_V{V}"] = lp
        order = np.argsort(-lp, axis=1, kind="stable")
        for si in range(len(cfg["settings"])):
            if f"keep_V{V}_s{si}" not in z:
                continue
            keep, tab = z[f"keep_V{V}_s{si}"], z[f"prob_V{V}_s{si}"]
            dist = np.zeros_like(lp)
            for r in range(lp.shape[0]):
                kept = order[r, : keep[r]]
                dist[r, kept] = tab[r, idx[r, kept]]
            d[f"dist_V{V}_s{si}"] = dist
    return d, cfg


def check_against_reference(got, ref, ahead, kind, p, what):
    """got, ref (V,) distributions over the kept sets (ours, the reference's), ahead (V,) float64 tempered mass ahead of each token.
    Kept sets equal, except tokens whose mass ahead lies within 1e-6 of p (the reference's fp32 cumsum decides those); at p = 1
    every token is kept here, while the reference's fp32 cumsum reaches 1 before the end of a long tail and drops what follows -
    such tokens must have at least 1 - 1e-3 of the mass ahead of them, and the comparison renormalises ours over the reference's
    set.  Probabilities agree within 1e-6 (+ 3e-6 relative: fp32 near 1)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    diff = (got > 0) != (ref > 0)
    if kind == "top-p" and p >= 1.0:
        assert (got > 0).all(), what
        assert (ahead[diff] >= 1 - 1e-3).all(), what
        got = np.where(ref > 0, got, 0.0)
        got /= got.sum()
        diff[:] = False
    else:
        assert not (diff & ~(np.abs(ahead - p) < 1e-6)).any(), (what, np.nonzero(diff)[0][:10])
    np.testing.assert_allclose(got[~diff], ref[~diff], rtol=3e-6, atol=1e-6, err_msg=str(what))
