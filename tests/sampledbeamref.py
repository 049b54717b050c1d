"""Shared pieces of the sampled-node beam search tests (ssc_beam_step_sampled / ssc_decode_sampled_beam, include/ssc.h) and of
tests/golden/make_sampled_beam_golden.py: the fixture's cases, the Philox uniforms of a draw, and an independent float64 NumPy
restatement of one step written from the semantics in the header (the kept set in float64, the scores in the device's float32
arithmetic, as tests/samplerref.py restates ssc_sample_rows).  The step function and the replay are tests/sbsref.py's."""
import numpy as np

import goldenlib
import samplerref
import sbsref

END = sbsref.END
SEED = 0x5A3B1ED_4567
MAX_STEPS = 5
KINDS = ("multinomial", "top-k", "top-p")


def _cases():
    cs = []
    Ts = (0.7, 1.0, 1.6)
    i = 0
    for kind in KINDS:
        for rep in (False, True):
            for V, k, n in ((51, 1, 1), (51, 3, 2), (10001, 5, 5), (51, 8, 2), (10001, 3, 1), (51, 5, 2)):
                T = Ts[i % 3]
                i += 1
                cs.append(dict(name=f"{kind}_r{int(rep)}_V{V}_k{k}_n{n}", kind=kind, rep=rep, V=V, k=k, n=n, T=T, top_k=max(n, 7),
                               top_p=0.6, B=2, steps=MAX_STEPS, boost=(0.0, 0.0)))
        # the global-memory form of the row kernel
        cs.append(dict(name=f"{kind}_V40003", kind=kind, rep=False, V=40003, k=3, n=2, T=1.0, top_k=9, top_p=0.6, B=2,
                       steps=4, boost=(0.0, 0.0)))
        # beams that end at different steps (the end token gains weight every step), with and without replacement
        for rep in (False, True):
            cs.append(dict(name=f"{kind}_r{int(rep)}_ends", kind=kind, rep=rep, V=51, k=3, n=2, T=1.0, top_k=7, top_p=0.6, B=2,
                           steps=9, boost=(6.0, 1.5)))
    # top-p with p below the top token's mass: without replacement the first n tokens are kept all the same
    cs.append(dict(name="top-p_forced", kind="top-p", rep=False, V=51, k=5, n=5, T=1.0, top_k=0, top_p=0.02, B=2, steps=MAX_STEPS,
                   boost=(0.0, 0.0)))
    return cs


CASES = _cases()


def sampler_args(case):
    """(kind id, top_k, top_p, T) of ssc_sampler_desc for a case."""
    return samplerref.KIND[case["kind"]], case["top_k"] if case["kind"] == "top-k" else 0, \
        case["top_p"] if case["kind"] == "top-p" else 1.0, case["T"]


def uniforms(V, seed, step, rows, d=0):
    """u (len(rows), V) float32: Philox4x32-10, key = seed, counter (v / 4, step, row, d), word v % 4, mapped to (0, 1)."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1)
    nj = (V + 3) // 4
    ctr = np.zeros((rows.size, nj, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(nj, dtype=np.uint32)[None]
    ctr[..., 1] = step
    ctr[..., 2] = rows[:, None]
    ctr[..., 3] = d
    x = samplerref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(rows.size, -1)[:, :V]
    return (((x >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def gumbel(u):
    """g = -log(-log(u)) in float32, as the device computes it."""
    return -np.log(-np.log(u))


# ---- float64 restatement -----------------------------------------------------------------------------------------------------

def kept_set(x, kind, top_k=0, top_p=1.0, T=1.0, n=1, rep=False):
    """x (V,) logits -> kept (V,) bool and the margin of the cut (inf where there is no cut): top-k keeps the top_k largest (ties:
    lower index); top-p keeps a token iff it is first or the tempered mass strictly ahead of it is < p, and without replacement
    also the first n tokens of the sorted order.  The top-p margin is the distance of the masses ahead from p, times 10: the
    device's masses are exact to ~1e-7 (2^-40 fixed point over fp32 exponentials), so a mass margin of 1e-6 is as safe as a
    logit margin of 1e-5."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    order = np.argsort(-x, kind="stable")
    kept = np.ones(V, dtype=bool)
    margin = np.inf
    if kind == "top-k" and top_k < V:
        kept[:] = False
        kept[order[:top_k]] = True
        margin = x[order[top_k - 1]] - x[order[top_k]]
    elif kind == "top-p" and top_p < 1.0:
        _, ahead = samplerref.filter_dist(x, "top-p", p=top_p, T=T)
        kept = ahead < top_p
        kept[order[0]] = True
        if not rep:
            kept[order[:n]] = True
        margin = 10 * np.abs(ahead[order[1:]] - top_p).min() if V > 1 else np.inf
    return kept, margin


def row_candidates(logits, last_pred, phi, n, kind, top_k, top_p, T, rep, seed, step, end=END):
    """Step t >= 1 for rows (R, V) of raw logits -> (tokens, summed log-probs, margin) (R, n), (R, n), (R,): the margin is the
    smallest gap of any decision of the row (the cut of the kept set, the n-th vs (n+1)-th score, each draw's best vs second)."""
    x32 = np.asarray(logits, dtype=np.float32)
    R, V = x32.shape
    x = x32.astype(np.float64)
    m = x.max(1, keepdims=True)
    lp = x - m - np.log(np.exp(x - m).sum(1, keepdims=True))
    tok = np.full((R, n), end, dtype=np.int64)
    L = np.full((R, n), -np.inf)
    gap = np.full(R, np.inf)
    for r in range(R):
        if last_pred[r] == end:
            L[r, 0] = phi[r]
            if rep:
                L[r, :] = phi[r]
            continue
        kept, gap[r] = kept_set(x[r], kind, top_k, top_p, T, n, rep)
        draws = range(n) if rep else (0,)
        for d in draws:
            s = x32[r] / np.float32(T) + gumbel(uniforms(V, seed, step, [r], d)[0])
            s = np.where(kept, s.astype(np.float64), -np.inf)
            o = np.argsort(-s, kind="stable")
            if rep:
                tok[r, d] = o[0]
                gap[r] = min(gap[r], s[o[0]] - s[o[1]] if np.isfinite(s[o[1]]) else np.inf)
            else:
                tok[r] = o[:n]
                if V > n and np.isfinite(s[o[n]]):
                    gap[r] = min(gap[r], np.diff(-s[o[: n + 1]]).min())
                elif n > 1:
                    gap[r] = min(gap[r], np.diff(-s[o[:n]]).min())
        L[r] = phi[r] + lp[r, tok[r]]
    return tok, L, gap


def merge(tok, L, B, k):
    """Per entry: the top k of the candidates by summed log-prob, descending (ties: lower candidate index).
    -> (tokens, log-probs, candidate index) (B, k)."""
    C = tok.size // B
    tok, L = tok.reshape(B, C), L.reshape(B, C)
    sel = np.argsort(-L, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(tok, sel, 1), np.take_along_axis(L, sel, 1), sel


def next_step(logits, last_pred, phi, B, k, n, kind, top_k, top_p, T, rep, seed, step):
    """Step >= 1 from (B*k, V) logits -> (tokens, log-probs, back-pointers, candidate margins (B,)) (B, k)."""
    tok, L, gap = row_candidates(logits, np.asarray(last_pred).reshape(-1), np.asarray(phi, dtype=np.float64).reshape(-1), n,
                                 kind, top_k, top_p, T, rep, seed, step)
    t, l, sel = merge(tok, L, B, k)
    return t, l, sel // n, gap.reshape(B, k).min(1)


def first_step(lp, k):
    """Step 0 (sample_beams = topk) from (B, V) log-probs -> (tokens, log-probs) (B, k)."""
    lp = np.asarray(lp, dtype=np.float64)
    m = lp.max(1, keepdims=True)
    lsm = lp - m - np.log(np.exp(lp - m).sum(1, keepdims=True))
    o = np.argsort(-lsm, axis=1, kind="stable")[:, :k]
    return o, np.take_along_axis(lsm, o, 1)


# ---- the fixture -------------------------------------------------------------------------------------------------------------

def load_fixture(name="g19_sampled_beam"):
    """-> {case name: {"pred" (B, k, steps), "lp" (B, k), "tok"/"lp_t" (steps, B, k), "bp" (steps, B, k) (row 0 unused),
    "gap" (steps, B)}} and the cases."""
    z = goldenlib.load_raw(name)
    out = {}
    for c in CASES:
        p = c["name"] + "/"
        out[c["name"]] = {key[len(p):]: v for key, v in z.items() if key.startswith(p)}
    return out, CASES


def replay(case, rec):
    """The log-prob rows every step of the fixture's search saw (sbsref.replay)."""
    return sbsref.replay(case, rec)
