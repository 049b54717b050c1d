"""Shared pieces of the stochastic beam search tests (ssc_beam_first_gumbel / ssc_beam_step_gumbel / ssc_decode_stochastic_beam,
include/ssc.h) and of tests/golden/make_sbs_golden.py: the fixture's cases, a small synthetic step function, the Philox uniforms
of a step, and an independent float64 NumPy restatement of the search written from the semantics in the header."""
import numpy as np

import goldenlib
import samplerref

END = 3
SEED = 0x5EED5B5_0123
MAX_STEPS = 5


def _cases():
    cs = []
    for V in (50, 10000):
        for k in (1, 3, 5):
            for n in sorted({1, 2, k}):
                if n > k:
                    continue
                for T in (0.7, 1.0, 1.6):
                    cs.append(dict(name=f"V{V}_k{k}_n{n}_T{T}", V=V, k=k, n=n, T=T, B=2, steps=MAX_STEPS, boost=(0.0, 0.0)))
    # beams that end at different steps (the end token gains weight every step), and a search that ends at step 0 with k = 1
    cs.append(dict(name="ends", V=50, k=3, n=2, T=1.0, B=2, steps=9, boost=(6.0, 1.5)))
    cs.append(dict(name="allend0", V=50, k=1, n=1, T=1.0, B=2, steps=MAX_STEPS, boost=(1000.0, 0.0)))
    return cs


CASES = _cases()


def start_state(B):
    return (np.arange(B, dtype=np.int64) * 13) % 1009


def next_state(acc, tokens):
    return (acc * 31 + np.asarray(tokens, dtype=np.int64)) % 1009


def step_rows(tokens, t, acc, V, boost=(0.0, 0.0)):
    """Log-probs (rows, V) float32 of the synthetic step: a hash of (token v, last token, step, per-row state) on a 1/256 grid in
    [0, 16), the end token raised by boost[0] + boost[1] * t; normalised in float64."""
    tokens = np.asarray(tokens, dtype=np.uint64).reshape(-1)
    acc = np.asarray(acc, dtype=np.uint64).reshape(-1)
    v = np.arange(V, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (v[None] * np.uint64(2654435761) + tokens[:, None] * np.uint64(40503) + np.uint64(977 * t) +
             acc[:, None] * np.uint64(7919)) & np.uint64(0xFFFFFFFF)
    x = (h >> np.uint64(20)).astype(np.float64) / 256.0
    x[:, END] += boost[0] + boost[1] * t
    m = x.max(1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(1, keepdims=True))).astype(np.float32)


def uniforms(V, seed, step, rows):
    """u (len(rows), V) float32: Philox4x32-10, key = seed, counter (v / 4, step, row, 0), word v % 4, mapped to (0, 1) as the
    device maps it (samplerref.gumbel, before the logs)."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1)
    nj = (V + 3) // 4
    ctr = np.zeros((rows.size, nj, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(nj, dtype=np.uint32)[None]
    ctr[..., 1] = step
    ctr[..., 2] = rows[:, None]
    x = samplerref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(rows.size, -1)[:, :V]
    return (((x >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


# ---- float64 restatement -----------------------------------------------------------------------------------------------------

def _lsm(x):
    m = x.max(1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(1, keepdims=True))


def perturbed(phi, u):
    """g = phi + Gumbel(u) in float64."""
    with np.errstate(divide="ignore"):
        return phi + (-np.log(-np.log(u.astype(np.float64))))


def transform(g, Tp):
    """gumbel_with_max's G from g (rows, V) and the targets Tp (rows,), in float64."""
    Z = g.max(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = Tp[:, None] - g + np.log1p(-np.exp(g - Z))
        return Tp[:, None] - np.logaddexp(0.0, w)


def top_by(x, n):
    """indices of the n largest of every row of x, descending, ties to the lower index."""
    return np.argsort(-x, axis=1, kind="stable")[:, :n]


def row_candidates(lp, last_pred, phi, Gprev, n, T, seed, step, end=END):
    """Row (b, j) of a step >= 1: its n candidates (tokens, G, summed log-prob) (rows, n) - ended rows: end at (G_bj, phi)."""
    lp = lp.astype(np.float64)
    R, V = lp.shape
    lpT = _lsm(lp / T) if T != 1.0 else lp
    g = perturbed(phi[:, None] + lpT, uniforms(V, seed, step, np.arange(R)))
    tok = top_by(g, n)
    G = np.take_along_axis(transform(g, Gprev), tok, 1)
    L = phi[:, None] + np.take_along_axis(lp, tok, 1)
    ended = np.asarray(last_pred) == end
    tok[ended] = end
    G[ended] = -np.inf
    L[ended] = -np.inf
    G[ended, 0] = Gprev[ended]
    L[ended, 0] = phi[ended]
    return tok, G, L


def merge(tok, G, L, B, k):
    """Per entry: top k of the candidates by G (ties: lower candidate index), stably sorted by summed log-prob descending.
    -> (tokens, log-probs, G, candidate index) (B, k)."""
    C = tok.size // B
    tok, G, L = tok.reshape(B, C), G.reshape(B, C), L.reshape(B, C)
    sel = top_by(G, k)
    order = np.argsort(-np.take_along_axis(L, sel, 1), axis=1, kind="stable")
    sel = np.take_along_axis(sel, order, 1)
    return (np.take_along_axis(tok, sel, 1), np.take_along_axis(L, sel, 1), np.take_along_axis(G, sel, 1), sel)


def first_step(lp, k, seed):
    """Step 0 from (B, V) log-probs -> (tokens, log-probs, G) (B, k)."""
    lp = lp.astype(np.float64)
    B, V = lp.shape
    g = perturbed(lp, uniforms(V, seed, 0, np.arange(B)))
    tok = top_by(g, k)
    G = np.take_along_axis(transform(g, np.zeros(B)), tok, 1)
    L = np.take_along_axis(lp, tok, 1)
    t, l, gg, _ = merge(tok, G, L, B, k)
    return t, l, gg


def next_step(lp, last_pred, phi, Gprev, B, k, n, T, seed, step):
    """Step >= 1 from (B*k, V) log-probs -> (tokens, log-probs, G, back-pointers) (B, k)."""
    tok, G, L = row_candidates(lp, last_pred.reshape(-1), phi.reshape(-1), Gprev.reshape(-1), n, T, seed, step)
    t, l, gg, sel = merge(tok, G, L, B, k)
    return t, l, gg, sel // n


# ---- the fixture -------------------------------------------------------------------------------------------------------------

def load_fixture(name="g18_stochastic_beam"):
    """-> {case name: {"pred" (B, k, steps), "lp" (B, k), "tok"/"lp_t"/"G" (steps, B, k), "bp" (steps, B, k) (row 0 unused),
    "gap" (steps, B)}} and the cases."""
    z = goldenlib.load_raw(name)
    out = {}
    for c in CASES:
        p = c["name"] + "/"
        out[c["name"]] = {k[len(p):]: v for k, v in z.items() if k.startswith(p)}
    return out, CASES


def replay(case, rec):
    """The rows every step of the fixture's search saw: yields (step, lp rows) - step 0: (B, V), later (B*k, V) - following the
    fixture's own tokens and back-pointers (the state re-ordered as the reference's _update_state does)."""
    B, k, V = case["B"], case["k"], case["V"]
    acc = start_state(B)
    start = np.full(B, END, dtype=np.int64)
    yield 0, step_rows(start, 0, acc, V, case["boost"])
    acc = np.repeat(next_state(acc, start), k)
    for t in range(1, rec["tok"].shape[0]):
        last = rec["tok"][t - 1].reshape(-1)
        yield t, step_rows(last, t, acc, V, case["boost"])
        acc = next_state(acc, last).reshape(B, k)
        acc = np.take_along_axis(acc, rec["bp"][t].astype(np.int64), 1).reshape(-1)
