"""A restatement of arithmetic sampling's integer arithmetic (include/ssc.h: ssc_arith_rows steps 2 to 4, ssc_arith_codes) with Python
integers, for the arithmetic-sampling tests.  The masses are an INPUT: the device's own (mass_out), or masses made up by a test.  What
is restated is exact, so the device has to agree bit for bit."""
import numpy as np

import samplerref

MASS_ONE = 1 << 40        # the mass of a row's top word
MASK = (1 << 64) - 1
STREAM = 0x41524954       # the last Philox counter word of the lattice shifts ("ARIT")


def divide(hi, lo, w):
    """floor((hi 2^64 + lo) / w) for hi < w, as the device forms it: 64 steps of shift and subtract -> (quotient, remainder)"""
    assert 0 <= hi < w and 0 <= lo <= MASK
    rem, quo = hi, 0
    for i in range(63, -1, -1):
        rem = (rem << 1) | ((lo >> i) & 1)
        quo <<= 1
        if rem >= w:
            rem -= w
            quo |= 1
    return quo, rem


def draw(w, c):
    """w: the V integer masses of a row in vocabulary order, c: its code (0 <= c < 2^64) -> (token, new code); (None, c) for a row
    without mass."""
    w = np.asarray(w, dtype=np.int64)
    c = int(c)
    assert 0 <= c <= MASK and bool((w >= 0).all()) and int(w.max()) * w.size < 1 << 62      # (the int64 sums below are exact)
    incl = np.cumsum(w)                              # cum(v) + w_v
    W = int(incl[-1])
    if W == 0:
        return None, c
    t, lo = divmod(c * W, 1 << 64)
    v = int(np.searchsorted(incl, t, side="right"))  # the first v with t < cum(v) + w_v: a word with w_v > 0
    wv, cum = int(w[v]), int(incl[v]) - int(w[v])
    assert cum <= t < cum + wv
    return v, divide(t - cum, lo, wv)[0]


def lattice(u, n):
    """the n codes of one image: u + floor(j 2^64 / n) (mod 2^64)"""
    return [(int(u) + (j << 64) // n) & MASK for j in range(n)]


def shifts(seed, nimg):
    """u_i of image i: words 0 (low) and 1 (high) of Philox4x32-10 at counter (0, 0, i, STREAM), key = seed"""
    ctr = np.zeros((nimg, 4), dtype=np.uint32)
    ctr[:, 2] = np.arange(nimg, dtype=np.uint32)
    ctr[:, 3] = STREAM
    x = samplerref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return [int(x[i, 0]) | (int(x[i, 1]) << 32) for i in range(nimg)]


def codes(seed, nimg, n):
    """ssc_arith_codes: row i n + j -> (nimg * n,) uint64"""
    return np.array([c for u in shifts(seed, nimg) for c in lattice(u, n)], dtype=np.uint64)


def masses64(x, kept, T):
    """The masses in float64 (unrounded): exp((x_v - mx) / T) 2^40 over the kept entries, 0 elsewhere; mx the row's maximum."""
    x = np.asarray(x, dtype=np.float64)
    mx = x.max()
    with np.errstate(invalid="ignore"):
        return np.where(kept & np.isfinite(x), np.exp((x - mx) / T) * MASS_ONE, 0.0)


def code_for(w, v, frac=0.5):
    """A code that draws word v of masses w (w[v] > 0): the code whose t lands at cum(v) + floor(frac w_v) (frac in [0, 1))."""
    w = [int(x) for x in w]
    W, cum = sum(w), sum(w[:v])
    t = cum + min(int(frac * w[v]), w[v] - 1)
    c = -((-t << 64) // W)          # the least c with floor(c W / 2^64) >= t
    assert c <= MASK and (c * W) >> 64 == t
    return c
