"""float64 restatement of the contrastive edit of the word samplers (ssc_contrast_rows, include/ssc.h): with lp = log_softmax(x),
m = max lp_e and logb = log(beta) rounded to float32 (as the library takes it),

    y[v] = lp_e[v] + alpha * (lp_e[v] - lp_a[v])   where beta == 0 or lp_e[v] >= logb + m,      -inf elsewhere,

with `kept` (the entries left finite), KL(p_e || p_a) in nats over all V entries and - a condition on a test's INPUTS - the tokens
whose membership float32 arithmetic cannot be expected to decide.

Undecidable tokens: any token with |lp_e[v] - m - logb| < D_BAND = 2e-5 that is not itself a maximal entry (a maximal entry is kept
in any arithmetic).  D_BAND is truncationref.D_BAND - the same kind of quantity, a float32 log-prob against a threshold; it is fixed
here, never fitted to the device.  Every device comparison first asserts that the restatement finds no undecidable token."""
import numpy as np

from truncationref import D_BAND


class Edit:
    """y (V,) float64 (-inf where dropped); kept (V,) bool; kl: KL(p_e || p_a) in nats (0 without an amateur); undecidable: sorted
    token ids; lp_e, lp_a (V,) float64 (lp_a None without an amateur)"""

    def __init__(self, y, kept, kl, undecidable, lp_e, lp_a):
        self.y, self.kept, self.kl, self.undecidable, self.lp_e, self.lp_a = y, kept, kl, undecidable, lp_e, lp_a


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    mx = x.max()
    return x - (mx + np.log(np.exp(x - mx).sum()))


def logb_of(beta):
    """log(beta) as the library takes it: of the float32 beta, in double, rounded to float32"""
    return float(np.float32(np.log(np.float64(np.float32(beta)))))


def contrast_row(x_e, x_a, alpha, beta):
    """-> Edit of one expert row x_e (V,) against the amateur row x_a (V,) or None (alpha must then be 0)."""
    xe32 = np.asarray(x_e, dtype=np.float32)
    lp_e = log_softmax(xe32)
    lp_a = None
    if x_a is None:
        if alpha != 0:
            raise ValueError("no amateur: alpha must be 0")
        y, kl = lp_e.copy(), 0.0
    else:
        lp_a = log_softmax(np.asarray(x_a, dtype=np.float32))
        d = lp_e - lp_a
        y = lp_e + float(np.float32(alpha)) * d
        kl = float((np.exp(lp_e) * d).sum())
    V = xe32.shape[0]
    if beta == 0:
        return Edit(y, np.ones(V, dtype=bool), kl, [], lp_e, lp_a)
    logb = logb_of(beta)
    m = lp_e.max()
    kept = lp_e >= logb + m
    top = xe32 == xe32.max()
    kept |= top
    und = [int(v) for v in np.nonzero((np.abs(lp_e - m - logb) < D_BAND) & ~top)[0]]
    return Edit(np.where(kept, y, -np.inf), kept, kl, und, lp_e, lp_a)


def edit_rows(x_e, x_a, V, alpha, beta, last_pred=None, end=None):
    """x_e (rows, ld), x_a (rows, lda) or None, float32 -> (edited copy of x_e as float64, kept (rows,) int, kl (rows,) float64,
    live (rows,) bool, undecidable: [(row, token)]).  Rows whose last_pred is `end` and columns V .. ld - 1 are returned as they came
    (statistics 0)."""
    out = np.array(x_e, dtype=np.float64, copy=True)
    rows = out.shape[0]
    kept = np.zeros(rows, dtype=np.int64)
    kl = np.zeros(rows)
    live = np.ones(rows, dtype=bool)
    und = []
    for r in range(rows):
        if last_pred is not None and int(last_pred[r]) == end:
            live[r] = False
            continue
        e = contrast_row(x_e[r, :V], None if x_a is None else x_a[r, :V], alpha, beta)
        out[r, :V] = e.y
        kept[r] = int(e.kept.sum())
        kl[r] = e.kl
        und += [(r, v) for v in e.undecidable]
    return out, kept, kl, live, und


# ---- the inputs of the kernel tests (shared by the CPU and the GPU tests) -----------------------------------------------------------------
# (V, ld, offset of the expert in floats past a 16-byte boundary, lda, offset of the amateur): aligned and misaligned on either side
SHAPES = [(37, 37, 0, 40, 0), (451, 452, 1, 451, 2), (1024, 1028, 1, 1024, 0), (1024, 1024, 0, 1028, 3), (2003, 2004, 0, 2008, 0),
          (10000, 10000, 0, 10000, 0), (40000, 40000, 0, 40004, 0)]
ALPHAS = (0.0, 0.5, 1.0, 2.0)
BETAS = (0.0, 0.1, 0.5)
N_ROWS = 5
END = 1
# per V: the first seed offset at which the restatement finds no undecidable token at any beta (found on the CPU with rows_case alone)
ROW_SEEDS = {}


def row_seed(V):
    return 1000 * V + 7 + ROW_SEEDS.get(V, 0) * 7919


def rows_case(V, ld, lda, seed):
    """Five rows of both streams: random; a peaked expert (one token holds nearly all the mass) against a random amateur; amateur
    equal to the expert; the expert on a grid of 0.5 with the maximum three times - exact ties at the top, and at beta = 0.5 / 0.1
    no value near the cut; an ended row full of NaN.  The pad columns are NaN.
    -> (x_e (5, ld), x_a (5, lda) float32, last_pred (5,) int64)"""
    rng = np.random.default_rng(seed)
    xe = np.full((N_ROWS, ld), np.nan, dtype=np.float32)
    xa = np.full((N_ROWS, lda), np.nan, dtype=np.float32)
    xe[0, :V] = rng.standard_normal(V) * 3
    xa[0, :V] = xe[0, :V] * 0.5 + rng.standard_normal(V)
    xe[1, :V] = rng.standard_normal(V)
    xe[1, V // 3] = 25.0
    xa[1, :V] = rng.standard_normal(V) * 2
    xe[2, :V] = rng.standard_normal(V) * 3
    xa[2, :V] = xe[2, :V]
    xe[3, :V] = np.round(rng.standard_normal(V) * 3 * 2) / 2
    xe[3, [1, V // 2, V - 1]] = xe[3, :V].max() + 0.5
    xa[3, :V] = rng.standard_normal(V) * 3
    last = np.full(N_ROWS, 7, dtype=np.int64)
    last[4] = END
    return xe, xa, last
