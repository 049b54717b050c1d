"""Float64 NumPy restatement of the diverse subset selection of include/ssc.h (ssc_eval_select), written from the definitions
there with no device code and no code of the runtime: MBR, MMR and the greedy MAP inference of a DPP, the shared fallback, and for
the DPP an INDEPENDENT brute-force variant that evaluates det L_{S + i} / det L_S with numpy.linalg.slogdet for every remaining
candidate at every step.

A rule is an object with objective() - the rule's value of every candidate that may still be picked, NaN elsewhere - and take(j).
run(rule, k) drives it: argmax with ties to the lowest index, the rule's stop, the fallback by q^ (stable descending), -1 tails.
run(rule, k, forced=picks) follows GIVEN picks instead of its own argmax and records the objective vector of every position:
that is how a test judges the picks of the code under test position by position without the two sides drifting apart after a
near-tie.

Fixtures (fixture(P, N)): random token rows, vocabulary 12..30 words, lengths 0..12, deliberate duplicates (every fourth caption
repeats an earlier one, half of them with the earlier one's quality too), at least one empty caption per image, random finite
qualities; the kernel is captionsetref.kernel_matrix on the CPU and ssc_eval_set on the device.

Tolerances.  Measured on the CPU over fixture(P, N) for P in {1, 5}, N in {2, 5, 20, 64, 65, 128}, k = N, both normalize settings
(test_caption_select_cpu.py measures them again and prints them), each as the largest deviation of a candidate's objective at any
position, relative to the image's largest gain:
  DPP   incremental rule against the brute-force slogdet rule, both float64:   5.47e-15 (MEASURED_DPP)
  MBR   sums over j ascending against the same sums over j descending:         9.03e-16 (MEASURED_MBR)
  MMR   has no sum (a product, a difference, a max): the two orders agree bit for bit: 0
The bound on `gains` and the margin below which a position's pick is not compared are FACTOR = 10 times the measured value: the
device may round exp differently and orders its wave reductions its own way, but it cannot be expected to be worse than an order
of magnitude beyond float64's own disagreement.  MMR's bound is therefore 0: its gains must match bit for bit."""
import numpy as np

import captionsetref as S

MBR, MMR, DPP = 1, 2, 3
FACTOR = 10.0
MEASURED_DPP = 5.47e-15
MEASURED_MBR = 9.03e-16
TOL = {MBR: FACTOR * MEASURED_MBR, MMR: 0.0, DPP: FACTOR * MEASURED_DPP}
SKIP_CAP = 0.10      # at most this share of a fixture's positions may be left out by the margin rule

SHAPES = [(P, N) for P in (1, 5) for N in (2, 5, 20, 64, 65, 128)]


def grid(N):
    """The cases every fixture is run through: (method, k, normalize, with the eligible mask, rule parameters)."""
    out = []
    for method in (MBR, MMR, DPP):
        for k in sorted(set(min(k, N) for k in (1, 5, N))):
            for normalize in (True, False):
                for masked in (False, True):
                    # (raw qualities spread over ~20 units: a DPP weight exp(theta q) with theta = 1 would spread the gains over
                    # 17 decades and leave most of them below any tolerance relative to the largest)
                    out.append((method, k, normalize, masked, dict(lam=0.7, theta=1.0 if normalize else 0.1, min_gain=1e-10)))
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def fixture(P, N, seed=None):
    """-> dict: tokens (P, N, 13) int64 rows of ids 2..V-1 closed by boundary 1 (id 0 unused), caps (P lists of N token tuples),
    quality (P, N) float64, eligible (P, N) uint8 (empty captions and a random tenth are 0), V."""
    rng = np.random.default_rng(1000 * P + N if seed is None else seed)
    V = int(rng.integers(12, 31)) + 2
    tok = np.ones((P, N, 13), dtype=np.int64)
    q = rng.normal(size=(P, N)) * 3.0 - 7.0          # log-prob-like: finite, negative and positive, no ties
    for p in range(P):
        empty = int(rng.choice([n for n in range(N) if n % 4 != 3]))
        for n in range(N):
            if n == empty:
                continue
            if n % 4 == 3:
                src = n - 1 - int(rng.integers(0, 3))
                tok[p, n] = tok[p, src]
                if rng.random() < 0.5:
                    q[p, n] = q[p, src]
                continue
            L = int(rng.integers(0, 13))
            tok[p, n, :L] = rng.integers(2, V, L)
    caps = [[tuple(int(t) for t in row[:list(row).index(1)]) for row in img] for img in tok]
    el = np.array([[len(c) > 0 for c in img] for img in caps], dtype=np.uint8)
    el &= (rng.random((P, N)) >= 0.1).astype(np.uint8)
    return {"tokens": tok, "caps": caps, "quality": q, "eligible": el, "V": V, "P": P, "N": N}


def fixture_refs(fx):
    """A small reference set over the fixture's vocabulary (the document frequencies of the kernel): (ref_off, tok_off, toks, W) in
    the CSR form of ssc_eval_refs with compact id = token id - 1, and the same as per-image token lists."""
    rng = np.random.default_rng(7 + fx["V"])
    refs = [[tuple(int(t) for t in rng.integers(2, fx["V"], int(rng.integers(3, 10)))) for _ in range(2)] for _ in range(6)]
    ref_off, tok_off, toks = [0], [0], []
    for rs in refs:
        for r in rs:
            toks += [t - 1 for t in r]
            tok_off.append(len(toks))
        ref_off.append(len(tok_off) - 1)
    return refs, (ref_off, tok_off, toks, fx["V"] - 1)


def fixture_kernel(fx):
    """(P, N, N) float64: the caption kernel of every image on the CPU (captionsetref.kernel_matrix), its upper triangle mirrored:
    the device's kernel is symmetric bit for bit, the restatement's only up to the order of its sums."""
    refs, _ = fixture_refs(fx)
    df, n_images = S.reference_df(refs)
    K = np.stack([S.kernel_matrix(c, df, n_images) for c in fx["caps"]])
    return np.triu(K) + np.triu(K, 1).transpose(0, 2, 1)


# ---- the rules --------------------------------------------------------------------------------------------------------------------

def qhat(q, el, normalize):
    """q^ of one image: q (N,) or None, el (N,) bool."""
    if q is None:
        return np.zeros(len(el))
    q = np.asarray(q, dtype=np.float64)
    if not normalize or not el.any():
        return q.copy()
    lo, hi = q[el].min(), q[el].max()
    return (q - lo) / (hi - lo) if hi - lo > 0 else np.zeros(len(el))


class _Rule:
    def __init__(self, K, q, el, normalize):
        self.K = np.asarray(K, dtype=np.float64)
        self.N = self.K.shape[0]
        self.el = np.ones(self.N, dtype=bool) if el is None else np.asarray(el).astype(bool)
        self.qh = qhat(q, self.el, normalize)
        self.S = []
        self.free = self.el.copy()

    def stops(self, best):
        return False

    def take(self, j):
        self.S.append(j)
        self.free[j] = False

    def _masked(self, v):
        return np.where(self.free, v, np.nan)


class MbrRule(_Rule):
    def __init__(self, K, q=None, el=None, normalize=True, reverse=False):
        super().__init__(K, q, el, normalize)
        ne = int(self.el.sum())
        self.s = np.zeros(self.N)
        order = range(self.N - 1, -1, -1) if reverse else range(self.N)
        for i in np.flatnonzero(self.el):
            tot = 0.0
            for j in order:
                if j != i and self.el[j]:
                    tot += self.K[i, j]
            self.s[i] = tot / (ne - 1) if ne > 1 else 0.0

    def objective(self):
        return self._masked(self.s)


class MmrRule(_Rule):
    def __init__(self, K, q, el=None, normalize=True, lam=0.5):
        super().__init__(K, q, el, normalize)
        self.lam = float(lam)

    def objective(self):
        if not self.S:
            return self._masked(self.qh)        # the first pick is argmax q^; its gain is lambda q^
        mx = self.K[:, self.S].max(axis=1)
        return self._masked(self.lam * self.qh - (1.0 - self.lam) * mx)

    def gain(self, v):
        return self.lam * v if not self.S else v


class _DppBase(_Rule):
    def __init__(self, K, q=None, el=None, normalize=True, theta=1.0, min_gain=1e-10):
        super().__init__(K, q, el, normalize)
        with np.errstate(over="ignore", invalid="ignore"):   # (a candidate that is not eligible may hold any quality)
            self.r = np.exp(float(theta) * self.qh)
            self.L = (self.r[:, None] * self.K) * self.r[None, :]
        self.min_gain = float(min_gain)

    def stops(self, best):
        return best < self.min_gain or not best > 0.0


class DppRule(_DppBase):
    """Chen, Zhang & Zhou's incremental update."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.d2 = np.diag(self.L).copy()
        self.c = np.zeros((self.N, 0))

    def objective(self):
        return self._masked(self.d2)

    def take(self, j):
        dj = np.sqrt(self.d2[j]) if self.d2[j] > 0 else np.nan
        dot = np.zeros(self.N)
        for u in range(self.c.shape[1]):            # components ascending
            dot = dot + self.c[j, u] * self.c[:, u]
        with np.errstate(over="ignore", invalid="ignore"):
            e = (self.L[j, :] - dot) / dj
            self.c = np.concatenate([self.c, e[:, None]], axis=1)
            self.d2 = self.d2 - e * e
        super().take(j)


class DppBruteRule(_DppBase):
    """det L_{S + i} / det L_S by slogdet for every remaining candidate: no state but S."""

    def objective(self):
        idx = np.flatnonzero(self.free)
        out = np.full(self.N, np.nan)
        if not len(idx):
            return out
        S_ = self.S
        base_sign, base_log = (1.0, 0.0) if not S_ else np.linalg.slogdet(self.L[np.ix_(S_, S_)])
        sub = np.stack([self.L[np.ix_(S_ + [i], S_ + [i])] for i in idx])
        sign, logdet = np.linalg.slogdet(sub)
        with np.errstate(over="ignore", invalid="ignore"):
            out[idx] = np.where(sign * base_sign > 0, np.exp(logdet - base_log), 0.0)
        return out


def make_rule(method, K, q, el, normalize=True, lam=0.5, theta=1.0, min_gain=1e-10):
    if method == MBR:
        return MbrRule(K, q, el, normalize)
    if method == MMR:
        return MmrRule(K, q, el, normalize, lam)
    return DppRule(K, q, el, normalize, theta, min_gain)


def _argmax(v):
    """Index of the largest non-NaN entry, the lowest on a tie; -1 when there is none."""
    ok = ~np.isnan(v)
    if not ok.any():
        return -1
    return int(np.flatnonzero(ok & (v == v[ok].max()))[0])


def run(rule, k, forced=None):
    """-> dict: picks (k,) int, gains (k,), n_primary, steps: per filled position (objective vector, primary?).  forced: follow
    these picks; a forced pick that is not available ends the run there (steps is then shorter than the filled positions)."""
    picks, gains, steps = np.full(k, -1, dtype=np.int64), np.zeros(k), []
    primary, n_primary, stop_value = True, 0, None
    for t in range(k):
        if primary:
            obj = rule.objective()
            j = _argmax(obj)
            if j < 0 or rule.stops(obj[j]):
                primary = False
                stop_value = None if j < 0 else float(obj[j])   # the best gain the rule refused
        if not primary:
            obj = rule._masked(rule.qh)
            j = _argmax(obj)
            if j < 0:
                break
        if forced is not None:
            j = int(forced[t])
            if j < 0 or j >= rule.N or np.isnan(obj[j]):
                break
        steps.append((obj, primary))
        picks[t] = j
        if primary:
            gains[t] = rule.gain(obj[j]) if hasattr(rule, "gain") else obj[j]
            n_primary += 1
            rule.take(j)
        else:
            _Rule.take(rule, j)
    return {"picks": picks, "gains": gains, "n_primary": n_primary, "steps": steps, "stop_value": stop_value}


def select(method, K, q=None, k=5, el=None, normalize=True, lam=0.5, theta=1.0, min_gain=1e-10):
    """All images: K (P, N, N), q (P, N) or None, el (P, N) or None -> picks (P, k), gains (P, k), n_primary (P,)."""
    out = [run(make_rule(method, K[p], None if q is None else q[p], None if el is None else el[p], normalize, lam, theta, min_gain), k)
           for p in range(len(K))]
    return (np.stack([o["picks"] for o in out]), np.stack([o["gains"] for o in out]), np.array([o["n_primary"] for o in out]))


# ---- judging picks ----------------------------------------------------------------------------------------------------------------

def undecided(obj, caps, tol):
    """True where the margin rule leaves a position out: a candidate with ANOTHER caption than the best one's has an objective
    within tol of the best.  One case is still compared: when every such candidate holds the best objective bit for bit (MBR of
    two captions: s_0 = K_01 = s_1; captions that share no n-gram with any other: s = 0), the tie is exact on both sides and the
    lowest index wins by the rule itself, not by rounding."""
    j = _argmax(obj)
    near = [obj[i] for i in range(len(obj)) if not np.isnan(obj[i]) and caps[i] != caps[j] and obj[j] - obj[i] <= tol]
    return any(v != obj[j] for v in near)


def judge(rule, k, caps, tol_rel, picks, gains=None, n_primary=None):
    """Follows `picks` through the rule.  At every filled position the pick must be a candidate whose objective is within tol of the
    best; where the best and the second-best DISTINCT caption differ by more than tol (or tie exactly: undecided()) the pick must be
    the best's caption.  gains
    (position by position) and n_primary are compared when given.  tol = tol_rel x the image's largest |gain| of the restatement.
    -> (positions, positions left out by the margin rule, largest gain deviation / scale)."""
    ref = run(rule, k, forced=picks)
    scale = max(1e-300, float(np.abs(ref["gains"]).max())) if k else 1.0
    tol = tol_rel * scale
    filled = int((np.asarray(picks) >= 0).sum())
    assert len(ref["steps"]) == filled, f"pick {picks[len(ref['steps'])]} at position {len(ref['steps'])} is not an available candidate"
    assert (np.asarray(picks)[filled:] == -1).all()
    skipped, dev = 0, 0.0
    for t, (obj, primary) in enumerate(ref["steps"]):
        j, best = int(picks[t]), _argmax(obj)
        assert obj[best] - obj[j] <= tol, f"position {t}: pick {j} has objective {obj[j]!r}, the best ({best}) {obj[best]!r}"
        if not undecided(obj, caps, tol):
            assert caps[j] == caps[best], f"position {t}: picked caption {caps[j]}, the best is {caps[best]}"
        else:
            skipped += 1
        if gains is not None:
            d = abs(gains[t] - ref["gains"][t])
            assert d <= tol, f"position {t}: gain {gains[t]!r}, restatement {ref['gains'][t]!r} (tol {tol:.3g})"
            dev = max(dev, d / scale)
    if gains is not None:
        assert not np.asarray(gains)[filled:].any()
    if n_primary is not None:
        assert int(n_primary) == ref["n_primary"], f"n_primary {n_primary}, restatement {ref['n_primary']}"
    # every eligible candidate is used before a -1 appears
    assert filled == min(k, int(rule.el.sum()))
    return filled, skipped, dev
