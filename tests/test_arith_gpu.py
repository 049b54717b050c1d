"""GPU: arithmetic sampling for the word samplers (include/ssc.h: ssc_arith).  The draw kernel (ssc_arith_rows) - its masses against
float64, its kept set against samplerref.filter_dist, token and new code bit for bit against the integer restatement
(tests/arithref.py) handed the device's own masses - and the lattice (ssc_arith_codes); the sampled decode along codes
(ssc_decode_sample_arith, DecodeEngine.sample) against the same decode driven step by step, against the call without it and against
the CPU oracle's CDF; share_latent; the module and scripts/inference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import arithref as R
import oracle
import samplerref
from oracle.seqcvae_oracle import cell_step, embed, output_logits, zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.inference import diverse_decode
from ssc_runtime.prefix import DecodePrefix
from test_attention_trace_gpu import R_, STEPS, VARIANTS, entry_inputs, medium, medium_params
from test_contrast_gpu import amateur_of, make_contrast, start_states
from test_latent_guide_gpu import bits, step_prior
from test_logit_rules_gpu import GUARD, SENTINEL, decode_inputs, padded, placed, yardstick_rules
from test_sampling_gpu import run_child
from test_truncation_gpu import NIMG, NS, SAMPLERS, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
TEMPS = (0.7, 1.0, 1.3)
N_ROWS = 7
LIVE = (0, 1, 2, 3, 4)
OP_END = 0      # the op-level END: inside [0, V) for V = 1 too
LAST = 7        # the last token of a live row (any value but OP_END: it is only compared)
# (V, ld, offset in floats past a 16-byte boundary): one word, a partial quad, one tile and a bit, the tile edge from below, at and
# above it (1024 = SAMPLE_THREADS quads), and the first Vs of the global form (above SAMPLE_LDS_MAX_V = 32768)
SHAPES = [(1, 1, 0), (5, 8, 1), (300, 300, 0), (1023, 1024, 1), (1024, 1028, 1), (1027, 1027, 0), (32771, 32772, 0)]
A_MAX = 25.0    # |a| = |(x - mx) / T| of every finite entry of the fixtures: every kept mass is at least 2^40 e^-25 = 15
P_BAND = 1e-6   # samplerref's: a top-p cut is decisive when no entry's mass ahead lies this close to p


def u64(values):
    """Python integers in [0, 2^64) -> the int64 tensor (on the device) that holds their bits"""
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)).cuda()


def ints(t):
    """an int64 tensor holding uint64 bits -> Python integers in [0, 2^64)"""
    return [int(v) for v in t.cpu().numpy().view(np.uint64).reshape(-1)]


def rows_case(V, ld, seed):
    """Seven rows whose finite entries span at most 17.5 (|a| <= 25 at T = 0.7): random; peaked; flat; values on a grid of 0.5 with
    the maximum three times - exact ties at a top-k cut and at the top; 30 % of the entries -inf; an ended row full of NaN; a row
    without a finite entry.  The pad columns are NaN.  -> (x (7, ld) float32, last_pred (7,) int64)"""
    rng = np.random.default_rng(seed)
    x = np.full((N_ROWS, ld), np.nan, dtype=np.float32)
    x[0, :V] = np.clip(rng.standard_normal(V) * 2.5, -8.5, 8.5)
    x[1, :V] = np.clip(rng.standard_normal(V), -3, 3)
    x[1, V // 3] = 14.0
    x[2, :V] = -1.25
    x[3, :V] = np.round(np.clip(rng.standard_normal(V) * 3, -8, 8) * 2) / 2
    x[3, [min(1, V - 1), V // 2, V - 1]] = x[3, :V].max() + 0.5
    x[4, :V] = np.clip(rng.standard_normal(V) * 2.5, -8.5, 8.5)
    x[4, :V][rng.random(V) < 0.3] = -np.inf
    if not np.isfinite(x[4, :V]).any():
        x[4, 0] = 0.5
    x[6, :V] = -np.inf
    last = np.full(N_ROWS, LAST, dtype=np.int64)
    last[5] = OP_END
    return x, last


def op_samplers(V):
    """(name, kind, top_k, top_p): multinomial, top-k inside the three-fold tie at the top of row 3 (k = 2) and - for the longer
    rows - inside the ties of its grid (k = 50), top-p"""
    s = [("multinomial", 0, 0, 1.0), ("top-k", 1, min(2, V), 1.0), ("top-p", 2, 0, 0.9)]
    if V >= 300:
        s.append(("top-k", 1, 50, 1.0))
    return s


class Out:
    """The guarded outputs of one ssc_arith_rows call"""

    def __init__(self, V, mass=True):
        self.pred_buf, self.pred = guarded(N_ROWS, torch.int64, -99)
        self.lp_buf, self.lp = guarded(N_ROWS, torch.float32, SENTINEL)
        self.code_buf, self.code = guarded(N_ROWS, torch.int64, -99)
        self.run_buf, self.run = guarded(N_ROWS, torch.float32, 0.5)
        self.mass_buf, self.mass = guarded(N_ROWS * V, torch.int64, -99) if mass else (None, None)

    def buffers(self):
        return [b for b in (self.pred_buf, self.lp_buf, self.code_buf, self.run_buf, self.mass_buf) if b is not None]

    def guards_intact(self):
        for b, fill in ((self.pred_buf, -99), (self.lp_buf, SENTINEL), (self.code_buf, -99), (self.run_buf, 0.5), (self.mass_buf, -99)):
            if b is not None and not (bool((b[:GUARD] == fill).all()) and bool((b[-GUARD:] == fill).all())):
                return False
        return True


def run_rows(view, ld, rows, V, sdesc, code_d, last_d, out, code_out=None):
    L.load().ssc_arith_rows(view.data_ptr(), ld, rows, V, C.byref(sdesc), L.ptr(code_d), L.ptr(last_d), L.ptr(out.run), OP_END, L.ptr(out.pred),
                            L.ptr(out.lp), L.ptr(out.code if code_out is None else code_out), L.ptr(out.mass), L.stream_ptr())
    torch.cuda.synchronize()


def plain_rows(view, ld, rows, V, sdesc, last_d):
    """ssc_sample_rows on the same rows -> (tokens, log-probs)"""
    pred = torch.full((rows,), -99, dtype=torch.int64, device="cuda")
    lp = torch.full((rows,), SENTINEL, device="cuda")
    L.load().ssc_sample_rows(view.data_ptr(), ld, rows, V, C.byref(sdesc), None, 0, L.ptr(last_d), None, OP_END, L.ptr(pred), L.ptr(lp), None,
                             L.stream_ptr())
    torch.cuda.synchronize()
    return pred, lp


@pytest.mark.parametrize("V,ld,off", SHAPES)
def test_rows_kernel_against_the_restatement(V, ld, off):
    """Per sampler and temperature.  MASSES: exactly 0 on cut and -inf entries, exactly 2^40 at the top, elsewhere within
    1e-5 w + 1 of float64 ((x - mx) / T is rounded twice in fp32 at |a| <= 25 - asserted -, plus a few ulp of expf).  KEPT SET (mass
    > 0: every kept mass of the fixtures is at least 15): samplerref.filter_dist's wherever no entry's mass ahead lies within 1e-6 of
    p.  AGAINST THE RESTATEMENT, handed the device's masses: token and new code bit-equal, for codes 0, 2^64 - 1 (t = W - 1), random
    ones, and codes built from the masses that draw word 0, word V - 1, words 1023 and 1024 on the tile edge (the nearest word with
    mass) at the first, a middle and the last t of the word; the log-prob within 1e-4 of float64.  The ended row (NaN logits) emits
    END at log-prob 0, the row without a finite entry what ssc_sample_rows yields for it, both keep their code; row_lp accumulates;
    pad columns and guards intact.  NULL mass_out, in-place codes and a second call give the same bits.  V = 1024: the 16-byte path
    (offset 0) gives the bits of the scalar path (offset 1)."""
    rng = np.random.default_rng(V)
    x, last = rows_case(V, ld, 1000 * V + 7)
    fin = np.isfinite(x[:5, :V])
    flat, view = placed(x, off)
    before = flat.clone()
    last_d = torch.from_numpy(last).cuda()
    decisive = checked = 0
    worst_mass = worst_lp = 0.0
    for name, kind, k, p in op_samplers(V):
        for T in TEMPS:
            tag = (V, ld, off, name, k, T)
            sdesc = L.SamplerDesc(kind, k, p, T, 99)
            x64 = x[:, :V].astype(np.float64)
            a_abs = max(np.abs((x64[r][fin[r]] - x64[r][fin[r]].max()) / T).max() for r in LIVE)
            assert a_abs <= A_MAX, (tag, a_abs)
            # ---- the first call: codes 0, the masses ---------------------------------------------------------------------------
            out = Out(V)
            run_rows(view, ld, N_ROWS, V, sdesc, u64([0] * N_ROWS), last_d, out)
            assert torch.equal(bits(flat), bits(before)) and out.guards_intact(), tag      # the logits are read only
            mass = out.mass.view(N_ROWS, V).cpu().numpy()
            plain_tok, plain_lp = plain_rows(view, ld, N_ROWS, V, sdesc, last_d)
            assert mass[5].tolist() == [R.MASS_ONE if v == OP_END else 0 for v in range(V)], tag
            assert not mass[6].any(), tag
            for r in LIVE:
                kept_ref = samplerref.filter_dist(np.where(fin[r], x64[r], -1e30), name, k, float(np.float32(p)), T)
                probs, ahead = kept_ref
                want_kept = (probs > 0) & fin[r]
                got_kept = mass[r] > 0
                assert not (got_kept & ~fin[r]).any(), tag                                  # -inf: exactly 0
                sure = name != "top-p" or not (np.abs(ahead[fin[r]] - float(np.float32(p))) < P_BAND).any()
                if sure:
                    decisive += 1
                    assert (got_kept == want_kept).all(), (tag, r, np.nonzero(got_kept != want_kept)[0][:8])
                w64 = R.masses64(x64[r], got_kept, T)
                err = np.abs(mass[r] - w64) - 1e-5 * w64
                worst_mass = max(worst_mass, float((np.abs(mass[r] - w64) / (1e-5 * w64 + 1)).max()))
                assert (err <= 1).all(), (tag, r, float(err.max()))
                top = fin[r] & (x64[r] == x64[r][fin[r]].max())
                assert mass[r].max() == R.MASS_ONE and mass[r][np.argmax(top)] == R.MASS_ONE, tag   # the lowest-index top word stays
                assert (mass[r][top & got_kept] == R.MASS_ONE).all(), tag
            # ---- the codes: fixed, random, and built from the device's masses ----------------------------------------------------
            code_sets = [[0] * N_ROWS, [R.MASK] * N_ROWS, [int(rng.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(N_ROWS)]]
            targets = []
            for v in sorted({0, V - 1, min(1023, V - 1), min(1024, V - 1)}):
                for frac in (0.0, 0.5, 1.0):
                    cs, tv = [], []
                    for r in range(N_ROWS):
                        nz = np.nonzero(mass[r])[0] if r in LIVE else np.array([], dtype=np.int64)
                        if nz.size == 0:
                            cs.append(12345 + r)
                            tv.append(None)
                            continue
                        u = int(nz[np.abs(nz - v).argmin()])
                        cs.append(R.code_for(mass[r], u, frac))
                        tv.append(u)
                    code_sets.append(cs)
                    targets.append((len(code_sets) - 1, tv))
                    if name == "multinomial":   # rows 0 to 3 hold mass everywhere: the exact words are drawn
                        assert tv[:4] == [v] * 4, tag
            for ci, codes in enumerate(code_sets):
                code_d = u64(codes)
                outs = []
                for _ in range(2):   # two calls on equal inputs
                    o = Out(V)
                    run_rows(view, ld, N_ROWS, V, sdesc, code_d, last_d, o)
                    outs.append(o)
                for b0, b1 in zip(outs[0].buffers(), outs[1].buffers()):
                    assert torch.equal(bits(b0), bits(b1)), tag
                o = outs[0]
                assert o.guards_intact() and torch.equal(bits(flat), bits(before)), tag
                assert torch.equal(o.mass, out.mass), tag                                     # the masses do not depend on the code
                tok, lp, code2, run = o.pred.tolist(), o.lp.cpu().numpy(), ints(o.code), o.run.cpu().numpy()
                for r in LIVE:
                    want_v, want_c = R.draw(mass[r], codes[r])
                    assert (tok[r], code2[r]) == (want_v, want_c), (tag, ci, r, tok[r], want_v, code2[r], want_c)
                    lse = x64[r][tok[r]] - np.log(np.exp(x64[r][fin[r]] - x64[r][fin[r]].max()).sum()) - x64[r][fin[r]].max()
                    worst_lp = max(worst_lp, abs(lp[r] - lse))
                    assert abs(lp[r] - lse) <= 1e-4, (tag, r, lp[r], lse)
                    assert run[r] == np.float32(0.5) + lp[r], tag
                    checked += 1
                for ti, tv in targets:
                    if ti == ci:
                        assert all(tok[r] == tv[r] for r in LIVE), (tag, ci)
                # the rows that pass through
                assert tok[5] == OP_END and lp[5] == 0.0 and code2[5] == codes[5] and run[5] == 0.5, tag
                assert tok[6] == int(plain_tok[6]) and code2[6] == codes[6], tag
                plain6 = plain_lp[6:7].cpu().numpy()
                assert (np.isnan(lp[6]) and np.isnan(plain6[0])) or lp[6:7].view(np.int32)[0] == plain6.view(np.int32)[0], tag
                if ci in (1, 2):
                    quiet = Out(V, mass=False)                                                # NULL mass_out changes nothing
                    run_rows(view, ld, N_ROWS, V, sdesc, code_d, last_d, quiet)
                    assert torch.equal(quiet.pred_buf, o.pred_buf) and torch.equal(bits(quiet.lp_buf), bits(o.lp_buf)), tag
                    assert torch.equal(quiet.code_buf, o.code_buf), tag
                    inplace = Out(V, mass=False)                                              # code_out = code_in
                    same = code_d.clone()
                    run_rows(view, ld, N_ROWS, V, sdesc, same, last_d, inplace, code_out=same)
                    assert torch.equal(same, o.code) and torch.equal(inplace.pred_buf, o.pred_buf), tag
                    if V == 1024:
                        flat0, view0 = placed(x, 0)
                        o0 = Out(V)
                        run_rows(view0, ld, N_ROWS, V, sdesc, code_d, last_d, o0)
                        for b0, b1 in zip(o0.buffers(), o.buffers()):
                            assert torch.equal(bits(b0), bits(b1)), tag
    print(f"V {V}: {checked} draws bit-equal to the restatement, {decisive} decisive kept sets, worst mass error "
          f"{worst_mass:.3f} of the bound, worst |lp - float64| {worst_lp:.2e}")
    assert decisive >= 5 * 2 * len(TEMPS)


def test_codes_kernel_is_the_restated_lattice():
    lib = L.load()
    for seed, nimg, n in ((5, 3, 1), (5, 3, 2), (2 ** 63 + 12345, 4, 5), (77, 2, 20), (77, 1, 7), (2 ** 64 - 1, 5, 64), (9, 300, 3)):
        buf, code = guarded(nimg * n, torch.int64, -99)
        lib.ssc_arith_codes(seed, nimg, n, L.ptr(code), L.stream_ptr())
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == -99).all()) and bool((buf[-GUARD:] == -99).all())
        assert ints(code) == [int(c) for c in R.codes(seed, nimg, n)], (seed, nimg, n)


def test_lattice_property_on_twenty_identical_rows():
    """20 rows with the same logits under the codes of ssc_arith_codes: every word's count of first-step draws is within 1 of
    20 w_v / W of the device's own masses - for a random and for a peaked row, the three samplers."""
    lib = L.load()
    n, V = 20, 300
    x, _ = rows_case(V, V, 4242)
    for r in (0, 1, 3):
        rows = torch.from_numpy(np.repeat(x[r:r + 1, :V], n, 0)).cuda().contiguous()
        for name, kind, k, p in op_samplers(V):
            for seed in (1, 2, 3):
                sdesc = L.SamplerDesc(kind, k, p, 1.0, seed)
                code = torch.zeros(n, dtype=torch.int64, device="cuda")
                lib.ssc_arith_codes(seed, 1, n, L.ptr(code), L.stream_ptr())
                pred = torch.zeros(n, dtype=torch.int64, device="cuda")
                lp = torch.zeros(n, device="cuda")
                mass = torch.zeros(n, V, dtype=torch.int64, device="cuda")
                lib.ssc_arith_rows(L.ptr(rows), V, n, V, C.byref(sdesc), L.ptr(code), None, None, OP_END, L.ptr(pred), L.ptr(lp), L.ptr(code),
                                   L.ptr(mass), L.stream_ptr())
                torch.cuda.synchronize()
                assert bool((mass == mass[0]).all())
                w = mass[0].cpu().numpy().astype(np.float64)
                count = np.bincount(pred.cpu().numpy(), minlength=V)
                dev = np.abs(count - n * w / w.sum()).max()
                assert dev < 1, (r, name, k, seed, dev)


# ---- the decode ---------------------------------------------------------------------------------------------------------------------------
MIRO = sampling.Mirostat(5.0, 0.3, mu0=6.0, unit="nats")
LATTICE = sampling.Arithmetic()


class ModeZero(sampling.Arithmetic):
    """An Arithmetic whose descriptor is off (mode 0) - DecodeEngine.sample hands it to ssc_decode_sample_arith all the same"""

    def desc(self, code):
        d = super().desc(code)
        d.mode = 0
        return d


class NullDesc(sampling.Arithmetic):
    """... and one whose descriptor is NULL"""

    def desc(self, code):
        return None


def drive(dec, ctx, sent_b, B, ns, steps, end, eps0, eps, sampler, seed, code0, miro=None, contrast=None, trunc=None, rules=None,
          start=None):
    """The sampled decode along codes driven from Python: per step DecodeEngine.step of the expert (and of a contrast's amateur),
    ssc_contrast_rows, ssc_logit_rules_rows, ssc_truncate_rows, ssc_mirostat_rows, ssc_arith_rows, ssc_mirostat_update.
    -> (tokens (B, steps), log-probs (B), codes (B, steps + 1), the first step's logits as they arrived at the draw)"""
    lib = L.load()
    V = dec.dims.V
    T = float(sampler.temperature)
    sdesc = sampler.desc(seed)
    rd = rules.desc(ns) if rules is not None else None
    run = torch.zeros(B, device="cuda")
    hist = torch.full((steps, B), -1, dtype=torch.int64, device="cuda")
    code = torch.zeros(steps + 1, B, dtype=torch.int64, device="cuda")
    code[0] = code0
    mu = torch.zeros(steps + 1, B, device="cuda")
    norm = torch.zeros(2, B, device="cuda")
    if miro is not None:
        md = miro.desc()
        mu[0] = md.mu0
    two = contrast is not None and contrast.alpha != 0
    if start is None:
        tokens, state = torch.full((B,), end, dtype=torch.int64, device="cuda"), None
        state_a = None
    else:
        tokens, state = start_states(dec, start, B, V, end)
        state_a = start_states(dec, contrast.start, B, V, end)[1] if two else None
    if two:
        a_dec, a_ctx, a_sent, a_eps0, a_eps = amateur_of(contrast, dec, ctx, sent_b, eps0, eps)
    last = None
    first = None
    for t in range(steps):
        pm, pv = step_prior(None, t, B, 1, sent_b, dec.dims)
        logits, state, _ = dec.step(ctx, tokens, state, sent_b, eps0 if t == 0 else eps[t - 1], raw_logits=True, prior_mean=pm, prior_var=pv)
        if contrast is not None:
            logits_a = None
            if two:
                logits_a, state_a, _ = a_dec.step(a_ctx, tokens, state_a, a_sent, a_eps0 if t == 0 else a_eps[t - 1], raw_logits=True,
                                                  prior_mean=pm, prior_var=pv)
            lib.ssc_contrast_rows(L.ptr(logits), V, L.ptr(logits_a), V, B, V, contrast.alpha, contrast.beta, L.ptr(last), end, None, None,
                                  L.stream_ptr())
        if rd is not None:
            lib.ssc_logit_rules_rows(L.ptr(logits), V, B, V, C.byref(rd[0]), L.ptr(hist), B, t, end, L.stream_ptr())
        if trunc is not None:
            td = trunc.desc(None, None)
            lib.ssc_truncate_rows(L.ptr(logits), V, B, V, C.byref(td), T, L.ptr(last), end, L.stream_ptr())
        if miro is not None:
            lib.ssc_mirostat_rows(L.ptr(logits), V, B, V, T, L.ptr(mu[t]), L.ptr(last), end, None, L.ptr(norm), L.stream_ptr())
        if t == 0:
            first = logits.clone()
        slp = torch.empty(B, device="cuda")
        lib.ssc_arith_rows(L.ptr(logits), V, B, V, C.byref(sdesc), L.ptr(code[t]), L.ptr(last), L.ptr(run), end, L.ptr(hist[t]), L.ptr(slp),
                           L.ptr(code[t + 1]), None, L.stream_ptr())
        if miro is not None:
            lib.ssc_mirostat_update(L.ptr(logits), V, B, V, T, md.tau, md.eta, L.ptr(norm), L.ptr(hist[t]), L.ptr(last), end, L.ptr(mu[t]),
                                    L.ptr(mu[t + 1]), None, L.stream_ptr())
        last = tokens = hist[t]
    return hist.t().contiguous(), run, code.t().contiguous(), first


def lattice_codes(seed, nimg, ns):
    return u64(R.codes(seed, nimg, ns))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_arith_decode_against_the_stepwise_driver(variant):
    """The one call gives the tokens, the log-probs and every code slab of the same decode driven step by step, bit for bit: each
    sampler, alone with skip_dead / early_stop on and off and an attention trace, with logit rules + a truncation + a contrast +
    Mirostat active together, and from a prefix start state (the codes start at the continuation's first step)."""
    cfg, _, _, dec = medium(variant)
    end, V = cfg.boundary_index, cfg.vocab_size
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    B = NIMG * NS
    rules = yardstick_rules(V, NIMG)
    tr = sampling.MinPTruncation(0.05)
    g = torch.Generator().manual_seed(3)
    prefix = torch.full((NIMG, 2), -1, dtype=torch.int64)
    prefix[1, :1] = torch.randint(2, V, (1,), generator=g)
    prefix[2, :2] = torch.randint(2, V, (2,), generator=g)
    peps = torch.randn(2, B, cfg.z_space, generator=g).cuda()
    flags = ((True, True, False), (False, False, False), (True, False, True), (False, True, False))
    code0 = lattice_codes(13, NIMG, NS)
    differs = False
    for name, smp in SAMPLERS.items():
        ctx = dec.prepare(feats)
        con = make_contrast("features", variant).prepare(dec, ctx.feats)
        plain, _ = dec.sample(ctx, sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=False)
        for what, kw, runs in (("alone", dict(), flags), ("rules+trunc+contrast+mirostat", dict(rules=rules, trunc=tr, contrast=con, miro=MIRO), flags[:2]),
                               ("prefix", dict(start=True), flags[:1])):
            dkw = dict(kw)
            if dkw.get("start"):
                dkw["start"] = dec.prime(ctx, sent_b, NS, DecodePrefix(prefix), end, peps)
            want = drive(dec, ctx, sent_b, B, NS, STEPS, end, eps0, eps, smp, 13, code0, **dkw)
            skw = {{"rules": "logit_rules", "trunc": "truncation", "miro": "mirostat"}.get(k, k): v for k, v in dkw.items()}
            for skip_dead, early_stop, attention in runs:
                out = dec.sample(ctx, sent_b, NS, STEPS, end, eps0, eps, smp, 13, early_stop=early_stop, attention=attention,
                                 skip_dead=skip_dead, arithmetic=LATTICE, arithmetic_codes=True, **skw)
                pred, lp, codes = out[0], out[1], out[-1]
                tag = (variant, name, what, skip_dead, early_stop, attention)
                n = pred.size(1)
                assert codes.shape == (B, n + 1) and codes.dtype == torch.int64, tag
                assert torch.equal(padded(pred, STEPS, end), want[0]), tag
                assert torch.equal(bits(lp), bits(want[1])), (tag, (lp - want[1]).abs().max().item())
                assert torch.equal(codes, want[2][:, :n + 1]), tag
                if attention:
                    assert dec.attention(out[2]).top_region.shape == (B, STEPS)
            assert torch.equal(want[2][:, 0], code0), (variant, name, what)    # under a prefix too: the lattice at the continuation
            if what == "alone":
                differs |= not torch.equal(want[0], plain)
    assert differs, "the arithmetic draw gave the plain samplers' words everywhere"


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_off_path_is_the_call_without_arithmetic(variant):
    """A mode-0 and a NULL descriptor handed to ssc_decode_sample_arith give the predictions and the log-probs of
    ssc_decode_sample_opts / ssc_decode_sample_mirostat, bit for bit - alone and under Mirostat; mode 2 with the lattice written by
    the caller is mode 1, bit for bit in tokens, log-probs and codes."""
    cfg, _, _, dec = medium(variant)
    feats, sent_b, eps0, eps = decode_inputs(cfg)
    ctx = dec.prepare(feats)
    seen = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("ssc_decode_sample") and not name.endswith("workspace_bytes"):
                seen.append(name)
            return getattr(self._lib, name)

    lib = dec.lib
    dec.lib = Spy(lib)
    try:
        for name, smp in SAMPLERS.items():
            args = (ctx, sent_b, NS, STEPS, cfg.boundary_index, eps0, eps, smp, 13)
            for kw in (dict(), dict(mirostat=MIRO)):
                del seen[:]
                pred0, lp0 = dec.sample(*args, **kw)
                assert seen == ["ssc_decode_sample_mirostat" if kw else "ssc_decode_sample_opts"], seen   # (None: the call of before)
                for off in (ModeZero(), NullDesc()):
                    del seen[:]
                    pred, lp = dec.sample(*args, arithmetic=off, **kw)
                    assert seen == ["ssc_decode_sample_arith"], seen
                    assert torch.equal(pred, pred0) and torch.equal(bits(lp), bits(lp0)), (variant, name, type(off).__name__, list(kw))
                mode1 = dec.sample(*args, arithmetic=LATTICE, arithmetic_codes=True, **kw)
                mine = sampling.Arithmetic(lattice_codes(13, NIMG, NS).view(torch.uint64))
                mode2 = dec.sample(*args, arithmetic=mine, arithmetic_codes=True, **kw)
                assert torch.equal(mode1[0], mode2[0]) and torch.equal(bits(mode1[1]), bits(mode2[1])) and torch.equal(mode1[2], mode2[2])
                other = dec.sample(*args[:-1], 14, arithmetic=LATTICE, arithmetic_codes=True, **kw)
                assert not torch.equal(other[2][:, 0], mode1[2][:, 0])                  # the seed decides the shifts
    finally:
        dec.lib = lib


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
ORACLE_SAMPLERS = {"T1": sampling.MultinomialSampler(1.0), "T0.7": sampling.MultinomialSampler(0.7), "T1.3": sampling.MultinomialSampler(1.3)}


@pytest.mark.parametrize("temp", list(ORACLE_SAMPLERS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_arith_decode_against_the_oracle(variant, temp):
    """The device's words teacher-forced through the oracle's decode step with the same noise: for EVERY live (step, row) the
    device's code c / 2^64 lies in [F(w - 1) - band, F(w) + band] of the oracle's float64 CDF, in vocabulary order, of the
    tempered distribution at the drawn word w; band = 2 * 1e-4 / T (the project's 1e-4 logit parity: a probability's relative error
    is at most about 2e-4 / T, so is a CDF value's absolute error)."""
    cfg, params = medium_params(variant)
    _, _, _, dec = medium(variant)
    smp = ORACLE_SAMPLERS[temp]
    T = float(smp.temperature)
    band = 2 * 1e-4 / T
    feats, senti, eps0, eps = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    B, end = NIMG * NS, cfg.boundary_index
    sent_b = senti.view(NIMG, 1).expand(NIMG, NS).reshape(B) if senti is not None else None
    pred, _, codes = dec.sample(dec.prepare(feats.cuda()), sent_b.cuda() if sent_b is not None else None, NS, STEPS, end, eps0.cuda(),
                                eps.cuda(), smp, 77, early_stop=False, arithmetic=LATTICE, arithmetic_codes=True)
    pred = pred.cpu()
    c = codes.cpu().numpy().view(np.uint64).astype(np.float64) / 2.0 ** 64      # (B, steps + 1); 2^-53 relative: far below the band
    fr = feats.unsqueeze(1).expand(NIMG, NS, feats.size(1), feats.size(2)).reshape(B, feats.size(1), -1)
    se = sent_b.view(B, 1) if sent_b is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
    states = zero_states(B, cfg.hidden_size, fr)
    tokens = torch.full((B,), end, dtype=torch.long)
    alive = np.ones(B, dtype=bool)
    checked, worst = 0, 0.0
    with torch.no_grad():
        for t in range(STEPS):
            e = eps0 if t == 0 else eps[t - 1]
            h_dec, states, _, _, _, _ = cell_step(params, cfg, fr, embed(params, cfg, tokens), states, False, se, pm, pv, e, None, None, True)
            logits = output_logits(params, cfg, h_dec).double().numpy()
            for b in range(B):
                w = int(pred[b, t])
                if not alive[b]:
                    assert w == end
                    continue
                z = logits[b] / T
                q = np.exp(z - z.max())
                F = np.cumsum(q / q.sum())
                lo, hi = (F[w - 1] if w > 0 else 0.0), F[w]
                worst = max(worst, lo - c[b, t], c[b, t] - hi)           # how far outside the oracle's own interval
                assert lo - band <= c[b, t] <= hi + band, (variant, temp, b, t, w, lo, c[b, t], hi)
                checked += 1
            alive &= (pred[:, t] != end).numpy()
            tokens = pred[:, t].clone()
    print(f"{variant} {temp}: {checked} live (step, row) pairs, the code at most {worst:.2e} outside the oracle's own interval (band {band:.1e})")
    assert checked >= B


# ---- share_latent and the interface ------------------------------------------------------------------------------------------------------------
def test_share_latent_gives_an_image_one_latent_and_a_lattice_of_first_words():
    """diverse_decode(arithmetic=Arithmetic(share_latent=True)) with 20 samples per image: DecodeEngine.sample is handed noise whose
    rows are equal within an image - contiguous tensors -, so the first-step logits of an image's rows are equal, and the returned
    first words are the draws of ssc_arith_rows along ssc_arith_codes' lattice on those logits and obey the lattice property
    against the device's masses.  Without share_latent the rows' noise differs."""
    cfg, _, _, dec = medium("untied-sv1")
    lib = L.load()
    nimg, ns = 3, 20
    B, V, end = nimg * ns, cfg.vocab_size, cfg.boundary_index
    feats, senti, _, _ = entry_inputs(cfg, nimg, 1, R_, 17, STEPS)
    smp = sampling.MultinomialSampler(1.0)
    seen = {}
    sample = dec.sample

    def spy(ctx, sent_b, n, steps, e, eps0, eps, *a, **kw):
        seen.update(ctx=ctx, sent_b=sent_b, eps0=eps0, eps=eps)
        return sample(ctx, sent_b, n, steps, e, eps0, eps, *a, **kw)

    dec.sample = spy
    try:
        torch.manual_seed(3)
        caps, _ = diverse_decode(dec, feats.cuda(), senti.cuda(), ns, 1, STEPS, end, sampler=smp, sample_seed=9,
                                 arithmetic=sampling.Arithmetic(share_latent=True))
        eps0, eps = seen["eps0"], seen["eps"]
        assert eps0.is_contiguous() and eps.is_contiguous() and eps0.shape == (B, cfg.z_space)
        assert bool((eps0.view(nimg, ns, -1) == eps0.view(nimg, ns, -1)[:, :1]).all())
        assert bool((eps.view(eps.size(0), nimg, ns, -1) == eps.view(eps.size(0), nimg, ns, -1)[:, :, :1]).all())
        assert not torch.equal(eps0[0], eps0[ns])                                       # the images' latents differ
        tokens = torch.full((B,), end, dtype=torch.int64, device="cuda")
        logits, _, _ = dec.step(seen["ctx"], tokens, None, seen["sent_b"], eps0, raw_logits=True)
        rows = logits.view(nimg, ns, V)
        assert torch.equal(bits(rows), bits(rows[:, :1].expand_as(rows).contiguous()))
        code = torch.zeros(B, dtype=torch.int64, device="cuda")
        lib.ssc_arith_codes(9, nimg, ns, L.ptr(code), L.stream_ptr())
        pred = torch.zeros(B, dtype=torch.int64, device="cuda")
        lp = torch.zeros(B, device="cuda")
        mass = torch.zeros(B, V, dtype=torch.int64, device="cuda")
        sdesc = smp.desc(9)
        lib.ssc_arith_rows(L.ptr(logits), V, B, V, C.byref(sdesc), L.ptr(code), None, None, end, L.ptr(pred), L.ptr(lp), L.ptr(code), L.ptr(mass),
                           L.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(caps[:, :, 0].reshape(B), pred)
        for i in range(nimg):
            w = mass[i * ns].cpu().numpy().astype(np.float64)
            count = np.bincount(pred[i * ns:(i + 1) * ns].cpu().numpy(), minlength=V)
            assert np.abs(count - ns * w / w.sum()).max() < 1, i
        torch.manual_seed(3)
        diverse_decode(dec, feats.cuda(), senti.cuda(), ns, 1, STEPS, end, sampler=smp, sample_seed=9, arithmetic=LATTICE)
        assert not bool((seen["eps0"].view(nimg, ns, -1) == seen["eps0"].view(nimg, ns, -1)[:, :1]).all())
    finally:
        dec.sample = sample


def test_diverse_decode_takes_an_arithmetic():
    cfg, _, _, dec = medium("untied-sv1")
    feats, senti, _, _ = entry_inputs(cfg, NIMG, NS, R_, 17, STEPS)
    end = cfg.boundary_index
    kw = dict(sampler=sampling.MultinomialSampler(1.0), sample_seed=9)

    def run(**more):
        torch.manual_seed(3)
        return diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, **kw, **more)

    plain, _ = run()
    on, k = run(arithmetic=LATTICE)
    again, _ = run(arithmetic=LATTICE)
    assert torch.equal(on, again) and on.shape == (NIMG, NS, k) and not torch.equal(on, plain)
    # composes with logit rules, a truncation, Mirostat, a contrast, a prefix and an attention trace
    rules = sampling.LogitRules(no_repeat_ngram=1, min_length=3)
    prefix = DecodePrefix(torch.tensor([[5, 6], [7, -1], [-1, -1]]))
    caps, _ = run(arithmetic=sampling.Arithmetic(share_latent=True), logit_rules=rules, truncation=sampling.EtaTruncation(0.01), prefix=prefix,
                  mirostat=MIRO)
    assert caps[0, :, :2].tolist() == [[5, 6]] * NS and caps[1, :, 0].tolist() == [7] * NS
    out = run(arithmetic=LATTICE, mirostat=MIRO, mirostat_stats=True, logit_rules=rules, attention="summary",
              contrast=make_contrast("features", "untied-sv1"), contrast_stats=True)
    assert out[2].top_region.shape[:2] == (NIMG, NS) and len(out[3]) == 2 and len(out[4]) == 3 and out[4][0].shape == out[0].shape
    for more, name in ((dict(sampler=None), "not the beam search"), (dict(sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                       (dict(sampled_beam=True), "sampled-node beam search"),
                       (dict(sampler=None, diverse_beam=sampling.DiverseBeam(1, 0.5)), "diverse beam search")):
        with pytest.raises(ValueError, match="arithmetic sampling belongs to the word samplers.*" + name):
            diverse_decode(dec, feats.cuda(), senti.cuda(), NS, 1, STEPS, end, arithmetic=LATTICE, **{**kw, **more})


MODULE_SCRIPT = r"""
import json, sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from ssc_runtime.config import Config
from ssc_runtime import sampling
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner
C = Config(config_override=["RANDOM_SEED", 3, "MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", 3, "MODEL.BEAM_SIZE", 1,
                            "MODEL.IMAGE_FEATURE_SIZE", 64, "MODEL.EMBEDDING_SIZE", 40, "MODEL.HIDDEN_SIZE", 48,
                            "MODEL.ATTENTION_PROJECTION_SIZE", 32, "MODEL.Z_SPACE", 16, "DATA.MAX_CAPTION_LENGTH", 8] + {keys!r})
def run(arithmetic="config"):
    torch.manual_seed(C.RANDOM_SEED)
    m = UpDownCaptioner.from_config(C, vocabulary=Vocabulary.synthetic(120), device=torch.device("cuda"),
                                    sampler=sampling.from_config(C.MODEL)).cuda().eval()
    if arithmetic != "config":
        m.arithmetic(arithmetic)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(1, 6, 64, generator=g).expand(8, 6, 64).contiguous().cuda()
    return m(feats)["predictions"].cpu().tolist()
print(json.dumps([run(), run(None), run(sampling.Arithmetic())]))
"""


def test_module_reads_the_keys_and_takes_an_arithmetic_in_a_child_process():
    """The eval forward of a top-k (k = 3) module: with the keys at their defaults it is the forward without arithmetic sampling;
    with MODEL.SAMPLER_ARITHMETIC set it differs and is the forward of arithmetic(Arithmetic()); arithmetic(None) switches the
    keys' choice off again."""
    pkg = os.path.join(ROOT, "style-seqcvae_amd")
    outs = {}
    for name, keys in (("off", []), ("on", ["MODEL.SAMPLER_ARITHMETIC", True])):
        src = MODULE_SCRIPT.format(root=ROOT, pkg=pkg, keys=keys)
        outs[name] = json.loads(run_child(["-c", src]).strip().splitlines()[-1])
    plain, plain_none, plain_on = outs["off"]
    keyed, keyed_none, keyed_on = outs["on"]
    assert plain == plain_none == keyed_none
    assert keyed != plain and keyed == keyed_on == plain_on
    assert len(keyed) == 8 and all(0 < len(c) <= 8 for c in keyed)


SCRIPT_YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 8\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
               "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
               "  BEAM_SIZE: 1\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
               "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 5\n  DECODE_SAMPLER: top-k\n  SAMPLER_TOP_K: 4\n")


def test_inference_script_with_the_arithmetic_flags(tmp_path):
    """scripts/inference.py: --arithmetic writes other captions than the run without it, the same as the key; with
    --arithmetic-share-latent the captions change again, the same as both keys; the flag without a word sampler is refused."""
    import subprocess
    import sys
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(SCRIPT_YAML)
    script = os.path.join(ROOT, "scripts", "inference.py")
    base = [script, "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4", "--vocab-size", "150", "--num-boxes", "5"]

    def run(name, *extra):
        out = tmp_path / (name + ".json")
        run_child(base + ["--output-path", str(out)] + list(extra))
        return out.read_bytes()

    plain = run("plain")
    on = run("on", "--arithmetic")
    assert on != plain and len(json.loads(on)) == 4 * 5
    assert on == run("keys", "--config-override", "MODEL.SAMPLER_ARITHMETIC", "True")
    shared = run("shared", "--arithmetic", "--arithmetic-share-latent")
    assert shared != on and len(json.loads(shared)) == 4 * 5
    assert shared == run("keys2", "--config-override", "MODEL.SAMPLER_ARITHMETIC", "True", "MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT", "True")
    r = subprocess.run([sys.executable] + base + ["--output-path", str(tmp_path / "x.json"), "--arithmetic", "--config-override",
                                                  "MODEL.DECODE_SAMPLER", "beam"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--arithmetic needs a word sampler" in r.stderr, r.stderr[-2000:]
