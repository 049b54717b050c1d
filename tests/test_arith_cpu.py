"""CPU: arithmetic sampling for the word samplers (include/ssc.h: ssc_arith) - the restatement (tests/arithref.py) against brute force
with Python's big integers and fractions, the lattice property, the exactness of the marginals over two steps, the class, the config
keys and their refusals, the struct and the bindings against the header, every refusal of the four new symbols (no launch is reached:
no GPU needed), the workspace size, the runtime's refusals and those of scripts/inference.py."""
import ctypes as C
import math
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import arithref as R
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config
from ssc_runtime.decode import DecodeEngine, EnsembleDecodeEngine
from ssc_runtime.engine import ModelDims
from ssc_runtime.inference import diverse_decode
from ssc_runtime.vocab import Vocabulary
from test_attention_trace_cpu import CFG, header, model_cfg, sample_opts, search_desc, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 1
LATTICE_NS = (1, 2, 5, 20)


def random_masses(rng, V, spread=6.0, holes=0.2):
    """V integer masses as the device forms them: the top word 2^40, the others exp(-|N(0, spread)|) 2^40 rounded, some cut (0)"""
    a = -np.abs(rng.standard_normal(V) * spread)
    a[rng.integers(V)] = 0.0
    w = np.rint(np.exp(a) * R.MASS_ONE).astype(np.int64)
    w[(rng.random(V) < holes) & (a < 0)] = 0
    return [int(x) for x in w]


# ---- division and lattice against brute force ---------------------------------------------------------------------------------------------
def test_division_against_big_integers():
    rnd = random.Random(5)
    cases = [(0, 0, 1), (0, R.MASK, 1), (R.MASS_ONE - 1, R.MASK, R.MASS_ONE), (0, 1, R.MASS_ONE), (1, 0, 2), (2, R.MASK, 3)]
    for _ in range(2000):
        w = rnd.randint(1, R.MASS_ONE) if rnd.random() < 0.7 else rnd.randint(1, 1000)
        cases.append((rnd.randrange(w), rnd.getrandbits(64), w))
    for hi, lo, w in cases:
        n = (hi << 64) + lo
        assert R.divide(hi, lo, w) == (n // w, n % w), (hi, lo, w)
        assert n // w <= R.MASK


def test_draw_against_fractions():
    """The token is the word whose interval of the exact CDF holds c / 2^64, and the new code is the floor of the exact position
    inside that interval, times 2^64."""
    rng = np.random.default_rng(11)
    rnd = random.Random(11)
    for V in (1, 2, 7, 300):
        for _ in range(30):
            w = random_masses(rng, V)
            W = sum(w)
            for c in [0, R.MASK, 1 << 63, rnd.getrandbits(64), rnd.getrandbits(64), rnd.getrandbits(20)]:
                v, c2 = R.draw(w, c)
                x = Fraction(c, 1 << 64)
                # the device's t is floor(x W): the interval test on integers is the one on x W
                lo_edge, hi_edge = Fraction(sum(w[:v])), Fraction(sum(w[:v + 1]))
                assert lo_edge <= math.floor(x * W) < hi_edge, (V, c)
                inside = (x * W - lo_edge) / w[v]
                assert 0 <= inside < 1 and c2 == math.floor(inside * (1 << 64)), (V, c)
    assert R.draw([0, 0, 0], 12345) == (None, 12345)
    assert R.draw([0, 5, 0], 0) == (1, 0) and R.draw([0, 5, 0], R.MASK)[0] == 1


def test_lattice_against_fractions():
    rnd = random.Random(3)
    for n in (1, 2, 3, 5, 20, 64, 1000, (1 << 24) - 1, 1 << 24):
        u = rnd.getrandbits(64)
        js = range(n) if n <= 1000 else [0, 1, 2, n // 2, n - 2, n - 1]
        full = R.lattice(u, n) if n <= 1000 else None
        for j in js:
            want = (u + math.floor(Fraction(j << 64, n))) & R.MASK
            got = full[j] if full is not None else (u + (j << 64) // n) & R.MASK
            assert got == want
            # the device's form: 2^64 = q n + r, floor(j 2^64 / n) = j q + floor(j r / n), every product below 2^64
            q, r = R.MASK // n, R.MASK % n + 1
            if r == n:
                q, r = (q + 1) & R.MASK, 0
            assert j * r < 1 << 64 and (u + j * q + j * r // n) & R.MASK == want
    codes = R.codes(77, 3, 4)
    assert codes.dtype == np.uint64 and codes.shape == (12,)
    u = R.shifts(77, 3)
    assert len(set(u)) == 3 and [int(codes[4 * i]) for i in range(3)] == u
    assert R.shifts(77, 3) != R.shifts(78, 3)


# ---- the lattice property -------------------------------------------------------------------------------------------------------------------
def test_lattice_property():
    """N rows with equal masses whose codes are a shifted lattice: every word is drawn floor or ceil of its expected count -
    |count - N w_v / W| < 1 - on 200 random rows of V = 300 for N in {1, 2, 5, 20}."""
    rng = np.random.default_rng(2023)
    rnd = random.Random(2023)
    worst = 0.0
    for _ in range(200):
        w = random_masses(rng, 300)
        W = sum(w)
        for n in LATTICE_NS:
            count = [0] * 300
            for c in R.lattice(rnd.getrandbits(64), n):
                count[R.draw(w, c)[0]] += 1
            dev = max(abs(count[v] - Fraction(n * w[v], W)) for v in range(300))
            assert dev < 1, (n, float(dev))
            worst = max(worst, float(dev))
    print(f"lattice property: worst |count - N w / W| {worst:.5f}")


# ---- marginal exactness ---------------------------------------------------------------------------------------------------------------------
def test_two_steps_of_uniform_codes_draw_the_product_distribution():
    """Uniform random codes (fixed seed): the joint frequencies of two successive steps - the second drawn with the code the first
    left - are within 4 sigma of the binomial of p (x) q, for every pair of words."""
    rnd = random.Random(1234)
    rng = np.random.default_rng(1234)
    w1 = [R.MASS_ONE, R.MASS_ONE // 3, 0, R.MASS_ONE // 7, 5]
    w2 = random_masses(rng, 6, spread=1.5, holes=0.0)
    p = [Fraction(x, sum(w1)) for x in w1]
    q = [Fraction(x, sum(w2)) for x in w2]
    n = 40000
    joint = np.zeros((len(w1), len(w2)), dtype=np.int64)
    for _ in range(n):
        a, c = R.draw(w1, rnd.getrandbits(64))
        b, _ = R.draw(w2, c)
        joint[a, b] += 1
    worst = 0.0
    for a in range(len(w1)):
        for b in range(len(w2)):
            pr = float(p[a] * q[b])
            sigma = math.sqrt(n * pr * (1 - pr))
            if pr == 0:
                assert joint[a, b] == 0
                continue
            z = abs(joint[a, b] - n * pr) / sigma
            worst = max(worst, z)
            assert z <= 4.0, (a, b, int(joint[a, b]), n * pr, sigma)
    print(f"marginal exactness: worst deviation {worst:.2f} sigma over {len(w1) * len(w2)} cells")


# ---- the class and the keys -----------------------------------------------------------------------------------------------------------------
def test_arithmetic_class_and_arguments():
    a = sampling.Arithmetic()
    assert a.lattice and a.share_latent is False and "lattice" in repr(a)
    assert sampling.Arithmetic("lattice", share_latent=True).share_latent is True
    given = sampling.Arithmetic(torch.zeros(6, dtype=torch.uint64))
    assert not given.lattice
    assert not sampling.Arithmetic(torch.zeros(6, dtype=torch.int64)).lattice
    for bad in ("sobol", 3, None, torch.zeros(6), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)):
        with pytest.raises(ValueError, match="arithmetic codes"):
            sampling.Arithmetic(bad)
    with pytest.raises(ValueError, match="share_latent"):
        sampling.Arithmetic(share_latent=1)
    # desc: mode 1 for the lattice, mode 2 with the caller's codes copied into slab 0 (the uint64 bits)
    block = torch.full((4, 6), 7, dtype=torch.int64)
    d = a.desc(block)
    assert d.mode == 1 and d.code == block.data_ptr() and bool((block == 7).all())
    mine = torch.tensor([0, 1, 2, 3, 2 ** 63 - 1, -1], dtype=torch.int64)
    d = sampling.Arithmetic(mine.view(torch.uint64)).desc(block)
    assert d.mode == 2 and torch.equal(block[0], mine) and bool((block[1:] == 7).all())
    with pytest.raises(ValueError, match="6 entries for 5 rows"):
        sampling.Arithmetic(mine).desc(torch.zeros(4, 5, dtype=torch.int64))


TOPP = ["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", 0.95, "MODEL.BEAM_SIZE", 1]


def test_config_keys():
    c = Config()
    assert c.MODEL.SAMPLER_ARITHMETIC is False and c.MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT is False
    assert sampling.arithmetic_from_config(c.MODEL) is None and sampling.arithmetic_from_config(Config(config_override=TOPP).MODEL) is None
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_ARITHMETIC", True])
    a = sampling.arithmetic_from_config(c.MODEL)
    assert a.lattice and not a.share_latent and isinstance(sampling.from_config(c.MODEL), sampling.TopPSampler)
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_ARITHMETIC", True, "MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT", True])
    assert sampling.arithmetic_from_config(c.MODEL).share_latent
    for other, match in (([], "needs MODEL.DECODE_SAMPLER"), (["MODEL.STOCHASTIC_BEAM_SEARCH", True], "needs MODEL.DECODE_SAMPLER"),
                         (["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLED_BEAM_SEARCH", True], "SAMPLED_BEAM_SEARCH exclude")):
        c = Config(config_override=["MODEL.SAMPLER_ARITHMETIC", True] + other)
        for read in (lambda: sampling.arithmetic_from_config(c.MODEL), lambda: sampling.from_config(c.MODEL)):
            with pytest.raises(ValueError, match=match) as e:
                read()
            assert "MODEL.SAMPLER_ARITHMETIC" in str(e.value)
    for override in (["MODEL.SAMPLER_ARITHMETIC", 1], ["MODEL.SAMPLER_ARITHMETIC", "yes"], ["MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT", 0.5]):
        with pytest.raises(ValueError, match=override[0].split(".")[1]):
            Config(config_override=TOPP + override)
    with pytest.raises(ValueError, match="SAMPLER_ARITHMETIC_SHARE_LATENT needs MODEL.SAMPLER_ARITHMETIC"):
        Config(config_override=TOPP + ["MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT", True])


def test_a_model_reads_the_keys_with_a_word_sampler_only():
    from var_updown.models import UpDownCaptioner
    small = ["MODEL.IMAGE_FEATURE_SIZE", 8, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
             "MODEL.Z_SPACE", 4]
    c = Config(config_override=TOPP + ["MODEL.SAMPLER_ARITHMETIC", True] + small)
    vocab = Vocabulary.synthetic(40)
    m = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu")     # (no sampler: the keys are not read)
    assert m._arithmetic is None
    with pytest.raises(ValueError, match="needs a word sampler"):
        m.arithmetic(sampling.Arithmetic())
    m.arithmetic(None)
    s = UpDownCaptioner.from_config(c, vocabulary=vocab, device="cpu", sampler=sampling.from_config(c.MODEL))
    assert isinstance(s._arithmetic, sampling.Arithmetic) and s._arithmetic.lattice
    s.arithmetic(None)
    assert s._arithmetic is None
    with pytest.raises(ValueError, match="Arithmetic or None"):
        s.arithmetic(sampling.Mirostat())
    off = UpDownCaptioner.from_config(Config(config_override=TOPP + small), vocabulary=vocab, device="cpu",
                                      sampler=sampling.TopPSampler(p=0.95))
    assert off._arithmetic is None


# ---- the struct and the bindings against the header -----------------------------------------------------------------------------------------
NEW = ("ssc_arith_codes", "ssc_arith_rows", "ssc_decode_sample_arith_workspace_bytes", "ssc_decode_sample_arith")


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
    return [a.strip() for a in m.group(1).split(",")]


def test_bindings_mirror_the_header():
    assert struct_fields("ssc_arith") == [f for f, _ in L.Arith._fields_] == ["mode", "code"]
    assert C.sizeof(L.Arith) == 16
    cdll = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(cdll, name), name
        args = declaration(name)
        assert len(args) == len(L.SYMBOLS[name][1]), name
        for a, ct in zip(args, L.SYMBOLS[name][1]):   # scalars by type, everything else a pointer
            want = (C.c_float if a.startswith("float ") else C.c_int if a.startswith("int ") else C.c_size_t if a.startswith("size_t ")
                    else C.c_uint64 if a.startswith("uint64_t ") and "*" not in a else None)
            assert (ct is want) if want is not None else ("*" in a and ct not in (C.c_float, C.c_int, C.c_size_t, C.c_uint64)), (name, a)
    # ssc_decode_sample_mirostat with one argument more, behind the Mirostat
    miro, arith = L.SYMBOLS["ssc_decode_sample_mirostat"][1], L.SYMBOLS["ssc_decode_sample_arith"][1]
    assert arith[:6] == miro[:6] and arith[6] is C.POINTER(L.Arith) and arith[7:] == miro[6:]
    miro, arith = L.SYMBOLS["ssc_decode_sample_mirostat_workspace_bytes"][1], L.SYMBOLS["ssc_decode_sample_arith_workspace_bytes"][1]
    assert arith == miro + [C.POINTER(L.Arith)]
    # the descriptor travels BESIDE the opts: the structs and the version are what they were
    assert struct_fields("ssc_sample_opts") == [f for f, _ in L.SampleOpts._fields_] and C.sizeof(L.SampleOpts) == 5 * C.sizeof(C.c_void_p)
    assert C.sizeof(L.Mirostat) == 40 and L.load().ssc_version() == 4
    assert "arith.hip" in open(os.path.join(ROOT, "style-seqcvae_amd", "build.py")).read()
    assert f"{R.STREAM:#x}" in header().lower()     # the header names the Philox stream the restatement uses


# ---- refusals, without a GPU ------------------------------------------------------------------------------------------------------------------
def test_rows_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    V = 50
    ok = L.SamplerDesc(0, 0, 1.0, 1.0, 3)

    def call(logits=a, ld=V, rows=3, V=V, s=ok, code_in=a, last=a, row_lp=a, end=END, pred=a, lp=a, code_out=a, mass=a):
        return lib._raw_ssc_arith_rows(logits, ld, rows, V, C.byref(s) if s is not None else None, code_in, last, row_lp, end, pred, lp,
                                       code_out, mass, None)

    assert call(rows=0) == 0 and call(rows=0, last=None, end=-7, row_lp=None, mass=None) == 0          # nothing to draw
    for kw in (dict(logits=None), dict(code_in=None), dict(pred=None), dict(lp=None), dict(code_out=None), dict(s=None), dict(ld=49),
               dict(rows=-1), dict(V=0), dict(end=-1), dict(end=50), dict(s=L.SamplerDesc(0, 0, 1.0, 0.0, 3)),
               dict(s=L.SamplerDesc(0, 0, 1.0, math.nan, 3)), dict(s=L.SamplerDesc(3, 0, 1.0, 1.0, 3)), dict(s=L.SamplerDesc(1, 0, 1.0, 1.0, 3)),
               dict(s=L.SamplerDesc(1, 51, 1.0, 1.0, 3)), dict(s=L.SamplerDesc(2, 0, 1.5, 1.0, 3))):
        assert call(**kw) == -1, kw
        if "rows" not in kw:
            assert call(rows=0, **kw) == -1, kw     # (refused with nothing to draw as well)
    for kw in (dict(code_in=a + 4), dict(code_out=a + 4), dict(code_in=a + 1), dict(mass=a + 4)):
        assert call(**kw) == -2, kw
    assert call(code_in=a + 4, V=0) == -1      # SSC_EINVAL comes first


def test_codes_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    call = lambda seed=5, nimg=2, n=3, out=a: lib._raw_ssc_arith_codes(seed, nimg, n, out, None)
    assert call(nimg=0) == 0 and call(nimg=0, seed=2 ** 64 - 1) == 0
    for kw in (dict(out=None), dict(nimg=-1), dict(n=0), dict(n=-2), dict(n=(1 << 24) + 1), dict(nimg=1 << 20, n=1 << 12)):
        assert call(**kw) == -1, kw
    assert call(out=a + 4) == -2 and call(out=a + 4, nimg=0) == -2
    assert call(out=a + 4, n=0) == -1          # SSC_EINVAL comes first


def arith(mode=1, code=None):
    return L.Arith(mode, code)


def test_decode_refuses_a_bad_descriptor_before_any_launch_and_keeps_the_workspace():
    """A descriptor that passes every check with a workspace one byte short: SSC_EWORKSPACE (-4) - it was accepted, nothing was
    launched; SSC_EINVAL / SSC_EALIGN for every bad one whatever the workspace.  The workspace is that of
    ssc_decode_sample_mirostat whatever the descriptor: the codes live in the caller's block."""
    lib = L.load()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    cfg = model_cfg()
    d = search_desc(a, beam=1, per_node=1)
    c, dd = C.byref(cfg), C.byref(d)
    miro = L.Mirostat(2.0, 0.1, 4.0, a, None, None)
    trunc = L.Truncation(2, 0.1, None, None)
    for o in (None, sample_opts(), sample_opts(trunc=trunc)):
        ob = C.byref(o) if o is not None else None
        for m in (None, miro):
            mb = C.byref(m) if m is not None else None
            n0 = lib.ssc_decode_sample_mirostat_workspace_bytes(c, dd, ob, mb)
            assert n0 > 0
            for ar in (None, arith(0), arith(1, a), arith(2, a)):
                assert lib.ssc_decode_sample_arith_workspace_bytes(c, dd, ob, mb, C.byref(ar) if ar is not None else None) == n0
    bad_opts = sample_opts(nbytes=3)
    assert lib.ssc_decode_sample_arith_workspace_bytes(c, dd, C.byref(bad_opts), None, C.byref(arith(1, a))) == 0
    n0 = lib.ssc_decode_sample_workspace_bytes(c, dd)
    p = L.Params()

    def call(ar, nbytes, smp=None, opts=None, m=None):
        smp = smp or L.SamplerDesc(0, 0, 1.0, 1.0, 3)
        return lib._raw_ssc_decode_sample_arith(c, C.byref(p), dd, C.byref(smp), C.byref(opts) if opts is not None else None,
                                                C.byref(m) if m is not None else None, C.byref(ar) if ar is not None else None, a, nbytes,
                                                None)

    # off and on: the plain call's workspace is enough (one byte less is not)
    assert call(None, n0 - 1) == -4 and call(arith(0), n0 - 1) == -4 and call(arith(0, a + 4), n0 - 1) == -4
    assert call(arith(1, a), n0 - 1) == -4 and call(arith(2, a), n0 - 1) == -4
    for ar in (arith(-1, a), arith(3, a), arith(1, None), arith(2, None)):
        assert call(ar, n0) == -1 and call(ar, n0 - 1) == -1, ar.mode
    assert call(arith(1, a + 4), n0) == -2 and call(arith(2, a + 1), n0) == -2
    assert call(arith(3, a + 4), n0) == -1      # SSC_EINVAL comes first
    # everything ssc_decode_sample_mirostat refuses stays refused
    assert call(arith(1, a), n0, smp=L.SamplerDesc(0, 0, 1.0, 0.0, 3)) == -1        # temperature 0
    assert call(arith(1, a), n0, smp=L.SamplerDesc(3, 0, 1.0, 1.0, 3)) == -1
    assert call(arith(1, a), n0, opts=bad_opts) == -1
    assert call(arith(1, a), n0, m=L.Mirostat(-1.0, 0.1, 4.0, a, None, None)) == -1
    n1 = lib.ssc_decode_sample_mirostat_workspace_bytes(c, dd, None, C.byref(miro))
    assert n1 > n0 and call(arith(1, a), n1 - 1, m=miro) == -4
    d.beam = 2
    assert call(arith(1, a), n0) == -1
    d.beam = 1
    assert CFG["V"] == 50


# ---- the runtime ------------------------------------------------------------------------------------------------------------------------------
def dims(**kw):
    base = dict(V=50, E=8, H=8, A=8, F=8, Z=4, S=0, kld_mode=0, pm_scale=0.0, prior_var=1.0)
    base.update(kw)
    return ModelDims(**base)


def test_diverse_decode_takes_an_arithmetic_with_a_word_sampler_only():
    dec = DecodeEngine(dims(), lambda: L.Params(), "cuda")
    feats = torch.zeros(2, 3, 8)
    base = dict(n_samples=3, max_steps=6, boundary_index=1, arithmetic=sampling.Arithmetic())
    for kw, name in ((dict(beam=2), "not the beam search"),
                     (dict(beam=2, sampler=sampling.GumbelSampler(1.0)), "stochastic beam search"),
                     (dict(beam=2, sampler=sampling.TopKSampler(k=5), sampled_beam=True), "sampled-node beam search"),
                     (dict(beam=2, diverse_beam=sampling.DiverseBeam(2, 0.5)), "diverse beam search"),
                     (dict(beam=2, rules=sampling.DecodeRules(2, 0, 1.0, ())), "beam search under decode rules")):
        with pytest.raises(ValueError, match="arithmetic sampling belongs to the word samplers.*" + name):
            diverse_decode(dec, feats, None, **base, **kw)
    with pytest.raises(NotImplementedError, match="arithmetic.*ensemble"):
        diverse_decode(EnsembleDecodeEngine([dec]), feats, None, beam=1, sampler=sampling.TopKSampler(k=5), **base)
    with pytest.raises(ValueError, match="arithmetic_codes needs an arithmetic"):
        dec.sample(None, None, 3, 6, 1, None, None, sampling.TopKSampler(k=5), 1, arithmetic_codes=True)


# ---- the script's refusals ----------------------------------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
BASE = ["--config", "unused.yaml", "--gpu-ids", "0", "--synthetic", "2"]


def script_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ssc_inference_script_arith", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_checks_the_arithmetic_flags():
    mod = script_module()
    args = lambda *a: mod.parser.parse_args(BASE + list(a))
    assert mod.check_arithmetic_args(args()) is None
    assert mod.check_arithmetic_args(args("--arithmetic-share-latent")) is None      # (the config may still turn it on)
    a = mod.check_arithmetic_args(args("--arithmetic"))
    assert a.lattice and not a.share_latent
    assert mod.check_arithmetic_args(args("--arithmetic", "--arithmetic-share-latent")).share_latent
    with pytest.raises(SystemExit, match="ensemble"):
        mod.check_arithmetic_args(args("--arithmetic", "--ensemble-checkpoints", "a.pth", "b.pth"))
    words = Config(config_override=TOPP).MODEL
    beam = Config().MODEL
    keyed = Config(config_override=TOPP + ["MODEL.SAMPLER_ARITHMETIC", True, "MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT", True]).MODEL
    assert mod.check_arithmetic_args(args(), words) is None
    assert mod.check_arithmetic_args(args("--arithmetic"), words).lattice
    assert mod.check_arithmetic_args(args(), keyed).share_latent
    with pytest.raises(SystemExit, match="needs a word sampler"):
        mod.check_arithmetic_args(args("--arithmetic"), beam)
    with pytest.raises(SystemExit, match="--arithmetic-share-latent needs arithmetic sampling"):
        mod.check_arithmetic_args(args("--arithmetic-share-latent"), words)
