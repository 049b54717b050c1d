"""CPU: KL annealing and free bits - the schedule (ssc_runtime/schedule.py), the OPTIM.KL_ANNEAL* / OPTIM.FREE_BITS* config keys, the
float64 reference of the GPU tests (tests/freebitsref.py) against autograd and the oracle, and the C ABI of ssc_latent_fwd_fb /
ssc_latent_bwd_fb / ssc_latent_fb_finish and the ssc_train_*_opts calls that carry the option beside the cfg: exported, mirrored in ctypes, and refusing bad
arguments before anything touches memory (no GPU here)."""
import ctypes as C
import os
import re

import pytest
import torch

import freebitsref as fr
import oracle
from ssc_runtime import lib as L
from ssc_runtime.config import Config
from ssc_runtime.schedule import kl_beta, kl_beta_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- schedule ---------------------------------------------------------------------------------------------------------------
def test_schedule_none_and_linear():
    assert kl_beta(0, "none") == 1.0 and kl_beta(12345, "none", 7, 0.3, 0.2) == 1.0
    assert kl_beta(0, "linear", 100) == 0.0
    assert kl_beta(50, "linear", 100) == 0.5
    assert kl_beta(100, "linear", 100) == 1.0 and kl_beta(5000, "linear", 100) == 1.0
    assert kl_beta(1, "linear", 1) == 1.0 and kl_beta(0, "linear", 1) == 0.0


def test_schedule_cyclical():
    got = [kl_beta(it, "cyclical", 100, 0.5) for it in (0, 25, 50, 99, 100)]
    assert got == [0.0, 0.5, 1.0, 1.0, 0.0]
    assert kl_beta(125, "cyclical", 100, 0.5) == 0.5 and kl_beta(10, "cyclical", 100, 1.0) == pytest.approx(0.1, abs=1e-15)


def test_schedule_start_above_zero():
    assert kl_beta(0, "linear", 100, start=0.2) == pytest.approx(0.2, abs=1e-15)
    assert kl_beta(50, "linear", 100, start=0.2) == pytest.approx(0.6, abs=1e-15)
    assert kl_beta(100, "linear", 100, start=0.2) == 1.0
    assert kl_beta(200, "cyclical", 100, 0.5, 0.2) == pytest.approx(0.2, abs=1e-15)
    assert kl_beta(225, "cyclical", 100, 0.5, 0.2) == pytest.approx(0.6, abs=1e-15)
    assert kl_beta(7, "linear", 100, start=1.0) == 1.0


def test_schedule_is_a_pure_function_of_the_iteration():
    want = {it: kl_beta(it, "cyclical", 10, 0.5, 0.1) for it in range(40)}
    for it in (39, 3, 17, 3, 0, 25, 39):                           # any history: the same iteration, the same beta
        assert kl_beta(it, "cyclical", 10, 0.5, 0.1) == want[it]
    assert [want[it] for it in range(10)] == [want[it + 20] for it in range(10)]
    for bad in (dict(kind="cosine"), dict(kind="linear", iteration=-1), dict(kind="linear", iters=0), dict(kind="cyclical", ratio=0.0),
                dict(kind="cyclical", ratio=1.5), dict(kind="linear", start=-0.1), dict(kind="linear", start=1.1)):
        args = dict(iteration=1, kind="linear", iters=10, ratio=0.5, start=0.0)
        args.update(bad)
        with pytest.raises(ValueError, match="kl_beta"):
            kl_beta(**args)


# ---- config -----------------------------------------------------------------------------------------------------------------
def test_config_keys_defaults_overrides_and_refusals():
    o = Config().OPTIM
    assert (o.KL_ANNEAL, o.KL_ANNEAL_RATIO, o.KL_ANNEAL_START, o.FREE_BITS, o.FREE_BITS_MODE) == ("none", 0.5, 0.0, 0.0, "dim")
    assert isinstance(o.KL_ANNEAL_ITERS, int) and o.KL_ANNEAL_ITERS >= 1
    assert kl_beta_from_config(o, 3) == 1.0
    c = Config(config_override=["OPTIM.KL_ANNEAL", "cyclical", "OPTIM.KL_ANNEAL_ITERS", "100", "OPTIM.KL_ANNEAL_RATIO", "0.25",
                                "OPTIM.KL_ANNEAL_START", "0.5", "OPTIM.FREE_BITS", "0.05", "OPTIM.FREE_BITS_MODE", "element"]).OPTIM
    assert (c.KL_ANNEAL, c.KL_ANNEAL_ITERS, c.KL_ANNEAL_RATIO, c.KL_ANNEAL_START, c.FREE_BITS, c.FREE_BITS_MODE) == \
        ("cyclical", 100, 0.25, 0.5, 0.05, "element")
    assert kl_beta_from_config(c, 110) == pytest.approx(0.5 + 0.5 * 0.4, abs=1e-15)
    assert Config(config_override=["OPTIM.FREE_BITS", 2]).OPTIM.FREE_BITS == 2.0
    assert Config(config_override=["OPTIM.KL_ANNEAL_RATIO", 1]).OPTIM.KL_ANNEAL_RATIO == 1.0
    for key, bads in {"OPTIM.KL_ANNEAL": ["cosine", "Linear"], "OPTIM.KL_ANNEAL_ITERS": ["0", "-3"],
                      "OPTIM.KL_ANNEAL_RATIO": ["0", "0.0", "1.5", "-0.5"], "OPTIM.KL_ANNEAL_START": ["-0.1", "1.01"],
                      "OPTIM.FREE_BITS": ["-0.5", float("inf"), float("nan")], "OPTIM.FREE_BITS_MODE": ["dims", "batch"]}.items():
        for bad in bads:
            with pytest.raises(ValueError, match=key):
                Config(config_override=[key, bad])
    # the reference's annealing keys stay accepted: nothing reads them
    assert Config(config_override=["MODEL.DO_USE_KLD_ANNEALING", True, "MODEL.KLD_INITIAL_WEIGHT", 3.0]).MODEL.DO_USE_KLD_ANNEALING is True


def test_captioner_takes_the_values_and_the_engine_checks_them():
    from ssc_runtime.engine import check_free_bits
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    over = ["MODEL.IMAGE_FEATURE_SIZE", 16, "MODEL.EMBEDDING_SIZE", 8, "MODEL.HIDDEN_SIZE", 8, "MODEL.ATTENTION_PROJECTION_SIZE", 8,
            "MODEL.Z_SPACE", 4, "MODEL.USE_CBS", False, "MODEL.MIN_CONSTRAINTS_TO_SATISFY", 0, "DATA.CBS.MAX_GIVEN_CONSTRAINTS", 0]
    voc = Vocabulary.synthetic(20)
    m = UpDownCaptioner.from_config(Config(config_override=over + ["OPTIM.FREE_BITS", 0.1, "OPTIM.FREE_BITS_MODE", "step"]),
                                    vocabulary=voc, device=None)
    assert (m.free_bits, m.free_bits_mode) == (0.1, "step")
    m = UpDownCaptioner.from_config(Config(config_override=over), vocabulary=voc, device=None)
    assert (m.free_bits, m.free_bits_mode) == (0.0, "dim")
    with pytest.raises(ValueError, match="free_bits"):
        UpDownCaptioner(voc, 16, 8, 8, 8, z_space=4, free_bits=-1.0)
    with pytest.raises(ValueError, match="free_bits_mode"):
        UpDownCaptioner(voc, 16, 8, 8, 8, z_space=4, free_bits_mode="row")
    assert check_free_bits(0.5, "step") == (0.5, 2) and check_free_bits(0, "element") == (0.0, 1) and check_free_bits(2.0) == (2.0, 3)
    with pytest.raises(ValueError, match="free_bits_mode"):
        check_free_bits(0.0, "rows")
    for bad in (-0.1, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match="free_bits"):
            check_free_bits(bad)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_structs_follow_the_header_and_the_option_travels_beside_the_cfg():
    """ssc_model_cfg keeps its layout (tests/test_label_smoothing_cpu.py pins its last field and the workspace views): the floor
    is a field pair of ssc_train_opts, the one descriptor of ssc_train_fwd_opts / ssc_train_bwd_opts, and its buffers have a view
    of their own."""
    text = open(os.path.join(ROOT, "include", "ssc.h")).read()
    body = text[text.index("typedef struct {\n  int V, E, H, A, F, Z;"):text.index("} ssc_model_cfg;")]
    names = [n.strip() for line in re.findall(r"(?:int|float)\s+([\w, ]+);", body) for n in line.split(",")]
    assert names == [f for f, _ in L.ModelCfg._fields_] and "free_bits" not in names
    body = text[text.index("typedef struct {\n  float lambda; int mode;"):text.index("} ssc_free_bits;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:float\*?|int)\s+(\w+);", body)
    assert names == [f.rstrip("_") for f, _ in L.FreeBits._fields_]
    lib = L.load()
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    assert lib.ssc_train_workspace_bytes(C.byref(cfg), 2, 3, 4) > 0
    ld = C.c_int(0)
    buf = (C.c_float * 16)()
    for which, want_ld in ((0, 2), (1, 4), (2, 2), (3, 4)):
        assert lib.ssc_train_free_bits_view(C.byref(cfg), 2, 3, 4, C.addressof(buf), which, C.byref(ld)) and ld.value == want_ld
    assert not lib.ssc_train_free_bits_view(C.byref(cfg), 2, 3, 4, C.addressof(buf), 4, C.byref(ld))
    assert not lib.ssc_train_free_bits_view(C.byref(cfg), 2, 3, 4, C.addressof(buf), -1, C.byref(ld))
    assert not lib.ssc_train_free_bits_view(C.byref(cfg), 0, 3, 4, C.addressof(buf), 0, C.byref(ld))
    cdll = C.CDLL(L.LIB_PATH)
    for name in ("ssc_latent_fwd_fb", "ssc_latent_bwd_fb", "ssc_latent_fb_finish", "ssc_train_fwd_opts", "ssc_train_bwd_opts",
                 "ssc_train_free_bits_view"):
        assert hasattr(cdll, name) and name in L.SYMBOLS
    # the descriptor: the header's fields in the header's order, 24 bytes; the two entries take what their SYMBOLS rows say
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = flat[:flat.index("} ssc_train_opts;")]
    body = body[body.rindex("typedef struct {"):]
    names = re.findall(r"(?:float|int|const ssc_sched_sampling\*|const ssc_distill\*)\s+(\w+);", body)
    assert names == [f for f, _ in L.TrainOpts._fields_] == ["free_bits", "free_bits_mode", "sched", "distill"]
    assert C.sizeof(L.TrainOpts) == 24 and L.TrainOpts.sched.offset == 8 and L.TrainOpts.distill.offset == 16
    for name in ("ssc_train_fwd_opts", "ssc_train_bwd_opts"):
        decl = flat[flat.index("int " + name + "("):]
        assert decl[:decl.index(");")].count(",") + 1 == len(L.SYMBOLS[name][1]), name
    assert len(L.SYMBOLS["ssc_train_fwd_opts"][1]) == len(L.SYMBOLS["ssc_train_fwd"][1]) + 1          # the plain call + opts
    assert len(L.SYMBOLS["ssc_train_bwd_opts"][1]) == len(L.SYMBOLS["ssc_train_bwd_phases"][1]) + 1
    # the entries that carried one option each are gone: not declared, not exported, not bound
    for name in ("ssc_train_fwd_fb", "ssc_train_fwd_ss", "ssc_train_fwd_kd", "ssc_train_bwd_fb", "ssc_train_bwd_ss", "ssc_train_bwd_kd",
                 "ssc_train_bwd_phases_fb", "ssc_train_bwd_phases_ss", "ssc_train_bwd_phases_kd"):
        assert name not in text and not hasattr(cdll, name) and name not in L.SYMBOLS, name
    assert lib.ssc_version() == 4


def _descs(a):
    """Forward and backward descriptors whose every pointer is the host buffer `a`: a call that got past its checks would fail on
    the launch (no GPU), not return -1."""
    f = L.LatentFwdDesc()
    f.B, f.Z, f.ldmulv, f.nslab, f.slab_stride, f.ldeps, f.ldz, f.prior_var = 2, 4, 8, 1, 0, 4, 4, 1.0
    for n in ("mulv", "bmu", "blv", "eps", "w", "mu", "lv", "z", "kld_acc"):
        setattr(f, n, a)
    b = L.LatentBwdDesc()
    b.B, b.Z, b.lddz, b.ldeps, b.ldz, b.lddmulv, b.nslab, b.prior_var = 2, 4, 4, 4, 4, 8, 1, 1.0
    for n in ("dz", "eps", "mu", "lv", "w", "gk", "dmulv"):
        setattr(b, n, a)
    return f, b


def _fb(a, lam=0.1, mode=3, **kw):
    fb = L.FreeBits()
    fb.lambda_, fb.mode, fb.kld_raw, fb.gate_step, fb.dim_acc, fb.lddim, fb.gate_dim = lam, mode, a, a, a, 4, a
    for k, v in kw.items():
        setattr(fb, k, v)
    return fb


def test_kernel_entries_refuse_bad_arguments_before_anything_is_launched():
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    f, b = _descs(a)
    fwd = lambda fb: lib._raw_ssc_latent_fwd_fb(C.byref(f), C.byref(fb) if fb is not None else None, None)
    bwd = lambda fb: lib._raw_ssc_latent_bwd_fb(C.byref(b), C.byref(fb) if fb is not None else None, None)
    for call in (fwd, bwd):
        assert call(None) == -1
        for lam in (-0.1, float("nan"), float("inf"), -float("inf")):
            for mode in (1, 2, 3):
                assert call(_fb(a, lam, mode)) == -1, (lam, mode)
        for mode in (0, 4, -1):
            assert call(_fb(a, 0.1, mode)) == -1, mode
        assert call(_fb(a, mode=2, gate_step=None)) == -1
    assert fwd(_fb(a, mode=1, kld_raw=None)) == -1 and fwd(_fb(a, mode=3, kld_raw=None)) == -1
    assert fwd(_fb(a, mode=3, dim_acc=None)) == -1 and fwd(_fb(a, mode=3, lddim=3)) == -1
    assert bwd(_fb(a, mode=3, gate_dim=None)) == -1
    # what the plain entries refuse is refused here too, with the floor on or off
    for lam in (0.0, 0.1):
        f2, b2 = _descs(a)
        f2.mu = None
        b2.gk = None
        assert lib._raw_ssc_latent_fwd_fb(C.byref(f2), C.byref(_fb(a, lam)), None) == -1
        assert lib._raw_ssc_latent_bwd_fb(C.byref(b2), C.byref(_fb(a, lam)), None) == -1
    fin = lambda acc=a, ld=4, B=2, Z=4, lam=0.1, kdim=a, gate=a, kld=a: lib._raw_ssc_latent_fb_finish(acc, ld, B, Z, lam, kdim, gate, kld, None)
    assert fin(acc=None) == -1 and fin(kdim=None) == -1 and fin(gate=None) == -1 and fin(kld=None) == -1
    assert fin(ld=3) == -1 and fin(B=0) == -1 and fin(Z=0) == -1 and fin(lam=-1.0) == -1 and fin(lam=float("nan")) == -1
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_latent_fwd_fb(C.byref(f), C.byref(_fb(a, 0.1, 0)), None)


def test_train_forward_refuses_a_bad_floor():
    """Everything but the floor is in order and the workspace is too small: a cfg that passes its checks ends at SSC_EWORKSPACE
    (before any launch), a bad floor at SSC_EINVAL."""
    lib = L.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    p = L.Params()
    for name, typ in L.Params._fields_:
        setattr(p, name, 4 if typ is C.c_int else a)
    bt = L.Batch(2, 3, 4, a, a, a, a, None)

    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)

    def fwd(free_bits, mode):
        return lib._raw_ssc_train_fwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(L.TrainOpts(free_bits, mode)), None)

    def bwd(free_bits, mode, phases=15):
        return lib._raw_ssc_train_bwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), phases,
                                           C.byref(L.TrainOpts(free_bits, mode)), None)

    for call in (fwd, bwd, lambda x, m: bwd(x, m, 32)):
        assert call(0.0, 0) == -4 and call(0.0, 7) == -4                         # off: the mode is not read
        for mode in (1, 2, 3):
            assert call(0.1, mode) == -4
        for mode in (0, 4):
            assert call(0.1, mode) == -1
        for lam in (-0.1, float("nan"), float("inf")):
            assert call(lam, 3) == -1
    # the plain entries are the same calls without a floor, as is a NULL descriptor
    assert lib._raw_ssc_train_fwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, None, None) == -4
    assert lib._raw_ssc_train_bwd_opts(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), 15, None, None) == -4
    assert lib._raw_ssc_train_fwd(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, None) == -4
    assert lib._raw_ssc_train_bwd(C.byref(cfg), C.byref(p), C.byref(bt), a, 16, a, a, C.byref(p), None) == -4


# ---- the reference ----------------------------------------------------------------------------------------------------------
def _latents(kld_mode, seed=0):
    g = torch.Generator().manual_seed(seed)
    T, B, Z = 4, 3, 5
    mean = torch.randn(T, B, Z, generator=g, dtype=torch.float64)
    log_var = torch.randn(T, B, Z, generator=g, dtype=torch.float64) * 0.5
    pm = torch.randn(T, B, Z, generator=g, dtype=torch.float64) * 0.3
    w = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 1.0]], dtype=torch.float64)
    gk = torch.tensor([0.7, -1.3, 0.25], dtype=torch.float64)
    return mean, log_var, pm, 0.8, w, gk


@pytest.mark.parametrize("kld_mode", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_reference_closed_form_gradients_equal_autograd(mode, kld_mode):
    mean, log_var, pm, pv, w, gk = _latents(kld_mode, 10 * mode + kld_mode)
    k = fr.k_elem(mean, log_var, pm, pv, kld_mode)
    lam, half = fr.pick_lambda(fr.compared(k, w, mode))
    assert half > 0
    leaves = [t.clone().requires_grad_(True) for t in (mean, log_var, pm)]
    kld, gate, K = fr.floored(fr.k_elem(*leaves, pv, kld_mode), w, lam, mode)
    assert bool(gate.any()) and not bool(gate.all())
    (gk * kld).sum().backward()
    want = fr.dlatent(mean, log_var, pm, pv, kld_mode, w, gk, gate)
    for leaf, ref in zip(leaves, want):
        got = leaf.grad if leaf.grad is not None else torch.zeros_like(ref)
        assert (got - ref).abs().max().item() <= 1e-12
    closed = ~fr.gate_full(gate, mean.shape)
    assert all(bool((ref[closed] == 0).all()) for ref in want)
    # the value: every term at or below the floor counts as the floor, strictly
    full = fr.gate_full(gate, mean.shape)
    if mode == 1:
        manual = (w * torch.where(full, k, torch.tensor(lam, dtype=torch.float64)).sum(-1)).sum(0)
        assert (kld.detach() - manual).abs().max().item() <= 1e-12
    # a term AT the floor is closed: elements of 0.25, step sums of Z * 0.25 = 1.25, dimension means of T * 0.25 = 1
    _, g2, _ = fr.floored(torch.full_like(k, 0.25), torch.ones_like(w), {1: 0.25, 2: 1.25, 3: 1.0}[mode], mode)
    assert not bool(g2.any())


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_reference_dim_mean_identity_and_zero_floor(mode):
    mean, log_var, pm, pv, w, gk = _latents(1, 3)
    k = fr.k_elem(mean, log_var, pm, pv, 1)
    lam, _ = fr.pick_lambda(fr.compared(k, w, 3))
    kld, gate, K = fr.floored(k, w, lam, 3)
    want = torch.where(K > lam, K, torch.tensor(lam, dtype=torch.float64)).sum()
    assert abs(float(kld.mean() - want)) <= 1e-12                               # mean_b kld_b = sum_j max(lam, K_j)
    # no floor: the raw KL in every mode (a KL element of these inputs is positive)
    assert bool((k > 0).all())
    assert (fr.floored(k, w, 0.0, mode)[0] - fr.raw(k, w)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("sv", [0, 1])
def test_reference_without_a_floor_is_the_oracle_kld(sv):
    cfg = oracle.OracleConfig(vocab_size=30, image_feature_size=12, embedding_size=8, hidden_size=10, attention_projection_size=6,
                              z_space=5, max_caption_length=4, sentiment_vae=sv, senti_prior_multip=0.5, prior_std=0.9)
    params = oracle.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(4)
    B, R, L_ = 3, 4, 4
    feats = torch.randn(B, R, 12, generator=g)
    caps = torch.tensor([[5, 6, 7, 0], [8, 9, 0, 0], [3, 4, 5, 6]])
    senti = torch.tensor([[1.0], [-1.0], [0.0]])
    eps = torch.randn(L_ + 1, B, 5, generator=g)
    out = oracle.train_forward(params, cfg, feats, caps, senti, eps, return_steps=True)
    stack = lambda key: torch.stack([s[key] for s in out["steps"]], 0)
    w = (out["tokens"][:, 1:] != cfg.pad_index).t().double()
    k = fr.k_elem(stack("mean"), stack("log_var"), stack("prior_mean"), cfg.prior_std ** 2, 0 if sv == 0 else 1)
    assert (fr.raw(k, w) - out["kld"].double()).abs().max().item() <= 1e-5 * max(1.0, float(out["kld"].abs().max()))
    for mode in (1, 2, 3):
        assert (fr.floored(k, w, 0.0, mode)[0] - out["kld"].double()).abs().max().item() <= 1e-5 * max(1.0, float(out["kld"].abs().max()))
