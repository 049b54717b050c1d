"""GPU: fused T-step forward + BPTT (ssc_train_fwd / ssc_train_bwd through the C ABI) against
(a) the committed golden vectors produced by the reference itself and (b) the CPU oracle on seeded
inputs at medium size.  Tolerance (BASELINE.json north_star): 1e-4 abs, fp32."""
import pytest
import torch

import oracle
from goldenlib import group, load
from gpuutil import dev, engine_from, maxdiff

pytestmark = pytest.mark.gpu

TRAIN = ["g1_train_sv1", "g2_train_sv0", "g3_train_tied", "g4_train_prior", "g4b_train_simple", "g7_train_odd", "g8_train_unk", "g8b_train_unk_sv0",
         "g14_train_sv2"]   # g14: SENTIMENT_VAE = 2 through the fused sequence kernels, vs the reference UpDownCell under autograd
TOL = 1e-4


def _loss_weights(cfg, caps):
    """w[b, t] = 1 iff the target of step t (token t+1 of the boundary-augmented caption) is not padding
    (updown_captioner.py:265-278): with an in-caption @@UNKNOWN@@ (id 0) this is NOT a prefix mask."""
    tok, _ = oracle.add_sentence_boundary_token_ids(caps, caps != cfg.pad_index, cfg.boundary_index, cfg.boundary_index)
    return tok[:, 1:] != cfg.pad_index


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", TRAIN)
def test_train_matches_reference_golden(name, mode):
    """mode 1 = default kernels (3xBF16, device-side row compaction), mode 0 = exact-fp32 MFMA kernels over all rows."""
    if mode == 0 and "unk" not in name and name not in ("g1_train_sv1", "g14_train_sv2"):
        pytest.skip("exact-fp32 mode: the UNK fixtures and one plain fixture")
    from ssc_runtime import lib as L
    lib = L.load()
    lib.ssc_set_gemm_mode(mode)
    try:
        _check_train_golden(name)
    finally:
        lib.ssc_set_gemm_mode(1)


def _check_train_golden(name):
    d, cfgd = load(name)
    cfg = oracle.OracleConfig(**cfgd)
    params = group(d, "param/")
    ins = group(d, "in/")
    eng = engine_from(cfg, params)
    obj = dev(ins["obj_atts"]) if "obj_atts" in ins else None
    loss, kld = eng.forward(dev(ins["feats"]), dev(ins["caps"]), dev(ins["sentiment"]) if "sentiment" in ins else None, dev(ins["eps"]),
                            obj)
    exp = group(d, "out/")
    assert maxdiff(loss, exp["loss"]) < TOL
    assert maxdiff(kld, exp["kld"]) < TOL
    T = ins["eps"].shape[0]
    names = {0: "h1", 1: "c1", 2: "h_encoder", 3: "c_encoder", 4: "h_decoder", 5: "c_decoder"}
    for t in (0, 1, T - 1):
        st = group(d, f"step{t}/")
        for which, key in names.items():
            assert maxdiff(eng.workspace_view(which)[t + 1], st[key]) < TOL, (t, key)
        assert maxdiff(eng.workspace_view(6)[t], st["alpha"]) < TOL
        assert maxdiff(eng.workspace_view(7)[t], st["mean"]) < TOL
        assert maxdiff(eng.workspace_view(8)[t], st["log_var"]) < TOL
        # logits exist only for rows with a real target (rows with loss weight 0 are skipped on the device; the reference
        # computes and then masks them)
        act = _loss_weights(cfg, ins["caps"])[:, t]
        if bool(act.any()) and "logits" in st:
            assert maxdiff(eng.workspace_view(9)[t][act.cuda()], st["logits"][act]) < TOL
    B = loss.numel()
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * 750.0), device="cuda")
    eng.backward(gl, gk)
    got = eng.grad_dict()
    grads = group(d, "grad/")
    for k, g in grads.items():
        if k == "_output_layer.weight" and cfg.tied:
            continue
        assert maxdiff(got[k], g) < TOL, k
        scale = g.abs().max().item()
        assert maxdiff(got[k], g) <= 1e-4 * max(scale, 1e-3) + 2e-6, (k, scale)


def test_train_sv2_matches_oracle_medium():
    """SENTIMENT_VAE = 2 at widths where the gate products run on the 3xBF16 MFMA kernels (F + 2H + 150 and the 150-wide c-block
    are no multiples of 4: padded K-segment / padded dx columns), zero-padded regions, objects without attributes."""
    dims = dict(V=600, E=128, H=192, A=96, F=256, Z=150, L=6)
    B, R = 24, 9
    cfg = oracle.OracleConfig(vocab_size=dims["V"], image_feature_size=dims["F"], embedding_size=dims["E"],
                              hidden_size=dims["H"], attention_projection_size=dims["A"], z_space=dims["Z"],
                              max_caption_length=dims["L"], sentiment_vae=2, prior_std=0.8)
    params = oracle.init_params(cfg, seed=6)
    g = torch.Generator().manual_seed(23)
    L, T = dims["L"], dims["L"] + 1
    feats = torch.randn(B, R, dims["F"], generator=g)
    feats[0, R - 3:] = 0
    obj = torch.randn(B, R, 150, generator=g) * 0.5
    obj[0, R - 3:] = 0
    obj[3, 2] = 0
    caps = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(3, L + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(2, dims["V"], (n,), generator=g)
    caps[1, 1] = 0   # in-caption @@UNKNOWN@@
    eps = torch.randn(T, B, dims["Z"], generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = oracle.train_forward(p, cfg, feats, caps, None, eps, obj_atts=obj)
    oracle.train_objective(out, cfg).backward()
    eng = engine_from(cfg, params)
    loss, kld = eng.forward(dev(feats), dev(caps), None, dev(eps), dev(obj))
    assert maxdiff(loss, out["loss"]) <= 1e-5 * float(out["loss"].detach().abs().max()) + 1e-4
    assert maxdiff(kld, out["kld"]) <= 1e-5 * float(out["kld"].detach().abs().max()) + 1e-4
    eng.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * cfg.kld_weight), device="cuda"))
    got = eng.grad_dict()
    for k, v in p.items():
        scale = v.grad.abs().max().item()
        assert maxdiff(got[k], v.grad) <= 1e-4 * max(scale, 1e-3) + 2e-6, (k, scale, maxdiff(got[k], v.grad))


@pytest.mark.parametrize("sv,B,R,dims", [
    (1, 8, 36, dict(V=1000, E=200, H=256, A=128, F=512, Z=64, L=12)),
    (0, 5, 10, dict(V=777, E=100, H=130, A=70, F=260, Z=30, L=9)),
    # minibatches of 128-511 rows take 128x128 tiles (grouped launches of the wave-specialised form) for every gate product
    (1, 128, 12, dict(V=900, E=192, H=320, A=160, F=512, Z=64, L=7)),
    (1, 200, 6, dict(V=600, E=128, H=256, A=128, F=256, Z=32, L=5)),
    # the shipped config.yaml's shape class: BATCH_SIZE 150, Z_SPACE 150 (no multiple of 4: the z-block products run on padded rows)
    (1, 150, 8, dict(V=500, E=96, H=192, A=96, F=256, Z=30, L=5)),
    # vocabulary sizes that are no multiple of 4 (the backward head products run on V & ~3 entries + a tail kernel): untied above
    # (V = 777), tied head (E = 300: frozen table, Linear + Tanh projection) here, and a large untied one
    (1, 6, 7, dict(V=451, E=300, H=64, A=48, F=128, Z=16, L=6)),
    (1, 64, 6, dict(V=2003, E=128, H=256, A=128, F=256, Z=32, L=5)),
    # FULL width (C2's model: what the kernel-form and split-K decisions of the launchers see in production), short captions to
    # keep the CPU oracle at seconds: minibatches on either side of the 64-row and 128-row tile boundaries and the yaml's 150
    (1, 65, 36, dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=3)),
    (1, 130, 36, dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=3)),
    (0, 150, 36, dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=3)),
    (1, 33, 36, dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=4)),
    (1, 1, 36, dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=4)),
    (0, 2, 9, dict(V=10000, E=1000, H=1200, A=768, F=2048, Z=128, L=3)),
    # BASELINE configs[4] (C5) at FULL width: B = 128 per GPU, 100 regions, V = 30000 (captions cut to 3 tokens for the CPU oracle)
    (1, 128, 100, dict(V=30000, E=1000, H=1200, A=768, F=2048, Z=128, L=3)),
])
def test_train_matches_oracle_medium(sv, B, R, dims):
    cfg = oracle.OracleConfig(vocab_size=dims["V"], image_feature_size=dims["F"], embedding_size=dims["E"],
                              hidden_size=dims["H"], attention_projection_size=dims["A"], z_space=dims["Z"],
                              max_caption_length=dims["L"], sentiment_vae=sv, senti_prior_multip=0.5)
    params = oracle.init_params(cfg, seed=5)
    g = torch.Generator().manual_seed(17)
    L, T = dims["L"], dims["L"] + 1
    feats = torch.randn(B, R, dims["F"], generator=g)
    feats[0, R - 3:] = 0
    caps = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(3, L + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(2, dims["V"], (n,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(T, B, dims["Z"], generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = oracle.train_forward(p, cfg, feats, caps, senti, eps)
    oracle.train_objective(out, cfg).backward()
    eng = engine_from(cfg, params)
    loss, kld = eng.forward(dev(feats), dev(caps), dev(senti), dev(eps))
    # north_star tolerance as the full-size tests state it: 1e-4 absolute + 1e-5 relative (losses here are O(80): one fp32 ulp is 8e-6)
    assert maxdiff(loss, out["loss"]) <= 1e-4 + 1e-5 * float(out["loss"].detach().abs().max())
    assert maxdiff(kld, out["kld"]) <= 1e-4 + 1e-5 * float(out["kld"].detach().abs().max())
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * cfg.kld_weight), device="cuda")
    eng.backward(gl, gk)
    got = eng.grad_dict()
    for k, v in p.items():
        assert maxdiff(got[k], v.grad) < TOL, k


def test_stress_shape_c5_like_regions_and_length():
    """BASELINE configs[4] geometry (R=100 regions, L=40 -> T=41, B=128) at reduced widths: parity vs the oracle."""
    cfg = oracle.OracleConfig(vocab_size=1500, image_feature_size=256, embedding_size=96, hidden_size=128,
                              attention_projection_size=64, z_space=32, max_caption_length=40, sentiment_vae=1,
                              senti_prior_multip=0.5)
    params = oracle.init_params(cfg, seed=9)
    g = torch.Generator().manual_seed(23)
    B, R, L = 128, 100, 40
    feats = torch.randn(B, R, 256, generator=g)
    feats[3, 60:] = 0
    caps = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(5, L + 1, (1,), generator=g))
        caps[b, :n] = torch.randint(2, 1500, (n,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(L + 1, B, 32, generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = oracle.train_forward(p, cfg, feats, caps, senti, eps)
    oracle.train_objective(out, cfg).backward()
    eng = engine_from(cfg, params)
    loss, kld = eng.forward(dev(feats), dev(caps), dev(senti), dev(eps))
    assert maxdiff(loss, out["loss"]) <= 1e-4 + 1e-5 * float(out["loss"].detach().abs().max())   # loss ~ O(250)
    assert maxdiff(kld, out["kld"]) <= 1e-4 + 1e-5 * float(out["kld"].detach().abs().max())
    eng.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * cfg.kld_weight), device="cuda"))
    got = eng.grad_dict()
    for k, v in p.items():
        assert maxdiff(got[k], v.grad) < TOL, k


# ---- BASELINE configs[1] (C2) at FULL size: properties that need no CPU oracle run ------------------------------------
def _c2_engine_and_batch(seed=1234):
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    V, F, E, H, A, Z, L, B, R = 10000, 2048, 1000, 1200, 768, 128, 20, 64, 36
    torch.manual_seed(2)
    model = UpDownCaptioner(Vocabulary.synthetic(V), image_feature_size=F, embedding_size=E, hidden_size=H,
                            attention_projection_size=A, max_caption_length=L, beam_size=5, z_space=Z, prior_std=1.0,
                            simple_vae=False, latent_embedding="glove", sentiment_vae=1, senti_prior_multip=0.5,
                            device=torch.device("cuda")).to("cuda")
    eng = model._engine()
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, R, F, generator=g)
    lens = torch.randint(8, L + 1, (B,), generator=g)
    caps = torch.zeros(B, L, dtype=torch.long)
    ids = torch.randint(2, V, (B, L), generator=g)
    for b in range(B):
        caps[b, : lens[b]] = ids[b, : lens[b]]
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(L + 1, B, Z, generator=g)
    return eng, (feats.cuda(), caps.cuda(), senti.cuda(), eps.cuda()), lens


def _step(eng, batch):
    B = batch[0].shape[0]
    loss, kld = eng.forward(*batch)
    eng.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * 750.0), device="cuda"))
    return loss.clone(), kld.clone(), {k: v.clone() for k, v in eng.grad_dict().items()}


def test_full_size_c2_two_independent_kernel_paths_agree():
    """C2 at full size (B=64, 36x2048 regions, T=21, V=10k, E/H/A=1000/1200/768).  The default path (3xBF16 kernels, padded
    rows skipped on the device, grouped launches) against the exact-fp32-MFMA mode, which shares none of those kernels and
    computes every padded row: losses and every gradient agree to fp32 level; and the default path is deterministic."""
    from ssc_runtime import lib as L
    eng, batch, _ = _c2_engine_and_batch()
    lib = L.load()
    l1, k1, g1 = _step(eng, batch)
    l1b, k1b, g1b = _step(eng, batch)
    assert torch.equal(l1, l1b) and torch.equal(k1, k1b)
    for k in g1:   # fixed summation orders everywhere: bit-identical reruns - except the embedding gradient, whose rows are
        if k == "_embedding_layer.weight":        # scatter-added with float atomics (the path's only atomics)
            assert maxdiff(g1[k], g1b[k]) <= 1e-6 * max(g1[k].abs().max().item(), 1e-6), k
        else:
            assert torch.equal(g1[k], g1b[k]), k
    lib.ssc_set_gemm_mode(0)
    try:
        l0, k0, g0 = _step(eng, batch)
    finally:
        lib.ssc_set_gemm_mode(1)
    assert maxdiff(l1, l0) < 2e-3 and maxdiff(k1, k0) < 2e-3          # loss ~ O(150)
    for k in g1:
        scale = max(g0[k].abs().max().item(), 1e-6)
        assert maxdiff(g1[k], g0[k]) <= 2e-4 * scale + 1e-7, (k, maxdiff(g1[k], g0[k]), scale)


def test_full_size_c2_batch_permutation_and_padding_invariance():
    """Permuting the minibatch permutes loss / kld and leaves the weight gradients unchanged (to summation order); token
    ids written behind a caption's padding boundary are never read."""
    eng, batch, lens = _c2_engine_and_batch(seed=77)
    feats, caps, senti, eps = batch
    l1, k1, g1 = _step(eng, batch)
    perm = torch.randperm(feats.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    l2, k2, g2 = _step(eng, (feats[perm].contiguous(), caps[perm].contiguous(), senti[perm].contiguous(), eps[:, perm].contiguous()))
    assert maxdiff(l2, l1[perm]) <= 1e-4 + 1e-5 * float(l1.abs().max()) and maxdiff(k2, k1[perm]) <= 1e-4 + 1e-5 * float(k1.abs().max())
    for k in g1:
        scale = max(g1[k].abs().max().item(), 1e-6)
        assert maxdiff(g1[k], g2[k]) <= 2e-4 * scale + 1e-7, k
    # eps rows of padded steps: change the noise wherever the step is padding -> nothing may change
    eps2 = eps.clone()
    T = eps.shape[0]
    for b in range(feats.shape[0]):
        eps2[int(lens[b]) + 1:, b] = 7.0
    l3, k3, g3 = _step(eng, (feats, caps, senti, eps2))
    assert torch.equal(l3, l1) and torch.equal(k3, k1)
    for k in g1:
        assert torch.equal(g1[k], g3[k]), k


# ---- full-size parity pinned to the REFERENCE (fixtures g10: outputs only; parameters and inputs are regenerated from seeds) ------
def _full_size_inputs(seed, B, R=36, F=2048, L=20, V=10000, Z=128, unk=False):
    """Same generator as tests/golden/make_golden.py::full_size_inputs."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, R, F, generator=g)
    lens = torch.randint(8, L + 1, (B,), generator=g)
    ids = torch.randint(2, V, (B, L), generator=g)
    caps = torch.where(torch.arange(L).unsqueeze(0) < lens.unsqueeze(1), ids, torch.zeros_like(ids))
    if unk:
        for b in range(0, B, 3):
            caps[b, int(lens[b]) // 2] = 0
    senti = torch.randint(-1, 2, (B, 1), generator=g).float()
    eps = torch.randn(L + 1, B, Z, generator=g)
    return feats, caps, senti, eps


def _full_size_model():
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    V, F, E, H, A, Z, L = 10000, 2048, 1000, 1200, 768, 128, 20
    torch.manual_seed(2)
    return UpDownCaptioner(Vocabulary.synthetic(V), image_feature_size=F, embedding_size=E, hidden_size=H,
                           attention_projection_size=A, max_caption_length=L, beam_size=5, z_space=Z, prior_std=1.0,
                           simple_vae=False, latent_embedding="glove", sentiment_vae=1, senti_prior_multip=0.5,
                           device=torch.device("cuda")).to("cuda")


@pytest.mark.parametrize("name", ["g10_full_c1", "g10_full_c2"])
def test_full_size_matches_reference_fixture(name):
    """BASELINE configs[0] (B=4) and configs[1] (B=64, with in-caption @@UNKNOWN@@) at FULL size against the reference's own
    forward / backward (fixture written by tests/golden/make_golden.py from the imported reference): the mirror's seeded
    init equals the reference's (per-tensor checksums), loss and kld per caption, and every gradient through its norm, sum
    and 64 sampled entries.  Tolerances: loss / kld 1e-5 relative + 1e-4; gradients 1e-4 of the tensor's largest entry."""
    import numpy as np
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    B = int(z["B"])
    m = _full_size_model()
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    for k in [f for f in z.files if f.startswith("psum/")]:
        w = sd[k[5:]]
        assert abs(float(w.sum()) - z[k][0]) <= 1e-9 * max(1.0, abs(z[k][0])) and abs(float(w.abs().sum()) - z[k][1]) <= 1e-9 * z[k][1], k
    eng = m._engine()
    feats, caps, senti, eps = _full_size_inputs(int(z["seed"]), B, unk=bool(int(z["unk"])))
    loss, kld = eng.forward(feats.cuda(), caps.cuda(), senti.cuda(), eps.cuda())
    for got, want in ((loss, z["out/loss"]), (kld, z["out/kld"])):
        want = torch.from_numpy(want)
        assert ((got.cpu() - want).abs() <= 1e-5 * want.abs() + 1e-4).all(), (got.cpu() - want).abs().max()
    eng.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * 750.0), device="cuda"))
    grads = eng.grad_dict()
    checked = 0
    for k in [f for f in z.files if f.startswith("gnorm/")]:
        n = k[6:]
        g = grads[n].reshape(-1).double().cpu()
        norm, gsum, gmax = z[k]
        tol = 1e-4 * gmax + 1e-9
        stride = max(1, g.numel() // 32)
        assert (g[:32] - torch.from_numpy(z["ghead/" + n]).double()).abs().max() <= tol, n
        assert (g[::stride][:32] - torch.from_numpy(z["gstride/" + n]).double()).abs().max() <= tol, n
        assert abs(float(g.norm()) - norm) <= 1e-4 * norm + 1e-9, (n, float(g.norm()), norm)
        checked += 1
    assert checked == len(grads)


def test_full_size_c2_matches_oracle_every_gradient():
    """C2 at full size, captions with in-caption @@UNKNOWN@@: ONE oracle train step on this box's host cores (a few seconds)
    against the default HIP path: loss, kld and EVERY gradient entry, 1e-4 of the tensor's scale."""
    m = _full_size_model()
    eng = m._engine()
    B = 64
    feats, caps, senti, eps = _full_size_inputs(777, B, unk=True)
    cfg = oracle.OracleConfig(vocab_size=10000, image_feature_size=2048, embedding_size=1000, hidden_size=1200,
                              attention_projection_size=768, z_space=128, max_caption_length=20, sentiment_vae=1,
                              senti_prior_multip=0.5)
    prev = torch.get_num_threads()
    torch.set_num_threads(min(16, prev))       # the default (every core of the box) is oversubscribed for this step
    try:
        p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        out = oracle.train_forward(p, cfg, feats, caps, senti, eps)
        oracle.train_objective(out, cfg).backward()
    finally:
        torch.set_num_threads(prev)
    loss, kld = eng.forward(feats.cuda(), caps.cuda(), senti.cuda(), eps.cuda())
    assert ((loss.cpu() - out["loss"]).abs() <= 1e-5 * out["loss"].abs() + 1e-4).all()
    assert ((kld.cpu() - out["kld"]).abs() <= 1e-5 * out["kld"].abs() + 1e-4).all()
    eng.backward(torch.full((B,), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / (B * cfg.kld_weight), device="cuda"))
    got = eng.grad_dict()
    for k, v in p.items():
        scale = max(v.grad.abs().max().item(), 1e-6)
        assert maxdiff(got[k], v.grad) <= 1e-4 * scale + 1e-7, (k, maxdiff(got[k], v.grad), scale)


def test_full_size_c5_properties():
    """BASELINE configs[4] (stress) at FULL width on one GPU: B=128, R=100 regions, L=40 (T=41), V=30000, E/H/A=1000/1200/768.
    No CPU run at this size: the default path against the exact-fp32-MFMA mode (independent GEMM kernels, every row
    computed), bit-identical reruns, and invariance to what lies behind the padding."""
    from ssc_runtime import lib as L
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    V, F, E, H, A, Z, Lc, B, R = 30000, 2048, 1000, 1200, 768, 128, 40, 128, 100
    torch.manual_seed(2)
    m = UpDownCaptioner(Vocabulary.synthetic(V), image_feature_size=F, embedding_size=E, hidden_size=H,
                        attention_projection_size=A, max_caption_length=Lc, beam_size=5, z_space=Z, prior_std=1.0,
                        simple_vae=False, latent_embedding="glove", sentiment_vae=1, senti_prior_multip=0.5,
                        device=torch.device("cuda")).to("cuda")
    eng = m._engine()
    feats, caps, senti, eps = _full_size_inputs(99, B, R=R, L=Lc, V=V, unk=True)
    feats[5, 70:] = 0                      # one image with 70 regions (zero-padded: adaptive features)
    batch = (feats.cuda(), caps.cuda(), senti.cuda(), eps.cuda())
    l1, k1, g1 = _step(eng, batch)
    l2, k2, g2 = _step(eng, batch)
    assert torch.equal(l1, l2) and torch.equal(k1, k2)
    lib = L.load()
    lib.ssc_set_gemm_mode(0)
    try:
        l0, k0, g0 = _step(eng, batch)
    finally:
        lib.ssc_set_gemm_mode(1)
    assert ((l1 - l0).abs() <= 1e-5 * l0.abs().max() + 1e-4).all() and ((k1 - k0).abs() <= 1e-5 * k0.abs().max() + 1e-4).all()
    for k in g1:
        scale = max(g0[k].abs().max().item(), 1e-6)
        assert maxdiff(g1[k], g0[k]) <= 2e-4 * scale + 1e-7, (k, maxdiff(g1[k], g0[k]), scale)
    assert float(eng.workspace_view(6)[:, 5, 70:].abs().max()) == 0.0      # no attention weight on the padded regions


def test_edge_cases_match_oracle():
    """Empty caption (only the boundary pair), full-length caption, caption that is ALL @@UNKNOWN@@, an image whose regions are
    all zero (mask all 0: alpha = 0, averaged features 0 - allennlp masked_softmax / masked_mean clamps), an image with one
    region, against the oracle; and a batch of one."""
    cfg = oracle.OracleConfig(vocab_size=60, image_feature_size=36, embedding_size=20, hidden_size=28,
                              attention_projection_size=12, z_space=8, max_caption_length=5, sentiment_vae=1,
                              senti_prior_multip=0.5)
    params = oracle.init_params(cfg, seed=19)
    g = torch.Generator().manual_seed(2)
    B, R, L = 6, 4, 5
    feats = torch.randn(B, R, 36, generator=g)
    feats[1] = 0                    # no region at all
    feats[2, 1:] = 0                # a single region
    caps = torch.zeros(B, L, dtype=torch.long)
    caps[1] = torch.randint(2, 60, (L,), generator=g)         # full length
    caps[2, :3] = torch.tensor([5, 0, 7])                     # UNK in the middle
    caps[3, :2] = 0                                           # "two unknown words" = indistinguishable from empty
    caps[4, :1] = 9
    caps[5] = torch.tensor([3, 4, 0, 0, 8])                   # UNK run, then a word
    senti = torch.tensor([[1.0], [0.0], [-1.0], [1.0], [0.0], [-1.0]])
    eps = torch.randn(L + 1, B, 8, generator=g)
    for rows in (slice(0, B), slice(2, 3)):                   # the whole batch, then a batch of one
        f, c, s_, e = feats[rows], caps[rows], senti[rows], eps[:, rows].contiguous()
        p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        out = oracle.train_forward(p, cfg, f, c, s_, e)
        oracle.train_objective(out, cfg).backward()
        eng = engine_from(cfg, params)
        loss, kld = eng.forward(dev(f), dev(c), dev(s_), dev(e))
        n = f.size(0)
        assert maxdiff(loss, out["loss"]) < TOL and maxdiff(kld, out["kld"]) < TOL
        eng.backward(torch.full((n,), 1.0 / n, device="cuda"), torch.full((n,), 1.0 / (n * cfg.kld_weight), device="cuda"))
        got = eng.grad_dict()
        for k, v in p.items():
            assert maxdiff(got[k], v.grad) < TOL, k
        assert torch.isfinite(loss).all() and all(torch.isfinite(x).all() for x in got.values())


@pytest.mark.parametrize("masks", [(16, 32, 8, 4, 2), (16, 32, 2, 4, 8), (1, 4, 2, 8), (16, 32, 4 | 8, 2), (15,),
                                   (16, 32, 64, 8, 4, 128), (16, 32, 128, 4, 64, 8)])   # 2 = 64 (embedding) + 128 (attention LSTM)
def test_phased_backward_equals_the_one_call_backward(masks):
    """ssc_train_bwd_phases (include/ssc.h): the vocabulary head (16) and the BPTT loop (32) first, then the three weight-gradient
    phases in ANY order - what lets the data-parallel engine reduce a finished gradient range under the phases that follow
    (engine.phase_ranges) - give the gradients of ssc_train_bwd BIT FOR BIT, at widths where every product takes its production
    kernel (wave-specialised gate products, grouped weight gradients), the embedding gradient included."""
    from gpuutil import engine_from
    cfg = oracle.OracleConfig(vocab_size=1200, image_feature_size=512, embedding_size=256, hidden_size=320,
                              attention_projection_size=192, z_space=64, max_caption_length=9, sentiment_vae=1,
                              senti_prior_multip=0.5)
    eng = engine_from(cfg, oracle.init_params(cfg, seed=11))
    g = torch.Generator().manual_seed(5)
    B, R, L = 64, 12, 9
    feats = torch.randn(B, R, 512, generator=g).cuda()
    caps = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = 2 + b % 8
        caps[b, :n] = torch.randint(2, 1200, (n,), generator=g)
    senti = torch.randint(-1, 2, (B, 1), generator=g).float().cuda()
    eps = torch.randn(L + 1, B, 64, generator=g).cuda()
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * 750.0), device="cuda")
    eng.forward(feats, caps.cuda(), senti, eps)
    eng.grads.flat.fill_(float("nan"))
    eng.backward(gl, gk)
    torch.cuda.synchronize()
    want = {n: v.clone() for n, v in eng.grads.views.items()}
    assert all(torch.isfinite(v).all() for v in want.values())
    eng.forward(feats, caps.cuda(), senti, eps)     # (the backward consumes the forward's workspace: logits become dlogits in place)
    eng.grads.flat.fill_(float("nan"))
    eng.backward_phased(gl, gk, masks)
    torch.cuda.synchronize()
    bad = {n: (v - want[n]).abs().max().item() for n, v in eng.grads.views.items() if not torch.equal(v, want[n])}
    assert not bad, bad


def test_opts_entries_are_the_plain_calls_when_off_and_compose_the_options():
    """ssc_train_fwd_opts / ssc_train_bwd_opts (include/ssc.h: ssc_train_opts) through the ctypes table, on an engine's own
    parameter, gradient and workspace buffers.  Options off - a NULL descriptor, a zeroed one, one whose every option is present
    but off - is ssc_train_fwd / ssc_train_bwd BIT FOR BIT.  Options on together (label smoothing in the cfg, a free-bits floor
    and distillation in the descriptor): the one-call backward (phases 15) and the phased one leave the same bits."""
    import ctypes as C
    from ssc_runtime import lib as L
    lib = L.load()
    cfg = oracle.OracleConfig(vocab_size=60, image_feature_size=36, embedding_size=20, hidden_size=28,
                              attention_projection_size=12, z_space=8, max_caption_length=4, sentiment_vae=1,
                              senti_prior_multip=0.5)
    eng = engine_from(cfg, oracle.init_params(cfg, seed=23))
    gen = torch.Generator().manual_seed(8)
    B, R, Lc, V = 3, 5, 4, 60
    T = Lc + 1
    feats = dev(torch.randn(B, R, 36, generator=gen))
    caps = torch.zeros(B, Lc, dtype=torch.long)
    caps[0] = torch.randint(2, V, (Lc,), generator=gen)            # fills L
    caps[1, :2] = torch.randint(2, V, (2,), generator=gen)         # a padded tail
    caps[2, :3] = torch.randint(2, V, (3,), generator=gen)
    caps = dev(caps)
    senti = dev(torch.tensor([[1.0], [0.0], [-1.0]]))
    eps = dev(torch.randn(T, B, 8, generator=gen))
    gl = torch.full((B,), 1.0 / B, device="cuda")
    gk = torch.full((B,), 1.0 / (B * 750.0), device="cuda")
    bt, keep = eng._batch(feats, caps, senti, eps)
    ws = eng._workspace(B, R, Lc)
    p, g = eng.params.c_struct(), eng.grads.c_struct()
    head = (C.byref(eng._cfg), C.byref(p), C.byref(bt), L.ptr(ws), ws.numel() * 4)

    def run(fwd, bwds):
        """One forward, then the backward as the given calls -> (loss, kld, every gradient)."""
        loss, kld = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        fwd(L.ptr(loss), L.ptr(kld))
        eng.grads.flat.fill_(float("nan"))
        for bwd in bwds:
            bwd()
        torch.cuda.synchronize()
        got = {n: v.clone() for n, v in eng.grads.views.items()}
        assert torch.isfinite(loss).all() and torch.isfinite(kld).all() and all(torch.isfinite(v).all() for v in got.values())
        return loss, kld, got

    def via_opts(opts, masks=(15,)):
        ref = C.byref(opts) if opts is not None else None
        return run(lambda lo, kl: lib.ssc_train_fwd_opts(*head, lo, kl, ref, L.stream_ptr()),
                   [lambda m=m: lib.ssc_train_bwd_opts(*head, L.ptr(gl), L.ptr(gk), C.byref(g), m, ref, L.stream_ptr()) for m in masks])

    def same(a, b, what):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what
        bad = [n for n in a[2] if not torch.equal(a[2][n], b[2][n])]
        assert not bad, (what, bad)

    # ---- options off is the plain call
    plain = run(lambda lo, kl: lib.ssc_train_fwd(*head, lo, kl, L.stream_ptr()),
                [lambda: lib.ssc_train_bwd(*head, L.ptr(gl), L.ptr(gk), C.byref(g), L.stream_ptr())])
    sched_off = L.SchedSampling(0.0, L.SamplerDesc(0, 0, 1.0, 1.0, 7))
    distill_off = L.Distill(None, 0, 0.0, 1.0, None, None)
    same(plain, via_opts(None), "opts NULL")
    same(plain, via_opts(L.TrainOpts()), "opts zeroed")
    same(plain, via_opts(L.TrainOpts(0.0, 3, C.pointer(sched_off), C.pointer(distill_off))), "every option present and off")

    # ---- options compose through the one entry: smoothing + free bits + distillation, one call against the phases
    eng._cfg.label_smoothing = 0.1
    teacher = torch.randn(T * B, V, generator=gen).cuda()           # held outside the workspace
    rows, kd_b = torch.zeros(3 * T * B, device="cuda"), torch.zeros(B, device="cuda")
    distill = L.Distill(teacher.data_ptr(), V, 0.5, 2.0, rows.data_ptr(), kd_b.data_ptr())
    opts = L.TrainOpts(0.05, 3, None, C.pointer(distill))
    one = via_opts(opts)
    assert not torch.equal(one[0], plain[0])                        # (the options did change the step)
    same(one, via_opts(opts, (16, 32, 2, 4, 8)), "phases 16, 32, 2, 4, 8")


@pytest.mark.parametrize("n,E", [(1344, 1000), (700, 37), (5, 300), (9000, 40)])
def test_embedding_scatter_sums_each_token_in_position_order(n, E):
    """ssc_embed_scatter_add (the embedding gradient of the train step) is deterministic: a token's rows are summed in ascending
    position order and each sum over 4096 positions from its first one is added to the table row in turn, so the result equals
    those float32 sums bit for bit, on every call.  Tokens repeat within and across 64-position mask words and 4096-position
    chunks; padding positions add nothing."""
    from ssc_runtime import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(n + E)
    V, pad = 60, 0
    ids = torch.randint(0, V, (n,), generator=g)
    ids[n // 2:] = torch.where(ids[n // 2:] % 3 == 0, torch.full_like(ids[n // 2:], 7), ids[n // 2:])
    d = torch.randn(n, E + 3, generator=g)
    table0 = torch.randn(V, E + 5, generator=g)
    want = table0.clone()
    first, sums = {}, {}
    for j in range(n):
        t = int(ids[j])
        if t != pad:
            key = (t, (j - first.setdefault(t, j)) // 4096)
            sums[key] = d[j, :E].clone() if key not in sums else sums[key] + d[j, :E]
    for (t, _), s in sorted(sums.items()):
        want[t, :E] = want[t, :E] + s
    ids_d, d_d = ids.cuda(), d.cuda()
    for _ in range(2):
        got = table0.cuda()
        lib.ssc_embed_scatter_add(L.ptr(got), got.stride(0), L.ptr(ids_d), n, E, L.ptr(d_d), d_d.stride(0), pad, L.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want)
