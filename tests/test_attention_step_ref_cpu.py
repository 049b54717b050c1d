"""CPU: the float64 attention-step reference of the op tests (attnstepref) is itself checked - against the oracle's attention,
against finite differences of its own forward, and on a fully masked image."""
import torch

import attnstepref as ref
import oracle
from oracle.seqcvae_oracle import P_BUTD


def _toy(rpi=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    G, R, A, F, D = 4, 5, 6, 3, 4
    nimg = G // rpi
    mask = torch.ones(nimg, R, dtype=torch.float64)
    mask[0, R - 2:] = 0.0
    mask[-1, 1] = 0.0
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t = {"q": r(G, A), "pv": r(nimg, R, A) * mask[:, :, None], "wa": 0.3 * r(A), "mask": mask,
         "feats": r(nimg, R, F) * mask[:, :, None], "obj": r(nimg, R, D) * mask[:, :, None],
         "datt": r(G, F), "dpool_a": r(G, 2), "dpool_b": r(G, D)}
    return t


def test_forward_equals_the_oracle_attention():
    """butd_attention with an identity query projection (q = h1), the weighted sums as cell_step forms them; 1e-12 in float64"""
    t = _toy()
    A = t["q"].size(1)
    params = {P_BUTD + "_query_vector_projection_layer.weight": torch.eye(A, dtype=torch.float64),
              P_BUTD + "_image_features_projection_layer.weight": torch.zeros(A, t["feats"].size(2), dtype=torch.float64),
              P_BUTD + "_attention_layer.weight": t["wa"][None, :]}
    alpha, _ = oracle.butd_attention(params, t["q"], t["feats"], t["mask"] > 0, t["pv"])
    out = ref.forward(t["q"], t["pv"], t["wa"], t["mask"], t["feats"], t["obj"])
    assert alpha.dtype == torch.float64
    assert (out["alpha"] - alpha).abs().max().item() <= 1e-12
    assert (out["att"] - torch.sum(alpha.unsqueeze(-1) * t["feats"], dim=1)).abs().max().item() <= 1e-12
    assert (out["pool"] - torch.sum(alpha.unsqueeze(-1) * t["obj"], dim=1)).abs().max().item() <= 1e-12
    assert float(out["alpha"][0, -2:].abs().max()) == 0.0 and float(out["alpha"][-1, 1]) == 0.0
    assert (out["alpha"].sum(1) - 1).abs().max().item() <= 1e-12


def _central(f, x, h=1e-6):
    """central finite difference of the scalar f at the tensor x, entry by entry"""
    d = torch.zeros_like(x)
    flat, dflat = x.view(-1), d.view(-1)
    for i in range(flat.numel()):
        keep = flat[i].item()
        flat[i] = keep + h
        up = f().item()
        flat[i] = keep - h
        dn = f().item()
        flat[i] = keep
        dflat[i] = (up - dn) / (2 * h)
    return d


def test_autograd_backward_equals_finite_differences():
    """every returned gradient against a central difference (h = 1e-6: truncation ~1e-12, rounding ~1e-10) to 1e-6; rows sharing
    an image (rpi = 2) included, where dpv sums over the rows of an image"""
    for rpi in (1, 2):
        t = _toy(rpi, seed=rpi)
        q, pv, mask, feats, obj = t["q"], t["pv"], t["mask"], t["feats"], t["obj"]
        G = q.size(0)
        dpool = ref.pool_grad(obj.size(2), t["dpool_a"], t["dpool_b"])
        got = ref.backward(q, pv, t["wa"], mask, feats, t["datt"], obj, t["dpool_a"], t["dpool_b"], rpi=rpi)
        wa_rows = t["wa"].expand(G, -1).clone()

        def from_alpha(alpha):
            return ref.objective(ref.pooled(alpha, feats, rpi), ref.pooled(alpha, obj, rpi), t["datt"], dpool)

        def loss():
            return from_alpha(ref.alpha_of(ref.logits_of(q, pv, wa_rows, rpi), mask, rpi))

        assert (got["dq"] - _central(loss, q)).abs().max().item() <= 1e-6
        assert (got["dpv"] - _central(loss, pv)).abs().max().item() <= 1e-6
        fd_rows = _central(loss, wa_rows)
        assert (got["dwa_rows"] - fd_rows).abs().max().item() <= 1e-6
        assert (got["dwa"] - fd_rows.sum(0)).abs().max().item() <= 1e-6
        logits, alpha = got["logits"].clone(), got["alpha"].clone()
        assert (got["dlogit"] - _central(lambda: from_alpha(ref.alpha_of(logits, mask, rpi)), logits)).abs().max().item() <= 1e-6
        assert (got["dalpha"] - _central(lambda: from_alpha(alpha), alpha)).abs().max().item() <= 1e-6
        assert got["dq"].abs().max().item() > 1e-3 and got["dwa"].abs().max().item() > 1e-3      # (not vacuous)


def test_fully_masked_image_gives_zero_weights_and_zero_finite_gradients():
    t = _toy()
    t["mask"][1] = 0.0
    for k in ("pv", "feats", "obj"):
        t[k][1] = 0.0
    got = ref.backward(t["q"], t["pv"], t["wa"], t["mask"], t["feats"], t["datt"], t["obj"], t["dpool_a"], t["dpool_b"])
    assert float(got["alpha"][1].abs().max()) == 0.0
    for k in ("dq", "dpv", "dwa_rows", "dlogit", "dalpha"):
        assert torch.isfinite(got[k]).all(), k
        assert float(got[k][1].abs().max()) == 0.0, k
    assert torch.isfinite(got["dwa"]).all() and got["dq"][0].abs().max().item() > 0
