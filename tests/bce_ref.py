"""Checker for the BCE loss kind (AFR_LOSS_BCE): the explicit formula of F.binary_cross_entropy_with_logits on the logits u
of a sigmoid head, the twin of oracle.mse_loss_grad.  The oracle's sheet_backward / glyph_backward / pixel_backward take du
and expose cache["u"], so a BCE step of the oracle is forward -> bce_logits_loss_grad(cache["u"], t) -> backward."""
import torch

from oracle import afr_oracle as oracle


def sigmoid_stable(u):
    """sigmoid(u) in the stable form the kernels use: e = exp(-|u|); u >= 0 ? 1/(1+e) : e/(1+e)."""
    e = torch.exp(-u.abs())
    return torch.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_logits_loss_grad(u, target, total_elems=None):
    """loss = sum(max(u,0) - t*u + log1p(exp(-|u|))) / n and du = (sigmoid(u) - t) / n, n = total_elems or u.numel()
    (the mean's denominator, overridable as in oracle.mse_loss_grad).  Soft targets t in [0, 1].  Returns (loss, du [B, pixels])."""
    u2 = u.reshape(u.shape[0], -1)
    t2 = target.reshape(u2.shape).to(u2.dtype)
    n = float(total_elems if total_elems is not None else u2.numel())
    e = torch.exp(-u2.abs())
    loss = (u2.clamp(min=0.0) - t2 * u2 + torch.log1p(e)).sum() / n
    du = (sigmoid_stable(u2) - t2) / n
    return loss, du


def train_step(P, M, V, t, x, target, cfg, font=None, masks=None, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=5e-4):
    """oracle.train_step with the BCE loss: zero_grad -> forward -> BCE-with-logits -> backward -> AdamW.
    Returns (loss, grads, newP, newM, newV)."""
    if cfg.kind == "sheet":
        _, cache = oracle.sheet_forward(P, x, cfg, masks)
        bwd = oracle.sheet_backward
    elif cfg.kind == "pixel":
        _, cache = oracle.pixel_forward(P, x, font, cfg)
        bwd = oracle.pixel_backward
    else:
        _, cache = oracle.glyph_forward(P, x, font, cfg)
        bwd = oracle.glyph_backward
    loss, du = bce_logits_loss_grad(cache["u"], target)
    G = bwd(P, cache, du, cfg)
    nP, nM, nV = {}, {}, {}
    for k in P:
        nP[k], nM[k], nV[k] = oracle.adamw_step(P[k], G[k], M[k], V[k], t, lr, beta1, beta2, eps, wd)
    return loss, G, nP, nM, nV
