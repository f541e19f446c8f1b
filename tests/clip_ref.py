"""Checker for global gradient-norm clipping (afr_set_grad_clip): torch.nn.utils.clip_grad_norm_'s formula made explicit on
the CPU oracle.  A clipped step of the oracle is forward -> loss -> backward -> norm and coefficient in f32 -> oracle.adamw_step
on g * coef (the engine keeps the coefficient inside the update and leaves the gradient buffer unscaled; the update is the same)."""
import numpy as np
import torch

from oracle import afr_oracle as oracle


def grad_sumsq(G):
    """Sum of squares over the ELEMENTS of the gradient tensors (no flat-buffer padding), accumulated in fp64."""
    return float(sum(float((g.double() ** 2).sum()) for g in G.values()))


def clip_coef(sumsq, max_norm, grad_scale=1.0):
    """(total_norm, coef) as f32: total_norm = |grad_scale| * sqrt(sumsq); coef = min(1, max_norm / (total_norm + 1e-6))."""
    total = np.float32(abs(grad_scale)) * np.sqrt(np.float32(sumsq))
    coef = min(np.float32(1.0), np.float32(max_norm) / (total + np.float32(1e-6)))
    return float(total), float(np.float32(coef))


def forward_backward(P, x, target, cfg, font=None, masks=None, total_elems=None, rnd=None):
    """(loss, grads) of one oracle step without the optimizer; target as floats in [0, 1]."""
    if cfg.kind == "sheet":
        _, cache = oracle.sheet_forward(P, x, cfg, masks, rnd=rnd)
        loss, du = oracle.mse_loss_grad(cache["u"], target, total_elems=total_elems)
        return loss, oracle.sheet_backward(P, cache, du, cfg, rnd=rnd)
    if cfg.kind == "pixel":
        _, cache = oracle.pixel_forward(P, x, font, cfg)
        loss, du = oracle.mse_loss_grad(cache["u"], target, total_elems=total_elems)
        return loss, oracle.pixel_backward(P, cache, du, cfg)
    _, cache = oracle.glyph_forward(P, x, font, cfg, rnd=rnd)
    loss, du = oracle.mse_loss_grad(cache["u"], target, total_elems=total_elems)
    return loss, oracle.glyph_backward(P, cache, du, cfg, rnd=rnd)


def clipped_train_step(P, M, V, t, x, target, cfg, max_norm, font=None, masks=None, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8,
                       wd=5e-4):
    """oracle.train_step with clip_grad_norm_(parameters, max_norm) between backward and the optimizer.
    Returns (loss, grads (unscaled), newP, newM, newV, total_norm, coef)."""
    loss, G = forward_backward(P, x, target, cfg, font=font, masks=masks)
    total, coef = clip_coef(grad_sumsq(G), max_norm)
    nP, nM, nV = {}, {}, {}
    for k in P:
        nP[k], nM[k], nV[k] = oracle.adamw_step(P[k], G[k] * coef, M[k], V[k], t, lr, beta1, beta2, eps, wd)
    return loss, G, nP, nM, nV, total, coef


def torch_clipped_step(P, G, M, V, t, max_norm, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=5e-4):
    """The same update by torch itself: clip_grad_norm_ on leaf tensors carrying G, then torch.optim.AdamW seeded with the moments
    (test_clip_cpu.py holds clipped_train_step's arithmetic to it).  Returns (newP, newM, newV, total_norm)."""
    leaves = {k: torch.nn.Parameter(v.clone()) for k, v in P.items()}
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd)
    for k, p in leaves.items():
        p.grad = G[k].clone()
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": M[k].clone(), "exp_avg_sq": V[k].clone()}
    total = torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_norm)
    opt.step()
    return ({k: p.detach() for k, p in leaves.items()}, {k: opt.state[p]["exp_avg"] for k, p in leaves.items()},
            {k: opt.state[p]["exp_avg_sq"] for k, p in leaves.items()}, float(total))
