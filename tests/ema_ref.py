"""Checker for the weight EMA (afr_set_ema / afr_op_ema / Engine.set_ema): the update in fp64 with the f32 alpha the library forms,
its closed form for constant parameters, and the per-element bound the GPU tests hold the kernel to."""
import numpy as np
import torch


def alpha32(decay):
    """alpha = 1.0f - decay as the host forms it: both operands and the difference in f32."""
    return float(np.float32(1.0) - np.float32(decay))


def ema_step(e, p, decay):
    """e + (p - e) * alpha in fp64, alpha the f32 value."""
    e, p = e.double(), p.double()
    return e + (p - e) * alpha32(decay)


def closed_form(e0, p, decay, k):
    """k applications of ema_step with a constant p: p + (e0 - p) (1 - alpha)^k."""
    e0, p = e0.double(), p.double()
    return p + (e0 - p) * (1.0 - alpha32(decay)) ** k


def bound(p, e_old):
    """Per element: one rounding of p - e (<= 2^-24 * 2 * max) scaled by alpha <= 1, plus one rounding of the fma result
    (<= 2^-24 * max): 3 * 2^-24 * max(|p|, |e_old|), held to 2^-22 * max (slack below 2x)."""
    return 2.0 ** -22 * torch.maximum(p.abs(), e_old.abs()).double()


def mixed(n, seed):
    """(p, e, same): random values of mixed magnitudes (1e-4 .. 1e+2); every eighth element (same) has p == e exactly."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 10.0 ** torch.randint(-4, 3, (n,), generator=gen).float()
    e = torch.randn(n, generator=gen) * 10.0 ** torch.randint(-4, 3, (n,), generator=gen).float()
    same = torch.arange(n) % 8 == 3
    e[same] = p[same]
    return p, e, same
