"""Checker for the optimizer groups (afr_set_param_groups / afr_op_opt_groups / Engine.set_param_groups): the per-tensor AdamW step
in fp64, the same step by torch.optim.AdamW with real param groups, the merged range table a plan must report, and the state and
hyper-parameters the GPU tests and the CPU tests share.

Semantics (include/afr.h): tensor i is stepped with lr_i = fl32(lr * lr_mult[i]) and wd_i = fl32(wd * wd_mult[i]), two f32 products
formed on the host; everything else of the step is global.  `f32_mul` forms them the same way here."""
import functools

import numpy as np
import torch

from . import clip_ref, lion_ref
from .util import tparams

LR, WD, B1, B2, EPS = 1e-3, 0.5, 0.9, 0.99, 1e-8     # the step of the stitch test and of the comparison with torch (the issue's)
LR_MULT_ND, WD_MULT_ND = 0.5, 0.0                    # the multipliers of the default rule's tensors there; every other tensor: (1, 1)
PBAR, MBAR = 2e-5, 1e-4                              # test_gpu_clip's bounds on a step: parameters (absolute), exp_avg (of the largest
                                                     # entry); exp_avg_sq 2 x MBAR


def f32_mul(a, b):
    """fl32(a * b) of two values taken as f32, returned as the Python float that converts back to that f32 exactly."""
    return float(np.float32(a) * np.float32(b))


def two_groups(cfg):
    """(lr_mult, wd_mult) of the two-group setting: the default rule's names get (0.5, 0), the rest is left at 1."""
    from ai_font_renderer_amd.config import no_decay_names
    names = no_decay_names(cfg)
    return {k: LR_MULT_ND for k in names}, {k: WD_MULT_ND for k in names}


def tensor_hyper(name, lr_mult, wd_mult, lr=LR, wd=WD):
    """(lr_i, wd_i) of one tensor."""
    return f32_mul(lr, (lr_mult or {}).get(name, 1.0)), f32_mul(wd, (wd_mult or {}).get(name, 1.0))


def adamw_step64(p, g, m, v, t, lr, wd, b1=B1, b2=B2, eps=EPS):
    """One torch.optim.AdamW update of one tensor in fp64 (lr, wd may be tensors of p's shape: a value per element)."""
    p, g, m, v = (a.double() for a in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / np.sqrt(1.0 - b2 ** t) + eps
    return p * (1.0 - lr * wd) - (lr / (1.0 - b1 ** t)) * (m / denom), m, v


def adamw_groups_step(P, G, M, V, t, lr_mult=None, wd_mult=None, lr=LR, wd=WD, b1=B1, b2=B2, eps=EPS):
    """One grouped AdamW step over a model in fp64: every tensor with its own (lr_i, wd_i).  Returns (newP, newM, newV)."""
    nP, nM, nV = {}, {}, {}
    for k in P:
        lr_i, wd_i = tensor_hyper(k, lr_mult, wd_mult, lr, wd)
        nP[k], nM[k], nV[k] = adamw_step64(P[k], G[k], M[k], V[k], t, lr_i, wd_i, b1, b2, eps)
    return nP, nM, nV


def torch_groups_step(P, G, M, V, t, lr_mult=None, wd_mult=None, lr=LR, wd=WD, b1=B1, b2=B2, eps=EPS):
    """The same step by torch itself: torch.optim.AdamW over fp64 leaves, ONE PARAM GROUP PER TENSOR carrying that tensor's lr and
    weight_decay, seeded with the moments."""
    leaves = {k: torch.nn.Parameter(v.double().clone()) for k, v in P.items()}
    groups = []
    for k, p in leaves.items():
        lr_i, wd_i = tensor_hyper(k, lr_mult, wd_mult, lr, wd)
        groups.append(dict(params=[p], lr=lr_i, weight_decay=wd_i))
    opt = torch.optim.AdamW(groups, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for k, p in leaves.items():
        p.grad = G[k].double().clone()
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": M[k].double().clone(), "exp_avg_sq": V[k].double().clone()}
    opt.step()
    return ({k: p.detach() for k, p in leaves.items()}, {k: opt.state[p]["exp_avg"] for k, p in leaves.items()},
            {k: opt.state[p]["exp_avg_sq"] for k, p in leaves.items()})


def merged_ranges(cfg, lr_mult=None, wd_mult=None):
    """[(end offset, lr_mult, wd_mult)] a plan of cfg must report: adjacent tensors with equal multipliers merged, the padding behind a
    tensor inside its range, the last range ending at the buffer's size."""
    from ai_font_renderer_amd.config import flat_layout
    table, total = flat_layout(cfg)
    out = []
    for i, (name, _, _, _) in enumerate(table):
        end = table[i + 1][2] if i + 1 < len(table) else total
        lm, wm = float(np.float32((lr_mult or {}).get(name, 1.0))), float(np.float32((wd_mult or {}).get(name, 1.0)))
        if out and out[-1][1:] == (lm, wm):
            out[-1] = (end, lm, wm)
        else:
            out.append((end, lm, wm))
    return out


def seeded_state(G, seed=77):
    """A non-zero optimizer state to step from: exp_avg = lion_ref.seeded_moment (randn x rms(g), an eighth exactly zero) and a
    POSITIVE exp_avg_sq = rms(g)^2 x uniform(0.5, 1.5) per tensor (1e-6 where the gradient is all zero)."""
    M = lion_ref.seeded_moment(G, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    V = {}
    for k, g in G.items():
        ms = float(g.double().pow(2).mean()) or 1e-6
        V[k] = ((0.5 + torch.rand(g.shape, generator=gen)) * ms).float()
    return M, V


@functools.lru_cache(maxsize=None)
def reference(name):
    """One grouped AdamW step (t = 1) of a fixture in f32 mode on the CPU oracle, from the seeded state, with the two groups of the
    stitch test: dict with P, G, M, V (the start), lr_mult, wd_mult and new_p, new_m, new_v (fp64).  Computed once."""
    cfg, x, font, t = lion_ref.case(name)
    P = tparams(cfg)
    _, G = clip_ref.forward_backward(P, x, t.float() / 255.0, cfg, font=font)
    M, V = seeded_state(G)
    lm, wm = two_groups(cfg)
    nP, nM, nV = adamw_groups_step(P, G, M, V, 1, lm, wm)
    return dict(cfg=cfg, P=P, G=G, M=M, V=V, lr_mult=lm, wd_mult=wm, new_p=nP, new_m=nM, new_v=nV)
