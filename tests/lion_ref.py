"""Checker for the Lion optimizer kind (afr_set_optimizer / afr_op_lion): the paper's update in fp64, one Lion training step on the
CPU oracle, and the element-by-element comparison the GPU tests and the CPU test share.

Lion's sign makes the update discontinuous: where the reference's c = b1 m + (1 - b1) g is within rounding of zero the engine may
legitimately take the other sign.  Nothing hides behind that: `compare` looks at EVERY element -- the moment everywhere, a decided
parameter (|c_ref| > tau) against the reference, an undecided one against the three legal outcomes p_old decay + {-lr, 0, +lr} --
and returns the number of undecided elements, which the callers hold under CAP of the model."""
import functools
from dataclasses import replace

import numpy as np
import torch

from oracle import afr_oracle as oracle

from . import clip_ref
from .util import MINI, GlyphConfig, engine_rounding, glyph_inputs, load, rnd_du, synth, tparams

LR, WD, B1, B2 = 1e-4, 5e-3, 0.9, 0.99        # the Lion step of the tests (test 6 of the issue: lr = 1e-4, wd = 5e-3)
CAP = 0.02                                     # undecided elements over all tensor elements of a model: a condition, not a measurement
NODROP = replace(MINI, p_embed=0.0, p_attn=0.0, p_fc=0.0)
SMALL = GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2)
# sheet-deep: 37 strings.  The sheet front end's backward leaves one partial slab per string up to 256 (afr_sheet_blocks(B) = min(B, 256)),
# and the grouped reduce takes its `deep` branch from 32 slabs on: B = 37 is past it and no multiple of anything
BF16_MOMENT_ONLY = ("glyph-small", "glyph-c1", "sheet-mini", "sheet-deep")                          # bf16 fixtures whose undecided share at the bf16 bound exceeds CAP (test_lion_cpu.py holds the list true)
CASES = ("glyph-small", "glyph-c1", "sheet-mini", "sheet-deep", "c5-mini")


def lion_step(p, g, m, lr, b1, b2, wd):
    """One Lion update in fp64.  Returns (new_p, new_m, c): c is the interpolation whose sign is taken."""
    p, g, m = p.double(), g.double(), m.double()
    c = b1 * m + (1.0 - b1) * g
    return p * (1.0 - lr * wd) - lr * torch.sign(c), b2 * m + (1.0 - b2) * g, c


def case(name):
    """(cfg, x, font, target u8) of a fixture's inputs."""
    from ai_font_renderer_amd.config import C5_MINI, WORKLOADS
    if name == "c5-mini":
        fx = load("pixel_twin.npz")
        return C5_MINI, torch.from_numpy(fx["x"]), torch.from_numpy(fx["font"]), torch.from_numpy(fx["target_u8"])
    if name == "sheet-mini":
        fx = load("sheet_mini.npz")
        return NODROP, torch.from_numpy(fx["x10"]), None, torch.from_numpy(fx["target_u8"])
    if name == "sheet-deep":
        x = synth.encode_strings(synth.dataset_strings(37), NODROP.max_length)
        return NODROP, torch.from_numpy(x), None, torch.from_numpy(synth.synth_sheet_targets(37, NODROP.sheet_h, NODROP.sheet_w, tensor_id=931))
    cfg, B = (SMALL, 300) if name == "glyph-small" else (WORKLOADS["c1"]["cfg"], 95)
    x, font, t = glyph_inputs(cfg, B)
    return cfg, torch.from_numpy(x), torch.from_numpy(font) if cfg.n_fonts else None, torch.from_numpy(t)


def forward_backward(P, x, target, cfg, font=None, rnd=None, train_step=True):
    """(loss, grads) of one oracle step.  rnd None: clip_ref.forward_backward (plain f32).  With the bf16 engine's rounding sites
    (util.engine_rounding) du is rounded too, as the loss epilogue stores it."""
    if rnd is None:
        return clip_ref.forward_backward(P, x, target, cfg, font=font)
    if cfg.kind == "sheet":
        _, cache = oracle.sheet_forward(P, x, cfg, None, rnd=rnd)
        loss, du = oracle.mse_loss_grad(cache["u"], target)
        return loss, oracle.sheet_backward(P, cache, rnd_du(rnd, du), cfg, rnd=rnd)
    _, cache = oracle.glyph_forward(P, x, font, cfg, rnd=rnd)
    loss, du = oracle.mse_loss_grad(cache["u"], target)
    return loss, oracle.glyph_backward(P, cache, rnd_du(rnd, du), cfg, rnd=rnd)


def seeded_moment(G, seed=77):
    """A non-zero exp_avg to start from: per tensor randn x rms(g) (1e-3 where the gradient is all zero), with a seeded eighth of
    the elements exactly zero -- there c = (1 - b1) g, so the gradient alone decides the sign, and where the gradient is exactly
    zero too (unused embedding rows, dead output pixels) c is exactly zero and both sides must take s = 0."""
    gen = torch.Generator().manual_seed(seed)
    M = {}
    for k, g in G.items():
        rms = float(g.double().pow(2).mean().sqrt()) or 1e-3
        m = torch.randn(g.shape, generator=gen) * rms
        m[torch.rand(g.shape, generator=gen) < 0.125] = 0.0
        M[k] = m.float()
    return M


def lion_train_step(P, M, x, target, cfg, font=None, max_norm=None, lr=LR, b1=B1, b2=B2, wd=WD, rnd=None):
    """One Lion training step on the CPU oracle: forward_backward, the optional clip coefficient (clip_ref.clip_coef on the
    gradient's fp64 sum of squares), then lion_step on g * coef.  Returns (loss, grads (unscaled), new_p, new_m, c, coef)."""
    loss, G = forward_backward(P, x, target, cfg, font=font, rnd=rnd)
    coef = 1.0 if max_norm is None else clip_ref.clip_coef(clip_ref.grad_sumsq(G), max_norm)[1]
    nP, nM, Cs = {}, {}, {}
    for k in P:
        nP[k], nM[k], Cs[k] = lion_step(P[k], G[k] * coef, M[k], lr, b1, b2, wd)
    return loss, G, nP, nM, Cs, coef


def grad_bar(name, dtype):
    """The existing gradient bound of a model and dtype, relative to the tensor's largest entry: 1e-4 in f32 and bf16x3
    (test_gpu_models, test_gpu_bf16x3); 3e-2 in bf16 against the oracle with the engine's rounding sites (test_gpu_models); C5-mini
    1e-5 against the oracle evaluated in fp64, which is how `reference` evaluates it (test_gpu_pixel: its f32 evaluation flips ReLU
    gates that are within rounding of zero and is itself 2.3e-3 away)."""
    return 3e-2 if dtype == "bf16" else 1e-5 if name == "c5-mini" else 1e-4


def moment_bar(name, dtype, ref, k, b2=B2):
    """The bound on exp_avg of tensor k.  f32, bf16x3 and C5-mini: the one test_gpu_clip holds exp_avg to, 1e-4 (C5-mini: 4e-3) of the
    tensor's largest entry.  bf16 has no such comparison yet: new_m = b2 m + (1 - b2) g moves by (1 - b2) times the gradient's error,
    3e-2 max|g_ref|, plus two roundings of the result."""
    top = float(ref["new_m"][k].abs().max())
    if dtype == "bf16":
        return (1.0 - b2) * ref["tau"][k] + 2.0 ** -22 * top
    return (4e-3 if name == "c5-mini" else 1e-4) * max(top, 1e-30)


def param_bar(name, dtype, ref_p, lr=LR):
    """The existing parameter bound -- 2e-5 in f32, 1e-4 in bf16x3, C5-mini max(2e-5 max|p|, 3.2e-5) (test_gpu_clip) -- but never more
    than lr / 4: the three legal outcomes of an undecided element are lr apart, and a bound of their distance would tell nothing."""
    bar = 1e-4 if dtype == "bf16x3" else max(2e-5 * float(ref_p.abs().max()), 3.2e-5) if name == "c5-mini" else 2e-5
    return min(bar, lr / 4)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="f32", clipped=False):
    """The oracle's Lion step of a case from the seeded moment, computed once: dict with P, M (the start), loss, G, new_p, new_m,
    c, coef, max_norm, and tau -- per tensor the absolute bound on the engine's gradient, grad_bar x max|g_ref| (x coef when
    clipped), below which |c_ref| does not decide the sign.  dtype "bf16": the oracle rounds where the bf16 engine rounds."""
    cfg, x, font, t = case(name)
    tf = t.float() / 255.0
    P = tparams(cfg)
    if name == "c5-mini":                          # the tight reference of this model is its fp64 evaluation (grad_bar)
        P, tf = {k: v.double() for k, v in P.items()}, t.double() / 255.0
    rnd = engine_rounding(cfg, dtype, train_step=True)
    _, G0 = forward_backward(P, x, tf, cfg, font=font, rnd=rnd)
    M = seeded_moment(G0)
    max_norm = 0.25 * float(np.sqrt(clip_ref.grad_sumsq(G0))) if clipped else None
    loss, G, nP, nM, Cs, coef = lion_train_step(P, M, x, tf, cfg, font=font, max_norm=max_norm, rnd=rnd)
    tau = {k: grad_bar(name, dtype) * coef * float(G[k].abs().max()) for k in G}
    P = {k: v.float() for k, v in P.items()}
    return dict(P=P, M=M, loss=float(loss), G=G, new_p=nP, new_m=nM, c=Cs, coef=coef, max_norm=max_norm, tau=tau)


def undecided_share(ref):
    """Undecided elements (|c_ref| <= tau, less those where c_ref is exactly zero because g and m both are) over all elements."""
    und = sum(int(((ref["c"][k].abs() <= ref["tau"][k]) & ~exact_zero(ref, k)).sum()) for k in ref["c"])
    return und / sum(v.numel() for v in ref["c"].values())


def exact_zero(ref, k):
    """Elements whose gradient is zero by STRUCTURE (unused embedding rows, dead output pixels: sums of exact zeros on both sides) and
    whose moment is zero: c = 0 exactly, so s = 0.  The key third of an attention in_proj_bias is not among them: its gradient is
    zero analytically (softmax does not see the key bias) but rounding noise numerically -- 1e-19 in the fp64 oracle, a few entries of
    which cancel to an exact 0 by chance -- so an engine may take either sign there: undecided by construction."""
    z = (ref["G"][k] == 0) & (ref["M"][k] == 0)
    if k.endswith("in_proj_bias"):
        n = z.numel() // 3
        z = z.clone()
        z.view(-1)[n:2 * n] = False
    return z


def compare(ref, k, p_old, p_new, m_new, pbar, mbar, lr=LR, wd=WD, check_p=True):
    """Tensor k of an engine step against ref, every element: the moment within mbar; a decided parameter within pbar of the
    reference's; an undecided one within pbar of p_old decay + one of {-lr, 0, +lr}; where g_ref and m are both exactly zero, of
    p_old decay itself.  Returns the number of undecided elements."""
    rp, rm, c = ref["new_p"][k], ref["new_m"][k], ref["c"][k]
    p_old, p_new, m_new = p_old.double().cpu(), p_new.double().cpu(), m_new.double().cpu()
    dm = float((m_new - rm).abs().max())
    assert dm <= mbar, ("exp_avg", k, dm, mbar)
    zero = exact_zero(ref, k)
    und = (c.abs() <= ref["tau"][k]) & ~zero
    if not check_p:
        return int(und.sum())
    dec = ~und & ~zero
    dp = float((p_new - rp)[dec].abs().max()) if bool(dec.any()) else 0.0
    assert dp <= pbar, ("decided parameter", k, dp, pbar)
    base = p_old * (1.0 - lr * wd)
    dz = float((p_new - base)[zero].abs().max()) if bool(zero.any()) else 0.0
    assert dz <= pbar, ("g = m = 0: s must be 0", k, dz, pbar)
    if bool(und.any()):
        legal = torch.stack([(p_new - (base - lr * s)).abs() for s in (-1.0, 0.0, 1.0)]).min(0).values
        du = float(legal[und].max())
        assert du <= pbar, ("undecided parameter is no legal outcome", k, du, pbar)
    return int(und.sum())
