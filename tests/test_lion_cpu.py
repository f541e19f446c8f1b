"""CPU: the Lion optimizer kind -- the checker (tests/lion_ref.py) against a second, naive statement of the paper's algorithm, the
ABI's argument checks (afr_set_optimizer is host-only: nothing is launched), the condition under which the GPU tests' element-wise
comparison is meaningful (the reference's undecided share stays under the cap for every input they use), and that the reference
itself trains."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from . import lion_ref
from .util import ROOT, tparams


def _plan(max_batch=64):
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    c = make_afr_config(config.WORKLOADS["c1"]["cfg"], "f32", max_batch)
    plan = C.c_void_p()
    _lib.check(_lib.lib().afr_plan_create(C.byref(c), C.byref(plan)))
    return plan


def test_new_symbols_are_exported_declared_and_named_in_python():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "afr.h")).read()
    for name in ("afr_set_optimizer", "afr_op_lion"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert "AFR_OPT_ADAMW = 0" in header and "AFR_OPT_LION = 1" in header
    assert (_lib.AFR_OPT_ADAMW, _lib.AFR_OPT_LION) == (0, 1)
    assert _lib.opt_kind("adamw") == 0 and _lib.opt_kind("lion") == 1
    for bad in ("sgd", "", None, 1):
        with pytest.raises(ValueError):
            _lib.opt_kind(bad)


def test_set_optimizer_accepts_both_kinds_and_rejects_others_with_a_message():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    plan = _plan()
    for ok in (0, 1, 0, 1):                                              # host-only: an unbound plan takes the setting, either way round
        assert lib.afr_set_optimizer(plan, ok) == 0, ok
    for bad in (-1, 2):
        assert lib.afr_set_optimizer(plan, bad) == -1, bad               # AFR_EINVAL
        assert b"optimizer kind" in lib.afr_last_error() and str(bad).encode() in lib.afr_last_error()
    assert lib.afr_set_optimizer(None, 1) == -1
    fake = C.c_void_p(0x1000)
    assert lib.afr_adamw_step(plan, 1e-4, 0.9, 0.99, 1e-8, 5e-3, 1, 1.0, None) == -2       # an unbound Lion plan: AFR_ESTATE
    assert b"Lion" in lib.afr_last_error()
    assert lib.afr_op_lion(None, fake, fake, None, 64, 1e-4, 0.9, 0.99, 5e-3, 1.0, None, 0.0, None) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):                 # a clipped slice step needs a max_norm, as afr_op_adamw_clip does
        assert lib.afr_op_lion(fake, fake, fake, None, 64, 1e-4, 0.9, 0.99, 5e-3, 1.0, fake, bad, None) == -1, bad
        assert b"max_norm" in lib.afr_last_error()
    lib.afr_plan_destroy(plan)


def _naive_lion(p, g, m, lr, b1, b2, wd):
    """Algorithm 2 of Chen et al. 2023, element by element in Python floats: c_t = b1 m + (1 - b1) g; theta = theta - lr (sign(c_t) +
    wd theta); m = b2 m + (1 - b2) g."""
    out_p, out_m = [], []
    for pi, gi, mi in zip(p.tolist(), g.tolist(), m.tolist()):
        c = b1 * mi + (1 - b1) * gi
        s = 1.0 if c > 0 else -1.0 if c < 0 else 0.0
        out_p.append(pi - lr * (s + wd * pi))
        out_m.append(b2 * mi + (1 - b2) * gi)
    return np.array(out_p), np.array(out_m)


def test_checker_equals_a_naive_statement_of_the_papers_algorithm():
    gen = torch.Generator().manual_seed(3)
    n = 4096
    p, g, m = (torch.randn(n, generator=gen) * s for s in (1.0, 0.37, 0.37))
    g[:64] = 0.0
    m[:32] = 0.0                                                         # c exactly 0 on the first 32: sign 0, decay only
    m[100:164] = -g[100:164] / 9.0                                       # c = 0.9 m + 0.1 g is a rounding residue there
    for lr, wd in ((1e-4, 5e-3), (1e-3, 0.0), (3e-2, 0.1)):
        np_, nm_, c = lion_ref.lion_step(p, g, m, lr, 0.9, 0.99, wd)
        rp, rm = _naive_lion(p.double(), g.double(), m.double(), lr, 0.9, 0.99, wd)
        sure = (c.abs().numpy() > 1e-12) | (c.numpy() == 0)              # (a rounding residue may take either sign in either statement)
        assert sure.sum() >= n - 64
        assert np.abs(np_.numpy() - rp)[sure].max() <= 1e-15
        assert np.abs(nm_.numpy() - rm).max() <= 1e-15
        assert np.array_equal(np_.numpy()[:32], (p.double() * (1.0 - lr * wd)).numpy()[:32])
        steps = (np_ - p.double() * (1.0 - lr * wd)).abs().numpy()[sure]
        assert np.allclose(steps[steps > 0], lr, rtol=0, atol=1e-15) and (steps == 0).sum() == 32


CASES = [(name, dtype) for name in lion_ref.CASES for dtype in ("f32",)] + [("sheet-mini", "bf16x3")]
BF16_CASES = [("glyph-small", "bf16"), ("glyph-c1", "bf16"), ("sheet-mini", "bf16"), ("sheet-deep", "bf16")]


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("name,dtype", CASES)
def test_reference_undecided_share_stays_under_the_cap(name, dtype, clipped):
    """Every (fixture, dtype) whose parameters test_gpu_lion.py compares with the oracle: the share of elements with |c_ref| <= tau
    (tau = the existing absolute gradient bound of the model, per tensor) must stay under 2 % of the model, or that comparison
    would excuse too much.  (bf16x3 shares f32's oracle and bound.)  The exactly-zero class must exist, or nothing checks s = 0."""
    ref = lion_ref.reference(name, "f32" if dtype == "bf16x3" else dtype, clipped)
    share = lion_ref.undecided_share(ref)
    zeros = sum(int(lion_ref.exact_zero(ref, k).sum()) for k in ref["c"])
    worst = max(ref["c"], key=lambda k: float((ref["c"][k].abs() <= ref["tau"][k]).double().mean()))
    print(f"{name}/{dtype} clipped={clipped}: undecided share {share:.2e}, exact zeros {zeros}, worst tensor {worst} "
          f"({float((ref['c'][worst].abs() <= ref['tau'][worst]).double().mean()):.3f}), coef {ref['coef']:.4f}")
    assert share <= lion_ref.CAP, (name, dtype, share)
    assert clipped == (ref["coef"] < 0.5)
    if name.startswith("sheet"):
        assert zeros > 0


@pytest.mark.parametrize("name,dtype", BF16_CASES)
def test_bf16_undecided_share_decides_what_the_gpu_test_compares(name, dtype):
    """bf16: tau is the bf16 gradient bound, 3e-2 of each tensor's largest gradient entry, against the oracle with the engine's
    rounding sites.  Where that leaves more than the cap undecided, test_gpu_lion.py compares only the moment with the oracle for the
    fixture (lion_ref.BF16_MOMENT_ONLY must name exactly those); the bf16 parameters are then covered by its bitwise path tests."""
    share = lion_ref.undecided_share(lion_ref.reference(name, dtype))
    print(f"{name}/{dtype}: undecided share {share:.3e} at tau = 3e-2 max|g|")
    assert (share > lion_ref.CAP) == (name in lion_ref.BF16_MOMENT_ONLY), (name, share)


def test_the_reference_trains_glyph_small_in_30_steps():
    """30 Lion steps of glyph-small at lr = 1e-4, wd = 5e-3 on the CPU oracle from a zero moment: the last loss lies below the first
    (test_gpu_lion.py asserts the same of the engine; the two trajectories part at the first undecided sign)."""
    cfg, x, font, t = lion_ref.case("glyph-small")
    tf = t.float() / 255.0
    P = tparams(cfg)
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    losses = []
    for _ in range(30):
        loss, _, nP, nM, _, _ = lion_ref.lion_train_step(P, M, x, tf, cfg, font=font)
        P, M = {k: v.float() for k, v in nP.items()}, {k: v.float() for k, v in nM.items()}
        losses.append(float(loss))
    print(f"CPU reference, glyph-small, 30 Lion steps: loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert losses[-1] < losses[0]
