"""CPU: the optimizer groups' checker (tests/groups_ref.py) against torch.optim.AdamW with real param groups, the power of the bounds the
GPU test holds a grouped step to, the host-only half of the C ABI (afr_set_param_groups / afr_param_group_ranges: validation and the
merged table; libafr.so loads without a GPU), and the default no-decay rule."""
import ctypes as C

import pytest
import torch

from . import groups_ref, lion_ref
from .util import MINI

C5_NAMES_HEAD = ["positional_encoding", "embedding.weight", "font_embedding.weight", "layers.0.ln1.weight", "layers.0.ln1.bias",
                 "layers.0.attn.in_proj_bias", "layers.0.attn.out_proj.bias", "layers.0.ln2.weight", "layers.0.ln2.bias", "layers.0.fc1.bias",
                 "layers.0.fc2.bias"]


def _configs():
    from ai_font_renderer_amd.config import C5_MINI
    return dict(mini=MINI, small=lion_ref.SMALL, c5=C5_MINI)


# ----------------------------------------------------------------------------- 1. the checker against torch
@pytest.mark.parametrize("which", ["small", "mini"])
def test_checker_equals_torch_adamw_with_real_param_groups(which):
    """Random p, g, m, v in the shapes of glyph-small / sheet-mini, three steps with fresh gradients, the two groups of the stitch test
    plus a third (one matrix at lr x 2, wd x 0.25): groups_ref.adamw_groups_step against torch.optim.AdamW built with one param group per
    tensor, both in fp64, to 1e-12 of each tensor's largest entry."""
    cfg = _configs()[which]
    gen = torch.Generator().manual_seed(3)
    shapes = dict(cfg.param_shapes())
    P = {k: torch.randn(s, generator=gen, dtype=torch.float64) * 0.5 for k, s in shapes.items()}
    M = {k: torch.randn(s, generator=gen, dtype=torch.float64) * 0.01 for k, s in shapes.items()}
    V = {k: torch.rand(s, generator=gen, dtype=torch.float64) * 1e-4 + 1e-8 for k, s in shapes.items()}
    lm, wm = groups_ref.two_groups(cfg)
    lm["fc_output.weight"], wm["fc_output.weight"] = 2.0, 0.25
    Pt, Mt, Vt = P, M, V
    for t in (1, 2, 3):
        G = {k: torch.randn(s, generator=gen, dtype=torch.float64) * 0.01 for k, s in shapes.items()}
        P, M, V = groups_ref.adamw_groups_step(P, G, M, V, t, lm, wm)
        Pt, Mt, Vt = groups_ref.torch_groups_step(Pt, G, Mt, Vt, t, lm, wm)
        for mine, theirs, tag in ((P, Pt, "p"), (M, Mt, "m"), (V, Vt, "v")):
            for k in mine:
                d = float((mine[k] - theirs[k]).abs().max())
                assert d <= 1e-12 * float(theirs[k].abs().max()), (t, tag, k, d)
    # (and the groups matter: the same three steps with one group end elsewhere)
    assert float((groups_ref.adamw_groups_step(Pt, G, Mt, Vt, 4)[0]["fc_output.weight"]
                  - groups_ref.adamw_groups_step(Pt, G, Mt, Vt, 4, lm, wm)[0]["fc_output.weight"]).abs().max()) > 1e-6


# ----------------------------------------------------------------------------- 2. the bound can fail
@pytest.mark.parametrize("name", ["glyph-small", "sheet-mini"])
def test_the_other_groups_scalars_move_every_tensor_past_the_gpu_tests_bound(name):
    """The GPU test compares one grouped step (lr 1e-3, wd 0.5; the default rule's tensors at (0.5, 0)) with this reference within 2e-5
    on the parameters.  A step that handed ANY tensor with a non-zero gradient the other group's (lr_i, wd_i) is further away than
    that: the hyper-parameters have power under the bound.  (The moments do not depend on lr and wd: only the parameters can tell.)"""
    ref = groups_ref.reference(name)
    lm, wm = ref["lr_mult"], ref["wd_mult"]
    mine = groups_ref.tensor_hyper("fc_output.weight", lm, wm)
    other = groups_ref.tensor_hyper("fc_output.bias", lm, wm)
    assert mine == (groups_ref.f32_mul(groups_ref.LR, 1.0), groups_ref.f32_mul(groups_ref.WD, 1.0)) and other == (groups_ref.f32_mul(groups_ref.LR, 0.5), 0.0)
    checked = 0
    for k in ref["P"]:
        if not bool((ref["G"][k] != 0).any()):
            continue
        swapped = other if groups_ref.tensor_hyper(k, lm, wm) == mine else mine
        wrong, _, _ = groups_ref.adamw_step64(ref["P"][k], ref["G"][k], ref["M"][k], ref["V"][k], 1, *swapped)
        moved = float((wrong - ref["new_p"][k]).abs().max())
        assert moved > 2 * groups_ref.PBAR, (k, moved)      # (twice: the engine itself may sit PBAR away from the reference)
        checked += 1
    assert checked == len(ref["P"])


# ----------------------------------------------------------------------------- 3. validation and the merged table, through libafr.so
def _plan(cfg):
    from ai_font_renderer_amd import _lib
    from ai_font_renderer_amd.engine import make_afr_config
    c = make_afr_config(cfg, "f32", 8)
    plan = C.c_void_p()
    _lib.check(_lib.lib().afr_plan_create(C.byref(c), C.byref(plan)))
    return plan


def _arr(cfg, mult):
    names = [k for k, _ in cfg.param_shapes()]
    return (C.c_float * len(names))(*[float((mult or {}).get(k, 1.0)) for k in names])


def _ranges(plan):
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    n = lib.afr_param_group_ranges(plan, None, 0)
    out = (_lib.AfrOptRange * max(n, 1))()
    assert lib.afr_param_group_ranges(plan, out, n) == n
    return [(r.end, r.lr_mult, r.wd_mult) for r in out[:n]]


def test_set_param_groups_validates_before_it_stores_anything():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    cfg = lion_ref.SMALL
    plan = _plan(cfg)
    n = lib.afr_param_count(plan)
    assert _ranges(plan) == []                                            # a new plan has no groups
    good = _arr(cfg, {"fc1.bias": 0.0})
    assert lib.afr_set_param_groups(plan, None, good, n) == 0
    table = _ranges(plan)
    assert len(table) == 3 and table == groups_ref.merged_ranges(cfg, None, {"fc1.bias": 0.0})
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        arr = _arr(cfg, {"fc2.weight": bad})
        for args in ((arr, None), (None, arr), (good, arr)):
            assert lib.afr_set_param_groups(plan, args[0], args[1], n) == _lib.AFR_EINVAL, bad
            assert b"finite and >= 0" in lib.afr_last_error()
            assert _ranges(plan) == table                                 # nothing was stored
    for wrong_n in (n - 1, n + 1, 0):
        assert lib.afr_set_param_groups(plan, good, good, wrong_n) == _lib.AFR_EINVAL
        assert _ranges(plan) == table
    assert lib.afr_set_param_groups(None, good, good, n) == _lib.AFR_EINVAL
    assert lib.afr_set_param_groups(plan, None, None, n) == 0             # both NULL: groups off
    assert _ranges(plan) == []
    assert lib.afr_set_param_groups(plan, _arr(cfg, None), _arr(cfg, None), n) == 0      # all ones: ON, one range
    assert _ranges(plan) == [(lib.afr_param_elems(plan), 1.0, 1.0)]
    assert lib.afr_set_param_groups(plan, _arr(cfg, None), None, n) == 0
    assert _ranges(plan) == [(lib.afr_param_elems(plan), 1.0, 1.0)]
    lib.afr_plan_destroy(plan)


@pytest.mark.parametrize("which", ["mini", "small", "c5"])
def test_merged_ranges_of_the_default_rule(which):
    """afr_param_group_ranges under the default rule with wd_mult = 0, and with the stitch test's (0.5, 0): the table groups_ref builds
    from the Python layout, and its shape spelled out -- ends at tensor offsets, the last one at the buffer's size, multipliers
    alternating."""
    from ai_font_renderer_amd import _lib
    from ai_font_renderer_amd.config import flat_layout, no_decay_names
    lib = _lib.lib()
    cfg = _configs()[which]
    plan = _plan(cfg)
    n = lib.afr_param_count(plan)
    wm = {k: 0.0 for k in no_decay_names(cfg)}
    assert lib.afr_set_param_groups(plan, None, _arr(cfg, wm), n) == 0
    got = _ranges(plan)
    assert got == groups_ref.merged_ranges(cfg, None, wm)
    table, total = flat_layout(cfg)
    offsets = {o for _, _, o, _ in table} | {total}
    assert got[-1][0] == total and all(e in offsets and e % 64 == 0 for e, _, _ in got)
    assert all(a[2] != b[2] for a, b in zip(got, got[1:])) and all(r[1] == 1.0 for r in got)
    # mini: [pos, emb] | in_proj_weight | in_proj_bias | out_proj.weight | out_proj.bias, ln.weight, ln.bias | fc1.weight | fc1.bias |
    #       fc_output.weight | fc_output.bias;  small: [emb, font] | fc1.w | fc1.b | fc2.w | fc2.b | out.w | out.b;  c5: 3 + 8 per block + 2 - 1
    assert len(got) == {"mini": 9, "small": 7, "c5": 1 + 8 * cfg.layers + 2 if which == "c5" else 0}[which]
    assert got[0] == (table[2][2] if which != "c5" else table[5][2], 1.0, 0.0)
    lm, wm2 = groups_ref.two_groups(cfg)
    assert lib.afr_set_param_groups(plan, _arr(cfg, lm), _arr(cfg, wm2), n) == 0
    assert _ranges(plan) == groups_ref.merged_ranges(cfg, lm, wm2) and len(_ranges(plan)) == len(got)
    # a cap smaller than the table: the count is still returned, only `cap` entries are written
    two = (_lib.AfrOptRange * 3)()
    two[2].end = -7
    assert lib.afr_param_group_ranges(plan, two, 2) == len(got) and two[2].end == -7 and two[1].end == got[1][0]
    lib.afr_plan_destroy(plan)


def test_op_opt_groups_refuses_bad_tables_before_it_launches():
    """Argument validation only (nothing is launched, no GPU): ends must be multiples of 4, strictly increasing, and reach the end of
    the slice; more than 128 ranges inside one slice are AFR_EUNSUPPORTED, never a silent drop."""
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(0x1000)

    def call(ranges, n=256, first=0, kind=0):
        arr = (_lib.AfrOptRange * len(ranges))(*[_lib.AfrOptRange(e, a, b) for e, a, b in ranges])
        return lib.afr_op_opt_groups(kind, fake, fake, fake, fake, None, n, first, arr, len(ranges), 1e-3, 0.9, 0.99, 1e-8, 0.5, 1, 1.0, None, 0.0, None)
    assert call([(64, 1.0, 1.0), (62, 1.0, 1.0), (256, 1.0, 1.0)]) == _lib.AFR_EINVAL
    assert call([(64, 1.0, 1.0), (64, 2.0, 1.0), (256, 1.0, 1.0)]) == _lib.AFR_EINVAL
    assert call([(64, 1.0, 1.0), (128, 1.0, 1.0)]) == _lib.AFR_EINVAL and b"before the slice's end" in lib.afr_last_error()
    assert call([(64, 1.0, 1.0), (256, 1.0, 1.0)], first=64) == _lib.AFR_EINVAL          # the slice ends at 320
    assert call([(256, -1.0, 1.0)]) == _lib.AFR_EINVAL and call([(256, 1.0, float("nan"))]) == _lib.AFR_EINVAL
    assert call([(256, 1.0, 1.0)], first=2) == _lib.AFR_EINVAL and call([(256, 1.0, 1.0)], kind=2) == _lib.AFR_EINVAL
    many = [(4 * (i + 1), 1.0 + i, 1.0) for i in range(129)]
    assert call(many, n=4 * 129) == _lib.AFR_EUNSUPPORTED and b"at most 128" in lib.afr_last_error()


# ----------------------------------------------------------------------------- 4. the default rule
def test_no_decay_names_of_the_three_configs():
    from ai_font_renderer_amd.config import no_decay_names
    cf = _configs()
    assert no_decay_names(cf["mini"]) == ["positional_encoding", "embedding.weight", "attention.in_proj_bias", "attention.out_proj.bias",
                                          "layer_norm.weight", "layer_norm.bias", "fc1.bias", "fc_output.bias"]
    assert no_decay_names(cf["small"]) == ["embedding.weight", "font_embedding.weight", "fc1.bias", "fc2.bias", "fc_output.bias"]
    c5 = no_decay_names(cf["c5"])
    assert c5[:len(C5_NAMES_HEAD)] == C5_NAMES_HEAD and c5[-3:] == ["ln_f.weight", "ln_f.bias", "fc_output.bias"]
    assert len(c5) == 3 + 8 * cf["c5"].layers + 3
    for cfg in cf.values():
        shapes = dict(cfg.param_shapes())
        decayed = [k for k in shapes if k not in no_decay_names(cfg)]
        assert decayed and all(len(shapes[k]) == 2 and k.endswith("weight") and "embedding" not in k for k in decayed)
