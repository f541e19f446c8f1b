"""GPU: the optimizer groups (afr_set_param_groups / afr_op_opt_groups / Engine.set_param_groups) through every optimizer path: the
range-aware flat kernel against fp64 and, bit for bit, against the plain kernels launched range by range; all-ones multipliers and
uniform multipliers against an engine without groups, bit for bit; the stitch test -- every tensor of a two-group engine bit-identical
to the same tensor of an ungrouped engine stepped with that tensor's (lr_i, wd_i), through every path that ends in an optimizer step;
one step against torch's param groups (tests/groups_ref.py); and the surface.

Gradients do not depend on the optimizer's scalars, so from the same state and batch a grouped engine and an ungrouped one see the
same gradients to the last bit: the bitwise tests need no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import clip_ref, groups_ref, lion_ref
from . import opt_paths as OP
from .groups_ref import B1, B2, EPS, LR, WD, f32_mul
from .gpu_util import ptr, stream
from .opt_paths import UNFUSED, assert_same_state, no_error_bits_left_behind  # noqa: F401
from .opt_paths import assert_tensor_same as _assert_tensor_same
from .opt_paths import engine as _engine
from .opt_paths import probe_grads as _probe_grads
from .opt_paths import seed_moments as _seed

pytestmark = pytest.mark.gpu

OPTS = ("adamw", "lion")


def _hyper(lr=LR, wd=WD):
    return dict(lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd)


# ----------------------------------------------------------------------------- 1. the flat kernel, op level
def _ranges_arr(ranges):
    from ai_font_renderer_amd import _lib
    return (_lib.AfrOptRange * len(ranges))(*[_lib.AfrOptRange(int(e), float(a), float(b)) for e, a, b in ranges])


def _op_groups(kind, p, g, m, v, shadow, first, ranges, t, gscale, sumsq, max_norm, lr=LR, wd=WD):
    from ai_font_renderer_amd import _lib
    _lib.check(_lib.lib().afr_op_opt_groups(_lib.opt_kind(kind), ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), p.numel(), first, _ranges_arr(ranges),
                                            len(ranges), lr, B1, B2, EPS, wd, t, gscale, ptr(sumsq), max_norm, stream()))
    torch.cuda.synchronize()


def _op_plain(kind, p, g, m, v, shadow, lr, wd, t, gscale, sumsq, max_norm):
    """The existing slice entries: afr_op_adamw / afr_op_adamw_clip / afr_op_lion."""
    from ai_font_renderer_amd import _lib
    lib, n = _lib.lib(), p.numel()
    if kind == "lion":
        _lib.check(lib.afr_op_lion(ptr(p), ptr(g), ptr(m), ptr(shadow), n, lr, B1, B2, wd, gscale, ptr(sumsq), max_norm, stream()))
    elif sumsq is not None:
        _lib.check(lib.afr_op_adamw_clip(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), n, lr, B1, B2, EPS, wd, t, gscale, ptr(sumsq), max_norm, stream()))
    else:
        _lib.check(lib.afr_op_adamw(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), n, lr, B1, B2, EPS, wd, t, gscale, stream()))


TRIP = 4 * 4096 * 256                           # elements of the first grid-stride trip: 4096 blocks x 256 lanes x 4
LAYOUTS = {
    # name: (n, first, [(end in FLAT coordinates, lr_mult, wd_mult)])
    "one-range": (64, 0, [(64, 0.5, 2.0)]),
    "wave-straddles-four": (256, 0, [(64, 0.5, 0.0), (128, 1.0, 1.0), (192, 2.0, 0.25), (256, 0.25, 3.0)]),
    # a range that ends before the slice, one early boundary, then boundaries 4 elements before, at and 4 elements after the end of
    # the first trip (slice coordinates), the last range reaching past the slice; first != 0
    "trip-boundaries": (4 * (4096 * 256 + 3), 192, [(128, 3.0, 3.0), (192 + 4000, 0.5, 0.0), (192 + TRIP - 4, 1.0, 1.0), (192 + TRIP, 2.0, 0.25),
                                                   (192 + TRIP + 4, 0.25, 3.0), (192 + 4 * (4096 * 256 + 3) + 64, 1.5, 0.5)]),
}
GUARD = 64


def _between_guards(x, fill):
    """x on the device between two guard bands of GUARD elements; returns (whole buffer, the view of x)."""
    buf = torch.full((x.numel() + 2 * GUARD,), fill, dtype=x.dtype, device="cuda")
    buf[GUARD:GUARD + x.numel()].copy_(x)
    return buf, buf[GUARD:GUARD + x.numel()]


def _per_element(n, first, ranges, lr, wd):
    """(lr_i, wd_i) of every element of the slice as fp64 vectors holding the f32 products, and the slice-relative pieces."""
    lrv, wdv, pieces = torch.empty(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64), []
    lo = 0
    for end, lm, wm in ranges:
        hi = min(max(end - first, 0), n)
        if hi > lo:
            lrv[lo:hi], wdv[lo:hi] = f32_mul(lr, lm), f32_mul(wd, wm)
            pieces.append((lo, hi, f32_mul(lr, lm), f32_mul(wd, wm)))
            lo = hi
    assert lo == n
    return lrv, wdv, pieces


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", OPTS)
def test_op_opt_groups_vs_fp64_and_the_plain_kernels_range_by_range(kind, layout):
    """afr_op_opt_groups on a slice with a bf16 shadow, plain (grad_scale 1 and 0.5) and clipped (a coefficient below 0.5), t = 2 from a
    non-zero state; p ~ 0.5, g and m ~ 0.01 as in test_adamw_three_steps_match_torch_optim.
    (a) Against fp64 with every element's own (lr_i, wd_i), every element.  AdamW: the parameter within 2e-6, that test's bound;
    exp_avg within 4 x 2^-24 x max(|g|, |m|) (two f32 operations on values of that size), exp_avg_sq within 6 x 2^-24 x (v + g^2) (four
    roundings of positive terms that size).  Lion: the element-wise rule of lion_ref.compare as test_op_lion_vs_fp64_every_element
    applies it -- the moment within 4 x 2^-24 x max(|g|, |m|), a decided parameter within 4 x 2^-24 x (|p| + lr_i) of the reference, an
    undecided one (|c| <= 4 x 2^-24 x max(|g|, |m|)) within that of one of the three legal outcomes.
    (b) Bit-identical -- p, m, v, shadow -- to afr_op_adamw / afr_op_adamw_clip / afr_op_lion launched range by range with lr_i, wd_i.
    (c) The 64-element guard bands around every buffer stay untouched."""
    n, first, ranges = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(40 + n % 11)
    p0 = torch.randn(n, generator=gen) * 0.5
    g = torch.randn(n, generator=gen) * 0.01
    m0 = torch.randn(n, generator=gen) * 0.01
    v0 = (torch.rand(n, generator=gen) + 0.5) * 1e-4
    g[5], m0[5] = 0.0, 0.0                                                # (Lion: c exactly zero, decay only)
    u, t = 2.0 ** -24, 2
    b1, b2, eps = (float(np.float32(a)) for a in (B1, B2, EPS))          # the f32 values the kernel is handed
    lrv, wdv, pieces = _per_element(n, first, ranges, LR, WD)
    assert layout != "wave-straddles-four" or len(pieces) == 4
    assert layout != "trip-boundaries" or [hi for _, hi, _, _ in pieces] == [4000, TRIP - 4, TRIP, TRIP + 4, n]
    sumsq_of_g = float((g.double() ** 2).sum())
    for gscale, clip in ((1.0, False), (0.5, False), (0.5, True)):
        factor, ss, max_norm = np.float32(gscale), None, 0.0
        if clip:
            max_norm = 0.25 * abs(gscale) * sumsq_of_g ** 0.5
            ss = torch.tensor([sumsq_of_g], dtype=torch.float32).cuda()
            coef = clip_ref.clip_coef(float(ss), max_norm, gscale)[1]
            assert coef < 0.5
            factor = np.float32(gscale) * np.float32(coef)
        bufs = {}
        for who in ("grouped", "plain"):
            bufs[who] = [_between_guards(x, fill) for x, fill in ((p0, 7.0), (g, 7.0), (m0, 7.0), (v0, 7.0), (torch.zeros(n, dtype=torch.bfloat16), 3.0))]
        (_, p), (_, gd), (_, m), (_, v), (_, sh) = bufs["grouped"]
        _op_groups(kind, p, gd, m, None if kind == "lion" else v, sh, first, ranges, t, gscale, ss, max_norm)
        (_, pp), (_, gp), (_, mp), (_, vp), (_, shp) = bufs["plain"]
        for lo, hi, lr_i, wd_i in pieces:
            _op_plain(kind, pp[lo:hi], gp[lo:hi], mp[lo:hi], vp[lo:hi], shp[lo:hi], lr_i, wd_i, t, gscale, ss, max_norm)
        torch.cuda.synchronize()
        # (b) and (c): whole buffers, guard bands included
        for (whole, _), (whole_p, _), tag in zip(bufs["grouped"], bufs["plain"], ("p", "g", "m", "v", "shadow")):
            assert torch.equal(whole, whole_p), (tag, gscale, clip, int((whole != whole_p).sum()))
            fill = 3.0 if tag == "shadow" else 7.0
            assert bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all()), tag
        assert torch.equal(gd.cpu(), g) and torch.equal(sh, p.to(torch.bfloat16))
        if kind == "lion":
            assert torch.equal(v.cpu(), v0)                               # exp_avg_sq is not touched (the pointer was NULL)
        # (a)
        ge = (g * torch.tensor(factor)).float()                          # one rounded product, as the kernel forms it
        got_p, got_m = p.cpu().double(), m.cpu().double()
        size = torch.maximum(ge.abs(), m0.abs()).double()
        if kind == "adamw":
            rp, rm, rv = groups_ref.adamw_step64(p0, ge, m0, v0, t, lrv, wdv, b1, b2, eps)
            assert float((got_p - rp).abs().max()) < 2e-6, (gscale, clip, float((got_p - rp).abs().max()))
            assert bool(((got_m - rm).abs() <= 4 * u * size).all()), (gscale, clip)
            assert bool(((v.cpu().double() - rv).abs() <= 6 * u * (v0.double() + ge.double() ** 2)).all()), (gscale, clip)
            continue
        c = b1 * m0.double() + (1.0 - b1) * ge.double()
        base = p0.double() * (1.0 - lrv * wdv)
        rp, rm = base - lrv * torch.sign(c), b2 * m0.double() + (1.0 - b2) * ge.double()
        assert bool(((got_m - rm).abs() <= 4 * u * size).all()), (gscale, clip)
        pbar = 4 * u * (p0.abs().double() + lrv)
        und = c.abs() <= 4 * u * size
        assert bool(((got_p - rp).abs() <= pbar)[~und].all()), (gscale, clip)
        legal = torch.stack([(got_p - (base - lrv * s)).abs() for s in (-1.0, 0.0, 1.0)]).min(0).values
        assert bool((legal <= pbar)[und].all()), (gscale, clip)
        assert bool(und[5]) and abs(float(got_p[5]) - float(base[5])) <= float(pbar[5])
        assert int(und.sum()) <= lion_ref.CAP * n + 2


@pytest.mark.parametrize("kind", OPTS)
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_op_opt_groups_non_finite_sumsq_leaves_everything_bit_identical(bad, kind):
    gen = torch.Generator().manual_seed(5)
    n = 4096
    p, g, m = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    v = torch.rand(n, generator=gen).cuda()
    shadow = torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda")
    ranges = [(1024, 0.5, 0.0), (4096, 1.0, 1.0)]
    before = [x.clone() for x in (p, m, v, shadow)]
    _op_groups(kind, p, g, m, v, shadow, 0, ranges, 1, 1.0, torch.tensor([bad], dtype=torch.float32).cuda(), 1.0)
    for x, w in zip((p, m, v, shadow), before):
        assert torch.equal(x, w)
    _op_groups(kind, p, g, m, v, shadow, 0, ranges, 1, 1.0, torch.tensor([1.0], dtype=torch.float32).cuda(), 1.0)
    assert not torch.equal(p, before[0]) and not torch.equal(m, before[1]) and torch.equal(shadow, p.to(torch.bfloat16))


# ----------------------------------------------------------------------------- 2 + 3. all ones is the identity; uniform multipliers scale
CASE_DTYPES = [(n, d) for n in lion_ref.CASES for d in ("f32", "bf16")]


@pytest.mark.parametrize("mode", ["all-ones", "uniform"])
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_all_ones_is_the_identity_and_uniform_multipliers_scale_the_step_bitwise(name, dtype, mode):
    """all-ones: an engine with every lr_mult / wd_mult at 1.0 (groups ON: one range) against an engine without groups stepped with the
    same lr, wd.  uniform: multipliers a = 0.5, b = 2 on every tensor against an ungrouped engine stepped with fl32(lr * a),
    fl32(wd * b).  Two AdamW steps each through the fused one-call step, AFR_CFG_UNFUSED_OPTIMIZER and a clipping plan (0.25 x the
    first norm): p, m, v, the bf16 shadows and the losses bit for bit.  glyph-c1 is the fused small-net step, sheet-deep (B = 37) the
    grouped reduce's deep branch."""
    cfg, x, font, t = lion_ref.case(name)
    B = x.shape[0]
    names = [k for k, _ in cfg.param_shapes()]
    a, b = (1.0, 1.0) if mode == "all-ones" else (0.5, 2.0)
    _, norm = _probe_grads(cfg, dtype, x, t, font)
    for path, kw in (("fused", {}), ("unfused", dict(flags=UNFUSED)), ("clipped", dict(max_grad_norm=0.25 * norm))):
        grouped = _engine(cfg, dtype, B, lr_mult={k: a for k in names}, wd_mult={k: b for k in names}, **kw)
        plain = _engine(cfg, dtype, B, **kw)
        assert grouped.param_group_ranges() == [(grouped.n_flat, a, b)] and plain.param_group_ranges() == []
        for i in range(2):
            grouped.train_step(x, t, font=font, step=i + 1, **_hyper())
            plain.train_step(x, t, font=font, step=i + 1, **_hyper(f32_mul(LR, a), f32_mul(WD, b)))
            assert grouped.read_loss() == plain.read_loss(), (path, i)
            if path == "clipped":
                assert grouped.clip_coef() == plain.clip_coef() and (i > 0 or plain.clip_coef() < 0.5)      # (the first step is clipped for sure)
        assert_same_state(grouped, plain, (mode, path), padding=True)      # (padding included: both took the same path)
        assert float(grouped.exp_avg.abs().max()) > 0


# ----------------------------------------------------------------------------- 4. the stitch test
def _stitch_engines(cfg, dtype, B, opt, M, V, **kw):
    """(the two-group engine, {(lr_i, wd_i): an ungrouped engine to be stepped with them}), all in the same seeded state."""
    lm, wm = groups_ref.two_groups(cfg)
    grouped = _engine(cfg, dtype, B, optimizer=opt, lr_mult=lm, wd_mult=wm, **kw)
    plain = {h: _engine(cfg, dtype, B, optimizer=opt, **kw) for h in sorted({groups_ref.tensor_hyper(k, lm, wm) for k, _ in cfg.param_shapes()})}
    assert len(plain) == 2 and len(grouped.param_group_ranges()) > 2
    for e in [grouped] + list(plain.values()):
        _seed(e, M, V)
    return grouped, plain


def _assert_stitched(grouped, plain, what):
    lm, wm = groups_ref.two_groups(grouped.cfg)
    for nm, _, _, _ in grouped.layout:
        _assert_tensor_same(grouped, plain[groups_ref.tensor_hyper(nm, lm, wm)], nm, what)
    a, b = plain.values()
    assert not torch.equal(a.flat_params, b.flat_params)                  # (the two settings do differ)


STITCH_CASES = [(n, d) for n in ("glyph-small", "sheet-mini", "sheet-deep", "c5-mini") for d in ("f32", "bf16")]


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("name,dtype", STITCH_CASES)
def test_stitch_every_tensor_equals_the_ungrouped_step_with_its_own_scalars_bitwise(name, dtype, opt):
    """Two groups -- the default rule's tensors at (lr x 0.5, wd x 0), the rest at (1, 1) -- with lr = 1e-3, wd = 0.5, ONE step from a
    seeded non-zero state: every tensor of the grouped engine (p, m, v, bf16 shadows) is bit-identical to the same tensor of the
    ungrouped engine stepped with that tensor's (lr_i, wd_i) from the same state and batch.  Paths: the fused one-call step,
    AFR_CFG_UNFUSED_OPTIMIZER, a clipping plan (0.25 x the norm), train_step_rows.  No tolerance."""
    cfg, x, font, t = lion_ref.case(name)
    B = x.shape[0]
    G, norm = _probe_grads(cfg, dtype, x, t, font)
    M, V = groups_ref.seeded_state(G)
    for path, kw in (("fused", {}), ("unfused", dict(flags=UNFUSED)), ("clipped", dict(max_grad_norm=0.25 * norm)), ("rows", {})):
        grouped, plain = _stitch_engines(cfg, dtype, B, opt, M, V, **kw)
        losses = []
        for eng, (lr_i, wd_i) in [(grouped, (LR, WD))] + [(e, h) for h, e in plain.items()]:
            if path == "rows":
                eng.bind_dataset(x, t, font=font)
                eng.train_step_rows(torch.arange(B), step=1, **_hyper(lr_i, wd_i))
            else:
                eng.train_step(x, t, font=font, step=1, **_hyper(lr_i, wd_i))
            losses.append(eng.read_loss())
        assert losses[0] == losses[1] == losses[2], path
        if path == "clipped":
            assert grouped.clip_coef() == min(e.clip_coef() for e in plain.values()) < 0.5
        _assert_stitched(grouped, plain, (name, dtype, opt, path))


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("name,dtype", STITCH_CASES)
def test_stitch_through_micro_batch_accumulation(name, dtype, opt):
    """The batch in three micro-batches of ceil(B / 3) samples (glyph-small 300 -> 100, sheet-deep 37 -> 13 + 13 + 11, ...): the
    accumulated step ends in afr_adamw_step, which takes the range-aware kernel over the whole buffer -- the pixel plan's 35 ranges
    included.  The three engines accumulate the same way, so their gradients are the same to the last bit."""
    cfg, x, font, t = lion_ref.case(name)
    B = x.shape[0]
    mb = (B + 2) // 3
    assert 0 < mb < B
    G, _ = _probe_grads(cfg, dtype, x, t, font)
    M, V = groups_ref.seeded_state(G)
    grouped, plain = _stitch_engines(cfg, dtype, B, opt, M, V, micro_batch=mb)
    assert grouped.max_batch == mb
    for eng, (lr_i, wd_i) in [(grouped, (LR, WD))] + [(e, h) for h, e in plain.items()]:
        eng.train_step(x, t, font=font, **_hyper(lr_i, wd_i))
    _assert_stitched(grouped, plain, ("accumulation", name, dtype, opt))


@pytest.mark.parametrize("opt", OPTS)
def test_stitch_through_the_cooperative_split_k_tail(opt):
    """C3's own layers at its batch of 8192 in bf16, the shape opt_paths.COOP_CASE names for the tail (afr_op_gemm_pair_plan: a split of
    8): the weight-gradient launch applies the update itself, with the tensor's own scalars."""
    cfg, B, x, font, t = OP.coop_inputs()
    gen = torch.Generator().manual_seed(11)
    lm, wm = groups_ref.two_groups(cfg)
    grouped = _engine(cfg, "bf16", B, optimizer=opt, lr_mult=lm, wd_mult=wm)
    n = grouped.n_flat
    m0, v0 = (torch.randn(n, generator=gen) * 1e-4).cuda(), ((torch.rand(n, generator=gen) + 0.5) * 1e-8).cuda()
    plain = {h: _engine(cfg, "bf16", B, optimizer=opt) for h in sorted({groups_ref.tensor_hyper(k, lm, wm) for k, _ in cfg.param_shapes()})}
    for e in [grouped] + list(plain.values()):
        e.exp_avg.copy_(m0)
        if e.exp_avg_sq is not None:
            e.exp_avg_sq.copy_(v0)
    grouped.profile(1)
    for eng, (lr_i, wd_i) in [(grouped, (LR, WD))] + [(e, h) for h, e in plain.items()]:
        eng.train_step(x, t, font=font, **_hyper(lr_i, wd_i))
    assert OP.ran_coop_tail(grouped)
    _assert_stitched(grouped, plain, ("cooperative tail", opt))


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped", "shard-force"])
def test_stitch_through_the_data_parallel_schedules_at_world_one(schedule, opt, monkeypatch):
    """The three schedules over world-1 RCCL, a glyph net, the sheet MINI model (dropout on) and C5-mini, f32 and bf16, plain and clipped:
    one-allreduce and overlapped end in afr_adamw_step, shard-force in Engine.adamw_range on the slice -- afr_op_opt_groups with the
    plan's ranges (with the all-reduced sum of squares when clipping)."""
    from ai_font_renderer_amd.parallel import DataParallelStepper
    with OP.rccl_world_one(schedule, monkeypatch) as dist:
        glyph, sheet = (OP.inputs(c, "cuda") for c in OP.DP_CASES)
        c5cfg, c5x, c5f, c5t = lion_ref.case("c5-mini")                    # the pixel plan: 35 ranges under the two groups
        pixel = (c5cfg, c5x.shape[0], c5x.cuda(), c5f.cuda(), c5t.cuda())
        for (cfg, B, x, font, t), dtype, clip in ((glyph, "f32", False), (glyph, "bf16", True), (sheet, "f32", True), (sheet, "bf16", False),
                                                  (pixel, "f32", True), (pixel, "bf16", False)):
            G, norm = _probe_grads(cfg, dtype, x, t, font)
            M, V = groups_ref.seeded_state(G)
            kw = dict(max_grad_norm=0.25 * norm) if clip else {}
            grouped, plain = _stitch_engines(cfg, dtype, B, opt, M, V, **kw)
            me = B * cfg.pixels
            for eng, (lr_i, wd_i) in [(grouped, (LR, WD))] + [(e, h) for h, e in plain.items()]:
                st = DataParallelStepper(eng, dist, world=1 if schedule == "shard-force" else 2)
                assert st.sharded() == (schedule == "shard-force")
                st.step(x, t, font, mean_elems=me, step=1, **_hyper(lr_i, wd_i))
            _assert_stitched(grouped, plain, (schedule, cfg.kind, dtype, opt, clip))
            if dtype == "bf16":           # the shadow the next forward reads follows the stitched masters
                fresh = _engine(cfg, dtype, B)
                fresh.load_params(grouped.state_dict())
                assert torch.equal(grouped.forward(x, font), fresh.forward(x, font))


# ----------------------------------------------------------------------------- 5. against torch's param groups
@pytest.mark.parametrize("name", ["glyph-small", "sheet-mini"])
def test_one_grouped_adamw_step_vs_groups_ref(name):
    """One AdamW step in f32 with the two groups of the stitch test from the seeded state, against groups_ref.reference (fp64, held to
    torch.optim.AdamW with real param groups by test_groups_cpu.py): parameters within 2e-5, exp_avg within 1e-4 and exp_avg_sq within
    2e-4 of the tensor's largest entry -- the bounds test_gpu_clip.py holds a step to.  test_groups_cpu.py shows that any tensor handed
    the other group's scalars lands more than 4e-5 away."""
    ref = groups_ref.reference(name)
    cfg, x, font, t = lion_ref.case(name)
    eng = _engine(cfg, "f32", x.shape[0], lr_mult=ref["lr_mult"], wd_mult=ref["wd_mult"])
    _seed(eng, ref["M"], ref["V"])
    eng.train_step(x, t, font=font, **_hyper())
    for nm, shp, o, k in eng.layout:
        got = [flat[o:o + k].cpu().double().view(shp) for flat in (eng.flat_params, eng.exp_avg, eng.exp_avg_sq)]
        dp, dm, dv = (float((a - ref[key][nm]).abs().max()) for a, key in zip(got, ("new_p", "new_m", "new_v")))
        print(f"{name} {nm}: dp {dp:.2e}, dm {dm:.2e} of {float(ref['new_m'][nm].abs().max()):.2e}, dv {dv:.2e} of {float(ref['new_v'][nm].abs().max()):.2e}")
        assert dp <= groups_ref.PBAR, (nm, dp)
        assert dm <= groups_ref.MBAR * max(float(ref["new_m"][nm].abs().max()), 1e-30), ("exp_avg", nm, dm)
        assert dv <= 2 * groups_ref.MBAR * max(float(ref["new_v"][nm].abs().max()), 1e-30), ("exp_avg_sq", nm, dv)


# ----------------------------------------------------------------------------- 6. surface
def test_surface_facade_ema_replanning_and_it_trains(monkeypatch):
    from ai_font_renderer_amd import _lib, model as Mod
    from ai_font_renderer_amd.config import no_decay_names
    # the facade: AFR_NO_DECAY=1 and no_decay=True give the default rule's table
    monkeypatch.setattr(Mod, "SHEET_HEIGHT", 8)
    monkeypatch.setattr(Mod, "SHEET_WIDTH", 24)
    monkeypatch.delenv("AFR_NO_DECAY", raising=False)
    m = Mod.AttentionFontRenderer(max_length=10, max_batch=8)
    assert not m.no_decay and m.engine.param_group_ranges() == []
    want = groups_ref.merged_ranges(m.config, None, {k: 0.0 for k in no_decay_names(m.config)})
    assert len(want) == 9
    m = Mod.AttentionFontRenderer(max_length=10, max_batch=8, no_decay=True)
    assert m.no_decay and m.engine.param_group_ranges() == want
    monkeypatch.setenv("AFR_NO_DECAY", "1")
    m = Mod.AttentionFontRenderer(max_length=10, max_batch=8)
    assert m.no_decay and m.engine.param_group_ranges() == want
    assert not Mod.AttentionFontRenderer(max_length=10, max_batch=8, no_decay=False).no_decay
    assert list(m.engine.state_dict()) == [k for k, _ in m.config.param_shapes()]         # the saved state knows nothing of groups
    # names
    cfg, x, font, t = lion_ref.case("glyph-small")
    eng = _engine(cfg, "f32", 64, ema_decay=0.9)
    with pytest.raises(KeyError):
        eng.set_param_groups(wd_mult={"no.such.tensor": 0.0})
    with pytest.raises(_lib.AfrError):
        eng.set_param_groups(lr_mult={"fc1.bias": -1.0})
    assert eng.param_group_ranges() == [] and eng.lr_mult is None
    # setting groups while the engine reads its EMA weights raises, in Python and in the library
    lm, wm = groups_ref.two_groups(cfg)
    with eng.ema_weights():
        with pytest.raises(_lib.AfrError):
            eng.set_param_groups(lm, wm)
        ones = (C.c_float * len(eng.layout))(*[1.0] * len(eng.layout))
        assert eng.lib.afr_set_param_groups(eng._plan, ones, ones, len(eng.layout)) == _lib.AFR_ESTATE
    assert eng.param_group_ranges() == []
    # groups survive ensure_batch's re-planning: 300 rows > 64, and the step after it is still the grouped one
    eng.set_param_groups(lm, wm)
    table = eng.param_group_ranges()
    assert table == groups_ref.merged_ranges(cfg, lm, wm)
    twin = _engine(cfg, "f32", 300, lr_mult=lm, wd_mult=wm, ema_decay=0.9)
    eng.train_step(x, t, font=font, **_hyper())
    twin.train_step(x, t, font=font, **_hyper())
    assert eng.max_batch >= 300 and eng.param_group_ranges() == table
    assert_same_state(eng, twin, "re-planned", padding=True)
    eng.set_param_groups(None, None)
    assert eng.param_group_ranges() == []
    # thirty steps of glyph-small under the default rule lower the loss
    tr = _engine(cfg, "f32", x.shape[0], wd_mult={k: 0.0 for k in no_decay_names(cfg)})
    losses = []
    for _ in range(30):
        tr.train_step(x, t, font=font)
        losses.append(tr.read_loss())
    print(f"glyph-small, 30 AdamW steps, default no-decay rule: loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
