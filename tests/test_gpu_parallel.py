"""GPU (one card): the staged backward used for all-reduce overlap equals the monolithic one bit for bit, and the
data-parallel step path runs end to end over RCCL (backend "nccl", world size 1: the collective is an identity, the
stream/async-handle plumbing is the real one)."""
import os

import numpy as np
import pytest
import torch

from .opt_paths import rccl_world_one
from .util import GlyphConfig, glyph_inputs, synth

pytestmark = pytest.mark.gpu


def _glyph_engine(max_batch=512, dtype="f32"):
    from ai_font_renderer_amd.engine import Engine
    cfg = GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2)
    eng = Engine(cfg, dtype=dtype, max_batch=max_batch)
    eng.load_params(synth.make_params(cfg))
    return cfg, eng


@pytest.mark.parametrize("kind", ["glyph", "sheet", "pixel"])
def test_staged_backward_equals_monolithic_and_covers_the_buffer(kind):
    from ai_font_renderer_amd.engine import Engine
    from .util import SheetConfig
    if kind == "pixel":                                       # one stage per block; stage 0 also the head, the last one the tables
        from ai_font_renderer_amd.config import PixelConfig
        cfg = PixelConfig(out_h=4, out_w=6, d_model=128, heads=2, layers=3, ff_dim=200, n_fonts=2)
        eng = Engine(cfg, max_batch=16)
        eng.load_params(synth.make_params(cfg))
        assert eng.backward_stages == 3
        args = dict(x=torch.from_numpy((32 + (np.arange(11) * 7) % 95).astype(np.int64)), font=torch.from_numpy((np.arange(11) % 2).astype(np.int64)),
                    target=torch.from_numpy(synth.hash_u8(931, (11, 4, 6))))
    elif kind == "glyph":
        cfg, eng = _glyph_engine()
        x, font, t = glyph_inputs(cfg, 300)
        args = dict(x=torch.from_numpy(x), target=torch.from_numpy(t), font=torch.from_numpy(font))
    else:
        cfg = SheetConfig(max_length=24, sheet_h=16, sheet_w=40)
        eng = Engine(cfg, max_batch=64)
        eng.load_params(synth.make_params(cfg))
        args = dict(x=torch.from_numpy(synth.encode_strings(synth.dataset_strings(37), 24)),
                    target=torch.from_numpy(synth.synth_sheet_targets(37, 16, 40, tensor_id=930)), font=None)
    eng.train_step(args["x"], args["target"], font=args["font"], step=5, do_step=False)
    ref, lref = eng.flat_grads.clone(), eng.read_loss()
    eng.flat_grads.fill_(float("nan"))
    eng.forward_loss(args["x"], args["target"], font=args["font"], step=5)
    covered = torch.zeros(eng.n_flat, dtype=torch.bool)
    base = eng.flat_grads.data_ptr()
    for s in range(eng.backward_stages):
        v = eng.backward_stage(s)
        off = (v.data_ptr() - base) // 4
        assert not covered[off:off + v.numel()].any()
        covered[off:off + v.numel()] = True
        torch.cuda.synchronize()
        for name, shape, o, n in eng.layout:                   # every tensor inside the reported range is final now
            if off <= o and o + n <= off + v.numel():          # (alignment pads between tensors are never written)
                assert not torch.isnan(eng.flat_grads[o:o + n]).any(), (s, name)
    assert covered.all()
    assert eng.read_loss() == lref
    for name, shape, o, n in eng.layout:
        assert torch.equal(eng.flat_grads[o:o + n], ref[o:o + n]), name


@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped"])
def test_data_parallel_stepper_over_rccl_world1(schedule, monkeypatch):
    from ai_font_renderer_amd.parallel import DataParallelStepper
    # small models take one all-reduce after backward; the two-collective overlapped schedule is forced for the other case
    with rccl_world_one(schedule, monkeypatch) as dist:
        cfg, eng = _glyph_engine()
        x, font, t = glyph_inputs(cfg, 300)
        xt, ft, tt = torch.from_numpy(x).cuda(), torch.from_numpy(font).cuda(), torch.from_numpy(t).cuda()
        st = DataParallelStepper(eng, dist, world=2)          # force the multi-rank code path
        for _ in range(3):
            st.step(xt, tt, ft, mean_elems=300 * cfg.pixels)
        l_dp = st.global_loss()
        p_dp = eng.flat_params.clone()
        cfg2, eng2 = _glyph_engine()
        st2 = DataParallelStepper(eng2, None, 1)
        for _ in range(3):
            st2.step(xt, tt, ft, mean_elems=300 * cfg.pixels)
        assert st2.global_loss() == l_dp
        assert torch.equal(eng2.flat_params, p_dp)


def test_pixel_transformer_through_the_data_parallel_step(monkeypatch):
    """BASELINE configs[4]'s model (C5-mini, bf16) through the multi-rank code path with the overlapped schedule (stage 0's range
    reduced asynchronously while the other blocks' stages run) over a world of one: the parameters of the single-GPU step."""
    from ai_font_renderer_amd.config import C5_MINI as cfg
    from ai_font_renderer_amd.engine import Engine
    from ai_font_renderer_amd.parallel import DataParallelStepper
    with rccl_world_one("overlapped", monkeypatch) as dist:
        B = 24
        xt = torch.from_numpy((32 + (np.arange(B) * 11) % 95).astype(np.int64)).cuda()
        ft = torch.from_numpy((np.arange(B) % 2).astype(np.int64)).cuda()
        tt = torch.from_numpy(synth.hash_u8(932, (B, cfg.out_h, cfg.out_w))).cuda()
        res = []
        for world in (2, 1):
            eng = Engine(cfg, dtype="bf16", max_batch=B)
            eng.load_params(synth.make_params(cfg))
            st = DataParallelStepper(eng, dist if world > 1 else None, world=world)
            for _ in range(3):
                st.step(xt, tt, ft, mean_elems=B * cfg.pixels, lr=1e-5)
            res.append((st.global_loss(), eng.flat_params.clone()))
            del eng
        assert res[0][0] == res[1][0]
        assert torch.equal(res[0][1], res[1][1])


def test_accumulating_rank_through_the_data_parallel_step(monkeypatch):
    """A rank whose batch exceeds its micro-batch (Engine(micro_batch=m): gradient accumulation) takes the plain schedule --
    accumulate, one all-reduce of the summed gradient, AdamW -- whatever the overlap threshold says; world of one over RCCL,
    equal to the same engine stepping by itself."""
    from ai_font_renderer_amd.config import C5_MINI as cfg
    from ai_font_renderer_amd.engine import Engine
    from ai_font_renderer_amd.parallel import DataParallelStepper
    with rccl_world_one("overlapped", monkeypatch) as dist:
        B = 20
        xt = torch.from_numpy((32 + (np.arange(B) * 11) % 95).astype(np.int64)).cuda()
        ft = torch.from_numpy((np.arange(B) % 2).astype(np.int64)).cuda()
        tt = torch.from_numpy(synth.hash_u8(935, (B, cfg.out_h, cfg.out_w))).cuda()
        res = []
        for world in (2, 1):
            eng = Engine(cfg, dtype="bf16", max_batch=B, micro_batch=8)
            eng.load_params(synth.make_params(cfg))
            st = DataParallelStepper(eng, dist if world > 1 else None, world=world)
            for _ in range(2):
                st.step(xt, tt, ft, mean_elems=B * cfg.pixels, lr=1e-5)
            res.append((st.global_loss(), eng.flat_params.clone()))
            del eng
        assert res[0][0] == res[1][0]
        assert torch.equal(res[0][1], res[1][1])


def test_c4_per_gpu_shard_through_the_data_parallel_step():
    """BASELINE configs[3]: the per-GPU shard (C3 net, bf16, 8192 glyphs) through the multi-rank code path (materialised
    gradients -> RCCL all-reduce -> AdamW kernel) over a world of one: the same parameters as the fused single-GPU step
    (AdamW inside the slab reduction), bit for bit -- both apply the same adamw_elem to the same ordered slab sums."""
    import torch.distributed as dist
    from ai_font_renderer_amd.config import WORKLOADS
    from ai_font_renderer_amd.engine import Engine
    from ai_font_renderer_amd.parallel import DataParallelStepper
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        cfg, B = WORKLOADS["c3"]["cfg"], WORKLOADS["c3"]["batch"]
        x, font, t = glyph_inputs(cfg, B)
        xt, ft, tt = torch.from_numpy(x).cuda(), torch.from_numpy(font).cuda(), torch.from_numpy(t).cuda()
        res = []
        for world in (2, 1):                                  # 2: forced multi-rank path; 1: fused single-GPU step
            eng = Engine(cfg, dtype="bf16", max_batch=B)
            eng.load_params(synth.make_params(cfg))
            st = DataParallelStepper(eng, dist if world > 1 else None, world=world)
            for _ in range(3):
                st.step(xt, tt, ft, mean_elems=B * cfg.pixels)
            res.append((st.global_loss(), eng.flat_params.clone()))
            del eng
        assert res[0][0] == res[1][0]
        assert torch.equal(res[0][1], res[1][1])
    finally:
        dist.destroy_process_group()


def test_opt_in_bf16_gradient_exchange_tracks_the_exact_exchange(monkeypatch):
    """AFR_DP_GRAD_BF16=1 rounds each rank's gradient to bf16 for the all-reduce (throughput mode only): three steps stay
    within bf16 rounding of the exact-f32 exchange; the f32 engine ignores the switch."""
    import torch.distributed as dist
    from ai_font_renderer_amd import parallel
    from ai_font_renderer_amd.parallel import DataParallelStepper
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        outs = {}
        for flag in (False, True):
            monkeypatch.setattr(parallel, "GRAD_BF16", flag)
            cfg, eng = _glyph_engine(dtype="bf16")
            x, font, t = glyph_inputs(cfg, 300)
            xt, ft, tt = torch.from_numpy(x).cuda(), torch.from_numpy(font).cuda(), torch.from_numpy(t).cuda()
            st = DataParallelStepper(eng, dist, world=2)
            for _ in range(3):
                st.step(xt, tt, ft, mean_elems=300 * cfg.pixels)
            outs[flag] = eng.flat_params.clone()
        rel = float((outs[True] - outs[False]).norm() / outs[False].norm())
        assert 0 < rel < 2e-3, rel
        monkeypatch.setattr(parallel, "GRAD_BF16", True)
        cfg, eng = _glyph_engine(dtype="f32")
        st = DataParallelStepper(eng, dist, world=2)
        st.step(xt, tt, ft, mean_elems=300 * cfg.pixels)
        cfg2, eng2 = _glyph_engine(dtype="f32")
        DataParallelStepper(eng2, None, 1).step(xt, tt, ft, mean_elems=300 * cfg.pixels)
        assert torch.equal(eng.flat_params, eng2.flat_params)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind,dtype", [("glyph", "f32"), ("glyph", "bf16"), ("sheet", "f32"), ("sheet", "bf16")])
def test_sharded_optimizer_schedule_over_rccl_world1(kind, dtype, monkeypatch):
    """The sharded-optimizer schedule (opt-in, AFR_DP_SCHEDULE=shard; here shard-force so that it runs at a world of one):
    in-place RCCL reduce_scatter_tensor -> Engine.adamw_range (afr_op_adamw on an offset slice of p/g/m/v) -> in-place
    all_gather_into_tensor -> shadow re-sync.  Three steps give bit-identical parameters and moments to the replicated
    path (one all-reduce + afr_adamw_step), in both dtypes, for a glyph net and the mini sheet model."""
    import torch.distributed as dist
    from ai_font_renderer_amd.engine import Engine
    from ai_font_renderer_amd.parallel import DataParallelStepper
    from .util import MINI
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        def make():
            if kind == "glyph":
                cfg, eng = _glyph_engine(dtype=dtype)
                x, font, t = glyph_inputs(cfg, 300)
                return cfg, eng, torch.from_numpy(x).cuda(), torch.from_numpy(font).cuda(), torch.from_numpy(t).cuda(), 300
            eng = Engine(MINI, dtype=dtype, max_batch=64)
            eng.load_params(synth.make_params(MINI))
            x = torch.from_numpy(synth.encode_strings(synth.dataset_strings(37), MINI.max_length)).cuda()
            t = torch.from_numpy(synth.synth_sheet_targets(37, MINI.sheet_h, MINI.sheet_w, tensor_id=931)).cuda()
            return MINI, eng, x, None, t, 37
        out = {}
        for sched in ("shard-force", "replicated"):
            if sched == "shard-force":
                monkeypatch.setenv("AFR_DP_SCHEDULE", "shard-force")
            else:
                monkeypatch.delenv("AFR_DP_SCHEDULE", raising=False)
            cfg, eng, xt, ft, tt, B = make()
            st = DataParallelStepper(eng, dist, world=1 if sched == "shard-force" else 2)     # 2: forced multi-rank replicated path
            assert st.sharded() == (sched == "shard-force")
            for i in range(3):
                st.step(xt, tt, ft, mean_elems=B * cfg.pixels, step=i + 1)
            y = eng.forward(xt, ft)                      # reads the bf16 shadow in bf16 mode: it was re-synced
            out[sched] = (st.global_loss(), eng.flat_params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), y.clone())
        a, b = out["shard-force"], out["replicated"]
        assert a[0] == b[0]
        for u, v in zip(a[1:], b[1:]):
            assert torch.equal(u, v)
    finally:
        dist.destroy_process_group()
