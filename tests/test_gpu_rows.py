"""GPU: training from an HBM-resident data set by row index (afr_bind_dataset + afr_*_rows; Engine.bind_dataset and the
*_rows methods; DataParallelStepper.step_rows; the training loop).

A call by rows does the arithmetic of the dense call on the gathered rows, in the same order on the same values: the
comparisons against gather-then-call are BITWISE (torch.equal), for every plan kind, every dtype and every loss path (the
loss kernel, the f32 / bf16x3 tile epilogue, the bf16 ring epilogue's early uint8 and late float32 target forms, the fused
small-net step).  One test anchors the path to the reference's own golden numbers instead of to the code under test."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from . import opt_paths as OP
from .opt_paths import no_error_bits_left_behind  # noqa: F401
from .util import MINI, R0, GlyphConfig, SheetConfig, load, maxabs, synth

pytestmark = pytest.mark.gpu


def _engine(cfg, dtype="f32", max_batch=64, **kw):
    return OP.engine(cfg, dtype, max_batch, load=False, **kw)


def _pair(cfg, dtype, max_batch, **kw):
    """Two engines holding the same parameters: one is driven by rows, the other by gathered tensors."""
    a, b = OP.engine(cfg, dtype, max_batch, **kw), _engine(cfg, dtype, max_batch, **kw)
    b.flat_params.copy_(a.flat_params)
    b.sync_params()
    return a, b


def _rows_with_duplicates(n_rows, B, seed):
    """A seeded permutation slice in which every eighth entry repeats the one seven before it."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randperm(n_rows, generator=g)
    r = r[torch.arange(B) % n_rows].clone()
    dst = r[7::8]
    r[7::8] = r[0::8][:dst.numel()]
    assert r.unique().numel() < B
    return r


def _sheet_dataset(n, L, h, w, tid):
    x = synth.encode_strings(synth.dataset_strings(n), L)
    return torch.from_numpy(x).cuda(), torch.from_numpy(synth.synth_sheet_targets(n, h, w, tensor_id=tid)).cuda(), None


def _glyph_dataset(cfg, n, tid, float_targets=False):
    i = np.arange(n)
    x = torch.from_numpy((32 + (i * 7) % 95).astype(np.int64)).cuda()
    font = torch.from_numpy(((i // 3) % cfg.n_fonts).astype(np.int64)).cuda() if cfg.n_fonts > 0 else None
    t = torch.from_numpy(synth.hash_u8(tid, (n, cfg.out_h, cfg.out_w))).cuda()
    if float_targets:
        t = t.float() / 255.0
    return x, t, font


def _gather(ds, rows):
    x, t, font = ds
    r = rows.to(x.device)
    return x[r].contiguous(), t[r].contiguous(), None if font is None else font[r].contiguous()


def _same(a, b, what):
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} elements differ"


def _check_rows_equal_gather(cfg, dtype, ds, rows, max_batch, step=None, **kw):
    """Every call by rows against its dense twin on the gathered rows, bitwise; error word clean throughout."""
    er, ed = _pair(cfg, dtype, max_batch, **kw)
    er.bind_dataset(ds[0], ds[1], ds[2])
    x, t, font = _gather(ds, rows)
    st = dict(step=step) if step is not None else {}
    # forward (inference and, for the model with dropout, training masks keyed by the in-batch row)
    _same(er.forward_rows(rows), ed.forward(x, font), "forward")
    if step is not None:
        _same(er.forward_rows(rows, training=True, step=step), ed.forward(x, font, training=True, step=step), "training forward")
    # forward + loss kernel + monolithic backward
    er.forward_rows(rows, training=True, step=step or 0, want_output=False)
    er.loss_grad_rows(rows)
    er.backward()
    ed.forward(x, font, training=True, step=step or 0, want_output=False)
    ed.loss_grad(t)
    ed.backward()
    _same(er.loss_accum, ed.loss_accum, "loss of forward + loss_grad")
    _same(er.flat_grads, ed.flat_grads, "gradients of forward + loss_grad + backward")
    # fused-loss forward + the backward stages in order
    er.forward_loss_rows(rows, **st)
    ed.forward_loss(x, t, font=font, **st)
    for s in range(er.backward_stages):
        er.backward_stage(s)
        ed.backward_stage(s)
    _same(er.loss_accum, ed.loss_accum, "loss of forward_loss")
    _same(er.flat_grads, ed.flat_grads, "gradients of forward_loss + backward stages")
    # a whole step without the optimizer: the gradients
    er.train_step_rows(rows, do_step=False, **st)
    ed.train_step(x, t, font=font, do_step=False, **st)
    _same(er.loss_accum, ed.loss_accum, "loss of train_step(do_step=False)")
    _same(er.flat_grads, ed.flat_grads, "gradients of train_step(do_step=False)")
    # three optimizer steps
    for i in range(3):
        er.train_step_rows(rows, **st)
        ed.train_step(x, t, font=font, **st)
        _same(er.loss_accum, ed.loss_accum, f"loss after step {i + 1}")
    _same(er.flat_params, ed.flat_params, "parameters after three steps")
    _same(er.exp_avg, ed.exp_avg, "exp_avg after three steps")
    _same(er.exp_avg_sq, ed.exp_avg_sq, "exp_avg_sq after three steps")
    assert er.t == ed.t == 3
    assert float(er.loss_accum.item()) > 0.0 and bool(torch.isfinite(er.flat_params).all())
    assert er.error_flags() == 0 and ed.error_flags() == 0
    return er, ed


# ----------------------------------------------------------------------------- 1. by rows == gather-then-call
def test_sheet_mini_with_dropout_by_rows_equals_gather():
    ds = _sheet_dataset(200, 10, 8, 24, 940)
    _check_rows_equal_gather(MINI, "f32", ds, _rows_with_duplicates(200, 24, 1), 32, step=7)


@pytest.mark.parametrize("L,dtype", [(37, "bf16"), (120, "f32")])
def test_sheet_r0_short_and_over_long_rows_by_rows_equals_gather(L, dtype):
    """A data set narrower than max_length (zero-pad branch) and one wider (truncate branch), B = 33 (ragged tiles)."""
    ds = _sheet_dataset(150, L, 80, 240, 941)
    _check_rows_equal_gather(R0, dtype, ds, _rows_with_duplicates(150, 33, 2), 33, step=7)


def test_glyph_c1_fused_small_net_f32_by_rows_equals_gather():
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c1"]["cfg"]
    ds = _glyph_dataset(cfg, 300, 942)
    _check_rows_equal_gather(cfg, "f32", ds, _rows_with_duplicates(300, 95, 3), 95)


def test_glyph_c2_fused_small_net_bf16_by_rows_equals_gather():
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c2"]["cfg"]
    ds = _glyph_dataset(cfg, 300, 943)
    _check_rows_equal_gather(cfg, "bf16", ds, _rows_with_duplicates(300, 4096, 4), 4096)


@pytest.mark.parametrize("dtype,float_targets", [("bf16", False), ("f32", False), ("bf16x3", False), ("bf16", True)])
def test_glyph_c3_by_rows_equals_gather(dtype, float_targets):
    """B = 8192: bf16 = combination table + the ring epilogue's early uint8 target request (float32 targets: its late form);
    f32 and bf16x3 = the 128x128 tile epilogue."""
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c3"]["cfg"]
    ds = _glyph_dataset(cfg, 380, 944, float_targets)
    assert ds[1].dtype == (torch.float32 if float_targets else torch.uint8)
    _check_rows_equal_gather(cfg, dtype, ds, _rows_with_duplicates(380, 8192, 5), 8192)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pixel_c5_mini_with_fonts_by_rows_equals_gather(dtype):
    from ai_font_renderer_amd.config import C5_MINI as cfg
    ds = _glyph_dataset(cfg, 200, 945)
    _check_rows_equal_gather(cfg, dtype, ds, _rows_with_duplicates(200, 12, 6), 12)


# ----------------------------------------------------------------------------- 2. anchored to the reference
def test_scattered_golden_rows_match_the_reference():
    """The rows of sheet_mini.npz at scattered positions of a larger data set of hashed filler: on those positions a step by
    rows gives the reference's loss, gradients and three AdamW steps, within the bounds the dense path is held to
    (test_mini_train_grads_match_reference_without_dropout, test_mini_three_adamw_steps_match_reference)."""
    fx = load("sheet_mini.npz")
    cfg = replace(MINI, p_embed=0.0, p_attn=0.0, p_fc=0.0)
    N, pos = 211, [190, 3, 77, 210, 42]
    x = 32 + (synth.hash_u8(946, (N, 10)).astype(np.int64) % 95)
    t = synth.hash_u8(947, (N, 8, 24))
    x[pos], t[pos] = fx["x10"], fx["target_u8"]
    eng = _engine(cfg, "f32", 8)
    eng.load_params(synth.make_params(cfg))
    eng.bind_dataset(torch.from_numpy(x), torch.from_numpy(t))
    rows = torch.tensor(pos)
    eng.train_step_rows(rows, do_step=False)
    assert abs(eng.read_loss() - float(fx["nodrop_loss"])) < 2e-6
    for k, g in eng.grads.items():
        ref = np.asarray(fx["nodrop_grad/" + k], dtype=np.float64)
        assert maxabs(g.cpu().numpy(), ref) / max(1e-7, float(np.abs(ref).max())) < 1e-4, k
    for i in range(3):
        eng.train_step_rows(rows)
        assert abs(eng.read_loss() - float(fx["adamw_losses"][i])) < 3e-6
    E = MINI.embed_dim
    for k, v in eng.state_dict().items():
        got, ref = v.cpu().numpy(), fx["adamw_param/" + k]
        if k == "attention.in_proj_bias":     # k-bias gradient is analytically 0: Adam amplifies rounding noise
            got, ref = np.delete(got, np.s_[E:2 * E]), np.delete(ref, np.s_[E:2 * E])
        assert maxabs(got, ref) < 2e-5, k
    assert eng.error_flags() == 0


# ----------------------------------------------------------------------------- 3. targets beyond 2 GiB
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_target_rows_beyond_2_gib(dtype):
    """A uint8 target buffer of 115 000 sheets (2.2 GB, filled on the device): 8 rows from its last thousand are addressed
    with 64-bit arithmetic: their byte offsets do not fit a signed 32-bit integer or a buffer descriptor's 2 GiB range."""
    cfg = SheetConfig(max_length=10)
    N, pix = 115000, cfg.pixels
    assert N * pix > (1 << 31)
    t = torch.empty(N, pix, dtype=torch.uint8, device="cuda")
    i = torch.arange(pix, device="cuda", dtype=torch.int64)
    for lo in range(0, N, 5000):                                            # pixel (r, i) = a hash of both: every row differs
        r = torch.arange(lo, min(N, lo + 5000), device="cuda", dtype=torch.int64)[:, None]
        t[lo:lo + r.shape[0]] = (((r * 2654435761 + i * 40503 + (r * i) % 8191) >> 7) & 0xFF).to(torch.uint8)
    x = torch.from_numpy(32 + (synth.hash_u8(948, (N, 10)).astype(np.int64) % 95)).cuda()
    rows = N - 1000 + torch.tensor([999, 0, 512, 37, 998, 640, 3, 999])
    assert int(rows.min()) * pix > (1 << 31)
    assert t[rows[:7].cuda()].unique(dim=0).shape[0] == 7                   # distinct rows hold distinct sheets
    _check_rows_equal_gather(cfg, dtype, (x, t, None), rows, 8, step=3)


# ----------------------------------------------------------------------------- 4. bad indices, unbound engine, regrown plan
def test_out_of_range_row_sets_bit_2_and_is_clamped():
    ds = _sheet_dataset(50, 10, 8, 24, 949)
    er, ed = _pair(MINI, "f32", 8)
    er.bind_dataset(*ds[:2])
    rows = torch.tensor([4, 50, 9, -1, 0, 49])              # n_rows and -1: one past either end
    er.train_step_rows(rows, step=2, do_step=False)
    assert er.error_flags() == 4                            # bit 2, no other bit; reading clears
    # the step ran on the clamped rows
    x, t, _ = _gather(ds, torch.tensor([4, 49, 9, 0, 0, 49]))
    ed.train_step(x, t, step=2, do_step=False)
    _same(er.flat_grads, ed.flat_grads, "gradients on the clamped rows")
    er.train_step_rows(torch.tensor([4, 49, 9, 0]), step=2, do_step=False)
    assert er.error_flags() == 0                            # the next clean step reads 0
    er.forward_rows(torch.tensor([0, 50]))
    assert er.error_flags() == 4
    er.forward_rows(torch.tensor([0, 1]))
    er.loss_grad_rows(torch.tensor([0, -7]))
    assert er.error_flags() == 4


def test_rows_without_a_data_set_raise_and_a_regrown_plan_stays_bound():
    import ctypes as C
    from ai_font_renderer_amd._lib import AfrError
    eng = _engine(MINI, "f32", 8)
    eng.load_params(synth.make_params(MINI))
    rows = torch.arange(4)
    for call in (lambda: eng.forward_rows(rows), lambda: eng.loss_grad_rows(rows), lambda: eng.forward_loss_rows(rows),
                 lambda: eng.train_step_rows(rows)):
        with pytest.raises(AfrError, match="data set"):
            call()
    # the C entry point itself, on the engine's bound plan
    dev_rows = rows.cuda()
    rc = eng.lib.afr_train_step_rows(eng._plan, C.c_void_p(dev_rows.data_ptr()), 4, 4 * 192, C.c_void_p(eng.loss_accum.data_ptr()), 1, 0,
                                     1e-3, 0.9, 0.99, 1e-8, 5e-4, 1, None)
    assert rc == -2 and b"data set" in eng.lib.afr_last_error()
    # bound; then a batch larger than max_batch re-creates the plan, which is bound again
    ds = _sheet_dataset(60, 10, 8, 24, 950)
    er, ed = _pair(MINI, "f32", 8)
    er.bind_dataset(*ds[:2])
    er.train_step_rows(torch.arange(8), step=1)
    ed.train_step(*_gather(ds, torch.arange(8))[:2], step=1)
    big = _rows_with_duplicates(60, 40, 8)
    assert er.max_batch == 8
    er.train_step_rows(big, step=2)
    assert er.max_batch == 40
    x, t, _ = _gather(ds, big)
    ed.train_step(x, t, step=2)
    _same(er.loss_accum, ed.loss_accum, "loss after the plan grew")
    _same(er.flat_params, ed.flat_params, "parameters after the plan grew")
    assert er.error_flags() == 0


# ----------------------------------------------------------------------------- 5. accumulation and data parallel
def test_micro_batch_accumulation_by_rows_equals_gather():
    from ai_font_renderer_amd.config import PixelConfig
    cfg = PixelConfig(out_h=4, out_w=6, d_model=128, heads=2, layers=2, ff_dim=200, n_fonts=2)
    ds = _glyph_dataset(cfg, 150, 951)
    er, ed = _pair(cfg, "f32", 80, micro_batch=32)
    assert er.max_batch == 32
    er.bind_dataset(*ds)
    rows = _rows_with_duplicates(150, 80, 9)
    x, t, font = _gather(ds, rows)
    er.train_step_rows(rows, do_step=False)
    ed.train_step(x, t, font=font, do_step=False)
    _same(er.flat_grads, ed.flat_grads, "accumulated gradients")
    for _ in range(2):
        er.train_step_rows(rows, lr=1e-4)
        ed.train_step(x, t, font=font, lr=1e-4)
    _same(er.loss_accum, ed.loss_accum, "loss")
    _same(er.flat_params, ed.flat_params, "parameters")
    _same(er.forward_rows(rows), ed.forward(x, font), "forward of 80 rows, 32 at a time")
    assert er.error_flags() == 0


@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped"])
def test_step_rows_over_rccl_world1_equals_step_on_gathered_tensors(schedule, monkeypatch):
    from ai_font_renderer_amd.parallel import DataParallelStepper
    with OP.rccl_world_one(schedule, monkeypatch) as dist:
        cfg = GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2)
        ds = _glyph_dataset(cfg, 400, 952)
        er, ed = _pair(cfg, "f32", 512)
        er.bind_dataset(*ds)
        rows = _rows_with_duplicates(400, 300, 10).cuda()
        x, t, font = _gather(ds, rows)
        sr, sd = DataParallelStepper(er, dist, world=2), DataParallelStepper(ed, dist, world=2)      # the multi-rank code path
        for _ in range(3):
            sr.step_rows(rows, mean_elems=300 * cfg.pixels)
            sd.step(x, t, font, mean_elems=300 * cfg.pixels)
        assert sr.global_loss() == sd.global_loss()
        _same(er.flat_params, ed.flat_params, "parameters")
        _same(er.exp_avg_sq, ed.exp_avg_sq, "exp_avg_sq")
        one = _pair(cfg, "f32", 512)[0]                                                                # a world of one: the engine's own step
        one.bind_dataset(*ds)
        s1 = DataParallelStepper(one, None, 1)
        for _ in range(3):
            s1.step_rows(rows, mean_elems=300 * cfg.pixels)
        _same(one.flat_params, ed.flat_params, "parameters of the single-process step by rows")


# ----------------------------------------------------------------------------- 6. the loop no longer gathers
def test_training_loop_never_index_selects_the_data_set(tmp_path, monkeypatch):
    """train_attention_model on the 80 sheets of train_loop.npz (run a, set up as
    test_training_loop_replays_the_references_own_trajectory does): torch.Tensor.index_select is never called on the resident
    inputs / targets, every step and every validation pass goes by rows, and the trajectory is the golden one."""
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.engine import Engine
    fx = load("train_loop.npz")
    sched_pat, stop_pat, n_epochs = (int(v) for v in fx["a/patience"])
    monkeypatch.chdir(tmp_path)
    for k, v in dict(NUM_EPOCHS=n_epochs, LEARNING_RATE=float(fx["a/lrs"][0]), SCHEDULER_PATIENCE=sched_pat, EARLY_STOPPING_PATIENCE=stop_pat,
                     OUTPUT_DIR="loop_out", SHEET_HEIGHT=8, SHEET_WIDTH=24, MAX_CHARS_PER_SHEET=10).items():
        monkeypatch.setattr(M, k, v)
    m = M.AttentionFontRenderer(max_length=10, max_batch=16, init=False)
    m.engine = Engine(replace(m.config, p_embed=0.0, p_attn=0.0, p_fc=0.0), dtype="f32", max_batch=16, device=M.device)
    m.engine.load_params(synth.make_params(MINI))
    ds = torch.utils.data.TensorDataset(torch.from_numpy(fx["a/x"]), torch.from_numpy(fx["a/target_u8"].astype(np.float32) / 255.0))
    seen = dict(gathers=0, on_dataset=0, by_rows=0, val_by_rows=0, dense=0)
    orig_select = torch.Tensor.index_select

    def counting_select(self, *a, **k):
        seen["gathers"] += 1
        if self.is_cuda and self.shape[0] == 80 and tuple(self.shape[1:]) in ((10,), (8, 24), (192,)):
            seen["on_dataset"] += 1
        return orig_select(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "index_select", counting_select)

    def counted(orig, key):
        def f(self, *a, **k):
            seen[key] += 1
            return orig(self, *a, **k)
        return f

    for name, key in (("train_step_rows", "by_rows"), ("forward_loss_rows", "by_rows"), ("loss_grad_rows", "val_by_rows"),
                      ("train_step", "dense"), ("forward_loss", "dense"), ("loss_grad", "dense")):
        monkeypatch.setattr(Engine, name, counted(getattr(Engine, name), key))
    vals = []
    Sched = torch.optim.lr_scheduler.ReduceLROnPlateau
    orig_step = Sched.step

    def sched_step(self, metrics, *a, **k):
        vals.append(float(metrics))
        return orig_step(self, metrics, *a, **k)

    monkeypatch.setattr(Sched, "step", sched_step)
    M.train_attention_model(m, ds, 16)
    assert seen["on_dataset"] == 0 and seen["dense"] == 0, seen
    epochs = len(vals)
    assert epochs == len(fx["a/val_losses"])
    assert seen["by_rows"] == epochs * 4 and seen["val_by_rows"] == epochs, seen      # 64 training rows / 16, 16 validation rows / 16
    assert np.abs(np.array(vals) / fx["a/val_losses"] - 1).max() < 1e-4
