"""CPU: the restatements of the evaluation kernel (tests/eval_ref.py) hold the bounds the GPU tests use, planted faults miss
them by 10x or more, the 8-bit level of float targets is helpers.targets_as_uint8's, the entry points refuse bad calls on the
host, and AFR_VAL_REPORT is parsed strictly and changes nothing when unset."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import eval_ref as R

COLS = (8, 64, 504, 512, 520, 2040, 2048, 2056, 4096, 19200)


def _case(cols, rows=5, seed=0, u8=True):
    g = np.random.default_rng(seed + cols)
    u = g.uniform(-0.5, 1.5, (rows, cols)).astype(np.float32)
    k = g.integers(0, 256, (2 * rows, cols), dtype=np.uint8)
    rowmap = np.array([(2 * rows - 1 - r) // 2 * 2 for r in range(rows)], dtype=np.int32)      # reversed, with duplicates
    return u, (k if u8 else k.astype(np.float32) / np.float32(255.0)), rowmap


def test_chain_depth_follows_the_documented_order():
    assert [R.chain_depth(c) for c in (8, 512, 520, 2048, 2056, 19200)] == [14, 14, 22, 38, 25, 89]
    assert R.lanes(2048) == 64 and R.lanes(2056) == 256


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("u8", [True, False])
def test_float32_order_is_within_the_mse_bound_of_fp64(cols, u8):
    u, tgt, rowmap = _case(cols, u8=u8)
    for rm in (None, rowmap):
        want = R.loss_rows64(u, tgt, "mse", rm)
        got = R.loss_rows32(u, tgt, "mse", rm).astype(np.float64)
        bound = R.mse_bound(cols, want)            # want = sum_i term_i / cols
        assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()


@pytest.mark.parametrize("cols", (64, 520, 2056, 19200))
@pytest.mark.parametrize("fault", ["fault_drop_last_group", "fault_div256", "fault_no_div", "fault_ignore_rowmap"])
def test_planted_loss_faults_miss_the_bound_tenfold(cols, fault):
    u, tgt, rowmap = _case(cols)
    want = R.loss_rows64(u, tgt, "mse", rowmap)
    got = R.loss_rows32(u, tgt, "mse", rowmap, **{fault: True}).astype(np.float64)
    assert (np.abs(got - want) / R.mse_bound(cols, want)).max() >= 10.0


def test_planted_level_faults_are_seen_by_the_exact_comparisons():
    """q and stats are compared exactly (no mismatch allowed): rounding instead of truncation, and d > 2 for d >= 2, each
    change far more than ten values."""
    u, tgt, _ = _case(2048)
    q = R.q64(u, "mse")
    assert np.array_equal(q, (np.clip(u, 0, 1) * np.float32(255)).astype(np.uint8))          # the truncating dump, quirk Q7
    assert (R.q64(u, "mse", fault_round=True) != q).sum() >= 10 * 10
    t8 = R.t8_of(tgt[:5])
    d = np.abs(q - t8)
    good, bad = R.stats_of(q, t8), R.stats_of(q, t8, fault_gt2=True)
    assert np.array_equal(good[:, 1], (d >= 2).sum(1)) and (good[:, 1] - bad[:, 1]).sum() == (d == 2).sum() >= 10
    assert np.array_equal(good[:, 0], (d >= 1).sum(1)) and np.array_equal(good[:, 2], d.max(1))
    assert np.array_equal(good[:, 3], ((q >= 128) != (t8 >= 128)).sum(1))


def test_nan_gives_level_zero_and_a_nan_row_only():
    u, tgt, _ = _case(64)
    u[2, 17] = np.nan
    for loss in ("mse", "bce"):
        assert R.q64(u, loss)[2, 17] == 0
        l64, l32 = R.loss_rows64(u, tgt[:5], loss), R.loss_rows32(u, tgt[:5], loss)
        assert np.isnan(l64[2]) and np.isnan(l32[2]) and np.isfinite(np.delete(l64, 2)).all() and np.isfinite(np.delete(l32, 2)).all()


def test_t8_of_float_targets_is_targets_as_uint8():
    from ai_font_renderer_amd import helpers
    k = np.arange(256, dtype=np.uint8).repeat(3).reshape(4, -1)
    t = torch.from_numpy(k.astype(np.float32) / np.float32(255.0))
    assert torch.equal(helpers.targets_as_uint8(t), torch.from_numpy(k))
    assert np.array_equal(R.t8_of(t.numpy()), k.astype(np.int64))
    assert np.array_equal(R.t8_of(k), k.astype(np.int64))
    assert R.t8_of(np.array([[-0.3, 1.7, 0.5, np.nan]], np.float32)).tolist() == [[0, 255, 128, 0]]      # limited to 0..255; 127.5 -> 128 (even)


def test_entry_points_refuse_bad_calls_on_the_host():
    """Fake non-null pointers: nothing is launched."""
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    EI, ES, EU = _lib.AFR_EINVAL, _lib.AFR_ESTATE, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)
    ok = dict(ad=0, lk=0, u=fk, t=fk, td=0, rm=None, rows=4, cols=64, lr=fk, st=fk, q=fk)

    def op(**kw):
        a = {**ok, **kw}
        return lib.afr_op_eval(a["ad"], a["lk"], a["u"], a["t"], a["td"], a["rm"], a["rows"], a["cols"], a["lr"], a["st"], a["q"], None)

    assert op(cols=12) == EU and b"multiple of 8" in lib.afr_last_error()
    assert op(t=None, lr=None) == EI and b"target" in lib.afr_last_error()            # a NULL target with stats
    assert op(t=None, st=None) == EI                                                 # ... with loss_rows
    assert op(lr=None, st=None, q=None) == EI and b"all NULL" in lib.afr_last_error()
    assert op(td=7) == EI and op(u=None) == EI and op(ad=2) == EI and op(lk=5) == EI and op(rows=0) == EI and op(cols=0) == EI
    assert op(st=C.c_void_p(0x1008)) == EI and op(q=C.c_void_p(0x1004)) == EI and b"aligned" in lib.afr_last_error()
    # the plan entries: an unbound plan is AFR_ESTATE; afr_eval_rows without a data set likewise
    c = make_afr_config(config.SheetConfig(max_length=10, sheet_h=8, sheet_w=24), "f32", 8)
    plan = C.c_void_p()
    _lib.check(lib.afr_plan_create(C.byref(c), C.byref(plan)))
    assert lib.afr_eval(plan, fk, 0, 4, fk, fk, fk, None) == ES
    assert lib.afr_eval_rows(plan, fk, 4, fk, fk, fk, None) == ES and b"data set" in lib.afr_last_error()
    assert lib.afr_eval_rows(plan, fk, 4, None, None, None, None) == EI
    lib.afr_plan_destroy(plan)


def test_val_report_setting_is_parsed_strictly(monkeypatch):
    from ai_font_renderer_amd import model as M
    for spec, want in (("", None), ("  ", None), ("1", 1), (" 12 ", 12)):
        monkeypatch.setenv("AFR_VAL_REPORT", spec)
        assert M._val_report_from_env() == want
    monkeypatch.delenv("AFR_VAL_REPORT")
    assert M._val_report_from_env() is None
    for spec in ("0", "-2", "2.5", "two", "1:2"):
        monkeypatch.setenv("AFR_VAL_REPORT", spec)
        with pytest.raises(ValueError, match="AFR_VAL_REPORT"):
            M._val_report_from_env()


class _Recorder:
    """Stands in for the model, its engine and the stepper: every method call is recorded by name, evaluate_last's keyword arguments
    are kept in eval_kwargs."""

    def __init__(self, calls, **attrs):
        self.__dict__.update(attrs)
        self._calls, self.eval_kwargs = calls, []

    def __getattr__(self, name):
        def call(*a, **k):
            self._calls.append(name)
            if name == "evaluate_last":
                self.eval_kwargs.append(k)
            return _EVAL if name == "evaluate_last" else 0.0
        return call


class _Eval:
    loss_rows = torch.tensor([0.25, 0.5])
    stats = torch.tensor([[3, 1, 2, 0], [5, 0, 1, 1]])
    u8 = None


_EVAL = _Eval()


def test_run_epoch_makes_no_new_call_when_the_report_is_off():
    from ai_font_renderer_amd import model as M
    calls = []
    eng = _Recorder(calls, ema_decay=None, optimizer="adamw")
    model = _Recorder(calls, engine=eng)
    inputs, targets = torch.zeros(10, 4, dtype=torch.int64), torch.zeros(10, 2, 4, dtype=torch.uint8)

    def run(**kw):
        del calls[:]
        M._run_epoch(model, _Recorder(calls), M._EpochOrder(10), inputs, targets, 4, 1e-3, 0, 1, **kw)
        return [c for c in calls if c not in ("train", "eval", "_next_step")]

    off = run()
    assert off == ["step_rows"] * 2 + ["global_loss"] + ["forward_rows", "loss_grad_rows"] + ["global_loss"]
    assert run(by_rows=False) == ["step"] * 2 + ["global_loss"] + ["forward", "loss_grad"] + ["global_loss"]
    rep = M._ValReport(2, "cpu")
    on = run(reports=[rep])
    assert on == ["step_rows"] * 2 + ["global_loss"] + ["forward_rows", "evaluate_last", "loss_grad_rows"] + ["global_loss"]
    # the accumulator: column sums, maximum, the two largest losses with the data-set indices of the validation rows
    assert rep.sums.tolist() == [8, 1, 1, 2] and int(rep.max) == 2
    assert rep.loss.tolist() == [0.5, 0.25]
    vidx = M._EpochOrder(10).val_idx
    assert rep.idx.tolist() == [int(vidx[1]), int(vidx[0])]
    line = rep.line(8)
    assert line.startswith("Val report: off by >= 1 level 0.500000, off by >= 2 levels 0.062500, wrong ink 0.062500, max level diff 2, worst 2: ")
    assert line.endswith(f"{int(vidx[1])}(0.500000), {int(vidx[0])}(0.250000)")
    # two reports that take batches still share one evaluation per batch, with bitmaps exactly when one of them reads bitmaps
    fed = []

    class Taker(M._Report):
        takes_batches = True

        def __init__(self, needs_u8):
            self.needs_u8 = needs_u8

        def add(self, res, rows):
            fed.append((self, res, rows.tolist()))

    for flags in ((False, False), (False, True), (True, False), (True, True)):
        takers = [Taker(f) for f in flags]
        del eng.eval_kwargs[:], fed[:]
        assert run(reports=[M._Report()] + takers) == on
        assert [k["want_u8"] for k in eng.eval_kwargs] == [any(flags)]
        assert [(t, r) for t, r, _ in fed] == [(takers[0], _EVAL), (takers[1], _EVAL)] and fed[0][2] == fed[1][2] == vidx.tolist()
    del eng.eval_kwargs[:]
    assert run(reports=[M._Report()]) == off and eng.eval_kwargs == []      # a report that takes no batches asks for no evaluation
