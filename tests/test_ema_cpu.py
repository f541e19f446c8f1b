"""CPU: the weight EMA's reference arithmetic, the host-only validation of afr_set_ema / afr_ema_update / afr_use_ema, and where the
data-parallel stepper counts an optimizer step for the EMA (two ranks over gloo, a stand-in engine that records its calls)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import ema_ref
from .util import ROOT, MINI


def test_ema_step_reproduces_the_closed_form_for_constant_parameters():
    gen = torch.Generator().manual_seed(3)
    p, e0 = torch.randn(257, generator=gen), torch.randn(257, generator=gen)
    for decay in (0.999, 0.5, 0.9):
        assert ema_ref.alpha32(decay) == float(torch.tensor(1.0) - torch.tensor(decay))          # the f32 difference, not 1 - decay in fp64
        e = e0.double()
        for k in range(1, 41):
            e = ema_ref.ema_step(e, p, decay)
            want = ema_ref.closed_form(e0, p, decay, k)
            assert float((e - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), (decay, k)
    assert torch.equal(ema_ref.ema_step(p, p, 0.999), p.double())                                 # p == e stays put
    p, e, same = ema_ref.mixed(4096, 1)
    assert int(same.sum()) == 512 and torch.equal(p[same], e[same]) and not bool((p[~same] == e[~same]).any())


def _plan(lib, cfg=MINI, dtype="f32"):
    from ai_font_renderer_amd import _lib
    from ai_font_renderer_amd.engine import make_afr_config
    c = make_afr_config(cfg, dtype, 8)
    plan = C.c_void_p()
    _lib.check(lib.afr_plan_create(C.byref(c), C.byref(plan)))
    return plan


def test_set_ema_validates_its_numbers_before_the_pointer_on_a_host_only_plan():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    plan = _plan(lib)
    fake = C.c_void_p(0x10000)                      # never dereferenced: the numbers are refused first
    try:
        for decay in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
            assert lib.afr_set_ema(plan, fake, decay, 1) == _lib.AFR_EINVAL, decay
            assert b"decay" in lib.afr_last_error(), decay
        for every in (0, -1):
            assert lib.afr_set_ema(plan, fake, 0.999, every) == _lib.AFR_EINVAL, every
            assert b"interval" in lib.afr_last_error(), every
        # nothing was set by the refused calls
        assert lib.afr_ema_update(plan, None, None) == _lib.AFR_ESTATE and b"no EMA" in lib.afr_last_error()
        assert lib.afr_use_ema(plan, 1, None) == _lib.AFR_ESTATE and b"no EMA" in lib.afr_last_error()
        assert lib.afr_use_ema(plan, 0, None) == _lib.AFR_OK                  # already off: a no-op
        assert lib.afr_set_ema(plan, None, float("nan"), -5) == _lib.AFR_OK   # off: decay and every are ignored
        assert lib.afr_set_ema(None, fake, 0.5, 1) == _lib.AFR_EINVAL
        # the slice op checks its numbers first too
        assert lib.afr_op_ema(fake, fake, 6, 0.5, None, None) == _lib.AFR_EINVAL and b"multiple of 4" in lib.afr_last_error()
        assert lib.afr_op_ema(fake, fake, 8, 1.0, None, None) == _lib.AFR_EINVAL and b"decay" in lib.afr_last_error()
        assert lib.afr_op_ema(None, fake, 8, 0.5, None, None) == _lib.AFR_EINVAL
    finally:
        lib.afr_plan_destroy(plan)


def test_engine_and_facade_refuse_bad_ema_settings_without_a_gpu(monkeypatch):
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.engine import Engine
    for decay, every in ((0.0, 1), (1.0, 1), (2.0, 1), (float("nan"), 1), (0.9, 0), (0.9, -1), (0.9, 1.5)):
        with pytest.raises(ValueError):
            Engine._check_ema(decay, every)
    assert Engine._check_ema(None, 7) == (None, 1) and Engine._check_ema(0.9, 2) == (0.9, 2)
    monkeypatch.delenv("AFR_EMA", raising=False)
    assert M._ema_from_env() == (None, 1)
    monkeypatch.setenv("AFR_EMA", "0.999")
    assert M._ema_from_env() == (0.999, 1)
    monkeypatch.setenv("AFR_EMA", "0.9:2")
    assert M._ema_from_env() == (0.9, 2)
    for bad in ("abc", "0.9:x", "0.9:2:3"):
        monkeypatch.setenv("AFR_EMA", bad)
        with pytest.raises(ValueError):
            M._ema_from_env()


# ----------------------------------------------------------------------------- the data-parallel stepper, two ranks over gloo
class RecordingEngine:
    """What DataParallelStepper needs of an engine, with every call that matters here appended to `log`."""
    N = 256

    def __init__(self, rank, ema, clip):
        self.flat_params = torch.zeros(self.N)
        self.flat_grads = torch.zeros(self.N)
        self.loss_accum = torch.zeros(1)
        self.backward_stages = 2
        self.max_grad_norm = 1.0 if clip else None
        self.ema_decay = 0.9 if ema else None
        self.rank, self.log = rank, []

    def train_step(self, x, target, font=None, mean_elems=None, do_step=True, **hyper):
        self.flat_grads.fill_(float(self.rank + 1))
        if do_step:
            self.adamw_step()

    def forward_loss(self, x, target, font=None, mean_elems=None, **kw):
        self.flat_grads.fill_(float(self.rank + 1))

    def backward_stage(self, stage):
        return self.flat_grads[self.N // 2:] if stage == 0 else self.flat_grads[:self.N // 2]

    def grad_sumsq(self, offset, n):
        return (self.flat_grads[offset:offset + n] ** 2).sum().reshape(1)

    def adamw_step(self, **hyper):
        self.log.append("adamw_step")           # (the engine's own step owns its EMA: afr_adamw_step ends in the hook)
        self.flat_params -= 0.1 * self.flat_grads

    def adamw_range(self, offset, n, sumsq=None, **hyper):
        self.log.append("adamw_range")
        self.flat_params[offset:offset + n] -= 0.1 * self.flat_grads[offset:offset + n]

    def ema_update(self, sumsq=None):
        # by now every rank's slice is in place: the whole buffer has moved by the summed gradient (1 + 2) * 0.1 per step
        whole = bool((self.flat_params == self.flat_params[0]).all()) and float(self.flat_params[0]) != 0.0
        self.log.append(("ema_update", None if sumsq is None else float(sumsq), whole))

    def sync_params(self):
        self.log.append("sync_params")


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ai_font_renderer_amd import parallel
    from ai_font_renderer_amd.parallel import DataParallelStepper
    torch.set_num_threads(1)
    gather = parallel._all_gather_inplace
    out = {}
    for schedule in ("one-allreduce", "overlapped", "sharded"):
        parallel.OVERLAP_MIN_BYTES = 0 if schedule == "overlapped" else 1 << 60
        parallel.SHARD_MIN_BYTES = 0
        os.environ["AFR_DP_SCHEDULE"] = "shard" if schedule == "sharded" else "overlap"
        for ema in (True, False):
            for clip in (False, True):
                eng = RecordingEngine(rank, ema, clip)

                def logged_gather(*a, _eng=eng, **kw):
                    gather(*a, **kw)
                    _eng.log.append("all_gather")
                parallel._all_gather_inplace = logged_gather
                st = DataParallelStepper(eng, dist, world)
                assert st.sharded() == (schedule == "sharded")
                x = torch.zeros(4, dtype=torch.int64)
                for _ in range(3):
                    st.step(x, x, None, mean_elems=8)
                out[(schedule, ema, clip)] = eng.log
    parallel._all_gather_inplace = gather
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_stepper_counts_the_sharded_step_once_after_the_all_gather_and_leaves_the_other_schedules_alone():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == [0, 1]
    for rank, out in res.items():
        for (schedule, ema, clip), log in out.items():
            updates = [c for c in log if isinstance(c, tuple)]
            if schedule != "sharded":
                assert log == ["adamw_step"] * 3, (rank, schedule, ema, clip, log)          # never the stepper's business there
                continue
            if not ema:
                assert log == ["adamw_range", "all_gather", "sync_params"] * 3, (rank, ema, clip, log)
                continue
            assert [c if isinstance(c, str) else c[0] for c in log] == ["adamw_range", "all_gather", "ema_update", "sync_params"] * 3, (rank, clip, log)
            assert len(updates) == 3 and all(u[2] for u in updates), (rank, clip, updates)   # the whole buffer was in place each time
            # clipping: the all-reduced sum of squares the slice update read, every element holds 1 + 2 = 3 after the sum: 9 * 128 per rank, all-reduced over the two; else none
            assert [u[1] for u in updates] == ([2304.0] * 3 if clip else [None] * 3), (rank, clip, updates)
