"""CPU: the row-index entry points (afr_bind_dataset, afr_*_rows) reject bad calls on the host, in the documented order, before
anything is launched; and DataParallelStepper.step_rows runs the schedules of step() on a rank's shard of an index vector
(world 2 over gloo, with the oracle-backed stand-in engine of test_parallel_cpu indexing its data set on the CPU)."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from .test_parallel_cpu import CFG, ROWS, OracleEngine, _inputs
from .util import ROOT

EINVAL, ESTATE, EUNSUPPORTED = -1, -2, -4


def _plan(cfg, dtype="f32", max_batch=8):
    from ai_font_renderer_amd import _lib
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    c = make_afr_config(cfg, dtype, max_batch)
    plan = C.c_void_p()
    _lib.check(lib.afr_plan_create(C.byref(c), C.byref(plan)))
    return lib, plan


def _rows_calls(lib, plan, rows, B):
    """The four calls by rows with otherwise valid (fake, never dereferenced) arguments: (name, return code, message)."""
    fake = C.c_void_p(0x1000)
    out = []
    for name, call in (("forward", lambda: lib.afr_forward_rows(plan, rows, B, fake, 0, 0, None)),
                       ("loss_grad", lambda: lib.afr_loss_grad_rows(plan, rows, B, 192 * 4, fake, None)),
                       ("forward_loss", lambda: lib.afr_forward_loss_rows(plan, rows, B, 192 * 4, fake, 1, None)),
                       ("train_step", lambda: lib.afr_train_step_rows(plan, rows, B, 192 * 4, fake, 1, 1, 1e-3, 0.9, 0.99, 1e-8, 5e-4, 1, None))):
        out.append((name, call(), lib.afr_last_error()))
    return out


def test_rows_calls_and_bind_dataset_are_validated_on_the_host():
    """Fake non-null pointers, nothing is launched (the plans have no parameters bound either)."""
    from ai_font_renderer_amd import config
    fake = C.c_void_p(0x1000)
    lib, plan = _plan(config.SheetConfig(max_length=10, sheet_h=8, sheet_w=24))
    # no data set bound: AFR_ESTATE before anything else, also with every other argument bad
    for rows, B in ((fake, 4), (None, 0)):
        for name, rc, msg in _rows_calls(lib, plan, rows, B):
            assert rc == ESTATE and b"data set" in msg, (name, rc, msg)
    # afr_bind_dataset itself
    assert lib.afr_bind_dataset(plan, fake, None, fake, 0, 1 << 31, 10) == EUNSUPPORTED and b"2^31" in lib.afr_last_error()
    assert lib.afr_bind_dataset(plan, fake, None, fake, 0, 100, 0) == EINVAL and b"L" in lib.afr_last_error()
    assert lib.afr_bind_dataset(plan, fake, None, fake, 0, 100, -3) == EINVAL
    assert lib.afr_bind_dataset(plan, fake, None, fake, 7, 100, 10) == EINVAL and b"target dtype" in lib.afr_last_error()
    assert lib.afr_bind_dataset(plan, fake, None, None, 0, 100, 10) == EINVAL          # codes without targets
    for name, rc, msg in _rows_calls(lib, plan, fake, 4):                              # a refused bind binds nothing
        assert rc == ESTATE and b"data set" in msg, (name, rc, msg)
    # bound: rows NULL / B outside 1..max_batch are AFR_EINVAL
    assert lib.afr_bind_dataset(plan, fake, None, fake, 0, (1 << 31) - 1, 37) == 0
    for rows, B, frag in ((None, 4, b"rows"), (fake, 0, b"batch"), (fake, 9, b"batch"), (fake, -1, b"batch")):
        for name, rc, msg in _rows_calls(lib, plan, rows, B):
            assert rc == EINVAL and frag in msg, (name, rows, B, rc, msg)
    # valid rows, but the plan has no parameters / workspace bound: refused before the prepare kernel is launched
    for name, rc, msg in _rows_calls(lib, plan, fake, 8):
        assert rc == ESTATE and b"bound parameters" in msg, (name, rc, msg)
    # all-NULL unbinds
    assert lib.afr_bind_dataset(plan, None, None, None, 0, 0, 0) == 0
    for name, rc, msg in _rows_calls(lib, plan, fake, 4):
        assert rc == ESTATE and b"data set" in msg, (name, rc, msg)
    lib.afr_plan_destroy(plan)
    # a plan with fonts needs font ids; glyph / pixel rows are single codes
    for cfg in (config.GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2), config.PixelConfig(out_h=2, out_w=4, d_model=64, heads=1, layers=1, ff_dim=32, n_fonts=2)):
        lib, plan = _plan(cfg)
        assert lib.afr_bind_dataset(plan, fake, None, fake, 0, 100, 1) == EINVAL and b"font" in lib.afr_last_error()
        assert lib.afr_bind_dataset(plan, fake, fake, fake, 0, 100, 2) == EINVAL
        assert lib.afr_bind_dataset(plan, fake, fake, fake, 1, 100, 1) == 0
        lib.afr_plan_destroy(plan)
    lib, plan = _plan(config.GlyphConfig(hidden=(48,), out_h=4, out_w=6))               # no fonts: none needed
    assert lib.afr_bind_dataset(plan, fake, None, fake, 0, 100, 1) == 0
    lib.afr_plan_destroy(plan)
    assert lib.afr_bind_dataset(None, fake, None, fake, 0, 100, 1) == EINVAL


class RowsOracleEngine(OracleEngine):
    """The stand-in engine with a bound data set: the calls by rows index it on the CPU and take the dense path."""

    def bind_dataset(self, x, target, font=None):
        self._ds = (x, target, font)

    def train_step_rows(self, rows, mean_elems=None, do_step=True, **hyper):
        x, target, font = self._ds
        self.train_step(x[rows], target[rows], font=None if font is None else font[rows], mean_elems=mean_elems, do_step=do_step, **hyper)


def _perm():
    return torch.randperm(ROWS, generator=torch.Generator().manual_seed(7))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ai_font_renderer_amd import parallel
    from ai_font_renderer_amd.parallel import DataParallelStepper, shard_rows
    parallel.SHARD_MIN_BYTES = 1 << 60
    torch.set_num_threads(1)
    x, font, t = _inputs(CFG, ROWS)
    eng = RowsOracleEngine(CFG)
    eng.bind_dataset(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(font))
    st = DataParallelStepper(eng, dist, world)
    mine = _perm()[shard_rows(ROWS, rank, world)]
    assert mine.numel() == (19, 18)[rank]
    for _ in range(3):
        st.step_rows(mine, mean_elems=ROWS * CFG.pixels)
    loss = st.global_loss()
    q.put((rank, {k: v.numpy() for k, v in eng.P.items()}, eng.flat_grads.numpy().copy(), loss))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_step_rows_equals_full_batch():
    """step_rows on the uneven shards (19 + 18 rows) of a permuted index vector == the single-process step on the whole
    permuted batch: what test_two_rank_data_parallel_equals_full_batch asserts for step()."""
    from ai_font_renderer_amd.parallel import DataParallelStepper
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x, font, t = _inputs(CFG, ROWS)
    perm = _perm().numpy()
    eng = OracleEngine(CFG)
    st = DataParallelStepper(eng, None, 1)
    for _ in range(3):
        st.step(torch.from_numpy(x[perm]), torch.from_numpy(t[perm]), torch.from_numpy(font[perm]), mean_elems=ROWS * CFG.pixels)
    full_loss = st.global_loss()
    for rank, P, g, loss in res:
        assert abs(loss - full_loss) < 1e-6 * full_loss
        assert np.abs(g - eng.flat_grads.numpy()).max() < 1e-6 * np.abs(g).max()
        for k in P:
            assert np.abs(P[k] - eng.P[k].numpy()).max() < 2e-6, (rank, k)
    for k in res[0][1]:                                     # replicas stay bit-identical to each other
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    # a world of one steps by rows through the engine's own optimizer step
    one = RowsOracleEngine(CFG)
    one.bind_dataset(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(font))
    st1 = DataParallelStepper(one, None, 1)
    for _ in range(3):
        st1.step_rows(_perm(), mean_elems=ROWS * CFG.pixels)
    assert abs(st1.global_loss() - full_loss) < 1e-6 * full_loss
    for k in one.P:
        assert np.abs(one.P[k].numpy() - eng.P[k].numpy()).max() < 2e-6, k
