"""CPU: global gradient-norm clipping -- the ABI's argument checks (host-only calls, nothing is launched), the checker
(tests/clip_ref.py) against torch's own clip_grad_norm_ + AdamW, and the data-parallel schedules (gloo, two ranks) driven with
an oracle-backed stand-in engine that clips the way the HIP engine does: sum of squares of a flat range, all-reduced under the
sharded optimizer, coefficient inside the update."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import clip_ref
from .test_parallel_cpu import CFG, ROWS, OracleEngine, _inputs
from .util import ROOT, oracle, tparams


def _plan(cfg=None, dtype="f32", max_batch=64):
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    c = make_afr_config(cfg or config.WORKLOADS["c1"]["cfg"], dtype, max_batch)
    plan = C.c_void_p()
    _lib.check(_lib.lib().afr_plan_create(C.byref(c), C.byref(plan)))
    return plan


def test_new_symbols_are_exported_and_declared():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "afr.h")).read()
    for name in ("afr_set_grad_clip", "afr_grad_sumsq", "afr_op_adamw_clip"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.afr_version() == 1


def test_setter_rejects_negative_and_non_finite_norms_with_a_message():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    plan = _plan()
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.afr_set_grad_clip(plan, bad, None) == -1, bad          # AFR_EINVAL
        assert b"max_norm" in lib.afr_last_error()
    assert lib.afr_set_grad_clip(None, 1.0, None) == -1
    for ok in (0.0, 1.0, 1e-3, 3e38):                                   # host-only: an unbound plan takes the setting
        assert lib.afr_set_grad_clip(plan, ok, None) == 0, ok
    lib.afr_plan_destroy(plan)


def test_grad_sumsq_rejects_unaligned_ranges_and_ranges_outside_the_buffer():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    plan = _plan()
    n = int(lib.afr_param_elems(plan))
    fake = C.c_void_p(0x1000)
    for off, cnt in ((2, 64), (0, 62), (-4, 64), (0, -4), (0, n + 4), (n, 4), (n - 60, 64), (1 << 62, 4)):
        assert lib.afr_grad_sumsq(plan, off, cnt, fake, None) == -1, (off, cnt)       # AFR_EINVAL, before anything is touched
        assert b"range" in lib.afr_last_error() or b"multiple" in lib.afr_last_error()
    assert lib.afr_grad_sumsq(plan, 0, n, None, None) == -1               # no output word
    assert lib.afr_grad_sumsq(plan, 0, n, fake, None) == -2               # a valid range on an unbound plan: AFR_ESTATE
    lib.afr_plan_destroy(plan)


def test_engine_argument_is_validated_before_anything_else():
    from ai_font_renderer_amd.engine import Engine
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Engine._check_clip(bad)
    assert Engine._check_clip(None) is None and Engine._check_clip(0) is None and Engine._check_clip(2) == 2.0


def test_checker_equals_torchs_clip_grad_norm_and_adamw():
    """clip_ref.clipped_train_step's arithmetic against torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW on the same
    gradients and moments: f32 against f32, so a few roundings (1e-6 of each tensor's largest entry)."""
    x, font, t = _inputs(CFG, ROWS)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(t).float() / 255.0
    P = tparams(CFG)
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    _, G = clip_ref.forward_backward(P, xt, tt, CFG, font=ft)
    norm = float(np.sqrt(clip_ref.grad_sumsq(G)))
    for frac in (0.25, 4.0):
        Pa, Ma, Va = P, M, V
        Pb, Mb, Vb = P, M, V
        for step in (1, 2):
            _, G, Pa, Ma, Va, total, coef = clip_ref.clipped_train_step(Pa, Ma, Va, step, xt, tt, CFG, frac * norm, font=ft)
            _, Gb = clip_ref.forward_backward(Pb, xt, tt, CFG, font=ft)
            Pb, Mb, Vb, ttotal = clip_ref.torch_clipped_step(Pb, Gb, Mb, Vb, step, frac * norm)
            assert abs(total - ttotal) <= 1e-6 * ttotal
            assert (coef < 1.0) == (frac < 1.0)
        for k in P:
            for a, b in ((Pa, Pb), (Ma, Mb), (Va, Vb)):
                assert float((a[k] - b[k]).abs().max()) <= 2e-6 * max(float(b[k].abs().max()), 1e-30), (frac, k)
    # the moments carry the coefficient (Adam's update alone would hide it): m = 0.1 * coef * g after one step from zero
    _, G, _, M1, V1, _, coef = clip_ref.clipped_train_step(P, M, V, 1, xt, tt, CFG, 0.25 * norm, font=ft)
    assert abs(coef - 0.25) < 1e-5
    k = "fc_output.weight"
    assert float((M1[k] - 0.1 * coef * G[k]).abs().max()) <= 1e-6 * float(G[k].abs().max())
    assert float((V1[k] - 0.01 * coef * coef * G[k] * G[k]).abs().max()) <= 1e-6 * float((G[k] * G[k]).max())


# ----------------------------------------------------------------------------- data parallel, two ranks over gloo
class ClippingOracleEngine(OracleEngine):
    """OracleEngine with the clipping surface of the HIP Engine: max_grad_norm, grad_sumsq over a flat range (tensor elements
    only) and the coefficient inside adamw_step / adamw_range(sumsq=)."""

    def __init__(self, cfg, max_grad_norm=None):
        super().__init__(cfg)
        self.max_grad_norm = max_grad_norm
        self.is_elem = torch.zeros(self.flat_params.numel(), dtype=torch.bool)
        for _, _, off, k in self.table:
            self.is_elem[off:off + k] = True
        self.last_coef = None

    def grad_sumsq(self, offset=0, n=None):
        n = self.flat_grads.numel() - offset if n is None else n
        assert offset % 4 == 0 and n % 4 == 0 and 0 <= offset and offset + n <= self.flat_grads.numel()
        g = self.flat_grads[offset:offset + n][self.is_elem[offset:offset + n]]
        return (g.double() ** 2).sum().to(torch.float32).reshape(1)

    def adamw_step(self, **hyper):
        n = self.flat_params.numel()
        if self.max_grad_norm:
            self.adamw_range(0, n, sumsq=self.grad_sumsq(0, n), **hyper)
        else:
            self.adamw_range(0, n, **hyper)

    def adamw_range(self, offset, n, sumsq=None, **hyper):
        if sumsq is None:
            return super().adamw_range(offset, n, **hyper)
        _, coef = clip_ref.clip_coef(float(sumsq), self.max_grad_norm)
        self.last_coef = coef
        self.t += 1
        sl = slice(offset, offset + n)
        p, m, v = oracle.adamw_step(self.flat_params[sl], self.flat_grads[sl] * coef, self.flat_m[sl], self.flat_v[sl], self.t)
        self.flat_params[sl], self.flat_m[sl], self.flat_v[sl] = p, m, v


def _worker(rank, world, port, q, shard, max_norm):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ai_font_renderer_amd import parallel
    from ai_font_renderer_amd.parallel import DataParallelStepper, shard_rows
    if shard:
        parallel.SHARD_MIN_BYTES = 0
        os.environ["AFR_DP_SCHEDULE"] = "shard"
    else:
        parallel.SHARD_MIN_BYTES = 1 << 60
    torch.set_num_threads(1)
    x, font, t = _inputs(CFG, ROWS)
    sl = shard_rows(ROWS, rank, world)
    eng = ClippingOracleEngine(CFG, max_norm)
    st = DataParallelStepper(eng, dist, world)
    assert st.sharded() == shard
    coefs = []
    for _ in range(3):
        st.step(torch.from_numpy(x[sl]), torch.from_numpy(t[sl]), torch.from_numpy(font[sl]), mean_elems=ROWS * CFG.pixels)
        coefs.append(eng.last_coef)
    q.put((rank, eng.flat_params.numpy().copy(), eng.flat_m.numpy().copy(), eng.flat_v.numpy().copy(), coefs))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("shard", [False, True])
def test_two_rank_clipped_step_equals_the_single_process_clipped_step(shard):
    """max_norm = 0.25 x the full-batch step-1 norm (the clip is active in every step).  Replicated: parameters and both moments
    identical on both ranks.  Sharded: identical parameters; a rank's moments are meaningful inside its own half only, so the
    two halves are put together.  Both against the single-process clipped step at test_parallel_cpu's bounds (parameters 2e-6;
    gradients there 1e-6 of the largest entry, which the first moment, linear in the gradient, inherits, and the second moment,
    quadratic in it, twice), and the single-process stand-in against clip_ref.clipped_train_step."""
    x, font, t = _inputs(CFG, ROWS)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(t)
    _, G = clip_ref.forward_backward(tparams(CFG), xt, tt.float() / 255.0, CFG, font=ft)
    max_norm = 0.25 * float(np.sqrt(clip_ref.grad_sumsq(G)))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000 + (1 if shard else 0)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, shard, max_norm)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from ai_font_renderer_amd.parallel import DataParallelStepper
    eng = ClippingOracleEngine(CFG, max_norm)
    st = DataParallelStepper(eng, None, 1)
    P = tparams(CFG)
    M ={k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    for i in range(3):
        st.step(xt, tt, ft, mean_elems=ROWS * CFG.pixels)
        _, _, P, M, V, _, coef = clip_ref.clipped_train_step(P, M, V, i + 1, xt, tt.float() / 255.0, CFG, max_norm, font=ft)
        assert abs(eng.last_coef - coef) <= 1e-6 and coef < 0.5, (i, coef)
    for k in P:                                                      # the stand-in is the checker's arithmetic
        assert float((eng.P[k] - P[k]).abs().max()) < 2e-6, k
        assert float((eng.M[k] - M[k]).abs().max()) <= 1e-6 * float(M[k].abs().max()), k
        assert float((eng.V[k] - V[k]).abs().max()) <= 2e-6 * float(V[k].abs().max()), k
    (_, p0, m0, v0, c0), (_, p1, m1, v1, c1) = res
    assert c0 == c1                                                  # every rank derives the same coefficient
    assert np.array_equal(p0, p1)
    if shard:
        h = p0.size // 2
        m0, v0 = np.concatenate([m0[:h], m1[h:]]), np.concatenate([v0[:h], v1[h:]])
    else:
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    fp, fm, fv = eng.flat_params.numpy(), eng.flat_m.numpy(), eng.flat_v.numpy()
    assert np.abs(p0 - fp).max() < 2e-6
    assert np.abs(m0 - fm).max() <= 1e-6 * np.abs(fm).max()
    assert np.abs(v0 - fv).max() <= 2e-6 * np.abs(fv).max()
    assert abs(c0[-1] - eng.last_coef) <= 1e-6
