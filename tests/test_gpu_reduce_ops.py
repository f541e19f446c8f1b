"""GPU: the slab reductions one launch at a time -- afr_op_reduce (reduce_slabs_kernel) and afr_op_reduce_group_step (reduce_group_kernel:
plain, and with the optimizer step a single-GPU training step fuses into it: the four OPT x GROUPS instantiations, reduce_finish's
stores of p / m / v / shadow and the transposed copies) -- against the checker tests/reduce_ref.py, by the method of tests/op_harness.py.

Every launch runs twice and must repeat bit for bit; every output lies between guard bands; every slab is `stride` > n apart with NaN
in [n, stride), so that an add that strays into the padding shows; the segments of a launch lie in one flat buffer, not in the caller's
order, with gaps of 64 floats or more whose NaN fill must survive -- in dst, p, m, v, the shadow, and in the transposed buffer
everywhere outside a segment's own columns.

PLAIN: dst equals reduce_ref.ordered_sum bit for bit (the fixed slab order of afr.h) and lies within (nslabs - 1) 2^-24 sum|v| of fp64.
FUSED (reduce_ref.check_fused): (a) p, m, v, shadow equal, bit for bit, what afr_op_adamw / afr_op_lion leave from the OWN gradient --
the plain launch of the same table -- segment by segment with the segment's folded (lr_i, wd_i); (b) AdamW: within 3e-6 max(1, max|.|)
of linear_ref.adamw in fp64 on the own gradient (test_gpu_linear_ops' bounds; t = 3); Lion: bit for bit afr_op_lion, which is (a) -- the
treatment test_gpu_linear_ops gives its fused Lion tail; (c) shadow == bf16(p); (d) every transposed block == bf16(p)^T at pitch tN;
(e) Lion is handed v = NULL, and the NaN buffer that lies where v would is untouched; (f) the kernel's name.  dst keeps its NaN fill
in a fused launch: the summed gradient is never stored.
The inputs' condition (the order shows in the bits) and every check against planted faults: tests/test_reduce_ref_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from . import reduce_ref as R
from .op_harness import Outs, judge, twice
from .test_gpu_linear_ops import ADAMW, LION
from .util import ratio

pytestmark = pytest.mark.gpu

HYPER = {"adamw": ADAMW, "lion": LION}
GUARD = 64


@functools.lru_cache(maxsize=2)
def dev_slabs(name):
    return [torch.from_numpy(sg.slabs).cuda() for sg in R.case(name).segs]


def group_launch(c, sl, dst, step=None):
    """one afr_op_reduce_group_step launch over the case's segments, dst = the flat buffer's first element; -> the kernel's name"""
    from ai_font_renderer_amd import _lib
    from .gpu_util import stream
    k = len(c.segs)
    name = C.create_string_buffer(32)
    _lib.check(_lib.lib().afr_op_reduce_group_step(
        k, (C.c_void_p * k)(*[dst.value + 4 * sg.off for sg in c.segs]), (C.c_void_p * k)(*[t.data_ptr() for t in sl]),
        (C.c_int * k)(*[sg.nslabs for sg in c.segs]), (C.c_int64 * k)(*[sg.stride for sg in c.segs]), (C.c_int64 * k)(*[sg.n for sg in c.segs]),
        C.byref(step) if step is not None else None, name, 32, stream()))
    return name.value.decode()


@functools.lru_cache(maxsize=None)
def own_plain(name):
    """The plain launch of a case, held to its checks; -> the own gradient of every segment (CPU)."""
    c, sl = R.case(name), dev_slabs(name)

    def run():
        o = Outs()
        dst = o.new("dst", c.total, torch.float32, guard=GUARD)
        return group_launch(c, sl, dst), o.finish(may_keep_fill=("dst",))
    kname, out = twice(run)
    assert kname == "reduce_group<0,0>"
    judge("plain " + name, R.check_plain(c, out["dst"]))
    return [out["dst"][sg.off:sg.off + sg.n].clone() for sg in c.segs]


@pytest.mark.parametrize("name", R.PLAIN_CASES)
def test_plain_launch_is_the_ordered_sum_bit_for_bit(name):
    own_plain(name)


# ------------------------------------------------------------------------------------------------------------- afr_op_reduce
REDUCE_N = (3, 1003, 4096, 4 * (2048 * 256) + 5)            # the last one is past the launcher's 2048 blocks: a second trip, and a tail


@functools.lru_cache(maxsize=1)
def reduce_inputs(n):
    nslabs = 3 if n > 100000 else 7
    stride = (n + 3) // 4 * 4 + 4
    sl = R.slab_values(6800 + n % 977, nslabs, n, stride)
    return nslabs, stride, sl, torch.from_numpy(sl).cuda(), R.synth.hash_uniform(6700 + n % 977, (n,), 3.0)


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", REDUCE_N)
def test_reduce_is_the_sum_in_slab_order(n, acc, scale):
    """Bit for bit where nothing is left to the compiler (scale 1 and 0.5: exact products; scale 0.3 without accumulate: one rounded
    product); scale 0.3 with accumulate: each element equals the product rounded and then added, or the single rounding of the fused
    form.  Against fp64: scale times the slab sum's bound, and 2^-24 of |scale sum| and of the result for the product and the add."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import ptr, stream
    nslabs, stride, sl, sld, old = reduce_inputs(n)

    def run():
        o = Outs()
        dst = o.new("dst", n, torch.float32, guard=GUARD, init=torch.from_numpy(old) if acc else None)
        _lib.check(_lib.lib().afr_op_reduce(dst, ptr(sld), nslabs, stride, n, scale, acc, stream()))
        return o.finish()
    got = twice(run)["dst"].numpy()
    forms = R.reduce_slabs_ref(sl, nslabs, n, scale, old if acc else None)
    assert len(forms) == (2 if acc and scale == 0.3 else 1)
    hit = np.zeros(n, dtype=bool)
    for f in forms:
        hit |= got.view(np.int32) == f.view(np.int32)
    assert hit.all(), "%d of %d elements are no legal float32 form of the sum in slab order" % (int((~hit).sum()), n)
    s32 = float(np.float32(scale))
    ref = R.sum64(sl, nslabs, n) * s32 + (old.astype(np.float64) if acc else 0.0)
    bound = s32 * R.sum_bound(sl, nslabs, n) + R.U24 * (np.abs(R.sum64(sl, nslabs, n) * s32) + np.abs(ref))
    judge("reduce n=%d acc=%d scale=%g" % (n, acc, scale), {"dst": ratio(torch.from_numpy(got), torch.from_numpy(ref), torch.from_numpy(bound))})


# ------------------------------------------------------------------------------------------------------------- the fused launch
@functools.lru_cache(maxsize=None)
def flat_entries(name, kind, groups):
    """p, m, v, shadow as afr_op_adamw / afr_op_lion leave them from the own gradient, one launch per segment with the segment's folded
    (lr_i, wd_i), laid out like the fused launch's buffers."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import ptr, stream
    c, h = R.case(name), HYPER[kind]
    grads = own_plain(name)
    P0, M0, V0 = R.state(name)
    lib = _lib.lib()
    parts = {k: [] for k in ("p", "m", "v", "shadow")}
    for i, sg in enumerate(c.segs):
        a = R.seg_hyper(h, sg, groups)
        p, m, v, g = (t.clone().cuda() for t in (P0[i], M0[i], V0[i], grads[i]))
        sh = torch.full((sg.n,), float("nan"), dtype=torch.bfloat16, device="cuda")
        if kind == "adamw":
            _lib.check(lib.afr_op_adamw(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), sg.n, a["lr"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"], a["t"],
                                        1.0, stream()))
        else:
            _lib.check(lib.afr_op_lion(ptr(p), ptr(g), ptr(m), ptr(sh), sg.n, a["lr"], a["beta1"], a["beta2"], a["weight_decay"], 1.0, None, 0.0, stream()))
        torch.cuda.synchronize()
        for k, t in zip(("p", "m", "v", "shadow"), (p, m, v, sh)):
            parts[k].append(t.cpu())
    return {k: c.scatter(v, dtype=torch.bfloat16 if k == "shadow" else torch.float32) for k, v in parts.items()}


def fused_case(name, kind, groups, shadow):
    from ai_font_renderer_amd import _lib
    c, h, sl = R.case(name), HYPER[kind], dev_slabs(name)
    grads = own_plain(name)
    flat = flat_entries(name, kind, groups)
    P0, M0, V0 = R.state(name)
    k = len(c.segs)
    names = ["dst", "p", "m", "v"] + (["shadow"] if shadow else []) + (["shT"] if c.tr_total else [])

    def run():
        o = Outs()
        dst = o.new("dst", c.total, torch.float32, guard=GUARD)
        p = o.new("p", c.total, torch.float32, guard=GUARD, init=c.scatter(P0))
        m = o.new("m", c.total, torch.float32, guard=GUARD, init=c.scatter(M0))
        v = o.new("v", c.total, torch.float32, guard=GUARD, init=c.scatter(V0) if kind == "adamw" else None)
        st = _lib.AfrReduceStep(opt_kind=_lib.OPT_KINDS[kind], lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], weight_decay=h["weight_decay"],
                                t=h["t"], gbase=dst.value, p=p.value, m=m.value, v=v.value if kind == "adamw" else None)       # (e): Lion is handed no v at all
        if shadow:
            st.shadow = o.new("shadow", c.total, torch.bfloat16, guard=GUARD).value
        if groups:
            st.lr_mult, st.wd_mult = (C.c_float * k)(*[sg.mult[0] for sg in c.segs]), (C.c_float * k)(*[sg.mult[1] for sg in c.segs])
        if c.tr_total:
            base = o.new("shT", c.tr_total, torch.bfloat16, guard=GUARD).value
            st.shT = (C.c_void_p * k)(*[base + 2 * sg.tr[0] if sg.tr else None for sg in c.segs])
            st.tN, st.tK = (C.c_int32 * k)(*[sg.tr[1] if sg.tr else 0 for sg in c.segs]), (C.c_int32 * k)(*[sg.tr[2] if sg.tr else 0 for sg in c.segs])
        return group_launch(c, sl, dst, st), o.finish(may_keep_fill=names)
    kname, out = twice(run)
    assert kname == "reduce_group<%d,%d>" % (kind == "lion", groups)                                   # (f)
    worst = R.check_fused(c, kind, h, groups, out, flat, grads)
    judge("fused %s %s groups=%d shadow=%d" % (name, kind, groups, shadow), worst or {"flat-entry bits (Lion)": 0.0})


@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("kind", ["adamw", "lion"])
@pytest.mark.parametrize("name", R.FUSED_SETS)
def test_fused_step_equals_the_flat_entries_on_the_own_gradient(name, kind, groups, shadow):
    fused_case(name, kind, groups, shadow)


@pytest.mark.parametrize("kind", ["adamw", "lion"])
def test_fused_step_past_the_block_cap(kind):
    """the deep segment whose every block takes a second trip, with the step: p, m, v are loaded by the first wave only, each trip"""
    fused_case("cap-deep", kind, False, True)
