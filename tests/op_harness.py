"""The single-launch method of the kernel op tests, stated once: ONE launch through an afr_op_* entry into pre-filled output buffers that
lie between two guard bands (Outs), the launch repeated and compared bit for bit (twice, same), every output against fp64 under its
derived bound with the largest error printed as a fraction of that bound (judge).  tests/test_op_harness_cpu.py plants one fault at a
time into each of these checks.  DESIGN.md 4 names the files that use it; a new single-launch test starts here.  Nothing in this module
needs a GPU to be imported: every helper that allocates takes the device."""
import ctypes as C
import math

import torch

from .util import ratio

BAND = 256                      # bytes: the least guard band, and the alignment that the plan's carve gives every workspace buffer
SENTINEL = -0x5A5A5A5B          # fill of int32 outputs: no index, count or flag word a kernel writes equals it


def bits(t):
    """the tensor's bytes as integers: comparisons that see the sign of a zero and in which a NaN equals itself"""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def tt(is_bf16):
    return torch.bfloat16 if is_bf16 else torch.float32


def dt(is_bf16):
    from ai_font_renderer_amd import _lib
    return _lib.AFR_BF16 if is_bf16 else _lib.AFR_F32


def _fill(n, dtype, device):
    """n elements of the dtype's fill: NaN (floats), SENTINEL (int32), 0xFF (uint8)"""
    value = float("nan") if dtype.is_floating_point else SENTINEL if dtype == torch.int32 else 0xFF
    return torch.full((n,), value, dtype=dtype, device=device)


def _banded(n, dtype, guard, device):
    """(fill-valued buffer of band + n + band elements, the band in elements): the band is `guard` elements rounded up to whole
    multiples of BAND bytes, and BAND bytes at the least, so element `band` keeps the allocation's alignment up to BAND"""
    size = torch.empty(0, dtype=dtype).element_size()
    band = -(-max(guard * size, BAND) // BAND) * BAND // size
    return _fill(n + 2 * band, dtype, device), band


def bands_kept(buf, band=BAND):
    """(in front, behind): whether the `band` elements at either end of buf still hold the fill's bits"""
    want = bits(_fill(band, buf.dtype, buf.device))
    return torch.equal(bits(buf[:band]), want), torch.equal(bits(buf[buf.numel() - band:]), want)


def guarded_bytes(nbytes, device="cuda"):
    """(whole uint8 buffer of 0xFF, its nbytes between two bands of BAND bytes): for launches whose results stay on the device;
    all(bands_kept(whole)) afterwards"""
    buf, band = _banded(nbytes, torch.uint8, 0, device)
    return buf, buf[band:band + nbytes]


class Outs:
    """output buffers of one launch, each between two guard bands and pre-filled like them (_fill)"""

    def __init__(self, device="cuda"):
        self.device, self.bufs = device, {}

    def new(self, name, shape, dtype, *, guard=0, init=None):
        """-> the pointer to hand to the library.  shape: a tuple, or the element count; guard: elements asked for in each band (never
        fewer than BAND bytes are given); init pre-loads the owned part, for kernels that work in place"""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        t, band = _banded(n, dtype, guard, self.device)
        if init is not None:
            t[band:band + n] = init.reshape(-1).to(device=self.device, dtype=dtype)
        self.bufs[name] = (t, band, n, shape)
        return C.c_void_p(t.data_ptr() + band * t.element_size())

    def finish(self, may_keep_fill=()):
        """-> name -> CPU tensor in the requested shape, after synchronising; asserts that both bands of every buffer kept their bits
        and that no fill value is left in the part the kernel owns (uint8 buffers and the names in may_keep_fill exempt)"""
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        out = {}
        for name, (t, band, n, shape) in self.bufs.items():
            front, behind = bands_kept(t, band)
            assert front, f"{name}: the guard band in front of the buffer was written"
            assert behind, f"{name}: the guard band behind the buffer was written"
            own = t[band:band + n]
            if t.dtype != torch.uint8 and name not in may_keep_fill:
                left = torch.isnan(own) if t.dtype.is_floating_point else own == SENTINEL
                assert not bool(left.any()), f"{name}: {int(left.sum())} elements the kernel owns were not written"
            out[name] = own.reshape(shape).cpu()
        return out


def same(a, b, what):
    """two results of a launch -- tensors, other values, or dicts, tuples and lists of them -- are the same: tensors bit for bit"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), f"{what}: other keys"
        for k in a:
            same(a[k], b[k], f"{what}: {k}")
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), f"{what}: another length"
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{what}: [{i}]")
    elif isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what} differs"
    else:
        assert not isinstance(b, torch.Tensor) and a == b, f"{what} differs"


def twice(launch):
    """launch() run twice on the same inputs: every tensor it returns repeats bit for bit, every other value is equal; -> the first"""
    a, b = launch(), launch()
    same(a, b, "a second launch on the same inputs")
    return a


def judge(name, got, ref=None, bound=None, keys=None):
    """Prints the case's line -- the largest error of every key as a fraction of its bound (util.ratio) -- and asserts each <= 1.
    got, ref, bound: key -> tensor; or got alone: key -> an already computed ratio."""
    worst = dict(got) if ref is None else {k: ratio(got[k].double().reshape(ref[k].shape), ref[k], bound[k]) for k in keys}
    print(f"{name}: max error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (name, k, v)
