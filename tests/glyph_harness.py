"""What the single-launch tests of the glyph kernels share (tests/test_gpu_glyph_ops.py, tests/test_gpu_glyph_step_ops.py): a case's tables
on the device, its ids on the device, and the rule a first layer's h1 and its ReLU gates are held to."""
from . import glyph_ref as R
from .gpu_util import dev, ptr


class Tables:
    """a case's parameters on the device"""

    def __init__(self, E, N1, vocab, n_fonts, tid):
        self.E, self.N1, self.vocab, self.n_fonts = E, N1, vocab, n_fonts
        self.t = R.make_tables(E, N1, vocab, n_fonts, tid)
        self.d = {k: (dev(v) if v is not None else None) for k, v in self.t.items()}

    def p(self, k):
        return ptr(self.d[k])


def ids_dev(x, font):
    return dev(x), (dev(font) if font is not None else None)


def check_h1(name, got_h1, Tr, Tb, b1, xc, fc, vocab, n_fonts, is_bf16):
    pre, bp, ref, bnd = R.h1_ref(Tr, Tb, b1, xc, fc, vocab, n_fonts, is_bf16)
    flipped = (got_h1.double() > 0) != (pre > 0)
    assert not bool((flipped & (pre.abs() > bp)).any()), f"{name}: a ReLU gate differs from fp64's where |pre| is above its bound"
    assert int(flipped.sum()) <= 1e-3 * pre.numel()
    return R.ratio(got_h1, ref, bnd), int(flipped.sum())
