"""CPU: the host side of the chained launch's fifth role (csrc/gemm.hip GemmGroup::l1; include/afr.h afr_op_linear_chain_l1*): the
block map of the first-layer range behind the four products, and the refusals of afr_op_linear_chain_l1 -- those of the chained
launch, those of the fused first-layer backward, and a d1 that is not the lower input gradient.  Every refusal is decided on
the host, ahead of any device call."""
import ctypes as C

from .test_chain_cpu import CUS, _plan
from .util import ROOT  # noqa: F401  (puts the repository on sys.path)

# (B, N_up, K_up, N1).  The fused first-layer kernel takes N1 = 128 m <= 1024; the chain needs 32 x ceil(N1 / 128) >= 232 tiles of
# the lower input gradient at its 32 row blocks at the most (tests/test_chain_cpu.py SMALLEST: 904 columns, and 896 is refused), so
# N1 = 1024 is the ONE first-layer width at which both hold, and with it the first layer always runs two column ranges of 512.
RAGGED = (7944, 1000, 1000, 1024)           # a last first-layer block of 8 glyphs, a last row block of 8 rows
TWO_RANGES = (8192, 1024, 1024, 1024)       # whole blocks: C3 itself (8192 rows in 8 slices need N_up, K_up >= 1024)
# eligible for the fused kernel, refused by the chain: 7 x 32 = 224 tiles; 8192 rows of a 1000-wide layer would be 9 slices
NOT_CHAINED = ((7944, 1000, 1000, 896), (8192, 1000, 1000, 1024))
VOCAB, FONTS = 96, 8


def _l1_plan(shape, has_loss=0, cus=CUS, vocab=VOCAB, fonts=FONTS):
    from ai_font_renderer_amd import _lib
    nb, ws = C.c_int(), C.c_size_t()
    rc = _lib.lib().afr_op_linear_chain_l1_plan(*shape, vocab, fonts, has_loss, cus, C.byref(nb), C.byref(ws))
    return rc, nb.value, ws.value


def _l1_block(shape, b, has_loss=0):
    from ai_font_renderer_amd import _lib
    role, rb, cr, wb = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = _lib.lib().afr_op_linear_chain_l1_block(*shape, VOCAB, FONTS, has_loss, b, C.byref(role), C.byref(rb), C.byref(cr), C.byref(wb))
    return rc, role.value, (rb.value, cr.value, wb.value)


def test_one_first_layer_width_chains_and_is_eligible():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    ok = [n1 for n1 in range(128, 1024 + 1, 128) for (B, n) in ((7944, 1000), (8192, 1024)) if _l1_plan((B, n, n, n1))[0] == 0]
    assert sorted(set(ok)) == [1024], ok
    assert lib.afr_glyph_l1_bwd_fused_eligible(_lib.AFR_BF16, 32, 896, VOCAB, FONTS) == 1
    for shape in NOT_CHAINED:
        assert _l1_plan(shape)[0] == _lib.AFR_EUNSUPPORTED and b"chained" in lib.afr_last_error()
        assert _op(shape) == _lib.AFR_EUNSUPPORTED and b"chained" in lib.afr_last_error()
    assert _l1_plan(RAGGED)[0] == 0 and _l1_plan(TWO_RANGES)[0] == 0
    assert _l1_plan(TWO_RANGES, cus=255)[0] == _lib.AFR_EUNSUPPORTED


def test_plan_adds_the_first_layer_range_and_a_second_set_of_counters():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    for shape in (RAGGED, TWO_RANGES):
        B, _, _, N1 = shape
        rc, _, _, nb, ws = _plan(*shape)
        assert rc == 0
        l1 = lib.afr_glyph_l1_bwd_fused_blocks(B, N1)
        counters = -(-(-(-B // 256) * 4) // 256) * 256
        assert _l1_plan(shape) == (0, nb + l1, ws + counters)
        assert _l1_plan(shape, has_loss=1) == (0, nb + l1 + 1, ws + counters)
    assert lib.afr_glyph_l1_bwd_fused_blocks(7944, 1024) == 250 and lib.afr_glyph_l1_bwd_fused_split(7944, 1024) == 2
    assert lib.afr_glyph_l1_bwd_fused_blocks(8192, 1024) == 256 and lib.afr_glyph_l1_bwd_fused_split(8192, 1024) == 2


def test_block_map_of_the_first_layer_range():
    """Behind the four products' blocks (role 0) every (64-glyph row block, column range) exactly once, in the stand-alone kernel's
    block order, each waiting for the 256-row block of dx_lo that holds its glyphs; then, only with deferred loss partials, the
    one loss-sum workgroup; nothing beyond."""
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    for shape in (RAGGED, TWO_RANGES):
        B, _, _, N1 = shape
        nb = _plan(*shape)[3]
        cs, l1 = lib.afr_glyph_l1_bwd_fused_split(B, N1), lib.afr_glyph_l1_bwd_fused_blocks(B, N1)
        for b in (0, nb // 2, nb - 1):
            assert _l1_block(shape, b) == (0, 0, (-1, -1, -1))
        seen = set()
        for j in range(l1):
            rc, role, (rb, cr, wb) = _l1_block(shape, nb + j)
            assert (rc, role) == (0, 1) and (rb, cr) == (j // cs, j % cs) and wb == rb * 64 // 256, (j, rb, cr, wb)
            assert wb < -(-B // 256) and rb * 64 < B
            seen.add((rb, cr))
        assert seen == {(r, c) for r in range(-(-B // 64)) for c in range(cs)}
        assert _l1_block(shape, nb + l1)[0] == _lib.AFR_EINVAL
        assert _l1_block(shape, nb + l1, has_loss=1) == (0, 2, (-1, -1, -1))
        assert _l1_block(shape, nb + l1 + 1, has_loss=1)[0] == _lib.AFR_EINVAL and _l1_block(shape, -1)[0] == _lib.AFR_EINVAL


def _op(shape, *, d1_is_dx=True, vocab=VOCAB, fonts=FONTS, ldh=32):
    """afr_op_linear_chain_l1 on made-up addresses: only refusals that are decided ahead of any device call are asked for"""
    from ai_font_renderer_amd import _lib
    B, N_up, K_up, N1 = shape
    a = lambda i: C.c_void_p(0x10000 * (i + 1))
    dx_lo = a(9)
    return _lib.lib().afr_op_linear_chain_l1(a(0), a(1), a(2), a(3), a(4), None, a(5), a(6), a(7), dx_lo, None, B, N_up, K_up, N1, a(8), 1 << 40,
                                             dx_lo if d1_is_dx else a(10), a(11), ldh, None, a(12), a(13), a(14), vocab, fonts, a(15),
                                             None, 0, 0, 0.0, None, None, 0, None)


def test_refusals_of_both_parts():
    from ai_font_renderer_amd import _lib
    lib, EU = _lib.lib(), _lib.AFR_EUNSUPPORTED
    # a shape the chain refuses (batch 4096: too few 256x256 tiles for the cooperative pairs), first layer eligible
    assert _op((4096, 1024, 1024, 1024)) == EU and b"chained" in lib.afr_last_error()
    assert _l1_plan((4096, 1024, 1024, 1024))[0] == EU and b"chained" in lib.afr_last_error()
    # a first layer the fused kernel is not eligible for: the smallest chained triple's 904 columns are no multiple of 128 ...
    assert _op((7944, 1000, 1000, 904)) == EU and b"fused backward" in lib.afr_last_error()
    assert _l1_plan((7944, 1000, 1000, 904))[0] == EU
    # ... and more than 144 table rows
    assert _op(TWO_RANGES, vocab=140, fonts=8) == EU and b"table rows" in lib.afr_last_error()
    assert _op(TWO_RANGES, ldh=36) == _lib.AFR_EINVAL
    # a d1 that is not member 3's output
    assert _op(TWO_RANGES, d1_is_dx=False) == EU and b"dx_lo" in lib.afr_last_error()


def test_plan_takes_the_new_switch():
    """config.reserved bit 9 (AFR_CFG_NO_L1_CHAIN) keeps the first-layer backward a launch of its own; it does not touch the pair chain."""
    from ai_font_renderer_amd import _lib
    from .test_chain_cpu import _glyph_plan
    lib = _lib.lib()
    for flags in (0, 512):
        plan = _glyph_plan(_lib.AFR_BF16, flags)
        try:
            assert lib.afr_plan_pair_chain(plan, 8192, CUS) == 1
        finally:
            lib.afr_plan_destroy(plan)
