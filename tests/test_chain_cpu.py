"""CPU: the host side of the chained gradient launch (csrc/gemm.hip GemmGroup::chain; include/afr.h afr_op_linear_chain*): when the
output layer's and the last hidden layer's gradient pairs leave as ONE launch, when they must fall back to the two
grouped launches, and the kernel's block -> (phase, member, tile, slice) map."""
import ctypes as C

from .util import ROOT  # noqa: F401  (puts the repository on sys.path)

CUS = 256                                   # the compute units of the device the flagship runs on
C3 = (8192, 1024, 1024, 1024)               # BASELINE C3: batch, output width, hidden width, hidden width
# The smallest layer triple the planner chains (found with afr_op_linear_chain_plan, see test_smallest_chained_triple).  On the grid of
# 256-multiples nothing with less work than C3 chains (the next are 4096 x 512 / 2048 / 2048 and up), so it is C3's tiling -- 32 row
# blocks, 4 x 4 weight tiles, 8 slices -- with every extent at the least multiple of 8 the planner still takes, the others held:
# 7944 rows (> 31 row blocks), 1000-wide output and hidden layer (8 slices of >= 993 rows each need B <= 8 N), 904 columns below
# (32 x ceil(K_lo / 128) >= 232 input-gradient tiles).  Every tile edge is ragged.  tests/test_gpu_chain.py runs its op-level cases there.
SMALLEST = (7944, 1000, 1000, 904)


def _plan(B, N_up, K_up, K_lo, cus=CUS):
    from ai_font_renderer_amd import _lib
    su, sl, nb, ws = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = _lib.lib().afr_op_linear_chain_plan(B, N_up, K_up, K_lo, cus, C.byref(su), C.byref(sl), C.byref(nb), C.byref(ws))
    return (rc, su.value, sl.value, nb.value, ws.value)


def _glyph_plan(dtype, flags=0, hidden=(1024, 1024), max_batch=8192):
    from ai_font_renderer_amd import _lib
    c = _lib.AfrConfig()
    c.kind, c.dtype, c.max_batch, c.vocab, c.embed_dim, c.out_h, c.out_w = _lib.AFR_KIND_GLYPH, dtype, max_batch, 96, 32, 32, 32
    c.n_hidden, c.n_fonts, c.seed, c.reserved = len(hidden), 8, 1, flags
    for i, h in enumerate(hidden):
        c.hidden[i] = h
    plan = C.c_void_p()
    _lib.check(_lib.lib().afr_plan_create(C.byref(c), C.byref(plan)))
    return plan


def test_planner_accepts_c3():
    from ai_font_renderer_amd import _lib
    rc, su, sl, nb, ws = _plan(*C3)
    assert (rc, su, sl, nb) == (0, 8, 8, 512)
    # two cooperative pairs' slices (16 tiles x 8 slices x 256 KiB each) and counters, and one hand-off counter per 256 rows
    pair = 16 * 8 * 256 * 256 * 4 + 256
    assert ws == 2 * pair + 256
    assert _plan(8008, 1024, 1024, 1024)[:4] == (0, 8, 8, 512)          # a ragged last row block chains as well
    assert _plan(*C3, cus=255)[0] == _lib.AFR_EUNSUPPORTED               # a CU per workgroup of a pair, or two launches


def test_planner_refuses_where_the_step_falls_back():
    """A batch, a width and a dtype at which the step keeps the two grouped launches."""
    from ai_font_renderer_amd import _lib
    lib, EU = _lib.lib(), _lib.AFR_EUNSUPPORTED
    # batch 4096: the pairs are 64 + 64 blocks of 256x256 tiles, too few for the cooperative 256x256 launch (192..272)
    assert _plan(4096, 1024, 1024, 1024)[0] == EU and b"chained" in lib.afr_last_error()
    # hidden width 512 below the output layer: dX_up has 64 blocks, dW_lo 2 x 2 tiles x 16 slices -- not a cooperative split
    assert _plan(8192, 1024, 512, 512)[0] == EU
    # a 2048-wide layer below C3's hidden layer: its pair is 256 + 256 blocks, beyond one round of 256x256 tiles (192..272)
    assert _plan(8192, 1024, 1024, 2048)[0] == EU
    assert _plan(8192, 2048, 1024, 1024)[0] == 0                          # (a wider OUTPUT layer chains: 8 x 4 tiles x 4 slices = 128 blocks)
    # dtype: the plans of the same model in f32 and bf16x3 never chain, the bf16 one does; nor does a switch that takes a pair
    # off the cooperative body, nor the chain's own switch
    for dtype, flags, want in ((_lib.AFR_BF16, 0, 1), (_lib.AFR_F32, 0, 0), (_lib.AFR_BF16X3, 0, 0), (_lib.AFR_BF16, 256, 0),
                               (_lib.AFR_BF16, 32, 0), (_lib.AFR_BF16, 2, 0)):
        plan = _glyph_plan(dtype, flags)
        try:
            assert lib.afr_plan_pair_chain(plan, 8192, CUS) == want, (dtype, flags)
            assert lib.afr_plan_pair_chain(plan, 4096, CUS) == 0
            assert lib.afr_plan_pair_chain(plan, 8192, 128) == 0
        finally:
            lib.afr_plan_destroy(plan)
    one_hidden = _glyph_plan(_lib.AFR_BF16, hidden=(1024,))               # the layer below the output layer is the folded first layer
    try:
        assert lib.afr_plan_pair_chain(one_hidden, 8192, CUS) == 0
    finally:
        lib.afr_plan_destroy(one_hidden)


def test_smallest_chained_triple():
    """On the grid of 256-multiples (batch to 8192, widths to 2048) nothing with fewer multiply-adds than C3 chains; SMALLEST chains,
    with C3's tiling, and no extent of it can shrink by 8."""
    from ai_font_renderer_amd import _lib
    B0, N0, K0, L0 = C3
    work0 = B0 * (N0 * K0 + K0 * L0)
    for B in range(256, 8192 + 1, 256):
        for N_up in range(256, 2048 + 1, 256):
            for K_up in range(256, 2048 + 1, 256):
                for K_lo in range(256, 2048 + 1, 256):
                    if B * (N_up * K_up + K_up * K_lo) < work0:
                        assert _plan(B, N_up, K_up, K_lo)[0] != 0, (B, N_up, K_up, K_lo)
    assert _plan(*SMALLEST)[:4] == _plan(*C3)[:4] == (0, 8, 8, 512)
    for k in range(4):
        less = tuple(v - 8 * (j == k) for j, v in enumerate(SMALLEST))
        assert _plan(*less)[0] == _lib.AFR_EUNSUPPORTED, less


def _block(shape, b):
    from ai_font_renderer_amd import _lib
    ph, m, tm, tn, z = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = _lib.lib().afr_op_linear_chain_block(*shape, b, C.byref(ph), C.byref(m), C.byref(tm), C.byref(tn), C.byref(z))
    return rc, ph.value, (m.value, tm.value, tn.value, z.value)


def _check_map(shape):
    from ai_font_renderer_amd import _lib
    B, N_up, K_up, K_lo = shape
    rc, su, sl, nb, _ = _plan(*shape)
    assert rc == 0
    t = lambda n: (n + 255) // 256
    # member -> (row tiles, column tiles, slices): 0 = dW_up [N_up][K_up], 1 = dx_up [B][K_up], 2 = dW_lo [K_up][K_lo], 3 = dx_lo [B][K_lo]
    dims = {0: (t(N_up), t(K_up), su), 1: (t(B), t(K_up), 1), 2: (t(K_up), t(K_lo), sl), 3: (t(B), t(K_lo), 1)}
    count = {m: d[0] * d[1] * d[2] for m, d in dims.items()}
    assert count[1] == count[2] and count[0] == count[3] and nb == sum(count.values())      # the swapped roles match
    seen = {0: {}, 1: {}}
    for b in range(nb):
        rc, ph, (m, tm, tn, z) = _block(shape, b)
        assert rc == 0
        # the grid is [dW_up | dx_up | dW_lo | dx_lo]: the upper pair (phase 0) is handed out first, the lower pair's long role
        # (dW_lo) follows the upper pair's short one (dx_up) onto the CUs
        assert m == sum(b >= sum(count[k] for k in range(j + 1)) for j in range(3)) and ph == (m >= 2), (b, ph, m)
        assert (m, tm, tn, z) not in seen[ph], (b, ph, seen[ph][(m, tm, tn, z)])
        seen[ph][(m, tm, tn, z)] = b
    for ph, members in ((0, (0, 1)), (1, (2, 3))):
        want = {(m, i, j, z) for m in members for i in range(dims[m][0]) for j in range(dims[m][1]) for z in range(dims[m][2])}
        assert set(seen[ph]) == want and len(want) == nb // 2, (ph, len(seen[ph]), len(want))
    assert _block(shape, nb)[0] == _lib.AFR_EINVAL and _block(shape, -1)[0] == _lib.AFR_EINVAL


def test_block_map_covers_every_block_of_the_four_products_once_per_phase():
    _check_map(C3)
    _check_map((8008, 1024, 1024, 1024))
    _check_map(SMALLEST)
