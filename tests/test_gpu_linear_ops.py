"""GPU: the Linear products' step-only tails one launch at a time through afr_op_linear (csrc/gemm.hip; the launch descriptions
and launchers of afr_train_step), against the fp64 checker tests/linear_ref.py.

CHAINED COMPARISON.  Nothing is compared across a discontinuity and no element is left out: the pre-activation / gradient of a
launch is compared with fp64; what a fused tail makes of it is compared with the checker applied to the kernel's OWN value, taken
from the same launch description without that tail (afr.h: fused and unfused paths leave the same bits).

BOUNDS (tests/linear_ref.py; none taken from what the kernels give): f32 results (2e-6 sqrt(R) + 1e-6) max(1, max|ref|), R the
reduction length (test_gpu_ops); AFR_BF16X3 products test_gpu_bf16x3's bound; bf16 results one bf16 ulp (2^-8 |ref|) on top;
mask_out, gates, gathers, Lion, the bf16 shadow: exact.  du from the own pre-activation: 1e-6 (f32) of the largest |du| -- the
measure of test_gpu_ops.test_mse_grad_matches_oracle; at most four f32 roundings of values <= 1 sit between u and du -- and in bf16
2^-8 |du| per element on top; the loss 1e-5 relative (test_c3_fused_loss_epilogue_equals_unfused_loss_kernel's bound).  Fused AdamW
from random m, v in (0, 1], t = 3: the weights within the project's 3e-6 max(1, max|p|) of fp64 AdamW on the own gradient; m and v
within 3e-6 max(1, max|m|), 3e-6 max(1, max|v|) -- they live at the gradient's scale (up to 60, its square times 1 - beta2 up to
40), where 3e-6 absolute is below the float32 spacing; each is two or three roundings, 2^-24 relative apiece, from its inputs.

Every output -- y, dx, dW, slabs, db, p, m, v, shadow, mask -- has a leading dimension larger than its width and rows behind its
last row, prefilled with a sentinel that must survive; every launch is repeated once and must reproduce its bytes; every test
asserts the kernel its launch ran on.
"""
import functools

import pytest
import torch

from . import linear_ref as R
from . import lion_ref
from .op_harness import bits, twice
from .util import ratio

pytestmark = pytest.mark.gpu

SENT = {torch.float32: -768.0, torch.bfloat16: -768.0, torch.uint8: 0xA5, torch.int32: -7}
EXTRA = 3                                                   # rows behind the last row
ADAMW = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=5e-4, t=3)
LION = dict(lr=lion_ref.LR, beta1=lion_ref.B1, beta2=lion_ref.B2, eps=0.0, weight_decay=lion_ref.WD, t=1)
NAMES = {"f32": "gemm_f32<%d,%d>", "bf16x3": "gemm_bf16x3<%d,%d>"}


def kname(dtype, a, b, wide=False):
    """the symbol of the tile / ring kernel for operand layouts (a, b): 1 = k-strided"""
    return "gemm_bf16<%d,%d,%d>" % (a, b, 4 if wide else 2) if dtype == "bf16" else NAMES[dtype] % (a, b)


def tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def dev(t, dt=None):
    return (t if dt is None else t.to(dt)).contiguous().cuda()


def padded(rows, cols, dt, ld=None, init=None):
    """device buffer [rows + EXTRA][ld] of the sentinel, its [rows][cols] corner optionally holding `init`"""
    ld = ld or cols + 8
    buf = torch.full((rows + EXTRA, ld), SENT[dt], dtype=dt, device="cuda")
    if init is not None:
        buf[:rows, :cols] = init.to(dt).cuda()
    return buf


def take(buf, rows, cols):
    """the [rows][cols] corner on the CPU, after checking that nothing outside it changed"""
    c = buf.cpu()
    out = c[:rows, :cols].clone()
    c[:rows, :cols] = SENT[buf.dtype]
    assert bool((c == SENT[buf.dtype]).all()), "a launch wrote outside [%d][%d] of a [%d][%d] buffer" % (rows, cols, *buf.shape)
    return out


def untouched(buf):
    assert bool((buf == SENT[buf.dtype]).all())


@functools.lru_cache(maxsize=None)
def inputs(dtype, B, N, K, tid=3000):
    return R.linear_inputs(dtype, B, N, K, tid)


def gate_expect(d0, keep):
    """the gated input gradient: +0 where the gate is closed, the ungated launch's bits elsewhere"""
    e = d0.clone()
    e[~keep] = 0.0
    return e


# =============================================================================== 128x128 tile kernels: forward and its tails
TILE = (200, 136, 96)          # ragged in both tile dimensions, 2 x 2 tiles; the reduction over B is no whole K-tile
TILE2 = (264, 192, 128)


@functools.lru_cache(maxsize=None)
def own_fwd(dtype, B, N, K, wide=False):
    """The plain forward launch: checked against fp64, returned as the kernel's own pre-activation (stored values, float32)."""
    from .gpu_util import linear
    i = inputs(dtype, B, N, K)
    dt = tdt(dtype)
    x, W, b = dev(i["x"], dt), dev(i["W"], dt), dev(i["b"])

    def run():
        y = padded(B, N, dt)
        return linear(dtype, "fwd", B, N, K, y, x=x, W=W, bias=b, ld_out=y.shape[1]), {"y": take(y, B, N)}
    name, o = twice(run)
    assert name == kname(dtype, 0, 0, wide)
    ref = R.fwd(i["x"], i["W"], i["b"])
    absprod = R.abs_product(i["x"], i["W"].t()) if dtype == "bf16x3" else None
    assert ratio(o["y"].float(), ref, R.product_bound(dtype, K, ref, absprod, i["b"], out_bf16=dtype == "bf16")) <= 1.0, "forward %s" % dtype
    return o["y"].float()


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("shape", [TILE, TILE2])
def test_tile_forward_vs_fp64(dtype, shape):
    own_fwd(dtype, *shape)


def fused_loss_case(dtype, B, N, K, kind, tgt, rows, wide, table_rows):
    """A forward launch with the fused loss against the checker's loss head applied to the own pre-activation."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import linear
    u = own_fwd(dtype, B, N, K, wide)
    i = inputs(dtype, B, N, K)
    dt = tdt(dtype)
    T = table_rows if rows else B
    tu8 = R.targets_u8(4100 + T, T, N)
    tf = R.target_f32(tu8)
    rmap = R.row_map(B, T) if rows else None
    n = B * N * 3                                           # (a denominator that is not the element count)
    loss_ref, du_ref = R.loss_du(kind, u, R.gather(tf, rmap) if rows else tf, n)
    x, W, b = dev(i["x"], dt), dev(i["W"], dt), dev(i["b"])
    td = dev(tu8) if tgt == "u8" else dev(tf)
    tail = dict(target=td, target_dtype=_lib.AFR_TARGET_U8 if tgt == "u8" else _lib.AFR_TARGET_F32, loss_kind=_lib.LOSS_KINDS[kind], mean_elems=n)
    if rows:
        tail["target_rows"] = dev(rmap)
    tiles = ((B + 127) // 128) * ((N + 127) // 128)
    scratch = torch.zeros(1040 + tiles + 16, device="cuda")        # zero before the FIRST call; the second launch finds it re-armed
    acc = torch.zeros(1, device="cuda")
    reads = []

    def run():
        du = padded(B, N, dt)
        name = linear(dtype, "fwd", B, N, K, du, x=x, W=W, bias=b, ld_out=du.shape[1], loss_accum=acc, loss_scratch=scratch, **tail)
        reads.append(float(acc.item()))
        return name, {"du": take(du, B, N)}
    name, o = twice(run)
    assert name == kname(dtype, 0, 0, wide)
    assert not scratch[1040 + tiles:].any()
    du = o["du"].float()
    scale = float(du_ref.abs().max())
    print("%s %s %s rows=%d: loss %.8f (fp64 of the own u %.8f), max |du - ref| / max|du| %.3e" %
          (dtype, kind, tgt, rows, reads[0], float(loss_ref), float((du.double() - du_ref).abs().max()) / scale))
    assert abs(reads[0] - float(loss_ref)) <= 1e-5 * float(loss_ref)
    assert reads[1] == 2.0 * reads[0]                       # loss_accum += : the same float32 added to itself
    assert ratio(du, du_ref, 1e-6 * scale + (2.0 ** -8 * du_ref.abs() if dtype == "bf16" else 0.0)) <= 1.0, "du"
    if kind == "mse":
        assert not du[(u < 0) | (u > 1)].any()              # the clamp's gate, decided on the kernel's own u: exactly zero outside


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("kind", ["mse", "bce"])
@pytest.mark.parametrize("tgt", ["u8", "f32"])
@pytest.mark.parametrize("rows", [0, 1])
def test_tile_fused_loss_from_own_preactivation(dtype, kind, tgt, rows):
    fused_loss_case(dtype, *TILE, kind, tgt, rows, False, 77)


def mask_out_case(B, N, K, wide):
    from .gpu_util import linear
    i = inputs("bf16", B, N, K)
    x, W, b = dev(i["x"], torch.bfloat16), dev(i["W"], torch.bfloat16), dev(i["b"])
    ldm = N // 8 + 3

    def run():
        y, m = padded(B, N, torch.bfloat16), padded(B, N // 8, torch.uint8, ldm)
        name = linear("bf16", "fwd", B, N, K, y, x=x, W=W, bias=b, ld_out=y.shape[1], mask_out=m, ldmask=ldm)
        return name, {"y": take(y, B, N), "mask": take(m, B, N // 8)}
    name, o = twice(run)
    assert name == kname("bf16", 0, 0, wide)
    u = R.fwd(i["x"], i["W"], i["b"])
    assert ratio(o["y"].float(), u.clamp(min=0), R.f32_bound(K, u) + 2.0 ** -8 * u.clamp(min=0)) <= 1.0, "ReLU output"
    assert torch.equal(o["mask"], R.pack_bits(o["y"].float() > 0))           # exactly the packing of (stored output > 0)
    assert 0.2 < float((o["y"].float() > 0).float().mean()) < 0.95


@pytest.mark.parametrize("shape", [TILE, TILE2])
def test_tile_mask_out_is_the_packing_of_the_stored_output(shape):
    mask_out_case(*shape, False)


# ========================================================================================= 128x128 tile kernels: input gradient
@functools.lru_cache(maxsize=None)
def own_dx(dtype, B, N, K, wide=False):
    """The ungated input-gradient launch: checked against fp64, returned as stored (in the output's type)."""
    from .gpu_util import linear
    i = inputs(dtype, B, N, K)
    dt = tdt(dtype)
    dy, W = dev(i["dy"], dt), dev(i["W"], dt)

    def run():
        d = padded(B, K, dt)
        return linear(dtype, "dx", B, N, K, d, dy=dy, W=W, ld_out=d.shape[1]), {"dx": take(d, B, K)}
    name, o = twice(run)
    assert name == kname(dtype, 0, 1, wide)
    ref = R.dx(i["dy"], i["W"])
    absprod = R.abs_product(i["dy"], i["W"]) if dtype == "bf16x3" else None
    assert ratio(o["dx"].float(), ref, R.product_bound(dtype, N, ref, absprod, out_bf16=dtype == "bf16")) <= 1.0, "input gradient %s" % dtype
    return o["dx"]


def gated_dx(dtype, B, N, K, wide, **tail):
    from .gpu_util import linear
    i = inputs(dtype, B, N, K)
    dt = tdt(dtype)
    dy, W = dev(i["dy"], dt), dev(i["W"], dt)

    def run():
        d = padded(B, K, dt)
        return linear(dtype, "dx", B, N, K, d, dy=dy, W=W, ld_out=d.shape[1], **tail), {"dx": take(d, B, K)}
    name, o = twice(run)
    assert name == kname(dtype, 0, 1, wide)
    return o["dx"]


def mask_in_case(B, N, K, ldm, wide=False):
    d0 = own_dx("bf16", B, N, K, wide)
    keep = inputs("bf16", B, N, K)["aux"] > 0
    m = padded(B, K // 8, torch.uint8, ldm, init=R.pack_bits(keep))
    got = gated_dx("bf16", B, N, K, wide, mask_in=m, ldmask=ldm)
    assert torch.equal(bits(got), bits(gate_expect(d0, keep)))
    assert 0.3 < float(keep.float().mean()) < 0.7


# (B, N, K, ldmask): K / 8 = 17 bytes per row, dense and padded: the byte loads; K / 8 = 16, dense and padded by 8: 8-byte aligned
# rows, one load per lane and two shuffles ("wide bits")
@pytest.mark.parametrize("B,N,K,ldm", [(200, 96, 136, 17), (200, 96, 136, 19), (264, 192, 128, 16), (264, 192, 128, 24)])
def test_tile_input_gradient_gated_by_bits(B, N, K, ldm):
    mask_in_case(B, N, K, ldm)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
def test_tile_input_gradient_gated_by_activation(dtype):
    B, N, K = TILE
    d0 = own_dx(dtype, B, N, K)
    aux = inputs(dtype, B, N, K)["aux"]
    a = padded(B, K, tdt(dtype), init=aux)
    got = gated_dx(dtype, B, N, K, False, aux=a, ldaux=a.shape[1])
    assert torch.equal(bits(got), bits(gate_expect(d0, aux > 0)))


def aux_rows_case(B, N, K, T, wide=False):
    d0 = own_dx("bf16", B, N, K, wide)
    table = R.rounded("bf16", R.rnd(4300 + T, (T, K)))
    rmap = R.row_map(B, T)
    tab = padded(T, K, torch.bfloat16, init=table)
    got = gated_dx("bf16", B, N, K, wide, aux=tab, ldaux=tab.shape[1], aux_rows=dev(rmap))
    dense = R.gather(table, rmap)
    a = padded(B, K, torch.bfloat16, init=dense)
    mat = gated_dx("bf16", B, N, K, wide, aux=a, ldaux=a.shape[1])
    assert torch.equal(bits(got), bits(mat))                                  # the same launch on the materialised rows
    assert torch.equal(bits(got), bits(gate_expect(d0, dense > 0)))


def test_tile_input_gradient_gated_by_gathered_rows():
    aux_rows_case(*TILE, 77)


# ======================================================================================== 128x128 tile kernels: weight gradient
# (B, splitk): unsplit; three slices; a split whose LAST slice starts beyond B in every dtype (K-tile 32: slices of 64 -> the fifth
# starts at 256 > 200; bf16, K-tile 64: (200, 3) and (320, 4) have slices of 128 and an empty last one as well)
DW_CASES = [(200, 1), (200, 3), (200, 5), (320, 4)]


def dw_check(dtype, B, N, K, sk, o, wide=False):
    i = inputs(dtype, B, N, K)
    bk = R.BK[dtype]
    sl = R.k_slices(B, sk, bk)
    longest = max(e - a for a, e in sl)
    ref = R.dw_slices(i["dy"], i["x"], sk, bk)
    if dtype == "bf16x3":
        bound = torch.stack([R.x3_bound(e - a, R.abs_product(i["dy"][a:e].t(), i["x"][a:e])) for a, e in sl])
    else:
        bound = R.f32_bound(longest, ref)
    assert ratio(o["dW"].reshape(sk, N, K), ref, bound) <= 1.0, "weight-gradient slabs"
    cref = R.colsum_slices(i["dy"], sk, bk)
    assert ratio(o["db"], cref, R.f32_bound(longest, cref)) <= 1.0, "bias-gradient partials"
    for z, (a, e) in enumerate(sl):
        if a == e:                                           # a slice that starts at or beyond B: zeros, not stale memory
            assert not o["dW"].reshape(sk, N, K)[z].any() and not o["db"][z].any()
    return ref


def dw_launch(dtype, B, N, K, sk, wide=False):
    from .gpu_util import linear
    i = inputs(dtype, B, N, K)
    dt = tdt(dtype)
    dy, x = dev(i["dy"], dt), dev(i["x"], dt)

    def run():
        g, db = padded(sk * N, K, torch.float32), padded(sk, N, torch.float32)
        name = linear(dtype, "dw", B, N, K, g, dy=dy, x=x, ld_out=g.shape[1], splitk=sk, db=db, ld_db=db.shape[1])
        return name, {"dW": take(g, sk * N, K), "db": take(db, sk, N)}
    name, o = twice(run)
    assert name == kname(dtype, 1, 1, wide)
    return o


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("B,sk", DW_CASES)
def test_tile_weight_gradient_slabs_and_bias_partials(dtype, B, sk):
    _, N, K = TILE
    dw_check(dtype, B, N, K, sk, dw_launch(dtype, B, N, K, sk))


def opt_state(N, K, tid):
    """weights (bound 0.2), a random first moment and a positive second moment in (0, 1]"""
    return R.rnd(tid, (N, K), 0.2), R.rnd(tid + 1, (N, K), 0.5), R.rnd(tid + 2, (N, K), 0.5, 0.5).abs() + 2.0 ** -20


def opt_check(kind, g, p0, m0, v0, o, shadow):
    """The fused step's p, m, v (and bf16 shadow) against the optimizer on the launch's own gradient g."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import ptr, stream
    if kind == "adamw":
        for got, ref, what in zip((o["p"], o["m"], o["v"]), R.adamw(p0, g, m0, v0, **ADAMW), "pmv"):
            assert ratio(got, ref, 3e-6 * max(1.0, float(ref.abs().max()))) <= 1.0, "fused AdamW " + what
    else:                                                    # afr.h: every site applies the Lion operations bit for bit
        pd, md, gd = dev(p0), dev(m0), dev(g)
        _lib.check(_lib.lib().afr_op_lion(ptr(pd), ptr(gd), ptr(md), None, g.numel(), LION["lr"], LION["beta1"], LION["beta2"], LION["weight_decay"],
                                          1.0, None, 0.0, stream()))
        torch.cuda.synchronize()
        assert torch.equal(bits(o["p"]), bits(pd.cpu())) and torch.equal(bits(o["m"]), bits(md.cpu()))
        assert torch.equal(bits(o["v"]), bits(v0))           # Lion keeps one moment: v is not touched
    assert not torch.equal(o["p"], p0) and not torch.equal(o["m"], m0)
    if shadow:
        assert torch.equal(bits(o["shadow"]), bits(o["p"].to(torch.bfloat16)))


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("kind", ["adamw", "lion"])
def test_tile_weight_gradient_fused_optimizer_on_own_gradient(dtype, kind):
    from ai_font_renderer_amd import _lib
    from .gpu_util import linear
    B, N, K = TILE
    g = dw_launch(dtype, B, N, K, 1)["dW"]
    i = inputs(dtype, B, N, K)
    dt = tdt(dtype)
    dy, x = dev(i["dy"], dt), dev(i["x"], dt)
    p0, m0, v0 = opt_state(N, K, 4500)
    shadow = dtype == "bf16"

    def run():
        gout, db = padded(N, K, torch.float32), padded(1, N, torch.float32)
        p, m, v = (padded(N, K, torch.float32, init=t) for t in (p0, m0, v0))
        sh = padded(N, K, torch.bfloat16) if shadow else None
        tail = dict(shadow=sh) if shadow else {}
        name = linear(dtype, "dw", B, N, K, gout, dy=dy, x=x, ld_out=gout.shape[1], db=db, ld_db=db.shape[1], p=p, m=m, v=v,
                      opt_kind=_lib.OPT_KINDS[kind], **(ADAMW if kind == "adamw" else LION), **tail)
        untouched(gout)                                      # the gradient is not stored
        o = {"p": take(p, N, K), "m": take(m, N, K), "v": take(v, N, K), "db": take(db, 1, N)}
        if shadow:
            o["shadow"] = take(sh, N, K)
        return name, o
    name, o = twice(run)
    assert name == kname(dtype, 1, 1)
    opt_check(kind, g, p0, m0, v0, o, shadow)
    cref = R.colsum_slices(i["dy"], 1, R.BK[dtype])
    assert ratio(o["db"], cref, R.f32_bound(B, cref)) <= 1.0, "bias gradient beside the fused step"


# ============================================================ 256x128 ring (bf16; >= 232 tiles, >= 256 of reduction per slice)
RING_FWD = (7384, 1024, 256)           # 29 x 8 = 232 tiles of 256 x 128, the last row tile 216 rows
RING_DX = (7384, 256, 1024)            # the same grid for dx [7384][1024]
RING_DW = [(14848, 58), (15000, 58)]   # N = 512, K = 256: 2 x 2 tiles x 58 slices of 256; at 15000 slices of 320, one of 280, 11 empty


def test_ring_forward_vs_fp64():
    own_fwd("bf16", *RING_FWD, True)


@pytest.mark.parametrize("kind", ["mse", "bce"])
@pytest.mark.parametrize("tgt", ["u8", "f32"])
@pytest.mark.parametrize("rows", [0, 1])
def test_ring_fused_loss_from_own_preactivation(kind, tgt, rows):
    fused_loss_case("bf16", *RING_FWD, kind, tgt, rows, True, 250)


def test_ring_mask_out_is_the_packing_of_the_stored_output():
    mask_out_case(*RING_FWD, True)


def test_ring_forward_gathers_rows_of_a_table():
    """x_rows: the A operand's rows come from a 250-row table (rows ldx apart).  Bit-equal to the launch on the materialised rows,
    and within the fp64 bound."""
    from .gpu_util import linear
    B, N, K = RING_FWD
    i = inputs("bf16", B, N, K)
    T = 250
    table = R.rounded("bf16", R.rnd(4700, (T, K)))
    rmap = R.row_map(B, T)
    W, b = dev(i["W"], torch.bfloat16), dev(i["b"])
    tab = padded(T, K, torch.bfloat16, init=table)
    xm = dev(R.gather(table, rmap), torch.bfloat16)
    rd = dev(rmap)

    def run(gathered):
        def f():
            y = padded(B, N, torch.bfloat16)
            tail = dict(x=tab, ldx=tab.shape[1], x_rows=rd) if gathered else dict(x=xm)
            return linear("bf16", "fwd", B, N, K, y, W=W, bias=b, ld_out=y.shape[1], **tail), {"y": take(y, B, N)}
        return f
    ng, og = twice(run(True))
    nm, om = twice(run(False))
    assert ng == nm == kname("bf16", 0, 0, True)
    assert torch.equal(bits(og["y"]), bits(om["y"]))
    ref = R.fwd(R.gather(table, rmap), i["W"], i["b"])
    assert ratio(og["y"].float(), ref, R.product_bound("bf16", K, ref, out_bf16=True)) <= 1.0, "gathered forward"


def test_ring_input_gradient_gated_by_wide_bits():
    B, N, K = RING_DX
    mask_in_case(B, N, K, K // 8 + 8, True)


def test_ring_input_gradient_gated_by_gathered_rows():
    aux_rows_case(*RING_DX, 250, True)


@pytest.mark.parametrize("B,sk", RING_DW)
def test_ring_weight_gradient_slabs_and_bias_partials(B, sk):
    N, K = 512, 256
    sl = R.k_slices(B, sk, 64)
    assert sum(1 for a, e in sl if a == e) == (0 if B == 14848 else 11)
    dw_check("bf16", B, N, K, sk, dw_launch("bf16", B, N, K, sk, True))


# ====================================================================================================== grouped launches
# The cooperative 256x256 pair: the smallest PAIR_CASES shape of test_gpu_tails.py and its ragged neighbour in K (the planner takes
# no other batch at N = 256: 8 slices of exactly 256 rows).  The 256x128 pair: the smallest batch (a multiple of 8) at N = 256 and
# K = 1016 -- eight ragged column tiles of the input gradient -- for which afr_op_linear_pair_plan answers a grouped, non-cooperative
# launch: 29 x 8 = 232 tiles, 15 slabs (test_linear_ref_cpu.py holds both answers true).
PAIR_256 = [(2048, 256, 3712), (2048, 256, 3704)]
PAIR_128 = (7176, 256, 1016)


def pair_launch(B, N, K, name_want, **variant):
    """One AFR_LIN_PAIR launch (twice).  variant: rows (x through a row map), bits (mask_in), aux_rows, opt ('adamw' | 'lion')."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import linear, linear_pair_plan
    t256, sk, coop, need = linear_pair_plan(B, N, K)
    i = inputs("bf16", B, N, K)
    bf = torch.bfloat16
    dy, W = dev(i["dy"], bf), dev(i["W"], bf)
    W0 = W.clone()
    tail = {}
    if variant.get("rows"):
        T = 1001
        table, rmap = R.rounded("bf16", R.rnd(4800, (T, K))), R.row_map(B, T)
        x = padded(T, K, bf, init=table)
        tail.update(ldx=x.shape[1], x_rows=dev(rmap))
    else:
        x = dev(variant["x"] if "x" in variant else i["x"], bf)
    if variant.get("bits"):
        m = padded(B, K // 8, torch.uint8, variant["bits"], init=R.pack_bits(i["aux"] > 0))
        tail.update(mask_in=m, ldmask=variant["bits"])
    if variant.get("aux_rows"):
        T = 1001
        atab = padded(T, K, bf, init=R.rounded("bf16", R.rnd(4810, (T, K))))
        tail.update(aux=atab, ldaux=atab.shape[1], aux_rows=dev(R.row_map(B, T, 5)))
    opt = variant.get("opt")
    p0, m0, v0 = opt_state(N, K, 4900)
    rows_dw = N if coop else sk * N

    def run():
        g, db, d = padded(rows_dw, K, torch.float32), padded(sk, N, torch.float32), padded(B, K, bf)
        ws = torch.full((max(need, 256),), 0x5A, dtype=torch.uint8, device="cuda")          # dirty on purpose: the entry owns its state
        t = dict(tail)
        if opt:
            p, mm, v = (padded(N, K, torch.float32, init=s) for s in (p0, m0, v0))
            sh = padded(N, K, bf)
            t.update(p=p, m=mm, v=v, shadow=sh, opt_kind=_lib.OPT_KINDS[opt], **(ADAMW if opt == "adamw" else LION))
        name = linear("bf16", "pair", B, N, K, g, dy=dy, x=x, W=W, out2=d, workspace=ws if coop else None, ld_out=g.shape[1], db=db,
                      ld_db=db.shape[1], **t)
        o = {"db": take(db, sk, N), "dX": take(d, B, K)}
        if opt:
            untouched(g)
            o.update(p=take(p, N, K), m=take(mm, N, K), v=take(v, N, K), shadow=take(sh, N, K))
        else:
            o["dW"] = take(g, rows_dw, K)
        return name, o
    name, o = twice(run)
    assert name == name_want
    assert torch.equal(bits(W), bits(W0))                    # a fused step writes the shadow, never the operand the dX member reads
    o.update(splitk=sk, coop=coop)
    return o


@functools.lru_cache(maxsize=None)
def own_pair(B, N, K):
    """The pair without tails, checked against fp64: dW (or its slabs), the per-slice db, dX."""
    o = pair_launch(B, N, K, "gemm_bf16_group256" if (B, N, K) in PAIR_256 else "gemm_bf16_group")
    i = inputs("bf16", B, N, K)
    sk = o["splitk"]
    sl = R.k_slices(B, sk, 64)
    if o["coop"]:
        ref = R.dw(i["dy"], i["x"])
        assert ratio(o["dW"], ref, R.f32_bound(B, ref)) <= 1.0, "cooperative weight gradient"
    else:
        ref = R.dw_slices(i["dy"], i["x"], sk, 64)
        assert ratio(o["dW"].reshape(sk, N, K), ref, R.f32_bound(max(e - a for a, e in sl), ref)) <= 1.0, "weight-gradient slabs of the pair"
    cref = R.colsum_slices(i["dy"], sk, 64)
    assert ratio(o["db"], cref, R.f32_bound(max(e - a for a, e in sl), cref)) <= 1.0, "per-slice bias gradient of the pair"
    dref = R.dx(i["dy"], i["W"])
    assert ratio(o["dX"].float(), dref, R.product_bound("bf16", N, dref, out_bf16=True)) <= 1.0, "input gradient of the pair"
    return o


@pytest.mark.parametrize("B,N,K", PAIR_256 + [PAIR_128])
def test_pair_vs_fp64(B, N, K):
    o = own_pair(B, N, K)
    assert (o["splitk"], o["coop"]) == ((8, 1) if (B, N, K) in PAIR_256 else (15, 0))


def same_but(o, own, *changed):
    for k in own:
        if k not in changed and torch.is_tensor(own[k]) and k in o:
            assert torch.equal(bits(o[k]), bits(own[k])), "%s differs from the launch without the tail" % k


@pytest.mark.parametrize("B,N,K", PAIR_256)
def test_cooperative_pair_gathers_x_through_a_row_map(B, N, K):
    """b_rowmap: the weight-gradient member reads x through a combination index over a 1001-row table.  Bit-equal to the pair on
    the materialised rows; that pair is within the fp64 bound."""
    table, rmap = R.rounded("bf16", R.rnd(4800, (1001, K))), R.row_map(B, 1001)
    xg = R.gather(table, rmap)
    got = pair_launch(B, N, K, "gemm_bf16_group256", rows=True)
    mat = pair_launch(B, N, K, "gemm_bf16_group256", x=xg)
    same_but(got, mat)
    ref = R.dw(inputs("bf16", B, N, K)["dy"], xg)
    assert ratio(got["dW"], ref, R.f32_bound(B, ref)) <= 1.0, "gathered weight gradient"
    same_but(got, own_pair(B, N, K), "dW")                    # db and dX do not read x


@pytest.mark.parametrize("B,N,K", PAIR_256 + [PAIR_128])
def test_pair_input_gradient_gated_by_bits(B, N, K):
    """K / 8 = 464 bytes padded to 472 (8-byte rows: wide bits); 463 padded to 465 and 127 to 129 (byte loads)."""
    own = own_pair(B, N, K)
    o = pair_launch(B, N, K, "gemm_bf16_group256" if own["coop"] else "gemm_bf16_group", bits={3712: 472, 3704: 465, 1016: 129}[K])
    same_but(o, own, "dX")
    assert torch.equal(bits(o["dX"]), bits(gate_expect(own["dX"], inputs("bf16", B, N, K)["aux"] > 0)))


@pytest.mark.parametrize("B,N,K", PAIR_256 + [PAIR_128])
def test_pair_input_gradient_gated_by_gathered_rows(B, N, K):
    own = own_pair(B, N, K)
    o = pair_launch(B, N, K, "gemm_bf16_group256" if own["coop"] else "gemm_bf16_group", aux_rows=True)
    same_but(o, own, "dX")
    keep = R.gather(R.rounded("bf16", R.rnd(4810, (1001, K))), R.row_map(B, 1001, 5)) > 0
    assert torch.equal(bits(o["dX"]), bits(gate_expect(own["dX"], keep)))


@pytest.mark.parametrize("B,N,K", PAIR_256)
@pytest.mark.parametrize("kind", ["adamw", "lion"])
def test_cooperative_pair_fused_optimizer_on_own_gradient(B, N, K, kind):
    """The optimizer step on the cooperative member: p, m, v, shadow from the pair's own gradient; db and dX bit for bit those of the
    launch without the step -- the dX member read the OLD weights."""
    own = own_pair(B, N, K)
    o = pair_launch(B, N, K, "gemm_bf16_group256_lion" if kind == "lion" else "gemm_bf16_group256", opt=kind)
    same_but(o, own)
    opt_check(kind, own["dW"], *opt_state(N, K, 4900), o, True)
