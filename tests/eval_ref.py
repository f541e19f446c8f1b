"""Restatements of the evaluation kernel (csrc/elementwise.hip eval_rows_kernel, include/afr.h afr_eval) in numpy.

fp64: q, t8, stats and loss_rows from the formulas of the header.  float32: loss_rows in the kernel's documented summation
order, from which the longest chain of additions D(cols) follows -- the way tests/test_gpu_clip.py derives its own.

The keyword arguments named fault_* plant one deliberate mistake each; tests/test_eval_cpu.py shows that every one of them
misses the bounds the GPU tests hold the kernel to by 10x or more, so those bounds can tell a wrong kernel from a right one.
"""
import numpy as np

WAVE_COLS = 2048          # up to here one wave (64 lanes) owns a row; beyond, one 256-lane workgroup
MAX_BLOCKS = 2048         # the grid cap: 4 rows per block in wave form, 1 in workgroup form
EPS32 = 2.0 ** -24        # one float32 rounding, relative


def lanes(cols):
    return 64 if cols <= WAVE_COLS else 256


def chain_depth(cols):
    """D(cols): the longest chain of float32 additions behind one loss_rows value.  Lane 0 adds 8 terms for each of its
    ceil(cols / (8 L)) groups, the wave butterfly adds 6 times, a workgroup adds its four waves (3)."""
    L = lanes(cols)
    return 8 * -(-cols // (8 * L)) + 6 + (3 if L == 256 else 0)


def mse_bound(cols, terms_sum_over_cols):
    """|float32 loss_rows - fp64| <= (D + 4) 2^-24 sum_i term_i / cols: D additions, and one rounding each for the subtraction,
    the square, the division and k / 255.0f (which fp64 takes from the float32 value of t)."""
    return (chain_depth(cols) + 4) * EPS32 * terms_sum_over_cols


def targets_f32(target, fault_div256=False):
    """t as the loss kernels form it: (float)k / 255.0f for uint8 pixels, the float itself otherwise."""
    if target.dtype == np.uint8:
        return target.astype(np.float32) / np.float32(256.0 if fault_div256 else 255.0)
    return target.astype(np.float32)


def t8_of(target):
    """The 8-bit level of a target: k, or rintf(t * 255.f) limited to 0..255 (round half to even, as rintf)."""
    if target.dtype == np.uint8:
        return target.astype(np.int64)
    r = np.rint(target.astype(np.float32) * np.float32(255.0))
    return np.clip(np.nan_to_num(r, nan=0.0), 0, 255).astype(np.int64)


def head64(u, loss):
    u = u.astype(np.float64)
    if loss == "bce":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-u))
    return np.clip(u, 0.0, 1.0)


def q64(u, loss, fault_round=False):
    """(uint8)(y * 255), truncating, in fp64; a NaN gives level 0."""
    v = head64(u, loss) * 255.0
    v = np.where(np.isnan(v), 0.0, v)
    return (np.rint(v) if fault_round else np.floor(v)).astype(np.int64)


def stats_of(q, t8, fault_gt2=False):
    """[rows, 4]: #(d >= 1), #(d >= 2), max d, #((q >= 128) != (t8 >= 128)) with d = |q - t8|."""
    d = np.abs(q.astype(np.int64) - t8.astype(np.int64))
    two = (d > 2) if fault_gt2 else (d >= 2)
    return np.stack([(d >= 1).sum(1), two.sum(1), d.max(1), ((q >= 128) != (t8 >= 128)).sum(1)], axis=1).astype(np.int64)


def terms64(u, t, loss):
    """The per-pixel loss terms in fp64, from the float32 values of u and t; a NaN u gives a NaN term."""
    u, t = u.astype(np.float64), t.astype(np.float64)
    if loss == "bce":
        return np.maximum(u, 0.0) - t * u + np.log1p(np.exp(-np.abs(u)))
    d = np.clip(u, 0.0, 1.0) - t
    return np.where(np.isnan(u), np.nan, d * d)


def gather(target, rowmap, fault_ignore_rowmap=False):
    """The target rows of the batch: row r of u is compared with row rowmap[r] of target (no map: row r)."""
    if rowmap is None:
        return target
    return target[:len(rowmap)] if fault_ignore_rowmap else target[np.asarray(rowmap)]


def loss_rows64(u, target, loss, rowmap=None):
    t = targets_f32(gather(target, rowmap)[:len(u)])
    return terms64(u.astype(np.float32), t, loss).sum(1) / u.shape[1]


def loss_rows32(u, target, loss="mse", rowmap=None, fault_drop_last_group=False, fault_div256=False, fault_no_div=False,
                fault_ignore_rowmap=False):
    """loss_rows in float32 and in the kernel's order: lane partials over the lane's groups in ascending order (pixel by pixel,
    from 0.f), the butterfly of wave_sum (v += v[lane ^ o], o = 32 .. 1), the waves of a workgroup in wave order, one division."""
    f32 = np.float32
    u = u.astype(f32)
    rows, cols = u.shape
    t = targets_f32(gather(target, rowmap, fault_ignore_rowmap)[:rows], fault_div256)
    if loss == "bce":
        term = (np.maximum(u, f32(0)) - t * u).astype(f32) + np.log1p(np.exp(-np.abs(u))).astype(f32)
    else:
        d = (np.clip(u, f32(0), f32(1)) - t).astype(f32)
        term = np.where(np.isnan(u), f32(np.nan), (d * d).astype(f32))
    term = term.astype(f32)
    L, G = lanes(cols), cols // 8
    if fault_drop_last_group:
        term = term.copy()
        term[:, 8 * (G - 1):] = 0
    trips = -(-G // L)
    pad = np.zeros((rows, trips * L * 8), f32)
    pad[:, :cols] = term
    pad = pad.reshape(rows, trips, L, 8)
    live = (np.arange(trips * L).reshape(trips, L) < G)            # a lane adds nothing for a group it does not have
    acc = np.zeros((rows, L), f32)
    for j in range(trips):
        for k in range(8):
            acc = np.where(live[j][None, :], (acc + pad[:, j, :, k]).astype(f32), acc)
    v = acc.reshape(rows, L // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lane ^ o]).astype(f32)
    s = v[:, 0, 0]
    for w in range(1, L // 64):
        s = (s + v[:, w, 0]).astype(f32)
    return s if fault_no_div else (s / f32(cols)).astype(f32)
