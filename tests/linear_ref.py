"""Checker for the Linear products' step-only tails (afr_op_linear; csrc/gemm.hip): the three products of
y[B][N] = x[B][K] . W[N][K]^T + b and what a training step hangs on them, in torch fp64 and with nothing from the library --
K-slices and their column sums, the ReLU mask as bits, row gathers, the loss heads as functions of a given pre-activation, AdamW
with the step's scalars folded as the host folds them -- plus the bounds the GPU tests hold the kernels to and the deterministic
inputs the CPU and GPU tests share.

THE BOUNDS are the suite's own or follow from a number format; none was taken from what the kernels give.
  * an f32 result of a reduction of length R (a product element, a column sum), from any dtype:
    (2e-6 sqrt(R) + 1e-6) max(1, max|ref|) -- test_gpu_ops' bound;
  * AFR_BF16X3 products: (3 2^-16 + R 2^-24) sum_k |a_k b_k| per element (+ one f32 rounding of the bias add) -- test_gpu_bf16x3's;
  * a bf16 result: 2^-8 |ref| per element (one bf16 ulp) on top of the f32 bound;
  * fused AdamW against fp64: 3e-6 max(1, max|p|); the loss: 1e-5 relative; du: 1e-6 (f32), 2^-8 (bf16) -- see the GPU tests.
"""
import math

import numpy as np
import torch

from oracle import afr_oracle as oracle

from . import bce_ref
from .util import synth

F64 = torch.float64
BK = {"f32": 32, "bf16x3": 32, "bf16": 64}      # the K-tile of each dtype's kernels (gemm.hip f32k / x3k / bf16k)


# ----------------------------------------------------------------------------------------------- inputs
def rnd(tid, shape, bound=1.0, center=0.0):
    return torch.from_numpy(synth.hash_uniform(tid, shape, bound)) + center


def rounded(dtype, t):
    """The operand as the kernels of `dtype` see it: bf16 operands are rounded on the host first, bf16x3 and f32 take f32."""
    return t.to(torch.bfloat16).to(torch.float32) if dtype == "bf16" else t.to(torch.float32)


def linear_inputs(dtype, B, N, K, tid=3000):
    """x [B][K] (bound 1), W [N][K] (bound 0.2), b [N] (0.5 +- 0.5), dy [B][N] (bound 1), aux [B][K] (bound 1), as the dtype's
    kernels see them.  About a third to a half of x . W^T + b then lies inside (0, 1) (test_linear_ref_cpu.py holds that true)."""
    return {"x": rounded(dtype, rnd(tid + 1, (B, K))), "W": rounded(dtype, rnd(tid + 2, (N, K), 0.2)), "b": rnd(tid + 3, (N,), 0.5, 0.5),
            "dy": rounded(dtype, rnd(tid + 4, (B, N))), "aux": rounded(dtype, rnd(tid + 5, (B, K)))}


def row_map(n, height, tid=0):
    """int32 [n] into a table of `height` rows: not monotone, with repeats, with row 0 and the table's last row."""
    i = np.arange(n, dtype=np.int64)
    r = (i * 37 + 11 + tid + (i * i) // 3) % height
    r[0], r[1], r[2], r[n - 1] = height - 1, 0, 0, height - 1
    return torch.from_numpy(r.astype(np.int32))


def targets_u8(tid, rows, cols):
    return torch.from_numpy(synth.hash_u8(tid, (rows, cols)))


def target_f32(tu8):
    """k / 255.0f in float32: the value the loss sees for the 8-bit pixel k."""
    return (tu8.to(torch.float32) / np.float32(255.0)).to(torch.float32)


# ------------------------------------------------------------------------------------------- the products
def fwd(x, W, b):
    """u [B][N] = x . W^T + b"""
    return x.to(F64) @ W.to(F64).t() + b.to(F64)


def dx(dy, W):
    """dx [B][K] = dy . W (ungated)"""
    return dy.to(F64) @ W.to(F64)


def dw(dy, x):
    """dW [N][K] = dy^T . x"""
    return dy.to(F64).t() @ x.to(F64)


def gather(table, rows):
    """row b of the result = row rows[b] of the table"""
    return table[rows.long()]


def k_slices(R, splitk, bk):
    """k_range of gemm.hip: `splitk` equal slices of whole bk-tiles over a reduction of length R, the last one clipped to R; a slice
    that starts at or beyond R is empty (beg == end)."""
    klen = -(-(-(-R // splitk)) // bk) * bk
    out = []
    for z in range(splitk):
        beg = z * klen
        end = min(R, beg + klen)
        out.append((beg, end) if end > beg else (min(beg, R), min(beg, R)))
    return out


def colsum_slices(dy, splitk, bk):
    """db partials [splitk][N]: the column sums of dy over each K-slice of the batch (an empty slice contributes zeros)"""
    d = dy.to(F64)
    return torch.stack([d[a:e].sum(0) for a, e in k_slices(d.shape[0], splitk, bk)])


def dw_slices(dy, x, splitk, bk):
    """dW partial slabs [splitk][N][K]"""
    d, xx = dy.to(F64), x.to(F64)
    return torch.stack([d[a:e].t() @ xx[a:e] for a, e in k_slices(d.shape[0], splitk, bk)])


def abs_product(a, b_t):
    """sum_k |a_k| |b_k| per output element, the scale of the bf16x3 bound: a [M][R], b_t [R][N]"""
    return a.to(F64).abs() @ b_t.to(F64).abs()


# ------------------------------------------------------------------------------------------------- bits
def pack_bits(mask):
    """bool [M][N] (N a multiple of 8) -> uint8 [M][N / 8]: bit n & 7 of byte [m][n / 8]"""
    m = mask.to(torch.uint8).reshape(mask.shape[0], -1, 8)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32)
    return (m.to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_bits(bits, N):
    b = bits.to(torch.int32)[:, : N // 8]
    return torch.stack([(b >> r) & 1 for r in range(8)], dim=-1).reshape(bits.shape[0], N).bool()


# ------------------------------------------------------------------------------------------------- loss
def loss_du(kind, u, t, mean_elems):
    """(loss, du) of the pre-activation u [B][N] against targets t [B][N] in fp64: kind "mse" = clamp(u, 0, 1) head + MSE
    (oracle.mse_loss_grad), "bce" = sigmoid head + BCE with logits (bce_ref); the mean's denominator is mean_elems."""
    if kind == "mse":
        return oracle.mse_loss_grad(u.to(F64), t.to(F64), total_elems=mean_elems)
    return bce_ref.bce_logits_loss_grad(u.to(F64), t.to(F64), total_elems=mean_elems)


# --------------------------------------------------------------------------------------------- optimizer
def f32(v):
    return float(np.float32(v))


def adamw(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay):
    """torch.optim.AdamW in fp64 with the step's scalars folded as the library's host folds them (bias corrections in double,
    every folded scalar rounded to float32): decay = 1 - lr wd, step = lr / (1 - b1^t), r = 1 / sqrt(1 - b2^t);
    p *= decay; m += (g - m)(1 - b1); v = b2 v + (1 - b2) g g; p -= step m / (sqrt(v) r + eps).  Returns (p, m, v)."""
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay)
    decay = f32(1.0 - f32(lr * wd))
    step = f32(lr / f32(1.0 - b1 ** t))
    r = f32(1.0 / math.sqrt(f32(1.0 - b2 ** t)))
    p, g, m, v = p.to(F64), g.to(F64), m.to(F64), v.to(F64)
    m = m + (g - m) * f32(1.0 - b1)
    v = b2 * v + f32(1.0 - b2) * g * g
    p = p * decay - step * (m / (v.sqrt() * r + eps))
    return p, m, v


# ------------------------------------------------------------------------------------------------ bounds
def f32_bound(R, ref):
    """test_gpu_ops' bound on an f32 result of a reduction of length R"""
    return (2e-6 * R ** 0.5 + 1e-6) * max(1.0, float(ref.abs().max()))


def x3_bound(R, absprod, ref=None, bias=None):
    """test_gpu_bf16x3's per-element bound on a split-bf16 product"""
    b = (3 * 2.0 ** -16 + R * 2.0 ** -24) * absprod
    if bias is not None:
        b = b + 2.0 ** -24 * (ref.abs() + bias.to(F64).abs())
    return b


def product_bound(dtype, R, ref, absprod=None, bias=None, out_bf16=False):
    """per-element bound (a tensor like ref) on a product element of `dtype` with reduction length R"""
    if dtype == "bf16x3":
        return x3_bound(R, absprod, ref, bias)
    b = torch.full_like(ref, f32_bound(R, ref))
    return b + 2.0 ** -8 * ref.abs() if out_bf16 else b
