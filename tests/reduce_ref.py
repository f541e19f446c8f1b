"""Checker for the slab reductions (csrc/elementwise.hip reduce_slabs_kernel, reduce_group_kernel) and for the optimizer step fused into
the grouped one (afr_op_reduce, afr_op_reduce_group_step): the float32 sum in the kernels' DOCUMENTED order, which only adds and is
therefore bit-exact; the same sum in fp64 with its a-priori bound; the cases, their inputs and their layout; and the checks that
tests/test_gpu_reduce_ops.py holds every launch to, stated here so that tests/test_reduce_ref_cpu.py can plant one fault at a time into a
host emulation of the launch (`emulate`) and see each check fail.  Nothing here needs a GPU.

ORDER (afr.h, DESIGN "Grouped reduce").  Fewer than 32 slabs: a = 0; a += v[s], s ascending.  32 slabs or more ("deep"): with per =
ceil(nslabs / 4) quarter g sums the slabs [g per, min(nslabs, (g + 1) per)) that way and the result is ((q0 + q1) + q2) + q3.
afr_op_reduce always takes the first form.

BOUND.  A float32 sum of nslabs values by any tree of nslabs - 1 additions is within (nslabs - 1) 2^-24 sum|v| of the exact sum (each
addition rounds once, relative 2^-24 of a partial sum that never exceeds sum|v| in magnitude; first order).  One slab: exact.

INPUTS.  Slab s holds (hashed uniform value in [-1, 1) + CENTER) * MAGS[s mod 5], the factors signed: consecutive slabs of like size
cancel, so that a rounding error made early is large against the final sum and the order of the additions shows in the bits (with
unsigned factors two orders of THREE slabs agree in two thirds of the columns: both results are within an ulp of the exact sum);
columns [n, stride) of every slab are NaN.  test_reduce_ref_cpu.py holds, for every case, that the documented order differs in
bits from the reversed order, and the deep order from the shallow one, in at least half of the columns.

LAYOUT.  The segments of a case lie in ONE flat buffer, not in the caller's order, with gaps of at least 64 floats between them, in
front of the first and behind the last; the gaps hold the harness's fill (NaN) and must keep it."""
import functools

import numpy as np
import torch

from . import linear_ref
from .groups_ref import LR_MULT_ND, WD_MULT_ND, f32_mul
from .op_harness import bits
from .util import ratio, synth

DEEP = 32                                   # afr_rtable_add: a segment of 32 slabs or more is summed in quarters
MAGS = (8.0, -8.0, 1.0, -2.0, 2.0)          # per-slab factors, by s mod 5
CENTER = 4.0                                # slab s holds (hashed uniform in [-1, 1) + CENTER) * MAGS[s mod 5]
GAP = 64                                    # floats between two segments, at the least
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the sums
def slab_groups(nslabs, deep=None):
    """the slabs of each partial sum, in the order they are added: one group (shallow) or the four quarters (deep)"""
    if not (nslabs >= DEEP if deep is None else deep):
        return [list(range(nslabs))]
    per = -(-nslabs // 4)
    return [list(range(g * per, min(nslabs, (g + 1) * per))) for g in range(4)]


def sum_groups(slabs, groups, n):
    """float32: every group summed from zero in its order, the partial sums then added in group order"""
    parts = []
    for idx in groups:
        a = np.zeros(n, dtype=np.float32)
        for s in idx:
            a = a + slabs[s, :n]
        parts.append(a)
    a = parts[0]
    for q in parts[1:]:
        a = a + q
    return a


def ordered_sum(slabs, nslabs, n):
    """the grouped reduce's result for slabs [nslabs][>= n] (numpy float32), bit for bit"""
    return sum_groups(slabs, slab_groups(nslabs), n)


def sum64(slabs, nslabs, n):
    return slabs[:nslabs, :n].astype(np.float64).sum(0)


def sum_bound(slabs, nslabs, n):
    return (nslabs - 1) * U24 * np.abs(slabs[:nslabs, :n].astype(np.float64)).sum(0)


def reduce_slabs_ref(slabs, nslabs, n, scale, old=None):
    """afr_op_reduce: (the sum in slab order) * scale (+ old).  -> the float32 forms that are legal per element: one where nothing
    is left to the compiler, two for an inexact product that is then added to (product rounded, then added; or one rounding of the
    fp64 value of sum * scale + old, the fused multiply-add)."""
    a = sum_groups(slabs, [list(range(nslabs))], n)
    prod = a * np.float32(scale)
    if old is None:
        return [prod]
    forms = [prod + old]
    exact = np.array_equal(prod.astype(np.float64), a.astype(np.float64) * float(np.float32(scale)))
    if not exact:
        forms.append((a.astype(np.float64) * float(np.float32(scale)) + old.astype(np.float64)).astype(np.float32))
    return forms


def differing_share(a, b):
    """share of the elements whose bits differ"""
    return float((a.view(np.int32) != b.view(np.int32)).mean())


# ------------------------------------------------------------------------------------------------ cases
def slab_values(tid, nslabs, n, stride):
    """[nslabs][stride] float32: (hashed value + CENTER) times the slab's factor, NaN behind column n"""
    v = synth.hash_uniform(tid, (nslabs, n), 1.0) + np.float32(CENTER)
    v *= np.array([MAGS[s % 5] for s in range(nslabs)], dtype=np.float32)[:, None]
    out = np.full((nslabs, stride), np.nan, dtype=np.float32)
    out[:, :n] = v
    return out


class Seg:
    """One segment: nslabs slabs of n elements, `stride` apart; off = its flat offset (set by Case); mult = its group's (lr_mult,
    wd_mult); tr = None or (shT offset in the case's transposed buffer, tN, tK)."""

    def __init__(self, nslabs, n, mult=(1.0, 1.0), tr=None, pad=None):
        self.nslabs, self.n, self.mult, self.tr = nslabs, n, mult, tr
        self.stride = n + (pad if pad is not None else 4 + 4 * (nslabs % 3))
        self.off = self.tid = None

    @property
    def label(self):
        return "s%dn%d@%d" % (self.nslabs, self.n, self.off)

    @functools.cached_property
    def slabs(self):
        return slab_values(self.tid, self.nslabs, self.n, self.stride)

    @functools.cached_property
    def own(self):
        return ordered_sum(self.slabs, self.nslabs, self.n)


ND = (LR_MULT_ND, WD_MULT_ND)               # groups_ref.two_groups' values for the tensors of its second group


class Case:
    """Segments in the CALLER's order; laid into the flat buffer in another order (the odd ones first, then the even ones from the
    back), each behind a gap of 64, 68 or 72 floats.  tr_total: elements of the transposed (bf16) buffer, 0 = none."""

    def __init__(self, name, segs, tid, tr_total=0):
        self.name, self.segs, self.tr_total = name, segs, tr_total
        k = len(segs)
        order = [i for i in range(k) if i % 2] + [i for i in reversed(range(k)) if i % 2 == 0]
        at = 0
        for j, i in enumerate(order):
            at += GAP + 4 * (j % 3)
            segs[i].off, segs[i].tid = at, tid + i
            at += segs[i].n
        self.total = at + GAP

    def mask(self):
        m = torch.zeros(self.total, dtype=torch.bool)
        for sg in self.segs:
            m[sg.off:sg.off + sg.n] = True
        return m

    def scatter(self, parts, fill=float("nan"), dtype=torch.float32):
        """the flat buffer that holds parts[i] (tensor or array) in segment i and `fill` in the gaps"""
        out = torch.full((self.total,), fill, dtype=dtype)
        for sg, part in zip(self.segs, parts):
            out[sg.off:sg.off + sg.n] = torch.as_tensor(part).reshape(-1).to(dtype)
        return out


SHALLOW_SLABS, SHALLOW_N = (1, 7, 8, 9, 17, 31), (4, 1000, 4 * 257, 4096)
DEEP_SLABS, DEEP_N = (32, 33, 35, 37, 40), (4, 4 * 65, 256)
CAP_SHALLOW, CAP_DEEP = (2, 4 * (1024 * 256 + 300)), (32, 4 * (1024 * 64 + 70))      # every block takes a second trip


def _mixed32():
    """32 segments of both modes; n = 4 .. 256: single-block segments between larger ones (the block -> segment scan)"""
    out = []
    for i in range(32):
        deep = i % 3 == 1
        nslabs = (32 + i) if deep else 1 + (i * 5) % 31
        n = (4, 260, 1028, 64, 4 * 70, 2052)[i % 6] if not deep else (4, 256, 4 * 65, 4 * 129)[i % 4]
        out.append(Seg(nslabs, n, ND if i % 2 else (1.0, 1.0)))
    return out


def _glyph_like():
    """W1 [64][32] with its transpose (tN 64, tK 32), deep; W2 [48][64] as two row ranges of 24 rows, each with shT = W2T + pc * 24 at pitch 48 (the
    column-split step's form), shallow; a bias without a transposed copy.  Transposed buffer: gap 64 | W1T 2048 | gap 64 | W2T 3072 | gap 64."""
    w2t = 64 + 2048 + 64
    return [Seg(24, 24 * 64, tr=(w2t, 48, 64)), Seg(36, 64 * 32, tr=(64, 64, 32)), Seg(5, 48, ND), Seg(24, 24 * 64, tr=(w2t + 24, 48, 64))], w2t + 3072 + 64


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("shallow-") or name.startswith("deep-"):
        n = int(name.split("-")[1])
        # (20 columns in all at n = 4: tensor ids at which the condition on the inputs holds for them)
        tid = {"shallow-4": 9200, "deep-4": 9000}.get(name, (12000 if name[0] == "s" else 9400) + n)
        return Case(name, [Seg(s, n) for s in (SHALLOW_SLABS if name[0] == "s" else DEEP_SLABS)], tid)
    if name == "cap-shallow":
        return Case(name, [Seg(*CAP_SHALLOW)], 7100)
    if name == "cap-deep":
        return Case(name, [Seg(*CAP_DEEP)], 7110)
    if name == "mixed32":
        return Case(name, _mixed32(), 7200)
    if name == "modes":                     # the fused launch's first set: shallow, deep, shallow
        return Case(name, [Seg(3, 4096), Seg(40, 256, ND), Seg(8, 1000)], 7300)
    if name == "glyph":
        segs, tr_total = _glyph_like()
        return Case(name, segs, 7400, tr_total)
    raise KeyError(name)


PLAIN_CASES = (["shallow-%d" % n for n in SHALLOW_N] + ["deep-%d" % n for n in DEEP_N] + ["cap-shallow", "cap-deep", "mixed32"])
FUSED_SETS = ("modes", "glyph")


# ------------------------------------------------------------------------------------------------ the fused step
def seg_hyper(h, sg, groups):
    """the step's arguments as segment sg takes them: (lr_i, wd_i) folded as the host folds them (groups_ref.f32_mul)"""
    if not groups:
        return dict(h)
    return dict(h, lr=f32_mul(h["lr"], sg.mult[0]), weight_decay=f32_mul(h["weight_decay"], sg.mult[1]))


@functools.lru_cache(maxsize=None)
def state(name):
    """(p0, m0, v0) per segment: p hashed in [-0.2, 0.2); m and v from groups_ref.seeded_state on the own gradients (v > 0)"""
    from .groups_ref import seeded_state
    c = case(name)
    G = {i: torch.from_numpy(sg.own) for i, sg in enumerate(c.segs)}
    M, V = seeded_state(G)
    P = [torch.from_numpy(synth.hash_uniform(c.segs[i].tid + 500, (c.segs[i].n,), 0.2)) for i in G]
    assert all(bool((V[i] > 0).all()) for i in G)
    return P, [M[i] for i in G], [V[i] for i in G]


def transposed_expect(c, p_flat):
    """the whole transposed buffer (bf16, NaN outside the segments' own columns) that belongs to the weights p_flat"""
    out = torch.full((c.tr_total,), float("nan"), dtype=torch.bfloat16)
    for sg in c.segs:
        if sg.tr:
            at, tN, tK = sg.tr
            rows = sg.n // tK
            w = p_flat[sg.off:sg.off + sg.n].reshape(rows, tK).to(torch.bfloat16)
            idx = at + torch.arange(tK)[:, None] * tN + torch.arange(rows)[None, :]
            out[idx] = w.t()
    return out


# ------------------------------------------------------------------------------------------------ the checks
def nan_fill(n, dtype=torch.float32):
    return torch.full((n,), float("nan"), dtype=dtype)


def check_gaps(c, what, buf):
    keep = ~c.mask()
    assert torch.equal(bits(buf[keep]), bits(nan_fill(int(keep.sum()), buf.dtype))), "%s: %s was written between two segments" % (c.name, what)


def check_plain(c, dst):
    """dst: the whole flat buffer after a plain launch.  -> segment label -> error / fp64 bound, for judge."""
    assert dst.numel() == c.total
    check_gaps(c, "dst", dst)
    worst = {}
    for sg in c.segs:
        got = dst[sg.off:sg.off + sg.n]
        assert torch.equal(bits(got), bits(torch.from_numpy(sg.own))), "%s %s: not the sum in the documented order" % (c.name, sg.label)
        worst[sg.label] = ratio(got, torch.from_numpy(sum64(sg.slabs, sg.nslabs, sg.n)), torch.from_numpy(sum_bound(sg.slabs, sg.nslabs, sg.n)))
    return worst


def check_fused(c, kind, h, groups, out, flat, grads):
    """out: whole buffers after a fused launch -- dst, p, m, v (Lion: the NaN buffer that lies where v would), shadow and shT where the
    launch has them.  flat: p, m, v, shadow as the flat entries leave them from the own gradient, in the same layout.  grads: the own
    gradient per segment.  The checks (a) .. (e) of the fused launch; -> key -> error / bound of check (b), for judge."""
    P0, M0, V0 = state(c.name)
    assert torch.equal(bits(out["dst"]), bits(nan_fill(c.total))), "%s: a fused launch stored into the gradient buffer" % c.name
    for k in ("p", "m", "v", "shadow"):
        if k in out:
            check_gaps(c, k, out[k])
    if kind == "lion":                                                                              # (e)
        assert torch.equal(bits(out["v"]), bits(nan_fill(c.total))), "%s: Lion touched v" % c.name
    for k in ("p", "m", "v", "shadow"):                                                             # (a)
        if k in out and not (k == "v" and kind == "lion"):
            for sg in c.segs:
                a, b = out[k][sg.off:sg.off + sg.n], flat[k][sg.off:sg.off + sg.n]
                assert torch.equal(bits(a), bits(b)), "%s %s: %s differs from the flat entry's on the own gradient" % (c.name, sg.label, k)
    worst = {}
    if kind == "adamw":                                                                             # (b)
        for i, sg in enumerate(c.segs):
            ref = linear_ref.adamw(P0[i], grads[i], M0[i], V0[i], **seg_hyper(h, sg, groups))
            for k, r in zip("pmv", ref):
                worst[k] = max(worst.get(k, 0.0), ratio(out[k][sg.off:sg.off + sg.n], r, 3e-6 * max(1.0, float(r.abs().max()))))
    for i, sg in enumerate(c.segs):
        assert not torch.equal(out["p"][sg.off:sg.off + sg.n], P0[i]) and not torch.equal(out["m"][sg.off:sg.off + sg.n], M0[i])
    if "shadow" in out:                                                                             # (c)
        keep = c.mask()
        assert torch.equal(bits(out["shadow"][keep]), bits(out["p"][keep].to(torch.bfloat16))), "%s: the shadow is not bf16(p)" % c.name
    if c.tr_total:                                                                                  # (d)
        assert torch.equal(bits(out["shT"]), bits(transposed_expect(c, out["p"]))), "%s: a transposed copy is not bf16(p)^T at pitch tN" % c.name
    return worst


# ------------------------------------------------------------------------------------------------ a launch on the host
FAULTS = ("skip", "swap", "quarter", "gap", "pitch", "hyper", "lion_v")


def _faulty_groups(nslabs, fault):
    g = slab_groups(nslabs)
    if fault == "skip":
        g[-1] = g[-1][:-2] + g[-1][-1:]                      # the last but one slab is not added
    elif fault == "swap":
        g[0][1], g[0][2] = g[0][2], g[0][1]
    elif fault == "quarter" and len(g) == 4:
        g[1], g[2] = g[1] + g[2][:1], g[2][1:]               # the boundary between the second and the third quarter, one slab late
    return g


def _step32(kind, p, g, m, v, a):
    """the update in plain float32 (the kernels spell out fused multiply-adds: last-bit differences, far inside check (b)'s bound)"""
    f = np.float32
    lr, b1, b2, eps, wd = (torch.tensor(f(a[k])) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
    decay = 1 - lr * wd
    if kind == "lion":
        cc = m + (g - m) * (1 - b1)
        return p * decay - lr * torch.sign(cc), m + (g - m) * (1 - b2), v
    t = a["t"]
    step = torch.tensor(f(float(lr) / f(1.0 - float(b1) ** t)))
    r = torch.tensor(f(1.0 / np.sqrt(f(1.0 - float(b2) ** t))))
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    return p * decay - step * (m / (v.sqrt() * r + eps)), m, v


def emulate(c, kind=None, h=None, groups=False, shadow=True, fault=None, seg=0):
    """What one launch leaves behind, computed on the host: kind None = the plain launch -> {dst}; else the fused one -> dst, p, m, v,
    shadow, shT as check_fused takes them.  fault: one of FAULTS, planted into segment `seg` (or behind it: "gap")."""
    grads = []
    for i, sg in enumerate(c.segs):
        grp = _faulty_groups(sg.nslabs, fault) if i == seg and fault in ("skip", "swap", "quarter") else slab_groups(sg.nslabs)
        grads.append(torch.from_numpy(sum_groups(sg.slabs, grp, sg.n)))
    sg = c.segs[seg]
    if kind is None:
        dst = c.scatter(grads)
        if fault == "gap":
            dst[sg.off + sg.n + 1] = 1.0
        return {"dst": dst}
    P0, M0, V0 = state(c.name)
    new = []
    for i, s in enumerate(c.segs):
        hs = c.segs[(i + 1) % len(c.segs)] if fault == "hyper" and i == seg else s
        new.append(_step32(kind, P0[i], grads[i], M0[i], V0[i], seg_hyper(h, hs, groups)))
    out = {"dst": nan_fill(c.total), "p": c.scatter([n[0] for n in new]), "m": c.scatter([n[1] for n in new])}
    out["v"] = nan_fill(c.total) if kind == "lion" else c.scatter([n[2] for n in new])
    if shadow:
        out["shadow"] = c.scatter([n[0] for n in new], dtype=torch.bfloat16)
    if c.tr_total:
        out["shT"] = transposed_expect(c, out["p"])
        if fault == "pitch":                                 # the segment's block at pitch tK (what would land behind the buffer is dropped)
            at, tN, tK = sg.tr
            rows = sg.n // tK
            k, r = torch.arange(tK)[:, None], torch.arange(rows)[None, :]
            out["shT"][at + k * tN + r] = float("nan")
            idx, w = at + k * tK + r, out["p"][sg.off:sg.off + sg.n].reshape(rows, tK).to(torch.bfloat16).t()
            out["shT"][idx[idx < c.tr_total]] = w[idx < c.tr_total]
    if fault == "gap":
        out["p"][sg.off + sg.n + 1] = 1.0
    if fault == "lion_v":
        out["v"][sg.off + 2] = 0.0
    return out
