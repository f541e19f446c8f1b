"""CPU: the checker of the slab reductions (tests/reduce_ref.py) is held true before tests/test_gpu_reduce_ops.py relies on it -- the
documented order against an independent replay, the fp64 bound on the reference itself, the condition on the inputs (the order shows in
the bits), every check clean on the host emulation of a launch and failing with one planted fault -- and afr_op_reduce_group_step's
refusals, with fake pointers and without a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import reduce_ref as R
from .test_gpu_linear_ops import ADAMW, LION

HYPER = {"adamw": ADAMW, "lion": LION}
SMALL_PLAIN = [n for n in R.PLAIN_CASES if not n.startswith("cap-")]


def test_ordered_sum_is_the_documented_order_replayed():
    """an independent statement of both orders, in torch float32, on ragged slab counts around the threshold and the quarter splits"""
    for nslabs in (1, 2, 7, 31, 32, 33, 35, 37, 40):
        sg = R.Seg(nslabs, 260)
        sg.tid = 6900 + nslabs
        v = torch.from_numpy(sg.slabs)[:, :260]

        def chain(lo, hi):
            a = torch.zeros(260)
            for s in range(lo, hi):
                a = a + v[s]
            return a
        if nslabs < 32:
            want = chain(0, nslabs)
        else:
            per = (nslabs + 3) // 4
            q = [chain(g * per, min(nslabs, (g + 1) * per)) for g in range(4)]
            want = ((q[0] + q[1]) + q[2]) + q[3]
        assert np.array_equal(R.ordered_sum(sg.slabs, nslabs, 260).view(np.int32), want.numpy().view(np.int32))
        assert sum(len(g) for g in R.slab_groups(nslabs)) == nslabs and np.isnan(sg.slabs[:, 260:]).all() and sg.stride % 4 == 0 and sg.stride > 260


@pytest.mark.parametrize("name", R.PLAIN_CASES + list(R.FUSED_SETS))
def test_the_order_shows_in_the_bits_and_the_reference_is_inside_its_bound(name):
    """The condition on the inputs: in every segment with three slabs or more (one or two slabs have one order only: a float32 addition
    commutes) the reversed order differs in bits in at least half of the columns, and so does the shallow order in a deep segment.
    Columns are counted over the case's segments of that kind together: a segment of 4 elements has too few to count alone."""
    c = R.case(name)
    rev, shal = [], []
    for sg in c.segs:
        assert R.ratio(torch.from_numpy(sg.own), torch.from_numpy(R.sum64(sg.slabs, sg.nslabs, sg.n)), torch.from_numpy(R.sum_bound(sg.slabs, sg.nslabs, sg.n))) <= 1.0
        if sg.nslabs >= 3:
            rev.append(sg.own.view(np.int32) != R.ordered_sum(sg.slabs[::-1], sg.nslabs, sg.n).view(np.int32))
        if sg.nslabs >= R.DEEP:
            shal.append(sg.own.view(np.int32) != R.sum_groups(sg.slabs, R.slab_groups(sg.nslabs, deep=False), sg.n).view(np.int32))
    for what, d in (("reversed", rev), ("shallow", shal)):
        if d:
            share = float(np.concatenate(d).mean())
            print("%s: %s order differs in %.2f of the columns" % (name, what, share))
            assert share >= 0.5, (name, what, share)
    assert bool(shal) == any(sg.nslabs >= R.DEEP for sg in c.segs)


def test_layout_is_out_of_order_with_gaps_and_inside_the_entry_s_rules():
    for name in R.PLAIN_CASES + list(R.FUSED_SETS):
        c = R.case(name)
        spans = sorted((sg.off, sg.off + sg.n) for sg in c.segs)
        assert spans[0][0] >= R.GAP and c.total - spans[-1][1] >= R.GAP
        assert all(b[0] - a[1] >= R.GAP for a, b in zip(spans, spans[1:]))
        assert all(sg.off % 4 == 0 and sg.n % 4 == 0 and sg.stride % 4 == 0 and sg.stride > sg.n for sg in c.segs)
        if len(c.segs) > 2:
            assert [sg.off for sg in c.segs] != sorted(sg.off for sg in c.segs)
        for sg in c.segs:
            if sg.tr:
                at, tN, tK = sg.tr
                assert tK % 4 == 0 and sg.n % tK == 0 and tN >= sg.n // tK and at + (tK - 1) * tN + sg.n // tK <= c.tr_total - 64 and at >= 64
    caps = R.case("cap-shallow").segs[0], R.case("cap-deep").segs[0]
    assert caps[0].n // 4 > 1024 * 256 and caps[1].n // 4 > 1024 * 64 and caps[0].n // 4 < 2 * 1024 * 256 and caps[1].n // 4 < 2 * 1024 * 64
    assert sum(1 for sg in R.case("mixed32").segs if sg.nslabs >= R.DEEP) >= 8 and len(R.case("mixed32").segs) == 32
    g = R.case("glyph")
    assert any(sg.tr and sg.nslabs >= R.DEEP for sg in g.segs) and any(sg.tr and sg.nslabs < R.DEEP for sg in g.segs)
    assert any(sg.tr and sg.tr[1] > sg.n // sg.tr[2] for sg in g.segs) and any(not sg.tr for sg in g.segs)


@pytest.mark.parametrize("name", SMALL_PLAIN)
def test_plain_checks_are_clean_on_the_reference_and_see_each_planted_fault(name):
    c = R.case(name)
    worst = R.check_plain(c, R.emulate(c)["dst"])
    assert max(worst.values()) <= 1.0
    for seg, sg in enumerate(c.segs):
        for fault in ("skip", "swap", "quarter", "gap"):
            if (fault == "skip" and sg.nslabs < 2) or (fault == "swap" and sg.nslabs < 3) or (fault == "quarter" and sg.nslabs < R.DEEP):
                continue
            if fault in ("swap", "quarter") and sg.n < 64:
                continue                                                   # (4 columns may all round alike; the wider segments carry this fault)
            with pytest.raises(AssertionError, match="written between" if fault == "gap" else "documented order"):
                R.check_plain(c, R.emulate(c, fault=fault, seg=seg)["dst"])


def test_a_skipped_slab_also_breaks_the_fp64_bound():
    c = R.case("deep-260")
    for seg, sg in enumerate(c.segs):
        got = R.emulate(c, fault="skip", seg=seg)["dst"][sg.off:sg.off + sg.n]
        assert R.ratio(got, torch.from_numpy(R.sum64(sg.slabs, sg.nslabs, sg.n)), torch.from_numpy(R.sum_bound(sg.slabs, sg.nslabs, sg.n))) > 1.0


def test_reduce_slabs_ref_forms():
    sg = R.Seg(7, 1003)
    sg.tid = 6990
    old = R.synth.hash_uniform(6991, (1003,), 3.0)
    for scale in (1.0, 0.5):
        assert len(R.reduce_slabs_ref(sg.slabs, 7, 1003, scale, old)) == 1
        assert np.array_equal(R.reduce_slabs_ref(sg.slabs, 7, 1003, scale)[0], sg.own * np.float32(scale))
    two = R.reduce_slabs_ref(sg.slabs, 7, 1003, 0.3, old)
    assert len(two) == 2 and 0.0 < R.differing_share(*two) < 0.5                # the two forms are told apart, and neither is far from the other
    assert np.abs(two[0].astype(np.float64) - two[1]).max() <= 2.0 ** -23 * np.abs(two[1]).max()


@pytest.mark.parametrize("kind", ["adamw", "lion"])
@pytest.mark.parametrize("groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("name", R.FUSED_SETS)
def test_fused_checks_are_clean_on_the_reference_and_see_each_planted_fault(name, kind, groups):
    c, h = R.case(name), HYPER[kind]
    grads = [torch.from_numpy(sg.own) for sg in c.segs]
    flat = R.emulate(c, kind, h, groups)
    worst = R.check_fused(c, kind, h, groups, R.emulate(c, kind, h, groups), flat, grads)
    assert (kind == "lion" and not worst) or max(worst.values()) <= 1.0

    def broken(fault, seg, match):
        with pytest.raises(AssertionError, match=match):
            R.check_fused(c, kind, h, groups, R.emulate(c, kind, h, groups, fault=fault, seg=seg), flat, grads)
    for seg, sg in enumerate(c.segs):
        broken("skip", seg, "flat entry")
        broken("swap", seg, "flat entry")
        if sg.nslabs >= R.DEEP:
            broken("quarter", seg, "flat entry")
        broken("gap", seg, "p was written between")
        if sg.tr:
            broken("pitch", seg, "transposed copy")
        if groups and sg.mult != c.segs[(seg + 1) % len(c.segs)].mult:
            broken("hyper", seg, "flat entry")
        if kind == "lion":
            broken("lion_v", seg, "Lion touched v")
    assert not groups or any(a.mult != b.mult for a, b in zip(c.segs, c.segs[1:]))


@pytest.mark.parametrize("fault", ["skip", "hyper"])
def test_check_b_alone_sees_a_wrong_gradient_and_a_wrong_hyper(fault):
    """with the flat entries' side given the SAME fault, only the comparison with fp64 is left to object"""
    c, h = R.case("modes"), ADAMW
    grads = [torch.from_numpy(sg.own) for sg in c.segs]
    bad = R.emulate(c, "adamw", h, True, fault=fault, seg=0)
    with pytest.raises(AssertionError):
        from .op_harness import judge
        judge("b", R.check_fused(c, "adamw", h, True, bad, bad, grads))


def test_refusals_come_with_a_message_and_without_a_launch():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI = _lib.AFR_EINVAL
    fk = 0x10000

    def call(nseg=2, dst=(fk + 1024, fk + 4096), slabs=(fk, fk), nslabs=(3, 40), stride=(72, 260), n=(64, 256), step=None, arrays=True, name_cap=32, **st):
        k = max(nseg, 1) if arrays else 0
        pad = lambda v: tuple(v) + (v[-1],) * (k - len(v))
        arr = lambda T, v: (T * k)(*pad(v)[:k]) if arrays else None
        s = None
        if step or st:
            f = dict(opt_kind=0, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.1, t=3, gbase=fk, p=fk, m=fk, v=fk)
            f.update(st)
            s = _lib.AfrReduceStep()
            keep = []
            for key, val in f.items():
                if key in ("lr_mult", "wd_mult"):
                    val = (C.c_float * k)(*pad(val)[:k])
                elif key in ("tN", "tK"):
                    val = (C.c_int32 * k)(*pad(val)[:k])
                elif key == "shT":
                    val = (C.c_void_p * k)(*pad(val)[:k])
                keep.append(val)
                setattr(s, key, val)
        name = C.create_string_buffer(32)
        return lib.afr_op_reduce_group_step(nseg, arr(C.c_void_p, dst), arr(C.c_void_p, slabs), arr(C.c_int, nslabs), arr(C.c_int64, stride),
                                            arr(C.c_int64, n), C.byref(s) if s is not None else None, name, name_cap, None)

    def refused(word, **kw):
        assert call(**kw) == EI, kw
        assert word.encode() in lib.afr_last_error(), (kw, lib.afr_last_error())
    refused("null segment array", arrays=False)
    refused("null pointer", dst=(fk, None))
    refused("null pointer", slabs=(None, fk))
    refused("1 to at most 32", nseg=0)
    refused("1 to at most 32", nseg=-1)
    refused("1 to at most 32", nseg=33)
    refused("negative or not a multiple of 4", n=(64, -4))
    refused("negative or not a multiple of 4", n=(62, 256))
    refused("nslabs = 0", nslabs=(0, 40))
    refused("stride 262", stride=(72, 262))
    refused("name_cap", name_cap=0)
    refused("dst - gbase", step=True, dst=(fk + 1024, fk - 16))
    refused("dst - gbase", step=True, dst=(fk + 1024 + 8, fk + 4096))
    refused("t starts at 1", step=True, t=0)
    refused("optimizer kind", step=True, opt_kind=2)
    refused("null gbase or moment", step=True, m=None)
    refused("null gbase or moment", step=True, v=None)
    refused("null gbase or moment", step=True, gbase=None)
    refused("multipliers", step=True, lr_mult=(1.0, -1.0))
    refused("multipliers", step=True, wd_mult=(float("nan"), 1.0))
    refused("tK = 6", step=True, shT=(fk, None), tN=(16, 0), tK=(6, 0))
    refused("no multiple of tK", step=True, shT=(fk, None), tN=(16, 0), tK=(12, 0))
    refused("smaller than its 8 rows", step=True, shT=(fk, None), tN=(7, 0), tK=(8, 0))
    refused("shT without tN and tK", step=True, shT=(fk, None))
    refused("shT without a fused step", p=None, shT=(None, fk), tN=(0, 4), tK=(0, 64))
    # afr_op_reduce_group is the same entry: the same refusals, and no segments at all is still nothing to do
    k = 2
    a = lambda T, v: (T * k)(*v)
    assert lib.afr_op_reduce_group(k, a(C.c_void_p, (fk, fk)), a(C.c_void_p, (fk, fk)), a(C.c_int, (3, 3)), a(C.c_int64, (66, 64)), a(C.c_int64, (64, 64)), None) == EI
    assert b"stride 66" in lib.afr_last_error()
    assert lib.afr_op_reduce_group(0, None, None, None, None, None, None) == 0
