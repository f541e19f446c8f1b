"""GPU: the sheet front end's two fused kernels (csrc/sheet.hip), ONE launch each through afr_op_sheet_fwd / afr_op_sheet_bwd, every
output element against the fp64 restatement of tests/sheet_ref.py under its derived bound: z and, from the save area, o, the row
maxima and 1/sum; the ten gradients as the fp64 sum of the per-block slabs.  The shapes are the smallest at which each mechanism
can fail: the L sweep (B = 3, max_length 120) walks the edges of the key pairs (L = 1: a lane without a key), of the guarded K tail
(L % 4), of the clamped edge tiles (L % 16), of the keep-bit words (64) and LMAX; the trip cases (max_length 24) drive the
persistent loop through one, exactly one, and up to three strings per block (600 = 2.34 trips); every batch mixes dataset strings,
one-code strings (an occurrence chain of length L), a code at distances 7, 8, 9, 17, all-distinct codes, codes 0 and vocab - 1,
and a rare code in strings 10, 266 and 522.  Besides the error, each case checks: buffers pre-filled with NaN hold none afterwards
(tests/op_harness.py checks z and the slabs of every launch, the case the float part of the save area) and their guard bands of 256
bytes on both sides keep their bits; z beyond L*64 is +0; in training the saved keep bits are the packed synth
masks; the kernel's ReLU gate (z > 0 where fc dropout kept the element) differs from fp64's only where |pre| is below its bound;
a second launch repeats the first bit for bit; the backward without a save area (the recompute path) gives the same slabs bit for
bit; every slab is finite, and the space between tensors, rows of dP at or beyond L and embedding rows of codes its block never
met are exactly zero in it.

Every case prints its largest error as a fraction of the bound (pytest -s).  Measured on MI355X, the largest per output over all
cases:
    forward    z 0.137 (float32) / 0.994 (bf16: the rounding to bf16 is the 2^-8 |ref| term of the bound itself), o 0.125,
               row maxima 0.082, 1/sum 0.208
    backward   the slabs summed in fp64: pos 0.063, emb 0.067, w_in 0.201, b_in 0.209, w_o 0.067, b_o 0.043, ln_g 0.043, ln_b 0.034,
               w1 0.127, b1 0.110;  summed in float32 (afr_op_reduce / the grouped reduce, bound with the slab-sum term): at most
               0.211 (w1)
    ReLU gates none of the 15.3 million gates of the cases differs from fp64's"""
import ctypes as C
import functools

import pytest
import torch

from ai_font_renderer_amd import _lib
from . import sheet_ref as R
from .gpu_util import dev, ptr, stream
from .op_harness import Outs, bits, dt, judge, tt, twice

pytestmark = pytest.mark.gpu
F64 = torch.float64


class Dev:
    """a case's inputs on the device"""

    def __init__(self, c, x=None):
        self.c = c
        self.P = {n: dev(t) for n, t in c["P"].items()}
        self.prm = _lib.AfrSheetParams(*[self.P[n].data_ptr() for n in R.NAMES])
        self.x = dev(c["x"] if x is None else x)
        self.dz = dev(c["dz"], tt(c["is_bf16"]))
        d = c["drop"]
        self.drop = None if d is None else _lib.AfrSheetDropout(d["seed"], d["step"], d["rank"], *d["p"])
        self.off, self.sizes, self.total = R.slab_layout(c["max_length"], c["vocab"])
        self.lay = _lib.AfrSheetSlabLayout(*[self.off[n] for n in R.NAMES], self.total)

    def _drop(self, drop):
        drop = self.drop if drop is None else drop
        return None if drop is None else C.byref(drop)

    def fwd(self, save=True, drop=None):
        c = self.c
        B, L = c["B"], c["L"]
        o = Outs()
        pz = o.new("z", (B, c["max_length"] * R.F), tt(c["is_bf16"]))
        ps = o.new("save", (B, L * R.SAVE_PER_POS), torch.float32) if save else C.c_void_p(0)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().afr_op_sheet_fwd(dt(c["is_bf16"]), C.byref(self.prm), ptr(self.x), c["ldx"], B, L, c["max_length"], c["vocab"],
                                               R.EPS, self._drop(drop), pz, ps, ptr(err), stream()))
        # save may keep its fill: its keep words are bit patterns (a word of ones is a NaN) and are not written at all outside training;
        # the float part of every row is checked for NaN by the case
        return dict(o.finish(may_keep_fill=("save",)), err=int(err.cpu()))

    def bwd(self, save):
        c = self.c
        nb = R.blocks(c["B"])
        o = Outs()
        psl = o.new("slabs", (nb, self.total), torch.float32)
        sv = None if save is None else save.cuda().contiguous()
        _lib.check(_lib.lib().afr_op_sheet_bwd(dt(c["is_bf16"]), C.byref(self.prm), ptr(self.x), c["ldx"], c["B"], c["L"], c["max_length"],
                                               c["vocab"], R.EPS, self._drop(None), ptr(self.dz), ptr(sv), psl, C.byref(self.lay), stream()))
        return o.finish()["slabs"]


def split_save(save, L, training):
    """the save area [B][L*56] -> o [B][L][32], smax, sinv [B][4][L], bits [B][4][L][4] (training; the words are not written otherwise)"""
    B = save.shape[0]
    o = save[:, :L * R.E].reshape(B, L, R.E)
    smax = save[:, L * 32:L * 36].reshape(B, R.H, L)
    sinv = save[:, L * 36:L * 40].reshape(B, R.H, L)
    keep = (bits(save[:, L * 40:]).to(torch.int64) & 0xFFFFFFFF).reshape(B, R.H, L, 4) if training else None
    return dict(o=o, smax=smax, sinv=sinv, bits=keep)


def grads_of(slabs, d, dtype=F64):
    """the ten gradients: the slabs summed over blocks in `dtype` on the host"""
    tot = slabs.to(dtype).sum(0)
    shp = dict(pos=(-1, R.E), emb=(-1, R.E), w_in=(R.QKV, R.E), w_o=(R.E, R.E), w1=(R.F, R.E))
    return {n: tot[d.off[n]:d.off[n] + d.sizes[n]].reshape(shp.get(n, (-1,))) for n in R.NAMES}


def check_slab_zeros(slabs, d, c, tok):
    """what a block does not own in its slab is exactly zero: the space between tensors, rows of dP at or beyond L, the embedding rows
    of codes none of its strings holds"""
    assert bool(torch.isfinite(slabs).all()), "a slab holds a NaN or an infinity"
    nb, L = slabs.shape[0], c["L"]
    owned = torch.zeros(d.total, dtype=torch.bool)
    for n in R.NAMES:
        owned[d.off[n]:d.off[n] + d.sizes[n]] = True
    assert not bool(slabs[:, ~owned].any()), "the space between two tensors of a slab is not zero"
    assert not bool(slabs[:, d.off["pos"] + L * R.E:d.off["pos"] + d.sizes["pos"]].any()), "a row of dP at or beyond L is not zero"
    met = torch.zeros(nb, c["vocab"], dtype=torch.bool)
    met[(torch.arange(c["B"]) % nb).unsqueeze(1).expand(-1, L).reshape(-1), tok.reshape(-1)] = True
    emb = slabs[:, d.off["emb"]:d.off["emb"] + d.sizes["emb"]].reshape(nb, c["vocab"], R.E)
    assert not bool(emb[~met].any()), "an embedding row of a code the block never met is not zero"


@functools.lru_cache(maxsize=2)
def _reference(B, L, ML, mode, kind, ldx):
    """the fp64 forward of a case and its bounds: one per (shape, mode, parameter set), shared by the f32 and the bf16 launch"""
    c = R.make_case(B, L, ML, mode, kind=kind, ldx=ldx)
    P64 = {n: t.double() for n, t in c["P"].items()}
    masks, scales = R.masks_for(B, L, c["drop"]), R.scales_for(c["drop"])
    fw = R.front_fwd(P64, c["x"], L, ML, masks, scales)
    return P64, masks, scales, fw, R.fwd_bounds(P64, fw, False), R.fwd_bounds(P64, fw, True)["z"]


def _run_case(B, L, ML, mode, is_bf16, kind="generic", ldx=None):
    ldx = L if ldx is None else ldx
    name = f"{B}x{L} ldx {ldx} {mode} {kind} {'bf16' if is_bf16 else 'f32'}"
    c = R.make_case(B, L, ML, mode, is_bf16, kind, ldx)
    P64, masks, scales, fw, fb, zb16 = _reference(B, L, ML, mode, kind, ldx)
    training = c["drop"] is not None
    d = Dev(c)
    # ---- forward
    f1 = twice(d.fwd)
    assert f1["err"] == 0
    z = f1["z"]                                                   # (no NaN left in it: Outs.finish)
    assert not bool(bits(z[:, L * R.F:]).any()), "z beyond L*64 is not +0"
    sv = split_save(f1["save"], L, training)
    assert not bool(torch.isnan(f1["save"][:, :L * 40]).any()), "save: NaN left in an element the kernel owns"     # (the keep words are compared below)
    got = dict(z=z.float(), o=sv["o"], smax=sv["smax"], sinv=sv["sinv"])
    bnd = dict(fb, z=zb16 if is_bf16 else fb["z"])
    judge(name, got, fw, bnd, ("z", "o", "smax", "sinv"))
    if training:
        assert torch.equal(sv["bits"], fw["bits"]), "the saved keep bits are not the packed synth masks"
    assert torch.equal(bits(d.fwd(save=False)["z"]), bits(z)), "z depends on whether a save area is given"
    # ---- the kernel's ReLU gate: z > 0 where fc dropout kept the element (elsewhere df is zero whatever the gate)
    cache = fw["cache"]
    kept = (masks["fc"] != 0) if training else torch.ones_like(cache["gate"])
    gate = torch.where(kept, z[:, :L * R.F].float().reshape(B, L, R.F) > 0, cache["gate"])
    flipped = gate != cache["gate"]
    assert not bool((flipped & (cache["pre"].abs() >= fb["pre"])).any()), "a ReLU gate differs from fp64's where |pre| is not below its bound"
    print(f"    gates that differ from fp64's: {int(flipped.sum())} of {gate.numel()}")
    # ---- backward: with the save area, again, and without it (the recompute path)
    s1 = twice(lambda: d.bwd(f1["save"]))
    assert torch.equal(bits(s1), bits(d.bwd(None))), "slabs: the recompute path (save = NULL) differs from the saved one"
    check_slab_zeros(s1, d, c, cache["tok"])
    fwg = fw if not bool(flipped.any()) else R.front_fwd(P64, c["x"], L, ML, masks, scales, relu_gate=gate)
    bw = R.front_bwd(P64, fwg, c["dz"].double())
    gb = R.bwd_bounds(P64, fwg, fb, bw)
    judge(name, grads_of(s1, d), bw["G"], gb, R.NAMES)
    return d, c, s1, fwg, fb, bw


def _params(cases, modes=R.MODES):
    return [pytest.param(B, L, m, bf, id=f"{B}x{L}-{m}-{'bf16' if bf else 'f32'}") for B, L in cases for m in modes for bf in (False, True)]


@pytest.mark.parametrize("B,L,mode,is_bf16", _params([(3, L) for L in R.L_SWEEP]))
def test_length_sweep(B, L, mode, is_bf16):
    _run_case(B, L, 120, mode, is_bf16)


@pytest.mark.parametrize("B,L,mode,is_bf16", _params(R.TRIPS))
def test_trips(B, L, mode, is_bf16):
    _run_case(B, L, 24, mode, is_bf16)


@pytest.mark.parametrize("kind", R.SPECIAL)
@pytest.mark.parametrize("B,L,mode,is_bf16", _params([(5, 65)], ("eval", "train")))
def test_special_parameter_sets(B, L, mode, is_bf16, kind):
    _run_case(B, L, 120, mode, is_bf16, kind)


@pytest.mark.parametrize("is_bf16", [False, True], ids=["f32", "bf16"])
def test_over_long_input_rows_are_truncated(is_bf16):
    """ldx = L + 7: a row of x is longer than the L codes that are read; the result is that of the truncated rows"""
    d, c, s1, *_ = _run_case(5, 17, 24, "train", is_bf16, ldx=24)
    c2 = dict(c, x=c["x"][:, :17].contiguous(), ldx=17)
    d2 = Dev(c2)
    f, f2 = d.fwd(), d2.fwd()
    assert torch.equal(bits(f["z"]), bits(f2["z"])) and torch.equal(bits(f["save"]), bits(f2["save"]))
    assert torch.equal(bits(s1), bits(d2.bwd(f2["save"])))


@pytest.mark.parametrize("is_bf16", [False, True], ids=["f32", "bf16"])
def test_slab_totals_in_float32_orders(is_bf16):
    """The slabs summed in float32 as the library does it: afr_op_reduce adds them in slab order, the grouped reduce (the plan's: 32
    slabs or more are summed in four quarters that meet in order) -- each equals that order replayed on the host bit for bit, and
    both stay inside the bound that counts the float32 slab sum."""
    lib = _lib.lib()
    d, c, s1, fwg, fb, bw = _run_case(300, 24, 24, "train", is_bf16)
    nb, n = s1.shape
    sl = s1.cuda()
    seq = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.afr_op_reduce(ptr(seq), ptr(sl), nb, n, n, 1.0, 0, stream()))
    grp = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.afr_op_reduce_group(1, (C.c_void_p * 1)(grp.data_ptr()), (C.c_void_p * 1)(sl.data_ptr()), (C.c_int * 1)(nb),
                                       (C.c_int64 * 1)(n), (C.c_int64 * 1)(n), stream()))
    torch.cuda.synchronize()

    def chain(lo, hi):
        a = torch.zeros(n, dtype=torch.float32)
        for s in range(lo, hi):
            a = a + s1[s]
        return a
    per = (nb + 3) // 4
    q = [chain(g * per, min(nb, (g + 1) * per)) for g in range(4)]
    assert torch.equal(bits(seq.cpu()), bits(chain(0, nb))), "afr_op_reduce is not the sum in slab order"
    assert torch.equal(bits(grp.cpu()), bits(((q[0] + q[1]) + q[2]) + q[3])), "the grouped reduce is not the plan's order"
    P64 = {k: t.double() for k, t in c["P"].items()}
    gb = R.bwd_bounds(P64, fwg, fb, bw, reduced=True)
    for nm, tot in (("afr_op_reduce", seq), ("grouped reduce", grp)):
        judge(nm, grads_of(tot.cpu().unsqueeze(0), d), bw["G"], gb, R.NAMES)


@pytest.mark.parametrize("is_bf16", [False, True], ids=["f32", "bf16"])
def test_no_dropout_is_independent_of_seed_and_step(is_bf16):
    """An eval forward takes no dropout description at all; what can still leak a seed or a step is a training launch whose rates
    are 0.  Its z and save rows are bitwise those of the eval forward whatever the seed and the step, and every keep bit is set."""
    c = R.make_case(5, 65, 120, "eval", is_bf16)
    d = Dev(c)
    ev = d.fwd()
    L = c["L"]
    for seed, step in ((42, 3), (7, 0), (2 ** 40 + 1, 2 ** 33)):
        tr = d.fwd(drop=_lib.AfrSheetDropout(seed, step, 0, 0.0, 0.0, 0.0))
        assert torch.equal(bits(tr["z"]), bits(ev["z"]))
        assert torch.equal(bits(tr["save"][:, :L * 40]), bits(ev["save"][:, :L * 40]))
        want = R.pack_bits(torch.ones(5, R.H, L, L, dtype=torch.uint8))
        assert torch.equal(split_save(tr["save"], L, True)["bits"], want)


@pytest.mark.parametrize("is_bf16", [False, True], ids=["f32", "bf16"])
def test_row_locality(is_bf16):
    """a string's z and save rows in eval are bitwise the same at batch index 0 of B = 1 and at index 299 of B = 300 (a second trip)"""
    c = R.make_case(300, 24, 24, "eval", is_bf16)
    big = Dev(c).fwd()
    one = Dev(dict(c, B=1, x=c["x"][299:300].contiguous(), dz=c["dz"][299:300].contiguous())).fwd()
    assert torch.equal(bits(big["z"][299]), bits(one["z"][0]))
    assert torch.equal(bits(big["save"][299, :24 * 40]), bits(one["save"][0, :24 * 40]))


@pytest.mark.parametrize("is_bf16", [False, True], ids=["f32", "bf16"])
def test_out_of_range_codes_set_the_flag_and_are_clamped(is_bf16):
    c = R.make_case(5, 17, 24, "train", is_bf16)
    bad = c["x"].clone()
    bad[0, 3], bad[2, 0], bad[4, 16] = -5, c["vocab"], 2 ** 40
    clamped = bad.clamp(0, c["vocab"] - 1)
    db, dc = Dev(c, bad), Dev(c, clamped)
    fb_, fc_ = db.fwd(), dc.fwd()
    assert fb_["err"] & 1 and fc_["err"] == 0
    assert torch.equal(bits(fb_["z"]), bits(fc_["z"])) and torch.equal(bits(fb_["save"]), bits(fc_["save"]))
    for save in (fc_["save"], None):
        assert torch.equal(bits(db.bwd(save)), bits(dc.bwd(save)))
