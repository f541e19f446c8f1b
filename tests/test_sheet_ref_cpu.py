"""CPU: the checker of the sheet front end's two kernels (tests/sheet_ref.py) is itself checked, on the inputs
tests/test_gpu_sheet_ops.py feeds the kernels: (a) the fp64 restatements ARE the model (they reproduce oracle.sheet_forward /
sheet_backward driven with an identity fc_output, so that du is dz); (b) the float32 restatement stays within a quarter of every
bound; (c) every planted fault misses a bound at least tenfold; (d) the bounds are not hollow: on the generic parameters the
largest bound of every output is at most 2e-5 of the output's largest fp64 magnitude (the special parameter sets are exempt: their
planted LayerNorm rows and score gaps are where float32 itself loses digits, and the bounds say so); (e) at most 1e-4 of the ReLU
gates sit closer to zero than the bound of their pre-activation."""
import pytest
import torch

from . import sheet_ref as R
from .util import oracle

F64, F32 = torch.float64, torch.float32
FWD_KEYS = ("z", "o", "smax", "sinv")


# --------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("L", [7, 12])
def test_a_fp64_restatements_are_the_oracle(train, L):
    from ai_font_renderer_amd.config import SheetConfig
    ML, B = 12, 6
    cfg = SheetConfig(max_length=ML, sheet_h=1, sheet_w=ML * R.F)
    c = R.make_case(B, L, ML, "train" if train else "eval")
    P = {n: t.double() for n, t in c["P"].items()}
    Po = {R.STATE[n]: t for n, t in P.items()}
    Po["fc_output.weight"], Po["fc_output.bias"] = torch.eye(ML * R.F, dtype=F64), torch.zeros(ML * R.F, dtype=F64)
    masks = R.masks_for(B, L, c["drop"])
    scales = tuple(1.0 / (1.0 - p) for p in R.RATES) if train else None            # the oracle's scales, in double
    fw = R.front_fwd(P, c["x"], L, ML, masks, scales)
    bw = R.front_bwd(P, fw, c["dz"].double())
    _, cache = oracle.sheet_forward(Po, c["x"], cfg, masks)
    Go = oracle.sheet_backward(Po, cache, c["dz"].double(), cfg)
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)              # noqa: E731
    assert rel(fw["z"], cache["z"]) <= 1e-12 and rel(fw["o"], cache["o"]) <= 1e-12
    S = (cache["qh"] * R.SCALE) @ cache["kh"].transpose(-1, -2)
    assert rel(fw["smax"], S.amax(-1)) <= 1e-12
    assert rel(fw["sinv"], 1.0 / torch.exp(S - S.amax(-1, keepdim=True)).sum(-1)) <= 1e-12
    for n in R.NAMES:
        assert rel(bw["G"][n], Go[R.STATE[n]]) <= 1e-12, n
    if train:       # the packed keep bits, read back by the kernels' formula
        j = torch.arange(L)
        word, bit = (j & 1) * 2 + (j >> 6), (j >> 1) & 31
        assert torch.equal((fw["bits"][..., word] >> bit) & 1, masks["attn"].to(torch.int64))


# --------------------------------------------------------------------------------------------------- (b), (d), (e)
def _cases():
    out = []
    for L in (1, 2, 17, 65, 120):
        out += [pytest.param(3, L, 120, m, "generic", id=f"3x{L}-{m}") for m in (("train", "eval") if L in (17, 65) else ("train",))]
    for B, L in ((257, 17), (600, 24)):
        out.append(pytest.param(B, L, 24, "train", "generic", id=f"{B}x{L}-train"))
    out.append(pytest.param(8, 120, 120, "train0", "generic", id="8x120-train0"))
    out.append(pytest.param(5, 65, 120, "train", "generic", id="5x65-train"))
    for kind in R.SPECIAL:
        out += [pytest.param(5, 65, 120, m, kind, id=f"5x65-{m}-{kind}") for m in ("train", "eval")]
    return out


@pytest.mark.parametrize("B,L,ML,mode,kind", _cases())
def test_b_float32_stays_within_a_quarter_of_bounds_that_are_not_hollow(B, L, ML, mode, kind):
    c = R.make_case(B, L, ML, mode, kind=kind)
    fw, bw = R.run(c, F64)
    gate = fw["cache"]["gate"]
    fb, gb = R.bounds(c, fw, bw)
    f32, b32 = R.run(c, F32, relu_gate=gate)                     # the gate is an input of the comparison, as on the GPU
    worst = {k: R.ratio(f32[k], fw[k], fb[k]) for k in FWD_KEYS}
    worst.update({n: R.ratio(b32["G"][n], bw["G"][n], gb[n]) for n in R.NAMES})
    frac = {k: float(fb[k].max()) / max(float(fw[k].abs().max()), 1e-300) for k in FWD_KEYS}
    frac.update({n: float(gb[n].max()) / max(float(bw["G"][n].abs().max()), 1e-300) for n in R.NAMES})
    near = int((fw["cache"]["pre"].abs() < fb["pre"]).sum())
    print(f"{B}x{L} {mode} {kind}: float32 error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    print("    largest bound / largest magnitude " + ", ".join(f"{k} {v:.1e}" for k, v in frac.items()))
    print(f"    gates with |pre| below the bound: {near} of {gate.numel()}")
    for k, v in worst.items():
        assert v <= 0.25, (k, v)
    zb = R.fwd_bounds({n: t.double() for n, t in c["P"].items()}, fw, is_bf16=True)["z"]
    assert R.ratio(R.bf16(f32["z"]), fw["z"], zb) <= 1.0         # a bf16 z: one more rounding, inside the bf16 bound
    if kind == "generic":                                        # the special parameter sets are exempt (module docstring)
        for k, v in frac.items():
            assert v <= 2e-5, (k, v)
        assert near <= 1e-4 * gate.numel(), near


# --------------------------------------------------------------------------------------------------------- (c)
FAULT_CASE = dict(keepword=(3, 100, 120), dk_scale=(3, 17, 120), demb_nomask=(3, 17, 120), chain8=(3, 17, 120), var31=(3, 17, 120),
                  dpos_tail=(3, 17, 120), trip2_codes=(300, 24, 24), recompute_eval=(3, 17, 120))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_c_planted_faults_miss_a_bound_tenfold(fault):
    B, L, ML = FAULT_CASE[fault]
    c = R.make_case(B, L, ML, "train")
    fw, bw = R.run(c, F64)
    fb, gb = R.bounds(c, fw, bw)
    ff, bf = R.run(c, F64, fault=fault, relu_gate=fw["cache"]["gate"])
    miss = {k: R.ratio(ff[k], fw[k], fb[k]) for k in FWD_KEYS}
    miss.update({n: R.ratio(bf["G"][n], bw["G"][n], gb[n]) for n in R.NAMES})
    print(f"{fault}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in miss.items() if v > 0))
    assert max(miss.values()) >= 10.0, miss
    if fault == "trip2_codes":                                   # nothing of the first trip moves: it is the later trip that is wrong
        assert R.ratio(ff["z"][:R.MAXBLK], fw["z"][:R.MAXBLK], fb["z"][:R.MAXBLK]) == 0.0
