"""GPU: the four ways afr_train_step goes (csrc/afr_api.hip decide_step), each at the smallest configuration another test
already drives down it.

* GLYPH1: C1's net, 95 glyphs, f32 -- forward, loss and backward in one launch, the optimizer inside the grouped reduce.
* SHEET_FUSED: MINI, 40 strings, f32 -- fc_output.weight is stepped inside its weight-gradient GEMM.
* STAGED_FUSED: the 256-256 net of 16x16 glyphs, 300 of them, bf16 -- the staged backward carries the step; the loss sum is
  deferred to the first-layer backward.
* UNFUSED: the same net with AFR_CFG_UNFUSED_OPTIMIZER (flags = 1) -- afr_backward, then afr_adamw_step.

The paths share their kernels: no launch NAME but GLYPH1's is unique to one path.  What tells the other three apart in the
per-launch table (Engine.profile_table) is a row's name together with its launch count and algorithmic bytes; each case names its
row below.
"""
import pytest
import torch

from ai_font_renderer_amd import _lib
from .gpu_util import ptr, stream
from .util import MINI, GlyphConfig, glyph_inputs, synth

pytestmark = pytest.mark.gpu

PRESET = 0.37109375
NET = GlyphConfig(hidden=(256, 256), out_h=16, out_w=16)


def _glyph_case(cfg, B):
    x, font, tu8 = glyph_inputs(cfg, B)
    return torch.from_numpy(x), torch.from_numpy(tu8), torch.from_numpy(font) if cfg.n_fonts else None


def _sheet_case(cfg, B):
    x = synth.encode_strings(synth.dataset_strings(B), cfg.max_length)
    return torch.from_numpy(x), torch.from_numpy(synth.synth_sheet_targets(B, cfg.sheet_h, cfg.sheet_w, tensor_id=974)), None


def _rows(table, name):
    return [r for r in table if r["kernel"].split("[")[0] == name]


def _ran_glyph1(table, eng):
    """`glyph1_step<f32>`: the one-launch step; no other path launches it."""
    assert len(_rows(table, "glyph1_step<f32>")) == 1 and _rows(table, "glyph1_step<f32>")[0]["launches"] == 1, table
    assert not _rows(table, "adamw"), table                  # the optimizer ran inside the grouped reduce


def _ran_sheet_fused(table, eng):
    """`gemm_f32<1,1>[192x640x40]`, the weight gradient of fc_output, with the algorithmic bytes of a product that steps its
    output: the operands once and 24 bytes per element (p, m, v read and written) instead of 4; and `adamw` once, on the 192
    elements of fc_output.bias alone."""
    M, N, K = 192, 640, 40
    dw = [r for r in table if r["kernel"] == "gemm_f32<1,1>[%dx%dx%d]" % (M, N, K)]
    assert len(dw) == 1 and dw[0]["launches"] == 1 and dw[0]["algo_bytes"] == 4.0 * (M * K + N * K) + 24.0 * M * N, table
    ad = _rows(table, "adamw")
    assert len(ad) == 1 and ad[0]["launches"] == 1 and ad[0]["algo_bytes"] == 192 * 28.0, table


def _ran_staged_fused(table, eng):
    """`adamw` four times: at 300 glyphs neither hidden-to-output Linear splits its weight gradient, so fc2 and fc_output write
    weight and bias gradients directly and reduce_and_step gives each of the four tensors the plain kernel; everything else is
    stepped inside `reduce_group`.  (The unfused path launches `adamw` once, over the whole flat buffer.)"""
    ad = _rows(table, "adamw")
    assert len(ad) == 1 and ad[0]["launches"] == 4, table
    assert sum(r["launches"] for r in _rows(table, "reduce_group")) == 1 and sum(r["launches"] for r in _rows(table, "glyph_l1_bwd_fused")) == 1, table


def _ran_unfused(table, eng):
    """`adamw` once, over the whole flat buffer: 28 bytes per element and 2 for the bf16 copy."""
    ad = _rows(table, "adamw")
    assert len(ad) == 1 and ad[0]["launches"] == 1 and ad[0]["algo_bytes"] == eng.n_flat * 30.0, table
    assert sum(r["launches"] for r in _rows(table, "reduce_group")) == 1, table


PATHS = {
    "GLYPH1": (GlyphConfig(hidden=(256,), out_h=16, out_w=16), "f32", 95, 0, _glyph_case, _ran_glyph1),
    "SHEET_FUSED": (MINI, "f32", 40, 0, _sheet_case, _ran_sheet_fused),
    "STAGED_FUSED": (NET, "bf16", 300, 0, _glyph_case, _ran_staged_fused),
    "UNFUSED": (NET, "bf16", 300, 1, _glyph_case, _ran_unfused),
}


def _engine(cfg, dtype, B, flags):
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(cfg, dtype=dtype, max_batch=B, flags=flags)
    eng.load_params(synth.make_params(cfg))
    eng.loss_accum.fill_(PRESET)
    return eng


def _state(eng):
    """(params, exp_avg, exp_avg_sq) as name -> tensor over the tensor elements (the padding between tensors is nobody's)."""
    return [{nm: flat[o:o + k].clone() for nm, shp, o, k in eng.layout} for flat in (eng.flat_params, eng.exp_avg, eng.exp_avg_sq)]


def _assert_same_state(a, b, what):
    for da, db, tag in zip(_state(a), _state(b), ("param", "exp_avg", "exp_avg_sq")):
        for k in da:
            assert torch.equal(da[k], db[k]), (what, tag, k, float((da[k] - db[k]).abs().max()))


def _bits(v):
    return torch.tensor([v], dtype=torch.float32).view(torch.int32).item()


@pytest.mark.parametrize("path", list(PATHS))
def test_refused_step_leaves_nothing_behind_and_the_path_runs(path):
    """afr_train_step(do_step = 1, t = 0) is refused with AFR_EINVAL before anything is enqueued: the accumulator, the
    parameters and both moments keep their bits, a backward finds no forward to continue (AFR_ESTATE), no error bit is set,
    and three ordinary steps afterwards give, bit for bit, the losses, parameters and moments of an engine that was never
    refused.  Then one profiled step shows the row of the per-launch table that only this path writes (the _ran_* docstrings)."""
    cfg, dtype, B, flags, case, ran = PATHS[path]
    x, t, font = case(cfg, B)
    a, b = _engine(cfg, dtype, B, flags), _engine(cfg, dtype, B, flags)
    before = [v.clone() for v in (a.loss_accum, a.flat_params, a.exp_avg, a.exp_avg_sq)]
    xd, fd = a._prep_x(x, font)
    td, tcode = a._target(t)
    L = xd.shape[1] if xd.dim() == 2 else 1
    with torch.cuda.device(a.device):
        rc = a.lib.afr_train_step(a._plan, ptr(xd.reshape(-1) if L == 1 else xd), ptr(fd), ptr(td), tcode, B, L, B * a.pixels, ptr(a.loss_accum), 1,
                                  1, 1e-3, 0.9, 0.99, 1e-8, 5e-4, 0, stream())
    assert rc == _lib.AFR_EINVAL and b"t starts at 1" in a.lib.afr_last_error()
    torch.cuda.synchronize()
    for was, now, what in zip(before, (a.loss_accum, a.flat_params, a.exp_avg, a.exp_avg_sq), ("loss_accum", "flat_params", "exp_avg", "exp_avg_sq")):
        assert torch.equal(was, now), what
    with pytest.raises(_lib.AfrError) as ei:
        a.backward()
    assert ei.value.code == _lib.AFR_ESTATE
    assert a.error_flags() == 0
    reads = {}
    for name, e in (("refused", a), ("fresh", b)):
        reads[name] = []
        for _ in range(3):
            e.train_step(x, t, font=font)
            reads[name].append(e.read_loss(reset=False))
        assert e.error_flags() == 0
    print(path, "losses:", reads["refused"])
    assert [_bits(v) for v in reads["refused"]] == [_bits(v) for v in reads["fresh"]], reads
    assert reads["refused"][0] > PRESET                      # the sum really ran
    _assert_same_state(a, b, path)
    a.profile(1)
    a.train_step(x, t, font=font)
    table = a.profile_table()
    a.profile(0)
    print(path, [(r["kernel"], r["launches"], r["algo_bytes"]) for r in table])
    ran(table, a)


def test_stage_entry_points_see_no_step_context():
    """forward_loss, afr_backward_stage stage by stage, afr_adamw_step on the engine whose afr_train_step takes the staged fused
    path with the deferred loss: the stage entry points hand no step context down, so no weight-gradient launch steps a weight
    and the first-layer backward adds no loss partials.  The result equals, bit for bit, one train_step of the unfused engine:
    the same kernels on the same operands, the slabs summed per stage instead of once at the end, the same stand-alone AdamW."""
    x, t, font = _glyph_case(NET, 300)
    s, u = _engine(NET, "bf16", 300, 0), _engine(NET, "bf16", 300, 1)
    s.forward_loss(x, t, font=font)
    for st in range(s.backward_stages):
        s.backward_stage(st)
    s.adamw_step()
    u.train_step(x, t, font=font)
    ls, lu = s.read_loss(reset=False), u.read_loss(reset=False)
    print("staged entry points: loss", ls, "unfused train_step: loss", lu)
    assert _bits(ls) == _bits(lu) and ls > PRESET, (ls, lu)
    _assert_same_state(s, u, "stage by stage")
    assert s.error_flags() == 0 and u.error_flags() == 0
