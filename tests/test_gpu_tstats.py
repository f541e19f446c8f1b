"""GPU: per-tensor statistics on the device -- afr_op_tensor_stats / afr_tensor_stats, Engine.tensor_stats and AFR_TENSOR_REPORT.

Yardstick: tests/tstats_ref.py (fp64 sums over the finite elements, classification by bit pattern, the bound (D + 1) 2^-24 sum|term|
derived from the documented order).  min, max, the three counts and numel are compared exactly, for every tensor.

Measured on MI355X, worst fraction of the bound over all tensors of a test: see the lines each test prints (DESIGN.md 4 quotes them)."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

from . import tstats_ref as R
from .op_harness import bands_kept, guarded_bytes
from .util import MINI, ROOT, GlyphConfig, glyph_inputs, load, synth

pytestmark = pytest.mark.gpu

NODROP = replace(MINI, p_embed=0.0, p_attn=0.0, p_fc=0.0)
SMALL = GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2)       # the glyph twin's small net
QNAN, NEG_NAN = 0x7FC00000, 0xFFC01234                                  # a quiet NaN; a negative NaN with a payload


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


PLANTS = np.concatenate([_bits(0x00000000, 0x80000000, 0x00000001), np.array([-1e-40], dtype=np.float32),      # +-0, 1e-45, -1e-40
                         _bits(0x7F800000, 0xFF800000, QNAN, NEG_NAN), np.array([1e18, -1e18], dtype=np.float32)])
PLANTED_AT = (63, 257, 1025)                                            # and C - 1, C + 1, 5C + 1029: first and last elements


@functools.lru_cache(maxsize=None)
def _chunk():
    from ai_font_renderer_amd import _lib
    return int(_lib.lib().afr_tensor_stats_chunk())


def _sizes():
    c = _chunk()
    return [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, c - 4, c - 1, c, c + 1, c + 4, 2 * c + 3, 5 * c + 1029]


def _fill_gaps(n):
    """What lies between the tensors: NaN patterns and 3e38 (one of them read as an element would show in every field)."""
    buf = np.empty(n, dtype=np.float32)
    buf[0::3], buf[1::3], buf[2::3] = _bits(QNAN)[0], np.float32(3e38), _bits(NEG_NAN)[0]
    return buf


@functools.lru_cache(maxsize=None)
def _table(finite_only=False):
    """(flat float32 buffer, [(offset, numel)]): every size of the issue's list, each tensor on a 64-element boundary with at least 64
    elements of gap behind it.  Shared by the tests and never written."""
    c = _chunk()
    g = np.random.default_rng(20260)
    segs, off = [], 64
    for n in _sizes():
        segs.append((off, n))
        off = (off + n + 63) // 64 * 64 + 64
    buf = _fill_gaps(off)
    for o, n in segs:
        x = g.uniform(-4, 4, n).astype(np.float32)
        if not finite_only:
            if n in PLANTED_AT + (c - 1, c + 1, 5 * c + 1029):
                x[:len(PLANTS)], x[-len(PLANTS):] = PLANTS, PLANTS[::-1]
            elif n == 1:
                x[:] = _bits(0x00000001)                        # 1e-45 alone: it is the minimum, the maximum and the sum
            elif n == 2:
                x[:] = _bits(0x80000000, 0x00000000)
            elif n == 3:
                x[:] = (np.float32(-1e-40), _bits(QNAN)[0], np.float32(1.5))
            elif n == 5:
                x[:] = (np.float32(np.inf), np.float32(-np.inf), np.float32(2.0), _bits(NEG_NAN)[0], np.float32(-3.0))
            elif n == 7:
                x[:] = _bits(0x7F800000, 0xFF800000, QNAN, NEG_NAN, 0x7F800001, 0xFF800000, 0x7FFFFFFF)      # no finite element
            elif n == 1023:
                x[5] = np.float32(R.FLT_MAX)
        buf[o:o + n] = x
    buf.setflags(write=False)
    return buf, tuple(segs)


def _seg_array(segs):
    from ai_font_renderer_amd import _lib
    return (_lib.AfrTensorSeg * len(segs))(*[_lib.AfrTensorSeg(int(o), int(n)) for o, n in segs])


def op_stats(a_dev, segs, minus=None):
    """One afr_op_tensor_stats call into guarded output and scratch buffers pre-filled with 0xFF bytes: the guards stay intact and no
    0xFFFFFFFF word is left in either.  Returns the records, int32 [n, 8] on the host."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import ptr, stream
    lib = _lib.lib()
    tab = _seg_array(segs)
    need = int(lib.afr_op_tensor_stats_scratch_bytes(tab, len(segs)))
    assert need == 32 * sum(R.chunks_of(n, _chunk()) for _, n in segs)
    obuf, out = guarded_bytes(32 * len(segs))
    sbuf, scr = guarded_bytes(need)
    _lib.check(lib.afr_op_tensor_stats(ptr(a_dev), ptr(minus), tab, len(segs), ptr(out), ptr(scr), need, stream()))
    del tab                                                     # the host table is not read after the call returns
    torch.cuda.synchronize()
    assert all(bands_kept(obuf)) and all(bands_kept(sbuf))
    raw = out.view(torch.int32).view(len(segs), 8).cpu().numpy()
    assert not (raw == -1).any() and not bool((scr.view(torch.int32) == -1).any())
    return raw


def _check_all(raw, values, what):
    """Every record against the yardstick; values[k] = the float32 elements record k describes.  Returns the worst bound fraction."""
    d = R.decode(raw)
    worst = 0.0
    for k, x in enumerate(values):
        worst = max(worst, R.check_record({f: d[f][k] for f in R.FIELDS}, x, _chunk(), f"{what} tensor {k} ({len(x)} elements)"))
    return worst


def _same_bits(t, u):
    return torch.equal(t.view(torch.int32), u.view(torch.int32))


# ------------------------------------------------------------------------------------------------------ op level
def test_op_planted_table_against_the_yardstick():
    from .gpu_util import dev
    buf, segs = _table()
    a = dev(buf.copy())
    before = a.clone()
    raw = op_stats(a, segs)
    assert _same_bits(a, before)                                 # inputs are only read
    d = R.decode(raw)
    by_n = {n: k for k, (_, n) in enumerate(segs)}
    assert np.isposinf(d["sumsq"][by_n[1023]]) and d["max"][by_n[1023]] == np.float32(R.FLT_MAX)
    k7 = by_n[7]
    assert np.isposinf(d["min"][k7]) and np.isneginf(d["max"][k7]) and d["sum"][k7] == 0 and d["sumsq"][k7] == 0
    assert (int(d["n_nan"][k7]), int(d["n_inf"][k7]), int(d["n_zero"][k7])) == (4, 3, 0)
    assert d["sum"][by_n[1]] == _bits(0x00000001)[0] and d["min"][by_n[1]] == d["max"][by_n[1]] == _bits(0x00000001)[0]
    worst = _check_all(raw, [buf[o:o + n] for o, n in segs], "planted")
    print(f"tensor stats, planted table of {len(segs)} tensors: worst sum / sumsq error at {worst:.3f} of the bound")


def test_op_records_are_local_and_repeat_bit_for_bit():
    """A tensor's record depends on its elements only: alone at offset 0 and inside the table at another offset, the same bits; a
    tensor of more than 64 chunks (the finish's second trip) likewise; the whole table twice, the same bits."""
    from .gpu_util import dev
    c = _chunk()
    buf, segs = _table()
    a = dev(buf.copy())
    full = op_stats(a, segs)
    assert np.array_equal(full, op_stats(a, segs))
    for n in (3, 257, c, c + 1, 2 * c + 3):
        k = [m for _, m in segs].index(n)
        o = segs[k][0]
        assert o != 0
        alone = op_stats(dev(buf[o:o + n].copy()), [(0, n)])
        assert np.array_equal(alone[0], full[k]), n
    n = 65 * c + 7
    x = np.random.default_rng(65).uniform(-4, 4, n).astype(np.float32)
    alone = op_stats(dev(x), [(0, n)])
    worst = _check_all(alone, [x], "65 chunks")
    shifted = np.concatenate([_fill_gaps(128), x, _fill_gaps(64)])
    shifted[3:8] = 1.0
    both = op_stats(dev(shifted), [(0, 10), (128, n)])
    assert np.array_equal(both[1], alone[0])
    print(f"tensor stats, one tensor of {n} elements (65 chunks): {worst:.3f} of the bound, D = {R.chain_depth(n, c)}")


def test_op_difference_mode():
    from .gpu_util import dev
    fin, segs = _table(finite_only=True)
    buf, _ = _table()
    a, af = dev(buf.copy()), dev(fin.copy())
    # minus = a, all finite: every element is a zero
    d = R.decode(op_stats(af, segs, minus=af.clone()))
    assert np.array_equal(d["n_zero"], d["numel"]) and d["numel"].tolist() == [n for _, n in segs]
    for f in ("sumsq", "sum", "min", "max"):
        assert (d[f] == 0).all(), f
    assert not d["n_nan"].any() and not d["n_inf"].any()
    # minus = a with its infinities and NaNs: inf - inf and NaN - NaN count as NaN, everything else is a zero
    raw = op_stats(a, segs, minus=a.clone())
    d = R.decode(raw)
    for k, (o, n) in enumerate(segs):
        bad = int((~R.classify(buf[o:o + n])[0]).sum())
        assert (int(d["n_nan"][k]), int(d["n_inf"][k]), int(d["n_zero"][k])) == (bad, 0, n - bad), (k, n)
    _check_all(raw, [R.difference(buf[o:o + n], buf[o:o + n]) for o, n in segs], "a - a")
    # a random minus (planted values on both sides: inf - finite, finite - inf, 1e18 - (-1e18), denormal differences)
    g = np.random.default_rng(77)
    m = g.uniform(-4, 4, buf.size).astype(np.float32)
    for o, n in segs:
        if n >= 2 * len(PLANTS):
            m[o + 3:o + 3 + len(PLANTS)] = PLANTS[::-1]
            m[o] = buf[o]
    md = dev(m)
    m_before = md.clone()
    raw = op_stats(a, segs, minus=md)
    assert _same_bits(md, m_before)
    worst = _check_all(raw, [R.difference(buf[o:o + n], m[o:o + n]) for o, n in segs], "a - minus")
    print(f"tensor stats, difference mode: worst sum / sumsq error at {worst:.3f} of the bound")


def test_op_argument_errors_launch_nothing():
    from ai_font_renderer_amd import _lib
    from .gpu_util import dev, ptr, stream
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    a = dev(np.ones(1024, dtype=np.float32))
    obuf, out = guarded_bytes(32 * 4)
    sbuf, scr = guarded_bytes(32 * 4)

    def call(segs=((0, 100), (128, 300)), a_=a, minus=None, out_=out, scr_=scr, nbytes=None, nseg=None):
        tab = _seg_array(segs) if segs else None
        return lib.afr_op_tensor_stats(ptr(a_), ptr(minus), tab, len(segs) if nseg is None else nseg, ptr(out_) if out_ is not None else None,
                                       ptr(scr_) if scr_ is not None else None, 32 * 4 if nbytes is None else nbytes, stream())

    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)                                # noqa: E731
    assert lib.afr_op_tensor_stats(ptr(a), None, _seg_array([(0, 8)]), 1, None, ptr(scr), 128, stream()) == EI          # out NULL
    assert lib.afr_op_tensor_stats(ptr(a), None, _seg_array([(0, 8)]), 1, off4(out), ptr(scr), 96, stream()) == EI      # out misaligned
    assert b"16-byte" in lib.afr_last_error()
    assert lib.afr_op_tensor_stats(ptr(a), off4(a), _seg_array([(0, 8)]), 1, ptr(out), ptr(scr), 128, stream()) == EI   # minus misaligned
    assert lib.afr_op_tensor_stats(None, None, _seg_array([(0, 8)]), 1, ptr(out), ptr(scr), 128, stream()) == EI
    assert call(nseg=0) == EI and b"nseg" in lib.afr_last_error()
    assert call(segs=tuple((64 * k, 1) for k in range(257))) == EI and b"nseg" in lib.afr_last_error()
    assert call(segs=((2, 100),)) == EI and b"multiple of 4" in lib.afr_last_error()
    assert call(segs=((-4, 100),)) == EI
    assert call(segs=((0, -1),)) == EI and b"negative" in lib.afr_last_error()
    assert call(nbytes=63) == EI and b"scratch too small" in lib.afr_last_error()
    assert call(segs=((0, 1 << 32),), nbytes=1 << 40) == EU and b"2^32" in lib.afr_last_error()
    assert lib.afr_op_tensor_stats_scratch_bytes(_seg_array([(0, 1 << 32)]), 1) == 0
    assert lib.afr_op_tensor_stats_scratch_bytes(_seg_array([(0, 0), (64, 1), (128, _chunk() + 1)]), 3) == 32 * 4
    torch.cuda.synchronize()
    assert bool((obuf == 0xFF).all()) and bool((sbuf == 0xFF).all())             # nothing was launched
    assert call() == 0                                                           # and the same buffers do take a good call
    torch.cuda.synchronize()
    assert not bool((out[:64] == 0xFF).all()) and all(bands_kept(obuf)) and all(bands_kept(sbuf))


# ------------------------------------------------------------------------------------------------------ plan level
def _case(name):
    """(cfg, x, font, target u8) of a fixture's inputs."""
    if name == "c5-mini":
        from ai_font_renderer_amd.config import C5_MINI
        fx = load("pixel_twin.npz")
        return C5_MINI, torch.from_numpy(fx["x"]), torch.from_numpy(fx["font"]), torch.from_numpy(fx["target_u8"])
    if name == "sheet-mini":
        fx = load("sheet_mini.npz")
        return NODROP, torch.from_numpy(fx["x10"]), None, torch.from_numpy(fx["target_u8"])
    x, font, t = glyph_inputs(SMALL, 300)
    return SMALL, torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(t)


def _engine(cfg, dtype="f32", max_batch=64, **kw):
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(cfg, dtype=dtype, max_batch=max_batch, **kw)
    eng.load_params(synth.make_params(cfg))
    return eng


def _check_engine(eng, which, flat_host, minus_host=None, minus=None):
    st = eng.tensor_stats(which, minus=minus).cpu()
    assert st.names == [nm for nm, _, _, _ in eng.layout] and tuple(st.raw.shape) == (len(eng.layout), 8) and st.raw.dtype == torch.int32
    vals = [flat_host[o:o + k] if minus_host is None else R.difference(flat_host[o:o + k], minus_host[o:o + k]) for _, _, o, k in eng.layout]
    return st, _check_all(st.raw.cpu().numpy(), vals, which)


def _sumsq_chain(eng):
    """The depth of afr_grad_sumsq's own sum over the whole buffer (tests/test_gpu_clip.py _chain): q float4 per lane, q the smallest
    power of two whose blocks fit its 1024-block grid."""
    sizes = [k for _, _, _, k in eng.layout]
    q = 1
    while True:
        blocks = sum(max(1, -(-(n // 4) // (256 * q))) for n in sizes)
        if blocks <= 1024:
            break
        q *= 2
    return q + 1 + 2 + 6 + 2 + -(-max(blocks, 1) // 256) + 8


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("model", ["sheet-mini", "glyph-small", "c5-mini"])
def test_plan_statistics_against_the_host_buffers(model, dtype):
    cfg, x, font, t = _case(model)
    eng = _engine(cfg, dtype, max_batch=x.shape[0])
    eng.forward_loss(x, t, font=font, step=1)
    eng.backward()
    g = eng.flat_grads.cpu().numpy()
    st, worst = _check_engine(eng, "grads", g)
    # the per-tensor sums of squares add up to the global one, within the two bounds added
    total = float(st.sumsq.astype(np.float64).sum())
    ref = sum(float((g[o:o + k].astype(np.float64) ** 2).sum()) for _, _, o, k in eng.layout)
    allow = sum(R.bounds(g[o:o + k], _chunk())[1] for _, _, o, k in eng.layout) + _sumsq_chain(eng) * R.EPS32 * ref
    assert abs(total - float(eng.grad_sumsq())) <= allow, (total, float(eng.grad_sumsq()), allow)
    snap = eng.flat_params.clone()
    eng.adamw_step(lr=1e-3)
    for which, flat in (("params", eng.flat_params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
        worst = max(worst, _check_engine(eng, which, flat.cpu().numpy())[1])
    sd, w = _check_engine(eng, "params", eng.flat_params.cpu().numpy(), snap.cpu().numpy(), minus=snap)
    assert float(sd.norm().sum()) > 0 and sd.nonfinite() == []
    print(f"tensor stats, {model} {dtype}: {len(eng.layout)} tensors, worst sum / sumsq error at {max(worst, w):.3f} of the bound")
    with pytest.raises(ValueError):
        eng.tensor_stats("weights")
    with pytest.raises(ValueError):
        eng.tensor_stats("params", minus=snap[:-4])


def test_plan_refuses_buffers_it_does_not_have_and_follows_the_ema_switch():
    from ai_font_renderer_amd import _lib
    from .gpu_util import ptr, stream
    cfg, x, font, t = _case("glyph-small")
    lion = _engine(cfg, max_batch=x.shape[0], optimizer="lion")
    for which in ("exp_avg_sq", "ema"):
        with pytest.raises(_lib.AfrError) as e:
            lion.tensor_stats(which)
        assert e.value.code == _lib.AFR_ESTATE
    lion.tensor_stats("exp_avg").cpu()
    bare = _engine(cfg, max_batch=x.shape[0], with_optimizer=False)
    with pytest.raises(_lib.AfrError) as e:
        bare.tensor_stats("exp_avg")
    assert e.value.code == _lib.AFR_ESTATE
    lib = _lib.lib()
    obuf, out = guarded_bytes(32 * len(lion.layout))
    assert lib.afr_tensor_stats(lion._plan, 9, None, ptr(out), stream()) == _lib.AFR_EINVAL
    assert lib.afr_tensor_stats(lion._plan, 0, None, None, stream()) == _lib.AFR_EINVAL
    assert lib.afr_tensor_stats(lion._plan, 0, None, C.c_void_p(out.data_ptr() + 8), stream()) == _lib.AFR_EINVAL
    assert lib.afr_tensor_stats(lion._plan, 3, None, ptr(out), stream()) == _lib.AFR_ESTATE
    torch.cuda.synchronize()
    assert bool((obuf == 0xFF).all())                            # nothing was launched
    # with an EMA: inside ema_weights() "params" is what the forward reads -- the average -- and "ema" the other buffer
    eng = _engine(cfg, max_batch=x.shape[0], ema_decay=0.5)
    eng.train_step(x, t, font=font, step=1, lr=1e-2)
    p, e_ = eng.flat_params.cpu().numpy(), eng.flat_ema.cpu().numpy()
    assert not np.array_equal(p, e_)
    _check_engine(eng, "params", p)
    _check_engine(eng, "ema", e_)
    with eng.ema_weights():
        _check_engine(eng, "params", e_)
        _check_engine(eng, "ema", p)
    _check_engine(eng, "params", p)


def _dead_sheet_engine():
    prm = synth.make_params(NODROP)
    prm["fc_output.bias"] = np.full_like(prm["fc_output.bias"], -10.0)
    prm["fc_output.weight"] = np.zeros_like(prm["fc_output.weight"])
    fx = load("sheet_mini.npz")
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(NODROP, dtype="f32", max_batch=fx["x10"].shape[0])
    eng.load_params(prm)
    return eng, torch.from_numpy(fx["x10"]), torch.from_numpy(fx["target_u8"])


def test_dead_output_head_shows_as_all_zero_gradients():
    """fc_output.bias = -10 and a zero fc_output.weight: every pre-activation is below the clamp, so no gradient passes it."""
    eng, x, t = _dead_sheet_engine()
    eng.flat_grads.fill_(1.0)
    eng.forward_loss(x, t, step=1)
    eng.backward()
    st = eng.tensor_stats("grads").cpu()
    assert np.array_equal(st.n_zero, st.numel) and st.numel.tolist() == [k for _, _, _, k in eng.layout]
    assert st.nonfinite() == [] and not st.sumsq.any()
    assert (st.min == 0).all() and (st.max == 0).all()


def test_a_nan_gradient_is_localised():
    cfg, x, font, t = _case("sheet-mini")
    eng = _engine(cfg, max_batch=x.shape[0])
    eng.forward_loss(x, t, step=1)
    eng.backward()
    assert eng.tensor_stats("grads").nonfinite() == []
    eng.grads["fc1.weight"].view(-1)[17] = float("nan")
    st = eng.tensor_stats("grads")
    assert st.nonfinite() == ["fc1.weight"]
    i = st.names.index("fc1.weight")
    assert int(st.n_nan[i]) == 1 and int(st.n_inf[i]) == 0 and np.isfinite(st.sumsq).all()


def test_model_passes_through_and_reuses_its_record_buffer():
    from ai_font_renderer_amd import model as M
    m = M.AttentionFontRenderer(max_length=10, max_batch=8, dtype="f32")
    a = m.tensor_stats("params")
    b = m.tensor_stats("params")
    assert a.raw.data_ptr() == b.raw.data_ptr() and a.names == [k for k, _ in m.named_parameters()]
    p = m.engine.flat_params.cpu().numpy()
    _check_all(b.cpu().raw.cpu().numpy(), [p[o:o + k] for _, _, o, k in m.engine.layout], "model params")


# ------------------------------------------------------------------------------------------------------ CLI
_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from ai_font_renderer_amd import model as M
M.NUM_SAMPLES, M.NUM_EPOCHS, M.OUTPUT_DIR = 96, 1, "out"
torch.manual_seed(42)
M.main(["model.py", "--train"])
"""


def _train_child(cwd, report):
    env = {k: v for k, v in os.environ.items() if k != "AFR_TENSOR_REPORT"}
    if report is not None:
        env["AFR_TENSOR_REPORT"] = report
    return subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_tensor_report_in_the_training_cli(tmp_path):
    """AFR_TENSOR_REPORT=1 python model.py --train in miniature (96 generated sheets, one epoch), each run a fresh child process: the
    block after epoch 0's status line, one line per tensor; everything else -- stdout, the file list, config.txt minus its own entry,
    the saved parameters bit for bit -- is the run without the variable."""
    from ai_font_renderer_amd import config, datagen
    datagen.generate(str(tmp_path / "train_input"), 96)
    for d in ("on", "off"):
        os.makedirs(tmp_path / d)
        shutil.copytree(tmp_path / "train_input", tmp_path / d / "train_input")
    on, off = _train_child(tmp_path / "on", "1"), _train_child(tmp_path / "off", None)
    assert on.returncode == 0 and off.returncode == 0, (on.stderr[-2000:], off.stderr[-2000:])
    lines_on, lines_off = on.stdout.splitlines(), off.stdout.splitlines()
    names = [nm for nm, _, _, _ in config.flat_layout(config.SheetConfig())[0]]
    heads = [i for i, l in enumerate(lines_on) if l == "Tensor report:"]
    assert len(heads) == 1 and heads[0] == [i for i, l in enumerate(lines_on) if l.startswith("Epoch 0, ")][0] + 1
    block = lines_on[heads[0]:heads[0] + 1 + len(names)]
    for nm, l in zip(names, block[1:]):
        assert l.startswith(f"  {nm} ") and all(k in l for k in ("|p| ", "|g| ", "|g|/|p| ", "g zero ", "|dp|/|p| ")) and "NON-FINITE" not in l, l
    dead = "Tensor report: DEAD OUTPUT HEAD (every gradient of fc_output.weight is zero)"
    if lines_on[heads[0] + len(block)] == dead:          # (a head that died within one epoch is reported, and is part of the block)
        block.append(dead)
    rest = lines_on[:heads[0]] + lines_on[heads[0] + len(block):]
    assert rest == lines_off and not any("Tensor report" in l for l in lines_off)
    assert _files(tmp_path / "on") == _files(tmp_path / "off")
    cfg_on, cfg_off = ((tmp_path / d / "out" / "config.txt").read_text().splitlines() for d in ("on", "off"))
    assert cfg_on == cfg_off + ["tensor_report = 1"]
    sd_on, sd_off = (torch.load(tmp_path / d / "font_renderer.pth", map_location="cpu", weights_only=True) for d in ("on", "off"))
    assert list(sd_on) == list(sd_off) == names
    for k in names:
        assert _same_bits(sd_on[k], sd_off[k]), k
    bad = _train_child(tmp_path / "off", "yes")
    assert bad.returncode != 0 and "AFR_TENSOR_REPORT" in bad.stderr
