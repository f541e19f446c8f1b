"""CPU: the C-ABI library loads and exports every symbol include/afr.h declares (no compute calls)."""
import ctypes as C
import os
import re

import pytest

from .util import ROOT


def _header_functions():
    src = open(os.path.join(ROOT, "include", "afr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(afr_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from ai_font_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = _header_functions()
    assert len(names) >= 20
    lib = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/afr.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert _lib.lib().afr_version() == 1


def test_plan_layout_matches_python_layout_without_gpu():
    """Plan creation is host-only: the flat layout must equal config.flat_layout (checkpoint contract)."""
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    for cfg in (config.SheetConfig(), config.SheetConfig(max_length=10, sheet_h=8, sheet_w=24),
                config.WORKLOADS["c1"]["cfg"], config.WORKLOADS["c3"]["cfg"]):
        c = make_afr_config(cfg, "f32", 64)
        plan = C.c_void_p()
        _lib.check(lib.afr_plan_create(C.byref(c), C.byref(plan)))
        table, total = config.flat_layout(cfg)
        assert lib.afr_param_elems(plan) == total
        assert lib.afr_param_count(plan) == len(table)
        name = C.create_string_buffer(128)
        off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int32()
        shape = (C.c_int64 * 4)()
        for i, (nm, shp, o, n) in enumerate(table):
            _lib.check(lib.afr_param_info(plan, i, name, 128, C.byref(off), C.byref(numel), C.byref(ndim), shape))
            assert (name.value.decode(), off.value, numel.value) == (nm, o, n)
            assert tuple(shape[k] for k in range(ndim.value)) == tuple(shp)
        assert lib.afr_workspace_bytes(plan) > 0
        lib.afr_plan_destroy(plan)


def test_bad_configs_are_rejected_with_a_message():
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    plan = C.c_void_p()
    c = make_afr_config(config.GlyphConfig(hidden=(30,)), "f32", 8)      # width not a multiple of 8
    assert lib.afr_plan_create(C.byref(c), C.byref(plan)) < 0
    assert b"multiple" in lib.afr_last_error()
    c = make_afr_config(config.SheetConfig(max_length=500), "f32", 8)
    assert lib.afr_plan_create(C.byref(c), C.byref(plan)) < 0
    with pytest.raises(_lib.AfrError):
        _lib.check(lib.afr_plan_create(C.byref(c), C.byref(plan)))
    # the sheet front end's one-launch entries refuse what their kernels cannot take, before anything is launched
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)
    prm = _lib.AfrSheetParams(*[0x1000] * 10)
    lay = _lib.AfrSheetSlabLayout(0, 3840, 7936, 11008, 11136, 12160, 12224, 12288, 12352, 14400, 14464)   # max_length 120, vocab 128

    def fwd(dt=0, ldx=24, B=4, L=24, ML=120, vocab=128, drop=None, z=fk, p=prm):
        return lib.afr_op_sheet_fwd(dt, C.byref(p) if p is not None else None, fk, ldx, B, L, ML, vocab, 1e-5, drop, z, None, None, None)

    def bwd(dt=0, ldx=24, B=4, L=24, ML=120, vocab=128, drop=None, dz=fk, slabs=fk, la=lay):
        return lib.afr_op_sheet_bwd(dt, C.byref(prm), fk, ldx, B, L, ML, vocab, 1e-5, drop, dz, None, slabs, C.byref(la) if la is not None else None, None)

    assert lib.afr_sheet_blocks(1) == 1 and lib.afr_sheet_blocks(256) == 256 and lib.afr_sheet_blocks(600) == 256
    assert lib.afr_sheet_save_floats(3, 17) == 3 * 17 * 56
    for call in (fwd, bwd):
        assert call(dt=2) == EI and b"act_dtype" in lib.afr_last_error()                 # AFR_BF16X3 is a plan mode, not an activation type
        assert call(L=0) == EI and b"L = 0" in lib.afr_last_error()
        assert call(L=121, ML=200, ldx=121) == EU and b"120" in lib.afr_last_error()
        assert call(L=30, ML=24, ldx=30) == EI and b"max_length" in lib.afr_last_error()
        assert call(ldx=23) == EI and b"ldx" in lib.afr_last_error()
        assert call(B=0) == EI and b"B = 0" in lib.afr_last_error()
        assert call(vocab=0) == EI
        for rates in ((1.0, 0.0, 0.0), (0.0, -0.1, 0.0), (0.0, 0.0, float("nan"))):
            d = _lib.AfrSheetDropout(42, 1, 0, *rates)
            assert call(drop=C.byref(d)) == EI and b"outside [0, 1)" in lib.afr_last_error()
    assert fwd(z=None) == EI and fwd(p=None) == EI
    assert fwd(p=_lib.AfrSheetParams(*([0x1000] * 9 + [None]))) == EI and b"parameter" in lib.afr_last_error()
    assert bwd(dz=None) == EI and bwd(slabs=None) == EI and bwd(la=None) == EI
    assert bwd(slabs=C.c_void_p(0x1008)) == EI and b"16-byte" in lib.afr_last_error()
    bad = _lib.AfrSheetSlabLayout.from_buffer_copy(lay)
    bad.total = 14466
    assert bwd(la=bad) == EI and b"multiple of 4" in lib.afr_last_error()
    bad = _lib.AfrSheetSlabLayout.from_buffer_copy(lay)
    bad.total = 14460                                                                  # fc1.bias ends at 14464
    assert bwd(la=bad) == EI and b"outside" in lib.afr_last_error()
    bad = _lib.AfrSheetSlabLayout.from_buffer_copy(lay)
    bad.emb = 3836                                                                     # the embedding rows start inside pos
    assert bwd(la=bad) == EI and b"overlap" in lib.afr_last_error()
    bad = _lib.AfrSheetSlabLayout.from_buffer_copy(lay)
    bad.b1 = -64
    assert bwd(la=bad) == EI
    assert bwd(vocab=129) == EI and b"overlap" in lib.afr_last_error()                 # the layout was made for 128 rows


def test_operands_of_2gib_or_more_are_rejected_not_silently_zero_filled():
    """The bf16 LDS-DMA path addresses an operand with 32-bit byte offsets (gemm.hip make_rsrc / stage_inst): an operand of
    2 GiB or more would read zeros past the limit.  Argument validation only -- nothing is launched."""
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    fake = C.c_void_p(0x1000)
    M, K = 32768, 32768                                           # 32768^2 bf16 = 2 GiB
    rc = lib.afr_op_gemm(_lib.AFR_BF16, 0, fake, fake, fake, None, None, M, 1024, K, K, K, 1024, 0, 1, None)
    assert rc == -4 and b"2 GiB" in lib.afr_last_error()          # AFR_EUNSUPPORTED
    plan = C.c_void_p()
    c = make_afr_config(config.SheetConfig(), "bf16", 60000)      # 60000 x 19200 bf16 activations = 2.3 GB
    assert lib.afr_plan_create(C.byref(c), C.byref(plan)) == -4
    assert b"2 GiB" in lib.afr_last_error()
    c = make_afr_config(config.SheetConfig(), "f32", 60000)       # the f32 kernels index with 64-bit arithmetic
    assert lib.afr_plan_create(C.byref(c), C.byref(plan)) == 0
    lib.afr_plan_destroy(plan)


def test_grouped_reduce_refuses_more_segments_than_it_can_hold():
    """afr_rtable_add used to drop the segment past its capacity silently (a gradient would have gone missing); now it is an error."""
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    n = 33
    ptrs = (C.c_void_p * n)(*[0x1000] * n)
    ns = (C.c_int * n)(*[2] * n)
    st = (C.c_int64 * n)(*[64] * n)
    ln = (C.c_int64 * n)(*[64] * n)
    assert lib.afr_op_reduce_group(n, ptrs, ptrs, ns, st, ln, None) == -1      # AFR_EINVAL
    assert b"at most 32" in lib.afr_last_error()


def test_library_sources_read_no_environment_and_keep_one_build_switch():
    """Kernel selection depends on the shapes and config.reserved only: the library reads no environment variables, and
    the one build-time switch left is the GEMM timeline instrumentation (-DAFR_GEMM_TIMING, tools/gemm_timeline.py)."""
    csrc = os.path.join(ROOT, "ai-font-renderer_amd", "csrc")
    sources = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".hpp", ".cpp", ".cc", ".c")))
    assert "gemm.hip" in sources and "afr_api.hip" in sources
    symbols = set()
    for f in sources:
        src = open(os.path.join(csrc, f)).read()
        assert not re.search(r"\bgetenv\s*\(", src), f"{f} calls getenv"
        for cond in re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif|elifdef|elifndef)\b(.*)$", src, flags=re.M):
            symbols |= set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
    assert symbols == {"AFR_GEMM_TIMING"}, symbols
