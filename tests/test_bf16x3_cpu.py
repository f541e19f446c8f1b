"""CPU: the bf16x3 mode (AFR_BF16X3) at the C ABI -- dtype value, plan creation, layout and workspace (no compute calls)."""
import ctypes as C
import os
import re

import pytest

from .util import ROOT


def _lib():
    from ai_font_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _plan(lib, c):
    plan = C.c_void_p()
    rc = lib.afr_plan_create(C.byref(c), C.byref(plan))
    return rc, plan


def test_header_and_python_agree_on_the_dtype_value():
    _l = _lib()
    src = open(os.path.join(ROOT, "include", "afr.h")).read()
    m = re.search(r"\bAFR_BF16X3\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == _l.AFR_BF16X3 == 2


@pytest.mark.parametrize("workload", ["r0", "c3", "c5"])
def test_bf16x3_plan_has_the_f32_plans_layout_and_workspace(workload):
    _l = _lib()
    from ai_font_renderer_amd import config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _l.lib()
    cfg, B = config.WORKLOADS[workload]["cfg"], min(64, config.WORKLOADS[workload]["batch"])
    plans = {}
    for dt in ("f32", "bf16x3"):
        c = make_afr_config(cfg, dt, B)
        assert c.dtype == {"f32": 0, "bf16x3": 2}[dt]
        rc, plan = _plan(lib, c)
        assert rc == 0, lib.afr_last_error()
        n = lib.afr_param_count(plan)
        name = C.create_string_buffer(128)
        off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int32()
        shape = (C.c_int64 * 4)()
        table = []
        for i in range(n):
            _l.check(lib.afr_param_info(plan, i, name, 128, C.byref(off), C.byref(numel), C.byref(ndim), shape))
            table.append((name.value.decode(), off.value, numel.value, tuple(shape[k] for k in range(ndim.value))))
        plans[dt] = (table, lib.afr_param_elems(plan), lib.afr_workspace_bytes(plan), lib.afr_backward_stages(plan))
        lib.afr_plan_destroy(plan)
    assert plans["bf16x3"] == plans["f32"]
    assert plans["f32"][0] and plans["f32"][2] > 0


def test_op_gemm_rejects_a_bf16_output_and_unknown_dtypes():
    """Argument validation only: nothing is launched (the pointers are never dereferenced)."""
    _l = _lib()
    lib = _l.lib()
    fake = C.c_void_p(0x1000)
    rc = lib.afr_op_gemm(_l.AFR_BF16X3, _l.GEMM_OUT_BF16, fake, fake, fake, None, None, 64, 64, 64, 64, 64, 64, 0, 1, None)
    assert rc == -1 and b"AFR_GEMM_OUT_BF16" in lib.afr_last_error()          # AFR_EINVAL
    for bad in (3, -1):
        rc = lib.afr_op_gemm(bad, 0, fake, fake, fake, None, None, 64, 64, 64, 64, 64, 64, 0, 1, None)
        assert rc == -1 and b"dtype" in lib.afr_last_error(), bad


def test_plan_rejects_dtype_3():
    _l = _lib()
    from ai_font_renderer_amd import config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _l.lib()
    c = make_afr_config(config.SheetConfig(max_length=10, sheet_h=8, sheet_w=24), "f32", 8)
    c.dtype = 3
    rc, _ = _plan(lib, c)
    assert rc == -1 and b"dtype" in lib.afr_last_error()


def test_engine_and_facade_know_the_mode_name():
    from ai_font_renderer_amd import engine
    assert engine._DT["bf16x3"] == 2
