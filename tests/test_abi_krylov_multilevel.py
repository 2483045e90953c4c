"""No device: the multilevel preconditioner at the ABI boundary -- its symbols are declared, exported and bound, the kind's
value is 5 beside the unchanged earlier kinds, null arguments are refused before anything is touched, and the Python names
select it while block Jacobi stays the default."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["c8_krylov_set_multilevel", "c8_krylov_levels", "c8_krylov_level", "c8_krylov_level_matrix"]


def header():
    return open(os.path.join(ROOT, "include", "c8.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from calibr8_amd import lib
    L = lib.load_library()
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    bound = {s[0]: s for s in lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][1] is C.c_int, name
    # the argument lists of the ctypes table follow the declarations
    assert len(bound["c8_krylov_set_multilevel"][2]) == 3 and len(bound["c8_krylov_levels"][2]) == 2
    assert len(bound["c8_krylov_level"][2]) == 7 and len(bound["c8_krylov_level_matrix"][2]) == 5


def test_the_kind_is_five_and_the_earlier_kinds_are_unchanged():
    from calibr8_amd import lib
    lines = header().splitlines()
    assert "enum { C8_PRECOND_MULTILEVEL = 5 };" in lines                      # on a line of its own
    assert "enum { C8_PRECOND_BLOCK_JACOBI = 0, C8_PRECOND_BLOCK_SGS = 1 };" in lines
    assert any(ln.startswith("enum { C8_PRECOND_TWO_LEVEL = 3 };  /* 2 stays unassigned:") for ln in lines)
    assert "two levels, dense coarse solve, capped" in header()
    assert (lib.C8_PRECOND_BLOCK_JACOBI, lib.C8_PRECOND_BLOCK_SGS, lib.C8_PRECOND_TWO_LEVEL, lib.C8_PRECOND_MULTILEVEL) == (0, 1, 3, 5)


def test_null_arguments_are_refused_and_leave_the_out_arguments_untouched():
    """null context, and null pointers beside a context that is never read: every check comes before any use"""
    from calibr8_amd import lib
    L = lib.load_library()
    i32p = C.POINTER(C.c_int32)
    never_read = C.cast(C.create_string_buffer(8), C.c_void_p)     # stands for a context; the refusals come first
    sy = lib.System()
    n, m = C.c_int32(77), C.c_int32(78)
    ap, cp, nd = i32p(n), i32p(n), i32p(n)
    here = C.addressof(n)

    def untouched():
        return (n.value, m.value) == (77, 78) and all(C.addressof(p.contents) == here for p in (ap, cp, nd))

    assert L.c8_krylov_set_multilevel(None, 100, 3) == lib.C8_ERR_ARG and b"c8_krylov_set_multilevel" in L.c8_last_error()
    for ctx, out in ((None, C.byref(n)), (never_read, None)):
        assert L.c8_krylov_levels(ctx, out) == lib.C8_ERR_ARG and b"c8_krylov_levels" in L.c8_last_error()
        assert untouched()
    full = [C.byref(n), C.byref(ap), C.byref(m), C.byref(cp), C.byref(nd)]
    assert L.c8_krylov_level(None, 0, *full) == lib.C8_ERR_ARG and b"c8_krylov_level:" in L.c8_last_error()
    for k in range(5):
        args = list(full)
        args[k] = None
        assert L.c8_krylov_level(never_read, 0, *args) == lib.C8_ERR_ARG and b"c8_krylov_level:" in L.c8_last_error()
        assert untouched()
    for ctx, sys_, out in ((None, C.byref(sy), C.byref(n)), (never_read, None, C.byref(n)), (never_read, C.byref(sy), None)):
        assert L.c8_krylov_level_matrix(ctx, sys_, 1, out, None) == lib.C8_ERR_ARG and b"c8_krylov_level_matrix" in L.c8_last_error()
        assert untouched()


class _Recorder:
    """stands for the library behind an Assembler: records the calls of the two setters"""

    def __init__(self):
        self.calls = []

    def c8_krylov_set_preconditioner(self, h, kind, sweeps):
        self.calls.append(("kind", kind, sweeps))
        return 0

    def c8_krylov_set_multilevel(self, h, coarse_max, max_levels):
        self.calls.append(("levels", coarse_max, max_levels))
        return 0


def test_python_names_select_the_kind_and_jacobi_stays_the_default():
    from calibr8_amd import Assembler, device_solver, distributed_device_solver, lib
    asm = Assembler.__new__(Assembler)       # no device: the methods under test only pass their arguments on
    asm.L, asm.h = _Recorder(), None
    asm.set_krylov_preconditioner("multilevel", 2)
    asm.set_krylov_multilevel()
    asm.set_krylov_multilevel(coarse_max=256, max_levels=4)
    asm.set_krylov_preconditioner("two_level")
    assert asm.L.calls == [("kind", lib.C8_PRECOND_MULTILEVEL, 2), ("levels", 0, 0), ("levels", 256, 4), ("kind", lib.C8_PRECOND_TWO_LEVEL, 1)]
    with pytest.raises(ValueError):
        asm.set_krylov_preconditioner("multigrid")
    for fn in (device_solver, distributed_device_solver):
        assert inspect.signature(fn).parameters["preconditioner"].default == "jacobi"
    internal = open(os.path.join(ROOT, "calibr8_amd", "csrc", "c8_api_internal.hpp")).read()
    assert "int kry_precond = C8_PRECOND_BLOCK_JACOBI" in internal         # the state of a fresh context
