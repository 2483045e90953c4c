"""The entry points of the two-level preconditioner of the device solve (C8_PRECOND_TWO_LEVEL, c8_krylov_aggregates,
c8_krylov_coarse_matrix): exported by libc8.so, declared in include/c8.h, bound in calibr8_amd/lib.py, and what they refuse
before they touch a device."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("c8_krylov_aggregates", "c8_krylov_coarse_matrix")


def test_two_level_entry_points_are_exported_and_declared():
    from calibr8_amd import lib
    raw = C.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "c8.h")).read()
    bound = {s[0]: s for s in lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(raw, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in bound, name
    assert re.search(r"enum \{ C8_PRECOND_TWO_LEVEL = 3 \};", header)
    assert re.search(r"enum \{ C8_PRECOND_BLOCK_JACOBI = 0, C8_PRECOND_BLOCK_SGS = 1 \};", header)   # the earlier kinds keep their values
    assert (lib.C8_PRECOND_BLOCK_JACOBI, lib.C8_PRECOND_BLOCK_SGS, lib.C8_PRECOND_TWO_LEVEL) == (0, 1, 3)
    assert re.search(r"int c8_krylov_aggregates\(c8_ctx\* ctx, int32_t\* num_aggregates, const int32_t\*\* aggregate_of_node\);", header)
    assert re.search(r"int c8_krylov_coarse_matrix\(c8_ctx\* ctx, const c8_system\* sys, int32_t\* n_coarse, double\* out_host\);", header)
    assert bound["c8_krylov_aggregates"][1:] == (C.c_int, [C.c_void_p, lib.i32p, C.POINTER(lib.i32p)])
    assert bound["c8_krylov_coarse_matrix"][1:] == (C.c_int, [C.c_void_p, C.POINTER(lib.System), lib.i32p, lib.dp])
    assert "two levels, dense coarse solve, capped" in header


def test_two_level_entry_points_refuse_null_arguments_without_a_device():
    from calibr8_amd import lib
    L = lib.load_library()
    assert L.c8_krylov_set_preconditioner(None, lib.C8_PRECOND_TWO_LEVEL, 1) == lib.C8_ERR_ARG
    assert b"c8_krylov_set_preconditioner" in L.c8_last_error()
    na, ptr = C.c_int32(7), C.POINTER(C.c_int32)()
    assert L.c8_krylov_aggregates(None, C.byref(na), C.byref(ptr)) == lib.C8_ERR_ARG
    assert b"c8_krylov_aggregates" in L.c8_last_error()
    assert na.value == 7 and not ptr
    n = C.c_int32(7)
    assert L.c8_krylov_coarse_matrix(None, None, C.byref(n), None) == lib.C8_ERR_ARG
    assert b"c8_krylov_coarse_matrix" in L.c8_last_error()
    assert n.value == 7


def test_the_two_level_kind_is_selectable_in_python():
    from calibr8_amd import Assembler, primal
    src = inspect.getsource(Assembler.set_krylov_preconditioner)
    assert '"two_level": _l.C8_PRECOND_TWO_LEVEL' in src
    for fn in (primal.device_solver, primal.distributed_device_solver):
        assert inspect.signature(fn).parameters["preconditioner"].default == "jacobi"   # block Jacobi stays the default
