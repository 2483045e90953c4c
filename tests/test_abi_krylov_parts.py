"""The entry points of the multi-part device solve (c8_krylov_solve_parts, c8_krylov_linear_solve_parts): exported by
libc8.so, declared in include/c8.h, bound in calibr8_amd/lib.py, and what they refuse before they touch a device or
exchange anything."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("c8_krylov_solve_parts", "c8_krylov_linear_solve_parts")


def test_parts_entry_points_are_exported_and_declared():
    from calibr8_amd import lib
    raw = C.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "c8.h")).read()
    bound = {s[0] for s in lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(raw, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in bound, name
    # the struct blocks are reused unchanged: the signature takes the existing option / info types
    assert re.search(r"int c8_krylov_solve_parts\(c8_ctx\* ctx, const c8_system\* sys, double\* const dx\[2\], const c8_krylov_opts\* opts,\s*"
                     r"c8_krylov_info\* info\);", header)


def test_parts_entry_points_refuse_null_arguments_without_a_device():
    from calibr8_amd import lib
    L = lib.load_library()
    info = lib.KrylovInfo(7, 7, 0, 1.0, 1.0)
    assert L.c8_krylov_solve_parts(None, None, None, None, C.byref(info)) == lib.C8_ERR_ARG
    assert b"c8_krylov_solve_parts" in L.c8_last_error()
    assert (info.iters, info.restarts, info.status) == (0, 0, lib.C8_ERR_ARG)
    assert L.c8_krylov_linear_solve_parts(None, None, None) == lib.C8_ERR_ARG
    user = lib.KrylovUser()  # no context in it
    assert L.c8_krylov_linear_solve_parts(C.byref(user), None, None) == lib.C8_ERR_ARG
    assert user.solves == 0


def test_distributed_device_solver_is_exported_and_opt_in():
    import inspect
    import calibr8_amd
    from calibr8_amd import primal
    assert calibr8_amd.distributed_device_solver is primal.distributed_device_solver
    sig = inspect.signature(primal.distributed_device_solver).parameters
    assert sig["rel_tol"].default == 1e-10 and sig["max_iters"].default == 20000
    assert inspect.signature(primal.PrimalDriver.__init__).parameters["solver"].default is None
