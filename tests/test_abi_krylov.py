"""The structs of the device-resident linear solve (c8_krylov_opts, c8_krylov_info, c8_krylov_user) as gcc -std=c11 and
g++ -std=c++17 lay them out, against their ctypes mirror in calibr8_amd/lib.py; and what the entry points refuse before
they touch a device."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("c8_abi_client_krylov"))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "abi_client_krylov"), "-s", "OUT=" + out])
    return [json.loads(subprocess.check_output([os.path.join(out, b)])) for b in ("layout_c", "layout_cpp")]


def test_krylov_structs_match_the_ctypes_mirror(layouts):
    from calibr8_amd import lib
    c_layout, cpp_layout = layouts
    assert c_layout == cpp_layout
    mirror = {"c8_krylov_opts": lib.KrylovOpts, "c8_krylov_info": lib.KrylovInfo, "c8_krylov_user": lib.KrylovUser}
    assert sorted(c_layout) == sorted(mirror)
    for name, cls in mirror.items():
        lay = c_layout[name]
        assert C.sizeof(cls) == lay["sizeof"], name
        fields = [f for f in lay if f != "sizeof"]
        assert fields == [f[0] for f in cls._fields_], (name, fields)  # same members, same order
        for f in fields:
            assert getattr(cls, f).offset == lay[f], (name, f)


def test_krylov_entry_points_refuse_null_arguments_without_a_device():
    from calibr8_amd import lib
    L = lib.load_library()
    info = lib.KrylovInfo(7, 7, 0, 1.0, 1.0)
    assert L.c8_krylov_solve(None, None, None, None, C.byref(info)) == lib.C8_ERR_ARG
    assert b"c8_krylov_solve" in L.c8_last_error()
    assert (info.iters, info.restarts, info.status) == (0, 0, lib.C8_ERR_ARG)
    assert L.c8_krylov_linear_solve(None, None, None) == lib.C8_ERR_ARG
    user = lib.KrylovUser()  # no context in it
    assert L.c8_krylov_linear_solve(C.byref(user), None, None) == lib.C8_ERR_ARG
    assert user.solves == 0


def test_device_solver_is_exported_and_opt_in():
    import inspect
    import calibr8_amd
    from calibr8_amd import primal
    assert calibr8_amd.device_solver is primal.device_solver
    # no solver given = the host direct solve, as before (tests/test_gpu_krylov.py runs both)
    assert inspect.signature(primal.PrimalDriver.__init__).parameters["solver"].default is None
