"""No device: the two-level preconditioner over parts (C8_PRECOND_TWO_LEVEL_PARTS) at the ABI boundary --
the kind's value is 7 beside the unchanged earlier kinds, the new symbol is declared, exported and bound, null arguments are
refused before anything is touched, the Python names select it while block Jacobi stays the default, and the numpy replay
of the aggregate rule on an owned sub-graph (tests/krylov_parts_replay.py, the reference of the GPU tests) keeps the
properties the definition states."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)


def header():
    return open(os.path.join(ROOT, "include", "c8.h")).read()


def test_the_kind_is_seven_and_the_symbol_is_declared_exported_and_bound():
    from calibr8_amd import lib
    L = lib.load_library()
    lines = header().splitlines()
    assert any(ln.startswith("enum { C8_PRECOND_TWO_LEVEL_PARTS = 7 };") for ln in lines)
    assert "enum { C8_PRECOND_MULTILEVEL = 5 };" in lines and "enum { C8_PRECOND_BLOCK_JACOBI = 0, C8_PRECOND_BLOCK_SGS = 1 };" in lines
    assert (lib.C8_PRECOND_BLOCK_JACOBI, lib.C8_PRECOND_BLOCK_SGS, lib.C8_PRECOND_TWO_LEVEL, lib.C8_PRECOND_MULTILEVEL,
            lib.C8_PRECOND_TWO_LEVEL_PARTS) == (0, 1, 3, 5, 7)
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint c8_krylov_aggregate_base\(c8_ctx\* ctx, int32_t\* base, int32_t\* total_aggregates\);", code)
    assert hasattr(L, "c8_krylov_aggregate_base")
    bound = {s[0]: s for s in lib.SYMBOLS}
    assert bound["c8_krylov_aggregate_base"][1:] == (C.c_int, [C.c_void_p, lib.i32p, lib.i32p])
    # the definition is stated in the header
    for words in ("OWNED sub-graph", "base_r + local id", "n_c^2 doubles", "five all-reduces"):
        assert words in header(), words


def test_null_arguments_are_refused_without_a_device():
    from calibr8_amd import lib
    L = lib.load_library()
    assert L.c8_krylov_set_preconditioner(None, lib.C8_PRECOND_TWO_LEVEL_PARTS, 1) == lib.C8_ERR_ARG
    assert b"c8_krylov_set_preconditioner" in L.c8_last_error()
    never_read = C.cast(C.create_string_buffer(8), C.c_void_p)     # stands for a context; the refusals come first
    base, total = C.c_int32(77), C.c_int32(78)
    for args in ((None, C.byref(base), C.byref(total)), (never_read, None, C.byref(total)), (never_read, C.byref(base), None)):
        assert L.c8_krylov_aggregate_base(*args) == lib.C8_ERR_ARG and b"c8_krylov_aggregate_base" in L.c8_last_error()
        assert (base.value, total.value) == (77, 78)


class _Recorder:
    def __init__(self):
        self.calls = []

    def c8_krylov_set_preconditioner(self, h, kind, sweeps):
        self.calls.append((kind, sweeps))
        return 0


def test_python_names_select_the_kind_and_jacobi_stays_the_default():
    from calibr8_amd import Assembler, device_solver, distributed_device_solver, lib
    asm = Assembler.__new__(Assembler)       # no device: the method under test only passes its arguments on
    asm.L, asm.h = _Recorder(), None
    asm.set_krylov_preconditioner("two_level_parts", 2)
    asm.set_krylov_preconditioner("two_level_parts")
    assert asm.L.calls == [(lib.C8_PRECOND_TWO_LEVEL_PARTS, 2), (lib.C8_PRECOND_TWO_LEVEL_PARTS, 1)]
    with pytest.raises(ValueError):
        asm.set_krylov_preconditioner("two_level_over_parts")
    assert '"two_level_parts"' in inspect.getsource(Assembler.krylov_preconditioner.fget)
    for fn in (device_solver, distributed_device_solver):
        assert inspect.signature(fn).parameters["preconditioner"].default == "jacobi"
    assert "two_level_parts" in distributed_device_solver.__doc__


def grid_graph(nx, ny):
    """node graph of an nx x ny grid of quads (a node and its up to 8 neighbours), rows sorted"""
    ids = np.arange(nx * ny).reshape(ny, nx)
    rows = []
    for j in range(ny):
        for i in range(nx):
            rows.append(np.sort(ids[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2].ravel()))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return ptr, np.concatenate(rows)


def test_the_aggregate_rule_on_an_owned_sub_graph():
    """The library's rule cannot run without a context (and a context needs a device), so this checks the replay the GPU tests
    compare the device with: on the owned sub-graph the three passes give every owned node one aggregate, ids in order of
    creation, no aggregate reaches a node >= num_owned, and with every node owned they are the single-part aggregates."""
    import krylov_parts_replay as R
    ptr, col = grid_graph(9, 7)
    n = 63
    for no in (63, 40, 27, 10, 1):
        agg, nagg = R.owned_aggregates(ptr, col, no)
        assert len(agg) == no and agg.min() == 0 and agg.max() == nagg - 1
        assert np.array_equal(np.unique(agg), np.arange(nagg))
        first = [int(np.nonzero(agg == a)[0][0]) for a in range(nagg)]
        # pass-1 aggregates come first, in ascending id of the node that opened them; members are neighbours of that node
        sub_ptr, sub_col = R.owned_subgraph(ptr, col, no)
        assert (sub_col < no).all()
        for a in range(nagg):
            members = np.nonzero(agg == a)[0]
            roots = [i for i in range(no) if set(members.tolist()) >= set(sub_col[sub_ptr[i]:sub_ptr[i + 1]].tolist())]
            assert len(members) == 1 or roots, (no, a)
        assert first[0] == 0
    full, nfull = R.owned_aggregates(ptr, col, n)
    ref, nref = R.aggregate_replay(ptr, col, n)
    assert nfull == nref and np.array_equal(full, ref)
    # two parts of the grid by the host rules alone: bases are the prefix sums, global ids cover 0 .. total - 1
    owner = (np.arange(n) % 9 > 4).astype(np.int64)
    parts = R.parts_of_graph(ptr, col, owner, 2)
    assert parts[0]["base"] == 0 and parts[1]["base"] == parts[0]["nagg"]
    gagg = np.full(n, -1)
    for q in parts:
        gagg[q["gid"]] = q["base"] + q["agg"]
    assert np.array_equal(np.unique(gagg), np.arange(parts[0]["nagg"] + parts[1]["nagg"]))
    for a in np.unique(gagg):
        assert len(set(owner[gagg == a].tolist())) == 1      # no aggregate crosses the part boundary
