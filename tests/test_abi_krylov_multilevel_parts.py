"""No device: the multilevel preconditioner over parts (C8_PRECOND_MULTILEVEL_PARTS) at the ABI
boundary -- the kind's value is 9 beside the unchanged earlier kinds, the header states the definition, null arguments are
refused before anything is touched, the Python names select it while block Jacobi stays the default, and the level-1 graph
rule of the numpy replay (tests/krylov_parts_multilevel_replay.py, the reference of the GPU tests) has the properties the
definition states."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_abi_krylov_two_level_parts import grid_graph, header  # noqa: E402


def test_the_kind_is_nine_and_the_header_states_the_definition():
    from calibr8_amd import lib
    lines = header().splitlines()
    assert any(ln.startswith("enum { C8_PRECOND_MULTILEVEL_PARTS = 9 };") for ln in lines)
    assert any(ln.startswith("enum { C8_PRECOND_TWO_LEVEL_PARTS = 7 };") for ln in lines)
    assert "enum { C8_PRECOND_MULTILEVEL = 5 };" in lines and "enum { C8_PRECOND_BLOCK_JACOBI = 0, C8_PRECOND_BLOCK_SGS = 1 };" in lines
    assert (lib.C8_PRECOND_BLOCK_JACOBI, lib.C8_PRECOND_BLOCK_SGS, lib.C8_PRECOND_TWO_LEVEL, lib.C8_PRECOND_MULTILEVEL,
            lib.C8_PRECOND_TWO_LEVEL_PARTS, lib.C8_PRECOND_MULTILEVEL_PARTS) == (0, 1, 3, 5, 7, 9)
    for words in ("replicated on every rank", "base_r +", "nnz_1 x NC^2 doubles", "one all-reduce of the n_1 doubles", "five all-reduces",
                  "bitwise equal on every rank", "names its size and what ended the recursion", "c8_krylov_level_matrix(l >= 1) is COLLECTIVE"):
        assert words in header(), words


def test_null_arguments_are_refused_without_a_device():
    from calibr8_amd import lib
    L = lib.load_library()
    assert L.c8_krylov_set_preconditioner(None, lib.C8_PRECOND_MULTILEVEL_PARTS, 1) == lib.C8_ERR_ARG
    assert b"c8_krylov_set_preconditioner" in L.c8_last_error()
    assert L.c8_krylov_set_multilevel(None, 100, 3) == lib.C8_ERR_ARG and b"c8_krylov_set_multilevel" in L.c8_last_error()
    never_read = C.cast(C.create_string_buffer(8), C.c_void_p)     # stands for a context; the refusals come first
    n = C.c_int32(77)
    assert L.c8_krylov_levels(None, C.byref(n)) == lib.C8_ERR_ARG and L.c8_krylov_levels(never_read, None) == lib.C8_ERR_ARG
    assert L.c8_krylov_level_matrix(never_read, None, 1, C.byref(n), None) == lib.C8_ERR_ARG and b"c8_krylov_level_matrix" in L.c8_last_error()
    assert L.c8_krylov_level_matrix(None, None, 1, C.byref(n), None) == lib.C8_ERR_ARG
    assert n.value == 77


class _Recorder:
    def __init__(self):
        self.calls = []

    def c8_krylov_set_preconditioner(self, h, kind, sweeps):
        self.calls.append((kind, sweeps))
        return 0

    def c8_krylov_set_multilevel(self, h, coarse_max, max_levels):
        self.calls.append(("levels", coarse_max, max_levels))
        return 0


def test_python_names_select_the_kind_and_jacobi_stays_the_default():
    from calibr8_amd import Assembler, device_solver, distributed_device_solver, lib
    asm = Assembler.__new__(Assembler)       # no device: the methods under test only pass their arguments on
    asm.L, asm.h = _Recorder(), None
    asm.set_krylov_preconditioner("multilevel_parts", 2)
    asm.set_krylov_preconditioner("multilevel_parts")
    asm.set_krylov_multilevel(coarse_max=100, max_levels=3)
    assert asm.L.calls == [(lib.C8_PRECOND_MULTILEVEL_PARTS, 2), (lib.C8_PRECOND_MULTILEVEL_PARTS, 1), ("levels", 100, 3)]
    with pytest.raises(ValueError):
        asm.set_krylov_preconditioner("multilevel_over_parts")
    assert '"multilevel_parts"' in inspect.getsource(Assembler.krylov_preconditioner.fget)
    for fn in (device_solver, distributed_device_solver):
        assert inspect.signature(fn).parameters["preconditioner"].default == "jacobi"
    assert "multilevel_parts" in distributed_device_solver.__doc__ and "C8_PRECOND_MULTILEVEL_PARTS" in distributed_device_solver.__doc__


def test_the_level_one_graph_rule_on_the_two_part_grid():
    """The library's rule needs a context (and a context needs a device), so this checks the replay the GPU tests compare
    the device with, on the two-part grid of test_the_aggregate_rule_on_an_owned_sub_graph: the level-1 graph is symmetric,
    holds every aggregate itself, and equals next_graph of the global graph under the global aggregate ids -- also when it is
    put together the way the ranks do it, every part from its own owned rows."""
    import krylov_parts_multilevel_replay as M
    import krylov_parts_replay as R
    ptr, col = grid_graph(9, 7)
    n = 63
    owner = (np.arange(n) % 9 > 4).astype(np.int64)
    parts = R.parts_of_graph(ptr, col, owner, 2)
    gagg, total = M.global_aggregates(parts, n)
    assert total == parts[0]["nagg"] + parts[1]["nagg"]
    rp1, ci1 = M.level1_graph(ptr, col, parts, n)
    assert len(rp1) == total + 1 and rp1[-1] == len(ci1)
    G = np.zeros((total, total), dtype=bool)
    G[np.repeat(np.arange(total), np.diff(rp1)), ci1] = True
    assert G.diagonal().all() and np.array_equal(G, G.T)
    assert all((np.diff(ci1[rp1[i]:rp1[i + 1]]) > 0).all() for i in range(total))      # rows in ascending global id
    rp2, ci2 = M.next_graph(ptr, col, gagg, total)
    assert np.array_equal(rp1, rp2) and np.array_equal(ci1, ci2)
    # rank by rank: the rows of a part's own aggregates come from its owned nodes' whole rows, other parts' columns included
    H = np.zeros((total, total), dtype=bool)
    for q in parts:
        for i in q["gid"]:
            H[gagg[i], gagg[col[ptr[i]:ptr[i + 1]]]] = True
    assert np.array_equal(G, H)
    assert (G[:parts[0]["nagg"], parts[0]["nagg"]:]).any()                             # the parts do couple on level 1
    # the levels below by the single-part rules: the counts fall, the last level has no aggregates
    levels = M.levels_below(rp1, ci1, M.part_centroids(np.stack([np.arange(n) % 9, np.arange(n) // 9], axis=1).astype(float), parts), 3, 1, 8)
    counts = [L["n"] for L in levels]
    assert counts[0] == total and counts == sorted(counts, reverse=True) and len(set(counts)) == len(counts) and "agg" not in levels[-1]
    assert [L["n"] for L in M.levels_below(rp1, ci1, levels[0]["x"], 3, 1, 2)] == [total]  # max_levels 2: level 1 is the last
