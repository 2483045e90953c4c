"""Phase B of the row-per-node kernels forms dN_m/dx from the inverse Jacobian another lane of the element holds and takes it
by a lane exchange (c8_assemble_node.hpp, lane_xor8): the kernel source run lane by lane on the CPU, where the exchange is
the header's own fall-back, get evaluated for the partner lane.  The meshes and the second plastic step of
node_rows_xlane_cases.py, in the form for nodes with at most eight elements and in the form that takes a node's elements
eight at a time: K1 and K3 against the oracle at the suite's bar and against the emulated staged closed-form wave kernel at
1e-13 (K1, stored state) and 1e-12 (K3); two runs bit for bit; assign mode against zero-then-accumulate.  And the
relabelling of phase A alone (lane l owns point hex_code(l)): the stored state and the right-hand side bit for bit those
of the kernel source BEFORE the change, a frozen copy of which (tests/emul/node_rows_before_xlane/) is built into a
second emulator.  The CPU twin of test_gpu_node_rows_xlane.py."""
import contextlib
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import emul_lib as em
import oracle_lib as ol
from node_rows_xlane_cases import (MESHES, NOT_PARALLELEPIPEDS, adjoint, check_against_oracle, check_against_wave,
                                   check_assign_and_accumulate, face_defects, forward, mesh, same_bits)

TOL = 1e-12  # test_emul_parity.py
CASES = [(n, m) for n in MESHES for m in (False, True)]
ROOT = os.path.dirname(em.HERE)


def _emul(name, kernel):
    c, conn, es, prm = mesh(name)
    dut = em.Emul(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)
    if kernel == "node":
        dut.node = dut.wave = True
    else:  # the staged one-wavefront-per-element kernel in its closed form
        dut.wave = dut.staged = True
    return dut


@functools.lru_cache(maxsize=None)
def _wave(name):
    """the staged wave kernels' second step, computed once: (forward system, state, adjoint system)"""
    wave = _emul(name, "wave")
    ls, xi = forward(wave, name)
    return ls, xi, adjoint(wave, name, xi)


@pytest.fixture(params=CASES, ids=["%s-%s" % (n, "many" if m else "lean") for n, m in CASES])
def case(request):
    name, many = request.param
    em.lib().c8emu_set_node_many(1 if many else 0)
    yield name
    em.lib().c8emu_set_node_many(0)


@pytest.mark.parametrize("name", NOT_PARALLELEPIPEDS)
def test_elements_are_not_parallelepipeds(name):
    d = face_defects(name)
    print(name, "x0 - x1 + x2 - x3 over the face diagonal: %.2e .. %.2e" % (d.min(), d.max()))
    assert (d > 1e-3).all()


def test_second_step_against_oracle_and_wave(case):
    dut = _emul(case, "node")
    ls, xi = forward(dut, case)
    ls_adj = adjoint(dut, case, xi)
    check_against_oracle(case, ls, xi, ls_adj, TOL)
    check_against_wave(case, ls, xi, ls_adj, *_wave(case))


def test_runs_repeat(case):
    dut = _emul(case, "node")
    ls, xi = forward(dut, case)
    ls2, xi2 = forward(dut, case)
    assert same_bits(ls2, ls) and np.array_equal(xi2, xi)
    assert same_bits(adjoint(dut, case, xi), adjoint(dut, case, xi))


def test_assign_equals_zero_then_accumulate(case):
    dut = _emul(case, "node")

    def set_assign(on):
        dut.assign = on
    check_assign_and_accumulate(case, dut, set_assign)


@pytest.fixture(scope="module")
def emulator_before(tmp_path_factory):
    """the emulator built from this tree with c8_assemble_node.hpp replaced by its frozen copy from before the change"""
    top = tmp_path_factory.mktemp("emul_before")
    csrc = os.path.join(ROOT, "calibr8_amd", "csrc")
    shutil.copytree(csrc, top / "calibr8_amd" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.hip", ".flags"))
    shutil.copytree(os.path.join(ROOT, "include"), top / "include")
    os.makedirs(top / "tests" / "emul")
    shutil.copy(os.path.join(em.EMUL_DIR, "c8_emul.cpp"), top / "tests" / "emul")
    shutil.copy(os.path.join(em.EMUL_DIR, "Makefile"), top / "tests" / "emul")
    shutil.copy(os.path.join(em.HERE, "math_ops.hpp"), top / "tests")
    shutil.copy(os.path.join(em.EMUL_DIR, "node_rows_before_xlane", "c8_assemble_node.hpp"), top / "calibr8_amd" / "csrc")
    subprocess.check_call(["make", "-C", str(top / "tests" / "emul"), "-s"])
    before = C.CDLL(str(top / "tests" / "emul" / "libc8emul.so"))
    now = em.lib()
    before.c8emu_call.restype, before.c8emu_call.argtypes = now.c8emu_call.restype, now.c8emu_call.argtypes

    @contextlib.contextmanager
    def use(many):
        before.c8emu_set_node_many(1 if many else 0)
        em._lib = before
        try:
            yield
        finally:
            em._lib = now
            before.c8emu_set_node_many(0)
    return use


@pytest.mark.parametrize("many", [False, True], ids=["lean", "many"])
@pytest.mark.parametrize("name", MESHES)
def test_state_and_rhs_have_the_bits_of_the_source_before(name, many, emulator_before):
    """Per point, phase A runs the operations it ran, in their order, on another lane: xi and b (the sum over the points of
    the shares phase A leaves in the records, in ascending point order) do not change by a bit.  A does: phase B sums the
    points in another order and takes dN_m/dx from G."""
    dut = _emul(name, "node")
    em.lib().c8emu_set_node_many(1 if many else 0)
    try:
        ls, xi = forward(dut, name)
    finally:
        em.lib().c8emu_set_node_many(0)
    with emulator_before(many):
        ls_b, xi_b = forward(_emul(name, "node"), name)
    assert np.array_equal(xi, xi_b)
    assert np.array_equal(ls.b[0], ls_b.b[0]) and np.array_equal(ls.b[1], ls_b.b[1])
    dA = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip([ls.A[i][j] for i in range(2) for j in range(2)],
                                                                          [ls_b.A[i][j] for i in range(2) for j in range(2)]))
    print(name, "A against the source before: %.2e of the block's largest entry" % dA)
    assert dA < 1e-13  # the bound of node against wave (check_against_wave): rounding, not another value
