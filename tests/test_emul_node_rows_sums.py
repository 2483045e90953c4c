"""Phase B of the row-per-node kernels sums over an element's points first and combines the three "a" terms of the (u, u) block
once, after the last point (c8_models.hpp: closed_form_block_sums / closed_form_block_finish): the kernel source run lane by
lane on the CPU.  The meshes and the second plastic step of node_rows_xlane_cases.py, in the form for nodes with at most
eight elements and in the form that takes a node's elements eight at a time: K1 and K3 against the oracle at the suite's bar
and against the emulated staged closed-form wave kernel at 1e-13 (K1, stored state) and 1e-12 (K3); two runs bit for bit;
assign mode against zero-then-accumulate; an elastic step, where the X terms stand alone.  And against an emulator built
from the kernel source BEFORE the change (tests/emul/node_rows_before_sums/): the stored state and the right-hand side bit
for bit, every block of A within 1e-13 of its largest entry.  The CPU twin of test_gpu_node_rows_sums.py.

Mutations of closed_form_block_finish / closed_form_block_sums tried while this was written (not committed), and what failed:
X_ik taken for X_ki: test_second_step_against_oracle_and_wave, test_elastic_step and test_blocks_against_the_source_before on
every mesh and form; a/2 of the element's first point used at all eight: test_second_step_against_oracle_and_wave and
test_blocks_against_the_source_before on every mesh and form (test_elastic_step passes, as it must: a is uniform there)."""
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
from node_rows_sums_cases import (ELASTIC_MESH, assert_inputs_can_show_the_identity_broken, check_elastic, elastic,
                                  no_negative_zero)
from node_rows_xlane_cases import (MESHES, adjoint, check_against_oracle, check_against_wave, check_assign_and_accumulate,
                                   forward, mesh, same_bits)

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


@pytest.fixture(params=[False, True], ids=["lean", "many"])
def form(request):
    em.lib().c8emu_set_node_many(1 if request.param else 0)
    yield request.param
    em.lib().c8emu_set_node_many(0)


def test_inputs_can_show_the_identity_broken():
    assert_inputs_can_show_the_identity_broken()


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
    dut.assign = True
    try:
        ls, xi = forward(dut, case)
        assert no_negative_zero(ls) and no_negative_zero(adjoint(dut, case, xi))
    finally:
        dut.assign = False


def test_elastic_step(form):
    check_elastic(*elastic(_emul(ELASTIC_MESH, "node")), elastic(_emul(ELASTIC_MESH, "wave")), TOL)


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
    shutil.copy(os.path.join(em.EMUL_DIR, "node_rows_before_sums", "c8_assemble_node.hpp"), top / "calibr8_amd" / "csrc")
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
def test_blocks_against_the_source_before(name, many, emulator_before):
    """Phase A, the residual shares and their sum are untouched: xi, b_u and b_p do not change by a bit, forward and adjoint.
    A changes to rounding: the same products summed over the points in the same order, combined after the sum instead of
    before it, and (p, p) closed by one multiplication with 1 / kappa."""
    dut = _emul(name, "node")
    em.lib().c8emu_set_node_many(1 if many else 0)
    try:
        ls, xi = forward(dut, name)
        adj = adjoint(dut, name, xi)
    finally:
        em.lib().c8emu_set_node_many(0)
    with emulator_before(many):
        before = _emul(name, "node")
        ls_b, xi_b = forward(before, name)
        adj_b = adjoint(before, name, xi_b)
    assert np.array_equal(xi, xi_b)
    for what, s, s_b in (("K1", ls, ls_b), ("K3", adj, adj_b)):
        assert np.array_equal(s.b[0], s_b.b[0]) and np.array_equal(s.b[1], s_b.b[1])
        dA = max(float(np.abs(s.A[i][j] - s_b.A[i][j]).max() / np.abs(s_b.A[i][j]).max()) for i in range(2) for j in range(2))
        print(name, what, "A against the source before: %.2e of the block's largest entry" % dA)
        assert dA < 1e-13  # the bound of node against wave (check_against_wave): rounding, not another value
