"""The row-per-node kernels issue their loads one phase ahead and carry them in the lane record (c8_assemble_node.hpp): the
kernel source run lane by lane on the CPU on a second plastic step whose previous state differs from point to point
(node_rows_chain_cases.py), in the form for nodes with at most eight elements and in the form that takes a node's elements
eight at a time.  K1 and K3 against the oracle at the suite's bar and against the emulated staged closed-form wave kernel
at 1e-13 (K1, stored state) and 1e-12 (K3); two runs bit for bit; assign and accumulate mode; two node ranges against one
call.  The CPU twin of test_gpu_node_rows_chain.py."""
import functools

import numpy as np
import pytest

import emul_lib as em
import oracle_lib as ol
from node_rows_chain_cases import (MESHES, adjoint, check_against_oracle, check_against_wave, check_assign_and_accumulate, forward,
                                   mesh, same_bits)

TOL = 1e-12  # test_emul_parity.py
CASES = [(n, m) for n in MESHES for m in (False, True)]


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


def test_assign_then_accumulate(case):
    dut = _emul(case, "node")

    def set_assign(on):
        dut.assign = on
    check_assign_and_accumulate(case, dut, set_assign)


def test_two_node_ranges_equal_one_call(case):
    dut = _emul(case, "node")
    ls, xi = forward(dut, case)
    ls_adj = adjoint(dut, case, xi)
    dut.staged = True  # the upper half of the nodes first, then the lower half
    ls2, xi2 = forward(dut, case)
    assert same_bits(ls2, ls) and np.array_equal(xi2, xi)
    assert same_bits(adjoint(dut, case, xi), ls_adj)
