"""`-m gpu`: phase B of the row-per-node kernels sums over an element's points first and combines the three "a" terms of the
(u, u) block once, after the last point (c8_models.hpp: closed_form_block_sums / closed_form_block_finish).  The meshes and
the second plastic step of node_rows_xlane_cases.py on the device (pinched_bricks runs the form for nodes with more than
eight elements, the others the lean one): `node` against the oracle at the suite's bar and against `wave` at 1e-13 (K1,
stored state) and 1e-12 (K3); two runs bit for bit; assign mode against zero-then-accumulate, forward and adjoint; an
elastic step, where the X terms stand alone.  The device twin of test_emul_node_rows_sums.py."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from node_rows_sums_cases import (ELASTIC_MESH, assert_inputs_can_show_the_identity_broken, check_elastic, elastic,
                                  no_negative_zero)
from node_rows_xlane_cases import (MESHES, adjoint, check_against_oracle, check_against_wave, check_assign_and_accumulate, forward,
                                   mesh, same_bits)

pytestmark = pytest.mark.gpu
TOL = 1e-12  # test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def _backend(name, kernel):
    from gpu_backend import GpuBackend
    c, conn, es, prm = mesh(name)
    return GpuBackend(ol.HEX8, c, conn, "small_J2", prm, scatter="gather", kernel=kernel, elem_set=es)


@functools.lru_cache(maxsize=None)
def _second_step(name, kernel):
    """the second step's assemblies, computed once, shared by the tests and left unchanged: (forward system, state, adjoint system)"""
    be = _backend(name, kernel)
    ls, xi = forward(be, name)
    return ls, xi, adjoint(be, name, xi)


def test_inputs_can_show_the_identity_broken():
    assert_inputs_can_show_the_identity_broken()


@pytest.mark.parametrize("name", MESHES)
def test_second_step_against_oracle_and_wave(name):
    ls, xi, ls_adj = _second_step(name, "node")
    check_against_oracle(name, ls, xi, ls_adj, TOL)
    check_against_wave(name, ls, xi, ls_adj, *_second_step(name, "wave"))


@pytest.mark.parametrize("name", MESHES)
def test_runs_repeat(name):
    ls, xi, ls_adj = _second_step(name, "node")
    be = _backend(name, "node")
    ls2, xi2 = forward(be, name)
    assert same_bits(ls2, ls) and np.array_equal(xi2, xi)
    assert same_bits(adjoint(be, name, xi), ls_adj)


@pytest.mark.parametrize("name", MESHES)
def test_assign_equals_zero_then_accumulate(name):
    be = _backend(name, "node")
    check_assign_and_accumulate(name, be, be.asm.set_assign_mode)
    be.asm.set_assign_mode(True)
    try:
        ls, xi = forward(be, name)
        assert no_negative_zero(ls) and no_negative_zero(adjoint(be, name, xi))
    finally:
        be.asm.set_assign_mode(False)


def test_elastic_step():
    check_elastic(*elastic(_backend(ELASTIC_MESH, "node")), elastic(_backend(ELASTIC_MESH, "wave")), TOL)
