"""`-m gpu`: the row-per-node kernels issue their loads one phase ahead and carry them in the lane record
(c8_assemble_node.hpp).  The meshes of node_rows_chain_cases.py on the device, on a second plastic step whose previous
state differs from point to point: `node` against the oracle at the suite's bar and against `wave` at 1e-13 (K1, stored
state) and 1e-12 (K3); two runs bit for bit; assign and accumulate mode; two node ranges against one call.  The device
twin of test_emul_node_rows_chain.py."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from node_rows_chain_cases import (MESHES, adjoint, check_against_oracle, check_against_wave, check_assign_and_accumulate, forward,
                                   mesh, same_bits, steps)

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
def test_assign_then_accumulate(name):
    be = _backend(name, "node")
    check_assign_and_accumulate(name, be, be.asm.set_assign_mode)


@pytest.mark.parametrize("name", MESHES)
def test_two_node_ranges_equal_one_call(name):
    import torch
    asm = _backend(name, "node").asm
    u1, p1, xi1, u2, p2 = (asm.dev(a) for a in steps(name))  # xi1 is kept: gather_finish reads the previous state again
    ref, xi_ref = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(u2, p2, u1, p1, xi1, xi_ref, ref) == 0
    nn = asm.nnodes
    asm.set_gather_early_nodes(nn // 3, max(nn // 2, nn // 3 + 1))
    try:
        ls, xi = asm.new_linsys(), asm.new_state()
        assert asm.forward_jacobian(u2, p2, u1, p1, xi1, xi, ls) == 0
        assert not torch.equal(ls.flat, ref.flat)
        assert asm.gather_finish() == 0
    finally:
        asm.set_gather_early_nodes(0, 0)
    assert torch.equal(ls.flat, ref.flat) and torch.equal(xi, xi_ref)
