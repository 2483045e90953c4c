"""`-m gpu`: the row-per-node kernels take dN/dx from the cached inverse Jacobian (c8_assemble_node.hpp, phase A).  The
meshes of node_rows_jinv_cases.py -- Jacobians that are neither diagonal nor symmetric nor constant -- on the device:
`node` against `wave` at 1e-13 (K1) and 1e-12 (K3) of the largest entry and against the oracle at the suite's bar, `auto`
equal to `node` and two runs equal bit for bit, two parts equal to one call, and the table itself through an assembly of a
field that is linear in x.  The device twin of test_emul_node_rows_jinv.py."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from node_rows_jinv_cases import (MESHES, adjoint, check_adjoint_against_oracle, check_forward_against_oracle, forward, linear_state,
                                  mesh, numpy_elastic_residual, oracle, plastic_state, rel_flat)
from parity import rel_vec

pytestmark = pytest.mark.gpu
TOL = 1e-12  # test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def _backend(name, kernel):
    from gpu_backend import GpuBackend
    c, conn, es, prm = mesh(name)
    return GpuBackend(ol.HEX8, c, conn, "small_J2", prm, scatter="gather", kernel=kernel, elem_set=es)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return oracle(name)


@functools.lru_cache(maxsize=None)
def _forward(name, kernel):
    """the forward assembly of the plastic state: computed once, shared by the tests, left unchanged"""
    return forward(_backend(name, kernel), name)


@pytest.mark.parametrize("name", MESHES)
def test_forward(name):
    ls, xi = _forward(name, "node")
    check_forward_against_oracle(_oracle(name), ls, xi, name, TOL)
    ls_w, xi_w = _forward(name, "wave")
    print(name, "K1 node against wave: %.2e, state %.2e" % (rel_flat(ls, ls_w), rel_vec(xi, xi_w)))
    assert rel_flat(ls, ls_w) < 1e-13 and rel_vec(xi, xi_w) < 1e-13


@pytest.mark.parametrize("name", MESHES)
def test_adjoint(name):
    xi = _forward(name, "node")[1]
    ls = adjoint(_backend(name, "node"), name, xi)
    check_adjoint_against_oracle(_oracle(name), ls, name, xi, TOL)
    ls_w = adjoint(_backend(name, "wave"), name, xi)
    print(name, "K3 node against wave: %.2e" % rel_flat(ls, ls_w))
    assert rel_flat(ls, ls_w) < 1e-12


@pytest.mark.parametrize("name", MESHES)
def test_auto_is_node_and_runs_repeat(name):
    import torch
    u, p, z, zp = plastic_state(name)
    res = []
    for kernel in ("auto", "node", "node"):
        asm = _backend(name, kernel).asm
        ls, xi = asm.new_linsys(), asm.new_state()
        assert asm.forward_jacobian(asm.dev(u), asm.dev(p), asm.dev(z), asm.dev(zp), asm.new_state(), xi, ls) == 0
        res.append((ls.flat.clone(), xi.clone()))
    for flat, xi in res[1:]:
        assert torch.equal(flat, res[0][0]) and torch.equal(xi, res[0][1])


def test_two_parts_equal_one_call():
    import torch
    name = "brick222"
    asm = _backend(name, "node").asm
    u, p, z, zp = (asm.dev(a) for a in plastic_state(name))
    xi0 = asm.new_state()  # kept: gather_finish reads the previous state again
    ref, xi_ref = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(u, p, z, zp, xi0, xi_ref, ref) == 0
    nn = asm.nnodes
    asm.set_gather_early_nodes(nn // 3, nn // 2)
    try:
        ls, xi = asm.new_linsys(), asm.new_state()
        assert asm.forward_jacobian(u, p, z, zp, xi0, xi, ls) == 0
        assert not torch.equal(ls.flat, ref.flat)
        assert asm.gather_finish() == 0
    finally:
        asm.set_gather_early_nodes(0, 0)
    assert torch.equal(ls.flat, ref.flat) and torch.equal(xi, xi_ref)


@pytest.mark.parametrize("name", ["sheared", "brick222"])
def test_table_through_a_linear_field(name):
    # u linear in x: grad u is the same matrix of nine distinct entries at every point whatever the element's shape, the
    # state stays elastic (stored xi: zero) and the residual follows from dN/dx alone
    st = linear_state(name)
    ls_o, xi_o = forward(_oracle(name), name, state=st)
    ls, xi = forward(_backend(name, "node"), name, state=st)
    assert not xi.any() and not xi_o.any()
    b_u, b_p, worst = numpy_elastic_residual(name)
    assert worst < 1e-12 * 9e-5  # dN/dx rebuilt in numpy reproduces the gradient (largest entry 9e-5)
    errs = {"b_u": rel_vec(ls.b[0], ls_o.b[0]), "b_p": rel_vec(ls.b[1], ls_o.b[1]),
            "b_u numpy": rel_vec(ls.b[0], b_u), "b_p numpy": rel_vec(ls.b[1], b_p)}
    print(name, errs)
    assert max(errs.values()) < TOL, errs
