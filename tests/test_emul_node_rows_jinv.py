"""The row-per-node kernels take dN/dx from the cached inverse Jacobian (c8_assemble_node.hpp, phase A): the kernel source
run lane by lane on the CPU, on meshes whose Jacobians are neither diagonal nor symmetric nor constant
(node_rows_jinv_cases.py).  K1 and K3 against the oracle at the suite's bar, K1 against the emulated staged closed-form
wave kernel at 1e-13 of the largest entry (stored state: 1e-13 of its largest entry, the suite's bound for that pair), in
assign and in accumulate mode; and the table itself through an assembly of a field that is linear in x.
The CPU twin of test_gpu_node_rows_jinv.py."""
import functools

import numpy as np
import pytest

import emul_lib as em
import oracle_lib as ol
from node_rows_jinv_cases import (MESHES, adjoint, blocks, check_adjoint_against_oracle, check_forward_against_oracle, forward,
                                  linear_state, mesh, numpy_elastic_residual, oracle, rel_flat)
from parity import rel_vec

TOL = 1e-12  # test_emul_parity.py


def _emul(name, kernel):
    c, conn, es, prm = mesh(name)
    dut = em.Emul(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)
    if kernel == "node":
        dut.node = dut.wave = True
    else:  # the staged one-wavefront-per-element kernel in its closed form
        dut.wave = dut.staged = True
    return dut


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return oracle(name)


def _cases():
    return [(n, m) for n in MESHES for m in ([False, True] if n == "pinched_bricks" else [False])]


@pytest.mark.parametrize("name,force_many", _cases())
def test_forward_and_adjoint(name, force_many):
    em.lib().c8emu_set_node_many(1 if force_many else 0)
    try:
        orc, dut, wave = _oracle(name), _emul(name, "node"), _emul(name, "wave")
        ls, xi = forward(dut, name)                       # accumulate mode, into zeros
        check_forward_against_oracle(orc, ls, xi, name, TOL)
        ls_w, xi_w = forward(wave, name)
        print(name, "K1 node against wave: %.2e, state %.2e" % (rel_flat(ls, ls_w), rel_vec(xi, xi_w)))
        assert rel_flat(ls, ls_w) < 1e-13 and rel_vec(xi, xi_w) < 1e-13
        stale = dut.new_linsys()                          # assign mode, over stale content
        for a in blocks(stale):
            a[:] = -7.25e3
        dut.assign = True
        ls_a, xi_a = forward(dut, name, ls=stale)
        dut.assign = False
        check_forward_against_oracle(orc, ls_a, xi_a, name, TOL)
        assert np.array_equal(xi_a, xi)
        check_adjoint_against_oracle(orc, adjoint(dut, name, xi), name, xi, TOL)
    finally:
        em.lib().c8emu_set_node_many(0)


@pytest.mark.parametrize("name", ["sheared", "sheared_corner", "brick222"])
def test_table_through_a_linear_field(name):
    # u linear in x: grad u is the same matrix of nine distinct entries at every point whatever the element's shape, the
    # state stays elastic (stored xi: zero) and the residual follows from dN/dx alone
    orc, dut = _oracle(name), _emul(name, "node")
    st = linear_state(name)
    ls_o, xi_o = forward(orc, name, state=st)
    ls, xi = forward(dut, name, state=st)
    assert not xi.any() and not xi_o.any()
    b_u, b_p, worst = numpy_elastic_residual(name)
    assert worst < 1e-12 * 9e-5  # dN/dx rebuilt in numpy reproduces the gradient (largest entry 9e-5)
    errs = {"b_u": rel_vec(ls.b[0], ls_o.b[0]), "b_p": rel_vec(ls.b[1], ls_o.b[1]),
            "b_u numpy": rel_vec(ls.b[0], b_u), "b_p numpy": rel_vec(ls.b[1], b_p)}
    print(name, errs)
    assert max(errs.values()) < TOL, errs
