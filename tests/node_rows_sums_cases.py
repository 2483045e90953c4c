"""Cases shared by test_emul_node_rows_sums.py and test_gpu_node_rows_sums.py: phase B of the row-per-node kernels sums over
an element's points FIRST and combines afterwards (c8_models.hpp: closed_form_block_sums / closed_form_block_finish).  The
three "a" terms of the (u, u) block are a fixed combination of one matrix X_ki = sum_pt (a/2 w g_k) h_i:
    sum_pt w [ delta_ik a/2 (g.h) + a/2 g_k h_i - a/3 g_i h_k ] = X_ki - 2/3 X_ik + delta_ik tr X.
Two ways to break it hide on symmetric or uniform inputs: X taken for its transpose (invisible where g is parallel to h)
and a/2 pulled out of the sum (invisible where a is the same at an element's eight points).  So the meshes and the second
plastic step of node_rows_xlane_cases.py, with the assertion that the state differs among the eight points of every element,
and one elastic case (b = 0, a uniform) in which the X terms stand alone.
Both backends (emulated kernels, HIP library through GpuBackend) take and return numpy arrays."""
import functools

import numpy as np

from meshes import prescribed_fields
from node_rows_xlane_cases import (MESHES, NOT_PARALLELEPIPEDS, check_against_wave, face_defects, mesh, oracle,  # noqa: F401
                                   reference, steps)
from parity import compare_systems

ELASTIC_MESH = "brick222"  # jiggled: nodes with 1 / 2 / 4 / 8 elements


def assert_inputs_can_show_the_identity_broken():
    """xi[:, :, 6] (alpha) of the previous state and of the second step's state differs among the eight points of every
    element of every plastic case: with K > 0 theta, hence a = 2 mu theta, differs from point to point.  And the elements of
    the jiggled meshes are no parallelepipeds: g and h of two nodes are not parallel at every point."""
    for name in MESHES:
        for xi in (steps(name)[2], reference(name)[1]):
            alpha = xi[:, :, 6]
            assert alpha.shape[1] == 8 and (alpha > 0).all()
            assert all(len(np.unique(row)) == 8 for row in alpha), name
    for name in NOT_PARALLELEPIPEDS:
        assert (face_defects(name) > 1e-3).all(), name


@functools.lru_cache(maxsize=None)
def elastic_fields():
    """a quarter of the yield strain, perturbed by a tenth of it from node to node: elastic at every point"""
    return prescribed_fields(mesh(ELASTIC_MESH)[0], 0.0005, ramp=False, perturb=1e-1)


def elastic(be):
    """forward and adjoint assembly of a first step from the zero state: (forward system, state, adjoint system)"""
    u, p = elastic_fields()
    z, zp = np.zeros_like(u), np.zeros_like(p)
    ls, xi = be.new_linsys(), be.new_state()
    assert be.forward_jacobian(u, p, z, zp, be.new_state(), xi, ls) == 0
    rng = np.random.default_rng(11)
    g = 1e-3 * rng.standard_normal((be.nelems, be.npts, be.nloc))
    f = 1e-3 * rng.standard_normal((be.nelems, be.npts, 4 * be.nn))
    adj = be.new_linsys()
    assert be.adjoint_jacobian(u, p, z, zp, be.new_state(), xi, g, f, adj) in (0, None)
    return ls, xi, adj


@functools.lru_cache(maxsize=None)
def elastic_reference():
    ls, xi, adj = elastic(oracle(ELASTIC_MESH))
    assert not xi.any()  # no point yields: b = 0 and a = 2 mu at every point
    return ls, xi, adj


def check_elastic(ls, xi, adj, wave, tol):
    """against the oracle at tol and against the staged wave kernels at their bounds"""
    ls_o, xi_o, adj_o = elastic_reference()
    orc = oracle(ELASTIC_MESH)
    assert np.array_equal(xi, xi_o)
    for what, a, b in (("K1", ls, ls_o), ("K3", adj, adj_o)):
        errs = compare_systems(orc, a, b)
        print("elastic", what, "against the oracle:", errs)
        assert max(errs.values()) < tol, errs
    check_against_wave("elastic " + ELASTIC_MESH, ls, xi, adj, *wave)


def no_negative_zero(ls):
    """phase B starts its sums with the first point instead of adding to zero, so a zero sum may be -0; the rows are added to
    an image that starts at +0 and then to +0 (assign mode) or to the old value: no -0 reaches the matrix"""
    return not any((np.signbit(a) & (a == 0.0)).any() for a in (ls.A[i][j] for i in range(2) for j in range(2)))
