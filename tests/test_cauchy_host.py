"""The per-point stress evaluation of c8_eval_cauchy (calibr8_amd/csrc/c8_cauchy.hpp: cauchy_point) on the CPU: the function
the device kernel compiles, built here with g++ (tests/cauchy_host) and checked on the oracle's converged states against the
oracle's global residual -- the stress field integrated against grad N is the momentum residual -- and against closed forms."""
import numpy as np
import pytest

import cauchy_cases as cc
import oracle_lib as ol
import parity_cases as pc


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    """the harness, built afresh for this session into its own temporary directory"""
    return cc.build_harness(tmp_path_factory.mktemp("c8_cauchy_host"))


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_stress_field_integrates_to_the_oracles_momentum_residual(harness, rid):
    """R_u[n, i] = sum_e sum_pt sum_j P_ij dN_n/dx_j w dv with quadrature and grad N from the oracle's kit, P = sigma, sigma
    cof(I + grad u) or t lambda_z J sigma F^-T (c8_models.hpp: Mechanics, MechanicsPlaneStress), against b[0] of the oracle's
    global residual at the same state.  Bar: 1e-12 of the largest per-entry sum of the absolute values of the terms (both
    sides are fp64 sums of at most a few hundred such terms; near equilibrium R itself is small, so |R| is no scale)."""
    cs = cc.case(rid)
    plastic, elastic = cs.branches()
    if cs.model not in cc.NO_PLASTICITY:
        assert plastic > 0 and elastic > 0, (rid, plastic, elastic)
    sigma = cs.host(harness)
    assert np.isfinite(sigma).all() and np.abs(sigma).max() > 0
    nd = cs.orc.ndims
    R, scale = cc.weak_form(sigma, cs, nd)
    ls = cs.orc.new_linsys()
    cs.orc.global_residual(*cs.state, ls)
    ref = ls.b[0].reshape(-1, nd)
    err = np.abs(R - ref).max()
    print("%s: |R - R_oracle| %.3e, scale %.3e, ratio %.3e, max |R| %.3e" % (rid, err, scale, err / scale, np.abs(ref).max()))
    assert err < 1e-12 * scale, (rid, err, scale)


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_entries_outside_the_ndims_block_are_exactly_zero(harness, rid):
    cs = cc.case(rid)
    sigma = cs.host(harness)
    nd = cs.orc.ndims
    assert sigma.shape == (len(cs.conn), cs.orc.npts, 3, 3)
    if nd == 2:
        assert np.all(sigma[:, :, 2, :] == 0.0) and np.all(sigma[:, :, :, 2] == 0.0)
        assert np.abs(sigma[:, :, 1, 1]).max() > 0
    else:
        assert np.abs(sigma[:, :, 2, 2]).max() > 0


@pytest.mark.parametrize("rid", ["small_J2-hex8", "small_J2-tet4", "small_J2-tri3"])
def test_small_J2_closed_form(harness, rid):
    """sigma = 2 mu (dev eps - eps_p) - p I with eps from this test's own grad N (the oracle's kit) and eps_p from xi in the
    packing (00, 01, 02, 11, 12, 22), in 2-D (00, 01, 11) with dev eps = eps - tr(eps)/3 I(2) (small_J2.cpp:266-277); 1e-12
    of max |sigma|"""
    cs = cc.case(rid)
    nd = cs.orc.ndims
    sigma = cs.host(harness)
    dN, N, _ = cc.point_tables(cs.et, cs.c, cs.conn)
    ue = cs.u.reshape(-1, nd)[cs.conn]
    grad_u = np.einsum("eni,epnj->epij", ue, dN[..., :nd])
    eps = 0.5 * (grad_u + np.swapaxes(grad_u, -1, -2))
    p = np.einsum("en,epn->ep", cs.p[cs.conn], N)
    mu = cs.params[0] / (2.0 * (1.0 + cs.params[1]))
    eye = np.eye(nd)
    ep = np.zeros_like(eps)
    pack = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)) if nd == 3 else ((0, 0), (0, 1), (1, 1))
    for k, (i, j) in enumerate(pack):
        ep[..., i, j] = ep[..., j, i] = cs.xi[:, :, k]
    assert np.abs(ep).max() > 0
    ref = 2.0 * mu * (eps - np.trace(eps, axis1=-2, axis2=-1)[..., None, None] / 3.0 * eye - ep) - p[..., None, None] * eye
    err = np.abs(sigma[..., :nd, :nd] - ref).max()
    assert err < 1e-12 * np.abs(ref).max(), (err, np.abs(ref).max())


@pytest.mark.parametrize("kind", ["hex8", "tet4"])
def test_two_element_sets_give_different_stresses_for_equal_strains(harness, kind):
    """the mesh and the parameter sets of parity_cases.check_two_element_sets under a homogeneous strain from the virgin
    state: every point of a set has that set's 2 mu dev(eps), and the two sets differ"""
    et, c, conn = pc.mesh_of(kind)
    es = (np.random.default_rng(21).random(len(conn)) < 0.4).astype(np.int32)
    assert 0 < es.sum() < len(es)
    params = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]
    G = 1e-3 * pc.G0
    u = np.ascontiguousarray((c @ G.T).ravel())
    z, zp = np.zeros_like(u), np.zeros(len(c))
    npts = len(ol.kit_points(et, 0)[0])
    xi = np.zeros((len(conn), npts, 7))
    sigma = cc.host_cauchy(harness, et, c, conn, "small_J2", params, u, zp, z, zp, xi, xi, elem_set=es)
    sym = 0.5 * (G + G.T)
    dev = sym - np.trace(sym) / 3.0 * np.eye(3)
    refs = [2.0 * (prm[0] / (2.0 * (1.0 + prm[1]))) * dev for prm in params]
    assert np.abs(refs[0] - refs[1]).max() > 0.1 * np.abs(refs[0]).max()
    for s in (0, 1):
        assert np.abs(sigma[es == s] - refs[s]).max() < 1e-12 * np.abs(refs[s]).max(), s
