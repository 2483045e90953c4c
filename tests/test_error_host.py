"""The per-point error contributions of c8_eval_error_contributions (calibr8_amd/csrc/c8_error.hpp: error_point) on the
CPU: the function the device kernel compiles, built here with g++ (tests/error_host) and checked against the oracle on its
second load step of every row of the model table (cauchy_cases.ROWS: plastic and elastic points both present), with random
z and phi."""
import numpy as np
import pytest

import cauchy_cases as cc
import error_cases as ec
import oracle_lib as ol
import parity_cases as pc


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    """the harness, built afresh for this session into its own temporary directory"""
    return ec.build_harness(tmp_path_factory.mktemp("c8_error_host"))


def one_element_oracle(cs, e, **kw):
    """an oracle context on the one-element mesh of element e: its nodes, the case's parameters (kw: oracle settings)"""
    nodes = cs.conn[e]
    c1, conn1 = np.ascontiguousarray(cs.c[nodes]), np.arange(len(nodes), dtype=np.int32).reshape(1, -1)
    if cs.model == cc.HYBRID:
        import hybrid_cases as hc
        return hc.hybrid_oracle((cs.et, c1, conn1), hc.NETS[cc.HYBRID_NET], **kw)[0]
    return ol.Oracle(cs.et, c1, conn1, cs.model, cs.params, **kw)


def check_E_R_against_element_residuals(harness, rid, stab_mult=1.0):
    """E_R[e] = z_e . b_e with b_e the oracle's global residual on the one-element mesh of e, to 1e-12 of sum |z_i b_i|;
    returns E_R"""
    cs = cc.case(rid)
    plastic, elastic = cs.branches()
    if cs.model not in cc.NO_PLASTICITY:
        assert plastic > 0 and elastic > 0, (rid, plastic, elastic)
    z_u, z_p, phi = ec.adjoints(cs)
    E_R, _ = ec.host_error(harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *cs.state, z_u, z_p, phi, nn=cs.nn, stab_mult=stab_mult)
    nd = cs.orc.ndims
    worst = 0.0
    for e, nodes in enumerate(cs.conn):
        orc = one_element_oracle(cs, e, stab_mult=stab_mult)
        loc = lambda a, w: np.ascontiguousarray(np.asarray(a).reshape(-1, w)[nodes].ravel())
        ls = orc.new_linsys()
        orc.global_residual(loc(cs.u, nd), loc(cs.p, 1), loc(cs.u_prev, nd), loc(cs.p_prev, 1), np.ascontiguousarray(cs.xi_prev[e:e + 1]),
                            np.ascontiguousarray(cs.xi[e:e + 1]), ls)
        terms = [loc(z_u, nd) * ls.b[0]] + ([loc(z_p, 1) * ls.b[1]] if orc.nres == 2 else [])
        ref, scale = sum(t.sum() for t in terms), sum(np.abs(t).sum() for t in terms)
        assert scale > 0 and abs(E_R[e] - ref) < 1e-12 * scale, (rid, e, E_R[e], ref, scale)
        worst = max(worst, abs(E_R[e] - ref) / scale)
    print("%s: worst |E_R - z.b| / sum|z_i b_i| = %.2e over %d elements" % (rid, worst, len(cs.conn)))
    return E_R


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_E_R_is_z_dot_the_oracles_element_residual(harness, rid):
    """E_R[e] = z_e . b_e with b_e the oracle's global residual on the one-element mesh of e, to 1e-12 of sum |z_i b_i|"""
    check_E_R_against_element_residuals(harness, rid)


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-tet4", "hyper_J2_plane_strain-tri3"])
def test_E_R_follows_the_stabilization_multiplier(harness, rid):
    """the same with stab_mult = 3.7 in the harness and in the oracle (settings_cases.STAB); E_R moves with the multiplier by
    more than 1e-5 of its largest entry, seven orders above the bar (the stabilisation term is one of many in z . R)"""
    E_R = check_E_R_against_element_residuals(harness, rid, stab_mult=3.7)
    cs = cc.case(rid)
    one, _ = ec.case_host(harness, cs, *ec.adjoints(cs))
    assert np.abs(E_R - one).max() > 1e-5 * np.abs(one).max()


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_E_C_vanishes_at_the_converged_state(harness, rid):
    """xi of the case is the oracle's c8o_forward_jacobian state.  Its local Newton iteration stops at |C|_2 < abs_tol (or at
    |C|_2 < rel_tol |C_0|_2, the smaller bound at these states: |C_0| is a strain increment, far below 1), so every equation
    of every point has |C_j| <= abs_tol and |E_C[e]| <= sum_pt sum_j |phi_j| abs_tol, abs_tol the oracle context's own"""
    cs = cc.case(rid)
    z_u, z_p, phi = ec.adjoints(cs)
    _, E_C = ec.case_host(harness, cs, z_u, z_p, phi)
    tol = getattr(cs.orc, "local_abs_tol", ec.ABS_TOL)
    bound = np.abs(phi).sum(axis=(1, 2)) * tol
    assert np.all(np.abs(E_C) <= bound), (rid, np.abs(E_C).max(), bound.min())
    if cs.model == "elastic":
        assert not E_C.any()
    # away from the converged state the same sum is not small: the check above is not vacuous
    if cs.model not in cc.NO_PLASTICITY:
        _, off = ec.case_host(harness, cs, z_u, z_p, phi, xi=ec.mid_state(cs))
        assert np.abs(off).max() > 1e6 * bound.max()


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_E_C_parameter_derivative_is_the_oracles_gradient(harness, rid):
    """d(sum_e E_C)/dp_k by central differences (h = 1e-5 |p_k|) against c8o_qoi_gradient with z = 0 under the average-
    displacement objective (dJ/dp = 0: the gradient is sum (dC/dp_k)^T phi), for every active parameter.  1e-7 of the scale
    of c8o_qoi_gradient_abs: truncation O(h^2) ~ 1e-10 and rounding eps / h ~ 1e-11 of that scale leave two orders of margin.

    The state.  The models divide their yield equation by val(mu), the VALUE of the shear modulus (c8_models.hpp, head):
    the reference's derivative leaves d(1/mu)/dp out on purpose, a difference quotient cannot, and the two differ by
    phi_f f dln(mu)/dp.  They agree where f = 0: at the converged state, whose plastic points have f = 0 to rounding.  There
    the branch test (f > tol or |f| < tol) must not flip under the perturbation, which moves f by at most 1e-5 |df/dln p| ~
    1e-5 x 1e-2: both sides therefore evaluate with the band tol = 1e-6, an oracle context of its own with that abs_tol
    (it solves nothing here) and the harness with the same setting; the converged elastic points have C = 0 identically.
    A state away from the surface (error_cases.mid_state) is smooth too but measures the val(mu) term: 1.6e-2 of the scale
    for small_J2 and p = E."""
    cs = cc.case(rid)
    _, _, phi = ec.adjoints(cs)
    z_u, z_p = np.zeros_like(cs.u), np.zeros_like(cs.p)
    act = ec.active_params(cs)
    band = 1e-6
    if cs.model == cc.HYBRID:
        import hybrid_cases as hc
        orc = hc.hybrid_oracle((cs.et, cs.c, cs.conn), hc.NETS[cc.HYBRID_NET], abs_tol=band, rel_tol=band)[0]
    else:
        orc = ol.Oracle(cs.et, cs.c, cs.conn, cs.model, cs.params, abs_tol=band, rel_tol=band)
    orc.set_active(0, act)
    st = list(cs.state)
    grad, gabs = orc.qoi_gradient_with_scale(*st, z_u, z_p, phi, len(act))
    if cs.model != "elastic":
        assert np.abs(grad).max() > 0
    for i, k in enumerate(act):
        h = 1e-5 * abs(cs.params[k])
        assert h > 0
        vals = []
        for s in (1.0, -1.0):
            prm = np.array(cs.params, dtype=np.float64)
            prm[k] += s * h
            vals.append(ec.host_error(harness, cs.et, cs.c, cs.conn, cs.model, prm, *st, z_u, z_p, phi, nn=cs.nn, abs_tol=band)[1].sum())
        fd = (vals[0] - vals[1]) / (2.0 * h)
        print("%s p[%d]: fd %.6e oracle %.6e scale %.3e ratio %.2e" % (rid, k, fd, grad[i], gabs[i], abs(fd - grad[i]) / max(gabs[i], 1e-300)))
        assert abs(fd - grad[i]) <= 1e-7 * gabs[i], (rid, k, fd, grad[i], gabs[i])


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_E_C_state_derivative_is_the_oracles_local_adjoint_system(harness, rid):
    """With z = 0, c8o_solve_adjoint_local returns the phi that solves the local adjoint system for the given g alone,
    (dC/dxi)^T phi = g, so for a direction v in xi the central difference of sum_e E_C(phi) along v is phi . (dC/dxi) v =
    g . v (the sign is that of the oracle's output: phi = +(dC/dxi)^-T g).  Step 1e-5 of v, tolerance 1e-7 of
    sum |g_j v_j|.  No parameter moves here, so the state may lie away from the yield surface: error_cases.smooth_state
    (per row), where h v moves no point across the branch test."""
    cs = cc.case(rid)
    rng = np.random.default_rng(9)
    xi = ec.smooth_state(rid, cs)
    g = rng.standard_normal(xi.shape)
    # v: random, each local unknown on the scale of its own increment over the step (the unknowns of the finite-deformation
    # models differ by three orders of magnitude: zeta ~ 1, alpha ~ 1e-3), so that h v is 1e-5 of that increment everywhere
    inc = np.abs(cs.xi - cs.xi_prev).max(axis=(0, 1))
    v = rng.standard_normal(xi.shape) * np.where(inc > 0, inc, inc.max())
    z_u, z_p = np.zeros_like(cs.u), np.zeros_like(cs.p)
    st = list(cs.state)
    st[5] = xi
    phi, g_io = np.zeros_like(xi), g.copy()
    cs.orc.solve_adjoint_local(*st, z_u, z_p, phi, g_io, np.zeros((len(cs.conn), cs.orc.npts, cs.orc.ndofs)))
    if cs.model == "elastic":  # no local equations: phi = 0 and E_C = 0 whatever g
        assert not phi.any() and not ec.case_host(harness, cs, z_u, z_p, rng.standard_normal(xi.shape), xi=xi)[1].any()
        return
    h = 1e-5
    up = ec.case_host(harness, cs, z_u, z_p, phi, xi=xi + h * v)[1].sum()
    dn = ec.case_host(harness, cs, z_u, z_p, phi, xi=xi - h * v)[1].sum()
    fd, ref, scale = (up - dn) / (2.0 * h), (g * v).sum(), np.abs(g * v).sum()
    print("%s: fd %.6e g.v %.6e scale %.3e ratio %.2e" % (rid, fd, ref, scale, abs(fd - ref) / scale))
    assert abs(fd - ref) <= 1e-7 * scale, (rid, fd, ref, scale)


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-tet4", "hyper_J2_plane_stress-tri3"])
def test_a_second_call_doubles_both_fields_exactly(harness, rid):
    cs = cc.case(rid)
    z_u, z_p, phi = ec.adjoints(cs)
    xi = ec.mid_state(cs)
    one = ec.case_host(harness, cs, z_u, z_p, phi, xi=xi)
    two = ec.case_host(harness, cs, z_u, z_p, phi, xi=xi, out=(one[0].copy(), one[1].copy()))
    assert np.abs(one[0]).min() > 0 and np.abs(one[1]).max() > 0
    assert np.array_equal(two[0], 2.0 * one[0]) and np.array_equal(two[1], 2.0 * one[1])


@pytest.mark.parametrize("kind", ["hex8", "tet4"])
def test_two_element_sets_give_the_per_set_values(harness, kind):
    """every element of a set has the values a one-set run with that set's parameters gives it, and the sets differ"""
    et, c, conn = pc.mesh_of(kind)
    es = (np.random.default_rng(21).random(len(conn)) < 0.4).astype(np.int32)
    assert 0 < es.sum() < len(es)
    params = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]
    npts = len(ol.kit_points(et, 0)[0])
    state = cc.synthetic_state(np.zeros((len(conn), npts, 7)), c, 3, 2, seed=4)
    rng = np.random.default_rng(6)
    adj = rng.standard_normal(3 * len(c)), rng.standard_normal(len(c)), rng.standard_normal((len(conn), npts, 7))
    both = ec.host_error(harness, et, c, conn, "small_J2", params, *state, *adj, elem_set=es)
    for s in (0, 1):
        one = ec.host_error(harness, et, c, conn, "small_J2", params[s], *state, *adj)
        for k in (0, 1):
            assert np.array_equal(both[k][es == s], one[k][es == s])
            assert np.abs(both[k][es != s] - one[k][es != s]).min() > 0


def test_model_form_error_replay_converges_at_second_order(harness):
    """The end-to-end case of test_gpu_error.py replayed on the CPU (tests/fe_driver.py over the oracle, the host harness
    for the element loop), which is how its delta was chosen: eta against dJ = J(fine primal run) - J(base) at delta and
    delta / 2.  Both are exact to first order in delta (Taylor), so |eta - dJ| falls by 4 up to the cubic term: band
    [2.5, 6.5]; the deviation of eta / (delta K) from dJ/dK of the base run's adjoint gradient halves: band [1.5, 3].  With
    the fine model equal to the base model eta is z . R of a converged run: |eta| <= |z|_2 |R|_2 + sum |phi| tol."""
    import fe_driver as fe
    c, conn, spec = ec.mfe_case()
    base = ec.replay_primal(c, conn, spec, pc.J2)
    assert all((x[:, :, 6] > 0).mean() > 0.5 for x in base.xi[1:])  # every step yields
    J0 = base.qoi()
    base.be.set_active(0, [2])
    dJdK = fe.adjoint_gradient(base, 1)[0]
    gap, dev = [], []
    for d in (ec.MFE_DELTA, 0.5 * ec.MFE_DELTA):
        prm = ec.mfe_params(d)
        dJ = ec.replay_primal(c, conn, spec, prm).qoi() - J0
        eta, bound = ec.replay_eta(harness, base, prm)
        assert abs(eta) <= bound
        gap.append(abs(eta - dJ))
        dev.append(abs(eta / (d * pc.J2[2]) - dJdK))
        print("delta %g: dJ %.6e eta %.6e |eta - dJ| / |dJ| %.3e  |eta / (delta K) - dJ/dK| %.3e" % (d, dJ, eta, gap[-1] / abs(dJ), dev[-1]))
    print("factors: %.3f (a), %.3f (b)" % (gap[0] / gap[1], dev[0] / dev[1]))
    assert 2.5 <= gap[0] / gap[1] <= 6.5 and 1.5 <= dev[0] / dev[1] <= 3.0
    eta, bound = ec.replay_eta(harness, base, pc.J2)
    assert abs(eta) <= bound and abs(eta) < 1e-9 * abs(J0)
