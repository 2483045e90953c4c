"""The per-point terms of c8_eval_exact_errors and c8_eval_linearization_errors (calibr8_amd/csrc/c8_exact.hpp) on the CPU:
the function the device kernel compiles, built here with g++ (tests/exact_host) and checked against the oracle and against
the harness of c8_eval_error_contributions (tests/error_host), on every row of the model table (cauchy_cases.ROWS).

Signs, pinned here: with d = st_fine - st,
    E_R = -z . (dR/dx dx + dR/dxi dxi),   E_C = -phi . (dC/dx dx + dC/dxi dxi + dC/dx_prev dx_prev + dC/dxi_prev dxi_prev),
    E_lin = E_exact - (error contributions),
and the oracle's local adjoint solve returns phi with (dC/dxi)^T phi = g - (dR/dxi)^T z, g_out = -(dC/dxi_prev)^T phi and
f_out = -(dC/dx_prev)^T phi."""
import numpy as np
import pytest

import cauchy_cases as cc
import error_cases as ec
import exact_cases as xc
import oracle_lib as ol
import parity_cases as pc

TOL = 1e-12


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return xc.build_harness(tmp_path_factory.mktemp("c8_exact_host"))


@pytest.fixture(scope="session")
def err_harness(tmp_path_factory):
    return ec.build_harness(tmp_path_factory.mktemp("c8_error_host_x"))


def local_adjoint(cs, st, z_u, z_p, g):
    """(phi, g_out, f_out) of the oracle's c8o_solve_adjoint_local at the state st"""
    phi, g_io = np.zeros_like(cs.xi), np.array(g)
    f = np.zeros((len(cs.conn), cs.orc.npts, cs.orc.ndofs))
    cs.orc.solve_adjoint_local(*st, z_u, z_p, phi, g_io, f)
    return phi, g_io, f


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_a_direction_in_xi_gives_minus_g_dot_v(harness, rid):
    """(a) at the oracle's converged state, phi from c8o_solve_adjoint_local for random z and g: (dC/dxi)^T phi =
    g - (dR/dxi)^T z, so along dxi = v alone  sum_e (E_R + E_C) = -(z . dR/dxi v + phi . dC/dxi v) = -g . v.  AD against AD:
    1e-12 of sum |g_j v_j| plus the harness's summed magnitudes."""
    cs = cc.case(rid)
    z_u, z_p, _ = ec.adjoints(cs)
    g = np.random.default_rng(11).standard_normal(cs.xi.shape)
    st = list(cs.state)
    phi, _, _ = local_adjoint(cs, st, z_u, z_p, g)
    d = xc.direction(cs, 12, x=False, x_prev=False, xi_prev=False)
    E_R, E_C, aR, aC = xc.case_exact(harness, cs, st, xc.moved(st, d), (z_u, z_p, phi), scales=True)
    v = d[5]
    if cs.model == "elastic":  # no local equations: nothing depends on xi
        assert not phi.any() and not E_R.any() and not E_C.any()
        return
    got, ref, scale = (E_R + E_C).sum(), -(g * v).sum(), np.abs(g * v).sum() + aR.sum() + aC.sum()
    print("%s: sum %.6e -g.v %.6e scale %.3e ratio %.2e" % (rid, got, ref, scale, abs(got - ref) / scale))
    assert np.abs(g * v).sum() > 0 and abs(got - ref) <= TOL * scale, (rid, got, ref, scale)


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_b_previous_step_directions_give_the_history_vectors(harness, rid):
    """(b) along dxi_prev = v alone  sum E_C = g_out . v  (g_out = -(dC/dxi_prev)^T phi, the history vector the oracle
    returns) and along dx_prev = w alone  sum E_C = sum_pt f_out . w_e  (f_out = -(dC/dx_prev)^T phi): non-zero for the
    finite-deformation rows, exactly 0 for the others.  E_R is exactly 0 in both (R is not differentiated along the
    previous step)."""
    cs = cc.case(rid)
    z_u, z_p, _ = ec.adjoints(cs)
    g = np.random.default_rng(13).standard_normal(cs.xi.shape)
    st = list(cs.state)
    phi, g_out, f_out = local_adjoint(cs, st, z_u, z_p, g)
    adj = (z_u, z_p, phi)
    d = xc.direction(cs, 14, x=False, xi=False, x_prev=False)
    E_R, E_C, aR, aC = xc.case_exact(harness, cs, st, xc.moved(st, d), adj, scales=True)
    assert not E_R.any(), rid
    if cs.model in cc.NO_PLASTICITY:  # no local equations, or none that read the previous state
        assert not E_C.any() and not g_out.any()
    else:
        ref, scale = (g_out * d[4]).sum(), np.abs(g_out * d[4]).sum() + aC.sum()
        print("%s xi_prev: sum E_C %.6e g_out.v %.6e ratio %.2e" % (rid, E_C.sum(), ref, abs(E_C.sum() - ref) / scale))
        assert np.abs(g_out * d[4]).sum() > 0 and abs(E_C.sum() - ref) <= TOL * scale, (rid, E_C.sum(), ref, scale)
    d = xc.direction(cs, 15, x=False, xi=False, xi_prev=False)
    E_R, E_C, aR, aC = xc.case_exact(harness, cs, st, xc.moved(st, d), adj, scales=True)
    assert not E_R.any(), rid
    if not cs.finite:
        assert not E_C.any() and not f_out.any(), rid
        return
    nd = cs.orc.ndims
    w_e = np.asarray(d[2]).reshape(-1, nd)[cs.conn].reshape(len(cs.conn), -1)  # the u slots of the element DOFs: node-major
    terms = f_out[:, :, :w_e.shape[1]] * w_e[:, None, :]
    ref, scale = terms.sum(), np.abs(terms).sum() + aC.sum()
    print("%s x_prev: sum E_C %.6e f_out.w %.6e ratio %.2e" % (rid, E_C.sum(), ref, abs(E_C.sum() - ref) / scale))
    assert abs(ref) > 0 and abs(E_C.sum()) > 0, rid
    assert abs(E_C.sum() - ref) <= TOL * scale, (rid, E_C.sum(), ref, scale)


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_c_direction_in_x_gives_the_forward_jacobian(harness, rid):
    """(c) along dx = w alone, with phi from the local adjoint solve with g = 0 ((dC/dxi)^T phi = -(dR/dxi)^T z):
    -sum_e (E_R + E_C) = z . (dR/dx - dR/dxi (dC/dxi)^-1 dC/dx) w = z . A w, A the four blocks of c8o_forward_jacobian.  The
    state is the one that call leaves in xi (its local solve from xi_prev; the linearisation point of A)."""
    import fe_driver as fe
    cs = cc.case(rid)
    z_u, z_p, _ = ec.adjoints(cs)
    st = list(cs.state)
    st[5] = np.array(cs.xi)
    ls = cs.orc.new_linsys()
    cs.orc.forward_jacobian(*st, ls)
    phi, _, _ = local_adjoint(cs, st, z_u, z_p, np.zeros_like(cs.xi))
    d = xc.direction(cs, 16, xi=False, x_prev=False, xi_prev=False)
    E_R, E_C, aR, aC = xc.case_exact(harness, cs, st, xc.moved(st, d), (z_u, z_p, phi), scales=True)
    A = fe.block_matrix(cs.orc, ls)
    two = cs.orc.nres == 2
    z = np.concatenate([z_u, z_p]) if two else z_u
    w = np.concatenate([d[0], d[1]]) if two else d[0]
    ref, scale = z @ (A @ w), np.abs(z) @ (abs(A) @ np.abs(w)) + aR.sum() + aC.sum()
    got = -(E_R + E_C).sum()
    print("%s: -sum %.6e z.A.w %.6e scale %.3e ratio %.2e" % (rid, got, ref, scale, abs(got - ref) / scale))
    assert abs(ref) > 0 and abs(got - ref) <= TOL * scale, (rid, got, ref, scale)


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_d_each_field_is_the_state_derivative_of_the_error_contributions(harness, err_harness, rid):
    """(d) E_R and E_C each on its own, at error_cases.smooth_state s:  E(exact) = -[E(s + h D) - E(s - h D)] / 2h with E(.)
    from the harness of c8_eval_error_contributions; D moves x and xi for E_R and all four parts for E_C.  h = 1e-5 of a
    direction of the size of the step's own increments, 1e-7 of the summed magnitudes of the terms (truncation O(h^2) and
    rounding eps / h leave two orders, as in test_E_C_state_derivative_is_the_oracles_local_adjoint_system).  Along a
    direction that moves only x_prev and xi_prev, E_R is exactly 0: the single pass seeded in all four directions
    differentiates R along x and xi only, because no model's global flux reads the previous step."""
    cs = cc.case(rid)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    h = 1e-5
    contrib = lambda s: ec.host_error(err_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *s, *adj, nn=cs.nn)
    for k, name, parts in ((0, "E_R", dict(x_prev=False, xi_prev=False)), (1, "E_C", {})):
        d = xc.direction(cs, 17 + k, **parts)
        ex = xc.case_exact(harness, cs, st, xc.moved(st, d), adj, scales=True)
        up, dn = contrib(xc.moved(st, d, h))[k], contrib(xc.moved(st, d, -h))[k]
        fd = -(up - dn).sum() / (2.0 * h)
        got, scale = ex[k].sum(), ex[2 + k].sum()
        if k == 1 and cs.model == "elastic":
            assert not ex[1].any() and fd == 0.0
            continue
        print("%s %s: exact %.6e fd %.6e scale %.3e ratio %.2e" % (rid, name, got, fd, scale, abs(got - fd) / scale))
        assert scale > 0 and abs(got) > 0 and abs(got - fd) <= 1e-7 * scale, (rid, name, got, fd, scale)
    d = xc.direction(cs, 19, x=False, xi=False)
    ex = xc.case_exact(harness, cs, st, xc.moved(st, d), adj)
    assert not ex[0].any(), rid
    if cs.model not in cc.NO_PLASTICITY:  # the local equations of the others do not read the previous step
        assert ex[1].any(), rid


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_e_linearization_is_exact_minus_contributions(harness, err_harness, rid):
    """(e) the linearization fields equal the exact fields minus the fields of the harness of
    c8_eval_error_contributions, to 1e-12 of the summed magnitudes; with st_fine = st the exact fields are exactly 0 and the
    linearization fields are bitwise the negated contributions."""
    cs = cc.case(rid)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    fine = xc.moved(st, xc.direction(cs, 20))
    ex = xc.case_exact(harness, cs, st, fine, adj)
    lin = xc.case_exact(harness, cs, st, fine, adj, lin=True, scales=True)
    con = ec.host_error(err_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *st, *adj, nn=cs.nn)
    for k in (0, 1):
        assert np.all(np.abs(lin[k] - (ex[k] - con[k])) <= TOL * lin[2 + k]), (rid, k)
    assert np.abs(ex[0]).min() > 0 and np.abs(con[0]).min() > 0
    same = [np.array(a) for a in st]
    ex0 = xc.case_exact(harness, cs, st, same, adj)
    lin0 = xc.case_exact(harness, cs, st, same, adj, lin=True)
    assert not ex0[0].any() and not ex0[1].any()
    assert np.array_equal(lin0[0], -con[0]) and np.array_equal(lin0[1], -con[1])


@pytest.mark.parametrize("rid", [r for r in cc.ROW_IDS if r.split("-")[0] in cc.NO_PLASTICITY])
def test_f_linear_models_have_no_linearization_error(harness, err_harness, rid):
    """(f) elastic and isotropic_elastic are linear in the state: R(s) + R'(s) d = R(s + d), so the linearization fields are
    the negated contributions evaluated AT the fine state, to 1e-12 of the summed magnitudes"""
    cs = cc.case(rid)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    fine = xc.moved(st, xc.direction(cs, 21))
    lin = xc.case_exact(harness, cs, st, fine, adj, lin=True, scales=True)
    con = ec.host_error(err_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *fine, *adj, nn=cs.nn, scales=True)
    for k in (0, 1):
        assert np.all(np.abs(lin[k] + con[k]) <= TOL * (lin[2 + k] + con[2 + k])), (rid, k)
    assert np.abs(lin[0]).min() > 0


# of a direction of the size of the step's increments (exact_cases.direction).  Chosen on the CPU so that no point changes
# branch: the L1 norm of the remainder over t^2 is constant (1.301, 1.758e-2, 0.4077 for the three rows) for every t from
# 2.5e-4 down to 5e-5; above it one element of hyper_J2-tet4 flips (t >= 5e-4: remainder 2.4e-3, not falling), and of
# hyper_J2_plane_stress-tri3 at t >= 1e-2.  At 1e-4 the remainder is 1e-9 to 1e-11 of the summed magnitudes: five orders
# above rounding.
REMAINDER_T = 1e-4


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-tet4", "hyper_J2_plane_stress-tri3"])
def test_f_plastic_models_have_a_quadratic_remainder(harness, err_harness, rid):
    """(f) a small-strain, a finite-deformation and a plane-stress plastic row: the remainder field
    E_lin(s, s + t D) + contributions(s + t D) = z . (R(s + t D) - R(s) - t R' D) + phi . (the same of C), per element, E_R and
    E_C together (the global residual of a small-strain model is linear in the state: its own remainder is rounding), is
    quadratic in t: its L1 norm falls by a factor in [2.5, 6.5] from t to t / 2 (4 in theory; the band the project uses for
    a quadratic remainder)."""
    cs = cc.case(rid)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    d = xc.direction(cs, 22)
    rem = []
    for t in (REMAINDER_T, 0.5 * REMAINDER_T):
        fine = xc.moved(st, d, t)
        lin = xc.case_exact(harness, cs, st, fine, adj, lin=True, scales=True)
        con = ec.host_error(err_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *fine, *adj, nn=cs.nn)
        rem.append(np.abs((lin[0] + con[0]) + (lin[1] + con[1])).sum())
        assert rem[-1] > 1e-13 * (lin[2] + lin[3]).sum()  # three orders above rounding
    print("%s: remainder factor %.3f; remainders %r" % (rid, rem[0] / rem[1], rem))
    assert 2.5 <= rem[0] / rem[1] <= 6.5, (rid, rem)


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-tet4", "hyper_J2_plane_stress-tri3"])
@pytest.mark.parametrize("lin", [False, True])
def test_g_a_second_call_doubles_both_fields_exactly(harness, rid, lin):
    cs = cc.case(rid)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    fine = xc.moved(st, xc.direction(cs, 23))
    one = xc.case_exact(harness, cs, st, fine, adj, lin=lin)
    two = xc.case_exact(harness, cs, st, fine, adj, lin=lin, out=(one[0].copy(), one[1].copy()))
    assert np.abs(one[0]).min() > 0 and np.abs(one[1]).max() > 0
    assert np.array_equal(two[0], 2.0 * one[0]) and np.array_equal(two[1], 2.0 * one[1])


@pytest.mark.parametrize("kind", ["hex8", "tet4"])
def test_g_two_element_sets_give_the_per_set_values(harness, kind):
    """every element of a set has the values a one-set run with that set's parameters gives it, and the sets differ"""
    et, c, conn = pc.mesh_of(kind)
    es = (np.random.default_rng(21).random(len(conn)) < 0.4).astype(np.int32)
    assert 0 < es.sum() < len(es)
    params = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]
    npts = len(ol.kit_points(et, 0)[0])
    state = cc.synthetic_state(np.zeros((len(conn), npts, 7)), c, 3, 2, seed=4)
    fine = cc.synthetic_state(np.zeros((len(conn), npts, 7)), c, 3, 2, seed=8)
    rng = np.random.default_rng(6)
    adj = rng.standard_normal(3 * len(c)), rng.standard_normal(len(c)), rng.standard_normal((len(conn), npts, 7))
    for lin in (False, True):
        both = xc.host_exact(harness, et, c, conn, "small_J2", params, state, fine, *adj, lin=lin, elem_set=es)
        for s in (0, 1):
            one = xc.host_exact(harness, et, c, conn, "small_J2", params[s], state, fine, *adj, lin=lin)
            for k in (0, 1):
                assert np.array_equal(both[k][es == s], one[k][es == s])
                assert np.abs(both[k][es != s] - one[k][es != s]).min() > 0


def test_g_model_form_error_verify_replay(harness, err_harness):
    """The end-to-end case of test_gpu_exact_errors.py replayed on the CPU (tests/fe_driver.py over the oracle, the two host
    harnesses for the element loops), which is how its delta was chosen.  For the linear objective (average displacement)
    E_exact = J_h - J_H = eta + E_lin_R + E_lin_C = E_computed: criterion of the reference's main_model_form_error_verify.cpp,
    |E_computed - E_exact| <= 1e-8 |E_exact| + allowance, allowance = steps (z_norm r + phi_norm c) with r = c = MFE_TOL the
    fine run's residual tolerances.  Both the linearization error and |eta - E_exact| exceed 1000 x that bound: the
    identity is not met by smallness.  The sum of the exact fields is E_exact as well (to the same bound)."""
    c, conn, spec = ec.mfe_case()
    base = ec.replay_primal(c, conn, spec, pc.J2)
    fine = ec.replay_primal(c, conn, spec, ec.mfe_params(xc.MFE_VERIFY_DELTA))
    r = xc.replay_verify(err_harness, harness, base, fine)
    bound = 1e-8 * abs(r["E_exact"]) + r["allowance"]
    gap, E_lin = abs(r["E_computed"] - r["E_exact"]), abs(r["E_lin_R"] + r["E_lin_C"])
    print("E_exact %.6e eta %.6e E_lin_R %.6e E_lin_C %.6e |E_computed - E_exact| %.3e allowance %.3e bound %.3e z_norm %.3e "
          "phi_norm %.3e |E_lin| / bound %.3e" % (r["E_exact"], r["eta"], r["E_lin_R"], r["E_lin_C"], gap, r["allowance"], bound,
                                                   r["z_norm"], r["phi_norm"], E_lin / bound))
    assert gap <= bound
    assert E_lin > 1000.0 * bound and abs(r["eta"] - r["E_exact"]) > 1000.0 * bound
    assert abs(sum(f.sum() for f in r["exact_fields"]) - r["E_exact"]) <= bound
