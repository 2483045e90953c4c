"""TEST INFRASTRUCTURE shared by test_exact_host.py and test_gpu_exact_errors.py: the host harness of the product's
per-point exact and linearization error terms (tests/exact_host/exact_host.cpp), second states and directions for its checks,
and the replay of model_form_error_verify on the CPU.  Rows, meshes and oracle states are those of cauchy_cases.py, the
adjoints and smooth states those of error_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import cauchy_cases as cc
import error_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))
dp, ip = cc.dp, cc.ip


def build_harness(out_dir):
    """compile the harness into out_dir and return its entry point"""
    so = os.path.join(str(out_dir), "libexacthost.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + cc.CXXFLAGS + ["-shared", "-o", so, os.path.join(HERE, "exact_host", "exact_host.cpp")])
    fn = C.CDLL(so).exact_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, dp, ip, dp, dp, dp] + [dp] * 12 + [dp] * 3 + [C.c_int] + [dp] * 4
    return fn


def host_exact(fn, et, coords, conn, model, params, state, fine, z_u, z_p, phi, lin=False, elem_set=None, nn=None, out=None,
               stab_mult=1.0, abs_tol=ec.ABS_TOL, thickness=1.0, scales=False):
    """(E_R, E_C) [nelems] of c8_eval_exact_errors (lin: of c8_eval_linearization_errors) from the host harness; state and
    fine are (u, p, u_prev, p_prev, xi_prev, xi); `out` = (E_R, E_C) is accumulated into.  scales: also the per-element sums
    of the magnitudes of the per-point terms, (E_R, E_C, abs_R, abs_C)"""
    d = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    coords, conn = d(coords), np.ascontiguousarray(conn, dtype=np.int32)
    params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, dtype=np.float64)))
    es = None if elem_set is None else np.ascontiguousarray(elem_set, dtype=np.int32)
    settings = np.array([stab_mult, abs_tol, thickness])
    arrs = [d(a) for a in (nn, settings) + tuple(state) + tuple(fine) + (z_u, z_p, phi)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    E_R, E_C = (np.zeros(len(conn)), np.zeros(len(conn))) if out is None else out
    abs_R, abs_C = (np.zeros(len(conn)), np.zeros(len(conn))) if scales else (None, None)
    got = fn(model.encode(), et, len(conn), conn.ctypes.data_as(ip), ptr(coords), None if es is None else es.ctypes.data_as(ip),
             ptr(params), *[ptr(a) for a in arrs], int(bool(lin)), ptr(E_R), ptr(E_C), ptr(abs_R), ptr(abs_C))
    assert got > 0, (model, et, got)
    return (E_R, E_C, abs_R, abs_C) if scales else (E_R, E_C)


def case_exact(fn, cs, state, fine, adj, lin=False, scales=False, out=None):
    return host_exact(fn, cs.et, cs.c, cs.conn, cs.model, cs.params, state, fine, *adj, lin=lin, nn=cs.nn, scales=scales, out=out)


def smooth(rid, cs):
    """the case's state with xi = error_cases.smooth_state: away from the branch test"""
    st = list(cs.state)
    st[5] = ec.smooth_state(rid, cs)
    return st


def direction(cs, seed, x=True, xi=True, x_prev=True, xi_prev=True):
    """a random direction (du, dp, du_prev, dp_prev, dxi_prev, dxi) in the layout of a state, zero in the parts not asked
    for.  Every part on the scale of the step's own increment: the nodal values by max |u - u_prev| (p: max |p|), each local
    unknown by its own increment over the step (the unknowns of the finite-deformation models differ by three orders of
    magnitude), as the direction of test_E_C_state_derivative_is_the_oracles_local_adjoint_system."""
    rng = np.random.default_rng(seed)
    su = np.abs(cs.u - cs.u_prev).max()
    sp = max(np.abs(cs.p).max(), np.abs(cs.p - cs.p_prev).max())
    inc = np.abs(cs.xi - cs.xi_prev).max(axis=(0, 1))
    inc = np.where(inc > 0, inc, inc.max() if inc.max() > 0 else 1.0)
    du, dpp = su * rng.standard_normal(len(cs.u)), sp * rng.standard_normal(len(cs.p))
    dup, dppp = su * rng.standard_normal(len(cs.u)), sp * rng.standard_normal(len(cs.p))
    dxp, dx = rng.standard_normal(cs.xi.shape) * inc, rng.standard_normal(cs.xi.shape) * inc
    z = np.zeros_like
    return [du if x else z(du), dpp if x else z(dpp), dup if x_prev else z(dup), dppp if x_prev else z(dppp),
            dxp if xi_prev else z(dxp), dx if xi else z(dx)]


def moved(state, d, t=1.0):
    """state + t d, part by part"""
    return [np.ascontiguousarray(np.asarray(s) + t * np.asarray(v)) for s, v in zip(state, d)]


# ---- model_form_error_verify end to end: error_cases.mfe_case, replayed on the CPU --------------------------------------
# The fine model is small_J2 with the hardening modulus K (1 + delta), delta < 0 (error_cases.MFE_DELTA explains the sign).
# The identity E_computed = E_exact has to close to 1e-8 |E_exact| + allowance while the linearization error and the gap
# between eta and E_exact are more than 1000 x that bound, so that the identity is not met by smallness.  Replayed on the CPU
# (test_exact_host.py::test_g_model_form_error_verify_replay), allowance = 3 (z_norm + phi_norm) 1e-12:
#   delta  E_exact      eta          E_lin_R + E_lin_C  |E_computed - E_exact|  allowance  |E_lin| / bound
#   -0.1   -8.2840e-06  -8.2691e-06  -1.4907e-08        8.1e-19                 1.318e-11  1.12e+03   (no room)
#   -0.2   -1.7356e-05  -1.7291e-05  -6.5442e-08        3.8e-18                 1.354e-11  4.77e+03
#   -0.4   -3.8368e-05  -3.8053e-05  -3.1449e-07        4.7e-18                 1.441e-11  2.13e+04   (chosen)
# (bound = 1e-8 |E_exact| + allowance = 1.480e-11 at -0.4; z_norm 1.93, phi_norm 2.87; E_lin_R itself is 1e-16: the global
# residual of small_J2 is linear in the state, so E_lin_R is z . R of the converged fine run.)
MFE_VERIFY_DELTA = -0.4


def replay_verify(fn_err, fn_ex, base, fine):
    """model_form_error_verify on the CPU: base and fine are solved fe_driver.Primal runs over oracle contexts on the same
    mesh; the adjoint of the fine model is marched about the base history (as error_cases.replay_eta does) and the two host
    harnesses are called after every step.  Returns a dict with the fields of calibr8_amd.ModelFormErrorVerify."""
    import fe_driver as fe
    import scipy.sparse.linalg as spla
    b0, be = base.be, fine.be
    prm = be.params
    g, f = np.zeros((be.nelems, be.npts, be.nloc)), np.zeros((be.nelems, be.npts, be.ndofs))
    n3 = be.nnodes * 3
    ls = be.new_linsys()
    eta_f, ex_f, lin_f = [(np.zeros(be.nelems), np.zeros(be.nelems)) for _ in range(3)]
    z_norm = phi_norm = 0.0
    nsteps = len(base.u) - 1
    assert nsteps == len(fine.u) - 1
    hist = lambda r, s: (r.u[s], r.p[s], r.u[s - 1], r.p[s - 1], r.xi[s - 1], r.xi[s])
    for step in range(nsteps, 0, -1):
        st, sf = hist(base, step), hist(fine, step)
        ls.zero()
        be.adjoint_jacobian(*st, g, f, ls)
        fe.apply_dbcs(be, ls, base.dbcs, [np.zeros(n3), np.zeros(be.nnodes)], base.coords, 0.0, is_adjoint=True)
        zz = spla.spsolve(fe.block_matrix(be, ls).tocsc(), fe.rhs_of(be, ls))
        z_u, z_p = np.ascontiguousarray(zz[:n3]), np.ascontiguousarray(zz[n3:])
        phi = np.zeros_like(g)
        be.solve_adjoint_local(*st, z_u, z_p, phi, g, f)
        kw = dict(abs_tol=ec.MFE_TOL)
        ec.host_error(fn_err, be.elem_type, b0.coords, b0.conn, "small_J2", prm, *st, z_u, z_p, phi, out=eta_f, **kw)
        host_exact(fn_ex, be.elem_type, b0.coords, b0.conn, "small_J2", prm, st, sf, z_u, z_p, phi, out=ex_f, **kw)
        host_exact(fn_ex, be.elem_type, b0.coords, b0.conn, "small_J2", prm, st, sf, z_u, z_p, phi, lin=True, out=lin_f, **kw)
        z_norm, phi_norm = max(z_norm, float(np.linalg.norm(zz))), max(phi_norm, float(np.abs(phi).sum()))
    J_H, J_h = base.qoi(), fine.qoi()
    eta, E_lin_R, E_lin_C = float((eta_f[0] + eta_f[1]).sum()), float(lin_f[0].sum()), float(lin_f[1].sum())
    return dict(J_H=J_H, J_h=J_h, eta=eta, E_lin_R=E_lin_R, E_lin_C=E_lin_C, E_exact=J_h - J_H, E_computed=eta + E_lin_R + E_lin_C,
                exact_fields=ex_f, lin_fields=lin_f, eta_fields=eta_f, z_norm=z_norm, phi_norm=phi_norm,
                allowance=nsteps * (z_norm * ec.MFE_TOL + phi_norm * ec.MFE_TOL))
