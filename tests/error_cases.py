"""TEST INFRASTRUCTURE shared by test_error_host.py and test_gpu_error.py: the host harness of the product's per-point
error contributions (tests/error_host/error_host.cpp) and the inputs of its checks.  The model rows, their meshes and their
oracle states are those of cauchy_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import cauchy_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
dp, ip = cc.dp, cc.ip
ABS_TOL = 1e-12  # the local Newton tolerance of the oracle contexts of cauchy_cases.Case (oracle_lib.Oracle's default)


def build_harness(out_dir):
    """compile the harness into out_dir and return its entry point"""
    so = os.path.join(str(out_dir), "liberrorhost.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + cc.CXXFLAGS + ["-shared", "-o", so, os.path.join(HERE, "error_host", "error_host.cpp")])
    fn = C.CDLL(so).error_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, dp, ip, dp, dp, dp] + [dp] * 6 + [dp] * 3 + [dp] * 4
    return fn


def host_error(fn, et, coords, conn, model, params, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi, elem_set=None, nn=None,
               out=None, stab_mult=1.0, abs_tol=ABS_TOL, thickness=1.0, scales=False):
    """(E_R, E_C) [nelems] from the host harness; `out` = (E_R, E_C) is accumulated into.  scales: also the per-element sums
    of the magnitudes of the per-point values, (E_R, E_C, abs_R, abs_C)"""
    d = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    coords, conn = d(coords), np.ascontiguousarray(conn, dtype=np.int32)
    params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, dtype=np.float64)))
    es = None if elem_set is None else np.ascontiguousarray(elem_set, dtype=np.int32)
    settings = np.array([stab_mult, abs_tol, thickness])
    arrs = [d(a) for a in (nn, settings, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    E_R, E_C = (np.zeros(len(conn)), np.zeros(len(conn))) if out is None else out
    abs_R, abs_C = (np.zeros(len(conn)), np.zeros(len(conn))) if scales else (None, None)
    got = fn(model.encode(), et, len(conn), conn.ctypes.data_as(ip), ptr(coords), None if es is None else es.ctypes.data_as(ip),
             ptr(params), *[ptr(a) for a in arrs], ptr(E_R), ptr(E_C), ptr(abs_R), ptr(abs_C))
    assert got > 0, (model, et, got)
    return (E_R, E_C, abs_R, abs_C) if scales else (E_R, E_C)


def adjoints(cs, seed=3):
    """random z_u, z_p, phi for the case cs"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(len(cs.u)), rng.standard_normal(len(cs.p)), rng.standard_normal(cs.xi.shape)


def case_host(fn, cs, z_u, z_p, phi, params=None, xi=None, out=None):
    st = list(cs.state)
    if xi is not None:
        st[5] = xi
    return host_error(fn, cs.et, cs.c, cs.conn, cs.model, cs.params if params is None else params, *st, z_u, z_p, phi, nn=cs.nn, out=out)


def mid_state(cs):
    """the local state halfway along the step: the plastic points then sit above their yield surface by half the step's
    increment and the elastic ones stay below it, so that a perturbation of 1e-5 (relative) of a parameter or of the state
    moves no point across the branch test -- the converged state itself has f = 0 to rounding at every plastic point"""
    return np.ascontiguousarray(cs.xi_prev + 0.5 * (cs.xi - cs.xi_prev))


def softened_state(cs):
    """the converged state with the hardening variable alone taken back to the middle of its increment: the flow stress of a
    plastic point drops, so its yield value is positive by half the step's hardening, and an elastic point (no increment of
    alpha) keeps its converged state and its distance below the surface.  mid_state is not smooth for the models whose local
    state carries the stress (the hypo-elastic rows): halfway between two states on the yield surface the yield value is
    near zero again.  The models without plasticity have no branch: their mid_state."""
    if cs.model in cc.NO_PLASTICITY:
        return mid_state(cs)
    xi = np.array(cs.xi)
    a = cc.ALPHA.get(cs.model, -1)
    xi[:, :, a] = cs.xi_prev[:, :, a] + 0.5 * (cs.xi[:, :, a] - cs.xi_prev[:, :, a])
    return xi


# The state of the derivative checks along xi, per row: mid_state, except where that state is not smooth.  hypo_hosford on
# hex8 and hypo_hill_plane_strain carry the stress in xi and have points that are plastic in both steps: halfway between two
# states on the yield surface their yield value is within the perturbation of zero (difference quotient 1e2 x the scale).
# They take softened_state -- which in turn is not smooth for hypo_barlat on hex8 (a point that has only just yielded has
# next to no hardening to take back).
SOFTENED_ROWS = ("hypo_hosford-hex8", "hypo_hill_plane_strain-tri3")


def smooth_state(rid, cs):
    return softened_state(cs) if rid in SOFTENED_ROWS else mid_state(cs)


def active_params(cs):
    import parity_cases as pc
    return [0, 1, 2] if cs.model == cc.HYBRID else pc.ACTIVE[cs.model]


# ---- model-form error end to end: the case of test_gpu_error.py and its replay on the CPU ------------------------------
MFE_STEPS = 3
MFE_TOL = 1e-12  # Newton (global and local) and linear tolerances of the case
# The fine model hardens with K (1 + delta).  delta < 0: the copied state of a yielded point has f_base = 0, so f_fine =
# -sqrt(2/3) delta K alpha / mu, and the fine model's own branch test (force_path is not supported) keeps the point on the
# plastic branch only when that is positive.  With delta > 0 every yielded point is evaluated on the elastic branch and eta
# does not depend on delta at all (replayed: eta = 1.98e-4 for every delta in 0.025 .. 0.8, beside dJ = 2.0e-6 .. 4.7e-5).
# The size is the replay's choice (test_error_host.py): |eta - dJ| falls by 4.19 from delta to delta / 2 and the deviation of
# eta / (delta K) from dJ/dK by 2.04 (-0.2: 4.39 and 2.09; -0.8 is outside the band: 1.31).
MFE_DELTA = -0.1


def mfe_case():
    """brick 3 x 3 x 3 hex8, small_J2 (parity_cases.J2), pulled along y in three Dirichlet-driven steps into yield; the
    average-displacement objective: (coords, conn, dirichlet conditions as (resid, eq, nodes, fn))"""
    from meshes import brick, jiggle
    c, conn, sets = brick(3, 3, 3, 1.0, 1.0, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero),
            (0, 1, sets["ymax"], lambda x, y, z, t: 0.003 * t), (0, 0, sets["ymax"], zero)]
    return c, conn, spec


def mfe_params(delta):
    import parity_cases as pc
    prm = list(pc.J2)
    prm[2] *= 1.0 + delta
    return prm


def replay_primal(coords, conn, spec, params):
    """the case solved on the CPU: tests/fe_driver.py over the oracle"""
    import fe_driver as fe
    import oracle_lib as ol
    orc = ol.Oracle(ol.HEX8, coords, conn, "small_J2", params, abs_tol=MFE_TOL, rel_tol=MFE_TOL)
    dbcs = [fe.Dbc(*s) for s in spec]
    return fe.Primal(orc, coords, dbcs, max_iters=25, abs_tol=MFE_TOL, rel_tol=MFE_TOL).solve(MFE_STEPS)


def replay_eta(fn, base, fine_params):
    """model_form_error on the CPU: the adjoint march of fe_driver.adjoint_gradient over an oracle context of the fine model
    with the base history, the host harness after every step.  Returns (eta, eta_bound)."""
    import fe_driver as fe
    import oracle_lib as ol
    import scipy.sparse.linalg as spla
    b0 = base.be
    be = ol.Oracle(ol.HEX8, b0.coords, b0.conn, "small_J2", fine_params, abs_tol=MFE_TOL, rel_tol=MFE_TOL)
    g, f = np.zeros((be.nelems, be.npts, be.nloc)), np.zeros((be.nelems, be.npts, be.ndofs))
    n3 = be.nnodes * 3
    ls = be.new_linsys()
    acc = np.zeros(be.nelems), np.zeros(be.nelems)
    for step in range(len(base.u) - 1, 0, -1):
        st = (base.u[step], base.p[step], base.u[step - 1], base.p[step - 1], base.xi[step - 1], base.xi[step])
        ls.zero()
        be.adjoint_jacobian(*st, g, f, ls)
        fe.apply_dbcs(be, ls, base.dbcs, [np.zeros(n3), np.zeros(be.nnodes)], base.coords, 0.0, is_adjoint=True)
        zz = spla.spsolve(fe.block_matrix(be, ls).tocsc(), fe.rhs_of(be, ls))
        z_u, z_p = np.ascontiguousarray(zz[:n3]), np.ascontiguousarray(zz[n3:])
        phi = np.zeros_like(g)
        be.solve_adjoint_local(*st, z_u, z_p, phi, g, f)
        host_error(fn, ol.HEX8, b0.coords, b0.conn, "small_J2", fine_params, *st, z_u, z_p, phi, out=acc, abs_tol=MFE_TOL)
    total = acc[0] + acc[1]
    return float(total.sum()), float(np.abs(total).sum())
