"""`-m gpu`: the device-resident linear solve (c8_krylov_solve, calibr8_amd.device_solver) against
its definition -- the true residual and SciPy's direct solve of the downloaded blocks --, bit for bit against itself, and
through the step drivers against the same runs with the host direct solve."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the fresh process of test_solve_is_reproducible
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from meshes import brick, fields_for, jiggle, notched_bar, prescribed_fields  # noqa: E402
from parity_cases import HILL, HILL_PS, J2  # noqa: E402

pytestmark = pytest.mark.gpu
REL_TOL = 1e-10
TABLE_SIZES = [(16, 4, 4), (32, 8, 8), (48, 12, 12)]  # the notched_bar sizes of DESIGN.md section 13


def golden(name):
    d = json.load(open(os.path.join(HERE, "golden", name)))
    return np.array(d["coords"]), np.array(d["conn"], dtype=np.int32), {k: np.array(v, dtype=np.int32) for k, v in d["node_sets"].items()}


def system_case(case):
    """(element type, coords, conn, model, params, Dirichlet spec [(resid, eq, nodes)], adjoint?)"""
    if case in ("notched_bar", "notched_bar_adjoint") or isinstance(case, tuple):
        n = case if isinstance(case, tuple) else (32, 8, 8)
        c, conn, s = notched_bar(*n)
        spec = [(0, d, s["xmin"]) for d in range(3)] + [(0, 0, s["xmax"])]
        return 8, c, conn, "small_J2", J2, spec, case == "notched_bar_adjoint"
    if case == "jiggled_brick":
        c, conn, s = brick(12, 12, 12)
        spec = [(0, d, s["xmin"]) for d in range(3)] + [(0, 0, s["xmax"])]
        return 8, jiggle(c, s, 0.03), conn, "small_J2", J2, spec, False
    if case == "notch_tet4_hill":
        c, conn, s = golden("notch_tet4.json")
        return 4, c, conn, "small_hill", HILL, [(0, 0, s["xmin"]), (0, 1, s["ymin"]), (0, 2, s["zmin"]), (0, 1, s["ymax"])], False
    c, conn, s = golden("notch2D_tri3.json")
    spec = [(0, 0, s["xmin"]), (0, 1, s["ymin"]), (0, 1, s["ymax"])]
    if case == "notch2D_mechanics":
        return 3, c, conn, "small_J2", J2, spec, False
    assert case == "notch2D_plane_stress"
    return 3, c, conn, "small_hill_plane_stress", HILL_PS, spec, False


def device_system(case):
    """The system of `case` on the device: c8_assemble_forward_jacobian (or c8_assemble_adjoint_jacobian) at a plastic
    state + c8_apply_dirichlet.  Returns the assembler and the LinearSystem."""
    import torch
    from calibr8_amd import Assembler
    et, c, conn, model, params, spec, adjoint = system_case(case)
    asm = Assembler(et, c, conn, model, params)
    u, p = fields_for(asm.ndims, *prescribed_fields(c, 0.004, ramp=True))
    U, P = asm.dev(u), asm.dev(p)
    Z, ZP = torch.zeros_like(U), torch.zeros_like(P)
    ls, xi = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(U, P, Z, ZP, asm.new_state(), xi, ls) == 0
    assert float(xi[:, :, -1].max()) > 0.0  # a plastic state
    if adjoint:
        ls.zero()
        g = torch.zeros(asm.nelems, asm.npts, asm.nloc, dtype=torch.float64, device=asm.device)
        f = torch.zeros(asm.nelems, asm.npts, asm.ndofs, dtype=torch.float64, device=asm.device)
        assert asm.adjoint_jacobian(U, P, Z, ZP, asm.new_state(), xi, g, f, ls) == 0
    dd = [(r, e, torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(np.zeros(len(n)))) for r, e, n in spec]
    asm.apply_dirichlet(dd, U, P, ls, is_adjoint=adjoint)
    torch.cuda.synchronize()
    return asm, ls


def host_system(asm, ls):
    """the downloaded blocks as one SciPy matrix (u rows, then p rows) and the right-hand side"""
    import scipy.sparse as sp
    n, nres = asm.nnodes, asm.nres
    blocks = [[sp.csr_matrix((ls.A[i][j].cpu().numpy(), asm.colidx[i][j], asm.rowptr[i][j]), shape=(n * asm.neq[i], n * asm.neq[j]))
               for j in range(nres)] for i in range(nres)]
    return sp.bmat(blocks, format="csr"), np.concatenate([ls.b[i].cpu().numpy() for i in range(nres)])


def new_dx(asm):
    import torch
    return (torch.full((asm.nnodes * asm.ndims,), 7.0, dtype=torch.float64, device=asm.device),  # (the start vector is 0
            torch.full((asm.nnodes,), 7.0, dtype=torch.float64, device=asm.device))              #  whatever dx holds)


def raw_solve(asm, ls, dx, **opts):
    """c8_krylov_solve straight through the ABI: (return code, info, x on the host)"""
    import torch
    from calibr8_amd import lib
    o = lib.KrylovOpts(opts.get("max_iters", 0), opts.get("check_every", 0), opts.get("max_restarts", 0), opts.get("rel_tol", REL_TOL), 0.0)
    info = lib.KrylovInfo()
    sy = ls.c_struct()
    ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
    rc = asm.L.c8_krylov_solve(asm.h, C.byref(sy), ptrs, C.byref(o), C.byref(info))
    torch.cuda.synchronize()
    x = np.concatenate([dx[i].cpu().numpy() for i in range(asm.nres)])
    return rc, info, x


def node_block_jacobi(asm, A):
    """the preconditioner of the device solve as a SciPy operator: inverse of each node's own diagonal block"""
    import scipy.sparse.linalg as spla
    n, nd = asm.nnodes, asm.ndims
    nb = nd + (1 if asm.nres == 2 else 0)
    idx = np.zeros((n, nb), dtype=np.int64)
    for k in range(nb):
        idx[:, k] = np.arange(n) * nd + k if k < nd else n * nd + np.arange(n)
    Ac = A.tocsr()
    D = np.stack([np.asarray(Ac[idx[:, r]][:, idx[:, c]].diagonal()) for r in range(nb) for c in range(nb)], axis=1).reshape(n, nb, nb)
    Dinv = np.linalg.inv(D)

    def apply(v):
        out = np.zeros_like(v)
        out[idx] = np.einsum("nij,nj->ni", Dinv, v[idx])
        return out
    return spla.LinearOperator(A.shape, matvec=apply)


# ---- 1. single solves against the definition --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["notched_bar", "jiggled_brick", "notch_tet4_hill", "notch2D_mechanics", "notch2D_plane_stress",
                                  "notched_bar_adjoint"])
def test_single_solve_meets_its_contract(case):
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    asm, ls = device_system(case)
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    A, b = host_system(asm, ls)
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    lu = spla.splu(A.tocsc())
    x_ref = lu.solve(b)
    inv_op = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    cond_est = spla.onenormest(A) * spla.onenormest(inv_op)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print("%s: n %d rc %d iters %d restarts %d host residual %.3e info %.3e cond_est %.3e x error %.3e" %
          (case, len(b), rc, info.iters, info.restarts, res, info.residual_norm / info.b_norm, cond_est, err))
    assert rc == lib.C8_OK and info.status == lib.C8_OK, asm.L.c8_last_error()
    assert res <= 1.01 * REL_TOL
    assert abs(info.residual_norm / np.linalg.norm(b - A @ x) - 1.0) < 1e-6
    assert abs(info.b_norm / np.linalg.norm(b) - 1.0) < 1e-12
    assert err <= cond_est * REL_TOL


# ---- 2. reproducible ---------------------------------------------------------------------------------------------------
def _solve_for_bytes(case="notched_bar"):
    asm, ls = device_system(case)
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == 0
    return info.iters, x


def test_solve_is_reproducible(tmp_path):
    asm, ls = device_system("notched_bar")
    rc1, i1, x1 = raw_solve(asm, ls, new_dx(asm))
    rc2, i2, x2 = raw_solve(asm, ls, new_dx(asm))
    assert rc1 == 0 and rc2 == 0
    assert i1.iters == i2.iters and x1.tobytes() == x2.tobytes()
    out = str(tmp_path / "x.bin")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), out])
    raw = np.fromfile(out)
    assert int(raw[0]) == i1.iters and raw[1:].tobytes() == x1.tobytes()


# ---- 3. reference decks end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck", ["cube_elastic", "cube_hyper_J2", "notch_small_J2", "notch2D_small_J2_plane_stress"])
def test_reference_decks_with_the_device_solver(deck):
    from calibr8_amd import Assembler, PrimalDriver, device_solver, scipy_solver
    zero = lambda x, y, z, t: 0.0
    kw = {}
    if deck.startswith("cube"):
        c, conn, ns = golden("cube_tet4.json")
        sym = [(0, 0, ns["xmin"], zero), (0, 1, ns["ymin"], zero), (0, 2, ns["zmin"], zero)]
        if deck == "cube_elastic":
            make = lambda: Assembler(4, c, conn, "elastic", [1000.0, 0.25, 1e-3, 10.0])
            dbcs, nsteps, expected, tol = sym, 1, 5.00000000000000184e-3, 1e-6
        else:
            make = lambda: Assembler(4, c, conn, "hyper_J2", [1000.0, 0.25, 10.0, 0.0, 0.0, 0.0, 0.0, 100.0], max_iters=30)
            dbcs, nsteps, expected, tol = sym + [(0, 1, ns["ymax"], lambda x, y, z, t: 0.01 * t)], 10, 1.57817536611772440e-02, 1e-4
    elif deck == "notch_small_J2":
        c, conn, ns = golden("notch_tet4.json")
        make = lambda: Assembler(4, c, conn, "small_hill", [1000.0, 0.25, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 10.0, 2.0], max_iters=500)
        dbcs = [(0, 0, ns["xmin"], zero), (0, 1, ns["ymin"], zero), (0, 2, ns["zmin"], zero), (0, 1, ns["ymax"], lambda x, y, z, t: 0.001 * t)]
        nsteps, expected, tol = 4, 1.4622046563394649e-04, 1e-9
    else:
        c, conn, ns = golden("notch2D_tri3.json")
        make = lambda: Assembler(3, c, conn, "small_hill_plane_stress", [1000.0, 0.25, 2.0, 10.0, 2.0, 1.0, 1.0, 1.0, 1.0])
        dbcs = [(0, 0, ns["xmin"], zero), (0, 1, ns["ymin"], zero), (0, 1, ns["ymax"], lambda x, y, z, t: 0.001 * t)]
        nsteps, expected, tol, kw = 4, 2.2831790025047405e-03, 1e-9, {"max_iters": 30}
    a_dev, a_host = make(), make()
    solver = device_solver(a_dev)
    dev = PrimalDriver(a_dev, dbcs, solver=solver, **kw).solve(nsteps)
    host = PrimalDriver(a_host, dbcs, solver=scipy_solver(a_host), **kw).solve(nsteps)
    Jd, Jh = dev.qoi(), host.qoi()
    print("%s: Newton %s / %s, linear solves %d, BiCGStab iterations %d, J %.16e / %.16e" %
          (deck, dev.newton_iters, host.newton_iters, solver.solves, solver.total_iters, Jd, Jh))
    assert solver.solves > 0 and solver.total_iters > 0 and solver.last.status == 0
    assert dev.newton_iters == host.newton_iters
    assert abs(Jd / Jh - 1.0) < 1e-8
    assert abs(Jd / expected - 1.0) < tol


# ---- 4. adjoint path -------------------------------------------------------------------------------------------------
def test_adjoint_gradient_with_the_device_solver():
    from calibr8_amd import Assembler, PrimalDriver, adjoint_gradient, device_solver
    c, conn, sets = brick(3, 4, 3, 1.0, 1.5, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero),
            (0, 1, sets["ymax"], lambda x, y, z, t: 0.003 * t), (0, 0, sets["ymax"], zero)]
    act = [0, 1, 2, 3]
    base = np.array(J2)

    def solve(params, device=True):
        asm = Assembler(8, c, conn, "small_J2", params)
        asm.set_active(0, act)
        return PrimalDriver(asm, spec, max_iters=15, abs_tol=1e-12, rel_tol=1e-12, solver=device_solver(asm) if device else None).solve(3)

    pr = solve(base)
    grad = adjoint_gradient(pr, len(act))
    assert pr.solver.solves >= 3 + sum(n - 1 for n in pr.newton_iters)  # the adjoint steps went through the device solve too
    gref = adjoint_gradient(solve(base, device=False), len(act))
    print("gradient device solver", grad, "host direct solve", gref)
    assert np.abs(grad - gref).max() < 1e-7 * np.abs(gref).max()
    direction = np.array([100.0, 0.02, 10.0, 0.2])
    gd = float(grad @ direction)
    errs = []
    for k in range(2, 7):
        h = 10.0 ** (-k)
        pp, pm = base.copy(), base.copy()
        pp[act] += h * direction
        pm[act] -= h * direction
        errs.append(abs((solve(pp).qoi() - solve(pm).qoi()) / (2 * h) - gd))
    print("central differences", errs, gd)
    assert min(errs) < 1e-7 * abs(gd) and max(errs) < 1e-4 * abs(gd), (errs, gd)


# ---- 5. calibration --------------------------------------------------------------------------------------------------
def test_inverse_problem_recovers_parameters_with_the_device_solver():
    import torch
    from calibr8_amd import Assembler, InverseProblem, PrimalDriver, device_solver
    c, conn, sets = brick(3, 4, 2, 1.0, 1.5, 1.0)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["xmin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["zmin"], zero),
            (0, 1, sets["ymax"], lambda x, y, z, t: 0.002 * t)]
    xmax = set(sets["xmax"].tolist())
    loc = ([0, 1, 2, 3], [0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [3, 0, 4, 7], [4, 5, 6, 7])
    faces = [[int(e[k]) for k in f] for e in conn for f in loc if all(int(e[k]) in xmax for k in f)]
    nsteps, truth = 3, np.array(J2)
    measured = [None]
    iters = [0, 0]

    def make_primal(params):
        asm = Assembler(8, c, conn, "small_J2", params)
        asm.set_qoi_calibration(faces, weights=(1.0, 1.0, 1.0), balance=1e-2, coord_idx=1, coord_value=0.0,
                                coord_tol=1e-8, comp=1, dt_over_T=1.0 / nsteps)
        pr = PrimalDriver(asm, spec, max_iters=20, abs_tol=1e-12, rel_tol=1e-12, solver=device_solver(asm)).solve(nsteps)
        iters[0] += pr.solver.solves
        iters[1] += pr.solver.total_iters
        if measured[0] is not None:
            pr.set_measured(*measured[0])
        return pr

    pt = make_primal(truth)
    loads, zm = [0.0], torch.zeros_like(pt.u[1])
    for s in range(1, nsteps + 1):
        pt.asm.set_measured(zm, 0.0)
        loads.append(pt.asm.qoi_preprocess(pt.u[s], pt.p[s], pt.u[s - 1], pt.p[s - 1], pt.xi[s - 1], pt.xi[s])[1])
    measured[0] = ([None] + [u.clone() for u in pt.u[1:]], loads)
    active = [2, 3]
    inv = InverseProblem(make_primal, truth, active, bounds=[[50.0, 200.0], [1.0, 4.0]])
    start = np.array([150.0, 3.0])
    found, info = inv.solve(start, max_iters=40, grad_tol=1e-14, step_tol=1e-12, max_ls_evals=8)
    print("found", found, info, "forward linear solves", iters)
    assert iters[0] > 0
    assert np.abs(found / truth[active] - 1.0).max() < 1e-3, (found, info)


# ---- 6. contract -----------------------------------------------------------------------------------------------------
def test_contract_of_the_refusals():
    import torch
    from calibr8_amd import lib
    import calibr8_amd.distributed as D
    asm, ls = device_system((16, 4, 4))
    A, b = host_system(asm, ls)
    # the iteration budget: not converged, the iterate and the true residual are reported
    dx = new_dx(asm)
    rc, info, x = raw_solve(asm, ls, dx, max_iters=3)
    assert rc == lib.C8_NOT_CONVERGED and info.status == lib.C8_NOT_CONVERGED and info.iters == 3
    assert np.isfinite(x).all() and np.abs(x).max() > 0
    # the same number as the host's: A x in the same CSR order on both sides; not compared bitwise because the norm itself
    # (sum of n squares: a block tree on the device, BLAS on the host) is rounded differently, by at most n eps < 1e-9
    assert abs(info.residual_norm / np.linalg.norm(b - A @ x) - 1.0) < 1e-9
    assert b"c8_krylov_solve" in asm.L.c8_last_error()
    # b = 0
    saved = [ls.b[i].clone() for i in range(2)]
    for i in range(2):
        ls.b[i].zero_()
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == lib.C8_OK and info.iters == 0 and not x.any() and info.b_norm == 0.0
    for i in range(2):
        ls.b[i].copy_(saved[i])
    # null pointers
    sy = ls.c_struct()
    ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
    L = asm.L
    assert L.c8_krylov_solve(None, C.byref(sy), ptrs, None, None) == lib.C8_ERR_ARG
    assert L.c8_krylov_solve(asm.h, None, ptrs, None, None) == lib.C8_ERR_ARG
    assert L.c8_krylov_solve(asm.h, C.byref(sy), None, None, None) == lib.C8_ERR_ARG
    assert L.c8_krylov_solve(asm.h, C.byref(sy), (C.c_void_p * 2)(dx[0].data_ptr(), None), None, None) == lib.C8_ERR_ARG
    bad = ls.c_struct()
    bad.A[0][1] = None
    assert L.c8_krylov_solve(asm.h, C.byref(bad), ptrs, None, None) == lib.C8_ERR_ARG
    assert L.c8_krylov_linear_solve(None, C.byref(sy), ptrs) == lib.C8_ERR_ARG
    # defaults (opts NULL) solve the system
    assert L.c8_krylov_solve(asm.h, C.byref(sy), ptrs, None, None) == lib.C8_OK
    # one node's diagonal block zeroed: refused by the set-up kernel's flag, the node is named
    node = asm.nnodes // 2
    rp, ci = asm.rowptr, asm.colidx
    for i in range(2):
        for j in range(2):
            vals = ls.A[i][j].cpu().numpy()
            for eq in range(asm.neq[i]):
                row = node * asm.neq[i] + eq
                lo, hi = rp[i][j][row], rp[i][j][row + 1]
                cols = ci[i][j][lo:hi]
                vals[lo:hi][(cols // asm.neq[j]) == node] = 0.0
            ls.A[i][j].copy_(asm.dev(vals))
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == lib.C8_ERR_ARG and ("node %d " % node).encode() in L.c8_last_error(), L.c8_last_error()
    # a context with a halo attached (host transport, one rank): the multi-part solve is not implemented
    et, c, conn, model, params, _, _ = system_case((16, 4, 4))
    part = D.part_from_global(c, conn, np.zeros(len(conn), dtype=np.int32), 0, 1)
    plan = D.HaloPlan(part, None)
    from calibr8_amd import Assembler
    asm2 = Assembler(et, plan.coords, part.conn, model, params)
    comm = D.Comm.host(None, 0, 1)
    halo = D.Halo(plan, asm2.rowptr[1][1], asm2.colidx[1][1], asm2, comm)
    ls2 = asm2.new_linsys()
    sy2 = ls2.c_struct()
    dx2 = new_dx(asm2)
    info = lib.KrylovInfo()
    rc = L.c8_krylov_solve(asm2.h, C.byref(sy2), (C.c_void_p * 2)(dx2[0].data_ptr(), dx2[1].data_ptr()), None, C.byref(info))
    assert rc == lib.C8_ERR_UNSUPPORTED and info.status == lib.C8_ERR_UNSUPPORTED and b"halo" in L.c8_last_error()
    torch.cuda.synchronize()
    halo.close()
    comm.close()


# ---- 7. iteration counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", TABLE_SIZES)
def test_iteration_counts_beside_scipy_bicgstab(size):
    """Convergence, and no more than twice SciPy's BiCGStab iterations for the same matrix, preconditioner and tolerance.
    Recorded on one MI355X (device / SciPy): 313 / 299, 925 / 1098, 2231 / 2146."""
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    asm, ls = device_system(size)
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    A, b = host_system(asm, ls)
    count = [0]

    def cb(_):
        count[0] += 1
    xs, flag = spla.bicgstab(A, b, rtol=REL_TOL, atol=0.0, maxiter=20000, M=node_block_jacobi(asm, A), callback=cb)
    res_s = np.linalg.norm(b - A @ xs) / np.linalg.norm(b)
    print("notched_bar%s: elements %d unknowns %d device iterations %d (restarts %d, residual %.2e), SciPy BiCGStab %d (flag %d, residual %.2e)" %
          (size, asm.nelems, len(b), info.iters, info.restarts, info.residual_norm / info.b_norm, count[0], flag, res_s))
    assert rc == lib.C8_OK, asm.L.c8_last_error()
    assert flag == 0
    assert info.iters <= 2 * count[0]


if __name__ == "__main__":
    it, x = _solve_for_bytes()
    np.concatenate([[float(it)], x]).tofile(sys.argv[1])
