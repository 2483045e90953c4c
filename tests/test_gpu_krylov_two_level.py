"""`-m gpu`: the two-level preconditioner of the device solve (C8_PRECOND_TWO_LEVEL) against its
definition in include/c8.h: the aggregates, the prolongator, A_c = P^T A P and the operator are replayed in numpy on the
downloaded blocks; the solve meets the contract of the one-level kinds, takes at most half the iterations of the
Gauss-Seidel one and grows slower with the mesh, is reproducible bit for bit, and leaves the other kinds as they were."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the fresh process of test_two_level_solve_is_reproducible
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from test_gpu_krylov import REL_TOL, device_system, host_system, new_dx, raw_solve, system_case  # noqa: E402
from test_gpu_krylov_sgs import (CASES, JACOBI, SGS, Replay, adjoint_system, device_apply, device_colors, node_index, precond,  # noqa: E402
                                 set_precond, system)

pytestmark = pytest.mark.gpu
TWO_LEVEL = 3   # C8_PRECOND_TWO_LEVEL (2 is no kind: test_gpu_krylov_sgs.py::test_refusals_and_state)
COARSE_CAP = 8192


# ---- the definition in numpy ----------------------------------------------------------------------------------------------
def aggregate_replay(rowptr, colidx, n):
    """the three passes of include/c8.h over the node graph: (aggregate of every node, number of aggregates)"""
    agg = np.full(n, -1, dtype=np.int64)
    nagg = 0
    for i in range(n):
        row = colidx[rowptr[i]:rowptr[i + 1]]
        if (agg[row] < 0).all():
            agg[row] = nagg
            nagg += 1
    first = agg.copy()
    for i in range(n):
        if agg[i] < 0:
            row = colidx[rowptr[i]:rowptr[i + 1]]
            hit = row[first[row] >= 0]
            if len(hit):
                agg[i] = first[hit.min()]
    for i in range(n):
        if agg[i] < 0:
            agg[i] = nagg
            nagg += 1
    return agg, nagg


def device_aggregates(asm):
    """c8_krylov_aggregates: (aggregate of every node, number of aggregates)"""
    from calibr8_amd import lib
    na, ptr = C.c_int32(), C.POINTER(C.c_int32)()
    lib.check(asm.L.c8_krylov_aggregates(asm.h, C.byref(na), C.byref(ptr)))
    return np.ctypeslib.as_array(ptr, shape=(asm.nnodes,)).astype(np.int64), na.value


def device_coarse_matrix(asm, ls):
    from calibr8_amd import lib
    n = C.c_int32()
    sy = ls.c_struct()
    lib.check(asm.L.c8_krylov_coarse_matrix(asm.h, C.byref(sy), C.byref(n), None))
    out = np.full((n.value, n.value), 7.0)
    lib.check(asm.L.c8_krylov_coarse_matrix(asm.h, C.byref(sy), C.byref(n), out.ctypes.data_as(lib.dp)))
    return out


def constrained_rows(A):
    """rows of A whose off-diagonal entries are all exactly 0"""
    off = A.tocsr().copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    return np.diff(off.indptr) == 0


def prolongator(asm, A, agg, nagg):
    """P of include/c8.h as a SciPy matrix, from the aggregates, the coordinates and the constrained rows of A"""
    import scipy.sparse as sp
    n, nd, two = asm.nnodes, asm.ndims, asm.nres == 2
    nc = nd + (3 if nd == 3 else 1) + (1 if two else 0)
    idx = node_index(n, nd, asm.nres)
    x = asm.coords[:, :nd]
    d = np.zeros((n, nd))
    for a in range(nagg):
        nodes = np.nonzero(agg == a)[0]
        d[nodes] = x[nodes] - np.cumsum(x[nodes], axis=0)[-1] / len(nodes)   # (summed in ascending id)
    rows, cols, vals = [], [], []

    def put(eq, col, v):
        rows.append(idx[:, eq])
        cols.append(agg * nc + col)
        vals.append(v * np.ones(n))
    for m in range(nd):
        put(m, m, 1.0)
    if nd == 3:
        for m in range(3):
            rot = np.cross(np.eye(3)[m], d)          # e_m x (x_i - centroid)
            for r in range(3):
                put(r, 3 + m, rot[:, r])
    else:
        put(0, 2, -d[:, 1])
        put(1, 2, d[:, 0])
    if two:
        put(nd, nc - 1, 1.0)
    P = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(A.shape[0], nagg * nc))
    P = sp.diags((~constrained_rows(A)).astype(float)) @ P
    P.eliminate_zeros()
    return P.tocsr()


def coarse_replay(A, P):
    """A_c = P^T A P with a unit diagonal where a column of P is zero"""
    Ac = (P.T @ A @ P).toarray()
    zero = np.nonzero(np.diff(P.tocsc().indptr) == 0)[0]
    Ac[zero, zero] = 1.0
    return Ac


class ReplayFrom(Replay):
    """Replay.sgs started from a given vector instead of 0"""

    def sgs_from(self, v, x0):
        x = np.array(x0, dtype=np.float64)
        nc, nb = len(self.colors), self.idx.shape[1]
        for _ in range(self.sweeps):
            for k in list(range(nc)) + list(range(nc - 2, -1, -1)):
                r = (v[self.rows[k]] - self.Ac[k] @ x).reshape(-1, nb)
                x[self.rows[k]] += np.einsum("nij,nj->ni", self.Dinv[self.colors[k]], r).ravel()
        return x


class TwoLevel:
    """y = M^-1 v of the definition, in numpy"""

    def __init__(self, asm, A, sweeps=1):
        import scipy.linalg as sl
        self.agg, self.nagg = device_aggregates(asm)
        self.P = prolongator(asm, A, self.agg, self.nagg)
        self.Ac = coarse_replay(A, self.P)
        self.lu = sl.lu_factor(self.Ac)
        self.rep = ReplayFrom(A, node_index(asm.nnodes, asm.ndims, asm.nres), device_colors(asm), sweeps)

    def apply(self, v):
        import scipy.linalg as sl
        v = np.asarray(v, dtype=np.float64)
        return self.rep.sgs_from(v, self.P @ sl.lu_solve(self.lu, self.P.T @ v))


@functools.lru_cache(maxsize=None)
def replay(case):
    """the numpy operator (one sweep) of system(case), built once per session"""
    asm, ls, A, b = system(case)
    return TwoLevel(asm, A)


def dirichlet_rows(asm, case):
    spec = system_case(case)[5]
    return np.unique(np.concatenate([np.asarray(nodes) * asm.ndims + eq for resid, eq, nodes in spec if resid == 0]))


# ---- 1. aggregates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(16, 4, 4), "jiggled_brick", "notch_tet4_hill", "notch2D_mechanics", "notch2D_plane_stress"])
def test_aggregates_are_the_three_pass_ones(case):
    asm = system(case)[0]
    agg, nagg = device_aggregates(asm)
    ref, nref = aggregate_replay(asm.rowptr[1][1], asm.colidx[1][1], asm.nnodes)
    sizes = np.bincount(agg, minlength=nagg)
    print("%s: %d nodes, %d aggregates, sizes min %d max %d" % (case, asm.nnodes, nagg, sizes.min(), sizes.max()))
    assert agg.min() == 0 and agg.max() == nagg - 1 and sizes.min() >= 1        # every node in exactly one aggregate
    assert nagg == nref and np.array_equal(agg, ref)                            # the same ids: in order of creation


# ---- 2. the coarse matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_coarse_matrix_equals_pt_a_p(case):
    asm, ls, A, b = system(case)
    rep = replay(case)
    Ac = device_coarse_matrix(asm, ls)
    err = np.linalg.norm(Ac - rep.Ac) / np.linalg.norm(rep.Ac)
    con = np.nonzero(constrained_rows(A))[0]
    print("%s: unknowns %d aggregates %d n_coarse %d constrained rows %d |A_c - P^T A P|_F / |P^T A P|_F %.3e" %
          (case, len(b), rep.nagg, Ac.shape[0], len(con), err))
    assert Ac.shape == rep.Ac.shape
    assert err < 1e-12
    if case.startswith("notched_bar"):
        assert np.array_equal(con, dirichlet_rows(asm, case))


# ---- 3. the operator against its definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_operator_equals_its_definition(case):
    """|y - y_ref| / |y_ref| <= 100 eps cond(A_c): the coarse solve is the only ill-conditioned step (the device applies an
    explicit inverse, numpy an LU solve), every other step differs in the order of sums only"""
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    base = replay(case)
    cond = np.linalg.cond(base.Ac)
    bound = 100.0 * np.finfo(np.float64).eps * cond
    v = np.random.default_rng(13).standard_normal(len(b))
    for sweeps in (1, 2):
        with precond(asm, TWO_LEVEL, sweeps):
            assert asm.L.c8_krylov_get_preconditioner(asm.h) == TWO_LEVEL
            rc, y = device_apply(asm, ls, v)
        assert rc == lib.C8_OK, asm.L.c8_last_error()
        base.rep.sweeps = sweeps
        y_ref = base.apply(v)
        base.rep.sweeps = 1
        err = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
        print("%s: n %d n_coarse %d cond(A_c) %.3e sweeps %d operator error %.3e bound %.3e" % (case, len(b), base.Ac.shape[0], cond, sweeps, err, bound))
        assert err <= bound


# ---- 4. the contract of the solve ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_two_level_solve_meets_the_contract(case):
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    with precond(asm, TWO_LEVEL):
        rc, info, x = raw_solve(asm, ls, new_dx(asm))
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    lu = spla.splu(A.tocsc())
    x_ref = lu.solve(b)
    inv_op = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    cond_est = spla.onenormest(A) * spla.onenormest(inv_op)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print("%s (two-level): n %d rc %d iters %d restarts %d host residual %.3e info %.3e cond_est %.3e x error %.3e" %
          (case, len(b), rc, info.iters, info.restarts, res, info.residual_norm / info.b_norm, cond_est, err))
    assert rc == lib.C8_OK and info.status == lib.C8_OK, asm.L.c8_last_error()
    assert info.iters > 0 and info.b_norm > 0.0
    assert res <= 1.01 * REL_TOL
    assert abs(info.residual_norm / np.linalg.norm(b - A @ x) - 1.0) < 1e-6
    assert abs(info.b_norm / np.linalg.norm(b) - 1.0) < 1e-12
    assert err <= cond_est * REL_TOL


# ---- 5. iteration counts --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts(size, adjoint):
    """(device two-level, device SGS, SciPy BiCGStab with the numpy two-level operator) on K1 / K3 of notched_bar(*size)"""
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    if adjoint:
        asm, ls = adjoint_system(size)
        A, b = host_system(asm, ls)
        A = A.tocsr()
    else:
        asm, ls, A, b = system(size)
    with precond(asm, SGS):
        rcs, isg, _ = raw_solve(asm, ls, new_dx(asm))
    with precond(asm, TWO_LEVEL):
        rct, itl, _ = raw_solve(asm, ls, new_dx(asm))
    op = TwoLevel(asm, A)
    count = [0]

    def cb(_):
        count[0] += 1
    xs, flag = spla.bicgstab(A, b, rtol=REL_TOL, atol=0.0, maxiter=20000, M=spla.LinearOperator(A.shape, matvec=op.apply), callback=cb)
    print("notched_bar%s %s: unknowns %d aggregates %d n_coarse %d device iterations two-level %d (restarts %d) SGS %d (restarts %d), "
          "SciPy BiCGStab with the two-level operator %d (flag %d)" %
          (size, "K3 (adjoint)" if adjoint else "K1", len(b), op.nagg, op.Ac.shape[0], itl.iters, itl.restarts, isg.iters, isg.restarts, count[0], flag))
    assert rcs == lib.C8_OK and rct == lib.C8_OK, asm.L.c8_last_error()
    assert flag == 0
    return itl.iters, isg.iters, count[0]


@pytest.mark.parametrize("size", [(16, 4, 4), (32, 8, 8)])
@pytest.mark.parametrize("adjoint", [False, True])
def test_iteration_counts(size, adjoint):
    """device two-level <= 2 x SciPy BiCGStab with the numpy operator (the margin of test_iteration_counts_beside_scipy_bicgstab)
    and <= half the device count with Gauss-Seidel (CPU ratios 5 and 9 on K1)"""
    two, sgs, scipy_two = counts(size, adjoint)
    assert two <= 2 * scipy_two
    assert 2 * two <= sgs


def test_iteration_counts_grow_slower_than_one_level():
    """K1 on (32,8,8) takes <= 1.75 x the iterations on (16,4,4): the CPU replay gives 1.31 with two levels, 2.4 with SGS"""
    small, large = counts((16, 4, 4), False)[0], counts((32, 8, 8), False)[0]
    print("two-level K1 iterations (16,4,4) %d (32,8,8) %d ratio %.2f" % (small, large, large / small))
    assert large <= 1.75 * small


# ---- 6. reproducible --------------------------------------------------------------------------------------------------------------
def _solve_for_bytes():
    asm, ls = device_system((16, 4, 4))
    set_precond(asm, TWO_LEVEL, 1)
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == 0
    return info.iters, x


def test_two_level_solve_is_reproducible(tmp_path):
    asm, ls = system((16, 4, 4))[:2]
    with precond(asm, TWO_LEVEL):
        rc1, i1, x1 = raw_solve(asm, ls, new_dx(asm))
        rc2, i2, x2 = raw_solve(asm, ls, new_dx(asm))
    assert rc1 == 0 and rc2 == 0
    assert i1.iters == i2.iters and x1.tobytes() == x2.tobytes()
    out = str(tmp_path / "x.bin")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), out])
    raw = np.fromfile(out)
    assert int(raw[0]) == i1.iters and raw[1:].tobytes() == x1.tobytes()


# ---- 7. state and refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [JACOBI, SGS])
def test_switching_kinds_leaves_the_other_kinds_as_they_were(other):
    from calibr8_amd import lib
    asm, ls = device_system((16, 4, 4))
    set_precond(asm, other)
    set_precond(asm, TWO_LEVEL, 0)                      # sweeps <= 0: one sweep
    assert asm.L.c8_krylov_get_preconditioner(asm.h) == lib.C8_PRECOND_TWO_LEVEL == TWO_LEVEL
    assert asm.krylov_preconditioner == "two_level"
    v = np.random.default_rng(5).standard_normal(asm.nnodes * (asm.ndims + 1))
    rc0, y0 = device_apply(asm, ls, v)
    set_precond(asm, TWO_LEVEL, 1)
    rc1, y1 = device_apply(asm, ls, v)
    assert rc0 == 0 and rc1 == 0 and y0.tobytes() == y1.tobytes()
    rc, info_t, xt = raw_solve(asm, ls, new_dx(asm))
    assert rc == lib.C8_OK
    set_precond(asm, other)
    rc, info_a, xa = raw_solve(asm, ls, new_dx(asm))
    asm_b, ls_b = device_system((16, 4, 4))             # a context that never switched
    set_precond(asm_b, other)
    rc_b, info_b, xb = raw_solve(asm_b, ls_b, new_dx(asm_b))
    assert rc == lib.C8_OK and rc_b == lib.C8_OK
    assert info_a.iters == info_b.iters and xa.tobytes() == xb.tobytes()
    assert info_t.iters < info_a.iters


def test_refusals():
    import torch
    from calibr8_amd import Assembler, lib
    import calibr8_amd.distributed as D
    from meshes import brick
    from parity_cases import J2
    # a halo attached (host transport, one rank)
    et, c, conn, model, params, _, _ = system_case((16, 4, 4))
    part = D.part_from_global(c, conn, np.zeros(len(conn), dtype=np.int32), 0, 1)
    plan = D.HaloPlan(part, None)
    asm = Assembler(et, plan.coords, part.conn, model, params)
    L = asm.L
    comm = D.Comm.host(None, 0, 1)
    halo = D.Halo(plan, asm.rowptr[1][1], asm.colidx[1][1], asm, comm)
    set_precond(asm, TWO_LEVEL)
    ls = asm.new_linsys()
    sy = ls.c_struct()
    dx = new_dx(asm)
    ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
    info = lib.KrylovInfo()
    na, ap, n = C.c_int32(), C.POINTER(C.c_int32)(), C.c_int32()
    for rc in (L.c8_krylov_solve_parts(asm.h, C.byref(sy), ptrs, None, C.byref(info)),
               L.c8_krylov_precondition(asm.h, C.byref(sy), ptrs, ptrs),
               L.c8_krylov_aggregates(asm.h, C.byref(na), C.byref(ap)),
               L.c8_krylov_coarse_matrix(asm.h, C.byref(sy), C.byref(n), None)):
        assert rc == lib.C8_ERR_UNSUPPORTED and b"halo" in L.c8_last_error() and b"two-level" in L.c8_last_error(), L.c8_last_error()
    assert info.status == lib.C8_ERR_UNSUPPORTED and info.iters == 0
    torch.cuda.synchronize()
    halo.close()
    comm.close()
    # the cap of the dense coarse solve: refused before anything is read or iterated (the system is never assembled)
    c, conn, s = brick(36, 36, 36)
    big = Assembler(8, c, conn, "small_J2", J2)
    agg, nagg = device_aggregates(big)
    n_coarse = nagg * 7
    print("brick(36,36,36): %d nodes, %d aggregates, n_coarse %d" % (big.nnodes, nagg, n_coarse))
    assert n_coarse > COARSE_CAP
    set_precond(big, TWO_LEVEL)
    lsb = big.new_linsys()
    rc, info, x = raw_solve(big, lsb, new_dx(big))
    msg = L.c8_last_error()
    assert rc == lib.C8_ERR_UNSUPPORTED and info.status == lib.C8_ERR_UNSUPPORTED and info.iters == 0
    assert ("n_coarse = %d" % n_coarse).encode() in msg and b"8192" in msg, msg
    rc, _ = device_apply(big, lsb, np.ones(big.nnodes * 4))
    assert rc == lib.C8_ERR_UNSUPPORTED and b"8192" in L.c8_last_error()
    syb = lsb.c_struct()
    assert L.c8_krylov_coarse_matrix(big.h, C.byref(syb), C.byref(n), None) == lib.C8_ERR_UNSUPPORTED
    # one node's diagonal block zeroed: the node is named, as with the one-level kinds
    asm, ls = device_system((16, 4, 4))
    set_precond(asm, TWO_LEVEL)
    node = asm.nnodes // 2
    rp, ci = asm.rowptr, asm.colidx
    for i in range(2):
        for j in range(2):
            vals = ls.A[i][j].cpu().numpy()
            for eq in range(asm.neq[i]):
                row = node * asm.neq[i] + eq
                lo, hi = rp[i][j][row], rp[i][j][row + 1]
                vals[lo:hi][(ci[i][j][lo:hi] // asm.neq[j]) == node] = 0.0
            ls.A[i][j].copy_(asm.dev(vals))
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == lib.C8_ERR_ARG and info.iters == 0 and ("node %d " % node).encode() in L.c8_last_error(), L.c8_last_error()
    rc, _ = device_apply(asm, ls, np.ones(asm.nnodes * 4))
    assert rc == lib.C8_ERR_ARG and ("node %d " % node).encode() in L.c8_last_error(), L.c8_last_error()
    # 2 (left unassigned) and the value after the last kind are unknown kinds; a refused call changes nothing
    for kind in (2, 4):
        assert L.c8_krylov_set_preconditioner(asm.h, kind, 1) == lib.C8_ERR_ARG and b"unknown preconditioner" in L.c8_last_error()
        assert L.c8_krylov_get_preconditioner(asm.h) == TWO_LEVEL
    # null arguments of the diagnostics
    assert L.c8_krylov_aggregates(asm.h, None, C.byref(ap)) == lib.C8_ERR_ARG and b"c8_krylov_aggregates" in L.c8_last_error()
    assert L.c8_krylov_coarse_matrix(asm.h, None, C.byref(n), None) == lib.C8_ERR_ARG and b"c8_krylov_coarse_matrix" in L.c8_last_error()
    with pytest.raises(ValueError):
        asm.set_krylov_preconditioner("multigrid")


# ---- 8. through the drivers -----------------------------------------------------------------------------------------------------------
def test_drivers_with_the_two_level_preconditioner():
    """the deck, comparison and tolerances of test_drivers_with_the_sgs_preconditioner"""
    from calibr8_amd import Assembler, PrimalDriver, adjoint_gradient, device_solver, scipy_solver
    from meshes import brick, jiggle
    from parity_cases import J2
    c, conn, sets = brick(3, 4, 3, 1.0, 1.5, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero),
            (0, 1, sets["ymax"], lambda x, y, z, t: 0.003 * t), (0, 0, sets["ymax"], zero)]
    act = [0, 1, 2, 3]

    def solve(device):
        asm = Assembler(8, c, conn, "small_J2", np.array(J2))
        asm.set_active(0, act)
        solver = device_solver(asm, preconditioner="two_level") if device else scipy_solver(asm)
        return PrimalDriver(asm, spec, max_iters=15, abs_tol=1e-12, rel_tol=1e-12, solver=solver).solve(3)

    dev, host = solve(True), solve(False)
    assert dev.asm.krylov_preconditioner == "two_level"
    grad, gref = adjoint_gradient(dev, len(act)), adjoint_gradient(host, len(act))
    s = dev.solver
    print("Newton %s / %s, linear solves %d, BiCGStab iterations %d, J %.16e / %.16e, gradient %s / %s" %
          (dev.newton_iters, host.newton_iters, s.solves, s.total_iters, dev.qoi(), host.qoi(), grad, gref))
    assert s.solves >= 3 + sum(n - 1 for n in dev.newton_iters) and s.total_iters > 0 and s.last.status == 0
    assert dev.newton_iters == host.newton_iters
    assert abs(dev.qoi() / host.qoi() - 1.0) < 1e-8
    assert np.abs(grad - gref).max() < 1e-7 * np.abs(gref).max()


if __name__ == "__main__":
    it, x = _solve_for_bytes()
    np.concatenate([[float(it)], x]).tofile(sys.argv[1])
