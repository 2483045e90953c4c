"""`-m gpu`: the multicolour node-block symmetric Gauss-Seidel preconditioner of the device solve
(c8_krylov_set_preconditioner) against its definition: the colouring and the operator are replayed in
numpy on the downloaded blocks; the solve meets the contract of the Jacobi-preconditioned one, takes at most half its
iterations, is reproducible bit for bit, and leaves the Jacobi path as it was."""
import contextlib
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the fresh process of test_sgs_solve_is_reproducible
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from test_gpu_krylov import REL_TOL, device_system, host_system, new_dx, raw_solve  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ["notched_bar", "jiggled_brick", "notch_tet4_hill", "notch2D_mechanics", "notch2D_plane_stress", "notched_bar_adjoint"]
JACOBI, SGS = 0, 1


@functools.lru_cache(maxsize=None)
def system(case):
    """device_system(case) and its host copy, built once per session; the tests leave the matrix and b as they are"""
    asm, ls = device_system(case)
    A, b = host_system(asm, ls)
    return asm, ls, A.tocsr(), b


def set_precond(asm, kind, sweeps=1):
    from calibr8_amd import lib
    lib.check(asm.L.c8_krylov_set_preconditioner(asm.h, kind, sweeps))


@contextlib.contextmanager
def precond(asm, kind, sweeps=1):
    """the preconditioner for the block; block Jacobi, the state the shared contexts of system() are kept in, afterwards --
    also when the block raises"""
    set_precond(asm, kind, sweeps)
    try:
        yield
    finally:
        set_precond(asm, JACOBI)


def adjoint_system(size):
    """K3 of notched_bar(*size) on the device: the adjoint system of test_gpu_krylov.device_system("notched_bar_adjoint"),
    assembled here for any mesh size (state, Dirichlet rows and parameters are those of that function)"""
    import torch
    from calibr8_amd import Assembler
    from meshes import fields_for, notched_bar, prescribed_fields
    from parity_cases import J2
    c, conn, s = notched_bar(*size)
    spec = [(0, d, s["xmin"]) for d in range(3)] + [(0, 0, s["xmax"])]
    asm = Assembler(8, c, conn, "small_J2", J2)
    u, p = fields_for(asm.ndims, *prescribed_fields(c, 0.004, ramp=True))
    U, P = asm.dev(u), asm.dev(p)
    Z, ZP = torch.zeros_like(U), torch.zeros_like(P)
    ls, xi = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(U, P, Z, ZP, asm.new_state(), xi, ls) == 0
    assert float(xi[:, :, -1].max()) > 0.0  # a plastic state
    ls.zero()
    g = torch.zeros(asm.nelems, asm.npts, asm.nloc, dtype=torch.float64, device=asm.device)
    f = torch.zeros(asm.nelems, asm.npts, asm.ndofs, dtype=torch.float64, device=asm.device)
    assert asm.adjoint_jacobian(U, P, Z, ZP, asm.new_state(), xi, g, f, ls) == 0
    dd = [(r, e, torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(np.zeros(len(n)))) for r, e, n in spec]
    asm.apply_dirichlet(dd, U, P, ls, is_adjoint=True)
    torch.cuda.synchronize()
    return asm, ls


def device_colors(asm):
    """c8_krylov_colors: list of node arrays, one per colour"""
    from calibr8_amd import lib
    nc, ptr, nodes = C.c_int32(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    lib.check(asm.L.c8_krylov_colors(asm.h, C.byref(nc), C.byref(ptr), C.byref(nodes)))
    cp = np.ctypeslib.as_array(ptr, shape=(nc.value + 1,)).copy()
    nd = np.ctypeslib.as_array(nodes, shape=(int(cp[-1]),)).copy() if cp[-1] else np.zeros(0, dtype=np.int32)
    assert cp[0] == 0 and (np.diff(cp) > 0).all()
    return [nd[cp[k]:cp[k + 1]] for k in range(nc.value)]


def greedy_colors(rowptr, colidx, n):
    """the rule of include/c8.h: nodes 0 .. n - 1 in ascending id over the sub-graph of these nodes, each takes the smallest
    colour that no already-coloured neighbour has"""
    color = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        nb = colidx[rowptr[i]:rowptr[i + 1]]
        used = set(color[nb[nb < i]].tolist())
        k = 0
        while k in used:
            k += 1
        color[i] = k
    return [np.nonzero(color == k)[0] for k in range(int(color.max()) + 1)] if n else []


def node_index(n, nd, nres, nloc=None):
    """idx[node, k]: position of equation k of the node in the flat vector (u segment, then p segment at nloc * nd)"""
    nloc = n if nloc is None else nloc
    nb = nd + (1 if nres == 2 else 0)
    idx = np.zeros((n, nb), dtype=np.int64)
    for k in range(nb):
        idx[:, k] = np.arange(n) * nd + k if k < nd else nloc * nd + np.arange(n)
    return idx


def block_inverses(A, idx):
    n, nb = idx.shape
    D = np.stack([np.asarray(A[idx[:, r]][:, idx[:, c]].diagonal()) for r in range(nb) for c in range(nb)], axis=1).reshape(n, nb, nb)
    return np.linalg.inv(D)


class Replay:
    """y = M^-1 v by the definition, in numpy.  Nodes of one colour do not couple, so a colour's nodes are updated at once
    from the x of before: the same numbers as one node after the other."""

    def __init__(self, A, idx, colors, sweeps=1):
        self.shape, self.idx, self.colors, self.sweeps = A.shape, idx, colors, sweeps
        self.Dinv = block_inverses(A, idx)
        self.rows = [idx[c].ravel() for c in colors]
        self.Ac = [A[r] for r in self.rows]

    def jacobi(self, v):
        out = np.zeros(v.shape)
        out[self.idx] = np.einsum("nij,nj->ni", self.Dinv, v[self.idx])
        return out

    def sgs(self, v):
        x = np.zeros(v.shape)   # (float64 whatever v is: SciPy probes an operator with an int8 vector)
        nc, nb = len(self.colors), self.idx.shape[1]
        for _ in range(self.sweeps):
            for k in list(range(nc)) + list(range(nc - 2, -1, -1)):
                r = (v[self.rows[k]] - self.Ac[k] @ x).reshape(-1, nb)
                x[self.rows[k]] += np.einsum("nij,nj->ni", self.Dinv[self.colors[k]], r).ravel()
        return x


def device_apply(asm, ls, v):
    """c8_krylov_precondition: (return code, y on the host)"""
    import torch
    n0 = asm.nnodes * asm.ndims
    vin = [asm.dev(np.ascontiguousarray(v[:n0])), asm.dev(np.ascontiguousarray(v[n0:]) if asm.nres == 2 else np.zeros(1))]
    y = [torch.full_like(vin[0], 7.0), torch.full_like(vin[1], 7.0)]
    sy = ls.c_struct()
    rc = asm.L.c8_krylov_precondition(asm.h, C.byref(sy), (C.c_void_p * 2)(vin[0].data_ptr(), vin[1].data_ptr()),
                                      (C.c_void_p * 2)(y[0].data_ptr(), y[1].data_ptr()))
    torch.cuda.synchronize()
    return rc, np.concatenate([y[i].cpu().numpy() for i in range(asm.nres)])


# ---- 1. colouring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(16, 4, 4), "jiggled_brick", "notch_tet4_hill", "notch2D_mechanics", "notch2D_plane_stress"])
def test_colouring_is_the_greedy_one(case):
    asm = system(case)[0]
    colors = device_colors(asm)
    rp, ci = asm.rowptr[1][1], asm.colidx[1][1]
    every = np.concatenate(colors)
    assert np.array_equal(np.sort(every), np.arange(asm.nnodes))            # every node in exactly one colour
    color_of = np.zeros(asm.nnodes, dtype=np.int64)
    for k, nodes in enumerate(colors):
        assert (np.diff(nodes) > 0).all()                                    # ascending
        color_of[nodes] = k
    rows = np.repeat(np.arange(asm.nnodes), np.diff(rp))
    off = rows != ci
    assert (color_of[rows[off]] != color_of[ci[off]]).all()                  # no neighbours share a colour
    ref = greedy_colors(rp, ci, asm.nnodes)
    print("%s: %d nodes, %d colours, sizes %s" % (case, asm.nnodes, len(colors), [len(c) for c in colors]))
    assert len(ref) == len(colors) and all(np.array_equal(a, b) for a, b in zip(ref, colors))


# ---- 2. the operator against its definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_operator_equals_its_definition(case):
    """|y - y_ref| / |y_ref| for a random v, SGS (1 and 2 sweeps) beside block Jacobi on the same system and with the same
    numpy block inverses: the two differ in the summation order inside a row only, hence the bound of 100 x the Jacobi figure
    beside the absolute one.  All three figures are printed."""
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    idx = node_index(asm.nnodes, asm.ndims, asm.nres)
    v = np.random.default_rng(11).standard_normal(len(b))
    colors = device_colors(asm)
    err = {}
    for name, kind, sweeps in (("jacobi", JACOBI, 1), ("sgs1", SGS, 1), ("sgs2", SGS, 2)):
        with precond(asm, kind, sweeps):
            assert asm.L.c8_krylov_get_preconditioner(asm.h) == kind
            rc, y = device_apply(asm, ls, v)
        assert rc == lib.C8_OK, asm.L.c8_last_error()
        rep = Replay(A, idx, colors, sweeps)
        y_ref = rep.jacobi(v) if kind == JACOBI else rep.sgs(v)
        err[name] = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
    print("%s: n %d colours %d operator error jacobi %.3e sgs(1) %.3e sgs(2) %.3e" % (case, len(b), len(colors), err["jacobi"], err["sgs1"], err["sgs2"]))
    for name in ("sgs1", "sgs2"):
        assert err[name] < 1e-10, err
        assert err[name] <= 100.0 * err["jacobi"], err


# ---- 3. the contract of the solve -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_sgs_solve_meets_the_contract(case):
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    with precond(asm, SGS):
        rc, info, x = raw_solve(asm, ls, new_dx(asm))
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    lu = spla.splu(A.tocsc())
    x_ref = lu.solve(b)
    inv_op = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    cond_est = spla.onenormest(A) * spla.onenormest(inv_op)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print("%s (SGS): n %d rc %d iters %d restarts %d host residual %.3e info %.3e cond_est %.3e x error %.3e" %
          (case, len(b), rc, info.iters, info.restarts, res, info.residual_norm / info.b_norm, cond_est, err))
    assert rc == lib.C8_OK and info.status == lib.C8_OK, asm.L.c8_last_error()
    assert res <= 1.01 * REL_TOL
    assert abs(info.residual_norm / np.linalg.norm(b - A @ x) - 1.0) < 1e-6
    assert abs(info.b_norm / np.linalg.norm(b) - 1.0) < 1e-12
    assert err <= cond_est * REL_TOL


# ---- 4. iteration counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 4, 4), (32, 8, 8)])
@pytest.mark.parametrize("adjoint", [False, True])
def test_iteration_counts(size, adjoint):
    """Device SGS <= 2 x SciPy BiCGStab with the numpy SGS operator (the rule of test_iteration_counts_beside_scipy_bicgstab)
    and <= half the device count with block Jacobi (CPU ratios 3.6 and 7.5 on K1), on K1 and on the adjoint system K3."""
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    if adjoint:
        asm, ls = adjoint_system(size)
        A, b = host_system(asm, ls)
        A = A.tocsr()
    else:
        asm, ls, A, b = system(size)
    with precond(asm, JACOBI):
        rcj, ij, _ = raw_solve(asm, ls, new_dx(asm))
    with precond(asm, SGS):
        rcs, isg, _ = raw_solve(asm, ls, new_dx(asm))
    colors = device_colors(asm)
    rep = Replay(A, node_index(asm.nnodes, asm.ndims, asm.nres), colors)
    count = [0]

    def cb(_):
        count[0] += 1
    xs, flag = spla.bicgstab(A, b, rtol=REL_TOL, atol=0.0, maxiter=20000, M=spla.LinearOperator(A.shape, matvec=rep.sgs), callback=cb)
    print("notched_bar%s %s: unknowns %d colours %d device iterations SGS %d (restarts %d) Jacobi %d (restarts %d), SciPy BiCGStab with SGS %d (flag %d)" %
          (size, "K3 (adjoint)" if adjoint else "K1", len(b), len(colors), isg.iters, isg.restarts, ij.iters, ij.restarts, count[0], flag))
    assert rcj == lib.C8_OK and rcs == lib.C8_OK, asm.L.c8_last_error()
    assert flag == 0
    assert isg.iters <= 2 * count[0]
    assert 2 * isg.iters <= ij.iters


# ---- 5. reproducible ------------------------------------------------------------------------------------------------------------
def _solve_for_bytes():
    asm, ls = device_system((16, 4, 4))
    set_precond(asm, SGS, 1)
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == 0
    return info.iters, x


def test_sgs_solve_is_reproducible(tmp_path):
    asm, ls = system((16, 4, 4))[:2]
    with precond(asm, SGS):
        rc1, i1, x1 = raw_solve(asm, ls, new_dx(asm))
        rc2, i2, x2 = raw_solve(asm, ls, new_dx(asm))
    assert rc1 == 0 and rc2 == 0
    assert i1.iters == i2.iters and x1.tobytes() == x2.tobytes()
    out = str(tmp_path / "x.bin")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), out])
    raw = np.fromfile(out)
    assert int(raw[0]) == i1.iters and raw[1:].tobytes() == x1.tobytes()


# ---- 6. refusals and state ------------------------------------------------------------------------------------------------------
def test_refusals_and_state():
    from calibr8_amd import lib
    asm, ls = device_system((16, 4, 4))   # a context of its own: the matrix is changed below
    L = asm.L
    assert L.c8_krylov_get_preconditioner(asm.h) == lib.C8_PRECOND_BLOCK_JACOBI      # the default of c8_create
    for kind in (2, -1, 99):
        assert L.c8_krylov_set_preconditioner(asm.h, kind, 1) == lib.C8_ERR_ARG
        assert b"c8_krylov_set_preconditioner" in L.c8_last_error()
        assert L.c8_krylov_get_preconditioner(asm.h) == lib.C8_PRECOND_BLOCK_JACOBI  # a refused call changes nothing
    assert L.c8_krylov_set_preconditioner(asm.h, lib.C8_PRECOND_BLOCK_SGS, 0) == lib.C8_OK   # sweeps <= 0: one sweep
    assert L.c8_krylov_get_preconditioner(asm.h) == lib.C8_PRECOND_BLOCK_SGS
    A, b = host_system(asm, ls)
    v = np.random.default_rng(5).standard_normal(len(b))
    rc0, y0 = device_apply(asm, ls, v)
    set_precond(asm, SGS, 1)
    rc1, y1 = device_apply(asm, ls, v)
    assert rc0 == 0 and rc1 == 0 and y0.tobytes() == y1.tobytes()
    rc, info_s, xs = raw_solve(asm, ls, new_dx(asm))
    assert rc == lib.C8_OK
    # back to Jacobi: the bytes of a context that never switched
    set_precond(asm, JACOBI)
    assert asm.krylov_preconditioner == "jacobi"
    rc, info_a, xa = raw_solve(asm, ls, new_dx(asm))
    asm_b, ls_b = device_system((16, 4, 4))
    rc_b, info_b, xb = raw_solve(asm_b, ls_b, new_dx(asm_b))
    assert rc == lib.C8_OK and rc_b == lib.C8_OK
    assert info_a.iters == info_b.iters and xa.tobytes() == xb.tobytes()
    assert info_s.iters < info_a.iters
    # the Python setter
    asm.set_krylov_preconditioner("sgs", 2)
    assert asm.krylov_preconditioner == "sgs"
    with pytest.raises(ValueError):
        asm.set_krylov_preconditioner("ilu")
    # null arguments of the apply
    sy = ls.c_struct()
    dx = new_dx(asm)
    ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
    assert L.c8_krylov_precondition(asm.h, C.byref(sy), None, ptrs) == lib.C8_ERR_ARG
    assert L.c8_krylov_precondition(asm.h, C.byref(sy), ptrs, (C.c_void_p * 2)(dx[0].data_ptr(), None)) == lib.C8_ERR_ARG
    assert b"c8_krylov_precondition" in L.c8_last_error()
    # a vector that is not finite
    vbad = v.copy()
    vbad[3] = np.nan
    rc, _ = device_apply(asm, ls, vbad)
    assert rc == lib.C8_ERR_ARG and b"not finite" in L.c8_last_error()
    # one node's diagonal block zeroed: refused by the solve and by the apply, the node is named
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
    rc, _ = device_apply(asm, ls, v)
    assert rc == lib.C8_ERR_ARG and ("node %d " % node).encode() in L.c8_last_error(), L.c8_last_error()


# ---- 7. through the drivers -------------------------------------------------------------------------------------------------------
def test_drivers_with_the_sgs_preconditioner():
    """the deck, comparison and tolerances of test_adjoint_gradient_with_the_device_solver and of
    test_reference_decks_with_the_device_solver"""
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
        solver = device_solver(asm, preconditioner="sgs") if device else scipy_solver(asm)
        return PrimalDriver(asm, spec, max_iters=15, abs_tol=1e-12, rel_tol=1e-12, solver=solver).solve(3)

    dev, host = solve(True), solve(False)
    assert dev.asm.krylov_preconditioner == "sgs"
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
