"""`-m gpu`: the multilevel preconditioner of the device solve (C8_PRECOND_MULTILEVEL) against its
definition in include/c8.h: the levels, their aggregates and colours, every A_l = P^T A P and the operator are replayed in
numpy from the downloaded blocks and the coordinates; with two levels it is the two-level kind; the solve meets the
contract of the other kinds, solves a mesh the two-level kind refuses, is reproducible bit for bit and leaves the other
kinds as they were."""
import contextlib
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the fresh process of test_multilevel_solve_is_reproducible
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from test_gpu_krylov import REL_TOL, device_system, host_system, new_dx, raw_solve, system_case  # noqa: E402
from test_gpu_krylov_sgs import (CASES, JACOBI, SGS, adjoint_system, device_apply, device_colors, greedy_colors, node_index,  # noqa: E402
                                 precond, set_precond, system)
from test_gpu_krylov_two_level import COARSE_CAP, TWO_LEVEL, ReplayFrom, aggregate_replay, coarse_replay, prolongator  # noqa: E402

pytestmark = pytest.mark.gpu
MULTILEVEL = 5  # C8_PRECOND_MULTILEVEL (2 and 4 are no kinds)
EPS = np.finfo(np.float64).eps


def set_levels(asm, coarse_max=0, max_levels=0):
    from calibr8_amd import lib
    lib.check(asm.L.c8_krylov_set_multilevel(asm.h, coarse_max, max_levels))


@contextlib.contextmanager
def multilevel(asm, coarse_max=0, max_levels=0, sweeps=1):
    """the multilevel kind with these settings for the block; block Jacobi and the default settings, the state the shared
    contexts of system() are kept in, afterwards"""
    set_levels(asm, coarse_max, max_levels)
    set_precond(asm, MULTILEVEL, sweeps)
    try:
        yield
    finally:
        set_precond(asm, JACOBI)
        set_levels(asm)


def coarse_columns(asm):
    return asm.ndims + (3 if asm.ndims == 3 else 1) + (1 if asm.nres == 2 else 0)


# ---- the device's levels ----------------------------------------------------------------------------------------------------
def device_levels(asm):
    """c8_krylov_levels / c8_krylov_level: [(nodes, aggregate of every node or None, [nodes of colour k])] per level"""
    from calibr8_amd import lib
    nl = C.c_int32()
    lib.check(asm.L.c8_krylov_levels(asm.h, C.byref(nl)))
    out = []
    for lev in range(nl.value):
        n, ncol = C.c_int32(), C.c_int32()
        ap, cp, nd = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        lib.check(asm.L.c8_krylov_level(asm.h, lev, C.byref(n), C.byref(ap), C.byref(ncol), C.byref(cp), C.byref(nd)))
        agg = np.ctypeslib.as_array(ap, shape=(n.value,)).astype(np.int64) if ap else None
        colors = []
        if ncol.value:
            ptr = np.ctypeslib.as_array(cp, shape=(ncol.value + 1,)).copy()
            nodes = np.ctypeslib.as_array(nd, shape=(int(ptr[-1]),)).copy()
            colors = [nodes[ptr[k]:ptr[k + 1]] for k in range(ncol.value)]
        out.append((n.value, agg, colors))
    return out


def device_level_matrix(asm, ls, level):
    from calibr8_amd import lib
    n = C.c_int32()
    sy = ls.c_struct()
    lib.check(asm.L.c8_krylov_level_matrix(asm.h, C.byref(sy), level, C.byref(n), None))
    out = np.full((n.value, n.value), 7.0)
    lib.check(asm.L.c8_krylov_level_matrix(asm.h, C.byref(sy), level, C.byref(n), out.ctypes.data_as(lib.dp)))
    return out


# ---- the definition in numpy ------------------------------------------------------------------------------------------------
def next_graph(rp, ci, agg, nagg):
    """graph of the next level: I and J are neighbours when a node of I is a neighbour of a node of J (self included)"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    pairs = np.unique(agg[rows] * nagg + agg[ci])
    return np.concatenate([[0], np.cumsum(np.bincount(pairs // nagg, minlength=nagg))]), pairs % nagg


def centroids(x, agg, nagg):
    """unweighted mean of the members' positions, summed in ascending id"""
    out = np.zeros((nagg, x.shape[1]))
    for a in range(nagg):
        nodes = np.nonzero(agg == a)[0]
        out[a] = np.cumsum(x[nodes], axis=0)[-1] / len(nodes)
    return out


def levels_replay(asm, coarse_max, max_levels):
    """the levels of include/c8.h from the node graph and the coordinates: a list of dicts n, rp, ci, x and, where a level
    below exists, agg, nagg, colors.  Level 1 always exists."""
    nc = coarse_columns(asm)
    levels = [dict(n=asm.nnodes, rp=np.asarray(asm.rowptr[1][1]), ci=np.asarray(asm.colidx[1][1]), x=np.asarray(asm.coords)[:, :asm.ndims])]
    while True:
        cur = levels[-1]
        if len(levels) >= 2 and (cur["n"] * nc <= coarse_max or len(levels) >= max_levels):
            break
        agg, nagg = aggregate_replay(cur["rp"], cur["ci"], cur["n"])
        if len(levels) >= 2 and nagg >= cur["n"]:
            break
        cur.update(agg=agg, nagg=nagg, colors=greedy_colors(cur["rp"], cur["ci"], cur["n"]))
        rp, ci = next_graph(cur["rp"], cur["ci"], agg, nagg)
        levels.append(dict(n=nagg, rp=rp, ci=ci, x=centroids(cur["x"], agg, nagg)))
    return levels


def level_prolongator(Al, x, agg, nagg, nd, nc):
    """P_l, l >= 1, dense: per node the identity plus rotation m -> translation e_m x d (2-D (-d_y, d_x)), d = x_a -
    centroid; the rows of the constrained equations of A_l (every off-diagonal entry exactly 0) are zero"""
    n = len(agg)
    d = x - centroids(x, agg, nagg)[agg]
    P = np.zeros((n * nc, nagg * nc))
    for a in range(n):
        B = np.eye(nc)
        if nd == 3:
            for m in range(3):
                B[:3, 3 + m] = np.cross(np.eye(3)[m], d[a])
        else:
            B[0, 2], B[1, 2] = -d[a, 1], d[a, 0]
        P[a * nc:(a + 1) * nc, agg[a] * nc:(agg[a] + 1) * nc] = B
    off = Al.copy()
    np.fill_diagonal(off, 0.0)
    P[~off.any(axis=1)] = 0.0
    return P


class Multilevel:
    """the levels, every P_l and A_l, and y = M^-1 v of the definition, in numpy"""

    def __init__(self, asm, A, coarse_max, max_levels, sweeps=1):
        import scipy.linalg as sl
        import scipy.sparse as sp
        nd, nc = asm.ndims, coarse_columns(asm)
        self.levels = levels_replay(asm, coarse_max, max_levels)
        last = len(self.levels) - 1
        self.P = [prolongator(asm, A, self.levels[0]["agg"], self.levels[0]["nagg"])]
        self.A = [A, coarse_replay(A, self.P[0])]                 # A_l, dense arrays for l >= 1
        self.rep = [ReplayFrom(A, node_index(asm.nnodes, nd, asm.nres), self.levels[0]["colors"], sweeps)]
        for lev in range(1, last):
            L, Al = self.levels[lev], self.A[lev]
            P = sp.csr_matrix(level_prolongator(Al, L["x"], L["agg"], L["nagg"], nd, nc))
            self.P.append(P)
            self.A.append(coarse_replay(sp.csr_matrix(Al), P))
            self.rep.append(ReplayFrom(sp.csr_matrix(Al), np.arange(L["n"] * nc).reshape(L["n"], nc), L["colors"], sweeps))
        self.lu = sl.lu_factor(self.A[last])
        # what the device inverts: the last level and the diagonal blocks of every other one
        self.cond_last = np.linalg.cond(self.A[last])
        self.cond_blocks = max(float(np.linalg.cond(r.Dinv).max()) for r in self.rep)
        self.cond = max(self.cond_last, self.cond_blocks)

    def set_sweeps(self, sweeps):
        for r in self.rep:
            r.sweeps = sweeps

    def apply(self, v, lev=0):
        import scipy.linalg as sl
        v = np.asarray(v, dtype=np.float64)
        if lev == len(self.levels) - 1:
            return sl.lu_solve(self.lu, v)
        return self.rep[lev].sgs_from(v, self.P[lev] @ self.apply(self.P[lev].T @ v, lev + 1))


FORCED = {3: (1, 3), 4: (1, 4)}   # levels wanted -> (coarse_max, max_levels): recursion as far as max_levels lets it go


@functools.lru_cache(maxsize=None)
def replay(case, nlev):
    """the numpy hierarchy and operator (one sweep) of system(case) with `nlev` levels forced, built once per session"""
    asm, ls, A, b = system(case)
    return Multilevel(asm, A, *FORCED[nlev])


# ---- 1. the hierarchy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,coarse_max,want", [((16, 4, 4), 100, [395, 24, 2]), ((32, 8, 8), 100, [2385, 93, 5]), ((32, 8, 8), 20, [2385, 93, 5, 2]),
                                                  ("jiggled_brick", 100, None), ("notch_tet4_hill", 100, None),
                                                  ("notch2D_mechanics", 20, None), ("notch2D_plane_stress", 20, None)])
def test_levels_aggregates_and_colours_are_those_of_the_rules(case, coarse_max, want):
    """`want`: the node counts of the numpy replay recorded in the issue (not from the device)"""
    asm = system(case)[0]
    ref = levels_replay(asm, coarse_max, 8)
    with multilevel(asm, coarse_max):
        dev = device_levels(asm)
    print("%s coarse_max %d: nodes per level %s, colours per level %s" % (case, coarse_max, [d[0] for d in dev], [len(d[2]) for d in dev]))
    assert [L["n"] for L in ref] == [d[0] for d in dev]
    if want is not None:
        assert [L["n"] for L in ref] == want
    assert len(dev) >= 3 and [d[0] for d in dev] == sorted([d[0] for d in dev], reverse=True)
    for lev, (L, (n, agg, colors)) in enumerate(zip(ref, dev)):
        if lev == len(dev) - 1:
            assert agg is None and colors == []                                 # the dense level
            continue
        assert np.array_equal(agg, L["agg"]) and agg.max() == L["nagg"] - 1
        assert len(colors) == len(L["colors"]) and all(np.array_equal(a, b) for a, b in zip(colors, L["colors"]))
    assert all(np.array_equal(a, b) for a, b in zip(dev[0][2], device_colors(asm)))   # level 0: the lists of the SGS kind


# ---- 2. the matrices --------------------------------------------------------------------------------------------------------
def check_matrices(case, nlev):
    asm, ls, A, b = system(case)
    rep = replay(case, nlev)
    with multilevel(asm, *FORCED[nlev]):
        got = [device_level_matrix(asm, ls, lev) for lev in range(1, len(rep.levels))]
    for lev, Ad in enumerate(got, start=1):
        err = np.linalg.norm(Ad - rep.A[lev]) / np.linalg.norm(rep.A[lev])
        print("%s, %d levels: level %d n %d |A_l - P^T A P|_F / |P^T A P|_F %.3e" % (case, len(rep.levels), lev, Ad.shape[0], err))
        assert Ad.shape == rep.A[lev].shape
        assert err < 1e-12
    return len(rep.levels)


@pytest.mark.parametrize("case", CASES)
def test_level_matrices_equal_pt_a_p(case):
    assert check_matrices(case, 3) == 3


def test_level_matrices_equal_pt_a_p_with_four_levels():
    assert check_matrices("notched_bar", 4) == 4


# ---- 3. the operator against its definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [3, 4])
@pytest.mark.parametrize("case", CASES)
def test_operator_equals_its_definition(case, nlev):
    """|y - y_ref| / |y_ref| <= 100 eps max cond over what the device inverts: the last level (an explicit inverse against
    numpy's LU solve) and the diagonal blocks of every other level (Gauss-Jordan against numpy's inverse); every other step
    differs in the order of sums only -- the reasoning of the two-level test.  The larger figure, max_l cond(A_l) over the
    whole matrices, is printed beside it and not used."""
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    base = replay(case, nlev)
    bound = 100.0 * EPS * base.cond
    whole = max(np.linalg.cond(Al) for Al in base.A[1:])
    v = np.random.default_rng(17).standard_normal(len(b))
    for sweeps in (1, 2):
        with multilevel(asm, *FORCED[nlev], sweeps=sweeps):
            assert asm.L.c8_krylov_get_preconditioner(asm.h) == MULTILEVEL
            rc, y = device_apply(asm, ls, v)
        assert rc == lib.C8_OK, asm.L.c8_last_error()
        base.set_sweeps(sweeps)
        y_ref = base.apply(v)
        base.set_sweeps(1)
        err = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
        print("%s: n %d levels %s cond(last) %.3e cond(blocks) %.3e [max cond(A_l) %.3e] sweeps %d operator error %.3e bound %.3e" %
              (case, len(b), [L["n"] for L in base.levels], base.cond_last, base.cond_blocks, whole, sweeps, err, bound))
        assert err <= bound


# ---- 4. two levels are the two-level kind -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_two_levels_are_the_two_level_kind(case):
    """max_levels = 2: the two kinds run one set-up and one apply on lists of one level with the same numbers, so the
    operator and the solve agree to the byte -- equal bytes of y = M^-1 v and of dx, equal iteration counts -- as the two
    kinds over parts do (test_two_levels_over_parts_are_the_two_level_kind_over_parts)"""
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    v = np.random.default_rng(19).standard_normal(len(b))
    with precond(asm, TWO_LEVEL):
        rc2, y2 = device_apply(asm, ls, v)
        rcs2, info2, x2 = raw_solve(asm, ls, new_dx(asm))
    with multilevel(asm, 0, 2):
        assert len(device_levels(asm)) == 2
        rcm, ym = device_apply(asm, ls, v)
        rcsm, infom, xm = raw_solve(asm, ls, new_dx(asm))
    assert rc2 == rcm == rcs2 == rcsm == lib.C8_OK, asm.L.c8_last_error()
    print("%s: multilevel(max_levels=2) against two-level: operator difference %.3e, dx difference %.3e, iterations %d / %d" %
          (case, np.linalg.norm(ym - y2) / np.linalg.norm(y2), np.linalg.norm(xm - x2) / np.linalg.norm(x2), infom.iters, info2.iters))
    assert ym.tobytes() == y2.tobytes()
    assert xm.tobytes() == x2.tobytes()
    assert infom.iters == info2.iters


# ---- 5. the contract of the solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_multilevel_solve_meets_the_contract(case):
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    asm, ls, A, b = system(case)
    with multilevel(asm, *FORCED[3]):
        nlev = len(device_levels(asm))
        rc, info, x = raw_solve(asm, ls, new_dx(asm))
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    lu = spla.splu(A.tocsc())
    x_ref = lu.solve(b)
    inv_op = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    cond_est = spla.onenormest(A) * spla.onenormest(inv_op)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print("%s (multilevel, %d levels): n %d rc %d iters %d restarts %d host residual %.3e info %.3e cond_est %.3e x error %.3e" %
          (case, nlev, len(b), rc, info.iters, info.restarts, res, info.residual_norm / info.b_norm, cond_est, err))
    assert nlev == 3
    assert rc == lib.C8_OK and info.status == lib.C8_OK, asm.L.c8_last_error()
    assert info.iters > 0 and info.b_norm > 0.0
    assert res <= 1.01 * REL_TOL
    assert abs(info.residual_norm / np.linalg.norm(b - A @ x) - 1.0) < 1e-6
    assert abs(info.b_norm / np.linalg.norm(b) - 1.0) < 1e-12
    assert err <= cond_est * REL_TOL


# ---- 6. beyond the cap of the two-level kind ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_brick():
    """brick(36,36,36) assembled as device_system assembles the jiggled brick: same state, same Dirichlet rows; the jiggle is
    0.01, the 0.03 of brick(12,12,12) scaled with the element size (0.03 is more than an element of this mesh)"""
    import torch
    from calibr8_amd import Assembler
    from meshes import brick, fields_for, jiggle, prescribed_fields
    from parity_cases import J2
    c, conn, s = brick(36, 36, 36)
    c = jiggle(c, s, 0.01)
    spec = [(0, d, s["xmin"]) for d in range(3)] + [(0, 0, s["xmax"])]
    asm = Assembler(8, c, conn, "small_J2", J2)
    u, p = fields_for(asm.ndims, *prescribed_fields(c, 0.004, ramp=True))
    U, P = asm.dev(u), asm.dev(p)
    Z, ZP = torch.zeros_like(U), torch.zeros_like(P)
    ls, xi = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(U, P, Z, ZP, asm.new_state(), xi, ls) == 0
    dd = [(r, e, torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(np.zeros(len(n)))) for r, e, n in spec]
    asm.apply_dirichlet(dd, U, P, ls, is_adjoint=False)
    torch.cuda.synchronize()
    return asm, ls


def test_solves_the_mesh_the_two_level_kind_refuses():
    """default settings; the residual from the downloaded matrix; at most half the iterations of the device SGS solve"""
    from calibr8_amd import lib
    asm, ls = big_brick()
    with precond(asm, TWO_LEVEL):
        rc2, info2, _ = raw_solve(asm, ls, new_dx(asm))
    assert rc2 == lib.C8_ERR_UNSUPPORTED and info2.iters == 0 and b"8192" in asm.L.c8_last_error()
    with precond(asm, SGS):
        rcs, infos, _ = raw_solve(asm, ls, new_dx(asm))
    with multilevel(asm):
        nodes = [d[0] for d in device_levels(asm)]
        rc, info, x = raw_solve(asm, ls, new_dx(asm))
    A, b = host_system(asm, ls)
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("brick(36,36,36): unknowns %d nodes per level %s iterations multilevel %d (restarts %d) SGS %d, host residual %.3e" %
          (len(b), nodes, info.iters, info.restarts, infos.iters, res))
    assert nodes[1] * 7 > COARSE_CAP and len(nodes) >= 3
    assert rc == lib.C8_OK and rcs == lib.C8_OK and info.status == lib.C8_OK, asm.L.c8_last_error()
    assert res <= 1.01 * REL_TOL
    assert 2 * info.iters <= infos.iters


# ---- 7. iteration counts ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts(size, adjoint):
    """(device multilevel, device SGS, SciPy BiCGStab with the numpy operator) on K1 / K3 of notched_bar(*size), coarse_max 100"""
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
    with multilevel(asm, 100):
        rcm, iml, _ = raw_solve(asm, ls, new_dx(asm))
    op = Multilevel(asm, A, 100, 8)
    count = [0]

    def cb(_):
        count[0] += 1
    xs, flag = spla.bicgstab(A, b, rtol=REL_TOL, atol=0.0, maxiter=20000, M=spla.LinearOperator(A.shape, matvec=op.apply), callback=cb)
    print("notched_bar%s %s: unknowns %d nodes per level %s device iterations multilevel %d (restarts %d) SGS %d (restarts %d), "
          "SciPy BiCGStab with the multilevel operator %d (flag %d)" %
          (size, "K3 (adjoint)" if adjoint else "K1", len(b), [L["n"] for L in op.levels], iml.iters, iml.restarts, isg.iters, isg.restarts, count[0], flag))
    assert rcs == lib.C8_OK and rcm == lib.C8_OK, asm.L.c8_last_error()
    assert flag == 0
    return iml.iters, isg.iters, count[0]


@pytest.mark.parametrize("size", [(16, 4, 4), (32, 8, 8)])
def test_iteration_counts(size):
    """K1: device multilevel <= 2 x SciPy BiCGStab with the numpy operator (the project's margin) and <= half the device
    count with Gauss-Seidel (the CPU replay gives 24 against 79 and 36 against 175)"""
    ml, sgs, scipy_ml = counts(size, False)
    assert ml <= 2 * scipy_ml
    assert 2 * ml <= sgs


def test_iteration_counts_of_the_adjoint_system_are_recorded():
    """K3 on (16,4,4): no CPU replay of K3 with three levels backs a bound, so the counts are printed (DESIGN.md section
    13e records them) and only the solves' success is asserted (inside counts)"""
    ml, sgs, scipy_ml = counts((16, 4, 4), True)
    assert ml > 0 and sgs > 0 and scipy_ml > 0


# ---- 8. reproducible ------------------------------------------------------------------------------------------------------------------
def _solve_for_bytes():
    asm, ls = device_system((16, 4, 4))
    set_levels(asm, 100)
    set_precond(asm, MULTILEVEL, 1)
    rc, info, x = raw_solve(asm, ls, new_dx(asm))
    assert rc == 0
    return info.iters, x


def test_multilevel_solve_is_reproducible(tmp_path):
    asm, ls = system((16, 4, 4))[:2]
    with multilevel(asm, 100):
        rc1, i1, x1 = raw_solve(asm, ls, new_dx(asm))
        rc2, i2, x2 = raw_solve(asm, ls, new_dx(asm))
    assert rc1 == 0 and rc2 == 0
    assert i1.iters == i2.iters and x1.tobytes() == x2.tobytes()
    out = str(tmp_path / "x.bin")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), out])
    raw = np.fromfile(out)
    assert int(raw[0]) == i1.iters and raw[1:].tobytes() == x1.tobytes()


# ---- 9. state and refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [JACOBI, SGS, TWO_LEVEL])
def test_switching_kinds_leaves_the_other_kinds_as_they_were(other):
    from calibr8_amd import lib
    asm, ls = device_system((16, 4, 4))
    assert asm.L.c8_krylov_get_preconditioner(asm.h) == JACOBI and asm.krylov_preconditioner == "jacobi"   # the default
    set_precond(asm, other)
    asm.set_krylov_multilevel(coarse_max=100)
    asm.set_krylov_preconditioner("multilevel", 0)          # sweeps <= 0: one sweep
    assert asm.L.c8_krylov_get_preconditioner(asm.h) == lib.C8_PRECOND_MULTILEVEL == MULTILEVEL
    assert asm.krylov_preconditioner == "multilevel"
    rc, info_m, xm = raw_solve(asm, ls, new_dx(asm))
    assert rc == lib.C8_OK and len(device_levels(asm)) == 3
    set_precond(asm, other)
    rc, info_a, xa = raw_solve(asm, ls, new_dx(asm))
    asm_b, ls_b = device_system((16, 4, 4))                 # a context that never switched
    set_precond(asm_b, other)
    rc_b, info_b, xb = raw_solve(asm_b, ls_b, new_dx(asm_b))
    assert rc == lib.C8_OK and rc_b == lib.C8_OK
    assert info_a.iters == info_b.iters and xa.tobytes() == xb.tobytes()


def test_changing_coarse_max_rebuilds_the_levels():
    from calibr8_amd import lib
    asm, ls = system((32, 8, 8))[:2]
    v = np.random.default_rng(23).standard_normal(asm.nnodes * 4)
    with multilevel(asm, 100):
        n3 = [d[0] for d in device_levels(asm)]
        rc3, y3 = device_apply(asm, ls, v)
        set_levels(asm, 20)
        n4 = [d[0] for d in device_levels(asm)]
        rc4, y4 = device_apply(asm, ls, v)
        set_levels(asm, 100)
        rc5, y5 = device_apply(asm, ls, v)
    assert rc3 == rc4 == rc5 == lib.C8_OK
    assert n3 == [2385, 93, 5] and n4 == [2385, 93, 5, 2]
    assert y3.tobytes() != y4.tobytes() and y3.tobytes() == y5.tobytes()


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
    set_precond(asm, MULTILEVEL)
    ls = asm.new_linsys()
    sy = ls.c_struct()
    dx = new_dx(asm)
    ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
    info = lib.KrylovInfo()
    n, ncol, ap, cp, nd = C.c_int32(), C.c_int32(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    for rc in (L.c8_krylov_solve_parts(asm.h, C.byref(sy), ptrs, None, C.byref(info)),
               L.c8_krylov_precondition(asm.h, C.byref(sy), ptrs, ptrs),
               L.c8_krylov_levels(asm.h, C.byref(n)),
               L.c8_krylov_level(asm.h, 0, C.byref(n), C.byref(ap), C.byref(ncol), C.byref(cp), C.byref(nd)),
               L.c8_krylov_level_matrix(asm.h, C.byref(sy), 1, C.byref(n), None)):
        assert rc == lib.C8_ERR_UNSUPPORTED and b"halo" in L.c8_last_error() and b"multilevel" in L.c8_last_error(), L.c8_last_error()
    assert info.status == lib.C8_ERR_UNSUPPORTED and info.iters == 0
    torch.cuda.synchronize()
    halo.close()
    comm.close()
    # max_levels = 2 on brick(36,36,36): the last level is above the cap; refused before anything is read or iterated
    c, conn, s = brick(36, 36, 36)
    big = Assembler(8, c, conn, "small_J2", J2)
    big.set_krylov_multilevel(max_levels=2)
    big.set_krylov_preconditioner("multilevel")
    nodes = [d[0] for d in device_levels(big)]              # (reported above the cap too)
    assert len(nodes) == 2 and nodes[1] * 7 > COARSE_CAP
    lsb = big.new_linsys()
    rc, info, x = raw_solve(big, lsb, new_dx(big))
    msg = L.c8_last_error()
    assert rc == lib.C8_ERR_UNSUPPORTED and info.status == lib.C8_ERR_UNSUPPORTED and info.iters == 0
    assert ("n = %d" % (nodes[1] * 7)).encode() in msg and b"8192" in msg and b"max_levels = 2" in msg, msg
    rc, _ = device_apply(big, lsb, np.ones(big.nnodes * 4))
    assert rc == lib.C8_ERR_UNSUPPORTED and b"8192" in L.c8_last_error()
    syb = lsb.c_struct()
    assert L.c8_krylov_level_matrix(big.h, C.byref(syb), 1, C.byref(n), None) == lib.C8_ERR_UNSUPPORTED
    # one node's diagonal block zeroed: the node is named, as with the other kinds
    asm, ls = device_system((16, 4, 4))
    set_levels(asm, 100)
    set_precond(asm, MULTILEVEL)
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
    # 2, 4 and the value after the last kind are unknown kinds; a refused call changes nothing
    for kind in (2, 4, 6):
        assert L.c8_krylov_set_preconditioner(asm.h, kind, 1) == lib.C8_ERR_ARG and b"unknown preconditioner" in L.c8_last_error()
        assert L.c8_krylov_get_preconditioner(asm.h) == MULTILEVEL
    assert L.c8_krylov_set_multilevel(asm.h, 0, 1) == lib.C8_ERR_ARG and b"max_levels" in L.c8_last_error()
    assert L.c8_krylov_level_matrix(asm.h, C.byref(ls.c_struct()), 0, C.byref(n), None) == lib.C8_ERR_ARG     # level 0 is the system
    # the setter during a staged assembly that waits for gather_finish
    with pytest.raises(ValueError):
        asm.set_krylov_preconditioner("multigrid")


def test_setter_is_refused_while_a_staged_assembly_waits():
    """the set-up of test_gpu_krylov.py::test_contract_of_the_refusals for c8_krylov_set_preconditioner"""
    import torch
    from calibr8_amd import Assembler, lib
    from meshes import brick, fields_for, prescribed_fields
    from parity_cases import J2
    c, conn, s = brick(4, 4, 4)
    asm = Assembler(8, c, conn, "small_J2", J2, scatter="gather")
    u, p = fields_for(asm.ndims, *prescribed_fields(c, 0.004, ramp=True))
    U, P = asm.dev(u), asm.dev(p)
    Z, ZP = torch.zeros_like(U), torch.zeros_like(P)
    ls, xi = asm.new_linsys(), asm.new_state()
    asm.set_gather_early_nodes(0, asm.nnodes // 2)
    assert asm.forward_jacobian(U, P, Z, ZP, asm.new_state(), xi, ls) == 0
    try:
        assert asm.L.c8_krylov_set_multilevel(asm.h, 100, 3) == lib.C8_ERR_ARG
        assert b"c8_krylov_set_multilevel" in asm.L.c8_last_error() and b"staged assembly" in asm.L.c8_last_error()
    finally:
        asm.gather_finish()
    torch.cuda.synchronize()
    assert asm.L.c8_krylov_set_multilevel(asm.h, 100, 3) == lib.C8_OK


# ---- 10. through the drivers ------------------------------------------------------------------------------------------------------------
def test_drivers_with_the_multilevel_preconditioner():
    """the deck, comparison and tolerances of test_drivers_with_the_two_level_preconditioner, three levels forced"""
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
        if device:
            asm.set_krylov_multilevel(coarse_max=1, max_levels=3)
        solver = device_solver(asm, preconditioner="multilevel") if device else scipy_solver(asm)
        return PrimalDriver(asm, spec, max_iters=15, abs_tol=1e-12, rel_tol=1e-12, solver=solver).solve(3)

    dev, host = solve(True), solve(False)
    assert dev.asm.krylov_preconditioner == "multilevel" and len(device_levels(dev.asm)) == 3
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
