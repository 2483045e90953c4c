"""`-m gpu`: the three small kernels that every Newton and adjoint step goes through -- k_traction, k_dirichlet and k_spmv
of c8_primal.hip, behind c8_apply_traction, c8_apply_dirichlet and c8_apply_A -- entry by entry against the long double
restatements of bc_ref.py (the bound and its counts are derived there), on warped quad4 faces, at the edges of the
256-thread block, on overlapping and empty node sets, on high-degree rows and on the 2-D and one-residual systems; then a
hex8 solve driven by a quad4 traction against the oracle-driven host driver, and a patch test.  Blocking calls on the
context's own stream throughout; every index handed to the device is a valid node of its mesh."""
import ctypes as C
import functools

import numpy as np
import pytest

import bc_ref as R
import oracle_lib as ol
from fe_driver import Dbc, Primal, Tbc
from meshes import brick, jiggle, pinched_bricks, tri_mesh

pytestmark = pytest.mark.gpu
LD = np.longdouble
J2 = [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0]
HILL_PS = [1000.0, 0.25, 2.0, 10.0, 2.0, 1.0, 1.0, 1.0, 1.0]
MODEL = {8: ("small_J2", J2), 4: ("elastic", [1000.0, 0.25, 1e-3, 10.0]), 3: ("small_J2", [1000.0, 0.25, 100.0, 10.0, 0.0, 0.0])}
TRACTION_CASES = ["warped_brick", "pinched_bricks", "tet_cube", "notch2d"]


@functools.lru_cache(maxsize=None)
def traction_case(name):
    from calibr8_amd import Assembler
    et, c, conn, sides = R.traction_cases()[name]
    assert len(c) < 1000 and sides.min() >= 0 and sides.max() < len(c)
    return Assembler(et, c, conn, *MODEL[et]), c, sides


@functools.lru_cache(maxsize=None)
def system_case(name):
    """assembler, coords, node sets of the meshes of the Dirichlet and A x tests"""
    from calibr8_amd import Assembler
    if name == "plate":      # brick(16, 16, 1): zmin has 289 nodes
        c, conn, sets = brick(16, 16, 1, 1.0, 1.0, 0.1)
        asm = Assembler(8, c, conn, "small_J2", J2)
    elif name == "pinched":  # node 13 has 53 graph neighbours
        c, conn = pinched_bricks()
        sets = {"centre": np.array([13]), "some": np.array([0, 13, 26, 27, 52])}
        asm = Assembler(8, c, conn, "small_J2", J2)
    elif name == "tri":      # 2-D `mechanics`: 2 + 1 equations per node
        c, conn, sets = tri_mesh(5, 4, 1.0, 0.8)
        asm = Assembler(3, c, conn, *MODEL[3])
    else:                    # `mechanics_plane_stress`: one residual
        c, conn, sets = tri_mesh(5, 4, 1.0, 0.8)
        asm = Assembler(3, c, conn, "small_hill_plane_stress", HILL_PS)
    assert len(c) < 1000
    return asm, c, sets


def prefill(asm, seed, signed=False):
    """a system with a different value in every entry (test_gpu_node_rows_image._prefill); `signed` for sums that cancel"""
    import torch
    ls = asm.new_linsys()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    P = 10.0 * (1.0 + torch.rand(ls.flat.numel(), generator=gen, dtype=torch.float64))
    if signed:
        P = P * (1.0 - 2.0 * (torch.rand(ls.flat.numel(), generator=gen) < 0.5).double())
    assert torch.unique(P).numel() == P.numel()
    ls.flat.copy_(P.to(asm.device))
    return ls, P.numpy().copy()


def blocks(asm, flat):
    """host views A[i][j], b[i] of a flat system image (LinearSystem's layout: A00 A01 A10 A11 b0 b1)"""
    sizes = [asm.nnz[i][j] for i in range(2) for j in range(2)] + [asm.nnodes * asm.neq[i] for i in range(2)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    v = [flat[off[k]:off[k + 1]] for k in range(6)]
    return [[v[0], v[1]], [v[2], v[3]]], [v[4], v[5]]


def device_points(asm, sides):
    from calibr8_amd import lib as L
    sides = np.ascontiguousarray(sides, dtype=np.int32)
    npf = sides.shape[1]
    pts = np.zeros((len(sides), R.NPTS[npf], 3))
    L.check(asm.L.c8_face_points(npf, len(sides), asm.coords.ctypes.data_as(L.dp), sides.ctypes.data_as(L.i32p), pts.ctypes.data_as(L.dp)))
    return pts


def tbc(asm, sides, T):
    import torch
    return (0, torch.as_tensor(np.ascontiguousarray(sides, dtype=np.int32), device=asm.device), asm.dev(np.asarray(T).ravel()))


def check_traction(asm, c, calls, sides_ref, T_ref, seed=5, zero_b=False):
    """apply `calls` (a list of tbc lists, one c8_apply_traction each) to a prefilled system; every entry of b[0] within the
    bound of bc_ref of b0 + traction_ref(sides_ref, T_ref); everything else bitwise as it was.  zero_b: b[0] starts from 0,
    where the bound is k u S and nothing but the terms' own roundings is allowed for"""
    import torch
    ls, P = prefill(asm, seed)
    if zero_b:
        ls.b[0].zero_()
        P[sum(asm.nnz[i][j] for i in range(2) for j in range(2)):][:asm.nnodes * asm.ndims] = 0.0
    for tbcs in calls:
        assert asm.apply_traction(tbcs, ls) == 0
    torch.cuda.synchronize()
    got = ls.flat.cpu().numpy()
    lo = sum(asm.nnz[i][j] for i in range(2) for j in range(2))
    hi = lo + asm.nnodes * asm.ndims
    val, S, cnt, kt = R.traction_ref(c, sides_ref, T_ref)
    b0 = P[lo:hi]
    err = np.abs(got[lo:hi].astype(LD) - (b0.astype(LD) + val))
    bound = R.sum_bound(S, cnt, kt, b0)
    print("traction: %d sides, terms per entry <= %d, k_term <= %d, max err / bound %.3f" % (len(sides_ref), cnt.max(), kt.max(), float((err[cnt > 0] / bound[cnt > 0]).max())))
    assert np.all(err <= bound)
    assert np.array_equal(got[lo:hi][cnt == 0], b0[cnt == 0])  # rows of nodes on no listed side
    assert np.array_equal(got[:lo], P[:lo]) and np.array_equal(got[hi:], P[hi:])
    return cnt


# ---- traction ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRACTION_CASES)
def test_face_points_match_restatement(name):
    asm, c, sides = traction_case(name)
    pts = device_points(asm, sides)
    ref, mag = R.face_points_ref(c, sides)
    assert np.all(np.abs(pts.astype(LD) - ref) <= R.K_POINTS[sides.shape[1]] * R.U * mag)


@pytest.mark.parametrize("name", TRACTION_CASES)
def test_traction_matches_restatement_entry_by_entry(name):
    # a traction that varies from point to point, on every boundary side of the mesh (quad4: warped faces in all six
    # orientations), and on a part of them so that whole node rows lie on no listed side
    asm, c, sides = traction_case(name)
    T = R.smooth_traction(device_points(asm, sides))
    cnt = check_traction(asm, c, [[tbc(asm, sides, T)]], sides, T)
    check_traction(asm, c, [[tbc(asm, sides, T)]], sides, T, zero_b=True)
    if name == "warped_brick":
        assert cnt.max() == 16 and (cnt == 0).sum() == 2 * 3  # corner of four faces x four points; two interior nodes
    part = np.arange(len(sides)) % 3 == 0
    cnt = check_traction(asm, c, [[tbc(asm, sides[part], T[part])]], sides[part], T[part], seed=6)
    assert (cnt == 0).sum() >= 2 * asm.ndims


def test_traction_accumulates_over_conditions_and_over_calls():
    asm, c, sides = traction_case("warped_brick")
    T = R.smooth_traction(device_points(asm, sides))
    twice, T2 = np.concatenate([sides, sides]), np.concatenate([T, T])
    val, S = R.traction_ref(c, sides, T)[:2]
    # the reference of both: twice the single one (to the rounding of long double sums taken in another order)
    assert np.all(np.abs(R.traction_ref(c, twice, T2)[0] - 2 * val) <= 64 * np.finfo(LD).eps * S)
    one = tbc(asm, sides, T)
    check_traction(asm, c, [[one, one]], twice, T2)
    check_traction(asm, c, [[one], [one]], twice, T2)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_traction_face_counts_around_the_block_size(n):
    # the face list of the warped brick repeated up to n faces (contributions add, so a repeated face is legal)
    asm, c, sides = traction_case("warped_brick")
    T = R.smooth_traction(device_points(asm, sides))
    pick = np.arange(n) % len(sides)
    check_traction(asm, c, [[tbc(asm, sides[pick], T[pick])]], sides[pick], T[pick])


# ---- Dirichlet --------------------------------------------------------------------------------------------------------
def check_dirichlet(asm, dbcs, is_adjoint=False, seed=9):
    """dbcs: (resid, eq, nodes, values) on the host.  A and b after the device call equal dirichlet_ref bit for bit."""
    import torch
    ls, P = prefill(asm, seed)
    rng = np.random.default_rng(seed)
    x = [rng.standard_normal(asm.nnodes * asm.ndims), rng.standard_normal(asm.nnodes)]
    dd = [(r, e, torch.as_tensor(np.asarray(nodes, dtype=np.int32), device=asm.device), asm.dev(np.asarray(vals, dtype=np.float64)))
          for r, e, nodes, vals in dbcs]
    for r, e, nodes, vals in dbcs:
        assert len(nodes) == len(vals) and (len(nodes) == 0 or (min(nodes) >= 0 and max(nodes) < asm.nnodes))
    assert asm.apply_dirichlet(dd, asm.dev(x[0]), asm.dev(x[1]), ls, is_adjoint=is_adjoint) == 0
    torch.cuda.synchronize()
    A0, b0 = blocks(asm, P)
    A1, b1 = R.dirichlet_ref(asm.rowptr, asm.colidx, A0, b0, x, dbcs, is_adjoint, neq=asm.neq)
    A, b = blocks(asm, ls.flat.cpu().numpy())
    for i in range(2):
        assert np.array_equal(b[i], b1[i])
        for j in range(2):
            assert np.array_equal(A[i][j], A1[i][j])
    return (A0, b0), (A1, b1), x


def values(nodes, seed):
    return np.random.default_rng(seed).standard_normal(len(nodes))


def test_dirichlet_later_condition_wins_on_shared_rows():
    asm, c, sets = system_case("plate")
    z = sets["zmin"]
    first, second = z[:200], z[100:]
    v1, v2 = values(first, 1), values(second, 2)
    (A0, b0), (A1, b1), x = check_dirichlet(asm, [(0, 1, first, v1), (0, 1, second, v2)])
    # said once more without the restatement: the shared rows carry the second value, the diagonal survived both
    rp, ci = asm.rowptr[0][0], asm.colidx[0][0]
    for k, node in enumerate(second[:100]):
        row = 3 * int(node) + 1
        assert node in first
        d = [q for q in range(rp[row], rp[row + 1]) if ci[q] == row]
        assert len(d) == 1 and A1[0][0][d[0]] == A0[0][0][d[0]] != 0.0
        assert b1[0][row] == A0[0][0][d[0]] * (x[0][row] - v2[k])


def test_dirichlet_every_equation_of_one_node_and_a_row_of_degree_53():
    asm, c, sets = system_case("pinched")
    assert asm.rowptr[1][1][14] - asm.rowptr[1][1][13] == 53
    n = sets["centre"]
    check_dirichlet(asm, [(0, 0, n, [0.5]), (0, 1, n, [-0.25]), (0, 2, n, [2.0]), (1, 0, n, [7.0])])
    s = sets["some"]
    check_dirichlet(asm, [(0, 2, s, values(s, 3)), (1, 0, s, values(s, 4))])


def test_dirichlet_empty_set_between_two_others():
    asm, c, sets = system_case("plate")
    check_dirichlet(asm, [(0, 0, sets["xmin"], values(sets["xmin"], 5)), (0, 1, [], []), (1, 0, sets["ymax"], values(sets["ymax"], 6))])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_dirichlet_set_sizes_around_the_block_size(n):
    asm, c, sets = system_case("plate")
    assert len(sets["zmin"]) == 289
    nodes = sets["zmin"][::-1][:n]
    check_dirichlet(asm, [(0, 2, nodes, values(nodes, n))])


def test_dirichlet_adjoint_rows_are_exactly_zero():
    asm, c, sets = system_case("plate")
    nodes = sets["ymin"]
    (A0, b0), (A1, b1), x = check_dirichlet(asm, [(0, 0, nodes, values(nodes, 7)), (1, 0, nodes, values(nodes, 8))], is_adjoint=True)
    assert np.all(b0[0][3 * nodes] != 0.0) and np.all(b1[0][3 * nodes] == 0.0) and np.all(b1[1][nodes] == 0.0)


def test_dirichlet_on_a_2d_mixed_mesh():
    asm, c, sets = system_case("tri")
    assert asm.ndims == 2 and asm.nres == 2
    check_dirichlet(asm, [(0, 0, sets["xmin"], values(sets["xmin"], 1)), (0, 1, sets["ymin"], values(sets["ymin"], 2)),
                          (1, 0, sets["ymax"], values(sets["ymax"], 3)), (0, 1, sets["xmin"], values(sets["xmin"], 4))])


def test_dirichlet_on_a_one_residual_system_without_second_blocks():
    # mechanics_plane_stress: the system is A[0][0], b[0] alone; every [1] pointer of system and x is NULL
    import torch
    from calibr8_amd import lib as L
    asm, c, sets = system_case("plane_stress")
    assert asm.nres == 1 and asm.ndims == 2
    gen = torch.Generator(device="cpu").manual_seed(3)
    A00 = 10.0 * (1.0 + torch.rand(asm.nnz[0][0], generator=gen, dtype=torch.float64))
    b0 = 10.0 * (1.0 + torch.rand(asm.nnodes * 2, generator=gen, dtype=torch.float64))
    x0 = np.random.default_rng(3).standard_normal(asm.nnodes * 2)
    dbcs = [(0, 0, sets["xmin"], values(sets["xmin"], 1)), (0, 1, sets["ymin"], values(sets["ymin"], 2)), (0, 1, sets["xmin"], values(sets["xmin"], 3))]
    dA, db, dx = A00.to(asm.device), b0.to(asm.device), asm.dev(x0)
    keep = [(torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(v)) for _, _, n, v in dbcs]
    d = (L.Dbc * len(dbcs))(*[L.Dbc(r, e, len(n), keep[k][0].data_ptr(), keep[k][1].data_ptr()) for k, (r, e, n, v) in enumerate(dbcs)])
    sy = L.System()
    sy.A[0][0], sy.b[0] = dA.data_ptr(), db.data_ptr()
    xs = (C.c_void_p * 2)(dx.data_ptr(), None)
    assert asm.L.c8_apply_dirichlet(asm.h, len(dbcs), d, xs, C.byref(sy), 0) == 0
    torch.cuda.synchronize()
    A1, b1 = R.dirichlet_ref([[asm.rowptr[0][0]]], [[asm.colidx[0][0]]], [[A00.numpy()]], [b0.numpy()], [x0], dbcs, False, neq=(2, 1))
    assert np.array_equal(dA.cpu().numpy(), A1[0][0]) and np.array_equal(db.cpu().numpy(), b1[0])


def test_dirichlet_refusals_leave_the_system_untouched():
    import torch
    from calibr8_amd import lib as L
    asm, c, sets = system_case("pinched")
    ls, P = prefill(asm, 4)
    nodes = torch.as_tensor(np.array([3, 13], dtype=np.int32), device=asm.device)
    vals, xu, xp = asm.dev(np.array([1.0, 2.0])), asm.dev(np.ones(asm.nnodes * 3)), asm.dev(np.ones(asm.nnodes))
    good = (0, 1, nodes, vals)
    for bad in [(2, 0), (-1, 0), (0, 3), (0, -1), (1, 1), (1, -1)]:
        for dbcs in ([bad + (nodes, vals)], [good, bad + (nodes, vals)]):  # alone, and behind a condition that is in order
            with pytest.raises(L.C8Error) as e:
                asm.apply_dirichlet(dbcs, xu, xp, ls)
            assert e.value.code == L.C8_ERR_ARG
    d = (L.Dbc * 1)(L.Dbc(0, 1, 2, nodes.data_ptr(), vals.data_ptr()))
    sy = ls.c_struct()
    assert asm.L.c8_apply_dirichlet(asm.h, -1, d, (C.c_void_p * 2)(xu.data_ptr(), xp.data_ptr()), C.byref(sy), 0) == L.C8_ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(ls.flat.cpu().numpy(), P)
    # a traction call is checked in the same way: a tri3 side list behind a quad4 one on residual 1 is refused as a whole
    quad = tbc(asm, [[0, 1, 4, 3]], np.ones((1, 4, 3)))
    with pytest.raises(L.C8Error) as e:
        asm.apply_traction([quad, (1,) + quad[1:]], ls)
    assert e.value.code == L.C8_ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(ls.flat.cpu().numpy(), P)


# ---- y = A x ----------------------------------------------------------------------------------------------------------
def check_apply_A(asm, ls, flat, x):
    """y prefilled with NaN; every row within (n + 1) u sum |a| |x| of spmv_ref; rows of a residual not in use stay NaN"""
    import torch
    nres = asm.nres
    y = [torch.full((asm.nnodes * asm.neq[i],), float("nan"), dtype=torch.float64, device=asm.device) for i in range(2)]
    assert asm.apply_A(ls, asm.dev(x[0]), asm.dev(x[1]), y[0], y[1]) == 0
    torch.cuda.synchronize()
    A, _ = blocks(asm, flat)
    ref, S, n = R.spmv_ref(asm.rowptr, asm.colidx, [row[:nres] for row in A[:nres]], x[:nres])
    for i in range(nres):
        got = y[i].cpu().numpy()
        assert not np.isnan(got).any()  # the first column block assigns
        err, bound = np.abs(got.astype(LD) - ref[i]), R.sum_bound(S[i], n[i], 1)
        print("A x: block %d, terms per row <= %d, max err / bound %.3f" % (i, n[i].max(), float((err / np.where(bound > 0, bound, 1)).max())))
        assert np.all(err <= bound)
    for i in range(nres, 2):
        assert np.isnan(y[i].cpu().numpy()).all()
    return [t.cpu().numpy() for t in y], n


@pytest.mark.parametrize("name", ["pinched", "tri", "plane_stress"])
def test_apply_A_matches_restatement_row_by_row(name):
    asm, c, sets = system_case(name)
    ls, P = prefill(asm, 12, signed=True)
    rng = np.random.default_rng(12)
    x = [rng.standard_normal(asm.nnodes * asm.ndims), rng.standard_normal(asm.nnodes)]
    y, n = check_apply_A(asm, ls, P, x)
    if name == "pinched":
        assert n[0].max() == 53 * (3 + 1) and n[1].max() == 53 * (3 + 1)
    zero = [np.zeros_like(x[0]), np.zeros_like(x[1])]
    y, n = check_apply_A(asm, ls, P, zero)
    assert all(np.all(y[i] == 0.0) for i in range(asm.nres))


def test_apply_A_after_dirichlet_rows():
    import torch
    asm, c, sets = system_case("pinched")
    ls, P = prefill(asm, 13, signed=True)
    rng = np.random.default_rng(13)
    x = [rng.standard_normal(asm.nnodes * 3), rng.standard_normal(asm.nnodes)]
    s = sets["some"]
    dd = [(r, e, torch.as_tensor(s.astype(np.int32), device=asm.device), asm.dev(values(s, 1))) for r, e in ((0, 0), (0, 2), (1, 0))]
    assert asm.apply_dirichlet(dd, asm.dev(x[0]), asm.dev(x[1]), ls) == 0
    torch.cuda.synchronize()
    flat = ls.flat.cpu().numpy()
    y, n = check_apply_A(asm, ls, flat, x)
    A, _ = blocks(asm, flat)
    for node in s:  # a constrained row has its diagonal entry alone: y = diag * x, one product
        row = 3 * int(node) + 2
        rp, ci = asm.rowptr[0][0], asm.colidx[0][0]
        d = [q for q in range(rp[row], rp[row + 1]) if ci[q] == row][0]
        assert y[0][row] == A[0][0][d] * x[0][row]


# ---- end to end: hex8 under a quad4 traction ----------------------------------------------------------------------------
def ymax_faces(conn, sets):
    top = set(sets["ymax"].tolist())
    return np.array([[int(e[k]) for k in f] for e in conn for f in R.HEX_SIDES if all(int(e[k]) in top for k in f)], dtype=np.int32)


def test_hex8_traction_driven_solve_matches_oracle_driven_newton():
    # the shape of test_device_newton_driver_matches_oracle_driven_newton with the load as a quad4 traction that varies
    # over the face (so that the [n][4][3] layout of PrimalDriver matters) and grows into the plastic range
    from calibr8_amd import Assembler, PrimalDriver
    c, conn, sets = brick(3, 4, 3, 1.0, 1.5, 1.0)
    c = jiggle(c, sets, 0.05)
    faces = ymax_faces(conn, sets)
    assert len(faces) == 9
    zero = lambda x, y, z, t: 0.0
    pull = lambda x, y, z, t: (0.1 * t * np.sin(2.0 * z), 0.8 * t * (1.0 + 0.3 * np.exp(x) * z), -0.05 * t * x)
    spec = [(0, d, sets["ymin"], zero) for d in range(3)]
    orc = ol.Oracle(ol.HEX8, c, conn, "small_J2", J2)
    ref = Primal(orc, c, [Dbc(*s) for s in spec], [Tbc(0, faces.tolist(), pull)], max_iters=15, abs_tol=1e-10, rel_tol=1e-10).solve(3)
    assert ref.xi[3][:, :, 6].max() > 1e-4  # plastic
    asm = Assembler(8, c, conn, "small_J2", J2)
    pr = PrimalDriver(asm, spec, [(0, faces, pull)], max_iters=15, abs_tol=1e-10, rel_tol=1e-10).solve(3)
    assert pr.newton_iters == ref.newton_iters
    for s in range(1, 4):
        du = np.abs(pr.u[s].cpu().numpy() - ref.u[s]).max() / np.abs(ref.u[s]).max()
        dxi = np.abs(pr.xi[s].cpu().numpy() - ref.xi[s]).max()
        print("step %d: u rel %.2e, xi %.2e" % (s, du, dxi))
        assert du < 1e-10 and dxi < 1e-10


def patch_problem():
    c, conn, sets = brick(3, 4, 3, 1.0, 1.5, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, k, sets[s], zero) for k, s in enumerate(["xmin", "ymin", "zmin"])]
    T, E, nu = 1.0, J2[0], J2[1]  # below the yield strength 2: the elastic range
    exact = np.stack([-nu * T / E * c[:, 0], T / E * c[:, 1], -nu * T / E * c[:, 2]], axis=1).ravel()
    return c, conn, sets, spec, ymax_faces(conn, sets), (lambda x, y, z, t: (0.0, T, 0.0)), exact, T * 1.5 / E


def patch_distance(u, exact, scale):
    return float(np.abs(u - exact).max() / scale)


def test_hex8_patch_test_under_constant_traction():
    # uniform uniaxial stress T on a jiggled mesh: u_y(ymax) = T l_y / E, u = (-nu T x, T y, -nu T z) / E in every node.
    # The bar is the oracle-driven host solve's own distance to the closed form (largest nodal error over T l_y / E) times
    # ten: the two solves differ in summation order and in the linear solver's rounding only.  Measured host distance:
    # 1.37e-13 (2.4e-14 for the mean of u_y over ymax), so the bar is 1.4e-12.
    from calibr8_amd import Assembler, PrimalDriver
    c, conn, sets, spec, faces, pull, exact, scale = patch_problem()
    orc = ol.Oracle(ol.HEX8, c, conn, "small_J2", J2)
    ref = Primal(orc, c, [Dbc(*s) for s in spec], [Tbc(0, faces.tolist(), pull)], max_iters=15, abs_tol=1e-10, rel_tol=1e-10).solve(1)
    host = patch_distance(ref.u[1], exact, scale)
    assert 1e-14 < host < 1e-12  # the figure above still describes the host solve
    asm = Assembler(8, c, conn, "small_J2", J2)
    pr = PrimalDriver(asm, spec, [(0, faces, pull)], max_iters=15, abs_tol=1e-10, rel_tol=1e-10).solve(1)
    u = pr.u[1].cpu().numpy()
    dev = patch_distance(u, exact, scale)
    print("patch test: host distance %.3e, device distance %.3e" % (host, dev))
    assert pr.newton_iters == ref.newton_iters
    assert abs(u.reshape(-1, 3)[sets["ymax"], 1].mean() / scale - 1.0) <= 10 * host
    assert dev <= 10 * host
