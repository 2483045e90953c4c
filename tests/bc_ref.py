"""High-precision restatements of the three boundary kernels of c8_primal.hip (TEST INFRASTRUCTURE): traction surface
integrals (tbcs.cpp:17-86), Dirichlet row replacement (dbcs.cpp:28-121) and y = A x over the CSR blocks.  Plain numpy in
np.longdouble (64-bit mantissa on x86), written from the formulas; every sum comes with the sum of the magnitudes of its
terms, which is what a rounding-error bound scales with.

The entrywise bound
-------------------
u = 2^-53.  A float64 evaluation of an entry  b0 + sum_t term_t  (any order of the additions: the device adds with
atomics) differs from the exact value by at most, to first order in u,

    u * ( k_term * S  +  n * (|b0| + S) ),      S = sum_t |term_t|,  n = number of terms,          (*)

where k_term bounds the relative roundings that FORM one term, and every one of the n additions rounds a partial sum that
is at most |b0| + S.  With b0 = 0 this is the form  k * u * S,  k = n + k_term.  n is counted from the mesh (a node of the
warped brick has up to 4 faces x 4 points = 16 quad4 terms, more where face lists are repeated).  Fused multiply-adds only
remove roundings, so the counts hold for a contracted build too.  All counts below are rounded up to integers.

k_term of a traction term  T_d * N_a * dv:
  * g = 1/sqrt(3) as a double: 1 rounding.  A factor (1 +- g) inherits g's error enlarged by g / (1 - g) = 1.37 and rounds
    once more: 2.37.  N_a = 0.25 * f1 * f2 (the product with 0.25 is exact): 2 * 2.37 + 1 -> K_N = 6.
  * dN_a/dxi = 0.25 * s * f: 2.37; a tangent component t_d = sum_a dN_a X_a,d takes one product and three additions more:
    |delta t_d| <= C1 * u * A_d,  C1 = 7,  A_d = sum_a |dN_a| |X_a,d|.  The tangents are DIFFERENCES of coordinates, so
    A_d / |t_d| is not a fixed number: it grows with the distance of the face from the origin over its size (about 6 on the
    unit bricks of the tests).  The restatement therefore does not assume it; it propagates A through the cross product,
        |delta c_x| <= u * ( C1 * (A1_y |t2_z| + |t1_y| A2_z + A1_z |t2_y| + |t1_z| A2_y) + 2 * (|t1_y t2_z| + |t1_z t2_y|) ),
    (two products and one subtraction round: 2 on the magnitude sum), and through dv = sqrt(c . c):
        k_dv = |delta c|_2 / (u |c|_2) + 2.5        (three squares and two additions: 3, halved by the root, + 1 for the root).
    This is the only mesh-dependent part of k_term, and it is computed from the mesh in long double, not from any device.
  * T_d * N_a, then * dv: 2.                                  quad4:  k_term = K_N + 2 + k_dv.
  * tri3: e = X_b - X_0 is one rounding of an exact difference (C1 = 1, A = |e|); the term is T_d * (1/3) * 0.5 * dv with
    1/3 rounded: 1 + 2 products (0.5 is exact).                tri3:   k_term = 3 + k_dv.
  * edge: len = sqrt(ex^2 + ey^2) with e as above: (1 + 1) for the squares halves to 1, + 0.5 for the addition, + 1 for the
    root -> 3; the term is T_d * 0.5 * len: 1 product.          edge:   k_term = 4.

A x: a row of a system with nres blocks has n = deg * (sum_j neq_j) terms a * x (deg * (3 + 1) for 3-D mechanics), each one
rounding (k_term = 1), and at most n additions (the sum of a block starts from an exact 0, the blocks are added to y):
k = n + 1, b0 = 0.

Face points x_q = sum_a N_a X_a: K_N + 1 product + 3 additions = K_POINTS[4] = 10 roundings on sum_a |N_a| |X_a| (tri3: two
additions and a division, 3; edge: one addition, the product with 0.5 is exact, 1).

The Dirichlet rows involve no sum: b = diag * (x - v) is one subtraction and one product, and a product of a difference
cannot be contracted.  `dirichlet_ref` therefore works in the dtype it is given, and on float64 input its result is to
be met bit for bit.
"""
import numpy as np

LD = np.longdouble
U = LD(2) ** -53
SX = (-1.0, 1.0, 1.0, -1.0)   # local nodes of a quad4 side: (-1,-1), (1,-1), (1,1), (-1,1)
SY = (-1.0, -1.0, 1.0, 1.0)
K_N, C1_QUAD, C1_DIFF = 6, 7, 1
K_POINTS = {2: 1, 3: 3, 4: 10}
NPTS = {2: 1, 3: 1, 4: 4}


def _quad_point(q, dtype):
    """(xi, eta) of Gauss point q: bit 0 of q chooses the sign of xi, bit 1 that of eta"""
    g = dtype(1) / np.sqrt(dtype(3))
    return (g if q & 1 else -g), (g if q & 2 else -g)


def _quad_shape(q, dtype):
    xi, eta = _quad_point(q, dtype)
    sx, sy = np.array(SX, dtype=dtype), np.array(SY, dtype=dtype)
    N = (1 + sx * xi) * (1 + sy * eta) / 4
    return N, sx * (1 + sy * eta) / 4, sy * (1 + sx * xi) / 4


def _cross_norm(t1, t2, A1, A2, c1):
    """|t1 x t2| per row and k_dv of the module docstring; A1, A2 are the magnitude sums behind t1, t2"""
    c = np.cross(t1, t2)
    a1, a2 = np.abs(t1), np.abs(t2)
    err = np.zeros_like(c)
    for d in range(3):
        y, z = (d + 1) % 3, (d + 2) % 3
        err[:, d] = c1 * (A1[:, y] * a2[:, z] + a1[:, y] * A2[:, z] + A1[:, z] * a2[:, y] + a1[:, z] * A2[:, y]) \
            + 2 * (a1[:, y] * a2[:, z] + a1[:, z] * a2[:, y])
    dv = np.sqrt((c * c).sum(axis=1))
    return dv, np.sqrt((err * err).sum(axis=1)) / dv + 2.5


def _weights(X, dtype):
    """per side and point: w[f][q][a] = N_a * w_q-scaled area element (the factor of T_q[d] in the entry of node a) and
    k_term[f][q] for it"""
    n, npf = X.shape[0], X.shape[1]
    w = np.zeros((n, NPTS[npf], npf), dtype=dtype)
    kt = np.zeros((n, NPTS[npf]), dtype=dtype)
    if npf == 2:    # midpoint, weight 2, dv = length / 2, N = 1/2
        e = X[:, 1, :2] - X[:, 0, :2]
        w[:, 0, :] = (np.sqrt((e * e).sum(axis=1)) / 2)[:, None]
        kt[:] = 4
    elif npf == 3:  # centroid, weight 1/2, dv = 2 * area, N = 1/3
        e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        dv, kdv = _cross_norm(e1, e2, np.abs(e1), np.abs(e2), C1_DIFF)
        w[:, 0, :] = (dv / 6)[:, None]
        kt[:, 0] = 3 + kdv
    else:           # 2 x 2 Gauss, weights 1
        for q in range(4):
            N, dNx, dNy = _quad_shape(q, dtype)
            t1, t2 = np.einsum("a,fad->fd", dNx, X), np.einsum("a,fad->fd", dNy, X)
            A1, A2 = np.einsum("a,fad->fd", np.abs(dNx), np.abs(X)), np.einsum("a,fad->fd", np.abs(dNy), np.abs(X))
            dv, kdv = _cross_norm(t1, t2, A1, A2, C1_QUAD)
            w[:, q, :] = dv[:, None] * N[None, :]
            kt[:, q] = K_N + 2 + kdv
    return w, kt


def traction_ref(coords, faces, traction, dtype=LD):
    """b[n_a, d] -= sum_q T_q[d] N_a(xi_q) w_q dv(xi_q) over the listed sides (a side listed twice counts twice).
    coords [N][3], faces [n][2|3|4], traction [n][1|1|4][3] (one vector per side and point).  Returns four arrays over the
    entries of b ([N * 2] for edges, [N * 3] otherwise): the value, S = the sum of the magnitudes of its terms, the number
    of terms, and the largest k_term among them (module docstring)."""
    faces = np.asarray(faces, dtype=np.int64)
    n, npf = faces.shape
    nd = 2 if npf == 2 else 3
    X = np.asarray(coords, dtype=dtype)[faces]
    T = np.asarray(traction, dtype=dtype).reshape(n, NPTS[npf], 3)
    w, kt = _weights(X, dtype)
    nrows = len(coords) * nd
    val, S = np.zeros(nrows, dtype=dtype), np.zeros(nrows, dtype=dtype)
    cnt, kmax = np.zeros(nrows, dtype=np.int64), np.zeros(nrows, dtype=dtype)
    for q in range(NPTS[npf]):
        for a in range(npf):
            for d in range(nd):
                rows = faces[:, a] * nd + d
                term = T[:, q, d] * w[:, q, a]
                np.subtract.at(val, rows, term)
                np.add.at(S, rows, np.abs(term))
                np.add.at(cnt, rows, 1)
                np.maximum.at(kmax, rows, kt[:, q])
    return val, S, cnt, np.ceil(kmax)


def sum_bound(S, nterms, kterm, b0=0.0):
    """(*) of the module docstring"""
    return U * (kterm * S + nterms * (np.abs(np.asarray(b0, dtype=LD)) + S))


def face_points_ref(coords, faces, dtype=LD):
    """physical integration points [n][1|1|4][3] in the order of the traction array, and sum_a |N_a| |X_a| for each"""
    faces = np.asarray(faces, dtype=np.int64)
    npf = faces.shape[1]
    X = np.asarray(coords, dtype=dtype)[faces]
    if npf < 4:
        return X.sum(axis=1)[:, None, :] / npf, np.abs(X).sum(axis=1)[:, None, :] / npf
    pts, mag = np.zeros((len(faces), 4, 3), dtype=dtype), np.zeros((len(faces), 4, 3), dtype=dtype)
    for q in range(4):
        N = _quad_shape(q, dtype)[0]
        pts[:, q], mag[:, q] = np.einsum("a,fad->fd", N, X), np.einsum("a,fad->fd", np.abs(N), np.abs(X))
    return pts, mag


def dirichlet_ref(rowptr, colidx, A, b, x, dbcs, is_adjoint, neq=(3, 1)):
    """Row replacement on copies of A[i][j], b[i] (lists over the residuals in use; CSR rows (node, eq) -> node * neq + eq):
    for every condition (resid, eq, nodes, values), in list order, and every node of it: keep the diagonal entry, zero
    the rest of the row in every column block, b = diag * (x - value), or 0 for the adjoint system.  Returns (A, b)."""
    nres = len(b)
    A = [[np.array(A[i][j], copy=True) for j in range(nres)] for i in range(nres)]
    b = [np.array(b[i], copy=True) for i in range(nres)]
    for resid, eq, nodes, values in dbcs:
        for node, v in zip(nodes, values):
            row = int(node) * neq[resid] + eq
            diag = b[resid].dtype.type(0)
            for j in range(nres):
                lo, hi = rowptr[resid][j][row], rowptr[resid][j][row + 1]
                for k in range(lo, hi):
                    if j == resid and colidx[resid][j][k] == row:
                        diag = A[resid][j][k]
                    else:
                        A[resid][j][k] = 0
            b[resid][row] = 0 if is_adjoint else diag * (x[resid][row] - b[resid].dtype.type(v))
    return A, b


def spmv_ref(rowptr, colidx, A, x):
    """y_i = sum_j A_ij x_j over the CSR blocks (lists over the residuals in use).  Returns per residual: y, sum |a| |x| per
    row, and the number of terms per row."""
    nres = len(x)
    ys, Ss, ns = [], [], []
    for i in range(nres):
        nrows = len(rowptr[i][0]) - 1
        y, S, n = np.zeros(nrows, dtype=LD), np.zeros(nrows, dtype=LD), np.zeros(nrows, dtype=np.int64)
        for j in range(nres):
            rp = np.asarray(rowptr[i][j])
            prod = np.asarray(A[i][j], dtype=LD) * np.asarray(x[j], dtype=LD)[np.asarray(colidx[i][j])]
            rows = np.repeat(np.arange(nrows), np.diff(rp))
            np.add.at(y, rows, prod)
            np.add.at(S, rows, np.abs(prod))
            n += np.diff(rp)
        ys.append(y), Ss.append(S), ns.append(n)
    return ys, Ss, ns


# ---- the cases shared by test_bc_ref.py (reference alone) and test_gpu_boundary.py (device) ------------------------------
# local side orderings (those of the calibration side sets in test_gpu_parity.py)
HEX_SIDES = ([0, 1, 2, 3], [0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [3, 0, 4, 7], [4, 5, 6, 7])
TET_SIDES = ([0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3])
TRI_SIDES = ([0, 1], [1, 2], [2, 0])


def boundary_sides(conn, local):
    """the element sides that belong to one element only, in the element's local ordering"""
    seen = {}
    for e in conn:
        for f in local:
            s = [int(e[k]) for k in f]
            seen.setdefault(tuple(sorted(s)), []).append(s)
    return np.array([v[0] for v in seen.values() if len(v) == 1], dtype=np.int32)


def warped_brick():
    """brick(3, 2, 2) with ALL nodes moved, the boundary included, by up to 0.05 of the cell size: warped boundary faces"""
    from meshes import brick
    c, conn, _ = brick(3, 2, 2, 1.0, 0.8, 0.7)
    rng = np.random.default_rng(11)
    c = c + 0.05 * np.array([1.0 / 3, 0.8 / 2, 0.7 / 2]) * (2.0 * rng.random(c.shape) - 1.0)
    return np.ascontiguousarray(c), conn


def smooth_traction(p):
    """a smooth non-polynomial traction vector at the points p [...][3]"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([np.sin(1.3 * x + 0.4 * z) + 0.5 * y, np.exp(0.7 * y - 0.3 * x) - 1.2, np.cos(0.9 * z + x * y) + 0.1], axis=-1)


def traction_cases():
    """name -> (elem_type, coords, conn, sides): the quad4 meshes, a tri3 case on the tet cube, an edge case on notch2D"""
    import json
    import os
    from meshes import pinched_bricks
    here = os.path.dirname(os.path.abspath(__file__))
    out = {}
    c, conn = warped_brick()
    out["warped_brick"] = (8, c, conn, boundary_sides(conn, HEX_SIDES))
    c, conn = pinched_bricks()
    out["pinched_bricks"] = (8, c, conn, boundary_sides(conn, HEX_SIDES))
    d = json.load(open(os.path.join(here, "golden", "cube_tet4.json")))
    c, conn = np.array(d["coords"]), np.array(d["conn"], dtype=np.int32)
    out["tet_cube"] = (4, c, conn, boundary_sides(conn, TET_SIDES))
    d = json.load(open(os.path.join(here, "golden", "notch2D_tri3.json")))
    c, conn = np.array(d["coords"]), np.array(d["conn"], dtype=np.int32)
    out["notch2d"] = (3, c, conn, boundary_sides(conn, TRI_SIDES))
    return out
