"""Cases shared by test_emul_node_rows_jinv.py and test_gpu_node_rows_jinv.py: the row-per-node kernels form dN/dx from the
cached inverse Jacobian G (c8_assemble_node.hpp, phase A).  On axis-aligned cubes G is a multiple of the identity, and a
transposed G, a swapped (k, d) or a wrong point index is invisible: these are the smallest meshes on which it is not.
Both backends (emulated kernels, HIP library through GpuBackend) take and return numpy arrays."""
import numpy as np

import oracle_lib as ol
from meshes import brick, jiggle, notched_bar, pinched_bricks, prescribed_fields
from parity import compare_systems, rel_vec
from parity_cases import J2

J2_B = [700.0, 0.3, 50.0, 1.2, 0.0, 0.0]  # the second element set of the jiggled brick
MESHES = ["sheared", "sheared_corner", "brick222", "notched_bar", "pinched_bricks"]
# a displacement gradient with nine distinct entries, small enough for every point to stay elastic
GRAD = 1e-4 * np.array([[1.0, 0.2, -0.3], [0.4, -0.5, 0.6], [-0.7, 0.8, 0.9]])


def mesh(name):
    """coords, conn, element sets (or None), parameters"""
    if name in ("sheared", "sheared_corner"):
        # one parallelepiped with edges (1, 0, 0), (0.3, 2, 0), (0.2, -0.4, 0.5): J constant, non-symmetric, non-diagonal;
        # with one corner moved J differs from point to point
        c, conn, _ = brick(1, 1, 1)
        c = c @ np.array([[1.0, 0.0, 0.0], [0.3, 2.0, 0.0], [0.2, -0.4, 0.5]])
        if name == "sheared_corner":
            c[conn[0, 6]] += np.array([0.15, -0.1, 0.2])
        return c, conn, None, J2
    if name == "brick222":  # degrees 8 / 12 / 18 / 27, stretched 1 : 3 : 0.5, two interleaved element sets
        c, conn, sets = brick(2, 2, 2, 1.0, 3.0, 0.5)
        return jiggle(c, sets, 0.15), conn, np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=np.int32), [J2, J2_B]
    if name == "notched_bar":
        c, conn, _ = notched_bar(10, 6, 3)
        return c, conn, None, J2
    c, conn = pinched_bricks()
    return c, conn, None, J2


def oracle(name):
    c, conn, es, prm = mesh(name)
    return ol.Oracle(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)


def plastic_state(name):
    """a state with plastic and elastic points: (u, p, zero fields, previous local state)"""
    c = mesh(name)[0]
    u, p = prescribed_fields(c, 0.004, ramp=True, perturb=5e-2)
    return u, p, np.zeros_like(u), np.zeros_like(p)


def blocks(ls):
    return [ls.A[i][j] for i in range(2) for j in range(2)] + [ls.b[0], ls.b[1]]


def rel_flat(ls, ref):
    """largest deviation of a system against the largest entry of the reference"""
    a, b = np.concatenate(blocks(ls)), np.concatenate(blocks(ref))
    return float(np.abs(a - b).max() / np.abs(b).max())


def forward(be, name, ls=None, state=None):
    u, p, z, zp = plastic_state(name) if state is None else state
    ls, xi = be.new_linsys() if ls is None else ls, be.new_state()
    assert be.forward_jacobian(u, p, z, zp, be.new_state(), xi, ls) == 0
    return ls, xi


def adjoint(be, name, xi):
    u, p, z, zp = plastic_state(name)
    rng = np.random.default_rng(11)
    g = 1e-3 * rng.standard_normal((be.nelems, be.npts, be.nloc))
    f = np.zeros((be.nelems, be.npts, 4 * be.nn))
    ls = be.new_linsys()
    assert be.adjoint_jacobian(u, p, z, zp, be.new_state(), xi, g, f, ls) in (0, None)  # the oracle's returns nothing
    return ls


def check_forward_against_oracle(orc, ls, xi, name, tol):
    ls_o, xi_o = forward(orc, name)
    assert (xi_o[:, :, -1] > 0).any() and (xi_o[:, :, -1] == 0).any()  # plastic and elastic points
    errs = compare_systems(orc, ls, ls_o)
    errs["xi"] = rel_vec(xi, xi_o)
    print(name, "K1 against the oracle:", errs)
    assert max(errs.values()) < tol, errs


def check_adjoint_against_oracle(orc, ls, name, xi, tol):
    errs = compare_systems(orc, ls, adjoint(orc, name, xi))
    print(name, "K3 against the oracle:", errs)
    assert max(errs.values()) < tol, errs


def linear_state(name):
    """u linear in x with the gradient GRAD, p linear in x: every point elastic"""
    c = mesh(name)[0]
    u = np.ascontiguousarray((c @ GRAD.T).ravel())
    p = 0.05 + c @ np.array([0.01, -0.02, 0.03])
    return u, p, np.zeros_like(u), np.zeros_like(p)


def numpy_elastic_residual(name):
    """The residual of the linear state with dN/dx rebuilt here from the coordinates and the Gauss points:
    b_u[a, i] = sum w dv (2 mu dev eps - p I)_ij dN_a/dx_j,   b_p[a] = sum w dv [-(tr eps + p / kappa) N_a - tau grad p . grad N_a],
    tau = h^2 / (2 mu), h the root mean square edge length (stabilisation multiplier 1).  Also returns the largest deviation
    of the interpolated displacement gradient from GRAD."""
    c, conn, es, prm = mesh(name)
    prm = np.atleast_2d(np.asarray(prm, dtype=np.float64))
    u, p = linear_state(name)[:2]
    u = u.reshape(-1, 3)
    sg = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
    gp = 1.0 / np.sqrt(3.0)
    b_u, b_p, worst = np.zeros((len(c), 3)), np.zeros(len(c)), 0.0
    for e, nodes in enumerate(conn):
        E, nu = prm[es[e] if es is not None else 0][:2]
        mu, kappa = E / (2 * (1 + nu)), E / (3 * (1 - 2 * nu))
        X = c[nodes]
        h = np.sqrt(np.mean([((X[b] - X[a]) ** 2).sum() for a, b in edges]))
        tau = 0.5 * h * h / mu
        for pt in range(8):
            xi = gp * np.array([1 if pt & 1 else -1, 1 if pt & 2 else -1, 1 if pt & 4 else -1])
            f = 1 + sg * xi
            N = 0.125 * f[:, 0] * f[:, 1] * f[:, 2]
            dNdxi = 0.125 * sg * np.stack([f[:, 1] * f[:, 2], f[:, 0] * f[:, 2], f[:, 0] * f[:, 1]], axis=1)
            Jm = dNdxi.T @ X                      # J[a][b] = d x_b / d xi_a
            dN = dNdxi @ np.linalg.inv(Jm).T      # dN_m/dx_d
            wdv = np.linalg.det(Jm)
            gu = u[nodes].T @ dN
            worst = max(worst, float(np.abs(gu - GRAD).max()))
            eps = 0.5 * (gu + gu.T)
            pp, gradp = N @ p[nodes], p[nodes] @ dN
            sig = 2 * mu * (eps - np.trace(eps) / 3 * np.eye(3)) - pp * np.eye(3)
            b_u[nodes] += wdv * dN @ sig.T
            b_p[nodes] += wdv * (-(np.trace(eps) + pp / kappa) * N - tau * dN @ gradp)
    return b_u.ravel(), b_p, worst
