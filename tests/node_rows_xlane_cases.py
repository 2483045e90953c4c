"""Cases shared by test_emul_node_rows_xlane.py and test_gpu_node_rows_xlane.py: phase B of the row-per-node kernels takes
dN_m/dx of a column node from the inverse Jacobian G(pt) that ANOTHER lane of the element holds in registers, handed over
by a lane exchange (c8_assemble_node.hpp: lane_xor8; lane l of an element owns point hex_code(l)).  The meshes of
node_rows_chain_cases.py and its second plastic step (plastic at every point, with points that unload and points that
yield further), plus a jiggled SINGLE element: on a parallelepiped G is the same at all eight points and a value taken
from the wrong lane of the group cannot show.
Both backends (emulated kernels, HIP library through GpuBackend) take and return numpy arrays."""
import functools

import numpy as np

import node_rows_chain_cases as chain
import oracle_lib as ol
from meshes import brick, jiggle, prescribed_fields
from node_rows_chain_cases import blocks, check_against_wave, same_bits  # noqa: F401  (the tests take them from here)
from parity import compare_systems, rel_vec
from parity_cases import J2

# brick111: one valid group of eight lanes; jiggled111: G differs from point to point in the one group; brick222 (jiggled):
# nodes with 1 / 2 / 4 / 8 elements, inactive groups beside active ones; pinched_bricks: sixteen elements at a node, two
# rounds; two_sets: parameters that change from element to element
MESHES = ["brick111", "jiggled111", "brick222", "pinched_bricks", "two_sets"]
NOT_PARALLELEPIPEDS = ["jiggled111", "brick222", "two_sets"]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """coords, conn, element sets (or None), parameters"""
    if name != "jiggled111":
        return chain.mesh(name)
    c, conn, _ = brick(1, 1, 1, 1.0, 0.8, 0.7)
    return jiggle(c, {}, 0.2), conn, None, J2  # no boundary sets: every node moves


def face_defects(name):
    """per element the largest |x0 - x1 + x2 - x3| over its six faces (nodes in the face's cyclic order; zero on a
    parallelogram), relative to the face's diagonal: zero for a parallelepiped"""
    c, conn = mesh(name)[:2]
    x = c[conn]
    faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    return np.max([np.linalg.norm(x[:, a] - x[:, b] + x[:, c_] - x[:, d], axis=1) / np.linalg.norm(x[:, c_] - x[:, a], axis=1)
                   for a, b, c_, d in faces], axis=0)


@functools.lru_cache(maxsize=None)
def oracle(name):
    c, conn, es, prm = mesh(name)
    return ol.Oracle(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)


@functools.lru_cache(maxsize=None)
def steps(name):
    """node_rows_chain_cases.steps on the meshes of this module: (u1, p1, xi1) of a first step that is plastic at every
    point with a different state at every point, (u2, p2) of a second step whose stretch grows along y"""
    if name != "jiggled111":
        return chain.steps(name)
    c = mesh(name)[0]
    orc = oracle(name)
    u1, p1 = prescribed_fields(c, 0.004, ramp=False, perturb=1e-1)
    xi1 = orc.new_state()
    assert orc.forward_jacobian(u1, p1, np.zeros_like(u1), np.zeros_like(p1), orc.new_state(), xi1, orc.new_linsys()) == 0
    rows = xi1.reshape(-1, xi1.shape[-1])
    assert (rows[:, -1] > 0).all()
    assert len(np.unique(rows, axis=0)) == len(rows)
    u2, p2 = prescribed_fields(c, 0.008, ramp=True, perturb=5e-2, seed=4321)
    return u1, p1, xi1, u2, p2


def forward(be, name, ls=None):
    """the second step's forward assembly: (system, state)"""
    u1, p1, xi1, u2, p2 = steps(name)
    ls, xi = be.new_linsys() if ls is None else ls, be.new_state()
    assert be.forward_jacobian(u2, p2, u1, p1, xi1.copy(), xi, ls) == 0
    return ls, xi


def adjoint(be, name, xi):
    """the second step's adjoint assembly at the state xi, with history terms g and f that differ from entry to entry"""
    u1, p1, xi1, u2, p2 = steps(name)
    rng = np.random.default_rng(11)
    g = 1e-3 * rng.standard_normal((be.nelems, be.npts, be.nloc))
    f = 1e-3 * rng.standard_normal((be.nelems, be.npts, 4 * be.nn))
    ls = be.new_linsys()
    assert be.adjoint_jacobian(u2, p2, u1, p1, xi1.copy(), xi, g, f, ls) in (0, None)  # the oracle's returns nothing
    return ls


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's second step, computed once: (forward system, state, adjoint system)"""
    orc = oracle(name)
    ls, xi = forward(orc, name)
    xi1 = steps(name)[2]
    grew = xi[:, :, -1] > xi1[:, :, -1]
    assert grew.any() and (~grew).any()  # points that yield further and points that unload
    return ls, xi, adjoint(orc, name, xi)


def check_against_oracle(name, ls, xi, ls_adj, tol):
    ls_o, xi_o, adj_o = reference(name)
    orc = oracle(name)
    errs = compare_systems(orc, ls, ls_o)
    errs["xi"] = rel_vec(xi, xi_o)
    print(name, "K1 against the oracle:", errs)
    assert max(errs.values()) < tol, errs
    errs = compare_systems(orc, ls_adj, adj_o)
    print(name, "K3 against the oracle:", errs)
    assert max(errs.values()) < tol, errs


def check_assign_and_accumulate(name, be, set_assign):
    """Assign mode over stale content gives the rows R themselves, forward and adjoint; accumulate mode on top of zeros gives
    the same bits, and on top of a prefilled system P it gives P + R with one addition per entry (phase D)."""
    def both(prefill):
        out = []
        for k in range(2):
            ls = be.new_linsys()
            P = []
            for a in blocks(ls):
                a[:] = prefill(a.shape, k)
                P.append(a.copy())
            if k == 0:
                ls, xi = forward(be, name, ls=ls)
            else:
                u1, p1, xi1, u2, p2 = steps(name)
                hist = np.random.default_rng(11)
                g = 1e-3 * hist.standard_normal((be.nelems, be.npts, be.nloc))
                f = 1e-3 * hist.standard_normal((be.nelems, be.npts, 4 * be.nn))
                assert be.adjoint_jacobian(u2, p2, u1, p1, xi1.copy(), reference(name)[1].copy(), g, f, ls) in (0, None)
                xi = None
            out.append((ls, xi, P))
        return out

    zero = both(lambda shape, k: 0.0)
    set_assign(True)
    try:
        assigned = both(lambda shape, k: -7.25e3)
    finally:
        set_assign(False)
    rng = np.random.default_rng(5)
    pre = both(lambda shape, k: 10.0 * (1.0 + rng.random(shape)))
    for (ls0, xi0, _), (lsa, xia, _), (lsp, xip, P) in zip(zero, assigned, pre):
        assert same_bits(lsa, ls0)
        assert all(np.array_equal(a, q + r) for a, q, r in zip(blocks(lsp), P, blocks(lsa)))
        if xi0 is not None:
            assert np.array_equal(xia, xi0) and np.array_equal(xip, xi0)
