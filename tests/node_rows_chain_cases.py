"""Cases shared by test_emul_node_rows_chain.py and test_gpu_node_rows_chain.py: the row-per-node kernels issue loads one
phase ahead of their use and hand them from phase to phase in the lane record (c8_assemble_node.hpp: the point's inverse
Jacobian, previous state and weights from A1 to A2, the first dN/dx rows from A2 to B, the old CSR values from B to D).
The smallest meshes on which such a hand-over can go wrong, and a SECOND plastic step: its previous state is the state a
first plastic step left, non-zero and different at every point, so that a stale or swapped xi_prev shows.
Both backends (emulated kernels, HIP library through GpuBackend) take and return numpy arrays."""
import functools

import numpy as np

import oracle_lib as ol
from meshes import brick, jiggle, pinched_bricks, prescribed_fields
from parity import compare_systems, rel_vec
from parity_cases import J2

J2_B = [700.0, 0.3, 50.0, 1.2, 0.0, 0.0]  # the second element set
# brick111: one valid element slot of eight in every wavefront; brick222: nodes with 1 / 2 / 4 / 8 elements; pinched_bricks: a
# node with sixteen elements (two rounds of eight); two_sets: parameters that change from element to element
MESHES = ["brick111", "brick222", "pinched_bricks", "two_sets"]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """coords, conn, element sets (or None), parameters"""
    import renumber_cases  # (imports nothing of this module)
    if name in renumber_cases.CHAIN_MESHES:  # shuffled node ids and element order, rotated local node order
        return renumber_cases.chain_mesh(name)
    if name == "brick111":
        c, conn, _ = brick(1, 1, 1, 1.0, 0.8, 0.7)
        return c, conn, None, J2
    if name == "brick222":
        c, conn, sets = brick(2, 2, 2, 1.0, 0.8, 0.7)
        return jiggle(c, sets, 0.1), conn, None, J2
    if name == "two_sets":
        c, conn, sets = brick(3, 2, 2, 1.0, 0.8, 0.7)
        return jiggle(c, sets, 0.08), conn, (np.arange(len(conn)) % 2).astype(np.int32), [J2, J2_B]
    c, conn = pinched_bricks()
    return c, conn, None, J2


@functools.lru_cache(maxsize=None)
def oracle(name):
    c, conn, es, prm = mesh(name)
    return ol.Oracle(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)


@functools.lru_cache(maxsize=None)
def steps(name):
    """Two load steps: (u1, p1, xi1) of a first step that is plastic at every point (uniform stretch of twice the yield
    strain, perturbed by a tenth of it from node to node), its state from the oracle, and (u2, p2) of a second step whose
    stretch grows along y from zero to four times the yield strain: points that unload and points that yield further."""
    c = mesh(name)[0]
    orc = oracle(name)
    u1, p1 = prescribed_fields(c, 0.004, ramp=False, perturb=1e-1)
    xi1 = orc.new_state()
    assert orc.forward_jacobian(u1, p1, np.zeros_like(u1), np.zeros_like(p1), orc.new_state(), xi1, orc.new_linsys()) == 0
    rows = xi1.reshape(-1, xi1.shape[-1])
    assert (rows[:, -1] > 0).all()                    # every point is plastic ...
    assert len(np.unique(rows, axis=0)) == len(rows)  # ... and no two points have the same state
    for j in range(rows.shape[1] - 1):                # nor, component by component, the same plastic strain
        assert len(np.unique(rows[:, j])) == len(rows)
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


def blocks(ls):
    return [ls.A[i][j] for i in range(2) for j in range(2)] + [ls.b[0], ls.b[1]]


def rel_flat(ls, ref):
    """largest deviation of a system against the largest entry of the reference"""
    a, b = np.concatenate(blocks(ls)), np.concatenate(blocks(ref))
    return float(np.abs(a - b).max() / np.abs(b).max())


def same_bits(ls, ref):
    return all(np.array_equal(a, b) for a, b in zip(blocks(ls), blocks(ref)))


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


def check_against_wave(name, ls, xi, ls_adj, ls_w, xi_w, adj_w):
    """`node` against `wave` at the suite's bounds for that pair: 1e-13 (K1, stored state), 1e-12 (K3)"""
    k1, st, k3 = rel_flat(ls, ls_w), rel_vec(xi, xi_w), rel_flat(ls_adj, adj_w)
    print(name, "node against wave: K1 %.2e, state %.2e, K3 %.2e" % (k1, st, k3))
    assert k1 < 1e-13 and st < 1e-13 and k3 < 1e-12


def check_assign_and_accumulate(name, be, set_assign):
    """Assign mode over stale content gives the rows R themselves; accumulate mode then adds R to whatever the system holds
    with ONE addition per entry (old value + R: phase D): on top of the assigned rows the result is R + R, on top of a
    prefilled system P it is P + R, both exactly."""
    ls_ref, xi_ref = forward(be, name)  # accumulate mode, into zeros
    stale = be.new_linsys()
    for a in blocks(stale):
        a[:] = -7.25e3
    set_assign(True)
    try:
        ls, xi = forward(be, name, ls=stale)
    finally:
        set_assign(False)
    assert same_bits(ls, ls_ref) and np.array_equal(xi, xi_ref)
    R = [a.copy() for a in blocks(ls)]
    ls2, xi2 = forward(be, name, ls=ls)  # accumulate on top of the assigned rows
    assert all(np.array_equal(a, r + r) for a, r in zip(blocks(ls2), R)) and np.array_equal(xi2, xi_ref)
    pre = be.new_linsys()
    rng = np.random.default_rng(5)
    P = []
    for a, r in zip(blocks(pre), R):
        a[:] = np.abs(r).max() * rng.standard_normal(a.shape)
        P.append(a.copy())
    ls3, _ = forward(be, name, ls=pre)
    assert all(np.array_equal(a, q + r) for a, q, r in zip(blocks(ls3), P, R))
