"""Cases shared by test_emul_node_rows_rowio.py and test_gpu_node_rows_rowio.py: the row-per-node kernels read and write a
node's CSR rows through range-checked accesses (c8_assemble_node.hpp: row_load / row_store; on the device a buffer descriptor
over exactly the row's bytes) and zero the whole row accumulator, not the node's part of it.  What can go wrong is at the
edges of a row: an entry past its end read as something else than zero, a store past its end that lands in the next node's
row, a row cut short.  So the meshes are those on which the iterations of 64 entries end in every way:
  brick111        every node has 8 columns: 72 / 24 / 24 / 8 entries -- one full iteration and a partial one, (p, p) on 8 lanes
  brick222        (jiggled) the centre node has 27 columns, 243 = 3 * 64 + 51 entries, beside nodes with 8, 12 and 18
  pinched_bricks  a node with sixteen elements: the form for more than eight elements at a node
  two_sets        (jiggled 3 x 2 x 2) two interleaved element sets with different parameters
on the second plastic step of node_rows_chain_cases.py.  A backend is driven through `run(kind, blocks, assign, parts)`, which
the two test modules provide: assemble K1 ("K1") or K3 ("K3") ONTO the six arrays `blocks` (A00, A01, A10, A11, b_u, b_p) and
return the six arrays after it; parts = "whole", "two" (the whole range of nodes in two launches) or a node range (first, end)."""
import functools

import numpy as np

import node_rows_chain_cases as chain
import node_rows_xlane_cases as xl
from node_rows_chain_cases import blocks, mesh, oracle, reference, steps  # noqa: F401  (the tests take them from here)
from node_rows_xlane_cases import check_against_oracle, check_against_wave  # noqa: F401

MESHES = ["brick111", "brick222", "pinched_bricks", "two_sets"]
KINDS = ["K1", "K3"]


def assert_meshes_reach_the_edges():
    """the degrees the module's text promises, the form each mesh runs in, and parameters that differ between the sets"""
    deg = {name: np.diff(np.asarray(oracle(name).rowptr[1][1])) for name in MESHES}
    assert (deg["brick111"] == 8).all()
    assert deg["brick222"].max() == 27 and (9 * 27) % 64 == 51 and {8, 12, 18} <= set(deg["brick222"].tolist())
    nelem = {name: np.bincount(mesh(name)[1].ravel()) for name in MESHES}
    assert nelem["pinched_bricks"].max() > 8 and all(nelem[n].max() <= 8 for n in MESHES if n != "pinched_bricks")
    es, prm = mesh("two_sets")[2:]
    assert set(es.tolist()) == {0, 1} and all(prm[0][k] != prm[1][k] for k in range(4))  # E, nu, K, Y
    assert (np.diff(es) != 0).all()                                                      # interleaved


def history(be):
    """history terms of the adjoint assembly that differ from entry to entry (node_rows_chain_cases.adjoint)"""
    rng = np.random.default_rng(11)
    return (1e-3 * rng.standard_normal((be.nelems, be.npts, be.nloc)), 1e-3 * rng.standard_normal((be.nelems, be.npts, 4 * be.nn)))


def assemble_onto(be, name, kind, ls):
    """K1 or K3 of the second step onto the system ls; K3 at the oracle's state of that step"""
    u1, p1, xi1, u2, p2 = steps(name)
    if kind == "K1":
        assert be.forward_jacobian(u2, p2, u1, p1, xi1.copy(), be.new_state(), ls) == 0
    else:
        g, f = history(be)
        assert be.adjoint_jacobian(u2, p2, u1, p1, xi1.copy(), reference(name)[1].copy(), g, f, ls) in (0, None)
    return ls


def sentinels(shapes):
    """a distinct finite value per entry of the six arrays, of the size of the assembled values' largest: k + 1 + j / 2^20 for
    entry j of array k, exactly representable"""
    return [(k + 1.0) + np.arange(int(np.prod(s)), dtype=np.float64).reshape(s) / 2.0 ** 20 for k, s in enumerate(shapes)]


def row_masks(orc, first, end):
    """per array: True at the entries of the rows of nodes [first, end)"""
    nodeptr = np.asarray(orc.rowptr[1][1])
    lo, hi, n = int(nodeptr[first]), int(nodeptr[end]), int(nodeptr[-1])
    out = []
    for width in (9, 3, 3, 1):
        m = np.zeros(width * n, dtype=bool)
        m[width * lo:width * hi] = True
        out.append(m)
    for width in (3, 1):
        m = np.zeros(width * orc.nnodes, dtype=bool)
        m[width * first:width * end] = True
        out.append(m)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def no_negative_zero(arrays):
    return not any((np.signbit(a) & (a == 0.0)).any() for a in arrays[:4])


def interior_range(name):
    """a strict interior sub-range of the nodes whose first and last rows are partial iterations of 64 entries"""
    n = oracle(name).nnodes
    first, end = max(1, n // 3), min(n - 1, n // 3 + max(2, n // 2))
    assert 0 < first < end < n
    return first, end


def check_rows_and_sentinels(name, kind, run, sub_ranges):
    """Accumulate mode adds ONE rounded sum to every entry of the assembled rows and leaves every other entry as it is; assign
    mode ignores what the rows held; the whole range of nodes in two launches gives what one launch gives."""
    orc = oracle(name)
    shapes = [a.shape for a in blocks(orc.new_linsys())]
    zeros = [np.zeros(s) for s in shapes]
    P = sentinels(shapes)
    assert all(len(np.unique(p)) == p.size and np.isfinite(p).all() for p in P)
    R = run(kind, zeros, False, "whole")                     # the rows themselves: accumulate mode onto zeros
    assert all(np.isfinite(r).all() for r in R) and all(np.abs(r).max() > 0 for r in R)
    want = [p + r for p, r in zip(P, R)]                     # one addition per entry, done on the host
    assert same(run(kind, P, False, "whole"), want)
    assert same(run(kind, P, False, "two"), want)
    assigned = run(kind, P, True, "whole")
    assert same(assigned, R) and no_negative_zero(assigned)  # = zero-then-accumulate, bit for bit
    assert same(run(kind, P, True, "two"), R)
    for first, end in sub_ranges:
        inside = row_masks(orc, first, end)
        assert all(m.any() and not m.all() for m in inside)
        for assign in (False, True):
            got = run(kind, P, assign, (first, end))
            for k, (g, m) in enumerate(zip(got, inside)):
                g, p = np.asarray(g).reshape(-1), P[k].reshape(-1)
                assert np.array_equal(bits(g[~m]), bits(p[~m])), (name, kind, k, "an entry outside the node range changed")
                w = (R[k] if assign else want[k]).reshape(-1)
                assert np.array_equal(bits(g[m]), bits(w[m])), (name, kind, k, "inside the node range")


# ---- the constants follow the parameters ----------------------------------------------------------------------------------
def other_params(name):
    """every parameter of every set changed, the thermal pair (expansion coefficient, temperature change) from zero to a
    strain of 6e-6: still plastic at every point of the second step"""
    prm = np.atleast_2d(np.asarray(mesh(name)[3], dtype=np.float64))
    new = prm * np.array([1.13, 0.9, 1.4, 0.85, 1.0, 1.0]) + np.array([0.0, 0.0, 0.0, 0.0, 3e-6, 2.0])
    assert (new != prm).all()
    return prm, new


def forward_and_adjoint(be, name):
    """(K1 system, state, K3 system at that state) of the second step"""
    ls, xi = xl.forward(be, name)
    return ls, xi, xl.adjoint(be, name, xi)


def same_results(a, b):
    return chain.same_bits(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and chain.same_bits(a[2], b[2])


@functools.lru_cache(maxsize=None)
def other_reference(name):
    """the oracle with other_params: (oracle, K1 system, state, K3 system)"""
    import oracle_lib as ol
    c, conn, es, _ = mesh(name)
    orc = ol.Oracle(ol.HEX8, c, conn, "small_J2", other_params(name)[1], elem_set=es)
    return (orc,) + forward_and_adjoint(orc, name)


def check_params_followed(name, make):
    """make(params) -> backend.  Set, change, set back on ONE context: after the change the results are those of a fresh context
    created with the new parameters, bit for bit, and agree with the oracle at them; set back, those of the first call."""
    from parity import compare_systems, rel_vec
    prm, new = other_params(name)
    be = make(prm)
    first = forward_and_adjoint(be, name)
    be.set_params(new)
    second = forward_and_adjoint(be, name)
    assert not np.array_equal(second[0].A[0][0], first[0].A[0][0]) and not np.array_equal(second[1], first[1])
    assert same_results(second, forward_and_adjoint(make(new), name))
    orc, ls_o, xi_o, adj_o = other_reference(name)
    assert (xi_o[:, :, -1] > steps(name)[2][:, :, -1]).any()  # points that yield at the new parameters
    errs = compare_systems(orc, second[0], ls_o)
    errs["xi"] = rel_vec(second[1], xi_o)
    errs.update({"K3 " + k: v for k, v in compare_systems(orc, second[2], adj_o).items()})
    print(name, "changed parameters against the oracle:", errs)
    assert max(errs.values()) < 1e-12, errs
    be.set_params(prm)
    assert same_results(forward_and_adjoint(be, name), first)
