"""Cases shared by test_emul_renumbered.py and test_gpu_renumbered.py: hex8 meshes with shuffled node ids, shuffled element
order and rotated local node order.  Every other hex8 mesh of the suite starts from meshes.brick: x-fastest node ids,
elements in the same order, one local node order everywhere, so that an interior node's eight elements (ascending) always
see it at the same eight distinct local indices in the same sequence, element e + 1 is the x-neighbour and every graph row
has the same shape.  An error tied to the pairing (element slot, local index), to two elements seeing a node at the same
local index, to the order of a node's elements or to an irregular chunk plan cannot show there.

HEX_ROTATIONS are the 24 proper symmetries of the reference hex as permutations of the local nodes, conn_new[i] =
conn_old[ROT[i]].  renumber() applies a node permutation, an element permutation and a rotation per element and returns a
record with the maps that carry nodal vectors, point fields, element sets and CSR blocks from the old numbering to the new.
The conditions under which a wrong kernel could hide on a brick are asserted NOT to hold on these meshes, from conn alone."""
import functools
import itertools

import numpy as np

import oracle_lib as ol
from meshes import brick, jiggle, notched_bar, pinched_bricks
from parity_cases import J2

J2_B = [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]  # the second parameter row of parity_cases.check_two_element_sets


def hex_code(n):
    """the local-state point that sits at local node n, and back (c8_assemble_node.hpp): an involution"""
    return n ^ ((n >> 1) & 1)


# sign of each reference coordinate at local node n: bits (n ^ n >> 1) & 1, (n >> 1) & 1, (n >> 2) & 1
NODE_SIGNS = np.array([[2 * ((n ^ (n >> 1)) & 1) - 1, 2 * ((n >> 1) & 1) - 1, 2 * ((n >> 2) & 1) - 1] for n in range(8)])
# a point's sign bits are its index itself
POINT_SIGNS = np.array([[2 * (q & 1) - 1, 2 * ((q >> 1) & 1) - 1, 2 * ((q >> 2) & 1) - 1] for q in range(8)])


def _rotations():
    """signed axis permutations R with det R = +1; new local node i lies where R maps it: NODE_SIGNS[ROT[i]] = R NODE_SIGNS[i]"""
    out = []
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), dtype=int)
            for i in range(3):
                R[i, perm[i]] = sg[i]
            if round(np.linalg.det(R)) != 1:
                continue
            Y = NODE_SIGNS @ R.T
            out.append([int(np.nonzero((NODE_SIGNS == y).all(axis=1))[0][0]) for y in Y])
    return np.array(out)


HEX_ROTATIONS = _rotations()
assert len(HEX_ROTATIONS) == 24 and len({tuple(r) for r in HEX_ROTATIONS}) == 24
assert all(sorted(r) == list(range(8)) for r in HEX_ROTATIONS.tolist())
# new point q of a rotated element = old point POINT_MAPS[r][q]
POINT_MAPS = np.array([[hex_code(int(rot[hex_code(q)])) for q in range(8)] for rot in HEX_ROTATIONS])
assert (NODE_SIGNS[[hex_code(q) for q in range(8)]] == POINT_SIGNS).all()  # point q sits at node hex_code(q)


def point_jacobians(coords, conn):
    """det dx/dxi at the eight points (+-1/sqrt 3) of every element: [nelems][8]"""
    xi = POINT_SIGNS / np.sqrt(3.0)
    dN = np.empty((8, 8, 3))  # [point][node][direction]
    for k in range(3):
        o = [l for l in range(3) if l != k]
        dN[:, :, k] = 0.125 * NODE_SIGNS[None, :, k] * (1 + NODE_SIGNS[None, :, o[0]] * xi[:, None, o[0]]) * \
            (1 + NODE_SIGNS[None, :, o[1]] * xi[:, None, o[1]])
    return np.linalg.det(np.einsum("enx,qnk->eqxk", coords[conn], dN))


def face_defects(coords, conn):
    """per element the largest |x0 - x1 + x2 - x3| over its six faces relative to the face's diagonal: zero for a
    parallelepiped (node_rows_xlane_cases.face_defects)"""
    x = coords[conn]
    faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    return np.max([np.linalg.norm(x[:, a] - x[:, b] + x[:, c] - x[:, d], axis=1) / np.linalg.norm(x[:, c] - x[:, a], axis=1)
                   for a, b, c, d in faces], axis=0)


class Renumbering:
    """pn[n]: new id of old node n; pe[j]: old element of new element j; rot[j]: the rotation of new element j;
    ptmap[j][q]: the old point (of old element pe[j]) that is new point q of new element j"""

    def __init__(self, pn, pe, rot):
        self.pn, self.pe, self.rot = pn, pe, rot
        self.ptmap = POINT_MAPS[rot]

    def dofs(self, neq):
        """new index of every old dof, neq per node"""
        return (self.pn[:, None] * neq + np.arange(neq)).ravel()

    def nodal(self, v, neq):
        out = np.empty_like(v)
        out[self.dofs(neq)] = v
        return out

    def back(self, v, neq):
        """a nodal vector in the new numbering, in the old one"""
        return np.ascontiguousarray(v[self.dofs(neq)])

    def node_set(self, ids):
        return np.sort(self.pn[np.asarray(ids, dtype=np.int64)])

    def points(self, x):
        """a point field [e][pt][...]"""
        idx = self.ptmap.reshape(self.ptmap.shape + (1,) * (x.ndim - 2))
        return np.ascontiguousarray(np.take_along_axis(x[self.pe], idx, axis=1))

    def points_back(self, x):
        """a point field of the new numbering, in the old one"""
        idx = np.broadcast_to(self.ptmap.reshape(self.ptmap.shape + (1,) * (x.ndim - 2)), x.shape)
        tmp = np.empty_like(x)
        np.put_along_axis(tmp, idx, x, axis=1)
        out = np.empty_like(x)
        out[self.pe] = tmp
        return out

    def point_dofs(self, f):
        """a point field over the element's 32 unknowns [e][pt][24 u (node, direction) + 8 p (node)]: the adjoint history f"""
        rot = HEX_ROTATIONS[self.rot]                                           # [e][new local node] -> old local node
        cols = np.concatenate([(rot[:, :, None] * 3 + np.arange(3)).reshape(len(rot), 24), 24 + rot], axis=1)
        return np.ascontiguousarray(np.take_along_axis(self.points(f), cols[:, None, :], axis=2))

    def elems(self, es):
        return None if es is None else np.ascontiguousarray(np.asarray(es)[self.pe])

    def csr_block(self, old, new, data, i, j, neq=(3, 1)):
        """values of block (i, j) of a system on the graphs of backend `old`, laid out on the graphs of backend `new`"""
        import scipy.sparse as sp
        shape = (len(new.rowptr[i][j]) - 1, len(new.rowptr[j][i]) - 1)
        A = sp.csr_matrix((data, old.colidx[i][j], old.rowptr[i][j]), shape=shape).tocoo()
        # explicit zeros stay: the structure is carried over entry by entry
        M = sp.csr_matrix((A.data, (self.dofs(neq[i])[A.row], self.dofs(neq[j])[A.col])), shape=shape)
        M.sort_indices()
        assert np.array_equal(M.indptr, new.rowptr[i][j]) and np.array_equal(M.indices, new.colidx[i][j])
        return M.data


def renumber(coords, conn, seed, rot=None, window=None, elem_set=None):
    """(coords, conn, elem_set, record) of the same mesh with random node ids, random element order (window=w: shuffled only
    inside consecutive windows of w elements) and rotated local node order (rot=None: a random rotation per element; an
    int: that one for all; an array: per OLD element)"""
    rng = np.random.default_rng(seed)
    pn = rng.permutation(len(coords))
    c2 = np.empty_like(coords)
    c2[pn] = coords
    ne = len(conn)
    if window:
        pe = np.concatenate([s + rng.permutation(min(window, ne - s)) for s in range(0, ne, window)])
    else:
        pe = rng.permutation(ne)
    if rot is None:
        r = rng.integers(0, 24, ne)
    elif np.ndim(rot) == 0:
        r = np.full(ne, int(rot))
    else:
        r = np.asarray(rot)[pe]
    conn2 = np.take_along_axis(pn[conn][pe], HEX_ROTATIONS[r], axis=1)
    rec = Renumbering(pn, pe, r)
    return np.ascontiguousarray(c2), np.ascontiguousarray(conn2.astype(np.int32)), rec.elems(elem_set), rec


def node_elements(conn, nnodes=None):
    """per node the list of (element, local index), ascending in the element: the library's node -> element list"""
    out = [[] for _ in range(int(conn.max()) + 1 if nnodes is None else nnodes)]
    for e, row in enumerate(conn):
        for a, n in enumerate(row):
            out[n].append((e, a))
    return out


def element_bandwidth(conn):
    """max over the nodes of last - first element + 1 (plan_staged_assembly)"""
    return max(le[-1][0] - le[0][0] + 1 for le in node_elements(conn) if le)


def staged_plan(conn, min_chunk):
    """(chunk, number of chunks) plan_staged_assembly takes below 256: the bandwidth, at least min_chunk, rounded up to
    four; one chunk when four of them cover the mesh"""
    chunk = (max(element_bandwidth(conn), min_chunk) + 3) // 4 * 4
    if chunk * 4 >= len(conn):
        return len(conn), 1
    return chunk, (len(conn) + chunk - 1) // chunk


def _check_geometry(c_old, conn_old, c, conn):
    assert (point_jacobians(c_old, conn_old) > 0).all()
    assert (point_jacobians(c, conn) > 0).all()         # every rotated element keeps positive Jacobians at its points
    assert face_defects(c, conn).min() > 1e-3            # no element is a parallelepiped
    # (the 24 rotations applied to every element of the old mesh, not only the one each element drew)
    for rot in HEX_ROTATIONS:
        assert (point_jacobians(c_old, conn_old[:, rot]) > 0).all()


def _sequences(conn, nnodes):
    return [tuple(a for _, a in le) for le in node_elements(conn, nnodes)]


@functools.lru_cache(maxsize=None)
def brick433():
    """the unshuffled mesh of shuffled433 (parity_cases.mesh_of("hex8"))"""
    c, conn, sets = brick(4, 3, 3, 1.0, 0.8, 0.7)
    return jiggle(c, sets, 0.04), conn


SEED_433 = 3


@functools.lru_cache(maxsize=None)
def shuffled433(rot=None):
    """brick(4, 3, 3), jiggled, everything random (rot: one rotation for all elements instead): coords, conn, record"""
    c0, conn0 = brick433()
    c, conn, _, rec = renumber(c0, conn0, SEED_433, rot=rot)
    _check_geometry(c0, conn0, c, conn)
    if rot is not None:
        return c, conn, rec
    lists = node_elements(conn, len(c))
    interior = [le for le in lists if len(le) == 8]
    assert len(interior) == 12
    # every local index is the row index of some interior node's first element
    assert {le[0][1] for le in interior} == set(range(8)), sorted({le[0][1] for le in interior})
    # the sequence of local indices over a node's elements is not the brick's at most nodes with two or more elements
    seq_old, seq_new = _sequences(conn0, len(c0)), _sequences(conn, len(c))
    shared = [n for n in range(len(c0)) if len(seq_old[n]) >= 2]
    differ = sum(seq_new[rec.pn[n]] != seq_old[n] for n in shared)
    assert 2 * differ >= len(shared), (differ, len(shared))
    # on the brick an interior node's eight elements see it at eight distinct local indices; here some nodes are seen at
    # the same local index by two of their elements
    assert all(len(set(s)) == 8 for s in seq_old if len(s) == 8)
    assert any(len(set(s)) < len(s) for s in seq_new)
    # element e + 1 is not the x-neighbour any more: most consecutive elements share no node
    assert np.mean([len(set(conn[e]) & set(conn[e + 1])) == 0 for e in range(len(conn) - 1)]) > 0.3
    return c, conn, rec


@functools.lru_cache(maxsize=None)
def same_corner222(a):
    """brick(2, 2, 2), jiggled, every element rotated so that the centre node is its local node `a`; node ids and element
    order random: coords, conn, record"""
    c0, conn0, sets = brick(2, 2, 2, 1.0, 0.8, 0.7)
    c0 = jiggle(c0, sets, 0.1)
    centre = 13
    rng = np.random.default_rng(40 + a)
    rot = []
    for row in conn0:
        k = int(np.nonzero(row == centre)[0][0])
        fits = [r for r in range(24) if HEX_ROTATIONS[r][a] == k]  # conn_new[a] = conn_old[ROT[a]] = the centre
        assert len(fits) == 3
        rot.append(fits[rng.integers(0, 3)])
    c, conn, _, rec = renumber(c0, conn0, 50 + a, rot=np.array(rot))
    _check_geometry(c0, conn0, c, conn)
    le = node_elements(conn, len(c))[rec.pn[centre]]
    assert len(le) == 8 and all(loc == a for _, loc in le)
    return c, conn, rec


@functools.lru_cache(maxsize=None)
def pinched_shuffled():
    """pinched_bricks(), every node jiggled, renumbered: the sixteen-element node goes through two rounds of eight with
    arbitrary local indices: coords, conn, record"""
    c0, conn0 = pinched_bricks()
    c0 = jiggle(c0, {}, 0.04, seed=9)
    c, conn, _, rec = renumber(c0, conn0, 5)
    _check_geometry(c0, conn0, c, conn)
    le = max(node_elements(conn, len(c)), key=len)
    assert len(le) == 16
    for half in (le[:8], le[8:]):  # neither round of eight sees the node at eight distinct local indices
        assert len({loc for _, loc in half}) < 8
    return c, conn, rec


@functools.lru_cache(maxsize=None)
def bar_windowed():
    """brick(2, 2, 24), jiggled, random node ids and rotations, elements shuffled inside windows of eight: with
    set_stage_chunk(4) the staged assembly takes chunks of at most 20 elements and at least five of them go through the ring
    of three, each with an irregular share of the node rows: coords, conn, record"""
    c0, conn0, sets = brick(2, 2, 24, 0.3, 0.3, 3.0)
    c0 = jiggle(c0, sets, 0.02)
    c, conn, _, rec = renumber(c0, conn0, 7, window=8)
    _check_geometry(c0, conn0, c, conn)
    bw = element_bandwidth(conn)
    assert element_bandwidth(conn0) == 8 and 8 < bw <= 20, bw
    chunk, nchunks = staged_plan(conn, 4)
    assert chunk <= 20 and nchunks >= 5, (chunk, nchunks)
    # the plan is not the brick's: the nodes whose rows are summed after chunk k are no contiguous id range
    last = np.array([le[-1][0] // chunk for le in node_elements(conn, len(c))])
    assert all(np.ptp(np.nonzero(last == k)[0]) + 1 > (last == k).sum() for k in range(nchunks))
    return c, conn, rec


@functools.lru_cache(maxsize=None)
def shuffled433_two_sets():
    """shuffled433 with two parameter rows and an interleaved element set that travels with the elements:
    coords, conn, element set, parameters, record"""
    c0, conn0 = brick433()
    es0 = (np.random.default_rng(21).random(len(conn0)) < 0.4).astype(np.int32)
    c, conn, es, rec = renumber(c0, conn0, SEED_433, elem_set=es0)
    assert np.array_equal(conn, shuffled433()[1]) and 0 < es.sum() < len(es) and np.array_equal(es, es0[rec.pe])
    assert not np.array_equal(es, es0)
    return c, conn, es.astype(np.int32), [J2, J2_B], rec


@functools.lru_cache(maxsize=None)
def notched_shuffled():
    """notched_bar(16, 4, 4) (node degrees 8 .. 27, nodes with 1 .. 8 elements) renumbered: coords, conn, node sets, record.
    The notch flanks are not jiggled (the Krylov tests need the mesh, not its geometry)."""
    c0, conn0, sets = notched_bar(16, 4, 4)
    c, conn, _, rec = renumber(c0, conn0, 13)
    assert (point_jacobians(c, conn) > 0).all()
    return c, conn, {k: rec.node_set(v) for k, v in sets.items()}, rec


# the meshes node_rows_chain_cases.mesh / node_rows_xlane_cases.mesh know by these names
CHAIN_MESHES = ["same_corner222_a0", "same_corner222_a5", "pinched_shuffled", "shuffled433_two_sets"]


def chain_mesh(name):
    """coords, conn, element sets (or None), parameters: the tuple of node_rows_chain_cases.mesh"""
    if name.startswith("same_corner222_a"):
        c, conn, _ = same_corner222(int(name[-1]))
        return c, conn, None, J2
    if name == "pinched_shuffled":
        c, conn, _ = pinched_shuffled()
        return c, conn, None, J2
    if name == "shuffled433_two_sets":
        c, conn, es, prm, _ = shuffled433_two_sets()
        return c, conn, es, prm
    raise KeyError(name)


def histories(be, seed=11):
    """history terms that differ from entry to entry, on the numbering of `be`"""
    rng = np.random.default_rng(seed)
    return 1e-3 * rng.standard_normal((be.nelems, be.npts, be.nloc)), 1e-3 * rng.standard_normal((be.nelems, be.npts, 4 * be.nn))


def renumbered_pair_errors(rec, old, new, c_old):
    """K1 (system and state) and K3 (system) of backend `new` on the renumbered mesh against those of backend `old` on the
    old mesh through the maps.  prescribed_fields draws per node in id order, so the fields of the new mesh are the old
    mesh's carried over, not drawn again."""
    from meshes import prescribed_fields
    u, p = prescribed_fields(c_old, 0.004, ramp=True, perturb=5e-2)
    z, zp = np.zeros_like(u), np.zeros_like(p)
    res = []
    g, f = histories(old)
    for be, uu, pp, gg, ff in ((old, u, p, g, f), (new, rec.nodal(u, 3), rec.nodal(p, 1), rec.points(g), rec.point_dofs(f))):
        ls, xi, la = be.new_linsys(), be.new_state(), be.new_linsys()
        assert be.forward_jacobian(uu, pp, z, zp, be.new_state(), xi, ls) == 0
        assert be.adjoint_jacobian(uu, pp, z, zp, be.new_state(), xi, gg.copy(), ff, la) in (0, None)
        res.append((ls, xi, la))
    (l0, x0, a0), (l1, x1, a1) = res
    assert 0.3 < (x0[:, :, -1] > 0).mean() < 1.0  # plastic and elastic points
    errs = equivariance_errors(rec, old, new, l0, x0, l1, x1)
    errs.update({"K3 " + k: v for k, v in equivariance_errors(rec, old, new, a0, x0, a1, x1).items() if k != "xi"})
    return errs, (x0, x1)


def equivariance_errors(rec, old, new, ls_old, xi_old, ls_new, xi_new):
    """deviations of a system and state on the renumbered mesh from the ones on the old mesh carried through the maps, each
    against the largest entry"""
    xm = rec.points(xi_old)
    errs = {"xi": float(np.abs(xi_new - xm).max() / np.abs(xm).max())}
    neq = (3, 1)
    for i in range(2):
        bm = rec.nodal(ls_old.b[i], neq[i])
        errs["b%d" % i] = float(np.abs(ls_new.b[i] - bm).max() / np.abs(bm).max())
        for j in range(2):
            M = rec.csr_block(old, new, ls_old.A[i][j], i, j)
            errs["A%d%d" % (i, j)] = float(np.abs(ls_new.A[i][j] - M).max() / np.abs(M).max())
    return errs
