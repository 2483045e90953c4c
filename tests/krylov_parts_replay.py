"""The two-level preconditioner over parts (C8_PRECOND_TWO_LEVEL_PARTS) by its definition in
include/c8.h, in numpy on the GATHERED matrix: unknowns ordered as tests/test_gpu_krylov_parts.py::check_contract orders them
(u of the global nodes, then p).  No device and no library: tests/test_gpu_krylov_two_level_parts.py compares the device with
it, and the CPU iteration counts of section 13f come from it.

A part is a dict: gid (global ids of its OWNED nodes in local order), agg (local aggregate of every owned node), nagg, base
(aggregates of the parts below it), colors (list of arrays of local owned ids, one per colour of the part-local sweeps)."""
import numpy as np


def aggregate_replay(rowptr, colidx, n):
    """the three passes of include/c8.h over a node graph: (aggregate of every node, number of aggregates)"""
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


def owned_subgraph(rowptr, colidx, no):
    """rows of the first `no` nodes of a node graph with the columns >= no dropped"""
    rp, ci = np.asarray(rowptr), np.asarray(colidx)
    rows = [ci[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] < no] for i in range(no)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, (np.concatenate(rows) if no else np.zeros(0, dtype=np.int64))


def owned_aggregates(rowptr, colidx, no):
    """the aggregates of a part: the three passes over its owned sub-graph"""
    return aggregate_replay(*owned_subgraph(rowptr, colidx, no), no)


def greedy_colors(rowptr, colidx, n):
    """the colouring rule of include/c8.h over the sub-graph of the first n nodes"""
    color = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        nb = colidx[rowptr[i]:rowptr[i + 1]]
        used = set(color[nb[nb < i]].tolist())
        k = 0
        while k in used:
            k += 1
        color[i] = k
    return [np.nonzero(color == k)[0] for k in range(int(color.max()) + 1)] if n else []


def global_index(N, nd, nres):
    """idx[node, k]: position of equation k of global node `node` in the gathered vector"""
    nb = nd + (1 if nres == 2 else 0)
    idx = np.zeros((N, nb), dtype=np.int64)
    for k in range(nb):
        idx[:, k] = np.arange(N) * nd + k if k < nd else N * nd + np.arange(N)
    return idx


def node_of_unknown(N, nd, nres):
    return np.concatenate([np.repeat(np.arange(N), nd)] + ([np.arange(N)] if nres == 2 else []))


def gathered_matrix(pieces, N, neq, nres):
    """the global owned system from the ranks' pieces of test_gpu_krylov_parts.owned_piece: (A, b)"""
    import scipy.sparse as sp
    off = [0, N * neq[0]]
    n = N * sum(neq[:nres])
    bg = np.zeros(n)
    R, Cc, V = [], [], []
    for q in pieces:
        rows = [off[i] + np.repeat(q["gid"][: q["no"]], neq[i]) * neq[i] + np.tile(np.arange(neq[i]), q["no"]) for i in range(nres)]
        for i in range(nres):
            bg[rows[i]] = q["b"][i]
            for j in range(nres):
                rp, ci, vals = q["A"][(i, j)]
                R.append(np.repeat(rows[i], np.diff(rp)))
                Cc.append(off[j] + q["gid"][ci // neq[j]] * neq[j] + ci % neq[j])
                V.append(vals)
    return sp.csr_matrix((np.concatenate(V), (np.concatenate(R), np.concatenate(Cc))), shape=(n, n)), bg


def constrained_rows(A):
    """rows of A whose off-diagonal entries are all exactly 0"""
    off = A.tocsr().copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    return np.diff(off.indptr) == 0


def prolongator(A, coords, nd, nres, parts):
    """P of include/c8.h over all parts as a SciPy matrix: (P, global aggregate of every node, number of aggregates)"""
    import scipy.sparse as sp
    N = len(coords)
    nc = nd + (3 if nd == 3 else 1) + (1 if nres == 2 else 0)
    idx = global_index(N, nd, nres)
    x = np.asarray(coords)[:, :nd]
    gagg, d = np.full(N, -1, dtype=np.int64), np.zeros((N, nd))
    total = 0
    for q in parts:
        assert q["base"] == total        # the prefix sums, in rank order
        gid = np.asarray(q["gid"])
        gagg[gid] = q["base"] + np.asarray(q["agg"])
        for a in range(q["nagg"]):
            nodes = gid[np.nonzero(np.asarray(q["agg"]) == a)[0]]     # members in ascending LOCAL id
            d[nodes] = x[nodes] - np.cumsum(x[nodes], axis=0)[-1] / len(nodes)
        total += q["nagg"]
    assert (gagg >= 0).all()
    rows, cols, vals = [], [], []

    def put(eq, col, v):
        rows.append(idx[:, eq])
        cols.append(gagg * nc + col)
        vals.append(v * np.ones(N))
    for m in range(nd):
        put(m, m, 1.0)
    if nd == 3:
        for m in range(3):
            rot = np.cross(np.eye(3)[m], d)
            for r in range(3):
                put(r, 3 + m, rot[:, r])
    else:
        put(0, 2, -d[:, 1])
        put(1, 2, d[:, 0])
    if nres == 2:
        put(nd, nc - 1, 1.0)
    P = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(A.shape[0], total * nc))
    P = sp.diags((~constrained_rows(A)).astype(float)) @ P
    P.eliminate_zeros()
    return P.tocsr(), gagg, total


def coarse_replay(A, P):
    """A_c = P^T A P with a unit diagonal where a column of P is zero"""
    Ac = (P.T @ A @ P).toarray()
    zero = np.nonzero(np.diff(P.tocsc().indptr) == 0)[0]
    Ac[zero, zero] = 1.0
    return Ac


def part_local_matrix(A, N, nd, nres, parts):
    """A with the entries dropped whose row and column nodes have different owners: what the part-local sweeps see"""
    owner = np.full(N, -1, dtype=np.int64)
    for r, q in enumerate(parts):
        owner[np.asarray(q["gid"])] = r
    node = node_of_unknown(N, nd, nres)
    C = A.tocoo()
    keep = owner[node[C.row]] == owner[node[C.col]]
    import scipy.sparse as sp
    return sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)


class PartLocalSGS:
    """the symmetric multicolour sweeps of every part on its own rows and columns, started from x0; colour k of all parts is
    one step (nodes of different parts do not couple in the part-local matrix)"""

    def __init__(self, A, N, nd, nres, parts, sweeps=1):
        self.sweeps = sweeps
        self.idx = global_index(N, nd, nres)
        B = part_local_matrix(A, N, nd, nres, parts)
        nb = self.idx.shape[1]
        D = np.stack([np.asarray(B[self.idx[:, r]][:, self.idx[:, c]].diagonal()) for r in range(nb) for c in range(nb)], axis=1).reshape(N, nb, nb)
        self.Dinv = np.linalg.inv(D)
        # every part runs its own sequence 0 .. nc_r - 1, nc_r - 2 .. 0; parts are independent, so they are replayed in turn
        self.steps = []
        for q in parts:
            gid, nc = np.asarray(q["gid"]), len(q["colors"])
            cols = [gid[np.asarray(c)] for c in q["colors"]]
            seq = list(range(nc)) + list(range(nc - 2, -1, -1))
            self.steps.append([(cols[k], self.idx[cols[k]].ravel(), B[self.idx[cols[k]].ravel()]) for k in seq])

    def apply(self, v, x0=None):
        v = np.asarray(v, dtype=np.float64)
        x = np.zeros(v.shape) if x0 is None else np.array(x0, dtype=np.float64)
        nb = self.idx.shape[1]
        for steps in self.steps:
            for _ in range(self.sweeps):
                for nodes, rows, Brows in steps:
                    r = (v[rows] - Brows @ x).reshape(-1, nb)
                    x[rows] += np.einsum("nij,nj->ni", self.Dinv[nodes], r).ravel()
        return x


class TwoLevelParts:
    """y = M^-1 v of C8_PRECOND_TWO_LEVEL_PARTS: x = P A_c^-1 P^T v, then the part-local sweeps started from x"""

    def __init__(self, A, coords, nd, nres, parts, sweeps=1):
        import scipy.linalg as sl
        self.P, self.gagg, self.nagg = prolongator(A, coords, nd, nres, parts)
        self.Ac = coarse_replay(A, self.P)
        self.lu = sl.lu_factor(self.Ac)
        self.sgs = PartLocalSGS(A, len(coords), nd, nres, parts, sweeps)

    def coarse(self, v):
        import scipy.linalg as sl
        return self.P @ sl.lu_solve(self.lu, self.P.T @ np.asarray(v, dtype=np.float64))

    def apply(self, v):
        return self.sgs.apply(v, self.coarse(v))


def parts_of_graph(rowptr, colidx, owner, world):
    """The parts of a global node graph by the host rules alone (owned nodes in ascending global id, as
    calibr8_amd.distributed orders them): aggregates and colours of every part over its owned sub-graph."""
    rp, ci = np.asarray(rowptr), np.asarray(colidx)
    parts, base = [], 0
    for r in range(world):
        gid = np.nonzero(owner == r)[0]
        loc = np.full(len(owner), -1, dtype=np.int64)
        loc[gid] = np.arange(len(gid))
        rows = [np.sort(loc[ci[rp[g]:rp[g + 1]]][loc[ci[rp[g]:rp[g + 1]]] >= 0]) for g in gid]
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
        col = np.concatenate(rows) if len(rows) else np.zeros(0, dtype=np.int64)
        agg, nagg = aggregate_replay(ptr, col, len(gid))
        parts.append({"gid": gid, "agg": agg, "nagg": nagg, "base": base, "colors": greedy_colors(ptr, col, len(gid))})
        base += nagg
    return parts
