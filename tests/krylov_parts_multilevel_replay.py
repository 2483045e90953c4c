"""The multilevel preconditioner over parts (C8_PRECOND_MULTILEVEL_PARTS) by its definition in
include/c8.h, in numpy on the GATHERED matrix (unknowns ordered as tests/krylov_parts_replay.py orders them).  No device and
no library: tests/test_gpu_krylov_multilevel_parts.py compares the device with it, and the CPU iteration counts of section
13g come from it (`python tests/krylov_parts_multilevel_replay.py`, which needs the CPU oracle).

Level 0 is that of krylov_parts_replay (parts, P_0, the part-local sweeps).  Level 1 has one node per aggregate of any part,
by global id; its graph comes from the global node graph (the node pattern of the gathered matrix) under the global aggregate
ids, its positions are the centroids.  The levels below follow by the rules of the single-part multilevel kind on that graph:
aggregate_replay, greedy_colors, next_graph, centroids, level_prolongator, coloured block sweeps."""
import numpy as np

import krylov_parts_replay as R


def next_graph(rp, ci, agg, nagg):
    """graph of the next level: I and J are neighbours when a node of I has a graph column in J (self included); rows sorted"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    pairs = np.unique(np.asarray(agg)[rows] * nagg + np.asarray(agg)[np.asarray(ci)])
    return np.concatenate([[0], np.cumsum(np.bincount(pairs // nagg, minlength=nagg))]).astype(np.int64), pairs % nagg


def node_graph(A, N, nd, nres):
    """the node graph behind the gathered matrix: (i, j) wherever an entry of node i's rows is stored in node j's columns
    (stored zeros count: the Dirichlet rows keep their pattern)"""
    node = R.node_of_unknown(N, nd, nres)
    C = A.tocoo()
    pairs = np.unique(node[C.row] * N + node[C.col])
    return np.concatenate([[0], np.cumsum(np.bincount(pairs // N, minlength=N))]).astype(np.int64), pairs % N


def global_aggregates(parts, N):
    """global aggregate of every global node (base of the part + local id) and their number"""
    gagg = np.full(N, -1, dtype=np.int64)
    for q in parts:
        gagg[np.asarray(q["gid"])] = q["base"] + np.asarray(q["agg"])
    assert (gagg >= 0).all()
    return gagg, sum(q["nagg"] for q in parts)


def level1_graph(rowptr, colidx, parts, N):
    """the level-1 graph of the definition from the GLOBAL node graph: an owned node of I has a column whose owner put it
    into J.  Every node is owned by one part, so this is next_graph under the global aggregate ids."""
    gagg, total = global_aggregates(parts, N)
    return next_graph(np.asarray(rowptr), np.asarray(colidx), gagg, total)


def part_centroids(x, parts):
    """centroids of the aggregates of all parts by global id: unweighted mean of the members, summed in ascending LOCAL id"""
    out = np.zeros((sum(q["nagg"] for q in parts), x.shape[1]))
    for q in parts:
        gid, agg = np.asarray(q["gid"]), np.asarray(q["agg"])
        for a in range(q["nagg"]):
            nodes = gid[np.nonzero(agg == a)[0]]
            out[q["base"] + a] = np.cumsum(x[nodes], axis=0)[-1] / len(nodes)
    return out


def centroids(x, agg, nagg):
    out = np.zeros((nagg, x.shape[1]))
    for a in range(nagg):
        nodes = np.nonzero(agg == a)[0]
        out[a] = np.cumsum(x[nodes], axis=0)[-1] / len(nodes)
    return out


def levels_below(rp, ci, x, nc, coarse_max, max_levels):
    """the levels from level 1 down as dicts n, rp, ci, x and, where a level below exists, agg, nagg, colors.  Level 1 is
    given and always exists; another level is built while n_l x nc > coarse_max, fewer than max_levels levels exist (level 0
    counts) and aggregation still reduces the node count."""
    levels = [dict(n=len(rp) - 1, rp=np.asarray(rp), ci=np.asarray(ci), x=np.asarray(x))]
    while levels[-1]["n"] * nc > coarse_max and len(levels) + 1 < max_levels:
        cur = levels[-1]
        agg, nagg = R.aggregate_replay(cur["rp"], cur["ci"], cur["n"])
        if nagg >= cur["n"]:
            break
        cur.update(agg=agg, nagg=nagg, colors=R.greedy_colors(cur["rp"], cur["ci"], cur["n"]))
        rp2, ci2 = next_graph(cur["rp"], cur["ci"], agg, nagg)
        levels.append(dict(n=nagg, rp=rp2, ci=ci2, x=centroids(cur["x"], agg, nagg)))
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


def dense_coarse(Al, P):
    """P^T A_l P with a unit diagonal where a column of P is zero"""
    out = P.T @ Al @ P
    zero = np.nonzero(~P.any(axis=0))[0]
    out[zero, zero] = 1.0
    return out


class LevelSGS:
    """`sweeps` symmetric multicolour block Gauss-Seidel sweeps on a dense block level (nc unknowns per node), every colour
    over the whole row: colours 0 .. k - 1, then k - 2 .. 0"""

    def __init__(self, Al, nc, colors, sweeps=1):
        n = Al.shape[0] // nc
        self.A, self.nc, self.sweeps = Al, nc, sweeps
        self.D = np.stack([Al[i * nc:(i + 1) * nc, i * nc:(i + 1) * nc] for i in range(n)])
        self.Dinv = np.linalg.inv(self.D)
        seq = list(range(len(colors))) + list(range(len(colors) - 2, -1, -1))
        idx = np.arange(n * nc).reshape(n, nc)
        self.steps = [(np.asarray(colors[k]), idx[np.asarray(colors[k])].ravel()) for k in seq]

    def sgs_from(self, v, x0):
        x = np.array(x0, dtype=np.float64)
        for _ in range(self.sweeps):
            for nodes, rows in self.steps:
                r = (v[rows] - self.A[rows] @ x).reshape(-1, self.nc)
                x[rows] += np.einsum("nij,nj->ni", self.Dinv[nodes], r).ravel()
        return x


class MultilevelParts:
    """the levels, every P_l and A_l, and y = M^-1 v of C8_PRECOND_MULTILEVEL_PARTS.  levels[k], A[k], for k >= 1, are level
    k's; A1 replaces P_0^T A P_0 (the controls of the tests)."""

    def __init__(self, A, coords, nd, nres, parts, coarse_max=1024, max_levels=8, sweeps=1, A1=None):
        import scipy.linalg as sl
        N = len(coords)
        nc = nd + (3 if nd == 3 else 1) + (1 if nres == 2 else 0)
        self.nc, self.sweeps = nc, sweeps
        self.P0, self.gagg, self.total = R.prolongator(A, coords, nd, nres, parts)
        self.sgs0 = R.PartLocalSGS(A, N, nd, nres, parts, sweeps)
        rp0, ci0 = node_graph(A, N, nd, nres)
        rp1, ci1 = level1_graph(rp0, ci0, parts, N)
        x1 = part_centroids(np.asarray(coords)[:, :nd], parts)
        self.levels = [None] + levels_below(rp1, ci1, x1, nc, coarse_max, max_levels)
        last = len(self.levels) - 1
        self.A = [A, R.coarse_replay(A, self.P0) if A1 is None else A1]
        self.P, self.rep = [self.P0], [None]
        for lev in range(1, last):
            L, Al = self.levels[lev], self.A[lev]
            P = level_prolongator(Al, L["x"], L["agg"], L["nagg"], nd, nc)
            self.P.append(P)
            self.A.append(dense_coarse(Al, P))
            self.rep.append(LevelSGS(Al, nc, L["colors"], sweeps))
        self.lu = sl.lu_factor(self.A[last])
        # what the device inverts: the last level and the diagonal blocks of every other one, the node blocks of level 0 included
        self.cond_last = float(np.linalg.cond(self.A[last]))
        self.cond_blocks = max([float(np.linalg.cond(self.sgs0.Dinv).max())] + [float(np.linalg.cond(r.D).max()) for r in self.rep[1:]])
        self.cond = max(self.cond_last, self.cond_blocks)

    def set_sweeps(self, sweeps):
        self.sweeps = self.sgs0.sweeps = sweeps
        for r in self.rep[1:]:
            r.sweeps = sweeps

    def cycle(self, r, lev=1, lower=True):
        """e_lev = M_lev^-1 r; lower = False leaves the levels below `lev` out (the sweeps start from zero)"""
        import scipy.linalg as sl
        if lev == len(self.levels) - 1:
            return sl.lu_solve(self.lu, r)
        x0 = self.P[lev] @ self.cycle(self.P[lev].T @ r, lev + 1) if lower else np.zeros(len(r))
        return self.rep[lev].sgs_from(r, x0)

    def apply(self, v, lower=True):
        v = np.asarray(v, dtype=np.float64)
        return self.sgs0.apply(v, self.P0 @ self.cycle(self.P0.T @ v, 1, lower))


# ---- the CPU table of DESIGN.md section 13g -----------------------------------------------------------------------------------
def slab_owner(c, conn, world):
    """elements cut into x-slabs of equal width; a shared node is owned by the lowest part"""
    xm = c[conn].mean(axis=1)[:, 0]
    lo, hi = c[:, 0].min(), c[:, 0].max()
    ep = np.minimum(((xm - lo) / (hi - lo) * world).astype(np.int64), world - 1)
    owner = np.full(len(c), world)
    for r in range(world - 1, -1, -1):
        owner[np.unique(conn[ep == r])] = r
    return owner


def oracle_system(n):
    """the oracle's K1 Jacobian of small_J2 on notched_bar(*n) with the state and the Dirichlet rows of device_system, in the
    gathered ordering (u of the nodes, then p)"""
    import scipy.sparse as sp
    import oracle_lib as ol
    from meshes import notched_bar, prescribed_fields
    from parity_cases import J2
    c, conn, s = notched_bar(*n)
    orc = ol.Oracle(ol.HEX8, c, conn, "small_J2", J2)
    u, p = prescribed_fields(c, 0.004, ramp=True)
    ls, xi = orc.new_linsys(), orc.new_state()
    assert orc.forward_jacobian(u, p, np.zeros_like(u), np.zeros_like(p), orc.new_state(), xi, ls) == 0
    N = len(c)
    neq = (3, 1)
    blocks = [[sp.csr_matrix((np.asarray(ls.A[i][j]), orc.colidx[i][j], orc.rowptr[i][j]), shape=(N * neq[i], N * neq[j])) for j in range(2)]
              for i in range(2)]
    A = sp.bmat(blocks, format="lil")
    b = np.concatenate([np.asarray(ls.b[0]), np.asarray(ls.b[1])])
    rows = np.concatenate([np.asarray(s["xmin"]) * 3 + d for d in range(3)] + [np.asarray(s["xmax"]) * 3])
    x = np.concatenate([np.asarray(u, dtype=np.float64).ravel(), np.asarray(p, dtype=np.float64).ravel()])
    for r in rows:     # c8_apply_dirichlet: the diagonal entry stays, the rest of the row is zeroed in place, b = diag * (x - 0)
        A.data[r] = [v if k == r else 0.0 for k, v in zip(A.rows[r], A.data[r])]
        b[r] = A[r, r] * x[r]
    return c, conn, A.tocsr(), b


def count(A, b, apply):
    import scipy.sparse.linalg as spla
    it = [0]

    def cb(_):
        it[0] += 1
    x, flag = spla.bicgstab(A, b, rtol=1e-10, atol=0.0, maxiter=20000, M=spla.LinearOperator(A.shape, matvec=apply), callback=cb)
    assert flag == 0
    return it[0]


def table(cases=(((16, 4, 4), 2), ((16, 4, 4), 4), ((32, 8, 8), 2), ((32, 8, 8), 4))):
    import scipy.sparse as sp
    for n, world in cases:
        c, conn, A, b = oracle_system(n)
        N = len(c)
        rp, ci = node_graph(A, N, 3, 2)
        parts = R.parts_of_graph(rp, ci, slab_owner(c, conn, world), world)
        two = R.TwoLevelParts(A, c, 3, 2, parts)
        row = ["%s (%d), %d parts, aggregates %s" % (n, A.shape[0], world, " + ".join(str(q["nagg"]) for q in parts)),
               "part-local SGS %d" % count(A, b, two.sgs.apply), "two levels %d" % count(A, b, two.apply)]
        for coarse_max in (100, 20):
            op = MultilevelParts(A, c, 3, 2, parts, coarse_max=coarse_max)
            row.append("coarse_max %d: %s -> %d" % (coarse_max, " / ".join(str(L["n"]) for L in op.levels[1:]), count(A, b, op.apply)))
        if n == (16, 4, 4):
            op = MultilevelParts(A, c, 3, 2, parts, coarse_max=100)
            v = np.random.default_rng(13).standard_normal(A.shape[0])
            y = op.apply(v)
            rel = lambda z: np.linalg.norm(z - y) / np.linalg.norm(y)
            row.append("controls: no lower levels %.1e, two levels %.1e, sweeps alone %.1e, bound %.1e" %
                       (rel(op.apply(v, lower=False)), rel(two.apply(v)), rel(two.sgs.apply(v)), 100 * np.finfo(float).eps * op.cond))
        print(" | ".join(row), flush=True)


if __name__ == "__main__":
    import os
    import sys
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
    table()
