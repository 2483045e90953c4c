"""TEST INFRASTRUCTURE shared by test_spr_host.py and test_gpu_spr.py: the meshes of the superconvergent patch recovery
checks (small on purpose), the references, and the host harness (tests/spr_host) around calibr8_amd/csrc/c8_spr.hpp.

The patch reference is a set-based restatement of the rules of cspr.cpp as include/c8.h states them; the value reference is
numpy.linalg.lstsq on the centred, scaled fit matrix, which also gives that matrix's condition number per node."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import meshes

HERE = os.path.dirname(os.path.abspath(__file__))
TRI3, TET4, HEX8 = 3, 4, 8
CXXFLAGS = ["-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-unused-but-set-variable"]
dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
RANK_TOL = 1e-8
STAGE_RULE = {TET4: (3, 2, 1), HEX8: (4, 2, 1), TRI3: (2, 1)}  # nodes in common for "shares a (d-1)-, ..., 0-entity"


class HopeLost(Exception):
    def __init__(self, node):
        super().__init__("all hope is lost at node %d" % node)
        self.node = node


# ---- meshes -----------------------------------------------------------------------------------------------------------
def tet_split(n, jig=0.0, seed=3, interior=False):
    """brick(n, n, n) cut into six tet4 per cell round the diagonal 0-6; jig: EVERY node moved by up to jig * h per axis, so
    that the coplanar centroids of the patches at the ends of a cell diagonal become nearly coplanar (accepted, condition
    number in the hundreds); interior: the interior nodes alone, as meshes.jiggle does for the other element types"""
    nx, ny, nz = (n, n, n) if isinstance(n, int) else n
    c, hexes, sets = meshes.brick(nx, ny, nz)
    if jig:
        c = meshes.jiggle(c, sets if interior else {}, 2.0 * jig / nx, seed=seed)
    tets = []
    for h in hexes:
        for a, b in ((1, 2), (2, 3), (3, 7), (7, 4), (4, 5), (5, 1)):
            t = [h[0], h[a], h[b], h[6]]
            if np.linalg.det(c[t[1:]] - c[t[0]]) < 0:
                t[1], t[2] = t[2], t[1]
            tets.append(t)
    return np.ascontiguousarray(c), np.array(tets, dtype=np.int32)


def fan(nt=66):
    """a two-ring fan: nt triangles round the centre node 0, a second ring of 2 nt triangles round them"""
    th = 2.0 * np.pi * np.arange(nt) / nt
    r1 = 1.0 + 0.1 * np.sin(3.0 * th)
    r2 = 2.0 + 0.15 * np.cos(5.0 * th)
    ring = lambda r, t: np.stack([r * np.cos(t), r * np.sin(t), np.zeros(nt)], axis=1)
    coords = np.concatenate([np.zeros((1, 3)), ring(r1, th), ring(r2, th + np.pi / nt)])
    tris = []
    for k in range(nt):
        i0, i1, o0, o1 = 1 + k, 1 + (k + 1) % nt, 1 + nt + k, 1 + nt + (k + 1) % nt
        tris += [[0, i0, i1], [i0, o0, i1], [i1, o0, o1]]
    return np.ascontiguousarray(coords), np.array(tris, dtype=np.int32)


def _hex(n, jig=0.0):
    c, conn, sets = meshes.brick(n, n, n)
    return np.ascontiguousarray(meshes.jiggle(c, sets, jig) if jig else c), conn


def _renumbered(mesh_, seed):
    import renumber_cases
    c, conn, _, _ = renumber_cases.renumber(mesh_[0], mesh_[1], seed)
    return c, conn


def _tri(nx, ny, jig=0.0):
    c, conn, sets = meshes.tri_mesh(nx, ny)
    return np.ascontiguousarray(meshes.jiggle_2d(c, sets, jig) if jig else c), conn


_MAKERS = {
    "brick1": lambda: (HEX8,) + _hex(1), "brick2": lambda: (HEX8,) + _hex(2), "brick3": lambda: (HEX8,) + _hex(3),
    "pinched_bricks": lambda: (HEX8,) + meshes.pinched_bricks(),
    "tet1": lambda: (TET4,) + tet_split(1), "tet2": lambda: (TET4,) + tet_split(2), "tet3": lambda: (TET4,) + tet_split(3),
    "tri11": lambda: (TRI3,) + _tri(1, 1), "tri22": lambda: (TRI3,) + _tri(2, 2), "tri33": lambda: (TRI3,) + _tri(3, 3),
    "tri61": lambda: (TRI3,) + _tri(6, 1), "fan": lambda: (TRI3,) + fan(),
    "fan64": lambda: (TRI3,) + fan(64),  # the widest fan a context takes: c8_create colours the elements round a node with at most 64 colours
    "tet3_jiggled": lambda: (TET4,) + tet_split(3, 0.08),
    "tet3_interior": lambda: (TET4,) + tet_split(3, 0.08, interior=True),
    # node counts on both sides of a launch block of k_spr_apply (16 nodes per block on hex8, 32 on tet4 and tri3)
    "brick221": lambda: (HEX8,) + meshes.brick(2, 2, 1)[:2], "tet223": lambda: (TET4,) + tet_split((2, 2, 3)),
    "tri73": lambda: (TRI3,) + _tri(7, 3), "tri102": lambda: (TRI3,) + _tri(10, 2),
    "brick3_jiggled": lambda: (HEX8,) + _hex(3, 0.05), "tri33_jiggled": lambda: (TRI3,) + _tri(3, 3, 0.05),
    # random node ids, random element order, a random rotation of every element's local nodes (renumber_cases.py)
    "brick3_jiggled_renumbered": lambda: (HEX8,) + _renumbered(_hex(3, 0.05), 31),
    "pinched_bricks_renumbered": lambda: (HEX8,) + _renumbered(meshes.pinched_bricks(), 32),
}
TABLE = ("brick1", "brick2", "brick3", "pinched_bricks", "tet1", "tet2", "tet3", "tri11", "tri22", "tri33", "tri61", "fan", "tet3_jiggled")
HOPELESS = ("tet1", "tri11")
GOOD = tuple(k for k in TABLE if k not in HOPELESS)
AFFINE = ("brick3_jiggled", "tet3_interior", "tri33_jiggled", "fan")


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(elem_type, coords [n][3], conn)"""
    et, c, conn = _MAKERS[name]()
    c.setflags(write=False)
    conn.setflags(write=False)
    return et, c, conn


# ---- references --------------------------------------------------------------------------------------------------------
def dims(et):
    return 2 if et == TRI3 else 3


def shape_values(et):
    """[points of ip set 0][nodes]: the element kit of c8_element.hpp restated"""
    if et == TET4:
        return np.full((1, 4), 0.25)
    if et == TRI3:
        return np.full((1, 3), 1.0 / 3.0)
    g = 1.0 / np.sqrt(3.0)
    N = np.zeros((8, 8))
    for pt in range(8):
        xi = [g if pt & 1 else -g, g if pt & 2 else -g, g if pt & 4 else -g]
        for n in range(8):
            s = [1.0 if (n ^ (n >> 1)) & 1 else -1.0, 1.0 if (n >> 1) & 1 else -1.0, 1.0 if (n >> 2) & 1 else -1.0]
            N[pt, n] = 0.125 * (1 + s[0] * xi[0]) * (1 + s[1] * xi[1]) * (1 + s[2] * xi[2])
    return N


def sample_points(et, coords, conn):
    """[nelems][points][dims]: the isoparametric map of the coupled points"""
    return np.einsum("pn,end->epd", shape_values(et), coords[conn][:, :, :dims(et)])


def fit_matrix(et, coords, pts, node, patch):
    """the centred, scaled fit matrix of a patch (elements ascending, points in order) and h"""
    x = pts[sorted(patch)].reshape(-1, dims(et)) - coords[node, :dims(et)]
    h = np.abs(x).max()
    return np.concatenate([np.ones((len(x), 1)), x / h], axis=1), h


def _accepted(et, coords, pts, node, patch):
    T = dims(et) + 1
    if pts.shape[1] * len(patch) < 1.1 * T:
        return False
    A, _ = fit_matrix(et, coords, pts, node, patch)
    if len(A) < T:
        return False
    R = np.linalg.qr(A, mode="r")
    return bool(np.abs(np.diag(R)).min() > RANK_TOL * np.sqrt(len(A)))


@functools.lru_cache(maxsize=None)
def patches_ref(name):
    """(list of sorted element lists per node, stages per node, reasons per node) by the rules, with Python sets; raises
    HopeLost.  reason: "" (no expansion), "points" or "rank" (what the initial patch lacked)."""
    et, coords, conn = mesh(name)
    pts = sample_points(et, coords, conn)
    node_elems = [set() for _ in range(len(coords))]
    for e, row in enumerate(conn):
        for n in row:
            node_elems[n].add(e)
    nodes_of = [frozenset(int(n) for n in row) for row in conn]
    out, stages, reasons = [], [], []
    for n in range(len(coords)):
        patch = set(node_elems[n])
        st, reason = 0, ""
        if not _accepted(et, coords, pts, n, patch):
            reason = "points" if pts.shape[1] * len(patch) < 1.1 * (dims(et) + 1) else "rank"
            done = False
            while not done:
                old = frozenset(patch)
                for common in STAGE_RULE[et]:
                    for e in old:
                        for f in set().union(*[node_elems[a] for a in nodes_of[e]]):
                            if len(nodes_of[e] & nodes_of[f]) >= common:
                                patch.add(f)
                    st += 1
                    if _accepted(et, coords, pts, n, patch):
                        done = True
                        break
                if not done and len(patch) == len(old):
                    raise HopeLost(n)
        out.append(sorted(patch))
        stages.append(st)
        reasons.append(reason)
    return out, np.array(stages, dtype=np.int32), reasons


def lstsq_ref(name, patches, field):
    """(nodal [nnodes][ncomp], kappa [nnodes], vmax [nnodes]): numpy.linalg.lstsq on the centred, scaled matrix; kappa its
    condition number, vmax the largest sample magnitude of the patch"""
    et, coords, conn = mesh(name)
    pts = sample_points(et, coords, conn)
    field = field.reshape(len(conn), pts.shape[1], -1)
    nodal, kappa, vmax = np.zeros((len(coords), field.shape[2])), np.zeros(len(coords)), np.zeros(len(coords))
    for n, patch in enumerate(patches):
        A, _ = fit_matrix(et, coords, pts, n, patch)
        V = field[sorted(patch)].reshape(len(A), -1)
        nodal[n] = np.linalg.lstsq(A, V, rcond=None)[0][0]
        kappa[n] = np.linalg.cond(A)
        vmax[n] = np.abs(V).max()
    return nodal, kappa, vmax


def as_lists(tab):
    return [list(tab["patch_elems"][tab["patch_ptr"][n]:tab["patch_ptr"][n + 1]]) for n in range(len(tab["patch_ptr"]) - 1)]


# ---- the host side of the product -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_tables(name):
    """c8_spr_build_host of libc8.so (no device)"""
    from calibr8_amd import spr_build_host
    et, coords, conn = mesh(name)
    return spr_build_host(et, coords, conn)


class Harness:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libsprhost.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-shared", "-o", so, os.path.join(HERE, "spr_host", "spr_host.cpp")])
        L = self.L = C.CDLL(so)
        L.spr_host_fit.restype = C.c_double
        L.spr_host_fit.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp]
        L.spr_host_points.restype = None
        L.spr_host_points.argtypes = [C.c_int, C.c_int, ip, dp, dp]
        L.spr_host_build.restype = C.c_int
        L.spr_host_build.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, lp, ip, C.c_int64, dp, dp, ip, dp]
        L.spr_host_patch_ratio.restype = C.c_double
        L.spr_host_patch_ratio.argtypes = [C.c_int, C.c_int, dp, ip, C.c_int, ip, C.c_int]
        L.spr_host_apply.restype = None
        L.spr_host_apply.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp, ip, lp, ip, dp, dp, dp, dp, dp, dp]

    def fit(self, points, xn):
        """(min |R_kk| / sqrt(m), g, h) of spr_fit on an explicit point set [m][dim]"""
        points = np.ascontiguousarray(points, dtype=np.float64)
        dim = points.shape[1]
        xn3 = np.zeros(3)
        xn3[:dim] = xn
        g, h = np.zeros(dim + 1), np.zeros(1)
        r = self.L.spr_host_fit(dim, len(points), points.ctypes.data_as(dp), xn3.ctypes.data_as(dp), g.ctypes.data_as(dp), h.ctypes.data_as(dp))
        return r, g, h[0]

    def points(self, name):
        et, coords, conn = mesh(name)
        pts = np.zeros((len(conn), shape_values(et).shape[0], dims(et)))
        self.L.spr_host_points(et, len(conn), conn.ctypes.data_as(ip), coords.ctypes.data_as(dp), pts.ctypes.data_as(dp))
        return pts

    def build(self, name):
        """spr_build_all of the header: tables with `ratio`, or raises HopeLost"""
        et, coords, conn = mesh(name)
        nn, T = len(coords), dims(et) + 1
        ptr = np.zeros(nn + 1, dtype=np.int64)
        args = (et, nn, len(conn), coords.ctypes.data_as(dp), conn.ctypes.data_as(ip), ptr.ctypes.data_as(lp))
        rc = self.L.spr_host_build(*args, None, 0, None, None, None, None)
        if rc >= 0:
            raise HopeLost(rc)
        elems = np.zeros(int(ptr[-1]), dtype=np.int32)
        g, h, st, ratio = np.zeros((nn, T)), np.zeros(nn), np.zeros(nn, dtype=np.int32), np.zeros(nn)
        rc = self.L.spr_host_build(*args, elems.ctypes.data_as(ip), len(elems), g.ctypes.data_as(dp), h.ctypes.data_as(dp),
                                   st.ctypes.data_as(ip), ratio.ctypes.data_as(dp))
        assert rc == -1, rc
        return {"patch_ptr": ptr, "patch_elems": elems, "g": g, "h": h, "stages": st, "ratio": ratio}

    def patch_ratio(self, name, node, elems):
        et, coords, conn = mesh(name)
        elems = np.ascontiguousarray(sorted(elems), dtype=np.int32)
        return self.L.spr_host_patch_ratio(et, len(conn), coords.ctypes.data_as(dp), conn.ctypes.data_as(ip), int(node),
                                           elems.ctypes.data_as(ip), len(elems))

    def apply(self, name, tab, field, weights=False):
        """spr_apply_host: (nodal [nnodes][ncomp], sum_s |w_s v_s| per entry[, w_s in table order])"""
        et, coords, conn = mesh(name)
        np0 = shape_values(et).shape[0]
        field = np.ascontiguousarray(field, dtype=np.float64).reshape(len(conn), np0, -1)
        ncomp = field.shape[2]
        nodal, mag = np.full((len(coords), ncomp), np.nan), np.full((len(coords), ncomp), np.nan)
        w = np.zeros(len(tab["patch_elems"]) * np0) if weights else None
        g, h = np.ascontiguousarray(tab["g"]), np.ascontiguousarray(tab["h"])
        self.L.spr_host_apply(et, len(coords), len(conn), ncomp, coords.ctypes.data_as(dp), conn.ctypes.data_as(ip),
                              tab["patch_ptr"].ctypes.data_as(lp), tab["patch_elems"].ctypes.data_as(ip), g.ctypes.data_as(dp),
                              h.ctypes.data_as(dp), field.ctypes.data_as(dp), nodal.ctypes.data_as(dp), mag.ctypes.data_as(dp),
                              None if w is None else w.ctypes.data_as(dp))
        return (nodal, mag, w) if weights else (nodal, mag)


def random_field(name, ncomp, seed=0):
    et, coords, conn = mesh(name)
    rng = np.random.default_rng(1000 * seed + ncomp)
    return rng.standard_normal((len(conn), shape_values(et).shape[0], ncomp))


def affine(et, x, ncomp=3, seed=5):
    """an affine field of the position, ncomp components: x [..., dims] -> [..., ncomp]"""
    rng = np.random.default_rng(seed)
    d = dims(et)
    return x[..., :d] @ rng.standard_normal((d, ncomp)) + rng.standard_normal(ncomp)


def write_mesh(path, name):
    """the text format of tests/spr_host/spr_host_main.cpp"""
    et, coords, conn = mesh(name)
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (et, len(coords), len(conn)))
        for row in coords:
            f.write("%.17g %.17g %.17g\n" % tuple(row))
        for row in conn:
            f.write(" ".join(str(int(v)) for v in row) + "\n")
