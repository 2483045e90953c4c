"""TEST INFRASTRUCTURE shared by test_cauchy_host.py and test_gpu_cauchy.py: the host harness of the product's per-point
stress evaluation (tests/cauchy_host/cauchy_host.cpp), the model rows with their oracle states, and the weak-form sums."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import oracle_lib as ol
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
# the flags of tests/emul/Makefile
CXXFLAGS = ["-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-unused-but-set-variable"]
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def build_harness(out_dir):
    """compile the harness into out_dir and return its entry point"""
    so = os.path.join(str(out_dir), "libcauchyhost.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-shared", "-o", so, os.path.join(HERE, "cauchy_host", "cauchy_host.cpp")])
    fn = C.CDLL(so).cauchy_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, dp, ip, dp, dp] + [dp] * 6 + [dp]
    return fn


def host_cauchy(fn, et, coords, conn, model, params, u, p, u_prev, p_prev, xi_prev, xi, elem_set=None, nn=None):
    """sigma [nelems][points][3][3] from the host harness"""
    d = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    coords, conn = d(coords), np.ascontiguousarray(conn, dtype=np.int32)
    params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, dtype=np.float64)))
    es = None if elem_set is None else np.ascontiguousarray(elem_set, dtype=np.int32)
    arrs = [d(a) for a in (nn, u, p, u_prev, p_prev, xi_prev, xi)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    npts = np.asarray(xi).shape[1]
    sigma = np.full((len(conn), npts, 3, 3), np.nan)
    got = fn(model.encode(), et, len(conn), conn.ctypes.data_as(ip), ptr(coords), None if es is None else es.ctypes.data_as(ip),
             ptr(params), *[ptr(a) for a in arrs], ptr(sigma))
    assert got == npts, (model, et, got, npts)
    return sigma


# ---- the model rows: (id, mesh kind, model, params, eps).  Every row of the model table on every element type it runs on;
# the parameter sets are those of parity_cases.py, at the strain at which the plastic models have yielded and elastic points
FINITE_DEF = {"hyper_J2", "hypo_hill", "hypo_hosford", "hypo_barlat", "hyper_J2_plane_strain", "hypo_hill_plane_strain",
              "hyper_J2_plane_stress", "hypo_hill_plane_stress", "hybrid_hyper_J2_plane_stress"}
NO_PLASTICITY = {"elastic", "isotropic_elastic"}
ALPHA = {"hypo_hill_plane_strain": 3, "hypo_hill_plane_stress": 3}  # position of alpha in xi where it is not the last unknown
HYBRID = "hybrid_hyper_J2_plane_stress"
HYBRID_NET = "tanh_16_16"


def _rows():
    rows = []
    for model, params, eps in pc.CASES[1:] + [c for c in pc.CASES_LINE_SEARCH if c[1] is not pc.HOSFORD_100]:
        rows += [("%s-%s" % (model, kind), kind, model, params, eps) for kind in ("hex8", "tet4")]
    for model, params, eps in pc.CASES_2D[1:] + pc.CASES_PLANE_STRESS[1:]:
        rows.append(("%s-tri3" % model, "tri3", model, params, eps))
    rows.append((HYBRID + "-tri3", "tri3", HYBRID, None, 0.004))
    return rows


ROWS = _rows()
ROW_IDS = [r[0] for r in ROWS]


def mesh(kind):
    return pc.mesh_2d("structured") if kind == "tri3" else pc.mesh_of(kind)


class Case:
    """one row on its mesh with the oracle's converged state of the second load step"""

    def __init__(self, kind, model, params, eps):
        self.kind, self.model, self.eps = kind, model, eps
        self.et, self.c, self.conn = mesh(kind)
        self.nn, self.embedded = None, None
        if model == HYBRID:
            import hybrid_cases as hc
            net = hc.NETS[HYBRID_NET]
            self.orc, _, _ = hc.hybrid_oracle((self.et, self.c, self.conn), net)
            self.params, self.nn, self.embedded = [hc.E, hc.NU, hc.Y], net.buffer(), net.embedded()
        else:
            self.orc = ol.Oracle(self.et, self.c, self.conn, model, params)
            self.params = params
            if model in ("small_hosford", "hypo_hosford", "hypo_barlat"):
                self.orc.set_local_line_search(*pc.LOCAL_LINE_SEARCH)
        st = pc.two_steps(self.orc, self.c, eps)
        (self.u, self.p, self.xi), (self.u_prev, self.p_prev, self.xi_prev) = st[2], st[1]
        self.plane_stress = self.orc.nres == 1
        self.finite = model in FINITE_DEF

    @property
    def state(self):
        return self.u, self.p, self.u_prev, self.p_prev, self.xi_prev, self.xi

    def host(self, fn):
        return host_cauchy(fn, self.et, self.c, self.conn, self.model, self.params, *self.state, nn=self.nn)

    def assembler_kw(self):
        kw = {}
        if self.model in ("small_hosford", "hypo_hosford", "hypo_barlat"):
            kw["line_search"] = pc.LOCAL_LINE_SEARCH
        if self.embedded is not None:
            kw["embedded"] = self.embedded
        return kw

    def branches(self):
        """(plastic points, elastic points) of the state"""
        a = self.xi[:, :, ALPHA.get(self.model, -1)]
        return int((a > 0).sum()), int((a == 0).sum())


@functools.lru_cache(maxsize=None)
def case(rid):
    _, kind, model, params, eps = ROWS[ROW_IDS.index(rid)]
    return Case(kind, model, params, eps)


def point_tables(et, coords, conn):
    """dN [nelems][points][nodes][3], N [nelems][points][nodes] and w dv [nelems][points] of ip set 0, from the oracle's kit"""
    pts, wts = ol.kit_points(et, 0)
    nn = conn.shape[1]
    dN, N, wdv = np.zeros((len(conn), len(pts), nn, 3)), np.zeros((len(conn), len(pts), nn)), np.zeros((len(conn), len(pts)))
    for e, nodes in enumerate(conn):
        for k in range(len(pts)):
            N[e, k], dN[e, k], dv = ol.shape(et, coords[nodes], pts[k])
            wdv[e, k] = wts[k] * dv
    return dN, N, wdv


def first_piola(sigma, grad_u, nd, finite, plane_stress, lambda_z=None, thickness=1.0):
    """P [..., nd, nd] of the weak form from sigma [..., 3, 3] and grad u [..., nd, nd]: sigma (small strain), sigma cof(I +
    grad u) (finite deformation under `mechanics`; in 2-D the in-plane block), t lambda_z J sigma F^-T (mechanics_plane_stress)"""
    s = sigma[..., :nd, :nd]
    if plane_stress:
        if not finite:
            return thickness * s
        F = np.eye(nd) + grad_u
        J = np.linalg.det(F)
        return thickness * (lambda_z * J)[..., None, None] * (s @ np.swapaxes(np.linalg.inv(F), -1, -2))
    if not finite:
        return s
    F = np.eye(nd) + grad_u
    cof = np.linalg.det(F)[..., None, None] * np.swapaxes(np.linalg.inv(F), -1, -2)
    return s @ cof


def weak_form(sigma, cs, nd, tables=None, lambda_z_index=4):
    """(R_u [nnodes][nd], scale): R_u[n, i] = sum_e sum_pt sum_j P_ij dN_n/dx_j w dv from the stress field `sigma` of the case
    `cs`, and the largest per-entry sum of the absolute values of those terms"""
    dN, _, wdv = tables if tables is not None else point_tables(cs.et, cs.c, cs.conn)
    dN = dN[..., :nd]
    ue = np.asarray(cs.u).reshape(-1, nd)[cs.conn]            # [e][n][i]
    grad_u = np.einsum("eni,epnj->epij", ue, dN)
    lam = cs.xi[:, :, lambda_z_index] if (cs.plane_stress and cs.finite) else None
    P = first_piola(sigma, grad_u, nd, cs.finite, cs.plane_stress, lam)
    terms = np.einsum("epij,epnj,ep->epnij", P, dN, wdv)     # one term per (element, point, node, i, j)
    R, A = np.zeros((len(cs.c), nd)), np.zeros((len(cs.c), nd))
    np.add.at(R, cs.conn, terms.sum(axis=(1, 4)))
    np.add.at(A, cs.conn, np.abs(terms).sum(axis=(1, 4)))
    return R, A.max()


def sub_mesh(coords, conn, n):
    """the first n elements with their nodes renumbered in the old order"""
    conn = np.asarray(conn)[:n]
    used = np.zeros(len(coords), dtype=bool)
    used[conn.ravel()] = True
    new_id = np.cumsum(used) - 1
    return np.ascontiguousarray(coords[used]), np.ascontiguousarray(new_id[conn].astype(np.int32))


def tet_mesh(nx, ny, nz):
    """a brick cut into six positively oriented tet4 per cell"""
    from meshes import brick
    c, hexes, _ = brick(nx, ny, nz, 1.0, 0.8, 0.7)
    tets = []
    for h in hexes:
        for a, b in ((1, 2), (2, 3), (3, 7), (7, 4), (4, 5), (5, 1)):  # the six tets around the diagonal 0-6
            t = [h[0], h[a], h[b], h[6]]
            if np.linalg.det(c[t[1:]] - c[t[0]]) < 0:
                t[1], t[2] = t[2], t[1]
            tets.append(t)
    return c, np.array(tets, dtype=np.int32)


def synthetic_state(xi0, coords, nd, nres, seed):
    """a smooth displacement step and the initial local state xi0 perturbed by 1e-2 (strain-like and stress-like unknowns
    then carry as much of the stress as the pressure does): inputs for comparing two evaluations of the same function (no
    oracle solve)"""
    rng = np.random.default_rng(seed)
    G = 0.01 * rng.standard_normal((nd, nd))
    u = (coords[:, :nd] @ G.T + 1e-3 * rng.standard_normal((len(coords), nd))).ravel()
    u_prev = 0.6 * u
    p = 0.01 * rng.standard_normal(len(coords))
    xi_prev = xi0
    xi = xi_prev + 1e-2 * rng.standard_normal(xi_prev.shape)
    return u, p, u_prev, 0.5 * p, xi_prev, xi
