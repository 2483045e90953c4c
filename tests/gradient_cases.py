"""TEST INFRASTRUCTURE: the cases of the per-parameter gradient tests and their difference reference.

One case per row of C8_MODEL_TABLE (c8_registry.hpp) and mesh: the total adjoint gradient dJ/dp (primal march, adjoint
march backwards, K3 -> K4 -> K5 summed over the steps) with respect to EVERY parameter of the row, on the smallest meshes
that still have nodes shared by one, two and four elements, through a load history with plastic loading, an elastic
unloading step and reloading.  `fd_gradient` is the reference that shares no algorithm with the adjoint: Richardson-
extrapolated central differences of the converged objective J(p), which uses the forward path only.

A case's gradient vector is indexed by SLOTS (element set, parameter index) in set order, the layout of K5
(c8_assemble_adjoint.hpp: lane k of set s writes slot act[s][0] + k); with one set the slots are the row's parameters in
their order, for the hybrid row E nu Y followed by every network weight.

test_oracle_gradient_fd.py   the oracle's adjoint gradient against fd_gradient, per parameter
test_emul_gradient.py        the kernel source (lane emulator) against the oracle's total gradient, per active group
test_gpu_gradient.py         the device drivers against the oracle's total gradient, per active group
"""
import os
import re

import numpy as np

import oracle_lib as ol
import parity_cases as pc
from fe_driver import Dbc, Primal, adjoint_gradient
from hybrid_cases import ABS_TOL as HYB_TOL
from hybrid_cases import HYB, NETS
from meshes import brick, tri_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# load factor of step t = 1, 2, ..: into plasticity, further, a partial (elastic) unloading, reloading beyond the maximum
LAM = (0.0, 1.0, 1.5, 1.15, 2.0)
NSTEPS = len(LAM) - 1
UNLOAD = 3                   # the step that is elastic at every point
SHEAR = 0.35                 # transverse (x) share of the displacement prescribed on ymax
RAMP = 0.8                   # the pull on ymax grows by this share of its mean from xmin to xmax: points yield one after another
NET = NETS["tanh_1"]         # the hybrid row's network: topology [1, 1, 1], four weights
ELASTIC = ("elastic", "isotropic_elastic")
PLANE_STRESS = ("small_hill_plane_stress", "hyper_J2_plane_stress", "hypo_hill_plane_stress", HYB)
HARDENING = {"hypo_hill_plane_strain": 3, "hypo_hill_plane_stress": 3}  # position of alpha in xi where it is not the last
LINE_SEARCH = ("small_hosford", "hypo_hosford", "hypo_barlat")


def model_table():
    """[(name, mesh dimension)] of C8_MODEL_TABLE, read from c8_registry.hpp: a row added there without a case here fails
    test_every_parameter_of_every_row_has_a_case"""
    src = open(os.path.join(ROOT, "calibr8_amd", "csrc", "c8_registry.hpp")).read()
    body = src[src.index("#define C8_MODEL_TABLE(X)"):src.index("// One row.")]
    return [(m.group(1), int(m.group(2))) for m in re.finditer(r'X\(MODEL_\w+,\s*"(\w+)",\s*(\d)\s*,', body)]


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def _perturb_in_planes(c, dims, amp, seed):
    """Every node of these meshes lies on the boundary (meshes.jiggle moves none): a node is moved along direction d only
    if it lies on neither bounding plane of d, so the node sets xmin .. zmax stay planar and keep their nodes."""
    rng = np.random.default_rng(seed)
    c = c.copy()
    for d in dims:
        lo, hi = c[:, d].min(), c[:, d].max()
        inner = (c[:, d] > lo + 1e-9) & (c[:, d] < hi - 1e-9)
        c[inner, d] += amp * (rng.random(int(inner.sum())) - 0.5)
    return c


# the two five-tetrahedron splits of a hex8 element (four corners cut off, one tetrahedron in the middle): alternated from
# cell to cell they conform across the shared faces, and a cut-off corner on the boundary is a node of one element only
_FIVE = (((0, 1, 3, 4), (2, 1, 6, 3), (5, 1, 4, 6), (7, 3, 6, 4), (1, 3, 4, 6)),
         ((1, 0, 5, 2), (3, 0, 2, 7), (4, 0, 7, 5), (6, 2, 5, 7), (0, 2, 5, 7)))


def tet_split(coords, hexes):
    """the cells of a brick that is one cell thick in y and z, in x order"""
    tets = []
    for i, h in enumerate(hexes):
        for t in _FIVE[i % 2]:
            n = [int(h[k]) for k in t]
            X = coords[n]
            if np.linalg.det(X[1:] - X[0]) < 0:
                n[1], n[2] = n[2], n[1]
            tets.append(n)
    return np.array(tets, dtype=np.int32)


def _node_sets(c, dims):
    names = "xyz"
    out = {}
    for d in dims:
        out[names[d] + "min"] = np.where(c[:, d] < c[:, d].min() + 1e-12)[0]
        out[names[d] + "max"] = np.where(c[:, d] > c[:, d].max() - 1e-12)[0]
    return out


_MESHES = {}


def mesh(kind):
    """(element type, coords, conn, node sets): a 2 x 2 x 1 hex8 bar (nodes of 1, 2 and 4 elements), the tet4 split of a
    2 x 1 x 1 brick (1, 2, 4 and 8), tri_mesh(2, 2) (2 and 8: its alternating diagonals leave no node to one triangle); the
    inner nodes are moved within their boundary planes, so no hex8 element is a parallelepiped"""
    if kind not in _MESHES:
        if kind == "hex8":
            c, conn, _ = brick(2, 2, 1, 1.0, 1.4, 0.6)
            et, c = ol.HEX8, _perturb_in_planes(c, (0, 1, 2), 0.16, 5)
        elif kind == "tet4":
            c, hexes, _ = brick(2, 1, 1, 1.2, 1.0, 0.7)
            c = _perturb_in_planes(c, (0, 1, 2), 0.2, 6)
            et, conn = ol.TET4, tet_split(c, hexes)
        else:
            c, conn, _ = tri_mesh(2, 2, 1.0, 1.3)
            et, c = ol.TRI3, _perturb_in_planes(c, (0, 1), 0.16, 8)
        sets = _node_sets(c, (0, 1, 2) if kind != "tri3" else (0, 1))
        _MESHES[kind] = (et, np.ascontiguousarray(c), np.ascontiguousarray(conn, dtype=np.int32), sets)
    return _MESHES[kind]


def elems_per_node(kind):
    et, c, conn, _ = mesh(kind)
    return np.bincount(conn.ravel(), minlength=len(c))


# ---- the cases ------------------------------------------------------------------------------------------------------------
class Case:
    """model on mesh `kind`, pulled in y with a transverse share through LAM at the rate `rate` (displacement of ymax at load
    factor 1).  params: one row per element set.  s: the relative difference step of fd_gradient.  zero: the slots whose
    adjoint component and difference are both exactly zero (named here, asserted in the tests).  yields: per step the share
    of points whose hardening variable must have grown, as (at least, at most)."""

    def __init__(self, model, kind, params, rate, s=1e-3, zero=(), objective="avg_disp", elem_set=None, slots=None,
                 yields=None, name=None, measured_scale=None, ramp=RAMP, mixed=True):
        self.model, self.kind, self.rate, self.s, self.zero, self.objective = model, kind, rate, s, tuple(zero), objective
        self.ramp, self.mixed = ramp, mixed
        self.hardening = HARDENING.get(model, -1)
        self.params = np.atleast_2d(np.asarray(params, dtype=np.float64))
        self.elem_set = None if elem_set is None else np.ascontiguousarray(elem_set, dtype=np.int32)
        self.slots = slots if slots is not None else [(0, k) for k in range(self.params.shape[1])]
        self.yields = yields
        self.measured_scale = measured_scale
        self.name = name or "%s-%s%s" % (model, kind, "" if objective == "avg_disp" else "-calibration")
        self.plane_stress = model in PLANE_STRESS
        self.width = 6 if self.plane_stress else 8   # lanes of K5 per element group

    def __repr__(self):
        return self.name

    @property
    def hybrid(self):
        return self.model == HYB

    # -- the parameter vector of the gradient: p[k] = params[slots[k]]
    def p0(self):
        return np.array([self.params[s, k] for s, k in self.slots])

    def rows(self, p):
        P = self.params.copy()
        for v, (s, k) in zip(p, self.slots):
            P[s, k] = v
        return P

    # -- problem definition shared by every backend
    def dbc_spec(self):
        """[(resid, eq, nodes, fn(x, y, z, t))]: symmetry planes, ymax pulled in y and sheared in x"""
        et, c, conn, sets = mesh(self.kind)
        zero = lambda x, y, z, t: 0.0
        rate, ramp, lx = self.rate, self.ramp, float(c[:, 0].max())
        lam = lambda t: float(np.interp(t, np.arange(len(LAM)), LAM))
        spec = [(0, 0, sets["xmin"], zero), (0, 1, sets["ymin"], zero),
                (0, 1, sets["ymax"], lambda x, y, z, t: rate * lam(t) * (1.0 + ramp * (x / lx - 0.5))),
                (0, 0, sets["ymax"], lambda x, y, z, t: SHEAR * rate * lam(t))]
        if self.kind != "tri3":
            spec.append((0, 2, sets["zmin"], zero))
        return spec

    def backend_kw(self, P):
        """(positional, keyword) arguments common to ol.Oracle, emul_lib.Emul and calibr8_amd.Assembler for the rows P"""
        et, c, conn, _ = mesh(self.kind)
        kw = {}
        if self.elem_set is not None:
            kw["elem_set"] = self.elem_set
        if self.hybrid:
            kw.update(abs_tol=HYB_TOL, rel_tol=HYB_TOL)
        return (et, c, conn, self.model, P[:, :3] if self.hybrid else P), kw

    def embedded(self, P):
        """the hybrid row's network with the weights of P (slots 3 ..)"""
        d = NET.embedded()
        d["params"] = np.ascontiguousarray(P[0, 3:])
        return d

    def calibration_kw(self):
        """the set-up of test_oracle_checks.calibration_bar / test_gpu_parity._calibration_pair: displacement mismatch on the
        xmax side (3-D: its faces; 2-D: the elements with a node on it), reaction load on the plane y = ymin, non-unit weights"""
        et, c, conn, sets = mesh(self.kind)
        xmax = set(sets["xmax"].tolist())
        if self.kind == "hex8":
            loc = ([0, 1, 2, 3], [0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [3, 0, 4, 7], [4, 5, 6, 7])
        elif self.kind == "tet4":
            loc = ([0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3])
        if self.kind == "tri3":
            faces = [e for e in range(len(conn)) if any(int(n) in xmax for n in conn[e])]
        else:
            faces = [[int(e[k]) for k in f] for e in conn for f in loc if all(int(e[k]) in xmax for k in f)]
        return faces, dict(weights=(1.0, 2.0, 0.5), balance=3e-4, coord_idx=1, coord_value=float(c[:, 1].min()), coord_tol=1e-8,
                           comp=1, dt_over_T=1.0 / NSTEPS)

    # -- the oracle
    def oracle(self, P):
        (args, kw) = self.backend_kw(P)
        if self.hybrid:
            kw["embedded"] = self.embedded(P)
        orc = ol.Oracle(*args, **kw)
        if self.model in LINE_SEARCH:
            orc.set_local_line_search(*pc.LOCAL_LINE_SEARCH)
        return orc

    def primal(self, be, measured=None):
        """fe_driver.Primal over the backend `be`, solved through the NSTEPS load steps"""
        et, c, conn, _ = mesh(self.kind)
        if self.objective == "calibration":
            faces, kw = self.calibration_kw()
            be.set_calibration(faces, **kw)
        pr = Primal(be, c, [Dbc(*s) for s in self.dbc_spec()], max_iters=30, abs_tol=1e-12, rel_tol=1e-12).solve(NSTEPS)
        if self.objective == "calibration":
            pr.measured = measured if measured is not None else self.measurements()
        return pr

    def measurements(self):
        """calibration: displacements and reaction loads of a solve at other parameters ([None, u_1 ..], [0, load_1 ..])"""
        if getattr(self, "_meas", None) is None:
            P = self.params * self.measured_scale
            orc = self.oracle(P)
            faces, kw = self.calibration_kw()
            orc.set_calibration(faces, **kw)
            et, c, conn, _ = mesh(self.kind)
            pt = Primal(orc, c, [Dbc(*s) for s in self.dbc_spec()], max_iters=30, abs_tol=1e-12, rel_tol=1e-12).solve(NSTEPS)
            loads = [0.0]
            for n in range(1, NSTEPS + 1):
                orc.set_measured(np.zeros_like(pt.u[n]), 0.0)
                loads.append(float(orc.qoi_preprocess(pt.u[n], pt.p[n], pt.u[n - 1], pt.p[n - 1], pt.xi[n - 1], pt.xi[n])[1]))
            self._meas = ([None] + [u.copy() for u in pt.u[1:]], loads)
        return self._meas

    def solve(self, p):
        """p (slot vector) -> solved fe_driver.Primal over the oracle: the `solve` of fd_gradient"""
        return self.primal(self.oracle(self.rows(p)))

    def groups_all(self):
        """all slots active at once, per element set (the oracle has no lane limit below 32)"""
        out = {}
        for s, k in self.slots:
            out.setdefault(s, []).append(k)
        return out

    def oracle_gradient(self, pr=None):
        """(J, dJ/dp per slot, the solved Primal) of the oracle with every slot active"""
        pr = pr if pr is not None else self.solve(self.p0())
        if self.hybrid:  # more than 32 weights would need chunks (hybrid_cases.oracle_theta_gradient); NET has four
            assert len(self.slots) <= 32
        for s, idx in self.groups_all().items():
            pr.be.set_active(s, idx)
        return pr.qoi(), adjoint_gradient(pr, len(self.slots)), pr


def active_groups(case):
    """[{set: [parameter indices]}]: the active lists of the emulator and device tests.  Across the groups every slot
    appears; one group is in descending order, one has the full lane width (8, or 6 under mechanics_plane_stress; the
    whole row where it has fewer parameters), one is a single parameter.  With two element sets the lists are the
    case's own (8 permuted entries and 1 entry)."""
    if case.elem_set is not None:
        return [case.groups_all()]
    n, w = case.params.shape[1], case.width
    if case.hybrid:
        n = 3  # E nu Y go through the lanes; the weights are appended by the weight-gradient kernel, whatever is active
    groups = [list(range(min(n, w) - 1, -1, -1))]          # descending, full width (or the whole row)
    rest = list(range(min(n, w), n))
    while len(rest) > 1:                                   # ascending groups, the last slot kept for the single-lane group
        take = min(w, len(rest) - 1)
        groups.append(rest[:take])
        rest = rest[take:]
    groups.append(rest if rest else [n // 2])              # a single parameter
    return [{0: g} for g in groups]


def slot_index(case, group):
    """positions in the case's gradient vector of a group's lanes, in lane order"""
    where = {sk: i for i, sk in enumerate(case.slots)}
    return [where[(s, k)] for s in sorted(group) for k in group[s]]


_REFERENCE = {}


def oracle_reference(case):
    """(J, dJ/dp per slot, the solved Primal) of the oracle with every slot active: computed once per case and shared,
    unchanged, by the tests that compare with it"""
    if case.name not in _REFERENCE:
        J, g, pr = case.oracle_gradient()
        g.setflags(write=False)
        _REFERENCE[case.name] = (J, g, pr)
    return _REFERENCE[case.name]


TOTAL_BAR = 1e-8  # emulator and device against the oracle's total gradient, of the largest scaled component


def check_groups_against_oracle(case, march, n_tail=0):
    """march(group) -> the gradient of one adjoint march with the active lists `group` ({set: [indices]}), lanes in slot
    order, then n_tail appended entries (the hybrid row's weights, slots 3 ..).  Every component must equal the component
    of the all-active oracle gradient at TOTAL_BAR of the largest scaled component: a component does not depend on its
    lane, on the other lanes or on the order of the list.  Returns the worst ratio."""
    J, g, _ = oracle_reference(case)
    sp = spans(case.p0())
    scale = np.abs(g * sp).max()
    assert scale > 0.0
    groups = active_groups(case)
    n_head = len(case.slots) - n_tail
    seen, worst = set(), 0.0
    width = max(sum(len(v) for v in grp.values()) for grp in groups)
    assert width == min(case.width, n_head) or case.elem_set is not None
    assert any(len(v) == 1 for grp in groups for v in grp.values())
    assert any(list(v) == sorted(v, reverse=True) and len(v) > 1 for grp in groups for v in grp.values()) or case.elem_set is not None
    bad = []  # every group is marched before the check fails: the report names all components that miss
    for grp in groups:
        idx = slot_index(case, grp) + list(range(n_head, n_head + n_tail))
        got = np.asarray(march(grp))
        assert got.shape == (len(idx),), (case.name, grp, got.shape)
        err = np.abs(got - g[idx]) * sp[idx] / scale
        worst = max(worst, float(err.max()))
        for lane, i in enumerate(idx):
            if not err[lane] <= TOTAL_BAR or (i in case.zero and got[lane] != 0.0):
                bad.append((grp, lane, case.slots[i], got[lane], g[i], err[lane]))
        seen.update(idx)
    assert seen == set(range(len(case.slots))), (case.name, "slots never active", set(range(len(case.slots))) - seen)
    assert not bad, (case.name, "components off the oracle's total gradient (group, lane, (set, parameter), got, oracle, ratio)", bad)
    return worst


def _two_sets():
    """small_hill on the hex8 bar, two element sets with different parameters: set 0 with 8 active parameters in a
    permuted order, set 1 with a single one; gradient length 9, slots in set order"""
    hill2 = [900.0, 0.3, 1.7, 1.05, 0.95, 1.1, 0.9, 1.0, 1.08, 2.0, 30.0]
    slots = [(0, k) for k in (9, 0, 3, 10, 6, 2, 8, 5)] + [(1, 2)]
    return Case("small_hill", "hex8", [pc.HILL, hill2], RATE["two_sets"], elem_set=[0, 1, 1, 0], slots=slots,
                yields=YIELDS, name="small_hill-hex8-two_sets")


# mean strain of the bar in y at load factor 1: the displacement of ymax is this times the bar's length (initial uniaxial
# yield strains: 0.002 with E = 1000 and Y = 2, Barlat 0.0029 with E = 70e3 and Y = 200)
STRAIN = {"elastic": 0.003, "isotropic_elastic": 0.003, "small_J2": 0.0021, "hyper_J2": 0.0021, "small_hill": 0.0021,
          "hypo_hill": 0.0021, "small_hosford": 0.0021, "hypo_hosford": 0.0021, "hypo_barlat": 0.0055,
          "small_hill_plane_strain": 0.0021, "hyper_J2_plane_strain": 0.0021, "hypo_hill_plane_strain": 0.0021,
          "small_hill_plane_stress": 0.0021, "hyper_J2_plane_stress": 0.0021, "hypo_hill_plane_stress": 0.0021, HYB: 0.0021}
LENGTH = {"hex8": 1.4, "tet4": 1.0, "tri3": 1.3}
RATE = {(m, k): e * LENGTH[k] for m, e in STRAIN.items() for k in LENGTH}
# moved away from a kink of J: at 0.0021 a point of these cases crosses its yield surface inside the difference stencil of
# E and Y (the yielded masks of the perturbed solves differ from the base solve's, or the two extrapolants disagree)
for _m in ("small_hosford", "hypo_hosford"):
    RATE[_m, "hex8"] = 0.0022 * LENGTH["hex8"]
RATE["two_sets"] = 0.0022 * LENGTH["hex8"]
# hypo_barlat: a uniform pull that takes every point plastic in the first step.  With the ramp, points of this row yield
# one after another within the stencil of a difference and J has a kink there, which the conditions on the reference refuse
BARLAT_LOAD = dict(ramp=0.0, mixed=False, yields={1: (1.0, 1.0), 2: (1.0, 1.0), UNLOAD: (0.0, 0.0), 4: (1.0, 1.0)})
PARAMS = {"elastic": pc.EL, "isotropic_elastic": [1000.0, 0.25], "small_J2": pc.J2, "hyper_J2": pc.HJ2, "small_hill": pc.HILL,
          "hypo_hill": pc.HILL, "small_hosford": pc.HOSFORD, "hypo_hosford": pc.HOSFORD, "hypo_barlat": pc.BARLAT,
          "small_hill_plane_strain": pc.HILL_PS, "hyper_J2_plane_strain": pc.HJ2_PS, "hypo_hill_plane_strain": pc.HILL_PS,
          "small_hill_plane_stress": pc.HILL_PS, "hyper_J2_plane_stress": pc.HJ2_PSS, "hypo_hill_plane_stress": pc.HYPO_PSS,
          HYB: [1000.0, 0.25, 2.0] + list(NET.theta)}
# share of points whose hardening variable grows, per step, as (at least, at most): step 1 has elastic and plastic points
# side by side, the unloading step none, the last step all
YIELDS = {1: (0.1, 0.9), 2: (0.5, 1.0), UNLOAD: (0.0, 0.0), 4: (0.6, 1.0)}
# parameters whose adjoint component and difference are both exactly zero (slot indices): small_J2's cte and delta_T,
# which the model carries and never reads, and hypo_hosford's K (its flow stress has no K term)
ZERO = {"small_J2": (4, 5), "hypo_hosford": (4,)}
# the relative step of fd_gradient where it is not 1e-3: at 1e-3 the cruder extrapolant of small_hill_plane_strain's
# parameters is 7e-9 off the finer one (the h^4 term), more than a tenth of the bar
STEP = {"small_hill_plane_strain": 5e-4}


def _cases():
    out = []
    for model, dim in model_table():
        for kind in (("hex8", "tet4") if dim == 3 else ("tri3",)):
            kw = dict(yields=None if model in ELASTIC else YIELDS)
            if model == "hypo_barlat":
                kw = BARLAT_LOAD
            out.append(Case(model, kind, PARAMS[model], RATE[model, kind], s=STEP.get(model, 1e-3), zero=ZERO.get(model, ()), **kw))
    scale = {"small_hill": [1.1, 1.0, 0.8, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.9, 1.2],
             "hyper_J2": [1.1, 1.0, 0.8, 1.2, 0.9, 1.0, 1.0, 1.0],
             "small_hill_plane_stress": [1.1, 1.0, 0.8, 0.9, 1.2, 1.0, 1.0, 1.0, 1.0]}
    for model, kind in (("small_hill", "hex8"), ("hyper_J2", "tet4"), ("small_hill_plane_stress", "tri3")):
        out.append(Case(model, kind, PARAMS[model], RATE[model, kind], objective="calibration", yields=YIELDS,
                        measured_scale=np.array(scale[model])))
    out.append(_two_sets())
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---- what the load history is there for -----------------------------------------------------------------------------------
def yielded_masks(pr, k=-1):
    """per step 1 .. the mask [nelems, npts] of points whose hardening variable xi[k] grew"""
    return [np.asarray(pr.xi[n])[:, :, k] > np.asarray(pr.xi[n - 1])[:, :, k] for n in range(1, len(pr.xi))]


def check_history(case, pr):
    """the branches the history is there for really ran (asserted from the stored xi)"""
    if case.yields is None:
        return
    masks, k = yielded_masks(pr, case.hardening), case.hardening
    assert len(masks) == NSTEPS and not np.asarray(pr.xi[0])[:, :, k].any()
    for n, m in enumerate(masks, start=1):
        lo, hi = case.yields[n]
        assert lo <= m.mean() <= hi, (case.name, n, float(m.mean()), (lo, hi))
    # the unloading step leaves the whole local state of a small-strain row, and the hardening variable of every row, as it was
    assert np.array_equal(pr.xi[UNLOAD][:, :, k], pr.xi[UNLOAD - 1][:, :, k]), case.name
    assert any(0 < m.sum() < m.size for m in masks) == case.mixed, (case.name, "a step with elastic and plastic points side by side")


# ---- the difference reference -----------------------------------------------------------------------------------------------
def fd_gradient(solve, p, k, span, s=1e-3, hardening=-1):
    """dJ/dp_k by central differences of the converged objective: D(s), D(s/2), D(s/4) at the steps s span, s span / 2,
    s span / 4 (span = |p_k|, or 1 where p_k = 0).  Returns (R, R2, masks): the Richardson value R = (4 D(s/4) - D(s/2)) / 3,
    the second extrapolant R2 = (4 D(s/2) - D(s)) / 3, and for each of the six solves the per-step masks of points whose
    hardening variable grew (yielded_masks).  D has the error c2 h^2 + c4 h^4: R and R2 differ by (15/16) c4 (s span)^4, five
    times the error of R -- unless J has a kink inside the stencil, which shows as a c1 h term that R and R2 do not cancel."""
    p = np.asarray(p, dtype=np.float64)
    D, masks = [], []
    for h in (s * span, 0.5 * s * span, 0.25 * s * span):
        J = []
        for sign in (1.0, -1.0):
            q = p.copy()
            q[k] += sign * h
            pr = solve(q)
            J.append(pr.qoi())
            masks.append(yielded_masks(pr, hardening))
        D.append((J[0] - J[1]) / (2.0 * h))
    return (4.0 * D[2] - D[1]) / 3.0, (4.0 * D[1] - D[0]) / 3.0, masks


def spans(p):
    p = np.asarray(p, dtype=np.float64)
    return np.where(p != 0.0, np.abs(p), 1.0)
