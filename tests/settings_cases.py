"""TEST INFRASTRUCTURE shared by test_emul_settings.py (the kernel bodies on the CPU) and test_gpu_settings.py (the device):
the numbers of ModelSettings (c8_assemble.hpp) away from their defaults -- stabilization multiplier, local Newton tolerances
and budget, the four numbers of the local line search -- as tables of settings, helpers that build an oracle and a backend
with the same settings, and the construction of a local solve that fails in exactly one element (two element sets).

A `settings` dict holds keyword arguments that oracle_lib.Oracle, emul_lib.Emul and calibr8_amd.Assembler share: stab_mult,
max_iters, abs_tol, rel_tol, and line_search = (c1, min factor, max factor, max evaluations).  Meshes are those of
launch_cases.py at one count per row of launch_cases.UNITS: unit + 1, the smallest with a ragged tail."""
import collections
import functools

import numpy as np

import cauchy_cases as cc
import gradient_cases as gc
import launch_cases as lc
import oracle_lib as ol
import parity_cases as pc
from meshes import fields_for, prescribed_fields

TOL = lc.TOL
LINE_SEARCH_MODELS = ("small_hosford", "hypo_hosford", "hypo_barlat")


# ---- an oracle and a backend with the same settings ----------------------------------------------------------------------
def oracle(et, c, conn, model, params, line_search=None, elem_set=None, **settings):
    orc = ol.Oracle(et, c, conn, model, params, elem_set=elem_set, **settings)
    if line_search is None and model in LINE_SEARCH_MODELS:
        line_search = pc.LOCAL_LINE_SEARCH
    if line_search is not None:
        orc.set_local_line_search(*line_search)
    return orc


def emulator(config, et, c, conn, model, params, line_search=None, elem_set=None, **settings):
    """the lane emulator with the switches `config` = (wave, closed, staged, node) of test_emul_launch_edges.emul_config"""
    import emul_lib as em
    dut = em.Emul(et, c, conn, model, params, elem_set=elem_set, **settings)
    dut.wave, dut.closed, dut.staged, dut.node = config
    if line_search is None and model in LINE_SEARCH_MODELS:
        line_search = pc.LOCAL_LINE_SEARCH
    if line_search is not None:
        dut.set_local_line_search(*line_search)
    return dut


def case_id(cs):
    return "%s-%s-%s-%s-%d%s" % (cs.kind, cs.form, cs.scatter, cs.model, cs.n, "c" if cs.cut else "")


def sid(settings):
    """a settings dict as part of a test id"""
    return ",".join("%s=%s" % (k[:4], "/".join("%g" % x for x in v) if isinstance(v, tuple) else "%g" % v) for k, v in sorted(settings.items()))


# ---- the rows ----------------------------------------------------------------------------------------------------------
def count_of(kind, form):
    """unit + 1 of the row of launch_cases.UNITS that the form's kernels have: hex8 lane groups 3, hex8 wave / node kernels 9
    (the groups of eight of K2, K4, K5), tet4 5, tri3 8, plane-stress tri3 11"""
    if kind == "hex8" and form != "slot":
        return lc.row("wave8", "hex8").unit + 1
    return lc.row("group", kind).unit + 1


def chain_rows():
    """every (kind, form, scatter, model) that launch_cases.chain_cases enumerates, once, at count_of (hex8: the cut brick)"""
    out, seen = [], set()
    for cs in lc.chain_cases():
        key = (cs.kind, cs.form, cs.scatter, cs.model)
        if key not in seen:
            seen.add(key)
            out.append(lc.Case("settings", cs.kind, cs.form, cs.scatter, cs.model, cs.params, cs.eps, count_of(cs.kind, cs.form), cs.kind == "hex8"))
    return out


def hosford_rows(params=pc.HOSFORD):
    """small_hosford on the hex8 wave kernels and the tet4 lane groups, at count_of"""
    return [lc.Case("settings", kind, form, "atomic", lc.HOSFORD[0], tuple(params), lc.HOSFORD[2], count_of(kind, form), False)
            for kind, form in (("hex8", "wave"), ("tet4", "auto"))]


def tolerance_rows():
    """the rows of the tolerance and budget runs: every form of small_J2 on hex8 (the row-per-node form both as `node` and as
    the library's own choice under `gather`), one automatically differentiated model on the hex8 wave kernels, and both
    models of every other element type"""
    want = [("hex8", "node", "gather", "small_J2"), ("hex8", "auto", "gather", "small_J2"), ("hex8", "wave", "atomic", "small_J2"),
            ("hex8", "wave_ad", "atomic", "small_J2"), ("hex8", "slot", "atomic", "small_J2"), ("hex8", "wave", "atomic", "hyper_J2"),
            ("tet4", "auto", "atomic", "small_J2"), ("tet4", "auto", "atomic", "hyper_J2"), ("tri3", "auto", "atomic", "small_J2"),
            ("tri3", "auto", "atomic", "hyper_J2_plane_strain"), ("tri3ps", "auto", "atomic", "hyper_J2_plane_stress")]
    rows = {(cs.kind, cs.form, cs.scatter, cs.model): cs for cs in chain_rows()}
    return [rows[k] for k in want]


STAB = (0.37, 3.7)  # neither 1 nor a power of two: no scaling by them is exact
TOLERANCES = ({"abs_tol": 1e-6, "rel_tol": 1e-6},
              {"abs_tol": 1e-14, "rel_tol": 1e-3})  # only the relative test can stop an iteration that began at a non-zero residual
BUDGETS = (7, 8)           # c8_api.hip: the closed form of a model runs from local_max_iters = 8 on, below it the iterated form
BAND_TOL = 1e-3            # abs_tol as the width of the yield band (c8_models.hpp: f > tol || |f| < tol)


def mesh_of(cs):
    return lc.mesh(cs.kind, cs.n, cs.cut)


def oracle_of(cs, **settings):
    et, c, conn = mesh_of(cs)
    return oracle(et, c, conn, cs.model, list(cs.params), **settings), c, conn


def mixed(cs):
    """two residuals (displacement and pressure): the rows that have a stabilisation term"""
    return cs.kind != "tri3ps"


# ---- 1(b): what the multiplier moves --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _systems_by_stab(cs):
    """the oracle's (xi, system) of the second step of the table's history for stab_mult = 1 and every value of STAB, at the
    state of the oracle with stab_mult = 1 (the state does not depend on the multiplier)"""
    base, c, _ = oracle_of(cs)
    st = pc.two_steps(base, c, cs.eps)
    (u, p, _), (up, pp, xip) = st[2], st[1]
    out = {}
    for s in (1.0,) + STAB:
        orc, _, _ = oracle_of(cs, stab_mult=s)
        ls, xi = orc.new_linsys(), orc.new_state()
        assert orc.forward_jacobian(u, p, up, pp, xip, xi, ls) == 0
        out[s] = (xi, ls)
    return out


def stab_power(cs, s):
    """{block: max |block(s) - block(1)| / max |block(1)|} of the oracle's Jacobian and residual"""
    sy = _systems_by_stab(cs)
    (_, l1), (_, ls) = sy[1.0], sy[s]
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0
    out = {"A%d%d" % (i, j): rel(ls.A[i][j], l1.A[i][j]) for i in range(2) for j in range(2)}
    out.update({"b%d" % i: rel(ls.b[i], l1.b[i]) for i in range(2)})
    return out


def assert_stab_power(cs, s):
    """the conditions under which a chain at stab_mult = s can tell a kernel that ignores the setting: the oracle's A11 moves
    by at least 0.1 of its largest entry (measured: at least 0.60), and A10 of a finite-deformation model by more than 1e-4
    (measured: at least 0.004) -- eleven and eight orders of magnitude above the bar of the chain"""
    pw = stab_power(cs, s)
    assert pw["A11"] >= 0.1, (case_id(cs), s, pw)
    if cs.model in cc.FINITE_DEF:
        assert pw["A10"] > 1e-4, (case_id(cs), s, pw)
    assert pw["A00"] == 0.0 and pw["A01"] == 0.0 and pw["b0"] == 0.0, (case_id(cs), s, pw)


GRADIENT_ROWS = ("small_J2-hex8", "hyper_J2-tet4")  # of gradient_cases.CASES


class StabCase(gc.Case):
    """a row of gradient_cases.py with the stabilization multiplier STAB[1] on every backend"""

    def __init__(self, base):
        gc.Case.__init__(self, base.model, base.kind, base.params, base.rate, s=base.s, zero=base.zero, yields=base.yields,
                         name="%s-stab%g" % (base.name, STAB[1]))

    def backend_kw(self, P):
        args, kw = gc.Case.backend_kw(self, P)
        kw["stab_mult"] = STAB[1]
        return args, kw


STAB_GRADIENT_CASES = {rid: StabCase(gc.BY_NAME[rid]) for rid in GRADIENT_ROWS}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def forward_at_step_two(cs, dut, base=None):
    """(xi, system) of K1 on `dut` at the second step of the table's history (solved by an oracle with default settings)"""
    if base is None:
        base = oracle_of(cs)[0]
    st = pc.two_steps(base, mesh_of(cs)[1], cs.eps)
    (u, p, _), (up, pp, xip) = st[2], st[1]
    ls, xi = dut.new_linsys(), dut.new_state()
    assert dut.forward_jacobian(u, p, up, pp, xip, xi, ls) == 0
    return xi, ls


def systems_same_bits(a, b, nres=2):
    (xa, la), (xb, lb) = a, b
    ok = same_bits(xa, xb)
    for i in range(nres):
        ok = ok and same_bits(la.b[i], lb.b[i])
        for j in range(nres):
            ok = ok and same_bits(la.A[i][j], lb.A[i][j])
    return ok


# ---- 2: the yield band ------------------------------------------------------------------------------------------------------
def trial_yield_values(et, c, conn, params, u, xi_prev):
    """small_J2 in 3-D: f0 = (|s_tr| - sqrt(2/3)(Y + K alpha_prev)) / mu at every local-state point, s_tr = 2 mu (dev eps(u) -
    pstrain_prev), from the oracle's shape-function kit (c8_models.hpp: SmallJ2::evaluate at the initial guess xi = xi_prev)"""
    E, nu, K, Y = params[:4]
    mu = E / (2.0 * (1.0 + nu))
    dN, _, _ = cc.point_tables(et, c, conn)
    ue = np.asarray(u).reshape(-1, 3)[conn]
    g = np.einsum("eni,epnj->epij", ue, dN)
    eps = 0.5 * (g + np.swapaxes(g, -1, -2))
    dev = eps - np.trace(eps, axis1=-2, axis2=-1)[..., None, None] / 3.0 * np.eye(3)
    x = xi_prev
    pl = np.stack([np.stack([x[..., 0], x[..., 1], x[..., 2]], -1), np.stack([x[..., 1], x[..., 3], x[..., 4]], -1),
                   np.stack([x[..., 2], x[..., 4], x[..., 5]], -1)], -2)
    s = 2.0 * mu * (dev - pl)
    return (np.sqrt((s * s).sum(axis=(-1, -2))) - np.sqrt(2.0 / 3.0) * (Y + K * x[..., 6])) / mu


BAND_EPS = (0.004, 0.005, 0.006, 0.003, 0.007, 0.008)  # the step is scaled through these until the band holds points on both sides


@functools.lru_cache(maxsize=None)
def band_case(kind, n, cut):
    """(eps, oracle with abs_tol = BAND_TOL, c, conn, counts): the first eps of BAND_EPS at which, over the two steps of the
    history that the chain runs, at least one point has a trial yield value in (0, BAND_TOL) and one in (-BAND_TOL, 0).  The
    values are computed from the oracle's kit and states and confirmed by the oracle itself: a point with 0 < f0 < BAND_TOL
    keeps its previous state bit for bit (the iteration stops at its first test), although an oracle with the default
    tolerance moves it."""
    et, c, conn = lc.mesh(kind, n, cut)
    for eps in BAND_EPS:
        orc = oracle(et, c, conn, "small_J2", list(pc.J2), abs_tol=BAND_TOL)
        sharp = oracle(et, c, conn, "small_J2", list(pc.J2))
        st = pc.two_steps(orc, c, eps)
        above = below = 0
        for k in (1, 2):
            (u, p, xi), (up, pp, xip) = st[k], st[k - 1]
            f = trial_yield_values(et, c, conn, pc.J2, u, xip)
            inside_above, inside_below = (f > 0) & (f < BAND_TOL), (f < 0) & (f > -BAND_TOL)
            xs = sharp.new_state()
            assert sharp.forward_jacobian(u, p, up, pp, xip, xs, sharp.new_linsys()) == 0
            kept = (xi == xip).all(axis=-1)
            moved_sharp = xs[:, :, 6] > xip[:, :, 6]
            # the oracle's own verdict on every point: kept in the band and below the surface, moved above the band
            assert np.array_equal(kept, f < BAND_TOL), (eps, k)
            assert np.array_equal(moved_sharp, f > 1e-12), (eps, k)
            above += int(inside_above.sum())
            below += int(inside_below.sum())
        if above > 0 and below > 0 and (st[2][2][:, :, 6] > 0).any():
            return eps, orc, c, conn, (above, below)
    raise AssertionError("no step of BAND_EPS puts points on both sides of the yield surface inside the band", kind, n)


BAND_ROWS = [lc.Case("band", "hex8", form, scatter, "small_J2", tuple(pc.J2), 0.0, 9, True)
             for form, scatter in (("wave", "atomic"), ("wave_ad", "atomic"), ("node", "gather"), ("slot", "atomic"))] + \
            [lc.Case("band", "tet4", form, "atomic", "small_J2", tuple(pc.J2), 0.0, 5, False) for form in ("auto", "slot")]


# ---- 3: a local solve that fails in one element ------------------------------------------------------------------------------
YIELD_STRESS = {"small_J2": 3, "hyper_J2": 2, "hyper_J2_plane_strain": 3, "hyper_J2_plane_stress": 2, "small_hosford": 2}  # index of Y
ELASTIC_Y = 1e6
FAIL_EPS = (0.004, 0.008, 0.016, 0.032, 0.064)  # raised until the target yields: the high-numbered triangles lie at the low end of the ramp
Failure = collections.namedtuple("Failure", "et c conn model params elem_set control_set step b eps")


def two_set_params(model, params, y1=None):
    """[set 0: the parameters with the yield stress raised to ELASTIC_Y, set 1: the parameters (yield stress y1 if given)]"""
    k = YIELD_STRESS[model]
    p0, p1 = list(params), list(params)
    p0[k] = ELASTIC_Y
    if y1 is not None:
        p1[k] = y1
    return [p0, p1]


def _grown(st):
    """[nelems, npts]: the points whose alpha (the last local unknown of every model here) grows in the second step"""
    return st[2][2][:, :, -1] > st[1][2][:, :, -1]


def yielding_elements(kind, model, params, n, eps):
    """the elements of lc.mesh(kind, n) with a point whose alpha grows in the second step, every element with `params`"""
    et, c, conn = lc.mesh(kind, n, kind == "hex8")
    orc = oracle(et, c, conn, model, list(params))
    return np.flatnonzero(_grown(pc.two_steps(orc, c, eps)).any(axis=1))


def targets_of(kind, form, n, first):
    """the elements where the lane arithmetic could lose the flag: the first yielding one, the last element of the last full
    unit, the single element of the ragged last unit"""
    unit = 8 if (kind == "hex8" and form != "slot") else lc.row("group", kind).unit
    assert n % unit == 1
    return sorted({int(first), n - 2, n - 1})


@functools.lru_cache(maxsize=None)
def failure(kind, model, params, n, targets, y1=None, want_points=None):
    """the state and sets in which the local solve fails in exactly the elements `targets`, with every condition the tests
    rely on asserted on the oracle: the step-2 state of the history at the first eps of FAIL_EPS at which exactly the targets
    have points whose alpha grows (want_points: exactly that many points), the smallest budget b at which the oracle returns
    0 (2 <= b <= 12), -1 at b - 1, and 0 at b - 1 in the control with no element in set 1"""
    et, c, conn = lc.mesh(kind, n, kind == "hex8")
    prm = two_set_params(model, params, y1)
    es = np.zeros(n, dtype=np.int32)
    es[list(targets)] = 1
    control = np.zeros(n, dtype=np.int32)
    seen = []
    for eps in FAIL_EPS:
        st = pc.two_steps(oracle(et, c, conn, model, prm, elem_set=es), c, eps)
        grown = _grown(st)
        seen.append((eps, np.flatnonzero(grown.any(axis=1)).tolist(), int(grown.sum())))
        if seen[-1][1] == sorted(targets) and (want_points is None or seen[-1][2] == want_points):
            break
    else:
        raise AssertionError("the targets do not yield alone", kind, model, n, targets, seen)
    (u, p, _), (up, pp, xip) = st[2], st[1]
    step = (u, p, up, pp, xip)

    def code(budget, elem_set):
        o = oracle(et, c, conn, model, prm, elem_set=elem_set, max_iters=budget)
        return o.forward_jacobian(*step, o.new_state(), o.new_linsys())

    codes = [code(k, es) for k in range(1, 13)]
    assert 0 in codes, (kind, model, n, targets, codes)
    b = codes.index(0) + 1
    assert 2 <= b <= 12 and codes[b - 2] == -1 and codes[b - 1] == 0, (kind, model, n, targets, codes)
    assert code(b - 1, control) == 0, (kind, model, n, targets, b)
    return Failure(et, c, conn, model, prm, es, control, step, b, eps)


def failure_rows():
    """(kind, form, scatter, model, params, n): the forms and models of the failure runs at n = unit + 1 and period unit + 1 of
    the lane groups, 9 and 17 elements of the kernels with eight elements per wavefront"""
    out = []
    for kind, forms in (("hex8", (("slot", "atomic"), ("wave", "atomic"), ("wave", "gather"), ("wave_ad", "atomic"), ("auto", "gather"))),
                        ("tet4", (("auto", "atomic"), ("slot", "atomic"))), ("tri3", (("auto", "atomic"),)), ("tri3ps", (("auto", "atomic"),))):
        for form, scatter in forms:
            r = lc.row("group", kind)
            ns = (r.unit + 1, r.period * r.unit + 1) if (kind != "hex8" or form == "slot") else (9, 17)
            models = [(m, p) for m, p, _ in lc.MODELS[kind]]
            if (kind, form, scatter) in (("hex8", "wave", "atomic"), ("tet4", "auto", "atomic")):
                models.append(lc.HOSFORD[:2])
            out += [(kind, form, scatter, m, tuple(p), n) for m, p in models for n in ns]
    return out


FAILURE_ROWS = failure_rows()
fid = lambda r: "%s-%s-%s-%s-%d" % (r[0], r[1], r[2], r[3], r[5])


def failure_targets(kind, form, model, params, n):
    first = yielding_elements(kind, model, params, n, FAIL_EPS[0])
    assert len(first)
    return targets_of(kind, form, n, first[0])


def check_failure_codes(make, fl, run=None):
    """the three return codes of a failure case on a backend: make(elem_set, max_iters) builds it with fl's mesh, model and
    parameters; run(backend) -> code (default: K1 over the whole mesh).  Nothing but the code is compared on a failed call
    (c8.h: outputs are undefined then)."""
    if run is None:
        run = lambda be: be.forward_jacobian(*fl.step, be.new_state(), be.new_linsys())
    got = (run(make(fl.elem_set, fl.b - 1)), run(make(fl.elem_set, fl.b)), run(make(fl.control_set, fl.b - 1)))
    assert got == (-1, 0, 0), (fl.model, len(fl.conn), np.flatnonzero(fl.elem_set).tolist(), fl.b, got)


@functools.lru_cache(maxsize=None)
def one_point_failure(model, params, n, target):
    """hex8: the yield stress of set 1 lowered from ELASTIC_Y until exactly ONE point of the target element yields in the
    second step (bisection on the largest yield stress at which a point yields); None if no yield stress gives one point"""
    et, c, conn = lc.mesh("hex8", n, True)
    es = np.zeros(n, dtype=np.int32)
    es[target] = 1

    def points(y1, eps):
        o = oracle(et, c, conn, model, two_set_params(model, params, y1), elem_set=es)
        return int(_grown(pc.two_steps(o, c, eps)).sum())

    k = YIELD_STRESS[model]
    for eps in FAIL_EPS:
        lo, hi = params[k], 50.0 * params[k]  # lo: points yield; hi: none does
        if points(lo, eps) == 0 or points(hi, eps) != 0:
            continue
        for _ in range(25):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if points(mid, eps) > 0 else (lo, mid)
        y1 = lo - 1e-3 * (hi - lo + 1e-9 * lo)
        for y in (lo, y1):
            if points(y, eps) == 1:
                try:
                    return failure("hex8", model, params, n, (target,), y1=y, want_points=1)
                except AssertionError:
                    continue
    return None


ONE_POINT = [(m, tuple(p), n) for m, p, _ in lc.MODELS["hex8"] for n in (9, 17)]


# ---- 4: the local line search -------------------------------------------------------------------------------------------------
DECK = pc.LOCAL_LINE_SEARCH                      # (1e-4, 0.5, 0.9, 100)
BACKTRACKING = (DECK, (0.45, 0.1, 0.5, 3))       # searches with several evaluations occur (asserted: one evaluation fails)
CAPPED = ((0.999, 0.5, 0.9, 3), (0.999, 0.3, 0.6, 2))  # no full step is ever accepted: every search ends at its cap
LS_MESHES = (("hex8", 2, "wave"), ("tet4", 5, "auto"))


def history_codes(orc, c, eps):
    """the return codes of the two steps of parity_cases.two_steps (which asserts them to be 0), up to the first failure"""
    u1, p1 = fields_for(orc.ndims, *prescribed_fields(c, eps, ramp=True, perturb=5e-2))
    prev, codes = (np.zeros_like(u1), np.zeros_like(p1), orc.new_state()), []
    for u, p in ((u1, p1), (1.5 * u1, 1.5 * p1)):
        xi = orc.new_state()
        codes.append(orc.forward_jacobian(u, p, prev[0], prev[1], prev[2], xi, orc.new_linsys()))
        if codes[-1] != 0:
            break
        prev = (np.ascontiguousarray(u), np.ascontiguousarray(p), xi)
    return codes


def ls_codes(kind, n, model, params, eps, line_search):
    et, c, conn = lc.mesh(kind, n)
    return history_codes(oracle(et, c, conn, model, list(params), line_search=line_search), c, eps)


def ls_case(kind, n, form, model, params, eps):
    return lc.Case("line_search", kind, form, "atomic", model, tuple(params), eps, n, False)


# hypo_hosford and hypo_barlat converge under the second capped setting as well (and fail with its c1 under a cap of 100)
CAP_RUNS = [(lc.HOSFORD[0], prm, 0.004, ls) for prm in (pc.HOSFORD, pc.HOSFORD_100) for ls in CAPPED] + \
           [("hypo_hosford", pc.HOSFORD, 0.004, CAPPED[1]), ("hypo_barlat", pc.BARLAT, 0.006, CAPPED[1])]
cap_id = lambda r: "%s-a%g-%s" % (r[0], r[1][3], "/".join("%g" % x for x in r[3]))
