"""The tables of settings_cases.py on the CPU: the kernel source run by the lane emulator (tests/emul) against an oracle
with the same ModelSettings, away from the defaults at which every other test runs them.
  1  stabilization multiplier 0.37 and 3.7: the chain K1 .. K5 and the objective on every (form, scatter, model) of the
     launch table, after asserting on the oracle that the multiplier moves what the chain compares; plane stress, which has no
     stabilisation, by bits; the total gradient against differences and against the oracle;
  2  local Newton tolerances (absolute, relative) and the budgets 7 and 8 on either side of the closed-form switch; abs_tol as
     the width of the yield band, with points inside the band on both sides of the surface;
  3  the return code of a local solve that fails in ONE element, at the places where the lane arithmetic could lose it;
  4  the backtracking of the local line search, and its cap.
test_gpu_settings.py runs the same tables through the library on the device."""
import numpy as np
import pytest

import gradient_cases as gc
import launch_cases as lc
import parity_cases as pc
import settings_cases as sc
import test_emul_gradient
import test_oracle_gradient_fd
from parity import rel_vec
from test_emul_launch_edges import emul_config


def by_emulator_run(rows, low_budget=False):
    """one row per distinct emulator run (the emulator has neither scatter modes nor a block remap).  low_budget: below eight
    local iterations no closed form runs, and `node` / `auto` under `gather` is the staged wave kernel"""
    seen, out = set(), []
    for cs in rows:
        cfg = config_of(cs, low_budget)
        key = (cs.kind, cs.model, cs.n, cs.cut, cfg)
        if key not in seen:
            seen.add(key)
            out.append(cs)
    return out


def config_of(cs, low_budget=False):
    wave, closed, staged, node = emul_config(cs)
    if low_budget:
        if node:
            staged, node = True, False  # c8_api.hip: node_rows_applies needs ms.closed_form
        closed = False
    return (wave, closed, staged, node)


def emul_of(cs, low_budget=False, **settings):
    et, c, conn = sc.mesh_of(cs)
    return sc.emulator(config_of(cs, low_budget), et, c, conn, cs.model, list(cs.params), **settings)


def chain(cs, low_budget=False, **settings):
    orc, c, _ = sc.oracle_of(cs, **settings)
    lc.run_chain(orc, emul_of(cs, low_budget, **settings), c, cs.model, cs.eps)
    return orc, c


# ---- 1: the stabilization multiplier ------------------------------------------------------------------------------------------
STAB_ROWS = by_emulator_run(sc.chain_rows() + sc.hosford_rows())


def test_the_rows_cover_the_launch_table():
    rows = sc.chain_rows()
    assert {(cs.kind, cs.form, cs.scatter, cs.model) for cs in rows} == {(cs.kind, cs.form, cs.scatter, cs.model) for cs in lc.chain_cases()}
    assert {(cs.kind, cs.form): cs.n for cs in rows if cs.form in ("slot", "wave")} == \
        {("hex8", "slot"): 3, ("hex8", "wave"): 9, ("tet4", "slot"): 5, ("tri3", "slot"): 8, ("tri3ps", "slot"): 11}
    assert all(cs.cut == (cs.kind == "hex8") for cs in rows)
    assert [(cs.kind, cs.n) for cs in sc.hosford_rows()] == [("hex8", 9), ("tet4", 5)]
    assert len(sc.tolerance_rows()) == 11 and all(s != 1.0 and np.log2(s) != round(np.log2(s)) for s in sc.STAB)


@pytest.mark.parametrize("s", sc.STAB)
@pytest.mark.parametrize("cs", STAB_ROWS, ids=[sc.case_id(cs) for cs in STAB_ROWS])
def test_stab_mult_chain_through_the_emulator(cs, s):
    orc, c, _ = sc.oracle_of(cs)
    plastic, elastic = lc.branches(orc, c, cs)
    assert plastic > 0 and (elastic > 0 or orc.nelems * orc.npts <= 8), (sc.case_id(cs), plastic, elastic)  # as the launch table
    if sc.mixed(cs):
        sc.assert_stab_power(cs, s)
    chain(cs, stab_mult=s)


def test_plane_stress_has_no_stabilisation():
    """one residual, no pressure: the oracle and the kernels give the same bits for stab_mult = 1 and 3.7"""
    rows = [cs for cs in by_emulator_run(sc.chain_rows()) if not sc.mixed(cs)]
    assert rows
    for cs in rows:
        for make in (lambda **kw: sc.oracle_of(cs, **kw)[0], lambda **kw: emul_of(cs, **kw)):
            a, b = (sc.forward_at_step_two(cs, make(stab_mult=s)) for s in (1.0, sc.STAB[1]))
            assert sc.systems_same_bits(a, b, nres=1) and np.abs(a[1].A[0][0]).max() > 0


@pytest.mark.parametrize("rid", sc.GRADIENT_ROWS)
def test_total_gradient_at_stab_mult(rid):
    """the oracle's total gradient against Richardson differences (the bar and the conditions on the reference of
    test_oracle_gradient_fd.py), the emulated kernels' against the oracle's (those of test_emul_gradient.py), and the
    objective itself moved by the multiplier"""
    case = sc.STAB_GRADIENT_CASES[rid]
    test_oracle_gradient_fd.test_oracle_adjoint_gradient_matches_differences_per_parameter(case)
    J1, g1, _ = gc.oracle_reference(gc.BY_NAME[rid])
    J, g, _ = gc.oracle_reference(case)
    assert abs(J - J1) > 1e-6 * abs(J1) and np.abs(g - g1).max() > 1e-6 * np.abs(g1).max(), (J, J1)
    for variant in ("slot",) + (("wave", "node") if case.kind == "hex8" else ()):
        test_emul_gradient.test_emulated_total_gradient_matches_oracle_per_parameter(case, variant)


# ---- 2: tolerances and budget -----------------------------------------------------------------------------------------------------
TOL_ROWS = by_emulator_run(sc.tolerance_rows())


@pytest.mark.parametrize("tols", sc.TOLERANCES, ids=sc.sid)
@pytest.mark.parametrize("cs", TOL_ROWS, ids=[sc.case_id(cs) for cs in TOL_ROWS])
def test_local_tolerances_through_the_emulator(cs, tols):
    orc, c = chain(cs, **tols)
    # the two sides stop at the same iteration: the local state agrees directly, without the allowance of ten times abs_tol
    # that parity_cases.check_forward grants once system and state have been checked against each other
    xo, _ = sc.forward_at_step_two(cs, orc)
    xd, _ = sc.forward_at_step_two(cs, emul_of(cs, **tols))
    assert rel_vec(xd, xo) < sc.TOL, rel_vec(xd, xo)


@pytest.mark.parametrize("budget", sc.BUDGETS)
@pytest.mark.parametrize("cs", by_emulator_run(sc.tolerance_rows(), True), ids=[sc.case_id(cs) for cs in by_emulator_run(sc.tolerance_rows(), True)])
def test_budgets_around_the_closed_form_switch_through_the_emulator(cs, budget):
    chain(cs, low_budget=budget < 8, max_iters=budget)


def test_band_rows_hold_both_forms():
    for kind in ("hex8", "tet4"):  # emul_config: (wave, closed, staged, node)
        assert {emul_config(cs)[1] for cs in sc.BAND_ROWS if cs.kind == kind} == {True, False}


@pytest.mark.parametrize("cs", sc.BAND_ROWS, ids=[sc.case_id(cs) for cs in sc.BAND_ROWS])
def test_wide_yield_band_through_the_emulator(cs):
    eps, orc, c, conn, (above, below) = sc.band_case(cs.kind, cs.n, cs.cut)
    assert above > 0 and below > 0  # points with a trial yield value in (0, abs_tol) and in (-abs_tol, 0)
    et, _, _ = sc.mesh_of(cs)
    dut = sc.emulator(emul_config(cs), et, c, conn, cs.model, list(cs.params), abs_tol=sc.BAND_TOL)
    lc.run_chain(orc, dut, c, cs.model, eps)


# ---- 3: the failure report ----------------------------------------------------------------------------------------------------------
def _emul_failure_rows():
    seen, out = set(), []
    for r in sc.FAILURE_ROWS:
        kind, form, scatter, model, params, n = r
        cfg = config_of(lc.Case("fail", kind, form, scatter, model, params, 0.0, n, kind == "hex8"), True)
        if (kind, model, n, cfg) not in seen:
            seen.add((kind, model, n, cfg))
            out.append(r)
    return out


def test_failure_rows_name_every_form_and_count():
    forms = {(r[0], r[1], r[2]) for r in sc.FAILURE_ROWS}
    assert forms == {("hex8", "slot", "atomic"), ("hex8", "wave", "atomic"), ("hex8", "wave", "gather"), ("hex8", "wave_ad", "atomic"),
                     ("hex8", "auto", "gather"), ("tet4", "auto", "atomic"), ("tet4", "slot", "atomic"), ("tri3", "auto", "atomic"),
                     ("tri3ps", "auto", "atomic")}
    assert {(r[0], r[1], r[5]) for r in sc.FAILURE_ROWS if r[1] in ("slot", "wave") or r[0].startswith("tri")} == \
        {("hex8", "slot", 3), ("hex8", "slot", 17), ("hex8", "wave", 9), ("hex8", "wave", 17), ("tet4", "slot", 5), ("tet4", "slot", 33),
         ("tri3", "auto", 8), ("tri3", "auto", 57), ("tri3ps", "auto", 11), ("tri3ps", "auto", 81)}
    assert {r[3] for r in sc.FAILURE_ROWS} == {"small_J2", "hyper_J2", "hyper_J2_plane_strain", "hyper_J2_plane_stress", "small_hosford"}
    assert sc.targets_of("hex8", "wave", 17, 1) == [1, 15, 16] and sc.targets_of("tri3ps", "auto", 81, 0) == [0, 79, 80]


@pytest.mark.parametrize("row", _emul_failure_rows(), ids=sc.fid)
def test_one_failing_element_is_reported_through_the_emulator(row):
    """-1 at the budget b - 1, 0 at b, 0 at b - 1 when no element is in the yielding set (settings_cases.failure asserts the
    same three on the oracle, and that exactly the target yields)"""
    kind, form, scatter, model, params, n = row
    cfg = config_of(lc.Case("fail", kind, form, scatter, model, params, 0.0, n, kind == "hex8"), True)
    for target in sc.failure_targets(kind, form, model, params, n):
        fl = sc.failure(kind, model, params, n, (target,))
        if model == "small_J2":
            assert fl.b == 2
        sc.check_failure_codes(lambda es, budget: sc.emulator(cfg, fl.et, fl.c, fl.conn, model, fl.params, elem_set=es, max_iters=budget), fl)


def test_one_failing_point_exists_on_a_hex8_mesh():
    assert any(sc.one_point_failure(m, p, n, n - 1) is not None for m, p, n in sc.ONE_POINT)


@pytest.mark.parametrize("model,params,n", sc.ONE_POINT, ids=["%s-%d" % (m, n) for m, _, n in sc.ONE_POINT])
@pytest.mark.parametrize("staged", [False, True], ids=["atomic", "gather"])
def test_one_failing_point_is_reported_through_the_emulator(model, params, n, staged):
    """the yield stress of the target's set lowered until exactly ONE of its eight points yields: one lane group of the
    wavefront raises the flag"""
    fl = sc.one_point_failure(model, params, n, n - 1)
    if fl is None:
        pytest.skip("no yield stress leaves exactly one point of element %d yielding" % (n - 1))
    sc.check_failure_codes(lambda es, budget: sc.emulator((True, False, staged, False), fl.et, fl.c, fl.conn, model, fl.params,
                                                         elem_set=es, max_iters=budget), fl)


# ---- 4: the local line search ---------------------------------------------------------------------------------------------------------
def ls_chain(kind, n, form, model, params, eps, line_search):
    cs = sc.ls_case(kind, n, form, model, params, eps)
    orc, c, _ = sc.oracle_of(cs, line_search=line_search)
    lc.run_chain(orc, emul_of(cs, line_search=line_search), c, model, eps)


@pytest.mark.parametrize("line_search", sc.BACKTRACKING, ids=lambda t: "/".join("%g" % x for x in t))
@pytest.mark.parametrize("kind,n,form", sc.LS_MESHES, ids=[m[0] for m in sc.LS_MESHES])
def test_backtracking_line_search_through_the_emulator(kind, n, form, line_search):
    """Hosford's exponent 100: with one evaluation per search (plain Newton) the oracle fails and with the deck's hundred it
    converges, so searches with several evaluations occur -- the cubic model and its safeguards run"""
    model, eps = lc.HOSFORD[0], lc.HOSFORD[2]
    assert -1 in sc.ls_codes(kind, n, model, pc.HOSFORD_100, eps, sc.DECK[:3] + (1,))
    assert sc.ls_codes(kind, n, model, pc.HOSFORD_100, eps, sc.DECK) == [0, 0]
    ls_chain(kind, n, form, model, pc.HOSFORD_100, eps, line_search)


@pytest.mark.parametrize("run", sc.CAP_RUNS, ids=sc.cap_id)
@pytest.mark.parametrize("kind,n,form", sc.LS_MESHES, ids=[m[0] for m in sc.LS_MESHES])
def test_line_search_cap_through_the_emulator(kind, n, form, run):
    """c1 = 0.999: the sufficient-decrease test cannot hold at a full step.  With a cap of 100 the oracle fails (the step
    shrinks away), so in the capped runs every search ends at its cap and takes the lowest-merit step"""
    model, params, eps, line_search = run
    assert -1 in sc.ls_codes(kind, n, model, params, eps, line_search[:3] + (100,))
    ls_chain(kind, n, form, model, params, eps, line_search)
