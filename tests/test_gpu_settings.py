"""`-m gpu`: the tables of settings_cases.py through the library on the device -- c8_create's plumbing of the model
descriptor into ModelSettings, the form selection of c8_set_kernel_variant at the budget of eight local iterations, the launch
wrappers, and c8_status.  test_emul_settings.py runs the same tables on the CPU and holds the tests of the tables themselves.
  1  stabilization multiplier 0.37 and 3.7: the chain on every (form, scatter, model) of the launch table; plane stress and
     c8_eval_cauchy by bits; the error kernels against their host harnesses; the total gradient and the Newton driver;
  2  local tolerances; the closed form from a budget of 8 on and the iterated form below it, by bits; the wide yield band;
  3  C8_LOCAL_SOLVE_FAILED from one element at the ragged ends of the launches, from one point of a wavefront, from an
     element subset, and through c8_status in synchronous and asynchronous mode;
  4  the backtracking of the local line search, and its cap."""
import numpy as np
import pytest

import cauchy_cases as cc
import error_cases as ec
import exact_cases as xc
import launch_cases as lc
import oracle_lib as ol
import parity_cases as pc
import settings_cases as sc
import test_gpu_error
import test_gpu_exact_errors
import test_gpu_gradient
from fe_driver import Dbc, Primal
from meshes import brick, fields_for, jiggle, prescribed_fields
from parity import rel_vec
from test_gpu_launch_edges import device

pytestmark = pytest.mark.gpu


def dev_of(cs, **settings):
    et, c, conn = sc.mesh_of(cs)
    return device(cs.form, cs.scatter)(et, c, conn, cs.model, list(cs.params), **settings)


def chain(cs, **settings):
    orc, c, _ = sc.oracle_of(cs, **settings)
    dut = dev_of(cs, **settings)
    assert dut.nelems == orc.nelems and dut.asm.scatter == cs.scatter
    lc.run_chain(orc, dut, c, cs.model, cs.eps)
    return orc, dut


# ---- 1: the stabilization multiplier ------------------------------------------------------------------------------------------
STAB_ROWS = sc.chain_rows() + sc.hosford_rows()


@pytest.mark.parametrize("s", sc.STAB)
@pytest.mark.parametrize("cs", STAB_ROWS, ids=[sc.case_id(cs) for cs in STAB_ROWS])
def test_stab_mult_chain(cs, s):
    if sc.mixed(cs):
        sc.assert_stab_power(cs, s)
    chain(cs, stab_mult=s)


def test_plane_stress_has_no_stabilisation():
    """one residual, no pressure: the same bits for stab_mult = 1 and 3.7, in both forms of the lane-group kernel.  Under
    `colored` (the element type has no staged assembly), where no two elements of a launch add into the same entry and the
    sums have a fixed order"""
    rows = [cs._replace(scatter="colored") for cs in sc.chain_rows() if not sc.mixed(cs)]
    assert [cs.form for cs in rows] == ["auto", "slot"]
    for cs in rows:
        a, b = (sc.forward_at_step_two(cs, dev_of(cs, stab_mult=s)) for s in (1.0, sc.STAB[1]))
        assert sc.systems_same_bits(a, b, nres=1) and np.abs(a[1].A[0][0]).max() > 0
        o1, o2 = (sc.forward_at_step_two(cs, sc.oracle_of(cs, stab_mult=s)[0]) for s in (1.0, sc.STAB[1]))
        assert sc.systems_same_bits(o1, o2, nres=1)


ERROR_ROWS = ("small_J2-hex8", "hyper_J2-tet4", "hyper_J2_plane_strain-tri3")


@pytest.fixture(scope="session")
def error_harness(tmp_path_factory):
    return ec.build_harness(tmp_path_factory.mktemp("c8_error_host_settings"))


@pytest.fixture(scope="session")
def exact_harness(tmp_path_factory):
    return xc.build_harness(tmp_path_factory.mktemp("c8_exact_host_settings"))


def assembler(cs, **settings):
    from calibr8_amd import Assembler
    return Assembler(cs.et, cs.c, cs.conn, cs.model, cs.params, **cs.assembler_kw(), **settings)


@pytest.mark.parametrize("rid", ERROR_ROWS)
def test_error_kernels_at_stab_mult(error_harness, exact_harness, rid):
    """c8_eval_error_contributions, c8_eval_exact_errors and c8_eval_linearization_errors with stab_mult = 3.7 against their
    host harnesses with the same multiplier, at the bars of test_gpu_error.py and test_gpu_exact_errors.py; the harness's
    E_R moves with the multiplier by more than 1e-5 of its largest entry (measured on the harness: 1.2e-4 .. 6e-3), seven orders
    above those bars, and its E_C not at all"""
    s = sc.STAB[1]
    cs = cc.case(rid)
    asm = assembler(cs, stab_mult=s)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    kw = dict(nn=cs.nn, scales=True)
    ref = ec.host_error(error_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *st, *adj, stab_mult=s, **kw)
    one = ec.host_error(error_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *st, *adj, **kw)
    assert np.abs(ref[0] - one[0]).max() > 1e-5 * np.abs(one[0]).max() and np.array_equal(ref[1], one[1])
    test_gpu_error.assert_close(test_gpu_error.device_error(asm, st, adj), ref, rid, st, adj[2])
    fine = xc.moved(st, xc.direction(cs, 31))
    for lin in (False, True):
        ref = xc.host_exact(exact_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, st, fine, *adj, lin=lin, stab_mult=s, **kw)
        one = xc.host_exact(exact_harness, cs.et, cs.c, cs.conn, cs.model, cs.params, st, fine, *adj, lin=lin, **kw)
        assert np.abs(ref[0] - one[0]).max() > 1e-5 * np.abs(one[0]).max() and np.array_equal(ref[1], one[1]), (rid, lin)
        dev = test_gpu_exact_errors.device_exact(asm, st, fine, adj, lin=lin)
        test_gpu_exact_errors.assert_close(dev, ref, (rid, "lin" if lin else "exact", s), st, fine, adj[2])


@pytest.mark.parametrize("rid", ERROR_ROWS)
def test_cauchy_does_not_read_stab_mult(rid):
    import torch
    cs = cc.case(rid)
    out = []
    for s in (1.0, sc.STAB[1]):
        asm = assembler(cs, stab_mult=s)
        out.append(asm.cauchy(*[asm.dev(a) for a in cs.state]))
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]) and float(out[0].abs().max()) > 0


@pytest.mark.parametrize("rid", sc.GRADIENT_ROWS)
def test_total_gradient_at_stab_mult(rid):
    """the device drivers' total gradient against the oracle's with the same multiplier (test_gpu_gradient.py's check and
    bar); test_emul_settings.py carries that oracle gradient to differences"""
    test_gpu_gradient.test_device_total_gradient_matches_oracle_per_parameter(sc.STAB_GRADIENT_CASES[rid], "auto")


def test_device_newton_driver_at_stab_mult():
    """test_gpu_primal.py::test_device_newton_driver_matches_oracle_driven_newton with stab_mult = 3.7 on both sides"""
    from calibr8_amd import Assembler, PrimalDriver
    s = sc.STAB[1]
    c, conn, sets = brick(3, 4, 3, 1.0, 1.5, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    pull = lambda x, y, z, t: 0.003 * t
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero),
            (0, 1, sets["ymax"], pull), (0, 0, sets["ymax"], zero)]
    solve = lambda be: Primal(be, c, [Dbc(*d) for d in spec], max_iters=15, abs_tol=1e-10, rel_tol=1e-10).solve(3)
    ref = solve(ol.Oracle(ol.HEX8, c, conn, "small_J2", pc.J2, stab_mult=s))
    one = solve(ol.Oracle(ol.HEX8, c, conn, "small_J2", pc.J2))
    assert np.abs(ref.p[3] - one.p[3]).max() > 1e-3 * np.abs(one.p[3]).max()  # the multiplier moves the solution
    asm = Assembler(8, c, conn, "small_J2", pc.J2, stab_mult=s)
    pr = PrimalDriver(asm, spec, max_iters=15, abs_tol=1e-10, rel_tol=1e-10).solve(3)
    assert pr.newton_iters == ref.newton_iters
    for k in range(1, 4):
        assert np.abs(pr.u[k].cpu().numpy() - ref.u[k]).max() < 1e-10 * np.abs(ref.u[k]).max()
        assert np.abs(pr.p[k].cpu().numpy() - ref.p[k]).max() < 1e-10 * np.abs(ref.p[k]).max()
        assert np.abs(pr.xi[k].cpu().numpy() - ref.xi[k]).max() < 1e-10
    assert abs(pr.qoi() - ref.qoi()) < 1e-12


# ---- 2: tolerances and budget -----------------------------------------------------------------------------------------------------
TOL_ROWS = sc.tolerance_rows()


@pytest.mark.parametrize("tols", sc.TOLERANCES, ids=sc.sid)
@pytest.mark.parametrize("cs", TOL_ROWS, ids=[sc.case_id(cs) for cs in TOL_ROWS])
def test_local_tolerances(cs, tols):
    orc, dut = chain(cs, **tols)
    # the two sides stop at the same iteration: the local state agrees directly, without the allowance of ten times abs_tol
    # that parity_cases.check_forward grants once system and state have been checked against each other
    xo, _ = sc.forward_at_step_two(cs, orc)
    xd, _ = sc.forward_at_step_two(cs, dut)
    assert rel_vec(xd, xo) < sc.TOL, rel_vec(xd, xo)


def _gather_run(kind, n, form, **settings):
    """(xi, system) of K1 on small_J2 under the staged assembly (the same bits from run to run)"""
    cs = lc.Case("budget", kind, form, "gather", "small_J2", tuple(pc.J2), 0.004, n, kind == "hex8")
    return sc.forward_at_step_two(cs, dev_of(cs, **settings))


@pytest.mark.parametrize("kind,n,forms,iterated", [("hex8", 9, ("auto", "wave"), "wave_ad"), ("tet4", 5, ("auto",), "slot")], ids=["hex8", "tet4"])
def test_the_closed_form_runs_from_a_budget_of_eight_on(kind, n, forms, iterated):
    """by bits, as test_gpu_parity.py::test_closed_form_against_iterated_form: at max_iters = 8 the library's choice and (hex8)
    `wave` give what they give at 500, the closed form; at 7 they give what the explicitly iterated form gives.  The two
    forms differ in the rounding of A00, so the bits tell them apart."""
    explicit = _gather_run(kind, n, iterated, max_iters=500)
    for form in forms:
        closed = _gather_run(kind, n, form, max_iters=500)
        assert not sc.same_bits(closed[1].A[0][0], explicit[1].A[0][0]), (kind, form, "the forms cannot be told apart")
        assert sc.systems_same_bits(_gather_run(kind, n, form, max_iters=8), closed), (kind, form, 8)
        assert sc.systems_same_bits(_gather_run(kind, n, form, max_iters=7), explicit), (kind, form, 7)
        assert sc.systems_same_bits(_gather_run(kind, n, iterated, max_iters=7), explicit), (kind, iterated, 7)


def test_below_eight_iterations_the_row_per_node_form_is_refused_and_auto_runs_the_staged_wave_form():
    from calibr8_amd import Assembler, C8Error, lib
    et, c, conn = lc.mesh("hex8", 9, True)
    asm = Assembler(et, c, conn, "small_J2", pc.J2, max_iters=7, scatter="gather")
    with pytest.raises(C8Error) as ei:
        asm.set_kernel("node")
    assert ei.value.code == lib.C8_ERR_UNSUPPORTED
    Assembler(et, c, conn, "small_J2", pc.J2, max_iters=8, scatter="gather").set_kernel("node")
    cs = next(r for r in TOL_ROWS if (r.form, r.scatter, r.model) == ("auto", "gather", "small_J2"))
    chain(cs, max_iters=7)


BUDGET_ROWS = [cs for cs in TOL_ROWS if cs.form != "node"]


@pytest.mark.parametrize("budget", sc.BUDGETS)
@pytest.mark.parametrize("cs", BUDGET_ROWS, ids=[sc.case_id(cs) for cs in BUDGET_ROWS])
def test_budgets_around_the_closed_form_switch(cs, budget):
    chain(cs, max_iters=budget)


@pytest.mark.parametrize("cs", sc.BAND_ROWS, ids=[sc.case_id(cs) for cs in sc.BAND_ROWS])
def test_wide_yield_band(cs):
    eps, orc, c, conn, (above, below) = sc.band_case(cs.kind, cs.n, cs.cut)
    assert above > 0 and below > 0  # points with a trial yield value in (0, abs_tol) and in (-abs_tol, 0)
    dut = device(cs.form, cs.scatter)(orc.elem_type, c, conn, cs.model, list(cs.params), abs_tol=sc.BAND_TOL)
    lc.run_chain(orc, dut, c, cs.model, eps)


# ---- 3: the failure report ----------------------------------------------------------------------------------------------------------
def maker(form, scatter, fl):
    return lambda es, budget: device(form, scatter)(fl.et, fl.c, fl.conn, fl.model, fl.params, elem_set=es, max_iters=budget)


@pytest.mark.parametrize("row", sc.FAILURE_ROWS, ids=sc.fid)
def test_one_failing_element_is_reported(row):
    """-1 at the budget b - 1, 0 at b, 0 at b - 1 when no element is in the yielding set (settings_cases.failure asserts the
    same three on the oracle, and that exactly the target yields); nothing but the code is compared"""
    kind, form, scatter, model, params, n = row
    for target in sc.failure_targets(kind, form, model, params, n):
        fl = sc.failure(kind, model, params, n, (target,))
        if model == "small_J2":
            assert fl.b == 2
        sc.check_failure_codes(maker(form, scatter, fl), fl)


@pytest.mark.parametrize("model,params,n", sc.ONE_POINT, ids=["%s-%d" % (m, n) for m, _, n in sc.ONE_POINT])
@pytest.mark.parametrize("form,scatter", [("wave", "atomic"), ("wave", "gather"), ("wave_ad", "atomic")])
def test_one_failing_point_is_reported(model, params, n, form, scatter):
    fl = sc.one_point_failure(model, params, n, n - 1)
    if fl is None:
        pytest.skip("no yield stress leaves exactly one point of element %d yielding" % (n - 1))
    sc.check_failure_codes(maker(form, scatter, fl), fl)


SUBSET_ROWS = [("hex8", "wave", "small_J2", tuple(pc.J2), 9), ("hex8", "wave", "hyper_J2", tuple(pc.HJ2), 9),
               ("hex8", "slot", "small_J2", tuple(pc.J2), 3), ("tet4", "auto", "hyper_J2", tuple(pc.HJ2), 5),
               ("tri3ps", "auto", "hyper_J2_plane_stress", tuple(pc.HJ2_PSS), 11)]


@pytest.mark.parametrize("kind,form,model,params,n", SUBSET_ROWS, ids=["%s-%s-%s" % r[:3] for r in SUBSET_ROWS])
def test_element_subset_reports_the_failure_of_a_listed_element_only(kind, form, model, params, n):
    """c8_assemble_forward_jacobian_subset at the budget b - 1: -1 when the failing element (the single one of the ragged last
    unit) is in the list, 0 when the list holds every other element"""
    import torch
    fl = sc.failure(kind, model, params, n, (n - 1,))
    be = maker(form, "atomic", fl)(fl.elem_set, fl.b - 1)
    asm = be.asm
    state = [asm.dev(a) for a in fl.step]

    def subset(elems):
        lst = torch.as_tensor(np.ascontiguousarray(elems, dtype=np.int32)).to(asm.device)
        return asm.forward_jacobian_subset(*state, asm.new_state(), asm.new_linsys(), lst)

    assert subset([n - 1]) == -1
    assert subset(np.arange(n - 1)) == 0
    assert subset([0, n - 1]) == -1
    assert subset(np.arange(n - 1)[::-1]) == 0
    assert asm.status() == 0


STATUS_ROWS = [("hex8", "wave", "atomic", "small_J2", tuple(pc.J2), 9), ("hex8", "auto", "gather", "hyper_J2", tuple(pc.HJ2), 9),
               ("hex8", "slot", "atomic", "small_J2", tuple(pc.J2), 3), ("tet4", "auto", "atomic", "hyper_J2", tuple(pc.HJ2), 5),
               ("tri3", "auto", "atomic", "hyper_J2_plane_strain", tuple(pc.HJ2_PS), 8),
               ("tri3ps", "auto", "atomic", "hyper_J2_plane_stress", tuple(pc.HJ2_PSS), 11),
               ("tet4", "auto", "atomic", "small_hosford", tuple(pc.HOSFORD), 5)]


def _small_step(fl):
    """a small step from the initial state at which no point yields and the oracle converges within the budget b - 1 (asserted);
    for return codes only: at strains of 5e-4 the residual of a finite-deformation model is a cancelled sum"""
    orc = sc.oracle(fl.et, fl.c, fl.conn, fl.model, fl.params, elem_set=fl.elem_set, max_iters=fl.b - 1)
    u, p = fields_for(orc.ndims, *prescribed_fields(fl.c, 0.0005, perturb=5e-2))
    step = (u, p, np.zeros_like(u), np.zeros_like(p), orc.new_state())
    xi = orc.new_state()
    assert orc.forward_jacobian(*step, xi, orc.new_linsys()) == 0 and np.array_equal(xi[:, :, -1], step[4][:, :, -1])
    return step


def _recovery(be, fl):
    """the failed step once more with the yield stress of the target's set raised as well: elastic everywhere, within the
    budget b - 1 (asserted on the oracle).  Returns the backend's code and its deviations from the oracle."""
    elastic = [fl.params[0], fl.params[0]]
    orc = sc.oracle(fl.et, fl.c, fl.conn, fl.model, elastic, elem_set=fl.elem_set, max_iters=fl.b - 1)
    be.set_params(elastic)
    ls_o, xo, ls_d, xd = orc.new_linsys(), orc.new_state(), be.new_linsys(), be.new_state()
    assert orc.forward_jacobian(*fl.step, xo, ls_o) == 0 and np.array_equal(xo[:, :, -1], fl.step[4][:, :, -1])
    rc = be.forward_jacobian(*fl.step, xd, ls_d)
    errs = pc.compare_systems(orc, ls_d, ls_o)
    errs["xi"] = rel_vec(xd, xo)
    return rc, errs


@pytest.mark.parametrize("kind,form,scatter,model,params,n", STATUS_ROWS, ids=["%s-%s-%s-%s" % r[:4] for r in STATUS_ROWS])
def test_failure_report_in_synchronous_mode_and_recovery(kind, form, scatter, model, params, n):
    from calibr8_amd import lib
    fl = sc.failure(kind, model, params, n, (n - 1,))
    be = maker(form, scatter, fl)(fl.elem_set, fl.b - 1)
    assert be.forward_jacobian(*fl.step, be.new_state(), be.new_linsys()) == lib.C8_LOCAL_SOLVE_FAILED == -1
    assert b"did not converge" in be.asm.L.c8_last_error()
    assert be.asm.status() == 0  # the flag was taken with the call's own return
    # the context recovers in its results, not only in its code
    rc, errs = _recovery(be, fl)
    assert rc == 0 and max(errs.values()) < sc.TOL, errs


@pytest.mark.parametrize("kind,form,scatter,model,params,n", STATUS_ROWS, ids=["%s-%s-%s-%s" % r[:4] for r in STATUS_ROWS])
def test_failure_report_in_asynchronous_mode(kind, form, scatter, model, params, n):
    """on the context's stream: the failing assembly and a converging one behind it both return 0, c8_status reports the
    failure exactly once"""
    fl = sc.failure(kind, model, params, n, (n - 1,))
    be = maker(form, scatter, fl)(fl.elem_set, fl.b - 1)
    asm = be.asm
    small = _small_step(fl)
    asm.set_async(1)
    try:
        assert be.forward_jacobian(*fl.step, be.new_state(), be.new_linsys()) == 0
        assert be.forward_jacobian(*small, be.new_state(), be.new_linsys()) == 0
        assert asm.status() == -1
        assert b"did not converge" in asm.L.c8_last_error()
        assert asm.status() == 0
    finally:
        asm.set_async(0)
    rc, errs = _recovery(be, fl)
    assert rc == 0 and max(errs.values()) < sc.TOL, errs


# ---- 4: the local line search ---------------------------------------------------------------------------------------------------------
def ls_chain(kind, n, form, model, params, eps, line_search):
    cs = sc.ls_case(kind, n, form, model, params, eps)
    orc, c, _ = sc.oracle_of(cs, line_search=line_search)
    lc.run_chain(orc, dev_of(cs, line_search=line_search), c, model, eps)


@pytest.mark.parametrize("line_search", sc.BACKTRACKING, ids=lambda t: "/".join("%g" % x for x in t))
@pytest.mark.parametrize("kind,n,form", sc.LS_MESHES, ids=[m[0] for m in sc.LS_MESHES])
def test_backtracking_line_search(kind, n, form, line_search):
    """Hosford's exponent 100: with one evaluation per search (plain Newton) the oracle fails and with the deck's hundred it
    converges, so searches with several evaluations occur -- the cubic model and its safeguards run"""
    model, eps = lc.HOSFORD[0], lc.HOSFORD[2]
    assert -1 in sc.ls_codes(kind, n, model, pc.HOSFORD_100, eps, sc.DECK[:3] + (1,))
    assert sc.ls_codes(kind, n, model, pc.HOSFORD_100, eps, sc.DECK) == [0, 0]
    ls_chain(kind, n, form, model, pc.HOSFORD_100, eps, line_search)


@pytest.mark.parametrize("run", sc.CAP_RUNS, ids=sc.cap_id)
@pytest.mark.parametrize("kind,n,form", sc.LS_MESHES, ids=[m[0] for m in sc.LS_MESHES])
def test_line_search_cap(kind, n, form, run):
    """c1 = 0.999: the sufficient-decrease test cannot hold at a full step.  With a cap of 100 the oracle fails (the step
    shrinks away), so in the capped runs every search ends at its cap and takes the lowest-merit step"""
    model, params, eps, line_search = run
    assert -1 in sc.ls_codes(kind, n, model, params, eps, line_search[:3] + (100,))
    ls_chain(kind, n, form, model, params, eps, line_search)
