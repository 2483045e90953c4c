"""Non-monotone load histories and trial states on the yield surface, through the kernel source on the CPU (lane
emulator) against the oracle.  Every other parity case runs the proportional history 0 -> u1 -> 1.5 u1; here the
kernels also see a hold and an elastic unloading of yielded points, reversed plastic flow from a nonzero plastic strain,
a rotating flow direction, unloading and reloading, and (small_J2) homogeneous trial states whose yield value lies in,
at and around the band |f0| < abs_tol where the local Newton iteration of the reference stops before its first step.
Both sides get the oracle's inputs at every step (parity_cases.load_history); forward for every step, the adjoint chain
backwards from the last."""
import pytest

import emul_lib as em
import oracle_lib as ol
from parity_cases import (CASES, CASES_2D, CASES_LINE_SEARCH, CASES_PLANE_STRESS, HISTORIES, J2, LOCAL_LINE_SEARCH,
                          check_adjoint_chain, check_forward, check_residual, mesh_2d, mesh_of)

TOL = 1e-12
NONPROP = [h for h in HISTORIES if h != "proportional"]  # the proportional history runs in test_emul_parity.py


def run(orc, dut, c, model, eps, history):
    check_forward(orc, dut, c, model, eps, TOL, history=history)
    check_residual(orc, dut, c, eps, TOL, history=history)
    check_adjoint_chain(orc, dut, c, model, eps, TOL, history=history)


@pytest.mark.parametrize("history", NONPROP)
@pytest.mark.parametrize("mesh", ["hex8", "tet4"])
@pytest.mark.parametrize("model,params,eps", CASES)
def test_history_3d(model, params, eps, mesh, history):
    et, c, conn = mesh_of(mesh)
    run(ol.Oracle(et, c, conn, model, params), em.Emul(et, c, conn, model, params), c, model, eps, history)


@pytest.mark.parametrize("history", NONPROP)
@pytest.mark.parametrize("model,params,eps", CASES_2D + CASES_PLANE_STRESS)
def test_history_2d(model, params, eps, history):
    et, c, conn = mesh_2d("structured")
    run(ol.Oracle(et, c, conn, model, params), em.Emul(et, c, conn, model, params), c, model, eps, history)


# small_J2 on hex8 through each kernel form: (wave, node, closed, staged) of emul_lib.Emul
FORMS = {"slot": (False, False, True, False), "wave": (True, False, True, False), "wave_ad": (True, False, False, False),
         "node": (True, True, True, False), "staged": (True, True, True, True)}


@pytest.mark.parametrize("history", HISTORIES + ("yield_band",))
@pytest.mark.parametrize("form", list(FORMS))
def test_small_J2_kernel_forms(form, history):
    et, c, conn = mesh_of("hex8")
    orc, dut = ol.Oracle(et, c, conn, "small_J2", J2), em.Emul(et, c, conn, "small_J2", J2)
    dut.wave, dut.node, dut.closed, dut.staged = FORMS[form]
    run(orc, dut, c, "small_J2", 0.004, history)


@pytest.mark.parametrize("mesh", ["hex8", "tet4"])
def test_small_J2_yield_band(mesh):
    # the lane-group kernels (tet4: closed form in K1; hex8: the library's default form of the emulator)
    et, c, conn = mesh_of(mesh)
    run(ol.Oracle(et, c, conn, "small_J2", J2), em.Emul(et, c, conn, "small_J2", J2), c, "small_J2", 0.004, "yield_band")


@pytest.mark.parametrize("history", NONPROP)
@pytest.mark.parametrize("model,params,eps,kind,wave", [CASES_LINE_SEARCH[1] + ("hex8", True),
                                                        CASES_LINE_SEARCH[3] + ("tet4", False)])
def test_history_line_search(model, params, eps, kind, wave, history):
    et, c, conn = mesh_of(kind)
    orc, dut = ol.Oracle(et, c, conn, model, params), em.Emul(et, c, conn, model, params)
    orc.set_local_line_search(*LOCAL_LINE_SEARCH)
    dut.set_local_line_search(*LOCAL_LINE_SEARCH)
    dut.wave = wave
    run(orc, dut, c, model, eps, history)
