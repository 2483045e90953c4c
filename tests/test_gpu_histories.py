"""`-m gpu`: non-monotone load histories and trial states on the yield surface through the HIP library, against the
oracle -- the matrix of test_emul_histories.py with every scatter mode and, for small_J2 on hex8, every kernel form by
name.  Forward for every step, the adjoint chain backwards from the last (parity_cases.load_history)."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from parity_cases import (AUDIT, CASES, CASES_2D, CASES_LINE_SEARCH, CASES_PLANE_STRESS, HISTORIES, J2, LOCAL_LINE_SEARCH,
                          check_adjoint_chain, check_forward, check_residual, mesh_2d, mesh_of)

pytestmark = pytest.mark.gpu
TOL = 1e-12
NONPROP = [h for h in HISTORIES if h != "proportional"]
SCATTERS = ["gather", "colored", "atomic"]


def gpu(et, c, conn, model, params, scatter=None, kernel="auto", **kw):
    from gpu_backend import GpuBackend
    return GpuBackend(et, c, conn, model, params, scatter=scatter, kernel=kernel, **kw)


def run(orc, dut, c, model, eps, history, adjoint=True):
    check_forward(orc, dut, c, model, eps, TOL, history=history)
    check_residual(orc, dut, c, eps, TOL, history=history)
    if adjoint:
        check_adjoint_chain(orc, dut, c, model, eps, TOL, history=history)


@pytest.mark.parametrize("scatter", SCATTERS)
@pytest.mark.parametrize("history", NONPROP)
@pytest.mark.parametrize("mesh", ["hex8", "tet4"])
@pytest.mark.parametrize("model,params,eps", CASES)
def test_history_3d(model, params, eps, mesh, history, scatter):
    AUDIT.ctx = "gpu hist %s auto %s" % (mesh, scatter)
    et, c, conn = mesh_of(mesh)
    run(ol.Oracle(et, c, conn, model, params), gpu(et, c, conn, model, params, scatter), c, model, eps, history)


@pytest.mark.parametrize("scatter", ["colored", "atomic"])
@pytest.mark.parametrize("history", NONPROP)
@pytest.mark.parametrize("model,params,eps", CASES_2D + CASES_PLANE_STRESS)
def test_history_2d(model, params, eps, history, scatter):
    AUDIT.ctx = "gpu hist tri3 %s" % scatter
    et, c, conn = mesh_2d("structured")
    run(ol.Oracle(et, c, conn, model, params), gpu(et, c, conn, model, params, scatter), c, model, eps, history)


@pytest.mark.parametrize("history", HISTORIES + ("yield_band",))
@pytest.mark.parametrize("kernel,scatter", [(k, s) for k in ["auto", "node", "wave", "wave_ad", "slot"] for s in SCATTERS
                                            if k != "node" or s == "gather"])  # the row-per-node kernel writes rows
def test_small_J2_kernels(kernel, history, scatter):
    AUDIT.ctx = "gpu hist hex8 %s %s" % (kernel, scatter)
    et, c, conn = mesh_of("hex8")
    # the lane-group adjoint kernel of hex8 cannot stage (refused): its forward and residual only
    run(ol.Oracle(et, c, conn, "small_J2", J2), gpu(et, c, conn, "small_J2", J2, scatter, kernel), c, "small_J2", 0.004,
        history, adjoint=not (kernel == "slot" and scatter == "gather"))


@pytest.mark.parametrize("scatter", SCATTERS)
def test_small_J2_yield_band_tet4(scatter):
    AUDIT.ctx = "gpu hist tet4 auto %s" % scatter
    et, c, conn = mesh_of("tet4")
    run(ol.Oracle(et, c, conn, "small_J2", J2), gpu(et, c, conn, "small_J2", J2, scatter), c, "small_J2", 0.004, "yield_band")


@pytest.mark.parametrize("history", NONPROP)
@pytest.mark.parametrize("kind", ["hex8", "tet4"])
@pytest.mark.parametrize("model,params,eps", CASES_LINE_SEARCH)
def test_history_line_search(model, params, eps, kind, history):
    AUDIT.ctx = "gpu hist %s line search" % kind
    et, c, conn = mesh_of(kind)
    orc = ol.Oracle(et, c, conn, model, params)
    orc.set_local_line_search(*LOCAL_LINE_SEARCH)
    run(orc, gpu(et, c, conn, model, params, line_search=LOCAL_LINE_SEARCH), c, model, eps, history)


@pytest.mark.parametrize("seed", range(int(os.environ.get("C8_FUZZ_SEEDS_HIST", "24"))))
def test_random_history_matches_oracle(seed):
    # the cases of test_gpu_fuzz.random_case (model, element, mesh, strain level, scatter mode, kernel) under a history
    # drawn from the seed as well
    from test_gpu_fuzz import random_case
    model, params, kind, c, conn, eps, scatter, kernel = random_case(seed)
    history = (HISTORIES + ("yield_band",))[np.random.default_rng(9000 + seed).integers(len(HISTORIES) + 1)]
    if history == "yield_band" and model != "small_J2":
        history = "reverse"
    et = ol.HEX8 if kind == "hex8" else ol.TET4
    AUDIT.ctx = "gpu hist fuzz %s %s %s" % (kind, kernel, scatter)
    run(ol.Oracle(et, c, conn, model, params), gpu(et, c, conn, model, params, scatter, kernel), c, model, eps, history,
        adjoint=not (kind == "hex8" and kernel == "slot" and scatter == "gather"))
