"""`-m gpu`: the device drivers' total gradient per parameter.  PrimalDriver (c8_primal_solve_step) through the load
history of gradient_cases.py, then calibr8_amd.primal.adjoint_gradient (c8_adjoint_solve_step marched backwards) once per
active group, against the oracle's total gradient (fe_driver) at 1e-8 of the largest scaled component; the objective values
agree to 1e-10.  No differences are taken on the device: test_oracle_gradient_fd.py carries the oracle's gradient to central
differences of the objective, and this test carries the device's gradient to the oracle's.

Every case of the table (all rows of C8_MODEL_TABLE on hex8 / tet4 or tri3, the three calibration cases, the case with two
element sets, the hybrid row with its appended weight block) under the library's own kernel choice; small_J2 also under
`wave_ad` and `slot` on hex8 (its `auto` is the row-per-node assembly with K4 / K5 in closed form) and `slot` on tet4."""
import types

import numpy as np
import pytest

import gradient_cases as gc
import parity_cases as pc

pytestmark = pytest.mark.gpu

RUNS = [(c, "auto") for c in gc.CASES] + \
       [(gc.BY_NAME["small_J2-hex8"], k) for k in ("wave_ad", "slot")] + [(gc.BY_NAME["small_J2-tet4"], "slot")]


def device_primal(case, kernel, measured):
    """the case on the device: Assembler, PrimalDriver solved through the load steps"""
    from calibr8_amd import Assembler
    from calibr8_amd.primal import PrimalDriver
    args, kw = case.backend_kw(case.params)
    if case.hybrid:
        kw["embedded"] = case.embedded(case.params)
    if case.model in gc.LINE_SEARCH:
        kw["line_search"] = pc.LOCAL_LINE_SEARCH
    asm = Assembler(*args, **kw)
    asm.set_kernel(kernel)
    if case.objective == "calibration":
        faces, ckw = case.calibration_kw()
        asm.set_qoi_calibration(faces, **ckw)
    drv = PrimalDriver(asm, case.dbc_spec(), max_iters=30, abs_tol=1e-12, rel_tol=1e-12).solve(gc.NSTEPS)
    if case.objective == "calibration":
        drv.set_measured([None] + [asm.dev(u) for u in measured[0][1:]], measured[1])
    return drv


@pytest.mark.parametrize("case,kernel", RUNS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_device_total_gradient_matches_oracle_per_parameter(case, kernel):
    from calibr8_amd.primal import adjoint_gradient
    J, g, ref = gc.oracle_reference(case)
    drv = device_primal(case, kernel, ref.measured if case.objective == "calibration" else None)
    asm = drv.asm
    assert drv.newton_iters == ref.newton_iters, (drv.newton_iters, ref.newton_iters)
    Jd = drv.qoi()
    assert abs(Jd - J) <= 1e-10 * abs(J), (Jd, J)
    gc.check_history(case, types.SimpleNamespace(xi=[x.cpu().numpy() for x in drv.xi]))
    n_tail = asm.num_embedded_params
    assert n_tail == (len(gc.NET.theta) if case.hybrid else 0)
    marches = [0]

    def march(group):
        for s, idx in group.items():
            asm.set_active(s, idx)
        n = sum(len(v) for v in group.values()) + n_tail
        assert asm.num_grad_params == n
        marches[0] += 1
        return adjoint_gradient(drv, n)

    worst = gc.check_groups_against_oracle(case, march, n_tail)
    assert 1 <= marches[0] <= 4
    if case.hybrid:
        assert np.abs(g[3:]).max() > 0.0
    print("%s %s worst ratio %.2e" % (case.name, kernel, worst))
