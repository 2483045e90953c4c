"""The kernel source, run by the CPU lane emulator under the host drivers (fe_driver.Primal and adjoint_gradient), against
the oracle's total gradient per parameter: every case of gradient_cases.py, 1e-8 of the largest scaled component (the figure
of test_gpu_primal.py's device check, made relative to the scale so that tiny components do not divide by themselves).
test_oracle_gradient_fd.py carries the oracle's gradient to central differences; together they carry the kernels' there.

The primal is solved once per case on the emulated kernels; the adjoint march is repeated per active group
(gradient_cases.active_groups: every parameter appears, one list is in descending order, one has the full lane width, one
is a single parameter; the two-set case has lists of 8 and 1).  K5 maps lane k to active[k] and to slot act[0] + k: every
component must equal the component of the all-active oracle gradient, whatever its lane."""
import numpy as np
import pytest

import emul_lib as em
import gradient_cases as gc
import parity_cases as pc
from fe_driver import adjoint_gradient
from test_emul_hybrid import HybridEmul, emu, emul_theta_gradient  # noqa: F401  (emu: the hybrid emulator's fixture)

# kernel forms per case: the lane-group ("slot") kernels everywhere; on hex8 also one wavefront per element ("wave"), and
# for small_J2 the row-per-node assembly with K4 and K5 in closed form ("node"), the library's choice there
RUNS = [(c, v) for c in gc.CASES if not c.hybrid
        for v in ("slot",) + (("wave",) if c.kind == "hex8" else ()) + (("node",) if (c.model, c.kind) == ("small_J2", "hex8") else ())]


def emulator(case, variant):
    args, kw = case.backend_kw(case.params)
    dut = em.Emul(*args, **kw)
    if case.model in gc.LINE_SEARCH:
        dut.set_local_line_search(*pc.LOCAL_LINE_SEARCH)
    dut.wave = variant in ("wave", "node")
    dut.node = variant == "node"
    return dut


def march_groups(case, pr, n_tail=0):
    def march(group):
        for s, idx in group.items():
            pr.be.set_active(s, idx)
        return adjoint_gradient(pr, sum(len(v) for v in group.values()) + n_tail)
    return gc.check_groups_against_oracle(case, march, n_tail)


@pytest.mark.parametrize("case,variant", RUNS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_emulated_total_gradient_matches_oracle_per_parameter(case, variant):
    J, g, ref = gc.oracle_reference(case)
    measured = ref.measured if case.objective == "calibration" else None
    pr = case.primal(emulator(case, variant), measured)
    assert pr.newton_iters == ref.newton_iters
    assert abs(pr.qoi() - J) <= 1e-10 * abs(J)
    gc.check_history(case, pr)
    print("%s %s worst ratio %.2e" % (case.name, variant, march_groups(case, pr)))


class HybridTotal(HybridEmul):
    """HybridEmul whose K5 appends the weight-gradient kernel's result, as the library's c8_param_gradient does"""

    def qoi_gradient(self, u, p, up, pp, xip, xi, z_u, z_p, phi, nparams):
        nt = len(gc.NET.theta)
        lanes = super().qoi_gradient(u, p, up, pp, xip, xi, z_u, z_p, phi, nparams - nt)
        return np.concatenate([lanes, emul_theta_gradient(self.emu, gc.NET, xi, phi)])


def test_emulated_hybrid_total_gradient_with_weights_matches_oracle(emu):  # noqa: F811
    # E nu Y through the lane groups, the four weights through the weight-gradient kernel with the march's own phi at every
    # step: the theta block as a TOTAL derivative through the steps
    case = gc.BY_NAME["%s-tri3" % gc.HYB]
    J, g, ref = gc.oracle_reference(case)
    et, c, conn, _ = gc.mesh("tri3")
    pr = case.primal(HybridTotal(emu, c, conn, gc.NET.buffer(), et))
    assert pr.newton_iters == ref.newton_iters
    assert abs(pr.qoi() - J) <= 1e-10 * abs(J)
    gc.check_history(case, pr)
    assert np.abs(g[3:]).max() > 0.0
    print("%s worst ratio %.2e" % (case.name, march_groups(case, pr, n_tail=len(gc.NET.theta))))
