"""calibr8_amd/csrc/c8_math.hpp at its edges, one operation at a time, against references that do not restate it
(tests/math_cases.py): the whole exponent range for the divisions, the scalar functions at the ends of their domains,
ill-conditioned and reflected tensors, eig_spd_cos on diagonal, volumetric, nearly and exactly repeated spectra, and
polar_rotation from pure rotations to kappa(U) = 1e3.  Runs the header on the CPU through the emulator's c8emu_math_op;
tests/test_gpu_dual_math.py runs the same cases on the device.  No GPU."""
import numpy as np
import pytest

import math_cases as mc

FAMILIES = {f.name: f for f in mc.all_families() if not f.device_only}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_against_its_reference(name):
    fam = FAMILIES[name]
    out, dout = mc.run_emul(*fam.arrays())
    worst = fam.check(out, dout, "cpu")
    print(name, len(fam), "cases; largest error / bar:", {k: round(float(v), 3) for k, v in worst.items()})


def test_unknown_operation_is_refused():
    with pytest.raises(AssertionError):
        mc.run_emul(np.array([99], dtype=np.int32), np.zeros((1, mc.NIN)), np.zeros((1, mc.NIN)))


def test_straddling_cases_stay_below_five_percent():
    for fam in mc.all_families():
        n = sum(1 for b in fam.branch_free if not b)
        assert n <= 0.05 * len(fam), (fam.name, n, len(fam))


def test_oracle_meets_the_bars_it_sets():
    """The constants of the eig_spd_cos and polar_rotation bars are 8 x what the oracle's own routines need; the figures
    written beside them are this measurement."""
    w = mc.oracle_constants()
    print("oracle error / (eps model):", {k: round(v, 2) for k, v in sorted(w.items())})
    for k, v in w.items():
        assert v <= getattr(mc, k) / 8.0 * 1.5, (k, v)  # 1.5: another libm or LAPACK under the same oracle


def test_reference_needs_no_more_ulps_than_the_device_bar_assumes():
    w = mc.reference_ulps()
    print("numpy float64 against longdouble, ulps:", {k: round(v, 2) for k, v in sorted(w.items())})
    for k, v in w.items():
        assert v <= mc.REF_ULPS[k], (k, v)
