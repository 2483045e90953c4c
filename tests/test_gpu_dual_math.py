"""calibr8_amd/csrc/c8_math.hpp on the device, one operation at a time: the cases, references and bars of
tests/math_cases.py (see tests/test_dual_math_edges.py for the CPU side) through tests/math_device, a small harness of
its own that is no part of libc8.so.  What only exists on the device is held here: c8_rcp (v_rcp_f64 and two Newton
steps) to its claim of one ulp and to its documented NaN for arguments without a finite reciprocal, the device libm in
ulps, and the agreement of the device with the CPU emulator on every case whose branches cannot decide differently.

The harness is loaded once; the lane-to-case mapping is checked with launches of 1, 63, 64, 65 and 257 cases, then all
families go to the device in ONE launch of a few thousand lanes.

At an exactly repeated eigenvalue (the two delta = 0 cases of the eig family) the tangents of eig_spd_cos are not
defined; whether they are finite is printed, not asserted.  Observed on an MI355X: finite in both cases, as on the CPU."""
import numpy as np
import pytest

import math_cases as mc

pytestmark = pytest.mark.gpu

FAMILIES = mc.all_families()
NAMES = [f.name for f in FAMILIES]


@pytest.fixture(scope="module")
def device():
    """the lane mapping of the harness first, then every family in one launch: {name: (out, dout)}"""
    for n in (1, 63, 64, 65, 257):
        x, dx = np.zeros((n, mc.NIN)), np.zeros((n, mc.NIN))
        x[:, 0], x[:, 1], dx[:, 0] = np.arange(n) + 1.0, 3.0, np.arange(n) + 0.5
        ops = np.where(np.arange(n) % 2 == 0, mc.OP["MUL_DS"], mc.OP["ADD_DS"]).astype(np.int32)
        out, dout = mc.run_device(ops, x, dx)
        even = np.arange(n) % 2 == 0
        assert (out[:, 0] == np.where(even, 3.0 * x[:, 0], x[:, 0] + 3.0)).all(), n
        assert (dout[:, 0] == np.where(even, 3.0 * dx[:, 0], dx[:, 0])).all(), n
        assert (out[:, 1:] == 0).all() and (dout[:, 1:] == 0).all(), n
    arrs = [f.arrays() for f in FAMILIES]
    out, dout = mc.run_device(*[np.concatenate([a[k] for a in arrs]) for k in range(3)])
    res, at = {}, 0
    for f in FAMILIES:
        res[f.name] = (out[at:at + len(f)], dout[at:at + len(f)])
        at += len(f)
    return res


@pytest.mark.parametrize("name", NAMES)
def test_family_against_its_reference(device, name):
    fam = FAMILIES[NAMES.index(name)]
    out, dout = device[name]
    worst = fam.check(out, dout, "device")
    print(name, len(fam), "cases; largest error / bar:", {k: round(float(v), 3) for k, v in worst.items()})


def test_rcp_is_accurate_to_the_last_place(device):
    """the claim in the comment of c8_rcp, over the whole exponent range and the mantissas next to 1 and 2"""
    fam = FAMILIES[NAMES.index("div_range")]
    out, _ = device["div_range"]
    idx = [i for i, m in enumerate(fam.meta) if m["op"] == "RCP"]
    x = np.array([fam.x[i][0] for i in idx])
    u = mc.ulps(out[idx, 0], 1.0 / x)
    print("c8_rcp against the host's 1 / x over %d arguments: largest error %.3f ulp, %d of them not correctly rounded"
          % (len(idx), u.max(), int((u > 0).sum())))
    assert u.max() <= mc.RCP_ULPS


@pytest.mark.parametrize("name", [f.name for f in FAMILIES if not f.device_only])
def test_device_agrees_with_emulator(device, name):
    fam = FAMILIES[NAMES.index(name)]
    out, dout = device[name]
    eout, edout = mc.run_emul(*fam.arrays())
    fails = mc.agreement(fam, out, dout, eout, edout)
    skipped = [i for i, b in enumerate(fam.branch_free) if not b]
    print(name, "cases not compared beyond their eigenvalues (branches may decide differently):",
          [(i, fam.meta[i].get("label")) for i in skipped])
    assert len(skipped) <= 0.05 * len(fam)
    assert not fails, fails[:20]
