"""The CPU twin of test_gpu_node_rows_image.py::test_every_entry_meets_its_own_accumulator: the row-per-node kernel source
run lane by lane on the CPU.  The assembly in accumulate mode into a system prefilled with a different value in every
entry equals, bit for bit, the prefill plus the assembly in assign mode -- a sum stored to another entry than the one its
old value was fetched from would meet another prefilled value.  (Where phase C puts a block is checked against the
oracle by test_emul_parity.py: both sides here come from the same kernel.)"""
import numpy as np
import pytest

import emul_lib as em
import oracle_lib as ol
from meshes import brick, jiggle, notched_bar, pinched_bricks, prescribed_fields
from parity_cases import J2


def _mesh(name):
    if name == "one_element":
        return brick(1, 1, 1)[:2]
    if name == "brick222":
        c, conn, sets = brick(2, 2, 2)
        return jiggle(c, sets, 0.05), conn
    if name == "brick321":
        return brick(3, 2, 1)[:2]
    if name == "notched_bar":
        return notched_bar(10, 6, 3)[:2]
    return pinched_bricks()


def _blocks(ls):
    return [ls.A[i][j] for i in range(2) for j in range(2)] + [ls.b[0], ls.b[1]]


@pytest.mark.parametrize("adjoint", [False, True], ids=["K1", "K3"])
@pytest.mark.parametrize("name", ["one_element", "brick222", "brick321", "notched_bar", "pinched_bricks"])
def test_every_entry_meets_its_own_accumulator(name, adjoint):
    c, conn = _mesh(name)
    dut = em.Emul(ol.HEX8, c, conn, "small_J2", J2)
    dut.node = dut.wave = True
    u, p = prescribed_fields(c, 0.004, ramp=True, perturb=5e-2)
    z, zp = np.zeros_like(u), np.zeros_like(p)
    xi0, xi1 = dut.new_state(), dut.new_state()
    assert dut.forward_jacobian(u, p, z, zp, xi0, xi1, dut.new_linsys()) == 0
    rng = np.random.default_rng(11)
    g = 1e-3 * rng.standard_normal((dut.nelems, dut.npts, dut.nloc))
    f = 1e-3 * rng.standard_normal((dut.nelems, dut.npts, 4 * dut.nn))

    def call(ls):
        if adjoint:
            g_in = g.copy()
            assert dut.adjoint_jacobian(u, p, z, zp, xi0, xi1, g_in, f, ls) == 0
            return g_in
        xi = dut.new_state()
        assert dut.forward_jacobian(u, p, z, zp, xi0, xi, ls) == 0
        return xi

    R = dut.new_linsys()
    for a in _blocks(R):
        a[:] = -7.25e3
    dut.assign = True
    st_R = call(R)
    dut.assign = False
    ls, P = dut.new_linsys(), []
    for a in _blocks(ls):
        a[:] = 10.0 * (1.0 + rng.random(a.shape))
        P.append(a.copy())
    assert len(np.unique(np.concatenate(P))) == sum(len(a) for a in P)
    st = call(ls)
    for a, pre, r in zip(_blocks(ls), P, _blocks(R)):
        assert not (r == -7.25e3).any()  # every node of these meshes has elements: every entry is assigned
        assert np.array_equal(a, pre + r)
    assert np.array_equal(st, st_R)
    if not adjoint:
        assert np.array_equal(st, xi1)
