"""The hex8 kernels on meshes with shuffled node ids, shuffled element order and rotated local node order (renumber_cases.py),
on the CPU: first the oracle against itself through the renumbering maps (this validates the maps and the reference before
anything is held against them), then the kernel source run by the lane emulator against the oracle built on the renumbered
mesh, at the suite's bar.  The no-GPU rehearsal of test_gpu_renumbered.py."""
import numpy as np
import pytest

import emul_lib as em
import node_rows_xlane_cases as xl
import oracle_lib as ol
import renumber_cases as rn
from parity_cases import (HJ2, HOSFORD, J2, LOCAL_LINE_SEARCH, check_adjoint_chain, check_forward, check_residual,
                          check_two_element_sets)

TOL = 1e-12
# (wave, staged, node) of emul_lib.Emul: slot, wave, wave staged, row-per-node, row-per-node in two parts
FORMS = {"slot": (False, False, False), "wave": (True, False, False), "wave_staged": (True, True, False),
         "node": (True, False, True), "node_two_parts": (True, True, True)}
MESHES = {"shuffled433": lambda: rn.shuffled433()[:2], "same_corner222_a0": lambda: rn.same_corner222(0)[:2],
          "same_corner222_a5": lambda: rn.same_corner222(5)[:2], "pinched_shuffled": lambda: rn.pinched_shuffled()[:2],
          "bar_windowed": lambda: rn.bar_windowed()[:2]}


def pair(mesh, model, params, form):
    c, conn = MESHES[mesh]()
    orc, dut = ol.Oracle(ol.HEX8, c, conn, model, params), em.Emul(ol.HEX8, c, conn, model, params)
    dut.wave, dut.staged, dut.node = FORMS[form]
    return orc, dut, c


def test_rotations_and_meshes():
    # the 24 rotations are derived, distinct and proper (asserted at import), every mesh builder asserts its own properties
    assert len(rn.HEX_ROTATIONS) == 24 and len({tuple(r) for r in rn.HEX_ROTATIONS}) == 24
    assert sorted(rn.HEX_ROTATIONS[:, 0]) == sorted(list(range(8)) * 3)  # each corner takes node 0's place three times
    for name, make in MESHES.items():
        c, conn = make()
        assert (rn.point_jacobians(c, conn) > 0).all() and rn.face_defects(c, conn).min() > 1e-3, name
    rn.shuffled433_two_sets()
    rn.notched_shuffled()
    # a mirrored element (an improper symmetry) is what the Jacobian check is there to catch
    c, conn = rn.brick433()
    assert (rn.point_jacobians(c, conn[:, [1, 0, 3, 2, 5, 4, 7, 6]]) < 0).all()
    assert rn.staged_plan(rn.bar_windowed()[1], 4)[1] >= 5
    # the maps and their inverses
    rec = rn.shuffled433()[2]
    rng = np.random.default_rng(1)
    x, v = rng.random((len(conn), 8, 7)), rng.random(3 * len(c))
    assert np.array_equal(rec.points_back(rec.points(x)), x) and np.array_equal(rec.back(rec.nodal(v, 3), 3), v)
    assert not np.array_equal(rec.points(x), x[rec.pe])


@pytest.mark.parametrize("rot", [None, 5, 17])
def test_oracle_is_equivariant(rot):
    # xi, b and the four blocks of a plastic forward step on the renumbered mesh equal the brick's through the maps
    c0, conn0 = rn.brick433()
    c, conn, rec = rn.shuffled433(rot)
    assert rot is None or not np.array_equal(rn.POINT_MAPS[rot], np.arange(8))
    o0, o1 = ol.Oracle(ol.HEX8, c0, conn0, "small_J2", J2), ol.Oracle(ol.HEX8, c, conn, "small_J2", J2)
    errs, (x0, x1) = rn.renumbered_pair_errors(rec, o0, o1, c0)
    print("oracle equivariance, rot = %s: %s" % (rot, {k: "%.1e" % v for k, v in errs.items()}))
    assert max(errs.values()) < TOL, errs
    # negative control: with the identity point map (elements reordered only) the states disagree -- the points differ
    xe = x0[rec.pe]
    wrong = float(np.abs(x1 - xe).max() / np.abs(xe).max())
    print("  with the identity point map: xi off by %.1e" % wrong)
    assert wrong > 1e-6


@pytest.mark.parametrize("model,params,form", [("small_J2", J2, f) for f in FORMS] +
                         [("hyper_J2", HJ2, f) for f in ("slot", "wave", "wave_staged")])
def test_emulated_kernels_on_shuffled433(model, params, form):
    orc, dut, c = pair("shuffled433", model, params, form)
    check_forward(orc, dut, c, model, 0.004, TOL)
    check_adjoint_chain(orc, dut, c, model, 0.004, TOL)


@pytest.mark.parametrize("form", ["slot", "wave"])
def test_emulated_residual_on_shuffled433(form):
    orc, dut, c = pair("shuffled433", "small_J2", J2, form)
    check_residual(orc, dut, c, 0.004, TOL)


@pytest.mark.parametrize("form", ["node", "node_two_parts", "wave", "wave_staged"])
@pytest.mark.parametrize("mesh", ["same_corner222_a0", "same_corner222_a5", "pinched_shuffled"])
def test_emulated_node_and_wave_kernels_where_local_indices_repeat(mesh, form):
    # the centre node is the SAME local node of all eight of its elements; sixteen elements at a node, two rounds of eight
    orc, dut, c = pair(mesh, "small_J2", J2, form)
    check_forward(orc, dut, c, "small_J2", 0.004, TOL)
    check_adjoint_chain(orc, dut, c, "small_J2", 0.004, TOL)


def test_emulated_staged_wave_kernel_on_bar_windowed():
    # chunks of the bandwidth (16 <= 20) through the ring of three, node rows summed as their last chunk completes
    orc, dut, c = pair("bar_windowed", "small_J2", J2, "wave_staged")
    check_forward(orc, dut, c, "small_J2", 0.004, TOL)
    assert em.lib().c8emu_last_nchunks() >= 5
    check_adjoint_chain(orc, dut, c, "small_J2", 0.004, TOL)


@pytest.mark.parametrize("form", ["slot", "wave", "wave_staged", "node"])
def test_emulated_two_element_sets_on_shuffled433(form):
    c, conn, es, _, _ = rn.shuffled433_two_sets()

    def factory(et, c, conn, model, params, **kw):
        dut = em.Emul(et, c, conn, model, params, **kw)
        dut.staged, dut.node = FORMS[form][1:]
        return dut

    check_two_element_sets(factory, "hex8", TOL, wave=FORMS[form][0], mesh=(ol.HEX8, c, conn, es))


def test_emulated_hosford_wave_kernel_on_shuffled433():
    # the Newton + line-search iteration in the 8-lanes-per-point layout
    c, conn = MESHES["shuffled433"]()
    orc, dut = ol.Oracle(ol.HEX8, c, conn, "small_hosford", HOSFORD), em.Emul(ol.HEX8, c, conn, "small_hosford", HOSFORD)
    orc.set_local_line_search(*LOCAL_LINE_SEARCH)
    dut.set_local_line_search(*LOCAL_LINE_SEARCH)
    dut.wave = True
    check_forward(orc, dut, c, "small_hosford", 0.004, TOL)
    check_adjoint_chain(orc, dut, c, "small_hosford", 0.004, TOL)


@pytest.mark.parametrize("name", rn.CHAIN_MESHES)
def test_emulated_second_plastic_step_node_against_oracle_and_wave(name):
    # the second plastic step of node_rows_chain_cases.py (a different non-zero previous state at every point): the
    # row-per-node kernel against the oracle and against the staged wave kernel, and assign mode over stale content
    c, conn, es, prm = xl.mesh(name)
    out = {}
    for kernel in ("node", "wave"):
        dut = em.Emul(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)
        dut.wave, dut.node, dut.staged = True, kernel == "node", kernel == "wave"
        ls, xi = xl.forward(dut, name)
        out[kernel] = (ls, xi, xl.adjoint(dut, name, xi))
        xl.check_against_oracle(name, *out[kernel], TOL)
    xl.check_against_wave(name, *out["node"], *out["wave"])

    def set_assign(on):
        dut.assign = on

    dut = em.Emul(ol.HEX8, c, conn, "small_J2", prm, elem_set=es)
    dut.wave = dut.node = True
    xl.check_assign_and_accumulate(name, dut, set_assign)
