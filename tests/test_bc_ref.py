"""The restatements of bc_ref.py by themselves, against closed forms, and the float64 host restatement (fe_driver.apply_tbcs)
inside the entrywise bound of bc_ref around the long double one: the bound that the device tests use is attainable by a
plain float64 evaluation of the same formulas.  No GPU."""
import numpy as np
import pytest

import bc_ref as R
from fe_driver import Tbc, apply_tbcs

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def rectangle(a, b, z=0.3):
    """one quad4 face [0, a] x [0, b] in the plane z, local order (0,0) (a,0) (a,b) (0,b)"""
    return np.array([[0.0, 0.0, z], [a, 0.0, z], [a, b, z], [0.0, b, z]]), np.array([[0, 1, 2, 3]])


def test_constant_traction_on_a_flat_rectangle():
    a, b = 1.7, 0.6
    c, f = rectangle(a, b)
    T = np.array([0.3, -2.0, 1.1])
    val, S, cnt, kt = R.traction_ref(c, f, np.tile(T, (1, 4, 1)))
    want = -(T.astype(LD) * LD(a) * LD(b) / 4)
    assert np.abs(val.reshape(4, 3) - want).max() < 8 * EPS_LD * np.abs(want).max()
    assert np.all(cnt == 4) and np.abs(S.reshape(4, 3) - np.abs(want)).max() < 8 * EPS_LD * np.abs(want).max()


def test_linear_traction_is_integrated_exactly_by_the_2x2_rule():
    # T = (alpha x, 0, 0) on [0, a] x [0, b]: int N_a alpha x dA = alpha a^2 b / 12 on the x = 0 nodes, / 6 on the x = a nodes
    a, b, alpha = 1.3, 0.7, 2.5
    c, f = rectangle(a, b)
    pts = R.face_points_ref(c, f)[0]
    T = np.zeros((1, 4, 3), dtype=LD)
    T[..., 0] = LD(alpha) * pts[..., 0]
    val = R.traction_ref(c, f, T)[0].reshape(4, 3)
    lo, hi = LD(alpha) * LD(a) ** 2 * LD(b) / 12, LD(alpha) * LD(a) ** 2 * LD(b) / 6
    assert np.abs(val[:, 0] + np.array([lo, hi, hi, lo])).max() < 16 * EPS_LD * hi
    assert np.all(val[:, 1:] == 0)


def test_partition_of_unity_on_warped_faces():
    # sum_a b[n_a] = -sum_q T_q dv_q, with dv from the tangents formed here from the bilinear map's derivatives
    et, c, conn, faces = R.traction_cases()["warped_brick"]
    pts = R.face_points_ref(c, faces)[0]
    T = R.smooth_traction(np.asarray(pts, dtype=np.float64))
    g = 1 / np.sqrt(LD(3))
    for f in (0, 5, len(faces) - 1):
        X = c[faces[f]].astype(LD)
        assert abs(np.linalg.det(np.array([X[1] - X[0], X[3] - X[0], X[2] - X[0]], dtype=np.float64))) > 1e-6  # warped
        val = R.traction_ref(c, faces[f:f + 1], T[f:f + 1])[0].reshape(-1, 3)
        want = np.zeros(3, dtype=LD)
        for q in range(4):
            xi, eta = (g if q & 1 else -g), (g if q & 2 else -g)
            tx = ((1 - eta) * (X[1] - X[0]) + (1 + eta) * (X[2] - X[3])) / 4
            ty = ((1 - xi) * (X[3] - X[0]) + (1 + xi) * (X[2] - X[1])) / 4
            cr = np.array([tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]])
            want -= T[f, q].astype(LD) * np.sqrt((cr * cr).sum())
        assert np.abs(val.sum(axis=0) - want).max() < 64 * EPS_LD * np.abs(want).max()


def test_face_points_follow_the_bilinear_map():
    rng = np.random.default_rng(3)
    c = rng.random((4, 3)) + np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    pts = R.face_points_ref(c, [[0, 1, 2, 3]])[0][0]
    g = 1 / np.sqrt(LD(3))
    X = c.astype(LD)
    for q, (xi, eta) in enumerate([(-g, -g), (g, -g), (-g, g), (g, g)]):  # bit 0 of q: xi, bit 1: eta
        want = ((1 - xi) * (1 - eta) * X[0] + (1 + xi) * (1 - eta) * X[1] + (1 + xi) * (1 + eta) * X[2] + (1 - xi) * (1 + eta) * X[3]) / 4
        assert np.abs(pts[q] - want).max() < 8 * EPS_LD * 2.0
    # tri3 and edge sides: centroid and midpoint
    assert np.abs(R.face_points_ref(c, [[0, 1, 2]])[0][0, 0] - (X[0] + X[1] + X[2]) / 3).max() < 8 * EPS_LD
    assert np.abs(R.face_points_ref(c, [[3, 1]])[0][0, 0] - (X[3] + X[1]) / 2).max() < 8 * EPS_LD


def test_dirichlet_ref_on_a_hand_made_system_with_overlapping_conditions():
    # 3 nodes, one equation each, one residual; dense 3 x 3 CSR
    rp = [[np.array([0, 3, 6, 9])]]
    ci = [[np.array([0, 1, 2, 0, 1, 2, 0, 1, 2])]]
    A = [[np.array([4.0, 1.0, 2.0, 3.0, 5.0, 7.0, 11.0, 13.0, 6.0])]]
    b = [np.array([100.0, 200.0, 300.0])]
    x = [np.array([0.5, 0.25, -1.0])]
    dbcs = [(0, 0, [0, 1], [1.0, 2.0]), (0, 0, [1, 2], [-3.0, 0.125])]  # node 1 is in both: the later value wins
    A1, b1 = R.dirichlet_ref(rp, ci, A, b, x, dbcs, False, neq=(1, 1))
    assert np.array_equal(A1[0][0], [4.0, 0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 6.0])
    assert np.array_equal(b1[0], [4.0 * (0.5 - 1.0), 5.0 * (0.25 + 3.0), 6.0 * (-1.0 - 0.125)])
    assert np.array_equal(A[0][0], [4.0, 1.0, 2.0, 3.0, 5.0, 7.0, 11.0, 13.0, 6.0])  # the input is left alone
    A2, b2 = R.dirichlet_ref(rp, ci, A, b, x, dbcs[:1], True, neq=(1, 1))
    assert np.array_equal(A2[0][0], [4.0, 0.0, 0.0, 0.0, 5.0, 0.0, 11.0, 13.0, 6.0]) and np.array_equal(b2[0], [0.0, 0.0, 300.0])


def test_spmv_ref_on_a_hand_made_system():
    rp = [[np.array([0, 2, 3])]]
    ci = [[np.array([0, 1, 1])]]
    y, S, n = R.spmv_ref(rp, ci, [[np.array([2.0, -3.0, 0.5])]], [np.array([1.5, 4.0])])
    assert np.array_equal(y[0], [-9.0, 2.0]) and np.array_equal(S[0], [15.0, 2.0]) and np.array_equal(n[0], [2, 1])


@pytest.mark.parametrize("name", ["warped_brick", "pinched_bricks", "tet_cube", "notch2d"])
def test_float64_apply_tbcs_lies_within_the_bound_of_the_long_double_restatement(name):
    # the meshes, sides and traction of the device tests: a plain float64 evaluation stays inside the bound that the
    # device is held to, with room (the bound is a worst case), and the bound itself stays far below the values
    et, c, conn, sides = R.traction_cases()[name]
    nd = 2 if et == 3 else 3
    fn = lambda x, y, z, t: tuple(R.smooth_traction(np.array([x, y, z])))

    class Sys:
        b = [np.zeros(len(c) * nd)]

    apply_tbcs(Sys, [Tbc(0, sides.tolist(), fn)], c, 0.0)
    T = R.smooth_traction(np.asarray(R.face_points_ref(c, sides, dtype=np.float64)[0]))
    val, S, cnt, kt = R.traction_ref(c, sides, T)
    bound = R.sum_bound(S, cnt, kt)
    touched = cnt > 0
    assert touched.any() and np.all(Sys.b[0][~touched] == 0.0)
    err = np.abs(Sys.b[0].astype(LD) - val)
    assert np.all(err <= bound)
    assert np.all(bound[touched] < 1e-12 * S[touched])  # k stays a few hundred: the bound resolves a relative 1e-12
    if et == 8:  # quad4: up to 16 terms at a node of the brick, and the conditioning of the tangents is counted
        assert cnt.max() <= 16 and kt.max() < 2000


def test_apply_tbcs_refuses_other_side_lengths():
    class Sys:
        b = [np.zeros(30)]

    with pytest.raises(ValueError):
        apply_tbcs(Sys, [Tbc(0, [[0, 1, 2, 3, 4]], lambda x, y, z, t: (0.0, 0.0, 0.0))], np.zeros((10, 3)), 0.0)
    assert np.all(Sys.b[0] == 0.0)
