"""Superconvergent patch recovery on the CPU: c8_spr_build_host of libc8.so (no device) and the functions of
calibr8_amd/csrc/c8_spr.hpp -- the source the device kernels compile -- built with g++ (tests/spr_host), against a set-based
restatement of the patch rules and numpy.linalg.lstsq (tests/spr_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import spr_cases as sc


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return sc.Harness(tmp_path_factory.mktemp("c8_spr_host"))


# ---- 1. patches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.GOOD)
def test_patch_lists_and_stage_counts_equal_the_restated_rules(harness, name):
    ref, stages, _ = sc.patches_ref(name)
    for tab in (sc.host_tables(name), harness.build(name)):
        assert sc.as_lists(tab) == ref
        assert np.array_equal(tab["stages"], stages)
        assert tab["patch_ptr"][0] == 0 and tab["patch_ptr"][-1] == len(tab["patch_elems"])


def test_what_the_table_meshes_exercise():
    """the facts of the issue's table, from the restated rules alone"""
    for name in ("brick1", "brick2", "brick3", "pinched_bricks"):
        assert sc.patches_ref(name)[1].max() == 0, name  # no expansion on hex8
    assert len(sc.patches_ref("pinched_bricks")[0][13]) * 8 == 128
    for name, too_few in (("tet2", 12), ("tet3", 18)):
        _, stages, reasons = sc.patches_ref(name)
        assert reasons.count("points") == too_few and reasons.count("rank") == 2 and stages.max() == 2, name
        assert all(stages[n] > 0 for n, r in enumerate(reasons) if r)
    for name in ("tri22", "tri33", "tri61"):
        assert 1 <= sc.patches_ref(name)[1].max() <= 2
    assert len(sc.patches_ref("fan")[0][0]) == 66


def test_rank_triggered_nodes_are_the_ends_of_a_cell_diagonal(harness):
    for name in ("tet2", "tet3"):
        et, coords, conn = sc.mesh(name)
        _, stages, reasons = sc.patches_ref(name)
        tab = sc.host_tables(name)
        rank_nodes = [n for n, r in enumerate(reasons) if r == "rank"]
        assert sorted(rank_nodes) == [0, len(coords) - 1]  # the two ends of the brick's 0-6 diagonal
        for n in rank_nodes:
            own = [e for e, row in enumerate(conn) if n in row]
            assert len(own) == 6 and tab["stages"][n] >= 1 and len(sc.as_lists(tab)[n]) > 6
            assert harness.patch_ratio(name, n, own) <= 1e-12  # six coplanar centroids


@pytest.mark.parametrize("name", sc.HOPELESS)
def test_hopeless_meshes_fail_and_name_a_node(harness, name):
    from calibr8_amd import C8Error, lib
    with pytest.raises(sc.HopeLost) as ref:
        sc.patches_ref(name)
    with pytest.raises(C8Error) as ei:
        sc.host_tables(name)
    assert ei.value.code == lib.C8_ERR_ARG and ei.value.node == ref.value.node
    assert "node %d" % ref.value.node in str(ei.value) and "all hope is lost" in str(ei.value)
    with pytest.raises(sc.HopeLost) as hi:
        harness.build(name)
    assert hi.value.node == ref.value.node


def test_build_host_arguments():
    import ctypes as C
    from calibr8_amd import lib
    L = lib.load_library()
    et, coords, conn = sc.mesh("tet2")
    ptr = np.zeros(len(coords) + 1, dtype=np.int64)
    a = (coords.ctypes.data_as(lib.dp), conn.ctypes.data_as(lib.i32p))
    # patch_elems == NULL: patch_ptr alone
    assert L.c8_spr_build_host(et, len(coords), len(conn), *a, ptr.ctypes.data_as(lib.i64p), None, 0, None, None, None, None) == lib.C8_OK
    assert ptr[-1] == len(sc.host_tables("tet2")["patch_elems"])
    small = np.zeros(int(ptr[-1]) - 1, dtype=np.int32)
    assert L.c8_spr_build_host(et, len(coords), len(conn), *a, ptr.ctypes.data_as(lib.i64p), small.ctypes.data_as(lib.i32p), len(small),
                               None, None, None, None) == lib.C8_ERR_ARG
    assert b"capacity" in L.c8_last_error()
    assert L.c8_spr_build_host(et, len(coords), len(conn), None, a[1], ptr.ctypes.data_as(lib.i64p), None, 0, None, None, None, None) == lib.C8_ERR_ARG
    assert L.c8_spr_build_host(5, len(coords), len(conn), *a, ptr.ctypes.data_as(lib.i64p), None, 0, None, None, None, None) == lib.C8_ERR_UNSUPPORTED
    bad = np.array(conn)
    bad[3, 1] = len(coords)
    assert L.c8_spr_build_host(et, len(coords), len(conn), a[0], bad.ctypes.data_as(lib.i32p), ptr.ctypes.data_as(lib.i64p), None, 0, None, None,
                               None, None) == lib.C8_ERR_ARG


# ---- 2. values against numpy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncomp", [1, 9])
@pytest.mark.parametrize("name", sc.GOOD)
def test_random_fields_against_lstsq(harness, name, ncomp):
    """|recovered - lstsq| <= 1e-12 max(1, (kappa_n / 10)^2) max_s |v_s| per node: the project's 1e-12 on the structured
    meshes (kappa <= 20 there, two numpy formulations differ by 1e-15 .. 8e-15), with the least-squares sensitivity to a
    large residual, kappa^2, on the jiggled tets (kappa up to 609).  kappa < 1e3 on every input, so the bar cannot hide a
    failure."""
    ref, _, _ = sc.patches_ref(name)
    field = sc.random_field(name, ncomp)
    nodal, kappa, vmax = sc.lstsq_ref(name, ref, field)
    assert kappa.max() < 1e3, (name, kappa.max())
    if name == "tet3_jiggled":
        assert kappa.max() > 100  # the case the kappa^2 factor is for
    got, _ = harness.apply(name, sc.host_tables(name), field)
    err = np.abs(got - nodal).max(axis=1)
    bar = 1e-12 * np.maximum(1.0, (kappa / 10.0) ** 2) * vmax
    print("%s ncomp %d: worst err/bar %.3e, kappa max %.1f" % (name, ncomp, (err / bar).max(), kappa.max()))
    assert np.isfinite(got).all() and (err <= bar).all(), (name, (err / bar).max())


# ---- 3. affine fields ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.AFFINE)
def test_affine_fields_are_reproduced_and_the_weights_are_consistent(harness, name):
    """1e-13 max |f| on jiggled hex8, tet4 (interior nodes moved) and tri3 and on the fan.  A weight is formed as
    w_s = g . terms(x_s): its rounding error is eps |g|_inf, and |g|_inf grows like cond^2 -- 1.5e4 on the nearly coplanar
    patches of tet3_jiggled (every node moved, cond 609), where the affine error measures 1.9e-12 of max |f| = eps |g|_inf.
    That mesh is held to the kappa-scaled bar below, the others to 1e-13."""
    et, coords, conn = sc.mesh(name)
    tab = sc.host_tables(name)
    pts = sc.sample_points(et, coords, conn)
    field = sc.affine(et, pts)
    exact = sc.affine(et, coords)
    fmax = np.abs(field).max()
    got, _, w = harness.apply(name, tab, field, weights=True)
    assert np.abs(got - exact).max() <= 1e-13 * fmax, np.abs(got - exact).max() / fmax
    # sum_s w_s = 1 and sum_s w_s (x_s - x_n) = 0 (lengths in units of the largest coordinate)
    np0, d = pts.shape[1], sc.dims(et)
    xmax = np.abs(coords).max()
    k = 0
    for n, patch in enumerate(sc.as_lists(tab)):
        ws = w[k:k + len(patch) * np0]
        k += len(ws)
        x = pts[patch].reshape(-1, d) - coords[n, :d]
        assert abs(ws.sum() - 1.0) <= 1e-13, (n, ws.sum() - 1.0)
        assert np.abs(ws @ x).max() <= 1e-13 * xmax, (n, np.abs(ws @ x).max())
    assert k == len(w)


def test_affine_field_on_the_nearly_coplanar_patches(harness):
    """tet3_jiggled: 1e-13 max(1, (kappa_n / 10)^2) max |f| per node (see above: eps |g|_inf, |g|_inf ~ kappa^2 / 25 there)"""
    name = "tet3_jiggled"
    et, coords, conn = sc.mesh(name)
    pts = sc.sample_points(et, coords, conn)
    field = sc.affine(et, pts)
    _, kappa, _ = sc.lstsq_ref(name, sc.patches_ref(name)[0], field)
    got, _ = harness.apply(name, sc.host_tables(name), field)
    err = np.abs(got - sc.affine(et, coords)).max(axis=1)
    bar = 1e-13 * np.maximum(1.0, (kappa / 10.0) ** 2) * np.abs(field).max()
    print("worst err / max|f| %.3e, err/bar %.3e" % (err.max() / np.abs(field).max(), (err / bar).max()))
    assert kappa.max() < 1e3 and (err <= bar).all()


# ---- 4. spr_fit on explicit point sets -----------------------------------------------------------------------------------
def test_fit_on_explicit_point_sets(harness):
    rng = np.random.default_rng(11)
    xn = np.array([0.3, -0.2, 0.1])
    tet = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) + 0.1
    r, g, h = harness.fit(tet, xn)
    assert r > 1e-3 and h == pytest.approx(np.abs(tet - xn).max(), rel=1e-15)
    A = np.concatenate([np.ones((4, 1)), (tet - xn) / h], axis=1)
    assert np.abs(g - np.linalg.inv(A.T @ A)[0]).max() < 1e-12 * np.abs(g).max()  # g = (A^T A)^-1 e_0 on a well-conditioned set
    t = rng.random((7, 1))
    collinear = xn + 0.2 + t * np.array([1.0, 2.0, -0.5])
    coplanar = xn + rng.random((9, 2)) @ np.array([[1.0, 0.3, 0.2], [-0.4, 1.0, 0.5]])
    for pts in (collinear, coplanar, tet[:3], tet[:1]):  # collinear, coplanar, too few
        r, g, _ = harness.fit(pts, xn)
        assert r <= 1e-12 and not g.any(), r
    # 2-D: a triangle has full rank, collinear points and two points do not
    tri = np.array([[0.0, 0], [1, 0], [0.2, 0.9]])
    assert harness.fit(tri, xn[:2])[0] > 1e-3
    assert harness.fit(xn[:2] + t * np.array([1.0, -3.0]), xn[:2])[0] <= 1e-12
    assert harness.fit(tri[:2], xn[:2])[0] <= 1e-12


@pytest.mark.parametrize("name", sc.GOOD)
def test_the_rank_threshold_sits_in_an_empty_band(harness, name):
    """min |R_kk| / sqrt(m) >= 1e-3 on every accepted patch, <= 1e-12 on every patch the rank test refused on the way"""
    tab = harness.build(name)
    print("%s: smallest accepted ratio %.3e" % (name, tab["ratio"].min()))
    assert tab["ratio"].min() >= 1e-3
    et, coords, conn = sc.mesh(name)
    _, _, reasons = sc.patches_ref(name)
    for n, r in enumerate(reasons):
        if r == "rank":
            own = [e for e, row in enumerate(conn) if n in row]
            assert harness.patch_ratio(name, n, own) <= 1e-12


# ---- 5. sanitizer run ----------------------------------------------------------------------------------------------------
def test_patch_builder_and_fit_under_address_and_undefined_sanitizers(tmp_path):
    """a stand-alone program (its own main) over the table's meshes, run as a plain process"""
    exe = str(tmp_path / "spr_host_main")
    src = os.path.join(sc.HERE, "spr_host", "spr_host_main.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-o", exe, src])
    files = []
    for name in sc.TABLE:
        files.append(str(tmp_path / (name + ".mesh")))
        sc.write_mesh(files[-1], name)
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(sc.TABLE)
    for name, line in zip(sc.TABLE, lines):
        words = line.split()
        if name in sc.HOPELESS:
            assert words[1] == "failed" and int(words[2]) == 0, line
        else:
            assert words[1] == "ok" and int(words[2]) == len(sc.host_tables(name)["patch_elems"]), line
