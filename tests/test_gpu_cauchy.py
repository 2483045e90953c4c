"""`-m gpu`: c8_eval_cauchy on the device.  The kernel compiles the same per-point function as the host harness of
test_cauchy_host.py (which checks it against the oracle), so the device is compared with that harness on identical inputs:
every row of the model table on its standard mesh, and the shapes at which the lane mapping (one lane per point, 256 per
block, the block's results passed through LDS) can go wrong."""
import ctypes as C

import numpy as np
import pytest

import cauchy_cases as cc
import oracle_lib as ol
import parity_cases as pc

pytestmark = pytest.mark.gpu
TOL = 1e-12  # of max |sigma|: the project's parity bar (device libm differs from glibc by ulps)


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return cc.build_harness(tmp_path_factory.mktemp("c8_cauchy_host"))


def device_cauchy(asm, state, out=None):
    import torch
    s = asm.cauchy(*[asm.dev(a) for a in state], out=out)
    torch.cuda.synchronize()
    return s.cpu().numpy()


def assembler(cs):
    from calibr8_amd import Assembler
    return Assembler(cs.et, cs.c, cs.conn, cs.model, cs.params, **cs.assembler_kw())


def assert_close(dev, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(dev - ref).max()
    assert np.isfinite(dev).all() and scale > 0 and err < TOL * scale, (what, err, scale)


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_device_matches_host_harness_on_every_model_row(harness, rid):
    cs = cc.case(rid)
    asm = assembler(cs)
    dev = device_cauchy(asm, cs.state)
    assert dev.shape == (len(cs.conn), asm.npts, 3, 3)
    assert_close(dev, cs.host(harness), rid)
    if asm.ndims == 2:
        assert np.all(dev[:, :, 2, :] == 0.0) and np.all(dev[:, :, :, 2] == 0.0)


def _shape_mesh(kind, n):
    from meshes import brick, jiggle, jiggle_2d, tri_mesh
    if kind == "hex8":
        c, conn, sets = brick(*n, 1.0 * n[0], 0.8 * n[1], 0.7 * n[2])
        return ol.HEX8, jiggle(c, sets, 0.04), conn
    if kind == "tet4":
        c, conn = cc.tet_mesh(2, 2, 3)  # 72 tets
        return (ol.TET4,) + cc.sub_mesh(c, conn, n)
    c, conn, sets = tri_mesh(6, 6, 1.0, 0.8)  # 72 triangles
    return (ol.TRI3,) + cc.sub_mesh(jiggle_2d(c, sets, 0.02), conn, n)


# the smallest shapes at which the lane mapping can go wrong: one element; hex8 with 9 elements (72 lanes: a ragged second
# wavefront) and with 33 and 36 (264 and 288 lanes: a ragged second block, an element count that is no multiple of 32); one
# lane per element (tet4, both tri3 classes) with 1 and 65 elements (a second wavefront of one lane)
SHAPES = [("hex8", (1, 1, 1), "small_J2", pc.J2), ("hex8", (3, 3, 1), "small_J2", pc.J2), ("hex8", (11, 3, 1), "hyper_J2", pc.HJ2),
          ("hex8", (4, 3, 3), "hypo_barlat", pc.BARLAT), ("tet4", 1, "hyper_J2", pc.HJ2), ("tet4", 65, "hyper_J2", pc.HJ2),
          ("tri3", 1, "small_J2", pc.J2), ("tri3", 65, "hypo_hill_plane_strain", pc.HILL_PS),
          ("tri3", 1, "hyper_J2_plane_stress", pc.HJ2_PSS), ("tri3", 65, "hyper_J2_plane_stress", pc.HJ2_PSS)]


@pytest.mark.parametrize("kind,n,model,params", SHAPES, ids=["%s-%s-%s" % (k, str(n).replace(" ", ""), m) for k, n, m, _ in SHAPES])
def test_lane_mapping_shapes(harness, kind, n, model, params):
    from calibr8_amd import Assembler
    et, c, conn = _shape_mesh(kind, n)
    asm = Assembler(et, c, conn, model, params)
    assert asm.nelems == (n if isinstance(n, int) else n[0] * n[1] * n[2])
    state = cc.synthetic_state(asm.new_state().cpu().numpy(), c, asm.ndims, asm.nres, seed=asm.nelems)
    dev = device_cauchy(asm, state)
    ref = cc.host_cauchy(harness, et, c, conn, model, params, *state)
    assert_close(dev, ref, (kind, n, model))
    assert len(np.unique(np.round(ref[:, :, 0, 0] / np.abs(ref).max(), 9))) == ref.shape[0] * ref.shape[1]  # no two points alike


def test_two_element_sets(harness):
    from calibr8_amd import Assembler
    et, c, conn = pc.mesh_of("hex8")
    es = (np.random.default_rng(21).random(len(conn)) < 0.4).astype(np.int32)
    params = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]
    asm = Assembler(et, c, conn, "small_J2", params, elem_set=es)
    state = cc.synthetic_state(asm.new_state().cpu().numpy(), c, 3, 2, seed=5)
    ref = cc.host_cauchy(harness, et, c, conn, "small_J2", params, *state, elem_set=es)
    assert_close(device_cauchy(asm, state), ref, "two sets")
    one = cc.host_cauchy(harness, et, c, conn, "small_J2", params[:1], *state)
    assert np.array_equal(one[es == 0], ref[es == 0]) and np.abs(one[es == 1] - ref[es == 1]).max() > 0.05 * np.abs(ref).max()


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-hex8", "hyper_J2_plane_stress-tri3"])
def test_weak_form_identity_on_the_device(rid):
    """Assembler.cauchy integrated against grad N (this test's quadrature, from the oracle's kit) is b[0] of
    Assembler.global_residual at the same state: a small-strain, a finite-deformation and a plane-stress model.  The bar is
    that of the host test: 1e-12 of the largest per-entry sum of the absolute values of the terms."""
    import torch
    cs = cc.case(rid)
    asm = assembler(cs)
    dstate = [asm.dev(a) for a in cs.state]
    sigma = asm.cauchy(*dstate).cpu().numpy()
    ls = asm.new_linsys()
    assert asm.global_residual(*dstate, ls) == 0
    torch.cuda.synchronize()
    nd = asm.ndims
    R, scale = cc.weak_form(sigma, cs, nd)
    err = np.abs(R - ls.b[0].cpu().numpy().reshape(-1, nd)).max()
    print("%s: |R - R_device| %.3e, scale %.3e" % (rid, err, scale))
    assert err < 1e-12 * scale, (rid, err, scale)


def test_out_is_overwritten_and_its_bounds_are_kept():
    import torch
    cs = cc.case("small_J2-hex8")
    asm = assembler(cs)
    dstate = [asm.dev(a) for a in cs.state]
    n = asm.nelems * asm.npts * 9
    ref = asm.cauchy(*dstate)
    # a canary-filled buffer one point longer than needed: the field is overwritten (not added to, also by a second call),
    # the tail stays
    buf = torch.full((n + 9,), -7.25, dtype=torch.float64, device=asm.device)
    out = buf[:n].view(asm.nelems, asm.npts, 3, 3)
    for _ in range(2):
        assert asm.cauchy(*dstate, out=out).data_ptr() == buf.data_ptr()
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and bool((buf[n:] == -7.25).all())
    # the same from an address that is 8-byte but not 16-byte aligned (the kernel's narrow store path), canaries on both sides
    buf = torch.full((n + 10,), -7.25, dtype=torch.float64, device=asm.device)
    out = buf[1:n + 1].view(asm.nelems, asm.npts, 3, 3)
    assert out.data_ptr() % 16 == 8
    asm.cauchy(*dstate, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and float(buf[0]) == -7.25 and bool((buf[n + 1:] == -7.25).all())
    # two calls give the same bytes
    assert torch.equal(asm.cauchy(*dstate), ref)


def test_primal_driver_stress_history():
    import torch
    from calibr8_amd import Assembler, PrimalDriver
    from meshes import brick, jiggle
    c, conn, sets = brick(3, 4, 3, 1.0, 1.5, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero),
            (0, 1, sets["ymax"], lambda x, y, z, t: 0.003 * t), (0, 0, sets["ymax"], zero)]
    asm = Assembler(8, c, conn, "small_J2", pc.J2)
    pr = PrimalDriver(asm, spec, max_iters=15, abs_tol=1e-12, rel_tol=1e-12).solve(2)
    s0 = pr.cauchy(0)
    assert s0.shape == (asm.nelems, asm.npts, 3, 3) and s0.is_cuda and not bool(s0.any())
    for step in (1, 2):
        s = pr.cauchy(step)
        direct = asm.cauchy(pr.u[step], pr.p[step], pr.u[step - 1], pr.p[step - 1], pr.xi[step - 1], pr.xi[step])
        torch.cuda.synchronize()
        assert torch.equal(s, direct) and float(s.abs().max()) > 0
    assert not torch.equal(pr.cauchy(1), pr.cauchy(2))
    assert (pr.xi[2][:, :, 6] > 0).any()  # the run reached the plastic range
    with pytest.raises(IndexError):
        pr.cauchy(3)


def test_null_arguments_are_refused():
    from calibr8_amd import lib
    cs = cc.case("small_J2-hex8")
    asm = assembler(cs)
    L = asm.L
    dstate = [asm.dev(a) for a in cs.state]
    out = asm.cauchy(*dstate)
    good = asm._state(*dstate)
    assert L.c8_eval_cauchy(asm.h, C.byref(good), C.c_void_p(out.data_ptr())) == lib.C8_OK
    assert L.c8_eval_cauchy(None, C.byref(good), C.c_void_p(out.data_ptr())) == lib.C8_ERR_ARG
    assert L.c8_eval_cauchy(asm.h, None, C.c_void_p(out.data_ptr())) == lib.C8_ERR_ARG
    assert L.c8_eval_cauchy(asm.h, C.byref(good), None) == lib.C8_ERR_ARG
    assert b"c8_eval_cauchy" in L.c8_last_error()

    def broken(field, k=None):
        s = asm._state(*dstate)
        if k is None:
            setattr(s, field, None)
        else:
            getattr(s, field)[k] = None
        return s

    for s in (broken("xi"), broken("xi_prev"), broken("x", 0), broken("x", 1), broken("x_prev", 0), broken("x_prev", 1)):
        assert L.c8_eval_cauchy(asm.h, C.byref(s), C.c_void_p(out.data_ptr())) == lib.C8_ERR_ARG
        assert b"c8_eval_cauchy: null" in L.c8_last_error()


def test_plane_stress_ignores_the_pressure_entries_and_the_hybrid_model_needs_its_network():
    from calibr8_amd import Assembler, lib
    cs = cc.case("hyper_J2_plane_stress-tri3")
    asm = assembler(cs)
    dstate = [asm.dev(a) for a in cs.state]
    ref = asm.cauchy(*dstate)
    s = asm._state(*dstate)
    s.x[1], s.x_prev[1] = None, None  # one residual: x[1] and x_prev[1] are not read
    out = ref.clone().zero_()
    assert asm.L.c8_eval_cauchy(asm.h, C.byref(s), C.c_void_p(out.data_ptr())) == lib.C8_OK
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy())
    hyb = cc.case(cc.HYBRID + "-tri3")
    bare = Assembler(hyb.et, hyb.c, hyb.conn, hyb.model, hyb.params)  # no embedded model set
    hs = [bare.dev(a) for a in hyb.state]
    with pytest.raises(lib.C8Error) as ei:
        bare.cauchy(*hs)
    assert ei.value.code == lib.C8_ERR_ARG and "embedded network" in str(ei.value)
