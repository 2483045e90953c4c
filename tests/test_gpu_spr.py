"""`-m gpu`: superconvergent patch recovery on the device (c8_spr_recover, c8_interpolate_to_points, c8_spr_table) against the
host set-up c8_spr_build_host and the sequential spr_apply_host of calibr8_amd/csrc/c8_spr.hpp (tests/spr_host), which
test_spr_host.py checks against numpy.  Meshes and references: tests/spr_cases.py."""
import ctypes as C

import numpy as np
import pytest

import spr_cases as sc

pytestmark = pytest.mark.gpu
J2 = [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0]  # small_J2 runs on all three element types; the recovery reads the mesh alone
# the fan has 64 triangles round its centre here, not the 66 of the host tests: c8_create refuses a mesh with more than 64
# elements round a node (element colours).  64 samples are still eight trips of the 8-lane group.
TABLE_MESHES = ("brick1", "brick3", "pinched_bricks", "tet2", "tet3", "tet3_jiggled", "tri22", "tri61", "fan64")
# ... and node counts on both sides of a launch block: hex8, 16 nodes per block: 8, 18 = 16 + 2, 53 = 3 x 16 + 5, 64 = 4 x 16;
# tet4 and tri3, 32 per block: 27, 36 = 32 + 4, 64 = 2 x 32; 9, 14, 32, 33 = 32 + 1, 129 = 4 x 32 + 1
RECOVER_MESHES = TABLE_MESHES + ("brick221", "tet223", "tri73", "tri102")


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return sc.Harness(tmp_path_factory.mktemp("c8_spr_host"))


_ASM = {}


def assembler(name):
    from calibr8_amd import Assembler
    if name not in _ASM:
        et, c, conn = sc.mesh(name)
        _ASM[name] = Assembler(et, c, conn, "small_J2", J2)
    return _ASM[name]


# ---- 1. device tables against the host set-up -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE_MESHES)
def test_device_tables_equal_the_host_setup(name):
    """patch lists and stage counts identical; g to 1e-12 max(1, (kappa_n / 10)^2) |g|_inf per node (the device contracts
    multiply-adds, the host build does not)"""
    dev, host = assembler(name).spr_patches(), sc.host_tables(name)
    assert np.array_equal(dev["patch_ptr"], host["patch_ptr"]) and np.array_equal(dev["patch_elems"], host["patch_elems"])
    assert np.array_equal(dev["stages"], host["stages"])
    et, coords, conn = sc.mesh(name)
    _, kappa, _ = sc.lstsq_ref(name, sc.as_lists(host), np.zeros((len(conn), sc.shape_values(et).shape[0], 1)))
    assert kappa.max() < 1e3
    gmax = np.abs(host["g"]).max(axis=1)
    err = np.abs(dev["g"] - host["g"]).max(axis=1)
    bar = 1e-12 * np.maximum(1.0, (kappa / 10.0) ** 2) * gmax
    print("%s: g worst err/bar %.3e, h rel %.3e, flagged %d" % (name, (err / bar).max(), np.abs(dev["h"] / host["h"] - 1).max(), dev["setup"][3]))
    assert (err <= bar).all() and np.abs(dev["h"] / host["h"] - 1).max() < 1e-14
    assert dev["setup"][3] == np.count_nonzero(host["stages"])  # the device fit flags exactly the nodes that need expansion
    if et == sc.HEX8:
        assert dev["setup"][3] == 0


# ---- 2. c8_spr_recover against spr_apply_host ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", RECOVER_MESHES)
def test_recover_against_the_sequential_host_sum(harness, name):
    """per entry 1e-12 sum_s |w_s v_s|: the device and the host form the same weights from the same g and h (the device's
    tables) and differ in the order of the sum, m eps = 1.4e-14 of that scale for m = 128, and in contracted multiply-adds,
    eps |g|_inf per weight (|g|_inf <= 1.5e4 on these meshes; sum |w_s| >= 1)"""
    import torch
    asm = assembler(name)
    tab = asm.spr_patches()
    for ncomp in (1, 2, 9, 16):
        field = sc.random_field(name, ncomp)
        ref, mag = harness.apply(name, tab, field)
        d_field = asm.dev(field)
        keep = d_field.clone()
        n = asm.nnodes * ncomp
        buf = torch.full((n + 3,), -7.25, dtype=torch.float64, device=asm.device)
        out = buf[1:n + 1].view(asm.nnodes, ncomp)  # 8-byte but not 16-byte aligned, canaries on both sides
        assert out.data_ptr() % 16 == 8
        assert asm.spr_recover(d_field, out=out).data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        err = np.abs(got - ref)
        assert np.isfinite(got).all() and (err <= 1e-12 * mag).all(), (name, ncomp, (err / mag).max())
        assert float(buf[0]) == -7.25 and bool((buf[n + 1:] == -7.25).all())
        assert torch.equal(d_field, keep)  # the input is not written
        again = asm.spr_recover(d_field)  # a fresh, aligned output: the same bytes
        torch.cuda.synchronize()
        assert torch.equal(again, out)


def test_trailing_dimensions_are_the_components():
    import torch
    asm = assembler("brick3")
    f = asm.dev(sc.random_field("brick3", 9)).view(asm.nelems, asm.npts, 3, 3)
    out = asm.spr_recover(f)
    assert tuple(out.shape) == (asm.nnodes, 3, 3)
    assert torch.equal(out.view(asm.nnodes, 9), asm.spr_recover(f.view(asm.nelems, asm.npts, 9)))
    scalar = asm.spr_recover(f[:, :, 0, 0].contiguous())
    assert tuple(scalar.shape) == (asm.nnodes,)


@pytest.mark.parametrize("name", ["pinched_bricks", "tet3", "fan64"])
def test_async_mode_and_a_caller_owned_stream(name):
    import torch
    asm = assembler(name)
    field = asm.dev(sc.random_field(name, 9))
    ref = asm.spr_recover(field)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=asm.device)
    try:
        with torch.cuda.stream(stream):
            asm.use_current_stream()
            asm.set_async(1)
            scaled = field * 2.0  # produced on the caller's stream: the recovery must be ordered after it
            out = asm.spr_recover(scaled)
            back = asm.interpolate_to_points(out)
        stream.synchronize()
        assert asm.status() == 0
        assert torch.equal(out, ref * 2.0)  # w (2 v) summed in the same order is twice the sum, exactly
        assert tuple(back.shape) == tuple(field.shape)
    finally:
        asm.set_async(0)
        asm.use_current_stream()


# ---- 3. affine reproduction on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["brick3_jiggled", "tet3_interior", "tri33_jiggled"])
def test_spr_smooth_returns_an_affine_nodal_field(name):
    import torch
    from calibr8_amd.error import spr_smooth
    asm = assembler(name)
    et, coords, _ = sc.mesh(name)
    nodal = sc.affine(et, coords)
    got = spr_smooth(asm, asm.dev(nodal))
    torch.cuda.synchronize()
    err = np.abs(got.cpu().numpy() - nodal).max()
    print("%s: affine error %.3e of max |f|" % (name, err / np.abs(nodal).max()))
    assert err <= 1e-13 * np.abs(nodal).max()


# ---- 4. interpolation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["brick3_jiggled", "brick221", "tet223", "tri102"])
def test_interpolate_to_points_against_numpy_shape_values(name):
    import torch
    asm = assembler(name)
    et, coords, conn = sc.mesh(name)
    N = sc.shape_values(et)
    for ncomp in (1, 7, 16):
        nodal = np.random.default_rng(ncomp).standard_normal((len(coords), ncomp))
        ref = np.einsum("pn,enc->epc", N, nodal[conn])
        n = ref.size
        buf = torch.full((n + 3,), -7.25, dtype=torch.float64, device=asm.device)
        out = buf[1:n + 1].view(*ref.shape)
        asm.interpolate_to_points(asm.dev(nodal), out=out)
        torch.cuda.synchronize()
        assert np.abs(out.cpu().numpy() - ref).max() <= 1e-14 * np.abs(nodal).max()
        assert float(buf[0]) == -7.25 and bool((buf[n + 1:] == -7.25).all())


# ---- 5. driver-level recovery ------------------------------------------------------------------------------------------
def test_primal_driver_nodal_fields():
    import torch
    import error_cases as ec
    import parity_cases as pc
    from calibr8_amd import Assembler, PrimalDriver
    c, conn, spec = ec.mfe_case()
    asm = Assembler(8, c, conn, "small_J2", pc.J2)
    pr = PrimalDriver(asm, spec, max_iters=25, abs_tol=ec.MFE_TOL, rel_tol=ec.MFE_TOL).solve(2)
    s0 = pr.nodal_cauchy(0)
    assert tuple(s0.shape) == (asm.nnodes, 3, 3) and s0.is_cuda and not bool(s0.any())
    for step in (1, 2):
        s, x = pr.nodal_cauchy(step), pr.nodal_local(step)
        torch.cuda.synchronize()
        assert tuple(s.shape) == (asm.nnodes, 3, 3) and tuple(x.shape) == (asm.nnodes, asm.nloc)
        assert torch.equal(s, asm.spr_recover(pr.cauchy(step))) and torch.equal(x, asm.spr_recover(pr.xi[step]))
        assert float(s.abs().max()) > 0
    assert torch.equal(pr.nodal_local(0), asm.spr_recover(pr.xi[0]))
    assert (pr.xi[2][:, :, 6] > 0).any() and float(pr.nodal_local(2)[:, 6].max()) > 0  # the run reached the plastic range
    for fn in (pr.nodal_cauchy, pr.nodal_local):
        with pytest.raises(IndexError):
            fn(3)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    from calibr8_amd import lib
    asm = assembler("brick1")
    L = asm.L
    f, out = asm.dev(sc.random_field("brick1", 16)), asm.dev(np.zeros((asm.nnodes, 16)))
    pf, po = C.c_void_p(f.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.c8_spr_recover(asm.h, 16, pf, po) == lib.C8_OK
    for fn, name in ((L.c8_spr_recover, b"c8_spr_recover"), (L.c8_interpolate_to_points, b"c8_interpolate_to_points")):
        a, b = (pf, po) if fn is L.c8_spr_recover else (po, pf)
        for ncomp in (0, 17, -1):
            assert fn(asm.h, ncomp, a, b) == lib.C8_ERR_ARG
            assert name in L.c8_last_error() and b"ncomp" in L.c8_last_error()
        assert fn(None, 1, a, b) == lib.C8_ERR_ARG
        assert fn(asm.h, 1, None, b) == lib.C8_ERR_ARG
        assert fn(asm.h, 1, a, None) == lib.C8_ERR_ARG
        assert name + b": null" in L.c8_last_error()
    n, data = C.c_int64(), C.c_void_p()
    assert L.c8_spr_table(None, 0, C.byref(n), C.byref(data)) == lib.C8_ERR_ARG
    assert L.c8_spr_table(asm.h, 6, C.byref(n), C.byref(data)) == lib.C8_ERR_ARG
    assert L.c8_spr_table(asm.h, 0, None, C.byref(data)) == lib.C8_ERR_ARG
    assert L.c8_spr_table(asm.h, 0, C.byref(n), C.byref(data)) == lib.C8_OK and n.value == asm.nnodes + 1


def test_hope_lost_names_the_node():
    from calibr8_amd import Assembler, C8Error, lib
    et, c, conn = sc.mesh("tet1")
    asm = Assembler(et, c, conn, "small_J2", J2)
    with pytest.raises(sc.HopeLost) as ref:
        sc.patches_ref("tet1")
    for call in (lambda: asm.spr_recover(asm.dev(sc.random_field("tet1", 2))), asm.spr_patches):
        with pytest.raises(C8Error) as ei:
            call()
        assert ei.value.code == lib.C8_ERR_ARG and "node %d" % ref.value.node in str(ei.value) and "all hope is lost" in str(ei.value)
    # the interpolation needs no patches
    assert tuple(asm.interpolate_to_points(asm.dev(np.ones((asm.nnodes, 2)))).shape) == (asm.nelems, 1, 2)


def test_a_context_with_a_halo_attached_is_refused():
    from calibr8_amd import Assembler, C8Error, lib
    import calibr8_amd.distributed as D
    et, c, conn = sc.mesh("brick2")
    part = D.part_from_global(c, conn, np.zeros(len(conn), dtype=np.int32), 0, 1)
    plan = D.HaloPlan(part, None)
    asm = Assembler(et, plan.coords, part.conn, "small_J2", J2)
    field = asm.dev(np.ones((asm.nelems, asm.npts, 1)))
    before = asm.spr_recover(field)  # fine without a halo; the tables exist from here on
    halo = D.Halo(plan, asm.rowptr[1][1], asm.colidx[1][1], asm, D.Comm.host(None, 0, 1))
    for call in (lambda: asm.spr_recover(field), asm.spr_patches):
        with pytest.raises(C8Error) as ei:
            call()
        assert ei.value.code == lib.C8_ERR_UNSUPPORTED and "halo" in str(ei.value)
    assert float((before - 1.0).abs().max()) < 1e-13  # a constant field is reproduced
    assert halo is not None
