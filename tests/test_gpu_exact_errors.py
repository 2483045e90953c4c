"""`-m gpu`: c8_eval_exact_errors and c8_eval_linearization_errors on the device and calibr8_amd.model_form_error_verify.
The kernel compiles the same per-point function as the host harness of test_exact_host.py (which checks it against the oracle
and against the harness of c8_eval_error_contributions), so the device is compared with that harness on identical inputs:
every row of the model table on its standard mesh, and the element counts at which the lane mapping (that of
c8_eval_error_contributions: 256 lanes per block, whole elements per block, values handed over through LDS) can go wrong."""
import ctypes as C

import numpy as np
import pytest

import cauchy_cases as cc
import error_cases as ec
import exact_cases as xc
import oracle_lib as ol
import parity_cases as pc

pytestmark = pytest.mark.gpu
TOL = 1e-12  # of the summed magnitudes of the per-point terms: the project's parity bar (device libm differs from glibc by ulps)


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return xc.build_harness(tmp_path_factory.mktemp("c8_exact_host"))


def assembler(cs):
    from calibr8_amd import Assembler
    return Assembler(cs.et, cs.c, cs.conn, cs.model, cs.params, **cs.assembler_kw())


def device_exact(asm, state, fine, adj, lin=False, E_R=None, E_C=None):
    import torch
    call = asm.linearization_errors if lin else asm.exact_errors
    r, c = call([asm.dev(a) for a in state], [asm.dev(a) for a in fine], *[asm.dev(a) for a in adj], E_R=E_R, E_C=E_C)
    torch.cuda.synchronize()
    return r.cpu().numpy(), c.cpu().numpy()


def assert_close(dev, ref, what, state, fine, phi):
    """device (E_R, E_C) against the harness's (E_R, E_C, abs_R, abs_C), element by element, at TOL of the summed magnitudes
    of the terms.  E_C: plus the operand term that assert_close of test_gpu_error.py adds, for the same reason -- C_j and its
    tangent are differences of numbers of the size of the local state and of its difference to the fine one (dC_j = dxi_j -
    dxi_prev_j - ...), which cannot be formed more exactly than that: |phi_j| (|xi_j| + |xi_prev_j| + |dxi_j| + |dxi_prev_j|)."""
    ops = np.abs(state[5]) + np.abs(state[4]) + np.abs(fine[5] - state[5]) + np.abs(fine[4] - state[4])
    operands = (np.abs(phi) * ops).sum(axis=(1, 2))
    worst = [0.0, 0.0]
    for k, name in ((0, "E_R"), (1, "E_C")):
        scale = ref[2 + k] + (operands if k == 1 else 0.0)
        assert np.isfinite(dev[k]).all() and np.isfinite(ref[k]).all(), (what, name)
        err = np.abs(dev[k] - ref[k])
        worst[k] = float((err / np.where(scale > 0, scale, 1.0)).max())
        bad = err > TOL * scale
        assert not bad.any(), (what, name, int(bad.sum()), err[bad][:4], scale[bad][:4])
    print("%s: worst |device - host| / scale %.2e (E_R) %.2e (E_C)" % (what, worst[0], worst[1]))


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_device_matches_host_harness_on_every_model_row(harness, rid):
    """at error_cases.smooth_state with a random second state (every part of the state moved by a random direction of the
    size of the step's own increments), both outputs"""
    cs = cc.case(rid)
    asm = assembler(cs)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    fine = xc.moved(st, xc.direction(cs, 31))
    for lin in (False, True):
        dev = device_exact(asm, st, fine, adj, lin=lin)
        ref = xc.case_exact(harness, cs, st, fine, adj, lin=lin, scales=True)
        assert dev[0].shape == (len(cs.conn),) and np.abs(ref[0]).min() > 0
        if cs.model != "elastic":
            assert np.abs(ref[1]).max() > 0
        assert_close(dev, ref, (rid, "lin" if lin else "exact"), st, fine, adj[2])


# the block layout of c8_eval_error_contributions is kept (c8_exact.hip: exact_elems_per_block): the table of test_gpu_error.py
PER_BLOCK = {"hex8": 32, "tet4": 51, "tri3": 64, "tri3ps": 256}
MODEL = {"hex8": ("small_J2", pc.J2), "tet4": ("hyper_J2", pc.HJ2), "tri3": ("small_J2", pc.J2), "tri3ps": ("hyper_J2_plane_stress", pc.HJ2_PSS)}
COUNTS = [(k, n) for k, b in PER_BLOCK.items() for n in (1, b - 1, b, b + 1, 2 * b + 3)]


def _shape_mesh(kind, n):
    from meshes import brick, jiggle, jiggle_2d, tri_mesh
    if kind == "hex8":
        c, conn, sets = brick(n, 1, 1, 1.0 * n, 0.8, 0.7)
        return ol.HEX8, jiggle(c, sets, 0.04), conn
    if kind == "tet4":
        c, conn = cc.tet_mesh(3, 3, 2)  # 108 tets
        return (ol.TET4,) + cc.sub_mesh(c, conn, n)
    c, conn, sets = tri_mesh(17, 16, 1.0, 0.8)  # 544 triangles
    return (ol.TRI3,) + cc.sub_mesh(jiggle_2d(c, sets, 0.01), conn, n)


def _synthetic(asm, c, seed):
    """two synthetic states (cauchy_cases.synthetic_state, the local state moved upwards only: a negative hardening variable
    has no power) and random adjoints"""
    out = []
    for s in (seed, seed + 1000):
        u, p, u_prev, p_prev, xi_prev, xi = cc.synthetic_state(asm.new_state().cpu().numpy(), c, asm.ndims, asm.nres, seed=s)
        out.append((u, p, u_prev, p_prev, xi_prev, xi_prev + np.abs(xi - xi_prev)))
    xi = out[0][5]
    rng = np.random.default_rng(seed + 1)
    adj = rng.standard_normal(len(out[0][0])), rng.standard_normal(len(out[0][1])), rng.standard_normal(xi.shape)
    return out[0], out[1], adj


@pytest.mark.parametrize("kind,n", COUNTS, ids=["%s-%d" % kn for kn in COUNTS])
def test_element_counts_around_a_block(harness, kind, n):
    from calibr8_amd import Assembler
    et, c, conn = _shape_mesh(kind, n)
    model, params = MODEL[kind]
    asm = Assembler(et, c, conn, model, params)
    assert asm.nelems == n
    state, fine, adj = _synthetic(asm, c, seed=n)
    for lin in (False, True):
        dev = device_exact(asm, state, fine, adj, lin=lin)
        ref = xc.host_exact(harness, et, c, conn, model, params, state, fine, *adj, lin=lin, scales=True)
        assert_close(dev, ref, (kind, n, lin), state, fine, adj[2])
        assert len(np.unique(np.round(ref[0] / np.abs(ref[0]).max(), 9))) == n  # no two elements alike


def test_two_element_sets(harness):
    from calibr8_amd import Assembler
    et, c, conn = pc.mesh_of("hex8")
    es = (np.random.default_rng(21).random(len(conn)) < 0.4).astype(np.int32)
    params = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]
    asm = Assembler(et, c, conn, "small_J2", params, elem_set=es)
    state, fine, adj = _synthetic(asm, c, seed=5)
    for lin in (False, True):
        ref = xc.host_exact(harness, et, c, conn, "small_J2", params, state, fine, *adj, lin=lin, elem_set=es, scales=True)
        assert_close(device_exact(asm, state, fine, adj, lin=lin), ref, ("two sets", lin), state, fine, adj[2])
        one = xc.host_exact(harness, et, c, conn, "small_J2", params[:1], state, fine, *adj, lin=lin)
        assert np.array_equal(one[0][es == 0], ref[0][es == 0]) and np.abs(one[0][es == 1] - ref[0][es == 1]).min() > 0


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-hex8", "hyper_J2_plane_stress-tri3"])
def test_linearization_plus_contributions_is_exact_on_the_device(harness, rid):
    """on the device alone: the linearization fields plus the fields of c8_eval_error_contributions equal the exact fields,
    element by element, to 1e-12 of the summed magnitudes of the terms of the linearization fields (which hold those of
    both): a small-strain, a finite-deformation and a plane-stress model"""
    import torch
    cs = cc.case(rid)
    asm = assembler(cs)
    adj = ec.adjoints(cs)
    st = xc.smooth(rid, cs)
    fine = xc.moved(st, xc.direction(cs, 32))
    ex = device_exact(asm, st, fine, adj)
    lin = device_exact(asm, st, fine, adj, lin=True)
    con = asm.error_contributions(*[asm.dev(a) for a in st], *[asm.dev(a) for a in adj])
    torch.cuda.synchronize()
    scales = xc.case_exact(harness, cs, st, fine, adj, lin=True, scales=True)
    for k in (0, 1):
        err = np.abs(lin[k] + con[k].cpu().numpy() - ex[k])
        print("%s %s: worst |lin + contributions - exact| / scale %.2e" % (rid, "RC"[k], (err / scales[2 + k]).max()))
        assert np.abs(ex[k]).max() > 0 and np.all(err <= TOL * scales[2 + k]), (rid, k)


@pytest.mark.parametrize("lin", [False, True])
def test_calls_are_reproducible_accumulate_and_leave_the_fine_state_alone(lin):
    import torch
    cs = cc.case("small_J2-hex8")
    asm = assembler(cs)
    st = xc.smooth("small_J2-hex8", cs)
    fine = xc.moved(st, xc.direction(cs, 33))
    dst, dfine = [asm.dev(a) for a in st], [asm.dev(a) for a in fine]
    adj = [asm.dev(a) for a in ec.adjoints(cs)]
    before = [t.clone() for t in dst + dfine + adj]
    call = asm.linearization_errors if lin else asm.exact_errors
    n = asm.nelems
    r1, c1 = call(dst, dfine, *adj)
    r2, c2 = call(dst, dfine, *adj)
    torch.cuda.synchronize()
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and float(r1.abs().min()) > 0 and float(c1.abs().max()) > 0
    call(dst, dfine, *adj, E_R=r2, E_C=c2)
    torch.cuda.synchronize()
    assert torch.equal(r2, 2.0 * r1) and torch.equal(c2, 2.0 * c1)
    start = torch.linspace(-3.0, 5.0, n, dtype=torch.float64, device=asm.device)
    r3, c3 = start.clone(), -start.clone()
    call(dst, dfine, *adj, E_R=r3, E_C=c3)
    torch.cuda.synchronize()
    assert torch.equal(r3, start + r1) and torch.equal(c3, -start + c1)
    # outputs at an address that is 8- but not 16-byte aligned, canaries on both sides
    bufs = [torch.full((n + 3,), -7.25, dtype=torch.float64, device=asm.device) for _ in range(2)]
    outs = [b[1:n + 1] for b in bufs]
    for o in outs:
        assert o.data_ptr() % 16 == 8
        o.zero_()
    call(dst, dfine, *adj, E_R=outs[0], E_C=outs[1])
    torch.cuda.synchronize()
    assert torch.equal(outs[0], r1) and torch.equal(outs[1], c1)
    for b in bufs:
        assert float(b[0]) == -7.25 and bool((b[n + 1:] == -7.25).all())
    assert all(torch.equal(a, b) for a, b in zip(before, dst + dfine + adj))  # every input as it was
    # st_fine = st: the exact fields stay exactly 0 (test_linearization_plus_contributions_is_exact_on_the_device has the rest)
    if not lin:
        same = call(dst, [t.clone() for t in dst], *adj)
        torch.cuda.synchronize()
        assert not bool(same[0].any()) and not bool(same[1].any())


def test_async_mode_reports_through_c8_status():
    import torch
    cs = cc.case("hyper_J2-tet4")
    asm = assembler(cs)
    st = xc.smooth("hyper_J2-tet4", cs)
    dst, dfine = [asm.dev(a) for a in st], [asm.dev(a) for a in xc.moved(st, xc.direction(cs, 34))]
    adj = [asm.dev(a) for a in ec.adjoints(cs)]
    ref = asm.exact_errors(dst, dfine, *adj), asm.linearization_errors(dst, dfine, *adj)
    asm.set_async(True)
    got = asm.exact_errors(dst, dfine, *adj), asm.linearization_errors(dst, dfine, *adj)
    assert asm.status() == 0  # synchronises the stream
    for g, r in zip(got, ref):
        assert torch.equal(g[0], r[0]) and torch.equal(g[1], r[1])
    asm.set_async(False)


@pytest.mark.parametrize("entry", ["c8_eval_exact_errors", "c8_eval_linearization_errors"])
def test_refusals(entry):
    from calibr8_amd import Assembler, lib
    cs = cc.case("small_J2-hex8")
    asm = assembler(cs)
    L = asm.L
    fn = getattr(L, entry)
    dstate = [asm.dev(a) for a in cs.state]
    dfine = [asm.dev(a) for a in xc.moved(cs.state, xc.direction(cs, 35))]
    z_u, z_p, phi = [asm.dev(a) for a in ec.adjoints(cs)]
    E_R, E_C = asm.exact_errors(dstate, dfine, z_u, z_p, phi)
    good, fine = asm._state(*dstate), asm._state(*dfine)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    zs = lambda a, b: (C.c_void_p * 2)(a, b)
    z = zs(z_u.data_ptr(), z_p.data_ptr())
    ok = [asm.h, C.byref(good), C.byref(fine), z, ptr(phi), ptr(E_R), ptr(E_C)]
    assert fn(*ok) == lib.C8_OK
    for k in range(7):
        bad = list(ok)
        bad[k] = None
        assert fn(*bad) == lib.C8_ERR_ARG
        assert (entry + ": null").encode() in L.c8_last_error()
    for zz in (zs(None, z_p.data_ptr()), zs(z_u.data_ptr(), None)):
        assert fn(asm.h, C.byref(good), C.byref(fine), zz, ptr(phi), ptr(E_R), ptr(E_C)) == lib.C8_ERR_ARG

    def broken(tensors, field, k=None):
        s = asm._state(*tensors)
        if k is None:
            setattr(s, field, None)
        else:
            getattr(s, field)[k] = None
        return s

    holes = (("xi", None), ("xi_prev", None), ("x", 0), ("x", 1), ("x_prev", 0), ("x_prev", 1))
    for field, k in holes:  # missing entries of st, then of st_fine
        assert fn(asm.h, C.byref(broken(dstate, field, k)), C.byref(fine), z, ptr(phi), ptr(E_R), ptr(E_C)) == lib.C8_ERR_ARG
        assert fn(asm.h, C.byref(good), C.byref(broken(dfine, field, k)), z, ptr(phi), ptr(E_R), ptr(E_C)) == lib.C8_ERR_ARG
        assert (entry + ": null").encode() in L.c8_last_error()
    # one residual: x[1], x_prev[1] of both states and z[1] are not read
    ps = cc.case("hyper_J2_plane_stress-tri3")
    pasm = assembler(ps)
    pstate = [pasm.dev(a) for a in ps.state]
    pfine = [pasm.dev(a) for a in xc.moved(ps.state, xc.direction(ps, 36))]
    pz_u, pz_p, pphi = [pasm.dev(a) for a in ec.adjoints(ps)]
    call = pasm.exact_errors if entry == "c8_eval_exact_errors" else pasm.linearization_errors
    ref = call(pstate, pfine, pz_u, pz_p, pphi)
    s, sf = pasm._state(*pstate), pasm._state(*pfine)
    for t in (s, sf):
        t.x[1], t.x_prev[1] = None, None
    out = [t.clone().zero_() for t in ref]
    assert getattr(pasm.L, entry)(pasm.h, C.byref(s), C.byref(sf), zs(pz_u.data_ptr(), None), ptr(pphi), ptr(out[0]), ptr(out[1])) == lib.C8_OK
    assert all(np.array_equal(o.cpu().numpy(), r.cpu().numpy()) for o, r in zip(out, ref))
    # the hybrid model without its network, as the assemblies refuse it
    hyb = cc.case(cc.HYBRID + "-tri3")
    bare = Assembler(hyb.et, hyb.c, hyb.conn, hyb.model, hyb.params)
    bcall = bare.exact_errors if entry == "c8_eval_exact_errors" else bare.linearization_errors
    hst = [bare.dev(a) for a in hyb.state]
    with pytest.raises(lib.C8Error) as ei:
        bcall(hst, hst, *[bare.dev(a) for a in ec.adjoints(hyb)])
    assert ei.value.code == lib.C8_ERR_ARG and "embedded network" in str(ei.value)


# ---- model_form_error_verify end to end (error_cases.mfe_case; replayed on the CPU by test_exact_host.py) ----------------
def _primal(params, model="small_J2", steps=ec.MFE_STEPS, **kw):
    from calibr8_amd import Assembler, PrimalDriver
    c, conn, spec = ec.mfe_case()
    asm = Assembler(8, c, conn, model, params, **kw)
    return PrimalDriver(asm, spec, max_iters=25, abs_tol=ec.MFE_TOL, rel_tol=ec.MFE_TOL).solve(steps)


@pytest.fixture(scope="module")
def base():
    return _primal(pc.J2)


def _check_identity(r, what, not_by_smallness=True):
    """main_model_form_error_verify.cpp:196 with the fine run's residual bound: |E_computed - E_exact| <= 1e-8 |E_exact| +
    allowance; and the linearization error and |eta - E_exact| both more than 1000 x that bound"""
    bound = 1e-8 * abs(r.E_exact) + r.allowance
    gap, E_lin = abs(r.E_computed - r.E_exact), abs(r.E_lin_R + r.E_lin_C)
    print("%s: E_exact %.6e eta %.6e E_lin_R %.6e E_lin_C %.6e traction %.3e |E_computed - E_exact| %.3e allowance %.3e bound "
          "%.3e |E_lin| / bound %.3e" % (what, r.E_exact, r.eta, r.E_lin_R, r.E_lin_C, r.traction, gap, r.allowance, bound, E_lin / bound))
    assert gap <= bound, (what, gap, bound)
    if not_by_smallness:
        assert E_lin > 1000.0 * bound and abs(r.eta - r.E_exact) > 1000.0 * bound, (what, E_lin, abs(r.eta - r.E_exact), bound)
    return bound


def test_model_form_error_verify_closes_the_identity(base):
    """mfe_case (3 x 3 x 3 hex8, three steps), fine model small_J2 with K (1 + delta), delta = exact_cases.MFE_VERIFY_DELTA as
    chosen by the replay on the CPU (figures there)."""
    from calibr8_amd import model_form_error, model_form_error_verify
    fine = _primal(ec.mfe_params(xc.MFE_VERIFY_DELTA))
    r = model_form_error_verify(base, fine)
    assert fine.asm.kernel == "auto" and r.traction == 0.0
    bound = _check_identity(r, "mfe_case")
    assert r.E_exact == r.J_h - r.J_H and r.E_computed == r.eta + r.E_lin_R + r.E_lin_C
    F = r.fields
    assert F["E_R"].shape == (base.asm.nelems,)
    assert abs(float((F["E_exact_R"] + F["E_exact_C"]).sum()) - r.E_exact) <= bound
    # eta and its fields are those of model_form_error
    m = model_form_error(base, fine.asm)
    assert m.eta == r.eta and bool((m.E_R == F["E_R"]).all()) and bool((m.E_C == F["E_C"]).all())


def test_model_form_error_verify_with_tractions():
    """a traction-driven run: z . T enters eta with a minus and E_lin_R with a plus sign (tbcs.cpp:322, :235) and cancels in
    E_computed; the criterion still holds"""
    from calibr8_amd import Assembler, PrimalDriver, model_form_error_verify
    from meshes import brick, jiggle
    c, conn, sets = brick(3, 3, 3, 1.0, 1.0, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero)]
    top = [[e[3], e[2], e[6], e[7]] for e in conn if np.isin(e[[3, 2, 6, 7]], sets["ymax"]).all()]  # quad faces of the ymax side
    assert len(top) == 9
    tbcs = [(0, np.array(top, dtype=np.int32), lambda x, y, z, t: (0.0, 0.8 * t, 0.0))]
    runs = []
    for prm in (pc.J2, ec.mfe_params(xc.MFE_VERIFY_DELTA)):
        asm = Assembler(8, c, conn, "small_J2", prm)
        runs.append(PrimalDriver(asm, spec, tbcs, max_iters=25, abs_tol=ec.MFE_TOL, rel_tol=ec.MFE_TOL).solve(3))
    assert float((runs[0].xi[3][:, :, 6] > 0).double().mean()) > 0.3
    r = model_form_error_verify(*runs)
    assert abs(r.traction) > 1e-6
    inner = float((r.fields["E_R"] + r.fields["E_C"]).sum())
    assert r.eta == inner + r.traction and r.E_lin_R == float(r.fields["E_lin_R"].sum()) - r.traction
    _check_identity(r, "traction run")
    assert abs(r.E_lin_R + r.E_lin_C) > 0


def test_model_form_error_verify_refusals(base):
    from calibr8_amd import Assembler, PrimalDriver, model_form_error_verify
    from meshes import brick
    c, conn, spec = ec.mfe_case()
    fine = _primal(ec.mfe_params(xc.MFE_VERIFY_DELTA), steps=1)
    with pytest.raises(ValueError, match="steps"):
        model_form_error_verify(base, fine)
    with pytest.raises(ValueError, match="local state"):
        model_form_error_verify(base, _primal(pc.HJ2, "hyper_J2", steps=0))
    c2, conn2, _ = brick(3, 3, 2, 1.0, 1.0, 1.0)
    other = PrimalDriver(Assembler(8, c2, conn2, "small_J2", pc.J2), [])
    with pytest.raises(ValueError, match="mesh"):
        model_form_error_verify(base, other)
    fewer = PrimalDriver(Assembler(8, c, conn, "small_J2", pc.J2), spec[:-1])
    fewer.u, fewer.p, fewer.xi = list(base.u), list(base.p), list(base.xi)
    with pytest.raises(ValueError, match="boundary conditions"):
        model_form_error_verify(base, fewer)
    # a non-linear objective: only valid for linear QoIs
    a1, a2 = Assembler(8, c, conn, "small_J2", pc.J2), Assembler(8, c, conn, "small_J2", pc.J2)
    for a in (a1, a2):
        a.set_qoi_calibration(conn[:2, :4], comp=1)
    p1, p2 = PrimalDriver(a1, spec), PrimalDriver(a2, spec)
    with pytest.raises(ValueError, match="linear QoIs"):
        model_form_error_verify(p1, p2)
