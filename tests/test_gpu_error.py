"""`-m gpu`: c8_eval_error_contributions on the device and calibr8_amd.model_form_error.  The kernel compiles the same
per-point function as the host harness of test_error_host.py (which checks it against the oracle), so the device is compared
with that harness on identical inputs: every row of the model table on its standard mesh, and the element counts at which
the lane mapping (256 lanes per block, whole elements per block, the block's values handed over through LDS) can go wrong."""
import ctypes as C

import numpy as np
import pytest

import cauchy_cases as cc
import error_cases as ec
import oracle_lib as ol
import parity_cases as pc

pytestmark = pytest.mark.gpu
TOL = 1e-12  # of the summed magnitudes of the per-point values: the project's parity bar (device libm differs from glibc by ulps)


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return ec.build_harness(tmp_path_factory.mktemp("c8_error_host"))


def assembler(cs):
    from calibr8_amd import Assembler
    return Assembler(cs.et, cs.c, cs.conn, cs.model, cs.params, **cs.assembler_kw())


def device_error(asm, state, adj, E_R=None, E_C=None):
    import torch
    r, c = asm.error_contributions(*[asm.dev(a) for a in state], *[asm.dev(a) for a in adj], E_R=E_R, E_C=E_C)
    torch.cuda.synchronize()
    return r.cpu().numpy(), c.cpu().numpy()


def assert_close(dev, ref, what, state, phi):
    """device (E_R, E_C) against the harness's (E_R, E_C, abs_R, abs_C), element by element, at TOL of the summed magnitudes
    of the terms.  E_R: the per-point values w dv flux . grad z.  E_C: the products phi_j C_j -- and, since C_j is itself a
    difference of numbers of the size of the local state (C_j = xi_j - xi_prev_j - ... ; where a point is elastic or converged
    nothing but the rounding of that difference is left, and two libm's do not share it), phi_j times those: |phi_j| (|C_j| +
    |xi_j| + |xi_prev_j|).  For the small-strain models all three have the size of a strain increment; the finite-deformation
    models carry unknowns of size 1 (zeta, lambda_z) or of the size of a stress, and C cannot be formed more exactly than
    that."""
    operands = (np.abs(phi) * (np.abs(state[5]) + np.abs(state[4]))).sum(axis=(1, 2))
    for k, name in ((0, "E_R"), (1, "E_C")):
        scale = ref[2 + k] + (operands if k == 1 else 0.0)
        assert np.isfinite(dev[k]).all() and np.isfinite(ref[k]).all(), (what, name)
        bad = np.abs(dev[k] - ref[k]) > TOL * scale
        assert not bad.any(), (what, name, int(bad.sum()), np.abs(dev[k] - ref[k])[bad][:4], scale[bad][:4])


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_device_matches_host_harness_on_every_model_row(harness, rid):
    """at the state of the derivative checks (error_cases.smooth_state): away from the converged state, where C is a rounding
    residue that two libm's do not share, and away from the branch test"""
    cs = cc.case(rid)
    asm = assembler(cs)
    adj = ec.adjoints(cs)
    st = list(cs.state)
    st[5] = ec.smooth_state(rid, cs)
    dev = device_error(asm, st, adj)
    ref = ec.host_error(harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *st, *adj, nn=cs.nn, scales=True)
    assert dev[0].shape == (len(cs.conn),) and np.abs(ref[0]).min() > 0
    if cs.model != "elastic":
        assert np.abs(ref[1]).max() > 0
    assert_close(dev, ref, rid, st, adj[2])
    # E_R alone at the converged state as well (E_C is |C| < tol there, on both sides)
    dev = device_error(asm, cs.state, adj)
    ref = ec.host_error(harness, cs.et, cs.c, cs.conn, cs.model, cs.params, *cs.state, *adj, nn=cs.nn, scales=True)
    assert np.all(np.abs(dev[0] - ref[0]) <= TOL * ref[2]), rid
    assert np.all(np.abs(dev[1]) <= np.abs(adj[2]).sum(axis=(1, 2)) * ec.ABS_TOL), rid


# A block has 256 lanes and takes 256 // L whole elements, L the evaluations of an element (c8_error.hip:
# error_elems_per_block): hex8 32 (8 lanes: a point of ip set 0 and the same point of ip set 1 share one), tet4 51 (1 + 4),
# tri3 64 (1 + 3), tri3 under mechanics_plane_stress 256 (1 + 0).  Per class: one element, one below, equal to and one above
# a block, and two blocks and a bit (a partly filled last block).
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
    """cauchy_cases.synthetic_state with the local state moved upwards only (a negative hardening variable has no power)"""
    u, p, u_prev, p_prev, xi_prev, xi = cc.synthetic_state(asm.new_state().cpu().numpy(), c, asm.ndims, asm.nres, seed=seed)
    rng = np.random.default_rng(seed + 1)
    adj = rng.standard_normal(len(u)), rng.standard_normal(len(p)), rng.standard_normal(xi.shape)
    return (u, p, u_prev, p_prev, xi_prev, xi_prev + np.abs(xi - xi_prev)), adj


@pytest.mark.parametrize("kind,n", COUNTS, ids=["%s-%d" % kn for kn in COUNTS])
def test_element_counts_around_a_block(harness, kind, n):
    from calibr8_amd import Assembler
    et, c, conn = _shape_mesh(kind, n)
    model, params = MODEL[kind]
    asm = Assembler(et, c, conn, model, params)
    assert asm.nelems == n
    state, adj = _synthetic(asm, c, seed=n)
    dev = device_error(asm, state, adj)
    ref = ec.host_error(harness, et, c, conn, model, params, *state, *adj, scales=True)
    assert_close(dev, ref, (kind, n), state, adj[2])
    assert len(np.unique(np.round(ref[0] / np.abs(ref[0]).max(), 9))) == n  # no two elements alike


def test_two_element_sets(harness):
    from calibr8_amd import Assembler
    et, c, conn = pc.mesh_of("hex8")
    es = (np.random.default_rng(21).random(len(conn)) < 0.4).astype(np.int32)
    params = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]
    asm = Assembler(et, c, conn, "small_J2", params, elem_set=es)
    state, adj = _synthetic(asm, c, seed=5)
    ref = ec.host_error(harness, et, c, conn, "small_J2", params, *state, *adj, elem_set=es, scales=True)
    assert_close(device_error(asm, state, adj), ref, "two sets", state, adj[2])
    one = ec.host_error(harness, et, c, conn, "small_J2", params[:1], *state, *adj)
    assert np.array_equal(one[0][es == 0], ref[0][es == 0]) and np.abs(one[0][es == 1] - ref[0][es == 1]).min() > 0


@pytest.mark.parametrize("rid", ["small_J2-hex8", "hyper_J2-hex8", "hyper_J2_plane_stress-tri3"])
def test_sum_of_E_R_is_z_dot_the_assembled_residual(rid):
    """on the device alone: sum_e E_R = z . b with b from Assembler.global_residual into a zeroed system at the same state,
    to 1e-12 of sum |z_i b_i|: a small-strain, a finite-deformation and a plane-stress model"""
    import torch
    cs = cc.case(rid)
    asm = assembler(cs)
    dstate = [asm.dev(a) for a in cs.state]
    z_u, z_p, phi = [asm.dev(a) for a in ec.adjoints(cs)]
    E_R, _ = asm.error_contributions(*dstate, z_u, z_p, phi)
    ls = asm.new_linsys()
    assert asm.global_residual(*dstate, ls) == 0
    torch.cuda.synchronize()
    terms = [z_u * ls.b[0]] + ([z_p * ls.b[1]] if asm.nres == 2 else [])
    ref, scale = sum(float(t.sum()) for t in terms), sum(float(t.abs().sum()) for t in terms)
    err = abs(float(E_R.sum()) - ref)
    print("%s: |sum E_R - z.b| %.3e, sum |z_i b_i| %.3e" % (rid, err, scale))
    assert scale > 0 and err < 1e-12 * scale, (rid, err, scale)


def test_calls_are_reproducible_accumulate_and_keep_their_bounds():
    import torch
    cs = cc.case("small_J2-hex8")
    asm = assembler(cs)
    st = list(cs.state)
    st[5] = ec.mid_state(cs)
    args = [asm.dev(a) for a in st] + [asm.dev(a) for a in ec.adjoints(cs)]
    n = asm.nelems
    r1, c1 = asm.error_contributions(*args)
    r2, c2 = asm.error_contributions(*args)
    torch.cuda.synchronize()
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and float(r1.abs().min()) > 0 and float(c1.abs().max()) > 0
    # accumulation into what the outputs hold: a second call doubles, and a non-zero start is added to
    asm.error_contributions(*args, E_R=r2, E_C=c2)
    torch.cuda.synchronize()
    assert torch.equal(r2, 2.0 * r1) and torch.equal(c2, 2.0 * c1)
    start = torch.linspace(-3.0, 5.0, n, dtype=torch.float64, device=asm.device)
    r3, c3 = start.clone(), -start.clone()
    asm.error_contributions(*args, E_R=r3, E_C=c3)
    torch.cuda.synchronize()
    assert torch.equal(r3, start + r1) and torch.equal(c3, -start + c1)
    # outputs at an address that is 8- but not 16-byte aligned, canaries on both sides
    bufs = [torch.full((n + 3,), -7.25, dtype=torch.float64, device=asm.device) for _ in range(2)]
    outs = [b[1:n + 1] for b in bufs]
    for o in outs:
        assert o.data_ptr() % 16 == 8
        o.zero_()
    asm.error_contributions(*args, E_R=outs[0], E_C=outs[1])
    torch.cuda.synchronize()
    assert torch.equal(outs[0], r1) and torch.equal(outs[1], c1)
    for b in bufs:
        assert float(b[0]) == -7.25 and bool((b[n + 1:] == -7.25).all())


def test_async_mode_reports_through_c8_status():
    import torch
    cs = cc.case("hyper_J2-tet4")
    asm = assembler(cs)
    args = [asm.dev(a) for a in cs.state] + [asm.dev(a) for a in ec.adjoints(cs)]
    ref = asm.error_contributions(*args)
    asm.set_async(True)
    got = asm.error_contributions(*args)
    assert asm.status() == 0  # synchronises the stream
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    asm.set_async(False)


def test_refusals():
    from calibr8_amd import Assembler, lib
    cs = cc.case("small_J2-hex8")
    asm = assembler(cs)
    L = asm.L
    dstate = [asm.dev(a) for a in cs.state]
    z_u, z_p, phi = [asm.dev(a) for a in ec.adjoints(cs)]
    E_R, E_C = asm.error_contributions(*dstate, z_u, z_p, phi)
    good = asm._state(*dstate)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    zs = lambda a, b: (C.c_void_p * 2)(a, b)
    z = zs(z_u.data_ptr(), z_p.data_ptr())
    call = lambda h, st, zz, ph, r, c: L.c8_eval_error_contributions(h, st, zz, ph, r, c)
    assert call(asm.h, C.byref(good), z, ptr(phi), ptr(E_R), ptr(E_C)) == lib.C8_OK
    for bad in ((None, C.byref(good), z, ptr(phi), ptr(E_R), ptr(E_C)), (asm.h, None, z, ptr(phi), ptr(E_R), ptr(E_C)),
                (asm.h, C.byref(good), None, ptr(phi), ptr(E_R), ptr(E_C)), (asm.h, C.byref(good), z, None, ptr(E_R), ptr(E_C)),
                (asm.h, C.byref(good), z, ptr(phi), None, ptr(E_C)), (asm.h, C.byref(good), z, ptr(phi), ptr(E_R), None),
                (asm.h, C.byref(good), zs(None, z_p.data_ptr()), ptr(phi), ptr(E_R), ptr(E_C)),
                (asm.h, C.byref(good), zs(z_u.data_ptr(), None), ptr(phi), ptr(E_R), ptr(E_C))):
        assert call(*bad) == lib.C8_ERR_ARG
        assert b"c8_eval_error_contributions: null" in L.c8_last_error()

    def broken(field, k=None):
        s = asm._state(*dstate)
        if k is None:
            setattr(s, field, None)
        else:
            getattr(s, field)[k] = None
        return s

    for s in (broken("xi"), broken("xi_prev"), broken("x", 0), broken("x", 1), broken("x_prev", 0), broken("x_prev", 1)):
        assert call(asm.h, C.byref(s), z, ptr(phi), ptr(E_R), ptr(E_C)) == lib.C8_ERR_ARG
    # one residual: x[1], x_prev[1] and z[1] are not read
    ps = cc.case("hyper_J2_plane_stress-tri3")
    pasm = assembler(ps)
    pstate = [pasm.dev(a) for a in ps.state]
    pz_u, pz_p, pphi = [pasm.dev(a) for a in ec.adjoints(ps)]
    ref = pasm.error_contributions(*pstate, pz_u, pz_p, pphi)
    s = pasm._state(*pstate)
    s.x[1], s.x_prev[1] = None, None
    out = [t.clone().zero_() for t in ref]
    assert call(pasm.h, C.byref(s), zs(pz_u.data_ptr(), None), ptr(pphi), ptr(out[0]), ptr(out[1])) == lib.C8_OK
    assert all(np.array_equal(o.cpu().numpy(), r.cpu().numpy()) for o, r in zip(out, ref))
    # the hybrid model without its network, as the assemblies refuse it
    hyb = cc.case(cc.HYBRID + "-tri3")
    bare = Assembler(hyb.et, hyb.c, hyb.conn, hyb.model, hyb.params)
    with pytest.raises(lib.C8Error) as ei:
        bare.error_contributions(*[bare.dev(a) for a in hyb.state], *[bare.dev(a) for a in ec.adjoints(hyb)])
    assert ei.value.code == lib.C8_ERR_ARG and "embedded network" in str(ei.value)


# ---- model_form_error end to end (error_cases.mfe_case; replayed on the CPU by test_error_host.py) ----------------------
def _primal(params, model="small_J2", **kw):
    from calibr8_amd import Assembler, PrimalDriver
    c, conn, spec = ec.mfe_case()
    asm = Assembler(8, c, conn, model, params, **kw)
    return PrimalDriver(asm, spec, max_iters=25, abs_tol=ec.MFE_TOL, rel_tol=ec.MFE_TOL).solve(ec.MFE_STEPS)


@pytest.fixture(scope="module")
def base():
    pr = _primal(pc.J2)
    assert all(float((x[:, :, 6] > 0).double().mean()) > 0.5 for x in pr.xi[1:])  # every step yields
    return pr


def test_model_form_error_is_second_order_accurate(base):
    """(a) |eta - dJ|, dJ = J(fine primal run) - J(base), falls by a factor in [2.5, 6.5] from delta to delta / 2: both are
    exact to first order in delta (Taylor), the width of the band allows for the cubic term.  (b) the deviation of
    eta / (delta K) from dJ/dK of the base run's adjoint_gradient halves, within [1.5, 3].  The fine model is small_J2 with
    the hardening modulus K (1 + delta); delta as chosen by the replay on the CPU (error_cases.MFE_DELTA)."""
    from calibr8_amd import Assembler, adjoint_gradient, model_form_error
    c, conn, _ = ec.mfe_case()
    J0 = base.qoi()
    base.asm.set_active(0, [2])
    dJdK = adjoint_gradient(base, 1)[0]
    gap, dev = [], []
    for d in (ec.MFE_DELTA, 0.5 * ec.MFE_DELTA):
        prm = ec.mfe_params(d)
        dJ = _primal(prm).qoi() - J0
        fine = Assembler(8, c, conn, "small_J2", prm)
        r = model_form_error(base, fine)
        assert fine.kernel == "auto" and r.traction == 0.0 and abs(r.eta) <= r.eta_bound
        assert r.eta == float((r.E_R + r.E_C).sum()) and r.E_R.shape == (len(conn),)
        gap.append(abs(r.eta - dJ))
        dev.append(abs(r.eta / (d * pc.J2[2]) - dJdK))
        print("delta %g: dJ %.6e eta %.6e |eta - dJ| / |dJ| %.3e  |eta / (delta K) - dJ/dK| %.3e" % (d, dJ, r.eta, gap[-1] / abs(dJ), dev[-1]))
    print("factors: %.3f (a), %.3f (b)" % (gap[0] / gap[1], dev[0] / dev[1]))
    assert 2.5 <= gap[0] / gap[1] <= 6.5, gap
    assert 1.5 <= dev[0] / dev[1] <= 3.0, dev


def test_model_form_error_of_the_base_model_itself_is_at_the_solver_tolerances(base):
    """(c) fine context = base context: eta = sum_steps (z . R + phi . C) of a converged run.  The Newton iteration stops at
    |R|_2 < 1e-12 max(1, |R_0|_2), R_0 the first residual of the step, which the constrained rows dominate (diagonal x 0.003
    per constrained node: of order 10), the local one at |C|_2 < 1e-12 per point, so with r_n the residual norm of step n on
    the free rows (measured here, and itself asserted below 1e-10)  |eta| <= sum_n z_norm r_n + steps phi_norm 1e-12.
    eta_bound = sum_e |E_R + E_C| bounds |eta| but is not small: the element residuals z_e . R_e balance each other only in
    the sum over the elements of a node, whatever the tolerances."""
    import torch
    from calibr8_amd import model_form_error
    asm = base.asm
    r = model_form_error(base, asm)
    assert asm.kernel == "auto"  # put back
    free = torch.ones(asm.nnodes, 3, dtype=torch.bool, device=asm.device)
    for resid, eq, nodes, _ in base.dbcs:
        free[torch.as_tensor(np.asarray(nodes), device=asm.device), eq] = False
    allowed = ec.MFE_STEPS * r.phi_norm * ec.MFE_TOL
    for n in range(1, ec.MFE_STEPS + 1):
        ls = asm.new_linsys()
        assert asm.global_residual(base.u[n], base.p[n], base.u[n - 1], base.p[n - 1], base.xi[n - 1], base.xi[n], ls) == 0
        rn = float(torch.sqrt((ls.b[0].view(-1, 3)[free] ** 2).sum() + (ls.b[1] ** 2).sum()))
        assert rn < 1e-10, (n, rn)
        allowed += r.z_norm * rn
    print("eta %.3e allowed %.3e eta_bound %.3e z_norm %.3e phi_norm %.3e" % (r.eta, allowed, r.eta_bound, r.z_norm, r.phi_norm))
    assert abs(r.eta) <= allowed and abs(r.eta) <= r.eta_bound


def test_model_form_error_small_J2_to_small_hosford_and_mismatched_layouts(base):
    """a different fine model with the same seven local unknowns: the run completes (eta and the true dJ are an example
    recorded in DESIGN.md, not a check); eight local unknowns (hyper_J2), another mesh or another objective are refused"""
    from calibr8_amd import Assembler, model_form_error
    from meshes import brick
    c, conn, _ = ec.mfe_case()
    kw = dict(line_search=pc.LOCAL_LINE_SEARCH)
    r = model_form_error(base, Assembler(8, c, conn, "small_hosford", pc.HOSFORD, **kw))
    dJ = _primal(pc.HOSFORD, "small_hosford", **kw).qoi() - base.qoi()
    print("small_J2 -> small_hosford: eta %.6e eta_bound %.6e dJ %.6e" % (r.eta, r.eta_bound, dJ))
    assert np.isfinite(r.eta) and abs(r.eta) <= r.eta_bound
    with pytest.raises(ValueError, match="local state"):
        model_form_error(base, Assembler(8, c, conn, "hyper_J2", pc.HJ2))
    c2, conn2, _ = brick(3, 3, 2, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="mesh"):
        model_form_error(base, Assembler(8, c2, conn2, "small_J2", pc.J2))
    other = Assembler(8, c, conn, "small_J2", pc.J2)
    other.set_qoi_calibration(conn[:2, :4], comp=1)
    with pytest.raises(ValueError, match="objective"):
        model_form_error(base, other)


def test_model_form_error_reports_the_traction_term():
    """a traction-driven run: eta includes z . (-T), reported separately; for fine = base it balances the element sums"""
    from calibr8_amd import Assembler, PrimalDriver, model_form_error
    from meshes import brick, jiggle
    c, conn, sets = brick(3, 3, 3, 1.0, 1.0, 1.0)
    c = jiggle(c, sets, 0.05)
    zero = lambda x, y, z, t: 0.0
    spec = [(0, 0, sets["ymin"], zero), (0, 1, sets["ymin"], zero), (0, 2, sets["ymin"], zero)]
    top = [[e[3], e[2], e[6], e[7]] for e in conn if np.isin(e[[3, 2, 6, 7]], sets["ymax"]).all()]  # quad faces of the ymax side
    assert len(top) == 9
    tbcs = [(0, np.array(top, dtype=np.int32), lambda x, y, z, t: (0.0, 0.8 * t, 0.0))]
    asm = Assembler(8, c, conn, "small_J2", pc.J2)
    pr = PrimalDriver(asm, spec, tbcs, max_iters=25, abs_tol=ec.MFE_TOL, rel_tol=ec.MFE_TOL).solve(3)
    assert float((pr.xi[3][:, :, 6] > 0).double().mean()) > 0.3
    r = model_form_error(pr, asm)
    inner = float((r.E_R + r.E_C).sum())
    print("traction run: eta %.3e element sums %.6e traction %.6e" % (r.eta, inner, r.traction))
    assert abs(r.traction) > 1e-6 and r.eta == inner + r.traction
    assert abs(r.eta) < 1e-9 * abs(r.traction)
