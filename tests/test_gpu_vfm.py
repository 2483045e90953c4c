"""`-m gpu`: the virtual fields method on the device (c8_vfm_*, calibr8_amd.VFMProblem).  The V, FS and A kernels against
the oracle compositions at 1e-12; the reference's two VFM decks (test/vfm/*.yaml.in, values restated here) end to end on
notch2D with synthetic data made on the device; consistency, reproducibility, part sums, refusals, a short calibration
and one step on a mesh of a million triangles."""
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
from parity import rel_vec
from vfm_cases import CYCLIC, MODELS, make_oracle, oracle_adjoint_step, oracle_power, vfm_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the decks: small_hill_plane_stress, E nu Y S D R00 R11 R22 R01; data generated at Y 2, S 10, D 50, calibrated from
# Y 2.2, S 8, D 60 within [1, 3] [5, 15] [40, 80]
TRUTH = [1000.0, 0.25, 2.0, 10.0, 50.0, 1.0, 1.0, 1.0, 1.0]
TRIAL = [1000.0, 0.25, 2.2, 8.0, 60.0, 1.0, 1.0, 1.0, 1.0]
ACTIVE = [2, 3, 4]
BOUNDS = [(1.0, 3.0), (5.0, 15.0), (40.0, 80.0)]


def notch2d():
    d = json.load(open(os.path.join(HERE, "golden", "notch2D_tri3.json")))
    return np.array(d["coords"]), np.array(d["conn"], dtype=np.int32), {k: np.array(v, dtype=np.int32) for k, v in d["node_sets"].items()}


def virtual_field(c):
    x, y = c[:, 0], c[:, 1]
    return np.ascontiguousarray(np.stack([np.cos(np.pi * (y - 0.5)) * x, y * y], axis=1).ravel())


def synthetic(tol=1e-8):
    """the primal run of the decks on the device: measured u_0..u_4 and the y reaction on y = 1 (L_1..L_4)"""
    import torch
    from calibr8_amd import Assembler
    from calibr8_amd.primal import PrimalDriver
    c, conn, ns = notch2d()
    asm = Assembler(3, c, conn, "small_hill_plane_stress", TRUTH, max_iters=20)
    dbcs = [(0, 0, ns["xmin"], lambda x, y, z, t: 0.0), (0, 1, ns["ymin"], lambda x, y, z, t: 0.0),
            (0, 1, ns["ymax"], lambda x, y, z, t: 0.01 * t)]
    drv = PrimalDriver(asm, dbcs, max_iters=30, abs_tol=tol, rel_tol=tol).solve(4)
    loads = []
    for s in range(1, 5):
        ls = asm.new_linsys()
        assert asm.global_residual(drv.u[s], drv.p[s], drv.u[s - 1], drv.p[s - 1], drv.xi[s - 1], drv.xi[s], ls) == 0
        loads.append(float(ls.b[0].reshape(-1, 2)[torch.as_tensor(ns["ymax"], device=asm.device).long(), 1].sum()))
    return c, conn, ns, [u.clone() for u in drv.u], loads


_DATA = {}


def data(tol=1e-8):
    if tol not in _DATA:
        _DATA[tol] = synthetic(tol)
    return _DATA[tol]


def problem(gradient, thickness=1.0, tol=1e-8, params=TRIAL):
    from calibr8_amd import Assembler, VFMProblem
    c, conn, ns, u, loads = data(tol)
    asm = Assembler(3, c, conn, "small_hill_plane_stress", params, max_iters=20)
    return VFMProblem(asm, u, loads, virtual_field(c), [0.0, 1.0, 2.0, 3.0, 4.0], scale=1e2, thickness=thickness,
                      active=ACTIVE, bounds=BOUNDS, gradient=gradient)


# ---- 1. the kernels against the oracle compositions -----------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["notch2D", "two_sets"])
@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_kernels_match_oracle(mesh, model, params):
    check_vfm_kernels(mesh, model, params, None)


@pytest.mark.parametrize("mesh", ["notch2D", "two_sets"])
@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_kernels_match_oracle_cyclic(mesh, model, params):
    # every step of the cyclic measured sequence (hold, elastic unloading, reversed flow)
    check_vfm_kernels(mesh, model, params, CYCLIC)


def check_vfm_kernels(mesh, model, params, seq):
    import torch
    from calibr8_amd import Assembler
    c, conn, es, P, active, steps, w = vfm_case(mesh, model, params, seq)
    orc = make_oracle(c, conn, model, P, es, active)
    asm = Assembler(3, c, conn, model, P, elem_set=es)
    for s, a in enumerate(active):
        asm.set_active(s, a)
    nact = sum(len(a) for a in active)
    d = asm.dev
    dw = d(w)
    asm.vfm_set_virtual_field(dw)
    p0 = torch.zeros(asm.nnodes, dtype=torch.float64, device=asm.device)
    xi_prev = orc.new_state()
    S_prev = None
    rng = np.random.default_rng(5)
    for n in range(1, len(steps)):
        u, up = steps[n], steps[n - 1]
        rc, xo, bo = oracle_power(orc, u, up, xi_prev)
        assert rc == 0
        wabs = float(np.abs(w) @ np.abs(bo))
        du, dup, dxip = d(u), d(up), d(xi_prev)
        xv, b, ivw = d(xi_prev), torch.zeros(len(u), dtype=torch.float64, device=asm.device), torch.zeros(1, dtype=torch.float64, device=asm.device)
        assert asm.vfm_internal_power(du, p0, dup, p0, dxip, xv, ivw, b) == 0
        assert rel_vec(xv.cpu().numpy(), xo) < 1e-12 and rel_vec(b.cpu().numpy(), bo) < 1e-12
        assert abs(float(ivw[0]) - float(w @ bo)) < 1e-12 * wabs
        xf, ivf = d(xi_prev), torch.zeros(1, dtype=torch.float64, device=asm.device)
        S = torch.zeros(orc.nelems * orc.npts * orc.nloc * nact, dtype=torch.float64, device=asm.device)
        divw = torch.zeros(nact, dtype=torch.float64, device=asm.device)
        assert asm.vfm_forward_sens(du, p0, dup, p0, dxip, xf, S_prev, S, ivf, divw) == 0
        assert rel_vec(xf.cpu().numpy(), xo) < 1e-12 and abs(float(ivf[0]) - float(w @ bo)) < 1e-12 * wabs
        S_prev = S
        # FS at step 1 against A with c = 1, h = 0: both are d(w^T R_1)/dp
        h = 1e-3 * rng.standard_normal(orc.nelems * orc.npts * orc.nloc) if n > 1 else np.zeros(orc.nelems * orc.npts * orc.nloc)
        cm = 0.7 if n > 1 else 1.0
        ho, go, gabs = oracle_adjoint_step(orc, u, up, xi_prev, xo, w, cm, h, nact)
        dh, grad = d(h), torch.zeros(nact, dtype=torch.float64, device=asm.device)
        assert asm.vfm_adjoint_step(du, p0, dup, p0, dxip, d(xo), cm, dh, grad) == 0
        gd = grad.cpu().numpy()
        assert rel_vec(dh.cpu().numpy(), ho) < 1e-12
        assert np.all(np.abs(gd - go) <= 1e-12 * np.maximum(gabs, 1e-300)), (gd, go)
        if n == 1:
            assert np.abs(divw.cpu().numpy() - gd).max() < 1e-10 * np.abs(gd).max()
        xi_prev = xo


# ---- 2. the reference's decks: gradient check ------------------------------------------------------------------------
@pytest.mark.parametrize("gradient", ["adjoint", "forward"])
def test_reference_vfm_decks_fd_drop(gradient):
    from test_oracle_checks import canonical_fd_drop
    prob = problem(gradient)

    class Solved:  # as ROL's checkGradient: differences of the objective's value, its gradient at the base point
        def __init__(self, canonical):
            self.x = canonical

        def qoi(self):
            return prob.value(self.x)

        @property
        def g(self):
            return prob.physical_value_and_gradient(self.x)[1]

    def solve(params):
        return Solved(prob.to_canonical(np.asarray(params)[ACTIVE]))

    drop = canonical_fd_drop(solve, lambda pr, n: pr.g, np.array(TRIAL), dict(zip(ACTIVE, BOUNDS)))
    print("log10 drop (%s): %.4f" % (gradient, drop))
    assert abs(drop - 7.6799236451528792) < 0.1, drop


# ---- 3. at the generating parameters the mismatch vanishes -----------------------------------------------------------
def test_mismatch_vanishes_at_the_generating_parameters():
    prob = problem("adjoint", tol=1e-12, params=TRUTH)
    J = prob.value(prob.to_canonical(np.array(TRUTH)[ACTIVE]))
    loads = np.array(data(1e-12)[4])
    assert np.all(np.abs(loads) > 1e-3)
    assert np.all(np.abs(prob.thickness * prob.ivw - loads) <= 1e-8 * np.abs(loads)), (prob.ivw, loads)
    assert J < 1e-12


# ---- 4, 5. forward and adjoint agree, match central differences, and are reproducible ---------------------------------
def test_forward_adjoint_and_fd_agree_with_thickness():
    pa, pf = problem("adjoint", thickness=0.7), problem("forward", thickness=0.7)
    x = pa.to_canonical(np.array([2.3, 9.0, 55.0]))
    Ja, ga = pa.value_and_gradient(x)
    Jf, gf = pf.value_and_gradient(x)
    assert abs(Ja - Jf) <= 1e-13 * Ja and Ja > 0  # (V and FS form w^T R in kernels of their own)
    assert np.abs(ga - gf).max() < 1e-10 * np.abs(ga).max(), (ga, gf)
    for i in range(3):
        hstep = 1e-5
        xp, xm = x.copy(), x.copy()
        xp[i] += hstep
        xm[i] -= hstep
        fd = (pa.value(xp) - pa.value(xm)) / (2 * hstep)
        assert abs(fd - ga[i]) < 1e-6 * np.abs(ga).max(), (i, fd, ga[i])
    # the "fd" mode (forward differences of the same value)
    pd = problem("fd", thickness=0.7)
    Jd, gd = pd.value_and_gradient(x)
    assert abs(Jd - Ja) <= 1e-13 * Ja and np.abs(gd - ga).max() < 1e-4 * np.abs(ga).max(), (gd, ga)


def test_value_and_gradients_are_bitwise_reproducible():
    for gradient in ("adjoint", "forward"):
        prob = problem(gradient)
        x = prob.to_canonical(np.array([2.1, 9.0, 57.0]))
        J1, g1 = prob.value_and_gradient(x)
        J2, g2 = prob.value_and_gradient(x)
        assert J1 == J2 and np.array_equal(g1, g2)


# ---- 6. parts sum to the whole ---------------------------------------------------------------------------------------
def test_parts_sum_to_the_whole():
    import torch
    from calibr8_amd import Assembler
    c, conn, ns, u, loads = data()
    w = virtual_field(c)
    part = (c[conn].mean(axis=1)[:, 0] > np.median(c[:, 0])).astype(int)
    whole = [(np.arange(len(c)), conn)]
    pieces = []
    for k in range(2):
        el = conn[part == k]
        nodes = np.unique(el)
        local = np.full(len(c), -1)
        local[nodes] = np.arange(len(nodes))
        pieces.append((nodes, local[el].astype(np.int32)))

    def run(nodes, cn):
        asm = Assembler(3, c[nodes], cn, "small_hill_plane_stress", TRIAL, max_iters=20)
        asm.set_active(0, ACTIVE)
        asm.vfm_set_virtual_field(asm.dev(w.reshape(-1, 2)[nodes].ravel()))
        um = [asm.dev(x.cpu().numpy().reshape(-1, 2)[nodes].ravel()) for x in u]
        p0 = torch.zeros(asm.nnodes, dtype=torch.float64, device=asm.device)
        z = lambda n: torch.zeros(n, dtype=torch.float64, device=asm.device)
        xi, ivw, divw = [asm.new_state()], z(4), z(12).reshape(4, 3)
        S = [z(asm.nelems * asm.npts * asm.nloc * 3) for _ in range(2)]
        for s in range(1, 5):
            x = xi[-1].clone()
            assert asm.vfm_forward_sens(um[s], p0, um[s - 1], p0, xi[-1], x, S[s % 2] if s > 1 else None, S[(s + 1) % 2], ivw[s - 1:s], divw[s - 1]) == 0
            xi.append(x)
        h, grad = z(asm.nelems * asm.npts * asm.nloc), z(3)
        for s in range(4, 0, -1):
            assert asm.vfm_adjoint_step(um[s], p0, um[s - 1], p0, xi[s - 1], xi[s], 0.3 * s, h, grad) == 0
        return ivw.cpu().numpy(), divw.cpu().numpy(), grad.cpu().numpy()

    ref = run(*whole[0])
    parts = [run(*pc) for pc in pieces]
    for k in range(3):
        tot = parts[0][k] + parts[1][k]
        assert np.abs(tot - ref[k]).max() < 1e-12 * np.abs(ref[k]).max(), (k, tot, ref[k])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    import torch
    from calibr8_amd import Assembler, lib as _l
    from calibr8_amd.lib import C8Error
    c, conn, ns, u, loads = data()
    w = virtual_field(c)
    mixed = Assembler(3, c, conn, "small_J2", [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0])
    with pytest.raises(C8Error) as ei:
        mixed.vfm_set_virtual_field(mixed.dev(w))
    assert ei.value.code == _l.C8_ERR_UNSUPPORTED and b"pressure is not measured" in mixed.L.c8_last_error()
    asm = Assembler(3, c, conn, "small_hill_plane_stress", TRIAL, max_iters=20)
    p0 = torch.zeros(asm.nnodes, dtype=torch.float64, device=asm.device)
    ivw = torch.zeros(1, dtype=torch.float64, device=asm.device)
    with pytest.raises(C8Error) as ei:  # no virtual field
        asm.vfm_internal_power(u[1], p0, u[0], p0, asm.new_state(), asm.new_state(), ivw)
    assert ei.value.code == _l.C8_ERR_ARG and b"no virtual field" in asm.L.c8_last_error()
    asm.vfm_set_virtual_field(asm.dev(w))
    st = asm._state(u[1], p0, u[0], p0, asm.new_state(), asm.new_state())
    assert asm.L.c8_vfm_internal_power(asm.h, C.byref(st), None, None) == _l.C8_ERR_ARG
    assert asm.L.c8_vfm_adjoint_step(asm.h, C.byref(st), 1.0, None, None) == _l.C8_ERR_ARG
    assert asm.L.c8_vfm_forward_sens(asm.h, C.byref(st), None, None, C.c_void_p(ivw.data_ptr()), None) == _l.C8_ERR_ARG
    # a local solve that cannot converge (one local Newton iteration into the plastic range)
    from calibr8_amd import VFMProblem
    one = Assembler(3, c, conn, "small_hill_plane_stress", TRIAL, max_iters=1)
    assert one.vfm_set_virtual_field(one.dev(w)) is None
    x = one.new_state()
    assert one.vfm_internal_power(u[4], p0, u[3], p0, one.new_state(), x, ivw) == _l.C8_LOCAL_SOLVE_FAILED
    prob = VFMProblem(one, u, loads, w, [0, 1, 2, 3, 4], scale=1e2, active=ACTIVE, bounds=BOUNDS)
    assert prob.value_and_gradient(prob.to_canonical(np.array([2.2, 8.0, 60.0]))) is None


# ---- 8. a short calibration ------------------------------------------------------------------------------------------
def test_short_calibration_lowers_the_objective():
    prob = problem("adjoint")
    x0 = prob.to_canonical(np.array([2.2, 8.0, 60.0]))
    J0 = prob.value(x0)
    p, info = prob.solve([2.2, 8.0, 60.0], max_iters=40, grad_tol=1e-10, max_ls_evals=20)
    print("VFM calibration from (2.2, 8, 60): %s -> %s (truth 2, 10, 50), J %.3e -> %.3e, %s" %
          ("(%.4f, %.4f, %.4f)" % tuple([2.2, 8.0, 60.0]), "(%.4f, %.4f, %.4f)" % tuple(p), J0, info["f"], info))
    assert info["f"] <= 1e-4 * J0, (J0, info)


# ---- 9. full size ----------------------------------------------------------------------------------------------------
def test_one_step_on_a_million_triangles():
    import torch
    from calibr8_amd import Assembler
    from meshes import fields_for, prescribed_fields, tri_mesh
    c, conn, _ = tri_mesh(708, 708)
    assert len(conn) > 1_000_000
    model, params = MODELS[0]
    asm = Assembler(3, c, conn, model, params)
    asm.set_active(0, [0, 2, 3])
    u1, _ = fields_for(2, *prescribed_fields(c, 0.004, ramp=True, perturb=5e-2))
    w = np.ascontiguousarray(np.stack([np.cos(np.pi * (c[:, 1] - 0.5)) * c[:, 0], c[:, 1] ** 2], axis=1).ravel())
    d = asm.dev
    asm.vfm_set_virtual_field(d(w))
    z = lambda n: torch.zeros(n, dtype=torch.float64, device=asm.device)
    p0, du, dup = z(asm.nnodes), d(u1), z(len(u1))
    xip = asm.new_state()
    xv, ivw = asm.new_state(), z(1)
    assert asm.vfm_internal_power(du, p0, dup, p0, xip, xv, ivw) == 0
    xf, ivf, S, divw = asm.new_state(), z(1), z(asm.nelems * asm.npts * asm.nloc * 3), z(3)
    assert asm.vfm_forward_sens(du, p0, dup, p0, xip, xf, None, S, ivf, divw) == 0
    h, grad = z(asm.nelems * asm.npts * asm.nloc), z(3)
    assert asm.vfm_adjoint_step(du, p0, dup, p0, xip, xv, 1.0, h, grad) == 0
    assert abs(float(ivw[0]) - float(ivf[0])) <= 1e-12 * abs(float(ivw[0])) and rel_vec(xf.cpu().numpy(), xv.cpu().numpy()) < 1e-12
    gd, gf = grad.cpu().numpy(), divw.cpu().numpy()
    assert np.abs(gd - gf).max() < 1e-10 * np.abs(gd).max(), (gd, gf)
    # 200 sampled elements against the oracle on the sub-mesh they span (every output is per element)
    sample = np.random.default_rng(3).choice(len(conn), 200, replace=False)
    nodes = np.unique(conn[sample])
    local = np.full(len(c), -1)
    local[nodes] = np.arange(len(nodes))
    orc = ol.Oracle(ol.TRI3, c[nodes], local[conn[sample]].astype(np.int32), model, params)
    orc.set_active(0, [0, 2, 3])
    us = u1.reshape(-1, 2)[nodes].ravel()
    ws = w.reshape(-1, 2)[nodes].ravel()
    xs0 = np.ascontiguousarray(xip.cpu().numpy()[sample])
    rc, xo, bo = oracle_power(orc, us, np.zeros_like(us), xs0)
    assert rc == 0 and rel_vec(xv.cpu().numpy()[sample], xo) < 1e-12
    ho, _, _ = oracle_adjoint_step(orc, us, np.zeros_like(us), xs0, xo, ws, 1.0, np.zeros(xo.size), 3)
    assert rel_vec(h.cpu().numpy().reshape(len(conn), -1)[sample].ravel(), ho) < 1e-12
