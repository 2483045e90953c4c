"""hybrid_hyper_J2_plane_stress on the device through the C ABI: the linear-network identity against
hyper_J2_plane_stress, the weight-gradient kernel against autograd of the restated residual (tests/hybrid_ref.py) and
its reproducibility, and the refusals of the embedded-network entry points."""
import numpy as np
import pytest

import hybrid_ref as hr
from hybrid_cases import ABS_TOL, E, NU, Y, linear_relu_net, notch2d, stretch, tri_mesh

pytestmark = pytest.mark.gpu


def hybrid(coords, conn, act, topo, s_in, s_out, theta, params=(E, NU, Y), **kw):
    from calibr8_amd import Assembler
    emb = dict(activation=act, topology=topo, input_scale=s_in, output_scale=s_out, params=theta)
    return Assembler(3, coords, conn, "hybrid_hyper_J2_plane_stress", list(params), max_iters=20, abs_tol=ABS_TOL,
                     rel_tol=ABS_TOL, embedded=emb, **kw)


def test_linear_relu_network_equals_hyper_J2_plane_stress_on_device():
    import torch
    from calibr8_amd import Assembler
    rng = np.random.default_rng(3)
    topo, s_in, s_out = [1, 4, 3, 1], 2.0, 5.0
    theta, prod = linear_relu_net(rng, topo)
    coords, conn = tri_mesh(40, 30)
    hyb = hybrid(coords, conn, "relu", topo, s_in, s_out, theta)
    ref = Assembler(3, coords, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 0, s_in * s_out * prod], max_iters=20,
                    abs_tol=ABS_TOL, rel_tol=ABS_TOL)
    res = {}
    for name, a in (("hyb", hyb), ("ref", ref)):
        pz = a.dev(np.zeros(coords.shape[0]))
        xi_prev, up = a.new_state(), a.dev(np.zeros(coords.shape[0] * 2))
        out = []
        for s in (1, 2, 3):
            us = a.dev(stretch(coords, 0.008 * s))
            xi = xi_prev.clone()
            ls = a.new_linsys()
            assert a.forward_jacobian(us, pz, up, pz, xi_prev, xi, ls) == 0
            torch.cuda.synchronize()
            out.append((ls.b[0].cpu().numpy(), ls.A[0][0].cpu().numpy(), xi.cpu().numpy()))
            xi_prev, up = xi, us
        res[name] = out
    assert res["ref"][2][2][..., 5].max() > 0.0
    for (bh, Ah, xh), (br, Ar, xr) in zip(res["hyb"], res["ref"]):
        assert np.max(np.abs(bh - br)) <= 1e-12 * max(1.0, np.max(np.abs(br)))
        assert np.max(np.abs(Ah - Ar)) <= 1e-12 * np.max(np.abs(Ar))
        assert np.max(np.abs(xh - xr)) <= 1e-12


@pytest.mark.parametrize("act,topo", [("tanh", [1, 16, 16, 1]), ("sigmoid", [1, 8, 5, 7, 1]), ("relu", [1, 12, 9, 1])])
def test_weight_gradient_on_device_matches_autograd_and_repeats_bitwise(act, topo):
    import torch
    rng = np.random.default_rng(5)
    nt = hr.num_params(topo)
    theta = rng.normal(0.0, 0.6, nt)
    s_in, s_out = 3.0, 4.0
    coords, conn = tri_mesh(60, 50)  # 6000 elements: several blocks of the weight-gradient kernel
    a = hybrid(coords, conn, act, topo, s_in, s_out, theta)
    assert a.num_embedded_params == nt and a.num_grad_params == 1 + nt
    npts = a.nelems * a.npts
    xi = np.zeros((a.nelems, a.npts, 6))
    xi[..., 0:3] = rng.normal(0.0, 4e-3, (a.nelems, a.npts, 3))
    xi[..., 3], xi[..., 4] = 1.0, 1.0
    xi[..., 5] = np.abs(rng.normal(0.0, 0.05, (a.nelems, a.npts)))
    phi = rng.normal(0.0, 1.0, (a.nelems, a.npts, 6))
    z = a.dev(np.zeros(coords.shape[0] * 2))
    pz = a.dev(np.zeros(coords.shape[0]))
    d_xi, d_phi = a.dev(xi), a.dev(phi)
    grads = []
    for _ in range(2):
        g = a.dev(np.zeros(a.num_grad_params))
        a.qoi_gradient(z, pz, z, pz, d_xi, d_xi, z, pz, d_phi, g)
        torch.cuda.synchronize()
        grads.append(g.cpu().numpy()[1:])
    want = hr.theta_gradient(xi.reshape(npts, 6), phi.reshape(npts, 6), E, NU, Y, act, topo, s_in, s_out, theta, ABS_TOL)
    # the kernel adds the NN(0) term once per block of 1024 points, autograd once per point: over 6000 points the two
    # orders of a cancelling sum differ by a few ulps of the summed terms, 1e-12 of which the largest entry is not
    assert np.max(np.abs(grads[0] - want)) <= 1e-11 * np.max(np.abs(want))
    assert grads[0].tobytes() == grads[1].tobytes()


def test_embedded_entry_points_refuse():
    from calibr8_amd import Assembler
    from calibr8_amd.lib import C8Error
    coords, conn = tri_mesh(4, 3)
    topo = [1, 4, 1]
    theta = np.linspace(0.1, 0.9, hr.num_params(topo))
    # other models have no network
    other = Assembler(3, coords, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 0, 10.0])
    assert other.num_embedded_params == 0 and other.num_grad_params == 1
    with pytest.raises(C8Error) as e:
        other.set_embedded_model("tanh", topo, 1.0, 1.0)
    assert e.value.code == -4
    # bad topologies
    a = hybrid(coords, conn, "tanh", topo, 1.0, 1.0, None)
    for bad in ([1, 1], [2, 4, 1], [1, 4, 2], [1, 65, 1], [1, 4, 4, 4, 4, 4, 1], [1, 0, 1]):
        with pytest.raises(C8Error) as e:
            a.set_embedded_model("tanh", bad, 1.0, 1.0)
        assert e.value.code == -2
    # no weights yet: assemblies refuse
    pz, u = a.dev(np.zeros(coords.shape[0])), a.dev(np.zeros(coords.shape[0] * 2))
    xi = a.new_state()
    with pytest.raises(C8Error) as e:
        a.forward_jacobian(u, pz, u, pz, xi, xi.clone(), a.new_linsys())
    assert e.value.code == -2
    a.set_embedded_params(theta)
    assert np.array_equal(a.get_embedded_params(), theta)
    # VFM
    with pytest.raises(C8Error) as e:
        a.vfm_set_virtual_field(u)
    assert e.value.code == -4
    # the weight gradient on two element sets
    es = (np.arange(conn.shape[0]) % 2).astype(np.int32)
    from calibr8_amd import Assembler as A
    two = A(3, coords, conn, "hybrid_hyper_J2_plane_stress", [[E, NU, Y], [E, NU, Y]], elem_set=es,
            embedded=dict(activation="tanh", topology=topo, input_scale=1.0, output_scale=1.0, params=theta))
    g = two.dev(np.zeros(two.num_grad_params))
    phi = two.dev(np.zeros((two.nelems, two.npts, 6)))
    with pytest.raises(C8Error) as e:
        two.qoi_gradient(u, pz, u, pz, xi, xi, u, pz, phi, g)
    assert e.value.code == -4


def monotone_tanh_net(seed, topo=(1, 16, 16, 1)):
    """positive weights: NN rises with its input, so the hardening does"""
    rng = np.random.default_rng(seed)
    theta = np.abs(rng.normal(0.0, 0.4, hr.num_params(list(topo))))
    for _, b in hr.unpack(theta, list(topo)):
        b -= 0.2
    return theta


def notch_bcs(ns, rate):
    return [(0, 0, ns["xmin"], lambda x, y, z, t: 0.0), (0, 1, ns["ymin"], lambda x, y, z, t: 0.0),
            (0, 1, ns["ymax"], lambda x, y, z, t: rate * t)]


def test_notch2D_primal_with_linear_network_matches_hyper_J2_plane_stress():
    # PrimalDriver on notch2D: the hybrid model with a linear ReLU net against hyper_J2_plane_stress with K = K_eff
    from calibr8_amd import Assembler
    from calibr8_amd.primal import PrimalDriver
    c, conn, ns = notch2d()
    topo, s_in, s_out = [1, 4, 3, 1], 2.0, 5.0
    theta, prod = linear_relu_net(np.random.default_rng(3), topo)
    dbcs = notch_bcs(ns, 0.005)
    hyb = hybrid(c, conn, "relu", topo, s_in, s_out, theta)
    ref = Assembler(3, c, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 1, s_in * s_out * prod], max_iters=20,
                    abs_tol=ABS_TOL, rel_tol=ABS_TOL)
    runs = [PrimalDriver(a, dbcs, max_iters=30, abs_tol=1e-10, rel_tol=1e-10).solve(5) for a in (hyb, ref)]
    assert runs[0].newton_iters == runs[1].newton_iters
    J = [r.qoi() for r in runs]
    assert abs(J[0] - J[1]) <= 1e-10 * abs(J[1]), J
    assert float(runs[1].xi[-1][..., 5].max()) > 0.0


def test_notch2D_primal_with_tanh_network_matches_oracle_driver():
    # PrimalDriver on notch2D with the nonlinear tanh [1,16,16,1] net of the catalogue against fe_driver.Primal run over
    # the oracle's hybrid class: the global Newton iteration with its line search and the local solves inside it, four
    # steps, up to alpha ~ 0.28 at the notch (the first layer deep in saturation there)
    from calibr8_amd import Assembler
    from calibr8_amd.primal import PrimalDriver
    from fe_driver import Dbc, Primal
    from hybrid_cases import HYB, NETS, hybrid_oracle
    c, conn, ns = notch2d()
    net = NETS["tanh_16_16"]
    dbcs = notch_bcs(ns, 0.005)
    asm = Assembler(3, c, conn, HYB, [E, NU, Y], max_iters=500, abs_tol=ABS_TOL, rel_tol=ABS_TOL, embedded=net.embedded())
    drv = PrimalDriver(asm, dbcs, max_iters=30, abs_tol=1e-10, rel_tol=1e-10).solve(4)
    orc, _, _ = hybrid_oracle((3, c, conn), net, max_iters=500)
    ref = Primal(orc, c, [Dbc(*s) for s in dbcs], max_iters=30, abs_tol=1e-10, rel_tol=1e-10).solve(4)
    assert drv.newton_iters == ref.newton_iters, (drv.newton_iters, ref.newton_iters)
    J, Jr = drv.qoi(), ref.qoi()
    assert abs(J - Jr) <= 1e-10 * abs(Jr), (J, Jr)
    assert float(ref.xi[-1][..., 5].max()) > 0.1


def test_notch2D_adjoint_gradient_with_network_passes_fd_check():
    # c8_adjoint_solve_step with theta appended to grad, against central differences of the device objective along
    # E, nu, Y and along a random theta direction (tanh [1, 16, 16, 1])
    from calibr8_amd.primal import PrimalDriver, adjoint_gradient
    c, conn, ns = notch2d()
    topo, s_in, s_out = [1, 16, 16, 1], 5.0, 2.0
    theta0 = monotone_tanh_net(7)
    dbcs = notch_bcs(ns, 0.005)
    p0 = np.array([E, NU, Y])

    def solve(p, th):
        a = hybrid(c, conn, "tanh", topo, s_in, s_out, th, params=p)
        a.set_active(0, [0, 1, 2])
        return PrimalDriver(a, dbcs, max_iters=30, abs_tol=1e-12, rel_tol=1e-12).solve(4)

    drv = solve(p0, theta0)
    assert float(drv.xi[-1][..., 5].max()) > 0.0
    g = adjoint_gradient(drv, drv.asm.num_grad_params)
    assert len(g) == 3 + len(theta0)
    rng = np.random.default_rng(9)
    dirs = [(np.array([100.0, 0.05, 1.0]) * 0.1, np.zeros_like(theta0)),
            (np.zeros(3), 0.05 * rng.standard_normal(len(theta0)))]
    for dp_, dth in dirs:
        gd = float(g[:3] @ dp_ + g[3:] @ dth)
        errs = []
        for h in (1e-2, 1e-3, 1e-4):
            jp = solve(p0 + h * dp_, theta0 + h * dth).qoi()
            jm = solve(p0 - h * dp_, theta0 - h * dth).qoi()
            errs.append(abs((jp - jm) / (2 * h) - gd))
        assert min(errs) < 1e-6 * abs(gd), (errs, gd)


def test_inverse_problem_recovers_network_weights_and_Y():
    # synthetic calibration on notch2D: measurements from (Y*, theta*), start from a 5 % perturbation, InverseProblem with
    # embedded_bounds (optimisation vector [Y (bound-scaled), theta])
    import torch
    from calibr8_amd import InverseProblem
    from calibr8_amd.primal import PrimalDriver
    c, conn, ns = notch2d()
    topo, s_in, s_out = [1, 16, 16, 1], 5.0, 2.0
    theta_true = monotone_tanh_net(7, topo)
    truth = np.array([E, NU, Y])
    nsteps = 3
    dbcs = notch_bcs(ns, 0.005)
    measured = [None]

    def make_primal(params, theta):
        a = hybrid(c, conn, "tanh", topo, s_in, s_out, theta, params=params)
        a.set_qoi_calibration(None, weights=(1.0, 1.0, 0.0), balance=1e-2, coord_idx=1, coord_value=float(c[:, 1].min()),
                              coord_tol=1e-8, comp=1, dt_over_T=1.0 / nsteps)
        pr = PrimalDriver(a, dbcs, max_iters=30, abs_tol=1e-12, rel_tol=1e-12).solve(nsteps)
        if measured[0] is not None:
            pr.set_measured(*measured[0])
        return pr

    pt = make_primal(truth, theta_true)
    loads, zm = [0.0], torch.zeros_like(pt.u[1])
    for s in range(1, nsteps + 1):
        pt.asm.set_measured(zm, 0.0)
        loads.append(pt.asm.qoi_preprocess(pt.u[s], pt.p[s], pt.u[s - 1], pt.p[s - 1], pt.xi[s - 1], pt.xi[s])[1])
    measured[0] = ([None] + [u.clone() for u in pt.u[1:]], loads)
    bounds = np.stack([theta_true - 1.0, theta_true + 1.0], axis=1)
    inv = InverseProblem(make_primal, truth, [2], [[1.0, 4.0]], embedded_bounds=bounds)
    rng = np.random.default_rng(2)
    start_theta = theta_true * (1.0 + 0.05 * rng.choice([-1.0, 1.0], len(theta_true)))
    x0 = inv.to_canonical(np.concatenate([[1.05 * Y], start_theta]))
    J0 = inv.value_and_gradient(x0)[0]
    found, info = inv.solve([1.05 * Y], start_theta, max_iters=60, grad_tol=1e-14, step_tol=1e-14, max_ls_evals=8)
    assert J0 > 0.0 and info["f"] < 1e-3 * J0, (info, J0)


def test_million_triangles_step_matches_emulator_on_sampled_elements(tmp_path):
    # one K1 step on ~1M triangles on the device; the local states of 200 sampled elements against the CPU emulator on
    # the sub-mesh of those elements (a local state depends only on its own element's fields)
    import ctypes as C
    import os
    import subprocess
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libc8emul_hybrid.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(root, "tests", "emul_hybrid", "c8_emul_hybrid.cpp"),
                           os.path.join(root, "calibr8_amd", "csrc", "c8_host.cpp")])
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.c8emu_hybrid_call.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, ip, C.c_int, C.c_int, C.c_double, C.c_double, dp, ip,
                                    dp, C.POINTER(dp)]
    topo, s_in, s_out = [1, 16, 16, 1], 5.0, 2.0
    theta = monotone_tanh_net(11)
    c, conn = tri_mesh(708, 708)
    a = hybrid(c, conn, "tanh", topo, s_in, s_out, theta)
    u = stretch(c, 0.01) + 1e-3 * np.sin(7.0 * np.repeat(c[:, 0], 2))
    pz = a.dev(np.zeros(c.shape[0]))
    xi = a.new_state()
    xip = xi.clone()
    assert a.forward_jacobian(a.dev(u), pz, a.dev(np.zeros_like(u)), pz, xip, xi, a.new_linsys()) == 0
    torch.cuda.synchronize()
    xi_d = xi.cpu().numpy()
    assert (xi_d[..., 5] > 0).mean() > 0.1
    sample = np.random.default_rng(1).choice(len(conn), 200, replace=False)
    nodes, sub = np.unique(conn[sample], return_inverse=True)
    sub = np.ascontiguousarray(sub.reshape(-1, 3), dtype=np.int32)
    sc = np.ascontiguousarray(c[nodes])
    su = np.ascontiguousarray(u.reshape(-1, 2)[nodes].ravel())
    nn_buf = hr.buffer("tanh", topo, s_in, s_out, theta)
    P = np.ascontiguousarray([E, NU, Y])
    act = np.zeros(10, dtype=np.int32)
    xi_e = np.zeros((200, 1, 6))
    xi_e[..., 3], xi_e[..., 4] = 1.0, 1.0
    xip_e = xi_e.copy()
    zeros = np.zeros(len(nodes) * 2)
    pze = np.zeros(len(nodes))
    import oracle_lib as ol
    orc = ol.Oracle(ol.TRI3, sc, sub, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 1, 0])
    ls = orc.new_linsys()
    ptrs = (dp * 18)()
    for k, arr in {0: su, 1: pze, 2: zeros, 3: pze, 4: xip_e, 5: xi_e, 6: ls.A[0][0], 7: ls.A[0][1], 8: ls.A[1][0],
                   9: ls.A[1][1], 10: ls.b[0], 11: ls.b[1]}.items():
        if arr is not None and len(arr):
            ptrs[k] = np.ascontiguousarray(arr).ctypes.data_as(dp)
    assert L.c8emu_hybrid_call(1, len(nodes), 200, sc.ctypes.data_as(dp), sub.ctypes.data_as(ip), None, 1, 500, ABS_TOL,
                               ABS_TOL, P.ctypes.data_as(dp), act.ctypes.data_as(ip), nn_buf.ctypes.data_as(dp), ptrs) == 0
    assert np.max(np.abs(xi_d[sample] - xi_e)) <= 1e-12 * max(1.0, np.max(np.abs(xi_e)))


# ---- the network catalogue (hybrid_cases.NETS) against the oracle's hybrid class, through the C ABI ----------------------
DEVICE_RUNS = [(n, k, h) for n in ("tanh_1", "relu_zero_bias", "tanh_softening", "tanh_saturated", "sigmoid_saturated")
               for k in ("structured", "notch2D") for h in ("proportional", "hold_unload", "reverse", "nonproportional",
                                                            "unload_reload")] + \
              [("tanh_widest", "structured", h) for h in ("proportional", "reverse")]


@pytest.mark.parametrize("name,kind,history", DEVICE_RUNS)
def test_catalogue_k1_to_k5_and_weight_gradient_against_oracle_on_device(name, kind, history):
    # K1-K5 of the device kernels against the oracle's hybrid class at every step, and the theta tail of
    # c8_param_gradient against the oracle's K5 along theta (the widest network: a sample of theta, see test_emul_hybrid)
    import parity_cases as pc
    from gpu_backend import GpuBackend
    from hybrid_cases import HYB, NETS, assert_allowances, check_purpose, hybrid_oracle, oracle_theta_gradient, theta_sample
    pc.ACTIVE.setdefault(HYB, [0, 1, 2])
    net = NETS[name]
    orc, c, conn = hybrid_oracle(kind, net)
    dut = GpuBackend(3, c, conn, HYB, [E, NU, Y], embedded=net.embedded(), max_iters=500, abs_tol=ABS_TOL, rel_tol=ABS_TOL)
    assert dut.asm.num_embedded_params == len(net.theta)
    used = dict(pc.AUDIT.used)
    pc.check_forward(orc, dut, c, HYB, 0.004, 1e-12, history)
    pc.check_residual(orc, dut, c, 0.004, 1e-12, history)
    idx = theta_sample(net) if name == "tanh_widest" else None
    seen = []

    def theta_check(n, step, z_u, z_p, phi):
        want, scale = oracle_theta_gradient(orc, step, z_u, z_p, phi, idx)
        got = dut.qoi_gradient(*step, z_u, z_p, phi, dut.asm.num_grad_params)[3:]
        got = got if idx is None else got[idx]
        assert np.max(np.abs(got - want)) <= 1e-12 * scale.max(), (n, np.max(np.abs(got - want)) / scale.max())
        seen.append(np.abs(want).max())

    pc.check_adjoint_chain(orc, dut, c, HYB, 0.004, 1e-12, history, k5_hook=theta_check)
    assert_allowances(used, net)
    assert seen and max(seen) > 0.0
    check_purpose(net, kind, history, [x for _, _, x in pc.load_history(orc, c, 0.004, history)])


@pytest.mark.parametrize("npts", [1, 15, 16, 17, 1023, 1024, 1025, 3 * 1024 + 5])
def test_weight_gradient_kernel_at_chunk_and_block_edges_on_device(npts):
    # tri3 has one point per element: a strip of npts triangles; the weight-gradient kernel against autograd of the
    # restated residual (one-layer and two-layer nets), two runs bitwise equal
    import torch
    from hybrid_cases import NETS
    ncell = (npts + 1) // 2
    coords, conn = tri_mesh(ncell, 1)
    conn = np.ascontiguousarray(conn[:npts])
    rng = np.random.default_rng(npts)
    for name in ("tanh_1", "tanh_16_16", "sigmoid_64"):
        net = NETS[name]
        a = hybrid(coords, conn, net.act, net.topo, net.s_in, net.s_out, net.theta)
        assert a.nelems * a.npts == npts
        xi = np.zeros((npts, 1, 6))
        xi[..., 0:3] = rng.normal(0.0, 4e-3, (npts, 1, 3))
        xi[..., 3], xi[..., 4] = 1.0, 1.0
        xi[..., 5] = np.abs(rng.normal(0.0, 0.005, (npts, 1)))
        xi[-1, 0, [0, 1, 2, 5]] = [0.01, 0.003, -0.008, 0.001]  # the last point, alone in its chunk or block, is plastic
        phi = rng.normal(0.0, 1.0, (npts, 1, 6))
        z = a.dev(np.zeros(coords.shape[0] * 2))
        pz = a.dev(np.zeros(coords.shape[0]))
        d_xi, d_phi = a.dev(xi), a.dev(phi)
        grads = []
        for _ in range(2):
            g = a.dev(np.zeros(a.num_grad_params))
            a.qoi_gradient(z, pz, z, pz, d_xi, d_xi, z, pz, d_phi, g)
            torch.cuda.synchronize()
            grads.append(g.cpu().numpy()[1:])
        want = hr.theta_gradient(xi.reshape(npts, 6), phi.reshape(npts, 6), E, NU, Y, net.act, net.topo, net.s_in,
                                 net.s_out, net.theta, ABS_TOL)
        assert np.max(np.abs(want)) > 0.0
        # the bar of the 6000-point test above: the NN(0) term summed per block against per point
        assert np.max(np.abs(grads[0] - want)) <= 1e-11 * np.max(np.abs(want)), (name, npts)
        assert grads[0].tobytes() == grads[1].tobytes()
