"""hybrid_hyper_J2_plane_stress on the CPU lane emulator (tests/emul_hybrid): the lane-group kernels against the
emulated hyper_J2_plane_stress through the linear-network identity, and the weight-gradient kernel against autograd of
the restated residual (tests/hybrid_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import emul_lib as el
import hybrid_ref as hr
import oracle_lib as ol
import parity_cases as pc
from hybrid_cases import (ABS_TOL, E, HYB, NETS, NU, Y, assert_allowances, check_purpose, dK_dtheta, hybrid_oracle,
                          linear_relu_net, oracle_theta_gradient, stretch, theta_sample, tri_mesh)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
REL_TOL = 1e-12
pc.ACTIVE.setdefault(HYB, [0, 1, 2])  # E nu Y: the same indices in the hybrid model and in hyper_J2_plane_stress


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/emul_hybrid/c8_emul_hybrid.cpp, built afresh for this session into its own temporary directory"""
    out = str(tmp_path_factory.mktemp("c8_emul_hybrid"))
    so = os.path.join(out, "libc8emul_hybrid.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(ROOT, "tests", "emul_hybrid", "c8_emul_hybrid.cpp"),
                           os.path.join(ROOT, "calibr8_amd", "csrc", "c8_host.cpp")])
    L = C.CDLL(so)
    L.c8emu_hybrid_call.restype = C.c_int
    L.c8emu_hybrid_call.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, ip, C.c_int, C.c_int, C.c_double, C.c_double, dp, ip,
                                    dp, C.POINTER(dp)]
    L.c8emu_nn_grad.restype = C.c_int
    L.c8emu_nn_grad.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, dp, dp, dp, ip, dp, C.c_int, dp]
    L.c8emu_nn_hardening.restype = None
    L.c8emu_nn_hardening.argtypes = [dp, C.c_double, dp]
    return L


class HybridEmul(el.Emul):
    """el.Emul with the hybrid kernels: the oracle object only supplies the graph and the state shapes"""

    def __init__(self, emu, coords, conn, nnbuf, et=ol.TRI3):
        super().__init__(et, coords, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 1, 0], abs_tol=ABS_TOL,
                         rel_tol=REL_TOL)
        self.emu, self.nnbuf = emu, np.ascontiguousarray(nnbuf)
        self.params = np.ascontiguousarray([[E, NU, Y]])

    def _call(self, what, ptrs):
        o = self.orc
        arr = (dp * 18)()
        for k, a in ptrs.items():
            arr[k] = a.ctypes.data_as(dp)
        return self.emu.c8emu_hybrid_call(what, o.nnodes, o.nelems, o.coords.ctypes.data_as(dp), o.conn.ctypes.data_as(ip),
                                          None, o.nsets, self.max_iters, self.abs_tol, self.rel_tol,
                                          self.params.ctypes.data_as(dp), self.active.ctypes.data_as(ip),
                                          self.nnbuf.ctypes.data_as(dp), arr)


@pytest.mark.parametrize("eps", [0.004, 0.02])
def test_linear_relu_network_equals_hyper_J2_plane_stress_with_K(emu, eps):
    # positive weights and alpha >= 0: every unit is active and s_out (NN(s_in alpha) - NN(0)) = K_eff alpha exactly
    rng = np.random.default_rng(3)
    topo, s_in, s_out = [1, 4, 3, 1], 2.0, 5.0
    theta, prod = linear_relu_net(rng, topo)
    K_eff = s_in * s_out * prod
    coords, conn = tri_mesh(3, 2)
    hyb = HybridEmul(emu, coords, conn, hr.buffer("relu", topo, s_in, s_out, theta))
    ref = el.Emul(ol.TRI3, coords, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 0, K_eff], abs_tol=ABS_TOL,
                  rel_tol=REL_TOL)
    u0 = np.zeros(coords.shape[0] * 2)
    xi0 = ref.new_state()
    out = {}
    for name, m in (("hyb", hyb), ("ref", ref)):
        u, xi_prev = stretch(coords, eps), xi0.copy()
        steps = []
        up = u0
        for s in (1, 2):  # two loading steps from the virgin state; the second starts from the first's state
            us = stretch(coords, eps * s)
            xi = xi_prev.copy()  # alpha = alpha_prev: the guess of both models
            ls = m.new_linsys()
            pz = np.zeros(coords.shape[0])
            rc = m.forward_jacobian(us, pz, up, pz, xi_prev, xi, ls)
            assert rc == 0
            steps.append((ls.b[0].copy(), ls.A[0][0].copy(), xi.copy()))
            xi_prev, up = xi, us
        out[name] = steps
    assert np.max(out["ref"][1][2][..., 5]) > 0.0, "the case must reach the plastic branch"
    for (bh, Ah, xh), (br, Ar, xr) in zip(out["hyb"], out["ref"]):
        assert np.max(np.abs(bh - br)) <= 1e-12 * max(1.0, np.max(np.abs(br)))
        assert np.max(np.abs(Ah - Ar)) <= 1e-12 * np.max(np.abs(Ar))
        assert np.max(np.abs(xh - xr)) <= 1e-12


@pytest.mark.parametrize("act,topo", [("tanh", [1, 16, 16, 1]), ("sigmoid", [1, 8, 5, 7, 1]), ("relu", [1, 12, 9, 1]),
                                      ("tanh", [1, 64, 64, 64, 64, 1])])
def test_weight_gradient_kernel_matches_autograd(emu, act, topo):
    rng = np.random.default_rng(11)
    nt = hr.num_params(topo)
    theta = rng.normal(0.0, 0.6, nt)
    s_in, s_out = 3.0, 4.0
    buf = hr.buffer(act, topo, s_in, s_out, theta)
    npts = 2500  # three blocks, the last one partial
    xi = np.zeros((npts, 6))
    xi[:, 0:3] = rng.normal(0.0, 4e-3, (npts, 3))
    xi[:, 3], xi[:, 4] = 1.0, 1.0
    xi[:, 5] = np.abs(rng.normal(0.0, 0.05, npts))
    phi = rng.normal(0.0, 1.0, (npts, 6))
    P = np.ascontiguousarray([E, NU, Y])
    got = np.zeros(nt)
    emu.c8emu_nn_grad(npts, 1, 6, 3, ABS_TOL, buf.ctypes.data_as(dp), xi.ctypes.data_as(dp), phi.ctypes.data_as(dp), None,
                      P.ctypes.data_as(dp), nt, got.ctypes.data_as(dp))
    want = hr.theta_gradient(xi, phi, E, NU, Y, act, topo, s_in, s_out, theta, ABS_TOL)
    # the case has both branches: the restated yield value f on either side of the tolerance band
    H = np.array([float(v) for v in hr.hardening(torch.tensor(theta), topo, act, s_in, s_out, torch.tensor(xi[:, 5]))])
    mu = E / (2.0 * (1.0 + NU))
    zzz = -(xi[:, 0] + xi[:, 2])
    f = (mu * np.sqrt(xi[:, 0] ** 2 + 2 * xi[:, 1] ** 2 + xi[:, 2] ** 2 + zzz ** 2) - np.sqrt(2.0 / 3.0) * (Y + H)) / mu
    plastic = (f > ABS_TOL) | (np.abs(f) < ABS_TOL)
    assert 0.02 * npts < plastic.sum() < 0.98 * npts, plastic.sum()
    assert np.max(np.abs(want)) > 0.0
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_theta_order_and_hardening_match_a_hand_built_network(emu):
    # topology [1, 2, 3, 1]: W0 (2x1), b0 (2), W1 (3x2, row-major), b1 (3), W2 (1x3), b2 (1)
    W0, b0 = np.array([0.5, -1.0]), np.array([0.1, 0.2])
    W1, b1 = np.array([[1.0, 2.0], [-0.5, 0.3], [0.7, -0.2]]), np.array([0.05, -0.1, 0.2])
    W2, b2 = np.array([0.4, -0.6, 0.9]), np.array([0.3])
    theta = np.concatenate([W0, b0, W1.ravel(), b1, W2, b2])
    topo, s_in, s_out = [1, 2, 3, 1], 1.5, 2.5

    def net(x):
        h1 = np.tanh(W0 * x + b0)
        h2 = np.tanh(W1 @ h1 + b1)
        return float(W2 @ h2 + b2[0])

    buf = hr.buffer("tanh", topo, s_in, s_out, theta)
    for alpha in (0.0, 0.03, 0.7):
        h = np.zeros(2)
        emu.c8emu_nn_hardening(buf.ctypes.data_as(dp), alpha, h.ctypes.data_as(dp))
        assert abs(h[0] - s_out * (net(s_in * alpha) - net(0.0))) <= 1e-14
        d = 1e-6
        fd = s_out * (net(s_in * (alpha + d)) - net(s_in * (alpha - d))) / (2 * d)
        assert abs(h[1] - fd) <= 1e-8


class AlphaPrevOracle:
    """the oracle's hyper_J2_plane_stress with every local solve started from alpha = alpha_prev, the initial guess of
    the hybrid model (hybrid_hyper_J2_plane_stress.cpp:256-259); the other unknowns start as the caller's xi"""

    def __init__(self, orc):
        self.orc = orc

    def __getattr__(self, k):
        return getattr(self.orc, k)

    def forward_jacobian(self, u, p, up, pp, xip, xi, ls):
        xi[..., 5] = xip[..., 5]
        return self.orc.forward_jacobian(u, p, up, pp, xip, xi, ls)


class AlphaPrevEmul(el.Emul):
    def forward_jacobian(self, u, p, up, pp, xip, xi, ls):
        xi[..., 5] = xip[..., 5]
        return super().forward_jacobian(u, p, up, pp, xip, xi, ls)


def identity_pair(emu, kind, topo=(1, 4, 3, 1), s_in=2.0, s_out=5.0, seed=3):
    """(oracle hyper_J2_plane_stress with K = K_eff, hybrid emulator with the linear ReLU net, coords, theta)"""
    theta, prod = linear_relu_net(np.random.default_rng(seed), list(topo))
    et, c, conn = pc.mesh_2d(kind)
    orc = AlphaPrevOracle(ol.Oracle(et, c, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 1, s_in * s_out * prod],
                                    abs_tol=ABS_TOL, rel_tol=REL_TOL))
    dut = HybridEmul(emu, c, conn, hr.buffer("relu", list(topo), s_in, s_out, theta), et)
    return orc, dut, c, theta


@pytest.mark.parametrize("history", pc.HISTORIES)
@pytest.mark.parametrize("kind", ["structured", "notch2D"])
def test_linear_network_identity_k1_to_k5_against_oracle(emu, kind, history):
    # K1 (forward), K2 (residual), K3-K6 (adjoint chain, K5 along E nu Y) of the hybrid kernels against the oracle's
    # hyper_J2_plane_stress with S = D = A = 0 and K = K_eff, every step of the history, at the parity bar
    orc, dut, c, _ = identity_pair(emu, kind)
    pc.check_forward(orc, dut, c, HYB, 0.004, 1e-12, history)
    pc.check_residual(orc, dut, c, 0.004, 1e-12, history)
    pc.check_adjoint_chain(orc, dut, c, HYB, 0.004, 1e-12, history)
    st = pc.load_history(orc, c, 0.004, history)
    assert max(float(x[..., 5].max()) for _, _, x in st) > 0.0, "the plastic branch must run"


@pytest.mark.parametrize("history", ["proportional", "reverse", "unload_reload"])
@pytest.mark.parametrize("kind", ["structured", "notch2D"])
def test_linear_network_weight_gradient_is_grad_K_times_dK_dtheta(emu, kind, history):
    # the weight-gradient kernel against the oracle's dJ/dK (= phi^T dC/dK) times dK_eff/dtheta, at every step
    topo, s_in, s_out = [1, 4, 3, 1], 2.0, 5.0
    orc, dut, c, theta = identity_pair(emu, kind, topo, s_in, s_out)
    st = pc.load_history(orc, c, 0.004, history)
    dK = dK_dtheta(theta, topo, s_in, s_out)
    rng = np.random.default_rng(17)
    orc.set_active(0, [7])
    nt = hr.num_params(topo)
    seen = 0.0
    for n in range(1, len(st)):
        (u, p, xi), (up, pp, xip) = st[n], st[n - 1]
        phi = rng.standard_normal((orc.nelems, orc.npts, orc.nloc))
        z_u, z_p = np.zeros(len(u)), np.zeros(len(p))
        gK, scale = orc.qoi_gradient_with_scale(u, p, up, pp, xip, xi, z_u, z_p, phi, 1)
        got = np.zeros(nt)
        P = np.ascontiguousarray([E, NU, Y])
        xic, phic = np.ascontiguousarray(xi), np.ascontiguousarray(phi)
        emu.c8emu_nn_grad(orc.nelems * orc.npts, orc.npts, 6, 3, ABS_TOL, dut.nnbuf.ctypes.data_as(dp),
                          xic.ctypes.data_as(dp), phic.ctypes.data_as(dp), None, P.ctypes.data_as(dp), nt,
                          got.ctypes.data_as(dp))
        want = gK[0] * dK
        assert np.max(np.abs(got - want)) <= 1e-12 * max(float(scale[0]), 1e-300) * np.max(np.abs(dK)), (n, got, want)
        seen = max(seen, abs(gK[0]))
    assert seen > 0.0


@pytest.mark.parametrize("act,topo", [("tanh", [1, 16, 16, 1]), ("sigmoid", [1, 8, 5, 1]), ("relu", [1, 12, 9, 1])])
def test_converged_state_satisfies_the_restated_hardening(emu, act, topo):
    # K1's converged alpha on a path through yield: on plastic points the restated R_alpha (with the network, including
    # ReLU units that are inactive) vanishes to the local tolerance, on elastic points alpha = alpha_prev
    rng = np.random.default_rng(23)
    theta = rng.normal(0.0, 0.5, hr.num_params(topo))
    if act == "relu":  # some units inactive, a hardening that still rises
        theta = np.abs(theta)
        for W, b in hr.unpack(theta, topo)[:-1]:
            b[::2] = -np.abs(b[::2]) - 2.0
    s_in, s_out = 4.0, 20.0 if act != "relu" else 2.0
    c, conn = tri_mesh(6, 5)
    dut = HybridEmul(emu, c, conn, hr.buffer(act, topo, s_in, s_out, theta))
    mu = E / (2.0 * (1.0 + NU))
    xip = dut.new_state()
    up = np.zeros(c.shape[0] * 2)
    pz = np.zeros(c.shape[0])
    nplastic = 0
    for s, eps in enumerate((0.006, 0.012, 0.004, 0.016), start=1):
        u = stretch(c, eps)
        xi = dut.new_state()
        assert dut.forward_jacobian(u, pz, up, pz, xip, xi, dut.new_linsys()) == 0
        x, a = xi.reshape(-1, 6), xi.reshape(-1, 6)[:, 5]
        ap = xip.reshape(-1, 6)[:, 5]
        H = hr.hardening(torch.tensor(theta), topo, act, s_in, s_out, torch.tensor(a)).numpy()
        zzz = -(x[:, 0] + x[:, 2])
        f = (mu * np.sqrt(x[:, 0] ** 2 + 2 * x[:, 1] ** 2 + x[:, 2] ** 2 + zzz ** 2) - np.sqrt(2.0 / 3.0) * (Y + H)) / mu
        moved = a > ap
        nplastic += int(moved.sum())
        assert np.all(np.abs(f[moved]) < 1e-10), (s, np.abs(f[moved]).max())
        assert np.all(f[~moved] < 1e-10)
        xip, up = xi, u
    assert nplastic > 0


# ---- the network catalogue (hybrid_cases.NETS) against the oracle's hybrid class ------------------------------------------
def emul_theta_gradient(emu, net, xi, phi, npts=None):
    """c8emu_nn_grad over the first npts points of xi / phi ([..., 6]): the weight-gradient kernel, block after block"""
    xi = np.ascontiguousarray(np.asarray(xi).reshape(-1, 6))
    phi = np.ascontiguousarray(np.asarray(phi).reshape(-1, 6))
    npts = len(xi) if npts is None else npts
    buf = net.buffer()
    P = np.ascontiguousarray([E, NU, Y])
    got = np.zeros(len(net.theta))
    assert emu.c8emu_nn_grad(npts, 1, 6, 3, ABS_TOL, buf.ctypes.data_as(dp), xi.ctypes.data_as(dp),
                             phi.ctypes.data_as(dp), None, P.ctypes.data_as(dp), len(got), got.ctypes.data_as(dp)) == 0
    return got


# every catalogue network on both meshes and all five histories; the widest on the structured mesh with two histories
# (the oracle evaluates its 12673 weights in forward-mode AD, ~40 s per history there)
CATALOGUE_RUNS = [(n, k, h) for n in sorted(NETS) if n != "tanh_widest" for k in ("structured", "notch2D")
                  for h in pc.HISTORIES] + [("tanh_widest", "structured", h) for h in ("proportional", "reverse")]


@pytest.mark.parametrize("name,kind,history", CATALOGUE_RUNS)
def test_catalogue_k1_to_k5_and_weight_gradient_against_oracle(emu, name, kind, history):
    # K1 (forward), K2 (residual), K3-K6 (adjoint chain, K5 along E nu Y) of the hybrid kernels against the oracle's hybrid
    # class, every step, at 1e-12 with no allowance; at every step of the chain the weight-gradient kernel with the chain's
    # phi against the oracle's K5 along theta
    net = NETS[name]
    orc, c, conn = hybrid_oracle(kind, net)
    et = pc.mesh_2d(kind)[0]
    dut = HybridEmul(emu, c, conn, net.buffer(), et)
    used = dict(pc.AUDIT.used)
    pc.check_forward(orc, dut, c, HYB, 0.004, 1e-12, history)
    pc.check_residual(orc, dut, c, 0.004, 1e-12, history)
    idx = theta_sample(net) if name == "tanh_widest" else None
    seen = []

    def theta_check(n, step, z_u, z_p, phi):
        want, scale = oracle_theta_gradient(orc, step, z_u, z_p, phi, idx)
        got = emul_theta_gradient(emu, net, step[5], phi)
        got = got if idx is None else got[idx]
        # the bar of the linear-network test: 1e-12 of the largest sum of product magnitudes (the kernel adds the NN(0)
        # term once per block, the oracle once per point)
        assert np.max(np.abs(got - want)) <= 1e-12 * scale.max(), (n, np.max(np.abs(got - want)) / scale.max())
        seen.append(np.abs(want).max())

    pc.check_adjoint_chain(orc, dut, c, HYB, 0.004, 1e-12, history, k5_hook=theta_check)
    assert_allowances(used, net)
    st = pc.load_history(orc, c, 0.004, history)
    assert len(seen) == len(st) - 1 and max(seen) > 0.0
    check_purpose(net, kind, history, [x for _, _, x in st])


@pytest.mark.parametrize("npts", [1, 15, 16, 17, 1023, 1024, 1025, 3 * 1024 + 5])
@pytest.mark.parametrize("name", ["tanh_16_16", "tanh_1", "sigmoid_64", "sigmoid_8_5_7"])
def test_weight_gradient_at_chunk_and_block_edges(emu, name, npts):
    # the kernel's chunks of 16 points and blocks of 1024 against autograd of the restated residual (non-saturated nets),
    # and two runs bitwise equal
    net = NETS[name]
    rng = np.random.default_rng(npts)
    xi = np.zeros((npts, 6))
    xi[:, 0:3] = rng.normal(0.0, 4e-3, (npts, 3))
    xi[:, 3], xi[:, 4] = 1.0, 1.0
    xi[:, 5] = np.abs(rng.normal(0.0, 0.005, npts))
    xi[-1, [0, 1, 2, 5]] = [0.01, 0.003, -0.008, 0.001]  # the last point, alone in its chunk or block, is plastic
    phi = rng.normal(0.0, 1.0, (npts, 6))
    got = emul_theta_gradient(emu, net, xi, phi)
    assert got.tobytes() == emul_theta_gradient(emu, net, xi, phi).tobytes()
    want = hr.theta_gradient(xi, phi, E, NU, Y, net.act, net.topo, net.s_in, net.s_out, net.theta, ABS_TOL)
    assert np.max(np.abs(want)) > 0.0
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1, npts / 1024) * np.max(np.abs(want)) * 10, np.max(np.abs(got - want)) / np.max(np.abs(want))
    # the last point alone decides the partial chunk / block: dropping it changes the result unless it is elastic
    if npts > 1:
        rest = emul_theta_gradient(emu, net, xi, phi, npts - 1)
        last = hr.theta_gradient(xi[-1:], phi[-1:], E, NU, Y, net.act, net.topo, net.s_in, net.s_out, net.theta, ABS_TOL)
        assert np.max(np.abs(got - rest - last)) <= 1e-11 * np.max(np.abs(want))
