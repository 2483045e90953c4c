"""The oracle's hybrid_hyper_J2_plane_stress (oracle/c8_oracle.cpp, HybridHyperJ2PlaneStress) tied to what is pinned: with a
positive ReLU network it is the oracle's hyper_J2_plane_stress with K = K_eff (pinned to the reference's notch2D deck); its
K1 is the derivative of its own residual for a tanh network; its weight gradient (K5 along theta) is autograd's derivative
of the restated residual (tests/hybrid_ref.py).  These check the oracle itself, not the kernels."""
import numpy as np
import pytest

import hybrid_ref as hr
import oracle_lib as ol
import parity_cases as pc
from fe_driver import block_matrix
from hybrid_cases import ABS_TOL, E, HYB, NETS, NU, Y, Net, check_purpose, hybrid_oracle, linear_relu_net, oracle_theta_gradient

pc.ACTIVE.setdefault(HYB, [0, 1, 2])


class AlphaPrevOracle:
    """the oracle's hyper_J2_plane_stress with every local solve started from alpha = alpha_prev, the hybrid model's
    initial guess; the other unknowns start as the caller's xi"""

    def __init__(self, orc):
        self.orc = orc

    def __getattr__(self, k):
        return getattr(self.orc, k)

    def forward_jacobian(self, u, p, up, pp, xip, xi, ls):
        xi[..., 5] = xip[..., 5]
        return self.orc.forward_jacobian(u, p, up, pp, xip, xi, ls)


class AsDut:
    """an oracle in the device-under-test seat of the parity checks (whose entry points return a status)"""

    def __init__(self, orc):
        self.orc = orc

    def __getattr__(self, k):
        return getattr(self.orc, k)

    def global_residual(self, *a):
        self.orc.global_residual(*a)
        return 0

    def adjoint_jacobian(self, *a):
        self.orc.adjoint_jacobian(*a)
        return 0

    def solve_adjoint_local(self, *a):
        self.orc.solve_adjoint_local(*a)
        return 0


def test_set_embedded_refuses_and_sizes_the_parameters():
    et, c, conn = pc.mesh_2d("structured")
    orc = ol.Oracle(et, c, conn, HYB, [E, NU, Y])
    orc.set_embedded("tanh", [1, 3, 2, 1], 1.0, 1.0)
    assert orc.params.shape == (1, 3 + hr.num_params([1, 3, 2, 1])) and list(orc.params[0, :3]) == [E, NU, Y]
    with pytest.raises(ValueError):
        orc.set_embedded("tanh", [1, 1], 1.0, 1.0)
    other = ol.Oracle(et, c, conn, "hyper_J2_plane_stress", pc.HJ2_PSS)
    with pytest.raises(ValueError):
        other.set_embedded("tanh", [1, 4, 1], 1.0, 1.0)


@pytest.mark.parametrize("history", pc.HISTORIES)
@pytest.mark.parametrize("kind", ["structured", "notch2D"])
def test_linear_relu_network_is_hyper_J2_plane_stress_with_K(kind, history):
    # positive weights and alpha >= 0: s_out (NN(s_in alpha) - NN(0)) = K_eff alpha; K1, K2, K3-K5 (E nu Y) at the bar
    topo, s_in, s_out = [1, 4, 3, 1], 2.0, 5.0
    theta, prod = linear_relu_net(np.random.default_rng(3), topo)
    net = Net("linear", "relu", topo, theta, s_in, s_out)
    hyb, c, conn = hybrid_oracle(kind, net)
    et = ol.TRI3
    ref = AlphaPrevOracle(ol.Oracle(et, c, conn, "hyper_J2_plane_stress", [E, NU, Y, 0, 0, 0, 1, s_in * s_out * prod],
                                    abs_tol=ABS_TOL, rel_tol=ABS_TOL))
    used = dict(pc.AUDIT.used)
    dut = AsDut(hyb)
    pc.check_forward(ref, dut, c, HYB, 0.004, 1e-12, history)
    pc.check_residual(ref, dut, c, 0.004, 1e-12, history)
    pc.check_adjoint_chain(ref, dut, c, HYB, 0.004, 1e-12, history)
    assert dict(pc.AUDIT.used) == used, "no allowance for the hybrid model"
    st = pc.load_history(ref, c, 0.004, history)
    assert max(float(x[..., 5].max()) for _, _, x in st) > 0.0


@pytest.mark.parametrize("name", ["tanh_16_16", "tanh_softening", "tanh_saturated"])
def test_jacobian_matches_finite_differences(name):
    # K1's condensed Jacobian against central differences of the oracle's own residual, from a yielded state
    net = NETS[name]
    orc, c, conn = hybrid_oracle("structured", net)
    st = pc.load_history(orc, c, 0.004, "proportional")
    (u, p, _), (up, pp, xip) = st[2], st[1]

    def resid(uu):
        ls, xi = orc.new_linsys(), orc.new_state()
        assert orc.forward_jacobian(uu, p, up, pp, xip, xi, ls) == 0
        return ls.b[0].copy(), ls, xi

    R, ls, xi = resid(u)
    assert (xi[..., 5] > xip[..., 5]).any()
    A = block_matrix(orc, ls).toarray()[:len(u), :len(u)]
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(6):
        v = rng.standard_normal(len(u))
        v /= np.linalg.norm(v)
        h = 1e-7 * max(1.0, np.abs(u).max())
        fd = (resid(u + h * v)[0] - resid(u - h * v)[0]) / (2 * h)
        worst = max(worst, np.abs(A @ v - fd).max() / np.abs(A @ v).max())
    assert worst < 2e-6, worst


@pytest.mark.parametrize("name", ["tanh_16_16", "sigmoid_8_5_7", "tanh_saturated", "sigmoid_saturated", "tanh_1",
                                  "relu_switching"])
@pytest.mark.parametrize("kind", ["structured", "notch2D"])
def test_theta_gradient_matches_autograd_at_oracle_states(name, kind):
    # K5 along every theta entry (the reference's DFAD gradient) against autograd of the restated residual at the oracle's
    # converged states.  torch's tanh' = 1 - y^2 and sigmoid' = y (1 - y) lose digits in saturation that the oracle's
    # 1/cosh^2 and quotient rule keep, so the bar is the loose one autograd allows there
    net = NETS[name]
    orc, c, conn = hybrid_oracle(kind, net)
    st = pc.load_history(orc, c, 0.004, "reverse")
    rng = np.random.default_rng(5)
    for n in range(1, len(st)):
        (u, p, xi), (up, pp, xip) = st[n], st[n - 1]
        phi = rng.standard_normal(xi.shape)
        z = np.zeros(len(u))
        got, scale = oracle_theta_gradient(orc, (u, p, up, pp, xip, xi), z, np.zeros(len(p)), phi)
        want = hr.theta_gradient(xi.reshape(-1, 6), phi.reshape(-1, 6), E, NU, Y, net.act, net.topo, net.s_in, net.s_out,
                                 net.theta, ABS_TOL)
        tol = 1e-6 if net.purpose == "saturated" else 1e-11
        assert np.abs(want).max() > 0.0
        assert np.max(np.abs(got - want)) <= tol * scale.max(), (n, np.max(np.abs(got - want)) / scale.max())


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(NETS) for k in ("structured", "notch2D")
                                       if not (n == "tanh_widest" and k == "notch2D")])  # as in test_emul_hybrid
def test_catalogue_case_does_what_it_is_there_for(name, kind):
    # the purpose of each catalogue network (hybrid_cases.check_purpose) in exactly the histories it lists, plastic points
    # in the others
    net = NETS[name]
    orc, c, conn = hybrid_oracle(kind, net)
    for h in (pc.HISTORIES if name != "tanh_widest" else ("proportional", "reverse")):
        check_purpose(net, kind, h, [x for _, _, x in pc.load_history(orc, c, 0.004, h)])
