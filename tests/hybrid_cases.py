"""TEST INFRASTRUCTURE: meshes, load paths and networks shared by the hybrid_hyper_J2_plane_stress tests."""
import json
import os

import numpy as np

import hybrid_ref as hr

HERE = os.path.dirname(os.path.abspath(__file__))
E, NU, Y = 1000.0, 0.25, 2.0
ABS_TOL = 1e-12
HYB = "hybrid_hyper_J2_plane_stress"
HISTORIES = ("proportional", "hold_unload", "reverse", "nonproportional", "unload_reload")  # parity_cases.HISTORIES


def tri_mesh(nx, ny):
    xs, ys = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing="ij")
    coords = np.zeros(((nx + 1) * (ny + 1), 3))
    coords[:, 0], coords[:, 1] = xs.ravel(), ys.ravel()
    conn = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = i * (ny + 1) + j, (i + 1) * (ny + 1) + j, (i + 1) * (ny + 1) + j + 1, i * (ny + 1) + j + 1
            conn += [[a, b, c], [a, c, d]]
    return coords, np.array(conn, dtype=np.int32)


def notch2d():
    d = json.load(open(os.path.join(HERE, "golden", "notch2D_tri3.json")))
    return np.array(d["coords"]), np.array(d["conn"], dtype=np.int32), {k: np.array(v, dtype=np.int32) for k, v in d["node_sets"].items()}


def stretch(coords, eps):
    u = np.zeros((coords.shape[0], 2))
    u[:, 0] = eps * coords[:, 0]
    u[:, 1] = -0.3 * eps * coords[:, 1] + 0.5 * eps * coords[:, 0]
    return np.ascontiguousarray(u.ravel())


def linear_relu_net(rng, topology):
    """positive weights and biases: every ReLU unit is active for inputs >= 0; returns theta and W_L ... W_1 W_0"""
    theta = rng.uniform(0.2, 1.0, hr.num_params(topology))
    K = np.eye(1)
    for W, _ in hr.unpack(theta, topology):
        K = W @ K
    return theta, float(K[0, 0])


def dK_dtheta(theta, topology, s_in, s_out):
    """d(s_in s_out W_L ... W_0)/dtheta in theta's order (zero for the biases)"""
    layers = hr.unpack(theta, topology)
    out = []
    for l, (W, b) in enumerate(layers):
        left, right = np.eye(1), np.eye(1)  # W_L ... W_{l+1} (1 x n_{l+1}) and W_{l-1} ... W_0 (n_l x 1)
        for Wm, _ in reversed(layers[l + 1:]):
            left = left @ Wm
        for Wm, _ in layers[:l]:
            right = Wm @ right
        out.append((s_in * s_out * np.outer(left[0], right[:, 0])).ravel())
        out.append(np.zeros(len(b)))
    return np.concatenate(out)


# ---- the network catalogue: nonlinear networks for the parity checks against the oracle's hybrid class -----------------
class Net:
    """one catalogue entry: activation, topology, theta (hybrid_ref order), scales, and `purpose`, the behaviour the case is
    there for (asserted by purpose_reached on the oracle's converged states)"""

    def __init__(self, name, act, topo, theta, s_in, s_out, purpose="plastic", reaches=None):
        """reaches: {mesh kind: the load histories (parity_cases.HISTORIES) in which the purpose is reached}; all of them
        on both meshes by default"""
        self.name, self.act, self.topo, self.s_in, self.s_out, self.purpose = name, act, list(topo), s_in, s_out, purpose
        self.reaches = reaches or {"structured": HISTORIES, "notch2D": HISTORIES}
        self.theta = np.ascontiguousarray(theta, dtype=np.float64)
        assert len(self.theta) == hr.num_params(self.topo)

    def __repr__(self):
        return self.name

    def embedded(self):
        return dict(activation=self.act, topology=self.topo, input_scale=self.s_in, output_scale=self.s_out, params=self.theta)

    def buffer(self):
        return hr.buffer(self.act, self.topo, self.s_in, self.s_out, self.theta)

    def preacts(self, alpha):
        """pre-activations of every hidden layer at the inputs s_in alpha: [layer][point, unit]"""
        act = {"relu": lambda z: np.where(z > 0, z, 0.0), "sigmoid": lambda z: 1.0 / (1.0 + np.exp(-z)), "tanh": np.tanh}
        h, out = self.s_in * np.asarray(alpha, dtype=np.float64).reshape(-1, 1), []
        for W, b in hr.unpack(self.theta, self.topo)[:-1]:
            z = h @ W.T + b
            out.append(z)
            h = act[self.act](z)
        return out

    def hardening_slope(self, alpha):
        """dH/dalpha at alpha (torch autograd, float64)"""
        import torch
        a = torch.tensor(np.asarray(alpha, dtype=np.float64).ravel(), requires_grad=True)
        H = hr.hardening(torch.tensor(self.theta), self.topo, self.act, self.s_in, self.s_out, a)
        H.sum().backward()
        return a.grad.numpy()


def _monotone(rng, topo, w=(0.1, 0.6), b=(0.0, 0.5)):
    """positive weights and biases: for relu, tanh and sigmoid a hardening that rises with alpha and is concave, so the
    local Newton iteration approaches from the plastic side (a convex one overshoots into the elastic branch and cycles)"""
    theta = []
    for i in range(len(topo) - 1):
        n0, n1 = topo[i], topo[i + 1]
        scale = 1.0 / np.sqrt(n0)
        theta += [rng.uniform(w[0], w[1], n0 * n1) * scale, rng.uniform(b[0], b[1], n1)]
    return np.concatenate(theta)


def _catalogue():
    r = lambda s: np.random.default_rng(s)
    out = [Net("tanh_16_16", "tanh", [1, 16, 16, 1], _monotone(r(101), [1, 16, 16, 1]), 200.0, 1.0),
           Net("sigmoid_8_5_7", "sigmoid", [1, 8, 5, 7, 1], _monotone(r(107), [1, 8, 5, 7, 1], b=(-2.0, 2.0)), 300.0, 4.0)]
    # ReLU units that switch along the path.  Units 6..11 of the first layer start on (b > 0, w < 0) and switch off at
    # s_in alpha = 0.1 .. 2.5; they reach the second layer through negative weights, so H rises and stays concave
    topo = [1, 12, 9, 1]
    th = _monotone(r(103), topo, w=(0.2, 1.0), b=(0.2, 0.6))
    (W0, b0), (W1, b1), _ = hr.unpack(th, topo)
    W0[6:, 0] *= -1.0
    b0[6:] = np.linspace(0.1, 2.5, 6) * -W0[6:, 0]
    W1[:, 6:] *= -1.0
    b1[:] += 3.0  # every second-layer unit stays on
    out.append(Net("relu_switching", "relu", topo, th, 500.0, 0.5, "relu_switch"))
    # zero first-layer biases: every unit sits on its kink at alpha = 0, where the reference's slope is 0, so the first
    # Newton iterate from the virgin state is perfectly plastic.  Units with w > 0 switch on for alpha > 0 with negative
    # output weights (a softening H' = -10 that the iterate approaches from the plastic side); those with w < 0 stay off
    topo = [1, 6, 1]
    th = np.zeros(hr.num_params(topo))
    (W0, b0), (W1, b1) = hr.unpack(th, topo)
    W0[:, 0] = [0.5, -0.7, 0.9, -0.4, 0.3, -1.1]
    W1[0, :] = [-0.4, 0.8, -0.3, 0.6, 0.5, 0.9]
    b1[:] = 0.3
    W1[0, :] *= 10.0 / (100.0 * abs(np.sum(np.where(W0[:, 0] > 0, W0[:, 0] * W1[0, :], 0.0))))
    out.append(Net("relu_zero_bias", "relu", topo, th, 100.0, 1.0, "virgin_plastic"))
    # one hidden layer: the degenerate layer loop and theta offsets
    out.append(Net("tanh_1", "tanh", [1, 1, 1], np.array([0.7, 0.1, 1.3, -0.2]), 300.0, 2.0))
    out.append(Net("sigmoid_64", "sigmoid", [1, 64, 1], _monotone(r(105), [1, 64, 1]), 400.0, 4.0))
    # the widest network (LDS work buffer at NN_MAX_WIDTH) and mixed widths
    out.append(Net("tanh_widest", "tanh", [1, 64, 64, 64, 64, 1], _monotone(r(106), [1, 64, 64, 64, 64, 1]), 200.0, 1.0))
    out.append(Net("tanh_asym", "tanh", [1, 3, 64, 2, 64, 1], _monotone(r(107), [1, 3, 64, 2, 64, 1]), 200.0, 1.0))
    # softening: NN(x) = tanh(x) - 1.5 tanh(x - 1.5) + two small units has a maximum near x = 0.6 and is concave up to
    # x = 1.5; |H'| <= 1.6 s_in s_out << 3 mu
    topo = [1, 4, 1]
    th = np.zeros(hr.num_params(topo))
    (W0, b0), (W1, b1) = hr.unpack(th, topo)
    W0[:, 0], b0[:] = [1.0, 1.0, 0.1, 0.2], [0.0, -1.5, 0.3, 0.1]
    W1[0, :], b1[:] = [1.0, -1.5, 0.05, 0.03], [0.2]
    out.append(Net("tanh_softening", "tanh", topo, th, 100.0, 0.5, "softening",
                   {"structured": ("reverse",), "notch2D": ("proportional", "reverse", "nonproportional", "unload_reload")}))
    # saturated first layers: |z| > 8 at plastic points, where 1 - a^2 and a (1 - a) keep only a few digits.  The output
    # weights (~3e3) also scale the rounding of NN ~ sum W a that two evaluation orders leave in H; larger ones would let
    # that rounding move the converged alpha beyond the parity bar
    topo = [1, 6, 1]
    for name, act, bias in (("tanh_saturated", "tanh", (8.2, 8.6)), ("sigmoid_saturated", "sigmoid", (14.2, 14.6))):
        th = np.zeros(hr.num_params(topo))
        (W0, b0), (W1, b1) = hr.unpack(th, topo)
        rng = r(108 if act == "tanh" else 109)
        W0[:, 0], b0[:] = rng.uniform(0.2, 0.4, 6), rng.uniform(*bias, 6)
        W1[0, :], b1[:] = rng.uniform(2e3, 4e3, 6), [0.5]
        out.append(Net(name, act, topo, th, 300.0, 1.0, "saturated"))
    return {n.name: n for n in out}


NETS = _catalogue()


def check_purpose(net, kind, history, states):
    """the catalogue entry's purpose is reached in exactly the histories net.reaches names for the mesh `kind`; in the
    others the case still has plastic points"""
    if history in net.reaches[kind]:
        return purpose_reached(net, states)
    try:
        seen = purpose_reached(net, states)
    except AssertionError as e:
        assert "no plastic point" not in str(e), e
        return "plastic, purpose not reached (as listed)"
    raise AssertionError("%s on %s, %s: the purpose is reached (%s) but not listed in reaches" % (net.name, kind, history, seen))


def purpose_reached(net, states):
    """states: [xi_0, xi_1, ...] converged local states of consecutive steps (alpha is xi[..., 5]).  Asserts that the case
    does what it is in the catalogue for; returns a short description of what was seen."""
    a = [np.asarray(x)[..., 5].ravel() for x in states]
    plastic = [(a[n] > a[n - 1]) for n in range(1, len(a))]
    assert any(p.any() for p in plastic), "%s: no plastic point" % net.name
    if net.purpose == "relu_switch":
        flips = 0
        for n in range(1, len(a)):
            for z0, z1 in zip(net.preacts(a[n - 1]), net.preacts(a[n])):
                flips += int(((z0 > 0) != (z1 > 0)).sum())
        assert flips > 0, "%s: no ReLU unit switched between steps" % net.name
        return "%d unit switches" % flips
    if net.purpose == "virgin_plastic":
        assert np.all(a[0] == 0.0) and plastic[0].any(), "%s: the step from the virgin state must be plastic" % net.name
        return "%d plastic points from the virgin state" % plastic[0].sum()
    if net.purpose == "softening":
        slopes = np.concatenate([net.hardening_slope(a[n][p]) for n, p in enumerate(plastic, start=1) if p.any()])
        assert slopes.min() < 0.0, "%s: no converged plastic point on the softening branch" % net.name
        assert np.abs(slopes).max() < 0.5 * 3.0 * E / (2.0 * (1.0 + NU))
        return "min H' %.3g" % slopes.min()
    if net.purpose == "saturated":
        z = np.concatenate([np.abs(net.preacts(a[n][p])[0]).ravel() for n, p in enumerate(plastic, start=1) if p.any()])
        assert z.min() > 8.0, "%s: first layer not saturated (min |z| %.3g)" % (net.name, z.min())
        return "min |z| %.3g" % z.min()
    return "%d plastic points" % sum(int(p.sum()) for p in plastic)


def hybrid_oracle(kind_or_mesh, net, **kw):
    """the oracle's hybrid_hyper_J2_plane_stress with the network `net` on pc.mesh_2d(kind), or on (et, coords, conn)"""
    import oracle_lib as ol
    import parity_cases as pc
    et, c, conn = pc.mesh_2d(kind_or_mesh) if isinstance(kind_or_mesh, str) else kind_or_mesh
    kw.setdefault("abs_tol", ABS_TOL)
    kw.setdefault("rel_tol", ABS_TOL)
    return ol.Oracle(et, c, conn, "hybrid_hyper_J2_plane_stress", [E, NU, Y], embedded=net.embedded(), **kw), c, conn


def oracle_theta_gradient(orc, step, z_u, z_p, phi, idx=None, restore=(0, 1, 2)):
    """the oracle's K5 along the theta entries idx (all by default), made active at most 32 at a time (the oracle's Fad
    width): returns (grad, scale), scale as qoi_gradient_with_scale.  The active set `restore` is set again afterwards."""
    nt = orc.params.shape[1] - 3
    idx = np.arange(nt) if idx is None else np.asarray(idx)
    g, s = np.zeros(len(idx)), np.zeros(len(idx))
    for k in range(0, len(idx), 32):
        chunk = idx[k:k + 32]
        orc.set_active(0, 3 + chunk)
        g[k:k + 32], s[k:k + 32] = orc.qoi_gradient_with_scale(*step, z_u, z_p, phi, len(chunk))
    orc.set_active(0, list(restore))
    return g, s


def theta_sample(net):
    """the theta entries the oracle checks for the widest network, whose 12673 entries would take ~400 oracle K5 passes
    per step: the first and the last 32 entries of every weight matrix and bias vector"""
    out, o = [], 0
    for W, b in hr.unpack(net.theta, net.topo):
        for n in (W.size, b.size):
            out += list(range(o, o + min(n, 32))) + list(range(max(o, o + n - 32), o + n))
            o += n
    return np.unique(out)


def assert_allowances(before, net):
    """no allowance of the parity checker for the hybrid model (counted in parity_cases.AUDIT since `before`), except
    `at_state` (the Jacobian within the bar at the device's own converged state) for the saturated networks: there the
    rounding of NN ~ sum W a, which two evaluation orders leave in H, moves the converged alpha by ~1e-13 and the
    Jacobian, which follows alpha, by up to 4e-11; at the same state the two agree to 1e-15"""
    import parity_cases as pc
    new = {k: v - before.get(k, 0) for k, v in pc.AUDIT.used.items() if v != before.get(k, 0)}
    ok = ("at_state",) if net.purpose == "saturated" else ()
    assert all(k.split("|")[-1] in ok for k in new), new
