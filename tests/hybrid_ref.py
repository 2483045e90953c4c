"""TEST INFRASTRUCTURE: hybrid_hyper_J2_plane_stress restated from its equations in float64 torch on the CPU.

The feed-forward network (hidden layers act(W x + b), a linear last layer; theta = W_0, b_0, W_1, b_1, ... with W_i
row-major) and the theta-dependent row of the local residual on the unforced plastic path,
    R_alpha = (|s| - sqrt(2/3) (Y + s_out (NN(s_in alpha) - NN(0)))) / mu,   s = mu zeta_3D,  zeta_zz = -(zeta_00 + zeta_11),
whose theta derivative autograd gives."""
import numpy as np
import torch

ACT = {"relu": lambda z: torch.where(z > 0, z, torch.zeros_like(z)), "sigmoid": torch.sigmoid, "tanh": torch.tanh}
ACT_ID = {"relu": 0, "sigmoid": 1, "tanh": 2}


def num_params(topology):
    return sum(topology[i + 1] * (topology[i] + 1) for i in range(len(topology) - 1))


def unpack(theta, topology):
    """[(W_i, b_i)] views of theta in the reference's order"""
    out, o = [], 0
    for i in range(len(topology) - 1):
        n0, n1 = topology[i], topology[i + 1]
        W = theta[o:o + n0 * n1].reshape(n1, n0)
        o += n0 * n1
        b = theta[o:o + n1]
        o += n1
        out.append((W, b))
    return out


def nn(theta, topology, act, x):
    """NN at the inputs x (shape [n]); returns shape [n]"""
    h = x.reshape(-1, 1)
    layers = unpack(theta, topology)
    for i, (W, b) in enumerate(layers):
        h = h @ W.T + b
        if i < len(layers) - 1:
            h = ACT[act](h)
    return h[:, 0]


def buffer(act, topology, s_in, s_out, theta):
    """the device buffer of c8_models.hpp (nn_value_slope) with NN(0)"""
    hdr = np.zeros(16)
    hdr[0], hdr[1] = ACT_ID[act], len(topology)
    hdr[2:2 + len(topology)] = topology
    hdr[10], hdr[11] = s_in, s_out
    t = torch.tensor(theta, dtype=torch.float64)
    hdr[12] = float(nn(t, topology, act, torch.zeros(1, dtype=torch.float64))[0])
    return np.ascontiguousarray(np.concatenate([hdr, theta]))


def hardening(theta, topology, act, s_in, s_out, alpha):
    zero = torch.zeros(1, dtype=torch.float64)
    return s_out * (nn(theta, topology, act, s_in * alpha) - nn(theta, topology, act, zero))


def theta_gradient(xi, phi, E, nu, Y, act, topology, s_in, s_out, theta, abs_tol):
    """sum over the points of phi^T dC/dtheta at the stored states xi [npts][6] (zeta 00 01 11, Ie, lambda_z, alpha)"""
    xi = torch.tensor(np.asarray(xi).reshape(-1, 6), dtype=torch.float64)
    phi = torch.tensor(np.asarray(phi).reshape(-1, 6), dtype=torch.float64)
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    mu = E / (2.0 * (1.0 + nu))
    z00, z01, z11, alpha = xi[:, 0], xi[:, 1], xi[:, 2], xi[:, 5]
    zzz = -(z00 + z11)
    s_mag = mu * torch.sqrt(z00 ** 2 + 2.0 * z01 ** 2 + z11 ** 2 + zzz ** 2)
    f = (s_mag - np.sqrt(2.0 / 3.0) * (Y + hardening(th, topology, act, s_in, s_out, alpha))) / mu
    plastic = (f.detach() > abs_tol) | (f.detach().abs() < abs_tol)
    (phi[:, 5] * torch.where(plastic, f, torch.zeros_like(f))).sum().backward()
    return th.grad.numpy()
