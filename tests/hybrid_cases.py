"""TEST INFRASTRUCTURE: meshes, load paths and networks shared by the hybrid_hyper_J2_plane_stress tests."""
import json
import os

import numpy as np

import hybrid_ref as hr

HERE = os.path.dirname(os.path.abspath(__file__))
E, NU, Y = 1000.0, 0.25, 2.0
ABS_TOL = 1e-12


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
