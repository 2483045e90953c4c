"""Shared set-up of the VFM tests (test_vfm_emul.py on the lane emulator, test_gpu_vfm.py on the device): meshes, measured
steps, the virtual field, and the oracle compositions the VFM kernels must reproduce (no change to the oracle)."""
import numpy as np

import oracle_lib as ol
from meshes import fields_for, prescribed_fields
from parity_cases import ACTIVE, HILL_PS, HJ2_PSS, HYPO_PSS, mesh_2d

MODELS = [("small_hill_plane_stress", HILL_PS), ("hyper_J2_plane_stress", HJ2_PSS), ("hypo_hill_plane_stress", HYPO_PSS)]
STRETCH = [0.0, 1.0, 1.5, 2.0, 2.4]  # measured u_n = STRETCH[n] u_1: four steps, into the plastic range
CYCLIC = [0.0, 1.5, 1.5, 0.8, -0.6, -1.2]  # a cyclic measured sequence: yield, hold, unloading, reversed plastic flow


def vfm_case(mesh, model, params, seq=None):
    """(coords, conn, elem_set or None, params [sets][n], active per set, measured steps u_n = seq[n] u_1 (STRETCH), w)"""
    et, c, conn = mesh_2d("notch2D" if mesh == "notch2D" else "structured")
    act = ACTIVE[model]
    if mesh == "notch2D":
        es, P, active = None, np.atleast_2d(np.array(params, dtype=float)), [act[:3]]
    else:  # two element sets with different parameters and different active lists
        es = (c[conn].mean(axis=1)[:, 0] > 0.5).astype(np.int32)
        p1 = np.array(params, dtype=float)
        p1[2] *= 1.3
        P, active = np.vstack([params, p1]), [act[:3], act[2:5]]
    u1, _ = fields_for(2, *prescribed_fields(c, 0.004, ramp=True, perturb=5e-2))
    steps = [s * u1 for s in (STRETCH if seq is None else seq)]
    x, y = c[:, 0], c[:, 1]
    w = np.ascontiguousarray(np.stack([np.cos(np.pi * (y - 0.5)) * x + 0.2 * y, y * y + 0.1 * x], axis=1).ravel())
    return c, conn, es, P, active, steps, w


def make_oracle(c, conn, model, P, es, active):
    orc = ol.Oracle(ol.TRI3, c, conn, model, P, elem_set=es)
    for s, a in enumerate(active):
        orc.set_active(s, a)
    return orc


def oracle_power(orc, u, up, xip):
    """xi_n and R from eval_forward_jacobian (the oracle's local solve; R assembled into ls.b)"""
    p0 = np.zeros(orc.nnodes)
    xi, ls = xip.copy(), orc.new_linsys()
    rc = orc.forward_jacobian(u, p0, up, p0, xip, xi, ls)
    return rc, xi, ls.b[0].copy()


def oracle_adjoint_step(orc, u, up, xip, xi, w, c, h, nact):
    """the VFM adjoint step as solve_adjoint_local(z = c w, g = -h) + qoi_gradient(z = c w, phi) under "average
    displacement" (dJ/dp = dJ/dxi = 0): (h_new, grad, grad_abs)"""
    p0 = np.zeros(orc.nnodes)
    phi = np.zeros((orc.nelems, orc.npts, orc.nloc))
    g = -np.asarray(h, dtype=float).reshape(orc.nelems, orc.npts, orc.nloc).copy()
    f = np.zeros((orc.nelems, orc.npts, orc.ndofs))
    z = c * w
    orc.solve_adjoint_local(u, p0, up, p0, xip, xi, z, p0, phi, g, f)
    grad, gabs = orc.qoi_gradient_with_scale(u, p0, up, p0, xip, xi, z, p0, phi, nact)
    return -g.ravel(), grad, gabs


def objective(ivw, loads, dt_over_T, scale, thickness):
    m = thickness * np.asarray(ivw) - np.asarray(loads)
    return float(np.sum(0.5 * scale * np.asarray(dt_over_T) * m * m)), thickness * scale * np.asarray(dt_over_T) * m
