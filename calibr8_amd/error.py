"""Model-form error on one mesh (the reference's main_model_form_error.cpp): what a richer local model would have changed
in the objective, estimated from the solved run of a cheaper one without solving the rich primal problem.

The local state of the base run is copied into the fine model (Disc::create_primal_fine_model, disc.cpp:686-704: x and xi
as they are -- both models have the same local layout), the adjoint problem of the fine model is solved linearised about
that state, and the adjoint-weighted residuals of the fine model at that state, summed over steps and elements,
    eta = sum_steps sum_e (E_R + E_C)        (c8_eval_error_contributions)
estimate J(fine) - J(base) to first order in the difference of the two models.

The fine model evaluates the copied state on the branch its own yield test chooses (the reference's force_path is not
supported).  A yielded point of the base run sits on the base model's yield surface; if the fine model puts that state
inside its own surface (a harder model: larger yield stress or hardening modulus), the point is linearised on the elastic
branch and eta stops following the difference of the models -- for small_J2 against small_J2 with the hardening modulus
K (1 + delta), eta is the same number for every delta > 0, and second-order accurate for delta < 0.

model_form_error_verify (the reference's main_model_form_error_verify.cpp) takes the solved run of the fine model as well
and adds what eta leaves out: with the linearization errors of the fine residuals between the two histories
(c8_eval_linearization_errors), for an objective that is linear in the state
    J(fine) - J(base) = eta + E_lin_R + E_lin_C
holds to rounding -- a number that must close, and closes only if the adjoint assembly, the local adjoint solve, the history
vectors and the error kernels agree with each other.
"""
import ctypes as C

import numpy as np

from . import lib as _l
from .primal import _callback, scipy_solver


class ModelFormError:
    """eta, eta_bound = sum_e |E_R + E_C| (main_model_form_error.cpp:103-125), the element fields E_R and E_C [nelems]
    (device tensors, summed over the steps), and the traction term z . (-T) summed over the steps, which eta includes (0
    without traction conditions; the reference's driver leaves it out).  z_norm and phi_norm: the largest |z|_2 and |phi|_1
    of a step -- what residuals of size r (global) and c (local, per point) of the base run can contribute to eta is at most
    steps (z_norm r + phi_norm c)."""

    def __init__(self, eta, eta_bound, E_R, E_C, traction, z_norm=0.0, phi_norm=0.0):
        self.eta, self.eta_bound, self.E_R, self.E_C, self.traction = eta, eta_bound, E_R, E_C, traction
        self.z_norm, self.phi_norm = z_norm, phi_norm

    def __repr__(self):
        return "ModelFormError(eta=%r, eta_bound=%r, traction=%r)" % (self.eta, self.eta_bound, self.traction)


def _same_discretisation(base, fine):
    if (base.elem_type, base.nnodes, base.nelems) != (fine.elem_type, fine.nnodes, fine.nelems) or \
            not np.array_equal(base.conn, fine.conn) or not np.array_equal(base.coords, fine.coords):
        raise ValueError("model_form_error: the fine assembler is not on the mesh of the primal run")
    if (base.nloc, base.npts) != (fine.nloc, fine.npts):
        raise ValueError("model_form_error: the local state of %s (%d unknowns at %d points) cannot be copied into %s (%d at %d)" %
                         (base.local_type, base.nloc, base.npts, fine.local_type, fine.nloc, fine.npts))
    if (base.ndims, base.nres) != (fine.ndims, fine.nres):
        raise ValueError("model_form_error: the two models run under different global residuals")
    if base.objective != fine.objective:
        raise ValueError("model_form_error: the two assemblers have different objectives")


def _adjoint_march(primal, fine_asm, solver, per_step):
    """The adjoint of `fine_asm` marched backwards about the history of the solved PrimalDriver `primal` through
    c8_adjoint_solve_step; per_step(step, hist, z_u, z_p, phi) after every step, hist = (u, p, u_prev, p_prev, xi_prev, xi)
    of the base run.  Returns (traction, z_norm, phi_norm): sum_steps z . (-T), and the largest |z|_2 and |phi|_1 of a step.

    A fine context that would take the row-per-node adjoint kernels (small_J2 on hex8 under the kernel choice 'auto' or
    'node') is put on 'wave_ad' for the duration of the march: those kernels recompute the local state from xi_prev and never
    read the stored xi, which for a copied state is the wrong linearisation point."""
    torch = primal.torch
    asm, dev = fine_asm, fine_asm.device
    nsteps = len(primal.u) - 1
    solver = solver if solver is not None else scipy_solver(asm)
    kernel = asm.kernel
    recomputes = asm.elem_type == 8 and asm.local_type == "small_J2" and kernel in ("auto", "node")
    if recomputes:
        asm.set_kernel("wave_ad")
    try:
        zeros = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        g, f = zeros(asm.nelems, asm.npts, asm.nloc), zeros(asm.nelems, asm.npts, asm.ndofs)
        phi = torch.zeros_like(g)
        grad = zeros(max(1, asm.num_grad_params))  # the step driver adds the parameter gradient of the fine model: not used
        z_u, z_p = zeros(asm.nnodes * asm.ndims), zeros(asm.nnodes)
        ls = asm.new_linsys()
        sy = ls.c_struct()
        zero_vals = [asm.dev(np.zeros(len(nodes))) for _, _, nodes, _ in primal.dbcs]
        d = (_l.Dbc * max(1, len(primal.dbcs)))()
        for k, (resid, eq, nodes, _) in enumerate(primal.dbcs):
            d[k] = _l.Dbc(resid, eq, len(nodes), primal._dbc_nodes[k].data_ptr(), zero_vals[k].data_ptr())
        fn, user = _callback(solver)
        traction, norms = zeros(1), zeros(2)
        for step in range(nsteps, 0, -1):
            if getattr(primal, "measured", None) is not None:
                asm.set_measured(primal.measured[0][step], primal.measured[1][step])
            hist = (primal.u[step], primal.p[step], primal.u[step - 1], primal.p[step - 1], primal.xi[step - 1], primal.xi[step])
            st = asm._state(*hist)
            z = (C.c_void_p * 2)(z_u.data_ptr(), z_p.data_ptr())
            _l.check(asm.L.c8_adjoint_solve_step(asm.h, C.byref(st), C.byref(sy), len(primal.dbcs), d, fn, user, z,
                                                 C.c_void_p(phi.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(f.data_ptr()),
                                                 C.c_void_p(grad.data_ptr())))
            per_step(step, hist, z_u, z_p, phi)
            step_norms = torch.stack([torch.sqrt(z_u.dot(z_u) + (z_p.dot(z_p) if asm.nres == 2 else 0.0)), phi.abs().sum()])
            norms = torch.maximum(norms, step_norms)
            if primal.tbcs:  # b = -T (c8_apply_traction subtracts the integrated traction from b)
                _, tb, keep = primal._bc_structs(step * primal.step_size)
                ls.zero()
                _l.check(asm.L.c8_apply_traction(asm.h, len(primal.tbcs), tb, C.byref(sy)))
                traction += torch.dot(z_u, ls.b[0])
                if asm.nres == 2:
                    traction += torch.dot(z_p, ls.b[1])
        torch.cuda.synchronize()
    finally:
        if recomputes:
            asm.set_kernel(kernel)
    return float(traction.item()), float(norms[0].item()), float(norms[1].item())


def model_form_error(primal, fine_asm, solver=None):
    """`primal`: a solved PrimalDriver of the base model; `fine_asm`: an Assembler of the richer model on the same mesh, with
    the same number of local unknowns and points and the same objective (else ValueError); `solver`: the linear solver of
    the adjoint systems of `fine_asm` (default scipy_solver(fine_asm)).  Marches the steps backwards through
    c8_adjoint_solve_step on `fine_asm` with the base history and calls Assembler.error_contributions with every step's z
    and phi.  Returns a ModelFormError.

    A fine context that would take the row-per-node adjoint kernels (small_J2 on hex8 under the kernel choice 'auto' or
    'node') is put on 'wave_ad' for the duration of the call: those kernels recompute the local state from xi_prev and never
    read the stored xi, which for a copied state is the wrong linearisation point."""
    torch, base = primal.torch, primal.asm
    _same_discretisation(base, fine_asm)
    asm = fine_asm
    E_R, E_C = [torch.zeros(asm.nelems, dtype=torch.float64, device=asm.device) for _ in range(2)]
    t, z_norm, phi_norm = _adjoint_march(primal, asm, solver,
                                         lambda step, hist, z_u, z_p, phi: asm.error_contributions(*hist, z_u, z_p, phi, E_R=E_R, E_C=E_C))
    total = E_R + E_C
    return ModelFormError(float(total.sum().item()) + t, float(total.abs().sum().item()), E_R, E_C, t, z_norm, phi_norm)


class ModelFormErrorVerify:
    """What model_form_error_verify returns (the reference's main_model_form_error_verify.cpp):
    J_H, J_h            the objective of the base and of the fine run
    eta                 sum_steps sum_e (E_R + E_C) of the error contributions, plus z . (-T) under traction conditions
    E_lin_R, E_lin_C    the linearization errors, summed over steps and elements; E_lin_R includes z . (+T)
    E_exact             J_h - J_H
    E_computed          eta + E_lin_R + E_lin_C: equals E_exact for a linear objective
    allowance           steps (z_norm r + phi_norm c), r and c the global and local residual tolerances of the fine run: what
                        residuals of that size can contribute to the identity (ModelFormError explains z_norm, phi_norm)
    traction            z . (-T) summed over the steps (it cancels in E_computed)
    fields              dict of element fields [nelems] (device tensors, summed over the steps): 'E_R', 'E_C' (error
                        contributions), 'E_exact_R', 'E_exact_C' (c8_eval_exact_errors: their sum is E_exact too),
                        'E_lin_R', 'E_lin_C'"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "ModelFormErrorVerify(E_exact=%r, E_computed=%r, eta=%r, E_lin_R=%r, E_lin_C=%r, allowance=%r)" % (
            self.E_exact, self.E_computed, self.eta, self.E_lin_R, self.E_lin_C, self.allowance)


def model_form_error_verify(primal, fine_primal, solver=None):
    """main_model_form_error_verify.cpp on one mesh.  `primal` and `fine_primal`: two solved PrimalDrivers, of the base and
    of the fine model, on the same mesh with the same local layout, objective, conditions and number of steps (else
    ValueError).  The objective must be linear in the state -- "Only valid for linear QoIs" (evaluations.hpp:105): average
    displacement or a displacement component over an element set -- else ValueError.  Marches the adjoint of the fine model about the BASE history exactly as
    model_form_error does and calls error_contributions, exact_errors and linearization_errors (state = base step, fine =
    the fine run's step) with every step's z and phi.  Returns a ModelFormErrorVerify; the reference's test is
    |E_computed - E_exact| <= 1e-8 |E_exact| (+ allowance)."""
    torch, base, asm = primal.torch, primal.asm, fine_primal.asm
    _same_discretisation(base, asm)
    linear = asm.objective[0] == "avg_disp" or asm.objective[:2] == ("subdomain", _l.C8_QOI_DISP_COMP)
    if not linear:
        raise ValueError("model_form_error_verify: only valid for linear QoIs (average displacement, displacement component), not %r" % (asm.objective[0],))
    if len(primal.u) != len(fine_primal.u):
        raise ValueError("model_form_error_verify: the two runs have %d and %d steps" % (len(primal.u) - 1, len(fine_primal.u) - 1))
    same = lambda a, b, k: len(a) == len(b) and all(np.array_equal(np.asarray(x[i]), np.asarray(y[i])) for x, y in zip(a, b) for i in range(k))
    # (resid, eq, nodes) of the Dirichlet conditions, (resid, faces) of the tractions; the value functions cannot be compared
    if not same(primal.dbcs, fine_primal.dbcs, 3) or not same(primal.tbcs, fine_primal.tbcs, 2) or \
            primal.step_size != fine_primal.step_size:
        raise ValueError("model_form_error_verify: the two runs have different boundary conditions")
    names = ("E_R", "E_C", "E_exact_R", "E_exact_C", "E_lin_R", "E_lin_C")
    F = {k: torch.zeros(asm.nelems, dtype=torch.float64, device=asm.device) for k in names}
    fp = fine_primal

    def per_step(step, hist, z_u, z_p, phi):
        fine = (fp.u[step], fp.p[step], fp.u[step - 1], fp.p[step - 1], fp.xi[step - 1], fp.xi[step])
        asm.error_contributions(*hist, z_u, z_p, phi, E_R=F["E_R"], E_C=F["E_C"])
        asm.exact_errors(hist, fine, z_u, z_p, phi, E_R=F["E_exact_R"], E_C=F["E_exact_C"])
        asm.linearization_errors(hist, fine, z_u, z_p, phi, E_R=F["E_lin_R"], E_C=F["E_lin_C"])

    t, z_norm, phi_norm = _adjoint_march(primal, asm, solver, per_step)
    J_H, J_h = primal.qoi(), fine_primal.qoi()
    eta = float((F["E_R"] + F["E_C"]).sum().item()) + t       # tbcs.cpp:322: -z . T
    E_lin_R = float(F["E_lin_R"].sum().item()) - t             # tbcs.cpp:235: +z . T
    E_lin_C = float(F["E_lin_C"].sum().item())
    nsteps = len(primal.u) - 1
    allowance = nsteps * (z_norm * fp.opts.abs_tol + phi_norm * asm.local_abs_tol)
    return ModelFormErrorVerify(J_H=J_H, J_h=J_h, eta=eta, E_lin_R=E_lin_R, E_lin_C=E_lin_C, E_exact=J_h - J_H,
                                E_computed=eta + E_lin_R + E_lin_C, allowance=allowance, traction=t, z_norm=z_norm,
                                phi_norm=phi_norm, fields=F)


def spr_smooth(asm, nodal, out=None):
    """The body of the reference's perform_SPR loop (main_spr_error.cpp) for one nodal field [nnodes, ...]: interpolate it to
    the local-state points (interpolate_to_cell_center), recover it to the nodes by superconvergent patch recovery
    (spr_recovery).  Affine fields come back unchanged; `out`, if given, is overwritten and returned."""
    return asm.spr_recover(asm.interpolate_to_points(nodal), out=out)
