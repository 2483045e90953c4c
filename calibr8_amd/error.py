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
        E_R, E_C = zeros(asm.nelems), zeros(asm.nelems)
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
            asm.error_contributions(*hist, z_u, z_p, phi, E_R=E_R, E_C=E_C)
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
    total = E_R + E_C
    t = float(traction.item())
    return ModelFormError(float(total.sum().item()) + t, float(total.abs().sum().item()), E_R, E_C, t, float(norms[0].item()),
                          float(norms[1].item()))
