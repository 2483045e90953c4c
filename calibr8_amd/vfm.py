"""Virtual fields method (VFM) calibration: the objectives Adjoint_VFM, FS_VFM and VFM (adjoint_sens_vfm_objective.cpp,
forward_sens_vfm_objective.cpp, fd_vfm_objective.cpp; selected in main_inverse.cpp:53-58) on the canonical variables of
InverseProblem, minimised by the same bound-constrained L-BFGS.

The local constitutive update is driven by MEASURED displacements (e.g. from digital image correlation) and at every
step the internal-force residual is contracted with a fixed nodal virtual field w:

    J = sum_n 1/2 s dt_n / T (t w^T R(u_meas,n, xi_n) - L_n)^2

with s the objective scale factor, t the thickness and L_n the measured load.  There is no global linear solve: every
step is one pass of per-element kernels (c8_vfm_*), and on a multi-part mesh the only communication is one sum of the
per-step values and one of the gradient.  Host control flow only."""
import numpy as np

from . import lib as _l
from .inverse import FEMUProblem


class VFMProblem(FEMUProblem):
    """value_and_gradient(canonical) -> (J, canonical gradient) or None (a local solve failed: the optimiser backs off);
    solve(initial_active, **opts) as InverseProblem.

    asm: Assembler of a one-residual system (`mechanics_plane_stress` on tri3); its parameters are the base values and the
    active ones (of element set 0) move.  u_meas: measured nodal displacements of steps 0..N ([nnodes * 2] each, device
    tensors or host arrays); loads: measured loads of steps 1..N; w: the nodal virtual field [nnodes * 2] (the caller
    evaluates its expression); times: t_0..t_N.  gradient: "adjoint" (Adjoint_VFM: the steps forward with every local
    state kept on the device, the mismatches summed over the parts, then the backward march), "forward" (FS_VFM: local
    sensitivities carried forward), "fd" (VFM: forward differences of the value, as FEMUProblem).  comm: distributed.Comm
    of a multi-part mesh (each part an Assembler on its own elements and local nodes).

    One deliberate deviation from the reference: the gradient is the exact derivative of the value, INCLUDING the
    thickness factor t of the mismatch.  Both reference gradients leave it out (adjoint_sens_vfm_objective.cpp:108-109,
    forward_sens_vfm_objective.cpp:100-106), which differs only when thickness != 1."""

    def __init__(self, asm, u_meas, loads, w, times, scale=1.0, thickness=1.0, active=(), bounds=(), gradient="adjoint",
                 comm=None, fd_step=1e-6):
        if gradient not in ("adjoint", "forward", "fd"):
            raise ValueError("gradient must be 'adjoint', 'forward' or 'fd'")
        self.asm = asm
        self.all_params = np.array(asm.params, dtype=np.float64)
        super().__init__(None, self.all_params[0], active, bounds, comm, fd_step)
        torch = asm.torch
        self.torch = torch
        self.u = [u.contiguous() if torch.is_tensor(u) else asm.dev(np.ravel(u)) for u in u_meas]
        self.nsteps = len(self.u) - 1
        self.loads = np.asarray(loads, dtype=np.float64).ravel()
        t = np.asarray(times, dtype=np.float64).ravel()
        if self.nsteps < 1 or len(self.loads) != self.nsteps or len(t) != self.nsteps + 1:
            raise ValueError("VFMProblem: steps 0..N of u_meas, N loads and N + 1 times")
        self.dt_over_T = np.diff(t) / (t[-1] - t[0])
        self.w = w.contiguous() if torch.is_tensor(w) else asm.dev(np.ravel(w))
        asm.vfm_set_virtual_field(self.w)
        self.scale, self.thickness, self.gradient = float(scale), float(thickness), gradient
        self.p0 = torch.zeros(asm.nnodes, dtype=torch.float64, device=asm.device)  # no pressure under one residual
        asm.set_active(0, self.active)
        self.ivw = None  # per-step w^T R of the last evaluation, summed over the parts

    def _set_params(self, canonical):
        phys = self.to_physical(canonical)
        params = self.all_params.copy()
        params[0, self.active] = phys
        self.asm.set_params(params)
        return phys

    def _sum(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a if self.comm is None else np.asarray(self.comm.allreduce(a), dtype=np.float64)

    def _march(self, sens):
        """the steps forward: (w^T R per step summed over the parts, local states, d(w^T R)/dp per step) or None"""
        asm, torch = self.asm, self.torch
        dev, n, na = asm.device, self.nsteps, len(self.active)
        ivw = torch.zeros(n, dtype=torch.float64, device=dev)
        divw = torch.zeros((n, max(na, 1)), dtype=torch.float64, device=dev)
        xi = [asm.new_state()]
        S = [torch.zeros(asm.nelems * asm.npts * asm.nloc * na, dtype=torch.float64, device=dev) for _ in range(2 if sens else 0)]
        failed = False
        for s in range(1, n + 1):
            x = xi[-1].clone()
            if sens:
                rc = asm.vfm_forward_sens(self.u[s], self.p0, self.u[s - 1], self.p0, xi[-1], x, S[s % 2] if s > 1 else None,
                                          S[(s + 1) % 2], ivw[s - 1:s], divw[s - 1])
            else:
                rc = asm.vfm_internal_power(self.u[s], self.p0, self.u[s - 1], self.p0, xi[-1], x, ivw[s - 1:s])
            if rc != 0:
                failed = True
                break
            xi.append(x)
        if self.comm is not None:  # every part backs off together
            failed = self._sum([1.0 if failed else 0.0])[0] > 0.0
        if failed:
            return None
        return self._sum(ivw.cpu().numpy()), xi, divw[:, :na]

    def _value_from(self, ivw):
        self.ivw = ivw
        mismatch = self.thickness * ivw - self.loads
        J = float(np.sum(0.5 * self.scale * self.dt_over_T * mismatch * mismatch))
        return J, mismatch

    def value(self, canonical):
        canonical = np.ascontiguousarray(canonical, dtype=np.float64)
        if self._last[0] is not None and np.array_equal(self._last[0], canonical):
            return self._last[1]
        self._set_params(canonical)
        r = self._march(False)
        if r is None:
            return None
        J = self._value_from(r[0])[0]
        self._last = (canonical.copy(), J)
        return J

    def physical_value_and_gradient(self, canonical):
        """(J, dJ/dp of the active parameters in physical units) by the problem's adjoint or forward gradient, or None"""
        canonical = np.ascontiguousarray(canonical, dtype=np.float64)
        self._set_params(canonical)
        r = self._march(self.gradient == "forward")
        if r is None:
            return None
        ivw, xi, divw = r
        J, mismatch = self._value_from(ivw)
        # dJ/d(w^T R)_n: the exact derivative, thickness included (see the class docstring)
        c = self.thickness * self.scale * self.dt_over_T * mismatch
        na = len(self.active)
        if self.gradient == "forward":
            g = self._sum(divw.cpu().numpy()).reshape(self.nsteps, na).T @ c
        else:
            asm, torch = self.asm, self.torch
            h = torch.zeros(asm.nelems * asm.npts * asm.nloc, dtype=torch.float64, device=asm.device)
            gd = torch.zeros(max(na, 1), dtype=torch.float64, device=asm.device)
            failed = False
            for s in range(self.nsteps, 0, -1):
                if asm.vfm_adjoint_step(self.u[s], self.p0, self.u[s - 1], self.p0, xi[s - 1], xi[s], float(c[s - 1]), h, gd) != 0:
                    failed = True
                    break
            if self.comm is not None:
                failed = self._sum([1.0 if failed else 0.0])[0] > 0.0
            if failed:
                return None
            g = self._sum(gd.cpu().numpy()[:na])
        return J, np.ascontiguousarray(g, dtype=np.float64)

    def value_and_gradient(self, canonical):
        if self.gradient == "fd":
            return super().value_and_gradient(canonical)
        r = self.physical_value_and_gradient(canonical)
        if r is None:
            return None
        J, g = r
        L = _l.load_library()
        canon = np.ascontiguousarray(canonical, dtype=np.float64)
        gc = np.zeros_like(g)
        _l.check(L.c8_transform_gradient(len(g), g.ctypes.data_as(_l.dp), canon.ctypes.data_as(_l.dp),
                                         self.kind.ctypes.data_as(_l.i32p), self.lo.ctypes.data_as(_l.dp),
                                         self.hi.ctypes.data_as(_l.dp), gc.ctypes.data_as(_l.dp)))
        self.history.append((self.to_physical(canon), float(J)))
        return J, gc
