"""Times the passes of the subdomain objectives (c8_qoi_point.hip) beside K3 on the bench workload (100^3 hex8 brick, ramped
state), per model: median / min / max of HIP-event times over --reps calls after 3 warm-ups.  The passes run inside
c8_assemble_adjoint_jacobian, so they are timed as differences of that call under four objectives over the whole mesh (the
most points a pass can have; a second, empty element set gives the zero objective):
    K3          empty set: the adjoint kernels alone
    pre + post  avg_stress - K3
    post        disp_comp - K3: the per-node pass, with a pre-pass that only writes its 104-byte records
    pre         avg_stress - disp_comp: the tangent evaluations of the pre-pass
and c8_eval_qoi (value kernel and its reduction) and c8_param_gradient (K5 with and without the gradient kernel) directly.
GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_cases as pc  # noqa: E402  (the parameter sets of the parity tests)

MODELS = {"small_J2": pc.J2, "hyper_J2": pc.HJ2, "small_hill": pc.HILL}


def timed(torch, call, reps):
    for _ in range(3):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        call()
        e.record()
    torch.cuda.synchronize()
    return np.array([s.elapsed_time(e) for s, e in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--models", default="small_J2,hyper_J2,small_hill")
    ap.add_argument("--tag", default="")
    ap.add_argument("--eps", type=float, default=0.004)
    a = ap.parse_args()
    import torch
    from calibr8_amd import Assembler
    from calibr8_amd.assembly import brick_mesh
    from meshes import prescribed_fields
    n = a.edge
    c, conn = brick_mesh(n, n, n)
    u_h, p_h = prescribed_fields(c, a.eps, ramp=True)
    for model in a.models.split(","):
        prm = MODELS[model]
        asm = Assembler(8, c, conn, model, [prm, prm], elem_set=np.zeros(len(conn), dtype=np.int32), scatter="gather")
        asm.set_active(0, [0, 1, 2, 3])
        u, p = asm.dev(u_h), asm.dev(p_h)
        u0, p0 = torch.zeros_like(u), torch.zeros_like(p)
        xi_prev, xi = asm.new_state(), asm.new_state()
        ls = asm.new_linsys()
        asm.set_async(True)
        asm.forward_jacobian(u, p, u0, p0, xi_prev, xi, ls)  # the converged state of the step
        st = (u, p, u0, p0, xi_prev, xi)
        g = torch.zeros(asm.nelems, asm.npts, asm.nloc, dtype=torch.float64, device=u.device)
        f = torch.zeros(asm.nelems, asm.npts, asm.ndofs, dtype=torch.float64, device=u.device)
        phi, J, grad = torch.zeros_like(g), torch.zeros(1, dtype=torch.float64, device=u.device), torch.zeros(4, dtype=torch.float64, device=u.device)
        z_u, z_p = torch.zeros_like(u), torch.zeros_like(p)
        k3 = lambda: asm.adjoint_jacobian(*st, g, f, ls)
        k5 = lambda: asm.qoi_gradient(*st, z_u, z_p, phi, grad)
        t = {}
        for name, (kind, es) in {"K3": ("avg_stress", 1), "stress": ("avg_stress", 0), "disp": ("disp_comp", 0), "local": ("avg_local_var", 0)}.items():
            asm.set_qoi_subdomain(kind, es, asm.nloc - 1 if kind == "avg_local_var" else 0)
            t[name] = timed(torch, k3, a.reps)
            if name in ("K3", "stress"):
                t["K5 " + name] = timed(torch, k5, a.reps)
        asm.set_qoi_subdomain("avg_stress", 0, 0)
        t["value"] = timed(torch, lambda: asm.eval_qoi(u, p, J, xi_prev=xi_prev, xi=xi, u_prev=u0, p_prev=p0), a.reps)
        assert asm.status() == 0 and float(J.item()) > 0 and bool(torch.isfinite(ls.flat).all())
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = lambda k, v, note="": print("%-10s %-10s %-22s %8.3f ms  %5.1f %% of K3   %s" % (a.tag, model, k, v, 100.0 * v / med["K3"], note), flush=True)
        print("%-10s %-10s K3 median %.3f ms  min %.3f  max %.3f   (%.1f M elements/s)" %
              (a.tag, model, med["K3"], t["K3"].min(), t["K3"].max(), len(conn) / med["K3"] / 1e3), flush=True)
        row("pre + post (stress)", med["stress"] - med["K3"])
        row("post (disp_comp)", med["disp"] - med["K3"], "with a pre-pass that writes records only")
        row("pre (stress - disp)", med["stress"] - med["disp"])
        row("pre (local_var)", med["local"] - med["K3"], "no tangents, no post-pass")
        row("value", med["value"], "c8_eval_qoi: kernel + reduction")
        row("gradient kernel", med["K5 stress"] - med["K5 K3"], "K5 alone %.3f ms" % med["K5 K3"])


if __name__ == "__main__":
    main()
