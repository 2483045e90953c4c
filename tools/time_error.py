"""Times c8_eval_error_contributions beside c8_assemble_residual (K2) on the bench workload (100^3 hex8 brick, small_J2,
ramped state, random z and phi): median / min / max of HIP-event times over --reps calls after 3 warm-ups, and the ratio of
the two medians.  GPU box.  --what k2 times the residual alone (tools/time_cauchy.py --what k2 does the same for a library
without this entry point)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--what", default="k2,error")
    ap.add_argument("--tag", default="")
    ap.add_argument("--eps", type=float, default=0.004)
    a = ap.parse_args()
    import torch
    from calibr8_amd import Assembler
    from calibr8_amd.assembly import brick_mesh
    from meshes import prescribed_fields
    n = a.edge
    c, conn = brick_mesh(n, n, n)
    asm = Assembler(8, c, conn, "small_J2", [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], scatter="gather")
    u_h, p_h = prescribed_fields(c, a.eps, ramp=True)
    u, p = asm.dev(u_h), asm.dev(p_h)
    u0, p0 = torch.zeros_like(u), torch.zeros_like(p)
    xi_prev, xi = asm.new_state(), asm.new_state()
    ls = asm.new_linsys()
    asm.set_async(True)
    asm.forward_jacobian(u, p, u0, p0, xi_prev, xi, ls)  # the converged state of the step
    gen = torch.Generator(device=u.device).manual_seed(1)
    rand = lambda t: torch.randn(t.shape, dtype=torch.float64, device=t.device, generator=gen)
    z_u, z_p, phi = rand(u), rand(p), rand(xi)
    E_R = torch.zeros(asm.nelems, dtype=torch.float64, device=u.device)
    E_C = torch.zeros_like(E_R)
    calls = {"k2": lambda: asm.global_residual(u, p, u0, p0, xi_prev, xi, ls),
             "error": lambda: asm.error_contributions(u, p, u0, p0, xi_prev, xi, z_u, z_p, phi, E_R=E_R, E_C=E_C)}
    med = {}
    for k in a.what.split(","):
        call = calls[k]
        for _ in range(3):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        assert asm.status() == 0
        t = np.array([s.elapsed_time(e) for s, e in ev])
        med[k] = np.median(t)
        print("%-10s %-7s median %.3f ms  min %.3f  max %.3f   (%.1f M elements/s)" %
              (a.tag, k, np.median(t), t.min(), t.max(), len(conn) / np.median(t) / 1e3), flush=True)
    if "error" in med:
        # what was timed is the estimate's element loop: sum_e E_R of one call is z . b of the residual at the same state
        E_R.zero_()
        E_C.zero_()
        calls["error"]()
        ls.zero()
        calls["k2"]()
        torch.cuda.synchronize()
        assert asm.status() == 0
        ref = float(z_u.dot(ls.b[0]) + z_p.dot(ls.b[1]))
        scale = float((z_u * ls.b[0]).abs().sum() + (z_p * ls.b[1]).abs().sum())
        err = abs(float(E_R.sum()) - ref)
        print("%-10s check   |sum E_R - z.b| %.2e of sum |z_i b_i| %.3e; max |E_C| %.2e" % (a.tag, err, scale, float(E_C.abs().max())))
        assert torch.isfinite(E_R).all() and torch.isfinite(E_C).all() and err < 1e-10 * scale
        if "k2" in med:
            print("%-10s ratio   error / k2 = %.2f" % (a.tag, med["error"] / med["k2"]))


if __name__ == "__main__":
    main()
