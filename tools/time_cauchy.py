"""Times c8_eval_cauchy beside c8_assemble_residual (K2) on the bench workload (100^3 hex8 brick, small_J2, ramped state):
median / min / max of HIP-event times over --reps calls after 3 warm-ups, and the achieved GB/s of c8_eval_cauchy against
its compulsory bytes (connectivity, xi, nodal coordinates / u / p, 72 B per point; small_J2 reads neither xi_prev nor
u_prev).  GPU box.  --what k2 times the residual alone (a library without c8_eval_cauchy can then be timed too)."""
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
    ap.add_argument("--what", default="k2,cauchy")
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
    calls = {"k2": lambda: asm.global_residual(u, p, u0, p0, xi_prev, xi, ls)}
    if "cauchy" in a.what.split(","):
        sigma = torch.empty(asm.nelems, asm.npts, 3, 3, dtype=torch.float64, device=u.device)
        calls["cauchy"] = lambda: asm.cauchy(u, p, u0, p0, xi_prev, xi, out=sigma)
    npoints = asm.nelems * asm.npts
    compulsory = conn.size * 4 + npoints * asm.nloc * 8 + asm.nnodes * (3 + 3 + 1) * 8 + npoints * 72
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
        extra = "   %.0f GB/s of %.3f GB compulsory" % (compulsory / np.median(t) / 1e6, compulsory / 1e9) if k == "cauchy" else ""
        print("%-10s %-7s median %.3f ms  min %.3f  max %.3f   (%.1f M elements/s)%s" %
              (a.tag, k, np.median(t), t.min(), t.max(), len(conn) / np.median(t) / 1e3, extra), flush=True)
    if "cauchy" in calls:  # the timed field is a stress field: finite, and yielded points carry |s| = sqrt(2/3) (Y + K alpha)
        s = sigma.reshape(-1, 3, 3)
        dev = s - torch.eye(3, dtype=s.dtype, device=s.device) * (s.diagonal(dim1=1, dim2=2).sum(1) / 3.0)[:, None, None]
        alpha = xi.reshape(-1, asm.nloc)[:, 6]
        on = alpha > 0
        gap = (dev[on].flatten(1).norm(dim=1) - np.sqrt(2.0 / 3.0) * (2.0 + 100.0 * alpha[on])).abs().max().item()
        print("%-10s check   %d of %d points yielded, largest distance from the yield surface %.2e" % (a.tag, int(on.sum()), npoints, gap))
        assert torch.isfinite(sigma).all() and int(on.sum()) > 0 and gap < 1e-9


if __name__ == "__main__":
    main()
