"""Times c8_eval_exact_errors and c8_eval_linearization_errors beside c8_eval_error_contributions on a 100^3 hex8 brick
(1 M elements) for small_J2 and hyper_J2: the converged state of a ramped step, a second state solved at a load 2 % higher,
random z and phi.  Median / min / max of HIP-event times over --reps calls after 3 warm-ups and the ratios of the medians
to c8_eval_error_contributions.  Prints the library's build id.  GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODELS = {"small_J2": [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], "hyper_J2": [1000.0, 0.25, 2.0, 1.0, 5.0, 0.5, 0.5, 100.0]}  # those of tests/parity_cases.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--models", default="small_J2,hyper_J2")
    ap.add_argument("--what", default="error,exact,lin")
    ap.add_argument("--tag", default="")
    ap.add_argument("--eps", type=float, default=0.004)
    a = ap.parse_args()
    import torch
    from calibr8_amd import Assembler, load_library
    from calibr8_amd.assembly import brick_mesh
    from meshes import prescribed_fields
    print("# build %s" % load_library().c8_build_info().decode(), flush=True)
    n = a.edge
    c, conn = brick_mesh(n, n, n)
    for model in a.models.split(","):
        asm = Assembler(8, c, conn, model, MODELS[model], scatter="gather")
        u_h, p_h = prescribed_fields(c, a.eps, ramp=True)
        u, p = asm.dev(u_h), asm.dev(p_h)
        u0, p0 = torch.zeros_like(u), torch.zeros_like(p)
        xi_prev, xi, xi_f = asm.new_state(), asm.new_state(), asm.new_state()
        ls = asm.new_linsys()
        asm.set_async(True)
        asm.forward_jacobian(u, p, u0, p0, xi_prev, xi, ls)  # the converged state of the step
        u_f, p_f = 1.02 * u, 1.02 * p
        asm.forward_jacobian(u_f, p_f, u0, p0, xi_prev, xi_f, ls)  # ... and of the second state
        assert asm.status() == 0
        del ls
        st, fine = (u, p, u0, p0, xi_prev, xi), (u_f, p_f, u0, p0, xi_prev, xi_f)
        gen = torch.Generator(device=u.device).manual_seed(1)
        rand = lambda t: torch.randn(t.shape, dtype=torch.float64, device=t.device, generator=gen)
        z_u, z_p, phi = rand(u), rand(p), rand(xi)
        out = {k: (torch.zeros(asm.nelems, dtype=torch.float64, device=u.device), torch.zeros(asm.nelems, dtype=torch.float64, device=u.device))
               for k in ("error", "exact", "lin")}
        calls = {"error": lambda: asm.error_contributions(*st, z_u, z_p, phi, E_R=out["error"][0], E_C=out["error"][1]),
                 "exact": lambda: asm.exact_errors(st, fine, z_u, z_p, phi, E_R=out["exact"][0], E_C=out["exact"][1]),
                 "lin": lambda: asm.linearization_errors(st, fine, z_u, z_p, phi, E_R=out["lin"][0], E_C=out["lin"][1])}
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
            print("%-8s %-9s %-6s median %.3f ms  min %.3f  max %.3f   (%.1f M elements/s)" %
                  (a.tag, model, k, np.median(t), t.min(), t.max(), len(conn) / np.median(t) / 1e3), flush=True)
        if len(med) == 3:
            # what was timed: one call each from zero, lin + error = exact element by element
            for pair in out.values():
                pair[0].zero_()
                pair[1].zero_()
            for k in calls:
                calls[k]()
            torch.cuda.synchronize()
            assert asm.status() == 0
            worst = 0.0
            for j in (0, 1):
                err = (out["lin"][j] + out["error"][j] - out["exact"][j]).abs()
                scale = out["lin"][j].abs() + out["error"][j].abs() + out["exact"][j].abs()
                assert torch.isfinite(out["exact"][j]).all() and float(out["exact"][j].abs().max()) > 0
                worst = max(worst, float(err.max() / scale.max()))
            print("%-8s %-9s check  max |lin + error - exact| / max scale %.2e" % (a.tag, model, worst))
            assert worst < 1e-10
            print("%-8s %-9s ratio  exact / error = %.2f   lin / error = %.2f" % (a.tag, model, med["exact"] / med["error"], med["lin"] / med["error"]),
                  flush=True)
        del asm, out, calls, st, fine, xi, xi_f, xi_prev, phi
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
