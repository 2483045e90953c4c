"""Times one c8_krylov_solve (K1 of small_J2 at a ramped plastic state, the Dirichlet rows of tests/test_gpu_krylov.py) on
notched_bar(48, 12, 12) and brick(40, 40, 40), for each preconditioner: HIP-event time around the call, median of --reps
solves after one warm-up; prints iterations, ms per solve and us per iteration.  GPU box.
The events are recorded on torch's current stream, which is the stream the Assembler gave the context (c8_set_stream), and the
solve synchronises that stream at every host read and before it returns, so the time between the two events is the whole
solve as the caller sees it: kernels, launch gaps and the host reads every check_every iterations.
--lib F times another build of libc8.so (an earlier commit's, say): entry points it lacks are left unbound and the
preconditioners it cannot select are skipped.  --profile runs one solve per mesh with the kind of --profile-kind (sgs,
two_level or multilevel) and nothing else (for rocprofv3 --kernel-trace --stats -- python tools/time_krylov.py --profile).
For the two-level kind the set-up of the coarse level (constrained-row flags, A_c = P^T A P, its dense inverse) is timed on
its own as the time of one c8_krylov_precondition call minus the time of the same call with the Gauss-Seidel kind: the
two calls differ by that set-up and one coarse correction; n_coarse is printed beside it.  The multilevel kind is timed once
per value of --coarse-max (0: the library's default), its set-up in the same way, with the nodes of every level printed."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_system(name):
    import torch
    from calibr8_amd import Assembler
    from meshes import brick, fields_for, notched_bar, prescribed_fields
    c, conn, s = notched_bar(48, 12, 12) if name == "notched_bar(48,12,12)" else brick(40, 40, 40)
    asm = Assembler(8, c, conn, "small_J2", [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0])
    u, p = fields_for(asm.ndims, *prescribed_fields(c, 0.004, ramp=True))
    U, P = asm.dev(u), asm.dev(p)
    Z, ZP = torch.zeros_like(U), torch.zeros_like(P)
    ls, xi = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(U, P, Z, ZP, asm.new_state(), xi, ls) == 0
    spec = [(0, d, s["xmin"]) for d in range(3)] + [(0, 0, s["xmax"])]
    dd = [(r, e, torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(np.zeros(len(n)))) for r, e, n in spec]
    asm.apply_dirichlet(dd, U, P, ls)
    torch.cuda.synchronize()
    return asm, ls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--meshes", default="notched_bar(48,12,12);brick(40,40,40)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-kind", default="sgs", choices=["sgs", "two_level", "multilevel"])
    ap.add_argument("--coarse-max", default="0", help="comma-separated coarse_max values of the multilevel kind (0: the default)")
    a = ap.parse_args()
    import torch  # before any libc8.so is loaded: the library has to bind to torch's HIP runtime (calibr8_amd/lib.py)
    from calibr8_amd import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
        raw = C.CDLL(lib.LIB_PATH)
        lib.SYMBOLS[:] = [s for s in lib.SYMBOLS if hasattr(raw, s[0])]
    L = lib.load_library()
    has_sgs = hasattr(L, "c8_krylov_set_preconditioner") and any(s[0] == "c8_krylov_set_preconditioner" for s in lib.SYMBOLS)
    has_two = has_sgs and any(s[0] == "c8_krylov_aggregates" for s in lib.SYMBOLS)
    has_multi = has_two and any(s[0] == "c8_krylov_set_multilevel" for s in lib.SYMBOLS)
    kinds = [("jacobi", 0)] + ([("sgs", 1)] if has_sgs else []) + ([("two_level", lib.C8_PRECOND_TWO_LEVEL)] if has_two else [])
    if has_multi:
        kinds += [("multilevel:%d" % int(v), lib.C8_PRECOND_MULTILEVEL) for v in a.coarse_max.split(",")]
    if a.profile:
        kinds, a.reps = [k for k in kinds if k[0].split(":")[0] == a.profile_kind], 1
    for name in a.meshes.split(";"):
        asm, ls = build_system(name)
        n = asm.nnodes * (asm.ndims + 1)
        dx = (torch.zeros(asm.nnodes * asm.ndims, dtype=torch.float64, device=asm.device), torch.zeros(asm.nnodes, dtype=torch.float64, device=asm.device))
        ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
        sy = ls.c_struct()
        for kind, code in kinds:
            if has_sgs:
                lib.check(L.c8_krylov_set_preconditioner(asm.h, code, 1))
            info = lib.KrylovInfo()
            if kind == "two_level":
                na, ap_ = C.c_int32(), C.POINTER(C.c_int32)()
                lib.check(L.c8_krylov_aggregates(asm.h, C.byref(na), C.byref(ap_)))
                if na.value * 7 > 8192:
                    print("%-10s %-22s unknowns %7d two_level skipped: n_coarse %d exceeds the cap of the dense coarse solve" % (a.tag, name, n, na.value * 7), flush=True)
                    continue
            levels = []
            if code == getattr(lib, "C8_PRECOND_MULTILEVEL", -1):
                lib.check(L.c8_krylov_set_multilevel(asm.h, int(kind.split(":")[1]), 0))
                nl, nn_, nc_ = C.c_int32(), C.c_int32(), C.c_int32()
                p1, p2, p3 = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
                lib.check(L.c8_krylov_levels(asm.h, C.byref(nl)))
                for lev in range(nl.value):
                    lib.check(L.c8_krylov_level(asm.h, lev, C.byref(nn_), C.byref(p1), C.byref(nc_), C.byref(p2), C.byref(p3)))
                    levels.append((nn_.value, nc_.value))

            def solve():
                lib.check(L.c8_krylov_solve(asm.h, C.byref(sy), ptrs, None, C.byref(info)))
            if not a.profile:
                solve()  # warm-up: buffers, colour lists
            t = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                solve()
                e.record()
                torch.cuda.synchronize()
                t.append(s.elapsed_time(e))
            ms = float(np.median(t))
            if (kind == "two_level" or levels) and not a.profile:
                def apply_ms(code_):
                    lib.check(L.c8_krylov_set_preconditioner(asm.h, code_, 1))
                    tt = []
                    for _ in range(a.reps + 1):
                        torch.cuda.synchronize()
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        lib.check(L.c8_krylov_precondition(asm.h, C.byref(sy), ptrs, ptrs))
                        e.record()
                        torch.cuda.synchronize()
                        tt.append(s.elapsed_time(e))
                    return float(np.median(tt[1:]))
                t_sgs, t_two = apply_ms(lib.C8_PRECOND_BLOCK_SGS), apply_ms(code)
                if levels:
                    print("%-10s %-22s %s: nodes per level %s colours per level %s, set-up of the levels %.2f ms (one apply with set-up %.2f ms, "
                          "the same with sgs %.2f ms)" % (a.tag, name, kind, [v[0] for v in levels], [v[1] for v in levels], t_two - t_sgs, t_two, t_sgs), flush=True)
                else:
                    print("%-10s %-22s two_level: aggregates %d n_coarse %d, set-up of the coarse level %.2f ms (one apply with set-up %.2f ms, "
                          "the same with sgs %.2f ms)" % (a.tag, name, na.value, na.value * 7, t_two - t_sgs, t_two, t_sgs), flush=True)
            print("%-10s %-22s unknowns %7d %-15s iterations %5d restarts %d  %9.2f ms per solve  %7.1f us per iteration  (min %.2f max %.2f ms, residual %.2e)" %
                  (a.tag, name, n, kind, info.iters, info.restarts, ms, 1e3 * ms / max(info.iters, 1), min(t), max(t),
                   info.residual_norm / info.b_norm), flush=True)


if __name__ == "__main__":
    main()
