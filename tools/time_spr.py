"""Times c8_spr_recover (k_spr_apply) on the 100^3 hex8 brick and on a tet4 mesh of about a million elements (the 6-tet split
of a 55^3 brick), for ncomp 1 and 9: median / min / max of HIP-event times over --reps calls after 3 warm-ups, the bytes a
call must move at least (sample values once, sample positions once, g and h, nodal coordinates, the patch table, the output)
and the bandwidth they imply; c8_interpolate_to_points beside it; and the one-off set-up, split into device fit and host
expansion (c8_spr_table's record).  GPU box.  --lib times another build of libc8.so (a -DC8_TUNE_SPR_GROUP_* build)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def tet_brick(n):
    """the 6-tet split of an n^3 unit brick round the cell diagonal 0-6, positively oriented"""
    from calibr8_amd.assembly import brick_mesh
    c, hexes = brick_mesh(n, n, n)
    tets = np.concatenate([np.stack([hexes[:, 0], hexes[:, a], hexes[:, b], hexes[:, 6]], axis=1)
                           for a, b in ((1, 2), (2, 3), (3, 7), (7, 4), (4, 5), (5, 1))]).astype(np.int32)
    vol = np.linalg.det(c[tets[:, 1:]] - c[tets[:, :1]])
    flip = vol < 0
    tets[flip, 1], tets[flip, 2] = tets[flip, 2].copy(), tets[flip, 1].copy()
    # cell-major order, as a mesher would number them
    order = np.argsort(np.tile(np.arange(len(hexes)), 6), kind="stable")
    return c, np.ascontiguousarray(tets[order])


def timed(call, reps, torch):
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
    ap.add_argument("--tet-edge", type=int, default=55)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--meshes", default="hex8,tet4")
    ap.add_argument("--ncomp", default="1,9")
    ap.add_argument("--tag", default="")
    ap.add_argument("--lib", default="")
    a = ap.parse_args()
    if a.lib:
        from calibr8_amd import lib
        lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    from calibr8_amd import Assembler
    from calibr8_amd.assembly import brick_mesh
    for kind in a.meshes.split(","):
        c, conn = brick_mesh(a.edge, a.edge, a.edge) if kind == "hex8" else tet_brick(a.tet_edge)
        asm = Assembler(conn.shape[1], c, conn, "small_J2", [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0])
        t0 = time.perf_counter()
        tab = asm.spr_patches()
        wall = (time.perf_counter() - t0) * 1e3
        dev_ms, host_ms, up_ms, flagged = tab["setup"]
        nsamp = int(tab["patch_ptr"][-1]) * asm.npts
        print("%-8s %-5s set-up: %d nodes, %d elements, %d table entries (%.1f samples per node, max %d), %d nodes flagged, stages max %d" %
              (a.tag, kind, asm.nnodes, asm.nelems, len(tab["patch_elems"]), nsamp / asm.nnodes,
               int(np.diff(tab["patch_ptr"]).max()) * asm.npts, int(flagged), int(tab["stages"].max())))
        print("%-8s %-5s set-up: device fit and read-back %.1f ms, host expansion and table %.1f ms, upload %.1f ms, wall with the host copies %.1f ms" %
              (a.tag, kind, dev_ms, host_ms, up_ms, wall), flush=True)
        asm.set_async(True)
        npoints = asm.nelems * asm.npts
        for ncomp in [int(v) for v in a.ncomp.split(",")]:
            field = torch.randn(asm.nelems, asm.npts, ncomp, dtype=torch.float64, device=asm.device)
            nodal = torch.empty(asm.nnodes, ncomp, dtype=torch.float64, device=asm.device)
            t = timed(lambda: asm.spr_recover(field, out=nodal), a.reps, torch)
            assert asm.status() == 0 and bool(torch.isfinite(nodal).all())
            # each of these once: sample values, sample positions, g and h, nodal coordinates, the patch table, the output
            least = (npoints * ncomp * 8 + npoints * asm.ndims * 8 + asm.nnodes * (asm.ndims + 2) * 8 + asm.nnodes * 24 +
                     asm.nnodes * 8 + len(tab["patch_elems"]) * 4 + asm.nnodes * ncomp * 8)
            touched = nsamp * (ncomp + asm.ndims) * 8  # what the lanes request: every sample of every patch
            print("%-8s %-5s recover ncomp %-2d median %.3f ms  min %.3f  max %.3f   %.0f GB/s of %.3f GB least, %.0f GB/s of %.3f GB requested" %
                  (a.tag, kind, ncomp, np.median(t), t.min(), t.max(), least / np.median(t) / 1e6, least / 1e9,
                   touched / np.median(t) / 1e6, touched / 1e9), flush=True)
            back = torch.empty_like(field)
            t = timed(lambda: asm.interpolate_to_points(nodal, out=back), a.reps, torch)
            least = conn.size * 4 + asm.nnodes * ncomp * 8 + npoints * ncomp * 8
            print("%-8s %-5s interp  ncomp %-2d median %.3f ms  min %.3f  max %.3f   %.0f GB/s of %.3f GB least" %
                  (a.tag, kind, ncomp, np.median(t), t.min(), t.max(), least / np.median(t) / 1e6, least / 1e9), flush=True)
        # the timed path on a field with a known answer: an affine field comes back
        from calibr8_amd.error import spr_smooth
        f = asm.dev(c @ np.array([[0.3, -1.0], [0.7, 0.2], [-0.4, 0.5]]) + np.array([0.1, -0.2]))
        err = float((spr_smooth(asm, f) - f).abs().max() / f.abs().max())
        print("%-8s %-5s check: affine field returned to %.2e of its maximum" % (a.tag, kind, err), flush=True)
        assert err < 1e-12
        del asm


if __name__ == "__main__":
    main()
