"""`-m gpu`: the Gauss-Seidel preconditioner of the device solve over the parts of a multi-part mesh:
part-local colouring and sweeps (ghost and phantom columns dropped) against a numpy replay, the solve against the contract
of the Jacobi-preconditioned one and against its iteration count.  The harness is that of test_gpu_krylov_parts.py: the ranks
share the card over the host transport."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_gpu_distributed import spawn  # noqa: E402
from test_gpu_krylov import new_dx, raw_solve, system_case  # noqa: E402
from test_gpu_krylov_parts import (assert_contract, bar_parts, check_contract, close, gather_pieces, init, owned_piece, part_system,  # noqa: E402
                                   solve_parts)
from test_gpu_krylov_sgs import JACOBI, SGS, Replay, device_colors, greedy_colors, node_index, precond, set_precond, system  # noqa: E402

pytestmark = pytest.mark.gpu


def owned_matrix(asm, ls, no):
    """the owned rows and owned columns of this part's matrix over the unknowns (u of the owned nodes, then their p)"""
    import scipy.sparse as sp
    n, nres, neq = asm.nnodes, asm.nres, asm.neq
    blocks = []
    for i in range(nres):
        nrows = no * neq[i]
        row = []
        for j in range(nres):
            rp, ci = asm.rowptr[i][j], asm.colidx[i][j]
            m = sp.csr_matrix((ls.A[i][j].cpu().numpy()[: rp[nrows]], ci[: rp[nrows]], rp[: nrows + 1]), shape=(nrows, n * neq[j]))
            row.append(m[:, : no * neq[j]])
        blocks.append(row)
    return sp.bmat(blocks, format="csr")


def part_apply(asm, ls, v, no):
    """c8_krylov_precondition on a part: v over the owned unknowns; (return code, y on the owned unknowns)"""
    n, nd = asm.nnodes, asm.ndims
    vu, vp = np.zeros(n * nd), np.zeros(n)
    vu[: no * nd], vp[:no] = v[: no * nd], v[no * nd:]
    vin = [asm.dev(vu), asm.dev(vp)]
    y = [torch.full_like(vin[0], 7.0), torch.full_like(vin[1], 7.0)]
    sy = ls.c_struct()
    rc = asm.L.c8_krylov_precondition(asm.h, C.byref(sy), (C.c_void_p * 2)(vin[0].data_ptr(), vin[1].data_ptr()),
                                      (C.c_void_p * 2)(y[0].data_ptr(), y[1].data_ptr()))
    torch.cuda.synchronize()
    return rc, np.concatenate([y[0].cpu().numpy()[: no * nd], y[1].cpu().numpy()[:no]])


# ---- 8. one rank with a halo attached ------------------------------------------------------------------------------------
def test_one_rank_with_a_halo_equals_the_single_part_solve():
    from calibr8_amd import Assembler, lib
    import calibr8_amd.distributed as D
    et, c, conn, model, params, spec, _ = system_case((16, 4, 4))
    part = D.part_from_global(c, conn, np.zeros(len(conn), dtype=np.int32), 0, 1)
    plan = D.HaloPlan(part, None)
    asm = Assembler(et, plan.coords, part.conn, model, params)
    comm = D.Comm.host(None, 0, 1)
    halo = D.Halo(plan, asm.rowptr[1][1], asm.colidx[1][1], asm, comm)
    S = dict(c=c, part=part, plan=plan, asm=asm, comm=comm, halo=halo)
    ls = part_system(S, spec)
    set_precond(asm, SGS, 1)
    rc, info, dx = solve_parts(asm, ls)
    colors = device_colors(asm)
    a1, l1 = system((16, 4, 4))[:2]
    ref_colors = device_colors(a1)
    with precond(a1, SGS):   # (a context shared with the other module's tests)
        rc1, i1, _ = raw_solve(a1, l1, new_dx(a1))
    close(S)
    print("one rank with a halo: SGS iterations %d, single-part solve %d, colours %d" % (info[0], i1.iters, len(colors)))
    assert rc == lib.C8_OK and rc1 == lib.C8_OK
    assert len(colors) == len(ref_colors) and all(np.array_equal(a, b) for a, b in zip(colors, ref_colors))
    assert info[0] == i1.iters


# ---- 9. two parts of notched_bar(16, 4, 4), K1 ---------------------------------------------------------------------------
def sgs_bar_worker(rank, world, port, out):
    init(rank, world, port)
    try:
        S, spec = bar_parts(rank, world)
        asm, no = S["asm"], S["part"].nowned
        res = {"no": no, "n": asm.nnodes}
        ls = part_system(S, spec)
        rc, info_j, _ = solve_parts(asm, ls)                    # block Jacobi, the default
        res["jacobi"] = (rc, info_j[0])
        # the colour lists: owned nodes only, the greedy colouring of the owned sub-graph
        set_precond(asm, SGS, 1)
        colors = device_colors(asm)
        ref = greedy_colors(asm.rowptr[1][1], asm.colidx[1][1], no)
        every = np.concatenate(colors)
        res["colors"] = (bool(np.array_equal(np.sort(every), np.arange(no))), bool(all((np.diff(k) > 0).all() for k in colors)),
                         bool(len(ref) == len(colors) and all(np.array_equal(a, b) for a, b in zip(ref, colors))), len(colors))
        # the operator: the replay on the owned rows and columns
        Aoo = owned_matrix(asm, ls, no)
        idx = node_index(no, asm.ndims, asm.nres)
        v = np.random.default_rng(17 + rank).standard_normal(Aoo.shape[0])
        rep = Replay(Aoo, idx, colors)
        err = {}
        for name, kind in (("jacobi", JACOBI), ("sgs", SGS)):
            set_precond(asm, kind, 1)
            rca, y = part_apply(asm, ls, v, no)
            y_ref = rep.jacobi(v) if kind == JACOBI else rep.sgs(v)
            err[name] = (rca, float(np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)))
        res["operator"] = err
        # the solve, twice
        rc, info, dx = solve_parts(asm, ls)
        res["rc"], res["info"], res["err"] = rc, info, asm.L.c8_last_error().decode() if rc else ""
        res["x1"] = np.concatenate([dx[i].cpu().numpy()[: no * asm.neq[i]] for i in range(2)]).tobytes()
        allp = gather_pieces(world, owned_piece(S, ls, dx))
        if rank == 0:
            res["contract"] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "two parts, SGS")
        rc2, info2, dx2 = solve_parts(asm, ls)
        res["x2"] = np.concatenate([dx2[i].cpu().numpy()[: no * asm.neq[i]] for i in range(2)]).tobytes()
        res["rc2"], res["iters2"] = rc2, info2[0]
        set_precond(asm, JACOBI)
        close(S)
        out[rank] = res
    finally:
        import torch.distributed as dist
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def sgs_bar_run():
    return spawn(sgs_bar_worker, 2)


def test_two_part_colours_and_operator(sgs_bar_run):
    for r in range(2):
        res = sgs_bar_run[r]
        partition, ascending, greedy, nc = res["colors"]
        op = res["operator"]
        print("rank %d: owned %d of %d local nodes, %d colours, operator error jacobi %.3e sgs %.3e" %
              (r, res["no"], res["n"], nc, op["jacobi"][1], op["sgs"][1]))
        assert res["no"] < res["n"]                    # there are ghost or phantom columns to drop
        assert partition and ascending and greedy, (r, res["colors"])
        assert op["jacobi"][0] == 0 and op["sgs"][0] == 0
        assert op["sgs"][1] < 1e-10 and op["sgs"][1] <= 100.0 * op["jacobi"][1], (r, op)


def test_two_part_sgs_solve(sgs_bar_run):
    from calibr8_amd import lib
    for r in range(2):
        res = sgs_bar_run[r]
        assert res["rc"] == lib.C8_OK and res["rc2"] == lib.C8_OK, (r, res["err"])
        assert res["jacobi"][0] == lib.C8_OK
        assert res["x1"] == res["x2"] and res["info"][0] == res["iters2"], r       # two runs: equal bytes, equal counts
    assert sgs_bar_run[0]["info"] == sgs_bar_run[1]["info"]
    m = sgs_bar_run[0]["contract"]
    print("notched_bar(16, 4, 4) over two parts: device iterations SGS %d, block Jacobi %d" % (m["iters"], sgs_bar_run[0]["jacobi"][1]))
    assert m["n"] == 1580
    assert_contract(m, "two parts, SGS")
    assert 2 * m["iters"] <= sgs_bar_run[0]["jacobi"][1]
