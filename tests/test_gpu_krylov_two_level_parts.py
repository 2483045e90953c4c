"""`-m gpu`: the two-level preconditioner of the device solve over the parts of a multi-part mesh
(C8_PRECOND_TWO_LEVEL_PARTS) against its definition in include/c8.h, replayed in numpy on the gathered
matrix (tests/krylov_parts_replay.py): per-part aggregates and their bases, the global A_c = P^T A P, the operator on the
owned entries, the contract of the solve, iteration counts, reproducible bytes, switching, the collective refusals and one
driver deck.  The harness is that of test_gpu_krylov_parts.py: the ranks share the card over the host transport, several
cases share one spawn.  Every test fails on a library without the kind (the setter refuses 7).

Recorded on one MI355X: see the tables of DESIGN.md section 13f."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import krylov_parts_replay as R  # noqa: E402
from test_gpu_distributed import bcs_for, setup_part, spawn  # noqa: E402
from test_gpu_krylov import REL_TOL, golden, new_dx, raw_solve  # noqa: E402
from test_gpu_krylov_parts import (J2, assert_contract, bar_parts, check_contract, close, gather_pieces, init, make_part, owned_piece,  # noqa: E402
                                   part_system, solve_parts)
from test_gpu_krylov_sgs import JACOBI, SGS, device_apply, device_colors, precond, set_precond, system  # noqa: E402

pytestmark = pytest.mark.gpu
TWO_LEVEL, MULTILEVEL, PARTS = 3, 5, 7   # C8_PRECOND_TWO_LEVEL, C8_PRECOND_MULTILEVEL, C8_PRECOND_TWO_LEVEL_PARTS
COARSE_CAP = 8192
EPS = np.finfo(np.float64).eps


# ---- access to the device ------------------------------------------------------------------------------------------------
def device_aggregates(asm, no):
    """c8_krylov_aggregates + c8_krylov_aggregate_base: (local aggregate of every owned node, their number, base, total)"""
    from calibr8_amd import lib
    na, ptr, base, total = C.c_int32(), C.POINTER(C.c_int32)(), C.c_int32(), C.c_int32()
    lib.check(asm.L.c8_krylov_aggregates(asm.h, C.byref(na), C.byref(ptr)))
    lib.check(asm.L.c8_krylov_aggregate_base(asm.h, C.byref(base), C.byref(total)))
    return np.ctypeslib.as_array(ptr, shape=(no,)).astype(np.int64), na.value, base.value, total.value


def device_coarse_matrix(asm, ls):
    """c8_krylov_coarse_matrix (collective with the kind over parts): (return code, A_c or None)"""
    from calibr8_amd import lib
    n = C.c_int32()
    sy = ls.c_struct()
    rc = asm.L.c8_krylov_coarse_matrix(asm.h, C.byref(sy), C.byref(n), None)
    if rc != lib.C8_OK:
        return rc, None
    out = np.full((n.value, n.value), 7.0)
    rc = asm.L.c8_krylov_coarse_matrix(asm.h, C.byref(sy), C.byref(n), out.ctypes.data_as(lib.dp))
    return rc, out


def part_apply(asm, ls, v_owned, no):
    """c8_krylov_precondition on a part (collective with the kind over parts): v over the owned unknowns (u, then p)"""
    n, nd, two = asm.nnodes, asm.ndims, asm.nres == 2
    vu, vp = np.zeros(n * nd), np.zeros(n)
    vu[: no * nd] = v_owned[: no * nd]
    if two:
        vp[:no] = v_owned[no * nd:]
    vin = [asm.dev(vu), asm.dev(vp)]
    y = [torch.full_like(vin[0], 7.0), torch.full_like(vin[1], 7.0)]
    sy = ls.c_struct()
    rc = asm.L.c8_krylov_precondition(asm.h, C.byref(sy), (C.c_void_p * 2)(vin[0].data_ptr(), vin[1].data_ptr()),
                                      (C.c_void_p * 2)(y[0].data_ptr(), y[1].data_ptr()))
    torch.cuda.synchronize()
    return rc, np.concatenate([y[0].cpu().numpy()[: no * nd]] + ([y[1].cpu().numpy()[:no]] if two else []))


def owned_bytes(asm, dx, no):
    return np.concatenate([dx[i].cpu().numpy()[: no * asm.neq[i]] for i in range(asm.nres)]).tobytes()


def owned_unknowns(gid_owned, N, nd, nres):
    """positions of a part's owned unknowns (u, then p) in the gathered vector"""
    idx = R.global_index(N, nd, nres)
    return np.concatenate([idx[gid_owned, :nd].ravel()] + ([idx[gid_owned, nd]] if nres == 2 else []))


def zero_node_block(asm, ls, node):
    rp, ci = asm.rowptr, asm.colidx
    for i in range(asm.nres):
        for j in range(asm.nres):
            vals = ls.A[i][j].cpu().numpy()
            for eq in range(asm.neq[i]):
                row = node * asm.neq[i] + eq
                lo, hi = rp[i][j][row], rp[i][j][row + 1]
                vals[lo:hi][(ci[i][j][lo:hi] // asm.neq[j]) == node] = 0.0
            ls.A[i][j].copy_(asm.dev(vals))


def coarse_checks(S, ls, world, rank, res, tag, sweeps=(1,), dx=None):
    """What every mesh is checked for with the kind selected: the aggregates against the replay on the owned sub-graph, the
    bases against the prefix sums, A_c against numpy P^T A P on the gathered matrix, the operator on the owned entries.
    Returns the numpy operator (every rank builds it: it needs its own rows of the reference)."""
    asm, no = S["asm"], S["part"].nowned
    N, nd, nres = S["part"].num_global_nodes, asm.ndims, asm.nres
    agg, nagg, base, total = device_aggregates(asm, no)
    ref, nref = R.owned_aggregates(asm.rowptr[1][1], asm.colidx[1][1], no)
    res[tag + "_agg"] = (bool(nagg == nref and np.array_equal(agg, ref)), nagg, base, total)
    rc, Ac = device_coarse_matrix(asm, ls)
    res[tag + "_Ac_rc"] = rc
    res[tag + "_Ac_bytes"] = Ac.tobytes() if Ac is not None else b""
    dx = dx or new_dx(asm)
    piece = owned_piece(S, ls, dx)
    piece.update(agg=agg, nagg=nagg, base=base, colors=device_colors(asm))
    allp = gather_pieces(world, piece)
    A, b = R.gathered_matrix(allp, N, asm.neq, nres)
    parts = [{"gid": q["gid"][: q["no"]], "agg": q["agg"], "nagg": q["nagg"], "base": q["base"], "colors": q["colors"]} for q in allp]
    op = R.TwoLevelParts(A, S["c"], nd, nres, parts)
    cond = float(np.linalg.cond(op.Ac))
    err = float(np.linalg.norm(Ac - op.Ac) / np.linalg.norm(op.Ac)) if Ac is not None and Ac.shape == op.Ac.shape else np.inf
    # what the check would see of a zero imported P_j or a skipped off-part column: A_c from the part-local matrix
    dropped = R.coarse_replay(R.part_local_matrix(A, N, nd, nres, parts), op.P)
    res[tag + "_Ac"] = (err, float(np.linalg.norm(dropped - op.Ac) / np.linalg.norm(op.Ac)), op.Ac.shape[0], cond, total)
    mine = owned_unknowns(parts[rank]["gid"], N, nd, nres)
    v = np.random.default_rng(13).standard_normal(A.shape[0])          # the same vector on every rank
    errs = []
    for s in sweeps:
        set_precond(asm, PARTS, s)
        rca, y = part_apply(asm, ls, v[mine], no)
        op.sgs.sweeps = s
        y_ref, y_coarse = op.apply(v)[mine], op.sgs.apply(v)[mine]     # (the second: the sweeps alone, without the coarse correction)
        errs.append((rca, s, float(np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)), float(np.linalg.norm(y_coarse - y_ref) / np.linalg.norm(y_ref))))
    op.sgs.sweeps = 1
    set_precond(asm, PARTS, 1)
    res[tag + "_op"] = errs
    print("%s rank %d: owned %d of %d local nodes, aggregates %d base %d of %d, n_c %d, cond(A_c) %.3e, |A_c - P^T A P|_F / |P^T A P|_F %.3e "
          "(off-part columns dropped: %.3e), operator errors %s, bound %.3e" %
          (tag, rank, no, asm.nnodes, nagg, base, total, op.Ac.shape[0], cond, err, res[tag + "_Ac"][1],
           ", ".join("%d sweeps %.3e (no coarse correction: %.3e)" % e[1:] for e in errs), 100.0 * EPS * cond), flush=True)
    return op, A, b, allp


def assert_coarse(out, world, tag, nc):
    """the assertions on what coarse_checks recorded, for every rank"""
    from calibr8_amd import lib
    bases = np.concatenate([[0], np.cumsum([out[r][tag + "_agg"][1] for r in range(world)])])
    for r in range(world):
        ok, nagg, base, total = out[r][tag + "_agg"]
        assert ok and nagg > 0, (tag, r, out[r][tag + "_agg"])                   # the three passes on the owned sub-graph
        assert base == bases[r] and total == bases[-1], (tag, r, base, total, bases)
        assert out[r][tag + "_Ac_rc"] == lib.C8_OK
        assert out[r][tag + "_Ac_bytes"] == out[0][tag + "_Ac_bytes"], (tag, r)  # the same matrix on every rank
        err, dropped, n_c, cond, _ = out[r][tag + "_Ac"]
        assert n_c == nc * bases[-1]
        assert err < 1e-12, (tag, r, err)
        assert dropped > 1e-3, (tag, r, dropped)                                 # the check sees a missing off-part column
        for rca, sweeps, e, without in out[r][tag + "_op"]:
            assert rca == lib.C8_OK
            assert e <= 100.0 * EPS * cond, (tag, r, sweeps, e, cond)
            assert without > 1e-3, (tag, r, sweeps, without)                     # ... and a missing coarse correction


# ---- 1. one rank with a halo: the single-part kind ---------------------------------------------------------------------------
def test_one_rank_with_a_halo_is_the_single_part_two_level_kind():
    from calibr8_amd import Assembler, lib
    import calibr8_amd.distributed as D
    from test_gpu_krylov import system_case
    from test_gpu_krylov_two_level import device_aggregates as single_aggregates, device_coarse_matrix as single_coarse_matrix
    et, c, conn, model, params, spec, _ = system_case((16, 4, 4))
    part = D.part_from_global(c, conn, np.zeros(len(conn), dtype=np.int32), 0, 1)
    plan = D.HaloPlan(part, None)
    asm = Assembler(et, plan.coords, part.conn, model, params)
    comm = D.Comm.host(None, 0, 1)
    halo = D.Halo(plan, asm.rowptr[1][1], asm.colidx[1][1], asm, comm)
    S = dict(c=c, part=part, plan=plan, asm=asm, comm=comm, halo=halo)
    ls = part_system(S, spec)
    set_precond(asm, PARTS, 1)
    assert asm.krylov_preconditioner == "two_level_parts"
    agg, nagg, base, total = device_aggregates(asm, asm.nnodes)
    rc_m, Ac = device_coarse_matrix(asm, ls)
    v = np.random.default_rng(13).standard_normal(asm.nnodes * 4)
    rc_a, y = part_apply(asm, ls, v, asm.nnodes)
    rc, info, dx = solve_parts(asm, ls)
    a1, l1 = system((16, 4, 4))[:2]
    agg1, nagg1 = single_aggregates(a1)
    Ac1 = single_coarse_matrix(a1, l1)
    with precond(a1, TWO_LEVEL):
        rc_a1, y1 = device_apply(a1, l1, v)
        rc1, i1, _ = raw_solve(a1, l1, new_dx(a1))
    close(S)
    cond = np.linalg.cond(Ac1)
    e_ac, e_op = np.linalg.norm(Ac - Ac1) / np.linalg.norm(Ac1), np.linalg.norm(y - y1) / np.linalg.norm(y1)
    print("one rank with a halo: aggregates %d / %d, A_c difference %.3e, operator difference %.3e (bound %.3e), iterations %d / %d" %
          (nagg, nagg1, e_ac, e_op, 100.0 * EPS * cond, info[0], i1.iters))
    assert rc == lib.C8_OK and rc1 == lib.C8_OK and rc_m == lib.C8_OK and rc_a == lib.C8_OK and rc_a1 == lib.C8_OK
    assert (base, total) == (0, nagg) and nagg == nagg1 and np.array_equal(agg, agg1)
    assert e_ac < 1e-12
    assert e_op <= 100.0 * EPS * cond
    assert abs(info[0] - i1.iters) <= 1


# ---- 2, 3, 6 (first half), 7, 8 (second half): two parts of notched_bar(16, 4, 4) ---------------------------------------------
def never_switched(rank, world, spec_kind):
    """the bytes and the count of a two-part solve on a context that only ever had `spec_kind`"""
    S, spec = bar_parts(rank, world)
    ls = part_system(S, spec)
    set_precond(S["asm"], spec_kind, 1)
    rc, info, dx = solve_parts(S["asm"], ls)
    out = (rc, info[0], owned_bytes(S["asm"], dx, S["part"].nowned))
    close(S)
    return out


def bar_worker(rank, world, port, out, full):
    init(rank, world, port)
    try:
        import scipy.sparse.linalg as spla
        from calibr8_amd import lib
        S, spec = bar_parts(rank, world)
        asm, no = S["asm"], S["part"].nowned
        L = asm.L
        res = {"no": no, "n": asm.nnodes}
        ls = part_system(S, spec)
        set_precond(asm, PARTS, 1)
        rc, info, dx = solve_parts(asm, ls)
        res["rc"], res["info"], res["err"] = rc, info, L.c8_last_error().decode() if rc else ""
        res["x1"] = owned_bytes(asm, dx, no)
        if not full:
            close(S)
            out[rank] = res
            return
        rc2, info2, dx2 = solve_parts(asm, ls)
        res["x2"], res["rc2"], res["iters2"] = owned_bytes(asm, dx2, no), rc2, info2[0]
        op, A, b, allp = coarse_checks(S, ls, world, rank, res, "k1", sweeps=(1, 2), dx=dx)
        if rank == 0:
            res["k1"] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "two parts, two-level over parts, K1")
            count = [0]

            def cb(_):
                count[0] += 1
            xs, flag = spla.bicgstab(A, b, rtol=REL_TOL, atol=0.0, maxiter=20000, M=spla.LinearOperator(A.shape, matvec=op.apply), callback=cb)
            res["scipy"] = (count[0], flag)
        # the part-local Gauss-Seidel count on the same system
        set_precond(asm, SGS, 1)
        rcs, info_s, _ = solve_parts(asm, ls)
        res["sgs"] = (rcs, info_s[0])
        # switching: other -> kind 7 -> other gives the bytes of a context that never switched
        res["switch"] = {}
        for name, other in (("jacobi", JACOBI), ("sgs", SGS)):
            set_precond(asm, other, 1)
            set_precond(asm, PARTS, 0)                      # sweeps <= 0: one sweep
            rct, info_t, dxt = solve_parts(asm, ls)
            set_precond(asm, other, 1)
            rco, info_o, dxo = solve_parts(asm, ls)
            res["switch"][name] = ((rct, info_t[0], owned_bytes(asm, dxt, no)), (rco, info_o[0], owned_bytes(asm, dxo, no)),
                                   never_switched(rank, world, other))
        # refusals with a halo attached: the single-part coarse kinds, and the single-part call with kind 7
        sy = ls.c_struct()
        ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
        ref = []
        for kind in (TWO_LEVEL, MULTILEVEL):
            set_precond(asm, kind, 1)
            rck, infok, _ = solve_parts(asm, ls)
            ref.append((rck, infok[0], L.c8_last_error().decode()))
        set_precond(asm, PARTS, 1)
        ki = lib.KrylovInfo()
        rck = L.c8_krylov_solve(asm.h, C.byref(sy), ptrs, None, C.byref(ki))
        ref.append((rck, ki.iters, L.c8_last_error().decode()))
        res["refused"] = ref
        # the K3 system of the same mesh
        ls3 = part_system(S, spec, adjoint=True)
        rc3, info3, dx3 = solve_parts(asm, ls3)
        res["rc3"], res["info3"] = rc3, info3
        allp3 = gather_pieces(world, owned_piece(S, ls3, dx3))
        if rank == 0:
            res["k3"] = check_contract(allp3, S["part"].num_global_nodes, asm.neq, asm.nres, info3, "two parts, two-level over parts, K3")
        # one owned node's diagonal block zeroed on rank 1 only: every rank returns the same refusal
        node = no // 2
        if rank == 1:
            zero_node_block(asm, ls, node)
        rcb, infob, _ = solve_parts(asm, ls)
        res["singular"] = (rcb, infob[0], L.c8_last_error().decode(), node)
        rcp, _ = part_apply(asm, ls, np.ones(no * 4), no)
        res["singular_apply"] = (rcp, L.c8_last_error().decode())
        set_precond(asm, JACOBI)
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def bar_run():
    return spawn(bar_worker, 2, True)


def test_two_part_aggregates_coarse_matrix_and_operator(bar_run):
    for r in range(2):
        assert bar_run[r]["no"] < bar_run[r]["n"]          # there are ghost or phantom columns
    assert_coarse(bar_run, 2, "k1", 7)


def test_two_part_solve_meets_the_contract(bar_run):
    from calibr8_amd import lib
    for r in range(2):
        assert bar_run[r]["rc"] == lib.C8_OK and bar_run[r]["rc3"] == lib.C8_OK, (r, bar_run[r]["err"])
    assert bar_run[0]["info"] == bar_run[1]["info"] and bar_run[0]["info3"] == bar_run[1]["info3"]
    assert bar_run[0]["k1"]["n"] == 1580
    assert_contract(bar_run[0]["k1"], "K1")
    assert_contract(bar_run[0]["k3"], "K3")


def test_two_part_iteration_counts(bar_run):
    """device <= 2 x SciPy BiCGStab with the numpy operator (the margin of test_iteration_counts_beside_scipy_bicgstab) and
    strictly fewer than the two-part device solve with the part-local Gauss-Seidel sweeps alone; the ratio is printed"""
    from calibr8_amd import lib
    it, (sc, flag), (rcs, sgs) = bar_run[0]["info"][0], bar_run[0]["scipy"], bar_run[0]["sgs"]
    print("notched_bar(16, 4, 4) over two parts, K1: device iterations two-level over parts %d, part-local SGS %d (ratio %.2f), "
          "SciPy BiCGStab with the numpy operator %d (flag %d); K3: %d" % (it, sgs, sgs / it, sc, flag, bar_run[0]["info3"][0]))
    assert flag == 0 and rcs == lib.C8_OK
    assert it <= 2 * sc
    assert it < sgs


def test_two_part_solve_is_reproducible(bar_run):
    """two solves in one process group and one in a fresh group: equal bytes of dx on the owned nodes, equal counts"""
    again = spawn(bar_worker, 2, False)
    for r in range(2):
        assert bar_run[r]["rc2"] == 0 and again[r]["rc"] == 0
        assert bar_run[r]["x1"] == bar_run[r]["x2"] and bar_run[r]["info"][0] == bar_run[r]["iters2"], r
        assert again[r]["x1"] == bar_run[r]["x1"] and again[r]["info"][0] == bar_run[r]["info"][0], r


@pytest.mark.parametrize("other", ["jacobi", "sgs"])
def test_switching_kinds_leaves_the_other_kinds_as_they_were(bar_run, other):
    for r in range(2):
        (rct, it_t, xt), (rco, it_o, xo), (rcn, it_n, xn) = bar_run[r]["switch"][other]
        assert rct == 0 and rco == 0 and rcn == 0
        assert it_t == bar_run[r]["info"][0] and xt == bar_run[r]["x1"]     # sweeps <= 0 is one sweep: the first solve again
        assert it_o == it_n and xo == xn, (r, other, it_o, it_n)
        assert it_t < it_o


def test_refusals_with_a_halo_are_collective(bar_run):
    from calibr8_amd import lib
    for r in range(2):
        two, multi, single = bar_run[r]["refused"]
        assert two[0] == lib.C8_ERR_UNSUPPORTED and two[1] == 0 and "halo" in two[2] and "two-level" in two[2], (r, two)
        assert multi[0] == lib.C8_ERR_UNSUPPORTED and multi[1] == 0 and "halo" in multi[2] and "multilevel" in multi[2], (r, multi)
        assert single[0] == lib.C8_ERR_UNSUPPORTED and single[1] == 0 and "halo" in single[2], (r, single)
        rc, iters, msg, _ = bar_run[r]["singular"]
        node = bar_run[1]["singular"][3]   # rank 1's local id
        assert rc == lib.C8_ERR_ARG and iters == 0, (r, bar_run[r]["singular"])
        assert ("node %d " % node) in msg and "rank 1" in msg, (r, msg)
        rcp, msgp = bar_run[r]["singular_apply"]
        assert rcp == lib.C8_ERR_ARG and ("node %d " % node) in msgp and "rank 1" in msgp, (r, msgp)


# ---- 4. four parts: phantom columns owned by three other ranks -----------------------------------------------------------------
def brick_worker(rank, world, port, out):
    init(rank, world, port)
    try:
        S = setup_part(rank, world, (6, 6, 4), (2, 2, 1))
        asm = S["asm"]
        sets = S["sets"]
        spec = [(0, d, sets["xmin"]) for d in range(3)] + [(0, 0, sets["xmax"])]
        ls = part_system(S, spec)
        set_precond(asm, PARTS, 1)
        rc, info, dx = solve_parts(asm, ls)
        res = {"rc": rc, "info": info, "err": asm.L.c8_last_error().decode() if rc else ""}
        op, A, b, allp = coarse_checks(S, ls, world, rank, res, "k1", dx=dx)
        # a node of this mesh has columns owned by three other ranks
        rp, ci, no = asm.rowptr[1][1], asm.colidx[1][1], S["part"].nowned
        gid = S["plan"].node_gid
        gowner = np.full(S["part"].num_global_nodes, -1)
        for r_, q in enumerate(allp):
            gowner[q["gid"][: q["no"]]] = r_
        res["others"] = max(len(set(gowner[gid[ci[rp[n]:rp[n + 1]]]].tolist()) - {rank}) for n in range(no))
        if rank == 0:
            res["k1"] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "brick(6, 6, 4) over 2 x 2 x 1, two-level over parts")
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_four_parts():
    from calibr8_amd import lib
    out = spawn(brick_worker, 4)
    for r in range(4):
        assert out[r]["rc"] == lib.C8_OK, (r, out[r]["err"])
        assert out[r]["info"] == out[0]["info"], r
    assert max(out[r]["others"] for r in range(4)) == 3
    assert_coarse(out, 4, "k1", 7)
    assert_contract(out[0]["k1"], "brick(6, 6, 4) over 2 x 2 x 1")


# ---- 5 and 8 (first half): two parts of notch2D_tri3, NC = 4 and 3; the cap ------------------------------------------------------
CAP_BRICK = 30   # brick(30, 30, 30) in two x-slabs: 726 + 605 aggregates, n_c 9317; brick(29, 29, 29): 600 + 500, n_c 7700


def hex_graph(conn, n):
    import scipy.sparse as sp
    r, c = np.repeat(conn, conn.shape[1], axis=1).ravel(), np.tile(conn, (1, conn.shape[1])).ravel()
    G = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    G.sum_duplicates()
    G.sort_indices()
    return G.indptr, G.indices


def brick_slabs(n):
    from meshes import brick
    c, conn, s = brick(n, n, n)
    ep = (c[conn].mean(axis=1)[:, 0] > 0.5 * (c[:, 0].min() + c[:, 0].max())).astype(np.int32)
    return c, conn, ep


def host_aggregate_count(n):
    """aggregates of brick(n, n, n) in two x-slabs by the host rule, on the CPU"""
    c, conn, ep = brick_slabs(n)
    owner = np.full(len(c), 2)
    for r in (1, 0):
        owner[np.unique(conn[ep == r])] = r       # lowest part id wins (part_from_global)
    return sum(q["nagg"] for q in R.parts_of_graph(*hex_graph(conn, len(c)), owner, 2))


def tri_cap_worker(rank, world, port, out):
    init(rank, world, port)
    try:
        from calibr8_amd import lib
        from parity_cases import HILL_PS
        res = {}
        c, conn, sets = golden("notch2D_tri3.json")
        ep = (c[conn].mean(axis=1)[:, 0] > 0.5 * (c[:, 0].min() + c[:, 0].max())).astype(np.int32)
        spec = [(0, 0, sets["xmin"]), (0, 1, sets["ymin"]), (0, 1, sets["ymax"])]
        for tag, model, params in (("mechanics", "small_J2", J2), ("plane_stress", "small_hill_plane_stress", HILL_PS)):
            S = make_part(rank, world, 3, c, conn, ep, model, params)
            asm = S["asm"]
            ls = part_system(S, spec)
            set_precond(asm, PARTS, 1)
            rc, info, dx = solve_parts(asm, ls)
            res[tag + "_rc"], res[tag + "_info"], res[tag + "_nres"] = rc, info, asm.nres
            res[tag + "_err"] = asm.L.c8_last_error().decode() if rc else ""
            op, A, b, allp = coarse_checks(S, ls, world, rank, res, tag, dx=dx)
            if rank == 0:
                res[tag] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "notch2D_tri3 over two parts, " + tag)
            close(S)
        # the cap: the system is never assembled, nothing is iterated, every rank returns the same refusal
        c, conn, ep = brick_slabs(CAP_BRICK)
        S = make_part(rank, world, 8, c, conn, ep, "small_J2", J2)
        asm, no = S["asm"], S["part"].nowned
        set_precond(asm, PARTS, 1)
        agg, nagg, base, total = device_aggregates(asm, no)          # reported above the cap too
        ls = asm.new_linsys()
        rc, info, _ = solve_parts(asm, ls)
        msg = asm.L.c8_last_error().decode()
        rcp, _ = part_apply(asm, ls, np.ones(no * 4), no)
        rcm, _ = device_coarse_matrix(asm, ls)
        res["cap"] = (rc, info[0], info[2], msg, rcp, rcm, nagg, base, total)
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def tri_cap_run():
    return spawn(tri_cap_worker, 2)


@pytest.mark.parametrize("tag,nres,nc", [("mechanics", 2, 4), ("plane_stress", 1, 3)])
def test_two_parts_on_the_2d_mesh(tri_cap_run, tag, nres, nc):
    from calibr8_amd import lib
    for r in range(2):
        assert tri_cap_run[r][tag + "_nres"] == nres
        assert tri_cap_run[r][tag + "_rc"] == lib.C8_OK, (r, tri_cap_run[r][tag + "_err"])
    assert tri_cap_run[0][tag + "_info"] == tri_cap_run[1][tag + "_info"]
    assert_coarse(tri_cap_run, 2, tag, nc)
    assert_contract(tri_cap_run[0][tag], tag)


def test_the_cap_is_refused_on_every_rank_before_anything_is_iterated(tri_cap_run):
    from calibr8_amd import lib
    below, above = host_aggregate_count(CAP_BRICK - 1), host_aggregate_count(CAP_BRICK)
    print("brick(%d) %d aggregates, brick(%d) %d aggregates over two parts: n_c %d and %d" % (CAP_BRICK - 1, below, CAP_BRICK, above, 7 * below, 7 * above))
    assert 7 * below <= COARSE_CAP < 7 * above          # the smallest brick above the cap, by the host rule on the CPU
    for r in range(2):
        rc, iters, status, msg, rcp, rcm, nagg, base, total = tri_cap_run[r]["cap"]
        assert total == above and (base == 0 if r == 0 else base == tri_cap_run[0]["cap"][6])
        assert rc == lib.C8_ERR_UNSUPPORTED and status == lib.C8_ERR_UNSUPPORTED and iters == 0, (r, msg)
        assert ("n_c = %d" % (7 * above)) in msg and "8192" in msg, msg
        assert rcp == lib.C8_ERR_UNSUPPORTED and rcm == lib.C8_ERR_UNSUPPORTED


# ---- 9. the step drivers ---------------------------------------------------------------------------------------------------------
def driver_worker(rank, world, port, out):
    """the deck of test_gpu_krylov_parts.py::driver_worker_device with preconditioner="two_level_parts" """
    init(rank, world, port)
    try:
        from calibr8_amd import Assembler, distributed_device_solver, scipy_solver
        from calibr8_amd.primal import PrimalDriver, adjoint_gradient
        S = setup_part(rank, world, (6, 4, 3), (2, 1, 1), jig=0.02)
        c, conn, part, plan, asm, comm = (S[k] for k in ("c", "conn", "part", "plan", "asm", "comm"))
        gid, no = plan.node_gid, part.nowned
        lc = c[gid]
        lo, hi = c.min(axis=0), c.max(axis=0)

        def local_sets(coords):
            def of(name):
                ax, side = "xyz".index(name[0]), name[1:]
                v = lo[ax] if side == "min" else hi[ax]
                return np.nonzero(np.abs(coords[:, ax] - v) < 1e-9)[0].astype(np.int32)
            return of

        act = [0, 1, 2, 3]
        asm.set_active(0, act)
        asm.set_stage_chunk(asm.nelems)
        asm.set_gather_early_nodes(no, part.ntouched)
        solver = distributed_device_solver(asm, preconditioner="two_level_parts")
        drv = PrimalDriver(asm, bcs_for(local_sets(lc), lc), solver=solver)
        drv.solve(2)
        J = comm.allreduce(np.array([drv.qoi()]))[0]
        primal_solves = solver.solves
        grad = comm.allreduce(adjoint_gradient(drv, len(act)))
        res = {"iters": list(drv.newton_iters), "J": float(J), "grad": grad, "primal_solves": primal_solves, "solves": solver.solves,
               "total_iters": solver.total_iters, "status": solver.last.status, "kind": asm.krylov_preconditioner}
        ref = Assembler(8, c, conn, "small_J2", J2)
        ref.set_active(0, act)
        rdrv = PrimalDriver(ref, bcs_for(local_sets(c), c), solver=scipy_solver(ref))
        rdrv.solve(2)
        res["ref_iters"], res["ref_J"], res["ref_grad"] = list(rdrv.newton_iters), rdrv.qoi(), adjoint_gradient(rdrv, len(act))
        torch.cuda.synchronize()
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_step_drivers_over_two_parts_with_the_two_level_preconditioner():
    out = spawn(driver_worker, 2)
    for r in range(2):
        res = out[r]
        print("rank %d: Newton %s / %s, linear solves %d (primal %d), BiCGStab iterations %d, J %.16e / %.16e" %
              (r, res["iters"], res["ref_iters"], res["solves"], res["primal_solves"], res["total_iters"], res["J"], res["ref_J"]))
        assert res["kind"] == "two_level_parts"
        assert res["iters"] == res["ref_iters"] and max(res["iters"]) > 2, (r, res["iters"], res["ref_iters"])
        assert abs(res["J"] / res["ref_J"] - 1.0) < 1e-8, (r, res["J"], res["ref_J"])
        assert np.abs(res["grad"] - res["ref_grad"]).max() < 1e-7 * np.abs(res["ref_grad"]).max(), (r, res["grad"], res["ref_grad"])
        assert res["primal_solves"] > 0 and res["solves"] == res["primal_solves"] + 2 and res["status"] == 0, (r, res)
