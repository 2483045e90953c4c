"""`-m gpu`: the multilevel preconditioner of the device solve over the parts of a multi-part mesh
(C8_PRECOND_MULTILEVEL_PARTS) against its definition in include/c8.h, replayed in numpy on the
gathered matrix (tests/krylov_parts_multilevel_replay.py): the per-part level 0, the replicated levels from 1 down with
their aggregates and colours, every A_l = P^T A P, the operator on the owned entries with two controls, the contract of the
solve, iteration counts, the cap of the two-level kind lifted, reproducible bytes, switching, the collective refusals and
one driver deck.  The harness is that of test_gpu_krylov_two_level_parts.py: the ranks share the card over the host
transport, several cases share one spawn (five spawns, at most four processes); every spawn has a time limit of its own and
a worker that fails ends its tests.  Every test fails on a library without the kind (the setter refuses 9).

Recorded on one MI355X: see the tables of DESIGN.md section 13g."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import krylov_parts_multilevel_replay as M  # noqa: E402
import krylov_parts_replay as R  # noqa: E402
from test_gpu_distributed import bcs_for, free_port, setup_part  # noqa: E402
from test_gpu_krylov import REL_TOL, golden, new_dx, raw_solve, system_case  # noqa: E402
from test_gpu_krylov_multilevel import Multilevel, device_level_matrix, device_levels, set_levels  # noqa: E402
from test_gpu_krylov_parts import (J2, assert_contract, check_contract, close, gather_pieces, init, make_part, owned_piece,  # noqa: E402
                                   part_system, solve_parts)
from test_gpu_krylov_sgs import JACOBI, SGS, device_apply, device_colors, precond, set_precond, system  # noqa: E402
from test_gpu_krylov_two_level_parts import device_aggregates, owned_bytes, owned_unknowns, part_apply, zero_node_block  # noqa: E402

pytestmark = pytest.mark.gpu
TWO_LEVEL, MULTILEVEL, PARTS, MLP = 3, 5, 7, 9   # C8_PRECOND_TWO_LEVEL, _MULTILEVEL, _TWO_LEVEL_PARTS, _MULTILEVEL_PARTS
EPS = np.finfo(np.float64).eps


def spawn(fn, world, *args, limit=240.0):
    """test_gpu_distributed.spawn with a time limit: the workers are ended when it runs out; a worker that fails ends the
    others and raises here, so that nothing more runs on the card for the tests that share this spawn"""
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(fn, args=(world, free_port(), out) + args, nprocs=world, join=False)
    deadline = time.monotonic() + limit
    while not ctx.join(timeout=2.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("%s: the workers did not finish within %.0f s" % (fn.__name__, limit))
    assert len(out) == world
    return dict(out)


def bar(rank, world, n=(16, 4, 4)):
    """bar_parts of test_gpu_krylov_parts.py for any notched_bar: two x-slabs of equal width"""
    et, c, conn, model, params, spec, _ = system_case(n)
    ep = (c[conn].mean(axis=1)[:, 0] > 0.5 * (c[:, 0].min() + c[:, 0].max())).astype(np.int32)
    return make_part(rank, world, et, c, conn, ep, model, params), spec


def gathered(S, ls, dx, world):
    """the gathered system and the parts of the replay from the ranks' pieces: (A, b, parts, pieces)"""
    asm, no = S["asm"], S["part"].nowned
    agg, nagg, base, total = device_aggregates(asm, no)
    piece = owned_piece(S, ls, dx)
    piece.update(agg=agg, nagg=nagg, base=base, colors=device_colors(asm))
    allp = gather_pieces(world, piece)
    A, b = R.gathered_matrix(allp, S["part"].num_global_nodes, asm.neq, asm.nres)
    parts = [{"gid": q["gid"][: q["no"]], "agg": q["agg"], "nagg": q["nagg"], "base": q["base"], "colors": q["colors"]} for q in allp]
    return A, b, parts, allp


def host_residual(pieces, N, neq, nres):
    """|b - A x| and |b| of the gathered system as check_contract forms them: rank by rank, every row in its own (local)
    column order, the order the solver defines the residual by"""
    import scipy.sparse as sp
    off = [0, N * neq[0]]
    xg = np.zeros(N * sum(neq[:nres]))
    for q in pieces:
        for i in range(nres):
            xg[off[i] + np.repeat(q["gid"][: q["no"]], neq[i]) * neq[i] + np.tile(np.arange(neq[i]), q["no"])] = q["x"][i]
    rr, bb = 0.0, 0.0
    for q in pieces:
        xl = [xg[off[j] + (q["gid"][:, None] * neq[j] + np.arange(neq[j])).ravel()] for j in range(nres)]
        blocks = [[sp.csr_matrix(q["A"][(i, j)][::-1], shape=(q["no"] * neq[i], q["n"] * neq[j])) for j in range(nres)] for i in range(nres)]
        rl = np.concatenate(q["b"]) - sp.bmat(blocks, format="csr") @ np.concatenate(xl)
        rr += float(rl @ rl)
        bb += float(np.concatenate(q["b"]) @ np.concatenate(q["b"]))
    return np.sqrt(rr), np.sqrt(bb)


def same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def level_checks(S, ls, world, rank, res, tag, coarse_max, sweeps=(1,), dx=None):
    """What every mesh is checked for with the kind selected and `coarse_max` set: level 0 against the replay on the owned
    sub-graph and the prefix sums, the replicated levels (node counts, aggregates, colours -- functions of the whole level
    graph -- and the block pattern of the downloaded A_1 inside the replayed level-1 graph), every A_l against numpy P^T A P
    on the gathered matrix, the operator on the owned entries with the two controls.  Returns the numpy operator."""
    asm, no = S["asm"], S["part"].nowned
    N, nd, nres = S["part"].num_global_nodes, asm.ndims, asm.nres
    set_levels(asm, coarse_max, 0)
    set_precond(asm, MLP, 1)
    agg, nagg, base, total = device_aggregates(asm, no)
    ref, nref = R.owned_aggregates(asm.rowptr[1][1], asm.colidx[1][1], no)
    res[tag + "_agg"] = (bool(nagg == nref and np.array_equal(agg, ref)), nagg, base, total)
    dev = device_levels(asm)
    A, b, parts, allp = gathered(S, ls, dx or new_dx(asm), world)
    op = M.MultilevelParts(A, S["c"], nd, nres, parts, coarse_max=coarse_max)
    nc, last = op.nc, len(op.levels) - 1
    ok = len(dev) == len(op.levels) and dev[0][0] == no and np.array_equal(dev[0][1], agg) and same_lists(dev[0][2], device_colors(asm))
    for lev in range(1, min(len(dev), len(op.levels))):
        n, a, colors = dev[lev]
        L = op.levels[lev]
        ok = ok and n == L["n"]
        if lev == last:
            ok = ok and a is None and colors == []
        else:
            ok = ok and a is not None and np.array_equal(a, L["agg"]) and same_lists(colors, L["colors"])
    res[tag + "_levels"] = (bool(ok), [d[0] for d in dev], [no] + [L["n"] for L in op.levels[1:]])
    mats = []
    for lev in range(1, len(dev)):
        Ad = device_level_matrix(asm, ls, lev)                         # (collective)
        ref_l = op.A[lev] if lev < len(op.A) else None
        err = float(np.linalg.norm(Ad - ref_l) / np.linalg.norm(ref_l)) if ref_l is not None and Ad.shape == ref_l.shape else np.inf
        inside = True
        if lev == 1 and last > 1:                                      # a block outside the replayed level-1 graph is zero
            L1 = op.levels[1]
            mask = np.zeros((L1["n"], L1["n"]), dtype=bool)
            mask[np.repeat(np.arange(L1["n"]), np.diff(L1["rp"])), L1["ci"]] = True
            blocks = np.abs(Ad.reshape(L1["n"], nc, L1["n"], nc)).max(axis=(1, 3))
            inside = bool((blocks[~mask] == 0.0).all())
        mats.append((lev, Ad.shape[0], err, inside, Ad.tobytes()))
    res[tag + "_A"] = mats
    # the controls: the levels below level 1 left out; the off-part columns dropped from A_1 (a zero imported P_j)
    dropped = M.MultilevelParts(A, S["c"], nd, nres, parts, coarse_max=coarse_max,
                                A1=R.coarse_replay(R.part_local_matrix(A, N, nd, nres, parts), op.P0))
    mine = owned_unknowns(parts[rank]["gid"], N, nd, nres)
    v = np.random.default_rng(13).standard_normal(A.shape[0])          # the same vector on every rank
    errs = []
    for s in sweeps:
        set_precond(asm, MLP, s)
        rca, y = part_apply(asm, ls, v[mine], no)
        op.set_sweeps(s), dropped.set_sweeps(s)
        y_ref = op.apply(v)[mine]
        rel = lambda z: float(np.linalg.norm(z - y) / np.linalg.norm(y_ref))
        errs.append((rca, s, rel(y_ref), rel(op.apply(v, lower=False)[mine]), rel(dropped.apply(v)[mine])))
    op.set_sweeps(1)
    set_precond(asm, MLP, 1)
    res[tag + "_op"] = (errs, op.cond)
    print("%s rank %d: owned %d of %d local nodes, aggregates %d base %d of %d, nodes per level %s (replay %s), cond(last) %.3e cond(blocks) %.3e, "
          "A_l errors %s, operator %s, bound %.3e" %
          (tag, rank, no, asm.nnodes, nagg, base, total, res[tag + "_levels"][1], res[tag + "_levels"][2], op.cond_last, op.cond_blocks,
           ", ".join("level %d (n %d) %.3e" % m[:3] for m in mats),
           ", ".join("%d sweeps %.3e (device against: no lower levels %.3e, off-part columns dropped %.3e)" % e[1:] for e in errs),
           100.0 * EPS * op.cond), flush=True)
    return op, A, b, allp


def assert_levels(out, world, tag, nc, want=None, min_levels=3, control=None):
    """The assertions on what level_checks recorded, for every rank.  `control`: what the two controls must differ from the
    device by.  The operator check accepts an error up to its bound, so it sees a skipped level or a missing off-part column
    exactly when that fault moves the result by more than the bound: the default asks for ten times the bound of the mesh
    (the factor covers the rounding of the control's own replay); the two-part bar passes the 1e-3 its CPU replay gave."""
    from calibr8_amd import lib
    bases = np.concatenate([[0], np.cumsum([out[r][tag + "_agg"][1] for r in range(world)])])
    for r in range(world):
        ok, nagg, base, total = out[r][tag + "_agg"]
        assert ok and nagg > 0, (tag, r, out[r][tag + "_agg"])                   # the three passes on the owned sub-graph
        assert base == bases[r] and total == bases[-1], (tag, r, base, total, bases)
        ok, dev_n, ref_n = out[r][tag + "_levels"]
        assert ok, (tag, r, dev_n, ref_n)
        assert dev_n == ref_n and len(dev_n) >= min_levels and dev_n[1] == total, (tag, r, dev_n, ref_n)
        if want is not None:
            assert dev_n[1:] == want, (tag, r, dev_n, want)                       # the node counts of the CPU replay of the issue
        assert out[r][tag + "_levels"][1][1:] == out[0][tag + "_levels"][1][1:]
        assert len(out[r][tag + "_A"]) == len(dev_n) - 1
        for (lev, n, err, inside, raw), (_, _, _, _, raw0) in zip(out[r][tag + "_A"], out[0][tag + "_A"]):
            assert n == nc * dev_n[lev], (tag, r, lev, n)
            assert raw == raw0, (tag, r, lev)                                     # the same matrix on every rank
            assert err < 1e-12, (tag, r, lev, err)
            assert inside, (tag, r, lev)
        errs, cond = out[r][tag + "_op"]
        differ = control if control is not None else 10.0 * 100.0 * EPS * cond
        for rca, sweeps, e, no_lower, dropped in errs:
            assert rca == lib.C8_OK
            assert e <= 100.0 * EPS * cond, (tag, r, sweeps, e, cond)
            if len(dev_n) > 2:
                assert no_lower > differ, (tag, r, sweeps, no_lower)             # the check sees a skipped level ...
            assert dropped > differ, (tag, r, sweeps, dropped)                    # ... and a missing off-part column


# ---- one rank with a halo: the single-part multilevel kind ---------------------------------------------------------------------
def test_one_rank_with_a_halo_is_the_single_part_multilevel_kind():
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
    set_levels(asm, 100, 0)
    set_precond(asm, MLP, 1)
    assert asm.krylov_preconditioner == "multilevel_parts"
    dev = device_levels(asm)
    mats = [device_level_matrix(asm, ls, lev) for lev in range(1, len(dev))]
    v = np.random.default_rng(13).standard_normal(asm.nnodes * 4)
    rc_a, y = part_apply(asm, ls, v, asm.nnodes)
    rc, info, dx = solve_parts(asm, ls)
    a1, l1, A1, b1 = system((16, 4, 4))
    set_levels(a1, 100, 0)
    try:
        with precond(a1, MULTILEVEL):
            dev1 = device_levels(a1)
            mats1 = [device_level_matrix(a1, l1, lev) for lev in range(1, len(dev1))]
            rc_a1, y1 = device_apply(a1, l1, v)
            rc1, i1, _ = raw_solve(a1, l1, new_dx(a1))
    finally:
        set_levels(a1)
    close(S)
    cond = Multilevel(a1, A1, 100, 8).cond     # what the device inverts: the numpy replay of the single-part kind
    e_op = np.linalg.norm(y - y1) / np.linalg.norm(y1)
    e_A = [float(np.linalg.norm(a - b) / np.linalg.norm(b)) for a, b in zip(mats, mats1)]
    print("one rank with a halo: nodes per level %s / %s, A_l differences %s, operator difference %.3e (bound %.3e), "
          "iterations %d / %d" % ([d[0] for d in dev], [d[0] for d in dev1], e_A, e_op, 100.0 * EPS * cond, info[0], i1.iters))
    assert rc == lib.C8_OK and rc1 == lib.C8_OK and rc_a == lib.C8_OK and rc_a1 == lib.C8_OK
    assert len(dev) == len(dev1) >= 3 and [d[0] for d in dev] == [d[0] for d in dev1]
    for (n, a, colors), (n1, a1_, colors1) in zip(dev, dev1):
        assert (a is None) == (a1_ is None) and (a is None or np.array_equal(a, a1_)) and same_lists(colors, colors1)
    assert len(e_A) == len(dev) - 1 and max(e_A) < 1e-12
    assert e_op <= 100.0 * EPS * cond
    assert abs(info[0] - i1.iters) <= 1


# ---- two parts of notched_bar(16, 4, 4) and (32, 8, 8) ---------------------------------------------------------------------------
def never_switched(rank, world, kind):
    """the bytes and the count of a two-part solve on a context that only ever had `kind` (default settings)"""
    S, spec = bar(rank, world)
    ls = part_system(S, spec)
    set_precond(S["asm"], kind, 1)
    rc, info, dx = solve_parts(S["asm"], ls)
    out = (rc, info[0], owned_bytes(S["asm"], dx, S["part"].nowned))
    close(S)
    return out


def scipy_count(A, b, op):
    import scipy.sparse.linalg as spla
    count = [0]

    def cb(_):
        count[0] += 1
    xs, flag = spla.bicgstab(A, b, rtol=REL_TOL, atol=0.0, maxiter=20000, M=spla.LinearOperator(A.shape, matvec=op.apply), callback=cb)
    return count[0], flag


def bar_worker(rank, world, port, out, full):
    init(rank, world, port)
    try:
        from calibr8_amd import lib
        S, spec = bar(rank, world)
        asm, no = S["asm"], S["part"].nowned
        L = asm.L
        res = {"no": no, "n": asm.nnodes}
        ls = part_system(S, spec)
        set_levels(asm, 100, 0)
        set_precond(asm, MLP, 1)
        rc, info, dx = solve_parts(asm, ls)
        res["rc"], res["info"], res["err"] = rc, info, L.c8_last_error().decode() if rc else ""
        res["x1"] = owned_bytes(asm, dx, no)
        if not full:
            close(S)
            out[rank] = res
            return
        rc2, info2, dx2 = solve_parts(asm, ls)
        res["x2"], res["rc2"], res["iters2"] = owned_bytes(asm, dx2, no), rc2, info2[0]
        op, A, b, allp = level_checks(S, ls, world, rank, res, "k1", 100, sweeps=(1, 2), dx=dx)
        if rank == 0:
            res["k1"] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "two parts, multilevel over parts, K1")
            res["scipy"] = scipy_count(A, b, op)
        # a changed coarse_max rebuilds the levels over parts: 26 / 3 / 1 with 20
        level_checks(S, ls, world, rank, res, "k1_20", 20, dx=dx)
        rc20, info20, _ = solve_parts(asm, ls)
        res["solve20"] = (rc20, info20[0])
        set_levels(asm, 100, 0)
        rcb, infob, dxb = solve_parts(asm, ls)
        res["back"] = (rcb, infob[0], owned_bytes(asm, dxb, no))
        # max_levels 2 over two parts is kind 7 in the bytes of dx and in the count
        set_levels(asm, 100, 2)
        n2 = [d[0] for d in device_levels(asm)]
        rcm, infom, dxm = solve_parts(asm, ls)
        set_precond(asm, PARTS, 1)
        rc7, info7, dx7 = solve_parts(asm, ls)
        res["two_levels"] = (n2, (rcm, infom[0], owned_bytes(asm, dxm, no)), (rc7, info7[0], owned_bytes(asm, dx7, no)))
        set_levels(asm, 100, 0)
        # the part-local Gauss-Seidel count on the same system
        set_precond(asm, SGS, 1)
        rcs, info_s, _ = solve_parts(asm, ls)
        res["sgs"] = (rcs, info_s[0])
        # switching: other -> kind 9 -> other gives the bytes of a context that never switched
        res["switch"] = {}
        for name, other in (("jacobi", JACOBI), ("sgs", SGS), ("two_level_parts", PARTS)):
            set_precond(asm, other, 1)
            set_precond(asm, MLP, 0)                        # sweeps <= 0: one sweep
            rct, info_t, dxt = solve_parts(asm, ls)
            set_precond(asm, other, 1)
            rco, info_o, dxo = solve_parts(asm, ls)
            res["switch"][name] = ((rct, info_t[0], owned_bytes(asm, dxt, no)), (rco, info_o[0], owned_bytes(asm, dxo, no)),
                                   never_switched(rank, world, other))
        # refusals with a halo attached: kind 8, the single-part coarse kinds, and the single-part call with kind 9
        res["eight"] = (L.c8_krylov_set_preconditioner(asm.h, 8, 1), L.c8_last_error().decode(), L.c8_krylov_get_preconditioner(asm.h))
        sy = ls.c_struct()
        ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
        ref = []
        for kind in (TWO_LEVEL, MULTILEVEL):
            set_precond(asm, kind, 1)
            rck, infok, _ = solve_parts(asm, ls)
            ref.append((rck, infok[0], L.c8_last_error().decode()))
        set_precond(asm, MLP, 1)
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
            res["k3"] = check_contract(allp3, S["part"].num_global_nodes, asm.neq, asm.nres, info3, "two parts, multilevel over parts, K3")
        # one owned node's diagonal block zeroed on rank 1 only: every rank returns the same refusal
        node = no // 2
        if rank == 1:
            zero_node_block(asm, ls, node)
        rcz, infoz, _ = solve_parts(asm, ls)
        res["singular"] = (rcz, infoz[0], L.c8_last_error().decode(), node)
        rcp, _ = part_apply(asm, ls, np.ones(no * 4), no)
        res["singular_apply"] = (rcp, L.c8_last_error().decode())
        set_precond(asm, JACOBI)
        close(S)
        # the larger bar: counts only
        S, spec = bar(rank, world, (32, 8, 8))
        asm, no = S["asm"], S["part"].nowned
        ls = part_system(S, spec)
        set_levels(asm, 100, 0)
        set_precond(asm, MLP, 1)
        rcl, infol, dxl = solve_parts(asm, ls)
        A, b, parts, allp = gathered(S, ls, dxl, world)
        set_precond(asm, SGS, 1)
        rcs, info_s, _ = solve_parts(asm, ls)
        set_precond(asm, MLP, 1)
        res["large"] = (rcl, infol[0], rcs, info_s[0], [d[0] for d in device_levels(asm)][1:])
        if rank == 0:
            res["large_scipy"] = scipy_count(A, b, M.MultilevelParts(A, S["c"], asm.ndims, asm.nres, parts, coarse_max=100))
        set_precond(asm, JACOBI)
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def bar_run():
    return spawn(bar_worker, 2, True)


def test_two_part_levels_matrices_and_operator(bar_run):
    for r in range(2):
        assert bar_run[r]["no"] < bar_run[r]["n"]          # there are ghost or phantom columns
        assert bar_run[r]["k1_agg"][1] == (14, 12)[r]
    assert_levels(bar_run, 2, "k1", 7, want=[26, 3], control=1e-3)


def test_a_changed_coarse_max_rebuilds_the_levels_over_parts(bar_run):
    assert_levels(bar_run, 2, "k1_20", 7, want=[26, 3, 1], control=1e-3)
    for r in range(2):
        rc20, it20 = bar_run[r]["solve20"]
        rcb, itb, xb = bar_run[r]["back"]
        assert rc20 == 0 and rcb == 0
        assert itb == bar_run[r]["info"][0] and xb == bar_run[r]["x1"], r      # ... and back: the first solve again


def test_two_part_solve_meets_the_contract(bar_run):
    from calibr8_amd import lib
    for r in range(2):
        assert bar_run[r]["rc"] == lib.C8_OK and bar_run[r]["rc3"] == lib.C8_OK, (r, bar_run[r]["err"])
    assert bar_run[0]["info"] == bar_run[1]["info"] and bar_run[0]["info3"] == bar_run[1]["info3"]
    assert bar_run[0]["k1"]["n"] == 1580
    assert_contract(bar_run[0]["k1"], "K1")
    assert_contract(bar_run[0]["k3"], "K3")


def test_two_part_iteration_counts(bar_run):
    """device <= 2 x SciPy BiCGStab with the numpy operator and strictly fewer than the two-part device solve with the
    part-local Gauss-Seidel sweeps alone, on both bars; the ratios are printed (CPU replay: 29 and 41 against 82 and 186)"""
    from calibr8_amd import lib
    it, (sc, flag), (rcs, sgs) = bar_run[0]["info"][0], bar_run[0]["scipy"], bar_run[0]["sgs"]
    rcl, itl, rcsl, sgsl, nodes = bar_run[0]["large"]
    scl, flagl = bar_run[0]["large_scipy"]
    print("two parts, K1, coarse_max 100: notched_bar(16, 4, 4) device iterations multilevel over parts %d, part-local SGS %d (ratio %.2f), SciPy "
          "BiCGStab with the numpy operator %d; K3: %d; coarse_max 20: %d; notched_bar(32, 8, 8) levels %s: %d, part-local SGS %d (ratio %.2f), SciPy %d" %
          (it, sgs, sgs / it, sc, bar_run[0]["info3"][0], bar_run[0]["solve20"][1], nodes, itl, sgsl, sgsl / itl, scl))
    assert flag == 0 and rcs == lib.C8_OK and flagl == 0 and rcl == lib.C8_OK and rcsl == lib.C8_OK
    assert nodes == [99, 5]
    assert it <= 2 * sc and it < sgs
    assert itl <= 2 * scl and itl < sgsl
    assert bar_run[1]["large"] == bar_run[0]["large"]


def test_two_levels_over_parts_are_the_two_level_kind_over_parts(bar_run):
    for r in range(2):
        n2, (rcm, itm, xm), (rc7, it7, x7) = bar_run[r]["two_levels"]
        assert len(n2) == 2 and n2[1] == 26
        assert rcm == 0 and rc7 == 0
        assert itm == it7 and xm == x7, (r, itm, it7)


def test_two_part_solve_is_reproducible(bar_run):
    """two solves in one process group and one in a fresh group: equal bytes of dx on the owned nodes, equal counts"""
    again = spawn(bar_worker, 2, False)
    for r in range(2):
        assert bar_run[r]["rc2"] == 0 and again[r]["rc"] == 0
        assert bar_run[r]["x1"] == bar_run[r]["x2"] and bar_run[r]["info"][0] == bar_run[r]["iters2"], r
        assert again[r]["x1"] == bar_run[r]["x1"] and again[r]["info"][0] == bar_run[r]["info"][0], r


@pytest.mark.parametrize("other", ["jacobi", "sgs", "two_level_parts"])
def test_switching_kinds_leaves_the_other_kinds_as_they_were(bar_run, other):
    for r in range(2):
        (rct, it_t, xt), (rco, it_o, xo), (rcn, it_n, xn) = bar_run[r]["switch"][other]
        assert rct == 0 and rco == 0 and rcn == 0
        assert it_t == bar_run[r]["info"][0] and xt == bar_run[r]["x1"]     # sweeps <= 0 is one sweep: the first solve again
        assert it_o == it_n and xo == xn, (r, other, it_o, it_n)


def test_refusals_with_a_halo_are_collective(bar_run):
    from calibr8_amd import lib
    for r in range(2):
        rc8, msg8, kind = bar_run[r]["eight"]
        assert rc8 == lib.C8_ERR_ARG and "unknown preconditioner 8" in msg8 and kind == PARTS, (r, bar_run[r]["eight"])
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


# ---- four parts: phantom columns owned by three other ranks -------------------------------------------------------------------
def brick_worker(rank, world, port, out):
    init(rank, world, port)
    try:
        S = setup_part(rank, world, (6, 6, 4), (2, 2, 1))
        asm = S["asm"]
        sets = S["sets"]
        spec = [(0, d, sets["xmin"]) for d in range(3)] + [(0, 0, sets["xmax"])]
        ls = part_system(S, spec)
        set_levels(asm, 100, 0)
        set_precond(asm, MLP, 1)
        rc, info, dx = solve_parts(asm, ls)
        res = {"rc": rc, "info": info, "err": asm.L.c8_last_error().decode() if rc else ""}
        op, A, b, allp = level_checks(S, ls, world, rank, res, "k1", 100, dx=dx)
        rp, ci, no = asm.rowptr[1][1], asm.colidx[1][1], S["part"].nowned
        gid = S["plan"].node_gid
        gowner = np.full(S["part"].num_global_nodes, -1)
        for r_, q in enumerate(allp):
            gowner[q["gid"][: q["no"]]] = r_
        res["others"] = max(len(set(gowner[gid[ci[rp[n]:rp[n + 1]]]].tolist()) - {rank}) for n in range(no))
        if rank == 0:
            res["k1"] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "brick(6, 6, 4) over 2 x 2 x 1, multilevel over parts")
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
    assert_levels(out, 4, "k1", 7, want=[18, 1])
    assert_contract(out[0]["k1"], "brick(6, 6, 4) over 2 x 2 x 1")


# ---- two parts of notch2D_tri3, NC = 4 and 3; the cap of the two-level kind lifted -----------------------------------------------
CAP_BRICK = 30     # brick(30, 30, 30) in two x-slabs: 726 + 605 aggregates, n_c 9317 for the two-level kind over parts
TRI_COARSE_MAX = 20


def cap_slabs():
    from meshes import brick, jiggle
    c, conn, s = brick(CAP_BRICK, CAP_BRICK, CAP_BRICK)
    ep = (c[conn].mean(axis=1)[:, 0] > 0.5 * (c[:, 0].min() + c[:, 0].max())).astype(np.int32)
    spec = [(0, d, s["xmin"]) for d in range(3)] + [(0, 0, s["xmax"])]
    return jiggle(c, s, 0.01), conn, ep, spec


def tri_cap_worker(rank, world, port, out):
    init(rank, world, port)
    try:
        from parity_cases import HILL_PS
        res = {}
        c, conn, sets = golden("notch2D_tri3.json")
        ep = (c[conn].mean(axis=1)[:, 0] > 0.5 * (c[:, 0].min() + c[:, 0].max())).astype(np.int32)
        spec = [(0, 0, sets["xmin"]), (0, 1, sets["ymin"]), (0, 1, sets["ymax"])]
        for tag, model, params in (("mechanics", "small_J2", J2), ("plane_stress", "small_hill_plane_stress", HILL_PS)):
            S = make_part(rank, world, 3, c, conn, ep, model, params)
            asm = S["asm"]
            ls = part_system(S, spec)
            set_levels(asm, TRI_COARSE_MAX, 0)
            set_precond(asm, MLP, 1)
            rc, info, dx = solve_parts(asm, ls)
            res[tag + "_rc"], res[tag + "_info"], res[tag + "_nres"] = rc, info, asm.nres
            res[tag + "_err"] = asm.L.c8_last_error().decode() if rc else ""
            op, A, b, allp = level_checks(S, ls, world, rank, res, tag, TRI_COARSE_MAX, dx=dx)
            if rank == 0:
                res[tag] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, "notch2D_tri3 over two parts, " + tag)
            close(S)
        # the cap: the two-level kind over parts is refused, this kind solves the system (default settings)
        c, conn, ep, spec = cap_slabs()
        S = make_part(rank, world, 8, c, conn, ep, "small_J2", J2)
        asm, no = S["asm"], S["part"].nowned
        ls = part_system(S, spec)
        set_precond(asm, PARTS, 1)
        rc7, info7, _ = solve_parts(asm, ls)
        msg7 = asm.L.c8_last_error().decode()
        set_precond(asm, MLP, 1)
        nodes = [d[0] for d in device_levels(asm)]
        rc, info, dx = solve_parts(asm, ls)
        msg = asm.L.c8_last_error().decode() if rc else ""
        allp = gather_pieces(world, owned_piece(S, ls, dx))
        hres = None
        if rank == 0:   # the residual of the gathered system (a direct solve of this size is no part of a quick test)
            r_, b_ = host_residual(allp, S["part"].num_global_nodes, asm.neq, asm.nres)
            hres = (float(r_ / b_), float(abs(info[4] / r_ - 1.0)), float(abs(info[3] / b_ - 1.0)), S["part"].num_global_nodes * 4)
        set_precond(asm, SGS, 1)
        rcs, info_s, _ = solve_parts(asm, ls)
        # max_levels 2 puts the last level above the cap: refused on every rank, nothing iterated
        set_levels(asm, 0, 2)
        set_precond(asm, MLP, 1)
        n2 = [d[0] for d in device_levels(asm)]           # reported above the cap too
        rcc, infoc, _ = solve_parts(asm, ls)
        msgc = asm.L.c8_last_error().decode()
        rcp, _ = part_apply(asm, ls, np.ones(no * 4), no)
        res["cap"] = dict(two=(rc7, info7[0], msg7), nodes=nodes, rc=rc, info=info, msg=msg, hres=hres, sgs=(rcs, info_s[0]),
                          refused=(n2, rcc, infoc[0], infoc[2], msgc, rcp))
        set_levels(asm)
        set_precond(asm, JACOBI)
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
        assert len(tri_cap_run[r][tag + "_levels"][2]) == 3            # the replay shows three levels with this coarse_max
    assert tri_cap_run[0][tag + "_info"] == tri_cap_run[1][tag + "_info"]
    assert_levels(tri_cap_run, 2, tag, nc)
    assert_contract(tri_cap_run[0][tag], tag)


def test_the_cap_of_the_two_level_kind_is_lifted(tri_cap_run):
    """two slabs of brick(30, 30, 30): kind 7 is refused (n_c 9317), kind 9 builds 1331 / 64 nodes on levels 1 / 2, meets the
    contract on the gathered matrix and needs at most half the iterations of the part-local sweeps (the bar that
    test_solves_the_mesh_the_two_level_kind_refuses sets for the single-part multilevel kind)"""
    from calibr8_amd import lib
    for r in range(2):
        cap = tri_cap_run[r]["cap"]
        rc7, it7, msg7 = cap["two"]
        assert rc7 == lib.C8_ERR_UNSUPPORTED and it7 == 0 and "n_c = 9317" in msg7, (r, cap["two"])
        assert cap["nodes"][1:] == [1331, 64], (r, cap["nodes"])
        assert cap["rc"] == lib.C8_OK and cap["info"][2] == lib.C8_OK, (r, cap["msg"])
        assert cap["info"] == tri_cap_run[0]["cap"]["info"]
        assert cap["sgs"][0] == lib.C8_OK and cap["sgs"] == tri_cap_run[0]["cap"]["sgs"]
    cap = tri_cap_run[0]["cap"]
    res, info_res, info_b, n = cap["hres"]
    print("brick(%d) over two parts (%d unknowns): nodes per level %s, multilevel over parts %d iterations, part-local SGS %d (ratio %.2f), "
          "host residual %.3e" % (CAP_BRICK, n, cap["nodes"], cap["info"][0], cap["sgs"][1], cap["sgs"][1] / cap["info"][0], res))
    assert res <= 1.01 * REL_TOL and info_res < 1e-9 and info_b < 1e-12      # (the bounds of assert_contract)
    assert 2 * cap["info"][0] <= cap["sgs"][1]


def test_a_last_level_above_the_cap_is_refused_on_every_rank(tri_cap_run):
    from calibr8_amd import lib
    for r in range(2):
        n2, rc, iters, status, msg, rcp = tri_cap_run[r]["cap"]["refused"]
        assert len(n2) == 2 and n2[1] == 1331
        assert rc == lib.C8_ERR_UNSUPPORTED and status == lib.C8_ERR_UNSUPPORTED and iters == 0, (r, msg)
        assert "n = 9317" in msg and "8192" in msg and "max_levels = 2" in msg, msg
        assert rcp == lib.C8_ERR_UNSUPPORTED


# ---- the step drivers ------------------------------------------------------------------------------------------------------------
def driver_worker(rank, world, port, out):
    """the deck of test_gpu_krylov_parts.py::driver_worker_device with preconditioner="multilevel_parts", three levels forced"""
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
        asm.set_krylov_multilevel(coarse_max=1, max_levels=3)
        solver = distributed_device_solver(asm, preconditioner="multilevel_parts")
        levels = [d[0] for d in device_levels(asm)]
        drv = PrimalDriver(asm, bcs_for(local_sets(lc), lc), solver=solver)
        drv.solve(2)
        J = comm.allreduce(np.array([drv.qoi()]))[0]
        primal_solves = solver.solves
        grad = comm.allreduce(adjoint_gradient(drv, len(act)))
        res = {"iters": list(drv.newton_iters), "J": float(J), "grad": grad, "primal_solves": primal_solves, "solves": solver.solves,
               "total_iters": solver.total_iters, "status": solver.last.status, "kind": asm.krylov_preconditioner, "levels": levels}
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


def test_step_drivers_over_two_parts_with_the_multilevel_preconditioner():
    out = spawn(driver_worker, 2)
    for r in range(2):
        res = out[r]
        print("rank %d: nodes per level %s, Newton %s / %s, linear solves %d (primal %d), BiCGStab iterations %d, J %.16e / %.16e" %
              (r, res["levels"], res["iters"], res["ref_iters"], res["solves"], res["primal_solves"], res["total_iters"], res["J"], res["ref_J"]))
        assert res["kind"] == "multilevel_parts" and len(res["levels"]) == 3
        assert res["iters"] == res["ref_iters"] and max(res["iters"]) > 2, (r, res["iters"], res["ref_iters"])
        assert abs(res["J"] / res["ref_J"] - 1.0) < 1e-8, (r, res["J"], res["ref_J"])
        assert np.abs(res["grad"] - res["ref_grad"]).max() < 1e-7 * np.abs(res["ref_grad"]).max(), (r, res["grad"], res["ref_grad"])
        assert res["primal_solves"] > 0 and res["solves"] == res["primal_solves"] + 2 and res["status"] == 0, (r, res)
