"""`-m gpu`: the device-resident linear solve over the parts of a multi-part mesh (c8_krylov_solve_parts,
calibr8_amd.distributed_device_solver) against its definition -- the true residual of the gathered
owned system and SciPy's direct solve of it --, beside SciPy's BiCGStab, bit for bit against itself on two parts, through
the step drivers against the single-part run with the host direct solve, and in its collective refusals.

The ranks share the one card through the host transport (gloo), as in test_gpu_distributed.py; one rank runs in-process,
over the host transport and over RCCL.  Several cases share one spawn: starting the processes costs more than the solves."""
import ctypes as C
import datetime
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_gpu_distributed import bcs_for, setup_part, spawn  # noqa: E402
from test_gpu_krylov import device_system, new_dx, node_block_jacobi, raw_solve, system_case  # noqa: E402

pytestmark = pytest.mark.gpu
REL_TOL = 1e-10
J2 = [1000.0, 0.25, 100.0, 2.0, 0.0, 0.0]


def init(rank, world, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    # a mismatch between the ranks' collectives ends in an error after a minute, not in a hang
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))


def make_part(rank, world, et, c, conn, ep, model, params, d=dist):
    from calibr8_amd import Assembler
    from calibr8_amd import distributed as D
    part = D.part_from_global(c, conn, ep, rank, world)
    plan = D.HaloPlan(part, d if world > 1 else None)
    asm = Assembler(et, c[plan.node_gid] if world > 1 else plan.coords, part.conn, model, params, extra_pairs=plan.extra_pairs)
    comm = D.Comm.host(d if world > 1 else None, rank, world)
    halo = D.Halo(plan, asm.rowptr[1][1], asm.colidx[1][1], asm, comm)
    return dict(c=c, part=part, plan=plan, asm=asm, comm=comm, halo=halo)


def part_system(S, spec, adjoint=False):
    """This part's system as the drivers hold it: K1 (or K3) of the prescribed plastic state assembled over the part's
    elements, c8_halo_gather, c8_apply_dirichlet on the owned rows.  spec: [(resid, eq, GLOBAL node ids)]."""
    from meshes import fields_for, prescribed_fields
    asm, plan, halo, c = S["asm"], S["plan"], S["halo"], S["c"]
    gid = plan.node_gid
    u, p = fields_for(asm.ndims, *prescribed_fields(c, 0.004, ramp=True))
    U, P = asm.dev(np.ascontiguousarray(u.reshape(-1, asm.ndims)[gid].ravel())), asm.dev(np.ascontiguousarray(p[gid]))
    Z, ZP = torch.zeros_like(U), torch.zeros_like(P)
    ls, xi = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(U, P, Z, ZP, asm.new_state(), xi, ls) == 0
    S["plastic"] = float(xi[:, :, -1].max())
    if adjoint:
        ls.zero()
        g = torch.zeros(asm.nelems, asm.npts, asm.nloc, dtype=torch.float64, device=asm.device)
        f = torch.zeros(asm.nelems, asm.npts, asm.ndofs, dtype=torch.float64, device=asm.device)
        assert asm.adjoint_jacobian(U, P, Z, ZP, asm.new_state(), xi, g, f, ls) == 0
    halo.gather(ls)
    local_of = {int(g_): k for k, g_ in enumerate(gid)}
    dd = []
    for r, e, nodes in spec:
        loc = np.array(sorted(local_of[int(n)] for n in nodes if int(n) in local_of), dtype=np.int32)
        dd.append((r, e, torch.as_tensor(loc, device=asm.device), asm.dev(np.zeros(len(loc)))))
    asm.apply_dirichlet(dd, U, P, ls, is_adjoint=adjoint)
    torch.cuda.synchronize()
    return ls


def solve_parts(asm, ls, dx=None, **opts):
    """c8_krylov_solve_parts straight through the ABI: (return code, info as a tuple, dx tensors)"""
    from calibr8_amd import lib
    dx = dx or new_dx(asm)
    o = lib.KrylovOpts(opts.get("max_iters", 0), opts.get("check_every", 0), opts.get("max_restarts", 0), opts.get("rel_tol", REL_TOL), 0.0)
    info = lib.KrylovInfo()
    sy = ls.c_struct()
    ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
    rc = asm.L.c8_krylov_solve_parts(asm.h, C.byref(sy), ptrs, C.byref(o), C.byref(info))
    torch.cuda.synchronize()
    return rc, (info.iters, info.restarts, info.status, info.b_norm, info.residual_norm), dx


def owned_piece(S, ls, dx):
    """what a rank contributes to the global owned system: its owned rows (local columns), b, x, and its local -> global ids"""
    asm, plan = S["asm"], S["plan"]
    no = plan.part.nowned
    piece = {"gid": plan.node_gid, "no": no, "n": asm.nnodes, "A": {}, "b": [], "x": []}
    for i in range(asm.nres):
        nrows = no * asm.neq[i]
        piece["b"].append(ls.b[i].cpu().numpy()[:nrows])
        piece["x"].append(dx[i].cpu().numpy()[:nrows])
        for j in range(asm.nres):
            rp, ci = asm.rowptr[i][j], asm.colidx[i][j]
            piece["A"][(i, j)] = (rp[: nrows + 1].copy(), ci[: rp[nrows]].copy(), ls.A[i][j].cpu().numpy()[: rp[nrows]])
    return piece


def check_contract(pieces, N, neq, nres, info, tag, with_scipy=False):
    """The contract of test_single_solve_meets_its_contract for the global owned system put together from the ranks' pieces.
    The residual is recomputed rank by rank in the rows' own (local) column order, the order the solver defines it by; the
    global matrix (columns by global id) serves the direct solve, the condition estimate and SciPy's BiCGStab."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    off = [0, N * neq[0]]
    xg, bg = np.zeros(N * sum(neq[:nres])), np.zeros(N * sum(neq[:nres]))
    rows_of = []
    for q in pieces:
        rows = [off[i] + np.repeat(q["gid"][: q["no"]], neq[i]) * neq[i] + np.tile(np.arange(neq[i]), q["no"]) for i in range(nres)]
        rows_of.append(rows)
        for i in range(nres):
            xg[rows[i]], bg[rows[i]] = q["x"][i], q["b"][i]
    R, Cc, V, rr = [], [], [], 0.0
    for q, rows in zip(pieces, rows_of):
        xl = [xg[off[j] + (q["gid"][:, None] * neq[j] + np.arange(neq[j])).ravel()] for j in range(nres)]
        blocks = [[sp.csr_matrix(q["A"][(i, j)][::-1], shape=(q["no"] * neq[i], q["n"] * neq[j])) for j in range(nres)] for i in range(nres)]
        Al = sp.bmat(blocks, format="csr")
        rl = np.concatenate(q["b"]) - Al @ np.concatenate(xl)
        rr += float(rl @ rl)
        for i in range(nres):
            for j in range(nres):
                rp, ci, vals = q["A"][(i, j)]
                R.append(np.repeat(rows[i], np.diff(rp)))
                Cc.append(off[j] + q["gid"][ci // neq[j]] * neq[j] + ci % neq[j])
                V.append(vals)
    A = sp.csr_matrix((np.concatenate(V), (np.concatenate(R), np.concatenate(Cc))), shape=(len(bg), len(bg)))
    res_norm, b_norm = np.sqrt(rr), np.linalg.norm(bg)
    lu = spla.splu(A.tocsc())
    x_ref = lu.solve(bg)
    inv_op = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    cond_est = spla.onenormest(A) * spla.onenormest(inv_op)
    err = np.linalg.norm(xg - x_ref) / np.linalg.norm(x_ref)
    out = {"n": len(bg), "res": res_norm / b_norm, "info_res": abs(info[4] / res_norm - 1.0), "info_b": abs(info[3] / b_norm - 1.0),
           "err": err, "cond": cond_est, "iters": info[0]}
    print("%s: n %d iters %d restarts %d host residual %.3e info/host-1 %.3e b_norm/host-1 %.3e cond_est %.3e x error %.3e" %
          (tag, len(bg), info[0], info[1], out["res"], out["info_res"], out["info_b"], cond_est, err))
    if with_scipy:
        class G:  # what node_block_jacobi reads of an assembler
            nnodes, ndims, nres = N, neq[0], 0
        G.nres = nres
        count = [0]

        def cb(_):
            count[0] += 1
        xs, flag = spla.bicgstab(A, bg, rtol=REL_TOL, atol=0.0, maxiter=20000, M=node_block_jacobi(G, A), callback=cb)
        out["scipy_iters"], out["scipy_flag"] = count[0], flag
    return out


def assert_contract(m, tag):
    assert m["res"] <= 1.01 * REL_TOL, (tag, m)
    assert m["info_res"] < 1e-9, (tag, m)   # n eps for the differently rounded sum of squares (test_contract_of_the_refusals)
    assert m["info_b"] < 1e-12, (tag, m)
    assert m["err"] <= m["cond"] * REL_TOL, (tag, m)


def gather_pieces(world, piece):
    allp = [None] * world
    if world > 1:
        dist.all_gather_object(allp, piece)
    else:
        allp = [piece]
    return allp


def run_case(S, spec, world, rank, tag, adjoint=False, with_scipy=False, res=None):
    """assemble, solve collectively, rank 0 checks the contract; every rank reports its info"""
    asm = S["asm"]
    ls = part_system(S, spec, adjoint)
    rc, info, dx = solve_parts(asm, ls)
    allp = gather_pieces(world, owned_piece(S, ls, dx))
    res[tag + "_rc"], res[tag + "_info"], res[tag + "_err"] = rc, info, asm.L.c8_last_error().decode() if rc else ""
    res[tag + "_plastic"] = S["plastic"]
    if rank == 0:
        res[tag] = check_contract(allp, S["part"].num_global_nodes, asm.neq, asm.nres, info, tag, with_scipy)
    return ls, dx


def close(S):
    S["halo"].close()
    S["comm"].close()


def part_lists(asm):
    n_i, n_b, ptr = C.c_int32(), C.c_int32(), C.POINTER(C.c_int32)()
    from calibr8_amd import lib
    lib.check(asm.L.c8_krylov_part_lists(asm.h, C.byref(n_i), C.byref(n_b), C.byref(ptr)))
    nodes = np.ctypeslib.as_array(ptr, shape=(n_i.value + n_b.value,)).copy() if n_i.value + n_b.value else np.zeros(0, dtype=np.int32)
    return n_i.value, n_b.value, nodes


def check_lists(asm, no):
    """interior and boundary lists partition [0, num_owned); interior = rows with owned columns only"""
    n_i, n_b, nodes = part_lists(asm)
    rp, ci = asm.rowptr[1][1], asm.colidx[1][1]
    inner = np.array([bool((ci[rp[n]:rp[n + 1]] < no).all()) for n in range(no)], dtype=bool)
    ok = (n_i + n_b == no and np.array_equal(np.sort(nodes), np.arange(no)) and inner[nodes[:n_i]].all() and not inner[nodes[n_i:]].any())
    return bool(ok), n_i, n_b


# ---- cases 1, 2, 5 (first half), 8: two parts of notched_bar(16, 4, 4) ---------------------------------------------------
def bar_parts(rank, world):
    et, c, conn, model, params, spec, _ = system_case((16, 4, 4))
    ep = (c[conn].mean(axis=1)[:, 0] > 0.5 * (c[:, 0].min() + c[:, 0].max())).astype(np.int32)
    return make_part(rank, world, et, c, conn, ep, model, params), spec


def bar_worker(rank, world, port, out, full):
    init(rank, world, port)
    try:
        from calibr8_amd import lib
        S, spec = bar_parts(rank, world)
        asm, no = S["asm"], S["part"].nowned
        res = {"lists": check_lists(asm, no)}
        ls, dx = run_case(S, spec, world, rank, "k1", with_scipy=full, res=res)
        res["x1"] = np.concatenate([dx[i].cpu().numpy()[: no * asm.neq[i]] for i in range(2)]).tobytes()
        if full:
            # reproducible in the process
            rc, info2, dx2 = solve_parts(asm, ls)
            res["x2"] = np.concatenate([dx2[i].cpu().numpy()[: no * asm.neq[i]] for i in range(2)]).tobytes()
            res["iters2"] = info2[0]
            # the budget: every rank reports the same iterate count and code
            rc, info3, _ = solve_parts(asm, ls, max_iters=3)
            res["budget"] = (rc, info3[0], info3[2])
            # refusals.  null pointers (every rank alike, nothing is exchanged)
            sy = ls.c_struct()
            ptrs = (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr())
            L = asm.L
            bad = ls.c_struct()
            bad.A[0][1] = None
            res["null"] = [L.c8_krylov_solve_parts(None, C.byref(sy), ptrs, None, None), L.c8_krylov_solve_parts(asm.h, None, ptrs, None, None),
                           L.c8_krylov_solve_parts(asm.h, C.byref(sy), None, None, None),
                           L.c8_krylov_solve_parts(asm.h, C.byref(sy), (C.c_void_p * 2)(dx[0].data_ptr(), None), None, None),
                           L.c8_krylov_solve_parts(asm.h, C.byref(bad), ptrs, None, None), L.c8_krylov_linear_solve_parts(None, C.byref(sy), ptrs)]
            # b = 0 on all ranks
            saved = [ls.b[i].clone() for i in range(2)]
            for i in range(2):
                ls.b[i].zero_()
            rc, info0, dx0 = solve_parts(asm, ls)
            res["zero"] = (rc, info0[0], info0[3], bool(any(dx0[i][: no * asm.neq[i]].any() for i in range(2))))
            for i in range(2):
                ls.b[i].copy_(saved[i])
            # one owned node's diagonal block zeroed on rank 1 only
            node = no // 2
            if rank == 1:
                rp, ci = asm.rowptr, asm.colidx
                for i in range(2):
                    for j in range(2):
                        vals = ls.A[i][j].cpu().numpy()
                        for eq in range(asm.neq[i]):
                            row = node * asm.neq[i] + eq
                            lo, hi = rp[i][j][row], rp[i][j][row + 1]
                            vals[lo:hi][(ci[i][j][lo:hi] // asm.neq[j]) == node] = 0.0
                        ls.A[i][j].copy_(asm.dev(vals))
            rc, infob, _ = solve_parts(asm, ls)
            res["singular"] = (rc, infob[0], L.c8_last_error().decode(), node)
            # the K3 system of the same mesh
            run_case(S, spec, world, rank, "k3", adjoint=True, res=res)
            if rank == 0:  # the single-part device count, printed beside the others
                a1, l1 = device_system((16, 4, 4))
                res["single_iters"] = raw_solve(a1, l1, new_dx(a1))[1].iters
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def bar_run():
    return spawn(bar_worker, 2, True)


def test_two_part_solve_meets_its_contract(bar_run):
    from calibr8_amd import lib
    for tag in ("k1", "k3"):
        for r in range(2):
            assert bar_run[r][tag + "_rc"] == lib.C8_OK, (tag, r, bar_run[r][tag + "_err"])
        assert bar_run[0][tag + "_info"] == bar_run[1][tag + "_info"], tag   # info is equal on both ranks
        assert bar_run[0][tag + "_info"][2] == lib.C8_OK
        assert_contract(bar_run[0][tag], tag)
    assert bar_run[0]["k1"]["n"] == 1580
    assert max(bar_run[r]["k1_plastic"] for r in range(2)) > 0.0   # a plastic state
    for r in range(2):
        assert bar_run[r]["lists"][0], (r, bar_run[r]["lists"])
        assert bar_run[r]["budget"] == (lib.C8_NOT_CONVERGED, 3, lib.C8_NOT_CONVERGED)


def test_two_part_iteration_count_beside_scipy_bicgstab(bar_run):
    """No more than twice SciPy's BiCGStab iterations on the gathered matrix (same preconditioner and tolerance): the margin
    and the comparison of test_iteration_counts_beside_scipy_bicgstab."""
    m = bar_run[0]["k1"]
    print("notched_bar(16, 4, 4) over two parts: device iterations %d, SciPy BiCGStab %d (flag %d), single-part device solve %d" %
          (m["iters"], m["scipy_iters"], m["scipy_flag"], bar_run[0]["single_iters"]))
    assert m["scipy_flag"] == 0
    assert m["iters"] <= 2 * m["scipy_iters"]


def test_two_part_solve_is_reproducible(bar_run):
    """Two solves in one spawn and one in a second spawn: the same bytes of dx on the owned nodes and the same iteration
    count (a two-rank sum is commutative, the transport cannot reorder it).  No such claim for four parts."""
    again = spawn(bar_worker, 2, False)
    for r in range(2):
        assert bar_run[r]["x1"] == bar_run[r]["x2"] and bar_run[r]["k1_info"][0] == bar_run[r]["iters2"], r
        assert again[r]["x1"] == bar_run[r]["x1"] and again[r]["k1_info"][0] == bar_run[r]["k1_info"][0], r


def test_refusals_are_collective(bar_run):
    from calibr8_amd import lib
    for r in range(2):
        res = bar_run[r]
        assert res["null"] == [lib.C8_ERR_ARG] * 6, (r, res["null"])
        assert res["zero"] == (lib.C8_OK, 0, 0.0, False), (r, res["zero"])
        rc, iters, msg, _ = res["singular"]
        node = bar_run[1]["singular"][3]   # rank 1's local id
        assert rc == lib.C8_ERR_ARG and iters == 0, (r, res["singular"])       # both ranks, nothing iterated
        assert ("node %d " % node) in msg and "rank 1" in msg, (r, msg)


# ---- case 3: four parts, nodes shared by four of them ---------------------------------------------------------------------
def brick_worker(rank, world, port, out):
    init(rank, world, port)
    try:
        S = setup_part(rank, world, (6, 6, 4), (2, 2, 1))
        sets = S["sets"]
        spec = [(0, d, sets["xmin"]) for d in range(3)] + [(0, 0, sets["xmax"])]
        res = {"lists": check_lists(S["asm"], S["part"].nowned)}
        run_case(S, spec, world, rank, "k1", res=res)
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_four_parts_meet_the_contract_and_the_lists_partition_the_owned_nodes():
    from calibr8_amd import lib
    out = spawn(brick_worker, 4)
    for r in range(4):
        assert out[r]["k1_rc"] == lib.C8_OK, (r, out[r]["k1_err"])
        assert out[r]["k1_info"] == out[0]["k1_info"], r
        ok, n_i, n_b = out[r]["lists"]
        print("rank %d: interior %d boundary %d" % (r, n_i, n_b))
        assert ok and n_b > 0, (r, out[r]["lists"])
    assert_contract(out[0]["k1"], "brick(6, 6, 4) over 2 x 2 x 1")


# ---- case 4: 2-D, 3 x 3 and 2 x 2 blocks -------------------------------------------------------------------------------------
def tri_worker(rank, world, port, out, model, params):
    init(rank, world, port)
    try:
        from meshes import jiggle_2d, tri_mesh
        c, conn, sets = tri_mesh(8, 6, 1.0, 0.8)
        c = jiggle_2d(c, sets, 0.02)
        ep = (c[conn].mean(axis=1)[:, 0] > 0.47).astype(np.int32)   # the split of driver_worker_2d
        S = make_part(rank, world, 3, c, conn, ep, model, params)
        spec = [(0, 0, sets["xmin"]), (0, 1, sets["ymin"]), (0, 1, sets["ymax"])]
        res = {"nres": S["asm"].nres}
        run_case(S, spec, world, rank, "k1", res=res)
        close(S)
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("model", ["small_J2", "small_hill_plane_stress"])
def test_two_parts_on_2d_meshes(model):
    from calibr8_amd import lib
    from parity_cases import HILL_PS
    out = spawn(tri_worker, 2, model, J2 if model == "small_J2" else HILL_PS)
    for r in range(2):
        assert out[r]["nres"] == (2 if model == "small_J2" else 1)
        assert out[r]["k1_rc"] == lib.C8_OK, (r, out[r]["k1_err"])
    assert out[0]["k1_info"] == out[1]["k1_info"]
    assert_contract(out[0]["k1"], model)


# ---- cases 6 and 9: one rank with a halo attached, in-process ------------------------------------------------------------------
def one_rank(make_comm):
    from calibr8_amd import Assembler, lib
    import calibr8_amd.distributed as D
    et, c, conn, model, params, spec, _ = system_case((16, 4, 4))
    part = D.part_from_global(c, conn, np.zeros(len(conn), dtype=np.int32), 0, 1)
    plan = D.HaloPlan(part, None)
    asm = Assembler(et, plan.coords, part.conn, model, params)
    comm = make_comm(D)
    halo = D.Halo(plan, asm.rowptr[1][1], asm.colidx[1][1], asm, comm)
    S = dict(c=c, part=part, plan=plan, asm=asm, comm=comm, halo=halo)
    res = {}
    ls, dx = run_case(S, spec, 1, 0, "k1", res=res)
    assert res["k1_rc"] == lib.C8_OK, res["k1_err"]
    assert_contract(res["k1"], "one rank")
    assert check_lists(asm, part.nowned) == (True, asm.nnodes, 0)   # no copies: every row is interior
    # the single-part call on the same context still refuses
    info = lib.KrylovInfo()
    sy = ls.c_struct()
    rc = asm.L.c8_krylov_solve(asm.h, C.byref(sy), (C.c_void_p * 2)(dx[0].data_ptr(), dx[1].data_ptr()), None, C.byref(info))
    assert rc == lib.C8_ERR_UNSUPPORTED and info.status == lib.C8_ERR_UNSUPPORTED and b"halo" in asm.L.c8_last_error()
    torch.cuda.synchronize()
    close(S)
    return res


def test_one_rank_with_a_halo_attached():
    one_rank(lambda D: D.Comm.host(None, 0, 1))


def test_one_rank_over_rccl():
    """the device-buffer ncclAllReduce between the two events, with the one rank RCCL admits on one card"""
    from calibr8_amd import lib

    def make(D):
        try:
            return D.Comm.rccl(None, 0, 1)
        except lib.C8Error as e:
            if e.code == lib.C8_ERR_UNSUPPORTED:
                pytest.skip("librccl cannot be loaded: %s" % e)
            raise
    one_rank(make)


# ---- case 7: the step drivers ------------------------------------------------------------------------------------------------
def driver_worker_device(rank, world, port, out):
    init(rank, world, port)
    try:
        from calibr8_amd import Assembler, distributed_device_solver, scipy_solver
        from calibr8_amd.primal import PrimalDriver, adjoint_gradient
        S = setup_part(rank, world, (6, 4, 3), (2, 1, 1), jig=0.02)   # driver_worker's problem
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
        solver = distributed_device_solver(asm)
        drv = PrimalDriver(asm, bcs_for(local_sets(lc), lc), solver=solver)
        drv.solve(2)
        J = comm.allreduce(np.array([drv.qoi()]))[0]
        primal_solves = solver.solves
        grad = comm.allreduce(adjoint_gradient(drv, len(act)))
        res = {"iters": list(drv.newton_iters), "J": float(J), "grad": grad, "primal_solves": primal_solves, "solves": solver.solves,
               "total_iters": solver.total_iters, "status": solver.last.status}
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


def test_step_drivers_over_two_parts_with_the_device_solver():
    out = spawn(driver_worker_device, 2)
    for r in range(2):
        res = out[r]
        print("rank %d: Newton %s / %s, linear solves %d (primal %d), BiCGStab iterations %d, J %.16e / %.16e" %
              (r, res["iters"], res["ref_iters"], res["solves"], res["primal_solves"], res["total_iters"], res["J"], res["ref_J"]))
        assert res["iters"] == res["ref_iters"] and max(res["iters"]) > 2, (r, res["iters"], res["ref_iters"])
        assert abs(res["J"] / res["ref_J"] - 1.0) < 1e-8, (r, res["J"], res["ref_J"])
        assert np.abs(res["grad"] - res["ref_grad"]).max() < 1e-7 * np.abs(res["ref_grad"]).max(), (r, res["grad"], res["ref_grad"])
        # the adjoint steps went through the device solve too: one more solve per load step
        assert res["primal_solves"] > 0 and res["solves"] == res["primal_solves"] + 2 and res["status"] == 0, (r, res)
