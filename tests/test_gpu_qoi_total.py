"""The subdomain and reaction objectives end to end on the device: the total gradient of `adjoint_gradient` against
differences of `PrimalDriver.qoi()`, the reaction value against c8_qoi_preprocess and over two parts, and the error chain
under a displacement-component objective."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gradient_cases as gc  # noqa: E402
import parity_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 7e-8  # of the largest scaled component: the bar test_oracle_gradient_fd.py holds the oracle to


def _two_set_case():
    """small_J2 on the hex8 bar with the element sets of gradient_cases' two-set case: the objectives live on set 0, the
    gradient has slots of both sets"""
    other = [900.0, 0.3, 60.0, 1.7, 0.0, 0.0]
    slots = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3)]
    return gc.Case("small_J2", "hex8", [pc.J2, other], gc.RATE["two_sets"], elem_set=[0, 1, 1, 0], slots=slots, yields=gc.YIELDS,
                   name="small_J2-hex8-two_sets")


CASES = {"small_J2-hex8": _two_set_case, "hyper_J2-tet4": lambda: gc.BY_NAME["hyper_J2-tet4"],
         "small_hill_plane_strain-tri3": lambda: gc.BY_NAME["small_hill_plane_strain-tri3"],
         "hyper_J2_plane_stress-tri3": lambda: gc.BY_NAME["hyper_J2_plane_stress-tri3"]}
KINDS = ("avg_stress", "avg_local_var", "disp_comp", "reaction")


def set_objective(asm, case, kind):
    et, c, conn, _ = gc.mesh(case.kind)
    if kind == "reaction":
        asm.set_qoi_reaction(coord_idx=1, coord_value=float(c[:, 1].min()), coord_tol=1e-8, comp=1)
    else:
        asm.set_qoi_subdomain(kind, 0, {"avg_stress": 0, "avg_local_var": "alpha", "disp_comp": 0}[kind])


def device_primal(case, p):
    from calibr8_amd import Assembler, PrimalDriver
    args, kw = case.backend_kw(case.rows(p))
    asm = Assembler(*args, **kw)
    return PrimalDriver(asm, case.dbc_spec(), max_iters=30, abs_tol=1e-12, rel_tol=1e-12).solve(gc.NSTEPS)


def objectives(case, pr):
    out = []
    for kind in KINDS:
        set_objective(pr.asm, case, kind)
        out.append(pr.qoi())
    return np.array(out)


def fd_all_kinds(case, p, k, span):
    """gradient_cases.fd_gradient with one primal solve per stencil point shared by the four objectives (the solve does not
    depend on the objective): (R, R2) per kind"""
    D = []
    for h in (case.s * span, 0.5 * case.s * span, 0.25 * case.s * span):
        J = []
        for sign in (1.0, -1.0):
            q = np.array(p, dtype=np.float64)
            q[k] += sign * h
            J.append(objectives(case, device_primal(case, q)))
        D.append((J[0] - J[1]) / (2.0 * h))
    return (4.0 * D[2] - D[1]) / 3.0, (4.0 * D[1] - D[0]) / 3.0


def adjoint_all_slots(case, pr):
    """the adjoint gradient per slot, marched in groups that fit the lanes of K5"""
    from calibr8_amd import adjoint_gradient
    g = np.zeros(len(case.slots))
    by_set = case.groups_all()
    width = case.width
    chunks = max((len(v) + width - 1) // width for v in by_set.values())
    for ch in range(chunks):
        grp = {s: v[ch * width:(ch + 1) * width] for s, v in by_set.items()}
        for s in range(case.params.shape[0]):
            pr.asm.set_active(s, grp.get(s, []))
        got = adjoint_gradient(pr, sum(len(v) for v in grp.values()))
        g[gc.slot_index(case, {s: v for s, v in grp.items() if v})] = got
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_total_gradient_against_differences(name):
    """adjoint_gradient under each of the four objectives, per parameter, against Richardson-extrapolated central
    differences of PrimalDriver.qoi() over the load history of gradient_cases (loading, elastic unloading, reloading): 7e-8 of
    the largest scaled component.  The differences are a reference at that bar: their two Richardson levels agree to a tenth
    of it in every component (asserted; measured on an MI355X: spreads of 2e-12 .. 2e-9, errors of 3e-12 .. 2e-9).  The
    displacement objective takes the x component: on the tet4 bar every node lies on ymin or ymax, where u_y is prescribed."""
    case = CASES[name]()
    p0 = case.p0()
    sp = gc.spans(p0)
    base = device_primal(case, p0)
    gc.check_history(case, type("H", (), {"xi": [x.cpu().numpy() for x in base.xi]})())
    adj = []
    for kind in KINDS:
        set_objective(base.asm, case, kind)
        adj.append(adjoint_all_slots(case, base))
    adj = np.array(adj)                                       # [kind][slot]
    R, R2 = np.zeros_like(adj), np.zeros_like(adj)
    for k in range(len(p0)):
        R[:, k], R2[:, k] = fd_all_kinds(case, p0, k, sp[k])
    bad = []
    for i, kind in enumerate(KINDS):
        scale = np.abs(R[i] * sp).max()
        assert scale > 0, (name, kind)
        err = np.abs(adj[i] - R[i]) * sp / scale
        spread = np.abs(R[i] - R2[i]) * sp / scale
        print("%s %s: J-scale %.3e worst err %.2e worst spread %.2e" % (name, kind, scale, err.max(), spread.max()))
        for k in range(len(p0)):
            print("    slot %s adjoint % .10e differences % .10e err %.2e spread %.2e" % (case.slots[k], adj[i][k], R[i][k], err[k], spread[k]))
            if not err[k] <= BAR:
                bad.append((kind, case.slots[k], adj[i][k], R[i][k], err[k], spread[k]))
        assert spread.max() <= 0.1 * BAR, (name, kind, "the differences do not settle", spread)
    assert not bad, (name, bad)


def test_reaction_value_is_the_preprocessed_load():
    case = CASES["small_J2-hex8"]()
    pr = device_primal(case, case.p0())
    set_objective(pr.asm, case, "reaction")
    J = pr.qoi()
    loads = [pr.asm.qoi_preprocess(pr.u[s], pr.p[s], pr.u[s - 1], pr.p[s - 1], pr.xi[s - 1], pr.xi[s])[1] for s in range(1, len(pr.u))]
    assert abs(J) > 0 and abs(J - sum(loads)) <= 1e-12 * sum(abs(v) for v in loads), (J, loads)


# ---- reaction over two parts sharing the card -----------------------------------------------------------------------------
def _reaction_value(asm, u, p, xi_prev):
    import torch
    d = asm.dev
    du, dp = d(u), d(p)
    dz, dzp = torch.zeros_like(du), torch.zeros_like(dp)
    xi, ls = asm.new_state(), asm.new_linsys()
    asm.set_scatter("atomic")
    assert asm.forward_jacobian(du, dp, dz, dzp, d(xi_prev), xi, ls) == 0
    asm.set_qoi_reaction(coord_idx=1, coord_value=0.0, coord_tol=1e-8, comp=1)
    J = torch.zeros(1, dtype=torch.float64, device=asm.device)
    assert asm.eval_qoi(du, dp, J, xi_prev=d(xi_prev), xi=xi, u_prev=dz, p_prev=dzp) == 0
    torch.cuda.synchronize()
    return float(J.item())


def reaction_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_gpu_distributed import setup_part
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from calibr8_amd import Assembler
        S = setup_part(rank, world, (6, 4, 2), (2, 1, 1))
        c, conn, u, p, part, plan, asm, comm = (S[k] for k in ("c", "conn", "u", "p", "part", "plan", "asm", "comm"))
        gid = plan.node_gid
        J = _reaction_value(asm, np.ascontiguousarray(u.reshape(-1, 3)[gid].ravel()), np.ascontiguousarray(p[gid]), np.zeros((len(part.conn), 8, 7)))
        res = {"J": J, "sum": float(comm.allreduce(np.array([J]))[0])}  # the caller sums J over the parts
        if rank == 0:
            res["ref"] = _reaction_value(Assembler(8, c, conn, "small_J2", pc.J2), u, p, np.zeros((len(conn), 8, 7)))
        S["halo"].close()
        comm.close()
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_reaction_over_two_parts_counts_the_load_once():
    from test_gpu_distributed import spawn
    out = spawn(reaction_worker, 2)
    ref = out[0]["ref"]
    assert abs(ref) > 1e-3
    for r in range(2):
        assert abs(out[r]["sum"] - ref) <= 1e-12 * abs(ref), (r, out[r], ref)
        assert abs(out[r]["J"] - 0.5 * ref) <= 1e-12 * abs(ref)   # every part reports its share: 1 / num_parts of the total


# ---- the error chain under a linear subdomain objective -----------------------------------------------------------------------
def test_model_form_error_verify_closes_under_a_displacement_component():
    """model_form_error_verify on the mesh, history and fine model of test_gpu_exact_errors.py, the objective the y
    displacement over the element set: linear in the state, so E_computed = E_exact to that test's tolerance, 1e-8 |E_exact|
    plus the allowance of the fine run's residuals -- and neither side is small against it"""
    import error_cases as ec
    import exact_cases as xc
    from calibr8_amd import Assembler, PrimalDriver, model_form_error_verify
    c, conn, spec = ec.mfe_case()
    runs = []
    for prm in (pc.J2, ec.mfe_params(xc.MFE_VERIFY_DELTA)):
        asm = Assembler(8, c, conn, "small_J2", prm)
        asm.set_qoi_subdomain("disp_comp", 0, 1)
        runs.append(PrimalDriver(asm, spec, max_iters=25, abs_tol=ec.MFE_TOL, rel_tol=ec.MFE_TOL).solve(ec.MFE_STEPS))
    r = model_form_error_verify(*runs)
    bound = 1e-8 * abs(r.E_exact) + r.allowance
    gap, E_lin = abs(r.E_computed - r.E_exact), abs(r.E_lin_R + r.E_lin_C)
    print("disp_comp: E_exact %.6e eta %.6e E_lin %.6e gap %.3e bound %.3e" % (r.E_exact, r.eta, E_lin, gap, bound))
    assert gap <= bound, (gap, bound)
    assert E_lin > 1000.0 * bound and abs(r.eta - r.E_exact) > 1000.0 * bound
    # the stress objective is not linear: refused
    runs[1].asm.set_qoi_subdomain("avg_stress", 0, 0)
    runs[0].asm.set_qoi_subdomain("avg_stress", 0, 0)
    with pytest.raises(ValueError, match="linear"):
        model_form_error_verify(*runs)
