"""The kernels of the subdomain objectives (calibr8_amd/csrc/c8_qoi_point.hip) against the host harness that compiles the
same per-point functions (tests/qoi_host, verified by test_qoi_host.py), through the four entry points, and what those entry
points promise around them.

How a pass is told from the adjoint kernel it runs beside.  A subdomain objective over an element set WITHOUT elements is a
zero objective: its passes touch nothing and K3 / K5 run exactly as under the real one.  So with the same inputs
    J                          c8_eval_qoi, directly
    g after the pre-pass       the g that c8_assemble_adjoint_jacobian returns (K3 only reads it), directly
    -dJ/dx of the post-pass    b(real set) - b(empty set, started from the g that the real run returned)
    dJ/dp                      c8_param_gradient with z = 0 and phi = 0, under which K5 adds exact zeros
Every mesh here therefore carries one more (empty) element set than it uses.  The bar is the project's parity bar, 1e-12, of
the magnitudes that enter each number (for the difference of two b: those of b itself)."""
import types

import numpy as np
import pytest

import cauchy_cases as cc
import launch_cases as lc
import oracle_lib as ol
import parity_cases as pc
import qoi_cases as qc

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    return qc.build_harness(tmp_path_factory.mktemp("c8_qoi_host_gpu"))


class Problem:
    """a mesh, its element sets (the last parameter row belongs to a set without elements), a model and a state"""

    def __init__(self, et, c, conn, model, rows, es, state, nn=None, kw=None):
        self.et, self.c, self.conn, self.model = et, np.ascontiguousarray(c), np.ascontiguousarray(conn, dtype=np.int32), model
        self.rows = np.ascontiguousarray(np.atleast_2d(np.asarray(rows, dtype=np.float64)))
        self.es = np.ascontiguousarray(es, dtype=np.int32)
        self.empty = len(self.rows) - 1
        assert not (self.es == self.empty).any()
        self.state, self.nn, self.kw = [np.ascontiguousarray(a, dtype=np.float64) for a in state], nn, dict(kw or {})
        self.nd = qc.NDIMS[et]

    def assembler(self, rows=None, es=None):
        from calibr8_amd import Assembler
        return Assembler(self.et, self.c, self.conn, self.model, self.rows if rows is None else rows,
                         elem_set=self.es if es is None else es, **self.kw)

    def host(self, harness, q, **kw):
        return qc.host_qoi(harness, self.et, self.c, self.conn, self.model, self.rows, *self.state, q, elem_set=self.es, nn=self.nn, **kw)


def of_case(rid):
    """a row of the model table on its mesh with the oracle's state: every element in set 0, set 1 empty"""
    cs = cc.case(rid)
    return Problem(cs.et, cs.c, cs.conn, cs.model, [cs.params, cs.params], np.zeros(len(cs.conn)), cs.state, nn=cs.nn, kw=cs.assembler_kw())


def of_mesh(et, c, conn, model, two_sets=True, seed=4):
    """small_J2 or hyper_J2 on a mesh with a synthetic state (no solve: two evaluations of one function are compared); two
    interleaved element sets with different parameters, set 2 empty"""
    base = {"small_J2": pc.J2, "hyper_J2": pc.HJ2}[model]
    other = [v * s for v, s in zip(base, (0.7, 1.2, 0.5, 0.6, 1.0, 1.0, 1.0, 1.0))]
    es = (np.arange(len(conn)) % 2) if two_sets else np.zeros(len(conn))
    npts = len(ol.kit_points(et, 0)[0])
    nloc = {"small_J2": 7, "hyper_J2": 8}[model]
    xi0 = ol.Oracle(et, c, conn, model, base).new_state()
    assert xi0.shape == (len(conn), npts, nloc)
    return Problem(et, c, conn, model, [base, other, base], es, cc.synthetic_state(xi0, c, 3, 2, seed=seed))


def device_passes(pb, q, active, seed=11):
    """the four numbers of the head of this file from the device, every output array between guard words.  Returns a dict of
    host arrays: J, g (after the pre-pass), db0 / db1 (what the post-pass added to b), b0 / b1 (b of the real run), bz0 / bz1
    (b of the zero-objective run), grad, grad0, A (the four blocks of the real run)."""
    from test_gpu_launch_edges import Guarded, GuardedSystem
    kind, s, index = q
    asm = pb.assembler()
    for es_, idx in active.items():
        asm.set_active(es_, idx)
    rng = np.random.default_rng(seed)
    st = [asm.dev(a) for a in pb.state]
    xi = pb.state[5]
    g0 = rng.standard_normal(xi.shape)
    f = asm.dev(rng.standard_normal((asm.nelems, asm.npts, asm.ndofs)))
    b_init = [rng.standard_normal(asm.nnodes * asm.ndims), rng.standard_normal(asm.nnodes)]
    out = {"g0": g0, "b_init": b_init}

    def k3(set_id, g_in):
        asm.set_qoi_subdomain(kind, set_id, index)
        host_ls = types.SimpleNamespace(A=[[np.zeros(asm.nnz[i][j]) for j in range(2)] for i in range(2)], b=[b.copy() for b in b_init])
        gs, gg = GuardedSystem(asm, host_ls), Guarded(asm, "g", g_in)
        assert asm.adjoint_jacobian(*st, gg.t, f, gs) == 0
        asm.torch.cuda.synchronize()
        return gg.check(False).copy(), [x.check(False).copy() for x in gs.gb], [[x.check(False).copy() for x in r] for r in gs.gA]

    out["g"], (out["b0"], out["b1"]), out["A"] = k3(s, g0)
    g_z, (out["bz0"], out["bz1"]), A_z = k3(pb.empty, out["g"])
    assert np.array_equal(g_z, out["g"])                       # the zero objective leaves g alone
    assert all(np.array_equal(A_z[i][j], out["A"][i][j]) for i in range(2) for j in range(2))  # A does not see the objective
    out["db0"], out["db1"] = out["b0"] - out["bz0"], out["b1"] - out["bz1"]
    asm.set_qoi_subdomain(kind, s, index)
    gJ = Guarded(asm, "J", np.array([0.25]))
    assert asm.eval_qoi(st[0], st[1], gJ.t, xi_prev=st[4], xi=st[5], u_prev=st[2], p_prev=st[3]) == 0
    out["J"] = float(gJ.check(False)[0]) - 0.25
    if pb.model == cc.HYBRID:  # its gradient entry point takes a mesh with one element set
        asm = pb.assembler(rows=pb.rows[:1], es=np.zeros(len(pb.conn), dtype=np.int32))
        asm.set_active(0, active[0])
        asm.set_qoi_subdomain(kind, 0, index)
        st = [asm.dev(a) for a in pb.state]
    out["grad0"] = rng.standard_normal(asm.num_grad_params)
    gg = Guarded(asm, "grad", out["grad0"])
    z_u, z_p, phi = asm.dev(np.zeros(asm.nnodes * asm.ndims)), asm.dev(np.zeros(asm.nnodes)), asm.dev(np.zeros(xi.shape))
    assert asm.qoi_gradient(*st, z_u, z_p, phi, gg.t) == 0
    asm.torch.cuda.synchronize()
    out["grad"] = gg.check(False).copy()
    return out


def check_against_host(pb, harness, q, active, dev):
    """J, g, b and grad of the device against the harness, at TOL of the magnitudes involved; what lies outside the chosen
    set is untouched bit for bit"""
    kind, s, index = q
    h = pb.host(harness, q, g=dev["g0"])
    inset = pb.es == s
    # J
    assert abs(dev["J"] - h.value.sum()) <= TOL * max(np.abs(h.value).sum(), 0.25), (dev["J"], h.value.sum())
    # g
    assert np.abs(dev["g"] - h.g).max() <= TOL * np.abs(h.g).max()
    assert np.array_equal(dev["g"][~inset], dev["g0"][~inset])
    if np.abs(h.dxi).max() > 0:
        assert np.abs(dev["g"][inset] - dev["g0"][inset]).max() > 0
    # b: the post-pass's share is the harness's b from zero
    sb = max(np.abs(dev["bz0"]).max(), np.abs(dev["b0"]).max())
    assert np.abs(dev["db0"] - h.b0).max() <= TOL * (sb + np.abs(h.b0).max())
    touched = np.zeros(len(pb.c), dtype=bool)
    touched[pb.conn[inset].ravel()] = True
    assert np.array_equal(dev["b0"].reshape(-1, pb.nd)[~touched], dev["bz0"].reshape(-1, pb.nd)[~touched])
    if pb.model.endswith("_plane_stress"):
        assert np.array_equal(dev["b1"], dev["b_init"][1])       # one residual: the pressure vector is not touched at all
    else:
        sb1 = max(np.abs(dev["bz1"]).max(), np.abs(dev["b1"]).max())
        assert np.abs(dev["db1"] - h.b1).max() <= TOL * (sb1 + np.abs(h.b1).max())
        assert np.array_equal(dev["b1"][~touched], dev["bz1"][~touched])
    if kind == qc.DISP_COMP and inset.any():
        assert np.abs(h.b0).max() > 0
    # grad: the slots of the chosen set, in K5's layout (the sets' active lists one after the other)
    ofs = 0
    for es_ in sorted(active):
        idx = active[es_]
        sl = slice(ofs, ofs + len(idx))
        if es_ == s:
            terms = h.dparam[:, :, idx]
            ref = terms.sum(axis=(0, 1))
            scale = np.abs(terms).sum(axis=(0, 1)) + np.abs(dev["grad0"][sl])
            assert np.all(np.abs(dev["grad"][sl] - dev["grad0"][sl] - ref) <= TOL * scale), (dev["grad"][sl] - dev["grad0"][sl], ref)
        else:
            assert np.array_equal(dev["grad"][sl], dev["grad0"][sl])
        ofs += len(idx)
    assert np.array_equal(dev["grad"][ofs:], dev["grad0"][ofs:])   # the hybrid row's weights: dev_cauchy has no network in it


def run_and_repeat(pb, harness, q, active):
    first = device_passes(pb, q, active)
    check_against_host(pb, harness, q, active, first)
    second = device_passes(pb, q, active)
    for k in ("J", "g", "b0", "b1", "grad"):
        assert np.array_equal(np.asarray(first[k]), np.asarray(second[k])), k     # bit for bit from run to run
    return first


def active_of(model, nparams):
    return [0, 1, 2] if model == cc.HYBRID else pc.ACTIVE[model][:8]


@pytest.mark.parametrize("rid", cc.ROW_IDS)
def test_every_row_against_the_harness(harness, rid):
    pb = of_case(rid)
    act = {0: active_of(pb.model, pb.rows.shape[1])}
    if pb.model.endswith("_plane_stress"):
        act[0] = act[0][:6]
    dev = run_and_repeat(pb, harness, (qc.AVG_STRESS, 0, 0), act)
    assert dev["J"] > 0
    nloc = pb.state[5].shape[2]
    if pb.model != "elastic":
        run_and_repeat(pb, harness, (qc.AVG_LOCAL_VAR, 0, cc.ALPHA.get(pb.model, nloc - 1)), act)
    run_and_repeat(pb, harness, (qc.DISP_COMP, 0, pb.nd - 1), act)


# one point per tet4 element: 1, 63, 64, 65 and 257 elements are the wavefront and block edges of the (element, point) lanes
# (256 per block); hex8 has eight: 1, 8 and 9 elements are 8, 64 and 72 lanes
SHAPES = [("tet4", n) for n in (1, 63, 64, 65, 257)] + [("hex8", n) for n in (1, 8, 9)]


@pytest.mark.parametrize("kind,n", SHAPES, ids=["%s-%d" % s for s in SHAPES])
@pytest.mark.parametrize("model", ["small_J2", "hyper_J2"])
def test_launch_edges_with_two_interleaved_sets(harness, model, kind, n):
    et, c, conn = lc.mesh(kind, n, kind == "hex8" and n > 1)
    pb = of_mesh(et, c, conn, model)
    act = {0: [0, 3], 1: [1, 2, 3]}
    for s in ((0, 1) if n > 1 else (0,)):
        run_and_repeat(pb, harness, (qc.AVG_STRESS, s, 0), act)
    run_and_repeat(pb, harness, (qc.DISP_COMP, 0, 1), act)
    run_and_repeat(pb, harness, (qc.AVG_LOCAL_VAR, 0, 6), act)


def test_per_node_pass_on_ragged_meshes(harness):
    """the post-pass sums over a node's elements: the hex8 mesh of the row-per-node tests with a node of sixteen elements
    (meshes.pinched_bricks) and a brick cut into tets whose nodes have 1 to 24 elements; in both, nodes that only the other
    set touches"""
    from meshes import pinched_bricks
    c, conn = pinched_bricks()
    per_node = np.bincount(np.asarray(conn).ravel())
    assert per_node.min() == 1 and per_node.max() == 16
    c2, conn2 = cc.tet_mesh(2, 2, 2)
    c2 = lc._skew(c2)
    per_node2 = np.bincount(conn2.ravel())
    assert per_node2.min() <= 2 and per_node2.max() >= 16
    for et, cc_, cn in ((ol.HEX8, c, conn), (ol.TET4, c2, conn2)):
        pb = of_mesh(et, cc_, cn, "small_J2")
        # three elements in four in set 1: some nodes have no element of set 0
        pb.es = np.ascontiguousarray((np.arange(len(cn)) % 4 != 0).astype(np.int32))
        touched = np.zeros(len(cc_), dtype=bool)
        touched[np.asarray(cn)[pb.es == 0].ravel()] = True
        assert (~touched).any() and touched.any()
        for s in (0, 1):
            run_and_repeat(pb, harness, (qc.AVG_STRESS, s, 0), {0: [0, 3], 1: [1, 2, 3]})


# ---- the entry points ----------------------------------------------------------------------------------------------------
def _hex8_problem():
    et, c, conn = pc.mesh_of("hex8")
    return of_mesh(et, c, conn, "small_J2")


def _k3(asm, st, g0, f, ls):
    g = g0.clone()
    rc = asm.adjoint_jacobian(*st, g, f, ls)
    return rc, g


def test_assign_mode_async_mode_and_the_matrix():
    import torch
    pb = _hex8_problem()
    rng = np.random.default_rng(5)
    asm = pb.assembler()
    assert asm.scatter == "gather"
    st = [asm.dev(a) for a in pb.state]
    g0 = asm.dev(rng.standard_normal(pb.state[5].shape))
    f = asm.dev(rng.standard_normal((asm.nelems, asm.npts, asm.ndofs)))
    asm.set_qoi_subdomain("avg_stress", 1, 0)
    ls = asm.new_linsys()
    rc, g_add = _k3(asm, st, g0, f, ls)
    assert rc == 0
    # assign mode on a system full of other numbers = add mode on a zeroed one
    asm.set_assign_mode(True)
    ls2 = asm.new_linsys()
    ls2.flat.copy_(asm.dev(rng.standard_normal(ls2.flat.numel())))
    rc, g_as = _k3(asm, st, g0, f, ls2)
    assert rc == 0 and torch.equal(g_as, g_add)
    assert torch.equal(ls2.flat, ls.flat)
    # ... and with the row sums in two parts the second part would overwrite -dJ/dx: refused
    asm.set_gather_early_nodes(0, asm.nnodes // 2)
    with pytest.raises(RuntimeError, match="subdomain objective"):
        _k3(asm, st, g0, f, asm.new_linsys())
    asm.set_gather_early_nodes(0, 0)
    asm.set_assign_mode(False)
    # add mode with two-part row sums is fine: the same system after c8_gather_finish
    asm.set_gather_early_nodes(0, asm.nnodes // 2)
    ls3 = asm.new_linsys()
    rc, g_two = _k3(asm, st, g0, f, ls3)
    assert rc == 0 and asm.gather_finish() == 0
    assert torch.equal(g_two, g_add) and float((ls3.flat - ls.flat).abs().max()) <= TOL * float(ls.flat.abs().max())
    asm.set_gather_early_nodes(0, 0)
    # the matrix does not depend on the objective: the bits of the average-displacement run
    asm.set_qoi_avg_disp()
    ls4 = asm.new_linsys()
    rc, _ = _k3(asm, st, g0, f, ls4)
    assert rc == 0
    for i in range(2):
        for j in range(2):
            assert torch.equal(ls4.A[i][j], ls.A[i][j]) and float(ls.A[i][j].abs().max()) > 0
    assert not torch.equal(ls4.b[0], ls.b[0])
    # async mode: the four entry points return with their work still queued behind a long kernel, and the status is clean
    asm.set_qoi_subdomain("avg_stress", 1, 0)
    asm.set_active(1, [0, 3])
    asm.set_async(True)
    big = torch.randn(4096, 4096, dtype=torch.float64, device=asm.device)
    J, grad = asm.dev(np.zeros(1)), asm.dev(np.zeros(asm.num_grad_params))
    z_u, z_p, phi = asm.dev(np.zeros(asm.nnodes * 3)), asm.dev(np.zeros(asm.nnodes)), torch.zeros_like(g0)
    ls5, g5, gw, fw = asm.new_linsys(), g0.clone(), g0.clone(), f.clone()
    torch.cuda.synchronize()
    acc = big
    for _ in range(40):
        acc = acc @ big * 1e-2
    assert asm.adjoint_jacobian(*st, g5, f, ls5) == 0
    assert asm.solve_adjoint_local(*st, z_u, z_p, phi, gw, fw) == 0
    assert asm.qoi_gradient(*st, z_u, z_p, phi, grad) == 0
    assert asm.eval_qoi(st[0], st[1], J, xi_prev=st[4], xi=st[5], u_prev=st[2], p_prev=st[3]) == 0
    done = torch.cuda.Event()
    done.record()
    queued = not done.query()
    torch.cuda.synchronize()
    assert queued, "an entry point waited for the device in async mode"
    assert asm.status() == 0
    asm.set_async(False)
    assert torch.equal(g5, g_add) and torch.equal(ls5.flat, ls.flat) and float(J.item()) > 0 and float(grad.abs().max()) > 0


def test_closed_form_kernels_are_still_the_ones_chosen_on_hex8_small_J2(harness):
    """under C8_KERNEL_AUTO the subdomain objective keeps the row-per-node K3 and the closed-form K4: A, b without the
    objective's share and phi carry the bits of C8_KERNEL_NODE and not those of the wave kernels -- and agree with the
    average-displacement run once that run's own share, -dJ/dx = -w dv N_a / 3 per component, is taken out the same way"""
    import torch
    pb = of_case("small_J2-hex8")   # a converged state: the closed forms are those of the converged local solve
    rng = np.random.default_rng(6)
    g0h = rng.standard_normal(pb.state[5].shape)
    res = {}
    for kernel in ("auto", "node", "wave"):
        asm = pb.assembler()
        asm.set_kernel(kernel)
        asm.set_active(0, [0, 2, 3])
        st = [asm.dev(a) for a in pb.state]
        f = asm.dev(np.random.default_rng(7).standard_normal((asm.nelems, asm.npts, asm.ndofs)))
        asm.set_qoi_subdomain("avg_stress", pb.empty, 0)      # the zero objective: b without the objective's share
        ls = asm.new_linsys()
        rc, g = _k3(asm, st, asm.dev(g0h), f, ls)
        assert rc == 0
        z_u, z_p = asm.dev(1e-3 * np.random.default_rng(8).standard_normal(asm.nnodes * 3)), asm.dev(1e-3 * np.random.default_rng(9).standard_normal(asm.nnodes))
        phi, gw, fw = torch.zeros_like(g), g.clone(), f.clone()
        assert asm.solve_adjoint_local(*st, z_u, z_p, phi, gw, fw) == 0
        grad = asm.dev(np.zeros(3))
        assert asm.qoi_gradient(*st, z_u, z_p, phi, grad) == 0
        res[kernel] = (ls.flat.clone(), phi.clone(), grad.clone())
        if kernel == "auto":
            asm.set_qoi_avg_disp()
            ls_a = asm.new_linsys()
            rc, _ = _k3(asm, st, asm.dev(g0h), f, ls_a)
            assert rc == 0
            _, N, wdv = cc.point_tables(pb.et, pb.c, pb.conn)
            share = np.zeros((len(pb.c), 3))
            np.add.at(share, pb.conn, np.einsum("ep,epn->en", wdv, N)[..., None] / 3.0 * np.ones(3))
            b0 = ls_a.b[0].cpu().numpy().reshape(-1, 3) + share
            ref = ls.b[0].cpu().numpy().reshape(-1, 3)
            assert np.abs(b0 - ref).max() <= TOL * np.abs(ref).max()
            assert torch.equal(ls_a.b[1], ls.b[1])
            for i in range(2):
                for j in range(2):
                    assert torch.equal(ls_a.A[i][j], ls.A[i][j])
    for k in range(2):  # the system and phi: fixed summation orders, so the kernel that ran shows in the bits
        assert torch.equal(res["auto"][k], res["node"][k])
        assert not torch.equal(res["auto"][k], res["wave"][k])
        assert float((res["auto"][k] - res["wave"][k]).abs().max()) <= 1e-10 * float(res["wave"][k].abs().max())
    # K5 adds its per-group sums to grad with atomics (c8_assemble_adjoint.hpp: param_gradient_flush): its bits depend on the
    # order in which the groups arrive, whatever kernel ran, so the three gradients are compared to rounding only
    for other in ("node", "wave"):
        assert float((res["auto"][2] - res[other][2]).abs().max()) <= 1e-10 * float(res[other][2].abs().max())
