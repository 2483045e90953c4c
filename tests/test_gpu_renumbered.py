"""`-m gpu`: the hex8 kernels on meshes with shuffled node ids, shuffled element order and rotated local node order
(renumber_cases.py), through GpuBackend / Assembler.  The oracle built on the renumbered mesh is the reference (it is held
against itself through the renumbering maps in test_emul_renumbered.py); the bar is the parity bar, or that of the file a
check is borrowed from.  Beyond the kernel bodies, which the emulator runs on the CPU, this covers what exists on the device
alone: the launch wrappers, the lane exchange, the tables c8_api.hip uploads, the ring on two streams, the colour batches,
the per-point kernels, the boundary kernels, SPR and the Krylov set-up."""
import functools

import numpy as np
import pytest

import node_rows_xlane_cases as xl
import oracle_lib as ol
import renumber_cases as rn
from parity_cases import (HJ2, HOSFORD, J2, LOCAL_LINE_SEARCH, check_adjoint_chain, check_forward, check_residual,
                          check_two_element_sets)

pytestmark = pytest.mark.gpu
TOL = 1e-12


def backend(c, conn, model, params, kernel, scatter, **kw):
    from gpu_backend import GpuBackend
    return GpuBackend(ol.HEX8, c, conn, model, params, scatter=scatter, kernel=kernel, **kw)


@functools.lru_cache(maxsize=None)
def oracle433(model):
    c, conn, _ = rn.shuffled433()
    return ol.Oracle(ol.HEX8, c, conn, model, {"small_J2": J2, "hyper_J2": HJ2}[model])


# ---- (a) parity on shuffled433 ---------------------------------------------------------------------------------------------
PAIRS = [("small_J2", J2, k, s) for k, s in (("auto", "gather"), ("node", "gather"), ("wave", "gather"), ("wave", "colored"),
                                             ("wave", "atomic"), ("wave_ad", "gather"), ("slot", "colored"), ("slot", "atomic"))] + \
        [("hyper_J2", HJ2, "wave", "gather"), ("hyper_J2", HJ2, "slot", "colored")]


@pytest.mark.parametrize("model,params,kernel,scatter", PAIRS, ids=["%s-%s-%s" % (m, k, s) for m, _, k, s in PAIRS])
def test_parity_on_shuffled433(model, params, kernel, scatter):
    c, conn, _ = rn.shuffled433()
    orc, gpu = oracle433(model), backend(c, conn, model, params, kernel, scatter)
    for i in range(2):
        for j in range(2):  # the graphs the device built from this numbering are the oracle's
            assert np.array_equal(gpu.rowptr[i][j], orc.rowptr[i][j]) and np.array_equal(gpu.colidx[i][j], orc.colidx[i][j])
    check_forward(orc, gpu, c, model, 0.004, TOL)
    check_adjoint_chain(orc, gpu, c, model, 0.004, TOL)


def test_parity_of_the_line_search_model_on_shuffled433():
    # small_hosford through the library's own choice on hex8: the wave-per-element kernels, staged
    c, conn, _ = rn.shuffled433()
    orc = ol.Oracle(ol.HEX8, c, conn, "small_hosford", HOSFORD)
    orc.set_local_line_search(*LOCAL_LINE_SEARCH)
    gpu = backend(c, conn, "small_hosford", HOSFORD, "auto", None, line_search=LOCAL_LINE_SEARCH)
    check_forward(orc, gpu, c, "small_hosford", 0.004, TOL)
    check_adjoint_chain(orc, gpu, c, "small_hosford", 0.004, TOL)


@pytest.mark.parametrize("kernel,scatter", [("auto", "atomic"), ("slot", "colored")])
def test_residual_only_on_shuffled433(kernel, scatter):
    # the eight-elements-per-wavefront residual kernel (atomic), the lane-group one (slot)
    c, conn, _ = rn.shuffled433()
    check_residual(oracle433("small_J2"), backend(c, conn, "small_J2", J2, kernel, scatter), c, 0.004, TOL)


def test_row_per_node_kernel_in_two_parts_on_shuffled433():
    # c8_set_gather_early_nodes over an arbitrary id range + c8_gather_finish: the bits of the one-part run, K1 and K3
    import torch
    from calibr8_amd import Assembler
    from meshes import prescribed_fields
    c, conn, _ = rn.shuffled433()
    asm = Assembler(8, c, conn, "small_J2", J2, scatter="gather")
    asm.set_kernel("node")
    u_h, p_h = prescribed_fields(c, 0.004, ramp=True, perturb=5e-2)
    u, p = asm.dev(u_h), asm.dev(p_h)
    z, zp = torch.zeros_like(u), torch.zeros_like(p)
    g_h, f_h = rn.histories(asm)
    g, f = asm.dev(g_h), asm.dev(f_h)
    xi0 = asm.new_state()

    def run():
        ls, xi, la, gg = asm.new_linsys(), asm.new_state(), asm.new_linsys(), g.clone()
        assert asm.forward_jacobian(u, p, z, zp, xi0, xi, ls) == 0
        assert asm.gather_finish() == 0
        assert asm.adjoint_jacobian(u, p, z, zp, xi0, xi, gg, f, la) == 0
        assert asm.gather_finish() == 0  # (gg lives until here: the second part reads it)
        asm.torch.cuda.synchronize()
        return ls.flat.clone(), xi.clone(), la.flat.clone()

    ref = run()
    assert float((ref[1][:, :, 6] > 0).double().mean()) > 0.3
    nn = len(c)
    for lo, hi in ((7, 31), (nn - 1, nn), (0, nn)):
        asm.set_gather_early_nodes(lo, hi)
        ls, xi = asm.new_linsys(), asm.new_state()
        assert asm.forward_jacobian(u, p, z, zp, xi0, xi, ls) == 0
        r3 = asm.rowptr[0][0]
        a, b = int(r3[3 * lo]), int(r3[3 * hi])
        assert torch.equal(ls.A[0][0][a:b], ref[0][:asm.nnz[0][0]][a:b])  # after the first part exactly the early rows are complete
        if hi - lo < nn:
            assert not torch.equal(ls.flat, ref[0])
        assert asm.gather_finish() == 0
        assert torch.equal(ls.flat, ref[0]) and torch.equal(xi, ref[1])
        got = run()
        assert all(torch.equal(a_, b_) for a_, b_ in zip(got, ref))
    asm.set_gather_early_nodes(0, 0)


# ---- (b) where local indices repeat, sixteen elements at a node, two element sets ------------------------------------------
@pytest.mark.parametrize("kernel", ["node", "wave"])
@pytest.mark.parametrize("name", rn.CHAIN_MESHES)
def test_parity_of_node_and_wave_kernels(name, kernel):
    c, conn, es, prm = xl.mesh(name)
    if es is not None:
        def factory(et, c, conn, model, params, **kw):
            return backend(c, conn, model, params, kernel, "gather", **kw)
        check_two_element_sets(factory, "hex8", TOL, mesh=(ol.HEX8, c, conn, es))
        return
    orc, gpu = ol.Oracle(ol.HEX8, c, conn, "small_J2", prm), backend(c, conn, "small_J2", prm, kernel, "gather")
    check_forward(orc, gpu, c, "small_J2", 0.004, TOL)
    check_adjoint_chain(orc, gpu, c, "small_J2", 0.004, TOL)


@functools.lru_cache(maxsize=None)
def _chain_backend(name, kernel):
    c, conn, es, prm = xl.mesh(name)
    return backend(c, conn, "small_J2", prm, kernel, "gather", elem_set=es)


@functools.lru_cache(maxsize=None)
def _second_step(name, kernel):
    """the second plastic step of node_rows_chain_cases.py, computed once and left unchanged: (forward system, state, adjoint system)"""
    be = _chain_backend(name, kernel)
    ls, xi = xl.forward(be, name)
    return ls, xi, xl.adjoint(be, name, xi)


@pytest.mark.parametrize("name", rn.CHAIN_MESHES)
def test_second_plastic_step_node_against_oracle_and_wave(name):
    ls, xi, ls_adj = _second_step(name, "node")
    xl.check_against_oracle(name, ls, xi, ls_adj, TOL)
    xl.check_against_oracle(name, *_second_step(name, "wave"), TOL)
    xl.check_against_wave(name, ls, xi, ls_adj, *_second_step(name, "wave"))
    be = _chain_backend(name, "node")  # two runs bit for bit
    ls2, xi2 = xl.forward(be, name)
    assert xl.same_bits(ls2, ls) and np.array_equal(xi2, xi) and xl.same_bits(xl.adjoint(be, name, xi), ls_adj)


@pytest.mark.parametrize("name", rn.CHAIN_MESHES)
def test_assign_mode_over_stale_content(name):
    be = _chain_backend(name, "node")
    xl.check_assign_and_accumulate(name, be, be.asm.set_assign_mode)


# ---- (c) the ring ------------------------------------------------------------------------------------------------------------
def _ring_backend(overlap):
    c, conn, _ = rn.bar_windowed()
    gpu = backend(c, conn, "small_J2", J2, "wave", "gather")  # `wave`: the default kernel of small_J2 does not stage
    gpu.asm.set_stage_chunk(4)
    gpu.asm.set_stage_overlap(overlap)
    return gpu, c, conn


@pytest.mark.parametrize("overlap", [False, True])
def test_staged_ring_on_bar_windowed(overlap):
    # chunks of the element bandwidth (at most 20, at least five of them: asserted in renumber_cases.bar_windowed) through the
    # ring of three; with overlap the row sums of chunk k on the second stream beside the assembly of chunk k + 1
    gpu, c, conn = _ring_backend(overlap)
    orc = ol.Oracle(ol.HEX8, c, conn, "small_J2", J2)
    check_forward(orc, gpu, c, "small_J2", 0.004, TOL)
    check_adjoint_chain(orc, gpu, c, "small_J2", 0.004, TOL)


def test_staged_ring_overlap_gives_the_same_bits():
    from meshes import prescribed_fields
    gpu, c, conn = _ring_backend(True)
    u, p = prescribed_fields(c, 0.004, ramp=True)
    z, zp = np.zeros_like(u), np.zeros_like(p)
    out = []
    for on in (True, False):
        gpu.asm.set_stage_overlap(on)
        ls = gpu.new_linsys()
        for _ in range(3):  # accumulates: three assemblies into the same system
            assert gpu.forward_jacobian(u, p, z, zp, gpu.new_state(), gpu.new_state(), ls) == 0
        out.append(ls)
    assert xl.same_bits(out[0], out[1]) and np.abs(out[0].A[0][0]).max() > 0
    # and it is the ring that ran: one chunk of the whole mesh sums every row in one pass over the stage, in the same order
    gpu.asm.set_stage_chunk(len(conn))
    ls = gpu.new_linsys()
    for _ in range(3):
        assert gpu.forward_jacobian(u, p, z, zp, gpu.new_state(), gpu.new_state(), ls) == 0
    assert xl.same_bits(ls, out[0])


# ---- (d) equivariance on the device, independent of the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["node", "wave"])
def test_device_is_equivariant_under_the_renumbering(kernel):
    c0, conn0 = rn.brick433()
    c, conn, rec = rn.shuffled433()
    old, new = backend(c0, conn0, "small_J2", J2, kernel, "gather"), backend(c, conn, "small_J2", J2, kernel, "gather")
    errs, (x0, x1) = rn.renumbered_pair_errors(rec, old, new, c0)
    print("%s: shuffled433 against the brick through the maps: %s" % (kernel, {k: "%.1e" % v for k, v in errs.items()}))
    assert max(errs.values()) < TOL, errs
    xe = x0[rec.pe]
    assert np.abs(x1 - xe).max() > 1e-6 * np.abs(xe).max()  # the point map matters
    again, _ = rn.renumbered_pair_errors(rec, old, new, c0)
    assert again == errs  # (the same bits give the same figures; the systems themselves: below)
    from meshes import prescribed_fields
    u, p = prescribed_fields(c, 0.004, ramp=True, perturb=5e-2)
    runs = []
    for _ in range(2):
        ls, xi = new.new_linsys(), new.new_state()
        assert new.forward_jacobian(u, p, 0 * u, 0 * p, new.new_state(), xi, ls) == 0
        g, f = rn.histories(new)
        la = new.new_linsys()
        assert new.adjoint_jacobian(u, p, 0 * u, 0 * p, new.new_state(), xi, g, f, la) == 0
        runs.append((ls, xi, la))
    assert xl.same_bits(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and xl.same_bits(runs[0][2], runs[1][2])


# ---- (e) the per-point entry points -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cauchy_harness(tmp_path_factory):
    import cauchy_cases as cc
    return cc.build_harness(tmp_path_factory.mktemp("c8_cauchy_host_renumbered"))


@pytest.fixture(scope="module")
def error_harness(tmp_path_factory):
    import error_cases as ec
    return ec.build_harness(tmp_path_factory.mktemp("c8_error_host_renumbered"))


@pytest.fixture(scope="module")
def exact_harness(tmp_path_factory):
    import exact_cases as xc
    return xc.build_harness(tmp_path_factory.mktemp("c8_exact_host_renumbered"))


@pytest.fixture(scope="module")
def qoi_harness(tmp_path_factory):
    import qoi_cases as qc
    return qc.build_harness(tmp_path_factory.mktemp("c8_qoi_host_renumbered"))


POINT_MODELS = [("small_J2", J2), ("hyper_J2", HJ2)]


def _assembler433(model, params):
    from calibr8_amd import Assembler
    c, conn, _ = rn.shuffled433()
    return Assembler(8, c, conn, model, params), c, conn


@pytest.mark.parametrize("model,params", POINT_MODELS)
def test_cauchy_on_shuffled433(cauchy_harness, model, params):
    import cauchy_cases as cc
    import test_gpu_cauchy as tc
    asm, c, conn = _assembler433(model, params)
    state = cc.synthetic_state(asm.new_state().cpu().numpy(), c, asm.ndims, asm.nres, seed=36)
    ref = cc.host_cauchy(cauchy_harness, ol.HEX8, c, conn, model, params, *state)
    tc.assert_close(tc.device_cauchy(asm, state), ref, ("shuffled433", model))
    assert len(np.unique(np.round(ref[:, :, 0, 0] / np.abs(ref).max(), 9))) == ref.shape[0] * ref.shape[1]  # no two points alike
    # the harness itself under the renumbering: the brick's stresses at the brick's state, through the point map
    c0, conn0 = rn.brick433()
    rec = rn.shuffled433()[2]
    u, p, u_prev, p_prev, xi_prev, xi = state
    old = [rec.back(u, 3), rec.back(p, 1), rec.back(u_prev, 3), rec.back(p_prev, 1)] + \
        [rec.points_back(x) for x in (xi_prev, xi)]
    ref0 = cc.host_cauchy(cauchy_harness, ol.HEX8, c0, conn0, model, params, *old)
    assert np.abs(rec.points(ref0) - ref).max() < TOL * np.abs(ref).max()


@pytest.mark.parametrize("model,params", POINT_MODELS)
def test_error_contributions_on_shuffled433(error_harness, model, params):
    import error_cases as ec
    import test_gpu_error as te
    asm, c, conn = _assembler433(model, params)
    state, adj = te._synthetic(asm, c, seed=36)
    ref = ec.host_error(error_harness, ol.HEX8, c, conn, model, params, *state, *adj, scales=True)
    te.assert_close(te.device_error(asm, state, adj), ref, ("shuffled433", model), state, adj[2])
    assert len(np.unique(np.round(ref[0] / np.abs(ref[0]).max(), 9))) == len(conn)  # no two elements alike


@pytest.mark.parametrize("model,params", POINT_MODELS)
def test_exact_errors_on_shuffled433(exact_harness, model, params):
    import exact_cases as xc
    import test_gpu_exact_errors as tx
    asm, c, conn = _assembler433(model, params)
    state, fine, adj = tx._synthetic(asm, c, seed=36)
    for lin in (False, True):
        ref = xc.host_exact(exact_harness, ol.HEX8, c, conn, model, params, state, fine, *adj, lin=lin, scales=True)
        tx.assert_close(tx.device_exact(asm, state, fine, adj, lin=lin), ref, ("shuffled433", model, lin), state, fine, adj[2])
        assert len(np.unique(np.round(ref[0] / np.abs(ref[0]).max(), 9))) == len(conn)


@pytest.mark.parametrize("model", ["small_J2", "hyper_J2"])
def test_subdomain_objectives_on_shuffled433(qoi_harness, model):
    # two interleaved element sets with different parameters plus the empty one (test_gpu_qoi_point.of_mesh)
    import qoi_cases as qc
    import test_gpu_qoi_point as tq
    c, conn, _ = rn.shuffled433()
    pb = tq.of_mesh(ol.HEX8, c, conn, model)
    act = {0: [0, 3], 1: [1, 2, 3]}
    for s in (0, 1):
        tq.run_and_repeat(pb, qoi_harness, (qc.AVG_STRESS, s, 0), act)
    tq.run_and_repeat(pb, qoi_harness, (qc.DISP_COMP, 0, 1), act)
    tq.run_and_repeat(pb, qoi_harness, (qc.AVG_LOCAL_VAR, 0, 6), act)


# ---- (f) boundary kernels on the assembled system ---------------------------------------------------------------------------
def test_dirichlet_rows_and_apply_A_on_the_assembled_shuffled433_system():
    import torch
    import bc_ref as R
    import test_gpu_boundary as tb
    from meshes import prescribed_fields
    asm, c, conn = _assembler433("small_J2", J2)
    rec = rn.shuffled433()[2]
    u_h, p_h = prescribed_fields(c, 0.004, ramp=True, perturb=5e-2)
    u, p = asm.dev(u_h), asm.dev(p_h)
    ls = asm.new_linsys()
    assert asm.forward_jacobian(u, p, torch.zeros_like(u), torch.zeros_like(p), asm.new_state(), asm.new_state(), ls) == 0
    torch.cuda.synchronize()
    P = ls.flat.cpu().numpy().copy()
    rng = np.random.default_rng(14)
    x = [rng.standard_normal(asm.nnodes * 3), rng.standard_normal(asm.nnodes)]
    tb.check_apply_A(asm, ls, P, x)
    # two conditions that share nodes (the brick's face x = 0 and its edge x = 0, y = 0 .. in scattered ids), and one on p
    c0 = rn.brick433()[0]
    face = rec.node_set(np.nonzero(c0[:, 0] < 1e-12)[0])
    strip = rec.node_set(np.nonzero(c0[:, 1] < 1e-12)[0])
    assert len(np.intersect1d(face, strip)) >= 4 and (np.diff(face) > 1).any()
    dbcs = [(0, 1, face, tb.values(face, 1)), (0, 1, strip, tb.values(strip, 2)), (0, 0, face, tb.values(face, 3)),
            (1, 0, strip, tb.values(strip, 4))]
    dd = [(r, e, torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(v)) for r, e, n, v in dbcs]
    assert asm.apply_dirichlet(dd, asm.dev(x[0]), asm.dev(x[1]), ls) == 0
    torch.cuda.synchronize()
    A0, b0 = tb.blocks(asm, P)
    A1, b1 = R.dirichlet_ref(asm.rowptr, asm.colidx, A0, b0, x, dbcs, False, neq=asm.neq)
    flat = ls.flat.cpu().numpy()
    A, b = tb.blocks(asm, flat)
    for i in range(2):
        assert np.array_equal(b[i], b1[i])
        for j in range(2):
            assert np.array_equal(A[i][j], A1[i][j])
    tb.check_apply_A(asm, ls, flat, x)


# ---- (g) SPR ----------------------------------------------------------------------------------------------------------------
SPR_MESHES = ["brick3_jiggled_renumbered", "pinched_bricks_renumbered"]


@pytest.fixture(scope="module")
def spr_harness(tmp_path_factory):
    import spr_cases as sc
    return sc.Harness(tmp_path_factory.mktemp("c8_spr_host_renumbered"))


@pytest.mark.parametrize("name", SPR_MESHES)
def test_spr_tables_recovery_and_affine_field(spr_harness, name):
    import torch
    import spr_cases as sc
    import test_gpu_spr as ts
    from calibr8_amd.error import spr_smooth
    asm = ts.assembler(name)
    # the device tables against c8_spr_build_host (test_device_tables_equal_the_host_setup, its bars)
    dev, host = asm.spr_patches(), sc.host_tables(name)
    assert np.array_equal(dev["patch_ptr"], host["patch_ptr"]) and np.array_equal(dev["patch_elems"], host["patch_elems"])
    assert np.array_equal(dev["stages"], host["stages"]) and dev["setup"][3] == 0
    assert all(sc.as_lists(host)[n] == sc.patches_ref(name)[0][n] for n in range(asm.nnodes))
    et, coords, conn = sc.mesh(name)
    _, kappa, _ = sc.lstsq_ref(name, sc.as_lists(host), np.zeros((len(conn), 8, 1)))
    assert kappa.max() < 1e3
    err = np.abs(dev["g"] - host["g"]).max(axis=1)
    bar = 1e-12 * np.maximum(1.0, (kappa / 10.0) ** 2) * np.abs(host["g"]).max(axis=1)
    assert (err <= bar).all() and np.abs(dev["h"] / host["h"] - 1).max() < 1e-14
    # the recovery against the sequential host sum (test_recover_against_the_sequential_host_sum, its bar)
    for ncomp in (1, 9):
        field = sc.random_field(name, ncomp)
        ref, mag = spr_harness.apply(name, dev, field)
        got = asm.spr_recover(asm.dev(field)).cpu().numpy().reshape(ref.shape)
        assert np.isfinite(got).all() and (np.abs(got - ref) <= 1e-12 * mag).all(), (name, ncomp)
    # an affine field comes back as it is, whatever the numbering (test_spr_smooth_returns_an_affine_nodal_field, its bar)
    nodal = sc.affine(et, coords)
    got = spr_smooth(asm, asm.dev(nodal))
    torch.cuda.synchronize()
    assert np.abs(got.cpu().numpy() - nodal).max() <= 1e-13 * np.abs(nodal).max()


# ---- (h) the Krylov set-up on a renumbered notched bar -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def krylov_system():
    """K1 of notched_bar(16, 4, 4) renumbered at a plastic state + Dirichlet rows, as test_gpu_krylov.device_system builds
    it, and its host copy; the tests leave the matrix and b as they are"""
    import torch
    from calibr8_amd import Assembler
    from meshes import prescribed_fields
    from test_gpu_krylov import host_system
    c, conn, sets, _ = rn.notched_shuffled()
    spec = [(0, d, sets["xmin"]) for d in range(3)] + [(0, 0, sets["xmax"])]
    asm = Assembler(8, c, conn, "small_J2", J2)
    u, p = prescribed_fields(c, 0.004, ramp=True)
    U, P = asm.dev(u), asm.dev(p)
    ls, xi = asm.new_linsys(), asm.new_state()
    assert asm.forward_jacobian(U, P, torch.zeros_like(U), torch.zeros_like(P), asm.new_state(), xi, ls) == 0
    assert float(xi[:, :, -1].max()) > 0.0  # a plastic state
    dd = [(r, e, torch.as_tensor(np.asarray(n, dtype=np.int32), device=asm.device), asm.dev(np.zeros(len(n)))) for r, e, n in spec]
    asm.apply_dirichlet(dd, U, P, ls)
    torch.cuda.synchronize()
    A, b = host_system(asm, ls)
    return asm, ls, A.tocsr(), b


def test_krylov_colours_aggregates_and_levels_on_the_renumbered_notched_bar():
    from test_gpu_krylov_multilevel import device_levels, levels_replay, multilevel
    from test_gpu_krylov_sgs import device_colors, greedy_colors
    from test_gpu_krylov_two_level import aggregate_replay, device_aggregates
    asm = krylov_system()[0]
    rp, ci = asm.rowptr[1][1], asm.colidx[1][1]
    deg = np.diff(rp)
    assert deg.min() < 12 and deg.max() == 27  # the notch flanks: rows of many shapes
    colors, ref = device_colors(asm), greedy_colors(rp, ci, asm.nnodes)
    assert np.array_equal(np.sort(np.concatenate(colors)), np.arange(asm.nnodes))
    assert len(ref) == len(colors) and all(np.array_equal(a, b) for a, b in zip(ref, colors))
    # on the brick numbering the greedy rule needs eight colours; scattered ids need more
    print("renumbered notched bar: %d nodes, %d colours, sizes %s" % (asm.nnodes, len(colors), [len(k) for k in colors]))
    agg, nagg = device_aggregates(asm)
    ragg, nref = aggregate_replay(rp, ci, asm.nnodes)
    assert nagg == nref and np.array_equal(agg, ragg)
    rl = levels_replay(asm, 100, 8)
    with multilevel(asm, 100):
        dl = device_levels(asm)
    print("  aggregates %d, nodes per level %s" % (nagg, [d[0] for d in dl]))
    assert [L["n"] for L in rl] == [d[0] for d in dl] and len(dl) >= 3
    for lev, (L, (n, a, cols)) in enumerate(zip(rl, dl)):
        if lev == len(dl) - 1:
            assert a is None and cols == []
            continue
        assert np.array_equal(a, L["agg"])
        assert len(cols) == len(L["colors"]) and all(np.array_equal(x, y) for x, y in zip(cols, L["colors"]))


def test_krylov_operators_equal_their_definitions_on_the_renumbered_notched_bar():
    from calibr8_amd import lib
    from test_gpu_krylov_multilevel import EPS, FORCED, Multilevel
    from test_gpu_krylov_multilevel import multilevel as ml_kind
    from test_gpu_krylov_sgs import JACOBI, SGS, Replay, device_apply, device_colors, node_index, precond
    from test_gpu_krylov_two_level import TWO_LEVEL, TwoLevel
    asm, ls, A, b = krylov_system()
    idx = node_index(asm.nnodes, asm.ndims, asm.nres)
    v = np.random.default_rng(11).standard_normal(len(b))
    rel = lambda y, y_ref: np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
    err = {}
    for name, kind, sweeps in (("jacobi", JACOBI, 1), ("sgs1", SGS, 1), ("sgs2", SGS, 2)):
        with precond(asm, kind, sweeps):
            rc, y = device_apply(asm, ls, v)
        assert rc == lib.C8_OK, asm.L.c8_last_error()
        rep = Replay(A, idx, device_colors(asm), sweeps)
        err[name] = rel(y, rep.jacobi(v) if kind == JACOBI else rep.sgs(v))
    # test_gpu_krylov_sgs.test_operator_equals_its_definition
    assert err["jacobi"] < 1e-10 and all(err[k] < 1e-10 and err[k] <= 100.0 * err["jacobi"] for k in ("sgs1", "sgs2")), err
    # test_gpu_krylov_two_level.test_operator_equals_its_definition
    two = TwoLevel(asm, A)
    with precond(asm, TWO_LEVEL):
        rc, y = device_apply(asm, ls, v)
    assert rc == lib.C8_OK, asm.L.c8_last_error()
    err["two_level"], bound2 = rel(y, two.apply(v)), 100.0 * EPS * np.linalg.cond(two.Ac)
    # test_gpu_krylov_multilevel.test_operator_equals_its_definition, three levels
    many = Multilevel(asm, A, *FORCED[3])
    with ml_kind(asm, *FORCED[3]):
        rc, y = device_apply(asm, ls, v)
    assert rc == lib.C8_OK, asm.L.c8_last_error()
    err["multilevel"], bound3 = rel(y, many.apply(v)), 100.0 * EPS * many.cond
    print("renumbered notched bar: operator errors %s, bounds two-level %.2e multilevel %.2e" % ({k: "%.2e" % e for k, e in err.items()}, bound2, bound3))
    assert len(many.levels) == 3 and err["two_level"] <= bound2 and err["multilevel"] <= bound3


@pytest.mark.parametrize("kind", ["jacobi", "sgs", "two_level", "multilevel"])
def test_krylov_solve_meets_its_contract_on_the_renumbered_notched_bar(kind):
    # test_gpu_krylov.test_single_solve_meets_its_contract; the iteration count is printed, not asserted (the numbering
    # changes what a Gauss-Seidel sweep achieves)
    import contextlib
    import scipy.sparse.linalg as spla
    from calibr8_amd import lib
    from test_gpu_krylov import REL_TOL, new_dx, raw_solve
    from test_gpu_krylov_multilevel import FORCED, multilevel
    from test_gpu_krylov_sgs import SGS, precond
    from test_gpu_krylov_two_level import TWO_LEVEL
    asm, ls, A, b = krylov_system()
    ctx = {"jacobi": contextlib.nullcontext, "sgs": lambda: precond(asm, SGS), "two_level": lambda: precond(asm, TWO_LEVEL),
           "multilevel": lambda: multilevel(asm, *FORCED[3])}[kind]
    with ctx():
        rc, info, x = raw_solve(asm, ls, new_dx(asm))
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    lu = spla.splu(A.tocsc())
    x_ref = lu.solve(b)
    inv_op = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    cond_est = spla.onenormest(A) * spla.onenormest(inv_op)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print("renumbered notched bar (%s): n %d rc %d iters %d restarts %d host residual %.3e cond_est %.3e x error %.3e" %
          (kind, len(b), rc, info.iters, info.restarts, res, cond_est, err))
    assert rc == lib.C8_OK and info.status == lib.C8_OK, asm.L.c8_last_error()
    assert info.iters > 0 and res <= 1.01 * REL_TOL
    assert abs(info.residual_norm / np.linalg.norm(b - A @ x) - 1.0) < 1e-6
    assert abs(info.b_norm / np.linalg.norm(b) - 1.0) < 1e-12
    assert err <= cond_est * REL_TOL


# ---- (i) end to end ------------------------------------------------------------------------------------------------------------
def test_primal_and_adjoint_drivers_solve_the_same_problem_in_another_order():
    # two steps of the uniaxial pull of test_gpu_distributed.bcs_for and the adjoint gradient with four active parameters, on
    # a jiggled brick and on its renumbering: that file's bars
    import torch
    from calibr8_amd import Assembler
    from calibr8_amd.primal import PrimalDriver, adjoint_gradient
    from meshes import brick, jiggle
    from test_gpu_distributed import bcs_for
    c0, conn0, sets = brick(6, 4, 3, 1.0, 0.8, 0.7)
    c0 = jiggle(c0, sets, 0.02)
    c, conn, _, rec = rn.renumber(c0, conn0, 17)
    assert (rn.point_jacobians(c, conn) > 0).all()
    act = [0, 1, 2, 3]

    def run(c_, conn_, sets_of):
        asm = Assembler(8, c_, conn_, "small_J2", J2)
        asm.set_active(0, act)
        drv = PrimalDriver(asm, bcs_for(sets_of, c_))
        drv.solve(2)
        J, grad = drv.qoi(), adjoint_gradient(drv, len(act))
        torch.cuda.synchronize()
        return drv, J, grad

    d0, J0, g0 = run(c0, conn0, lambda name: sets[name].astype(np.int32))
    d1, J1, g1 = run(c, conn, lambda name: rec.node_set(sets[name]).astype(np.int32))
    assert list(d1.newton_iters) == list(d0.newton_iters) and max(d0.newton_iters) > 2, (d0.newton_iters, d1.newton_iters)
    u_ref = rec.nodal(d0.u[2].cpu().numpy(), 3)
    du = float(np.abs(d1.u[2].cpu().numpy() - u_ref).max() / np.abs(u_ref).max())
    dxi = float(np.abs(d1.xi[2].cpu().numpy() - rec.points(d0.xi[2].cpu().numpy())).max())
    print("renumbered brick(6, 4, 3): iterations %s, du %.2e, dxi %.2e, J %.15e / %.15e, gradient %s / %s" %
          (list(d1.newton_iters), du, dxi, J1, J0, g1, g0))
    assert float(d0.xi[2][:, :, 6].max()) > 0  # plastic
    assert du < 1e-9 and dxi < 1e-9
    assert abs(J1 - J0) < 1e-9 * abs(J0)
    assert np.abs(g1 - g0).max() < 1e-7 * np.abs(g0).max()
