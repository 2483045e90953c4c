"""`-m gpu`: the row-per-node kernels read and write a node's CSR rows through buffer descriptors over exactly the row's bytes
(c8_assemble_node.hpp: row_load / row_store; GpuExec in c8_kernels.hip) -- the address unit gives 0 for a load past the
row's end and drops a store there -- and zero the whole row accumulator.  The meshes and the second plastic step of
node_rows_rowio_cases.py on the device (pinched_bricks runs the form for nodes with more than eight elements, the others
the lean one):
  1. `node` against the oracle at the suite's bar and against `wave` at 1e-13 (K1, stored state) and 1e-12 (K3); two runs bit
     for bit;
  2. rows assembled onto a distinct sentinel per entry, every array between guard words (test_gpu_launch_edges.Guarded):
     sentinel + row with one addition, assign mode = zero-then-accumulate without -0, the whole range of nodes in two parts,
     and a strict interior node range [first, end) alone (c8_set_gather_early_nodes): every entry of every other row keeps
     its bits, and so do the rows of a node without elements;
  3. every parameter of every set changed with c8_set_params and set back, against fresh contexts.
The device twin of test_emul_node_rows_rowio.py."""
import functools

import numpy as np
import pytest

import node_rows_rowio_cases as rc
import oracle_lib as ol
from test_gpu_launch_edges import GuardedSystem

pytestmark = pytest.mark.gpu
TOL = 1e-12  # test_gpu_parity.py


def _make(name, kernel, params=None, **kw):
    from gpu_backend import GpuBackend
    c, conn, es, prm = rc.mesh(name)
    return GpuBackend(ol.HEX8, c, conn, "small_J2", prm if params is None else params, scatter="gather", kernel=kernel, elem_set=es, **kw)


@functools.lru_cache(maxsize=None)
def _backend(name, kernel):
    return _make(name, kernel)


@functools.lru_cache(maxsize=None)
def _second_step(name, kernel):
    """computed once, shared by the tests and left unchanged: (forward system, state, adjoint system)"""
    return rc.forward_and_adjoint(_backend(name, kernel), name)


def test_meshes_reach_the_edges():
    rc.assert_meshes_reach_the_edges()


@pytest.mark.parametrize("name", rc.MESHES)
def test_second_step_against_oracle_and_wave(name):
    ls, xi, adj = _second_step(name, "node")
    rc.check_against_oracle(name, ls, xi, adj, TOL)
    rc.check_against_wave(name, ls, xi, adj, *_second_step(name, "wave"))
    assert rc.same_results(rc.forward_and_adjoint(_backend(name, "node"), name), (ls, xi, adj))


def _guarded_run(be, name):
    """run(kind, arrays, assign, parts) of node_rows_rowio_cases.py on the device: the six arrays in six guarded buffers,
    the guard words compared after every launch"""
    import torch
    asm = be.asm
    u1, p1, xi1, u2, p2 = rc.steps(name)
    state = [asm.dev(v) for v in (u2, p2, u1, p1, xi1)]
    xi_ref = asm.dev(rc.reference(name)[1])
    g, f = (asm.dev(v) for v in rc.history(be))

    def snapshot(gs, host):
        torch.cuda.synchronize()
        gs.finish(host)  # asserts the guard words intact and copies the arrays
        return [a.copy() for a in rc.blocks(host)]

    def run(kind, arrays, assign, parts):
        host = be.new_linsys()
        for a, v in zip(rc.blocks(host), arrays):
            a[:] = v
        gs = GuardedSystem(asm, host)
        n = be.nnodes
        first, end = {"whole": (0, 0), "two": (n // 2, n)}.get(parts, parts)
        xi_out, g_io = asm.new_state(), g.clone()  # alive until c8_gather_finish has launched the remaining rows
        asm.set_assign_mode(assign)
        asm.set_gather_early_nodes(first, end)
        try:
            if kind == "K1":
                assert asm.forward_jacobian(*state, xi_out, gs) == 0
            else:
                assert asm.adjoint_jacobian(*state, xi_ref, g_io, f, gs) == 0
            out = snapshot(gs, host)        # a node range: the rows of [first, end) alone
            assert asm.gather_finish() == 0  # ... and the rows around it (nothing after a whole launch)
            if parts == "two":
                out = snapshot(gs, host)
            else:
                torch.cuda.synchronize()
        finally:
            asm.set_gather_early_nodes(0, 0)
            asm.set_assign_mode(False)
        return out
    return run


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("name", rc.MESHES)
def test_rows_onto_sentinels_between_guards(name, kind):
    be = _backend(name, "node")
    n = be.nnodes
    # a strict interior range, and the two single rows next to the mesh's largest: their neighbours' rows on both sides
    big = int(np.argmax(np.diff(np.asarray(rc.oracle(name).rowptr[1][1]))))
    ranges = {rc.interior_range(name), (max(1, min(big, n - 2)), max(1, min(big, n - 2)) + 1)}
    rc.check_rows_and_sentinels(name, kind, _guarded_run(be, name), sorted(ranges))


@pytest.mark.parametrize("kind", rc.KINDS)
def test_a_node_without_elements_keeps_its_rows(kind):
    """brick222 with one more node that no element has, coupled to node 0 in the graph (a phantom column of a mesh part): its
    rows -- three entries of b_u, one of b_p, its graph row in the four blocks -- keep their bits in both modes"""
    from gpu_backend import GpuBackend
    name = "brick222"
    c, conn, es, prm = rc.mesh(name)
    n = len(c)
    c2 = np.vstack([c, [[2.0, 2.0, 2.0]]])
    be = GpuBackend(ol.HEX8, c2, conn, "small_J2", prm, scatter="gather", kernel="node", extra_pairs=[[n, 0], [0, n], [n, n]])
    nodeptr = np.asarray(be.rowptr[1][1])
    assert be.nnodes == n + 1 and nodeptr[n + 1] - nodeptr[n] >= 1 and not (conn == n).any()
    u1, p1, xi1, u2, p2 = rc.steps(name)
    pad = lambda u, k: np.concatenate([u, np.full(k, 0.125)])  # noqa: E731
    fields = (pad(u2, 3), pad(p2, 1), pad(u1, 3), pad(p1, 1))
    g, f = rc.history(be)
    lo, hi = int(nodeptr[n]), int(nodeptr[n + 1])
    for assign in (False, True):
        be.asm.set_assign_mode(assign)
        try:
            ls = be.new_linsys()
            P = rc.sentinels([a.shape for a in rc.blocks(ls)])
            for a, v in zip(rc.blocks(ls), P):
                a[:] = v
            if kind == "K1":
                assert be.forward_jacobian(*fields, xi1.copy(), be.new_state(), ls) == 0
            else:
                assert be.adjoint_jacobian(*fields, xi1.copy(), rc.reference(name)[1].copy(), g, f, ls) == 0
        finally:
            be.asm.set_assign_mode(False)
        got = rc.blocks(ls)
        for k, width in enumerate((9, 3, 3, 1)):
            assert np.array_equal(rc.bits(got[k][width * lo:width * hi]), rc.bits(P[k][width * lo:width * hi])), (k, assign)
            assert not np.array_equal(got[k][:width * lo], P[k][:width * lo])  # the other rows were assembled
        assert np.array_equal(rc.bits(got[4][3 * n:]), rc.bits(P[4][3 * n:])) and np.array_equal(rc.bits(got[5][n:]), rc.bits(P[5][n:]))


@pytest.mark.parametrize("name", rc.MESHES)
def test_parameters_changed_and_set_back(name):
    rc.check_params_followed(name, lambda prm: _make(name, "node", prm))
