"""`-m gpu`: the row-per-node kernels (c8_assemble_node.hpp) keep a node's row accumulator in LDS as an image of its four
CSR row blocks and copy it out entry for entry.  These tests pin what that mapping must deliver, on meshes whose node
degrees (8 / 12 / 18 / 27 and beyond) put the block lengths 9 deg, 3 deg and deg on either side of 64, 128 and 192:
every entry meets its own accumulator (the fetch of the old values and the store of the sums address the same entry), two
parts equal one call, runs repeat bit for bit, and the staged wave kernel computes the same system (which is what checks
where phase C puts a block: an assembly compared with itself would move a misplaced value on both sides)."""
import functools

import numpy as np
import pytest

from meshes import brick, jiggle, notched_bar, pinched_bricks, prescribed_fields
from parity_cases import J2

pytestmark = pytest.mark.gpu


def _mesh(name):
    if name == "one_element":          # degree 8
        return brick(1, 1, 1)[:2]
    if name == "brick222":             # degrees 8 / 12 / 18 / 27, nodes with 1 / 2 / 4 / 8 elements
        c, conn, sets = brick(2, 2, 2)
        return jiggle(c, sets, 0.05), conn
    if name == "brick321":
        return brick(3, 2, 1)[:2]
    if name == "notched_bar":
        return notched_bar(10, 6, 3)[:2]
    if name == "pinched_bricks":       # a node with sixteen elements: the kernel's form for more than eight
        return pinched_bricks()
    raise KeyError(name)


MESHES = ["one_element", "brick222", "brick321", "notched_bar", "pinched_bricks"]


@functools.lru_cache(maxsize=None)
def _case(name, kernel="node"):
    """assembler, fields and the states of a forward call on the mesh: built once, shared by the tests, left unchanged"""
    import torch
    from calibr8_amd import Assembler
    c, conn = _mesh(name)
    asm = Assembler(8, c, conn, "small_J2", J2, scatter="gather")
    asm.set_kernel(kernel)
    u_h, p_h = prescribed_fields(c, 0.004, ramp=True, perturb=5e-2)
    u, p = asm.dev(u_h), asm.dev(p_h)
    z, zp = torch.zeros_like(u), torch.zeros_like(p)
    xi0, xi1 = asm.new_state(), asm.new_state()
    assert asm.forward_jacobian(u, p, z, zp, xi0, xi1, asm.new_linsys()) == 0
    gen = torch.Generator(device="cpu").manual_seed(11)
    g = (1e-3 * torch.randn(asm.nelems, asm.npts, asm.nloc, generator=gen, dtype=torch.float64)).to(asm.device)
    f = (1e-3 * torch.randn(asm.nelems, asm.npts, asm.ndofs, generator=gen, dtype=torch.float64)).to(asm.device)
    return asm, (u, p, z, zp, xi0), xi1, g, f


def _prefill(asm, seed):
    """a different value in every entry of the system"""
    import torch
    ls = asm.new_linsys()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    P = (10.0 * (1.0 + torch.rand(ls.flat.numel(), generator=gen, dtype=torch.float64))).to(asm.device)
    assert torch.unique(P).numel() == P.numel()
    ls.flat.copy_(P)
    return ls, P


def _assign_then_accumulate(name, adjoint):
    """R: the assembly in assign mode into garbage; then the assembly in accumulate mode into P.  Returns (P + R, result, states)"""
    import torch
    asm, (u, p, z, zp, xi0), xi1, g, f = _case(name)

    def call(ls):
        if adjoint:
            g_in = g.clone()
            assert asm.adjoint_jacobian(u, p, z, zp, xi0, xi1, g_in, f, ls) == 0
            return g_in
        xi = asm.new_state()
        assert asm.forward_jacobian(u, p, z, zp, xi0, xi, ls) == 0
        return xi

    R = asm.new_linsys()
    R.flat.fill_(-7.25e3)
    asm.set_assign_mode(True)
    try:
        st_R = call(R)
    finally:
        asm.set_assign_mode(False)
    assert not bool((R.flat == -7.25e3).any())  # every node of these meshes has elements: every entry is assigned
    ls, P = _prefill(asm, 5)
    st = call(ls)
    return P + R.flat, ls.flat.clone(), st_R, st


@pytest.mark.parametrize("adjoint", [False, True], ids=["K1", "K3"])
@pytest.mark.parametrize("name", MESHES)
def test_every_entry_meets_its_own_accumulator(name, adjoint):
    # exact: both sides round one addition of the same two doubles.  A sum stored to another entry than the one its old value
    # was fetched from meets another prefilled value, which a zero-filled system would not show.  (Both sides come from the
    # same kernel: an entry that phase C adds into the wrong place of the image is test_agrees_with_staged_wave_kernel's to find.)
    import torch
    want, got, st_R, st = _assign_then_accumulate(name, adjoint)
    assert torch.equal(got, want)
    assert torch.equal(st, st_R)  # K1: the stored state; K3: g stays as it is (average displacement)
    if not adjoint:
        assert torch.equal(st, _case(name)[2])


def test_two_parts_equal_one_call():
    import torch
    asm, (u, p, z, zp, xi0), xi1, g, f = _case("notched_bar")
    ref = asm.new_linsys()
    assert asm.forward_jacobian(u, p, z, zp, xi0, asm.new_state(), ref) == 0
    nn = asm.nnodes
    asm.set_gather_early_nodes(nn // 3, nn // 2)
    try:
        ls, xi = asm.new_linsys(), asm.new_state()
        assert asm.forward_jacobian(u, p, z, zp, xi0, xi, ls) == 0
        assert not torch.equal(ls.flat, ref.flat)
        assert asm.gather_finish() == 0
    finally:
        asm.set_gather_early_nodes(0, 0)
    assert torch.equal(ls.flat, ref.flat) and torch.equal(xi, xi1)


@pytest.mark.parametrize("adjoint", [False, True], ids=["K1", "K3"])
@pytest.mark.parametrize("name", ["brick222", "pinched_bricks"])
def test_repeatable(name, adjoint):
    import torch
    a, b = _assign_then_accumulate(name, adjoint), _assign_then_accumulate(name, adjoint)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("adjoint", [False, True], ids=["K1", "K3"])
@pytest.mark.parametrize("name", ["brick222", "pinched_bricks"])
def test_agrees_with_staged_wave_kernel(name, adjoint):
    # the staged one-wavefront-per-element form sums in another order and knows nothing of the image.  K1: 1e-13 relative, the
    # bound of the existing suite for this pair; K3: 1e-12, its bound for the closed form against dual numbers with elimination
    # (test_gpu_parity.py::test_adjoint_row_per_node_kernel_against_iterated_form).  Both on the states of the node kernel.
    import torch
    _, (u, p, z, zp, xi0), xi1, g, f = _case(name)
    res = []
    for kernel in ("node", "wave"):
        asm = _case(name, kernel)[0]
        ls = asm.new_linsys()
        if adjoint:
            assert asm.adjoint_jacobian(u, p, z, zp, xi0, xi1, g.clone(), f, ls) == 0
        else:
            assert asm.forward_jacobian(u, p, z, zp, xi0, asm.new_state(), ls) == 0
        res.append(ls.flat.clone())
    err = float((res[0] - res[1]).abs().max() / res[1].abs().max())
    print("%s %s node against wave: %.2e" % (name, "K3" if adjoint else "K1", err))
    assert err < (1e-12 if adjoint else 1e-13)
