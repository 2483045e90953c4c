"""The table of vfm_edge_cases.py on the CPU.  c8emu_vfm_blocks (tests/emul_vfm/c8_emul_vfm.cpp) walks the elements in the
blocks of the device launch and routes the lane sums through vfm_group_sums and vfm_block_sums (c8_assemble_vfm.hpp), the
routines that do so on the device, then sums the partials in the order of k_vfm_reduce: the slots of the active lists, the
groups past the end of the mesh and the partials of the last block are under test here without a device.  Every case
against the oracle's references at 1e-12, the block sums against the element-by-element sums of c8emu_vfm at 1e-12 of
the absolute sums, and the arithmetic of the table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vfm_edge_cases as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
V, FS, A = 0, 1, 2


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/emul_vfm/c8_emul_vfm.cpp, built afresh for this session into its own temporary directory"""
    out = str(tmp_path_factory.mktemp("c8_emul_vfm_edges"))
    so = os.path.join(out, "libc8emulvfm.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(ROOT, "tests", "emul_vfm", "c8_emul_vfm.cpp"),
                           os.path.join(ROOT, "calibr8_amd", "csrc", "c8_host.cpp")])
    L = C.CDLL(so)
    for fn in (L.c8emu_vfm, L.c8emu_vfm_blocks):
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, ip, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_double,
                       C.c_double, dp, ip, C.c_int, C.c_double, C.POINTER(dp)]
    return L


class EmuDut:
    """the interface of vfm_edge_cases.run_case on an entry of the emulator library"""

    def __init__(self, L, cs, blocks=True, max_iters=500):
        self.max_iters = max_iters
        self.fn = L.c8emu_vfm_blocks if blocks else L.c8emu_vfm
        self.model = cs.model
        self.c, self.conn, self.es, self.P, _, self.w = ve.setup(cs.model, cs.n)
        self.c = np.ascontiguousarray(self.c, dtype=np.float64)
        self.conn = np.ascontiguousarray(self.conn, dtype=np.int32)
        self.P = np.ascontiguousarray(self.P, dtype=np.float64)
        self.act = np.zeros((2, 10), dtype=np.int32)
        ofs = 0
        for s, a in enumerate(cs.active):
            self.act[s, 0], self.act[s, 1] = ofs, len(a)
            self.act[s, 2:2 + len(a)] = a
            ofs += len(a)
        self.nact = ofs

    def _call(self, what, u, up, xip, xi, b=None, S_prev=None, S=None, h=None, ivw=None, grad=None, cm=0.0):
        arrs = [u, up, xip, xi, self.w, b, S_prev, S, h, ivw, grad]
        ptrs = (dp * 11)(*[None if a is None else a.ctypes.data_as(dp) for a in arrs])
        return self.fn(what, len(self.c), len(self.conn), self.c.ctypes.data_as(dp), self.conn.ctypes.data_as(ip),
                       self.es.ctypes.data_as(ip), 2, self.model.encode(), self.max_iters, 1e-12, 1e-12, 1.0,
                       self.P.ctypes.data_as(dp), self.act.ctypes.data_as(ip), self.nact, cm, ptrs)

    def V(self, u, up, xip, xi, b, ivw):
        return self._call(V, u, up, xip, xi, b=b, ivw=ivw)

    def FS(self, u, up, xip, xi, S_prev, S, ivw, divw):
        return self._call(FS, u, up, xip, xi, S_prev=S_prev, S=S, ivw=ivw, grad=divw)

    def A(self, u, up, xip, xi, cm, h, grad):
        return self._call(A, u, up, xip, xi, h=h, grad=grad, cm=cm)


CASES = ve.count_cases() + ve.layout_cases()
WORST = {}


@pytest.mark.parametrize("cs", CASES, ids=[ve.case_id(cs) for cs in CASES])
def test_table_case_through_the_block_sums(emu, cs):
    plastic, elastic = ve.plastic_points(cs)
    if cs.n >= ve.LAYOUT_COUNT:
        assert plastic > 0 and elastic > 0, (ve.case_id(cs), plastic, elastic)
    worst = WORST.setdefault(cs.model, ve.Worst())
    Ss = ve.run_case(EmuDut(emu, cs), cs, worst)
    print("worst so far, %s: %s" % (cs.model, worst))
    if cs.n >= ve.LAYOUT_COUNT and ve.nact_of(cs):
        # the duality check has something to check: every column of S of every parameter is non-zero at every step
        es = ve.setup(cs.model, cs.n)[2]
        for S in Ss[1:]:
            assert (np.abs(ve.owned(cs, es, S)).max(axis=(0, 1, 2)) > 0).all(), ve.case_id(cs)


class Recorder:
    """runs the calls of run_case on two entries and compares their sums"""

    def __init__(self, a, b):
        self.a, self.b, self.n = a, b, 0

    def _both(self, name, args, outs, sums):
        mine = [x.copy() if isinstance(x, np.ndarray) else x for x in args]
        rc = getattr(self.a, name)(*args)
        assert getattr(self.b, name)(*mine) == rc
        for i in outs:  # per-element outputs: the same code on the same inputs
            assert args[i] is None or np.array_equal(args[i], mine[i]), (name, i)
        for i, scale in sums:
            assert (np.abs(args[i] - mine[i]) <= ve.TOL * scale).all(), (name, i, args[i], mine[i])
            self.n += 1
        return rc

    def V(self, *args):
        return self._both("V", list(args), (3, 4), [(5, self.scale_v(args))])

    def FS(self, *args):
        return self._both("FS", list(args), (3, 5), [(6, self.scale_v(args)), (7, self.scale_g)])

    def A(self, *args):
        return self._both("A", list(args), (5,), [(6, self.scale_g)])


@pytest.mark.parametrize("cs", [cs for cs in CASES if cs.n in (ve.LAYOUT_COUNT, 171, 2561)], ids=ve.case_id)
def test_block_sums_match_the_element_by_element_sums(emu, cs):
    """c8emu_vfm_blocks against c8emu_vfm, call by call: per-element outputs bit for bit, ivw within 1e-12 of sum |w_i| |R_i|,
    divw and grad within 1e-12 of the oracle's sums of absolute terms"""
    ref = ve.references(cs)
    w = ve.setup(cs.model, cs.n)[5]
    nact = ve.nact_of(cs)
    rec = Recorder(EmuDut(emu, cs, True), EmuDut(emu, cs, False))
    wabs = max(float(np.abs(w) @ np.abs(b)) for b in ref.b[1:])
    gmax = np.max([g for g in ref.gabs[1:] + ref.divw_abs[1:]], axis=0) if nact else np.zeros(1)
    rec.scale_v = lambda args: wabs
    rec.scale_g = gmax if nact else 0.0  # without active parameters both leave the sentinel
    ve.run_case(rec, cs)
    assert rec.n > 0


# ---- the arithmetic of the table ---------------------------------------------------------------------------------------
def test_rows_restate_the_launch_arithmetic():
    assert (ve.K_VFM.unit, ve.K_VFM.period) == (10, 8) and ve.VBLOCK - 10 * ve.NDOF == 4  # ten groups of six, four lanes idle
    assert ve.K_VFM_REDUCE.unit == 256
    assert ve.COUNTS == (1, 9, 10, 11, 79, 80, 81, 171)
    assert [ve.nblocks(n) for n in ve.REDUCE_COUNTS] == [255, 256, 256, 257, 513]
    assert 2551 % 10 == 1 and 2561 % 10 == 1 and 5121 % 10 == 1  # the last block holds one element
    # thread 0 of the reduction: one block up to 256 blocks, two at 257, three at 513 (the other threads two)
    turns = lambda nb, t: len(range(t, nb, ve.K_VFM_REDUCE.unit))
    assert [turns(ve.nblocks(n), 0) for n in ve.REDUCE_COUNTS] == [1, 1, 1, 2, 3]
    assert turns(255, 255) == 0 and turns(256, 255) == 1 and turns(513, 1) == 2 and turns(513, 255) == 2


@pytest.mark.parametrize("n", ve.COUNTS + ve.REDUCE_COUNTS + (ve.LAYOUT_COUNT,))
def test_every_count_is_covered_block_by_block(n):
    nb, grid = ve.nblocks(n), ve.grid(n)
    assert (nb - 1) * ve.K_VFM.unit < n <= nb * ve.K_VFM.unit and grid % 8 == 0 and nb <= grid < nb + 8
    # xcd_block over the rounded grid visits each logical block once; the blocks it sends past the end return
    lbs = [ve.xcd_block(b, nb) for b in range(grid)]
    assert sorted(lb for lb in lbs if lb < nb) == list(range(nb)) and len(set(lbs)) == grid
    # the elements of the blocks, group by group, are the mesh once; the groups past the end lie in the last block alone
    elems = [lb * ve.K_VFM.unit + g for lb in range(nb) for g in range(ve.K_VFM.unit)]
    assert [e for e in elems if e < n] == list(range(n))
    assert all(e // ve.K_VFM.unit == nb - 1 for e in elems if e >= n)


def test_the_table_holds_what_it_promises():
    cases = ve.count_cases()
    for m in ve.MODELS:
        assert {cs.n for cs in cases if cs.model == m} >= set(ve.COUNTS)
    for m in ve.REDUCE_MODELS:
        assert {cs.n for cs in cases if cs.model == m} >= set(ve.REDUCE_COUNTS)
    assert max(cs.n for cs in cases) == 5121 and ve.nblocks(ve.LAYOUT_COUNT) == 3 and ve.LAYOUT_COUNT % 10 == 1
    for m, params in ve.MODELS.items():
        lays = ve.layouts(m)
        assert sorted(q for g in ve.GROUPS[m] for q in g) == list(range(len(params)))  # every parameter of the model
        for g in ve.GROUPS[m]:
            assert len(g) <= ve.MAX_ACTIVE
            assert any(g in lay and () in lay for lay in lays)                              # (a) nothing on the other set
            assert any(lay[1] == g and 0 < len(lay[0]) <= len(g) and lay[0] == tuple(reversed(g))[:len(lay[0])] for lay in lays)  # (b)
            assert any(len(lay[0]) == len(lay[1]) == 6 and set(g) <= set(lay[0]) and lay[0] != lay[1] for lay in lays)  # (c)
        assert ((), ()) in lays
        assert all(len(a) <= ve.MAX_ACTIVE and len(set(a)) == len(a) for lay in lays for a in lay)
    assert {lay[0] == () for m in ve.MODELS for lay in ve.layouts(m) if lay != ((), ())} == {True, False}  # either set empty
