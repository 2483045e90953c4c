"""The row-per-node kernels read and write a node's CSR rows through range-checked accesses, zero the whole row
accumulator (c8_assemble_node.hpp: row_load / row_store, zero_acc) and take what the closed form computes from the
parameters alone from a table per element set (c8_models.hpp: closed_form_constants / closed_form_c): the kernel source run
lane by lane on the CPU, where the executor has neither and the header takes the guarded accesses and forms the constants
in place.  The meshes and the second plastic step of
node_rows_rowio_cases.py, in the form for nodes with at most eight elements and in the form that takes a node's elements
eight at a time:
  1. K1 and K3 against the oracle at the suite's bar and against the emulated staged closed-form wave kernel at 1e-13 (K1,
     stored state) and 1e-12 (K3); two runs bit for bit;
  2. rows assembled onto a distinct sentinel per entry: sentinel + row with one addition, assign mode = zero-then-accumulate
     without -0, the whole range of nodes in two parts = in one;
  3. parameters changed and set back on one backend against fresh ones;
  4. against an emulator built from the kernel source BEFORE the change (tests/emul/node_rows_before_rowio/): every array of
     K1 and K3 bit for bit, on the five meshes of node_rows_xlane_cases.py, in one part and in two; and the staged
     closed-form wave kernel, another caller of Model::closed_form, bit for bit as well.
The CPU twin of test_gpu_node_rows_rowio.py, which adds what only the device has: node sub-ranges and guard bands."""
import contextlib
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import emul_lib as em
import node_rows_rowio_cases as rc
import node_rows_xlane_cases as xl
import oracle_lib as ol

TOL = 1e-12  # test_emul_parity.py
CASES = [(n, m) for n in rc.MESHES for m in (False, True)]
ROOT = os.path.dirname(em.HERE)


def _emul(name, kernel, params=None):
    c, conn, es, prm = xl.mesh(name)
    dut = em.Emul(ol.HEX8, c, conn, "small_J2", prm if params is None else params, elem_set=es)
    if kernel == "node":
        dut.node = dut.wave = True
    else:  # the staged one-wavefront-per-element kernel in its closed form
        dut.wave = dut.staged = True
    return dut


@functools.lru_cache(maxsize=None)
def _wave(name):
    return rc.forward_and_adjoint(_emul(name, "wave"), name)


@pytest.fixture(params=CASES, ids=["%s-%s" % (n, "many" if m else "lean") for n, m in CASES])
def case(request):
    name, many = request.param
    em.lib().c8emu_set_node_many(1 if many else 0)
    yield name
    em.lib().c8emu_set_node_many(0)


def test_meshes_reach_the_edges():
    rc.assert_meshes_reach_the_edges()


def test_second_step_against_oracle_and_wave(case):
    dut = _emul(case, "node")
    ls, xi, adj = rc.forward_and_adjoint(dut, case)
    rc.check_against_oracle(case, ls, xi, adj, TOL)
    rc.check_against_wave(case, ls, xi, adj, *_wave(case))
    assert rc.same_results(rc.forward_and_adjoint(dut, case), (ls, xi, adj))


@pytest.mark.parametrize("kind", rc.KINDS)
def test_rows_onto_sentinels(case, kind):
    dut = _emul(case, "node")

    def run(kind, arrays, assign, parts):
        dut.assign, dut.staged = assign, parts == "two"  # staged: the upper half of the nodes first, then the lower half
        try:
            ls = dut.new_linsys()
            for a, v in zip(rc.blocks(ls), arrays):
                a[:] = v
            return [a.copy() for a in rc.blocks(rc.assemble_onto(dut, case, kind, ls))]
        finally:
            dut.assign = dut.staged = False
    rc.check_rows_and_sentinels(case, kind, run, [])  # the emulator assembles every node: no sub-ranges here


def test_parameters_changed_and_set_back(case):
    rc.check_params_followed(case, lambda prm: _emul(case, "node", prm))


# ---- 4. against the source before the change ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emulator_before(tmp_path_factory):
    """the emulator built from this tree with the headers of tests/emul/node_rows_before_rowio/ in place of today's"""
    top = tmp_path_factory.mktemp("emul_before")
    csrc = os.path.join(ROOT, "calibr8_amd", "csrc")
    shutil.copytree(csrc, top / "calibr8_amd" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.hip", ".flags"))
    shutil.copytree(os.path.join(ROOT, "include"), top / "include")
    os.makedirs(top / "tests" / "emul")
    shutil.copy(os.path.join(em.EMUL_DIR, "c8_emul.cpp"), top / "tests" / "emul")
    shutil.copy(os.path.join(em.EMUL_DIR, "Makefile"), top / "tests" / "emul")
    shutil.copy(os.path.join(em.HERE, "math_ops.hpp"), top / "tests")
    frozen = os.path.join(em.EMUL_DIR, "node_rows_before_rowio")
    for f in sorted(os.listdir(frozen)):
        shutil.copy(os.path.join(frozen, f), top / "calibr8_amd" / "csrc")
    subprocess.check_call(["make", "-C", str(top / "tests" / "emul"), "-s"])
    before = C.CDLL(str(top / "tests" / "emul" / "libc8emul.so"))
    now = em.lib()
    before.c8emu_call.restype, before.c8emu_call.argtypes = now.c8emu_call.restype, now.c8emu_call.argtypes

    @contextlib.contextmanager
    def use(many):
        before.c8emu_set_node_many(1 if many else 0)
        em._lib = before
        try:
            yield
        finally:
            em._lib = now
            before.c8emu_set_node_many(0)
    return use


@pytest.mark.parametrize("two_parts", [False, True], ids=["one-call", "two-parts"])
@pytest.mark.parametrize("many", [False, True], ids=["lean", "many"])
@pytest.mark.parametrize("name", xl.MESHES)
def test_every_array_against_the_source_before(name, many, two_parts, emulator_before):
    """Loads and stores keep their addresses and values: A (four blocks), b_u, b_p and xi of K1, A and b of K3, bit for bit"""
    def both():
        dut = _emul(name, "node")
        dut.staged = two_parts
        return rc.forward_and_adjoint(dut, name)
    em.lib().c8emu_set_node_many(1 if many else 0)
    try:
        now = both()
    finally:
        em.lib().c8emu_set_node_many(0)
    with emulator_before(many):
        before = both()
    assert np.abs(now[0].A[0][0]).max() > 0 and np.abs(now[2].A[0][0]).max() > 0
    assert rc.same_results(now, before)


def test_other_callers_of_closed_form_against_the_source_before(emulator_before):
    """Model::closed_form is now closed_form_constants followed by closed_form_c (c8_models.hpp) and keeps its signature: the
    staged closed-form wave kernel, which calls it, on the mesh with two parameter sets, bit for bit against the emulator
    built with the model header from before the split.  (closed_form against constants + core directly would compare the
    function with itself.)"""
    name = "two_sets"
    now = rc.forward_and_adjoint(_emul(name, "wave"), name)
    with emulator_before(False):
        before = rc.forward_and_adjoint(_emul(name, "wave"), name)
    assert rc.same_results(now, before)
