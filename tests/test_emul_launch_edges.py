"""The case table of launch_cases.py on the CPU: its arithmetic, and every case through the kernel source run by the lane
emulator (tests/emul) against the oracle.  The emulator has loops of its own in place of the launch wrappers of
c8_kernels.hip, so what this file checks of the kernels is their bodies at the ragged ends of the table -- groups of eight
hex8 elements that hold fewer than eight (`..._wave8(..., n)`, n < 8), element counts that leave lane groups of a tri3 block
without an element -- and that every mesh and state of the table is sound (the oracle solves it, both branches of the model
run) before test_gpu_launch_edges.py takes the same table to the device."""
import numpy as np
import pytest

import emul_lib as em
import launch_cases as lc
import parity_cases as pc


def emul_config(cs):
    """the emulator's switches for a (form, scatter, model) of the table, or None where the emulator has no such form:
    (wave, closed, staged, node)"""
    gather = cs.scatter == "gather"
    closed_model = cs.model in lc.CLOSED_FORM
    if cs.form == "slot":
        return (False, False, gather, False)  # an explicit C8_KERNEL_SLOT iterates
    if cs.kind != "hex8":
        return (False, True, gather, False)   # auto: the closed form where the model has one
    if cs.form == "node" or (cs.form == "auto" and gather and closed_model):
        return (True, True, False, True)      # K1 / K3 row per node, K4 / K5 in closed form
    if cs.form in ("auto", "wave"):
        return (True, True, gather, False)
    if cs.form == "wave_ad":
        return (True, False, gather, False)
    return None


def make_emul(cs, et, c, conn):
    wave, closed, staged, node = emul_config(cs)
    dut = em.Emul(et, c, conn, cs.model, list(cs.params))
    dut.wave, dut.closed, dut.staged, dut.node = wave, closed, staged, node
    if cs.model == lc.HOSFORD[0]:
        dut.set_local_line_search(*pc.LOCAL_LINE_SEARCH)
    return dut


def _emul_cases():
    """the table, one case per distinct emulator run (the emulator has neither colours nor a block remap: cases that differ
    only in those are one run here)"""
    seen, out = set(), []
    for cs in lc.chain_cases() + lc.colored_cases() + lc.hosford_cases():
        key = (cs.kind, cs.model, cs.n, cs.cut, emul_config(cs))
        if key not in seen:
            seen.add(key)
            out.append(cs)
    return out


EMUL_CASES = _emul_cases()


@pytest.mark.parametrize("cs", EMUL_CASES, ids=[lc.case_id(cs) for cs in EMUL_CASES])
def test_table_case_through_the_emulator(cs):
    assert emul_config(cs) is not None
    orc, c, conn = lc.oracle_of(cs)
    assert orc.nelems == (cs.n if cs.n > 0 else orc.nelems) and (cs.n > 0 or orc.nnodes == -cs.n)
    plastic, elastic = lc.branches(orc, c, cs)
    if orc.nelems * orc.npts > 8:
        assert plastic > 0 and elastic > 0, (lc.case_id(cs), plastic, elastic)
    lc.run_chain(orc, make_emul(cs, orc.elem_type, c, conn), c, cs.model, cs.eps)


@pytest.mark.parametrize("kind,form,n", lc.two_set_cases(), ids=["%s-%s-%d" % t for t in lc.two_set_cases()])
def test_two_element_sets_at_a_ragged_tail(kind, form, n):
    def factory(et, c, conn, model, params, **kw):
        dut = em.Emul(et, c, conn, model, params, **kw)
        dut.wave = form == "wave"
        dut.closed = form != "slot"
        return dut
    lc.check_two_sets(factory, kind, n)


# ---- the arithmetic of the table ---------------------------------------------------------------------------------------
def test_units_restate_the_launch_arithmetic():
    """the rows as read from c8_kernels.hip, written out once more as numbers: a change of launch_cases.UNITS shows here"""
    got = {(r.family, r.kind): (r.unit, r.period) for r in lc.UNITS}
    assert got == {("group", "hex8"): (2, 8), ("group", "tet4"): (4, 8), ("group", "tri3"): (7, 8), ("group", "tri3ps"): (10, 8),
                   ("wave", "hex8"): (1, 8), ("wave_stripe", "hex8"): (1, 256), ("wave8_k2", "hex8"): (8, 8),
                   ("wave8", "hex8"): (8, None), ("node", "hex8"): (1, 2048)}
    assert lc.BLOCK - 7 * lc.NDOF["tri3"] == 1 and lc.BLOCK - 10 * lc.NDOF["tri3ps"] == 4  # the idle lanes of the tri3 blocks
    # the counts above the cap of 2048 blocks, as the loop's first wrap with a partly filled last unit
    assert [lc.above_cap("hex8", True), lc.above_cap("hex8"), lc.above_cap("tet4"), lc.above_cap("tri3"), lc.above_cap("tri3ps")] == \
        [16391, 4099, 8195, 14339, 20483]
    for kind in lc.KINDS:
        u = lc.BLOCK // lc.NDOF[kind]
        n = lc.above_cap(kind)
        assert (n + u - 1) // u > lc.CAP and n % u != 0 and n < (lc.CAP + 2) * u  # wraps, with a partly filled last block, at once
    n = lc.above_cap("hex8", True)
    assert (n + 7) // 8 > lc.CAP and n % 8 != 0 and n < (lc.CAP + 1) * 8


@pytest.mark.parametrize("r", lc.UNITS, ids=["%s-%s" % (r.family, r.kind) for r in lc.UNITS])
def test_counts_hold_every_edge_of_a_row(r):
    ns = lc.counts(r.unit, r.period)
    assert ns == sorted(set(ns)) and min(ns) == 1
    if r.unit > 1:
        assert {r.unit - 1, r.unit, r.unit + 1} <= set(ns)
    if r.period:
        edge = r.period * r.unit
        assert {edge - 1, edge, edge + 1} <= set(ns)
        tail = [n for n in ns if n > 2 * edge]
        assert len(tail) == 1 and tail[0] < 3 * edge and (tail[0] % r.unit != 0 or r.unit == 1) and tail[0] % edge != 0
    else:
        assert any(n > 2 * r.unit and n % r.unit for n in ns)
    # ... and the table runs every one of them for every form and scatter mode that reaches the row
    cases = [cs for cs in lc.chain_cases() if cs.family == r.family and cs.kind == r.kind]
    assert cases
    if r.family == "node":
        for fs in {(cs.form, cs.scatter, cs.model) for cs in cases}:
            want = lc.NODE_COUNTS if fs[0] == "node" else lc.NODE_COUNTS[-1:]  # `auto` resolves to the same launch
            assert {-n for n in want} <= {cs.n for cs in cases if (cs.form, cs.scatter, cs.model) == fs}
        assert any(cs.form == "node" for cs in cases) and lc.NODE_COUNTS == (edge - 1, edge, edge + 1)
        return
    reached = {(cs.form, cs.scatter, cs.model) for cs in lc.chain_cases() if cs.kind == r.kind and
               (r.kind != "hex8" or r.family in lc._hex8_families(cs.form, cs.scatter, cs.model))}
    for fs in reached:
        # a count may stand under another row of the same (form, scatter, model): the chain runs every kernel of the form
        have = {cs.n for cs in lc.chain_cases() if cs.kind == r.kind and (cs.form, cs.scatter, cs.model) == fs and not cs.cut}
        assert set(ns) <= have, (fs, sorted(set(ns) - have))


def test_no_form_of_an_element_type_is_left_out():
    """every (form, element type) pair is either run by the table, with every scatter mode the element type accepts and
    with a closed-form and an automatically differentiated model where the form takes both, or listed as refused;
    test_gpu_launch_edges.py asserts that the library refuses exactly the listed ones"""
    cases = lc.chain_cases()
    for kind in lc.KINDS:
        for form in lc.FORMS:
            mine = [cs for cs in cases if cs.kind == kind and cs.form == form]
            if (form, kind) in lc.UNSUPPORTED:
                assert not mine
                continue
            assert mine, (form, kind)
            scatters = {s for s in lc.SCATTERS[kind] if (form, kind, s) not in lc.CHAIN_REFUSED and (form != "node" or s == "gather")}
            assert {cs.scatter for cs in mine} == scatters, (form, kind)
            models = {m for m, _, _ in lc.MODELS[kind] if form not in ("node", "wave_ad") or m in lc.CLOSED_FORM}
            assert {cs.model for cs in mine} == models, (form, kind)
    assert lc.UNSUPPORTED == {(f, k) for f in ("wave", "wave_ad", "node") for k in ("tet4", "tri3", "tri3ps")}
    assert lc.CHAIN_REFUSED == {("slot", "hex8", "gather")}
    # the families named by the issue: colours at two counts per element type, the line-search model at 1, unit - 1, unit + 1
    col = lc.colored_cases()
    assert all(sum(1 for cs in col if cs.kind == k) >= 2 for k in lc.KINDS)
    hos = lc.hosford_cases()
    assert sorted(cs.n for cs in hos if cs.kind == "hex8") == [1, 7, 9] and sorted(cs.n for cs in hos if cs.kind == "tet4") == [1, 3, 5]
    assert all(emul_config(cs) is not None for cs in cases + col + hos)


def test_meshes_have_the_counts_they_are_asked_for():
    for kind in lc.KINDS:
        for n in lc.counts(lc.row("group", kind).unit, 8):
            et, c, conn = lc.mesh(kind, n)
            assert len(conn) == n and et == lc.ELEM_TYPE[kind]
    # the cut brick has nodes with one to eight elements
    _, c, conn = lc.mesh("hex8", 65, True)
    assert set(np.bincount(conn.ravel())) >= {1, 2, 4, 8}
    for nn in lc.NODE_COUNTS:
        assert len(lc.node_mesh(nn)[1]) == nn
