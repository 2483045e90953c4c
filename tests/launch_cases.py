"""TEST INFRASTRUCTURE shared by test_emul_launch_edges.py (the kernel bodies on the CPU) and test_gpu_launch_edges.py (the
launch wrappers of c8_kernels.hip on the device): the element and node counts at which the index arithmetic of a launch can
go wrong, meshes with exactly those counts, and the chain of checks that every case runs.

UNITS restates, row by row, what c8_kernels.hip does with a count -- read from the source and quoted, not imported from
it: a rewrite of a launch wrapper that changes a unit or a remap period has to change the row here as well, and the
arithmetic test of test_emul_launch_edges.py then shows which counts the suite runs for it."""
import collections
import functools

import numpy as np

import cauchy_cases as cc
import oracle_lib as ol
import parity_cases as pc
from meshes import brick, jiggle, jiggle_2d, tri_mesh

TOL = 1e-12  # the project's parity bar (BASELINE.json)
KINDS = ("hex8", "tet4", "tri3", "tri3ps")
FORMS = ("auto", "slot", "wave", "wave_ad", "node")  # c8.h: C8_KERNEL_AUTO .. C8_KERNEL_NODE
ELEM_TYPE = {"hex8": ol.HEX8, "tet4": ol.TET4, "tri3": ol.TRI3, "tri3ps": ol.TRI3}
# c8_kernels.hip:20 `#define C8_BLOCK 64`, :199 `#define C8_JBLOCK 64`: one wavefront per workgroup everywhere (WPB = 1)
BLOCK = 64
# c8_element.hpp:26 `NDOF = 32` (hex8), :70 `NDOF = 16` (tet4), :108 `NDOF = 9` (tri3), :139 `NDOF = 6` (tri3 under
# mechanics_plane_stress)
NDOF = {"hex8": 32, "tet4": 16, "tri3": 9, "tri3ps": 6}
CAP = 2048  # c8_kernels.hip:373, :382, :642, :678, :686 `grid = nblocks < 2048 ? nblocks : 2048`

Row = collections.namedtuple("Row", "family kind what unit period source")


def _rows():
    rows = []
    for kind in KINDS:
        # c8_kernels.hip:142 / :546 `constexpr int GPB = BLOCK / E::NDOF`, :180 / :649 `nblocks = (a.count + GPB - 1) / GPB`,
        # :181 / :650 `grid = ((nblocks + 7) / 8) * 8`, :145 / :547 `lb = xcd_block(blockIdx.x, nblocks)`; tri3 leaves
        # 64 - 7 * 9 = 1 lane idle, plane-stress tri3 64 - 10 * 6 = 4 (:148 / :550 `if (gib >= GPB) return`)
        rows.append(Row("group", kind, "K1 K2 K3 K4 K5 QoI in lane groups", BLOCK // NDOF[kind], 8,
                        "c8_kernels.hip:142,180-181,546-553,647-651"))
    # c8_kernels.hip:250-251 `nblocks = (a.count + WPB - 1) / WPB; grid = a.sa.stage ? stripe_grid(nblocks, STAGE_STRIPE)
    # : ((nblocks + 7) / 8) * 8`, :210 `lb = (sa.stage && STAGE_STRIPE) ? xcd_stripe(...) : xcd_block(...)`; K3 :288-289, :272
    rows.append(Row("wave", "hex8", "K1 K3, one wavefront per element, atomic or colored", 1, 8, "c8_kernels.hip:210,250-251,272,288-289"))
    # c8_kernels.hip:117 `#define C8_TUNE_STAGE_STRIPE 32`, :120 stripe_grid rounds to 8 * stripe = 256 blocks, :124 xcd_stripe
    # repeats every 8 * stripe blocks; K4 wave: :308 `lb = STAGE_STRIPE ? xcd_stripe(...)`, :362 `grid = stripe_grid(nblocks, STAGE_STRIPE)`
    rows.append(Row("wave_stripe", "hex8", "K1 K3 staged (gather), K4 wave", 1, 8 * 32, "c8_kernels.hip:117-125,210,251,289,308,362"))
    # c8_kernels.hip:421-424 `EPB = (BLOCK / 64) * 8; nblocks = (a.count + EPB - 1) / EPB; grid = ((nblocks + 7) / 8) * 8`, :409
    # xcd_block, :414-418 `e0 = (lb * WPB + wib) * 8 ... (count - e0 < 8) ? count - e0 : 8`
    rows.append(Row("wave8_k2", "hex8", "K2 k_residual_wave, eight elements per wavefront", 8, 8, "c8_kernels.hip:409-424"))
    # c8_kernels.hip:346-350 K4 closed `gidx * 8 >= count ... (count - gidx * 8 < 8) ? ...`, :355-356 `ngroups = (a.count + 7) / 8`
    # (no remap); K5 wave / closed :334-336, :371-373, :380-382; QoI wave :632-634, :640-642
    rows.append(Row("wave8", "hex8", "K4 closed, K5 wave / closed, QoI wave, eight elements per wavefront", 8, None,
                    "c8_kernels.hip:334-336,346-356,371-373,380-382,632-642"))
    # c8_kernels.hip:476 `#define C8_TUNE_NODE_STRIPE 256`, :519-520 `nblocks = count; grid = stripe_grid(nblocks, NODE_STRIPE)`,
    # :484-485 `lb = xcd_stripe(blockIdx.x, NODE_STRIPE); if (lb >= count) return`: one NODE per block, 8 * 256 = 2048 blocks
    rows.append(Row("node", "hex8", "K1 K3 row per node (counts are NODES)", 1, 8 * 256, "c8_kernels.hip:476-500,519-520"))
    return rows


UNITS = _rows()


def row(family, kind):
    return next(r for r in UNITS if r.family == family and r.kind == kind)


def counts(unit, period):
    """1; unit - 1, unit, unit + 1; period unit - 1, period unit, period unit + 1; two periods, a full unit and one more
    (a partly filled last unit in a partly filled third period); zeros and duplicates dropped"""
    out = [1]
    if unit > 1:
        out += [unit - 1, unit, unit + 1]
    if period:
        out += [period * unit - 1, period * unit, period * unit + 1, 2 * period * unit + unit + 1]
    else:
        out += [2 * unit + 1]
    return sorted({n for n in out if n > 0})


def above_cap(kind, eight_per_wave=False):
    """K5 and the QoI kernels: a count just above CAP full blocks, where the grid-stride loop takes its first second turn and
    the last unit is partly filled: CAP * unit + 3 for the lane groups (hex8, two per block: one full block and one element
    more), CAP * 8 + 7 for the groups of eight"""
    unit = 8 if eight_per_wave else BLOCK // NDOF[kind]
    return CAP * unit + (7 if eight_per_wave else 3)


# ---- models: one with a closed form and one automatically differentiated per element type; parameters and strain
# amplitudes of parity_cases.py.  The closed form is small_J2's (c8_models.hpp: HAS_CLOSED_FORM); plane-stress tri3 has none.
MODELS = {"hex8": [("small_J2", pc.J2, 0.004), ("hyper_J2", pc.HJ2, 0.004)],
          "tet4": [("small_J2", pc.J2, 0.004), ("hyper_J2", pc.HJ2, 0.004)],
          "tri3": [("small_J2", pc.J2, 0.004), ("hyper_J2_plane_strain", pc.HJ2_PS, 0.004)],
          "tri3ps": [("hyper_J2_plane_stress", pc.HJ2_PSS, 0.004)]}
HOSFORD = ("small_hosford", pc.HOSFORD, 0.004)  # with pc.LOCAL_LINE_SEARCH
CLOSED_FORM = ("small_J2",)

# (form, kind) pairs that c8_set_kernel_variant refuses (c8_api.hip:324-327): the wave-per-element and the row-per-node
# kernels exist for hex8 only; on hex8 the row-per-node kernel needs a model with a closed form (CLOSED_FORM)
UNSUPPORTED = {(f, k) for f in ("wave", "wave_ad", "node") for k in ("tet4", "tri3", "tri3ps")}
# scatter modes a kind accepts: the staged assembly is built for 3-D elements (c8_api.hip:265)
SCATTERS = {"hex8": ("atomic", "gather"), "tet4": ("atomic", "gather"), "tri3": ("atomic",), "tri3ps": ("atomic",)}
# hex8 `slot` under `gather`: K1 stages, K3 is refused at the call (c8_api.hip:510-511) -- the chain cannot run
CHAIN_REFUSED = {("slot", "hex8", "gather")}


# ---- meshes with an exact element count -------------------------------------------------------------------------------
SKEW = np.array([[1.0, 0.1, 0.12], [0.2, 1.0, 0.15], [0.1, 0.08, 1.0]])


def _skew(c):
    """the linear map SKEW of the coordinates (z stays 0 in the plane).  A tet or a triangle cut out of a grid has nodes
    whose shape function does not change along one of the axes; under finite deformation, or with a node moved at random
    nearly back onto the axis, the rows of A01 that belong to them are small sums of cancelling terms, which the row-wise
    metric of parity.py cannot judge (tet4 hyper_J2: 2.4e-12 of such a row on the device AND on the emulator, every other
    row at 1e-15).  After the map every component of every gradient is at least a tenth of the largest."""
    out = np.asarray(c) @ SKEW.T
    if not np.asarray(c)[:, 2].any():
        out[:, 2] = 0.0
    return np.ascontiguousarray(out)


def _y_fastest(conn, nx, ny, nz, per_cell=1):
    """the elements of a brick (x fastest, then y, then z; per_cell consecutive elements per cell) in the order y fastest,
    then x, then z: the first few of them are a column along y, the direction of the strain ramp of prescribed_fields, so
    that already a cut of two elements holds elastic and plastic points; later ones give nodes with one to eight elements"""
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    order = np.lexsort((j.ravel(), i.ravel(), k.ravel()))  # by k, then i, then j
    cells = np.arange(nx * ny * nz * per_cell).reshape(-1, per_cell)
    return np.ascontiguousarray(np.asarray(conn)[cells[order].ravel()])


@functools.lru_cache(maxsize=None)
def mesh(kind, n, cut=False):
    """(elem_type, coords, conn) with exactly n elements, each advancing along y.  hex8: a row of n elements with every node
    moved (cut=False), or the first n elements of a 3 x 3 x k brick taken in columns along y (cut=True: nodes with 1 to 8 elements);
    tet4: the first n tets of a 2 x 2 x k brick cut into tets, in columns along y; tri3: the first n triangles of a strip four cells
    wide"""
    if kind == "hex8" and not cut:
        c, conn, _ = brick(1, n, 1, 0.8, 0.25 * n, 0.7)
        c = jiggle(c, {}, 0.04)  # no node set: every node moves (a row of elements has no interior node)
    elif kind == "hex8":
        nz = (n + 8) // 9
        # cells of 1 x 4 x 0.5: long along y, so that the shear of the ramp (x d eps / dy) stays below the stretch, and large,
        # because the perturbation of prescribed_fields is an absolute displacement (strains of 1e-4 here)
        c, conn, sets = brick(3, 3, nz, 3.0, 12.0, 0.5 * nz)
        c, conn = cc.sub_mesh(jiggle(c, sets, 0.1), _y_fastest(conn, 3, 3, nz), n)
    elif kind == "tet4":
        nz = (n + 23) // 24
        c, conn = cc.tet_mesh(2, 2, nz)
        c[:, 2] *= 0.5 * nz
        c = _skew(c)
        assert (np.linalg.det(c[conn[:, 1:]] - c[conn[:, :1]]) > 0).all()
        c, conn = cc.sub_mesh(c, _y_fastest(conn, 2, 2, nz, per_cell=6), n)
    else:
        ny = (n + 7) // 8
        c, conn, sets = tri_mesh(4, ny, 2.0, 4.0 * ny)  # cells of 0.5 x 4, for the reasons given above
        c = _skew(jiggle_2d(c, sets, 0.01))
        c[:, :2] = c[:, :2].max(axis=0) - c[:, :2]  # a half turn: the centroid of the first triangle lies in the upper part of its cell
        c, conn = cc.sub_mesh(c, conn, n)
    assert len(conn) == n and len(np.unique(conn)) == len(c)
    c[:, 1] -= c[:, 1].min()  # the ramp of prescribed_fields starts at y = 0
    return ELEM_TYPE[kind], c, conn


@functools.lru_cache(maxsize=None)
def node_mesh(nnodes):
    """hex8 meshes with exactly 2047, 2048 and 2049 nodes around the 2048-block period of the row-per-node launch: the
    15 x 15 x 7 brick has 16 * 16 * 8 = 2048, without its last (corner) element 2047; 2049 = a cut of a 6 x 6 x 42 brick
    (NODES_2049: counted, and asserted here)"""
    if nnodes in (2047, 2048):
        c, conn, sets = brick(15, 15, 7, 1.0, 0.8, 0.7)
        c = jiggle(c, sets, 0.01)
        if nnodes == 2047:
            c, conn = cc.sub_mesh(c, conn, len(conn) - 1)
    else:
        dims, n = NODES_2049
        c, conn, sets = brick(*dims, 1.0, 0.8, 2.0)
        c, conn = cc.sub_mesh(jiggle(c, sets, 0.01), conn, n)
    assert len(c) == nnodes and len(np.unique(conn)) == nnodes, (nnodes, len(c))
    return ol.HEX8, c, conn


NODES_2049 = ((6, 6, 42), 1468)  # found by counting the nodes of every cut of small bricks (node_mesh asserts it)
NODE_COUNTS = (2047, 2048, 2049)


# ---- the case table -------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "family kind form scatter model params eps n cut")


def case_id(cs):
    return "%s-%s-%s-%s-%s-%d%s" % (cs.family, cs.kind, cs.form, cs.scatter, cs.model, cs.n, "c" if cs.cut else "")


def _hex8_families(form, scatter, model):
    """the rows of UNITS that a (form, scatter, model) chain on hex8 reaches (c8_api.hip:576, :595, :621, :635-639, :649-652,
    :516-518): every count of every one of them is a case"""
    closed = model in CLOSED_FORM and form in ("auto", "node")
    if form == "slot":
        return ["group"]
    fam = ["wave8_k2", "wave8"]                      # K2 eight per wavefront; K5 / QoI (and K4 closed) eight per wavefront
    if closed and scatter == "gather":
        fam.append("node")                           # K1 / K3 row per node, K4 / K5 closed
    else:
        fam.append("wave_stripe" if scatter == "gather" else "wave")  # K1 / K3
        if not closed:
            fam.append("wave_stripe")                # K4 wave
    return fam


def chain_cases():
    """every (family, kind, form, scatter, model, count) that runs the chain K1, K2, K3, K4, K5, QoI against the oracle"""
    out = []
    for kind in KINDS:
        for form in FORMS:
            if (form, kind) in UNSUPPORTED:
                continue
            for scatter in SCATTERS[kind]:
                if (form, kind, scatter) in CHAIN_REFUSED:
                    continue
                if form == "node" and scatter != "gather":  # c8_api.hip:514-515: C8_KERNEL_NODE needs C8_SCATTER_GATHER
                    continue
                for model, params, eps in MODELS[kind]:
                    if form == "node" and model not in CLOSED_FORM:
                        continue
                    # wave_ad differs from wave only where the model has a closed form (c8_api.hip:332: the flag it clears
                    # is read by the closed-form instantiations alone): the other models run the identical kernels as `wave`
                    if form == "wave_ad" and model not in CLOSED_FORM:
                        continue
                    fams = ["group"] if kind != "hex8" else _hex8_families(form, scatter, model)
                    seen = set()
                    for fam in fams:
                        r = row(fam, kind)
                        if fam == "node":
                            # element counts of small cut meshes (nodes with 1 to 8 elements; the groups of eight of K4 / K5
                            # closed), then the three node counts around the period
                            # `auto` on a model with a closed form IS the row-per-node launch under `gather` (c8_api.hip:397-398,
                            # :516-518): it runs the small meshes and the node count past the period, `node` all three
                            ns = [(n, True) for n in counts(8, None) + [27]] + \
                                [(-nn, False) for nn in (NODE_COUNTS if form == "node" else NODE_COUNTS[-1:])]
                        else:
                            ns = [(n, False) for n in counts(r.unit, r.period)]
                            if kind == "hex8":  # the cut brick as well at unit + 1 and period unit + 1
                                ns += [(r.unit + 1, True)] + ([(r.period * r.unit + 1, True)] if r.period else [])
                        for n, cut in ns:
                            if (n, cut) not in seen:
                                seen.add((n, cut))
                                out.append(Case(fam, kind, form, scatter, model, tuple(params), eps, n, cut))
    return out


def colored_cases():
    """`colored` at two counts per element type (its per-colour launches are ragged already): unit + 1 and period unit + 1 of
    the lane groups, and of the wave kernels on hex8"""
    out = []
    for kind in KINDS:
        model, params, eps = MODELS[kind][0]
        r = row("group", kind)
        form = "slot" if kind == "hex8" else "auto"
        for n in (r.unit + 1, r.period * r.unit + 1):
            out.append(Case("group", kind, form, "colored", model, tuple(params), eps, n, kind == "hex8"))
    for n in (2, 9):
        out.append(Case("wave", "hex8", "wave", "colored", "hyper_J2", tuple(pc.HJ2), 0.004, n, True))
    return out


def hosford_cases():
    """small_hosford with the local line search on the hex8 wave kernels and the tet4 lane groups: 1, unit - 1 and unit + 1 of
    the units that its kernels have (hex8: the groups of eight of K2 / K5; tet4: four elements per block)"""
    out = []
    for kind, fam, form in (("hex8", "wave8", "wave"), ("tet4", "group", "auto")):
        u = row(fam, kind).unit
        for n in sorted({1, u - 1, u + 1}):
            out.append(Case(fam, kind, form, "atomic", HOSFORD[0], tuple(HOSFORD[1]), HOSFORD[2], n, False))
    return out


def mesh_of_case(cs):
    if cs.n < 0:
        return node_mesh(-cs.n)
    return mesh(cs.kind, cs.n, cs.cut)


def oracle_of(cs):
    et, c, conn = mesh_of_case(cs)
    orc = ol.Oracle(et, c, conn, cs.model, list(cs.params))
    if cs.model == HOSFORD[0]:
        orc.set_local_line_search(*pc.LOCAL_LINE_SEARCH)
    return orc, c, conn


def branches(orc, c, cs):
    """(plastic points, elastic points) of the second step of the history that run_chain uses"""
    xi = pc.two_steps(orc, c, cs.eps)[2][2]
    a = xi[:, :, -1]  # alpha is the last local unknown of every model of this table
    return int((a > 0).sum()), int((a == 0).sum())


def run_chain(orc, dut, c, model, eps, tol=TOL):
    """K1, K2, and K3 -> K4 -> K5 -> QoI against the oracle: the project's checks, unchanged, at the project's bar"""
    pc.check_forward(orc, dut, c, model, eps, tol)
    pc.check_residual(orc, dut, c, eps, tol)
    pc.check_adjoint_chain(orc, dut, c, model, eps, tol)


def two_set_cases():
    """two interleaved element sets with different parameters and active lists at unit + 1 and 8 unit + 1: a group of eight
    (or a block of lane groups) straddles a set boundary at the tail"""
    out = []
    for kind, fam, form in (("hex8", "wave8", "wave"), ("hex8", "group", "slot"), ("tet4", "group", "auto")):
        u = row(fam, kind).unit
        out += [(kind, form, n) for n in (u + 1, 8 * u + 1)]
    return out


TWO_SET_PARAMS = [[1000.0, 0.25, 100.0, 2.0, 0.0, 0.0], [700.0, 0.3, 50.0, 1.2, 1e-4, 5.0]]  # of parity_cases.check_two_element_sets
TWO_SET_ACTIVE = ([0, 3], [1, 2, 3])


def check_two_sets(factory, kind, n, tol=TOL):
    """parity_cases.check_two_element_sets on a mesh of exactly n elements, sets alternating irregularly"""
    et, c, conn = mesh(kind, n, kind == "hex8")
    es = (np.random.default_rng(21).random(n) < 0.4).astype(np.int32)
    es[-1], es[-2] = 1, 0  # the last two elements (one group of eight, one block) lie in different sets
    orc = ol.Oracle(et, c, conn, "small_J2", TWO_SET_PARAMS, elem_set=es)
    dut = factory(et, c, conn, "small_J2", TWO_SET_PARAMS, elem_set=es)
    st = pc.two_steps(orc, c, 0.004)
    (u, p, xi), (up, pp, xip) = st[2], st[1]
    ls_o, ls_d, xo, xd = orc.new_linsys(), dut.new_linsys(), orc.new_state(), dut.new_state()
    assert orc.forward_jacobian(u, p, up, pp, xip, xo, ls_o) == 0
    assert dut.forward_jacobian(u, p, up, pp, xip, xd, ls_d) == 0
    errs = pc.compare_systems(orc, ls_d, ls_o)
    errs["xi"] = pc.rel_vec(xd, xo)
    assert max(errs.values()) < tol, errs
    for b in (orc, dut):
        b.set_active(0, TWO_SET_ACTIVE[0])
        b.set_active(1, TWO_SET_ACTIVE[1])
    g = np.zeros((orc.nelems, orc.npts, orc.nloc))
    f = np.zeros((orc.nelems, orc.npts, orc.ndofs))
    orc.adjoint_jacobian(u, p, up, pp, xip, xi, g, f, orc.new_linsys())
    rng = np.random.default_rng(22)
    z_u, z_p = rng.standard_normal(len(u)) * 1e-3, rng.standard_normal(len(p)) * 1e-3
    phi, g_d, f_d, phi_d = np.zeros_like(g), g.copy(), f.copy(), np.zeros_like(g)
    orc.solve_adjoint_local(u, p, up, pp, xip, xi, z_u, z_p, phi, g, f)
    assert dut.solve_adjoint_local(u, p, up, pp, xip, xi, z_u, z_p, phi_d, g_d, f_d) == 0
    assert pc.rel_vec(phi_d, phi) < tol and pc.rel_vec(g_d, g) < tol and np.abs(f_d - f).max() <= tol * max(1.0, np.abs(f).max())
    gr_o, gr_scale = orc.qoi_gradient_with_scale(u, p, up, pp, xip, xi, z_u, z_p, phi, 5)
    gr_d = dut.qoi_gradient(u, p, up, pp, xip, xi, z_u, z_p, phi, 5)
    assert np.abs(gr_o).min() > 0 and (np.abs(gr_d - gr_o) / np.maximum(gr_scale, 1e-300)).max() < tol, (gr_d, gr_o, gr_scale)
