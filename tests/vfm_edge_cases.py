"""TEST INFRASTRUCTURE shared by test_vfm_emul_edges.py (the kernel source and the block sums on the CPU) and
test_gpu_vfm_edges.py (k_vfm and k_vfm_reduce on the device): the element counts at which the launch of the VFM kernels can
go wrong, every parameter of the three plane-stress models in active lists of every shape, and references for every output
of V (c8_vfm_internal_power), FS (c8_vfm_forward_sens) and A (c8_vfm_adjoint_step) -- the carried sensitivities S included.

The launch rows restate what the source does with a count, read from it and quoted, not imported (as launch_cases.UNITS).

THE TABLE is count_cases() + layout_cases():
  count_cases    every count of COUNTS for the three models and every count of REDUCE_COUNTS for REDUCE_MODELS, under
                 COUNT_LAYOUT (six parameters on set 0, three in reversed order on set 1: nact = 9);
  layout_cases   every layout of layouts(model) at LAYOUT_COUNT = 21 elements (two full blocks and a tail of one).
Two element sets alternate element by element, so every block mixes the offsets of both.

REFERENCES (references(cs)): everything comes from the oracle (vfm_cases.oracle_power, oracle_adjoint_step); nothing
restates the kernels.
  xi, b, ivw     of V and FS: the oracle's local solve and residual R; ivw = w^T R within TOL of sum |w_i| |R_i|.
  h, grad        of A, marched backwards from the last step with c_n = 0.3 n and h = 0 at the start; every step is given
                 the oracle's h, so a step's error is its own.  grad within TOL of the oracle's sum of absolute terms.
  divw           at step n, for EVERY step: the oracle's adjoint march from step n down to step 1 with c = 1 at step n,
                 c = 0 below it and h = 0 at the start; the grad of its steps added up is d(w^T R_n)/dp, their sums of
                 absolute terms added up is the scale.
  S by duality   S_n = -C_xi^-1 (C_p + C_xiprev S_{n-1}) has no reference of its own in the oracle, its transpose has:
                 the march from step n down to 1 with c = 0 everywhere and h = r at the start gives, added up over its
                 steps, grad[k] = +sum r . S_n[..., k] exactly (phi_n = -C_xi^-T r, grad_n = C_p^T phi_n,
                 h_{n-1} = C_xiprev^T phi_n is the r of step n - 1).  Three independent random r [elems][points][nloc] per
                 step; the scale is sum |r| |S_n[..., k]|.  A wrong point index, a wrong column stride or a wrong slot
                 changes these sums; a sum over the mesh with a fixed weight would not see them.
  The columns of S that belong to the other set's parameters are never written and never read (asserted bitwise against
  a sentinel); they count as zero here.

THE BAR is the project's 1e-12 (BASELINE.json) of the scales above, for every figure.

MEASURED worst values over the whole table, as a multiple of the scale (every run prints them; `pytest -s`):
                                      xi        b         ivw       h         grad      divw      S (duality)
  emulator  small_hill_plane_stress   5.0e-15   2.2e-14   5.7e-16   1.3e-14   8.0e-14   7.1e-15   9.8e-15
            hyper_J2_plane_stress     8.9e-16   7.3e-13   8.3e-14   2.7e-15   2.0e-15   1.3e-13   2.2e-13
            hypo_hill_plane_stress    1.7e-13   8.0e-14   1.4e-15   3.2e-14   1.8e-14   5.6e-15   5.6e-15
  MI355X    small_hill_plane_stress   7.4e-15   2.0e-14   7.4e-16   3.5e-14   8.9e-14   1.0e-14   1.3e-14
            hyper_J2_plane_stress     8.9e-16   6.1e-13   1.2e-13   2.0e-15   4.5e-14   1.1e-13   1.5e-13
            hypo_hill_plane_stress    1.8e-13   1.2e-13   2.6e-15   1.9e-14   2.3e-14   1.2e-14   5.6e-15
The device meets the bar wherever the emulator does.  hyper_J2_plane_stress is the worst in b, divw and S on both (its b:
see REDUCE_MODELS); its divw and S are largest on the meshes of 1 to 11 elements, where a scale is a handful of products.
Two inputs were changed because a scale collapsed, each described where it is set: the virtual field (setup) and the
measured field on the long strips of the reduce edges (_folded).
"""
import collections
import functools

import numpy as np

import launch_cases as lc
import vfm_cases as vc
from meshes import fields_for, prescribed_fields
from parity import rel_vec

TOL = 1e-12  # the project's parity bar (BASELINE.json)

# ---- the launch rows --------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "kernel unit period source")
VBLOCK, NDOF = 64, 6  # c8_kernels.hip:694 `constexpr int VBLOCK = 64`; c8_element.hpp:139 `NDOF = 6` (plane-stress tri3)
# c8_kernels.hip:698 `constexpr int GPB = VBLOCK / E::NDOF` (ten lane groups of six lanes, 64 - 60 = 4 lanes idle),
# :702-703 `lb = xcd_block(blockIdx.x, nblocks); if (lb >= nblocks) return`, :722-723 `nblocks = (a.count + GPB - 1) / GPB;
# grid = ((nblocks + 7) / 8) * 8`
K_VFM = Row("k_vfm", VBLOCK // NDOF, 8, "c8_kernels.hip:698,702-703,722-723")
# c8_vfm.hip:21 `constexpr int REDUCE_THREADS = 256`, :28 `for (int b = t; b < nblocks; b += REDUCE_THREADS)`: one block of 256
# threads, thread t sums the partials of the blocks t, t + 256, ...
K_VFM_REDUCE = Row("k_vfm_reduce", 256, None, "c8_vfm.hip:21,28")
MAX_ACTIVE = 6  # c8_api.hip:247: at most six active parameters per element set under mechanics_plane_stress


def nblocks(n):
    return (n + K_VFM.unit - 1) // K_VFM.unit


def grid(n):
    return ((nblocks(n) + 7) // 8) * 8


def xcd_block(b, nb):
    """c8_kernels.hip:134-135 `chunk = (nblocks + 7) >> 3; return (b & 7) * chunk + (b >> 3)`"""
    return (b & 7) * ((nb + 7) >> 3) + (b >> 3)


COUNTS = tuple(lc.counts(K_VFM.unit, K_VFM.period))  # 1, 9, 10, 11, 79, 80, 81, 171
# in elements: 255 blocks; 256 blocks, the last holding one element; 256 full blocks; 257 blocks (thread 0 of the reduction
# takes a second block); 513 blocks (thread 0 takes three blocks, the others two)
REDUCE_COUNTS = (2550, 2551, 2560, 2561, 5121)
LAYOUT_COUNT = 21
SEQ = (0.0, 1.5, 2.0, 0.8)  # measured u_n = SEQ[n] u_1: loading, further loading, unloading

MODELS = dict(vc.MODELS)
# The two models of the reduce edges are the two Hill models.  What those counts probe -- which partials a thread of the
# reduction takes -- does not depend on the model, and hyper_J2_plane_stress leaves the comparison of b no room: its
# unknowns lambda_z and I_e are numbers near 1, the strains are 0.006 to 0.012 and the stress is E = 1000 times a strain,
# so one ulp of such an unknown (2.2e-16) is 2e-14 to 4e-14 of the stress and of R, and the oracle and the kernels, adding
# in different orders, agree in xi to about 1e-15 (a few ulp) at best.  Measured on the emulator: b at 0.4e-12 to 0.75e-12
# of max |b| at every count from 9 to 5121, the largest at 5121 (the more points, the larger the worst of them), every other
# figure of that model at 2.2e-13 or below; the Hill models have no such unknown (b below 2e-13).  Up to 171 elements all
# three models run.
REDUCE_MODELS = ("small_hill_plane_stress", "hypo_hill_plane_stress")
# every parameter of each model, in groups of at most MAX_ACTIVE
GROUPS = {"small_hill_plane_stress": ((0, 1, 2, 3, 4, 5), (6, 7, 8)),
          "hyper_J2_plane_stress": ((0, 1, 2, 3, 4, 5), (6, 7)),
          "hypo_hill_plane_stress": ((0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11), (12,))}
COUNT_LAYOUT = ((0, 1, 2, 3, 4, 5), (5, 4, 3))

Case = collections.namedtuple("Case", "model n active")


def case_id(cs):
    return "%s-%d-%s" % (cs.model, cs.n, "+".join("".join("%x" % q for q in a) or "none" for a in cs.active))


def _six(model, group):
    """the group filled up to MAX_ACTIVE parameters with the first ones that it does not hold"""
    rest = [q for q in range(len(MODELS[model])) if q not in group]
    return tuple(group) + tuple(rest[:MAX_ACTIVE - len(group)])


def layouts(model):
    """per group of parameters: (a) the group on one set and nothing on the other (the sets take turns), (b) the group on
    set 1 behind a reversed partial list on set 0 (offset != 0, order permuted), (c) six parameters on both sets (nact = 12,
    set 1 rotated by three); then no active parameter at all"""
    out = []
    for i, g in enumerate(GROUPS[model]):
        out.append((g, ()) if i % 2 == 0 else ((), g))
        out.append((tuple(reversed(g))[:(len(g) + 1) // 2], g))
        six = _six(model, g)
        out.append((six, six[3:] + six[:3]))
    out.append(((), ()))
    return out


def count_cases():
    return [Case(m, n, COUNT_LAYOUT) for m in MODELS for n in COUNTS] + \
        [Case(m, n, COUNT_LAYOUT) for m in REDUCE_MODELS for n in REDUCE_COUNTS]


def layout_cases():
    return [Case(m, LAYOUT_COUNT, lay) for m in MODELS for lay in layouts(m)]


def nact_of(cs):
    return sum(len(a) for a in cs.active)


# ---- meshes, measured steps, virtual field ------------------------------------------------------------------------------
FOLD = 64.0  # sixteen rows of cells


def _folded(c):
    """the coordinates at which prescribed_fields is evaluated.  Up to 171 elements (a strip 88 long) they are the mesh's own.
    On the strips of the reduce edges (1276 to 2564 long, and skewed: x follows y) the ramp of prescribed_fields would reach
    u_y = 15 and u_x = 0.25 while u differs by 0.05 across a cell: grad u = sum_a u_a grad N_a then carries 1 ulp(15) |grad N| =
    7e-15 of rounding against strains of 0.006 to 0.012, so any two orders of that sum differ by 1e-12 of the strain --
    measured on the emulator against the oracle at 5121 elements: xi 8.7e-13, b 2.9e-12, h 1.7e-12 (1e-15 at 171 elements).
    That is the conditioning of the input, the same for the oracle and for the kernels, and it sits at the bar.  There y is
    replaced by g(y) = FOLD / pi sin^2(pi y / FOLD), g' = sin(2 pi y / FOLD), and x by its distance from the strip's centre
    line: the same field of (x, g), strains of the same size that change sign along the strip (tension and compression,
    elastic bands between; 2341 of 5121 points yield in the first step), and |u| below 0.1.  With it the same figures are
    xi 2.9e-15, b 7.3e-15, h 5.6e-15."""
    y = c[:, 1]
    if y.max() <= 2 * FOLD:
        return c
    out = c.copy()
    out[:, 1] = FOLD / np.pi * np.sin(np.pi * y / FOLD) ** 2
    out[:, 0] = c[:, 0] - np.polyval(np.polyfit(y, c[:, 0], 1), y)  # x from the strip's centre line (the meshes are skewed)
    return out


@functools.lru_cache(maxsize=None)
def setup(model, n):
    """(coords, conn, elem_set, params [2][n], measured steps, w) on launch_cases.mesh("tri3ps", n).  The sets alternate
    element by element; set 1 has parameter 2 scaled by 1.3 (as vfm_cases).  w has the form of vfm_cases' field with
    wave numbers that make it change from node to node (cells of 0.5 x 4; a field that is smooth over a strip 2500 long
    would leave every element's w^T R_e a cancelled sum).  A first choice, (cos(1.3 x + 0.7 y) + 0.2, sin(0.9 y - 0.4 x) +
    0.1 x), was replaced: on the mesh of ONE element its gradient nearly annihilates [(dR/dxi)^T w]^T S against (dR/dp)^T w
    for hyper_J2_plane_stress, the scale of divw (one product there) collapsed and divw stood at 1.8e-12 of it on the
    emulator while S itself was within 2.2e-13; three other fields gave 0.5e-13 to 2.9e-13."""
    _, c, conn = lc.mesh("tri3ps", n)
    es = (np.arange(n) % 2).astype(np.int32)
    p1 = np.array(MODELS[model], dtype=float)
    p1[2] *= 1.3
    P = np.vstack([MODELS[model], p1])
    u1, _ = fields_for(2, *prescribed_fields(_folded(c), 0.004, ramp=True, perturb=5e-2))
    steps = [s * u1 for s in SEQ]
    x, y = c[:, 0], c[:, 1]
    w = np.ascontiguousarray(np.stack([np.cos(0.6 * y) * x + 0.2 * np.sin(y), np.sin(0.7 * y) + 0.1 * x], axis=1).ravel())
    return c, conn, es, P, steps, w


ALPHA = {"small_hill_plane_stress": 3, "hyper_J2_plane_stress": 5, "hypo_hill_plane_stress": 3}  # c8_models.hpp: alpha in xi


def plastic_points(cs):
    """(points that yield in the first step, points that do not) of the case's history"""
    a = references(cs).xi[1][:, :, ALPHA[cs.model]]
    return int((a > 0).sum()), int((a == 0).sum())


# ---- references ---------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "xi b h_in cm h_out grad gabs divw divw_abs dual")
NDUAL = 3


@functools.lru_cache(maxsize=None)
def references(cs):
    """the oracle's values for every step of the case (lists indexed by the step, entry 0 unused but xi[0]); computed
    once per case and shared -- callers must leave the arrays as they are"""
    c, conn, es, P, steps, w = setup(cs.model, cs.n)
    orc = vc.make_oracle(c, conn, cs.model, P, es, [list(a) for a in cs.active])
    nact, N = nact_of(cs), len(steps) - 1
    shape = (orc.nelems, orc.npts, orc.nloc)
    xi, b = [orc.new_state()], [None]
    for n in range(1, N + 1):
        rc, xo, bo = vc.oracle_power(orc, steps[n], steps[n - 1], xi[-1])
        assert rc == 0
        xi.append(xo)
        b.append(bo)

    def step(n, cm, h):
        ho, g, ga = vc.oracle_adjoint_step(orc, steps[n], steps[n - 1], xi[n - 1], xi[n], w, cm, h, max(nact, 1))
        return ho, g[:nact], ga[:nact]

    def march(n, cm, h):
        """from step n down to step 1, c = cm at step n and 0 below: (sum of grad, sum of the sums of absolute terms)"""
        g, ga = np.zeros(nact), np.zeros(nact)
        for m in range(n, 0, -1):
            h, gm, gam = step(m, cm if m == n else 0.0, h)
            g += gm
            ga += gam
        return g, ga

    none = [None] * (N + 1)
    h_in, cms, h_out, grad, gabs, divw, divw_abs, dual = (list(none) for _ in range(8))
    h = np.zeros(int(np.prod(shape)))
    for n in range(N, 0, -1):
        h_in[n], cms[n] = h, 0.3 * n
        h, grad[n], gabs[n] = step(n, cms[n], h)
        h_out[n] = h
    for n in range(1, N + 1):
        divw[n], divw_abs[n] = march(n, 1.0, np.zeros(int(np.prod(shape))))
        dual[n] = []
        for j in range(NDUAL):
            r = np.random.default_rng(1000 * n + j).standard_normal(shape)
            dual[n].append((r, march(n, 0.0, r.ravel().copy())[0]))
    for a in xi + b[1:] + h_in[1:] + h_out[1:]:
        a.setflags(write=False)
    return Ref(xi, b, h_in, cms, h_out, grad, gabs, divw, divw_abs, dual)


# ---- the checks that every case runs ------------------------------------------------------------------------------------
SENTINEL = -3.75  # what S, and divw / grad without active parameters, hold before a call
_SENTINEL_BITS = np.array([SENTINEL]).view(np.int64)[0]


def columns_of(cs, es):
    """[elems][nact] bool: the columns of S that belong to the element's own set"""
    nact = nact_of(cs)
    own = np.zeros((len(es), nact), dtype=bool)
    ofs = 0
    for s, a in enumerate(cs.active):
        own[np.ix_(np.flatnonzero(es == s), np.arange(ofs, ofs + len(a)))] = True
        ofs += len(a)
    return own


def owned(cs, es, S):
    """S [elems][points][nloc][nact] with the other set's columns asserted untouched (SENTINEL, bit for bit) and set to zero"""
    own = np.broadcast_to(columns_of(cs, es)[:, None, None, :], S.shape)
    assert (S.view(np.int64)[~own] == _SENTINEL_BITS).all(), "FS wrote a column of S that belongs to the other set"
    return np.where(own, S, 0.0)


def dual_errors(ref_n, So):
    """per random r: |sum r . S[..., k] - march| / sum |r| |S[..., k]|, the worst over k (0 without columns)"""
    worst = 0.0
    for r, g in ref_n:
        got = np.einsum("epj,epjk->k", r, So)
        scale = np.einsum("epj,epjk->k", np.abs(r), np.abs(So))
        if got.size:
            worst = max(worst, float((np.abs(got - g) / np.maximum(scale, 1e-300)).max()))
    return worst


class Worst(dict):
    """the largest error per figure, as a multiple of its scale"""

    def note(self, name, value):
        self[name] = max(self.get(name, 0.0), float(value))

    def __str__(self):
        return "  ".join("%s %.1e" % kv for kv in self.items())


def run_case(dut, cs, worst=None):
    """V -> FS over the steps with FS's own S carried along, then A backwards; every output against references(cs).
    dut: .V(u, up, xip, xi, b, ivw), .FS(u, up, xip, xi, S_prev, S, ivw, divw), .A(u, up, xip, xi, cm, h, grad) on host arrays,
    outputs in place (xi is given holding xi_prev: hyper_J2_plane_stress starts its local iteration from it), each
    returning the entry point's return value.  Returns the S of every step."""
    ref = references(cs)
    c, conn, es, P, steps, w = setup(cs.model, cs.n)
    nact, N = nact_of(cs), len(steps) - 1
    shape = ref.xi[0].shape
    worst = Worst() if worst is None else worst
    errs = Worst()
    S_prev, Ss = None, [None]
    for n in range(1, N + 1):
        u, up, xip, xo, bo = steps[n], steps[n - 1], ref.xi[n - 1], ref.xi[n], ref.b[n]
        wabs, ivw_ref = float(np.abs(w) @ np.abs(bo)), float(w @ bo)
        xi, b, ivw = xip.copy(), np.zeros(len(u)), np.zeros(1)
        assert dut.V(u, up, xip, xi, b, ivw) == 0
        errs.note("xi", rel_vec(xi, xo))
        errs.note("b", rel_vec(b, bo))
        errs.note("ivw", abs(ivw[0] - ivw_ref) / wabs)
        xi, ivw = xip.copy(), np.zeros(1)
        S = np.full(shape + (nact,), SENTINEL) if nact else None
        divw = np.zeros(nact) if nact else np.full(1, SENTINEL)
        assert dut.FS(u, up, xip, xi, S_prev, S, ivw, divw) == 0
        errs.note("xi", rel_vec(xi, xo))
        errs.note("ivw", abs(ivw[0] - ivw_ref) / wabs)
        if nact:
            errs.note("divw", (np.abs(divw - ref.divw[n]) / np.maximum(ref.divw_abs[n], 1e-300)).max())
            errs.note("S", dual_errors(ref.dual[n], owned(cs, es, S)))
        else:
            assert divw.view(np.int64)[0] == _SENTINEL_BITS, "FS without active parameters wrote divw"
        S_prev = S
        Ss.append(S)
    for n in range(N, 0, -1):
        h = ref.h_in[n].copy()
        grad = np.zeros(nact) if nact else np.full(1, SENTINEL)
        assert dut.A(steps[n], steps[n - 1], ref.xi[n - 1], ref.xi[n], ref.cm[n], h, grad) == 0
        errs.note("h", rel_vec(h, ref.h_out[n]))
        if nact:
            errs.note("grad", (np.abs(grad - ref.grad[n]) / np.maximum(ref.gabs[n], 1e-300)).max())
        else:
            assert grad.view(np.int64)[0] == _SENTINEL_BITS, "A without active parameters wrote grad"
    print("%s: %s" % (case_id(cs), errs))
    for k, v in errs.items():
        worst.note(k, v)
    assert all(v < TOL for v in errs.values()), (case_id(cs), dict(errs))
    return Ss
