"""`-m gpu`: K1-K5 and the point-QoI kernels at the edges of their launches (launch_cases.py), through the launch wrappers of
c8_kernels.hip that only the device runs: the rounding of a grid to 8 blocks with the xcd_block remap, the stripes of 32 and
256 blocks, the `first` offsets and `mt.order`, the cap of 2048 blocks with its grid-stride loop.
  (a) every case of the table against the oracle, at the project's bar;
  (b) every array between guard words, at an address that is 8- but not 16-byte aligned, inputs compared bit for bit after
      every call;
  (c) K5 and the objective above the cap of 2048 blocks, against the oracle;
  (d) c8_assemble_forward_jacobian_subset against the oracle on the listed elements alone.
test_emul_launch_edges.py runs the same table on the CPU and holds the arithmetic tests of the table."""
import functools

import numpy as np
import pytest

import cauchy_cases as cc
import launch_cases as lc
import oracle_lib as ol
import parity_cases as pc
from parity import rel_vec

pytestmark = pytest.mark.gpu
TOL = lc.TOL


def device(form, scatter, guarded=False):
    """factory of a device backend with the kernel form set through c8_set_kernel_variant itself (GpuBackend passes over
    `wave` on other elements than hex8; here a refusal is an error)"""
    def make(et, c, conn, model, params, **kw):
        from gpu_backend import GpuBackend
        if model == lc.HOSFORD[0]:
            kw.setdefault("line_search", pc.LOCAL_LINE_SEARCH)
        be = (guarded_backend() if guarded else GpuBackend)(et, c, conn, model, params, scatter=scatter, **kw)
        be.asm.set_kernel(form)
        return be
    return make


# ---- (a) counts around every edge ----------------------------------------------------------------------------------------
CHAIN = lc.chain_cases() + lc.colored_cases() + lc.hosford_cases()


@pytest.mark.parametrize("cs", CHAIN, ids=[lc.case_id(cs) for cs in CHAIN])
def test_chain_at_the_count(cs):
    orc, c, conn = lc.oracle_of(cs)
    dut = device(cs.form, cs.scatter)(orc.elem_type, c, conn, cs.model, list(cs.params))
    assert dut.nelems == orc.nelems and dut.nnodes == orc.nnodes and dut.asm.scatter == cs.scatter
    lc.run_chain(orc, dut, c, cs.model, cs.eps)


@pytest.mark.parametrize("scatter", ["atomic", "gather"])
@pytest.mark.parametrize("kind,form,n", lc.two_set_cases(), ids=["%s-%s-%d" % t for t in lc.two_set_cases()])
def test_two_element_sets_at_a_ragged_tail(kind, form, n, scatter):
    lc.check_two_sets(device(form, scatter), kind, n)


def test_the_library_refuses_what_the_table_lists_as_refused_and_nothing_else():
    from calibr8_amd import Assembler, C8Error, lib
    for kind in lc.KINDS:
        et, c, conn = lc.mesh(kind, lc.row("group", kind).unit + 1)
        for model, params, _ in lc.MODELS[kind]:
            for form in lc.FORMS:
                asm = Assembler(et, c, conn, model, params)
                if (form, kind) in lc.UNSUPPORTED or (form == "node" and model not in lc.CLOSED_FORM):
                    with pytest.raises(C8Error) as ei:
                        asm.set_kernel(form)
                    assert ei.value.code == lib.C8_ERR_UNSUPPORTED, (form, kind, model)
                else:
                    asm.set_kernel(form)
            for scatter in ("atomic", "colored", "gather"):
                asm = Assembler(et, c, conn, model, params)
                if scatter in lc.SCATTERS[kind] + ("colored",):
                    asm.set_scatter(scatter)
                else:
                    with pytest.raises(C8Error) as ei:
                        asm.set_scatter(scatter)
                    assert ei.value.code == lib.C8_ERR_UNSUPPORTED, (scatter, kind)
    # the chain that the table leaves out on hex8: slot-per-lane kernels under the staged assembly stop at K3
    assert lc.CHAIN_REFUSED == {("slot", "hex8", "gather")}
    et, c, conn = lc.mesh("hex8", 3)
    gs = device("slot", "gather")(et, c, conn, "small_J2", pc.J2)
    u, p = np.zeros(3 * len(c)), np.zeros(len(c))
    assert gs.forward_jacobian(u, p, u, p, gs.new_state(), gs.new_state(), gs.new_linsys()) == 0
    with pytest.raises(C8Error, match="wave-per-element") as ei:
        gs.adjoint_jacobian(u, p, u, p, gs.new_state(), gs.new_state(), np.zeros((gs.nelems, gs.npts, gs.nloc)),
                            np.zeros((gs.nelems, gs.npts, 4 * gs.nn)), gs.new_linsys())
    assert ei.value.code == lib.C8_ERR_UNSUPPORTED
    # the row-per-node form under another scatter mode is refused at the call
    gn = device("node", "atomic")(et, c, conn, "small_J2", pc.J2)
    with pytest.raises(C8Error, match="C8_KERNEL_NODE"):
        gn.forward_jacobian(u, p, u, p, gn.new_state(), gn.new_state(), gn.new_linsys())


# ---- (b) guard bands and untouched inputs ----------------------------------------------------------------------------------
GUARD = -7.25
_GUARD_BITS = np.array([GUARD]).view(np.int64)[0]


class Guarded:
    """a host array on the device as the slice [1 : n + 1] of its own buffer of n + 3 doubles filled with GUARD"""

    def __init__(self, asm, name, host):
        import torch
        h = np.ascontiguousarray(host, dtype=np.float64)
        self.name, self.shape, self.n = name, h.shape, h.size
        self.buf = torch.full((self.n + 3,), GUARD, dtype=torch.float64, device=asm.device)
        self.t = self.buf[1:self.n + 1]
        assert self.t.data_ptr() % 16 == 8 and self.t.is_contiguous() and self.t.numel() == self.n
        self.sent = h.reshape(-1).copy()
        self.t.copy_(torch.from_numpy(self.sent))

    def check(self, is_input):
        """after the call: the guard words bitwise, an input bitwise what was uploaded; returns the array"""
        w = self.buf.cpu().numpy()
        bits = w.view(np.int64)
        assert bits[0] == _GUARD_BITS and (bits[self.n + 1:] == _GUARD_BITS).all(), \
            ("guard word overwritten", self.name, w[0], w[self.n + 1:])
        if is_input:
            same = bits[1:self.n + 1] == self.sent.view(np.int64)
            assert same.all(), ("input changed", self.name, np.flatnonzero(~same)[:8])
        return w[1:self.n + 1].reshape(self.shape)


class GuardedSystem:
    """the six arrays of a linear system in six separate guarded buffers, with the interface of calibr8_amd.LinearSystem that
    Assembler uses (.A, .b, c_struct())"""

    def __init__(self, asm, ls):
        self.gA = [[Guarded(asm, "A%d%d" % (i, j), ls.A[i][j]) for j in range(2)] for i in range(2)]
        self.gb = [Guarded(asm, "b%d" % i, ls.b[i]) for i in range(2)]
        self.A = [[g.t for g in row] for row in self.gA]
        self.b = [g.t for g in self.gb]

    def c_struct(self):
        from calibr8_amd import lib as _l
        s = _l.System()
        for i in range(2):
            s.b[i] = self.b[i].data_ptr()
            for j in range(2):
                s.A[i][j] = self.A[i][j].data_ptr()
        return s

    def finish(self, ls, A_is_input=False):
        for i in range(2):
            ls.b[i][:] = self.gb[i].check(False)
            for j in range(2):
                ls.A[i][j][:] = self.gA[i][j].check(A_is_input)


@functools.lru_cache(maxsize=None)
def guarded_backend():
    """the class GuardedBackend, derived from gpu_backend.GpuBackend (which imports the device package) at first use"""
    from gpu_backend import GpuBackend

    class GuardedBackend(GpuBackend):
        """GpuBackend with every device array between guard words: after every entry point and one synchronisation the guards
        and the inputs of that entry point are compared bit for bit"""
        calls = 0

        def _ins(self, **named):
            return [Guarded(self.asm, k, v) for k, v in named.items()]

        def _done(self, inputs, outputs=(), system=None, A_is_input=False):
            import torch
            torch.cuda.synchronize()
            for g in inputs:
                g.check(True)
            for g, host in outputs:
                host[...] = g.check(False)
            if system is not None:
                system[0].finish(system[1], A_is_input)
            self.calls += 1

        def forward_jacobian(self, u, p, u_prev, p_prev, xi_prev, xi, ls):
            st = self._ins(u=u, p=p, u_prev=u_prev, p_prev=p_prev, xi_prev=xi_prev)
            gxi, gs = Guarded(self.asm, "xi", xi), GuardedSystem(self.asm, ls)
            rc = self.asm.forward_jacobian(*[g.t for g in st], gxi.t, gs)
            self._done(st, [(gxi, xi)], (gs, ls))
            return rc

        def global_residual(self, u, p, u_prev, p_prev, xi_prev, xi, ls):
            st = self._ins(u=u, p=p, u_prev=u_prev, p_prev=p_prev, xi_prev=xi_prev, xi=xi)
            gs = GuardedSystem(self.asm, ls)
            rc = self.asm.global_residual(*[g.t for g in st], gs)
            self._done(st, (), (gs, ls), A_is_input=True)  # the residual-only assembly leaves the matrix as it is
            return rc

        def adjoint_jacobian(self, u, p, u_prev, p_prev, xi_prev, xi, g, f, ls):
            st = self._ins(u=u, p=p, u_prev=u_prev, p_prev=p_prev, xi_prev=xi_prev, xi=xi)
            gf, gg, gs = Guarded(self.asm, "f", f), Guarded(self.asm, "g", g), GuardedSystem(self.asm, ls)
            rc = self.asm.adjoint_jacobian(*[x.t for x in st], gg.t, gf.t, gs)
            self._done(st + [gf], [(gg, g)], (gs, ls))
            return rc

        def solve_adjoint_local(self, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi, g, f):
            st = self._ins(u=u, p=p, u_prev=u_prev, p_prev=p_prev, xi_prev=xi_prev, xi=xi)
            z = self._ins(z_u=z_u, z_p=z_p)
            gphi, gg, gf = Guarded(self.asm, "phi", phi), Guarded(self.asm, "g", g), Guarded(self.asm, "f", f)
            rc = self.asm.solve_adjoint_local(*[x.t for x in st], z[0].t, z[1].t, gphi.t, gg.t, gf.t)
            self._done(st + z, [(gphi, phi), (gg, g), (gf, f)])
            return rc

        def qoi_gradient(self, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi, nparams):
            st = self._ins(u=u, p=p, u_prev=u_prev, p_prev=p_prev, xi_prev=xi_prev, xi=xi, z_u=z_u, z_p=z_p, phi=phi)
            grad = np.zeros(nparams)
            gg = Guarded(self.asm, "grad", grad)
            self.asm.qoi_gradient(*[x.t for x in st], gg.t)
            self._done(st, [(gg, grad)])
            return grad

        def eval_qoi(self, u, p):
            st = self._ins(u=u, p=p)
            J = np.zeros(1)
            gJ = Guarded(self.asm, "J", J)
            self.asm.eval_qoi(st[0].t, st[1].t, gJ.t)
            self._done(st, [(gJ, J)])
            return float(J[0])

    return GuardedBackend


def _guard_cases():
    """every (form, element type) pair that the library accepts, under every scatter mode it accepts for the chain, at
    unit + 1 and period unit + 1 of the rows of UNITS that the form reaches"""
    out = []
    for kind in lc.KINDS:
        u = lc.row("group", kind).unit
        for form in lc.FORMS:
            if (form, kind) in lc.UNSUPPORTED:
                continue
            for scatter in lc.SCATTERS[kind]:
                if (form, kind, scatter) in lc.CHAIN_REFUSED or (form == "node" and scatter != "gather"):
                    continue
                models = [lc.MODELS[kind][0]]
                if (kind, form) in (("hex8", "wave"), ("tet4", "auto"), ("tri3", "auto")):
                    models.append(lc.MODELS[kind][1])  # an automatically differentiated model as well
                for model, params, eps in models:
                    if kind != "hex8" or form == "slot":
                        ns = [(u + 1, kind == "hex8"), (8 * u + 1, False)]
                    elif form == "node":
                        ns = [(9, True), (27, True), (-2049, False)]  # 9 = a group of eight and one; 2049 nodes = period + 1
                    elif form == "auto" and scatter == "gather" and model in lc.CLOSED_FORM:
                        ns = [(9, True), (27, True)]                  # the same launch as `node` (c8_api.hip:516-518)
                    else:
                        ns = [(9, True), (65, False), (257, False)]   # groups of eight: 8 + 1, 64 + 1; stripes: 256 + 1
                    out += [lc.Case("guard", kind, form, scatter, model, tuple(params), eps, n, cut) for n, cut in ns]
    return out


GUARD_CASES = _guard_cases()
# xi of K1 is an output by c8.h.  One model of the table reads it: hyper_J2_plane_stress keeps lambda_z and alpha of the xi it
# is given as the starting point of its local Newton iteration (c8_models.hpp, HyperJ2PlaneStress::initial_guess, as the
# reference's model does; with lambda_z = -1.5e-3 the iteration does not converge and the call returns -1).  For it the two
# prefills are two starting points near the initial state, and the comparison at 1e-12 is: the two local states directly
# (3.4e-13 and 5.8e-13 on the emulator at 11 and 81 triangles), and each system against the oracle by the project's rule for
# K1 (parity_cases.forward_errors: directly, or against the oracle at the device's own converged state).  The two systems
# themselves differ by up to 2e-10 of |b| and 5e-11 of a row of A: the iteration stops at |C| < 1e-12, two starting points stop
# at states 5e-13 apart, and the residual follows the state (the figures of forward_errors' own note).  Every other form of
# every other model gives the same bits whatever xi holds.
READS_XI = ("hyper_J2_plane_stress",)


@functools.lru_cache(maxsize=1)
def _steps(cs):
    """the oracle's history of a case, solved once for the several uses of one test"""
    orc, c, _ = lc.oracle_of(cs)
    return pc.two_steps(orc, c, cs.eps)


def _sequence(be, orc, c, cs, rng_seed=31):
    """K1, K2, K3, K4, K5 and the objective once, at the second step of the table's history: {name: array}"""
    st = _steps(cs)
    (u, p, xi), (up, pp, xip) = st[2], st[1]
    rng = np.random.default_rng(rng_seed)
    out = {}
    ls, x = be.new_linsys(), be.new_state()
    assert be.forward_jacobian(u, p, up, pp, xip, x, ls) == 0
    out.update({"K1.xi": x, "K1.b0": ls.b[0], "K1.b1": ls.b[1]}, **{"K1.A%d%d" % (i, j): ls.A[i][j] for i in range(2) for j in range(2)})
    ls = be.new_linsys()
    assert be.global_residual(u, p, up, pp, xip, xi, ls) == 0
    out.update({"K2.b0": ls.b[0], "K2.b1": ls.b[1]})
    g = 1e-3 * rng.standard_normal((orc.nelems, orc.npts, orc.nloc))
    f = 1e-3 * rng.standard_normal((orc.nelems, orc.npts, orc.ndofs))
    ls = be.new_linsys()
    assert be.adjoint_jacobian(u, p, up, pp, xip, xi, g, f, ls) == 0
    out.update({"K3.g": g.copy(), "K3.b0": ls.b[0], "K3.b1": ls.b[1]}, **{"K3.A%d%d" % (i, j): ls.A[i][j] for i in range(2) for j in range(2)})
    z_u, z_p = 1e-3 * rng.standard_normal(len(u)), 1e-3 * rng.standard_normal(len(p))
    phi = np.zeros_like(g)
    assert be.solve_adjoint_local(u, p, up, pp, xip, xi, z_u, z_p, phi, g, f) == 0
    out.update({"K4.phi": phi, "K4.g": g, "K4.f": f})
    act = pc.ACTIVE[cs.model]
    be.set_active(0, act)
    out["K5.grad"] = be.qoi_gradient(u, p, up, pp, xip, xi, z_u, z_p, phi, len(act))
    out["K6.J"] = np.array([be.eval_qoi(u, p)])
    return out


def _agree(a, b, exact, name, bound=1e-13):
    if exact:
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (name, float(np.abs(a - b).max()))
    elif a.size:
        assert np.abs(a - b).max() <= bound * max(np.abs(b).max(), 1e-300), (name, float(np.abs(a - b).max()), float(np.abs(b).max()))


def _reproducible(name, scatter):
    """whether two runs of an output give the same bits: per-element outputs always; the systems of K1 and K3 under the
    staged assembly (fixed order of the row sums); never what is added with atomics in every mode (K2's residual, K5, the
    objective)"""
    if name in ("K1.xi", "K3.g") or name.startswith("K4."):
        return True
    return scatter == "gather" and name[:2] in ("K1", "K3")


@pytest.mark.parametrize("cs", GUARD_CASES, ids=[lc.case_id(cs) for cs in GUARD_CASES])
def test_guard_bands_and_untouched_inputs(cs):
    """every array of every entry point between guard words at an address = 8 mod 16: the chain against the oracle, then
    K1 .. K5 and the objective once more beside the unguarded backend -- the same bits where the scatter mode is
    reproducible, 1e-13 of the largest entry where it adds with atomics -- and K1 with two different contents of its
    output xi (READS_XI above: hyper_J2_plane_stress takes its starting point from it, compared at 1e-12)"""
    orc, c, conn = lc.oracle_of(cs)
    gd = device(cs.form, cs.scatter, guarded=True)(orc.elem_type, c, conn, cs.model, list(cs.params))
    lc.run_chain(orc, gd, c, cs.model, cs.eps)
    assert gd.calls >= 10
    plain = device(cs.form, cs.scatter)(orc.elem_type, c, conn, cs.model, list(cs.params))
    a, b = _sequence(gd, orc, c, cs), _sequence(plain, orc, c, cs)
    assert a.keys() == b.keys()
    for name in a:
        _agree(a[name], b[name], _reproducible(name, cs.scatter), name)
    # K1 into two different prefills of xi
    st = _steps(cs)
    (u, p, _), (up, pp, xip) = st[2], st[1]
    x0 = gd.new_state()
    k = np.arange(x0.size, dtype=np.float64).reshape(x0.shape)
    if cs.model in READS_XI:
        fills = [x0 * (1.0 + 1e-3 * np.cos(k)), x0 + 1e-3 * np.sin(k)]
    else:
        fills = [0.37 + 1e-6 * k, -1.5e-3 - 1e-5 * np.cos(k)]
    res = []
    for fill in fills:
        x, ls = fill.copy(), gd.new_linsys()
        assert gd.forward_jacobian(u, p, up, pp, xip, x, ls) == 0
        res.append((x, ls))
    (xa, la), (xb, lb) = res
    if cs.model in READS_XI:
        assert rel_vec(xa, xb) < 1e-12, rel_vec(xa, xb)
        ls_o, xo = orc.new_linsys(), orc.new_state()
        assert orc.forward_jacobian(u, p, up, pp, xip, xo, ls_o) == 0
        for x, ls in res:
            errs, direct, same = pc.forward_errors(orc, ls, x, ls_o, xo, u, p, up, pp, xip)
            print("%s: xi prefill: direct deviation of the system %.3e, at the device's own state %.3e, xi %.3e" %
                  (lc.case_id(cs), direct, max(v for k, v in errs.items() if k != "xi"), errs["xi"]))
            assert max(errs.values()) < 1e-12, errs
    else:
        _agree(xa, xb, True, "xi")
        for i in range(2):
            _agree(la.b[i], lb.b[i], cs.scatter == "gather", "b%d" % i)
            for j in range(2):
                _agree(la.A[i][j], lb.A[i][j], cs.scatter == "gather", "A%d%d" % (i, j))


# ---- (c) above the cap of 2048 blocks -------------------------------------------------------------------------------------------
# (kind, form, model, params, count): K5 and the objective in every form they have, where the grid-stride loop takes a
# second turn with a partly filled last unit (launch_cases.above_cap)
CAP_CASES = [("hex8", "wave", "hyper_J2", pc.HJ2, lc.above_cap("hex8", True)),    # k_param_gradient_wave, k_qoi_wave
             ("hex8", "auto", "small_J2", pc.J2, lc.above_cap("hex8", True)),     # k_param_gradient_wave<CLOSED>
             ("hex8", "slot", "small_J2", pc.J2, lc.above_cap("hex8")),           # k_param_gradient, k_qoi
             ("tet4", "auto", "hyper_J2", pc.HJ2, lc.above_cap("tet4")),
             ("tri3", "auto", "small_J2", pc.J2, lc.above_cap("tri3")),
             ("tri3ps", "auto", "hyper_J2_plane_stress", pc.HJ2_PSS, lc.above_cap("tri3ps"))]


@pytest.mark.parametrize("kind,form,model,params,n", CAP_CASES, ids=["%s-%s-%s-%d" % (t[0], t[1], t[2], t[4]) for t in CAP_CASES])
def test_param_gradient_and_objective_above_the_block_cap(kind, form, model, params, n):
    """K5 and eval_qoi (average displacement) against the oracle on cauchy_cases.synthetic_state (no oracle solve) with
    random z and phi, at the bar that check_adjoint_chain applies to K5: every component within 1e-12 of the sum of the
    magnitudes of the products summed into it; the objective within 1e-12 max(1, |J|).  No allowance for the longer sum
    was needed.  Measured on an MI355X (printed by every run): K5 between 7e-17 (tet4) and 5.4e-15 (plane-stress tri3) of
    that scale; the objective between 1e-15 and 1.7e-14 of |J| (hex8 2.7e-11 of J = 1479, tri3 6.1e-10 of J = 1.56e5)."""
    assert [n] == [c for c in [16391, 4099, 8195, 14339, 20483] if c == n]  # the counts of the table's arithmetic test
    et, c, conn = lc.mesh(kind, n)
    orc = ol.Oracle(et, c, conn, model, params)
    dut = device(form, "atomic")(et, c, conn, model, params)
    u, p, up, pp, xip, xi = cc.synthetic_state(orc.new_state(), c, orc.ndims, orc.nres, seed=n)
    xi = xip + np.abs(xi - xip)  # the local state moved upwards only (a negative hardening variable has no power)
    rng = np.random.default_rng(n + 1)
    z_u, z_p, phi = rng.standard_normal(len(u)), rng.standard_normal(len(p)), rng.standard_normal(xi.shape)
    act = pc.ACTIVE[model]
    orc.set_active(0, act)
    dut.set_active(0, act)
    gr_o, gr_scale = orc.qoi_gradient_with_scale(u, p, up, pp, xip, xi, z_u, z_p, phi, len(act))
    gr_d = dut.qoi_gradient(u, p, up, pp, xip, xi, z_u, z_p, phi, len(act))
    k5 = np.abs(gr_d - gr_o) / np.maximum(gr_scale, 1e-300)
    J_o, J_d = orc.eval_qoi(u, p), dut.eval_qoi(u, p)
    print("%s %s %s %d: K5 max deviation / scale %.3e, |J - J_ref| %.3e (J %.6e)" % (kind, form, model, n, k5.max(), abs(J_d - J_o), J_o))
    assert np.abs(gr_o).min() > 0 and np.isfinite(gr_d).all()
    assert k5.max() < TOL, (gr_d, gr_o, gr_scale)
    assert abs(J_d - J_o) < TOL * max(1.0, abs(J_o)), (J_d, J_o)


# ---- (d) c8_assemble_forward_jacobian_subset --------------------------------------------------------------------------------
SUBSET_CASES = [("hex8", "wave", "small_J2", pc.J2, 8), ("hex8", "wave", "hyper_J2", pc.HJ2, 8), ("hex8", "slot", "small_J2", pc.J2, 2),
                ("tet4", "auto", "hyper_J2", pc.HJ2, 4), ("tri3", "auto", "small_J2", pc.J2, 7),
                ("tri3ps", "auto", "hyper_J2_plane_stress", pc.HJ2_PSS, 10)]


def _dense(be, ls, i, j):
    import scipy.sparse as sp
    shape = (len(be.rowptr[i][j]) - 1, len(be.rowptr[j][i]) - 1)
    return sp.csr_matrix((ls.A[i][j], be.colidx[i][j], be.rowptr[i][j]), shape=shape).toarray()


def _subset_call(be, state, elems, ls_host, xi_host):
    """forward_jacobian_subset through guarded arrays; returns the device system and xi on the host"""
    import torch
    asm = be.asm
    names = ("u", "p", "u_prev", "p_prev", "xi_prev")
    st = [Guarded(asm, k, v) for k, v in zip(names, state)]
    gxi, gs = Guarded(asm, "xi", xi_host), GuardedSystem(asm, ls_host)
    lst = torch.as_tensor(np.ascontiguousarray(elems, dtype=np.int32)).to(asm.device)
    rc = asm.forward_jacobian_subset(*[g.t for g in st], gxi.t, gs, lst)
    torch.cuda.synchronize()
    for g in st:
        g.check(True)
    assert np.array_equal(lst.cpu().numpy(), np.asarray(elems, dtype=np.int32))
    xi_host[...] = gxi.check(False)
    gs.finish(ls_host)
    return rc


def _onto_submesh(be, sub, used, ls_d):
    """the device's system (graph of the whole mesh) as a system over the graph of the oracle `sub` on the nodes `used`:
    every entry outside the rows and columns of those nodes, and outside the sub-mesh's graph, must be exactly zero"""
    neq = (be.ndims, 1)
    dofs = [(used[:, None] * neq[i] + np.arange(neq[i])).ravel() for i in range(2)]
    out = sub.new_linsys()
    for i in range(2):
        b = np.asarray(ls_d.b[i])
        out.b[i][:] = b[dofs[i]]
        assert np.count_nonzero(b) == np.count_nonzero(out.b[i])
        for j in range(2):
            D = _dense(be, ls_d, i, j)
            rp, ci = np.asarray(sub.rowptr[i][j]), np.asarray(sub.colidx[i][j])
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
            out.A[i][j][:] = D[np.ix_(dofs[i], dofs[j])][rows, ci]
            assert np.count_nonzero(D) == np.count_nonzero(out.A[i][j]), (i, j)
    return out


class SubsetDut:
    """c8_assemble_forward_jacobian_subset on the whole mesh behind the interface of a backend on the mesh of the listed
    elements alone: fields given on the sub-mesh go to their places in the whole mesh, every other nodal value and every
    other element's previous state is NaN (an element that is not listed must not be read), the system comes back over
    the sub-mesh's graph (every other entry must be exactly zero) and xi of every other element must be left as it was"""
    FILL = 0.625

    def __init__(self, dut, sub, elems, used):
        self.dut, self.sub, self.elems, self.used = dut, sub, np.asarray(elems), used
        self.new_state, self.new_linsys = sub.new_state, sub.new_linsys

    def _nodal(self, v, k):
        out = np.full((self.dut.nnodes, k), np.nan)
        out[self.used] = np.asarray(v).reshape(-1, k)
        return out.ravel()

    def forward_jacobian(self, u, p, u_prev, p_prev, xi_prev, xi, ls):
        d, nd = self.dut, self.dut.ndims
        xip = np.full((d.nelems, d.npts, d.nloc), np.nan)
        xip[self.elems] = xi_prev
        xif = np.full((d.nelems, d.npts, d.nloc), self.FILL)
        xif[self.elems] = xi
        full = d.new_linsys()
        rc = _subset_call(d, (self._nodal(u, nd), self._nodal(p, 1), self._nodal(u_prev, nd), self._nodal(p_prev, 1), xip),
                          self.elems, full, xif)
        rest = np.setdiff1d(np.arange(d.nelems), self.elems)
        assert (xif[rest] == self.FILL).all()
        xi[...] = xif[self.elems]
        part = _onto_submesh(d, self.sub, self.used, full)
        for i in range(2):
            ls.b[i][:] += part.b[i]
            for j in range(2):
                ls.A[i][j][:] += part.A[i][j]
        return rc


@pytest.mark.parametrize("kind,form,model,params,unit", SUBSET_CASES, ids=["%s-%s-%s" % t[:3] for t in SUBSET_CASES])
def test_forward_jacobian_subset(kind, form, model, params, unit):
    """lists of 1, unit - 1 and unit + 1 elements (unit: the elements of a block; on the hex8 wave kernel the 8 blocks of the
    remap), a permuted list, and two disjoint lists whose union is the mesh: each through parity_cases.check_forward,
    unchanged, against the oracle on the mesh of the listed elements alone (SubsetDut), at 1e-12; the union against the
    full atomic assembly at 1e-13 of the largest entry, with the same bits in xi"""
    n = 8 * unit + 3 if unit < 8 else 3 * unit + 3
    et, c, conn = lc.mesh(kind, n, kind == "hex8")
    dut = device(form, "atomic")(et, c, conn, model, params)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    half = np.sort(perm[:n // 2 + 1])
    lists = {"one": perm[:1], "unit-1": np.sort(perm[:unit - 1]), "unit+1": np.sort(perm[:unit + 1]), "permuted": perm[:unit + 3],
             "half": half, "other half": np.setdiff1d(np.arange(n), half)}
    assert len(lists["half"]) + len(lists["other half"]) == n and not np.array_equal(lists["permuted"], np.sort(lists["permuted"]))
    for name, elems in lists.items():
        used = np.unique(conn[elems])
        cs_, conn_s = cc.sub_mesh(c, conn[elems], len(elems))
        sub = ol.Oracle(et, cs_, conn_s, model, params)
        pc.check_forward(sub, SubsetDut(dut, sub, elems, used), cs_, model, 0.004, TOL)
    full = ol.Oracle(et, c, conn, model, params)
    st = pc.two_steps(full, c, 0.004)
    (u, p, _), (up, pp, xip) = st[2], st[1]
    union, union_xi = dut.new_linsys(), dut.new_state()
    for name in ("half", "other half"):
        assert _subset_call(dut, (u, p, up, pp, xip), lists[name], union, union_xi) == 0
    whole, xw = dut.new_linsys(), dut.new_state()
    assert dut.forward_jacobian(u, p, up, pp, xip, xw, whole) == 0
    assert np.array_equal(union_xi, xw) and not np.array_equal(xw, dut.new_state())
    for i in range(2):
        _agree(union.b[i], whole.b[i], False, "union b%d" % i)
        for j in range(2):
            _agree(union.A[i][j], whole.A[i][j], False, "union A%d%d" % (i, j))
