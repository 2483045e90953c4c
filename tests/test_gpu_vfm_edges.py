"""`-m gpu`: k_vfm and k_vfm_reduce (c8_kernels.hip, c8_vfm.hip) at the edges of their launch, through c8_vfm_internal_power
(V), c8_vfm_forward_sens (FS) and c8_vfm_adjoint_step (A); the table and the references are those of vfm_edge_cases.py,
test_vfm_emul_edges.py runs the same table on the CPU.
  (a) every count of the table, V -> FS over the steps and A backwards, every array between guard words at an address that
      is 8- but not 16-byte aligned, inputs compared bit for bit after every call, every output against the oracle;
  (b) every parameter of the three models in every layout of the active lists, at 21 elements: the columns of S of the
      other set's parameters keep a sentinel, without active parameters S is NULL and divw / grad are left alone;
  (c) ivw, divw and grad are added to what the caller holds with one add; b += R; S_prev NULL is an all-zero S_prev;
      x[1] / x_prev[1] NULL change nothing;
  (d) the same bits on every run, and from a partials buffer that has grown and holds stale values;
  (e) async mode on the default stream.
One process, no mesh above 5121 triangles."""
import numpy as np
import pytest

import vfm_edge_cases as ve
from parity import rel_vec

pytestmark = pytest.mark.gpu
TRI3 = 3  # c8.h: C8_TRI3


def _guarded():
    from test_gpu_launch_edges import Guarded
    return Guarded


class GpuDut:
    """the interface of vfm_edge_cases.run_case on calibr8_amd.Assembler, every array of every call in a guarded buffer of
    its own (test_gpu_launch_edges.Guarded); after the call and one synchronisation the guard words and the inputs -- u,
    u_prev, xi_prev, w, S_prev, and for A also xi -- are compared bit for bit"""

    def __init__(self, cs, max_iters=None, null_p=False):
        import torch
        from calibr8_amd import Assembler
        self.torch, self.Guarded = torch, _guarded()
        c, conn, es, P, _, w = ve.setup(cs.model, cs.n)
        kw = {} if max_iters is None else {"max_iters": max_iters}
        self.asm = Assembler(TRI3, c, conn, cs.model, P, elem_set=es, **kw)
        assert self.asm.nelems == cs.n
        self.set_active(cs.active)
        self.gw = self.Guarded(self.asm, "w", w)
        self.asm.vfm_set_virtual_field(self.gw.t)
        self.p0 = torch.zeros(self.asm.nnodes, dtype=torch.float64, device=self.asm.device)
        self.calls = 0
        if null_p:  # c8.h: under one residual the entries [1] of x and x_prev are not read
            make = type(self.asm)._state

            def state(*a):
                st = make(*a)
                st.x[1], st.x_prev[1] = None, None
                return st
            self.asm._state = state

    def set_active(self, active):
        for s, a in enumerate(active):
            self.asm.set_active(s, list(a))

    def _up(self, **named):
        return {k: self.Guarded(self.asm, k, v) for k, v in named.items() if v is not None}

    def _done(self, ins, outs, hosts):
        self.torch.cuda.synchronize()
        self.gw.check(True)
        for g in ins.values():
            g.check(True)
        for k, g in outs.items():
            hosts[k][...] = g.check(False)
        self.calls += 1

    @staticmethod
    def _t(d, k):
        return d[k].t if k in d else None

    def V(self, u, up, xip, xi, b, ivw):
        i, o = self._up(u=u, u_prev=up, xi_prev=xip), self._up(xi=xi, b=b, ivw=ivw)
        rc = self.asm.vfm_internal_power(i["u"].t, self.p0, i["u_prev"].t, self.p0, i["xi_prev"].t, o["xi"].t, o["ivw"].t, self._t(o, "b"))
        self._done(i, o, {"xi": xi, "b": b, "ivw": ivw})
        return rc

    def FS(self, u, up, xip, xi, S_prev, S, ivw, divw):
        i, o = self._up(u=u, u_prev=up, xi_prev=xip, S_prev=S_prev), self._up(xi=xi, S=S, ivw=ivw, divw=divw)
        rc = self.asm.vfm_forward_sens(i["u"].t, self.p0, i["u_prev"].t, self.p0, i["xi_prev"].t, o["xi"].t, self._t(i, "S_prev"),
                                       self._t(o, "S"), o["ivw"].t, o["divw"].t)
        self._done(i, o, {"xi": xi, "S": S, "ivw": ivw, "divw": divw})
        return rc

    def A(self, u, up, xip, xi, cm, h, grad):
        i, o = self._up(u=u, u_prev=up, xi_prev=xip, xi=xi), self._up(h=h, grad=grad)
        rc = self.asm.vfm_adjoint_step(i["u"].t, self.p0, i["u_prev"].t, self.p0, i["xi_prev"].t, i["xi"].t, cm, o["h"].t, o["grad"].t)
        self._done(i, o, {"h": h, "grad": grad})
        return rc


WORST = {}


def _run(cs):
    worst = WORST.setdefault(cs.model, ve.Worst())
    dut = GpuDut(cs)
    ve.run_case(dut, cs, worst)
    assert dut.calls == 3 * (len(ve.SEQ) - 1)
    print("device, worst so far, %s: %s" % (cs.model, worst))


# ---- (a) counts and guard bands ---------------------------------------------------------------------------------------------
COUNT_CASES = ve.count_cases()


@pytest.mark.parametrize("cs", COUNT_CASES, ids=[ve.case_id(cs) for cs in COUNT_CASES])
def test_chain_at_the_count_between_guard_words(cs):
    _run(cs)


# ---- (b) every parameter, every layout --------------------------------------------------------------------------------------
LAYOUT_CASES = ve.layout_cases()


@pytest.mark.parametrize("cs", LAYOUT_CASES, ids=[ve.case_id(cs) for cs in LAYOUT_CASES])
def test_every_parameter_in_every_layout(cs):
    """run_case fills S with a sentinel and asserts that the other set's columns keep it; without active parameters it
    passes S = None and asserts that divw and grad keep their sentinel while xi, ivw and h are right"""
    _run(cs)


# ---- single calls at one step -----------------------------------------------------------------------------------------------
class Step:
    """the inputs of V, FS and A at step 2 of a case (loaded further, S_prev and h not trivial) and single calls from
    given starting values of the sums; every call returns its outputs by name"""

    def __init__(self, cs, seed=7):
        self.cs, self.ref = cs, ve.references(cs)
        self.steps = ve.setup(cs.model, cs.n)[4]
        self.shape = self.ref.xi[0].shape
        self.rng = np.random.default_rng(seed)
        self.h = 1e-3 * self.rng.standard_normal(int(np.prod(self.shape)))

    def s_prev(self, nact):
        return 1e-3 * np.random.default_rng(11).standard_normal(self.shape + (nact,)) if nact else None

    def V(self, dut, ivw0=0.0, b0=None, n=2, expect=0):
        xi, ivw = self.ref.xi[n - 1].copy(), np.full(1, ivw0)
        b = np.zeros(len(self.steps[n])) if b0 is None else b0.copy()
        assert dut.V(self.steps[n], self.steps[n - 1], self.ref.xi[n - 1], xi, b, ivw) == expect
        return {"xi": xi, "b": b, "ivw": ivw}

    def FS(self, dut, nact, ivw0=0.0, divw0=None, S_prev="random", n=2):
        xi, ivw = self.ref.xi[n - 1].copy(), np.full(1, ivw0)
        divw = np.zeros(nact) if divw0 is None else divw0.copy()
        S = np.full(self.shape + (nact,), ve.SENTINEL)
        Sp = self.s_prev(nact) if isinstance(S_prev, str) else S_prev
        assert dut.FS(self.steps[n], self.steps[n - 1], self.ref.xi[n - 1], xi, Sp, S, ivw, divw) == 0
        return {"xi": xi, "S": S, "ivw": ivw, "divw": divw}

    def A(self, dut, nact, grad0=None, n=2):
        h = self.h.copy()
        grad = np.zeros(nact) if grad0 is None else grad0.copy()
        assert dut.A(self.steps[n], self.steps[n - 1], self.ref.xi[n - 1], self.ref.xi[n], 0.7, h, grad) == 0
        return {"h": h, "grad": grad}


def same_bits(a, b, skip=("b",)):
    assert a.keys() == b.keys()
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), (k, float(np.abs(a[k] - b[k]).max()))


# ---- (c) += semantics, NULL arguments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ve.REDUCE_MODELS)
def test_sums_are_added_to_what_the_caller_holds(model):
    """ivw, divw, grad: the reduction does ONE add per output, so from a start value the result is start + (the result from
    zero), bit for bit; b += R is an atomic scatter and holds to 1e-12 of the largest entry of R"""
    cs = ve.Case(model, 171, ve.COUNT_LAYOUT)
    st, dut, nact = Step(cs), GpuDut(cs), ve.nact_of(cs)
    rng = np.random.default_rng(3)
    zero = st.V(dut)
    b0 = rng.standard_normal(zero["b"].size)
    got = st.V(dut, ivw0=0.37, b0=b0)
    assert zero["ivw"][0] != 0 and got["ivw"][0] == 0.37 + zero["ivw"][0]
    assert np.array_equal(got["xi"], zero["xi"]) and np.abs(zero["b"]).max() > 0
    assert np.abs(got["b"] - (b0 + zero["b"])).max() <= ve.TOL * np.abs(zero["b"]).max()
    zero = st.FS(dut, nact)
    d0 = rng.standard_normal(nact)
    got = st.FS(dut, nact, ivw0=-1.25, divw0=d0)
    assert (zero["divw"] != 0).all() and got["ivw"][0] == -1.25 + zero["ivw"][0]
    assert np.array_equal(got["divw"], d0 + zero["divw"])
    same_bits({k: got[k] for k in ("xi", "S")}, {k: zero[k] for k in ("xi", "S")})
    zero = st.A(dut, nact)
    g0 = rng.standard_normal(nact)
    got = st.A(dut, nact, grad0=g0)
    assert (zero["grad"] != 0).all() and np.array_equal(got["grad"], g0 + zero["grad"]) and np.array_equal(got["h"], zero["h"])


@pytest.mark.parametrize("model", ve.REDUCE_MODELS)
def test_null_arguments_are_what_the_header_says(model):
    cs = ve.Case(model, 171, ve.COUNT_LAYOUT)
    st, dut, nact = Step(cs), GpuDut(cs), ve.nact_of(cs)
    # S_prev = NULL is an all-zero S_prev
    same_bits(st.FS(dut, nact, S_prev=None), st.FS(dut, nact, S_prev=np.zeros(st.shape + (nact,))))
    # x[1] and x_prev[1] are not read under one residual: NULL there changes nothing
    nul = GpuDut(cs, null_p=True)
    same_bits(st.V(nul), st.V(dut))
    same_bits(st.FS(nul, nact), st.FS(dut, nact))
    same_bits(st.A(nul, nact), st.A(dut, nact))
    assert nul.calls == 3


# ---- (d) fixed order, the partials buffer -------------------------------------------------------------------------------------
ONE = ((3,), ())
TWELVE = ((0, 1, 2, 3, 4, 5), (3, 4, 5, 0, 1, 2))


@pytest.mark.parametrize("model", ve.REDUCE_MODELS)
def test_same_bits_on_every_run_and_from_a_regrown_partials_buffer(model):
    """at 2561 elements (257 blocks: thread 0 of the reduction takes two).  On ONE context: V (a buffer of 257 partials), FS
    with twelve active parameters (c8_vfm.hip:61-67: the buffer is freed and allocated anew for 13 x 257), A with one (the
    larger buffer, holding the partials of FS).  Each against the same call alone on a fresh context, bit for bit."""
    cs = ve.Case(model, 2561, ve.COUNT_LAYOUT)
    st, dut, nact = Step(cs), GpuDut(cs), ve.nact_of(cs)
    for call in (lambda: st.V(dut), lambda: st.FS(dut, nact), lambda: st.A(dut, nact)):
        a, b = call(), call()
        same_bits(a, b)
        assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in a.values())
    one = GpuDut(cs)
    v = st.V(one)
    one.set_active(TWELVE)
    fs = st.FS(one, 12)
    one.set_active(ONE)
    a = st.A(one, 1)
    same_bits(v, st.V(GpuDut(cs)))
    fresh = GpuDut(ve.Case(model, 2561, TWELVE))
    same_bits(fs, st.FS(fresh, 12))
    fresh = GpuDut(ve.Case(model, 2561, ONE))
    same_bits(a, st.A(fresh, 1))
    assert a["grad"][0] != 0 and (fs["divw"] != 0).all()


# ---- (e) async mode on the default stream -------------------------------------------------------------------------------------
def test_async_mode_on_the_default_stream():
    from calibr8_amd import lib as _l
    cs = ve.Case("small_hill_plane_stress", 171, ve.COUNT_LAYOUT)
    st, sync, dut, nact = Step(cs), GpuDut(cs), GpuDut(cs), ve.nact_of(cs)
    dut.asm.set_async(1)
    for got, want in ((st.V(dut), st.V(sync)), (st.FS(dut, nact), st.FS(sync, nact)), (st.A(dut, nact), st.A(sync, nact))):
        assert dut.asm.status() == 0
        same_bits(got, want)
    # one local Newton iteration into the plastic range: the synchronous call reports it, the asynchronous one returns 0
    # and c8_status reports it
    assert ve.plastic_points(cs)[0] > 0
    one = GpuDut(cs, max_iters=1)
    st.V(one, n=1, expect=_l.C8_LOCAL_SOLVE_FAILED)
    one.asm.set_async(1)
    st.V(one, n=1, expect=0)
    assert one.asm.status() == _l.C8_LOCAL_SOLVE_FAILED
    assert one.asm.status() == 0  # reported once
