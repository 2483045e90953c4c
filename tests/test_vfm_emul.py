"""The VFM kernel source (calibr8_amd/csrc/c8_assemble_vfm.hpp) on the CPU lane emulator: V, FS and A against the oracle
compositions at 1e-12 on notch2D and on a two-set tri3 mesh for the three plane-stress models, and the full-objective
gradient from forward sensitivities against the one from the adjoint march and against central differences."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from parity import rel_vec
from vfm_cases import CYCLIC, MODELS, make_oracle, objective, oracle_adjoint_step, oracle_power, vfm_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
V, FS, A = 0, 1, 2


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/emul_vfm/c8_emul_vfm.cpp, built afresh for this session into its own temporary directory"""
    out = str(tmp_path_factory.mktemp("c8_emul_vfm"))
    so = os.path.join(out, "libc8emulvfm.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(ROOT, "tests", "emul_vfm", "c8_emul_vfm.cpp"),
                           os.path.join(ROOT, "calibr8_amd", "csrc", "c8_host.cpp")])
    L = C.CDLL(so)
    L.c8emu_vfm.restype = C.c_int
    L.c8emu_vfm.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, ip, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_double,
                            C.c_double, dp, ip, C.c_int, C.c_double, C.POINTER(dp)]
    return L


class EmuVfm:
    def __init__(self, L, c, conn, model, P, es, active, thickness=1.0):
        self.L, self.model, self.thickness = L, model, thickness
        self.c = np.ascontiguousarray(c, dtype=np.float64)
        self.conn = np.ascontiguousarray(conn, dtype=np.int32)
        self.es = None if es is None else np.ascontiguousarray(es, dtype=np.int32)
        self.P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        self.act = np.zeros((self.P.shape[0], 10), dtype=np.int32)
        ofs = 0
        for s, a in enumerate(active):
            self.act[s, 0], self.act[s, 1] = ofs, len(a)
            self.act[s, 2:2 + len(a)] = a
            ofs += len(a)
        self.nact = ofs

    def call(self, what, u, up, xip, xi, w, b=None, S_prev=None, S=None, h=None, cm=0.0):
        ivw, grad = np.zeros(1), np.zeros(max(self.nact, 1))
        arrs = [u, up, xip, xi, w, b, S_prev, S, h, ivw, grad]
        ptrs = (dp * 11)(*[None if a is None else a.ctypes.data_as(dp) for a in arrs])
        rc = self.L.c8emu_vfm(what, len(self.c), len(self.conn), self.c.ctypes.data_as(dp), self.conn.ctypes.data_as(ip),
                              None if self.es is None else self.es.ctypes.data_as(ip), self.P.shape[0], self.model.encode(),
                              500, 1e-12, 1e-12, self.thickness, self.P.ctypes.data_as(dp), self.act.ctypes.data_as(ip),
                              self.nact, cm, ptrs)
        return rc, float(ivw[0]), grad[:self.nact]


@pytest.mark.parametrize("mesh", ["notch2D", "two_sets"])
@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_kernels_match_oracle_composition(emu, mesh, model, params):
    check_composition(emu, mesh, model, params, None, 3)


@pytest.mark.parametrize("mesh", ["notch2D", "two_sets"])
@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_kernels_match_oracle_composition_cyclic(emu, mesh, model, params):
    # every step of the cyclic measured sequence (hold, elastic unloading, reversed flow)
    check_composition(emu, mesh, model, params, CYCLIC, len(CYCLIC))


def check_composition(emu, mesh, model, params, seq, nsteps):
    c, conn, es, P, active, steps, w = vfm_case(mesh, model, params, seq)
    orc = make_oracle(c, conn, model, P, es, active)
    dut = EmuVfm(emu, c, conn, model, P, es, active)
    nact = dut.nact
    shape = (orc.nelems, orc.npts, orc.nloc)
    xi_prev = orc.new_state()
    S_prev = None
    rng = np.random.default_rng(5)
    for n in range(1, nsteps):
        u, up = steps[n], steps[n - 1]
        rc, xo, bo = oracle_power(orc, u, up, xi_prev)
        assert rc == 0
        wabs = float(np.abs(w) @ np.abs(bo))
        # V: the converged state, w^T R and R itself
        xd, bd = xi_prev.copy(), np.zeros(len(u))
        rc, ivw, _ = dut.call(V, u, up, xi_prev, xd, w, b=bd)
        assert rc == 0
        assert rel_vec(xd, xo) < 1e-12 and rel_vec(bd, bo) < 1e-12
        assert abs(ivw - float(w @ bo)) < 1e-12 * wabs, (ivw, float(w @ bo))
        # FS: the same state and value (its sensitivities are checked through the gradients below)
        xf, S = xi_prev.copy(), np.zeros(orc.nelems * orc.npts * orc.nloc * nact)
        rc, ivw_f, divw = dut.call(FS, u, up, xi_prev, xf, w, S_prev=S_prev, S=S)
        assert rc == 0 and rel_vec(xf, xo) < 1e-12 and abs(ivw_f - float(w @ bo)) < 1e-12 * wabs
        assert np.abs(divw).max() > 0 and np.abs(S).max() > 0
        S_prev = S
        # A at the converged state: K4 with z = c w, g = -h, then K5 under an objective without own terms
        h = 1e-3 * rng.standard_normal(np.prod(shape))
        cm = 0.7
        ho, go, gabs = oracle_adjoint_step(orc, u, up, xi_prev, xo, w, cm, h, nact)
        hd = h.copy()
        rc, _, gd = dut.call(A, u, up, xi_prev, xo, w, h=hd, cm=cm)
        assert rc == 0
        assert rel_vec(hd, ho) < 1e-12
        assert np.all(np.abs(gd - go) <= 1e-12 * np.maximum(gabs, 1e-300)), (gd, go, gabs)
        xi_prev = xo


def emul_objective(dut, steps, w, loads, dt_over_T, scale, thickness, P=None, gradient=None):
    """value (and gradient: 'forward' | 'adjoint') of the VFM objective over the measured steps on the emulator"""
    if P is not None:
        dut.P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
    n = len(steps) - 1
    xi = [dut.xi0.copy()]
    ivw, divw = np.zeros(n), np.zeros((n, dut.nact))
    S_prev = None
    for s in range(1, n + 1):
        x = xi[-1].copy()
        if gradient == "forward":
            S = np.zeros(x.size * dut.nact)
            rc, ivw[s - 1], divw[s - 1] = dut.call(FS, steps[s], steps[s - 1], xi[-1], x, w, S_prev=S_prev, S=S)
            S_prev = S
        else:
            rc, ivw[s - 1], _ = dut.call(V, steps[s], steps[s - 1], xi[-1], x, w)
        assert rc == 0
        xi.append(x)
    J, cvec = objective(ivw, loads, dt_over_T, scale, thickness)
    if gradient is None:
        return J
    if gradient == "forward":
        return J, divw.T @ cvec
    h, grad = np.zeros(xi[0].size), np.zeros(dut.nact)
    for s in range(n, 0, -1):
        rc, _, g = dut.call(A, steps[s], steps[s - 1], xi[s - 1], xi[s], w, h=h, cm=float(cvec[s - 1]))
        assert rc == 0
        grad += g
    return J, grad


@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_forward_and_adjoint_gradients_agree_and_match_central_differences(emu, model, params):
    check_gradients(emu, model, params, None)


@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_gradients_agree_and_match_central_differences_cyclic(emu, model, params):
    check_gradients(emu, model, params, CYCLIC)


@pytest.mark.parametrize("model,params", MODELS)
def test_vfm_forward_sensitivities_match_central_differences_cyclic(emu, model, params):
    # the local sensitivities S = dxi/dp that FS carries forward, checked directly over the cyclic sequence: against
    # central differences of the oracle's converged state with respect to each active parameter of both sets
    c, conn, es, P, active, steps, w = vfm_case("two_sets", model, params, CYCLIC)
    orc = make_oracle(c, conn, model, P, es, active)
    dut = EmuVfm(emu, c, conn, model, P, es, active)
    nact, shape = dut.nact, (orc.nelems, orc.npts, orc.nloc)
    Ss, xi, S_prev = [], orc.new_state(), None
    for n in range(1, len(steps)):
        x, S = xi.copy(), np.zeros(xi.size * nact)
        rc, _, _ = dut.call(FS, steps[n], steps[n - 1], xi, x, w, S_prev=S_prev, S=S)
        assert rc == 0
        Ss.append(S.reshape(shape + (nact,)))
        xi, S_prev = x, S

    def states(Pq):
        o = make_oracle(c, conn, model, Pq, es, active)
        out, xp = [], o.new_state()
        for n in range(1, len(steps)):
            rc, xp, _ = oracle_power(o, steps[n], steps[n - 1], xp)
            assert rc == 0
            out.append(xp)
        return out

    k = 0
    for s, a in enumerate(active):
        for q in a:
            h = 1e-5 * max(1.0, abs(P[s, q]))  # central differences: truncation ~h^2, rounding ~1e-16 |xi| / h
            Pp, Pm = P.copy(), P.copy()
            Pp[s, q] += h
            Pm[s, q] -= h
            fds = [(xp - xm) / (2 * h) for xp, xm in zip(states(Pp), states(Pm))]
            scale = max(max(np.abs(fd).max() for fd in fds), 1e-300)  # the column's largest entry over the sequence
            assert scale > 0
            for n, fd in enumerate(fds):
                err = np.abs(Ss[n][..., k] - fd).max() / scale
                assert err <= 1e-6, (model, s, q, n + 1, err)
            k += 1


def check_gradients(emu, model, params, seq):
    c, conn, es, P, active, steps, w = vfm_case("two_sets", model, params, seq)
    orc = make_oracle(c, conn, model, P, es, active)
    thickness, scale = 0.7, 1e2
    dut = EmuVfm(emu, c, conn, model, P, es, active)
    dut.xi0 = orc.new_state()
    n = len(steps) - 1
    dt_over_T = np.full(n, 1.0 / n)
    # loads: the internal virtual power at other parameters, so that every step has a mismatch
    Pl = P.copy()
    Pl[:, 2] *= 1.1
    dut.P = np.ascontiguousarray(Pl)
    loads = []
    xip = dut.xi0.copy()
    for s in range(1, n + 1):
        x = xip.copy()
        rc, v, _ = dut.call(V, steps[s], steps[s - 1], xip, x, w)
        assert rc == 0
        loads.append(thickness * v)
        xip = x
    Jf, gf = emul_objective(dut, steps, w, loads, dt_over_T, scale, thickness, P=P, gradient="forward")
    Ja, ga = emul_objective(dut, steps, w, loads, dt_over_T, scale, thickness, P=P, gradient="adjoint")
    assert Jf == Ja and Jf > 0
    assert np.abs(gf - ga).max() < 1e-10 * np.abs(ga).max(), (gf, ga)
    # central differences of the emulated value, every active parameter of both sets
    k = 0
    for s, a in enumerate(active):
        for q in a:
            step = 1e-6 * max(1.0, abs(P[s, q]))
            Pp, Pm = P.copy(), P.copy()
            Pp[s, q] += step
            Pm[s, q] -= step
            fd = (emul_objective(dut, steps, w, loads, dt_over_T, scale, thickness, P=Pp) -
                  emul_objective(dut, steps, w, loads, dt_over_T, scale, thickness, P=Pm)) / (2 * step)
            assert abs(fd - ga[k]) < 1e-5 * np.abs(ga).max() + 1e-6 * abs(ga[k]), (model, s, q, fd, ga[k])
            k += 1
