"""TEST INFRASTRUCTURE shared by test_qoi_host.py and the GPU tests of the subdomain objectives: the host harness of the
product's per-point objective functions (tests/qoi_host/qoi_host.cpp).  The model rows, their meshes and their oracle states
are those of cauchy_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import cauchy_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
dp, ip = cc.dp, cc.ip
AVG_STRESS, AVG_LOCAL_VAR, DISP_COMP = 0, 1, 2  # C8_QOI_* of include/c8.h
REC = 13                                        # QOI_REC of c8_qoi_point.hpp
NDIMS = {3: 2, 4: 3, 8: 3}                      # by element type


def build_harness(out_dir):
    """compile the harness into out_dir and return its entry point"""
    so = os.path.join(str(out_dir), "libqoihost.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + cc.CXXFLAGS + ["-shared", "-o", so, os.path.join(HERE, "qoi_host", "qoi_host.cpp")])
    fn = C.CDLL(so).qoi_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, ip, dp, ip, dp, dp] + [dp] * 6 + [ip] + [dp] * 8
    return fn


class HostQoi:
    """the outputs of one harness call: value [e][pt], dxi [e][pt][nloc], rec [e][pt][13], dxe [e][pt][node][4] (du[3], dp),
    dparam [e][pt][nparams]; g, b0, b1 = the caller's arrays (or zeros) with the passes' subtractions applied"""


def host_qoi(fn, et, coords, conn, model, params, u, p, u_prev, p_prev, xi_prev, xi, qoi, elem_set=None, nn=None, g=None, b0=None, b1=None):
    d = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    coords, conn = d(coords), np.ascontiguousarray(conn, dtype=np.int32)
    params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, dtype=np.float64)))
    es = None if elem_set is None else np.ascontiguousarray(elem_set, dtype=np.int32)
    arrs = [d(a) for a in (nn, u, p, u_prev, p_prev, xi_prev, xi)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    xi = arrs[-1]
    ne, npts, nloc = xi.shape
    nnodes, nd = len(coords), NDIMS[et]
    o = HostQoi()
    o.value, o.dxi, o.rec = np.zeros((ne, npts)), np.zeros((ne, npts, nloc)), np.zeros((ne, npts, REC))
    o.dxe, o.dparam = np.zeros((ne, npts, conn.shape[1], 4)), np.zeros((ne, npts, params.shape[1]))
    o.g = np.zeros((ne, npts, nloc)) if g is None else np.array(g, dtype=np.float64).reshape(ne, npts, nloc)
    o.b0 = np.zeros(nnodes * nd) if b0 is None else np.array(b0, dtype=np.float64).ravel()
    o.b1 = np.zeros(nnodes) if b1 is None else np.array(b1, dtype=np.float64).ravel()
    q = np.array(qoi, dtype=np.int32)
    got = fn(model.encode(), et, ne, nnodes, conn.ctypes.data_as(ip), ptr(coords), None if es is None else es.ctypes.data_as(ip),
             ptr(params), *[ptr(a) for a in arrs], q.ctypes.data_as(ip),
             *[ptr(a) for a in (o.value, o.dxi, o.rec, o.dxe, o.dparam, o.g, o.b0, o.b1)])
    assert got == npts, (model, et, got, npts)
    return o


def case_qoi(fn, cs, qoi, **over):
    """host_qoi on a cauchy_cases.Case; `over`: u, p, xi, params replace the case's"""
    st = dict(zip(("u", "p", "u_prev", "p_prev", "xi_prev", "xi"), cs.state))
    params = over.pop("params", cs.params)
    kw = {k: over.pop(k) for k in ("elem_set", "g", "b0", "b1") if k in over}
    st.update(over)
    return host_qoi(fn, cs.et, cs.c, cs.conn, cs.model, params, st["u"], st["p"], st["u_prev"], st["p_prev"], st["xi_prev"], st["xi"],
                    qoi, nn=cs.nn, **kw)


def alpha_dof(cs):
    """flat position of the hardening variable in xi"""
    return cc.ALPHA.get(cs.model, cs.xi.shape[2] - 1)
