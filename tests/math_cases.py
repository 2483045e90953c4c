"""Input families, independent references and error bars for calibr8_amd/csrc/c8_math.hpp, shared by
tests/test_dual_math_edges.py (the header on the CPU, through c8emu_math_op) and tests/test_gpu_dual_math.py (the header
on the device, through tests/math_device).  TEST INFRASTRUCTURE.

No reference here restates an algorithm of the header: scalar values are numpy float64, scalar derivatives are complex
steps (h = 1e-30) or written-out formulas, tensor algebra is numpy.linalg with the closed derivative formulas, the
eigen-decomposition is held to numpy.linalg.eigh and to order-free identities, the polar rotation to the SVD and a
Sylvester equation.

A family is a list of cases (operation number of tests/math_ops.hpp, 18 inputs, 18 tangents) and a check(out, dout,
where) that raises AssertionError; `where` is "cpu" or "device" and selects the value bar of the libm functions only.
Every check returns a dict of the largest error / bar ratios it saw, which the tests print."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEV_DIR = os.path.join(HERE, "math_device")
DEV_LIB = os.path.join(DEV_DIR, "libc8mathdev.so")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
EPS = float(np.finfo(np.float64).eps)
NIN, NOUT = 18, 21
H = 1e-30  # complex step

# operation numbers of tests/math_ops.hpp
_names = {0: "ADD SUB MUL DIV NEG ADD_DS ADD_SD SUB_DS SUB_SD MUL_DS MUL_SD DIV_DS DIV_SD IADD ISUB IADD_S ISUB_S",
          20: "RCP SQRT CBRT EXP LOG COS ACOS ABS POW",
          30: "DET COFACTOR INVERSE DEV NORM TRACE MATMUL TRANSPOSE DIFF2 DOT3",
          40: "EIG DYAD0 DYAD1 DYAD2 NORM1 NORMINF POLAR",
          50: "SYM6 PACK6 SYM_2 SYM_3 PACK_2 PACK_3 MSE_2 MSE_3 MSE_2S MSE_3S"}
OP = {n: base + k for base, names in _names.items() for k, n in enumerate(names.split())}

# ---------------------------------------------------------------------------
# The bars
# ---------------------------------------------------------------------------
# Well-conditioned scalar and tensor algebra: the bars of tests/test_dual_math.py.
VAL_REL = 1e-15   # values, relative
DER_REL = 1e-14   # derivatives, times max(1, |d|) (relative to |d| where a family says so: never wider)

# Device libm against numpy, in ulps of the numpy value.  The ROCm installation this was written on carries no accuracy
# table of its device library, so the count is what the reference itself needs: numpy float64 against numpy longdouble
# (x87 extended, 64-bit mantissa) on the inputs of the families below, rounded up to a whole ulp, times 4.  Measured
# (reference_ulps() repeats the measurement and the CPU test holds it to these counts): sqrt 0.28, cbrt 0.24, exp 0.33,
# log 0.49, cos 0.49, acos 0.52, pow 0.46 -- one ulp each.
REF_ULPS = {"SQRT": 1, "CBRT": 1, "EXP": 1, "LOG": 1, "COS": 1, "ACOS": 1, "POW": 1}
DEV_ULPS = {k: 4 * v for k, v in REF_ULPS.items()}

# c8_rcp: the header's own claim, "accurate to the last place": at most 1 ulp against the host's 1.0 / x.
RCP_ULPS = 1.0

# det, cofactor, inverse: K_ALG eps kappa(A).  No oracle run sets this one; by reasoning: an entry of the cofactor
# inverse goes through at most 10 roundings (2 x 2 minor, the 3-term determinant, the reciprocal and the product), each
# amplified by at most kappa, the LU of numpy.linalg has a bound of the same form with a constant of about 3 n = 9, and
# the derivative formulas apply the inverse twice: 32.
K_ALG = 32.0

# eig_spd_cos and polar_rotation: K eps (model), K = 8 x the largest ratio that the ORACLE's own eig_spd_cos /
# polar_rotation (oracle/c8_oracle.cpp through c8o_tensor_probe) needs on the inputs of the two families against the
# same references (oracle_constants() repeats the measurement); the 8 allows for another summation order and fused
# multiply-adds.  Written as (the oracle's ratio, rounded up) * 8.  Never taken from the emulator or the device.
K_EIG_VAL = 3.3 * 8      # sorted eigenvalues against eigh: eps |A|                             oracle: 3.29
K_EIG_ORTH = 2.3 * 8     # |V^T V - I| and | |det V| - 1 |: eps                                 oracle: 2.30
K_EIG_RES = 1.8 * 8      # |A V - V diag(D)|: eps |A|                                           oracle: 1.78
K_EIG_DLAM = 1.7 * 8     # d lambda_i = v_i^T dA v_i: eps |A| |dA| / gap                         oracle: 1.63
K_EIG_DIDENT = 1.6 * 8   # d(V diag(D) V^T) = dA: eps |A| |dA| / gap                            oracle: 1.55
K_POL_VAL = 2.9 * 8      # R against W Z^T of the SVD: eps |A|                                  oracle: 2.89
K_POL_DER = 1.1 * 8      # dR against the Sylvester equation: eps kappa(U) |dA| / sigma_min     oracle: 1.06
# what the two early returns of eig_spd_cos give away, by their own thresholds (shared with the reference algorithm):
# an off-diagonal part of Frobenius norm <= 2.22e-16 moves an eigenvalue by at most that much (Weyl), and J2 <= 1e-30
# bounds a deviatoric eigenvalue by sqrt(4 J2 / 3)
ABS_DIAG_RETURN = 2.220446049250313e-16
ABS_VOL_RETURN = math.sqrt(4e-30 / 3.0)
POLAR_STOP = 1.9611031010039037e-08  # sqrt(sqrt(3) eps): polar_rotation ends when a trip moves X by no more


def fro(a):
    """Frobenius norm, scaled so that entries near the ends of the exponent range neither overflow nor vanish"""
    a = np.asarray(a, dtype=np.float64)
    m = float(np.abs(a).max()) if a.size else 0.0
    if not (0.0 < m < np.inf):
        return m
    return m * float(np.sqrt(((a / m) ** 2).sum()))


def ulps(v, ref):
    """|v - ref| in units of the spacing of doubles at ref"""
    v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(v - ref) / np.spacing(np.abs(ref))


class Checker:
    """collects failures of one family and the largest error / bar ratio per kind of bar"""

    def __init__(self, family):
        self.family, self.fail, self.worst = family, [], {}

    def le(self, kind, case, err, bar):
        err = float(err)
        ok = err <= bar  # False for NaN
        if bar > 0 and np.isfinite(err):
            self.worst[kind] = max(self.worst.get(kind, 0.0), err / bar)
        elif not ok:
            self.worst[kind] = float("inf")
        if not ok:
            self.fail.append("%s[%s] %s: error %.3e > bar %.3e" % (self.family, case, kind, err, bar))

    def true(self, kind, case, cond, msg=""):
        if not cond:
            self.fail.append("%s[%s] %s %s" % (self.family, case, kind, msg))

    def done(self):
        assert not self.fail, "%d failures:\n" % len(self.fail) + "\n".join(self.fail[:40])
        return self.worst


class Family:
    def __init__(self, name, device_only=False):
        self.name, self.device_only = name, device_only
        self.ops, self.x, self.dx, self.meta = [], [], [], []
        # cases within 4 eps of a branch threshold of the header: the device and the emulator may decide differently
        # there, so their eigenvectors and tangents are not compared with each other (at most 5 % of a family)
        self.branch_free = []

    def add(self, op, x, dx=None, **meta):
        x = np.asarray(x, dtype=np.float64).ravel()
        dx = np.zeros_like(x) if dx is None else np.asarray(dx, dtype=np.float64).ravel()
        self.ops.append(OP[op] if isinstance(op, str) else op)
        self.x.append(np.concatenate([x, np.zeros(NIN - len(x))]))
        self.dx.append(np.concatenate([dx, np.zeros(NIN - len(dx))]))
        meta["op"] = op
        self.meta.append(meta)
        self.branch_free.append(not meta.get("straddles", False))
        return len(self.ops) - 1

    def arrays(self):
        return (np.array(self.ops, dtype=np.int32), np.ascontiguousarray(self.x, dtype=np.float64),
                np.ascontiguousarray(self.dx, dtype=np.float64))

    def __len__(self):
        return len(self.ops)


# ---------------------------------------------------------------------------
# Running a family
# ---------------------------------------------------------------------------
def run_emul(ops, x, dx):
    """the header on the CPU: tests/emul, c8emu_math_op, one call per operation number"""
    import emul_lib as em
    L = em.lib()
    L.c8emu_math_op.restype = C.c_int
    L.c8emu_math_op.argtypes = [C.c_int, dp, dp, C.c_int, dp, dp]
    out, dout = np.full((len(ops), NOUT), np.nan), np.full((len(ops), NOUT), np.nan)
    for op in sorted(set(int(o) for o in ops)):
        idx = np.nonzero(ops == op)[0]
        xi, dxi = np.ascontiguousarray(x[idx]), np.ascontiguousarray(dx[idx])
        o, do = np.zeros((len(idx), NOUT)), np.zeros((len(idx), NOUT))
        assert L.c8emu_math_op(op, xi.ctypes.data_as(dp), dxi.ctypes.data_as(dp), len(idx), o.ctypes.data_as(dp),
                               do.ctypes.data_as(dp)) == 0, op
        out[idx], dout[idx] = o, do
    return out, dout


def run_oracle(what, A, dA):
    """the oracle's eig_spd_cos (what = 0) / polar_rotation (what = 1): [n][3][3] -> V or R [n][3][3], D [n][3], tangents"""
    import oracle_lib as ol
    L = ol.lib()
    L.c8o_tensor_probe.restype = C.c_int
    L.c8o_tensor_probe.argtypes = [C.c_int, dp, dp, C.c_int, dp, dp]
    a, da = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 9), np.ascontiguousarray(dA, dtype=np.float64).reshape(-1, 9)
    out, dout = np.zeros((len(a), 12)), np.zeros((len(a), 12))
    assert L.c8o_tensor_probe(what, a.ctypes.data_as(dp), da.ctypes.data_as(dp), len(a), out.ctypes.data_as(dp),
                              dout.ctypes.data_as(dp)) == 0
    return out, dout


_dev = None


def device_lib():
    """tests/math_device/libc8mathdev.so; built once when it is missing (a failure of that build is an error)"""
    global _dev
    if _dev is None:
        if not os.path.exists(DEV_LIB):
            subprocess.check_call(["make", "-C", DEV_DIR, "-s"])
        L = C.CDLL(DEV_LIB)
        L.c8mathdev_run.restype = C.c_int
        L.c8mathdev_run.argtypes = [ip, dp, dp, C.c_int, dp, dp, ip]
        _dev = L
    return _dev


def run_device(ops, x, dx):
    """the header on the GPU: every case of the arrays in ONE launch, one lane per case"""
    L = device_lib()
    n = len(ops)
    ops, x, dx = np.ascontiguousarray(ops, dtype=np.int32), np.ascontiguousarray(x), np.ascontiguousarray(dx)
    out, dout, rc = np.full((n, NOUT), np.nan), np.full((n, NOUT), np.nan), np.full(n, -7, dtype=np.int32)
    err = L.c8mathdev_run(ops.ctypes.data_as(ip), x.ctypes.data_as(dp), dx.ctypes.data_as(dp), n, out.ctypes.data_as(dp),
                          dout.ctypes.data_as(dp), rc.ctypes.data_as(ip))
    assert err == 0, "HIP error %d" % err
    assert (rc > 0).all(), "unknown operation in cases %s" % np.nonzero(rc <= 0)[0][:10]
    return out, dout


# ---------------------------------------------------------------------------
# Helpers for the inputs
# ---------------------------------------------------------------------------
def rotation(rng):
    """a random proper rotation that is not aligned with any axis"""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def axis_rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def sym(a):
    return 0.5 * (a + a.T)


# ---------------------------------------------------------------------------
# Scalars
# ---------------------------------------------------------------------------
_BIN = {"ADD": lambda a, b: a + b, "SUB": lambda a, b: a - b, "MUL": lambda a, b: a * b, "DIV": lambda a, b: a / b,
        "NEG": lambda a, b: -a, "ADD_DS": lambda a, b: a + b, "ADD_SD": lambda a, b: a + b, "SUB_DS": lambda a, b: a - b,
        "SUB_SD": lambda a, b: a - b, "MUL_DS": lambda a, b: a * b, "MUL_SD": lambda a, b: a * b,
        "DIV_DS": lambda a, b: a / b, "DIV_SD": lambda a, b: a / b, "IADD": lambda a, b: a + b,
        "ISUB": lambda a, b: a - b, "IADD_S": lambda a, b: a + b, "ISUB_S": lambda a, b: a - b}


def _tangent_mask(op):
    """(first argument carries a tangent, second one does)"""
    if op.endswith("_DS") or op.endswith("_S"):
        return 1.0, 0.0
    if op.endswith("_SD"):
        return 0.0, 1.0
    return 1.0, 1.0


def _check_binary(fam, out, dout, where):
    ck = Checker(fam.name)
    for i, m in enumerate(fam.meta):
        a, b, da, db = fam.x[i][0], fam.x[i][1], fam.dx[i][0], fam.dx[i][1]
        f = _BIN[m["op"]]
        ref = f(a, b)
        cs = f(complex(a, H * da), complex(b, H * db)).imag / H
        ck.le("value", i, abs(out[i, 0] - ref), VAL_REL * abs(ref))
        ck.le("derivative", i, abs(dout[i, 0] - cs), DER_REL * max(1.0, abs(cs)))
    return ck.done()


def family_dual_ops():
    """every Dual operator overload on well-conditioned arguments of both signs"""
    fam = Family("dual_ops")
    rng = np.random.default_rng(101)
    for op in _BIN:
        ma, mb = _tangent_mask(op)
        for _ in range(20):
            a, b = rng.uniform(0.3, 2.5, 2) * rng.choice([-1.0, 1.0], 2)
            da, db = rng.standard_normal(2)
            fam.add(op, [a, b], [da * ma, db * mb])
    fam.check = lambda out, dout, where: _check_binary(fam, out, dout, where)
    return fam


def range_grid():
    """|x| from 2^-1000 to 2^1000 in steps of 2^50, mantissas 1, 1 + 2^-52, 2 - 2^-52, sqrt 2 and 1.5, both signs"""
    mant = [1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, math.sqrt(2.0), 1.5]
    return np.array([s * math.ldexp(m, e) for e in range(-1000, 1001, 50) for m in mant for s in (1.0, -1.0)])


def family_div_range():
    """c8_rcp and the three divisions over the whole exponent range.  The quotient is kept O(1) (numerator and both
    tangents scale with the denominator), so the existing bars (absolute below 1) bite."""
    fam = Family("div_range")
    rng = np.random.default_rng(102)
    # seeded random fill for c8_rcp: the mantissas of the grid are kind to a Newton iteration (a reciprocal with one step
    # fewer still rounds all of them correctly), random ones are not
    for _ in range(200):
        fam.add("RCP", [rng.choice([-1.0, 1.0]) * math.ldexp(rng.uniform(1.0, 2.0), int(rng.integers(-1000, 1001)))])
    for x in range_grid():
        fam.add("RCP", [x])
        for op in ("DIV", "DIV_DS", "DIV_SD"):
            ma, mb = (1.0, 1.0) if op == "DIV" else ((1.0, 0.0) if op == "DIV_DS" else (0.0, 1.0))
            q0, t1, t2 = rng.uniform(0.3, 2.5), rng.standard_normal(), rng.standard_normal()
            if op == "DIV_SD":  # double / Dual: the tangent of the quotient is -q db / b
                fam.add(op, [q0 * x, x], [0.0, x * t2])
            else:
                fam.add(op, [q0 * x, x], [x * t1 * ma, x * t2 * mb])

    def check(out, dout, where):
        ck = Checker(fam.name)
        worst_rcp = 0.0
        for i, m in enumerate(fam.meta):
            a, b, da, db = fam.x[i][0], fam.x[i][1], fam.dx[i][0], fam.dx[i][1]
            if m["op"] == "RCP":
                u = float(ulps(out[i, 0], 1.0 / a))
                worst_rcp = max(worst_rcp, u)
                ck.le("rcp_ulps", i, u, RCP_ULPS)
                continue
            ref = a / b
            # the quotient and its tangent do not change when numerator, denominator and both tangents are scaled by the
            # same power of two (exactly, in floating point too): the complex step is taken on the problem scaled to
            # O(1), where h = 1e-30 times a tangent neither underflows nor swamps the argument
            s = math.ldexp(1.0, -math.frexp(b)[1])
            cs = (complex(a * s, H * (da * s)) / complex(b * s, H * (db * s))).imag / H
            ck.le("value", i, abs(out[i, 0] - ref), VAL_REL * abs(ref))
            ck.le("derivative", i, abs(dout[i, 0] - cs), DER_REL * max(1.0, abs(cs)))
        w = ck.done()
        w["rcp_max_ulps"] = worst_rcp
        return w
    fam.check = check
    return fam


def family_rcp_special():
    """What c8_rcp documents for arguments without a finite reciprocal: NaN on the device (the CPU build divides and
    gives inf or 0).  Zeros, infinities, and the denormals whose reciprocal overflows."""
    fam = Family("rcp_special", device_only=True)
    for x in (0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, math.ldexp(1.0, -1030), -math.ldexp(1.5, -1026)):
        fam.add("RCP", [x])

    def check(out, dout, where):
        ck = Checker(fam.name)
        for i in range(len(fam)):
            ck.true("nan", i, np.isnan(out[i, 0]), "c8_rcp(%r) = %r, documented NaN" % (fam.x[i][0], out[i, 0]))
        return ck.done()
    fam.check = check
    return fam


_UNARY = {"SQRT": np.sqrt, "CBRT": lambda z: z ** (1.0 / 3.0) if isinstance(z, complex) else np.cbrt(z), "EXP": np.exp,
          "LOG": np.log, "COS": np.cos, "ACOS": np.arccos}


def unary_inputs():
    pts = {"SQRT": [1e-300, 1e-8, 1.0, 1e300], "CBRT": [1e-300, 1e-8, 1.0, 1e300], "LOG": [1e-300, 1e-8, 1.0, 1e300],
           "EXP": [-300.0, -1.0, 0.0, 1.0, 700.0],
           "ACOS": [1.0 - 2.0 ** -53, -(1.0 - 2.0 ** -53), 0.999999, -0.999999, 0.0, 0.5, -0.5],
           "COS": list(np.linspace(0.0, math.pi, 33))}  # the range of its one caller (theta / 3 (+ 2 pi / 3) in eig_spd_cos)
    return pts


def complex_step(op, a, da):
    """Im f(a + i h da) / h.  At 1e-300 the step h da underflows, and at 1e300 numpy's complex power loses digits to the
    size of the logarithm, so sqrt, cbrt and log are stepped at a 2^+-996 instead: scaling argument and tangent by
    2^996 (an even power and a cube, exact in floating point) scales the tangent of sqrt by 2^498, of cbrt by 2^332 and
    leaves that of log unchanged."""
    k = 0
    if op in ("SQRT", "CBRT", "LOG") and not 1e-200 < a < 1e200:
        k = 996 if a < 1.0 else -996
    z = complex(math.ldexp(a, k), H * math.ldexp(da, k))
    cs = complex(_UNARY[op](z)).imag / H
    return math.ldexp(cs, {"SQRT": -k // 2, "CBRT": -k // 3, "LOG": 0}.get(op, 0))


def pow_inputs():
    """(a, b, da, db).  Base 0; a negative base with a zero-tangent exponent; a zero-tangent base; the exponents 1, 2
    (von Mises), 8 and 100 of the Hosford / Barlat decks on stress-sized bases of both signs"""
    c = [(0.0, 2.0, 1.0, 0.5), (0.0, 0.5, -2.0, 0.0), (0.0, 8.0, 1.0, 1.0),
         (-1.7, 2.0, 0.8, 0.0), (-1.7, 3.0, -0.4, 0.0), (-250.0, 8.0, 1.3, 0.0),
         (1.7, 2.3, 0.0, 0.9), (0.4, 0.15, 0.0, -1.1), (250.0, 8.0, 0.0, 1.0)]
    for n in (1.0, 2.0, 8.0, 100.0):
        for a in (0.5, 1.3, 2.0, 250.0, -0.5, -250.0):
            c.append((a, n, 0.7, 0.0))
        c.append((1.3, n, 0.7, -0.3))
        c.append((250.0, n, -1.2, 0.01))
    return c


def pow_ref(a, b, da, db):
    """Sacado's rule as the header states it, written out: zero at a == 0, and only the terms of the operands that carry
    a tangent"""
    r = float(np.power(a, b))
    if a == 0.0:
        return r, 0.0, 0.0
    t1 = db * math.log(a) * r if db != 0.0 else 0.0
    t2 = b * da / a * r if da != 0.0 else 0.0
    return r, t1 + t2, abs(t1) + abs(t2)


def family_scalar_edges():
    """c8_sqrt, c8_cbrt, c8_exp, c8_log, c8_cos, c8_acos, c8_abs and c8_pow at their edges.  A tangent scales with its
    argument where the argument is tiny, so the complex step stays a small perturbation.  Derivative bars are relative
    to |d| (never wider than the existing 1e-14 max(1, |d|)); for c8_acos the bar carries the conditioning of the
    formula the header shares with Sacado, -1 / sqrt(1 - a a): rounding a a (at most eps / 4 below 1) moves the
    derivative by eps / (8 (1 - a^2)) relative, times 4."""
    fam = Family("scalar_edges")
    rng = np.random.default_rng(103)
    for op, pts in unary_inputs().items():
        for a in pts:
            t = float(rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0]))
            fam.add(op, [a], [a * t if op in ("SQRT", "CBRT", "LOG") else t])
    tiny = 5e-324
    for a in (0.0, -0.0, tiny, -tiny, 1e-300, -1e-300, 2.5, -2.5):
        fam.add("ABS", [a], [1.25])
    for a, b, da, db in pow_inputs():
        fam.add("POW", [a, b], [da, db])

    def check(out, dout, where):
        ck = Checker(fam.name)
        for i, m in enumerate(fam.meta):
            op, a, da = m["op"], fam.x[i][0], fam.dx[i][0]
            if op == "ABS":  # Sacado's rule: d|a| = +da for a >= 0, -0.0 included, and -da below
                ck.true("abs value", i, out[i, 0] == abs(a) and out[i, 1] == abs(a), "%r -> %r" % (a, out[i, :2]))
                ck.true("abs derivative", i, dout[i, 0] == (da if a >= 0.0 else -da), "%r -> %r" % (a, dout[i, 0]))
                continue
            if op == "POW":
                b, db = fam.x[i][1], fam.dx[i][1]
                ref, d, dscale = pow_ref(a, b, da, db)
                cs = d
            else:
                with np.errstate(all="ignore"):
                    ref = float(_UNARY[op](a))
                    cs = complex_step(op, a, da)
                dscale = abs(cs)
            for slot in (0, 1):  # the Dual and the double overload
                if where == "device":
                    ck.le("value_ulps_" + op, i, float(ulps(out[i, slot], ref)), DEV_ULPS[op])
                else:
                    ck.le("value", i, abs(out[i, slot] - ref), VAL_REL * abs(ref))
            rel = DER_REL
            if op == "ACOS":
                rel += EPS / (2.0 * (1.0 - a * a))
            ck.le("derivative", i, abs(dout[i, 0] - cs), rel * dscale)
            ck.true("finite", i, np.isfinite(dout[i, 0]))
        return ck.done()
    fam.check = check
    return fam


def reference_ulps():
    """what the numpy float64 reference itself needs: its distance from numpy longdouble on the inputs above, in ulps"""
    ld = np.longdouble
    fns = {"SQRT": np.sqrt, "CBRT": np.cbrt, "EXP": np.exp, "LOG": np.log, "COS": np.cos, "ACOS": np.arccos}
    worst = {}
    for op, pts in unary_inputs().items():
        x = np.array(pts, dtype=np.float64)
        hi = fns[op](x.astype(ld))
        lo = fns[op](x)
        nz = hi != 0
        u = np.abs((lo.astype(ld) - hi)[nz]) / np.spacing(np.abs(lo[nz])).astype(ld)
        worst[op] = float(u.max())
    p = np.array([(a, b) for a, b, _, _ in pow_inputs()])
    hi, lo = np.power(p[:, 0].astype(ld), p[:, 1].astype(ld)), np.power(p[:, 0], p[:, 1])
    nz = hi != 0
    worst["POW"] = float((np.abs((lo.astype(ld) - hi)[nz]) / np.spacing(np.abs(lo[nz])).astype(ld)).max())
    return worst


# ---------------------------------------------------------------------------
# Tensor algebra
# ---------------------------------------------------------------------------
def _perm_abs(A):
    a = np.abs(A)
    return sum(a[0, i] * a[1, j] * a[2, k] for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)))


def conditioned_matrices():
    """(label, A): conditioning 1, 1e4 and 1e8, a deformation gradient I + 1e-3 G, a reflection (det < 0), random fill"""
    rng = np.random.default_rng(104)
    mats = []
    for kappa in (1.0, 1e4, 1e8):
        for _ in range(2):
            s = np.array([1.0, kappa ** -0.5, 1.0 / kappa]) * rng.uniform(0.5, 2.0)
            mats.append(("kappa=%g" % kappa, rotation(rng) @ np.diag(s) @ rotation(rng).T))
    for _ in range(3):
        mats.append(("F=I+1e-3G", np.eye(3) + 1e-3 * rng.standard_normal((3, 3))))
    for _ in range(2):
        U = rotation(rng)
        mats.append(("reflection", np.diag([1.0, 1.0, -1.0]) @ rotation(rng) @ (U @ np.diag([0.7, 1.1, 1.6]) @ U.T)))
    for _ in range(5):
        mats.append(("random", rng.standard_normal((3, 3)) + 3.0 * np.eye(3)))
    return mats


def family_tensor_solve():
    """det, cofactor and inverse against numpy.linalg, with d det = det tr(A^-1 dA), d A^-1 = -A^-1 dA A^-1 and the
    cofactor as det A^-T.  The bar is the error model K_ALG eps kappa(A); for det itself, whose formula cancels, it is
    K_ALG eps times the sum of the absolute values of its six products."""
    fam = Family("tensor_solve")
    rng = np.random.default_rng(105)
    for label, A in conditioned_matrices():
        dA = rng.standard_normal((3, 3))
        for op in ("DET", "COFACTOR", "INVERSE"):
            fam.add(op, A, dA, label=label)

    def check(out, dout, where):
        ck = Checker(fam.name)
        for i, m in enumerate(fam.meta):
            A, dA = fam.x[i][:9].reshape(3, 3), fam.dx[i][:9].reshape(3, 3)
            inv, dt, kappa = np.linalg.inv(A), float(np.linalg.det(A)), float(np.linalg.cond(A))
            dinv = -inv @ dA @ inv
            ddt = dt * np.trace(inv @ dA)
            tag = "%d:%s" % (i, m["label"])
            if m["op"] == "DET":
                ck.true("sign", tag, (out[i, 0] < 0) == (dt < 0))
                ck.le("det", tag, abs(out[i, 0] - dt), K_ALG * EPS * _perm_abs(A))
                ck.le("d det", tag, abs(dout[i, 0] - ddt), K_ALG * EPS * kappa * abs(dt) * fro(inv) * fro(dA))
            elif m["op"] == "COFACTOR":
                ref, dref = dt * inv.T, ddt * inv.T + dt * dinv.T
                ck.le("cofactor", tag, fro(out[i, :9].reshape(3, 3) - ref), K_ALG * EPS * kappa * fro(ref))
                ck.le("d cofactor", tag, fro(dout[i, :9].reshape(3, 3) - dref), K_ALG * EPS * kappa * abs(dt) * fro(inv) ** 2 * fro(dA))
            else:
                ck.le("inverse", tag, fro(out[i, :9].reshape(3, 3) - inv), K_ALG * EPS * kappa * fro(inv))
                ck.le("d inverse", tag, fro(dout[i, :9].reshape(3, 3) - dinv), K_ALG * EPS * kappa * fro(inv) ** 2 * fro(dA))
        return ck.done()
    fam.check = check
    return fam


def family_tensor_algebra():
    """dev, norm, trace, matmul, transpose, diff2, dot3, add_dyad_col, norm_1, norm_infinity and the packing helpers on
    well-conditioned random tensors: the existing bars (1e-15 on values, 1e-14 max(1, .) on derivatives), relative to
    the sum of the absolute values of the terms where an operation adds products.  The two max-norms are also run where
    their selects decide: two equal column / row sums (the first one wins) and zero entries (d|0| = +d0)."""
    fam = Family("tensor_algebra")
    rng = np.random.default_rng(106)

    def rt():
        return rng.standard_normal((3, 3)) + rng.choice([0.0, 2.0]) * np.eye(3)

    for _ in range(5):
        for op in ("DEV", "NORM", "TRACE", "TRANSPOSE", "NORM1", "NORMINF"):
            fam.add(op, rt(), rng.standard_normal((3, 3)))
        fam.add("MATMUL", np.concatenate([rt().ravel(), rt().ravel()]), rng.standard_normal(18))
        fam.add("DIFF2", rng.standard_normal(4), rng.standard_normal(4))
        fam.add("DOT3", rng.standard_normal(6), rng.standard_normal(6))
        for c in range(3):
            x, dx = np.zeros(18), np.zeros(18)
            x[:7], dx[:7] = rng.standard_normal(7), rng.standard_normal(7)
            x[9:], dx[9:] = rotation(rng).ravel(), rng.standard_normal(9)
            fam.add("DYAD%d" % c, x, dx)
        for op, n in (("SYM6", 6), ("SYM_3", 6), ("SYM_2", 3)):
            fam.add(op, rng.standard_normal(n), rng.standard_normal(n))
        for op in ("PACK6", "PACK_3", "PACK_2"):
            fam.add(op, sym(rt()), sym(rng.standard_normal((3, 3))))
        for op in ("MSE_2", "MSE_3", "MSE_2S", "MSE_3S"):
            fam.add(op, np.concatenate([rt().ravel(), rng.standard_normal(1)]), rng.standard_normal(10))
    tie = np.array([[1.0, -2.0, 0.5], [-2.0, 1.0, 0.5], [0.0, 0.0, 0.0]])  # columns 0 and 1, rows 0 and 1 tie at 3
    for op in ("NORM1", "NORMINF"):
        fam.add(op, tie, rng.standard_normal((3, 3)))
        fam.add(op, tie.T, rng.standard_normal((3, 3)))
        fam.add(op, np.zeros((3, 3)), rng.standard_normal((3, 3)))

    def max_norm(A, dA, axis):
        """largest absolute column (axis 0) or row (axis 1) sum; the first of equal sums; d|a| = +da at a == 0"""
        s = np.abs(A).sum(axis=axis)
        k = int(np.argmax(s))  # first occurrence
        sg = np.where(A >= 0.0, 1.0, -1.0)
        return s[k], (sg * dA).sum(axis=axis)[k], np.abs(dA).sum(axis=axis)[k]

    def check(out, dout, where):
        ck = Checker(fam.name)
        for i, m in enumerate(fam.meta):
            op, x, dx = m["op"], fam.x[i], fam.dx[i]
            A, dA = x[:9].reshape(3, 3), dx[:9].reshape(3, 3)
            o9, do9 = out[i, :9].reshape(3, 3), dout[i, :9].reshape(3, 3)

            def pair(ref, dref, scale=None, dscale=None, got=None, dgot=None):
                ref, dref = np.asarray(ref, dtype=np.float64), np.asarray(dref, dtype=np.float64)
                g = (o9 if ref.ndim == 2 else out[i, 0]) if got is None else got
                dg = (do9 if ref.ndim == 2 else dout[i, 0]) if dgot is None else dgot
                ck.le(op, i, fro(g - ref), VAL_REL * (fro(ref) if scale is None else scale))
                ck.le("d " + op, i, fro(dg - dref), DER_REL * max(1.0, fro(dref) if dscale is None else dscale))

            if op == "DEV":
                pair(A - np.trace(A) / 3.0 * np.eye(3), dA - np.trace(dA) / 3.0 * np.eye(3), scale=fro(A))
            elif op == "NORM":
                pair(np.linalg.norm(A), (A * dA).sum() / np.linalg.norm(A))
            elif op == "TRACE":
                pair(np.trace(A), np.trace(dA), scale=np.abs(np.diag(A)).sum())
            elif op == "TRANSPOSE":
                ck.true(op, i, (o9 == A.T).all() and (do9 == dA.T).all())
            elif op in ("NORM1", "NORMINF"):
                v, d, ds = max_norm(A, dA, 0 if op == "NORM1" else 1)
                assert v == np.linalg.norm(A, 1 if op == "NORM1" else np.inf)
                pair(v, d, dscale=ds)
            elif op == "MATMUL":
                B, dB = x[9:].reshape(3, 3), dx[9:].reshape(3, 3)
                pair(A @ B, dA @ B + A @ dB, scale=fro(np.abs(A) @ np.abs(B)), dscale=fro(np.abs(dA) @ np.abs(B) + np.abs(A) @ np.abs(dB)))
            elif op == "DIFF2":
                ref, dref = x[0] * x[1] - x[2] * x[3], x[0] * dx[1] + dx[0] * x[1] - x[2] * dx[3] - dx[2] * x[3]
                sc = abs(x[0] * x[1]) + abs(x[2] * x[3])
                pair(ref, dref, scale=sc)
                ck.le(op + " double", i, abs(out[i, 1] - ref), VAL_REL * sc)
            elif op == "DOT3":
                a, b, da, db = x[0:6:2], x[1:6:2], dx[0:6:2], dx[1:6:2]
                pair(a @ b, da @ b + a @ db, scale=np.abs(a) @ np.abs(b))
                ck.le(op + " double", i, abs(out[i, 1] - a @ b), VAL_REL * (np.abs(a) @ np.abs(b)))
            elif op.startswith("DYAD"):
                c = int(op[4])
                s, ds = x[:6], dx[:6]
                S = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
                dS = np.array([[ds[0], ds[1], ds[2]], [ds[1], ds[3], ds[4]], [ds[2], ds[4], ds[5]]])
                w, dw, v, dv = x[6], dx[6], x[9:].reshape(3, 3)[:, c], dx[9:].reshape(3, 3)[:, c]
                pair(S + w * np.outer(v, v), dS + dw * np.outer(v, v) + w * (np.outer(dv, v) + np.outer(v, dv)),
                     scale=fro(np.abs(S) + abs(w) * np.outer(np.abs(v), np.abs(v))))
            elif op in ("SYM6", "SYM_3", "SYM_2"):
                def unpack(s):
                    if op == "SYM_2":
                        return np.array([[s[0], s[1], 0.0], [s[1], s[2], 0.0], [0.0, 0.0, 0.0]])
                    return np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
                ck.true(op, i, (o9 == unpack(x)).all() and (do9 == unpack(dx)).all())
            elif op in ("PACK6", "PACK_3", "PACK_2"):
                def pack(t):
                    return [t[0, 0], t[0, 1], t[1, 1], 0.0, 0.0, 0.0] if op == "PACK_2" else [t[0, 0], t[0, 1], t[0, 2], t[1, 1], t[1, 2], t[2, 2]]
                ck.true(op, i, (out[i, :6] == pack(A)).all() and (dout[i, :6] == pack(dA)).all())
            elif op.startswith("MSE"):
                I = np.diag([1.0, 1.0, 1.0 if "3" in op else 0.0])
                ds = 0.0 if op.endswith("S") else dx[9]
                ck.true(op, i, (o9 == A - x[9] * I).all() and (do9 == dA - ds * I).all())
            else:
                raise AssertionError(op)
        return ck.done()
    fam.check = check
    return fam


# ---------------------------------------------------------------------------
# eig_spd_cos
# ---------------------------------------------------------------------------
def eig_cases():
    """(label, A, kind, delta).  kind: "full" (every assertion), "diag" (the diagonal early return: V = I, values and
    d lambda only), "vol" (the volumetric return: values only), "repeated" (delta = 0: values and A V = V D only)"""
    rng = np.random.default_rng(107)
    cases = []
    # exactly diagonal, and an off-diagonal part of Frobenius norm 1e-16, 2e-16 (returned as diagonal), 3e-16 and 1e-12
    # (the full algorithm): both sides of the 2.22e-16 early return, at tensor scale 1 and 1e3
    for scale in (1.0, 1e3):
        d = np.array([0.7, -1.2, 1.9]) * scale
        cases.append(("diag scale=%g" % scale, np.diag(d), "diag", None))
        cases.append(("diag scale=%g unsorted" % scale, np.diag(d[[2, 0, 1]]), "diag", None))
        for off in (1e-16, 2e-16, 3e-16, 1e-12):
            o = rng.standard_normal(3)
            o *= off / (math.sqrt(2.0) * np.linalg.norm(o))  # each entry counts twice in the Frobenius norm
            A = np.diag(d) + np.array([[0, o[0], o[1]], [o[0], 0, o[2]], [o[1], o[2], 0]])
            cases.append(("off=%g scale=%g" % (off, scale), A, "diag" if off < 2.2e-16 else "full", None))
    # the volumetric tensor (taken by the diagonal return) and J2 on both sides of 1e-30 behind that return: J2 is the
    # square of the off-diagonal entry here
    cases.append(("volumetric", 1.3 * np.eye(3), "vol", None))
    for c in (0.0, 1.0):
        for xy, kind in ((5e-16, "vol"), (7e-16, "vol"), (1.5e-15, "full"), (3e-15, "full")):
            A = c * np.eye(3)
            A[0, 1] = A[1, 0] = xy
            cases.append(("J2=%.1e c=%g" % (xy * xy, c), A, kind, None))
    # well-separated random symmetric tensors
    for scale in (1e-3, 1.0, 1e3):
        for _ in range(8):
            lam = np.array([-1.3, 0.2, 1.9]) * rng.uniform(0.7, 1.4, 3) * scale
            Q = rotation(rng)
            cases.append(("random scale=%g" % scale, sym(Q @ np.diag(lam) @ Q.T), "full", None))
    # rotated diag(a, a, b) and diag(a, b, b) with a relative gap delta between the close pair; delta = 0 is the uniaxial
    # stress of a tension test
    for delta in (1e-2, 1e-4, 1e-6, 1e-8):
        for _ in range(5):
            Q = rotation(rng)
            a, b = rng.uniform(0.8, 1.2), rng.uniform(2.0, 3.0)
            cases.append(("aab delta=%g" % delta, sym(Q @ np.diag([a, a * (1 + delta), b]) @ Q.T), "full", delta))
            Q = rotation(rng)
            cases.append(("abb delta=%g" % delta, sym(Q @ np.diag([a, b, b * (1 + delta)]) @ Q.T), "full", delta))
    Q = rotation(rng)
    cases.append(("aab delta=0", sym(Q @ np.diag([0.0, 0.0, 250.0]) @ Q.T), "repeated", 0.0))
    Q = rotation(rng)
    cases.append(("abb delta=0", sym(Q @ np.diag([-1.0, 2.5, 2.5]) @ Q.T), "repeated", 0.0))
    return cases


def eig_errors(A, dA, V, D, dV, dD):
    """the order-free error measures of one decomposition against numpy.linalg.eigh, each divided by its model"""
    w, Q = np.linalg.eigh(A)
    nA, ndA = fro(A), fro(dA)
    gap = float(min(w[1] - w[0], w[2] - w[1]))
    o = np.argsort(D)
    e = {"val": np.abs(D[o] - w).max() / EPS,   # / |A| by the caller (with the allowance of the early returns)
         "orth": max(fro(V.T @ V - np.eye(3)), abs(abs(np.linalg.det(V)) - 1.0)) / EPS,
         "res": fro(A @ V - V * D) / (EPS * nA) if nA > 0 else fro(A @ V - V * D)}
    if gap > 0:
        dlam = np.array([Q[:, k] @ dA @ Q[:, k] for k in range(3)])
        model = EPS * nA * ndA / gap
        e["dlam"] = np.abs(dD[o] - dlam).max() / model
        ident = dV @ np.diag(D) @ V.T + V @ np.diag(dD) @ V.T + V @ np.diag(D) @ dV.T
        e["dident"] = fro(ident - dA) / model
    return e


def family_eig():
    """eig_spd_cos against numpy.linalg.eigh, order-free.

    At an exactly repeated eigenvalue (delta = 0, the uniaxial stress state) the derivative of an eigenvalue of the pair
    is not defined and the algorithm promises nothing.  Observed, not asserted (printed by both tests): the tangents of
    both delta = 0 cases are finite, on the CPU and on an MI355X.  det V is recorded per case and printed as counts:
    -1 wherever the full algorithm ran (v1 = v0 x v2), +1 where an early return gave V = I."""
    fam = Family("eig")
    rng = np.random.default_rng(108)
    for label, A, kind, delta in eig_cases():
        dA = sym(rng.standard_normal((3, 3))) * max(fro(A), 1e-15) / 1.7
        # delta = 0: pivots and the 2 x 2 problem decide between equal candidates, the basis of the plane is arbitrary
        fam.add("EIG", A, dA, label=label, kind=kind, delta=delta, straddles=(kind == "repeated"))

    def check(out, dout, where):
        ck = Checker(fam.name)
        notes = {}
        for i, m in enumerate(fam.meta):
            A, dA = fam.x[i][:9].reshape(3, 3), fam.dx[i][:9].reshape(3, 3)
            V, dV, D, dD = out[i, :9].reshape(3, 3), dout[i, :9].reshape(3, 3), out[i, 9:12], dout[i, 9:12]
            kind, tag = m["kind"], "%d:%s" % (i, m["label"])
            ck.true("finite values", tag, np.isfinite(V).all() and np.isfinite(D).all())
            if not (np.isfinite(V).all() and np.isfinite(D).all()):
                continue
            e = eig_errors(A, dA, V, D, dV, dD)
            allow = {"diag": ABS_DIAG_RETURN, "vol": ABS_VOL_RETURN}.get(kind, 0.0)
            ck.le("eigenvalues", tag, e["val"] * EPS, K_EIG_VAL * EPS * fro(A) + allow)
            ck.le("V^T V = I, |det V| = 1", tag, e["orth"], K_EIG_ORTH)
            notes.setdefault("det V = %+d" % round(float(np.linalg.det(V))), []).append(i)
            if kind in ("diag", "vol"):
                ck.true("early return gives V = I", tag, (V == np.eye(3)).all())
            if kind in ("full", "repeated"):
                ck.le("A V = V D", tag, e["res"], K_EIG_RES)
            if kind == "repeated":
                notes.setdefault("delta = 0 tangents finite" if np.isfinite(dV).all() and np.isfinite(dD).all()
                                 else "delta = 0 tangents NOT finite", []).append(i)
                continue
            ck.true("finite tangents", tag, np.isfinite(dV).all() and np.isfinite(dD).all())
            if kind == "vol":
                continue
            ck.le("d lambda", tag, e["dlam"], K_EIG_DLAM)
            if kind == "full":
                ck.le("d(V D V^T) = dA", tag, e["dident"], K_EIG_DIDENT)
        w = ck.done()
        w.update({k: len(v) for k, v in notes.items()})
        return w
    fam.check = check
    return fam


# ---------------------------------------------------------------------------
# polar_rotation
# ---------------------------------------------------------------------------
def polar_cases():
    rng = np.random.default_rng(109)
    cases = []
    for kappa in (1.0, 10.0, 100.0, 1e3):  # R U, kappa(U) from 1 to 1e3
        for _ in range(4):
            Q = rotation(rng)
            s = np.array([kappa ** 0.5, rng.uniform(kappa ** -0.5, kappa ** 0.5), kappa ** -0.5])
            cases.append(("RU kappa=%g" % kappa, rotation(rng) @ (Q @ np.diag(s) @ Q.T)))
    for _ in range(4):
        cases.append(("pure rotation", rotation(rng)))
    for _ in range(3):
        Q = rotation(rng)
        cases.append(("pure stretch", sym(Q @ np.diag(rng.uniform(0.5, 2.0, 3)) @ Q.T)))
    cases.append(("identity", np.eye(3)))
    for _ in range(4):
        cases.append(("I+1e-8G", np.eye(3) + 1e-8 * rng.standard_normal((3, 3))))
    for ang in (math.pi - 1e-3, math.pi - 1e-8, math.pi, math.pi + 1e-3):
        Q = rotation(rng)
        cases.append(("angle=pi%+.0e" % (ang - math.pi), axis_rotation(rng.standard_normal(3), ang) @ (Q @ np.diag([0.8, 1.0, 1.3]) @ Q.T)))
        cases.append(("angle=pi%+.0e, no stretch" % (ang - math.pi), axis_rotation(rng.standard_normal(3), ang)))
    return cases


def polar_reference(A, dA):
    """R = W Z^T of A = W S Z^T; dR = R Om with U Om + Om U = R^T dA - dA^T R, U = R^T A, solved as a 3 x 3 system in
    the three entries of the skew Om"""
    W, S, Zt = np.linalg.svd(A)
    R = W @ Zt
    U = R.T @ A
    rhs = R.T @ dA - dA.T @ R
    basis = []
    for (p, q) in ((0, 1), (0, 2), (1, 2)):
        E = np.zeros((3, 3))
        E[p, q], E[q, p] = 1.0, -1.0
        basis.append(E)
    pick = lambda M: np.array([M[0, 1], M[0, 2], M[1, 2]])
    M = np.column_stack([pick(U @ E + E @ U) for E in basis])
    om = np.linalg.solve(M, pick(rhs))
    Om = sum(c * E for c, E in zip(om, basis))
    return R, R @ Om, float(S.max() / S.min()), float(S.min())


def polar_errors(A, dA, R, dR):
    """error / (eps model) of the value and of the tangent.  The tangent is allowed what the stopping rule of the
    iteration gives away: it ends on VALUES, when a trip moves X by no more than 1.96e-8.  For an input A = R (I + E)
    with |E| below that, the first trip ends it: X1 = R (I + E^2 / 2 + ...) is R to rounding, but its tangent still
    carries d(E^2 / 2) = (E dE + dE E) / 2, at most |E| |dA| -- the tangent is one trip behind the value.  Allowed:
    2 |E| |dA| where |E| <= 2 x 1.96e-8 (a case just above the threshold takes a second trip and needs none of it)."""
    Rr, dRr, kappa, smin = polar_reference(A, dA)
    E = fro(Rr.T @ A - np.eye(3))
    trunc = 2.0 * E * fro(dA) if E <= 2.0 * POLAR_STOP else 0.0
    return {"val": fro(R - Rr) / (EPS * fro(A)), "der": max(fro(dR - dRr) - trunc, 0.0) / (EPS * kappa * fro(dA) / smin),
            "der_raw": fro(dR - dRr) / (EPS * kappa * fro(dA) / smin)}


def family_polar():
    """polar_rotation against the SVD and the Sylvester equation.  The trip count of its iteration is not visible
    through the header's interface; a pure rotation, which ends it in the first trip, is held to the same value bar."""
    fam = Family("polar")
    rng = np.random.default_rng(110)
    for label, A in polar_cases():
        fam.add("POLAR", A, rng.standard_normal((3, 3)), label=label)

    def check(out, dout, where):
        ck = Checker(fam.name)
        for i, m in enumerate(fam.meta):
            A, dA = fam.x[i][:9].reshape(3, 3), fam.dx[i][:9].reshape(3, 3)
            R, dR = out[i, :9].reshape(3, 3), dout[i, :9].reshape(3, 3)
            tag = "%d:%s" % (i, m["label"])
            ck.true("finite", tag, np.isfinite(R).all() and np.isfinite(dR).all())
            e = polar_errors(A, dA, R, dR)
            ck.le("R", tag, e["val"], K_POL_VAL)
            ck.le("dR", tag, e["der"], K_POL_DER)
        return ck.done()
    fam.check = check
    return fam


def oracle_constants():
    """the ratios error / (eps model) that the oracle's own eig_spd_cos and polar_rotation need on the inputs of the two
    families: the first factor of each K above"""
    fe, fp = family_eig(), family_polar()
    worst = {}
    A, dA = np.array([x[:9] for x in fe.x]).reshape(-1, 3, 3), np.array([x[:9] for x in fe.dx]).reshape(-1, 3, 3)
    out, dout = run_oracle(0, A, dA)
    for i, m in enumerate(fe.meta):
        V, dV, D, dD = out[i, :9].reshape(3, 3), dout[i, :9].reshape(3, 3), out[i, 9:12], dout[i, 9:12]
        e = eig_errors(A[i], dA[i], V, D, dV, dD)
        kind = m["kind"]
        allow = {"diag": ABS_DIAG_RETURN, "vol": ABS_VOL_RETURN}.get(kind, 0.0)
        use = {"K_EIG_VAL": max(e["val"] * EPS - allow, 0.0) / (EPS * fro(A[i])) if fro(A[i]) > 0 else 0.0, "K_EIG_ORTH": e["orth"]}
        if kind in ("full", "repeated"):
            use["K_EIG_RES"] = e["res"]
        if kind in ("full", "diag"):
            use["K_EIG_DLAM"] = e["dlam"]
        if kind == "full":
            use["K_EIG_DIDENT"] = e["dident"]
        for k, v in use.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    A, dA = np.array([x[:9] for x in fp.x]).reshape(-1, 3, 3), np.array([x[:9] for x in fp.dx]).reshape(-1, 3, 3)
    out, dout = run_oracle(1, A, dA)
    for i in range(len(fp)):
        e = polar_errors(A[i], dA[i], out[i, :9].reshape(3, 3), dout[i, :9].reshape(3, 3))
        worst["K_POL_VAL"] = max(worst.get("K_POL_VAL", 0.0), e["val"])
        worst["K_POL_DER"] = max(worst.get("K_POL_DER", 0.0), e["der"])
    return worst


def all_families():
    return [family_dual_ops(), family_div_range(), family_rcp_special(), family_scalar_edges(), family_tensor_solve(),
            family_tensor_algebra(), family_eig(), family_polar()]


def agreement(fam, a, da, b, db):
    """The device (a, da) against the emulator (b, db), case by case, on the cases whose branch decisions cannot differ.
    Both run the same operations in the same order; they differ by fused multiply-adds, the device libm (ulps) and
    c8_rcp (one ulp), and a cancellation amplifies those like any other rounding.  So the distance allowed is the error
    model of the operation, with the constants used against the reference:
      eig_spd_cos     values eps |A| (eigenvectors: / the relative gap), tangents eps |A| |dA| / gap / the relative gap
      polar_rotation  eps |A| and eps kappa(U) |dA| / sigma_min
      det, cofactor, inverse   K_ALG eps kappa(A)
      everything else 1e-13 of the size of the case's results and of its tangents (10 x the derivative bar), with
                      c8_acos widened by the conditioning of 1 - a a as against the reference
    and the same entries are NaN on both sides.  On a case that is not branch-free only the eigenvalues are compared.
    Returns the list of failures."""
    fails = []
    for i, m in enumerate(fam.meta):
        op = m["op"]
        x9, dx9 = fam.x[i][:9].reshape(3, 3), fam.dx[i][:9].reshape(3, 3)
        if not fam.branch_free[i]:
            assert op == "EIG"
            if not np.abs(np.sort(a[i, 9:12]) - np.sort(b[i, 9:12])).max() <= K_EIG_VAL * EPS * fro(x9):
                fails.append((fam.name, i, "eigenvalues"))
            continue
        if ((np.isnan(a[i]) | np.isnan(da[i])) != (np.isnan(b[i]) | np.isnan(db[i]))).any():
            fails.append((fam.name, i, "NaN pattern"))
            continue
        dv, dd = fro(a[i] - b[i]), fro(da[i] - db[i])
        if op == "EIG":
            w = np.linalg.eigh(x9)[0]
            full = m["kind"] == "full"
            relgap = min(1.0, float(min(w[1] - w[0], w[2] - w[1])) / fro(x9)) if full else 1.0
            vbar = max(K_EIG_VAL, K_EIG_ORTH) * EPS * max(fro(x9), 1.0) / relgap
            dbar = K_EIG_DIDENT * EPS * max(fro(x9), 1.0) * fro(dx9) / (relgap * fro(x9)) / relgap if full else K_EIG_DLAM * EPS * fro(dx9)
        elif op == "POLAR":
            sv = np.linalg.svd(x9)[1]
            vbar, dbar = K_POL_VAL * EPS * fro(x9), K_POL_DER * EPS * (sv.max() / sv.min()) * fro(dx9) / sv.min()
        else:
            rel = 1e-13
            if op in ("DET", "COFACTOR", "INVERSE"):
                rel = K_ALG * EPS * float(np.linalg.cond(x9))
            if op == "ACOS":
                rel += EPS / (2.0 * (1.0 - fam.x[i][0] ** 2))
            vbar = K_ALG * EPS * _perm_abs(x9) if op == "DET" else rel * fro(b[i])
            # a tangent that is a sum of products can cancel: its size is then that of the tangents that went in
            dbar = rel * max(fro(db[i]), fro(fam.dx[i]) if op in ("MATMUL", "DOT3", "DIFF2") else 0.0)
            if op == "DET":
                dbar = rel * abs(b[i, 0]) * fro(np.linalg.inv(x9)) * fro(dx9)
        if not dv <= vbar:
            fails.append((fam.name, i, m.get("label", op), "values differ by %.3e > %.3e" % (dv, vbar)))
        if not dd <= dbar:
            fails.append((fam.name, i, m.get("label", op), "tangents differ by %.3e > %.3e" % (dd, dbar)))
    return fails
