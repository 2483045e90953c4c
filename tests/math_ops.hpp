// math_ops.hpp -- one table of the operations of calibr8_amd/csrc/c8_math.hpp, callable by number (TEST INFRASTRUCTURE).
//
// The CPU hook (tests/emul/c8_emul.cpp, c8emu_math_op) and the device harness (tests/math_device/math_device.hip)
// compile this same table, so both run the same call of the header on the same layout:
//
//   in[18], din[18]    values and tangents of the arguments: scalars in the leading slots, a tensor as nine slots in
//                      row order (xx xy xz yx yy yz zx zy zz), a second tensor from slot 9
//   out[21], dout[21]  values and tangents of the results, in the same orders; slots an operation does not write are 0
//
// Returns the number of result slots, -1 for an unknown operation.  tests/math_cases.py holds the same numbers.
#pragma once

#include "../calibr8_amd/csrc/c8_math.hpp"

namespace c8_math_ops {

enum {
  MO_NIN = 18,
  MO_NOUT = 21,
  // Dual operators
  MO_ADD = 0, MO_SUB, MO_MUL, MO_DIV, MO_NEG, MO_ADD_DS, MO_ADD_SD, MO_SUB_DS, MO_SUB_SD, MO_MUL_DS, MO_MUL_SD, MO_DIV_DS,
  MO_DIV_SD, MO_IADD, MO_ISUB, MO_IADD_S, MO_ISUB_S,
  // scalar functions
  MO_RCP = 20, MO_SQRT, MO_CBRT, MO_EXP, MO_LOG, MO_COS, MO_ACOS, MO_ABS, MO_POW,
  // tensor algebra
  MO_DET = 30, MO_COFACTOR, MO_INVERSE, MO_DEV, MO_NORM, MO_TRACE, MO_MATMUL, MO_TRANSPOSE, MO_DIFF2, MO_DOT3,
  // eigen-decomposition and polar decomposition
  MO_EIG = 40, MO_DYAD0, MO_DYAD1, MO_DYAD2, MO_NORM1, MO_NORMINF, MO_POLAR,
  // packing
  MO_SYM6 = 50, MO_PACK6, MO_SYM_2, MO_SYM_3, MO_PACK_2, MO_PACK_3, MO_MSE_2, MO_MSE_3, MO_MSE_2S, MO_MSE_3S
};

using c8::Dual;
using c8::Tens3;

C8_HD Tens3<Dual> mo_tens(double const* in, double const* din) {
  Tens3<Dual> t;
  t.xx = Dual(in[0], din[0]); t.xy = Dual(in[1], din[1]); t.xz = Dual(in[2], din[2]);
  t.yx = Dual(in[3], din[3]); t.yy = Dual(in[4], din[4]); t.yz = Dual(in[5], din[5]);
  t.zx = Dual(in[6], din[6]); t.zy = Dual(in[7], din[7]); t.zz = Dual(in[8], din[8]);
  return t;
}
C8_HD void mo_put(Dual const& x, double* out, double* dout) { *out = x.v; *dout = x.d; }
C8_HD int mo_put_tens(Tens3<Dual> const& t, double* out, double* dout) {
  mo_put(t.xx, out + 0, dout + 0); mo_put(t.xy, out + 1, dout + 1); mo_put(t.xz, out + 2, dout + 2);
  mo_put(t.yx, out + 3, dout + 3); mo_put(t.yy, out + 4, dout + 4); mo_put(t.yz, out + 5, dout + 5);
  mo_put(t.zx, out + 6, dout + 6); mo_put(t.zy, out + 7, dout + 7); mo_put(t.zz, out + 8, dout + 8);
  return 9;
}

C8_HD int math_op(int op, double const* in, double const* din, double* out, double* dout) {
  using namespace c8;
  for (int k = 0; k < MO_NOUT; ++k) { out[k] = 0.; dout[k] = 0.; }
  Dual const a(in[0], din[0]), b(in[1], din[1]);
  Dual r(0.);
  switch (op) {
    case MO_ADD: r = a + b; break;
    case MO_SUB: r = a - b; break;
    case MO_MUL: r = a * b; break;
    case MO_DIV: r = a / b; break;
    case MO_NEG: r = -a; break;
    case MO_ADD_DS: r = a + in[1]; break;
    case MO_ADD_SD: r = in[0] + b; break;
    case MO_SUB_DS: r = a - in[1]; break;
    case MO_SUB_SD: r = in[0] - b; break;
    case MO_MUL_DS: r = a * in[1]; break;
    case MO_MUL_SD: r = in[0] * b; break;
    case MO_DIV_DS: r = a / in[1]; break;
    case MO_DIV_SD: r = in[0] / b; break;
    case MO_IADD: r = a; r += b; break;
    case MO_ISUB: r = a; r -= b; break;
    case MO_IADD_S: r = a; r += in[1]; break;
    case MO_ISUB_S: r = a; r -= in[1]; break;
    case MO_RCP: r = Dual(c8_rcp(in[0])); break;
    // the scalar functions: slot 0 the Dual overload, slot 1 the double overload
    case MO_SQRT: mo_put(c8_sqrt(a), out, dout); out[1] = c8_sqrt(in[0]); return 2;
    case MO_CBRT: mo_put(c8_cbrt(a), out, dout); out[1] = c8_cbrt(in[0]); return 2;
    case MO_EXP: mo_put(c8_exp(a), out, dout); out[1] = c8_exp(in[0]); return 2;
    case MO_LOG: mo_put(c8_log(a), out, dout); out[1] = c8_log(in[0]); return 2;
    case MO_COS: mo_put(c8_cos(a), out, dout); out[1] = c8_cos(in[0]); return 2;
    case MO_ACOS: mo_put(c8_acos(a), out, dout); out[1] = c8_acos(in[0]); return 2;
    case MO_ABS: mo_put(c8_abs(a), out, dout); out[1] = c8_abs(in[0]); return 2;
    case MO_POW: mo_put(c8_pow(a, b), out, dout); out[1] = c8_pow(in[0], in[1]); return 2;
    case MO_DET: r = det(mo_tens(in, din)); break;
    case MO_COFACTOR: return mo_put_tens(cofactor(mo_tens(in, din)), out, dout);
    case MO_INVERSE: return mo_put_tens(inverse(mo_tens(in, din)), out, dout);
    case MO_DEV: return mo_put_tens(dev(mo_tens(in, din)), out, dout);
    case MO_NORM: r = norm(mo_tens(in, din)); break;
    case MO_TRACE: r = trace(mo_tens(in, din)); break;
    case MO_MATMUL: return mo_put_tens(matmul(mo_tens(in, din), mo_tens(in + 9, din + 9)), out, dout);
    case MO_TRANSPOSE: return mo_put_tens(transpose(mo_tens(in, din)), out, dout);
    case MO_DIFF2: {  // slot 0 the Dual overload, slot 1 the double overload
      mo_put(diff2(a, b, Dual(in[2], din[2]), Dual(in[3], din[3])), out, dout);
      out[1] = diff2(in[0], in[1], in[2], in[3]);
      return 2;
    }
    case MO_DOT3: {
      mo_put(dot3(a, b, Dual(in[2], din[2]), Dual(in[3], din[3]), Dual(in[4], din[4]), Dual(in[5], din[5])), out, dout);
      out[1] = dot3(in[0], in[1], in[2], in[3], in[4], in[5]);
      return 2;
    }
    case MO_EIG: {  // V in slots 0..8, D in slots 9..11
      Tens3<Dual> V;
      Dual D[3];
      eig_spd_cos(mo_tens(in, din), V, D);
      mo_put_tens(V, out, dout);
      mo_put(D[0], out + 9, dout + 9); mo_put(D[1], out + 10, dout + 10); mo_put(D[2], out + 11, dout + 11);
      return 12;
    }
    case MO_DYAD0: case MO_DYAD1: case MO_DYAD2: {  // S = sym6(slots 0..5), w = slot 6, V = slots 9..17
      Dual s[6];
      for (int k = 0; k < 6; ++k) s[k] = Dual(in[k], din[k]);
      Tens3<Dual> S = sym6(s);
      add_dyad_col(S, Dual(in[6], din[6]), mo_tens(in + 9, din + 9), op - MO_DYAD0);
      return mo_put_tens(S, out, dout);
    }
    case MO_NORM1: r = norm_1(mo_tens(in, din)); break;
    case MO_NORMINF: r = norm_infinity(mo_tens(in, din)); break;
    case MO_POLAR: return mo_put_tens(polar_rotation(mo_tens(in, din)), out, dout);
    case MO_SYM6: case MO_SYM_2: case MO_SYM_3: {
      Dual s[6];
      for (int k = 0; k < 6; ++k) s[k] = Dual(in[k], din[k]);
      return mo_put_tens(op == MO_SYM6 ? sym6(s) : op == MO_SYM_2 ? sym_dim<2>(s) : sym_dim<3>(s), out, dout);
    }
    case MO_PACK6: case MO_PACK_2: case MO_PACK_3: {
      Dual s[6];
      for (int k = 0; k < 6; ++k) s[k] = Dual(0.);
      Tens3<Dual> const t = mo_tens(in, din);
      if (op == MO_PACK6) pack_sym6(t, s);
      else if (op == MO_PACK_2) pack_sym_dim<2>(t, s);
      else pack_sym_dim<3>(t, s);
      for (int k = 0; k < 6; ++k) mo_put(s[k], out + k, dout + k);
      return op == MO_PACK_2 ? 3 : 6;
    }
    // A - s I with s in slot 9: a Dual (MSE_2, MSE_3) or a double (MSE_2S, MSE_3S)
    case MO_MSE_2: return mo_put_tens(minus_s_eye<2>(mo_tens(in, din), Dual(in[9], din[9])), out, dout);
    case MO_MSE_3: return mo_put_tens(minus_s_eye<3>(mo_tens(in, din), Dual(in[9], din[9])), out, dout);
    case MO_MSE_2S: return mo_put_tens(minus_s_eye<2>(mo_tens(in, din), in[9]), out, dout);
    case MO_MSE_3S: return mo_put_tens(minus_s_eye<3>(mo_tens(in, din), in[9]), out, dout);
    default: return -1;
  }
  mo_put(r, out, dout);
  return 1;
}

}  // namespace c8_math_ops
