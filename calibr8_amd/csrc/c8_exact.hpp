// c8_exact.hpp -- eval_exact_errors (evaluations.cpp:1462-1654) and eval_linearization_errors (:1075-1266) at one
// integration point.  The reference builds six Jacobians per point by AD (dR/dx, dR/dxi, dC/dx, dC/dxi, dC/dx_prev,
// dC/dxi_prev) and multiplies each by one fixed direction, the fine state minus the stored one: that is a single
// Jacobian-vector product, and with the one-tangent Dual it is ONE evaluation of the model whose tangent part is
//   er_t = z . (dR/dx dx + dR/dxi dxi),   ec_t = phi . (dC/dx dx + dC/dxi dxi + dC/dx_prev dx_prev + dC/dxi_prev dxi_prev).
// The reference differentiates R along x and xi only (:1222, :1608).  One pass seeded in all four directions gives that
// as long as no model's global flux reads x_prev or xi_prev -- none does: cauchy(), hydro_cauchy(), pressure_scale_factor()
// and the plane-stress stretch xi[Z_STRETCH] of every row of the model table read grad u, p and xi alone (grad_u_prev and
// xi_prev appear in trial(), initial_guess() and evaluate() only; tests/test_exact_host.py pins it: E_R is exactly 0 along
// a direction that moves only x_prev and xi_prev).
// Lane and slot layout, PointTables and the staging are those of error_point (c8_error.hpp).  HIP-free.
#pragma once

#include "c8_error.hpp"

namespace c8 {

// nodal values of element nodes `node` into sh -- the stored state (DIFF false) or fine minus stored (DIFF true) --
// interpolated at the point
template <class E, bool PREV, bool DIFF>
C8_HD void exact_interpolate(PointTables<E>& sh, size_t const* node, FieldArgs const& fa, FieldArgs const& ff, int pt,
                             PointState<double>& g) {
  C8_UNROLL
  for (int n = 0; n < E::NN; ++n) {
    C8_UNROLL
    for (int i = 0; i < 3; ++i) {
      bool const in = i < E::DIM;
      size_t const q = node[n] * E::DIM + i;
      sh.u[n][i] = in ? (DIFF ? ff.u[q] - fa.u[q] : fa.u[q]) : 0.;
      if (PREV) sh.u_prev[n][i] = in ? (DIFF ? ff.u_prev[q] - fa.u_prev[q] : fa.u_prev[q]) : 0.;
    }
    sh.p[n] = (E::NRES == 2) ? (DIFF ? ff.p[node[n]] - fa.p[node[n]] : fa.p[node[n]]) : 0.;
  }
  interpolate_values<E, double, PREV>(sh, pt, g);
}

C8_HD void exact_pair(Tens3<Dual>& t, Tens3<double> const& v, Tens3<double> const& d) {
  t.xx = Dual(v.xx, d.xx); t.xy = Dual(v.xy, d.xy); t.xz = Dual(v.xz, d.xz);
  t.yx = Dual(v.yx, d.yx); t.yy = Dual(v.yy, d.yy); t.yz = Dual(v.yz, d.yz);
  t.zx = Dual(v.zx, d.zx); t.zy = Dual(v.zy, d.zy); t.zz = Dual(v.zz, d.zz);
}

// The tangent parts of evaluation `slot` of element e (slots and lanes as error_point): with the model evaluated at the
// stored state fa and every input carrying the tangent (fine state ff) - (stored state fa), formed here,
//   slot < NP0:   er_t = w dv d(Gu : grad z_u + Vp z_p + Gp . grad z_p),  ec_t = phi_pt . dC,
//                 er_same_t = the value of point slot of ip set 1 if error_shares_points<E>(), else 0
//   otherwise:    er_t = w dv d(flux_pressure) z_p  (tangent along dx: the pressure flux reads p alone),  ec_t = er_same_t = 0
// on the branch the model chooses from the VALUES (the reference's force_path is not supported).  Nodal u and p carry
// x_fine - x, u_prev (finite-deformation models) x_prev_fine - x_prev, m.xi and m.xi_prev the differences of the local
// states.  The value parts of the same evaluation are error_point's er, ec, er_same up to the rounding of Dual's
// division (a reciprocal and a product); exact_terms takes them from error_point itself.
template <class E, template <class> class ModelT>
C8_HD void exact_point(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, FieldArgs const& ff, ErrorArgs const& ea,
                       int e, int slot, double& er_t, double& ec_t, double& er_same_t) {
  using Model = ModelT<Dual>;
  constexpr int NL = Model::NLOC;
  constexpr bool PREV = Model::FINITE_DEF;
  bool const coupled = slot < E::NP0;
  int const ip_set = coupled ? 0 : 1, pt = coupled ? slot : slot - E::NP0;
  PointTables<E> sh;
  size_t node[E::NN];
  C8_UNROLL
  for (int n = 0; n < E::NN; ++n) {
    node[n] = (size_t)mt.conn[(size_t)e * E::NN + n];
    C8_UNROLL
    for (int i = 0; i < 3; ++i) sh.X[n][i] = (i < E::DIM) ? mt.coords[node[n] * 3 + i] : 0.;
  }
  shape_entry<E>(sh, ip_set, pt, 0, E::NN);
  double const h = elem_size<E>(sh);
  double zpv = 0., zpg[3] = {0., 0., 0.}, zg[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
  C8_UNROLL
  for (int n = 0; n < E::NN; ++n) {
    double const d0 = sh.dN[pt][n][0], d1 = sh.dN[pt][n][1], d2 = sh.dN[pt][n][2];
    if constexpr (E::NRES == 2) {
      double const zp = ea.z_p[node[n]];
      zpv += zp * sh.N[pt][n];
      zpg[0] += zp * d0; zpg[1] += zp * d1; zpg[2] += zp * d2;
    }
    if (coupled) {
      C8_UNROLL
      for (int i = 0; i < E::DIM; ++i) {
        double const zu = ea.z_u[node[n] * E::DIM + i];
        zg[i][0] += zu * d0; zg[i][1] += zu * d1; zg[i][2] += zu * d2;
      }
    }
  }
  Model m;
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  C8_UNROLL
  for (int q = 0; q < Model::NPARAMS; ++q) m.params[q] = Dual(mt.params[(size_t)es * Model::NPARAMS + q]);
  attach_embedded(m, mt);
  PointState<double> gv, gd;
  PointState<Dual> g;
  ec_t = 0.;
  er_same_t = 0.;
  if (!coupled) {
    if constexpr (E::NRES == 2) {
      exact_interpolate<E, false, false>(sh, node, fa, ff, pt, gv);
      exact_interpolate<E, false, true>(sh, node, fa, ff, pt, gd);
      g.p = Dual(gv.p, gd.p);
      er_t = Mechanics::flux_pressure(m, g).d * zpv * sh.wdv[pt];
    } else {
      er_t = 0.;
    }
    return;
  }
  exact_interpolate<E, PREV, false>(sh, node, fa, ff, pt, gv);
  exact_interpolate<E, PREV, true>(sh, node, fa, ff, pt, gd);
  C8_UNROLL
  for (int i = 0; i < 3; ++i) {
    g.u[i] = Dual(gv.u[i], gd.u[i]);
    g.grad_p[i] = Dual(gv.grad_p[i], gd.grad_p[i]);
  }
  g.p = Dual(gv.p, gd.p);
  exact_pair(g.grad_u, gv.grad_u, gd.grad_u);
  exact_pair(g.grad_u_prev, gv.grad_u_prev, gd.grad_u_prev);
  size_t const q0 = ((size_t)e * E::NP0 + pt) * NL;
  C8_UNROLL
  for (int j = 0; j < NL; ++j) {
    double const x = fa.xi[q0 + j], xp = fa.xi_prev[q0 + j];
    m.xi[j] = Dual(x, ff.xi[q0 + j] - x);
    m.xi_prev[j] = Dual(xp, ff.xi_prev[q0 + j] - xp);
    m.R[j] = Dual(0.);
  }
  {  // the global fluxes, contracted and freed before the local residual
    MechFlux<Dual> f;
    global_flux<E>(m, g, h, ms, f);
    double s = f.Vp.d * zpv + f.Gp[0].d * zpg[0] + f.Gp[1].d * zpg[1] + f.Gp[2].d * zpg[2];
    if constexpr (E::DIM == 3) {
      s += f.Gu.xx.d * zg[0][0] + f.Gu.xy.d * zg[0][1] + f.Gu.xz.d * zg[0][2];
      s += f.Gu.yx.d * zg[1][0] + f.Gu.yy.d * zg[1][1] + f.Gu.yz.d * zg[1][2];
      s += f.Gu.zx.d * zg[2][0] + f.Gu.zy.d * zg[2][1] + f.Gu.zz.d * zg[2][2];
    } else {
      s += f.Gu.xx.d * zg[0][0] + f.Gu.xy.d * zg[0][1];
      s += f.Gu.yx.d * zg[1][0] + f.Gu.yy.d * zg[1][1];
    }
    er_t = s * sh.wdv[pt];
  }
  if constexpr (error_shares_points<E>()) er_same_t = Mechanics::flux_pressure(m, g).d * zpv * sh.wdv[pt];
  m.evaluate(g, ms.abs_tol);
  double c = 0.;
  C8_UNROLL
  for (int j = 0; j < NL; ++j) c += ea.phi[q0 + j] * m.R[j].d;
  ec_t = c;
}

// What evaluation `slot` adds to an element's two sums, before the sign: the tangent parts (eval_exact_errors), or value
// plus tangent (LIN: eval_linearization_errors, R + dR -- the residual linearised about the stored state, at the fine
// one).  The values are error_point's own, bit for bit: with st_fine = st the linearization fields are the negated error
// contributions exactly, and lin + contributions = exact holds to the rounding of one addition per term.
template <class E, template <class> class ModelT, bool LIN>
C8_HD void exact_terms(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, FieldArgs const& ff, ErrorArgs const& ea,
                       int e, int slot, double& er, double& ec, double& er_same) {
  double tr, tc, ts;
  exact_point<E, ModelT>(mt, ms, fa, ff, ea, e, slot, tr, tc, ts);
  // the double pass second: three numbers are live across it, not the value pass's across the Dual one (the heavy hex8
  // rows keep 150 to 280 bytes a lane less in scratch this way round)
  double vr = 0., vc = 0., vs = 0.;
  if constexpr (LIN) error_point<E, ModelT>(mt, ms, fa, ea, e, slot, vr, vc, vs);
  er = LIN ? vr + tr : tr;
  ec = LIN ? vc + tc : tc;
  er_same = LIN ? vs + ts : ts;
}

}  // namespace c8
