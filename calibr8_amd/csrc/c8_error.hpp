// c8_error.hpp -- eval_error_contributions (evaluations.cpp:930-1073): the adjoint-weighted residuals of one integration
// point, from the stored state.  No local solve, no AD: the global residual's point fluxes contracted with the interpolated
// adjoint z, and the local model's residual C contracted with the local adjoint phi.  Written for ONE lane per (element,
// point), as cauchy_point is (c8_cauchy.hpp), whose PointTables it shares.  HIP-free: the kernel
// (c8_error.hip) and the host harness of the tests compile this same function.
#pragma once

#include "c8_cauchy.hpp"

namespace c8 {

// the global adjoint solution, as c8_solve_adjoint_local takes it, and the local one
struct ErrorArgs {
  double const* z_u;  // [nnodes][DIM]
  double const* z_p;  // [nnodes]; not read under mechanics_plane_stress (one residual)
  double const* phi;  // [nelems][NP0][NLOC]
};

// values of an element: one per point of ip set 0, then one per point of ip set 1 (E_R and E_C are summed in this order)
template <class E> constexpr int error_slots() { return E::NP0 + (E::NSETS == 2 ? E::NP1 : 0); }
// ... and the evaluations that produce them: where the two ip sets have the same points (hex8), the evaluation of point pt of
// set 0 has N, w dv, p and z_p of point pt of set 1 in hand and returns that point's value as well
template <class E> constexpr bool error_shares_points() { return E::NSETS == 2 && E::SAME_POINTS; }
template <class E> constexpr int error_lanes() { return error_shares_points<E>() ? E::NP0 : error_slots<E>(); }

// Evaluation `slot` of element e:
//   slot < NP0 (point slot of ip set 0):   er = w dv (Gu : grad z_u + Vp z_p + Gp . grad z_p),  ec = phi_pt . C(x, xi, xi_prev),
//                                          er_same = the value of point slot of ip set 1 if error_shares_points<E>(), else 0
//   otherwise (point slot - NP0 of set 1): er = w dv flux_pressure z_p,  ec = 0,  er_same = 0
// with z interpolated by the element's shape functions; the fluxes are those of residual_element (K2), so that the sum of er
// over an element's points is z_e . R_e.  C is the model's evaluate() on the branch the model itself chooses; a model whose
// evaluate() fills nothing (elastic) gives ec = 0.
template <class E, template <class> class ModelT>
C8_HD void error_point(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, ErrorArgs const& ea, int e, int slot,
                       double& er, double& ec, double& er_same) {
  using Model = ModelT<double>;
  constexpr int NL = Model::NLOC;
  constexpr bool PREV = Model::FINITE_DEF;
  bool const coupled = slot < E::NP0;
  int const ip_set = coupled ? 0 : 1, pt = coupled ? slot : slot - E::NP0;
  // in stages, each of which leaves a few numbers behind and frees the nodal values it read (a lane has no shared tables to
  // park them in): geometry -> shape functions and element size; z -> its value and gradients; u, p -> the point state
  PointTables<E> sh;
  size_t node[E::NN];
  C8_UNROLL
  for (int n = 0; n < E::NN; ++n) {
    node[n] = (size_t)mt.conn[(size_t)e * E::NN + n];
    C8_UNROLL
    for (int i = 0; i < 3; ++i) sh.X[n][i] = (i < E::DIM) ? mt.coords[node[n] * 3 + i] : 0.;  // 2-D: out-of-plane entries are zero
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
  C8_UNROLL
  for (int n = 0; n < E::NN; ++n) {
    C8_UNROLL
    for (int i = 0; i < 3; ++i) {
      bool const in = i < E::DIM;
      sh.u[n][i] = in ? fa.u[node[n] * E::DIM + i] : 0.;
      if (PREV) sh.u_prev[n][i] = in ? fa.u_prev[node[n] * E::DIM + i] : 0.;
    }
    sh.p[n] = (E::NRES == 2) ? fa.p[node[n]] : 0.;
  }
  Model m;
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  C8_UNROLL
  for (int q = 0; q < Model::NPARAMS; ++q) m.params[q] = mt.params[(size_t)es * Model::NPARAMS + q];
  attach_embedded(m, mt);
  PointState<double> g;
  ec = 0.;
  er_same = 0.;
  if (!coupled) {
    if constexpr (E::NRES == 2) {
      interpolate_values<E, double, false>(sh, pt, g);
      er = Mechanics::flux_pressure(m, g) * zpv * sh.wdv[pt];
    } else {
      er = 0.;
    }
    return;
  }
  interpolate_values<E, double, PREV>(sh, pt, g);
  size_t const q0 = ((size_t)e * E::NP0 + pt) * NL;
  C8_UNROLL
  for (int j = 0; j < NL; ++j) {
    m.xi[j] = fa.xi[q0 + j];
    m.xi_prev[j] = fa.xi_prev[q0 + j];
    m.R[j] = 0.;
  }
  MechFlux<double> f;
  global_flux<E>(m, g, h, ms, f);
  double s = f.Vp * zpv + f.Gp[0] * zpg[0] + f.Gp[1] * zpg[1] + f.Gp[2] * zpg[2];
  if constexpr (E::DIM == 3) {
    s += f.Gu.xx * zg[0][0] + f.Gu.xy * zg[0][1] + f.Gu.xz * zg[0][2];
    s += f.Gu.yx * zg[1][0] + f.Gu.yy * zg[1][1] + f.Gu.yz * zg[1][2];
    s += f.Gu.zx * zg[2][0] + f.Gu.zy * zg[2][1] + f.Gu.zz * zg[2][2];
  } else {  // the in-plane block: the element has no out-of-plane rows
    s += f.Gu.xx * zg[0][0] + f.Gu.xy * zg[0][1];
    s += f.Gu.yx * zg[1][0] + f.Gu.yy * zg[1][1];
  }
  er = s * sh.wdv[pt];
  if constexpr (error_shares_points<E>()) er_same = Mechanics::flux_pressure(m, g) * zpv * sh.wdv[pt];
  m.evaluate(g, ms.abs_tol);
  double c = 0.;
  C8_UNROLL
  for (int j = 0; j < NL; ++j) c += ea.phi[q0 + j] * m.R[j];
  ec = c;
}

}  // namespace c8
