// c8_qoi_point.hpp -- the subdomain objectives (avg_stress.cpp, avg_local_var.cpp, disp_comp.cpp): value and partial
// derivatives of the integrand at one local-state point, from the stored state.  No local solve and no element vector:
// like cauchy_point (c8_cauchy.hpp), whose PointTables it shares, it is written for ONE lane per (element, point).  HIP-free:
// the kernels (c8_qoi_point.hip) and the host harness of the tests (tests/qoi_host) compile these same functions.
//
//   kind                   value of a point of the chosen element set       depends on
//   C8_QOI_AVG_STRESS      w dv |dev_cauchy(g)|_F over the DIM x DIM block  grad u, p (through the PointState), xi, params
//   C8_QOI_AVG_LOCAL_VAR   w dv xi[index]                                   xi[index]
//   C8_QOI_DISP_COMP       w dv u[index]                                    u[index]
//
// A point of another element set has value 0 and derivative 0.  |D| is not differentiable at D = 0 (the reference's
// derivative is 0/0 there): such a point has value 0 and derivative 0 here (include/c8.h).
//
// The integrand depends on the nodal values only through the PointState, so its x-derivative at a point is the record
//   rec[0..8] = dq/d(grad u) row-major, rec[9] = dq/dp, rec[10..12] = dq/du
// (QOI_REC doubles; the out-of-plane entries of a 2-D element and rec[9] under one residual are 0), and
//   dq/du_a[i] = sum_j rec[3 i + j] dN_a/dx_j + rec[10 + i] N_a,   dq/dp_a = rec[9] N_a
// for node a of the element (qoi_node_contract).  The derivatives are partial: x unseeded while xi is seeded and the other
// way round, as K3 takes them (c8_assemble_adjoint.hpp).
#pragma once

#include "../../include/c8.h"  // C8_QOI_*
#include "c8_cauchy.hpp"

namespace c8 {

constexpr int QOI_REC = 13;

struct SubdomainQoi {
  int kind, elem_set, index;  // c8_subdomain_qoi_desc
};

// what a point's evaluations read: the interpolated state, w dv, the set's parameters and the point's local state
template <template <class> class ModelT> struct QoiPoint {
  PointState<double> g;
  double wdv;
  double params[ModelT<double>::NPARAMS];
  double xi[ModelT<double>::NLOC];
};

template <class E, template <class> class ModelT>
C8_HD void qoi_point_load(MeshTables const& mt, FieldArgs const& fa, int e, int pt, QoiPoint<ModelT>& d) {
  using Model = ModelT<double>;
  constexpr bool PREV = Model::FINITE_DEF;
  PointTables<E> sh;
  C8_UNROLL
  for (int n = 0; n < E::NN; ++n) {
    size_t const node = (size_t)mt.conn[(size_t)e * E::NN + n];
    C8_UNROLL
    for (int i = 0; i < 3; ++i) {
      bool const in = i < E::DIM;  // 2-D: the out-of-plane entries of the 3-wide containers are zero
      sh.X[n][i] = in ? mt.coords[node * 3 + i] : 0.;
      sh.u[n][i] = in ? fa.u[node * E::DIM + i] : 0.;
      if (PREV) sh.u_prev[n][i] = in ? fa.u_prev[node * E::DIM + i] : 0.;
    }
    sh.p[n] = (E::NRES == 2) ? fa.p[node] : 0.;
  }
  shape_entry<E>(sh, 0, pt, 0, E::NN);
  interpolate_values<E, double, PREV>(sh, pt, d.g);
  d.wdv = sh.wdv[pt];
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  C8_UNROLL
  for (int q = 0; q < Model::NPARAMS; ++q) d.params[q] = mt.params[(size_t)es * Model::NPARAMS + q];
  size_t const q0 = ((size_t)e * E::NP0 + pt) * Model::NLOC;
  C8_UNROLL
  for (int j = 0; j < Model::NLOC; ++j) d.xi[j] = fa.xi[q0 + j];
}

C8_HD bool qoi_in_set(MeshTables const& mt, SubdomainQoi const& sq, int e) { return (mt.elem_set ? mt.elem_set[e] : 0) == sq.elem_set; }

// |D|_F over the DIM x DIM block and its tangent D : dD / |D|; both 0 at D = 0
template <int DIM> C8_HD void qoi_block_norm(Tens3<Dual> const& D, double& v, double& d) {
  double n2 = D.xx.v * D.xx.v + D.xy.v * D.xy.v + D.yx.v * D.yx.v + D.yy.v * D.yy.v;
  double dd = D.xx.v * D.xx.d + D.xy.v * D.xy.d + D.yx.v * D.yx.d + D.yy.v * D.yy.d;
  if (DIM == 3) {
    n2 += D.xz.v * D.xz.v + D.yz.v * D.yz.v + D.zx.v * D.zx.v + D.zy.v * D.zy.v + D.zz.v * D.zz.v;
    dd += D.xz.v * D.xz.d + D.yz.v * D.yz.d + D.zx.v * D.zx.d + D.zy.v * D.zy.d + D.zz.v * D.zz.d;
  }
  v = sqrt(n2);
  d = (v > 0.) ? dd / v : 0.;
}
template <int DIM> C8_HD double qoi_block_norm(Tens3<double> const& D) {
  double n2 = D.xx * D.xx + D.xy * D.xy + D.yx * D.yx + D.yy * D.yy;
  if (DIM == 3) n2 += D.xz * D.xz + D.yz * D.yz + D.zx * D.zx + D.zy * D.zy + D.zz * D.zz;
  return sqrt(n2);
}

C8_HD void qoi_lift(Tens3<double> const& a, Tens3<Dual>& b) {
  b.xx = Dual(a.xx); b.xy = Dual(a.xy); b.xz = Dual(a.xz);
  b.yx = Dual(a.yx); b.yy = Dual(a.yy); b.yz = Dual(a.yz);
  b.zx = Dual(a.zx); b.zy = Dual(a.zy); b.zz = Dual(a.zz);
}

// the value of the point (the caller has checked the element set)
template <class E, template <class> class ModelT>
C8_HD double qoi_point_value(MeshTables const& mt, SubdomainQoi const& sq, QoiPoint<ModelT> const& d) {
  using Model = ModelT<double>;
  if (sq.kind == C8_QOI_AVG_LOCAL_VAR) {
    double v = 0.;
    C8_UNROLL
    for (int j = 0; j < Model::NLOC; ++j) v = (j == sq.index) ? d.xi[j] : v;
    return d.wdv * v;
  }
  if (sq.kind == C8_QOI_DISP_COMP) return d.wdv * (sq.index == 0 ? d.g.u[0] : (sq.index == 1 ? d.g.u[1] : d.g.u[2]));
  Model m;
  C8_UNROLL
  for (int q = 0; q < Model::NPARAMS; ++q) m.params[q] = d.params[q];
  attach_embedded(m, mt);
  C8_UNROLL
  for (int j = 0; j < Model::NLOC; ++j) m.xi[j] = d.xi[j];
  return d.wdv * qoi_block_norm<E::DIM>(m.dev_cauchy(d.g));
}

// d(w dv |dev_cauchy|) along ONE direction: tx in [0, 10) seeds entry tx of (grad u row-major, p), txi in [0, NLOC) seeds
// xi[txi], tp in [0, NPARAMS) seeds parameter tp; -1 seeds nothing of that group.  One evaluation of ModelT<Dual>::dev_cauchy.
template <class E, template <class> class ModelT>
C8_HD double qoi_stress_tangent(MeshTables const& mt, QoiPoint<ModelT> const& d, int tx, int txi, int tp) {
  using Model = ModelT<Dual>;
  Model m;
  C8_UNROLL
  for (int q = 0; q < Model::NPARAMS; ++q) m.params[q] = Dual(d.params[q], (q == tp) ? 1. : 0.);
  attach_embedded(m, mt);
  C8_UNROLL
  for (int j = 0; j < Model::NLOC; ++j) m.xi[j] = Dual(d.xi[j], (j == txi) ? 1. : 0.);
  PointState<Dual> g;
  C8_UNROLL
  for (int i = 0; i < 3; ++i) { g.u[i] = Dual(d.g.u[i]); g.grad_p[i] = Dual(d.g.grad_p[i]); }
  g.p = Dual(d.g.p, (tx == 9) ? 1. : 0.);
  qoi_lift(d.g.grad_u, g.grad_u);
  qoi_lift(d.g.grad_u_prev, g.grad_u_prev);
  g.grad_u.xx.d = (tx == 0) ? 1. : 0.; g.grad_u.xy.d = (tx == 1) ? 1. : 0.; g.grad_u.xz.d = (tx == 2) ? 1. : 0.;
  g.grad_u.yx.d = (tx == 3) ? 1. : 0.; g.grad_u.yy.d = (tx == 4) ? 1. : 0.; g.grad_u.yz.d = (tx == 5) ? 1. : 0.;
  g.grad_u.zx.d = (tx == 6) ? 1. : 0.; g.grad_u.zy.d = (tx == 7) ? 1. : 0.; g.grad_u.zz.d = (tx == 8) ? 1. : 0.;
  double v, dv;
  qoi_block_norm<E::DIM>(m.dev_cauchy(g), v, dv);
  return d.wdv * dv;
}

// entry t of the x-record: zero where the element has no such unknown
template <class E, template <class> class ModelT>
C8_HD double qoi_point_dx(MeshTables const& mt, SubdomainQoi const& sq, QoiPoint<ModelT> const& d, int t) {
  if (sq.kind == C8_QOI_DISP_COMP) return (t == 10 + sq.index) ? d.wdv : 0.;
  if (sq.kind != C8_QOI_AVG_STRESS || t > 9) return 0.;
  if (t == 9 ? E::NRES == 1 : (t / 3 >= E::DIM || t % 3 >= E::DIM)) return 0.;
  return qoi_stress_tangent<E, ModelT>(mt, d, t, -1, -1);
}
template <class E, template <class> class ModelT>
C8_HD double qoi_point_dxi(MeshTables const& mt, SubdomainQoi const& sq, QoiPoint<ModelT> const& d, int j) {
  if (sq.kind == C8_QOI_AVG_LOCAL_VAR) return (j == sq.index) ? d.wdv : 0.;
  if (sq.kind != C8_QOI_AVG_STRESS) return 0.;
  return qoi_stress_tangent<E, ModelT>(mt, d, -1, j, -1);
}
template <class E, template <class> class ModelT>
C8_HD double qoi_point_dparam(MeshTables const& mt, SubdomainQoi const& sq, QoiPoint<ModelT> const& d, int q) {
  if (sq.kind != C8_QOI_AVG_STRESS) return 0.;
  return qoi_stress_tangent<E, ModelT>(mt, d, -1, -1, q);
}

// N_a and grad N_a of ONE node at ONE point, in the member layout shape_entry (c8_assemble.hpp) writes: both indices ignored
template <class E> struct NodeAtPoint {
  double X[E::NN][3];
  AtPoint<AtPoint<double>> N;
  AtPoint<AtPoint<double[3]>> dN;
  AtPoint<double> wdv;
};

// the record of a point contracted with node a of its element: du[i] = dq/du_a[i] (i < DIM), dp = dq/dp_a
template <class E> C8_HD void qoi_node_contract(NodeAtPoint<E>& sh, int pt, int a, double const* rec, double du[3], double& dp) {
  shape_entry<E>(sh, 0, pt, a, a + 1);
  double const N = sh.N[pt][a], *dN = sh.dN[pt][a];
  C8_UNROLL
  for (int i = 0; i < 3; ++i) du[i] = rec[3 * i] * dN[0] + rec[3 * i + 1] * dN[1] + rec[3 * i + 2] * dN[2] + rec[10 + i] * N;
  dp = rec[9] * N;
}

}  // namespace c8
