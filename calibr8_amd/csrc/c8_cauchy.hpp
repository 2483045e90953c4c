// c8_cauchy.hpp -- eval_cauchy (evaluations.cpp:1659-1748): the local model's Cauchy stress at one local-state point,
// from the stored state.  No local solve, no AD, no element vector: the whole evaluation belongs to one point, so it is
// written for ONE lane per (element, point) pair instead of the lane groups of c8_assemble.hpp.  HIP-free: the kernel
// (c8_cauchy.hip) and the host harness of the tests compile this same function.
#pragma once

#include "c8_assemble.hpp"

namespace c8 {

// a model whose cauchy() reads the previous local state says so with `static constexpr bool CAUCHY_READS_XI_PREV = true`
// (none of the present models does: they form the stress from xi and the interpolated global state alone)
template <class M, class = void> struct cauchy_reads_xi_prev : std::false_type {};
template <class M> struct cauchy_reads_xi_prev<M, std::enable_if_t<M::CAUCHY_READS_XI_PREV>> : std::true_type {};

// The nodal data and the shape table of ONE point, in the member layout that shape_entry and interpolate_values
// (c8_assemble.hpp) read from the group-shared tables: the point index they subscript with is ignored, so the lane keeps
// one point's N, dN/dx and w dv in registers and no array is indexed by a run-time value.
template <class T> struct AtPoint {
  T v;
  C8_HD T& operator[](int) { return v; }
  C8_HD T const& operator[](int) const { return v; }
};
template <class E> struct PointTables {
  double X[E::NN][3];
  double u[E::NN][3], p[E::NN];
  double u_prev[E::NN][3];
  AtPoint<double[E::NN]> N;
  AtPoint<double[E::NN][3]> dN;
  AtPoint<double> wdv;
};

// sigma of point pt (ip set 0: the points of the local-state field) of element e, row-major 3 x 3 into out9; the entries
// with a row or column index >= E::DIM are 0 (the reference fills an apf::Matrix3x3 over ndims x ndims).  Connectivity,
// coordinates and nodal values are read straight from the global arrays; the local state is that of the real point pt
// (as K2 does, c8_assemble_adjoint.hpp).  Under mechanics_plane_stress (E::NRES == 1) fa.p is not read; fa.u_prev only
// by the finite-deformation models; fa.p_prev never.
template <class E, template <class> class ModelT>
C8_HD void cauchy_point(MeshTables const& mt, ModelSettings const&, FieldArgs const& fa, int e, int pt, double* out9) {
  using Model = ModelT<double>;
  constexpr int NL = Model::NLOC;
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
  PointState<double> g;
  interpolate_values<E, double, PREV>(sh, pt, g);
  Model m;
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  C8_UNROLL
  for (int q = 0; q < Model::NPARAMS; ++q) m.params[q] = mt.params[(size_t)es * Model::NPARAMS + q];
  attach_embedded(m, mt);
  size_t const q0 = ((size_t)e * E::NP0 + pt) * NL;
  C8_UNROLL
  for (int j = 0; j < NL; ++j) m.xi[j] = fa.xi[q0 + j];
  if constexpr (cauchy_reads_xi_prev<Model>::value) {
    C8_UNROLL
    for (int j = 0; j < NL; ++j) m.xi_prev[j] = fa.xi_prev[q0 + j];
  }
  Tens3<double> const s = m.cauchy(g);
  constexpr bool D3 = E::DIM == 3;
  out9[0] = s.xx; out9[1] = s.xy; out9[2] = D3 ? s.xz : 0.;
  out9[3] = s.yx; out9[4] = s.yy; out9[5] = D3 ? s.yz : 0.;
  out9[6] = D3 ? s.zx : 0.; out9[7] = D3 ? s.zy : 0.; out9[8] = D3 ? s.zz : 0.;
}

}  // namespace c8
