// tests/qoi_host/qoi_host.cpp -- TEST INFRASTRUCTURE.
//
// The product's subdomain objectives (calibr8_amd/csrc/c8_qoi_point.hpp) compiled for the CPU: per-point values and partial
// derivatives, and the four sums the device kernels form from them (J, g, b, grad), the sums over a node's elements in the
// post-pass's order.  tests/test_qoi_host.py checks it against numpy references and central differences;
// tests/test_gpu_qoi_point.py checks the device kernels, which compile the same functions, against it.
#include <cstring>
#include <vector>

#include "../../calibr8_amd/csrc/c8_qoi_point.hpp"
#include "../../calibr8_amd/csrc/c8_registry.hpp"

using namespace c8;

struct Out {
  double* value;   // [points]                 per-point values (0 outside the set)
  double* dxi;     // [points][NLOC]           dq/dxi
  double* rec;     // [points][QOI_REC]        the x-records
  double* dxe;     // [points][NN][4]          the records contracted with every element node: du[3], dp
  double* dparam;  // [points][NPARAMS]        dq/dp for every parameter
  double* g;       // [points][NLOC]           -= dq/dxi                       (pre-pass)
  double* b0;      // [nnodes][DIM]            -= dJ/du                        (post-pass)
  double* b1;      // [nnodes]                 -= dJ/dp; ignored under one residual
};

template <class E, template <class> class ModelT>
static int run(ModelTag<ModelT>, MeshTables const& mt, FieldArgs const& fa, SubdomainQoi const& sq, int nelems, int nnodes, Out const& o) {
  constexpr int NL = ModelT<double>::NLOC, NP = ModelT<double>::NPARAMS;
  std::vector<double> rec((size_t)nelems * E::NP0 * QOI_REC, 0.);
  for (int e = 0; e < nelems; ++e)
    for (int pt = 0; pt < E::NP0; ++pt) {
      size_t const q = (size_t)e * E::NP0 + pt;
      if (!qoi_in_set(mt, sq, e)) continue;
      QoiPoint<ModelT> d;
      qoi_point_load<E, ModelT>(mt, fa, e, pt, d);
      if (o.value) o.value[q] = qoi_point_value<E, ModelT>(mt, sq, d);
      for (int t = 0; t < QOI_REC; ++t) rec[q * QOI_REC + t] = qoi_point_dx<E, ModelT>(mt, sq, d, t);
      for (int j = 0; j < NL; ++j) {
        double const dj = qoi_point_dxi<E, ModelT>(mt, sq, d, j);
        if (o.dxi) o.dxi[q * NL + j] = dj;
        if (o.g) o.g[q * NL + j] -= dj;
      }
      if (o.dparam)
        for (int k = 0; k < NP; ++k) o.dparam[q * NP + k] = qoi_point_dparam<E, ModelT>(mt, sq, d, k);
    }
  if (o.rec) std::memcpy(o.rec, rec.data(), rec.size() * sizeof(double));
  // the contraction with the element nodes, and the per-node sums: elements ascending, the points of an element ascending
  std::vector<double> su((size_t)nnodes * 4, 0.);
  std::vector<char> any(nnodes, 0);
  for (int e = 0; e < nelems; ++e) {
    if (!qoi_in_set(mt, sq, e)) continue;
    NodeAtPoint<E> sh;
    for (int m = 0; m < E::NN; ++m)
      for (int i = 0; i < 3; ++i) sh.X[m][i] = (i < E::DIM) ? mt.coords[(size_t)mt.conn[(size_t)e * E::NN + m] * 3 + i] : 0.;
    for (int pt = 0; pt < E::NP0; ++pt)
      for (int a = 0; a < E::NN; ++a) {
        size_t const q = (size_t)e * E::NP0 + pt;
        int const node = mt.conn[(size_t)e * E::NN + a];
        double du[3], dp;
        qoi_node_contract<E>(sh, pt, a, &rec[q * QOI_REC], du, dp);
        if (o.dxe) {
          for (int i = 0; i < 3; ++i) o.dxe[(q * E::NN + a) * 4 + i] = du[i];
          o.dxe[(q * E::NN + a) * 4 + 3] = dp;
        }
        for (int i = 0; i < 3; ++i) su[(size_t)node * 4 + i] += du[i];
        su[(size_t)node * 4 + 3] += dp;
        any[node] = 1;
      }
  }
  for (int n = 0; n < nnodes; ++n) {
    if (!any[n]) continue;
    if (o.b0)
      for (int i = 0; i < E::DIM; ++i) o.b0[(size_t)n * E::DIM + i] -= su[(size_t)n * 4 + i];
    if (o.b1 && E::NRES == 2) o.b1[n] -= su[(size_t)n * 4 + 3];
  }
  return E::NP0;
}

// The model `name` on elem_type (3 tri3, 4 tet4, 8 hex8); elem_set and nn may be null; qoi = {kind, element set, index}.
// Every output may be null; value, dxi, rec, dxe and dparam are assigned (points outside the set are left as they are),
// g, b0 and b1 are subtracted from, as the device passes do.  Returns the number of points per element, or -1 if the model
// table has no such row on that element type.
extern "C" int qoi_host(char const* name, int elem_type, int nelems, int nnodes, int32_t const* conn, double const* coords,
                        int32_t const* elem_set, double const* params, double const* nn, double const* u, double const* p,
                        double const* u_prev, double const* p_prev, double const* xi_prev, double const* xi, int32_t const* qoi,
                        double* value, double* dxi, double* rec, double* dxe, double* dparam, double* g, double* b0, double* b1) {
  MeshTables mt{};
  mt.conn = conn;
  mt.coords = coords;
  mt.elem_set = elem_set;
  mt.params = params;
  mt.nn = nn;
  FieldArgs const fa{u, p, u_prev, p_prev, xi_prev, const_cast<double*>(xi)};
  SubdomainQoi const sq{qoi[0], qoi[1], qoi[2]};
  Out const o{value, dxi, rec, dxe, dparam, g, b0, b1};
  int npts = -1;
  visit_models([&](auto row) {
    using R = decltype(row);
    if (std::strcmp(row.name, name) != 0) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) npts = run<Elem<C8_HEX8>>(row, mt, fa, sq, nelems, nnodes, o);
      if (elem_type == C8_TET4) npts = run<Elem<C8_TET4>>(row, mt, fa, sq, nelems, nnodes, o);
    } else {
      if (elem_type == C8_TRI3) npts = run<typename R::Elem2D>(row, mt, fa, sq, nelems, nnodes, o);
    }
  });
  return npts;
}
