// tests/cauchy_host/cauchy_host.cpp -- TEST INFRASTRUCTURE.
//
// The product's per-point stress evaluation (calibr8_amd/csrc/c8_cauchy.hpp: cauchy_point) compiled for the CPU and
// looped over elements and points.  tests/test_cauchy_host.py checks it against the oracle's residual and closed forms;
// tests/test_gpu_cauchy.py checks the device kernel, which compiles the same function, against it.
#include <cstring>

#include "../../calibr8_amd/csrc/c8_cauchy.hpp"
#include "../../calibr8_amd/csrc/c8_registry.hpp"

using namespace c8;

template <class E, template <class> class ModelT>
static int run(ModelTag<ModelT>, MeshTables const& mt, FieldArgs const& fa, int nelems, double* sigma) {
  ModelSettings const ms{};
  for (int e = 0; e < nelems; ++e)
    for (int pt = 0; pt < E::NP0; ++pt) cauchy_point<E, ModelT>(mt, ms, fa, e, pt, sigma + ((size_t)e * E::NP0 + pt) * 9);
  return E::NP0;
}

// sigma [nelems][points][3][3] of the model `name` on elem_type (3 tri3, 4 tet4, 8 hex8); elem_set and nn may be null.
// Returns the number of points per element, or -1 if the model table has no such row on that element type.
extern "C" int cauchy_host(char const* name, int elem_type, int nelems, int32_t const* conn, double const* coords,
                           int32_t const* elem_set, double const* params, double const* nn, double const* u, double const* p,
                           double const* u_prev, double const* p_prev, double const* xi_prev, double const* xi, double* sigma) {
  MeshTables mt{};
  mt.conn = conn;
  mt.coords = coords;
  mt.elem_set = elem_set;
  mt.params = params;
  mt.nn = nn;
  FieldArgs const fa{u, p, u_prev, p_prev, xi_prev, const_cast<double*>(xi)};
  int npts = -1;
  visit_models([&](auto row) {
    using R = decltype(row);
    if (std::strcmp(row.name, name) != 0) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) npts = run<Elem<C8_HEX8>>(row, mt, fa, nelems, sigma);
      if (elem_type == C8_TET4) npts = run<Elem<C8_TET4>>(row, mt, fa, nelems, sigma);
    } else {
      if (elem_type == C8_TRI3) npts = run<typename R::Elem2D>(row, mt, fa, nelems, sigma);
    }
  });
  return npts;
}
