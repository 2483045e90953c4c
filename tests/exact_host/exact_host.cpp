// tests/exact_host/exact_host.cpp -- TEST INFRASTRUCTURE.
//
// The product's per-point exact and linearization error terms (calibr8_amd/csrc/c8_exact.hpp: exact_terms) compiled for the
// CPU and summed per element in the kernel's order (the points of ip set 0 ascending, then those of ip set 1) and with the
// kernel's sign (E += -sum).  tests/test_exact_host.py checks it against the oracle and against tests/error_host;
// tests/test_gpu_exact_errors.py checks the device kernel, which compiles the same function, against it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../calibr8_amd/csrc/c8_exact.hpp"
#include "../../calibr8_amd/csrc/c8_registry.hpp"

using namespace c8;

template <class E, template <class> class ModelT, bool LIN>
static void sums(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, FieldArgs const& ff, ErrorArgs const& ea,
                 int nelems, double* E_R, double* E_C) {
  for (int e = 0; e < nelems; ++e) {
    double sr = 0., sc = 0.;
    double same[E::NP0];  // the values of ip set 1 that the evaluations of ip set 0 return: added after those, as the kernel does
    for (int s = 0; s < error_lanes<E>(); ++s) {
      double er, ec, er_same;
      exact_terms<E, ModelT, LIN>(mt, ms, fa, ff, ea, e, s, er, ec, er_same);
      sr += er;
      sc += ec;
      if (s < E::NP0) same[s] = er_same;
    }
    if (error_shares_points<E>())
      for (int s = 0; s < E::NP0; ++s) sr += same[s];
    E_R[e] += -sr;
    E_C[e] += -sc;
  }
}

template <class E, template <class> class ModelT>
static int run(ModelTag<ModelT>, MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, FieldArgs const& ff,
               ErrorArgs const& ea, int nelems, bool lin, double* E_R, double* E_C, double* abs_R, double* abs_C) {
  constexpr int NL = ModelT<double>::NLOC;
  if (lin) sums<E, ModelT, true>(mt, ms, fa, ff, ea, nelems, E_R, E_C);
  else sums<E, ModelT, false>(mt, ms, fa, ff, ea, nelems, E_R, E_C);
  if (!abs_R || !abs_C) return error_slots<E>();
  // The magnitudes of the terms, as tests/error_host forms them: every value is linear in the adjoint, so with every entry
  // of z but one (of phi but one) set to zero the function returns that entry's term.  Tangent terms always; for the
  // linearization fields the value terms (error_point's) as well, each with its own magnitude.
  int nnodes = 0;
  for (int i = 0; i < nelems * E::NN; ++i) nnodes = std::max(nnodes, mt.conn[i] + 1);
  std::vector<double> zu((size_t)nnodes * E::DIM, 0.), zp(nnodes, 0.), ph((size_t)nelems * E::NP0 * NL, 0.);
  ErrorArgs const one{zu.data(), zp.data(), ph.data()};
  for (int e = 0; e < nelems; ++e)
    for (int s = 0; s < error_lanes<E>(); ++s) {
      double er, ec, er_same;
      for (int n = 0; n < E::NN; ++n) {
        size_t const node = (size_t)mt.conn[(size_t)e * E::NN + n];
        for (int i = 0; i < E::DIM + (E::NRES == 2 ? 1 : 0); ++i) {
          double& z = i < E::DIM ? zu[node * E::DIM + i] : zp[node];
          z = i < E::DIM ? ea.z_u[node * E::DIM + i] : ea.z_p[node];
          exact_point<E, ModelT>(mt, ms, fa, ff, one, e, s, er, ec, er_same);
          abs_R[e] += std::fabs(er) + std::fabs(er_same);
          if (lin) {
            error_point<E, ModelT>(mt, ms, fa, one, e, s, er, ec, er_same);
            abs_R[e] += std::fabs(er) + std::fabs(er_same);
          }
          z = 0.;
        }
      }
      if (s < E::NP0)
        for (int j = 0; j < NL; ++j) {
          size_t const q = ((size_t)e * E::NP0 + s) * NL + j;
          ph[q] = ea.phi[q];
          exact_point<E, ModelT>(mt, ms, fa, ff, one, e, s, er, ec, er_same);
          abs_C[e] += std::fabs(ec);
          if (lin) {
            error_point<E, ModelT>(mt, ms, fa, one, e, s, er, ec, er_same);
            abs_C[e] += std::fabs(ec);
          }
          ph[q] = 0.;
        }
    }
  return error_slots<E>();
}

// E_R, E_C [nelems] += the exact (lin == 0) or linearization (lin != 0) error fields of the model `name` on elem_type (3 tri3,
// 4 tet4, 8 hex8), from the stored state (u .. xi) and the fine state (u_f .. xi_f); elem_set and nn may be null; settings =
// {stabilisation multiplier, absolute tolerance of the local residual (the branch test), thickness}.  abs_R, abs_C [nelems]
// (both or neither) += the sums of the magnitudes of the terms.  Returns the number of slots per element, or -1 if the
// model table has no such row on that element type.
extern "C" int exact_host(char const* name, int elem_type, int nelems, int32_t const* conn, double const* coords,
                          int32_t const* elem_set, double const* params, double const* nn, double const* settings, double const* u,
                          double const* p, double const* u_prev, double const* p_prev, double const* xi_prev, double const* xi,
                          double const* u_f, double const* p_f, double const* u_prev_f, double const* p_prev_f,
                          double const* xi_prev_f, double const* xi_f, double const* z_u, double const* z_p, double const* phi,
                          int lin, double* E_R, double* E_C, double* abs_R, double* abs_C) {
  MeshTables mt{};
  mt.conn = conn;
  mt.coords = coords;
  mt.elem_set = elem_set;
  mt.params = params;
  mt.nn = nn;
  ModelSettings ms{};
  ms.stab_mult = settings[0];
  ms.abs_tol = settings[1];
  ms.thickness = settings[2];
  FieldArgs const fa{u, p, u_prev, p_prev, xi_prev, const_cast<double*>(xi)};
  FieldArgs const ff{u_f, p_f, u_prev_f, p_prev_f, xi_prev_f, const_cast<double*>(xi_f)};
  ErrorArgs const ea{z_u, z_p, phi};
  int slots = -1;
  visit_models([&](auto row) {
    using R = decltype(row);
    if (std::strcmp(row.name, name) != 0) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) slots = run<Elem<C8_HEX8>>(row, mt, ms, fa, ff, ea, nelems, lin != 0, E_R, E_C, abs_R, abs_C);
      if (elem_type == C8_TET4) slots = run<Elem<C8_TET4>>(row, mt, ms, fa, ff, ea, nelems, lin != 0, E_R, E_C, abs_R, abs_C);
    } else {
      if (elem_type == C8_TRI3) slots = run<typename R::Elem2D>(row, mt, ms, fa, ff, ea, nelems, lin != 0, E_R, E_C, abs_R, abs_C);
    }
  });
  return slots;
}
