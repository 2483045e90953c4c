// spr_host.cpp -- TEST HARNESS: the functions of calibr8_amd/csrc/c8_spr.hpp (the source the device kernels compile)
// built with g++ and called from tests/spr_cases.py.
#include <cstdint>
#include <vector>

#include "../../calibr8_amd/csrc/c8_spr.hpp"

using namespace c8;

extern "C" {

// spr_fit on an explicit point set [npoints][dim] (one sample per "element"); returns min |R_kk| / sqrt(m)
double spr_host_fit(int dim, int npoints, double const* points, double const* xn, double* g, double* h) {
  std::vector<int32_t> ids((size_t)npoints);
  for (int i = 0; i < npoints; ++i) ids[i] = i;
  return spr_fit_any(dim, ids.data(), npoints, 0, 1, points, xn, g, h);
}

// sample positions [nelems][np0][dim]
void spr_host_points(int elem_type, int nelems, int32_t const* conn, double const* coords, double* pts) {
  spr_points_host(elem_type, nelems, conn, coords, pts);
}

// the whole set-up, with min |R_kk| / sqrt(m) of every accepted patch; the return value of spr_build_all
int spr_host_build(int elem_type, int nnodes, int nelems, double const* coords, int32_t const* conn, int64_t* patch_ptr,
                   int32_t* patch_elems, int64_t capacity, double* g, double* h, int32_t* stages, double* ratio) {
  std::vector<int32_t> ne_ptr, ne;
  spr_node_elems(nnodes, nelems, elem_type, conn, ne_ptr, ne);
  std::vector<double> pts((size_t)nelems * spr_np0(elem_type) * spr_dim(elem_type));
  spr_points_host(elem_type, nelems, conn, coords, pts.data());
  SprMesh const m{elem_type, nnodes, nelems, coords, conn, ne_ptr.data(), ne.data(), 0, pts.data()};
  return spr_build_all(m, patch_ptr, patch_elems, capacity, g, h, stages, ratio);
}

// min |R_kk| / sqrt(m) of the fit of node `node` over the elements elems[0 .. nel)
double spr_host_patch_ratio(int elem_type, int nelems, double const* coords, int32_t const* conn, int node, int32_t const* elems, int nel) {
  std::vector<double> pts((size_t)nelems * spr_np0(elem_type) * spr_dim(elem_type));
  spr_points_host(elem_type, nelems, conn, coords, pts.data());
  double g[4], h;
  return spr_fit_any(spr_dim(elem_type), elems, nel, 0, spr_np0(elem_type), pts.data(), coords + (size_t)node * 3, g, &h);
}

// spr_apply_host; weights (may be null) [total samples in table order] = w_s
void spr_host_apply(int elem_type, int nnodes, int nelems, int ncomp, double const* coords, int32_t const* conn, int64_t const* patch_ptr,
                    int32_t const* patch_elems, double const* g, double const* h, double const* field, double* nodal, double* abs_sum,
                    double* weights) {
  int const np0 = spr_np0(elem_type), dim = spr_dim(elem_type);
  std::vector<double> pts((size_t)nelems * np0 * dim);
  spr_points_host(elem_type, nelems, conn, coords, pts.data());
  spr_apply_host(elem_type, nnodes, ncomp, patch_ptr, patch_elems, g, h, pts.data(), coords, field, nodal, abs_sum);
  if (weights) {
    size_t s = 0;
    for (int n = 0; n < nnodes; ++n)
      for (int64_t k = patch_ptr[n]; k < patch_ptr[n + 1]; ++k)
        for (int pt = 0; pt < np0; ++pt, ++s) {
          double t[4] = {0., 0., 0., 0.};
          double const* x = pts.data() + ((size_t)patch_elems[k] * np0 + pt) * dim;
          if (dim == 2) spr_terms<2>(x, coords + (size_t)n * 3, 1. / h[n], t);
          else spr_terms<3>(x, coords + (size_t)n * 3, 1. / h[n], t);
          double w = 0.;
          for (int i = 0; i <= dim; ++i) w += g[(size_t)n * (dim + 1) + i] * t[i];
          weights[s] = w;
        }
  }
}

}  // extern "C"
