// c8_spr.hpp -- superconvergent patch recovery (the reference's cspr.cpp) of a point field [elements][points][ncomp] to the
// nodes [nodes][ncomp], restated for linear meshes: the fit polynomial is 1, x, y (tri3) or 1, x, y, z (hex8, tet4), the
// samples are the coupled points (ip set 0) at their isoparametric positions.
//
// Per node n the recovered value is the constant coefficient of the least-squares polynomial through the samples of the
// node's patch, in coordinates centred at the node and scaled by h = max_s |x_s - x_n|_inf.  That coefficient is linear in
// the sample values: value = sum_s w_s v_s with w_s = g . terms((x_s - x_n) / h) and g = R^-1 R^-T e_0, R the triangular
// factor of the fit matrix.  g and h depend on the mesh alone, so the geometric set-up (patches, g, h) is done once and a
// recovery is one weighted sum per node (spr_apply_host here, k_spr_apply on the device).
//
// HIP-free: the fit (spr_fit) is C8_HD and compiles for the device too; the patch builder is host code.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "c8_element.hpp"

namespace c8 {

// a patch is rank-deficient when some |R_kk| <= SPR_RANK_TOL sqrt(m), m samples (|R_00| = sqrt(m)): accepted patches
// measure >= 6.6e-3, deficient ones ~1e-16
constexpr double SPR_RANK_TOL = 1e-8;
constexpr int SPR_MAX_COMP = 16;

C8_HD int spr_dim(int elem_type) { return elem_type == C8_TRI3 ? 2 : 3; }
C8_HD int spr_np0(int elem_type) { return elem_type == C8_HEX8 ? 8 : 1; }
// countPatchPoints >= 1.1 polynomial_terms (cspr.cpp: hasEnoughPoints), in integers
C8_HD bool spr_enough_points(int np0, int nelems_in_patch, int terms) { return 10ll * np0 * nelems_in_patch >= 11ll * terms; }

// the polynomial terms at the centred, scaled position of x: t[0] = 1, t[1 + d] = (x_d - xn_d) / h
template <int DIM> C8_HD void spr_terms(double const* x, double const* xn, double inv_h, double* t) {
  t[0] = 1.;
  C8_UNROLL
  for (int d = 0; d < DIM; ++d) t[1 + d] = (x[d] - xn[d]) * inv_h;
}

// position of coupled point pt of element e: the isoparametric map of the point
template <class E> C8_HD void spr_point(int32_t const* conn, double const* coords, int e, int pt, double* x) {
  double xi[3], w;
  E::point(0, pt, xi, w);
  C8_UNROLL
  for (int d = 0; d < E::DIM; ++d) x[d] = 0.;
  C8_UNROLL
  for (int a = 0; a < E::NN; ++a) {
    double const Na = E::N(a, xi);
    int32_t const na = conn[(size_t)e * E::NN + a];
    C8_UNROLL
    for (int d = 0; d < E::DIM; ++d) x[d] += Na * coords[(size_t)na * 3 + d];
  }
}

// x = R^-1 R^-T b for the upper triangle R: R^T y = b, then R x = y
template <int T> C8_HD void spr_solve_rtr(double const (&R)[T][T], double const* b, double* x) {
  double y[T];
  C8_UNROLL
  for (int i = 0; i < T; ++i) {
    double s = b[i];
    C8_UNROLL
    for (int j = 0; j < i; ++j) s -= R[j][i] * y[j];
    y[i] = s / R[i][i];
  }
  C8_UNROLL
  for (int i = T - 1; i >= 0; --i) {
    double s = y[i];
    C8_UNROLL
    for (int j = i + 1; j < T; ++j) s -= R[i][j] * x[j];
    x[i] = s / R[i][i];
  }
}

// Streaming QR of the centred, scaled fit matrix by Givens rotations, one sample row at a time: the state is the upper
// triangle of R (10 or 6 doubles), A is never stored.  The samples are the np0 points of the elements elems[k] >> shift,
// k < nel (shift 3: the packed node -> element lists of HostGraph; 0: plain element ids), at pts [nelems][np0][DIM].
// Writes h and g [DIM + 1] (zeros for a rank-deficient patch) and returns min_k |R_kk| / sqrt(m).
template <int DIM>
C8_HD double spr_fit(int32_t const* elems, int nel, int shift, int np0, double const* pts, double const* xn, double* g, double* h_out) {
  constexpr int T = DIM + 1;
  double h = 0.;
  for (int k = 0; k < nel; ++k) {
    double const* x = pts + (size_t)(elems[k] >> shift) * np0 * DIM;
    for (int q = 0; q < np0 * DIM; ++q) {
      double const d = fabs(x[q] - xn[q % DIM]);
      h = d > h ? d : h;
    }
  }
  if (!(h > 0.)) h = 1.;
  double const inv_h = 1. / h;
  double R[T][T];
  C8_UNROLL
  for (int i = 0; i < T; ++i) {
    C8_UNROLL
    for (int j = 0; j < T; ++j) R[i][j] = 0.;
  }
  for (int k = 0; k < nel; ++k) {
    double const* xe = pts + (size_t)(elems[k] >> shift) * np0 * DIM;
    for (int pt = 0; pt < np0; ++pt) {
      double a[T];
      spr_terms<DIM>(xe + pt * DIM, xn, inv_h, a);
      C8_UNROLL
      for (int i = 0; i < T; ++i) {
        double const r = sqrt(R[i][i] * R[i][i] + a[i] * a[i]);
        bool const rot = a[i] != 0.;  // r > 0 then
        double const c = rot ? R[i][i] / r : 1., s = rot ? a[i] / r : 0.;
        R[i][i] = rot ? r : R[i][i];
        C8_UNROLL
        for (int j = i + 1; j < T; ++j) {
          double const Rij = R[i][j], aj = a[j];
          R[i][j] = c * Rij + s * aj;
          a[j] = c * aj - s * Rij;
        }
      }
    }
  }
  double const m = (double)nel * np0;
  double rmin = fabs(R[0][0]);
  C8_UNROLL
  for (int i = 1; i < T; ++i) rmin = fabs(R[i][i]) < rmin ? fabs(R[i][i]) : rmin;
  double const ratio = m > 0. ? rmin / sqrt(m) : 0.;
  *h_out = h;
  if (!(ratio > SPR_RANK_TOL)) {
    C8_UNROLL
    for (int i = 0; i < T; ++i) g[i] = 0.;
    return ratio;
  }
  double e0[T];
  C8_UNROLL
  for (int i = 0; i < T; ++i) e0[i] = i == 0 ? 1. : 0.;
  spr_solve_rtr<T>(R, e0, g);
  // One step of refinement against the samples themselves (corrected semi-normal equations): R^T R g = e_0 alone loses
  // cond(A)^2, which an affine field on a nearly coplanar patch shows; with the residual e_0 - A^T (A g) taken from a
  // second pass over the rows the error is that of a backward-stable least-squares solve.
  for (int k = 0; k < nel; ++k) {
    double const* xe = pts + (size_t)(elems[k] >> shift) * np0 * DIM;
    for (int pt = 0; pt < np0; ++pt) {
      double a[T];
      spr_terms<DIM>(xe + pt * DIM, xn, inv_h, a);
      double w = 0.;
      C8_UNROLL
      for (int i = 0; i < T; ++i) w += a[i] * g[i];
      C8_UNROLL
      for (int i = 0; i < T; ++i) e0[i] -= a[i] * w;
    }
  }
  double dg[T];
  spr_solve_rtr<T>(R, e0, dg);
  C8_UNROLL
  for (int i = 0; i < T; ++i) g[i] += dg[i];
  return ratio;
}

// ---- host side: sample positions, patches, the sequential recovery ---------------------------------------------------

// the mesh as the patch builder sees it.  ne_ptr / ne: node -> elements, ascending, entries (element << ne_shift) | low bits that are not read
struct SprMesh {
  int elem_type = 0, nnodes = 0, nelems = 0;
  double const* coords = nullptr;   // [nnodes][3]
  int32_t const* conn = nullptr;    // [nelems][nn]
  int32_t const* ne_ptr = nullptr;  // [nnodes + 1]
  int32_t const* ne = nullptr;
  int ne_shift = 0;
  double const* pts = nullptr;      // [nelems][np0][dim] (spr_points_host)
};

// plain node -> element lists (ascending element ids, shift 0)
inline void spr_node_elems(int nnodes, int nelems, int nn, int32_t const* conn, std::vector<int32_t>& ptr, std::vector<int32_t>& list) {
  ptr.assign((size_t)nnodes + 1, 0);
  for (size_t q = 0; q < (size_t)nelems * nn; ++q) ptr[(size_t)conn[q] + 1]++;
  for (int n = 0; n < nnodes; ++n) ptr[n + 1] += ptr[n];
  list.assign((size_t)nelems * nn, 0);
  std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
  for (int e = 0; e < nelems; ++e)
    for (int a = 0; a < nn; ++a) list[(size_t)fill[conn[(size_t)e * nn + a]]++] = e;
}

inline void spr_points_host(int elem_type, int nelems, int32_t const* conn, double const* coords, double* pts) {
  for (int e = 0; e < nelems; ++e) {
    if (elem_type == C8_HEX8)
      for (int pt = 0; pt < 8; ++pt) spr_point<Elem<C8_HEX8>>(conn, coords, e, pt, pts + ((size_t)e * 8 + pt) * 3);
    else if (elem_type == C8_TET4)
      spr_point<Elem<C8_TET4>>(conn, coords, e, 0, pts + (size_t)e * 3);
    else
      spr_point<Elem<C8_TRI3>>(conn, coords, e, 0, pts + (size_t)e * 2);
  }
}

inline double spr_fit_any(int dim, int32_t const* elems, int nel, int shift, int np0, double const* pts, double const* xn, double* g, double* h) {
  return dim == 2 ? spr_fit<2>(elems, nel, shift, np0, pts, xn, g, h) : spr_fit<3>(elems, nel, shift, np0, pts, xn, g, h);
}

// hasEnoughPoints: enough samples and a fit matrix of full column rank; g and h are those of this patch
inline bool spr_accept(SprMesh const& m, int node, std::vector<int32_t> const& patch, double* g, double* h, double* ratio = nullptr) {
  int const dim = spr_dim(m.elem_type), np0 = spr_np0(m.elem_type);
  double r = 0.;
  bool ok = spr_enough_points(np0, (int)patch.size(), dim + 1);
  if (ok) {
    r = spr_fit_any(dim, patch.data(), (int)patch.size(), 0, np0, m.pts, m.coords + (size_t)node * 3, g, h);
    ok = r > SPR_RANK_TOL;
  }
  if (ratio) *ratio = r;
  return ok;
}

// The elements that share a k-entity with an element of `old`, by the node-count rule of a conforming mesh: at least
// `common` nodes in common.  Added to `patch` (kept ascending, no duplicates).
inline void spr_add_sharing(SprMesh const& m, std::vector<int32_t> const& old, int common, std::vector<int32_t>& patch) {
  int const nn = m.elem_type;  // 3, 4, 8: the type ids are the node counts
  std::vector<int32_t> cand, add;
  for (int32_t e : old) {
    cand.clear();
    for (int a = 0; a < nn; ++a) {
      int32_t const na = m.conn[(size_t)e * nn + a];
      for (int32_t k = m.ne_ptr[na]; k < m.ne_ptr[na + 1]; ++k) cand.push_back(m.ne[k] >> m.ne_shift);
    }
    std::sort(cand.begin(), cand.end());
    for (size_t i = 0; i < cand.size();) {
      size_t j = i;
      while (j < cand.size() && cand[j] == cand[i]) ++j;
      if ((int)(j - i) >= common) add.push_back(cand[i]);
      i = j;
    }
  }
  patch.insert(patch.end(), add.begin(), add.end());
  std::sort(patch.begin(), patch.end());
  patch.erase(std::unique(patch.begin(), patch.end()), patch.end());
}

// nodes in common for "shares a (d-1)-, ..., 0-entity": faces, edges, vertices
inline int spr_stage_rule(int elem_type, int const** rule) {
  static int const tet[3] = {3, 2, 1}, hex[3] = {4, 2, 1}, tri[2] = {2, 1};
  *rule = elem_type == C8_HEX8 ? hex : (elem_type == C8_TET4 ? tet : tri);
  return elem_type == C8_TRI3 ? 2 : 3;
}

// buildPatch (cspr.cpp): the elements of the node, grown stage by stage until accepted.  Returns false when the patch stops
// growing ("all hope is lost").  `stages` counts the expansion stages that were run.
inline bool spr_build_patch(SprMesh const& m, int node, std::vector<int32_t>& patch, double* g, double* h, int* stages) {
  patch.clear();
  for (int32_t k = m.ne_ptr[node]; k < m.ne_ptr[node + 1]; ++k) patch.push_back(m.ne[k] >> m.ne_shift);
  *stages = 0;
  if (spr_accept(m, node, patch, g, h)) return true;
  int const* rule = nullptr;
  int const nstages = spr_stage_rule(m.elem_type, &rule);
  for (;;) {
    std::vector<int32_t> const old = patch;
    for (int s = 0; s < nstages; ++s) {
      spr_add_sharing(m, old, rule[s], patch);
      ++*stages;
      if (spr_accept(m, node, patch, g, h)) return true;
    }
    if (patch.size() == old.size()) return false;
  }
}

// Sequential recovery: nodal [nnodes][ncomp] = sum over the node's samples, in table order, of w_s v_s.  abs_sum (may be
// null) receives sum_s |w_s v_s| per entry, the scale of the rounding error of that sum.
inline void spr_apply_host(int elem_type, int nnodes, int ncomp, int64_t const* patch_ptr, int32_t const* patch_elems, double const* g,
                           double const* h, double const* pts, double const* coords, double const* field, double* nodal, double* abs_sum) {
  int const dim = spr_dim(elem_type), np0 = spr_np0(elem_type), T = dim + 1;
  for (int n = 0; n < nnodes; ++n) {
    double acc[SPR_MAX_COMP], mag[SPR_MAX_COMP];
    for (int c = 0; c < ncomp; ++c) acc[c] = mag[c] = 0.;
    double const inv_h = 1. / h[n];
    for (int64_t k = patch_ptr[n]; k < patch_ptr[n + 1]; ++k)
      for (int pt = 0; pt < np0; ++pt) {
        size_t const q = (size_t)patch_elems[k] * np0 + pt;
        double t[4];
        if (dim == 2) spr_terms<2>(pts + q * 2, coords + (size_t)n * 3, inv_h, t);
        else spr_terms<3>(pts + q * 3, coords + (size_t)n * 3, inv_h, t);
        double w = 0.;
        for (int i = 0; i < T; ++i) w += g[(size_t)n * T + i] * t[i];
        for (int c = 0; c < ncomp; ++c) {
          double const wv = w * field[q * ncomp + c];
          acc[c] += wv;
          mag[c] += std::fabs(wv);
        }
      }
    for (int c = 0; c < ncomp; ++c) {
      nodal[(size_t)n * ncomp + c] = acc[c];
      if (abs_sum) abs_sum[(size_t)n * ncomp + c] = mag[c];
    }
  }
}

// The whole set-up on the host.  patch_ptr [nnodes + 1] is always filled; patch_elems (capacity entries), g [nnodes][dim + 1],
// h [nnodes], stages [nnodes] and ratio [nnodes] (min |R_kk| / sqrt(m) of the accepted patch) where not null.  Returns -1,
// or the first node whose patch cannot be completed (nothing after it is filled), or -2 when capacity is too small.
inline int spr_build_all(SprMesh const& m, int64_t* patch_ptr, int32_t* patch_elems, int64_t capacity, double* g, double* h, int32_t* stages,
                         double* ratio) {
  int const T = spr_dim(m.elem_type) + 1;
  std::vector<int32_t> patch;
  patch_ptr[0] = 0;
  for (int n = 0; n < m.nnodes; ++n) {
    double gn[4] = {0., 0., 0., 0.}, hn = 1.;
    int st = 0;
    if (!spr_build_patch(m, n, patch, gn, &hn, &st)) return n;
    patch_ptr[n + 1] = patch_ptr[n] + (int64_t)patch.size();
    if (patch_elems) {
      if (patch_ptr[n + 1] > capacity) return -2;
      std::copy(patch.begin(), patch.end(), patch_elems + patch_ptr[n]);
    }
    if (g) std::copy(gn, gn + T, g + (size_t)n * T);
    if (h) h[n] = hn;
    if (stages) stages[n] = st;
    if (ratio) spr_accept(m, n, patch, gn, &hn, ratio + n);
  }
  return -1;
}

}  // namespace c8
