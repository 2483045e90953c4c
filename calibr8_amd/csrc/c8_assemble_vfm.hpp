// c8_assemble_vfm.hpp -- the virtual fields method (VFM): per-element kernels that drive the local constitutive update
// with MEASURED displacements and contract the internal-force residual with a fixed nodal virtual field w, in the SPMD
// form and lane mapping of c8_assemble.hpp (lane k of an element's group owns element DOF slot k).
//
//   V   vfm_power_element<.., false>   eval_measured_residual            evaluations.cpp:1750-1845
//   FS  vfm_power_element<.., true>    eval_measured_residual_and_grad   evaluations.cpp:1847-1973
//                                      + VirtualPower::compute_at_step_forward_sens (virtual_power.cpp:141-186)
//   A   vfm_adjoint_element            eval_vfm_adjoint_gradient         evaluations.cpp:1975-2143
//
// One-residual systems only (`mechanics_plane_stress` on Tri3PlaneStress), as the reference (virtual_power.cpp:110,148).
// Every product with w is formed per point and per element: the reference's dofs x params multivector dR
// (eval_measured_residual_and_grad) is never formed.  The per-element sums leave the group in its lanes (acc_v: w_k R_k,
// acc_g: the share of active parameter k); the kernels (c8_kernels.hip: k_vfm) add them up per block in a fixed order.
#pragma once

#include "c8_assemble_adjoint.hpp"

namespace c8 {

struct VfmArgs {
  double const* w;         // virtual field [nnodes][DIM]
  double const* S_prev;    // FS: local sensitivities of the previous step [nelems][NP0][NLOC][nact], or null (= 0)
  double* S;               // FS: those of this step, same layout
  double* h;               // A: local history (dC_{n+1}/dxi_n)^T phi_{n+1} [nelems][NP0][NLOC], in / out
  double c;                // A: the step's scaled mismatch
  int32_t const* active;   // [nsets][2 + 8]: {offset into grad, n_active, param indices...}
  int nact;                // active parameters over all element sets (columns of S, length of grad)
};

template <class E, template <class> class ModelT> struct VfmLane : ForwardLane<E, ModelT> {
  double acc_v;  // w_k R_k summed over the element's points
  double acc_g;  // derivative of w^T R_e with respect to active parameter k of the element's set
  double dRw_dp;
};

// K1's local Newton iteration (forward_jacobian_element) from the seeded state the caller set up: on exit the lanes
// hold the converged xi (values; lane k < NL still seeded along xi_k) and `failed` is set as K1 sets it
template <int NL, class Model, class EX, class SH>
C8_HD void vfm_local_solve(EX& ex, SH& sh, ModelSettings const& ms) {
  if constexpr (uses_line_search<Model>::value) {
    local_newton_line_search<NL>(ex, sh, ms);
  } else if (Model::HAS_LOCAL) {
    auto active = [&](int k) { auto& r = ex.lane(k); return (r.iter <= ms.max_iters) && !r.converged; };
    while (ex.any(active)) {
      ex.each([&](int k) {
        auto& r = ex.lane(k);
        if (!active(k)) return;
        r.m.evaluate(r.g, ms.abs_tol);
        double nrm = 0.;
        C8_UNROLL
        for (int j = 0; j < NL; ++j) nrm += r.m.R[j].v * r.m.R[j].v;
        double const R_norm = sqrt(nrm);
        if (r.iter == 1) r.R_norm_0 = R_norm;
        double const R_norm_rel = R_norm / r.R_norm_0;
        if ((R_norm_rel < ms.rel_tol) || (R_norm < ms.abs_tol)) r.converged = true;
        if (k < NL) C8_UNROLL for (int j = 0; j < NL; ++j) sh.M[j][k] = r.m.R[j].d;
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.b[j] = -r.m.R[j].v;
      });
      ex.sync();
      if (!ex.any(active)) break;
      bool const ok = gj_solve<NL>(ex, sh, [&](int k) { return ex.lane(k).b; });
      ex.each([&](int k) {
        auto& r = ex.lane(k);
        if (!ok) { r.failed = true; r.iter = ms.max_iters + 1; return; }
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.m.xi[j].v += r.b[j];
        r.iter++;
      });
    }
    ex.each([&](int k) {
      auto& r = ex.lane(k);
      if ((r.iter > ms.max_iters) && !r.converged) r.failed = true;
    });
  }
}

// the element's virtual-field values into sh.z (where the adjoint kernels keep z: flux_dot_adjoint reads them there), the
// parameters into the lanes, the accumulators cleared
template <class E, class EX, class SH>
C8_HD void vfm_load(EX& ex, SH& sh, MeshTables const& mt, VfmArgs const& va, int e) {
  ex.each([&](int k) {
    auto& r = ex.lane(k);
    int ik, nk, eqk;
    slot_to_dof<E>(k, ik, nk, eqk);
    sh.z[k] = va.w[(size_t)sh.node[nk] * E::DIM + eqk];
    r.acc_v = 0.;
    r.acc_g = 0.;
    r.Rk = 0.;
    r.failed = false;
    load_params(r.m, mt, e);
    if (k == 0) sh.h = elem_size<E>(sh);
  });
  ex.sync();
}

// =====================================================================================================================
// V (SENS = false): local solve from xi_prev with the measured x, x_prev; xi written; acc_v = w_k R_k; R scattered into
// sa.b[0] when that is not null.
// FS (SENS = true): V, and per point the local sensitivities of the active parameters (lane k: column k)
//   S = -(dC/dxi)^-1 (dC/dp + dC/dxi_prev S_prev),   acc_g += [(dR/dxi)^T w]^T S + (dR/dp)^T w.
// =====================================================================================================================
template <class E, template <class> class ModelT, bool SENS, class EX>
C8_HD void vfm_power_element(EX& ex, GroupShared<E, ModelT<Dual>::NLOC>& sh, MeshTables const& mt, ModelSettings const& ms,
                             FieldArgs const& fa, VfmArgs const& va, SystemArgs const& sa, int e) {
  using Model = ModelT<Dual>;
  constexpr int NL = Model::NLOC;
  constexpr bool PREV = Model::FINITE_DEF;
  static_assert(E::NRES == 1 && E::NSETS == 1, "VFM applies to one-residual systems");
  load_element<E>(ex, sh, mt, fa, e, PREV);
  vfm_load<E>(ex, sh, mt, va, e);
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  int32_t const* act = va.active + es * 10;
  shape_tables<E>(ex, sh, 0);
  for (int pt = 0; pt < E::NP0; ++pt) {
    size_t const qp = (size_t)e * E::NP0 + pt;
    ex.each([&](int k) {  // local->gather, seed_wrt_xi (as K1)
      auto& r = ex.lane(k);
      interpolate_values<E, Dual, PREV>(sh, pt, r.g);
      C8_UNROLL
      for (int j = 0; j < NL; ++j) {
        r.m.xi_prev[j] = Dual(fa.xi_prev[qp * NL + j]);
        r.m.xi[j] = Dual(fa.xi[qp * NL + j], (j == k) ? 1. : 0.);
        r.m.R[j] = Dual(0.);
      }
      r.m.initial_guess(r.g);
      r.iter = 1;
      r.R_norm_0 = 1.;
      r.converged = !Model::HAS_LOCAL;
    });
    vfm_local_solve<NL, Model>(ex, sh, ms);
    ex.each([&](int k) {  // local->scatter, unseed; the point's share of R_e
      auto& r = ex.lane(k);
      if (k == 0) {
        C8_UNROLL
        for (int j = 0; j < NL; ++j) fa.xi[qp * NL + j] = r.m.xi[j].v;
      }
      C8_UNROLL
      for (int j = 0; j < NL; ++j) r.m.xi[j].d = 0.;
      MechFlux<Dual> f;
      global_flux<E>(r.m, r.g, sh.h, ms, f);
      r.Rk += residual_entry<E>(sh, pt, k, f);
    });
    if constexpr (SENS) {
      ex.each([&](int k) {
        auto& r = ex.lane(k);
        // xi seeded (lane k < NL: xi_k): dC/dxi into sh.M, (dR/dxi_k)^T w into sh.vec[k]
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.m.xi[j].d = (j == k) ? 1. : 0.;
        r.m.evaluate(r.g, ms.abs_tol);
        MechFlux<Dual> f;
        global_flux<E>(r.m, r.g, sh.h, ms, f);
        double const dRw_dxi = flux_dot_adjoint<E>(sh, pt, f, true);
        if (k < NL) {
          C8_UNROLL
          for (int j = 0; j < NL; ++j) sh.M[j][k] = r.m.R[j].d;
          sh.vec[k] = dRw_dxi;
        }
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.m.xi[j].d = 0.;
        // parameter act[2 + k] seeded, xi_prev seeded along column k of S_prev: C.d = dC/dp + dC/dxi_prev S_prev;
        // the global flux does not read xi_prev, so f.d = dR/dp
        int const nact = act[1];
        int const mine = (k < nact) ? act[2 + k] : -1;
        int const slot = (k < nact) ? act[0] + k : -1;
        C8_UNROLL
        for (int q = 0; q < Model::NPARAMS; ++q) r.m.params[q].d = (q == mine) ? 1. : 0.;
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.m.xi_prev[j].d = (slot >= 0 && va.S_prev) ? va.S_prev[(qp * NL + j) * va.nact + slot] : 0.;
        r.m.evaluate(r.g, ms.abs_tol);
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.b[j] = -r.m.R[j].d;
        global_flux<E>(r.m, r.g, sh.h, ms, f);
        r.dRw_dp = flux_dot_adjoint<E>(sh, pt, f, true);
        C8_UNROLL
        for (int q = 0; q < Model::NPARAMS; ++q) r.m.params[q].d = 0.;
        C8_UNROLL
        for (int j = 0; j < NL; ++j) r.m.xi_prev[j].d = 0.;
      });
      ex.sync();
      bool const ok = gj_solve<NL>(ex, sh, [&](int k) { return ex.lane(k).b; });
      ex.each([&](int k) {
        auto& r = ex.lane(k);
        if (!ok) r.failed = true;
        int const slot = (k < act[1]) ? act[0] + k : -1;
        if (slot < 0) return;
        double s = r.dRw_dp;
        C8_UNROLL
        for (int j = 0; j < NL; ++j) {
          va.S[(qp * NL + j) * va.nact + slot] = r.b[j];
          s += sh.vec[j] * r.b[j];
        }
        r.acc_g += s;
      });
    }
  }
  ex.sync();
  ex.each([&](int k) {
    auto& r = ex.lane(k);
    r.acc_v = sh.z[k] * r.Rk;
  });
  if (sa.b[0]) scatter_rhs<E>(ex, sh, sa, [&](int k) { return ex.lane(k).Rk; });
  ex.each([&](int k) {
    if (k == 0 && ex.lane(k).failed) ex.flag(sa.status);
  });
}

// =====================================================================================================================
// A: one backward step at the stored local state, with c the step's scaled mismatch:
//   phi = (dC/dxi)^-T (-c (dR/dxi)^T w - h),  h <- (dC/dxi_prev)^T phi,  acc_g += c (dR/dp)^T w + (dC/dp)^T phi.
// This is K4 with z = c w and g = -h followed by K5's share under an objective without own terms, in one pass.
// =====================================================================================================================
template <class E, template <class> class ModelT, class EX>
C8_HD void vfm_adjoint_element(EX& ex, GroupShared<E, ModelT<Dual>::NLOC>& sh, MeshTables const& mt, ModelSettings const& ms,
                               FieldArgs const& fa, VfmArgs const& va, SystemArgs const& sa, int e) {
  using Model = ModelT<Dual>;
  constexpr int NL = Model::NLOC;
  constexpr bool PREV = Model::FINITE_DEF;
  static_assert(E::NRES == 1 && E::NSETS == 1, "VFM applies to one-residual systems");
  load_element<E>(ex, sh, mt, fa, e, PREV);
  vfm_load<E>(ex, sh, mt, va, e);
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  int32_t const* act = va.active + es * 10;
  shape_tables<E>(ex, sh, 0);
  for (int pt = 0; pt < E::NP0; ++pt) {
    size_t const qp = (size_t)e * E::NP0 + pt;
    // xi seeded: (dC/dxi)^T into sh.M (transposed fill, as K4), right-hand side -c (dR/dxi)^T w - h
    ex.each([&](int k) {
      auto& r = ex.lane(k);
      interpolate_values<E, Dual, PREV>(sh, pt, r.g);
      C8_UNROLL
      for (int j = 0; j < NL; ++j) {
        r.m.xi_prev[j] = Dual(fa.xi_prev[qp * NL + j]);
        r.m.xi[j] = Dual(fa.xi[qp * NL + j], (j == k) ? 1. : 0.);
        r.m.R[j] = Dual(0.);
      }
      MechFlux<Dual> f;
      global_flux<E>(r.m, r.g, sh.h, ms, f);
      double const dRw = flux_dot_adjoint<E>(sh, pt, f, true);
      r.m.evaluate(r.g, ms.abs_tol);
      if (k < NL) {
        C8_UNROLL
        for (int j = 0; j < NL; ++j) sh.M[k][j] = r.m.R[j].d;
        sh.vec[k] = -va.c * dRw - va.h[qp * NL + k];
      }
    });
    ex.sync();
    ex.each([&](int k) {
      auto& r = ex.lane(k);
      C8_UNROLL
      for (int j = 0; j < NL; ++j) r.b[j] = sh.vec[j];
    });
    bool const ok = gj_solve<NL>(ex, sh, [&](int k) { return ex.lane(k).b; });
    ex.each([&](int k) {
      auto& r = ex.lane(k);
      if (!ok) r.failed = true;
      C8_UNROLL
      for (int j = 0; j < NL; ++j) r.m.xi[j].d = 0.;
      // xi_prev seeded (lane k < NL): h_k = ((dC/dxi_prev)^T phi)_k
      C8_UNROLL
      for (int j = 0; j < NL; ++j) r.m.xi_prev[j].d = (j == k) ? 1. : 0.;
      r.m.evaluate(r.g, ms.abs_tol);
      double hk = 0.;
      C8_UNROLL
      for (int j = 0; j < NL; ++j) hk += r.m.R[j].d * r.b[j];
      C8_UNROLL
      for (int j = 0; j < NL; ++j) r.m.xi_prev[j].d = 0.;
      if (k < NL) va.h[qp * NL + k] = hk;
      // parameter act[2 + k] seeded: (dC/dp)^T phi + c (dR/dp)^T w
      int const mine = (k < act[1]) ? act[2 + k] : -1;
      if (mine < 0) return;
      C8_UNROLL
      for (int q = 0; q < Model::NPARAMS; ++q) r.m.params[q].d = (q == mine) ? 1. : 0.;
      r.m.evaluate(r.g, ms.abs_tol);
      double s = 0.;
      C8_UNROLL
      for (int j = 0; j < NL; ++j) s += r.m.R[j].d * r.b[j];
      MechFlux<Dual> f;
      global_flux<E>(r.m, r.g, sh.h, ms, f);
      s += va.c * flux_dot_adjoint<E>(sh, pt, f, true);
      C8_UNROLL
      for (int q = 0; q < Model::NPARAMS; ++q) r.m.params[q].d = 0.;
      r.acc_g += s;
    });
  }
  ex.sync();
  ex.each([&](int k) {
    if (k == 0 && ex.lane(k).failed) ex.flag(sa.status);
  });
}

// ---- fixed-order block sums ------------------------------------------------------------------------------------------
// The groups of a block leave their lane sums here; vfm_block_sums then writes one partial sum per output and block,
// part[o][block], in a fixed order (groups in order, lanes in order).  Output 0 is w^T R where the kernel forms it, the
// others are the active parameters in grad order.  A single-block pass (c8_vfm.hip) sums the partials in a fixed order:
// no floating-point atomics anywhere, the values are exact functions of the inputs.
template <int GPB, int NDOF> struct VfmBlockSums {
  double v[GPB][NDOF];
  double g[GPB][NDOF];
  int ofs[GPB], n[GPB];
};

template <class S> C8_HD void vfm_group_sums(S& red, int gib, int k, double acc_v, double acc_g, int ofs, int n) {
  red.v[gib][k] = acc_v;
  red.g[gib][k] = acc_g;
  if (k == 0) { red.ofs[gib] = ofs; red.n[gib] = n; }
}

template <int GPB, int NDOF>
C8_HD void vfm_block_sums(VfmBlockSums<GPB, NDOF> const& red, int t, int nthreads, bool has_v, int nact, double* part, int lb,
                          int nblocks) {
  int const nv = has_v ? 1 : 0;
  for (int o = t; o < nv + nact; o += nthreads) {
    double s = 0.;
    if (o < nv) {
      for (int g = 0; g < GPB; ++g)
        for (int k = 0; k < NDOF; ++k) s += red.v[g][k];
    } else {
      for (int g = 0; g < GPB; ++g) {
        int const i = o - nv - red.ofs[g];
        if (i >= 0 && i < red.n[g]) s += red.g[g][i];
      }
    }
    part[(size_t)o * nblocks + lb] = s;
  }
}

}  // namespace c8
