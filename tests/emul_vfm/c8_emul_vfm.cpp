// tests/emul_vfm/c8_emul_vfm.cpp -- TEST INFRASTRUCTURE.
//
// The VFM kernels (calibr8_amd/csrc/c8_assemble_vfm.hpp) on the CPU lane emulator of tests/emul/c8_emul.cpp, which this
// file includes unchanged: the same serial executor, one lane group per element.  c8emu_vfm adds the per-element lane sums
// element by element; c8emu_vfm_blocks adds them as the device does, per block and then over the blocks in a fixed order
// (the tests compare values, not bits).
#include "../emul/c8_emul.cpp"

#include "../../calibr8_amd/csrc/c8_assemble_vfm.hpp"

enum { VFM_POWER = 0, VFM_FORWARD_SENS = 1, VFM_ADJOINT = 2 };

template <template <class> class ModelT>
static void vfm_run(ModelTag<ModelT>, int what, Call const& c, VfmArgs const& va, double* ivw, double* grad) {
  using E = Tri3PlaneStress;
  GroupShared<E, ModelT<Dual>::NLOC> sh;
  auto* ex = new CpuExec<VfmLane<E, ModelT>, E::NDOF>();
  for (int e = 0; e < c.nelems; ++e) {
    if (what == VFM_ADJOINT) vfm_adjoint_element<E, ModelT>(*ex, sh, c.mt, c.ms, c.fa, va, c.sa, e);
    else if (what == VFM_FORWARD_SENS) vfm_power_element<E, ModelT, true>(*ex, sh, c.mt, c.ms, c.fa, va, c.sa, e);
    else vfm_power_element<E, ModelT, false>(*ex, sh, c.mt, c.ms, c.fa, va, c.sa, e);
    int32_t const* act = va.active + (c.mt.elem_set ? c.mt.elem_set[e] : 0) * 10;
    for (int k = 0; k < E::NDOF; ++k) {
      if (ivw) *ivw += ex->lanes[k].acc_v;
      if (grad && k < act[1]) grad[act[0] + k] += ex->lanes[k].acc_g;
    }
  }
  delete ex;
}

// The same elements in the blocks of the device launch, through the routines that route the lane sums on the device
// (c8_assemble_vfm.hpp: vfm_group_sums, vfm_block_sums), then the partials summed in the order of k_vfm_reduce.  The
// launch itself is restated here, quoted from the source and not included from it:
//   c8_kernels.hip:694 `constexpr int VBLOCK = 64`, :698 `GPB = VBLOCK / E::NDOF`, :704-705 `gib = threadIdx.x / E::NDOF,
//   k = threadIdx.x % E::NDOF; gi = lb * GPB + gib`, :706-715 a group runs its element or, past the end, leaves zeros,
//   :717 `vfm_block_sums(red, threadIdx.x, VBLOCK, KIND != 2, KIND != 0 ? va.nact : 0, part, lb, nblocks)`, :722 `nblocks =
//   (a.count + GPB - 1) / GPB`;
//   c8_vfm.hip:21 `REDUCE_THREADS = 256`, :28 thread t sums the blocks t, t + 256, ..., :31-34 the halving tree, :37
//   `*dst += s[0]`, :59-60 the outputs and the size of the partials buffer, :73 no sum without outputs or elements.
// The block's sums and the partials start as NaN: a group, an output or a block that is left out shows in the result.
template <template <class> class ModelT>
static void vfm_run_blocks(ModelTag<ModelT>, int what, Call const& c, VfmArgs const& va, double* ivw, double* grad) {
  using E = Tri3PlaneStress;
  constexpr int VBLOCK = 64, GPB = VBLOCK / E::NDOF, REDUCE_THREADS = 256;
  double const stale = std::nan("");
  int const nblocks = (c.nelems + GPB - 1) / GPB;
  bool const has_v = what != VFM_ADJOINT;
  int const nact = what != VFM_POWER ? va.nact : 0;
  int const nout = (has_v ? 1 : 0) + nact;
  std::vector<double> part((size_t)(nout > 0 ? nout : 1) * (size_t)(nblocks > 0 ? nblocks : 1), stale);
  GroupShared<E, ModelT<Dual>::NLOC> sh;
  auto* ex = new CpuExec<VfmLane<E, ModelT>, E::NDOF>();
  auto* red = new VfmBlockSums<GPB, E::NDOF>();
  for (int lb = 0; lb < nblocks; ++lb) {
    for (int g = 0; g < GPB; ++g) {
      red->ofs[g] = -1;
      red->n[g] = E::NDOF;
      for (int k = 0; k < E::NDOF; ++k) red->v[g][k] = red->g[g][k] = stale;
    }
    for (int gib = 0; gib < GPB; ++gib) {
      int const gi = lb * GPB + gib;
      if (gi < c.nelems) {
        if (what == VFM_ADJOINT) vfm_adjoint_element<E, ModelT>(*ex, sh, c.mt, c.ms, c.fa, va, c.sa, gi);
        else if (what == VFM_FORWARD_SENS) vfm_power_element<E, ModelT, true>(*ex, sh, c.mt, c.ms, c.fa, va, c.sa, gi);
        else vfm_power_element<E, ModelT, false>(*ex, sh, c.mt, c.ms, c.fa, va, c.sa, gi);
        int32_t const* act = va.active + (c.mt.elem_set ? c.mt.elem_set[gi] : 0) * 10;
        for (int k = 0; k < E::NDOF; ++k) vfm_group_sums(*red, gib, k, ex->lanes[k].acc_v, ex->lanes[k].acc_g, act[0], act[1]);
      } else {
        for (int k = 0; k < E::NDOF; ++k) vfm_group_sums(*red, gib, k, 0., 0., 0, 0);
      }
    }
    for (int t = 0; t < VBLOCK; ++t) vfm_block_sums(*red, t, VBLOCK, has_v, nact, part.data(), lb, nblocks);
  }
  delete red;
  delete ex;
  if (nout <= 0 || c.nelems <= 0) return;
  int const nv = has_v ? 1 : 0;
  for (int o = 0; o < nout; ++o) {
    double s[REDUCE_THREADS];
    for (int t = 0; t < REDUCE_THREADS; ++t) {
      double a = 0.;
      for (int b = t; b < nblocks; b += REDUCE_THREADS) a += part[(size_t)o * nblocks + b];
      s[t] = a;
    }
    for (int w = REDUCE_THREADS / 2; w > 0; w >>= 1)
      for (int t = 0; t < w; ++t) s[t] += s[t + w];
    double* dst = (o < nv) ? ivw : grad + (o - nv);
    *dst += s[0];
  }
}

static int vfm_entry(bool blocks, int what, int nnodes, int nelems, double const* coords, int const* conn, int const* elem_set,
                     int nsets, char const* local_type, int max_iters, double abs_tol, double rel_tol, double thickness,
                     double const* params, int const* active, int nact, double cm, double** ptrs);

// ptrs: 0 u, 1 u_prev, 2 xi_prev, 3 xi, 4 w, 5 b (or null), 6 S_prev (or null), 7 S, 8 h, 9 ivw, 10 grad
extern "C" int c8emu_vfm(int what, int nnodes, int nelems, double const* coords, int const* conn, int const* elem_set, int nsets,
                         char const* local_type, int max_iters, double abs_tol, double rel_tol, double thickness,
                         double const* params, int const* active, int nact, double cm, double** ptrs) {
  return vfm_entry(false, what, nnodes, nelems, coords, conn, elem_set, nsets, local_type, max_iters, abs_tol, rel_tol, thickness,
                   params, active, nact, cm, ptrs);
}

// c8emu_vfm with the sums formed as the device forms them (vfm_run_blocks); same arguments
extern "C" int c8emu_vfm_blocks(int what, int nnodes, int nelems, double const* coords, int const* conn, int const* elem_set,
                                int nsets, char const* local_type, int max_iters, double abs_tol, double rel_tol, double thickness,
                                double const* params, int const* active, int nact, double cm, double** ptrs) {
  return vfm_entry(true, what, nnodes, nelems, coords, conn, elem_set, nsets, local_type, max_iters, abs_tol, rel_tol, thickness,
                   params, active, nact, cm, ptrs);
}

static int vfm_entry(bool blocks, int what, int nnodes, int nelems, double const* coords, int const* conn, int const* elem_set,
                     int nsets, char const* local_type, int max_iters, double abs_tol, double rel_tol, double thickness,
                     double const* params, int const* active, int nact, double cm, double** ptrs) {
  HostMesh mesh;
  HostGraph graph;
  mesh.elem_type = C8_TRI3;
  mesh.nn = 3;
  mesh.nnodes = nnodes;
  mesh.nelems = nelems;
  mesh.nsets = nsets;
  mesh.coords.assign(coords, coords + (size_t)nnodes * 3);
  mesh.conn.assign(conn, conn + (size_t)nelems * 3);
  std::string const err = build_node_graph(mesh, graph);
  if (!err.empty()) { std::fprintf(stderr, "c8emu_vfm: %s\n", err.c_str()); return -3; }
  int status = 0;
  Call c{};
  c.nelems = nelems;
  c.mt = MeshTables{mesh.conn.data(), mesh.coords.data(), graph.nodeptr.data(), graph.pos.data(), elem_set, nullptr, params};
  c.ms = ModelSettings{1., abs_tol, rel_tol, max_iters};
  c.ms.thickness = thickness;
  c.fa = FieldArgs{ptrs[0], nullptr, ptrs[1], nullptr, ptrs[2], ptrs[3]};
  c.sa = SystemArgs{{{nullptr, nullptr}, {nullptr, nullptr}}, {ptrs[5], nullptr}, &status, 0};
  VfmArgs const va{ptrs[4], ptrs[6], ptrs[7], ptrs[8], cm, active, nact};
  double* ivw = what == VFM_ADJOINT ? nullptr : ptrs[9];
  double* grad = what == VFM_POWER ? nullptr : ptrs[10];
  bool known = false;
  visit_models([&](auto row) {  // the plane-stress rows of the model table, but those with network weights (as the library)
    using R = decltype(row);
    if constexpr (R::plane_stress && !has_embedded<typename R::Real>::value) {
      if (std::strcmp(row.name, local_type) == 0) {
        if (blocks) vfm_run_blocks(row, what, c, va, ivw, grad);
        else vfm_run(row, what, c, va, ivw, grad);
        known = true;
      }
    }
  });
  if (!known) return -2;
  return status ? -1 : 0;
}
