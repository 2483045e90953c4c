// tests/emul_vfm/c8_emul_vfm.cpp -- TEST INFRASTRUCTURE.
//
// The VFM kernels (calibr8_amd/csrc/c8_assemble_vfm.hpp) on the CPU lane emulator of tests/emul/c8_emul.cpp, which this
// file includes unchanged: the same serial executor, one lane group per element.  The per-element lane sums are added
// element by element here (the device adds them per block in a fixed order; the tests compare values, not bits).
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

// ptrs: 0 u, 1 u_prev, 2 xi_prev, 3 xi, 4 w, 5 b (or null), 6 S_prev (or null), 7 S, 8 h, 9 ivw, 10 grad
extern "C" int c8emu_vfm(int what, int nnodes, int nelems, double const* coords, int const* conn, int const* elem_set, int nsets,
                         char const* local_type, int max_iters, double abs_tol, double rel_tol, double thickness,
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
      if (std::strcmp(row.name, local_type) == 0) { vfm_run(row, what, c, va, ivw, grad); known = true; }
    }
  });
  if (!known) return -2;
  return status ? -1 : 0;
}
