// tests/emul_hybrid/c8_emul_hybrid.cpp -- TEST INFRASTRUCTURE.
//
// hybrid_hyper_J2_plane_stress on the CPU lane emulator of tests/emul/c8_emul.cpp, which this file includes unchanged:
// the lane-group kernels K1-K6 with the network buffer in MeshTables::nn, and the weight-gradient kernel
// (calibr8_amd/csrc/c8_assemble_nn.hpp) with a serial block executor, block after block.
#include "../emul/c8_emul.cpp"

#include "../../calibr8_amd/csrc/c8_assemble_nn.hpp"

// ptrs as c8emu_call: 0 u, 1 p, 2 u_prev, 3 p_prev, 4 xi_prev, 5 xi, 6..9 A, 10 b0, 11 b1, 12 g, 13 f, 14 z_u, 15 z_p,
// 16 phi, 17 out
extern "C" int c8emu_hybrid_call(int what, int nnodes, int nelems, double const* coords, int const* conn, int const* elem_set,
                                 int nsets, int max_iters, double abs_tol, double rel_tol, double const* params,
                                 int const* active, double const* nn, double** ptrs) {
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
  if (!err.empty()) { std::fprintf(stderr, "c8emu_hybrid: %s\n", err.c_str()); return -3; }
  int status = 0;
  Call c{};
  what &= 0xff;  // the kernel-form flags of c8emu_call: the lane-group kernels only
  c.what = what;
  c.nnodes = nnodes;
  c.graph = &graph;
  c.mesh = &mesh;
  c.nchunks_out = &g_last_nchunks;
  c.nelems = nelems;
  c.mt = MeshTables{mesh.conn.data(), mesh.coords.data(), graph.nodeptr.data(), graph.pos.data(), elem_set, nullptr, params,
                    nullptr, nn};
  c.ms = ModelSettings{1., abs_tol, rel_tol, max_iters};
  c.fa = FieldArgs{ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5]};
  c.sa = SystemArgs{{{ptrs[6], ptrs[7]}, {ptrs[8], ptrs[9]}}, {ptrs[10], ptrs[11]}, &status, 0};
  c.aa = AdjointArgs{ptrs[12], ptrs[13], ptrs[14], ptrs[15], ptrs[16], ptrs[17], active, QoiArgs{1., 0., 0, nullptr, 2.}};
  if (what != K_FORWARD && what != K_RESIDUAL && what != K_ADJ_JAC && what != K_ADJ_LOCAL && what != K_GRAD && what != K_QOI) return -4;
  run<Tri3PlaneStress, HybridHyperJ2PlaneStress>(c);
  return status ? -1 : 0;
}

struct CpuBlockExec {
  template <class F> void each(F f) { for (int t = 0; t < NN_GRAD_THREADS; ++t) f(t); }
  void sync() {}
};

// the weight gradient: out[0 .. ntheta) += the sum of the blocks' partial rows, in block order (as on the device)
extern "C" int c8emu_nn_grad(int npts, int pts_per_elem, int nloc, int nparams, double abs_tol, double const* nn, double const* xi,
                             double const* phi, int const* elem_set, double const* params, int ntheta, double* out) {
  int const nblocks = nn_grad_blocks(npts);
  std::vector<double> part((size_t)nblocks * ntheta), lds(NN_LDS_SIZE);
  NnGradArgs const ga{nn, xi, phi, elem_set, params, npts, pts_per_elem, nloc, nparams, abs_tol, ntheta, part.data()};
  CpuBlockExec ex;
  for (int b = 0; b < nblocks; ++b) nn_grad_block<HybridHyperJ2PlaneStress<double>>(ex, lds.data(), ga, b);
  for (int q = 0; q < ntheta; ++q) nn_grad_reduce_entry(part.data(), nblocks, ntheta, q, out);
  return 0;
}

// s_out (NN(s_in alpha) - NN(0)) and its alpha derivative, as the models evaluate it
extern "C" void c8emu_nn_hardening(double const* nn, double alpha, double* out) { nn_hardening(nn, alpha, out[0], out[1]); }
