// spr_host_main.cpp -- TEST PROGRAM: the patch builder, the fit and the sequential recovery of c8_spr.hpp over the meshes
// named on the command line, as a plain process (tests/test_spr_host.py builds it with -fsanitize=address,undefined).
// A mesh file is text: elem_type nnodes nelems, then nnodes x 3 coordinates, then nelems x elem_type node ids.
// Prints one line per mesh: "<file> ok <table entries> <checksum>" or "<file> failed <node>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibr8_amd/csrc/c8_spr.hpp"

using namespace c8;

static int run(char const* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 2;
  int et = 0, nnodes = 0, nelems = 0;
  if (std::fscanf(f, "%d %d %d", &et, &nnodes, &nelems) != 3 || (et != 3 && et != 4 && et != 8) || nnodes <= 0 || nelems <= 0) {
    std::fclose(f);
    return 2;
  }
  std::vector<double> coords((size_t)nnodes * 3);
  std::vector<int32_t> conn((size_t)nelems * et);
  bool ok = true;
  for (double& x : coords) ok = ok && std::fscanf(f, "%lf", &x) == 1;
  for (int32_t& c : conn) ok = ok && std::fscanf(f, "%d", &c) == 1 && c >= 0 && c < nnodes;
  std::fclose(f);
  if (!ok) return 2;
  int const dim = spr_dim(et), np0 = spr_np0(et), T = dim + 1;
  std::vector<int32_t> ne_ptr, ne;
  spr_node_elems(nnodes, nelems, et, conn.data(), ne_ptr, ne);
  std::vector<double> pts((size_t)nelems * np0 * dim);
  spr_points_host(et, nelems, conn.data(), coords.data(), pts.data());
  SprMesh const m{et, nnodes, nelems, coords.data(), conn.data(), ne_ptr.data(), ne.data(), 0, pts.data()};
  std::vector<int64_t> ptr((size_t)nnodes + 1);
  int bad = spr_build_all(m, ptr.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr);
  if (bad >= 0) {
    std::printf("%s failed %d\n", path, bad);
    return 0;
  }
  std::vector<int32_t> elems((size_t)ptr[nnodes]), stages((size_t)nnodes);
  std::vector<double> g((size_t)nnodes * T), h((size_t)nnodes), ratio((size_t)nnodes);
  bad = spr_build_all(m, ptr.data(), elems.data(), (int64_t)elems.size(), g.data(), h.data(), stages.data(), ratio.data());
  if (bad != -1) return 3;
  int const ncomp = 9;
  std::vector<double> field((size_t)nelems * np0 * ncomp), nodal((size_t)nnodes * ncomp), mag((size_t)nnodes * ncomp);
  for (size_t i = 0; i < field.size(); ++i) field[i] = 1. + 0.001 * (double)(i % 97);
  spr_apply_host(et, nnodes, ncomp, ptr.data(), elems.data(), g.data(), h.data(), pts.data(), coords.data(), field.data(), nodal.data(), mag.data());
  double sum = 0.;
  for (double v : nodal) sum += v;
  std::printf("%s ok %lld %.17g\n", path, (long long)elems.size(), sum);
  return 0;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int const rc = run(argv[i]);
    if (rc != 0) {
      std::fprintf(stderr, "%s: error %d\n", argv[i], rc);
      return rc;
    }
  }
  return 0;
}
