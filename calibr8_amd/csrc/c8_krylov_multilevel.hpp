// c8_krylov_multilevel.hpp -- the block levels below level 1 of the aggregation preconditioners of the device solve, the
// cycle over a list of levels, and the set-up and apply of the kinds of one part (C8_PRECOND_TWO_LEVEL: a list of one
// level, C8_PRECOND_MULTILEVEL; DESIGN.md sections 13d, 13e, 13h).  Included by c8_krylov.hip inside its unnamed namespace,
// after c8_krylov_coarse.hpp and launch_sgs.
//
//   levels    level 0 is the system (node blocks, the four CSR value arrays, the aggregates and kernels of
//             c8_krylov_coarse.hpp).  Level l >= 1 has one node per aggregate of level l - 1 with NC unknowns; its graph is
//             the neighbour list of those aggregates; its matrix is block-sparse over that graph, one row-major NC x NC block
//             per graph entry (A[entry][r][c]), its vectors are node-major ([node][NC]).  The last level is dense
//             (d_kry_Ac, d_kry_cvec, coarse_invert, k_coarse_apply).  A list lv holds level k + 1 in lv[k].
//   P_l       l >= 1, never stored: the aggregate of a node, its offset d from the aggregate's centroid, the constrained
//             flags of level l.  NC x NC block: identity, plus rotation m -> translation e_m x d (pb_entry).
//   set-up    k_constrained -> k_galerkin (A_1, dense when level 1 is the last, else block-sparse) -> per level l >= 1:
//             k_level_setup (flags, inverses of the diagonal blocks) -> k_level_galerkin (A_l+1, block-sparse or dense) ->
//             coarse_invert -> k_coarse_check
//   apply     k_restrict, k_level_restrict ... -> k_coarse_apply -> per level upwards: k_level_prolong, the colour launches of
//             k_level_sgs -> k_prolong; the sweeps of level 0 (launch_sgs) follow in the caller
// With one level the loops over the block levels are empty: the launches are k_constrained, k_galerkin, coarse_invert,
// k_coarse_check and k_restrict, k_coarse_apply, k_prolong.  Every sum has a fixed order and no kernel uses a floating-point
// atomic.  levels_begin, levels_form, levels_invert, levels_bad_row and launch_level_cycle serve the kinds over parts too
// (c8_krylov_parts_levels.hpp), which keep an error discipline of their own.
constexpr int LEVEL_G = 8;  // lanes per node of k_level_sgs

// entry (r, c) of the block of P_l, l >= 1, before the constrained flags; d = x_a - centroid of the node's aggregate.  The
// translation rows are those of p_entry; a rotation or the pressure passes to itself.  r is a compile-time constant at
// every call.
template <int ND, int NRES>
__device__ __forceinline__ double pb_entry(int r, int c, double const* d) {
  return r < ND ? p_entry<ND, NRES>(r, c, d) : (r == c ? 1. : 0.);
}

struct LevelTables {  // device mirror of a block-sparse level
  int n;
  int32_t const *ptr, *adj;  // graph: entries ptr[i] .. ptr[i + 1) of node i, columns ascending, i itself among them
  double const* A;           // [entries][NC * NC]
};

// ---- set-up of a block-sparse level, one work item per node: bit r of flags[node] is set when every off-diagonal entry of
// the node's equation r is exactly 0 (the rule of k_constrained); the node's own block is inverted by the elimination of
// k_setup (Gauss-Jordan, partial pivoting by selects, every index a compile-time constant: two NC x NC blocks in
// registers).  k_setup itself is left as it is: its instructions are those of the other three kinds.
template <int NC>
__global__ void __launch_bounds__(TPB) k_level_setup(LevelTables L, double* __restrict__ minv, int32_t* __restrict__ flags, int32_t* bad) {
  int const node = blockIdx.x * TPB + threadIdx.x;
  if (node >= L.n) return;
  int const p0 = L.ptr[node], p1 = L.ptr[node + 1];
  int ks = -1, nz = 0;
  for (int e = p0; e < p1; ++e) {
    bool const self = L.adj[e] == node;
    if (self) ks = e;
    double const* blk = L.A + (size_t)e * NC * NC;
#pragma unroll
    for (int r = 0; r < NC; ++r)
#pragma unroll
      for (int cj = 0; cj < NC; ++cj)
        if (!(self && r == cj) && blk[r * NC + cj] != 0.) nz |= 1 << r;
  }
  flags[node] = ~nz & ((1 << NC) - 1);
  double a[NC][NC], inv[NC][NC];
  bool ok = ks >= 0;
  if (ks < 0) ks = p0;
#pragma unroll
  for (int r = 0; r < NC; ++r)
#pragma unroll
    for (int cj = 0; cj < NC; ++cj) {
      a[r][cj] = p1 > p0 ? L.A[(size_t)ks * NC * NC + r * NC + cj] : 0.;
      inv[r][cj] = r == cj ? 1. : 0.;
    }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
#pragma unroll
    for (int r = c + 1; r < NC; ++r) {  // after these selects row c holds the largest |entry| of column c
      bool const sw = fabs(a[r][c]) > fabs(a[c][c]);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        double const a0 = a[c][k], a1 = a[r][k], i0 = inv[c][k], i1 = inv[r][k];
        a[c][k] = sw ? a1 : a0;
        a[r][k] = sw ? a0 : a1;
        inv[c][k] = sw ? i1 : i0;
        inv[r][k] = sw ? i0 : i1;
      }
    }
    double const piv = a[c][c];
    if (piv == 0. || !finite_d(piv)) ok = false;
    double const ip = 1. / piv;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      a[c][k] *= ip;
      inv[c][k] *= ip;
    }
#pragma unroll
    for (int r = 0; r < NC; ++r) {
      if (r == c) continue;
      double const f = a[r][c];
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        a[r][k] -= f * a[c][k];
        inv[r][k] -= f * inv[c][k];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NC; ++r)
#pragma unroll
    for (int cj = 0; cj < NC; ++cj) {
      if (!finite_d(inv[r][cj])) ok = false;
      minv[(size_t)node * NC * NC + r * NC + cj] = inv[r][cj];
    }
  if (!ok) atomicMin(bad, node);  // (integer) the smallest such node of the level
}

// ---- A_l+1 = P_l^T A_l P_l for l >= 1, the ownership rule of k_galerkin: one workgroup owns the block row of aggregate I,
// a work item the tile columns q = slot * NC + c; it walks the aggregate's nodes in ascending id and each node's graph row
// in column order.  DENSE: the tile goes to the dense row-major matrix of the last level (the other entries are the zeros
// of the memset before the launch); otherwise to the block of graph entry nbr_ptr[I] + slot of level l + 1, whose graph is
// the neighbour list.
template <int ND, int NRES, bool DENSE>
__global__ void __launch_bounds__(TPB) k_level_galerkin(AggTables T, LevelTables L, double* __restrict__ out, int lda) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  extern __shared__ double tile[];
  int const I = blockIdx.x;
  int const a0 = T.ptr[I], a1 = T.ptr[I + 1], b0 = T.nbr_ptr[I];
  int const W = (T.nbr_ptr[I + 1] - b0) * NC;
  for (int q = threadIdx.x; q < W; q += TPB) {
    int const sl = q / NC, c = q % NC;
    bool const own = T.nbr[b0 + sl] == I;
    bool colnz = false;
    double acc[NC];
#pragma unroll
    for (int r = 0; r < NC; ++r) acc[r] = 0.;
    for (int a = a0; a < a1; ++a) {
      int const node = T.nodes[a];
      int const fi = T.flags[node];
      double di[ND];
#pragma unroll
      for (int e = 0; e < ND; ++e) di[e] = T.off[(size_t)node * ND + e];
      if (own) {
#pragma unroll
        for (int e = 0; e < NC; ++e)
          if (!((fi >> e) & 1) && pb_entry<ND, NRES>(e, c, di) != 0.) colnz = true;
      }
      for (int k = L.ptr[node]; k < L.ptr[node + 1]; ++k) {
        if (T.slot[k] != sl) continue;
        int const cn = L.adj[k];
        int const fj = T.flags[cn];
        double dj[ND], pj[NC], w[NC];
#pragma unroll
        for (int e = 0; e < ND; ++e) dj[e] = T.off[(size_t)cn * ND + e];
#pragma unroll
        for (int e = 0; e < NC; ++e) pj[e] = ((fj >> e) & 1) ? 0. : pb_entry<ND, NRES>(e, c, dj);
        double const* blk = L.A + (size_t)k * NC * NC;
#pragma unroll
        for (int ri = 0; ri < NC; ++ri) {
          double s = 0.;
#pragma unroll
          for (int e = 0; e < NC; ++e) s += blk[ri * NC + e] * pj[e];
          w[ri] = s;
        }
#pragma unroll
        for (int r = 0; r < NC; ++r) {
          double s = 0.;
#pragma unroll
          for (int ri = 0; ri < NC; ++ri) s += (((fi >> ri) & 1) ? 0. : pb_entry<ND, NRES>(ri, r, di)) * w[ri];
          acc[r] += s;
        }
      }
    }
    bool const unit = own && !colnz;
#pragma unroll
    for (int r = 0; r < NC; ++r) tile[r * W + q] = (unit && r == c) ? 1. : acc[r];
  }
  __syncthreads();
  int32_t const* nbr = T.nbr + b0;
  for (int idx = threadIdx.x; idx < NC * W; idx += TPB) {
    int const r = idx / W, q = idx % W;
    // (DENSE: row I * NC + r, column block of the neighbour; otherwise the block of graph entry b0 + slot)
    size_t const at = DENSE ? ((size_t)I * NC + r) * lda + (size_t)nbr[q / NC] * NC : ((size_t)(b0 + q / NC) * NC + r) * NC;
    out[at + q % NC] = tile[idx];
  }
}

// ---- one colour of the block Gauss-Seidel sweep on a block-sparse level, the structure of k_sgs_color:
//   x_i <- x_i + D_i^-1 (rhs_i - sum_j A_ij x_j)   for the nodes i of list[0 .. nlist), j over the node's whole graph row.
// LEVEL_G = 8 lanes per node for every NC: lane l takes the graph entries l, l + 8, ... and all NC rows of their blocks, a
// butterfly over the 8 lanes, then lane r < NC forms row r of the update.  With NC = 7 one lane in 8 idles in that last
// step (7 multiply-adds of the 49 + 49 deg / 8 a lane does), none in the loop over the entries; the launch is bound by its
// latency on levels of a few hundred nodes, not by these lanes.  x is read and written in one launch: a plain pointer.
template <int NC>
__global__ void __launch_bounds__(TPB) k_level_sgs(int32_t const* __restrict__ list, int nlist, LevelTables L, double const* __restrict__ minv,
                                                   double const* __restrict__ rhs, double* x, KryScalars const* S) {
  constexpr int NPB = TPB / LEVEL_G;
  if (S->stop) return;
  int const li = blockIdx.x * NPB + threadIdx.x / LEVEL_G, lane = threadIdx.x % LEVEL_G;
  bool const live = li < nlist;
  int const node = live ? list[li] : 0;
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.;
  if (live) {
    for (int e = L.ptr[node] + lane; e < L.ptr[node + 1]; e += LEVEL_G) {
      double const* xc = x + (size_t)L.adj[e] * NC;
      double const* blk = L.A + (size_t)e * NC * NC;
      double xv[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) xv[c] = xc[c];
#pragma unroll
      for (int r = 0; r < NC; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[r] += blk[r * NC + c] * xv[c];
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k)
    for (int o = LEVEL_G / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, LEVEL_G);
  if (live && lane < NC) {
    double const* m = minv + (size_t)node * NC * NC + lane * NC;
    double d = 0.;
#pragma unroll
    for (int cj = 0; cj < NC; ++cj) d += m[cj] * (rhs[(size_t)node * NC + cj] - acc[cj]);
    x[(size_t)node * NC + lane] += d;
  }
}

// ---- r_l+1 = P_l^T v between block levels: one wavefront per aggregate, the lanes and the butterfly of k_restrict
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_level_restrict(int nagg, AggTables T, double const* __restrict__ v, double* __restrict__ rc,
                                                        KryScalars const* S) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  if (S->stop) return;
  int const I = blockIdx.x * (TPB / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.;
  if (I < nagg) {
    for (int a = T.ptr[I] + lane; a < T.ptr[I + 1]; a += 64) {
      int const node = T.nodes[a];
      int const f = T.flags[node];
      double d[ND], vv[NC];
#pragma unroll
      for (int e = 0; e < ND; ++e) d[e] = T.off[(size_t)node * ND + e];
#pragma unroll
      for (int e = 0; e < NC; ++e) vv[e] = ((f >> e) & 1) ? 0. : v[(size_t)node * NC + e];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < NC; ++e) acc[c] += pb_entry<ND, NRES>(e, c, d) * vv[e];
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
  if (I < nagg && lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) rc[(size_t)I * NC + c] = acc[c];
  }
}

// ---- x_l = P_l e between block levels, one work item per node: the start of the level's sweeps
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_level_prolong(int n, AggTables T, double const* __restrict__ e, double* __restrict__ x,
                                                       KryScalars const* S) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  if (S->stop) return;
  int const node = blockIdx.x * TPB + threadIdx.x;
  if (node >= n) return;
  int const f = T.flags[node];
  double const* ea = e + (size_t)T.agg_of[node] * NC;
  double d[ND], ev[NC];
#pragma unroll
  for (int k = 0; k < ND; ++k) d[k] = T.off[(size_t)node * ND + k];
#pragma unroll
  for (int c = 0; c < NC; ++c) ev[c] = ea[c];
#pragma unroll
  for (int r = 0; r < NC; ++r) {
    double s = 0.;
#pragma unroll
    for (int c = 0; c < NC; ++c) s += pb_entry<ND, NRES>(r, c, d) * ev[c];
    x[(size_t)node * NC + r] = ((f >> r) & 1) ? 0. : s;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

constexpr int ML_COARSE_MAX = 1024;  // default of c8_krylov_set_multilevel
constexpr int ML_MAX_LEVELS = 8;

inline int ml_coarse_max(c8_ctx const* c) { return c->kry_ml_coarse_max > 0 ? c->kry_ml_coarse_max : ML_COARSE_MAX; }
inline int ml_max_levels(c8_ctx const* c) { return c->kry_ml_max_levels > 0 ? c->kry_ml_max_levels : ML_MAX_LEVELS; }

void free_level_list(std::vector<c8_kry_level>& lv) {
  for (c8_kry_level& L : lv) {
    void* bufs[] = {L.d_graph, L.d_agg, L.d_off, L.d_flags, L.d_colors, L.d_A, L.d_minv, L.d_vec};
    for (void* b : bufs)
      if (b) (void)hipFree(b);
  }
  lv.clear();
}
void free_levels(c8_ctx* c) {
  free_level_list(c->kry_levels);
  c->kry_ml_built = false;
}

template <class T>
int upload(T** dst, std::vector<T> const& src) {
  *dst = nullptr;
  if (src.empty()) return C8_OK;
  C8_HIP(hipMalloc((void**)dst, src.size() * sizeof(T)));
  C8_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return C8_OK;
}

// The levels below level 1 of a list that holds level 1 as (n, graph, positions): lv[k] is level k + 1.  Another level is
// built while the last one has more than coarse_max unknowns, fewer than max_levels levels exist (level 0 counts) and
// aggregation still reduces the node count.  Host rules only: the same list in gives the same levels out.
int extend_levels(c8_ctx* c, std::vector<c8_kry_level>& lv) {
  int const nd = c->ndims, nc = coarse_columns(c);
  int rc;
  while ((long long)lv.back().n * nc > ml_coarse_max(c) && (int)lv.size() + 1 < ml_max_levels(c)) {
    c8_kry_level& L = lv.back();
    Aggregates H = aggregate_graph(L.n, nd, L.gp, L.ga, L.x.data());
    if (H.nagg >= L.n) break;
    L.nagg = H.nagg, L.max_nbr = H.max_nbr, L.agg_of = H.agg;
    color_graph(L.n, L.gp, L.ga, &L.color_ptr, &L.color_nodes);
    std::vector<int32_t> graph(L.gp);
    graph.insert(graph.end(), L.ga.begin(), L.ga.end());
    if ((rc = upload(&L.d_graph, graph)) != C8_OK) return rc;
    if ((rc = upload_aggregates(H, &L.d_agg, L.agg_at, &L.d_off)) != C8_OK) return rc;
    if ((rc = upload(&L.d_colors, L.color_nodes)) != C8_OK) return rc;
    size_t const nnc = (size_t)L.n * nc;
    C8_HIP(hipMalloc((void**)&L.d_flags, (size_t)L.n * sizeof(int32_t)));
    C8_HIP(hipMalloc((void**)&L.d_A, L.ga.size() * nc * nc * sizeof(double)));
    C8_HIP(hipMalloc((void**)&L.d_minv, nnc * nc * sizeof(double)));
    C8_HIP(hipMalloc((void**)&L.d_vec, 2 * nnc * sizeof(double)));
    c8_kry_level next;
    next.n = H.nagg;
    next.gp = std::move(H.nbr_ptr), next.ga = std::move(H.nbr), next.x = std::move(H.centroid);
    lv.push_back(std::move(next));
  }
  return C8_OK;
}

// The levels below level 0 from the aggregates of level 0, once per setting of c8_krylov_set_multilevel: kry_levels[k] is
// level k + 1.  Level 1 always exists: a copy of the two-level kind's one entry (host data only); the levels below it by
// extend_levels.
int build_levels(c8_ctx* c) {
  if (c->kry_ml_built) return C8_OK;
  free_levels(c);
  int rc = build_aggregates(c);
  if (rc != C8_OK) return rc;
  c->kry_levels = c->kry_agg_levels;
  if ((rc = extend_levels(c, c->kry_levels)) != C8_OK) return rc;
  c->kry_ml_built = true;
  return C8_OK;
}

inline AggTables level_agg_tables(c8_kry_level const& L) {
  int32_t const* b = L.d_agg;
  size_t const* o = L.agg_at;
  return AggTables{b + o[0], b + o[1], b + o[2], b + o[3], b + o[4], b + o[5], L.d_off, L.d_flags};
}
inline LevelTables level_tables(c8_kry_level const& L) { return LevelTables{L.n, L.d_graph, L.d_graph + L.n + 1, L.d_A}; }

// what a call must refuse before any device work of the multilevel kind: a halo, a last level above the cap of the dense
// solve
int multilevel_refusals(c8_ctx* c, char const* who) {
  if (c->halo)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": the multilevel preconditioner (C8_PRECOND_MULTILEVEL) is not supported with a halo "
                                    "attached to the context: its coarse spaces cover one part only");
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, std::string(who) + ": empty mesh");
  int const rc = build_levels(c);
  if (rc != C8_OK) return rc;
  int const nl = (int)c->kry_levels.size();
  long long const n = (long long)c->kry_levels.back().n * coarse_columns(c);
  if (n > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED,
                std::string(who) + ": the multilevel preconditioner solves its last level densely: level " + std::to_string(nl) + " has n = " +
                    std::to_string(n) + " unknowns (" + std::to_string(c->kry_levels.back().n) + " aggregates), which exceeds the cap of " +
                    std::to_string(COARSE_CAP) + "; " +
                    (nl + 1 >= ml_max_levels(c) ? "max_levels = " + std::to_string(ml_max_levels(c)) + " (c8_krylov_set_multilevel) ends the recursion there"
                                                    : std::string("aggregation no longer reduces the node count")));
  return C8_OK;
}

// The numeric set-up of a list of levels (lv[k] is level k + 1, the last one dense) in three steps, shared by the kinds of
// one part and the kinds over parts (c8_krylov_parts_levels.hpp), which differ in how A_1 is completed between the first
// two.  levels_begin: the buffers of the last level and the status words `info` (getrf, getri, first row of the inverse
// that is not finite, then per level k + 1 its bad block), r_c and e zeroed.
template <int NC>
int levels_begin(c8_ctx* c, std::vector<c8_kry_level> const& lv, std::vector<int32_t>* h_info, int32_t** info) {
  int const nl = (int)lv.size(), n = lv.back().n * NC, lda = (n + 1) & ~1;
  int rc;
  if ((rc = grow(&c->d_kry_Ac, &c->kry_Ac_n, (size_t)n * lda)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_cvec, &c->kry_cvec_n, 2 * (size_t)lda)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_ipiv, &c->kry_ipiv_n, (size_t)n + 4 + nl)) != C8_OK) return rc;
  *info = c->d_kry_ipiv + n;
  h_info->assign(3 + nl, INT_MAX);
  (*h_info)[0] = (*h_info)[1] = 0;
  C8_HIP(hipMemcpyAsync(*info, h_info->data(), h_info->size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  C8_HIP(hipMemsetAsync(c->d_kry_cvec, 0, 2 * (size_t)lda * sizeof(double), c->stream));
  return C8_OK;
}

// levels_form: with A_1 in place, level k + 1 -> level k + 2 for every level up to `upto` (k_level_setup, k_level_galerkin)
template <int ND, int NRES>
int levels_form(c8_ctx* c, std::vector<c8_kry_level> const& lv, int upto, int32_t* info) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  int const nl = (int)lv.size(), n = lv.back().n * NC, lda = (n + 1) & ~1;
  hipStream_t const st = c->stream;
  for (int k = 0; k + 1 < nl && k + 1 < upto; ++k) {
    c8_kry_level const& L = lv[k];
    hipLaunchKernelGGL((k_level_setup<NC>), dim3((L.n + TPB - 1) / TPB), dim3(TPB), 0, st, level_tables(L), L.d_minv, L.d_flags, info + 3 + k);
    C8_HIP(hipGetLastError());
    size_t const lds = (size_t)L.max_nbr * NC * NC * sizeof(double);
    if (k + 2 == nl)
      hipLaunchKernelGGL((k_level_galerkin<ND, NRES, true>), dim3(L.nagg), dim3(TPB), lds, st, level_agg_tables(L), level_tables(L), c->d_kry_Ac, lda);
    else
      hipLaunchKernelGGL((k_level_galerkin<ND, NRES, false>), dim3(L.nagg), dim3(TPB), lds, st, level_agg_tables(L), level_tables(L), lv[k + 1].d_A, 0);
    C8_HIP(hipGetLastError());
  }
  return C8_OK;
}

// levels_invert: the checked inverse of the last level; the status words come back in h_info (a host read)
template <int NC>
int levels_invert(c8_ctx* c, std::vector<c8_kry_level> const& lv, int32_t* info, std::vector<int32_t>* h_info) {
  int const n = lv.back().n * NC, lda = (n + 1) & ~1;
  hipStream_t const st = c->stream;
  int rc;
  if ((rc = coarse_invert(c, n, lda, c->d_kry_Ac, c->d_kry_ipiv, info)) != C8_OK) return rc;
  int const nb_c = (int)std::min<size_t>(((size_t)n * lda + TPB - 1) / TPB, (size_t)UPDATE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_coarse_check, dim3(nb_c), dim3(TPB), 0, st, n, lda, c->d_kry_Ac, info + 2);
  C8_HIP(hipGetLastError());
  C8_HIP(hipMemcpyAsync(h_info->data(), info, h_info->size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  C8_HIP(hipStreamSynchronize(st));
  return C8_OK;
}
// ... the bad row of the last level in those words (-1: none)
inline int levels_bad_row(std::vector<int32_t> const& h) { return h[0] > 0 ? h[0] - 1 : h[1] > 0 ? h[1] - 1 : h[2] != INT_MAX ? h[2] : -1; }

// The part's block rows of A_1 for the matrix of q -- dense into d_kry_Ac when level 1 is the last level, else block-sparse
// into lv[0].d_A from the part's first row.  The caller has zeroed the target and formed the flags.
template <int ND, int NRES>
hipError_t launch_level0_galerkin(Solve const& q) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  c8_ctx const* c = q.c;
  std::vector<c8_kry_level> const& lv = *q.lv;
  Level0 const& l0 = q.l0;
  if (l0.nagg <= 0) return hipSuccess;
  size_t const lds = (size_t)l0.max_nbr * NC * NC * sizeof(double);
  int const n = lv.back().n * NC, lda = (n + 1) & ~1;
  if (lv.size() == 1)
    hipLaunchKernelGGL((k_galerkin<ND, NRES, false>), dim3(l0.nagg), dim3(TPB), lds, c->stream, l0.T, l0.base, c->d_nodeptr, c->d_nodeadj, q.A, c->d_kry_Ac, lda);
  else
    hipLaunchKernelGGL((k_galerkin<ND, NRES, true>), dim3(l0.nagg), dim3(TPB), lds, c->stream, l0.T, l0.base, c->d_nodeptr, c->d_nodeadj, q.A,
                       lv[0].d_A + (size_t)lv[0].gp[l0.base] * NC * NC, 0);
  return hipGetLastError();
}

// The levels of q (q.lv, q.l0: use_levels) for the matrix of q: A_1 .. A_upto (upto < 0: all levels, then the checked inverse
// of the last one).  The two-level kind and the multilevel kind differ in the length of the list and in the wording of
// their messages (q.multi).  Needs the kind's refusals passed.
template <int ND, int NRES, int G>
int levels_setup(Solve const& q, int upto) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  c8_ctx* c = q.c;
  std::vector<c8_kry_level> const& lv = *q.lv;
  int const nl = (int)lv.size();  // level k + 1 is lv[k]; the last one is dense
  int const n = lv.back().n * NC, lda = (n + 1) & ~1;
  bool const invert = upto < 0;
  if (invert) upto = nl;
  int worst = q.l0.max_nbr;
  for (int k = 0; k + 1 < nl; ++k) worst = std::max(worst, lv[k].max_nbr);
  if ((size_t)worst * NC * NC * sizeof(double) > GALERKIN_LDS)
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov: an aggregate has " + std::to_string(worst) + " neighbouring aggregates: the block row of " +
                                    (q.multi ? "a" : "the") + " coarse matrix does not fit the tile of k_galerkin");
  int rc;
  hipStream_t const st = c->stream;
  int32_t* info = nullptr;
  std::vector<int32_t> h_info;
  if ((rc = levels_begin<NC>(c, lv, &h_info, &info)) != C8_OK) return rc;
  int const nb_g = (q.nn + TPB / G - 1) / (TPB / G);
  hipLaunchKernelGGL((k_constrained<ND, NRES, G>), dim3(xcd_grid(nb_g)), dim3(TPB), 0, st, q.nn, nb_g, c->d_nodeptr, c->d_nodeadj, q.A, c->d_kry_cflags);
  C8_HIP(hipGetLastError());
  if (upto >= nl) C8_HIP(hipMemsetAsync(c->d_kry_Ac, 0, (size_t)n * lda * sizeof(double), st));
  C8_HIP((launch_level0_galerkin<ND, NRES>(q)));
  if ((rc = levels_form<ND, NRES>(c, lv, upto, info)) != C8_OK) return rc;
  if (!invert) return C8_OK;
  if ((rc = levels_invert<NC>(c, lv, info, &h_info)) != C8_OK) return rc;
  for (int k = 0; k + 1 < nl; ++k)
    if (h_info[3 + k] != INT_MAX)
      return fail(C8_ERR_ARG, "c8_krylov: the diagonal block of aggregate " + std::to_string(h_info[3 + k]) + " on level " + std::to_string(k + 1) +
                              " of the multilevel preconditioner is singular or not finite");
  int const bad = levels_bad_row(h_info);
  if (bad < 0) return C8_OK;
  if (!q.multi)
    return fail(C8_ERR_ARG, "c8_krylov: the coarse matrix of the two-level preconditioner is singular or not finite at aggregate " +
                            std::to_string(bad / NC) + " (coarse row " + std::to_string(bad) + " of " + std::to_string(n) + ")");
  return fail(C8_ERR_ARG, "c8_krylov: the matrix of level " + std::to_string(nl) + " (the last) of the multilevel preconditioner is singular or not finite at aggregate " +
                          std::to_string(bad / NC) + " (row " + std::to_string(bad) + " of " + std::to_string(n) + ")");
}

// right-hand side and iterate of level k + 1 of a list: the two halves of the level's vector, of d_kry_cvec on the last level
template <int NC>
inline double* level_rhs(c8_ctx const* c, std::vector<c8_kry_level> const& lv, int k) { return k + 1 == (int)lv.size() ? c->d_kry_cvec : lv[k].d_vec; }
template <int NC>
inline double* level_x(c8_ctx const* c, std::vector<c8_kry_level> const& lv, int k) {
  return k + 1 == (int)lv.size() ? c->d_kry_cvec + ((lv[k].n * NC + 1) & ~1) : lv[k].d_vec + (size_t)lv[k].n * NC;
}

// e_1 = M_1^-1 r_1 on a list of levels, r_1 and e_1 in level_rhs(0) and level_x(0): down the levels, the dense solve, up
// again with the sweeps of every block level, level 1 included.  The dense solve forms the rows [row0, row0 + nrows) of the
// last level's e: all of them, or -- over parts with level 1 the last level -- the rows of the rank's own aggregates.
template <int ND, int NRES>
hipError_t launch_level_cycle(c8_ctx const* c, std::vector<c8_kry_level> const& lv, int row0, int nrows, KryScalars const* S) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  int const nl = (int)lv.size(), n = lv.back().n * NC, lda = (n + 1) & ~1, wpb = TPB / 64;
  hipStream_t const st = c->stream;
  auto rhs_of = [&](int k) { return level_rhs<NC>(c, lv, k); };
  auto x_of = [&](int k) { return level_x<NC>(c, lv, k); };
  for (int k = 0; k + 1 < nl; ++k)
    hipLaunchKernelGGL((k_level_restrict<ND, NRES>), dim3((lv[k].nagg + wpb - 1) / wpb), dim3(TPB), 0, st, lv[k].nagg, level_agg_tables(lv[k]), rhs_of(k),
                       rhs_of(k + 1), S);
  if (nrows > 0)
    hipLaunchKernelGGL(k_coarse_apply, dim3((nrows + wpb - 1) / wpb), dim3(TPB), 0, st, row0, nrows, lda, c->d_kry_Ac, rhs_of(nl - 1), x_of(nl - 1), S);
  for (int k = nl - 2; k >= 0; --k) {
    c8_kry_level const& L = lv[k];
    hipLaunchKernelGGL((k_level_prolong<ND, NRES>), dim3((L.n + TPB - 1) / TPB), dim3(TPB), 0, st, L.n, level_agg_tables(L), x_of(k + 1), x_of(k), S);
    int const ncol = (int)L.color_ptr.size() - 1;
    auto color = [&](int j) {
      int const lo = L.color_ptr[j], m = L.color_ptr[j + 1] - lo, npb = TPB / LEVEL_G;
      hipLaunchKernelGGL((k_level_sgs<NC>), dim3((m + npb - 1) / npb), dim3(TPB), 0, st, L.d_colors + lo, m, level_tables(L), L.d_minv, rhs_of(k), x_of(k), S);
    };
    for (int s = 0; s < c->kry_sweeps; ++s) {
      for (int j = 0; j < ncol; ++j) color(j);
      for (int j = ncol - 2; j >= 0; --j) color(j);
    }
  }
  return hipGetLastError();
}

// x = P_0 M_1^-1 P_0^T rhs on the levels of q: k_restrict, the cycle over the levels, k_prolong; the caller's sweeps on
// level 0 start from this x
template <int ND, int NRES>
hipError_t levels_apply(Solve const& q, double const* rhs, double* x) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  c8_ctx const* c = q.c;
  std::vector<c8_kry_level> const& lv = *q.lv;
  Level0 const& l0 = q.l0;
  int const wpb = TPB / 64;
  hipStream_t const st = c->stream;
  hipLaunchKernelGGL((k_restrict<ND, NRES>), dim3((l0.total + wpb - 1) / wpb), dim3(TPB), 0, st, l0.total, l0.base, l0.nagg, l0.T, q.nn, rhs,
                     level_rhs<NC>(c, lv, 0), q.S);
  hipError_t const err = launch_level_cycle<ND, NRES>(c, lv, 0, lv.back().n * NC, q.S);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((k_prolong<ND, NRES>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, st, l0.nown, q.nn, q.nb_node, l0.T, level_x<NC>(c, lv, 0), x, q.S);
  return hipGetLastError();
}

// what c8_krylov_level_matrix refuses of a list: a level that is not there, a dense copy above the cap
inline int level_matrix_refusals(std::vector<c8_kry_level> const& lv, int level, int nc) {
  int const nl = (int)lv.size();
  if (level < 1 || level > nl)
    return fail(C8_ERR_ARG, "c8_krylov_level_matrix: level " + std::to_string(level) + " is not one of the levels 1 .. " + std::to_string(nl));
  long long const nlong = (long long)lv[level - 1].n * nc;
  if (nlong > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov_level_matrix: level " + std::to_string(level) + " has " + std::to_string(nlong) +
                                    " unknowns: a dense copy is refused above the cap of " + std::to_string(COARSE_CAP));
  return C8_OK;
}

// the dense copy of level `level` of a list on the host, after a set-up up to that level (the copy itself is the caller's:
// C8_HIP, or the notes of Parts): the last level from d_kry_Ac by rows, a block-sparse one spread from its blocks
inline hipError_t level_copy_start(c8_ctx const* c, std::vector<c8_kry_level> const& lv, int level, int nc, double* out_host, std::vector<double>* blocks) {
  c8_kry_level const& L = lv[level - 1];
  int const n = L.n * nc, lda = (n + 1) & ~1;
  if (level == (int)lv.size())
    return hipMemcpy2DAsync(out_host, (size_t)n * sizeof(double), c->d_kry_Ac, (size_t)lda * sizeof(double), (size_t)n * sizeof(double), n,
                            hipMemcpyDeviceToHost, c->stream);
  blocks->resize(L.ga.size() * nc * nc);
  return hipMemcpyAsync(blocks->data(), L.d_A, blocks->size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
}
inline void level_copy_finish(std::vector<c8_kry_level> const& lv, int level, int nc, double* out_host, std::vector<double> const& blocks) {
  if (level == (int)lv.size()) return;
  c8_kry_level const& L = lv[level - 1];
  size_t const n = (size_t)L.n * nc;
  std::fill(out_host, out_host + n * n, 0.);
  for (int i = 0; i < L.n; ++i)
    for (int32_t e = L.gp[i]; e < L.gp[i + 1]; ++e)
      for (int r = 0; r < nc; ++r)
        for (int k = 0; k < nc; ++k) out_host[((size_t)i * nc + r) * n + (size_t)L.ga[e] * nc + k] = blocks[((size_t)e * nc + r) * nc + k];
}
