// c8_krylov_parts_multilevel.hpp -- the multilevel preconditioner over the parts of a multi-part mesh
// (C8_PRECOND_MULTILEVEL_PARTS in include/c8.h).  Included by c8_krylov.hip inside its unnamed
// namespace, after c8_krylov_parts_coarse.hpp (level 0: the per-part aggregates, the imported P_0, k_restrict_parts,
// k_prolong_own, parts_agree) and c8_krylov_multilevel.hpp (the block-sparse levels and their kernels), which it joins.
//
//   level 0      distributed, the level 0 of C8_PRECOND_TWO_LEVEL_PARTS unchanged (parts_aggregates, parts_coarse_build)
//   level 1      one node per aggregate of any rank (global id = base of the rank + local id).  Its graph (the neighbour
//                lists parts_coarse_build forms for the rank's own aggregates) and its positions (the centroids) are
//                REPLICATED on every rank by three host all-reduces in which every entry is written by one rank and is zero
//                elsewhere: exact, and bitwise equal everywhere
//   levels >= 2  extend_levels on that level 1: the same host code on the same bits gives every rank the same hierarchy
//                without a message
//   set-up       parts_flags (one import) -> k_galerkin_parts<SPARSE> (the block rows of the rank's own aggregates of the
//                block-sparse A_1, the other entries zero) -> one all-reduce of the nnz_1 * NC^2 doubles -> levels_form,
//                levels_invert on every rank; the ranks then agree on the outcome (parts_levels_agree)
//   apply        k_restrict_parts (own slots of r_1, zeros elsewhere) -> one all-reduce of r_1 -> launch_level_cycle on the
//                whole of level 1, on every rank -> k_prolong_own (x = P_0 e_1 on the owned nodes), then the part-local sweeps
//                of k_sgs_color started from this x: two imports and five all-reduces per iteration, as with two levels
// When level 1 is the last level the launches are those of C8_PRECOND_TWO_LEVEL_PARTS (parts_coarse_setup, parts_coarse).
// The one kernel instance of this file is k_galerkin_parts<ND, NRES, true>; every sum has a fixed order and no kernel uses
// a floating-point atomic.

// The levels below level 0, once per attached halo, per num_owned and per setting of c8_krylov_set_multilevel.
// COLLECTIVE: parts_aggregates, parts_coarse_build, the three all-reduces of the replication and the agreement on a device
// error of the uploads.  No cap on the last level here (c8_krylov_levels reports above it too).
int parts_levels_build(c8_ctx* c, Parts& P, char const* who) {
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, std::string(who) + ": empty mesh");
  int rc = parts_aggregates(c, P);
  if (rc != C8_OK) return rc;
  int const nc = coarse_columns(c), nd = c->ndims;
  if (c->kry_pc_total * nc > (long long)INT_MAX)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": level 1 of the multilevel preconditioner over parts has more than 2^31 unknowns");
  if ((rc = parts_coarse_build(c, P, who)) != C8_OK) return rc;
  if (c->kry_pl_for == P.nown) return C8_OK;
  c->kry_pl_for = -1;
  free_level_list(c->kry_pl_levels);
  int const total = (int)c->kry_pc_total, base = (int)c->kry_pc_base, nagg = c->kry_pc_nagg;
  // every buffer below: this rank's entries in its own slots, zeros elsewhere; ids travel as doubles (exact below 2^53)
  std::vector<double> len(total, 0.);
  for (int a = 0; a < nagg; ++a) len[base + a] = (double)(c->kry_pc_nbr_ptr[a + 1] - c->kry_pc_nbr_ptr[a]);
  if ((rc = c8_comm_allreduce_sum(P.cm, len.data(), total)) != C8_OK) return rc;
  c8_kry_level L1;
  L1.n = total;
  L1.gp.assign(total + 1, 0);
  long long nnz = 0;
  for (int i = 0; i < total; ++i) {
    nnz += (long long)len[i];
    L1.gp[i + 1] = (int32_t)std::min<long long>(nnz, INT_MAX);
  }
  if (nnz * nc * nc > (long long)INT_MAX)  // (the same sum on every rank)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": the matrix of level 1 of the multilevel preconditioner over parts has " + std::to_string(nnz) +
                                    " blocks: more than one all-reduce moves");
  std::vector<double> cols((size_t)nnz, 0.);
  if (L1.gp[base + nagg] - L1.gp[base] == (int32_t)c->kry_pc_nbr.size())
    for (size_t k = 0; k < c->kry_pc_nbr.size(); ++k) cols[(size_t)L1.gp[base] + k] = (double)c->kry_pc_nbr[k];
  if ((rc = c8_comm_allreduce_sum(P.cm, cols.data(), (int)nnz)) != C8_OK) return rc;
  L1.ga.resize((size_t)nnz);
  for (size_t k = 0; k < (size_t)nnz; ++k) L1.ga[k] = (int32_t)cols[k];
  std::vector<double> cen((size_t)total * nd, 0.);
  for (int a = 0; a < nagg; ++a)
    for (int d = 0; d < nd; ++d) cen[(size_t)(base + a) * nd + d] = c->kry_pc_x[(size_t)a * 3 + d];
  if ((rc = c8_comm_allreduce_sum(P.cm, cen.data(), total * nd)) != C8_OK) return rc;
  L1.x.assign((size_t)total * 3, 0.);
  for (int i = 0; i < total; ++i)
    for (int d = 0; d < nd; ++d) L1.x[(size_t)i * 3 + d] = cen[(size_t)i * nd + d];
  std::vector<c8_kry_level>& lv = c->kry_pl_levels;
  lv.push_back(std::move(L1));
  P.note(extend_levels(c, lv));
  if ((rc = parts_agree(P, who, -1., [&](int, long long) { return C8_OK; })) != C8_OK) return rc;
  c->kry_pl_for = P.nown;
  return C8_OK;
}

// What a call of the kind refuses before anything is assembled or iterated, the same on every rank without a message: a
// block row of a replicated level that does not fit the tile of k_level_galerkin, a last level above the cap of the dense
// solve.  COLLECTIVE (parts_levels_build).
int parts_levels_prepare(c8_ctx* c, Parts& P, char const* who) {
  int const rc = parts_levels_build(c, P, who);
  if (rc != C8_OK) return rc;
  std::vector<c8_kry_level> const& lv = c->kry_pl_levels;
  int const nl = (int)lv.size(), nc = coarse_columns(c);
  for (int k = 0; k + 1 < nl; ++k)
    if ((size_t)lv[k].max_nbr * nc * nc * sizeof(double) > GALERKIN_LDS)
      return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": an aggregate of level " + std::to_string(k + 1) + " has " + std::to_string(lv[k].max_nbr) +
                                      " neighbouring aggregates: the block row of a coarse matrix does not fit the tile of k_level_galerkin");
  long long const n = (long long)lv.back().n * nc;
  if (n > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED,
                std::string(who) + ": the multilevel preconditioner over parts solves its last level densely on every rank: level " + std::to_string(nl) +
                    " has n = " + std::to_string(n) + " unknowns (" + std::to_string(lv.back().n) + " aggregates over " + std::to_string(P.nranks) +
                    " parts), which exceeds the cap of " + std::to_string(COARSE_CAP) + "; " +
                    (nl + 1 >= ml_max_levels(c) ? "max_levels = " + std::to_string(ml_max_levels(c)) + " (c8_krylov_set_multilevel) ends the recursion there"
                                                    : std::string("aggregation no longer reduces the node count")));
  return C8_OK;
}

// The hierarchy for the gathered matrix of P.q: A_1 .. A_upto (upto < 0: all levels, then the checked inverse of the last
// one).  Errors go to P; parts_levels_agree() after it gives every rank the same code.  Needs parts_levels_prepare() passed.
template <int ND, int NRES, int G>
void parts_levels_setup(Parts& P, int upto) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  Solve const& q = P.q;
  c8_ctx* c = q.c;
  std::vector<c8_kry_level> const& lv = c->kry_pl_levels;
  int const nl = (int)lv.size();
  bool const invert = upto < 0;
  c->kry_pl_bad = -1.;
  if (nl == 1) {  // level 1 is the last: the dense coarse level of the two-level kind over parts
    parts_coarse_setup<ND, NRES, G>(P, invert);
    return;
  }
  if (invert) upto = nl;
  int const nagg = c->kry_pc_nagg, base = (int)c->kry_pc_base, n = lv.back().n * NC, lda = (n + 1) & ~1;
  size_t const nnz1 = lv[0].ga.size() * NC * NC;
  hipStream_t const st = c->stream;
  int32_t* info = nullptr;
  std::vector<int32_t> h_info;
  if (!P.failed) P.note(levels_begin<NC>(c, lv, &h_info, &info));
  parts_flags<ND, NRES, G>(P);
  if (!P.failed) P.hip(hipMemsetAsync(lv[0].d_A, 0, nnz1 * sizeof(double), st), "hipMemsetAsync");
  if (!P.failed && nagg > 0) {  // the rank's rows of the level-1 graph are the entries gp[base] .. gp[base + nagg)
    hipLaunchKernelGGL((k_galerkin_parts<ND, NRES, true>), dim3(nagg), dim3(TPB), (size_t)c->kry_pc_max_nbr * NC * NC * sizeof(double), st,
                       parts_agg_tables(c), base, c->d_nodeptr, c->d_nodeadj, q.A, lv[0].d_A + (size_t)lv[0].gp[base] * NC * NC, 0);
    P.hip(hipGetLastError(), "k_galerkin_parts");
  }
  P.note(c8_comm_allreduce_device_long(P.cm, st, lv[0].d_A, nnz1, P.failed));
  if (!P.failed && upto >= nl) P.hip(hipMemsetAsync(c->d_kry_Ac, 0, (size_t)n * lda * sizeof(double), st), "hipMemsetAsync");
  if (!P.failed) P.note(levels_form<ND, NRES>(c, lv, upto, info));
  if (!invert || P.failed) return;
  P.note(levels_invert<NC>(c, lv, info, &h_info));
  if (P.failed) return;
  double const two32 = 4294967296.;
  for (int k = nl - 2; k >= 0; --k)  // (the finding of the finest such level wins, as in multilevel_setup)
    if (h_info[3 + k] != INT_MAX) c->kry_pl_bad = (k + 1) * two32 + h_info[3 + k];
  if (c->kry_pl_bad < 0. && levels_bad_row(h_info) >= 0) c->kry_pl_bad = nl * two32 + levels_bad_row(h_info);
}

// the outcome of parts_levels_setup, agreed over the ranks.  COLLECTIVE.
int parts_levels_agree(Parts& P, char const* who) {
  c8_ctx* c = P.q.c;
  int const nl = (int)c->kry_pl_levels.size(), nc = coarse_columns(c);
  if (nl == 1) return parts_coarse_agree(P, who);
  return parts_agree(P, who, c->kry_pl_bad, [&](int r, long long f) {
    int const level = (int)(f >> 32);
    long long const at = f & 0xffffffffLL;
    if (level < nl)
      return fail(C8_ERR_ARG, std::string(who) + ": the diagonal block of aggregate " + std::to_string(at) + " (global id) on level " + std::to_string(level) +
                              " of the multilevel preconditioner over parts is singular or not finite, as found by rank " + std::to_string(r));
    return fail(C8_ERR_ARG, std::string(who) + ": the matrix of level " + std::to_string(nl) +
                            " (the last) of the multilevel preconditioner over parts is singular or not finite at aggregate " + std::to_string(at / nc) +
                            " (row " + std::to_string(at) + " of " + std::to_string((long long)c->kry_pl_levels.back().n * nc) + "), as found by rank " +
                            std::to_string(r));
  });
}

// x = P_0 M_1^-1 P_0^T rhs on the owned nodes: one all-reduce of the n_1 doubles of r_1 between the restriction and the
// cycle over the replicated levels, which every rank runs on the whole of level 1
template <int ND, int NRES>
void parts_levels_apply(Parts& P, double const* rhs, double* x) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  Solve const& q = P.q;
  c8_ctx const* c = q.c;
  std::vector<c8_kry_level> const& lv = c->kry_pl_levels;
  if (lv.size() == 1) {
    parts_coarse<ND, NRES>(P, rhs, x);
    return;
  }
  int const nagg = c->kry_pc_nagg, base = (int)c->kry_pc_base, total = (int)c->kry_pc_total, wpb = TPB / 64;
  AggTables const T = parts_agg_tables(c);
  double *r1 = lv[0].d_vec, *e1 = lv[0].d_vec + (size_t)total * NC;
  C8_PARTS_LAUNCH(P, (k_restrict_parts<ND, NRES>), (total + wpb - 1) / wpb, TPB, total, base, nagg, T, q.nn, rhs, r1, q.S);
  P.note(c8_comm_allreduce_device_long(P.cm, c->stream, r1, (size_t)total * NC, P.failed));
  if (!P.failed) P.hip(launch_level_cycle<ND, NRES>(c, lv, q.S), "launch_level_cycle");
  C8_PARTS_LAUNCH(P, (k_prolong_own<ND, NRES>), xcd_grid(P.nb_own), TPB, P.nown, q.nn, P.nb_own, T, e1, x, q.S);
}

// parts_iteration_two_level with the cycle over the replicated levels in the place of the dense coarse solve
template <int ND, int NRES, int G>
void parts_iteration_multilevel(Parts& P) {
  Solve const& q = P.q;
  size_t const n0 = (size_t)q.nn * ND, nu = (size_t)P.nown * ND, np_ = NRES == 2 ? (size_t)P.nown : (size_t)0;
  C8_PARTS_LAUNCH(P, (k_vec<0>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.p, q.phat, q.S);
  parts_levels_apply<ND, NRES>(P, q.p, q.phat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, P.nown, q.p, q.phat, false), "k_sgs_color");
  parts_spmv<ND, NRES, G, 0>(P, q.phat, P.phat1, q.v, q.rhat);
  parts_scalars<0>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, (k_vec<1>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.s, q.shat, q.S);
  parts_levels_apply<ND, NRES>(P, q.s, q.shat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, P.nown, q.s, q.shat, false), "k_sgs_color");
  parts_spmv<ND, NRES, G, 1>(P, q.shat, P.shat1, q.t, q.s);
  parts_scalars<1>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, k_update_own, P.nb_upd, TPB, nu, np_, n0, q.x, q.r, q.s, q.t, q.phat, q.shat, q.rhat, q.part, q.S);
  parts_scalars<2>(P, P.nb_upd);
}

// c8_krylov_level_matrix with the kind selected and a halo attached: the dense copy of the replicated A_level, level >= 1,
// on every rank.  COLLECTIVE.
int parts_level_matrix(c8_ctx* c, const c8_system* sys, int32_t level, int32_t* n_level, double* out_host) {
  char const* who = "c8_krylov_level_matrix";
  Parts P = parts_of(c);
  int rc = parts_levels_prepare(c, P, who);
  if (rc != C8_OK) return rc;
  std::vector<c8_kry_level> const& lv = c->kry_pl_levels;
  int const nl = (int)lv.size(), nc = coarse_columns(c);
  if (level < 1 || level > nl)
    return fail(C8_ERR_ARG, "c8_krylov_level_matrix: level " + std::to_string(level) + " is not one of the levels 1 .. " + std::to_string(nl));
  c8_kry_level const& L = lv[level - 1];
  long long const nlong = (long long)L.n * nc;
  if (nlong > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov_level_matrix: level " + std::to_string(level) + " has " + std::to_string(nlong) +
                                    " unknowns: a dense copy is refused above the cap of " + std::to_string(COARSE_CAP));
  int const n = (int)nlong, lda = (n + 1) & ~1;
  *n_level = n;
  if (!out_host) return C8_OK;
  bool const two = c->nres == 2;
  P.q.A = Blocks{sys->A[0][0], sys->A[0][1], sys->A[1][0], sys->A[1][1]};
  if (c->ndims == 3 && two) parts_levels_setup<3, 2, 16>(P, level);
  else if (c->ndims == 2 && two) parts_levels_setup<2, 2, 8>(P, level);
  else if (c->ndims == 2 && !two) parts_levels_setup<2, 1, 8>(P, level);
  else return fail(C8_ERR_UNSUPPORTED, "c8_krylov_level_matrix: no kernels for this number of dimensions and residuals");
  std::vector<double> blocks;
  if (level == nl) {
    if (!P.failed)
      P.hip(hipMemcpy2DAsync(out_host, (size_t)n * sizeof(double), c->d_kry_Ac, (size_t)lda * sizeof(double), (size_t)n * sizeof(double), n,
                             hipMemcpyDeviceToHost, c->stream), "hipMemcpy2DAsync");
  } else {
    blocks.resize(L.ga.size() * nc * nc);  // the block-sparse level, spread over the dense copy on the host
    if (!P.failed) P.hip(hipMemcpyAsync(blocks.data(), L.d_A, blocks.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
  }
  if (!P.failed) P.hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  if (!P.failed && level < nl) {
    std::fill(out_host, out_host + (size_t)n * n, 0.);
    for (int i = 0; i < L.n; ++i)
      for (int32_t e = L.gp[i]; e < L.gp[i + 1]; ++e)
        for (int r = 0; r < nc; ++r)
          for (int k = 0; k < nc; ++k) out_host[(size_t)(i * nc + r) * n + (size_t)L.ga[e] * nc + k] = blocks[((size_t)e * nc + r) * nc + k];
  }
  return parts_agree(P, who, -1., [&](int, long long) { return C8_OK; });
}
