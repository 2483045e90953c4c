// c8_assemble_node.hpp -- K1 for hex8 models with a closed form: ONE WAVEFRONT PER NODE, no element stage.
//
// eval_forward_jacobian (evaluations.cpp:12-154) assembles element by element and scatters each element matrix into
// the rows of its eight nodes (global_residual.cpp:556-586).  The staged kernels of c8_assemble_wave.hpp keep that
// shape -- element matrices go to an element-major stage (8.4 KB per hex8 element), a second kernel sums the rows of
// each node -- and move six times the bytes the assembly needs.  Here the loop is turned inside out: a wavefront OWNS
// the four CSR rows (u_0, u_1, u_2, p) of one node, forms them from the node's (up to eight) elements and writes each
// row once.  No stage, no atomics on global memory, every sum in a fixed order: bitwise reproducible.
//
// What makes it affordable is the model's closed form (Model::closed_form, Model::closed_form_row / _block_sums): the
// tangent data of a point are a handful of doubles, so the eight nodes of an element each recompute them (on all 64
// lanes at once, one lane per (element, point)) instead of sharing them through memory, and the contraction with
// the shape functions -- the bulk of the arithmetic -- is split over the nodes without redundancy: every 4 x 4
// block of the element matrix is formed exactly once, by the wavefront of its row node.
//
//   top      lane = pattern         forward assembly: the eight shape values of the reference element at its points into LDS
//            (nshape, hex_pattern): the row node reads its N_a there instead of forming it
//   phase A  lane = (element s of the node, point)      interpolate the point quantities from the element's nodal
//            values -- their gradients in the reference element first, then the point's cached inverse Jacobian (nine
//            coalesced loads) --, closed form (radial return, consistent tangent), the row node's record of the point into
//            LDS, the point's share of the node's residual; the lane of the element's local node 0 stores the converged
//            local state.  The loads of a phase are issued one dependent round trip ahead of it where they depend on the
//            element alone (NodeLane): the point's inverse Jacobian, previous state and weights beside the connectivity.
//            Lane l of an element owns point hex_code(l), not point l (phase B, below); the eight lanes still read 64
//            contiguous bytes per load, and per point nothing changes
//   phase B  lane = (element s of the node, column node m)   the 4 x 4 block d R_(node,.) / d x_(m,.) summed over the
//            element's eight points.  The sum comes first and the combination of its terms after it: a point adds to the 25
//            sums of Model::closed_form_block_sums, closed_form_block_finish forms the 16 entries from them once, after the
//            eighth point (the three "a" terms of the (u, u) entries are entries of ONE 3 x 3 matrix summed over the points;
//            c8_models.hpp).  No load and no table: dN_m/dx at a point is G(pt)^T dN_m/dxi(pt); the
//            lane that holds G(pt) since phase A forms it for the lane that needs it at that step, and a register exchange
//            inside the group of eight lanes (lane_xor8: DPP moves on the GPU) delivers the three doubles.  With the points
//            owned as above, step c pairs lane l with lane l ^ c and the reference gradient is a constant of the step
//   phase C  blocks added into the node's row accumulator in LDS, every entry summed in ascending element order.  The
//            accumulator is an IMAGE of the node's four CSR row blocks, entry for entry in their order (NodeShared::img*)
//   phase D  the finished rows added to (or assigned to) the four CSR blocks -- four straight copies, lane j + 64 it
//            takes entry j + 64 it of a block -- the residual entries to b
//
// Requires an element with 8 nodes, 8 coupled points and identical point sets for both ip sets (hex8), the cached
// shape tables (c8_set_shape_cache: of an element's entry these kernels read the inverse Jacobians, the weights and the size,
// not the dN/dx section), xi != xi_prev (an element's previous state is read by eight wavefronts), and an executor whose
// groups of eight lanes are active or inactive as a whole wherever lane_xor8 is called (NodeLane::valid is per element).
#pragma once

#include "c8_assemble_wave.hpp"

// Diagnostic build only (-DC8_STAMPS, tools/stamp_node.py): s_memtime stamps at the phase boundaries of sampled nodes.
#ifdef C8_STAMPS
#define C8_NSTAMP(i) ex.stamp_node(ga.stamps, node, i)
#else
#define C8_NSTAMP(i)
#endif

namespace c8 {

template <class M, class = void> struct has_closed_form_rows : std::false_type {};
template <class M> struct has_closed_form_rows<M, std::enable_if_t<M::HAS_CLOSED_FORM_ROWS>> : std::true_type {};

// MANY = false (every node of the mesh has at most eight elements): the row accumulator takes the place of the point
// records once phase B has read them; MANY = true: a node's elements go through phases A-C eight at a time and the
// accumulator has its own storage.
// The accumulator of a node of degree deg is the image of its four CSR row blocks, 16 deg doubles, entry (row i, position
// pos of the column node in the node's graph row, column col) where the CSR block has it:
//   img00 [i * 3 deg + 3 pos + col]  (u_i, u_col)   9 deg     img01 [i * deg + pos]  (u_i, p)   3 deg
//   img10 [3 pos + col]              (p, u_col)     3 deg     img11 [pos]            (p, p)       deg
// Within one ds_add_f64 of phase C the lanes' addresses are 3 or 1 doubles apart per position: 16 consecutive positions
// meet in 16 different bank pairs.
template <class E, class ModelD, int MAXDEG, bool MANY> struct NodeShared {
  static constexpr int NR = ModelD::NROW;
  // record + the point's four residual shares.  Even (16-byte LDS reads) and such that the records of two elements lie
  // 32 banks apart modulo the 64 banks (8 points * LDR * 8 bytes = 128 modulo 256): the two element groups of a
  // 16-lane LDS access then never meet in a bank
  static constexpr int LDR = NR + 4;
  static_assert(LDR % 2 == 0 && (E::NP0 * LDR * 8) % 256 == 128, "record stride: 16-byte aligned, element groups 32 banks apart");
  static constexpr int NREC = 8 * E::NP0 * LDR, NACC = MAXDEG * 16;
  alignas(16) double buf[MANY ? NREC + NACC : (NREC > NACC ? NREC : NACC)];
  alignas(16) double nodal[8][E::NN][4];    // (u_0, u_1, u_2, p) of the nodes of the eight elements, loaded one node per lane
  double nshape[8];                         // N of the reference element by agreement pattern of node and point (hex_pattern)
                                            // (forward assembly; the struct has no ADJ parameter, the adjoint leaves it unused)
  double el[8][2];                          // per element: the model's per-element scalars (closed_form_block_scalars)
  double bsum[4];
  C8_HD double* rec(int s, int pt) { return buf + (s * E::NP0 + pt) * LDR; }
  C8_HD double* img() { return buf + (MANY ? NREC : 0); }  // img00 starts here, the others at:
  C8_HD static int img01(int deg) { return 9 * deg; }
  C8_HD static int img10(int deg) { return 12 * deg; }
  C8_HD static int img11(int deg) { return 15 * deg; }
};

// the double at BYTE offset off (a multiple of 8) from p
C8_HD double const* at_byte(double const* p, int off) { return reinterpret_cast<double const*>(reinterpret_cast<char const*>(p) + off); }

// Loads issued one phase ahead of their use and carried in the lane record: lane (s, m) of phase A1 is lane (s, point
// hex_code(m)) of phase A2 and lane (s, column node m) of phase B, so a lane issues its own later loads as soon as it knows
// its element.  G stays in the record through phase B, each row times the point's sign along that axis: the lanes of the
// element form their column nodes' dN/dx from it (lane_xor8)
constexpr int NODE_NXI = 7;  // entries of the local state a lane carries (small_J2)
template <int MAXDEG> struct NodeLane {
  static constexpr int N00 = (9 * MAXDEG + 63) / 64, N01 = (3 * MAXDEG + 63) / 64;
  double J[16];
  double a00[N00], a01[N01], a10[N01], a11;  // current values of this lane's CSR entries
  double bold;                               // ... and of its residual entry (lanes 0..3)
  double rs;
  double G[9], xo[NODE_NXI], w, h;           // A1 -> A2: the point's inverse Jacobian, previous state (forward), weight; the element's size
                                             // A2 -> B: G, row k times the point's sign along k
  int e, a, pos;
  bool valid;
};

// get(l ^ C), C = 1 .. 7: the value of get at the partner lane inside the caller's group of eight lanes (phase B: the lanes of
// one element).  get(l) may read only what lane l's record (ex.lane(l)) held before the phase began.  An executor with a
// register exchange provides xor8<C>(lane, get) (the GPU's: DPP moves, every lane evaluates get for itself and the values
// change places); one without it addresses every lane's record, and get is evaluated for the partner -- with the marker `cur`
// of an executor that watches which lane's record is touched (the CPU emulation) moved to the partner for the call.
// A group of eight lanes is valid or invalid as a whole (NodeLane::valid), so no exchange reaches into an inactive group.
template <class EX, class = void> struct has_xor8 : std::false_type {};
template <class EX> struct has_xor8<EX, std::void_t<typename EX::has_xor8>> : std::true_type {};
template <class EX, class = void> struct has_lane_marker : std::false_type {};
template <class EX> struct has_lane_marker<EX, std::void_t<decltype(std::declval<EX&>().cur)>> : std::true_type {};
template <int C, class EX, class F> C8_HD double lane_xor8(EX& ex, int lane, F get) {
  static_assert(C >= 0 && C < 8, "partner inside the group of eight lanes");
  if constexpr (C == 0) return get(lane);
  else if constexpr (has_xor8<EX>::value) return ex.template xor8<C>(lane, get);
  else if constexpr (has_lane_marker<EX>::value) {
    int const saved = ex.cur;
    ex.cur = lane ^ C;
    double const v = get(lane ^ C);
    ex.cur = saved;
    return v;
  } else return get(lane ^ C);
}

// The reference hex8 at its Gauss points BY AGREEMENT PATTERN.  Node signs and point coordinates are +-1 and +-1/sqrt(3) per
// axis, so N_m and dN_m/dxi at a point depend only on the set j of axes on which the node's sign equals the point's (bit k of
// j):   N = v[0],   dN/dxi_k = s_k v[1 + k]   with s_k the node's sign along k,
// operation for operation E::N and E::dNdxi (a change of sign is exact).  hex_code(n) holds node n's sign bits, the point's
// are pt itself: j = hex_code(n) ^ pt ^ 7.  hex_code is linear over ^ and its own inverse, so the node with pattern j at
// point pt is hex_code(j) ^ hex_code(pt ^ 7).  With j a compile-time constant the four values are constants.
C8_HD constexpr int hex_code(int n) { return n ^ ((n >> 1) & 1); }
template <class E> C8_HD void hex_pattern(int j, double* v) {
  double c[3], w;
  E::point(0, 7, c, w);  // (+, +, +)
  double const a = 1. + ((j & 1) ? c[0] : -c[0]), b = 1. + ((j & 2) ? c[1] : -c[1]), d = 1. + ((j & 4) ? c[2] : -c[2]);
  v[0] = 0.125 * a * b * d;
  v[1] = 0.125 * b * d;
  v[2] = 0.125 * a * d;
  v[3] = 0.125 * a * b;
}

// shape values of the reference hex8 at its Gauss points: E::N(n, xi) operation for operation, 0.125 (1 + sx xi_0)
// (1 + sy xi_1) (1 + sz xi_2), with the point fixed per lane and the node a lane value; signs are selected as values (no
// indexed tables: they would live in scratch).
// Adjoint assembly only, for N_a of the row node (the forward assembly reads NodeShared::nshape; with that table K3 measured
// 2.5-3.4 % SLOWER).  The signs are +-1, so 1 + s * xi is exact in the product, and the factors are multiplied in
// the order of hex_pattern: the same bits.
template <class E> struct HexShape {
  double c[3];  // the point's coordinates
  C8_HD static HexShape of_point(int pt) {
    double w;
    HexShape h;
    E::point(0, pt, h.c, w);
    return h;
  }
  C8_HD double at_node(int n) const {
    double const sx = ((n ^ (n >> 1)) & 1) ? 1. : -1., sy = ((n >> 1) & 1) ? 1. : -1., sz = ((n >> 2) & 1) ? 1. : -1.;  // E::sign
    return 0.125 * (1. + sx * c[0]) * (1. + sy * c[1]) * (1. + sz * c[2]);
  }
};

// ADJ = false: eval_forward_jacobian (evaluations.cpp:12-154): A += dR/dx, b += R, xi = the converged local state.
// ADJ = true:  eval_adjoint_jacobian (evaluations.cpp:349-526) for the objective "average displacement": A += (dR/dx)^T at
//              the stored state, b += -dJ/dx + f + (dxi/dx)^T g; g is left as it is (dJ/dxi = 0 for this objective) and
//              no state is written.  The transposed blocks come from the same code with another record
//              (Model::closed_form_row<true>), (dxi/dx)^T g from Model::closed_form_adjoint.
template <class E, template <class> class ModelT, int MAXDEG, bool MANY, bool ADJ = false, class EX>
C8_HD void node_rows_closed(EX& ex, NodeShared<E, ModelT<Dual>, MAXDEG, MANY>& sh, MeshTables const& mt, ModelSettings const& ms,
                            FieldArgs const& fa, GatherArgs const& ga, int node, AdjointArgs const& aa = AdjointArgs{}) {
  using Model = ModelT<Dual>;
  using SH = NodeShared<E, Model, MAXDEG, MANY>;
  using NL_ = NodeLane<MAXDEG>;
  constexpr int NL = Model::NLOC, NR = SH::NR;
  static_assert(NL <= NODE_NXI, "NodeLane::xo holds a point's local state");
  static_assert(E::NN == 8 && E::NP0 == 8 && E::SAME_POINTS, "row-per-node kernel: hex8-like element");
  static_assert(!Mechanics::USES_U && !Model::FINITE_DEF, "row-per-node kernel: small-strain weak form without u terms");
  C8_NSTAMP(6);
  int const nptr = ga.nodeptr[node], deg = ga.nodeptr[node + 1] - nptr;
  int const e0 = ga.nodeelem_ptr[node], e1 = ga.nodeelem_ptr[node + 1];
  size_t const np = (size_t)nptr;
  int const n3 = 3 * deg;
  if (e0 == e1) return;  // a node without elements (phantom columns of a mesh part): its rows are not touched
  C8_NSTAMP(0);
  auto zero_acc = [&](int lane) {
    C8_UNROLL
    for (int it = 0; it < (SH::NACC + 63) / 64; ++it) {
      int const q = lane + 64 * it;
      if (q < 16 * deg) sh.img()[q] = 0.;
    }
    if (lane < 4) sh.bsum[lane] = 0.;
  };
  // forward assembly: the reference element's shape values, lane = pattern.  Here and not in the kernel's wrapper: the
  // function is the unit the CPU emulation calls
  if (!ADJ || MANY) {
    ex.each([&](int lane) {
      if (!ADJ && lane < 8) {
        double v[4];
        hex_pattern<E>(lane, v);
        sh.nshape[lane] = v[0];
      }
      if (MANY) zero_acc(lane);
    });
    ex.sync();
  }
  for (int c0 = e0; c0 < e1; c0 += 8) {  // eight elements of the node at a time (MANY = false: exactly one round)
    int const ne = (e1 - c0 < 8) ? e1 - c0 : 8;
    // ---- phase A: nodal values, lane = (element s, node m): every lane fetches one node of one element, the eight lanes
    //      of an element then read all eight from LDS (a lane per point fetching its own copies costs eight times the
    //      loads and their registers) ------------------------------------------------------------------------------------
    ex.each([&](int lane) {
      auto& r = ex.lane(lane);
      int const s = lane >> 3, m = lane & 7, mp = hex_code(m);  // mp: the point this lane owns in phase A2
      r.valid = s < ne;
      r.rs = 0.;
      if (!r.valid) return;
      int const packed = ga.nodeelem[c0 + s];
      int const e = packed >> 3, a = packed & 7;
      r.e = e;
      r.a = a;
      int const nd = mt.conn[(size_t)e * E::NN + m];  // first: it gates the loads of u and p
      // phase B's operand of this lane (column node m): position of m in the node's graph row
      r.pos = ga.pos[((size_t)e * E::NN + m) * E::NN + a];
      // what this lane needs in phase A2 as point m of its element, issued one round trip early: the wait for nd leaves
      // these outstanding (the counter of outstanding loads is in order), they return under the fetch of u and p.
      // Adjoint: the previous state and the history entries stay in A2 (issued here they changed K3's rounding)
      {
        double const* const t = mt.shape + (size_t)e * SHAPE_STRIDE;
        C8_UNROLL
        for (int c = 0; c < 9; ++c) r.G[c] = t[SHAPE_JINV + 8 * c + mp];
        if constexpr (!ADJ) {
          size_t const q0 = ((size_t)e * E::NP0 + mp) * NL;
          C8_UNROLL
          for (int j = 0; j < NL; ++j) r.xo[j] = fa.xi_prev[q0 + j];
        }
        r.w = t[SHAPE_WDV + mp];
        r.h = t[SHAPE_H];
      }
      double* const nv = sh.nodal[s][m];
      nv[0] = fa.u[(size_t)nd * 3 + 0]; nv[1] = fa.u[(size_t)nd * 3 + 1]; nv[2] = fa.u[(size_t)nd * 3 + 2];
      nv[3] = fa.p[nd];
    });
    ex.sync();
    // ---- phase A, continued: lane = (element s, point) ---------------------------------------------------------------
    ex.each([&](int lane_) {
      auto& r = ex.lane(lane_);
      int lane = lane_;
      C8_PIN(lane);  // the offsets below are formed here, not at the top of the kernel and kept in registers
      int const s = lane >> 3, pt = hex_code(lane & 7);  // lane l of an element owns point hex_code(l): phase B, below
      if (!r.valid) return;
      int const e = r.e, a = r.a;
      size_t const q0 = ((size_t)e * E::NP0 + pt) * NL;
      // the point's inverse Jacobian G[3 k + d] = d xi_k / d x_d (the eight lanes of an element read 64 contiguous bytes per
      // component) and, forward, its previous state: fetched by this lane in phase A1
      double G[9], xi_old[NL];
      C8_UNROLL
      for (int c = 0; c < 9; ++c) G[c] = r.G[c];
      if constexpr (!ADJ) {
        C8_UNROLL
        for (int j = 0; j < NL; ++j) xi_old[j] = r.xo[j];
      }
      // adjoint assembly: this point's history entries (f at the node's four rows, g), fetched under the interpolation
      double fh4[4] = {0., 0., 0., 0.}, gx[NL];
      C8_UNROLL
      for (int j = 0; j < NL; ++j) gx[j] = 0.;
      if constexpr (ADJ) {
        double const* const fh = aa.f + ((size_t)e * E::NP0 + pt) * E::NDOF;
        fh4[0] = fh[3 * a + 0]; fh4[1] = fh[3 * a + 1]; fh4[2] = fh[3 * a + 2]; fh4[3] = fh[3 * E::NN + a];
        C8_UNROLL
        for (int j = 0; j < NL; ++j) gx[j] = aa.g[((size_t)e * E::NP0 + pt) * NL + j];
      }
      // interpolation (global_residual.cpp:289-332): the gradients of u_0, u_1, u_2, p in the REFERENCE element first (R),
      // then q = R G.  The nodes are taken in the order of their agreement pattern with the point, i = 0 .. 7 -- node
      // hex_code(i) ^ hex_code(pt ^ 7) --, so the reference values of a step are compile-time constants up to the point's
      // own signs, which leave the sum and multiply R afterwards: 13 multiply-adds and one 32-byte LDS read per node, no
      // table.  The row node's own dN_a/dx (g below) is dN_a/dxi G.  (Until this form the phase walked the skewed dN/dx
      // table, 24 bytes per lane and node: DESIGN 3.8.)
      double q[WQ];
      C8_UNROLL
      for (int c = 0; c < WQ; ++c) q[c] = 0.;
      double g[3];
      {
        double R[12], pN = 0.;
        C8_UNROLL
        for (int c = 0; c < 12; ++c) R[c] = 0.;
        int const mo = hex_code(pt ^ 7) * 32;  // byte offset of a node's four values in sh.nodal[s]
        C8_UNROLL
        for (int i = 0; i < E::NN; ++i) {
          double v[4];
          hex_pattern<E>(i, v);
          double const t0 = (i & 1) ? v[1] : -v[1], t1 = (i & 2) ? v[2] : -v[2], t2 = (i & 4) ? v[3] : -v[3];
          double const* const nv = at_byte(sh.nodal[s][0], mo ^ (hex_code(i) * 32));
          double const u0 = nv[0], u1 = nv[1], u2 = nv[2], pm = nv[3];
          R[0] += u0 * t0; R[1] += u0 * t1; R[2] += u0 * t2;
          R[3] += u1 * t0; R[4] += u1 * t1; R[5] += u1 * t2;
          R[6] += u2 * t0; R[7] += u2 * t1; R[8] += u2 * t2;
          pN += pm * v[0];
          R[9] += pm * t0; R[10] += pm * t1; R[11] += pm * t2;
        }
        double const s0 = (pt & 1) ? 1. : -1., s1 = (pt & 2) ? 1. : -1., s2 = (pt & 4) ? 1. : -1.;
        C8_UNROLL
        for (int f = 0; f < 4; ++f) {
          double const r0 = s0 * R[3 * f], r1 = s1 * R[3 * f + 1], r2 = s2 * R[3 * f + 2];
          C8_UNROLL
          for (int d = 0; d < 3; ++d) q[(f < 3 ? 3 * f : 10) + d] = r0 * G[d] + r1 * G[3 + d] + r2 * G[6 + d];
        }
        q[9] = pN;
        double xa[3], wa, da[3];
        E::point(0, pt, xa, wa);
        E::dNdxi(a, xa, da);
        C8_UNROLL
        for (int d = 0; d < 3; ++d) g[d] = da[0] * G[d] + da[1] * G[3 + d] + da[2] * G[6 + d];
      }
      C8_NSTAMP(7);
      if constexpr (ADJ) {
        C8_UNROLL
        for (int j = 0; j < NL; ++j) xi_old[j] = fa.xi_prev[q0 + j];
      }
      int const es = mt.elem_set ? mt.elem_set[e] : 0;
      // phase B's operand of this lane as the holder of G(pt): G with row k times the sign of the point along k, which is
      // the sign of node (lane & 7) along k (exact).  In the record: the lanes of the element read it there (lane_xor8)
      C8_UNROLL
      for (int c = 0; c < 9; ++c) r.G[c] = ((pt >> (c / 3)) & 1) ? G[c] : -G[c];
      typename Model::ClosedForm cf;
      Model::closed_form(mt.params + (size_t)es * Model::NPARAMS, q, xi_old, ms.abs_tol, r.h, ms.stab_mult, cf, true);
      // phase B's scalars of the element (tau kappa, 1 / kappa), formed here, from the parameters the closed form has just
      // read: behind the store below they would be fetched again
      double esc[2];
      Model::closed_form_block_scalars(mt.params + (size_t)es * Model::NPARAMS, cf.t, esc);
      if (!ADJ && a == 0) {  // local->scatter (local_residual.cpp:624-631): once per element, by the wavefront of its first node
        C8_UNROLL
        for (int j = 0; j < NL; ++j) fa.xi[q0 + j] = cf.xi[j];
      }
      C8_NSTAMP(8);
      double const w = r.w;
      double Na;
      if constexpr (ADJ) Na = HexShape<E>::of_point(pt).at_node(a);
      else Na = sh.nshape[hex_code(a) ^ pt ^ 7];
      double* const rc = sh.rec(s, pt);
      double el[2];
      Model::template closed_form_row<ADJ>(cf.t, w, g, Na, rc, el);
      if (pt == 0) { sh.el[s][0] = esc[0]; sh.el[s][1] = esc[1]; }
      if constexpr (!ADJ) {
        // the point's share of R_(node,.): fluxes contracted with the row node's shape entries
        C8_UNROLL
        for (int i = 0; i < 3; ++i) rc[NR + i] = w * (cf.F[3 * i] * g[0] + cf.F[3 * i + 1] * g[1] + cf.F[3 * i + 2] * g[2]);
        rc[NR + 3] = w * (cf.F[9] * Na + cf.F[10] * g[0] + cf.F[11] * g[1] + cf.F[12] * g[2]);
      } else {
        // the point's share of the adjoint right-hand side at the node's rows (:486-487): [-dJ/dq + (dxi/dq)^T g] dq/dx + f
        // with dJ/dq = c_avg w / ndims on the displacement itself (avg_disp.cpp:16-33) and (dxi/dq)^T g = Re on grad u
        double Re[6];
        double dq[10];  // dJ/dq of the objective's load term at fixed xi (grad u 0..8, p 9); zero for "average displacement"
        C8_UNROLL
        for (int k = 0; k < 10; ++k) dq[k] = 0.;
        if (aa.qoi.c_load != 0.) {  // calibration objective (uniform over the launch): g -= dJ/dxi first (:474-481); the
          double dxi[NL];           // updated g is stored by node_rows_update_g once every wavefront has read the old one
          Model::closed_form_load_term(mt.params + (size_t)es * Model::NPARAMS, aa.qoi.c_load * w, aa.qoi.comp,
                                       aa.qoi.S + ((size_t)e * E::NP0 + pt) * 3, dxi, dq);
          C8_UNROLL
          for (int j = 0; j < NL; ++j) gx[j] -= dxi[j];
        }
        Model::closed_form_adjoint(mt.params + (size_t)es * Model::NPARAMS, cf.t, gx, Re);
        double const dJ = aa.qoi.c_avg * w / aa.qoi.ndims * Na;
        rc[NR + 0] = (Re[0] - dq[0]) * g[0] + (Re[1] - dq[1]) * g[1] + (Re[2] - dq[2]) * g[2] - dJ + fh4[0];
        rc[NR + 1] = (Re[1] - dq[3]) * g[0] + (Re[3] - dq[4]) * g[1] + (Re[4] - dq[5]) * g[2] - dJ + fh4[1];
        rc[NR + 2] = (Re[2] - dq[6]) * g[0] + (Re[4] - dq[7]) * g[1] + (Re[5] - dq[8]) * g[2] - dJ + fh4[2];
        rc[NR + 3] = -dq[9] * Na + fh4[3];
      }
    });
    ex.sync();
    C8_NSTAMP(1);
    // ---- phase B: lane = (element s, column node m) ----------------------------------------------------------------
    ex.each([&](int lane_) {
      auto& r = ex.lane(lane_);
      int lane = lane_;
      C8_PIN(lane);
      if (!r.valid) return;  // a lane without an element has no block: phase C passes it over (s >= ne), J is not read
      int const s = lane >> 3, m = lane & 7;
      // The sums over the element's eight points the block is a fixed combination of (Model::closed_form_block_sums), combined
      // once after the last step (closed_form_block_finish): the three "a" terms of the (u, u) entries are entries of ONE 3 x 3
      // matrix X summed over the points, so a step accumulates X and the b term's C, not the nine combined entries
      double S[Model::NSUM];
      double const rho = sh.el[s][0];  // tau kappa (phase A2); 1 / kappa is read after the last step
      // dN_m/dx of this lane's column node from the inverse Jacobians the element's lanes hold since phase A2, no table.  At
      // step c the lane takes the point of lane l ^ c, pt = hex_code(l) ^ hex_code(c): node m = l agrees with that point on
      // the axes hex_code(c) ^ 7 -- the same pattern in every lane, so N_m(pt) and |dN_m/dxi_k| are constants of the step.
      // The HOLDER of G(pt) forms h = G^T dN_m'/dxi for its asker m' = l ^ c: the asker's sign along k is the holder's own
      // (in NodeLane::G since A2) times the step's flip, bit k of hex_code(c); nine operations, then a lane exchange
      auto step = [&](auto cc) {
        constexpr int c = decltype(cc)::value, hc = hex_code(c);
        double v[4];
        hex_pattern<E>(hc ^ 7, v);
        double const k0 = (hc & 1) ? -v[1] : v[1], k1 = (hc & 2) ? -v[2] : v[2], k2 = (hc & 4) ? -v[3] : v[3];
        double h[3];
        C8_UNROLL
        for (int d = 0; d < 3; ++d)
          h[d] = lane_xor8<c>(ex, lane, [&](int l) -> double {
            double const* const Gs = ex.lane(l).G;
            return k0 * Gs[d] + k1 * Gs[3 + d] + k2 * Gs[6 + d];
          });
        // step 0 starts the sums (no zeroing moves).  A zero sum may then be -0 where adding to +0 gave +0; phase C adds the
        // block to an image that starts at +0, and (+0) + (-0) = +0: the stored values are the same
        Model::template closed_form_block_sums<c == 0>(sh.rec(s, hex_code(m) ^ hc), rho, h, v[0], S);
        // one point's record in registers at a time: without the lines below the compiler fetches the records of all
        // eight points first (over a hundred doubles) and spills
        C8_UNROLL
        for (int j = 0; j < Model::NSUM; ++j) C8_PIN(S[j]);
        C8_SCHED_FENCE();
      };
      step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{});
      step(std::integral_constant<int, 2>{}); step(std::integral_constant<int, 3>{});
      step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
      step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{});
      Model::closed_form_block_finish(S, sh.el[s][1], r.J);
      if (m < 4) {
        double v = 0.;
        C8_UNROLL
        for (int pt = 0; pt < E::NP0; ++pt) v += sh.rec(s, pt)[NR + m];
        r.rs = v;
      }
    });
    C8_NSTAMP(2);
    if (c0 == e0) {
      // the CSR entries this lane updates in phase D, fetched while phase C runs (assign mode: nothing to read, the rows start from
      // zero -- uniform over the launch).  Not earlier: the counter of outstanding loads is in order, so the first wait of
      // phase B for a shape entry out of L2 would also wait for these, which come from HBM
      ex.each([&](int lane_) {
        auto& r = ex.lane(lane_);
        int lane = lane_;
        C8_PIN(lane);  // what follows is derived from the lane number here, not at the top of the kernel and kept in registers
        C8_UNROLL
        for (int it = 0; it < NL_::N00; ++it) {
          int const j = lane + 64 * it;
          r.a00[it] = 0.;
          if (!ga.assign && j < 9 * deg) r.a00[it] = ga.A[0][0][np * 9 + j];
        }
        C8_UNROLL
        for (int it = 0; it < NL_::N01; ++it) {
          int const j = lane + 64 * it;
          r.a01[it] = r.a10[it] = 0.;
          if (!ga.assign && j < n3) { r.a01[it] = ga.A[0][1][np * 3 + j]; r.a10[it] = ga.A[1][0][np * 3 + j]; }
        }
        r.a11 = 0.;
        if (!ga.assign && lane < deg) r.a11 = ga.A[1][1][np + lane];
        r.bold = 0.;
        if (!ga.assign && lane < 4) r.bold = lane < 3 ? ga.b[0][(size_t)node * 3 + lane] : ga.b[1][node];
      });
    }
    if (!MANY) {  // the accumulator takes the records' place
      ex.sync();
      ex.each([&](int lane) { zero_acc(lane); });
    }
    ex.sync();
    C8_NSTAMP(3);
    // ---- phase C: the elements' blocks into the row accumulator (ds_add_f64), the sums into one entry taken in ascending
    //      element order --------------------------------------------------------------------------------------------
    // A lane forms its few base addresses once from pos, deg and n3; the sixteen adds keep the order of the block's entries
    auto add_block = [&](int lane) {
      auto& r = ex.lane(lane);
      double* const c00 = sh.img() + 3 * r.pos;                // (u_0, u_.) of this column node; rows u_1, u_2 follow n3 apart
      double* const c01 = sh.img() + SH::img01(deg) + r.pos;   // (u_0, p); rows u_1, u_2 follow deg apart
      double* const c10 = sh.img() + SH::img10(deg) + 3 * r.pos;
      double* const c11 = sh.img() + SH::img11(deg) + r.pos;
      C8_UNROLL
      for (int j = 0; j < 16; ++j) {
        int const i = j >> 2, col = j & 3;
        ex.lds_add(i < 3 ? (col < 3 ? c00 + i * n3 + col : c01 + i * deg) : (col < 3 ? c10 + col : c11), r.J[j]);
      }
      if ((lane & 7) < 4) ex.lds_add(&sh.bsum[lane & 7], r.rs);
    };
#ifndef C8_TUNE_NODE_C_BY_ELEMENT
    // all elements in one pass.  Lanes of one instruction that add to the same entry (a column node shared by several of the
    // node's elements) are served by the LDS unit in ascending lane order, i.e. in ascending element order: the results are
    // bitwise those of the element-by-element form below (measured on jiggled meshes, forward and adjoint, tools/README.md),
    // which took eight times the LDS instructions (K1 4.68 -> 4.46 ms)
    ex.each([&](int lane) {
      if ((lane >> 3) >= ne) return;
      add_block(lane);
    });
#else  // one element after the other: within one element the column nodes are distinct and so are the addresses
    for (int s2 = 0; s2 < ne; ++s2) {
      ex.each([&](int lane) {
        if ((lane >> 3) != s2) return;
        add_block(lane);
      });
    }
#endif
    ex.sync();
    C8_NSTAMP(4);
    // MANY = false is the form for nodes with at most eight elements: one round, said here so that the compiler does not keep
    // the CSR entries fetched above in registers for a second one (they would be live through phases A and B)
    if (!MANY) break;
  }
  // ---- phase D: rows out (the tail of gather_node_rows) -------------------------------------------------------------
  ex.each([&](int lane_) {
    auto& r = ex.lane(lane_);
    int lane = lane_;
    C8_PIN(lane);
    // all fetched values complete HERE, once, outside the conditional stores below: with the waits inside the branches the
    // compiler's count of outstanding memory operations is lost at every join, and it then drains the counter -- the
    // previous store included -- in front of each store (ten serialised write round trips per node)
    C8_UNROLL
    for (int it = 0; it < NL_::N00; ++it) C8_PIN(r.a00[it]);
    C8_UNROLL
    for (int it = 0; it < NL_::N01; ++it) { C8_PIN(r.a01[it]); C8_PIN(r.a10[it]); }
    C8_PIN(r.a11);
    C8_PIN(r.bold);
    // the image is in the blocks' own order: entry j of a block is entry j of its image
    double const* const i00 = sh.img(), * const i01 = i00 + SH::img01(deg), * const i10 = i00 + SH::img10(deg), * const i11 = i00 + SH::img11(deg);
    C8_UNROLL
    for (int it = 0; it < NL_::N00; ++it) {
      int const j = lane + 64 * it;
      if (j < 9 * deg) ga.A[0][0][np * 9 + j] = r.a00[it] + i00[j];
    }
    C8_UNROLL
    for (int it = 0; it < NL_::N01; ++it) {
      int const j = lane + 64 * it;
      if (j < n3) {
        ga.A[0][1][np * 3 + j] = r.a01[it] + i01[j];
        ga.A[1][0][np * 3 + j] = r.a10[it] + i10[j];
      }
    }
    if (lane < deg) ga.A[1][1][np + lane] = r.a11 + i11[lane];
    if (lane < 3) ga.b[0][(size_t)node * 3 + lane] = r.bold + sh.bsum[lane];
    if (lane == 3) ga.b[1][node] = r.bold + sh.bsum[3];
  });
  ex.sync();
  C8_NSTAMP(5);
}

// The adjoint assembly's update of the local history, g -= dJ/dxi (evaluations.cpp:474-481), for the objective's load term:
// one lane per (element, point), run AFTER the row-per-node launches of the call (every wavefront reads the old g of its
// elements' points; eight wavefronts read each).  The shape-table weight and the model's derivative are those of phase A.
template <class E, template <class> class ModelT>
C8_HD void node_rows_update_g(MeshTables const& mt, AdjointArgs const& aa, size_t qp) {
  using Model = ModelT<Dual>;
  int const e = (int)(qp / E::NP0), pt = (int)(qp % E::NP0);
  int const es = mt.elem_set ? mt.elem_set[e] : 0;
  double const w = mt.shape[(size_t)e * SHAPE_STRIDE + SHAPE_WDV + pt];
  double dxi[Model::NLOC], dq[10];
  Model::closed_form_load_term(mt.params + (size_t)es * Model::NPARAMS, aa.qoi.c_load * w, aa.qoi.comp, aa.qoi.S + qp * 3, dxi, dq);
  C8_UNROLL
  for (int j = 0; j < Model::NLOC; ++j) aa.g[qp * Model::NLOC + j] -= dxi[j];
}

}  // namespace c8
