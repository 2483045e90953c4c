// c8_assemble_nn.hpp -- the gradient of the objective with respect to the weights theta of the embedded network of
// hybrid_hyper_J2_plane_stress (the reference's DFAD parameters, evaluations.cpp:873-879).
//
// theta enters the local residual only through R_alpha on the unforced plastic path:
//   R_alpha = (|s| - sqrt(2/3) (Y + s_out (NN(s_in alpha) - NN(0)))) / val(mu),
// so at the stored state every point adds
//   phi_alpha (-sqrt(2/3) s_out / val(mu)) (dNN(s_in alpha)/dtheta - dNN(0)/dtheta)
// to grad_theta; the global residual does not see theta.  That is a backward pass of the network per point.
//
// A block takes NN_GRAD_POINTS consecutive points in chunks of NN_GRAD_CHUNK.  Per chunk, the activations of every
// hidden layer and the deltas of two layers live in LDS; threads map to (point, unit) items in the forward and the
// delta passes, and every theta entry has one owner thread, which adds its chunk sum (points in ascending order) to the
// block's partial row part[block][theta].  The NN(0) term is one more pass per block, at input 0 with weight minus the
// block's sum of point factors.  nn_grad_reduce adds the partial rows in block order.  No floating-point atomics and a
// grid that depends on the number of points only: the same inputs give the same bits.
//
// The code is generic over a block executor: each(f) runs f for every thread of the block (the calling thread on the
// device, all of them in turn in the CPU emulator, tests/emul_hybrid) and sync() separates the phases.  Within a phase
// no thread reads what another one writes.
#pragma once

#include <stdint.h>

#include "c8_models.hpp"

namespace c8 {

constexpr int NN_GRAD_THREADS = 256, NN_GRAD_CHUNK = 16, NN_GRAD_POINTS = 1024;
// LDS doubles: inputs, point factors, the running factor sum, the activations of the hidden layers, two delta layers
constexpr int NN_LDS_X = 0, NN_LDS_C = NN_GRAD_CHUNK, NN_LDS_CSUM = 2 * NN_GRAD_CHUNK, NN_LDS_A = 2 * NN_GRAD_CHUNK + 1;
constexpr int NN_LDS_D = NN_LDS_A + NN_MAX_HIDDEN * NN_MAX_WIDTH * NN_GRAD_CHUNK;
constexpr int NN_LDS_SIZE = NN_LDS_D + 2 * NN_MAX_WIDTH * NN_GRAD_CHUNK;

struct NnGradArgs {
  double const* nn;         // network buffer (c8_models.hpp: nn_value_slope)
  double const* xi;         // stored local state [npts][nloc]
  double const* phi;        // local adjoint [npts][nloc]
  int32_t const* elem_set;  // [nelems] or null
  double const* params;     // [nsets][nparams]
  int npts, pts_per_elem, nloc, nparams;
  double abs_tol;
  int ntheta;
  double* part;             // [nblocks][ntheta]
};

inline int nn_grad_blocks(int npts) { return (npts + NN_GRAD_POINTS - 1) / NN_GRAD_POINTS; }

// forward pass of the chunk's points: activations of the hidden layers into LDS; returns nothing, the output layer is
// formed by the caller
template <class EX> C8_HD void nn_chunk_forward(EX& ex, double* lds, double const* nn) {
  int const act = (int)nn[0], nl = (int)nn[1];
  double const* th = nn + NN_HEADER;
  int aoff = NN_LDS_A;
  for (int l = 1; l < nl - 1; ++l) {
    int const n = (int)nn[2 + l], np = (int)nn[1 + l];
    double const* b = th + n * np;
    ex.each([&](int t) {
      for (int i = t; i < NN_GRAD_CHUNK * n; i += NN_GRAD_THREADS) {
        int const p = i / n, j = i - p * n;
        double z;
        if (l == 1) {
          z = th[j] * lds[NN_LDS_X + p] + b[j];
        } else {
          double const* a = lds + aoff - np * NN_GRAD_CHUNK + p * np;
          z = b[j];
          for (int k = 0; k < np; ++k) z += th[j * np + k] * a[k];
        }
        lds[aoff + p * n + j] = nn_act(act, z);
      }
    });
    ex.sync();
    th = b + n;
    aoff += n * NN_GRAD_CHUNK;
  }
}

// backward pass: the chunk's points with weights C[p] (LDS) added to the block's partial row, owner by owner
template <class EX> C8_HD void nn_chunk_backward(EX& ex, double* lds, double const* nn, double* part_row) {
  int const act = (int)nn[0], nl = (int)nn[1];
  int const L = nl - 1;  // weight layers
  // theta offsets and activation offsets of every layer
  int toff[NN_MAX_HIDDEN + 2], aoff[NN_MAX_HIDDEN + 2];
  int o = 0, a = NN_LDS_A;
  for (int l = 0; l < L; ++l) {
    int const n0 = (int)nn[2 + l], n1 = (int)nn[3 + l];
    toff[l] = o;
    o += n1 * (n0 + 1);
    aoff[l + 1] = a;  // activations of hidden layer l + 1 (l + 1 < L)
    a += n1 * NN_GRAD_CHUNK;
  }
  double const* th = nn + NN_HEADER;
  int dcur = NN_LDS_D, dnext = NN_LDS_D + NN_MAX_WIDTH * NN_GRAD_CHUNK;
  for (int l = L - 1; l >= 0; --l) {
    int const n0 = (int)nn[2 + l], n1 = (int)nn[3 + l];
    double const* W = th + toff[l];
    // deltas of this layer's outputs: C[p] for the output layer, else the buffer dcur [p][n1]
    auto delta = [&](int p, int j) { return l == L - 1 ? lds[NN_LDS_C + p] : lds[dcur + p * n1 + j]; };
    auto input = [&](int p, int k) { return l == 0 ? lds[NN_LDS_X + p] : lds[aoff[l] + p * n0 + k]; };
    ex.each([&](int t) {
      for (int q = t; q < n1 * (n0 + 1); q += NN_GRAD_THREADS) {
        double s = 0.;
        if (q < n1 * n0) {
          int const j = q / n0, k = q - j * n0;
          for (int p = 0; p < NN_GRAD_CHUNK; ++p) s += delta(p, j) * input(p, k);
        } else {
          int const j = q - n1 * n0;
          for (int p = 0; p < NN_GRAD_CHUNK; ++p) s += delta(p, j);
        }
        part_row[toff[l] + q] += s;
      }
    });
    if (l == 0) break;
    // deltas of hidden layer l (width n0) into dnext.  The slope is formed from the pre-activation z, recomputed here as the
    // forward pass formed it from the layer below (LDS keeps the activations only)
    int const nb = (int)nn[1 + l];  // width of the layer below hidden layer l
    double const* Wb = th + toff[l - 1];
    ex.each([&](int t) {
      for (int i = t; i < NN_GRAD_CHUNK * n0; i += NN_GRAD_THREADS) {
        int const p = i / n0, k = i - p * n0;
        double s = 0.;
        for (int j = 0; j < n1; ++j) s += W[j * n0 + k] * delta(p, j);
        double z;
        if (l == 1) {
          z = Wb[k] * lds[NN_LDS_X + p] + Wb[n0 + k];
        } else {
          double const* a = lds + aoff[l - 1] + p * nb;
          z = Wb[n0 * nb + k];
          for (int q = 0; q < nb; ++q) z += Wb[k * nb + q] * a[q];
        }
        lds[dnext + p * n0 + k] = nn_act_slope(act, z) * s;
      }
    });
    ex.sync();
    int const tmp = dcur; dcur = dnext; dnext = tmp;
  }
  ex.sync();
}

// output of the network at the chunk's points from the last hidden layer
C8_HD double nn_chunk_output(double const* lds, double const* nn, int p) {
  int const nl = (int)nn[1];
  int const nh = (int)nn[nl];  // topology[nl - 2]: width of the last hidden layer
  double const* th = nn + NN_HEADER;
  int aoff = NN_LDS_A;
  for (int l = 0; l < nl - 2; ++l) {
    int const n0 = (int)nn[2 + l], n1 = (int)nn[3 + l];
    th += n1 * (n0 + 1);
    if (l > 0) aoff += n0 * NN_GRAD_CHUNK;
  }
  double const* a = lds + aoff + p * nh;
  double y = th[nh];
  for (int j = 0; j < nh; ++j) y += th[j] * a[j];
  return y;
}

// one block: points [blk * NN_GRAD_POINTS, +NN_GRAD_POINTS) into part[blk][:]
template <class Model, class EX> C8_HD void nn_grad_block(EX& ex, double* lds, NnGradArgs const& ga, int blk) {
  double const* nn = ga.nn;
  double* const row = ga.part + (size_t)blk * ga.ntheta;
  ex.each([&](int t) {
    for (int q = t; q < ga.ntheta; q += NN_GRAD_THREADS) row[q] = 0.;
    if (t == 0) lds[NN_LDS_CSUM] = 0.;
  });
  ex.sync();
  int const first = blk * NN_GRAD_POINTS;
  int const last = (first + NN_GRAD_POINTS < ga.npts) ? first + NN_GRAD_POINTS : ga.npts;
  double const s_in = nn[NN_HEADER - 6], s_out = nn[NN_HEADER - 5], nn0 = nn[NN_HEADER - 4];
  for (int base = first; base < last; base += NN_GRAD_CHUNK) {
    ex.each([&](int t) {
      if (t < NN_GRAD_CHUNK) {
        int const q = base + t;
        lds[NN_LDS_X + t] = q < last ? s_in * ga.xi[(size_t)q * ga.nloc + 5] : 0.;
      }
    });
    ex.sync();
    nn_chunk_forward(ex, lds, nn);
    ex.each([&](int t) {  // point factors
      if (t < NN_GRAD_CHUNK) {
        int const q = base + t;
        double c = 0.;
        if (q < last) {
          int const es = ga.elem_set ? ga.elem_set[q / ga.pts_per_elem] : 0;
          double const* x = ga.xi + (size_t)q * ga.nloc;
          double const H = s_out * (nn_chunk_output(lds, nn, t) - nn0);
          c = Model::theta_factor(ga.params + (size_t)es * ga.nparams, H, x, ga.abs_tol, s_out) * ga.phi[(size_t)q * ga.nloc + 5];
        }
        lds[NN_LDS_C + t] = c;
      }
    });
    ex.sync();
    ex.each([&](int t) {
      if (t == 0) {
        double s = lds[NN_LDS_CSUM];
        for (int p = 0; p < NN_GRAD_CHUNK; ++p) s += lds[NN_LDS_C + p];
        lds[NN_LDS_CSUM] = s;
      }
    });
    nn_chunk_backward(ex, lds, nn, row);
  }
  // the NN(0) term: input 0 with weight minus the block's factor sum
  ex.each([&](int t) {
    if (t < NN_GRAD_CHUNK) {
      lds[NN_LDS_X + t] = 0.;
      lds[NN_LDS_C + t] = t == 0 ? -lds[NN_LDS_CSUM] : 0.;
    }
  });
  ex.sync();
  nn_chunk_forward(ex, lds, nn);
  nn_chunk_backward(ex, lds, nn, row);
}

// out[q] += sum over the blocks, in block order
C8_HD void nn_grad_reduce_entry(double const* part, int nblocks, int ntheta, int q, double* out) {
  double s = 0.;
  for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * ntheta + q];
  out[q] += s;
}

}  // namespace c8
