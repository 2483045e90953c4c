// c8_kernels.hip -- gfx950 kernels: one lane group (E::NDOF lanes) per element,
// 64/NDOF elements per wavefront, 4 wavefronts per workgroup.  No workgroup barrier is
// ever used: groups are independent and local Newton iteration counts differ, so all
// cooperation is wave-synchronous through LDS (in-order per wave) with compiler fences.
#include <hip/hip_runtime.h>

#include "c8_assemble_adjoint.hpp"
#include "c8_assemble_wave.hpp"
#include "c8_assemble_node.hpp"
#include "c8_kernels.hpp"

namespace c8 {

#ifdef C8_TUNE_VECTOR_WIB  // tuning build (same results): the wave's index in its block as a vector value
#define C8_WAVE_IN_BLOCK(WPB) (threadIdx.x >> 6)
#else
#define C8_WAVE_IN_BLOCK(WPB) ((WPB) == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6))
#endif
#ifndef C8_BLOCK
#define C8_BLOCK 64
#endif
constexpr int BLOCK = C8_BLOCK;

struct NoLane {};  // kernels whose lanes keep nothing between the phases
template <class Lane> struct GpuExec {
  int k;
  Lane& L;
  __device__ __forceinline__ GpuExec(int k_, Lane& l) : k(k_), L(l) {}
  template <class F> __device__ __forceinline__ void each(F f) { f(k); }
  __device__ __forceinline__ Lane& lane(int) { return L; }
  template <class F> __device__ __forceinline__ bool any(F f) { return f(k); }
  template <class F> __device__ __forceinline__ bool any_wave(F f) { return __any(f(k)) != 0; }
  // callable INSIDE each(): true in every active lane if x is true in any of them -- a scalar branch around work that
  // is a no-op for the lanes where x is false (the emulator simply returns x)
  __device__ __forceinline__ bool uniform_any(bool x) { return __any(x) != 0; }
  // the value of f at the first active lane, in every lane
  template <class F> __device__ __forceinline__ int first_lane(F f) { return __builtin_amdgcn_readfirstlane(f(k)); }
  // Lanes of one wavefront exchange data through LDS.  LDS instructions of a wave execute in order, so
  // only the compiler has to be kept from moving LDS accesses across the exchange point: a
  // wavefront-scope fence does that without draining the memory counters (a workgroup-scope fence
  // also waits for outstanding global loads/stores/atomics).
  __device__ __forceinline__ void sync() {
#ifdef C8_SYNC_WORKGROUP
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
  }
  __device__ __forceinline__ void add(double* p, double v, int atomic) {
    if (atomic) unsafeAtomicAdd(p, v);  // global_atomic_add_f64
    else *p += v;
  }
  __device__ __forceinline__ void flag(int* s) { atomicOr(s, 1); }
  // *p += v for p in LDS, without a return value: ds_add_f64, no vector ALU instruction.  Adds of one wavefront to one
  // address take effect in program order.
  __device__ __forceinline__ void lds_add(double* p, double v) { unsafeAtomicAdd(p, v); }
  // get(l) evaluated in lane S of the caller's group of 8 lanes (lanes 8g .. 8g+7), returned to every lane of the
  // group: two DPP row broadcasts (lane S and lane 8+S of each row of 16) and a select per 32-bit half, no LDS and no
  // barrier.  The source lane must be active whenever a reader is (a group is active or inactive as a whole wherever
  // this is used).  (ds_bpermute_b32 instead of DPP: measured slower on every model.)
  template <int S, class F> __device__ __forceinline__ double bcast8(int lane, F get) {
    double const x = get(lane);
    int const lo = __double2loint(x), hi = __double2hiint(x);
    int const a_lo = __builtin_amdgcn_update_dpp(0, lo, 0x150 + S, 0xf, 0xf, false);  // row_newbcast:S
    int const a_hi = __builtin_amdgcn_update_dpp(0, hi, 0x150 + S, 0xf, 0xf, false);
    int const b_lo = __builtin_amdgcn_update_dpp(0, lo, 0x158 + S, 0xf, 0xf, false);  // row_newbcast:8+S
    int const b_hi = __builtin_amdgcn_update_dpp(0, hi, 0x158 + S, 0xf, 0xf, false);
    bool const upper = (k & 8) != 0;
    return __hiloint2double(upper ? b_hi : a_hi, upper ? b_lo : a_lo);
  }
  // get(l) of lane l ^ C, C = 1 .. 7, inside the caller's group of 8 lanes (lane_xor8, c8_assemble_node.hpp): every lane
  // evaluates get for itself and v_mov_b32 DPP exchanges both halves of the double -- quad_perm for C = 1, 2, 3,
  // row_half_mirror (lane i of a half row takes lane 7 - i = i ^ 7) for C = 7, the mirror followed by the quad_perm of
  // C ^ 7 for C = 4, 5, 6.  No LDS, no barrier.  A disabled source lane would leave the reader its own value: a group of 8
  // lanes must be active or inactive as a whole wherever this is used.
  using has_xor8 = void;
  template <int C, class F> __device__ __forceinline__ double xor8(int lane, F get) {
    static_assert(C >= 1 && C <= 7, "partner inside the group of 8 lanes");
    constexpr int Q = C < 4 ? C : C ^ 7, QP = Q == 1 ? 0xB1 : (Q == 2 ? 0x4E : 0x1B);  // quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]
    double const x = get(lane);
    int lo = __double2loint(x), hi = __double2hiint(x);
    if constexpr (C >= 4) {
      lo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xf, 0xf, false);  // row_half_mirror
      hi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xf, 0xf, false);
    }
    if constexpr (C != 7) {
      lo = __builtin_amdgcn_update_dpp(lo, lo, QP, 0xf, 0xf, false);
      hi = __builtin_amdgcn_update_dpp(hi, hi, QP, 0xf, 0xf, false);
    }
    return __hiloint2double(hi, lo);
  }
  // Range-checked row I/O (row_load / row_store, c8_assemble_node.hpp): entry j of a row of n doubles at base through a buffer
  // descriptor over exactly those 8 n bytes.  The address unit checks the range: a lane with j >= n loads 0 and its store is
  // dropped -- no compare, no exec-mask region, no 64-bit address per lane.  base and n must be wave-uniform and PROVABLY so
  // (kernel arguments, blockIdx, values loaded through them): the descriptor then stays in scalar registers and is built once
  // for the accesses of a phase that share it; from a per-lane value the compiler would wrap every access in a
  // v_readfirstlane loop.  0 <= j, 8 j < 2^31.
  using has_row_io = void;
  using has_const_table = void;  // the library fills MeshTables::cf_const (k_closed_form_constants, c8_api.hip)
  __device__ __forceinline__ static auto row_rsrc(double const* base, int n) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), 0, 8 * n, 0x00020000);  // raw buffer, 32-bit data format
  }
  __device__ __forceinline__ double row_load(double const* base, int n, int j) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    v2u const v = __builtin_amdgcn_raw_buffer_load_b64(row_rsrc(base, n), 8 * j, 0, 0);
    return __hiloint2double((int)v[1], (int)v[0]);
  }
  __device__ __forceinline__ void row_store(double* base, int n, int j, double x) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    v2u v;
    v[0] = (unsigned)__double2loint(x);
    v[1] = (unsigned)__double2hiint(x);
    __builtin_amdgcn_raw_buffer_store_b64(v, row_rsrc(base, n), 8 * j, 0, 0);
  }
  // get(l) of lane l ^ 32 (the other half of the wavefront)
  template <class F> __device__ __forceinline__ double xor32(int lane, F get) { return __shfl_xor(get(lane), 32); }
  // lanes 0..31: getA(lane) + getA(lane + 32); lanes 32..63: getB(lane - 32) + getB(lane).  v_permlane32_swap (gfx950)
  // exchanges the upper half of one register with the lower half of another: two swaps per double, then one add.
  template <class FA, class FB> __device__ __forceinline__ double pair_sum32(int lane, FA getA, FB getB) {
    double const a = getA(lane), b = getB(lane);
#ifdef C8_TUNE_NO_SWAP32  // tuning build (same results): the exchange through ds_bpermute and selects
    double const recv = __shfl_xor(lane < 32 ? b : a, 32);
    return lane < 32 ? a + __shfl_xor(a, 32) + 0. * recv : __shfl_xor(b, 32) + b;
#endif
    auto const lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    auto const hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
  }
#ifdef C8_STAMPS
  // row-per-node kernel: node n is sampled when n % 244 == 0; the stamp does not wait for outstanding memory operations
  __device__ __forceinline__ void stamp_node(unsigned long long* stamps, int n, int i) {
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    if (k == 0 && stamps && (n % 244) == 0 && n / 244 < 4096) stamps[(size_t)(n / 244) * 16 + i] = t;
  }
  // element e is sampled when e % 244 == 0 (4096 samples over a 1M-element mesh)
  __device__ __forceinline__ void stamp(SystemArgs const& sa, int e, int i) {
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    if (k == 0 && sa.stamps && (e % 244) == 0 && e / 244 < 4096) sa.stamps[(size_t)(e / 244) * 16 + i] = t;
  }
#endif
};

// XCD-aware block remap: the dispatcher deals workgroups round-robin over the 8 XCDs
// (blocks b and b+8 share an XCD, MI355X_MICROARCH.md), so give each XCD one contiguous
// chunk of the element order: neighbouring elements then meet in the same L2.
// stripe > 0: XCD x takes every 8th STRIPE of `stripe` consecutive blocks instead of one contiguous eighth -- the element
// order is then dealt out evenly and no XCD is left with the expensive (plastic) end of the mesh; the grid must be a
// multiple of 8 * stripe (stripe_grid).  The kernels that add into shared rows with atomics keep the contiguous eighths
// (their neighbours meet in one L2); the staged Jacobian kernels and the per-element ones use stripes: 11.02 against
// 11.23-11.32 ms per assembly (gpurun_out/tune_xcd.log).
#ifndef C8_TUNE_STAGE_STRIPE
#define C8_TUNE_STAGE_STRIPE 32
#endif
constexpr int STAGE_STRIPE = C8_TUNE_STAGE_STRIPE;
inline int stripe_grid(int nblocks, int stripe) { return stripe ? ((nblocks + 8 * stripe - 1) / (8 * stripe)) * (8 * stripe) : ((nblocks + 7) / 8) * 8; }
__device__ __forceinline__ int xcd_stripe(int b, int stripe) {
  int const x = b & 7, k = b >> 3;  // k-th block of XCD x
  int const s = stripe > 0 ? stripe : 1;
  return ((k / s) * 8 + x) * s + (k % s);
}
__device__ __forceinline__ int xcd_block(int b, int nblocks) {
#if defined(C8_TUNE_NO_XCD_REMAP)   // tuning build (same results): blocks in launch order, round-robin over the XCDs
  return b;
#elif defined(C8_TUNE_XCD_STRIPE)   // tuning build (same results): XCD x takes every 8th stripe of C8_TUNE_XCD_STRIPE blocks
  int const S = C8_TUNE_XCD_STRIPE;
  int const x = b & 7, k = b >> 3;        // k-th block of XCD x
  return ((k / S) * 8 + x) * S + (k % S);
#else
  int const chunk = (nblocks + 7) >> 3;
  return (b & 7) * chunk + (b >> 3);
#endif
}

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_forward_jacobian(MeshTables mt, ModelSettings ms, FieldArgs fa, SystemArgs sa,
                                                          int first, int count, int nblocks) {
  constexpr int GPB = BLOCK / E::NDOF;
  using Lane = ForwardLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const gib = threadIdx.x / E::NDOF, k = threadIdx.x % E::NDOF;
  if (gib >= GPB) return;  // lanes left over when NDOF does not divide the block (tri3: 7 groups of 9)
  int const gi = lb * GPB + gib;
  if (gi >= count) return;
  int const e = mt.order ? mt.order[first + gi] : first + gi;
  Lane L;
  GpuExec<Lane> ex(k, L);
  forward_jacobian_element<E, ModelT>(ex, shs[gib], mt, ms, fa, sa, e);
}

// K1 in lane groups with the model's closed form (Model::HAS_CLOSED_FORM) in place of the local Newton iteration and the AD
// passes of the first ip set
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_forward_jacobian_closed(MeshTables mt, ModelSettings ms, FieldArgs fa, SystemArgs sa,
                                                                 int first, int count, int nblocks) {
  constexpr int GPB = BLOCK / E::NDOF;
  using Lane = ForwardLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const gib = threadIdx.x / E::NDOF, k = threadIdx.x % E::NDOF;
  if (gib >= GPB) return;
  int const gi = lb * GPB + gib;
  if (gi >= count) return;
  int const e = mt.order ? mt.order[first + gi] : first + gi;
  Lane L;
  GpuExec<Lane> ex(k, L);
  forward_jacobian_element<E, ModelT, true>(ex, shs[gib], mt, ms, fa, sa, e);
}

template <class E, template <class> class ModelT>
static hipError_t launch_forward(LaunchArgs const& a) {
  constexpr int GPB = BLOCK / E::NDOF;
  int const nblocks = (a.count + GPB - 1) / GPB;
  int const grid = ((nblocks + 7) / 8) * 8;
  if (a.count <= 0) return hipSuccess;
  if constexpr (has_closed_form<ModelT<Dual>>::value) {
    if (a.ms.closed_form_slot) {
      hipLaunchKernelGGL((k_forward_jacobian_closed<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.sa,
                         a.first, a.count, nblocks);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((k_forward_jacobian<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.sa,
                     a.first, a.count, nblocks);
  return hipGetLastError();
}

// One wavefront per workgroup for the wave Jacobian kernels: a workgroup's registers and LDS are released only when
// its last wavefront retires, and element durations differ (elastic / plastic points, Newton iterations), so with four
// wavefronts per workgroup finished slots idle until the slowest is done (12.5 ms against 12.7-12.9 ms).
#ifndef C8_JBLOCK
#define C8_JBLOCK 64
#endif
constexpr int JBLOCK = C8_JBLOCK;
// K1, one wavefront per hex8 element (c8_assemble_wave.hpp)
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(JBLOCK) __attribute__((amdgpu_waves_per_eu(ModelT<Dual>::WAVE_BLOCKS_PER_CU, ModelT<Dual>::WAVE_BLOCKS_PER_CU)))
k_forward_jacobian_wave(MeshTables mt, ModelSettings ms, FieldArgs fa, SystemArgs sa,
                                                               int first, int count, int nblocks) {
  constexpr int WPB = JBLOCK / 64;
  using Lane = WaveLane<ModelT>;
  __shared__ WaveShared<E, ModelT<Dual>::NLOC, false, ModelT<Dual>::FINITE_DEF> shs[WPB];
  int const lb = (sa.stage && STAGE_STRIPE) ? xcd_stripe(blockIdx.x, STAGE_STRIPE) : xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const gi = lb * WPB + wib;
  if (gi >= count) return;
  int const e = mt.order ? mt.order[first + gi] : first + gi;
  Lane L;
  GpuExec<Lane> ex(lane, L);
  forward_jacobian_wave<E, ModelT>(ex, shs[wib], mt, ms, fa, sa, e);
}

#ifndef C8_CLOSED_WAVES
#define C8_CLOSED_WAVES 3  // 156 registers, 13.5 KB of LDS per wave: three waves per SIMD measured 0.6 % ahead of two
#endif
// K1 with the model's closed form (Model::HAS_CLOSED_FORM): no local Newton iteration, no local elimination, no AD passes
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(JBLOCK) __attribute__((amdgpu_waves_per_eu(C8_CLOSED_WAVES, C8_CLOSED_WAVES)))
k_forward_jacobian_wave_closed(MeshTables mt, ModelSettings ms, FieldArgs fa, SystemArgs sa,
                                                                         int first, int count, int nblocks) {
  constexpr int WPB = JBLOCK / 64;
  using Lane = WaveLane<ModelT>;
  __shared__ WaveShared<E, ModelT<Dual>::NLOC, false, ModelT<Dual>::FINITE_DEF, true> shs[WPB];
  int const lb = (sa.stage && STAGE_STRIPE) ? xcd_stripe(blockIdx.x, STAGE_STRIPE) : xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const gi = lb * WPB + wib;
  if (gi >= count) return;
  int const e = mt.order ? mt.order[first + gi] : first + gi;
  Lane L;
  GpuExec<Lane> ex(lane, L);
  forward_jacobian_wave_closed<E, ModelT>(ex, shs[wib], mt, ms, fa, sa, e);
}

template <class E, template <class> class ModelT>
static hipError_t launch_forward_wave(LaunchArgs const& a) {
  constexpr int WPB = JBLOCK / 64;
  int const nblocks = (a.count + WPB - 1) / WPB;
  int const grid = a.sa.stage ? stripe_grid(nblocks, STAGE_STRIPE) : ((nblocks + 7) / 8) * 8;
  if (a.count <= 0) return hipSuccess;
  if constexpr (has_closed_form<ModelT<Dual>>::value) {
    if (a.ms.closed_form) {
      hipLaunchKernelGGL((k_forward_jacobian_wave_closed<E, ModelT>), dim3(grid), dim3(JBLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.sa,
                         a.first, a.count, nblocks);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((k_forward_jacobian_wave<E, ModelT>), dim3(grid), dim3(JBLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.sa,
                     a.first, a.count, nblocks);
  return hipGetLastError();
}

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(JBLOCK) __attribute__((amdgpu_waves_per_eu(ModelT<Dual>::WAVE_BLOCKS_PER_CU, ModelT<Dual>::WAVE_BLOCKS_PER_CU)))
k_adjoint_jacobian_wave(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa,
                                                                  SystemArgs sa, int first, int count, int nblocks) {
  constexpr int WPB = JBLOCK / 64;
  using Lane = WaveLane<ModelT>;
  __shared__ WaveShared<E, ModelT<Dual>::NLOC, true, ModelT<Dual>::FINITE_DEF> shs[WPB];
  int const lb = (sa.stage && STAGE_STRIPE) ? xcd_stripe(blockIdx.x, STAGE_STRIPE) : xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const gi = lb * WPB + wib;
  if (gi >= count) return;
  int const e = mt.order ? mt.order[first + gi] : first + gi;
  Lane L;
  GpuExec<Lane> ex(lane, L);
  adjoint_jacobian_wave<E, ModelT, PointQoi>(ex, shs[wib], mt, ms, fa, aa, sa, e);
}

template <class E, template <class> class ModelT>
static hipError_t launch_adjoint_jacobian_wave(LaunchArgs const& a) {
  constexpr int WPB = JBLOCK / 64;
  int const nblocks = (a.count + WPB - 1) / WPB;
  int const grid = a.sa.stage ? stripe_grid(nblocks, STAGE_STRIPE) : ((nblocks + 7) / 8) * 8;
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_adjoint_jacobian_wave<E, ModelT>), dim3(grid), dim3(JBLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa,
                     a.sa, a.first, a.count, nblocks);
  return hipGetLastError();
}

#ifdef C8_TUNE_K4_WAVES  // tuning build (same results): waves per SIMD of the local-adjoint kernel, every model
#define C8_K4_WAVES(M) C8_TUNE_K4_WAVES
#else
#define C8_K4_WAVES(M) M::WAVE_BLOCKS_PER_CU_K4
#endif
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(JBLOCK) __attribute__((amdgpu_waves_per_eu(C8_K4_WAVES(ModelT<Dual>), C8_K4_WAVES(ModelT<Dual>))))
k_adjoint_local_wave(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa,
                                                               SystemArgs sa, int first, int count, int nblocks) {
  constexpr int WPB = JBLOCK / 64;
  using Lane = WaveLaneA<ModelT>;
  __shared__ WaveSharedA<E, ModelT<Dual>::NLOC> shs[WPB];
  int const lb = STAGE_STRIPE ? xcd_stripe(blockIdx.x, STAGE_STRIPE) : xcd_block(blockIdx.x, nblocks);  // per-element outputs only: stripes
  if (lb >= nblocks) return;
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const gi = lb * WPB + wib;
  if (gi >= count) return;
  Lane L;
  GpuExec<Lane> ex(lane, L);
  adjoint_local_wave<E, ModelT>(ex, shs[wib], mt, ms, fa, aa, sa, first + gi);
}

// CLOSED: the model's closed form of the point's share (Model::closed_form_param_gradient) instead of dual numbers
template <class E, template <class> class ModelT, bool CLOSED = false>
__global__ void __launch_bounds__(BLOCK, CLOSED ? 2 : ModelT<Dual>::WAVE_BLOCKS_PER_CU_ADJ) k_param_gradient_wave(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa, int count) {
  constexpr int WPB = BLOCK / 64;
  using Lane = GradWaveLane<ModelT>;
  __shared__ GradWaveShared<E> shs[WPB];
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  Lane L;
  L.slot0 = -1;
  C8_UNROLL
  for (int a = 0; a < 8; ++a) L.acc[a] = 0.;
  GpuExec<Lane> ex(lane, L);
  int const ngroups = (count + 7) / 8;
  for (int gidx = blockIdx.x * WPB + wib; gidx < ngroups; gidx += gridDim.x * WPB)
    param_gradient_wave8<E, ModelT, PointQoi, CLOSED>(ex, shs[wib], mt, ms, fa, aa, gidx * 8, (count - gidx * 8 < 8) ? count - gidx * 8 : 8);
  param_gradient_wave8_flush(ex, shs[wib].red, aa);
}

// K4 in closed form (adjoint_local_closed_wave8): eight consecutive elements per wavefront
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_adjoint_local_closed(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa, int first, int count) {
  constexpr int WPB = BLOCK / 64;
  __shared__ GradWaveShared<E> shs[WPB];
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const gidx = blockIdx.x * WPB + wib;
  if (gidx * 8 >= count) return;
  NoLane L;
  GpuExec<NoLane> ex(lane, L);
  adjoint_local_closed_wave8<E, ModelT>(ex, shs[wib], mt, ms, fa, aa, first + gidx * 8, (count - gidx * 8 < 8) ? count - gidx * 8 : 8);
}
template <class E, template <class> class ModelT> static hipError_t launch_adjoint_local_closed(LaunchArgs const& a) {
  constexpr int WPB = BLOCK / 64;
  if (a.count <= 0) return hipSuccess;
  int const ngroups = (a.count + 7) / 8;
  hipLaunchKernelGGL((k_adjoint_local_closed<E, ModelT>), dim3((ngroups + WPB - 1) / WPB), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.first, a.count);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_adjoint_local_wave(LaunchArgs const& a) {
  constexpr int WPB = JBLOCK / 64;
  int const nblocks = (a.count + WPB - 1) / WPB;
  int const grid = stripe_grid(nblocks, STAGE_STRIPE);
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_adjoint_local_wave<E, ModelT>), dim3(grid), dim3(JBLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.sa,
                     a.first, a.count, nblocks);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_param_gradient_wave(LaunchArgs const& a) {
  constexpr int WPB = BLOCK / 64;
  if (a.count <= 0) return hipSuccess;
  int const ngroups = (a.count + 7) / 8;
  int const nblocks = (ngroups + WPB - 1) / WPB;
  int const grid = nblocks < 2048 ? nblocks : 2048;
  hipLaunchKernelGGL((k_param_gradient_wave<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.count);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_param_gradient_closed(LaunchArgs const& a) {
  constexpr int WPB = BLOCK / 64;
  if (a.count <= 0) return hipSuccess;
  int const ngroups = (a.count + 7) / 8;
  int const nblocks = (ngroups + WPB - 1) / WPB;
  int const grid = nblocks < 2048 ? nblocks : 2048;
  hipLaunchKernelGGL((k_param_gradient_wave<E, ModelT, true>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.count);
  return hipGetLastError();
}

// cached shape tables of the wave kernels: one wavefront per element, once per context
template <class E> __global__ void __launch_bounds__(64) k_shape_tables(MeshTables mt, double* tab, int nelems) {
  __shared__ ShapeShared<E> sh;
  int const e = blockIdx.x;
  if (e >= nelems) return;
  ShapeLane L;
  GpuExec<ShapeLane> ex(threadIdx.x, L);
  store_shape_tables<E>(ex, sh, mt, tab, e);
}
template <class E> static hipError_t launch_shape_tables(MeshTables const& mt, double* tab, int nelems, hipStream_t stream) {
  if (nelems <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_shape_tables<E>), dim3(nelems), dim3(64), 0, stream, mt, tab, nelems);
  return hipGetLastError();
}

// K2 for hex8: eight elements per wavefront, 32 per workgroup (residual_wave8)
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK, 2) k_residual_wave(MeshTables mt, ModelSettings ms, FieldArgs fa, SystemArgs sa,
                                                          int count, int nblocks) {
  constexpr int WPB = BLOCK / 64;
  using Lane = ResidualWaveLane<ModelT>;
  __shared__ ResidualWaveShared<E> shs[WPB];
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const e0 = (lb * WPB + wib) * 8;
  if (e0 >= count) return;
  Lane L;
  GpuExec<Lane> ex(lane, L);
  residual_wave8<E, ModelT>(ex, shs[wib], mt, ms, fa, sa, e0, (count - e0 < 8) ? count - e0 : 8);
}
template <class E, template <class> class ModelT> static hipError_t launch_residual_wave(LaunchArgs const& a) {
  constexpr int EPB = (BLOCK / 64) * 8;
  if (a.count <= 0) return hipSuccess;
  int const nblocks = (a.count + EPB - 1) / EPB;
  int const grid = ((nblocks + 7) / 8) * 8;
  hipLaunchKernelGGL((k_residual_wave<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.sa, a.count, nblocks);
  return hipGetLastError();
}

// staged assembly: one wavefront per node sums the node's rows from the element-major stage
template <class E, int MAXDEG>
__global__ void __launch_bounds__(BLOCK) k_gather_rows(GatherArgs ga, int first, int count, int nblocks) {
  constexpr int WPB = BLOCK / 64;
  __shared__ GatherShared<E, MAXDEG> shs[WPB];
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  int const gi = lb * WPB + wib;
  if (gi >= count) return;
  GatherLane<E, MAXDEG> L;
  GpuExec<GatherLane<E, MAXDEG>> ex(lane, L);
  gather_node_rows<E, MAXDEG>(ex, shs[wib], ga, ga.node_order[first + gi]);
}
template <class E> static hipError_t launch_gather_rows(GatherArgs const& ga, int first, int count, int max_degree, hipStream_t stream) {
  constexpr int WPB = BLOCK / 64;
  if (count <= 0) return hipSuccess;
  int const nblocks = (count + WPB - 1) / WPB;
  int const grid = ((nblocks + 7) / 8) * 8;
  if (max_degree <= 32)
    hipLaunchKernelGGL((k_gather_rows<E, 32>), dim3(grid), dim3(BLOCK), 0, stream, ga, first, count, nblocks);
  else if (max_degree <= GATHER_MAX_DEGREE)
    hipLaunchKernelGGL((k_gather_rows<E, GATHER_MAX_DEGREE>), dim3(grid), dim3(BLOCK), 0, stream, ga, first, count, nblocks);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// K1, one wavefront per node (c8_assemble_node.hpp): the node's rows formed from its elements with the model's closed form
// and written once -- no element stage.  XCD x takes every 8th stripe of NODE_STRIPE consecutive nodes: neighbouring nodes
// share their elements' shape tables and state in one L2, and the eight XCDs work on one region of the mesh at a time.
// Measured on the 100^3 brick (K1 ms / K3 ms / HBM-side GB per assembly with FETCH_SIZE doubled): stripes of 64: 4.37 / 5.20 /
// 16.9; 256: 4.33 / 5.12 / 13.9; 512: 4.36 / 5.21 / 13.0; 1024: 4.36 / 5.30 / 12.5; 2048: 4.36 / 5.28 / 12.3; 16384 and one
// contiguous eighth of the nodes per XCD: 4.71 / - / 12.1 (profiles/README.md, round 3).  Those are the figures of the kernel
// before its index and shape-value bookkeeping was stripped; with stripes of 256 the kernels without that
// bookkeeping took 4.22 / 5.11-5.14 ms beside 4.40 / 5.15-5.17 ms of their predecessors in one call (profiles/README.md,
// node_image_*).  The present kernels take phase A's gradients from the cached inverse Jacobian instead of the dN/dx table:
// 3.68 / 4.51 ms beside 4.18 / 5.21 ms of those in one call (profiles/README.md, jinv_*).  They also issue phase
// A2's table and state loads beside the connectivity and two of phase B's first rows under the closed form (same loads, same
// bits, one dependent round trip earlier each): 3.54 / 4.35 ms beside 3.61 / 4.44 ms in one call (last part;
// profiles/README.md, chain_*).  Phase B no longer walks the dN/dx table: a column node's gradient is formed from the inverse
// Jacobian by the lane that holds it and handed over by GpuExec::xor8 (16 vector-memory instructions and 24 eight-byte units per
// lane and node less, 60 DPP moves and about 110 vector-ALU instructions more): 3.31-3.33 / 3.78-3.79 ms beside 3.62-3.63 /
// 4.46 ms in one call (profiles/README.md, xlane_*).  Phase B now sums over an element's points first and
// combines the terms of the block once, after the eighth point (Model::closed_form_block_sums / _finish: 41 operations per
// step and 24 at the end instead of 59 per step; 111 of 868 FP64 instructions less in K1, 128 registers, four wavefronts
// per SIMD as before): 3.15-3.16 / 3.65-3.66 ms beside 3.35-3.36 / 3.79-3.82 ms in one call (last part;
// profiles/README.md, sums_*).  The rows now go in and out through one buffer descriptor per CSR block (GpuExec::row_load /
// row_store: the address unit checks the range, no compare, exec-mask region or 64-bit address per lane), the accumulator is
// zeroed whole in 16-byte LDS writes, and K1 reads what the closed form computes from the parameters alone from a table per
// element set (MeshTables::cf_const, k_closed_form_constants) instead of forming five reciprocals at every point: 1 767 ->
// 1 525 static instructions in the lean K1 (FP64 763 -> 722, other vector ALU 418 -> 313, scalar 403 -> 313), the same
// bits: 2.98-3.01 / 3.53-3.60 ms beside 3.07-3.11 / 3.57-3.66 ms in one call (last part; profiles/README.md,
// rowio_*).
#ifndef C8_NODE_WAVES
#define C8_NODE_WAVES 3
#endif
#ifndef C8_TUNE_NODE_STRIPE
#define C8_TUNE_NODE_STRIPE 256
#endif
constexpr int NODE_STRIPE = C8_TUNE_NODE_STRIPE;
template <class E, template <class> class ModelT, int MAXDEG, bool MANY>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MANY ? 2 : C8_NODE_WAVES, 4)))
k_node_rows_closed(MeshTables mt, ModelSettings ms, FieldArgs fa, GatherArgs ga, int first, int count, int nblocks) {
  using Lane = NodeLane<MAXDEG>;
  __shared__ NodeShared<E, ModelT<Dual>, MAXDEG, MANY> sh;
  int const lb = xcd_stripe(blockIdx.x, NODE_STRIPE);
  if (lb >= count) return;
  Lane L;
  GpuExec<Lane> ex(threadIdx.x, L);
  node_rows_closed<E, ModelT, MAXDEG, MANY>(ex, sh, mt, ms, fa, ga, first + lb);  // nodes [first, first + count)
}
// K3 in the same form (objective "average displacement"): the transposed rows and the adjoint right-hand side
template <class E, template <class> class ModelT, int MAXDEG, bool MANY>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MANY ? 2 : C8_NODE_WAVES, 4)))
k_node_rows_closed_adjoint(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa, GatherArgs ga, int first, int count, int nblocks) {
  using Lane = NodeLane<MAXDEG>;
  __shared__ NodeShared<E, ModelT<Dual>, MAXDEG, MANY> sh;
  int const lb = xcd_stripe(blockIdx.x, NODE_STRIPE);
  if (lb >= count) return;
  Lane L;
  GpuExec<Lane> ex(threadIdx.x, L);
  node_rows_closed<E, ModelT, MAXDEG, MANY, true>(ex, sh, mt, ms, fa, ga, first + lb, aa);
}
// max_node_elems <= 8 (every hex8 mesh cut out of a structured one, most others): the lean form; otherwise a node's
// elements go through the kernel eight at a time
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(256) k_node_rows_update_g(MeshTables mt, AdjointArgs aa, size_t npoints) {
  size_t const qp = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (qp < npoints) node_rows_update_g<E, ModelT>(mt, aa, qp);
}
// first = -1: the update of g that closes an adjoint assembly under the calibration objective (count = elements)
template <class E, template <class> class ModelT>
static hipError_t launch_node_rows(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, AdjointArgs const* aa, GatherArgs const& ga,
                                   int first, int count, int max_degree, int max_node_elems, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (first < 0) {
    size_t const npoints = (size_t)count * E::NP0;
    hipLaunchKernelGGL((k_node_rows_update_g<E, ModelT>), dim3((unsigned)((npoints + 255) / 256)), dim3(256), 0, stream, mt, *aa, npoints);
    return hipGetLastError();
  }
  if (!mt.cf_const) return hipErrorInvalidValue;  // the kernels read the closed form's constants there
  int const nblocks = count;
  int const grid = stripe_grid(nblocks, NODE_STRIPE);
  bool const lean = max_degree <= 32 && max_node_elems <= 8;
  if (max_degree > GATHER_MAX_DEGREE) return hipErrorInvalidValue;
  if (aa) {  // adjoint assembly
    if (lean) hipLaunchKernelGGL((k_node_rows_closed_adjoint<E, ModelT, 32, false>), dim3(grid), dim3(64), 0, stream, mt, ms, fa, *aa, ga, first, count, nblocks);
    else hipLaunchKernelGGL((k_node_rows_closed_adjoint<E, ModelT, GATHER_MAX_DEGREE, true>), dim3(grid), dim3(64), 0, stream, mt, ms, fa, *aa, ga, first, count, nblocks);
  } else {
    if (lean) hipLaunchKernelGGL((k_node_rows_closed<E, ModelT, 32, false>), dim3(grid), dim3(64), 0, stream, mt, ms, fa, ga, first, count, nblocks);
    else hipLaunchKernelGGL((k_node_rows_closed<E, ModelT, GATHER_MAX_DEGREE, true>), dim3(grid), dim3(64), 0, stream, mt, ms, fa, ga, first, count, nblocks);
  }
  return hipGetLastError();
}
// The closed form's per-set constants (Model::closed_form_constants; MeshTables::cf_const): one lane per element set.  On the
// device, not on the host: c8_rcp is v_rcp_f64 and two Newton steps here and 1 / x there.
template <template <class> class ModelT>
__global__ void __launch_bounds__(64) k_closed_form_constants(double const* params, double* table, int nsets) {
  using Model = ModelT<Dual>;
  int const es = blockIdx.x * 64 + threadIdx.x;
  if (es < nsets) Model::closed_form_constants(params + (size_t)es * Model::NPARAMS, table + (size_t)es * Model::NCONST);
}
template <template <class> class ModelT>
static hipError_t launch_closed_form_constants(double const* params, double* table, int nsets, hipStream_t stream) {
  hipLaunchKernelGGL((k_closed_form_constants<ModelT>), dim3((unsigned)((nsets + 63) / 64)), dim3(64), 0, stream, params, table, nsets);
  return hipGetLastError();
}
template <class E, template <class> class ModelT, class = void> struct NodeKernel {
  static NodeRowsFn get() { return nullptr; }
  static ConstantsFn get_constants() { return nullptr; }
  static constexpr int NCONST = 0;
  static LaunchFn get_adjoint_local() { return nullptr; }
  static LaunchFn get_param_gradient() { return nullptr; }
};
template <template <class> class ModelT>
struct NodeKernel<Elem<C8_HEX8>, ModelT, std::enable_if_t<has_closed_form_rows<ModelT<Dual>>::value>> {
  static NodeRowsFn get() { return &launch_node_rows<Elem<C8_HEX8>, ModelT>; }
  static ConstantsFn get_constants() { return &launch_closed_form_constants<ModelT>; }
  static constexpr int NCONST = ModelT<Dual>::NCONST;
  static LaunchFn get_adjoint_local() { return &launch_adjoint_local_closed<Elem<C8_HEX8>, ModelT>; }
  static LaunchFn get_param_gradient() { return &launch_param_gradient_closed<Elem<C8_HEX8>, ModelT>; }
};

// group index -> element for the colour-batched / atomic element-parallel kernels
#define C8_GROUP_PROLOGUE(E)                                                  \
  constexpr int GPB = BLOCK / E::NDOF;                                        \
  int const lb = xcd_block(blockIdx.x, nblocks);                              \
  if (lb >= nblocks) return;                                                  \
  int const gib = threadIdx.x / E::NDOF, k = threadIdx.x % E::NDOF;           \
  if (gib >= GPB) return; /* lanes left over when NDOF does not divide the block (tri3: 7 groups of 9) */ \
  int const gi = lb * GPB + gib;                                              \
  if (gi >= count) return;                                                    \
  int const e = mt.order ? mt.order[first + gi] : first + gi;

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_residual(MeshTables mt, ModelSettings ms, FieldArgs fa, SystemArgs sa,
                                                  int first, int count, int nblocks) {
  C8_GROUP_PROLOGUE(E)
  using Lane = ResidualLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  Lane L;
  GpuExec<Lane> ex(k, L);
  residual_element<E, ModelT>(ex, shs[gib], mt, ms, fa, sa, e);
}

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_adjoint_jacobian(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa,
                                                          SystemArgs sa, int first, int count, int nblocks) {
  C8_GROUP_PROLOGUE(E)
  using Lane = AdjointLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  Lane L;
  GpuExec<Lane> ex(k, L);
  adjoint_jacobian_element<E, ModelT, PointQoi>(ex, shs[gib], mt, ms, fa, aa, sa, e);
}

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_adjoint_local(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa,
                                                       SystemArgs sa, int first, int count, int nblocks) {
  C8_GROUP_PROLOGUE(E)
  using Lane = AdjointLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  Lane L;
  GpuExec<Lane> ex(k, L);
  adjoint_local_element<E, ModelT>(ex, shs[gib], mt, ms, fa, aa, sa, e);
}

// K5/K6: each group walks the elements with a grid stride and adds its sums once at the end
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_param_gradient(MeshTables mt, ModelSettings ms, FieldArgs fa, AdjointArgs aa, int count) {
  constexpr int GPB = BLOCK / E::NDOF;
  using Lane = GradLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  int const gib = threadIdx.x / E::NDOF, k = threadIdx.x % E::NDOF;
  if (gib >= GPB) return;
  Lane L;
  L.slot = -1;
  L.acc = 0.;
  GpuExec<Lane> ex(k, L);
  for (int e = blockIdx.x * GPB + gib; e < count; e += gridDim.x * GPB)
    param_gradient_element<E, ModelT, PointQoi>(ex, shs[gib], mt, ms, fa, aa, e);
  param_gradient_flush(ex, aa);
}

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK) k_qoi(MeshTables mt, FieldArgs fa, AdjointArgs aa, int count) {
  constexpr int GPB = BLOCK / E::NDOF;
  using Lane = QoiLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  int const gib = threadIdx.x / E::NDOF, k = threadIdx.x % E::NDOF;
  if (gib >= GPB) return;
  Lane L;
  L.acc = 0.;
  GpuExec<Lane> ex(k, L);
  for (int e = blockIdx.x * GPB + gib; e < count; e += gridDim.x * GPB)
    qoi_element<E, ModelT, PointQoi>(ex, shs[gib], mt, fa, aa.qoi, e);
  qoi_flush<E>(ex, aa.out);
}

// K6 for hex8: eight elements per wavefront (qoi_wave8), grid-stride, one add per wavefront
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(BLOCK, 2) k_qoi_wave(MeshTables mt, FieldArgs fa, AdjointArgs aa, int count) {
  constexpr int WPB = BLOCK / 64;
  using Lane = QoiWaveLane<ModelT>;
  __shared__ GradWaveShared<E> shs[WPB];
  // the wave's index in the block is wave-uniform: as a scalar it keeps the element / node number and every address
  // derived from it in SGPRs (one wave per block: zero)
  int const wib = C8_WAVE_IN_BLOCK(WPB), lane = threadIdx.x & 63;
  Lane L;
  L.acc = 0.;
  GpuExec<Lane> ex(lane, L);
  int const ngroups = (count + 7) / 8;
  for (int gidx = blockIdx.x * WPB + wib; gidx < ngroups; gidx += gridDim.x * WPB)
    qoi_wave8<E, ModelT, PointQoi>(ex, shs[wib], mt, fa, aa.qoi, gidx * 8, (count - gidx * 8 < 8) ? count - gidx * 8 : 8);
  qoi_wave8_flush(ex, shs[wib].red, aa.out);
}
template <class E, template <class> class ModelT> static hipError_t launch_qoi_wave(LaunchArgs const& a) {
  constexpr int WPB = BLOCK / 64;
  if (a.count <= 0) return hipSuccess;
  int const ngroups = (a.count + 7) / 8;
  int const nblocks = (ngroups + WPB - 1) / WPB;
  int const grid = nblocks < 2048 ? nblocks : 2048;
  hipLaunchKernelGGL((k_qoi_wave<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.fa, a.aa, a.count);
  return hipGetLastError();
}

template <class E> static void grid_for(LaunchArgs const& a, int& nblocks, int& grid) {
  constexpr int GPB = BLOCK / E::NDOF;
  nblocks = (a.count + GPB - 1) / GPB;
  grid = ((nblocks + 7) / 8) * 8;
}

template <class E, template <class> class ModelT> static hipError_t launch_residual(LaunchArgs const& a) {
  int nblocks, grid;
  grid_for<E>(a, nblocks, grid);
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_residual<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.sa, a.first, a.count, nblocks);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_adjoint_jacobian(LaunchArgs const& a) {
  int nblocks, grid;
  grid_for<E>(a, nblocks, grid);
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_adjoint_jacobian<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.sa, a.first, a.count, nblocks);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_adjoint_local(LaunchArgs const& a) {
  int nblocks, grid;
  grid_for<E>(a, nblocks, grid);
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_adjoint_local<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.sa, a.first, a.count, nblocks);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_param_gradient(LaunchArgs const& a) {
  int nblocks, grid;
  grid_for<E>(a, nblocks, grid);
  if (a.count <= 0) return hipSuccess;
  grid = nblocks < 2048 ? nblocks : 2048;
  hipLaunchKernelGGL((k_param_gradient<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.ms, a.fa, a.aa, a.count);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static hipError_t launch_qoi(LaunchArgs const& a) {
  int nblocks, grid;
  grid_for<E>(a, nblocks, grid);
  if (a.count <= 0) return hipSuccess;
  grid = nblocks < 2048 ? nblocks : 2048;
  hipLaunchKernelGGL((k_qoi<E, ModelT>), dim3(grid), dim3(BLOCK), 0, a.stream, a.mt, a.fa, a.aa, a.count);
  return hipGetLastError();
}

// VFM (c8_assemble_vfm.hpp): one lane group per element as K1, KIND 0 = V, 1 = FS, 2 = A.  One wavefront per workgroup:
// after its groups are done the block writes one partial sum per output (vfm_block_sums, fixed order) and c8_vfm.hip sums
// the partials in a single block -- no floating-point atomics, the same bits on every run.
constexpr int VBLOCK = 64;
template <class E, template <class> class ModelT, int KIND>
__global__ void __launch_bounds__(VBLOCK) k_vfm(MeshTables mt, ModelSettings ms, FieldArgs fa, VfmArgs va, SystemArgs sa, double* part,
                                               int count, int nblocks) {
  constexpr int GPB = VBLOCK / E::NDOF;
  using Lane = VfmLane<E, ModelT>;
  __shared__ GroupShared<E, ModelT<Dual>::NLOC> shs[GPB];
  __shared__ VfmBlockSums<GPB, E::NDOF> red;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;  // the whole block
  int const gib = threadIdx.x / E::NDOF, k = threadIdx.x % E::NDOF;
  int const gi = lb * GPB + gib;
  if (gib < GPB && gi < count) {
    Lane L;
    GpuExec<Lane> ex(k, L);
    if constexpr (KIND == 2) vfm_adjoint_element<E, ModelT>(ex, shs[gib], mt, ms, fa, va, sa, gi);
    else vfm_power_element<E, ModelT, KIND == 1>(ex, shs[gib], mt, ms, fa, va, sa, gi);
    int32_t const* act = va.active + (mt.elem_set ? mt.elem_set[gi] : 0) * 10;
    vfm_group_sums(red, gib, k, L.acc_v, L.acc_g, act[0], act[1]);
  } else if (gib < GPB) {  // groups past the end of the mesh add nothing
    vfm_group_sums(red, gib, k, 0., 0., 0, 0);
  }
  __syncthreads();
  vfm_block_sums(red, threadIdx.x, VBLOCK, KIND != 2, KIND != 0 ? va.nact : 0, part, lb, nblocks);
}
template <class E, template <class> class ModelT, int KIND> static hipError_t launch_vfm(LaunchArgs const& a, VfmArgs const& va, double* part) {
  constexpr int GPB = VBLOCK / E::NDOF;
  if (a.count <= 0) return hipSuccess;
  int const nblocks = (a.count + GPB - 1) / GPB;
  int const grid = ((nblocks + 7) / 8) * 8;
  hipLaunchKernelGGL((k_vfm<E, ModelT, KIND>), dim3(grid), dim3(VBLOCK), 0, a.stream, a.mt, a.ms, a.fa, va, a.sa, part, a.count, nblocks);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> struct VfmKernel {
  static void set(KernelSet&) {}
};
template <template <class> class ModelT> struct VfmKernel<Tri3PlaneStress, ModelT> {
  static void set(KernelSet& ks) {
    if constexpr (!has_embedded<ModelT<Dual>>::value) {  // VFM with network weights: not available
      ks.vfm_power = &launch_vfm<Tri3PlaneStress, ModelT, 0>;
      ks.vfm_forward_sens = &launch_vfm<Tri3PlaneStress, ModelT, 1>;
      ks.vfm_adjoint = &launch_vfm<Tri3PlaneStress, ModelT, 2>;
      ks.vfm_groups_per_block = VBLOCK / Tri3PlaneStress::NDOF;
    }
  }
};

template <class E, template <class> class ModelT> struct WaveKernel {
  static LaunchFn get() { return nullptr; }
  static LaunchFn get_adjoint() { return nullptr; }
  static LaunchFn get_adjoint_local() { return nullptr; }
  static LaunchFn get_param_gradient() { return nullptr; }
  static LaunchFn get_residual() { return nullptr; }
  static LaunchFn get_qoi() { return nullptr; }
  static constexpr hipError_t (*shape_tables)(MeshTables const&, double*, int, hipStream_t) = nullptr;
};
template <template <class> class ModelT> struct WaveKernel<Elem<C8_HEX8>, ModelT> {
  static LaunchFn get() { return &launch_forward_wave<Elem<C8_HEX8>, ModelT>; }
  static LaunchFn get_adjoint() { return &launch_adjoint_jacobian_wave<Elem<C8_HEX8>, ModelT>; }
  static LaunchFn get_adjoint_local() { return &launch_adjoint_local_wave<Elem<C8_HEX8>, ModelT>; }
  static LaunchFn get_param_gradient() { return &launch_param_gradient_wave<Elem<C8_HEX8>, ModelT>; }
  static LaunchFn get_residual() { return &launch_residual_wave<Elem<C8_HEX8>, ModelT>; }
  static LaunchFn get_qoi() { return &launch_qoi_wave<Elem<C8_HEX8>, ModelT>; }
  static constexpr hipError_t (*shape_tables)(MeshTables const&, double*, int, hipStream_t) = &launch_shape_tables<Elem<C8_HEX8>>;
};

template <class E, template <class> class ModelT> static KernelSet kernel_set(ModelTag<ModelT>) {
  using WK = WaveKernel<E, ModelT>;
  KernelSet ks;
  ks.forward_jacobian = &launch_forward<E, ModelT>;
  ks.forward_jacobian_wave = WK::get();
  ks.adjoint_jacobian_wave = WK::get_adjoint();
  ks.adjoint_local_wave = WK::get_adjoint_local();
  ks.param_gradient_wave = WK::get_param_gradient();
  ks.residual = &launch_residual<E, ModelT>;
  ks.residual_wave = WK::get_residual();
  ks.adjoint_jacobian = &launch_adjoint_jacobian<E, ModelT>;
  ks.adjoint_local = &launch_adjoint_local<E, ModelT>;
  ks.param_gradient = &launch_param_gradient<E, ModelT>;
  ks.qoi = WK::get_qoi() ? WK::get_qoi() : &launch_qoi<E, ModelT>;
  ks.qoi_slot = &launch_qoi<E, ModelT>;
  ks.shape_tables = WK::shape_tables;
  ks.shape_stride = SHAPE_STRIDE;
  ks.gather_rows = &launch_gather_rows<E>;
  ks.node_rows = NodeKernel<E, ModelT>::get();
  ks.closed_form_constants = NodeKernel<E, ModelT>::get_constants();
  ks.num_constants = NodeKernel<E, ModelT>::NCONST;
  ks.adjoint_local_closed = NodeKernel<E, ModelT>::get_adjoint_local();
  ks.param_gradient_closed = NodeKernel<E, ModelT>::get_param_gradient();
  ks.stage_stride = stage_stride<E>();
  ks.adjoint_slot_stages = E::NDOF <= 16;  // the slot-per-lane adjoint kernel holds assembled columns only for small elements
  ks.can_stage = E::DIM == 3;              // the stage and the row-sum kernel are laid out for 3 + 1 equations per node
  VfmKernel<E, ModelT>::set(ks);
  return ks;
}

// The registry: the kernel sets of the rows of the model table (c8_registry.hpp).  The instantiations are compiled in
// PARTS -- this file is compiled once per part with -DC8_KERNEL_PART=n (calibr8_amd/build.py, in parallel) and once as a
// whole by the tools that read its assembly; the table gives the part of each row on each element type.
#ifndef C8_KERNEL_PART
#define C8_KERNEL_PART -1  // all parts in this translation unit
#endif
#define C8_PART(n) (C8_KERNEL_PART == -1 || C8_KERNEL_PART == (n))
template <int P> static KernelSet part_kernels(int elem_type, int model) {
  KernelSet ks;
  // hex8 before the other elements: the kernels of a part come out grouped by element, and the labels of their assembly
  // (numbered in order of instantiation) stay comparable between builds
  visit_models([&](auto row) {
    if constexpr (decltype(row)::hex8_part == P) { if (elem_type == C8_HEX8 && row.id == model) ks = kernel_set<Elem<C8_HEX8>>(row); }
  });
  visit_models([&](auto row) {
    using R = decltype(row);
    if constexpr (R::tet4_part == P) { if (elem_type == C8_TET4 && row.id == model) ks = kernel_set<Elem<C8_TET4>>(row); }
    if constexpr (R::tri3_part == P) { if (elem_type == C8_TRI3 && row.id == model) ks = kernel_set<typename R::Elem2D>(row); }
  });
  return ks;
}
// one entry point per part, defined in the part's translation unit
KernelSet kernels_part0(int elem_type, int model);
KernelSet kernels_part1(int elem_type, int model);
KernelSet kernels_part2(int elem_type, int model);
KernelSet kernels_part3(int elem_type, int model);
KernelSet kernels_part4(int elem_type, int model);
KernelSet kernels_part5(int elem_type, int model);
#if C8_PART(0)
KernelSet kernels_part0(int elem_type, int model) { return part_kernels<0>(elem_type, model); }
#endif
#if C8_PART(1)
KernelSet kernels_part1(int elem_type, int model) { return part_kernels<1>(elem_type, model); }
#endif
#if C8_PART(2)
KernelSet kernels_part2(int elem_type, int model) { return part_kernels<2>(elem_type, model); }
#endif
#if C8_PART(3)
KernelSet kernels_part3(int elem_type, int model) { return part_kernels<3>(elem_type, model); }
#endif
#if C8_PART(4)
KernelSet kernels_part4(int elem_type, int model) { return part_kernels<4>(elem_type, model); }

// the weight gradient of the embedded network (c8_assemble_nn.hpp): one block per NN_GRAD_POINTS points, then one thread
// per theta entry adds the partial rows in block order
struct BlockExec {
  template <class F> __device__ __forceinline__ void each(F f) { f((int)threadIdx.x); }
  __device__ __forceinline__ void sync() { __syncthreads(); }
};
__global__ void __launch_bounds__(NN_GRAD_THREADS) k_nn_param_gradient(NnGradArgs ga) {
  __shared__ double lds[NN_LDS_SIZE];
  BlockExec ex;
  nn_grad_block<HybridHyperJ2PlaneStress<double>>(ex, lds, ga, blockIdx.x);
}
__global__ void __launch_bounds__(256) k_nn_param_gradient_reduce(double const* part, int nblocks, int ntheta, double* out) {
  int const q = blockIdx.x * 256 + threadIdx.x;
  if (q < ntheta) nn_grad_reduce_entry(part, nblocks, ntheta, q, out);
}
hipError_t launch_nn_param_gradient(NnGradArgs const& ga, double* out, hipStream_t stream) {
  int const nblocks = nn_grad_blocks(ga.npts);
  if (nblocks <= 0 || ga.ntheta <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_nn_param_gradient, dim3(nblocks), dim3(NN_GRAD_THREADS), 0, stream, ga);
  hipError_t const e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_nn_param_gradient_reduce, dim3((ga.ntheta + 255) / 256), dim3(256), 0, stream, ga.part, nblocks, ga.ntheta, out);
  return hipGetLastError();
}
#endif
#if C8_PART(5)
KernelSet kernels_part5(int elem_type, int model) { return part_kernels<5>(elem_type, model); }
#endif

#if C8_PART(0)
KernelSet get_kernels(int elem_type, int model) {
  for (auto part : {kernels_part0, kernels_part1, kernels_part2, kernels_part3, kernels_part4, kernels_part5}) {
    KernelSet const ks = part(elem_type, model);
    if (ks.forward_jacobian) return ks;
  }
  return KernelSet{};
}
#endif

}  // namespace c8
