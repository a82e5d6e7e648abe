// Time-averaged Poynting flux through the faces of a box from the raw
// accumulators of a running-DFT monitor (models/flux.py): per face and
// frequency k the sum over the face cells of
//
//   sign * (Re E_b Re H_c + Im E_b Im H_c),
//
// each operand the face-centre average of the 1, 2 or 4 accumulator samples
// around the cell.  ONE launch covers every product of every face at every
// frequency, in the style of dft_kernels.hip: a device table of fixed-size
// entries (one product E_b x H_c on one face), the block's entry by binary
// search over blk0, table reads through the constant address space.
//
// A thread owns one face cell, linearised (x, y, z) with z fastest: lanes run
// along z on x- and y-normal faces and along y on z-normal faces (extent 1
// along z), where a lane reads the aligned 16-byte group around its one or two
// z samples.  Accumulators are converted to fp64 before they are averaged and
// multiplied (fp32 runs too): the net flux of a lossless scatterer is a small
// difference of large face sums.  The block's K sums are reduced within the
// wave by shuffles, across its 4 waves through LDS in a fixed order, and
// written with plain stores to partials[block][K]; a second small launch folds
// the partials of each face in a fixed order.  No atomics: the same input
// gives the same bits.
//
// The kernel checks nothing beyond the face extent: the host verifies every
// entry's reach against its accumulator block (ops/hip_monitors.py dft_flux).
#include "common.h"
#include "monitor_dev.h"

namespace {

constexpr int FLUX_MAX_K = 8;
constexpr int FLUX_BLOCK = 256;
constexpr int FLUX_WAVES = FLUX_BLOCK / 64;

struct FluxEnt {
  long long e, h;            // accumulator bases, [k][re|im][x][y][z'], 16-byte aligned
  long long eplane, hplane;  // elements of one [x][y][z'] block (re -> im; k -> k + 1 is twice that)
  int esx, esy, hsx, hsy;    // x and y strides in elements (z' stride 1)
  int e0[3], h0[3];          // first sample of the first face cell
  int ext[3];                // face extent in cells (1 along the normal)
  int eavg, havg;            // bit a: average the samples first and first + 1 along axis a
  int face;                  // row of the result
  int sign;                  // +1 / -1
  int blk0;                  // first block of the entry
  int zvec;                  // z-normal face with whole aligned z' groups: vector loads
  int pad;
};
static_assert(sizeof(FluxEnt) == 112, "FluxEnt layout (ops/dft.py FLUX_ENT_SIZE)");

template <typename T, bool ZVEC>
__device__ __forceinline__ void flux_cell(const FluxEnt& e, int idx, int K, double (&acc)[FLUX_MAX_K]) {
  const int k = idx % e.ext[2], jj = idx / e.ext[2];
  const int j = jj % e.ext[1], i = jj / e.ext[1];
  const T* E = (const T*)e.e + (size_t)(e.e0[0] + i) * e.esx + (size_t)(e.e0[1] + j) * e.esy;
  const T* H = (const T*)e.h + (size_t)(e.h0[0] + i) * e.hsx + (size_t)(e.h0[1] + j) * e.hsy;
  const int ze = e.e0[2] + k, zh = e.h0[2] + k;
  const double sg = (double)e.sign;
#pragma unroll
  for (int q = 0; q < FLUX_MAX_K; ++q) {
    if (q < K) {
      const double er = mon::face_avg<T>(E + (size_t)(2 * q) * e.eplane, e.esx, e.esy, ze, e.eavg, ZVEC);
      const double ei = mon::face_avg<T>(E + (size_t)(2 * q + 1) * e.eplane, e.esx, e.esy, ze, e.eavg, ZVEC);
      const double hr = mon::face_avg<T>(H + (size_t)(2 * q) * e.hplane, e.hsx, e.hsy, zh, e.havg, ZVEC);
      const double hi = mon::face_avg<T>(H + (size_t)(2 * q + 1) * e.hplane, e.hsx, e.hsy, zh, e.havg, ZVEC);
      acc[q] = sg * __dadd_rn(__dmul_rn(er, hr), __dmul_rn(ei, hi));
    }
  }
}

// sum over the block's threads of v, valid in thread 0..K-1 for column q = thread
__device__ __forceinline__ void flux_block_sums(const double (&acc)[FLUX_MAX_K], int K, double (*red)[FLUX_MAX_K]) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < FLUX_MAX_K; ++q) {
    if (q < K) {
      const double v = mon::wave_sum(acc[q]);
      if (lane == 0) red[wave][q] = v;
    }
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(FLUX_BLOCK) void k_flux_partial(const FluxEnt* __restrict__ tab, int n, int K,
                                                              double* __restrict__ partials) {
  __shared__ double red[FLUX_WAVES][FLUX_MAX_K];
  // the block's entry: binary search over blk0 (monitor_dev.h)
  const mon::ConstTab<FluxEnt> E = (mon::ConstTab<FluxEnt>)tab;
  const int b = (int)blockIdx.x;
  const int lo = mon::entry_of_block(tab, n, b);
  FluxEnt e;  // (field by field: the constant-address-space entry has no implicit copy)
  e.e = E[lo].e;
  e.h = E[lo].h;
  e.eplane = E[lo].eplane;
  e.hplane = E[lo].hplane;
  e.esx = E[lo].esx;
  e.esy = E[lo].esy;
  e.hsx = E[lo].hsx;
  e.hsy = E[lo].hsy;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e.e0[d] = E[lo].e0[d];
    e.h0[d] = E[lo].h0[d];
    e.ext[d] = E[lo].ext[d];
  }
  e.eavg = E[lo].eavg;
  e.havg = E[lo].havg;
  e.sign = E[lo].sign;
  e.blk0 = E[lo].blk0;
  e.zvec = E[lo].zvec;
  double acc[FLUX_MAX_K];
#pragma unroll
  for (int q = 0; q < FLUX_MAX_K; ++q) acc[q] = 0.0;
  const int idx = (b - e.blk0) * FLUX_BLOCK + (int)threadIdx.x;
  if (idx < e.ext[0] * e.ext[1] * e.ext[2]) {
    if (e.zvec)
      flux_cell<T, true>(e, idx, K, acc);
    else
      flux_cell<T, false>(e, idx, K, acc);
  }
  flux_block_sums(acc, K, red);
  const int q = (int)threadIdx.x;
  if (q < K) {
    double v = red[0][q];
#pragma unroll
    for (int w = 1; w < FLUX_WAVES; ++w) v += red[w][q];
    partials[(size_t)b * K + q] = v;
  }
}

// out[f][q] = the partials of the face's blocks fblk[f] .. fblk[f + 1], summed
// in a fixed order: one block per face, thread t takes blocks t, t + 256, ...
__global__ __launch_bounds__(FLUX_BLOCK) void k_flux_fold(const double* __restrict__ partials,
                                                           const int* __restrict__ fblk, int K,
                                                           double* __restrict__ out) {
  __shared__ double red[FLUX_WAVES][FLUX_MAX_K];
  const int f = (int)blockIdx.x;
  const int b0 = fblk[f], b1 = fblk[f + 1];
  double acc[FLUX_MAX_K];
#pragma unroll
  for (int q = 0; q < FLUX_MAX_K; ++q) acc[q] = 0.0;
  for (int b = b0 + (int)threadIdx.x; b < b1; b += FLUX_BLOCK) {
#pragma unroll
    for (int q = 0; q < FLUX_MAX_K; ++q)
      if (q < K) acc[q] += partials[(size_t)b * K + q];
  }
  flux_block_sums(acc, K, red);
  const int q = (int)threadIdx.x;
  if (q < K) {
    double v = red[0][q];
#pragma unroll
    for (int w = 1; w < FLUX_WAVES; ++w) v += red[w][q];
    out[(size_t)f * K + q] = v;
  }
}

template <typename T>
int flux_eval(const void* tab, int n, int nblocks, int K, const void* fblk, int F, void* partials, void* out,
              hipStream_t s) {
  if (F <= 0) return 0;
  if (K < 1 || K > FLUX_MAX_K || n < 0 || nblocks < 0 || !fblk || !out) return (int)hipErrorInvalidValue;
  if (nblocks > 0) {
    if (n < 1 || !tab || !partials) return (int)hipErrorInvalidValue;
    k_flux_partial<T><<<nblocks, FLUX_BLOCK, 0, s>>>((const FluxEnt*)tab, n, K, (double*)partials);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  k_flux_fold<<<F, FLUX_BLOCK, 0, s>>>((const double*)partials, (const int*)fblk, K, (double*)out);
  FDTD_RETURN_LAUNCH_STATUS();
}

}  // namespace

// The face sums of a flux monitor: `tab` = n device entries of
// fdtd_flux_ent_size() bytes ordered by face (nblocks = the last entry's blk0
// + its blocks), `fblk` = F + 1 device ints, the first block of every face,
// `partials` = nblocks x K doubles of scratch, `out` = F x K doubles.
FDTD_API int fdtd_flux_eval_f32(const void* tab, int n, int nblocks, int K, const void* fblk, int F, void* partials,
                                void* out, void* s) {
  return flux_eval<float>(tab, n, nblocks, K, fblk, F, partials, out, (hipStream_t)s);
}
FDTD_API int fdtd_flux_eval_f64(const void* tab, int n, int nblocks, int K, const void* fblk, int F, void* partials,
                                void* out, void* s) {
  return flux_eval<double>(tab, n, nblocks, K, fblk, F, partials, out, (hipStream_t)s);
}
FDTD_API int fdtd_flux_ent_size() { return (int)sizeof(FluxEnt); }
