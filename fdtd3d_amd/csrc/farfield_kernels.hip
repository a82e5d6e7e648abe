// Radiation vectors of the equivalent currents on the faces of a box from the
// raw accumulators of a running-DFT monitor (models/farfield.py): per
// wavelength k, direction a and current
//
//   sum over the face cells c of avg(acc[k][0] + i acc[k][1])(c) exp(-i kappa_k rhat_a . r'(c)),
//   r'(c) = pos0 + dx * (cell index),
//
// each value the face-centre average of the 1, 2 or 4 accumulator samples
// around the cell, taken in fp64 (fp32 runs too).  TWO launches cover every
// face, current, direction and wavelength, in the style of flux_kernels.hip: a
// device table of fixed-size entries read through the constant address space,
// the block's entry by binary search over blk0.
//
// An entry is a face group: up to FAR_GROUP currents on the same cells (the
// four tangential-current terms of one box face), so one phase factor serves
// all of them.  A thread owns one direction for one (group, wavelength, cell
// split); a block covers FAR_BLOCK directions.  The block walks its cells in
// chunks of FAR_BLOCK, linearised (x, y, z) with z fastest: its threads load
// and average one cell each (monitor_dev.h face_avg, with the aligned 16-byte
// group load on z-normal faces) and park (re, im) of every
// current in LDS as fp64; then every thread loops over the chunk, reading LDS
// at a wave-uniform address (a broadcast: no bank conflicts).  The phase is an
// exact fp64 sincos at the start of every face row and of every chunk, and in
// between the thread's own step exp(-i kappa rhat_f dx) along the row axis f
// rotates it: at most FAR_BLOCK - 1 rotations since the last exact value.
//
// No atomics: a block writes its sums with plain stores to
// partials[row][k][current][a], row = (group, cell split); the splits are a
// pure function of the table.  The second launch folds the rows of every slot
// in the fixed order of the fold table, applying the sign.  The same input
// gives the same bits.
//
// The kernel checks nothing beyond the face extent and the direction count:
// the host verifies every operand's reach against its accumulator block
// (ops/hip_monitors.py dft_farfield).
#include "common.h"
#include "monitor_dev.h"

namespace {

constexpr int FAR_MAX_K = 8;
constexpr int FAR_BLOCK = 256;
constexpr int FAR_GROUP = 4;
constexpr int FAR_SLOTS = 6;

struct FarEnt {
  long long acc[FAR_GROUP];    // accumulator bases, [k][re|im][x][y][z'], 16-byte aligned
  long long plane[FAR_GROUP];  // elements of one [x][y][z'] block (re -> im; k -> k + 1 is twice that)
  double pos0[3];              // first face-cell centre relative to the phase origin, metres
  int sx[FAR_GROUP], sy[FAR_GROUP];  // x and y strides in elements (z' stride 1)
  int first[FAR_GROUP][3];     // first sample of the first face cell
  int flags[FAR_GROUP];        // bit a < 3: average first and first + 1 along axis a; bit 3: whole aligned z' groups
  int ext[3];                  // face extent in cells (1 along the normal)
  int ncur;                    // currents of the group, 1..FAR_GROUP
  int blk0;                    // first block of the entry
  int splits;                  // cell splits: the entry has splits * K * tiles blocks
  int prow0;                   // first partials row of the entry (one row per split)
  int pad;
};
static_assert(sizeof(FarEnt) == 216, "FarEnt layout (ops/dft.py FAR_ENT_SIZE)");

template <typename T>
__global__ __launch_bounds__(FAR_BLOCK) void k_far_partial(const FarEnt* __restrict__ tab, int n, int K, int A,
                                                            int tiles, const double* __restrict__ dirs,
                                                            const double* __restrict__ wn, double dx,
                                                            double* __restrict__ partials) {
  __shared__ double val[FAR_BLOCK][2 * FAR_GROUP];  // (re, im) of every current of the chunk's cells
  // the block's entry: binary search over blk0 (monitor_dev.h)
  const mon::ConstTab<FarEnt> E = (mon::ConstTab<FarEnt>)tab;
  const int b = (int)blockIdx.x;
  const int lo = mon::entry_of_block(tab, n, b);
  const int e0 = E[lo].ext[0], e1 = E[lo].ext[1], e2 = E[lo].ext[2];
  const int ncur = E[lo].ncur, splits = E[lo].splits;
  const int local = b - E[lo].blk0;
  const int tile = local % tiles, q = (local / tiles) % K, split = local / (tiles * K);
  const int tid = (int)threadIdx.x;
  const int a = tile * FAR_BLOCK + tid;
  const int ac = a < A ? a : A - 1;  // idle lanes of the last tile follow the last direction and store nothing
  const double kap = wn[q];
  const double rx = dirs[3 * (size_t)ac], ry = dirs[3 * (size_t)ac + 1], rz = dirs[3 * (size_t)ac + 2];
  const double px = E[lo].pos0[0], py = E[lo].pos0[1], pz = E[lo].pos0[2];
  // rows run along the fastest axis that has more than one cell
  const int rowlen = e2 > 1 ? e2 : (e1 > 1 ? e1 : e0);
  const double rf = e2 > 1 ? rz : (e1 > 1 ? ry : rx);
  double stc, sts;
  sincos(kap * rf * dx, &sts, &stc);
  sts = -sts;  // the step exp(-i kappa rhat_f dx)
  const int cells = e0 * e1 * e2;
  const int nchunks = (cells + FAR_BLOCK - 1) / FAR_BLOCK;
  const int c_begin = (int)((long long)split * nchunks / splits);
  const int c_end = (int)((long long)(split + 1) * nchunks / splits);
  double sr[FAR_GROUP], si[FAR_GROUP];
#pragma unroll
  for (int c = 0; c < FAR_GROUP; ++c) sr[c] = si[c] = 0.0;
  for (int ch = c_begin; ch < c_end; ++ch) {
    const int c0 = ch * FAR_BLOCK;
    const int cnt = min(FAR_BLOCK, cells - c0);
    if (tid < cnt) {
      const int idx = c0 + tid;
      const int k = idx % e2, jj = idx / e2;
      const int j = jj % e1, i = jj / e1;
#pragma unroll
      for (int c = 0; c < FAR_GROUP; ++c) {
        if (c < ncur) {
          const int sx = E[lo].sx[c], sy = E[lo].sy[c], fl = E[lo].flags[c];
          const long long plane = E[lo].plane[c];
          const T* p = (const T*)E[lo].acc[c] + (size_t)(2 * q) * plane + (size_t)(E[lo].first[c][0] + i) * sx +
                       (size_t)(E[lo].first[c][1] + j) * sy;
          const int z = E[lo].first[c][2] + k;
          val[tid][2 * c] = mon::face_avg<T>(p, sx, sy, z, fl, (fl >> 3) & 1);
          val[tid][2 * c + 1] = mon::face_avg<T>(p + plane, sx, sy, z, fl, (fl >> 3) & 1);
        }
      }
    }
    __syncthreads();
    int pos = 0;
    while (pos < cnt) {  // the segments of face rows inside the chunk (wave-uniform)
      const int idx = c0 + pos;
      const int seg = min(rowlen - idx % rowlen, cnt - pos);
      const int k = idx % e2, jj = idx / e2;
      const int j = jj % e1, i = jj / e1;
      const double arg = kap * (rx * (px + dx * i) + ry * (py + dx * j) + rz * (pz + dx * k));
      double pr, pi;
      sincos(arg, &pi, &pr);
      pi = -pi;
      for (int t = 0; t < seg; ++t) {
        const double* v = val[pos + t];
#pragma unroll
        for (int c = 0; c < FAR_GROUP; ++c) {
          if (c < ncur) {
            const double vr = v[2 * c], vi = v[2 * c + 1];
            sr[c] = fma(vr, pr, fma(-vi, pi, sr[c]));
            si[c] = fma(vr, pi, fma(vi, pr, si[c]));
          }
        }
        const double npr = fma(pr, stc, -(pi * sts));
        pi = fma(pr, sts, pi * stc);
        pr = npr;
      }
      pos += seg;
    }
    __syncthreads();
  }
  if (a < A) {
    const size_t row = (size_t)(E[lo].prow0 + split) * K + q;
#pragma unroll
    for (int c = 0; c < FAR_GROUP; ++c) {
      if (c < ncur) {
        double* o = partials + ((row * FAR_GROUP + c) * (size_t)A + a) * 2;
        o[0] = sr[c];
        o[1] = si[c];
      }
    }
  }
}

// out[k][a][slot] = the partials of the slot's fold entries fold[7 + 3 j ..] = (row, current, sign), j in
// fold[slot] .. fold[slot + 1], summed in that order; a slot without entries is zero.  One thread per (k, a, slot).
__global__ __launch_bounds__(FAR_BLOCK) void k_far_fold(const double* __restrict__ partials,
                                                         const int* __restrict__ fold, int K, int A,
                                                         double* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * FAR_BLOCK + threadIdx.x;
  if (idx >= (long long)K * A * FAR_SLOTS) return;
  const int slot = (int)(idx % FAR_SLOTS);
  const int a = (int)((idx / FAR_SLOTS) % A);
  const int q = (int)(idx / ((long long)FAR_SLOTS * A));
  double re = 0.0, im = 0.0;
  for (int j = fold[slot]; j < fold[slot + 1]; ++j) {
    const int row = fold[FAR_SLOTS + 1 + 3 * j], c = fold[FAR_SLOTS + 2 + 3 * j];
    const double sg = (double)fold[FAR_SLOTS + 3 + 3 * j];
    const double* p = partials + ((((size_t)row * K + q) * FAR_GROUP + c) * (size_t)A + a) * 2;
    re += sg * p[0];
    im += sg * p[1];
  }
  out[2 * idx] = re;
  out[2 * idx + 1] = im;
}

template <typename T>
int far_eval(const void* tab, int n, int nblocks, int K, int A, const void* dirs, const void* wn, double dx,
             const void* fold, void* partials, void* out, hipStream_t s) {
  if (A <= 0) return 0;
  if (K < 1 || K > FAR_MAX_K || n < 0 || nblocks < 0 || !fold || !out || !dirs || !wn) return (int)hipErrorInvalidValue;
  const int tiles = (A + FAR_BLOCK - 1) / FAR_BLOCK;
  if (nblocks > 0) {
    if (n < 1 || !tab || !partials) return (int)hipErrorInvalidValue;
    k_far_partial<T><<<nblocks, FAR_BLOCK, 0, s>>>((const FarEnt*)tab, n, K, A, tiles, (const double*)dirs,
                                                  (const double*)wn, dx, (double*)partials);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  const long long total = (long long)K * A * FAR_SLOTS;
  k_far_fold<<<(unsigned)((total + FAR_BLOCK - 1) / FAR_BLOCK), FAR_BLOCK, 0, s>>>(
      (const double*)partials, (const int*)fold, K, A, (double*)out);
  FDTD_RETURN_LAUNCH_STATUS();
}

}  // namespace

// The radiation vectors of a far-field monitor: `tab` = n device entries of
// fdtd_farfield_ent_size() bytes (nblocks = the last entry's blk0 + its splits
// * K * ceil(A / 256) blocks), `dirs` = A x 3 device doubles (unit vectors),
// `wn` = K device doubles (wavenumbers), `fold` = the device fold table (7
// slot starts, then (partials row, current, sign) per entry), `partials` =
// rows x K x 4 x A x 2 doubles of scratch, `out` = K x A x 6 x 2 doubles.
FDTD_API int fdtd_farfield_eval_f32(const void* tab, int n, int nblocks, int K, int A, const void* dirs,
                                    const void* wn, double dx, const void* fold, void* partials, void* out, void* s) {
  return far_eval<float>(tab, n, nblocks, K, A, dirs, wn, dx, fold, partials, out, (hipStream_t)s);
}
FDTD_API int fdtd_farfield_eval_f64(const void* tab, int n, int nblocks, int K, int A, const void* dirs,
                                    const void* wn, double dx, const void* fold, void* partials, void* out, void* s) {
  return far_eval<double>(tab, n, nblocks, K, A, dirs, wn, dx, fold, partials, out, (hipStream_t)s);
}
FDTD_API int fdtd_farfield_ent_size() { return (int)sizeof(FarEnt); }
