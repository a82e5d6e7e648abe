// Device code shared by the monitor kernels (dft, flux, farfield and energy
// _kernels.hip): the block-to-entry lookup of their device tables, the
// face-centre average of accumulator samples, the wave stage of their sums.
#pragma once

#include "common.h"

namespace mon {

// a device table through the constant address space: wave-uniform scalar loads
template <typename Ent>
using ConstTab = const __attribute__((address_space(4))) Ent*;

// the entry of block b among n entries ordered by blk0, their first blocks
template <typename Ent>
__device__ __forceinline__ int entry_of_block(const Ent* tab, int n, int b) {
  const ConstTab<Ent> E = (ConstTab<Ent>)tab;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (E[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// s += the one or two z samples of a row at z (in this order); zvec: rows are
// whole aligned 16-byte groups, and the lane loads the group around z
template <typename T>
__device__ __forceinline__ void face_row(const T* __restrict__ row, int z, bool two, bool zvec, double& s) {
  constexpr int V = 16 / sizeof(T);
  typedef T VT __attribute__((ext_vector_type(V)));
  if (zvec) {
    const int g = z & ~(V - 1), l = z - g;
    const VT v = *reinterpret_cast<const VT*>(row + g);
    T a = v[0], b = v[V - 1];
#pragma unroll
    for (int m = 1; m < V; ++m) a = (m == l) ? v[m] : a;
    s = __dadd_rn(s, (double)a);
    if (two) {
      if (l + 1 < V) {
#pragma unroll
        for (int m = 1; m < V; ++m) b = (m == l + 1) ? v[m] : b;
      } else {
        b = row[z + 1];  // the next group (the padded extent holds it)
      }
      s = __dadd_rn(s, (double)b);
    }
  } else {
    s = __dadd_rn(s, (double)row[z]);
    if (two) s = __dadd_rn(s, (double)row[z + 1]);
  }
}

// Face-centre average in fp64 of one accumulator plane at the thread's cell:
// p = the first sample's row, z its z' index, bit a < 3 of avg_bits = average
// the samples first and first + 1 along axis a.  A constant zvec folds away.
template <typename T>
__device__ __forceinline__ double face_avg(const T* __restrict__ p, int sx, int sy, int z, int avg_bits, bool zvec) {
  const int nx = (avg_bits & 1) + 1, ny = ((avg_bits >> 1) & 1) + 1;
  const bool two = (avg_bits >> 2) & 1;
  double s = 0.0;
  for (int ox = 0; ox < nx; ++ox)
    for (int oy = 0; oy < ny; ++oy) face_row<T>(p + (size_t)ox * sx + (size_t)oy * sy, z, two, zvec, s);
  const int cnt = nx * ny * (two ? 2 : 1);
  return s * (1.0 / cnt);  // a power of two: exact
}

// the sum of v over the 64 lanes of the wave, in lane 0 (fixed order)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

}  // namespace mon
