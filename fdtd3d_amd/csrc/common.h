// Shared definitions for the fdtd3d-amd HIP kernels (gfx950 / MI355X).
//
// Layout convention (same as the reference Grid, Source/Grid/Grid.cpp:127-139):
// a field of local shape (nx, ny, nz) is one contiguous array, z fastest,
// linear index  i*ny*nz + j*nz + k.  All kernels take boxes in LOCAL indices;
// the Python/C++ host code maps global computation ranges to local boxes.
#pragma once

#include <cstdlib>
#include <type_traits>

#include <hip/hip_runtime.h>
#include <stdint.h>

#define FDTD_API extern "C" __attribute__((visibility("default")))

struct Box3 {
  int lo[3];
  int hi[3];
};

__device__ __forceinline__ bool in_box(const Box3& b, int i, int j, int k) {
  return i >= b.lo[0] && i < b.hi[0] && j >= b.lo[1] && j < b.hi[1] && k >= b.lo[2] && k < b.hi[2];
}

__host__ __device__ static inline bool box_empty(const Box3& b) {
  return b.hi[0] <= b.lo[0] || b.hi[1] <= b.lo[1] || b.hi[2] <= b.lo[2];
}

__host__ __device__ static inline Box3 box_union(const Box3& a, const Box3& b) {
  if (box_empty(a)) return b;
  if (box_empty(b)) return a;
  Box3 r;
  for (int d = 0; d < 3; ++d) {
    r.lo[d] = a.lo[d] < b.lo[d] ? a.lo[d] : b.lo[d];
    r.hi[d] = a.hi[d] > b.hi[d] ? a.hi[d] : b.hi[d];
  }
  return r;
}

static inline Box3 make_box(const int* lohi) {
  Box3 b;
  for (int d = 0; d < 3; ++d) {
    b.lo[d] = lohi[d];
    b.hi[d] = lohi[3 + d];
  }
  return b;
}

static inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

// What every blocked 3D entry point reads first (yee3d_tb.hip, yee3d_tb64.hip):
// the six update boxes (Ex Ey Ez Hx Hy Hz), the output box and the hard
// source's value at each of the `steps` levels (SV = TbSrc / TbSrc64; all 0
// without a source, src[3] < 0).  False: the output box is empty, nothing to
// launch.
template <typename SV>
struct TbPass {
  Box3 b[6];
  Box3 O;
  SV sv;
};
template <typename SV>
static inline bool tb_pass(TbPass<SV>& p, const int* boxes, const int* obox, int steps, const int* src,
                           const double* src_vals) {
  for (int n = 0; n < 6; ++n) p.b[n] = make_box(boxes + 6 * n);
  p.O = make_box(obox);
  typedef typename std::remove_reference<decltype(p.sv.v[0])>::type R;
  for (int l = 0; l < 8; ++l) p.sv.v[l] = (src[3] >= 0 && l < steps) ? (R)src_vals[l] : (R)0;
  return !box_empty(p.O);
}

// x planes per workgroup of the x-streaming split kernels: 16 (measured best
// on full grids), halved while the launch would hold fewer than 2048
// workgroups -- thin shell / slab windows (hybrid blocking, PML slabs) would
// otherwise leave most CUs idle.  `wg_per_chunk` = workgroups per x chunk.
// x planes per workgroup of the split (per-step) kernels: halve from `base`
// until the launch has FDTD3D_SPLIT_WGS workgroups (default 2048), not below
// FDTD3D_SPLIT_MINXC planes (default 2) -- read once per library at first use
static inline int split_param(int which) {
  static const int wgs = [] {
    const char* e = getenv("FDTD3D_SPLIT_WGS");
    return e && atoi(e) > 0 ? atoi(e) : 2048;
  }();
  static const int mxc = [] {
    const char* e = getenv("FDTD3D_SPLIT_MINXC");
    return e && atoi(e) > 0 ? atoi(e) : 2;
  }();
  return which ? mxc : wgs;
}

static inline int split_xchunk(int nxo, long long wg_per_chunk, int req, int base = 16, int min_xc = 0) {
  if (req > 0) return req;
  if (min_xc <= 0) min_xc = split_param(1);
  const long long target = split_param(0);
  int xc = base;
  while (xc > min_xc && wg_per_chunk * (long long)cdiv(nxo, xc) < target) xc /= 2;
  return xc;
}

#define FDTD_RETURN_LAUNCH_STATUS() return (int)hipGetLastError()
