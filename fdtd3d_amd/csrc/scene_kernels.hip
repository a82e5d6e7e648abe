// File scenes (layout/scene_file.py): boxes, spheres and cylinders painted
// over vacuum, first to last, evaluated at the material stencil points of one
// field component and reduced to the component's averaged material in ONE
// pass: a thread per two cells along z, no eps-layout grid, no temporaries,
// no LDS, no atomics.  The oracle is ops/torch_ops.py scene_sample: every
// operation here is rounded on its own, in that expression's order (contraction
// off, the round-to-nearest square root), so both give the same bits.
//
// A wave covers a tile of one x plane: 2^zl lanes along z (two cells each),
// 64 >> zl rows along y (zl chosen by the host from the z extent).  The object
// table is read through the constant address space with a wave-uniform index.
// Culling: an object whose bounding box, grown by one cell (the smoothing half
// cell and half a cell of slack against the rounding of the comparison), misses
// the eps-grid points of the wave's tile has d > 0.5 at every one of them,
// which leaves the value below untouched bit for bit; the test is on
// wave-uniform values and broadcast, so the branch is a scalar one.
#include "common.h"
#include "monitor_dev.h"

namespace {

enum { SCENE_BOX = 0, SCENE_SPHERE = 1, SCENE_CYLINDER = 2 };
enum { SCENE_MAX_OBJECTS = 256, SCENE_MAX_POINTS = 8 };
enum { SCENE_IGNORE_SHIFT = 2, SCENE_SHARP = 32 };  // SceneEnt.flags (bits 0-1: the cylinder's axis)
enum { SCENE_CULL = 1, SCENE_VEC = 2 };             // SceneArgs.flags

struct SceneEnt {
  int kind;
  int flags;
  double p[3];  // box lo | sphere centre | cylinder centre, the span's lower end at its axis
  double q[3];  // box hi | radius, -, - | radius, the span's upper end, -
  double eps;
  double omega;  // rad/s
};
static_assert(sizeof(SceneEnt) == 72, "SceneEnt layout (layout/scene_file.py SCENE_ENT)");

struct SceneArgs {
  int n[3];                       // the region
  int stride[3];                  // eps-grid points per cell
  int base[3];                    // stride * origin: the eps index of cell 0, offset 0
  int off[SCENE_MAX_POINTS][3];   // the stencil's offsets
  int omin[3], omax[3];           // their extremes per axis
  int npts, nobj, flags, zl;
  unsigned ty_tiles, tz_tiles, waves;
  double mod;
};

// the signed distance of the point (x, y, z) from an object (already scaled)
__device__ __forceinline__ double scene_dist(int kind, int flags, const double (&a)[3], const double (&b)[3],
                                             const double (&P)[3]) {
#pragma clang fp contract(off)
  const int ign = flags >> SCENE_IGNORE_SHIFT;
  if (kind == SCENE_BOX) {
    double d = -__builtin_inf();
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (!((ign >> c) & 1)) d = fmax(d, fmax(a[c] - P[c], P[c] - b[c]));
    return d;
  }
  if (kind == SCENE_SPHERE) {
    double s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t = P[c] - a[c];
      s[c] = ((ign >> c) & 1) ? 0.0 : t * t;
    }
    return __dsqrt_rn((s[0] + s[1]) + s[2]) - b[0];
  }
  // a cylinder along ax: (b, c) = the two other axes, in x, y, z order
  const int ax = flags & 3;
  const double Pb = ax == 0 ? P[1] : P[0], Pc = ax == 2 ? P[1] : P[2], Pa = ax == 0 ? P[0] : (ax == 1 ? P[1] : P[2]);
  const double ab = ax == 0 ? a[1] : a[0], ac = ax == 2 ? a[1] : a[2], aa = ax == 0 ? a[0] : (ax == 1 ? a[1] : a[2]);
  const double db = Pb - ab, dc = Pc - ac;
  double d = __dsqrt_rn(db * db + dc * dc) - b[0];
  if (!((ign >> ax) & 1)) d = fmax(d, fmax(aa - Pa, Pa - b[1]));
  return d;
}

template <int Q>  // 0: eps, 1: omega
__global__ __launch_bounds__(256) void k_scene_sample(const SceneEnt* __restrict__ tab, double* __restrict__ out,
                                                      SceneArgs A) {
#pragma clang fp contract(off)
  const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (w >= A.waves) return;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned tz = w % A.tz_tiles, t = w / A.tz_tiles;
  const unsigned ty = t % A.ty_tiles;
  const int x = (int)(t / A.ty_tiles);
  const int zlanes = 1 << A.zl, ylanes = 64 >> A.zl;
  const int y0 = (int)ty * ylanes, z0 = (int)tz * 2 * zlanes;
  const int y = y0 + (lane >> A.zl), z = z0 + 2 * (lane & (zlanes - 1));

  // the eps-grid points of the wave's tile, per axis (wave-uniform)
  const int y1 = min(y0 + ylanes, A.n[1]) - 1, z1 = min(z0 + 2 * zlanes, A.n[2]) - 1;
  const int ilo[3] = {x, y0, z0}, ihi[3] = {x, y1, z1};
  double wlo[3], whi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    wlo[c] = (double)(A.base[c] + A.stride[c] * ilo[c] + A.omin[c]) + 0.5;
    whi[c] = (double)(A.base[c] + A.stride[c] * ihi[c] + A.omax[c]) + 0.5;
  }

  // the thread's points: cell j (z + j) x point k
  const int cell[3] = {x, y, z};
  double px[SCENE_MAX_POINTS], py[SCENE_MAX_POINTS], pz[2][SCENE_MAX_POINTS];
#pragma unroll
  for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
    px[k] = (double)(A.base[0] + A.stride[0] * cell[0] + A.off[k][0]) + 0.5;
    py[k] = (double)(A.base[1] + A.stride[1] * cell[1] + A.off[k][1]) + 0.5;
    pz[0][k] = (double)(A.base[2] + A.stride[2] * cell[2] + A.off[k][2]) + 0.5;
    pz[1][k] = (double)(A.base[2] + A.stride[2] * (cell[2] + 1) + A.off[k][2]) + 0.5;
  }
  double v[2][SCENE_MAX_POINTS];
#pragma unroll
  for (int k = 0; k < SCENE_MAX_POINTS; ++k) v[0][k] = v[1][k] = Q == 0 ? 1.0 : 0.0;

  const mon::ConstTab<SceneEnt> E = (mon::ConstTab<SceneEnt>)tab;
  for (int o = 0; o < A.nobj; ++o) {
    const int kind = E[o].kind, flags = E[o].flags;
    const double a[3] = {E[o].p[0] * A.mod, E[o].p[1] * A.mod, E[o].p[2] * A.mod};
    const double b[3] = {E[o].q[0] * A.mod, E[o].q[1] * A.mod, E[o].q[2] * A.mod};
    if (A.flags & SCENE_CULL) {
      // the object's bounding box per axis; an ignored axis never culls
      const int ign = flags >> SCENE_IGNORE_SHIFT, ax = flags & 3;
      bool miss = false;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double lo, hi;
        if (kind == SCENE_BOX) {
          lo = a[c], hi = b[c];
        } else if (kind == SCENE_CYLINDER && c == ax) {
          lo = a[c], hi = b[1];
        } else {
          lo = a[c] - b[0], hi = a[c] + b[0];
        }
        if (!((ign >> c) & 1)) miss = miss || lo - whi[c] > 1.0 || wlo[c] - hi > 1.0;
      }
      if (__builtin_amdgcn_readfirstlane((int)miss)) continue;
    }
    const double obj = Q == 0 ? E[o].eps : E[o].omega;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
        if (k >= A.npts) continue;
        const double P[3] = {px[k], py[k], pz[j][k]};
        const double d = scene_dist(kind, flags, a, b, P);
        const double below = v[j][k];
        if (Q == 1 || (flags & SCENE_SHARP)) {
          v[j][k] = d < 0.0 ? obj : below;
        } else {
          const double prop = 0.5 - d;
          const double mid = prop * obj + (1.0 - prop) * below;
          const double r = d < -0.5 ? obj : mid;
          v[j][k] = d > 0.5 ? below : r;
        }
      }
  }

  double res[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (Q == 0) {
      // the pairwise-hierarchical mean (layout/approximation.py approximate_material)
      double m[SCENE_MAX_POINTS];
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k) m[k] = v[j][k];
#pragma unroll
      for (int step = 1; step < SCENE_MAX_POINTS; step *= 2)
        if (step < A.npts) {
#pragma unroll
          for (int k = 0; k + step < SCENE_MAX_POINTS; k += 2 * step) m[k] = (m[k] + m[k + step]) / 2.0;
        }
      res[j] = m[0];
    } else {
      // sqrt(sum(w * w) / n), the sum left to right from 0 (approximate_drude)
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k)
        if (k < A.npts) s = s + v[j][k] * v[j][k];
      res[j] = __dsqrt_rn(s / (double)A.npts);
    }
  }

  if (y >= A.n[1] || z >= A.n[2]) return;
  double* o = out + ((size_t)x * (size_t)A.n[1] + (size_t)y) * (size_t)A.n[2] + (size_t)z;
  if (z + 1 < A.n[2]) {
    if (A.flags & SCENE_VEC) {
      typedef double D2 __attribute__((ext_vector_type(2)));
      *reinterpret_cast<D2*>(o) = D2{res[0], res[1]};  // even z, even rows, an aligned base: 16 bytes
    } else {
      o[0] = res[0];
      o[1] = res[1];
    }
  } else {
    o[0] = res[0];
  }
}

}  // namespace

// One component's averaged material of a file scene: `tab` = nobj device
// entries of fdtd_scene_ent_size() bytes (at most fdtd_scene_max_objects()),
// quantity 0 = eps / 1 = omega, `points` = npts x 3 eps-grid offsets (npts 1, 2,
// 4 or 8), `origin`, `shape`, `stride` (1 or 2) of 3 ints each, `out` = the
// shape's cells, contiguous fp64.  cull = 0 evaluates every object everywhere.
FDTD_API int fdtd_scene_sample(const void* tab, int nobj, int quantity, const int* points, int npts,
                               const int* origin, const int* shape, const int* stride, double mod, int cull,
                               void* out, void* s) {
  if (!tab || !points || !origin || !shape || !stride || !out) return (int)hipErrorInvalidValue;
  if (nobj < 0 || nobj > SCENE_MAX_OBJECTS || (quantity != 0 && quantity != 1)) return (int)hipErrorInvalidValue;
  if (npts != 1 && npts != 2 && npts != 4 && npts != 8) return (int)hipErrorInvalidValue;
  if (mod != 1.0 && mod != 2.0) return (int)hipErrorInvalidValue;
  SceneArgs A = {};
  for (int c = 0; c < 3; ++c) {
    if (shape[c] < 0 || (stride[c] != 1 && stride[c] != 2)) return (int)hipErrorInvalidValue;
    const long long reach = 2LL * ((long long)std::llabs((long long)origin[c]) + shape[c]);
    if (reach >= (1LL << 30)) return (int)hipErrorInvalidValue;  // eps indices stay far inside int
    A.n[c] = shape[c];
    A.stride[c] = stride[c];
    A.base[c] = stride[c] * origin[c];
    A.omin[c] = A.omax[c] = points[c];
  }
  for (int k = 0; k < SCENE_MAX_POINTS; ++k)
    for (int c = 0; c < 3; ++c) {
      const int v = points[3 * (k < npts ? k : 0) + c];
      if (v < -(1 << 20) || v > (1 << 20)) return (int)hipErrorInvalidValue;
      A.off[k][c] = v;
      A.omin[c] = v < A.omin[c] ? v : A.omin[c];
      A.omax[c] = v > A.omax[c] ? v : A.omax[c];
    }
  if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return 0;
  // lanes along z: the smallest power of two covering the row's cell pairs, at most the wave
  int zl = 0;
  while (zl < 6 && (2 << zl) < shape[2]) ++zl;
  const long long ty = cdiv(shape[1], 64 >> zl), tz = cdiv(shape[2], 2 << zl);
  const long long waves = (long long)shape[0] * ty * tz;
  if (waves >= (1LL << 31)) return (int)hipErrorInvalidValue;
  A.npts = npts;
  A.nobj = nobj;
  A.zl = zl;
  A.ty_tiles = (unsigned)ty;
  A.tz_tiles = (unsigned)tz;
  A.waves = (unsigned)waves;
  A.mod = mod;
  A.flags = (cull ? SCENE_CULL : 0) | ((shape[2] % 2 == 0 && ((uintptr_t)out & 15) == 0) ? SCENE_VEC : 0);
  const unsigned blocks = cdiv(waves, 4);
  if (quantity == 0)
    k_scene_sample<0><<<blocks, 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (double*)out, A);
  else
    k_scene_sample<1><<<blocks, 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (double*)out, A);
  FDTD_RETURN_LAUNCH_STATUS();
}
FDTD_API int fdtd_scene_ent_size() { return (int)sizeof(SceneEnt); }
FDTD_API int fdtd_scene_max_objects() { return (int)SCENE_MAX_OBJECTS; }
