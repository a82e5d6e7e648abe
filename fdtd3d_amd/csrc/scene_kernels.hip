// File scenes (layout/scene_file.py): boxes, spheres, cylinders and closed
// triangle meshes painted
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
//
// A mesh (k_scene_sample_mesh, the same body with the fourth kind compiled in)
// is one more object of the painter's loop: its entry holds its bounding box,
// a second table its range of the triangle buffer, which is read like the
// object table, one triangle per trip of every wave.  Sign: the parity of the
// triangles a ray along +z crosses (mesh_crossed); magnitude: the distance to
// the closest triangle (mesh_dist2), evaluated only under linear smoothing.
// Per-wave culling: a triangle takes part in the parity only if its box meets
// the wave's columns in x and y and does not end below the wave's lowest point
// -- mesh_crossed tests the same box per point, so leaving it out changes
// nothing -- and in the distance only if its box grown by one cell meets the
// tile: the others lie farther than a cell from every point, which can move a
// distance only where it stays beyond 0.5 and the painting rule does not read it.
//
// The magnetic pole and the collision frequencies (k_scene_sample_drude and its
// mesh twin, the same body once more) read a second table, an object's
// (gamma_e, omega_m, gamma_m), the same way.  All are sharp.  A collision
// frequency paints two values per point, the pole and its damping, and reduces
// to the mean damping of the points whose pole is not zero (approximate_drude);
// an object culled for a wave paints neither.
#include "common.h"
#include "monitor_dev.h"

namespace {

enum { SCENE_BOX = 0, SCENE_SPHERE = 1, SCENE_CYLINDER = 2, SCENE_MESH = 3 };
enum { SCENE_MAX_OBJECTS = 256, SCENE_MAX_POINTS = 8, SCENE_MAX_TRIANGLES = 1 << 20 };
enum { SCENE_IGNORE_SHIFT = 2, SCENE_SHARP = 32 };  // SceneEnt.flags (bits 0-1: the cylinder's axis)
enum { SCENE_CULL = 1, SCENE_VEC = 2 };             // SceneArgs.flags

struct SceneEnt {
  int kind;
  int flags;
  double p[3];  // box, mesh lo | sphere centre | cylinder centre, the span's lower end at its axis
  double q[3];  // box, mesh hi | radius, -, - | radius, the span's upper end, -
  double eps;
  double omega;  // rad/s
};
static_assert(sizeof(SceneEnt) == 72, "SceneEnt layout (layout/scene_file.py SCENE_ENT)");

// what travels beside an entry (layout/scene_file.py SceneTable.drude), rad/s
struct SceneDrude {
  double gamma_e, omega_m, gamma_m;
};
static_assert(sizeof(SceneDrude) == 24, "SceneDrude layout (layout/scene_file.py SceneTable.drude)");

// a triangle: its vertices in ascending (x, y, z) order (layout/scene_file.py Mesh)
struct SceneTri {
  double v[3][3];
};
struct SceneRange {  // a mesh's triangles: first, first + 1, ... first + count - 1
  int first, count;
};
struct SceneMesh {
  const SceneTri* tris;
  const SceneRange* ranges;  // one per object
  int ntris;
};

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

// A triangle as both mesh functions read it (wave-uniform): its vertices v0 <=
// v1 <= v2, the edges ab = v1 - v0, ac = v2 - v0, bc = v2 - v1, the normal
// n = ab x ac (n[2] is twice the signed projected area), its bounding box.
struct TriGeom {
  double v0[3], v1[3], v2[3], ab[3], ac[3], bc[3], n[3], lo[3], hi[3];
};

__device__ __forceinline__ double dot3(const double (&u)[3], const double (&w)[3]) {
#pragma clang fp contract(off)
  return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
}

// Does the ray from P along +z cross the triangle?  P lies in the projected
// triangle when it is on the inner side of the three edge functions, each taken
// from the edge's lower vertex to its higher one -- the two triangles of an
// edge evaluate one expression -- with e >= 0 counting as left of the edge for
// both (the ray displaced by (-e^2, +e)); then the plane decides.
__device__ __forceinline__ bool mesh_crossed(const TriGeom& T, const double (&P)[3]) {
#pragma clang fp contract(off)
  const double ap[3] = {P[0] - T.v0[0], P[1] - T.v0[1], P[2] - T.v0[2]};
  const double bpx = P[0] - T.v1[0], bpy = P[1] - T.v1[1];
  const bool l01 = T.ab[0] * ap[1] - T.ab[1] * ap[0] >= 0.0;
  const bool l02 = T.ac[0] * ap[1] - T.ac[1] * ap[0] >= 0.0;
  const bool l12 = T.bc[0] * bpy - T.bc[1] * bpx >= 0.0;
  const bool up = T.n[2] > 0.0, down = T.n[2] < 0.0;
  const bool inside = (up & l01 & l12 & !l02) | (down & !l01 & !l12 & l02);
  const bool box = (P[0] >= T.lo[0]) & (P[0] <= T.hi[0]) & (P[1] >= T.lo[1]) & (P[1] <= T.hi[1]) & (P[2] <= T.hi[2]);
  const double tt = dot3(T.n, ap);
  return inside & box & ((up & (tt < 0.0)) | (down & (tt > 0.0)));
}

// The squared distance of P from the closest point of the triangle, by the
// region of that point: the face (the plane's distance), an edge or a vertex.
// The conditions are those of the usual if-chain (v0, v1, edge v0v1, v2, edge
// v0v2, edge v1v2, face), applied last to first so the first that holds wins.
__device__ __forceinline__ double mesh_dist2(const TriGeom& T, double nn, const double (&P)[3]) {
#pragma clang fp contract(off)
  double ap[3], bp[3], cp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ap[c] = P[c] - T.v0[c];
    bp[c] = P[c] - T.v1[c];
    cp[c] = P[c] - T.v2[c];
  }
  const double d1 = dot3(T.ab, ap), d2 = dot3(T.ac, ap), d3 = dot3(T.ab, bp), d4 = dot3(T.ac, bp);
  const double d5 = dot3(T.ab, cp), d6 = dot3(T.ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double d43 = d4 - d3, d56 = d5 - d6;
  const double tt = dot3(T.n, ap);
  double num = tt * tt, den = nn, r[3] = {ap[0], ap[1], ap[2]}, e[3] = {T.ab[0], T.ab[1], T.ab[2]};
  bool face = true;
#define SCENE_REGION(cond, N, D, R, E)   \
  {                                      \
    const bool c_ = (cond);              \
    num = c_ ? (N) : num;                \
    den = c_ ? (D) : den;                \
    face = face & !c_;                   \
    _Pragma("unroll") for (int c = 0; c < 3; ++c) { \
      r[c] = c_ ? (R)[c] : r[c];         \
      e[c] = c_ ? (E)[c] : e[c];         \
    }                                    \
  }
  SCENE_REGION((va <= 0.0) & (d43 >= 0.0) & (d56 >= 0.0), d43, d43 + d56, bp, T.bc)
  SCENE_REGION((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), d2, d2 - d6, ap, T.ac)
  SCENE_REGION((d6 >= 0.0) & (d5 <= d6), 0.0, 1.0, cp, T.ac)
  SCENE_REGION((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), d1, d1 - d3, ap, T.ab)
  SCENE_REGION((d3 >= 0.0) & (d4 <= d3), 0.0, 1.0, bp, T.ab)
  SCENE_REGION((d1 <= 0.0) & (d2 <= 0.0), 0.0, 1.0, ap, T.ab)
#undef SCENE_REGION
  const double x = num / den;
  const double q[3] = {r[0] - x * e[0], r[1] - x * e[1], r[2] - x * e[2]};
  return face ? x : dot3(q, q);
}

// a mesh's signed distance from the parity bit and the squared distance (+-1 where only the sign is read)
__device__ __forceinline__ double mesh_signed(unsigned parity, bool magnitude, double dist2) {
  const double far = magnitude ? __dsqrt_rn(dist2) : 1.0;
  return (parity & 1u) ? -far : far;
}

template <int Q>  // 0: eps, 1: omega
__global__ __launch_bounds__(256) void k_scene_sample(const SceneEnt* __restrict__ tab, double* __restrict__ out,
                                                      SceneArgs A) {
#define SCENE_WITH_MESH 0
#define SCENE_WITH_DRUDE 0
#define SCENE_WITH_COND 0
#include "scene_body.inc"
#undef SCENE_WITH_COND
#undef SCENE_WITH_DRUDE
#undef SCENE_WITH_MESH
}

template <int Q>
__global__ __launch_bounds__(256) void k_scene_sample_mesh(const SceneEnt* __restrict__ tab,
                                                           double* __restrict__ out, SceneArgs A, SceneMesh M) {
#define SCENE_WITH_MESH 1
#define SCENE_WITH_DRUDE 0
#define SCENE_WITH_COND 0
#include "scene_body.inc"
#undef SCENE_WITH_COND
#undef SCENE_WITH_DRUDE
#undef SCENE_WITH_MESH
}

template <int Q>  // 2: omega_m, 3: gamma, 4: gamma_m
__global__ __launch_bounds__(256) void k_scene_sample_drude(const SceneEnt* __restrict__ tab,
                                                            const SceneDrude* __restrict__ drude,
                                                            double* __restrict__ out, SceneArgs A) {
#define SCENE_WITH_MESH 0
#define SCENE_WITH_DRUDE 1
#define SCENE_WITH_COND 0
#include "scene_body.inc"
#undef SCENE_WITH_COND
#undef SCENE_WITH_DRUDE
#undef SCENE_WITH_MESH
}

template <int Q>
__global__ __launch_bounds__(256) void k_scene_sample_drude_mesh(const SceneEnt* __restrict__ tab,
                                                                 const SceneDrude* __restrict__ drude,
                                                                 double* __restrict__ out, SceneArgs A, SceneMesh M) {
#define SCENE_WITH_MESH 1
#define SCENE_WITH_DRUDE 1
#define SCENE_WITH_COND 0
#include "scene_body.inc"
#undef SCENE_WITH_COND
#undef SCENE_WITH_DRUDE
#undef SCENE_WITH_MESH
}

template <int Q>  // 5: cond
__global__ __launch_bounds__(256) void k_scene_sample_cond(const SceneEnt* __restrict__ tab,
                                                           const double* __restrict__ cond,
                                                           double* __restrict__ out, SceneArgs A) {
#define SCENE_WITH_MESH 0
#define SCENE_WITH_DRUDE 0
#define SCENE_WITH_COND 1
#include "scene_body.inc"
#undef SCENE_WITH_COND
#undef SCENE_WITH_DRUDE
#undef SCENE_WITH_MESH
}

template <int Q>
__global__ __launch_bounds__(256) void k_scene_sample_cond_mesh(const SceneEnt* __restrict__ tab,
                                                                const double* __restrict__ cond,
                                                                double* __restrict__ out, SceneArgs A, SceneMesh M) {
#define SCENE_WITH_MESH 1
#define SCENE_WITH_DRUDE 0
#define SCENE_WITH_COND 1
#include "scene_body.inc"
#undef SCENE_WITH_COND
#undef SCENE_WITH_DRUDE
#undef SCENE_WITH_MESH
}

// the arguments the entry points share (quantity one of qlo .. qhi), checked and turned into SceneArgs;
// 0: launch, -1: nothing to do
int scene_args(const void* tab, int nobj, int quantity, int qlo, int qhi, const int* points, int npts,
               const int* origin, const int* shape, const int* stride, double mod, int cull, void* out, SceneArgs& A) {

  if (!tab || !points || !origin || !shape || !stride || !out) return (int)hipErrorInvalidValue;
  if (nobj < 0 || nobj > SCENE_MAX_OBJECTS || quantity < qlo || quantity > qhi) return (int)hipErrorInvalidValue;
  if (npts != 1 && npts != 2 && npts != 4 && npts != 8) return (int)hipErrorInvalidValue;
  if (mod != 1.0 && mod != 2.0) return (int)hipErrorInvalidValue;
  A = SceneArgs{};
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
  if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return -1;
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
  return 0;
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
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, 0, 1, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc) return rc < 0 ? 0 : rc;
  const unsigned blocks = cdiv(A.waves, 4);
  if (quantity == 0)
    k_scene_sample<0><<<blocks, 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (double*)out, A);
  else
    k_scene_sample<1><<<blocks, 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (double*)out, A);
  FDTD_RETURN_LAUNCH_STATUS();
}

// The same for a scene with meshes (kind 3 entries, their bounding boxes in p / q): `tris` = ntris
// device triangles of fdtd_scene_tri_size() bytes (at most fdtd_scene_max_triangles()), every triangle's
// vertices in ascending (x, y, z) order; `ranges` = nobj device pairs (first, count) of ints, a mesh's
// triangles.  A range is clamped to the buffer on the device; the caller checks it on the host.
FDTD_API int fdtd_scene_sample_mesh(const void* tab, int nobj, int quantity, const int* points, int npts,
                                    const int* origin, const int* shape, const int* stride, double mod, int cull,
                                    void* out, void* s, const void* tris, int ntris, const void* ranges) {
  if (ntris < 0 || ntris > SCENE_MAX_TRIANGLES || (ntris > 0 && !tris) || !ranges) return (int)hipErrorInvalidValue;
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, 0, 1, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc) return rc < 0 ? 0 : rc;
  const SceneMesh M = {(const SceneTri*)tris, (const SceneRange*)ranges, ntris};
  const unsigned blocks = cdiv(A.waves, 4);
  if (quantity == 0)
    k_scene_sample_mesh<0><<<blocks, 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (double*)out, A, M);
  else
    k_scene_sample_mesh<1><<<blocks, 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (double*)out, A, M);
  FDTD_RETURN_LAUNCH_STATUS();
}

// The magnetic plasma frequency and the collision frequencies: quantity 2 = omega_m, 3 = gamma, 4 =
// gamma_m, `drude` = ndrude device triples (gamma_e, omega_m, gamma_m) of doubles, one per object
// (ndrude == nobj); everything else as fdtd_scene_sample.
FDTD_API int fdtd_scene_sample_drude(const void* tab, int nobj, int quantity, const int* points, int npts,
                                     const int* origin, const int* shape, const int* stride, double mod, int cull,
                                     void* out, void* s, const void* drude, int ndrude) {
  if (!drude || ndrude != nobj) return (int)hipErrorInvalidValue;
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, 2, 4, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc) return rc < 0 ? 0 : rc;
  const unsigned blocks = cdiv(A.waves, 4);
  const SceneEnt* T = (const SceneEnt*)tab;
  const SceneDrude* D = (const SceneDrude*)drude;
  if (quantity == 2)
    k_scene_sample_drude<2><<<blocks, 256, 0, (hipStream_t)s>>>(T, D, (double*)out, A);
  else if (quantity == 3)
    k_scene_sample_drude<3><<<blocks, 256, 0, (hipStream_t)s>>>(T, D, (double*)out, A);
  else
    k_scene_sample_drude<4><<<blocks, 256, 0, (hipStream_t)s>>>(T, D, (double*)out, A);
  FDTD_RETURN_LAUNCH_STATUS();
}

// The same for a scene with meshes: `tris`, `ntris`, `ranges` as fdtd_scene_sample_mesh.
FDTD_API int fdtd_scene_sample_drude_mesh(const void* tab, int nobj, int quantity, const int* points, int npts,
                                          const int* origin, const int* shape, const int* stride, double mod,
                                          int cull, void* out, void* s, const void* drude, int ndrude,
                                          const void* tris, int ntris, const void* ranges) {
  if (!drude || ndrude != nobj) return (int)hipErrorInvalidValue;
  if (ntris < 0 || ntris > SCENE_MAX_TRIANGLES || (ntris > 0 && !tris) || !ranges) return (int)hipErrorInvalidValue;
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, 2, 4, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc) return rc < 0 ? 0 : rc;
  const SceneMesh M = {(const SceneTri*)tris, (const SceneRange*)ranges, ntris};
  const unsigned blocks = cdiv(A.waves, 4);
  const SceneEnt* T = (const SceneEnt*)tab;
  const SceneDrude* D = (const SceneDrude*)drude;
  if (quantity == 2)
    k_scene_sample_drude_mesh<2><<<blocks, 256, 0, (hipStream_t)s>>>(T, D, (double*)out, A, M);
  else if (quantity == 3)
    k_scene_sample_drude_mesh<3><<<blocks, 256, 0, (hipStream_t)s>>>(T, D, (double*)out, A, M);
  else
    k_scene_sample_drude_mesh<4><<<blocks, 256, 0, (hipStream_t)s>>>(T, D, (double*)out, A, M);
  FDTD_RETURN_LAUNCH_STATUS();
}
// The conductivity: quantity 5, `cond` = ncond device doubles, one per object (ncond == nobj, S/m);
// everything else as fdtd_scene_sample.
FDTD_API int fdtd_scene_sample_cond(const void* tab, int nobj, int quantity, const int* points, int npts,
                                    const int* origin, const int* shape, const int* stride, double mod, int cull,
                                    void* out, void* s, const void* cond, int ncond) {
  if (!cond || ncond != nobj) return (int)hipErrorInvalidValue;
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, 5, 5, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc) return rc < 0 ? 0 : rc;
  k_scene_sample_cond<5><<<cdiv(A.waves, 4), 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab, (const double*)cond,
                                                                       (double*)out, A);
  FDTD_RETURN_LAUNCH_STATUS();
}

// The same for a scene with meshes: `tris`, `ntris`, `ranges` as fdtd_scene_sample_mesh.
FDTD_API int fdtd_scene_sample_cond_mesh(const void* tab, int nobj, int quantity, const int* points, int npts,
                                         const int* origin, const int* shape, const int* stride, double mod,
                                         int cull, void* out, void* s, const void* cond, int ncond,
                                         const void* tris, int ntris, const void* ranges) {
  if (!cond || ncond != nobj) return (int)hipErrorInvalidValue;
  if (ntris < 0 || ntris > SCENE_MAX_TRIANGLES || (ntris > 0 && !tris) || !ranges) return (int)hipErrorInvalidValue;
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, 5, 5, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc) return rc < 0 ? 0 : rc;
  const SceneMesh M = {(const SceneTri*)tris, (const SceneRange*)ranges, ntris};
  k_scene_sample_cond_mesh<5><<<cdiv(A.waves, 4), 256, 0, (hipStream_t)s>>>((const SceneEnt*)tab,
                                                                            (const double*)cond, (double*)out, A, M);
  FDTD_RETURN_LAUNCH_STATUS();
}
FDTD_API int fdtd_scene_drude_size() { return (int)sizeof(SceneDrude); }
FDTD_API int fdtd_scene_ent_size() { return (int)sizeof(SceneEnt); }
FDTD_API int fdtd_scene_max_objects() { return (int)SCENE_MAX_OBJECTS; }
FDTD_API int fdtd_scene_tri_size() { return (int)sizeof(SceneTri); }
FDTD_API int fdtd_scene_max_triangles() { return (int)SCENE_MAX_TRIANGLES; }
