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
// All of it is ONE kernel, k_scene_sample<Q, MESH>: Q the quantity, MESH
// whether the fourth kind is compiled in.  What Q decides is named once, in the
// traits q_averaged, q_damped, q_reads_drude and q_reads_cond, and applied with
// `if constexpr`; a variant that reads no side table, or no mesh tables, gets
// an empty argument in their place and loads none.  The twelve instantiations
// are launched from one table (SCENE_LAUNCH) by the one entry point.
//
// A mesh (MESH) is one more object of the painter's loop: its entry holds its bounding box,
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
// The magnetic pole and the collision frequencies (q_reads_drude) read a side
// table, an object's (gamma_e, omega_m, gamma_m), the same way.  All are sharp.
// A collision frequency (q_damped) paints two values per point, the pole and
// its damping, and reduces to the mean damping of the points whose pole is not
// zero (approximate_drude); an object culled for a wave paints neither.  The
// conductivity (q_reads_cond: a double per object) is painted and averaged by
// the rule of eps (q_averaged), over 0.
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

// What a quantity Q is (layout/scene_file.py sample_args: 0 eps, 1 omega, 2 omega_m, 3 gamma, 4 gamma_m,
// 5 cond), decided here and nowhere else.
constexpr bool q_averaged(int Q) { return Q == 0 || Q == 5; }      // painted and averaged like eps
constexpr bool q_damped(int Q) { return Q == 3 || Q == 4; }        // paints a damping beside the pole
constexpr bool q_reads_drude(int Q) { return 2 <= Q && Q <= 4; }   // reads the SceneDrude side table
constexpr bool q_reads_cond(int Q) { return Q == 5; }              // reads the conductivity side table
enum { SCENE_QUANTITIES = 6 };

// The kernel's side table and mesh tables as typed arguments; a variant that reads none gets SceneNone
// in their place, which nothing loads.
struct SceneNone {};
template <int Q>
using SceneSide = std::conditional_t<q_reads_drude(Q), const SceneDrude* __restrict__,
                                     std::conditional_t<q_reads_cond(Q), const double* __restrict__, SceneNone>>;
template <bool MESH>
using SceneMeshArg = std::conditional_t<MESH, SceneMesh, SceneNone>;

// one point painted with an object at signed distance d: v the value, g the damping beside it
template <int Q>
__device__ __forceinline__ void scene_paint(double d, int flags, double obj, double damp, double& v, double& g) {
#pragma clang fp contract(off)
  const double below = v;
  if (!q_averaged(Q) || (flags & SCENE_SHARP)) {
    v = d < 0.0 ? obj : below;
    if constexpr (q_damped(Q)) g = d < 0.0 ? damp : g;
  } else {
    const double prop = 0.5 - d;
    const double mid = prop * obj + (1.0 - prop) * below;
    const double r = d < -0.5 ? obj : mid;
    v = d > 0.5 ? below : r;
  }
}

template <int Q, bool MESH>
__global__ __launch_bounds__(256) void k_scene_sample(const SceneEnt* __restrict__ tab, SceneSide<Q> side,
                                                      double* __restrict__ out, SceneArgs A, SceneMeshArg<MESH> M) {
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
  double g[2][SCENE_MAX_POINTS];  // the dampings (read only where q_damped)
#pragma unroll
  for (int k = 0; k < SCENE_MAX_POINTS; ++k) g[0][k] = g[1][k] = 0.0;

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
        if (kind == SCENE_BOX || (MESH && kind == SCENE_MESH)) {
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
    // the value a point is painted with (gamma: the electric pole, which decides whether the point is
    // dispersive) and the damping that goes with it
    double obj, damp = 0.0;
    if constexpr (q_reads_drude(Q)) {
      const mon::ConstTab<SceneDrude> D = (mon::ConstTab<SceneDrude>)side;
      obj = Q == 3 ? E[o].omega : D[o].omega_m;
      damp = Q == 3 ? D[o].gamma_e : D[o].gamma_m;
    } else if constexpr (q_reads_cond(Q)) {
      obj = ((mon::ConstTab<double>)side)[o];
    } else {
      obj = Q == 0 ? E[o].eps : E[o].omega;
    }
    if constexpr (MESH) {
      // a mesh: bit 8 j + k of par = the parity of the triangles crossed above point (j, k), dm = the
      // squared distance of the closest one (under linear smoothing)
      const bool is_mesh = kind == SCENE_MESH;
      const bool magnitude = q_averaged(Q) && !(flags & SCENE_SHARP);
      unsigned par = 0u;
      double dm[2][SCENE_MAX_POINTS];
      if (is_mesh) {
#pragma unroll
        for (int k = 0; k < SCENE_MAX_POINTS; ++k) dm[0][k] = dm[1][k] = __builtin_inf();
        const mon::ConstTab<SceneRange> R = (mon::ConstTab<SceneRange>)M.ranges;
        const mon::ConstTab<SceneTri> G = (mon::ConstTab<SceneTri>)M.tris;
        // (the range clamped to the buffer: nothing outside it is ever read)
        const int t0 = min(max(R[o].first, 0), M.ntris), t1 = t0 + min(max(R[o].count, 0), M.ntris - t0);
        for (int t = t0; t < t1; ++t) {
          TriGeom T;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            T.v0[c] = G[t].v[0][c] * A.mod;
            T.v1[c] = G[t].v[1][c] * A.mod;
            T.v2[c] = G[t].v[2][c] * A.mod;
            T.lo[c] = fmin(T.v0[c], fmin(T.v1[c], T.v2[c]));
            T.hi[c] = fmax(T.v0[c], fmax(T.v1[c], T.v2[c]));
          }
          bool hit = true, near = magnitude;
          if (A.flags & SCENE_CULL) {
            hit = T.hi[0] >= wlo[0] && T.lo[0] <= whi[0] && T.hi[1] >= wlo[1] && T.lo[1] <= whi[1] && T.hi[2] >= wlo[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) near = near && !(T.lo[c] - whi[c] > 1.0 || wlo[c] - T.hi[c] > 1.0);
          }
          hit = __builtin_amdgcn_readfirstlane((int)hit) != 0;
          near = __builtin_amdgcn_readfirstlane((int)near) != 0;
          if (!hit && !near) continue;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            T.ab[c] = T.v1[c] - T.v0[c];
            T.ac[c] = T.v2[c] - T.v0[c];
            T.bc[c] = T.v2[c] - T.v1[c];
          }
          T.n[0] = T.ab[1] * T.ac[2] - T.ab[2] * T.ac[1];
          T.n[1] = T.ab[2] * T.ac[0] - T.ab[0] * T.ac[2];
          T.n[2] = T.ab[0] * T.ac[1] - T.ab[1] * T.ac[0];
          if (hit) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
                if (k >= A.npts) continue;
                const double P[3] = {px[k], py[k], pz[j][k]};
                par ^= (unsigned)mesh_crossed(T, P) << (8 * j + k);
              }
          }
          if (near) {
            const double nn = dot3(T.n, T.n);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
                if (k >= A.npts) continue;
                const double P[3] = {px[k], py[k], pz[j][k]};
                const double ds = mesh_dist2(T, nn, P);
                dm[j][k] = ds < dm[j][k] ? ds : dm[j][k];  // (a NaN never lowers it)
              }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
          if (k >= A.npts) continue;
          const double P[3] = {px[k], py[k], pz[j][k]};
          scene_paint<Q>(is_mesh ? mesh_signed(par >> (8 * j + k), magnitude, dm[j][k]) : scene_dist(kind, flags, a, b, P), flags, obj, damp, v[j][k], g[j][k]);
        }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
          if (k >= A.npts) continue;
          const double P[3] = {px[k], py[k], pz[j][k]};
          scene_paint<Q>(scene_dist(kind, flags, a, b, P), flags, obj, damp, v[j][k], g[j][k]);
        }
    }
  }

  double res[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if constexpr (q_averaged(Q)) {
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
    } else if constexpr (!q_damped(Q)) {
      // sqrt(sum(w * w) / n), the sum left to right from 0 (approximate_drude)
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k)
        if (k < A.npts) s = s + v[j][k] * v[j][k];
      res[j] = __dsqrt_rn(s / (double)A.npts);
    } else {
      // sum(g) / count over the dispersive points (pole != 0), both left to right from 0; 0 without one
      double s = 0.0, n = 0.0;
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k)
        if (k < A.npts) {
          s = s + g[j][k];
          n = n + (v[j][k] != 0.0 ? 1.0 : 0.0);
        }
      const double mean = s / (n > 0.0 ? n : 1.0);
      res[j] = n > 0.0 ? mean : 0.0;
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

// the entry point's arguments but the side and mesh tables, checked and turned into SceneArgs;
// 0: launch, -1: nothing to do
int scene_args(const void* tab, int nobj, int quantity, const int* points, int npts, const int* origin,
               const int* shape, const int* stride, double mod, int cull, void* out, SceneArgs& A) {
  if (!tab || !points || !origin || !shape || !stride || !out) return (int)hipErrorInvalidValue;
  if (nobj < 0 || nobj > SCENE_MAX_OBJECTS || quantity < 0 || quantity >= SCENE_QUANTITIES)
    return (int)hipErrorInvalidValue;
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

// the launch of one (quantity, mesh): `side` and `M` go in where the variant reads them
template <int Q, bool MESH>
void scene_launch(const SceneEnt* tab, const void* side, double* out, const SceneArgs& A, const SceneMesh& M,
                  hipStream_t s) {
  SceneSide<Q> S{};
  SceneMeshArg<MESH> G{};
  if constexpr (q_reads_drude(Q) || q_reads_cond(Q)) S = (SceneSide<Q>)side;
  if constexpr (MESH) G = M;
  k_scene_sample<Q, MESH><<<cdiv(A.waves, 4), 256, 0, s>>>(tab, S, out, A, G);
}
constexpr decltype(&scene_launch<0, false>) SCENE_LAUNCH[SCENE_QUANTITIES][2] = {
    {scene_launch<0, false>, scene_launch<0, true>}, {scene_launch<1, false>, scene_launch<1, true>},
    {scene_launch<2, false>, scene_launch<2, true>}, {scene_launch<3, false>, scene_launch<3, true>},
    {scene_launch<4, false>, scene_launch<4, true>}, {scene_launch<5, false>, scene_launch<5, true>}};

}  // namespace

// One component's averaged material of a file scene: `tab` = nobj device entries of fdtd_scene_ent_size()
// bytes (at most fdtd_scene_max_objects()), quantity 0 = eps, 1 = omega, 2 = omega_m, 3 = gamma, 4 = gamma_m,
// 5 = cond, `points` = npts x 3 eps-grid offsets (npts 1, 2, 4 or 8), `origin`, `shape`, `stride` (1 or 2) of
// 3 ints each, `out` = the shape's cells, contiguous fp64.  cull = 0 evaluates every object everywhere.
// `side` = the quantity's side table on the device, one row per object, `side_bytes` its size: none (null,
// 0) for eps and omega, triples (gamma_e, omega_m, gamma_m) of fdtd_scene_drude_size() bytes, rad/s, for
// quantities 2 to 4, doubles (S/m) for cond; a table of another size is refused.
// `ranges` selects the mesh form (kind 3 entries, their bounding boxes in p / q): nobj device pairs (first,
// count) of ints, a mesh's triangles among `tris` = ntris device triangles of fdtd_scene_tri_size() bytes (at
// most fdtd_scene_max_triangles()), every triangle's vertices in ascending (x, y, z) order.  A range is
// clamped to the buffer on the device; the caller checks it on the host.  Without `ranges`: no `tris`, ntris 0.
FDTD_API int fdtd_scene_sample(const void* tab, int nobj, int quantity, const int* points, int npts,
                               const int* origin, const int* shape, const int* stride, double mod, int cull,
                               void* out, void* s, const void* side, size_t side_bytes, const void* tris, int ntris,
                               const void* ranges) {
  const bool mesh = ranges != nullptr;
  if (mesh && (ntris < 0 || ntris > SCENE_MAX_TRIANGLES || (ntris > 0 && !tris))) return (int)hipErrorInvalidValue;
  if (!mesh && (tris || ntris != 0)) return (int)hipErrorInvalidValue;
  SceneArgs A;
  const int rc = scene_args(tab, nobj, quantity, points, npts, origin, shape, stride, mod, cull, out, A);
  if (rc > 0) return rc;
  const size_t row = q_reads_drude(quantity) ? sizeof(SceneDrude) : q_reads_cond(quantity) ? sizeof(double) : 0;
  if ((side != nullptr) != (row != 0) || side_bytes != (size_t)nobj * row) return (int)hipErrorInvalidValue;
  if (rc < 0) return 0;
  const SceneMesh M = {(const SceneTri*)tris, (const SceneRange*)ranges, ntris};
  SCENE_LAUNCH[quantity][mesh]((const SceneEnt*)tab, side, (double*)out, A, M, (hipStream_t)s);
  FDTD_RETURN_LAUNCH_STATUS();
}
FDTD_API int fdtd_scene_drude_size() { return (int)sizeof(SceneDrude); }
FDTD_API int fdtd_scene_ent_size() { return (int)sizeof(SceneEnt); }
FDTD_API int fdtd_scene_max_objects() { return (int)SCENE_MAX_OBJECTS; }
FDTD_API int fdtd_scene_tri_size() { return (int)sizeof(SceneTri); }
FDTD_API int fdtd_scene_max_triangles() { return (int)SCENE_MAX_TRIANGLES; }

