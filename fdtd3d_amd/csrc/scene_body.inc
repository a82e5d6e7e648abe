// The body of k_scene_sample and k_scene_sample_mesh (scene_kernels.hip), included once in each with
// SCENE_WITH_MESH 0 / 1: the kernel's parameters tab, out, A (and M, the mesh tables) are in scope.
// With 0 the preprocessor drops every mesh statement: the kernel of scenes without meshes stays, instruction
// for instruction, what it was before the fourth kind existed.
// SCENE_WITH_DRUDE 1 (k_scene_sample_drude and its mesh twin, Q = 2 omega_m, 3 gamma, 4 gamma_m; the
// parameter drude in scope) compiles in the second table and, for a collision frequency, the damping g painted
// beside the pole v; with 0 the preprocessor drops those statements too, and eps / omega stay what they were.
// SCENE_WITH_COND 1 (k_scene_sample_cond and its mesh twin, Q = 5; the parameter cond in scope, one double per
// object) paints the conductivity by the rule of eps, over 0; with 0 every such test folds away.
#pragma clang fp contract(off)
constexpr bool MESH = SCENE_WITH_MESH;
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
#if SCENE_WITH_DRUDE
  double g[2][SCENE_MAX_POINTS];
#pragma unroll
  for (int k = 0; k < SCENE_MAX_POINTS; ++k) g[0][k] = g[1][k] = 0.0;
  const mon::ConstTab<SceneDrude> D = (mon::ConstTab<SceneDrude>)drude;
#endif

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
#if SCENE_WITH_DRUDE
    // the pole a point is painted with (gamma: the electric one, which decides whether the point is
    // dispersive) and the damping that goes with it
    const double obj = Q == 3 ? E[o].omega : D[o].omega_m;
    const double damp = Q == 3 ? D[o].gamma_e : D[o].gamma_m;
#elif SCENE_WITH_COND
    const double obj = ((mon::ConstTab<double>)cond)[o];
#else
    const double obj = Q == 0 ? E[o].eps : E[o].omega;
#endif
#if SCENE_WITH_MESH
    // a mesh: bit 8 j + k of par = the parity of the triangles crossed above point (j, k), dm = the
    // squared distance of the closest one (under linear smoothing)
    const bool is_mesh = kind == SCENE_MESH;
    const bool magnitude = (Q == 0 || SCENE_WITH_COND) && !(flags & SCENE_SHARP);
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
#endif
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k) {
        if (k >= A.npts) continue;
        const double P[3] = {px[k], py[k], pz[j][k]};
#if SCENE_WITH_MESH
        const double d = is_mesh ? mesh_signed(par >> (8 * j + k), magnitude, dm[j][k])
                                 : scene_dist(kind, flags, a, b, P);
#else
        const double d = scene_dist(kind, flags, a, b, P);
#endif
        const double below = v[j][k];
        if ((Q >= 1 && !SCENE_WITH_COND) || (flags & SCENE_SHARP)) {
          v[j][k] = d < 0.0 ? obj : below;
#if SCENE_WITH_DRUDE
          if (Q >= 3) g[j][k] = d < 0.0 ? damp : g[j][k];
#endif
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
    if (Q == 0 || SCENE_WITH_COND) {
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
    } else if (Q <= 2) {
      // sqrt(sum(w * w) / n), the sum left to right from 0 (approximate_drude)
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < SCENE_MAX_POINTS; ++k)
        if (k < A.npts) s = s + v[j][k] * v[j][k];
      res[j] = __dsqrt_rn(s / (double)A.npts);
    }
#if SCENE_WITH_DRUDE
    else {
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
#endif
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
