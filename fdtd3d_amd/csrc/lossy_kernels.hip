// The conductive E update of a lossy medium (scene-file key `sigma`):
//
//   E_new = ca * E + cb * curl(H)
//
// on the lossy box only -- the one update of the solver whose old field has a
// factor.  The plain, fused and blocked kernels keep `dst += cb * curl` and
// run everywhere else; the scheme cuts the box out of their windows
// (models/scheme.py _update), so this launch runs beside theirs on the shell
// streams.
//
// One launch updates Ex, Ey and Ez of a half step.  (ca, cb) are stored
// box-local, one pair per cell and component, over one storage box R shared by
// the three components (models/regions.py LossyCoefs).  Lanes run along z and
// own V consecutive cells: 16 bytes (V = 4 fp32, 2 fp64) when the rows of the
// fields and of R are whole lanes and R starts on one, so that a field lane
// and its coefficient lane are both aligned; one cell otherwise.  A thread is
// one lane of one (x, y) row: the boxes are small next to the grid, so the
// x - 1 plane is re-read through the cache instead of carried in registers.
//
// Every operand of a thread is loaded before its first store, and a thread
// stores only the cells its masks hold: a lane cut by a z border writes its
// own elements one by one, never the neighbour's (the launches of the plain
// windows next to the box are in flight at the same time).
#include "common.h"

namespace {

template <typename T, int V>
struct alignas(sizeof(T) * V) Lane {
  T v[V];
};

template <typename T, int V>
__device__ __forceinline__ Lane<T, V> ld(const T* p, size_t off) {
  return *reinterpret_cast<const Lane<T, V>*>(p + off);
}

// bit q: cell (i, j, kb + q) lies in b
template <int V>
__device__ __forceinline__ unsigned lane_mask(const Box3& b, int i, int j, int kb) {
  if (i < b.lo[0] || i >= b.hi[0] || j < b.lo[1] || j >= b.hi[1]) return 0u;
  unsigned m = 0u;
#pragma unroll
  for (int q = 0; q < V; ++q) m |= (kb + q >= b.lo[2] && kb + q < b.hi[2]) ? (1u << q) : 0u;
  return m;
}

template <typename T, int V>
__device__ __forceinline__ void st_masked(T* p, size_t off, const Lane<T, V>& e, unsigned m) {
  if constexpr (V > 1) {
    if (m == (1u << V) - 1u) {
      // a whole lane: one 16-byte store
      typedef T VT __attribute__((ext_vector_type(V)));
      VT w;
#pragma unroll
      for (int q = 0; q < V; ++q) w[q] = e.v[q];
      *reinterpret_cast<VT*>(p + off) = w;
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < V; ++q)
    if (m & (1u << q)) p[off + q] = e.v[q];
}

struct LossyArgs {
  Box3 bx, by, bz;  // update boxes of Ex, Ey, Ez (local indices)
  Box3 U;           // their union
  Box3 R;           // storage box of the coefficients
  int ny, nz;       // field rows
  int zshift;       // log2 of the lanes per z row of a workgroup
};

template <typename T, int V>
__global__ __launch_bounds__(256) void k_lossy_e(T* __restrict__ ex, T* __restrict__ ey, T* __restrict__ ez,
                                                 const T* __restrict__ hx, const T* __restrict__ hy,
                                                 const T* __restrict__ hz, const T* __restrict__ cax,
                                                 const T* __restrict__ cay, const T* __restrict__ caz,
                                                 const T* __restrict__ cbx, const T* __restrict__ cby,
                                                 const T* __restrict__ cbz, LossyArgs A) {
  typedef Lane<T, V> L;
  const int lz = 1 << A.zshift;
  const int zl = (int)threadIdx.x & (lz - 1);
  const int kb = (A.U.lo[2] & ~(V - 1)) + V * ((int)blockIdx.x * lz + zl);
  const int j = A.U.lo[1] + (int)blockIdx.y * (256 >> A.zshift) + ((int)threadIdx.x >> A.zshift);
  const int i = A.U.lo[0] + (int)blockIdx.z;
  if (kb >= A.U.hi[2] || j >= A.U.hi[1]) return;
  const unsigned mx = lane_mask<V>(A.bx, i, j, kb);
  const unsigned my = lane_mask<V>(A.by, i, j, kb);
  const unsigned mz = lane_mask<V>(A.bz, i, j, kb);
  if (!(mx | my | mz)) return;

  const size_t plane = (size_t)A.ny * (size_t)A.nz;
  const size_t off = (size_t)i * plane + (size_t)j * (size_t)A.nz + (size_t)kb;
  const int rny = A.R.hi[1] - A.R.lo[1], rnz = A.R.hi[2] - A.R.lo[2];
  const size_t roff =
      ((size_t)(i - A.R.lo[0]) * (size_t)rny + (size_t)(j - A.R.lo[1])) * (size_t)rnz + (size_t)(kb - A.R.lo[2]);

  // ---- loads: a whole lane lies inside its row (host: rows are whole lanes, or V = 1); the j - 1 row, the
  // i - 1 plane and the k - 1 cell are read only by the components whose boxes the host checked for them
  const L z = {};
  const L hxc = ld<T, V>(hx, off), hyc = ld<T, V>(hy, off), hzc = ld<T, V>(hz, off);
  L hz_j = z, hx_j = z, hz_i = z, hy_i = z;
  T hy_k = (T)0, hx_k = (T)0;
  if (mx) hz_j = ld<T, V>(hz, off - (size_t)A.nz);
  if (mz) hx_j = ld<T, V>(hx, off - (size_t)A.nz);
  if (my) hz_i = ld<T, V>(hz, off - plane);
  if (mz) hy_i = ld<T, V>(hy, off - plane);
  if ((mx & 1u) && kb > 0) hy_k = hy[off - 1];
  if ((my & 1u) && kb > 0) hx_k = hx[off - 1];
  L e_x = z, e_y = z, e_z = z, a_x = z, a_y = z, a_z = z, b_x = z, b_y = z, b_z = z;
  if (mx) e_x = ld<T, V>(ex, off), a_x = ld<T, V>(cax, roff), b_x = ld<T, V>(cbx, roff);
  if (my) e_y = ld<T, V>(ey, off), a_y = ld<T, V>(cay, roff), b_y = ld<T, V>(cby, roff);
  if (mz) e_z = ld<T, V>(ez, off), a_z = ld<T, V>(caz, roff), b_z = ld<T, V>(cbz, roff);

  // ---- the curl of layout/yee.py CURL_TERMS, term for term as the plain kernels take it
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const T hym = q == 0 ? hy_k : hyc.v[q > 0 ? q - 1 : 0];
    const T hxm = q == 0 ? hx_k : hxc.v[q > 0 ? q - 1 : 0];
    e_x.v[q] = a_x.v[q] * e_x.v[q] + b_x.v[q] * ((hzc.v[q] - hz_j.v[q]) - (hyc.v[q] - hym));
    e_y.v[q] = a_y.v[q] * e_y.v[q] + b_y.v[q] * ((hxc.v[q] - hxm) - (hzc.v[q] - hz_i.v[q]));
    e_z.v[q] = a_z.v[q] * e_z.v[q] + b_z.v[q] * ((hyc.v[q] - hy_i.v[q]) - (hxc.v[q] - hx_j.v[q]));
  }

  // ---- stores: own cells only
  if (mx) st_masked<T, V>(ex, off, e_x, mx);
  if (my) st_masked<T, V>(ey, off, e_y, my);
  if (mz) st_masked<T, V>(ez, off, e_z, mz);
}

inline bool inside(const Box3& b, const Box3& o) {
  for (int d = 0; d < 3; ++d)
    if (b.lo[d] < o.lo[d] || b.hi[d] > o.hi[d]) return false;
  return true;
}

template <typename T>
int lossy_e(void* const* e, const void* const* h, const void* const* ca, const void* const* cb, int nx, int ny,
            int nz, const int* boxes, const int* rbox, hipStream_t s, int* lanes_out) {
  if (!e || !h || !ca || !cb || !boxes || !rbox || nx <= 0 || ny <= 0 || nz <= 0) return (int)hipErrorInvalidValue;
  for (int c = 0; c < 3; ++c)
    if (!e[c] || !h[c] || !ca[c] || !cb[c]) return (int)hipErrorInvalidValue;
  LossyArgs A;
  A.bx = make_box(boxes), A.by = make_box(boxes + 6), A.bz = make_box(boxes + 12);
  A.R = make_box(rbox);
  const Box3 arr = {{0, 0, 0}, {nx, ny, nz}};
  // the axes a component's curl reads at index - 1 (layout/yee.py CURL_TERMS)
  const int back[3][2] = {{1, 2}, {0, 2}, {0, 1}};
  Box3* b[3] = {&A.bx, &A.by, &A.bz};
  Box3 U = {{0, 0, 0}, {0, 0, 0}};
  for (int c = 0; c < 3; ++c) {
    if (box_empty(*b[c])) {
      *b[c] = Box3{{0, 0, 0}, {0, 0, 0}};
      continue;
    }
    if (!inside(*b[c], arr) || !inside(*b[c], A.R)) return (int)hipErrorInvalidValue;
    if (b[c]->lo[back[c][0]] < 1 || b[c]->lo[back[c][1]] < 1) return (int)hipErrorInvalidValue;
    U = box_union(U, *b[c]);
  }
  if (box_empty(U)) return 0;
  A.U = U;
  A.ny = ny, A.nz = nz;
  const int V = 16 / (int)sizeof(T);
  const int rnz = A.R.hi[2] - A.R.lo[2];
  bool vec = nz % V == 0 && rnz % V == 0 && A.R.lo[2] % V == 0 && A.R.lo[2] >= 0;
  for (int c = 0; c < 3; ++c)
    vec = vec && (uintptr_t)e[c] % 16 == 0 && (uintptr_t)h[c] % 16 == 0 && (uintptr_t)ca[c] % 16 == 0 &&
          (uintptr_t)cb[c] % 16 == 0;
  const int v = vec ? V : 1;
  if (lanes_out) *lanes_out = v;  // the cells a lane owns: which instance runs
  const int z0 = vec ? (U.lo[2] & ~(V - 1)) : U.lo[2];
  const int lanes = (U.hi[2] - z0 + v - 1) / v;
  int zshift = 0;
  while (zshift < 6 && (1 << zshift) < lanes) ++zshift;
  A.zshift = zshift;
  const dim3 grid(cdiv(lanes, 1 << zshift), cdiv(U.hi[1] - U.lo[1], 256 >> zshift), (unsigned)(U.hi[0] - U.lo[0]));
  if (grid.y > 65535u || grid.z > 65535u) return (int)hipErrorInvalidValue;
  T* const* E = (T* const*)e;
  const T* const* H = (const T* const*)h;
  const T* const* CA = (const T* const*)ca;
  const T* const* CB = (const T* const*)cb;
  if (vec)
    k_lossy_e<T, 16 / (int)sizeof(T)><<<grid, 256, 0, s>>>(E[0], E[1], E[2], H[0], H[1], H[2], CA[0], CA[1], CA[2],
                                                            CB[0], CB[1], CB[2], A);
  else
    k_lossy_e<T, 1><<<grid, 256, 0, s>>>(E[0], E[1], E[2], H[0], H[1], H[2], CA[0], CA[1], CA[2], CB[0], CB[1],
                                         CB[2], A);
  FDTD_RETURN_LAUNCH_STATUS();
}

}  // namespace

FDTD_API int fdtd_lossy_e_f32(void* const* e, const void* const* h, const void* const* ca, const void* const* cb,
                              int nx, int ny, int nz, const int* boxes, const int* rbox, void* s, int* lanes) {
  return lossy_e<float>(e, h, ca, cb, nx, ny, nz, boxes, rbox, (hipStream_t)s, lanes);
}

FDTD_API int fdtd_lossy_e_f64(void* const* e, const void* const* h, const void* const* ca, const void* const* cb,
                              int nx, int ny, int nz, const int* boxes, const int* rbox, void* s, int* lanes) {
  return lossy_e<double>(e, h, ca, cb, nx, ny, nz, boxes, rbox, (hipStream_t)s, lanes);
}
