// User-placed sources (layout/source_file.py, ops/source.py): soft (added) and
// hard (set) dipole entries at chosen Yee samples.  ONE launch per half step
// covers every entry of a kind (E or H): a device table of fixed-size entries
// (field array, linear element offset, fp64 amplitude, signal index, flags)
// sorted by cell, read through the constant address space.
//
// A thread owns one distinct cell -- the first entry of the cell; an entry
// flagged SRC_SAME (same cell as the previous entry) belongs to that thread.
// It widens the field value to fp64 (exact), or starts from 0 when the cell's
// first entry is hard, adds amplitude * value[signal] for each of the cell's
// entries in table order (multiply and add rounded separately: no FMA
// contraction, as the oracle ops/torch_ops.py source_inject does) and stores
// the sum once, rounded to the field type.  No atomics, no LDS: the result
// does not depend on launch order.
//
// The up-to-64 signal values of the half step are computed by the host in fp64
// and passed BY VALUE in the kernel arguments (as the DFT kernel takes its
// twiddles).  The kernel checks nothing beyond i < n: the host validates every
// offset against its array and every signal index against the value count
// before the table is built (ops/hip_monitors.py), and the entry point refuses
// more than SRC_MAX_SIGNALS values.
#include "common.h"
#include "monitor_dev.h"

namespace {

constexpr int SRC_MAX_SIGNALS = 64;
constexpr int SRC_SAME = 1;  // same cell as the previous entry
constexpr int SRC_HARD = 2;  // the field is set, not added to

struct SrcEnt {
  long long f;    // field array base
  long long off;  // element offset of the cell in it
  double amp;     // field units
  int sig;        // index into the half step's signal values
  int flags;
};
static_assert(sizeof(SrcEnt) == 32, "SrcEnt layout (ops/source.py SOURCE_ENT_SIZE)");

struct SrcVals {
  double v[SRC_MAX_SIGNALS];
};

template <typename T>
__global__ __launch_bounds__(256) void k_source_inject(const SrcEnt* __restrict__ tab, int n, SrcVals vals) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const mon::ConstTab<SrcEnt> E = (mon::ConstTab<SrcEnt>)tab;
  const int fl = E[i].flags;
  if (fl & SRC_SAME) return;  // the cell's first entry owns it
  T* F = (T*)E[i].f;
  const long long off = E[i].off;
  double acc = (fl & SRC_HARD) ? 0.0 : (double)F[off];
  int j = i;
  do {
    // product and sum rounded separately (HIP contracts a * b + c by default, __dmul_rn / __dadd_rn included)
#pragma clang fp contract(off)
    const double term = E[j].amp * vals.v[E[j].sig];
    acc = acc + term;
    ++j;
  } while (j < n && (E[j].flags & SRC_SAME));
  F[off] = (T)acc;
}

template <typename T>
int source_inject(const void* tab, int n, const double* values, int nvalues, hipStream_t s) {
  if (n < 0 || nvalues < 0 || nvalues > SRC_MAX_SIGNALS || !tab || (nvalues > 0 && !values))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  SrcVals v;
  for (int k = 0; k < SRC_MAX_SIGNALS; ++k) v.v[k] = k < nvalues ? values[k] : 0.0;
  k_source_inject<T><<<cdiv(n, 256), 256, 0, s>>>((const SrcEnt*)tab, n, v);
  FDTD_RETURN_LAUNCH_STATUS();
}

}  // namespace

// One half step of a source list: `tab` = n device entries of
// fdtd_source_ent_size() bytes sorted by cell, `values` = nvalues <=
// fdtd_source_max_signals() host doubles, the signals' values at this half step.
FDTD_API int fdtd_source_inject_f32(const void* tab, int n, const double* values, int nvalues, void* s) {
  return source_inject<float>(tab, n, values, nvalues, (hipStream_t)s);
}
FDTD_API int fdtd_source_inject_f64(const void* tab, int n, const double* values, int nvalues, void* s) {
  return source_inject<double>(tab, n, values, nvalues, (hipStream_t)s);
}
FDTD_API int fdtd_source_ent_size() { return (int)sizeof(SrcEnt); }
FDTD_API int fdtd_source_max_signals() { return SRC_MAX_SIGNALS; }
