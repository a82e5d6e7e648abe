// Field probes (models/probe.py): the time series of single Yee samples.  ONE
// launch per sample covers every slot of a monitor: a device table of
// fixed-size entries (field array, linear element offset), thread s loads the
// element of slot s, widens it to fp64 (exact) and stores it to row `row` of
// the row-major fp64 buffer series[capacity][nslots].  No arithmetic, no
// atomics, no LDS; a slot is a RAW sample -- cell-centre means are formed on
// read, so serial and decomposed runs share one path.
//
// The sample number is passed BY VALUE (as the DFT kernel takes its twiddles):
// nothing on the device counts samples, and the host never reads one back.
// The kernel checks nothing beyond s < nslots: the host validates every offset
// against its array before the table is built (ops/hip_monitors.py), and the
// entry point refuses a row outside the buffer.
#include "common.h"
#include "monitor_dev.h"

namespace {

struct ProbeEnt {
  long long f;    // field array base
  long long off;  // element offset of the sample in it
};
static_assert(sizeof(ProbeEnt) == 16, "ProbeEnt layout (ops/probe.py PROBE_ENT_SIZE)");

template <typename T>
__global__ __launch_bounds__(256) void k_probe_sample(const ProbeEnt* __restrict__ tab, int nslots,
                                                      double* __restrict__ series, long long row) {
  const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (s >= nslots) return;
  const mon::ConstTab<ProbeEnt> E = (mon::ConstTab<ProbeEnt>)tab;
  const T* F = (const T*)E[s].f;
  series[(size_t)row * (size_t)nslots + (size_t)s] = (double)F[E[s].off];
}

template <typename T>
int probe_sample(const void* tab, int nslots, void* series, int row, int capacity, hipStream_t s) {
  if (nslots < 0 || row < 0 || row >= capacity || !tab || !series) return (int)hipErrorInvalidValue;
  if (nslots == 0) return 0;
  k_probe_sample<T><<<cdiv(nslots, 256), 256, 0, s>>>((const ProbeEnt*)tab, nslots, (double*)series, (long long)row);
  FDTD_RETURN_LAUNCH_STATUS();
}

}  // namespace

// One sample of a probe monitor: `tab` = nslots device entries of
// fdtd_probe_ent_size() bytes, `series` = capacity x nslots device doubles,
// 0 <= row < capacity the row this sample fills.
FDTD_API int fdtd_probe_sample_f32(const void* tab, int nslots, void* series, int row, int capacity, void* s) {
  return probe_sample<float>(tab, nslots, series, row, capacity, (hipStream_t)s);
}
FDTD_API int fdtd_probe_sample_f64(const void* tab, int nslots, void* series, int row, int capacity, void* s) {
  return probe_sample<double>(tab, nslots, series, row, capacity, (hipStream_t)s);
}
FDTD_API int fdtd_probe_ent_size() { return (int)sizeof(ProbeEnt); }
