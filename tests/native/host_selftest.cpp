// Host-runtime self test, built with AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_native_cpu.py::test_host_runtime_under_sanitizers (the
// reference's only guards were ASSERT + backtrace, Source/Helpers/Assert.h:25-91).
// Exercises the settings parser (every option kind, cmd-file round trip, bad
// input), the topology optimiser, chunk bounds, the chain / plain region plan
// of 3D UPML / dispersive runs, file naming and the DAT / BMP writers; exits
// non-zero when a check failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_native.h"
#include "settings_native.h"

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

using fdtd::Box6;

static long long vol6(const Box6& b) {
  if (b[3] <= b[0] || b[4] <= b[1] || b[5] <= b[2]) return 0;
  return (long long)(b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
}

// chain + plain regions: pairwise disjoint, volumes summing to the grid's
static void check_partition(const fdtd::ChainRegions& R, const fdtd::Int3& n) {
  std::vector<Box6> all = R.chain;
  all.insert(all.end(), R.plain.begin(), R.plain.end());
  long long sum = 0;
  for (size_t p = 0; p < all.size(); ++p) {
    CHECK(vol6(all[p]) > 0);
    sum += vol6(all[p]);
    for (size_t q = p + 1; q < all.size(); ++q) {
      Box6 c;
      for (int a = 0; a < 3; ++a) {
        c[a] = std::max(all[p][a], all[q][a]);
        c[3 + a] = std::min(all[p][3 + a], all[q][3 + a]);
      }
      CHECK(vol6(c) == 0);
    }
  }
  CHECK(sum == (long long)n[0] * n[1] * n[2]);
  CHECK(R.disp.size() == R.chain.size());
}

// fdtd::chain_regions on a 40^3 grid with a sphere at the centre: the four
// region plans of a 3D UPML / dispersive run, expected boxes derived by hand
static void check_chain_regions() {
  const fdtd::Int3 n = {40, 40, 40};
  const int pml[3] = {10, 10, 10};
  const double ctr[3] = {20.0, 20.0, 20.0};
  const Box6 none = {0, 0, 0, 0, 0, 0};
  // the six slabs of [0, 40)^3 minus [11, 29)^3: x low / high, then y, then z
  const std::vector<Box6> shell = {{0, 0, 0, 11, 40, 40},   {29, 0, 0, 40, 40, 40},   {11, 0, 0, 29, 11, 40},
                                   {11, 29, 0, 29, 40, 40}, {11, 11, 0, 29, 29, 11}, {11, 11, 29, 29, 29, 40}};
  const Box6 inner = {11, 11, 11, 29, 29, 29};
  {  // A: PML 10 and a radius-5 sphere: its box [13, 28)^3 lies inside the inner box
    const Box6 d = fdtd::dispersive_box(n, ctr, 5.0);
    CHECK((d == Box6{13, 13, 13, 28, 28, 28}));
    const fdtd::ChainRegions R = fdtd::chain_regions(n, pml, true, true, d);
    CHECK(R.chain.size() == 7 && R.plain.size() == 6);
    for (size_t q = 0; q < 6 && q < R.chain.size(); ++q) CHECK(R.chain[q] == shell[q] && !R.disp[q]);
    CHECK(R.chain.back() == d && R.disp.back());
    const std::vector<Box6> rest = {{11, 11, 11, 13, 29, 29}, {28, 11, 11, 29, 29, 29}, {13, 11, 11, 28, 13, 29},
                                    {13, 28, 11, 28, 29, 29}, {13, 13, 11, 28, 28, 13}, {13, 13, 28, 28, 28, 29}};
    CHECK(R.plain == rest);
    check_partition(R, n);
  }
  {  // B: radius 8: the box starts at 10, below the inner box's 11 -- one dispersive chain region, the grid
    const Box6 d = fdtd::dispersive_box(n, ctr, 8.0);
    CHECK(d[0] == 10 && d[3] == 31);
    const fdtd::ChainRegions R = fdtd::chain_regions(n, pml, true, true, d);
    CHECK(R.chain.size() == 1 && R.plain.empty());
    CHECK((R.chain[0] == Box6{0, 0, 0, 40, 40, 40}) && R.disp[0]);
    check_partition(R, n);
  }
  {  // C: no PML, the radius-5 sphere: the chain is its box, the plain update on the six slabs around it
    const Box6 d = fdtd::dispersive_box(n, ctr, 5.0);
    const fdtd::ChainRegions R = fdtd::chain_regions(n, pml, false, true, d);
    CHECK(R.chain.size() == 1 && R.chain[0] == d && R.disp[0]);
    const std::vector<Box6> rest = {{0, 0, 0, 13, 40, 40},   {28, 0, 0, 40, 40, 40},   {13, 0, 0, 28, 13, 40},
                                    {13, 28, 0, 28, 40, 40}, {13, 13, 0, 28, 28, 13}, {13, 13, 28, 28, 28, 40}};
    CHECK(R.plain == rest);
    check_partition(R, n);
  }
  {  // D: PML only: the six slabs, none dispersive, and the inner box on the plain update
    const fdtd::ChainRegions R = fdtd::chain_regions(n, pml, true, false, none);
    CHECK(R.chain == shell);
    for (bool f : R.disp) CHECK(!f);
    CHECK(R.plain.size() == 1 && R.plain[0] == inner);
    check_partition(R, n);
  }
  // the dispersive box is clamped to the grid
  const double corner[3] = {1.0, 20.0, 39.0};
  CHECK((fdtd::dispersive_box(n, corner, 5.0) == Box6{0, 13, 32, 9, 28, 40}));
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  check_chain_regions();
  {
    fdtd::Settings s;
    const char* a[] = {"fdtd3d", "--3d", "--sizex", "64", "--same-size", "--use-pml", "--pml-type", "cpml",
                       "--cpml-kappa-max", "3.5", "--angle-teta", "30", "--output-dir", "/tmp/x", "--time-block", "5"};
    CHECK(s.parse(16, a) == fdtd::SETTINGS_OK);
    CHECK(s.sizeX == 64 && s.sizeY == 64 && s.sizeZ == 64);
    CHECK(s.doUsePML && s.pmlType == "cpml" && s.cpmlKappaMax == 3.5);
    CHECK(s.timeBlock == 5);
    CHECK(!s.help().empty() && !s.to_json().empty());
  }
  {
    fdtd::Settings s;
    const char* bad[] = {"fdtd3d", "--sizex", "not-a-number"};
    CHECK(s.parse(3, bad) != fdtd::SETTINGS_OK);
    const char* unk[] = {"fdtd3d", "--no-such-option"};
    fdtd::Settings s2;
    CHECK(s2.parse(2, unk) != fdtd::SETTINGS_OK);
    const char* missing[] = {"fdtd3d", "--sizex"};
    fdtd::Settings s3;
    CHECK(s3.parse(2, missing) != fdtd::SETTINGS_OK);
  }
  {
    fdtd::Settings s;
    std::vector<std::string> toks = {"--2d", "--sizex", "40", "--sizey", "30", "--dx", "0.001"};
    CHECK(s.parse(toks, false) == fdtd::SETTINGS_OK);
    CHECK(s.sizeX == 40 && s.sizeY == 30 && s.gridStep == 0.001);
  }
  for (int p : {1, 2, 3, 4, 6, 8, 12, 16}) {
    const fdtd::Int3 t = fdtd::optimal_topology({128, 96, 64}, p, {0, 1, 2});
    CHECK(t[0] * t[1] * t[2] == p);
    int covered = 0;
    for (int c = 0; c < t[0]; ++c) {
      int lo = 0, hi = 0;
      fdtd::chunk_bounds(128, t[0], c, lo, hi);
      CHECK(lo == covered && hi > lo);
      covered = hi;
    }
    CHECK(covered == 128);
  }
  CHECK(fdtd::halo_cost({64, 64, 64}, {2, 2, 2}) > 0.0);
  const std::string name = fdtd::grid_file_name(100, 3, "Ez", dir);
  CHECK(name.find("[100]") != std::string::npos && name.find("rank-3") != std::string::npos);
  std::vector<float> data(4096);
  for (size_t n = 0; n < data.size(); ++n) data[n] = 0.5f * (float)n;
  CHECK(fdtd::write_dat(dir + "/selftest.dat", data.data(), data.size() * sizeof(float)));
  std::vector<double> img(37 * 23);
  for (size_t n = 0; n < img.size(); ++n) img[n] = (double)((n * 7919) % 101) - 50.0;
  CHECK(fdtd::write_bmp(dir + "/selftest.bmp", img, 37, 23, "rgb"));
  CHECK(fdtd::write_bmp(dir + "/selftest-gray.bmp", img, 37, 23, "gray"));
  std::printf("host selftest: %d failed checks\n", g_fail);
  return g_fail ? 1 : 0;
}
