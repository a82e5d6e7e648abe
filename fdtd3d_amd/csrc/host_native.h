// Host-side native runtime pieces shared by the standalone driver:
// topology optimiser, Yee computation ranges, hybrid pass geometry, the chain /
// plain region plan of 3D UPML runs, DAT/BMP writers.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace fdtd {

using Int3 = std::array<int, 3>;

// ---- topology (same cost model as fdtd3d_amd/parallel/topology.py) ----
double halo_cost(const Int3& size, const Int3& topo);
Int3 optimal_topology(const Int3& size, int nprocs, const std::vector<int>& axes);
void chunk_bounds(int n, int p, int coord, int& lo, int& hi);

// ---- Yee layout (fdtd3d_amd/layout/yee.py) ----
// component index: 0..2 = Ex,Ey,Ez; 3..5 = Hx,Hy,Hz
void global_range(int comp, const Int3& size, const std::vector<int>& active_axes, Int3& lo, Int3& hi);

// ---- hybrid pass geometry (one plan for both drivers) ----
// A hybrid pass (models/blocking.py _init_hybrid) advances the core box K by
// T steps in the blocked kernel and steps the rest; step s (0-based) of the
// stepped shell covers everything of the allocated box but the core cells
// deeper than T - s inside K (depth along the active axes; a side of K on the
// domain border has no shell beyond it), plus the cut box Dm (a stepped
// dispersive box inside K; empty: none) grown by T - s; after the pass the
// shell (alloc minus K, plus Dm) is copied into the core pass's output.
// Boxes are lo[3], hi[3].  False when a step's core vanishes.
using Box6 = std::array<int, 6>;
std::vector<Box6> box_minus6(const Box6& a, const Box6& b);  // non-empty slabs: x low / high, y, z
bool hybrid_windows(const Box6& alloc, const Box6& K, const Box6& Dm, int T, const bool* act, const Int3& size,
                    std::vector<std::vector<Box6>>& shells, std::vector<Box6>& copy);

// ---- chain / plain regions of a 3D UPML or dispersive run (models/scheme.py _init_chain_regions) ----
// The D/B chain runs only where it differs from the plain update: the PML
// slabs (one cell of staggering slack: whole minus the inner box) and the
// dispersive sphere's box; the plain kernels run on the rest.  `chain` lists
// the slabs (x low / high, then y, then z; disp false), then the dispersive
// box (disp true); `plain` the inner box, or its slabs around the dispersive
// box.  A dispersive box that reaches the slabs (or an inner box that
// vanishes) makes the whole grid one dispersive chain region.
struct ChainRegions {
  std::vector<Box6> chain, plain;
  std::vector<bool> disp;  // per chain region: holds dispersive cells
};
// bounding box of the sphere's smoothed cells with the stencils' reach, clamped to the grid
Box6 dispersive_box(const Int3& size, const double* ctr, double radius);
ChainRegions chain_regions(const Int3& size, const int* pml, bool use_pml, bool has_dbox, const Box6& dbox);

// ---- files (reference naming, Source/File-Management/Commons.h:56-68) ----
std::string grid_file_name(long step, int rank, const std::string& name, const std::string& dir);
bool write_dat(const std::string& path, const void* data, size_t bytes);
// rgb: "rgb" (blue-green-red) or "gray"; values row-major [w][h]; pixel (x, y), y = 0 top
bool write_bmp(const std::string& path, const std::vector<double>& values, int w, int h,
               const std::string& palette);

}  // namespace fdtd
