// bl_grid.h - everything about a grid except its cells, built on the host (bl_grid.cpp): validation of the caller's description, the
// merged tiling or the block lattice, coordinate rows, bucket tables, search guesses, the (level, location) hash, the fused kernels'
// descriptors and the three LDS byte budgets. No GPU call: bl_api.hip uploads each table once and binds BlGridDevice's pointers;
// tests/grid_host_main.cpp runs everything here on any machine.
#ifndef BLACKLIGHT_AMD_BL_GRID_H_
#define BLACKLIGHT_AMD_BL_GRID_H_
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/blacklight_amd.h"
#include "bl_device.h"

namespace blhost {

// How the caller's planes ([variable][block][k][j][i]) become the cell array: the eight variables in the kernels' order, and where a
// block's cells go in a merged array (has_origin; else the blocks stay one behind the other)
struct CellPlacement {
  size_t n_cells = 0;
  int nb[3] = {0, 0, 0};
  int order[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool has_origin = false;
  std::vector<unsigned long long> origin;   // first target cell of every block
  unsigned long long row_stride = 0, plane_stride = 0;
};

// Where in its buffer each table of BlGridDevice starts (elements; kNone: the pointer stays null). fused_desc, hash_keys and sks_map
// are buffers of their own: bound where the table is not empty / dev.fmks is set.
struct GridOffsets {
  static constexpr size_t kNone = ~static_cast<size_t>(0);
  size_t xf[3] = {kNone, kNone, kNone}, xv[3] = {kNone, kNone, kNone}, angle_trig[2] = {kNone, kNone};                      // coords, merged grid
  size_t bxf[3] = {kNone, kNone, kNone}, bxv[3] = {kNone, kNone, kNone}, xv_next[3] = {kNone, kNone, kNone};                // coords, lattice
  size_t row_guess[3] = {kNone, kNone, kNone}, edge[3] = {kNone, kNone, kNone};
  size_t bucket[3] = {kNone, kNone, kNone};                                                                                 // buckets
  size_t lattice = kNone, block_row[3] = {kNone, kNone, kNone};                                                             // lattice
  size_t levels = kNone, locations = kNone, hash_blocks = kNone;                                                            // block_table
};

struct GridTables {
  std::vector<double> coords;              // merged: x1f x1v x2f x2v x3f x3v, (cos, sin) of the theta and phi centres; lattice: per axis rows, next centres, row guesses, edges
  std::vector<unsigned short> buckets;     // merged: bucket -> first candidate cell, the three axes
  std::vector<int> lattice;                // box -> block, then the blocks' rows
  std::vector<unsigned int> fused_desc;    // per box, where the fused kernels take the mesh
  std::vector<int> block_table;            // inter-block interpolation: levels, locations, hash blocks
  std::vector<unsigned long long> block_keys;   // ... and hash keys
  std::vector<float> kappa;                // plasma_model = code_kappa on a merged grid of several blocks: the plane repacked; else it is uploaded as it lies
  BlGridDevice dev{};                      // every scalar; every pointer null
  GridOffsets at;
  bool code_kappa = false;                 // dev.kappa is to be bound
  CellPlacement placement;
  int lds_table_bytes = 0;                 // merged grid: what the locate kernels stage in LDS; 0: searched in HBM
  int merged_blocks[3] = {1, 1, 1};        // merged grid: the block lattice's extent
  std::vector<int> merged_block_at;        // ... and lattice position (k, j, i of the block) -> MeshBlock of the file (sample checkpoints)
  double outer_x1 = 0.0;                   // largest outer x1 face of the grid's blocks
  // The geometry as handed over - block table, coordinate arrays, FMKS look-up table - and its hash: what decides WHERE a sample lies.
  // Two descriptions with the same geometry (SameGeometry) may differ in their cells only.
  unsigned long long geometry = 0;
  std::vector<unsigned char> given;        // the bytes the hash ran over: extents, the six coordinate arrays, levels, locations, sks_map and its scalars
  int given_tables = 0;                    // ... and which of levels (1), locations (2), sks_map (4) were there
};

// Validates `g` and builds the tables: the merged tiling, else (or with simulation_block_interp) the block lattice. Throws Failure
// with the refusal's code and text. Reads g.prim for the repacked kappa plane only; with g.prim null (cells in device memory) kappa
// stays empty and the staging kernel places that plane.
GridTables BuildGridTables(const bl_params &p, const bl_grid_desc &g);
// ... its first step, which bl_set_grid takes before it reads the arrays: extents of at least 1 block of 2 x 2 x 2 cells, the six
// coordinate arrays there
void ValidateGridDescription(const bl_grid_desc &g);
// t.dev with every pointer set, in this one place: base of the table's buffer plus its offset (device buffers for the kernels; the
// host vectors themselves for a program that reads the tables as a kernel would)
struct GridBases {
  const float *cells, *kappa;
  const double *coords;
  const unsigned short *buckets;
  const int *lattice;
  const unsigned int *fused_desc;
  const int *block_table;
  const unsigned long long *block_keys;
  const double *sks_map;
};
BlGridDevice BindGridTables(const GridTables &t, const GridBases &base);
unsigned long long GridGeometryHash(const bl_grid_desc &g);
// The eight variables in the kernels' order; false: an index (ind_kappa too, where `code_kappa`) lies outside [0, n_var)
bool GridVariableOrder(const bl_grid_desc &g, bool code_kappa, int order[8]);
// bl_set_grid_device's description of the caller's device array, checked as far as the host can (Failure with BL_E_ARG and a text
// each): `cells` and its prim there, prim aligned to its element, dtype one of the two, both strides at least 1, and the furthest
// element the staging kernel reads - over the eight variables of GridVariableOrder, ind_kappa too where `code_kappa`, every block,
// a block's cells - below n_elements, in 64-bit arithmetic that notices its overflows. A description whose extents or indices are
// themselves out of range is left to ValidateGridDescription and GridVariableOrder, which refuse it before anything is launched.
void CheckDeviceCells(const bl_grid_desc &g, bool code_kappa, const bl_device_cells *cells);
// `g` carries the geometry `t` was built from, bit for bit (hash first, then the arrays themselves)
bool SameGeometry(const GridTables &t, const bl_grid_desc &g);

}  // namespace blhost
#endif  // BLACKLIGHT_AMD_BL_GRID_H_
