// device_grid_host_main.cpp - the host's check of a bl_device_cells description (CheckDeviceCells, blacklight_amd/csrc/bl_grid.cpp)
// without a GPU and without the library: tests/test_device_grid_host.py builds this file with bl_grid.cpp, once plainly and once under
// the host sanitizers.
//
//   device_grid_host_main < cases
//       every line of standard input is one case of 15 integers:
//         n_blocks n_i n_j n_k n_var ind_kappa first_index code_kappa  cells prim dtype wait var_stride block_stride n_elements
//       first_index: ind_rho; the other seven variables follow it one by one. cells: 0 hands the check a null description. prim: the
//       address itself (never read). For every case one line comes out: "ok", or "refused <code> <text>".
#include <cinttypes>
#include <cstdio>

#include "bl_ctx.h"
#include "bl_grid.h"

int main() {
  long long v[15];
  int cases = 0;
  for (;;) {
    int got = 0;
    for (; got < 15; got++)
      if (std::scanf("%lld", &v[got]) != 1) break;
    if (got == 0) break;
    if (got != 15) {
      std::fprintf(stderr, "case %d cut short\n", cases);
      return 1;
    }
    bl_grid_desc g{};
    g.n_blocks = static_cast<int32_t>(v[0]); g.n_i = static_cast<int32_t>(v[1]); g.n_j = static_cast<int32_t>(v[2]); g.n_k = static_cast<int32_t>(v[3]);
    g.n_var = static_cast<int32_t>(v[4]);
    g.ind_kappa = static_cast<int32_t>(v[5]);
    const int32_t first = static_cast<int32_t>(v[6]);
    g.ind_rho = first; g.ind_pgas = first + 1; g.ind_uu1 = first + 2; g.ind_uu2 = first + 3; g.ind_uu3 = first + 4;
    g.ind_bb1 = first + 5; g.ind_bb2 = first + 6; g.ind_bb3 = first + 7;
    bl_device_cells cells{};
    cells.prim = reinterpret_cast<const void *>(static_cast<uintptr_t>(v[9]));
    cells.dtype = static_cast<int32_t>(v[10]);
    cells.wait = static_cast<int32_t>(v[11]);
    cells.var_stride = v[12]; cells.block_stride = v[13]; cells.n_elements = v[14];
    try {
      blhost::CheckDeviceCells(g, v[7] != 0, v[8] != 0 ? &cells : nullptr);
      std::printf("ok\n");
    } catch (const blhost::Failure &failure) {
      std::printf("refused %d %s\n", failure.code, failure.message.c_str());
    }
    cases++;
  }
  return cases > 0 ? 0 : 1;
}
