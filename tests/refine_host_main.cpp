// refine_host_main.cpp - the per-pixel criteria and the verdict of blacklight_amd/csrc/bl_refine.h without the library and without a GPU
// (tests/test_refine_shared_host.py builds this file with the host compiler, plainly and under ASan / UBSan). The blocks are read the
// way bl_refine_kernel reads them - every pixel through bl_refine_examined, the counts summed over all pixels - not by the host
// loop of bl_host.cpp, so that the header is exercised on its own.
//   refine_host_main < cases      one case per line: bs, five cuts, five fracs, then bs * bs pixels (nan, inf, -inf allowed)
//   prints one line per case: the block's flag, then examined / exceeded of every criterion that is on ("-" for one that is off)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bl_refine.h"

int main() {
  int bs = 0;
  while (std::scanf("%d", &bs) == 1) {
    if (bs < 1 || bs > 1024) return 2;
    BlRefineCuts cuts{};
    for (int c = 0; c < BL_REFINE_CRITERIA; c++)
      if (std::scanf("%lf", &cuts.cut[c]) != 1) return 2;
    for (int c = 0; c < BL_REFINE_CRITERIA; c++)
      if (std::scanf("%lf", &cuts.frac[c]) != 1) return 2;
    std::vector<double> block(static_cast<size_t>(bs) * bs);   // (exactly the block: a read beside it is the sanitizer's to report)
    for (double &value : block) {
      char word[64];
      if (std::scanf("%63s", word) != 1) return 2;
      value = std::strtod(word, nullptr);
    }
    auto q_at = [&](int i, int j) { return block[static_cast<size_t>(i) * bs + j]; };
    bool flag = false;
    std::string counts;
    for (int c = 0; c < BL_REFINE_CRITERIA; c++) {
      if (!(cuts.frac[c] >= 0.0)) {
        counts += " -";
        continue;
      }
      const int margin = bl_refine_margin(c);
      int num_examined = 0, num_exceeded = 0;
      for (int pixel = 0; pixel < bs * bs; pixel++) {
        const int i = pixel / bs, j = pixel - i * bs;
        if (i < margin || i >= bs - margin || j < margin || j >= bs - margin) continue;
        const double q = bl_refine_examined(c, q_at, i, j, bs);
        if (!bl_refine_counts(q)) continue;
        num_examined++;
        if (q > cuts.cut[c]) num_exceeded++;
      }
      counts += " " + std::to_string(num_examined) + "/" + std::to_string(num_exceeded);
      flag = flag || bl_refine_verdict(num_exceeded, num_examined, cuts.frac[c]);
    }
    std::printf("%d%s\n", flag ? 1 : 0, counts.c_str());
  }
  return 0;
}
