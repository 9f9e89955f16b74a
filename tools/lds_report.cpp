// Tuning aid (not part of the product): prints the map update's workgroup LDS layout and the fused step's LDS total over the
// capacities and launch shapes the engine can pick, one line each, so that two builds can be diffed:
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -Iinclude -Irfs-slam_amd/csrc tools/lds_report.cpp -o lds_report && ./lds_report
// Column 4 (the step's total) decides workgroups per CU and must not move when the map layout changes.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "rfsgpu.h"
#include "step_fused.h"

int main() {
  for (int cap = 32; cap <= 1024; cap += 32) {
    std::printf("map  cap %4d  Z+block %6zu\n", cap, (size_t)RFS_Z_LDS_BYTES + update_map_block_lds_bytes(cap));
    for (int evalCap : {15, 40, 64})
      for (int nZ : {1, 30, 64})
        for (int wpp : {2, 3})
          for (int gl : {5, 6})
            std::printf("step cap %4d evalCap %2d nZ %2d wpp %d GL %d  total %6zu\n", cap, evalCap, nZ, wpp, gl,
                        step_fused_lds_total(cap, evalCap, nZ, wpp, gl));
  }
  return 0;
}
