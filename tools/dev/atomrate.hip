// Development only: the rate of returning atomicAdd(1) on ONE device address, drawn the way the lane kernel draws chunks --
// one lane of one wave per workgroup, each draw waiting for the one before it -- from 1, 64 and 256 workgroups.
//   hipcc -O3 --offload-arch=gfx950 -o tools/dev/atomrate tools/dev/atomrate.hip && tools/dev/atomrate
#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void draw(unsigned *ctr, unsigned per_wg, unsigned *sink)
{
  unsigned v = 0;
  if (threadIdx.x == 0)
    for (unsigned i = 0; i < per_wg; i++) v += atomicAdd(ctr, 1u);
  if (v == 0xdeadbeefu) *sink = v;
}
int main()
{
  unsigned *d;
  hipEvent_t a, b;
  if (hipMalloc(&d, 8) != hipSuccess || hipMemset(d, 0, 8) != hipSuccess) return 1;
  hipEventCreate(&a); hipEventCreate(&b);
  for (unsigned wgs : {1u, 64u, 256u}) {
    const unsigned per_wg = 20000;
    draw<<<wgs, 64>>>(d, 100, d + 1);
    hipEventRecord(a); draw<<<wgs, 64>>>(d, per_wg, d + 1); hipEventRecord(b);
    float ms = 0;
    if (hipEventSynchronize(b) != hipSuccess) return 1;
    hipEventElapsedTime(&ms, a, b);
    printf("%3u workgroups x %u dependent draws: %.3f ms, %.1f M atomics/s in all, %.0f ns per draw of a workgroup\n", wgs, per_wg, ms,
           wgs * (double)per_wg / ms / 1e3, ms * 1e6 / per_wg);
  }
  return 0;
}
