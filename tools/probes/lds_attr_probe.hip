// Host time of one hipFuncSetAttribute(MaxDynamicSharedMemorySize) call against one hipGetDevice call: what a per-device cache in cvae_allow_lds
// (csrc/common.h) could save per large-LDS launch.  No kernel runs.  Record: profiles/launch_lds.md.
//   hipcc --offload-arch=gfx950 -O2 -o lds_attr_probe tools/probes/lds_attr_probe.hip && ./lds_attr_probe
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
__global__ void k0(float* p) { extern __shared__ float s[]; if (p) p[0] = s[0]; }
__global__ void k1(float* p) { extern __shared__ float s[]; if (p) p[1] = s[1]; }
int main() {
    if (hipSetDevice(0) != hipSuccess) return 1;
    if (hipFree(nullptr) != hipSuccess) return 1;
    const int N = 200000;
    for (int rep = 0; rep < 3; ++rep) {
        auto t0 = std::chrono::steady_clock::now();
        int bad = 0;
        for (int i = 0; i < N; ++i) bad += hipFuncSetAttribute((i & 1) ? (const void*)k1 : (const void*)k0, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess;
        auto t1 = std::chrono::steady_clock::now();
        int dev = 0, sum = 0;
        for (int i = 0; i < N; ++i) { bad += hipGetDevice(&dev) != hipSuccess; sum += dev; }
        auto t2 = std::chrono::steady_clock::now();
        printf("rep %d: hipFuncSetAttribute %.1f ns/call, hipGetDevice %.1f ns/call (errors %d, %d)\n", rep,
               std::chrono::duration<double, std::nano>(t1 - t0).count() / N, std::chrono::duration<double, std::nano>(t2 - t1).count() / N, bad, sum);
    }
    return 0;
}
