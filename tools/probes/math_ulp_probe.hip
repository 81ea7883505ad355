// Largest error, in fp32 ulps of the exact result, of the device math functions csrc/losses.hip calls (expf, logf, log1pf, sqrtf, rsqrtf, powf, the
// fp32 division and 1.f / x), against the float64 function of the same fp32 argument, over the argument ranges of tests/test_loss_reference.py; and of
// __expf, which apply_act (common.h) calls for the sigmoid, over [-8, 8], the range tests/test_dense_reference.py keeps its sigmoid pre-activations in.
// Compiled with the flags of csrc/Makefile, so the functions are the ones the library gets.  Record: the ULP tables of oracle/loss64.py and oracle/dense64.py.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o math_ulp_probe tools/probes/math_ulp_probe.hip && ./math_ulp_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

enum { F_EXP, F_LOG, F_LOG1P, F_SQRT, F_RSQRT, F_POW09, F_POW0999, F_DIV, F_RCP, F_FASTEXP, F_COUNT };
static const char* NAMES[F_COUNT] = {"expf", "logf", "log1pf(-p)", "sqrtf", "rsqrtf", "powf(0.9f, t)", "powf(0.999f, t)", "a / b", "1.f / x", "__expf"};

// |got - want| in ulps of want as an fp32 number (normal range)
__device__ double ulps(float got, double want) {
    if (want == 0.0) return got == 0.f ? 0.0 : 1e30;
    int e;
    frexp(fabs(want), &e);                                   // |want| = f 2^e, f in [0.5, 1): ulp = 2^(e - 24)
    if (e < -125) e = -125;
    return fabs((double)got - want) / ldexp(1.0, e - 24);
}
// sample i of n of [lo, hi], geometrically when lo > 0 && geo
__device__ float sample(long long i, long long n, double lo, double hi, bool geo) {
    const double t = (double)i / (double)(n - 1);
    return (float)(geo ? lo * pow(hi / lo, t) : lo + (hi - lo) * t);
}
__global__ void probe(int fn, long long n, double lo, double hi, bool geo, double* worst, float* arg) {
    double w = 0.0;
    float wa = 0.f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = sample(i, n, lo, hi, geo);
        float got;
        double want;
        switch (fn) {
        case F_EXP: got = expf(x); want = exp((double)x); break;
        case F_LOG: got = logf(x); want = log((double)x); break;
        case F_LOG1P: got = log1pf(-x); want = log1p(-(double)x); break;
        case F_SQRT: got = sqrtf(x); want = sqrt((double)x); break;
        case F_RSQRT: got = rsqrtf(x); want = 1.0 / sqrt((double)x); break;
        case F_POW09: { const float t = floorf(x); got = powf(0.9f, t); want = pow((double)0.9f, (double)t); break; }
        case F_POW0999: { const float t = floorf(x); got = powf(0.999f, t); want = pow((double)0.999f, (double)t); break; }
        case F_DIV: { const float b = sample((i * 7919) % n, n, lo, hi, geo); got = x / b; want = (double)x / (double)b; break; }
        case F_FASTEXP: got = __expf(x); want = exp((double)x); break;
        default: got = 1.f / x; want = 1.0 / (double)x; break;
        }
        if (fabs(want) < 1e-37) continue;                    // subnormal results are not in any case's range
        const double u = ulps(got, want);
        if (u > w) { w = u; wa = x; }
    }
    worst[blockIdx.x * blockDim.x + threadIdx.x] = w;
    arg[blockIdx.x * blockDim.x + threadIdx.x] = wa;
}

int main() {
    struct Range { int fn; double lo, hi; bool geo; };
    const Range R[] = {
        {F_EXP, -80.0, 0.0, false}, {F_EXP, -10.0, 10.0, false}, {F_EXP, -1.0, 1.0, false},
        {F_LOG, 1e-37, 1.0, true}, {F_LOG, 0.5, 2.0, false}, {F_LOG, 1.0, 1e6, true},
        {F_LOG1P, 1e-30, 0.5, true}, {F_LOG1P, 0.5, 0.99999994, false},
        {F_SQRT, 1e-30, 1e12, true}, {F_RSQRT, 1e-12, 1e12, true}, {F_RSQRT, 1e-6, 4.0, false},
        {F_POW09, 1.0, 2000.0, false}, {F_POW09, 1.0, 100001.0, false}, {F_POW0999, 1.0, 2000.0, false}, {F_POW0999, 1.0, 100001.0, false},
        {F_DIV, 1e-12, 1e12, true}, {F_DIV, 0.5, 2.0, false}, {F_RCP, 1e-12, 1e12, true}, {F_RCP, 0.5, 2.0, false},
        {F_FASTEXP, -8.0, 8.0, false}, {F_FASTEXP, -1.0, 1.0, false}, {F_FASTEXP, -8.0, -7.0, false}, {F_FASTEXP, 7.0, 8.0, false},
    };
    const int blocks = 1024, threads = 256, T = blocks * threads;
    const long long n = 1LL << 26;
    double* dw;
    float* da;
    if (hipMalloc(&dw, T * sizeof(double)) != hipSuccess || hipMalloc(&da, T * sizeof(float)) != hipSuccess) return 1;
    std::vector<double> w(T);
    std::vector<float> a(T);
    double per_fn[F_COUNT] = {0};
    for (const Range& r : R) {
        hipLaunchKernelGGL(probe, dim3(blocks), dim3(threads), 0, 0, r.fn, n, r.lo, r.hi, r.geo, dw, da);
        if (hipMemcpy(w.data(), dw, T * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        if (hipMemcpy(a.data(), da, T * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        int best = 0;
        for (int i = 1; i < T; ++i) if (w[i] > w[best]) best = i;
        printf("%-16s [%g, %g] %s: max %.4f ulp at %.9g\n", NAMES[r.fn], r.lo, r.hi, r.geo ? "geometric" : "linear", w[best], a[best]);
        if (w[best] > per_fn[r.fn]) per_fn[r.fn] = w[best];
    }
    for (int f = 0; f < F_COUNT; ++f) printf("MAX %-16s %.4f ulp\n", NAMES[f], per_fn[f]);
    hipFree(dw);
    hipFree(da);
    return 0;
}
