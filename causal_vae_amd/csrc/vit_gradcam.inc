// vit_gradcam.inc — Grad-CAM on the stem output (DESIGN.md section 21; the arithmetic of mnist_test/02_mechanism_analysis/analyze_gradcam.py's
// GradCAM.__call__ without its resize): one workgroup of 256 threads per image, one launch, no workspace, no atomics.
//   1. w[c] = (1 / n) sum_i dA[b][i][c]: thread c owns channel c and adds the n rows in index order (one fp32 chain; a row is 256 consecutive elements
//      across the workgroup, so every load instruction is coalesced), then multiplies by 1.0f / n once.
//   2. cam[i] = max(0, sum_c w[c] A[b][i][c]): wave v takes rows v, v + 4, ...; lane l the channels 4 l .. 4 l + 3 (one 16-byte / 8-byte load) as a 4-term fma
//      chain started at 0, then the xor-shuffle wave sum (offsets 32, 16, ..., 1).  The map stays in LDS.
//   3. normalize: cam = (cam - min) / (max - min + 1e-8f) with the workgroup's min and max over i (order-free), else the map as it is.
// n <= GRADCAM_MAX_N (the LDS map); included inside vit.hip's anonymous namespace.
#define GRADCAM_MAX_N 4096

template <typename T>
__global__ __launch_bounds__(256) void vit_gradcam_kernel(const T* __restrict__ A, const T* __restrict__ dA, float* __restrict__ cam, int n, int normalize) {
    __shared__ __attribute__((aligned(16))) float wsh[VIT_DIM];
    __shared__ float map[GRADCAM_MAX_N];
    __shared__ float red[8];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t base = (size_t)blockIdx.x * n * VIT_DIM;
    const T* dAb = dA + base;
    const T* Ab = A + base;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += to_f32(dAb[(size_t)i * VIT_DIM + t]);
    wsh[t] = s * (1.0f / (float)n);
    __syncthreads();
    const f32x4 wv = *(const f32x4*)&wsh[4 * lane];
    float lo = INFINITY, hi = -INFINITY;
    for (int i = wave; i < n; i += 4) {
        float a[4];
        load_f32<4>(Ab + (size_t)i * VIT_DIM + 4 * lane, a);
        float p = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) p = fmaf(wv[e], a[e], p);
        p = fmaxf(wave_sum(p), 0.f);
        if (lane == 0) map[i] = p;
        lo = fminf(lo, p);
        hi = fmaxf(hi, p);
    }
    if (lane == 0) { red[wave] = lo; red[4 + wave] = hi; }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    const float inv = hi - lo + 1e-8f;
    float* out = cam + (size_t)blockIdx.x * n;
    for (int i = t; i < n; i += 256) out[i] = normalize ? (map[i] - lo) / inv : map[i];
}
