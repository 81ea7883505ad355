// heads.hip — the dense heads of CausalViTVAE (vessel_analysis/00_core/models.py:225-250, 281-302) in ONE launch each:
//   enc_adapter      [cls_out | m | t] 287 -> 512 (BatchNorm1d, LeakyReLU 0.2) -> 256, split at 128 into mu (clamp +-100) | logvar (clamp +-10), z = mu + eps exp(logvar / 2)
//   dec_adapter      [m | z]           140 -> 256 (BatchNorm1d, LeakyReLU 0.2) -> 512
//   morph predictor  [t]                19 -> 64 (LeakyReLU 0.2) -> 64 (LeakyReLU 0.2) -> 12 | 12, the last layer read from two weight tensors, the second half clamped +-10
// fp32 throughout.  A workgroup owns HEADS_ROWS batch rows and carries them through every layer: the concatenated input rows and the hidden rows live in two LDS
// buffers that swap roles from layer to layer, nothing but the outputs goes back to memory (no cat buffer, no hidden activations, no chunk copies).
//
// Per layer the weight passes through LDS in tiles of HEADS_NC output columns x HEADS_KC inputs, pitch HEADS_KC + 1 words.  Both accesses are 4-byte ones
// (ds_write_b32, ds_read_b32 / ds_read2_b32), which bank on (address / 4) % 32 within each 32-lane half of a wave: the tile is written with lanes along k
// (consecutive words) and read with lanes along the columns (a stride of 129 words, 1 mod 32), so a half's 32 lanes fall on 32 different banks in both.
// The next tile's global loads are issued into registers before the
// current tile's products, so that only the first tile of a layer waits for memory.  Thread (c, g) owns column c of the tile for the row group g (HEADS_RPT
// rows): per k one ds_read of the weight, one 16-byte broadcast ds_read per row and 4 k, HEADS_RPT v_fma.  A row's value is ONE chain of fmaf over k = 0 .. K-1
// in one thread, started from 0, the bias added after it: the bits do not depend on the batch size, on the row's position in the batch, or on the grid (the
// sweeps compare a batched row with the same row alone).  No atomics, no cross-thread sums.
//
// Eval-mode BatchNorm1d is applied from the LIVE tensors on every call (scale = gamma / sqrt(running_var + eps), y = (v - running_mean) scale + beta): nothing
// derived from parameters survives a call, because parameters may be rewritten through raw pointers between calls.
//
// LDS: tile HEADS_NC (HEADS_KC + 1) 4 = 66 048 B, two activation buffers HEADS_ROWS (512 + 4) 4 = 33 024 B each: 132 096 B of the CU's 160 KiB (one workgroup
// per CU; the launch has one workgroup per 16 rows, so only the sweeps ever fill the chip).  A workgroup re-reads the head's weights (1.1 MB for enc_adapter)
// from L2 / Infinity Cache for its 16 rows.
#include "common.h"

// ---- tunables: each may be overridden for an A/B build with make EXTRA=-DCVAE_<NAME>=<n> (CVAE_TUNABLE, common.h) ----
CVAE_TUNABLE(HEADS_NC, 128);            // output columns per weight tile = threads per row group
CVAE_TUNABLE(HEADS_KC, 128);            // inputs per weight tile (a multiple of 64: the tile's write lanes then stay inside one column)
CVAE_TUNABLE(HEADS_RG, 4);              // row groups per workgroup (threads = HEADS_NC * HEADS_RG)
CVAE_TUNABLE(HEADS_RPT, 4);             // batch rows per thread (rows per workgroup = HEADS_RG * HEADS_RPT)

namespace {
constexpr int NC = (int)HEADS_NC, KC = (int)HEADS_KC, RG = (int)HEADS_RG, RPT = (int)HEADS_RPT;
constexpr int THREADS = NC * RG, ROWS = RG * RPT, WST = KC + 1, AST = CVAE_HEADS_MAX_WIDTH + 4, PF = NC * KC / THREADS;
static_assert(KC % 64 == 0 && NC % 64 == 0 && THREADS <= 1024 && (NC * KC) % THREADS == 0, "heads.hip: tile shape");
constexpr size_t LDS_BYTES = (size_t)(NC * WST + 2 * ROWS * AST) * sizeof(float);
static_assert(LDS_BYTES <= 160 * 1024, "heads.hip: a workgroup's LDS");

struct HeadsArgs {
    cvae_heads_panel panels[CVAE_HEADS_MAX_PANELS];
    cvae_heads_layer layers[CVAE_HEADS_MAX_LAYERS];
    int n_panels, n_layers;
    int64_t split, B;
    int clamp0, clamp1;
    float lo0, hi0, lo1, hi1;
    const float* eps;
    int64_t eps_stride;
    float *out0, *out1, *z;
    int64_t out0_stride, out1_stride, z_stride;
};

// the registers of one weight tile: columns n0 .. n0 + NC - 1, inputs k0 .. k0 + KC - 1, zero outside the layer
__device__ __forceinline__ void tile_fetch(float (&reg)[PF], const cvae_heads_layer& L, int K, int N, int n0, int k0) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int e = i * THREADS + (int)threadIdx.x, row = e / KC, k = k0 + e % KC, n = n0 + row;
        float v = 0.f;
        if (n < N && k < K) v = (n < L.out_first) ? L.W[(int64_t)n * K + k] : L.W2[(int64_t)(n - L.out_first) * K + k];
        reg[i] = v;
    }
}

// torch.clamp: NaN passes
__device__ __forceinline__ float clamp_f32(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(THREADS) void mlp_heads_kernel(const HeadsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Wt = lds;
    float* const buf0 = lds + NC * WST;          // activation buffer i = buf0 + i * ROWS * AST
    const int tid = (int)threadIdx.x, c = tid % NC, g = __builtin_amdgcn_readfirstlane(tid / NC);      // NC % 64 == 0: a wave sits in one row group
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    // rows of this thread's group that exist: the others are skipped in the product loops (a forward brings 1..8 rows to a 16-row workgroup; their waves then
    // only help moving the weight tiles).  A row that exists runs the same fmaf chain whatever the others do.
    const int nr = (int)max((int64_t)0, min((int64_t)RPT, a.B - row0 - (int64_t)g * RPT));

    // the concatenated input rows -> activation buffer 0 (rows past the batch: zeros), zero columns up to the next multiple of 4
    int K = 0;
    for (int p = 0; p < a.n_panels; ++p) {
        const int w = (int)a.panels[p].width;
        for (int idx = tid; idx < ROWS * w; idx += THREADS) {
            const int r = idx / w, j = idx % w;
            buf0[r * AST + K + j] = (row0 + r < a.B) ? a.panels[p].ptr[(row0 + r) * a.panels[p].stride + j] : 0.f;
        }
        K += w;
    }
    for (int idx = tid; idx < ROWS * 4; idx += THREADS)
        if (K + idx % 4 < ((K + 3) & ~3)) buf0[(idx / 4) * AST + K + idx % 4] = 0.f;

    for (int l = 0; l < a.n_layers; ++l) {
        const cvae_heads_layer& L = a.layers[l];
        const int N = (int)L.out, nk = (K + KC - 1) / KC, nt = (N + NC - 1) / NC, T = nt * nk;
        const float* hin = buf0 + (l & 1) * ROWS * AST;
        float* hout = buf0 + ((l + 1) & 1) * ROWS * AST;
        const bool last = l == a.n_layers - 1;
        float reg[PF], acc[RPT];
        tile_fetch(reg, L, K, N, 0, 0);
        for (int ti = 0; ti < T; ++ti) {
            const int n0 = (ti / nk) * NC, k0 = (ti % nk) * KC;
            __syncthreads();                       // the previous tile's products are done with Wt (first tile: the layer's input rows are complete)
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int e = i * THREADS + tid;
                Wt[(e / KC) * WST + e % KC] = reg[i];
            }
            __syncthreads();
            if (ti + 1 < T) tile_fetch(reg, L, K, N, ((ti + 1) / nk) * NC, ((ti + 1) % nk) * KC);
            if (k0 == 0) {
#pragma unroll
                for (int r = 0; r < RPT; ++r) acc[r] = 0.f;
            }
            const int kc4 = (min(KC, K - k0) + 3) & ~3;          // the tile's weights and the rows' columns are zero between K and its multiple of 4
            const float* wrow = Wt + c * WST;
            const float* hrow = hin + (g * RPT) * AST + k0;
            for (int k = 0; k < (nr > 0 ? kc4 : 0); k += 4) {
                const float w0 = wrow[k], w1 = wrow[k + 1], w2 = wrow[k + 2], w3 = wrow[k + 3];
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    if (r >= nr) break;
                    const float4 h = *reinterpret_cast<const float4*>(hrow + r * AST + k);
                    acc[r] = fmaf(w0, h.x, acc[r]);
                    acc[r] = fmaf(w1, h.y, acc[r]);
                    acc[r] = fmaf(w2, h.z, acc[r]);
                    acc[r] = fmaf(w3, h.w, acc[r]);
                }
            }
            if (k0 + KC >= K) {                    // the column's sums are complete: bias, BatchNorm1d, LeakyReLU, clamp
                const int n = n0 + c;
                if (n < N) {
                    const float bias = (n < L.out_first) ? L.b[n] : L.b2[n - L.out_first];
                    float scale = 1.f, mean = 0.f, beta = 0.f;
                    if (L.bn_var) {
                        scale = L.bn_weight[n] * (1.f / sqrtf(L.bn_var[n] + L.bn_eps));
                        mean = L.bn_mean[n];
                        beta = L.bn_bias[n];
                    }
#pragma unroll
                    for (int r = 0; r < RPT; ++r) {
                        float v = acc[r] + bias;
                        if (L.bn_var) v = fmaf(v - mean, scale, beta);
                        if (L.leaky) v = v > 0.f ? v : L.slope * v;
                        if (last) {
                            if (n < a.split) { if (a.clamp0) v = clamp_f32(v, a.lo0, a.hi0); }
                            else if (a.clamp1) v = clamp_f32(v, a.lo1, a.hi1);
                        }
                        hout[(g * RPT + r) * AST + n] = v;
                    }
                }
            }
        }
        for (int idx = tid; idx < ROWS * 4; idx += THREADS)
            if (N + idx % 4 < ((N + 3) & ~3)) hout[(idx / 4) * AST + N + idx % 4] = 0.f;
        K = N;
    }
    __syncthreads();

    // the outputs, rows along the lanes' slow index: coalesced stores
    const float* res = buf0 + (a.n_layers & 1) * ROWS * AST;
    const int N = K, S = (int)a.split;
    for (int idx = tid; idx < ROWS * N; idx += THREADS) {
        const int r = idx / N, n = idx % N;
        if (row0 + r >= a.B) break;
        const float v = res[r * AST + n];
        if (n < S) a.out0[(row0 + r) * a.out0_stride + n] = v;
        else a.out1[(row0 + r) * a.out1_stride + (n - S)] = v;
    }
    if (a.z) {
        for (int idx = tid; idx < ROWS * S; idx += THREADS) {
            const int r = idx / S, n = idx % S;
            if (row0 + r >= a.B) break;
            const float e = a.eps[(row0 + r) * a.eps_stride + n];
            a.z[(row0 + r) * a.z_stride + n] = fmaf(e, expf(0.5f * res[r * AST + S + n]), res[r * AST + n]);
        }
    }
}
}  // namespace

extern "C" int cvae_mlp_heads_fwd(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t split,
                                  const float* clamp0, const float* clamp1, const float* eps, int64_t eps_stride, float* out0, int64_t out0_stride,
                                  float* out1, int64_t out1_stride, float* z, int64_t z_stride, int64_t B, void* stream) {
    if (n_panels < 1 || n_panels > CVAE_HEADS_MAX_PANELS || n_layers < 1 || n_layers > CVAE_HEADS_MAX_LAYERS) return CVAE_E_UNSUPPORTED;
    if (!panels || !layers) return CVAE_E_NULLPTR;
    if (B < 0 || B > ((int64_t)1 << 24)) return CVAE_E_BADSHAPE;
    HeadsArgs a = {};
    int64_t K = 0;
    for (int p = 0; p < n_panels; ++p) {
        if (panels[p].width < 1 || panels[p].stride < panels[p].width) return CVAE_E_BADSHAPE;
        a.panels[p] = panels[p];
        K += panels[p].width;
    }
    if (K > CVAE_HEADS_MAX_WIDTH) return CVAE_E_UNSUPPORTED;
    for (int l = 0; l < n_layers; ++l) {
        const cvae_heads_layer& L = layers[l];
        if (L.out < 1 || L.out > CVAE_HEADS_MAX_WIDTH) return CVAE_E_UNSUPPORTED;
        if (L.out_first < 1 || L.out_first > L.out) return CVAE_E_BADSHAPE;
        if (L.out_first < L.out && l != n_layers - 1) return CVAE_E_UNSUPPORTED;         // two weight tensors: the last layer's column halves only
        a.layers[l] = L;
    }
    const int64_t N = layers[n_layers - 1].out;
    if (split < 1 || split > N || (z && 2 * split != N)) return CVAE_E_BADSHAPE;
    if (out0_stride < split || (split < N && out1_stride < N - split) || (z && (z_stride < split || eps_stride < split))) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    for (int p = 0; p < n_panels; ++p)
        if (!panels[p].ptr) return CVAE_E_NULLPTR;
    for (int l = 0; l < n_layers; ++l) {
        const cvae_heads_layer& L = layers[l];
        if (!L.W || !L.b || (L.out_first < L.out && (!L.W2 || !L.b2))) return CVAE_E_NULLPTR;
        if (L.bn_var && (!L.bn_weight || !L.bn_bias || !L.bn_mean)) return CVAE_E_NULLPTR;
    }
    if (!out0 || (split < N && !out1) || (z && !eps)) return CVAE_E_NULLPTR;
    a.n_panels = n_panels; a.n_layers = n_layers; a.split = split; a.B = B;
    if (clamp0) { a.clamp0 = 1; a.lo0 = clamp0[0]; a.hi0 = clamp0[1]; }
    if (clamp1) { a.clamp1 = 1; a.lo1 = clamp1[0]; a.hi1 = clamp1[1]; }
    a.eps = eps; a.eps_stride = eps_stride;
    a.out0 = out0; a.out1 = out1; a.z = z;
    a.out0_stride = out0_stride; a.out1_stride = out1_stride; a.z_stride = z_stride;
    // on every call: the attribute belongs to the current device, and a flag kept here would be shared by every device and thread of the process
    if (hipFuncSetAttribute((const void*)mlp_heads_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES) != hipSuccess) return CVAE_E_LAUNCH;
    hipLaunchKernelGGL(mlp_heads_kernel, dim3((unsigned)((B + ROWS - 1) / ROWS)), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, a);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
