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
static_assert(LDS_BYTES <= CVAE_LDS_MAX, "heads.hip: a workgroup's LDS");

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

// ---- what the three entries check, once ----
// A layer counts as BatchNorm1d by bn_var in eval (running statistics are what eval needs) and by bn_weight in training and backward (batch statistics
// need none; gamma is what both have).
enum HeadsMode { HEADS_EVAL, HEADS_TRAIN, HEADS_BWD };
inline bool has_bn(const HeadsMode m, const cvae_heads_layer& L) { return m == HEADS_EVAL ? L.bn_var != nullptr : L.bn_weight != nullptr; }

// shapes and limits: refused before the B == 0 return, and by the workspace queries; *K0 receives the concatenated input width
int heads_check_shape(const HeadsMode m, const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t B, int64_t* K0) {
    if (n_panels < 1 || n_panels > CVAE_HEADS_MAX_PANELS || n_layers < 1 || n_layers > CVAE_HEADS_MAX_LAYERS) return CVAE_E_UNSUPPORTED;
    if (!panels || !layers) return CVAE_E_NULLPTR;
    if (B < 0 || B > ((int64_t)1 << 24)) return CVAE_E_BADSHAPE;
    int64_t K = 0;
    for (int p = 0; p < n_panels; ++p) {
        if (panels[p].width < 1 || panels[p].stride < panels[p].width) return CVAE_E_BADSHAPE;
        K += panels[p].width;
    }
    if (K > CVAE_HEADS_MAX_WIDTH) return CVAE_E_UNSUPPORTED;
    for (int l = 0; l < n_layers; ++l) {
        const cvae_heads_layer& L = layers[l];
        if (L.out < 1 || L.out > CVAE_HEADS_MAX_WIDTH) return CVAE_E_UNSUPPORTED;
        if (L.out_first < 1 || L.out_first > L.out) return CVAE_E_BADSHAPE;
        if (L.out_first < L.out && l != n_layers - 1) return CVAE_E_UNSUPPORTED;         // two weight tensors: the last layer's column halves only
        if (m == HEADS_EVAL) continue;
        if (l == n_layers - 1 && (L.bn_weight || L.leaky)) return CVAE_E_UNSUPPORTED;     // training: the output layer is a plain Linear
        if (L.bn_weight && B < 2) return CVAE_E_BADSHAPE;                                 // batch statistics of one row: torch raises too
    }
    *K0 = K;
    return CVAE_OK;
}

// HeadsArgs of a head whose shape passed, and the split and stride rules (still before the B == 0 return).  paired: z (forward) or its cotangent (backward)
// is wanted, which needs N == 2 split and eps; the backward passes no outputs.
int heads_fill(const HeadsMode m, HeadsArgs& a, const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t split,
               const float* clamp0, const float* clamp1, const float* eps, int64_t eps_stride, float* out0, int64_t out0_stride, float* out1,
               int64_t out1_stride, float* z, int64_t z_stride, int64_t B, bool paired) {
    const int64_t N = layers[n_layers - 1].out;
    if (split < 1 || split > N || (paired && 2 * split != N)) return CVAE_E_BADSHAPE;
    if (m != HEADS_BWD && (out0_stride < split || (split < N && out1_stride < N - split) || (z && z_stride < split))) return CVAE_E_BADSHAPE;
    if (paired && eps_stride < split) return CVAE_E_BADSHAPE;
    for (int p = 0; p < n_panels; ++p) a.panels[p] = panels[p];
    for (int l = 0; l < n_layers; ++l) a.layers[l] = layers[l];
    a.n_panels = n_panels; a.n_layers = n_layers; a.split = split; a.B = B;
    if (clamp0) { a.clamp0 = 1; a.lo0 = clamp0[0]; a.hi0 = clamp0[1]; }
    if (clamp1) { a.clamp1 = 1; a.lo1 = clamp1[0]; a.hi1 = clamp1[1]; }
    a.eps = eps; a.eps_stride = eps_stride;
    a.out0 = out0; a.out1 = out1; a.z = z;
    a.out0_stride = out0_stride; a.out1_stride = out1_stride; a.z_stride = z_stride;
    return CVAE_OK;
}

// the pointers a launch would read or write: checked after the B == 0 return
int heads_check_ptrs(const HeadsMode m, const HeadsArgs& a, bool paired) {
    for (int p = 0; p < a.n_panels; ++p)
        if (!a.panels[p].ptr) return CVAE_E_NULLPTR;
    for (int l = 0; l < a.n_layers; ++l) {
        const cvae_heads_layer& L = a.layers[l];
        if (!L.W || !L.b || (L.out_first < L.out && (!L.W2 || !L.b2))) return CVAE_E_NULLPTR;
        if (has_bn(m, L) && (!L.bn_weight || !L.bn_bias || (m == HEADS_EVAL && !L.bn_mean))) return CVAE_E_NULLPTR;
    }
    if (m != HEADS_BWD && (!a.out0 || (a.split < a.layers[a.n_layers - 1].out && !a.out1))) return CVAE_E_NULLPTR;
    return paired && !a.eps ? CVAE_E_NULLPTR : CVAE_OK;
}
}  // namespace

extern "C" int cvae_mlp_heads_fwd(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t split,
                                  const float* clamp0, const float* clamp1, const float* eps, int64_t eps_stride, float* out0, int64_t out0_stride,
                                  float* out1, int64_t out1_stride, float* z, int64_t z_stride, int64_t B, void* stream) {
    int64_t K0;
    HeadsArgs a = {};
    int rc = heads_check_shape(HEADS_EVAL, panels, n_panels, layers, n_layers, B, &K0);
    if (rc == CVAE_OK) rc = heads_fill(HEADS_EVAL, a, panels, n_panels, layers, n_layers, split, clamp0, clamp1, eps, eps_stride, out0, out0_stride, out1,
                                       out1_stride, z, z_stride, B, z != nullptr);
    if (rc != CVAE_OK || B == 0) return rc;
    if ((rc = heads_check_ptrs(HEADS_EVAL, a, z != nullptr)) != CVAE_OK) return rc;
    if (cvae_allow_lds<mlp_heads_kernel>(LDS_BYTES) != CVAE_OK) return CVAE_E_LAUNCH;
    hipLaunchKernelGGL(mlp_heads_kernel, dim3((unsigned)((B + ROWS - 1) / ROWS)), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, a);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

// ==== training mode: batch-statistics BatchNorm1d forward and the backward ==================================================================
// Forward: the eval kernel's walk (16 rows per workgroup, weight tiles through LDS, one fmaf chain per value) cut at every BatchNorm1d layer, because a
// column's statistics are sums over rows that live in different workgroups and a grid-wide dependency is a launch boundary here:
//   heads_train_rows_kernel(l_begin = 0)   panels -> Linear 0 .. : a BatchNorm layer's Linear output v goes to memory (the x^ slot) and the launch ends
//   heads_bn_stats_kernel                  one thread per column walks rows 0 .. B-1 twice (mean, then sum (v - mean)^2), writes mean and rstd, updates the
//                                          running statistics (unbiased variance) and num_batches_tracked
//   heads_train_rows_kernel(l_begin = l+1) normalises its rows in place (v -> x^), gamma x^ + beta, LeakyReLU, and carries on to the outputs
// Backward (heads_bwd_kernel, blocks of 256 threads with one of three roles per launch):
//   rows   16 rows per workgroup: the gated output cotangent g, then da = g W (thread k walks n in order, W read coalesced along k), the LeakyReLU gate from
//          the saved activation; it stops where a BatchNorm layer needs dgamma / dbeta (sums over all rows) and resumes there one launch later
//   wgrad  thread (k; 4 columns n): dW[n][k] = ONE fmaf chain over rows 0 .. B-1; db[n] one add chain over the rows
//   sums   thread n: dbeta = sum dy, dgamma = sum dy x^, rows in order
// No atomics, no cross-thread sums: every result's bits are independent of the grid and of timing.
namespace {
constexpr int BT = 256, WN = 4;            // backward: threads per workgroup, dW columns per thread

struct TrainLayout {                       // offsets in floats into the saved buffer; -1: the layer has no such slot
    int64_t mean[CVAE_HEADS_MAX_LAYERS], rstd[CVAE_HEADS_MAX_LAYERS], xhat[CVAE_HEADS_MAX_LAYERS], pre[CVAE_HEADS_MAX_LAYERS], act[CVAE_HEADS_MAX_LAYERS];
    int64_t preclamp, total;
};

TrainLayout train_layout(const cvae_heads_layer* layers, int n_layers, int64_t B) {
    TrainLayout t = {};
    int64_t o = 0;
    for (int l = 0; l < CVAE_HEADS_MAX_LAYERS; ++l) t.mean[l] = t.rstd[l] = t.xhat[l] = t.pre[l] = t.act[l] = -1;
    for (int l = 0; l + 1 < n_layers; ++l) {
        const int64_t N = layers[l].out;
        if (layers[l].bn_weight) { t.mean[l] = o; o += N; t.rstd[l] = o; o += N; t.xhat[l] = o; o += B * N; }
        t.pre[l] = o; o += B * N;
        t.act[l] = o; o += B * N;
    }
    t.preclamp = o; o += B * layers[n_layers - 1].out;
    t.total = o;
    return t;
}

struct TrainArgs {
    HeadsArgs h;
    cvae_heads_bn_train bn[CVAE_HEADS_MAX_LAYERS];
    float* saved;
    TrainLayout lay;
};

// acc + cmp += w h with the rounding errors of the product and of the sum kept in cmp (TwoProduct by fma, TwoSum; the _rn forms are never contracted): the
// Linear in front of a BatchNorm1d layer.  Batch statistics subtract nearly equal values — at B = 2, x^ = d / sqrt(d^2 + eps) with d = (v0 - v1) / 2, and
// the backward's dv = delta (1 - x^2) = delta eps / (d^2 + eps) lives on the columns where d is small — so the rounding error of v reaches the
// gradients amplified by |v| / |d|; a plain chain of K terms carries ~sqrt(K) u |v|, this sum ~u |v|.
__device__ __forceinline__ void comp_fma(const float w, const float h, float& acc, float& cmp) {
    const float p = __fmul_rn(w, h), ep = fmaf(w, h, -p);
    const float s = __fadd_rn(acc, p), bb = __fsub_rn(s, acc);
    const float es = __fadd_rn(__fsub_rn(acc, __fsub_rn(s, bb)), __fsub_rn(p, bb));
    acc = s;
    cmp = __fadd_rn(cmp, __fadd_rn(ep, es));
}

__global__ __launch_bounds__(THREADS) void heads_train_rows_kernel(const TrainArgs t, const int l_begin) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const HeadsArgs& a = t.h;
    float* Wt = lds;
    float* const buf0 = lds + NC * WST;
    const int tid = (int)threadIdx.x, c = tid % NC, g = __builtin_amdgcn_readfirstlane(tid / NC);
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int nr = (int)max((int64_t)0, min((int64_t)RPT, a.B - row0 - (int64_t)g * RPT));

    int K = 0;
    float* const in0 = buf0 + (l_begin & 1) * ROWS * AST;
    if (l_begin == 0) {
        for (int p = 0; p < a.n_panels; ++p) {
            const int w = (int)a.panels[p].width;
            for (int idx = tid; idx < ROWS * w; idx += THREADS) {
                const int r = idx / w, j = idx % w;
                in0[r * AST + K + j] = (row0 + r < a.B) ? a.panels[p].ptr[(row0 + r) * a.panels[p].stride + j] : 0.f;
            }
            K += w;
        }
    } else {                                       // resume behind a BatchNorm layer: v -> x^ in place, gamma x^ + beta, LeakyReLU
        const int lb = l_begin - 1;
        const cvae_heads_layer& L = a.layers[lb];
        K = (int)L.out;
        float* xh = t.saved + t.lay.xhat[lb];
        float* pre = t.saved + t.lay.pre[lb];
        float* act = t.saved + t.lay.act[lb];
        const float *mean = t.saved + t.lay.mean[lb], *rstd = t.saved + t.lay.rstd[lb];
        for (int idx = tid; idx < ROWS * K; idx += THREADS) {
            const int r = idx / K, n = idx % K;
            float y = 0.f;
            if (row0 + r < a.B) {
                const int64_t i = (row0 + r) * K + n;
                const float x = (xh[i] - mean[n]) * rstd[n];
                const float p = fmaf(x, L.bn_weight[n], L.bn_bias[n]);
                y = L.leaky ? (p > 0.f ? p : L.slope * p) : p;
                xh[i] = x; pre[i] = p; act[i] = y;
            }
            in0[r * AST + n] = y;
        }
    }
    for (int idx = tid; idx < ROWS * 4; idx += THREADS)
        if (K + idx % 4 < ((K + 3) & ~3)) in0[(idx / 4) * AST + K + idx % 4] = 0.f;

    for (int l = l_begin; l < a.n_layers; ++l) {
        const cvae_heads_layer& L = a.layers[l];
        const int N = (int)L.out, nk = (K + KC - 1) / KC, nt = (N + NC - 1) / NC, T = nt * nk;
        const float* hin = buf0 + (l & 1) * ROWS * AST;
        float* hout = buf0 + ((l + 1) & 1) * ROWS * AST;
        const bool last = l == a.n_layers - 1, bn = !last && L.bn_weight;
        float reg[PF], acc[RPT], cmp[RPT];
        tile_fetch(reg, L, K, N, 0, 0);
        for (int ti = 0; ti < T; ++ti) {
            const int n0 = (ti / nk) * NC, k0 = (ti % nk) * KC;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int e = i * THREADS + tid;
                Wt[(e / KC) * WST + e % KC] = reg[i];
            }
            __syncthreads();
            if (ti + 1 < T) tile_fetch(reg, L, K, N, ((ti + 1) / nk) * NC, ((ti + 1) % nk) * KC);
            if (k0 == 0) {
#pragma unroll
                for (int r = 0; r < RPT; ++r) acc[r] = cmp[r] = 0.f;
            }
            const int kc4 = (min(KC, K - k0) + 3) & ~3;
            const float* wrow = Wt + c * WST;
            const float* hrow = hin + (g * RPT) * AST + k0;
            if (bn) {                              // in front of batch statistics: the compensated sum (comp_fma)
                for (int k = 0; k < (nr > 0 ? kc4 : 0); k += 4) {
                    const float w0 = wrow[k], w1 = wrow[k + 1], w2 = wrow[k + 2], w3 = wrow[k + 3];
#pragma unroll
                    for (int r = 0; r < RPT; ++r) {
                        if (r >= nr) break;
                        const float4 h = *reinterpret_cast<const float4*>(hrow + r * AST + k);
                        comp_fma(w0, h.x, acc[r], cmp[r]);
                        comp_fma(w1, h.y, acc[r], cmp[r]);
                        comp_fma(w2, h.z, acc[r], cmp[r]);
                        comp_fma(w3, h.w, acc[r], cmp[r]);
                    }
                }
            } else
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
            if (k0 + KC >= K) {
                const int n = n0 + c;
                if (n < N) {
                    const float bias = (n < L.out_first) ? L.b[n] : L.b2[n - L.out_first];
#pragma unroll
                    for (int r = 0; r < RPT; ++r) {
                        const bool live = r < nr;
                        const int64_t i = (row0 + g * RPT + r) * N + n;
                        float v = bn ? acc[r] + (cmp[r] + bias) : acc[r] + bias;
                        if (bn) {                              // the Linear output waits in the x^ slot for the statistics
                            if (live) t.saved[t.lay.xhat[l] + i] = v;
                        } else if (!last) {
                            if (live) t.saved[t.lay.pre[l] + i] = v;
                            if (L.leaky) v = v > 0.f ? v : L.slope * v;
                            if (live) t.saved[t.lay.act[l] + i] = v;
                        } else {
                            if (live) t.saved[t.lay.preclamp + i] = v;
                            if (n < a.split) { if (a.clamp0) v = clamp_f32(v, a.lo0, a.hi0); }
                            else if (a.clamp1) v = clamp_f32(v, a.lo1, a.hi1);
                        }
                        hout[(g * RPT + r) * AST + n] = v;
                    }
                }
            }
        }
        if (bn) return;                                        // uniform: the statistics launch and the resuming launch follow
        for (int idx = tid; idx < ROWS * 4; idx += THREADS)
            if (N + idx % 4 < ((N + 3) & ~3)) hout[(idx / 4) * AST + N + idx % 4] = 0.f;
        K = N;
    }
    __syncthreads();

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

// one thread owns a column and walks the rows in row order, twice: the bits do not depend on the grid
__global__ __launch_bounds__(64) void heads_bn_stats_kernel(const float* __restrict__ v, const int64_t B, const int N, const float eps, float* __restrict__ mean,
                                                            float* __restrict__ rstd, const cvae_heads_bn_train st) {
    const int n = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (n >= N) return;
    float s = 0.f;
    for (int64_t r = 0; r < B; ++r) s += v[r * N + n];
    const float m = s / (float)B;
    float q = 0.f;
    for (int64_t r = 0; r < B; ++r) {
        const float d = v[r * N + n] - m;
        q = fmaf(d, d, q);
    }
    mean[n] = m;
    rstd[n] = 1.f / sqrtf(q / (float)B + eps);
    if (st.running_mean) st.running_mean[n] = fmaf(st.momentum, m, (1.f - st.momentum) * st.running_mean[n]);
    if (st.running_var) st.running_var[n] = fmaf(st.momentum, q / (float)(B - 1), (1.f - st.momentum) * st.running_var[n]);
    if (n == 0 && st.num_batches_tracked) *st.num_batches_tracked += 1;
}

struct BwdArgs {
    HeadsArgs h;                                   // panels, layers, split, clamps, eps; out0 / out1 / z are unused
    float* pgrad[CVAE_HEADS_MAX_PANELS];
    int64_t pgrad_stride[CVAE_HEADS_MAX_PANELS];
    cvae_heads_layer_grad grads[CVAE_HEADS_MAX_LAYERS];
    const float *g0, *g1, *gz;
    int64_t g0_stride, g1_stride, gz_stride;
    const float* saved;
    TrainLayout lay;
    float* ws;                                     // per layer [B][out]: the gradient with respect to the Linear output (a BatchNorm layer: to the BatchNorm output dy)
    int64_t goff[CVAE_HEADS_MAX_LAYERS];
    int K0;
    // this launch
    int top, n_row_blocks;                         // rows role: starts at layer `top` (n_row_blocks == 0: none)
    int wl_lo, wl_hi, fly;                         // wgrad role: layers wl_lo .. wl_hi; fly: wl_hi is a BatchNorm layer whose dv is formed from dy, x^ and the sums
    int sums;                                      // sums role: the BatchNorm layer whose dgamma / dbeta this launch writes, or -1
};

// the width of layer l's input; with wgrad_items also what bwd_launch counts blocks by
__host__ __device__ __forceinline__ int in_width(const BwdArgs& a, int l) { return l == 0 ? a.K0 : (int)a.h.layers[l - 1].out; }

// the input of layer l, row r, column k
__device__ __forceinline__ float layer_input(const BwdArgs& a, int l, int64_t r, int k) {
    if (l > 0) return a.saved[a.lay.act[l - 1] + r * a.h.layers[l - 1].out + k];
    int p = 0;
    while (k >= (int)a.h.panels[p].width) { k -= (int)a.h.panels[p].width; ++p; }
    return a.h.panels[p].ptr[r * a.h.panels[p].stride + k];
}

// training-mode BatchNorm backward for one element: dv = gamma rstd (dy - dbeta / B - x^ dgamma / B), the sums read from the gradient tensors
__device__ __forceinline__ float bn_dv(const BwdArgs& a, int l, int64_t r, int n) {
    const int64_t i = r * a.h.layers[l].out + n;
    const float invB = 1.f / (float)a.h.B;
    const float dy = a.ws[a.goff[l] + i], x = a.saved[a.lay.xhat[l] + i];
    float u = dy - a.grads[l].dbeta[n] * invB;
    u = fmaf(-x, a.grads[l].dgamma[n] * invB, u);
    return a.h.layers[l].bn_weight[n] * a.saved[a.lay.rstd[l] + n] * u;
}

__device__ __forceinline__ float layer_grad(const BwdArgs& a, int l, bool fly, int64_t r, int n) {
    return fly ? bn_dv(a, l, r, n) : a.ws[a.goff[l] + r * a.h.layers[l].out + n];
}

__device__ void bwd_rows(const BwdArgs& a, float* lds, const int blk) {
    const HeadsArgs& h = a.h;
    const int tid = (int)threadIdx.x, L1 = h.n_layers - 1;
    const int64_t row0 = (int64_t)blk * ROWS;
    const int rows = (int)min((int64_t)ROWS, h.B - row0);
    float* gbuf = lds;
    float* nbuf = lds + ROWS * AST;
    {   // the gradient with respect to layer top's Linear output, rows past the batch zero
        const int N = (int)h.layers[a.top].out, S = (int)h.split;
        for (int idx = tid; idx < ROWS * N; idx += BT) {
            const int r = idx / N, n = idx % N;
            float g = 0.f;
            if (r < rows) {
                const int64_t R = row0 + r;
                if (a.top != L1) g = bn_dv(a, a.top, R, n);
                else {
                    const float pc = a.saved[a.lay.preclamp + R * N + n];
                    if (n < S) {
                        if (a.g0) g = a.g0[R * a.g0_stride + n];
                        if (a.gz) g += a.gz[R * a.gz_stride + n];
                        if (h.clamp0 && !(pc >= h.lo0 && pc <= h.hi0)) g = 0.f;
                    } else {
                        const int j = n - S;
                        if (a.g1) g = a.g1[R * a.g1_stride + j];
                        if (a.gz) {
                            const float lv = h.clamp1 ? clamp_f32(pc, h.lo1, h.hi1) : pc;
                            g = fmaf(a.gz[R * a.gz_stride + j] * h.eps[R * h.eps_stride + j], 0.5f * expf(0.5f * lv), g);
                        }
                        if (h.clamp1 && !(pc >= h.lo1 && pc <= h.hi1)) g = 0.f;
                    }
                    a.ws[a.goff[L1] + R * N + n] = g;
                }
            }
            gbuf[r * AST + n] = g;
        }
    }
    for (int l = a.top; l >= 0; --l) {
        __syncthreads();
        const cvae_heads_layer& L = h.layers[l];
        const int N = (int)L.out, K = in_width(a, l), N4 = N & ~3;
        if (l == 0) {
            bool any = false;
            for (int p = 0; p < h.n_panels; ++p) any = any || a.pgrad[p];
            if (!any) return;
        }
        for (int k = tid; k < K; k += BT) {
            int p = 0, kp = k;
            if (l == 0) {
                while (kp >= (int)h.panels[p].width) { kp -= (int)h.panels[p].width; ++p; }
                if (!a.pgrad[p]) continue;
            }
            float acc[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
            for (int n = 0; n < N4; n += 4) {
                float w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = (n + j < L.out_first) ? L.W[(int64_t)(n + j) * K + k] : L.W2[(int64_t)(n + j - L.out_first) * K + k];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const float4 g = *reinterpret_cast<const float4*>(gbuf + r * AST + n);
                    acc[r] = fmaf(g.x, w[0], acc[r]);
                    acc[r] = fmaf(g.y, w[1], acc[r]);
                    acc[r] = fmaf(g.z, w[2], acc[r]);
                    acc[r] = fmaf(g.w, w[3], acc[r]);
                }
            }
            for (int n = N4; n < N; ++n) {
                const float w = (n < L.out_first) ? L.W[(int64_t)n * K + k] : L.W2[(int64_t)(n - L.out_first) * K + k];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) acc[r] = fmaf(gbuf[r * AST + n], w, acc[r]);
            }
            if (l == 0) {
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
                    if (r < rows) a.pgrad[p][(row0 + r) * a.pgrad_stride[p] + kp] = acc[r];
            } else {
                const cvae_heads_layer& P = h.layers[l - 1];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    float d = 0.f;
                    if (r < rows) {
                        const int64_t i = (row0 + r) * K + k;
                        d = acc[r];
                        if (P.leaky && !(a.saved[a.lay.act[l - 1] + i] > 0.f)) d *= P.slope;
                        a.ws[a.goff[l - 1] + i] = d;
                    }
                    nbuf[r * AST + k] = d;
                }
            }
        }
        if (l == 0 || h.layers[l - 1].bn_weight) return;       // a BatchNorm layer's dy waits in memory for dgamma and dbeta
        float* s = gbuf; gbuf = nbuf; nbuf = s;
    }
}

__device__ void bwd_wgrad(const BwdArgs& a, const int l, const bool fly, const int item) {
    const cvae_heads_layer& L = a.h.layers[l];
    const int N = (int)L.out, K = in_width(a, l), kt = (K + BT - 1) / BT;
    const int n0 = (item / kt) * WN, k = (item % kt) * BT + (int)threadIdx.x;
    float acc[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) acc[j] = 0.f;
    for (int64_t r = 0; r < a.h.B; ++r) {
        const float x = k < K ? layer_input(a, l, r, k) : 0.f;
#pragma unroll
        for (int j = 0; j < WN; ++j)
            if (n0 + j < N) acc[j] = fmaf(layer_grad(a, l, fly, r, n0 + j), x, acc[j]);
    }
    if (k < K) {
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int n = n0 + j;
            if (n >= N) break;
            if (n < L.out_first) a.grads[l].dW[(int64_t)n * K + k] = acc[j];
            else a.grads[l].dW2[(int64_t)(n - L.out_first) * K + k] = acc[j];
        }
    }
    if (item % kt == 0 && (int)threadIdx.x < WN && n0 + (int)threadIdx.x < N) {
        const int n = n0 + (int)threadIdx.x;
        float s = 0.f;
        for (int64_t r = 0; r < a.h.B; ++r) s += layer_grad(a, l, fly, r, n);
        if (n < L.out_first) a.grads[l].db[n] = s;
        else a.grads[l].db2[n - L.out_first] = s;
    }
}

__host__ __device__ __forceinline__ int wgrad_items(const BwdArgs& a, int l) { return (((int)a.h.layers[l].out + WN - 1) / WN) * ((in_width(a, l) + BT - 1) / BT); }

__global__ __launch_bounds__(BT) void heads_bwd_kernel(const BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int blk = (int)blockIdx.x;                     // uniform: a workgroup has one role
    if (blk < a.n_row_blocks) { bwd_rows(a, lds, blk); return; }
    blk -= a.n_row_blocks;
    for (int l = a.wl_lo; l <= a.wl_hi; ++l) {
        const int items = wgrad_items(a, l);
        if (blk < items) { bwd_wgrad(a, l, a.fly && l == a.wl_hi, blk); return; }
        blk -= items;
    }
    if (a.sums >= 0) {
        const int N = (int)a.h.layers[a.sums].out, n = blk * BT + (int)threadIdx.x;
        if (n >= N) return;
        const float *dy = a.ws + a.goff[a.sums], *x = a.saved + a.lay.xhat[a.sums];
        float sb = 0.f, sg = 0.f;
        for (int64_t r = 0; r < a.h.B; ++r) {
            const float d = dy[r * N + n];
            sb += d;
            sg = fmaf(d, x[r * N + n], sg);
        }
        a.grads[a.sums].dbeta[n] = sb;
        a.grads[a.sums].dgamma[n] = sg;
    }
}
constexpr size_t BWD_LDS = (size_t)2 * ROWS * AST * sizeof(float);

int bwd_launch(BwdArgs& a, hipStream_t stream) {
    unsigned blocks = (unsigned)a.n_row_blocks;
    for (int l = a.wl_lo; l <= a.wl_hi; ++l) blocks += (unsigned)wgrad_items(a, l);
    if (a.sums >= 0) blocks += (unsigned)(((int)a.h.layers[a.sums].out + BT - 1) / BT);
    if (!blocks) return CVAE_OK;
    hipLaunchKernelGGL(heads_bwd_kernel, dim3(blocks), dim3(BT), BWD_LDS, stream, a);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
}  // namespace

extern "C" size_t cvae_mlp_heads_train_workspace_bytes(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t B) {
    int64_t K0;
    if (heads_check_shape(HEADS_TRAIN, panels, n_panels, layers, n_layers, B, &K0) != CVAE_OK) return 0;
    return (size_t)train_layout(layers, n_layers, B).total * sizeof(float);
}

extern "C" size_t cvae_mlp_heads_bwd_workspace_bytes(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t B) {
    int64_t K0, o = 0;
    if (heads_check_shape(HEADS_BWD, panels, n_panels, layers, n_layers, B, &K0) != CVAE_OK) return 0;
    for (int l = 0; l < n_layers; ++l) o += B * layers[l].out;
    return (size_t)o * sizeof(float);
}

extern "C" int cvae_mlp_heads_train_fwd(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, const cvae_heads_bn_train* bn,
                                        int64_t split, const float* clamp0, const float* clamp1, const float* eps, int64_t eps_stride, float* out0,
                                        int64_t out0_stride, float* out1, int64_t out1_stride, float* z, int64_t z_stride, int64_t B, void* saved,
                                        size_t saved_bytes, void* stream) {
    int64_t K0;
    TrainArgs t = {};
    int rc = heads_check_shape(HEADS_TRAIN, panels, n_panels, layers, n_layers, B, &K0);
    if (rc == CVAE_OK) rc = heads_fill(HEADS_TRAIN, t.h, panels, n_panels, layers, n_layers, split, clamp0, clamp1, eps, eps_stride, out0, out0_stride, out1,
                                       out1_stride, z, z_stride, B, z != nullptr);
    if (rc != CVAE_OK || B == 0) return rc;
    if ((rc = heads_check_ptrs(HEADS_TRAIN, t.h, z != nullptr)) != CVAE_OK) return rc;
    for (int l = 0; l < n_layers; ++l) {
        if (!layers[l].bn_weight) continue;
        if (!bn) return CVAE_E_NULLPTR;
        t.bn[l] = bn[l];
    }
    if (!saved) return CVAE_E_NULLPTR;
    t.lay = train_layout(layers, n_layers, B);
    if (saved_bytes < (size_t)t.lay.total * sizeof(float)) return CVAE_E_WORKSPACE;
    t.saved = (float*)saved;
    if (cvae_allow_lds<heads_train_rows_kernel>(LDS_BYTES) != CVAE_OK) return CVAE_E_LAUNCH;
    const dim3 grid((unsigned)((B + ROWS - 1) / ROWS));
    for (int l_begin = 0;;) {
        hipLaunchKernelGGL(heads_train_rows_kernel, grid, dim3(THREADS), LDS_BYTES, (hipStream_t)stream, t, l_begin);
        CVAE_CHECK_LAUNCH();
        int l = l_begin;
        while (l < n_layers - 1 && !layers[l].bn_weight) ++l;
        if (l >= n_layers - 1) break;
        const int Nl = (int)layers[l].out;
        hipLaunchKernelGGL(heads_bn_stats_kernel, dim3((unsigned)((Nl + 63) / 64)), dim3(64), 0, (hipStream_t)stream, t.saved + t.lay.xhat[l], B, Nl,
                           layers[l].bn_eps, t.saved + t.lay.mean[l], t.saved + t.lay.rstd[l], t.bn[l]);
        CVAE_CHECK_LAUNCH();
        l_begin = l + 1;
    }
    return CVAE_OK;
}

extern "C" int cvae_mlp_heads_bwd(const cvae_heads_panel* panels, int n_panels, float* const* panel_grads, const int64_t* panel_grad_strides,
                                  const cvae_heads_layer* layers, int n_layers, const cvae_heads_layer_grad* grads, int64_t split, const float* clamp0,
                                  const float* clamp1, const float* eps, int64_t eps_stride, const float* g0, int64_t g0_stride, const float* g1,
                                  int64_t g1_stride, const float* gz, int64_t gz_stride, int64_t B, const void* saved, size_t saved_bytes, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    int64_t K0;
    BwdArgs a = {};
    HeadsArgs& h = a.h;
    int rc = heads_check_shape(HEADS_BWD, panels, n_panels, layers, n_layers, B, &K0);
    if (rc != CVAE_OK) return rc;
    if (!grads) return CVAE_E_NULLPTR;
    rc = heads_fill(HEADS_BWD, h, panels, n_panels, layers, n_layers, split, clamp0, clamp1, eps, eps_stride, nullptr, 0, nullptr, 0, nullptr, 0, B, gz != nullptr);
    if (rc != CVAE_OK) return rc;
    if ((g0 && g0_stride < split) || (g1 && g1_stride < layers[n_layers - 1].out - split) || (gz && gz_stride < split)) return CVAE_E_BADSHAPE;
    for (int p = 0; p < n_panels; ++p)
        if (panel_grads && panel_grads[p] && (!panel_grad_strides || panel_grad_strides[p] < panels[p].width)) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if ((rc = heads_check_ptrs(HEADS_BWD, h, gz != nullptr)) != CVAE_OK) return rc;
    for (int p = 0; p < n_panels; ++p)
        if (panel_grads && panel_grads[p]) { a.pgrad[p] = panel_grads[p]; a.pgrad_stride[p] = panel_grad_strides[p]; }
    int64_t o = 0;
    for (int l = 0; l < n_layers; ++l) {
        const cvae_heads_layer& L = layers[l];
        const cvae_heads_layer_grad& G = grads[l];
        if (!G.dW || !G.db || (L.out_first < L.out && (!G.dW2 || !G.db2)) || (L.bn_weight && (!G.dgamma || !G.dbeta))) return CVAE_E_NULLPTR;
        a.grads[l] = G;
        a.goff[l] = o;
        o += B * L.out;
    }
    if (!saved || !workspace) return CVAE_E_NULLPTR;
    a.lay = train_layout(layers, n_layers, B);
    if (saved_bytes < (size_t)a.lay.total * sizeof(float) || workspace_bytes < (size_t)o * sizeof(float)) return CVAE_E_WORKSPACE;
    a.saved = (const float*)saved; a.ws = (float*)workspace; a.K0 = (int)K0;
    a.g0 = g0; a.g1 = g1; a.gz = gz; a.g0_stride = g0_stride; a.g1_stride = g1_stride; a.gz_stride = gz_stride;
    if (cvae_allow_lds<heads_bwd_kernel>(BWD_LDS) != CVAE_OK) return CVAE_E_LAUNCH;
    const int row_blocks = (int)((B + ROWS - 1) / ROWS);
    // segments between BatchNorm layers, from the output down: rows (top) [+ the wgrad of `top` with dv on the fly], then the wgrads below it and the next sums
    for (int top = n_layers - 1;;) {
        int s = top - 1;
        while (s >= 0 && !layers[s].bn_weight) --s;           // the rows role stops at BatchNorm layer s (-1: it reaches the panels)
        const bool fly = top != n_layers - 1;
        bool rows_work = !fly || s >= 0 || top > 0;           // the output segment forms the gated cotangent; below a BatchNorm layer 0 the rows role has the panel gradients only
        for (int p = 0; p < n_panels; ++p) rows_work = rows_work || a.pgrad[p];
        a.top = top; a.n_row_blocks = rows_work ? row_blocks : 0; a.sums = -1;
        a.wl_lo = fly ? top : 1; a.wl_hi = fly ? top : 0; a.fly = fly;
        int e = bwd_launch(a, (hipStream_t)stream);
        if (e != CVAE_OK) return e;
        a.n_row_blocks = 0; a.fly = 0; a.sums = s;
        a.wl_lo = s + 1; a.wl_hi = fly ? top - 1 : top;
        e = bwd_launch(a, (hipStream_t)stream);
        if (e != CVAE_OK) return e;
        if (s < 0) break;
        top = s;
    }
    return CVAE_OK;
}
