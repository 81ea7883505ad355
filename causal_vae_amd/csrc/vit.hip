// vit.hip — the transformer side of the ViT-VAE encoder in eval mode (vessel_analysis/00_core/vit_backbone.py:158-179 of the reference):
//   * token assembly: CLS + stem output + position embedding -> fp32 residual stream [B][N][256];
//   * LayerNorm(256): one wave per row, two-pass (mean, then squared deviations), xor-shuffle wave sums;
//   * token GEMM y = epi(x W^T + b) with epilogues none / exact-erf GELU / + residual, K <= 512 walked in LDS chunks (no split-K, no finish launch);
//   * fused multi-head self-attention (8 heads x 32): online softmax over 64-key tiles, scores never leave the registers.
// And its backward, for training the transformer in eval mode on a frozen stem (second half of the file): the training forms of attention (+ one
// fp32 row statistic) and of the GELU GEMM (+ the pre-activation), a recompute-style attention backward in two passes, the token GEMM's data and weight gradients,
// the LayerNorm backward and the token assembly's; slabs plus ordered finish launches wherever a sum crosses workgroups.
// The token GEMM's and the attention's forward kernels live in vit_gemm.inc / vit_attention.inc, each included three times: the inference kernel, its training form
// and the training form with dropout (Philox masks recomputed in registers, fp32 only); vit_gemm_bwd_data.inc and vit_attention_bwd.inc hold
// the two backward kernels that have a dropout form, each included twice.  The dropout forms take their Philox key by value or (the *_devkey entries, DESIGN.md
// section 19) read it from device memory at kernel entry, which is what lets a captured training step replay with a new key; vit_dropout_keys_step_kernel derives
// a step's keys from a device-resident counter and advances it.
// vit_attention_probe.inc holds the one forward-only kernel that looks inside: the attention probabilities the fused forward never writes,
// recomputed from q, k and the training forward's row statistic, stored (per head or head-averaged) or folded into one attention-rollout factor.
// vit_attention_grad_probe.inc is its counterpart on the backward's side: the gradient with respect to those probabilities, dO V^T, stored
// per head or folded with P into one step of gradient-weighted attention relevance, the query tiles split over workgroups and added by an ordered finish launch.
// Two arithmetic modes from one template: bf16 operands on v_mfma_f32_32x32x16_bf16, or exact fp32 on v_mfma_f32_32x32x2_f32 (the form the conv family uses
// for fp32); accumulation, softmax, LayerNorm statistics and the residual stream are fp32 in both.  No atomics anywhere: every sum has a fixed order,
// and an output element's bits do not depend on which other rows share its launch (row r of a one-row call equals row r of a full call: the CLS-only
// last block, n_query_rows).
//
// MFMA maps used throughout (lane l: r = l & 31, h = l >> 5): D[i][j] has column j = r on the lane and rows i = crow(e, h) = (e & 3) + 8 (e >> 2) + 4 h in
// its 16 registers e.  Every product is arranged so that the TOKEN (query) index is the column: a lane then owns one token's values, four consecutive
// features per register group — row-wise softmax needs one exchange with lane l ^ 32, and stores are 16-byte (fp32) / 8-byte (bf16) pieces along the features.
#include "common.h"

namespace {

#define VIT_DIM 256
#define VIT_HEADS 8
#define VIT_HD 32

__device__ __forceinline__ int crow(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------------------ dropout masks (include/cvae_hip.h)
// Counter-based: a mask element is a pure function of (key, site coordinates), recomputed in registers wherever it is needed, never stored.  One
// Philox4x32-10 call gives the words of four neighbouring elements; an element is kept iff (word >> 8) >= thr, and kept values are multiplied by scale.
struct DropArgs { uint32_t thr, k0, k1; float scale; };
__device__ __forceinline__ void drop_words(const DropArgs& d, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t w[4]) {
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = 0u;
    philox4x32_10(w[0], w[1], w[2], w[3], d.k0, d.k1);
}
__device__ __forceinline__ bool drop_keep(const DropArgs& d, uint32_t w) { return (w >> 8) >= d.thr; }
// row site: the words of columns c .. c + 3 (c % 4 == 0) of logical row R
__device__ __forceinline__ void drop_row_words(const DropArgs& d, int64_t R, int c, uint32_t w[4]) {
    drop_words(d, (uint32_t)(c >> 2), (uint32_t)R, (uint32_t)((uint64_t)R >> 32), w);
}
__device__ __forceinline__ void drop_apply4(const DropArgs& d, const uint32_t w[4], float v[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = drop_keep(d, w[e]) ? v[e] * d.scale : 0.f;
}
// attention site, one element: (batch b, head, query i, key j)
__device__ __forceinline__ bool drop_keep_attn(const DropArgs& d, uint32_t bh, uint32_t i, uint32_t j) {
    uint32_t w[4];
    drop_words(d, j >> 2, i, bh, w);
    const uint32_t s = j & 3;
    return drop_keep(d, s == 0 ? w[0] : (s == 1 ? w[1] : (s == 2 ? w[2] : w[3])));
}

// The key of a launch: the two words the entry passed by value, or (key_dev non-null: the *_devkey entries) the two words of the 64-bit key in
// device memory, low word first, read when the kernel runs — the same address in every lane, so one load per wave.
__device__ __forceinline__ DropArgs drop_with_key(DropArgs d, const uint32_t* __restrict__ key_dev) {
    if (key_dev) {
        d.k0 = key_dev[0];
        d.k1 = key_dev[1];
    }
    return d;
}

// y[m][c] = keep(R(m), c) ? x[m][c] * scale : 0 on fp32 rows: a thread per four columns
__global__ __launch_bounds__(256) void vit_dropout_rows_kernel(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t M, int N, const DropArgs drop_arg,
                                                               int64_t mask_row0, int64_t mask_row_step, const uint32_t* key_dev) {
    const DropArgs drop = drop_with_key(drop_arg, key_dev);
    const int n4 = N >> 2;
    const int64_t total = M * n4;
    for (int64_t g = blockIdx.x * (int64_t)256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t m = g / n4;
        const int c = (int)(g - m * n4) * 4;
        float v[4];
        uint32_t w[4];
        load_f32(x + m * ldx + c, v);
        drop_row_words(drop, mask_row0 + m * mask_row_step, c, w);
        drop_apply4(drop, w, v);
        store_from_f32(y + m * ldy + c, v);
    }
}

// The keys of one training step, derived where the counter lives (the rule of include/cvae_hip.h, which is ops.DropoutKeys.key):
// table[4 b + site] = splitmix64(base + (s << 20 | b << 4 | site)), s = *step mod 2^44 as the kernel finds it.  One workgroup: every thread reads s, the
// barrier orders those reads before the one store of s + 1, so a replayed graph walks the steps without the host.
__device__ __forceinline__ uint64_t splitmix64_dev(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void vit_dropout_keys_step_kernel(uint64_t base, int64_t* step, uint64_t* table, int n_blocks) {
    const uint64_t s = (uint64_t)*step & (((uint64_t)1 << 44) - 1);
    __syncthreads();
    if (threadIdx.x == 0) *step = (int64_t)(s + 1);
    for (int i = threadIdx.x; i < 4 * n_blocks; i += 256) table[i] = splitmix64_dev(base + (s << 20 | (uint64_t)(i >> 2) << 4 | (uint64_t)(i & 3)));
}

// ------------------------------------------------------------------------------------------------ token assembly
// tokens[b][0] = cls + pos[0]; tokens[b][1 + i] = stem[b][i] + pos[1 + i]  (torch.cat((cls, x), 1) + pos_embedding, one fp32 add per element)
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_kernel(const T* __restrict__ stem, const float* __restrict__ cls, const float* __restrict__ pos,
                                                         float* __restrict__ tokens, int64_t B, int64_t Np) {
    const int64_t total = B * (Np + 1) * (VIT_DIM / 4);
    for (int64_t g = blockIdx.x * (int64_t)256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(g & (VIT_DIM / 4 - 1));
        const int64_t row = g >> 6, b = row / (Np + 1), i = row - b * (Np + 1);
        float v[4], p[4];
        load_f32(pos + i * VIT_DIM + c4 * 4, p);
        if (i == 0) load_f32(cls + c4 * 4, v);
        else load_f32(stem + (b * Np + i - 1) * VIT_DIM + c4 * 4, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += p[e];
        store_from_f32(tokens + row * VIT_DIM + c4 * 4, v);
    }
}

// ------------------------------------------------------------------------------------------------ LayerNorm(256)
// one wave per row (4 elements per lane): mean, then the squared deviations from it (two-pass, as nn.LayerNorm), biased variance, 1 / sqrt(var + eps)
template <typename TO>
__global__ __launch_bounds__(256) void vit_layernorm_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, TO* __restrict__ y, int64_t rows, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[4], g[4], b[4];
    load_f32(x + row * ldx + lane * 4, v);
    load_f32(gamma + lane * 4, g);
    load_f32(beta + lane * 4, b);
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.f / VIT_DIM);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] -= mean;
    const float var = wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) * (1.f / VIT_DIM);
    const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] * rstd * g[e] + b[e];
    store_from_f32(y + row * VIT_DIM + lane * 4, v);
}

// ------------------------------------------------------------------------------------------------ token GEMM
// Workgroup tile: 128 tokens x 64 features, 4 waves of 32 tokens x 64 features (two accumulator tiles).  D = W x^T: A = the weight tile (rows = features),
// B = the activations (columns = tokens).  K is walked in chunks of 128 bytes per row (64 bf16 / 32 fp32); the next chunk's global loads are in flight
// while the MFMAs of the current one run.  W is the fp32 nn.Linear weight [N][K] as it is: rounded to bf16 on its way into LDS in bf16 mode.
#define GEMM_BM 128
#define GEMM_BN 64
#define GEMM_EPI_NONE 0
#define GEMM_EPI_GELU 1
#define GEMM_EPI_RESID 2
#define GEMM_EPI_GELU_SAVE 3                              // GELU, and the pre-activation stored next to it (the training forward: the backward's gate)

template <typename T> struct GemmGeom {
    static constexpr int KC = 128 / sizeof(T);            // k elements per chunk
    static constexpr int PITCH = KC + 16 / sizeof(T);     // LDS row pitch in elements: 144 bytes (16-byte aligned, rows 36 banks apart)
    static constexpr int E16 = 16 / sizeof(T);            // elements per 16-byte piece
    static constexpr int WP = KC / 16;                    // float4 pieces of W per thread and chunk
};

__device__ __forceinline__ void lds_put_w(bf16* dst, float4 w) { *(uint2*)dst = make_uint2(pack2_bf16(w.x, w.y), pack2_bf16(w.z, w.w)); }
__device__ __forceinline__ void lds_put_w(float* dst, float4 w) { *(float4*)dst = w; }

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

#define VIT_GEMM_KERNEL vit_gemm_kernel
#define VIT_GEMM_TRAIN 0
#include "vit_gemm.inc"
#undef VIT_GEMM_KERNEL
#undef VIT_GEMM_TRAIN
#define VIT_GEMM_KERNEL vit_gemm_train_kernel
#define VIT_GEMM_TRAIN 1
#include "vit_gemm.inc"
#undef VIT_GEMM_KERNEL
#undef VIT_GEMM_TRAIN
#define VIT_GEMM_KERNEL vit_gemm_dropout_kernel
#define VIT_GEMM_TRAIN 2
#include "vit_gemm.inc"
#undef VIT_GEMM_KERNEL
#undef VIT_GEMM_TRAIN

template <typename T>
int gemm_launch(const T* x, int64_t ldx, const float* W, const float* bias, const float* resid, int64_t ldr, void* y, int64_t ldy, int64_t M, int K, int N,
                int epi, void* prev, int64_t ldp, hipStream_t st) {
    const dim3 grid((unsigned)((M + GEMM_BM - 1) / GEMM_BM), (unsigned)(N / GEMM_BN));
    if (epi == GEMM_EPI_NONE) hipLaunchKernelGGL((vit_gemm_kernel<T, GEMM_EPI_NONE>), grid, dim3(256), 0, st, x, ldx, W, bias, resid, ldr, y, ldy, M, K, N);
    else if (epi == GEMM_EPI_GELU) hipLaunchKernelGGL((vit_gemm_kernel<T, GEMM_EPI_GELU>), grid, dim3(256), 0, st, x, ldx, W, bias, resid, ldr, y, ldy, M, K, N);
    else if (epi == GEMM_EPI_GELU_SAVE)
        hipLaunchKernelGGL((vit_gemm_train_kernel<T, GEMM_EPI_GELU_SAVE>), grid, dim3(256), 0, st, x, ldx, W, bias, resid, ldr, y, ldy, M, K, N, (T*)prev, ldp);
    else hipLaunchKernelGGL((vit_gemm_kernel<T, GEMM_EPI_RESID>), grid, dim3(256), 0, st, x, ldx, W, bias, resid, ldr, y, ldy, M, K, N);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

// ------------------------------------------------------------------------------------------------ fused attention
// Workgroup = 4 waves = 128 query rows of one (batch, head); a wave owns 32 rows.  K and V are staged per 64-key tile (two 32-key sub-tiles) in LDS, the next
// tile's global loads in flight during the current tile's arithmetic.  LDS per workgroup: bf16 64 x 80 B (K rows) + 32 x 144 B (V transposed: [d][key]) =
// 9.5 KiB; fp32 64 x 144 B + 64 x 160 B = 19 KiB.
//   S^T = K Q^T (A = K tile, B = Q): lane (r, h) holds, for query r, the scores of keys crow(e, h).  Row max / sum: in-lane over 16 registers, then one
//   exchange with lane l ^ 32.  Running max m, running sum l (per lane half, joined at the end), O rescaled by exp2(m_old - m_new) per tile.
//   O^T = V^T P^T (A = V^T, B = P): the score registers ARE the B operand (sum over their row index), so P never moves between lanes.  bf16: registers
//   8 s .. 8 s + 7 -> one bf16x8 fragment whose element j is key 16 s + 8 (j >> 2) + 4 h + (j & 3), matched by two 8-byte reads of the transposed V
//   tile.  P is rounded to bf16 there; the row sum l adds the unrounded fp32 values.  fp32: register e multiplies V[crow(e, h)][d = r], 16 32x32x2 steps.
// Keys past N get score -inf (P = 0) and their staged K / V rows are zeros.  Query rows past Nq are clamped on load and never stored.
#define ATT_KT 64
template <typename T> struct AttGeom;
template <> struct AttGeom<bf16> {
    static constexpr int KP = 40, VP = 72;                // K row pitch (80 B), V^T row pitch (144 B)
    static constexpr int KS = ATT_KT * KP, VS = VIT_HD * VP;
    static constexpr int NR = 1;                          // 16-byte pieces per thread, tensor and tile
};
template <> struct AttGeom<float> {
    static constexpr int KP = 36, VP = 40;                // K row pitch (144 B), V row pitch (160 B: the lane halves' rows 4 apart fall 32 banks apart)
    static constexpr int KS = ATT_KT * KP, VS = ATT_KT * VP;
    static constexpr int NR = 2;
};

#define VIT_ATT_KERNEL vit_attention_kernel
#define VIT_ATT_TRAIN 0
#include "vit_attention.inc"
#undef VIT_ATT_KERNEL
#undef VIT_ATT_TRAIN
#define VIT_ATT_KERNEL vit_attention_train_kernel
#define VIT_ATT_TRAIN 1
#include "vit_attention.inc"
#undef VIT_ATT_KERNEL
#undef VIT_ATT_TRAIN
#define VIT_ATT_KERNEL vit_attention_dropout_kernel
#define VIT_ATT_TRAIN 2
#include "vit_attention.inc"
#undef VIT_ATT_KERNEL
#undef VIT_ATT_TRAIN

// ================================================================================================ backward (training the transformer)
// Compensated (Kahan) running sum: the value is s - c.
__device__ __forceinline__ void kahan_add(float& s, float& c, float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// ------------------------------------------------------------------------------------------------ token assembly, backward
// dpos[i] = sum_b dtokens[b][i] (b in order), dcls = dpos[0], dstem[b][i] = dtokens[b][1 + i] (* act'(gate[b][i]) with a gate: the fp32 product, one
// rounding) in the stem's dtype.  The sums take the ungated values.
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_bwd_kernel(const float* __restrict__ dtok, float* __restrict__ dpos, float* __restrict__ dcls,
                                                             T* __restrict__ dstem, int64_t B, int64_t Np, const T* __restrict__ gate, float slope) {
    const int64_t total = (Np + 1) * (VIT_DIM / 4);
    for (int64_t g = blockIdx.x * (int64_t)256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(g & (VIT_DIM / 4 - 1));
        const int64_t i = g >> 6;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int64_t b = 0; b < B; ++b) {
            float v[4];
            load_f32(dtok + (b * (Np + 1) + i) * VIT_DIM + c4 * 4, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
            if (i > 0) {
                if (gate) {
                    float gt[4];
                    load_f32(gate + (b * Np + i - 1) * VIT_DIM + c4 * 4, gt);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= gt[e] > 0.f ? 1.f : slope;
                }
                store_from_f32(dstem + (b * Np + i - 1) * VIT_DIM + c4 * 4, v);
            }
        }
        store_from_f32(dpos + i * VIT_DIM + c4 * 4, s);
        if (i == 0) store_from_f32(dcls + c4 * 4, s);
    }
}

// ------------------------------------------------------------------------------------------------ LayerNorm(256), backward
// One wave per row, statistics recomputed two-pass from the saved fp32 input as the forward computes them: xh = (x - mean) rstd, a = gamma g,
// dx = rstd (a - mean(a) - xh mean(a xh)), written or added to dx.  dgamma = sum_rows g xh, dbeta = sum_rows g: a workgroup owns LN_SLAB rows (a wave adds its
// 8 rows in row order, the 4 waves are added in wave order) and leaves one partial row pair; vit_colsum_finish_kernel adds the partials in slab order.
#define LN_SLAB 32
template <typename TG>
__global__ __launch_bounds__(256) void vit_layernorm_bwd_kernel(const TG* __restrict__ g, int64_t ldg, const float* __restrict__ x, int64_t ldx,
                                                                const float* __restrict__ gamma, float* dx, int64_t lddx, float* __restrict__ part,
                                                                int64_t rows, float eps, int accumulate) {
    __shared__ float red[4][2][VIT_DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gm[4], dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    load_f32(gamma + lane * 4, gm);
    for (int i = 0; i < LN_SLAB / 4; ++i) {
        const int64_t row = blockIdx.x * (int64_t)LN_SLAB + wave + 4 * i;
        if (row >= rows) break;
        float v[4], gv[4], a[4];
        load_f32(x + row * ldx + lane * 4, v);
        load_f32(g + row * ldg + lane * 4, gv);
        const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.f / VIT_DIM);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] -= mean;
        const float var = wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) * (1.f / VIT_DIM);
        const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] *= rstd;
            a[e] = gm[e] * gv[e];
            dg[e] += gv[e] * v[e];
            db[e] += gv[e];
        }
        const float m1 = wave_sum((a[0] + a[1]) + (a[2] + a[3])) * (1.f / VIT_DIM);
        const float m2 = wave_sum((a[0] * v[0] + a[1] * v[1]) + (a[2] * v[2] + a[3] * v[3])) * (1.f / VIT_DIM);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * ((a[e] - m1) - v[e] * m2);
        float* dp = dx + row * lddx + lane * 4;
        if (accumulate) {
            float old[4];
            load_f32(dp, old);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = old[e] + o[e];
        }
        store_from_f32(dp, o);
    }
    store_from_f32(&red[wave][0][lane * 4], dg);
    store_from_f32(&red[wave][1][lane * 4], db);
    __syncthreads();
    const int c = threadIdx.x;
#pragma unroll
    for (int w = 0; w < 2; ++w)
        part[(blockIdx.x * (int64_t)2 + w) * VIT_DIM + c] = ((red[0][w][c] + red[1][w][c]) + red[2][w][c]) + red[3][w][c];
}

// out0[c] = sum_s part[s][0][c], out1[c] = sum_s part[s][1][c], slabs in order (compensated: the slab count grows with the row count)
__global__ __launch_bounds__(512) void vit_colsum_finish_kernel(const float* __restrict__ part, int64_t nslab, float* __restrict__ out0, float* __restrict__ out1) {
    const int w = threadIdx.x >> 8, c = threadIdx.x & 255;
    float s = 0.f, k = 0.f;
    for (int64_t i = 0; i < nslab; ++i) kahan_add(s, k, part[(i * 2 + w) * VIT_DIM + c]);
    (w ? out1 : out0)[c] = s - k;
}

// ------------------------------------------------------------------------------------------------ token GEMM, data gradient
// dx[M][K] = (g[M][N] W[N][K]) * gelu'(pre) + resid: vit_gemm_kernel's tile and MFMA maps (token on the lane) with the roles of W's two indices exchanged.
// W stays the fp32 nn.Linear tensor [N][K]: a chunk of KC reduction rows n x 64 output columns k is read along k and written TRANSPOSED into LDS
// (ws[k][n], rounded to bf16 in bf16 mode), so no transposed or cast copy exists in HBM.  g may be fp32 in bf16 mode (the residual-stream gradient): it is
// rounded to bf16 on its way into LDS as W is.  TO: bf16 / fp32 result (fp32: a stream-side gradient, the only form that takes the residual).
__device__ __forceinline__ float gelu_erf_grad(float v) {
    return 0.5f * (1.f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

#define VIT_GEMM_BWD_DATA_KERNEL vit_gemm_bwd_data_kernel
#define VIT_GEMM_BWD_DROP 0
#include "vit_gemm_bwd_data.inc"
#undef VIT_GEMM_BWD_DATA_KERNEL
#undef VIT_GEMM_BWD_DROP
#define VIT_GEMM_BWD_DATA_KERNEL vit_gemm_bwd_data_dropout_kernel
#define VIT_GEMM_BWD_DROP 1
#include "vit_gemm_bwd_data.inc"
#undef VIT_GEMM_BWD_DATA_KERNEL
#undef VIT_GEMM_BWD_DROP

// ------------------------------------------------------------------------------------------------ token GEMM, weight gradient
// dW[N][K] = sum_m g[m][n] x[m][k], db[n] = sum_m g[m][n].  An MFMA GEMM whose reduction index is the token: D = x^T g, so lane (r, h) owns output row
// n = r and, per register group, four consecutive k (16-byte stores).  Workgroup = a 64 (n) x 64 (k) tile of ONE slab of WG_SLAB tokens (the slab cut
// depends on M only), 4 waves of 32 x 32, tokens walked in chunks of 64.  bf16: both operands are written transposed into LDS ([feature][token]) so that a
// fragment is 8 consecutive tokens; fp32 (32x32x2, the token pair on the lane halves): natural layout.  Each workgroup writes its partial tile once;
// vit_wgrad_finish_kernel adds the slabs in slab order.  Bias: the workgroups of k tile 0 keep a compensated sum per thread (its 4 columns, its tokens in
// order), join the 16 threads of a column in thread order, and leave (sum, compensation) in the slab.
#define WG_SLAB 512
#define WG_CHUNK 64
template <typename T> struct WgradGeom;
template <> struct WgradGeom<bf16> { static constexpr int ROWS = 64, PITCH = WG_CHUNK + 8; };     // [feature][token], 144-byte rows
template <> struct WgradGeom<float> { static constexpr int ROWS = WG_CHUNK, PITCH = 64 + 4; };   // [token][feature], 272-byte rows

template <typename T, typename TG>
__global__ __launch_bounds__(256) void vit_gemm_wgrad_kernel(const TG* __restrict__ g, int64_t ldg, const T* __restrict__ x, int64_t ldx,
                                                             float* __restrict__ part, float* __restrict__ bpart, int64_t M, int K, int N) {
    using G = WgradGeom<T>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    __shared__ __attribute__((aligned(16))) T gs[G::ROWS * G::PITCH];
    __shared__ __attribute__((aligned(16))) T xs[G::ROWS * G::PITCH];
    __shared__ float bred[16][64][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5, wn = wave >> 1, wk = wave & 1;
    const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int64_t slab = blockIdx.z, mbeg = slab * WG_SLAB, mend = mbeg + WG_SLAB < M ? mbeg + WG_SLAB : M;
    const int tok = t >> 4, piece = t & 15;               // this thread's pieces: tokens tok + 16 i of the chunk, columns 4 piece .. 4 piece + 3
    const bool want_bias = blockIdx.y == 0;
    float bs[4] = {0.f, 0.f, 0.f, 0.f}, bc[4] = {0.f, 0.f, 0.f, 0.f};
    float rg[4][4], rx[4][4];
    auto fetch = [&](int64_t mc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t m = mc + tok + 16 * i;
            if (m < mend) {
                load_f32(g + m * ldg + n0 + piece * 4, rg[i]);
                load_f32(x + m * ldx + k0 + piece * 4, rx[i]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) rg[i][e] = rx[i][e] = 0.f;
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    fetch(mbeg);
    for (int64_t mc = mbeg; mc < mend; mc += WG_CHUNK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (BF) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    gs[(piece * 4 + e) * G::PITCH + tok + 16 * i] = (bf16)rg[i][e];
                    xs[(piece * 4 + e) * G::PITCH + tok + 16 * i] = (bf16)rx[i][e];
                }
            } else {
                store_from_f32(gs + (tok + 16 * i) * G::PITCH + piece * 4, rg[i]);
                store_from_f32(xs + (tok + 16 * i) * G::PITCH + piece * 4, rx[i]);
            }
            if (want_bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) kahan_add(bs[e], bc[e], rg[i][e]);
            }
        }
        __syncthreads();
        if (mc + WG_CHUNK < mend) fetch(mc + WG_CHUNK);
        if constexpr (BF) {
#pragma unroll
            for (int s = 0; s < WG_CHUNK / 16; ++s) {
                const bf16x8 a = *(const bf16x8*)(xs + (wk * 32 + r) * G::PITCH + 16 * s + 8 * h);
                const bf16x8 b = *(const bf16x8*)(gs + (wn * 32 + r) * G::PITCH + 16 * s + 8 * h);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
        } else {
#pragma unroll 8
            for (int s = 0; s < WG_CHUNK / 2; ++s) {
                const float a = xs[(2 * s + h) * G::PITCH + wk * 32 + r], b = gs[(2 * s + h) * G::PITCH + wn * 32 + r];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
    }
    float* pt = part + (slab * N + n0 + wn * 32 + r) * K + k0 + wk * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[4 * q + e];
        store_from_f32(pt + 8 * q + 4 * h, v);
    }
    if (!want_bias) return;                               // uniform over the workgroup
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bred[tok][piece * 4 + e][0] = bs[e];
        bred[tok][piece * 4 + e][1] = bc[e];
    }
    __syncthreads();
    if (t < 64) {
        float s = 0.f, c = 0.f;
        for (int j = 0; j < 16; ++j) {
            kahan_add(s, c, bred[j][t][0]);
            kahan_add(s, c, -bred[j][t][1]);
        }
        bpart[(slab * N + n0 + t) * 2] = s;
        bpart[(slab * N + n0 + t) * 2 + 1] = c;
    }
}

__global__ __launch_bounds__(256) void vit_wgrad_finish_kernel(const float* __restrict__ part, const float* __restrict__ bpart, float* __restrict__ dW,
                                                               float* __restrict__ db, int64_t nslab, int64_t NK, int N) {
    const int64_t id = blockIdx.x * (int64_t)256 + threadIdx.x;
    for (int64_t p = id; p < NK / 4; p += (int64_t)gridDim.x * 256) {
        float s[4];
        load_f32(part + p * 4, s);
        for (int64_t i = 1; i < nslab; ++i) {
            float v[4];
            load_f32(part + i * NK + p * 4, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
        }
        store_from_f32(dW + p * 4, s);
    }
    if (id < N) {
        float s = 0.f, c = 0.f;
        for (int64_t i = 0; i < nslab; ++i) {
            kahan_add(s, c, bpart[(i * N + id) * 2]);
            kahan_add(s, c, -bpart[(i * N + id) * 2 + 1]);
        }
        db[id] = s - c;
    }
}

// ------------------------------------------------------------------------------------------------ fused attention, backward
// Recompute-style (no N x N matrix leaves the registers): P = 2^(s log2e / sqrt(32) - lse) from the forward's saved row statistic,
// dP = dO V^T, dS = P (dP - delta) / sqrt(32) with delta = rowsum(dO * O) in fp32, dQ = dS K, dK = dS^T Q, dV = P^T dO.  No atomics: two passes of ONE kernel
// template, each the forward's loop with the roles of the two token axes chosen so that the OWNED token is the lane:
//   dq pass  (DKV = false): a workgroup owns 128 query rows (own pair = Q, dO) and walks the key tiles (walk pair = K, V); it also computes delta for its
//            rows and leaves it in the workspace;
//   dkv pass (DKV = true):  a workgroup owns 128 key rows (own pair = K, V) and walks the query tiles (walk pair = Q, dO), reading lse and delta per tile.
// Per 32-row walk sub-tile: S = W1 own1^T and dP = W2 own2^T (A = the walk tile from LDS, B = the lane's own fragment, as the forward's S^T = K Q^T), then
// acc1 += W1^T dS (dQ^T resp. dK^T) and, in the dkv pass, acc2 += W2^T P (dV^T), with the score registers as the B operand (as the forward's O^T = V^T P^T).
// bf16: both walk tensors are staged twice, natural and transposed; P and dS are rounded to bf16 for their products.  Walk rows past the end are zeros
// with P = 0; own rows past the end are clamped on load and never stored.
struct AttBwdArgs {
    const void *own1, *own2, *walk1, *walk2, *out;
    int64_t ld_o1, ld_o2, ld_w1, ld_w2, bs_o1, bs_o2, bs_w1, bs_w2;
    const float* lse;
    float* delta;
    void *g1, *g2;
    int64_t ld_g1, ld_g2, bs_g1, bs_g2;
    int n_own, n_walk, Nq;
    float scale_log2e, scale;
};
template <typename T> struct AttBwdGeom;
template <> struct AttBwdGeom<bf16> { static constexpr int NP = 40, TP = 72, NS = ATT_KT * NP, TS = VIT_HD * TP, NR = 1; };
template <> struct AttBwdGeom<float> { static constexpr int NP = 40, TP = 0, NS = ATT_KT * NP, TS = 4, NR = 2; };

#define VIT_ATT_BWD_KERNEL vit_attention_bwd_kernel
#define VIT_ATT_BWD_DROP 0
#include "vit_attention_bwd.inc"
#undef VIT_ATT_BWD_KERNEL
#undef VIT_ATT_BWD_DROP
#define VIT_ATT_BWD_KERNEL vit_attention_bwd_dropout_kernel
#define VIT_ATT_BWD_DROP 1
#include "vit_attention_bwd.inc"
#undef VIT_ATT_BWD_KERNEL
#undef VIT_ATT_BWD_DROP

// ------------------------------------------------------------------------------------------------ attention weights and rollout
#include "vit_attention_probe.inc"

// ------------------------------------------------------------------------------------------------ attention gradients and relevance
#include "vit_attention_grad_probe.inc"

// ------------------------------------------------------------------------------------------------ Grad-CAM on the stem output
#include "vit_gradcam.inc"

}  // namespace

static bool gemm_shape_ok(int64_t K, int64_t N) { return (K == 256 && (N == 768 || N == 256 || N == 512)) || (K == 512 && N == 256); }

extern "C" int cvae_vit_tokens(const void* stem, int stem_dtype, const float* cls, const float* pos, float* tokens, int64_t B, int64_t n_patches, void* stream) {
    if (B < 1 || n_patches < 1 || B * (n_patches + 1) > ((int64_t)1 << 32)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(stem_dtype)) return CVAE_E_DTYPE;
    if (!stem || !cls || !pos || !tokens) return CVAE_E_NULLPTR;
    if (!aligned16(stem) || !aligned16(cls) || !aligned16(pos) || !aligned16(tokens)) return CVAE_E_UNSUPPORTED;
    const int blocks = cvae_grid_1d(B * (n_patches + 1) * (VIT_DIM / 4), 256, 256 * 32);
    return with_dtype(stem_dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(vit_tokens_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)stem, cls, pos, tokens, B, n_patches);
        return launch_rc();
    });
}

extern "C" int cvae_layernorm256(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* y, int64_t rows, float eps, int out_dtype, void* stream) {
    if (rows < 1 || rows > ((int64_t)1 << 32) || x_stride < VIT_DIM || (x_stride & 3)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(out_dtype)) return CVAE_E_DTYPE;
    if (!x || !gamma || !beta || !y) return CVAE_E_NULLPTR;
    if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(y)) return CVAE_E_UNSUPPORTED;
    const dim3 grid((unsigned)((rows + 3) / 4));
    return with_dtype(out_dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(vit_layernorm_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, x, x_stride, gamma, beta, (T*)y, rows, eps);
        return launch_rc();
    });
}

// ---- what a launch that drops carries.  The dropout entries are the entries around them with a Philox mask recomputed in registers: fp32 only (no
// dtype code is taken, the float instances are launched directly), and p = 0 gives the bits of the entry without dropout.

static bool drop_args(float p, uint64_t key, DropArgs* d) {
    if (!(p >= 0.f && p < 1.f)) return false;
    d->thr = (uint32_t)((double)p * 16777216.0);
    d->k0 = (uint32_t)key;
    d->k1 = (uint32_t)(key >> 32);
    d->scale = 1.0f / (1.0f - p);
    return true;
}

// The key of a dropout entry: a value (the entries of DESIGN §18), or an 8-byte-aligned device pointer that the kernels read when they run (the *_devkey
// entries of DESIGN §19: a captured graph replays with whatever the pointer holds then).
struct DropKey {
    uint64_t value;
    const uint64_t* dev;
    bool on_device;
    bool missing() const { return on_device && !dev; }
    bool misaligned() const { return on_device && ((uintptr_t)dev & 7); }
    const uint32_t* words() const { return on_device ? (const uint32_t*)dev : nullptr; }
};
static DropKey key_value(uint64_t key) { return {key, nullptr, false}; }
static DropKey key_device(const uint64_t* key) { return {0, key, true}; }

// logical rows R = row0 + m step of a row site: with m < 2^30 they stay far below 2^63
static bool mask_rows_ok(int64_t row0, int64_t step) { return row0 >= 0 && row0 <= ((int64_t)1 << 40) && step >= 1 && step <= ((int64_t)1 << 30); }

// One dropout site as the host bodies below take it, by pointer: null = the launch does not drop.  An attention site has no mask rows (0, 1).
struct Drop {
    DropArgs d;
    DropKey key;
    int64_t row0, row_step;
    bool ok;                                                // the rate and the mask rows are in range
};
static Drop drop_site(float p, DropKey key, int64_t row0 = 0, int64_t row_step = 1) {
    Drop s = {{}, key, row0, row_step, false};
    s.ok = drop_args(p, key.value, &s.d) && mask_rows_ok(row0, row_step);
    return s;
}
static bool drop_bad(const Drop* s) { return s && !s->ok; }                           // CVAE_E_BADSHAPE
static bool key_missing(const Drop* s) { return s && s->key.missing(); }              // CVAE_E_NULLPTR
static bool key_misaligned(const Drop* s) { return s && s->key.misaligned(); }        // CVAE_E_UNSUPPORTED

// ---- the token GEMM, forward: cvae_token_gemm, cvae_token_gemm_gelu_train and cvae_token_gemm_dropout[_devkey] (drop: fp32, epilogue RESID or GELU_SAVE)
static int token_gemm(const void* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, void* y, int64_t y_stride,
                      int64_t M, int64_t K, int64_t N, int epilogue, int max_epilogue, int dtype, void* pre, int64_t pre_stride, const Drop* drop, void* stream) {
    if (M < 1 || M > ((int64_t)1 << 30) || x_stride < K || y_stride < N || drop_bad(drop)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (epilogue < GEMM_EPI_NONE || epilogue > max_epilogue) return CVAE_E_BADSHAPE;
    if (!gemm_shape_ok(K, N)) return CVAE_E_UNSUPPORTED;
    if (!x || !W || !bias || !y || key_missing(drop)) return CVAE_E_NULLPTR;
    if (epilogue == CVAE_GEMM_EPI_RESIDUAL) {
        if (!resid) return CVAE_E_NULLPTR;
        if (resid_stride < N) return CVAE_E_BADSHAPE;
        if ((resid_stride & 3) || !aligned16(resid)) return drop ? CVAE_E_UNSUPPORTED : CVAE_E_BADSHAPE;      // the code each family has always answered
    }
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4, ye16 = (epilogue == CVAE_GEMM_EPI_RESIDUAL || dtype == CVAE_F32) ? 4 : 8;
    if ((x_stride % e16) || (y_stride % ye16) || !aligned16(x) || !aligned16(W) || !aligned16(bias) || !aligned16(y) || key_misaligned(drop)) return CVAE_E_UNSUPPORTED;
    if (epilogue == GEMM_EPI_GELU_SAVE) {
        if (!pre) return CVAE_E_NULLPTR;
        if (pre_stride < N) return CVAE_E_BADSHAPE;
        if ((pre_stride % e16) || !aligned16(pre)) return CVAE_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (drop) {                                             // the operand its epilogue does not read is passed as null
        const dim3 grid((unsigned)((M + GEMM_BM - 1) / GEMM_BM), (unsigned)(N / GEMM_BN));
        auto launch = [&](auto kernel, const float* r, int64_t ldr, float* p, int64_t ldp) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const float*)x, x_stride, W, bias, r, ldr, y, y_stride, M, (int)K, (int)N, p, ldp, drop->d, drop->row0,
                               drop->row_step, drop->key.words());
            return launch_rc();
        };
        if (epilogue == GEMM_EPI_RESID) return launch(vit_gemm_dropout_kernel<float, GEMM_EPI_RESID>, resid, resid_stride, nullptr, 0);
        return launch(vit_gemm_dropout_kernel<float, GEMM_EPI_GELU_SAVE>, nullptr, 0, (float*)pre, pre_stride);
    }
    return with_dtype(dtype, [&](auto tv) {
        return gemm_launch((const decltype(tv)*)x, x_stride, W, bias, resid, resid_stride, y, y_stride, M, (int)K, (int)N, epilogue, pre, pre_stride, st);
    });
}

extern "C" int cvae_token_gemm(const void* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, void* y,
                               int64_t y_stride, int64_t M, int64_t K, int64_t N, int epilogue, int dtype, void* stream) {
    return token_gemm(x, x_stride, W, bias, resid, resid_stride, y, y_stride, M, K, N, epilogue, CVAE_GEMM_EPI_RESIDUAL, dtype, nullptr, 0, nullptr, stream);
}

extern "C" int cvae_token_gemm_gelu_train(const void* x, int64_t x_stride, const float* W, const float* bias, void* pre, int64_t pre_stride, void* y, int64_t y_stride,
                                          int64_t M, int64_t K, int64_t N, int dtype, void* stream) {
    return token_gemm(x, x_stride, W, bias, nullptr, 0, y, y_stride, M, K, N, GEMM_EPI_GELU_SAVE, GEMM_EPI_GELU_SAVE, dtype, pre, pre_stride, nullptr, stream);
}

// the dropout entries' epilogue: CVAE_GEMM_EPI_GELU means GELU with the pre-activation saved; anything but it and RESIDUAL is out of range
static int drop_epilogue(int epilogue) {
    return epilogue == CVAE_GEMM_EPI_GELU ? GEMM_EPI_GELU_SAVE : (epilogue == CVAE_GEMM_EPI_RESIDUAL ? GEMM_EPI_RESID : -1);
}

extern "C" int cvae_token_gemm_dropout(const float* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, float* pre,
                                       int64_t pre_stride, float* y, int64_t y_stride, int64_t M, int64_t K, int64_t N, int epilogue, float p, uint64_t key,
                                       int64_t mask_row0, int64_t mask_row_step, void* stream) {
    const Drop s = drop_site(p, key_value(key), mask_row0, mask_row_step);
    return token_gemm(x, x_stride, W, bias, resid, resid_stride, y, y_stride, M, K, N, drop_epilogue(epilogue), GEMM_EPI_GELU_SAVE, CVAE_F32, pre, pre_stride, &s, stream);
}

extern "C" int cvae_token_gemm_dropout_devkey(const float* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride,
                                              float* pre, int64_t pre_stride, float* y, int64_t y_stride, int64_t M, int64_t K, int64_t N, int epilogue, float p,
                                              const uint64_t* key, int64_t mask_row0, int64_t mask_row_step, void* stream) {
    const Drop s = drop_site(p, key_device(key), mask_row0, mask_row_step);
    return token_gemm(x, x_stride, W, bias, resid, resid_stride, y, y_stride, M, K, N, drop_epilogue(epilogue), GEMM_EPI_GELU_SAVE, CVAE_F32, pre, pre_stride, &s, stream);
}

// ---- fused attention, forward: cvae_mhsa_fwd, cvae_mhsa_fwd_train (lse) and cvae_mhsa_fwd_train_dropout[_devkey] (lse and drop: fp32)
static int mhsa_fwd(const void* q, const void* k, const void* v, void* out, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride,
                    int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype, float* lse, const Drop* drop,
                    void* stream) {
    if (B < 1 || B > 65535 || n_tokens < 1 || n_tokens > ((int64_t)1 << 24) || n_query_rows < 1 || n_query_rows > n_tokens || drop_bad(drop)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (!q || !k || !v || !out || (drop && !lse) || key_missing(drop)) return CVAE_E_NULLPTR;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4;
    if (q_stride < VIT_DIM || k_stride < VIT_DIM || v_stride < VIT_DIM || q_batch_stride < 0 || k_batch_stride < 0 || v_batch_stride < 0) return CVAE_E_BADSHAPE;
    if ((q_stride % e16) || (k_stride % e16) || (v_stride % e16) || (q_batch_stride % e16) || (k_batch_stride % e16) || (v_batch_stride % e16) || !aligned16(q) ||
        !aligned16(k) || !aligned16(v) || !aligned16(out) || (drop && !aligned16(lse)) || key_misaligned(drop))      // lse: judged by the dropout entries alone
        return CVAE_E_UNSUPPORTED;
    const dim3 grid((unsigned)((n_query_rows + 127) / 128), VIT_HEADS, (unsigned)B);
    const float scale_log2e = 0.17677669529663688110f * 1.44269504088896340736f;       // 1 / sqrt(32) * log2(e)
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto tv, auto kernel, auto... more) {    // more: the row statistics a training kernel saves, then the mask of one that drops
        using T = decltype(tv);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (T*)out, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride,
                           v_batch_stride, (int)n_tokens, (int)n_query_rows, scale_log2e, more...);
        return launch_rc();
    };
    if (drop) return launch(float{}, vit_attention_dropout_kernel<float>, lse, drop->d, drop->key.words());
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        return lse ? launch(tv, vit_attention_train_kernel<T>, lse) : launch(tv, vit_attention_kernel<T>);
    });
}

extern "C" int cvae_mhsa_fwd(const void* q, const void* k, const void* v, void* out, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride,
                             int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype, void* stream) {
    return mhsa_fwd(q, k, v, out, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, B, n_tokens, n_query_rows, dtype, nullptr, nullptr, stream);
}

extern "C" int cvae_mhsa_fwd_train(const void* q, const void* k, const void* v, void* out, float* lse, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                   int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype,
                                   void* stream) {
    if (!lse) return CVAE_E_NULLPTR;
    return mhsa_fwd(q, k, v, out, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, B, n_tokens, n_query_rows, dtype, lse, nullptr, stream);
}

extern "C" int cvae_mhsa_fwd_train_dropout(const float* q, const float* k, const float* v, float* out, float* lse, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                           int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows,
                                           float p, uint64_t key, void* stream) {
    const Drop s = drop_site(p, key_value(key));
    return mhsa_fwd(q, k, v, out, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, B, n_tokens, n_query_rows, CVAE_F32, lse, &s, stream);
}

extern "C" int cvae_mhsa_fwd_train_dropout_devkey(const float* q, const float* k, const float* v, float* out, float* lse, int64_t q_stride, int64_t k_stride,
                                                  int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens,
                                                  int64_t n_query_rows, float p, const uint64_t* key, void* stream) {
    const Drop s = drop_site(p, key_device(key));
    return mhsa_fwd(q, k, v, out, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, B, n_tokens, n_query_rows, CVAE_F32, lse, &s, stream);
}

// ---- backward entries.  Every argument check precedes the first launch; workspaces are the caller's.

extern "C" int cvae_vit_tokens_bwd(const float* dtokens, float* dpos, float* dcls, void* dstem, int stem_dtype, const void* gate, int gate_act, int64_t B,
                                   int64_t n_patches, void* stream) {
    if (B < 1 || n_patches < 1 || B * (n_patches + 1) > ((int64_t)1 << 32)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(stem_dtype)) return CVAE_E_DTYPE;
    if (!dtokens || !dpos || !dcls || !dstem) return CVAE_E_NULLPTR;
    if (gate_act != CVAE_ACT_NONE && gate_act != CVAE_ACT_RELU && gate_act != CVAE_ACT_LEAKY001 && gate_act != CVAE_ACT_LEAKY02) return CVAE_E_UNSUPPORTED;
    if (gate_act == CVAE_ACT_NONE) gate = nullptr;                          // not read: whatever the caller passed
    else if (!gate) return CVAE_E_NULLPTR;
    if (!aligned16(dtokens) || !aligned16(dpos) || !aligned16(dcls) || !aligned16(dstem) || !aligned16(gate)) return CVAE_E_UNSUPPORTED;
    const float slope = gate_act == CVAE_ACT_LEAKY02 ? 0.2f : (gate_act == CVAE_ACT_LEAKY001 ? 0.01f : 0.f);
    const int blocks = cvae_grid_1d((n_patches + 1) * (VIT_DIM / 4), 256, 256 * 32);
    return with_dtype(stem_dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(vit_tokens_bwd_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dtokens, dpos, dcls, (T*)dstem, B, n_patches, (const T*)gate, slope);
        return launch_rc();
    });
}

extern "C" size_t cvae_layernorm256_bwd_workspace_bytes(int64_t rows) {
    return rows < 1 ? 0 : (size_t)((rows + LN_SLAB - 1) / LN_SLAB) * 2 * VIT_DIM * sizeof(float);
}

extern "C" int cvae_layernorm256_bwd(const void* g, int64_t g_stride, int g_dtype, const float* x, int64_t x_stride, const float* gamma, float* dx, int64_t dx_stride,
                                     int accumulate, float* dgamma, float* dbeta, int64_t rows, float eps, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows < 1 || rows > ((int64_t)1 << 32) || x_stride < VIT_DIM || (x_stride & 3) || dx_stride < VIT_DIM || (dx_stride & 3) || g_stride < VIT_DIM) return CVAE_E_BADSHAPE;
    if (!dtype_ok(g_dtype)) return CVAE_E_DTYPE;
    if (!g || !x || !gamma || !dx || !dgamma || !dbeta || !workspace) return CVAE_E_NULLPTR;
    if ((g_stride % (g_dtype == CVAE_BF16 ? 8 : 4)) || !aligned16(g) || !aligned16(x) || !aligned16(gamma) || !aligned16(dx) || !aligned16(workspace)) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_layernorm256_bwd_workspace_bytes(rows)) return CVAE_E_WORKSPACE;
    const int64_t nslab = (rows + LN_SLAB - 1) / LN_SLAB;
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype(g_dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(vit_layernorm_bwd_kernel<T>, dim3((unsigned)nslab), dim3(256), 0, st, (const T*)g, g_stride, x, x_stride, gamma, dx, dx_stride, (float*)workspace, rows,
                           eps, accumulate);
        return launch_rc();
    });
    if (rc != CVAE_OK) return rc;
    hipLaunchKernelGGL(vit_colsum_finish_kernel, dim3(1), dim3(512), 0, st, (const float*)workspace, nslab, dgamma, dbeta);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

// cvae_token_gemm_bwd_data and cvae_token_gemm_bwd_data_dropout[_devkey] (drop: fp32 throughout, no resid)
static int token_gemm_bwd_data(const void* g, int64_t g_stride, int g_dtype, const float* W, const void* pre, int64_t pre_stride, const float* resid,
                               int64_t resid_stride, void* dx, int64_t dx_stride, int dx_dtype, int64_t M, int64_t K, int64_t N, int dtype, const Drop* drop,
                               void* stream) {
    if (M < 1 || M > ((int64_t)1 << 30) || g_stride < N || dx_stride < K || drop_bad(drop)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype) || !dtype_ok(g_dtype) || !dtype_ok(dx_dtype)) return CVAE_E_DTYPE;
    if (dtype == CVAE_F32 && (g_dtype != CVAE_F32 || dx_dtype != CVAE_F32)) return CVAE_E_DTYPE;
    if (!gemm_shape_ok(K, N)) return CVAE_E_UNSUPPORTED;
    if (!g || !W || !dx || key_missing(drop)) return CVAE_E_NULLPTR;
    if (resid && (dx_dtype != CVAE_F32 || resid_stride < K || (resid_stride & 3))) return CVAE_E_BADSHAPE;
    if (pre && pre_stride < K) return CVAE_E_BADSHAPE;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4;
    if ((g_stride % (g_dtype == CVAE_BF16 ? 8 : 4)) || (dx_stride % (dx_dtype == CVAE_BF16 ? 8 : 4)) || (pre && (pre_stride % e16)) || !aligned16(g) || !aligned16(W) ||
        !aligned16(dx) || !aligned16(pre) || !aligned16(resid) || key_misaligned(drop))
        return CVAE_E_UNSUPPORTED;
    const dim3 grid((unsigned)((M + GEMM_BM - 1) / GEMM_BM), (unsigned)(K / GEMM_BN));
    hipStream_t st = (hipStream_t)stream;
    if (drop) {
        hipLaunchKernelGGL((vit_gemm_bwd_data_dropout_kernel<float, float, float>), grid, dim3(256), 0, st, (const float*)g, g_stride, W, (const float*)pre, pre_stride, resid,
                           resid_stride, (float*)dx, dx_stride, M, (int)K, (int)N, drop->d, drop->row0, drop->row_step, drop->key.words());
        return launch_rc();
    }
    return with_dtype(dtype, [&](auto tv) { return with_dtype2(g_dtype, dx_dtype, [&](auto tg, auto to) {
        using T = decltype(tv);
        using TG = std::conditional_t<std::is_same_v<T, float>, float, decltype(tg)>;      // an fp32 product has fp32 ends (checked above): no mixed instance of it
        using TO = std::conditional_t<std::is_same_v<T, float>, float, decltype(to)>;
        hipLaunchKernelGGL((vit_gemm_bwd_data_kernel<T, TG, TO>), grid, dim3(256), 0, st, (const TG*)g, g_stride, W, (const T*)pre, pre_stride, resid, resid_stride, (TO*)dx,
                           dx_stride, M, (int)K, (int)N);
        return launch_rc();
    }); });
}

extern "C" int cvae_token_gemm_bwd_data(const void* g, int64_t g_stride, int g_dtype, const float* W, const void* pre, int64_t pre_stride, const float* resid,
                                        int64_t resid_stride, void* dx, int64_t dx_stride, int dx_dtype, int64_t M, int64_t K, int64_t N, int dtype, void* stream) {
    return token_gemm_bwd_data(g, g_stride, g_dtype, W, pre, pre_stride, resid, resid_stride, dx, dx_stride, dx_dtype, M, K, N, dtype, nullptr, stream);
}

extern "C" int cvae_token_gemm_bwd_data_dropout(const float* g, int64_t g_stride, const float* W, const float* pre, int64_t pre_stride, float* dx, int64_t dx_stride,
                                                int64_t M, int64_t K, int64_t N, float p, uint64_t key, int64_t mask_row0, int64_t mask_row_step, void* stream) {
    const Drop s = drop_site(p, key_value(key), mask_row0, mask_row_step);
    return token_gemm_bwd_data(g, g_stride, CVAE_F32, W, pre, pre_stride, nullptr, 0, dx, dx_stride, CVAE_F32, M, K, N, CVAE_F32, &s, stream);
}

extern "C" int cvae_token_gemm_bwd_data_dropout_devkey(const float* g, int64_t g_stride, const float* W, const float* pre, int64_t pre_stride, float* dx,
                                                       int64_t dx_stride, int64_t M, int64_t K, int64_t N, float p, const uint64_t* key, int64_t mask_row0,
                                                       int64_t mask_row_step, void* stream) {
    const Drop s = drop_site(p, key_device(key), mask_row0, mask_row_step);
    return token_gemm_bwd_data(g, g_stride, CVAE_F32, W, pre, pre_stride, nullptr, 0, dx, dx_stride, CVAE_F32, M, K, N, CVAE_F32, &s, stream);
}

extern "C" size_t cvae_token_gemm_wgrad_workspace_bytes(int64_t M, int64_t K, int64_t N) {
    if (M < 1 || M > (int64_t)65535 * WG_SLAB || !gemm_shape_ok(K, N)) return 0;
    return (size_t)((M + WG_SLAB - 1) / WG_SLAB) * (size_t)(N * K + 2 * N) * sizeof(float);
}

extern "C" int cvae_token_gemm_wgrad(const void* g, int64_t g_stride, int g_dtype, const void* x, int64_t x_stride, float* dW, float* db, int64_t M, int64_t K,
                                     int64_t N, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (M < 1 || M > (int64_t)65535 * WG_SLAB || g_stride < N || x_stride < K) return CVAE_E_BADSHAPE;      // the slab index is grid.z
    if (!dtype_ok(dtype) || !dtype_ok(g_dtype) || (dtype == CVAE_F32 && g_dtype != CVAE_F32)) return CVAE_E_DTYPE;
    if (!gemm_shape_ok(K, N)) return CVAE_E_UNSUPPORTED;
    if (!g || !x || !dW || !db || !workspace) return CVAE_E_NULLPTR;
    if ((g_stride % (g_dtype == CVAE_BF16 ? 8 : 4)) || (x_stride % (dtype == CVAE_BF16 ? 8 : 4)) || !aligned16(g) || !aligned16(x) || !aligned16(dW) || !aligned16(workspace))
        return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_token_gemm_wgrad_workspace_bytes(M, K, N)) return CVAE_E_WORKSPACE;
    const int64_t nslab = (M + WG_SLAB - 1) / WG_SLAB;
    float* part = (float*)workspace;
    float* bpart = part + nslab * N * K;
    const dim3 grid((unsigned)(N / 64), (unsigned)(K / 64), (unsigned)nslab);
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype2(dtype, g_dtype, [&](auto tv, auto tg) {
        using T = decltype(tv);
        using TG = std::conditional_t<std::is_same_v<T, float>, float, decltype(tg)>;      // as in cvae_token_gemm_bwd_data
        hipLaunchKernelGGL((vit_gemm_wgrad_kernel<T, TG>), grid, dim3(256), 0, st, (const TG*)g, g_stride, (const T*)x, x_stride, part, bpart, M, (int)K, (int)N);
        return launch_rc();
    });
    if (rc != CVAE_OK) return rc;
    hipLaunchKernelGGL(vit_wgrad_finish_kernel, dim3((unsigned)(N * K / 4 / 256)), dim3(256), 0, st, (const float*)part, (const float*)bpart, dW, db, nslab, N * K, (int)N);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" size_t cvae_mhsa_bwd_workspace_bytes(int64_t B, int64_t n_query_rows) {
    return (B < 1 || n_query_rows < 1) ? 0 : (size_t)(B * VIT_HEADS * n_query_rows) * sizeof(float);
}

// cvae_mhsa_bwd and cvae_mhsa_bwd_dropout[_devkey] (drop: fp32)
static int mhsa_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse, const void* dout, void* dq, void* dk, void* dv, int64_t q_stride,
                    int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t dq_stride, int64_t dk_stride,
                    int64_t dv_stride, int64_t dq_batch_stride, int64_t dk_batch_stride, int64_t dv_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows,
                    int dtype, const Drop* drop, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || B > 65535 || n_tokens < 1 || n_tokens > ((int64_t)1 << 24) || n_query_rows < 1 || n_query_rows > n_tokens || drop_bad(drop)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !workspace || key_missing(drop)) return CVAE_E_NULLPTR;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4;
    const int64_t strides[12] = {q_stride, k_stride, v_stride, dq_stride, dk_stride, dv_stride, q_batch_stride, k_batch_stride, v_batch_stride,
                                 dq_batch_stride, dk_batch_stride, dv_batch_stride};
    for (int i = 0; i < 12; ++i)
        if (strides[i] < (i < 6 ? VIT_DIM : 0)) return CVAE_E_BADSHAPE;
    for (int i = 0; i < 12; ++i)
        if (strides[i] % e16) return CVAE_E_UNSUPPORTED;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(dout) || !aligned16(dq) || !aligned16(dk) || !aligned16(dv)) return CVAE_E_UNSUPPORTED;
    if (drop && (!aligned16(lse) || !aligned16(workspace) || key_misaligned(drop))) return CVAE_E_UNSUPPORTED;      // lse, workspace: judged by the dropout entries alone
    if (workspace_bytes < cvae_mhsa_bwd_workspace_bytes(B, n_query_rows)) return CVAE_E_WORKSPACE;
    const int N = (int)n_tokens, Nq = (int)n_query_rows;
    const int64_t ob = (int64_t)Nq * VIT_DIM;
    const float scale = 0.17677669529663688110f, scale_log2e = scale * 1.44269504088896340736f;
    const AttBwdArgs aq = {q, dout, k, v, out, q_stride, VIT_DIM, k_stride, v_stride, q_batch_stride, ob, k_batch_stride, v_batch_stride, lse, (float*)workspace,
                           dq, nullptr, dq_stride, 0, dq_batch_stride, 0, Nq, N, Nq, scale_log2e, scale};
    const AttBwdArgs ak = {k, v, q, dout, out, k_stride, v_stride, q_stride, VIT_DIM, k_batch_stride, v_batch_stride, q_batch_stride, ob, lse, (float*)workspace,
                           dk, dv, dk_stride, dv_stride, dk_batch_stride, dv_batch_stride, N, Nq, Nq, scale_log2e, scale};
    const dim3 gq((unsigned)((Nq + 127) / 128), VIT_HEADS, (unsigned)B), gk((unsigned)((N + 127) / 128), VIT_HEADS, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (drop) {
        hipLaunchKernelGGL((vit_attention_bwd_dropout_kernel<float, false>), gq, dim3(256), 0, st, aq, drop->d, drop->key.words());
        CVAE_CHECK_LAUNCH();
        hipLaunchKernelGGL((vit_attention_bwd_dropout_kernel<float, true>), gk, dim3(256), 0, st, ak, drop->d, drop->key.words());
        return launch_rc();
    }
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL((vit_attention_bwd_kernel<T, false>), gq, dim3(256), 0, st, aq);
        CVAE_CHECK_LAUNCH();
        hipLaunchKernelGGL((vit_attention_bwd_kernel<T, true>), gk, dim3(256), 0, st, ak);
        return launch_rc();
    });
}

extern "C" int cvae_mhsa_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse, const void* dout, void* dq, void* dk, void* dv,
                             int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride,
                             int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int64_t dq_batch_stride, int64_t dk_batch_stride, int64_t dv_batch_stride,
                             int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return mhsa_bwd(q, k, v, out, lse, dout, dq, dk, dv, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, dq_stride, dk_stride, dv_stride,
                    dq_batch_stride, dk_batch_stride, dv_batch_stride, B, n_tokens, n_query_rows, dtype, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int cvae_mhsa_bwd_dropout(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* dout, float* dq, float* dk,
                                     float* dv, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride,
                                     int64_t v_batch_stride, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int64_t dq_batch_stride, int64_t dk_batch_stride,
                                     int64_t dv_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, float p, uint64_t key, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const Drop s = drop_site(p, key_value(key));
    return mhsa_bwd(q, k, v, out, lse, dout, dq, dk, dv, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, dq_stride, dk_stride, dv_stride,
                    dq_batch_stride, dk_batch_stride, dv_batch_stride, B, n_tokens, n_query_rows, CVAE_F32, &s, workspace, workspace_bytes, stream);
}

extern "C" int cvae_mhsa_bwd_dropout_devkey(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* dout, float* dq, float* dk,
                                            float* dv, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride,
                                            int64_t v_batch_stride, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int64_t dq_batch_stride,
                                            int64_t dk_batch_stride, int64_t dv_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, float p,
                                            const uint64_t* key, void* workspace, size_t workspace_bytes, void* stream) {
    const Drop s = drop_site(p, key_device(key));
    return mhsa_bwd(q, k, v, out, lse, dout, dq, dk, dv, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, dq_stride, dk_stride, dv_stride,
                    dq_batch_stride, dk_batch_stride, dv_batch_stride, B, n_tokens, n_query_rows, CVAE_F32, &s, workspace, workspace_bytes, stream);
}

// ---- attention weights and attention rollout: forward-only views inside the encoder, recomputed from q, k and cvae_mhsa_fwd_train's lse.

// the checks the two entries share (pointers and strides as cvae_mhsa_fwd); CVAE_OK with B == 0 means: nothing to launch
static int mhsa_probe_check(const void* q, const void* k, const float* lse, int64_t q_stride, int64_t k_stride, int64_t q_batch_stride, int64_t k_batch_stride,
                            int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype) {
    if (B < 0 || B > 65535 || n_tokens < 1 || n_tokens > ((int64_t)1 << 24) || n_query_rows < 1 || n_query_rows > n_tokens) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (B == 0) return CVAE_OK;
    if (!q || !k || !lse) return CVAE_E_NULLPTR;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4;
    if (q_stride < VIT_DIM || k_stride < VIT_DIM || q_batch_stride < 0 || k_batch_stride < 0) return CVAE_E_BADSHAPE;
    if ((q_stride % e16) || (k_stride % e16) || (q_batch_stride % e16) || (k_batch_stride % e16) || !aligned16(q) || !aligned16(k) || ((uintptr_t)lse & 3))
        return CVAE_E_UNSUPPORTED;
    return CVAE_OK;
}

// the one launch of both entries: a workgroup per (128 keys, head in the per-head form, batch row)
static int mhsa_probe_launch(const AttProbeArgs& a, int mode, int64_t B, int dtype, void* stream) {
    const dim3 grid((unsigned)((a.N + 127) / 128), mode == PROBE_HEADS ? VIT_HEADS : 1, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        if (mode == PROBE_HEADS) hipLaunchKernelGGL((vit_attention_probe_kernel<T, PROBE_HEADS>), grid, dim3(256), 0, st, a);
        else if (mode == PROBE_AVERAGE) hipLaunchKernelGGL((vit_attention_probe_kernel<T, PROBE_AVERAGE>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((vit_attention_probe_kernel<T, PROBE_ROLLOUT>), grid, dim3(256), 0, st, a);
        return launch_rc();
    });
}

extern "C" int cvae_mhsa_weights(const void* q, const void* k, const float* lse, float* w, int64_t q_stride, int64_t k_stride, int64_t q_batch_stride,
                                 int64_t k_batch_stride, int64_t w_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int average_heads, int dtype,
                                 void* stream) {
    const int rc = mhsa_probe_check(q, k, lse, q_stride, k_stride, q_batch_stride, k_batch_stride, B, n_tokens, n_query_rows, dtype);
    if (rc != CVAE_OK || B == 0) return rc;
    if (!w) return CVAE_E_NULLPTR;
    if (w_batch_stride < (average_heads ? 1 : VIT_HEADS) * n_query_rows * n_tokens) return CVAE_E_BADSHAPE;
    if (!aligned16(w)) return CVAE_E_UNSUPPORTED;
    const AttProbeArgs a = {q, k, q_stride, k_stride, q_batch_stride, k_batch_stride, lse, nullptr, w, w_batch_stride, (int)n_tokens, (int)n_query_rows,
                            0.17677669529663688110f * 1.44269504088896340736f, 0.f};       // 1 / sqrt(32) * log2(e), as cvae_mhsa_fwd
    return mhsa_probe_launch(a, average_heads ? PROBE_AVERAGE : PROBE_HEADS, B, dtype, stream);
}

extern "C" int cvae_mhsa_rollout_step(const void* q, const void* k, const float* lse, const float* r, float* out, int64_t q_stride, int64_t k_stride,
                                      int64_t q_batch_stride, int64_t k_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, float residual, int dtype,
                                      void* stream) {
    const int rc = mhsa_probe_check(q, k, lse, q_stride, k_stride, q_batch_stride, k_batch_stride, B, n_tokens, n_query_rows, dtype);
    if (rc != CVAE_OK) return rc;
    if (!(residual >= 0.f && residual <= 1.f)) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if (!r || !out) return CVAE_E_NULLPTR;
    if (((uintptr_t)r & 3) || ((uintptr_t)out & 3)) return CVAE_E_UNSUPPORTED;
    if (r < out + B * n_tokens && out < r + B * n_tokens) return CVAE_E_UNSUPPORTED;       // out == r, or any overlap: other workgroups still read r
    const AttProbeArgs a = {q, k, q_stride, k_stride, q_batch_stride, k_batch_stride, lse, r, out, 0, (int)n_tokens, (int)n_query_rows,
                            0.17677669529663688110f * 1.44269504088896340736f, residual};
    return mhsa_probe_launch(a, PROBE_ROLLOUT, B, dtype, stream);
}

// ---- attention gradients and gradient-weighted relevance: forward-only, from the data-only backward's datt and the walk's q, k, v, lse.

// the checks of dout (dense [B][n_query_rows][256]) and the v view.  cvae_mhsa_relevance_step runs them after mhsa_probe_check's; cvae_mhsa_weight_grads has no q, k
// or lse and passes its sizes (sizes = true): the same size and dtype checks first; CVAE_OK with B == 0 means: nothing to launch
static int mhsa_grad_probe_check(const void* dout, const void* v, int64_t v_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows,
                                 int dtype, bool sizes) {
    if (sizes) {
        if (B < 0 || B > 65535 || n_tokens < 1 || n_tokens > ((int64_t)1 << 24) || n_query_rows < 1 || n_query_rows > n_tokens) return CVAE_E_BADSHAPE;
        if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
        if (B == 0) return CVAE_OK;
    }
    if (!dout || !v) return CVAE_E_NULLPTR;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4;
    if (v_stride < VIT_DIM || v_batch_stride < 0) return CVAE_E_BADSHAPE;
    if ((v_stride % e16) || (v_batch_stride % e16) || !aligned16(dout) || !aligned16(v)) return CVAE_E_UNSUPPORTED;
    return CVAE_OK;
}

// the one launch of both entries: a workgroup per (128 keys, head or chunk of query tiles, batch row)
static int mhsa_grad_probe_launch(const AttGradProbeArgs& a, int mode, unsigned grid_y, int64_t B, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + 127) / 128), grid_y, (unsigned)B);
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        if (mode == GRADP_HEADS) hipLaunchKernelGGL((vit_attention_grad_probe_kernel<T, GRADP_HEADS>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((vit_attention_grad_probe_kernel<T, GRADP_RELEVANCE>), grid, dim3(256), 0, st, a);
        return launch_rc();
    });
}

// query tiles -> chunks of the relevance step: a function of n_query_rows alone
static int64_t relevance_chunks(int64_t n_query_rows) {
    const int64_t tiles = (n_query_rows + ATT_KT - 1) / ATT_KT;
    return (tiles + GRADP_CHUNK_TILES - 1) / GRADP_CHUNK_TILES;
}

extern "C" int cvae_mhsa_weight_grads(const void* dout, const void* v, float* w, int64_t v_stride, int64_t v_batch_stride, int64_t w_batch_stride, int64_t B,
                                      int64_t n_tokens, int64_t n_query_rows, int dtype, void* stream) {
    const int rc = mhsa_grad_probe_check(dout, v, v_stride, v_batch_stride, B, n_tokens, n_query_rows, dtype, true);
    if (rc != CVAE_OK || B == 0) return rc;
    if (!w) return CVAE_E_NULLPTR;
    if (w_batch_stride < VIT_HEADS * n_query_rows * n_tokens) return CVAE_E_BADSHAPE;
    if (!aligned16(w)) return CVAE_E_UNSUPPORTED;
    const AttGradProbeArgs a = {nullptr, nullptr, v, dout, 0, 0, v_stride, 0, 0, v_batch_stride, nullptr, nullptr, w, w_batch_stride, (int)n_tokens,
                                (int)n_query_rows, 0.f};
    return mhsa_grad_probe_launch(a, GRADP_HEADS, VIT_HEADS, B, dtype, (hipStream_t)stream);
}

extern "C" size_t cvae_mhsa_relevance_step_workspace_bytes(int64_t B, int64_t n_tokens, int64_t n_query_rows) {
    if (B < 1 || n_tokens < 1 || n_query_rows < 1 || n_query_rows > n_tokens) return 0;
    const int64_t S = relevance_chunks(n_query_rows);
    return S < 2 ? 0 : (size_t)(B * S * n_tokens) * sizeof(float);      // one chunk writes out itself
}

extern "C" int cvae_mhsa_relevance_step(const void* q, const void* k, const void* v, const float* lse, const void* dout, const float* r, float* out, int64_t q_stride,
                                        int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B,
                                        int64_t n_tokens, int64_t n_query_rows, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = mhsa_probe_check(q, k, lse, q_stride, k_stride, q_batch_stride, k_batch_stride, B, n_tokens, n_query_rows, dtype);
    if (rc != CVAE_OK || B == 0) return rc;
    rc = mhsa_grad_probe_check(dout, v, v_stride, v_batch_stride, B, n_tokens, n_query_rows, dtype, false);
    if (rc != CVAE_OK) return rc;
    const int64_t S = relevance_chunks(n_query_rows);
    if (!r || !out || (S > 1 && !workspace)) return CVAE_E_NULLPTR;
    if (((uintptr_t)r & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 3) || S > 65535) return CVAE_E_UNSUPPORTED;      // the chunk index is grid.y
    if (r < out + B * n_tokens && out < r + B * n_tokens) return CVAE_E_UNSUPPORTED;       // out == r, or any overlap: other workgroups still read r
    if (workspace_bytes < cvae_mhsa_relevance_step_workspace_bytes(B, n_tokens, n_query_rows)) return CVAE_E_WORKSPACE;
    const AttGradProbeArgs a = {q, k, v, dout, q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, lse, r,
                                S > 1 ? (float*)workspace : out, 0, (int)n_tokens, (int)n_query_rows, 0.17677669529663688110f * 1.44269504088896340736f};
    hipStream_t st = (hipStream_t)stream;
    rc = mhsa_grad_probe_launch(a, GRADP_RELEVANCE, (unsigned)S, B, dtype, st);
    if (rc != CVAE_OK || S == 1) return rc;
    const int64_t total = B * n_tokens;
    hipLaunchKernelGGL(vit_relevance_finish_kernel, dim3(cvae_grid_1d(total, 256, 256 * 32)), dim3(256), 0, st, (const float*)workspace, r, out, (int)S, (int)n_tokens, total);
    return launch_rc();
}

// ---- Grad-CAM on the stem output: forward-only, one workgroup per image.  The checks and the launch, as for the probe entries above.
static int gradcam_check(const void* A, const void* dA, const float* cam, int64_t B, int64_t n, int dtype) {
    if (B < 0 || n < 1) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (n > GRADCAM_MAX_N || B > 0x7fffffff) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!A || !dA || !cam) return CVAE_E_NULLPTR;
    if (!aligned16(A) || !aligned16(dA) || ((uintptr_t)cam & 3)) return CVAE_E_UNSUPPORTED;
    const size_t in_bytes = (size_t)(B * n) * VIT_DIM * (dtype == CVAE_BF16 ? 2 : 4), out_bytes = (size_t)(B * n) * sizeof(float);
    const uintptr_t c0 = (uintptr_t)cam, a0 = (uintptr_t)A, d0 = (uintptr_t)dA;
    if ((c0 < a0 + in_bytes && a0 < c0 + out_bytes) || (c0 < d0 + in_bytes && d0 < c0 + out_bytes)) return CVAE_E_UNSUPPORTED;      // cam inside an input
    return CVAE_OK;
}

static int gradcam_launch(const void* A, const void* dA, float* cam, int64_t B, int n, int normalize, int dtype, void* stream) {
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(vit_gradcam_kernel<T>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const T*)A, (const T*)dA, cam, n, normalize);
        return launch_rc();
    });
}

extern "C" int cvae_gradcam256(const void* A, const void* dA, float* cam, int64_t B, int64_t n, int normalize, int dtype, void* stream) {
    const int rc = gradcam_check(A, dA, cam, B, n, dtype);
    if (rc != CVAE_OK || B == 0) return rc;
    return gradcam_launch(A, dA, cam, B, (int)n, normalize != 0, dtype, stream);
}

// ---- dropout on rows: the one dropout entry that is no form of another.  Every argument check precedes the launch.

static int dropout_rows(const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t M, int64_t N, float p, DropKey key, int64_t mask_row0,
                        int64_t mask_row_step, void* stream) {
    DropArgs d;
    if (M < 1 || M > ((int64_t)1 << 30) || N < 4 || N > ((int64_t)1 << 30) || (N & 3) || x_stride < N || y_stride < N || !drop_args(p, key.value, &d) ||
        !mask_rows_ok(mask_row0, mask_row_step))
        return CVAE_E_BADSHAPE;
    if (!x || !y || key.missing()) return CVAE_E_NULLPTR;
    if ((x_stride & 3) || (y_stride & 3) || !aligned16(x) || !aligned16(y) || key.misaligned()) return CVAE_E_UNSUPPORTED;
    const int blocks = cvae_grid_1d(M * (N / 4), 256, 256 * 32);
    hipLaunchKernelGGL(vit_dropout_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, x_stride, y, y_stride, M, (int)N, d, mask_row0, mask_row_step,
                       key.words());
    return launch_rc();
}

extern "C" int cvae_dropout_rows(const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t M, int64_t N, float p, uint64_t key, int64_t mask_row0,
                                 int64_t mask_row_step, void* stream) {
    return dropout_rows(x, x_stride, y, y_stride, M, N, p, key_value(key), mask_row0, mask_row_step, stream);
}

extern "C" int cvae_dropout_rows_devkey(const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t M, int64_t N, float p, const uint64_t* key,
                                        int64_t mask_row0, int64_t mask_row_step, void* stream) {
    return dropout_rows(x, x_stride, y, y_stride, M, N, p, key_device(key), mask_row0, mask_row_step, stream);
}

// ---- device-resident keys: the keys of one step's sites, derived on the device from a counter that the same launch advances ----------------
extern "C" int cvae_dropout_keys_step(uint64_t base, int64_t* step, uint64_t* table, int n_blocks, void* stream) {
    if (n_blocks < 1 || n_blocks > 65536) return CVAE_E_BADSHAPE;
    if (!step || !table) return CVAE_E_NULLPTR;
    if (((uintptr_t)step & 7) || ((uintptr_t)table & 7)) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(vit_dropout_keys_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, base, step, table, n_blocks);
    return launch_rc();
}
