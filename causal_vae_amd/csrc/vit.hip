// vit.hip — the transformer side of the ViT-VAE encoder in eval mode (vessel_analysis/00_core/vit_backbone.py:158-179 of the reference):
//   * token assembly: CLS + stem output + position embedding -> fp32 residual stream [B][N][256];
//   * LayerNorm(256): one wave per row, two-pass (mean, then squared deviations), xor-shuffle wave sums;
//   * token GEMM y = epi(x W^T + b) with epilogues none / exact-erf GELU / + residual, K <= 512 walked in LDS chunks (no split-K, no finish launch);
//   * fused multi-head self-attention (8 heads x 32): online softmax over 64-key tiles, scores never leave the registers.
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

template <typename T> struct GemmGeom {
    static constexpr int KC = 128 / sizeof(T);            // k elements per chunk
    static constexpr int PITCH = KC + 16 / sizeof(T);     // LDS row pitch in elements: 144 bytes (16-byte aligned, rows 36 banks apart)
    static constexpr int E16 = 16 / sizeof(T);            // elements per 16-byte piece
    static constexpr int WP = KC / 16;                    // float4 pieces of W per thread and chunk
};

__device__ __forceinline__ void lds_put_w(bf16* dst, float4 w) { *(uint2*)dst = make_uint2(pack2_bf16(w.x, w.y), pack2_bf16(w.z, w.w)); }
__device__ __forceinline__ void lds_put_w(float* dst, float4 w) { *(float4*)dst = w; }

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

template <typename T, int EPI>
__global__ __launch_bounds__(256) void vit_gemm_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* resid, int64_t ldr, void* yv, int64_t ldy, int64_t M, int K, int N) {
    using G = GemmGeom<T>;
    __shared__ __attribute__((aligned(16))) T xs[GEMM_BM * G::PITCH];
    __shared__ __attribute__((aligned(16))) T ws[GEMM_BN * G::PITCH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int64_t m0 = blockIdx.x * (int64_t)GEMM_BM;
    const int n0 = blockIdx.y * GEMM_BN;
    uint4 rx[4];
    float4 rw[G::WP];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = t + 256 * i, row = p >> 3, piece = p & 7;
            const int64_t gm = m0 + row;
            rx[i] = gm < M ? *(const uint4*)(x + gm * ldx + k0 + piece * G::E16) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < G::WP; ++i) {
            const int p = t + 256 * i, row = p / (G::KC / 4), piece = p % (G::KC / 4);
            rw[i] = *(const float4*)(W + (int64_t)(n0 + row) * K + k0 + piece * 4);
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += G::KC) {
        __syncthreads();                                    // the previous chunk's fragment reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = t + 256 * i, row = p >> 3, piece = p & 7;
            *(uint4*)(xs + row * G::PITCH + piece * G::E16) = rx[i];
        }
#pragma unroll
        for (int i = 0; i < G::WP; ++i) {
            const int p = t + 256 * i, row = p / (G::KC / 4), piece = p % (G::KC / 4);
            lds_put_w(ws + row * G::PITCH + piece * 4, rw[i]);
        }
        __syncthreads();
        if (k0 + G::KC < K) fetch(k0 + G::KC);
        if constexpr (std::is_same<T, bf16>::value) {
#pragma unroll
            for (int s = 0; s < G::KC / 16; ++s) {
                const bf16x8 b = *(const bf16x8*)(xs + (wave * 32 + r) * G::PITCH + 16 * s + 8 * h);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bf16x8 a = *(const bf16x8*)(ws + (j * 32 + r) * G::PITCH + 16 * s + 8 * h);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
                }
            }
        } else {
            // 32x32x2: the instruction's k index is the lane half; step (c, u) multiplies k = 16 h + 4 c + u of the chunk (any k order gives the product)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float b[4], a[2][4];
                load_f32(xs + (wave * 32 + r) * G::PITCH + 16 * h + 4 * c, b);
#pragma unroll
                for (int j = 0; j < 2; ++j) load_f32(ws + (j * 32 + r) * G::PITCH + 16 * h + 4 * c, a[j]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j][u], b[u], acc[j], 0, 0, 0);
            }
        }
    }
    const int64_t gm = m0 + wave * 32 + r;
    if (gm >= M) return;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = n0 + j * 32 + 8 * g + 4 * h;
            float v[4], bv[4];
            load_f32(bias + n, bv);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[j][4 * g + e] + bv[e];
            if (EPI == GEMM_EPI_RESID) {
                float rv[4];
                load_f32(resid + gm * ldr + n, rv);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rv[e] + v[e];
                store_from_f32((float*)yv + gm * ldy + n, v);
            } else {
                if (EPI == GEMM_EPI_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
                }
                store_from_f32((T*)yv + gm * ldy + n, v);
            }
        }
}

template <typename T>
int gemm_launch(const T* x, int64_t ldx, const float* W, const float* bias, const float* resid, int64_t ldr, void* y, int64_t ldy, int64_t M, int K, int N,
                int epi, hipStream_t st) {
    const dim3 grid((unsigned)((M + GEMM_BM - 1) / GEMM_BM), (unsigned)(N / GEMM_BN));
    if (epi == GEMM_EPI_NONE) hipLaunchKernelGGL((vit_gemm_kernel<T, GEMM_EPI_NONE>), grid, dim3(256), 0, st, x, ldx, W, bias, resid, ldr, y, ldy, M, K, N);
    else if (epi == GEMM_EPI_GELU) hipLaunchKernelGGL((vit_gemm_kernel<T, GEMM_EPI_GELU>), grid, dim3(256), 0, st, x, ldx, W, bias, resid, ldr, y, ldy, M, K, N);
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

template <typename T>
__global__ __launch_bounds__(256) void vit_attention_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
                                                            int64_t ldq, int64_t ldk, int64_t ldv, int64_t bsq, int64_t bsk, int64_t bsv, int N, int Nq,
                                                            float scale_log2e) {
    using G = AttGeom<T>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    __shared__ __attribute__((aligned(16))) T Ks[G::KS];
    __shared__ __attribute__((aligned(16))) T Vs[G::VS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int qrow = blockIdx.x * 128 + wave * 32 + r;
    const int qld = qrow < Nq ? qrow : Nq - 1;
    const T* kb = k + b * bsk + head * VIT_HD;
    const T* vb = v + b * bsv + head * VIT_HD;

    // Q fragment of this lane, kept for the whole key loop: bf16 k order natural (16 s + 8 h + j), fp32 k = 16 h + i
    bf16x8 qf[2];
    float qs[16];
    {
        const T* qp = q + b * bsq + (int64_t)qld * ldq + head * VIT_HD;
        if constexpr (BF) {
            qf[0] = *(const bf16x8*)(qp + 8 * h);
            qf[1] = *(const bf16x8*)(qp + 16 + 8 * h);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float4 a = *(const float4*)(qp + 16 * h + 4 * c);
                qs[4 * c] = a.x; qs[4 * c + 1] = a.y; qs[4 * c + 2] = a.z; qs[4 * c + 3] = a.w;
            }
        }
    }
    uint4 rk[G::NR], rv[G::NR];
    auto fetch = [&](int kt0) {
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            const int key = BF ? (p >> 2) : (p >> 3), piece = BF ? (p & 3) : (p & 7);
            const int gk = kt0 + key;
            if (gk < N) {
                rk[i] = *(const uint4*)(kb + (int64_t)gk * ldk + piece * (16 / (int)sizeof(T)));
                rv[i] = *(const uint4*)(vb + (int64_t)gk * ldv + piece * (16 / (int)sizeof(T)));
            } else {
                rk[i] = make_uint4(0, 0, 0, 0);
                rv[i] = make_uint4(0, 0, 0, 0);
            }
        }
    };
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    float m_run = -__builtin_inff(), l_run = 0.f;
    fetch(0);
    for (int kt0 = 0; kt0 < N; kt0 += ATT_KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            if constexpr (BF) {
                const int key = p >> 2, piece = p & 3;
                *(uint4*)(Ks + key * G::KP + piece * 8) = rk[i];
                const bf16x8 vv = __builtin_bit_cast(bf16x8, rv[i]);
#pragma unroll
                for (int e = 0; e < 8; ++e) Vs[(piece * 8 + e) * G::VP + key] = vv[e];
            } else {
                const int key = p >> 3, piece = p & 7;
                *(uint4*)(Ks + key * G::KP + piece * 4) = rk[i];
                *(uint4*)(Vs + key * G::VP + piece * 4) = rv[i];
            }
        }
        __syncthreads();
        if (kt0 + ATT_KT < N) fetch(kt0 + ATT_KT);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int key0 = kt0 + sub * 32;
            if (key0 >= N) break;                           // uniform over the workgroup
            f32x16 sc;
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = 0.f;
            if constexpr (BF) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 a = *(const bf16x8*)(Ks + (sub * 32 + r) * G::KP + 16 * s + 8 * h);
                    sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], sc, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float a[4];
                    load_f32((const float*)Ks + (sub * 32 + r) * G::KP + 16 * h + 4 * c, a);
#pragma unroll
                    for (int u = 0; u < 4; ++u) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], qs[4 * c + u], sc, 0, 0, 0);
                }
            }
            float p[16];
            float mx = -__builtin_inff();
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                p[e] = (key0 + crow(e, h) < N) ? sc[e] * scale_log2e : -__builtin_inff();
                mx = fmaxf(mx, p[e]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);           // finite: key0 < N, so the sub-tile has at least one live key
            const float alpha = exp2f(m_run - m_new);       // first tile: exp2(-inf) = 0
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                p[e] = exp2f(p[e] - m_new);
                ls += p[e];
            }
            l_run = l_run * alpha + ls;
            m_run = m_new;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e] *= alpha;
            if constexpr (BF) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint4 pk = make_uint4(pack2_bf16(p[8 * s], p[8 * s + 1]), pack2_bf16(p[8 * s + 2], p[8 * s + 3]),
                                                pack2_bf16(p[8 * s + 4], p[8 * s + 5]), pack2_bf16(p[8 * s + 6], p[8 * s + 7]));
                    const uint2 v0 = *(const uint2*)(Vs + r * G::VP + sub * 32 + 16 * s + 4 * h);
                    const uint2 v1 = *(const uint2*)(Vs + r * G::VP + sub * 32 + 16 * s + 8 + 4 * h);
                    const bf16x8 a = __builtin_bit_cast(bf16x8, make_uint4(v0.x, v0.y, v1.x, v1.y));
                    o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, pk), o, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float a = ((const float*)Vs)[(sub * 32 + crow(e, h)) * G::VP + r];
                    o = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[e], o, 0, 0, 0);
                }
            }
        }
    }
    const float l = l_run + __shfl_xor(l_run, 32, 64);
    if (qrow >= Nq) return;
    T* op = out + (b * Nq + qrow) * VIT_DIM + head * VIT_HD;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = o[4 * g + e] / l;
        store_from_f32(op + 8 * g + 4 * h, w);
    }
}

}  // namespace

extern "C" int cvae_vit_tokens(const void* stem, int stem_dtype, const float* cls, const float* pos, float* tokens, int64_t B, int64_t n_patches, void* stream) {
    if (B < 1 || n_patches < 1 || B * (n_patches + 1) > ((int64_t)1 << 32)) return CVAE_E_BADSHAPE;
    if (stem_dtype != CVAE_F32 && stem_dtype != CVAE_BF16) return CVAE_E_DTYPE;
    if (!stem || !cls || !pos || !tokens) return CVAE_E_NULLPTR;
    if (!aligned16(stem) || !aligned16(cls) || !aligned16(pos) || !aligned16(tokens)) return CVAE_E_UNSUPPORTED;
    const int blocks = cvae_grid_1d(B * (n_patches + 1) * (VIT_DIM / 4), 256, 256 * 32);
    if (stem_dtype == CVAE_BF16)
        hipLaunchKernelGGL(vit_tokens_kernel<bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)stem, cls, pos, tokens, B, n_patches);
    else
        hipLaunchKernelGGL(vit_tokens_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)stem, cls, pos, tokens, B, n_patches);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" int cvae_layernorm256(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* y, int64_t rows, float eps, int out_dtype, void* stream) {
    if (rows < 1 || rows > ((int64_t)1 << 32) || x_stride < VIT_DIM || (x_stride & 3)) return CVAE_E_BADSHAPE;
    if (out_dtype != CVAE_F32 && out_dtype != CVAE_BF16) return CVAE_E_DTYPE;
    if (!x || !gamma || !beta || !y) return CVAE_E_NULLPTR;
    if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(y)) return CVAE_E_UNSUPPORTED;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (out_dtype == CVAE_BF16) hipLaunchKernelGGL(vit_layernorm_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, x, x_stride, gamma, beta, (bf16*)y, rows, eps);
    else hipLaunchKernelGGL(vit_layernorm_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x, x_stride, gamma, beta, (float*)y, rows, eps);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" int cvae_token_gemm(const void* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, void* y,
                               int64_t y_stride, int64_t M, int64_t K, int64_t N, int epilogue, int dtype, void* stream) {
    if (M < 1 || M > ((int64_t)1 << 30) || x_stride < K || y_stride < N) return CVAE_E_BADSHAPE;
    if (dtype != CVAE_F32 && dtype != CVAE_BF16) return CVAE_E_DTYPE;
    if (epilogue < CVAE_GEMM_EPI_NONE || epilogue > CVAE_GEMM_EPI_RESIDUAL) return CVAE_E_BADSHAPE;
    if (!((K == 256 && (N == 768 || N == 256 || N == 512)) || (K == 512 && N == 256))) return CVAE_E_UNSUPPORTED;
    if (!x || !W || !bias || !y) return CVAE_E_NULLPTR;
    if (epilogue == CVAE_GEMM_EPI_RESIDUAL && (!resid || resid_stride < N || (resid_stride & 3) || !aligned16(resid))) return resid ? CVAE_E_BADSHAPE : CVAE_E_NULLPTR;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4, ye16 = (epilogue == CVAE_GEMM_EPI_RESIDUAL || dtype == CVAE_F32) ? 4 : 8;
    if ((x_stride % e16) || (y_stride % ye16) || !aligned16(x) || !aligned16(W) || !aligned16(bias) || !aligned16(y)) return CVAE_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CVAE_BF16) return gemm_launch<bf16>((const bf16*)x, x_stride, W, bias, resid, resid_stride, y, y_stride, M, (int)K, (int)N, epilogue, st);
    return gemm_launch<float>((const float*)x, x_stride, W, bias, resid, resid_stride, y, y_stride, M, (int)K, (int)N, epilogue, st);
}

extern "C" int cvae_mhsa_fwd(const void* q, const void* k, const void* v, void* out, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride,
                             int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype, void* stream) {
    if (B < 1 || B > 65535 || n_tokens < 1 || n_tokens > ((int64_t)1 << 24) || n_query_rows < 1 || n_query_rows > n_tokens) return CVAE_E_BADSHAPE;
    if (dtype != CVAE_F32 && dtype != CVAE_BF16) return CVAE_E_DTYPE;
    if (!q || !k || !v || !out) return CVAE_E_NULLPTR;
    const int64_t e16 = dtype == CVAE_BF16 ? 8 : 4;
    if (q_stride < VIT_DIM || k_stride < VIT_DIM || v_stride < VIT_DIM || q_batch_stride < 0 || k_batch_stride < 0 || v_batch_stride < 0) return CVAE_E_BADSHAPE;
    if ((q_stride % e16) || (k_stride % e16) || (v_stride % e16) || (q_batch_stride % e16) || (k_batch_stride % e16) || (v_batch_stride % e16) || !aligned16(q) ||
        !aligned16(k) || !aligned16(v) || !aligned16(out))
        return CVAE_E_UNSUPPORTED;
    const dim3 grid((unsigned)((n_query_rows + 127) / 128), VIT_HEADS, (unsigned)B);
    const float scale_log2e = 0.17677669529663688110f * 1.44269504088896340736f;       // 1 / sqrt(32) * log2(e)
    if (dtype == CVAE_BF16)
        hipLaunchKernelGGL(vit_attention_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)out, q_stride,
                           k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, (int)n_tokens, (int)n_query_rows, scale_log2e);
    else
        hipLaunchKernelGGL(vit_attention_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)q, (const float*)k, (const float*)v, (float*)out,
                           q_stride, k_stride, v_stride, q_batch_stride, k_batch_stride, v_batch_stride, (int)n_tokens, (int)n_query_rows, scale_log2e);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
