// vit_attention_grad_probe.inc — the gradient of a target with respect to the attention probabilities, and gradient-weighted attention relevance (DESIGN.md
// section 22), one text in two modes, included once by vit.hip:
//   GRADP_HEADS      w[b][head][i][j] = gA[b][head][i][j] = sum_{d < 32} dO[b][i][32 head + d] V[b][j][32 head + d]      (cvae_mhsa_weight_grads; head = blockIdx.y)
//   GRADP_RELEVANCE  part[b][c][j] = sum_{i in chunk c} r[b][i] Abar[b][i][j],  Abar = 0.125 sum_h max(0, gA P)        (cvae_mhsa_relevance_step; c = blockIdx.y)
// gA is the gradient with respect to the probabilities taken as a free variable (out = A V), what a hook on the softmax output receives; P is recomputed as in
// vit_attention_probe.inc, P = 2^(s log2e / sqrt(32) - lse).  The arrangement is that kernel's, with the dk / dv pass's second product: the KEY is on the lane, a
// workgroup owns 128 keys of one batch row, a wave 32 of them; the query tile AND the dO tile of the current (query tile, head) pair are staged in LDS, the lane's
// own key and value fragments stay in registers, and per 32 x 32 sub-tile two MFMA chains run: S = Q K^T and gA = dO V^T.  Lane (r, h) then holds, for key r, both
// values of queries crow(e, h), so
//   * a store of register e is 32 consecutive floats of one row of w per lane half: plain 4-byte stores, rows are n_tokens floats, dense;
//   * the relevance's head sum stays in the lane: acc = (((t_0 + t_1) + ...) + t_7), t_h = max(0, gA_h P_h), then col += r[i] (acc * 0.125f) in the order
//     (sub-tile, register), the two lane halves joined once at the end.
// The relevance step is NOT the rollout step's launch shape (one workgroup walking every query tile): a workgroup takes GRADP_CHUNK_TILES query tiles (chunk
// blockIdx.y) and leaves its key's partial sum in part[b][chunk][key]; vit_relevance_finish_kernel adds the chunks in order and the r[j] term.  With one chunk the
// kernel writes out = r + sum itself.  No atomics, no ticket; every order depends on n_tokens and n_query_rows only.  Query rows past n_query_rows are staged as
// zeros with P = 0; keys past n_tokens are clamped on load and never stored.
#define GRADP_HEADS 0
#define GRADP_RELEVANCE 1
#define GRADP_CHUNK_TILES 1                               // query tiles (of ATT_KT rows) per relevance workgroup
struct AttGradProbeArgs {
    const void *q, *k, *v, *dout;                         // dout: dense [B][Nq][256]
    int64_t ldq, ldk, ldv, bsq, bsk, bsv;
    const float* lse;                                     // [B][8][Nq]
    const float* r;                                       // [B][N]
    float* out;                                           // w; or part [B][chunks][N]; or, with one chunk, the relevance's out [B][N]
    int64_t bs_out;                                       // w's batch stride
    int N, Nq;
    float scale_log2e;
};

template <typename T, int MODE>
__global__ __launch_bounds__(256) void vit_attention_grad_probe_kernel(const AttGradProbeArgs a) {
    using G = AttBwdGeom<T>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    constexpr bool REL = MODE == GRADP_RELEVANCE;
    constexpr int NH = REL ? VIT_HEADS : 1;
    __shared__ __attribute__((aligned(16))) T Qs[REL ? G::NS : 8];
    __shared__ __attribute__((aligned(16))) T Gs[G::NS];
    __shared__ float Ls[ATT_KT], Rs[ATT_KT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int head0 = REL ? 0 : blockIdx.y;
    const int64_t b = blockIdx.z;
    const int krow = blockIdx.x * 128 + wave * 32 + r;
    const int kld = krow < a.N ? krow : a.N - 1;
    const T* kp = REL ? (const T*)a.k + b * a.bsk + (int64_t)kld * a.ldk : nullptr;
    const T* vp = (const T*)a.v + b * a.bsv + (int64_t)kld * a.ldv;
    const T* qb = REL ? (const T*)a.q + b * a.bsq : nullptr;
    const T* gb = (const T*)a.dout + b * (int64_t)a.Nq * VIT_DIM;
    const int ntiles = (a.Nq + ATT_KT - 1) / ATT_KT;
    const int tile0 = REL ? blockIdx.y * GRADP_CHUNK_TILES : 0;
    const int mytiles = REL ? (ntiles - tile0 < GRADP_CHUNK_TILES ? ntiles - tile0 : GRADP_CHUNK_TILES) : ntiles;
    const int niter = mytiles * NH;

    // the pair in flight: its query and dO tiles (16-byte pieces), row statistics and this lane's key and value fragments (k order as in vit_attention_probe.inc)
    uint4 rq[G::NR], rg[G::NR];
    float rl = 0.f, rr = 0.f;
    bf16x8 nkf[2], nvf[2], kf[2], vf[2];
    float nks[16], nvs[16], ks[16], vs[16];
    auto fetch = [&](int it) {
        const int tile = tile0 + it / NH, head = head0 + (it - (it / NH) * NH);
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            const int row = BF ? (p >> 2) : (p >> 3), piece = BF ? (p & 3) : (p & 7);
            const int gr = tile * ATT_KT + row;
            const int col = head * VIT_HD + piece * (16 / (int)sizeof(T));
            if constexpr (REL) rq[i] = gr < a.Nq ? *(const uint4*)(qb + (int64_t)gr * a.ldq + col) : make_uint4(0, 0, 0, 0);
            rg[i] = gr < a.Nq ? *(const uint4*)(gb + (int64_t)gr * VIT_DIM + col) : make_uint4(0, 0, 0, 0);
        }
        if constexpr (REL) {
            if (t < ATT_KT) {
                const int gr = tile * ATT_KT + t;
                rl = gr < a.Nq ? a.lse[(b * VIT_HEADS + head) * a.Nq + gr] : 0.f;
                rr = gr < a.Nq ? a.r[b * a.N + gr] : 0.f;
            }
        }
        if constexpr (BF) {
            if constexpr (REL) {
                nkf[0] = *(const bf16x8*)(kp + head * VIT_HD + 8 * h);
                nkf[1] = *(const bf16x8*)(kp + head * VIT_HD + 16 + 8 * h);
            }
            nvf[0] = *(const bf16x8*)(vp + head * VIT_HD + 8 * h);
            nvf[1] = *(const bf16x8*)(vp + head * VIT_HD + 16 + 8 * h);
        } else {
            if constexpr (REL) load_f32(kp + head * VIT_HD + 16 * h, nks);
            load_f32(vp + head * VIT_HD + 16 * h, nvs);
        }
    };
    float acc[2][16];                                     // gA of the current tile (GRADP_HEADS), or the relevance's head sums of it
    float col = 0.f;                                      // the relevance's column sum of this lane half
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[sub][e] = 0.f;
    fetch(0);
    for (int it = 0; it < niter; ++it) {
        const int tile = tile0 + it / NH, hi = it - (it / NH) * NH;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            const int o = BF ? (p >> 2) * G::NP + (p & 3) * 8 : (p >> 3) * G::NP + (p & 7) * 4;
            if constexpr (REL) *(uint4*)(Qs + o) = rq[i];
            *(uint4*)(Gs + o) = rg[i];
        }
        if constexpr (REL) {
            if (t < ATT_KT) {
                Ls[t] = rl;
                Rs[t] = rr;
            }
        }
        if constexpr (BF) {
            if constexpr (REL) {
                kf[0] = nkf[0];
                kf[1] = nkf[1];
            }
            vf[0] = nvf[0];
            vf[1] = nvf[1];
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if constexpr (REL) ks[e] = nks[e];
                vs[e] = nvs[e];
            }
        }
        __syncthreads();
        if (it + 1 < niter) fetch(it + 1);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int row0 = tile * ATT_KT + sub * 32;
            if (row0 < a.Nq) {                              // uniform over the workgroup
                f32x16 sc, ga;
#pragma unroll
                for (int e = 0; e < 16; ++e) sc[e] = 0.f, ga[e] = 0.f;
                if constexpr (BF) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o = (sub * 32 + r) * G::NP + 16 * s + 8 * h;
                        if constexpr (REL) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Qs + o), kf[s], sc, 0, 0, 0);
                        ga = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Gs + o), vf[s], ga, 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int o = (sub * 32 + r) * G::NP + 16 * h + 4 * c;
                        float x[4], y[4];
                        if constexpr (REL) load_f32((const float*)Qs + o, x);
                        load_f32((const float*)Gs + o, y);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if constexpr (REL) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u], ks[4 * c + u], sc, 0, 0, 0);
                            ga = __builtin_amdgcn_mfma_f32_32x32x2f32(y[u], vs[4 * c + u], ga, 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if constexpr (REL) {
                        const int wr = sub * 32 + crow(e, h);
                        const float p = (tile * ATT_KT + wr < a.Nq) ? exp2f(sc[e] * a.scale_log2e - Ls[wr]) : 0.f;
                        const float term = fmaxf(0.f, ga[e] * p);
                        acc[sub][e] = hi == 0 ? term : acc[sub][e] + term;
                    } else {
                        acc[sub][e] = ga[e];
                    }
                }
                if constexpr (REL) {
                    if (hi == NH - 1) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) col += Rs[sub * 32 + crow(e, h)] * (acc[sub][e] * 0.125f);
                    }
                }
            }
        }
        if constexpr (!REL) {
            if (krow < a.N) {
                float* wp = a.out + b * a.bs_out + (int64_t)head0 * a.Nq * a.N + krow;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int qi = tile * ATT_KT + sub * 32 + crow(e, h);
                        if (qi < a.Nq) wp[(int64_t)qi * a.N] = acc[sub][e];
                    }
            }
        }
    }
    if constexpr (REL) {
        const float tot = col + __shfl_xor(col, 32, 64);
        if (h == 0 && krow < a.N) {
            if (gridDim.y == 1) a.out[b * a.N + krow] = a.r[b * a.N + krow] + tot;
            else a.out[(b * gridDim.y + blockIdx.y) * a.N + krow] = tot;
        }
    }
}

// out[b][j] = r[b][j] + (((part[b][0][j] + part[b][1][j]) + ...) + part[b][S-1][j]): the chunks in index order, then the one add of r
__global__ __launch_bounds__(256) void vit_relevance_finish_kernel(const float* __restrict__ part, const float* __restrict__ r, float* __restrict__ out, int S, int N,
                                                                    int64_t total) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / N, j = idx - b * N;
        const float* p = part + b * S * N + j;
        float s = p[0];
        for (int c = 1; c < S; ++c) s += p[(int64_t)c * N];
        out[idx] = r[idx] + s;
    }
}
