// vit_attention_probe.inc — the two kernels that look inside the encoder's attention (DESIGN.md section 20), one text in three modes, included once by vit.hip:
//   PROBE_HEADS    w[b][head][i][j] = P[b][head][i][j]                                          (cvae_mhsa_weights, average_heads = 0; head = blockIdx.y)
//   PROBE_AVERAGE  w[b][i][j] = ((((P_0 + P_1) + P_2) + ...) + P_7) * 0.125f                     (cvae_mhsa_weights, average_heads = 1)
//   PROBE_ROLLOUT  out[b][j] = residual r[b][j] + (1 - residual) 0.125 sum_h sum_i r[b][i] P[b][h][i][j]   (cvae_mhsa_rollout_step)
// P is recomputed as the backward recomputes it: P = 2^(s log2e / sqrt(32) - lse) from q, k and the forward's row statistic; no max or sum pass.
// All three put the KEY on the lane and walk the queries (the dk / dv pass of vit_attention_bwd.inc: A = the staged query tile, B = the lane's own key
// fragment): a workgroup owns 128 keys of one batch row, a wave 32 of them, and lane (r, h) holds, for key r, the probabilities of queries crow(e, h).
//   * a store of register e is then 32 consecutive floats of ONE row of w per lane half — plain 4-byte stores, so a row start needs no alignment
//     (rows are n_tokens floats, dense) and the writes still coalesce;
//   * the rollout's column sum stays in the lane: a += r[i] p in the order (query tile, head, sub-tile, register), the two lane halves joined once at the end.
// The walk is over (query tile, head) pairs, head innermost: the averaged form keeps one tile of sums in registers across the 8 heads and stores it once.
// The next pair's query tile, row statistics and key fragment are in flight during the current pair's arithmetic.  Query rows past n_query_rows are staged
// as zeros with P = 0; keys past n_tokens are clamped on load and never stored.  No atomics; every order above depends on n_tokens and n_query_rows only.
#define PROBE_HEADS 0
#define PROBE_AVERAGE 1
#define PROBE_ROLLOUT 2
struct AttProbeArgs {
    const void *q, *k;
    int64_t ldq, ldk, bsq, bsk;
    const float* lse;                                     // [B][8][Nq]
    const float* r;                                       // rollout: [B][N]
    float* out;                                           // w, or the rollout's out [B][N]
    int64_t bs_out;                                       // w's batch stride
    int N, Nq;
    float scale_log2e, residual;
};

template <typename T, int MODE>
__global__ __launch_bounds__(256) void vit_attention_probe_kernel(const AttProbeArgs a) {
    using G = AttBwdGeom<T>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    constexpr int NH = MODE == PROBE_HEADS ? 1 : VIT_HEADS;
    __shared__ __attribute__((aligned(16))) T Qs[G::NS];
    __shared__ float Ls[ATT_KT], Rs[ATT_KT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int head0 = MODE == PROBE_HEADS ? blockIdx.y : 0;
    const int64_t b = blockIdx.z;
    const int krow = blockIdx.x * 128 + wave * 32 + r;
    const int kld = krow < a.N ? krow : a.N - 1;
    const T* kp = (const T*)a.k + b * a.bsk + (int64_t)kld * a.ldk;
    const T* qb = (const T*)a.q + b * a.bsq;
    const int niter = ((a.Nq + ATT_KT - 1) / ATT_KT) * NH;

    // the pair in flight: its query tile (16-byte pieces), row statistics and this lane's key fragment (bf16 k order natural 16 s + 8 h + j, fp32 k = 16 h + i)
    uint4 rq[G::NR];
    float rl = 0.f, rr = 0.f;
    bf16x8 nf[2], kf[2];
    float ns[16], ks[16];
    auto fetch = [&](int it) {
        const int tile = it / NH, head = head0 + (it - tile * NH);
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            const int row = BF ? (p >> 2) : (p >> 3), piece = BF ? (p & 3) : (p & 7);
            const int gr = tile * ATT_KT + row;
            rq[i] = gr < a.Nq ? *(const uint4*)(qb + (int64_t)gr * a.ldq + head * VIT_HD + piece * (16 / (int)sizeof(T))) : make_uint4(0, 0, 0, 0);
        }
        if (t < ATT_KT) {
            const int gr = tile * ATT_KT + t;
            rl = gr < a.Nq ? a.lse[(b * VIT_HEADS + head) * a.Nq + gr] : 0.f;
            if constexpr (MODE == PROBE_ROLLOUT) rr = gr < a.Nq ? a.r[b * a.N + gr] : 0.f;
        }
        if constexpr (BF) {
            nf[0] = *(const bf16x8*)(kp + head * VIT_HD + 8 * h);
            nf[1] = *(const bf16x8*)(kp + head * VIT_HD + 16 + 8 * h);
        } else {
            load_f32(kp + head * VIT_HD + 16 * h, ns);
        }
    };
    float acc[2][16];                                     // the averaged form's head sums of the current query tile
    float col = 0.f;                                      // the rollout's column sum of this lane half
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[sub][e] = 0.f;
    fetch(0);
    for (int it = 0; it < niter; ++it) {
        const int tile = it / NH, hi = it - tile * NH;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            if constexpr (BF) *(uint4*)(Qs + (p >> 2) * G::NP + (p & 3) * 8) = rq[i];
            else *(uint4*)(Qs + (p >> 3) * G::NP + (p & 7) * 4) = rq[i];
        }
        if (t < ATT_KT) {
            Ls[t] = rl;
            if constexpr (MODE == PROBE_ROLLOUT) Rs[t] = rr;
        }
        if constexpr (BF) {
            kf[0] = nf[0];
            kf[1] = nf[1];
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) ks[e] = ns[e];
        }
        __syncthreads();
        if (it + 1 < niter) fetch(it + 1);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int row0 = tile * ATT_KT + sub * 32;
            if (row0 < a.Nq) {                              // uniform over the workgroup
                f32x16 sc;
#pragma unroll
                for (int e = 0; e < 16; ++e) sc[e] = 0.f;
                if constexpr (BF) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const bf16x8 x = *(const bf16x8*)(Qs + (sub * 32 + r) * G::NP + 16 * s + 8 * h);
                        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, kf[s], sc, 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float x[4];
                        load_f32((const float*)Qs + (sub * 32 + r) * G::NP + 16 * h + 4 * c, x);
#pragma unroll
                        for (int u = 0; u < 4; ++u) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u], ks[4 * c + u], sc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int wr = sub * 32 + crow(e, h);
                    const float p = (tile * ATT_KT + wr < a.Nq) ? exp2f(sc[e] * a.scale_log2e - Ls[wr]) : 0.f;
                    if constexpr (MODE == PROBE_ROLLOUT) col += Rs[wr] * p;
                    else acc[sub][e] = hi == 0 ? p : acc[sub][e] + p;
                }
            }
        }
        if constexpr (MODE != PROBE_ROLLOUT) {
            if (hi == NH - 1 && krow < a.N) {
                float* wp = a.out + b * a.bs_out + (int64_t)head0 * a.Nq * a.N + krow;     // head0 = 0 in the averaged form
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int qi = tile * ATT_KT + sub * 32 + crow(e, h);
                        if (qi < a.Nq) wp[(int64_t)qi * a.N] = MODE == PROBE_AVERAGE ? acc[sub][e] * 0.125f : acc[sub][e];
                    }
            }
        }
    }
    if constexpr (MODE == PROBE_ROLLOUT) {
        const float tot = col + __shfl_xor(col, 32, 64);
        if (h == 0 && krow < a.N) a.out[b * a.N + krow] = a.residual * a.r[b * a.N + krow] + (1.f - a.residual) * 0.125f * tot;
    }
}
