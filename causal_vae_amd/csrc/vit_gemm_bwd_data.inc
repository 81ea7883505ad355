// vit_gemm_bwd_data.inc — the token GEMM's data-gradient kernel's text, included twice by vit.hip: as vit_gemm_bwd_data_kernel (VIT_GEMM_BWD_DROP 0: signature
// and machine code as they were) and as vit_gemm_bwd_data_dropout_kernel (VIT_GEMM_BWD_DROP 1: + a row-site dropout mask on the product, before the gate).
template <typename T, typename TG, typename TO>
__global__ __launch_bounds__(256) void VIT_GEMM_BWD_DATA_KERNEL(const TG* __restrict__ g, int64_t ldg, const float* __restrict__ W, const T* __restrict__ pre,
                                                                int64_t ldp, const float* resid, int64_t ldr, TO* dx, int64_t lddx, int64_t M, int K, int N
#if VIT_GEMM_BWD_DROP
                                                                , const DropArgs drop_arg, int64_t mask_row0, int64_t mask_row_step, const uint32_t* key_dev
#endif
) {
#if VIT_GEMM_BWD_DROP
    const DropArgs drop = drop_with_key(drop_arg, key_dev);
#endif
    using G = GemmGeom<T>;
    constexpr int NP = G::KC / 8;                         // 4-element pieces of g per thread and chunk
    __shared__ __attribute__((aligned(16))) T xs[GEMM_BM * G::PITCH];
    __shared__ __attribute__((aligned(16))) T ws[GEMM_BN * G::PITCH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int64_t m0 = blockIdx.x * (int64_t)GEMM_BM;
    const int k0 = blockIdx.y * GEMM_BN;                  // output columns of this workgroup
    float rg[NP][4];
    float4 rw[G::WP];
    auto fetch = [&](int n0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = t + 256 * i, row = p / (G::KC / 4), piece = p % (G::KC / 4);
            const int64_t gm = m0 + row;
            if (gm < M) load_f32(g + gm * ldg + n0 + piece * 4, rg[i]);
            else rg[i][0] = rg[i][1] = rg[i][2] = rg[i][3] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < G::WP; ++i) {
            const int p = t + 256 * i, n = p >> 4, piece = p & 15;
            rw[i] = *(const float4*)(W + (int64_t)(n0 + n) * K + k0 + piece * 4);
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    fetch(0);
    for (int n0 = 0; n0 < N; n0 += G::KC) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = t + 256 * i, row = p / (G::KC / 4), piece = p % (G::KC / 4);
            lds_put_w(xs + row * G::PITCH + piece * 4, make_float4(rg[i][0], rg[i][1], rg[i][2], rg[i][3]));
        }
#pragma unroll
        for (int i = 0; i < G::WP; ++i) {
            const int p = t + 256 * i, n = p >> 4, piece = p & 15;
            ws[(piece * 4 + 0) * G::PITCH + n] = from_f32<T>(rw[i].x);
            ws[(piece * 4 + 1) * G::PITCH + n] = from_f32<T>(rw[i].y);
            ws[(piece * 4 + 2) * G::PITCH + n] = from_f32<T>(rw[i].z);
            ws[(piece * 4 + 3) * G::PITCH + n] = from_f32<T>(rw[i].w);
        }
        __syncthreads();
        if (n0 + G::KC < N) fetch(n0 + G::KC);
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
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + j * 32 + 8 * q + 4 * h;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[j][4 * q + e];
#if VIT_GEMM_BWD_DROP
            uint32_t mw[4];
            drop_row_words(drop, mask_row0 + gm * mask_row_step, k, mw);
            drop_apply4(drop, mw, v);
#endif
            if (pre) {
                float pv[4];
                load_f32(pre + gm * ldp + k, pv);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= gelu_erf_grad(pv[e]);
            }
            if (resid) {
                float rv[4];
                load_f32(resid + gm * ldr + k, rv);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rv[e] + v[e];
            }
            store_from_f32(dx + gm * lddx + k, v);
        }
}
