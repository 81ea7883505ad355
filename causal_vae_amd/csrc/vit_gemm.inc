// vit_gemm.inc — the token GEMM kernel's text, included twice by vit.hip: as vit_gemm_kernel (VIT_GEMM_TRAIN 0: the inference kernel, its signature and machine
// code as they were), as vit_gemm_train_kernel (VIT_GEMM_TRAIN 1: + the pre-activation's pointer and stride, stored by the GELU_SAVE epilogue) and as
// vit_gemm_dropout_kernel (VIT_GEMM_TRAIN 2: + a row-site dropout mask on what the GELU_SAVE epilogue stores as y, or on the product the RESID epilogue adds
// to the residual).  An include and not a shared device function: the function form moved scalar instructions in every inference instance
// (tools/kernel_isa_diff.py).
template <typename T, int EPI>
__global__ __launch_bounds__(256) void VIT_GEMM_KERNEL(const T* __restrict__ x, int64_t ldx, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* resid, int64_t ldr, void* yv, int64_t ldy, int64_t M, int K, int N
#if VIT_GEMM_TRAIN
                                                       , T* __restrict__ pre, int64_t ldp
#endif
#if VIT_GEMM_TRAIN == 2
                                                       , const DropArgs drop_arg, int64_t mask_row0, int64_t mask_row_step, const uint32_t* key_dev
#endif
) {
#if VIT_GEMM_TRAIN == 2
    const DropArgs drop = drop_with_key(drop_arg, key_dev);
#endif
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
#if VIT_GEMM_TRAIN == 2
            uint32_t mw[4];
            drop_row_words(drop, mask_row0 + gm * mask_row_step, n, mw);
#endif
            if (EPI == GEMM_EPI_RESID) {
                float rv[4];
#if VIT_GEMM_TRAIN == 2
                drop_apply4(drop, mw, v);
#endif
                load_f32(resid + gm * ldr + n, rv);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rv[e] + v[e];
                store_from_f32((float*)yv + gm * ldy + n, v);
            } else {
#if VIT_GEMM_TRAIN
                if (EPI == GEMM_EPI_GELU_SAVE) store_from_f32(pre + gm * ldp + n, v);
#endif
                if (EPI == GEMM_EPI_GELU || EPI == GEMM_EPI_GELU_SAVE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
                }
#if VIT_GEMM_TRAIN == 2
                drop_apply4(drop, mw, v);
#endif
                store_from_f32((T*)yv + gm * ldy + n, v);
            }
        }
}
