// vit_attention.inc — the fused attention kernel's text, included twice by vit.hip: as vit_attention_kernel (VIT_ATT_TRAIN 0: the inference kernel, its signature
// and machine code as they were), as vit_attention_train_kernel (VIT_ATT_TRAIN 1: + one fp32 row statistic per (batch, head, query) for the backward) and as
// vit_attention_dropout_kernel (VIT_ATT_TRAIN 2: + dropout on the probabilities: the row statistics are those of the undropped row, the dropped p[e] are zeroed
// between the row sum and the P V product, and the kept ones' scale 1 / (1 - p) multiplies the output row once, next to 1 / l).
template <typename T>
__global__ __launch_bounds__(256) void VIT_ATT_KERNEL(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
                                                            int64_t ldq, int64_t ldk, int64_t ldv, int64_t bsq, int64_t bsk, int64_t bsv, int N, int Nq,
                                                            float scale_log2e
#if VIT_ATT_TRAIN
                                                            , float* __restrict__ lse
#endif
#if VIT_ATT_TRAIN == 2
                                                            , const DropArgs drop_arg, const uint32_t* key_dev
#endif
) {
#if VIT_ATT_TRAIN == 2
    const DropArgs drop = drop_with_key(drop_arg, key_dev);
#endif
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
#if VIT_ATT_TRAIN == 2
#pragma unroll
            for (int g = 0; g < 4; ++g) {                   // registers 4 g .. 4 g + 3 are keys key0 + 8 g + 4 h + (0 .. 3): one Philox call
                uint32_t mw[4];
                drop_words(drop, (uint32_t)((key0 + 8 * g + 4 * h) >> 2), (uint32_t)qld, (uint32_t)(b * VIT_HEADS + head), mw);
#pragma unroll
                for (int e = 0; e < 4; ++e) p[4 * g + e] = drop_keep(drop, mw[e]) ? p[4 * g + e] : 0.f;
            }
#endif
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
#if VIT_ATT_TRAIN
    if (h == 0) lse[(b * VIT_HEADS + head) * Nq + qrow] = m_run + log2f(l);       // log2 of the row's sum of 2^(score): the backward's P = 2^(s - lse)
#endif
    T* op = out + (b * Nq + qrow) * VIT_DIM + head * VIT_HD;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = o[4 * g + e] / l;
#if VIT_ATT_TRAIN == 2
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] *= drop.scale;
#endif
        store_from_f32(op + 8 * g + 4 * h, w);
    }
}
