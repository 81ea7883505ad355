// vit_attention_bwd.inc — the attention backward kernel's text, included twice by vit.hip: as vit_attention_bwd_kernel (VIT_ATT_BWD_DROP 0: signature and machine
// code as they were) and as vit_attention_bwd_dropout_kernel (VIT_ATT_BWD_DROP 1: the forward's dropout mask, recomputed per (query, key) from the token indices:
// dP = (dO V^T) keep scale, and dV takes P keep scale; P itself, lse and delta are those of the undropped row).
template <typename T, bool DKV>
__global__ __launch_bounds__(256) void VIT_ATT_BWD_KERNEL(const AttBwdArgs a
#if VIT_ATT_BWD_DROP
                                                          , const DropArgs drop_arg, const uint32_t* key_dev
#endif
) {
#if VIT_ATT_BWD_DROP
    const DropArgs drop = drop_with_key(drop_arg, key_dev);
#endif
    using G = AttBwdGeom<T>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    __shared__ __attribute__((aligned(16))) T W1n[G::NS];
    __shared__ __attribute__((aligned(16))) T W2n[G::NS];
    __shared__ __attribute__((aligned(16))) T W1t[G::TS];
    __shared__ __attribute__((aligned(16))) T W2t[G::TS];
    __shared__ float Ls[ATT_KT], Ds[ATT_KT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int orow = blockIdx.x * 128 + wave * 32 + r;
    const int old = orow < a.n_own ? orow : a.n_own - 1;
    const T* w1 = (const T*)a.walk1 + b * a.bs_w1 + head * VIT_HD;
    const T* w2 = (const T*)a.walk2 + b * a.bs_w2 + head * VIT_HD;
    const int64_t stat0 = (b * VIT_HEADS + head) * a.Nq;

    // own fragments, kept for the whole walk: bf16 k order natural (16 s + 8 h + j), fp32 k = 16 h + i
    bf16x8 f1[2], f2[2];
    float s1[16], s2[16];
    float lse_own = 0.f, delta_own = 0.f;
    {
        const T* p1 = (const T*)a.own1 + b * a.bs_o1 + (int64_t)old * a.ld_o1 + head * VIT_HD;
        const T* p2 = (const T*)a.own2 + b * a.bs_o2 + (int64_t)old * a.ld_o2 + head * VIT_HD;
        if constexpr (BF) {
            f1[0] = *(const bf16x8*)(p1 + 8 * h);
            f1[1] = *(const bf16x8*)(p1 + 16 + 8 * h);
            f2[0] = *(const bf16x8*)(p2 + 8 * h);
            f2[1] = *(const bf16x8*)(p2 + 16 + 8 * h);
        } else {
            load_f32(p1 + 16 * h, s1);
            load_f32(p2 + 16 * h, s2);
        }
        if constexpr (!DKV) {                             // delta of this lane's query row: its half of the 32 columns, then the other half's
            const T* po = (const T*)a.out + (b * a.Nq + old) * VIT_DIM + head * VIT_HD;
            float d = 0.f;
            if constexpr (BF) {
                float o0[8], o1[8];
                load_f32(po + 8 * h, o0);
                load_f32(po + 16 + 8 * h, o1);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += (float)f2[0][j] * o0[j];
#pragma unroll
                for (int j = 0; j < 8; ++j) d += (float)f2[1][j] * o1[j];
            } else {
                float o[16];
                load_f32(po + 16 * h, o);
#pragma unroll
                for (int j = 0; j < 16; ++j) d += s2[j] * o[j];
            }
            delta_own = d + __shfl_xor(d, 32, 64);
            lse_own = a.lse[stat0 + old];
            if (h == 0 && orow < a.n_own) a.delta[stat0 + orow] = delta_own;
        }
    }
    uint4 r1[G::NR], r2[G::NR];
    float rl = 0.f, rd = 0.f;
    auto fetch = [&](int wt0) {
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            const int row = BF ? (p >> 2) : (p >> 3), piece = BF ? (p & 3) : (p & 7);
            const int gr = wt0 + row;
            if (gr < a.n_walk) {
                r1[i] = *(const uint4*)(w1 + (int64_t)gr * a.ld_w1 + piece * (16 / (int)sizeof(T)));
                r2[i] = *(const uint4*)(w2 + (int64_t)gr * a.ld_w2 + piece * (16 / (int)sizeof(T)));
            } else {
                r1[i] = make_uint4(0, 0, 0, 0);
                r2[i] = make_uint4(0, 0, 0, 0);
            }
        }
        if (DKV && t < ATT_KT) {
            const int gr = wt0 + t;
            rl = gr < a.n_walk ? a.lse[stat0 + gr] : 0.f;
            rd = gr < a.n_walk ? a.delta[stat0 + gr] : 0.f;
        }
    };
    f32x16 acc1, acc2;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc1[e] = acc2[e] = 0.f;
    fetch(0);
    for (int wt0 = 0; wt0 < a.n_walk; wt0 += ATT_KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G::NR; ++i) {
            const int p = t + 256 * i;
            if constexpr (BF) {
                const int row = p >> 2, piece = p & 3;
                *(uint4*)(W1n + row * G::NP + piece * 8) = r1[i];
                *(uint4*)(W2n + row * G::NP + piece * 8) = r2[i];
                const bf16x8 v1 = __builtin_bit_cast(bf16x8, r1[i]), v2 = __builtin_bit_cast(bf16x8, r2[i]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    W1t[(piece * 8 + e) * G::TP + row] = v1[e];
                    if (DKV) W2t[(piece * 8 + e) * G::TP + row] = v2[e];
                }
            } else {
                const int row = p >> 3, piece = p & 7;
                *(uint4*)(W1n + row * G::NP + piece * 4) = r1[i];
                *(uint4*)(W2n + row * G::NP + piece * 4) = r2[i];
            }
        }
        if (DKV && t < ATT_KT) {
            Ls[t] = rl;
            Ds[t] = rd;
        }
        __syncthreads();
        if (wt0 + ATT_KT < a.n_walk) fetch(wt0 + ATT_KT);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int row0 = wt0 + sub * 32;
            if (row0 >= a.n_walk) break;                    // uniform over the workgroup
            f32x16 sc, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = dp[e] = 0.f;
            if constexpr (BF) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 x1 = *(const bf16x8*)(W1n + (sub * 32 + r) * G::NP + 16 * s + 8 * h);
                    const bf16x8 x2 = *(const bf16x8*)(W2n + (sub * 32 + r) * G::NP + 16 * s + 8 * h);
                    sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1, f1[s], sc, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2, f2[s], dp, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float x1[4], x2[4];
                    load_f32((const float*)W1n + (sub * 32 + r) * G::NP + 16 * h + 4 * c, x1);
                    load_f32((const float*)W2n + (sub * 32 + r) * G::NP + 16 * h + 4 * c, x2);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[u], s1[4 * c + u], sc, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(x2[u], s2[4 * c + u], dp, 0, 0, 0);
                    }
                }
            }
            float p[16], ds[16];
#if VIT_ATT_BWD_DROP
            bool keep[16];                                  // the forward's mask element (query, key) of each register
            const uint32_t bh = (uint32_t)(b * VIT_HEADS + head);
            if constexpr (!DKV) {                           // the lane is the query; registers 4 g .. 4 g + 3 are four consecutive keys: one Philox call
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint32_t mw[4];
                    drop_words(drop, (uint32_t)((row0 + 8 * g + 4 * h) >> 2), (uint32_t)old, bh, mw);
#pragma unroll
                    for (int e = 0; e < 4; ++e) keep[4 * g + e] = drop_keep(drop, mw[e]);
                }
            } else {                                        // the lane is the key; every register is another query: a call each
#pragma unroll
                for (int e = 0; e < 16; ++e) keep[e] = drop_keep_attn(drop, bh, (uint32_t)(row0 + crow(e, h)), (uint32_t)old);
            }
#endif
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int wr = sub * 32 + crow(e, h);
                const float lv = DKV ? Ls[wr] : lse_own, dv = DKV ? Ds[wr] : delta_own;
                p[e] = (wt0 + wr < a.n_walk) ? exp2f(sc[e] * a.scale_log2e - lv) : 0.f;
#if VIT_ATT_BWD_DROP
                dp[e] = keep[e] ? dp[e] * drop.scale : 0.f;
#endif
                ds[e] = p[e] * (dp[e] - dv) * a.scale;
#if VIT_ATT_BWD_DROP
                if (DKV) p[e] = keep[e] ? p[e] * drop.scale : 0.f;     // dV takes the dropped probabilities
#endif
            }
            if constexpr (BF) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint4 dk = make_uint4(pack2_bf16(ds[8 * s], ds[8 * s + 1]), pack2_bf16(ds[8 * s + 2], ds[8 * s + 3]),
                                                pack2_bf16(ds[8 * s + 4], ds[8 * s + 5]), pack2_bf16(ds[8 * s + 6], ds[8 * s + 7]));
                    const uint2 u0 = *(const uint2*)(W1t + r * G::TP + sub * 32 + 16 * s + 4 * h);
                    const uint2 u1 = *(const uint2*)(W1t + r * G::TP + sub * 32 + 16 * s + 8 + 4 * h);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, make_uint4(u0.x, u0.y, u1.x, u1.y)), __builtin_bit_cast(bf16x8, dk),
                                                                   acc1, 0, 0, 0);
                    if constexpr (DKV) {
                        const uint4 pk = make_uint4(pack2_bf16(p[8 * s], p[8 * s + 1]), pack2_bf16(p[8 * s + 2], p[8 * s + 3]),
                                                    pack2_bf16(p[8 * s + 4], p[8 * s + 5]), pack2_bf16(p[8 * s + 6], p[8 * s + 7]));
                        const uint2 v0 = *(const uint2*)(W2t + r * G::TP + sub * 32 + 16 * s + 4 * h);
                        const uint2 v1 = *(const uint2*)(W2t + r * G::TP + sub * 32 + 16 * s + 8 + 4 * h);
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, make_uint4(v0.x, v0.y, v1.x, v1.y)),
                                                                       __builtin_bit_cast(bf16x8, pk), acc2, 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float x1 = ((const float*)W1n)[(sub * 32 + crow(e, h)) * G::NP + r];
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, ds[e], acc1, 0, 0, 0);
                    if constexpr (DKV) {
                        const float x2 = ((const float*)W2n)[(sub * 32 + crow(e, h)) * G::NP + r];
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x2, p[e], acc2, 0, 0, 0);
                    }
                }
            }
        }
    }
    if (orow >= a.n_own) return;
    T* o1 = (T*)a.g1 + b * a.bs_g1 + (int64_t)orow * a.ld_g1 + head * VIT_HD;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = acc1[4 * q + e];
        store_from_f32(o1 + 8 * q + 4 * h, w);
    }
    if constexpr (DKV) {
        T* o2 = (T*)a.g2 + b * a.bs_g2 + (int64_t)orow * a.ld_g2 + head * VIT_HD;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = acc2[4 * q + e];
            store_from_f32(o2 + 8 * q + 4 * h, w);
        }
    }
}
