// conv_splitk_finish_kernel.inc — the text of the split-K finish kernel, included twice by conv_mfma.hip: with CONV_GATED 0 as conv_splitk_finish_kernel (the kernel every existing launch
// runs: its signature and machine code are what they were when the text stood in conv_mfma.hip) and with CONV_GATED 1 as conv_splitk_finish_gated_kernel, which takes one more
// argument, gate_slope, and MULTIPLIES the fp32 value by it where the mask is not positive instead of zeroing it: the LeakyReLU derivative of the producing
// activation, read off its output (cvae_conv_down_bwd_data).  CONV_GATE_PARAM / CONV_GATE_OFF come from conv_mfma.hip.
#if CONV_GATED
#define CONV_SPLITK_FINISH_KERNEL conv_splitk_finish_gated_kernel
#else
#define CONV_SPLITK_FINISH_KERNEL conv_splitk_finish_kernel
#endif
template <typename T, int EPI>
__global__ __launch_bounds__(256) void CONV_SPLITK_FINISH_KERNEL(const float* __restrict__ ws, const float* __restrict__ bias, const T* __restrict__ mask,
                                                                  T* __restrict__ out, int64_t total, int Cout, int ksplit, int act, float acc_scale, float out_scale, F8Side f8 CONV_GATE_PARAM) {
    const int64_t i8 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    float amx = 0.f;
    if (i8 < total) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0.f;
        constexpr int U = 8;                                 // slab loads in flight (clamped index, predicated add: same order of the sum)
        for (int k0 = 0; k0 < ksplit; k0 += U) {
            float4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float* p = ws + (size_t)min(k0 + u, ksplit - 1) * total + i8;
                a[u] = *(const float4*)p; b[u] = *(const float4*)(p + 4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + u < ksplit) { v[0] += a[u].x; v[1] += a[u].y; v[2] += a[u].z; v[3] += a[u].w; v[4] += b[u].x; v[5] += b[u].y; v[6] += b[u].z; v[7] += b[u].w; }
        }
        const float accs = f8.dscale ? f8.dscale[0] : acc_scale;
        const int c = (int)(i8 % Cout);
        Piece<T> mp, op;
        unsigned mb = 0xffu;
        if (f8.mask_bits) mb = ((const unsigned char*)f8.mask_bits)[i8 >> 3];
        else if (mask) {
            piece_load_raw<T>(mp, mask + i8);
            const T* mv = (const T*)&mp;
            mb = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) mb |= (to_f32(mv[q]) > 0.f ? 1u : 0u) << q;
        }
        T* ov = (T*)&op;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float x = v[q] * accs + (bias ? bias[c + q] : 0.f);
            x = apply_act_t<EPI>(x, act);
            if (!((mb >> q) & 1u)) x = CONV_GATE_OFF(x);
            v[q] = x;
            ov[q] = from_f32<T>(x);
            amx = fmaxf(amx, fabsf(x));
        }
        piece_store<T>(op, (char*)(out + i8));
        if (f8.bits_out) ((unsigned char*)f8.bits_out)[i8 >> 3] = (unsigned char)mask_byte_of(v);
        if (f8.out8) *(uint2*)(f8.out8 + i8) = pack8_fp8(v, f8.dscale ? f8.dscale[1] : out_scale);     // by value when the caller keeps no device scales
    }
    __shared__ float red[4];
    if (f8.amax) amax_publish_wg(f8.amax, amx, blockIdx.x, red);
}
#undef CONV_SPLITK_FINISH_KERNEL
