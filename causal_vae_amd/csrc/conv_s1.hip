// conv_s1.hip — the stride-1 window convolutions and the latent-to-grid GEMM of the ViT-VAE decoder in eval mode
// (vessel_analysis/00_core/vit_backbone.py:7-19, 115-156, 186-193 of the reference):
//   * cvae_conv_s1: halo-tiled implicit GEMM on the MFMA over channels-last [B][H][W][C] tensors, two window forms from one template:
//       K3        Conv2d(k3, s1, p1), Cin = Cout in {32, 64, 128} (the ResBlock convs): 3 x 3 centred window, zero padding of one;
//       SUBPIXEL  ConvTranspose2d(k3, s2, p1, output_padding 1) with Cout = 16, Cin in {32, 16}, as a stride-1 conv with a 2 x 2 FORWARD window (input
//                 padded by one at the right and bottom) to N = 4 Cout channels (py, px, co) and a pixel-shuffle store: out[2y + py][2x + px][co].
//                 o = 2i - 1 + k gives, per direction: parity 0 reads in[y] with k = 1; parity 1 reads in[y] with k = 2 and in[y + 1] with k = 0.
//     The weight is the GEMM matrix [N][KT] in the compute dtype, k = tap * Cin + ci, KT = K rounded up to 64 with zero columns (what cvae_fold_bn_conv's
//     kinds CVAE_FOLD_CONV_K3S1 / CVAE_FOLD_CONVT_K3S2_SUBPIXEL write in fp32; cvae_conv_s1_pack_weights casts a list of them to bf16 in one launch).
//     Workgroup = 4 waves = 8 x 16 output positions (a wave owns two rows of 16); the tile plus its halo is staged in LDS ONCE at full channel depth, then
//     K is walked in 128-byte chunks of the weight rows (64 bf16 / 32 fp32) through LDS, the next chunk's global loads in flight while the MFMAs of the
//     current one run.  D = W x^T as in csrc/vit.hip: A = weight rows (output channels), B = positions, so a lane owns ONE position and four consecutive
//     channels per register group.  bf16 operands on v_mfma_f32_32x32x16_bf16, exact fp32 on v_mfma_f32_32x32x2_f32; accumulation fp32 in a fixed order
//     (no atomics, no split-K; the tile geometry does not depend on B, so a sample's bits do not depend on the batch it travels in).
//     Epilogue in fp32 before the one rounding: + bias, + residual (optional, the output's shape and dtype), activation.  Stores are 16 bytes: fp32 as
//     they are; bf16 after one v_permlane32_swap per dword that hands lane half 0 channels 0-7 and lane half 1 channels 8-15 of a 16-channel block.
//   * cvae_conv_s1_c1: Conv2d(16 -> 1, k3, s1, p1) to an fp32 [B][1][H][W] image: bandwidth-bound, one thread per four output pixels of a row, 16-byte loads.
//   * cvae_latent_to_grid: out[b][p][c] = sum_k W[c P + p][k] z[b][k] + bias[c P + p]: nn.Linear(latent, C P) + view(B, C, gh, gw) written channels-last
//     in the compute dtype.  W is the fp32 nn.Linear tensor, read ONCE per launch with 16-byte loads for up to 16 batch rows (z sits in LDS).
// The input-gradient path of the same (frozen, eval-mode) decoder:
//   * cvae_conv_s1_bwd_data: dx = (conv(g, w^T) + resid) * act'(gate) from the SAME kernel template (BWD = true: no bias, the gate in the epilogue):
//       K3          the input gradient of Conv2d(C, C, 3, 1, 1) is a K3 conv with the taps flipped and the channels transposed: only the matrix differs;
//       SUBPIXEL_T  the input gradient of ConvTranspose2d(Cin, 16, 3, 2, 1, output_padding 1), dx[y][x] = sum_k g[2y - 1 + ky][2x - 1 + kx] w[..][ky][kx]:
//                   g [B][2H][2W][16] read space-to-depth as [B][H][W][64 = (py, px, co)] with a 2 x 2 BACKWARD window (positions y - 1, y: the zero row
//                   and column sit at the top and left), K = 256 of which 9/16 are taps, N = 32 rows (Cin = 16: the upper 16 rows are zeros, not stored).
//   * cvae_conv_s1_c1_bwd_data: the 1 -> 16 gradient of the output conv, one thread per pixel, gated by the conv's input, 16-byte stores.
//   * cvae_latent_to_grid_bwd: dz[b][k] = sum_{p, c} g[b][p][c] W[c P + p][k]: W streamed once in slabs of 32 channels x 8 positions, per-slab partial
//     sums in the caller's workspace, added in slab order by a second launch (no float atomics).
#include "common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));          // a 16-byte piece that stays in registers when held in an array

// f(Int<0>{}) .. f(Int<N - 1>{}): a loop whose index is a compile-time constant in every iteration (register arrays stay in registers)
template <int N, typename Fn> __device__ __forceinline__ void static_for(Fn&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(Int<N - 1>{});
    }
}

// ------------------------------------------------------------------------------------------------ stride-1 window conv on the MFMA
// the factor a backward epilogue applies where the gate (the activation's output) is not positive: torch's rule x > 0 ? 1 : slope, once per launch
__device__ __forceinline__ float gate_slope(int act) { return act == CVAE_ACT_LEAKY02 ? 0.2f : (act == CVAE_ACT_LEAKY001 ? 0.01f : (act == CVAE_ACT_RELU ? 0.f : 1.f)); }
#define S1_TH 8
#define S1_TW 16
#define S1_KPAD 64                 // K is padded to a multiple of this many elements in the packed weight (both dtypes)

template <typename T, int CIN, int FORM> struct S1Geom {
    static constexpr int WIN = FORM == CVAE_CONV_S1_K3 ? 3 : 2;
    static constexpr int PADL = FORM == CVAE_CONV_S1_SUBPIXEL ? 0 : 1; // the window starts at output position - PADL
    static constexpr int TAPS = WIN * WIN;
    static constexpr int K = TAPS * CIN;
    static constexpr int KT = (K + S1_KPAD - 1) / S1_KPAD * S1_KPAD;
    static constexpr int HR = S1_TH + WIN - 1, HC = S1_TW + WIN - 1;
    static constexpr int E16 = 16 / sizeof(T);
    static constexpr int PITCH = CIN + E16;                            // halo position pitch in elements: + 16 bytes (rows fall 4 banks apart mod 32)
    static constexpr int KC = 128 / sizeof(T);                         // k elements per weight chunk
    static constexpr int WPITCH = KC + E16;                            // 144 bytes
    static constexpr int PPP = CIN / E16;                              // 16-byte pieces per position
};

// BWD (cvae_conv_s1_bwd_data): x is the incoming gradient, no bias, y = (acc + resid) * act'(gate); COUT_T = the channels stored in form SUBPIXEL_T
template <typename T, int CIN, int NT, int FORM, bool BWD = false, int COUT_T = 0>
__global__ __launch_bounds__(256) void conv_s1_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, const T* resid, T* y,
                                                      int H, int W, int act, const T* gate) {
    using G = S1Geom<T, CIN, FORM>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    constexpr int N = 32 * NT;
    constexpr int COUT = FORM == CVAE_CONV_S1_K3 ? N : (FORM == CVAE_CONV_S1_SUBPIXEL ? N / 4 : COUT_T);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* hs = (T*)smem;                                                   // [HR * HC + 1][PITCH]: the last row is zeros, read for the zero-padded k >= K
    T* ws = hs + (G::HR * G::HC + 1) * G::PITCH;                        // [N][WPITCH]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int x0 = blockIdx.x * S1_TW, y0 = blockIdx.y * S1_TH;
    const int64_t b = blockIdx.z;
    const T* xb = x + b * (int64_t)H * W * CIN;

    u32x4 rw[NT];
    const T* wt = w + (int64_t)(t >> 3) * G::KT + (t & 7) * G::E16;      // this thread's piece of weight rows (t >> 3) + 32 i
    static_for<NT>([&](auto iv) { constexpr int i = decltype(iv)::value; rw[i] = *(const u32x4*)(wt + (int64_t)32 * i * G::KT); });
    // the tile and its halo, once, at full channel depth; positions outside the image are zeros (the conv's padding)
    for (int i = t; i < (G::HR * G::HC + 1) * G::PPP; i += 256) {
        const int pos = i / G::PPP, piece = i - pos * G::PPP;
        const int hy = pos / G::HC, hx = pos - hy * G::HC;
        const int gy = y0 - G::PADL + hy, gx = x0 - G::PADL + hx;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pos < G::HR * G::HC && gy >= 0 && gy < H && gx >= 0 && gx < W) {
            if constexpr (FORM == CVAE_CONV_S1_SUBPIXEL_T) {            // channel (py, px, co) of position (gy, gx) is g[2 gy + py][2 gx + px][co]
                const int e = piece * G::E16, q = e >> 4;
                v = *(const uint4*)(xb + (((int64_t)(2 * gy + (q >> 1)) * (2 * W)) + 2 * gx + (q & 1)) * 16 + (e & 15));
            } else {
                v = *(const uint4*)(xb + ((int64_t)gy * W + gx) * CIN + piece * G::E16);
            }
        }
        *(uint4*)(hs + pos * G::PITCH + piece * G::E16) = v;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const int ly = wave * 2 + (r >> 4), lx = r & 15;                    // this lane's output position in the tile
    for (int k0 = 0; k0 < G::KT; k0 += G::KC) {
        __syncthreads();                                                // the previous chunk's fragment reads are done (first pass: nothing pending)
        static_for<NT>([&](auto iv) {
            constexpr int i = decltype(iv)::value;
            *(u32x4*)(ws + ((t >> 3) + 32 * i) * G::WPITCH + (t & 7) * G::E16) = rw[i];
        });
        __syncthreads();                                                // weights of this chunk (and, on the first pass, the halo) are visible
        if (k0 + G::KC < G::KT)
            static_for<NT>([&](auto iv) { constexpr int i = decltype(iv)::value; rw[i] = *(const u32x4*)(wt + (int64_t)32 * i * G::KT + k0 + G::KC); });
        if constexpr (BF) {
#pragma unroll
            for (int s = 0; s < G::KC / 16; ++s) {
                const int kk = k0 + 16 * s + 8 * h;
                const int tap = kk / CIN, ci = kk - tap * CIN;
                const int dy = tap / G::WIN, dx = tap - dy * G::WIN;
                const int pos = tap < G::TAPS ? (ly + dy) * G::HC + lx + dx : G::HR * G::HC;      // zero-padded weight columns meet the zero row: exact zeros
                const bf16x8 bv = *(const bf16x8*)(hs + pos * G::PITCH + ci);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const bf16x8 av = *(const bf16x8*)(ws + (j * 32 + r) * G::WPITCH + 16 * s + 8 * h);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[j], 0, 0, 0);
                }
            }
        } else {
            // 32x32x2: the instruction's k index is the lane half; step (c, u) multiplies k = 16 h + 4 c + u of the chunk
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int kk = k0 + 16 * h + 4 * c;
                const int tap = kk / CIN, ci = kk - tap * CIN;
                const int dy = tap / G::WIN, dx = tap - dy * G::WIN;
                const int pos = tap < G::TAPS ? (ly + dy) * G::HC + lx + dx : G::HR * G::HC;
                float bv[4], av[NT][4];
                load_f32(hs + pos * G::PITCH + ci, bv);
#pragma unroll
                for (int j = 0; j < NT; ++j) load_f32(ws + (j * 32 + r) * G::WPITCH + 16 * h + 4 * c, av[j]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][u], bv[u], acc[j], 0, 0, 0);
            }
        }
    }
    // epilogue: lane (r, h) holds, for its position, channels j 32 + 8 g + 4 h + e in register 4 g + e of acc[j]
    const int gy = y0 + ly, gx = x0 + lx;
    [[maybe_unused]] const float slope = BWD ? gate_slope(act) : 0.f;
    const bool live = gy < H && gx < W;                                 // lanes r and r + 32 share a position: the swap below pairs equals
    auto out_index = [&](int n) -> int64_t {                            // element index of channel n of this position in y (and resid)
        if (FORM != CVAE_CONV_S1_SUBPIXEL) return ((b * H + gy) * (int64_t)W + gx) * COUT + n;
        const int q = n / COUT, co = n - q * COUT;
        return ((b * 2 * H + 2 * gy + (q >> 1)) * (int64_t)(2 * W) + 2 * gx + (q & 1)) * COUT + co;
    };
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            if (FORM == CVAE_CONV_S1_SUBPIXEL_T && j * 32 + 16 * gp >= COUT) continue;      // zero rows of the matrix: nothing to store (uniform: no lane skips the swap alone)
            float v[2][4];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int g = 2 * gp + q, n = j * 32 + 8 * g + 4 * h;
                if constexpr (BWD) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q][e] = acc[j][4 * g + e];
                } else {
                    float bv[4];
                    load_f32(bias + (n % COUT), bv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q][e] = acc[j][4 * g + e] + bv[e];
                }
                if (resid && live) {
                    float rv[4];
                    load_f32(resid + out_index(n), rv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q][e] += rv[e];
                }
                if constexpr (BWD) {
                    if (gate && live) {                                 // torch's rule: x > 0 ? 1 : slope, read off the activation's OUTPUT (LeakyReLU keeps the sign)
                        float gv[4];
                        load_f32(gate + out_index(n), gv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[q][e] *= gv[e] > 0.f ? 1.f : slope;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q][e] = apply_act(v[q][e], act);
                }
            }
            if constexpr (BF) {
                const uint2 a = make_uint2(pack2_bf16(v[0][0], v[0][1]), pack2_bf16(v[0][2], v[0][3]));
                const uint2 c = make_uint2(pack2_bf16(v[1][0], v[1][1]), pack2_bf16(v[1][2], v[1][3]));
                const auto sx = __builtin_amdgcn_permlane32_swap(a.x, c.x, false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(a.y, c.y, false, false);
                if (live) *(uint4*)(y + out_index(j * 32 + 16 * gp + 8 * h)) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
            } else if (live) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    *(float4*)(y + out_index(j * 32 + 8 * (2 * gp + q) + 4 * h)) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
            }
        }
}

// one launch of the template: the forward passes gate = nullptr, the backward (BWD) bias = nullptr; `act` is the backward's gate activation
struct S1Args { const void *x, *w; const float* bias; const void *resid, *gate; void* y; int64_t B, H, W; int act; hipStream_t st; };
template <typename T, int CIN, int NT, int FORM, bool BWD = false, int COUT_T = 0> int conv_s1_launch(const S1Args& a) {
    using G = S1Geom<T, CIN, FORM>;
    constexpr auto kern = conv_s1_kernel<T, CIN, NT, FORM, BWD, COUT_T>;
    constexpr size_t LDS = ((size_t)(G::HR * G::HC + 1) * G::PITCH + (size_t)32 * NT * G::WPITCH) * sizeof(T);
    static_assert(LDS <= CVAE_LDS_MAX, "tile does not fit a workgroup's LDS");
    if (cvae_allow_lds<kern>(LDS) != CVAE_OK) return CVAE_E_LAUNCH;
    const dim3 grid((unsigned)((a.W + S1_TW - 1) / S1_TW), (unsigned)((a.H + S1_TH - 1) / S1_TH), (unsigned)a.B);
    hipLaunchKernelGGL(kern, grid, dim3(256), LDS, a.st, (const T*)a.x, (const T*)a.w, a.bias, (const T*)a.resid, (T*)a.y, (int)a.H, (int)a.W, a.act, (const T*)a.gate);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
// the K3 ladder: C = Cin = Cout in {32, 64, 128} (checked by the caller through cvae_conv_s1_weight_elems), one 32-row block of the matrix per 32 channels
template <typename T, bool BWD> int conv_s1_k3(int64_t C, const S1Args& a) {
    if (C == 32) return conv_s1_launch<T, 32, 1, CVAE_CONV_S1_K3, BWD>(a);
    if (C == 64) return conv_s1_launch<T, 64, 2, CVAE_CONV_S1_K3, BWD>(a);
    return conv_s1_launch<T, 128, 4, CVAE_CONV_S1_K3, BWD>(a);
}
// argument checks the entries share
bool s1_dims_ok(int64_t B, int64_t H, int64_t W) { return B >= 0 && H > 0 && W > 0 && H <= 65535 * S1_TH && B <= 65535 && W <= ((int64_t)1 << 24); }
bool c1_dims_ok(int64_t B, int64_t H, int64_t W) { return B >= 0 && H > 0 && W > 0 && H <= ((int64_t)1 << 24) && W <= ((int64_t)1 << 24); }
bool s1_act_ok(int act) { return act == CVAE_ACT_NONE || act == CVAE_ACT_LEAKY02 || act == CVAE_ACT_LEAKY001 || act == CVAE_ACT_RELU; }

// fp32 -> bf16 for a list of tensors in one launch (the packed weights of the bf16 decoder)
#define S1_PACK_MAX 16
struct PackTable {
    const float* src[S1_PACK_MAX];
    bf16* dst[S1_PACK_MAX];
    int end[S1_PACK_MAX];             // exclusive prefix sums of blocks
    int64_t n4[S1_PACK_MAX];          // float4 groups
    int count;
};
__global__ __launch_bounds__(256) void conv_s1_pack_kernel(const PackTable T) {
    int k = 0;
    while (k < T.count - 1 && (int)blockIdx.x >= T.end[k]) ++k;
    const int64_t g = ((int64_t)blockIdx.x - (k ? T.end[k - 1] : 0)) * 256 + threadIdx.x;
    if (g >= T.n4[k]) return;
    const float4 v = ((const float4*)T.src[k])[g];
    ((uint2*)T.dst[k])[g] = make_uint2(pack2_bf16(v.x, v.y), pack2_bf16(v.z, v.w));
}

// ------------------------------------------------------------------------------------------------ Conv2d(16 -> 1, k3, s1, p1) -> fp32 image
// One thread per four consecutive output pixels of a row: 3 rows x 6 columns of 16 channels, each read with 16-byte loads; every output pixel adds
// its 144 products in (ky, kx, ci) order.  Weights sit in LDS as [tap][ci] fp32 (rounded to bf16 first in bf16 mode).
#define C1_CIN 16
template <typename T>
__global__ __launch_bounds__(256) void conv_s1_c1_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
                                                         int64_t B, int H, int W, int act) {
    __shared__ float wsm[9][C1_CIN];
    if (threadIdx.x < 9 * C1_CIN) {
        const int tap = threadIdx.x / C1_CIN, ci = threadIdx.x % C1_CIN;
        const float v = w[ci * 9 + tap];
        wsm[tap][ci] = std::is_same<T, bf16>::value ? (float)(bf16)v : v;
    }
    __syncthreads();
    const int W4 = (W + 3) >> 2;
    const int64_t total = B * H * W4, g = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (g >= total) return;
    const int xq = (int)(g % W4), yy = (int)((g / W4) % H);
    const int64_t b = g / ((int64_t)W4 * H);
    const int xs = xq * 4;
    const float b0 = bias ? bias[0] : 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int gy = yy - 1 + dy;
        if (gy < 0 || gy >= H) continue;
        const T* row = x + (b * H + gy) * (int64_t)W * C1_CIN;
#pragma unroll
        for (int cx = 0; cx < 6; ++cx) {
            const int gx = xs - 1 + cx;
            if (gx < 0 || gx >= W) continue;
            float v[C1_CIN];
            load_f32(row + (int64_t)gx * C1_CIN, v);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int dx = cx - o;
                if (dx < 0 || dx > 2) continue;
#pragma unroll
                for (int ci = 0; ci < C1_CIN; ++ci) acc[o] = fmaf(v[ci], wsm[dy * 3 + dx][ci], acc[o]);
            }
        }
    }
    float* out = y + (b * H + yy) * (int64_t)W + xs;
    if ((W & 3) == 0) {
        *(float4*)out = make_float4(apply_act(acc[0] + b0, act), apply_act(acc[1] + b0, act), apply_act(acc[2] + b0, act), apply_act(acc[3] + b0, act));
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (xs + o < W) out[o] = apply_act(acc[o] + b0, act);
    }
}

// ------------------------------------------------------------------------------------------------ latent -> channels-last grid
// One wave per (grid position p, block of 32 channels): four steps of 8 channels, 8 lanes per weight row W[c P + p][0 .. K) (16-byte loads, k = 4 l + 32 i
// per lane), each batch row's dot product summed per lane in k order and then over the 8 lanes by xor shuffles (a fixed tree: a row's bits do not
// depend on the other rows of the launch).  z [nb <= 16][K] sits in LDS.
#define L2G_BT 16
#define L2G_KMAX 512
template <typename T>
__global__ __launch_bounds__(256) void latent_to_grid_kernel(const float* __restrict__ z, const float* __restrict__ Wt, const float* __restrict__ bias, T* __restrict__ out,
                                                             int nb, int K, int64_t P, int C) {
    __shared__ __attribute__((aligned(16))) float zs[L2G_BT * L2G_KMAX];
    for (int i = threadIdx.x; i < nb * (K >> 2); i += 256) ((float4*)zs)[i] = ((const float4*)z)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, l8 = lane & 7, grp = lane >> 3;
    const int cblocks = C >> 5;
    const int64_t task = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
    if (task >= P * cblocks) return;
    const int64_t p = task / cblocks;
    const int cb = (int)(task - p * cblocks);
    const int steps = (K + 31) >> 5;
    for (int s = 0; s < 4; ++s) {
        const int c = cb * 32 + s * 8 + grp;
        const int64_t n = (int64_t)c * P + p;
        const float* wr = Wt + n * K;
        float4 wv[L2G_KMAX / 32];
#pragma unroll
        for (int i = 0; i < L2G_KMAX / 32; ++i) {
            const int k = 4 * l8 + 32 * i;
            wv[i] = (i < steps && k < K) ? *(const float4*)(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float bn = bias ? bias[n] : 0.f;
        float keep[2] = {0.f, 0.f};
        for (int bb = 0; bb < nb; ++bb) {
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < L2G_KMAX / 32; ++i) {
                const int k = 4 * l8 + 32 * i;
                if (i < steps && k < K) {
                    const float4 zv = *(const float4*)(zs + bb * K + k);
                    a = fmaf(wv[i].x, zv.x, a); a = fmaf(wv[i].y, zv.y, a); a = fmaf(wv[i].z, zv.z, a); a = fmaf(wv[i].w, zv.w, a);
                }
            }
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            a += __shfl_xor(a, 4, 64);
            if ((bb & 7) == l8) keep[bb >> 3] = a + bn;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int bb = l8 + 8 * q;
            if (bb < nb) out[((int64_t)bb * P + p) * C + c] = from_f32<T>(keep[q]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ input gradient of Conv2d(16 -> 1, k3, s1, p1)
// One thread per pixel: dx[y][x][ci] = (sum_{ky, kx} g[y + 1 - ky][x + 1 - kx] w[ci][ky][kx]) * act'(gate[y][x][ci]), the 9 products of a channel added
// in (ky, kx) order; 16 channels leave as 16-byte stores (four fp32 / two bf16 pieces per thread, consecutive threads consecutive pixels).  g is the fp32
// image cotangent; the weights as the forward reads them (rounded to bf16 first in bf16 mode).
template <typename T>
__global__ __launch_bounds__(256) void conv_s1_c1_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w, const T* __restrict__ gate, T* __restrict__ dx,
                                                             int64_t B, int H, int W, int act) {
    __shared__ float wsm[9][C1_CIN];
    if (threadIdx.x < 9 * C1_CIN) {
        const int tap = threadIdx.x / C1_CIN, ci = threadIdx.x % C1_CIN;
        const float v = w[ci * 9 + tap];
        wsm[tap][ci] = std::is_same<T, bf16>::value ? (float)(bf16)v : v;
    }
    __syncthreads();
    const int64_t total = B * H * W, i = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (i >= total) return;
    const int xx = (int)(i % W), yy = (int)((i / W) % H);
    const float* gb = g + (i / ((int64_t)W * H)) * (int64_t)H * W;
    float gv[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int sy = yy + 1 - ky, sx = xx + 1 - kx;
            gv[ky * 3 + kx] = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? gb[(int64_t)sy * W + sx] : 0.f;
        }
    float acc[C1_CIN], gt[C1_CIN];
#pragma unroll
    for (int ci = 0; ci < C1_CIN; ++ci) acc[ci] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ci = 0; ci < C1_CIN; ++ci) acc[ci] = fmaf(gv[tap], wsm[tap][ci], acc[ci]);
    if (gate) {
        const float slope = gate_slope(act);
        load_f32(gate + i * C1_CIN, gt);
#pragma unroll
        for (int ci = 0; ci < C1_CIN; ++ci) acc[ci] *= gt[ci] > 0.f ? 1.f : slope;
    }
    store_from_f32(dx + i * C1_CIN, acc);
}

// ------------------------------------------------------------------------------------------------ channels-last grid gradient -> latent gradient
// dz[b][k] = sum_n G[b][n] W[n][k], n = c P + p, G[b][c P + p] = g[b][p][c].  A slab = 32 channels x 8 positions = 256 rows of W (per channel 8 consecutive
// rows: 8 K floats contiguous); the slab list depends on C and P only.  One workgroup per slab: its g values (all rows of the launch) go to LDS with
// coalesced reads of 32 consecutive channels and are transposed there to [b][cl][pl]; thread (kq, rp) owns columns 4 kq .. 4 kq + 3 and walks the
// 4-row groups rp, rp + RP, .. of the slab, two groups (eight 16-byte loads of W) issued before the first is used, every batch row's 4 sums in
// registers, added in row order.  The RP phases are then added in phase order through LDS -> part[slab][b][K]; l2g_bwd_finish adds the slabs in slab order.
#define L2GB_CB 32
#define L2GB_PB 8
#define L2GB_ROWS (L2GB_CB * L2GB_PB)
template <typename T>
__global__ __launch_bounds__(256) void l2g_bwd_kernel(const T* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ part, int nb, int K, int64_t P, int C,
                                                      int kq_pad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* gs = (float*)smem;                                           // [nb][256]: row cl * 8 + pl
    float* red = gs + nb * L2GB_ROWS;                                   // [RP][nb][K]
    const int t = threadIdx.x;
    const int pblocks = (int)((P + L2GB_PB - 1) / L2GB_PB);
    const int cb = blockIdx.x / pblocks, pb = blockIdx.x - cb * pblocks;
    const int64_t p0 = (int64_t)pb * L2GB_PB;
    for (int i = t; i < nb * L2GB_ROWS; i += 256) {                     // i = (b, pl, cl): 32 consecutive channels per read
        const int b = i / L2GB_ROWS, r = i - b * L2GB_ROWS, pl = r / L2GB_CB, cl = r - pl * L2GB_CB;
        const int64_t p = p0 + pl;
        gs[b * L2GB_ROWS + cl * L2GB_PB + pl] = p < P ? to_f32(g[((int64_t)b * P + p) * C + cb * L2GB_CB + cl]) : 0.f;
    }
    __syncthreads();
    const int kq = t % kq_pad, rp = t / kq_pad, RP = 256 / kq_pad;
    const bool col = 4 * kq < K;
    float acc[L2G_BT][4];
#pragma unroll
    for (int b = 0; b < L2G_BT; ++b) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0.f;
    if (col) {
        for (int rg = rp; rg < L2GB_ROWS / 4; rg += 2 * RP) {           // 64 row groups; RP divides 32
            float4 wv[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int lr = (rg + u * RP) * 4, cl = lr / L2GB_PB, pl = lr - cl * L2GB_PB;
                const float* wr = Wt + ((int64_t)(cb * L2GB_CB + cl) * P + p0 + pl) * K + 4 * kq;
#pragma unroll
                for (int e = 0; e < 4; ++e) wv[u][e] = p0 + pl + e < P ? *(const float4*)(wr + (int64_t)e * K) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int lr = (rg + u * RP) * 4;
#pragma unroll
                for (int b = 0; b < L2G_BT; ++b)
                    if (b < nb) {
                        const float4 gv = *(const float4*)(gs + b * L2GB_ROWS + lr);
                        const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc[b][0] = fmaf(ge[e], wv[u][e].x, acc[b][0]); acc[b][1] = fmaf(ge[e], wv[u][e].y, acc[b][1]);
                            acc[b][2] = fmaf(ge[e], wv[u][e].z, acc[b][2]); acc[b][3] = fmaf(ge[e], wv[u][e].w, acc[b][3]);
                        }
                    }
            }
        }
#pragma unroll
        for (int b = 0; b < L2G_BT; ++b)
            if (b < nb) *(float4*)(red + ((int64_t)rp * nb + b) * K + 4 * kq) = make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
    }
    __syncthreads();
    float* out = part + (int64_t)blockIdx.x * nb * K;
    for (int i = t; i < nb * K; i += 256) {
        float s = red[i];
        for (int q = 1; q < RP; ++q) s += red[q * nb * K + i];
        out[i] = s;
    }
}

__global__ __launch_bounds__(256) void l2g_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ dz, int n, int slabs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int q = 0; q < slabs; ++q) s += part[(int64_t)q * n + i];
    dz[i] = s;
}

int l2g_bwd_kq_pad(int64_t K) {                                         // threads across a row of W: the power of two at or above K / 4, 8 .. 128
    int v = 8;
    while (4 * v < K) v <<= 1;
    return v;
}
int64_t l2g_bwd_slabs(int64_t P, int64_t C) { return (C / L2GB_CB) * ((P + L2GB_PB - 1) / L2GB_PB); }

// ------------------------------------------------------------------------------------------------ weight gradient of the stride-1 window convs
// dWmat[n][tap][ci] = sum over pixels of g[pixel][n] x[pixel + tap][ci]: a GEMM whose K runs over the B H W pixels.  The matrix is cut into 32 x 32 blocks
// (n block nb, ci block cb: a "pair") times the taps; channel counts below 32 are padded with zero channels in LDS.  A workgroup stages the family's 8 x 16
// tile of x with its halo and the tile of g (zeros outside the image) channels-last, as the forward does; a wave owns one pair and every TS-th tap and keeps
// those blocks in registers while the workgroup walks tiles blockIdx.x, + slabs, ..: the pixel index is the MFMA's k, A = g (rows n), B = x (columns ci).
//   C = 128: 16 pairs, 4 per workgroup (one n block, the four ci blocks), grid.y = 4: the split over (tap, co) that keeps a slab's owner count low
//   C = 64:  4 pairs, one workgroup        C = 32, 16: one pair, the 9 taps dealt over the 4 waves        SUBPIXEL: 2 pairs (py), 2 waves each over the 4 taps
// The blocks leave as part[slab][pair][tap][32][32] (only rows and columns that exist are written); s1w_finish adds the slabs in slab order and writes the torch
// layout; the bias gradient rides along: thread t < GN adds channel t of the staged g tile, pixel by pixel, as a compensated (Kahan) fp32 sum — a plain chain
// over the 10^5 .. 10^7 pixels of a channel loses digits an eager sum keeps; sum and compensation both leave in the slab, and s1w_finish adds them the same way.
struct KahanSum {
    float s = 0.f, c = 0.f;                                             // the value is s - c
    __device__ __forceinline__ void add(float v) {
        const float y = v - c, t = s + y;
        c = (t - s) - y;
        s = t;
    }
};
template <typename T, int C, int FORM> struct S1WGeom {
    static constexpr bool SUB = FORM == CVAE_CONV_S1_SUBPIXEL;
    static constexpr int WIN = SUB ? 2 : 3, PADL = SUB ? 0 : 1, TAPS = WIN * WIN;
    static constexpr int N = SUB ? 64 : C;                              // rows of the matrix: (py, px, co) in the sub-pixel form
    static constexpr int COUT = SUB ? 16 : C;
    static constexpr int CP = C < 32 ? 32 : C, NP = N < 32 ? 32 : N;
    static constexpr int CB = CP / 32, NB = NP / 32, PAIRS = NB * CB;
    static constexpr int PW = PAIRS >= 4 ? 4 : PAIRS, TS = 4 / PW;       // pairs per workgroup, waves per pair
    static constexpr int NTW = (TAPS + TS - 1) / TS;                    // accumulator blocks per wave
    static constexpr int GROUPS = PAIRS / PW;                           // grid.y
    static constexpr int GN = GROUPS > 1 ? 32 : NP;                     // channels of g a workgroup stages
    static_assert(GROUPS == 1 || PW == CB, "a workgroup of a split layer owns one n block");
    static constexpr int HR = S1_TH + WIN - 1, HC = S1_TW + WIN - 1;
    static constexpr int E16 = 16 / sizeof(T);
    static constexpr int XPITCH = CP + E16, GPITCH = GN + E16;
    static constexpr int SLAB = PAIRS * TAPS * 1024;
    static constexpr size_t LDS = ((size_t)HR * HC * XPITCH + (size_t)S1_TH * S1_TW * GPITCH) * sizeof(T);
    static constexpr int MAX_SLABS = C >= 128 ? 64 : (C == 64 ? 256 : 512);
};

template <typename T, int C, int FORM>
__global__ __launch_bounds__(256) void conv_s1_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ g, float* __restrict__ part, float* __restrict__ pbias,
                                                            int H, int W, int tiles_x, int tiles_y, int tiles, int slabs) {
    using G = S1WGeom<T, C, FORM>;
    constexpr bool BF = std::is_same<T, bf16>::value;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* hs = (T*)smem;                                                   // [HR * HC][XPITCH]
    T* gs = hs + G::HR * G::HC * G::XPITCH;                             // [128][GPITCH]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int ts = wave % G::TS, pair = blockIdx.y * G::PW + wave / G::TS, nb = pair / G::CB, cb = pair % G::CB;
    const int goff = G::GROUPS > 1 ? blockIdx.y * 32 : 0;               // first channel of g this workgroup stages
    const int arow = nb * 32 - goff + r, bcol = cb * 32 + r;
    f32x16 acc[G::NTW];
#pragma unroll
    for (int i = 0; i < G::NTW; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    KahanSum bsum;
    for (int tile = blockIdx.x; tile < tiles; tile += slabs) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y;
        const int64_t b = tile / (tiles_x * tiles_y);
        const int x0 = tx * S1_TW, y0 = ty * S1_TH;
        const T* xb = x + b * (int64_t)H * W * C;
        __syncthreads();                                                // the previous tile's fragment reads are done
        constexpr int XPP = G::CP / G::E16, GPP = G::GN / G::E16;
        for (int i = t; i < G::HR * G::HC * XPP; i += 256) {
            const int pos = i / XPP, piece = i - pos * XPP;
            const int hy = pos / G::HC, hx = pos - hy * G::HC;
            const int gy = y0 - G::PADL + hy, gx = x0 - G::PADL + hx;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (piece * G::E16 < C && gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const uint4*)(xb + ((int64_t)gy * W + gx) * C + piece * G::E16);
            *(uint4*)(hs + pos * G::XPITCH + piece * G::E16) = v;
        }
        for (int i = t; i < S1_TH * S1_TW * GPP; i += 256) {
            const int p = i / GPP, piece = i - p * GPP;
            const int gy = y0 + (p >> 4), gx = x0 + (p & 15), ch = goff + piece * G::E16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ch < G::N && gy < H && gx < W) {
                if constexpr (G::SUB) {                                 // channel (py, px, co) of position (gy, gx) is g[2 gy + py][2 gx + px][co]
                    const int q = ch >> 4;
                    v = *(const uint4*)(g + (((b * 2 * H + 2 * gy + (q >> 1)) * (int64_t)(2 * W)) + 2 * gx + (q & 1)) * 16 + (ch & 15));
                } else {
                    v = *(const uint4*)(g + ((b * H + gy) * (int64_t)W + gx) * C + ch);
                }
            }
            *(uint4*)(gs + p * G::GPITCH + piece * G::E16) = v;
        }
        __syncthreads();
        if (t < G::GN)
            for (int p = 0; p < S1_TH * S1_TW; ++p) bsum.add(to_f32(gs[p * G::GPITCH + t]));
        if constexpr (BF) {
            // step s = tile row s: lane half h holds pixels (s, 8 h + j), j = 0 .. 7, in the instruction's k slots of both operands
#pragma unroll 1
            for (int s = 0; s < S1_TH; ++s) {
                bf16x8 av;
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = gs[(16 * s + 8 * h + j) * G::GPITCH + arow];
#pragma unroll
                for (int i = 0; i < G::NTW; ++i) {
                    const int tap = ts + i * G::TS;
                    if (tap < G::TAPS) {                                // the same for the whole wave
                        const int dy = tap / G::WIN, dx = tap - dy * G::WIN;
                        bf16x8 bv;
#pragma unroll
                        for (int j = 0; j < 8; ++j) bv[j] = hs[((s + dy) * G::HC + 8 * h + j + dx) * G::XPITCH + bcol];
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[i], 0, 0, 0);
                    }
                }
            }
        } else {
            // 32x32x2: the instruction's k index is the lane half: pixel 2 pp + h
#pragma unroll 2
            for (int pp = 0; pp < S1_TH * S1_TW / 2; ++pp) {
                const int p = 2 * pp + h, ly = p >> 4, lx = p & 15;
                const float av = gs[p * G::GPITCH + arow];
#pragma unroll
                for (int i = 0; i < G::NTW; ++i) {
                    const int tap = ts + i * G::TS;
                    if (tap < G::TAPS) {
                        const int dy = tap / G::WIN, dx = tap - dy * G::WIN;
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hs[((ly + dy) * G::HC + lx + dx) * G::XPITCH + bcol], acc[i], 0, 0, 0);
                    }
                }
            }
        }
    }
    // lane (r, h) holds rows 8 g + 4 h + e (n) of column r (ci) in register 4 g + e
    float* out = part + ((int64_t)blockIdx.x * G::PAIRS + pair) * G::TAPS * 1024;
#pragma unroll
    for (int i = 0; i < G::NTW; ++i) {
        const int tap = ts + i * G::TS;
        if (tap < G::TAPS && bcol < C) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = 8 * (e >> 2) + 4 * h + (e & 3);
                if (nb * 32 + row < G::N) out[(tap * 32 + row) * 32 + r] = acc[i][e];
            }
        }
    }
    if (t < G::GN && goff + t < G::N) {
        pbias[((int64_t)blockIdx.x * 2) * G::NP + goff + t] = bsum.s;
        pbias[((int64_t)blockIdx.x * 2 + 1) * G::NP + goff + t] = -bsum.c;
    }
}

// one thread per element of a slab: the slabs added in slab order, the sum written to the torch layout; the last block adds the bias partials
template <int C, int FORM>
__global__ __launch_bounds__(256) void s1w_finish_kernel(const float* __restrict__ part, const float* __restrict__ pbias, float* __restrict__ dW, float* __restrict__ db,
                                                         int slabs) {
    using G = S1WGeom<float, C, FORM>;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == G::SLAB / 256) {
        const int co = threadIdx.x;
        if (co >= G::COUT || !db) return;
        KahanSum s;
        for (int q = 0; q < 2 * slabs; ++q)                             // rows 2 q, 2 q + 1 of slab q: the sum and its compensation
            for (int u = 0; u < G::N / G::COUT; ++u) s.add(pbias[(int64_t)q * G::NP + u * G::COUT + co]);
        db[co] = s.s - s.c;
        return;
    }
    const int col = idx & 31, row = (idx >> 5) & 31, ut = idx >> 10, tap = ut % G::TAPS, pair = ut / G::TAPS;
    const int n = (pair / G::CB) * 32 + row, ci = (pair % G::CB) * 32 + col;
    if (n >= G::N || ci >= C) return;
    int o;
    if constexpr (G::SUB) {
        const int q = n >> 4, co = n & 15, py = q >> 1, px = q & 1, dy = tap >> 1, dx = tap & 1;
        const int ky = py ? (dy ? 0 : 2) : (dy ? -1 : 1), kx = px ? (dx ? 0 : 2) : (dx ? -1 : 1);
        if (ky < 0 || kx < 0) return;                                   // no tap of the transposed conv
        o = (ci * 16 + co) * 9 + ky * 3 + kx;
    } else {
        o = (n * C + ci) * 9 + tap;
    }
    float s = 0.f;
    for (int q = 0; q < slabs; ++q) s += part[(int64_t)q * G::SLAB + idx];
    dW[o] = s;
}

struct S1WArgs { const void *x, *g; float *dW, *db, *ws; int64_t B, H, W; hipStream_t st; };
int64_t s1w_tiles(int64_t B, int64_t H, int64_t W) { return B * ((H + S1_TH - 1) / S1_TH) * ((W + S1_TW - 1) / S1_TW); }
template <typename T, int C, int FORM> int conv_s1_wgrad_launch(const S1WArgs& a) {
    using G = S1WGeom<T, C, FORM>;
    static_assert(G::LDS <= CVAE_LDS_MAX, "tile does not fit a workgroup's LDS");
    constexpr auto kern = conv_s1_wgrad_kernel<T, C, FORM>;
    if (cvae_allow_lds<kern>(G::LDS) != CVAE_OK) return CVAE_E_LAUNCH;
    const int tiles_x = (int)((a.W + S1_TW - 1) / S1_TW), tiles_y = (int)((a.H + S1_TH - 1) / S1_TH), tiles = (int)s1w_tiles(a.B, a.H, a.W);
    const int slabs = tiles < G::MAX_SLABS ? tiles : G::MAX_SLABS;
    float* pbias = a.ws + (int64_t)slabs * G::SLAB;
    hipLaunchKernelGGL(kern, dim3((unsigned)slabs, G::GROUPS), dim3(256), G::LDS, a.st, (const T*)a.x, (const T*)a.g, a.ws, pbias, (int)a.H, (int)a.W, tiles_x, tiles_y,
                       tiles, slabs);
    CVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL((s1w_finish_kernel<C, FORM>), dim3(G::SLAB / 256 + 1), dim3(256), 0, a.st, (const float*)a.ws, (const float*)pbias, a.dW, a.db, slabs);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
// f(Int<C>{}, Int<FORM>{}) for a supported (C, form); false otherwise
template <typename F> bool s1w_with_layer(int64_t C, int form, F&& f) {
    if (form == CVAE_CONV_S1_K3) {
        if (C == 16) return f(Int<16>{}, Int<CVAE_CONV_S1_K3>{}), true;
        if (C == 32) return f(Int<32>{}, Int<CVAE_CONV_S1_K3>{}), true;
        if (C == 64) return f(Int<64>{}, Int<CVAE_CONV_S1_K3>{}), true;
        if (C == 128) return f(Int<128>{}, Int<CVAE_CONV_S1_K3>{}), true;
    } else if (form == CVAE_CONV_S1_SUBPIXEL) {
        if (C == 16) return f(Int<16>{}, Int<CVAE_CONV_S1_SUBPIXEL>{}), true;
        if (C == 32) return f(Int<32>{}, Int<CVAE_CONV_S1_SUBPIXEL>{}), true;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------ weight gradient of Conv2d(16 -> 1, k3, s1, p1)
// dW[ci][ky][kx] = sum over pixels q of x[q][ci] g[q - (ky - 1, kx - 1)], dbias = sum g: 145 sums over all pixels.  A thread walks pixels i, i + 256 blocks, ..
// with its 145 sums in registers (x read once with 16-byte loads, the nine g values from the cache); a workgroup adds its threads' sums in a fixed tree and
// leaves 145 partials; c1w_finish adds the workgroups in order.
#define C1W_MAX_BLOCKS 1024
#define C1W_SUMS (9 * C1_CIN + 1)
#define C1W_PITCH 148
template <typename T>
__global__ __launch_bounds__(256) void conv_s1_c1_wgrad_kernel(const T* __restrict__ x, const float* __restrict__ g, float* __restrict__ part, int64_t B, int H, int W) {
    __shared__ float red[4][C1W_SUMS];
    float acc[9][C1_CIN], bs = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ci = 0; ci < C1_CIN; ++ci) acc[tap][ci] = 0.f;
    const int64_t total = B * H * W;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xx = (int)(i % W), yy = (int)((i / W) % H);
        const float* gb = g + (i / ((int64_t)W * H)) * (int64_t)H * W;
        float xv[C1_CIN];
        load_f32(x + i * C1_CIN, xv);
        bs += gb[(int64_t)yy * W + xx];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int sy = yy + 1 - ky, sx = xx + 1 - kx;
                const float gv = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? gb[(int64_t)sy * W + sx] : 0.f;
#pragma unroll
                for (int ci = 0; ci < C1_CIN; ++ci) acc[ky * 3 + kx][ci] = fmaf(xv[ci], gv, acc[ky * 3 + kx][ci]);
            }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ci = 0; ci < C1_CIN; ++ci) {
            const float v = wave_sum(acc[tap][ci]);
            if (lane == 0) red[wave][tap * C1_CIN + ci] = v;
        }
    bs = wave_sum(bs);
    if (lane == 0) red[wave][9 * C1_CIN] = bs;
    __syncthreads();
    if (threadIdx.x < C1W_SUMS) part[(int64_t)blockIdx.x * C1W_PITCH + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
__global__ __launch_bounds__(256) void c1w_finish_kernel(const float* __restrict__ part, float* __restrict__ dW, float* __restrict__ db, int blocks) {
    const int i = threadIdx.x;
    if (i >= C1W_SUMS) return;
    float s = 0.f;
    for (int q = 0; q < blocks; ++q) s += part[(int64_t)q * C1W_PITCH + i];
    if (i == 9 * C1_CIN) {
        if (db) db[0] = s;
    } else {
        dW[(i % C1_CIN) * 9 + i / C1_CIN] = s;                         // [1][ci][ky][kx]
    }
}
int64_t c1w_blocks(int64_t B, int64_t H, int64_t W) {
    const int64_t n = (B * H * W + 255) / 256;
    return n < C1W_MAX_BLOCKS ? n : C1W_MAX_BLOCKS;
}

// ------------------------------------------------------------------------------------------------ weight gradient of latent -> grid
// dW[n][k] = sum_b G[b][n] z[b][k], n = c P + p, G[b][c P + p] = g[b][p][c]; dbias[n] = sum_b G[b][n].  A workgroup owns 16 consecutive rows n: thread i
// holds float4 pieces i, i + 256, .. of the 16 x K block in registers and adds the batch rows in order, 16 at a time through LDS (z and the 16 x 16 g values);
// the block leaves once, 16-byte stores along the rows.
#define L2GW_ROWS 16
template <typename T>
__global__ __launch_bounds__(256) void l2g_wgrad_kernel(const T* __restrict__ g, const float* __restrict__ z, float* __restrict__ dW, float* __restrict__ db, int64_t B,
                                                        int K, int64_t P, int C) {
    __shared__ __attribute__((aligned(16))) float zs[L2G_BT * L2G_KMAX];
    __shared__ float gsm[L2G_BT][L2GW_ROWS];
    const int t = threadIdx.x, k4 = K >> 2, items = L2GW_ROWS * k4;
    const int64_t n0 = (int64_t)blockIdx.x * L2GW_ROWS, N = P * C;
    constexpr int PER = L2GW_ROWS * (L2G_KMAX / 4) / 256;
    float4 acc[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    float bsum = 0.f;
    for (int64_t b0 = 0; b0 < B; b0 += L2G_BT) {
        const int nb = (int)(B - b0 < L2G_BT ? B - b0 : L2G_BT);
        __syncthreads();
        for (int i = t; i < nb * k4; i += 256) ((float4*)zs)[i] = ((const float4*)(z + b0 * K))[i];
        {
            const int bb = t >> 4, rr = t & 15;
            const int64_t n = n0 + rr;
            gsm[bb][rr] = (bb < nb && n < N) ? to_f32(g[((b0 + bb) * P + n % P) * C + n / P]) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = t + 256 * j;
            if (i < items) {
                const int row = i / k4, kq = i - row * k4;
                for (int bb = 0; bb < nb; ++bb) {
                    const float gv = gsm[bb][row];
                    const float4 zv = ((const float4*)zs)[bb * k4 + kq];
                    acc[j].x = fmaf(gv, zv.x, acc[j].x); acc[j].y = fmaf(gv, zv.y, acc[j].y);
                    acc[j].z = fmaf(gv, zv.z, acc[j].z); acc[j].w = fmaf(gv, zv.w, acc[j].w);
                }
            }
        }
        if (t < L2GW_ROWS)
            for (int bb = 0; bb < nb; ++bb) bsum += gsm[bb][t];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = t + 256 * j;
        if (i < items) {
            const int row = i / k4, kq = i - row * k4;
            if (n0 + row < N) ((float4*)(dW + (n0 + row) * K))[kq] = acc[j];
        }
    }
    if (db && t < L2GW_ROWS && n0 + t < N) db[n0 + t] = bsum;
}

}  // namespace

extern "C" size_t cvae_conv_s1_wgrad_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int form) {
    if (B <= 0 || !s1_dims_ok(B, H, W) || s1w_tiles(B, H, W) > 0x7fffffff) return 0;
    size_t n = 0;
    s1w_with_layer(C, form, [&](auto cv, auto fv) {
        using G = S1WGeom<float, decltype(cv)::value, decltype(fv)::value>;
        const int64_t tiles = s1w_tiles(B, H, W), slabs = tiles < G::MAX_SLABS ? tiles : G::MAX_SLABS;
        n = (size_t)slabs * (G::SLAB + 2 * G::NP) * sizeof(float);
    });
    return n;
}

extern "C" int cvae_conv_s1_wgrad(const void* x, const void* g, float* dW, float* dbias, int64_t B, int64_t H, int64_t W, int64_t C, int form, int dtype,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0 || !s1_dims_ok(B, H, W) || s1w_tiles(B, H, W) > 0x7fffffff) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    const size_t need = cvae_conv_s1_wgrad_workspace_bytes(B, H, W, C, form);
    if (need == 0) return CVAE_E_UNSUPPORTED;
    if (!x || !g || !dW) return CVAE_E_NULLPTR;
    if (!aligned16(x) || !aligned16(g) || !aligned16(workspace)) return CVAE_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < need) return CVAE_E_WORKSPACE;
    const S1WArgs a{x, g, dW, dbias, (float*)workspace, B, H, W, (hipStream_t)stream};
    return with_dtype(dtype, [&](auto tv) {
        int rc = CVAE_E_UNSUPPORTED;
        s1w_with_layer(C, form, [&](auto cv, auto fv) { rc = conv_s1_wgrad_launch<decltype(tv), decltype(cv)::value, decltype(fv)::value>(a); });
        return rc;
    });
}

extern "C" size_t cvae_conv_s1_c1_wgrad_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (B <= 0 || !c1_dims_ok(B, H, W)) return 0;
    return (size_t)c1w_blocks(B, H, W) * C1W_PITCH * sizeof(float);
}

extern "C" int cvae_conv_s1_c1_wgrad(const void* x, const float* g, float* dW, float* dbias, int64_t B, int64_t H, int64_t W, int64_t Cin, int dtype, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (B <= 0 || !c1_dims_ok(B, H, W)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (Cin != C1_CIN) return CVAE_E_UNSUPPORTED;
    if (!x || !g || !dW) return CVAE_E_NULLPTR;
    if (!aligned16(x)) return CVAE_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < cvae_conv_s1_c1_wgrad_workspace_bytes(B, H, W)) return CVAE_E_WORKSPACE;
    const int blocks = (int)c1w_blocks(B, H, W);
    const hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int rc = with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(conv_s1_c1_wgrad_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, g, part, B, (int)H, (int)W);
        return launch_rc();
    });
    if (rc != CVAE_OK) return rc;
    hipLaunchKernelGGL(c1w_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)part, dW, dbias, blocks);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" int cvae_latent_to_grid_wgrad(const void* g, const float* z, float* dW, float* dbias, int64_t B, int64_t K, int64_t P, int64_t C, int dtype, void* stream) {
    if (B <= 0 || K <= 0 || P <= 0 || C <= 0 || P * C > ((int64_t)1 << 40)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (K > L2G_KMAX || (K & 3) || (C & 31)) return CVAE_E_UNSUPPORTED;
    if (!g || !z || !dW) return CVAE_E_NULLPTR;
    if (!aligned16(z) || !aligned16(dW)) return CVAE_E_UNSUPPORTED;
    const int64_t blocks = (P * C + L2GW_ROWS - 1) / L2GW_ROWS;
    if (blocks > 0x7fffffff) return CVAE_E_BADSHAPE;
    const hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(l2g_wgrad_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)g, z, dW, dbias, B, (int)K, P, (int)C);
        return launch_rc();
    });
}

extern "C" int64_t cvae_conv_s1_weight_elems(int64_t Cin, int64_t Cout, int form) {
    if (form == CVAE_CONV_S1_K3) return (Cin == Cout && (Cin == 32 || Cin == 64 || Cin == 128)) ? Cout * ((9 * Cin + S1_KPAD - 1) / S1_KPAD * S1_KPAD) : 0;
    if (form == CVAE_CONV_S1_SUBPIXEL) return (Cout == 16 && (Cin == 32 || Cin == 16)) ? 4 * Cout * ((4 * Cin + S1_KPAD - 1) / S1_KPAD * S1_KPAD) : 0;
    if (form == CVAE_CONV_S1_SUBPIXEL_T) return (Cout == 16 && (Cin == 32 || Cin == 16)) ? 32 * 256 : 0;      // the backward matrix [32][4 taps x 64]
    return 0;
}

extern "C" int cvae_conv_s1_pack_weights(int count, const float* const* w, void* const* packed, const int64_t* n, void* stream) {
    if (count <= 0) return CVAE_E_BADSHAPE;
    if (count > S1_PACK_MAX) return CVAE_E_UNSUPPORTED;
    if (!w || !packed || !n) return CVAE_E_NULLPTR;
    PackTable T{};
    T.count = count;
    int64_t blocks = 0;
    for (int k = 0; k < count; ++k) {
        if (n[k] <= 0 || (n[k] & 3) || n[k] > ((int64_t)1 << 30)) return CVAE_E_BADSHAPE;
        if (!w[k] || !packed[k]) return CVAE_E_NULLPTR;
        if (!aligned16(w[k]) || ((uintptr_t)packed[k] & 7)) return CVAE_E_UNSUPPORTED;
        T.src[k] = w[k]; T.dst[k] = (bf16*)packed[k]; T.n4[k] = n[k] >> 2;
        blocks += (T.n4[k] + 255) / 256;
        T.end[k] = (int)blocks;
    }
    hipLaunchKernelGGL(conv_s1_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" int cvae_conv_s1(const void* x, const void* w, const float* bias, const void* resid, void* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                            int form, int dtype, int act, void* stream) {
    if (!s1_dims_ok(B, H, W)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (form != CVAE_CONV_S1_K3 && form != CVAE_CONV_S1_SUBPIXEL) return CVAE_E_UNSUPPORTED;
    if (cvae_conv_s1_weight_elems(Cin, Cout, form) == 0 || !s1_act_ok(act)) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!x || !w || !bias || !y) return CVAE_E_NULLPTR;
    if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y) || !aligned16(resid)) return CVAE_E_UNSUPPORTED;
    const S1Args a{x, w, bias, resid, nullptr, y, B, H, W, act, (hipStream_t)stream};
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        if (form == CVAE_CONV_S1_K3) return conv_s1_k3<T, false>(Cin, a);
        if (Cin == 32) return conv_s1_launch<T, 32, 2, CVAE_CONV_S1_SUBPIXEL>(a);
        return conv_s1_launch<T, 16, 2, CVAE_CONV_S1_SUBPIXEL>(a);
    });
}

extern "C" int cvae_conv_s1_c1(const void* x, const float* w, const float* bias, float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int dtype, int act,
                               void* stream) {
    if (!c1_dims_ok(B, H, W)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (Cin != C1_CIN) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!x || !w || !y) return CVAE_E_NULLPTR;
    if (!aligned16(x) || !aligned16(y)) return CVAE_E_UNSUPPORTED;
    const int64_t total = B * H * ((W + 3) >> 2), blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) return CVAE_E_BADSHAPE;
    const hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(conv_s1_c1_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, w, bias, y, B, (int)H, (int)W, act);
        return launch_rc();
    });
}

extern "C" int cvae_latent_to_grid(const float* z, const float* W, const float* bias, void* out, int64_t B, int64_t K, int64_t P, int64_t C, int dtype, void* stream) {
    if (B < 0 || K <= 0 || P <= 0 || C <= 0 || P * C > ((int64_t)1 << 40)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (B > L2G_BT || K > L2G_KMAX || (K & 3) || (C & 31)) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!z || !W || !out) return CVAE_E_NULLPTR;
    if (!aligned16(z) || !aligned16(W)) return CVAE_E_UNSUPPORTED;
    const int64_t blocks = (P * (C >> 5) + 3) / 4;
    if (blocks > 0x7fffffff) return CVAE_E_BADSHAPE;
    const hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(latent_to_grid_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, z, W, bias, (T*)out, (int)B, (int)K, P, (int)C);
        return launch_rc();
    });
}

extern "C" int cvae_conv_s1_bwd_data(const void* g, const void* w, const void* resid, const void* gate, void* dx, int64_t B, int64_t H, int64_t W, int64_t C, int form,
                                     int dtype, int gate_act, void* stream) {
    if (!s1_dims_ok(B, H, W)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (form != CVAE_CONV_S1_K3 && form != CVAE_CONV_S1_SUBPIXEL_T) return CVAE_E_UNSUPPORTED;
    if (cvae_conv_s1_weight_elems(C, form == CVAE_CONV_S1_K3 ? C : 16, form) == 0 || !s1_act_ok(gate_act)) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!g || !w || !dx || (gate_act != CVAE_ACT_NONE && !gate)) return CVAE_E_NULLPTR;
    if (!aligned16(g) || !aligned16(w) || !aligned16(dx) || !aligned16(resid) || !aligned16(gate)) return CVAE_E_UNSUPPORTED;
    if (gate_act == CVAE_ACT_NONE) gate = nullptr;
    const S1Args a{g, w, nullptr, resid, gate, dx, B, H, W, gate_act, (hipStream_t)stream};
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        if (form == CVAE_CONV_S1_K3) return conv_s1_k3<T, true>(C, a);
        if (C == 32) return conv_s1_launch<T, 64, 1, CVAE_CONV_S1_SUBPIXEL_T, true, 32>(a);
        return conv_s1_launch<T, 64, 1, CVAE_CONV_S1_SUBPIXEL_T, true, 16>(a);
    });
}

extern "C" int cvae_conv_s1_c1_bwd_data(const float* g, const float* w, const void* gate, void* dx, int64_t B, int64_t H, int64_t W, int64_t Cin, int dtype, int gate_act,
                                        void* stream) {
    if (!c1_dims_ok(B, H, W)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (Cin != C1_CIN) return CVAE_E_UNSUPPORTED;
    if (!s1_act_ok(gate_act)) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!g || !w || !dx || (gate_act != CVAE_ACT_NONE && !gate)) return CVAE_E_NULLPTR;
    if (!aligned16(dx) || !aligned16(gate)) return CVAE_E_UNSUPPORTED;
    if (gate_act == CVAE_ACT_NONE) gate = nullptr;
    const int64_t blocks = (B * H * W + 255) / 256;
    if (blocks > 0x7fffffff) return CVAE_E_BADSHAPE;
    const hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(conv_s1_c1_bwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, g, w, (const T*)gate, (T*)dx, B, (int)H, (int)W, gate_act);
        return launch_rc();
    });
}

extern "C" size_t cvae_latent_to_grid_bwd_workspace_bytes(int64_t B, int64_t K, int64_t P, int64_t C) {
    if (B <= 0 || B > L2G_BT || K <= 0 || K > L2G_KMAX || P <= 0 || C <= 0 || (C & 31) || P * C > ((int64_t)1 << 40)) return 0;
    return (size_t)l2g_bwd_slabs(P, C) * B * K * sizeof(float);
}

extern "C" int cvae_latent_to_grid_bwd(const void* g, const float* W, float* dz, int64_t B, int64_t K, int64_t P, int64_t C, int dtype, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (B < 0 || K <= 0 || P <= 0 || C <= 0 || P * C > ((int64_t)1 << 40)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (B > L2G_BT || K > L2G_KMAX || (K & 3) || (C & 31)) return CVAE_E_UNSUPPORTED;
    if (B == 0) return CVAE_OK;
    if (!g || !W || !dz) return CVAE_E_NULLPTR;
    if (!aligned16(W) || !aligned16(workspace)) return CVAE_E_UNSUPPORTED;
    const int64_t slabs = l2g_bwd_slabs(P, C);
    if (slabs > 0x7fffffff) return CVAE_E_BADSHAPE;
    if (!workspace || workspace_bytes < cvae_latent_to_grid_bwd_workspace_bytes(B, K, P, C)) return CVAE_E_WORKSPACE;
    const int kq_pad = l2g_bwd_kq_pad(K), RP = 256 / kq_pad;
    const size_t lds = ((size_t)B * L2GB_ROWS + (size_t)RP * B * K) * sizeof(float);         // at most 16 KB + 64 KB
    const hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int rc = with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        if (cvae_allow_lds<l2g_bwd_kernel<T>>(lds) != CVAE_OK) return CVAE_E_LAUNCH;
        hipLaunchKernelGGL(l2g_bwd_kernel<T>, dim3((unsigned)slabs), dim3(256), lds, st, (const T*)g, W, part, (int)B, (int)K, P, (int)C, kq_pad);
        return launch_rc();
    });
    if (rc != CVAE_OK) return rc;
    const int n = (int)(B * K);
    hipLaunchKernelGGL(l2g_bwd_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)part, dz, n, (int)slabs);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
