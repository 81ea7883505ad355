// vessel_infer.hip — the eval-mode (inference) side of CausalVesselVAE (vessel_analysis/00_core/models.py:9-166 of the reference):
//   * BatchNorm2d on running statistics folded into the conv that precedes it, for a table of layers in ONE launch;
//   * per-row difference norms ||a[r] - b[ref[r]]|| (feature-importance / m-influence sweeps), two-level fixed-order sums;
//   * the element-wise mean and unbiased std over K equal-length tensors (ensembles of fold models).
//
// The fold, per output channel c:  s = gamma[c] rsqrt(var[c] + eps),  w'[c] = w[c] s,  b'[c] = (b[c] - mean[c]) s + beta[c]
// (the same rsqrt(var + eps) form as BatchNorm2dAct's eval branch).  A Conv2d(k4) weight [Cout][Cin][4][4] keeps its layout; an
// UpConv2dK3 weight [Cout][Cin][3][3] leaves as the transposed k4 weight [Cin][Cout][4][4] = A W3 A^T of cvae_conv3_to_k4 (same sums in the
// same order, so an entry without BatchNorm reproduces cvae_conv3_to_k4's bits).  A Conv2d(k3, s2, p1) weight [Cout][Cin][3][3] (the ViT-VAE stem) leaves as
// the k4/s2/p1 weight [Cout][Cin][4][4] whose fourth row and column are zero: both read in[2o - 1 + k], so the products are the same.
// The ViT-VAE decoder adds three kinds: a ConvTranspose2d(k3, s2, p1, output_padding 1) weight zero-embedded into the transposed k4 weight (scale per
// Cout = dimension 1), and the GEMM matrices csrc/conv_s1.hip reads for a Conv2d(k3, s1, p1) and for the sub-pixel form of the narrow transposed convs.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ fold table
#define FOLD_MAX 16
#define FOLD_K3_TILE 16           // (cout, cin) tile of an UpConv2dK3 entry: 16 x 16 weights through LDS
#define FOLD_K4_PER_BLOCK 1024    // float4 groups per block of a Conv2d(k4) entry: 4 per thread, loads issued together

struct FoldEntry {
    const float* w;
    const float* bias;
    const float* gamma;
    const float* beta;
    const float* mean;
    const float* var;
    float* w_out;
    float* b_out;
    float eps;
    int kind;
    int cout, cin;
    int wblocks;                  // blocks of this entry's weight part; one more block range of ceil(cout / 256) does the bias
    int bblocks;
};
struct FoldTable {
    FoldEntry e[FOLD_MAX];
    int end[FOLD_MAX];            // exclusive prefix sums of wblocks + bblocks
    int count;
};

__device__ __forceinline__ float fold_scale(const FoldEntry& E, int c) {
    return E.gamma ? E.gamma[c] * rsqrtf(E.var[c] + E.eps) : 1.f;
}

__constant__ const float A43f[4][3] = {{0.f, 0.f, 1.f}, {0.f, 1.f, 1.f}, {1.f, 1.f, 0.f}, {1.f, 0.f, 0.f}};

__global__ __launch_bounds__(256) void fold_bn_conv_kernel(const FoldTable T) {
    __shared__ float tile[FOLD_K3_TILE][FOLD_K3_TILE * 9 + 4];         // [cout][cin * 9 + tap]; +4: rows stay 16-byte aligned
    __shared__ float scale[FOLD_K3_TILE];
    int k = 0;
    while (k < T.count - 1 && (int)blockIdx.x >= T.end[k]) ++k;
    const FoldEntry& E = T.e[k];
    const int blk = (int)blockIdx.x - (k ? T.end[k - 1] : 0), t = threadIdx.x;
    if (blk >= E.wblocks) {                                            // bias part
        const int c = (blk - E.wblocks) * 256 + t;
        if (c < E.cout) {
            const float b = E.bias ? E.bias[c] : 0.f;
            E.b_out[c] = E.gamma ? (b - E.mean[c]) * fold_scale(E, c) + E.beta[c] : b;
        }
        return;
    }
    if (E.kind == CVAE_FOLD_CONV_K4) {
        // [Cout][Cin][16]: a float4 group is 4 consecutive taps of one (cout, cin); cout = group / (Cin * 4)
        const int64_t n4 = (int64_t)E.cout * E.cin * 4, per_c = (int64_t)E.cin * 4;
        const int64_t g0 = (int64_t)blk * FOLD_K4_PER_BLOCK + t;
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t g = g0 + u * 256;
            if (g < n4) v[u] = ((const float4*)E.w)[g];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t g = g0 + u * 256;
            if (g < n4) {
                const float s = fold_scale(E, (int)(g / per_c));
                ((float4*)E.w_out)[g] = make_float4(v[u].x * s, v[u].y * s, v[u].z * s, v[u].w * s);
            }
        }
        return;
    }
    if (E.kind == CVAE_FOLD_CONV_K3S2) {
        // [Cout][Cin][3][3] -> [Cout][Cin][4][4] with a zero fourth row and column: a float4 group is the 4 kw taps of one (cout, cin, kh)
        const int64_t n4 = (int64_t)E.cout * E.cin * 4, per_c = (int64_t)E.cin * 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t g = (int64_t)blk * FOLD_K4_PER_BLOCK + t + u * 256;
            if (g < n4) {
                const int kh = (int)(g & 3);
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kh < 3) {
                    const float* w3 = E.w + (g >> 2) * 9 + kh * 3;
                    const float s = fold_scale(E, (int)(g / per_c));
                    o = make_float4(w3[0] * s, w3[1] * s, w3[2] * s, 0.f);
                }
                ((float4*)E.w_out)[g] = o;
            }
        }
        return;
    }
    if (E.kind == CVAE_FOLD_CONVT_K3S2) {
        // ConvTranspose2d(k3, s2, p1, output_padding 1) [Cin][Cout][3][3] -> the transposed k4/s2/p1 weight [Cin][Cout][4][4] with a zero fourth row and column
        // (both scatter in[i] to out[2 i - 1 + k]; the k4 extent 2 n is the k3 extent with output_padding 1); the scale runs over Cout, dimension 1
        const int64_t n4 = (int64_t)E.cout * E.cin * 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t g = (int64_t)blk * FOLD_K4_PER_BLOCK + t + u * 256;
            if (g < n4) {
                const int kh = (int)(g & 3);
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kh < 3) {
                    const float* w3 = E.w + (g >> 2) * 9 + kh * 3;
                    const float s = fold_scale(E, (int)((g >> 2) % E.cout));
                    o = make_float4(w3[0] * s, w3[1] * s, w3[2] * s, 0.f);
                }
                ((float4*)E.w_out)[g] = o;
            }
        }
        return;
    }
    if (E.kind == CVAE_FOLD_CONV_K3S1 || E.kind == CVAE_FOLD_CONVT_K3S2_SUBPIXEL || E.kind == CVAE_FOLD_CONV_K3S1_GRAD || E.kind == CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD) {
        // the GEMM matrix [N][KT] of cvae_conv_s1 (csrc/conv_s1.hip), k = tap * Cin + ci, KT = K rounded up to 64 with zero columns; a float4 group is 4
        // consecutive ci of one (n, tap).  K3S1: Conv2d [Cout][Cin][3][3], N = Cout, tap = ky * 3 + kx.  SUBPIXEL: ConvTranspose2d [Cin][Cout][3][3],
        // N = 4 Cout with n = (py * 2 + px) * Cout + co, tap = dy * 2 + dx, k index per direction: parity 0: {d 0 -> k 1}; parity 1: {d 0 -> k 2, d 1 -> k 0}
        // The _GRAD kinds append the input gradient's matrix (cvae_conv_s1_bwd_data) behind the forward one.  K3: [Cin][KTb], k = tap' * Cout + co,
        // w[co][ci][8 - tap'] s[co] (taps flipped, channels transposed).  SUBPIXEL: [32][256], k = (dy 2 + dx) 64 + (py 2 + px) 16 + co over the
        // space-to-depth view of the gradient, tap index per direction 2 d + parity - 1 (negative: no tap), rows ci >= Cin zero.
        const bool sp = E.kind == CVAE_FOLD_CONVT_K3S2_SUBPIXEL || E.kind == CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD;
        const bool grad = E.kind == CVAE_FOLD_CONV_K3S1_GRAD || E.kind == CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD;
        const int ktb4 = sp ? 64 : ((9 * E.cout + 63) / 64 * 64) >> 2;
        const int64_t nb4 = grad ? (int64_t)(sp ? 32 : E.cin) * ktb4 : 0;
        const int taps = sp ? 4 : 9, N = sp ? 4 * E.cout : E.cout;
        const int K = taps * E.cin, KT = (K + 63) / 64 * 64, kt4 = KT >> 2;
        const int64_t n4 = (int64_t)N * kt4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t g = (int64_t)blk * FOLD_K4_PER_BLOCK + t + u * 256;
            if (g >= n4 && g < n4 + nb4) {
                const int64_t gb = g - n4;
                const int ci = (int)(gb / ktb4), k = (int)(gb - (int64_t)ci * ktb4) * 4;
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if (!sp) {
                    const int tap = k / E.cout, co = k - tap * E.cout;
                    if (tap < 9) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = E.w[((size_t)(co + e) * E.cin + ci) * 9 + 8 - tap] * fold_scale(E, co + e);
                    }
                } else {
                    const int tap = k >> 6, q = (k >> 4) & 3, co = k & 15;
                    const int ky = 2 * (tap >> 1) + (q >> 1) - 1, kx = 2 * (tap & 1) + (q & 1) - 1;
                    if (ci < E.cin && ky >= 0 && kx >= 0) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = E.w[((size_t)ci * E.cout + co + e) * 9 + ky * 3 + kx] * fold_scale(E, co + e);
                    }
                }
                ((float4*)E.w_out)[g] = make_float4(o[0], o[1], o[2], o[3]);
            }
            if (g < n4) {
                const int n = (int)(g / kt4), k = (int)(g - (int64_t)n * kt4) * 4;
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if (k < K) {
                    const int tap = k / E.cin, ci = k - tap * E.cin;
                    if (!sp) {
                        const float s = fold_scale(E, n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = E.w[((size_t)n * E.cin + ci + e) * 9 + tap] * s;
                    } else {
                        const int q = n / E.cout, co = n - q * E.cout, py = q >> 1, px = q & 1, dy = tap >> 1, dx = tap & 1;
                        const int ky = py ? (dy ? 0 : 2) : (dy ? -1 : 1), kx = px ? (dx ? 0 : 2) : (dx ? -1 : 1);
                        if (ky >= 0 && kx >= 0) {
                            const float s = fold_scale(E, co);
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] = E.w[((size_t)(ci + e) * E.cout + co) * 9 + ky * 3 + kx] * s;
                        }
                    }
                }
                ((float4*)E.w_out)[g] = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        return;
    }
    // UpConv2dK3: tile (co0 .. co0 + 16) x (ci0 .. ci0 + 16).  In: row cout of the tile is w3[cout][ci0 .. ci0 + nci][9], nci * 9 contiguous floats
    // (16-byte loads when Cin % 4 == 0: the row start (cout Cin + ci0) * 9 floats is then a multiple of 4).  Out: k4[cin][co0 .. co0 + nco][16],
    // nco * 16 contiguous floats per cin — one float4 (4 kw taps of one kh) per thread and step.
    const int tiles_ci = (E.cin + FOLD_K3_TILE - 1) / FOLD_K3_TILE;
    const int co0 = (blk / tiles_ci) * FOLD_K3_TILE, ci0 = (blk % tiles_ci) * FOLD_K3_TILE;
    const int nco = min(FOLD_K3_TILE, E.cout - co0), nci = min(FOLD_K3_TILE, E.cin - ci0);
    const int rowf = nci * 9;
    if ((E.cin & 3) == 0) {
        const int row4 = rowf >> 2;
        for (int i = t; i < nco * row4; i += 256) {
            const int r = i / row4, q = i - r * row4;
            const float4 x = ((const float4*)(E.w + ((size_t)(co0 + r) * E.cin + ci0) * 9))[q];
            *(float4*)&tile[r][q * 4] = x;
        }
    } else {
        for (int i = t; i < nco * rowf; i += 256) {
            const int r = i / rowf, q = i - r * rowf;
            tile[r][q] = E.w[((size_t)(co0 + r) * E.cin + ci0) * 9 + q];
        }
    }
    if (t < nco) scale[t] = fold_scale(E, co0 + t);
    __syncthreads();
    for (int i = t; i < nci * nco * 4; i += 256) {
        const int ci = i / (nco * 4), rem = i - ci * nco * 4, co = rem >> 2, kh = rem & 3;
        const float* w = &tile[co][ci * 9];
        float o[4];
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) {
            float v = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) v += A43f[kh][a] * A43f[kw][b] * w[a * 3 + b];
            o[kw] = E.gamma ? v * scale[co] : v;
        }
        ((float4*)(E.w_out + ((size_t)(ci0 + ci) * E.cout + co0 + co) * 16))[kh] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ------------------------------------------------------------------------------------------------ row difference norms
// Level 1: block (chunk, row) sums (a - b)^2 and |a - b| over CHUNK elements of one row: 256 threads x ROWDIFF_ITER groups of E
// elements (E = one 16-byte load: 4 fp32 / 8 bf16), each thread in (iter, element) order, then the wave sums (xor shuffles) and the four waves
// in index order -> part[row][chunk][2].  Level 2: one wave per row (row_diff_finish_kernel).  The geometry depends on n only, so a
// row's bits do not depend on how many rows share the launch.
#define ROWDIFF_ITER 4
template <typename T> struct RowDiffGeom {
    static constexpr int E = 16 / sizeof(T);
    static constexpr int64_t CHUNK = (int64_t)256 * ROWDIFF_ITER * E;
};

template <typename T>
__global__ __launch_bounds__(256) void row_diff_partial_kernel(const T* __restrict__ a, const T* __restrict__ b, const int64_t* __restrict__ ref,
                                                               float* __restrict__ part, int64_t rows, int64_t b_rows, int64_t n, int64_t chunks, int vec) {
    constexpr int E = RowDiffGeom<T>::E;
    __shared__ float red[2][4];
    const int t = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const int64_t rb = ref ? ref[r] : r;
        float ss = 0.f, sa = 0.f;
        if (rb >= 0 && rb < b_rows) {
            const T* pa = a + r * n;
            const T* pb = b + rb * n;
            __attribute__((aligned(16))) T ra[ROWDIFF_ITER][E], rv[ROWDIFF_ITER][E];     // raw 16-byte pieces: all loads in flight before the arithmetic
#pragma unroll
            for (int it = 0; it < ROWDIFF_ITER; ++it) {
                const int64_t e0 = chunk * RowDiffGeom<T>::CHUNK + ((int64_t)it * 256 + t) * E;
                if (vec && e0 + E <= n) {
                    *(uint4*)ra[it] = *(const uint4*)(pa + e0);
                    *(uint4*)rv[it] = *(const uint4*)(pb + e0);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const bool in = e0 + e < n;
                        ra[it][e] = in ? pa[e0 + e] : from_f32<T>(0.f);
                        rv[it][e] = in ? pb[e0 + e] : from_f32<T>(0.f);
                    }
                }
            }
#pragma unroll
            for (int it = 0; it < ROWDIFF_ITER; ++it)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float d = to_f32(ra[it][e]) - to_f32(rv[it][e]);
                    ss += d * d;
                    sa += fabsf(d);
                }
        } else {
            ss = sa = __builtin_nanf("");                              // ref outside b: the row's results are NaN (nothing is read)
        }
        ss = wave_sum(ss);
        sa = wave_sum(sa);
        __syncthreads();
        if ((t & 63) == 0) { red[0][t >> 6] = ss; red[1][t >> 6] = sa; }
        __syncthreads();
        if (t == 0) {
            part[(r * chunks + chunk) * 2 + 0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            part[(r * chunks + chunk) * 2 + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
    }
}
// one wave per row: lane l adds chunks l, l + 64, .. in order, then the xor-shuffle tree of wave_sum (fixed for a given chunk count)
__global__ __launch_bounds__(64) void row_diff_finish_kernel(const float* __restrict__ part, float* __restrict__ l2, float* __restrict__ mean_abs, int64_t rows,
                                                             int64_t chunks, float inv_n) {
    const int64_t r = blockIdx.x;
    const int l = threadIdx.x;
    float ss = 0.f, sa = 0.f;
    for (int64_t c = l; c < chunks; c += 64) {
        const float2 q = ((const float2*)part)[r * chunks + c];
        ss += q.x;
        sa += q.y;
    }
    ss = wave_sum(ss);
    sa = wave_sum(sa);
    if (l == 0) {
        l2[r] = sqrtf(ss);
        if (mean_abs) mean_abs[r] = sa * inv_n;
    }
}

// ------------------------------------------------------------------------------------------------ the way back through the fold
// One workgroup per (layer, BatchNorm channel c): thread t walks elements t, t + 256, .. of the channel's Cin x 9 weights (dw = s dwf written on the way, the
// products dwf w added in that order), then a fixed tree over the workgroup; thread 0 finishes db, dgamma and dbeta.
struct FoldBwdEntry {
    const float *w, *bias, *gamma, *mean, *var, *dwf, *dbf;
    float *dw, *db, *dgamma, *dbeta;
    float eps;
    int kind, cout, cin;
};
struct FoldBwdTable {
    FoldBwdEntry e[FOLD_MAX];
    int end[FOLD_MAX];            // exclusive prefix sums of cout
    int count;
};

__global__ __launch_bounds__(256) void fold_bn_conv_bwd_kernel(const FoldBwdTable T) {
    __shared__ float red[4];
    int k = 0;
    while (k < T.count - 1 && (int)blockIdx.x >= T.end[k]) ++k;
    const FoldBwdEntry& E = T.e[k];
    const int c = (int)blockIdx.x - (k ? T.end[k - 1] : 0), t = threadIdx.x;
    // weight layout [Cin][Cout] (the transposed convs) or [Cout][Cin]; dwf with 16 taps per pair (the k4 weight gradients: 3 x 3 of 4 x 4 read) or 9
    const bool convt = E.kind != CVAE_FOLD_CONV_K3S1 && E.kind != CVAE_FOLD_CONV_K3S2, k4 = E.kind == CVAE_FOLD_CONVT_K3S2 || E.kind == CVAE_FOLD_CONV_K3S2;
    const float rstd = E.gamma ? rsqrtf(E.var[c] + E.eps) : 1.f, s = E.gamma ? E.gamma[c] * rstd : 1.f;
    float part = 0.f;
    for (int i = t; i < E.cin * 9; i += 256) {
        const int ci = i / 9, tap = i - ci * 9;
        const size_t pair = convt ? (size_t)ci * E.cout + c : (size_t)c * E.cin + ci;
        const float gv = E.dwf[k4 ? pair * 16 + (tap / 3) * 4 + tap % 3 : pair * 9 + tap];
        E.dw[pair * 9 + tap] = s * gv;
        part = fmaf(gv, E.w[pair * 9 + tap], part);
    }
    part = wave_sum(part);
    if ((t & 63) == 0) red[t >> 6] = part;
    __syncthreads();
    if (t == 0) {
        const float tot = ((red[0] + red[1]) + red[2]) + red[3], b = E.bias ? E.bias[c] : 0.f, gb = E.dbf[c];
        if (E.db) E.db[c] = s * gb;
        if (E.gamma) {
            E.dgamma[c] = rstd * (tot + gb * (b - E.mean[c]));
            E.dbeta[c] = gb;
        }
    }
}

// ------------------------------------------------------------------------------------------------ stack mean / std
// One thread per group of 4 elements: the K <= 16 inputs' loads issued together (K a template argument), mean = (x_0 + .. + x_{K-1}) / K, then
// std = sqrt(sum_k (x_k - mean)^2 / (K - 1)) — the two-pass form; K = 1 gives 0 / 0 = NaN, as torch.std does.
struct StackPtrs { const float* x[FOLD_MAX]; };

template <int K>
__global__ __launch_bounds__(256) void stack_mean_std_kernel(const StackPtrs P, float* __restrict__ mean, float* __restrict__ stdv, int64_t n, int vec) {
    const int64_t g = blockIdx.x * (int64_t)256 + threadIdx.x, e0 = g * 4;
    if (e0 >= n) return;
    float v[K][4];
    const bool full = vec && e0 + 4 <= n;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (full) {
            const float4 q = ((const float4*)P.x[k])[g];
            v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[k][e] = e0 + e < n ? P.x[k][e0 + e] : 0.f;
        }
    }
    float mu[4], sd[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) s += v[k][e];
        mu[e] = s / (float)K;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { const float d = v[k][e] - mu[e]; q += d * d; }
        sd[e] = sqrtf(q / (float)(K - 1));
    }
    if (full) {
        ((float4*)mean)[g] = make_float4(mu[0], mu[1], mu[2], mu[3]);
        ((float4*)stdv)[g] = make_float4(sd[0], sd[1], sd[2], sd[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e0 + e < n) { mean[e0 + e] = mu[e]; stdv[e0 + e] = sd[e]; }
    }
}
template <int K>
void stack_launch(int count, const StackPtrs& P, float* mean, float* stdv, int64_t n, int vec, unsigned blocks, hipStream_t st) {
    if constexpr (K > 1) {
        if (count < K) return stack_launch<K - 1>(count, P, mean, stdv, n, vec, blocks, st);
    }
    hipLaunchKernelGGL(stack_mean_std_kernel<K>, dim3(blocks), dim3(256), 0, st, P, mean, stdv, n, vec);
}


template <typename T>
int row_diff_t(const T* a, const T* b, const int64_t* ref, float* l2, float* mean_abs, int64_t rows, int64_t b_rows, int64_t n, float* ws, hipStream_t st) {
    const int64_t chunks = (n + RowDiffGeom<T>::CHUNK - 1) / RowDiffGeom<T>::CHUNK;
    const int vec = (n % RowDiffGeom<T>::E == 0) && aligned16(a) && aligned16(b);
    const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
    hipLaunchKernelGGL(row_diff_partial_kernel<T>, dim3((unsigned)chunks, gy), dim3(256), 0, st, a, b, ref, ws, rows, b_rows, n, chunks, vec);
    hipLaunchKernelGGL(row_diff_finish_kernel, dim3((unsigned)rows), dim3(64), 0, st, (const float*)ws, l2, mean_abs, rows, chunks, 1.f / (float)n);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

int64_t row_diff_chunks(int64_t n, int dtype) {
    return dtype == CVAE_BF16 ? (n + RowDiffGeom<bf16>::CHUNK - 1) / RowDiffGeom<bf16>::CHUNK : (n + RowDiffGeom<float>::CHUNK - 1) / RowDiffGeom<float>::CHUNK;
}

}  // namespace

extern "C" int cvae_fold_bn_conv(int count, const float* const* w, const int* kind, const int64_t* dims, const float* const* bias, const float* const* gamma,
                                 const float* const* beta, const float* const* mean, const float* const* var, const float* eps, float* const* w_out,
                                 float* const* b_out, void* stream) {
    if (count <= 0) return CVAE_E_BADSHAPE;
    if (count > FOLD_MAX) return CVAE_E_UNSUPPORTED;
    if (!w || !kind || !dims || !w_out || !b_out || !eps) return CVAE_E_NULLPTR;
    FoldTable T{};
    T.count = count;
    int64_t blocks = 0;
    for (int k = 0; k < count; ++k) {
        FoldEntry& E = T.e[k];
        const int64_t Cout = dims[2 * k], Cin = dims[2 * k + 1];
        if (Cout <= 0 || Cin <= 0 || Cout * Cin > ((int64_t)1 << 28)) return CVAE_E_BADSHAPE;
        if (kind[k] != CVAE_FOLD_CONV_K4 && kind[k] != CVAE_FOLD_UPCONV_K3 && kind[k] != CVAE_FOLD_CONV_K3S2 && kind[k] != CVAE_FOLD_CONVT_K3S2 &&
            kind[k] != CVAE_FOLD_CONV_K3S1 && kind[k] != CVAE_FOLD_CONVT_K3S2_SUBPIXEL && kind[k] != CVAE_FOLD_CONV_K3S1_GRAD &&
            kind[k] != CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD)
            return CVAE_E_UNSUPPORTED;
        const bool k3_form = kind[k] == CVAE_FOLD_CONV_K3S1 || kind[k] == CVAE_FOLD_CONV_K3S1_GRAD;
        const bool grad_form = kind[k] == CVAE_FOLD_CONV_K3S1_GRAD || kind[k] == CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD;
        const bool gemm_form = k3_form || kind[k] == CVAE_FOLD_CONVT_K3S2_SUBPIXEL || grad_form;
        if (gemm_form && (Cin & 3)) return CVAE_E_UNSUPPORTED;
        if (grad_form && (k3_form ? (Cout & 3) != 0 : (Cout != 16 || Cin > 32))) return CVAE_E_UNSUPPORTED;
        if (!w[k] || !w_out[k] || !b_out[k]) return CVAE_E_NULLPTR;
        const bool bn = gamma && gamma[k];
        if (bn && (!beta || !beta[k] || !mean || !mean[k] || !var || !var[k])) return CVAE_E_NULLPTR;
        if (!aligned16(w_out[k]) || (kind[k] == CVAE_FOLD_CONV_K4 && !aligned16(w[k])) || (kind[k] == CVAE_FOLD_UPCONV_K3 && (Cin & 3) == 0 && !aligned16(w[k])))
            return CVAE_E_UNSUPPORTED;
        E.w = w[k]; E.w_out = w_out[k]; E.b_out = b_out[k];
        E.bias = bias ? bias[k] : nullptr;
        E.gamma = bn ? gamma[k] : nullptr;
        E.beta = bn ? beta[k] : nullptr;
        E.mean = bn ? mean[k] : nullptr;
        E.var = bn ? var[k] : nullptr;
        E.eps = eps[k];
        E.kind = kind[k];
        E.cout = (int)Cout; E.cin = (int)Cin;
        const int64_t gemm_kt = ((k3_form ? 9 : 4) * Cin + 63) / 64 * 64;
        const int64_t grad4 = !grad_form ? 0 : (k3_form ? Cin * ((9 * Cout + 63) / 64 * 64 / 4) : 32 * 64);        // float4 groups of the appended backward matrix
        E.wblocks = gemm_form ? (int)(((k3_form ? 1 : 4) * Cout * (gemm_kt / 4) + grad4 + FOLD_K4_PER_BLOCK - 1) / FOLD_K4_PER_BLOCK)
                  : kind[k] != CVAE_FOLD_UPCONV_K3 ? (int)((Cout * Cin * 4 + FOLD_K4_PER_BLOCK - 1) / FOLD_K4_PER_BLOCK)
                                                 : (int)(((Cout + FOLD_K3_TILE - 1) / FOLD_K3_TILE) * ((Cin + FOLD_K3_TILE - 1) / FOLD_K3_TILE));
        E.bblocks = (int)((Cout + 255) / 256);
        blocks += E.wblocks + E.bblocks;
        if (blocks > ((int64_t)1 << 30)) return CVAE_E_BADSHAPE;
        T.end[k] = (int)blocks;
    }
    hipLaunchKernelGGL(fold_bn_conv_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" int cvae_fold_bn_conv_bwd(int count, const float* const* w, const int* kind, const int64_t* dims, const float* const* bias, const float* const* gamma,
                                     const float* const* mean, const float* const* var, const float* eps, const float* const* dwf, const float* const* dbf,
                                     float* const* dw, float* const* db, float* const* dgamma, float* const* dbeta, void* stream) {
    if (count <= 0) return CVAE_E_BADSHAPE;
    if (count > FOLD_MAX) return CVAE_E_UNSUPPORTED;
    if (!w || !kind || !dims || !dwf || !dbf || !dw || !eps) return CVAE_E_NULLPTR;
    FoldBwdTable T{};
    T.count = count;
    int64_t blocks = 0;
    for (int k = 0; k < count; ++k) {
        FoldBwdEntry& E = T.e[k];
        const int64_t Cout = dims[2 * k], Cin = dims[2 * k + 1];
        if (Cout <= 0 || Cin <= 0 || Cout * Cin > ((int64_t)1 << 24)) return CVAE_E_BADSHAPE;
        if (kind[k] != CVAE_FOLD_CONVT_K3S2 && kind[k] != CVAE_FOLD_CONV_K3S1 && kind[k] != CVAE_FOLD_CONVT_K3S2_SUBPIXEL && kind[k] != CVAE_FOLD_CONV_K3S2)
            return CVAE_E_UNSUPPORTED;
        if (!w[k] || !dwf[k] || !dbf[k] || !dw[k]) return CVAE_E_NULLPTR;
        const bool bn = gamma && gamma[k];
        if (bn && (!mean || !mean[k] || !var || !var[k] || !dgamma || !dgamma[k] || !dbeta || !dbeta[k])) return CVAE_E_NULLPTR;
        E.w = w[k]; E.dwf = dwf[k]; E.dbf = dbf[k]; E.dw = dw[k];
        E.bias = bias ? bias[k] : nullptr;
        E.db = db ? db[k] : nullptr;
        E.gamma = bn ? gamma[k] : nullptr;
        E.mean = bn ? mean[k] : nullptr;
        E.var = bn ? var[k] : nullptr;
        E.dgamma = bn ? dgamma[k] : nullptr;
        E.dbeta = bn ? dbeta[k] : nullptr;
        E.eps = eps[k];
        E.kind = kind[k];
        E.cout = (int)Cout; E.cin = (int)Cin;
        blocks += Cout;
        T.end[k] = (int)blocks;
    }
    hipLaunchKernelGGL(fold_bn_conv_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

extern "C" size_t cvae_row_diff_norms_workspace_bytes(int64_t rows, int64_t n, int dtype) {
    if (rows <= 0 || n <= 0 || !dtype_ok(dtype)) return 0;
    return (size_t)rows * row_diff_chunks(n, dtype) * 2 * sizeof(float);
}
extern "C" int cvae_row_diff_norms(const void* a, const void* b, const int64_t* ref, float* l2, float* mean_abs, int64_t rows, int64_t b_rows, int64_t n,
                                   int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows <= 0 || b_rows <= 0 || n <= 0 || (!ref && b_rows < rows)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (row_diff_chunks(n, dtype) > 0x7fffffff) return CVAE_E_BADSHAPE;
    if (!a || !b || !l2 || !workspace) return CVAE_E_NULLPTR;
    if (workspace_bytes < cvae_row_diff_norms_workspace_bytes(rows, n, dtype)) return CVAE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        return row_diff_t((const T*)a, (const T*)b, ref, l2, mean_abs, rows, b_rows, n, (float*)workspace, st);
    });
}

extern "C" int cvae_stack_mean_std(const float* const* x, int count, float* mean, float* stdv, int64_t n, void* stream) {
    if (count <= 0 || n <= 0) return CVAE_E_BADSHAPE;
    if (count > FOLD_MAX) return CVAE_E_UNSUPPORTED;
    if (!x || !mean || !stdv) return CVAE_E_NULLPTR;
    StackPtrs P{};
    int vec = aligned16(mean) && aligned16(stdv);
    for (int k = 0; k < count; ++k) {
        if (!x[k]) return CVAE_E_NULLPTR;
        P.x[k] = x[k];
        vec = vec && aligned16(x[k]);
    }
    const int64_t groups = (n + 3) / 4;
    if ((groups + 255) / 256 > 0x7fffffff) return CVAE_E_BADSHAPE;
    stack_launch<FOLD_MAX>(count, P, mean, stdv, n, vec, (unsigned)((groups + 255) / 256), (hipStream_t)stream);     // one instance per K: v[K][4] stays in registers
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
