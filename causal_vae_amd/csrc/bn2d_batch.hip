// bn2d_batch.hip — batch-statistics BatchNorm2d (+ the activation behind it) on a channels-last tensor [P = B H W][C]: the forward for the ViT-VAE stem's
// training walk; its residual form and the backward for the decoder's (section 24, below).  The tensor is read TWICE (cvae_bn2d_fwd(training=1) in vessel2d.hip reads it three times in five launches):
//   moments  each workgroup reads ONE contiguous chunk of rows once and leaves (mean, M2) of the chunk per channel, from SHIFTED sums
//            s1 = sum (y - K), s2 = sum (y - K)^2 with K = the chunk's first row: mean = K + s1 / n, M2 = s2 - s1^2 / n.  K lies inside the data, so the
//            subtraction in M2 cancels a few times the chunk's variance at most, never the square of its mean (E[y^2] - E[y]^2 would).
//   finish   merges the chunks IN INDEX ORDER with the pairwise update (Chan et al.): n = na + nb, d = mb - ma, mean = ma + d nb / n,
//            M2 = M2a + M2b + d^2 na nb / n; writes mean, rstd = 1 / sqrt(M2 / P + eps) and, when given, the running statistics (unbiased variance).
//   apply    a = act((y - mean) rstd gamma + beta): one read of y, one write of a.
// No float atomics and no "last workgroup": the chunking depends on P alone (never on the device), every sum has one fixed order, so the bits are the same
// from run to run and from device to device.  The stem's backward is cvae_bn2d_bwd (vessel2d.hip) on (x = y, dy, y = a, gamma, mean, rstd).
//
// For the ViT-VAE decoder's training walk:
//   cvae_bn2d_batch_fwd_res   the same moments and finish launches, and an apply instance a = resid + ((y - mean) rstd gamma + beta) for the BatchNorm that ends
//                             a ResBlock: y and resid read once, the sum formed in fp32 and rounded once.
//   cvae_bn2d_batch_bwd       (y, dy, a, gamma, mean, rstd) -> (dx, dgamma, dbeta) in three launches on the forward's chunking and thread layout.  With
//                             g = dy act'(a) (act' read off the activation's OUTPUT) and xh = (y - mean) rstd:
//     sums     one workgroup per chunk reads the chunk once and leaves (sum g, sum g xh) per channel: row-group sums added through LDS in group order;
//     finish   adds the partials in an order set by the chunk count alone (BNB_SEGS runs per channel, then the runs in order) -> dbeta, dgamma;
//     apply    dx = gamma rstd (g - dbeta / P - xh dgamma / P): y, dy and a read once, dx written once, a row group's constants in registers.
#include "common.h"

namespace {

constexpr int BNB_ROWS = 256;          // a chunk is a multiple of this many rows ..
constexpr int BNB_MAX_PARTS = 1024;    // .. the smallest that leaves at most this many chunks
constexpr int BNB_SEGS = 16;           // finish: a channel's chunks are merged in BNB_SEGS consecutive runs (one thread each), then the runs in order

int64_t bnb_chunk(int64_t P) {
    const int64_t unit = (int64_t)BNB_ROWS * BNB_MAX_PARTS;
    return BNB_ROWS * ((P + unit - 1) / unit);
}
int64_t bnb_parts(int64_t P) {
    const int64_t chunk = bnb_chunk(P);
    return (P + chunk - 1) / chunk;
}

// The thread layout of every kernel that walks rows.  A lane owns 8 consecutive channels c0 .. c0 + 7 (16 bytes of bf16, 32 of fp32); the 256 threads are
// R = 256 / (C / 8) row groups of C / 8 lanes (threads past R groups idle: C / 8 need not divide 256); thread t is lane cl of row group rg.
struct BnbLayout { int lanes, R, cl, rg, c0; };
__device__ __forceinline__ BnbLayout bnb_layout(int C) {
    const int lanes = C >> 3, R = 256 / lanes, t = threadIdx.x;
    const int cl = t % lanes, rg = t / lanes, c0 = cl * 8;
    return {lanes, R, cl, rg, c0};
}

// Two sums per channel over a workgroup's rows: each thread leaves its 8 channels' pair in LDS, then thread c < C adds its channel's R row-group sums in
// group order and hands them to write(c, sum1, sum2).  BNB_INLINE: the callable is inlined with the helper, as if its text stood in the kernel.
#define BNB_INLINE __attribute__((always_inline))
template <typename Write>
__device__ __forceinline__ void bnb_group_sums(float (&red)[2][256][8 + 1], const float (&s1)[8], const float (&s2)[8], const BnbLayout& L, int C, Write write) {
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][t][e] = s1[e]; red[1][t][e] = s2[e]; }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        const int l = c >> 3, e = c & 7;
        float a1 = 0.f, a2 = 0.f;
        for (int q = 0; q < L.R; ++q) { a1 += red[0][q * L.lanes + l][e]; a2 += red[1][q * L.lanes + l][e]; }
        write(c, a1, a2);
    }
}

// Row group rg reads rows p0 + rg, p0 + rg + R, ... of the chunk, four rows in flight.  `part` row 2 g = the chunk's mean, row 2 g + 1 = its M2; its count
// follows from g (bnb_chunk).
template <typename T>
__global__ __launch_bounds__(256) void bn2d_batch_moments_kernel(const T* __restrict__ y, float* __restrict__ part, int64_t P, int C, int64_t chunk) {
    __shared__ float red[2][256][8 + 1];
    const BnbLayout L = bnb_layout(C);
    const int R = L.R, rg = L.rg, c0 = L.c0;
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = (p0 + chunk < P) ? p0 + chunk : P;
    float K[8], s1[8], s2[8];
    load_f32<8>(y + p0 * C + c0, K);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    if (rg < R) {
        int64_t p = p0 + rg;
        for (; p + 3 * (int64_t)R < p1; p += 4 * (int64_t)R) {
            float v[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) load_f32<8>(y + (p + (int64_t)u * R) * C + c0, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = v[u][e] - K[e]; s1[e] += d; s2[e] += d * d; }
        }
        for (; p < p1; p += R) {
            float v[8];
            load_f32<8>(y + p * C + c0, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[e] - K[e]; s1[e] += d; s2[e] += d * d; }
        }
    }
    const float n = (float)(p1 - p0);
    bnb_group_sums(red, s1, s2, L, C, [&](int c, float a1, float a2) BNB_INLINE {          // the row groups share the shift K, so their sums add as they are
        const float m1 = a1 / n;
        part[((size_t)blockIdx.x * 2) * C + c] = to_f32(y[p0 * C + c]) + m1;
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = fmaxf(a2 - a1 * m1, 0.f);
    });
}

// (na, ma, M2a) <- (na, ma, M2a) merged with (nb, mb, M2b); an empty side leaves the other as it is
__device__ __forceinline__ void bnb_merge(float& na, float& ma, float& M2a, float nb, float mb, float M2b) {
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; M2a = M2b; return; }
    const float n = na + nb, d = mb - ma, f = nb / n;
    ma += d * f;
    M2a += M2b + d * d * (na * f);
    na = n;
}
// A block serves 16 channels: thread (s, cc) merges run s of channel cc's chunks (ceil(G / BNB_SEGS) consecutive ones) in index order, then thread (0, cc)
// merges the BNB_SEGS runs in order.  The order is a function of G alone.
struct BnbRun { int cc, s, c, g0, g1; };        // thread (s, cc) of a finish kernel: its channel c and its run [g0, g1) of the G chunks
__device__ __forceinline__ BnbRun bnb_run(int G) {
    const int cc = threadIdx.x & 15, s = threadIdx.x >> 4, c = blockIdx.x * 16 + cc;
    const int per = (G + BNB_SEGS - 1) / BNB_SEGS, g0 = s * per, g1 = (g0 + per < G) ? g0 + per : G;
    return {cc, s, c, g0, g1};
}
__global__ __launch_bounds__(256) void bn2d_batch_finish_kernel(const float* __restrict__ part, int G, float* __restrict__ mean, float* __restrict__ rstd,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var, int64_t P, int C, int64_t chunk,
                                                                 float eps, float momentum) {
    __shared__ float sn[BNB_SEGS][16], sm[BNB_SEGS][16], sq[BNB_SEGS][16];
    const BnbRun run = bnb_run(G);
    const int cc = run.cc, s = run.s, c = run.c, g0 = run.g0, g1 = run.g1;
    float n = 0.f, m = 0.f, M2 = 0.f;
    if (c < C)
        for (int g = g0; g < g1; ++g) {
            const int64_t r0 = (int64_t)g * chunk, r1 = (r0 + chunk < P) ? r0 + chunk : P;
            bnb_merge(n, m, M2, (float)(r1 - r0), part[((size_t)g * 2) * C + c], part[((size_t)g * 2 + 1) * C + c]);
        }
    sn[s][cc] = n; sm[s][cc] = m; sq[s][cc] = M2;
    __syncthreads();
    if (s != 0 || c >= C) return;
    for (int q = 1; q < BNB_SEGS; ++q) bnb_merge(n, m, M2, sn[q][cc], sm[q][cc], sq[q][cc]);
    const float fP = (float)P, var = M2 / fP;
    mean[c] = m;
    rstd[c] = 1.f / sqrtf(var + eps);
    if (running_mean) {
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * var * (fP / (fP - 1.f));
    }
}

// the moments kernel's thread layout; a row group keeps its 8 channels' (mean, rstd gamma, beta) in registers and walks rows with the grid's stride
template <typename T, int EPI>
__global__ __launch_bounds__(256) void bn2d_batch_apply_kernel(const T* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ a, int64_t P, int C,
                                                                int act) {
    const BnbLayout L = bnb_layout(C);
    const int R = L.R, rg = L.rg, c0 = L.c0;
    if (rg >= R) return;
    float mu[8], k[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[c0 + e]; k[e] = rstd[c0 + e] * gamma[c0 + e]; b[e] = beta[c0 + e]; }
    const int64_t step = (int64_t)gridDim.x * R;
    int64_t p = (int64_t)blockIdx.x * R + rg;
    for (; p + 3 * step < P; p += 4 * step) {
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) load_f32<8>(y + (p + u * step) * C + c0, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[u][e] = apply_act_t<EPI>((v[u][e] - mu[e]) * k[e] + b[e], act);
            store_from_f32<8>(a + (p + u * step) * C + c0, v[u]);
        }
    }
    for (; p < P; p += step) {
        float v[8];
        load_f32<8>(y + p * C + c0, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = apply_act_t<EPI>((v[e] - mu[e]) * k[e] + b[e], act);
        store_from_f32<8>(a + p * C + c0, v);
    }
}

// ---- the residual form of the apply pass: a = resid + ((y - mean) rstd gamma + beta), no activation (the BatchNorm that ends a ResBlock) ----
template <typename T>
__global__ __launch_bounds__(256) void bn2d_batch_apply_res_kernel(const T* __restrict__ y, const T* __restrict__ resid, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    T* __restrict__ a, int64_t P, int C) {
    const BnbLayout L = bnb_layout(C);
    const int R = L.R, rg = L.rg, c0 = L.c0;
    if (rg >= R) return;
    float mu[8], k[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[c0 + e]; k[e] = rstd[c0 + e] * gamma[c0 + e]; b[e] = beta[c0 + e]; }
    const int64_t step = (int64_t)gridDim.x * R;
    int64_t p = (int64_t)blockIdx.x * R + rg;
    for (; p + step < P; p += 2 * step) {
        float v[2][8], r[2][8];
#pragma unroll
        for (int u = 0; u < 2; ++u) { load_f32<8>(y + (p + u * step) * C + c0, v[u]); load_f32<8>(resid + (p + u * step) * C + c0, r[u]); }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[u][e] = r[u][e] + ((v[u][e] - mu[e]) * k[e] + b[e]);
            store_from_f32<8>(a + (p + u * step) * C + c0, v[u]);
        }
    }
    for (; p < P; p += step) {
        float v[8], r[8];
        load_f32<8>(y + p * C + c0, v);
        load_f32<8>(resid + p * C + c0, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = r[e] + ((v[e] - mu[e]) * k[e] + b[e]);
        store_from_f32<8>(a + p * C + c0, v);
    }
}

// ---- the backward ----
// sums: the moments kernel's chunks and thread layout.  `part` row 2 g = the chunk's sum of g, row 2 g + 1 = its sum of g xh.  GATED: g = dy act'(a), else g = dy
// and `a` is not read.
template <typename T, bool GATED>
__global__ __launch_bounds__(256) void bn2d_batch_bwd_sums_kernel(const T* __restrict__ y, const T* __restrict__ dy, const T* __restrict__ a,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ part,
                                                                   int64_t P, int C, int64_t chunk, int act) {
    __shared__ float red[2][256][8 + 1];
    const BnbLayout L = bnb_layout(C);
    const int R = L.R, rg = L.rg, c0 = L.c0;
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = (p0 + chunk < P) ? p0 + chunk : P;
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    if (rg < R) {
        float mu[8], rs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { mu[e] = mean[c0 + e]; rs[e] = rstd[c0 + e]; }
        int64_t p = p0 + rg;
        for (; p + (int64_t)R < p1; p += 2 * (int64_t)R) {
            float v[2][8], d[2][8], o[2][8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                load_f32<8>(y + (p + (int64_t)u * R) * C + c0, v[u]);
                load_f32<8>(dy + (p + (int64_t)u * R) * C + c0, d[u]);
                if (GATED) load_f32<8>(a + (p + (int64_t)u * R) * C + c0, o[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float g = GATED ? d[u][e] * act_grad_from_out(o[u][e], act) : d[u][e];
                    s1[e] += g;
                    s2[e] += g * ((v[u][e] - mu[e]) * rs[e]);
                }
        }
        for (; p < p1; p += R) {
            float v[8], d[8], o[8];
            load_f32<8>(y + p * C + c0, v);
            load_f32<8>(dy + p * C + c0, d);
            if (GATED) load_f32<8>(a + p * C + c0, o);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float g = GATED ? d[e] * act_grad_from_out(o[e], act) : d[e];
                s1[e] += g;
                s2[e] += g * ((v[e] - mu[e]) * rs[e]);
            }
        }
    }
    bnb_group_sums(red, s1, s2, L, C, [&](int c, float a1, float a2) BNB_INLINE {
        part[((size_t)blockIdx.x * 2) * C + c] = a1;
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = a2;
    });
}

// finish: the forward finish's runs (thread (s, cc) adds run s of channel cc's partials in index order, thread (0, cc) the BNB_SEGS runs in order), plain sums
__global__ __launch_bounds__(256) void bn2d_batch_bwd_finish_kernel(const float* __restrict__ part, int G, float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                                     int C) {
    __shared__ float sb[BNB_SEGS][16], sg[BNB_SEGS][16];
    const BnbRun run = bnb_run(G);
    const int cc = run.cc, s = run.s, c = run.c, g0 = run.g0, g1 = run.g1;
    float b = 0.f, w = 0.f;
    if (c < C)
        for (int g = g0; g < g1; ++g) { b += part[((size_t)g * 2) * C + c]; w += part[((size_t)g * 2 + 1) * C + c]; }
    sb[s][cc] = b; sg[s][cc] = w;
    __syncthreads();
    if (s != 0 || c >= C) return;
    for (int q = 1; q < BNB_SEGS; ++q) { b += sb[q][cc]; w += sg[q][cc]; }
    dbeta[c] = b;
    dgamma[c] = w;
}

// apply: the forward apply's layout; a row group keeps (mean, rstd, gamma rstd, dbeta / P, dgamma / P) of its 8 channels in registers
template <typename T, bool GATED>
__global__ __launch_bounds__(256) void bn2d_batch_bwd_apply_kernel(const T* __restrict__ y, const T* __restrict__ dy, const T* __restrict__ a,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                    const float* __restrict__ dbeta, const float* __restrict__ dgamma, T* __restrict__ dx, int64_t P,
                                                                    int C, int act) {
    const BnbLayout L = bnb_layout(C);
    const int R = L.R, rg = L.rg, c0 = L.c0;
    if (rg >= R) return;
    float mu[8], rs[8], k[8], mb[8], mg[8];
    const float fP = (float)P;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        mu[e] = mean[c0 + e]; rs[e] = rstd[c0 + e]; k[e] = gamma[c0 + e] * rs[e]; mb[e] = dbeta[c0 + e] / fP; mg[e] = dgamma[c0 + e] / fP;
    }
    const int64_t step = (int64_t)gridDim.x * R;
    int64_t p = (int64_t)blockIdx.x * R + rg;
    for (; p + step < P; p += 2 * step) {
        float v[2][8], d[2][8], o[2][8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            load_f32<8>(y + (p + u * step) * C + c0, v[u]);
            load_f32<8>(dy + (p + u * step) * C + c0, d[u]);
            if (GATED) load_f32<8>(a + (p + u * step) * C + c0, o[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float g = GATED ? d[u][e] * act_grad_from_out(o[u][e], act) : d[u][e];
                v[u][e] = k[e] * ((g - mb[e]) - ((v[u][e] - mu[e]) * rs[e]) * mg[e]);
            }
            store_from_f32<8>(dx + (p + u * step) * C + c0, v[u]);
        }
    }
    for (; p < P; p += step) {
        float v[8], d[8], o[8];
        load_f32<8>(y + p * C + c0, v);
        load_f32<8>(dy + p * C + c0, d);
        if (GATED) load_f32<8>(a + p * C + c0, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float g = GATED ? d[e] * act_grad_from_out(o[e], act) : d[e];
            v[e] = k[e] * ((g - mb[e]) - ((v[e] - mu[e]) * rs[e]) * mg[e]);
        }
        store_from_f32<8>(dx + p * C + c0, v);
    }
}

// The launch geometry of both directions: one workgroup per chunk (moments, sums), one per 16 channels (the finish kernels), and for an apply kernel a grid
// over the passes of R rows, `unroll` passes per workgroup.
struct BnbGeom {
    int64_t chunk, passes;
    int G;
    dim3 chunks, finish;
    BnbGeom(int64_t P, int C) : chunk(bnb_chunk(P)), passes((P + 256 / (C >> 3) - 1) / (256 / (C >> 3))), G((int)bnb_parts(P)), chunks((unsigned)G),
                                finish((unsigned)((C + 15) / 16)) {}
    dim3 apply(int unroll) const { return dim3(cvae_grid_1d(passes, unroll, 2048)); }
};

// the three launches; the entry point has checked everything but the dtype code, which with_dtype refuses before the first launch
// resid (non-null only with act == CVAE_ACT_NONE): the residual instance of the apply pass
int bn2d_batch_launch(const void* y, const void* resid, const float* gamma, const float* beta, void* a, float* mean, float* rstd, float* running_mean,
                      float* running_var, int64_t P, int C, float momentum, float eps, int act, int dtype, float* part, hipStream_t st) {
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        const BnbGeom geo(P, C);
        hipLaunchKernelGGL(bn2d_batch_moments_kernel<T>, geo.chunks, dim3(256), 0, st, (const T*)y, part, P, C, geo.chunk);
        hipLaunchKernelGGL(bn2d_batch_finish_kernel, geo.finish, dim3(256), 0, st, (const float*)part, geo.G, mean, rstd, running_mean, running_var, P, C, geo.chunk,
                           eps, momentum);
        if (resid) {
            hipLaunchKernelGGL(bn2d_batch_apply_res_kernel<T>, geo.apply(2), dim3(256), 0, st, (const T*)y, (const T*)resid, (const float*)mean, (const float*)rstd,
                               gamma, beta, (T*)a, P, C);
            return launch_rc();
        }
        return with_epi(act, [&](auto epi) {
            hipLaunchKernelGGL((bn2d_batch_apply_kernel<T, decltype(epi)::value>), geo.apply(4), dim3(256), 0, st, (const T*)y, (const float*)mean,
                               (const float*)rstd, gamma, beta, (T*)a, P, C, act);
            return launch_rc();
        });
    });
}

// the backward's three launches; as above, with_dtype refuses a dtype code before the first of them
int bn2d_batch_bwd_launch(const void* y, const void* dy, const void* a, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                          float* dbeta, int64_t P, int C, int act, int dtype, float* part, hipStream_t st) {
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        return with_bool(act != CVAE_ACT_NONE, [&](auto gated) {
            constexpr bool GATED = decltype(gated)::value;
            const BnbGeom geo(P, C);
            hipLaunchKernelGGL((bn2d_batch_bwd_sums_kernel<T, GATED>), geo.chunks, dim3(256), 0, st, (const T*)y, (const T*)dy, (const T*)a, mean, rstd, part, P, C,
                               geo.chunk, act);
            hipLaunchKernelGGL(bn2d_batch_bwd_finish_kernel, geo.finish, dim3(256), 0, st, (const float*)part, geo.G, dbeta, dgamma, C);
            hipLaunchKernelGGL((bn2d_batch_bwd_apply_kernel<T, GATED>), geo.apply(2), dim3(256), 0, st, (const T*)y, (const T*)dy, (const T*)a, mean, rstd, gamma,
                               (const float*)dbeta, (const float*)dgamma, (T*)dx, P, C, act);
            return launch_rc();
        });
    });
}

bool bnb_shape_ok(int64_t P, int64_t C) { return P >= 2 && P <= ((int64_t)1 << 40) && C >= 8 && C % 8 == 0 && C <= 2048; }

}  // namespace

extern "C" size_t cvae_bn2d_batch_workspace_bytes(int64_t P, int64_t C) {
    if (!bnb_shape_ok(P, C)) return 0;
    // monotone in P: the chunk count itself drops where the chunk grows (1024 chunks of 256 rows at P = 262144, 513 of 512 one row later)
    const int64_t units = (P + BNB_ROWS - 1) / BNB_ROWS;
    return (size_t)2 * (units < BNB_MAX_PARTS ? units : BNB_MAX_PARTS) * C * sizeof(float);
}
// the forward's checks, shared by the plain and the residual entry (resid == nullptr: the plain one)
static int bn2d_batch_fwd_checked(const void* y, const void* resid, const float* gamma, const float* beta, void* a, float* mean, float* rstd, float* running_mean,
                                  float* running_var, int64_t P, int64_t C, float momentum, float eps, int act, int dtype, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    if (!bnb_shape_ok(P, C)) return CVAE_E_BADSHAPE;
    if (!(momentum >= 0.f && momentum <= 1.f) || !(eps > 0.f)) return CVAE_E_BADSHAPE;       // written so that a NaN is refused too
    if (act < CVAE_ACT_NONE || act > CVAE_ACT_LEAKY001) return CVAE_E_UNSUPPORTED;
    if (resid && act != CVAE_ACT_NONE) return CVAE_E_UNSUPPORTED;       // behind an activation `a` would no longer carry the sign the backward reads
    if (any_null(y, gamma, beta, a, mean, rstd, workspace) || (running_mean == nullptr) != (running_var == nullptr)) return CVAE_E_NULLPTR;
    if (!all_aligned<16>(y, resid, a) || !all_aligned<4>(gamma, beta, mean, rstd, running_mean, running_var, workspace)) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_bn2d_batch_workspace_bytes(P, C)) return CVAE_E_WORKSPACE;
    return bn2d_batch_launch(y, resid, gamma, beta, a, mean, rstd, running_mean, running_var, P, (int)C, momentum, eps, act, dtype, (float*)workspace,
                             (hipStream_t)stream);
}
extern "C" int cvae_bn2d_batch_fwd(const void* y, const float* gamma, const float* beta, void* a, float* mean, float* rstd, float* running_mean,
                                   float* running_var, int64_t P, int64_t C, float momentum, float eps, int act, int dtype, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return bn2d_batch_fwd_checked(y, nullptr, gamma, beta, a, mean, rstd, running_mean, running_var, P, C, momentum, eps, act, dtype, workspace, workspace_bytes,
                                  stream);
}
extern "C" int cvae_bn2d_batch_fwd_res(const void* y, const float* gamma, const float* beta, void* a, float* mean, float* rstd, float* running_mean,
                                       float* running_var, int64_t P, int64_t C, float momentum, float eps, int act, int dtype, void* workspace,
                                       size_t workspace_bytes, void* stream, const void* resid) {
    return bn2d_batch_fwd_checked(y, resid, gamma, beta, a, mean, rstd, running_mean, running_var, P, C, momentum, eps, act, dtype, workspace, workspace_bytes,
                                  stream);
}

extern "C" size_t cvae_bn2d_batch_bwd_workspace_bytes(int64_t P, int64_t C) { return cvae_bn2d_batch_workspace_bytes(P, C); }      // two rows per chunk here too
extern "C" int cvae_bn2d_batch_bwd(const void* y, const void* dy, const void* a, const float* gamma, const float* mean, const float* rstd, void* dx,
                                   float* dgamma, float* dbeta, int64_t P, int64_t C, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!bnb_shape_ok(P, C)) return CVAE_E_BADSHAPE;
    if (act < CVAE_ACT_NONE || act > CVAE_ACT_LEAKY001) return CVAE_E_UNSUPPORTED;
    const bool gated = act != CVAE_ACT_NONE;
    if (any_null(y, dy, gamma, mean, rstd, dx, dgamma, dbeta, workspace) || (gated && !a)) return CVAE_E_NULLPTR;
    if (!all_aligned<16>(y, dy, dx) || (gated && !aligned16(a)) || !all_aligned<4>(gamma, mean, rstd, dgamma, dbeta, workspace)) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_bn2d_batch_bwd_workspace_bytes(P, C)) return CVAE_E_WORKSPACE;
    return bn2d_batch_bwd_launch(y, dy, a, gamma, mean, rstd, dx, dgamma, dbeta, P, (int)C, act, dtype, (float*)workspace, (hipStream_t)stream);
}
