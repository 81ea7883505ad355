// elementwise.hip — HBM-bound kernels of the CausalVAE step: layout/precision plumbing, pooling, (bi|tri)linear
// resize, activation backward, channel sums.  All are streaming kernels: coalesced 64-lane rows, grid-stride,
// grid capped at 8 blocks/CU (cdna_hip_programming.md Guideline 11).
#include "common.h"

// ------------------------------------------------------------------------------------------------- cast
template <typename TS, typename TD>
__global__ void cast_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = from_f32<TD>(to_f32(src[i]));
}

extern "C" int cvae_cast(const void* src, void* dst, int64_t n, int sd, int dd, void* stream) {
    if (n < 0) return CVAE_E_BADSHAPE;
    if (n == 0) return CVAE_OK;
    if (!src || !dst) return CVAE_E_NULLPTR;
    return with_dtype2(sd, dd, [&](auto s, auto d) {
        using TS = decltype(s);
        using TD = decltype(d);
        hipLaunchKernelGGL((cast_kernel<TS, TD>), dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const TS*)src, (TD*)dst, n);
        return launch_rc();
    });
}

// ------------------------------------------------------------------------------- [B,C,S] <-> [B,S,C]
// 64x64 tile through LDS (+1 pad): reads run along S (contiguous in the source), writes along C.
template <typename TS, typename TD, bool TO_NSC>
__global__ void transpose_cs_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int64_t C, int64_t S) {
    __shared__ float tile[64][65];
    const int64_t b = blockIdx.z;
    const int64_t s0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 256 threads: 4 rows per pass
    // a thread's 16 loads are issued together from clamped indices, then stored to LDS (a load under a bounds test: one dependent round trip per row pass)
    if (TO_NSC) {   // src [C][S] -> dst [S][C]
        {
            float v[16];
            const int64_t s = s0 + tx, sc = s < S ? s : S - 1;
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int64_t c = c0 + ty + 4 * u; v[u] = to_f32(src[(b * C + (c < C ? c : C - 1)) * S + sc]); }
#pragma unroll
            for (int u = 0; u < 16; ++u) tile[ty + 4 * u][tx] = (c0 + ty + 4 * u < C && s < S) ? v[u] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 64; r += 4) {
            int64_t s = s0 + r, c = c0 + tx;
            if (s < S && c < C) dst[(b * S + s) * C + c] = from_f32<TD>(tile[tx][r]);
        }
    } else {        // src [S][C] -> dst [C][S]
        {
            float v[16];
            const int64_t c = c0 + tx, cc = c < C ? c : C - 1;
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int64_t sr = s0 + ty + 4 * u; v[u] = to_f32(src[(b * S + (sr < S ? sr : S - 1)) * C + cc]); }
#pragma unroll
            for (int u = 0; u < 16; ++u) tile[ty + 4 * u][tx] = (c < C && s0 + ty + 4 * u < S) ? v[u] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 64; r += 4) {
            int64_t c = c0 + r, s = s0 + tx;
            if (s < S && c < C) dst[(b * C + c) * S + s] = from_f32<TD>(tile[tx][r]);
        }
    }
}

template <bool TO_NSC>
static int transpose_cs(const void* src, void* dst, int64_t B, int64_t C, int64_t S, int sd, int dd, void* stream) {
    if (B < 0 || C <= 0 || S < 0) return CVAE_E_BADSHAPE;
    if (B == 0 || S == 0) return CVAE_OK;
    if (!src || !dst) return CVAE_E_NULLPTR;
    if (C == 1) return cvae_cast(src, dst, B * S, sd, dd, stream);
    if (B > 65535 || (C + 63) / 64 > 65535) return CVAE_E_BADSHAPE;
    return with_dtype2(sd, dd, [&](auto s, auto d) {
        using TS = decltype(s);
        using TD = decltype(d);
        dim3 grid((unsigned)((S + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)B);
        hipLaunchKernelGGL((transpose_cs_kernel<TS, TD, TO_NSC>), grid, dim3(256), 0, (hipStream_t)stream,
                           (const TS*)src, (TD*)dst, C, S);
        return launch_rc();
    });
}
extern "C" int cvae_ncs_to_nsc(const void* src, void* dst, int64_t B, int64_t C, int64_t S, int sd, int dd, void* stream) {
    return transpose_cs<true>(src, dst, B, C, S, sd, dd, stream);
}
extern "C" int cvae_nsc_to_ncs(const void* src, void* dst, int64_t B, int64_t C, int64_t S, int sd, int dd, void* stream) {
    return transpose_cs<false>(src, dst, B, C, S, sd, dd, stream);
}

// ------------------------------------------------------------------------------------- concat panels
// Several panels in ONE launch (torch.cat of 2-3 small matrices was 2-3 launches of < 5 us): gather == 0 writes panel i = src[i] ([B, w_i], row
// stride ss[i]) into dst[:, col0 + sum_{k<i} w_k ..]; gather != 0 copies those column ranges of the wide matrix out into the panels (cat's backward).
#define PANELS_MAX 8
struct PanelTable { float* p[PANELS_MAX]; int64_t w[PANELS_MAX], ss[PANELS_MAX], off[PANELS_MAX + 1]; int n; };
__global__ void copy_panels_kernel(PanelTable tb, float* __restrict__ wide, int64_t B, int64_t ws, int64_t col0, int gather) {
    const int64_t tot = tb.off[tb.n], n = B * tot;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / tot, j = i - b * tot;
        int k = 0;
        while (k + 1 < tb.n && j >= tb.off[k + 1]) ++k;
        float* pp = tb.p[k] + b * tb.ss[k] + (j - tb.off[k]);
        float* wp = wide + b * ws + col0 + j;
        if (gather) *pp = *wp; else *wp = *pp;
    }
}
extern "C" int cvae_copy_panels(float* const* panels, const int64_t* widths, const int64_t* strides, int count, float* wide, int64_t B, int64_t wide_stride,
                                int64_t col0, int gather, void* stream) {
    if (count < 1 || count > PANELS_MAX || B < 0 || col0 < 0) return CVAE_E_BADSHAPE;
    if (!panels || !widths || !strides || !wide) return CVAE_E_NULLPTR;
    PanelTable tb;
    tb.n = count; tb.off[0] = 0;
    for (int i = 0; i < count; ++i) {
        if (widths[i] < 0 || strides[i] < widths[i]) return CVAE_E_BADSHAPE;
        if (!panels[i] && widths[i] > 0 && B > 0) return CVAE_E_NULLPTR;
        tb.p[i] = panels[i]; tb.w[i] = widths[i]; tb.ss[i] = strides[i]; tb.off[i + 1] = tb.off[i] + widths[i];
    }
    if (wide_stride < col0 + tb.off[count]) return CVAE_E_BADSHAPE;
    if (B * tb.off[count] == 0) return CVAE_OK;
    hipLaunchKernelGGL(copy_panels_kernel, dim3(cvae_grid_1d(B * tb.off[count], 256)), dim3(256), 0, (hipStream_t)stream, tb, wide, B, wide_stride, col0, gather);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
__global__ void onehot_panel_kernel(const int64_t* __restrict__ t, float* __restrict__ dst, int64_t B, int64_t nc, int64_t ds, int64_t col0) {
    const int64_t n = B * nc;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t b = i / nc, j = i - b * nc;
        dst[b * ds + col0 + j] = (t[b] == j) ? 1.f : 0.f;
    }
}
extern "C" int cvae_onehot_panel(const int64_t* t, float* dst, int64_t B, int64_t nc, int64_t ds, int64_t col0, void* stream) {
    if (B < 0 || nc <= 0 || col0 < 0 || ds < col0 + nc) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if (!t || !dst) return CVAE_E_NULLPTR;
    hipLaunchKernelGGL(onehot_panel_kernel, dim3(cvae_grid_1d(B * nc, 256)), dim3(256), 0, (hipStream_t)stream, t, dst, B, nc, ds, col0);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

// ------------------------------------------------------------------------------------- activation bwd
template <typename T>
__global__ void act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, int64_t n, int act) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dx[i] = from_f32<T>(to_f32(dy[i]) * act_grad_from_out(to_f32(y[i]), act));
}
extern "C" int cvae_act_bwd(const void* dy, const void* y, void* dx, int64_t n, int act, int dtype, void* stream) {
    if (n < 0) return CVAE_E_BADSHAPE;
    if (n == 0) return CVAE_OK;
    if (!dy || !y || !dx) return CVAE_E_NULLPTR;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(act_bwd_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)y, (T*)dx, n, act);
        return launch_rc();
    });
}

template <typename T>
__global__ void act_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n, int act) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = from_f32<T>(apply_act(to_f32(x[i]), act));
}
extern "C" int cvae_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, void* stream) {
    if (n < 0) return CVAE_E_BADSHAPE;
    if (n == 0) return CVAE_OK;
    if (!x || !y) return CVAE_E_NULLPTR;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(act_fwd_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, n, act);
        return launch_rc();
    });
}

// ------------------------------------------------------------------------------------- channel sum
// x [P, C] channels-last -> out[c] = sum_p x[p, c].  Each thread owns one 16-byte group of channels (8 bf16 / 4 fp32) and
// strides the rows, so every load is a full 16 B per lane and a block row covers whole 128-byte lines; block partials
// meet in LDS.  A single-block-per-chunk launch (small inputs, or no scratch) writes the result directly; larger inputs spread
// rows over blockIdx.x, every block leaves its partial row in the caller's scratch [gx][C] with plain stores and a finish
// launch adds the rows in index order — no memset, no float atomics: the sums are bit-reproducible.
// C == 1 is the plain sum of all elements (rows of VEC "pseudo-channels" folded into one value).
template <typename T>
__global__ __launch_bounds__(256) void channel_sum_vec_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t P, int64_t C, int fold) {
    constexpr int VEC = 16 / sizeof(T);
    __shared__ float red[256 * VEC];
    const int groups = (int)(C / VEC);                      // 16-byte groups per row (C % VEC == 0)
    const int gpb = groups < 256 ? groups : 256;            // groups handled per block row
    const int rows = 256 / gpb;
    const int gi = threadIdx.x % gpb, ri = threadIdx.x / gpb;
    const int64_t grp = (int64_t)blockIdx.y * gpb + gi;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    if (ri < rows && grp < groups) {
        const int64_t stride = (int64_t)gridDim.x * rows;
        int64_t p = (int64_t)blockIdx.x * rows + ri;
        for (; p + 3 * stride < P; p += 4 * stride) {        // 4 independent 16-byte loads in flight per thread
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const uint4*)(x + (p + u * stride) * C + grp * VEC);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T* pv = (const T*)&v[u];
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += to_f32(pv[e]);
            }
        }
        for (; p < P; p += stride) {
            const uint4 v = *(const uint4*)(x + p * C + grp * VEC);
            const T* pv = (const T*)&v;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += to_f32(pv[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[threadIdx.x * VEC + e] = acc[e];
    __syncthreads();
    // tree over the block's rows (all threads take part; rows need not be a power of two)
    int span = 1;
    while (span < rows) span <<= 1;
    for (int sft = span >> 1; sft > 0; sft >>= 1) {
        if (ri < sft && ri + sft < rows) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) red[threadIdx.x * VEC + e] += red[(threadIdx.x + sft * gpb) * VEC + e];
        }
        __syncthreads();
    }
    if (ri == 0 && grp < groups) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = red[threadIdx.x * VEC + e];
        // `out` is the result itself (gridDim.x == 1) or this block's row of the scratch (the host passes row 0's address)
        float* o = out + (size_t)blockIdx.x * (fold ? 1 : C);
        if (fold) {                                         // C == 1 viewed as [P / VEC, VEC]
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) s += acc[e];
            o[0] = s;
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[grp * VEC + e] = acc[e];
        }
    }
}
// scalar fallback (C not a multiple of the vector width)
template <typename T>
__global__ void channel_sum_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t P, int64_t C) {
    __shared__ float red[256];
    const int cl = (C >= 256) ? 256 : (int)C;
    const int rows = 256 / cl;
    const int c_in = threadIdx.x % cl, r_in = threadIdx.x / cl;
    const int64_t c = (int64_t)blockIdx.y * cl + c_in;
    float acc = 0.f;
    if (r_in < rows && c < C) {
        constexpr int U = 8;                                 // loads in flight per thread (clamped row, predicated add: same order of the sum)
        const int64_t stride = (int64_t)gridDim.x * rows;
        for (int64_t p0 = (int64_t)blockIdx.x * rows + r_in; p0 < P; p0 += U * stride) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { const int64_t p = p0 + u * stride; v[u] = to_f32(x[(p < P ? p : P - 1) * C + c]); }
#pragma unroll
            for (int u = 0; u < U; ++u) if (p0 + u * stride < P) acc += v[u];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (r_in == 0 && c < C) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += red[r * cl + c_in];
        out[(size_t)blockIdx.x * C + c] = s;
    }
}
// out[c] = sum_r part[r][c], r in index order
__global__ __launch_bounds__(256) void channel_sum_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int rows, int64_t C) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    constexpr int U = 8;
    for (int r0 = 0; r0 < rows; r0 += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = part[(size_t)min(r0 + u, rows - 1) * C + c];
#pragma unroll
        for (int u = 0; u < U; ++u) if (r0 + u < rows) s += v[u];
    }
    out[c] = s;
}
// Row blocks (gx) a launch over [P][C] would use when scratch is available
template <typename T>
static int64_t channel_sum_gx(const T* x, int64_t P, int64_t C, bool* vec_path, int64_t* Cv_out, int64_t* Pv_out, int* fold_out) {
    constexpr int VEC = 16 / sizeof(T);
    int64_t Pv = P, Cv = C;
    int fold = 0;
    if (C == 1 && P % VEC == 0 && P >= VEC) { Pv = P / VEC; Cv = VEC; fold = 1; }
    const bool vec = Cv % VEC == 0 && (((uintptr_t)x) & 15) == 0;
    if (vec_path) *vec_path = vec;
    if (Cv_out) *Cv_out = Cv;
    if (Pv_out) *Pv_out = Pv;
    if (fold_out) *fold_out = fold;
    if (vec) {
        const int groups = (int)(Cv / VEC), gpb = groups < 256 ? groups : 256, rows = 256 / gpb;
        const int64_t gy = (groups + gpb - 1) / gpb;
        const int64_t passes = (Pv + rows - 1) / rows;       // row passes if one block did everything
        int64_t gx = 1;
        if (passes > 64) { gx = (passes + 31) / 32; const int64_t cap = (1024 + gy - 1) / gy; if (gx > cap) gx = cap; }
        return gx;
    }
    const int cl = (C >= 256) ? 256 : (int)C, rows = 256 / cl;
    const int64_t gy = (C + cl - 1) / cl;
    int64_t gx = (P + (int64_t)rows * 64 - 1) / ((int64_t)rows * 64);
    const int64_t cap = (2048 + gy - 1) / gy;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    return gx;
}
template <typename T>
static int channel_sum_launch(const T* x, float* out, int64_t P, int64_t C, float* ws, size_t ws_bytes, hipStream_t st) {
    constexpr int VEC = 16 / sizeof(T);
    bool vec;
    int64_t Cv, Pv;
    int fold;
    int64_t gx = channel_sum_gx<T>(x, P, C, &vec, &Cv, &Pv, &fold);
    const int64_t row = fold ? 1 : C;                        // floats per partial row
    if (gx > 1 && (!ws || ws_bytes < (size_t)gx * row * sizeof(float))) gx = 1;      // no scratch: one row block (still no atomics)
    float* dst = gx > 1 ? ws : out;
    if (vec) {
        const int groups = (int)(Cv / VEC), gpb = groups < 256 ? groups : 256;
        const int64_t gy = (groups + gpb - 1) / gpb;
        if (gy > 65535) return CVAE_E_BADSHAPE;
        hipLaunchKernelGGL(channel_sum_vec_kernel<T>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, x, dst, Pv, Cv, fold);
    } else {
        const int cl = (C >= 256) ? 256 : (int)C;
        const int64_t gy = (C + cl - 1) / cl;
        if (gy > 65535) return CVAE_E_BADSHAPE;
        hipLaunchKernelGGL(channel_sum_kernel<T>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, x, dst, P, C);
    }
    if (gx > 1) hipLaunchKernelGGL(channel_sum_finish_kernel, dim3((unsigned)((row + 255) / 256)), dim3(256), 0, st, (const float*)ws, out, (int)gx, row);
    return CVAE_OK;
}
extern "C" size_t cvae_channel_sum_workspace_bytes(int64_t P, int64_t C, int dtype) {
    if (P <= 0 || C <= 0) return 0;
    // the 16-byte-aligned geometry (the misaligned fallback never needs more rows than 2048 / gy)
    const int64_t gx_v = dtype == CVAE_BF16 ? channel_sum_gx<bf16>((const bf16*)nullptr, P, C, nullptr, nullptr, nullptr, nullptr)
                                            : channel_sum_gx<float>((const float*)nullptr, P, C, nullptr, nullptr, nullptr, nullptr);
    const int cl = (C >= 256) ? 256 : (int)C, rows = 256 / cl;
    int64_t gx_s = (P + (int64_t)rows * 64 - 1) / ((int64_t)rows * 64);
    const int64_t cap = (2048 + (C + cl - 1) / cl - 1) / ((C + cl - 1) / cl);
    if (gx_s > cap) gx_s = cap;
    const int64_t gx = gx_v > gx_s ? gx_v : gx_s;
    return gx > 1 ? (size_t)gx * C * sizeof(float) : 0;
}
extern "C" int cvae_channel_sum(const void* x, float* out, int64_t P, int64_t C, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || C <= 0) return CVAE_E_BADSHAPE;
    if (!out) return CVAE_E_NULLPTR;
    if (P == 0) return hipMemsetAsync(out, 0, C * sizeof(float), (hipStream_t)stream) == hipSuccess ? CVAE_OK : CVAE_E_LAUNCH;
    if (!x) return CVAE_E_NULLPTR;
    const int rc = with_dtype(dtype, [&](auto tv) {
        return channel_sum_launch((const decltype(tv)*)x, out, P, C, (float*)workspace, workspace_bytes, (hipStream_t)stream);
    });
    if (rc != CVAE_OK) return rc;
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

// ------------------------------------------------------------------------------------- adaptive avg pool
template <typename T>
__global__ void avgpool_fwd_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                                   int64_t OD, int64_t OH, int64_t OW, int64_t out_stride) {
    const int64_t OV = OD * OH * OW, n = B * OV * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i % C, o = (i / C) % OV, b = i / (C * OV);
        const int64_t ow = o % OW, oh = (o / OW) % OH, od = o / (OW * OH);
        const int64_t d0 = pool_lo(od, D, OD), d1 = pool_hi(od, D, OD);
        const int64_t h0 = pool_lo(oh, H, OH), h1 = pool_hi(oh, H, OH);
        const int64_t w0 = pool_lo(ow, W, OW), w1 = pool_hi(ow, W, OW);
        float acc = 0.f;
        for (int64_t d = d0; d < d1; ++d)
            for (int64_t h = h0; h < h1; ++h)
                for (int64_t w = w0; w < w1; ++w) acc += to_f32(x[(((b * D + d) * H + h) * W + w) * C + c]);
        out[b * out_stride + c * OV + o] = acc / (float)((d1 - d0) * (h1 - h0) * (w1 - w0));
    }
}
// Bare Flatten (1-voxel windows): out[b][c * V + p] = x[b][p][c] — a [V x C] -> [C x V] transpose per sample, through a 64 x 64 LDS tile so that both
// sides move whole rows (the generic kernel above writes one float per thread at a stride of V floats: 35 us for MNIST's 1024 x 49 x 64).
template <typename T>
__global__ __launch_bounds__(256) void flatten_fwd_kernel(const T* __restrict__ x, float* __restrict__ out, int V, int C, int64_t out_stride) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const T* xb = x + (size_t)b * V * C;
    {   // all 16 loads of a thread first, from clamped indices (a load under a bounds test is a dependent round trip per iteration), then the LDS stores
        float v[16];
        const int c = c0 + tx, cc = min(c, C - 1);
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = to_f32(xb[(size_t)min(p0 + ty + 4 * u, V - 1) * C + cc]);
#pragma unroll
        for (int u = 0; u < 16; ++u) tile[ty + 4 * u][tx] = (p0 + ty + 4 * u < V && c < C) ? v[u] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, p = p0 + tx;
        if (c < C && p < V) out[(size_t)b * out_stride + (size_t)c * V + p] = tile[tx][r];
    }
}
// and its backward: dx[b][p][c] = dout[b][c * V + p], zeroed where the (ReLU output) x is not positive
template <typename T>
__global__ __launch_bounds__(256) void flatten_bwd_kernel(const float* __restrict__ dout, const T* __restrict__ mask, T* __restrict__ dx, int V, int C, int64_t dstride) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float mk[16];
    {   // the 16 gradient loads and the 16 mask loads of a thread are issued together, from clamped indices (see flatten_fwd_kernel)
        float v[16];
        const int p = p0 + tx, pc = min(p, V - 1), cm = min(c0 + tx, C - 1);
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = dout[(size_t)b * dstride + (size_t)min(c0 + ty + 4 * u, C - 1) * V + pc];
#pragma unroll
        for (int u = 0; u < 16; ++u) mk[u] = mask ? to_f32(mask[((size_t)b * V + min(p0 + ty + 4 * u, V - 1)) * C + cm]) : 1.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) tile[ty + 4 * u][tx] = (c0 + ty + 4 * u < C && p < V) ? v[u] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int r = ty + 4 * u, p = p0 + r, c = c0 + tx;
        if (p < V && c < C) {
            const size_t i = ((size_t)b * V + p) * C + c;
            const float g = tile[tx][r];
            dx[i] = from_f32<T>(mk[u] > 0.f ? g : 0.f);
        }
    }
}
extern "C" int cvae_adaptive_avgpool_fwd(const void* x, float* out, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                                         int64_t OD, int64_t OH, int64_t OW, int64_t out_stride, int dtype, void* stream) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || OD <= 0 || OH <= 0 || OW <= 0 || out_stride < C * OD * OH * OW) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if (!x || !out) return CVAE_E_NULLPTR;
    if (OD == D && OH == H && OW == W && D * H * W < ((int64_t)1 << 22) && C < ((int64_t)1 << 22) && B <= 65535 && dtype != CVAE_FP8) {   // bare Flatten
        const int V = (int)(D * H * W);
        const dim3 grid((unsigned)((V + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)B);
        return with_dtype(dtype, [&](auto tv) {
            using T = decltype(tv);
            hipLaunchKernelGGL(flatten_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, out, V, (int)C, out_stride);
            return launch_rc();
        });
    }
    const int64_t n = B * OD * OH * OW * C;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(avgpool_fwd_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, out, B, D, H, W, C, OD, OH, OW, out_stride);
        return launch_rc();
    });
}

template <typename T>
__global__ void avgpool_bwd_kernel(const float* __restrict__ dout, const T* __restrict__ mask, T* __restrict__ dx, int64_t B, int64_t D, int64_t H,
                                   int64_t W, int64_t C, int64_t OD, int64_t OH, int64_t OW, int64_t dstride) {
    const int64_t V = D * H * W, OV = OD * OH * OW, n = B * V * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i % C, p = (i / C) % V, b = i / (C * V);
        const int64_t w = p % W, h = (p / W) % H, d = p / (W * H);
        float acc = 0.f;
        if (!mask || to_f32(mask[i]) > 0.f) {
            // the windows that contain index i of an axis are exactly o = floor(i O / I) .. ceil((i + 1) O / I) - 1 (window o is [floor(o I / O), ceil((o + 1) I / O)):
            // i >= lo(o) <=> o <= floor(((i + 1) O - 1) / I), i < hi(o) <=> o >= floor(i O / I)), for any I and O: no membership test, ascending order as before
            for (int64_t od = (d * OD) / D; od <= ((d + 1) * OD - 1) / D; ++od) {
                const int64_t d0 = pool_lo(od, D, OD), d1 = pool_hi(od, D, OD);
                for (int64_t oh = (h * OH) / H; oh <= ((h + 1) * OH - 1) / H; ++oh) {
                    const int64_t h0 = pool_lo(oh, H, OH), h1 = pool_hi(oh, H, OH);
                    for (int64_t ow = (w * OW) / W; ow <= ((w + 1) * OW - 1) / W; ++ow) {
                        const int64_t w0 = pool_lo(ow, W, OW), w1 = pool_hi(ow, W, OW);
                        acc += dout[b * dstride + c * OV + (od * OH + oh) * OW + ow] / (float)((d1 - d0) * (h1 - h0) * (w1 - w0));
                    }
                }
            }
        }
        dx[i] = from_f32<T>(acc);
    }
}
extern "C" int cvae_adaptive_avgpool_bwd(const float* dout, const void* mask, void* dx, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                                         int64_t OD, int64_t OH, int64_t OW, int64_t dstride, int dtype, void* stream) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || OD <= 0 || OH <= 0 || OW <= 0 || dstride < C * OD * OH * OW) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if (!dout || !dx) return CVAE_E_NULLPTR;
    if (OD == D && OH == H && OW == W && D * H * W < ((int64_t)1 << 22) && C < ((int64_t)1 << 22) && B <= 65535 && dtype != CVAE_FP8) {   // bare Flatten
        const int V = (int)(D * H * W);
        const dim3 grid((unsigned)((V + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)B);
        return with_dtype(dtype, [&](auto tv) {
            using T = decltype(tv);
            hipLaunchKernelGGL(flatten_bwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, dout, (const T*)mask, (T*)dx, V, (int)C, dstride);
            return launch_rc();
        });
    }
    const int64_t n = B * D * H * W * C;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, dout, (const T*)mask, (T*)dx, B, D, H, W, C, OD, OH, OW, dstride);
        return launch_rc();
    });
}

// ------------------------------------------------------------------------------------- linear resize
// torch upsample_{bi,tri}linear, align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0, scale = in/out (float).
template <typename T>
__global__ void upsample_fwd_kernel(const T* __restrict__ src, float* __restrict__ dst, int64_t B, int64_t d, int64_t h, int64_t w,
                                    int64_t D, int64_t H, int64_t W, int64_t C) {
    const float sd = (float)d / (float)D, sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int64_t n = B * D * H * W * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i % C;
        int64_t r = i / C;
        const int64_t ow = r % W; r /= W;
        const int64_t oh = r % H; r /= H;
        const int64_t od = r % D;
        const int64_t b = r / D;
        const LinTap<int64_t> td = lin_tap(od, d, sd), th = lin_tap(oh, h, sh), tw = lin_tap(ow, w, sw);
        auto at = [&](int64_t z, int64_t y, int64_t x) { return to_f32(src[(((b * d + z) * h + y) * w + x) * C + c]); };
        // same association as aten's CPU kernel: depth, then height, then width taps
        float v = td.w0 * (th.w0 * (tw.w0 * at(td.i0, th.i0, tw.i0) + tw.w1 * at(td.i0, th.i0, tw.i1)) +
                           th.w1 * (tw.w0 * at(td.i0, th.i1, tw.i0) + tw.w1 * at(td.i0, th.i1, tw.i1))) +
                  td.w1 * (th.w0 * (tw.w0 * at(td.i1, th.i0, tw.i0) + tw.w1 * at(td.i1, th.i0, tw.i1)) +
                           th.w1 * (tw.w0 * at(td.i1, th.i1, tw.i0) + tw.w1 * at(td.i1, th.i1, tw.i1)));
        dst[i] = v;
    }
}
// ---- exact 2x fast paths (the 64^3 -> 128^3 case of the benchmark): 32-bit index math, 4 outputs per thread along W
// (one 16-byte store), and for the backward a fixed 4-candidate window per dim [2i-1, 2i+2] whose weights come from the
// same lin_tap as the forward (bit-identical coefficients, borders included).
template <typename T>
__global__ void upsample2x_fwd_kernel(const T* __restrict__ src, float* __restrict__ dst, int B, int d, int h, int w, int D, int H, int W) {
    const float sd = (float)d / (float)D, sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int W4 = W >> 2;
    const int n = B * D * H * W4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int r = i;
        const int ow0 = (r % W4) * 4; r /= W4;
        const int oh = r % H; r /= H;
        const int od = r % D;
        const int b = r / D;
        const LinTap<int64_t> td = lin_tap<int64_t>(od, d, sd), th = lin_tap<int64_t>(oh, h, sh);
        const T* p00 = src + ((size_t)(b * d + (int)td.i0) * h + (int)th.i0) * w;
        const T* p01 = src + ((size_t)(b * d + (int)td.i0) * h + (int)th.i1) * w;
        const T* p10 = src + ((size_t)(b * d + (int)td.i1) * h + (int)th.i0) * w;
        const T* p11 = src + ((size_t)(b * d + (int)td.i1) * h + (int)th.i1) * w;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const LinTap<int64_t> tw = lin_tap<int64_t>(ow0 + j, w, sw);
            const int x0 = (int)tw.i0, x1 = (int)tw.i1;
            o[j] = td.w0 * (th.w0 * (tw.w0 * to_f32(p00[x0]) + tw.w1 * to_f32(p00[x1])) + th.w1 * (tw.w0 * to_f32(p01[x0]) + tw.w1 * to_f32(p01[x1]))) +
                   td.w1 * (th.w0 * (tw.w0 * to_f32(p10[x0]) + tw.w1 * to_f32(p10[x1])) + th.w1 * (tw.w0 * to_f32(p11[x0]) + tw.w1 * to_f32(p11[x1])));
        }
        *(float4*)(dst + (((size_t)(b * D + od) * H + oh) * W + ow0)) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

template <typename T>
__global__ void upsample2x_bwd_kernel(const float* __restrict__ ddst, T* __restrict__ dsrc, int B, int d, int h, int w, int D, int H, int W) {
    const float sd = (float)d / (float)D, sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int n = B * d * h * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int r = i;
        const int x = r % w; r /= w;
        const int y = r % h; r /= h;
        const int z = r % d;
        const int b = r / d;
        const Win4 wz = win4<int64_t>(z, d, D, sd, D != d), wy = win4<int64_t>(y, h, H, sh, true), wx = win4<int64_t>(x, w, W, sw, true);
        // the 4 x 4 x 4 gradient values around this voxel are requested first, unconditionally, from clamped indices (a value whose weight is 0 — beyond the
        // volume, or the unstrided depth axis — is loaded and not used): with the loads behind the weight tests every one of them was a dependent round trip
        // (42 us for 33.5 MB at 4 x 128^3)
        float v[4][4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                const float* row = ddst + ((size_t)(b * D + min(max(wz.j0 + a, 0), D - 1)) * H + min(max(wy.j0 + bb, 0), H - 1)) * W;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[a][bb][c] = row[min(max(wx.j0 + c, 0), W - 1)];
            }
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (wz.w[a] == 0.f) continue;
            float pl = 0.f;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                if (wy.w[bb] == 0.f) continue;
                float rs = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) if (wx.w[c] != 0.f) rs += wx.w[c] * v[a][bb][c];
                pl += wy.w[bb] * rs;
            }
            acc += wz.w[a] * pl;
        }
        dsrc[i] = from_f32<T>(acc);
    }
}
static bool is_exact_2x(int64_t B, int64_t d, int64_t h, int64_t w, int64_t D, int64_t H, int64_t W, int64_t C) {
    return C == 1 && (D == 2 * d || (D == 1 && d == 1)) && H == 2 * h && W == 2 * w && (W % 4) == 0 && B * D * H * W < (int64_t)1 << 31;
}

extern "C" int cvae_upsample_linear_fwd(const void* src, float* dst, int64_t B, int64_t d, int64_t h, int64_t w,
                                        int64_t D, int64_t H, int64_t W, int64_t C, int dtype, void* stream) {
    if (B < 0 || d <= 0 || h <= 0 || w <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if (!src || !dst) return CVAE_E_NULLPTR;
    if (is_exact_2x(B, d, h, w, D, H, W, C)) {
        const int64_t n4 = B * D * H * (W / 4);
        return with_dtype(dtype, [&](auto tv) {
            using T = decltype(tv);
            hipLaunchKernelGGL(upsample2x_fwd_kernel<T>, dim3(cvae_grid_1d(n4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)src, dst, (int)B, (int)d, (int)h, (int)w, (int)D, (int)H, (int)W);
            return launch_rc();
        });
    }
    const int64_t n = B * D * H * W * C;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(upsample_fwd_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)src, dst, B, d, h, w, D, H, W, C);
        return launch_rc();
    });
}

// Gather form of the transpose: for source index i, the destination indices whose taps touch i lie in
// [floor((i-0.5)/scale - 0.5), ceil((i+1.5)/scale - 0.5)]; each candidate re-derives its taps with lin_tap, so the
// weights are bit-identical to the forward's.
__device__ __forceinline__ void cand_range(int64_t i, int64_t out, float scale, int64_t& lo, int64_t& hi) {
    const float inv = 1.f / scale;
    float a = ((float)i - 1.0f + 0.5f) * inv - 0.5f, b = ((float)i + 1.0f + 0.5f) * inv - 0.5f;
    lo = (int64_t)floorf(a) - 1;
    hi = (int64_t)ceilf(b) + 1;
    if (lo < 0) lo = 0;
    if (hi > out - 1) hi = out - 1;
}
template <typename T>
__global__ void upsample_bwd_kernel(const float* __restrict__ ddst, T* __restrict__ dsrc, int64_t B, int64_t d, int64_t h, int64_t w,
                                    int64_t D, int64_t H, int64_t W, int64_t C) {
    const float sd = (float)d / (float)D, sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int64_t n = B * d * h * w * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i % C;
        int64_t r = i / C;
        const int64_t x = r % w; r /= w;
        const int64_t y = r % h; r /= h;
        const int64_t z = r % d;
        const int64_t b = r / d;
        int64_t dlo, dhi, hlo, hhi, wlo, whi;
        cand_range(z, D, sd, dlo, dhi);
        cand_range(y, H, sh, hlo, hhi);
        cand_range(x, W, sw, wlo, whi);
        float acc = 0.f;
        for (int64_t od = dlo; od <= dhi; ++od) {
            const LinTap<int64_t> td = lin_tap(od, d, sd);
            const float wd = (td.i0 == z ? td.w0 : 0.f) + (td.i1 == z ? td.w1 : 0.f);
            if (wd == 0.f) continue;
            for (int64_t oh = hlo; oh <= hhi; ++oh) {
                const LinTap<int64_t> th = lin_tap(oh, h, sh);
                const float wh = (th.i0 == y ? th.w0 : 0.f) + (th.i1 == y ? th.w1 : 0.f);
                if (wh == 0.f) continue;
                float row = 0.f;
                for (int64_t ow = wlo; ow <= whi; ++ow) {
                    const LinTap<int64_t> tw = lin_tap(ow, w, sw);
                    const float ww = (tw.i0 == x ? tw.w0 : 0.f) + (tw.i1 == x ? tw.w1 : 0.f);
                    if (ww != 0.f) row += ww * ddst[(((b * D + od) * H + oh) * W + ow) * C + c];
                }
                acc += wd * wh * row;
            }
        }
        dsrc[i] = from_f32<T>(acc);
    }
}
extern "C" int cvae_upsample_linear_bwd(const float* ddst, void* dsrc, int64_t B, int64_t d, int64_t h, int64_t w,
                                        int64_t D, int64_t H, int64_t W, int64_t C, int dtype, void* stream) {
    if (B < 0 || d <= 0 || h <= 0 || w <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return CVAE_E_BADSHAPE;
    if (B == 0) return CVAE_OK;
    if (!ddst || !dsrc) return CVAE_E_NULLPTR;
    if (is_exact_2x(B, d, h, w, D, H, W, C)) {
        const int64_t ns = B * d * h * w;
        return with_dtype(dtype, [&](auto tv) {
            using T = decltype(tv);
            hipLaunchKernelGGL(upsample2x_bwd_kernel<T>, dim3(cvae_grid_1d(ns, 256, 8192)), dim3(256), 0, (hipStream_t)stream, ddst, (T*)dsrc, (int)B, (int)d, (int)h, (int)w, (int)D, (int)H, (int)W);
            return launch_rc();
        });
    }
    const int64_t n = B * d * h * w * C;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(upsample_bwd_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, ddst, (T*)dsrc, B, d, h, w, D, H, W, C);
        return launch_rc();
    });
}
