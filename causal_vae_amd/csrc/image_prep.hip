// image_prep.hip — the vessel image transforms on the device: what the reference does on the host, one image at a time, between a stack
// and a model's input (vessel_analysis/00_core/dataset.py:192-237; latent_translator/utils.py:18-60 + dataset.py:57-70).
//   cvae_mip_max                  [B][D][Hs][Ws] uint16 / fp32 -> fp32 maximum over D.  A pure stream: a thread owns 8 consecutive pixels (16-byte loads), D is
//                                 its inner loop, four planes in flight.
//   cvae_resize_bilinear_aa_f32   torch's antialiased bilinear resize in ONE launch: a workgroup owns an AA_TILE_H x AA_TILE_W output tile, builds the tile's
//                                 two weight tables in fp64 (rounded to fp32 once), filters the source rows [r0, r1) its tile needs along W into LDS, then along
//                                 H from LDS.  The tap loops run to each output's own count, so any ratio works until the row window outgrows LDS (refused).
//   cvae_minmax_binarise          three launches over an image that stays in L2: extremes per chunk; the fp64 sum of v = (y - mn) / (mx - mn) per chunk; then
//                                 every workgroup merges the chunk sums in the same fixed order, thresholds at their mean and writes the 1 or 4 flip variants.
//   cvae_percentile_clip_scale    radix select of four order statistics at once: 4 passes of (per-workgroup LDS digit histograms, integer atomics) + (merge in
//                                 chunk order, pick each rank's digit); ranks whose prefixes still agree share one histogram.  Then numpy's lerp, clip and scale
//                                 in fp64, rounded once.
// No float atomics; a chunk is a fixed number of pixels, so grids and every order of summation depend on the image's shape alone: an image's bits depend on
// nothing but the image (a workgroup combines its threads' values with common.h's LDS tree, block_tree).  The only global atomic is the INTEGER count of ones.  fp contraction is off for the whole file: numpy and torch do not fuse, and
// the host replays the window arithmetic of the resize; the fp32 filter sums ask for their fma by name.
#include <float.h>
#include <math.h>
#include "common.h"
#pragma clang fp contract(off)

CVAE_TUNABLE(AA_TILE_W, 64);             // output tile of the antialiased resize: columns (a power of two, at least 64) ..
CVAE_TUNABLE(AA_TILE_H, 8);              // .. and rows; AA_TILE_W + AA_TILE_H <= 256 threads build the weight tables
CVAE_TUNABLE(PREP_CHUNK, 4096);          // pixels per workgroup of the binarise launches (a multiple of 1024)
CVAE_TUNABLE(SELECT_CHUNK, 16384);       // pixels per workgroup of a radix-select histogram launch (a multiple of 1024)

namespace {

constexpr int NT = 256;
constexpr int TW = (int)AA_TILE_W, TH = (int)AA_TILE_H;
static_assert(TW >= 64 && (TW & (TW - 1)) == 0 && TH >= 1 && TW + TH <= NT, "AA_TILE_W: a power of two >= 64; AA_TILE_W + AA_TILE_H <= 256");
static_assert(PREP_CHUNK % 1024 == 0 && PREP_CHUNK >= 1024 && SELECT_CHUNK % 1024 == 0 && SELECT_CHUNK >= 1024, "PREP_CHUNK, SELECT_CHUNK: multiples of 1024");
constexpr int64_t MAX_PIXELS = 0x7fffffffLL, MAX_BATCH = 65535;

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= FLT_MAX; }

// up to four consecutive floats from element i of an n-element image (VEC: n % 4 == 0 and p 16-byte aligned); returns how many
template <bool VEC> __device__ __forceinline__ int load4(const float* __restrict__ p, int64_t i, int64_t n, float (&v)[4]) {
    if (i >= n) return 0;
    if (VEC) {
        const float4 f = *(const float4*)(p + i);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        return 4;
    }
    const int c = (int)(n - i < 4 ? n - i : 4);
    for (int e = 0; e < c; ++e) v[e] = p[i + e];
    return c;
}

// ------------------------------------------------------------------------------------------------ maximum-intensity projection
__device__ __forceinline__ void mip_load8(const float* p, float (&v)[8]) { load_f32<8>(p, v); }
__device__ __forceinline__ void mip_load8(const uint16_t* p, float (&v)[8]) {
    const uint4 q = *(const uint4*)p;
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = (float)(w[e] & 0xffffu); v[2 * e + 1] = (float)(w[e] >> 16); }
}
// np.max: the larger of the two, and a NaN once seen stays (a NaN v is taken; against a NaN m both tests are false for an ordinary v)
__device__ __forceinline__ float mip_step(float m, float v) { return (v > m || v != v) ? v : m; }

template <typename S, bool VEC> __global__ __launch_bounds__(NT) void mip_max_kernel(const S* __restrict__ src, float* __restrict__ dst, int D, int64_t P) {
    const int64_t b = blockIdx.y, i0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * 8;
    if (i0 >= P) return;
    const S* s = src + b * D * P + i0;
    float* o = dst + b * P + i0;
    float m[8];
    if (VEC) {
        mip_load8(s, m);
#pragma unroll 4
        for (int d = 1; d < D; ++d) {
            float v[8];
            mip_load8(s + (int64_t)d * P, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = mip_step(m[e], v[e]);
        }
        store_from_f32<8>(o, m);
    } else {
        const int n = (int)(P - i0 < 8 ? P - i0 : 8);
        for (int e = 0; e < n; ++e) {
            float mm = (float)s[e];
            for (int d = 1; d < D; ++d) mm = mip_step(mm, (float)s[(int64_t)d * P + e]);
            o[e] = mm;
        }
    }
}

// ------------------------------------------------------------------------------------------------ antialiased bilinear resize
// torch's window of output i of an axis n_in -> n_out (aten UpSampleKernel.cpp, _compute_indices_min_size_weights_aa), in fp64; the host replays it
struct AaAxis { double scale, support, inv; };
inline __host__ __device__ AaAxis aa_axis(int n_in, int n_out) {
    AaAxis a;
    a.scale = (double)n_in / (double)n_out;
    a.support = a.scale > 1.0 ? a.scale : 1.0;
    a.inv = 1.0 / a.support;
    return a;
}
inline __host__ __device__ void aa_window(const AaAxis& a, int i, int n_in, int& lo, int& hi) {
    const double c = a.scale * ((double)i + 0.5);
    lo = (int)(c - a.support + 0.5);
    hi = (int)(c + a.support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
}
__device__ __forceinline__ double aa_weight(const AaAxis& a, int i, int j) {
    const double c = a.scale * ((double)i + 0.5);
    const double w = 1.0 - fabs(((double)j - c + 0.5) * a.inv);
    return w > 0.0 ? w : 0.0;
}
inline size_t aa_lds_bytes(int R, int KW, int KH) { return 4 * ((size_t)R * TW + (size_t)KW * TW + (size_t)KH * TH + 2 * TW + 2 * TH); }

// LDS: tmp [R][TW] (the W-filtered source rows r0 .. of the tile), wW [KW][TW], wH [KH][TH] (tap k of column / row l at [k][l]: consecutive lanes, consecutive
// banks), then each column's / row's first tap and tap count.  R, KW, KH are the largest the shape needs (the host computed them with aa_window); the kernel
// clamps to them all the same, so that no disagreement could become an access outside LDS.
__global__ __launch_bounds__(NT) void resize_aa_kernel(const float* __restrict__ src, float* __restrict__ dst, int Hs, int Ws, int H, int W, int R, int KW, int KH) {
    extern __shared__ float aa_smem[];
    float* tmp = aa_smem;
    float* wW = tmp + (size_t)R * TW;
    float* wH = wW + (size_t)KW * TW;
    int* x0 = (int*)(wH + (size_t)KH * TH);
    int* xn = x0 + TW;
    int* y0 = xn + TW;
    int* yn = y0 + TH;
    const int t = threadIdx.x, ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
    const float* s = src + (size_t)blockIdx.z * Hs * Ws;
    float* d = dst + (size_t)blockIdx.z * H * W;

    if (t < TW + TH) {          // the two weight tables: one thread per column, one per row
        const bool isw = t < TW;
        const int l = isw ? t : t - TW, o = (isw ? ox0 : oy0) + l, n_in = isw ? Ws : Hs, n_out = isw ? W : H, K = isw ? KW : KH, ld = isw ? TW : TH;
        float* wt = isw ? wW : wH;
        int lo = 0, hi = 0;
        if (o < n_out) {
            const AaAxis a = aa_axis(n_in, n_out);
            aa_window(a, o, n_in, lo, hi);
            if (hi - lo > K) hi = lo + K;
            double sum = 0.0;
            for (int j = lo; j < hi; ++j) sum += aa_weight(a, o, j);
            for (int j = lo; j < hi; ++j) wt[(j - lo) * ld + l] = (float)(aa_weight(a, o, j) / sum);
        }
        (isw ? x0 : y0)[l] = lo;
        (isw ? xn : yn)[l] = hi - lo;
    }
    __syncthreads();
    const int th = H - oy0 < TH ? H - oy0 : TH;
    const int r0 = y0[0], r1 = y0[th - 1] + yn[th - 1];          // windows move monotonically with the output index
    const int rows = r1 - r0 < R ? r1 - r0 : R;

    for (int it = t; it < rows * TW; it += NT) {          // W pass: source row r0 + r, output column ox0 + l
        const int r = it / TW, l = it % TW, n = xn[l];
        const float* p = s + (size_t)(r0 + r) * Ws + x0[l];
        float acc = 0.f;
        for (int k = 0; k < n; ++k) acc = fmaf(wW[k * TW + l], p[k], acc);
        tmp[r * TW + l] = acc;
    }
    __syncthreads();
    for (int it = t; it < th * TW; it += NT) {            // H pass
        const int oy = it / TW, l = it % TW;
        if (ox0 + l >= W) continue;
        const int n = yn[oy], rr = y0[oy] - r0;
        float acc = 0.f;
        for (int k = 0; k < n && rr + k < rows; ++k) acc = fmaf(wH[k * TH + oy], tmp[(rr + k) * TW + l], acc);
        d[(size_t)(oy0 + oy) * W + ox0 + l] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ min-max, mean threshold, flips
struct BinWs { double* psum; float* pmn; float* pmx; int* pbad; };
inline int64_t bin_chunks(int64_t n) { return (n + PREP_CHUNK - 1) / PREP_CHUNK; }
inline size_t bin_ws_bytes(int64_t B, int64_t n) { return (size_t)(B * bin_chunks(n)) * (sizeof(double) + 2 * sizeof(float) + sizeof(int)); }
inline BinWs bin_ws(void* ws, int64_t B, int64_t n) {
    const size_t m = (size_t)(B * bin_chunks(n));
    BinWs w;
    w.psum = (double*)ws;
    w.pmn = (float*)(w.psum + m);
    w.pmx = w.pmn + m;
    w.pbad = (int*)(w.pmx + m);
    return w;
}
struct BinRed { double d[NT]; float f[NT]; int i[NT]; };
constexpr int BIN_STEPS = (int)(PREP_CHUNK / (NT * 4));

template <bool VEC> __global__ __launch_bounds__(NT) void bin_extremes_kernel(const float* __restrict__ y, int64_t n, int G, BinWs ws) {
    __shared__ BinRed red;
    const int t = threadIdx.x, g = blockIdx.x;
    const float* yi = y + (int64_t)blockIdx.y * n;
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (int k = 0; k < BIN_STEPS; ++k) {
        float v[4];
        const int c = load4<VEC>(yi, (int64_t)g * PREP_CHUNK + (int64_t)(k * NT + t) * 4, n, v);
        for (int e = 0; e < c; ++e) { mn = fminf(mn, v[e]); mx = fmaxf(mx, v[e]); bad |= !finite_f32(v[e]); }
    }
    mn = block_tree<NT>(mn, red.f, [](float a, float b) { return fminf(a, b); });
    mx = block_tree<NT>(mx, red.f, [](float a, float b) { return fmaxf(a, b); });
    bad = block_tree<NT>(bad, red.i, [](int a, int b) { return a | b; });
    if (t == 0) {
        const size_t at = (size_t)blockIdx.y * G + g;
        ws.pmn[at] = mn; ws.pmx[at] = mx; ws.pbad[at] = bad;
    }
}
// the image's extremes from its G chunks (every workgroup of the later launches repeats this: G words from L2)
__device__ __forceinline__ void bin_merge_extremes(const BinWs& ws, int G, BinRed& red, float& mn, float& mx, int& bad) {
    const size_t at = (size_t)blockIdx.y * G;
    mn = INFINITY; mx = -INFINITY; bad = 0;
    for (int j = threadIdx.x; j < G; j += NT) { mn = fminf(mn, ws.pmn[at + j]); mx = fmaxf(mx, ws.pmx[at + j]); bad |= ws.pbad[at + j]; }
    mn = block_tree<NT>(mn, red.f, [](float a, float b) { return fminf(a, b); });
    mx = block_tree<NT>(mx, red.f, [](float a, float b) { return fmaxf(a, b); });
    bad = block_tree<NT>(bad, red.i, [](int a, int b) { return a | b; });
}
template <bool VEC> __global__ __launch_bounds__(NT) void bin_sum_kernel(const float* __restrict__ y, int64_t n, int G, BinWs ws, cvae_binarise_record* __restrict__ rec) {
    __shared__ BinRed red;
    const int t = threadIdx.x, g = blockIdx.x;
    const float* yi = y + (int64_t)blockIdx.y * n;
    float mn, mx;
    int bad;
    bin_merge_extremes(ws, G, red, mn, mx, bad);
    const float range = mx - mn;
    double acc = 0.0;
    if (!bad && mx > mn)
        for (int k = 0; k < BIN_STEPS; ++k) {
            float v[4];
            const int c = load4<VEC>(yi, (int64_t)g * PREP_CHUNK + (int64_t)(k * NT + t) * 4, n, v);
            for (int e = 0; e < c; ++e) acc += (double)((v[e] - mn) / range);
        }
    acc = block_tree<NT>(acc, red.d, [](double a, double b) { return a + b; });
    if (t == 0) {
        ws.psum[(size_t)blockIdx.y * G + g] = acc;
        if (g == 0) rec[blockIdx.y].ones = 0;          // the apply launch counts into it
    }
}
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void bin_apply_kernel(const float* __restrict__ y, T* __restrict__ out, int H, int W, int A, int G, BinWs ws,
                                                        cvae_binarise_record* __restrict__ rec) {
    __shared__ BinRed red;
    __shared__ int ones_s;
    const int t = threadIdx.x, g = blockIdx.x;
    const int64_t n = (int64_t)H * W, b = blockIdx.y;
    const float* yi = y + b * n;
    if (t == 0) ones_s = 0;
    float mn, mx;
    int bad;
    bin_merge_extremes(ws, G, red, mn, mx, bad);
    double total = 0.0;
    for (int j = t; j < G; j += NT) total += ws.psum[(size_t)b * G + j];
    total = block_tree<NT>(total, red.d, [](double a, double c) { return a + c; });
    const int flags = bad ? CVAE_PREP_NONFINITE : (mx > mn ? 0 : CVAE_PREP_CONSTANT);
    const double thr = flags ? 0.0 : total / (double)n;
    const float range = mx - mn;
    int ones = 0;
    for (int k = 0; k < BIN_STEPS; ++k) {
        float v[4], m[4];
        const int64_t i = (int64_t)g * PREP_CHUNK + (int64_t)(k * NT + t) * 4;
        const int c = load4<VEC>(yi, i, n, v);
        if (c == 0) continue;
        for (int e = 0; e < c; ++e) {
            const bool one = !flags && (double)((v[e] - mn) / range) > thr;
            m[e] = one ? 1.f : 0.f;
            ones += one;
        }
        const int h = (int)(i / W), w = (int)(i - (int64_t)h * W);
        if (VEC) {          // W % 4 == 0: the four pixels share a row, and every variant's four are an aligned group
            const float rv[4] = {m[3], m[2], m[1], m[0]};
            for (int a = 0; a < A; ++a) {
                const int hh = (a & 2) ? H - 1 - h : h, ww = (a & 1) ? W - 4 - w : w;
                T* o = out + (b * A + a) * n + (int64_t)hh * W + ww;
                if (a & 1) store_from_f32<4>(o, rv);
                else store_from_f32<4>(o, m);
            }
        } else {
            for (int e = 0; e < c; ++e) {
                const int64_t ie = i + e;
                const int he = (int)(ie / W), we = (int)(ie - (int64_t)he * W);
                for (int a = 0; a < A; ++a) {
                    const int hh = (a & 2) ? H - 1 - he : he, ww = (a & 1) ? W - 1 - we : we;
                    out[(b * A + a) * n + (int64_t)hh * W + ww] = from_f32<T>(m[e]);
                }
            }
        }
    }
    if (ones) atomicAdd(&ones_s, ones);
    __syncthreads();
    if (t == 0) {
        if (ones_s) atomicAdd((unsigned long long*)&rec[b].ones, (unsigned long long)ones_s);          // integers: the order cannot show
        if (g == 0) { rec[b].thr = thr; rec[b].mn = mn; rec[b].mx = mx; rec[b].flags = flags; rec[b].reserved = 0; }
    }
}

// ------------------------------------------------------------------------------------------------ percentile clip and scale
// the order-preserving uint32 image of a float (-0 sorts just below +0) and back
__device__ __forceinline__ unsigned sel_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

struct SelState { unsigned prefix[4]; int64_t k[4]; };          // per image and rank: the digits found so far, and the rank among the keys that share them
struct SelRanks { int64_t k[4]; };
struct SelWs { SelState* state[2]; unsigned* hist; int* bad; };
inline int64_t sel_chunks(int64_t N) { return (N + SELECT_CHUNK - 1) / SELECT_CHUNK; }
inline size_t sel_ws_bytes(int64_t B, int64_t N) { return (size_t)B * 2 * sizeof(SelState) + (size_t)(B * sel_chunks(N)) * (4 * 256 * sizeof(unsigned) + sizeof(int)); }
inline SelWs sel_ws(void* ws, int64_t B, int64_t N) {
    SelWs w;
    w.state[0] = (SelState*)ws;
    w.state[1] = w.state[0] + B;
    w.hist = (unsigned*)(w.state[1] + B);
    w.bad = (int*)(w.hist + (size_t)(B * sel_chunks(N)) * 1024);
    return w;
}
constexpr int SEL_STEPS = (int)(SELECT_CHUNK / (NT * 4));
// the first rank whose prefix equals rank r's: the ranks of one percentile (and, early on, all four) share their digits and one histogram
__device__ __forceinline__ int sel_rep(const unsigned (&pre)[4], int r) {
    for (int q = 0; q < r; ++q)
        if (pre[q] == pre[r]) return q;
    return r;
}

// pass p (0 .. 3) looks at bits 31 - 8 p .. 24 - 8 p of the keys whose higher bits equal a rank's prefix
template <bool VEC> __global__ __launch_bounds__(NT) void sel_hist_kernel(const float* __restrict__ x, int64_t N, int pass, int G, const SelState* __restrict__ state,
                                                                          unsigned* __restrict__ hist, int* __restrict__ bad) {
    __shared__ unsigned h[4][256];
    __shared__ int bad_s;
    const int t = threadIdx.x, g = blockIdx.x;
    const int64_t b = blockIdx.y;
    const float* xi = x + b * N;
    for (int i = t; i < 1024; i += NT) (&h[0][0])[i] = 0u;
    if (t == 0) bad_s = 0;
    unsigned pre[4] = {0u, 0u, 0u, 0u};
    if (pass)
        for (int r = 0; r < 4; ++r) pre[r] = state[b].prefix[r];
    bool own[4];
    for (int r = 0; r < 4; ++r) own[r] = sel_rep(pre, r) == r;
    const unsigned himask = pass ? ~0u << (32 - 8 * pass) : 0u;
    const int shift = 24 - 8 * pass;
    __syncthreads();
    int lbad = 0;
    for (int k = 0; k < SEL_STEPS; ++k) {
        float v[4];
        const int c = load4<VEC>(xi, (int64_t)g * SELECT_CHUNK + (int64_t)(k * NT + t) * 4, N, v);
        for (int e = 0; e < c; ++e) {
            const unsigned key = sel_key(v[e]), hi = key & himask, dg = (key >> shift) & 255u;
            lbad |= !finite_f32(v[e]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (own[r] && hi == pre[r]) atomicAdd(&h[r][dg], 1u);
        }
    }
    if (lbad) atomicOr(&bad_s, 1);
    __syncthreads();
    unsigned* ho = hist + ((size_t)b * G + g) * 1024;
    for (int i = t; i < 1024; i += NT) ho[i] = (&h[0][0])[i];
    if (pass == 0 && t == 0) bad[b * G + g] = bad_s;
}
// one workgroup per (rank, image): the chunks' histograms added in chunk order, then the digit that holds the rank
// (PICK_SEGS x 256 threads: segment s adds its run of consecutive chunks with several loads in flight, then the segments are added in order; one thread
// walking all chunks cost 81 us per pass at 475 chunks, profiles/image_prep.md)
constexpr int PICK_SEGS = 4;
__global__ __launch_bounds__(PICK_SEGS * 256) void sel_pick_kernel(int pass, int G, SelRanks first, const unsigned* __restrict__ hist, const int* __restrict__ bad,
                                                                   const SelState* __restrict__ in, SelState* __restrict__ outs, cvae_clip_record* __restrict__ rec) {
    __shared__ unsigned seg[PICK_SEGS][256];
    __shared__ unsigned cnt[256];
    const int t = threadIdx.x & 255, s = threadIdx.x >> 8, r = blockIdx.x;
    const int64_t b = blockIdx.y;
    unsigned pre[4] = {0u, 0u, 0u, 0u};
    if (pass)
        for (int q = 0; q < 4; ++q) pre[q] = in[b].prefix[q];
    const int rep = sel_rep(pre, r);
    const unsigned* hb = hist + (size_t)b * G * 1024 + rep * 256 + t;
    const int per = (G + PICK_SEGS - 1) / PICK_SEGS, g0 = s * per, g1 = g0 + per < G ? g0 + per : G;
    unsigned c = 0u;
#pragma unroll 4
    for (int g = g0; g < g1; ++g) c += hb[(size_t)g * 1024];
    seg[s][t] = c;
    if (pass == 0 && r == 0) {
        int any = 0;
        for (int g = threadIdx.x; g < G; g += PICK_SEGS * 256) any |= bad[b * G + g];
        any = __syncthreads_or(any);
        if (threadIdx.x == 0) { rec[b].flags = any ? CVAE_PREP_NONFINITE : 0; rec[b].reserved = 0; }
    }
    __syncthreads();
    if (s == 0) {
        c = 0u;
        for (int q = 0; q < PICK_SEGS; ++q) c += seg[q][t];
        cnt[t] = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int64_t k = pass ? in[b].k[r] : first.k[r], cum = 0;
    int digit = 255;
    for (int dgt = 0; dgt < 256; ++dgt) {
        if (k < cum + (int64_t)cnt[dgt]) { digit = dgt; break; }
        cum += cnt[dgt];
    }
    outs[b].prefix[r] = pre[r] | ((unsigned)digit << (24 - 8 * pass));
    outs[b].k[r] = k - cum;
}
// numpy's _lerp on two float32 neighbours: the difference is formed in float32, everything after it in float64, product and sum rounded separately
__device__ __forceinline__ double np_lerp(float a, float b, double t) {
    const double d = (double)(b - a);
    if (t >= 0.5) {
        const double p = d * (1.0 - t);
        return (double)b - p;
    }
    const double p = d * t;
    return (double)a + p;
}
template <bool VEC> __global__ __launch_bounds__(NT) void clip_scale_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t N, const SelState* __restrict__ state,
                                                                            double t_lo, double t_hi, cvae_clip_record* __restrict__ rec) {
    const int64_t b = blockIdx.y;
    const SelState st = state[b];
    const double vmin = np_lerp(sel_value(st.prefix[0]), sel_value(st.prefix[1]), t_lo), vmax = np_lerp(sel_value(st.prefix[2]), sel_value(st.prefix[3]), t_hi);
    double denom = vmax - vmin;
    if (denom == 0.0) denom = 1e-5;
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec[b].vmin = vmin; rec[b].vmax = vmax; }
    const float* xi = x + b * N;
    float* oi = out + b * N;
    for (int k = 0; k < 4; ++k) {
        float v[4], o[4];
        const int64_t i = (int64_t)blockIdx.x * (NT * 16) + (int64_t)(k * NT + threadIdx.x) * 4;
        const int c = load4<VEC>(xi, i, N, v);
        if (c == 0) continue;
        for (int e = 0; e < c; ++e) {
            const double clipped = fmin(fmax((double)v[e], vmin), vmax);
            o[e] = (float)((clipped - vmin) / denom);
        }
        if (VEC) store_from_f32<4>(oi + i, o);
        else
            for (int e = 0; e < c; ++e) oi[i + e] = o[e];
    }
}

int prep_shape_rc(int64_t B, int64_t n) { return (B > MAX_BATCH || n > MAX_PIXELS) ? CVAE_E_UNSUPPORTED : CVAE_OK; }

}  // namespace

// ---- the C entries ----
extern "C" int cvae_mip_max(const void* src, float* dst, int64_t B, int64_t D, int64_t Hs, int64_t Ws, int src_dtype, void* stream) {
    if (B < 1 || D < 1 || Hs < 1 || Ws < 1) return CVAE_E_BADSHAPE;
    if (src_dtype != CVAE_F32 && src_dtype != CVAE_U16) return CVAE_E_DTYPE;
    if (Hs > MAX_PIXELS || Ws > MAX_PIXELS || D > MAX_PIXELS || prep_shape_rc(B, Hs * Ws) != CVAE_OK) return CVAE_E_UNSUPPORTED;
    if (any_null(src, dst)) return CVAE_E_NULLPTR;
    const int64_t P = Hs * Ws;
    const dim3 grid((unsigned)((P + NT * 8 - 1) / (NT * 8)), (unsigned)B);
    return with_bool(src_dtype == CVAE_U16, [&](auto u16) {
        using S = std::conditional_t<decltype(u16)::value, uint16_t, float>;
        return with_bool(P % 8 == 0 && aligned16(src) && aligned16(dst), [&](auto vec) {
            hipLaunchKernelGGL((mip_max_kernel<S, decltype(vec)::value>), grid, dim3(NT), 0, (hipStream_t)stream, (const S*)src, dst, (int)D, P);
            return launch_rc();
        });
    });
}

extern "C" int cvae_resize_bilinear_aa_f32(const float* src, float* dst, int64_t B, int64_t Hs, int64_t Ws, int64_t H, int64_t W, void* stream) {
    if (B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return CVAE_E_BADSHAPE;
    if (Hs > MAX_PIXELS || Ws > MAX_PIXELS || H > MAX_PIXELS || W > MAX_PIXELS || prep_shape_rc(B, Hs * Ws) != CVAE_OK || prep_shape_rc(B, H * W) != CVAE_OK ||
        (H + TH - 1) / TH > 65535)
        return CVAE_E_UNSUPPORTED;
    // the largest windows of the shape, by the kernel's own arithmetic
    const AaAxis ah = aa_axis((int)Hs, (int)H), aw = aa_axis((int)Ws, (int)W);
    int R = 1, KW = 1, KH = 1, lo, hi;
    for (int o = 0; o < (int)W; ++o) { aa_window(aw, o, (int)Ws, lo, hi); if (hi - lo > KW) KW = hi - lo; }
    for (int o = 0; o < (int)H; ++o) { aa_window(ah, o, (int)Hs, lo, hi); if (hi - lo > KH) KH = hi - lo; }
    for (int o0 = 0; o0 < (int)H; o0 += TH) {
        int lo1, hi1;
        aa_window(ah, o0, (int)Hs, lo, hi);
        aa_window(ah, (o0 + TH < (int)H ? o0 + TH : (int)H) - 1, (int)Hs, lo1, hi1);
        if (hi1 - lo > R) R = hi1 - lo;
    }
    const size_t lds = aa_lds_bytes(R, KW, KH);
    if (lds > CVAE_LDS_MAX) return CVAE_E_UNSUPPORTED;
    if (any_null(src, dst)) return CVAE_E_NULLPTR;
    if (cvae_allow_lds<resize_aa_kernel>(lds) != CVAE_OK) return CVAE_E_LAUNCH;
    hipLaunchKernelGGL(resize_aa_kernel, dim3((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)B), dim3(NT), lds, (hipStream_t)stream, src, dst,
                       (int)Hs, (int)Ws, (int)H, (int)W, R, KW, KH);
    return launch_rc();
}

extern "C" size_t cvae_minmax_binarise_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (B < 1 || H < 1 || W < 1 || H > MAX_PIXELS || W > MAX_PIXELS || prep_shape_rc(B, H * W) != CVAE_OK) return 0;
    return bin_ws_bytes(B, H * W);
}
extern "C" int cvae_minmax_binarise(const float* y, void* out, cvae_binarise_record* rec, int64_t B, int64_t H, int64_t W, int augment4, int out_dtype, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (B < 1 || H < 1 || W < 1) return CVAE_E_BADSHAPE;
    if (out_dtype != CVAE_F32 && out_dtype != CVAE_BF16) return CVAE_E_DTYPE;
    if (H > MAX_PIXELS || W > MAX_PIXELS || prep_shape_rc(B, H * W) != CVAE_OK) return CVAE_E_UNSUPPORTED;
    if (any_null(y, out, rec)) return CVAE_E_NULLPTR;
    const int64_t n = H * W;
    if (!workspace || workspace_bytes < bin_ws_bytes(B, n) || !aligned8(workspace)) return CVAE_E_WORKSPACE;
    const int G = (int)bin_chunks(n), A = augment4 ? 4 : 1;
    const BinWs ws = bin_ws(workspace, B, n);
    const dim3 grid((unsigned)G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    return with_bool(n % 4 == 0 && aligned16(y), [&](auto vin) {
        constexpr bool VIN = decltype(vin)::value;
        hipLaunchKernelGGL(bin_extremes_kernel<VIN>, grid, dim3(NT), 0, st, y, n, G, ws);
        CVAE_CHECK_LAUNCH();
        hipLaunchKernelGGL(bin_sum_kernel<VIN>, grid, dim3(NT), 0, st, y, n, G, ws, rec);
        CVAE_CHECK_LAUNCH();
        return with_bool(out_dtype == CVAE_BF16, [&](auto half) {
            using T = std::conditional_t<decltype(half)::value, bf16, float>;
            return with_bool(VIN && W % 4 == 0 && aligned16(out), [&](auto vec) {
                hipLaunchKernelGGL((bin_apply_kernel<T, decltype(vec)::value>), grid, dim3(NT), 0, st, y, (T*)out, (int)H, (int)W, A, G, ws, rec);
                return launch_rc();
            });
        });
    });
}

extern "C" size_t cvae_percentile_clip_scale_workspace_bytes(int64_t B, int64_t N) {
    if (B < 1 || N < 1 || prep_shape_rc(B, N) != CVAE_OK) return 0;
    return sel_ws_bytes(B, N);
}
extern "C" int cvae_percentile_clip_scale(const float* x, float* out, cvae_clip_record* rec, int64_t B, int64_t N, const int64_t* ranks, const double* t, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    if (B < 1 || N < 1) return CVAE_E_BADSHAPE;
    if (prep_shape_rc(B, N) != CVAE_OK) return CVAE_E_UNSUPPORTED;
    if (any_null(x, out, rec, ranks, t)) return CVAE_E_NULLPTR;
    SelRanks first;
    for (int r = 0; r < 4; ++r) {
        if (ranks[r] < 0 || ranks[r] >= N) return CVAE_E_BADSHAPE;
        first.k[r] = ranks[r];
    }
    if (!(t[0] == t[0]) || !(t[1] == t[1])) return CVAE_E_BADSHAPE;
    if (!workspace || workspace_bytes < sel_ws_bytes(B, N) || !aligned8(workspace)) return CVAE_E_WORKSPACE;
    const int G = (int)sel_chunks(N);
    const SelWs ws = sel_ws(workspace, B, N);
    hipStream_t st = (hipStream_t)stream;
    const double t_lo = t[0], t_hi = t[1];
    return with_bool(N % 4 == 0 && aligned16(x) && aligned16(out), [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        for (int pass = 0; pass < 4; ++pass) {
            const SelState* in = ws.state[(pass + 1) & 1];          // written by the pass before; pass 0 reads none
            SelState* outs = ws.state[pass & 1];
            hipLaunchKernelGGL(sel_hist_kernel<VEC>, dim3((unsigned)G, (unsigned)B), dim3(NT), 0, st, x, N, pass, G, in, ws.hist, ws.bad);
            CVAE_CHECK_LAUNCH();
            hipLaunchKernelGGL(sel_pick_kernel, dim3(4, (unsigned)B), dim3(PICK_SEGS * 256), 0, st, pass, G, first, (const unsigned*)ws.hist, (const int*)ws.bad, in, outs, rec);
            CVAE_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(clip_scale_kernel<VEC>, dim3((unsigned)((N + NT * 16 - 1) / (NT * 16)), (unsigned)B), dim3(NT), 0, st, x, out, N,
                           (const SelState*)ws.state[1], t_lo, t_hi, rec);
        return launch_rc();
    });
}
