// ridge.hip — the latent translator (the reference's latent_translator/analysis.py:11-82, 91-165): a Ridge regression from the
// latents Z [N, d] to the morphology table M [N, F] with an unpenalised intercept, its EXACT leave-one-out predictions from one factorisation, the ranking
// statistics of those predictions, and the resampled group means of the group-contrast bootstrap; and, on the eigendecomposition of eigh.hip (DESIGN.md
// section 26), the leave-one-out predictions of a whole grid of alphas and the latent PCA.  Everything here is float64; with eigh.hip the library's only fp64 code.
//   col means    zbar, mbar: per-chunk column sums, added in chunk order, divided by N
//   gram         A = Xc^T Xc + alpha I [d, d] and R = Xc^T Yc [d, F] with Xc = Z - zbar, Yc = M - mbar: the centring happens on load (mean first, then the
//                centred products; never E[xy] - E[x] E[y]).  v_mfma_f64_16x16x4_f64: a wave owns a 32 x 32 tile of the [d, d + F] product, the four rows of a
//                k step come straight from global memory (16 lanes read 128 contiguous bytes).  The rows are split into chunks (a function of N alone); the
//                chunks' partial products are added in chunk order by a finish launch, which also adds alpha to the diagonal.
//   chol         A = L L^T in place (lower triangle), right-looking in 64-column blocks: panel (one workgroup, in LDS), the rows below it (the trsm kernel, one
//                thread per row), the trailing update (32 x 32 tiles) — three launches per block, a launch boundary being the only grid-wide synchronisation.
//   trsm         L T = B (forward) or L^T W = B (backward) on [d, n] right-hand sides, one thread per column, 32 rows of it in registers at a time
//   loo          h_i = 1 / N + sum_k T[k, i]^2;  Yhat = mbar + Xc W;  P = M - (M - Yhat) / (1 - h);  coef = W^T, intercept = mbar - zbar^T W
//   stats        per feature: R^2 and Pearson correlation of P against M under the reference's rules
//   group means  out[b, g] = mean over i, in index order, of Z[idx[b, i]] whose group code is g
//   matmul       out = (X - mean) B on the fp64 MFMA, the mean subtracted on load, either operand a transpose in place: P = Xc V, Q = V^T Xc^T Yc, PCA's transform
//   path         per alpha of a grid in device memory: h = 1 / N + sum_k P_k^2 / (lambda_k + alpha), loo from Yhat = mbar + P diag(1 / (lambda + alpha)) Q, sse
//   pca          the top components in descending order with sklearn's sign rule, their variances, ratios and singular values
// No float atomics, no workgroup waits on another, every sum has one fixed order and every grid is a function of the shape alone: two runs give equal bits.
// A sum is a thread's terms in index order, chunks in chunk order, and across a workgroup common.h's LDS tree (block_tree: stats, sse, PCA's arg-max).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int RG_ROWS = 256;          // a row chunk is a multiple of this many rows ..
constexpr int RG_MAX_PARTS = 16;      // .. the smallest that leaves at most this many chunks
constexpr int CH_NB = 64;             // Cholesky block width
constexpr int CH_TILE = 32;           // trailing-update tile
constexpr int TR_ROWS = 32;           // trsm: rows of a column held in registers
constexpr int TR_COLS = 64;           // trsm: columns (threads) per workgroup

int64_t rg_chunk(int64_t N) {
    const int64_t unit = (int64_t)RG_ROWS * RG_MAX_PARTS;
    return RG_ROWS * ((N + unit - 1) / unit);
}
int64_t rg_parts(int64_t N) {
    const int64_t chunk = rg_chunk(N);
    return (N + chunk - 1) / chunk;
}

// the sum of v over the 256 threads of a workgroup by common.h's LDS tree; every thread gets it
__device__ __forceinline__ double tree_sum256(double v, double* red) {
    return block_tree<256>(v, red, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ double clamp0(double x) { return x > 0.0 ? x : 0.0; }          // an eigenvalue of a positive semidefinite matrix

// ---- column means ----
// grid (ceil(C / 256), parts): thread c adds its column over the chunk's rows in row order
__global__ __launch_bounds__(256) void col_sums_kernel(const double* __restrict__ x, int64_t N, int C, int64_t stride, int64_t chunk, double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = (p0 + chunk < N) ? p0 + chunk : N;
    double s = 0.0;
    for (int64_t p = p0; p < p1; ++p) s += x[p * stride + c];
    part[(size_t)blockIdx.y * C + c] = s;
}
__global__ __launch_bounds__(256) void col_means_finish_kernel(const double* __restrict__ part, int parts, int64_t N, int C, double* __restrict__ mean) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int g = 0; g < parts; ++g) s += part[(size_t)g * C + c];
    mean[c] = s / (double)N;
}

// ---- the centred Gram matrix on the fp64 MFMA ----
// Operand lane map of v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one double each; result register r of lane l
// is C[row (l >> 4) + 4 r][col l & 15].  Here A = Xc^T (row i of the product = column i of Z) and B = [Xc | Yc].
// grid (ceil((d + F) / 64), ceil(d / 64), parts), 4 waves: wave w owns the 32 x 32 tile (w >> 1, w & 1) of the workgroup's 64 x 64.
__global__ __launch_bounds__(256) void ridge_gram_kernel(const double* __restrict__ Z, int64_t zs, const double* __restrict__ zbar, const double* __restrict__ M,
                                                         int64_t ms, const double* __restrict__ mbar, int64_t N, int d, int F, int64_t chunk,
                                                         double* __restrict__ part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int W = d + F;
    const int i0 = blockIdx.y * 64 + (w >> 1) * 32, j0 = blockIdx.x * 64 + (w & 1) * 32;
    if (i0 >= d || j0 >= W) return;          // wave-uniform; the kernel has no barrier
    const int64_t p0 = (int64_t)blockIdx.z * chunk, p1 = (p0 + chunk < N) ? p0 + chunk : N;
    const double* pa[2];
    const double* pb[2];
    int64_t sb[2];
    double ca[2], cb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = i0 + 16 * u + lr, j = j0 + 16 * u + lr;
        pa[u] = i < d ? Z + i : nullptr;
        ca[u] = i < d ? zbar[i] : 0.0;
        pb[u] = j < d ? Z + j : (j < W ? M + (j - d) : nullptr);
        sb[u] = j < d ? zs : ms;
        cb[u] = j < d ? zbar[j] : (j < W ? mbar[j - d] : 0.0);
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t p = p0; p < p1; p += 4) {
        const int64_t row = p + lk;
        const bool in = row < p1;
        double a[2], b[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            a[u] = (in && pa[u]) ? pa[u][row * zs] - ca[u] : 0.0;
            b[u] = (in && pb[u]) ? pb[u][row * sb[u]] - cb[u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
    }
    double* out = part + (size_t)blockIdx.z * d * W;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * u + lk + 4 * r, j = j0 + 16 * v + lr;
                if (i < d && j < W) out[(size_t)i * W + j] = acc[u][v][r];
            }
}
// the chunks' partial products added in chunk order; alpha joins the diagonal of A
__global__ __launch_bounds__(256) void ridge_gram_finish_kernel(const double* __restrict__ part, int parts, int d, int F, double alpha, double* __restrict__ A,
                                                                double* __restrict__ R) {
    const int W = d + F;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)d * W) return;
    const int i = (int)(e / W), j = (int)(e % W);
    double s = 0.0;
    for (int g = 0; g < parts; ++g) s += part[(size_t)g * d * W + e];
    if (j < d) A[(size_t)i * d + j] = (i == j) ? s + alpha : s;
    else R[(size_t)i * F + (j - d)] = s;
}

// ---- Cholesky ----
// panel: the diagonal block [k0, k0 + nb) in LDS, lower triangle only.  A pivot that is not > 0 (NaN included) becomes NaN and is recorded in *info as
// column + 1 unless an earlier column already was; the NaN then spreads over every later column by the arithmetic itself.
__global__ __launch_bounds__(256) void chol_panel_kernel(double* __restrict__ A, int d, int k0, int nb, int* __restrict__ info) {
    __shared__ double S[CH_NB][CH_NB + 1];
    const int t = threadIdx.x;
    for (int e = t; e < nb * nb; e += 256) {
        const int i = e / nb, j = e % nb;
        if (j <= i) S[i][j] = A[(size_t)(k0 + i) * d + k0 + j];
    }
    int bad = 0;
    for (int j = 0; j < nb; ++j) {
        __syncthreads();
        if (t == 0) {
            double p = S[j][j];
            if (!(p > 0.0)) {
                if (bad == 0) bad = k0 + j + 1;
                p = __builtin_nan("");
            }
            S[j][j] = sqrt(p);
        }
        __syncthreads();
        const double piv = S[j][j];
        for (int i = j + 1 + t; i < nb; i += 256) S[i][j] /= piv;
        __syncthreads();
        const int m = nb - j - 1;
        for (int e = t; e < m * m; e += 256) {
            const int i = j + 1 + e / m, k = j + 1 + e % m;
            if (k <= i) S[i][k] -= S[i][j] * S[k][j];
        }
    }
    __syncthreads();
    for (int e = t; e < nb * nb; e += 256) {
        const int i = e / nb, j = e % nb;
        if (j <= i) A[(size_t)(k0 + i) * d + k0 + j] = S[i][j];
    }
    if (t == 0) {
        if (k0 == 0) *info = bad;
        else if (bad != 0 && *info == 0) *info = bad;
    }
}
// the trailing update A22 -= L21 L21^T on 32 x 32 tiles with tile row >= tile column (the tiles on the diagonal whole); thread (ty, tx) owns a 2 x 2 patch
__global__ __launch_bounds__(256) void chol_update_kernel(double* __restrict__ A, int d, int k0, int nb) {
    if (blockIdx.x > blockIdx.y) return;
    __shared__ double Pi[CH_TILE][CH_NB + 1], Pj[CH_TILE][CH_NB + 1];
    const int t = threadIdx.x, t0 = k0 + nb;
    const int ib = t0 + blockIdx.y * CH_TILE, jb = t0 + blockIdx.x * CH_TILE;
    for (int e = t; e < CH_TILE * CH_NB; e += 256) {
        const int r = e / CH_NB, m = e % CH_NB;
        Pi[r][m] = (ib + r < d && m < nb) ? A[(size_t)(ib + r) * d + k0 + m] : 0.0;
        Pj[r][m] = (jb + r < d && m < nb) ? A[(size_t)(jb + r) * d + k0 + m] : 0.0;
    }
    __syncthreads();
    const int ty = t >> 4, tx = t & 15;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll 4
    for (int m = 0; m < CH_NB; ++m) {
        const double a0 = Pi[ty][m], a1 = Pi[ty + 16][m], b0 = Pj[tx][m], b1 = Pj[tx + 16][m];
        acc[0][0] += a0 * b0; acc[0][1] += a0 * b1; acc[1][0] += a1 * b0; acc[1][1] += a1 * b1;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = ib + ty + 16 * u, j = jb + tx + 16 * v;
            if (i < d && j < d) A[(size_t)i * d + j] -= acc[u][v];
        }
}

// ---- triangular solves ----
// One thread per right-hand-side column c; TR_ROWS rows of the column live in registers while the rows already solved are read back (by the thread that wrote
// them) and the matching TR_ROWS x 64 piece of L passes through LDS.  REV (L^T W = B) is the forward solve on reversed indices k' = d - 1 - k, in which L^T is
// lower triangular again.  The right-hand side is read as in[row * in_rs + c * in_cs] - shift[row] (shift may be null), so X_c^T is taken from Z in place; the
// result goes to out[row * out_rs + c * out_cs], so the Cholesky's rows below a panel (X L11^T = A21, i.e. L11 X^T = A21^T) are solved where they lie.
// The diagonal block is solved by rotation: x = acc[0] / L[r][r], then acc[i] = acc[i + 1] - L[r + 1 + i][r] x, so the register indices are constants.
template <bool REV>
__global__ __launch_bounds__(TR_COLS) void trsm_kernel(const double* L, int64_t ldl, const double* in, int64_t in_rs, int64_t in_cs, const double* __restrict__ shift,
                                                        double* out, int64_t out_rs, int64_t out_cs, int d, int64_t n) {
    __shared__ double Ls[TR_ROWS * 64];          // [TR_ROWS][64] below the diagonal block, [2 TR_ROWS][TR_ROWS] on it (rows past TR_ROWS zero)
    const int t = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * TR_COLS + t;
    const bool active = c < n;
    auto Lop = [&](int k, int j) -> double { return REV ? L[(size_t)(d - 1 - j) * ldl + (d - 1 - k)] : L[(size_t)k * ldl + j]; };
    auto row_of = [&](int k) -> int { return REV ? d - 1 - k : k; };
    for (int k0 = 0; k0 < d; k0 += TR_ROWS) {
        double acc[TR_ROWS];
#pragma unroll
        for (int r = 0; r < TR_ROWS; ++r) {
            const int k = k0 + r;
            acc[r] = 0.0;
            if (active && k < d) {
                const int row = row_of(k);
                acc[r] = in[(size_t)row * in_rs + c * in_cs] - (shift ? shift[row] : 0.0);
            }
        }
        for (int j0 = 0; j0 < k0; j0 += 64) {
            const int jw = (k0 - j0 < 64) ? k0 - j0 : 64;
            __syncthreads();
            for (int e = t; e < TR_ROWS * 64; e += TR_COLS) {
                const int r = REV ? e % TR_ROWS : e / 64, jj = REV ? e / TR_ROWS : e % 64;
                Ls[r * 64 + jj] = (k0 + r < d && jj < jw) ? Lop(k0 + r, j0 + jj) : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int jj = 0; jj < jw; ++jj) {
                const double x = active ? out[(size_t)row_of(j0 + jj) * out_rs + c * out_cs] : 0.0;
#pragma unroll
                for (int r = 0; r < TR_ROWS; ++r) acc[r] -= Ls[r * 64 + jj] * x;
            }
        }
        __syncthreads();
        for (int e = t; e < 2 * TR_ROWS * TR_ROWS; e += TR_COLS) {
            const int r = REV ? e % (2 * TR_ROWS) : e / TR_ROWS, jj = REV ? e / (2 * TR_ROWS) : e % TR_ROWS;
            Ls[r * TR_ROWS + jj] = (r < TR_ROWS && k0 + r < d && jj <= r) ? Lop(k0 + r, k0 + jj) : (r == jj ? 1.0 : 0.0);
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < TR_ROWS; ++r) {
            const double x = acc[0] / Ls[r * TR_ROWS + r];
            if (active && k0 + r < d) out[(size_t)row_of(k0 + r) * out_rs + c * out_cs] = x;
#pragma unroll
            for (int i = 0; i < TR_ROWS - 1; ++i) acc[i] = acc[i + 1] - Ls[(r + 1 + i) * TR_ROWS + r] * x;
            acc[TR_ROWS - 1] = 0.0;
        }
    }
}

// ---- leverages, fit, leave-one-out predictions ----
__global__ __launch_bounds__(256) void ridge_leverage_kernel(const double* __restrict__ T, int64_t N, int d, double* __restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const double v = T[(size_t)k * N + i];
        s += v * v;
    }
    h[i] = 1.0 / (double)N + s;
}
__global__ __launch_bounds__(256) void ridge_fit_kernel(const double* __restrict__ Z, int64_t zs, const double* __restrict__ zbar, const double* __restrict__ M,
                                                        int64_t ms, const double* __restrict__ mbar, const double* __restrict__ Wm, const double* __restrict__ h,
                                                        int64_t N, int d, int F, double* __restrict__ fitted, double* __restrict__ loo) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * F) return;
    const int64_t i = e / F;
    const int j = (int)(e % F);
    double s = 0.0;
    for (int k = 0; k < d; ++k) s += (Z[i * zs + k] - zbar[k]) * Wm[(size_t)k * F + j];
    const double yh = mbar[j] + s, y = M[i * ms + j];
    fitted[e] = yh;
    loo[e] = y - (y - yh) / (1.0 - h[i]);
}
// coef [F, d] = W^T; intercept = mbar - zbar^T W (written by the thread of k == 0)
__global__ __launch_bounds__(256) void ridge_coef_kernel(const double* __restrict__ Wm, const double* __restrict__ zbar, const double* __restrict__ mbar, int d, int F,
                                                         double* __restrict__ coef, double* __restrict__ intercept) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)F * d) return;
    const int j = (int)(e / d), k = (int)(e % d);
    coef[e] = Wm[(size_t)k * F + j];
    if (k == 0) {
        double s = 0.0;
        for (int q = 0; q < d; ++q) s += zbar[q] * Wm[(size_t)q * F + j];
        intercept[j] = mbar[j] - s;
    }
}
__global__ __launch_bounds__(256) void ridge_predict_kernel(const double* __restrict__ Z, int64_t zs, const double* __restrict__ coef, const double* __restrict__ intercept,
                                                            int64_t N, int d, int F, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * F) return;
    const int64_t i = e / F;
    const int j = (int)(e % F);
    double s = 0.0;
    for (int k = 0; k < d; ++k) s += Z[i * zs + k] * coef[(size_t)j * d + k];
    out[e] = intercept[j] + s;
}

// ---- ranking statistics: one workgroup per feature ----
__global__ __launch_bounds__(256) void ranking_stats_kernel(const double* __restrict__ Y, int64_t ys, const double* __restrict__ P, int64_t ps, int64_t N,
                                                            double* __restrict__ r2, double* __restrict__ corr) {
    __shared__ double red[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double sy = 0.0, sp = 0.0;
    for (int64_t i = t; i < N; i += 256) { sy += Y[i * ys + j]; sp += P[i * ps + j]; }
    const double my = tree_sum256(sy, red) / (double)N, mp = tree_sum256(sp, red) / (double)N;
    double res = 0.0, syy = 0.0, spp = 0.0, syp = 0.0;
    for (int64_t i = t; i < N; i += 256) {
        const double y = Y[i * ys + j], p = P[i * ps + j], dy = y - my, dp = p - mp;
        res += (y - p) * (y - p); syy += dy * dy; spp += dp * dp; syp += dy * dp;
    }
    res = tree_sum256(res, red); syy = tree_sum256(syy, red); spp = tree_sum256(spp, red); syp = tree_sum256(syp, red);
    if (t != 0) return;
    r2[j] = (syy == 0.0) ? (res == 0.0 ? 1.0 : 0.0) : 1.0 - res / syy;      // a constant truth: sklearn's r2_score gives 1 for a perfect prediction, else 0
    double c = 0.0;
    if (!(sqrt(syy / (double)N) < 1e-12 || sqrt(spp / (double)N) < 1e-12)) {
        c = syp / (sqrt(syy) * sqrt(spp));
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);                          // numpy.corrcoef clips as well
    }
    corr[j] = c;
}

// ---- resampled group means: grid (ceil(d / 64), G, n_boot), thread = one latent dimension ----
// an index outside [0, N) or a code outside [0, G) belongs to no group
__global__ __launch_bounds__(64) void group_means_resampled_kernel(const double* __restrict__ Z, int64_t zs, const int* __restrict__ codes, const int* __restrict__ idx,
                                                                   int64_t N, int d, int G, double* __restrict__ out, int* __restrict__ counts) {
    const int c = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int* ib = idx + b * N;
    double s = 0.0;
    int cnt = 0;
    for (int64_t i = 0; i < N; ++i) {
        const int r = ib[i];
        if (r < 0 || r >= N || codes[r] != g) continue;
        ++cnt;
        if (c < d) s += Z[(size_t)r * zs + c];
    }
    if (c < d) out[((size_t)b * G + g) * d + c] = cnt ? s / (double)cnt : 0.0;
    if (c == 0) counts[b * G + g] = cnt;
}

// ---- the alpha path and the latent PCA on an eigendecomposition of the centred Gram matrix ----
// out [R][C] = (X - mean) B on the fp64 MFMA: X is read as x[i * xrs + k * xcs] - mean[k] (mean may be null), B as b[k * brs + j * bcs], so either operand may be
// a transpose in place.  The mean is subtracted on load (centre first, then multiply).  grid (ceil(C / 64), ceil(R / 64)), 4 waves, a wave owns a 32 x 32 tile
// and walks the whole of K in order: no split, one fixed order.
__global__ __launch_bounds__(256) void centered_matmul_kernel(const double* __restrict__ x, int64_t xrs, int64_t xcs, const double* __restrict__ mean,
                                                              const double* __restrict__ b, int64_t brs, int64_t bcs, int64_t R, int K, int64_t C,
                                                              double* __restrict__ out, int64_t ldo) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.y * 64 + (w >> 1) * 32, j0 = (int64_t)blockIdx.x * 64 + (w & 1) * 32;
    if (i0 >= R || j0 >= C) return;          // wave-uniform; the kernel has no barrier
    const double* pa[2];
    const double* pb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t i = i0 + 16 * u + lr, j = j0 + 16 * u + lr;
        pa[u] = i < R ? x + i * xrs : nullptr;
        pb[u] = j < C ? b + j * bcs : nullptr;
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + lk;
        const bool in = k < K;
        const double mk = (in && mean) ? mean[k] : 0.0;
        double a[2], bb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            a[u] = (in && pa[u]) ? pa[u][k * xcs] - mk : 0.0;
            bb[u] = (in && pb[u]) ? pb[u][k * brs] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bb[v], acc[u][v], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + 16 * u + lk + 4 * r, j = j0 + 16 * v + lr;
                if (i < R && j < C) out[i * ldo + j] = acc[u][v][r];
            }
}

// the path: with P = Xc V [N, d], Q = V^T Xc^T Yc [d, F] and the eigenvalues clamped at 0 from below (the Gram matrix is positive semidefinite by construction),
//   h[g, i] = 1 / N + sum_k P[i, k]^2 / (lambda_k + alpha_g),  yhat = mbar + sum_k P[i, k] Q[k, j] / (lambda_k + alpha_g),  loo = y - (y - yhat) / (1 - h)
// every sum over k in index order.  grid (ceil(N / 256), G); the threads of row 0 also write the clamped eigenvalues.
__global__ __launch_bounds__(256) void ridge_path_leverage_kernel(const double* __restrict__ P, const double* __restrict__ lam, const double* __restrict__ alphas,
                                                                  int64_t N, int d, double* __restrict__ h, double* __restrict__ lam_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int g = blockIdx.y;
    if (g == 0 && blockIdx.x == 0)
        for (int k = threadIdx.x; k < d; k += 256) lam_out[k] = clamp0(lam[k]);
    if (i >= N) return;
    const double alpha = alphas[g];
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const double v = P[i * d + k], l = clamp0(lam[k]);
        s += v * v / (l + alpha);
    }
    h[(size_t)g * N + i] = 1.0 / (double)N + s;
}
// grid (ceil(N F / 256), G)
__global__ __launch_bounds__(256) void ridge_path_loo_kernel(const double* __restrict__ P, const double* __restrict__ Q, const double* __restrict__ lam,
                                                             const double* __restrict__ alphas, const double* __restrict__ M, int64_t ms,
                                                             const double* __restrict__ mbar, const double* __restrict__ h, int64_t N, int d, int F,
                                                             double* __restrict__ loo) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int g = blockIdx.y;
    if (e >= N * F) return;
    const int64_t i = e / F;
    const int j = (int)(e % F);
    const double alpha = alphas[g];
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const double l = clamp0(lam[k]);
        s += P[i * d + k] * Q[(size_t)k * F + j] / (l + alpha);
    }
    const double yh = mbar[j] + s, y = M[i * ms + j];
    loo[(size_t)g * N * F + e] = y - (y - yh) / (1.0 - h[(size_t)g * N + i]);
}
// grid (F, G): one workgroup per (feature, alpha); a thread adds its rows in row order, the 256 partial sums are added in a fixed tree
__global__ __launch_bounds__(256) void ridge_path_sse_kernel(const double* __restrict__ M, int64_t ms, const double* __restrict__ loo, int64_t N, int F,
                                                             double* __restrict__ sse) {
    __shared__ double red[256];
    const int j = blockIdx.x, g = blockIdx.y;
    const double* lg = loo + (size_t)g * N * F;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const double r = M[i * ms + j] - lg[i * F + j];
        s += r * r;
    }
    s = tree_sum256(s, red);
    if (threadIdx.x == 0) sse[(size_t)g * F + j] = s;
}

// PCA's components from an ascending eigendecomposition (w [d], V [d][d], column k the eigenvector of w[k]): workgroup c takes column d - 1 - c (descending
// order), finds its entry of largest |value| (lowest index on a tie) and writes the column, signed so that this entry is positive, as row c of comp [k][d];
// thread 0 writes the variance w / (N - 1), its share of the sum of all d eigenvalues (added in index order) and the singular value sqrt(w), w clamped at 0.
struct ArgMax { double v; int i; };
__global__ __launch_bounds__(256) void pca_components_kernel(const double* __restrict__ w, const double* __restrict__ V, int64_t ldv, int d, int64_t N,
                                                             double* __restrict__ comp, double* __restrict__ var, double* __restrict__ ratio,
                                                             double* __restrict__ sing) {
    __shared__ ArgMax red[256];
    const int c = blockIdx.x, t = threadIdx.x, col = d - 1 - c;
    ArgMax best = {-1.0, d};
    for (int i = t; i < d; i += 256) {          // ascending i within a thread: a strict > keeps the lowest index
        const double a = fabs(V[(size_t)i * ldv + col]);
        if (a > best.v) best = {a, i};
    }
    // a larger value wins, at equal value the lower index
    const int lead = block_tree<256>(best, red, [](ArgMax a, ArgMax b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }).i;
    const double sign = (lead < d && V[(size_t)lead * ldv + col] < 0.0) ? -1.0 : 1.0;
    for (int i = t; i < d; i += 256) comp[(size_t)c * d + i] = sign * V[(size_t)i * ldv + col];
    if (t != 0) return;
    double total = 0.0;
    for (int k = 0; k < d; ++k) total += clamp0(w[k]);
    const double l = clamp0(w[col]);
    var[c] = l / (double)(N - 1);
    ratio[c] = l / total;
    sing[c] = sqrt(l);
}

constexpr int64_t RIDGE_MAX_ROWS = (int64_t)1 << 31;      // N and n stay below 2^31, F below 2^21 and N F below 2^38 (a grid of 256-thread workgroups over it)
bool rows_features_ok(int64_t N, int64_t F) { return N < RIDGE_MAX_ROWS && F >= 1 && F < RIDGE_MAX_ROWS / 1024 && N * F < ((int64_t)1 << 38); }
bool ridge_shape_ok(int64_t N, int64_t d, int64_t F) { return N >= 2 && d >= 1 && d <= 1024 && rows_features_ok(N, F); }
bool gram_shape_ok(int64_t N, int64_t d, int64_t F) { return N >= 1 && N < RIDGE_MAX_ROWS && d >= 1 && d <= 1024 && F >= 0 && F < RIDGE_MAX_ROWS / 1024; }
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// behind both Gram entries, each of which has made its own checks of shape, pointers and alignment: the workspace (one [d, d + F] partial product per row
// chunk), the chunks' products, and their sum in chunk order with `shift` added to the diagonal
size_t gram_ws_bytes(int64_t N, int64_t d, int64_t F) { return (size_t)rg_parts(N) * d * (d + F) * sizeof(double); }
int gram_launch(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, int64_t N, int64_t d, int64_t F,
                double shift, double* A, double* R, void* workspace, size_t workspace_bytes, void* stream) {
    if (workspace_bytes < gram_ws_bytes(N, d, F)) return CVAE_E_WORKSPACE;
    const int parts = (int)rg_parts(N);
    const int64_t W = d + F;
    hipLaunchKernelGGL(ridge_gram_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((d + 63) / 64), (unsigned)parts), dim3(256), 0, (hipStream_t)stream, Z, z_stride,
                       z_mean, M, m_stride, m_mean, N, (int)d, (int)F, rg_chunk(N), (double*)workspace);
    hipLaunchKernelGGL(ridge_gram_finish_kernel, dim3(blocks256(d * W)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, parts, (int)d, (int)F, shift, A, R);
    return launch_rc();
}

}  // namespace

extern "C" size_t cvae_col_means_f64_workspace_bytes(int64_t N, int64_t C) {
    if (N < 1 || N >= RIDGE_MAX_ROWS || C < 1 || C >= RIDGE_MAX_ROWS) return 0;
    return (size_t)rg_parts(N) * C * sizeof(double);
}
extern "C" int cvae_col_means_f64(const double* x, int64_t N, int64_t C, int64_t stride, double* mean, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 1 || N >= RIDGE_MAX_ROWS || C < 1 || C >= RIDGE_MAX_ROWS || stride < C) return CVAE_E_BADSHAPE;
    if (any_null(x, mean, workspace)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(x, mean, workspace)) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_col_means_f64_workspace_bytes(N, C)) return CVAE_E_WORKSPACE;
    const int parts = (int)rg_parts(N);
    hipLaunchKernelGGL(col_sums_kernel, dim3(blocks256(C), (unsigned)parts), dim3(256), 0, (hipStream_t)stream, x, N, (int)C, stride, rg_chunk(N), (double*)workspace);
    hipLaunchKernelGGL(col_means_finish_kernel, dim3(blocks256(C)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, parts, N, (int)C, mean);
    return launch_rc();
}

extern "C" size_t cvae_ridge_gram_f64_workspace_bytes(int64_t N, int64_t d, int64_t F) {
    if (!ridge_shape_ok(N, d, F)) return 0;
    return gram_ws_bytes(N, d, F);
}
extern "C" int cvae_ridge_gram_f64(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, int64_t N,
                                   int64_t d, int64_t F, double alpha, double* A, double* R, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ridge_shape_ok(N, d, F) || z_stride < d || m_stride < F) return CVAE_E_BADSHAPE;
    if (!(alpha > 0.0) || !finite_f64(alpha)) return CVAE_E_BADSHAPE;      // a NaN or an infinity too: the centred Gram matrix is singular without alpha
    if (any_null(Z, z_mean, M, m_mean, A, R, workspace)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Z, z_mean, M, m_mean, A, R, workspace)) return CVAE_E_UNSUPPORTED;
    return gram_launch(Z, z_stride, z_mean, M, m_stride, m_mean, N, d, F, alpha, A, R, workspace, workspace_bytes, stream);
}

extern "C" int cvae_chol_f64(double* A, int64_t d, int* info, void* stream) {
    if (d < 1 || d > 1024) return CVAE_E_BADSHAPE;
    if (any_null(A, info)) return CVAE_E_NULLPTR;
    if (!aligned8(A) || !aligned4(info)) return CVAE_E_UNSUPPORTED;
    const int n = (int)d;
    for (int k0 = 0; k0 < n; k0 += CH_NB) {
        const int nb = (n - k0 < CH_NB) ? n - k0 : CH_NB, rest = n - k0 - nb;
        hipLaunchKernelGGL(chol_panel_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, A, n, k0, nb, info);
        if (rest > 0) {
            const unsigned tiles = (unsigned)((rest + CH_TILE - 1) / CH_TILE);
            double* L11 = A + (size_t)k0 * n + k0;
            double* A21 = A + (size_t)(k0 + nb) * n + k0;          // row i of A21 is column i of the right-hand side A21^T, solved in place
            hipLaunchKernelGGL(trsm_kernel<false>, dim3((unsigned)((rest + TR_COLS - 1) / TR_COLS)), dim3(TR_COLS), 0, (hipStream_t)stream, (const double*)L11,
                               (int64_t)n, (const double*)A21, (int64_t)1, (int64_t)n, (const double*)nullptr, A21, (int64_t)1, (int64_t)n, nb, (int64_t)rest);
            hipLaunchKernelGGL(chol_update_kernel, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, A, n, k0, nb);
        }
    }
    return launch_rc();
}

extern "C" int cvae_trsm_f64(const double* L, int64_t ldl, const double* in, int64_t in_row_stride, int64_t in_col_stride, const double* row_shift, double* out,
                             int64_t ldo, int64_t d, int64_t n, int transpose, void* stream) {
    if (d < 1 || d > 1024 || n < 1 || n >= RIDGE_MAX_ROWS || ldl < d || ldo < n || in_row_stride < 1 || in_col_stride < 1) return CVAE_E_BADSHAPE;
    if (transpose != 0 && transpose != 1) return CVAE_E_UNSUPPORTED;
    if (any_null(L, in, out)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(L, in, row_shift, out)) return CVAE_E_UNSUPPORTED;
    if (in == out && (in_row_stride != ldo || in_col_stride != 1)) return CVAE_E_UNSUPPORTED;      // in place only element for element
    return with_bool(transpose != 0, [&](auto rev) {
        hipLaunchKernelGGL(trsm_kernel<decltype(rev)::value>, dim3((unsigned)((n + TR_COLS - 1) / TR_COLS)), dim3(TR_COLS), 0, (hipStream_t)stream, L, ldl, in,
                           in_row_stride, in_col_stride, row_shift, out, ldo, (int64_t)1, (int)d, n);
        return launch_rc();
    });
}

extern "C" int cvae_ridge_loo_f64(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, const double* W,
                                  const double* T, int64_t N, int64_t d, int64_t F, double* leverage, double* fitted, double* loo, double* coef, double* intercept,
                                  void* stream) {
    if (!ridge_shape_ok(N, d, F) || z_stride < d || m_stride < F) return CVAE_E_BADSHAPE;
    if (any_null(Z, z_mean, M, m_mean, W, T, leverage, fitted, loo, coef, intercept)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Z, z_mean, M, m_mean, W, T, leverage, fitted, loo, coef, intercept)) return CVAE_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ridge_leverage_kernel, dim3(blocks256(N)), dim3(256), 0, st, T, N, (int)d, leverage);
    hipLaunchKernelGGL(ridge_fit_kernel, dim3(blocks256(N * F)), dim3(256), 0, st, Z, z_stride, z_mean, M, m_stride, m_mean, W, (const double*)leverage, N, (int)d,
                       (int)F, fitted, loo);
    hipLaunchKernelGGL(ridge_coef_kernel, dim3(blocks256(F * d)), dim3(256), 0, st, W, z_mean, m_mean, (int)d, (int)F, coef, intercept);
    return launch_rc();
}

extern "C" int cvae_ridge_predict_f64(const double* Z, int64_t z_stride, const double* coef, const double* intercept, int64_t N, int64_t d, int64_t F, double* out,
                                      void* stream) {
    if (N < 0 || d < 1 || d > 1024 || !rows_features_ok(N, F) || z_stride < d) return CVAE_E_BADSHAPE;
    if (N == 0) return CVAE_OK;
    if (any_null(Z, coef, intercept, out)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Z, coef, intercept, out)) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(ridge_predict_kernel, dim3(blocks256(N * F)), dim3(256), 0, (hipStream_t)stream, Z, z_stride, coef, intercept, N, (int)d, (int)F, out);
    return launch_rc();
}

extern "C" int cvae_ranking_stats_f64(const double* Y, int64_t y_stride, const double* P, int64_t p_stride, int64_t N, int64_t F, double* r2, double* corr,
                                      void* stream) {
    if (N < 1 || !rows_features_ok(N, F) || y_stride < F || p_stride < F) return CVAE_E_BADSHAPE;
    if (any_null(Y, P, r2, corr)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Y, P, r2, corr)) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(ranking_stats_kernel, dim3((unsigned)F), dim3(256), 0, (hipStream_t)stream, Y, y_stride, P, p_stride, N, r2, corr);
    return launch_rc();
}

extern "C" int cvae_group_means_resampled_f64(const double* Z, int64_t z_stride, const int* codes, const int* idx, int64_t N, int64_t d, int64_t G, int64_t n_boot,
                                              double* out, int* counts, void* stream) {
    if (N < 1 || N >= RIDGE_MAX_ROWS || d < 1 || d > 65536 || G < 1 || G > 65535 || n_boot < 0 || n_boot > 65535 || z_stride < d) return CVAE_E_BADSHAPE;
    if (n_boot == 0) return CVAE_OK;
    if (any_null(Z, codes, idx, out, counts)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Z, out) || !all_aligned<4>(codes, idx, counts)) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(group_means_resampled_kernel, dim3((unsigned)((d + 63) / 64), (unsigned)G, (unsigned)n_boot), dim3(64), 0, (hipStream_t)stream, Z, z_stride, codes,
                       idx, N, (int)d, (int)G, out, counts);
    return launch_rc();
}

// ---- the alpha path and the latent PCA ----
extern "C" size_t cvae_centered_gram_f64_workspace_bytes(int64_t N, int64_t d, int64_t F) {
    if (!gram_shape_ok(N, d, F)) return 0;
    return gram_ws_bytes(N, d, F);
}
extern "C" int cvae_centered_gram_f64(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, int64_t N,
                                      int64_t d, int64_t F, double* G, double* R, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gram_shape_ok(N, d, F) || z_stride < d || (F > 0 && m_stride < F)) return CVAE_E_BADSHAPE;
    if (any_null(Z, z_mean, G, workspace) || (F > 0 && any_null(M, m_mean, R))) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Z, z_mean, G, workspace) || (F > 0 && !all_aligned<8>(M, m_mean, R))) return CVAE_E_UNSUPPORTED;
    return gram_launch(Z, z_stride, z_mean, M, m_stride, m_mean, N, d, F, 0.0, G, R, workspace, workspace_bytes, stream);
}

extern "C" int cvae_centered_matmul_f64(const double* x, int64_t x_row_stride, int64_t x_col_stride, const double* mean, const double* b, int64_t b_row_stride,
                                        int64_t b_col_stride, int64_t R, int64_t K, int64_t C, double* out, int64_t ldo, void* stream) {
    if (R < 1 || R >= RIDGE_MAX_ROWS || K < 1 || K > 1024 || C < 1 || C >= RIDGE_MAX_ROWS / 1024 || ldo < C || x_row_stride < 1 || x_col_stride < 1 ||
        b_row_stride < 1 || b_col_stride < 1)
        return CVAE_E_BADSHAPE;
    if (any_null(x, b, out)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(x, mean, b, out)) return CVAE_E_UNSUPPORTED;
    if (out == x || out == b) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(centered_matmul_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)((R + 63) / 64)), dim3(256), 0, (hipStream_t)stream, x, x_row_stride,
                       x_col_stride, mean, b, b_row_stride, b_col_stride, R, (int)K, C, out, ldo);
    return launch_rc();
}

extern "C" int cvae_ridge_path_f64(const double* P, const double* Q, const double* lambda, const double* alphas, const double* M, int64_t m_stride,
                                   const double* m_mean, int64_t N, int64_t d, int64_t F, int64_t G, double* eigenvalues, double* leverage, double* loo, double* sse,
                                   void* stream) {
    if (!ridge_shape_ok(N, d, F) || m_stride < F || G < 1 || G > 64) return CVAE_E_BADSHAPE;
    if (any_null(P, Q, lambda, alphas, M, m_mean, eigenvalues, leverage, loo, sse)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(P, Q, lambda, alphas, M, m_mean, eigenvalues, leverage, loo, sse)) return CVAE_E_UNSUPPORTED;
    if (eigenvalues == lambda) return CVAE_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ridge_path_leverage_kernel, dim3(blocks256(N), (unsigned)G), dim3(256), 0, st, P, lambda, alphas, N, (int)d, leverage, eigenvalues);
    hipLaunchKernelGGL(ridge_path_loo_kernel, dim3(blocks256(N * F), (unsigned)G), dim3(256), 0, st, P, Q, lambda, alphas, M, m_stride, m_mean,
                       (const double*)leverage, N, (int)d, (int)F, loo);
    hipLaunchKernelGGL(ridge_path_sse_kernel, dim3((unsigned)F, (unsigned)G), dim3(256), 0, st, M, m_stride, (const double*)loo, N, (int)F, sse);
    return launch_rc();
}

extern "C" int cvae_pca_components_f64(const double* w, const double* V, int64_t ldv, int64_t d, int64_t k, int64_t N, double* components,
                                       double* explained_variance, double* explained_variance_ratio, double* singular_values, void* stream) {
    if (d < 1 || d > 1024 || ldv < d || N < 2 || N >= RIDGE_MAX_ROWS || k < 1 || k > d || k > N - 1) return CVAE_E_BADSHAPE;
    if (any_null(w, V, components, explained_variance, explained_variance_ratio, singular_values)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(w, V, components, explained_variance, explained_variance_ratio, singular_values)) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(pca_components_kernel, dim3((unsigned)k), dim3(256), 0, (hipStream_t)stream, w, V, ldv, (int)d, N, components, explained_variance,
                       explained_variance_ratio, singular_values);
    return launch_rc();
}
