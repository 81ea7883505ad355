// tsne.hip — exact t-SNE in float64, two components, one degree of freedom: sklearn's method="exact" pipeline (_joint_probabilities,
// _kl_divergence, _gradient_descent, TSNE._tsne) for 3 <= N <= 4096 points.
//   distances    D[i][j] = sum_k (z_ik - z_jk)^2 from differences, k in index order, one fma per term: (i, j) and (j, i) run the same operations on negated
//                differences, so D is bitwise symmetric; the diagonal is written as 0
//   affinities   one workgroup per row: the row minus its off-diagonal minimum stays in LDS for the whole search; e_j = exp(-beta d'_j), S = sum e_j,
//                H = log S + beta (sum d'_j e_j) / S; sklearn's search for beta (from 1, doubling or halving until bracketed, then midpoints), at most
//                TSNE_SEARCH_STEPS steps, stopping at the first with |H - log perplexity| <= tol.  The trip count is bounded for every input.
//   joint        P = max((Pc + Pc^T) / s, 2^-52) off the diagonal, s the ordered sum of the 32 x 32 tile sums; a + b commutes, so P is bitwise symmetric
//   forces       per row i over j != i with w = 1 / (1 + |y_i - y_j|^2): S_i = sum w, A_i = sum P w (y_i - y_j), R_i = sum w^2 (y_i - y_j) and, when asked,
//                sum P log P, sum P log w, sum P.  TSNE_FORCE_ROWS rows per workgroup, the columns strided over its 256 threads, Y in LDS, P loaded one stride ahead.
//   update       Zs = sum S_i, grad = 4 (ex A - R / Zs), sklearn's gains / momentum step written to a second set of buffers (nothing is updated in place, so
//                workgroup 0 can recompute every row for the record: KL of the exaggerated P, |gains grad|^2, a non-finite flag, Zs)
//   fit          the host loop of TSNE._tsne: two launches per iteration; the host reads the record (4 doubles) at every multiple of 50 iterations and stops
//                launching.  NOT enqueue-only.
// No atomics, no workgroup waits on another.  Every sum: a thread's strided terms in index order, then common.h's butterfly (block_sum_f64, ordered_sum_f64:
// a 64-lane xor butterfly, the four waves in order); ordered finishes across workgroups.  Grids are functions of N alone: two runs give equal bits.
#include <float.h>
#include "common.h"

CVAE_TUNABLE(TSNE_FORCE_ROWS, 4);          // rows of the embedding per forces workgroup: N / 4 workgroups fill the chip at N = 2000 (profiles/tsne.md: 1, 2, 4, 8)

namespace {

constexpr int TSNE_MIN_N = 3, TSNE_MAX_N = 4096;
constexpr int TSNE_TILE = 32;                    // distances and the joint pass: 32 x 32 outputs per workgroup, four per thread
constexpr int TSNE_SEARCH_STEPS = 100;           // sklearn's n_steps
constexpr int TSNE_CHECK = 50, TSNE_EXPLORE = 250;          // sklearn's _N_ITER_CHECK and _EXPLORATION_MAX_ITER
constexpr double TSNE_EPS = 2.220446049250313e-16;          // 2^-52, sklearn's MACHINE_EPSILON
constexpr int FR = (int)TSNE_FORCE_ROWS;
static_assert(FR >= 1 && FR <= 8, "TSNE_FORCE_ROWS: 1 .. 8");
enum { REC_KL = 0, REC_GN2 = 1, REC_BAD = 2, REC_ZS = 3, REC_WORDS = 4 };

// ---- distances ----
template <typename T> __global__ __launch_bounds__(256) void tsne_sqdist_kernel(const T* __restrict__ Z, int64_t ldz, int N, int d, double* __restrict__ D) {
    __shared__ double zi[TSNE_TILE][TSNE_TILE + 1], zj[TSNE_TILE][TSNE_TILE + 1];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int i0 = blockIdx.y * TSNE_TILE, j0 = blockIdx.x * TSNE_TILE;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int k0 = 0; k0 < d; k0 += TSNE_TILE) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q, r = e >> 5, c = e & 31, k = k0 + c;
            zi[r][c] = (i0 + r < N && k < d) ? (double)Z[(size_t)(i0 + r) * ldz + k] : 0.0;          // a zero pad adds fma(0, 0, acc) = acc
            zj[r][c] = (j0 + r < N && k < d) ? (double)Z[(size_t)(j0 + r) * ldz + k] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < TSNE_TILE; ++c) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double diff = zi[ty + 16 * a][c] - zj[tx + 16 * b][c];
                    acc[a][b] = __builtin_fma(diff, diff, acc[a][b]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < N && j < N) D[(size_t)i * N + j] = (i == j) ? 0.0 : acc[a][b];
        }
}

// ---- conditional affinities: one workgroup per row.  Thread t only ever touches the columns j = t mod 256 of the LDS row, so the row needs no barrier. ----
__global__ __launch_bounds__(256) void tsne_affinities_kernel(const double* __restrict__ D, int N, double log_perplexity, double tol, double* __restrict__ Pc,
                                                              double* __restrict__ beta_out, int* __restrict__ steps_out) {
    extern __shared__ double tsne_row[];
    __shared__ double red[8];
    const int t = threadIdx.x, i = blockIdx.x;
    const double* drow = D + (size_t)i * N;
    double mn = __builtin_inf();
    for (int j = t; j < N; j += 256) {
        const double v = drow[j];
        tsne_row[j] = v;
        if (j != i) mn = fmin(mn, v);
    }
    mn = wave_min_f64(mn);
    if ((t & 63) == 0) red[t >> 6] = mn;
    __syncthreads();
    mn = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    for (int j = t; j < N; j += 256) tsne_row[j] -= mn;
    double beta = 1.0, lo = -__builtin_inf(), hi = __builtin_inf(), be = 1.0, S = 1.0;
    int steps = 0;
    for (int step = 0; step < TSNE_SEARCH_STEPS; ++step) {          // every thread holds the same bits of beta, lo, hi, H: the exit is uniform
        be = beta;
        double v[2] = {0.0, 0.0};
        for (int j = t; j < N; j += 256) {
            if (j == i) continue;
            const double dj = tsne_row[j], e = exp(-be * dj);
            v[0] += e;
            v[1] = __builtin_fma(dj, e, v[1]);
        }
        block_sum_f64(v, red);
        S = v[0];
        const double diff = (log(S) + be * v[1] / S) - log_perplexity;
        steps = step + 1;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            lo = be;
            beta = (hi == __builtin_inf()) ? be * 2.0 : (be + hi) * 0.5;
        } else {
            hi = be;
            beta = (lo == -__builtin_inf()) ? be * 0.5 : (be + lo) * 0.5;
        }
    }
    double* prow = Pc + (size_t)i * N;
    for (int j = t; j < N; j += 256) prow[j] = (j == i) ? 0.0 : exp(-be * tsne_row[j]) / S;
    if (t == 0) {
        beta_out[i] = be;
        steps_out[i] = steps;
    }
}

// ---- joint affinities ----
// tile (by, bx): V[i][j] = Pc[i][j] + Pc[j][i], the transposed operand through LDS; the tile's sum (NaN where an entry of D, Pc or V is not finite)
__global__ __launch_bounds__(256) void tsne_joint_sum_kernel(const double* __restrict__ D, const double* __restrict__ Pc, int N, double* __restrict__ V,
                                                             double* __restrict__ part) {
    __shared__ double tb[TSNE_TILE][TSNE_TILE + 1];
    __shared__ double red[4];
    const int t = threadIdx.x;
    const int i0 = blockIdx.y * TSNE_TILE, j0 = blockIdx.x * TSNE_TILE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + 256 * q, r = e >> 5, c = e & 31;
        tb[r][c] = (j0 + r < N && i0 + c < N) ? Pc[(size_t)(j0 + r) * N + i0 + c] : 0.0;
    }
    __syncthreads();
    double s[1] = {0.0};
    int bad = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + 256 * q, r = e >> 5, c = e & 31, i = i0 + r, j = j0 + c;
        if (i < N && j < N) {
            const double a = Pc[(size_t)i * N + j], v = a + tb[c][r];
            bad |= (finite_f64(D[(size_t)i * N + j]) && finite_f64(a) && finite_f64(v)) ? 0 : 1;
            V[(size_t)i * N + j] = v;
            s[0] += v;
        }
    }
    bad = __syncthreads_or(bad);
    block_sum_f64(s, red);
    if (t == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = bad ? __builtin_nan("") : s[0];
}
// one workgroup: the tile sums in order -> s; info[0] = 2 unless it is finite and positive
__global__ __launch_bounds__(256) void tsne_joint_finish_kernel(const double* __restrict__ part, int parts, double* __restrict__ total, int* __restrict__ info) {
    __shared__ double red[4];
    const double s = ordered_sum_f64(part, parts, red);
    if (threadIdx.x == 0) {
        *total = s;
        info[0] = (finite_f64(s) && s > 0.0) ? 0 : 2;
    }
}
__global__ __launch_bounds__(256) void tsne_joint_scale_kernel(double* __restrict__ P, int N, const double* __restrict__ total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * N) return;
    const int i = (int)(e / N), j = (int)(e % N);
    P[e] = (i == j) ? 0.0 : fmax(P[e] / *total, TSNE_EPS);
}

// ---- forces: the pair pass ----
template <bool KL> __global__ __launch_bounds__(256) void tsne_forces_kernel(const double* __restrict__ Y, const double* __restrict__ P, int N,
                                                                             double* __restrict__ A, double* __restrict__ R, double* __restrict__ S,
                                                                             double* __restrict__ klp) {
    constexpr int NV = KL ? 8 : 5;
    extern __shared__ double tsne_y[];          // x [N], y [N]
    __shared__ double red[4 * FR * NV];
    double* yx = tsne_y;
    double* yy = tsne_y + N;
    const int t = threadIdx.x, i0 = blockIdx.x * FR;
    for (int j = t; j < N; j += 256) {
        yx[j] = Y[2 * j];
        yy[j] = Y[2 * j + 1];
    }
    __syncthreads();
    int row[FR];
    double xi[FR], yi[FR], acc[FR * NV];
#pragma unroll
    for (int r = 0; r < FR; ++r) {
        row[r] = (i0 + r < N) ? i0 + r : N - 1;          // a row past the end repeats the last one and is not written
        xi[r] = yx[row[r]];
        yi[r] = yy[row[r]];
    }
#pragma unroll
    for (int k = 0; k < FR * NV; ++k) acc[k] = 0.0;
    double pcur[FR];          // this stride's P, loaded one stride ahead: the loads of the next stride are in flight under this one's arithmetic
#pragma unroll
    for (int r = 0; r < FR; ++r) pcur[r] = (t < N) ? P[(size_t)row[r] * N + t] : 0.0;
    for (int j = t; j < N; j += 256) {
        const double xj = yx[j], yj = yy[j];
        const int jn = j + 256;
        double pnext[FR];
#pragma unroll
        for (int r = 0; r < FR; ++r) pnext[r] = (jn < N) ? P[(size_t)row[r] * N + jn] : 0.0;
#pragma unroll
        for (int r = 0; r < FR; ++r) {
            const double p = pcur[r];
            pcur[r] = pnext[r];
            if (j == row[r]) continue;
            const double dx = xi[r] - xj, dy = yi[r] - yj;
            const double w = 1.0 / (1.0 + __builtin_fma(dx, dx, dy * dy));
            const double pw = p * w, ww = w * w;
            double* a = acc + r * NV;
            a[0] += w;
            a[1] = __builtin_fma(pw, dx, a[1]);
            a[2] = __builtin_fma(pw, dy, a[2]);
            a[3] = __builtin_fma(ww, dx, a[3]);
            a[4] = __builtin_fma(ww, dy, a[4]);
            if (KL) {
                a[5] = __builtin_fma(p, log(p), a[5]);
                a[6] = __builtin_fma(p, log(w), a[6]);
                a[7] += p;
            }
        }
    }
    block_sum_f64(acc, red);
    if (t < FR && i0 + t < N) {
        const int i = i0 + t;
        const double* a = acc;          // every thread holds every sum; thread t writes row t's
#pragma unroll
        for (int r = 0; r < FR; ++r)
            if (r == t) {
                S[i] = a[r * NV];
                A[2 * i] = a[r * NV + 1];
                A[2 * i + 1] = a[r * NV + 2];
                R[2 * i] = a[r * NV + 3];
                R[2 * i + 1] = a[r * NV + 4];
                if (KL) {
                    klp[i] = a[r * NV + 5];
                    klp[N + i] = a[r * NV + 6];
                    klp[2 * N + i] = a[r * NV + 7];
                }
            }
    }
}

// KL of the exaggerated P from the row partials klp = (sum P log P [N], sum P log w [N], sum P [N]): ex (sum P log P + (log ex + log Zs) sum P - sum P log w)
__device__ __forceinline__ double tsne_kl(const double* __restrict__ klp, int N, double ex, double Zs, double* red) {
    const double a = ordered_sum_f64(klp, N, red), b = ordered_sum_f64(klp + N, N, red), c = ordered_sum_f64(klp + 2 * N, N, red);
    return ex * ((a + (log(ex) + log(Zs)) * c) - b);
}
__device__ __forceinline__ double tsne_grad(double a, double r, double ex, double Zs) { return 4.0 * (ex * a - r / Zs); }

// grad [N][2] and, from workgroup 0 when kl is not null, the KL
__global__ __launch_bounds__(256) void tsne_grad_kernel(const double* __restrict__ A, const double* __restrict__ R, const double* __restrict__ S,
                                                        const double* __restrict__ klp, int N, double ex, double* __restrict__ grad, double* __restrict__ kl) {
    __shared__ double red[4];
    const double Zs = ordered_sum_f64(S, N, red);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < 2 * N) grad[e] = tsne_grad(A[e], R[e], ex, Zs);
    if (blockIdx.x == 0 && kl) {
        const double v = tsne_kl(klp, N, ex, Zs, red);
        if (threadIdx.x == 0) *kl = v;
    }
}

struct tsne_elem { double y, u, g, gg; };
// sklearn's _gradient_descent on one element: gains, the update, the position, and gains grad
__device__ __forceinline__ tsne_elem tsne_step_elem(double y, double u, double g, double grad, double momentum, double lr) {
    g = (u * grad < 0.0) ? g + 0.2 : g * 0.8;
    g = (g < 0.01) ? 0.01 : g;
    const double gg = g * grad;
    tsne_elem o;
    o.g = g;
    o.gg = gg;
    o.u = momentum * u - lr * gg;
    o.y = y + o.u;
    return o;
}
// one element per thread, written to the out buffers; with a record, workgroup 0 also walks every element again (the same arithmetic on the same inputs,
// which nothing overwrites) for |gains grad|^2 and the non-finite flag, and assembles the KL
__global__ __launch_bounds__(256) void tsne_update_kernel(const double* __restrict__ Yin, const double* __restrict__ Uin, const double* __restrict__ Gin,
                                                          const double* __restrict__ A, const double* __restrict__ R, const double* __restrict__ S,
                                                          const double* __restrict__ klp, int N, double ex, double momentum, double lr, double* __restrict__ Yout,
                                                          double* __restrict__ Uout, double* __restrict__ Gout, double* __restrict__ rec) {
    __shared__ double red[4];
    const double Zs = ordered_sum_f64(S, N, red);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < 2 * N) {
        const tsne_elem o = tsne_step_elem(Yin[e], Uin[e], Gin[e], tsne_grad(A[e], R[e], ex, Zs), momentum, lr);
        Yout[e] = o.y;
        Uout[e] = o.u;
        Gout[e] = o.g;
    }
    if (blockIdx.x != 0 || !rec) return;
    double v[1] = {0.0};
    int bad = 0;
    for (int k = threadIdx.x; k < 2 * N; k += 256) {
        const tsne_elem o = tsne_step_elem(Yin[k], Uin[k], Gin[k], tsne_grad(A[k], R[k], ex, Zs), momentum, lr);
        v[0] = __builtin_fma(o.gg, o.gg, v[0]);
        bad |= finite_f64(o.y) ? 0 : 1;
    }
    bad = __syncthreads_or(bad);
    block_sum_f64(v, red);
    const double kl = tsne_kl(klp, N, ex, Zs, red);
    if (threadIdx.x == 0) {
        rec[REC_KL] = kl;
        rec[REC_GN2] = v[0];
        rec[REC_BAD] = (bad || !finite_f64(kl) || !finite_f64(v[0])) ? 1.0 : 0.0;
        rec[REC_ZS] = Zs;
    }
}

// ---- the fit's first and last launches ----
__global__ __launch_bounds__(256) void tsne_fit_init_kernel(const double* __restrict__ Y, int N, double* __restrict__ y0, double* __restrict__ u0, double* __restrict__ g0) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * N) return;
    y0[e] = Y[e];
    u0[e] = 0.0;
    g0[e] = 1.0;
}
// one workgroup: Y out, the KL of P itself (exaggeration 1) at it, info = (status, the last iteration's index, why it stopped, how many records were read)
__global__ __launch_bounds__(256) void tsne_fit_end_kernel(const double* __restrict__ y, const double* __restrict__ S, const double* __restrict__ klp, int N,
                                                           int status, int last_iter, int reason, int checks, double* __restrict__ Y, double* __restrict__ kl,
                                                           int* __restrict__ info) {
    __shared__ double red[4];
    int bad = 0;
    for (int k = threadIdx.x; k < 2 * N; k += 256) {
        const double v = y[k];
        Y[k] = v;
        bad |= finite_f64(v) ? 0 : 1;
    }
    bad = __syncthreads_or(bad);
    const double Zs = ordered_sum_f64(S, N, red);
    const double v = tsne_kl(klp, N, 1.0, Zs, red);
    if (threadIdx.x == 0) {
        *kl = v;
        info[0] = (status != 0) ? status : ((bad || !finite_f64(v)) ? 2 : 0);
        info[1] = last_iter;
        info[2] = reason;
        info[3] = checks;
    }
}

inline bool tsne_n_ok(int64_t N) { return N >= TSNE_MIN_N && N <= TSNE_MAX_N; }
inline unsigned tsne_tiles(int64_t N) { return (unsigned)((N + TSNE_TILE - 1) / TSNE_TILE); }
inline unsigned tsne_elem_blocks(int64_t N) { return (unsigned)((2 * N + 255) / 256); }

// the launches behind the entries, every argument already checked
int launch_forces(const double* Y, const double* P, int N, double* A, double* R, double* S, double* klp, hipStream_t st) {
    const size_t lds = (size_t)2 * N * sizeof(double);
    const unsigned grid = (unsigned)((N + FR - 1) / FR);
    return with_bool(klp != nullptr, [&](auto kl) {
        constexpr bool KL = decltype(kl)::value;
        if (cvae_allow_lds<tsne_forces_kernel<KL>>(lds, 4 * FR * (KL ? 8 : 5) * sizeof(double)) != CVAE_OK) return (int)CVAE_E_LAUNCH;
        hipLaunchKernelGGL(tsne_forces_kernel<KL>, dim3(grid), dim3(256), lds, st, Y, P, N, A, R, S, klp);
        return (int)CVAE_OK;
    });
}
void launch_update(const double* Yin, const double* Uin, const double* Gin, const double* A, const double* R, const double* S, const double* klp, int N, double ex,
                   double momentum, double lr, double* Yout, double* Uout, double* Gout, double* rec, hipStream_t st) {
    hipLaunchKernelGGL(tsne_update_kernel, dim3(tsne_elem_blocks(N)), dim3(256), 0, st, Yin, Uin, Gin, A, R, S, klp, N, ex, momentum, lr, Yout, Uout, Gout, rec);
}

struct tsne_fit_layout {
    size_t y[2], u[2], g[2], a, r, s, klp, rec, bytes;
};
tsne_fit_layout tsne_fit_plan(int64_t N) {
    tsne_fit_layout L;
    const size_t n2 = (size_t)2 * N * sizeof(double), n1 = (size_t)N * sizeof(double);
    size_t o = 0;
    for (int b = 0; b < 2; ++b) {
        L.y[b] = o; o += n2;
        L.u[b] = o; o += n2;
        L.g[b] = o; o += n2;
    }
    L.a = o; o += n2;
    L.r = o; o += n2;
    L.s = o; o += n1;
    L.klp = o; o += 3 * n1;
    L.rec = o; o += REC_WORDS * sizeof(double);
    L.bytes = o;
    return L;
}

}  // namespace

extern "C" int cvae_tsne_sqdist_f64(const void* Z, int z_is_f32, int64_t z_stride, int64_t N, int64_t d, double* D, void* stream) {
    if (!tsne_n_ok(N) || d < 1 || d > INT32_MAX || z_stride < d) return CVAE_E_BADSHAPE;
    if (any_null(Z, D)) return CVAE_E_NULLPTR;
    if (!(z_is_f32 ? aligned4(Z) : aligned8(Z)) || !aligned8(D)) return CVAE_E_UNSUPPORTED;
    const dim3 grid(tsne_tiles(N), tsne_tiles(N));
    if (z_is_f32) hipLaunchKernelGGL(tsne_sqdist_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)Z, z_stride, (int)N, (int)d, D);
    else hipLaunchKernelGGL(tsne_sqdist_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)Z, z_stride, (int)N, (int)d, D);
    return launch_rc();
}

extern "C" int cvae_tsne_affinities_f64(const double* D, int64_t N, double perplexity, double tol, double* Pc, double* beta, int* steps, void* stream) {
    if (!tsne_n_ok(N) || !(perplexity > 0.0 && perplexity < (double)N) || !(tol >= 0.0)) return CVAE_E_BADSHAPE;
    if (any_null(D, Pc, beta, steps)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(D, Pc, beta) || !aligned4(steps) || D == Pc) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3((unsigned)N), dim3(256), (size_t)N * sizeof(double), (hipStream_t)stream, D, (int)N, log(perplexity), tol, Pc,
                       beta, steps);
    return launch_rc();
}

extern "C" size_t cvae_tsne_joint_f64_workspace_bytes(int64_t N) {
    if (!tsne_n_ok(N)) return 0;
    return ((size_t)tsne_tiles(N) * tsne_tiles(N) + 1) * sizeof(double);
}

extern "C" int cvae_tsne_joint_f64(const double* D, const double* Pc, int64_t N, double* P, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (!tsne_n_ok(N)) return CVAE_E_BADSHAPE;
    if (any_null(D, Pc, P, info, workspace)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(D, Pc, P, workspace) || !aligned4(info) || P == Pc || P == D) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_tsne_joint_f64_workspace_bytes(N)) return CVAE_E_WORKSPACE;
    const unsigned T = tsne_tiles(N);
    double* part = (double*)workspace;
    double* total = part + (size_t)T * T;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsne_joint_sum_kernel, dim3(T, T), dim3(256), 0, st, D, Pc, (int)N, P, part);
    hipLaunchKernelGGL(tsne_joint_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, (int)(T * T), total, info);
    hipLaunchKernelGGL(tsne_joint_scale_kernel, dim3((unsigned)((N * N + 255) / 256)), dim3(256), 0, st, P, (int)N, (const double*)total);
    return launch_rc();
}

extern "C" int cvae_tsne_forces_f64(const double* Y, const double* P, int64_t N, double* A, double* R, double* S, double* kl_partials, void* stream) {
    if (!tsne_n_ok(N)) return CVAE_E_BADSHAPE;
    if (any_null(Y, P, A, R, S)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Y, P, A, R, S, kl_partials)) return CVAE_E_UNSUPPORTED;
    const int rc = launch_forces(Y, P, (int)N, A, R, S, kl_partials, (hipStream_t)stream);
    return rc != CVAE_OK ? rc : launch_rc();
}

extern "C" int cvae_tsne_grad_f64(const double* A, const double* R, const double* S, const double* kl_partials, int64_t N, double exaggeration, double* grad,
                                  double* kl, void* stream) {
    if (!tsne_n_ok(N) || !(exaggeration > 0.0)) return CVAE_E_BADSHAPE;
    if (any_null(A, R, S, grad) || (kl && !kl_partials)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(A, R, S, kl_partials, grad, kl)) return CVAE_E_UNSUPPORTED;
    hipLaunchKernelGGL(tsne_grad_kernel, dim3(tsne_elem_blocks(N)), dim3(256), 0, (hipStream_t)stream, A, R, S, kl_partials, (int)N, exaggeration, grad, kl);
    return launch_rc();
}

extern "C" int cvae_tsne_update_f64(const double* Y, const double* update, const double* gains, const double* A, const double* R, const double* S,
                                    const double* kl_partials, int64_t N, double exaggeration, double momentum, double learning_rate, double* Y_out,
                                    double* update_out, double* gains_out, double* record, void* stream) {
    if (!tsne_n_ok(N) || !(exaggeration > 0.0)) return CVAE_E_BADSHAPE;
    if (any_null(Y, update, gains, A, R, S, Y_out, update_out, gains_out) || (record && !kl_partials)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(Y, update, gains, A, R, S, kl_partials, Y_out, update_out, gains_out, record)) return CVAE_E_UNSUPPORTED;
    if (Y_out == Y || update_out == update || gains_out == gains) return CVAE_E_UNSUPPORTED;
    launch_update(Y, update, gains, A, R, S, kl_partials, (int)N, exaggeration, momentum, learning_rate, Y_out, update_out, gains_out, record, (hipStream_t)stream);
    return launch_rc();
}

extern "C" size_t cvae_tsne_fit_f64_workspace_bytes(int64_t N) {
    if (!tsne_n_ok(N)) return 0;
    return tsne_fit_plan(N).bytes;
}

extern "C" int cvae_tsne_fit_f64(const double* P, double* Y, int64_t N, double early_exaggeration, double learning_rate, int64_t max_iter,
                                 int64_t n_iter_without_progress, double min_grad_norm, double* kl, int* info, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!tsne_n_ok(N) || !(early_exaggeration > 0.0) || !(learning_rate > 0.0) || max_iter < 0 || max_iter > INT32_MAX || n_iter_without_progress < 0)
        return CVAE_E_BADSHAPE;
    if (any_null(P, Y, kl, info, workspace)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(P, Y, kl, workspace) || !aligned4(info)) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_tsne_fit_f64_workspace_bytes(N)) return CVAE_E_WORKSPACE;
    const tsne_fit_layout L = tsne_fit_plan(N);
    char* base = (char*)workspace;
    double *y[2], *u[2], *g[2];
    for (int b = 0; b < 2; ++b) {
        y[b] = (double*)(base + L.y[b]);
        u[b] = (double*)(base + L.u[b]);
        g[b] = (double*)(base + L.g[b]);
    }
    double *A = (double*)(base + L.a), *R = (double*)(base + L.r), *S = (double*)(base + L.s), *klp = (double*)(base + L.klp), *rec = (double*)(base + L.rec);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)N;
    hipLaunchKernelGGL(tsne_fit_init_kernel, dim3(tsne_elem_blocks(N)), dim3(256), 0, st, (const double*)Y, n, y[0], u[0], g[0]);
    CVAE_CHECK_LAUNCH();
    int cur = 0, status = 0, reason = 0, checks = 0;          // reason: 0 the iterations ran out, 1 the gradient norm, 2 no progress (in the second phase)
    int64_t last = 0, next = 0;
    bool stop = false;
    for (int phase = 0; phase < 2 && !stop; ++phase) {
        const double ex = phase == 0 ? early_exaggeration : 1.0, momentum = phase == 0 ? 0.5 : 0.8;
        const int64_t end = phase == 0 ? (max_iter < TSNE_EXPLORE ? max_iter : TSNE_EXPLORE) : max_iter;
        const int64_t limit = phase == 0 ? TSNE_EXPLORE : n_iter_without_progress;
        double best = DBL_MAX;
        int64_t best_iter = next;
        for (int64_t i = next; i < end; ++i) {
            const bool check = (i + 1) % TSNE_CHECK == 0, want = check || i == end - 1;
            const int rc = launch_forces(y[cur], P, n, A, R, S, want ? klp : nullptr, st);
            if (rc != CVAE_OK) return rc;
            launch_update(y[cur], u[cur], g[cur], A, R, S, klp, n, ex, momentum, learning_rate, y[cur ^ 1], u[cur ^ 1], g[cur ^ 1], want ? rec : nullptr, st);
            CVAE_CHECK_LAUNCH();
            cur ^= 1;
            last = i;
            next = i + 1;
            if (!check) continue;
            double h[REC_WORDS];          // the one read: this iteration's KL, |gains grad|^2, the non-finite flag, Zs
            if (hipMemcpyAsync(h, rec, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return CVAE_E_LAUNCH;
            ++checks;
            if (h[REC_BAD] != 0.0) { status = 2; stop = true; break; }
            if (h[REC_KL] < best) { best = h[REC_KL]; best_iter = i; }
            else if (i - best_iter > limit) { if (phase == 1) reason = 2; break; }          // sklearn's order: progress first, then the norm
            if (sqrt(h[REC_GN2]) <= min_grad_norm) { reason = 1; stop = true; break; }
        }
    }
    const int rc = launch_forces(y[cur], P, n, A, R, S, klp, st);
    if (rc != CVAE_OK) return rc;
    hipLaunchKernelGGL(tsne_fit_end_kernel, dim3(1), dim3(256), 0, st, (const double*)y[cur], (const double*)S, (const double*)klp, n, status, (int)last, reason,
                       checks, Y, kl, info);
    return launch_rc();
}
