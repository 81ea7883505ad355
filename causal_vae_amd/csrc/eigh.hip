// eigh.hip — cvae_eigh_f64: the eigendecomposition A = V diag(w) V^T of a symmetric float64 matrix, n <= 1024, for the ridge alpha path
// and the latent PCA.  A two-sided Jacobi method in the round-robin (tournament) order: with m = n rounded up to even, a sweep is m - 1 rounds of m / 2 disjoint
// pairs (p, q); in round r the pairs are (m - 1, r) and ((r + k) mod (m - 1), (r - k) mod (m - 1)) for k = 1 .. m / 2 - 1.  An odd n has a bye: the pair whose
// second index is n rotates by the identity.  Every pair of a round rotates in the same launch: the m / 2 pairs cut the matrix into 2 x 2 blocks
// B = A[{p, q}][{p', q'}], and the round maps each block to J_k^T B J_k' on its own, reading the matrix of the round before and writing the next one (two
// buffers, so no thread reads what another writes).  The same thread turns the rows p, q of V by J_k' alone.
//   rotation     zeta = (a_qq - a_pp) / (2 a_pq), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t (Rutishauser's form: the smaller
//                angle).  An a_pq of 0 or a t that is not finite rotates by the identity.  A zeta that overflows gives t = 0, which is its limit.
//   on the diagonal block   a_pp -= t a_pq, a_qq += t a_pq, a_pq = a_qp = 0 exactly
//   symmetry     block (k, k') with k < k' turns its rows first, block (k', k) its columns first: the two do the same operations on transposed operands, every
//                product-sum an explicit fma, so the matrix stays bitwise symmetric
//   convergence  every rotation's |a_pq| (before it) is maximised per diagonal tile by the one workgroup that owns the tile; a launch at the end of the sweep
//                reduces the tiles, and the sweep in which no |a_pq| exceeded 2^-53 max |A| is the last.  The host reads that one word after every sweep (never
//                inside one) and stops launching; EIGH_MAX_SWEEPS bounds the loop.  No kernel has a loop whose trip count depends on data.
//   sort         ascending by rank counting in one workgroup, ties by original index; a gather launch permutes the columns of V
// No float atomics, no workgroup waits on another, every grid and the pair order are functions of n alone: two runs give equal bits.  The only reductions
// are maxima (common.h's block_tree at the start, plain loops in one thread after that), whose result no order can change.
#include "common.h"

namespace {

constexpr int EIGH_MAX_N = 1024;
constexpr int EIGH_MAX_SWEEPS = 48;          // the sweep cap: cyclic Jacobi needs about log2(n) + 3 sweeps, 13 at n = 1024
constexpr int EIGH_TILE = 16;                // a workgroup owns 16 x 16 pair blocks, one per thread
constexpr double EIGH_U = 1.1102230246251565e-16;          // 2^-53
enum { ST_DONE = 0, ST_INFO = 1, ST_SWEEPS = 2, ST_WORDS = 4 };

struct eigh_layout {
    size_t a[2], v[2], part, off, tol, perm, state, bytes;          // offsets in bytes
};
eigh_layout eigh_plan(int64_t n) {
    eigh_layout L;
    const size_t nn = (size_t)n * n * sizeof(double);
    size_t o = 0;
    L.a[0] = o; o += nn;
    L.a[1] = o; o += nn;
    L.v[0] = o; o += nn;
    L.v[1] = o; o += nn;
    L.part = o; o += (size_t)((n * n + 255) / 256) * sizeof(double);
    L.off = o; o += (size_t)(EIGH_MAX_N / 2 / EIGH_TILE) * sizeof(double);
    L.tol = o; o += sizeof(double);
    L.perm = o; o += (size_t)EIGH_MAX_N * sizeof(int);
    L.state = o; o += ST_WORDS * sizeof(int);
    L.bytes = o;
    return L;
}

struct MaxF64 {          // block_tree's op for the two maxima
    __device__ __forceinline__ double operator()(double a, double b) const { return b > a ? b : a; }
};

// (x, y) -> (c x - s y, s x + c y)
__device__ __forceinline__ void rot2(double x, double y, double c, double s, double& lo, double& hi) {
    const double sy = s * y, cy = c * y;
    lo = __builtin_fma(c, x, -sy);
    hi = __builtin_fma(s, x, cy);
}

// the lower triangle of A mirrored into a0, v0 = I, and per workgroup the largest |a| (infinity where an entry is not finite)
__global__ __launch_bounds__(256) void eigh_init_kernel(const double* __restrict__ A, int64_t lda, int n, double* __restrict__ a0, double* __restrict__ v0,
                                                        double* __restrict__ part) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * 256 + t;
    double m = 0.0;
    if (e < (int64_t)n * n) {
        const int i = (int)(e / n), j = (int)(e % n);
        const double a = A[(size_t)(i > j ? i : j) * lda + (i > j ? j : i)];
        a0[e] = a;
        v0[e] = (i == j) ? 1.0 : 0.0;
        m = finite_f64(a) ? fabs(a) : __builtin_inf();
    }
    m = block_tree<256>(m, red, MaxF64{});
    if (t == 0) part[blockIdx.x] = m;
}
// one workgroup: the threshold 2^-53 max |A|, the state words, the per-tile maxima cleared.  A non-finite entry ends the run here (info 2).
__global__ __launch_bounds__(256) void eigh_setup_kernel(const double* __restrict__ part, int parts, double* __restrict__ off, double* __restrict__ tol,
                                                         int* __restrict__ state) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double m = 0.0;
    for (int g = t; g < parts; g += 256) m = part[g] > m ? part[g] : m;
    m = block_tree<256>(m, red, MaxF64{});
    if (t < EIGH_MAX_N / 2 / EIGH_TILE) off[t] = 0.0;
    if (t == 0) {
        const bool bad = !finite_f64(m);
        *tol = EIGH_U * m;
        state[ST_DONE] = bad ? 1 : 0;
        state[ST_INFO] = bad ? 2 : 0;
        state[ST_SWEEPS] = 0;
    }
}

// One round.  grid (T, T) with T = ceil(m / 2 / 16): workgroup (bx, by) owns the pair blocks (row pair by 16 + ty, column pair bx 16 + tx).  Its first 32
// threads work out the 16 + 16 rotations it needs from the matrix of the round before (every workgroup of a tile row does the same arithmetic on the same
// three numbers, so all agree).
__global__ __launch_bounds__(256) void eigh_round_kernel(const double* __restrict__ ain, double* __restrict__ aout, const double* __restrict__ vin,
                                                         double* __restrict__ vout, int n, int round, const int* __restrict__ state, double* __restrict__ off) {
    if (state[ST_DONE]) return;
    __shared__ double rc[2 * EIGH_TILE], rs[2 * EIGH_TILE], rt[2 * EIGH_TILE], ro[EIGH_TILE];
    __shared__ int rp[2 * EIGH_TILE], rq[2 * EIGH_TILE];
    const int t = threadIdx.x, m = n + (n & 1), h = m / 2;
    if (t < 2 * EIGH_TILE) {
        const int k = (t < EIGH_TILE) ? blockIdx.y * EIGH_TILE + t : blockIdx.x * EIGH_TILE + (t - EIGH_TILE);
        int p = -1, q = -1;
        double c = 1.0, s = 0.0, tt = 0.0, o = 0.0;
        if (k < h) {
            const int a = (k == 0) ? m - 1 : (round + k) % (m - 1), b = (k == 0) ? round : (round - k + (m - 1)) % (m - 1);
            p = a < b ? a : b;
            q = a < b ? b : a;
            if (q < n) {
                const double app = ain[(size_t)p * n + p], aqq = ain[(size_t)q * n + q], apq = ain[(size_t)p * n + q];
                o = fabs(apq);
                if (apq != 0.0) {
                    const double zeta = (aqq - app) / (2.0 * apq);
                    const double t1 = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c1 = 1.0 / sqrt(1.0 + t1 * t1), s1 = c1 * t1;
                    if (finite_f64(t1) && finite_f64(c1) && finite_f64(s1)) { tt = t1; c = c1; s = s1; }
                }
            }
        }
        rp[t] = p; rq[t] = q; rc[t] = c; rs[t] = s; rt[t] = tt;
        if (t < EIGH_TILE) ro[t] = o;
    }
    __syncthreads();
    if (blockIdx.x == blockIdx.y && t == 0) {          // this tile's pairs are visited by this workgroup alone, launch after launch: a plain read-modify-write
        double mx = off[blockIdx.x];
        for (int i = 0; i < EIGH_TILE; ++i) mx = ro[i] > mx ? ro[i] : mx;
        off[blockIdx.x] = mx;
    }
    const int ty = t >> 4, tx = t & 15;
    const int k = blockIdx.y * EIGH_TILE + ty, k2 = blockIdx.x * EIGH_TILE + tx;
    if (k >= h || k2 >= h) return;
    const int p = rp[ty], q = rq[ty], p2 = rp[EIGH_TILE + tx], q2 = rq[EIGH_TILE + tx];
    const double c1 = rc[ty], s1 = rs[ty], c2 = rc[EIGH_TILE + tx], s2 = rs[EIGH_TILE + tx];
    const bool hq = q < n, hq2 = q2 < n;
    const double b00 = ain[(size_t)p * n + p2], b01 = hq2 ? ain[(size_t)p * n + q2] : 0.0;
    const double b10 = hq ? ain[(size_t)q * n + p2] : 0.0, b11 = (hq && hq2) ? ain[(size_t)q * n + q2] : 0.0;
    double n00, n01, n10, n11;
    if (k == k2) {
        const double d = rt[ty] * b01;
        n00 = b00 - d; n11 = b11 + d; n01 = 0.0; n10 = 0.0;
    } else if (k < k2) {          // rows by J_k, then columns by J_k2
        double r00, r10, r01, r11;
        rot2(b00, b10, c1, s1, r00, r10);
        rot2(b01, b11, c1, s1, r01, r11);
        rot2(r00, r01, c2, s2, n00, n01);
        rot2(r10, r11, c2, s2, n10, n11);
    } else {                      // columns by J_k2, then rows by J_k: block (k2, k)'s operations on the transposed block
        double r00, r01, r10, r11;
        rot2(b00, b01, c2, s2, r00, r01);
        rot2(b10, b11, c2, s2, r10, r11);
        rot2(r00, r10, c1, s1, n00, n10);
        rot2(r01, r11, c1, s1, n01, n11);
    }
    aout[(size_t)p * n + p2] = n00;
    if (hq2) aout[(size_t)p * n + q2] = n01;
    if (hq) aout[(size_t)q * n + p2] = n10;
    if (hq && hq2) aout[(size_t)q * n + q2] = n11;
    // V's rows p and q, columns (p2, q2)
    double lo, hi;
    rot2(vin[(size_t)p * n + p2], hq2 ? vin[(size_t)p * n + q2] : 0.0, c2, s2, lo, hi);
    vout[(size_t)p * n + p2] = lo;
    if (hq2) vout[(size_t)p * n + q2] = hi;
    if (hq) {
        rot2(vin[(size_t)q * n + p2], hq2 ? vin[(size_t)q * n + q2] : 0.0, c2, s2, lo, hi);
        vout[(size_t)q * n + p2] = lo;
        if (hq2) vout[(size_t)q * n + q2] = hi;
    }
}

// the end of a sweep, one workgroup: the largest |a_pq| the sweep met against the threshold, the diagonal checked for a non-finite entry
__global__ __launch_bounds__(256) void eigh_sweep_end_kernel(const double* __restrict__ a, int n, double* __restrict__ off, const double* __restrict__ tol,
                                                             int* __restrict__ state) {
    if (state[ST_DONE]) return;
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += 256) bad |= finite_f64(a[(size_t)i * n + i]) ? 0 : 1;
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0) return;
    double mx = 0.0;
    for (int g = 0; g < EIGH_MAX_N / 2 / EIGH_TILE; ++g) {
        mx = off[g] > mx ? off[g] : mx;
        off[g] = 0.0;
    }
    const int sweeps = state[ST_SWEEPS] + 1;
    state[ST_SWEEPS] = sweeps;
    if (bad || !finite_f64(mx)) { state[ST_INFO] = 2; state[ST_DONE] = 1; }
    else if (mx <= *tol) { state[ST_INFO] = 0; state[ST_DONE] = 1; }
    else if (sweeps >= EIGH_MAX_SWEEPS) { state[ST_INFO] = 1; state[ST_DONE] = 1; }
}

// one workgroup: rank of every diagonal entry (how many are smaller, or equal with a lower index), w[rank] = a_ii, perm[rank] = i; info's two words
__global__ __launch_bounds__(256) void eigh_sort_kernel(const double* __restrict__ a, int n, double* __restrict__ w, int* __restrict__ perm,
                                                        const int* __restrict__ state, int* __restrict__ info) {
    __shared__ double dg[EIGH_MAX_N];
    for (int i = threadIdx.x; i < n; i += 256) dg[i] = a[(size_t)i * n + i];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const double x = dg[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (dg[j] < x || (dg[j] == x && j < i)) ? 1 : 0;
        w[rank] = x;          // rank < n whatever the values are (a NaN compares false: ranks may then collide, never leave the range)
        perm[rank] = i;
    }
    if (threadIdx.x == 0) {
        info[0] = state[ST_INFO];
        info[1] = state[ST_SWEEPS];
    }
}
__global__ __launch_bounds__(256) void eigh_gather_kernel(const double* __restrict__ v, int n, const int* __restrict__ perm, double* __restrict__ out, int64_t ldv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), r = (int)(e % n);
    const int src = perm[r];
    out[(size_t)i * ldv + r] = (src >= 0 && src < n) ? v[(size_t)i * n + src] : 0.0;
}

}  // namespace

extern "C" int cvae_eigh_max_sweeps(void) { return EIGH_MAX_SWEEPS; }

extern "C" size_t cvae_eigh_f64_workspace_bytes(int64_t n) {
    if (n < 1 || n > EIGH_MAX_N) return 0;
    return eigh_plan(n).bytes;
}

extern "C" int cvae_eigh_f64(const double* A, int64_t lda, int64_t n, double* w, double* V, int64_t ldv, int* info, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (n < 1 || n > EIGH_MAX_N || lda < n || ldv < n) return CVAE_E_BADSHAPE;
    if (any_null(A, w, V, info, workspace)) return CVAE_E_NULLPTR;
    if (!all_aligned<8>(A, w, V, workspace) || !aligned4(info)) return CVAE_E_UNSUPPORTED;
    if (workspace_bytes < cvae_eigh_f64_workspace_bytes(n)) return CVAE_E_WORKSPACE;
    const eigh_layout L = eigh_plan(n);
    char* base = (char*)workspace;
    double* a[2] = {(double*)(base + L.a[0]), (double*)(base + L.a[1])};
    double* v[2] = {(double*)(base + L.v[0]), (double*)(base + L.v[1])};
    double* part = (double*)(base + L.part);
    double* off = (double*)(base + L.off);
    double* tol = (double*)(base + L.tol);
    int* perm = (int*)(base + L.perm);
    int* state = (int*)(base + L.state);
    hipStream_t st = (hipStream_t)stream;
    const int nn = (int)n, m = nn + (nn & 1), rounds = m - 1;
    const unsigned eblocks = (unsigned)((n * n + 255) / 256), tiles = (unsigned)((m / 2 + EIGH_TILE - 1) / EIGH_TILE);
    hipLaunchKernelGGL(eigh_init_kernel, dim3(eblocks), dim3(256), 0, st, A, lda, nn, a[0], v[0], part);
    hipLaunchKernelGGL(eigh_setup_kernel, dim3(1), dim3(256), 0, st, (const double*)part, (int)eblocks, off, tol, state);
    CVAE_CHECK_LAUNCH();
    int cur = 0;
    for (int sweep = 0;; ++sweep) {
        int done = 0;          // the one word the host reads: before the first sweep (a non-finite entry ends the run at the setup) and after every sweep
        if (hipMemcpyAsync(&done, state + ST_DONE, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return CVAE_E_LAUNCH;
        if (done || sweep == EIGH_MAX_SWEEPS) break;          // the sweep-end launch sets the word at the cap, so the second test only states the bound
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(eigh_round_kernel, dim3(tiles, tiles), dim3(256), 0, st, (const double*)a[cur], a[cur ^ 1], (const double*)v[cur], v[cur ^ 1], nn, r,
                               (const int*)state, off);
            cur ^= 1;
        }
        hipLaunchKernelGGL(eigh_sweep_end_kernel, dim3(1), dim3(256), 0, st, (const double*)a[cur], nn, off, (const double*)tol, state);
        CVAE_CHECK_LAUNCH();
    }
    // a run that a non-finite entry ended at the setup never turned a buffer: a[0], v[0] hold the input and the identity, and info says 2
    hipLaunchKernelGGL(eigh_sort_kernel, dim3(1), dim3(256), 0, st, (const double*)a[cur], nn, w, perm, (const int*)state, info);
    hipLaunchKernelGGL(eigh_gather_kernel, dim3(eblocks), dim3(256), 0, st, (const double*)v[cur], nn, (const int*)perm, V, ldv);
    return launch_rc();
}
