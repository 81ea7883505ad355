// morphology.hip — the 12 morphology features of a batch of small grey images: the reference's extract_refined_features
// (mnist_test/01_baseline_causal_vae/dataset.py:11-99: skimage label / regionprops, scipy distance_transform_edt) as ONE launch, one workgroup per image, the
// image and every working array in LDS.  1 <= H, W <= 64.  Everything up to the last phase is integer arithmetic and exact:
//   mask         x > threshold in fp32 (a NaN is background)
//   components   8-connectivity by union-find on the raster index with atomicMin (a root is its component's first pixel in raster order, so label order is
//                root order); no iteration count anywhere: every loop ends because labels only fall.  The measured component is the one of largest area,
//                ties to the lowest root (one atomicMax on area << 12 | 4095 - root)
//   sums         A, the bounding box, sum r, c, r^2, c^2, rc, and each row's leftmost and rightmost pixel of the component
//   perimeter    border = component minus its erosion by the 4-neighbour cross; code = 1 + 2 (4-neighbours in border) + 10 (diagonal ones); the ten counts
//                of the codes that carry a weight (CVAE_MORPH_RAW_PERIM)
//   thickness    max over the WHOLE mask of the squared Euclidean distance to the nearest background pixel of the image, by the separable two-pass form:
//                g = the distance along the column, then min over c' of (c - c')^2 + g(r, c')^2
//   convex area  the hull of the points (r +- 1/2, c), (r, c +- 1/2) in doubled coordinates.  A component covers every row of its box, so per doubled row
//                R = 2 rmin - 1 .. 2 rmax + 1 the hull only needs the smallest and largest doubled column; two threads run a monotone chain over these
//                (at most 129 points each, the right side negated so that both run the same code), then one thread per row counts the centres inside or ON
//   Euler        bit-quads over the zero-padded component, (Q1 - Q3 - 2 QD) / 4
//   symmetry     sum |x - fliplr x| and sum |x - flipud x|: fp32 differences, added in fp64 along each row by one thread, the rows in order by thread 0
// then thread 0 forms the twelve features in fp64 from the integers and rounds each once.  Integer LDS atomics only; fp64 sums in one fixed order that does
// not depend on the thread count either: an image's bits depend on nothing but the image.  The threads per image are a function of the shape.
#include <math.h>
#include "common.h"

CVAE_TUNABLE(MORPH_THREADS, 128);          // threads per image of at most MORPH_SMALL_PIXELS pixels (profiles/morphology.md: 64, 128, 256 at 28 x 28)
CVAE_TUNABLE(MORPH_THREADS_LARGE, 256);    // threads per larger image (the same three at 64 x 64)
CVAE_TUNABLE(MORPH_SMALL_PIXELS, 1024);    // between 784 and 4096 pixels the crossover was not measured

namespace {

constexpr bool threads_ok(long long n) { return n == 64 || n == 128 || n == 256 || n == 512; }
static_assert(threads_ok(MORPH_THREADS) && threads_ok(MORPH_THREADS_LARGE), "MORPH_THREADS, MORPH_THREADS_LARGE: 64, 128, 256 or 512");
constexpr int SIDE = CVAE_MORPH_MAX_SIDE, CHAIN = 2 * SIDE + 2;
constexpr int G_INF = 1 << 12;          // "no background in this column": its square plus 63^2 stays far below 2^31
enum { IN_MASK = 1, IN_COMP = 2, IN_BORDER = 4 };
enum { ACC_MASK, ACC_NCOMP, ACC_AREA, ACC_MINR, ACC_MINC, ACC_MAXR, ACC_MAXC, ACC_SR, ACC_SC, ACC_SRR, ACC_SCC, ACC_SRC, ACC_PERIM, ACC_MAXD2 = ACC_PERIM + 10,
       ACC_CONVEX, ACC_Q1, ACC_Q3, ACC_QD, ACC_WORDS };
__device__ const int PERIM_CODES[10] = {5, 7, 15, 17, 25, 27, 21, 33, 13, 23};

struct MorphFixed {
    double rowsum[2][SIDE];          // per row: sum |x - fliplr x|, sum |x - flipud x|
    int acc[ACC_WORDS];
    unsigned best;                   // area << 12 | 4095 - root of the largest component
    int cmin[SIDE], cmax[SIDE];      // the component's leftmost / rightmost column per row
    int ptc[2][CHAIN];               // per doubled row: smallest doubled column, minus the largest
    int hk[2][CHAIN], nh[2];         // the chains: indices into ptc
};
constexpr size_t FIXED_BYTES = (sizeof(MorphFixed) + 15) / 16 * 16;
inline size_t morph_lds_bytes(int P) { return FIXED_BYTES + (size_t)P * 9; }

__device__ __forceinline__ int find_root(int* lab, int p) {
    const volatile int* l = lab;
    for (int q; (q = l[p]) != p;) p = q;
    return p;
}
// lock-free union: the larger root is hung under the smaller; if another thread lowered it first, go on from what it wrote
__device__ __forceinline__ void unite(int* lab, int a, int b) {
    for (;;) {
        a = find_root(lab, a);
        b = find_root(lab, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}

template <int NT> __global__ __launch_bounds__(NT) void morph12_kernel(const float* __restrict__ x, int H, int W, float thr, double area_norm, double perimeter_norm,
                                                     double thickness_norm, double axis_norm, float* __restrict__ feats, int* __restrict__ raw) {
    extern __shared__ double morph_smem[];
    MorphFixed& S = *(MorphFixed*)morph_smem;
    const int P = H * W, t = threadIdx.x;
    int* buf = (int*)((char*)morph_smem + FIXED_BYTES);          // the image, then component areas, then the column distances
    float* img = (float*)buf;
    int* lab = buf + P;
    unsigned char* flag = (unsigned char*)(lab + P);
    const float* xi = x + (size_t)blockIdx.x * P;
    float* fo = feats + (size_t)blockIdx.x * 12;
    int* ro = raw ? raw + (size_t)blockIdx.x * CVAE_MORPH_RAW_WORDS : nullptr;

    // ---- load, mask ----
    for (int i = t; i < ACC_WORDS; i += NT) S.acc[i] = (i == ACC_MINR || i == ACC_MINC) ? SIDE : ((i == ACC_MAXR || i == ACC_MAXC || i == ACC_MAXD2) ? -1 : 0);
    for (int i = t; i < SIDE; i += NT) { S.cmin[i] = SIDE; S.cmax[i] = -1; }
    if (t == 0) S.best = 0u;
    int n_mask = 0;
    for (int p = t; p < P; p += NT) {
        const float v = xi[p];
        const bool m = v > thr;
        img[p] = v;
        flag[p] = m ? IN_MASK : 0;
        lab[p] = m ? p : -1;
        n_mask += m;
    }
    __syncthreads();
    if (n_mask) atomicAdd(&S.acc[ACC_MASK], n_mask);

    // ---- symmetry sums (the last use of the image) and the unions ----
    for (int j = t; j < 2 * SIDE; j += NT) {
        const int which = j / SIDE, r = j % SIDE;
        if (r >= H) continue;
        const float* row = img + r * W;
        const float* other = which ? img + (H - 1 - r) * W : row + (W - 1);
        const int step = which ? 1 : -1;
        double s = 0.0;
        for (int c = 0; c < W; ++c) s += (double)fabsf(row[c] - other[step * c]);
        S.rowsum[which][r] = s;
    }
    for (int p = t; p < P; p += NT) {
        if (!flag[p]) continue;
        const int r = p / W, c = p - r * W;
        if (c > 0 && flag[p - 1]) unite(lab, p, p - 1);
        if (r > 0) {
            if (flag[p - W]) unite(lab, p, p - W);
            if (c > 0 && flag[p - W - 1]) unite(lab, p, p - W - 1);
            if (c < W - 1 && flag[p - W + 1]) unite(lab, p, p - W + 1);
        }
    }
    __syncthreads();

    // ---- every pixel to its root; buf becomes the area table ----
    for (int p = t; p < P; p += NT) {
        buf[p] = 0;
        if (flag[p]) lab[p] = find_root(lab, p);
    }
    __syncthreads();
    int n_comp = 0;
    for (int p = t; p < P; p += NT) {
        if (!flag[p]) continue;
        atomicAdd(&buf[lab[p]], 1);
        n_comp += lab[p] == p;
    }
    if (n_comp) atomicAdd(&S.acc[ACC_NCOMP], n_comp);
    __syncthreads();
    for (int p = t; p < P; p += NT)
        if (lab[p] == p) atomicMax(&S.best, ((unsigned)buf[p] << 12) | (unsigned)(4095 - p));
    __syncthreads();
    const unsigned best = S.best;
    if (best == 0u) {          // an empty mask: twelve zeros, as the reference returns
        if (t < 12) fo[t] = 0.f;
        if (ro && t < CVAE_MORPH_RAW_WORDS) ro[t] = t == CVAE_MORPH_RAW_STATUS ? CVAE_MORPH_EMPTY : (t == CVAE_MORPH_RAW_FIRST ? -1 : 0);
        return;
    }
    const int root = 4095 - (int)(best & 4095u);

    // ---- the component's sums and row extremes; the column pass of the distance transform (buf is free again) ----
    {
        int a = 0, r0 = SIDE, c0 = SIDE, r1 = -1, c1 = -1, sr = 0, sc = 0, srr = 0, scc = 0, src = 0;
        for (int p = t; p < P; p += NT) {
            if (lab[p] != root) continue;
            const int r = p / W, c = p - r * W;
            flag[p] = IN_MASK | IN_COMP;
            ++a; sr += r; sc += c; srr += r * r; scc += c * c; src += r * c;
            r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, c); c1 = max(c1, c);
            atomicMin(&S.cmin[r], c);
            atomicMax(&S.cmax[r], c);
        }
        if (a) {
            atomicAdd(&S.acc[ACC_AREA], a); atomicAdd(&S.acc[ACC_SR], sr); atomicAdd(&S.acc[ACC_SC], sc);
            atomicAdd(&S.acc[ACC_SRR], srr); atomicAdd(&S.acc[ACC_SCC], scc); atomicAdd(&S.acc[ACC_SRC], src);
            atomicMin(&S.acc[ACC_MINR], r0); atomicMin(&S.acc[ACC_MINC], c0); atomicMax(&S.acc[ACC_MAXR], r1); atomicMax(&S.acc[ACC_MAXC], c1);
        }
    }
    __syncthreads();          // every read of the area table is behind us (S.best), every IN_COMP bit is set
    for (int c = t; c < W; c += NT) {
        int d = G_INF;
        for (int r = 0; r < H; ++r) {
            d = flag[r * W + c] ? min(d + 1, G_INF) : 0;
            buf[r * W + c] = d;
        }
        d = G_INF;
        for (int r = H - 1; r >= 0; --r) {
            d = flag[r * W + c] ? min(d + 1, G_INF) : 0;
            buf[r * W + c] = min(buf[r * W + c], d);
        }
    }
    const int rmin = S.acc[ACC_MINR], rmax = S.acc[ACC_MAXR], cmin = S.acc[ACC_MINC], cmax = S.acc[ACC_MAXC];
    const int n_rows2 = 2 * (rmax - rmin) + 3;          // doubled rows 2 rmin - 1 .. 2 rmax + 1
    for (int j = t; j < 2 * n_rows2; j += NT) {
        const int s = j / n_rows2, k = j - s * n_rows2, R = 2 * rmin - 1 + k;
        int v;
        if (R & 1) {          // between rows (R - 1) / 2 and (R + 1) / 2: the vertical points (r +- 1/2, c) of whichever of the two exist
            const int ra = (R - 1) >> 1, rb = ra + 1;
            const bool ha = ra >= rmin, hb = rb <= rmax;
            if (s == 0) v = min(ha ? 2 * S.cmin[ra] : 4 * SIDE, hb ? 2 * S.cmin[rb] : 4 * SIDE);
            else v = -max(ha ? 2 * S.cmax[ra] : -1, hb ? 2 * S.cmax[rb] : -1);
        } else {              // a pixel row: the horizontal points (r, c +- 1/2)
            v = s == 0 ? 2 * S.cmin[R >> 1] - 1 : -(2 * S.cmax[R >> 1] + 1);
        }
        S.ptc[s][k] = v;
    }
    // border pixels of the component
    for (int p = t; p < P; p += NT) {
        if (!(flag[p] & IN_COMP)) continue;
        const int r = p / W, c = p - r * W;
        const bool inner = r > 0 && r < H - 1 && c > 0 && c < W - 1 && (flag[p - W] & IN_COMP) && (flag[p + W] & IN_COMP) && (flag[p - 1] & IN_COMP) &&
                           (flag[p + 1] & IN_COMP);
        if (!inner) flag[p] = IN_MASK | IN_COMP | IN_BORDER;          // only this pixel's own byte changes, and nobody reads its IN_BORDER bit before the barrier
    }
    // bit-quads: window (i, j) covers pixels (i - 1 .. i, j - 1 .. j)
    {
        int q1 = 0, q3 = 0, qd = 0;
        for (int q = t; q < (H + 1) * (W + 1); q += NT) {
            const int i = q / (W + 1), j = q - i * (W + 1);
            const int p00 = (i > 0 && j > 0) ? (flag[(i - 1) * W + j - 1] >> 1) & 1 : 0, p01 = (i > 0 && j < W) ? (flag[(i - 1) * W + j] >> 1) & 1 : 0;
            const int p10 = (i < H && j > 0) ? (flag[i * W + j - 1] >> 1) & 1 : 0, p11 = (i < H && j < W) ? (flag[i * W + j] >> 1) & 1 : 0;
            const int n = p00 + p01 + p10 + p11;
            q1 += n == 1; q3 += n == 3; qd += (n == 2 && p00 == p11);
        }
        if (q1) atomicAdd(&S.acc[ACC_Q1], q1);
        if (q3) atomicAdd(&S.acc[ACC_Q3], q3);
        if (qd) atomicAdd(&S.acc[ACC_QD], qd);
    }
    __syncthreads();

    // ---- perimeter codes, the row pass of the distance transform, the two chains ----
    for (int s = t; s < 2; s += NT) {          // the lower convex envelope of (k, ptc[s][k])
        const int* C = S.ptc[s];
        int* hk = S.hk[s];
        int n = 0;
        for (int k = 0; k < n_rows2; ++k) {
            while (n >= 2) {
                const int k0 = hk[n - 2], k1 = hk[n - 1];
                if ((C[k1] - C[k0]) * (k - k0) >= (C[k] - C[k0]) * (k1 - k0)) --n; else break;          // k1 on or above the segment k0 - k: not a vertex
            }
            hk[n++] = k;
        }
        S.nh[s] = n;
    }
    {
        int d2max = -1;
        for (int p = t; p < P; p += NT) {
            const int f = flag[p];
            if (!f) continue;
            const int r = p / W, c = p - r * W;
            if (f & IN_BORDER) {
                int n4 = 0, nd = 0;
                if (r > 0) { n4 += (flag[p - W] >> 2) & 1; if (c > 0) nd += (flag[p - W - 1] >> 2) & 1; if (c < W - 1) nd += (flag[p - W + 1] >> 2) & 1; }
                if (r < H - 1) { n4 += (flag[p + W] >> 2) & 1; if (c > 0) nd += (flag[p + W - 1] >> 2) & 1; if (c < W - 1) nd += (flag[p + W + 1] >> 2) & 1; }
                if (c > 0) n4 += (flag[p - 1] >> 2) & 1;
                if (c < W - 1) n4 += (flag[p + 1] >> 2) & 1;
                const int code = 1 + 2 * n4 + 10 * nd;
#pragma unroll
                for (int i = 0; i < 10; ++i)
                    if (code == PERIM_CODES[i]) atomicAdd(&S.acc[ACC_PERIM + i], 1);
            }
            const int* g = buf + r * W;
            int best2 = G_INF * G_INF;
            for (int cc = 0; cc < W; ++cc) {
                const int gg = g[cc], dc = c - cc;
                best2 = min(best2, dc * dc + gg * gg);
            }
            d2max = max(d2max, best2);
        }
        if (d2max >= 0) atomicMax(&S.acc[ACC_MAXD2], d2max);
    }
    __syncthreads();

    // ---- pixel centres inside or on the hull: one thread per row of the box ----
    for (int r = rmin + t; r <= rmax; r += NT) {
        const int k = 2 * (r - rmin) + 1;
        int k0[2], k1[2], C0[2], C1[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int i = 0;
            while (S.hk[s][i + 1] < k) ++i;          // the chain ends at n_rows2 - 1 > k
            k0[s] = S.hk[s][i]; k1[s] = S.hk[s][i + 1];
            C0[s] = S.ptc[s][k0[s]]; C1[s] = S.ptc[s][k1[s]];
        }
        int n = 0;
        for (int c = cmin; c <= cmax; ++c)
            n += ((2 * c - C0[0]) * (k1[0] - k0[0]) >= (C1[0] - C0[0]) * (k - k0[0])) && ((-2 * c - C0[1]) * (k1[1] - k0[1]) >= (C1[1] - C0[1]) * (k - k0[1]));
        atomicAdd(&S.acc[ACC_CONVEX], n);
    }
    __syncthreads();

    // ---- the features, in fp64 from the integers, each rounded once ----
    if (t != 0) return;
    const int* a = S.acc;
    const bool no_background = a[ACC_MASK] == P;
    const int euler = (a[ACC_Q1] - a[ACC_Q3] - 2 * a[ACC_QD]) / 4, maxd2 = no_background ? -1 : a[ACC_MAXD2];
    if (ro) {
        ro[CVAE_MORPH_RAW_STATUS] = no_background ? CVAE_MORPH_NO_BACKGROUND : 0;
        ro[CVAE_MORPH_RAW_COMPONENTS] = a[ACC_NCOMP];
        ro[CVAE_MORPH_RAW_FIRST] = root;
        ro[CVAE_MORPH_RAW_AREA] = a[ACC_AREA];
        ro[CVAE_MORPH_RAW_MINR] = rmin; ro[CVAE_MORPH_RAW_MINC] = cmin; ro[CVAE_MORPH_RAW_MAXR] = rmax + 1; ro[CVAE_MORPH_RAW_MAXC] = cmax + 1;
        ro[CVAE_MORPH_RAW_SR] = a[ACC_SR]; ro[CVAE_MORPH_RAW_SC] = a[ACC_SC]; ro[CVAE_MORPH_RAW_SRR] = a[ACC_SRR]; ro[CVAE_MORPH_RAW_SCC] = a[ACC_SCC];
        ro[CVAE_MORPH_RAW_SRC] = a[ACC_SRC];
        for (int i = 0; i < 10; ++i) ro[CVAE_MORPH_RAW_PERIM + i] = a[ACC_PERIM + i];
        ro[CVAE_MORPH_RAW_MAXD2] = maxd2;
        ro[CVAE_MORPH_RAW_CONVEX] = a[ACC_CONVEX];
        ro[CVAE_MORPH_RAW_Q1] = a[ACC_Q1]; ro[CVAE_MORPH_RAW_Q3] = a[ACC_Q3]; ro[CVAE_MORPH_RAW_QD] = a[ACC_QD]; ro[CVAE_MORPH_RAW_EULER] = euler;
        for (int i = CVAE_MORPH_RAW_EULER + 1; i < CVAE_MORPH_RAW_WORDS; ++i) ro[i] = 0;
    }
    const double A = (double)a[ACC_AREA];
    const long long ia = a[ACC_AREA], sr = a[ACC_SR], sc = a[ACC_SC];
    const long long m20 = ia * a[ACC_SRR] - sr * sr, m02 = ia * a[ACC_SCC] - sc * sc, m11 = ia * a[ACC_SRC] - sr * sc;          // A^2 (mu / A), exact
    const double sqrt2 = 1.4142135623730951, pi = 3.141592653589793;
    const double n1 = (double)(a[ACC_PERIM] + a[ACC_PERIM + 1] + a[ACC_PERIM + 2] + a[ACC_PERIM + 3] + a[ACC_PERIM + 4] + a[ACC_PERIM + 5]);
    const double n2 = (double)(a[ACC_PERIM + 6] + a[ACC_PERIM + 7]), n3 = (double)(a[ACC_PERIM + 8] + a[ACC_PERIM + 9]);
    // skimage's inertia tensor is a = mu02 / A, c = mu20 / A, b = -mu11 / A; p = A^2 (a + c), q = A^2 (a - c), hyp = A^2 sqrt((a - c)^2 + 4 b^2)
    const double p = (double)(m02 + m20), q = (double)(m02 - m20), d11 = (double)m11;
    const double hyp = sqrt(q * q + 4.0 * d11 * d11);
    const double l1 = fmax((p + hyp) / (2.0 * A * A), 0.0);
    const double ori = m02 == m20 ? (m11 > 0 ? -pi / 4.0 : pi / 4.0) : atan2(2.0 * d11, (double)(m20 - m02)) / 2.0;          // atan2(-2 b, c - a) / 2
    const double h = (double)(rmax + 1 - rmin), w = (double)(cmax + 1 - cmin);
    double slr = 0.0, sud = 0.0;
    for (int r = 0; r < H; ++r) { slr += S.rowsum[0][r]; sud += S.rowsum[1][r]; }
    fo[0] = (float)(A / area_norm);
    fo[1] = (float)((n1 + n2 * sqrt2 + n3 * ((1.0 + sqrt2) / 2.0)) / perimeter_norm);
    fo[2] = no_background ? __builtin_nanf("") : (float)(sqrt((double)maxd2) / thickness_norm);
    fo[3] = (float)(4.0 * sqrt(l1) / axis_norm);
    fo[4] = (float)(l1 > 0.0 ? sqrt(2.0 * hyp / (p + hyp)) : 0.0);
    fo[5] = (float)((ori + pi / 2.0) / pi);
    fo[6] = (float)(A / (double)a[ACC_CONVEX]);
    fo[7] = (float)(A / (h * w));
    fo[8] = (float)((w / h) / 3.0);
    fo[9] = (float)(((double)euler + 2.0) / 4.0);
    fo[10] = (float)(1.0 - slr / (double)P);
    fo[11] = (float)(1.0 - sud / (double)P);
}

}  // namespace

// ---- the C entries ----
static int morph_threads(int64_t H, int64_t W) { return (int)(H * W <= MORPH_SMALL_PIXELS ? MORPH_THREADS : MORPH_THREADS_LARGE); }
extern "C" int cvae_morph12_threads(int64_t H, int64_t W) { return morph_threads(H, W); }

extern "C" int cvae_morph12_f32(const float* x, int64_t B, int64_t H, int64_t W, float threshold, double area_norm, double perimeter_norm, double thickness_norm,
                                double axis_norm, float* feats, int* raw, void* stream) {
    if (B < 1 || H < 1 || W < 1) return CVAE_E_BADSHAPE;
    if (!(area_norm > 0.0) || !(perimeter_norm > 0.0) || !(thickness_norm > 0.0) || !(axis_norm > 0.0) || threshold != threshold) return CVAE_E_BADSHAPE;
    if (H > CVAE_MORPH_MAX_SIDE || W > CVAE_MORPH_MAX_SIDE || B > 0x7fffffffLL) return CVAE_E_UNSUPPORTED;
    if (!x || !feats) return CVAE_E_NULLPTR;
    const int P = (int)(H * W);
    return with_bool(morph_threads(H, W) == (int)MORPH_THREADS, [&](auto small) {
        constexpr int NT = decltype(small)::value ? (int)MORPH_THREADS : (int)MORPH_THREADS_LARGE;
        hipLaunchKernelGGL(morph12_kernel<NT>, dim3((unsigned)B), dim3(NT), morph_lds_bytes(P), (hipStream_t)stream, x, (int)H, (int)W, threshold, area_norm,
                           perimeter_norm, thickness_norm, axis_norm, feats, raw);
        return launch_rc();
    });
}
