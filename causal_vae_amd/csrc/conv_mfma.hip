// conv_mfma.hip — the k4/s2/p1 convolution family on the CDNA4 matrix cores, channels-last.
//
// Every strided conv of the model relates a SMALL tensor S [B, sd, sh, sw, Cs] and a LARGE tensor L [B, ld, lh, lw, Cl]
// (l = 2 s - 1 + k, k = 0..3 per strided dim; nd = 2 has one depth tap).  Three products cover all six ops
// (include/cvae_hip.h): down (S from L), up (L from S), wgrad (dW from S and L).
//
// down / up  — implicit GEMM, M = output positions, N = output channels, K = (tap, input channel):
//   * a workgroup owns a spatial tile of M (3D: 4x4x8 or 4x8x8 positions; 2D: 8x16 or 16x16) and loads the INPUT
//     HALO of that tile ONCE per 16-channel chunk into LDS with coalesced 16-byte rows; all 64 (down) / 8 (up, per
//     output parity) taps then read their A fragments straight out of that tile — the im2col matrix is never
//     materialised and each input byte crosses L2->LDS ~1.8x instead of 8x.
//   * `up` is the transposed conv in its parity form: the 2x2x2 output parity classes are 8 independent k2/s1
//     sub-convolutions (8 taps each), so no zero-insertion FLOPs are spent.
//   * B (weights, pre-packed [tap][K/16][N][16] by cvae_conv_pack_weight): the 64-channel-tile forms of bf16 (and of fp8 3D `up`) run 1 x 2 waves x 2 K-split
//     groups that fetch their fragments per wave straight from the packed global panels into a register ring ("BD", "TS"); every other form (fp32, 32-channel
//     tiles, the remaining fp8 products) streams them through a double-buffered LDS panel, 4 taps per barrier.  DataForm (below the kernels) is the ONE table of
//     which instance serves which product; dispatch_conv is the one place that lifts act / stage depth into template arguments.  A second `up` kernel
//     (conv_up_full_kernel) stages the halo of ALL input channels once and walks the output parities inside the workgroup; it serves the large grids of the
//     decode sweep (32-channel tiles only).
//   * bf16: v_mfma_f32_32x32x16_bf16 (fp32 accumulate);  fp32: v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain);  fp8: v_mfma_scale_f32_32x32x64_f8f6f4.
//   * epilogue fuses bias + ReLU/Sigmoid (forward use) or the ReLU mask of the saved activation (backward use).  The three kernels with that mask
//     (conv_data_kernel, conv_splitk_finish_kernel, conv_up_full_kernel) live in .inc files included twice: the second, "gated" instance multiplies by a
//     LeakyReLU slope where the first one zeroes (cvae_conv_down_bwd_data: the ViT-VAE stem's input gradients).
// wgrad — M = Cs, N = Cl, K = positions.  Both operands are [position][channel] in memory, i.e. K-strided: bf16 uses
//   the gfx950 transposing LDS read (ds_read_b64_tr_b16) to build K-contiguous fragments; fp32's 32x32x2 MFMA takes
//   one element per lane and needs no transpose.  Every workgroup leaves ONE fp32 slab [kh][64 cs][32 cl][kw] of partial sums with
//   plain stores; wgrad_reduce_kernel adds the slabs in index order and writes the reference [Cs][Cl][taps] layout (no atomics).  A layer
//   with one slab per (kd, channel block) group skips that round trip: its workgroups write the reference layout themselves.
#include "common.h"

// Development aid (make EXTRA=-DCVAE_STAMP, tools/stamp_probe.py): thread 0 of every workgroup of conv_data_kernel records the
// shader clock at its phase boundaries into a device array that cvae_debug_stamps() copies out.  Not compiled by default.
#ifdef CVAE_STAMP
#define CVAE_STAMP_SLOTS 32
#define CVAE_STAMP_WGS 8192
__device__ unsigned long long g_stamp[(size_t)CVAE_STAMP_WGS * CVAE_STAMP_SLOTS];
#define STAMP(i)                                                                                                         \
    do {                                                                                                                 \
        if (t == 0 && stamp_wg < CVAE_STAMP_WGS) g_stamp[(size_t)stamp_wg * CVAE_STAMP_SLOTS + (i)] = __builtin_readcyclecounter(); \
    } while (0)
// head of a probed kernel (declares stamp_wg; `t` is the thread index): wall clock into slot 30, hardware id registers into slot 29, then STAMP(0)
#define STAMP_BEGIN()                                                                                                    \
    const unsigned stamp_wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                            \
    if (t == 0 && stamp_wg < CVAE_STAMP_WGS) {                                                                           \
        g_stamp[(size_t)stamp_wg * CVAE_STAMP_SLOTS + 30] = wall_clock64();                                              \
        g_stamp[(size_t)stamp_wg * CVAE_STAMP_SLOTS + 29] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | __builtin_amdgcn_s_getreg(63492); \
    }                                                                                                                    \
    STAMP(0)
// its tail: once the stores have left the wave (vmcnt(0)), STAMP(27) and the wall clock into slot 31
#define STAMP_END()                                                                                                      \
    do {                                                                                                                 \
        __builtin_amdgcn_s_waitcnt(0);                                                                                   \
        STAMP(27);                                                                                                       \
        if (t == 0 && stamp_wg < CVAE_STAMP_WGS) g_stamp[(size_t)stamp_wg * CVAE_STAMP_SLOTS + 31] = wall_clock64();     \
    } while (0)
#else
#define STAMP(i)
#define STAMP_BEGIN()
#define STAMP_END()
#endif

namespace {

// ---- tunables: each may be overridden for an A/B build with make EXTRA=-DCVAE_<NAME>=<n> (CVAE_TUNABLE, common.h) ----
CVAE_TUNABLE(BD_GS, 8);                 // k-steps per weight register group of the BD tap loop, chunks of >= 64 k-steps (3D down)
CVAE_TUNABLE(APIPE, 3);                 // k-steps the activation ds_reads are issued ahead of their MFMAs (MI = 2 forms and conv_up_full_kernel)
CVAE_TUNABLE(UPFULL_MIN_GRID, 2048);    // workgroups (tiles x channel blocks x batch) from which conv_up_full_kernel is used: many rounds of one workgroup per CU (the
                                        // 240-row decode sweep: -12 % on its 64 -> 32 channel layer); at the training step's 512 it measured +-0 against conv_data_kernel<UP>
CVAE_TUNABLE(UPFULL_MIN_WG, 512);       // workgroups below which conv_up_full_kernel spreads a tile's parity classes over sibling workgroups (~2 per CU)
CVAE_TUNABLE(XPAIR_MIN_WGS, 2048);      // workgroups from which a 3D `up` layer at most half a tile wide puts two samples in one tile (XB = 2): the decode sweep's 4^3 -> 8^3 layer
CVAE_TUNABLE(XPAIR_2D_MIN_WGS, 512);    // the same for 2D layers, `down` and `up` (the 7 x 7 grids of the MNIST model at batch 1024)
CVAE_TUNABLE(WG_TILES, 16);             // wgrad: tiles of 128 positions summed into one slab
CVAE_TUNABLE(WG_MIN_WG, 64);            // wgrad: workgroups a layer gets at least, whatever WG_TILES says

struct ConvGeom {
    int B;
    int sd, sh, sw, Cs;
    int ld, lh, lw, Cl;
    int tiles_d, tiles_h, tiles_w;   // tiling of the M grid (S grid for down / wgrad, q grid for up)
};

// ---------------------------------------------------------------------------------------------- fragments
// f8x2: TWO consecutive fp8 (e4m3) channels as one 2-byte element.  With it the fp8 product is, byte for byte, the bf16 kernel on a tensor of
// Cin / 2 "elements": a 16-byte piece is 16 channels, a halo stage (two pieces per position) is 32 channels, the packed weight panels are
// [tap][Cin / 32][N][32 fp8] = [tap][Cin' / 16][N][16 elements] — the same LDS images, the same conflict-free layout, the same staging.  The one
// difference is the MFMA: v_mfma_scale_f32_32x32x64_f8f6f4 (block-scaled; unit block scales give plain per-tensor fp8) multiplies K = 64
// per instruction at twice the bf16 rate per FLOP, so TWO k-steps (two taps of a 32-channel stage) feed ONE instruction: registers 0-3 of
// both operands hold k-step s, registers 4-7 k-step s + 1.  The order of K inside an instruction does not matter to a dot product as
// long as both operands use the same one, which the symmetric A / B operand maps guarantee.
struct f8x2 { unsigned short v; };
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
template <typename T> struct IsF8 { static constexpr bool value = false; };
template <> struct IsF8<f8x2> { static constexpr bool value = true; };
template <typename T> struct Frag;
template <> struct Frag<bf16> { bf16x8 v; };
template <> struct Frag<float> { float v[8]; };
template <> struct Frag<f8x2> { i32x4 v; };

__device__ __forceinline__ void lds_load(Frag<bf16>& f, const char* p) { f.v = *(const bf16x8*)p; }
__device__ __forceinline__ void lds_load(Frag<float>& f, const char* p) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 16);
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
}
__device__ __forceinline__ void lds_load(Frag<f8x2>& f, const char* p) { f.v = *(const i32x4*)p; }
#define CVAE_E8M0_ONE 0x7F7F7F7F        // block scale 2^0 in every byte: the scaled instruction then is a plain fp8 x fp8 product
// lane (r = lane & 31, h = lane >> 5) holds elements k = 8h .. 8h+7 of its row/column in both precisions
__device__ __forceinline__ void mma(f32x16& acc, const Frag<bf16>& a, const Frag<bf16>& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x16& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}
// What ONE MFMA consumes: a k-step's fragment — or, for fp8, the fragments of TWO k-steps as one 8-register operand, put together where they are
// LOADED (two 16-byte reads into the halves of one register tuple).  Joining single-step fragments in front of each MFMA instead made the
// register allocator juggle 4-register values into 8-register tuples: 256 VGPRs + 59 spilled on the `down` form, a 20 k-cycle epilogue.
struct Frag2 { i32x8 v; };
template <typename T> struct StepFrag { using type = Frag<T>; static constexpr int PW = 1; };
template <> struct StepFrag<f8x2> { using type = Frag2; static constexpr int PW = 2; };
template <typename F>
__device__ __forceinline__ void load_step(F& f, const char* p0, const char*) { lds_load(f, p0); }
__device__ __forceinline__ void load_step(Frag2& f, const char* p0, const char* p1) {
    const i32x4 lo = *(const i32x4*)p0, hi = *(const i32x4*)p1;
    f.v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void mma(f32x16& acc, const Frag2& a, const Frag2& b) {
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.v, b.v, acc, 0, 0, 0, CVAE_E8M0_ONE, 0, CVAE_E8M0_ONE);
}

template <int ND, int BM> struct Tile;
template <> struct Tile<3, 128> { static constexpr int TD = 4, TH = 4, TW = 8; };
template <> struct Tile<3, 256> { static constexpr int TD = 4, TH = 8, TW = 8; };
template <> struct Tile<2, 128> { static constexpr int TD = 1, TH = 8, TW = 16; };
template <> struct Tile<2, 256> { static constexpr int TD = 1, TH = 16, TW = 16; };

// ---- bank-conflict-free halo layout (tools/lds_layout_search.py) ---------------------------------------------------
// ds_read_b128 is served in fixed 16-lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31}; a group is conflict-free when
// its 16 fragments fall in 16 different 16-byte slots of the 256-byte bank row.  Two free choices make that true for
// every tap: (a) WHICH output position each MFMA row (lane) stands for inside its 32-position sub-tile — any bijection
// works as long as the epilogue uses the same one — and (b) the halo row pitch RS (in 16-byte slots), with the
// stride-2 (down) halo split into even-x / odd-x planes so that consecutive outputs read consecutive slots.
// Found by exhaustive search over bit permutations and pitches: 3D sub-tile 4(h) x 8(w), 2D sub-tile 2(h) x 16(w).
template <int ND> struct SubTile;
template <> struct SubTile<3> {
    static constexpr int SH = 4, SW = 8;
    __device__ static __forceinline__ int w_of(int r) { return ((r >> 2) & 1) | (((r >> 3) & 1) << 1) | ((r & 1) << 2); }
    __device__ static __forceinline__ int h_of(int r) { return ((r >> 4) & 1) | (((r >> 1) & 1) << 1); }
};
template <> struct SubTile<2> {
    static constexpr int SH = 2, SW = 16;
    __device__ static __forceinline__ int w_of(int r) { return ((r >> 2) & 1) | (((r >> 3) & 1) << 1) | ((r & 1) << 2) | (((r >> 1) & 1) << 3); }
    __device__ static __forceinline__ int h_of(int r) { return (r >> 4) & 1; }
};
template <int ND, bool UP> struct HaloPitch;                 // slots per halo row (per x-parity plane when !UP)
template <> struct HaloPitch<3, false> { static constexpr int RS = 10; };
template <> struct HaloPitch<3, true> { static constexpr int RS = 12; };
template <> struct HaloPitch<2, false> { static constexpr int RS = 18; };
template <> struct HaloPitch<2, true> { static constexpr int RS = 20; };

// One 8-element fragment piece (8 B fp8 / 16 B bf16 / 32 B fp32) in flight between a global load and its LDS store.  Staging
// is always written as "issue ALL loads of a tile, then store them": the loads overlap each other (and, for the weight
// panels, the MFMA work placed between the two halves) instead of paying one memory latency per piece.
template <typename T> struct PieceW { using type = uint4; static constexpr int N = (8 * sizeof(T)) / 16; };
template <> struct PieceW<fp8> { using type = uint2; static constexpr int N = 1; };       // 8 fp8 codes: an OUTPUT piece (8 channels of one position)
__device__ __forceinline__ uint4 piece_sel(bool ok, uint4 v) { return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u); }
__device__ __forceinline__ uint2 piece_sel(bool ok, uint2 v) { return make_uint2(ok ? v.x : 0u, ok ? v.y : 0u); }
template <typename T> struct Piece { typename PieceW<T>::type v[PieceW<T>::N]; };
template <typename T>
__device__ __forceinline__ void piece_load(Piece<T>& p, const T* src, bool ok) {
    using W = typename PieceW<T>::type;
#pragma unroll
    for (int u = 0; u < PieceW<T>::N; ++u) {
        // `src` is always a readable address (callers pass the tensor base when !ok): load unconditionally and select, so the
        // compiler emits one straight-line global_load per piece instead of an exec-masked branch around each of them
        p.v[u] = piece_sel(ok, ((const W*)src)[u]);
    }
}
template <typename T>
__device__ __forceinline__ void piece_load_raw(Piece<T>& p, const T* src) {
    using W = typename PieceW<T>::type;
#pragma unroll
    for (int u = 0; u < PieceW<T>::N; ++u) p.v[u] = ((const W*)src)[u];
}
template <typename T>
__device__ __forceinline__ void piece_store_sel(const Piece<T>& p, bool ok, char* dst) {     // zero when !ok (decided at store time)
    using W = typename PieceW<T>::type;
#pragma unroll
    for (int u = 0; u < PieceW<T>::N; ++u) ((W*)dst)[u] = piece_sel(ok, p.v[u]);
}
template <typename T>
__device__ __forceinline__ void piece_store(const Piece<T>& p, char* dst) {
    using W = typename PieceW<T>::type;
#pragma unroll
    for (int u = 0; u < PieceW<T>::N; ++u) ((W*)dst)[u] = p.v[u];
}

// XCD-aware block -> tile map (cdna_hip_programming.md T1, bijective form): blocks b and b+8 share an XCD (and its L2),
// so each XCD gets a contiguous run of spatially adjacent tiles whose halos overlap.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int b, int n) {
    const int q = n >> 3, r = n & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// ---------------------------------------------------------------------------------------------- down / up
// EPI: 0 = bias only, 1 = bias + ReLU, 2 = generic activation code
// KH: 16-channel k-steps per staged halo (1, or 2 for `up` in bf16: its halo box is small enough to hold 32 channels, which halves
// the stage / barrier count per MFMA and fetches 64 contiguous bytes per position instead of 32).
// TO: output (and mask) dtype, = T except on the fp8 inference path, where an fp8 x fp8 product leaves as fp8 (next fp8 layer) or bf16
// (the layer in front of the single-channel kernel): out = act(acc * acc_scale + bias) * out_scale, acc_scale = s_in * s_w the product of the
// operands' per-tensor scales, out_scale = 1 / s_out.
// BD ("B direct"): every wave fetches its weight fragments straight from the packed global panels into a two-group register ring (the panels are
// laid out so that one fragment of a wave is 1 KB contiguous) instead of all waves staging them through LDS: no weight traffic on the LDS
// pipe, which the activation fragments already load to ~2/3 of the MFMA time, and no barrier inside a channel chunk's tap loop.
// TS ("K split", BD only): TS = 2 wave groups of WM x WN waves each own every second k-step (odd / even taps for KH = 1, the two 16-channel halves
// of a stage for KH = 2) of the WHOLE tile and add their accumulators through LDS once, before the epilogue.  With WM = 1 no two waves fetch the
// same weight fragment, and a fetched fragment feeds MI = 4 MFMAs: half the bytes per MFMA on the vector-memory path the BD tap loop is bound by.
// The three kernels below live in .inc files, each included twice: as it was (CONV_GATED 0) and in its gated form (CONV_GATED 1), see conv_data_kernel.inc.
#define CONV_GATE_PARAM_0
#define CONV_GATE_PARAM_1 , float gate_slope
#define CONV_GATE_OFF_0(x) 0.f
#define CONV_GATE_OFF_1(x) ((x) * gate_slope)
#define CONV_CAT_(a, b) a##b
#define CONV_CAT(a, b) CONV_CAT_(a, b)
#define CONV_GATE_PARAM CONV_CAT(CONV_GATE_PARAM_, CONV_GATED)
#define CONV_GATE_OFF(x) CONV_CAT(CONV_GATE_OFF_, CONV_GATED)(x)
#define CONV_GATED 0
#include "conv_data_kernel.inc"
#undef CONV_GATED
#define CONV_GATED 1
#include "conv_data_kernel.inc"
#undef CONV_GATED

// out[p][c] = act(acc_scale * sum_ks ws[ks][p][c] + bias[c]) (* mask > 0): 8 channels per thread, 16-byte bf16 stores.  acc_scale is 1 except behind an
// fp8 product (x * 1.0f is exact: the other dtypes' bits do not change), whose side channel (second fp8 output, amax) is served here too.
#define CONV_GATED 0
#include "conv_splitk_finish_kernel.inc"
#undef CONV_GATED
#define CONV_GATED 1
#include "conv_splitk_finish_kernel.inc"
#undef CONV_GATED

// Kernel-form selection of one `up` launch.  The library picks by launch size (-1 / 0 = automatic); cvae_conv_up and cvae_conv_fp8 let a caller
// force a form for ONE call — the tests run every narrow case through both forms that way.  No process-wide state.
struct UpVariant {
    int upfull = -1;            // conv_up_full_kernel: -1 by grid size (UPFULL_MIN_GRID), 0 never, 1 whenever the shape fits it
    int xpair = -1;             // two samples per tile for layers at most half a tile wide: -1 by grid size (XPAIR_MIN_WGS / XPAIR_2D_MIN_WGS), 0 never, 1 always
    long long walk_units = 0;   // single-channel output layer: 0 = by launch size (C1U_WALK_MIN_UNITS, conv_c1.hip), > 0 = that many units
};

// Split-K factor for a launch of `nwg` workgroups over `nchunks` channel chunks: the layers with 8^3 / 4^3 grids fill a fraction
// of the 256 CUs with one long serial K loop each; slicing K puts ~2 workgroups on every CU.  Largest divisor of nchunks <= target.
// Only `down` splits: an `up` launch already has 8 (4) parity classes per tile and its output is 8x (4x) its input, so the fp32 slabs
// cost more than the shorter K loop saves (measured: enc4 backward-data 23 -> 34 us, dec2 forward 12 -> 22 us with split-K).
static int pick_ksplit(bool up, long long nwg, int nchunks) {
    // a launch that already has one workgroup per CU stays whole: enc3's forward (256 workgroups) took 39 us unsplit against 34 + 8 (finish) split
    if (up || nwg >= 256 || nwg < 1 || nchunks < 2) return 1;
    long long target = (512 + nwg - 1) / nwg;
    if (target > 16) target = 16;
    int best = 1;
    for (int d = 1; d <= nchunks && d <= target; ++d)
        if (nchunks % d == 0) best = d;
    return best;
}

// THE tile form of conv_data_kernel that serves (T, ND, UP, output channel tile): WIDE = 64-channel tiles (Cout % 64 == 0; every `down`), else 32.
//   * KSPLIT forms (bf16; fp8 3D `up`): 1 x 2 waves x 2 K-split groups, MI = 4, weights fetched per wave (BD).  bf16: 0.867 -> 0.832 ms/step at 128^3 B = 4 for BD
//     against LDS weight panels, 0.793 -> 0.785 for (K split) x (N sub-tile) against (M half) x (N sub-tile) waves.  fp8 (rocprofv3 device durations, 4 x 128^3
//     shapes, profiles/r03_fp8_forms.txt): `up` keeps the bf16 form (dec1 9.9 vs 11.2 us, dec2 8.1 vs 8.4 us); `down` wants its weights on LDS panels, since the
//     per-wave fetch needs > 256 VGPRs with 8-register fp8 operands (59 spilled; enc2 57 us against 36 us).
//   * otherwise weights through LDS panels: 2 x 2 waves (64-channel tiles) or 4 x 1 waves (32-channel tiles, 256 rows), MI = 2.
template <typename T, int ND, bool UP, bool WIDE> struct DataForm {
    static constexpr bool KSPLIT = WIDE && (std::is_same<T, bf16>::value || (IsF8<T>::value && UP && ND == 3));
    static constexpr int WM = KSPLIT ? 1 : (WIDE ? 2 : 4), WN = WIDE ? 2 : 1, MI = KSPLIT ? 4 : 2, NI = 1, TS = KSPLIT ? 2 : 1;
    static constexpr bool BD = KSPLIT;
    static constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    // 32-channel stages (KH = 2): bf16 `up` only, where the K loop is long and the grid small (measured: Cin 256: -12 %, 128: -5 %, 64: +2 %)
    static constexpr int KH_MAX = (UP && std::is_same<T, bf16>::value) ? 2 : 1;
    static int kh(const ConvGeom& g) { return (KH_MAX == 2 && g.Cs >= 128 && (g.Cs % 32) == 0) ? 2 : 1; }
    // XB = 2 (two samples per tile) exists for these forms; launch_data_epi takes it by layer width and launch size
    static constexpr bool XPAIR = sizeof(T) <= 2 && ((UP && ND == 3 && (TS == 2 || IsF8<T>::value)) || ND == 2);
};

struct ConvArgs {
    const void *in, *wp;
    const float* bias;
    const void* mask;
    void* out;
    ConvGeom g;
    int act;
    void* ws;
    size_t ws_bytes;
    hipStream_t stream;
    float acc_scale = 1.f, out_scale = 1.f;
    F8Side f8 = F8Side{nullptr, nullptr, nullptr};
    UpVariant var = UpVariant{};
    float gate_slope = 0.f;     // GATED launches only: `mask` is the gate, the value where it is not positive is multiplied by this instead of zeroed
};

template <typename T, int ND, bool UP, bool WIDE, int EPI, int KH, typename TO, int XB = 1, bool GATED = false>
int launch_data_epi(const ConvArgs& a) {
    using F = DataForm<T, ND, UP, WIDE>;
    using TL = Tile<ND, F::BM>;
    ConvGeom g = a.g;
    constexpr int ID = (ND == 3) ? (UP ? TL::TD + 1 : 2 * TL::TD + 2) : 1;
    constexpr int IH = UP ? TL::TH + 1 : 2 * TL::TH + 2;
    constexpr int FB = 8 * sizeof(T);
    constexpr size_t LDS_MAIN = (size_t)2 * KH * (UP ? 1 : 2) * ID * IH * HaloPitch<ND, UP>::RS * FB + (F::BD ? 0 : (size_t)2 * 4 * KH * 2 * F::BN * FB);
    constexpr size_t LDS_X = F::TS == 2 ? (size_t)F::WM * F::WN * F::TS * (F::MI / 2) * F::NI * 16 * 64 * sizeof(float) : 0;      // the K split's accumulator exchange
    constexpr size_t LDS = LDS_MAIN > LDS_X ? LDS_MAIN : LDS_X;
    static_assert(LDS <= CVAE_LDS_MAX, "LDS tile exceeds the 160 KiB of a CDNA4 CU");
    const int md = UP ? ((ND == 3) ? (g.ld + 1) / 2 : 1) : g.sd, mh = UP ? (g.lh + 1) / 2 : g.sh, mw = UP ? (g.lw + 1) / 2 : g.sw;
    if constexpr (F::XPAIR && XB == 1) {
        // a layer at most half a tile wide, on a launch that fills the chip several times over (the decode sweep's 4^3 -> 8^3 layer; round 3: the 7 x 7 grids of the
        // MNIST model at batch 1024, where one image fills 49 of a tile's 128 positions, in both directions): two samples per tile
        const long long wgs = (long long)((md + TL::TD - 1) / TL::TD) * ((mh + TL::TH - 1) / TL::TH) * ((UP ? g.Cl : g.Cs) / F::BN) * (UP ? (ND == 3 ? 8 : 4) : 1) * g.B;
        if (mw <= TL::TW / 2 && g.B >= 2 && (a.var.xpair == 1 || (a.var.xpair < 0 && wgs >= (ND == 3 ? XPAIR_MIN_WGS : XPAIR_2D_MIN_WGS))))
            return launch_data_epi<T, ND, UP, WIDE, EPI, KH, TO, 2, GATED>(a);
    }
    constexpr auto kern = [] {                               // GATED: the second instance of the same text (conv_data_kernel.inc), one more argument
        if constexpr (GATED) return conv_data_gated_kernel<T, ND, UP, F::WM, F::WN, F::MI, F::NI, EPI, KH, TO, F::BD, F::TS, XB>;
        else return conv_data_kernel<T, ND, UP, F::WM, F::WN, F::MI, F::NI, EPI, KH, TO, F::BD, F::TS, XB>;
    }();
    if (cvae_allow_lds<kern>(LDS) != CVAE_OK) return CVAE_E_LAUNCH;
    g.tiles_d = (md + TL::TD - 1) / TL::TD; g.tiles_h = (mh + TL::TH - 1) / TL::TH; g.tiles_w = (mw + TL::TW - 1) / TL::TW;
    const int Cout = UP ? g.Cl : g.Cs, Cin = (UP ? g.Cs : g.Cl) / (IsF8<T>::value ? 2 : 1);
    const int npar = UP ? ((ND == 3) ? 8 : 4) : 1;
    const long long tiles = (long long)g.tiles_d * g.tiles_h * g.tiles_w;
    long long gy = (long long)(Cout / F::BN) * npar;
    const int64_t total = (int64_t)g.B * (UP ? (int64_t)g.ld * g.lh * g.lw : (int64_t)g.sd * g.sh * g.sw) * Cout;
    int ksplit = pick_ksplit(UP, tiles * gy * g.B, Cin / (16 * KH));
    if (!a.ws || a.ws_bytes < (size_t)ksplit * total * sizeof(float)) ksplit = 1;     // no (or too small a) workspace: unsplit
    if (IsF8<T>::value && sizeof(TO) != 2) ksplit = 1;       // the finish pass writes bf16
    gy *= ksplit;
    if (gy > 65535 || g.B > 65535) return CVAE_E_BADSHAPE;
    dim3 grid((unsigned)tiles, (unsigned)gy, (unsigned)((g.B + XB - 1) / XB));
    if constexpr (GATED)
        hipLaunchKernelGGL(kern, grid, dim3(F::WM * F::WN * F::TS * 64), LDS, a.stream, (const T*)a.in, (const T*)a.wp, a.bias, (const TO*)a.mask, (TO*)a.out, g, a.act,
                           (float*)a.ws, ksplit, a.acc_scale, a.out_scale, a.f8, a.gate_slope);
    else
        hipLaunchKernelGGL(kern, grid, dim3(F::WM * F::WN * F::TS * 64), LDS, a.stream, (const T*)a.in, (const T*)a.wp, a.bias, (const TO*)a.mask, (TO*)a.out, g, a.act,
                           (float*)a.ws, ksplit, a.acc_scale, a.out_scale, a.f8);
    CVAE_CHECK_LAUNCH();
    if constexpr (sizeof(TO) != 1) if (ksplit > 1) {
        const dim3 fgrid((unsigned)((total / 8 + 255) / 256));
        if constexpr (GATED)                                 // unreachable today: GATED launches are `up` launches, and pick_ksplit returns 1 for every `up`
            hipLaunchKernelGGL((conv_splitk_finish_gated_kernel<TO, EPI>), fgrid, dim3(256), 0, a.stream, (const float*)a.ws, a.bias, (const TO*)a.mask, (TO*)a.out, total,
                               Cout, ksplit, a.act, 1.f, a.out_scale, a.f8, a.gate_slope);
        else
            hipLaunchKernelGGL((conv_splitk_finish_kernel<TO, EPI>), fgrid, dim3(256), 0, a.stream, (const float*)a.ws, a.bias,
                               (const TO*)a.mask, (TO*)a.out, total, Cout, ksplit, a.act, IsF8<T>::value ? a.acc_scale : 1.f, a.out_scale, a.f8);
        CVAE_CHECK_LAUNCH();
    }
    return CVAE_OK;
}

// One `down` / `up` product through conv_data_kernel: the form from DataForm, act -> EPI and the stage depth KH lifted here and nowhere else.
template <typename T, int ND, bool UP, bool WIDE, typename TO = T>
int dispatch_conv(const ConvArgs& a) {
    using F = DataForm<T, ND, UP, WIDE>;
    return with_epi(a.act, [&](auto epi) {
        constexpr int EPI = decltype(epi)::value;
        return F::kh(a.g) == 2 ? launch_data_epi<T, ND, UP, WIDE, EPI, F::KH_MAX, TO>(a) : launch_data_epi<T, ND, UP, WIDE, EPI, 1, TO>(a);
    });
}

// The gated `up` product (cvae_conv_down_bwd_data): no bias, no activation (EPI 0), so only the stage depth is lifted.
template <typename T, int ND, bool WIDE>
int dispatch_conv_gated(const ConvArgs& a) {
    using F = DataForm<T, ND, true, WIDE>;
    return F::kh(a.g) == 2 ? launch_data_epi<T, ND, true, WIDE, 0, F::KH_MAX, T, 1, true>(a) : launch_data_epi<T, ND, true, WIDE, 0, 1, T, 1, true>(a);
}

// Workspace the split-K path of dispatch_conv would use for this geometry (0: the launch fills the chip without it).  The tile extents do not depend on the dtype.
template <int ND, bool UP, bool WIDE>
size_t data_workspace_bytes(const ConvGeom& g) {
    using F = DataForm<float, ND, UP, WIDE>;
    static_assert(F::BM == DataForm<bf16, ND, UP, WIDE>::BM && F::BN == DataForm<bf16, ND, UP, WIDE>::BN, "one workspace size for both dtypes");
    using TL = Tile<ND, F::BM>;
    const int md = UP ? ((ND == 3) ? (g.ld + 1) / 2 : 1) : g.sd, mh = UP ? (g.lh + 1) / 2 : g.sh, mw = UP ? (g.lw + 1) / 2 : g.sw;
    const long long tiles = (long long)((md + TL::TD - 1) / TL::TD) * ((mh + TL::TH - 1) / TL::TH) * ((mw + TL::TW - 1) / TL::TW);
    const int Cout = UP ? g.Cl : g.Cs, Cin = UP ? g.Cs : g.Cl;
    const int npar = UP ? ((ND == 3) ? 8 : 4) : 1;
    const int ksplit = pick_ksplit(UP, tiles * (Cout / F::BN) * npar * g.B, Cin / 16);
    if (ksplit <= 1) return 0;
    return (size_t)ksplit * g.B * (UP ? (size_t)g.ld * g.lh * g.lw : (size_t)g.sd * g.sh * g.sw) * Cout * sizeof(float);
}


// ---------------------------------------------------------------------------------------------- up, whole-K halo ("up_full")
// The transposed conv has only 2^nd taps per output parity, so one 16- or 32-channel stage of conv_data_kernel<UP> feeds 16-32 MFMAs per wave
// between two barriers and a global->LDS round trip: the layers with few input channels spend more time staging than multiplying (stamp probes:
// ~3.7 k cycles per stage for 2.7 k cycles of taps on dec1's forward; enc2's backward-data ran at 480 TFLOP/s).  Here the (T + 2)^nd halo of the
// q tile is staged ONCE for ALL input channels (Cin = 16 KCH) and serves every parity class the workgroup owns (`ppw` of the 2^nd; the rest go to
// sibling workgroups when the grid is small).  The weights of a parity come through LDS in half panels (2^nd / 2 taps x all k-steps, two
// buffers, ONE barrier per half panel, fetched two half panels ahead: a per-wave fetch of the same fragments by every wave ran into the
// L2 -> L1 bandwidth, 22 B/clk/CU).  What the stamp probes and the ISA showed about the inner loop, with one wave per SIMD:
//   * the compiler sinks every ds_read to just in front of the MFMA that uses it (read / s_waitcnt / MFMA per step): the reads are issued
//     APIPE steps ahead by hand and pinned with sched_barrier;
//   * with in-order issue every non-MFMA instruction between two MFMAs costs issue time the MFMA pipe idles for once there are more than
//     ~6 per MFMA: the LDS image is position-major ([halo slot][8-channel piece], pitch NPC + 1 pieces: the odd pitch keeps the reads
//     conflict-free exactly as the plane-major image did, and the pieces of one position, stored by consecutive lanes, hit different banks),
//     so that every read of a parity is `ds_read_b128 base, offset:imm` off two per-parity base registers — no address VALU in the loop;
//   * bias and the ReLU mask of a parity are fetched before its taps, not in the epilogue.
#define CONV_GATED 0
#include "conv_up_full_kernel.inc"
#undef CONV_GATED
#define CONV_GATED 1
#include "conv_up_full_kernel.inc"
#undef CONV_GATED

template <typename T, int ND, int WM, int WN, int MI, int NI, int KCH> constexpr size_t up_full_lds_bytes() {
    using TL = Tile<ND, WM * MI * 32>;
    constexpr int ID = (ND == 3) ? TL::TD + 2 : 1, IH = TL::TH + 2;
    return ((size_t)(ID * IH * HaloPitch<ND, true>::RS) * (2 * KCH + 1) + (size_t)2 * (((ND == 3) ? 8 : 4) / 2) * KCH * 2 * (WN * NI * 32)) * 8 * sizeof(T);
}

// Launch of conv_up_full_kernel; CVAE_E_UNSUPPORTED when this channel count does not fit the LDS or the grid is below UPFULL_MIN_GRID (the caller falls back
// to dispatch_conv<UP>).  Only the 32-channel tile form (DataForm<.., WIDE = false>) goes here: on 64-channel tiles the kernel measured slower than
// conv_data_kernel<UP> with BD.
template <typename T, int ND, int KCH, bool GATED = false>
int launch_up_full(const ConvArgs& a) {
    using F = DataForm<T, ND, true, false>;
    constexpr int WM = F::WM, WN = F::WN, MI = F::MI, NI = F::NI;
    constexpr size_t LDS = up_full_lds_bytes<T, ND, WM, WN, MI, NI, KCH>();
    if constexpr (LDS > CVAE_LDS_MAX || (KCH * 2 * F::BN) % (WM * WN * 64) != 0) {
        return CVAE_E_UNSUPPORTED;
    } else {
        using TL = Tile<ND, F::BM>;
        ConvGeom g = a.g;
        const int md = (ND == 3) ? (g.ld + 1) / 2 : 1, mh = (g.lh + 1) / 2, mw = (g.lw + 1) / 2;
        g.tiles_d = (md + TL::TD - 1) / TL::TD; g.tiles_h = (mh + TL::TH - 1) / TL::TH; g.tiles_w = (mw + TL::TW - 1) / TL::TW;
        const long long tiles = (long long)g.tiles_d * g.tiles_h * g.tiles_w;
        const int npar = (ND == 3) ? 8 : 4, nblocks = g.Cl / F::BN;
        if (a.var.upfull == 0 || (a.var.upfull < 0 && tiles * nblocks * g.B < UPFULL_MIN_GRID)) return CVAE_E_UNSUPPORTED;
        // parity classes per workgroup: all of them (one halo stage per tile) once the grid has ~2 workgroups per CU without splitting them
        int psplit = 1;
        while (psplit < npar && tiles * nblocks * g.B * psplit < UPFULL_MIN_WG) psplit *= 2;
        const long long gy = (long long)nblocks * psplit;
        if (gy > 65535 || g.B > 65535) return CVAE_E_BADSHAPE;
        dim3 grid((unsigned)tiles, (unsigned)gy, (unsigned)g.B), block(WM * WN * 64);
        if constexpr (GATED) {                               // cvae_conv_down_bwd_data: no bias, no activation (EPI 0)
            constexpr auto kern = conv_up_full_gated_kernel<T, ND, WM, WN, MI, NI, KCH, 0, T>;
            if (cvae_allow_lds<kern>(LDS) != CVAE_OK) return CVAE_E_LAUNCH;
            hipLaunchKernelGGL(kern, grid, block, LDS, a.stream, (const T*)a.in, (const T*)a.wp, a.bias, (const T*)a.mask, (T*)a.out, g, a.act, npar / psplit,
                               a.acc_scale, a.out_scale, a.gate_slope);
            CVAE_CHECK_LAUNCH();
            return CVAE_OK;
        } else
        return with_epi(a.act, [&](auto epi) {
            constexpr auto kern = conv_up_full_kernel<T, ND, WM, WN, MI, NI, KCH, decltype(epi)::value, T>;
            if (cvae_allow_lds<kern>(LDS) != CVAE_OK) return CVAE_E_LAUNCH;
            hipLaunchKernelGGL(kern, grid, block, LDS, a.stream, (const T*)a.in, (const T*)a.wp, a.bias, (const T*)a.mask, (T*)a.out, g, a.act, npar / psplit,
                               a.acc_scale, a.out_scale);
            return launch_rc();
        });
    }
}

// `up` through the whole-K kernel when the input channel count is one it is built for (64 / 128 / 256 where the halo fits): CVAE_E_UNSUPPORTED otherwise.
template <typename T, int ND, bool GATED = false>
int try_up_full(const ConvArgs& a) {
    if (a.g.Cs == 64) return launch_up_full<T, ND, 4, GATED>(a);
    if (a.g.Cs == 128) return launch_up_full<T, ND, 8, GATED>(a);
    if (a.g.Cs == 256) return launch_up_full<T, ND, 16, GATED>(a);
    return CVAE_E_UNSUPPORTED;
}

// ---------------------------------------------------------------------------------------------- weight packing
// CH: input channels per panel chunk — 16 (bf16 / fp32: one MFMA k-step) or 32 (fp8: the f8x2 element is two channels, so a chunk of 16
// elements is 32 channels; see Frag<f8x2>)
template <typename T, int CH = 16>
__global__ void pack_weight_kernel(const float* __restrict__ w, T* __restrict__ out, int Cs, int Cl, int taps, int for_up, float mul = 1.f) {
    const int64_t n = (int64_t)Cs * Cl * taps;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        // i enumerates the OUTPUT so writes are contiguous
        const int e = (int)(i % CH);
        int64_t rr = i / CH;
        int cs, cl, tap;
        if (!for_up) { cs = (int)(rr % Cs); rr /= Cs; const int ch = (int)(rr % (Cl / CH)); tap = (int)(rr / (Cl / CH)); cl = ch * CH + e; }
        else { cl = (int)(rr % Cl); rr /= Cl; const int ch = (int)(rr % (Cs / CH)); tap = (int)(rr / (Cs / CH)); cs = ch * CH + e; }
        out[i] = from_f32<T>(sizeof(T) == 1 ? w[((int64_t)cs * Cl + cl) * taps + tap] * mul : w[((int64_t)cs * Cl + cl) * taps + tap]);
    }
}

// fp8 panels of several layers in one launch, scales read from DEVICE memory (a captured training step re-reads them on every replay), and the
// largest |w| of every layer recorded for the next step's scale (delayed scaling: cvae_fp8_scale_update).
#define F8PACK_MAX 12
struct F8PackTable {
    const float* w[F8PACK_MAX];
    fp8* out[F8PACK_MAX];
    const float* inv_scale[F8PACK_MAX];      // device: 1 / s_w
    unsigned* amax[F8PACK_MAX];              // device: CVAE_AMAX_SLOTS words, or null
    int Cs[F8PACK_MAX], Cl[F8PACK_MAX], for_up[F8PACK_MAX], blk_start[F8PACK_MAX + 1];
    int count, taps;
};
__global__ __launch_bounds__(256) void pack_weight_fp8_multi_kernel(F8PackTable tb) {
    constexpr int CH = 32;
    int ti = 0;
    while (ti + 1 < tb.count && (int)blockIdx.x >= tb.blk_start[ti + 1]) ++ti;
    const int Cs = tb.Cs[ti], Cl = tb.Cl[ti], taps = tb.taps, for_up = tb.for_up[ti];
    const float* w = tb.w[ti];
    fp8* out = tb.out[ti];
    const float mul = tb.inv_scale[ti][0];
    const int64_t n = (int64_t)Cs * Cl * taps;
    const int nb = tb.blk_start[ti + 1] - tb.blk_start[ti];
    float amx = 0.f;
    for (int64_t i = (((int64_t)blockIdx.x - tb.blk_start[ti]) * 256 + threadIdx.x) * 4; i < n; i += (int64_t)nb * 1024) {      // 4 consecutive codes per thread: one dword store
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t iu = i + u;
            const int e = (int)(iu % CH);
            int64_t rr = iu / CH;
            int cs, cl, tap;
            if (!for_up) { cs = (int)(rr % Cs); rr /= Cs; const int ch = (int)(rr % (Cl / CH)); tap = (int)(rr / (Cl / CH)); cl = ch * CH + e; }
            else { cl = (int)(rr % Cl); rr /= Cl; const int ch = (int)(rr % (Cs / CH)); tap = (int)(rr / (Cs / CH)); cs = ch * CH + e; }
            v[u] = w[((int64_t)cs * Cl + cl) * taps + tap];
            amx = fmaxf(amx, fabsf(v[u]));
            v[u] = __builtin_amdgcn_fmed3f(v[u] * mul, -CVAE_FP8_MAX, CVAE_FP8_MAX);
        }
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], c, true);
        *(int*)(out + i) = c;
    }
    __shared__ float red[4];
    if (tb.amax[ti]) amax_publish_wg(tb.amax[ti], amx, blockIdx.x, red);
}

// Delayed scaling, once per step: every tracked tensor i gets scale[i] = headroom * amax_i / 448 from the largest value recorded since the last
// call (its slots are cleared; a tensor that recorded nothing keeps its scale), then every fp8 layer l its pair {s_in * s_w, 1 / s_out}.
#define F8LAYER_MAX 16
struct F8LayerIdx { int in[F8LAYER_MAX], w[F8LAYER_MAX], out[F8LAYER_MAX]; int count; };
// One workgroup per tracked tensor reduces that tensor's record (a single workgroup reading all of them ran at one CU's load rate: 11.6 us for 12 tensors).
// The per-layer pairs need EVERY scale: the workgroup whose ticket add comes last computes them.  Hand-off per MI355X_MICROARCH.md (visibility, valid forms):
// every scale is written by an agent-scope (sc1) atomic store, the writing lane drains it (s_waitcnt vmcnt(0)) before its agent-scope ticket add, and the last
// arriver — told by the value its add returned — reads the scales with agent-scope atomic loads, never through its L1.  `ticket` is one device word that the
// last arriver resets, so a replayed graph finds it zero.
__global__ __launch_bounds__(1024) void fp8_scale_update_kernel(unsigned* __restrict__ amax, float* __restrict__ scale, float* __restrict__ inv_scale, int n, float headroom,
                                                                F8LayerIdx li, float* __restrict__ dscale, unsigned* __restrict__ ticket) {
    static_assert(CVAE_AMAX_SLOTS == 4096, "one uint4 per thread");
    __shared__ float red[16];
    __shared__ unsigned last;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = blockIdx.x;
    uint4* a4 = (uint4*)amax + (size_t)i * (CVAE_AMAX_SLOTS / 4);
    const uint4 v = a4[t];
    a4[t] = make_uint4(0u, 0u, 0u, 0u);
    float a = fmaxf(fmaxf(__uint_as_float(v.x), __uint_as_float(v.y)), fmaxf(__uint_as_float(v.z), __uint_as_float(v.w)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));         // not wave_max(): see amax_publish_wg (common.h)
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (t == 0) {
        float m = 0.f;
        for (int w_ = 0; w_ < 16; ++w_) m = fmaxf(m, red[w_]);
        if (m > 0.f) {
            const float s_ = headroom * m / CVAE_FP8_MAX;
            __hip_atomic_store(scale + i, s_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(inv_scale + i, 1.f / s_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores have left this CU before the ticket says so
        const unsigned got = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (got == (unsigned)n - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (last && li.count > 0) {
        if (t < li.count) {
            const float si = __hip_atomic_load(scale + li.in[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float sw = __hip_atomic_load(scale + li.w[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dscale[2 * t] = si * sw;
            dscale[2 * t + 1] = li.out[t] >= 0 ? 1.f / __hip_atomic_load(scale + li.out[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        }
    }
    if (last && t == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// max |x| of a tensor into CVAE_AMAX_SLOTS words (calibration of the first step's scales; the training step records its amax in the producers' epilogues)
__global__ __launch_bounds__(256) void absmax_kernel(const void* __restrict__ src, int dtype, int64_t n, unsigned* __restrict__ slots) {
    float amx = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        amx = fmaxf(amx, fabsf(dtype == CVAE_BF16 ? to_f32(((const bf16*)src)[i]) : ((const float*)src)[i]));
    __shared__ float red[4];
    amax_publish_wg(slots, amx, blockIdx.x, red);
}

// Both directions of every weight in one launch, through an LDS transpose: a block takes a 16 cs x 16 cl x 16 taps tile of one fp32
// master (64-byte runs, float4 loads), and writes the `down` panel ([tap][cl / 16][cs][16 cl]) and the `up` panel
// ([tap][cs / 16][cl][16 cs]) in 512-byte (bf16) runs — the gather form above reads every source line 16 times.  3D weights
// (64 taps) take 4 blocks per (cs, cl) tile: ~1300 small blocks for the model instead of ~330 long ones.
#define PAIR_MAX 16
struct PairTable {
    const float* w[PAIR_MAX];
    void* down[PAIR_MAX];
    void* up[PAIR_MAX];
    int Cs[PAIR_MAX], Cl[PAIR_MAX], blk_start[PAIR_MAX + 1];
    int count;
    // fp8 training forward: f8dir 1 / 2 = the `down` / `up` panel of this weight is written as fp8 codes of w * *inv_scale ([tap][C_in / 32][C_out][32],
    // into f8out) INSTEAD of its bf16 panel (the forward product reads the fp8 one; the other direction serves the bf16 backward pass); amax records max |w|
    int f8dir[PAIR_MAX];
    fp8* f8out[PAIR_MAX];
    const float* inv_scale[PAIR_MAX];
    unsigned* amax[PAIR_MAX];
};
template <typename T, int TAPS>
__global__ __launch_bounds__(256) void pack_weight_pairs_kernel(PairTable tb) {
    constexpr int TT = 16, TSPLIT = TAPS / TT, TP = TT + 1;
    __shared__ float tile[16 * 17 * TP];                     // [(cs * 17 + cl)][tap]
    int ti = 0;
    while (ti + 1 < tb.count && (int)blockIdx.x >= tb.blk_start[ti + 1]) ++ti;
    const int Cs = tb.Cs[ti], Cl = tb.Cl[ti];
    int blk = (int)blockIdx.x - tb.blk_start[ti];
    const int tq = blk % TSPLIT; blk /= TSPLIT;
    const int nclt = Cl / 16, ncst = Cs / 16;
    const int cst = blk / nclt, clt = blk % nclt, cs0 = cst * 16, cl0 = clt * 16;
    const float* w = tb.w[ti];
    const int f8dir = tb.f8dir[ti];
    float amx = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int i = threadIdx.x + it * 256, f = i & 3, cl = (i >> 2) & 15, cs = i >> 6;
        const float4 v = *(const float4*)(w + ((size_t)(cs0 + cs) * Cl + cl0 + cl) * TAPS + tq * TT + 4 * f);
        float* d = tile + (cs * 17 + cl) * TP + 4 * f;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        amx = fmaxf(fmaxf(amx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    __syncthreads();
    T* od = (T*)tb.down[ti];
    T* ou = (T*)tb.up[ti];
    const float mul8 = f8dir ? tb.inv_scale[ti][0] : 1.f;
    // per tap both panels are 256 contiguous elements ([16][16]); a thread writes 8 of them (16 bytes bf16) for one of 8 taps at a time
    const int tg = threadIdx.x >> 5, e0 = (threadIdx.x & 31) * 8, a = e0 >> 4, b0 = e0 & 15;
#pragma unroll
    for (int tl = tg; tl < TT; tl += 8) {
        const int tap = tq * TT + tl;
        __attribute__((aligned(16))) T vd[8], vu[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            vd[q] = from_f32<T>(tile[(a * 17 + b0 + q) * TP + tl]);              // down: (cs = a, cl = b0 + q)
            vu[q] = from_f32<T>(tile[((b0 + q) * 17 + a) * TP + tl]);            // up:   (cl = a, cs = b0 + q)
        }
        T* pd = od + ((size_t)(tap * nclt + clt) * Cs + cs0 + a) * 16 + b0;
        T* pu = ou + ((size_t)(tap * ncst + cst) * Cl + cl0 + a) * 16 + b0;
        constexpr int NU = (8 * sizeof(T)) / 16;
        if (f8dir != 1) {
#pragma unroll
            for (int u = 0; u < NU; ++u) ((uint4*)pd)[u] = ((const uint4*)vd)[u];
        }
        if (f8dir != 2) {
#pragma unroll
            for (int u = 0; u < NU; ++u) ((uint4*)pu)[u] = ((const uint4*)vu)[u];
        }
        if (f8dir) {                                         // 32-channel chunks: this 16-wide tile is one half of a chunk row
            float v8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v8[q] = f8dir == 1 ? tile[(a * 17 + b0 + q) * TP + tl] : tile[((b0 + q) * 17 + a) * TP + tl];
            fp8* p8 = f8dir == 1 ? tb.f8out[ti] + ((size_t)(tap * (Cl / 32) + (cl0 >> 5)) * Cs + cs0 + a) * 32 + (cl0 & 16) + b0
                                 : tb.f8out[ti] + ((size_t)(tap * (Cs / 32) + (cs0 >> 5)) * Cl + cl0 + a) * 32 + (cs0 & 16) + b0;
            *(uint2*)p8 = pack8_fp8(v8, mul8);
        }
    }
    if (f8dir && tb.amax[ti]) {                              // uniform over the workgroup
        __syncthreads();
        amax_publish_wg(tb.amax[ti], amx, blockIdx.x, tile);
    }
}

// ---------------------------------------------------------------------------------------------- wgrad
// Workgroup: 8 waves; block of 64 cs x 32 cl; one depth tap kd (3D) / all taps (2D); wave w owns kh = w & 3, kw = 0..3 and
// the 32-row half sg = w >> 2 of the cs block: 4 accumulator tiles (64 VGPRs), so two workgroups (16 waves) fit a CU with the
// next tile's global loads held in registers during the MFMA phase.
// Several layers can share ONE launch (cvae_conv_wgrad_multi: the deferred weight gradients of a whole backward pass): the grid is the
// concatenation of the per-layer grids and a workgroup finds its layer in the table that rides in the kernel arguments.  The small layers
// (a handful of tiles each, latency-bound on their own) then run in the shadow of the large ones instead of each paying a launch.
#define WG_MULTI_MAX 8
struct WgradEntry {
    const void* S; const void* L; float* ws; float* bias_ws;
    ConvGeom g;
    int n_split, cb, tg, bias_mode;
    int xb;             // 2D layers at most TW / 2 wide: two samples per tile, side by side in x (the 7 x 7 maps of the MNIST model fill 49 of a tile's 128 positions)
    float* dW;          // n_split == 1: the group's only slab IS the sum, so the workgroup stores it into dW[Cs][Cl][taps] itself (nullptr: slab + reduce pass)
};
struct WgradTable { WgradEntry e[WG_MULTI_MAX]; int blk_start[WG_MULTI_MAX + 1]; int count; };

template <typename T, int ND>
__global__ __launch_bounds__(512, sizeof(T) == 2 ? 4 : 2) void conv_wgrad_kernel(WgradTable tb) {
    int ti = 0;
    while (ti + 1 < tb.count && (int)blockIdx.x >= tb.blk_start[ti + 1]) ++ti;
    const T* __restrict__ S = (const T*)tb.e[ti].S;
    const T* __restrict__ L = (const T*)tb.e[ti].L;
    float* __restrict__ ws = tb.e[ti].ws;
    float* __restrict__ bias_ws = tb.e[ti].bias_ws;
    const ConvGeom g = tb.e[ti].g;
    const int n_split = tb.e[ti].n_split, bias_mode = tb.e[ti].bias_mode, grid_y = tb.e[ti].cb;
    const int xb = (ND == 2) ? tb.e[ti].xb : 0;
    // the layer's own grid (n_split, cb, tg), x fastest
    int lb = (int)blockIdx.x - tb.blk_start[ti];
    const int bx = lb % n_split; lb /= n_split;
    const int by = lb % grid_y, bz = lb / grid_y;
    using TL = Tile<ND, 128>;
    constexpr int NT = 512;
    constexpr int TD = TL::TD, TH = TL::TH, TW = TL::TW;
    // L tile: TD planes (one kd) x IH x IW positions x 32 cl.  2D: two more columns, so that two samples' halos (2 (TW / 2) + 2 columns each) fit side by side (xb)
    constexpr int IW1 = 2 * TW + 2, IW = IW1 + (ND == 2 ? 2 : 0), IH = 2 * TH + 2;
    constexpr int SROW = 64 * sizeof(T), LROW = 32 * sizeof(T);
    constexpr int S_BYTES = 128 * SROW;
    constexpr int FB = 8 * sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* s_lds = smem;
    char* l_lds = smem + S_BYTES;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int cl_blocks = g.Cl / 32;
    const int cs0 = (by / cl_blocks) * 64, cl0 = (by % cl_blocks) * 32;
    const int kd = (ND == 3) ? bz : 0;
    const int kh = wave & 3, sg = wave >> 2;
    // Bank-conflict-free LDS images for the transposing reads.  One 32-lane group of ds_read_b64_tr_b16 reads 4 k-rows x 64
    // bytes = the whole 256-byte bank row, provided the 4 rows sit in 4 different 64-byte quarters.  The k-rows of a group are 4
    // consecutive output positions m .. m+3 along w.  S image (128-byte rows): the 64-byte halves of row m are swapped when bit 1
    // of m is set.  L image (64-byte rows): the stride-2 input columns x = 2 w + kw are split into an even-x and an odd-x plane,
    // so consecutive w are consecutive rows of plane kw & 1 and every tap is a constant row offset (kw >> 1).
    constexpr int LHALF = IW / 2, LPLANE = TD * IH * LHALF;  // rows per line / per parity plane
    auto s_byte = [](int m, int c) -> int { return m * SROW + ((((c >> 3) ^ (((m >> 1) & 1) << 2)) << 3) + (c & 7)) * (int)sizeof(T); };
    auto l_row = [](int line, int x) -> int { return (x & 1) * LPLANE + line * LHALF + (x >> 1); };
    const int tiles_per_b = g.tiles_d * g.tiles_h * g.tiles_w, total_tiles = (xb ? (g.B + 1) / 2 : g.B) * tiles_per_b;
    STAMP_BEGIN();                                           // a 1D grid: stamp_wg = blockIdx.x
#ifdef CVAE_STAMP
    int stamp_it = 0;
#endif

    f32x16 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;

    // Bias gradients ride along (no separate channel-sum pass over the gradient tensor): bias_mode 1 = per-channel sum of S (Conv
    // layers), done by the (cl block 0, kd 0) workgroups from their S tiles; bias_mode 2 = per-channel sum of L (ConvTranspose
    // layers), done by the (cs block 0, kd 1 | 2) workgroups from the non-halo part of their L tiles (kd = 1 sees the even planes,
    // kd = 2 the odd ones; in 2D the single tap group sees the one plane).  Partials go to bias_ws, wgrad_reduce_kernel sums them.
    const bool bias_s = bias_mode == 1 && (by % cl_blocks) == 0 && kd == 0;
    const bool bias_l = bias_mode == 2 && (by / cl_blocks) == 0 && (ND == 2 || kd == 1 || kd == 2);
    float bacc = 0.f;
    // S tile: 128 positions x 64 channels; L tile: planes lz = 2 (o0d + d) - 1 + kd, rows 2 o0h - 1 + y, cols 2 o0w - 1 + x.
    // The global loads of tile i+1 are issued right after tile i has been stored to LDS, so they are in flight during tile i's
    // MFMA phase; out-of-range pieces are loaded from a clamped (valid) address and zeroed when they are stored, which keeps the
    // loads unconditional and straight-line.  Addresses are 32-bit offsets inside one sample (geom_ok bounds the sample size) on a
    // wave-uniform 64-bit base.
    // Which pieces a thread moves does not depend on the tile, so everything but the tile origin is worked out once:
    //  S: pass i of thread t is the 8-channel piece t & 7 of position m = (t >> 3) + 64 i: the same w, and (hh, d) a compile-time step further;
    //  L: thread t keeps ONE column-piece cp = t % (4 IW) = (x, piece) and takes the lines lg + LG i, lg = t / (4 IW): x, its clamp, its ok bit and
    //     the sample half are per tile, a pass adds the line's (d, y) — a constant plus one carry — two clamps and one multiply-add chain.
    // The LDS destination of pass i is a per-thread base plus a compile-time offset.  What a thread needs of this rides in ONE packed
    // register (lpk) across the MFMA phase; the kernel sits at the 128-VGPR cap and eight hoisted offsets spill.
    constexpr int SN = (128 * 8) / NT, MSTEP = NT / 8;
    constexpr int S_HSTEP = (MSTEP / TW) % TH, S_DSTEP = MSTEP / (TW * TH);          // (hh, d) of position m + MSTEP against m
    static_assert(MSTEP % TW == 0 && (MSTEP / TW < TH ? MSTEP / TW : TH) - 1 + (SN - 1) * S_HSTEP < TH, "S passes step (hh, d) without carries");
    constexpr int LCP = IW * 4, LG = NT / LCP;                                       // column-pieces of a line; lines per pass
    constexpr int NLINES = TD * IH, LN = (NLINES + LG - 1) / LG, LN_FULL = NLINES / LG;
    static_assert(LG >= 1 && LG <= IH && LG <= 7 && LN <= 7 && IW <= 64, "lpk fields; a pass carries into d at most once");
    static_assert(((LPLANE + LG * LHALF + LHALF) * 4 + 3) * FB < 65536, "the L image offset of a thread's first line fits 16 bits");
    Piece<T> sp[SN], lp[LN];
    unsigned okmask = 0;
    const int s_sample = g.sd * g.sh * g.sw * g.Cs, l_sample = g.ld * g.lh * g.lw * g.Cl;
    unsigned lpk;       // [0, 16) byte offset of (line lg, x, piece) in the L image; [16, 22) x; [22, 24) piece; [24, 27) lg; [27, 30) passes that store (0: a spare thread)
    {
        const int cp = t % LCP, lg = t / LCP, x = cp >> 2, piece = cp & 3;
        const int nl = lg < LG ? (NLINES - lg + LG - 1) / LG : 0;
        lpk = (unsigned)((l_row(lg, x) * 4 + piece) * FB) | (unsigned)x << 16 | (unsigned)piece << 22 | (unsigned)lg << 24 | (unsigned)nl << 27;
    }
    // the tile walk bx, bx + n_split, ... as digits (pair of samples, td, th, tw): load_tile adds the digits of n_split with carries
    int nx_tw, nx_th, nx_td, nx_b, st_tw, st_th, st_td, st_b;
    {
        int r = bx;
        nx_tw = r % g.tiles_w; r /= g.tiles_w; nx_th = r % g.tiles_h; r /= g.tiles_h; nx_td = r % g.tiles_d; nx_b = r / g.tiles_d;
        r = n_split;
        st_tw = r % g.tiles_w; r /= g.tiles_w; st_th = r % g.tiles_h; r /= g.tiles_h; st_td = r % g.tiles_d; st_b = r / g.tiles_d;
    }
    auto load_tile = [&]() {                                 // issues the loads of tile (nx_b, nx_td, nx_th, nx_tw), then steps to the workgroup's next tile
        const int b = nx_b * (1 + xb);                       // xb: samples b (tile columns 0 .. TW / 2 - 1) and b + 1 (the other half)
        const int o0d = nx_td * TD, o0h = nx_th * TH, o0w = nx_tw * TW;
        const T* Sb = S + (size_t)b * s_sample + cs0;
        const T* Lb = L + (size_t)b * l_sample + cl0;
        const bool b1ok = b + 1 < g.B;
        okmask = 0;
        int tz = t;
        unsigned pk = lpk;
        asm volatile("" : "+v"(tz), "+v"(pk));               // opaque: the unpacked fields live only inside the call (hoisted, they spill)
        {
            const int piece = tz & 7, m0 = tz >> 3;
            const int w = m0 % TW, hh0 = m0 / TW % TH, d0 = m0 / (TW * TH);
            const int sx = (xb && w >= TW / 2) ? 1 : 0;
            const int ow = o0w + w - sx * (TW / 2);
            const bool okw = (ow < g.sw) & (!sx | b1ok);
            const unsigned cw = (unsigned)(min(ow, g.sw - 1) * g.Cs + piece * 8) + ((sx && b1ok) ? (unsigned)s_sample : 0u);
            const unsigned s_line = (unsigned)(g.sw * g.Cs);
#pragma unroll
            for (int i = 0; i < SN; ++i) {
                const int od = o0d + d0 + i * S_DSTEP, oh = o0h + hh0 + i * S_HSTEP;
                const bool ok = (od < g.sd) & (oh < g.sh) & okw;
                const unsigned off = (unsigned)(min(od, g.sd - 1) * g.sh + min(oh, g.sh - 1)) * s_line + cw;
                piece_load_raw<T>(sp[i], Sb + off);
                okmask |= (unsigned)ok << i;
            }
        }
        {
            const int x = (pk >> 16) & 63, piece = (pk >> 22) & 3, lg = (pk >> 24) & 7;
            const int sx = (xb && x >= IW / 2) ? 1 : 0;
            const int lx = 2 * o0w - 1 + x - sx * (IW / 2);
            const bool okx = ((unsigned)lx < (unsigned)g.lw) & (!sx | b1ok) & (xb | (x < IW1));
            const unsigned cx = (unsigned)(min(max(lx, 0), g.lw - 1) * g.Cl + piece * 8) + ((sx && b1ok) ? (unsigned)l_sample : 0u);
            const unsigned l_line = (unsigned)(g.lw * g.Cl);
            const int lz0 = 2 * o0d - 1 + kd, ly0 = 2 * o0h - 1;
#pragma unroll
            for (int i = 0; i < LN; ++i) {                   // line lg + LG i = (d, y): lines past the tile (a thread's last pass) load a clamped address and are never stored
                const int dq = (i * LG) / IH, yr = (i * LG) % IH;
                const int carry = (lg + yr >= IH) ? 1 : 0;
                const int lz = (ND == 3) ? lz0 + 2 * (dq + carry) : 0, ly = ly0 + lg + yr - carry * IH;
                const bool ok = ((unsigned)lz < (unsigned)g.ld) & ((unsigned)ly < (unsigned)g.lh) & okx;
                const unsigned off = (unsigned)(min(max(lz, 0), g.ld - 1) * g.lh + min(max(ly, 0), g.lh - 1)) * l_line + cx;
                piece_load_raw<T>(lp[i], Lb + off);
                okmask |= (unsigned)ok << (SN + i);
            }
        }
        nx_tw += st_tw;
        int carry = nx_tw >= g.tiles_w ? 1 : 0;
        nx_tw -= carry ? g.tiles_w : 0;
        nx_th += st_th + carry;
        carry = nx_th >= g.tiles_h ? 1 : 0;
        nx_th -= carry ? g.tiles_h : 0;
        nx_td += st_td + carry;
        carry = nx_td >= g.tiles_d ? 1 : 0;
        nx_td -= carry ? g.tiles_d : 0;
        nx_b += st_b + carry;
    };
    if (bx < total_tiles) load_tile();
    for (int tile = bx; tile < total_tiles; tile += n_split) {
        __syncthreads();                                     // the previous tile's readers are done with both images
#ifdef CVAE_STAMP
        if (stamp_it < 8) STAMP(2 + 3 * stamp_it);
#endif
        {
            int tz = t;
            unsigned pk = lpk;
            asm volatile("" : "+v"(tz), "+v"(pk));           // as in load_tile
            char* sdst = s_lds + s_byte(tz >> 3, (tz & 7) * 8);
#pragma unroll
            for (int i = 0; i < SN; ++i) piece_store_sel<T>(sp[i], (okmask >> i) & 1, sdst + i * MSTEP * SROW);       // s_byte's swizzle has the period 4 in m
            char* ldst = l_lds + (pk & 0xffffu);
            const int nl = (int)(pk >> 27);
            if (nl) {
#pragma unroll
                for (int i = 0; i < LN; ++i)
                    if (i < LN_FULL || nl > i) piece_store_sel<T>(lp[i], (okmask >> (SN + i)) & 1, ldst + i * LG * LHALF * LROW);
            }
        }
        __syncthreads();
#ifdef CVAE_STAMP
        if (stamp_it < 8) STAMP(3 + 3 * stamp_it);
#endif
        if (tile + n_split < total_tiles) load_tile();
        if (bias_s) {                                        // thread (c, pg): 16 of the tile's 128 positions of channel c
            const int c = t & 63, pg = t >> 6;
#pragma unroll 4
            for (int j = 0; j < 16; ++j) bacc += to_f32(*(const T*)(s_lds + s_byte(pg * 16 + j, c)));
        } else if (bias_l) {                                 // thread (c, pg): 32 of the 512 owned (non-halo) positions of channel c
            const int c = t & 31, pg = t >> 5;
#pragma unroll 4
            for (int j = 0; j < 32; ++j) {
                const int pp = pg + 16 * j;
                const int xx = pp % (2 * TW), yy = pp / (2 * TW) % (2 * TH), dd = pp / (4 * TW * TH);
                const int xs = xx + 1 + ((xb && xx >= TW) ? 2 : 0);           // xb: the second sample's own columns start two columns further right
                bacc += to_f32(*(const T*)(l_lds + l_row(dd * IH + yy + 1, xs) * LROW + c * (int)sizeof(T)));
            }
        }
        if constexpr (sizeof(T) == 2) {
            // bf16: transposing LDS reads.  Lane i of 16-lane group gq supplies the address of k-row q = i>>2,
            // 4 channels at 4*(i&3); it receives channel i of the 4 k-rows  (cdna_hip_programming.md T10).
            const int gq = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
            const int hk = gq >> 1, colblk = gq & 1;
            typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
            // k-row of (c, jj): position m = 16 c + r0 with r0 = 8 hk + 4 jj + q.  The lane part (w, hh) = (r0 % TW, r0 / TW) and
            // the c part (hh, d) = (16 c / TW % TH, 16 c / (TW TH)) add without carries, so with the loop fully unrolled every
            // LDS address below is one per-lane base plus a compile-time offset.
            const char* abase[2];
            const char* bbase[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int r0 = 8 * hk + 4 * jj + q;
                abase[jj] = s_lds + s_byte(r0, sg * 32 + 16 * colblk + 4 * p);
                bbase[jj] = l_lds + l_row(2 * (r0 / TW) + kh, 2 * (r0 % TW) + ((xb && (r0 % TW) >= TW / 2) ? 2 : 0)) * LROW + (16 * colblk + 4 * p) * 2;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int hh_c = (16 * c / TW) % TH, d_c = (16 * c) / (TW * TH);
                bf16x8 a;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(abase[jj] + 16 * c * SROW));
                    a[4 * jj + 0] = v[0]; a[4 * jj + 1] = v[1]; a[4 * jj + 2] = v[2]; a[4 * jj + 3] = v[3];
                }
#pragma unroll
                for (int kw = 0; kw < 4; ++kw) {
                    bf16x8 bv;
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const char* bp = bbase[jj] + (((kw & 1) * LPLANE + (d_c * IH + 2 * hh_c) * LHALF + (kw >> 1)) * LROW);
                        const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)bp);
                        bv[4 * jj + 0] = v[0]; bv[4 * jj + 1] = v[1]; bv[4 * jj + 2] = v[2]; bv[4 * jj + 3] = v[3];
                    }
                    acc[kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv, acc[kw], 0, 0, 0);
                }
            }
        } else {
            // fp32: 32x32x2 MFMA, lane (r, h) feeds A[r][k = h], B[k = h][r]: one element each, no transpose needed
            const int r = lane & 31, hk = lane >> 5;
#pragma unroll 1
            for (int mm = 0; mm < 128; mm += 2) {
                const int m = mm + hk;
                const int w = m % TW, hh = m / TW % TH, d = m / (TW * TH);
                const int line = d * IH + 2 * hh + kh;
                const float a = *(const float*)(s_lds + s_byte(m, sg * 32 + r));
#pragma unroll
                for (int kw = 0; kw < 4; ++kw) {
                    const float bv = *(const float*)(l_lds + l_row(line, 2 * w + kw + ((xb && w >= TW / 2) ? 2 : 0)) * LROW + r * 4);
                    acc[kw] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[kw], 0, 0, 0);
                }
            }
        }
#ifdef CVAE_STAMP
        if (stamp_it < 8) STAMP(4 + 3 * stamp_it);
        ++stamp_it;
#endif
    }
    STAMP(26);
    // ---- write-out: this workgroup's partial sums leave as ONE slab [kh][64 cs][32 cl][kw] of plain stores; wgrad_reduce_kernel sums the slabs
    // (fp32 atomics here cost more than the MFMA phase: 67 MB of adds at < 1 TB/s).  A group with a single slab writes dW itself ----
    if (bias_s || bias_l) {                                   // block-uniform
        __syncthreads();                                     // the last tile's readers are done with the S image: reuse it as scratch
        float* red = (float*)s_lds;
        red[t] = bacc;
        __syncthreads();
        if (bias_s && t < 64) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) v += red[q * 64 + t];
            bias_ws[((size_t)(by / cl_blocks) * n_split + bx) * 64 + t] = v;
        }
        if (bias_l && t < 32) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) v += red[q * 32 + t];
            const int half = (ND == 3) ? kd - 1 : 0, nhalf = (ND == 3) ? 2 : 1;
            bias_ws[(((size_t)(by % cl_blocks) * nhalf + half) * n_split + bx) * 32 + t] = v;
        }
    }
    const int col = lane & 31, hq = lane >> 5;
    if (float* __restrict__ dW = tb.e[ti].dW) {
        // one slab per group: it IS the sum, so it goes straight to dW[cs][cl][kd][kh][0..3] and the layer has no dW blocks in the reduce pass.  + 0.f: the
        // reduce pass starts its sum from +0, so a -0 partial comes out as +0 there; every other bit is the same.
        // A lane holds the four kw of ONE kh: stored as they lie, a wave would write 64 16-byte pieces 256 bytes apart (measured: the launch 1 - 4 us longer, profiles/wgrad_roundtrips.md).  The
        // images are free after the last tile, so the four kh waves meet in LDS, 4 accumulator rows at a time, and four adjacent lanes store the 64
        // contiguous bytes of a (cs, cl, kd); the kh slot is xor-ed with cl & 3 against bank conflicts of the 64-byte-strided writes.
        const int taps = (ND == 3) ? 64 : 16;
        float4* xch = (float4*)smem;                         // [4 e][2 sg x 2 hq rows][32 cl][4 kh]: 32 KB
#pragma unroll
        for (int e0 = 0; e0 < 16; e0 += 4) {
            __syncthreads();                                 // the last tile's / the previous pass's readers are done
#pragma unroll
            for (int k = 0; k < 4; ++k)
                xch[((k * 4 + sg * 2 + hq) * 32 + col) * 4 + (kh ^ (col & 3))] = make_float4(acc[0][e0 + k] + 0.f, acc[1][e0 + k] + 0.f, acc[2][e0 + k] + 0.f, acc[3][e0 + k] + 0.f);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = t + k * NT, khj = j & 3, clj = (j >> 2) & 31, r4 = (j >> 7) & 3, e = e0 + k;
                const int row = (r4 >> 1) * 32 + (e & 3) + 8 * (e >> 2) + 4 * (r4 & 1);
                *(float4*)(dW + ((size_t)(cs0 + row) * g.Cl + cl0 + clj) * taps + kd * 16 + khj * 4) = xch[(j & ~3) | (khj ^ (clj & 3))];
            }
        }
    } else {
        float* slab = ws + ((size_t)(bz * grid_y + by) * n_split + bx) * 32768;
        // slab layout [kh][64 cs][32 cl][kw]: the lane owns the four kw values of (cs row, cl col), so they leave as ONE 16-byte store (32 lanes = 512 contiguous
        // bytes) and wgrad_reduce_kernel reads them back as one 16-byte load per slab — a quarter of the memory instructions of the [kh][kw][cs][cl] form on both sides
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = sg * 32 + (e & 3) + 8 * (e >> 2) + 4 * hq;
            *(float4*)(slab + ((kh * 64 + row) * 32 + col) * 4) = make_float4(acc[0][e], acc[1][e], acc[2][e], acc[3][e]);
        }
    }
    STAMP_END();
}

// dW[cs][cl][kd][kh][0..3] = sum over the n_split slabs of group (kd, channel block).  One thread per (kd, kh, cs, cl)
// sums the 4 kw values (a 16-byte store into the reference layout); 4 thread groups split the slab range, LDS combines.
// Blocks past the dW range sum the bias partials: block j handles 64 channels, 4 thread groups split the partial rows.
// A layer with one slab per group has no dW blocks (dw_blocks == 0: conv_wgrad_kernel stored its dW), only its bias blocks.
struct WgradReduceEntry {
    const float* ws; float* dW; const float* bias_ws; float* dbias;
    int Cs, Cl, n_split, cb, dw_blocks, bias_n, bias_rows, bias_width;
};
struct WgradReduceTable { WgradReduceEntry e[WG_MULTI_MAX]; int blk_start[WG_MULTI_MAX + 1]; int count, taps; };
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WgradReduceTable tb) {
    int ti = 0;
    while (ti + 1 < tb.count && (int)blockIdx.x >= tb.blk_start[ti + 1]) ++ti;
    const float* __restrict__ ws = tb.e[ti].ws;
    float* __restrict__ dW = tb.e[ti].dW;
    const float* __restrict__ bias_ws = tb.e[ti].bias_ws;
    float* __restrict__ dbias = tb.e[ti].dbias;
    const int Cl = tb.e[ti].Cl, taps = tb.taps, n_split = tb.e[ti].n_split, cb = tb.e[ti].cb, dw_blocks = tb.e[ti].dw_blocks;
    const int bias_n = tb.e[ti].bias_n, bias_rows = tb.e[ti].bias_rows, bias_width = tb.e[ti].bias_width;
    const int lbx = (int)blockIdx.x - tb.blk_start[ti];
    __shared__ float4 part[4][64];
    if (lbx >= dw_blocks) {
        // bias_ws is [channel group][bias_rows][bias_width]; channel = group * bias_width + lane
        __shared__ float bred[4][64];
        const int ch = (lbx - dw_blocks) * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
        float v = 0.f;
        if (ch < bias_n) {
            const float* base = bias_ws + (size_t)(ch / bias_width) * bias_rows * bias_width + (ch % bias_width);
            for (int r = q; r < bias_rows; r += 4) v += base[(size_t)r * bias_width];
        }
        bred[q][threadIdx.x & 63] = v;
        __syncthreads();
        if (q == 0 && ch < bias_n) dbias[ch] = bred[0][threadIdx.x] + bred[1][threadIdx.x] + bred[2][threadIdx.x] + bred[3][threadIdx.x];
        return;
    }
    const int cl_blocks = Cl / 32;
    // lbx enumerates (group = kd * cb + block, kh, cs row pair) ; 64 threads = 2 cs rows x 32 cl
    int bi = lbx;
    const int rowpair = bi % 32; bi /= 32;
    const int kh = bi % 4; bi /= 4;
    const int grp = bi;                                      // kd * cb + channel block
    const int kd = grp / cb, blk = grp % cb;
    const int lane64 = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int row = rowpair * 2 + (lane64 >> 5), col = lane64 & 31;
    const float* base = ws + (size_t)grp * n_split * 32768 + ((kh * 64 + row) * 32 + col) * 4;      // slab layout [kh][cs][cl][kw]
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    // U slabs' loads are issued before the first add (clamped slab index, predicated add: the order of the sum is unchanged).  The plain loop compiled to
    // load / wait / add per slab: one dependent round trip per slab, 16-64 of them per thread.
    constexpr int U = 8;
    for (int x0 = q; x0 < n_split; x0 += 4 * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = *(const float4*)(base + (size_t)min(x0 + 4 * u, n_split - 1) * 32768);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (x0 + 4 * u < n_split) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
    }
    part[q][lane64] = a;
    __syncthreads();
    if (q == 0) {
        const float4 b = part[1][lane64], c = part[2][lane64], d = part[3][lane64];
        a.x += b.x + c.x + d.x; a.y += b.y + c.y + d.y; a.z += b.z + c.z + d.z; a.w += b.w + c.w + d.w;
        const int cs = (blk / cl_blocks) * 64 + row, cl = (blk % cl_blocks) * 32 + col;
        *(float4*)(dW + ((size_t)cs * Cl + cl) * taps + kd * 16 + kh * 4) = a;
    }
}

#define WGRAD_MAX_WG 512
template <typename T, int ND> constexpr size_t wgrad_lds_bytes() {
    using TL = Tile<ND, 128>;
    return (size_t)128 * 64 * sizeof(T) + (size_t)TL::TD * (2 * TL::TH + 2) * (2 * TL::TW + 2 + (ND == 2 ? 2 : 0)) * 32 * sizeof(T);
}
// Launch geometry of one layer's weight gradient: fills the two table entries, returns the workgroup counts of the main and the reduce pass.
template <typename T, int ND>
int plan_wgrad(const void* S, const void* L, float* ws, float* dW, float* dbias, int bias_mode, ConvGeom g, WgradEntry* me, WgradReduceEntry* re, int* main_blocks,
               int* reduce_blocks, long long n_split_req = 0) {
    using TL = Tile<ND, 128>;
    g.tiles_d = (g.sd + TL::TD - 1) / TL::TD; g.tiles_h = (g.sh + TL::TH - 1) / TL::TH; g.tiles_w = (g.sw + TL::TW - 1) / TL::TW;
    // 2D layers at most half a tile wide (7 x 7, 4 x 4 maps): two samples per tile — a property of the layer's shape alone, like the slab count below
    const int xb = (ND == 2 && g.sw <= TL::TW / 2 && g.B >= 2) ? 1 : 0;
    const long long total_tiles = (long long)(xb ? (g.B + 1) / 2 : g.B) * g.tiles_d * g.tiles_h * g.tiles_w;
    const int cb = (g.Cs / 64) * (g.Cl / 32), tg = (ND == 3) ? 4 : 1;
    // each workgroup ends with a 128 KB slab: ~2 workgroups per CU at most, and >= 4 tiles of work per slab
    long long n_split = WGRAD_MAX_WG / ((long long)cb * tg);   // in-step scan of 256 / 512 / 768 / 1024: 234 / 231 / 248 / 253 us for the six launches + reductions
    // >= 4 tiles per slab, except that a small layer may go down to one tile per slab until it has one workgroup per CU (in-step scan:
    // dec1 29 -> 22 us, dec2 26 -> 20 us incl. their reductions; more slabs than that only lengthen the reduction)
    long long floor_split = 256 / ((long long)cb * tg);
    if (floor_split > total_tiles) floor_split = total_tiles;
    long long by_tiles = total_tiles / 4;
    if (by_tiles < floor_split) by_tiles = floor_split;
    if (n_split > by_tiles) n_split = by_tiles;
    {   // ~WG_TILES tiles of 128 positions per slab, at least WG_MIN_WG workgroups: a function of THIS layer only, the same whether the layer
        // is launched alone (cvae_conv_wgrad) or as one entry of a grouped launch (cvae_conv_wgrad_multi) — the summation order, and with it every bit
        // of the gradient, does not depend on how the caller batches its launches
        long long req = (total_tiles + WG_TILES - 1) / WG_TILES;
        const long long groups = (long long)cb * tg;
        if (req * groups < WG_MIN_WG) req = (WG_MIN_WG + groups - 1) / groups;
        if (req < n_split) n_split = req;
    }
    if (n_split_req > 0 && n_split_req < n_split) n_split = n_split_req;
    if (n_split < 1) n_split = 1;
    if (n_split > total_tiles) n_split = total_tiles;
    if ((long long)cb * tg * n_split > (1 << 24)) return CVAE_E_BADSHAPE;
    // bias partials live behind the slabs: [channel group][rows][width] with (mode 1) 64-wide groups of cs, n_split rows;
    // (mode 2) 32-wide groups of cl, (2 plane parities in 3D) * n_split rows
    const long long wgs = (long long)cb * tg * n_split;
    float* bias_ws = ws + (size_t)(wgs > WGRAD_MAX_WG ? wgs : WGRAD_MAX_WG) * 32768;
    if (!dbias) bias_mode = 0;
    // one slab per group: the main kernel writes dW itself and the reduce pass keeps only the layer's bias blocks (a function of the shape alone, like n_split)
    const bool direct = n_split == 1;
    *me = WgradEntry{S, L, ws, bias_ws, g, (int)n_split, cb, tg, bias_mode, xb, direct ? dW : nullptr};
    *main_blocks = (int)wgs;
    const int dw_blocks = direct ? 0 : cb * tg * 4 * 32;
    const int bias_n = bias_mode == 1 ? g.Cs : (bias_mode == 2 ? g.Cl : 0), bias_width = bias_mode == 1 ? 64 : 32;
    const int bias_rows = (int)n_split * ((bias_mode == 2 && ND == 3) ? 2 : 1);
    *re = WgradReduceEntry{ws, dW, bias_ws, dbias, g.Cs, g.Cl, (int)n_split, cb, dw_blocks, bias_n, bias_rows, bias_width};
    *reduce_blocks = dw_blocks + (bias_n + 63) / 64;
    return CVAE_OK;
}
template <typename T, int ND>
int launch_wgrad_tables(WgradTable& mt, WgradReduceTable& rt, hipStream_t stream) {
    constexpr size_t LDS = wgrad_lds_bytes<T, ND>();
    static_assert(LDS <= CVAE_LDS_MAX, "LDS tile exceeds the 160 KiB of a CDNA4 CU");
    constexpr auto kern = conv_wgrad_kernel<T, ND>;
    if (cvae_allow_lds<kern>(LDS) != CVAE_OK) return CVAE_E_LAUNCH;
    rt.taps = (ND == 3) ? 64 : 16;
    hipLaunchKernelGGL(kern, dim3((unsigned)mt.blk_start[mt.count]), dim3(512), LDS, stream, mt);
    CVAE_CHECK_LAUNCH();
    if (rt.blk_start[rt.count] == 0) return CVAE_OK;         // every layer stored its dW directly and none has a bias sum
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)rt.blk_start[rt.count]), dim3(256), 0, stream, rt);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
template <typename T, int ND>
int launch_wgrad(const void* S, const void* L, float* ws, float* dW, float* dbias, int bias_mode, ConvGeom g, hipStream_t stream) {
    WgradTable mt;
    WgradReduceTable rt;
    int mb, rb;
    const int rc = plan_wgrad<T, ND>(S, L, ws, dW, dbias, bias_mode, g, &mt.e[0], &rt.e[0], &mb, &rb);
    if (rc != CVAE_OK) return rc;
    mt.count = rt.count = 1;
    mt.blk_start[0] = rt.blk_start[0] = 0;
    mt.blk_start[1] = mb; rt.blk_start[1] = rb;
    return launch_wgrad_tables<T, ND>(mt, rt, stream);
}

bool geom_ok(int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd) {
    if (nd != 2 && nd != 3) return false;
    if (B < 0 || sd <= 0 || sh <= 0 || sw <= 0 || Cs <= 0 || ld <= 0 || lh <= 0 || lw <= 0 || Cl <= 0) return false;
    if (B > 65535 || sd > 32767 || sh > 32767 || sw > 32767 || ld > 65535 || lh > 65535 || lw > 65535) return false;
    if (nd == 2 && (sd != 1 || ld != 1)) return false;
    if (sd * sh * sw * Cs >= (int64_t(1) << 31) || ld * lh * lw * Cl >= (int64_t(1) << 31)) return false;   // 32-bit offsets inside a sample
    auto pair_ok = [](int64_t s, int64_t l) { return s == l / 2; };        // floor((l + 2 - 4) / 2) + 1 == l / 2
    if (nd == 3 && !pair_ok(sd, ld)) return false;
    return pair_ok(sh, lh) && pair_ok(sw, lw) && lh >= 2 && lw >= 2 && (nd == 2 || ld >= 2);
}

}  // namespace

// C1 kernels live in conv_c1.hip
int cvae_conv_down_c1(const void* L, int l_dtype, const float* w, const float* bias, const void* mask, void* S, int64_t B, int64_t sd, int64_t sh, int64_t sw,
                      int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, int act, hipStream_t stream, F8Side f8 = F8Side{nullptr, nullptr, nullptr});
int cvae_conv_up_c1(const void* S, const float* w, const float* bias, const void* mask, void* L, int64_t B, int64_t sd, int64_t sh, int64_t sw,
                    int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, int act, hipStream_t stream, long long walk_units = 0);
int cvae_conv_up_c1_fp8in_impl(const void* S8, const float* w, const float* bias, void* L, float in_scale, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int act,
                               hipStream_t stream);
size_t cvae_conv_wgrad_c1_workspace_bytes(int64_t Cs, int nd);
int cvae_conv_wgrad_c1(const void* S, const void* L, int l_dtype, float* dW, float* dbias, float* dbias_l, void* workspace, size_t workspace_bytes, int64_t B, int64_t sd, int64_t sh,
                       int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, hipStream_t stream);

#ifdef CVAE_STAMP
extern "C" int cvae_debug_stamps(unsigned long long* host, size_t count) {
    if (count > (size_t)CVAE_STAMP_WGS * CVAE_STAMP_SLOTS) return CVAE_E_BADSHAPE;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamp), count * sizeof(unsigned long long)) == hipSuccess ? CVAE_OK : CVAE_E_LAUNCH;
}
#endif

extern "C" int cvae_conv_pack_weight(const float* w, void* packed, int64_t Cs, int64_t Cl, int nd, int for_up, int dtype, void* stream) {
    if ((nd != 2 && nd != 3) || Cs <= 0 || Cl <= 0) return CVAE_E_BADSHAPE;
    if ((!for_up && Cl % 16) || (for_up && (Cs % 16 || Cl % 32))) return CVAE_E_UNSUPPORTED;      // what cvae_conv_up accepts
    if (!w || !packed) return CVAE_E_NULLPTR;
    const int taps = (nd == 3) ? 64 : 16;
    const int64_t n = Cs * Cl * taps;
    return with_dtype(dtype, [&](auto tv) {
        using T = decltype(tv);
        hipLaunchKernelGGL(pack_weight_kernel<T>, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, w, (T*)packed, (int)Cs, (int)Cl, taps, for_up);
        return launch_rc();
    });
}

// channel counts an fp8 product accepts (cvae_conv_fp8): conv C_in % 32, C_out % 64; ConvTranspose C_in % 32, C_out % 32, C_out > 1
static bool fp8_pack_ok(int64_t Cs, int64_t Cl, int for_up) { return for_up ? (Cs % 32 == 0 && Cl % 32 == 0 && Cl > 1) : (Cl % 32 == 0 && Cs % 64 == 0); }
extern "C" int cvae_conv_pack_weight_pairs(const float* const* w, void* const* packed_down, void* const* packed_up, const int64_t* Cs, const int64_t* Cl,
                                           const int* f8dir, void* const* f8out, const float* const* inv_scale_dev, void* const* amax_slots,
                                           int count, int nd, int dtype, void* stream) {
    if ((nd != 2 && nd != 3) || count < 0) return CVAE_E_BADSHAPE;
    if (count == 0) return CVAE_OK;
    if (!w || !packed_down || !packed_up || !Cs || !Cl) return CVAE_E_NULLPTR;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    const int tsplit = (nd == 3) ? 4 : 1;                    // blocks per (cs, cl) tile: 16 taps each
    for (int c0 = 0; c0 < count; c0 += PAIR_MAX) {
        PairTable tb;
        const int cnt = (count - c0 < PAIR_MAX) ? count - c0 : PAIR_MAX;
        long long blocks = 0;
        for (int i = 0; i < cnt; ++i) {
            const int64_t cs = Cs[c0 + i], cl = Cl[c0 + i];
            if (cs <= 0 || cl <= 0) return CVAE_E_BADSHAPE;
            if (cs % 16 || cl % 16) return CVAE_E_UNSUPPORTED;
            const int fd = f8dir ? f8dir[c0 + i] : 0;
            if (fd < 0 || fd > 2) return CVAE_E_BADSHAPE;
            if (fd) {
                if (dtype != CVAE_BF16) return CVAE_E_DTYPE;
                if (!fp8_pack_ok(cs, cl, fd == 2)) return CVAE_E_UNSUPPORTED;
                if (!f8out || !f8out[c0 + i] || !inv_scale_dev || !inv_scale_dev[c0 + i]) return CVAE_E_NULLPTR;
            }
            if (!w[c0 + i] || (fd != 1 && !packed_down[c0 + i]) || (fd != 2 && !packed_up[c0 + i])) return CVAE_E_NULLPTR;
            tb.w[i] = w[c0 + i]; tb.down[i] = packed_down[c0 + i]; tb.up[i] = packed_up[c0 + i]; tb.Cs[i] = (int)cs; tb.Cl[i] = (int)cl;
            tb.f8dir[i] = fd; tb.f8out[i] = fd ? (fp8*)f8out[c0 + i] : nullptr; tb.inv_scale[i] = fd ? inv_scale_dev[c0 + i] : nullptr;
            tb.amax[i] = (fd && amax_slots) ? (unsigned*)amax_slots[c0 + i] : nullptr;
            tb.blk_start[i] = (int)blocks;
            blocks += (cs / 16) * (cl / 16) * tsplit;
            if (blocks > (1 << 30)) return CVAE_E_BADSHAPE;
        }
        tb.blk_start[cnt] = (int)blocks;
        tb.count = cnt;
        const dim3 grid((unsigned)blocks);
        hipStream_t st = (hipStream_t)stream;
        const int rc = with_dtype(dtype, [&](auto tv) { return with_nd(nd, [&](auto n) {
            constexpr int TAPS = decltype(n)::value == 3 ? 64 : 16;
            hipLaunchKernelGGL((pack_weight_pairs_kernel<decltype(tv), TAPS>), grid, dim3(256), 0, st, tb);
            return launch_rc();
        }); });
        if (rc != CVAE_OK) return rc;
    }
    return CVAE_OK;
}

#define GEOM_INIT() ConvGeom g{(int)B, (int)sd, (int)sh, (int)sw, (int)Cs, (int)ld, (int)lh, (int)lw, (int)Cl, 0, 0, 0}

extern "C" size_t cvae_conv_data_workspace_bytes(int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                                                  int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int for_up) {
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd) || B == 0 || Cl == 1) return 0;
    GEOM_INIT();
    const bool wide = !for_up || Cl % 64 == 0;
    if (for_up ? (Cs % 16 || Cl % 32) : (Cl % 16 || Cs % 64)) return 0;
    return with_nd(nd, [&](auto n) { return with_bool(for_up != 0, [&](auto up) { return with_bool(wide, [&](auto wd) {
        return data_workspace_bytes<decltype(n)::value, decltype(up)::value, decltype(wd)::value>(g);
    }); }); });
}

// ReLU masks as BITS (F8Side, common.h): mask_bits replaces `mask` (1 bit per element of the result instead of the saved activation: 1/16 of the
// bytes the backward launch reads for it), relu_bits_out receives the mask of THIS launch's result for the backward pass to come.
static bool bits_ok(int64_t Cout) { return Cout % 32 == 0; }
extern "C" int cvae_conv_down(const void* L, const void* w, const float* bias, const void* mask, const void* mask_bits, void* S, void* relu_bits_out,
                              int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                              int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int dtype, int act,
                              void* workspace, size_t workspace_bytes, int xpair, void* stream) {
    if (xpair < -1 || xpair > 1 || (mask && mask_bits)) return CVAE_E_BADSHAPE;
    if ((mask_bits || relu_bits_out) && !bits_ok(Cs)) return CVAE_E_UNSUPPORTED;
    if (Cl == 1 && mask_bits && !(dtype == CVAE_BF16)) return CVAE_E_UNSUPPORTED;
    F8Side side{nullptr, nullptr, nullptr};
    side.mask_bits = (const unsigned*)mask_bits; side.bits_out = (unsigned*)relu_bits_out;
    UpVariant var;
    var.xpair = xpair;
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (B == 0) return CVAE_OK;
    if (!L || !w || !S) return CVAE_E_NULLPTR;
    hipStream_t st = (hipStream_t)stream;
    if (Cl == 1) return cvae_conv_down_c1(L, dtype, (const float*)w, bias, mask, S, B, sd, sh, sw, Cs, ld, lh, lw, nd, dtype, act, st, side);
    if (Cl % 16 || Cs % 64) return CVAE_E_UNSUPPORTED;
    GEOM_INIT();
    const ConvArgs a{L, w, bias, mask, S, g, act, workspace, workspace_bytes, st, 1.f, 1.f, side, var};
    return with_dtype(dtype, [&](auto t) { return with_nd(nd, [&](auto n) { return dispatch_conv<decltype(t), decltype(n)::value, false, true>(a); }); });
}
// ---- the single-channel image end of the network, image read in the dtype it is stored in (no cast pass in front of the first conv) ----
extern "C" int cvae_conv_image_supported(const void* L, int64_t lw, int l_dtype, int dtype) {
    if (l_dtype == dtype) return 1;
    if (!(dtype == CVAE_BF16 && l_dtype == CVAE_F32)) return 0;
    return lw % 4 == 0 && lw >= 4 && (((uintptr_t)L) & 15) == 0;
}
extern "C" int cvae_conv_down_image(const void* L, int l_dtype, const float* w, const float* bias, const void* mask, void* S,
                                    int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, int act, void* stream) {
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, 1, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype) || !dtype_ok(l_dtype)) return CVAE_E_DTYPE;
    if (B == 0) return CVAE_OK;
    if (!L || !w || !S) return CVAE_E_NULLPTR;
    if (!cvae_conv_image_supported(L, lw, l_dtype, dtype)) return CVAE_E_UNSUPPORTED;
    return cvae_conv_down_c1(L, l_dtype, w, bias, mask, S, B, sd, sh, sw, Cs, ld, lh, lw, nd, dtype, act, (hipStream_t)stream);
}
extern "C" int cvae_conv_down_image_f8(const void* L, int l_dtype, const float* w, const float* bias, void* S, void* S8, const float* inv_scale_dev, void* amax_slots,
                                       void* relu_bits_out, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int act,
                                       void* stream) {
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, 1, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(l_dtype)) return CVAE_E_DTYPE;
    if (B == 0) return CVAE_OK;
    if (!L || !w || !S || (S8 && !inv_scale_dev)) return CVAE_E_NULLPTR;
    if (!cvae_conv_image_supported(L, lw, l_dtype, CVAE_BF16) && l_dtype != CVAE_BF16) return CVAE_E_UNSUPPORTED;
    F8Side side{inv_scale_dev, (fp8*)S8, (unsigned*)amax_slots};
    side.bits_out = (unsigned*)relu_bits_out;
    return cvae_conv_down_c1(L, l_dtype, w, bias, nullptr, S, B, sd, sh, sw, Cs, ld, lh, lw, nd, CVAE_BF16, act, (hipStream_t)stream, side);
}
extern "C" int cvae_conv_wgrad_image(const void* S, const void* L, int l_dtype, float* dW, float* dbias, void* workspace, size_t workspace_bytes,
                                     int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, void* stream) {
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, 1, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype) || !dtype_ok(l_dtype)) return CVAE_E_DTYPE;
    if (!dW) return CVAE_E_NULLPTR;
    const int taps = (nd == 3) ? 64 : 16;
    if (B == 0) {
        if (dbias && hipMemsetAsync(dbias, 0, (size_t)Cs * sizeof(float), (hipStream_t)stream) != hipSuccess) return CVAE_E_LAUNCH;
        return hipMemsetAsync(dW, 0, (size_t)Cs * taps * sizeof(float), (hipStream_t)stream) == hipSuccess ? CVAE_OK : CVAE_E_LAUNCH;
    }
    if (!S || !L) return CVAE_E_NULLPTR;
    return cvae_conv_wgrad_c1(S, L, l_dtype, dW, dbias, nullptr, workspace, workspace_bytes, B, sd, sh, sw, Cs, ld, lh, lw, nd, dtype, (hipStream_t)stream);
}

extern "C" int cvae_conv_up(const void* S, const void* w, const float* bias, const void* mask, const void* mask_bits, void* L, void* relu_bits_out,
                            int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                            int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int dtype, int act,
                            void* workspace, size_t workspace_bytes, int upfull, int xpair, int64_t c1_walk_units, void* stream) {
    if (upfull < -1 || upfull > 1 || xpair < -1 || xpair > 1 || c1_walk_units < 0 || c1_walk_units >= ((int64_t)1 << 30) || (mask && mask_bits)) return CVAE_E_BADSHAPE;
    if ((mask_bits || relu_bits_out) && (!bits_ok(Cl) || Cl == 1)) return CVAE_E_UNSUPPORTED;
    F8Side side{nullptr, nullptr, nullptr};
    side.mask_bits = (const unsigned*)mask_bits; side.bits_out = (unsigned*)relu_bits_out;
    UpVariant var;
    var.upfull = upfull; var.xpair = xpair; var.walk_units = c1_walk_units;
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (B == 0) return CVAE_OK;
    if (!S || !w || !L) return CVAE_E_NULLPTR;
    hipStream_t st = (hipStream_t)stream;
    if (Cl == 1) return cvae_conv_up_c1(S, (const float*)w, bias, mask, L, B, sd, sh, sw, Cs, ld, lh, lw, nd, dtype, act, st, var.walk_units);
    if (Cs % 16 || Cl % 32) return CVAE_E_UNSUPPORTED;
    GEOM_INIT();
    const bool wide = (Cl % 64) == 0;     // 64-channel output tiles, else 32 (DataForm)
    const ConvArgs a{S, w, bias, mask, L, g, act, workspace, workspace_bytes, st, 1.f, 1.f, side, var};
    return with_dtype(dtype, [&](auto t) { return with_nd(nd, [&](auto n) {
        using T = decltype(t);
        constexpr int ND = decltype(n)::value;
        // the whole-K kernel: bf16, 32-channel tiles, and the tensor form of the mask only (inference sweeps: no mask at all)
        if constexpr (std::is_same<T, bf16>::value) if (!wide && !side.mask_bits && !side.bits_out) {
            const int rc = try_up_full<T, ND>(a);
            if (rc != CVAE_E_UNSUPPORTED) return rc;
        }
        return with_bool(wide, [&](auto wd) { return dispatch_conv<T, ND, true, decltype(wd)::value>(a); });
    }); });
}

// dx = scatter(g, w) * act'(gate): cvae_conv_up's product, forms and dispatch.  act' is 1 (NONE: no gate read) or a 0 / 1 mask (RELU) through cvae_conv_up
// itself — the same launches, the same bits — and a LeakyReLU slope through the gated instances of the three kernels.
extern "C" int cvae_conv_down_bwd_data(const void* grad, const void* w, const void* gate, void* dx, int64_t B, int64_t sh, int64_t sw, int64_t Cs, int64_t lh, int64_t lw,
                                       int64_t Cl, int nd, int dtype, int gate_act, void* workspace, size_t workspace_bytes, int upfull, int xpair, void* stream) {
    if (gate_act != CVAE_ACT_NONE && gate_act != CVAE_ACT_RELU && gate_act != CVAE_ACT_LEAKY001 && gate_act != CVAE_ACT_LEAKY02) return CVAE_E_UNSUPPORTED;
    if (nd != 2 || Cs <= 0 || Cl <= 0 || Cs % 16 || Cl % 32) return CVAE_E_UNSUPPORTED;
    if (gate_act != CVAE_ACT_NONE && !gate && B > 0) return CVAE_E_NULLPTR;
    if (gate_act == CVAE_ACT_NONE || gate_act == CVAE_ACT_RELU)
        return cvae_conv_up(grad, w, nullptr, gate_act == CVAE_ACT_RELU ? gate : nullptr, nullptr, dx, nullptr, B, 1, sh, sw, Cs, 1, lh, lw, Cl, 2, dtype, CVAE_ACT_NONE,
                            workspace, workspace_bytes, upfull, xpair, 0, stream);
    if (upfull < -1 || upfull > 1 || xpair < -1 || xpair > 1) return CVAE_E_BADSHAPE;
    const int64_t sd = 1, ld = 1;
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (B == 0) return CVAE_OK;
    if (!grad || !w || !dx) return CVAE_E_NULLPTR;
    UpVariant var;
    var.upfull = upfull; var.xpair = xpair;
    GEOM_INIT();
    const bool wide = (Cl % 64) == 0;
    ConvArgs a{grad, w, nullptr, gate, dx, g, CVAE_ACT_NONE, workspace, workspace_bytes, (hipStream_t)stream, 1.f, 1.f, F8Side{nullptr, nullptr, nullptr}, var};
    a.gate_slope = gate_act == CVAE_ACT_LEAKY02 ? 0.2f : 0.01f;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (std::is_same<T, bf16>::value) if (!wide) {            // the whole-K kernel, as in cvae_conv_up
            const int rc = try_up_full<T, 2, true>(a);
            if (rc != CVAE_E_UNSUPPORTED) return rc;
        }
        return with_bool(wide, [&](auto wd) { return dispatch_conv_gated<T, 2, decltype(wd)::value>(a); });
    });
}

extern "C" size_t cvae_conv_wgrad_workspace_bytes(int64_t Cs, int64_t Cl, int nd) {
    if (Cl == 1) return cvae_conv_wgrad_c1_workspace_bytes(Cs, nd);
    const int64_t groups = (Cs / 64) * (Cl / 32) * ((nd == 3) ? 4 : 1);             // slab groups (kd, channel block)
    const int64_t wgs = groups > WGRAD_MAX_WG ? groups : WGRAD_MAX_WG;             // groups * n_split <= max(WGRAD_MAX_WG, groups)
    const int64_t bias_floats = 2 * wgs * 64;                                      // bias partials: < 2 rows of 64 floats per workgroup
    return (size_t)(wgs * 32768 + bias_floats) * sizeof(float);
}

extern "C" int cvae_conv_wgrad(const void* S, const void* L, float* dW, float* dbias, int dbias_side, void* workspace, size_t workspace_bytes,
                               int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                               int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int dtype, void* stream) {
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd)) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (!dW) return CVAE_E_NULLPTR;
    if (dbias_side != 0 && dbias_side != 1) return CVAE_E_BADSHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int taps = (nd == 3) ? 64 : 16;
    if (B == 0) {
        if (dbias && hipMemsetAsync(dbias, 0, (size_t)(dbias_side ? Cl : Cs) * sizeof(float), st) != hipSuccess) return CVAE_E_LAUNCH;
        return hipMemsetAsync(dW, 0, (size_t)Cs * Cl * taps * sizeof(float), st) == hipSuccess ? CVAE_OK : CVAE_E_LAUNCH;
    }
    if (!S || !L) return CVAE_E_NULLPTR;
    if (Cl == 1) {
        float* dbias_l = nullptr;
        if (dbias && dbias_side == 1) {                      // ConvTranspose to one channel: its bias gradient is the plain sum of L
            if (lh == 2 * sh && lw == 2 * sw && (nd != 3 || ld == 2 * sd)) dbias_l = dbias;     // fused: the kernel reads all of L anyway
            else {
                const int rcb = cvae_channel_sum(L, dbias, B * ld * lh * lw, 1, dtype, workspace, workspace_bytes, stream);   // scratch shared in stream order
                if (rcb != CVAE_OK) return rcb;
            }
            dbias = nullptr;
        }
        return cvae_conv_wgrad_c1(S, L, dtype, dW, dbias, dbias_l, workspace, workspace_bytes, B, sd, sh, sw, Cs, ld, lh, lw, nd, dtype, st);   // S-side bias sum fused (S^T . ones)
    }
    if (Cs % 64 || Cl % 32) return CVAE_E_UNSUPPORTED;
    int bias_mode = dbias ? (dbias_side ? 2 : 1) : 0;
    if (bias_mode == 2 && (lh != 2 * sh || lw != 2 * sw || (nd == 3 && ld != 2 * sd))) {
        // an odd L extent leaves a plane / row outside every tile's non-halo part: sum L separately
        const int rcb = cvae_channel_sum(L, dbias, B * ld * lh * lw, Cl, dtype, workspace, workspace_bytes, stream);   // scratch shared in stream order
        if (rcb != CVAE_OK) return rcb;
        bias_mode = 0;
    }
    const size_t need = cvae_conv_wgrad_workspace_bytes(Cs, Cl, nd);
    if (!workspace) return CVAE_E_NULLPTR;
    if (workspace_bytes < need) return CVAE_E_WORKSPACE;
    GEOM_INIT();
    float* db = bias_mode ? dbias : nullptr;
    return with_dtype(dtype, [&](auto tv) { return with_nd(nd, [&](auto n) {
        return launch_wgrad<decltype(tv), decltype(n)::value>(S, L, (float*)workspace, dW, db, bias_mode, g, st);
    }); });
}

template <typename T, int ND>
static int wgrad_multi_t(int count, const void* const* S, const void* const* L, float* const* dW, float* const* dbias, const int* dbias_side, void* const* workspace,
                         const int64_t* dims, hipStream_t st) {
    WgradTable mt;
    WgradReduceTable rt;
    int mb = 0, rb = 0;
    // Together the layers need ~2-3 workgroups per CU, not 2 each: every workgroup ends with a 128 KB slab, and 6 x 512 slabs (384 MB) no longer fit
    // the 256 MB Infinity Cache between the main pass and the reduction (measured: the grouped reduction 77 us against 64 us for six separate
    // ones).  The slab count of a layer depends on THAT layer only — ~WG_TILES tiles of 128 positions per slab, at least WG_MIN_WG
    // workgroups — never on what else rides in the launch: the split-backward capture flushes decoder and encoder separately, and its
    // gradients must have the summation order (the bits) of the single-launch step.
    using TLm = Tile<ND, 128>;
    // longest workgroups first (tiles per slab, descending): the launch is ~2.5 rounds of workgroups, and a long one started last is the tail
    long long req[WG_MULTI_MAX], key[WG_MULTI_MAX];
    int order[WG_MULTI_MAX];
    for (int i = 0; i < count; ++i) {
        const int64_t* d = dims + 9 * i;
        const long long tiles = d[0] * ((d[1] + TLm::TD - 1) / TLm::TD) * ((d[2] + TLm::TH - 1) / TLm::TH) * ((d[3] + TLm::TW - 1) / TLm::TW);
        const long long groups = (d[4] / 64) * (d[8] / 32) * ((ND == 3) ? 4 : 1);            // workgroups per slab index
        req[i] = (tiles + WG_TILES - 1) / WG_TILES;
        if (req[i] * groups < WG_MIN_WG) req[i] = (WG_MIN_WG + groups - 1) / groups;
        if (req[i] > tiles) req[i] = tiles;
        key[i] = (tiles + req[i] - 1) / req[i];
        int k = i;
        while (k > 0 && key[order[k - 1]] < key[i]) { order[k] = order[k - 1]; --k; }
        order[k] = i;
    }
    for (int k = 0; k < count; ++k) {
        const int i = order[k];
        const int64_t* d = dims + 9 * i;
        ConvGeom g{(int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], (int)d[6], (int)d[7], (int)d[8], 0, 0, 0};
        const int bias_mode = dbias[i] ? (dbias_side[i] ? 2 : 1) : 0;
        int m1, r1;
        const int rc = plan_wgrad<T, ND>(S[i], L[i], (float*)workspace[i], dW[i], dbias[i], bias_mode, g, &mt.e[k], &rt.e[k], &m1, &r1, req[i]);
        if (rc != CVAE_OK) return rc;
        mt.blk_start[k] = mb; rt.blk_start[k] = rb;
        mb += m1; rb += r1;
    }
    mt.blk_start[count] = mb; rt.blk_start[count] = rb;
    mt.count = rt.count = count;
    return launch_wgrad_tables<T, ND>(mt, rt, st);
}

extern "C" int cvae_conv_wgrad_multi(int count, const void* const* S, const void* const* L, float* const* dW, float* const* dbias, const int* dbias_side,
                                     void* const* workspace, const size_t* workspace_bytes, const int64_t* dims, int nd, int dtype, void* stream) {
    if (count < 0 || count > WG_MULTI_MAX || (nd != 2 && nd != 3)) return CVAE_E_BADSHAPE;
    if (count == 0) return CVAE_OK;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (!S || !L || !dW || !dbias || !dbias_side || !workspace || !workspace_bytes || !dims) return CVAE_E_NULLPTR;
    for (int i = 0; i < count; ++i) {
        const int64_t* d = dims + 9 * i;
        const int64_t B = d[0], sd = d[1], sh = d[2], sw = d[3], Cs = d[4], ld = d[5], lh = d[6], lw = d[7], Cl = d[8];
        if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd) || B == 0) return CVAE_E_BADSHAPE;
        if (Cl == 1 || Cs % 64 || Cl % 32) return CVAE_E_UNSUPPORTED;                       // the single-channel layers have their own kernels
        if (dbias_side[i] != 0 && dbias_side[i] != 1) return CVAE_E_BADSHAPE;
        if (dbias[i] && dbias_side[i] == 1 && (lh != 2 * sh || lw != 2 * sw || (nd == 3 && ld != 2 * sd))) return CVAE_E_UNSUPPORTED;   // odd L extent: cvae_conv_wgrad sums L separately
        if (!S[i] || !L[i] || !dW[i] || !workspace[i]) return CVAE_E_NULLPTR;
        if (workspace_bytes[i] < cvae_conv_wgrad_workspace_bytes(Cs, Cl, nd)) return CVAE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto tv) { return with_nd(nd, [&](auto n) {
        return wgrad_multi_t<decltype(tv), decltype(n)::value>(count, S, L, dW, dbias, dbias_side, workspace, dims, st);
    }); });
}

// ---------------------------------------------------------------------------------------------- fp8 (e4m3) products
// BASELINE.json configs[4].  Conv / ConvTranspose products with C_in >= 32 and C_out > 1 on fp8 operands with per-tensor scales and fp32
// accumulation, on the block-scaled CDNA4 MFMA v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (K = 64 per instruction, twice the
// bf16 FLOPs per clock).  conv_data_kernel<f8x2, ..>: the bf16 kernel's tiles, staging and epilogue on half the operand bytes (see Frag<f8x2>).
//   * inference (the counterfactual decode sweep): static scales from a calibration pass, fp8 codes travel between fp8 layers;
//   * training forward (the step of causal_cascade/train.py:19-39 with fp8 conv inputs): scales live on the device and follow the tensors with
//     one step of delay (cvae_fp8_scale_update), every producer leaves its result twice — bf16 for the backward pass, fp8 for the next layer —
//     and records its amax; the backward pass runs the bf16 kernels on the bf16 copies.
__global__ void quantize_fp8_kernel(const void* __restrict__ src, int src_dtype, fp8* __restrict__ dst, int64_t n, float inv_scale, const float* __restrict__ inv_scale_dev,
                                    unsigned* __restrict__ amax) {
    const float mul = inv_scale_dev ? inv_scale_dev[0] : inv_scale;
    float amx = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = src_dtype == CVAE_BF16 ? to_f32(((const bf16*)src)[i]) : ((const float*)src)[i];
        amx = fmaxf(amx, fabsf(v));
        dst[i] = from_f32<fp8>(v * mul);
    }
    __shared__ float red[4];
    if (amax) amax_publish_wg(amax, amx, blockIdx.x, red);
}
extern "C" int cvae_quantize_fp8(const void* src, int src_dtype, void* dst, int64_t n, float inv_scale, const float* inv_scale_dev, void* amax_slots, void* stream) {
    if (n < 0 || (!inv_scale_dev && !(inv_scale > 0.f))) return CVAE_E_BADSHAPE;
    if (!dtype_ok(src_dtype)) return CVAE_E_DTYPE;
    if (n == 0) return CVAE_OK;
    if (!src || !dst) return CVAE_E_NULLPTR;
    hipLaunchKernelGGL(quantize_fp8_kernel, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, src, src_dtype, (fp8*)dst, n, inv_scale, inv_scale_dev, (unsigned*)amax_slots);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
extern "C" int cvae_absmax(const void* src, int dtype, int64_t n, void* amax_slots, void* stream) {
    if (n < 0) return CVAE_E_BADSHAPE;
    if (!dtype_ok(dtype)) return CVAE_E_DTYPE;
    if (n == 0) return CVAE_OK;
    if (!src || !amax_slots) return CVAE_E_NULLPTR;
    hipLaunchKernelGGL(absmax_kernel, dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dtype, n, (unsigned*)amax_slots);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
extern "C" int cvae_conv_pack_weight_fp8(const float* w, void* packed, int64_t Cs, int64_t Cl, int nd, int for_up, float inv_scale, void* stream) {
    if ((nd != 2 && nd != 3) || Cs <= 0 || Cl <= 0 || !(inv_scale > 0.f)) return CVAE_E_BADSHAPE;
    if (!fp8_pack_ok(Cs, Cl, for_up)) return CVAE_E_UNSUPPORTED;      // what cvae_conv_fp8 accepts
    if (!w || !packed) return CVAE_E_NULLPTR;
    const int taps = (nd == 3) ? 64 : 16;
    const int64_t n = Cs * Cl * taps;
    hipLaunchKernelGGL((pack_weight_kernel<fp8, 32>), dim3(cvae_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, w, (fp8*)packed, (int)Cs, (int)Cl, taps, for_up, inv_scale);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
extern "C" int cvae_conv_pack_weights_fp8(const float* const* w, void* const* packed, const int64_t* Cs, const int64_t* Cl, const int* for_up,
                                           const float* const* inv_scale_dev, void* const* amax_slots, int count, int nd, void* stream) {
    if ((nd != 2 && nd != 3) || count < 0 || count > F8PACK_MAX) return CVAE_E_BADSHAPE;
    if (count == 0) return CVAE_OK;
    if (!w || !packed || !Cs || !Cl || !for_up || !inv_scale_dev) return CVAE_E_NULLPTR;
    F8PackTable tb;
    tb.taps = (nd == 3) ? 64 : 16;
    int blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (Cs[i] <= 0 || Cl[i] <= 0) return CVAE_E_BADSHAPE;
        if (!fp8_pack_ok(Cs[i], Cl[i], for_up[i])) return CVAE_E_UNSUPPORTED;
        if (!w[i] || !packed[i] || !inv_scale_dev[i]) return CVAE_E_NULLPTR;
        tb.w[i] = w[i]; tb.out[i] = (fp8*)packed[i]; tb.inv_scale[i] = inv_scale_dev[i]; tb.amax[i] = amax_slots ? (unsigned*)amax_slots[i] : nullptr;
        tb.Cs[i] = (int)Cs[i]; tb.Cl[i] = (int)Cl[i]; tb.for_up[i] = for_up[i];
        tb.blk_start[i] = blocks;
        int64_t nb = (Cs[i] * Cl[i] * tb.taps + 4095) / 4096;
        if (nb > 1024) nb = 1024;
        blocks += (int)nb;
    }
    tb.blk_start[count] = blocks;
    tb.count = count;
    hipLaunchKernelGGL(pack_weight_fp8_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tb);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}
extern "C" int cvae_fp8_scale_update(void* amax_slots, float* scale, float* inv_scale, int n, float headroom, const int* layer_in, const int* layer_w, const int* layer_out,
                                     int n_layers, float* dscale, void* ticket, void* stream) {
    if (n < 0 || n > 4096 || n_layers < 0 || n_layers > F8LAYER_MAX || !(headroom > 0.f)) return CVAE_E_BADSHAPE;
    if (n == 0) return CVAE_OK;
    if (!amax_slots || !scale || !inv_scale || !ticket || (n_layers && (!layer_in || !layer_w || !layer_out || !dscale))) return CVAE_E_NULLPTR;
    F8LayerIdx li;
    li.count = n_layers;
    for (int l = 0; l < n_layers; ++l) {
        if (layer_in[l] < 0 || layer_in[l] >= n || layer_w[l] < 0 || layer_w[l] >= n || layer_out[l] >= n) return CVAE_E_BADSHAPE;
        li.in[l] = layer_in[l]; li.w[l] = layer_w[l]; li.out[l] = layer_out[l];
    }
    hipLaunchKernelGGL(fp8_scale_update_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, (unsigned*)amax_slots, scale, inv_scale, n, headroom, li, dscale, (unsigned*)ticket);
    CVAE_CHECK_LAUNCH();
    return CVAE_OK;
}

// One fp8 product.  up = 0: S = conv(L) ("down"), up = 1: L = convT(S).  out_dtype CVAE_BF16 (bf16 result; `out8` may ask for a second copy as fp8
// codes) or CVAE_FP8 (codes only).  Scales: by value (acc_scale = s_in * s_w, out8_inv_scale = 1 / s_out8), or, when `dscale` is not null,
// read from the device pair {acc_scale, out8_inv_scale} at run time.
template <int ND, bool UP, typename TO>
static int conv_fp8_t(const void* in, const void* w, const float* bias, void* out, ConvGeom g, int act, float acc_scale, float out_scale, F8Side f8, void* ws, size_t wsb, hipStream_t st,
                      UpVariant var) {
    const ConvArgs a{in, w, bias, nullptr, out, g, act, ws, wsb, st, acc_scale, out_scale, f8, var};
    if ((UP ? g.Cl : g.Cs) % 64 == 0) return dispatch_conv<f8x2, ND, UP, true, TO>(a);
    if constexpr (UP) return dispatch_conv<f8x2, ND, UP, false, TO>(a);
    else return CVAE_E_UNSUPPORTED;
}
extern "C" int cvae_conv_fp8(int up, const void* in8, const void* w8, const float* bias, void* out, int out_dtype, void* out8, const float* dscale, float acc_scale,
                             float out8_inv_scale, void* amax_slots, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int64_t Cl,
                             int nd, int act, void* workspace, size_t workspace_bytes, int xpair, void* relu_bits_out, void* stream) {
    if (!geom_ok(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd) || (up != 0 && up != 1) || xpair < -1 || xpair > 1) return CVAE_E_BADSHAPE;
    if (out_dtype != CVAE_FP8 && out_dtype != CVAE_BF16) return CVAE_E_DTYPE;
    if (!dscale && (!(acc_scale > 0.f) || ((out_dtype == CVAE_FP8 || out8) && !(out8_inv_scale > 0.f)))) return CVAE_E_BADSHAPE;
    if (out_dtype == CVAE_FP8 && out8) return CVAE_E_BADSHAPE;        // codes-only output: there is no second copy to ask for
    if (B == 0) return CVAE_OK;
    if (!in8 || !w8 || !out) return CVAE_E_NULLPTR;
    if (!fp8_pack_ok(Cs, Cl, up)) return CVAE_E_UNSUPPORTED;
    if (up ? (lh != 2 * sh || lw != 2 * sw || (nd == 3 && ld != 2 * sd)) : false) return CVAE_E_UNSUPPORTED;   // forward products only: exact 2x extents
    GEOM_INIT();
    hipStream_t st = (hipStream_t)stream;
    F8Side f8{dscale, (fp8*)out8, (unsigned*)amax_slots};
    f8.bits_out = (unsigned*)relu_bits_out;
    UpVariant var;
    var.xpair = xpair;
    return with_nd(nd, [&](auto n) {
        constexpr int ND = decltype(n)::value;
        auto run = [&](auto to, void* ws, size_t wsb) {      // codes-only output: no split-K (its finish pass writes bf16), hence no workspace
            using TO = decltype(to);
            return up ? conv_fp8_t<ND, true, TO>(in8, w8, bias, out, g, act, acc_scale, out8_inv_scale, f8, ws, wsb, st, var)
                      : conv_fp8_t<ND, false, TO>(in8, w8, bias, out, g, act, acc_scale, out8_inv_scale, f8, ws, wsb, st, var);
        };
        return out_dtype == CVAE_FP8 ? run(fp8{}, nullptr, 0) : run(bf16{}, workspace, workspace_bytes);
    });
}

extern "C" int cvae_conv_up_c1_fp8in(const void* S8, const float* w, const float* bias, void* L, float in_scale, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int nd,
                                     int act, void* stream) {
    if (!S8 || !w || !L) return CVAE_E_NULLPTR;
    if (nd != 3 || B < 1 || sd < 1 || sh < 1 || sw < 1) return CVAE_E_UNSUPPORTED;
    if (act < CVAE_ACT_NONE || act > CVAE_ACT_LEAKY001) return CVAE_E_BADSHAPE;
    return cvae_conv_up_c1_fp8in_impl(S8, w, bias, L, in_scale, B, sd, sh, sw, Cs, act, (hipStream_t)stream);
}
