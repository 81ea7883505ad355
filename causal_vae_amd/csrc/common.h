// common.h — shared device helpers for libcvae_hip (gfx950 / CDNA4 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/cvae_hip.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CVAE_WAVE 64

// did the launch just issued fail?  launch_rc() is the answer as a value (the last line of a launch lambda), CVAE_CHECK_LAUNCH() returns on failure
inline int launch_rc() { return hipGetLastError() == hipSuccess ? CVAE_OK : CVAE_E_LAUNCH; }
#define CVAE_CHECK_LAUNCH()                                   \
    do {                                                      \
        if (launch_rc() != CVAE_OK) return CVAE_E_LAUNCH;     \
    } while (0)

// Dynamic LDS above the runtime's default limit: a kernel has to have its limit raised first, and that attribute belongs to the CURRENT DEVICE's copy
// of the kernel.  Every launch that may need it calls cvae_allow_lds<kernel>(dynamic bytes[, the kernel's static LDS]) before its entry point's first
// launch, so that a refusal leaves nothing written.  At or below 48 KiB nothing is done; above, the limit becomes all that the static part leaves of a
// workgroup's 160 KiB, whatever this launch needs: one value, good for every later launch of the kernel on that device.  Stateless on purpose: the
// runtime call takes ~70 ns of host time, its own current-device query ~55 ns, so a per-device "already done" mask would save nothing, and a flag that
// ignores the device or the host thread is wrong (profiles/launch_lds.md).  The kernel is a template ARGUMENT, not a function
// argument: instances of one kernel template share their pointer type.
constexpr size_t CVAE_LDS_MAX = 160 * 1024, CVAE_LDS_OPT_IN = 48 * 1024;
template <auto KERN> int cvae_allow_lds(size_t dynamic_bytes, size_t static_bytes = 0) {
    if (dynamic_bytes <= CVAE_LDS_OPT_IN) return CVAE_OK;
    const int limit = (int)(CVAE_LDS_MAX - static_bytes);
    return hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, limit) == hipSuccess ? CVAE_OK : CVAE_E_LAUNCH;
}

// CVAE_TUNABLE(WG_TILES, 16): the constant WG_TILES is 16 unless the build passes -DCVAE_WG_TILES=<non-negative integer> (make EXTRA=-D..., then
// tools/ab.sh with CVAE_HIP_LIB).  Every file keeps its tunables in ONE block at its top, one line each.  `text` is the macro's name stringified after
// expansion: still the name when no -D defined it, the override's digits otherwise.
constexpr long long cvae_tunable(const char* name, const char* text, long long value) {
    int i = 0;
    while (name[i] && name[i] == text[i]) ++i;
    if (!name[i] && !text[i]) return value;
    long long v = 0;
    for (i = 0; text[i]; ++i) v = (text[i] >= '0' && text[i] <= '9' && v >= 0) ? v * 10 + (text[i] - '0') : -1;
    return i ? v : -1;
}
#define CVAE_STR_(x) #x
#define CVAE_STR(x) CVAE_STR_(x)
#define CVAE_TUNABLE(name, value)                                                                 \
    constexpr long long name = cvae_tunable("CVAE_" #name, CVAE_STR(CVAE_##name), value); \
    static_assert(name >= 0, "-DCVAE_" #name " takes a non-negative integer")

static inline int cvae_grid_1d(int64_t n, int block, int max_blocks = 256 * 8) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// OCP fp8 e4m3 ("e4m3fn": max 448, no infinities) — the gfx950 format (MI300X's fnuz encoding is a different one).  One byte of storage;
// values carry a per-tensor scale that lives outside the tensor (the inference-only decode path, csrc/conv_mfma.hip).
struct fp8 { unsigned char b; };
#define CVAE_FP8_MAX 448.f

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16 x) { return (float)x; }
__device__ __forceinline__ float to_f32(fp8 x) { return __builtin_amdgcn_cvt_f32_fp8((int)x.b, 0); }
template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16 from_f32<bf16>(float x) { return (bf16)x; }   // v_cvt_pk_bf16_f32: RNE, NaN-safe
// two floats -> one dword of two bf16 (lo = a): ONE v_cvt_pk_bf16_f32, where two scalar casts cost two conversions and a v_perm to join them
typedef __bf16 cvae_bf16x2 __attribute__((ext_vector_type(2)));
typedef float cvae_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack2_bf16(float a, float b) {
    const cvae_f32x2 f = {a, b};
    const cvae_bf16x2 r = __builtin_convertvector(f, cvae_bf16x2);
    return __builtin_bit_cast(uint32_t, r);
}
template <> __device__ __forceinline__ fp8 from_f32<fp8>(float x) {                       // saturating (the hardware conversion would give NaN past 448)
    x = fminf(fmaxf(x, -CVAE_FP8_MAX), CVAE_FP8_MAX);
    return fp8{(unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(x, x, 0, false) & 0xff)};
}
// N consecutive fp32 / bf16 elements <-> N floats, moved in 16-byte pieces (one 8-byte piece for four bf16); p is aligned to the piece
template <int N> __device__ __forceinline__ void load_f32(const float* p, float (&v)[N]) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
        const float4 f = ((const float4*)p)[q];
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
}
template <int N> __device__ __forceinline__ void load_f32(const bf16* p, float (&v)[N]) {
    typedef bf16 vec __attribute__((ext_vector_type(N), aligned(N < 8 ? 8 : 16)));
    const vec q = *(const vec*)p;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (float)q[i];
}
template <int N> __device__ __forceinline__ void store_from_f32(float* p, const float (&v)[N]) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) ((float4*)p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
template <int N> __device__ __forceinline__ void store_from_f32(bf16* p, const float (&v)[N]) {
    typedef uint32_t vec __attribute__((ext_vector_type(N / 2), aligned(N < 8 ? 8 : 16)));
    vec q;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) q[i] = pack2_bf16(v[2 * i], v[2 * i + 1]);
    *(vec*)p = q;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
// The refusal chains of the entry points: if (any_null(a, b)) return CVAE_E_NULLPTR; if (!all_aligned<8>(a, b, opt)) return CVAE_E_UNSUPPORTED;
// A null pointer is aligned, so an optional argument goes into all_aligned as it is and stays out of any_null.
template <typename... P> inline bool any_null(const P*... p) { return (... || (p == nullptr)); }
template <int A, typename... P> inline bool all_aligned(const P*... p) { return (... && (((uintptr_t)p & (A - 1)) == 0)); }
__host__ __device__ __forceinline__ bool finite_f64(double x) { return fabs(x) <= 1.7976931348623157e308; }          // DBL_MAX; false for a NaN

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// Block-wide sum; result valid in thread 0. `red` must hold blockDim.x/64 floats.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; ++i) r += red[i];
    return r;
}

// ---- The two fixed-order workgroup reductions of the analysis kernels (ridge, eigh, tsne, image_prep: "two runs give equal bits").  Each combines the
// threads' values in ONE order that depends on the workgroup size alone.  The two orders differ, so their sums differ in the low bits: a call site keeps
// the one it has and never switches.
// (1) The LDS tree: thread t's value goes to red[t], then for s = NT / 2 .. 1 red[t] = op(red[t], red[t + s]) in the threads t < s; every thread
// returns red[0].  Any type and any op (sum, max, an arg-max on a {value, index} pair).  A barrier at the head, none at the tail: `red` (NT elements of
// LDS) is free to reuse after the call returns only behind the barrier at the head of the next call.
template <int NT, typename T, typename Op> __device__ __forceinline__ T block_tree(T v, T* red, Op op) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = op(red[t], red[t + s]);
        __syncthreads();
    }
    return red[0];
}
// (2) The butterfly: a 64-lane xor butterfly (offsets 32 .. 1) inside each wave, then the four waves of a 256-thread workgroup in wave order.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
// NV sums over a 256-thread workgroup, the result in every thread: red holds 4 NV doubles
template <int NV> __device__ __forceinline__ void block_sum_f64(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum_f64(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[4 * k + wid] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = ((red[4 * k] + red[4 * k + 1]) + red[4 * k + 2]) + red[4 * k + 3];
}
// sum of x[0 .. n) by a 256-thread workgroup: a thread's strided terms in index order, then the butterfly
__device__ __forceinline__ double ordered_sum_f64(const double* __restrict__ x, int n, double* red) {
    double v[1] = {0.0};
    for (int j = threadIdx.x; j < n; j += 256) v[0] += x[j];
    block_sum_f64(v, red);
    return v[0];
}

// 8 floats -> 8 fp8 (e4m3) codes of v * mul, saturating at +-448 (v_cvt_pk_fp8_f32 alone would produce NaN past the range)
__device__ __forceinline__ uint2 pack8_fp8(const float (&v)[8], float mul) {
    float c[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) c[q] = __builtin_amdgcn_fmed3f(v[q] * mul, -CVAE_FP8_MAX, CVAE_FP8_MAX);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], hi, true);
    return make_uint2((unsigned)lo, (unsigned)hi);
}
// The MFMA epilogues leave lane (r, h) with channels 8h..8h+7 (`a`) and 16+8h..23+8h (`b`) of its position's 32-channel block, as 8-byte fp8 pieces.
// One v_permlane32_swap per dword hands lane h = 0 channels 0..15 and lane h = 1 channels 16..31: ONE 16-byte store per lane at channel 16 h instead
// of two 8-byte ones (the swap exchanges the first operand of lanes 32-63 with the second operand of lanes 0-31).
__device__ __forceinline__ uint4 fp8_pair_to_16(uint2 a, uint2 b) {
    const auto x = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
    const auto y = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
    return make_uint4(x[0], y[0], x[1], y[1]);
}
// fp8 side channel of a producing kernel (all members may be null): `dscale` = device floats {acc_scale, 1 / s_out8} that replace by-value scales
// (a captured training step re-reads them on every replay: delayed scaling), `out8` = a second copy of the result as fp8 codes of result / s_out8
// (what the next fp8 layer reads, while the bf16 result stays for the backward pass), `amax` = CVAE_AMAX_SLOTS words that receive max |result| as
// float bits (non-negative floats order like unsigned integers).
struct F8Side {
    const float* dscale;
    fp8* out8;
    unsigned* amax;
    // ReLU masks as bits (round 3): one bit per element of the result, in element order — dword i covers elements 32 i .. 32 i + 31 (channel counts are
    // multiples of 32: a dword is one position's 32-channel block), bit set <=> element > 0.  `bits_out`: the producing launch leaves the mask of ITS result
    // (1/16 of the bf16 bytes) so that the backward launch that applies this ReLU reads `mask_bits` instead of the whole saved activation.
    const unsigned* mask_bits;
    unsigned* bits_out;
};
// this lane's two mask bytes (channels 8h..8h+7 -> `b0`, 16+8h..23+8h -> `b1` of its position's 32-channel block) -> the block's dword, in the lanes with
// h = 0 (one v_permlane32_swap; every lane must take part)
__device__ __forceinline__ unsigned mask_bytes_to_dword(unsigned b0, unsigned b1) {
    const unsigned a = b0 | (b1 << 16);
    const auto x = __builtin_amdgcn_permlane32_swap(a, a, false, false);       // lanes 0-31: (own, the partner lane's)
    return (x[0] & 0xffu) | ((x[1] & 0xffu) << 8) | (((x[0] >> 16) & 0xffu) << 16) | ((x[1] >> 16) << 24);
}
__device__ __forceinline__ unsigned mask_byte_of(const float (&v)[8]) {
    unsigned b = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) b |= (v[q] > 0.f ? 1u : 0u) << q;
    return b;
}
// ---- epilogue of a 32x32 MFMA whose A operand was the WEIGHT fragment: D rows are output channels, D columns are positions.  Lane (r, h) holds, for
// position r, channels (e & 3) + 8 (e >> 2) + 4 h of the 32-channel block in acc[e].  Two v_permlane32_swap per register pair regroup them so that the lane
// owns two 8-channel pieces, v[j] = channels 16 j + 8 h .. + 7 (float v[2][8]): each ONE 16-byte (bf16) store and ONE 16-byte mask load instead of eight
// 2-byte ones.  Every lane of the wave must take part.  A macro, not a function: every function form tried (accumulator by reference, by value) moved
// instructions in the epilogues that use it.
#define REGROUP_D32(acc, v)                                                                                                                      \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                                                           \
        const auto lo_ = __builtin_amdgcn_permlane32_swap(__float_as_uint((acc)[i_]), __float_as_uint((acc)[4 + i_]), false, false);              \
        const auto hi_ = __builtin_amdgcn_permlane32_swap(__float_as_uint((acc)[8 + i_]), __float_as_uint((acc)[12 + i_]), false, false);         \
        (v)[0][i_] = __uint_as_float(lo_[0]); (v)[0][4 + i_] = __uint_as_float(lo_[1]);                                                          \
        (v)[1][i_] = __uint_as_float(hi_[0]); (v)[1][4 + i_] = __uint_as_float(hi_[1]);                                                          \
    }
// max |.| of the workgroup (`red`: one float per wave, in LDS), then ONE atomicMax per WORKGROUP on the slot of its linear index: with
// CVAE_AMAX_SLOTS = 4096 the workgroups of a launch rarely share a word.  (One atomic per wave on 64 slots cost the 64 -> 32 channel layer 14 of
// its 23 us: same-address atomics serialise at the memory side at ~100 ns each.)  Every thread of the workgroup must call this.
__device__ __forceinline__ void amax_publish_wg(unsigned* slots, float amx, unsigned wg, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amx = fmaxf(amx, __shfl_xor(amx, o, 64));       // not wave_max(): the call form reorders two instructions in every conv epilogue
    const int nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = red[0];
        for (int i = 1; i < nw; ++i) m = fmaxf(m, red[i]);
        if (m > 0.f) atomicMax(slots + (wg & (CVAE_AMAX_SLOTS - 1)), __float_as_uint(m));
    }
}

__device__ __forceinline__ float apply_act(float v, int act) {
    switch (act) {
        case CVAE_ACT_RELU: return v > 0.f ? v : 0.f;
        case CVAE_ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
        case CVAE_ACT_LEAKY02: return v > 0.f ? v : 0.2f * v;
        case CVAE_ACT_LEAKY001: return v > 0.f ? v : 0.01f * v;
        default: return v;
    }
}
// The same with the activation fixed at compile time where a launch can afford a template instance per code: EPI 0 = none, 1 = ReLU
// (one v_max), 2 = the runtime code.  A runtime switch inside an unrolled epilogue compiles to a scalar branch PER ELEMENT (~100 taken
// branches per wave in the single-channel kernels), which costs more than the arithmetic it selects.
// ReLU as ONE instruction: fmaxf(v, 0) on a value the compiler cannot prove canonical (an MFMA result read back from an AGPR, a lane swap) costs
// a second v_max that quietens a possible signalling NaN first (and it folds v_med3(v, 0, inf) back into that pair), hence the asm.  NaN -> 0.
__device__ __forceinline__ float relu_f32(float v) {
    float r;
    asm("v_max_f32_e32 %0, 0, %1" : "=v"(r) : "v"(v));
    return r;
}
template <int EPI> __device__ __forceinline__ float apply_act_t(float v, int act) {
    if (EPI == 0) return v;
    if (EPI == 1) return relu_f32(v);
    return apply_act(v, act);
}
#define CVAE_EPI_OF(act) ((act) == CVAE_ACT_NONE ? 0 : ((act) == CVAE_ACT_RELU ? 1 : 2))
// Runtime -> template lifting on the host, each written once: f receives the value as a std::integral_constant (nd, EPI, a flag) or as a value of the
// element type (dtype), e.g.  with_epi(act, [&](auto epi) { launch<decltype(epi)::value>(...); return CVAE_OK; }).  This is the ONLY place where a
// runtime value becomes a template argument: kernel files nest these and name each argument once (constexpr bool VEC = ...), they define no launch
// macros.  with_dtype answers CVAE_E_DTYPE for every code that is not an element type, so no launch is reachable with one; an
// entry point whose contract puts the dtype check earlier asks dtype_ok() there.
template <int V> using Int = std::integral_constant<int, V>;
inline bool dtype_ok(int dtype) { return dtype == CVAE_F32 || dtype == CVAE_BF16; }
template <typename F> auto with_nd(int nd, F&& f) { return nd == 3 ? f(Int<3>{}) : f(Int<2>{}); }
template <typename F> int with_dtype(int dtype, F&& f) { return dtype == CVAE_BF16 ? f(bf16{}) : (dtype == CVAE_F32 ? f(float{}) : CVAE_E_DTYPE); }
template <typename F> int with_dtype2(int da, int db, F&& f) {      // two independent element types, f(a, b)
    return with_dtype(da, [&](auto a) { return with_dtype(db, [&](auto b) { return f(a, b); }); });
}
template <typename F> auto with_epi(int act, F&& f) { return CVAE_EPI_OF(act) == 0 ? f(Int<0>{}) : (CVAE_EPI_OF(act) == 1 ? f(Int<1>{}) : f(Int<2>{})); }
template <typename F> auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// derivative expressed through the activation OUTPUT y
__device__ __forceinline__ float act_grad_from_out(float y, int act) {
    switch (act) {
        case CVAE_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        case CVAE_ACT_SIGMOID: return y * (1.f - y);
        case CVAE_ACT_LEAKY02: return y > 0.f ? 1.f : 0.2f;
        case CVAE_ACT_LEAKY001: return y > 0.f ? 1.f : 0.01f;
        default: return 1.f;
    }
}

// 8 fp8 (e4m3) codes -> 8 bf16 (exact: every e4m3 value is a bf16 value)
__device__ __forceinline__ uint4 fp8x8_to_bf16x8(uint2 c) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
    const auto d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
    return make_uint4(pack2_bf16(a[0], a[1]), pack2_bf16(b[0], b[1]), pack2_bf16(d[0], d[1]), pack2_bf16(e[0], e[1]));
}

// ---- Philox4x32-10 -> four N(0,1) draws (Box-Muller), shared by cvae_philox_normal* (losses.hip) and the bottleneck's first launch (bottleneck.hip):
// counter words 0-1 = position in the stream (4 normals each), words 2-3 = subsequence, key = seed.
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
// the ten rounds: counter (c0 .. c3) -> the four output words, in place
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
}
__device__ __forceinline__ void philox_normal4(uint64_t ctr, uint64_t subseq, uint64_t seed, float v[4]) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = (uint32_t)subseq, c3 = (uint32_t)(subseq >> 32);
    philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u0 = ((float)(c0 >> 8) + 0.5f) * (1.f / 16777216.f), u1 = ((float)(c1 >> 8) + 0.5f) * (1.f / 16777216.f);
    const float u2 = ((float)(c2 >> 8) + 0.5f) * (1.f / 16777216.f), u3 = ((float)(c3 >> 8) + 0.5f) * (1.f / 16777216.f);
    const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
    sincosf(6.283185307179586f * u1, &v[1], &v[0]);
    sincosf(6.283185307179586f * u3, &v[3], &v[2]);
    v[0] *= r0; v[1] *= r0; v[2] *= r1; v[3] *= r1;
}

// Adaptive average pooling (torch): output index o of `out` averages inputs [pool_lo, pool_hi) of `in`
template <typename I> __device__ __forceinline__ I pool_lo(I o, I in, I out) { return (o * in) / out; }
template <typename I> __device__ __forceinline__ I pool_hi(I o, I in, I out) { return ((o + 1) * in + out - 1) / out; }

// torch upsample_{bi,tri}linear, align_corners=False: src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out (float).  I = the index width of the
// calling kernel (int or int64_t); the weights do not depend on it.
template <typename I> struct LinTap { I i0, i1; float w0, w1; };
template <typename I> __device__ __forceinline__ LinTap<I> lin_tap(I o, I in, float scale) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    LinTap<I> t;
    t.i0 = (I)s;
    if (t.i0 > in - 1) t.i0 = in - 1;
    t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
    t.w1 = s - (float)t.i0;
    t.w0 = 1.f - t.w1;
    return t;
}
// weights with which outputs j0 .. j0 + 3 (j0 = 2 i - 1) of a 2x-resized axis read source index i; an unstrided axis (2D depth) reads itself
struct Win4 { int j0; float w[4]; };
template <typename I> __device__ __forceinline__ Win4 win4(int i, int in, int out, float scale, bool strided) {
    Win4 r;
    if (!strided) { r.j0 = i; r.w[0] = 1.f; r.w[1] = r.w[2] = r.w[3] = 0.f; return r; }
    r.j0 = 2 * i - 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = r.j0 + c;
        float wv = 0.f;
        if (j >= 0 && j < out) {
            const LinTap<I> t = lin_tap<I>(j, in, scale);
            wv = (t.i0 == i ? t.w0 : 0.f) + (t.i1 == i ? t.w1 : 0.f);
        }
        r.w[c] = wv;
    }
    return r;
}
