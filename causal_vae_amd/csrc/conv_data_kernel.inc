// conv_data_kernel.inc — the text of the down / up tile kernel, included twice by conv_mfma.hip: with CONV_GATED 0 as conv_data_kernel (the kernel every existing launch
// runs: its signature and machine code are what they were when the text stood in conv_mfma.hip) and with CONV_GATED 1 as conv_data_gated_kernel, which takes one more
// argument, gate_slope, and MULTIPLIES the fp32 value by it where the mask is not positive instead of zeroing it: the LeakyReLU derivative of the producing
// activation, read off its output (cvae_conv_down_bwd_data).  CONV_GATE_PARAM / CONV_GATE_OFF come from conv_mfma.hip.
#if CONV_GATED
#define CONV_DATA_KERNEL conv_data_gated_kernel
#else
#define CONV_DATA_KERNEL conv_data_kernel
#endif
template <typename T, int ND, bool UP, int WM, int WN, int MI, int NI, int EPI, int KH = 1, typename TO = T, bool BD = false, int TS = 1, int XB = 1>
__global__ __launch_bounds__(WM * WN * TS * 64, BD ? 2 : 1) void CONV_DATA_KERNEL(const T* __restrict__ in, const T* __restrict__ wp, const float* __restrict__ bias,
                                                                  const TO* __restrict__ mask, TO* __restrict__ out, ConvGeom g, int act,
                                                                  float* __restrict__ ws, int ksplit, float acc_scale, float out_scale, F8Side f8 CONV_GATE_PARAM) {
    constexpr bool F8 = IsF8<T>::value;
    static_assert(!F8 || sizeof(TO) <= 2, "fp8 products leave as bf16 or as fp8 codes");
    static_assert(TS == 1 || (TS == 2 && BD && MI % 2 == 0), "the K split needs the per-wave weight fetch and an even number of M sub-tiles");
    constexpr int NT = WM * WN * TS * 64;
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    using TL = Tile<ND, BM>;
    constexpr int TD = TL::TD, TH = TL::TH, TW = TL::TW;
    constexpr int STR = UP ? 1 : 2;
    // UP: an output parity class reads q - 1 + pr + {0, 1} per dimension, so its halo box is (T + 1)^nd with the origin shifted by the
    // parity — 405 instead of the parity-independent 600 positions for 4 x 8 x 8 tiles (the halo loads are the largest single cost of
    // the `up` launches: 29 of 78 us on enc2's backward-data by ablation).
    constexpr int ID = (ND == 3) ? (UP ? TD + 1 : 2 * TD + 2) : 1;
    // XB == 2: a layer at most TW / 2 wide puts two samples side by side in x (the 4^3 decoder input would leave half of every MFMA row tile
    // empty): sample s owns tile columns [s TW / 2, (s + 1) TW / 2) and its own HWS halo columns, so a row of the halo is two sample rows with
    // the zero padding of each in place; a tile column w reads slot w + s (+ tap), which is one more term in the per-lane base.
    static_assert(XB == 1 || XB == 2, "one sample per tile, or two side by side in x");
    constexpr int IH = UP ? TH + 1 : 2 * TH + 2, IW = (UP ? TW + 1 : 2 * TW + 2) + (XB - 1) * (UP ? 1 : 2), HWS = IW / XB;
    constexpr int NPOS = ID * IH * IW;
    constexpr int FB = 8 * sizeof(T);                    // bytes of one fragment piece (8 channels)
    constexpr int NG = UP ? (ND == 3 ? 2 : 1) : (ND == 3 ? 16 : 4);   // tap groups of 4
    using ST = SubTile<ND>;
    constexpr int RS = HaloPitch<ND, UP>::RS, NROWS = ID * IH;
    constexpr int PLANE = (UP ? 1 : 2) * NROWS * RS;     // slots of one k-half plane (down: even-x rows then odd-x rows)
    static_assert(RS >= (UP ? IW : IW / 2), "halo pitch too small");
    constexpr int HALO_BYTES = 2 * KH * PLANE * FB;           // planes: (k-step, k-half)
    // slot of halo position (z, y, x) inside a k-half plane
    auto hslot = [](int z, int y, int x) -> int {
        return UP ? (z * IH + y) * RS + x : ((x & 1) * NROWS + z * IH + y) * RS + (x >> 1);
    };
    constexpr int BT_BYTES = BD ? 0 : 4 * KH * 2 * BN * FB;       // one B buffer: [4 taps][KH k-steps][2 halves][BN]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* halo = smem;
    char* bt = smem + HALO_BYTES;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    STAMP_BEGIN();
    const int ts = wave / (WM * WN), wv = wave % (WM * WN);      // K-split group (0 when TS == 1)
    const int wm = wv / WN, wn = wv % WN;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z * XB;
    const int Cin = (UP ? g.Cs : g.Cl) / (F8 ? 2 : 1), Cout = UP ? g.Cl : g.Cs;      // fp8: input channels counted in 2-channel elements
    const int nblocks = Cout / BN;
    constexpr int NPAR = UP ? (ND == 3 ? 8 : 4) : 1;
    // blockIdx.y = (ks * NPAR + par) * nblocks + nb; par: output parity class (UP only); ks: split-K slice of the channel chunks
    const int nb = blockIdx.y % nblocks, par = (blockIdx.y / nblocks) % NPAR, ks = blockIdx.y / (nblocks * NPAR);
    const int prd = (UP && ND == 3) ? ((par >> 2) & 1) : 0, prh = UP ? ((par >> 1) & 1) : 0, prw = UP ? (par & 1) : 0;
    const int n0 = nb * BN;
    int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tw_i = tile % g.tiles_w; tile /= g.tiles_w;
    const int th_i = tile % g.tiles_h; tile /= g.tiles_h;
    const int td_i = tile;
    const int o0d = td_i * TD, o0h = th_i * TH, o0w = tw_i * TW;       // tile origin in the M grid
    // input dims
    const int in_d = UP ? g.sd : g.ld, in_h = UP ? g.sh : g.lh, in_w = UP ? g.sw : g.lw;
    const int g0d = (ND == 3) ? (UP ? o0d - 1 + prd : 2 * o0d - 1) : 0;
    const int g0h = UP ? o0h - 1 + prh : 2 * o0h - 1, g0w = UP ? o0w - 1 + prw : 2 * o0w - 1;
    const int nchunks = Cin / (16 * KH);                    // stages; the packed weights are indexed in 16-channel chunks (nch16)
    const int nch16 = Cin / 16;

    // per-lane halo base position of each M sub-tile row
    // sub-tile ms of the workgroup tile covers d = ms / HB, h in [(ms % HB) * SH, +SH), all of w (SW == TW)
    static_assert(ST::SW == TW && TH % ST::SH == 0, "sub-tile must tile the workgroup tile");
    constexpr int HB = TH / ST::SH;
    int pbase[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int ms = wm * MI + mi;
        const int w = ST::w_of(r), hh = (ms % HB) * ST::SH + ST::h_of(r), d = ms / HB;
        pbase[mi] = (UP ? (d * IH + hh) * RS + w : ((2 * d) * IH + 2 * hh) * RS + w) + ((XB == 2 && w >= TW / 2) ? 1 : 0);
    }
    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

    auto tap_halo_off = [&](int grp, int j) -> int {
        if (!UP) {
            const int kd = (ND == 3) ? (grp >> 2) : 0, kh = (ND == 3) ? (grp & 3) : grp;
            return ((j & 1) * NROWS + kd * IH + kh) * RS + (j >> 1);      // kw = j: x-parity plane j & 1, slot shift j >> 1
        } else {
            const int a = (ND == 3) ? grp : 0, bb = j >> 1, c = j & 1;
            return (a * IH + bb) * RS + c;                                 // the halo origin already carries the parity
        }
    };
    auto tap_weight_idx = [&](int grp, int j) -> int {
        if (!UP) return grp * 4 + j;
        const int a = (ND == 3) ? grp : 0, bb = j >> 1, c = j & 1;
        const int kd = (ND == 3) ? (3 - prd - 2 * a) : 0, kh = 3 - prh - 2 * bb, kw = 3 - prw - 2 * c;
        return (kd * 4 + kh) * 4 + kw;
    };
    // ---- halo staging plan: the (position, half) pieces this thread moves are the same for every channel chunk ----
    constexpr int PPP = 2 * KH;                            // 8-channel pieces per position per stage
    constexpr int HN = (NPOS * PPP + NT - 1) / NT;
    int hoff[HN];                                          // element offset of the piece at chunk 0, or -1 (zero fill)
    int hdst[HN];                                          // its LDS byte offset, or -1 (past the halo box)
    {
        // piece t + i NT = (position t / PPP + i PSTEP, half t % PPP): the position's (x, y, z) is stepped, not divided (the divisions were
        // ~3 k cycles at the head of every workgroup, 10-15 % of the lifetime of the small layers' workgroups)
        static_assert(NT % PPP == 0, "a position's pieces stay in one pass");
        constexpr int PSTEP = NT / PPP, DX = PSTEP % IW, DY = (PSTEP / IW) % IH, DZ = PSTEP / (IW * IH);
        const int half = t % PPP, pos0 = t / PPP;
        int x = pos0 % IW, y = (pos0 / IW) % IH, z = pos0 / (IW * IH);
#pragma unroll
        for (int i = 0; i < HN; ++i) {
            const int sx = (XB == 2 && x >= HWS) ? 1 : 0;   // sample of this halo column (its columns restart at the sample's own left padding)
            const int gz = g0d + z, gy = g0h + y, gx = g0w + x - sx * HWS;
            const bool inbox = z < ID;
            const bool ok = inbox & (gz >= 0) & (gz < in_d) & (gy >= 0) & (gy < in_h) & (gx >= 0) & (gx < in_w) & (b + sx < g.B);
            hoff[i] = ok ? ((((sx * in_d + gz) * in_h + gy) * in_w + gx) * Cin + 8 * half) : -1;
            hdst[i] = inbox ? (half * PLANE + hslot(z, y, x)) * FB : -1;
            x += DX; if (x >= IW) { x -= IW; y += 1; }
            y += DY; if (y >= IH) { y -= IH; z += 1; }
            if (y >= IH) { y -= IH; z += 1; }
            z += DZ;
        }
    }
    const T* in_b = in + (size_t)b * in_d * in_h * in_w * Cin;
    constexpr int BP = (4 * KH * 2 * BN) / NT;             // weight pieces per thread per tap group
    static_assert((4 * KH * 2 * BN) % NT == 0, "weight panel must divide evenly over the workgroup");
    auto load_b = [&](Piece<T> (&pb)[BP], int chunk, int grp) {
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            const int it = t + i * NT, half = it & 1, n = (it >> 1) % BN, kk = it / (2 * BN) % KH, j = it / (2 * BN * KH);
            const int wt = tap_weight_idx(grp, j);
            piece_load<T>(pb[i], wp + (((size_t)wt * nch16 + chunk * KH + kk) * Cout + n0 + n) * 16 + 8 * half, true);
        }
    };
    auto store_b = [&](const Piece<T> (&pb)[BP], int buf) {
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            const int it = t + i * NT, half = it & 1, n = (it >> 1) % BN, kk = it / (2 * BN) % KH, j = it / (2 * BN * KH);
            piece_store<T>(pb[i], bt + buf * BT_BYTES + (((j * KH + kk) * 2 + half) * BN + n) * FB);
        }
    };

    // ---- BD: k-steps of a chunk in the order the LDS form walks them (tap group, tap, k-step), cut into NGRP groups of GS steps; group g + 1
    // (or the next chunk's group 0) is in flight while group g feeds the MFMAs ----
    // With TS = 2 a wave walks its OWN steps u = 0 .. STEPS - 1 <-> stage step 2 u + ts.  The ts part never enters the loops: for KH = 1 it is the
    // tap's low bit (down: the odd-x halo plane and the next weight tap; up: one slot to the right and weight tap kw - 2), for KH = 2 the second
    // 16-channel half of the stage — a constant offset of this wave's LDS and weight base addresses.
    constexpr int STEPS = NG * 4 * KH / TS, GS = STEPS >= 64 ? BD_GS : (STEPS >= 16 ? (MI >= 4 ? 4 : 8) : STEPS / 2), NGRP = STEPS / GS;      // MI = 4: a step is 4 MFMAs, 4 steps are as long as 8
    static_assert(!BD || (NGRP % 2 == 0 && GS * NGRP == STEPS && (GS * TS) % KH == 0), "BD walks the groups in pairs");
    static_assert(TS == 1 || KH <= 2, "K split: one or two k-steps per stage");
    const long long w_tap = (long long)nch16 * Cout * 16;     // elements between two taps of the packed panels
    const long long w_ts = (TS == 1) ? 0 : (KH == 2 ? (long long)ts * Cout * 16 : (UP ? -2 * ts * w_tap : ts * w_tap));
    const int a_ts = (TS == 1) ? 0 : (KH == 2 ? ts * 2 * PLANE : (UP ? ts : ts * NROWS * RS));
    const T* wl = wp + ((size_t)(n0 + wn * NI * 32 + r)) * 16 + 8 * h + w_ts;
    const char* halo_a = halo + (size_t)a_ts * FB;
    constexpr int PW = StepFrag<T>::PW;                       // k-steps per MFMA (fp8: 2)
    using SF = typename StepFrag<T>::type;
    constexpr int GSX = GS / PW;                              // MFMAs (per accumulator) of a weight group
    static_assert(GS % PW == 0, "a weight group holds whole MFMA steps");
    SF qa[BD ? GSX : 1][NI], qb[BD ? GSX : 1][NI];
    auto load_q = [&](SF (&q)[BD ? GSX : 1][NI], int chunk, int gidx) {
#pragma unroll
        for (int ix = 0; ix < GSX; ++ix) {
            const T* wsrc[2];
#pragma unroll
            for (int u = 0; u < PW; ++u) {
                const int i = ix * PW + u;
                const int kk = (i * TS) % KH, tj = gidx * (GS * TS / KH) + (i * TS) / KH;
                const int wt = tap_weight_idx(tj >> 2, tj & 3);
                wsrc[u] = wl + (size_t)(wt * nch16 + chunk * KH + kk) * Cout * 16;
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) load_step(q[ix][ni], (const char*)(wsrc[0] + (size_t)ni * 32 * 16), (const char*)(wsrc[PW - 1] + (size_t)ni * 32 * 16));
        }
    };
    STAMP(1);
    const int chunk_per = nchunks / ksplit;                 // host guarantees ksplit divides nchunks
    // what the epilogue needs from memory — this lane's bias values and ReLU-mask pieces — is requested now, not in the epilogue, where each was
    // an exposed global round trip at the end of every workgroup
    constexpr int MO = MI / TS;                               // M sub-tiles this wave finishes (TS = 2: the other half goes to its partner wave)
    const int mi0 = ts * MO;
    float bpre[NI][2][8];
    unsigned mbw[MO][NI];                                    // ReLU mask of this lane's channels, as bits of the position's 32-channel block dword
    const bool masked = !F8 && (mask || f8.mask_bits);
    const int out_d = UP ? g.ld : g.sd, out_h = UP ? g.lh : g.sh, out_w = UP ? g.lw : g.sw;
    if (ksplit == 1) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h;
#pragma unroll
                for (int q = 0; q < 8; ++q) bpre[ni][j][q] = bias ? bias[c + q] : 0.f;
            }
        if (masked) {                                        // fp8 products are forward products: no mask
#pragma unroll
            for (int mo = 0; mo < MO; ++mo) {
                const int mi = mi0 + mo, ms = wm * MI + mi;
                const int wt = ST::w_of(r), sx = (XB == 2 && wt >= TW / 2) ? 1 : 0, w = wt - sx * (TW / 2);
                const int hh = (ms % HB) * ST::SH + ST::h_of(r), d = ms / HB;
                int od, oh, ow;
                if (UP) { od = (ND == 3) ? 2 * (o0d + d) + prd : 0; oh = 2 * (o0h + hh) + prh; ow = 2 * (o0w + w) + prw; }
                else { od = o0d + d; oh = o0h + hh; ow = o0w + w; }
                const bool ok = od < out_d && oh < out_h && ow < out_w && b + sx < g.B;
                const size_t pidx = ok ? ((((size_t)(b + sx) * out_d + od) * out_h + oh) * out_w + ow) * Cout : 0;
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    if (f8.mask_bits) {                      // one dword per (position, 32-channel block) instead of two 16-byte pieces of the saved activation
                        mbw[mo][ni] = f8.mask_bits[(pidx + n0 + (wn * NI + ni) * 32) >> 5];
                    } else {                                 // the activation itself as the mask (callers without the bit form): turned into bits here
                        unsigned wbits = 0;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            Piece<TO> mp;
                            piece_load_raw<TO>(mp, mask + pidx + n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h);
                            const TO* mv = (const TO*)&mp;
#pragma unroll
                            for (int q = 0; q < 8; ++q) wbits |= (to_f32(mv[q]) > 0.f ? 1u : 0u) << (16 * j + 8 * h + q);
                        }
                        mbw[mo][ni] = wbits;
                    }
                }
            }
        }
    }
    // UP with 32-channel stages (long K loops on small grids): the NEXT stage's halo is requested right after this stage's LDS image is
    // complete and lands under the tap loop (-5 %).  Elsewhere the prefetch loses: DOWN stages 14 pieces per thread (registers), and the
    // Cin = 64 `up` launches fill the chip, where the co-resident workgroups already hide the stage (+4 % measured).
    constexpr bool HPRE = UP && KH == 2;
    // Groups gp (weights in qa) and gp + 1 (qb) as ONE run of 2 GS k-steps; the group after them goes back into qa once qa is spent.  The activation
    // fragments are software-pipelined by hand: the ds_reads of step i + APD are issued in front of the MFMAs of step i (APD + 1 register slots), so an
    // MFMA never waits for a read issued right before it — left to itself the compiler emits read / s_waitcnt / MFMA per step and the loop runs at
    // LDS latency (~35 % of the MFMA rate by the stamp probes, one wave per SIMD).
    auto bd_pair = [&](int chunk, int gp) {
        // in MFMA steps (fp8: one step = two k-steps).  MI = 4: 4 reads per k-step, 2 k-steps ahead is as many in flight
        constexpr int NS = 2 * GSX, APW = (MI >= 4) ? 2 / PW : (APIPE + PW - 1) / PW, APD = APW < NS ? APW : NS - 1;
        load_q(qb, chunk, gp + 1);
        SF ar[APD + 1][MI];
        auto lda = [&](int slot, int ix) {
            int off[2];
#pragma unroll
            for (int u = 0; u < PW; ++u) {
                const int i = ix * PW + u;
                const int gidx = gp + i / GS, ii = i % GS;
                const int kk = (ii * TS) % KH, tj = gidx * (GS * TS / KH) + (ii * TS) / KH;
                off[u] = (kk * 2 + h) * PLANE + tap_halo_off(tj >> 2, tj & 3);
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) load_step(ar[slot][mi], halo_a + (size_t)(off[0] + pbase[mi]) * FB, halo_a + (size_t)(off[PW - 1] + pbase[mi]) * FB);
        };
#pragma unroll
        for (int d = 0; d < APD; ++d) lda(d, d);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (i + APD < NS) lda((i + APD) % (APD + 1), i + APD);
            if (i == GSX) {
                const bool wrap = gp + 2 >= NGRP;
                if (!wrap || chunk + 1 < (ks + 1) * chunk_per) load_q(qa, wrap ? chunk + 1 : chunk, wrap ? 0 : gp + 2);
            }
            __builtin_amdgcn_sched_barrier(0);             // keep the reads where they are written: the scheduler would sink them back to their uses
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) mma(acc[mi][ni], (i < GSX ? qa[i % GSX] : qb[i % GSX])[ni], ar[i % (APD + 1)][mi]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto bd_chunk = [&](int chunk) {
        if constexpr (NGRP > 2) {                           // 3D down: 64 taps; rolled, or the unrolled LDS reads spill
#pragma unroll 1
            for (int gp = 0; gp < NGRP; gp += 2) bd_pair(chunk, gp);
        } else {
            bd_pair(chunk, 0);
        }
    };
    if constexpr (BD) load_q(qa, ks * chunk_per, 0);
    Piece<T> hp[HN];
    if (HPRE) {
#pragma unroll
        for (int i = 0; i < HN; ++i) piece_load<T>(hp[i], in_b + (hoff[i] < 0 ? 0 : hoff[i]) + ks * chunk_per * (16 * KH), hoff[i] >= 0);
    }
    for (int chunk = ks * chunk_per; chunk < (ks + 1) * chunk_per; ++chunk) {
        {
            Piece<T> pb0[BP];
            if (!HPRE) {
#pragma unroll
                for (int i = 0; i < HN; ++i) piece_load<T>(hp[i], in_b + (hoff[i] < 0 ? 0 : hoff[i]) + chunk * (16 * KH), hoff[i] >= 0);
            }
            if constexpr (!BD) load_b(pb0, chunk, 0);
            __syncthreads();                               // previous chunk's readers are done with halo + B buffers
            if (chunk - ks * chunk_per < 8) STAMP(2 + 3 * (chunk - ks * chunk_per));
#pragma unroll
            for (int i = 0; i < HN; ++i)
                if (hdst[i] >= 0) piece_store<T>(hp[i], halo + hdst[i]);
            if constexpr (!BD) store_b(pb0, 0);
        }
        __syncthreads();
        if (chunk - ks * chunk_per < 8) STAMP(3 + 3 * (chunk - ks * chunk_per));
        if (HPRE && chunk + 1 < (ks + 1) * chunk_per) {
#pragma unroll
            for (int i = 0; i < HN; ++i) piece_load<T>(hp[i], in_b + (hoff[i] < 0 ? 0 : hoff[i]) + (chunk + 1) * (16 * KH), hoff[i] >= 0);
        }
        if constexpr (BD) {
            bd_chunk(chunk);
        } else {
            // Weight panels ride a 2-deep ring: the panel of group g+2 is loaded into registers at the start of group g and
            // stored to LDS at the end of group g+1, so every panel load has two groups of MFMA work to land (one group is
            // shorter than the L2 latency).  The loop is unrolled by two so the register sets pbA / pbB stay static.
            auto taps = [&](int grp, const char* btb) {
    #pragma unroll
                for (int sp = 0; sp < 4 * KH; sp += PW) {   // k-steps (tap j, k-step kk); fp8 feeds one K = 64 instruction per pair
                    SF a[MI], bf[NI];
                    int aoff[2], boff[2];
    #pragma unroll
                    for (int u = 0; u < PW; ++u) {
                        const int j = (sp + u) / KH, kk = (sp + u) % KH;
                        aoff[u] = (kk * 2 + h) * PLANE + tap_halo_off(grp, j);
                        boff[u] = ((j * KH + kk) * 2 + h) * BN;
                    }
    #pragma unroll
                    for (int mi = 0; mi < MI; ++mi) load_step(a[mi], halo + (size_t)(aoff[0] + pbase[mi]) * FB, halo + (size_t)(aoff[PW - 1] + pbase[mi]) * FB);
    #pragma unroll
                    for (int ni = 0; ni < NI; ++ni) load_step(bf[ni], btb + (boff[0] + (wn * NI + ni) * 32 + r) * FB, btb + (boff[PW - 1] + (wn * NI + ni) * 32 + r) * FB);
    #pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
    #pragma unroll
                        for (int ni = 0; ni < NI; ++ni) mma(acc[mi][ni], bf[ni], a[mi]);     // D = W^T x X^T: rows = channels (see epilogue)
                }
            };
            Piece<T> pbA[BP], pbB[BP];
            if (NG > 1) load_b(pbA, chunk, 1);
    #pragma unroll 1
            for (int grp = 0; grp < NG; grp += 2) {
                if (grp + 2 < NG) load_b(pbB, chunk, grp + 2);
                taps(grp, bt);
                if (grp + 1 < NG) store_b(pbA, 1);
                __syncthreads();
                if (grp + 1 < NG) {
                    if (grp + 3 < NG) load_b(pbA, chunk, grp + 3);
                    taps(grp + 1, bt + BT_BYTES);
                    if (grp + 2 < NG) store_b(pbB, 0);
                    __syncthreads();
                }
            }
        }
        if (chunk - ks * chunk_per < 8) STAMP(4 + 3 * (chunk - ks * chunk_per));
    }
    STAMP(26);

    // ---- epilogue.  The MFMAs ran with the WEIGHT fragment as the A operand (D rows are output channels, D columns positions): REGROUP_D32, common.h.
    // The exchange and the epilogue index the accumulators with ts: written once as a generic lambda and called with the wave's ts as a compile-time
    // constant (a run-time index would put the accumulator array in scratch memory)
    float amx = 0.f;                                          // fp8 side channel: largest |result| this lane stored
    const float accs = (F8 && f8.dscale) ? f8.dscale[0] : acc_scale, o8s = (F8 && f8.dscale) ? f8.dscale[1] : out_scale;
    auto finish = [&](auto TSV) {
        constexpr int tsc = decltype(TSV)::value, mi0c = tsc * MO;
        if constexpr (TS == 2) {
            // each wave hands the accumulators of the partner's M sub-tiles over through LDS (the halo is spent) and adds what the partner hands it
            __syncthreads();
            float4* xb = (float4*)smem;
            const int pw = wave ^ (WM * WN);
#pragma unroll
            for (int mo = 0; mo < MO; ++mo)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        const f32x16& a = acc[(1 - tsc) * MO + mo][ni];
                        xb[(((size_t)wave * MO + mo) * NI + ni) * 4 * 64 + e4 * 64 + lane] = make_float4(a[4 * e4], a[4 * e4 + 1], a[4 * e4 + 2], a[4 * e4 + 3]);
                    }
            __syncthreads();
#pragma unroll
            for (int mo = 0; mo < MO; ++mo)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        const float4 v = xb[(((size_t)pw * MO + mo) * NI + ni) * 4 * 64 + e4 * 64 + lane];
                        f32x16& a = acc[mi0c + mo][ni];
                        a[4 * e4] += v.x; a[4 * e4 + 1] += v.y; a[4 * e4 + 2] += v.z; a[4 * e4 + 3] += v.w;
                    }
        }
#pragma unroll
    for (int mo = 0; mo < MO; ++mo) {
        const int mi = mi0c + mo;
        const int ms = wm * MI + mi;                                            // same lane -> position map as pbase
        const int wt = ST::w_of(r), sx = (XB == 2 && wt >= TW / 2) ? 1 : 0, w = wt - sx * (TW / 2);
        const int hh = (ms % HB) * ST::SH + ST::h_of(r), d = ms / HB;
        int od, oh, ow;
        if (UP) { od = (ND == 3) ? 2 * (o0d + d) + prd : 0; oh = 2 * (o0h + hh) + prh; ow = 2 * (o0w + w) + prw; }
        else { od = o0d + d; oh = o0h + hh; ow = o0w + w; }
        const bool ok = od < out_d && oh < out_h && ow < out_w && b + sx < g.B;
        const size_t pidx = ((((size_t)(b + sx) * out_d + od) * out_h + oh) * out_w + ow) * Cout;
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            float v[2][8];
            REGROUP_D32(acc[mi][ni], v)
            if (ksplit > 1) {
                // split-K: this workgroup saw only its slice of the input channels; leave the raw fp32 partial sums in slab ks of
                // the workspace ([ks][B][positions][Cout]); conv_splitk_finish_kernel adds the slabs, bias, activation and mask.
                if (ok) {
                    float* wrow = ws + (size_t)ks * g.B * out_d * out_h * out_w * Cout + pidx;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int c = n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h;
                        *(float4*)(wrow + c) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
                        *(float4*)(wrow + c + 4) = make_float4(v[j][4], v[j][5], v[j][6], v[j][7]);
                    }
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float x = (F8 ? v[j][q] * accs : v[j][q]) + bpre[ni][j][q];
                    if (EPI == 1) x = relu_f32(x);
                    else if (EPI == 2) x = apply_act(x, act);
                    v[j][q] = x;
                }
                if (!ok) continue;
                if (masked) {
                    const unsigned mb = mbw[mo][ni] >> (16 * j + 8 * h);
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (!((mb >> q) & 1u)) v[j][q] = CONV_GATE_OFF(v[j][q]);
                }
                if constexpr (F8) {
                    if (f8.amax) {
#pragma unroll
                        for (int q = 0; q < 8; ++q) amx = fmaxf(amx, fabsf(v[j][q]));
                    }
                }
                if constexpr (sizeof(TO) == 2 && sizeof(T) == 2) {           // bf16: one v_cvt_pk_bf16_f32 per pair
                    *(uint4*)(out + pidx + c) = make_uint4(pack2_bf16(v[j][0], v[j][1]), pack2_bf16(v[j][2], v[j][3]), pack2_bf16(v[j][4], v[j][5]), pack2_bf16(v[j][6], v[j][7]));
                } else if constexpr (F8) {                                   // fp8 codes only (the inference chain between two fp8 layers): below, 16 bytes per lane
                } else {
                    Piece<TO> op;
                    TO* ov = (TO*)&op;
#pragma unroll
                    for (int q = 0; q < 8; ++q) ov[q] = from_f32<TO>(v[j][q]);
                    piece_store<TO>(op, (char*)(out + pidx + c));
                }
            }
            if (f8.bits_out) {                               // uniform: every lane takes part in the lane swap; lanes h = 0 store the block's dword
                const unsigned dw = mask_bytes_to_dword(mask_byte_of(v[0]), mask_byte_of(v[1]));
                if (ok && h == 0) f8.bits_out[(pidx + n0 + (wn * NI + ni) * 32) >> 5] = dw;
            }
            if constexpr (F8) {
                // the fp8 copy of this 32-channel block: 16 bytes per lane (all lanes take part in the lane swap; `ok` only guards the store)
                fp8* o8 = sizeof(TO) == 1 ? (fp8*)out : f8.out8;
                if (o8) {
                    const uint4 q16 = fp8_pair_to_16(pack8_fp8(v[0], o8s), pack8_fp8(v[1], o8s));
                    if (ok) *(uint4*)(o8 + pidx + n0 + (wn * NI + ni) * 32 + 16 * h) = q16;
                }
            }
        }
    }
    };
    if constexpr (TS == 2) {
        if (ts == 0) finish(std::integral_constant<int, 0>{}); else finish(std::integral_constant<int, 1>{});
    } else {
        finish(std::integral_constant<int, 0>{});
    }
    if constexpr (F8) {
        if (f8.amax && ksplit == 1) {                          // uniform over the workgroup
            __syncthreads();                                   // the LDS image (halo / accumulator exchange) is spent
            amax_publish_wg(f8.amax, amx, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), (float*)smem);
        }
    }
    STAMP_END();
}
#undef CONV_DATA_KERNEL
