// conv_up_full_kernel.inc — the text of the whole-K `up` kernel, included twice by conv_mfma.hip: with CONV_GATED 0 as conv_up_full_kernel (the kernel every existing launch
// runs: its signature and machine code are what they were when the text stood in conv_mfma.hip) and with CONV_GATED 1 as conv_up_full_gated_kernel, which takes one more
// argument, gate_slope, and MULTIPLIES the fp32 value by it where the mask is not positive instead of zeroing it: the LeakyReLU derivative of the producing
// activation, read off its output (cvae_conv_down_bwd_data).  CONV_GATE_PARAM / CONV_GATE_OFF come from conv_mfma.hip.
#if CONV_GATED
#define CONV_UP_FULL_KERNEL conv_up_full_gated_kernel
#else
#define CONV_UP_FULL_KERNEL conv_up_full_kernel
#endif
template <typename T, int ND, int WM, int WN, int MI, int NI, int KCH, int EPI, typename TO = T>
__global__ __launch_bounds__(WM * WN * 64) void CONV_UP_FULL_KERNEL(const T* __restrict__ in, const T* __restrict__ wp, const float* __restrict__ bias,
                                                                     const TO* __restrict__ mask, TO* __restrict__ out, ConvGeom g, int act, int ppw,
                                                                     float acc_scale, float out_scale CONV_GATE_PARAM) {
    constexpr int NT = WM * WN * 64;
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    using TL = Tile<ND, BM>;
    constexpr int TD = TL::TD, TH = TL::TH, TW = TL::TW;
    constexpr int ID = (ND == 3) ? TD + 2 : 1, IH = TH + 2, IW = TW + 2, NPOS = ID * IH * IW;
    constexpr int FB = 8 * sizeof(T);
    using ST = SubTile<ND>;
    constexpr int RS = HaloPitch<ND, true>::RS, NROWS = ID * IH, NSLOT = NROWS * RS;
    static_assert(RS >= IW, "halo pitch too small");
    constexpr int NPC = 2 * KCH, SPITCH = NPC + 1;           // 8-channel pieces per position; slot pitch in pieces (odd)
    constexpr int NTAP = (ND == 3) ? 8 : 4;                  // taps per parity class (= number of parity classes)
    constexpr int HTAP = NTAP / 2, PT = KCH * 2 * BN, HP_PIECES = HTAP * PT, HP_BYTES = HP_PIECES * FB, HPP = HP_PIECES / NT;
    static_assert(PT % NT == 0, "a tap's weight pieces must be a whole number of workgroup passes");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* halo = smem;
    char* wbuf = smem + (size_t)NSLOT * SPITCH * FB;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    STAMP_BEGIN();
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z;
    const int Cin = g.Cs, Cout = g.Cl;
    const int nblocks = Cout / BN;
    const int nb = blockIdx.y % nblocks, pg = blockIdx.y / nblocks;
    const int n0 = nb * BN;
    int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tw_i = tile % g.tiles_w; tile /= g.tiles_w;
    const int th_i = tile % g.tiles_h; tile /= g.tiles_h;
    const int o0d = tile * TD, o0h = th_i * TH, o0w = tw_i * TW;
    const int g0d = (ND == 3) ? o0d - 1 : 0, g0h = o0h - 1, g0w = o0w - 1;
    static_assert(ST::SW == TW && TH % ST::SH == 0, "sub-tile must tile the workgroup tile");
    constexpr int HB = TH / ST::SH;
    int pbase[MI];                                           // halo slot of this lane's position in each M sub-tile, parity (0, 0, 0), tap (0, 0, 0)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int ms = wm * MI + mi;
        pbase[mi] = ((ms / HB) * IH + (ms % HB) * ST::SH + ST::h_of(r)) * RS + ST::w_of(r);
    }
    const int par0 = pg * ppw, nhp = 2 * ppw;
    auto tap_abc = [](int tap, int& a, int& bb, int& c) { a = (ND == 3) ? (tap >> 2) : 0; bb = (tap >> 1) & 1; c = tap & 1; };
    // ---- weight half panels: hpi -> (parity par0 + hpi / 2, taps (hpi & 1) * HTAP ..); LDS image [tap][k-step][half][n] ----
    const unsigned w_lane = (unsigned)((((t / (2 * BN)) * Cout + (t >> 1) % BN) * 16 + 8 * (t & 1)) * sizeof(T));     // the thread's piece inside a pass
    const int w_slot = (t / (2 * BN)) * (2 * BN) + (t & 1) * BN + (t >> 1) % BN;
    struct HalfPanel { Piece<T> p[HPP]; };                   // by value: as reference parameters of the lambdas the two register sets ended up in scratch
    auto load_hp = [&](int hpi) -> HalfPanel {
        HalfPanel wr;
        const int par = par0 + (hpi >> 1), th = hpi & 1;
        const int prd = (ND == 3) ? ((par >> 2) & 1) : 0, prh = (par >> 1) & 1, prw = par & 1;
#pragma unroll
        for (int i = 0; i < HPP; ++i) {
            const int tl = (i * NT) / PT, k0 = ((i * NT) % PT) / (2 * BN);       // pass i: tap tl of the half, k-steps k0 .. k0 + NT / (2 BN) - 1
            int a, bb, c;
            tap_abc(th * HTAP + tl, a, bb, c);
            const int kd = (ND == 3) ? (3 - prd - 2 * a) : 0, kh = 3 - prh - 2 * bb, kw = 3 - prw - 2 * c;
            const T* wu = wp + ((size_t)(((kd * 4 + kh) * 4 + kw) * KCH + k0) * Cout + n0) * 16;     // uniform
            piece_load_raw<T>(wr.p[i], (const T*)((const char*)wu + w_lane));
        }
        return wr;
    };
    auto store_hp = [&](const HalfPanel& wr, int buf) {
#pragma unroll
        for (int i = 0; i < HPP; ++i) piece_store<T>(wr.p[i], wbuf + (size_t)buf * HP_BYTES + (size_t)(i * NT + w_slot) * FB);
    };
    f32x16 acc[MI][NI];
    const char* abase[MI];                                   // per parity: LDS address of (lane position + parity shift, piece h)
    auto compute_hp = [&](const char* wb, int th) {          // HTAP * KCH k-steps, both operands from LDS, reads APD steps ahead of their MFMAs
        constexpr int NS = HTAP * KCH, APD = APIPE < NS ? APIPE : NS - 1;
        Frag<T> ar[APD + 1][MI], br[APD + 1][NI];
        const char* bb0 = wb + (size_t)(h * BN + wn * NI * 32 + r) * FB;
        auto ld = [&](int slot, int i) {
            const int tl = i / KCH, kk = i % KCH;
            int a, bb, c;
            tap_abc(tl, a, bb, c);                            // th * HTAP + tl: the half only moves the first tap coordinate (a in 3D, bb in 2D)
            const int tapc = (ND == 3) ? ((a + th) * IH + bb) * RS + c : (bb + th) * RS + c;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) lds_load(ar[slot][mi], abase[mi] + (size_t)(tapc * SPITCH + 2 * kk) * FB);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) lds_load(br[slot][ni], bb0 + (size_t)((tl * KCH + kk) * 2 * BN + ni * 32) * FB);
        };
#pragma unroll
        for (int d = 0; d < APD; ++d) ld(d, d);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (i + APD < NS) ld((i + APD) % (APD + 1), i + APD);
            __builtin_amdgcn_sched_barrier(0);              // keep the reads where they are written: the scheduler would sink them back to their uses
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) mma(acc[mi][ni], br[i % (APD + 1)][ni], ar[i % (APD + 1)][mi]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    STAMP(1);
    HalfPanel wra = load_hp(0), wrb = wra;
    // ---- stage the whole halo (all channels), once: thread t moves piece t % NPC of positions t / NPC + i * (NT / NPC) ----
    {
        static_assert(NT % NPC == 0, "pieces of a position must stay in one pass");
        constexpr int PSTEP = NT / NPC, HN = (NPOS + PSTEP - 1) / PSTEP;
        constexpr int DX = PSTEP % IW, DY = (PSTEP / IW) % IH, DZ = PSTEP / (IW * IH);
        const T* in_b = in + (size_t)b * g.sd * g.sh * g.sw * Cin;
        const int pc = t % NPC, pos0 = t / NPC;
        int x = pos0 % IW, y = (pos0 / IW) % IH, z = pos0 / (IW * IH);
        Piece<T> hp[HN];
        int hs[HN];
#pragma unroll
        for (int i = 0; i < HN; ++i) {
            const int gz = g0d + z, gy = g0h + y, gx = g0w + x;
            const bool in_tile = z < ID;
            const bool ok = in_tile & (gz >= 0) & (gz < g.sd) & (gy >= 0) & (gy < g.sh) & (gx >= 0) & (gx < g.sw);
            piece_load<T>(hp[i], in_b + (ok ? (((size_t)gz * g.sh + gy) * g.sw + gx) * Cin + 8 * pc : 0), ok);
            hs[i] = in_tile ? ((z * IH + y) * RS + x) * SPITCH + pc : -1;
            x += DX; if (x >= IW) { x -= IW; y += 1; }
            y += DY; if (y >= IH) { y -= IH; z += 1; }
            z += DZ;
        }
        STAMP(2);
#pragma unroll
        for (int i = 0; i < HN; ++i)
            if (hs[i] >= 0) piece_store<T>(hp[i], halo + (size_t)hs[i] * FB);
    }
    store_hp(wra, 0);
    wra = load_hp(1);
    __syncthreads();
    STAMP(3);

    const int out_d = g.ld, out_h = g.lh, out_w = g.lw;
    Piece<TO> mpre[MI][NI][2];
    float bpre[NI][2][8];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h;
#pragma unroll
            for (int q = 0; q < 8; ++q) bpre[ni][j][q] = bias ? bias[c + q] : 0.f;
        }
    auto parity_begin = [&](int par) {                       // accumulators, LDS base of the parity's reads, its mask pieces
        const int prd = (ND == 3) ? ((par >> 2) & 1) : 0, prh = (par >> 1) & 1, prw = par & 1;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            abase[mi] = halo + (size_t)((pbase[mi] + (prd * IH + prh) * RS + prw) * SPITCH + h) * FB;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
        }
        if (!mask) return;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int ms = wm * MI + mi;
            const int w = ST::w_of(r), hh = (ms % HB) * ST::SH + ST::h_of(r), d = ms / HB;
            const int od = (ND == 3) ? 2 * (o0d + d) + prd : 0, oh = 2 * (o0h + hh) + prh, ow = 2 * (o0w + w) + prw;
            const bool ok = od < out_d && oh < out_h && ow < out_w;
            const size_t pidx = ok ? ((((size_t)b * out_d + od) * out_h + oh) * out_w + ow) * Cout : 0;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int j = 0; j < 2; ++j) piece_load_raw<TO>(mpre[mi][ni][j], mask + pidx + n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h);
        }
    };
    auto epilogue = [&](int par) {                           // as conv_data_kernel's, but its own text: one sample per workgroup (no b + sx), the mask as pieces of the saved activation, no side channel
        const int prd = (ND == 3) ? ((par >> 2) & 1) : 0, prh = (par >> 1) & 1, prw = par & 1;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int ms = wm * MI + mi;
            const int w = ST::w_of(r), hh = (ms % HB) * ST::SH + ST::h_of(r), d = ms / HB;
            const int od = (ND == 3) ? 2 * (o0d + d) + prd : 0, oh = 2 * (o0h + hh) + prh, ow = 2 * (o0w + w) + prw;
            const bool ok = od < out_d && oh < out_h && ow < out_w;
            const size_t pidx = ((((size_t)b * out_d + od) * out_h + oh) * out_w + ow) * Cout;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                float v[2][8];
                REGROUP_D32(acc[mi][ni], v)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int c = n0 + (wn * NI + ni) * 32 + 16 * j + 8 * h;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        float x = (sizeof(T) == 1 ? v[j][q] * acc_scale : v[j][q]) + bpre[ni][j][q];
                        if (EPI == 1) x = relu_f32(x);
                        else if (EPI == 2) x = apply_act(x, act);
                        v[j][q] = x;
                    }
                    if (!ok) continue;
                    if (mask) {
                        const TO* mv = (const TO*)&mpre[mi][ni][j];
#pragma unroll
                        for (int q = 0; q < 8; ++q)
                            if (!(to_f32(mv[q]) > 0.f)) v[j][q] = CONV_GATE_OFF(v[j][q]);
                    }
                    Piece<TO> op;
                    TO* ov = (TO*)&op;
#pragma unroll
                    for (int q = 0; q < 8; ++q) ov[q] = from_f32<TO>(sizeof(T) == 1 ? v[j][q] * out_scale : v[j][q]);
                    piece_store<TO>(op, (char*)(out + pidx + c));
                }
            }
        }
    };
    // half panels in pairs = one parity per iteration; panel hpi + 1 sits in wra, hpi + 2 is requested into wrb at the top
    for (int hpi = 0; hpi < nhp; hpi += 2) {
        const int par = par0 + (hpi >> 1);
        if (hpi + 2 < nhp) wrb = load_hp(hpi + 2);
        parity_begin(par);
        compute_hp(wbuf, 0);
        store_hp(wra, 1);
        __syncthreads();
        if (hpi + 3 < nhp) wra = load_hp(hpi + 3);
        compute_hp(wbuf + HP_BYTES, 1);
        if (hpi + 2 < nhp) store_hp(wrb, 0);
        STAMP(4 + hpi);
        epilogue(par);
        STAMP(5 + hpi);
        __syncthreads();
    }
    STAMP_END();
}
#undef CONV_UP_FULL_KERNEL
