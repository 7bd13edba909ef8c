// The backward block kernel's body (block_bwd_split.hip, which includes this file once per MFMA
// form): the kernel SW_KERNEL on fragments of shape SW_FRAG (splitwave.h Frag32 / Frag16).  The
// body stays inside the __global__ function: called from a wrapper it compiles to other code.
//
// SX (block 0, one-segment layout, d = 1, no D_0): the start conv's backward folded into the
// epilogue -- out = d loss / d e_0 is not stored; per position the wave's three dot products
// sum_c W0[k][c] out[t][c] over its 32 channels go to spart (launch_startx_gx sums the four
// waves and forms d loss / d x): no 2 GiB g_0 round trip (model.py:82-93)
// WHOLE (one-segment layout with n == 64: every tile is a whole sub-sequence, d = T / 64): both
// halo rows (p0 - 1, p0 + 64) are SAME padding, so the column tiles cover p0 .. p0 + 63 and rows
// 0 / 65 of the g_u image stay zero: no halo MFMA tile
template <bool MASKED, bool ONESEG, bool HAS_D, bool SX, bool WHOLE>
__global__ void __launch_bounds__(FT, 1) SW_KERNEL(BwdArgsS a, Layout) {
    using S = SW_FRAG;
    // the layout as compile-time constants (pick_layout: one segment or masked: M = 64 with two
    // halo rows; else segments of SEGM = 32 with their pad rows), not the launch argument
    constexpr bool GEO1 = ONESEG || MASKED;
    const Layout ly = {GEO1 ? TMS : SEGM, GEO1 ? TMS + 2 : (TMS / SEGM) * (SEGM + 2)};
    static_assert(!WHOLE || (ONESEG && !MASKED), "WHOLE is a one-segment layout");
    __shared__ __attribute__((aligned(16))) uint8_t XS[ISLOT];        // split tot image
    __shared__ __attribute__((aligned(16))) uint8_t XG[GROWS * RS];   // split g_u image
    __shared__ __attribute__((aligned(16))) uint8_t ER[2][ISLOT];     // fp32 tot + D_l rows
    __shared__ __attribute__((aligned(16))) float W0S[SX ? 3 * C : 4];   // SX: W0 [3][C]
    __shared__ uint32_t WMX[4];                                     // the drain's per-wave maxima

    const int tiles = a.T / TMS;
    const int ntiles = a.B * tiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const S fs(lane, w);                         // the lane's fragment coordinates (splitwave.h)
    const int G = (int)gridDim.x;
    STAMP_DECL

    auto tile_of = [&](int tl) { return tile_at<MASKED>(tl, a.ft, a.fn, a.d, ly); };
    auto clampt = [&](int tl) { return tl < ntiles ? tl : ntiles - 1; };
#ifdef ASTYLE_DIAG_BWD_L2ROWS
    // diagnostic build only (tools): every row load and store addresses the workgroup's first
    // tile, so the same instruction stream runs from L2 instead of HBM (results wrong)
    const Tile t0f = tile_of(blockIdx.x);
    auto memt = [&](const Tile& t) { (void)t; return t0f; };
#else
    auto memt = [&](const Tile& t) { return t; };
#endif

    // this wave's split weight halves (A: rows = channels 32 w.., K = the other side's channels)
    uint4 wr[8][2], wd[3][8][2];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl)
            wr[kb][hl] = a.wrb[((size_t)(w * 8 + kb) * 2 + hl) * 64 + lane];
#pragma unroll
    for (int tp = 0; tp < 3; ++tp)
#pragma unroll
        for (int kb = 0; kb < 8; ++kb)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
                wd[tp][kb][hl] = a.wdb[((size_t)((w * 3 + tp) * 8 + kb) * 2 + hl) * 64 + lane];
    pin_all(wd, wr);
    // the g_u image's pad / unused halo rows stay zero (only column and halo rows are written)
    for (int i = tid; i < GROWS * RS / 16; i += FT) reinterpret_cast<uint4*>(XG)[i] = make_uint4(0, 0, 0, 0);
    if (SX)   // (read after the first tile's T barrier)
        for (int i = tid; i < 3 * C; i += FT) W0S[i] = a.w0[i];

    // image row and time offset of the lane's column of column half j, column block cb
    int Lc[2][S::NCB], toff[2][S::NCB];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int cb = 0; cb < S::NCB; ++cb) {
            Lc[j][cb] = frow(fs.col(j, cb), ly);
            toff[j][cb] = MASKED ? 0 : row_toff(Lc[j][cb], ly, a.d);
        }
    // unit g of a column half = (column block S::cb(g), row block rb = g % UR): channels
    // ch0 + CHR rb .. + 3, mask group mg0 + MGR rb.  The lambdas form rb once per unit and the
    // rest from it: with S::choff(g) / S::mgoff(g) at each use the 16x16x32 kernels compile to
    // other code
    constexpr int UR = 4 / S::NCB, CHR = 32 / UR, MGR = S::NCB;
    const int ch0 = fs.ch0();     // first channel of this lane's unit 0
    const int mg0 = fs.mg0();     // mask group of unit 0
    const int mwo = fs.mword();   // the lane's word of a position's 8 mask words
    auto ctime = [&](const Tile& t, int cc, int to) { return col_time<MASKED>(t, cc, to, a.fn, a.d); };
    // g_v / g_u rows.  One-segment layouts shift the two column tiles by one row: they cover
    // image rows 2..65 (positions p0 + 1 .. p0 + 64, the right halo included), and rows 0 / 1
    // (p0 - 1, p0) are either the previous tile's rows 64 / 65 (the workgroup's previous tile is
    // the left neighbour in the same sub-sequence: copied, no MFMAs) or the halo tile's
    // (one column block: lane lc == 0 -> row 0, lc == 1 -> row 1; lanes lc >= 2 compute a copy
    // of row 0 and write it to unused row 66).  Other layouts: the tile's columns, no halo rows.
    // masked layouts have the one-segment geometry (row L = position p0 + L - 1, gathered) and
    // a tile may start / end inside a sub-sequence: the same halo rows, tap masks in g_a
    constexpr bool HALO = (ONESEG && !WHOLE) || MASKED;
    // CARRY tiles: the last tile of a sub-sequence with a next position in the clip (p0 + 64,
    // the next sub-sequence's first position, time q + 1)
    constexpr bool CARRY = ONESEG && !WHOLE && !MASKED;
    auto carry_of = [&](const Tile& t) { return CARRY && t.m0 + TMS >= a.n && t.p0 + TMS < a.T; };
    int Lv[2][S::NCB];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int cb = 0; cb < S::NCB; ++cb) Lv[j][cb] = HALO ? Lc[j][cb] + 1 : Lc[j][cb];
    const int Lh = fs.lc == 1 ? 1 : 0;
    const int Lhw = fs.lc < 2 ? Lh : TMS + 2;

    // ---- rows of the next tile: tot (-> split image) and D_l (-> residual) ----
    RowUnits<MASKED, ONESEG> ru;
    ru.init(w, lane, ly, a.d);
    float4 lt[NU], lg[NU];
    // unmasked layouts load through buffer resources of the tile (rs_t / rs_d, set with the tile)
    rsrc_t rs_t, rs_d;
    auto set_rs = [&](const Tile& t_) {
        const Tile t = memt(t_);
        if (!MASKED) {
            rs_t = ru.rsrc_of(a.tin, t, a.T, a.d);
            if (HAS_D) rs_d = ru.rsrc_of(a.dadd, t, a.T, a.d);
        }
    };
    auto load_unit = [&](const Tile& t_, int k) {
        const Tile t = memt(t_);
        if (MASKED) {
            lt[k] = ru.load(a.tin, t, k, a.T, a.fn, a.d);
            if (HAS_D) lg[k] = ru.load(a.dadd, t, k, a.T, a.fn, a.d);
        } else if (CARRY && k == NU - 1) {
            // unit 8 by 64-bit address: in a CARRY tile the lanes of row 65 (lr == 1) read the
            // next sub-sequence's first tot row (its D row stays the dummy: row 65's residual is
            // no output)
            const int q = t.tb - t.m0 * a.d;
            const float* pn = a.tin + ((size_t)t.b * a.T + q + 1) * C + ru.cq;
            const float* pr = reinterpret_cast<const float*>(
                reinterpret_cast<const char*>(a.tin + ((ptrdiff_t)t.b * a.T + t.tb - a.d) * C) + ru.unit_off(t, k, a.fn));
            lt[k] = *reinterpret_cast<const float4*>(carry_of(t) && ru.lr == 1 ? pn : pr);
            if (HAS_D) lg[k] = ru.loadb(rs_d, t, k, a.fn);
        } else {
            lt[k] = ru.loadb(rs_t, t, k, a.fn);
            if (HAS_D) lg[k] = ru.loadb(rs_d, t, k, a.fn);
        }
    };
    auto conv_unit = [&](int k, uint8_t* er, float s, uint32_t zb) {
        const float4 v = lt[k];
        float4 e = v;
        if (HAS_D) { e.x += lg[k].x; e.y += lg[k].y; e.z += lg[k].z; e.w += lg[k].w; }
        *reinterpret_cast<float4*>(er + ru.ero + 8 * k * RS) = e;
        const float sk = (zb >> k) & 1u ? 0.f : s;
        uint32_t h01, l01, h23, l23;
        split2s(v.x * sk, v.y * sk, h01, l01);
        split2s(v.z * sk, v.w * sk, h23, l23);
        uint8_t* p = XS + ru.imgo + 8 * k * RS;
        *reinterpret_cast<uint2*>(p) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(p + 256) = make_uint2(l01, l23);
    };
    // zero bits of a tile's units: a CARRY tile's row 65 is real
    auto zbits = [&](const Tile& t) {
        uint32_t z = ru.zero_bits(t, a.fn);
        if (carry_of(t) && ru.lr == 1) z &= ~(1u << (NU - 1));
        return z;
    };
    // ---- relu-mask words (u16, position-indexed): u > 0 of the tile's columns and halos,
    //      e_l > 0 of its columns ----
    //      (per column half j and column block cb: the lane's word of its column)
    uint32_t mu_c[2][S::NCB], muh_c = 0, me_c[2][S::NCB], mu_n[2][S::NCB], muh_n = 0, me_n[2][S::NCB], me_p[S::NCB] = {};
    auto load_masks = [&](const Tile& t, uint32_t (&mu)[2][S::NCB], uint32_t& muh, uint32_t (&me)[2][S::NCB]) {
        const size_t pb = (size_t)t.b * a.T + t.p0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int cb = 0; cb < S::NCB; ++cb) {
                // u > 0 of the g_v rows Lv[j][cb]; a position past the clip reads any word (its
                // tot row is zero)
                const int c = fs.col(j, cb);
                const int pv = HALO ? min(t.p0 + 1 + c, a.T - 1) : t.p0 + c;
                mu[j][cb] = a.mu[((size_t)t.b * a.T + pv) * 8 + mwo];
                me[j][cb] = a.me[(pb + c) * 8 + mwo];
            }
        if (HALO) {     // rows 0 / 1: p0 - 1 (outside the clip at p0 == 0: its tot row is zero or tap-masked), p0
            const int p = t.p0 + (fs.lc == 1 ? 0 : -1);
            muh = a.mu[((size_t)t.b * a.T + (p < 0 ? 0 : p)) * 8 + mwo];
        }
    };

    // ---- step 1: g_v of column half J (0, 1; 2 = the halo columns: column block 0 only).  Step
    //      st of a column half = (K block S::skb(st), column block S::scb(st)); the halo GEMM
    //      walks the K blocks of its one column block in 8 / NCB steps, which carry NCB side
    //      slots each ----
    typename S::Acc acc1[3];
    auto gemm1 = [&](auto j_tag, auto side) {
        constexpr int J = decltype(j_tag)::value;
        constexpr int NS = J < 2 ? 8 : 8 / S::NCB;
        S::zero(acc1[J]);
        uint4 bh[LA + 1], bl[LA + 1];
        auto bread = [&](int st, uint4& xh, uint4& xl) {
            const int kb = J < 2 ? S::skb(st) : st, cb = J < 2 ? S::scb(st) : 0;
            const int row = J < 2 ? Lv[J < 2 ? J : 0][cb] : Lh;
            const uint8_t* p = fs.bfrag(XS + row * RS, kb);
            xh = lds16(p);
            xl = lds16(p + 256);
        };
#pragma unroll
        for (int q = 0; q < LA; ++q) bread(q, bh[q], bl[q]);
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            const int kb = J < 2 ? S::skb(st) : st, cb = J < 2 ? S::scb(st) : 0, bi = st % (LA + 1);
            S::step_first(acc1[J], wr, kb, cb, bh[bi]);
            if (st + LA < NS) bread(st + LA, bh[(st + LA) % (LA + 1)], bl[(st + LA) % (LA + 1)]);
            if (J < 2) side(st);
            else { side(S::NCB * st); if (S::NCB > 1) side(S::NCB * st + 1); }   // (as a loop: other code)
            S::step_rest(acc1[J], wr, kb, cb, bh[bi], bl[bi]);
        }
    };
    // g_u of unit (J, g) (the halo tile: the units of column block 0) in two parts: mask;
    // scale + split -> image row
    float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
    // rows of half 1's first and last column block (a CARRY tile: its right-halo column 63 -> row
    // 67); initialised as an aggregate: filled by a loop over NCB it compiles to other code
    int Lv1t[2] = {Lv[1][0], Lv[1][S::NCB - 1]};
    auto gu_part = [&](int J, int g, int part, float f) {
        const int rb = g & (UR - 1), cb = S::cb(g);
        if (part == 0) {
            const uint32_t wd_ = J < 2 ? mu_c[J < 2 ? J : 0][cb] : muh_c;
            const int mg = mg0 + MGR * rb;
            const f32x4 au = S::unit(acc1[J], g);
            gq.x = keep_if(au[0], wd_, mg);
            gq.y = keep_if(au[1], wd_, 4 + mg);
            gq.z = keep_if(au[2], wd_, 8 + mg);
            gq.w = keep_if(au[3], wd_, 12 + mg);
        } else {
            // the scale after the mask (f is a power of two: the same values), so that the
            // split's low half fuses with it into one v_fma_mix_f32
            uint32_t h01, l01, h23, l23;
            split2s(gq.x * f, gq.y * f, h01, l01);
            split2s(gq.z * f, gq.w * f, h23, l23);
            uint8_t* p = XG + (J == 0 ? Lv[0][cb] : J == 1 ? Lv1t[cb] : Lhw) * RS + 2 * (ch0 + CHR * rb);
            *reinterpret_cast<uint2*>(p) = make_uint2(h01, h23);
            *reinterpret_cast<uint2*>(p + 256) = make_uint2(l01, l23);
        }
    };

    // ---- step 2: g_a of column half J; step st = (tap st >> 3, step st & 7 of the tap's K
    //      pass: S::skb, S::scb) ----
    typename S::Acc acc2[2];
    auto gemm2 = [&](auto j_tag, auto side, const Tile& cu) {
        constexpr int J = decltype(j_tag)::value;
        bool ok0[S::NCB], ok2[S::NCB];
#pragma unroll
        for (int cb = 0; cb < S::NCB; ++cb) ok0[cb] = ok2[cb] = true;
        if (MASKED) {
#pragma unroll
            for (int cb = 0; cb < S::NCB; ++cb) {
                const int pc = cu.p0 + fs.col(J, cb);
                const int m = pc - (int)fdiv((uint32_t)pc, a.fn) * a.n;
                ok0[cb] = m > 0;
                ok2[cb] = m < a.n - 1;
            }
        }
        S::zero(acc2[J]);
        uint4 bh[LA + 1], bl[LA + 1];
        auto bread = [&](int st, uint4& xh, uint4& xl) {
            const int tp = st >> 3, s = st & 7;
            const uint8_t* p = fs.bfrag(XG + (Lc[J][S::scb(s)] + 1 - tp) * RS, S::skb(s));
            xh = lds16(p);
            xl = lds16(p + 256);
        };
#pragma unroll
        for (int q = 0; q < LA; ++q) bread(q, bh[q], bl[q]);
#pragma unroll
        for (int st = 0; st < 24; ++st) {
            const int tp = st >> 3, s = st & 7, cb = S::scb(s), bi = st % (LA + 1);
            uint4 xh = bh[bi], xl = bl[bi];
            if (MASKED && ((tp == 0 && !ok2[cb]) || (tp == 2 && !ok0[cb]))) {
                xh = make_uint4(0, 0, 0, 0);
                xl = xh;
            }
            S::step_first(acc2[J], wd[tp], S::skb(s), cb, xh);
            if (st + LA < 24) bread(st + LA, bh[(st + LA) % (LA + 1)], bl[(st + LA) % (LA + 1)]);
            side(st);
            S::step_rest(acc2[J], wd[tp], S::skb(s), cb, xh, xl);
        }
    };

    // ---- epilogue unit (J, g) of tile et in three parts: residual read; out -> HBM; max
    //      (channels ch0 + S::choff(g) .. + 3 of the lane's column of column block S::cb(g)) ----
    float omax = 0.f, inv2p = 0.f;
    float* dst[S::NCB] = {};
    rsrc_t rs_o;            // unmasked layouts: the stores through a resource at the tile's base time
    uint32_t colo[2][S::NCB];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int cb = 0; cb < S::NCB; ++cb) colo[j][cb] = (uint32_t)((toff[j][cb] * C + ch0) * 4);
    uint32_t ocol[S::NCB] = {};
    float4 oe, oo;
    float sk0 = 0.f, sk1 = 0.f, sk2 = 0.f;   // SX: the lane's dot products over its channels of a column
    size_t sxo[S::NCB] = {};                 // SX: spart float index of (column, wave)
    auto epi_begin = [&](const Tile& et_, int J) {
        const Tile et = memt(et_);
#pragma unroll
        for (int cb = 0; cb < S::NCB; ++cb) {
            const int c = fs.col(J, cb);
            if (SX) sxo[cb] = (((size_t)et.b * a.T + ctime(et, c, toff[J][cb])) * 4 + w) * 4;
            else if (MASKED) dst[cb] = a.gout + ((size_t)et.b * a.T + ctime(et, c, toff[J][cb])) * C + ch0;
            else ocol[cb] = colo[J][cb];
        }
        if (!SX && !MASKED) rs_o = mk_rsrc(a.gout + ((size_t)et.b * a.T + et.tb) * C);
    };
    auto epi_part = [&](int J, int g, int part, const uint8_t* er, const uint32_t (&mw)[S::NCB], float inv2) {
        const int rb = g & (UR - 1), cb = S::cb(g), ch = ch0 + CHR * rb, mg = mg0 + MGR * rb;
        if (part == 0) {
            oe = *reinterpret_cast<const float4*>(er + Lc[J][cb] * RS + 4 * ch);
        } else if (part == 1) {
            const f32x4 au = S::unit(acc2[J], g);
            oo.x = fmaf(keep_if(au[0], mw[cb], mg), inv2, oe.x);
            oo.y = fmaf(keep_if(au[1], mw[cb], 4 + mg), inv2, oe.y);
            oo.z = fmaf(keep_if(au[2], mw[cb], 8 + mg), inv2, oe.z);
            oo.w = fmaf(keep_if(au[3], mw[cb], 12 + mg), inv2, oe.w);
            if (SX) {
                const float4 q0 = *reinterpret_cast<const float4*>(&W0S[ch]);
                const float4 q1 = *reinterpret_cast<const float4*>(&W0S[C + ch]);
                const float4 q2 = *reinterpret_cast<const float4*>(&W0S[2 * C + ch]);
                sk0 = fmaf(q0.w, oo.w, fmaf(q0.z, oo.z, fmaf(q0.y, oo.y, fmaf(q0.x, oo.x, sk0))));
                sk1 = fmaf(q1.w, oo.w, fmaf(q1.z, oo.z, fmaf(q1.y, oo.y, fmaf(q1.x, oo.x, sk1))));
                sk2 = fmaf(q2.w, oo.w, fmaf(q2.z, oo.z, fmaf(q2.y, oo.y, fmaf(q2.x, oo.x, sk2))));
            } else if (MASKED) *reinterpret_cast<float4*>(dst[cb] + CHR * rb) = oo;
            else bst4(rs_o, ocol[cb] + 4 * CHR * rb, 0u, oo);
        } else {
            omax = fmaxf(omax, fmaxf(fmaxf(fabsf(oo.x), fabsf(oo.y)), fmaxf(fabsf(oo.z), fabsf(oo.w))));
            if (SX && rb == UR - 1) {   // the column's channels of this lane done: + the other lanes' of the column -> spart
                fs.col_sum(sk0, sk1, sk2);
                if (fs.lk == 0)
                    *reinterpret_cast<float4*>(a.spart + sxo[cb]) = make_float4(sk0, sk1, sk2, 0.f);
                sk0 = sk1 = sk2 = 0.f;
            }
        }
    };
    auto epi_max = [&](int b) {
        const uint32_t m = wave_max_bits(omax);
        if (lane == 0) atomicMax(gslot(a.gmax_out, b, blockIdx.x), m);
        omax = 0.f;
    };
    using J0 = std::integral_constant<int, 0>;
    using J1 = std::integral_constant<int, 1>;
    using J2 = std::integral_constant<int, 2>;

    if (blockIdx.x >= ntiles) return;   // (grid = min(tiles, CUs): not taken)

    // prologue: the first tile's image, residual rows and masks; the second tile's rows in flight
    float gm_c;     // max |tot| of the current tile's clip (one scalar load per tile: the next one's)
    {
        const Tile t0 = tile_of(blockIdx.x);
        set_rs(t0);
#pragma unroll
        for (int k = 0; k < NU; ++k) load_unit(t0, k);
        load_masks(t0, mu_c, muh_c, me_c);
        const uint32_t z0 = zbits(t0);
        gm_c = sload_gmax(a.gmax_in, t0.b);
        const float s0 = exp2i(scale_exp(gm_c));
#pragma unroll
        for (int k = 0; k < NU; ++k) conv_unit(k, &ER[0][0], s0, z0);
        const Tile t1 = tile_of(clampt(blockIdx.x + G));
        set_rs(t1);
#pragma unroll
        for (int k = 0; k < NU; ++k) load_unit(t1, k);
    }

    Tile prv = tile_of(blockIdx.x);
    STAMP(14)
    auto tile_body = [&](auto first_tag, int tile, int it) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const Tile cu = tile_of(tile);
        const Tile nt = tile_of(clampt(tile + G));
        const Tile n2 = tile_of(clampt(tile + 2 * G));
        set_rs(n2);   // (the previous ones' loads are all issued: units reload right after conversion)
        // T: this tile's tot image complete (converted during the previous phase C)
        lds_barrier();
        STAMP(6)
        const float gm = gm_c;
        const int m_t = scale_exp(gm);
        const int m_u = scale_exp(a.wrn * gm);
        const float f_u = exp2i(m_u - m_t - a.kr);   // acc units 2^(m_t + k_r) -> g_u 2^m_u
        const float inv2 = exp2i(-(m_u + a.kd));
        if (nt.b != cu.b) gm_c = sload_gmax(a.gmax_in, nt.b);   // (usually the same clip: tile order)
        const float s_next = exp2i(scale_exp(gm_c));
        const uint32_t zn = zbits(nt);
        uint8_t* erc = &ER[it & 1][0];          // this tile's residual
        uint8_t* ero = &ER[(it & 1) ^ 1][0];    // the previous tile's, then the next tile's

        // rows 0 / 1 from the previous tile's rows 64 / 65 when it is the left neighbour (every
        // wave its channel quarter; the previous tile's g_a reads are behind the T barrier, this
        // tile's first writes to rows 64 / 65 come in B)
        // (CARRY: the previous sub-sequence's last tile left row 65 zero and the first position's
        // g_u in row 67: rows 0 / 1 = 0 / row 67)
        const bool cont = HALO && !FIRST && prv.b == cu.b && prv.p0 + TMS == cu.p0 && (MASKED || CARRY || cu.m0 != 0);
        const bool fos = CARRY && cu.m0 == 0;
        const bool cry = carry_of(cu);
        // column 63: the last lane column of half 1's last column block
        Lv1t[S::NCB - 1] = cry && fs.col(1, S::NCB - 1) == TMS - 1 ? GROWS - 1 : Lv[1][S::NCB - 1];
        const int cpo = ((lane >> 2) & 1) * 256 + 64 * w + 16 * (lane & 3);   // (side work of A)
        const int csr = fos ? ((lane >> 3) ? GROWS - 1 : TMS) : TMS + (lane >> 3);
        uint4 cpv = make_uint4(0, 0, 0, 0);
        STAMP(11)
        // A: g_v half 0 + epilogue half 1 of the previous tile (parts 0..7)
        if (!FIRST) epi_begin(prv, 1);
        gemm1(J0{}, [&](int kb) {
            if (!FIRST) epi_part(1, kb / 3, kb % 3, ero, me_p, inv2p);
            if (cont && lane < 16) {   // rows 64 / 65 -> 0 / 1, read one step before the write
                if (kb == 0) {
                    cpv = lds16(XG + csr * RS + cpo);
                    if (fos && lane < 8) cpv = make_uint4(0, 0, 0, 0);
                }
                if (kb == 1) *reinterpret_cast<uint4*>(XG + (lane >> 3) * RS + cpo) = cpv;
            }
            // a CARRY tile's row 65 is SAME padding for its own g_a (after the copy's read)
            if (cry && lane < 8 && kb == 2) *reinterpret_cast<uint4*>(XG + (TMS + 1) * RS + cpo) = make_uint4(0, 0, 0, 0);
        });
        // B: g_v half 1 + the epilogue's parts 8..11 + g_u of half 0
        gemm1(J1{}, [&](int kb) {
            if (!FIRST && kb < 4) epi_part(1, (kb + 8) / 3, (kb + 8) % 3, ero, me_p, inv2p);
            gu_part(0, kb >> 1, kb & 1, f_u);
        });
        // max |out| of clip prv.b -> gmax_out once per run of tiles of one clip (omax runs on:
        // with the clip-interleaved tile order a workgroup usually keeps its clip)
        if (!FIRST && cu.b != prv.b) epi_max(prv.b);
        if (HALO && !cont) {
            // H: g_v of rows 0 / 1 + g_u of half 1; then g_u of rows 0 / 1
            gemm1(J2{}, [&](int kb) { gu_part(1, kb >> 1, kb & 1, f_u); });
#pragma unroll
            for (int q = 0; q < 8 / S::NCB; ++q) gu_part(2, q >> 1, q & 1, f_u);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) gu_part(1, q >> 1, q & 1, f_u);
        }
        lds_barrier();   // g_u image complete; every wave is done with the tot image
        STAMP(7)
        // C: g_a half 0 + conversion of tile i+1, each unit's registers reloaded with tile i+2
        //    right away (a tile of latency before the next conversion: issued later, the loads'
        //    latency shows)
        gemm2(J0{}, [&](int st) {
            // unit k at step 24 k / 9 (0 2 5 8 10 13 16 18 21): spread over the phase
#pragma unroll
            for (int k = 0; k < NU; ++k)
                if (st == (24 * k) / NU) {
                    conv_unit(k, ero, s_next, zn);
                    load_unit(n2, k);
                }
            if (st == 3) load_masks(nt, mu_n, muh_n, me_n);
        }, cu);
        STAMP(8)
        // D: g_a half 1 + epilogue half 0 of this tile
        epi_begin(cu, 0);
        gemm2(J1{}, [&](int st) { if (st < 12) epi_part(0, st / 3, st % 3, erc, me_c[0], inv2); }, cu);
        STAMP(9)
        prv = cu;
        inv2p = inv2;
#pragma unroll
        for (int cb = 0; cb < S::NCB; ++cb) {
            me_p[cb] = me_c[1][cb];
            me_c[0][cb] = me_n[0][cb]; me_c[1][cb] = me_n[1][cb];
            mu_c[0][cb] = mu_n[0][cb]; mu_c[1][cb] = mu_n[1][cb];
        }
        muh_c = muh_n;
    };
    tile_body(std::true_type{}, (int)blockIdx.x, 0);
    int it = 1;
    for (int tile = (int)blockIdx.x + G; tile < ntiles; tile += G, ++it)
        tile_body(std::false_type{}, tile, it);
    // drain: epilogue half 1 of the last tile
    {
        const uint8_t* erl = &ER[(it - 1) & 1][0];
        epi_begin(prv, 1);
#pragma unroll
        for (int q = 0; q < 12; ++q) epi_part(1, q / 3, q % 3, erl, me_p, inv2p);
        wg_max_flush(WMX, wave_max_bits(omax), gslot(a.gmax_out, prv.b, blockIdx.x));
    }
    STAMP(12)
    STAMP_FLUSH(a.stamps)
}
