// The ours-Gram forward kernels' body (gram_split.hip includes this file inside each of its four
// forward kernels, which name: A, the arithmetic (GramSplit / GramF32); NCH, channels per
// workgroup; NRING, fills of loads in flight).  The body stays inside the __global__ function:
// called as a function from a wrapper it compiles to other code (the callee is simplified on its
// own before it is inlined).
//
// NCH = 32 is the wide geometry, one wave per 4 channels; 8 and 4 are the narrow ones for few
// clips, one wave per channel: a clip's chunk spreads over 16 or 32 workgroups instead of 4.  A
// fill is the rows staged between two barrier pairs: one 16-row stage (wide) or 4 stages (64
// rows, narrow); a wave issues 4 MFMA groups per fill, over its 4 channels (wide) or over the 4
// stages of its one channel (narrow).  Per channel, stage by stage, every geometry issues the
// same MFMAs on the same fragments: a clip's partials are the same bits whichever kernel the
// batch size selects.
// Staging: a thread loads tensor su, channel quad sq, rows 8 g .. + 8 of the fill (one load
// instruction covers 8 whole lines) and writes image rows [(g >> 1) NCH + 4 sq + j][su] at
// 8 (g & 1):
//   NCH = 32: su = 8 (w & 3) + (l & 7), sq = l >> 3,       g = w >> 2
//   NCH = 8:  su = 8 (w & 3) + (l & 7), sq = (l >> 3) & 1, g = (l >> 4) + 4 (w >> 2)
//   NCH = 4:  su = 8 w + (l & 7),       sq = 0,            g = l >> 3   (16-B row pieces)
// NRING fills of loads in flight, a ring of NRING register sets (wide, 3: 192 KiB per workgroup,
// the registers of a third stage fit beside the accumulators at the same two waves per SIMD).
// Every load is unconditional (past the chunk a fill re-reads the chunk's last rows, an L2 hit)
// and the loop runs whole rings, the remainder after it: a conditional load made the compiler
// copy the ring registers (v_mov) behind vmcnt(0) waits, so no fill stayed in flight across a fill
    constexpr bool WIDE = NCH == GCS;
    constexpr int FILL = WIDE ? GSS : GFN, NACC = WIDE ? 4 : 1;
    __shared__ __attribute__((aligned(16))) A::elem I[(FILL / GSS) * NCH * 32 * A::RS];   // [stage][c][u][t]
    // the workgroup's clip, chunk and first channel: decode(), which the narrow kernels have in
    // place for their NCH (through the function they compile to other code, as the wide ones do
    // with it in place)
    int b, ch, c0;
    if constexpr (WIDE) {
        decode(a, b, ch, c0);
    } else {
        constexpr int ncg = C / NCH;
        const int nwg = a.B * a.nchunk * ncg;
        int work = xcd_remap(blockIdx.x, nwg);   // the channel groups of a chunk share one XCD
        const int cgi = work % ncg; work /= ncg;
        ch = work % a.nchunk, b = work / a.nchunk, c0 = cgi * NCH;
    }
    const int tlen = a.T / a.nchunk, tbeg = ch * tlen, tend = tbeg + tlen;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const A::lane_t ln(lane);   // the lane's fragment coordinates
    const int wc = WIDE ? 4 * w : w;   // the wave's first channel
    const int su = NCH == 4 ? 8 * w + (lane & 7) : 8 * (w & 3) + (lane & 7);
    const int sq = WIDE ? lane >> 3 : NCH == 8 ? (lane >> 3) & 1 : 0;
    const int g = WIDE ? w >> 2 : NCH == 8 ? (lane >> 4) + 4 * (w >> 2) : lane >> 3;
    const bool real = su < a.nu;
    const float* src = real ? (const float*)a.act + (size_t)a.uid[su] * a.tstride +
                              (size_t)b * a.T * C + c0 + 4 * sq + (size_t)8 * g * C
                            : (const float*)a.zero16;
    const size_t rs = real ? C : 0;
    A::acc_t acc[NACC];
#pragma unroll
    for (int cc = 0; cc < NACC; ++cc) A::zero(acc[cc]);
    float4 v[NRING][8];
    auto load = [&](float4 (&vv)[8], int t0) {
        const int tr = min(t0, tend - FILL);
#pragma unroll
        for (int k = 0; k < 8; ++k) vv[k] = *reinterpret_cast<const float4*>(src + (size_t)(tr + k) * rs);
    };
    auto fill = [&](float4 (&vv)[8], int t0) {
        A::piece p0[4], p1[4];       // channel 4 sq + j: 8 consecutive rows as two 16-B pieces
        A::cut(vv, p0, p1);
        load(vv, t0 + NRING * FILL);
        __syncthreads();   // the previous fill's MFMA reads are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // stage g >> 1, channel 4 sq + j, tensor su; rows 8 (g & 1) .. of the stage
            A::elem* row = &I[(((WIDE ? 0 : g >> 1) * NCH + 4 * sq + j) * 32 + su) * A::RS + 8 * (WIDE ? g : g & 1)];
            *reinterpret_cast<A::piece*>(row) = p0[j];
            *reinterpret_cast<A::piece*>(row + A::P1) = p1[j];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) {   // wide: channel wc + m of the stage; narrow: stage m of channel wc
            const int st = WIDE ? 0 : m, cc = WIDE ? m : 0;
            const int ro = (st * NCH + wc + cc) * 32;
            const A::elem* row = &I[A::at(ln, ro)];
            const A::piece x0 = *reinterpret_cast<const A::piece*>(row);
            const A::piece x1 = *reinterpret_cast<const A::piece*>(row + A::R1);
            A::mma(x0, x1, acc[cc]);
        }
    };
#pragma unroll
    for (int q = 0; q < NRING; ++q) load(v[q], tbeg + q * FILL);
    const int nf = tlen / FILL, nring = nf / NRING;
    int t0 = tbeg;
    for (int i = 0; i < nring; ++i, t0 += NRING * FILL) {
#pragma unroll
        for (int q = 0; q < NRING; ++q) fill(v[q], t0 + q * FILL);
    }
#pragma unroll
    for (int q = 0; q < NRING - 1; ++q)
        if (q < nf - nring * NRING) fill(v[q], t0 + q * FILL);
#pragma unroll
    for (int cc = 0; cc < NACC; ++cc) {
        float* dst = a.gpart + (((size_t)b * a.nchunk + ch) * C + c0 + wc + cc) * 1024;
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[A::gat(ln, i)] = A::gval(acc[cc], i);
    }
