// Host-side packing of a block's 128 x 128 conv weights into the MFMA A-fragment arrays that the
// bf16 and split-fp16 block kernels read (ast_set_weight packs, the kernels' FwdArgsC / BwdArgsC /
// FwdArgsS / BwdArgsS pointers read).  Host only, no HIP includes: tests/test_pack_cpu.py rebuilds
// every array from the formulas below and compares bytes.
//
// A block has W_d [3 taps][ci][co] and W_r [ci][co] (HWIO, as the checkpoint stores them).  A
// fragment array is a sequence of slots of [64 lanes][8 elements]; the forward kernels take
// K = the input channel (element W[kk][mm]), the backward kernels K = the output channel (element
// W[mm][kk]), mm being the fragment's row.  With kb the slot's index within its 8, and (kk, mm)
// of lane `lane`, element e, row group w given by frag_index:
//   32x32x16 fragments:  kk = 16 kb + 8 (lane >> 5) + e          mm = 32 w + (lane & 31)
//   16x16x32 fragments:  kk = 32 (kb >> 1) + 8 (lane >> 4) + e   mm = 32 w + 16 (kb & 1) + (lane & 15)
//   (16x16x32: slot kb = 2 K-block + row block, split-fp16 only; ASTYLE_MFMA16 picks the form per
//   direction, api.hip)
//
// bf16 (precision 1), u16 elements, one value per element (round to nearest even), 32x32x16 only:
//   WFB   [3 tap][4 w][8 kb][64][8]   W_d[tap][kk][mm]
//   WRFB  [4 w][8 kb][64][8]          W_r[kperm(kb, lane >> 5, e)][mm]: K in the order in which the
//                                     forward kernel's W_d accumulators hold its channels
//   WBFB  [3 tap][4 w][8 kb][64][8]   W_d[tap][mm][kk]
//   WRBFB [4 w][8 kb][64][8]          W_r[mm][kk]
// split fp16 (precision 2), in uint4 units (8 fp16), two halves hl per slot: with k = weight_exp of
// the whole tensor (max |W| 2^k in [2^13, 2^14)), hl = 0 holds hi = fp16(W 2^k) (round to nearest),
// hl = 1 holds lo = fp16(W 2^k - hi), the fp32 difference rounded:
//   SWDF [4 w][3 tap][8 kb][2 hl][64]   W_d[tap][kk][mm]        SWRF [4 w][8 kb][2 hl][64]   W_r[kk][mm]
//   SWDB [4 w][3 tap][8 kb][2 hl][64]   W_d[tap][mm][kk]        SWRB [4 w][8 kb][2 hl][64]   W_r[mm][kk]
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>

namespace ast {

constexpr int WC = 128;   // channels (common.h: C)
// offsets inside one block's fragments: bf16 in u16 elements, split in uint4 units
constexpr size_t WFB = 0, WRFB = 3 * WC * WC, WBFB = 4 * WC * WC, WRBFB = 7 * WC * WC, BLKB_SZ = 8 * WC * WC;
constexpr size_t SWDF = 0, SWRF = 4 * 3 * 8 * 2 * 64, SWRB = SWRF + 4 * 8 * 2 * 64,
                 SWDB = SWRB + 4 * 8 * 2 * 64, SBLK = SWDB + 4 * 3 * 8 * 2 * 64;

inline int kperm(int s, int h, int e) { return 32 * (s >> 1) + 16 * (s & 1) + (e & 3) + 8 * (e >> 2) + 4 * h; }

// (K index kk, row index mm) of element e of lane ln in slot kb of row group w
inline void frag_index(bool m16, int kb, int ln, int e, int w, int& kk, int& mm) {
    if (m16) {
        kk = 32 * (kb >> 1) + 8 * (ln >> 4) + e;
        mm = 32 * w + 16 * (kb & 1) + (ln & 15);
    } else {
        kk = 16 * kb + 8 * (ln >> 5) + e;
        mm = 32 * w + (ln & 31);
    }
}

// power-of-two exponent k that puts max |w| 2^k in [2^13, 2^14) (fp16 range, splitwave.h)
inline int weight_exp(const float* w, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(w[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 0;
    int e = 0;
    (void)std::frexp(mx, &e);
    return 14 - e;
}
// fp16 halves of w 2^k (round to nearest): hi, lo = fp16(w 2^k - hi)
inline void split_half(float w, int k, uint16_t& hi, uint16_t& lo) {
    const float v = std::ldexp(w, k);
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    memcpy(&hi, &h, 2);
    memcpy(&lo, &l, 2);
}
inline uint16_t host_bf16(float f) {   // round to nearest even
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// W [taps][WC][WC] at (tap, K index kk, row mm) of a forward (W[kk][mm]) or backward (W[mm][kk]) fragment
inline float frag_elem(const float* W, int tap, bool bwd, int kk, int mm) {
    return W[(size_t)tap * WC * WC + (bwd ? mm * WC + kk : kk * WC + mm)];
}

// split-fp16 fragments of W [taps][WC][WC] (3: W_d, 1: W_r) -> out [4 w][taps][8 kb][2 hl][64][8]
// fp16 (taps * WC * WC * 2 elements); returns the exponent k
inline int pack_split(const float* W, int taps, bool bwd, bool m16, uint16_t* out) {
    const int k = weight_exp(W, (size_t)taps * WC * WC);
    for (int w = 0; w < 4; ++w)
        for (int tp = 0; tp < taps; ++tp)
            for (int kb = 0; kb < 8; ++kb)
                for (int ln = 0; ln < 64; ++ln)
                    for (int e = 0; e < 8; ++e) {
                        int kk, mm;
                        frag_index(m16, kb, ln, e, w, kk, mm);
                        const size_t o = ((((size_t)(w * taps + tp) * 8 + kb) * 2) * 64 + ln) * 8 + e;
                        split_half(frag_elem(W, tp, bwd, kk, mm), k, out[o], out[o + 64 * 8]);
                    }
    return k;
}

// bf16 fragments of W [taps][WC][WC] -> out [taps][4 w][8 kb][64][8] (taps * WC * WC elements).
// The one special case: the forward W_r fragments (taps == 1) take K in kperm order
inline void pack_bf16(const float* W, int taps, bool bwd, uint16_t* out) {
    for (int tp = 0; tp < taps; ++tp)
        for (int w = 0; w < 4; ++w)
            for (int kb = 0; kb < 8; ++kb)
                for (int ln = 0; ln < 64; ++ln)
                    for (int e = 0; e < 8; ++e) {
                        int kk, mm;
                        frag_index(false, kb, ln, e, w, kk, mm);
                        if (taps == 1 && !bwd) kk = kperm(kb, ln >> 5, e);
                        out[((((size_t)tp * 4 + w) * 8 + kb) * 64 + ln) * 8 + e] = host_bf16(frag_elem(W, tp, bwd, kk, mm));
                    }
}

// operand bounds of the split kernels' range checks (splitwave.h), W [rows][WC]:
// wdn = max_co sum_{tap, ci} |W_d| (rows = 3 WC): |W_d e| <= wdn max |e|
inline float col_abs_sum_max(const float* W, int rows) {
    float nrm = 0.f;
    for (int co = 0; co < WC; ++co) {
        float s = 0.f;
        for (int i = 0; i < rows; ++i) s += std::fabs(W[(size_t)i * WC + co]);
        nrm = std::max(nrm, s);
    }
    return nrm;
}
// wrn = max_ci sum_co |W_r|: |W_r tot| <= wrn max |tot| (the backward's product)
inline float row_abs_sum_max(const float* W, int rows) {
    float nrm = 0.f;
    for (int ci = 0; ci < rows; ++ci) {
        float s = 0.f;
        for (int co = 0; co < WC; ++co) s += std::fabs(W[(size_t)ci * WC + co]);
        nrm = std::max(nrm, s);
    }
    return nrm;
}
// bdm = max |b_d|
inline float abs_max(const float* v, int n) {
    float m = 0.f;
    for (int i = 0; i < n; ++i) m = std::max(m, std::fabs(v[i]));
    return m;
}

}  // namespace ast
