// Split-fp16 encoder block forward (precision 2): model.py:95-116 for one block,
//   u = dconv_d(relu(e_l)) + b_d        (masked.py:110-160, K = 3, SAME zero padding)
//   e_{l+1} = e_l + W_r^T relu(u) + b_r
// fp32 storage, MFMA on split fp16 operands, fp32 accumulation and fp32 epilogues (splitwave.h).
// One kernel body (block_fwd_split_body.h) in two MFMA forms (splitwave.h Frag32 / Frag16):
//   k_block_fwd_s    v_mfma_f32_32x32x16_f16: the shipped forward (ASTYLE_MFMA16=2, the default,
//                    and 0)
//   k_block_fwd_s16  v_mfma_f32_16x16x32_f16 (ASTYLE_MFMA16=1, 3; the weights are packed for it
//                    then): the K accumulation order differs, so results match the other form to
//                    fp32 rounding, not bit for bit; 4-5 % slower per launch (round 6)
//
// One workgroup per CU (wave w owns output channels 32 w .. 32 w + 31), persistent over tiles
// of 64 positions, one wave per SIMD: every epilogue runs in the shadow of MFMAs.  The two
// 32-column halves j of a tile are separate MFMA phases, so the epilogue of one half overlaps
// the GEMM of the other.  A tile's e_l arrives in registers (rows: unit k = image rows 8 k ..
// 8 k + 7 x wave w's 32 channels, 8 cache lines per wave instruction), loaded during phases A
// and B of the previous tile, and is converted into the LDS image (split relu(e_l), scaled by
// 2^m_e from the clip's max |e_l|) and into the wave's quarter of a residual buffer (fp32 e_l,
// double-buffered, read back by the same wave only).  Per tile i:
//   T  barrier (image i complete)
//   A  GEMM 1, column half 0 (3 taps x 8 k-blocks x 3 products); carries epilogue 2 of tile
//      i-1 (8 units of 3 steps: e_i = e_{i-1} + y + b_r back into the residual rows, e > 0
//      bits, max |e|), the flush of its half 0 (residual rows -> HBM as whole lines) and the
//      row loads of tile i+1, units 0..4
//   B  GEMM 1, column half 1; carries epilogue 1 of half 0 (u = acc 2^-(m_e+k_d) + b_d, u > 0
//      bits, v = relu(u) 2^m_v -> split v image; m_v from the bound |u| <= wdn max|e_l| + bdm),
//      the flush of epilogue 2's half 1 and the row loads of units 5..8; barrier
//   C  GEMM 2 (8 k-blocks x 3 products), half 0; carries epilogue 1 of half 1; barrier
//   D  GEMM 2, half 1; carries the conversion of tile i+1 (image + residual)
// Round-2 measurements of this structure: ~13k cycles per tile against an MFMA
// floor of 6.2k; moving the loads / conversions between phases does not change the tile time.
// non-temporal (gfx950 CPol nt) row loads and e_{l+1} stores: every row streams through once, and
// the stores are whole 128-B lines (round 6: -1.0 % per launch from the stores, -0.4 % from the
// loads, profiles/r6_diag/block_ab.txt); -DSW_FWD_DEFAULT_POLICY (A/B builds) restores the default
#ifndef SW_FWD_DEFAULT_POLICY
#define SW_LD_AUX 2
#define SW_ST_AUX 2
#endif
#include "splitwave.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace ast {
namespace {
using namespace sw;

constexpr int IROWS = 72;             // image / residual rows: 66 or 68 used, 9 units x 8 rows
constexpr int ISLOT = IROWS * RS;     // bytes per image / residual buffer
constexpr int LA = 2;                 // B-fragment lookahead (steps)

#define SW_KERNEL k_block_fwd_s
#define SW_FRAG Frag32
#include "block_fwd_split_body.h"
#undef SW_KERNEL
#undef SW_FRAG
#define SW_KERNEL k_block_fwd_s16
#define SW_FRAG Frag16
#include "block_fwd_split_body.h"
#undef SW_KERNEL
#undef SW_FRAG

template <class S, bool MASKED, bool ONESEG, bool XIN>
void launch_as(dim3 grid, hipStream_t s, const FwdArgsS& a, const Layout& ly) {
    if constexpr (std::is_same_v<S, Frag32>) hipLaunchKernelGGL((k_block_fwd_s<MASKED, ONESEG, XIN>), grid, dim3(FT), 0, s, a, ly);
    else hipLaunchKernelGGL((k_block_fwd_s16<MASKED, ONESEG, XIN>), grid, dim3(FT), 0, s, a, ly);
}

template <class S>
void launch_fwd(const FwdArgsS& a0, hipStream_t s) {
    FwdArgsS a = a0;
    a.fn = make_fdiv((uint32_t)a.n);
    a.ft = make_fdiv((uint32_t)(SW_TILE_INTERLEAVE ? a.B : a.T / TMS));
    const int nt = a.B * (a.T / TMS);
    const dim3 grid(std::min(nt, a.cus > 0 ? std::min(a.cus, sw::num_cus()) : sw::num_cus()));
    Layout ly;
    const bool masked = pick_layout(a.n, ly);
    if (a.xin && (masked || ly.M != TMS || a.d != 1)) { fprintf(stderr, "block_fwd_s: xin needs d = 1\n"); abort(); }
    if (masked) launch_as<S, true, false, false>(grid, s, a, ly);
    else if (ly.M == TMS && a.xin) launch_as<S, false, true, true>(grid, s, a, ly);
    else if (ly.M == TMS) launch_as<S, false, true, false>(grid, s, a, ly);
    else launch_as<S, false, false, false>(grid, s, a, ly);
}

}  // namespace

void launch_block_fwd_s(const FwdArgsS& a, hipStream_t s) { launch_fwd<Frag32>(a, s); }
void launch_block_fwd_s16(const FwdArgsS& a, hipStream_t s) { launch_fwd<Frag16>(a, s); }

int sw::num_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (cus <= 0) cus = 256;
    }
    return cus;
}

}  // namespace ast
