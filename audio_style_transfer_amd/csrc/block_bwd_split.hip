// Split-fp16 encoder block backward (precision 2): d loss / d e_l for one block of
// model.py:95-116, restated by oracle/astyle_oracle.py:171-189 (encoder_backward):
//   tot = d loss / d e_{l+1} (the chain, its own direct loss term included)
//   g_u = [u > 0] (W_r tot)                         1x1 conv transposed
//   g_a = sum_k W_d[k] g_u(p - k + 1)                K = 3 SAME dilated conv transposed, in
//                                                    time_to_batch positions (masked.py:110-160)
//   out = tot + D_l + [e_l > 0] g_a                  D_l: direct loss gradient of e_l, if tapped
// fp32 storage, MFMA on split fp16 operands, fp32 accumulation and epilogue (splitwave.h).
// One kernel body (block_bwd_split_body.h) in two MFMA forms (splitwave.h Frag32 / Frag16):
//   k_block_bwd_s16  v_mfma_f32_16x16x32_f16: the shipped backward (ASTYLE_MFMA16=2, the default,
//                    and 1; the weights are packed for it then)
//   k_block_bwd_s    v_mfma_f32_32x32x16_f16 (ASTYLE_MFMA16=0, 3): the K accumulation order
//                    differs, so results match the other form to fp32 rounding, not bit for bit;
//                    0.3-1.2 % slower per launch (round 6)
//
// One workgroup per CU (wave w owns channels 32 w .. 32 w + 31), persistent over tiles of 64
// positions, one wave per SIMD; the structure of the forward (block_fwd_split.hip): a tile's
// tot and D_l rows arrive in registers a tile ahead in row units (8 cache lines per wave
// instruction) and are converted during the previous tile's second GEMM into the split tot
// image and the wave's quarter of a residual buffer (tot + D_l in fp32, double-buffered, read
// back by the same wave); the relu-mask words come by plain loads.  Per tile i:
//   T  barrier (tot image i complete)
//   A  g_v = W_r tot, column half 0 (8 k-steps x 3 products); carries epilogue half 1 of tile
//      i-1 (out = residual + [e_l > 0] g_a 2^-(m_u+k_d) -> HBM)
//   B  g_v column half 1; carries the rest of that epilogue and g_u of half 0 (mask, scale
//      2^m_u from the bound |g_v| <= wrn max|tot|, split -> g_u image)
//   H  (one-segment layouts, unless the workgroup's previous tile is the left neighbour: then
//      its g_u rows 64 / 65 are copied to rows 0 / 1) g_v of rows 0 / 1 (positions p0 - 1, p0;
//      the column tiles cover p0 + 1 .. p0 + 64); carries g_u of half 1; g_u of the last column
//      tile; barrier (g_u image complete, tot image free).  The left neighbour includes the
//      last tile of the previous sub-sequence (CARRY): that tile's right-halo column (p0 + 64,
//      SAME padding for its own g_a) is computed on the next sub-sequence's first position
//      instead of a zero row and set aside in g_u row 67, so the next tile's rows 0 / 1 are
//      (0, row 67) and no tile of a walk pays the halo MFMAs but its first
//   C  g_a, column half 0 (3 taps x 8 k-steps x 3 products over the g_u image); carries the
//      conversion of tile i+1 and, unit by unit behind it, the row loads of tile i+2
//   D  g_a, column half 1; carries epilogue half 0 of tile i
// The first tile is peeled so every loop iteration issues the same vector-memory sequence.
// non-temporal (nt) row loads; the stores keep the default policy: they leave the accumulator
// layout as 16-B pieces of 32 lines per instruction, which L2 merges into whole lines, and nt made
// them partial-line writes to DRAM (+75 % per launch, profiles/r6_diag/block_ab.txt)
#ifndef SW_BWD_DEFAULT_POLICY
#define SW_LD_AUX 2
#endif
#include "splitwave.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace ast {
namespace {
using namespace sw;

constexpr int IROWS = 72;             // tot image / residual rows (9 units x 8)
constexpr int ISLOT = IROWS * RS;
constexpr int GROWS = 68;             // g_u image rows (66 / 68 used; 66 takes unused halo writes)
constexpr int LA = 2;                 // B-fragment lookahead (steps)

#define SW_KERNEL k_block_bwd_s
#define SW_FRAG Frag32
#include "block_bwd_split_body.h"
#undef SW_KERNEL
#undef SW_FRAG
#define SW_KERNEL k_block_bwd_s16
#define SW_FRAG Frag16
#include "block_bwd_split_body.h"
#undef SW_KERNEL
#undef SW_FRAG

// max |x| over each clip's n elements -> out[b] (atomic max of the float bits)
__global__ void __launch_bounds__(256) k_absmax(const float* __restrict__ x, size_t n, int chunks,
                                                unsigned* __restrict__ out) {
    const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
    const size_t len = n / chunks;
    const float4* p = reinterpret_cast<const float4*>(x + (size_t)b * n + (size_t)ch * len);
    float m = 0.f;
    for (size_t i = threadIdx.x; i < len / 4; i += 256) {
        const float4 v = p[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(gslot(out, b, blockIdx.x), __float_as_uint(m));
}

template <class S, bool MASKED, bool ONESEG, bool HAS_D, bool SX, bool WHOLE>
void launch_as(dim3 grid, hipStream_t s, const BwdArgsS& a, const Layout& ly) {
    if constexpr (std::is_same_v<S, Frag32>) hipLaunchKernelGGL((k_block_bwd_s<MASKED, ONESEG, HAS_D, SX, WHOLE>), grid, dim3(FT), 0, s, a, ly);
    else hipLaunchKernelGGL((k_block_bwd_s16<MASKED, ONESEG, HAS_D, SX, WHOLE>), grid, dim3(FT), 0, s, a, ly);
}

template <class S>
void launch_bwd(const BwdArgsS& a0, hipStream_t s) {
    BwdArgsS a = a0;
    a.fn = make_fdiv((uint32_t)a.n);
    a.ft = make_fdiv((uint32_t)(SW_TILE_INTERLEAVE ? a.B : a.T / TMS));
    const int nt = a.B * (a.T / TMS);
    const dim3 grid(std::min(nt, a.cus > 0 ? std::min(a.cus, sw::num_cus()) : sw::num_cus()));
    Layout ly;
    const bool masked = pick_layout(a.n, ly);
    const bool oneseg = !masked && ly.M == TMS;
    if (a.spart && (!oneseg || a.dadd || a.d != 1)) { fprintf(stderr, "block_bwd_s: spart needs d = 1, no D\n"); abort(); }
    const bool whole = oneseg && a.n == TMS;
#define BWD_LAUNCH(M, O, D, X, W) launch_as<S, M, O, D, X, W>(grid, s, a, ly)
    if (masked) { if (a.dadd) BWD_LAUNCH(true, false, true, false, false); else BWD_LAUNCH(true, false, false, false, false); }
    else if (whole && !a.spart) {
        if (a.dadd) BWD_LAUNCH(false, true, true, false, true); else BWD_LAUNCH(false, true, false, false, true);
    } else if (oneseg) {
        if (a.dadd) BWD_LAUNCH(false, true, true, false, false);
        else if (a.spart) BWD_LAUNCH(false, true, false, true, false);
        else BWD_LAUNCH(false, true, false, false, false);
    } else { if (a.dadd) BWD_LAUNCH(false, false, true, false, false); else BWD_LAUNCH(false, false, false, false, false); }
#undef BWD_LAUNCH
}

}  // namespace

void launch_block_bwd_s(const BwdArgsS& a, hipStream_t s) { launch_bwd<Frag32>(a, s); }
void launch_block_bwd_s16(const BwdArgsS& a, hipStream_t s) { launch_bwd<Frag16>(a, s); }

void launch_absmax(const float* x, size_t per_clip, int B, unsigned* out, hipStream_t s) {
    int chunks = 1;
    while (chunks < 64 && per_clip % ((size_t)chunks * 8) == 0 && per_clip / (chunks * 2) >= 4096) chunks *= 2;
    hipLaunchKernelGGL(k_absmax, dim3(B * chunks), dim3(256), 0, s, x, per_clip, chunks, out);
}

}  // namespace ast
