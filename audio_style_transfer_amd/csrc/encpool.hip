// The NSynth encoding (model.py:121-128 `ae_pool`; fastgen.py:86-113 `encode`): the 16-channel
// bottleneck averaged over 512-sample hops, R = T / 512 rows per clip,
//
//   enc[b, r, j] = (1/512) sum_{t = 512 r .. 512 r + 511} (sum_c e_30[b, t, c] W_b[c, j] + b_b[j])
//
// and the optional loss term enc_term_b = omega mean_{r, j} (enc[b, r, j] - phi_e[b, r, j])^2.
// pool1d with window = stride = 512 and T % 512 == 0 pads nothing: a plain mean.  Pooling before
// the 1x1 is the same linear map, so the kernel reduces 512 rows to 128 channel means first; the
// operation order below is the definition of the result.  fp32 whatever the precision mode.
//
// k_encpool_fwd: one 256-thread workgroup per (clip, hop) streams the hop's 512 x 128 tile of
// e_30 once with 16-byte loads (a wave instruction covers whole rows: 2 fp32 rows, 4 bf16 rows).
// A thread owns one 16-byte column group and every NG-th row (NG = 8 fp32, 16 bf16), summed in
// row order; the NG row-group sums per channel meet in LDS and are added in group (= wave)
// order; 16 threads form the outputs from the 128 channel means in channel order, then add the
// bias.  With a target, d = enc - phi_e goes to dbuf and the hop's squared error, summed in j
// order, to epart[b][r].
// k_encpool_bwd: per (clip, hop) v[c] = coef sum_j W_b[c, j] d[b, r, j] (j in order), stored to
// (or added into) all 512 rows of tensor 30's content-gradient buffer with the same 16-byte
// accesses; coef = 2 omega / (16 R 512).
// k_encpool_loss: per clip, epart[b][0..R) in hop order, times omega / (16 R) -> enc_loss[b],
// added to parts[b][0].  No atomics anywhere: a clip's encoding, term and gradient do not depend
// on its batch slot, the batch size or the run.
#include "common.h"

namespace ast {
namespace {

constexpr int HOP = 512;      // ae_hop_length (model.py:24)
constexpr int NJ = 16;        // ae_bottleneck_width (model.py:23)

template <typename S> struct Vec;
template <> struct Vec<float> {
    static constexpr int N = 4;
    __device__ static void load(const float* p, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    __device__ static void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Vec<u16> {
    static constexpr int N = 8;
    __device__ static void load(const u16* p, float (&v)[8]) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = bflo(q.x); v[1] = bfhi(q.x); v[2] = bflo(q.y); v[3] = bfhi(q.y);
        v[4] = bflo(q.z); v[5] = bfhi(q.z); v[6] = bflo(q.w); v[7] = bfhi(q.w);
    }
    __device__ static void store(u16* p, const float (&v)[8]) {
        *reinterpret_cast<uint4*>(p) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]),
                                                  pack2(v[4], v[5]), pack2(v[6], v[7]));
    }
};

template <typename S>
__global__ void __launch_bounds__(256) k_encpool_fwd(const S* __restrict__ e,
                                                     const float* __restrict__ wb,
                                                     const float* __restrict__ bb,
                                                     const float* __restrict__ phi,
                                                     size_t phi_bstride, float* __restrict__ enc,
                                                     float* __restrict__ dbuf,
                                                     float* __restrict__ epart, int T) {
    constexpr int N = Vec<S>::N, NQ = C / N, NG = 256 / NQ, ROWS = HOP / NG;
    __shared__ float red[NG][C];
    __shared__ float mean[C];
    __shared__ float sq[NJ];
    const int j = threadIdx.x;
    const int R = T / HOP, b = blockIdx.x / R, r = blockIdx.x % R;
    const int q = j % NQ, g = j / NQ;
    const S* p = e + ((size_t)b * T + (size_t)r * HOP + g) * C + q * N;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    for (int i = 0; i < ROWS; i += 8) {       // 8 loads in flight, added in row order
        float v[8][N];
#pragma unroll
        for (int u = 0; u < 8; ++u) Vec<S>::load(p + (size_t)(i + u) * NG * C, v[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] += v[u][k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) red[g][q * N + k] = acc[k];
    __syncthreads();
    if (j < C) {
        float s = red[0][j];
#pragma unroll
        for (int k = 1; k < NG; ++k) s += red[k][j];
        mean[j] = s * (1.0f / HOP);
    }
    __syncthreads();
    if (j < NJ) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(mean[c], wb[c * NJ + j], s);
        s += bb[j];
        const size_t o = ((size_t)b * R + r) * NJ + j;
        enc[o] = s;
        if (phi) {
            const float d = s - phi[(size_t)b * phi_bstride + (size_t)r * NJ + j];
            dbuf[o] = d;
            sq[j] = d * d;
        }
    }
    if (!phi) return;
    __syncthreads();
    if (j == 0) {
        float s = sq[0];
#pragma unroll
        for (int k = 1; k < NJ; ++k) s += sq[k];
        epart[(size_t)b * R + r] = s;
    }
}

template <typename S>
__global__ void __launch_bounds__(256) k_encpool_bwd(const float* __restrict__ dbuf,
                                                     const float* __restrict__ wb,
                                                     S* __restrict__ cg, float coef,
                                                     int accumulate, int T) {
    constexpr int N = Vec<S>::N, NQ = C / N, NG = 256 / NQ, ROWS = HOP / NG;
    __shared__ float vs[C];
    const int j = threadIdx.x;
    const int R = T / HOP, b = blockIdx.x / R, r = blockIdx.x % R;
    if (j < C) {
        const float* d = dbuf + ((size_t)b * R + r) * NJ;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NJ; ++k) s = fmaf(wb[j * NJ + k], d[k], s);
        vs[j] = coef * s;
    }
    __syncthreads();
    const int q = j % NQ, g = j / NQ;
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = vs[q * N + k];
    S* p = cg + ((size_t)b * T + (size_t)r * HOP + g) * C + q * N;
    if (!accumulate) {
        for (int i = 0; i < ROWS; ++i) Vec<S>::store(p + (size_t)i * NG * C, v);
        return;
    }
    for (int i = 0; i < ROWS; i += 4) {
        float o[4][N];
#pragma unroll
        for (int u = 0; u < 4; ++u) Vec<S>::load(p + (size_t)(i + u) * NG * C, o[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int k = 0; k < N; ++k) o[u][k] += v[k];
            Vec<S>::store(p + (size_t)(i + u) * NG * C, o[u]);
        }
    }
}

__global__ void __launch_bounds__(64) k_encpool_loss(const float* __restrict__ epart,
                                                     float* __restrict__ eloss,
                                                     float* __restrict__ parts, float scale,
                                                     int R, int B) {
#pragma clang fp contract(off)   // parts gets the stored value added, not an fma of its factors
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += epart[(size_t)b * R + r];
    const float v = s * scale;
    eloss[b] = v;
    parts[b * 4 + 0] += v;
}

}  // namespace

template <typename S>
void launch_encpool_fwd(const S* e30, const float* wb, const float* bb, const float* phi,
                        size_t phi_bstride, float* enc, float* dbuf, float* epart, int B, int T,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_encpool_fwd<S>, dim3((unsigned)(T / HOP) * B), dim3(256), 0, s, e30, wb, bb, phi,
                       phi_bstride, enc, dbuf, epart, T);
}
template <typename S>
void launch_encpool_bwd(const float* dbuf, const float* wb, S* cg30, float omega, int accumulate,
                        int B, int T, hipStream_t s) {
    const float coef = 2.0f * omega / ((float)NJ * (float)(T / HOP) * (float)HOP);
    hipLaunchKernelGGL(k_encpool_bwd<S>, dim3((unsigned)(T / HOP) * B), dim3(256), 0, s, dbuf, wb, cg30, coef,
                       accumulate, T);
}
void launch_encpool_loss(const float* epart, float* eloss, float* parts, float omega, int B, int T,
                         hipStream_t s) {
    const int R = T / HOP;
    hipLaunchKernelGGL(k_encpool_loss, dim3((B + 63) / 64), dim3(64), 0, s, epart, eloss, parts,
                       omega / ((float)NJ * (float)R), R, B);
}
template void launch_encpool_fwd<float>(const float*, const float*, const float*, const float*, size_t, float*, float*, float*, int, int, hipStream_t);
template void launch_encpool_fwd<u16>(const u16*, const float*, const float*, const float*, size_t, float*, float*, float*, int, int, hipStream_t);
template void launch_encpool_bwd<float>(const float*, const float*, float*, float, int, int, int, hipStream_t);
template void launch_encpool_bwd<u16>(const float*, const float*, u16*, float, int, int, int, hipStream_t);

}  // namespace ast
