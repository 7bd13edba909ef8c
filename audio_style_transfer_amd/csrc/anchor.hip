// Seam anchor term of the long-form mode (no reference counterpart): per clip b
//
//   anchor_b = mu * sum_t w[b,t] (a(x[b,t]) - ref[b,t])^2 / sum_t w[b,t]      (0 when sum w = 0)
//
// with a = the TF inv_mu_law (mulaw.h), ref in audio units and w >= 0 the caller's buffers, read
// at every evaluation (the caller may overwrite their values in place, also under a captured
// graph, so sum w is part of the evaluation).  fp32 whatever the context precision.
//
// k_anchor_part: one 256-thread workgroup per (clip, 1024-sample chunk) sums w d^2 and w over its
// chunk: four samples per thread, a butterfly over the wave, the four waves in order.
// k_anchor_apply: every workgroup of a clip adds the clip's chunk partials in chunk order (the
// same order in every workgroup and for every batch size, so a clip's value and gradient do not
// depend on its slot or on the batch), then adds 2 mu w (a - ref) a'(x) / sum w to grad; the
// clip's first workgroup adds the value to parts[b][0] and stores it for ast_anchor_loss.
// No atomics.  Samples with w == 0 never read ref.  ~5 x 4 B per sample and pass: HBM bound.
#include "common.h"
#include "mulaw.h"

namespace ast {
namespace {

constexpr int ACH = 1024;      // samples per workgroup

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(256) k_anchor_part(const float* __restrict__ x,
                                                     const float* __restrict__ ref,
                                                     const float* __restrict__ w,
                                                     float* __restrict__ part, int T, int nch) {
    __shared__ float red[4][2];
    const int j = threadIdx.x;
    const int b = blockIdx.y, c = blockIdx.x;
    float sq = 0.f, sw = 0.f;
#pragma unroll
    for (int i = 0; i < ACH / 256; ++i) {
        const int t = c * ACH + j + 256 * i;
        if (t < T) {
            const size_t k = (size_t)b * T + t;
            const float wv = w[k];
            if (wv != 0.f) {
                const float d = inv_mu_law(x[k]) - ref[k];
                sq += wv * d * d;
                sw += wv;
            }
        }
    }
    sq = wave_sum_f(sq);
    sw = wave_sum_f(sw);
    if ((j & 63) == 0) { red[j >> 6][0] = sq; red[j >> 6][1] = sw; }
    __syncthreads();
    if (j < 2) part[((size_t)b * nch + c) * 2 + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
}

__global__ void __launch_bounds__(256) k_anchor_apply(const float* __restrict__ x,
                                                      const float* __restrict__ ref,
                                                      const float* __restrict__ w,
                                                      const float* __restrict__ part,
                                                      float* __restrict__ grad,
                                                      float* __restrict__ parts,
                                                      float* __restrict__ aloss, int T, int nch,
                                                      float mu) {
    __shared__ float tot[2];
    const int j = threadIdx.x;
    const int b = blockIdx.y, c = blockIdx.x;
    if (j < 2) {
        float s = 0.f;
        for (int i = 0; i < nch; ++i) s += part[((size_t)b * nch + i) * 2 + j];
        tot[j] = s;
    }
    __syncthreads();
    const float sq = tot[0], sw = tot[1];
    if (c == 0 && j == 0) {
        const float v = sw > 0.f ? mu * sq / sw : 0.f;
        aloss[b] = v;
        if (sw > 0.f) parts[b * 4 + 0] += v;
    }
    if (!(sw > 0.f)) return;
    const float sc = 2.f * mu / sw;
#pragma unroll
    for (int i = 0; i < ACH / 256; ++i) {
        const int t = c * ACH + j + 256 * i;
        if (t < T) {
            const size_t k = (size_t)b * T + t;
            const float wv = w[k];
            if (wv != 0.f) {
                const float xv = x[k];
                grad[k] += sc * wv * (inv_mu_law(xv) - ref[k]) * inv_mu_law_grad(xv);
            }
        }
    }
}

}  // namespace

int anchor_chunks(int T) { return T / ACH + (T % ACH != 0); }

void launch_anchor(const float* x, const float* ref, const float* w, float* part, float* grad,
                   float* parts, float* aloss, float mu, int B, int T, hipStream_t s) {
    const int nch = anchor_chunks(T);
    hipLaunchKernelGGL(k_anchor_part, dim3(nch, B), dim3(256), 0, s, x, ref, w, part, T, nch);
    hipLaunchKernelGGL(k_anchor_apply, dim3(nch, B), dim3(256), 0, s, x, ref, w, part, grad, parts,
                       aloss, T, nch, mu);
}

}  // namespace ast
