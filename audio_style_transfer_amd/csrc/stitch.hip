// ast_stitch: join the optimised windows of a long-form run into one signal (no reference
// counterpart).  Window k of n holds T mu-law samples and starts hop = T - 2 late - fade samples
// after window k - 1; the guard of `late` samples at both ends of a window is discarded
// (methods.py:39,176) and neighbours overlap by `fade` valid samples.  Output sample s (file
// position st + late + s) lies in window k = min(s / hop, n - 1) at valid index j = s - k hop and,
// when k > 0 and j < fade, also in the fade-out of window k - 1 at j + hop:
//
//   out[s] = a(x[k][late + j])                                             outside a crossfade
//          = (1 - r) a(x[k-1][late + j + hop]) + r a(x[k][late + j]),      r = sin^2(pi/2 (j + 1/2) / fade)
//
// (the fade-out weight r((fade - j - 1/2) / fade) is 1 - r).  a is the output path's
// inv_mu_law_numpy (utils.py:85-90, x == 0 -> 0).  A gather: one thread per output sample, no
// atomics, so the result is deterministic; equal neighbours return their common value exactly.
#include "common.h"

namespace ast {
namespace {

// utils.py:85-90 inv_mu_law_numpy: sign(o) / 255 (256^|o| - 1), o = (x + 0.5) 2 / 256
__device__ __forceinline__ float inv_mu_law_out(float x) {
    const float o = fmaf(x, 2.f / 256.f, 1.f / 256.f);
    const float v = (exp2f(8.f * fabsf(o)) - 1.f) / 255.f;
    return x == 0.f ? 0.f : copysignf(v, o);
}

__global__ void __launch_bounds__(256) k_stitch(const float* __restrict__ x, float* __restrict__ out,
                                                int n, int T, int late, int fade, int hop,
                                                long long n_out) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_out) return;
    long long k = s / hop;
    if (k > n - 1) k = n - 1;
    const int j = (int)(s - k * hop);              // 0 <= j < T - 2 late
    const float cur = inv_mu_law_out(x[(size_t)k * T + late + j]);
    float v = cur;
    if (k > 0 && j < fade) {
        const float prev = inv_mu_law_out(x[(size_t)(k - 1) * T + late + j + hop]);
        const float sn = sinpif(0.5f * ((float)j + 0.5f) / (float)fade);
        v = fmaf(sn * sn, cur - prev, prev);
    }
    out[s] = v;
}

}  // namespace

void launch_stitch(const float* x, float* out, int n, int T, int late, int fade, hipStream_t s) {
    const int hop = T - 2 * late - fade;
    const long long n_out = (long long)(n - 1) * hop + T - 2 * late;
    hipLaunchKernelGGL(k_stitch, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, x, out, n, T,
                       late, fade, hop, n_out);
}

}  // namespace ast
