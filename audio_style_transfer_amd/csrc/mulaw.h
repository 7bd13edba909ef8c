// The TF inv_mu_law (utils.py:92-104) and its derivative on the device, shared by the loss terms
// that see the audio rather than the mu-law units: the STFT regulariser (stft_reg.hip) and the
// seam anchor term (anchor.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ast {

__device__ __forceinline__ float abs_tf(float v) { return fmaxf(v, 1e-12f) + fmaxf(0.f, -v); }
__device__ __forceinline__ float abs_tf_grad(float v) {
    return (v >= 1e-12f ? 1.f : 0.f) - (v < 0.f ? 1.f : 0.f);
}

// utils.py:99-104 inv_mu_law (TF version): value
__device__ __forceinline__ float inv_mu_law(float x) {
    const float o = (x + 0.5f) * (2.f / 256.f);
    const float a = abs_tf(o);
    const float num = fabsf(o) <= 1e-12f ? 0.f : o;
    const float out = num / a / 255.f * (exp2f(8.f * a) - 1.f);   // 256^a = 2^(8a)
    return x == 0.f ? x : out;
}

// ... and d value / d x (same formula as the oracle's inv_mu_law_tf)
__device__ __forceinline__ float inv_mu_law_grad(float x) {
    const float o = (x + 0.5f) * (2.f / 256.f);
    const float a = abs_tf(o);
    const float da = abs_tf_grad(o);
    const bool tiny = fabsf(o) <= 1e-12f;
    const float num = tiny ? 0.f : o;
    const float dnum = tiny ? 0.f : 1.f;
    const float sgn = num / a;
    const float dsgn = (dnum * a - num * da) / (a * a);
    const float p = exp2f(8.f * a);
    const float dp = p * 5.545177444479562f * da;                    // ln 256
    const float dout = (dsgn * (p - 1.f) + sgn * dp) / 255.f * (2.f / 256.f);
    return x == 0.f ? 1.f : dout;
}

}  // namespace ast
