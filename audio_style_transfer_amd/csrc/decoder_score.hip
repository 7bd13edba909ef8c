// The NSynth WaveNet decoder teacher-forced over whole sequences: the probability it assigns to a
// given waveform under a given encoding (Config.build's decoder and loss, nsynth/wavenet/model.py:
// 264-320, in the arithmetic of the step form in decoder.hip).
//
// Nothing is sequential here, so time goes on the N side of every product:
//   Y[M, T] = W[M, K] X[K, T]  on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation),
// with the packed A chunks of the ast_dec context exactly as decoder.hip lays them out (chunk (m, g):
// rows 16m.., k 16g.., 64 lanes x float4), and activations stored [clip][t][channel], so the B
// operand of column t is a float4 of row t (row t - rate, t - 2 rate for the earlier taps; rows
// before 0 read as zero).  One set_weights / restore serves synthesis and scoring.
//
// Kernels, per call (layer dependencies are kernel boundaries; no atomics, no cross-workgroup
// synchronisation, vector stores only):
//   k_score_start   l(t) = startconv(x_s(t-2), x_s(t-1), x_s(t)),  x_s(t) = table[bins[t-1]], x_s(0) = 0
//   k_score_mix     s = skip_start(l)                               (the mix kernel, skip rows only)
//   per layer i:
//     k_score_gate  d = sigmoid(a[:w]) tanh(a[w:]),  a = W0 l(t-2r) + W1 l(t-r) + W2 l(t) + Wc enc[t / hop] + b
//     k_score_mix   l += res_i(d);  s += skip_i(d)    -- in place: the update is pointwise in (t,
//                   channel), each element is owned by one lane, and the gate kernel that reads
//                   l(t - r) of other tiles has finished (a kernel boundary) before it runs
//   k_score_tail    relu, out1 + cond_map_out1, relu, logits, softmax, logp
//   k_score_nll     nll[b] = -(1/T) sum_t logp[b, t]
//
// A wave owns a tile of 32 output channels (gate: the 32 sigmoid rows and their 32 tanh rows) by
// 64 time steps of one clip; a workgroup is 2 x 2 waves (64 channels x 128 steps).  Tiles never
// mix clips; columns at t >= T load zeros and store nothing.
//
// The order that defines the result, the same for every batch size, slot, T and tile position
// (every output column is a function of its own B column only):
//   gate / mix / skip_start / out1 / logits: one accumulator per output element over the chunks
//     g = 0, 1, ... in ascending order (gate: tap t - 2r, tap t - r, tap t, then the encoding chunk),
//     the four MFMAs of a chunk in ascending k; then the biases (gate: + b_dil, then + b_cond);
//   softmax: max (exact), expf, the denominator a running fp32 sum in bin order;
//     logp = (logit[label] - max) - logf(sum);  pmf = exp / sum;
//   nll: thread j of 256 adds logp[j], logp[j + 256], ... in fp64, then a fixed binary tree.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string>

#include "../../include/astyle.h"
#include "decoder.h"

namespace {

constexpr int NBIN = 256;
constexpr int PST = NBIN + 1;      // LDS row stride of the logits (odd: no bank conflicts by column)
constexpr int NT = 4;              // 16-column chunks per wave: 64 time steps
constexpr int TW = 2 * NT * 16;    // time steps per workgroup (2 waves along time)
constexpr int TAILW = 8;           // waves of the tail kernel

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ inline f4 mfma_chunk(const f4 a, const f4 b, f4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline f4 ldv(const float* p) { return *reinterpret_cast<const f4*>(p); }

__device__ inline float table_xs(const float* tab_xs, int bin, int mode) {
    bin = min(max(bin, 0), NBIN - 1);
    return mode == 0 ? tab_xs[bin] : (float)(bin - 128) / 128.f;
}

// startconv at one channel, as decoder.hip's start_val
__device__ inline float start_val(float w0, float w1, float w2, float b, float x2, float x1, float x0) {
    return fmaf(x0, w2, fmaf(x1, w1, x2 * w0)) + b;
}

struct SStart {
    const float* wstart;   // [3][width]
    const float* bstart;   // [width]
    const float* tab_xs;
    const int* bins;       // [B][T]
    float* l;              // [B][T][width]
    int T, width, mode;
};

__global__ __launch_bounds__(256) void k_score_start(SStart a) {
    const int W4 = a.width / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.T * W4) return;
    const int t = (int)(i / W4), k = (int)(i - (long long)t * W4) * 4, clip = blockIdx.y;
    const int* bn = a.bins + (size_t)clip * a.T;
    const float x0 = t >= 1 ? table_xs(a.tab_xs, bn[t - 1], a.mode) : 0.f;
    const float x1 = t >= 2 ? table_xs(a.tab_xs, bn[t - 2], a.mode) : 0.f;
    const float x2 = t >= 3 ? table_xs(a.tab_xs, bn[t - 3], a.mode) : 0.f;
    const float4 c0 = ld4(a.wstart + k), c1 = ld4(a.wstart + a.width + k), c2 = ld4(a.wstart + 2 * a.width + k);
    const float4 cb = ld4(a.bstart + k);
    const float4 v = make_float4(start_val(c0.x, c1.x, c2.x, cb.x, x2, x1, x0), start_val(c0.y, c1.y, c2.y, cb.y, x2, x1, x0),
                                 start_val(c0.z, c1.z, c2.z, cb.z, x2, x1, x0), start_val(c0.w, c1.w, c2.w, cb.w, x2, x1, x0));
    *reinterpret_cast<float4*>(a.l + ((size_t)clip * a.T + t) * a.width + k) = v;
}

struct SGate {
    const float* A;       // packed [2 width / 16][(3 width + 16) / 16][256]
    const float* bdil;    // [2 width]
    const float* bcond;   // [2 width]
    const float* l;       // [B][T][width]
    const float* enc;     // [B][R][16]
    float* d;             // [B][T][width]
    int T, width, rate, R, hop;
};

__global__ __launch_bounds__(256) void k_score_gate(SGate a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int clip = blockIdx.z;
    const int t0 = blockIdx.y * TW + (wave >> 1) * (NT * 16);
    if (t0 >= a.T) return;
    const int Gw = a.width / 16, G = 3 * Gw + 1;
    const int m0 = blockIdx.x * 4 + (wave & 1) * 2;       // sigmoid chunks m0, m0 + 1; tanh chunks Gw + those
    const float* Ap[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) Ap[m] = a.A + (size_t)((m >> 1) * Gw + m0 + (m & 1)) * G * 256 + lane * 4;
    f4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f4{0.f, 0.f, 0.f, 0.f};
    const float* lc = a.l + (size_t)clip * a.T * a.width + q * 4;
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    // K in ascending chunks: taps t - 2 rate, t - rate, t (Gw chunks each), then the encoding row.
    // B loads are unconditional from a clamped row and masked afterwards; within a tap, chunk
    // gi + 1 is loaded before the MFMAs of chunk gi (the last trip loads the last chunk again).
    for (int seg = 0; seg < 3; ++seg) {
        const int shift = (2 - seg) * a.rate;
        const float* bp[NT];
        bool ok[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int t = t0 + 16 * n + r, ts = t - shift;
            ok[n] = t < a.T && ts >= 0;
            bp[n] = lc + (size_t)(ok[n] ? ts : 0) * a.width;
        }
        const float* As[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) As[m] = Ap[m] + (size_t)seg * Gw * 256;
        // two buffers in turn, so no register copies tie a trip's MFMAs to the next trip's loads
        f4 av[4], bv[NT], aw[4], bw[NT];
#define SCORE_LOAD(A_, B_, G_)                                           \
    _Pragma("unroll") for (int m = 0; m < 4; ++m) A_[m] = ldv(As[m] + (size_t)(G_) * 256); \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) B_[n] = ldv(bp[n] + (G_) * 16);        \
    __builtin_amdgcn_sched_barrier(0);
#define SCORE_MMA(A_, B_)                                                                \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) B_[n] = ok[n] ? B_[n] : zero;         \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                        \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) acc[m][n] = mfma_chunk(A_[m], B_[n], acc[m][n]); \
    __builtin_amdgcn_sched_barrier(0);
        SCORE_LOAD(av, bv, 0)
        for (int gi = 0; gi < Gw; gi += 2) {               // Gw is a multiple of 4
            SCORE_LOAD(aw, bw, gi + 1)
            SCORE_MMA(av, bv)
            SCORE_LOAD(av, bv, min(gi + 2, Gw - 1))
            SCORE_MMA(aw, bw)
        }
#undef SCORE_LOAD
#undef SCORE_MMA
    }
    {                                                      // the encoding chunk: row t / hop per column
        f4 av[4], bv[NT];
#pragma unroll
        for (int m = 0; m < 4; ++m) av[m] = ldv(Ap[m] + (size_t)3 * Gw * 256);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int t = t0 + 16 * n + r;
            bv[n] = ldv(a.enc + ((size_t)clip * a.R + (t < a.T ? t / a.hop : 0)) * 16 + q * 4);
            bv[n] = t < a.T ? bv[n] : zero;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = mfma_chunk(av[m], bv[n], acc[m][n]);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int ch = (m0 + mi) * 16 + q * 4;
        const float4 bs = ld4(a.bdil + ch), cs = ld4(a.bcond + ch);
        const float4 bt = ld4(a.bdil + a.width + ch), ct = ld4(a.bcond + a.width + ch);
        const float bsv[4] = {bs.x, bs.y, bs.z, bs.w}, csv[4] = {cs.x, cs.y, cs.z, cs.w};
        const float btv[4] = {bt.x, bt.y, bt.z, bt.w}, ctv[4] = {ct.x, ct.y, ct.z, ct.w};
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int t = t0 + 16 * n + r;
            if (t >= a.T) continue;
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float vs = acc[mi][n][i] + bsv[i] + csv[i];
                const float vt = acc[2 + mi][n][i] + btv[i] + ctv[i];
                o[i] = (1.f / (1.f + expf(-vs))) * tanhf(vt);
            }
            *reinterpret_cast<float4*>(a.d + ((size_t)clip * a.T + t) * a.width + ch) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

struct SMix {
    const float* A;      // packed [Mc][width / 16][256]: nres res chunks, then skip chunks
    const float* bres;   // [width]
    const float* bskip;  // [skip]
    const float* x;      // [B][T][width]: d (skip_start: l)
    float* l;            // [B][T][width]
    float* s;            // [B][T][skip]
    int T, width, skip, Mc, nres, init;   // init: s = skip(x) (skip_start) instead of s += skip(x)
};

__global__ __launch_bounds__(256) void k_score_mix(SMix a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int clip = blockIdx.z;
    const int t0 = blockIdx.y * TW + (wave >> 1) * (NT * 16);
    const int m0 = blockIdx.x * 4 + (wave & 1) * 2;       // output chunks m0, m0 + 1: both res or both skip
    if (t0 >= a.T || m0 >= a.Mc) return;
    const int Gw = a.width / 16;
    const float* Ap[2] = {a.A + (size_t)m0 * Gw * 256 + lane * 4, a.A + (size_t)(m0 + 1) * Gw * 256 + lane * 4};
    f4 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f4{0.f, 0.f, 0.f, 0.f};
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* bp[NT];
    bool ok[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int t = t0 + 16 * n + r;
        ok[n] = t < a.T;
        bp[n] = a.x + ((size_t)clip * a.T + (ok[n] ? t : 0)) * a.width + q * 4;
    }
    // chunk g + 1 is loaded before the MFMAs of chunk g (the last trip reloads its own chunk);
    // B loads are unconditional from a clamped row and masked afterwards
    f4 av[2], bv[NT], aw[2], bw[NT];                       // two buffers in turn: no register copies
#define SCORE_LOAD(A_, B_, G_)                                           \
    _Pragma("unroll") for (int m = 0; m < 2; ++m) A_[m] = ldv(Ap[m] + (size_t)(G_) * 256); \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) B_[n] = ldv(bp[n] + (G_) * 16);        \
    __builtin_amdgcn_sched_barrier(0);
#define SCORE_MMA(A_, B_)                                                                \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) B_[n] = ok[n] ? B_[n] : zero;         \
    _Pragma("unroll") for (int m = 0; m < 2; ++m)                                        \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) acc[m][n] = mfma_chunk(A_[m], B_[n], acc[m][n]); \
    __builtin_amdgcn_sched_barrier(0);
    SCORE_LOAD(av, bv, 0)
    for (int g = 0; g < Gw; g += 2) {                      // Gw is a multiple of 4
        SCORE_LOAD(aw, bw, g + 1)
        SCORE_MMA(av, bv)
        SCORE_LOAD(av, bv, min(g + 2, Gw - 1))
        SCORE_MMA(aw, bw)
    }
#undef SCORE_LOAD
#undef SCORE_MMA
    const bool res = m0 < a.nres;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int ch = (res ? m0 + mi : m0 + mi - a.nres) * 16 + q * 4;
        const float4 b = ld4((res ? a.bres : a.bskip) + ch);
        const int cw = res ? a.width : a.skip;
        float* dst = res ? a.l : a.s;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            if (!ok[n]) continue;
            float4* p = reinterpret_cast<float4*>(dst + ((size_t)clip * a.T + t0 + 16 * n + r) * cw + ch);
            const f4 v = acc[mi][n];
            float4 o = make_float4(v[0] + b.x, v[1] + b.y, v[2] + b.z, v[3] + b.w);
            if (res || !a.init) {
                const float4 old = *p;
                o = make_float4(old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w);
            }
            *p = o;
        }
    }
}

struct STail {
    const float* A1;      // out1 | cond_map_out1 packed [skip/16][(skip + 16)/16][256]
    const float* b1;      // out1 biases [skip]
    const float* bc1;     // cond_map_out1 biases [skip]
    const float* A2;      // logits packed [16][skip/16][256]
    const float* b2;      // [256]
    const float* s;       // [B][T][skip]
    const float* enc;     // [B][R][16]
    const int* bins;      // [B][T]
    float* logp;          // [B][T]
    float* pmf;           // NULL or [B][T][256]
    float* logits;        // NULL or [B][T][256]
    int T, skip, R, hop;
};

// 16 time steps of one clip per workgroup
__global__ __launch_bounds__(TAILW * 64) void k_score_tail(STail a) {
    extern __shared__ __align__(16) float lds[];
    const int clip = blockIdx.y, t0 = blockIdx.x * 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int K1 = a.skip + 16, XS = K1 + 4, HS = a.skip + 4;
    float* X = lds;                  // [16][XS]: relu(s) | en
    float* H = X + 16 * XS;          // [16][HS]
    float* P = H + 16 * HS;          // [16][PST]: logits -> exp
    float* sums = P + 16 * PST;      // [16]
    float* lab = sums + 16;          // [16]: logit[label] - max
    for (int i = tid; i < 16 * K1; i += TAILW * 64) {
        const int c = i / K1, k = i - c * K1, t = t0 + c;
        float v = 0.f;
        if (t < a.T)
            v = k < a.skip ? fmaxf(a.s[((size_t)clip * a.T + t) * a.skip + k], 0.f)
                           : a.enc[((size_t)clip * a.R + t / a.hop) * 16 + (k - a.skip)];
        X[c * XS + k] = v;
    }
    __syncthreads();
    const int G1 = K1 / 16, G2 = a.skip / 16;
    for (int m = wave; m < G2; m += TAILW) {      // out1 + cond_map_out1, relu
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* A = a.A1 + (size_t)m * G1 * 256 + lane * 4;
        for (int g = 0; g < G1; ++g) acc = mfma_chunk(ldv(A + (size_t)g * 256), ldv(X + r * XS + g * 16 + q * 4), acc);
        for (int i = 0; i < 4; ++i) {
            const int ch = m * 16 + q * 4 + i;
            H[r * HS + ch] = fmaxf(acc[i] + a.b1[ch] + a.bc1[ch], 0.f);
        }
    }
    __syncthreads();
    for (int m = wave; m < NBIN / 16; m += TAILW) {   // logits
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* A = a.A2 + (size_t)m * G2 * 256 + lane * 4;
        for (int g = 0; g < G2; ++g) acc = mfma_chunk(ldv(A + (size_t)g * 256), ldv(H + r * HS + g * 16 + q * 4), acc);
        for (int i = 0; i < 4; ++i) {
            const int ch = m * 16 + q * 4 + i;
            P[r * PST + ch] = acc[i] + a.b2[ch];
        }
    }
    __syncthreads();
    for (int c = wave; c < 16; c += TAILW) {          // exp(x - max); the label's logit - max
        const int t = t0 + c;
        const int label = t < a.T ? min(max(a.bins[(size_t)clip * a.T + t], 0), NBIN - 1) : 0;
        float v[4], mx;
        for (int i = 0; i < 4; ++i) v[i] = P[c * PST + lane + 64 * i];
        if (a.logits && t < a.T)
            for (int i = 0; i < 4; ++i) a.logits[((size_t)clip * a.T + t) * NBIN + lane + 64 * i] = v[i];
        mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        for (int i = 0; i < 4; ++i) {
            if (lane + 64 * i == label) lab[c] = v[i] - mx;
            P[c * PST + lane + 64 * i] = expf(v[i] - mx);
        }
    }
    __syncthreads();
    if (tid < 16) {                                   // the denominator: a running sum in bin order
        float sum = 0.f;
#pragma unroll 16
        for (int k = 0; k < NBIN; ++k) sum += P[tid * PST + k];
        sums[tid] = sum;
        if (t0 + tid < a.T) a.logp[(size_t)clip * a.T + t0 + tid] = lab[tid] - logf(sum);
    }
    if (a.pmf) {
        __syncthreads();
        for (int i = tid; i < 16 * NBIN; i += TAILW * 64) {
            const int c = i >> 8, k = i & 255, t = t0 + c;
            if (t < a.T) a.pmf[((size_t)clip * a.T + t) * NBIN + k] = P[c * PST + k] / sums[c];
        }
    }
}

__global__ __launch_bounds__(256) void k_score_nll(const float* logp, float* nll, int T) {
    __shared__ double part[256];
    const float* p = logp + (size_t)blockIdx.x * T;
    double acc = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) acc += (double)p[t];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) nll[blockIdx.x] = (float)(-part[0] / (double)T);
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// l, d [batch][T][width], s [batch][T][skip]
size_t score_bytes(const ast_dec_cfg& c, int batch, int T, size_t* off_d, size_t* off_s) {
    const size_t n = (size_t)batch * T;
    const size_t lw = up256(n * c.width * 4), sw = up256(n * c.skip_width * 4);
    if (off_d) *off_d = lw;
    if (off_s) *off_s = 2 * lw;
    return 2 * lw + sw;
}

int check_bt(const char* who, int batch, int T, int width) {
    char m[256];
    if (batch < 1 || batch > 65535) {
        snprintf(m, sizeof m, "%s: batch %d, must be 1..65535", who, batch);
        return ast::set_error(AST_E_ARG, m);
    }
    if (T < 1 || (long long)T * width >= (1LL << 33)) {
        snprintf(m, sizeof m, "%s: T %d, must be >= 1 with T * width < 2^33", who, T);
        return ast::set_error(AST_E_ARG, m);
    }
    return 0;
}

}  // namespace

extern "C" {

int ast_dec_score_workspace_bytes(const ast_dec_cfg* cfg, int batch, int T, size_t* out) {
    if (!out) return ast::set_error(AST_E_ARG, "ast_dec_score_workspace_bytes: null argument");
    int rc = ast::dec_check_cfg(cfg);
    if (rc) return rc;
    rc = check_bt("ast_dec_score_workspace_bytes", batch, T, cfg->width);
    if (rc) return rc;
    *out = score_bytes(*cfg, batch, T, nullptr, nullptr);
    return 0;
}

int ast_dec_score(ast_dec* x, const int* bins_dev, const float* enc_dev, int batch, int R, int T, int input_mode,
                  void* work_dev, size_t work_bytes, float* logp_dev, float* nll_dev, float* pmf_dev,
                  float* logits_dev, void* stream) {
    if (!x || !bins_dev || !enc_dev || !work_dev || !logp_dev || !nll_dev)
        return ast::set_error(AST_E_ARG, "ast_dec_score: null argument (context, bins, enc, work, logp and nll are required)");
    const ast_dec_cfg& c = x->c;
    if (R < 1 || T < 1 || (long long)T > (long long)R * c.hop)
        return ast::set_error(AST_E_ARG, "ast_dec_score: T " + std::to_string(T) + " must be 1..R*hop = " +
                                             std::to_string((long long)R * c.hop));
    const int rc = check_bt("ast_dec_score", batch, T, c.width);
    if (rc) return rc;
    if (input_mode != 0 && input_mode != 1)
        return ast::set_error(AST_E_ARG, "ast_dec_score: input_mode " + std::to_string(input_mode) +
                                             ", must be 0 (the synthesis table) or 1 ((bin - 128) / 128)");
    size_t off_d, off_s;
    const size_t need = score_bytes(c, batch, T, &off_d, &off_s);
    if (work_bytes < need)
        return ast::set_error(AST_E_ARG, "ast_dec_score: work_bytes " + std::to_string(work_bytes) + ", batch " +
                                             std::to_string(batch) + " x T " + std::to_string(T) + " needs " +
                                             std::to_string(need));
    if ((size_t)work_dev & 15) return ast::set_error(AST_E_ARG, "ast_dec_score: work_dev must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int w = c.width, s = c.skip_width, Gw = w / 16;
    float* l = (float*)work_dev;
    float* d = (float*)((char*)work_dev + off_d);
    float* sk = (float*)((char*)work_dev + off_s);
    const unsigned tiles = (unsigned)((T + TW - 1) / TW);
    SStart sa = {x->wstart, x->bstart, x->tab_xs, bins_dev, l, T, w, input_mode};
    const long long n4 = (long long)T * (w / 4);
    k_score_start<<<dim3((unsigned)((n4 + 255) / 256), batch), 256, 0, st>>>(sa);
    SMix m0 = {x->A_skip0, x->bskip0, x->bskip0, l, l, sk, T, w, s, s / 16, 0, 1};
    k_score_mix<<<dim3((s / 16 + 3) / 4, tiles, batch), 256, 0, st>>>(m0);
    for (int i = 0; i < c.n_layers; ++i) {
        SGate ga = {x->A_gate + (size_t)i * x->gate_sz, x->bdil + (size_t)i * 2 * w, x->bcond + (size_t)i * 2 * w,
                    l, enc_dev, d, T, w, 1 << (i % c.n_stages), R, c.hop};
        k_score_gate<<<dim3(Gw / 4, tiles, batch), 256, 0, st>>>(ga);
        SMix ma = {x->A_mix + (size_t)i * x->mix_sz, x->bres + (size_t)i * w, x->bskip + (size_t)i * s,
                   d, l, sk, T, w, s, Gw + s / 16, Gw, 0};
        k_score_mix<<<dim3((Gw + s / 16 + 3) / 4, tiles, batch), 256, 0, st>>>(ma);
    }
    STail ta = {x->A1, x->b1, x->bc1, x->A2, x->b2, sk, enc_dev, bins_dev, logp_dev, pmf_dev, logits_dev, T, s, R, c.hop};
    const size_t lds = (size_t)(16 * (s + 20) + 16 * (s + 4) + 16 * PST + 32) * 4;
    k_score_tail<<<dim3((T + 15) / 16, batch), TAILW * 64, lds, st>>>(ta);
    k_score_nll<<<batch, 256, 0, st>>>(logp_dev, nll_dev, T);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ast::set_error(AST_E_HIP, std::string("ast_dec_score: ") + hipGetErrorString(e));
}

}  // extern "C"
