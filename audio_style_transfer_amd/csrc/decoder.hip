// The NSynth WaveNet decoder, one sample step at a time (nsynth/wavenet/model.py:28-137
// FastGenerationConfig, nsynth/utils.py:838-908 causal_linear / linear, fastgen.py:160-212).
//
// Every product is a skinny GEMM  Y[M, clips] = W[M, K] X[K, clips]  on v_mfma_f32_16x16x4_f32
// (fp32 operands, fp32 accumulation): output channels on the M side, 16 clips (padded with zero
// columns) on the N side.  Weights are stored packed for the A operand: chunk (m, g) holds rows
// 16m..16m+15 and k 16g..16g+15 as 64 lanes x float4, lane (q = lane >> 4, r = lane & 15) holding
// W[16m + r][16g + 4q + 0..3]; MFMA j of the chunk pairs element j of that float4 with the B
// operand X[16g + 4q + j][clip r], which is a float4 of the clip's channel-contiguous row.  So one
// chunk is one 1 KiB wave load and four MFMAs.
//
// The order that defines the result, the same for every batch size and slot:
//   gate / mix / skip_start: wave w of NW (gate: NWG) accumulates chunks g = w, w + NW, ... in
//     ascending g; the NW partial tiles are added in ascending w, then the biases;
//   out1 / logits: one wave accumulates a tile's chunks in ascending g, then the biases;
//   softmax: max (exact), expf, the denominator a running sum in bin order, one division per bin;
//   cdf: a running sum in bin order.
// No atomics, no cross-workgroup synchronisation: layer dependencies are kernel boundaries.
//
// Queues: layer i (rate r) keeps its input l of the last 2r steps in a ring [2r][B][width].  The
// slot t mod 2r holds l(t - 2r), which every gate workgroup of the step reads; the mix kernel
// overwrites it with l(t) after the gate kernel finished, each workgroup copying the rows it owns
// before it updates them.  Steps before 0 read as zero by a position test, so the ring needs no
// clearing.  The position lives per 16-clip tile (all equal), so the tail workgroup that advances
// a tile's position is the only workgroup of that kernel that reads it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/astyle.h"
#include "ckpt.h"
#include "decoder.h"

namespace {

constexpr int NW = 8;             // waves per workgroup
constexpr int NWG = 16;           // ... of the gate kernel (the most bytes per workgroup)
constexpr int DEPTH = 4;          // chunks a wave loads before their MFMAs (bytes in flight)
constexpr int NBIN = 256;
constexpr int PST = NBIN + 1;     // LDS row stride of the logits / pmf (odd: no bank conflicts by clip)
constexpr int MAX_SKIP = 352;     // the tail kernel's LDS (16 clips) stays within 64 KiB
constexpr int MAX_WIDTH = 4096;
constexpr int MAX_LAYERS = 64;

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ inline f4 mfma_chunk(const float4 a, const float4 b, f4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the partial tiles of the NW waves, added in ascending wave order: thread (row rr, clip cc)
__device__ inline float reduce_tile(const float* red /*[nw][64][4]*/, int rr, int cc, int nw = NW) {
    const int ln = (rr >> 2) * 16 + cc, i = rr & 3;
    float v = red[ln * 4 + i];
    for (int w = 1; w < nw; ++w) v += red[(w * 64 + ln) * 4 + i];
    return v;
}

// startconv at one channel: (state_2 w_0 + state_1 w_1) + x w_2 + b, as causal_linear adds them
__device__ inline float start_val(float w0, float w1, float w2, float b, float x2, float x1, float x0) {
    return fmaf(x0, w2, fmaf(x1, w1, x2 * w0)) + b;
}

struct StartArgs {
    const float* A;        // skip_start packed [skip/16][width/16][256]
    const float* wstart;   // [3][width]
    const float* bstart;   // [width]
    const float* bskip0;   // [skip]
    const float* xq;       // [B][4]: x_s(t), x_s(t-1), x_s(t-2)
    const int* pos;
    float* l;              // [B][width]
    float* s;              // [B][skip]
    int B, width, skip, total;
};

__global__ __launch_bounds__(NW * 64) void k_dec_start(StartArgs a) {
    __shared__ float red[NW * 64 * 4];
    const int tile = blockIdx.y;
    const int t = a.pos[tile];
    if (t >= a.total) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int col = tile * 16 + r;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (col < a.B) {
        x0 = a.xq[col * 4 + 0];
        x1 = a.xq[col * 4 + 1];
        x2 = a.xq[col * 4 + 2];
    }
    const int G = a.width / 16;
    const float *w0 = a.wstart, *w1 = a.wstart + a.width, *w2 = a.wstart + 2 * a.width;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int g = wave; g < G; g += NW) {
        const int k = g * 16 + q * 4;
        const float4 c0 = ld4(w0 + k), c1 = ld4(w1 + k), c2 = ld4(w2 + k), cb = ld4(a.bstart + k);
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < a.B)
            b = make_float4(start_val(c0.x, c1.x, c2.x, cb.x, x2, x1, x0), start_val(c0.y, c1.y, c2.y, cb.y, x2, x1, x0),
                            start_val(c0.z, c1.z, c2.z, cb.z, x2, x1, x0), start_val(c0.w, c1.w, c2.w, cb.w, x2, x1, x0));
        if (blockIdx.x == 0 && col < a.B) *reinterpret_cast<float4*>(a.l + (size_t)col * a.width + k) = b;
        acc = mfma_chunk(ld4(a.A + ((size_t)blockIdx.x * G + g) * 256 + lane * 4), b, acc);
    }
    *reinterpret_cast<f4*>(red + (wave * 64 + lane) * 4) = acc;
    __syncthreads();
    if (tid < 256) {
        const int rr = tid & 15, cc = tid >> 4, c = tile * 16 + cc, ch = blockIdx.x * 16 + rr;
        if (c < a.B) a.s[(size_t)c * a.skip + ch] = reduce_tile(red, rr, cc) + a.bskip0[ch];
    }
}

struct GateArgs {
    const float* A;       // packed [2 width / 16][(3 width + 16) / 16][256]
    const float* bdil;    // [2 width]
    const float* bcond;   // [2 width]
    const float* l;       // [B][width]
    const float* ring;    // [2 rate][B][width]
    const float* enc;     // [B][R][16]
    const int* pos;
    float* d;             // [B][width]
    int B, width, rate, R, hop, total;
};

__global__ __launch_bounds__(NWG * 64) void k_dec_gate(GateArgs a) {
    __shared__ float red[2 * NWG * 64 * 4];
    const int tile = blockIdx.y;
    const int t = a.pos[tile];
    if (t >= a.total) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int col = tile * 16 + r;
    const bool live = col < a.B;
    const int Gw = a.width / 16, G = 3 * Gw + 1, slots = 2 * a.rate;
    const size_t cw = (size_t)(live ? col : 0) * a.width;
    const float* x2 = a.ring + (size_t)(t % slots) * a.B * a.width + cw;              // l(t - 2 rate)
    const float* x1 = a.ring + (size_t)((t + a.rate) % slots) * a.B * a.width + cw;   // l(t - rate)
    const float* x0 = a.l + cw;
    const float* xe = a.enc + ((size_t)(live ? col : 0) * a.R + t / a.hop) * 16;
    const bool ok2 = live && t >= 2 * a.rate, ok1 = live && t >= a.rate;
    const float* As = a.A + (size_t)blockIdx.x * G * 256 + lane * 4;
    const float* At = a.A + (size_t)(Gw + blockIdx.x) * G * 256 + lane * 4;
    f4 as = {0.f, 0.f, 0.f, 0.f}, at = {0.f, 0.f, 0.f, 0.f};
    auto load_b = [&](int g) {
        const int seg = g / Gw, gi = g - seg * Gw;
        const int o = gi * 16 + q * 4;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (seg == 0) {
            if (ok2) b = ld4(x2 + o);
        } else if (seg == 1) {
            if (ok1) b = ld4(x1 + o);
        } else if (seg == 2) {
            if (live) b = ld4(x0 + o);
        } else if (live) {
            b = ld4(xe + q * 4);
        }
        return b;
    };
    // DEPTH chunks per trip, all loads before the MFMAs; ascending g per wave
    for (int g0 = wave; g0 < G; g0 += DEPTH * NWG) {
        float4 sa[DEPTH], ta[DEPTH], bb[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            const int g = g0 + i * NWG;
            if (g < G) {
                sa[i] = ld4(As + (size_t)g * 256);
                ta[i] = ld4(At + (size_t)g * 256);
                bb[i] = load_b(g);
            }
        }
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            if (g0 + i * NWG < G) {
                as = mfma_chunk(sa[i], bb[i], as);
                at = mfma_chunk(ta[i], bb[i], at);
            }
        }
    }
    *reinterpret_cast<f4*>(red + (wave * 64 + lane) * 4) = as;
    *reinterpret_cast<f4*>(red + NWG * 256 + (wave * 64 + lane) * 4) = at;
    __syncthreads();
    if (tid < 256) {
        const int rr = tid & 15, cc = tid >> 4, c = tile * 16 + cc, ch = blockIdx.x * 16 + rr;
        if (c < a.B) {
            const float vs = reduce_tile(red, rr, cc, NWG) + a.bdil[ch] + a.bcond[ch];
            const float vt = reduce_tile(red + NWG * 256, rr, cc, NWG) + a.bdil[a.width + ch] + a.bcond[a.width + ch];
            a.d[(size_t)c * a.width + ch] = (1.f / (1.f + expf(-vs))) * tanhf(vt);
        }
    }
}

struct MixArgs {
    const float* A;      // packed [(width + skip) / 16][width / 16][256]: res rows, then skip rows
    const float* bres;   // [width]
    const float* bskip;  // [skip]
    const float* d;      // [B][width]
    const int* pos;
    float* l;
    float* s;
    float* ring;         // [2 rate][B][width]
    int B, width, skip, rate, total;
};

__global__ __launch_bounds__(NW * 64) void k_dec_mix(MixArgs a) {
    __shared__ float red[NW * 64 * 4];
    const int tile = blockIdx.y;
    const int t = a.pos[tile];
    if (t >= a.total) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int col = tile * 16 + r;
    const int G = a.width / 16;
    const float* x = a.d + (size_t)(col < a.B ? col : 0) * a.width + q * 4;
    const float* A = a.A + (size_t)blockIdx.x * G * 256 + lane * 4;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    const bool live = col < a.B;
    for (int g0 = wave; g0 < G; g0 += DEPTH * NW) {
        float4 aa[DEPTH], bb[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            const int g = g0 + i * NW;
            if (g < G) {
                aa[i] = ld4(A + (size_t)g * 256);
                bb[i] = live ? ld4(x + g * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int i = 0; i < DEPTH; ++i)
            if (g0 + i * NW < G) acc = mfma_chunk(aa[i], bb[i], acc);
    }
    *reinterpret_cast<f4*>(red + (wave * 64 + lane) * 4) = acc;
    __syncthreads();
    if (tid < 256) {
        const int rr = tid & 15, cc = tid >> 4, c = tile * 16 + cc;
        if (c < a.B) {
            const float v = reduce_tile(red, rr, cc);
            if ((int)blockIdx.x < G) {          // res rows: push the layer's input, then l += res(d)
                const int ch = blockIdx.x * 16 + rr;
                const size_t o = (size_t)c * a.width + ch;
                const float old = a.l[o];
                a.ring[(size_t)(t % (2 * a.rate)) * a.B * a.width + o] = old;
                a.l[o] = old + (v + a.bres[ch]);
            } else {                            // skip rows: s += skip(d)
                const int ch = (blockIdx.x - G) * 16 + rr;
                const size_t o = (size_t)c * a.skip + ch;
                a.s[o] = a.s[o] + (v + a.bskip[ch]);
            }
        }
    }
}

struct TailArgs {
    const float* A1;      // out1 | cond_map_out1 packed [skip/16][(skip + 16)/16][256]
    const float* b1;      // out1 biases [skip]
    const float* bc1;     // cond_map_out1 biases [skip]
    const float* A2;      // logits packed [16][skip/16][256]
    const float* b2;      // [256]
    const float* s;       // [B][skip]
    const float* enc;     // [B][R][16]
    const float* u;       // [B][total]
    const int* force;     // NULL or [B][total]
    const float* tab_audio;
    const float* tab_xs;
    int* pos;
    float* xq;            // [B][4]
    int* bins;            // [B][total]
    float* audio;         // [B][total]
    float* pmf;           // NULL or [B][total][256]
    int B, skip, R, hop, total;
};

__global__ __launch_bounds__(NW * 64) void k_dec_tail(TailArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int tile = blockIdx.x;
    const int t = a.pos[tile];
    if (t >= a.total) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int K1 = a.skip + 16, XS = K1 + 4, HS = a.skip + 4;
    float* X = lds;                  // [16][XS]: relu(s) | en
    float* H = X + 16 * XS;          // [16][HS]
    float* P = H + 16 * HS;          // [16][PST]: logits -> exp -> pmf
    float* sums = P + 16 * PST;      // [16]
    for (int i = tid; i < 16 * K1; i += NW * 64) {
        const int c = i / K1, k = i - c * K1, col = tile * 16 + c;
        float v = 0.f;
        if (col < a.B)
            v = k < a.skip ? fmaxf(a.s[(size_t)col * a.skip + k], 0.f)
                           : a.enc[((size_t)col * a.R + t / a.hop) * 16 + (k - a.skip)];
        X[c * XS + k] = v;
    }
    __syncthreads();
    const int G1 = K1 / 16, G2 = a.skip / 16;
    for (int m = wave; m < G2; m += NW) {      // out1 + cond_map_out1, relu
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* A = a.A1 + (size_t)m * G1 * 256 + lane * 4;
        for (int g = 0; g < G1; ++g) acc = mfma_chunk(ld4(A + (size_t)g * 256), ld4(X + r * XS + g * 16 + q * 4), acc);
        for (int i = 0; i < 4; ++i) {
            const int ch = m * 16 + q * 4 + i;
            H[r * HS + ch] = fmaxf(acc[i] + a.b1[ch] + a.bc1[ch], 0.f);
        }
    }
    __syncthreads();
    for (int m = wave; m < NBIN / 16; m += NW) {   // logits
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* A = a.A2 + (size_t)m * G2 * 256 + lane * 4;
        for (int g = 0; g < G2; ++g) acc = mfma_chunk(ld4(A + (size_t)g * 256), ld4(H + r * HS + g * 16 + q * 4), acc);
        for (int i = 0; i < 4; ++i) {
            const int ch = m * 16 + q * 4 + i;
            P[r * PST + ch] = acc[i] + a.b2[ch];
        }
    }
    __syncthreads();
    for (int c = wave; c < 16; c += NW) {          // exp(x - max)
        float v[4], mx;
        for (int i = 0; i < 4; ++i) v[i] = P[c * PST + lane + 64 * i];
        mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        for (int i = 0; i < 4; ++i) P[c * PST + lane + 64 * i] = expf(v[i] - mx);
    }
    __syncthreads();
    if (tid < 16) {                                // the denominator: a running sum in bin order
        float sum = 0.f;
#pragma unroll 16
        for (int k = 0; k < NBIN; ++k) sum += P[tid * PST + k];
        sums[tid] = sum;
    }
    __syncthreads();
    for (int i = tid; i < 16 * NBIN; i += NW * 64) {
        const int c = i >> 8, k = i & 255;
        P[c * PST + k] = P[c * PST + k] / sums[c];
    }
    __syncthreads();
    if (tid < 16 && tile * 16 + tid < a.B) {       // the draw: first k with cdf[k] >= u, clamped to 255
        const int col = tile * 16 + tid;
        const size_t o = (size_t)col * a.total + t;
        const float uu = a.u[o];
        float cdf = 0.f;
        int bin = NBIN - 1;
        bool found = false;
#pragma unroll 16
        for (int k = 0; k < NBIN; ++k) {
            cdf += P[tid * PST + k];
            if (!found && cdf >= uu) { bin = k; found = true; }
        }
        a.bins[o] = bin;
        a.audio[o] = a.tab_audio[bin];
        int nxt = bin;
        if (a.force) nxt = min(max(a.force[o], 0), NBIN - 1);
        a.xq[col * 4 + 2] = a.xq[col * 4 + 1];
        a.xq[col * 4 + 1] = a.xq[col * 4 + 0];
        a.xq[col * 4 + 0] = a.tab_xs[nxt];
    }
    if (a.pmf) {
        for (int i = tid; i < 16 * NBIN; i += NW * 64) {
            const int c = i >> 8, k = i & 255, col = tile * 16 + c;
            if (col < a.B) a.pmf[((size_t)col * a.total + t) * NBIN + k] = P[c * PST + k];
        }
    }
    if (tid == 0) a.pos[tile] = t + 1;
}

__global__ void k_dec_reset(int* pos, int ntile, float* xq, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ntile) pos[i] = 0;
    if (i < n) xq[i] = 0.f;
}

__global__ void k_dec_position(const int* pos, int* out) { *out = pos[0]; }

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

namespace {

int rate_of(const ast_dec_cfg& c, int layer) { return 1 << (layer % c.n_stages); }

int check_cfg(const ast_dec_cfg* c) {
    char m[256];
    if (!c) return ast::set_error(AST_E_ARG, "ast_dec: null configuration");
#define DEC_REQ(cond, ...)                                    \
    if (!(cond)) {                                            \
        snprintf(m, sizeof m, __VA_ARGS__);                   \
        return ast::set_error(AST_E_ARG, m);                  \
    }
    DEC_REQ(c->batch >= 1 && c->batch <= 256, "ast_dec: batch %d, must be 1..256", c->batch)
    DEC_REQ(c->width >= 64 && c->width % 64 == 0 && c->width <= MAX_WIDTH,
            "ast_dec: width %d, must be a multiple of 64 up to %d", c->width, MAX_WIDTH)
    DEC_REQ(c->skip_width >= 32 && c->skip_width % 32 == 0 && c->skip_width <= MAX_SKIP,
            "ast_dec: skip_width %d, must be a multiple of 32 up to %d", c->skip_width, MAX_SKIP)
    DEC_REQ(c->n_layers >= 1 && c->n_layers <= MAX_LAYERS, "ast_dec: n_layers %d, must be 1..%d", c->n_layers, MAX_LAYERS)
    DEC_REQ(c->n_stages >= 1 && c->n_stages <= 16, "ast_dec: n_stages %d, must be 1..16", c->n_stages)
    DEC_REQ(c->n_z == 16, "ast_dec: n_z %d, must be 16", c->n_z)
    DEC_REQ(c->hop >= 1, "ast_dec: hop %d, must be >= 1", c->hop)
#undef DEC_REQ
    return 0;
}

// carve the workspace; with base == nullptr only the size is computed
size_t carve(ast_dec* x, char* base) {
    const ast_dec_cfg& c = x->c;
    const size_t w = c.width, s = c.skip_width, L = c.n_layers, B = c.batch;
    size_t off = 0;
    auto take = [&](size_t floats) {
        char* p = base ? base + off : nullptr;
        off += up256(floats * 4);
        return (float*)p;
    };
    x->ntile = (c.batch + 15) / 16;
    x->gate_sz = 2 * w * (3 * w + 16);
    x->mix_sz = (w + s) * w;
    x->A_skip0 = take(s * w);
    x->wstart = take(3 * w);
    x->bstart = take(w);
    x->bskip0 = take(s);
    x->A_gate = take(L * x->gate_sz);
    x->bdil = take(L * 2 * w);
    x->bcond = take(L * 2 * w);
    x->A_mix = take(L * x->mix_sz);
    x->bres = take(L * w);
    x->bskip = take(L * s);
    x->A1 = take(s * (s + 16));
    x->b1 = take(s);
    x->bc1 = take(s);
    x->A2 = take((size_t)NBIN * s);
    x->b2 = take(NBIN);
    x->tab_audio = take(NBIN);
    x->tab_xs = take(NBIN);
    x->l = take(B * w);
    x->s = take(B * s);
    x->d = take(B * w);
    x->xq = take(B * 4);
    x->pos = (int*)take(x->ntile);
    x->ring_off.assign(L, 0);
    size_t rf = 0;
    for (size_t i = 0; i < L; ++i) {
        x->ring_off[i] = rf;
        rf += (size_t)2 * rate_of(c, (int)i) * B * w;
    }
    x->ring = take(rf);
    return off;
}

int hip_fail(hipError_t e, const char* what) {
    return ast::set_error(AST_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// HWIO rows [kk][M] (input channel, output channel) -> A chunks [M/16][kk/16][64][4]
void pack_chunks(const float* host, int kk, int M, std::vector<float>& out) {
    out.resize((size_t)kk * M);
    const int G = kk / 16;
    for (int m = 0; m < M / 16; ++m)
        for (int g = 0; g < G; ++g)
            for (int ln = 0; ln < 64; ++ln)
                for (int j = 0; j < 4; ++j)
                    out[(((size_t)m * G + g) * 64 + ln) * 4 + j] =
                        host[(size_t)(16 * g + 4 * (ln >> 4) + j) * M + 16 * m + (ln & 15)];
}

int upload_block(float* A, int Gtot, int tile0, int g0, const float* host, int kk, int M) {
    std::vector<float> p;
    pack_chunks(host, kk, M, p);
    const size_t rowb = (size_t)(kk / 16) * 1024;
    const hipError_t e = hipMemcpy2D(A + ((size_t)tile0 * Gtot + g0) * 256, (size_t)Gtot * 1024, p.data(), rowb, rowb,
                                     M / 16, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : hip_fail(e, "ast_dec_set_weight: upload");
}

int upload_vec(float* dst, const float* host, size_t n) {
    const hipError_t e = hipMemcpy(dst, host, n * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : hip_fail(e, "ast_dec_set_weight: upload");
}

// "<base>_<k>/<leaf>" with k in 1..n_layers -> layer k - 1; -1 otherwise
int layer_of(const std::string& name, const char* base, const char* leaf, int n_layers) {
    const std::string pre = std::string(base) + "_";
    const std::string suf = std::string("/") + leaf;
    if (name.size() <= pre.size() + suf.size() || name.compare(0, pre.size(), pre) != 0 ||
        name.compare(name.size() - suf.size(), suf.size(), suf) != 0)
        return -1;
    const std::string num = name.substr(pre.size(), name.size() - pre.size() - suf.size());
    if (num.empty() || num.size() > 3 || num[0] == '0') return -1;
    int k = 0;
    for (char ch : num) {
        if (ch < '0' || ch > '9') return -1;
        k = 10 * k + (ch - '0');
    }
    return k >= 1 && k <= n_layers ? k - 1 : -1;
}

void fill_tables(float* audio, float* xs) {
    // bin -> audio: inv_mu_law_numpy (nsynth/utils.py:122-136) in float64, cast to float32 (the
    // network's placeholder); audio -> next input: mu_law (nsynth/utils.py:70-85) with floor, / 128
    const float inv_log = (float)log(256.0);
    for (int bin = 0; bin < NBIN; ++bin) {
        const double x = (double)(bin - 128);
        double o = (x + 0.5) * 2.0 / 256.0;
        const double sg = o > 0 ? 1.0 : o < 0 ? -1.0 : 0.0;
        o = sg / 255.0 * (pow(256.0, fabs(o)) - 1.0);
        if (x == 0.0) o = x;
        const float a = (float)o;
        audio[bin] = a;
        const float sf = a > 0.f ? 1.f : a < 0.f ? -1.f : 0.f;
        const float ml = sf * logf(1.f + 255.f * fabsf(a)) / inv_log;
        xs[bin] = floorf(ml * 128.f) / 128.f;
    }
}

}  // namespace

namespace ast {
int dec_check_cfg(const ast_dec_cfg* c) { return check_cfg(c); }
}

extern "C" {

int ast_dec_tables(float* audio256, float* xs256) {
    if (!audio256 || !xs256) return ast::set_error(AST_E_ARG, "ast_dec_tables: null argument");
    fill_tables(audio256, xs256);
    return 0;
}

int ast_dec_workspace_bytes(const ast_dec_cfg* cfg, size_t* out) {
    if (!out) return ast::set_error(AST_E_ARG, "ast_dec_workspace_bytes: null argument");
    const int rc = check_cfg(cfg);
    if (rc) return rc;
    ast_dec tmp;
    tmp.c = *cfg;
    *out = carve(&tmp, nullptr);
    return 0;
}

int ast_dec_create(const ast_dec_cfg* cfg, int hip_device, ast_dec** out) {
    if (!out) return ast::set_error(AST_E_ARG, "ast_dec_create: null argument");
    *out = nullptr;
    const int rc = check_cfg(cfg);
    if (rc) return rc;
    hipError_t e = hipSetDevice(hip_device);
    if (e != hipSuccess) return hip_fail(e, "ast_dec_create: hipSetDevice");
    ast_dec* x = new ast_dec();
    x->c = *cfg;
    x->dev = hip_device;
    x->ws_bytes = carve(x, nullptr);
    e = hipMalloc((void**)&x->ws, x->ws_bytes);
    if (e != hipSuccess) {
        delete x;
        return hip_fail(e, "ast_dec_create: hipMalloc");
    }
    carve(x, x->ws);
    float ta[NBIN], tx[NBIN];
    fill_tables(ta, tx);
    // weights start at zero; the rings need no clearing (position test), the state does
    e = hipMemset(x->ws, 0, (size_t)((char*)x->l - x->ws));
    if (e == hipSuccess) e = hipMemcpy(x->tab_audio, ta, sizeof ta, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->tab_xs, tx, sizeof tx, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ast_dec_destroy(x);
        return hip_fail(e, "ast_dec_create: initialisation");
    }
    const int r2 = ast_dec_reset(x, nullptr);
    if (r2 == 0) e = hipDeviceSynchronize();
    if (r2 || e != hipSuccess) {
        ast_dec_destroy(x);
        return r2 ? r2 : hip_fail(e, "ast_dec_create: reset");
    }
    *out = x;
    return 0;
}

void ast_dec_destroy(ast_dec* x) {
    if (!x) return;
    if (x->ws) (void)hipFree(x->ws);
    delete x;
}

int ast_dec_set_weight(ast_dec* x, const char* tf_name, const float* host, size_t n) {
    if (!x || !tf_name || !host) return ast::set_error(AST_E_ARG, "ast_dec_set_weight: null argument");
    const ast_dec_cfg& c = x->c;
    const int w = c.width, s = c.skip_width, L = c.n_layers, Gw = w / 16;
    const std::string nm(tf_name);
    hipError_t e = hipSetDevice(x->dev);
    if (e != hipSuccess) return hip_fail(e, "ast_dec_set_weight: hipSetDevice");
    size_t want = 0;
    int rc = -100;
    int k;
#define DEC_W(count, call)                   \
    {                                        \
        want = (count);                      \
        if (n == want) rc = (call);          \
    }
    if (nm == "startconv/W") DEC_W((size_t)3 * w, upload_vec(x->wstart, host, n))
    else if (nm == "startconv/biases") DEC_W((size_t)w, upload_vec(x->bstart, host, n))
    else if (nm == "skip_start/W") DEC_W((size_t)w * s, upload_block(x->A_skip0, Gw, 0, 0, host, w, s))
    else if (nm == "skip_start/biases") DEC_W((size_t)s, upload_vec(x->bskip0, host, n))
    else if ((k = layer_of(nm, "dilatedconv", "W", L)) >= 0) {
        want = (size_t)3 * w * 2 * w;
        if (n == want) {
            rc = 0;
            for (int tap = 0; tap < 3 && !rc; ++tap)
                rc = upload_block(x->A_gate + (size_t)k * x->gate_sz, 3 * Gw + 1, 0, tap * Gw,
                                  host + (size_t)tap * w * 2 * w, w, 2 * w);
        }
    } else if ((k = layer_of(nm, "dilatedconv", "biases", L)) >= 0)
        DEC_W((size_t)2 * w, upload_vec(x->bdil + (size_t)k * 2 * w, host, n))
    else if ((k = layer_of(nm, "cond_map", "W", L)) >= 0)
        DEC_W((size_t)16 * 2 * w, upload_block(x->A_gate + (size_t)k * x->gate_sz, 3 * Gw + 1, 0, 3 * Gw, host, 16, 2 * w))
    else if ((k = layer_of(nm, "cond_map", "biases", L)) >= 0)
        DEC_W((size_t)2 * w, upload_vec(x->bcond + (size_t)k * 2 * w, host, n))
    else if ((k = layer_of(nm, "res", "W", L)) >= 0)
        DEC_W((size_t)w * w, upload_block(x->A_mix + (size_t)k * x->mix_sz, Gw, 0, 0, host, w, w))
    else if ((k = layer_of(nm, "res", "biases", L)) >= 0)
        DEC_W((size_t)w, upload_vec(x->bres + (size_t)k * w, host, n))
    else if ((k = layer_of(nm, "skip", "W", L)) >= 0)
        DEC_W((size_t)w * s, upload_block(x->A_mix + (size_t)k * x->mix_sz, Gw, Gw, 0, host, w, s))
    else if ((k = layer_of(nm, "skip", "biases", L)) >= 0)
        DEC_W((size_t)s, upload_vec(x->bskip + (size_t)k * s, host, n))
    else if (nm == "out1/W") DEC_W((size_t)s * s, upload_block(x->A1, s / 16 + 1, 0, 0, host, s, s))
    else if (nm == "out1/biases") DEC_W((size_t)s, upload_vec(x->b1, host, n))
    else if (nm == "cond_map_out1/W") DEC_W((size_t)16 * s, upload_block(x->A1, s / 16 + 1, 0, s / 16, host, 16, s))
    else if (nm == "cond_map_out1/biases") DEC_W((size_t)s, upload_vec(x->bc1, host, n))
    else if (nm == "logits/W") DEC_W((size_t)s * NBIN, upload_block(x->A2, s / 16, 0, 0, host, s, NBIN))
    else if (nm == "logits/biases") DEC_W((size_t)NBIN, upload_vec(x->b2, host, n))
    else return ast::set_error(AST_E_NAME, "ast_dec_set_weight: unknown decoder variable " + nm);
#undef DEC_W
    if (rc == -100)
        return ast::set_error(AST_E_NAME, "ast_dec_set_weight: " + nm + " has " + std::to_string(n) +
                                              " elements, the decoder expects " + std::to_string(want));
    return rc;
}

int ast_dec_restore(ast_dec* x, const char* prefix) {
    if (!x || !prefix) return ast::set_error(AST_E_ARG, "ast_dec_restore: null argument");
    try {   // nothing may unwind through the C ABI
        ast::Checkpoint ck;
        std::string err;
        if (ck.open(prefix, &err)) return ast::set_error(AST_E_NAME, err);
        const int64_t w = x->c.width, s = x->c.skip_width;
        typedef std::vector<int64_t> Shape;
        std::vector<std::pair<std::string, Shape>> names = {
            {"startconv", {1, 3, 1, w}}, {"skip_start", {1, 1, w, s}}, {"out1", {1, 1, s, s}},
            {"cond_map_out1", {1, 1, 16, s}}, {"logits", {1, 1, s, NBIN}}};
        for (int l = 1; l <= x->c.n_layers; ++l) {
            const std::string k = "_" + std::to_string(l);
            names.push_back({"dilatedconv" + k, {1, 3, w, 2 * w}});
            names.push_back({"cond_map" + k, {1, 1, 16, 2 * w}});
            names.push_back({"res" + k, {1, 1, w, w}});
            names.push_back({"skip" + k, {1, 1, w, s}});
        }
        std::vector<float> buf;
        for (const auto& nm : names) {
            for (int leaf = 0; leaf < 2; ++leaf) {
                const std::string full = nm.first + (leaf ? "/biases" : "/W");
                const Shape shape = leaf ? Shape{nm.second.back()} : nm.second;
                const ast::CkptEntry* e = ck.find(full);
                if (!e) return ast::set_error(AST_E_NAME, std::string(prefix) + ": no variable " + full +
                                                              " (Saver.restore needs every decoder variable)");
                if (e->shape != shape)
                    return ast::set_error(AST_E_NAME, full + ": the checkpoint's shape is not the decoder's");
                int64_t n = 1;
                for (int64_t d : shape) n *= d;
                buf.resize((size_t)n);
                if (ck.read_f32(*e, buf.data(), &err)) return ast::set_error(AST_E_ARG, err);
                const int rc = ast_dec_set_weight(x, full.c_str(), buf.data(), buf.size());
                if (rc) return rc;
            }
        }
        return 0;
    } catch (const std::exception& ex) {
        return ast::set_error(AST_E_ARG, std::string("ast_dec_restore: ") + ex.what());
    }
}

int ast_dec_reset(ast_dec* x, void* stream) {
    if (!x) return ast::set_error(AST_E_ARG, "ast_dec_reset: null context");
    const int n = x->c.batch * 4;
    k_dec_reset<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(x->pos, x->ntile, x->xq, n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "ast_dec_reset");
}

int ast_dec_position(ast_dec* x, int* out_dev, void* stream) {
    if (!x || !out_dev) return ast::set_error(AST_E_ARG, "ast_dec_position: null argument");
    k_dec_position<<<1, 1, 0, (hipStream_t)stream>>>(x->pos, out_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "ast_dec_position");
}

int ast_dec_step(ast_dec* x, const float* enc_dev, int R, const float* u_dev, const int* force_dev, int total,
                 int* bins_dev, float* audio_dev, float* pmf_dev, void* stream) {
    if (!x || !enc_dev || !u_dev || !bins_dev || !audio_dev)
        return ast::set_error(AST_E_ARG, "ast_dec_step: null argument");
    const ast_dec_cfg& c = x->c;
    if (R < 1 || total < 1 || (long long)total > (long long)R * c.hop)
        return ast::set_error(AST_E_ARG, "ast_dec_step: total " + std::to_string(total) + " must be 1..R*hop = " +
                                             std::to_string((long long)R * c.hop));
    hipStream_t st = (hipStream_t)stream;
    const int B = c.batch, w = c.width, s = c.skip_width, Gw = w / 16;
    const dim3 blk(NW * 64);
    StartArgs sa = {x->A_skip0, x->wstart, x->bstart, x->bskip0, x->xq, x->pos, x->l, x->s, B, w, s, total};
    k_dec_start<<<dim3(s / 16, x->ntile), blk, 0, st>>>(sa);
    for (int i = 0; i < c.n_layers; ++i) {
        const int rate = rate_of(c, i);
        float* ring = x->ring + x->ring_off[i];
        GateArgs ga = {x->A_gate + (size_t)i * x->gate_sz, x->bdil + (size_t)i * 2 * w, x->bcond + (size_t)i * 2 * w,
                       x->l, ring, enc_dev, x->pos, x->d, B, w, rate, R, c.hop, total};
        k_dec_gate<<<dim3(Gw, x->ntile), dim3(NWG * 64), 0, st>>>(ga);
        MixArgs ma = {x->A_mix + (size_t)i * x->mix_sz, x->bres + (size_t)i * w, x->bskip + (size_t)i * s,
                      x->d, x->pos, x->l, x->s, ring, B, w, s, rate, total};
        k_dec_mix<<<dim3(Gw + s / 16, x->ntile), blk, 0, st>>>(ma);
    }
    TailArgs ta = {x->A1, x->b1, x->bc1, x->A2, x->b2, x->s, enc_dev, u_dev, force_dev, x->tab_audio, x->tab_xs,
                   x->pos, x->xq, bins_dev, audio_dev, pmf_dev, B, s, R, c.hop, total};
    const size_t lds = (size_t)(16 * (s + 20) + 16 * (s + 4) + 16 * PST + 16) * 4;
    k_dec_tail<<<dim3(x->ntile), blk, lds, st>>>(ta);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "ast_dec_step");
}

}  // extern "C"
