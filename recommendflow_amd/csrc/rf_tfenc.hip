// rf_tfenc.hip — rf_tfenc_fwd: a stack of TransformerEncoder blocks (backend/layers/network_layers.py:319-352, with
// MultiHeadAttention.call attention_layers.py:153-168, the query-row mask of layer_utils.py:13-19 and FFN :301-316) in
// one launch. Per block, x [L][d] per example:
//   q, k, v = x W + b;  att = softmax_keys(mask(q_h k_h^T / sqrt(depth))) v_h, heads merged
//   out1 = LN(x + att; g1, be1);  x' = LN(out1 + relu(out1 W1 + b1) W2 + b2; g2, be2)
//
// One workgroup owns one example; its waves (ceil(L / 16), at most 8) share the example's K and V in LDS and otherwise
// work alone, each on 16-row tiles. Resident state: K as bf16 [Lr][d + 8] and V transposed as bf16 [d][Lr + 8], Lr = L
// padded to 32. Nothing else lives in LDS: the chain is computed TRANSPOSED, so that each product's accumulator is
// the next product's B operand with no lane movement. The kernel is instantiated per (ND, NJ), d <= 16 ND and
// L <= 32 NJ with ND in {1, 2, 4, 8, 16} and NJ in {1, 2, 4, 8}, so that every register array has static indices;
// tiles between the real size and the instantiated one compute on zeros (weights, x) or on clamped LDS addresses
// (keys past Lr: their logits are -inf) and cost no LDS.
// For v_mfma_f32_16x16x32_bf16 lane l (lr = l & 15, g = l >> 4) holds A[row lr][k = 8 g + e], B[k = 8 g + e][col lr]
// and C[row 4 g + r][col lr]. A pair of accumulator tiles (t0, t1) of a transposed result X^T[c][i] (c on the rows, the
// tile's 16 query rows i on the lanes), rounded to bf16, is the B fragment of one k step of the next product if that
// product's k slot (g, e) means c = 32 s + 16 (e >> 2) + 4 g + (e & 3) ("permuted k"); the other operand is read in
// that order: two 8-byte LDS reads for K and V^T, and images packed in that order for W1 and W2.
//   phase A  per 16-key tile: K^T = Wk^T x^T (A = Wk image, B = x fragment) -> LDS K [j][c], 8-byte writes;
//            V = x Wv (A = the same x fragment, B = Wv image) -> LDS V^T [c][j], 8-byte writes. Keys padded in beyond
//            L get k = bk, v = bv (finite); they never enter a softmax (logit -inf, probability exactly 0).
//   phase B  per 16-row tile and head: Q^T = Wq^T x^T two tiles at a time -> the B fragment of S^T = K Q^T (all key
//            tiles in accumulators: 64 VGPRs at L 256); scale, mask replacement and softmax over the keys in fp32 (keys
//            in the registers and across g: a register sum, then xor-shuffles 16, 32); P^T -> B fragments;
//            att^T = V^T P^T per 16 columns, + x, written to the tile's own rows of out (fp32). After the heads the
//            lane reads its own values back (the residual row has to be whole for the LayerNorm statistics, and an
//            accumulator array indexed by a runtime head would go to scratch), LN1 -> out1 (fp32 in registers, bf16
//            fragments), h^T = relu(W1^T out1^T + b1) 32 hidden units at a time -> B fragment of y^T += W2^T h^T,
//            + b2 + out1, LN2, store.
// Blocks after the first read their input from out (the tile rows a wave reads in phase B are the rows it then
// writes; phase A of the next block starts after a workgroup barrier). Weights and the fp32 vectors come from the
// packed image (L2): [Wq | Wk | Wv | W1 | W2] as [16-column tile][k step][lane][8 bf16] (a fragment is one 16-byte
// load), then bq bk bv b2 g1 be1 g2 be2 [dp] and b1 [fp = ffn padded to 32] in fp32, zero in every padding.
//
// Precision: every MFMA operand is an fp32 value rounded once (RNE) to bf16: x, the weights, q k v after the bias, the
// softmax probabilities, out1 as the FFN's input, relu(.) as W2's input. Accumulation is fp32. The scale, the mask
// replacement, the softmax (max subtracted), the residual stream (x, x + att, out1 + ffn), the LayerNorm statistics
// (biased variance) and out are fp32. Deterministic: no atomics, fixed reduction orders.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rf_common.h"
#include "rf_wave.h"

namespace {

constexpr int kTfMaxL = 256, kTfMaxD = 256, kTfMaxFfn = 1024, kTfMaxBlocks = 8, kTfMaxWaves = 8;
constexpr size_t kTfMaxLds = 160 * 1024;

struct TfPlan {
    int L, d, heads, depth, ffn;
    int ND, NJ;      // the instantiation: d <= dp = 16 ND, L <= 32 NJ
    int dp, Lr, fp;  // Lr = L padded to 32 (the key rows held in LDS), fp = ffn padded to 32
    int KS;          // k steps of 32 over dp
    int pK, pV;      // LDS pitches in bf16 elements: d + 8, Lr + 8
    // one block's image, offsets in bytes
    int64_t oWq, oWk, oWv, oW1, oW2, oVec, block_bytes;
};

inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the image's shape depends on d_model and ffn_hidden only
bool tf_plan_image(int d, int ffn, TfPlan& p, const char* who) {
    if (d < 16 || d > kTfMaxD || d % 16) {
        rf_set_error(RF_EINVAL, "%s: d_model (%d) must be a multiple of 16 in [16, %d]", who, d, kTfMaxD);
        return false;
    }
    if (ffn < 16 || ffn > kTfMaxFfn || ffn % 16) {
        rf_set_error(RF_EINVAL, "%s: ffn_hidden (%d) must be a multiple of 16 in [16, %d]", who, ffn, kTfMaxFfn);
        return false;
    }
    p.d = d;
    p.ffn = ffn;
    p.ND = pow2_at_least(d / 16);
    p.dp = 16 * p.ND;
    p.KS = (p.ND + 1) / 2;
    p.fp = (ffn + 31) / 32 * 32;
    const int64_t frag = 64 * 16;  // bytes of one (tile, k step)
    p.oWq = 0;
    p.oWk = p.oWq + (int64_t)p.ND * p.KS * frag;
    p.oWv = p.oWk + (int64_t)p.ND * p.KS * frag;
    p.oW1 = p.oWv + (int64_t)p.ND * p.KS * frag;
    p.oW2 = p.oW1 + (int64_t)(p.fp / 16) * p.KS * frag;
    p.oVec = p.oW2 + (int64_t)p.ND * (p.fp / 32) * frag;
    p.block_bytes = p.oVec + (int64_t)(8 * p.dp + p.fp) * 4;  // a multiple of 16
    return true;
}

bool tf_plan(int L, int d, int heads, int ffn, TfPlan& p, const char* who) {
    if (!tf_plan_image(d, ffn, p, who)) return false;
    if (L < 1 || L > kTfMaxL) {
        rf_set_error(RF_EINVAL, "%s: L (%d) must be in [1, %d]", who, L, kTfMaxL);
        return false;
    }
    if (heads < 1 || d % heads || (d / heads) % 16) {
        rf_set_error(RF_EINVAL, "%s: heads (%d) must divide d_model (%d) with a depth that is a multiple of 16", who, heads, d);
        return false;
    }
    p.L = L;
    p.heads = heads;
    p.depth = d / heads;
    p.NJ = pow2_at_least((L + 31) / 32);
    p.Lr = (L + 31) / 32 * 32;
    p.pK = d + 8;
    p.pV = p.Lr + 8;
    return true;
}

inline size_t tf_lds_bytes(const TfPlan& p) { return ((size_t)p.Lr * p.pK + (size_t)p.d * p.pV) * 2; }

struct TfPackArgs {
    const float *Wq, *bq, *Wk, *bk, *Wv, *bv, *g1, *be1, *W1, *b1, *W2, *b2, *g2, *be2;
    char* img;  // this block's image
    TfPlan p;
};

// one thread per 16-byte fragment element or per fp32 vector element
__global__ __launch_bounds__(256) void tfenc_pack_kernel(const TfPackArgs a) {
    const TfPlan& p = a.p;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nfrag = p.oVec / 16;
    if (t < nfrag) {
        const int64_t byte = t * 16;
        const float* W;
        int64_t base;
        int Kd, Nd, steps;
        bool perm;
        if (byte < p.oWk) { W = a.Wq; base = p.oWq; Kd = p.d; Nd = p.d; steps = p.KS; perm = false; }
        else if (byte < p.oWv) { W = a.Wk; base = p.oWk; Kd = p.d; Nd = p.d; steps = p.KS; perm = false; }
        else if (byte < p.oW1) { W = a.Wv; base = p.oWv; Kd = p.d; Nd = p.d; steps = p.KS; perm = false; }
        else if (byte < p.oW2) { W = a.W1; base = p.oW1; Kd = p.d; Nd = p.ffn; steps = p.KS; perm = true; }
        else { W = a.W2; base = p.oW2; Kd = p.ffn; Nd = p.d; steps = p.fp / 32; perm = true; }
        const int64_t q = t - base / 16;
        const int lane = (int)(q & 63);
        const int s = (int)((q >> 6) % steps), tile = (int)((q >> 6) / steps);
        const int lr = lane & 15, g = lane >> 4;
        const int n = 16 * tile + lr;
        uint32_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = perm ? 32 * s + 16 * (e >> 2) + 4 * g + (e & 3) : 32 * s + 8 * g + e;
            const float v = k < Kd && n < Nd ? W[(int64_t)k * Nd + n] : 0.f;
            h[e] = f32_to_bf16_bits(v);
        }
        reinterpret_cast<uint4*>(a.img)[t] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        return;
    }
    const int64_t v = t - nfrag;
    if (v >= 8 * p.dp + p.fp) return;
    float* vec = reinterpret_cast<float*>(a.img + p.oVec);
    if (v < 8 * p.dp) {
        const float* src[8] = {a.bq, a.bk, a.bv, a.b2, a.g1, a.be1, a.g2, a.be2};
        const int which = (int)(v / p.dp), c = (int)(v % p.dp);
        float val = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w)
            if (w == which && c < p.d) val = src[w][c];
        vec[v] = val;
    } else {
        const int f = (int)(v - 8 * p.dp);
        vec[v] = f < p.ffn ? a.b1[f] : 0.f;
    }
}

struct TfArgs {
    const void* x;
    int x_bf16, x_vec;  // x_vec: the 16-byte (f32) / 8- and 16-byte (bf16) loads of x are aligned
    int64_t xsb, xsl;
    const float* mask;
    float* out;
    int o_vec;
    int64_t osb, osl;
    const char* img;
    int n_blocks;
    float eps, scale;
    TfPlan p;
};

// the input of one block: x for the first, out for the rest
struct TfIn {
    const char* base;  // the example
    int64_t sl;        // elements
    bool bf16, vec;
};

// 8 consecutive elements of a row as a bf16 fragment (c0 a multiple of 8, d a multiple of 16: all or nothing)
__device__ __forceinline__ bf16x8 tf_ld8(const TfIn& in, int row, int c0, bool live) {
    bf16x8 f;
    if (!live) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (__bf16)0.f;
        return f;
    }
    if (in.bf16) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(in.base) + (int64_t)row * in.sl + c0;
        if (in.vec) return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p));
        uint16_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = p[e];
        uint4 u = make_uint4(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16), h[4] | ((uint32_t)h[5] << 16),
                             h[6] | ((uint32_t)h[7] << 16));
        return __builtin_bit_cast(bf16x8, u);
    }
    const float* p = reinterpret_cast<const float*>(in.base) + (int64_t)row * in.sl + c0;
    float v[8];
    if (in.vec) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (__bf16)v[e];
    return f;
}

// 4 consecutive elements of a row in fp32
__device__ __forceinline__ f32x4 tf_ld4(const TfIn& in, int row, int c0) {
    f32x4 r;
    if (in.bf16) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(in.base) + (int64_t)row * in.sl + c0;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = bf16_bits_to_f32(p[e]);
        return r;
    }
    const float* p = reinterpret_cast<const float*>(in.base) + (int64_t)row * in.sl + c0;
    if (in.vec) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = p[e];
    return r;
}

__device__ __forceinline__ void tf_st4(float* p, bool vec, f32x4 v) {
    if (vec) {
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = v[e];
    }
}

// LayerNorm over the d columns of each row of a transposed tile set r[t][e] = R[row lr][c = 16 t + 4 g + e]
template <int ND>
__device__ __forceinline__ void tf_layernorm(f32x4 (&r)[ND], int d, float eps, const float* gamma, const float* beta, int g) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < ND; ++t)
        if (16 * t < d) s += (r[t][0] + r[t][1]) + (r[t][2] + r[t][3]);
    const float mean = rows4_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < ND; ++t)
        if (16 * t < d) {
            const float a = r[t][0] - mean, b = r[t][1] - mean, c = r[t][2] - mean, e = r[t][3] - mean;
            q += (a * a + b * b) + (c * c + e * e);
        }
    const float inv = 1.f / sqrtf(rows4_sum(q) / (float)d + eps);
#pragma unroll
    for (int t = 0; t < ND; ++t) {
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + 16 * t + 4 * g);
        const f32x4 be = *reinterpret_cast<const f32x4*>(beta + 16 * t + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[t][e] = 16 * t < d ? (r[t][e] - mean) * inv * ga[e] + be[e] : 0.f;
    }
}

template <int ND, int NJ>
__global__ __launch_bounds__(64 * kTfMaxWaves) void tfenc_kernel(const TfArgs a) {
    constexpr int KS = (ND + 1) / 2, NT2 = 2 * NJ;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TfPlan& p = a.p;
    uint16_t* Kl = reinterpret_cast<uint16_t*>(smem);  // [Lr][pK]
    uint16_t* Vl = Kl + (size_t)p.Lr * p.pK;           // [d][pV]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int64_t b = blockIdx.x;
    const int L = p.L, d = p.d, Lr = p.Lr, pK = p.pK, pV = p.pV;
    const int ntile = (L + 15) / 16, nt = p.depth / 16;
    float* outb = a.out + b * a.osb;

    for (int blk = 0; blk < a.n_blocks; ++blk) {
        TfIn in;
        if (blk == 0) {
            in.base = static_cast<const char*>(a.x) + b * a.xsb * (a.x_bf16 ? 2 : 4);
            in.sl = a.xsl;
            in.bf16 = a.x_bf16 != 0;
            in.vec = a.x_vec != 0;
        } else {
            in.base = reinterpret_cast<const char*>(outb);
            in.sl = a.osl;
            in.bf16 = false;
            in.vec = a.o_vec != 0;
        }
        const char* img = a.img + (int64_t)blk * p.block_bytes;
        const uint4* Wq = reinterpret_cast<const uint4*>(img + p.oWq);
        const uint4* Wk = reinterpret_cast<const uint4*>(img + p.oWk);
        const uint4* Wv = reinterpret_cast<const uint4*>(img + p.oWv);
        const uint4* W1 = reinterpret_cast<const uint4*>(img + p.oW1);
        const uint4* W2 = reinterpret_cast<const uint4*>(img + p.oW2);
        const float* vec = reinterpret_cast<const float*>(img + p.oVec);
        const float *bq = vec, *bk = vec + p.dp, *bv = vec + 2 * p.dp, *b2 = vec + 3 * p.dp, *g1 = vec + 4 * p.dp,
                    *be1 = vec + 5 * p.dp, *g2 = vec + 6 * p.dp, *be2 = vec + 7 * p.dp, *b1 = vec + 8 * p.dp;

        // ---- phase A: K and V^T of every key tile up to Lr (the padded rows too: LDS must hold finite values) ----
        for (int jt = wave; 16 * jt < Lr; jt += nw) {
            const int j = 16 * jt + lr;
            bf16x8 xf[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) xf[s] = tf_ld8(in, j, 32 * s + 8 * g, j < L && 32 * s + 8 * g < d);
            for (int ct = 0; 16 * ct < d; ++ct) {
                f32x4 ak = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const bf16x8 wk = __builtin_bit_cast(bf16x8, Wk[(ct * KS + s) * 64 + lane]);
                    const bf16x8 wv = __builtin_bit_cast(bf16x8, Wv[(ct * KS + s) * 64 + lane]);
                    ak = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wk, xf[s], ak, 0, 0, 0);  // K^T[c = 4 g + r][j = lr]
                    av = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[s], wv, av, 0, 0, 0);  // V[j = 4 g + r][c = lr]
                }
                const f32x4 kb = *reinterpret_cast<const f32x4*>(bk + 16 * ct + 4 * g);
                const float vb = bv[16 * ct + lr];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ak[e] += kb[e];
                    av[e] += vb;
                }
                *reinterpret_cast<uint2*>(Kl + (size_t)j * pK + 16 * ct + 4 * g) = bf16_pack4(ak);
                *reinterpret_cast<uint2*>(Vl + (size_t)(16 * ct + lr) * pV + 16 * jt + 4 * g) = bf16_pack4(av);
            }
        }
        __syncthreads();

        // ---- phase B: one 16-row tile per wave and pass ----
        for (int it = wave; it < ntile; it += nw) {
            const int i = 16 * it + lr;
            const bool live = i < L;
            float* orow = outb + (int64_t)i * a.osl;
            bf16x8 xf[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) xf[s] = tf_ld8(in, i, 32 * s + 8 * g, live && 32 * s + 8 * g < d);
            const bool masked = a.mask != nullptr && live && a.mask[b * L + i] == 0.f;

            for (int h = 0; h < p.heads; ++h) {
                const int c0 = h * p.depth;
                f32x4 S[NT2];
#pragma unroll
                for (int jt = 0; jt < NT2; ++jt) S[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int s2 = 0; 2 * s2 < nt; ++s2) {
                    // two tiles of Q^T: the B fragment of one k step of S^T = K Q^T
                    const bool two = 2 * s2 + 1 < nt;
                    const int T0 = h * nt + 2 * s2, T1 = two ? T0 + 1 : T0;
                    f32x4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const bf16x8 w0 = __builtin_bit_cast(bf16x8, Wq[(T0 * KS + s) * 64 + lane]);
                        const bf16x8 w1 = __builtin_bit_cast(bf16x8, Wq[(T1 * KS + s) * 64 + lane]);
                        q0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, xf[s], q0, 0, 0, 0);
                        q1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, xf[s], q1, 0, 0, 0);
                    }
                    const f32x4 qb0 = *reinterpret_cast<const f32x4*>(bq + 16 * T0 + 4 * g);
                    const f32x4 qb1 = *reinterpret_cast<const f32x4*>(bq + 16 * T1 + 4 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        q0[e] += qb0[e];
                        q1[e] = two ? q1[e] + qb1[e] : 0.f;
                    }
                    const bf16x8 qf = bf16_join(bf16_pack4(q0), bf16_pack4(q1));
                    const uint16_t* kcol = Kl + c0 + 32 * s2 + 4 * g;
                    const int hi = two ? 16 : 0;  // one tile: the upper half of the step multiplies zeros
#pragma unroll
                    for (int jt = 0; jt < NT2; ++jt) {
                        const uint16_t* kp = kcol + (size_t)min(16 * jt + lr, Lr - 1) * pK;  // past Lr: any row, logit -inf
                        const bf16x8 kf = bf16_join(*reinterpret_cast<const uint2*>(kp), *reinterpret_cast<const uint2*>(kp + hi));
                        S[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, S[jt], 0, 0, 0);  // S^T[j = 4 g + r][i = lr]
                    }
                }
                // softmax over the keys of query row i: fp32, max subtracted; a masked row is uniform over the L keys
                float m = -INFINITY;
#pragma unroll
                for (int jt = 0; jt < NT2; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float l = masked ? -4294967295.f : S[jt][r] * a.scale;
                        if (16 * jt + 4 * g + r >= L) l = -INFINITY;
                        S[jt][r] = l;
                        m = fmaxf(m, l);
                    }
                m = rows4_max(m);
                float sum = 0.f;
#pragma unroll
                for (int jt = 0; jt < NT2; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        S[jt][r] = __expf(S[jt][r] - m);
                        sum += S[jt][r];
                    }
                const float inv = 1.f / rows4_sum(sum);
                bf16x8 P[NJ];
#pragma unroll
                for (int s = 0; s < NJ; ++s) {
                    f32x4 lo, hi;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        lo[r] = S[2 * s][r] * inv;
                        hi[r] = S[2 * s + 1][r] * inv;
                    }
                    P[s] = bf16_join(bf16_pack4(lo), bf16_pack4(hi));
                }
                // att^T = V^T P^T per 16 columns of the head, + x, to the tile's rows of out
                for (int tt = 0; tt < nt; ++tt) {
                    const int T = h * nt + tt;
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    const uint16_t* vp = Vl + (size_t)(16 * T + lr) * pV + 4 * g;
#pragma unroll
                    for (int s = 0; s < NJ; ++s) {
                        const int j0 = 32 * s < Lr ? 32 * s : 0;  // past Lr: P is exactly zero, any finite v
                        const bf16x8 vf = bf16_join(*reinterpret_cast<const uint2*>(vp + j0),
                                                  *reinterpret_cast<const uint2*>(vp + j0 + 16));
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, P[s], acc, 0, 0, 0);  // att^T[c = 4 g + r][i = lr]
                    }
                    if (live) {
                        const f32x4 xr = tf_ld4(in, i, 16 * T + 4 * g);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = xr[e] + acc[e];
                        tf_st4(orow + 16 * T + 4 * g, a.o_vec != 0, acc);
                    }
                }
            }

            // the residual rows back (each lane its own values), LayerNorm 1
            f32x4 o1[ND];
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                o1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (16 * t < d && live) {
                    if (a.o_vec) {
                        o1[t] = *reinterpret_cast<const f32x4*>(orow + 16 * t + 4 * g);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o1[t][e] = orow[16 * t + 4 * g + e];
                    }
                }
            }
            tf_layernorm<ND>(o1, d, a.eps, g1, be1, g);
            bf16x8 of[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                uint2 hi2 = make_uint2(0u, 0u);
                if constexpr (ND > 1) hi2 = bf16_pack4(o1[2 * s + (ND > 1 ? 1 : 0)]);
                of[s] = bf16_join(bf16_pack4(o1[2 * s]), hi2);
            }
            // FFN, 32 hidden units at a time
            f32x4 y[ND];
#pragma unroll
            for (int t = 0; t < ND; ++t) y[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int nfs = p.fp / 32;
            for (int fs = 0; fs < nfs; ++fs) {
                f32x4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const bf16x8 w0 = __builtin_bit_cast(bf16x8, W1[((2 * fs) * KS + s) * 64 + lane]);
                    const bf16x8 w1 = __builtin_bit_cast(bf16x8, W1[((2 * fs + 1) * KS + s) * 64 + lane]);
                    h0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, of[s], h0, 0, 0, 0);  // h^T[f = 4 g + r][i = lr]
                    h1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, of[s], h1, 0, 0, 0);
                }
                const f32x4 hb0 = *reinterpret_cast<const f32x4*>(b1 + 32 * fs + 4 * g);
                const f32x4 hb1 = *reinterpret_cast<const f32x4*>(b1 + 32 * fs + 16 + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    h0[e] = fmaxf(h0[e] + hb0[e], 0.f);
                    h1[e] = fmaxf(h1[e] + hb1[e], 0.f);
                }
                const bf16x8 hf = bf16_join(bf16_pack4(h0), bf16_pack4(h1));
#pragma unroll
                for (int t = 0; t < ND; ++t) {
                    const bf16x8 w2 = __builtin_bit_cast(bf16x8, W2[(t * nfs + fs) * 64 + lane]);
                    y[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, hf, y[t], 0, 0, 0);  // y^T[c = 4 g + r][i = lr]
                }
            }
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                const f32x4 yb = *reinterpret_cast<const f32x4*>(b2 + 16 * t + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[t][e] = o1[t][e] + (y[t][e] + yb[e]);
            }
            tf_layernorm<ND>(y, d, a.eps, g2, be2, g);
            if (live) {
#pragma unroll
                for (int t = 0; t < ND; ++t)
                    if (16 * t < d) tf_st4(orow + 16 * t + 4 * g, a.o_vec != 0, y[t]);
            }
        }
        __syncthreads();  // the next block's phase A reads out and overwrites K, V
    }
}

template <int ND, int NJ>
int launch_tfenc(const TfArgs& a, int batch, int waves, size_t lds, hipStream_t st) {
    auto kern = tfenc_kernel<ND, NJ>;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return rf_set_error(RF_EHIP, "rf_tfenc_fwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(64 * waves), lds, st, a);
    return RF_OK;
}

template <int ND>
int launch_tfenc_nj(const TfArgs& a, int batch, int waves, size_t lds, hipStream_t st) {
    switch (a.p.NJ) {
        case 1: return launch_tfenc<ND, 1>(a, batch, waves, lds, st);
        case 2: return launch_tfenc<ND, 2>(a, batch, waves, lds, st);
        case 4: return launch_tfenc<ND, 4>(a, batch, waves, lds, st);
        default: return launch_tfenc<ND, 8>(a, batch, waves, lds, st);
    }
}

}  // namespace

extern "C" size_t rf_tfenc_packed_bytes(int32_t d_model, int32_t ffn_hidden, int32_t n_blocks) {
    TfPlan p;
    if (!tf_plan_image(d_model, ffn_hidden, p, "rf_tfenc_packed_bytes")) return 0;
    if (n_blocks < 1 || n_blocks > kTfMaxBlocks) {
        rf_set_error(RF_EINVAL, "rf_tfenc_packed_bytes: n_blocks (%d) must be in [1, %d]", n_blocks, kTfMaxBlocks);
        return 0;
    }
    return (size_t)p.block_bytes * n_blocks;
}

extern "C" size_t rf_tfenc_lds_bytes(int32_t L, int32_t d_model, int32_t heads, int32_t ffn_hidden) {
    TfPlan p;
    if (!tf_plan(L, d_model, heads, ffn_hidden, p, "rf_tfenc_lds_bytes")) return 0;
    const size_t lds = tf_lds_bytes(p);
    if (lds > kTfMaxLds) {
        rf_set_error(RF_EINVAL, "rf_tfenc_lds_bytes: needs %zu bytes of LDS (> 160 KiB)", lds);
        return 0;
    }
    return lds;
}

extern "C" int rf_tfenc_pack(int32_t block, int32_t d_model, int32_t ffn_hidden, int32_t n_blocks, const float* Wq,
                             const float* bq, const float* Wk, const float* bk, const float* Wv, const float* bv,
                             const float* gamma1, const float* beta1, const float* W1, const float* b1, const float* W2,
                             const float* b2, const float* gamma2, const float* beta2, void* packed, void* stream) {
    TfPackArgs a;
    if (!tf_plan_image(d_model, ffn_hidden, a.p, "rf_tfenc_pack")) return RF_EINVAL;
    RF_REQUIRE(n_blocks >= 1 && n_blocks <= kTfMaxBlocks, "rf_tfenc_pack: n_blocks (%d) must be in [1, %d]", n_blocks, kTfMaxBlocks);
    RF_REQUIRE(block >= 0 && block < n_blocks, "rf_tfenc_pack: block (%d) must be in [0, %d)", block, n_blocks);
    RF_REQUIRE(Wq && bq && Wk && bk && Wv && bv && gamma1 && beta1 && W1 && b1 && W2 && b2 && gamma2 && beta2,
               "rf_tfenc_pack: null parameter pointer");
    RF_REQUIRE(packed && ((uintptr_t)packed & 15) == 0, "rf_tfenc_pack: packed is null or not 16-byte aligned");
    a.Wq = Wq; a.bq = bq; a.Wk = Wk; a.bk = bk; a.Wv = Wv; a.bv = bv; a.g1 = gamma1; a.be1 = beta1;
    a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.g2 = gamma2; a.be2 = beta2;
    a.img = static_cast<char*>(packed) + (int64_t)block * a.p.block_bytes;
    a.p.L = a.p.heads = a.p.depth = a.p.NJ = a.p.Lr = a.p.pK = a.p.pV = 0;
    const int64_t total = a.p.oVec / 16 + 8 * a.p.dp + a.p.fp;
    hipLaunchKernelGGL(tfenc_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, rf_stream(stream), a);
    return rf_check_launch("rf_tfenc_pack");
}

extern "C" int rf_tfenc_fwd(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t x_stride_l, const float* mask,
                            int32_t batch, int32_t L, int32_t d_model, int32_t heads, int32_t ffn_hidden, int32_t n_blocks,
                            const void* packed, float eps, float* out, int64_t out_stride_b, int64_t out_stride_l,
                            void* stream) {
    TfArgs a;
    if (!tf_plan(L, d_model, heads, ffn_hidden, a.p, "rf_tfenc_fwd")) return RF_EINVAL;
    RF_REQUIRE(n_blocks >= 1 && n_blocks <= kTfMaxBlocks, "rf_tfenc_fwd: n_blocks (%d) must be in [1, %d]", n_blocks, kTfMaxBlocks);
    RF_REQUIRE(batch >= 0, "rf_tfenc_fwd: batch must be >= 0");
    RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_tfenc_fwd: x_dtype must be F32 or BF16");
    RF_REQUIRE(x_stride_l >= d_model && x_stride_b >= 0, "rf_tfenc_fwd: x_stride_l must be >= d_model and x_stride_b >= 0");
    RF_REQUIRE(out_stride_l >= d_model && out_stride_b >= (int64_t)(L - 1) * out_stride_l + d_model,
               "rf_tfenc_fwd: out_stride_l must be >= d_model and out_stride_b >= (L - 1) * out_stride_l + d_model");
    RF_REQUIRE(eps >= 0.f && std::isfinite(eps), "rf_tfenc_fwd: eps must be finite and >= 0");
    const size_t lds = tf_lds_bytes(a.p);
    RF_REQUIRE(lds <= kTfMaxLds, "rf_tfenc_fwd: needs %zu bytes of LDS (> 160 KiB)", lds);
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && packed && out, "rf_tfenc_fwd: null pointer");
    RF_REQUIRE(((uintptr_t)packed & 15) == 0, "rf_tfenc_fwd: packed must be 16-byte aligned");
    a.x = x;
    a.x_bf16 = x_dtype == RF_DTYPE_BF16;
    a.xsb = x_stride_b;
    a.xsl = x_stride_l;
    const int xal = a.x_bf16 ? 8 : 4;  // elements per 16 bytes
    a.x_vec = ((uintptr_t)x & 15) == 0 && x_stride_b % xal == 0 && x_stride_l % xal == 0;
    a.mask = mask;
    a.out = out;
    a.osb = out_stride_b;
    a.osl = out_stride_l;
    a.o_vec = ((uintptr_t)out & 15) == 0 && out_stride_b % 4 == 0 && out_stride_l % 4 == 0;
    a.img = static_cast<const char*>(packed);
    a.n_blocks = n_blocks;
    a.eps = eps;
    a.scale = 1.f / sqrtf((float)a.p.depth);
    const int waves = std::min(kTfMaxWaves, (L + 15) / 16);
    hipStream_t st = rf_stream(stream);
    int rc;
    switch (a.p.ND) {
        case 1: rc = launch_tfenc_nj<1>(a, batch, waves, lds, st); break;
        case 2: rc = launch_tfenc_nj<2>(a, batch, waves, lds, st); break;
        case 4: rc = launch_tfenc_nj<4>(a, batch, waves, lds, st); break;
        case 8: rc = launch_tfenc_nj<8>(a, batch, waves, lds, st); break;
        default: rc = launch_tfenc_nj<16>(a, batch, waves, lds, st); break;
    }
    if (rc != RF_OK) return rc;
    return rf_check_launch("rf_tfenc_fwd");
}
