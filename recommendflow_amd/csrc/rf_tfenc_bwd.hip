// rf_tfenc_bwd.hip — rf_tfenc_bwd: the backward of rf_tfenc_fwd's stack of TransformerEncoder blocks (rf_tfenc.hip; the
// notation of its header, r1 = x + att, r2 = out1 + ffn). Recompute, as rf_cin_bwd does: the forward saves nothing.
//
//   1. x -> fp32 [B L][d] (exact for bf16), then rf_tfenc_fwd itself, one block per launch, leaves the fp32 input of
//      every block in the workspace (the same instantiations, the same bits as the stack in one launch: a block after
//      the first reads fp32 rows either way). The last block's forward is not run.
//   2. Per block from the last to the first, every arrow of the chain is a [B L][d] or [B L][ffn] tensor in the
//      workspace (fp32 where it is a residual or a LayerNorm operand, bf16 where it is only an MFMA operand):
//        tfb_rowgemm   out[row][n] = sum_k A[row][k] Wt[n][k] (+ bias, relu / gate / residual): a wave owns 16 rows x 64
//                      columns; both fragments are 16-byte global loads (A = the weight rows, B = the activation rows, so
//                      a lane ends with 4 consecutive columns of one row). q k v, pre -> h, ffn -> r2, dh, d_out1, dx.
//        tfb_transpose bf16 copies [B][cols][Lp] (Lp = L padded to 32, zeros in the padding) of q k v and datt: the
//                      operands whose contraction runs over the rows of an example.
//        tfb_attn<NJ, 0>  query-stationary: S^T = K Q^T (all key tiles in accumulators), softmax, att^T = V^T P^T -> r1.
//        tfb_attn<NJ, 1>  query-stationary: S^T and dP^T = V datt^T again, P (fp32, unrounded), delta = rowsum(dP P),
//                         dS = P (dP - delta), dq^T = K^T dS^T / sqrt(depth); leaves max, 1 / sum and delta per row.
//        tfb_attn<NJ, 2>  key-stationary: S = Q K^T and dP = datt V^T with the key on the lanes, P and dS from the row
//                         scalars, dv^T = datt^T P, dk^T = Q^T dS / sqrt(depth). All queries of an example pass through one
//                         wave: no sum across waves. A masked query row has P = 1 / L and dS = 0 exactly; keys and
//                         queries past L have P = dS = 0 exactly.
//                      In all three the accumulators of the first products, rounded, are the B fragments of the second
//                      ("permuted k" as in rf_tfenc.hip); the A fragments are two 8-byte loads of a transposed copy.
//        tfb_ln_fwd / tfb_ln_bwd  one wave per row, fp32.
//        tfb_dw        C[M][N] = sum_rows A[row][M] B[row][N] over row chunks (length from B L only), both operands
//                      staged transposed in LDS as bf16; tfb_reduce adds the chunk partials in chunk order.
//        tfb_colsum    the vector gradients: fp32 column sums over 512 rows per workgroup (four row phases, each in row
//                      order, added in order), then tfb_vreduce over the partials in a fixed order.
//   No atomics; every reduction has a fixed order: two launches give the same bits.
//
// Precision: every MFMA operand is an fp32 value rounded once (RNE) to bf16: the recomputed forward operands at the
// forward's rounding points (x, the weights, q k v after the bias, P, out1, relu(.)), and dr2, dh, datt, dS / sqrt(depth),
// dq, dk, dv and the transposed weights. Accumulation is fp32. Both LayerNorm backwards, the softmax backward on the
// unrounded P, the residual gradient stream (dy, dr2 + dh W1^T, dr1 + the projections), dx and every parameter gradient
// are fp32; db1 and dbq / dbk / dbv sum the rounded dh and dq / dk / dv (the values the weight gradients contract).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rf_common.h"
#include "rf_wave.h"

namespace {

constexpr int kTbChunks = 64;          // at most this many row chunks ...
constexpr int64_t kTbMinChunk = 1024;  // ... of at least this many rows
constexpr int kTbMaxBlocks = 8;
constexpr int64_t kTbSumRows = 512;     // rows of one column-sum partial

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

struct TbPlan {
    int64_t B, R;  // R = B L rows
    int L, Lp, d, heads, depth, ffn, nb, NJ;
    int dp, fp;                  // the forward image's paddings
    int64_t oVec, block_bytes;   // the forward image: offset of the fp32 vectors, bytes of one block
    int64_t pt_block;            // bytes of one block of the transposed image
    int64_t chunk;
    int nchunks;
    int nsub;  // column-sum partials: ceil(R / kTbSumRows)
    size_t o_xin, o_qkv, o_qkvT, o_r1, o_out1, o_h, o_r2, o_dy[2], o_dr2, o_gc, o_dh, o_dr1, o_dattT, o_datt, o_dqkv, o_stats,
        o_slab, o_vslab, total;
};

// bf16 elements of one block of the transposed image: [WqkvT | Wcat | W1T | W1 | W2T | W2]
struct TbImg {
    int64_t oQkvT, oCat, oW1T, oW1, oW2T, oW2, elems;
};
inline TbImg tb_img(int d, int ffn) {
    TbImg g;
    g.oQkvT = 0;
    g.oCat = g.oQkvT + 3ll * d * d;
    g.oW1T = g.oCat + 3ll * d * d;
    g.oW1 = g.oW1T + (int64_t)d * ffn;
    g.oW2T = g.oW1 + (int64_t)d * ffn;
    g.oW2 = g.oW2T + (int64_t)d * ffn;
    g.elems = g.oW2 + (int64_t)d * ffn;
    return g;
}

// the forward's limits and messages (rf_tfenc.hip), then the workspace. false with the error set.
bool tb_plan(int64_t batch, int L, int d, int heads, int ffn, int nb, TbPlan& p) {
    if (rf_tfenc_lds_bytes(L, d, heads, ffn) == 0) return false;
    const size_t one = rf_tfenc_packed_bytes(d, ffn, 1);
    if (one == 0 || rf_tfenc_packed_bytes(d, ffn, nb) == 0) return false;
    p.B = batch; p.L = L; p.d = d; p.heads = heads; p.depth = d / heads; p.ffn = ffn; p.nb = nb;
    p.R = batch * L;
    p.Lp = (L + 31) / 32 * 32;
    int nj = 1;
    while (32 * nj < L) nj <<= 1;
    p.NJ = nj;
    int nd = 1;
    while (16 * nd < d) nd <<= 1;
    p.dp = 16 * nd;
    p.fp = (ffn + 31) / 32 * 32;
    p.block_bytes = (int64_t)one;
    p.oVec = p.block_bytes - (int64_t)(8 * p.dp + p.fp) * 4;  // the vectors end the block's image
    p.pt_block = tb_img(d, ffn).elems * 2;
    p.chunk = std::max<int64_t>(kTbMinChunk, ((p.R + kTbChunks - 1) / kTbChunks + 31) / 32 * 32);
    p.nchunks = (int)std::max<int64_t>(1, (p.R + p.chunk - 1) / p.chunk);
    const size_t R = (size_t)std::max<int64_t>(p.R, 1), Bn = (size_t)std::max<int64_t>(batch, 1);
    const size_t rd4 = al256(R * d * 4);
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += al256(n); return o; };
    p.o_xin = take(rd4 * nb);
    p.o_qkv = take(R * 3 * d * 2);
    p.o_qkvT = take(Bn * 3 * d * p.Lp * 2);
    p.o_r1 = take(rd4);
    p.o_out1 = take(rd4);
    p.o_h = take(R * ffn * 2);
    p.o_r2 = take(rd4);  // r2, then d_out1
    p.o_dy[0] = take(nb > 2 ? rd4 : 0);  // block blk hands its dx to the block below in o_dy[blk & 1]
    p.o_dy[1] = take(nb > 1 ? rd4 : 0);
    p.o_dr2 = take(rd4);
    p.o_gc = take(rd4);
    p.o_dh = take(R * ffn * 2);
    p.o_dr1 = take(rd4);
    p.o_dattT = take(Bn * d * p.Lp * 2);
    p.o_datt = take(R * d * 2);
    p.o_dqkv = take(R * 3 * d * 2);
    p.o_stats = take(3 * Bn * heads * p.Lp * 4);
    p.o_slab = take((size_t)p.nchunks * d * std::max(3 * d, ffn) * 4);
    p.nsub = (int)std::max<int64_t>(1, (p.R + kTbSumRows - 1) / kTbSumRows);
    p.o_vslab = take((size_t)p.nsub * std::max(3 * d, ffn) * 4);
    p.total = off;
    return true;
}

__device__ __forceinline__ bf16x8 tb_zero8() {
    bf16x8 f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (__bf16)0.f;
    return f;
}
__device__ __forceinline__ bf16x8 tb_ld8(const uint16_t* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p)); }
__device__ __forceinline__ bf16x8 tb_ld8(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    bf16x8 f;
    f[0] = (__bf16)a.x; f[1] = (__bf16)a.y; f[2] = (__bf16)a.z; f[3] = (__bf16)a.w;
    f[4] = (__bf16)b.x; f[5] = (__bf16)b.y; f[6] = (__bf16)b.z; f[7] = (__bf16)b.w;
    return f;
}
// Every MFMA here is issued unconditionally (tiles past L or Lp run on clamped addresses and are masked or multiply exact
// zeros): a product under a branch came back with two of its four accumulator rows read before the MFMA had written them
// (the compiler places the wait states between an MFMA and the read of its result only inside one basic block).

// ---- the transposed image ---------------------------------------------------------------------------------------------
struct TbPackArgs {
    const float *Wq, *Wk, *Wv, *W1, *W2;
    uint16_t* img;
    int d, ffn;
    TbImg g;
};

__global__ __launch_bounds__(256) void tfb_pack_kernel(const TbPackArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.g.elems) return;
    const int d = a.d, ffn = a.ffn;
    float v;
    if (t < a.g.oCat) {  // WqkvT [3 d][d]: [n][k] = W[k][n]
        const int n = (int)(t / d), k = (int)(t % d);
        const float* W = n < d ? a.Wq : n < 2 * d ? a.Wk : a.Wv;
        v = W[(int64_t)k * d + n % d];
    } else if (t < a.g.oW1T) {  // Wcat [d][3 d]: [c][k] = W[c][k % d]
        const int64_t q = t - a.g.oCat;
        const int c = (int)(q / (3 * d)), k = (int)(q % (3 * d));
        const float* W = k < d ? a.Wq : k < 2 * d ? a.Wk : a.Wv;
        v = W[(int64_t)c * d + k % d];
    } else if (t < a.g.oW1) {  // W1T [ffn][d]
        const int64_t q = t - a.g.oW1T;
        v = a.W1[(q % d) * ffn + q / d];
    } else if (t < a.g.oW2T) {  // W1 [d][ffn]
        v = a.W1[t - a.g.oW1];
    } else if (t < a.g.oW2) {  // W2T [d][ffn]
        const int64_t q = t - a.g.oW2T;
        v = a.W2[(q % ffn) * d + q / ffn];
    } else {  // W2 [ffn][d]
        v = a.W2[t - a.g.oW2];
    }
    a.img[t] = (uint16_t)f32_to_bf16_bits(v);
}

// ---- x -> fp32 rows ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tfb_cvt_kernel(const void* x, int bf16, int64_t sb, int64_t sl, int L, int d, int64_t total,
                                                      float* out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t row = t / d;
    const int c = (int)(t % d);
    const int64_t off = (row / L) * sb + (row % L) * sl + c;
    out[t] = bf16 ? bf16_bits_to_f32(static_cast<const uint16_t*>(x)[off]) : static_cast<const float*>(x)[off];
}

// ---- row GEMM -----------------------------------------------------------------------------------------------------------
enum { EPI_BF16 = 0, EPI_RELU = 1, EPI_GATE = 2, EPI_RES = 3 };

struct RgArgs {
    const void* A;       // [R][lda], f32 or bf16
    int64_t lda;
    const uint16_t* W;   // [N][ldw] bf16
    int64_t ldw;
    int K, N;
    int64_t R;
    const float* bias;   // element (n / bseg) * bstride + n % bseg, or null
    int bseg, bstride;
    const float* res;    // EPI_RES: [R][N] f32
    const uint16_t* gate;  // EPI_GATE: [R][N] bf16, the gradient passes where gate > 0
    void* out;           // bf16 [R][N], or (EPI_RES) f32 at (row / L) * osb + (row % L) * osl + n
    int L;
    int64_t osb, osl;
    int o_vec;
};

template <bool AF32, int EPI>
__global__ __launch_bounds__(64) void tfb_rowgemm(const RgArgs a) {
    const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const int n0 = blockIdx.y * 64;
    const int64_t arow = row0 + lr < a.R ? row0 + lr : a.R - 1;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.K; k0 += 32) {
        const int kk = k0 + 8 * g;
        const bool kv = kk < a.K;
        bf16x8 af = tb_zero8();
        if (kv) {
            if constexpr (AF32) af = tb_ld8(static_cast<const float*>(a.A) + arow * a.lda + kk);
            else af = tb_ld8(static_cast<const uint16_t*>(a.A) + arow * a.lda + kk);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = n0 + 16 * t + lr;
            const bf16x8 wf = kv && n < a.N ? tb_ld8(a.W + (int64_t)n * a.ldw + kk) : tb_zero8();
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[t], 0, 0, 0);  // out^T[n = 4 g + r][row = lr]
        }
    }
    const int64_t row = row0 + lr;
    if (row >= a.R) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + 4 * g;
        if (n >= a.N) continue;
        f32x4 v = acc[t];
        if (a.bias) {
            const float* bp = a.bias + (n / a.bseg) * a.bstride + n % a.bseg;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bp[e];
        }
        if constexpr (EPI == EPI_RES) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(a.res + row * a.N + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = r[e] + v[e];
            float* op = static_cast<float*>(a.out) + (row / a.L) * a.osb + (row % a.L) * a.osl + n;
            if (a.o_vec) {
                *reinterpret_cast<f32x4*>(op) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) op[e] = v[e];
            }
        } else {
            if constexpr (EPI == EPI_RELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            if constexpr (EPI == EPI_GATE) {
                const uint2 gt = *reinterpret_cast<const uint2*>(a.gate + row * a.N + n);
                const uint32_t h[4] = {gt.x & 0xffffu, gt.x >> 16, gt.y & 0xffffu, gt.y >> 16};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = bf16_bits_to_f32(h[e]) > 0.f ? v[e] : 0.f;
            }
            *reinterpret_cast<uint2*>(static_cast<uint16_t*>(a.out) + row * a.N + n) = bf16_pack4(v);
        }
    }
}

// ---- transposed bf16 copies ---------------------------------------------------------------------------------------------
// src [B L][ld] (its first ncol columns) -> T [B][ncol][Lp] with zeros past L, and optionally rm [B L][ncol]
template <bool F32>
__global__ __launch_bounds__(256) void tfb_transpose(const void* src, int64_t ld, int ncol, int L, int Lp, int64_t total, uint16_t* T,
                                                     uint16_t* rm) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % ncol);
    const int l = (int)((t / ncol) % Lp);
    const int64_t b = t / ((int64_t)ncol * Lp);
    uint16_t h = 0;
    if (l < L) {
        const int64_t si = (b * L + l) * ld + c;
        if constexpr (F32) h = (uint16_t)f32_to_bf16_bits(static_cast<const float*>(src)[si]);
        else h = static_cast<const uint16_t*>(src)[si];
        if (rm) rm[(b * L + l) * ncol + c] = h;
    }
    T[(b * ncol + c) * Lp + l] = h;
}

// ---- attention ------------------------------------------------------------------------------------------------------------
struct AtArgs {
    const uint16_t* qkv;    // [B L][3 d]: q | k | v, rounded after the bias
    const uint16_t* qkvT;   // [B][3 d][Lp]
    const uint16_t* datt;   // [B L][d]
    const uint16_t* dattT;  // [B][d][Lp]
    const float* xin;       // [B L][d]
    float* r1;              // mode 0: x + att
    uint16_t* dqkv;         // [B L][3 d]: modes 1 (dq) and 2 (dk, dv)
    float* stats;           // [3][B][heads][Lp]: max, 1 / sum, delta
    int64_t nstat;          // B heads Lp
    const float* mask;
    int L, Lp, d, heads, depth;
    float scale;
};

__device__ __forceinline__ bf16x8 tb_ld44(const uint16_t* p) {
    return bf16_join(*reinterpret_cast<const uint2*>(p), *reinterpret_cast<const uint2*>(p + 16));
}

template <int NJ, int MODE>
__global__ __launch_bounds__(64) void tfb_attn(const AtArgs a) {
    constexpr int NT2 = 2 * NJ;
    const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
    const int64_t b = blockIdx.x;
    const int h = blockIdx.y, t0 = blockIdx.z;
    const int L = a.L, Lp = a.Lp, d = a.d, depth = a.depth, c0 = h * depth, ld = 3 * d;
    const int sidx = 16 * t0 + lr;  // the stationary index: a query row (modes 0, 1) or a key (mode 2)
    const bool live = sidx < L;
    const int64_t srow = b * L + min(sidx, L - 1);
    const uint16_t* base = a.qkv + b * L * ld;
    const uint16_t* dbase = a.datt + b * L * d;
    const int staCol = (MODE == 2 ? d : 0) + c0, othCol = (MODE == 2 ? 0 : d) + c0, vCol = 2 * d + c0;

    // S^T[o = 4 g + r][s = lr] = sum_c Oth[o][c] Sta[s][c], and the same for dP^T with (V, datt) / (datt, V)
    f32x4 S[NT2], dP[NT2];
#pragma unroll
    for (int ot = 0; ot < NT2; ++ot) S[ot] = dP[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; 32 * ks < depth; ++ks) {
        const int cc = 32 * ks + 8 * g;
        const bool kv = cc < depth;
        const bf16x8 sS = kv ? tb_ld8(a.qkv + srow * ld + staCol + cc) : tb_zero8();
        bf16x8 sD = tb_zero8();
        if constexpr (MODE == 1) sD = kv ? tb_ld8(a.datt + srow * d + c0 + cc) : tb_zero8();
        if constexpr (MODE == 2) sD = kv ? tb_ld8(a.qkv + srow * ld + vCol + cc) : tb_zero8();
#pragma unroll
        for (int ot = 0; ot < NT2; ++ot) {
            const int orow = min(16 * ot + lr, L - 1);  // tiles past L: a clamped row, masked below
            const bf16x8 oS = kv ? tb_ld8(base + (int64_t)orow * ld + othCol + cc) : tb_zero8();
            S[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oS, sS, S[ot], 0, 0, 0);
            if constexpr (MODE == 1) {
                const bf16x8 oD = kv ? tb_ld8(base + (int64_t)orow * ld + vCol + cc) : tb_zero8();
                dP[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oD, sD, dP[ot], 0, 0, 0);
            }
            if constexpr (MODE == 2) {
                const bf16x8 oD = kv ? tb_ld8(dbase + (int64_t)orow * d + c0 + cc) : tb_zero8();
                dP[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oD, sD, dP[ot], 0, 0, 0);
            }
        }
    }
    const int nt = depth / 16;
    float* st_m = a.stats + (b * a.heads + h) * Lp;
    float* st_i = st_m + a.nstat;
    float* st_d = st_i + a.nstat;

    if constexpr (MODE != 2) {
        // softmax over the keys (registers and the four lane groups) of query row sidx, as the forward computes it
        const bool masked = a.mask != nullptr && live && a.mask[b * L + sidx] == 0.f;
        float m = -INFINITY;
#pragma unroll
        for (int ot = 0; ot < NT2; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float l = masked ? -4294967295.f : S[ot][r] * a.scale;
                if (16 * ot + 4 * g + r >= L) l = -INFINITY;
                S[ot][r] = l;
                m = fmaxf(m, l);
            }
        m = rows4_max(m);
        float sum = 0.f;
#pragma unroll
        for (int ot = 0; ot < NT2; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                S[ot][r] = __expf(S[ot][r] - m);
                sum += S[ot][r];
            }
        const float inv = 1.f / rows4_sum(sum);
#pragma unroll
        for (int ot = 0; ot < NT2; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) S[ot][r] *= inv;  // P, fp32; exactly 0 for keys past L, 1 / L on a masked row
        bf16x8 F[NJ];
        if constexpr (MODE == 0) {
#pragma unroll
            for (int s = 0; s < NJ; ++s) F[s] = bf16_join(bf16_pack4(S[2 * s]), bf16_pack4(S[2 * s + 1]));
            for (int tt = 0; tt < nt; ++tt) {
                const uint16_t* vp = a.qkvT + ((b * ld + vCol + 16 * tt + lr) * Lp + 4 * g);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NJ; ++s)  // past Lp: F is exactly zero, any finite operand
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tb_ld44(vp + (32 * s < Lp ? 32 * s : 0)), F[s], acc, 0, 0, 0);
                            if (live) {
                    const int64_t o = (b * L + sidx) * d + c0 + 16 * tt + 4 * g;
                    const f32x4 xr = *reinterpret_cast<const f32x4*>(a.xin + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = xr[e] + acc[e];
                    *reinterpret_cast<f32x4*>(a.r1 + o) = acc;
                }
            }
        } else {
            float ds = 0.f;
#pragma unroll
            for (int ot = 0; ot < NT2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) ds += dP[ot][r] * S[ot][r];
            const float delta = rows4_sum(ds);
#pragma unroll
            for (int ot = 0; ot < NT2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) dP[ot][r] = masked ? 0.f : S[ot][r] * (dP[ot][r] - delta) * a.scale;
#pragma unroll
            for (int s = 0; s < NJ; ++s) F[s] = bf16_join(bf16_pack4(dP[2 * s]), bf16_pack4(dP[2 * s + 1]));
            if (live && g == 0) {
                st_m[sidx] = m;
                st_i[sidx] = inv;
                st_d[sidx] = delta;
            }
            for (int tt = 0; tt < nt; ++tt) {
                const uint16_t* kp = a.qkvT + ((b * ld + d + c0 + 16 * tt + lr) * Lp + 4 * g);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NJ; ++s)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tb_ld44(kp + (32 * s < Lp ? 32 * s : 0)), F[s], acc, 0, 0, 0);
                            if (live) *reinterpret_cast<uint2*>(a.dqkv + (b * L + sidx) * ld + c0 + 16 * tt + 4 * g) = bf16_pack4(acc);
            }
        }
    } else {
        // the key sidx on the lanes, the queries i = 16 ot + 4 g + r in the registers
        bf16x8 FP[NJ], FD[NJ];
#pragma unroll
        for (int ot = 0; ot < NT2; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ot + 4 * g + r;
                float pv = 0.f, dv = 0.f;
                if (i < L && live) {
                    const bool mrow = a.mask != nullptr && a.mask[b * L + i] == 0.f;
                    const float inv = st_i[i];
                    if (mrow) {
                        pv = inv;  // 1 / L; dS = 0
                    } else {
                        pv = __expf(S[ot][r] * a.scale - st_m[i]) * inv;
                        dv = pv * (dP[ot][r] - st_d[i]) * a.scale;
                    }
                }
                S[ot][r] = pv;
                dP[ot][r] = dv;
            }
#pragma unroll
        for (int s = 0; s < NJ; ++s) {
            FP[s] = bf16_join(bf16_pack4(S[2 * s]), bf16_pack4(S[2 * s + 1]));
            FD[s] = bf16_join(bf16_pack4(dP[2 * s]), bf16_pack4(dP[2 * s + 1]));
        }
        for (int tt = 0; tt < nt; ++tt) {
            const uint16_t* ap = a.dattT + ((b * d + c0 + 16 * tt + lr) * Lp + 4 * g);
            const uint16_t* qp = a.qkvT + ((b * ld + c0 + 16 * tt + lr) * Lp + 4 * g);
            f32x4 av = {0.f, 0.f, 0.f, 0.f}, ak = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NJ; ++s)
            {
                const int j0 = 32 * s < Lp ? 32 * s : 0;
                av = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tb_ld44(ap + j0), FP[s], av, 0, 0, 0);  // dv^T[c][j]
                ak = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tb_ld44(qp + j0), FD[s], ak, 0, 0, 0);  // dk^T[c][j]
            }
                    if (live) {
                uint16_t* o = a.dqkv + (b * L + sidx) * ld + c0 + 16 * tt + 4 * g;
                *reinterpret_cast<uint2*>(o + d) = bf16_pack4(ak);
                *reinterpret_cast<uint2*>(o + 2 * d) = bf16_pack4(av);
            }
        }
    }
}

// ---- LayerNorm, one wave per row (d <= 256: four columns per lane) ------------------------------------------------------
__global__ __launch_bounds__(256) void tfb_ln_fwd(const float* r, const float* gamma, const float* beta, float eps, int d, int64_t R,
                                                  float* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    float v[4], s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = lane + 64 * e;
        v[e] = c < d ? r[row * d + c] : 0.f;
        s += v[e];
    }
    const float mean = wave_sum_butterfly(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = lane + 64 * e < d ? v[e] - mean : 0.f;
        q += t * t;
    }
    const float inv = 1.f / sqrtf(wave_sum_butterfly(q) / (float)d + eps);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = lane + 64 * e;
        if (c < d) out[row * d + c] = (v[e] - mean) * inv * gamma[c] + beta[c];
    }
}

// dr = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; gc = dy xhat (the rows of dgamma). dy at
// (row / L) * sb + (row % L) * sl
__global__ __launch_bounds__(256) void tfb_ln_bwd(const float* r, const float* dy, int L, int64_t sb, int64_t sl, const float* gamma,
                                                  float eps, int d, int64_t R, float* dr, float* gc) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float* dyr = dy + (row / L) * sb + (row % L) * sl;
    float v[4], gy[4], dyv[4], s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = lane + 64 * e;
        v[e] = c < d ? r[row * d + c] : 0.f;
        dyv[e] = c < d ? dyr[c] : 0.f;
        gy[e] = c < d ? dyv[e] * gamma[c] : 0.f;
        s += v[e];
    }
    const float mean = wave_sum_butterfly(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = lane + 64 * e < d ? v[e] - mean : 0.f;
        q += v[e] * v[e];
    }
    const float inv = 1.f / sqrtf(wave_sum_butterfly(q) / (float)d + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] *= inv;  // xhat
        s1 += gy[e];
        s2 += gy[e] * v[e];
    }
    const float m1 = wave_sum_butterfly(s1) / (float)d, m2 = wave_sum_butterfly(s2) / (float)d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = lane + 64 * e;
        if (c < d) {
            dr[row * d + c] = inv * (gy[e] - m1 - v[e] * m2);
            gc[row * d + c] = dyv[e] * v[e];
        }
    }
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------
struct DwArgs {
    const void* A;  // [R][lda], columns 0 .. M
    int64_t lda;
    int M;
    const void* Bm;  // [R][ldb], columns 0 .. N
    int64_t ldb;
    int N;
    int64_t R, chunk;
    float* part;  // [chunks][M][N]
};

template <bool F32>
__device__ __forceinline__ void tb_stage(const void* src, int64_t ld, int ncol, int c, int64_t grow, int64_t rend, uint16_t (*T)[40],
                                         int c8, int row) {
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (grow < rend && c + c8 < ncol) {
        if constexpr (F32) u = __builtin_bit_cast(uint4, tb_ld8(static_cast<const float*>(src) + grow * ld + c + c8));
        else u = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(src) + grow * ld + c + c8);
    }
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) T[c8 + e][row] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
}

template <bool AF32, bool BF32>
__global__ __launch_bounds__(256) void tfb_dw(const DwArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t At[64][40], Bt[64][40];  // [column][32 rows + 8]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int64_t rbeg = (int64_t)blockIdx.z * a.chunk, rend = rbeg + a.chunk < a.R ? rbeg + a.chunk : a.R;
    const int srow = tid >> 3, c8 = (tid & 7) * 8;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t rr = rbeg; rr < rend; rr += 32) {
        __syncthreads();
        tb_stage<AF32>(a.A, a.lda, a.M, m0, rr + srow, rend, At, c8, srow);
        tb_stage<BF32>(a.Bm, a.ldb, a.N, n0, rr + srow, rend, Bt, c8, srow);
        __syncthreads();
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(&At[16 * w + lr][8 * g]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bf16x8 bf = *reinterpret_cast<const bf16x8*>(&Bt[16 * t + lr][8 * g]);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[t], 0, 0, 0);  // C[m = 4 g + r][n = lr]
        }
    }
    float* part = a.part + (int64_t)blockIdx.z * a.M * a.N;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * w + 4 * g + r;
            if (m < a.M && n < a.N) part[(int64_t)m * a.N + n] = acc[t][r];
        }
    }
}

// column sums of src (row at (row / L) * sb + (row % L) * sl) over kTbSumRows rows per workgroup: 64 columns x 4 row
// phases, each phase its rows in order, the four phases added in order: part [nsub][N]
template <bool BF16>
__global__ __launch_bounds__(256) void tfb_colsum(const void* src, int L, int64_t sb, int64_t sl, int N, int64_t R, float* part) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + c;
    const int64_t rbeg = (int64_t)blockIdx.x * kTbSumRows, rend = rbeg + kTbSumRows < R ? rbeg + kTbSumRows : R;
    float s = 0.f;
    if (n < N)
        for (int64_t row = rbeg + ph; row < rend; row += 4) {
            const int64_t o = (row / L) * sb + (row % L) * sl + n;
            s += BF16 ? bf16_bits_to_f32(static_cast<const uint16_t*>(src)[o]) : static_cast<const float*>(src)[o];
        }
    red[ph][c] = s;
    __syncthreads();
    if (ph == 0 && n < N) part[(int64_t)blockIdx.x * N + n] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// the vector gradients from their partials: 64 columns x 4 phases, phase ph adds its quarter of the partials in order,
// the four quarters are added in order. dst[seg][n % (N / nseg)]
struct VrArgs {
    const float* part;
    int nsub, N, nseg;
    float* dst[3];
};
__global__ __launch_bounds__(256) void tfb_vreduce(const VrArgs a) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int q = (a.nsub + 3) / 4;
    float s = 0.f;
    if (n < a.N)
        for (int i = ph * q; i < min((ph + 1) * q, a.nsub); ++i) s += a.part[(int64_t)i * a.N + n];
    red[ph][c] = s;
    __syncthreads();
    if (ph == 0 && n < a.N) {
        const int sw = a.N / a.nseg, seg = n / sw;
        float* dst = seg == 0 ? a.dst[0] : seg == 1 ? a.dst[1] : a.dst[2];
        dst[n % sw] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    }
}

// dst[seg][m][n % (N / nseg)] = sum over the chunks, in chunk order
struct RdArgs {
    const float* part;
    int nchunks, N, nseg;
    int64_t elems;  // M N
    float* dst[3];
};
__global__ __launch_bounds__(256) void tfb_reduce(const RdArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.elems) return;
    float s = 0.f;
    for (int c = 0; c < a.nchunks; ++c) s += a.part[(int64_t)c * a.elems + t];
    const int64_t m = t / a.N;
    const int n = (int)(t % a.N), sw = a.N / a.nseg, seg = n / sw;
    float* dst = seg == 0 ? a.dst[0] : seg == 1 ? a.dst[1] : a.dst[2];
    dst[m * sw + n % sw] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct TbRun {
    TbPlan p;
    char* ws;
    hipStream_t st;
    template <typename T>
    T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
};

template <bool AF32, int EPI>
void tb_rowgemm(const TbRun& r, const void* A, int64_t lda, const uint16_t* W, int K, int N, const float* bias, int bseg, int bstride,
                const float* res, const uint16_t* gate, void* out, int64_t osb, int64_t osl) {
    RgArgs a;
    a.A = A; a.lda = lda; a.W = W; a.ldw = K; a.K = K; a.N = N; a.R = r.p.R;
    a.bias = bias; a.bseg = bseg; a.bstride = bstride; a.res = res; a.gate = gate; a.out = out;
    a.L = r.p.L; a.osb = osb; a.osl = osl;
    a.o_vec = ((uintptr_t)out & 15) == 0 && osb % 4 == 0 && osl % 4 == 0;
    hipLaunchKernelGGL((tfb_rowgemm<AF32, EPI>), dim3((unsigned)((r.p.R + 15) / 16), (unsigned)((N + 63) / 64)), dim3(64), 0, r.st, a);
}

template <int MODE>
void tb_attn(const TbRun& r, const AtArgs& a) {
    const dim3 grid((unsigned)r.p.B, (unsigned)r.p.heads, (unsigned)((r.p.L + 15) / 16));
    switch (r.p.NJ) {
        case 1: hipLaunchKernelGGL((tfb_attn<1, MODE>), grid, dim3(64), 0, r.st, a); break;
        case 2: hipLaunchKernelGGL((tfb_attn<2, MODE>), grid, dim3(64), 0, r.st, a); break;
        case 4: hipLaunchKernelGGL((tfb_attn<4, MODE>), grid, dim3(64), 0, r.st, a); break;
        default: hipLaunchKernelGGL((tfb_attn<8, MODE>), grid, dim3(64), 0, r.st, a); break;
    }
}

void tb_reduce(const TbRun& r, const float* part, int M, int N, int nseg, float* d0, float* d1, float* d2) {
    RdArgs a;
    a.part = part; a.nchunks = r.p.nchunks; a.N = N; a.nseg = nseg; a.elems = (int64_t)M * N;
    a.dst[0] = d0; a.dst[1] = d1; a.dst[2] = d2;
    hipLaunchKernelGGL(tfb_reduce, dim3((unsigned)((a.elems + 255) / 256)), dim3(256), 0, r.st, a);
}

template <bool AF32, bool BF32>
void tb_dw(const TbRun& r, const void* A, int64_t lda, int M, const void* Bm, int64_t ldb, int N, int nseg, float* d0, float* d1,
           float* d2) {
    DwArgs a;
    a.A = A; a.lda = lda; a.M = M; a.Bm = Bm; a.ldb = ldb; a.N = N; a.R = r.p.R; a.chunk = r.p.chunk;
    a.part = r.at<float>(r.p.o_slab);
    hipLaunchKernelGGL((tfb_dw<AF32, BF32>), dim3((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64), (unsigned)r.p.nchunks), dim3(256),
                       0, r.st, a);
    tb_reduce(r, a.part, M, N, nseg, d0, d1, d2);
}

template <bool BF16>
void tb_colsum(const TbRun& r, const void* src, int64_t sb, int64_t sl, int N, int nseg, float* d0, float* d1, float* d2) {
    float* part = r.at<float>(r.p.o_vslab);
    hipLaunchKernelGGL((tfb_colsum<BF16>), dim3((unsigned)r.p.nsub, (unsigned)((N + 63) / 64)), dim3(256), 0, r.st, src, r.p.L, sb, sl, N,
                       r.p.R, part);
    VrArgs a;
    a.part = part; a.nsub = r.p.nsub; a.N = N; a.nseg = nseg;
    a.dst[0] = d0; a.dst[1] = d1; a.dst[2] = d2;
    hipLaunchKernelGGL(tfb_vreduce, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, r.st, a);
}

}  // namespace

extern "C" size_t rf_tfenc_bwd_packed_bytes(int32_t d_model, int32_t ffn_hidden, int32_t n_blocks) {
    if (rf_tfenc_packed_bytes(d_model, ffn_hidden, n_blocks) == 0) return 0;  // the forward's limits and messages
    return (size_t)tb_img(d_model, ffn_hidden).elems * 2 * n_blocks;
}

extern "C" int rf_tfenc_bwd_pack(int32_t block, int32_t d_model, int32_t ffn_hidden, int32_t n_blocks, const float* Wq, const float* Wk,
                                 const float* Wv, const float* W1, const float* W2, void* packed_t, void* stream) {
    if (rf_tfenc_packed_bytes(d_model, ffn_hidden, n_blocks) == 0) return RF_EINVAL;
    RF_REQUIRE(block >= 0 && block < n_blocks, "rf_tfenc_bwd_pack: block (%d) must be in [0, %d)", block, n_blocks);
    RF_REQUIRE(Wq && Wk && Wv && W1 && W2, "rf_tfenc_bwd_pack: null parameter pointer");
    RF_REQUIRE(packed_t && ((uintptr_t)packed_t & 15) == 0, "rf_tfenc_bwd_pack: packed_t is null or not 16-byte aligned");
    TbPackArgs a;
    a.Wq = Wq; a.Wk = Wk; a.Wv = Wv; a.W1 = W1; a.W2 = W2;
    a.d = d_model; a.ffn = ffn_hidden;
    a.g = tb_img(d_model, ffn_hidden);
    a.img = static_cast<uint16_t*>(packed_t) + (int64_t)block * a.g.elems;
    hipLaunchKernelGGL(tfb_pack_kernel, dim3((unsigned)((a.g.elems + 255) / 256)), dim3(256), 0, rf_stream(stream), a);
    return rf_check_launch("rf_tfenc_bwd_pack");
}

extern "C" size_t rf_tfenc_bwd_ws_bytes(int32_t batch, int32_t L, int32_t d_model, int32_t heads, int32_t ffn_hidden, int32_t n_blocks) {
    if (batch < 0) {
        rf_set_error(RF_EINVAL, "rf_tfenc_bwd_ws_bytes: batch must be >= 0");
        return 0;
    }
    if (n_blocks < 1 || n_blocks > kTbMaxBlocks) {
        rf_set_error(RF_EINVAL, "rf_tfenc_bwd_ws_bytes: n_blocks (%d) must be in [1, %d]", n_blocks, kTbMaxBlocks);
        return 0;
    }
    TbPlan p;
    if (!tb_plan(batch, L, d_model, heads, ffn_hidden, n_blocks, p)) return 0;
    return p.total;
}

extern "C" int rf_tfenc_bwd(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t x_stride_l, const float* mask, int32_t batch,
                            int32_t L, int32_t d_model, int32_t heads, int32_t ffn_hidden, int32_t n_blocks, const void* packed,
                            const void* packed_t, float eps, const float* dout, int64_t dout_stride_b, int64_t dout_stride_l, float* dx,
                            int64_t dx_stride_b, int64_t dx_stride_l, float* const* grads, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(n_blocks >= 1 && n_blocks <= kTbMaxBlocks, "rf_tfenc_bwd: n_blocks (%d) must be in [1, %d]", n_blocks, kTbMaxBlocks);
    RF_REQUIRE(batch >= 0, "rf_tfenc_bwd: batch must be >= 0");
    TbRun r;
    if (!tb_plan(batch, L, d_model, heads, ffn_hidden, n_blocks, r.p)) return RF_EINVAL;
    const TbPlan& p = r.p;
    const int d = d_model, ffn = ffn_hidden;
    RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_tfenc_bwd: x_dtype must be F32 or BF16");
    RF_REQUIRE(x_stride_l >= d && x_stride_b >= 0, "rf_tfenc_bwd: x_stride_l must be >= d_model and x_stride_b >= 0");
    RF_REQUIRE(dout_stride_l >= d && dout_stride_b >= 0, "rf_tfenc_bwd: dout_stride_l must be >= d_model and dout_stride_b >= 0");
    RF_REQUIRE(dx_stride_l >= d && dx_stride_b >= (int64_t)(L - 1) * dx_stride_l + d,
               "rf_tfenc_bwd: dx_stride_l must be >= d_model and dx_stride_b >= (L - 1) * dx_stride_l + d_model");
    RF_REQUIRE(eps >= 0.f && std::isfinite(eps), "rf_tfenc_bwd: eps must be finite and >= 0");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && packed && packed_t && dout && dx, "rf_tfenc_bwd: null pointer (x, packed, packed_t, dout or dx)");
    RF_REQUIRE(grads, "rf_tfenc_bwd: grads is null");
    for (int i = 0; i < 14 * n_blocks; ++i) RF_REQUIRE(grads[i], "rf_tfenc_bwd: grads[%d] is null", i);
    RF_REQUIRE(((uintptr_t)packed & 15) == 0, "rf_tfenc_bwd: packed must be 16-byte aligned");
    RF_REQUIRE(((uintptr_t)packed_t & 15) == 0, "rf_tfenc_bwd: packed_t must be 16-byte aligned");
    RF_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "rf_tfenc_bwd: ws is null or not 16-byte aligned");
    RF_REQUIRE(ws_bytes >= p.total, "rf_tfenc_bwd: ws_bytes (%zu) is less than rf_tfenc_bwd_ws_bytes (%zu)", ws_bytes, p.total);
    {
        const uintptr_t d0 = (uintptr_t)dout, d1 = d0 + ((uint64_t)(batch - 1) * dout_stride_b + (uint64_t)(L - 1) * dout_stride_l + d) * 4;
        const uintptr_t e0 = (uintptr_t)dx, e1 = e0 + ((uint64_t)(batch - 1) * dx_stride_b + (uint64_t)(L - 1) * dx_stride_l + d) * 4;
        RF_REQUIRE(d1 <= e0 || e1 <= d0, "rf_tfenc_bwd: dx may not alias dout");
    }
    r.ws = static_cast<char*>(ws);
    r.st = rf_stream(stream);
    const int64_t R = p.R, Ld = (int64_t)L * d;
    const TbImg g = tb_img(d, ffn);

    // 1. the fp32 input of every block
    float* xin = r.at<float>(p.o_xin);
    const int64_t xin_stride = (int64_t)(al256((size_t)R * d * 4) / 4);
    hipLaunchKernelGGL(tfb_cvt_kernel, dim3((unsigned)((R * d + 255) / 256)), dim3(256), 0, r.st, x, x_dtype == RF_DTYPE_BF16 ? 1 : 0,
                       x_stride_b, x_stride_l, L, d, R * d, xin);
    for (int blk = 0; blk + 1 < n_blocks; ++blk) {
        const int rc = rf_tfenc_fwd(xin + blk * xin_stride, RF_DTYPE_F32, Ld, d, mask, batch, L, d, heads, ffn, 1,
                                    static_cast<const char*>(packed) + blk * p.block_bytes, eps, xin + (blk + 1) * xin_stride, Ld, d, stream);
        if (rc != RF_OK) return rc;
    }

    // 2. block by block, last to first
    uint16_t* qkv = r.at<uint16_t>(p.o_qkv);
    uint16_t* qkvT = r.at<uint16_t>(p.o_qkvT);
    float* r1 = r.at<float>(p.o_r1);
    float* out1 = r.at<float>(p.o_out1);
    uint16_t* hb = r.at<uint16_t>(p.o_h);
    float* r2 = r.at<float>(p.o_r2);
    float* dout1 = r2;  // r2 is dead after LayerNorm 2's backward
    float* dr2 = r.at<float>(p.o_dr2);
    float* gc = r.at<float>(p.o_gc);
    uint16_t* dh = r.at<uint16_t>(p.o_dh);
    float* dr1 = r.at<float>(p.o_dr1);
    uint16_t* dattT = r.at<uint16_t>(p.o_dattT);
    uint16_t* datt = r.at<uint16_t>(p.o_datt);
    uint16_t* dqkv = r.at<uint16_t>(p.o_dqkv);
    const unsigned ln_grid = (unsigned)((R + 3) / 4);

    for (int blk = n_blocks - 1; blk >= 0; --blk) {
        const float* X = xin + blk * xin_stride;
        const uint16_t* pt = static_cast<const uint16_t*>(packed_t) + (int64_t)blk * g.elems;
        const float* vec = reinterpret_cast<const float*>(static_cast<const char*>(packed) + blk * p.block_bytes + p.oVec);
        const float *b2 = vec + 3 * p.dp, *g1 = vec + 4 * p.dp, *be1 = vec + 5 * p.dp, *g2 = vec + 6 * p.dp, *b1 = vec + 8 * p.dp;
        float* const* G = grads + 14 * blk;  // Wq bq Wk bk Wv bv gamma1 beta1 W1 b1 W2 b2 gamma2 beta2
        const float* dy;
        int64_t dysb, dysl;
        if (blk == n_blocks - 1) { dy = dout; dysb = dout_stride_b; dysl = dout_stride_l; }
        else { dy = r.at<float>(p.o_dy[(blk + 1) & 1]); dysb = Ld; dysl = d; }
        float* dxo;
        int64_t dxsb, dxsl;
        if (blk == 0) { dxo = dx; dxsb = dx_stride_b; dxsl = dx_stride_l; }
        else { dxo = r.at<float>(p.o_dy[blk & 1]); dxsb = Ld; dxsl = d; }

        // the forward chain again
        tb_rowgemm<true, EPI_BF16>(r, X, d, pt + g.oQkvT, d, 3 * d, vec, d, p.dp, nullptr, nullptr, qkv, 0, 0);
        {
            const int64_t total = p.B * p.Lp * 3 * d;
            hipLaunchKernelGGL((tfb_transpose<false>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, r.st, qkv, (int64_t)3 * d, 3 * d,
                               L, p.Lp, total, qkvT, (uint16_t*)nullptr);
        }
        AtArgs at;
        at.qkv = qkv; at.qkvT = qkvT; at.datt = datt; at.dattT = dattT; at.xin = X; at.r1 = r1; at.dqkv = dqkv;
        at.stats = r.at<float>(p.o_stats); at.nstat = p.B * heads * p.Lp; at.mask = mask;
        at.L = L; at.Lp = p.Lp; at.d = d; at.heads = heads; at.depth = p.depth; at.scale = 1.f / sqrtf((float)p.depth);
        tb_attn<0>(r, at);
        hipLaunchKernelGGL(tfb_ln_fwd, dim3(ln_grid), dim3(256), 0, r.st, r1, g1, be1, eps, d, R, out1);
        tb_rowgemm<true, EPI_RELU>(r, out1, d, pt + g.oW1T, d, ffn, b1, ffn, 0, nullptr, nullptr, hb, 0, 0);
        tb_rowgemm<false, EPI_RES>(r, hb, ffn, pt + g.oW2T, ffn, d, b2, d, 0, out1, nullptr, r2, Ld, d);

        // LayerNorm 2 and the FFN
        hipLaunchKernelGGL(tfb_ln_bwd, dim3(ln_grid), dim3(256), 0, r.st, r2, dy, L, dysb, dysl, g2, eps, d, R, dr2, gc);
        tb_colsum<false>(r, gc, Ld, d, d, 1, G[12], nullptr, nullptr);
        tb_colsum<false>(r, dy, dysb, dysl, d, 1, G[13], nullptr, nullptr);
        tb_colsum<false>(r, dr2, Ld, d, d, 1, G[11], nullptr, nullptr);
        tb_rowgemm<true, EPI_GATE>(r, dr2, d, pt + g.oW2, d, ffn, nullptr, 1, 0, nullptr, hb, dh, 0, 0);
        tb_colsum<true>(r, dh, (int64_t)L * ffn, ffn, ffn, 1, G[9], nullptr, nullptr);
        tb_dw<false, true>(r, hb, ffn, ffn, dr2, d, d, 1, G[10], nullptr, nullptr);
        tb_dw<true, false>(r, out1, d, d, dh, ffn, ffn, 1, G[8], nullptr, nullptr);
        tb_rowgemm<false, EPI_RES>(r, dh, ffn, pt + g.oW1, ffn, d, nullptr, 1, 0, dr2, nullptr, dout1, Ld, d);

        // LayerNorm 1 and the attention
        hipLaunchKernelGGL(tfb_ln_bwd, dim3(ln_grid), dim3(256), 0, r.st, r1, dout1, L, Ld, (int64_t)d, g1, eps, d, R, dr1, gc);
        tb_colsum<false>(r, gc, Ld, d, d, 1, G[6], nullptr, nullptr);
        tb_colsum<false>(r, dout1, Ld, d, d, 1, G[7], nullptr, nullptr);
        {
            const int64_t total = p.B * p.Lp * d;
            hipLaunchKernelGGL((tfb_transpose<true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, r.st, dr1, (int64_t)d, d, L, p.Lp,
                               total, dattT, datt);
        }
        tb_attn<1>(r, at);
        tb_attn<2>(r, at);
        tb_colsum<true>(r, dqkv, (int64_t)L * 3 * d, 3 * d, 3 * d, 3, G[1], G[3], G[5]);
        tb_dw<true, false>(r, X, d, d, dqkv, 3 * d, 3 * d, 3, G[0], G[2], G[4]);
        tb_rowgemm<false, EPI_RES>(r, dqkv, 3 * d, pt + g.oCat, 3 * d, d, nullptr, 1, 0, dr1, nullptr, dxo, dxsb, dxsl);
    }
    return rf_check_launch("rf_tfenc_bwd");
}
