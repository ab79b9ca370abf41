// rf_interact.hip — feature-interaction layers of the non-attention rankers (backend/layers/network_layers.py), forward:
//   rf_fm_fwd     FM_Layer.call :43-56 and New_FM.call :193-207 (DeepFM): first order + 0.5 sum_d((sum_f e)^2 - sum_f e^2)
//   rf_cross_fwd  CrossNetwork.call :163-171 (DCN): x_{l+1} = x_0 (x_l . w_l) + b_l + x_l, every layer in one launch
//   rf_cin_fwd    CIN.call :238-255 (xDeepFM): per layer a GEMM whose A operand (the outer products X0[i,d] X^k[j,d]) is
//                 generated in registers and never written to HBM
// and their backward: rf_fm_bwd and rf_cross_bwd (memory-bound) and rf_cin_bwd (two more generated-operand GEMMs per
// layer), each described at its kernels below.
// All are deterministic: no floating-point atomics, every reduction in a fixed order.
//
// FM: one wave per example. A lane owns the columns d = lane, lane + 64, ...; the field sum is sequential in f (eight
// row loads in flight, compensated: the two sums cancel), the column sum and the first-order sum are xor-shuffle
// trees. fp32 throughout.
//
// Cross: one block per row, the row (x_0 and x_l) in registers for all layers: 256 threads x up to 16 elements for
// dim <= 4096, 1024 threads x up to 32 elements above. x is read once and out is written once; w_l and b_l come from
// L2. The dot product is summed per thread in element order, then by the shuffle tree, then over the waves in order.
//
// CIN: rows of the GEMMs are (example, d) pairs, an example's d padded to 16-row subtiles (D <= 256: at most 16), so
// that a subtile belongs to one example. A workgroup of 4 waves owns MS subtiles (MS = 4, 2, 1: the largest whose LDS
// fits) and runs every layer on them: X0 and X^k stay in LDS as fp32 [row][h + pad], pitch = 4 mod 8 floats, which
// makes the 32-byte row reads of the A fragment conflict-free. For v_mfma_f32_16x16x32_bf16 lane l holds A[row l & 15]
// [k = 8 (l >> 4) + e]; with H_k padded to a multiple of 8 a lane's eight k are one field i of X0 and eight consecutive
// j of X^k, so a fragment is one X0 value times eight X^k values, each product formed in fp32 and rounded once (RNE,
// v_cvt_pk_bf16_f32). The fragment is reused for every 16-column tile of the layer's output that the wave owns. W_k is
// read as a packed bf16 image (rf_cin_pack_w) [k step of 32][16-column tile][lane][8], so a wave's B fragment is one
// conflict-free 16-byte LDS read and a stage of the image is a flat copy; two stages sit in LDS and two more are in
// flight in registers, with one barrier per stage. The accumulators are fp32; X^{k+1} goes back to LDS in fp32, its sum over the subtile's
// 16 rows goes to the workspace, and a second kernel adds an example's subtiles in order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rf_common.h"
#include "rf_wave.h"

namespace {

template <typename T>
__device__ __forceinline__ float ld_f32(const T* p);
template <>
__device__ __forceinline__ float ld_f32<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld_f32<uint16_t>(const uint16_t* p) { return bf16_bits_to_f32(*p); }

// ---------------------------------------------------------------------------------------------------------------
// FM
// ---------------------------------------------------------------------------------------------------------------
constexpr int kFmMaxDim = 1024, kFmMaxFields = 4096;

// sum += v with the rounding error carried in c (Kahan): the field sums cancel in (sum e)^2 - sum e^2, and plain
// sequential fp32 sums of a few hundred fields leave 1e-6 of the result
__device__ __forceinline__ void kahan_add(float& sum, float& c, float v) {
    const float y = v - c;
    const float t = sum + y;
    c = (t - sum) - y;
    sum = t;
}

// GATHER: e[b][f] = V[ids[b][f]] (a row outside [0, v_rows) reads as NaN, as rf_embedding_bag_fwd's rows do)
template <typename T, bool GATHER>
__global__ __launch_bounds__(256) void fm_kernel(const T* __restrict__ x, int64_t sb, int64_t sf,
                                                 const int64_t* __restrict__ ids, int64_t ld_ids, int64_t v_rows, int B,
                                                 int fields, int dim, const float* __restrict__ w0,
                                                 const float* __restrict__ w, const int64_t* __restrict__ w_ids, int n,
                                                 int64_t ld_wids, int64_t w_rows, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t* idr = GATHER ? ids + b * ld_ids : nullptr;
    const T* xb = GATHER ? x : x + b * sb;
    auto row = [&](int f) -> const T* {
        if (!GATHER) return xb + (int64_t)f * sf;
        const int64_t r = idr[f];
        return r < 0 || r >= v_rows ? nullptr : xb + r * (int64_t)dim;
    };
    float second = 0.f;
    for (int d = lane; d < dim; d += 64) {
        float s = 0.f, q = 0.f, cs = 0.f, cq = 0.f;  // cs, cq: the running compensations of s and q
        int f = 0;
        for (; f + 8 <= fields; f += 8) {
            float e[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const T* r = row(f + u);
                e[u] = r ? ld_f32(r + d) : __uint_as_float(0x7fc00000u);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                kahan_add(s, cs, e[u]);
                kahan_add(q, cq, e[u] * e[u]);
            }
        }
        for (; f < fields; ++f) {
            const T* r = row(f);
            const float e = r ? ld_f32(r + d) : __uint_as_float(0x7fc00000u);
            kahan_add(s, cs, e);
            kahan_add(q, cq, e * e);
        }
        second += s * s - q;
    }
    second = wave_sum_butterfly(second);
    float first = 0.f;
    if (w) {
        const int64_t* wr = w_ids + b * ld_wids;
        for (int i = lane; i < n; i += 64) {
            const int64_t r = wr[i];
            first += r < 0 || r >= w_rows ? __uint_as_float(0x7fc00000u) : w[r];
        }
        first = wave_sum_butterfly(first);
    }
    if (lane == 0) out[b] = ((w0 ? *w0 : 0.f) + first) + 0.5f * second;
}

// ---------------------------------------------------------------------------------------------------------------
// Cross
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCrossMaxLayers = 16, kCrossMaxDim = 32768;

template <typename T, int THREADS, int EPT>
__global__ __launch_bounds__(THREADS) void cross_kernel(const T* __restrict__ x, int64_t ldx, int dim, int L,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ out, int64_t ldo) {
    constexpr int NW = THREADS / 64;
    __shared__ float red[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* xr = x + (int64_t)blockIdx.x * ldx;
    const int ne = tid < dim ? (dim - tid + THREADS - 1) / THREADS : 0;  // this thread's elements: e < ne
    float x0[EPT], xl[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        x0[e] = e < ne ? ld_f32(xr + tid + e * THREADS) : 0.f;
        xl[e] = x0[e];
    }
    for (int l = 0; l < L; ++l) {
        const float* wl = w + (int64_t)l * dim;
        const float* bl = bias + (int64_t)l * dim;
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            dot += xl[e] * (e < ne ? wl[tid + e * THREADS] : 0.f);
            if (e % 8 == 7) __builtin_amdgcn_sched_barrier(0);  // at most eight w loads in flight: no spills at EPT = 32
        }
        dot = wave_sum_butterfly(dot);
        if (lane == 0) red[l & 1][wave] = dot;  // two buffers: one barrier per layer is enough
        __syncthreads();
        float s = red[l & 1][0];
#pragma unroll
        for (int v = 1; v < NW; ++v) s += red[l & 1][v];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            xl[e] = (x0[e] * s + (e < ne ? bl[tid + e * THREADS] : 0.f)) + xl[e];
            if (e % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
    float* o = out + (int64_t)blockIdx.x * ldo;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        if (e < ne) o[tid + e * THREADS] = xl[e];
    }
}

template <typename T, int THREADS, int EPT>
void launch_cross(const void* x, int64_t ldx, int B, int dim, int L, const float* w, const float* b, float* out,
                  int64_t ldo, hipStream_t st) {
    hipLaunchKernelGGL((cross_kernel<T, THREADS, EPT>), dim3(B), dim3(THREADS), 0, st, (const T*)x, ldx, dim, L, w, b, out,
                       ldo);
}

template <typename T>
void dispatch_cross(const void* x, int64_t ldx, int B, int dim, int L, const float* w, const float* b, float* out,
                    int64_t ldo, hipStream_t st) {
#define RF_CROSS(TH, E) launch_cross<T, TH, E>(x, ldx, B, dim, L, w, b, out, ldo, st)
    if (dim <= 256) RF_CROSS(256, 1);
    else if (dim <= 512) RF_CROSS(256, 2);
    else if (dim <= 1024) RF_CROSS(256, 4);
    else if (dim <= 2048) RF_CROSS(256, 8);
    else if (dim <= 4096) RF_CROSS(256, 16);
    else if (dim <= 8192) RF_CROSS(1024, 8);
    else if (dim <= 16384) RF_CROSS(1024, 16);
    else RF_CROSS(1024, 32);
#undef RF_CROSS
}

// ---------------------------------------------------------------------------------------------------------------
// FM backward
// ---------------------------------------------------------------------------------------------------------------
// de[b][f][d] = g (S[d] - e[b][f][d]), S = sum_f e, g = dout[b]. One wave per example as the forward; a lane's NC =
// ceil(dim / 64) columns of S stay in registers. Pass 1 forms S (sequential in f, compensated as the forward's field
// sums: S - e cancels where one field dominates), pass 2 re-reads the rows (L2) and stores dx once. U rows are in
// flight in both passes (U * NC loads, eight up to dim 512).
template <typename T, bool GATHER, int NC>
__global__ __launch_bounds__(256) void fm_bwd_kernel(const T* __restrict__ x, int64_t sb, int64_t sf,
                                                     const int64_t* __restrict__ ids, int64_t ld_ids, int64_t v_rows, int B,
                                                     int fields, int dim, const float* __restrict__ dout,
                                                     float* __restrict__ dx, int64_t dsb, int64_t dsf) {
    constexpr int U = NC >= 8 ? 1 : 8 / NC;
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t* idr = GATHER ? ids + b * ld_ids : nullptr;
    const T* xb = GATHER ? x : x + b * sb;
    const float nan = __uint_as_float(0x7fc00000u);
    auto row = [&](int f) -> const T* {
        if (!GATHER) return xb + (int64_t)f * sf;
        const int64_t r = idr[f];
        return r < 0 || r >= v_rows ? nullptr : xb + r * (int64_t)dim;
    };
    auto load = [&](const T* r, int j) -> float {
        const int d = lane + 64 * j;
        return d < dim ? (r ? ld_f32(r + d) : nan) : 0.f;
    };
    float S[NC], C[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) S[j] = C[j] = 0.f;
    int f = 0;
    for (; f + U <= fields; f += U) {
        float e[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T* r = row(f + u);
#pragma unroll
            for (int j = 0; j < NC; ++j) e[u][j] = load(r, j);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j < NC; ++j) kahan_add(S[j], C[j], e[u][j]);
        }
    }
    for (; f < fields; ++f) {
        const T* r = row(f);
#pragma unroll
        for (int j = 0; j < NC; ++j) kahan_add(S[j], C[j], load(r, j));
    }
    const float g = dout[b];
    float* dxb = dx + b * dsb;
    f = 0;
    for (; f + U <= fields; f += U) {
        float e[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T* r = row(f + u);
#pragma unroll
            for (int j = 0; j < NC; ++j) e[u][j] = load(r, j);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float* o = dxb + (int64_t)(f + u) * dsf;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int d = lane + 64 * j;
                if (d < dim) o[d] = g * (S[j] - e[u][j]);
            }
        }
    }
    for (; f < fields; ++f) {
        const T* r = row(f);
        float* o = dxb + (int64_t)f * dsf;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int d = lane + 64 * j;
            if (d < dim) o[d] = g * (S[j] - load(r, j));
        }
    }
}

// The same backward with the example in registers, for examples large enough to fill a block of 1024 threads: x is
// read once. With DP = dim padded to a power of two (>= 64) and G = 1024 / DP, thread (fg, d) = (tid / DP, tid % DP)
// owns the fields fg, fg + G, ... of column d (at most EPT of them). Its compensated partial sum goes to LDS, the G
// partials of a column are added in order (compensated), and dx is stored from the registers.
template <typename T, bool GATHER, int EPT>
__global__ __launch_bounds__(1024) void fm_bwd_reg_kernel(const T* __restrict__ x, int64_t sb, int64_t sf,
                                                          const int64_t* __restrict__ ids, int64_t ld_ids, int64_t v_rows,
                                                          int fields, int dim, int dshift, const float* __restrict__ dout,
                                                          float* __restrict__ dx, int64_t dsb, int64_t dsf) {
    __shared__ float part[1024];  // [fg][d]: the thread's own slot
    __shared__ float Ssh[1024];   // S[d]
    const int tid = threadIdx.x, DP = 1 << dshift, G = 1024 >> dshift;
    const int d = tid & (DP - 1), fg = tid >> dshift;
    const int64_t b = blockIdx.x;
    const int64_t* idr = GATHER ? ids + b * ld_ids : nullptr;
    const T* xb = GATHER ? x : x + b * sb;
    const float nan = __uint_as_float(0x7fc00000u);
    float e[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int f = fg + G * k;
        e[k] = 0.f;
        if (d < dim && f < fields) {
            if (GATHER) {
                const int64_t r = idr[f];
                e[k] = r < 0 || r >= v_rows ? nan : ld_f32(xb + r * (int64_t)dim + d);
            } else {
                e[k] = ld_f32(xb + (int64_t)f * sf + d);
            }
        }
    }
    float s = 0.f, c = 0.f;
#pragma unroll
    for (int k = 0; k < EPT; ++k) kahan_add(s, c, e[k]);
    part[tid] = s;
    __syncthreads();
    if (tid < DP) {
        float S = 0.f, C = 0.f;
        for (int g = 0; g < G; ++g) kahan_add(S, C, part[g * DP + tid]);
        Ssh[tid] = S;
    }
    __syncthreads();
    const float S = Ssh[d], g = dout[b];
    float* o = dx + b * dsb + d;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int f = fg + G * k;
        if (d < dim && f < fields) o[(int64_t)f * dsf] = g * (S - e[k]);
    }
}

// the register kernel's shape for (fields, dim): 0 when it does not apply (a small example, or more than 32 fields per
// thread), else the elements per thread (8, 16, 32); dshift = log2 DP
inline int fm_bwd_reg_ept(int fields, int dim, int& dshift) {
    dshift = 6;
    while ((1 << dshift) < dim) ++dshift;
    const int G = 1024 >> dshift;
    const int need = (fields + G - 1) / G;
    if ((int64_t)fields << dshift < 8192 || need > 32) return 0;
    return need <= 8 ? 8 : need <= 16 ? 16 : 32;
}

template <typename T, bool GATHER>
void dispatch_fm_bwd(const void* x, int64_t sb, int64_t sf, const int64_t* ids, int64_t ld_ids, int64_t v_rows, int B,
                     int fields, int dim, const float* dout, float* dx, int64_t dsb, int64_t dsf, hipStream_t st) {
    int dshift;
    const int ept = fm_bwd_reg_ept(fields, dim, dshift);
    if (ept) {
#define RF_FMR(E)                                                                                               \
    hipLaunchKernelGGL((fm_bwd_reg_kernel<T, GATHER, E>), dim3(B), dim3(1024), 0, st, (const T*)x, sb, sf, ids, ld_ids, \
                       v_rows, fields, dim, dshift, dout, dx, dsb, dsf)
        if (ept == 8) RF_FMR(8);
        else if (ept == 16) RF_FMR(16);
        else RF_FMR(32);
#undef RF_FMR
        return;
    }
    const dim3 grid((B + 3) / 4), block(256);
#define RF_FMB(NC)                                                                                                       \
    hipLaunchKernelGGL((fm_bwd_kernel<T, GATHER, NC>), grid, block, 0, st, (const T*)x, sb, sf, ids, ld_ids, v_rows, B, \
                       fields, dim, dout, dx, dsb, dsf)
    if (dim <= 64) RF_FMB(1);
    else if (dim <= 128) RF_FMB(2);
    else if (dim <= 256) RF_FMB(4);
    else if (dim <= 512) RF_FMB(8);
    else RF_FMB(16);
#undef RF_FMB
}

// ---------------------------------------------------------------------------------------------------------------
// Cross backward
// ---------------------------------------------------------------------------------------------------------------
// x_l = c_l x_0 + beta_l with c_l = 1 + sum_{m<l} s_m and beta_l = sum_{m<l} b_m, so an example's backward follows from
// L + 1 dot products of its row: p = dout . x_0 and q_m = w_m . x_0 (t_m = beta_m . w_m does not depend on the example):
//   s_l = c_l q_l + t_l,   ds_l = p + sum_{m>l} ds_m q_m,   a_l = ds_l c_l
//   dx   = c_L dout + sum_l a_l w_l
//   dw_l = sum_b a_l x_0 + beta_l sum_b ds_l,   db_l = sum_b dout + sum_{m>l} w_m sum_b ds_m
// cross_bwd_const_kernel: t. cross_bwd_row_kernel (the forward's block shapes; x_0 and dout in registers): the dots,
// dx written once, a and ds of the example to the workspace. cross_bwd_col_kernel: over chunks of kCrossChunk
// examples, a thread owns a column and adds a_l x_0 and dout in example order. cross_bwd_reduce_kernel adds the chunks
// in order and applies beta and w. No [B][L][dim] intermediate, no atomics: the same bits on every launch.
constexpr int kCrossChunk = 128;

struct CrossWs {
    size_t t, scal, sds, part, total;  // byte offsets
    int nchunks;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

inline CrossWs cross_ws(int64_t batch, int dim, int L) {
    CrossWs l;
    l.nchunks = (int)((batch + kCrossChunk - 1) / kCrossChunk);
    l.t = 0;
    l.scal = align16(kCrossMaxLayers * sizeof(float));
    l.sds = l.scal + align16((size_t)batch * 2 * L * sizeof(float));
    l.part = l.sds + align16((size_t)l.nchunks * L * sizeof(float));
    l.total = l.part + align16((size_t)l.nchunks * (L + 1) * dim * sizeof(float));
    return l;
}

// t[l] = sum_d (sum_{m<l} b_m[d]) w_l[d]; one block per layer
__global__ __launch_bounds__(256) void cross_bwd_const_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                              int dim, float* __restrict__ t) {
    __shared__ float red[4];
    const int l = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int d0 = tid; d0 < dim; d0 += 8 * 256) {  // eight columns per pass: their loads are in flight together
        float wv[8], beta[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int d = d0 + 256 * u;
            wv[u] = d < dim ? w[(int64_t)l * dim + d] : 0.f;
            beta[u] = 0.f;
        }
        for (int m = 0; m < l; ++m) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int d = d0 + 256 * u;
                beta[u] += d < dim ? bias[(int64_t)m * dim + d] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += beta[u] * wv[u];
    }
    s = wave_sum_butterfly(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) t[l] = ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T, int THREADS, int EPT>
__global__ __launch_bounds__(THREADS) void cross_bwd_row_kernel(const T* __restrict__ x, int64_t ldx, int dim, int L,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ dout, int64_t lddo,
                                                                float* __restrict__ dx, int64_t lddx,
                                                                const float* __restrict__ t, float* __restrict__ scal) {
    constexpr int NW = THREADS / 64;
    __shared__ float red[kCrossMaxLayers + 1][NW];
    __shared__ float dots[kCrossMaxLayers + 1];  // p, q_0 .. q_{L-1}
    __shared__ float coef[kCrossMaxLayers + 1];  // a_0 .. a_{L-1}, c_L
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* xr = x + (int64_t)blockIdx.x * ldx;
    const float* gr = dout + (int64_t)blockIdx.x * lddo;
    const int ne = tid < dim ? (dim - tid + THREADS - 1) / THREADS : 0;
    float x0[EPT], g[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        x0[e] = e < ne ? ld_f32(xr + tid + e * THREADS) : 0.f;
        g[e] = e < ne ? gr[tid + e * THREADS] : 0.f;
    }
    {
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < EPT; ++e) dot += g[e] * x0[e];
        dot = wave_sum_butterfly(dot);
        if (lane == 0) red[0][wave] = dot;
    }
    for (int m = 0; m < L; ++m) {
        const float* wm = w + (int64_t)m * dim;
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            dot += x0[e] * (e < ne ? wm[tid + e * THREADS] : 0.f);
            if (e % 8 == 7) __builtin_amdgcn_sched_barrier(0);  // at most eight w loads in flight, as the forward
        }
        dot = wave_sum_butterfly(dot);
        if (lane == 0) red[m + 1][wave] = dot;
    }
    __syncthreads();
    if (tid <= L) {
        float s = red[tid][0];
#pragma unroll
        for (int v = 1; v < NW; ++v) s += red[tid][v];
        dots[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float c = 1.f;
        for (int l = 0; l < L; ++l) {
            coef[l] = c;  // c_l until the loop below replaces it with a_l
            c = c + (c * dots[l + 1] + t[l]);
        }
        coef[L] = c;
        float* sc = scal + (int64_t)blockIdx.x * 2 * L;
        float r = dots[0];
        for (int l = L - 1; l >= 0; --l) {
            const float ds = r;
            r = r + ds * dots[l + 1];
            const float a = ds * coef[l];
            coef[l] = a;
            sc[l] = a;
            sc[L + l] = ds;
        }
    }
    __syncthreads();
    const float cL = coef[L];
#pragma unroll
    for (int e = 0; e < EPT; ++e) g[e] = g[e] * cL;
    for (int m = 0; m < L; ++m) {
        const float* wm = w + (int64_t)m * dim;
        const float a = coef[m];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            g[e] = g[e] + a * (e < ne ? wm[tid + e * THREADS] : 0.f);
            if (e % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
    float* o = dx + (int64_t)blockIdx.x * lddx;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        if (e < ne) o[tid + e * THREADS] = g[e];
    }
}

// part[chunk][l][d] = sum_{b in chunk} a[b][l] x_0[b][d] (l < L), part[chunk][L][d] = sum_{b in chunk} dout[b][d],
// sds[chunk][l] = sum_{b in chunk} ds[b][l]; all in example order. LP: L padded (the accumulators are registers).
template <typename T, int LP>
__global__ __launch_bounds__(256) void cross_bwd_col_kernel(const T* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ dout, int64_t lddo, int64_t B, int dim,
                                                            int L, const float* __restrict__ scal, float* __restrict__ sds,
                                                            float* __restrict__ part) {
    constexpr int R = 8;  // rows in flight (2 R loads)
    __shared__ float a[kCrossChunk + R][LP];
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kCrossChunk;  // chunks on x: their count has no 65535 limit
    const int nb = (int)min((int64_t)kCrossChunk, B - b0);
    for (int i = tid; i < (kCrossChunk + R) * LP; i += 256) {
        const int r = i / LP, l = i % LP;
        a[r][l] = r < nb && l < L ? scal[(b0 + r) * 2 * L + l] : 0.f;
    }
    __syncthreads();
    if (blockIdx.y == 0 && tid < L) {
        float s = 0.f;
        for (int r = 0; r < nb; ++r) s += scal[(b0 + r) * 2 * L + L + tid];
        sds[(int64_t)blockIdx.x * L + tid] = s;
    }
    const int d = blockIdx.y * 256 + tid;
    if (d >= dim) return;
    float acc[LP], q = 0.f;
#pragma unroll
    for (int l = 0; l < LP; ++l) acc[l] = 0.f;
    for (int r = 0; r < nb; r += R) {
        float xv[R], gv[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const bool live = r + u < nb;  // past the chunk: a is zero there and adds nothing
            xv[u] = live ? ld_f32(x + (b0 + r + u) * ldx + d) : 0.f;
            gv[u] = live ? dout[(b0 + r + u) * lddo + d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            q += gv[u];
#pragma unroll
            for (int l = 0; l < LP; ++l) acc[l] += a[r + u][l] * xv[u];
        }
    }
    float* p = part + (int64_t)blockIdx.x * (L + 1) * dim + d;
#pragma unroll
    for (int l = 0; l < LP; ++l) {
        if (l < L) p[(int64_t)l * dim] = acc[l];
    }
    p[(int64_t)L * dim] = q;
}

// the chunks added in order, then dw_l = . + beta_l sum_b ds_l and db_l = sum_b dout + sum_{m>l} w_m sum_b ds_m
// (64 threads per block: at dim 29184 that is 456 blocks, where 256 threads would leave half of the CUs idle)
__global__ __launch_bounds__(64) void cross_bwd_reduce_kernel(const float* __restrict__ part, const float* __restrict__ sds,
                                                               int nchunks, int dim, int L, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ dw,
                                                               float* __restrict__ db) {
    __shared__ float S[kCrossMaxLayers];
    const int tid = threadIdx.x;
    if (tid < L) {
        float s = 0.f;
        for (int c = 0; c < nchunks; ++c) s += sds[(int64_t)c * L + tid];
        S[tid] = s;
    }
    __syncthreads();
    const int d = blockIdx.x * 64 + tid;
    if (d >= dim) return;
    const int64_t cs = (int64_t)(L + 1) * dim;  // one chunk of part
    float beta = 0.f;
    for (int l = 0; l < L; ++l) {
        const float* p = part + (int64_t)l * dim + d;
        float s = 0.f;
#pragma unroll 8
        for (int c = 0; c < nchunks; ++c) s += p[c * cs];
        dw[(int64_t)l * dim + d] = s + beta * S[l];
        beta += bias[(int64_t)l * dim + d];
    }
    const float* p = part + (int64_t)L * dim + d;
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) acc += p[c * cs];
    for (int l = L - 1; l >= 0; --l) {
        db[(int64_t)l * dim + d] = acc;
        acc = acc + w[(int64_t)l * dim + d] * S[l];
    }
}

template <typename T>
void dispatch_cross_bwd(const void* x, int64_t ldx, int B, int dim, int L, const float* w, const float* bias,
                        const float* dout, int64_t lddo, float* dx, int64_t lddx, float* dw, float* db, char* ws,
                        const CrossWs& lay, hipStream_t st) {
    float* t = reinterpret_cast<float*>(ws + lay.t);
    float* scal = reinterpret_cast<float*>(ws + lay.scal);
    float* sds = reinterpret_cast<float*>(ws + lay.sds);
    float* part = reinterpret_cast<float*>(ws + lay.part);
    hipLaunchKernelGGL(cross_bwd_const_kernel, dim3(L), dim3(256), 0, st, w, bias, dim, t);
#define RF_CROSSB(TH, E)                                                                                                  \
    hipLaunchKernelGGL((cross_bwd_row_kernel<T, TH, E>), dim3(B), dim3(TH), 0, st, (const T*)x, ldx, dim, L, w, dout, lddo, \
                       dx, lddx, t, scal)
    if (dim <= 256) RF_CROSSB(256, 1);
    else if (dim <= 512) RF_CROSSB(256, 2);
    else if (dim <= 1024) RF_CROSSB(256, 4);
    else if (dim <= 2048) RF_CROSSB(256, 8);
    else if (dim <= 4096) RF_CROSSB(256, 16);
    else if (dim <= 8192) RF_CROSSB(1024, 8);
    else if (dim <= 16384) RF_CROSSB(1024, 16);
    else RF_CROSSB(1024, 32);
#undef RF_CROSSB
    const dim3 grid(lay.nchunks, (dim + 255) / 256);
#define RF_CROSSC(LP)                                                                                                  \
    hipLaunchKernelGGL((cross_bwd_col_kernel<T, LP>), grid, dim3(256), 0, st, (const T*)x, ldx, dout, lddo, (int64_t)B, \
                       dim, L, scal, sds, part)
    if (L <= 4) RF_CROSSC(4);
    else if (L <= 8) RF_CROSSC(8);
    else RF_CROSSC(16);
#undef RF_CROSSC
    hipLaunchKernelGGL(cross_bwd_reduce_kernel, dim3((dim + 63) / 64), dim3(64), 0, st, part, sds, lay.nchunks, dim, L, w,
                       bias, dw, db);
}

// ---------------------------------------------------------------------------------------------------------------
// CIN
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCinMaxLayers = 8, kCinMaxF = 512, kCinMaxH = 512, kCinMaxD = 256;
constexpr int kStageVec = 1024;  // uint4 per W stage (16 KiB): KST k steps x NTC tiles x 64 lanes

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

struct CinPlan {
    int K, F0, D, dsub;   // dsub: 16-row subtiles per example
    int H[kCinMaxLayers + 1];   // H[0] = F0, H[k + 1] = sizes[k]
    int Hp[kCinMaxLayers + 1];  // padded to 8: the k index of layer k is i * Hp[k] + j
    int nks[kCinMaxLayers];     // k steps of 32
    int nt[kCinMaxLayers];      // 16-column tiles of the layer's output
    int ooff[kCinMaxLayers];    // first column of the layer in out
    int64_t woff[kCinMaxLayers + 1];  // the layer's image in the packed buffer, in uint4
    int sumH, pitch0, pitchX;
};

// sizes is a host array; returns false (and names the argument) on a limit
bool cin_plan(int fields, int dim, const int32_t* sizes, int n_layers, CinPlan& p, const char* who) {
    if (n_layers < 1 || n_layers > kCinMaxLayers) {
        rf_set_error(RF_EINVAL, "%s: n_layers (%d) must be in [1, %d]", who, n_layers, kCinMaxLayers);
        return false;
    }
    if (fields < 1 || fields > kCinMaxF) {
        rf_set_error(RF_EINVAL, "%s: fields (%d) must be in [1, %d]", who, fields, kCinMaxF);
        return false;
    }
    if (dim < 1 || dim > kCinMaxD) {
        rf_set_error(RF_EINVAL, "%s: dim (%d) must be in [1, %d]", who, dim, kCinMaxD);
        return false;
    }
    if (!sizes) {
        rf_set_error(RF_EINVAL, "%s: sizes is null", who);
        return false;
    }
    p.K = n_layers;
    p.F0 = fields;
    p.D = dim;
    p.dsub = (dim + 15) / 16;
    p.H[0] = fields;
    p.Hp[0] = pad_to(fields, 8);
    p.sumH = 0;
    p.woff[0] = 0;
    int hmax = 0;
    for (int k = 0; k < n_layers; ++k) {
        if (sizes[k] < 1 || sizes[k] > kCinMaxH) {
            rf_set_error(RF_EINVAL, "%s: sizes[%d] (%d) must be in [1, %d]", who, k, sizes[k], kCinMaxH);
            return false;
        }
        p.H[k + 1] = sizes[k];
        p.Hp[k + 1] = pad_to(sizes[k], 8);
        p.nks[k] = pad_to(fields * p.Hp[k], 32) / 32;
        p.nt[k] = (sizes[k] + 15) / 16;
        p.ooff[k] = p.sumH;
        p.sumH += sizes[k];
        p.woff[k + 1] = p.woff[k] + (int64_t)p.nks[k] * p.nt[k] * 64;
        if (k + 1 < n_layers) hmax = std::max(hmax, sizes[k]);
    }
    p.pitch0 = p.Hp[0] + 4;
    p.pitchX = pad_to(std::max(hmax, 1), 16) + 4;  // every computed column (tiles of 16) is stored
    return true;
}

// LDS of a workgroup of MS subtiles: X0, the X^k ping-pong (none for one layer, one for two) and two W stages
inline size_t cin_lds_bytes(const CinPlan& p, int ms) {
    const int nbuf = p.K >= 3 ? 2 : p.K - 1;
    return (size_t)ms * 16 * ((size_t)p.pitch0 + (size_t)nbuf * p.pitchX) * sizeof(float) + 2 * kStageVec * sizeof(uint4);
}

struct CinArgs {
    const void* x;
    int64_t sb, sf;
    int64_t n_sub;  // batch * dsub
    const uint4* wimg;
    float* part;  // [n_sub][sumH]
    CinPlan p;
    // the stashing forward of rf_cin_bwd (STASH): X^k, k < K, row-minor fp32 [pad16(H_k)][nr] (k = 0: x itself)
    float* xt[kCinMaxLayers];
    int64_t nr;
};

// image of one layer: [k step][tile][lane][8 bf16]; element e of lane l of (ks, tile) is W[k = 32 ks + 8 (l >> 4) + e]
// [n = 16 tile + (l & 15)] with k = i * Hp + j, zero where i, j or n is padding
__global__ __launch_bounds__(256) void cin_pack_kernel(const float* __restrict__ W, int F0, int Hk, int Hp, int Hn, int nt,
                                                       int64_t total, uint4* __restrict__ img) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    const int64_t kt = t >> 6;
    const int tile = (int)(kt % nt);
    const int64_t ks = kt / nt;
    const int n = tile * 16 + (lane & 15);
    const int64_t k0 = ks * 32 + 8 * (lane >> 4);
    const int i = (int)(k0 / Hp), j0 = (int)(k0 % Hp);
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = j0 + e;
        const float v = i < F0 && j < Hk && n < Hn ? W[((int64_t)i * Hk + j) * Hn + n] : 0.f;
        h[e] = f32_to_bf16_bits(v);
    }
    img[t] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

template <int MS, typename T, bool STASH = false>
__global__ __launch_bounds__(256) void cin_kernel(const CinArgs a) {
    constexpr int MT = MS * 16;           // rows of the workgroup
    constexpr int NW = 4 / MS;            // waves side by side over the output columns
    constexpr int TPW = MS == 1 ? 4 : 8;  // tiles per wave and pass
    constexpr int NTC = NW * TPW;         // tiles per pass: 8, 16, 16
    constexpr int KST = kStageVec / (NTC * 64);  // k steps per stage: 2, 1, 1
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const CinPlan& p = a.p;
    float* x0s = reinterpret_cast<float*>(smem);
    float* xs[2];
    xs[0] = x0s + MT * p.pitch0;
    xs[1] = xs[0] + MT * p.pitchX;
    const int nbuf = p.K >= 3 ? 2 : p.K - 1;
    uint4* wst = reinterpret_cast<uint4*>(x0s + MT * (p.pitch0 + nbuf * p.pitchX));

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % MS, wn = wave / MS;
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * MS;

    // X0 -> LDS [row][i], zero in the padding (i >= F0, d >= D, subtiles past the batch)
    {
        const int m = tid % MT;
        const int64_t u = u0 + m / 16;
        const int64_t b = u / p.dsub;
        const int d = (int)(u - b * p.dsub) * 16 + (m & 15);
        const bool live = u < a.n_sub && d < p.D;
        const T* xp = static_cast<const T*>(a.x) + b * a.sb + d;
        for (int i = tid / MT; i < p.Hp[0]; i += 256 / MT) {
            const float v = live && i < p.F0 ? ld_f32(xp + (int64_t)i * a.sf) : 0.f;
            x0s[m * p.pitch0 + i] = v;
            if constexpr (STASH) a.xt[0][(int64_t)i * a.nr + u0 * 16 + m] = v;
        }
    }
    __syncthreads();

    for (int k = 0; k < p.K; ++k) {
        const float* src = k == 0 ? x0s : xs[(k - 1) & 1];
        const int spitch = k == 0 ? p.pitch0 : p.pitchX;
        float* dst = xs[k & 1];
        const bool last = k + 1 == p.K;
        const int Hp = p.Hp[k], F0 = p.F0, nks = p.nks[k], NT = p.nt[k], Hn = p.H[k + 1];
        const int stepi = 32 / Hp, stepj = 32 % Hp;
        const uint4* wl = a.wimg + p.woff[k];
        const float* arow = src + (wm * 16 + lr) * spitch;
        const float* x0row = x0s + (wm * 16 + lr) * p.pitch0;
        const int nstage = (nks + KST - 1) / KST;

        for (int c0 = 0; c0 < NT; c0 += NTC) {
            const int ntc = min(NTC, NT - c0);
            f32x4 acc[TPW];
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            int i = (8 * lg) / Hp, j = (8 * lg) % Hp;

            // W stages: two in flight in registers (the stage after next is requested before this one is computed),
            // two in LDS
            uint4 pre[4], nxt[4];
            auto prefetch = [&](int s, uint4(&dr)[4]) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = tid + 256 * e;
                    const int ks = q / (NTC * 64), r = q % (NTC * 64);
                    const int kstep = s * KST + ks;
                    dr[e] = kstep < nks && r < ntc * 64 ? wl[((int64_t)kstep * NT + c0) * 64 + r] : make_uint4(0, 0, 0, 0);
                }
            };
            auto commit = [&](int buf) {
#pragma unroll
                for (int e = 0; e < 4; ++e) wst[buf * kStageVec + tid + 256 * e] = pre[e];
            };
            prefetch(0, pre);
            commit(0);
            __syncthreads();
            if (nstage > 1) prefetch(1, pre);
            for (int s = 0; s < nstage; ++s) {
                if (s + 2 < nstage) prefetch(s + 2, nxt);
                const uint4* wb = wst + (s & 1) * kStageVec;
#pragma unroll
                for (int ks = 0; ks < KST; ++ks) {
                    {
                        // no branch on the k step or the tile: past the layer's k steps and past the pass's tiles the
                        // stage holds zeros, and a branch here makes the compiler shuffle the accumulators.
                        // the A fragment: X0[i] times X^k[j .. j + 7], fp32 products rounded once to bf16
                        const float x0v = i < F0 ? x0row[i] : 0.f;
                        const float4 v0 = *reinterpret_cast<const float4*>(arow + j);
                        const float4 v1 = *reinterpret_cast<const float4*>(arow + j + 4);
                        bf16x8 af;
                        af[0] = (__bf16)(x0v * v0.x);
                        af[1] = (__bf16)(x0v * v0.y);
                        af[2] = (__bf16)(x0v * v0.z);
                        af[3] = (__bf16)(x0v * v0.w);
                        af[4] = (__bf16)(x0v * v1.x);
                        af[5] = (__bf16)(x0v * v1.y);
                        af[6] = (__bf16)(x0v * v1.z);
                        af[7] = (__bf16)(x0v * v1.w);
#pragma unroll
                        for (int t = 0; t < TPW; ++t) {
                            const int tl = wn + NW * t;  // tile of this pass
                            const bf16x8 bfr = __builtin_bit_cast(bf16x8, wb[(ks * NTC + tl) * 64 + lane]);
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[t], 0, 0, 0);
                        }
                        i += stepi;
                        j += stepj;
                        if (j >= Hp) {
                            j -= Hp;
                            ++i;
                        }
                    }
                }
                if (s + 1 < nstage) commit((s + 1) & 1);
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) pre[e] = nxt[e];
            }
            // C: column lr, rows 4 lg + r. X^{k+1} -> LDS (all 16 columns of a tile: the padding is exactly zero),
            // the subtile's row sum -> the workspace
            const int64_t u = u0 + wm;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int tl = wn + NW * t;
                if (tl < ntc) {
                    const int col = (c0 + tl) * 16 + lr;
                    if (!last) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) dst[(wm * 16 + 4 * lg + r) * p.pitchX + col] = acc[t][r];
                        if constexpr (STASH)
                            *reinterpret_cast<f32x4*>(a.xt[k + 1] + (int64_t)col * a.nr + u * 16 + 4 * lg) = acc[t];
                    }
                    float v = ((acc[t][0] + acc[t][1]) + acc[t][2]) + acc[t][3];
                    v += __shfl_xor(v, 16, 64);
                    v += __shfl_xor(v, 32, 64);
                    if (lg == 0 && col < Hn && u < a.n_sub) a.part[u * p.sumH + p.ooff[k] + col] = v;
                }
            }
        }
        __syncthreads();
    }
}

// out[b][c] = the example's subtile sums added in subtile order
__global__ __launch_bounds__(256) void cin_reduce_kernel(const float* __restrict__ part, int64_t total, int sumH, int dsub,
                                                         float* __restrict__ out, int64_t ldo) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t b = t / sumH;
    const int c = (int)(t - b * sumH);
    const float* pr = part + b * dsub * (int64_t)sumH + c;
    float s = 0.f;
    for (int u = 0; u < dsub; ++u) s += pr[(int64_t)u * sumH];
    out[b * ldo + c] = s;
}

template <int MS, typename T, bool STASH = false>
int launch_cin(const CinArgs& a, size_t lds, hipStream_t st) {
    auto kern = cin_kernel<MS, T, STASH>;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return rf_set_error(RF_EHIP, "%s: hipFuncSetAttribute: %s", STASH ? "rf_cin_bwd" : "rf_cin_fwd", hipGetErrorString(e));
    }
    // STASH: every subtile of the stash (nr / 16, a multiple of 4) is written, the ones past the batch with zeros
    const int64_t grid = STASH ? a.nr / 16 / MS : (a.n_sub + MS - 1) / MS;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, st, a);
    return RF_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// CIN backward
// ---------------------------------------------------------------------------------------------------------------
// Rows are the forward's: (example, d) pairs in 16-row subtiles, nr = 16 * (batch * dsub padded to 4) of them. The
// stashing forward (cin_kernel<.., STASH>) leaves X^k, k < K, in the workspace row-minor, fp32 [h][row]: eight
// consecutive rows of one h are contiguous, which is what both GEMMs below read. Then for k = K-1 .. 0:
//   cin_g_kernel     G^{k+1} = dout + dX^{k+1} rounded once to bf16, row-minor [h][row], zero on the padding (d >= D,
//                    subtiles past the batch, h >= H_{k+1}): those rows add exactly zero to dW and to dx.
//   cin_dz_kernel    one wave per subtile, MS waves per workgroup. For a field i and 16 consecutive j the dZ tile
//                    [16 rows][16 j] = G (A operand, bf16 fragments in LDS) x W_k^T (B operand, the image of
//                    rf_cin_bwd_pack_w read in place) stays in the accumulators; dX^k[row][j] += X0[row][i] acc (in
//                    registers across the i loop) and dX0[row][i] += sum_j X^k[row][j] acc (a 16-lane DPP tree, then
//                    added in (j tile) order into the wave's own LDS column). dZ is never written.
//   cin_dw_kernel    D[m = j][n = h] += sum_rows A[j][row] B[row][h]: a lane's A fragment is X0^T[i][8 rows] times
//                    X^k^T[j][8 rows], fp32 products rounded once; B is G^T[h][8 rows]. A workgroup owns four fields (one
//                    per wave), four j tiles and all h, and walks one row chunk; the partial goes to the workspace.
//   cin_dw_reduce_kernel adds the chunks in order into dW_k and drops the padding.
// The chunk length depends only on nr: max(1024, nr / 16 rounded up to 32) rows, at most 16 chunks beyond 16384 rows.
constexpr int kCinDwMinChunk = 1024, kCinDwChunks = 16;

struct CinBwdPlan {
    int64_t nr;      // rows of every stash (a multiple of 64)
    int64_t chunk;   // rows per dW chunk (a multiple of 32)
    int nchunks;
    int nj[kCinMaxLayers];   // 16-wide j tiles of layer k: ceil(H_k / 16)
    int nkh[kCinMaxLayers];  // k steps of 32 over h: ceil(H_{k+1} / 32)
    int64_t wtoff[kCinMaxLayers + 1];  // the layer's transposed image, in uint4
    size_t part, xt[kCinMaxLayers], dxt[kCinMaxLayers], gt, slab, total;  // byte offsets (dxt[0] unused)
    size_t slab_elems;  // floats of one chunk's partial: max_k F0 * pad16(H_k) * pad16(H_{k+1})
};

inline void cin_bwd_images(const CinPlan& p, CinBwdPlan& q) {
    q.wtoff[0] = 0;
    for (int k = 0; k < p.K; ++k) {
        q.nj[k] = (p.H[k] + 15) / 16;
        q.nkh[k] = (p.H[k + 1] + 31) / 32;
        q.wtoff[k + 1] = q.wtoff[k] + (int64_t)p.F0 * q.nj[k] * q.nkh[k] * 64;
    }
}

inline void cin_bwd_plan(const CinPlan& p, int64_t batch, CinBwdPlan& q) {
    cin_bwd_images(p, q);
    const int64_t n_sub = batch * p.dsub;
    q.nr = std::max<int64_t>((n_sub + 3) / 4 * 4, 4) * 16;
    q.chunk = std::max<int64_t>(kCinDwMinChunk, ((q.nr + kCinDwChunks - 1) / kCinDwChunks + 31) / 32 * 32);
    q.nchunks = (int)((q.nr + q.chunk - 1) / q.chunk);
    size_t off = 0;
    q.part = off;
    off += align16((size_t)std::max<int64_t>(n_sub, 1) * p.sumH * sizeof(float));
    int hn32 = 0;
    q.slab_elems = 0;
    for (int k = 0; k < p.K; ++k) {
        const size_t bytes = (size_t)pad_to(p.H[k], 16) * q.nr * sizeof(float);
        q.xt[k] = off;
        off += bytes;
        q.dxt[k] = off;
        if (k > 0) off += bytes;
        hn32 = std::max(hn32, pad_to(p.H[k + 1], 32));
        q.slab_elems = std::max(q.slab_elems, (size_t)p.F0 * pad_to(p.H[k], 16) * pad_to(p.H[k + 1], 16));
    }
    q.gt = off;
    off += (size_t)hn32 * q.nr * sizeof(uint16_t);
    q.slab = off;
    off += (size_t)q.nchunks * q.slab_elems * sizeof(float);
    q.total = off;
}

// LDS of one wave of cin_dz_kernel: X0 and dX0 as fp32 [i][16 rows], G as bf16 [16 rows][32 nkh + 8]
__host__ __device__ inline size_t cin_dz_lds_bytes(int F0, int nkh) { return (size_t)F0 * 16 * 4 * 2 + (size_t)16 * (32 * nkh + 8) * 2; }

// transposed image of one layer: [i][j tile][k step over h][lane][8 bf16]; element e of lane l is
// W[(i H_k + j)][h] with j = 16 tile + (l & 15), h = 32 ks + 8 (l >> 4) + e, zero where j or h is padding
__global__ __launch_bounds__(256) void cin_pack_t_kernel(const float* __restrict__ W, int Hk, int Hn, int nj, int nkh,
                                                         int64_t total, uint4* __restrict__ img) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    int64_t q = t >> 6;
    const int ks = (int)(q % nkh);
    q /= nkh;
    const int jt = (int)(q % nj);
    const int64_t i = q / nj;
    const int j = jt * 16 + (lane & 15);
    const int h0 = ks * 32 + 8 * (lane >> 4);
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = j < Hk && h0 + e < Hn ? W[(i * Hk + j) * Hn + h0 + e] : 0.f;
        h[e] = f32_to_bf16_bits(v);
    }
    img[t] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// gt[h][row .. row + 7] for h < hn32: a thread owns eight consecutive rows (one example) of one h
__global__ __launch_bounds__(256) void cin_g_kernel(const float* __restrict__ dout, int64_t lddo, int ooff, int Hn, int hn32,
                                                    const float* __restrict__ dxn, int64_t nr, int64_t n_sub, int dsub,
                                                    int D, uint4* __restrict__ gt) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n8 = nr / 8;
    if (t >= n8 * hn32) return;
    const int h = (int)(t / n8);
    const int64_t row0 = (t - (int64_t)h * n8) * 8;
    const int64_t u = row0 / 16;
    const int64_t b = u / dsub;
    const int d0 = (int)(u - b * dsub) * 16 + (int)(row0 & 15);
    uint32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0;
    if (h < Hn && u < n_sub && d0 < D) {
        const float g = dout[b * lddo + ooff + h];
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
        if (dxn) {
            const float4 a0 = *reinterpret_cast<const float4*>(dxn + (int64_t)h * nr + row0);
            const float4 a1 = *reinterpret_cast<const float4*>(dxn + (int64_t)h * nr + row0 + 4);
            a[0] = a0.x, a[1] = a0.y, a[2] = a0.z, a[3] = a0.w;
            a[4] = a1.x, a[5] = a1.y, a[6] = a1.z, a[7] = a1.w;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (d0 + e < D) v[e] = f32_to_bf16_bits(g + a[e]);
        }
    }
    gt[t] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}

struct CinDzArgs {
    const float* x0t;   // [.][nr]
    const float* xkt;   // [pad16(H_k)][nr] (layer 0: x0t)
    const uint16_t* gt;  // [32 nkh][nr]
    const uint4* wt;    // the layer's transposed image
    float* dxkt;        // [pad16(H_k)][nr], layers >= 1
    float* dx;
    int64_t dsb, dsf, nr, n_sub;
    int F0, Hk, nj, nkh, dsub, D, layer0, first;
};

// NK: the layer's k steps over h (nkh) rounded up to a power of two. The wave's A fragments (G) stay in registers for
// the whole kernel; the B fragments of UI fields are requested together, so that one trip to L2 is paid per UI fields
// and not per field (a wave per SIMD hides nothing by itself: the LDS of X0 and dX0 allows no second one).
template <int NK>
__global__ __launch_bounds__(256) void cin_dz_kernel(const CinDzArgs a) {
    constexpr int UI = NK <= 4 ? 8 : 32 / NK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lg = lane >> 4;
    const int F0 = a.F0, nkh = a.nkh, gp = 32 * nkh + 8;  // gp: pitch of G in bf16 (16 bytes past a multiple of 64)
    char* mine = smem + (size_t)wave * cin_dz_lds_bytes(F0, nkh);
    float* x0s = reinterpret_cast<float*>(mine);  // [i][16]
    float* dx0s = x0s + F0 * 16;                   // [i][16]
    uint16_t* gs = reinterpret_cast<uint16_t*>(dx0s + F0 * 16);  // [16][gp]
    const int64_t u = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;  // < nr / 16
    const int64_t row0 = u * 16;

    for (int q = lane; q < F0 * 16; q += 64) {
        x0s[q] = a.x0t[(int64_t)(q >> 4) * a.nr + row0 + (q & 15)];
        dx0s[q] = 0.f;
    }
    for (int q = lane; q < 32 * nkh * 16; q += 64) {
        const int h = q >> 4, m = q & 15;
        gs[m * gp + h] = a.gt[(int64_t)h * a.nr + row0 + m];
    }
    wave_lds_sync();

    // A: G[row lr][h = 32 ks + 8 lg + e]; zero past the layer's k steps (the B fragment there is a repeat)
    bf16x8 af[NK];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ks < nkh) v = *reinterpret_cast<const uint4*>(gs + lr * gp + 8 * lg + 32 * ks);
        af[ks] = __builtin_bit_cast(bf16x8, v);
    }
    const int64_t istride = (int64_t)a.nj * nkh * 64;  // uint4 per field of the image
    for (int jt = 0; jt < a.nj; ++jt) {
        const int j = jt * 16 + lr;
        f32x4 xk = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < a.Hk) xk = *reinterpret_cast<const f32x4*>(a.xkt + (int64_t)j * a.nr + row0 + 4 * lg);
        f32x4 dxk = f32x4{0.f, 0.f, 0.f, 0.f};
        const uint4* wb = a.wt + (int64_t)jt * nkh * 64 + lane;
        for (int i0 = 0; i0 < F0; i0 += UI) {
            uint4 bw[UI][NK];
#pragma unroll
            for (int v = 0; v < UI; ++v) {
                const uint4* wi = wb + (int64_t)min(i0 + v, F0 - 1) * istride;
#pragma unroll
                for (int ks = 0; ks < NK; ++ks) {
                    const uint4 w = wi[min(ks, nkh - 1) * 64];
                    bw[v][ks] = ks < nkh ? w : make_uint4(0, 0, 0, 0);
                }
            }
#pragma unroll
            for (int v = 0; v < UI; ++v) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < NK; ++ks)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], __builtin_bit_cast(bf16x8, bw[v][ks]), acc, 0, 0, 0);
                // acc: dZ[row 4 lg + r][i, j]
                const int i = i0 + v;
                if (i < F0) {
                    const f32x4 x0v = *reinterpret_cast<const f32x4*>(x0s + i * 16 + 4 * lg);
                    f32x4 t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        dxk[r] += x0v[r] * acc[r];
                        t[r] = xk[r] * acc[r];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] = row16_sum(t[r]);
                    if (lr == 0) {
                        f32x4* p = reinterpret_cast<f32x4*>(dx0s + i * 16 + 4 * lg);
                        *p = *p + t;
                    }
                }
            }
        }
        if (a.layer0) {
            // X^0 is both factors: the j side lands in dx too
            wave_lds_sync();
            if (j < F0) {
                f32x4* p = reinterpret_cast<f32x4*>(dx0s + j * 16 + 4 * lg);
                *p = *p + dxk;
            }
            wave_lds_sync();
        } else {
            *reinterpret_cast<f32x4*>(a.dxkt + (int64_t)j * a.nr + row0 + 4 * lg) = dxk;
        }
    }
    wave_lds_sync();
    if (u >= a.n_sub) return;
    const int64_t b = u / a.dsub;
    const int dbase = (int)(u - b * a.dsub) * 16;
    float* dxb = a.dx + b * a.dsb + dbase;
    for (int q = lane; q < F0 * 16; q += 64) {
        const int i = q >> 4, m = q & 15;
        if (dbase + m < a.D) {
            float* o = dxb + (int64_t)i * a.dsf + m;
            *o = a.first ? dx0s[q] : *o + dx0s[q];
        }
    }
}

template <int NK>
int launch_cin_dz(const CinDzArgs& z, int ms, size_t lds, hipStream_t st) {
    auto kern = cin_dz_kernel<NK>;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return rf_set_error(RF_EHIP, "rf_cin_bwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(z.nr / 16 / ms)), dim3(64 * ms), lds, st, z);
    return RF_OK;
}

struct CinDwArgs {
    const float* x0t;
    const float* xkt;
    const uint4* gt;  // bf16 [32 nkh][nr], eight rows per uint4
    float* slab;      // [nchunks][F0][16 nj][16 nh]
    int64_t nr, chunk, slab_elems;
    int F0, Hk, nj, nh, njg;  // nh: 16-wide h tiles; njg: groups of four j tiles
};

// A workgroup owns four fields (one per wave) and four j tiles; a wave's G fragments of a 32-row step are loaded once
// and used for its four j tiles (32 MFMAs per 8 + 10 fragment loads), and the waves' G and X^k loads hit the same lines.
__global__ __launch_bounds__(256) void cin_dw_kernel(const CinDwArgs a) {
    constexpr int TPW = 8, PJ = 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lg = lane >> 4;
    const int i = (blockIdx.x / a.njg) * 4 + wave;
    const int jt0 = (blockIdx.x % a.njg) * PJ;
    if (i >= a.F0) return;  // no barrier below
    const int64_t r0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t r1 = min(r0 + a.chunk, a.nr);
    const float* xi = a.x0t + (int64_t)i * a.nr + 8 * lg;
    const float* xj[PJ];
    bool jlive[PJ];
#pragma unroll
    for (int pj = 0; pj < PJ; ++pj) {
        const int j = (jt0 + pj) * 16 + lr;
        jlive[pj] = j < a.Hk;  // also false for a tile past nj
        xj[pj] = a.xkt + (int64_t)(jlive[pj] ? j : 0) * a.nr + 8 * lg;
    }
    const int64_t n8 = a.nr / 8;
    const int ldo = a.nh * 16;
    float* out = a.slab + (int64_t)blockIdx.y * a.slab_elems + ((int64_t)i * a.nj + jt0) * 16 * ldo;
    for (int hp = 0; hp < a.nh; hp += TPW) {
        f32x4 acc[PJ][TPW];
#pragma unroll
        for (int pj = 0; pj < PJ; ++pj) {
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[pj][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int64_t row = r0; row < r1; row += 32) {
            const float4 p0 = *reinterpret_cast<const float4*>(xi + row);
            const float4 p1 = *reinterpret_cast<const float4*>(xi + row + 4);
            const uint4* gp = a.gt + (row >> 3) + lg;
            bf16x8 bfr[TPW];
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int ht = min(hp + t, a.nh - 1);  // past the last tile: a repeat whose accumulator is dropped
                bfr[t] = __builtin_bit_cast(bf16x8, gp[(int64_t)(ht * 16 + lr) * n8]);
            }
#pragma unroll
            for (int pj = 0; pj < PJ; ++pj) {
                float4 q0 = *reinterpret_cast<const float4*>(xj[pj] + row);
                float4 q1 = *reinterpret_cast<const float4*>(xj[pj] + row + 4);
                if (!jlive[pj]) q0 = q1 = make_float4(0.f, 0.f, 0.f, 0.f);
                bf16x8 af;
                af[0] = (__bf16)(p0.x * q0.x);
                af[1] = (__bf16)(p0.y * q0.y);
                af[2] = (__bf16)(p0.z * q0.z);
                af[3] = (__bf16)(p0.w * q0.w);
                af[4] = (__bf16)(p1.x * q1.x);
                af[5] = (__bf16)(p1.y * q1.y);
                af[6] = (__bf16)(p1.z * q1.z);
                af[7] = (__bf16)(p1.w * q1.w);
#pragma unroll
                for (int t = 0; t < TPW; ++t)
                    acc[pj][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[t], acc[pj][t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int pj = 0; pj < PJ; ++pj) {
            if (jt0 + pj < a.nj) {
#pragma unroll
                for (int t = 0; t < TPW; ++t) {
                    if (hp + t < a.nh) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            out[(pj * 16 + 4 * lg + r) * (int64_t)ldo + (hp + t) * 16 + lr] = acc[pj][t][r];
                    }
                }
            }
        }
    }
}

// dW[(i H_k + j)][h] = the chunks' partials added in chunk order
__global__ __launch_bounds__(256) void cin_dw_reduce_kernel(const float* __restrict__ slab, int64_t slab_elems, int nchunks,
                                                            int Hk, int Hn, int nj, int nh, int64_t total,
                                                            float* __restrict__ dW) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int h = (int)(t % Hn);
    const int64_t ij = t / Hn;
    const int j = (int)(ij % Hk);
    const int64_t i = ij / Hk;
    const float* p = slab + ((i * nj * 16 + j) * (int64_t)(nh * 16)) + h;
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += p[(int64_t)c * slab_elems];
    dW[t] = s;
}

}  // namespace

extern "C" int rf_fm_fwd(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t x_stride_f, const float* V,
                         const int64_t* ids, int64_t ld_ids, int64_t v_rows, int32_t batch, int32_t fields, int32_t dim,
                         const float* w0, const float* w, const int64_t* w_ids, int32_t n, int64_t ld_wids, int64_t w_rows,
                         float* out, void* stream) {
    RF_REQUIRE(batch >= 0, "rf_fm_fwd: batch must be >= 0");
    RF_REQUIRE(dim >= 1 && dim <= kFmMaxDim, "rf_fm_fwd: dim (%d) must be in [1, %d]", dim, kFmMaxDim);
    RF_REQUIRE(fields >= 1 && fields <= kFmMaxFields, "rf_fm_fwd: fields (%d) must be in [1, %d]", fields, kFmMaxFields);
    RF_REQUIRE(n >= 0 && n <= kFmMaxFields, "rf_fm_fwd: n (%d) must be in [0, %d]", n, kFmMaxFields);
    RF_REQUIRE((x != nullptr) != (V != nullptr), "rf_fm_fwd: give exactly one of x (dense) and V (gathered)");
    if (x) {
        RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_fm_fwd: x_dtype must be F32 or BF16");
        RF_REQUIRE(x_stride_f >= dim && x_stride_b >= 0, "rf_fm_fwd: x_stride_f must be >= dim");
    } else {
        RF_REQUIRE(ids && ld_ids >= fields && v_rows >= 1, "rf_fm_fwd: the gathered form needs ids, ld_ids >= fields, v_rows >= 1");
    }
    RF_REQUIRE(!w || (w_ids && ld_wids >= n && w_rows >= 1), "rf_fm_fwd: w needs w_ids, ld_wids >= n, w_rows >= 1");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(out, "rf_fm_fwd: out is null");
    hipStream_t st = rf_stream(stream);
    const dim3 grid((batch + 3) / 4), block(256);
#define RF_FM(T, G, XP)                                                                                                    \
    hipLaunchKernelGGL((fm_kernel<T, G>), grid, block, 0, st, (const T*)(XP), x_stride_b, x_stride_f, ids, ld_ids, v_rows, \
                       batch, fields, dim, w0, w, w_ids, n, ld_wids, w_rows, out)
    if (V) RF_FM(float, true, V);
    else if (x_dtype == RF_DTYPE_F32) RF_FM(float, false, x);
    else RF_FM(uint16_t, false, x);
#undef RF_FM
    return rf_check_launch("rf_fm_fwd");
}

extern "C" int rf_cross_fwd(const void* x, int32_t x_dtype, int64_t ldx, int32_t batch, int32_t dim, int32_t n_layers,
                            const float* w, const float* b, float* out, int64_t ldo, void* stream) {
    RF_REQUIRE(batch >= 0, "rf_cross_fwd: batch must be >= 0");
    RF_REQUIRE(n_layers >= 1 && n_layers <= kCrossMaxLayers, "rf_cross_fwd: n_layers (%d) must be in [1, %d]", n_layers, kCrossMaxLayers);
    RF_REQUIRE(dim >= 1 && dim <= kCrossMaxDim, "rf_cross_fwd: dim (%d) must be in [1, %d]", dim, kCrossMaxDim);
    RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_cross_fwd: x_dtype must be F32 or BF16");
    RF_REQUIRE(ldx >= dim && ldo >= dim, "rf_cross_fwd: ldx and ldo must be >= dim");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && w && b && out, "rf_cross_fwd: null pointer");
    hipStream_t st = rf_stream(stream);
    if (x_dtype == RF_DTYPE_F32) dispatch_cross<float>(x, ldx, batch, dim, n_layers, w, b, out, ldo, st);
    else dispatch_cross<uint16_t>(x, ldx, batch, dim, n_layers, w, b, out, ldo, st);
    return rf_check_launch("rf_cross_fwd");
}

extern "C" size_t rf_cin_packed_w_bytes(int32_t fields, const int32_t* sizes, int32_t n_layers) {
    CinPlan p;
    if (!cin_plan(fields, 1, sizes, n_layers, p, "rf_cin_packed_w_bytes")) return 0;
    return (size_t)p.woff[n_layers] * sizeof(uint4);
}

extern "C" size_t rf_cin_ws_bytes(int32_t batch, int32_t fields, int32_t dim, const int32_t* sizes, int32_t n_layers) {
    CinPlan p;
    if (batch < 0 || !cin_plan(fields, dim, sizes, n_layers, p, "rf_cin_ws_bytes")) return 0;
    return std::max<size_t>((size_t)batch * p.dsub * p.sumH * sizeof(float), 16);
}

extern "C" int rf_cin_pack_w(const float* W, int32_t layer, int32_t fields, const int32_t* sizes, int32_t n_layers,
                             void* packed, void* stream) {
    CinPlan p;
    if (!cin_plan(fields, 1, sizes, n_layers, p, "rf_cin_pack_w")) return RF_EINVAL;
    RF_REQUIRE(layer >= 0 && layer < n_layers, "rf_cin_pack_w: layer (%d) must be in [0, %d)", layer, n_layers);
    RF_REQUIRE(W && packed && ((uintptr_t)packed & 15) == 0, "rf_cin_pack_w: null pointer or packed not 16-byte aligned");
    const int64_t total = p.woff[layer + 1] - p.woff[layer];
    hipLaunchKernelGGL(cin_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, rf_stream(stream), W, p.F0,
                       p.H[layer], p.Hp[layer], p.H[layer + 1], p.nt[layer], total,
                       static_cast<uint4*>(packed) + p.woff[layer]);
    return rf_check_launch("rf_cin_pack_w");
}

extern "C" int rf_cin_fwd(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t x_stride_f, int32_t batch,
                          int32_t fields, int32_t dim, const int32_t* sizes, int32_t n_layers, const void* packed_w,
                          float* out, int64_t ldo, void* ws, size_t ws_bytes, void* stream) {
    CinArgs a{};
    if (!cin_plan(fields, dim, sizes, n_layers, a.p, "rf_cin_fwd")) return RF_EINVAL;
    RF_REQUIRE(batch >= 0, "rf_cin_fwd: batch must be >= 0");
    RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_cin_fwd: x_dtype must be F32 or BF16");
    RF_REQUIRE(x_stride_f >= dim && x_stride_b >= 0, "rf_cin_fwd: x_stride_f must be >= dim");
    RF_REQUIRE(ldo >= a.p.sumH, "rf_cin_fwd: ldo must be >= sum(sizes)");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && packed_w && out, "rf_cin_fwd: null pointer");
    RF_REQUIRE(((uintptr_t)packed_w & 15) == 0, "rf_cin_fwd: packed_w must be 16-byte aligned");
    RF_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "rf_cin_fwd: null or misaligned workspace");
    RF_REQUIRE(ws_bytes >= rf_cin_ws_bytes(batch, fields, dim, sizes, n_layers), "rf_cin_fwd: ws_bytes too small");
    a.x = x;
    a.sb = x_stride_b;
    a.sf = x_stride_f;
    a.n_sub = (int64_t)batch * a.p.dsub;
    a.wimg = static_cast<const uint4*>(packed_w);
    a.part = static_cast<float*>(ws);
    RF_REQUIRE(a.n_sub < ((int64_t)1 << 31), "rf_cin_fwd: batch * dim too large");
    hipStream_t st = rf_stream(stream);
    int ms = 4;
    while (ms > 1 && cin_lds_bytes(a.p, ms) > 160 * 1024) ms >>= 1;
    const size_t lds = cin_lds_bytes(a.p, ms);
    RF_REQUIRE(lds <= 160 * 1024, "rf_cin_fwd: needs %zu bytes of LDS (> 160 KiB)", lds);
    const bool f32 = x_dtype == RF_DTYPE_F32;
    int rc;
    if (ms == 4) rc = f32 ? launch_cin<4, float>(a, lds, st) : launch_cin<4, uint16_t>(a, lds, st);
    else if (ms == 2) rc = f32 ? launch_cin<2, float>(a, lds, st) : launch_cin<2, uint16_t>(a, lds, st);
    else rc = f32 ? launch_cin<1, float>(a, lds, st) : launch_cin<1, uint16_t>(a, lds, st);
    if (rc != RF_OK) return rc;
    const int64_t total = (int64_t)batch * a.p.sumH;
    hipLaunchKernelGGL(cin_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.part, total, a.p.sumH,
                       a.p.dsub, out, ldo);
    return rf_check_launch("rf_cin_fwd");
}

extern "C" int rf_fm_bwd(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t x_stride_f, const float* V,
                         const int64_t* ids, int64_t ld_ids, int64_t v_rows, int32_t batch, int32_t fields, int32_t dim,
                         const float* dout, float* dx, int64_t dx_stride_b, int64_t dx_stride_f, void* stream) {
    RF_REQUIRE(batch >= 0, "rf_fm_bwd: batch must be >= 0");
    RF_REQUIRE(dim >= 1 && dim <= kFmMaxDim, "rf_fm_bwd: dim (%d) must be in [1, %d]", dim, kFmMaxDim);
    RF_REQUIRE(fields >= 1 && fields <= kFmMaxFields, "rf_fm_bwd: fields (%d) must be in [1, %d]", fields, kFmMaxFields);
    RF_REQUIRE((x != nullptr) != (V != nullptr), "rf_fm_bwd: give exactly one of x (dense) and V (gathered)");
    if (x) {
        RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_fm_bwd: x_dtype must be F32 or BF16");
        RF_REQUIRE(x_stride_f >= dim && x_stride_b >= 0, "rf_fm_bwd: x_stride_f must be >= dim");
    } else {
        RF_REQUIRE(ids && ld_ids >= fields && v_rows >= 1, "rf_fm_bwd: the gathered form needs ids, ld_ids >= fields, v_rows >= 1");
    }
    RF_REQUIRE(dx_stride_f >= dim && dx_stride_b >= (int64_t)(fields - 1) * dx_stride_f + dim,
               "rf_fm_bwd: dx_stride_f must be >= dim and dx_stride_b >= (fields - 1) * dx_stride_f + dim");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(dout && dx, "rf_fm_bwd: dout or dx is null");
    hipStream_t st = rf_stream(stream);
    if (V) dispatch_fm_bwd<float, true>(V, 0, 0, ids, ld_ids, v_rows, batch, fields, dim, dout, dx, dx_stride_b, dx_stride_f, st);
    else if (x_dtype == RF_DTYPE_F32)
        dispatch_fm_bwd<float, false>(x, x_stride_b, x_stride_f, nullptr, 0, 0, batch, fields, dim, dout, dx, dx_stride_b, dx_stride_f, st);
    else
        dispatch_fm_bwd<uint16_t, false>(x, x_stride_b, x_stride_f, nullptr, 0, 0, batch, fields, dim, dout, dx, dx_stride_b, dx_stride_f, st);
    return rf_check_launch("rf_fm_bwd");
}

extern "C" size_t rf_cross_bwd_ws_bytes(int32_t batch, int32_t dim, int32_t n_layers) {
    if (batch < 0 || dim < 1 || dim > kCrossMaxDim || n_layers < 1 || n_layers > kCrossMaxLayers) return 0;
    return cross_ws(batch, dim, n_layers).total;
}

extern "C" int rf_cross_bwd(const void* x, int32_t x_dtype, int64_t ldx, int32_t batch, int32_t dim, int32_t n_layers,
                            const float* w, const float* b, const float* dout, int64_t lddo, float* dx, int64_t lddx,
                            float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(batch >= 0, "rf_cross_bwd: batch must be >= 0");
    RF_REQUIRE(n_layers >= 1 && n_layers <= kCrossMaxLayers, "rf_cross_bwd: n_layers (%d) must be in [1, %d]", n_layers, kCrossMaxLayers);
    RF_REQUIRE(dim >= 1 && dim <= kCrossMaxDim, "rf_cross_bwd: dim (%d) must be in [1, %d]", dim, kCrossMaxDim);
    RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_cross_bwd: x_dtype must be F32 or BF16");
    RF_REQUIRE(ldx >= dim && lddo >= dim && lddx >= dim, "rf_cross_bwd: ldx, lddo and lddx must be >= dim");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && w && b && dout && dx && dw && db, "rf_cross_bwd: null pointer");
    RF_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "rf_cross_bwd: null or misaligned workspace");
    const CrossWs lay = cross_ws(batch, dim, n_layers);
    RF_REQUIRE(ws_bytes >= lay.total, "rf_cross_bwd: ws_bytes too small (%zu < %zu)", ws_bytes, lay.total);
    hipStream_t st = rf_stream(stream);
    if (x_dtype == RF_DTYPE_F32)
        dispatch_cross_bwd<float>(x, ldx, batch, dim, n_layers, w, b, dout, lddo, dx, lddx, dw, db, static_cast<char*>(ws), lay, st);
    else
        dispatch_cross_bwd<uint16_t>(x, ldx, batch, dim, n_layers, w, b, dout, lddo, dx, lddx, dw, db, static_cast<char*>(ws), lay, st);
    return rf_check_launch("rf_cross_bwd");
}

extern "C" size_t rf_cin_bwd_packed_w_bytes(int32_t fields, const int32_t* sizes, int32_t n_layers) {
    CinPlan p;
    if (!cin_plan(fields, 1, sizes, n_layers, p, "rf_cin_bwd_packed_w_bytes")) return 0;
    CinBwdPlan q;
    cin_bwd_images(p, q);
    return (size_t)q.wtoff[n_layers] * sizeof(uint4);
}

extern "C" size_t rf_cin_bwd_ws_bytes(int32_t batch, int32_t fields, int32_t dim, const int32_t* sizes, int32_t n_layers) {
    CinPlan p;
    if (batch < 0 || !cin_plan(fields, dim, sizes, n_layers, p, "rf_cin_bwd_ws_bytes")) return 0;
    CinBwdPlan q;
    cin_bwd_plan(p, batch, q);
    return q.total;
}

extern "C" int rf_cin_bwd_pack_w(const float* W, int32_t layer, int32_t fields, const int32_t* sizes, int32_t n_layers,
                                 void* packed_t, void* stream) {
    CinPlan p;
    if (!cin_plan(fields, 1, sizes, n_layers, p, "rf_cin_bwd_pack_w")) return RF_EINVAL;
    RF_REQUIRE(layer >= 0 && layer < n_layers, "rf_cin_bwd_pack_w: layer (%d) must be in [0, %d)", layer, n_layers);
    RF_REQUIRE(W && packed_t && ((uintptr_t)packed_t & 15) == 0,
               "rf_cin_bwd_pack_w: null pointer or packed_t not 16-byte aligned");
    CinBwdPlan q;
    cin_bwd_images(p, q);
    const int64_t total = q.wtoff[layer + 1] - q.wtoff[layer];
    hipLaunchKernelGGL(cin_pack_t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, rf_stream(stream), W,
                       p.H[layer], p.H[layer + 1], q.nj[layer], q.nkh[layer], total,
                       static_cast<uint4*>(packed_t) + q.wtoff[layer]);
    return rf_check_launch("rf_cin_bwd_pack_w");
}

extern "C" int rf_cin_bwd(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t x_stride_f, int32_t batch,
                          int32_t fields, int32_t dim, const int32_t* sizes, int32_t n_layers, const void* packed_w,
                          const void* packed_w_t, const float* dout, int64_t lddo, float* dx, int64_t dx_stride_b,
                          int64_t dx_stride_f, float* const* dW, void* ws, size_t ws_bytes, void* stream) {
    CinArgs a{};
    if (!cin_plan(fields, dim, sizes, n_layers, a.p, "rf_cin_bwd")) return RF_EINVAL;
    const CinPlan& p = a.p;
    RF_REQUIRE(batch >= 0, "rf_cin_bwd: batch must be >= 0");
    RF_REQUIRE(x_dtype == RF_DTYPE_F32 || x_dtype == RF_DTYPE_BF16, "rf_cin_bwd: x_dtype must be F32 or BF16");
    RF_REQUIRE(x_stride_f >= dim && x_stride_b >= 0, "rf_cin_bwd: x_stride_f must be >= dim");
    RF_REQUIRE(lddo >= p.sumH, "rf_cin_bwd: lddo must be >= sum(sizes)");
    RF_REQUIRE(dx_stride_f >= dim && dx_stride_b >= (int64_t)(fields - 1) * dx_stride_f + dim,
               "rf_cin_bwd: dx_stride_f must be >= dim and dx_stride_b >= (fields - 1) * dx_stride_f + dim");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && packed_w && packed_w_t && dout && dx && dW, "rf_cin_bwd: null pointer");
    for (int k = 0; k < n_layers; ++k) RF_REQUIRE(dW[k], "rf_cin_bwd: dW[%d] is null", k);
    RF_REQUIRE(((uintptr_t)packed_w & 15) == 0, "rf_cin_bwd: packed_w must be 16-byte aligned");
    RF_REQUIRE(((uintptr_t)packed_w_t & 15) == 0, "rf_cin_bwd: packed_w_t must be 16-byte aligned");
    RF_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "rf_cin_bwd: null or misaligned workspace");
    CinBwdPlan q;
    cin_bwd_plan(p, batch, q);
    RF_REQUIRE(ws_bytes >= q.total, "rf_cin_bwd: ws_bytes too small (%zu < %zu)", ws_bytes, q.total);
    RF_REQUIRE(q.nr < ((int64_t)1 << 31), "rf_cin_bwd: batch * dim too large");
    int ms = 4;
    while (ms > 1 && cin_lds_bytes(p, ms) > 160 * 1024) ms >>= 1;
    const size_t lds = cin_lds_bytes(p, ms);
    RF_REQUIRE(lds <= 160 * 1024, "rf_cin_bwd: the recomputing forward needs %zu bytes of LDS (> 160 KiB)", lds);
    int zms[kCinMaxLayers];
    for (int k = 0; k < n_layers; ++k) {
        zms[k] = 4;
        while (zms[k] > 1 && zms[k] * cin_dz_lds_bytes(p.F0, q.nkh[k]) > 160 * 1024) zms[k] >>= 1;
        const size_t need = zms[k] * cin_dz_lds_bytes(p.F0, q.nkh[k]);
        RF_REQUIRE(need <= 160 * 1024, "rf_cin_bwd: layer %d needs %zu bytes of LDS (> 160 KiB)", k, need);
    }
    char* w8 = static_cast<char*>(ws);
    hipStream_t st = rf_stream(stream);

    // the forward again, X^k (k < K) to the workspace
    a.x = x;
    a.sb = x_stride_b;
    a.sf = x_stride_f;
    a.n_sub = (int64_t)batch * p.dsub;
    a.wimg = static_cast<const uint4*>(packed_w);
    a.part = reinterpret_cast<float*>(w8 + q.part);
    a.nr = q.nr;
    for (int k = 0; k < n_layers; ++k) a.xt[k] = reinterpret_cast<float*>(w8 + q.xt[k]);
    const bool f32 = x_dtype == RF_DTYPE_F32;
    int rc;
    if (ms == 4) rc = f32 ? launch_cin<4, float, true>(a, lds, st) : launch_cin<4, uint16_t, true>(a, lds, st);
    else if (ms == 2) rc = f32 ? launch_cin<2, float, true>(a, lds, st) : launch_cin<2, uint16_t, true>(a, lds, st);
    else rc = f32 ? launch_cin<1, float, true>(a, lds, st) : launch_cin<1, uint16_t, true>(a, lds, st);
    if (rc != RF_OK) return rc;

    uint4* gt = reinterpret_cast<uint4*>(w8 + q.gt);
    float* slab = reinterpret_cast<float*>(w8 + q.slab);
    for (int k = n_layers - 1; k >= 0; --k) {
        const int Hk = p.H[k], Hn = p.H[k + 1], hn32 = 32 * q.nkh[k];
        const float* dxn = k + 1 < n_layers ? reinterpret_cast<const float*>(w8 + q.dxt[k + 1]) : nullptr;
        const int64_t gtotal = q.nr / 8 * hn32;
        hipLaunchKernelGGL(cin_g_kernel, dim3((unsigned)((gtotal + 255) / 256)), dim3(256), 0, st, dout, lddo, p.ooff[k], Hn,
                           hn32, dxn, q.nr, a.n_sub, p.dsub, p.D, gt);

        CinDzArgs z;
        z.x0t = a.xt[0];
        z.xkt = a.xt[k];
        z.gt = reinterpret_cast<const uint16_t*>(gt);
        z.wt = static_cast<const uint4*>(packed_w_t) + q.wtoff[k];
        z.dxkt = k > 0 ? reinterpret_cast<float*>(w8 + q.dxt[k]) : nullptr;
        z.dx = dx;
        z.dsb = dx_stride_b;
        z.dsf = dx_stride_f;
        z.nr = q.nr;
        z.n_sub = a.n_sub;
        z.F0 = p.F0;
        z.Hk = Hk;
        z.nj = q.nj[k];
        z.nkh = q.nkh[k];
        z.dsub = p.dsub;
        z.D = p.D;
        z.layer0 = k == 0;
        z.first = k == n_layers - 1;
        const size_t zlds = zms[k] * cin_dz_lds_bytes(p.F0, q.nkh[k]);
        int rcz;
        if (z.nkh <= 1) rcz = launch_cin_dz<1>(z, zms[k], zlds, st);
        else if (z.nkh <= 2) rcz = launch_cin_dz<2>(z, zms[k], zlds, st);
        else if (z.nkh <= 4) rcz = launch_cin_dz<4>(z, zms[k], zlds, st);
        else if (z.nkh <= 8) rcz = launch_cin_dz<8>(z, zms[k], zlds, st);
        else rcz = launch_cin_dz<16>(z, zms[k], zlds, st);
        if (rcz != RF_OK) return rcz;

        CinDwArgs w;
        w.x0t = a.xt[0];
        w.xkt = a.xt[k];
        w.gt = gt;
        w.slab = slab;
        w.nr = q.nr;
        w.chunk = q.chunk;
        w.slab_elems = (int64_t)q.slab_elems;
        w.Hk = Hk;
        w.nj = q.nj[k];
        w.nh = (Hn + 15) / 16;
        w.F0 = p.F0;
        w.njg = (w.nj + 3) / 4;
        hipLaunchKernelGGL(cin_dw_kernel, dim3((unsigned)((p.F0 + 3) / 4 * w.njg), (unsigned)q.nchunks), dim3(256), 0, st, w);
        const int64_t total = (int64_t)p.F0 * Hk * Hn;
        hipLaunchKernelGGL(cin_dw_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slab,
                           (int64_t)q.slab_elems, q.nchunks, Hk, Hn, w.nj, w.nh, total, dW[k]);
    }
    return rf_check_launch("rf_cin_bwd");
}
