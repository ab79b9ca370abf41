// rf_fusion.hip — Que2Search AttentionFusion forward and backward (backend/layers/fusion_layers.py:35-46):
//   att = softmax(concat(x_1..x_C) @ W)            W: [C*d][C] (the Keras weight as stored)
//   out = sum_c att_c * x_c, then l2-normalised when is_norm
// One wave per example: the C logits are C dot products of length C*d (lanes stride the K axis,
// xor-shuffle reductions), the softmax and the weighted channel sum stay in registers. fp32 throughout.
// Backward (rf_attention_fusion_bwd): a row pass of the same one-wave-per-example shape (u, ss recomputed from x and
// the saved att; writes g_u = dL/du and the logit gradient dl), then a column pass with one lane per column of x that
// keeps its W row in registers over a fixed batch chunk: dx, and dW = x^T dl as one partial [C*d][C] slab per chunk,
// summed in chunk order: no atomics, the same bits on every launch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rf_common.h"
#include "rf_wave.h"

namespace {

constexpr int kMaxC = 16;

__global__ __launch_bounds__(256) void fusion_kernel(const float* __restrict__ x, int B, int C, int d, int64_t ldx,
                                                     const float* __restrict__ W, int is_norm, float* __restrict__ out,
                                                     int64_t ldo, float* __restrict__ att_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* xr = x + b * ldx;
    const int K = C * d;
    float logit[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) logit[c] = 0.f;
    for (int kx = lane; kx < K; kx += 64) {
        const float xv = xr[kx];
        const float* wr = W + (int64_t)kx * C;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
            if (c < C) logit[c] += xv * wr[c];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
        if (c < C) {
            logit[c] = wave_sum_butterfly(logit[c]);
            mx = fmaxf(mx, logit[c]);
        }
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
        if (c < C) {
            logit[c] = expf(logit[c] - mx);
            z += logit[c];
        }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
        if (c < C) logit[c] /= z;
    if (att_out && lane < C) {
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
            if (c == lane) att_out[b * C + c] = logit[c];
    }
    // weighted channel sum (lane owns columns lane, lane + 64, ...), then the row norm
    float ss = 0.f;
    for (int j = lane; j < d; j += 64) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
            if (c < C) acc += logit[c] * xr[(int64_t)c * d + j];
        out[b * ldo + j] = acc;
        ss += acc * acc;
    }
    if (is_norm) {
        // tf.nn.l2_normalize: x * rsqrt(max(sum(x^2), 1e-12))
        const float inv = rsqrtf(fmaxf(wave_sum_butterfly(ss), 1e-12f));
        for (int j = lane; j < d; j += 64) out[b * ldo + j] *= inv;
    }
}

// Backward, row pass: one wave per example. g_u = dL/du (u = sum_c a_c x_c, before the l2 normalisation):
//   is_norm: r = rsqrt(max(ss, 1e-12)); g_u = r g - r^3 (u.g) u when ss >= 1e-12, else r g (the clamp passes no gradient)
//   s_c = g_u . x_c; dl_c = a_c (s_c - sum_c' a_c' s_c')
// Writes g_u [B][ldgu] and dl [B][C] to the workspace for the column pass.
template <int C>
__global__ __launch_bounds__(256) void fusion_bwd_row_kernel(const float* __restrict__ x, int B, int d, int64_t ldx,
                                                             int is_norm, const float* __restrict__ att,
                                                             const float* __restrict__ g, int64_t ldg,
                                                             float* __restrict__ gu_out, int64_t ldgu,
                                                             float* __restrict__ dl_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* xr = x + b * ldx;
    const float* gr = g + b * ldg;
    float* gur = gu_out + b * ldgu;
    float a[C];
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = att[b * C + c];
    float r = 1.f, coef = 0.f;
    if (is_norm) {
        float ss = 0.f, ug = 0.f;
        for (int j = lane; j < d; j += 64) {
            float u = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) u = fmaf(a[c], xr[(int64_t)c * d + j], u);
            ss = fmaf(u, u, ss);
            ug = fmaf(u, gr[j], ug);
        }
        ss = wave_sum_butterfly(ss);
        ug = wave_sum_butterfly(ug);
        r = rsqrtf(fmaxf(ss, 1e-12f));
        coef = ss >= 1e-12f ? r * r * r * ug : 0.f;
    }
    float s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.f;
    for (int j = lane; j < d; j += 64) {
        float xv[C];
        float u = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xv[c] = xr[(int64_t)c * d + j];
            u = fmaf(a[c], xv[c], u);
        }
        const float gu = is_norm ? r * gr[j] - coef * u : gr[j];
        gur[j] = gu;
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] = fmaf(gu, xv[c], s[c]);
    }
    float sbar = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        s[c] = wave_sum_butterfly(s[c]);
        sbar = fmaf(a[c], s[c], sbar);
    }
    if (lane < C) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == lane) dl_out[b * C + c] = a[c] * (s[c] - sbar);
    }
}

// Backward, column pass: a block owns 64 columns k = c d + j of x (lane = column, its W row in registers) and one batch
// chunk; its 4 waves take the chunk's examples b0 + wave, b0 + wave + 4, ... in order (dl[b][.] is wave-uniform: scalar
// loads), four examples' loads in flight:
//   dx[b][k] = a[b][c] g_u[b][j] + sum_c' dl[b][c'] W[k][c']
//   DW: the chunk's partial dW[k][c'] = sum_b x[b][k] dl[b][c'], the four waves' sums added in wave order through LDS.
template <int C, bool DW>
__global__ __launch_bounds__(256) void fusion_bwd_col_kernel(const float* __restrict__ x, int B, int64_t K, int d,
                                                             int64_t ldx, const float* __restrict__ W,
                                                             const float* __restrict__ att, const float* __restrict__ gu,
                                                             int64_t ldgu, const float* __restrict__ dl, int rows,
                                                             float* __restrict__ dx, int64_t lddx,
                                                             float* __restrict__ part) {
    __shared__ float red[DW ? 3 : 1][C][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    const bool live = k < K;
    const int64_t kc = live ? k : K - 1;  // lanes past K read the last column and write nothing
    const int c = (int)(kc / d);
    const int j = (int)(kc - (int64_t)c * d);
    float w[C];
#pragma unroll
    for (int c2 = 0; c2 < C; ++c2) w[c2] = W[kc * C + c2];
    const float* xk = x + kc;
    const float* guj = gu + j;
    const float* ac = att + c;
    float* dxk = dx + kc;
    const int64_t b0 = (int64_t)blockIdx.y * rows;
    const int64_t b1 = b0 + rows < B ? b0 + rows : B;
    float acc[C];
#pragma unroll
    for (int c2 = 0; c2 < C; ++c2) acc[c2] = 0.f;
    int64_t b = b0 + wave;
    for (; b + 12 < b1; b += 16) {
        float xv[4], gv[4], av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t bi = b + 4 * i;
            xv[i] = DW ? xk[bi * ldx] : 0.f;
            gv[i] = guj[bi * ldgu];
            av[i] = ac[bi * C];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t bi = b + 4 * i;
            const float* dr = dl + bi * C;
            float o = av[i] * gv[i];
#pragma unroll
            for (int c2 = 0; c2 < C; ++c2) o = fmaf(dr[c2], w[c2], o);
            if (live) dxk[bi * lddx] = o;
            if (DW) {
#pragma unroll
                for (int c2 = 0; c2 < C; ++c2) acc[c2] = fmaf(xv[i], dr[c2], acc[c2]);
            }
        }
    }
    for (; b < b1; b += 4) {
        const float* dr = dl + b * C;
        float o = ac[b * C] * guj[b * ldgu];
#pragma unroll
        for (int c2 = 0; c2 < C; ++c2) o = fmaf(dr[c2], w[c2], o);
        if (live) dxk[b * lddx] = o;
        if (DW) {
            const float xv = xk[b * ldx];
#pragma unroll
            for (int c2 = 0; c2 < C; ++c2) acc[c2] = fmaf(xv, dr[c2], acc[c2]);
        }
    }
    if (DW) {
        if (wave) {
#pragma unroll
            for (int c2 = 0; c2 < C; ++c2) red[wave - 1][c2][lane] = acc[c2];
        }
        __syncthreads();
        if (wave == 0 && live) {
            float* p = part + ((int64_t)blockIdx.y * K + k) * C;
#pragma unroll
            for (int c2 = 0; c2 < C; ++c2) p[c2] = ((acc[c2] + red[0][c2][lane]) + red[1][c2][lane]) + red[2][c2][lane];
        }
    }
}

// dW[i] = the chunks' partials summed in chunk order.
__global__ __launch_bounds__(256) void fusion_dw_sum_kernel(const float* __restrict__ part, int64_t n, int nchunks,
                                                            float* __restrict__ dW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
#pragma unroll 8
    for (int ch = 0; ch < nchunks; ++ch) s += part[(int64_t)ch * n + i];
    dW[i] = s;
}

// The batch chunks of the column pass: a function of the batch alone (not of the device), at most 64 chunks of at
// least 32 rows.
inline void dw_chunks(int64_t B, int& nchunks, int& rows) {
    int64_t n = std::min<int64_t>(64, (B + 31) / 32);
    n = std::max<int64_t>(n, 1);
    rows = (int)((B + n - 1) / n);
    rows = std::max(rows, 1);
    nchunks = (int)std::max<int64_t>((B + rows - 1) / rows, 1);
}

// workspace: g_u [B][pad4(d)] | dl [B][C] | the chunk partials [nchunks][C*d][C] (each part a multiple of 4 floats)
inline int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }

template <int C>
void launch_bwd(const float* x, int B, int d, int64_t ldx, const float* W, int is_norm, const float* att, const float* g,
                int64_t ldg, float* dx, int64_t lddx, float* dW, float* ws, hipStream_t st) {
    const int64_t K = (int64_t)C * d, ldgu = pad4(d);
    float* gu = ws;
    float* dl = gu + (int64_t)B * ldgu;
    float* part = dl + pad4((int64_t)B * C);
    int nchunks, rows;
    dw_chunks(B, nchunks, rows);
    const dim3 grid((unsigned)((K + 63) / 64), nchunks);
    hipLaunchKernelGGL(fusion_bwd_row_kernel<C>, dim3((B + 3) / 4), dim3(256), 0, st, x, B, d, ldx, is_norm, att, g, ldg, gu,
                       ldgu, dl);
    if (!dW) {
        hipLaunchKernelGGL((fusion_bwd_col_kernel<C, false>), grid, dim3(256), 0, st, x, B, K, d, ldx, W, att, gu, ldgu, dl,
                           rows, dx, lddx, part);
        return;
    }
    hipLaunchKernelGGL((fusion_bwd_col_kernel<C, true>), grid, dim3(256), 0, st, x, B, K, d, ldx, W, att, gu, ldgu, dl, rows,
                       dx, lddx, part);
    hipLaunchKernelGGL(fusion_dw_sum_kernel, dim3((unsigned)((K * C + 255) / 256)), dim3(256), 0, st, part, K * C, nchunks,
                       dW);
}

}  // namespace

extern "C" int rf_attention_fusion_fwd(const float* x, int32_t batch, int32_t channels, int32_t dim, int64_t ldx,
                                       const float* W, int32_t is_norm, float* out, int64_t ldo, float* att_out,
                                       void* stream) {
    RF_REQUIRE(batch >= 0 && channels >= 1 && channels <= kMaxC && dim >= 1, "rf_attention_fusion_fwd: need 1 <= channels <= 16");
    RF_REQUIRE(ldx >= (int64_t)channels * dim && ldo >= dim, "rf_attention_fusion_fwd: bad leading dimension");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && W && out, "rf_attention_fusion_fwd: null pointer");
    hipLaunchKernelGGL(fusion_kernel, dim3((batch + 3) / 4), dim3(256), 0, rf_stream(stream), x, batch, channels, dim, ldx,
                       W, is_norm, out, ldo, att_out);
    return rf_check_launch("rf_attention_fusion_fwd");
}

extern "C" size_t rf_attention_fusion_bwd_ws_bytes(int32_t batch, int32_t channels, int32_t dim) {
    if (batch < 0 || channels < 1 || channels > kMaxC || dim < 1) return 16;
    int nchunks, rows;
    dw_chunks(batch, nchunks, rows);
    const int64_t KC = (int64_t)channels * dim * channels;
    return (size_t)((int64_t)batch * pad4(dim) + pad4((int64_t)batch * channels) + (int64_t)nchunks * KC + 4) * sizeof(float);
}

extern "C" int rf_attention_fusion_bwd(const float* x, int32_t batch, int32_t channels, int32_t dim, int64_t ldx,
                                       const float* W, int32_t is_norm, const float* att, const float* dout, int64_t ldg,
                                       float* dx, int64_t lddx, float* dW, void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(batch >= 0 && channels >= 1 && channels <= kMaxC && dim >= 1, "rf_attention_fusion_bwd: need 1 <= channels <= 16");
    RF_REQUIRE((int64_t)channels * dim * channels < ((int64_t)1 << 31), "rf_attention_fusion_bwd: channels * dim too large");
    RF_REQUIRE(ldx >= (int64_t)channels * dim && lddx >= (int64_t)channels * dim && ldg >= dim,
               "rf_attention_fusion_bwd: bad leading dimension");
    if (batch == 0) return RF_OK;
    RF_REQUIRE(x && W && att && dout && dx, "rf_attention_fusion_bwd: null pointer");
    RF_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "rf_attention_fusion_bwd: null or misaligned workspace");
    RF_REQUIRE(ws_bytes >= rf_attention_fusion_bwd_ws_bytes(batch, channels, dim), "rf_attention_fusion_bwd: ws_bytes too small");
    hipStream_t st = rf_stream(stream);
    float* wsf = static_cast<float*>(ws);
    switch (channels) {
#define RF_FUSION_BWD_CASE(C)                                                                                  \
    case C:                                                                                                    \
        launch_bwd<C>(x, batch, dim, ldx, W, is_norm, att, dout, ldg, dx, lddx, dW, wsf, st);                  \
        break;
        RF_FUSION_BWD_CASE(1) RF_FUSION_BWD_CASE(2) RF_FUSION_BWD_CASE(3) RF_FUSION_BWD_CASE(4)
        RF_FUSION_BWD_CASE(5) RF_FUSION_BWD_CASE(6) RF_FUSION_BWD_CASE(7) RF_FUSION_BWD_CASE(8)
        RF_FUSION_BWD_CASE(9) RF_FUSION_BWD_CASE(10) RF_FUSION_BWD_CASE(11) RF_FUSION_BWD_CASE(12)
        RF_FUSION_BWD_CASE(13) RF_FUSION_BWD_CASE(14) RF_FUSION_BWD_CASE(15) RF_FUSION_BWD_CASE(16)
#undef RF_FUSION_BWD_CASE
    }
    return rf_check_launch("rf_attention_fusion_bwd");
}
