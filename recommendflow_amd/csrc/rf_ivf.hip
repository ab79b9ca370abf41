// rf_ivf.hip — IVF-Flat approximate search (FaissSearcher "IVF{nlist},Flat"; the reference hands the string to
// faiss.index_factory, backend/third_party_components/faiss_searcher.py:107-122):
//   rf_ivf_build_lists  inverted lists from a list id per item: a stable counting sort (ids ascend inside a list)
//   rf_ivf_list_mean    the k-means centroid update: per-list mean of the rows in list order, optionally l2-normalised
//   rf_ivf_scan_f32     the list scan: exact fp32 scores of every (query, probed list) pair's items, list-major
// Everything here is replay-deterministic: no result depends on the arrival order of atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rf_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// build lists
// ---------------------------------------------------------------------------------------------
// The items are cut into C contiguous chunks. cnt[c][l] = items of chunk c in list l (integer atomics: the counts
// do not depend on the order), turned into each chunk's start inside its list (prefix over c), list_off = prefix of
// the totals over l; then one workgroup per chunk walks its items IN ORDER, 256 at a time, and places every item at
// list_off[l] + cnt[c][l] + (items of the same list earlier in the tile): stable, so ids ascend inside a list.
constexpr int kBuildThreads = 256;
constexpr int kBuildChunkMin = 512;       // items per chunk at least (2 tiles)
constexpr int kBuildMaxChunks = 512;
constexpr int64_t kBuildMaxCells = (int64_t)1 << 23;  // C * nlist counters at most (32 MiB)
constexpr int kMaxLists = 32768;

int build_chunks(int64_t n, int nlist) {
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kBuildMaxChunks, kBuildMaxCells / nlist));
    return (int)std::max<int64_t>(1, std::min<int64_t>(cap, (n + kBuildChunkMin - 1) / kBuildChunkMin));
}

__global__ __launch_bounds__(kBuildThreads) void ivf_hist_kernel(const int32_t* __restrict__ assign, int64_t n, int nlist,
                                                                 int64_t chunk_len, uint32_t* __restrict__ cnt) {
    const int c = blockIdx.x;
    const int64_t i0 = c * chunk_len, i1 = min(n, i0 + chunk_len);
    uint32_t* row = cnt + (int64_t)c * nlist;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBuildThreads) {
        const int l = assign[i];
        if (l >= 0 && l < nlist) atomicAdd(&row[l], 1u);
    }
}

// cnt[c][l] -> items of list l in chunks before c; tot[l] = the list's size
__global__ __launch_bounds__(256) void ivf_chunk_prefix_kernel(uint32_t* __restrict__ cnt, int C, int nlist,
                                                               uint32_t* __restrict__ tot) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nlist) return;
    uint32_t run = 0;
    for (int c = 0; c < C; ++c) {
        const uint32_t v = cnt[(int64_t)c * nlist + l];
        cnt[(int64_t)c * nlist + l] = run;
        run += v;
    }
    tot[l] = run;
}

// list_off[0 .. nlist] = exclusive prefix of tot[0 .. nlist) (one workgroup; nlist <= 32768 = 1024 threads x 32)
__global__ __launch_bounds__(1024) void ivf_list_off_kernel(const uint32_t* __restrict__ tot, int nlist,
                                                            int32_t* __restrict__ list_off) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    const int l0 = t * per, l1 = min(nlist, l0 + per);
    uint32_t s = 0;
    for (int l = l0; l < l1; ++l) s += tot[l];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan
        const uint32_t y = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int l = l0; l < l1; ++l) {
        list_off[l] = (int32_t)run;
        run += tot[l];
    }
    if (t == 1023) list_off[nlist] = (int32_t)part[1023];
}

__global__ __launch_bounds__(kBuildThreads) void ivf_scatter_kernel(const int32_t* __restrict__ assign, int64_t n, int nlist,
                                                                    int64_t chunk_len, uint32_t* __restrict__ cnt,
                                                                    const int32_t* __restrict__ list_off,
                                                                    uint32_t* __restrict__ list_ids) {
    __shared__ __attribute__((aligned(16))) int sid[kBuildThreads];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t i0 = c * chunk_len, i1 = min(n, i0 + chunk_len);
    uint32_t* row = cnt + (int64_t)c * nlist;
    for (int64_t b = i0; b < i1; b += kBuildThreads) {  // uniform over the workgroup
        const int64_t i = b + t;
        int l = i < i1 ? assign[i] : -1;
        if (l >= nlist) l = -1;  // out of range: the caller's error, dropped rather than written out of bounds
        sid[t] = l;
        __syncthreads();
        uint32_t next = 0;
        bool last = false;
        if (l >= 0) {
            const uint32_t base = row[l];  // written by this workgroup only, in an earlier tile
            // one pass over the tile's ids (the same LDS address in every lane: broadcast reads, four ids each)
            int before = 0, after = 0;
#pragma unroll 8
            for (int j4 = 0; j4 < kBuildThreads / 4; ++j4) {
                const int4 s = *reinterpret_cast<const int4*>(&sid[4 * j4]);
                const int j = 4 * j4;
                before += (s.x == l && j < t) + (s.y == l && j + 1 < t) + (s.z == l && j + 2 < t) + (s.w == l && j + 3 < t);
                after += (s.x == l && j > t) + (s.y == l && j + 1 > t) + (s.z == l && j + 2 > t) + (s.w == l && j + 3 > t);
            }
            last = after == 0;
            list_ids[(int64_t)list_off[l] + base + before] = (uint32_t)i;
            next = base + before + 1;
        }
        __syncthreads();  // every read of row[] of this tile is done
        if (last) row[l] = next;  // the tile's last item of list l: the list's fill after this tile
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// list mean
// ---------------------------------------------------------------------------------------------
// One workgroup per list. CT = min(K, 256) column threads x RL = 256 / CT row lanes; the list's rows are cut into
// chunks of 32, row lane r sums the chunks r, r + RL, ... (each chunk summed in row order, then added to the lane's
// total) and the lanes' totals are added in lane order: the partition is a function of K and the list's length
// only, so the bits are the same on every launch.
constexpr int kMeanThreads = 256;
constexpr int kMeanChunk = 32;
constexpr int kMeanMaxK = 1024;

__global__ __launch_bounds__(kMeanThreads) void ivf_list_mean_kernel(const float* __restrict__ rows, int K,
                                                                     const int32_t* __restrict__ list_off, int normalize,
                                                                     float* __restrict__ centroids) {
    __shared__ float part[kMeanThreads];
    __shared__ float mean[kMeanMaxK];
    const int l = blockIdx.x, t = threadIdx.x;
    const int64_t r0 = list_off[l];
    const int len = list_off[l + 1] - list_off[l];
    if (len <= 0) return;  // an empty list keeps its centroid
    const int CT = min(K, kMeanThreads), RL = kMeanThreads / CT;
    const int ct = t % CT, rl = t / CT;
    for (int kb = 0; kb < K; kb += CT) {
        const int k = kb + ct;
        float s = 0.f;
        if (rl < RL && k < K)
            for (int c0 = rl * kMeanChunk; c0 < len; c0 += RL * kMeanChunk) {
                float cs = 0.f;
                const int c1 = min(len, c0 + kMeanChunk);
                for (int r = c0; r < c1; ++r) cs += rows[(r0 + r) * K + k];
                s += cs;
            }
        part[t] = s;
        __syncthreads();
        if (rl == 0 && k < K) {
            float a = part[ct];
            for (int j = 1; j < RL; ++j) a += part[j * CT + ct];
            mean[k] = a / (float)len;
        }
        __syncthreads();
    }
    float inv = 1.f;
    if (normalize) {
        float s = 0.f;
        for (int k = t; k < K; k += kMeanThreads) s += mean[k] * mean[k];
        part[t] = s;
        __syncthreads();
        for (int o = kMeanThreads / 2; o > 0; o >>= 1) {  // fixed tree
            if (t < o) part[t] += part[t + o];
            __syncthreads();
        }
        const float n2 = part[0];
        if (n2 > 0.f) inv = sqrtf(n2);
        else normalize = 0;
    }
    for (int k = t; k < K; k += kMeanThreads) centroids[(int64_t)l * K + k] = normalize ? mean[k] / inv : mean[k];
}

// ---------------------------------------------------------------------------------------------
// list scan
// ---------------------------------------------------------------------------------------------
// grid (S, G): workgroup (s, g) takes the rows 32 (s + S i) .. + 31 of group g's list against every query that probes
// it, 16 queries (one zero-padded tile, gathered through pair_q) at a time. Two waves, 16 list rows each: one
// v_mfma_f32_16x16x4_f32 per 4 k with A = the query tile, B = the wave's rows, both read from LDS one float per lane
// (A[i = lane & 15][k = 4 s + (lane >> 4)]) so that k ascends along the MFMA chain: a score is the fmaf chain over
// k = 0 .. K-1 of its own query row and item row, whatever else shares the tile. K goes through LDS in spans of 256
// (row stride span + 4 floats: the 16 rows x 4 k of one read fall on 64 distinct banks when the span is a multiple
// of 64). With K <= 256 the rows are staged once per 32-row chunk and reused by every query tile, so a list is read
// from HBM once; a deeper K re-stages them per query tile (the later reads of the chunk hit L2).
constexpr int kScanThreads = 128;
constexpr int kScanRows = 32;
constexpr int kScanQ = 16;
constexpr int kScanKC = 256;
constexpr int kScanMaxSplit = 1024;
constexpr int kScanBatch = kScanRows * (kScanKC / 4) / kScanThreads;  // item float4 per thread and span (16)
constexpr int kScanQBatch = kScanQ * (kScanKC / 4) / kScanThreads;    // query float4 per thread and span (8)
typedef float scan_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kScanThreads) void ivf_scan_kernel(const float* __restrict__ q, int64_t ldq,
                                                                const float* __restrict__ items, int K,
                                                                const int32_t* __restrict__ list_off,
                                                                const uint32_t* __restrict__ list_ids,
                                                                const int32_t* __restrict__ grp_list,
                                                                const int32_t* __restrict__ grp_off,
                                                                const int32_t* __restrict__ pair_q,
                                                                const int32_t* __restrict__ pair_col,
                                                                float* __restrict__ cand_val, uint32_t* __restrict__ cand_idx,
                                                                int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) float scan_smem[];
    const int g = blockIdx.y;
    const int l = grp_list[g];
    const int64_t r0 = list_off[l];
    const int len = list_off[l + 1] - list_off[l];
    const int p0 = grp_off[g], np = grp_off[g + 1] - p0;
    if (len <= 0 || np <= 0) return;
    const int kspan = min(K, kScanKC), KS = kspan + 4;
    float* qs = scan_smem;                  // [16][KS]
    float* its = scan_smem + kScanQ * KS;   // [32][KS]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int ntile = (np + kScanQ - 1) / kScanQ;
    const int nkc = (K + kScanKC - 1) / kScanKC;
    const bool resident = nkc == 1;
    for (int rc = blockIdx.x * kScanRows; rc < len; rc += gridDim.x * kScanRows) {  // uniform over the workgroup
        const int nrows = min(kScanRows, len - rc);
        for (int tile = 0; tile < ntile; ++tile) {
            scan_f4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int kc = 0; kc < nkc; ++kc) {
                const int k0 = kc * kScanKC;
                const int kw = min(kScanKC, K - k0), kw4 = kw >> 2;
                __syncthreads();  // the MFMA reads of the previous span are done
                // staging: a span holds at most 32 x 64 item float4 and 16 x 64 query float4, 16 and 8 per thread. The
                // queries' row numbers are loaded first, then every item load and query load is issued before the
                // first LDS store, so one span costs about one trip to memory
                const int sh = (kw4 & (kw4 - 1)) == 0 ? __builtin_ctz(kw4) : -1;  // span width a power of two: no division
                const bool items_too = !(resident && tile > 0);
                int qrow[kScanQBatch];
#pragma unroll
                for (int u = 0; u < kScanQBatch; ++u) {
                    const int e = t + u * kScanThreads;
                    const int i = sh >= 0 ? e >> sh : e / kw4;
                    const int pi = tile * kScanQ + i;
                    qrow[u] = (i < kScanQ && pi < np) ? pair_q[p0 + pi] : -1;
                }
                float4 v[kScanBatch], w[kScanQBatch];
                const float* src = items + (r0 + rc) * K + k0;
#pragma unroll
                for (int u = 0; u < kScanBatch; ++u) {
                    const int e = t + u * kScanThreads;
                    const int r = sh >= 0 ? e >> sh : e / kw4, c4 = e - r * kw4;
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (items_too && r < nrows) v[u] = *reinterpret_cast<const float4*>(src + (int64_t)r * K + 4 * c4);
                }
#pragma unroll
                for (int u = 0; u < kScanQBatch; ++u) {
                    const int e = t + u * kScanThreads;
                    const int i = sh >= 0 ? e >> sh : e / kw4, c4 = e - i * kw4;
                    w[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (qrow[u] >= 0) w[u] = *reinterpret_cast<const float4*>(q + (int64_t)qrow[u] * ldq + k0 + 4 * c4);
                }
                if (items_too) {
#pragma unroll
                    for (int u = 0; u < kScanBatch; ++u) {
                        const int e = t + u * kScanThreads;
                        const int r = sh >= 0 ? e >> sh : e / kw4, c4 = e - r * kw4;
                        if (r < kScanRows) *reinterpret_cast<float4*>(its + r * KS + 4 * c4) = v[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < kScanQBatch; ++u) {
                    const int e = t + u * kScanThreads;
                    const int i = sh >= 0 ? e >> sh : e / kw4, c4 = e - i * kw4;
                    if (i < kScanQ) *reinterpret_cast<float4*>(qs + i * KS + 4 * c4) = w[u];
                }
                __syncthreads();
                if (wave * 16 < nrows) {  // wave-uniform
                    const float* ap = qs + (lane & 15) * KS + (lane >> 4);
                    const float* bp = its + (wave * 16 + (lane & 15)) * KS + (lane >> 4);
                    int s = 0;
                    for (; s + 8 <= kw4; s += 8) {  // 16 LDS reads in flight, then the chain of 8 MFMAs (k ascending)
                        float a[8], b[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            a[u] = ap[4 * (s + u)];
                            b[u] = bp[4 * (s + u)];
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
                    }
                    for (; s < kw4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * s], bp[4 * s], acc, 0, 0, 0);
                }
            }
            // C layout: column (lane & 15) = the list row, row 4 (lane >> 4) + e = the query of the tile
            const int j = rc + wave * 16 + (lane & 15);
            if (j < len) {
                const uint32_t id = list_ids[r0 + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int pi = tile * kScanQ + 4 * (lane >> 4) + e;
                    if (pi < np) {
                        const int64_t o = (int64_t)pair_q[p0 + pi] * ld + pair_col[p0 + pi] + j;
                        cand_val[o] = acc[e];
                        cand_idx[o] = id;
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" size_t rf_ivf_build_ws_bytes(int64_t n, int32_t nlist) {
    if (n < 0 || nlist < 1 || nlist > kMaxLists) return 0;
    return ((size_t)build_chunks(n, nlist) + 1) * (size_t)nlist * sizeof(uint32_t);
}

extern "C" int rf_ivf_build_lists(const int32_t* assign, int64_t n, int32_t nlist, int32_t* list_off, uint32_t* list_ids,
                                  void* ws, size_t ws_bytes, void* stream) {
    RF_REQUIRE(nlist >= 1 && nlist <= kMaxLists, "rf_ivf_build_lists: nlist must be in [1, %d]", kMaxLists);
    RF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "rf_ivf_build_lists: n must be in [0, 2^31)");
    RF_REQUIRE(ws_bytes >= rf_ivf_build_ws_bytes(n, nlist), "rf_ivf_build_lists: workspace too small");
    RF_REQUIRE(list_off && ws && (n == 0 || (assign && list_ids)), "rf_ivf_build_lists: null pointer");
    hipStream_t st = rf_stream(stream);
    const int C = build_chunks(n, nlist);
    const int64_t chunk_len = std::max<int64_t>(1, (n + C - 1) / C);
    uint32_t* cnt = static_cast<uint32_t*>(ws);
    uint32_t* tot = cnt + (size_t)C * nlist;
    const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)C * nlist * sizeof(uint32_t), st);
    if (e != hipSuccess) return rf_set_error(RF_EHIP, "rf_ivf_build_lists: %s", hipGetErrorString(e));
    if (n > 0) hipLaunchKernelGGL(ivf_hist_kernel, dim3(C), dim3(kBuildThreads), 0, st, assign, n, nlist, chunk_len, cnt);
    hipLaunchKernelGGL(ivf_chunk_prefix_kernel, dim3((nlist + 255) / 256), dim3(256), 0, st, cnt, C, nlist, tot);
    hipLaunchKernelGGL(ivf_list_off_kernel, dim3(1), dim3(1024), 0, st, tot, nlist, list_off);
    if (n > 0)
        hipLaunchKernelGGL(ivf_scatter_kernel, dim3(C), dim3(kBuildThreads), 0, st, assign, n, nlist, chunk_len, cnt, list_off,
                           list_ids);
    return rf_check_launch("rf_ivf_build_lists");
}

extern "C" int rf_ivf_list_mean(const float* rows_sorted, int32_t K, const int32_t* list_off, int32_t nlist,
                                int32_t normalize, float* centroids, void* stream) {
    RF_REQUIRE(K >= 1 && K <= kMeanMaxK, "rf_ivf_list_mean: K must be in [1, %d]", kMeanMaxK);
    RF_REQUIRE(nlist >= 1 && nlist <= kMaxLists, "rf_ivf_list_mean: nlist must be in [1, %d]", kMaxLists);
    RF_REQUIRE(normalize == 0 || normalize == 1, "rf_ivf_list_mean: normalize must be 0 or 1");
    RF_REQUIRE(rows_sorted && list_off && centroids, "rf_ivf_list_mean: null pointer");
    hipLaunchKernelGGL(ivf_list_mean_kernel, dim3(nlist), dim3(kMeanThreads), 0, rf_stream(stream), rows_sorted, K, list_off,
                       normalize, centroids);
    return rf_check_launch("rf_ivf_list_mean");
}

extern "C" int rf_ivf_scan_f32(const float* q, int64_t ldq, int32_t M, const float* items_sorted, int64_t N, int32_t K,
                               const int32_t* list_off, const uint32_t* list_ids, const int32_t* grp_list,
                               const int32_t* grp_off, int32_t G, const int32_t* pair_q, const int32_t* pair_col,
                               float* cand_val, uint32_t* cand_idx, int64_t ld, void* stream) {
    RF_REQUIRE(K >= 4 && K <= 1024 && K % 4 == 0, "rf_ivf_scan_f32: needs K %% 4 == 0, 4 <= K <= 1024");
    RF_REQUIRE(M >= 1 && ldq >= K && ldq % 4 == 0, "rf_ivf_scan_f32: needs M >= 1, ldq >= K, ldq %% 4 == 0");
    RF_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && G >= 0 && G <= 65535 && ld >= 0,
               "rf_ivf_scan_f32: needs 0 <= N < 2^31, 0 <= G <= 65535, ld >= 0");
    if (G == 0 || N == 0) return RF_OK;
    RF_REQUIRE(q && items_sorted && list_off && list_ids && grp_list && grp_off && pair_q && pair_col && cand_val && cand_idx,
               "rf_ivf_scan_f32: null pointer");
    RF_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)items_sorted & 15) == 0,
               "rf_ivf_scan_f32: q and items_sorted must be 16-byte aligned");
    // row chunks per list: about one workgroup per 32 rows of an average list (longer lists loop)
    const int64_t avg = (N + G - 1) / G;
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(kScanMaxSplit, (avg + kScanRows - 1) / kScanRows));
    const size_t lds = (size_t)(kScanQ + kScanRows) * (std::min(K, kScanKC) + 4) * sizeof(float);
    hipLaunchKernelGGL(ivf_scan_kernel, dim3(S, G), dim3(kScanThreads), lds, rf_stream(stream), q, ldq, items_sorted, K,
                       list_off, list_ids, grp_list, grp_off, pair_q, pair_col, cand_val, cand_idx, ld);
    return rf_check_launch("rf_ivf_scan_f32");
}
