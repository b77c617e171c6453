// clusterpcd.hip -- cluster_pcd as a whole behind the C ABI (utils_cluster.py:10-63): icpflow_cluster_pcd and
// icpflow_track_frame_points.  The clustering itself is cluster.hip's (DBSCAN) and hdbscan.hip's + hdbscan_tree.cpp's (HDBSCAN),
// unchanged; what is here is the rest of cluster_pcd -- the stack of both clouds, the counts of live and noise rows, the keep
// rule (utils_cluster.py:19-27, 39-46) and the float labels (:54-62) -- as small, latency-bound kernels, so that the DBSCAN
// branch needs no host between the points and the labels track() reads.
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "kernels.hpp"
#include "host.hpp"
#include "clusterpcd_host.hpp"

namespace icpflow {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// words of `misc` (int32): [0, 4) the four words of d_info as the host uploads them (HDBSCAN), then
constexpr int kMiscClusters = 4, kMiscLive = 5, kMiscNoise = 6, kMiscWords = 8;

// both segments as one cloud of packed (x, y, z) rows, dst first, with a mask byte per row (1 where the caller gave no mask);
// the counters of count_kernel start at zero
__global__ __launch_bounds__(kBlock) void stack_kernel(const float *__restrict__ dst, int nDst, const float *__restrict__ src,
                                                       int n, int stride, const uint8_t *__restrict__ maskDst,
                                                       const uint8_t *__restrict__ maskSrc, float *__restrict__ pts,
                                                       uint8_t *__restrict__ mask, int32_t *__restrict__ misc)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) misc[kMiscLive] = misc[kMiscNoise] = 0;
    if (i >= n) return;
    const bool inDst = i < nDst;
    const int r = inDst ? i : i - nDst;
    const float *p = (inDst ? dst : src) + (size_t)r * stride;
    const uint8_t *m = inDst ? maskDst : maskSrc;
    pts[(size_t)i * 3] = p[0];
    pts[(size_t)i * 3 + 1] = p[1];
    pts[(size_t)i * 3 + 2] = p[2];
    mask[i] = m ? (m[r] ? 1 : 0) : 1;
}

// (labels > -2).sum() and (labels == -1).sum() of icpflow_dbscan's labels: ballots, the waves of a workgroup added in LDS in
// a fixed order, one integer atomic per workgroup and counter
__global__ __launch_bounds__(kBlock) void count_kernel(const int32_t *__restrict__ labels, int n, int32_t *__restrict__ misc)
{
    __shared__ int part[2][kWaves];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l = i < n ? labels[i] : -2;
    const int live = __popcll(__ballot(l > -2)), noise = __popcll(__ballot(l == -1));
    if (lane == 0) {
        part[0][w] = live;
        part[1][w] = noise;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int sum = 0;
        for (int v = 0; v < kWaves; ++v) sum += part[threadIdx.x][v];
        if (sum) atomicAdd(misc + (threadIdx.x == 0 ? kMiscLive : kMiscNoise), sum);
    }
}

// The keep rule on sizes[0..C), C read from device memory (utils_cluster.py:39-46): rank of cluster c = the number of candidates
// that beat it (cluster_beats), kept iff it is a candidate and rank < numKeep.  Candidates: every cluster when there is a noise
// row (the first unique label, dropped unseen, is -1), else every cluster but 0.  The sizes pass through LDS a tile at a time.
// The grid is sized for the most clusters n rows can form and strides, so any C is served; workgroups without a cluster leave.
__global__ __launch_bounds__(kBlock) void keep_rank_kernel(const int32_t *__restrict__ sizes, const int32_t *__restrict__ misc,
                                                           int numKeep, uint8_t *__restrict__ keep, int32_t *__restrict__ info)
{
    __shared__ int tile[kBlock];
    const int C = misc[kMiscClusters], live = misc[kMiscLive], noise = misc[kMiscNoise];
    const int first = noise > 0 ? 0 : 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = C;
        info[1] = min(numKeep, max(C - first, 0));
        info[2] = noise;
        info[3] = live;
    }
    for (int base = blockIdx.x * kBlock; base < C; base += gridDim.x * kBlock) {   // (uniform per workgroup)
        const int c = base + threadIdx.x;
        const int mine = c < C ? sizes[c] : 0;
        int rank = 0;
        for (int t0 = first; t0 < C; t0 += kBlock) {
            const int j = t0 + threadIdx.x;
            __syncthreads();
            tile[threadIdx.x] = j < C ? sizes[j] : -1;
            __syncthreads();
            const int m = min(kBlock, C - t0);
            for (int k = 0; k < m; ++k) rank += cluster_beats(tile[k], t0 + k, mine, c) ? 1 : 0;
        }
        if (c < C) keep[c] = (c >= first && rank < numKeep) ? 1 : 0;
    }
}

// int32 label + keep table -> cluster_pcd's float label (utils_cluster.py:54-62), written per segment: row i of the stack is
// row i of dst or row i - nDst of src.  infoSrc (HDBSCAN: the four words the host uploaded) -> info
__global__ __launch_bounds__(kBlock) void finish_kernel(const int32_t *__restrict__ labels, const uint8_t *__restrict__ keep,
                                                        int n, int nDst, float *__restrict__ outDst,
                                                        float *__restrict__ outSrc, const int32_t *__restrict__ infoSrc,
                                                        int32_t *__restrict__ info)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (infoSrc != nullptr && i < 4) info[i] = infoSrc[i];
    if (i >= n) return;
    const int l = labels[i];
    const float f = l <= -2 ? -1e8f : (l >= 0 && keep[l]) ? (float)l : -1.0f;
    if (i < nDst) outDst[i] = f;
    else outSrc[i - nDst] = f;
}

// HDBSCAN: what the host needs of the spanning tree, ready to sort and download: a state byte per row (clusterpcd_host.hpp;
// icpflow_hdbscan_mst marks the rows that took no part with a NaN core distance), the edges as (squared weight, a << 32 | b)
// with +inf behind the last edge -- the sort runs over n entries, the number of edges stays on the device
__global__ __launch_bounds__(kBlock) void hdb_pack_kernel(const double *__restrict__ core2, const uint8_t *__restrict__ mask,
                                                          const int32_t *__restrict__ ea, const int32_t *__restrict__ eb,
                                                          const double *__restrict__ w2, const int32_t *__restrict__ cnt,
                                                          int n, double *__restrict__ key,
                                                          unsigned long long *__restrict__ val, uint8_t *__restrict__ state)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    state[i] = !mask[i] ? kRowMasked : core2[i] == core2[i] ? kRowLive : kRowUnclustered;
    const bool edge = i < cnt[0];
    key[i] = edge ? w2[i] : HUGE_VAL;
    val[i] = edge ? ((unsigned long long)(uint32_t)ea[i] << 32) | (uint32_t)eb[i] : 0ull;
}

struct Carve {
    float *pts;
    uint8_t *mask, *keep, *state;
    int32_t *labels, *misc, *counts, *ea, *eb, *cnt;
    double *core2, *w2, *keyIn, *keyOut;
    unsigned long long *valIn, *valOut;
    void *sortTmp, *inner;
    size_t sortTmpBytes, innerBytes, total;
    size_t oUp, upBytes, oDown, downBytes;   // the spans of the one upload and the one download
    size_t oKeepInUp, oMiscInUp, oStateInDown, oKeyInDown, oValInDown;
};

hipError_t carve(int n, int method, void *ws, Carve *c, hipStream_t s)
{
    const size_t N = (size_t)n;
    Carver mem(ws);
    c->pts = mem.take<float>(N * 12);
    c->mask = mem.take<uint8_t>(N);
    c->oUp = mem.total();
    c->labels = mem.take<int32_t>(N * 4);
    c->oKeepInUp = mem.total() - c->oUp;
    c->keep = mem.take<uint8_t>(N);
    c->oMiscInUp = mem.total() - c->oUp;
    c->misc = mem.take<int32_t>(kMiscWords * 4);
    c->upBytes = c->oMiscInUp + 16;
    hipError_t e = hipSuccess;
    if (method == ICPFLOW_CLUSTER_DBSCAN) {
        c->counts = mem.take<int32_t>(N * 4);
        e = dbscan_workspace_bytes(n, &c->innerBytes);
    } else {
        c->core2 = mem.take<double>(N * 8);
        c->ea = mem.take<int32_t>(N * 4);
        c->eb = mem.take<int32_t>(N * 4);
        c->w2 = mem.take<double>(N * 8);
        c->keyIn = mem.take<double>(N * 8);
        c->valIn = mem.take<unsigned long long>(N * 8);
        c->oDown = mem.total();
        c->cnt = mem.take<int32_t>(8);
        c->oStateInDown = mem.total() - c->oDown;
        c->state = mem.take<uint8_t>(N);
        c->oKeyInDown = mem.total() - c->oDown;
        c->keyOut = mem.take<double>(N * 8);
        c->oValInDown = mem.total() - c->oDown;
        c->valOut = mem.take<unsigned long long>(N * 8);
        c->downBytes = c->oValInDown + N * 8;
        c->sortTmpBytes = 0;
        e = rocprim::radix_sort_pairs(nullptr, c->sortTmpBytes, (double *)nullptr, (double *)nullptr,
                                      (unsigned long long *)nullptr, (unsigned long long *)nullptr, N, 0, 64, s);
        if (e != hipSuccess) return e;
        c->sortTmp = mem.take<void>(c->sortTmpBytes);
        e = hdbscan_workspace_bytes(n, &c->innerBytes);
    }
    if (e != hipSuccess) return e;
    c->inner = mem.take<void>(c->innerBytes);
    c->total = mem.total();
    return hipSuccess;
}

// the checks both the size query and the call make: -> 0 or the status of the refusal
int check_params(const char *fn, int nDst, int nSrc, const icpflow_cluster_params_t *p)
{
    if (!p) return pointer_error(fn);
    if (p->struct_size < sizeof(icpflow_cluster_params_t))
        return report_errorf(ICPFLOW_E_ARG, "%s: params.struct_size %zu, this library's icpflow_cluster_params_t has %zu bytes", fn,
                             p->struct_size, sizeof(icpflow_cluster_params_t));
    if (nDst < 0 || nSrc < 0 || (nDst == 0 && nSrc == 0))
        return report_errorf(ICPFLOW_E_ARG, "%s: n_dst and n_src must not be negative, nor both zero (got %d, %d)", fn, nDst, nSrc);
    if (p->method != ICPFLOW_CLUSTER_DBSCAN && p->method != ICPFLOW_CLUSTER_HDBSCAN)
        return report_errorf(ICPFLOW_E_ARG, "%s: unknown method %d", fn, p->method);
    const bool hdb = p->method == ICPFLOW_CLUSTER_HDBSCAN;
    if (!hdb && !(p->eps > 0.0)) return report_errorf(ICPFLOW_E_ARG, "%s: eps must be positive (got %g)", fn, p->eps);
    if (p->min_cluster_size < (hdb ? 2 : 1))
        return report_errorf(ICPFLOW_E_ARG, "%s: min_cluster_size must be >= %d (got %d)", fn, hdb ? 2 : 1, p->min_cluster_size);
    if (p->num_clusters < 1) return report_errorf(ICPFLOW_E_ARG, "%s: num_clusters must be >= 1 (got %d)", fn, p->num_clusters);
    if (!(p->cell >= 0.0)) return report_errorf(ICPFLOW_E_ARG, "%s: cell must not be negative (got %g)", fn, p->cell);
    if (hdb && p->min_cluster_size > 63)
        return report_errorf(ICPFLOW_E_LIMIT, "%s: HDBSCAN takes min_cluster_size up to 63 (min_samples = min_cluster_size + 1 <= 64), got %d",
                             fn, p->min_cluster_size);
    const int64_t n = (int64_t)nDst + nSrc;
    // cluster ids are written as float32: every id must be exact
    if (n > 0x7fffffffLL || (n + p->min_cluster_size - 1) / p->min_cluster_size > (1LL << 24))
        return report_errorf(ICPFLOW_E_LIMIT, "%s: %lld rows with min_cluster_size %d can form more than 2^24 clusters: ids would not be exact in float32",
                             fn, (long long)n, p->min_cluster_size);
    return 0;
}

struct HostWork {   // per host thread
    Pinned pin;
    std::vector<int32_t> sub, a, b, subLabels, sizes;
    std::vector<double> w;
};

}  // namespace

}  // namespace icpflow

using namespace icpflow;

extern "C" int icpflow_cluster_default_params(icpflow_cluster_params_t *p)
{
    if (!p) return pointer_error("icpflow_cluster_default_params");
    memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->method = ICPFLOW_CLUSTER_DBSCAN;   // main.py:83-84: --if_hdbscan is a switch, off unless given
    p->min_cluster_size = 30;             // main.py:79
    p->num_clusters = 100;                // main.py:77
    p->eps = 0.25;                        // main.py:81
    p->cell = 0.0;
    return 0;
}

extern "C" size_t icpflow_cluster_pcd_workspace_bytes(int n_dst, int n_src, const icpflow_cluster_params_t *params)
{
    if (check_params("icpflow_cluster_pcd_workspace_bytes", n_dst, n_src, params)) return 0;
    Carve c;
    if (carve(n_dst + n_src, params->method, nullptr, &c, nullptr) != hipSuccess) return 0;
    return c.total;
}

extern "C" int icpflow_cluster_pcd(const float *d_dst, int n_dst, const float *d_src, int n_src, int stride,
                                   const uint8_t *d_mask_dst, const uint8_t *d_mask_src, const icpflow_cluster_params_t *params,
                                   float *d_labels_dst, float *d_labels_src, int32_t *d_info, void *d_ws, size_t ws_bytes,
                                   icpflow_stream_t stream)
{
    const char *fn = "icpflow_cluster_pcd";
    if (int r = check_params(fn, n_dst, n_src, params)) return r;
    if ((n_dst > 0 && (!d_dst || !d_labels_dst)) || (n_src > 0 && (!d_src || !d_labels_src)) || !d_info) return pointer_error(fn);
    if (stride < 3) return report_errorf(ICPFLOW_E_ARG, "%s: stride must be >= 3 floats (got %d)", fn, stride);
    hipStream_t s = (hipStream_t)stream;
    const int n = n_dst + n_src, minSize = params->min_cluster_size;
    Carve c;
    ICPFLOW_TRY(carve(n, params->method, d_ws, &c, s));
    if (!d_ws || ws_bytes < c.total) return workspace_error(fn, "icpflow_cluster_pcd_workspace_bytes", d_ws, ws_bytes, c.total);
    const int blocks = (n + kBlock - 1) / kBlock;
    bool small = false;
    stack_kernel<<<blocks, kBlock, 0, s>>>(d_dst, n_dst, d_src, n, stride, d_mask_dst, d_mask_src, c.pts, c.mask, c.misc);

    if (params->method == ICPFLOW_CLUSTER_DBSCAN) {
        ICPFLOW_TRY(launch_dbscan(c.pts, 3, c.mask, n, params->eps, minSize, c.labels, c.counts, c.misc + kMiscClusters, c.inner,
                                  c.innerBytes, &small, s));
        if (small) return report_errorf(ICPFLOW_E_WORKSPACE, "%s: the carve of the DBSCAN workspace fell short (internal error)", fn);
        count_kernel<<<blocks, kBlock, 0, s>>>(c.labels, n, c.misc);
        const int worst = (int)(((int64_t)n + minSize - 1) / minSize);   // the most clusters n rows can form
        keep_rank_kernel<<<(worst + kBlock - 1) / kBlock, kBlock, 0, s>>>(c.counts, c.misc, params->num_clusters, c.keep, d_info);
        finish_kernel<<<blocks, kBlock, 0, s>>>(c.labels, c.keep, n, n_dst, d_labels_dst, d_labels_src, nullptr, d_info);
        ICPFLOW_TRY(hipGetLastError());
        return 0;
    }

    // ---- HDBSCAN: BLOCKING.  Tree and sorted edges on the device, one download, the sequential remainder here, one upload
    static thread_local HostWork H;
    const int minSamples = minSize + 1;
    ICPFLOW_TRY(launch_hdbscan_mst(c.pts, 3, c.mask, n, minSamples, params->cell > 0.0 ? params->cell : 0.25, c.core2, c.ea, c.eb,
                                   c.w2, c.cnt, c.cnt + 1, c.inner, c.innerBytes, &small, s));
    if (small) return report_errorf(ICPFLOW_E_WORKSPACE, "%s: the carve of the HDBSCAN workspace fell short (internal error)", fn);
    hdb_pack_kernel<<<blocks, kBlock, 0, s>>>(c.core2, c.mask, c.ea, c.eb, c.w2, c.cnt, n, c.keyIn, c.valIn, c.state);
    ICPFLOW_TRY(rocprim::radix_sort_pairs(c.sortTmp, c.sortTmpBytes, c.keyIn, c.keyOut, c.valIn, c.valOut, (size_t)n, 0, 64, s));
    char *pin = H.pin.need(c.downBytes + c.upBytes);
    if (pin == nullptr) return report_errorf(ICPFLOW_E_HOSTMEM, "%s: no pinned host memory", fn);
    char *down = pin, *up = pin + c.downBytes;
    ICPFLOW_TRY(hipMemcpyAsync(down, static_cast<char *>(d_ws) + c.oDown, c.downBytes, hipMemcpyDeviceToHost, s));
    ICPFLOW_TRY(hipStreamSynchronize(s));
    const int32_t *cnt = reinterpret_cast<const int32_t *>(down);
    const uint8_t *state = reinterpret_cast<const uint8_t *>(down + c.oStateInDown);
    const double *w2 = reinterpret_cast<const double *>(down + c.oKeyInDown);
    const unsigned long long *ab = reinterpret_cast<const unsigned long long *>(down + c.oValInDown);
    const int ne = cnt[0], nl = cnt[1];
    if (nl < minSamples)
        return report_errorf(ICPFLOW_E_ARG, "%s: %d points cannot be clustered with min_samples %d (min_cluster_size + 1)", fn, nl, minSamples);
    H.sub.resize((size_t)n);
    if (ne != nl - 1 || subset_rows(state, n, H.sub.data()) != nl)
        return report_errorf(ICPFLOW_E_ARG, "%s: %d tree edges for %d points (internal error)", fn, ne, nl);
    H.a.resize((size_t)ne);
    H.b.resize((size_t)ne);
    H.w.resize((size_t)ne);
    for (int e = 0; e < ne; ++e) {
        const uint32_t a = (uint32_t)(ab[e] >> 32), b = (uint32_t)ab[e];
        if (a >= (uint32_t)n || b >= (uint32_t)n || H.sub[a] < 0 || H.sub[b] < 0)
            return report_errorf(ICPFLOW_E_ARG, "%s: a tree edge names a row outside the clustered subset (internal error)", fn);
        H.a[(size_t)e] = H.sub[a];
        H.b[(size_t)e] = H.sub[b];
        H.w[(size_t)e] = std::sqrt(w2[e]);
    }
    H.subLabels.resize((size_t)nl);
    if (icpflow_hdbscan_labels(H.a.data(), H.b.data(), H.w.data(), nl, minSize, H.subLabels.data()) != 0)
        return report_errorf(ICPFLOW_E_ARG, "%s: the edges do not span the clustered subset (internal error)", fn);
    int32_t *labels = reinterpret_cast<int32_t *>(up);
    uint8_t *keep = reinterpret_cast<uint8_t *>(up + c.oKeepInUp);
    int32_t *info = reinterpret_cast<int32_t *>(up + c.oMiscInUp);
    scatter_labels(state, H.sub.data(), H.subLabels.data(), n, labels);
    int64_t noise = 0, live = 0;
    const int C = label_histogram(labels, n, H.sizes, &noise, &live);
    info[0] = C;
    info[1] = keep_rule(H.sizes.data(), C, noise, params->num_clusters, keep);
    info[2] = (int32_t)noise;
    info[3] = (int32_t)live;
    ICPFLOW_TRY(hipMemcpyAsync(static_cast<char *>(d_ws) + c.oUp, up, c.upBytes, hipMemcpyHostToDevice, s));
    finish_kernel<<<blocks, kBlock, 0, s>>>(c.labels, c.keep, n, n_dst, d_labels_dst, d_labels_src, c.misc, d_info);
    ICPFLOW_TRY(hipGetLastError());
    ICPFLOW_TRY(hipStreamSynchronize(s));   // (the staging buffer is this thread's next call's as well)
    return 0;
}

extern "C" int icpflow_track_frame_points(const float *d_points_src, const uint8_t *d_mask_src, int n_src, const float *d_points_dst,
                                          const uint8_t *d_mask_dst, int n_dst, const icpflow_cluster_params_t *cluster,
                                          float *d_labels_src, float *d_labels_dst, const icpflow_registration_t *reg,
                                          const icpflow_frame_params_t *par, float *d_rows, float *d_T, int32_t *h_pairs,
                                          const float *d_flow_points, const float *d_pose, float *d_flow, void *d_scratch,
                                          size_t scratch_bytes, size_t *scratch_needed, icpflow_stream_t stream,
                                          const icpflow_options_t *opt)
{
    const char *fn = "icpflow_track_frame_points";
    if (!d_points_src || !d_points_dst || !d_labels_src || !d_labels_dst || !reg || !par || !d_rows || !d_T || !h_pairs || !scratch_needed)
        return pointer_error(fn);
    if (n_src <= 0 || n_dst <= 0) return report_errorf(ICPFLOW_E_ARG, "%s: n_src and n_dst must be positive (got %d, %d)", fn, n_src, n_dst);
    if (int r = check_params(fn, n_dst, n_src, cluster)) return r;
    *h_pairs = ICPFLOW_FRAME_HOST_PATH;
    // the scratch: the four words of d_info, the clustering's workspace, then the frame's own (whose size the frame code reports
    // as it learns it).  The frame's first refusal -- asked for with no scratch at all -- comes before the clustering runs: a
    // refused call has written nothing
    const size_t cws = icpflow_cluster_pcd_workspace_bytes(n_dst, n_src, cluster);
    if (cws == 0) return report_errorf(ICPFLOW_E_ARG, "%s: the size of the clustering's workspace cannot be had (no device?)", fn);
    const size_t head = align256(4 * sizeof(int32_t)) + cws;
    size_t inner = 0;
    int r = icpflow_track_frame(d_points_src, d_labels_src, n_src, d_points_dst, d_labels_dst, n_dst, reg, par, d_rows, d_T, h_pairs,
                                d_flow_points, d_pose, d_flow, nullptr, 0, &inner, stream, opt);
    if (r != ICPFLOW_E_WORKSPACE) return r;
    *scratch_needed = head + inner;
    if (d_scratch == nullptr || scratch_bytes < head + inner)
        return report_errorf(ICPFLOW_E_WORKSPACE, "%s: scratch too small (see *scratch_needed)", fn);
    char *base = static_cast<char *>(d_scratch);
    r = icpflow_cluster_pcd(d_points_dst, n_dst, d_points_src, n_src, 3, d_mask_dst, d_mask_src, cluster, d_labels_dst, d_labels_src,
                            reinterpret_cast<int32_t *>(base), base + (head - cws), cws, stream);
    if (r != 0) return r;
    r = icpflow_track_frame(d_points_src, d_labels_src, n_src, d_points_dst, d_labels_dst, n_dst, reg, par, d_rows, d_T, h_pairs,
                            d_flow_points, d_pose, d_flow, base + head, scratch_bytes - head, &inner, stream, opt);
    *scratch_needed = head + inner;
    if (r == ICPFLOW_E_WORKSPACE) return report_errorf(ICPFLOW_E_WORKSPACE, "%s: scratch too small (see *scratch_needed)", fn);
    return r;
}
