// clusterpcd_host.hpp -- the host half of icpflow_cluster_pcd's HDBSCAN branch: what utils_cluster.py:19-29 does with the labels
// of the clustered subset.  Plain C++17, no HIP types: a host compiler builds it alone (tests/cluster_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ICPFLOW_HOST_DEVICE __host__ __device__
#else
#define ICPFLOW_HOST_DEVICE
#endif

namespace icpflow {

// what a row of the stack is to the clustering (one byte per row, written on the device)
constexpr uint8_t kRowMasked = 0;      // mask 0: a ground row, label -2 (-1e8 once finished)
constexpr uint8_t kRowLive = 1;        // a row of the clustered subset
constexpr uint8_t kRowUnclustered = 2; // unmasked, yet not in the subset (a non-finite coordinate): noise

// caller row -> row of the clustered subset (-1: not in it).  -> the subset's size
inline int subset_rows(const uint8_t *state, int n, int32_t *sub)
{
    int nl = 0;
    for (int i = 0; i < n; ++i) sub[i] = state[i] == kRowLive ? nl++ : -1;
    return nl;
}

// labels of the subset -> labels of the stack: -2 masked, -1 noise and unclustered rows, else the cluster id
inline void scatter_labels(const uint8_t *state, const int32_t *sub, const int32_t *subLabels, int n, int32_t *labels)
{
    for (int i = 0; i < n; ++i)
        labels[i] = state[i] == kRowLive ? subLabels[sub[i]] : state[i] == kRowMasked ? -2 : -1;
}

// np.unique(labels[labels >= -1], return_counts=True) as a table: sizes[c] of cluster c, *noise rows with -1, *live rows in all.
// -> the number of clusters (largest id + 1)
inline int label_histogram(const int32_t *labels, int n, std::vector<int32_t> &sizes, int64_t *noise, int64_t *live)
{
    int C = 0;
    for (int i = 0; i < n; ++i) C = std::max(C, labels[i] + 1);
    sizes.assign((size_t)C, 0);
    *noise = *live = 0;
    for (int i = 0; i < n; ++i) {
        const int l = labels[i];
        if (l >= 0) ++sizes[(size_t)l];
        if (l == -1) ++*noise;
        if (l >= -1) ++*live;
    }
    return C;
}

// does cluster a beat cluster b?  (the library's own tie rule: among equal sizes the LARGER id wins; the keep-rule kernel of
// clusterpcd.hip ranks with the same function)
ICPFLOW_HOST_DEVICE inline bool cluster_beats(int32_t sizeA, int a, int32_t sizeB, int b) { return sizeA > sizeB || (sizeA == sizeB && a > b); }

// The keep rule of utils_cluster.py:19-27 / :39-46 on the sizes of clusters 0..C-1: the first unique label is dropped unseen
// (-1 with at least one noise row, else cluster 0), the numClusters largest of the rest survive.  keep[c] = 1 / 0.
// -> how many survive = min(numClusters, candidates)
inline int keep_rule(const int32_t *sizes, int C, int64_t noise, int numClusters, uint8_t *keep)
{
    const int first = noise > 0 ? 0 : 1;
    std::vector<int> ids;
    for (int c = first; c < C; ++c) ids.push_back(c);
    for (int c = 0; c < C; ++c) keep[c] = 0;
    std::sort(ids.begin(), ids.end(), [&](int a, int b) { return cluster_beats(sizes[a], a, sizes[b], b); });
    const int kept = std::min<int64_t>((int64_t)std::max(numClusters, 0), (int64_t)ids.size());
    for (int k = 0; k < kept; ++k) keep[ids[(size_t)k]] = 1;
    return kept;
}

}  // namespace icpflow
