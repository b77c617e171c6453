// The host half of icpflow_cluster_pcd's HDBSCAN branch alone (icp_flow_amd/csrc/clusterpcd_host.hpp): row mapping, label
// histogram, keep rule.  Built by the host compiler with -fsanitize=address,undefined and run by tests/test_cluster_pcd.py.
// Every buffer is a heap allocation of exactly the size the routine is given, so a step past an end is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../icp_flow_amd/csrc/clusterpcd_host.hpp"

using namespace icpflow;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #cond);                  \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static std::vector<uint8_t> kept(const std::vector<int32_t> &sizes, int64_t noise, int numClusters, int *count)
{
    std::vector<uint8_t> keep(sizes.size(), 0x5A);
    *count = keep_rule(sizes.data(), (int)sizes.size(), noise, numClusters, keep.data());
    return keep;
}

int main()
{
    // ---- row mapping: masked, live and unclustered rows, the subset in caller order
    {
        const std::vector<uint8_t> state = {kRowLive, kRowMasked, kRowLive, kRowUnclustered, kRowMasked, kRowLive, kRowLive};
        std::vector<int32_t> sub(state.size(), 77);
        CHECK(subset_rows(state.data(), (int)state.size(), sub.data()) == 4);
        CHECK((sub == std::vector<int32_t>{0, -1, 1, -1, -1, 2, 3}));
        const std::vector<int32_t> subLabels = {1, -1, 0, 1};
        std::vector<int32_t> labels(state.size(), 77);
        scatter_labels(state.data(), sub.data(), subLabels.data(), (int)state.size(), labels.data());
        CHECK((labels == std::vector<int32_t>{1, -2, -1, -1, -2, 0, 1}));
        // ---- the histogram: np.unique(labels[labels >= -1], return_counts=True)
        std::vector<int32_t> sizes;
        int64_t noise = -1, live = -1;
        CHECK(label_histogram(labels.data(), (int)labels.size(), sizes, &noise, &live) == 2);
        CHECK((sizes == std::vector<int32_t>{1, 2}) && noise == 2 && live == 5);
    }
    {   // nothing live, nothing at all
        const std::vector<uint8_t> state = {kRowMasked, kRowUnclustered};
        std::vector<int32_t> sub(2, 77), labels(2, 77), sizes;
        CHECK(subset_rows(state.data(), 2, sub.data()) == 0);
        scatter_labels(state.data(), sub.data(), nullptr, 2, labels.data());
        CHECK((labels == std::vector<int32_t>{-2, -1}));
        int64_t noise = -1, live = -1;
        CHECK(label_histogram(labels.data(), 2, sizes, &noise, &live) == 0 && sizes.empty() && noise == 1 && live == 1);
        CHECK(label_histogram(nullptr, 0, sizes, &noise, &live) == 0 && noise == 0 && live == 0);
        CHECK(subset_rows(nullptr, 0, nullptr) == 0);
    }
    // ---- the keep rule, each quirk on a vector one can read
    int count = -1;
    // noise present: every cluster is a candidate, the two largest survive
    CHECK((kept({5, 9, 7, 3}, 4, 2, &count) == std::vector<uint8_t>{0, 1, 1, 0}) && count == 2);
    // no noise: cluster 0 is dropped unseen, however large
    CHECK((kept({50, 9, 7, 3}, 0, 2, &count) == std::vector<uint8_t>{0, 1, 1, 0}) && count == 2);
    CHECK((kept({50, 9, 7, 3}, 0, 9, &count) == std::vector<uint8_t>{0, 1, 1, 1}) && count == 3);
    // C <= num_clusters: all candidates
    CHECK((kept({5, 9}, 1, 2, &count) == std::vector<uint8_t>{1, 1}) && count == 2);
    CHECK((kept({5, 9}, 1, 200, &count) == std::vector<uint8_t>{1, 1}) && count == 2);
    // nothing left (where the reference raises): C = 0, and C = 1 without noise
    CHECK(kept({}, 3, 5, &count).empty() && count == 0);
    CHECK(kept({}, 0, 5, &count).empty() && count == 0);
    CHECK((kept({8}, 0, 5, &count) == std::vector<uint8_t>{0}) && count == 0);
    CHECK((kept({8}, 1, 5, &count) == std::vector<uint8_t>{1}) && count == 1);
    // ties at the cut: the larger id wins
    CHECK((kept({4, 4, 4, 9}, 1, 2, &count) == std::vector<uint8_t>{0, 0, 1, 1}) && count == 2);
    CHECK((kept({4, 4, 4, 9}, 0, 3, &count) == std::vector<uint8_t>{0, 1, 1, 1}) && count == 3);
    CHECK((kept({4, 4, 4, 9}, 1, 1, &count) == std::vector<uint8_t>{0, 0, 0, 1}) && count == 1);
    // a long vector against the rank statement the kernel uses: kept iff fewer than numClusters candidates beat it
    {
        std::vector<int32_t> sizes(3000);
        uint32_t x = 12345;
        for (auto &s : sizes) {
            x = x * 1664525u + 1013904223u;
            s = 2 + (int32_t)((x >> 8) % 97);   // many ties
        }
        for (const int64_t noise : {0, 6})
            for (const int numClusters : {1, 255, 256, 257, 2999, 3000, 4000}) {
                const std::vector<uint8_t> keep = kept(sizes, noise, numClusters, &count);
                const int first = noise > 0 ? 0 : 1;
                int total = 0;
                for (int c = 0; c < (int)sizes.size(); ++c) {
                    int rank = 0;
                    for (int j = first; j < (int)sizes.size(); ++j) rank += cluster_beats(sizes[j], j, sizes[c], c) ? 1 : 0;
                    CHECK(keep[c] == (c >= first && rank < numClusters ? 1 : 0));
                    total += keep[c];
                }
                CHECK(total == count);
            }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
