// The workspace carver alone (icp_flow_amd/csrc/carver.hpp), built by the host compiler with -fsanitize=address,undefined
// and run by tests/test_host_layer.py:  carver_check <bytes icpflow_ground_workspace_bytes recorded for n = 513>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../icp_flow_amd/csrc/carver.hpp"

using icpflow::align256;
using icpflow::Carver;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #cond);                  \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// one pass over sizes that cover every rounding case, on a null or a real base: -> the offsets, the total in `total`
static std::vector<size_t> walk(char *base, size_t *total)
{
    const size_t sizes[] = {1, 0, 0, 256, 257, 255, 512, 513, 12345, 0, 1};
    Carver mem(base);
    std::vector<size_t> offs;
    size_t sum = 0;
    for (const size_t bytes : sizes) {
        const size_t before = mem.total();
        unsigned char *p = mem.take<unsigned char>(bytes);
        offs.push_back(before);
        CHECK(before % 256 == 0);
        CHECK(mem.total() - before == (bytes + 255) / 256 * 256);   // take(0) does not advance, take(1) and take(256) by 256, take(257) by 512
        if (base) {
            CHECK(p == (unsigned char *)base + before);
            for (size_t k = 0; k < bytes; ++k) p[k] = 0x5A;          // the whole region is inside the allocation (the sanitizer's check)
        } else {
            CHECK(p == nullptr);
        }
        CHECK(mem.at<unsigned char>(before) == p);
        sum += align256(bytes);
    }
    CHECK(mem.total() == sum);
    *total = mem.total();
    return offs;
}

int main(int argc, char **argv)
{
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(255) == 256 && align256(256) == 256 && align256(257) == 512);
    {
        Carver mem;
        CHECK(mem.take(0) == 0 && mem.total() == 0);
        CHECK(mem.take(1) == 0 && mem.total() == 256);
        CHECK(mem.take(256) == 256 && mem.total() == 512);
        CHECK(mem.take(257) == 512 && mem.total() == 1024);
        CHECK(mem.take(0) == 1024 && mem.total() == 1024);
    }
    size_t totalNull = 0, totalHeap = 0;
    const std::vector<size_t> offsNull = walk(nullptr, &totalNull);
    char *heap = (char *)std::malloc(totalNull);   // exactly the bytes the null pass asked for
    CHECK(heap != nullptr);
    const std::vector<size_t> offsHeap = walk(heap, &totalHeap);
    std::free(heap);
    CHECK(offsNull == offsHeap && totalNull == totalHeap);

    // ground.hip's seven regions for n = 513 (two binning waves), in its field order: the size the library recorded
    const size_t n = 513, waves = 2, patches = 504, cols = 16;
    Carver mem;
    const size_t pid = mem.take(n * sizeof(int32_t)), order = mem.take(n * sizeof(int32_t)), points = mem.take(n * 3 * sizeof(float));
    const size_t state = mem.take(n), waveCount = mem.take(waves * patches * sizeof(int32_t));
    const size_t start = mem.take((patches + 1) * sizeof(int32_t)), table = mem.take(patches * cols * sizeof(double));
    CHECK(pid == 0 && order == 2304 && points == 4608 && state == 11008 && waveCount == 11776 && start == 15872 && table == 17920);
    CHECK(argc == 2 && mem.total() == std::strtoull(argc == 2 ? argv[1] : "0", nullptr, 10));
    std::printf("%s %zu\n", failures ? "FAILED" : "ok", mem.total());
    return failures ? 1 : 0;
}
