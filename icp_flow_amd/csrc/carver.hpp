// carver.hpp -- the one bump allocator over a caller's workspace.  Plain C++17, no HIP types: a host compiler builds it alone
// (tests/carver_check.cpp).  Every *_bytes() query and the call it sizes run the same carve, the query on a null base.
#pragma once
#include <cstddef>

namespace icpflow {

// every region of every workspace starts a multiple of 256 bytes behind the base
inline size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

class Carver {
public:
    explicit Carver(void *base = nullptr) : base_(static_cast<char *>(base)) {}
    // the next region: -> its offset, the position moves on by align256(bytes)
    size_t take(size_t bytes)
    {
        const size_t off = total_;
        total_ += align256(bytes);
        return off;
    }
    // an offset as a pointer; null on a null base (a size query)
    template <class T> T *at(size_t off) const { return base_ ? reinterpret_cast<T *>(base_ + off) : nullptr; }
    template <class T> T *take(size_t bytes) { return at<T>(take(bytes)); }
    // the bytes handed out so far
    size_t total() const { return total_; }

private:
    char *base_;
    size_t total_ = 0;
};

}  // namespace icpflow
