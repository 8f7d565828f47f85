// block_layout.h -- the section arithmetic of a batched step's argument blob, written once.  A blob is a run of sections, one
// per launch: the launch's argument block of each of the n problems back to back, the section rounded up to ALIGN bytes so that
// every section starts on an ALIGN boundary of the device array (DeviceArgArray, arg_array.h).  A layout advances two totals:
// bytes(), the blob of THIS call's n problems, and room(), the same sections at the batch maximum -- what a slot is given when it
// is allocated, so that a batch that grows later allocates nothing.
// Includes nothing of HIP or of the library: a plain C++17 program can hold it to its rule (tests/test_block_layout_cpu.py).
#pragma once
#include <cstddef>

namespace icem {

class BlockLayout {
    size_t n_, max_, bytes_ = 0, room_ = 0;
    static size_t rounded(size_t b) { return (b + ALIGN - 1) / ALIGN * ALIGN; }

  public:
    static constexpr size_t ALIGN = 256;
    BlockLayout(int n, int n_max) : n_((size_t)n), max_((size_t)n_max) {}
    // a section of n blocks of block_bytes each -> its offset in the blob
    size_t add(size_t block_bytes) {
        const size_t at = bytes_;
        bytes_ += rounded(block_bytes * n_);
        room_ += rounded(block_bytes * max_);
        return at;
    }
    size_t bytes() const { return bytes_; }
    size_t room() const { return room_; }
};

}  // namespace icem
