// The upload decision of DeviceArgArray (icem_amd/csrc/arg_array.h) on the host alone: the four HIP calls the type makes are
// replaced by counting stubs (the "device" arrays are host memory), so the program needs no GPU.  Prints "0 failures" and
// exits 0 when every expectation holds.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct Calls {
    int mallocs = 0, frees = 0, copies = 0, syncs = 0;
    int syncs_at_last_free = -1;   // how many synchronisations had happened when a live array was freed
    size_t last_room = 0, last_bytes = 0;
    void* last_dst = nullptr;
} calls;
hipError_t stub_malloc(void** p, size_t n) {
    *p = std::malloc(n);
    ++calls.mallocs;
    calls.last_room = n;
    return hipSuccess;
}
hipError_t stub_free(void* p) {
    std::free(p);
    ++calls.frees;
    calls.syncs_at_last_free = calls.syncs;
    return hipSuccess;
}
hipError_t stub_copy(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
    std::memcpy(dst, src, n);
    ++calls.copies;
    calls.last_bytes = n;
    calls.last_dst = dst;
    return hipSuccess;
}
hipError_t stub_sync(hipStream_t) {
    ++calls.syncs;
    return hipSuccess;
}
}  // namespace
#define hipMalloc stub_malloc
#define hipFree stub_free
#define hipMemcpyAsync stub_copy
#define hipStreamSynchronize stub_sync
#include "arg_array.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: expected %s\n", __LINE__, #cond);   \
            ++failures;                                               \
        }                                                             \
    } while (0)

int main() {
    using Blob = std::vector<unsigned char>;
    {
        icem::DeviceArgArray<3> a;
        unsigned long long ups = 0, want = 0;   // the owner's upload counter, and what it should read
        Blob b(1000);
        for (size_t i = 0; i < b.size(); ++i) b[i] = (unsigned char)(i * 7);
        // first use of a slot: allocated with the caller's room (no array to free, so no synchronisation), uploaded
        EXPECT(a.put(0, b, b.size() + 4096, nullptr, &ups) == hipSuccess && ups == ++want);
        EXPECT(calls.mallocs == 1 && calls.last_room == 5096 && calls.syncs == 0 && calls.frees == 0 && calls.copies == 1 && calls.last_bytes == 1000);
        EXPECT(calls.last_dst == a.dev(0) && std::memcmp(a.dev(0), b.data(), 1000) == 0 && a.holds(0) == b);
        // the same bytes: nothing
        EXPECT(a.put(0, b, b.size() + 4096, nullptr, &ups) == hipSuccess && ups == want && calls.copies == 1 && calls.mallocs == 1);
        // one changed byte (the last one): an upload, no allocation
        b[999] ^= 1;
        EXPECT(a.put(0, b, b.size() + 4096, nullptr, &ups) == hipSuccess && ups == ++want && calls.copies == 2 && calls.mallocs == 1);
        EXPECT(std::memcmp(a.dev(0), b.data(), 1000) == 0);
        EXPECT(a.put(0, b, b.size() + 4096, nullptr, &ups) == hipSuccess && ups == want && calls.copies == 2);
        // a changed size with the same leading bytes, inside the capacity: an upload, no allocation -- shorter, then longer again
        Blob s(b.begin(), b.begin() + 600);
        EXPECT(a.put(0, s, s.size() + 4096, nullptr, &ups) == hipSuccess && ups == ++want && calls.copies == 3 && calls.last_bytes == 600 && calls.mallocs == 1);
        EXPECT(a.put(0, b, b.size() + 4096, nullptr, &ups) == hipSuccess && ups == ++want && calls.copies == 4 && calls.mallocs == 1 && calls.syncs == 0);
        // slots are independent: the same blob in another slot is new there, and leaves slot 0 as it was
        EXPECT(a.dev(1) == nullptr && a.holds(1).empty());
        EXPECT(a.put(1, b, 2000, nullptr, &ups) == hipSuccess && ups == ++want && calls.mallocs == 2 && calls.last_room == 2000 && calls.copies == 5);
        EXPECT(a.dev(1) != a.dev(0) && calls.last_dst == a.dev(1));
        EXPECT(a.put(0, b, b.size() + 4096, nullptr, &ups) == hipSuccess && ups == want && calls.copies == 5);
        // growth past the capacity: the stream is synchronised BEFORE the old array is freed, the new one has the caller's room
        Blob g(6000, 3);
        EXPECT(a.put(0, g, 8192, nullptr, &ups) == hipSuccess && ups == ++want);
        EXPECT(calls.syncs == 1 && calls.frees == 1 && calls.syncs_at_last_free == 1 && calls.mallocs == 3 && calls.last_room == 8192);
        EXPECT(calls.copies == 6 && calls.last_bytes == 6000 && std::memcmp(a.dev(0), g.data(), 6000) == 0);
        EXPECT(a.put(0, g, 8192, nullptr, &ups) == hipSuccess && ups == want && calls.copies == 6 && calls.mallocs == 3);
        // ... and slot 1 still holds its blob, slot 2 was never touched
        EXPECT(a.put(1, b, 2000, nullptr, &ups) == hipSuccess && ups == want && calls.copies == 6);
        EXPECT(a.dev(2) == nullptr);
    }
    // the destructor frees the two arrays that were live
    EXPECT(calls.frees == 3);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
