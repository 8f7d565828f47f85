// arg_array.h -- the device arrays a batched step's argument blocks live in (every icem_plan_step_*_batch): SLOTS of them, each
// with a host shadow of what it holds and written only when a byte changed -- a steady-state step uploads nothing.  Which slot a
// step uses and how much room a slot gets when it has to grow are the caller's; what a blob holds where is block_layout.h's, and
// the blocks of recorded launches get there through recorded_batch.h.  Internal; not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

namespace icem {

template <int SLOTS>
class DeviceArgArray {
    struct Slot {
        void* dev = nullptr;
        size_t cap = 0;
        std::vector<unsigned char> shadow;   // what dev holds
    } slots_[SLOTS];

  public:
    DeviceArgArray() = default;
    DeviceArgArray(const DeviceArgArray&) = delete;
    DeviceArgArray& operator=(const DeviceArgArray&) = delete;
    ~DeviceArgArray() {
        for (Slot& s : slots_)
            if (s.dev) (void)hipFree(s.dev);
    }
    const void* dev(int slot) const { return slots_[slot].dev; }
    const std::vector<unsigned char>& holds(int slot) const { return slots_[slot].shadow; }
    // Make `slot` hold `blob`.  A slot smaller than the blob is replaced by one of `room` (>= blob.size()) bytes, behind a
    // synchronisation of `st`: launches of an earlier step may still read the old array.  ++*uploads when the size or a byte
    // differed from what the slot held and the blob went to the device (ordered on `st`; the source is pageable, so the
    // runtime has staged it when the call returns).
    hipError_t put(int slot, const std::vector<unsigned char>& blob, size_t room, hipStream_t st, unsigned long long* uploads) {
        Slot& s = slots_[slot];
        const size_t bytes = blob.size();
        if (s.cap < bytes) {
            if (s.dev) {
                if (hipError_t e = hipStreamSynchronize(st)) return e;
                (void)hipFree(s.dev);
            }
            s.dev = nullptr;
            s.cap = 0;
            s.shadow.clear();
            if (hipError_t e = hipMalloc(&s.dev, room)) return e;
            s.cap = room;
        }
        if (s.shadow.size() == bytes && std::memcmp(s.shadow.data(), blob.data(), bytes) == 0) return hipSuccess;
        if (hipError_t e = hipMemcpyAsync(s.dev, blob.data(), bytes, hipMemcpyHostToDevice, st)) return e;
        s.shadow = blob;
        ++*uploads;
        return hipSuccess;
    }
};

}  // namespace icem
