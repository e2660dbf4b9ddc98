// Host only: the one owner of whatever the HIP runtime hands out and wants back -- device, fine-grained and pinned memory,
// IPC mappings, events, streams, graphs and graph executables.  Every release call of the library is in this file.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace mppi {

// A raw handle P (a pointer in every case) and the policy D that releases it -- D::free(P) -- and, for memory, obtains it --
// D::alloc(void **, bytes).  Move-only; reads as the raw handle wherever one is expected, so parameter structs, launchers and
// HIP calls take it as before.  Nothing is released behind the caller's back but at scope exit: reset() and move assignment
// release what is held when they are reached, so they stand where the hand-written release stood (behind the synchronisation
// that makes the object idle).
template <typename P, typename D> class Owner {
    P v_ = P{};

public:
    Owner() = default;
    Owner(Owner &&o) noexcept : v_(o.release()) {}
    Owner &operator=(Owner &&o) noexcept {  // what is held goes first, then o's moves in
        if (this != &o) (void)reset(), v_ = o.release();
        return *this;
    }
    ~Owner() { (void)reset(); }

    P get() const { return v_; }
    operator P() const { return v_; }
    P operator->() const { return v_; }
    P *put() { return &v_; }  // for the runtime's create / open calls to fill: on an empty owner only
    P release() { return std::exchange(v_, P{}); }
    hipError_t reset() { return v_ ? D::free(release()) : hipSuccess; }  // empty afterwards, whatever the runtime answers
    hipError_t alloc(size_t bytes) {  // empty after a failure
        (void)reset();
        void *p = nullptr;
        const hipError_t e = D::alloc(&p, bytes);
        if (e == hipSuccess) v_ = static_cast<P>(p);
        return e;
    }
};

struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void *p) { return hipFree(p); }
};
struct FineGrainedMem : DeviceMem {  // a peer GPU's stores become visible to this GPU's loads without a cache writeback here
    static hipError_t alloc(void **p, size_t bytes) { return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained); }
};
struct PinnedMappedMem {  // host memory the device writes through its own alias of it (hipHostGetDevicePointer)
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
    static hipError_t free(void *p) { return hipHostFree(p); }
};
struct IpcMapping { static hipError_t free(void *p) { return hipIpcCloseMemHandle(p); } };
struct EventPolicy { static hipError_t free(hipEvent_t e) { return hipEventDestroy(e); } };
struct StreamPolicy { static hipError_t free(hipStream_t s) { return hipStreamDestroy(s); } };
struct GraphPolicy { static hipError_t free(hipGraph_t g) { return hipGraphDestroy(g); } };
struct GraphExecPolicy { static hipError_t free(hipGraphExec_t g) { return hipGraphExecDestroy(g); } };

template <typename T> using DevBuf = Owner<T *, DeviceMem>;  // T = void: elements in the handle's precision
template <typename T> using FineBuf = Owner<T *, FineGrainedMem>;
template <typename T> using PinnedBuf = Owner<T *, PinnedMappedMem>;
using IpcMap = Owner<void *, IpcMapping>;
using Event = Owner<hipEvent_t, EventPolicy>;
using Stream = Owner<hipStream_t, StreamPolicy>;
using Graph = Owner<hipGraph_t, GraphPolicy>;
using GraphExec = Owner<hipGraphExec_t, GraphExecPolicy>;

static_assert(!std::is_copy_constructible_v<DevBuf<void>> && !std::is_copy_constructible_v<FineBuf<char>> &&
              !std::is_copy_constructible_v<PinnedBuf<int>> && !std::is_copy_constructible_v<IpcMap> &&
              !std::is_copy_constructible_v<Event> && !std::is_copy_constructible_v<Stream> &&
              !std::is_copy_constructible_v<Graph> && !std::is_copy_constructible_v<GraphExec>);

}  // namespace mppi
