// Device plumbing of the C ABI: the per-device HBM arena, the per-thread
// streams, device queries and page-locked host memory.
#include "cpd_gpu_internal.hpp"

namespace {

// Per-device HBM arena (cpd_device_arena): one block committed up front —
// e.g. on a host thread while the plan is being contracted — that the
// long-lived bulk buffers on that device are carved from (bump allocation:
// a carved buffer is never returned to it, the whole block is freed by
// cpd_device_arena_release).  Only allocations inside an ArenaScope are
// carved — a build's batch buffers, its row sets, an index's move tables —
// so short-lived scratch never fills it; what does not fit
// falls back to hipMalloc.  `live` counts the carved buffers still held:
// the release refuses while any is.
struct Arena {
    char* base = nullptr;
    size_t cap = 0, top = 0;
    size_t live = 0;
};
std::mutex g_arena_mu;
std::map<int, Arena> g_arena;
thread_local int t_arena_scope = 0;

}  // namespace

namespace cpd {

ArenaScope::ArenaScope() { ++t_arena_scope; }
ArenaScope::~ArenaScope() { --t_arena_scope; }

void* arena_take(size_t bytes) {
    if (t_arena_scope <= 0) return nullptr;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> l(g_arena_mu);
    auto it = g_arena.find(d);
    if (it == g_arena.end() || !it->second.base) return nullptr;
    Arena& a = it->second;
    const size_t at = (a.top + 255u) & ~(size_t)255u;
    if (at + bytes > a.cap) return nullptr;
    a.top = at + bytes;
    ++a.live;
    return a.base + at;
}

// true (and one live buffer fewer) when p was carved from an arena
bool arena_drop(const void* p) {
    std::lock_guard<std::mutex> l(g_arena_mu);
    for (auto& kv : g_arena) {
        const char* c = static_cast<const char*>(p);
        if (kv.second.base && c >= kv.second.base && c < kv.second.base + kv.second.cap) {
            if (kv.second.live) --kv.second.live;
            return true;
        }
    }
    return false;
}

// One non-blocking stream per (host thread, device), kept for the thread's
// lifetime: exports from several host threads never queue behind a build's
// stream or each other.
hipStream_t thread_stream(int device) {
    thread_local std::vector<hipStream_t> streams;
    if (streams.size() <= (size_t)device) streams.resize(device + 1, nullptr);
    hipStream_t& st = streams[device];
    if (!st) HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    return st;
}

void require_device() {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        throw Error(CPD_E_HIP, "no HIP device available (libcpd has no CPU fallback)");
}

}  // namespace cpd

extern "C" {

int cpd_device_count(int* count) {
    return guarded([&] {
        CPD_REQUIRE(count, CPD_E_ARG, "null count");
        hipError_t e = hipGetDeviceCount(count);
        if (e != hipSuccess) *count = 0;
    });
}

int cpd_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
    return guarded([&] {
        CPD_REQUIRE(free_bytes && total_bytes, CPD_E_ARG, "null argument");
        require_device();
        int count = 0;
        HIP_CHECK(hipGetDeviceCount(&count));
        CPD_REQUIRE(device >= 0 && device < count, CPD_E_ARG, "no such device");
        HIP_CHECK(hipSetDevice(device));
        size_t f = 0, t = 0;
        HIP_CHECK(hipMemGetInfo(&f, &t));
        *free_bytes = f;
        *total_bytes = t;
    });
}

int cpd_device_arena(int device, uint64_t bytes, int touch) {
    return guarded([&] {
        require_device();
        int count = 0;
        HIP_CHECK(hipGetDeviceCount(&count));
        CPD_REQUIRE(device >= 0 && device < count, CPD_E_ARG, "no such device");
        HIP_CHECK(hipSetDevice(device));
        {
            std::lock_guard<std::mutex> l(g_arena_mu);
            CPD_REQUIRE(!g_arena[device].base, CPD_E_ARG, "device arena already committed");
        }
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<uint64_t>(bytes, 256)));
        if (touch) {  // first-touch costs paid here, off the build's path
            HIP_CHECK(hipMemset(p, 0, std::max<uint64_t>(bytes, 256)));
            HIP_CHECK(hipDeviceSynchronize());
        }
        std::lock_guard<std::mutex> l(g_arena_mu);
        g_arena[device] = Arena{static_cast<char*>(p), (size_t)std::max<uint64_t>(bytes, 256), 0};
    });
}

int cpd_device_arena_release(int device) {
    return guarded([&] {
        char* p = nullptr;
        {
            std::lock_guard<std::mutex> l(g_arena_mu);
            auto it = g_arena.find(device);
            if (it == g_arena.end()) return;
            CPD_REQUIRE(it->second.live == 0, CPD_E_ARG,
                        "device arena still holds " + std::to_string(it->second.live) +
                            " live buffers: free the graphs, row sets and indexes first");
            p = it->second.base;
            g_arena.erase(it);
        }
        if (p) {
            HIP_CHECK(hipSetDevice(device));
            HIP_CHECK(hipFree(p));
        }
    });
}

int cpd_host_alloc(size_t bytes, void** out) {
    return guarded([&] {
        CPD_REQUIRE(out, CPD_E_ARG, "host alloc: null output");
        *out = nullptr;
        require_device();
        HIP_CHECK(hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault));
    });
}

void cpd_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

}  // extern "C"
