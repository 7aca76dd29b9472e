// Test harness (tests/test_host_abi.py): the argument-checking paths of the
// GPU half of the C ABI that need no device, called on the library's own
// cpd_device / cpd_graph / cpd_rows / cpd_index / cpd_search sources built
// with -fsanitize=address,undefined.  Prints one "ok <what>" line per check,
// "FAIL <what>: ..." otherwise; exit status = number of failures.
#include <cstdio>
#include <cstring>
#include <string>

#include "cpd_api.h"

static int failures = 0;

static void expect(const char* what, int rc, int want_rc, const char* want_msg) {
    const bool ok = rc == want_rc && (!want_msg || std::strstr(cpd_last_error(), want_msg));
    if (ok) {
        std::printf("ok %s\n", what);
    } else {
        std::printf("FAIL %s: rc %d (want %d), last error \"%s\"\n", what, rc, want_rc,
                    cpd_last_error());
        ++failures;
    }
}

int main() {
    int count = -1;
    expect("device_count", cpd_device_count(&count), CPD_OK, nullptr);
    expect("device_count >= 0", count >= 0 ? CPD_OK : CPD_E_ARG, CPD_OK, nullptr);
    expect("device_count(null)", cpd_device_count(nullptr), CPD_E_ARG, "null count");

    uint64_t b1 = 0, b2 = 0;
    expect("batch_bytes(1000)", cpd_batch_bytes(1000, 4, 1000, &b1), CPD_E_ARG,
           "batch_bytes: batch must be a positive multiple of 1024");
    expect("batch_bytes(0)", cpd_batch_bytes(1000, 4, 0, &b1), CPD_E_ARG,
           "batch_bytes: batch must be a positive multiple of 1024");
    expect("batch_bytes(null)", cpd_batch_bytes(1000, 4, 1024, nullptr), CPD_E_ARG,
           "batch_bytes: batch must be a positive multiple of 1024");
    expect("batch_bytes(1024)", cpd_batch_bytes(1000, 4, 1024, &b1), CPD_OK, nullptr);
    expect("batch_bytes(2048)", cpd_batch_bytes(1000, 4, 2048, &b2), CPD_OK, nullptr);
    // the fixed part: 4096 n + 512 n + 64 MiB; the rest grows with the batch
    expect("batch_bytes grows", b1 > 4608ull * 1000 + (64ull << 20) && b2 > b1 ? CPD_OK : CPD_E_ARG,
           CPD_OK, nullptr);

    cpd_graph* g = reinterpret_cast<cpd_graph*>(1);
    expect("graph_create(null plan)", cpd_graph_create(nullptr, 0, &g), CPD_E_ARG,
           "graph: null argument");
    expect("graph_create(null out)", cpd_graph_create(nullptr, 0, nullptr), CPD_E_ARG,
           "graph: null argument");
    expect("query_search(null)", cpd_query_search(nullptr, nullptr, nullptr), CPD_E_ARG,
           "null index");
    expect("query_paths(null)", cpd_query_paths(nullptr, -1, nullptr, nullptr), CPD_E_ARG,
           "paths: null argument");

    expect("host_alloc(null out)", cpd_host_alloc(16, nullptr), CPD_E_ARG,
           "host alloc: null output");
    void* p = reinterpret_cast<void*>(1);
    if (count > 0) {
        expect("host_alloc", cpd_host_alloc(16, &p), CPD_OK, nullptr);
        expect("host_alloc pointer", p ? CPD_OK : CPD_E_ARG, CPD_OK, nullptr);
        if (p) std::memset(p, 0, 16);
    } else {
        expect("host_alloc without a device", cpd_host_alloc(16, &p), CPD_E_HIP,
               "no HIP device available (libcpd has no CPU fallback)");
        expect("host_alloc leaves null", p == nullptr ? CPD_OK : CPD_E_ARG, CPD_OK, nullptr);
    }
    cpd_host_free(p);
    cpd_host_free(nullptr);
    expect("arena_release without an arena", cpd_device_arena_release(0), CPD_OK, nullptr);

    std::printf("%d failures\n", failures);
    return failures;
}
