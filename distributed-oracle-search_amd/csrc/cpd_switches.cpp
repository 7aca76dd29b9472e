#include "cpd_switches.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace cpd {
namespace {

bool env_on(const char* name) {  // an optimisation switch: on unless "0..."
    const char* e = std::getenv(name);
    return !(e && *e == '0');
}
bool env_set(const char* name) {  // a diagnostic: off unless set and not "0..."
    const char* e = std::getenv(name);
    return e && *e && *e != '0';
}

Switches read_switches() {
    Switches s;
    s.live = env_on("CPD_LIVE");
    s.sort = env_on("CPD_SORT");
    s.lane_key = env_on("CPD_LANE_KEY");
    s.xcd = env_on("CPD_XCD");
    s.async = env_on("CPD_ASYNC");
    s.rle_fused = env_on("CPD_RLE_FUSED");
    s.leaffm = env_on("CPD_LEAFFM");
    s.overlap = env_on("CPD_OVERLAP");
    s.fm_order = env_on("CPD_FM_ORDER");
    const char* e = std::getenv("CPD_BATCH_MAX");
    const unsigned long b = e && *e ? std::strtoul(e, nullptr, 10) : 28672ul;
    s.batch_max = (uint32_t)std::max(1024ul, std::min(32768ul, b / 1024ul * 1024ul));
    s.trace = env_set("CPD_TRACE");
    s.search_trace = env_set("CPD_SEARCH_TRACE");
    return s;
}

}  // namespace

const Switches& switches() {
    static const Switches s = read_switches();
    return s;
}

bool narrow_rows_on() { return env_on("CPD_NARROW"); }

uint64_t search_pool_words(uint64_t words) {
    const char* e = std::getenv("CPD_SEARCH_POOL_WORDS");
    return e && *e ? std::min<uint64_t>(words, std::strtoull(e, nullptr, 10)) : words;
}

ChPrio ch_prio() {
    ChPrio p;
    if (const char* e = std::getenv("CPD_CH_PRIO")) {
        long a, b, c;
        if (std::sscanf(e, "%ld,%ld,%ld", &a, &b, &c) == 3) p = {a, b, c};
    }
    return p;
}

}  // namespace cpd
