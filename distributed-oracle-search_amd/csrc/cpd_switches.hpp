// The library's environment switches, in one place.  Every optimisation
// switch is on by default and CPD_<NAME>=0 turns it off: the rows and answers
// are identical either way (each fallback runs bit-exact in the GPU tests),
// only the path taken and its speed change.
#pragma once
#include <cstdint>

namespace cpd {

// Process-wide switches: read once, on first use.
struct Switches {
    bool live;          // CPD_LIVE=0: no up-sweep row skipping (every slab computed and stored)
    bool sort;          // CPD_SORT=0: batches keep the caller's target order
    bool lane_key;      // CPD_LANE_KEY=0: cpd_graph_set_coords' keys do not order the targets
    bool xcd;           // CPD_XCD=0: workgroups keep the dispatch order (no XCD-aware remap)
    bool async;         // CPD_ASYNC=0: every emit finishes before its batch returns
    bool rle_fused;     // CPD_RLE_FUSED=0: count / seam repair / emit passes, not the fused emit
    bool leaffm;        // CPD_LEAFFM=0: first_moves computes leaf columns like any other
    bool overlap;       // CPD_OVERLAP=0: no early up-sweep of the next batch
    bool fm_order;      // CPD_FM_ORDER=0: first_moves takes segments in column order
    // Largest auto batch (CPD_BATCH_MAX, a multiple of 1024 in [1024, 32768]).
    // 28672 since the rows are built at the packed width (8.0 MB per target at
    // 1M nodes; profiles/batch_ab/r05am: 387.3k against 380.8k rows/s at 24576).
    uint32_t batch_max;
    bool trace;         // CPD_TRACE=1: host-side phase times of every batch on stderr
    bool search_trace;  // CPD_SEARCH_TRACE=1: the search passes' sizes on stderr
};
const Switches& switches();

// CPD_NARROW=0: dense 32-bit final rows instead of the narrow u16 rows.  Read
// at every cpd_graph_create, not cached: one process builds graphs of both
// kinds and compares them.
bool narrow_rows_on();

// CPD_SEARCH_POOL_WORDS: `words` capped to it — a smaller spill pool, so that
// some records find it full and their searches restart instead.  Read at
// every search call, not cached: one process searches with and without it.
uint64_t search_pool_words(uint64_t words);

// The contraction priority's weights, for the host and the GPU contraction
// alike so that they stay equal: priority = ed * edge difference + deleted *
// contracted neighbours + depth * node depth; the depth bounds the sweep levels.
// CPD_CH_PRIO="ed,deleted,depth" sets them (tuning knob).  Round 3
// (profiles/ch_prio_ab/): 8,2,12 — 166 + 159 levels, 5.20M arcs, 343k rows/s
// on the 1M bench graph — against round 2's 8,2,3 (189 + 194 levels, 5.09M
// arcs, 338k rows/s): fewer latency-bound narrow levels outweigh 2% more arcs
// (8,2,20 / 8,2,30: 343-345k / 345.6k, with the down-sweep's arcs and time
// growing).
struct ChPrio {
    int64_t ed = 8, deleted = 2, depth = 12;
};
ChPrio ch_prio();

}  // namespace cpd
