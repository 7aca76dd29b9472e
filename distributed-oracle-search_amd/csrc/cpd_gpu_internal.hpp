// Private to the GPU half of the C ABI (cpd_device / cpd_graph / cpd_rows /
// cpd_index / cpd_query / cpd_search .cpp): device plumbing and the three objects behind
// the opaque handles of cpd_api.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "cpd_internal.hpp"
#include "cpd_kernels.hpp"
#include "cpd_switches.hpp"

#define HIP_CHECK(expr)                                                          \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess)                                                    \
            throw ::cpd::Error(_e == hipErrorOutOfMemory ? CPD_E_OOM : CPD_E_HIP, \
                               std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace cpd {

// Per-device HBM arena (cpd_device.cpp): allocations inside an ArenaScope are
// carved from the device's arena when one is committed and they fit.
struct ArenaScope {
    ArenaScope();
    ~ArenaScope();
    ArenaScope(const ArenaScope&) = delete;
    ArenaScope& operator=(const ArenaScope&) = delete;
};
void* arena_take(size_t bytes);
bool arena_drop(const void* p);

// Owning device buffer.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && !arena_drop(p)) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        if (count <= n && p) return;
        release();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        if (void* q = arena_take(bytes)) p = static_cast<T*>(q);
        else HIP_CHECK(hipMalloc(&p, bytes));
        n = count;
    }
    void upload(const T* src, size_t count, hipStream_t s) {
        alloc(count);
        if (count) HIP_CHECK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    }
};

// Page-locked host buffer: the staging side of every host<->device copy on
// the build's path.  A pageable source or destination makes hipMemcpyAsync
// wait for the device (the early up-sweep's target upload then waited for
// the whole previous batch).
template <class T>
struct HostBuf {
    T* p = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() {
        if (p) (void)hipHostFree(p);
    }
    void alloc(size_t count) {
        if (count <= n && p) return;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T),
                                hipHostMallocDefault));
        n = count;
    }
};

// One timed interval: a single launch (events on its dispatch packet) or a
// group of consecutive launches of one kernel (events recorded around them).
struct Pending {
    const char* name;
    hipEvent_t a, b;
    double bytes;  // launches whose bytes are known at launch time
    std::vector<std::function<double()>> late;  // bytes known only after the batch ran
    uint64_t launches = 1;
};

struct Agg {
    uint64_t launches = 0;
    double ms = 0.0, bytes = 0.0;
};

hipStream_t thread_stream(int device);  // cpd_device.cpp
void require_device();                  // cpd_device.cpp

// the fused one-pass emit: 4-bit sets only (CPD_RLE_FUSED=0: never)
inline bool rle_fused(uint32_t fmb) { return fmb == 4 && switches().rle_fused; }

}  // namespace cpd

using namespace cpd;

struct cpd_graph {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n = 0, m = 0, npad = 0;
    std::vector<uint32_t> order;       // node -> column
    std::vector<uint32_t> inv;         // column -> node
    DevBuf<uint32_t> order_d;          // node -> column (query preparation)
    DevBuf<uint32_t> inv_d;            // column -> node (path extraction; at first use)
    DevBuf<uint32_t> slot_of_edge_d;   // file edge -> adjacency slot (edge loads; at first use)
    std::vector<uint32_t> edge_perm;   // column-space edge -> file edge
    std::vector<uint32_t> w_free_col;  // free-flow weights, column-space edges
    std::vector<uint32_t> rowc_host;   // column-space row_ptr (host copy)
    std::vector<uint32_t> dst_col_host;  // column-space edge heads (host copy)
    // column-space CSR of the original graph
    DevBuf<uint32_t> row_ptr, dst, w;
    // packed fixed-stride adjacency for table-search: (dst col, w) pairs,
    // 2^adj_shift slots per column, dst = 0xFFFFFFFF past the out-degree
    uint32_t adj_shift = 0;
    DevBuf<uint32_t> adj;

    std::vector<uint32_t> packed_adjacency(const std::vector<uint32_t>& wcol) const {
        const size_t stride = (size_t)1 << adj_shift;
        std::vector<uint32_t> a(2 * stride * n, 0xFFFFFFFFu);
        for (uint32_t c = 0; c < n; ++c)
            for (uint32_t e = rowc_host[c]; e < rowc_host[c + 1]; ++e) {
                size_t slot = ((size_t)c * stride + (e - rowc_host[c])) * 2;
                a[slot] = dst_col_host[e];
                a[slot + 1] = wcol[e];
            }
        return a;
    }
    // sweeps: level-ordered node lists, per-slot arc offsets, (col, w) arcs
    DevBuf<uint32_t> asc_nodes, asc_off, asc_arcs;
    DevBuf<uint32_t> dsc_nodes, dsc_off, dsc_arcs, dsc_desc;
    std::vector<uint32_t> asc_lvl, dsc_lvl;         // level -> first slot
    // bytes model: gathered arcs and own-row reads per level
    std::vector<double> asc_lvl_arcs, dsc_lvl_arcs, dsc_lvl_reads;
    std::vector<uint32_t> asc_off_host;
    uint64_t ch_arcs = 0;
    bool has_ch = false;
    // batch workspace
    uint32_t B = 0;
    uint32_t fmb = 16;  // bits per first-move set (fm_bits(adj_shift))
    // bits per move in the packed compact form: every move indexes its
    // column's out-list (wildcard runs take bit 0), so out-degrees <= 2^bits
    uint32_t move_bits = 4;
    // the move tables in HBM (built rows, dense indexes) at the same width:
    // 2^tlb bits per column
    uint32_t tlb = 2;
    // dist: the dense final rows (narrow rows off only); counts: run counts
    DevBuf<uint32_t> dist, counts;
    // The compact up stores, one per batch slot (see BatchSlot): up[u][B],
    // u = ascending slot - ubase for the n_up nodes of up-level >= 2, their
    // live masks and the batch's target masks.
    uint32_t ubase = 0, n_up = 0;
    DevBuf<uint32_t> upx[2], livex[2], tmaskx[2];
    DevBuf<uint32_t> dsc_up;  // descending slot -> up index (~0: closed form)
    // Emit overlap (CPD_ASYNC, default on): a batch's move-table emit
    // (rle_moves) runs on `estream` while the next batch's sweeps start on
    // `stream` — the sweeps' narrow, latency-bound levels overlap the emit.
    // The buffers the emit reads (first-move rows, RLE segment states, lane ->
    // row map) come in up to kSets sets used round robin: set x is reused
    // only after the emit that read it (ev_emit[x]) has finished.  Three
    // sets give an emit two steps to finish: it runs at low occupancy beside
    // the sweeps, and with two sets the next-but-one batch's first moves
    // waited ~16 ms per step for it (profiles/up_store_ab/, round 6).
    static constexpr uint32_t kSets = 3;
    hipStream_t estream = nullptr;
    bool async = false;
    uint32_t nsets = 1, cur = 0;
    hipEvent_t ev_emit[kSets] = {nullptr, nullptr, nullptr};
    bool emit_pending[kSets] = {false, false, false};
    DevBuf<uint32_t> fmx[kSets];      // [B][npad] fmb-bit sets
    DevBuf<uint32_t> rle_stx[kSets];  // [B][npad/32] RLE segment entry states
    DevBuf<uint8_t> rle_rcx[kSets];   // [B][npad/32] runs ending in each segment
    DevBuf<uint32_t> lane_rowx[kSets];  // [B] table row of each batch lane
    // chunk exit states / run counts of the chunked count (read by rle_fix on
    // the same stream before the next batch: one set)
    DevBuf<uint32_t> rle_xs, rle_cc, rle_hard;
    DevBuf<uint32_t> emit_ck;  // fused emit: the chunks' guessed entries, exits, breaks
    HostBuf<uint32_t> rle_hard_h;          // [1]
    // the buffer set the next batch uses, once the emit that last read it is done
    uint32_t acquire_set() {
        const uint32_t x = cur;
        cur = (cur + 1u) % nsets;
        if (emit_pending[x]) {
            HIP_CHECK(hipStreamWaitEvent(stream, ev_emit[x], 0));
            emit_pending[x] = false;
        }
        return x;
    }
    void drain_emits() {
        if (estream) HIP_CHECK(hipStreamSynchronize(estream));
        for (auto& p : emit_pending) p = false;
    }
    // leaf first moves from the down-sweep (4-bit sets only): leafbits[col/32]
    // bit = column is a CH leaf; fmleaf [col][B/4] u16 = its sets, 4 per lane
    bool leaf_fm = false;
    DevBuf<uint32_t> leafbits;
    DevBuf<uint16_t> fmleaf;
    // narrow final-distance rows (NarrowRows, cpd_kernels.hpp): on unless
    // CPD_NARROW=0 at graph creation or a finite distance could reach the
    // wide-row marker; group rows that do not fit are kept wide in the pool
    // (counted: ovf)
    bool narrow = false;
    // the first kNarrowProbe full batches count their wide group rows; if
    // most are wide (long edges: the spread of 256 distances passes 0xFFFF),
    // narrow rows only add a base load per gather and are switched off for
    // the graph's lifetime — the results are identical either way
    static constexpr uint32_t kNarrowProbe = 2;
    uint32_t narrow_probe = kNarrowProbe;
    HostBuf<uint32_t> ovf_hb;  // [1] wide group rows of the last down-sweep
    uint32_t ovf_h() const { return ovf_hb.p ? ovf_hb.p[0] : 0u; }
    DevBuf<uint16_t> d16;
    DevBuf<uint32_t> dbase, ovf, pool;
    uint32_t pool_cap = 0;
    NarrowRows narrow_rows(bool on) {
        if (!on) return NarrowRows{nullptr, nullptr, n, nullptr, nullptr, 0};
        return NarrowRows{d16.p, dbase.p, n, ovf.p, pool.p, pool_cap};
    }
    double n_leaf = 0, m_leaf = 0;    // leaves, their out-edges
    std::vector<double> dsc_lvl_leaves;
    // Per-batch state, two slots (batches alternate): a batch's up-sweep runs
    // (on ustream) while the previous batch's down-sweep reads the other
    // slot's up store.  tgt: the batch's target columns by lane; pos_of[i] =
    // lane of the caller's target i; stat: per-level sweep counters (timing
    // runs; 2 per launch: stored / own rows, gathered rows), stat_h its host
    // copy; up_late: (level, arcs, nodes) of the up levels whose bytes wait
    // for it.  ev_fm[slot] marks the end of the slot's batch (its first
    // moves); its down-sweep is the last reader of its up store, live and
    // target masks and stats, and first moves read the targets from fm_tgt.
    struct BatchSlot {
        DevBuf<uint32_t> tgt;
        std::vector<uint32_t> pos_of, tgt_col;
        HostBuf<uint32_t> tgt_h;  // upload staging
        DevBuf<unsigned int> stat;
        HostBuf<unsigned int> stat_h;
        std::vector<std::array<double, 3>> up_late;
    };
    BatchSlot bs[2];
    DevBuf<uint32_t> fm_tgt;  // the targets of the batch whose first moves are queued
    // Timing runs: a batch's sweep bytes that depend on its live-row counts
    // (stat_h, copied out after its first moves), folded into agg once those
    // have landed — at the end of the next batch, or at timing_get / reset.
    // up: (level, arcs, nodes) per up level; down: (stat index, known bytes).
    struct LateRec {
        uint32_t slot = 0;
        std::vector<std::array<double, 3>> up;
        std::vector<std::array<double, 2>> down;
    };
    std::vector<LateRec> late_q;
    uint32_t next_slot = 0;
    // Early up-sweep of the next batch:
    // build_batch launches it on ustream right after queueing the current
    // batch's down-sweep, into the other slot's up store, so it runs beside
    // that down-sweep.  prep: the slot and targets it was launched for, ev_up
    // its end.
    hipStream_t ustream = nullptr;
    hipEvent_t ev_up = nullptr, ev_down = nullptr, ev_fm[2] = {nullptr, nullptr};
    bool prepped = false;
    uint32_t prep_slot = 0;
    std::vector<uint32_t> prep_targets, hint;
    void drop_prep() {  // wait for an early up-sweep nobody will use
        if (ustream) HIP_CHECK(hipStreamSynchronize(ustream));
        prepped = false;
    }
    DevBuf<uint32_t> asc_lvl_of, dsc_lvl_of;  // slot -> level
    // narrow upward levels (<= kNarrow nodes) run chunked: per level l,
    // items [up_item_first[l], up_item_first[l+1]) of (slot, a0, a1, 0);
    // up_init_slots = the ascending slots of all their nodes (leaf-form init)
    std::vector<uint32_t> up_item_first;
    DevBuf<uint32_t> up_items, up_init_slots;
    uint32_t n_init_slots = 0;
    // lane position of each caller target in the current batch (sorted by
    // lane_key when the caller gave coordinates, else by column)
    std::vector<uint32_t> lane_key;  // node -> Hilbert key of its coordinates (may be empty)
    // first_moves' segment order: the 32-column segments by the Hilbert key
    // of their middle column's node (empty: column order)
    DevBuf<uint32_t> seg_order;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<Pending> pending;
    std::map<std::string, Agg> agg;

    ~cpd_graph();

    hipEvent_t get_event() {
        if (ev_pool.empty()) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            return e;
        }
        hipEvent_t e = ev_pool.back();
        ev_pool.pop_back();
        return e;
    }
    // Time one launch when timing is on: the events are attached to the
    // kernel's own dispatch packet (hipExtLaunchKernelGGL, see launchers).
    // Inside group_begin(name) / group_end() the launches of `name` carry no
    // events: one pair recorded around the whole run of launches times them
    // (per-packet profiling signals cost ~7 us per launch, ~3 % of a batch's
    // ~580 sweep launches; the group interval also counts the inter-kernel
    // gaps, so its per-launch average is a slight over-estimate).
    // Every launch is checked: hipGetLastError() is cleared first, so an
    // error left behind by an unrelated earlier runtime call on this thread
    // (it is sticky until read) is not blamed on the launch.
    template <class F>
    void timed(const char* name, double bytes, F&& launch,
               std::function<double()> late_bytes = nullptr);
    Pending group;
    bool group_open = false;
    hipStream_t group_stream = nullptr;
    void group_begin(const char* name, hipStream_t st);
    void group_end();
    // Wait for `stream` (all = also the emit stream), then fold the timed
    // intervals that have completed into agg; intervals of an emit still
    // running on estream stay pending until a later sync.
    void sync(bool all = false);
    void select() const { HIP_CHECK(hipSetDevice(device)); }
    uint32_t wpr() const { return npad >> (5u - tlb); }  // words per move-table row

    uint64_t hbm_reserve = 0;  // cpd_graph_set_hbm_reserve
    void reserve_batch(uint32_t want);
    // The final rows of a batch of B: narrow (u16 offsets, bases, the pool of
    // wide group rows) or the dense 32-bit rows.
    void alloc_final_rows();
};

struct cpd_rows {
    int device = 0;
    uint32_t nrows = 0;
    mutable uint64_t total = 0;  // runs of all rows (valid after settle())
    hipEvent_t done = nullptr;   // after the last batch's count + emit (emit stream)
    void wait() const {
        if (done) HIP_CHECK(hipEventSynchronize(done));
    }
    ~cpd_rows() {
        if (done) {
            (void)hipEventSynchronize(done);
            (void)hipEventDestroy(done);
        }
    }
    // A batch's run counts arrive after its rows are queued: the count pass
    // runs on the emit stream, beside the next batch's sweeps.  Per batch:
    // its rows' lanes and two page-locked buffers — the lane -> table row map
    // the emit reads and the per-lane run counts it lands — turned into run
    // offsets by settle() once `done` has passed.  A rebuild into these rows
    // retires the unsettled batches (their copies may still be in flight).
    struct Batch {
        uint32_t k = 0;
        std::vector<uint32_t> pos_of;
        HostBuf<uint32_t> lane_rows, counts;
        hipEvent_t ev = nullptr;  // after the batch's last copy (emit stream)
        ~Batch() {
            if (ev) (void)hipEventDestroy(ev);
        }
    };
    mutable std::mutex settle_mu;
    mutable std::vector<std::unique_ptr<Batch>> pending, retired, spare;
    Batch* new_batch(uint32_t B);
    void retire() {
        for (auto& b : pending) retired.push_back(std::move(b));
        pending.clear();
    }
    void settle() const;
    std::vector<uint32_t> targets;   // node ids, row order
    std::vector<uint32_t> lanes;     // batch lane of each row
    mutable std::vector<uint64_t> offsets;  // run offsets (host), nrows+1 (after settle())
    // The rows in their compact form: move tables at 2^tlb bits per column,
    // wpr = npad * 2^tlb / 32 words per row (rle_moves) — the RLE row
    // expanded, 10x smaller than its runs on the bench graph (2 bits).  Run
    // words are decoded from them on demand (moves_runs, at `off`).
    uint32_t n = 0, wpr = 0, bits = 4, tlb = 2;  // bits: per move in the exported form
    DevBuf<uint32_t> moves;
    mutable DevBuf<uint64_t> off;
    uint32_t packed_words() const { return (uint32_t)(((uint64_t)n * bits + 31u) / 32u); }
    // device staging for decoded runs, one buffer per concurrent exporter
    // (make_cpd_auto's writer threads), kept until the rows are freed
    mutable std::mutex stage_mu;
    mutable std::vector<std::unique_ptr<DevBuf<uint32_t>>> stages;
    std::unique_ptr<DevBuf<uint32_t>> acquire_stage() const {
        std::lock_guard<std::mutex> l(stage_mu);
        if (stages.empty()) return std::make_unique<DevBuf<uint32_t>>();
        auto b = std::move(stages.back());
        stages.pop_back();
        return b;
    }
    void release_stage(std::unique_ptr<DevBuf<uint32_t>> b) const {
        std::lock_guard<std::mutex> l(stage_mu);
        stages.push_back(std::move(b));
    }
};

// A table-search index: nrows rows (row i = target row_targets[i]) that arrive
// in append order — all at once (cpd_index_create / _from_rows) or streamed
// (cpd_index_create_empty + cpd_index_append_*).  Two HBM forms:
//   keep_rle      the RLE runs stay resident (offsets + runs); dense tables,
//                 if asked for, are expanded from them on first use;
//   stream_dense  each appended chunk is expanded into the 4-bit move tables
//                 straight away and its runs are dropped, so a worker whose
//                 runs outgrow HBM (1M nodes div 8: ~312 GB of runs, 62.5 GB
//                 of tables) is still served.
struct cpd_index {
    cpd_graph* g = nullptr;
    // g->device, kept here so that cpd_index_free never reads a graph that was
    // freed first (a garbage collector finalises a cycle in any order)
    int device = 0;
    uint32_t nrows = 0;   // rows when complete
    uint32_t added = 0;   // rows appended so far
    uint64_t total = 0;   // runs resident so far (keep_rle)
    uint64_t cap = 0;     // run capacity of `runs` (keep_rle)
    uint64_t declared = 0;  // total runs of all rows (from the caller or the rows)
    std::vector<uint32_t> row_of_col;   // host copy
    std::vector<uint32_t> row_targets;  // declared targets, row order
    std::vector<uint64_t> offsets;      // host copy, added + 1 (keep_rle)
    DevBuf<uint32_t> d_row_of_col, runs, adj_sel;  // adj_sel: packed adjacency, custom weights
    DevBuf<uint64_t> off;
    bool custom_w = false;
    // CPD_INDEX_AUTO / _RLE / _DENSE; dense = 4-bit move tables expanded from
    // the RLE rows (built on first use, or as rows stream in)
    int mode = CPD_INDEX_AUTO;
    bool keep_rle = true;
    bool stream_dense = false;
    DevBuf<uint32_t> dense;
    bool dense_ready = false;
    // staging of host-appended chunks (stream_dense), format flag
    DevBuf<uint32_t> stage, pstage;  // pstage: packed compact rows before unpacking
    DevBuf<uint32_t> xstage, lost;   // nibble rows before narrowing; repack's flag
    DevBuf<uint64_t> stage_off;
    DevBuf<uint32_t> flag;
    // expand_rows work split: first run-chunk of each row being expanded
    std::vector<uint32_t> chunk_first_h;
    DevBuf<uint32_t> chunk_first;

    bool use_dense() const {
        if (stream_dense) return true;
        if (mode == CPD_INDEX_DENSE) return true;
        if (mode == CPD_INDEX_RLE) return false;
        // auto: the table whose bytes are fewer (4 B per run vs npad * bits / 8
        // B per row)
        return nrows > 0 && 4.0 * (double)declared > 4.0 * (double)g->wpr() * nrows;
    }
    // the adjacency a walk that costs its moves reads: the custom weights' when set
    const uint32_t* walk_adj() const { return custom_w ? adj_sel.p : g->adj.p; }
    // CPD-search: per-row tables when they fit (hrow free-flow heuristic,
    // crow / lrow incumbent cost and moves under the current weights; rebuilt
    // for new weights), row target columns, workspace (per lane slot),
    // per-query counters, sums
    DevBuf<uint64_t> hrow, crow;
    DevBuf<uint32_t> lrow, tcol, qstats;
    DevBuf<uint8_t> sws;
    DevBuf<unsigned long long> sagg;
    // resumable overflow: the two spill pools (records of the pass that just
    // ran / of the one running), their bump counters, record offsets
    DevBuf<uint32_t> spool[2];
    DevBuf<unsigned long long> stop, sat;
    bool h_ready = false, c_ready = false;
    bool searched = false;  // qstats hold the counters of the prepared queries
    // query workspace; queries run sorted by target row (qperm[i] = caller
    // index of sorted query i), all of it prepared on the GPU
    uint32_t nq = 0;
    DevBuf<uint32_t> qin_s, qin_t, qkey, qkey2, qval, qperm, qbad;
    DevBuf<uint8_t> qsort_tmp, qout;
    DevBuf<uint32_t> qs, qt, qrow, hops;
    DevBuf<uint64_t> cost;
    DevBuf<uint8_t> fin;
    DevBuf<unsigned long long> agg;
    // path extraction (cpd_query_paths): node counts and path offsets in the
    // caller's order (device, host copy), the nodes; paths_ready: they are
    // those of the prepared queries
    DevBuf<uint64_t> plens, poff;
    std::vector<uint64_t> poff_h;
    DevBuf<uint32_t> pnodes;
    bool paths_ready = false;
    // costs under several weight sets (cpd_index_set_weight_sets /
    // cpd_query_costs): the set table — a record of wset_words (4 or 8) u32
    // per adjacency slot, word j = the slot's weight in set j — and the
    // result buffers of the last cpd_query_costs in sorted order (cs_cols
    // values per query: nsets, or 1 when sliced); costs_ready: they are those
    // of the prepared queries.  Independent of adj_sel / custom_w.  Carved
    // from the arena when one is committed, like every DevBuf allocated
    // inside an ArenaScope: the arena never takes them back, so a larger
    // table or batch than any before uses up that many more arena bytes.
    DevBuf<uint32_t> wsets;
    uint32_t nsets = 0, wset_words = 0;
    DevBuf<uint64_t> cs_cost;
    DevBuf<uint32_t> cs_hops;
    DevBuf<uint8_t> cs_fin;
    uint32_t cs_cols = 0;
    bool costs_ready = false;
    // edge loads (cpd_query_loads): the resident table in slot space —
    // ld_slices planes of n << adj_shift u64 counters, counter (column <<
    // adj_shift) + move — kept across prepares until cpd_query_loads_clear;
    // ld_slice_moves: the moves per slice it was filled with (0: one plane);
    // ld_period: non-zero for a table cpd_query_timed filled — its planes are
    // the intervals [j * ld_period, (j + 1) * ld_period) of clock time, the
    // last open-ended, ld_slices = the sets it was filled under, ld_slice_moves
    // = 0; a table is of one kind, accumulated into only by its own
    // (cpd_query_search_loads fills and adds to the one-plane kind).
    // The batch's demand (caller order) and the fetch's edge-order copy.  The
    // table is carved from the arena when one is committed (see wsets above).
    DevBuf<uint64_t> ld_tab, ld_out;
    DevBuf<uint32_t> ld_demand;
    uint32_t ld_slices = 0, ld_slice_moves = 0;
    uint64_t ld_period = 0;
    bool loads_ready = false;
    // timed walks (cpd_query_timed): the batch's departures (caller order)
    // and the result buffers of the last call in sorted order; timed_ready:
    // they are those of the prepared queries.  Carved like cs_cost.
    DevBuf<uint64_t> tm_depart, tm_cost;
    DevBuf<uint32_t> tm_hops;
    DevBuf<uint8_t> tm_fin;
    bool timed_ready = false;
    // search paths (cpd_query_search_paths, _search_loads), scratch of one call, freed when
    // it returns (the cursor stays): the prefix pool and its cursor;
    // per query (sorted order) the prefix's place and length, v* and lw(v*);
    // the suffix walk's offset pairs and their index (search_path_plan)
    DevBuf<uint32_t> spp_pool, spp_pn, spp_vcol, spp_vlw, spp_wperm;
    DevBuf<unsigned long long> spp_top, spp_off;
    DevBuf<uint64_t> spp_woff;
    // loads to weights (cpd_index_weights_from_loads, cpd_query_assign): the
    // call's capacities as uploaded (edge order) and permuted to slot order,
    // the 128-bit sum and the changed count; the edge-order copy of a weights
    // fetch (cpd_index_get_weights / _weight_sets).  Carved like ld_tab.
    DevBuf<uint32_t> vdf_cap_in, vdf_cap, vdf_out;
    DevBuf<unsigned long long> vdf_acc;
    // the flow step (cpd_index_flow_step, cpd_query_assign_line): the flow
    // table — one u64 X (Q16) per adjacency slot, the load table's order —
    // kept until cpd_index_flow_clear, independent of ld_tab; the step's
    // device state (kFlowWords, assign_kernels.hpp) and the fetch's
    // edge-order copy.  Carved like ld_tab.
    DevBuf<uint64_t> fl_tab, fl_out;
    DevBuf<unsigned long long> fl_st;
    bool flow_ready = false;
    // the conjugate step (cpd_index_flow_step_conj, cpd_query_assign_conj):
    // the target table S beside fl_tab, same layout; target_ready only after
    // a conjugate step, dropped by cpd_index_flow_step and _flow_clear.
    DevBuf<uint64_t> tg_tab;
    bool target_ready = false;
    // the bi-conjugate step (cpd_index_flow_step_bi, cpd_query_assign_bi): the
    // second target table S2 (the target before tg_tab's), same layout, and
    // the lambda of the last such step; every other step and _flow_clear drop
    // S2, and lambda_prev is 65536 whenever S2 is not resident.
    DevBuf<uint64_t> tg2_tab;
    bool target2_ready = false;
    uint32_t lambda_prev = 65536u;
};

template <class F>
void cpd_graph::timed(const char* name, double bytes, F&& launch,
           std::function<double()> late_bytes) {
    (void)hipGetLastError();
    if (!timing) {
        launch();
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (group_open && std::strcmp(group.name, name) == 0) {
        launch();
        HIP_CHECK(hipGetLastError());
        if (late_bytes) group.late.push_back(std::move(late_bytes));
        else group.bytes += bytes;
        group.launches++;
        return;
    }
    hipEvent_t a = get_event(), b = get_event();
    set_launch_events(a, b);
    launch();
    HIP_CHECK(hipGetLastError());
    Pending p{name, a, b, late_bytes ? 0.0 : bytes, {}, 1};
    if (late_bytes) p.late.push_back(std::move(late_bytes));
    pending.push_back(std::move(p));
}

// Events taken from a graph's pool for the steps of one call: they go back
// to the pool however the call ends.
template <int N>
struct Events {
    cpd_graph* g;
    hipEvent_t e[N];
    explicit Events(cpd_graph* gr) : g(gr) {
        for (hipEvent_t& x : e) x = g->get_event();
    }
    ~Events() {
        for (hipEvent_t x : e) g->ev_pool.push_back(x);
    }
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
};

namespace cpd {
// Helpers that cross the units (defined in the unit named).
void fold_late(cpd_graph* g, size_t keep);  // cpd_rows.cpp
void ensure_dense(cpd_index* ix);           // cpd_index.cpp
void reset_load_table(cpd_index* ix, uint32_t planes, uint32_t slice_moves,
                      uint64_t period);     // cpd_index.cpp
void ensure_slot_of_edge(cpd_graph* g);     // cpd_index.cpp
// cpd_query.cpp: checks and the paths tail its calls share with cpd_search.cpp's.
// `who` is the call's message prefix ("loads", "search paths", ...).
void require_complete(const cpd_index* ix, const char* who);  // every declared row appended
void require_load_slots(const cpd_graph* g, const char* who);  // adjacency slots fit the load kernels' u32
// The tail of cpd_query_paths / _search_paths: the empty batch's return; the
// offsets (ix->poff) copied to poff_h and pnodes carved for their total, which
// is returned; poff_h copied out and paths_ready set.
void paths_empty(cpd_index* ix, uint64_t* offsets);
uint64_t paths_reserve(cpd_index* ix, const char* who);
void paths_copy_out(cpd_index* ix, uint64_t* offsets);
}  // namespace cpd
