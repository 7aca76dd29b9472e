// The query calls on a table-search index (cpd_query_*): query preparation,
// the walk and its variants (costs under weight sets, edge loads, timed walks)
// behind one host frame, path extraction and the fetches.  The index itself
// — its rows, tables, weights and load table — is cpd_index.cpp's; the search
// calls are cpd_search.cpp's and share the paths tail and the checks below.
#include <cmath>

#include "cpd_gpu_internal.hpp"

void cpd::require_complete(const cpd_index* ix, const char* who) {
    CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                std::string(who) + ": index incomplete (" + std::to_string(ix->added) + " of " +
                    std::to_string(ix->nrows) + " rows appended)");
}

// the load kernels keep a slot as u32, 0xFFFFFFFF = none
void cpd::require_load_slots(const cpd_graph* g, const char* who) {
    CPD_REQUIRE(((uint64_t)g->n << g->adj_shift) < 0xFFFFFFFFull, CPD_E_RANGE,
                std::string(who) + ": 2^32 adjacency slots or more");
}

void cpd::paths_empty(cpd_index* ix, uint64_t* offsets) {
    offsets[0] = 0;
    ix->poff_h.assign(1, 0);
    ix->paths_ready = true;
}

// The nodes come from the arena when there is one: it is a bump allocator, so
// a batch with more nodes than any before it carves a new buffer and the old
// one's bytes stay taken until cpd_device_arena_release; a batch that fits the
// buffer it has allocates nothing.
uint64_t cpd::paths_reserve(cpd_index* ix, const char* who) {
    cpd_graph* g = ix->g;
    const uint32_t nq = ix->nq;
    ix->poff_h.resize((size_t)nq + 1u);
    HIP_CHECK(hipMemcpyAsync(ix->poff_h.data(), ix->poff.p, ((size_t)nq + 1u) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipStreamSynchronize(g->stream));
    const uint64_t total = ix->poff_h[nq];
    try {
        ArenaScope carve;
        ix->pnodes.alloc((size_t)total);
    } catch (const Error& e) {
        (void)hipGetLastError();
        if (e.code != CPD_E_OOM) throw;
        throw Error(CPD_E_OOM, std::string(who) + ": " + std::to_string(4ull * total) +
                                   " bytes of HBM for " + std::to_string(total) +
                                   " path nodes of " + std::to_string(nq) + " queries do not fit");
    }
    return total;
}

void cpd::paths_copy_out(cpd_index* ix, uint64_t* offsets) {
    std::memcpy(offsets, ix->poff_h.data(), ((size_t)ix->nq + 1u) * sizeof(uint64_t));
    ix->paths_ready = true;
}

namespace {

// Algorithmic bytes of a table-search walk of nq queries and `moves` moves.
double walk_model_bytes(const cpd_index* ix, bool dense, uint32_t nq, uint64_t moves) {
    // dense: per query 8 (s,t) + 13 (outputs) + 4 (row); per move one 4-B
    // move word + one 8-B packed edge
    if (dense) return 25.0 * nq + 12.0 * (double)moves;
    // SURVEY.md §8(d) B_q = 8 + 12 + 8 + L * (4 ceil(log2 R) + 16)
    double mean_log = 0.0;
    if (ix->nrows) {
        double s = 0.0;
        for (uint32_t i = 0; i < ix->nrows; ++i)
            s += std::ceil(std::log2((double)std::max<uint64_t>(
                2, ix->offsets[i + 1] - ix->offsets[i])));
        mean_log = s / ix->nrows;
    }
    return 28.0 * nq + (double)moves * (4.0 * mean_log + 16.0);
}

// The rows a walk reads, dense tables made at their first use.  An entry
// point's first step: should the tables not fit (CPD_E_RANGE, CPD_E_OOM), the
// call has changed nothing yet.
void resolve_rows(cpd_index* ix) {
    if (ix->use_dense() && !ix->dense_ready) ensure_dense(ix);
}

// The result buffers of a walk that keeps its own (costs, timed).
void carve_results(uint32_t nq, uint32_t cols, DevBuf<uint64_t>& cost, DevBuf<uint32_t>& hops,
                   DevBuf<uint8_t>& fin) {
    ArenaScope carve;
    const size_t m = std::max<uint32_t>(nq, 1u);
    cost.alloc(m * cols);
    hops.alloc(m);
    fin.alloc(m);
}

struct WalkRun {
    float ms = 0.f;
    uint64_t finished = 0, moves = 0, cost = 0;  // the batch's sums (wave_stats)
    bool dense = false;
    double walk_bytes = 0.0;  // walk_model_bytes, when timing is on (else 0)
};

// One walk kernel over the prepared queries, timed: launch(dense) starts the
// dense or the RLE form (not called for an empty batch); the kernel leaves
// its sums in ix->agg.  With timing on, one launch is booked under `stem` or
// `stem`_dense with walk_model_bytes + extra_bytes(moves).
template <class Launch, class ExtraBytes>
WalkRun walk_call(cpd_index* ix, const char* stem, Launch&& launch, ExtraBytes&& extra_bytes,
                  cpd_query_stats* st) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint32_t nq = ix->nq;
    WalkRun r;
    r.dense = ix->use_dense();
    HIP_CHECK(hipMemsetAsync(ix->agg.p, 0, 3 * sizeof(unsigned long long), s));
    Events<2> ev(g);
    HIP_CHECK(hipEventRecord(ev.e[0], s));
    (void)hipGetLastError();
    if (nq) launch(r.dense);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    unsigned long long hagg[3] = {0, 0, 0};  // finished, moves, cost
    HIP_CHECK(hipMemcpyAsync(hagg, ix->agg.p, sizeof hagg, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventElapsedTime(&r.ms, ev.e[0], ev.e[1]));
    r.finished = hagg[0];
    r.moves = hagg[1];
    r.cost = hagg[2];
    if (g->timing) {
        Agg& ag = g->agg[r.dense ? std::string(stem) + "_dense" : std::string(stem)];
        ag.launches++;
        ag.ms += r.ms;
        r.walk_bytes = walk_model_bytes(ix, r.dense, nq, r.moves);
        ag.bytes += r.walk_bytes + extra_bytes(r.moves);
    }
    if (st) {
        st->queries = nq;
        st->finished = r.finished;
        st->hops = r.moves;
        st->cost = r.cost;
        st->kernel_ms = r.ms;
    }
    return r;
}

// The table-search walk of the prepared queries (cpd_query_run; the count
// pass of cpd_query_paths): cost / hops / fin in sorted order, sums in agg.
// Returns the launch's algorithmic bytes when timing is on (else 0).
double run_walk(cpd_index* ix, int32_t k_moves, cpd_query_stats* st) {
    cpd_graph* g = ix->g;
    g->select();
    resolve_rows(ix);
    const uint32_t* adj = ix->walk_adj();
    auto launch = [&](bool dense) {
        if (dense)
            launch_table_search_dense(adj, g->adj_shift, ix->dense.p, g->npad, g->tlb, ix->qs.p,
                                      ix->qt.p, ix->qrow.p, ix->nq, k_moves, g->n, ix->cost.p,
                                      ix->hops.p, ix->fin.p, ix->agg.p, g->stream);
        else
            launch_table_search(adj, g->adj_shift, ix->off.p, ix->runs.p, ix->qs.p, ix->qt.p,
                                ix->qrow.p, ix->nq, k_moves, g->n, ix->cost.p, ix->hops.p,
                                ix->fin.p, ix->agg.p, g->stream);
    };
    return walk_call(ix, "table_search", launch, [](uint64_t) { return 0.0; }, st).walk_bytes;
}

// Results in sorted order -> the caller's, on the GPU, then copied out: `cols`
// u64 per query from `cost_d` (by_rows: the rows form of the scatter, which
// cpd_query_costs_fetch uses at any width), hops and fin.  qout serves the
// three in turn, the stream drained between them.
void fetch_results(cpd_index* ix, const uint64_t* cost_d, uint32_t cols, bool by_rows,
                   const uint32_t* hops_d, const uint8_t* fin_d, uint64_t* cost, uint32_t* hops,
                   uint8_t* finished) {
    cpd_graph* g = ix->g;
    g->select();
    const uint32_t nq = ix->nq;
    if (!nq) return;
    hipStream_t st = g->stream;
    ix->qout.alloc((size_t)nq * 8u * cols);
    if (cost) {
        uint64_t* out = reinterpret_cast<uint64_t*>(ix->qout.p);
        if (by_rows) launch_scatter_u64_rows(cost_d, ix->qperm.p, nq, cols, out, st);
        else launch_scatter_u64(cost_d, ix->qperm.p, nq, out, st);
        HIP_CHECK(hipMemcpyAsync(cost, ix->qout.p, (size_t)nq * 8u * cols, hipMemcpyDeviceToHost, st));
    }
    if (hops) {
        HIP_CHECK(hipStreamSynchronize(st));  // qout is reused
        launch_scatter_u32(hops_d, ix->qperm.p, nq, 1u, reinterpret_cast<uint32_t*>(ix->qout.p), st);
        HIP_CHECK(hipMemcpyAsync(hops, ix->qout.p, nq * 4ull, hipMemcpyDeviceToHost, st));
    }
    if (finished) {
        HIP_CHECK(hipStreamSynchronize(st));
        launch_scatter_u8(fin_d, ix->qperm.p, nq, ix->qout.p, st);
        HIP_CHECK(hipMemcpyAsync(finished, ix->qout.p, nq, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

extern "C" {

int cpd_query_prepare(cpd_index* ix, const uint32_t* s, const uint32_t* t, uint32_t nq) {
    return guarded([&] {
        CPD_REQUIRE(ix && (nq == 0 || (s && t)), CPD_E_ARG, "query: null argument");
        require_complete(ix, "query");
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t st = g->stream;
        // on the GPU: columns and target rows of the queries, a stable radix
        // sort by row (a wave's lanes then walk the same row), the sorted
        // columns; the caller's order comes back in cpd_query_fetch
        ix->nq = 0;
        ix->searched = false;
        ix->paths_ready = false;
        ix->costs_ready = false;
        ix->timed_ready = false;
        const size_t m = std::max<uint32_t>(nq, 1u);
        for (DevBuf<uint32_t>* b : {&ix->qin_s, &ix->qin_t, &ix->qkey, &ix->qkey2, &ix->qval,
                                    &ix->qperm, &ix->qs, &ix->qt, &ix->qrow, &ix->hops})
            b->alloc(m);
        ix->qbad.alloc(1);
        ix->cost.alloc(m);
        ix->fin.alloc(m);
        if (nq) {
            HIP_CHECK(hipMemcpyAsync(ix->qin_s.p, s, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(ix->qin_t.p, t, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemsetAsync(ix->qbad.p, 0, sizeof(uint32_t), st));
            launch_query_keys(ix->qin_s.p, ix->qin_t.p, nq, g->n, g->order_d.p, ix->d_row_of_col.p,
                              ix->qkey.p, ix->qval.p, ix->qbad.p, st);
            HIP_CHECK(hipGetLastError());
            uint32_t bad = 0;
            HIP_CHECK(hipMemcpyAsync(&bad, ix->qbad.p, sizeof bad, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (bad) {  // name the first offending query (error path only)
                for (uint32_t q = 0; q < nq; ++q) {
                    CPD_REQUIRE(s[q] < g->n && t[q] < g->n, CPD_E_ARG, "query node out of range");
                    if (ix->row_of_col[g->order[t[q]]] == CPD_INF)
                        throw Error(CPD_E_NOROW, "target " + std::to_string(t[q]) +
                                                     " has no CPD row in this index");
                }
            }
            const size_t tb = query_sort_bytes(nq);
            ix->qsort_tmp.alloc(tb);
            launch_query_sort(ix->qsort_tmp.p, ix->qsort_tmp.n, ix->qkey.p, ix->qkey2.p, ix->qval.p,
                              ix->qperm.p, nq, std::max(1u, ix->nrows), st);
            HIP_CHECK(hipGetLastError());
            launch_query_gather(ix->qin_s.p, ix->qin_t.p, g->order_d.p, ix->qkey2.p, ix->qperm.p,
                                nq, ix->qs.p, ix->qt.p, ix->qrow.p, st);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(st));
        }
        ix->nq = nq;
    });
}

int cpd_query_run(cpd_index* ix, int32_t k_moves, cpd_query_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        ix->paths_ready = false;
        run_walk(ix, k_moves, st);
    });
}

int cpd_query_paths(cpd_index* ix, int32_t k_moves, uint64_t* offsets, cpd_query_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix && offsets, CPD_E_ARG, "paths: null argument");
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t s = g->stream;
        const uint32_t nq = ix->nq;
        CPD_REQUIRE(nq < 0x7FFFFFFFu, CPD_E_RANGE, "paths: too many queries for one batch");
        ix->paths_ready = false;
        // count: the walk itself (hops, cost, fin in sorted order; agg)
        const double walk_bytes = run_walk(ix, k_moves, st);
        if (!nq) {
            paths_empty(ix, offsets);
            return;
        }
        // offsets: hops to the caller's order, + 1, exclusive sum
        if (!g->inv_d.p) g->inv_d.upload(g->inv.data(), g->n, s);
        ix->qout.alloc((size_t)nq * 8u);
        ix->plens.alloc((size_t)nq + 1u);
        ix->poff.alloc((size_t)nq + 1u);
        size_t scan_bytes = 0;
        HIP_CHECK(path_scan_bytes(nq, &scan_bytes));
        ix->qsort_tmp.alloc(scan_bytes);
        Events<3> ev(g);
        const hipEvent_t e0 = ev.e[0], e1 = ev.e[1], e2 = ev.e[2];
        HIP_CHECK(hipEventRecord(e0, s));
        uint32_t* hops_c = reinterpret_cast<uint32_t*>(ix->qout.p);
        launch_scatter_u32(ix->hops.p, ix->qperm.p, nq, 1u, hops_c, s);
        HIP_CHECK(launch_path_offsets(ix->qsort_tmp.p, ix->qsort_tmp.n, hops_c, nq, ix->plens.p,
                                      ix->poff.p, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(e1, s));
        const uint64_t total = paths_reserve(ix, "paths");
        // fill: the same walks once more, storing their nodes
        const bool dense = ix->use_dense();
        const uint32_t* adj = ix->walk_adj();
        if (dense)
            launch_table_paths_dense(adj, g->adj_shift, ix->dense.p, g->npad, g->tlb, ix->qs.p,
                                     ix->qt.p, ix->qrow.p, ix->qperm.p, ix->poff.p, g->inv_d.p, nq,
                                     k_moves, g->n, ix->pnodes.p, s);
        else
            launch_table_paths(adj, g->adj_shift, ix->off.p, ix->runs.p, ix->qs.p, ix->qt.p,
                               ix->qrow.p, ix->qperm.p, ix->poff.p, g->inv_d.p, nq, k_moves, g->n,
                               ix->pnodes.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(e2, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms_off = 0.f, ms_fill = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms_off, e0, e1));
        HIP_CHECK(hipEventElapsedTime(&ms_fill, e1, e2));
        if (g->timing) {
            // offsets: hops read twice and written once (4 B), lens and poff
            // written and read (8 B each way)
            Agg& ao = g->agg["table_paths_offsets"];
            ao.launches++;
            ao.ms += ms_off;
            ao.bytes += 44.0 * nq;
            // fill: the walk's bytes + the stored nodes + the cursors
            Agg& af = g->agg[dense ? "table_paths_dense" : "table_paths"];
            af.launches++;
            af.ms += ms_fill;
            af.bytes += walk_bytes + 4.0 * (double)total + 8.0 * nq;
        }
        paths_copy_out(ix, offsets);
    });
}

int cpd_query_paths_fetch(cpd_index* ix, uint32_t first, uint32_t count, uint32_t* nodes) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->paths_ready, CPD_E_ARG,
                    "paths fetch: no cpd_query_paths / cpd_query_search_paths on the prepared queries yet");
        CPD_REQUIRE((uint64_t)first + count <= ix->nq, CPD_E_ARG,
                    "paths fetch: queries [" + std::to_string(first) + ", " +
                        std::to_string((uint64_t)first + count) + ") past the batch's " +
                        std::to_string(ix->nq));
        const uint64_t a = ix->poff_h[first], b = ix->poff_h[(size_t)first + count];
        if (a == b) return;
        CPD_REQUIRE(nodes, CPD_E_ARG, "paths fetch: null argument");
        cpd_graph* g = ix->g;
        g->select();
        HIP_CHECK(hipMemcpyAsync(nodes, ix->pnodes.p + a, (size_t)(b - a) * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, g->stream));
        HIP_CHECK(hipStreamSynchronize(g->stream));
    });
}

int cpd_query_costs(cpd_index* ix, int32_t k_moves, uint32_t slice_moves, cpd_query_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->nsets, CPD_E_ARG, "costs: no weight sets loaded (cpd_index_set_weight_sets)");
        require_complete(ix, "costs");
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t s = g->stream;
        const uint32_t nq = ix->nq;
        const uint32_t cols = slice_moves ? 1u : ix->nsets;
        ix->costs_ready = false;
        resolve_rows(ix);
        carve_results(nq, cols, ix->cs_cost, ix->cs_hops, ix->cs_fin);
        // the route needs the adjacency's heads only: the free-flow one serves
        auto launch = [&](bool dense) {
            if (dense)
                launch_table_costs_dense(g->adj.p, g->adj_shift, ix->dense.p, g->npad, g->tlb,
                                         ix->wsets.p, ix->nsets, slice_moves, ix->qs.p, ix->qt.p,
                                         ix->qrow.p, nq, k_moves, g->n, ix->cs_cost.p,
                                         ix->cs_hops.p, ix->cs_fin.p, ix->agg.p, s);
            else
                launch_table_costs(g->adj.p, g->adj_shift, ix->off.p, ix->runs.p, ix->wsets.p,
                                   ix->nsets, slice_moves, ix->qs.p, ix->qt.p, ix->qrow.p, nq,
                                   k_moves, g->n, ix->cs_cost.p, ix->cs_hops.p, ix->cs_fin.p,
                                   ix->agg.p, s);
        };
        // a record (sliced: one word) per move + the stored columns
        auto extra = [&](uint64_t moves) {
            return (slice_moves ? 4.0 : 4.0 * ix->wset_words) * (double)moves + 8.0 * cols * nq;
        };
        walk_call(ix, "table_costs", launch, extra, st);
        ix->cs_cols = cols;
        ix->costs_ready = true;
    });
}

int cpd_query_costs_fetch(cpd_index* ix, uint64_t* costs, uint32_t* hops, uint8_t* finished) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->costs_ready, CPD_E_ARG,
                    "costs fetch: no cpd_query_costs on the prepared queries yet");
        fetch_results(ix, ix->cs_cost.p, ix->cs_cols, true, ix->cs_hops.p, ix->cs_fin.p, costs, hops,
                      finished);
    });
}

int cpd_query_loads(cpd_index* ix, int32_t k_moves, const uint32_t* demand, uint32_t nslices,
                    uint32_t slice_moves, uint32_t flags, cpd_query_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(nslices >= 1 && nslices <= CPD_MAX_LOAD_SLICES, CPD_E_ARG,
                    "loads: " + std::to_string(nslices) + " slices, 1 to " +
                        std::to_string(CPD_MAX_LOAD_SLICES));
        CPD_REQUIRE((nslices == 1) == (slice_moves == 0), CPD_E_ARG,
                    "loads: slice_moves must be 0 with one slice and non-zero with more");
        require_complete(ix, "loads");
        const bool keep = (flags & CPD_LOADS_ACCUMULATE) && ix->loads_ready;
        CPD_REQUIRE(!keep || !ix->ld_period, CPD_E_ARG,
                    "loads: accumulate into the table of a timed walk (period " +
                        std::to_string(ix->ld_period) + ")");
        CPD_REQUIRE(!keep || (ix->ld_slices == nslices && ix->ld_slice_moves == slice_moves),
                    CPD_E_ARG,
                    "loads: accumulate into a table of " + std::to_string(ix->ld_slices) +
                        " slices of " + std::to_string(ix->ld_slice_moves) + " moves asked with " +
                        std::to_string(nslices) + " of " + std::to_string(slice_moves));
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t s = g->stream;
        const uint32_t nq = ix->nq;
        require_load_slots(g, "loads");
        ix->paths_ready = false;
        resolve_rows(ix);
        if (!keep) reset_load_table(ix, nslices, slice_moves, 0);
        if (demand && nq) ix->ld_demand.upload(demand, nq, s);
        const uint32_t* dem = demand && nq ? ix->ld_demand.p : nullptr;
        const uint32_t* adj = ix->walk_adj();
        auto launch = [&](bool dense) {
            if (dense)
                launch_table_loads_dense(adj, g->adj_shift, ix->dense.p, g->npad, g->tlb, ix->qs.p,
                                         ix->qt.p, ix->qrow.p, ix->qperm.p, dem, nq, k_moves, g->n,
                                         nslices, slice_moves, ix->ld_tab.p, ix->cost.p,
                                         ix->hops.p, ix->fin.p, ix->agg.p, s);
            else
                launch_table_loads(adj, g->adj_shift, ix->off.p, ix->runs.p, ix->qs.p, ix->qt.p,
                                   ix->qrow.p, ix->qperm.p, dem, nq, k_moves, g->n, nslices,
                                   slice_moves, ix->ld_tab.p, ix->cost.p, ix->hops.p, ix->fin.p,
                                   ix->agg.p, s);
        };
        // a demand and its index per query + one 8-B counter per move
        auto extra = [&](uint64_t moves) { return (dem ? 8.0 : 0.0) * nq + 8.0 * (double)moves; };
        walk_call(ix, "table_loads", launch, extra, st);
    });
}

int cpd_query_loads_fetch(cpd_index* ix, uint64_t* loads) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->loads_ready, CPD_E_ARG,
                    "loads fetch: no cpd_query_loads on this index since it was made or cleared");
        cpd_graph* g = ix->g;
        const size_t total = (size_t)ix->ld_slices * g->m;
        if (!total) return;
        CPD_REQUIRE(loads, CPD_E_ARG, "loads fetch: null argument");
        g->select();
        hipStream_t s = g->stream;
        // slot space -> original edge order, on the GPU, then copied out once
        ix->ld_out.alloc(total);
        (void)hipGetLastError();
        launch_loads_gather(ix->ld_tab.p, g->slot_of_edge_d.p, g->m, g->n << g->adj_shift,
                            ix->ld_slices, ix->ld_out.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(loads, ix->ld_out.p, total * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int cpd_query_loads_clear(cpd_index* ix) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        ix->g->select();
        ix->ld_tab.release();
        ix->ld_out.release();
        ix->ld_slices = ix->ld_slice_moves = 0;
        ix->ld_period = 0;
        ix->loads_ready = false;
    });
}

int cpd_query_timed(cpd_index* ix, int32_t k_moves, const uint64_t* depart, uint64_t period,
                    const uint32_t* demand, uint32_t flags, cpd_query_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->nsets, CPD_E_ARG, "timed: no weight sets loaded (cpd_index_set_weight_sets)");
        require_complete(ix, "timed");
        const bool loads = (flags & CPD_TIMED_LOADS) != 0;
        CPD_REQUIRE(loads || !(flags & CPD_LOADS_ACCUMULATE), CPD_E_ARG,
                    "timed: CPD_LOADS_ACCUMULATE without CPD_TIMED_LOADS");
        CPD_REQUIRE(period >= 1 && period <= (1ull << 60), CPD_E_ARG,
                    "timed: period " + std::to_string(period) + ", 1 to 2^60");
        const uint32_t nq = ix->nq;
        if (depart)
            for (uint32_t q = 0; q < nq; ++q)
                CPD_REQUIRE(depart[q] < (1ull << 63), CPD_E_ARG,
                            "timed: departure " + std::to_string(depart[q]) + " of query " +
                                std::to_string(q) + ", must be below 2^63");
        const uint32_t nsets = ix->nsets;
        const bool keep = loads && (flags & CPD_LOADS_ACCUMULATE) && ix->loads_ready;
        CPD_REQUIRE(!keep || (ix->ld_period == period && ix->ld_slices == nsets), CPD_E_ARG,
                    "timed: accumulate into a table of " + std::to_string(ix->ld_slices) +
                        " planes of " +
                        (ix->ld_period ? "period " + std::to_string(ix->ld_period)
                                       : std::to_string(ix->ld_slice_moves) + " moves") +
                        " asked with " + std::to_string(nsets) + " sets of period " +
                        std::to_string(period));
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t s = g->stream;
        if (loads) require_load_slots(g, "timed");
        ix->timed_ready = false;
        resolve_rows(ix);
        carve_results(nq, 1u, ix->tm_cost, ix->tm_hops, ix->tm_fin);
        if (loads && !keep) reset_load_table(ix, nsets, 0, period);
        if (depart && nq) ix->tm_depart.upload(depart, nq, s);
        const uint64_t* dep = depart && nq ? ix->tm_depart.p : nullptr;
        if (loads && demand && nq) ix->ld_demand.upload(demand, nq, s);
        const uint32_t* dem = loads && demand && nq ? ix->ld_demand.p : nullptr;
        uint64_t* tab = loads ? ix->ld_tab.p : nullptr;
        // the route needs the adjacency's heads only: the free-flow one serves
        auto launch = [&](bool dense) {
            if (dense)
                launch_table_timed_dense(g->adj.p, g->adj_shift, ix->dense.p, g->npad, g->tlb,
                                         ix->wsets.p, nsets, ix->qs.p, ix->qt.p, ix->qrow.p,
                                         ix->qperm.p, dep, period, dem, nq, k_moves, g->n, tab,
                                         ix->tm_cost.p, ix->tm_hops.p, ix->tm_fin.p, ix->agg.p, s);
            else
                launch_table_timed(g->adj.p, g->adj_shift, ix->off.p, ix->runs.p, ix->wsets.p,
                                   nsets, ix->qs.p, ix->qt.p, ix->qrow.p, ix->qperm.p, dep, period,
                                   dem, nq, k_moves, g->n, tab, ix->tm_cost.p, ix->tm_hops.p,
                                   ix->tm_fin.p, ix->agg.p, s);
        };
        // a record per move (+ one 8-B counter with loads) + the permutation
        // word and what is read through it per query + the stored cost
        auto extra = [&](uint64_t moves) {
            const double per_q = (dep ? 8.0 : 0.0) + (dem ? 4.0 : 0.0);
            return (4.0 * ix->wset_words + (loads ? 8.0 : 0.0)) * (double)moves +
                   (per_q + 4.0) * nq + 8.0 * nq;
        };
        walk_call(ix, "table_timed", launch, extra, st);
        ix->timed_ready = true;
    });
}

int cpd_query_timed_fetch(cpd_index* ix, uint64_t* cost, uint32_t* hops, uint8_t* finished) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->timed_ready, CPD_E_ARG,
                    "timed fetch: no cpd_query_timed on the prepared queries yet");
        fetch_results(ix, ix->tm_cost.p, 1u, false, ix->tm_hops.p, ix->tm_fin.p, cost, hops, finished);
    });
}

int cpd_query_fetch(cpd_index* ix, uint64_t* cost, uint32_t* hops, uint8_t* finished) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        fetch_results(ix, ix->cost.p, 1u, false, ix->hops.p, ix->fin.p, cost, hops, finished);
    });
}

int cpd_query_batch(cpd_index* ix, const uint32_t* s, const uint32_t* t, uint32_t nq,
                    int32_t k_moves, uint64_t* cost, uint32_t* hops, uint8_t* finished,
                    cpd_query_stats* st) {
    int rc = cpd_query_prepare(ix, s, t, nq);
    if (rc) return rc;
    rc = cpd_query_run(ix, k_moves, st);
    if (rc) return rc;
    return cpd_query_fetch(ix, cost, hops, finished);
}

}  // extern "C"
