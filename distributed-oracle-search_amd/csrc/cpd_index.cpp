// The table-search index (cpd_index): rows appended as RLE runs, move rows or
// built rows, expanded into dense tables on demand (ensure_dense); its custom
// weights and weight sets, the load table's helpers, its mode, info and end.
// The query calls on it are cpd_query.cpp's.
#include "cpd_gpu_internal.hpp"

namespace {

// Runs staged per host chunk of a streamed dense index (a row larger than
// this is staged alone).
constexpr uint64_t kStageRuns = 1ull << 28;  // 1 GiB

std::unique_ptr<cpd_index> index_init(cpd_graph* g, const uint32_t* row_targets, uint32_t nrows) {
    CPD_REQUIRE(nrows == 0 || row_targets, CPD_E_ARG, "index: null row targets");
    auto ix = std::make_unique<cpd_index>();
    ix->g = g;
    ix->device = g->device;
    ix->nrows = nrows;
    ix->row_of_col.assign(g->n, CPD_INF);
    if (nrows) ix->row_targets.assign(row_targets, row_targets + nrows);
    for (uint32_t i = 0; i < nrows; ++i) {
        CPD_REQUIRE(row_targets[i] < g->n, CPD_E_ARG, "index: row target out of range");
        ix->row_of_col[g->order[row_targets[i]]] = i;
    }
    ix->offsets.assign(1, 0);
    ix->d_row_of_col.upload(ix->row_of_col.data(), g->n, g->stream);
    ix->agg.alloc(4);
    ix->flag.alloc(1);
    return ix;
}

void index_keep_rle(cpd_index* ix, uint64_t cap) {
    ix->keep_rle = true;
    ix->stream_dense = false;
    ix->cap = cap;
    ix->runs.alloc(cap);
    ix->off.alloc((size_t)ix->nrows + 1);
    HIP_CHECK(hipMemsetAsync(ix->off.p, 0, sizeof(uint64_t), ix->g->stream));
}

void index_stream_dense(cpd_index* ix) {
    cpd_graph* g = ix->g;
    CPD_REQUIRE(g->npad / kFmTile < 65536u, CPD_E_RANGE, "graph too large for dense tables");
    ix->keep_rle = false;
    ix->stream_dense = true;
    ix->mode = CPD_INDEX_DENSE;
    {
        ArenaScope carve;  // an index's move tables (fifo_auto commits them early)
        ix->dense.alloc((size_t)ix->nrows * g->wpr());
    }
    ix->dense_ready = true;
}

// Moves an index's tables can hold: 16 (any 4-bit word) or 2^bits.
uint32_t table_move_limit(const cpd_graph* g) { return g->tlb == 2u ? 16u : 1u << (1u << g->tlb); }

// Host-side checks of a chunk's offsets (relative, offsets[0] == 0).
void check_chunk_offsets(const uint64_t* offsets, uint32_t count) {
    CPD_REQUIRE(offsets[0] == 0, CPD_E_ARG, "index: offsets[0] must be 0");
    for (uint32_t i = 0; i < count; ++i)
        CPD_REQUIRE(offsets[i + 1] > offsets[i], CPD_E_ARG, "index: empty or unsorted row");
}

// expand_rows' / validate_rows' work split for `count` rows whose host
// offsets are h_off (count + 1 values): the first run-chunk of each row,
// uploaded to ix->chunk_first; returns the number of chunks.  Every caller
// syncs the stream before the next call reuses the table.
uint32_t prepare_chunks(cpd_index* ix, const uint64_t* h_off, uint32_t count) {
    const uint64_t per = expand_chunk_runs();
    std::vector<uint32_t>& cf = ix->chunk_first_h;
    cf.assign((size_t)count + 1, 0);
    uint64_t tot = 0;
    for (uint32_t i = 0; i < count; ++i) {
        cf[i] = (uint32_t)tot;
        tot += (h_off[i + 1] - h_off[i] + per - 1) / per;
        CPD_REQUIRE(tot < (1ull << 31), CPD_E_RANGE, "index: too many runs in one append");
    }
    cf[count] = (uint32_t)tot;
    ix->chunk_first.upload(cf.data(), cf.size(), ix->g->stream);
    return (uint32_t)tot;
}

// Format check of `count` device rows (validate_rows); throws on a bad row.
// Leaves the rows' chunk table in ix->chunk_first and returns its size, for
// expand_into.
uint32_t validate_device_rows(cpd_index* ix, const uint64_t* d_off, const uint32_t* d_runs,
                              const uint64_t* h_off, uint32_t count, uint32_t mlimit = 16u) {
    cpd_graph* g = ix->g;
    const uint32_t chunks = prepare_chunks(ix, h_off, count);
    HIP_CHECK(hipMemsetAsync(ix->flag.p, 0, sizeof(uint32_t), g->stream));
    g->timed("validate_rows", 4.0 * (double)(h_off[count] - h_off[0]), [&] {
        launch_validate_rows(d_off, d_runs, ix->chunk_first.p, count, chunks, g->n, mlimit,
                             ix->flag.p, g->stream);
    });
    uint32_t bad = 0;
    HIP_CHECK(hipMemcpyAsync(&bad, ix->flag.p, sizeof bad, hipMemcpyDeviceToHost, g->stream));
    g->sync();
    CPD_REQUIRE(!bad, CPD_E_ARG,
                "index: malformed row (must start at column 0, run columns strictly increasing "
                "and < n" + std::string(mlimit < 16u ? ", moves < " + std::to_string(mlimit) +
                                                           " for this graph's move tables" : "") + ")");
    return chunks;
}

// Expand `count` rows (device offsets into d_runs; h_off = the same count + 1
// offsets on the host) into dense rows starting at index row `first`.
// chunks: the rows' chunk table is already in ix->chunk_first (what
// validate_device_rows returned), or 0 to build it here.
void expand_into(cpd_index* ix, const uint64_t* d_off, const uint32_t* d_runs,
                 const uint64_t* h_off, uint32_t count, uint64_t runs_in_chunk, uint32_t first,
                 uint32_t chunks = 0) {
    cpd_graph* g = ix->g;
    if (g->tlb != 2u) {
        // narrower tables: nibble rows into a stage (<= 256 MiB), then
        // narrowed into the index — rows checked to fit (validate_rows)
        const size_t w4 = g->npad / 8u, wpr = g->wpr();
        const uint32_t piece = (uint32_t)std::max<size_t>(1, ((size_t)1 << 26) / w4);
        ix->xstage.alloc((size_t)std::min(piece, count) * w4);
        for (uint32_t p0 = 0; p0 < count; p0 += piece) {
            const uint32_t p1 = std::min(count, p0 + piece);
            const uint32_t ch = prepare_chunks(ix, h_off + p0, p1 - p0);
            g->timed("expand_rows", 4.0 * (double)(h_off[p1] - h_off[p0]) + 4.0 * (double)w4 * (p1 - p0),
                     [&] {
                         launch_expand_rows(d_off + p0, d_runs, ix->chunk_first.p, p1 - p0, ch,
                                            g->npad, ix->xstage.p, g->stream);
                     });
            launch_repack_moves(ix->xstage.p, (uint32_t)w4, (uint32_t)w4, 4u, p1 - p0,
                                ix->dense.p + (size_t)(first + p0) * wpr, (uint32_t)wpr,
                                (uint32_t)wpr, 1u << g->tlb, g->stream);
            HIP_CHECK(hipGetLastError());
            g->sync();  // the chunk table and the stage are reused by the next piece
        }
        return;
    }
    const size_t wpr = g->npad / 8u;
    if (!chunks) chunks = prepare_chunks(ix, h_off, count);
    g->timed("expand_rows", 4.0 * (double)runs_in_chunk + 4.0 * (double)wpr * count + 16.0 * count,
             [&] {
                 launch_expand_rows(d_off, d_runs, ix->chunk_first.p, count, chunks, g->npad,
                                    ix->dense.p + first * wpr, g->stream);
             });
}

// Append `count` host rows (offsets relative, count + 1 values).
void append_host(cpd_index* ix, uint32_t count, const uint64_t* offsets, const uint32_t* runs) {
    cpd_graph* g = ix->g;
    CPD_REQUIRE(offsets, CPD_E_ARG, "index: null offsets");
    CPD_REQUIRE(count <= ix->nrows - ix->added, CPD_E_ARG, "index: more rows than declared");
    if (!count) return;
    check_chunk_offsets(offsets, count);
    const uint64_t nr = offsets[count];
    CPD_REQUIRE(runs, CPD_E_ARG, "index: null runs");
    hipStream_t s = g->stream;
    if (ix->keep_rle) {
        CPD_REQUIRE(ix->total + nr <= ix->cap, CPD_E_ARG,
                    "index: more runs than the index was created for");
        std::vector<uint64_t> o(count + 1);
        for (uint32_t i = 0; i <= count; ++i) o[i] = ix->total + offsets[i];
        HIP_CHECK(hipMemcpyAsync(ix->runs.p + ix->total, runs, nr * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ix->off.p + ix->added, o.data(), o.size() * sizeof(uint64_t),
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        validate_device_rows(ix, ix->off.p + ix->added, ix->runs.p, o.data(), count);
        ix->offsets.insert(ix->offsets.end(), o.begin() + 1, o.end());
        ix->total += nr;
        ix->added += count;
        return;
    }
    // stream_dense: stage pieces of <= kStageRuns runs (a longer row alone)
    for (uint32_t r0 = 0; r0 < count;) {
        uint32_t r1 = r0 + 1;
        while (r1 < count && offsets[r1 + 1] - offsets[r0] <= kStageRuns) ++r1;
        const uint64_t base = offsets[r0], pr = offsets[r1] - base;
        std::vector<uint64_t> o(r1 - r0 + 1);
        for (uint32_t i = r0; i <= r1; ++i) o[i - r0] = offsets[i] - base;
        ix->stage.alloc(std::max<uint64_t>(pr, std::min<uint64_t>(nr, kStageRuns)));
        ix->stage_off.alloc(std::max<size_t>(o.size(), std::min<size_t>(count + 1, 1u << 20)));
        HIP_CHECK(hipMemcpyAsync(ix->stage.p, runs + base, pr * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ix->stage_off.p, o.data(), o.size() * sizeof(uint64_t),
                                 hipMemcpyHostToDevice, s));
        const uint32_t ch = validate_device_rows(ix, ix->stage_off.p, ix->stage.p, o.data(), r1 - r0,
                                                 table_move_limit(g));
        expand_into(ix, ix->stage_off.p, ix->stage.p, o.data(), r1 - r0, pr, ix->added, ch);
        g->sync();  // the stage is reused by the next piece
        ix->added += r1 - r0;
        r0 = r1;
    }
}

// Append every row of a device-built cpd_rows (no host round trip): the
// move tables are copied as they are into a dense index, decoded into run
// words for an RLE one (and, for an index created from these rows whose
// AUTO mode resolves to dense, copied too).
void append_built(cpd_index* ix, const cpd_rows* r) {
    cpd_graph* g = ix->g;
    CPD_REQUIRE(r->device == g->device, CPD_E_ARG, "index: rows live on another device");
    r->settle();
    g->select();
    CPD_REQUIRE(r->nrows <= ix->nrows - ix->added, CPD_E_ARG, "index: more rows than declared");
    if (!r->nrows) return;
    // the built rows must be the declared rows at these positions (row i of
    // the index = row_targets[i]): a mismatch would file runs under the
    // wrong target, undetectable once a dense index has dropped them
    for (uint32_t i = 0; i < r->nrows; ++i)
        CPD_REQUIRE(r->targets[i] == ix->row_targets[ix->added + i], CPD_E_ARG,
                    "index: built row " + std::to_string(i) + " (target " +
                        std::to_string(r->targets[i]) + ") is not the declared row " +
                        std::to_string(ix->added + i));
    CPD_REQUIRE(r->n == g->n && r->wpr == (g->npad >> (5u - r->tlb)), CPD_E_ARG,
                "index: rows built for another graph");
    const size_t wpr = g->wpr();
    if (ix->dense.p && (ix->stream_dense || !ix->keep_rle || ix->dense_ready)) {
        if (r->tlb == g->tlb)
            HIP_CHECK(hipMemcpyAsync(ix->dense.p + (size_t)ix->added * wpr, r->moves.p,
                                     (size_t)r->nrows * wpr * sizeof(uint32_t),
                                     hipMemcpyDeviceToDevice, g->stream));
        else  // the rows' nibble tables narrowed to the index's width
            g->timed("repack_moves", 4.0 * ((double)r->wpr + (double)wpr) * r->nrows, [&] {
                launch_repack_moves(r->moves.p, r->wpr, r->wpr, 1u << r->tlb, r->nrows,
                                    ix->dense.p + (size_t)ix->added * wpr, (uint32_t)wpr,
                                    (uint32_t)wpr, 1u << g->tlb, g->stream);
            });
    }
    if (ix->keep_rle) {
        CPD_REQUIRE(ix->total + r->total <= ix->cap, CPD_E_ARG,
                    "index: more runs than the index was created for");
        std::vector<uint64_t> o(r->nrows + 1);
        for (uint32_t i = 0; i <= r->nrows; ++i) o[i] = ix->total + r->offsets[i];
        g->timed("moves_runs", 4.0 * (double)r->wpr * r->nrows + 4.0 * (double)r->total, [&] {
            launch_moves_runs(r->moves.p, r->wpr, r->tlb, r->n, r->nrows, r->off.p, 0,
                              ix->runs.p + ix->total, g->stream);
        });
        HIP_CHECK(hipMemcpyAsync(ix->off.p + ix->added, o.data(), o.size() * sizeof(uint64_t),
                                 hipMemcpyHostToDevice, g->stream));
        HIP_CHECK(hipStreamSynchronize(g->stream));
        ix->offsets.insert(ix->offsets.end(), o.begin() + 1, o.end());
        ix->total += r->total;
    }
    g->sync();
    ix->added += r->nrows;
}

// Append `count` host rows in the compact form (ceil(n * bits / 32) words
// each).  They are staged and, at the tables' width, copied into a dense
// index as they are (a pitched device copy to the table stride), else
// repacked — narrowing checks every move fits; an RLE index decodes them on
// the GPU, counting first.  No other format check is needed: every field is
// some move, and a move naming no out-edge of its column stops the walk
// (unfinished) like the oracle's.
void append_moves(cpd_index* ix, uint32_t count, uint32_t bits, const uint32_t* moves) {
    cpd_graph* g = ix->g;
    CPD_REQUIRE(count <= ix->nrows - ix->added, CPD_E_ARG, "index: more rows than declared");
    if (!count) return;
    CPD_REQUIRE(moves, CPD_E_ARG, "index: null move rows");
    CPD_REQUIRE(bits == 1 || bits == 2 || bits == 4, CPD_E_ARG, "index: bits per move must be 1, 2 or 4");
    const size_t w = ((uint64_t)g->n * bits + 31u) / 32u, wpr = g->wpr();
    const uint32_t tb = 1u << g->tlb;
    hipStream_t s = g->stream;
    // pieces of <= 1 GiB of tables or packed rows
    const uint32_t piece = (uint32_t)std::max<size_t>(1, ((size_t)1 << 28) / std::max(w, wpr));
    ix->lost.alloc(1);
    for (uint32_t r0 = 0; r0 < count; r0 += piece) {
        const uint32_t nr = std::min(piece, count - r0);
        uint32_t* tables = nullptr;
        if (!ix->keep_rle) {
            tables = ix->dense.p + (size_t)ix->added * wpr;
        } else {
            ix->stage.alloc((size_t)std::min(piece, count) * wpr);
            tables = ix->stage.p;
        }
        ix->pstage.alloc((size_t)std::min(piece, count) * w);
        HIP_CHECK(hipMemcpyAsync(ix->pstage.p, moves + (size_t)r0 * w, (size_t)nr * w * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, s));
        const bool narrowing = bits > tb;
        if (bits == tb) {
            HIP_CHECK(hipMemcpy2DAsync(tables, wpr * sizeof(uint32_t), ix->pstage.p,
                                       w * sizeof(uint32_t), w * sizeof(uint32_t), nr,
                                       hipMemcpyDeviceToDevice, s));
        } else {
            if (narrowing) HIP_CHECK(hipMemsetAsync(ix->lost.p, 0, sizeof(uint32_t), s));
            launch_repack_moves(ix->pstage.p, (uint32_t)w, (uint32_t)w, bits, nr, tables,
                                (uint32_t)wpr, (uint32_t)wpr, tb, s, narrowing ? ix->lost.p : nullptr);
            HIP_CHECK(hipGetLastError());
        }
        if (narrowing) {
            uint32_t lost = 0;
            HIP_CHECK(hipMemcpyAsync(&lost, ix->lost.p, sizeof lost, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            CPD_REQUIRE(!lost, CPD_E_ARG,
                        "index: a move does not fit this graph's " + std::to_string(tb) +
                            "-bit move tables (malformed rows)");
        }
        if (!ix->keep_rle) {
            HIP_CHECK(hipStreamSynchronize(s));
            ix->added += nr;
            continue;
        }
        ix->flag.alloc(std::max<size_t>(ix->flag.n, (size_t)std::min(piece, count)));
        launch_moves_count(tables, (uint32_t)wpr, g->tlb, g->n, nr, ix->flag.p, s);
        HIP_CHECK(hipGetLastError());
        std::vector<uint32_t> cnt(nr);
        HIP_CHECK(hipMemcpyAsync(cnt.data(), ix->flag.p, nr * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::vector<uint64_t> o(nr + 1);
        o[0] = ix->total;
        for (uint32_t i = 0; i < nr; ++i) o[i + 1] = o[i] + cnt[i];
        CPD_REQUIRE(o[nr] <= ix->cap, CPD_E_ARG, "index: more runs than the index was created for");
        HIP_CHECK(hipMemcpyAsync(ix->off.p + ix->added, o.data(), o.size() * sizeof(uint64_t),
                                 hipMemcpyHostToDevice, s));
        launch_moves_runs(tables, (uint32_t)wpr, g->tlb, g->n, nr, ix->off.p + ix->added, 0,
                          ix->runs.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        ix->offsets.insert(ix->offsets.end(), o.begin() + 1, o.end());
        ix->total = o[nr];
        ix->added += nr;
    }
}

}  // namespace

extern "C" {

int cpd_index_create(cpd_graph* g, const uint32_t* row_targets, uint32_t nrows,
                     const uint64_t* offsets, const uint32_t* runs, cpd_index** out) {
    return guarded([&] {
        CPD_REQUIRE(g && out && row_targets && offsets, CPD_E_ARG, "index: null argument");
        *out = nullptr;
        g->select();
        auto ix = index_init(g, row_targets, nrows);
        ix->declared = offsets[nrows];
        index_keep_rle(ix.get(), ix->declared);
        append_host(ix.get(), nrows, offsets, runs);
        *out = ix.release();
    });
}

int cpd_index_from_rows(cpd_graph* g, const cpd_rows* r, cpd_index** out) {
    return guarded([&] {
        CPD_REQUIRE(g && r && out, CPD_E_ARG, "index: null argument");
        *out = nullptr;
        g->select();
        r->settle();
        g->select();
        auto ix = index_init(g, r->targets.data(), r->nrows);
        ix->declared = r->total;
        index_keep_rle(ix.get(), r->total);
        if (ix->use_dense()) {  // AUTO resolves dense: the rows' tables, copied
            CPD_REQUIRE(g->npad / kFmTile < 65536u, CPD_E_RANGE, "graph too large for dense tables");
            {
                ArenaScope carve;  // an index's move tables
                ix->dense.alloc((size_t)ix->nrows * g->wpr());
            }
            ix->dense_ready = true;
        }
        append_built(ix.get(), r);
        *out = ix.release();
    });
}

int cpd_index_create_empty(cpd_graph* g, const uint32_t* row_targets, uint32_t nrows, int mode,
                           uint64_t total_runs, cpd_index** out) {
    return guarded([&] {
        CPD_REQUIRE(g && out, CPD_E_ARG, "index: null argument");
        CPD_REQUIRE(mode == CPD_INDEX_AUTO || mode == CPD_INDEX_RLE || mode == CPD_INDEX_DENSE,
                    CPD_E_ARG, "index mode must be CPD_INDEX_AUTO, _RLE or _DENSE");
        *out = nullptr;
        g->select();
        auto ix = index_init(g, row_targets, nrows);
        ix->declared = total_runs;
        ix->mode = mode;
        if (ix->use_dense()) index_stream_dense(ix.get());
        else index_keep_rle(ix.get(), total_runs);
        HIP_CHECK(hipStreamSynchronize(g->stream));
        *out = ix.release();
    });
}

int cpd_index_append_rows(cpd_index* ix, uint32_t count, const uint64_t* offsets,
                          const uint32_t* runs) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "index: null argument");
        ix->g->select();
        append_host(ix, count, offsets, runs);
    });
}

int cpd_index_append_moves(cpd_index* ix, uint32_t count, uint32_t bits, const uint32_t* moves) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "index: null argument");
        ix->g->select();
        append_moves(ix, count, bits, moves);
    });
}

int cpd_index_append_built_rows(cpd_index* ix, const cpd_rows* r) {
    return guarded([&] {
        CPD_REQUIRE(ix && r, CPD_E_ARG, "index: null argument");
        ix->g->select();
        append_built(ix, r);
    });
}

int cpd_index_info(const cpd_index* ix, uint32_t* nrows, uint32_t* added, uint64_t* runs_resident,
                   uint64_t* dense_bytes) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "index: null argument");
        if (nrows) *nrows = ix->nrows;
        if (added) *added = ix->added;
        if (runs_resident) *runs_resident = ix->keep_rle ? ix->total : 0;
        if (dense_bytes) *dense_bytes = ix->dense_ready ? ix->dense.n * sizeof(uint32_t) : 0;
    });
}

int cpd_index_set_weights(cpd_index* ix, const uint32_t* w) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        cpd_graph* g = ix->g;
        g->select();
        if (!w) {
            if (ix->custom_w) ix->c_ready = false;
            ix->custom_w = false;
            return;
        }
        std::vector<uint32_t> wc(g->m);
        for (uint32_t e = 0; e < g->m; ++e) wc[e] = w[g->edge_perm[e]];
        std::vector<uint32_t> adj = g->packed_adjacency(wc);
        ix->adj_sel.upload(adj.data(), adj.size(), g->stream);
        HIP_CHECK(hipStreamSynchronize(g->stream));
        ix->custom_w = true;
        ix->c_ready = false;  // the search's incumbent tables follow the weights
    });
}

}  // extern "C"

// The load table's fetch order (edge loads, timed walks; at first use):
// column-space edge ec of column c sits in slot c * stride + its place in c's
// out-list; edge_perm names its file edge.
void cpd::ensure_slot_of_edge(cpd_graph* g) {
    if (g->slot_of_edge_d.p) return;
    const size_t stride = (size_t)1 << g->adj_shift;
    std::vector<uint32_t> soe(g->m);
    for (uint32_t c = 0; c < g->n; ++c)
        for (uint32_t e = g->rowc_host[c]; e < g->rowc_host[c + 1]; ++e)
            soe[g->edge_perm[e]] = (uint32_t)(c * stride + (e - g->rowc_host[c]));
    g->slot_of_edge_d.upload(soe.data(), soe.size(), g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));  // soe leaves scope
}

// The resident load table made again: `planes` zeroed planes of the kind given
// (slice_moves and period as cpd_index keeps them), from the arena when one is
// committed.
void cpd::reset_load_table(cpd_index* ix, uint32_t planes, uint32_t slice_moves, uint64_t period) {
    cpd_graph* g = ix->g;
    const uint32_t nslots = g->n << g->adj_shift;
    ensure_slot_of_edge(g);
    ix->loads_ready = false;
    {
        ArenaScope carve;
        ix->ld_tab.alloc((size_t)planes * nslots);
    }
    HIP_CHECK(hipMemsetAsync(ix->ld_tab.p, 0, (size_t)planes * nslots * sizeof(uint64_t), g->stream));
    ix->ld_slices = planes;
    ix->ld_slice_moves = slice_moves;
    ix->ld_period = period;
    ix->loads_ready = true;
}

// Expand the resident RLE rows into dense move tables (once per index).
void cpd::ensure_dense(cpd_index* ix) {
    cpd_graph* g = ix->g;
    CPD_REQUIRE(g->npad / kFmTile < 65536u, CPD_E_RANGE, "graph too large for dense tables");
    {
        ArenaScope carve;  // an index's move tables (fifo_auto commits them early)
        ix->dense.alloc((size_t)ix->nrows * g->wpr());
    }
    if (ix->nrows && g->tlb != 2u)  // the runs' moves must fit the narrower tables
        validate_device_rows(ix, ix->off.p, ix->runs.p, ix->offsets.data(), ix->nrows,
                             table_move_limit(g));
    if (ix->nrows)
        expand_into(ix, ix->off.p, ix->runs.p, ix->offsets.data(), ix->nrows, ix->total, 0);
    g->sync();
    ix->dense_ready = true;
}

extern "C" {

int cpd_index_set_mode(cpd_index* ix, int mode) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(mode == CPD_INDEX_AUTO || mode == CPD_INDEX_RLE || mode == CPD_INDEX_DENSE,
                    CPD_E_ARG, "index mode must be CPD_INDEX_AUTO, _RLE or _DENSE");
        CPD_REQUIRE(!(ix->stream_dense && mode == CPD_INDEX_RLE), CPD_E_ARG,
                    "index was streamed into dense tables: its runs were not kept");
        if (!ix->stream_dense) ix->mode = mode;
    });
}

int cpd_index_get_mode(const cpd_index* ix, int* mode) {
    return guarded([&] {
        CPD_REQUIRE(ix && mode, CPD_E_ARG, "null argument");
        *mode = ix->use_dense() ? CPD_INDEX_DENSE : CPD_INDEX_RLE;
    });
}

int cpd_index_set_weight_sets(cpd_index* ix, uint32_t nsets, const uint32_t* const* w) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(nsets <= CPD_MAX_WEIGHT_SETS, CPD_E_ARG,
                    "weight sets: " + std::to_string(nsets) + " sets, at most " +
                        std::to_string(CPD_MAX_WEIGHT_SETS));
        CPD_REQUIRE(nsets == 0 || w, CPD_E_ARG, "weight sets: null argument");
        cpd_graph* g = ix->g;
        g->select();
        if (!nsets) {
            ix->wsets.release();
            ix->nsets = ix->wset_words = 0;
            return;
        }
        // one record per adjacency slot, as packed_adjacency lays the slots
        // out: word j = the slot's weight in set j, zeros past nsets and
        // past the out-degree; one more record of zeros closes the table
        // (what a lane that takes no move loads)
        const uint32_t kw = weight_set_words(nsets);
        const size_t stride = (size_t)1 << g->adj_shift;
        // the kernel takes the zero record's index as u32
        CPD_REQUIRE(stride * g->n < (1ull << 32), CPD_E_RANGE,
                    "weight sets: more than 2^32 adjacency slots");
        std::vector<uint32_t> tab((stride * g->n + 1u) * kw, 0u);
        for (uint32_t j = 0; j < nsets; ++j) {
            const uint32_t* wj = w[j];  // NULL: free flow
            for (uint32_t c = 0; c < g->n; ++c)
                for (uint32_t e = g->rowc_host[c]; e < g->rowc_host[c + 1]; ++e)
                    tab[((size_t)c * stride + (e - g->rowc_host[c])) * kw + j] =
                        wj ? wj[g->edge_perm[e]] : g->w_free_col[e];
        }
        ix->nsets = ix->wset_words = 0;  // none loaded should the upload fail
        {
            ArenaScope carve;
            ix->wsets.upload(tab.data(), tab.size(), g->stream);
        }
        HIP_CHECK(hipStreamSynchronize(g->stream));
        ix->nsets = nsets;
        ix->wset_words = kw;
    });
}

void cpd_index_free(cpd_index* ix) {
    if (ix && ix->g) (void)hipSetDevice(ix->device);
    delete ix;
}

}  // extern "C"
