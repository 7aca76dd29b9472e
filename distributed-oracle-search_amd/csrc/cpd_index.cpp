// The table-search index (cpd_index): rows appended as RLE runs, move rows or
// built rows, expanded into dense tables on demand; query preparation, the
// walk, path extraction and the fetches.
#include <cmath>

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

int cpd_query_prepare(cpd_index* ix, const uint32_t* s, const uint32_t* t, uint32_t nq) {
    return guarded([&] {
        CPD_REQUIRE(ix && (nq == 0 || (s && t)), CPD_E_ARG, "query: null argument");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "query: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
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

}  // extern "C"

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

// The table-search walk of the prepared queries (cpd_query_run; the count
// pass of cpd_query_paths): cost / hops / fin in sorted order, sums in agg.
// Returns the launch's algorithmic bytes when timing is on (else 0).
double run_walk(cpd_index* ix, int32_t k_moves, cpd_query_stats* st) {
    cpd_graph* g = ix->g;
    g->select();
    const uint32_t nq = ix->nq;
    const bool dense = ix->use_dense();
    if (dense && !ix->dense_ready) ensure_dense(ix);
    HIP_CHECK(hipMemsetAsync(ix->agg.p, 0, 3 * sizeof(unsigned long long), g->stream));
    Events<2> ev(g);
    const hipEvent_t a = ev.e[0], b = ev.e[1];
    HIP_CHECK(hipEventRecord(a, g->stream));
    const uint32_t* adj = ix->custom_w ? ix->adj_sel.p : g->adj.p;
    (void)hipGetLastError();
    if (nq && dense)
        launch_table_search_dense(adj, g->adj_shift, ix->dense.p, g->npad, g->tlb, ix->qs.p,
                                  ix->qt.p, ix->qrow.p, nq, k_moves, g->n, ix->cost.p,
                                  ix->hops.p, ix->fin.p, ix->agg.p, g->stream);
    else if (nq)
        launch_table_search(adj, g->adj_shift, ix->off.p, ix->runs.p, ix->qs.p, ix->qt.p,
                            ix->qrow.p, nq, k_moves, g->n, ix->cost.p, ix->hops.p,
                            ix->fin.p, ix->agg.p, g->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(b, g->stream));
    unsigned long long hagg[3] = {0, 0, 0};  // finished, moves, cost (wave_stats)
    HIP_CHECK(hipMemcpyAsync(hagg, ix->agg.p, sizeof hagg, hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipStreamSynchronize(g->stream));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    double bytes = 0.0;
    if (g->timing) {
        Agg& ag = g->agg[dense ? "table_search_dense" : "table_search"];
        ag.launches++;
        ag.ms += ms;
        bytes = walk_model_bytes(ix, dense, nq, hagg[1]);
        ag.bytes += bytes;
    }
    if (st) {
        st->queries = nq;
        st->finished = hagg[0];
        st->hops = hagg[1];
        st->cost = hagg[2];
        st->kernel_ms = ms;
    }
    return bytes;
}

}  // namespace

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
            offsets[0] = 0;
            ix->poff_h.assign(1, 0);
            ix->paths_ready = true;
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
        ix->poff_h.resize((size_t)nq + 1u);
        HIP_CHECK(hipMemcpyAsync(ix->poff_h.data(), ix->poff.p, ((size_t)nq + 1u) * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const uint64_t total = ix->poff_h[nq];
        // fill: the same walks once more, storing their nodes
        // (from the arena when there is one: it is a bump allocator, so a
        // batch with more nodes than any before it carves a new buffer and
        // the old one's bytes stay taken until cpd_device_arena_release; a
        // batch that fits the buffer it has allocates nothing)
        try {
            ArenaScope carve;
            ix->pnodes.alloc((size_t)total);
        } catch (const Error& e) {
            (void)hipGetLastError();
            if (e.code != CPD_E_OOM) throw;
            throw Error(CPD_E_OOM, "paths: " + std::to_string(4ull * total) + " bytes of HBM for " +
                                       std::to_string(total) + " path nodes of " +
                                       std::to_string(nq) + " queries do not fit");
        }
        const bool dense = ix->use_dense();
        const uint32_t* adj = ix->custom_w ? ix->adj_sel.p : g->adj.p;
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
        std::memcpy(offsets, ix->poff_h.data(), ((size_t)nq + 1u) * sizeof(uint64_t));
        ix->paths_ready = true;
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

int cpd_query_costs(cpd_index* ix, int32_t k_moves, uint32_t slice_moves, cpd_query_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->nsets, CPD_E_ARG, "costs: no weight sets loaded (cpd_index_set_weight_sets)");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "costs: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t s = g->stream;
        const uint32_t nq = ix->nq;
        const uint32_t cols = slice_moves ? 1u : ix->nsets;
        ix->costs_ready = false;
        const bool dense = ix->use_dense();
        if (dense && !ix->dense_ready) ensure_dense(ix);
        {
            ArenaScope carve;
            const size_t m = std::max<uint32_t>(nq, 1u);
            ix->cs_cost.alloc(m * cols);
            ix->cs_hops.alloc(m);
            ix->cs_fin.alloc(m);
        }
        HIP_CHECK(hipMemsetAsync(ix->agg.p, 0, 3 * sizeof(unsigned long long), s));
        Events<2> ev(g);
        const hipEvent_t a = ev.e[0], b = ev.e[1];
        HIP_CHECK(hipEventRecord(a, s));
        (void)hipGetLastError();
        // the route needs the adjacency's heads only: the free-flow one serves
        if (nq && dense)
            launch_table_costs_dense(g->adj.p, g->adj_shift, ix->dense.p, g->npad, g->tlb,
                                     ix->wsets.p, ix->nsets, slice_moves, ix->qs.p, ix->qt.p,
                                     ix->qrow.p, nq, k_moves, g->n, ix->cs_cost.p, ix->cs_hops.p,
                                     ix->cs_fin.p, ix->agg.p, s);
        else if (nq)
            launch_table_costs(g->adj.p, g->adj_shift, ix->off.p, ix->runs.p, ix->wsets.p,
                               ix->nsets, slice_moves, ix->qs.p, ix->qt.p, ix->qrow.p, nq, k_moves,
                               g->n, ix->cs_cost.p, ix->cs_hops.p, ix->cs_fin.p, ix->agg.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(b, s));
        unsigned long long hagg[3] = {0, 0, 0};  // finished, moves, cost (wave_stats)
        HIP_CHECK(hipMemcpyAsync(hagg, ix->agg.p, sizeof hagg, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        if (g->timing) {
            // the walk's bytes + a record (sliced: one word) per move + the
            // stored columns
            Agg& ag = g->agg[dense ? "table_costs_dense" : "table_costs"];
            ag.launches++;
            ag.ms += ms;
            ag.bytes += walk_model_bytes(ix, dense, nq, hagg[1]) +
                        (slice_moves ? 4.0 : 4.0 * ix->wset_words) * (double)hagg[1] +
                        8.0 * cols * nq;
        }
        if (st) {
            st->queries = nq;
            st->finished = hagg[0];
            st->hops = hagg[1];
            st->cost = hagg[2];
            st->kernel_ms = ms;
        }
        ix->cs_cols = cols;
        ix->costs_ready = true;
    });
}

int cpd_query_costs_fetch(cpd_index* ix, uint64_t* costs, uint32_t* hops, uint8_t* finished) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->costs_ready, CPD_E_ARG,
                    "costs fetch: no cpd_query_costs on the prepared queries yet");
        cpd_graph* g = ix->g;
        g->select();
        const uint32_t nq = ix->nq, cols = ix->cs_cols;
        if (!nq) return;
        // sorted order -> the caller's, on the GPU, then copied out
        hipStream_t st = g->stream;
        ix->qout.alloc((size_t)nq * 8u * cols);
        if (costs) {
            launch_scatter_u64_rows(ix->cs_cost.p, ix->qperm.p, nq, cols,
                                    reinterpret_cast<uint64_t*>(ix->qout.p), st);
            HIP_CHECK(hipMemcpyAsync(costs, ix->qout.p, (size_t)nq * 8u * cols,
                                     hipMemcpyDeviceToHost, st));
        }
        if (hops) {
            HIP_CHECK(hipStreamSynchronize(st));  // qout is reused
            launch_scatter_u32(ix->cs_hops.p, ix->qperm.p, nq, 1u,
                               reinterpret_cast<uint32_t*>(ix->qout.p), st);
            HIP_CHECK(hipMemcpyAsync(hops, ix->qout.p, nq * 4ull, hipMemcpyDeviceToHost, st));
        }
        if (finished) {
            HIP_CHECK(hipStreamSynchronize(st));
            launch_scatter_u8(ix->cs_fin.p, ix->qperm.p, nq, ix->qout.p, st);
            HIP_CHECK(hipMemcpyAsync(finished, ix->qout.p, nq, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
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
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "loads: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
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
        const size_t stride = (size_t)1 << g->adj_shift;
        // the kernel keeps a slot as u32, 0xFFFFFFFF = none
        CPD_REQUIRE(stride * g->n < 0xFFFFFFFFull, CPD_E_RANGE, "loads: 2^32 adjacency slots or more");
        ix->paths_ready = false;
        const bool dense = ix->use_dense();
        if (dense && !ix->dense_ready) ensure_dense(ix);
        if (!keep) reset_load_table(ix, nslices, slice_moves, 0);
        if (demand && nq) ix->ld_demand.upload(demand, nq, s);
        const uint32_t* dem = demand && nq ? ix->ld_demand.p : nullptr;
        HIP_CHECK(hipMemsetAsync(ix->agg.p, 0, 3 * sizeof(unsigned long long), s));
        Events<2> ev(g);
        const hipEvent_t a = ev.e[0], b = ev.e[1];
        HIP_CHECK(hipEventRecord(a, s));
        const uint32_t* adj = ix->custom_w ? ix->adj_sel.p : g->adj.p;
        (void)hipGetLastError();
        if (nq && dense)
            launch_table_loads_dense(adj, g->adj_shift, ix->dense.p, g->npad, g->tlb, ix->qs.p,
                                     ix->qt.p, ix->qrow.p, ix->qperm.p, dem, nq, k_moves, g->n,
                                     nslices, slice_moves, ix->ld_tab.p, ix->cost.p, ix->hops.p,
                                     ix->fin.p, ix->agg.p, s);
        else if (nq)
            launch_table_loads(adj, g->adj_shift, ix->off.p, ix->runs.p, ix->qs.p, ix->qt.p,
                               ix->qrow.p, ix->qperm.p, dem, nq, k_moves, g->n, nslices,
                               slice_moves, ix->ld_tab.p, ix->cost.p, ix->hops.p, ix->fin.p,
                               ix->agg.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(b, s));
        unsigned long long hagg[3] = {0, 0, 0};  // finished, moves, cost (wave_stats)
        HIP_CHECK(hipMemcpyAsync(hagg, ix->agg.p, sizeof hagg, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        if (g->timing) {
            // the walk's bytes + a demand and its index per query + one
            // 8-B counter per move
            Agg& ag = g->agg[dense ? "table_loads_dense" : "table_loads"];
            ag.launches++;
            ag.ms += ms;
            ag.bytes += walk_model_bytes(ix, dense, nq, hagg[1]) + (dem ? 8.0 : 0.0) * nq +
                        8.0 * (double)hagg[1];
        }
        if (st) {
            st->queries = nq;
            st->finished = hagg[0];
            st->hops = hagg[1];
            st->cost = hagg[2];
            st->kernel_ms = ms;
        }
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
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "timed: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
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
        const size_t stride = (size_t)1 << g->adj_shift;
        // the kernel keeps a slot as u32, 0xFFFFFFFF = none
        CPD_REQUIRE(!loads || stride * g->n < 0xFFFFFFFFull, CPD_E_RANGE,
                    "timed: 2^32 adjacency slots or more");
        ix->timed_ready = false;
        const bool dense = ix->use_dense();
        if (dense && !ix->dense_ready) ensure_dense(ix);
        {
            ArenaScope carve;
            const size_t m = std::max<uint32_t>(nq, 1u);
            ix->tm_cost.alloc(m);
            ix->tm_hops.alloc(m);
            ix->tm_fin.alloc(m);
        }
        if (loads && !keep) reset_load_table(ix, nsets, 0, period);
        if (depart && nq) ix->tm_depart.upload(depart, nq, s);
        const uint64_t* dep = depart && nq ? ix->tm_depart.p : nullptr;
        if (loads && demand && nq) ix->ld_demand.upload(demand, nq, s);
        const uint32_t* dem = loads && demand && nq ? ix->ld_demand.p : nullptr;
        HIP_CHECK(hipMemsetAsync(ix->agg.p, 0, 3 * sizeof(unsigned long long), s));
        Events<2> ev(g);
        const hipEvent_t a = ev.e[0], b = ev.e[1];
        HIP_CHECK(hipEventRecord(a, s));
        (void)hipGetLastError();
        uint64_t* tab = loads ? ix->ld_tab.p : nullptr;
        // the route needs the adjacency's heads only: the free-flow one serves
        if (nq && dense)
            launch_table_timed_dense(g->adj.p, g->adj_shift, ix->dense.p, g->npad, g->tlb,
                                     ix->wsets.p, nsets, ix->qs.p, ix->qt.p, ix->qrow.p,
                                     ix->qperm.p, dep, period, dem, nq, k_moves, g->n, tab,
                                     ix->tm_cost.p, ix->tm_hops.p, ix->tm_fin.p, ix->agg.p, s);
        else if (nq)
            launch_table_timed(g->adj.p, g->adj_shift, ix->off.p, ix->runs.p, ix->wsets.p, nsets,
                               ix->qs.p, ix->qt.p, ix->qrow.p, ix->qperm.p, dep, period, dem, nq,
                               k_moves, g->n, tab, ix->tm_cost.p, ix->tm_hops.p, ix->tm_fin.p,
                               ix->agg.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(b, s));
        unsigned long long hagg[3] = {0, 0, 0};  // finished, moves, cost (wave_stats)
        HIP_CHECK(hipMemcpyAsync(hagg, ix->agg.p, sizeof hagg, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        if (g->timing) {
            // the walk's bytes + a record per move (+ one 8-B counter with
            // loads) + the permutation word and what is read through it per
            // query + the stored cost
            Agg& ag = g->agg[dense ? "table_timed_dense" : "table_timed"];
            ag.launches++;
            ag.ms += ms;
            const double per_q = (dep ? 8.0 : 0.0) + (dem ? 4.0 : 0.0);
            ag.bytes += walk_model_bytes(ix, dense, nq, hagg[1]) +
                        (4.0 * ix->wset_words + (loads ? 8.0 : 0.0)) * (double)hagg[1] +
                        (per_q + 4.0) * nq + 8.0 * nq;
        }
        if (st) {
            st->queries = nq;
            st->finished = hagg[0];
            st->hops = hagg[1];
            st->cost = hagg[2];
            st->kernel_ms = ms;
        }
        ix->timed_ready = true;
    });
}

int cpd_query_timed_fetch(cpd_index* ix, uint64_t* cost, uint32_t* hops, uint8_t* finished) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        CPD_REQUIRE(ix->timed_ready, CPD_E_ARG,
                    "timed fetch: no cpd_query_timed on the prepared queries yet");
        cpd_graph* g = ix->g;
        g->select();
        const uint32_t nq = ix->nq;
        if (!nq) return;
        // sorted order -> the caller's, on the GPU, then copied out
        hipStream_t st = g->stream;
        ix->qout.alloc((size_t)nq * 8u);
        if (cost) {
            launch_scatter_u64(ix->tm_cost.p, ix->qperm.p, nq,
                               reinterpret_cast<uint64_t*>(ix->qout.p), st);
            HIP_CHECK(hipMemcpyAsync(cost, ix->qout.p, nq * 8ull, hipMemcpyDeviceToHost, st));
        }
        if (hops) {
            HIP_CHECK(hipStreamSynchronize(st));  // qout is reused
            launch_scatter_u32(ix->tm_hops.p, ix->qperm.p, nq, 1u,
                               reinterpret_cast<uint32_t*>(ix->qout.p), st);
            HIP_CHECK(hipMemcpyAsync(hops, ix->qout.p, nq * 4ull, hipMemcpyDeviceToHost, st));
        }
        if (finished) {
            HIP_CHECK(hipStreamSynchronize(st));
            launch_scatter_u8(ix->tm_fin.p, ix->qperm.p, nq, ix->qout.p, st);
            HIP_CHECK(hipMemcpyAsync(finished, ix->qout.p, nq, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

int cpd_query_fetch(cpd_index* ix, uint64_t* cost, uint32_t* hops, uint8_t* finished) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        cpd_graph* g = ix->g;
        g->select();
        const uint32_t nq = ix->nq;
        if (!nq) return;
        // results come back in target-sorted order: scattered to the
        // caller's order on the GPU, then copied out
        hipStream_t st = g->stream;
        ix->qout.alloc((size_t)nq * 8u);
        if (cost) {
            launch_scatter_u64(ix->cost.p, ix->qperm.p, nq, reinterpret_cast<uint64_t*>(ix->qout.p), st);
            HIP_CHECK(hipMemcpyAsync(cost, ix->qout.p, nq * 8ull, hipMemcpyDeviceToHost, st));
        }
        if (hops) {
            HIP_CHECK(hipStreamSynchronize(st));  // qout is reused
            launch_scatter_u32(ix->hops.p, ix->qperm.p, nq, 1u, reinterpret_cast<uint32_t*>(ix->qout.p), st);
            HIP_CHECK(hipMemcpyAsync(hops, ix->qout.p, nq * 4ull, hipMemcpyDeviceToHost, st));
        }
        if (finished) {
            HIP_CHECK(hipStreamSynchronize(st));
            launch_scatter_u8(ix->fin.p, ix->qperm.p, nq, ix->qout.p, st);
            HIP_CHECK(hipMemcpyAsync(finished, ix->qout.p, nq, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
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

void cpd_index_free(cpd_index* ix) {
    if (ix && ix->g) (void)hipSetDevice(ix->device);
    delete ix;
}

}  // extern "C"
