// The row build: a batch's up-sweep, down-sweep, first moves and move-table
// emit (build_batch), the built rows (cpd_rows) and their export.
#include "cpd_gpu_internal.hpp"

void cpd_rows::settle() const {
    std::lock_guard<std::mutex> l(settle_mu);
    HIP_CHECK(hipSetDevice(device));
    wait();
    for (auto& b : retired) spare.push_back(std::move(b));
    retired.clear();
    if (pending.empty()) return;
    for (auto& b : pending) {
        for (uint32_t i = 0; i < b->k; ++i)
            offsets.push_back(offsets.back() + b->counts.p[b->pos_of[i]]);
        spare.push_back(std::move(b));
    }
    pending.clear();
    total = offsets.back();
    hipStream_t st = thread_stream(device);
    off.upload(offsets.data(), offsets.size(), st);
    HIP_CHECK(hipStreamSynchronize(st));
}

cpd_rows::Batch* cpd_rows::new_batch(uint32_t B) {
    for (size_t i = 0; i < retired.size();) {  // recycle what the device is done with
        if (hipEventQuery(retired[i]->ev) == hipSuccess) {
            spare.push_back(std::move(retired[i]));
            retired.erase(retired.begin() + (long)i);
        } else {
            ++i;
        }
    }
    std::unique_ptr<Batch> b;
    if (!spare.empty()) {
        b = std::move(spare.back());
        spare.pop_back();
    } else {
        b = std::make_unique<Batch>();
    }
    b->lane_rows.alloc(B);
    b->counts.alloc(B);
    if (!b->ev) HIP_CHECK(hipEventCreateWithFlags(&b->ev, hipEventDisableTiming));
    pending.push_back(std::move(b));
    return pending.back().get();
}

// Fold the late bytes of all but the newest `keep` batches: their stats
// (stat_h of their slot) have landed — the caller has seen a later point of
// the main stream (the next batch's down-sweep end, or a full sync).
void cpd::fold_late(cpd_graph* g, size_t keep) {
    while (g->late_q.size() > keep) {
        const auto& rec = g->late_q.front();
        const unsigned int* sh = g->bs[rec.slot].stat_h.p;
        double up = 0.0, down = 0.0;
        for (const auto& u : rec.up) {
            const size_t l = (size_t)u[0];
            up += 4096.0 * ((double)sh[2 * l] + (double)sh[2 * l + 1]) + 12.0 * u[1] + 20.0 * u[2];
        }
        for (const auto& d : rec.down) down += 4096.0 * (double)sh[(size_t)d[0]] + d[1];
        g->agg["sweep_up"].bytes += up;
        g->agg["sweep_down"].bytes += down;
        g->late_q.erase(g->late_q.begin());
    }
}

namespace {

// Runs decoded per export piece (a longer row alone): 256 MB of staging.
constexpr uint64_t kDecodeRuns = 64ull << 20;

// After a full narrow batch (g->ovf_h = its wide group rows): switch narrow
// rows off for good when most group rows had to be kept wide — the dense
// final rows replace the narrow rows and the pool (nothing may still read
// them: the caller has synchronised the main stream).  True if switched.
bool narrow_decide(cpd_graph* g) {
    const uint64_t groups = (uint64_t)g->n * (g->B / 256u);
    if (2ull * g->ovf_h() <= groups) return false;
    g->narrow = false;
    g->narrow_probe = 0;
    g->alloc_final_rows();
    if (switches().trace)
        std::fprintf(stderr, "[cpd] narrow rows off: %u of %llu group rows wide\n", g->ovf_h(),
                     (unsigned long long)groups);
    return true;
}

// Phase U of a batch of k targets (slot's columns already uploaded), on
// stream st: the target mask, the leaf-form init of the chunked levels and the
// up-sweep levels, into the slot's up store, live and target masks — which
// only this slot's down-sweep reads: the caller orders st after the slot's
// previous batch (its first moves, ev_fm[slot]).
void launch_up(cpd_graph* g, uint32_t k, uint32_t slot, hipStream_t st) {
    const uint32_t B = g->B;
    auto& S = g->bs[slot];
    const uint32_t slabs = (k + 1023u) / 1024u;  // active 1024-target slabs
    const uint32_t active = slabs * 1024u;
    uint32_t* up = g->upx[slot].p;
    uint32_t* tmask = g->tmaskx[slot].p;
    uint32_t* live = switches().live ? g->livex[slot].p : nullptr;
    unsigned int* stat = g->timing ? S.stat.p : nullptr;
    const size_t nasc = g->asc_lvl.size();
    S.up_late.clear();
    if (stat) HIP_CHECK(hipMemsetAsync(stat, 0, S.stat.n * sizeof(unsigned int), st));
    if (live) {
        HIP_CHECK(hipMemsetAsync(tmask, 0, (size_t)g->n * sizeof(uint32_t), st));
        launch_target_mask(S.tgt.p, active, tmask, st);
        g->timed("sweep_up_init", 4.0 * g->n_init_slots * active, [&] {
            launch_sweep_up_init(g->up_init_slots.p, g->n_init_slots, g->asc_nodes.p, up, g->ubase,
                                 S.tgt.p, B, slabs, live, tmask, st);
        });
    }
    // ascending sweep: each level reads lower levels' rows.  Levels 0 and 1
    // are never materialised (closed forms, kLeafBit / kL1Bit): not launched.
    // Dense bytes per level: gathered rows 4 B x target, row writes 4 B x
    // target, arcs 8 B and node slot 12 B per 1024-target slab.  Sparse: 4 KiB
    // per live (row, slab) stored and per live row gathered, arcs 8 B + their
    // masks 4 B, node slot 12 B + masks 8 B, once per node — known once the
    // batch's live_stats have run (added by build_batch from S.up_late).
    g->group_begin("sweep_up", st);
    // bytes of level l (0 when they wait for the batch's stats)
    auto level_bytes = [&](size_t l) {
        const uint32_t s0 = g->asc_lvl[l], cnt = g->asc_lvl[l + 1] - s0;
        const double arcs_l = (double)(g->asc_off_host[g->asc_lvl[l + 1]] - g->asc_off_host[s0]);
        if (live && stat) {
            S.up_late.push_back({(double)l, arcs_l, (double)cnt});
            return 0.0;
        }
        return (4.0 * g->asc_lvl_arcs[l] + 4.0 * cnt) * active + 8.0 * arcs_l * slabs +
               12.0 * cnt * slabs;
    };
    auto items_of = [&](size_t l) { return g->up_item_first[l + 1] - g->up_item_first[l]; };
    for (size_t l = 2; l + 1 < nasc; ++l) {
        uint32_t s0 = g->asc_lvl[l], cnt = g->asc_lvl[l + 1] - s0;
        if (!cnt) continue;
        const uint32_t i0 = g->up_item_first[l], ni = items_of(l);
        const double dense = level_bytes(l);
        g->timed("sweep_up", dense, [&] {
            if (live && ni)
                launch_sweep_up_chunks(g->up_items.p + 4 * (size_t)i0, ni, g->asc_arcs.p, up,
                                       g->ubase, S.tgt.p, B, slabs, g->asc_nodes.p,
                                       g->asc_off.p, g->asc_arcs.p, live, tmask, st);
            else
                launch_sweep(true, g->asc_nodes.p, g->asc_off.p, g->asc_arcs.p, s0, cnt, nullptr,
                             up, g->ubase, nullptr, S.tgt.p, B, slabs, g->asc_nodes.p,
                             g->asc_off.p, g->asc_arcs.p, live, tmask, g->adj.p, g->adj_shift,
                             nullptr, g->narrow_rows(false), nullptr, st);
        });
    }
    g->group_end();
}

// Phase D of the batch in `slot` (its up-sweep done or ordered before), on
// g->stream: the down-sweep (own rows from the slot's up store), the pool
// rows it took (narrow; the count lands in g->ovf_h), the live stats
// (timing runs), then ev_down.
void launch_down(cpd_graph* g, uint32_t k, bool narrow, uint32_t slot) {
    const uint32_t B = g->B, n = g->n;
    auto& S = g->bs[slot];
    const NarrowRows nr = g->narrow_rows(narrow);
    if (narrow) HIP_CHECK(hipMemsetAsync(g->ovf.p, 0, sizeof(uint32_t), g->stream));
    // bytes per target of a final-distance row access: 4 wide; 2 + a 4-B base
    // per 256 targets narrow
    const double drow = narrow ? 2.0 + 4.0 / 256.0 : 4.0;
    const uint32_t slabs = (k + 1023u) / 1024u;  // active 1024-target slabs
    const uint32_t active = slabs * 1024u;
    uint32_t* live = switches().live ? g->livex[slot].p : nullptr;
    unsigned int* stat = g->timing ? S.stat.p : nullptr;
    const size_t nasc = g->asc_lvl.size();
    cpd_graph::LateRec rec;
    rec.slot = slot;
    rec.up.swap(S.up_late);  // this batch's up levels (launch_up)
    g->group_begin("sweep_down", g->stream);
    for (size_t l = 0; l + 1 < g->dsc_lvl.size(); ++l) {
        uint32_t s0 = g->dsc_lvl[l], cnt = g->dsc_lvl[l + 1] - s0;
        if (!cnt) continue;
        const size_t si = 2 * (nasc + l);
        double base = (drow * g->dsc_lvl_arcs[l] + drow * cnt) * active +
                      8.0 * g->dsc_lvl_arcs[l] * slabs + 12.0 * cnt * slabs;
        if (g->leaf_fm) base += 0.5 * g->dsc_lvl_leaves[l] * active;  // leaf sets
        double dense = base + 4.0 * g->dsc_lvl_reads[l] * active;
        if (live && stat) {  // own rows: 4 KiB per live (row, slab), counted by live_stats
            rec.down.push_back({(double)si, 4.0 * g->dsc_lvl_reads[l] * slabs});
            dense = base;
        }
        g->timed("sweep_down", dense, [&] {
            launch_sweep(false, g->dsc_nodes.p, g->dsc_off.p, g->dsc_arcs.p, s0, cnt, g->dist.p,
                         g->upx[slot].p, g->ubase, g->dsc_up.p, S.tgt.p, B, slabs, g->asc_nodes.p,
                         g->asc_off.p, g->asc_arcs.p, live, g->tmaskx[slot].p, g->adj.p,
                         g->adj_shift, g->leaf_fm ? g->fmleaf.p : nullptr, nr, g->dsc_desc.p,
                         g->stream);
        });
    }
    g->group_end();
    if (stat) g->late_q.push_back(std::move(rec));
    if (narrow)
        HIP_CHECK(hipMemcpyAsync(g->ovf_hb.p, g->ovf.p, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                 g->stream));
    if (live && stat && nasc > 2) {  // row counts behind the late byte counts
        g->timed("live_stats", 0.0, [&] {
            launch_live_stats(true, g->asc_nodes.p, g->asc_off.p, g->asc_arcs.p,
                              g->asc_lvl_of.p, g->asc_lvl[2], n, g->ubase, g->dsc_up.p, live,
                              stat, g->stream);
        });
        g->timed("live_stats", 0.0, [&] {
            launch_live_stats(false, g->dsc_nodes.p, g->dsc_off.p, g->dsc_arcs.p,
                              g->dsc_lvl_of.p, 0, n, g->ubase, g->dsc_up.p, live,
                              stat + 2 * nasc, g->stream);
        });
    }
    // the slot is free for the batch after next once these land: its targets
    // copied for the first moves, the stats copied out
    HIP_CHECK(hipMemcpyAsync(g->fm_tgt.p, S.tgt.p, (size_t)B * sizeof(uint32_t),
                             hipMemcpyDeviceToDevice, g->stream));
    if (stat)
        HIP_CHECK(hipMemcpyAsync(S.stat_h.p, stat, S.stat.n * sizeof(unsigned int),
                                 hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipEventRecord(g->ev_down, g->stream));
}

// Phase F: the first moves of the batch in `slot` into fm (after its
// down-sweep on g->stream), then ev_fm[slot]; the timing stats' copy.
void launch_fm(cpd_graph* g, uint32_t k, bool narrow, uint32_t* fm, uint32_t slot) {
    const uint32_t B = g->B, n = g->n;
    const NarrowRows nr = g->narrow_rows(narrow);
    const double drow = narrow ? 2.0 + 4.0 / 256.0 : 4.0;
    // per row: own distance 4n (kernels that read it) + neighbour distances
    // 4m + first-move write npad * fmb / 8; the packed adjacency (8 B per
    // slot) is read once per 1024-target slab.  Leaf columns (leaf_fm) read
    // 0.5 B of sets instead of their own and neighbour distances.
    const uint32_t fslabs = (k + 1023u) / 1024u;
    const double nl = g->leaf_fm ? g->n_leaf : 0.0, ml = g->leaf_fm ? g->m_leaf : 0.0;
    const double own = first_moves_reads_own(g->adj_shift, narrow) ? drow * (n - nl) : 0.0;
    double fbytes =
        (own + drow * (g->m - ml) + 0.5 * nl + g->fmb / 8.0 * g->npad) *
            (fslabs * 1024.0) +
        8.0 * (double)(n - nl) * (double)(1u << g->adj_shift) * fslabs + 4.0 * g->npad / 32.0;
    g->timed("first_moves", fbytes, [&] {
        launch_first_moves(g->adj.p, g->adj_shift, g->dist.p, g->fm_tgt.p, B, k, n, g->npad,
                           fm, g->leaf_fm ? g->leafbits.p : nullptr,
                           g->leaf_fm ? g->fmleaf.p : nullptr, nr, g->stream, g->seg_order.p);
    });
    HIP_CHECK(hipEventRecord(g->ev_fm[slot], g->stream));
}

void launch_down_fm(cpd_graph* g, uint32_t k, bool narrow, uint32_t* fm, uint32_t slot) {
    launch_down(g, k, narrow, slot);
    launch_fm(g, k, narrow, fm, slot);
}

// Upload a batch's targets as columns into `slot`, on stream st.  With
// sorting on, lanes hold the targets in column order (DFS preorder is
// spatially coherent, so a 1024-lane slab covers one compact region and the
// up-sweep skips most rows); pos_of[i] = lane of the caller's target i.
// The batch's lane order and columns into the slot's host buffers (host
// work only; upload_targets copies them to the device).
void prepare_targets(cpd_graph* g, const uint32_t* targets, uint32_t k, uint32_t slot) {
    auto& S = g->bs[slot];
    CPD_REQUIRE(g->has_ch, CPD_E_ARG,
                "graph was created from a plan without hierarchy: it can serve queries "
                "but not build rows");
    std::vector<uint32_t> cols(g->B), idx(k);
    for (uint32_t i = 0; i < k; ++i) {
        CPD_REQUIRE(targets[i] < g->n, CPD_E_ARG,
                    "target " + std::to_string(targets[i]) + " out of range");
        idx[i] = i;
    }
    if (switches().sort && k > 0) {
        // lanes by (Hilbert key, column), or by column without coordinates:
        // compact 2-D groups — a 256-lane group spans a small square, so its
        // final distances fit the narrow rows' 16-bit offsets (column order:
        // 5.5% of group rows wide on the 1M-node bench batch).
        // A stable LSD radix sort of the 64-bit keys (a comparison sort of a
        // 16k batch took ~1.7 ms of host time between two batches' kernels).
        const bool hk = !g->lane_key.empty() && switches().lane_key;
        std::vector<uint64_t> kv(k), kt(k);
        std::vector<uint32_t> it(k);
        for (uint32_t i = 0; i < k; ++i)
            kv[i] = ((hk ? (uint64_t)g->lane_key[targets[i]] : 0ull) << 32) |
                    g->order[targets[i]];
        for (int pass = 0; pass < (hk ? 8 : 4); ++pass) {
            const int sh = 8 * pass;
            uint32_t cnt[257] = {0};
            for (uint32_t i = 0; i < k; ++i) ++cnt[((kv[i] >> sh) & 0xFFu) + 1];
            if (cnt[((kv[0] >> sh) & 0xFFu) + 1] == k) continue;  // one digit value: no-op
            for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
            for (uint32_t i = 0; i < k; ++i) {
                const uint32_t pos = cnt[(kv[i] >> sh) & 0xFFu]++;
                kt[pos] = kv[i];
                it[pos] = idx[i];
            }
            kv.swap(kt);
            idx.swap(it);
        }
    }
    S.pos_of.resize(k);
    for (uint32_t p = 0; p < k; ++p) {
        cols[p] = g->order[targets[idx[p]]];
        S.pos_of[idx[p]] = p;
    }
    for (uint32_t i = k; i < g->B; ++i) cols[i] = cols[0];  // padding lanes
    S.tgt_col = cols;
    std::copy(cols.begin(), cols.end(), S.tgt_h.p);
}

void upload_targets(cpd_graph* g, const uint32_t* targets, uint32_t k, uint32_t slot,
                    hipStream_t st, bool prepared = false) {
    if (!prepared) prepare_targets(g, targets, k, slot);
    auto& S = g->bs[slot];
    HIP_CHECK(hipMemcpyAsync(S.tgt.p, S.tgt_h.p, (size_t)g->B * sizeof(uint32_t),
                             hipMemcpyHostToDevice, st));
}

void build_batch(cpd_graph* g, const uint32_t* targets, uint32_t k, cpd_rows* r,
                 const uint32_t* next, uint32_t next_k);

// The batch's slot, its up-sweep done or queued before g->stream's next work:
// the one the previous batch launched for these targets, else one launched here.
uint32_t take_slot(cpd_graph* g, const uint32_t* targets, uint32_t k) {
    uint32_t slot;
    if (g->prepped && g->prep_targets.size() == k &&
        std::equal(targets, targets + k, g->prep_targets.begin())) {
        slot = g->prep_slot;  // up-sweep launched by the previous batch
        HIP_CHECK(hipStreamWaitEvent(g->stream, g->ev_up, 0));
        g->prepped = false;
    } else {
        if (g->prepped) g->drop_prep();
        slot = g->next_slot;
        upload_targets(g, targets, k, slot, g->stream);
        launch_up(g, k, slot, g->stream);
    }
    g->next_slot = slot ^ 1u;
    return slot;
}

// The next batch's up-sweep (ustream, high priority) into the other slot,
// after that slot's last batch's down-sweep (the last reader of the
// slot's targets, up store, masks and stats; its first moves read the
// targets from fm_tgt).  The host queues it as soon as this batch starts:
// it runs beside the previous batch's first moves, ahead of this
// down-sweep, which the host's launch latency then never delays.
void queue_next_up(cpd_graph* g, uint32_t ns, const uint32_t* next, uint32_t next_k) {
    if (!(next && next_k && switches().overlap)) return;
    prepare_targets(g, next, next_k, ns);
    // after the other slot's last batch: its down-sweep (ev_down, not yet
    // re-recorded for this batch), so this up-sweep runs beside its first
    // moves (after them, ev_fm[ns], it ran beside this down-sweep: with
    // the one-row emit the same rows/s within noise, 371.9-376.9k against
    // 374.6-377.1k, profiles/up_store_ab/r06k_*; with the eight-row emit
    // 414.2-415.1k against 413.2-423.4k, the down-sweep's launches 12%
    // longer, r06o_*; with first_moves at 8 waves per SIMD 419.0-420.5k
    // against 425.2-431.7k, r06z_*)
    HIP_CHECK(hipStreamWaitEvent(g->ustream, g->ev_down, 0));
    upload_targets(g, next, next_k, ns, g->ustream, true);
    launch_up(g, next_k, ns, g->ustream);
    HIP_CHECK(hipEventRecord(g->ev_up, g->ustream));
    g->prepped = true;
    g->prep_slot = ns;
    g->prep_targets.assign(next, next + next_k);
}

// Narrow rows: the pool rows the down-sweep took (wide group rows).  Past
// the pool the batch must be rebuilt (returns true); the first full batches
// decide whether narrow rows pay at all (narrow_decide).
// (The host waits for this down-sweep in any case: the next batch's
// target staging buffers are then free.)
bool narrow_check(cpd_graph* g, uint32_t k, bool narrow) {
    HIP_CHECK(hipEventSynchronize(g->ev_down));  // g->ovf_h has landed
    if (!narrow) return false;
    const uint64_t groups = (uint64_t)g->n * (g->B / 256u);
    if (g->timing) {  // group rows kept wide / all group rows
        g->agg["wide_rows"].launches += g->ovf_h();
        g->agg["group_rows"].launches += groups;
    }
    // emit_sets is recorded only for narrow batches
    if (g->timing) g->agg["emit_sets"].launches = g->nsets;  // the emit overlap's depth
    const bool rebuild = g->ovf_h() > g->pool_cap;
    if (g->narrow_probe && k == g->B) {
        --g->narrow_probe;
        if (2ull * g->ovf_h() > groups) {
            HIP_CHECK(hipStreamSynchronize(g->stream));  // nothing reads the narrow rows
            narrow_decide(g);
        }
    }
    return rebuild;
}

// This batch's rows are not emitted: they are built again, with the
// dense rows when narrow rows were just switched off, else in pieces
// of pool_cap / (4 n) slabs, whose group rows all fit the pool.
void rebuild_in_pieces(cpd_graph* g, const uint32_t* targets, uint32_t k, cpd_rows* r,
                       const uint32_t* next, uint32_t next_k) {
    HIP_CHECK(hipStreamSynchronize(g->stream));
    g->drop_prep();
    if (g->timing) g->agg["pool_rebuilds"].launches += 1;
    if (switches().trace)
        std::fprintf(stderr, "[cpd] batch of %u rows: %u wide group rows past the pool's %u, rebuilt\n",
                     k, g->ovf_h(), g->pool_cap);
    const uint32_t piece =
        g->narrow ? std::min(g->B, std::max(1024u, (uint32_t)(g->pool_cap / (4ull * g->n)) * 1024u))
                  : g->B;
    for (uint32_t b = 0; b < k; b += piece) {
        const uint32_t kk = std::min(piece, k - b);
        const bool last = b + kk >= k;
        build_batch(g, targets + b, kk, r, last ? next : targets + b + kk,
                    last ? next_k : std::min(piece, k - b - kk));
    }
}

// One batch's emit: k rows from buffer set x of g (fm: the first-move sets;
// rst / rrc: the RLE segment states) into r's tables and the batch record rb,
// on stream es.  fm_row: first-move bytes per row; st_row: + per 32-column
// segment a 4-B entry state and a 1-B count (fmb == 4).
struct Emit {
    cpd_graph* g;
    cpd_rows* r;
    cpd_rows::Batch* rb;
    uint32_t k, x;
    hipStream_t es;
    uint32_t *fm, *rst;
    uint8_t* rrc;
    double fm_row, st_row;
};

// one pass: each set read once, the tables written, the run counts
// summed from the chunks (rle_emit8 + the seam check rle_emit_fix)
void emit_fused(const Emit& e) {
    cpd_graph* g = e.g;
    const uint32_t k = e.k, npad = g->npad;
    const uint32_t ec = rle_emit_chunks(npad);
    const size_t cks = (size_t)k * ec;
    g->timed("rle_emit", (e.fm_row + 4.0 * e.r->wpr) * k + 24.0 * cks + 8.0 * k, [&] {
        launch_rle_emit(e.fm, npad, k, g->lane_rowx[e.x].p, e.r->tlb, e.r->moves.p, g->emit_ck.p,
                        g->emit_ck.p + cks, g->emit_ck.p + 2 * cks, g->counts.p, e.es);
    });
    HIP_CHECK(hipMemcpyAsync(e.rb->counts.p, g->counts.p, k * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, e.es));
    HIP_CHECK(hipEventRecord(e.rb->ev, e.es));
}

// after either count: the run counts to the host, then the move tables
void emit_tables(const Emit& e) {
    cpd_graph* g = e.g;
    const uint32_t k = e.k, npad = g->npad;
    HIP_CHECK(hipMemcpyAsync(e.rb->counts.p, g->counts.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             e.es));
    HIP_CHECK(hipEventRecord(e.rb->ev, e.es));
    // per row: the sets (fm_row), the segment states (4 B per 32 columns;
    // the run counts are read only where the look-ahead needs them), the
    // table (npad * bits / 8)
    const double ebytes = (e.fm_row + 4.0 * npad / 32.0 + 4.0 * e.r->wpr) * k + 4.0 * k;
    g->timed("rle_moves", ebytes, [&] {
        launch_rle_moves(e.fm, g->fmb, npad, k, e.rst, e.rrc, g->lane_rowx[e.x].p, e.r->tlb,
                         e.r->moves.p, e.es);
    });
}

// chunked count + seam repair (rescans are rare and not counted), the emit
void emit_chunked(const Emit& e, uint32_t nch) {
    cpd_graph* g = e.g;
    const uint32_t k = e.k, npad = g->npad;
    HIP_CHECK(hipMemsetAsync(g->rle_hard.p, 0, sizeof(uint32_t), e.es));
    g->timed("rle_count", (e.fm_row + e.st_row + 12.0 * nch) * k, [&] {
        launch_rle_count_ch(e.fm, npad, k, e.rst, e.rrc, g->rle_xs.p, g->rle_cc.p, e.es);
    });
    g->timed("rle_fix", (12.0 * nch + 4.0) * k, [&] {
        launch_rle_fix(e.fm, npad, k, e.rst, e.rrc, g->rle_xs.p, g->rle_cc.p, g->counts.p,
                       g->rle_hard.p, e.es);
    });
    // runs too long for the seam repair: the bounded pass, which does
    // nothing unless rle_fix raised rle_hard
    g->timed("rle_recount", 0.0, [&] {
        launch_rle_count(e.fm, g->fmb, npad, k, g->counts.p, e.rst, e.rrc, e.es, g->rle_hard.p);
    });
    emit_tables(e);
}

// the count and the emit (8/16-bit sets)
void emit_plain(const Emit& e) {
    cpd_graph* g = e.g;
    const uint32_t k = e.k;
    g->timed("rle_count", (e.fm_row + e.st_row) * k + 4.0 * k, [&] {
        launch_rle_count(e.fm, g->fmb, g->npad, k, g->counts.p, e.rst, e.rrc, e.es);
    });
    emit_tables(e);
}

// The count, the seam repair and the move-table emit of this batch go to
// the emit stream (estream; `stream` when the overlap is off), after its
// first moves (ev_fm): they run beside the next batch's sweeps, and the
// run counts land in a page-locked buffer the rows settle from later
// (cpd_rows::settle) — the host waits for none of it here.
void queue_emit(cpd_graph* g, cpd_rows* r, uint32_t k, uint32_t x, uint32_t slot) {
    const uint32_t npad = g->npad;
    hipStream_t es = g->async ? g->estream : g->stream;
    if (es != g->stream) HIP_CHECK(hipStreamWaitEvent(es, g->ev_fm[slot], 0));
    // the batch's rows become table rows r->nrows + i, written by lane pos_of[i]
    const std::vector<uint32_t>& pos_of = g->bs[slot].pos_of;
    CPD_REQUIRE(r->moves.n >= (size_t)(r->nrows + k) * r->wpr, CPD_E_ARG,
                "rows: move table capacity");
    cpd_rows::Batch* rb = r->new_batch(g->B);
    rb->k = k;
    rb->pos_of.assign(pos_of.begin(), pos_of.begin() + k);
    for (uint32_t i = 0; i < k; ++i) rb->lane_rows.p[pos_of[i]] = r->nrows + i;
    const Emit e{g, r, rb, k, x, es, g->fmx[x].p, g->rle_stx[x].p, g->rle_rcx[x].p,
                 g->fmb / 8.0 * npad, 5.0 * npad / 32.0};
    HIP_CHECK(hipMemcpyAsync(g->lane_rowx[x].p, rb->lane_rows.p, k * sizeof(uint32_t),
                             hipMemcpyHostToDevice, es));
    const uint32_t nch = g->fmb == 4 ? rle_count_chunks(npad) : 0u;
    if (rle_fused(g->fmb)) emit_fused(e);
    else if (nch) emit_chunked(e, nch);  // 4-bit sets with CPD_RLE_FUSED=0
    else emit_plain(e);
    if (!r->done) HIP_CHECK(hipEventCreateWithFlags(&r->done, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(r->done, es));
    if (g->async) {
        HIP_CHECK(hipEventRecord(g->ev_emit[x], es));
        g->emit_pending[x] = true;
    }
}

// Build rows for one batch of k <= B targets; append to r (device).  next /
// next_k (may be null / 0): the targets of the batch that follows; its
// up-sweep is queued first, on ustream behind this batch's own: it writes
// the other slot's up store, so it starts as soon as this batch's up-sweep
// ends — with this batch's down-sweep — and runs beside it.
void build_batch(cpd_graph* g, const uint32_t* targets, uint32_t k, cpd_rows* r,
                 const uint32_t* next, uint32_t next_k) {
    const double t0 = now_seconds();
    const uint32_t slot = take_slot(g, targets, k);
    const bool narrow = g->narrow;
    queue_next_up(g, slot ^ 1u, next, next_k);
    launch_down(g, k, narrow, slot);
    // the first moves' buffer set, once the emit that last read it is done
    const uint32_t x = g->acquire_set();
    launch_fm(g, k, narrow, g->fmx[x].p, slot);
    const double t1 = now_seconds();
    if (narrow_check(g, k, narrow)) {
        // returns before fold_late folds the previous batch's bytes
        rebuild_in_pieces(g, targets, k, r, next, next_k);
        return;
    }
    const double t2 = now_seconds();
    queue_emit(g, r, k, x, slot);
    // the previous batch's sweep bytes: its stats landed before this down-sweep
    if (g->timing) fold_late(g, 1);
    if (switches().trace)
        std::fprintf(stderr, "[cpd] batch %u rows: launch sweeps+fm %.2f ms, to down-sweep end %.2f "
                             "ms, count+emit queued %.2f ms\n",
                     k, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (now_seconds() - t2) * 1e3);
    const std::vector<uint32_t>& pos_of = g->bs[slot].pos_of;
    r->targets.insert(r->targets.end(), targets, targets + k);
    r->lanes.insert(r->lanes.end(), pos_of.begin(), pos_of.begin() + k);
    r->nrows += k;
}

}  // namespace

extern "C" {

int cpd_build_rows(cpd_graph* g, const uint32_t* targets, uint32_t ntargets,
                   cpd_rows* reuse, cpd_rows** out) {
    return guarded([&] {
        CPD_REQUIRE(g && out && (targets || ntargets == 0), CPD_E_ARG, "build: null argument");
        *out = nullptr;
        g->select();
        if (!g->B) g->reserve_batch(0);
        cpd_rows* r = reuse ? reuse : new cpd_rows();
        std::unique_ptr<cpd_rows> owned(reuse ? nullptr : r);
        r->device = g->device;
        r->retire();  // an earlier build's unsettled batches (copies may be in flight)
        r->nrows = 0;
        r->total = 0;
        r->targets.clear();
        r->lanes.clear();
        r->offsets.assign(1, 0);
        r->n = g->n;
        // built rows at the graph's packed width (2 bits per column on the
        // bench graph): the register-resident fused emit writes them with
        // 16-B stores, half the bytes of nibble tables (6.2 against 12.3 GB
        // per 24576-row step), and the export and an index take them as
        // they are (round 4 built nibble tables and narrowed them on the way
        // out, when narrowing cost the unfused emit ~0.5 ms)
        r->tlb = g->tlb;
        r->wpr = g->npad >> (5u - r->tlb);
        r->bits = g->move_bits;
        if (r->moves.n < (size_t)ntargets * r->wpr) {
            r->wait();  // an earlier build's emit may still write the old table
            ArenaScope carve;
            r->moves.alloc((size_t)ntargets * r->wpr);
        }
        for (uint32_t b = 0; b < ntargets; b += g->B) {
            uint32_t k = std::min(g->B, ntargets - b);
            const uint32_t* next = nullptr;
            uint32_t next_k = 0;
            if (b + k < ntargets) {  // the call's own next batch
                next = targets + b + k;
                next_k = std::min(g->B, ntargets - b - k);
            } else if (!g->hint.empty()) {  // the next call's first batch
                next = g->hint.data();
                next_k = (uint32_t)std::min<size_t>(g->B, g->hint.size());
            }
            build_batch(g, targets + b, k, r, next, next_k);
        }
        g->hint.clear();
        owned.release();
        *out = r;
    });
}

int cpd_graph_hint_next(cpd_graph* g, const uint32_t* targets, uint32_t ntargets) {
    return guarded([&] {
        CPD_REQUIRE(g && (targets || ntargets == 0), CPD_E_ARG, "hint: null argument");
        for (uint32_t i = 0; i < ntargets; ++i)
            CPD_REQUIRE(targets[i] < g->n, CPD_E_ARG, "hint: target out of range");
        g->hint.assign(targets, targets + ntargets);
    });
}

int cpd_rows_count(const cpd_rows* r, uint32_t* nrows, uint64_t* total_runs) {
    return guarded([&] {
        CPD_REQUIRE(r, CPD_E_ARG, "null rows");
        if (total_runs) r->settle();
        if (nrows) *nrows = r->nrows;
        if (total_runs) *total_runs = r->total;
    });
}

int cpd_rows_wait(const cpd_rows* r) {
    return guarded([&] {
        CPD_REQUIRE(r, CPD_E_ARG, "null rows");
        r->settle();
    });
}

int cpd_rows_export(const cpd_rows* r, uint64_t* offsets, uint32_t* runs) {
    return cpd_rows_export_range(r, 0, r ? r->nrows : 0, offsets, runs);
}

int cpd_rows_export_range(const cpd_rows* r, uint32_t first, uint32_t count, uint64_t* offsets,
                          uint32_t* runs) {
    return guarded([&] {
        CPD_REQUIRE(r, CPD_E_ARG, "null rows");
        CPD_REQUIRE(first <= r->nrows && count <= r->nrows - first, CPD_E_ARG,
                    "export range: rows out of range");
        r->settle();
        const uint64_t base = r->offsets[first], end = r->offsets[first + count];
        if (offsets)
            for (uint32_t i = 0; i <= count; ++i) offsets[i] = r->offsets[first + i] - base;
        if (!runs || end == base) return;
        HIP_CHECK(hipSetDevice(r->device));
        hipStream_t st = thread_stream(r->device);
        // decode piece by piece (<= kDecodeRuns runs, a longer row alone) into
        // a staging buffer of the rows' pool, then copy out
        auto stage = r->acquire_stage();
        for (uint32_t p0 = first; p0 < first + count;) {
            uint32_t p1 = p0 + 1;
            while (p1 < first + count && r->offsets[p1 + 1] - r->offsets[p0] <= kDecodeRuns) ++p1;
            const uint64_t nr = r->offsets[p1] - r->offsets[p0];
            stage->alloc(std::max<uint64_t>(nr, std::min<uint64_t>(end - base, kDecodeRuns)));
            launch_moves_runs(r->moves.p + (size_t)p0 * r->wpr, r->wpr, r->tlb, r->n, p1 - p0,
                              r->off.p + p0, r->offsets[p0], stage->p, st);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(runs + (r->offsets[p0] - base), stage->p, nr * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            p0 = p1;
        }
        r->release_stage(std::move(stage));
    });
}

int cpd_rows_move_words(const cpd_rows* r, uint32_t* words) {
    return guarded([&] {
        CPD_REQUIRE(r && words, CPD_E_ARG, "null argument");
        *words = r->packed_words();
    });
}

int cpd_rows_move_bits(const cpd_rows* r, uint32_t* bits) {
    return guarded([&] {
        CPD_REQUIRE(r && bits, CPD_E_ARG, "null argument");
        *bits = r->bits;
    });
}

int cpd_rows_export_moves(const cpd_rows* r, uint32_t first, uint32_t count, uint32_t* moves) {
    return guarded([&] {
        CPD_REQUIRE(r && (moves || count == 0), CPD_E_ARG, "null argument");
        CPD_REQUIRE(first <= r->nrows && count <= r->nrows - first, CPD_E_ARG,
                    "export range: rows out of range");
        if (!count) return;
        HIP_CHECK(hipSetDevice(r->device));
        r->wait();
        hipStream_t st = thread_stream(r->device);
        const size_t w = r->packed_words();
        const uint32_t* src = r->moves.p + (size_t)first * r->wpr;
        if (w == r->wpr && r->bits == (1u << r->tlb)) {  // the tables as they are
            HIP_CHECK(hipMemcpyAsync(moves, src, (size_t)count * w * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            return;
        }
        // rows made contiguous at the exported width on the GPU (a pitched
        // device copy when the widths agree, else repacked), then one copy out
        auto stage = r->acquire_stage();
        stage->alloc((size_t)count * w);
        if (r->bits == (1u << r->tlb))
            HIP_CHECK(hipMemcpy2DAsync(stage->p, w * sizeof(uint32_t), src,
                                       (size_t)r->wpr * sizeof(uint32_t), w * sizeof(uint32_t),
                                       count, hipMemcpyDeviceToDevice, st));
        else
            launch_repack_moves(src, r->wpr, r->wpr, 1u << r->tlb, count, stage->p, (uint32_t)w,
                                (uint32_t)w, r->bits, st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(moves, stage->p, (size_t)count * w * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        r->release_stage(std::move(stage));
    });
}

int cpd_rows_targets(const cpd_rows* r, uint32_t* targets) {
    return guarded([&] {
        CPD_REQUIRE(r && targets, CPD_E_ARG, "null argument");
        std::memcpy(targets, r->targets.data(), r->nrows * sizeof(uint32_t));
    });
}

int cpd_rows_lanes(const cpd_rows* r, uint32_t* lanes) {
    return guarded([&] {
        CPD_REQUIRE(r && lanes, CPD_E_ARG, "null argument");
        std::memcpy(lanes, r->lanes.data(), r->nrows * sizeof(uint32_t));
    });
}

void cpd_rows_free(cpd_rows* r) {
    if (r) (void)hipSetDevice(r->device);
    delete r;
}

int cpd_debug_rows(cpd_graph* g, const uint32_t* targets, uint32_t ntargets, uint32_t* dist,
                   uint16_t* fm) {
    return guarded([&] {
        CPD_REQUIRE(g && targets, CPD_E_ARG, "debug: null argument");
        g->select();
        if (!g->B) g->reserve_batch(0);
        CPD_REQUIRE(ntargets > 0 && ntargets <= g->B, CPD_E_ARG, "debug: 0 < ntargets <= batch");
        if (g->prepped) g->drop_prep();
        const uint32_t slot = g->next_slot;
        upload_targets(g, targets, ntargets, slot, g->stream);
        launch_up(g, ntargets, slot, g->stream);
        uint32_t x = 0;
        for (;;) {
            x = g->acquire_set();
            const bool narrow = g->narrow;
            launch_down_fm(g, ntargets, narrow, g->fmx[x].p, slot);
            g->sync();
            // wide group rows past the pool: again with the dense rows
            if (!narrow || g->ovf_h() <= g->pool_cap) break;
            g->ovf_hb.p[0] = 2u * g->n * (g->B / 256u);
            narrow_decide(g);
        }
        fold_late(g, 0);
        const std::vector<uint32_t>& pos_of = g->bs[slot].pos_of;
        const std::vector<uint32_t>& tgt_col = g->bs[slot].tgt_col;
        const uint32_t n = g->n, B = g->B;
        // lane p holds the caller's target i = pos_of^-1(p)
        std::vector<uint32_t> h((size_t)n * B);
        if (!g->narrow) {
            HIP_CHECK(hipMemcpy(h.data(), g->dist.p, h.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost));
        } else {  // base + u16 offset (0xFFFF = unreachable), or a pool row
            std::vector<uint16_t> q((size_t)n * B);
            std::vector<uint32_t> b((size_t)n * (B / 256u));
            std::vector<uint32_t> pr((size_t)std::min(g->ovf_h(), g->pool_cap) * 256u);
            HIP_CHECK(hipMemcpy(q.data(), g->d16.p, q.size() * sizeof(uint16_t),
                                hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(b.data(), g->dbase.p, b.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost));
            if (!pr.empty())
                HIP_CHECK(hipMemcpy(pr.data(), g->pool.p, pr.size() * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost));
            for (uint32_t c = 0; c < n; ++c)
                for (uint32_t p = 0; p < B; ++p) {
                    const uint32_t base = b[(size_t)(p / 256u) * n + c];
                    if (base == 0xFFFFFFFEu) {  // kept wide: the pool row in its d16 words
                        const size_t w = ((size_t)c * B + (p & ~1u)) / 2u * 2u;
                        const uint32_t idx = (uint32_t)q[w] | ((uint32_t)q[w + 1] << 16);
                        h[(size_t)c * B + p] = pr[(size_t)idx * 256u + (p & 255u)];
                        continue;
                    }
                    const uint16_t d = q[(size_t)c * B + p];
                    h[(size_t)c * B + p] = d == 0xFFFFu ? CPD_INF : base + d;
                }
        }
        if (dist)
            for (uint32_t v = 0; v < n; ++v)
                for (uint32_t i = 0; i < ntargets; ++i)
                    dist[(size_t)v * ntargets + i] = h[(size_t)g->order[v] * B + pos_of[i]];
        if (fm) {
            // unpack fmb-bit sets; a column whose set is the wildcard (the
            // target, unreachable columns) reports CPD_FM_ALL like the oracle
            const uint32_t per = 32u / g->fmb, all = (1u << g->fmb) - 1u;
            const size_t row_words = g->npad / per;
            std::vector<uint32_t> w((size_t)B * row_words);
            HIP_CHECK(hipMemcpy(w.data(), g->fmx[x].p, w.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < ntargets; ++i) {
                const uint32_t p = pos_of[i];
                for (uint32_t v = 0; v < n; ++v) {
                    const uint32_t c = g->order[v];
                    // 4-bit rows are row-group interleaved (cpd_kernels.hip
                    // fm4_piece): 16-B piece (p/4, segment c/32, p%4)
                    const size_t wi =
                        g->fmb == 4 ? ((((size_t)(p >> 2) * (g->npad / 32u) + c / 32u) * 4u +
                                        (p & 3u)) * 4u + (c % 32u) / 8u)
                                    : (size_t)p * row_words + c / per;
                    const uint32_t f = (w[wi] >> (g->fmb * (c % per))) & all;
                    const bool wild = c == tgt_col[p] || h[(size_t)c * B + p] == CPD_INF;
                    fm[(size_t)i * n + v] = wild ? (uint16_t)CPD_FM_ALL : (uint16_t)f;
                }
            }
        }
    });
}

}  // extern "C"
