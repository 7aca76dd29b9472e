// cpd_graph: upload of a plan (column-space CSR, the two sweeps' lists and
// descriptors), batch sizing, and the per-kernel timing table.
#include <cmath>
#include <thread>

#include "cpd_gpu_internal.hpp"

namespace {

// Pool rows (1 KiB: one 256-target group row kept 32-bit) of a narrow batch
// of B targets: an eighth of its group rows, and at least every group row of
// one 1024-target slab, so that a batch whose wide rows overflow the pool is
// rebuilt in pieces of pool_cap / (4 n) slabs that cannot.
uint64_t pool_rows(uint32_t n, uint32_t B) {
    return std::max<uint64_t>((uint64_t)n * (B / 256u) / 8u, 4ull * n);
}

// HBM per row of batch width: the final rows (narrow: 2n of u16 offsets, the
// bases and the wide-row pool; else 4n of u32) + two compact up stores (4 B
// per node of up-level >= 2 each: batch k + 1's up-sweep runs beside batch
// k's down-sweep) + three buffer sets of first-move rows and RLE segment states
// (emit overlap) + the chunked count's chunk states (12 B per chunk: exit,
// count, entry) + leaf sets + two rows of move tables (npad / 2 each: the
// row set being built and the one a caller such as make_cpd_auto is
// exporting).  The pool's 1024-row floor is in the fixed part (pool_rows).
double batch_bytes_per_row(uint32_t n, uint32_t n_up, uint32_t npad, uint32_t fmb, bool narrow,
                           bool leaf_fm, uint32_t mbits) {
    // the fused emit keeps no segment states: 12 B per chunk of 32k columns
    const double rle = rle_fused(fmb) ? 12.0 * rle_emit_chunks(npad)
                                      : 3.0 * 5.0 / 32.0 * npad +
                                            (fmb == 4 ? 12.0 * rle_count_chunks(npad) : 0.0);
    const double fin = narrow ? (2.0 + 4.0 / 256.0 + 0.5) * n : 4.0 * n;
    return fin + 8.0 * n_up + 3.0 * fmb / 8.0 * npad + rle + (leaf_fm ? 0.5 * n : 0.0) +
           2.0 * mbits / 8.0 * npad;
}

// Nodes ordered by (level, column): node_of_slot, and lvl_first[l] = first slot.
std::vector<uint32_t> level_order(const cpd_plan& p, const std::vector<uint32_t>& level,
                                  uint32_t nlev, std::vector<uint32_t>& lvl_first) {
    const uint32_t n = p.n;
    std::vector<uint32_t> cnt(nlev + 1, 0);
    for (uint32_t v = 0; v < n; ++v) cnt[level[v] + 1]++;
    for (uint32_t l = 0; l < nlev; ++l) cnt[l + 1] += cnt[l];
    lvl_first.assign(cnt.begin(), cnt.end());
    std::vector<uint32_t> node_of_slot(n), pos(cnt.begin(), cnt.end() - 1);
    for (uint32_t c = 0; c < n; ++c) {  // columns ascending inside a level
        uint32_t v = p.inv[c];
        node_of_slot[pos[level[v]]++] = v;
    }
    return node_of_slot;
}

// Build the level-ordered sweep arrays in column space, with the closed-form
// encodings of cpd_kernels.hip (kLeafBit: upward level 0, kL1Bit: level 1,
// referenced by its slot in the ASCENDING list, asc_slot[node]).
// lvl_arcs: gathered arcs per level; lvl_reads: nodes reading their own row.
// leaf_edges (descending only): a leaf's list is its out-edges in file order
// (self loops and parallel edges included) instead of its up-arcs — the same
// minimum, and the list position is the move index for the leaf's first-move
// set (the down-sweep computes leaf sets, cpd_kernels.hip sweep_down8).
// Nodes of up-level >= 2 own a row of the compact up store, u = ascending
// slot - ubase: ascending arcs into them carry u; uidx (descending only)
// gets each slot's u (~0 for the closed forms).
void build_sweep(const cpd_plan& p, bool ascend, const std::vector<uint32_t>& asc_slot,
                 uint32_t ubase, std::vector<uint32_t>& nodes, std::vector<uint32_t>& off,
                 std::vector<uint32_t>& arcs, std::vector<uint32_t>& lvl_first,
                 std::vector<double>& lvl_arcs, std::vector<double>& lvl_reads,
                 bool leaf_edges = false, std::vector<uint32_t>* uidx = nullptr) {
    const Hierarchy& H = p.ch;
    const uint32_t n = p.n;
    const std::vector<uint32_t>& level = ascend ? H.level_up : H.level_dn;
    const uint32_t nlev = ascend ? H.nlev_up : H.nlev_dn;
    // ascend reads each node's DOWN arcs; descend reads its UP arcs
    const std::vector<uint64_t>& aoff = ascend ? H.dn_off : H.up_off;
    const std::vector<uint32_t>& adst = ascend ? H.dn_dst : H.up_dst;
    const std::vector<uint32_t>& aw = ascend ? H.dn_w : H.up_w;
    const std::vector<uint32_t>& lup = H.level_up;
    CPD_REQUIRE(aoff[n] < 0xFFFFFFFFull, CPD_E_RANGE, "hierarchy has >= 2^32 arcs");
    // (ordering a level's nodes by their lowest up-arc head instead, so that
    // nodes gathering the same rows run side by side, measured no faster)
    std::vector<uint32_t> node_of_slot = level_order(p, level, nlev, lvl_first);
    // how a node is referenced: closed form (level 0 / 1 of the up sweep) or row
    auto ref = [&](uint32_t v) -> uint32_t {
        if (lup[v] == 0) return p.order[v] | kLeafBit;
        if (lup[v] == 1) return asc_slot[v] | kL1Bit;
        return p.order[v];
    };
    nodes.assign(n, 0);
    if (uidx) uidx->assign(n, 0xFFFFFFFFu);
    for (uint32_t s = 0; s < n; ++s) {
        uint32_t v = node_of_slot[s];
        nodes[s] = ascend ? p.order[v] : ref(v);  // descending: closed-form init
        if (uidx && lup[v] >= 2) (*uidx)[s] = asc_slot[v] - ubase;
    }
    const bool leaf_rows = !ascend && leaf_edges;  // a leaf's arcs: its out-edges
    off.assign(n + 1, 0);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t v = node_of_slot[s];
        off[s + 1] = off[s] + (leaf_rows && lup[v] == 0 ? p.row_ptr[v + 1] - p.row_ptr[v]
                                                        : (uint32_t)(aoff[v + 1] - aoff[v]));
    }
    arcs.assign(2ull * off[n], 0u);
    // slots filled by 8 host threads (each writes its slots' arcs; level
    // counts per thread, summed after)
    constexpr uint32_t kThreads = 8;
    std::vector<std::vector<double>> la(kThreads, std::vector<double>(nlev, 0.0)),
        lr(kThreads, std::vector<double>(nlev, 0.0));
    auto fill = [&](uint32_t t, uint32_t s0, uint32_t s1) {
        std::vector<std::pair<uint32_t, uint32_t>> tmp;
        for (uint32_t s = s0; s < s1; ++s) {
            const uint32_t v = node_of_slot[s];
            uint32_t* out = arcs.data() + 2ull * off[s];
            if (leaf_rows && lup[v] == 0) {
                for (uint32_t e = p.row_ptr[v]; e < p.row_ptr[v + 1]; ++e) {
                    *out++ = p.order[p.dst[e]];
                    *out++ = p.w[e];
                    if (p.dst[e] != v) la[t][level[v]] += 1.0;
                }
                continue;
            }
            tmp.clear();
            for (uint64_t e = aoff[v]; e < aoff[v + 1]; ++e) tmp.push_back({p.order[adst[e]], aw[e]});
            std::sort(tmp.begin(), tmp.end());
            for (auto& a : tmp) {
                // ascending arcs into upward levels 0/1 use the closed forms,
                // the others the head's up-store row
                const uint32_t h = p.inv[a.first];
                const uint32_t r = !ascend ? a.first : lup[h] >= 2 ? asc_slot[h] - ubase : ref(h);
                *out++ = r;
                *out++ = a.second;
                if (!(r & (kLeafBit | kL1Bit))) la[t][level[v]] += 1.0;
            }
            if (!ascend && !(nodes[s] & (kLeafBit | kL1Bit))) lr[t][level[v]] += 1.0;
        }
    };
    {
        std::vector<std::thread> th;
        const uint32_t per = (n + kThreads - 1u) / kThreads;
        for (uint32_t t = 0; t < kThreads; ++t)
            th.emplace_back(fill, t, std::min(n, t * per), std::min(n, (t + 1u) * per));
        for (auto& x : th) x.join();
    }
    lvl_arcs.assign(nlev, 0.0);
    lvl_reads.assign(nlev, 0.0);
    for (uint32_t t = 0; t < kThreads; ++t)
        for (uint32_t l = 0; l < nlev; ++l) {
            lvl_arcs[l] += la[t][l];
            lvl_reads[l] += lr[t][l];
        }
}

// Hilbert-curve index of each node's (x, y), scaled to a 2^16 x 2^16 grid over
// the bounding box: nearby keys are nearby points, and any run of keys covers
// a compact region (the DFS column order follows the DFS tree, whose long
// branches and back-jumps spread a run of columns out).
std::vector<uint32_t> hilbert_keys(const int32_t* x, const int32_t* y, uint32_t n) {
    std::vector<uint32_t> key(n, 0);
    if (!n) return key;
    const int64_t x0 = *std::min_element(x, x + n), y0 = *std::min_element(y, y + n);
    const int64_t ext = std::max<int64_t>(*std::max_element(x, x + n) - x0,
                                          *std::max_element(y, y + n) - y0) + 1;
    constexpr uint32_t kSide = 1u << 16;
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t px = (uint32_t)(((int64_t)x[v] - x0) * (kSide - 1) / ext);
        uint32_t py = (uint32_t)(((int64_t)y[v] - y0) * (kSide - 1) / ext);
        uint64_t d = 0;
        for (uint32_t s = kSide / 2; s > 0; s /= 2) {
            const uint32_t rx = (px & s) ? 1u : 0u, ry = (py & s) ? 1u : 0u;
            d += (uint64_t)s * s * ((3u * rx) ^ ry);
            if (ry == 0) {  // rotate the quadrant (only the lower bits matter from here)
                if (rx == 1) {
                    px = kSide - 1 - px;
                    py = kSide - 1 - py;
                }
                std::swap(px, py);
            }
        }
        key[v] = (uint32_t)d;
    }
    return key;
}

}  // namespace

cpd_graph::~cpd_graph() {
    if (hipSetDevice(device) == hipSuccess) {
        if (estream) (void)hipStreamSynchronize(estream);
        for (auto e : ev_emit)
            if (e) (void)hipEventDestroy(e);
        if (estream) (void)hipStreamDestroy(estream);
        if (ustream) (void)hipStreamSynchronize(ustream);
        for (auto e : {ev_up, ev_down, ev_fm[0], ev_fm[1]})
            if (e) (void)hipEventDestroy(e);
        if (ustream) (void)hipStreamDestroy(ustream);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto& p : pending) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
}

void cpd_graph::group_begin(const char* name, hipStream_t st) {
    if (!timing) return;
    group = Pending{name, get_event(), nullptr, 0.0, {}, 0};
    group_stream = st;
    HIP_CHECK(hipEventRecord(group.a, st));
    group_open = true;
}

void cpd_graph::group_end() {
    if (!group_open) return;
    group_open = false;
    group.b = get_event();
    HIP_CHECK(hipEventRecord(group.b, group_stream));
    if (group.launches) {
        pending.push_back(std::move(group));
    } else {
        ev_pool.push_back(group.a);
        ev_pool.push_back(group.b);
    }
    group = Pending{};
}

void cpd_graph::sync(bool all) {
    HIP_CHECK(hipStreamSynchronize(stream));
    if (all) {
        drain_emits();
        if (ustream) HIP_CHECK(hipStreamSynchronize(ustream));
    }
    std::vector<Pending> keep;
    for (auto& p : pending) {
        if (hipEventQuery(p.b) != hipSuccess) {
            keep.push_back(std::move(p));
            continue;
        }
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
        Agg& g = agg[p.name];
        g.launches += p.launches;
        g.ms += ms;
        g.bytes += p.bytes;
        for (auto& f : p.late) g.bytes += f();
        ev_pool.push_back(p.a);
        ev_pool.push_back(p.b);
    }
    pending.swap(keep);
}

void cpd_graph::reserve_batch(uint32_t want) {
    ArenaScope carve;  // the batch's buffers: what an arena is committed for
    if (want == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        // per target (batch_bytes_per_row), in 85% of free HBM; at most
        // 24 slabs.  Larger batches amortise the latency-bound
        // narrow levels: at 1M nodes 20480 rows per batch measured 310.5k
        // rows/s against 296.1k for 16384 (round 2).
        const double per = batch_bytes_per_row(n, n_up, npad, fmb, narrow, leaf_fm,
                                               1u << tlb);
        const double fixed = narrow ? 4096.0 * n : 0.0;  // the pool's floor (pool_rows)
        const double avail = free_b > hbm_reserve + fixed ? (double)free_b - hbm_reserve - fixed
                                                          : 0.0;
        const double fit = 0.85 * avail / per;
        CPD_REQUIRE(hbm_reserve == 0 || fit >= 1024.0, CPD_E_OOM,
                    "HBM reserve of " + std::to_string(hbm_reserve >> 20) + " MiB leaves " +
                        std::to_string((size_t)avail >> 20) + " MiB: too little for a 1024-row batch");
        want = (uint32_t)std::min((double)switches().batch_max, std::max(1024.0, std::floor(fit / 1024) * 1024));
    }
    want = (want + 1023u) / 1024u * 1024u;
    if (want == B && upx[0].p) return;
    drain_emits();
    drop_prep();
    B = want;
    for (int s = 0; s < 2; ++s) {
        upx[s].alloc(std::max<size_t>((size_t)n_up * B, 1));
        livex[s].alloc(std::max<uint32_t>(n_up, 1u));
        tmaskx[s].alloc(n);
    }
    alloc_final_rows();
    // each further buffer set when it takes under an eighth of the HBM
    // still free after the batch's own buffers (one set: emits do not
    // overlap)
    const bool fused = rle_fused(fmb);
    const size_t set_bytes = (size_t)B * (npad / (32u / fmb)) * 4u +
                             (fused ? 0u : (size_t)B * (npad / 32u) * 5u) + 4u * B;
    nsets = 1;
    for (uint32_t x = 0; x < kSets; ++x) {
        if (x >= 1) {
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            if (!(switches().async && set_bytes * 8 < (free_b > hbm_reserve ? free_b - hbm_reserve : 0))) {
                for (uint32_t y = x; y < kSets; ++y) {
                    fmx[y].release();
                    rle_stx[y].release();
                    rle_rcx[y].release();
                    lane_rowx[y].release();
                }
                break;
            }
            nsets = x + 1;
        }
        fmx[x].alloc((size_t)B * (npad / (32u / fmb)));
        if (fused) {
            rle_stx[x].release();
            rle_rcx[x].release();
        } else {
            rle_stx[x].alloc((size_t)B * (npad / 32u));
            rle_rcx[x].alloc((size_t)B * (npad / 32u));
        }
        lane_rowx[x].alloc(B);
    }
    async = nsets > 1;
    cur = 0;
    if (fused) {
        emit_ck.alloc(3ull * B * rle_emit_chunks(npad));
    } else if (fmb == 4 && rle_count_chunks(npad)) {
        rle_xs.alloc(2ull * B * rle_count_chunks(npad));
        rle_cc.alloc((size_t)B * rle_count_chunks(npad));
        rle_hard.alloc(1);
    }
    if (leaf_fm) fmleaf.alloc((size_t)n * (B / 4u));
    for (auto& b : bs) {
        b.tgt.alloc(B);
        b.tgt_h.alloc(B);
    }
    fm_tgt.alloc(B);
    counts.alloc(B);
    rle_hard_h.alloc(1);
    ovf_hb.alloc(1);
    ovf_hb.p[0] = 0;
}

void cpd_graph::alloc_final_rows() {
    ArenaScope carve;
    if (narrow) {
        dist.release();
        d16.alloc((size_t)n * B);
        dbase.alloc((size_t)n * (B / 256u));
        pool_cap = (uint32_t)std::min<uint64_t>(pool_rows(n, B), 0xFFFFFFFEull);
        pool.alloc((size_t)pool_cap * 256u);
        ovf.alloc(1);
    } else {
        d16.release();
        dbase.release();
        pool.release();
        pool_cap = 0;
        dist.alloc((size_t)n * B);
    }
}

namespace {

// The steps of cpd_graph_create, in its order; tg0: when it began.
void trace_step(const char* what, double tg0) {
    if (switches().trace) std::fprintf(stderr, "[cpd] graph %s %.3f s\n", what, now_seconds() - tg0);
}

// Three streams: the main one (down-sweep, first moves), the emit
// stream and the up-sweep stream, where the next batch's up-sweep runs
// beside the previous batch's first moves.  CU masks were measured and
// removed: the up-sweep given q of every 8 CUs and the other streams
// the rest (rounds 4-6: 350.6k / 324.2k against 366.7k rows/s; r06d:
// 355.9k / 310.6k against 380.1k), or the up-sweep alone confined to
// q of 8 (397.3-420.4k against 420.0-421.5k, profiles/up_store_ab/r06s_*).
void create_streams(cpd_graph* g) {
    HIP_CHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    // (a lowest-priority emit stream measured the same: 65.2-65.7 ms/step
    // in round 5, 374.6-375.9k against 375.2-375.9k rows/s with the
    // one-wave emit, profiles/up_store_ab/r06k_*)
    HIP_CHECK(hipStreamCreateWithFlags(&g->estream, hipStreamNonBlocking));
    {
        // the highest priority: its small, latency-bound level kernels
        // must get CUs while the other streams' workgroups are queued (at
        // equal priority they waited for all of them to be dispatched:
        // 15 ms for a 0.7-ms init kernel; beside the first moves, as now,
        // normal priority measured the same: 419.1k against 413.2-419.1k
        // rows/s, profiles/up_store_ab/r06o_*)
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&g->ustream, hipStreamNonBlocking, greatest));
    }
    for (hipEvent_t* e : {&g->ev_up, &g->ev_down, &g->ev_fm[0], &g->ev_fm[1]})
        HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (auto& e : g->ev_emit) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

// The plan's graph in column space (host side) and the widths that follow
// from its largest out-degree, which is returned.
uint32_t column_space_csr(cpd_graph* g, const cpd_plan* p) {
    const uint32_t n = p->n, m = p->m;
    g->n = n;
    g->m = m;
    g->npad = (n + kFmTile - 1u) / kFmTile * kFmTile;
    g->order = p->order;
    g->inv = p->inv;
    // column-space CSR, per-node out-edge order preserved (moves = file order)
    g->rowc_host.assign(n + 1, 0);
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t v = p->inv[c];
        g->rowc_host[c + 1] = g->rowc_host[c] + (p->row_ptr[v + 1] - p->row_ptr[v]);
    }
    std::vector<uint32_t>& dstc = g->dst_col_host;
    dstc.resize(m);
    g->edge_perm.resize(m);
    g->w_free_col.resize(m);
    uint32_t maxdeg = 1;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t v = p->inv[c];
        uint32_t b = p->row_ptr[v], k = p->row_ptr[v + 1] - b;
        maxdeg = std::max(maxdeg, k);
        for (uint32_t i = 0; i < k; ++i) {
            uint32_t e = g->rowc_host[c] + i;
            g->edge_perm[e] = b + i;
            dstc[e] = p->order[p->dst[b + i]];
            g->w_free_col[e] = p->w[b + i];
        }
    }
    while ((1u << g->adj_shift) < maxdeg) ++g->adj_shift;
    g->fmb = fm_bits(g->adj_shift);
    g->move_bits = maxdeg <= 2 ? 1u : maxdeg <= 4 ? 2u : 4u;
    g->tlb = g->move_bits == 1u ? 0u : g->move_bits == 2u ? 1u : 2u;
    return maxdeg;
}

void upload_adjacency(cpd_graph* g) {
    hipStream_t s = g->stream;
    g->order_d.upload(g->order.data(), g->n, s);
    g->row_ptr.upload(g->rowc_host.data(), g->n + 1, s);
    g->dst.upload(g->dst_col_host.data(), g->m, s);
    g->w.upload(g->w_free_col.data(), g->m, s);
    std::vector<uint32_t> adj = g->packed_adjacency(g->w_free_col);
    g->adj.upload(adj.data(), adj.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
}

// The two sweeps' lists on the host, kept for the down-sweep's descriptors.
struct SweepLists {
    std::vector<uint32_t> nodes, off, arcs;          // ascending
    std::vector<uint32_t> dnodes, doff, darcs, dup;  // descending; dup: slot -> up index
};

// Both sweeps' level-ordered lists, built and uploaded (build_sweep).
SweepLists build_sweep_lists(cpd_graph* g, const cpd_plan* p, double tg0) {
    const uint32_t n = g->n;
    hipStream_t s = g->stream;
    SweepLists L;
    std::vector<uint32_t> lvl;
    std::vector<double> unused;
    std::vector<uint32_t> asc_slot(n);
    {
        std::vector<uint32_t> node_of_slot =
            level_order(*p, p->ch.level_up, p->ch.nlev_up, lvl);
        for (uint32_t s2 = 0; s2 < n; ++s2) asc_slot[node_of_slot[s2]] = s2;
    }
    // the up store's rows: the nodes of up-level >= 2, in ascending slot order
    g->ubase = lvl.size() > 2 ? lvl[2] : n;
    g->n_up = n - g->ubase;
    // the two sweeps' lists are independent host work (~0.1 s each at 1M
    // nodes): the down-sweep's is built on a second thread meanwhile
    g->leaf_fm = g->fmb == 4 && switches().leaffm;
    std::exception_ptr derr;
    std::thread dthr([&] {
        try {
            build_sweep(*p, false, asc_slot, g->ubase, L.dnodes, L.doff, L.darcs, g->dsc_lvl,
                        g->dsc_lvl_arcs, g->dsc_lvl_reads, g->leaf_fm, &L.dup);
        } catch (...) {
            derr = std::current_exception();
        }
    });
    struct Join {
        std::thread& t;
        ~Join() {
            if (t.joinable()) t.join();
        }
    } djoin{dthr};
    build_sweep(*p, true, asc_slot, g->ubase, L.nodes, L.off, L.arcs, g->asc_lvl, g->asc_lvl_arcs,
                unused);
    g->asc_off_host = L.off;
    g->asc_nodes.upload(L.nodes.data(), L.nodes.size(), s);
    g->asc_off.upload(L.off.data(), L.off.size(), s);
    g->asc_arcs.upload(L.arcs.data(), L.arcs.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    trace_step("up lists", tg0);
    g->ch_arcs = L.arcs.size() / 2;
    // leaf first moves in the down-sweep: 4-bit sets only (<= 4 slots)
    dthr.join();
    if (derr) std::rethrow_exception(derr);
    g->dsc_nodes.upload(L.dnodes.data(), L.dnodes.size(), s);
    g->dsc_off.upload(L.doff.data(), L.doff.size(), s);
    g->dsc_arcs.upload(L.darcs.data(), L.darcs.size(), s);
    g->dsc_up.upload(L.dup.data(), L.dup.size(), s);
    return L;
}

// The narrow down-sweep's slot descriptors (down_desc_arcs, cpd_kernels.hpp).
void fill_down_desc(cpd_graph* g, const SweepLists& L) {
    const uint32_t n = g->n;
    const std::vector<uint32_t>&nodes = L.dnodes, &off = L.doff, &arcs = L.darcs, &dup = L.dup;
    const uint32_t na = down_desc_arcs();
    std::vector<uint32_t> desc((size_t)n * 32u, 0u);
    const std::vector<uint32_t>& aoff = g->asc_off_host;
    // 128 B per node written by 8 host threads (each node's own slots)
    auto fill = [&](uint32_t x0, uint32_t x1) {
        for (uint32_t x = x0; x < x1; ++x) {
            uint32_t* d = desc.data() + (size_t)x * 32u;
            d[0] = nodes[x];
            d[1] = off[x];
            d[2] = off[x + 1];
            d[3] = dup[x];
            for (uint32_t i = 0; i < na; ++i) {
                const bool in = off[x] + i < off[x + 1];
                d[4 + 2 * i] = in ? arcs[2 * (size_t)(off[x] + i)] : 0xFFFFFFFFu;
                d[5 + 2 * i] = in ? arcs[2 * (size_t)(off[x] + i) + 1] : 0u;
            }
            if (nodes[x] & kL1Bit) {  // level-1 closed form inputs
                const uint32_t s1 = nodes[x] & ~kL1Bit;
                d[16] = L.nodes[s1];
                d[17] = aoff[s1 + 1] - aoff[s1];
                for (uint32_t i = 0; i < 4 && aoff[s1] + i < aoff[s1 + 1]; ++i) {
                    d[18 + 2 * i] = L.arcs[2 * (size_t)(aoff[s1] + i)] & ~kLeafBit;
                    d[19 + 2 * i] = L.arcs[2 * (size_t)(aoff[s1] + i) + 1];
                }
            }
        }
    };
    {
        constexpr uint32_t kFillThreads = 8;
        const uint32_t per = (n + kFillThreads - 1u) / kFillThreads;
        std::vector<std::thread> ft;
        for (uint32_t t = 0; t < kFillThreads; ++t)
            ft.emplace_back(fill, std::min(n, t * per), std::min(n, (t + 1u) * per));
        for (auto& t : ft) t.join();
    }
    g->dsc_desc.upload(desc.data(), desc.size(), g->stream);
}

// The CH leaves' column bits, and their counts for the bytes model.
void mark_leaves(cpd_graph* g, const cpd_plan* p) {
    std::vector<uint32_t> lb(g->npad / 32u, 0u);
    g->dsc_lvl_leaves.assign(g->dsc_lvl.size(), 0.0);
    for (uint32_t v = 0; v < g->n; ++v)
        if (p->ch.level_up[v] == 0) {
            const uint32_t c = p->order[v];
            lb[c >> 5] |= 1u << (c & 31u);
            g->n_leaf += 1;
            g->m_leaf += p->row_ptr[v + 1] - p->row_ptr[v];
            g->dsc_lvl_leaves[p->ch.level_dn[v]] += 1;
        }
    g->leafbits.upload(lb.data(), lb.size(), g->stream);
}

void chunk_narrow_up_levels(cpd_graph* g) {
    // up levels of at most kNarrow nodes run chunked (256 / 1024 / 4096:
    // 341.1k / 341.2k / 333.8k rows/s, profiles/narrow_ab/)
    constexpr uint32_t kNarrow = 1024u;
    const uint32_t C = sweep_chunk_arcs();
    std::vector<uint32_t> items, slots;
    g->up_item_first.assign(g->asc_lvl.size(), 0);
    for (size_t l = 0; l + 1 < g->asc_lvl.size(); ++l) {
        g->up_item_first[l] = (uint32_t)(items.size() / 4);
        const uint32_t s0 = g->asc_lvl[l], s1 = g->asc_lvl[l + 1];
        if (l < 2 || s1 - s0 > kNarrow) continue;
        for (uint32_t x = s0; x < s1; ++x) {
            slots.push_back(x);
            for (uint32_t a = g->asc_off_host[x]; a < g->asc_off_host[x + 1]; a += C)
                items.insert(items.end(),
                             {x, a, std::min(a + C, g->asc_off_host[x + 1]), 0u});
        }
    }
    g->up_item_first.back() = (uint32_t)(items.size() / 4);
    g->up_items.upload(items.data(), items.size(), g->stream);
    g->up_init_slots.upload(slots.data(), slots.size(), g->stream);
    g->n_init_slots = (uint32_t)slots.size();
}

// slot -> level of both sweeps (live_stats)
void upload_level_maps(cpd_graph* g) {
    const uint32_t n = g->n;
    auto lvl_of = [n](const std::vector<uint32_t>& first) {
        std::vector<uint32_t> v(n, 0);
        for (size_t l = 0; l + 1 < first.size(); ++l)
            for (uint32_t x = first[l]; x < first[l + 1]; ++x) v[x] = (uint32_t)l;
        return v;
    };
    std::vector<uint32_t> la = lvl_of(g->asc_lvl), ld = lvl_of(g->dsc_lvl);
    g->asc_lvl_of.upload(la.data(), n, g->stream);
    g->dsc_lvl_of.upload(ld.data(), n, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
}

}  // namespace

extern "C" {

int cpd_batch_bytes(uint32_t n, uint32_t max_degree, uint32_t batch, uint64_t* bytes) {
    return guarded([&] {
        CPD_REQUIRE(bytes && batch % 1024u == 0 && batch > 0, CPD_E_ARG,
                    "batch_bytes: batch must be a positive multiple of 1024");
        uint32_t shift = 0;
        while ((1u << shift) < std::max(1u, max_degree)) ++shift;
        const uint32_t fmb = fm_bits(shift);
        const uint32_t npad = (n + kFmTile - 1u) / kFmTile * kFmTile;
        // narrow rows and leaf sets assumed, every node with a row in the up
        // stores (their upper bounds: the hierarchy is not known yet), plus the
        // pool's floor, the per-column arrays and the lane tables
        const uint32_t mbits = max_degree <= 2u ? 1u : max_degree <= 4u ? 2u : 4u;
        *bytes = (uint64_t)(batch_bytes_per_row(n, n, npad, fmb, true, fmb == 4, mbits) * batch) +
                 (uint64_t)batch * (n / 256u + 1u) * 4u + 4096ull * n + 512ull * n + (64ull << 20);
    });
}

int cpd_graph_create(const cpd_plan* p, int device, cpd_graph** out) {
    return guarded([&] {
        CPD_REQUIRE(p && out, CPD_E_ARG, "graph: null argument");
        *out = nullptr;
        CPD_REQUIRE(p->order.size() == p->n, CPD_E_ARG, "plan holds a hierarchy only");
        require_device();
        const double tg0 = now_seconds();
        auto g = std::make_unique<cpd_graph>();
        g->device = device;
        g->select();
        create_streams(g.get());
        trace_step("streams", tg0);
        column_space_csr(g.get(), p);
        upload_adjacency(g.get());
        trace_step("csr+adjacency", tg0);
        g->has_ch = !p->ch.rank.empty();
        if (!g->has_ch) {  // query-only graph (fifo_auto)
            *out = g.release();
            return;
        }
        const SweepLists lists = build_sweep_lists(g.get(), p, tg0);
        fill_down_desc(g.get(), lists);
        HIP_CHECK(hipStreamSynchronize(g->stream));
        trace_step("down lists+desc", tg0);
        g->ch_arcs += lists.darcs.size() / 2;
        g->narrow = narrow_rows_on() && p->dist_bound < 0xFFFFFFFEull;
        mark_leaves(g.get(), p);
        for (auto& b : g->bs) {
            b.stat.alloc(2 * (g->asc_lvl.size() + g->dsc_lvl.size()));
            b.stat_h.alloc(b.stat.n);
            std::fill(b.stat_h.p, b.stat_h.p + b.stat.n, 0u);
        }
        chunk_narrow_up_levels(g.get());
        upload_level_maps(g.get());
        trace_step("levels", tg0);
        *out = g.release();
    });
}

int cpd_graph_set_batch(cpd_graph* g, uint32_t batch) {
    return guarded([&] {
        CPD_REQUIRE(g, CPD_E_ARG, "null graph");
        CPD_REQUIRE(batch % 1024u == 0 && batch <= 32768u, CPD_E_ARG,
                    "batch must be a multiple of 1024, at most 32768");
        g->select();
        HIP_CHECK(hipStreamSynchronize(g->stream));
        g->reserve_batch(batch);
    });
}

int cpd_graph_set_hbm_reserve(cpd_graph* g, uint64_t bytes) {
    return guarded([&] {
        CPD_REQUIRE(g, CPD_E_ARG, "null graph");
        g->hbm_reserve = bytes;
    });
}

int cpd_graph_set_coords(cpd_graph* g, const int32_t* x, const int32_t* y) {
    return guarded([&] {
        CPD_REQUIRE(g, CPD_E_ARG, "null graph");
        if (!x || !y) {
            g->lane_key.clear();
            g->seg_order.release();
            return;
        }
        g->lane_key = hilbert_keys(x, y, g->n);
        if (switches().fm_order) {
            // first_moves gathers each column's out-neighbours' rows: with the
            // segments handed out in Hilbert order, the blocks one XCD runs at
            // once cover a compact patch of the graph and gather overlapping
            // rows (in DFS order a lattice node's cross neighbours are far)
            const uint32_t nseg = g->npad / 32u;
            std::vector<uint32_t> node_of(g->n);
            for (uint32_t v = 0; v < g->n; ++v) node_of[g->order[v]] = v;
            std::vector<uint64_t> kv(nseg);
            for (uint32_t sg = 0; sg < nseg; ++sg) {
                const uint32_t c = std::min(g->n - 1u, sg * 32u + 16u);
                kv[sg] = ((uint64_t)g->lane_key[node_of[c]] << 32) | sg;
            }
            std::sort(kv.begin(), kv.end());
            std::vector<uint32_t> so(nseg);
            for (uint32_t i = 0; i < nseg; ++i) so[i] = (uint32_t)kv[i];
            g->select();
            g->seg_order.upload(so.data(), nseg, g->stream);
            HIP_CHECK(hipStreamSynchronize(g->stream));
        }
    });
}

int cpd_graph_move_bits(const cpd_graph* g, uint32_t* bits) {
    return guarded([&] {
        CPD_REQUIRE(g && bits, CPD_E_ARG, "null argument");
        *bits = g->move_bits;
    });
}

int cpd_graph_get_batch(const cpd_graph* g, uint32_t* batch) {
    return guarded([&] {
        CPD_REQUIRE(g && batch, CPD_E_ARG, "null argument");
        *batch = g->B;
    });
}

void cpd_graph_free(cpd_graph* g) { delete g; }

// ---------------------------------------------------------------------------
// Timing

int cpd_timing_enable(cpd_graph* g, int enable) {
    return guarded([&] {
        CPD_REQUIRE(g, CPD_E_ARG, "null graph");
        g->timing = enable != 0;
    });
}

int cpd_timing_reset(cpd_graph* g) {
    return guarded([&] {
        CPD_REQUIRE(g, CPD_E_ARG, "null graph");
        g->select();
        g->sync(true);
        fold_late(g, 0);
        g->agg.clear();
    });
}

int cpd_timing_get(const cpd_graph* g, cpd_kernel_time* out, int max, int* count) {
    return guarded([&] {
        CPD_REQUIRE(g && count, CPD_E_ARG, "null argument");
        // emits may still run on the emit stream: fold them in first
        auto* gm = const_cast<cpd_graph*>(g);
        gm->select();
        gm->sync(true);
        fold_late(gm, 0);
        int k = 0;
        for (auto& kv : g->agg) {
            if (out && k < max) {
                std::memset(out[k].name, 0, sizeof out[k].name);
                std::strncpy(out[k].name, kv.first.c_str(), sizeof out[k].name - 1);
                out[k].launches = kv.second.launches;
                out[k].ms = kv.second.ms;
                out[k].bytes = kv.second.bytes;
            }
            ++k;
        }
        *count = std::min(k, out ? max : k);
    });
}

}  // extern "C"
