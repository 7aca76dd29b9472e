// The CPD-heuristic search driver (cpd_query_search): option checks, the
// per-row tables, the workspace policy and the passes.
#include "cpd_gpu_internal.hpp"

namespace {

// The search workspace policy (fifo_auto and the bench
// run the same one).  capacity 0 = automatic: the first pass's columns per
// lane are 2^13 when fscale > 0 (a bounded-suboptimal search expands ~140
// nodes on the 1M bench graph) and 2^14 at fscale 0 (~47k expansions on
// average, heavy-tailed: a first pass that stops the long searches early and
// resumes them in fuller waves beats one that spills fewer —
// profiles/search_heap_ab/r05y_*: 5.08k q/s from 2^14, 4.73k from 2^15),
// lowered to 2^10 at most until
// every search of the request gets a lane (profiles/search_cap_ab/,
// search_lanes_ab/); capacity_max 0 = 4x the graph's columns rounded up to
// a power of 2 (a search holds each column once, its heap some stale
// entries more), at most 2^24; workspace_frac 0 = 0.85 of the free HBM.
// An explicit capacity keeps the old defaults (no escalation, 0.25).
uint32_t pow2_at_least(uint64_t x) {
    uint32_t c = 64;
    while (c < x && c < (1u << 24)) c <<= 1;
    return c;
}

// The option checks; returns the share of HBM the passes may use.
double check_search_opts(const cpd_index* ix, const cpd_search_opts& o) {
    const bool auto_cap = o.capacity == 0;
    CPD_REQUIRE(auto_cap || ((o.capacity & (o.capacity - 1)) == 0 && o.capacity >= 64 &&
                             o.capacity <= (1u << 24)),
                CPD_E_ARG, "search capacity must be 0 (automatic) or a power of 2 in [64, 2^24]");
    CPD_REQUIRE(o.capacity_max == 0 ||
                    ((o.capacity_max & (o.capacity_max - 1)) == 0 &&
                     o.capacity_max >= std::max<uint32_t>(o.capacity, 64u) &&
                     o.capacity_max <= (1u << 24)),
                CPD_E_ARG, "search capacity_max must be 0 or a power of 2 in [capacity, 2^24]");
    CPD_REQUIRE(o.hscale >= 0.0 && o.fscale >= 0.0, CPD_E_ARG,
                "hscale and fscale must be >= 0");
    CPD_REQUIRE(o.workspace_frac >= 0.0 && o.workspace_frac <= 0.9, CPD_E_ARG,
                "workspace_frac must be in [0, 0.9]");
    const double wfrac = o.workspace_frac > 0.0 ? o.workspace_frac : auto_cap ? 0.85 : 0.25;
    CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG, "search: index incomplete");
    CPD_REQUIRE(o.tables == CPD_SEARCH_AUTO || o.tables == CPD_SEARCH_TABLES ||
                    o.tables == CPD_SEARCH_WALKS,
                CPD_E_ARG, "search tables must be CPD_SEARCH_AUTO, _TABLES or _WALKS");
    return wfrac;
}

// per-row tables (20 B per column per row) when they fit in half of
// the free HBM (AUTO) or when asked for; else memoised walks
bool decide_tables(const cpd_index* ix, const cpd_search_opts& o) {
    const size_t cells = (size_t)ix->nrows * ix->g->n;
    bool tables = o.tables == CPD_SEARCH_TABLES;
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t have = ix->hrow.p ? 20u * cells : 0u;
    const bool fits = 20u * cells - have < (free_b + have) / 2;
    if (o.tables == CPD_SEARCH_AUTO) tables = fits;
    CPD_REQUIRE(!tables || fits, CPD_E_OOM,
                "cpd-search tables need " + std::to_string((20u * cells) >> 20) +
                    " MiB (20 B per column per index row): use the walk form");
    return tables;
}

// The per-row tables, (re)built when they are missing or the weights have
// changed; returns the kernel time in ms (0: nothing to build).
double build_search_tables(cpd_index* ix, const uint32_t* adj_w, bool tables) {
    cpd_graph* g = ix->g;
    const uint32_t n = g->n;
    const size_t cells = (size_t)ix->nrows * n;
    Events<2> ev(g);
    if (!tables || (ix->h_ready && ix->c_ready)) return 0.0;
    size_t free_b = 0, total_b = 0;
    ix->hrow.alloc(cells);
    ix->crow.alloc(cells);
    ix->lrow.alloc(cells);
    std::vector<uint32_t> tc(ix->nrows, 0);
    for (uint32_t c = 0; c < n; ++c)
        if (ix->row_of_col[c] != CPD_INF) tc[ix->row_of_col[c]] = c;
    ix->tcol.upload(tc.data(), tc.size(), g->stream);
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    // scratch for the doubling rounds: 48 B per column per chunk row
    const uint32_t chunk = (uint32_t)std::max<size_t>(
        1, std::min<size_t>(ix->nrows, (size_t)(free_b / 4) / (48ull * n + 1)));
    DevBuf<uint8_t> scratch;
    scratch.alloc((size_t)chunk * n * 48u);
    HIP_CHECK(hipEventRecord(ev.e[0], g->stream));
    launch_search_tables(ix->dense.p, g->npad, g->tlb, g->adj.p, adj_w, g->adj_shift, ix->tcol.p,
                         ix->nrows, n, scratch.p, chunk, ix->hrow.p, ix->crow.p,
                         ix->lrow.p, ix->h_ready ? 0 : 1, g->stream);
    HIP_CHECK(hipEventRecord(ev.e[1], g->stream));
    HIP_CHECK(hipStreamSynchronize(g->stream));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ix->h_ready = ix->c_ready = true;
    return ms;
}

// The passes: pass 1 runs every query at `cap` columns per lane; a
// search that would outgrow it stops whole and spills its state
// (fin 3) or, with the pool full, stops to restart (fin 2); each
// later pass runs those at 4x the capacity — spilled ones resumed
// from their records — until none is left or capacity_max (or the
// HBM) is reached; what is left then reports finished = 2.
struct SearchPasses {
    cpd_index* ix;
    cpd_graph* g;
    const cpd_search_opts& o;
    const uint32_t* adj_w;
    const bool tables;
    const double wfrac;
    // paths: the PATHS form of the kernel (cpd_query_search_paths) — par in
    // the workspace and the records, every search's prefix into ix->spp_pool
    // (pool_entries u32, allocated by the caller before the first pass is
    // sized: avail() then sees what is left)
    const bool paths;
    const uint64_t pool_entries;
    hipStream_t sm;
    uint32_t cap_max, cap;
    uint64_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double ms = 0.0;
    uint64_t reruns = 0, resumed = 0, restarted = 0, wasted = 0, lanes1 = 0;
    uint32_t passes = 0, cap_last;
    // Pass-local arrays (m queries; pass 1: the index's own, m = nq).
    uint32_t m;
    std::vector<uint32_t> gidx;               // pass query -> caller-sorted query (pass >= 2)
    DevBuf<uint32_t> d_idx, d_q, d_hops, d_st;
    DevBuf<uint64_t> d_cost;
    DevBuf<uint8_t> d_fin;
    DevBuf<unsigned long long> d_agg, d_res;
    // paths: the pass's prefix records (pass >= 2; pass 1: the index's own)
    DevBuf<unsigned long long> d_poff;
    DevBuf<uint32_t> d_pn, d_vcol, d_vlw;
    SearchPathsArgs pa;
    int pin = 0;                              // spool[pin]: the records the pass resumes from
    bool have_resume = false;
    // the pass being run (size_pass): its inputs and outputs, lanes, spill pool
    bool first = true, more = false;          // more: a later pass can take what overflows
    const uint32_t *pq_s = nullptr, *pq_t = nullptr, *pq_r = nullptr;
    uint64_t* p_cost = nullptr;
    uint32_t *p_hops = nullptr, *p_st = nullptr;
    uint8_t* p_fin = nullptr;
    unsigned long long* p_agg = nullptr;
    uint32_t slots = 0;
    SearchSpillArgs sa;
    unsigned long long hp[8];                 // the pass's sums (launch_pass)

    SearchPasses(cpd_index* index, const cpd_search_opts& opts, const uint32_t* adj, bool tab,
                 double frac, bool with_paths = false, uint64_t pool = 0)
        : ix(index), g(index->g), o(opts), adj_w(adj), tables(tab), wfrac(frac),
          paths(with_paths), pool_entries(pool), sm(g->stream), m(index->nq) {
        const bool auto_cap = o.capacity == 0;
        cap_max = o.capacity_max ? o.capacity_max
                  : auto_cap     ? pow2_at_least(4ull * std::max(g->n, 16u))
                                 : o.capacity;
        cap = auto_cap ? first_capacity() : o.capacity;
        cap_last = cap;
        ix->qstats.alloc(5ull * std::max(1u, m));
        ix->sagg.alloc(8);
        ix->stop.alloc(1);
        if (paths) {
            for (DevBuf<uint32_t>* b : {&ix->spp_pn, &ix->spp_vcol, &ix->spp_vlw})
                b->alloc(std::max(1u, m));
            ix->spp_off.alloc(std::max(1u, m));
            ix->spp_top.alloc(1);
            HIP_CHECK(hipMemsetAsync(ix->spp_top.p, 0, sizeof(unsigned long long), sm));
        }
    }

    // HBM the passes may use: what is free plus what this index's search
    // buffers already hold (reused)
    size_t avail(size_t live) const {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        return free_b + ix->sws.n + ix->spool[0].n * 4u + ix->spool[1].n * 4u - live;
    }

    // The automatic first capacity (see the policy above).
    uint32_t first_capacity() const {
        // (walks: 2^14 at fscale > 0 too — a walk's columns count, and
        // at 2^13 the few searches that outgrew it took a second pass of
        // 10% of the time: 271-280k against 245-252k q/s, r05ap)
        uint32_t c = std::min(o.fscale > 0.0 && tables ? (1u << 13) : (1u << 14), cap_max);
        const size_t budget = (size_t)(wfrac * (double)avail(0) * (c < cap_max ? 0.75 : 1.0));
        const uint64_t lanes = m ? search_slots(m) : 64u;
        while (c > (1u << 10) && lanes * search_ws_bytes_per_slot(c, tables, paths) > budget) c >>= 1;
        return c;
    }

    // The pass's arrays, its lanes and workspace, its spill pool.
    void size_pass() {
        ++passes;
        first = passes == 1;
        more = cap < cap_max;
        pq_s = first ? ix->qs.p : d_q.p;
        pq_t = first ? ix->qt.p : d_q.p + m;
        pq_r = first ? ix->qrow.p : d_q.p + 2ull * m;
        p_cost = first ? ix->cost.p : d_cost.p;
        p_hops = first ? ix->hops.p : d_hops.p;
        p_fin = first ? ix->fin.p : d_fin.p;
        p_st = first ? ix->qstats.p : d_st.p;
        p_agg = first ? ix->sagg.p : d_agg.p;
        if (paths)
            pa = SearchPathsArgs{ix->spp_pool.p,
                                 ix->spp_top.p,
                                 pool_entries,
                                 first ? ix->spp_off.p : d_poff.p,
                                 first ? ix->spp_pn.p : d_pn.p,
                                 first ? ix->spp_vcol.p : d_vcol.p,
                                 first ? ix->spp_vlw.p : d_vlw.p};
        // lanes: as many as the workspace share holds (whole waves),
        // leaving a quarter of it to the spill pool when a later pass
        // can resume; the pool takes the rest of the share
        const size_t live_in = have_resume ? ix->spool[pin].n * 4u : 0u;
        const size_t av = avail(live_in);
        const size_t share = (size_t)(wfrac * (double)av);
        const size_t per_slot = search_ws_bytes_per_slot(cap, tables, paths);
        // (a quarter in pass 1, a tenth later: fewer searches spill again)
        const size_t ws_budget = more ? (first ? share / 4u * 3u : share / 10u * 9u) : share;
        const uint64_t fit = ws_budget / (64ull * per_slot);
        CPD_REQUIRE(fit > 0 || av / 2 >= 64ull * per_slot, CPD_E_OOM,
                    "search workspace of 64 lanes x capacity " + std::to_string(cap) +
                        " does not fit in HBM");
        slots = (uint32_t)std::min<uint64_t>(search_slots(m), std::max<uint64_t>(1, fit) * 64u);
        if (first) lanes1 = slots;
        ix->sws.release();
        ix->sws.alloc((size_t)slots * per_slot);
        sa = SearchSpillArgs{};
        if (have_resume) {
            sa.resume = d_res.p;
            sa.rin = ix->spool[pin].p;
        }
        if (more) {
            const uint64_t want = (uint64_t)m * search_spill_words(cap, tables, paths);
            const uint64_t left = share > (size_t)slots * per_slot ? share - (size_t)slots * per_slot : 0;
            const uint64_t words = search_pool_words(std::min<uint64_t>(want, left / 4u));
            if (words >= search_spill_words(cap, tables, paths)) {
                DevBuf<uint32_t>& out = ix->spool[pin ^ 1];
                out.release();
                out.alloc(words);
                ix->sat.alloc(m);
                sa.rout = out.p;
                sa.at = ix->sat.p;
                sa.top = ix->stop.p;
                sa.cap_words = words;
                HIP_CHECK(hipMemsetAsync(ix->stop.p, 0, sizeof(unsigned long long), sm));
            }
        }
    }

    // The search kernel, a later pass's results over the first pass's, the
    // pass's sums into hp and h.
    void launch_pass() {
        HIP_CHECK(hipMemsetAsync(p_agg, 0, 8 * sizeof(unsigned long long), sm));
        Events<2> ev(g);
        HIP_CHECK(hipEventRecord(ev.e[0], sm));
        (void)hipGetLastError();
        launch_cpd_search(g->adj.p, adj_w, g->adj_shift, ix->dense.p, g->npad, g->tlb,
                          tables ? ix->hrow.p : nullptr, ix->crow.p, ix->lrow.p, g->n, pq_s, pq_t,
                          pq_r, m, o.hscale, o.fscale, o.k_moves, o.itrs, o.time_ns,
                          o.virtual_tick_ns, ix->sws.p, cap, slots, sa, p_cost, p_hops, p_fin,
                          p_st, p_agg, sm, paths ? &pa : nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev.e[1], sm));
        if (!first) {  // this pass's results over the first pass's
            launch_scatter_u64(d_cost.p, d_idx.p, m, ix->cost.p, sm);
            launch_scatter_u32(d_hops.p, d_idx.p, m, 1u, ix->hops.p, sm);
            launch_scatter_u8(d_fin.p, d_idx.p, m, ix->fin.p, sm);
            launch_scatter_u32(d_st.p, d_idx.p, m, 5u, ix->qstats.p, sm);
            if (paths) {  // each query's prefix is the one of the pass it ended in
                launch_scatter_u64(reinterpret_cast<const uint64_t*>(d_poff.p), d_idx.p, m,
                                   reinterpret_cast<uint64_t*>(ix->spp_off.p), sm);
                launch_scatter_u32(d_pn.p, d_idx.p, m, 1u, ix->spp_pn.p, sm);
                launch_scatter_u32(d_vcol.p, d_idx.p, m, 1u, ix->spp_vcol.p, sm);
                launch_scatter_u32(d_vlw.p, d_idx.p, m, 1u, ix->spp_vlw.p, sm);
            }
        }
        HIP_CHECK(hipMemcpyAsync(hp, p_agg, sizeof hp, hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipStreamSynchronize(sm));
        float pms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&pms, ev.e[0], ev.e[1]));
        ms += pms;
        for (int k = 0; k < 7; ++k) h[k] += hp[k];
        h[7] = hp[7];
        cap_last = cap;
        if (switches().search_trace)
            std::fprintf(stderr, "[cpd_search] pass %u: %u queries, capacity %u, %u lanes, "
                         "%.3f ms, %llu expanded, %llu overflowed, pool %llu words\n",
                         passes, m, cap, slots, pms, (unsigned long long)hp[0],
                         (unsigned long long)hp[7], (unsigned long long)sa.cap_words);
    }

    // The next capacity, 2x to 4x: the largest at which every search
    // left gets a lane (one round: the long searches run side by side
    // instead of waiting for lanes), else the largest at which 64
    // lanes fit (never throw there — what cannot grow
    // reports finished = 2).  With resumed searches a smaller step
    // wastes nothing.  (Fixed 4x or 2x steps lost their A/Bs, rounds 4-5.)
    // f: the pass's fin values; 0: no larger workspace fits.
    uint32_t next_capacity(const std::vector<uint8_t>& f) const {
        uint32_t next = 0;
        if (!more) return next;
        uint32_t left = 0;
        for (uint32_t i = 0; i < m; ++i) left += f[i] == 2u || f[i] == 3u;
        const size_t av2 = avail(sa.rout ? ix->spool[pin ^ 1].n * 4u : 0u);
        const double share2 = wfrac * (double)av2;
        for (uint32_t c = std::min(cap * 4u, cap_max); c > cap; c >>= 1) {
            const double per = (double)search_ws_bytes_per_slot(c, tables, paths);
            if (64.0 * per > share2) continue;
            if (!next) next = c;
            if ((double)search_slots(left) * per <= 0.9 * share2) {
                next = c;
                break;
            }
        }
        return next;
    }

    // After a pass with overflows: the searches to run again become the next
    // pass's queries, at the next capacity.  False: no larger workspace fits,
    // what overflowed is final.
    bool collect_reruns() {
        // the searches that overflowed: spilled (fin 3) resume, the others
        // (fin 2) restart from scratch — their counters leave the sums
        std::vector<uint8_t> f(m);
        std::vector<uint32_t> qst(5ull * m), hq(3ull * m);
        std::vector<unsigned long long> at(m, ~0ull);
        HIP_CHECK(hipMemcpyAsync(f.data(), p_fin, m, hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipMemcpyAsync(qst.data(), p_st, 20ull * m, hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipMemcpyAsync(hq.data(), pq_s, 4ull * m, hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipMemcpyAsync(hq.data() + m, pq_t, 4ull * m, hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipMemcpyAsync(hq.data() + 2ull * m, pq_r, 4ull * m, hipMemcpyDeviceToHost, sm));
        if (sa.rout) HIP_CHECK(hipMemcpyAsync(at.data(), ix->sat.p, 8ull * m, hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipStreamSynchronize(sm));
        const uint32_t next = next_capacity(f);
        std::vector<uint32_t> idx, sub;
        std::vector<unsigned long long> res;
        bool any_res = false;
        for (uint32_t i = 0; i < m; ++i) {
            if (f[i] != 2u && f[i] != 3u) continue;
            const bool spilled = f[i] == 3u;
            // restarted: its first pass leaves the sums — only when a
            // next pass runs it again; otherwise it ends here as an
            // overflow and its counters stay
            if (!spilled && next) {
                for (int k = 0; k < 5; ++k) h[k] -= qst[5ull * i + k];
                wasted += qst[5ull * i];
            }
            idx.push_back(i);
            res.push_back(spilled ? at[i] : ~0ull);
            any_res |= spilled;
        }
        const uint32_t m2 = (uint32_t)idx.size();
        if (!next) {
            // no larger workspace fits: spilled searches are final
            // overflows too (finished = 2, their counters in the sums)
            if (any_res) {
                for (uint32_t i = 0; i < m; ++i)
                    if (f[i] == 3u) {
                        f[i] = 2u;
                        for (int k = 0; k < 5; ++k) h[k] += qst[5ull * i + k];
                    }
                HIP_CHECK(hipMemcpyAsync(p_fin, f.data(), m, hipMemcpyHostToDevice, sm));
                if (!first) launch_scatter_u8(d_fin.p, d_idx.p, m, ix->fin.p, sm);
                HIP_CHECK(hipStreamSynchronize(sm));
            }
            return false;
        }
        reruns += m2;
        for (unsigned long long r : res) (r == ~0ull ? restarted : resumed)++;
        sub.resize(3ull * m2);
        std::vector<uint32_t> g2(m2);
        for (uint32_t j = 0; j < m2; ++j) {
            const uint32_t i = idx[j];  // target-sorted order is kept
            sub[j] = hq[i];
            sub[m2 + j] = hq[m + i];
            sub[2ull * m2 + j] = hq[2ull * m + i];
            g2[j] = first ? i : gidx[i];
        }
        gidx.swap(g2);
        d_idx.upload(gidx.data(), m2, sm);
        d_q.upload(sub.data(), 3ull * m2, sm);
        d_res.upload(res.data(), m2, sm);
        d_hops.alloc(m2);
        d_st.alloc(5ull * m2);
        d_cost.alloc(m2);
        d_fin.alloc(m2);
        d_agg.alloc(8);
        if (paths) {
            d_poff.alloc(m2);
            d_pn.alloc(m2);
            d_vcol.alloc(m2);
            d_vlw.alloc(m2);
        }
        have_resume = any_res;
        keep_spill_pool(any_res);
        m = m2;
        cap = next;
        return true;
    }

    // The pool the pass resumed from is done with; the records it wrote stay
    // for the next pass, copied to a buffer of their size when that is
    // under 9/10 of the pool.
    void keep_spill_pool(bool any_res) {
        ix->spool[pin].release();            // the records this pass resumed from
        if (any_res) {                       // the records just written, kept at their size
            unsigned long long used = 0;
            HIP_CHECK(hipMemcpy(&used, ix->stop.p, sizeof used, hipMemcpyDeviceToHost));
            DevBuf<uint32_t>& full = ix->spool[pin ^ 1];
            used = std::min<unsigned long long>(used, full.n);
            if (used < full.n / 10 * 9) {
                DevBuf<uint32_t>& fit = ix->spool[pin];
                fit.alloc(std::max<unsigned long long>(used, 1));
                HIP_CHECK(hipMemcpyAsync(fit.p, full.p, 4ull * used, hipMemcpyDeviceToDevice, sm));
                HIP_CHECK(hipStreamSynchronize(sm));
                full.release();
            } else {
                pin ^= 1;
            }
        } else {
            ix->spool[pin ^ 1].release();
        }
    }
};

void fill_search_stats(cpd_search_stats* st, const SearchPasses& p, uint32_t nq, uint32_t cap0,
                       double tables_ms) {
    st->queries = nq;
    st->expanded = p.h[0];
    st->inserted = p.h[1];
    st->touched = p.h[2];
    st->updated = p.h[3];
    st->surplus = p.h[4];
    st->plen = p.h[5];
    st->finished = p.h[6];
    st->overflow = p.h[7];
    st->kernel_ms = p.ms;
    st->lanes = p.lanes1;
    st->tables_ms = tables_ms;
    st->tables = p.tables ? CPD_SEARCH_TABLES : CPD_SEARCH_WALKS;
    st->reruns = p.reruns;
    st->resumed = p.resumed;
    st->restarted = p.restarted;
    st->wasted_expanded = p.wasted;
    st->passes = p.passes;
    st->capacity = cap0;
    st->capacity_last = p.cap_last;
}

// The automatic prefix pool (cpd_query_search_paths, prefix_bytes = 0): a
// prefix is a simple path, so 4 n bytes per query always suffice; at most
// 1/32 of the free HBM — the pool is taken before the workspace is sized, and
// every byte of it is a byte fewer for lanes.  The share is a policy, not a
// measured optimum: nobody has swept it.  What it cannot hold is reported
// with the size to ask for.
uint64_t auto_prefix_bytes(uint32_t nq, uint32_t n) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t bound = 4ull * std::max(1u, nq) * std::max(1u, n);
    return std::max<uint64_t>(256u, std::min<uint64_t>(bound, free_b / 32u));
}

// cpd_query_search; with `paths` the PATHS form (cpd_query_search_paths),
// its prefix pool of *pool_bytes (0: automatic; the size used comes back) —
// returns the pool's cursor, the prefix nodes of all queries.
uint64_t run_search(cpd_index* ix, const cpd_search_opts* opts, cpd_search_stats* st, bool paths,
                    uint64_t* pool_bytes) {
    cpd_search_opts o{1.0, 0.0, -1, -1, 0, 0, 0, CPD_SEARCH_AUTO, 0.0, 0};
    if (opts) o = *opts;
    const double wfrac = check_search_opts(ix, o);
    cpd_graph* g = ix->g;
    g->select();
    const uint32_t nq = ix->nq;
    if (!ix->dense_ready) ensure_dense(ix);
    const uint32_t* adj_w = ix->walk_adj();
    const bool tables = decide_tables(ix, o);
    const double tables_ms = build_search_tables(ix, adj_w, tables);
    uint64_t pool_entries = 0;
    if (paths) {
        // the pool at the size asked for, before the first pass is sized
        ix->spp_pool.release();
        if (!*pool_bytes) *pool_bytes = auto_prefix_bytes(nq, g->n);
        pool_entries = *pool_bytes / 4u;
        ix->spp_pool.alloc(pool_entries);
    }
    SearchPasses p(ix, o, adj_w, tables, wfrac, paths, pool_entries);
    const uint32_t cap0 = p.cap;
    while (p.m) {
        p.size_pass();
        p.launch_pass();
        if (!p.hp[7] || !p.collect_reruns()) break;
    }
    // the spill pools are scratch: freed with the pass that used them
    ix->spool[0].release();
    ix->spool[1].release();
    if (g->timing) {
        Agg& ag = g->agg["cpd_search"];
        ag.launches += p.passes;
        ag.ms += p.ms;
    }
    ix->searched = true;
    if (st) fill_search_stats(st, p, nq, cap0, tables_ms);
    unsigned long long used = 0;
    if (paths)
        HIP_CHECK(hipMemcpy(&used, ix->spp_top.p, sizeof used, hipMemcpyDeviceToHost));
    return used;
}

// The prefix pool and the per-query records are scratch of one PATHS call
// (cpd_query_search_paths, cpd_query_search_loads): freed however it ends (as
// the spill pools are), so that a later search on the index is sized from the
// same HBM as before.
struct PathsScratch {
    cpd_index* ix;
    ~PathsScratch() {
        for (DevBuf<uint32_t>* b : {&ix->spp_pool, &ix->spp_pn, &ix->spp_vcol, &ix->spp_vlw,
                                    &ix->spp_wperm})
            b->release();
        ix->spp_off.release();
        ix->spp_woff.release();
    }
};

// Every prefix of a PATHS call must have been stored: `used` nodes in a pool
// of pool_bytes.
void require_prefix_pool(const char* who, uint64_t used, uint64_t pool_bytes) {
    CPD_REQUIRE(used <= pool_bytes / 4u, CPD_E_OOM,
                std::string(who) + ": the prefixes need " + std::to_string(4ull * used) +
                    " bytes of prefix pool, " + std::to_string(pool_bytes) +
                    " were given: call again with prefix_bytes >= " + std::to_string(4ull * used));
}

}  // namespace

extern "C" {

int cpd_query_search(cpd_index* ix, const cpd_search_opts* opts, cpd_search_stats* st) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "null index");
        run_search(ix, opts, st, false, nullptr);
    });
}

int cpd_query_search_paths(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                           uint64_t* offsets, cpd_search_stats* st, cpd_search_paths_info* info) {
    return guarded([&] {
        CPD_REQUIRE(ix && offsets, CPD_E_ARG, "search paths: null argument");
        const uint32_t nq = ix->nq;
        CPD_REQUIRE(nq < 0x7FFFFFFFu, CPD_E_RANGE, "search paths: too many queries for one batch");
        ix->paths_ready = false;
        if (info) *info = cpd_search_paths_info{0, 0, 0, 0.0};
        PathsScratch scratch{ix};
        uint64_t pool_bytes = prefix_bytes;
        const uint64_t used = run_search(ix, opts, st, true, &pool_bytes);
        if (info) {
            info->prefix_nodes = used;
            info->prefix_bytes = pool_bytes;
        }
        // the search's results are whole and fetchable from here on, whatever
        // becomes of the paths
        require_prefix_pool("search paths", used, pool_bytes);
        if (!nq) {
            paths_empty(ix, offsets);
            return;
        }
        cpd_graph* g = ix->g;
        hipStream_t s = g->stream;
        if (!g->inv_d.p) g->inv_d.upload(g->inv.data(), g->n, s);
        ix->plens.alloc((size_t)nq + 1u);
        ix->poff.alloc((size_t)nq + 1u);
        ix->spp_woff.alloc(2ull * nq);
        ix->spp_wperm.alloc(nq);
        size_t scan_bytes = 0;
        HIP_CHECK(path_scan_bytes(nq, &scan_bytes));
        ix->qsort_tmp.alloc(scan_bytes);
        Events<4> ev(g);
        // offsets: pn + lw(v*) per query in the caller's order, exclusive sum
        HIP_CHECK(hipEventRecord(ev.e[0], s));
        HIP_CHECK(launch_search_path_offsets(ix->qsort_tmp.p, ix->qsort_tmp.n, ix->spp_pn.p,
                                             ix->spp_vlw.p, ix->qperm.p, nq, ix->plens.p,
                                             ix->poff.p, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev.e[1], s));
        const uint64_t total = paths_reserve(ix, "search paths");  // the index's path buffer
        // the suffixes: the table-search walk from every v* (k_moves < 0: to
        // t) into the end of its path — over the dense rows the search
        // itself used, with buffers of its own (the search's cost / hops /
        // fin stay) — then the prefixes in front
        HIP_CHECK(hipEventRecord(ev.e[2], s));
        launch_search_path_plan(ix->spp_pn.p, ix->spp_vlw.p, ix->qperm.p, ix->poff.p, nq,
                                ix->spp_woff.p, ix->spp_wperm.p, s);
        launch_table_paths_dense(g->adj.p, g->adj_shift, ix->dense.p, g->npad, g->tlb,
                                 ix->spp_vcol.p, ix->qt.p, ix->qrow.p, ix->spp_wperm.p,
                                 ix->spp_woff.p, g->inv_d.p, nq, -1, g->n, ix->pnodes.p, s);
        launch_search_path_join(ix->spp_pool.p, ix->spp_off.p, ix->spp_pn.p, ix->qperm.p,
                                ix->poff.p, g->inv_d.p, nq, ix->pnodes.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev.e[3], s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms_off = 0.f, ms_fill = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms_off, ev.e[0], ev.e[1]));
        HIP_CHECK(hipEventElapsedTime(&ms_fill, ev.e[2], ev.e[3]));
        if (g->timing) {
            Agg& ag = g->agg["search_paths"];
            ag.launches++;
            ag.ms += ms_off + ms_fill;
            // the walk's bytes are not modelled: nodes written, prefixes read
            ag.bytes += 4.0 * (double)total + 4.0 * (double)used;
        }
        if (info) {
            info->nodes = total;
            info->paths_ms = (double)ms_off + (double)ms_fill;
        }
        paths_copy_out(ix, offsets);
    });
}

int cpd_query_search_loads(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                           const uint32_t* demand, uint32_t flags, cpd_search_stats* st,
                           cpd_search_loads_info* info) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "search loads: null index");
        CPD_REQUIRE(!(flags & ~CPD_LOADS_ACCUMULATE), CPD_E_ARG,
                    "search loads: unknown flag bits " + std::to_string(flags & ~CPD_LOADS_ACCUMULATE));
        if (info) *info = cpd_search_loads_info{0, 0, 0, 0, 0.0};
        const bool keep = (flags & CPD_LOADS_ACCUMULATE) && ix->loads_ready;
        CPD_REQUIRE(!keep || !ix->ld_period, CPD_E_ARG,
                    "search loads: accumulate into the table of a timed walk (period " +
                        std::to_string(ix->ld_period) + ")");
        CPD_REQUIRE(!keep || (ix->ld_slices == 1 && ix->ld_slice_moves == 0), CPD_E_ARG,
                    "search loads: accumulate into a table of " + std::to_string(ix->ld_slices) +
                        " slices of " + std::to_string(ix->ld_slice_moves) +
                        " moves: a search loads one plane");
        cpd_graph* g = ix->g;
        require_load_slots(g, "search loads");
        const uint32_t nq = ix->nq;
        ix->paths_ready = false;
        PathsScratch scratch{ix};
        uint64_t pool_bytes = prefix_bytes;
        const uint64_t used = run_search(ix, opts, st, true, &pool_bytes);
        if (info && nq) {
            info->prefix_nodes = used;
            info->prefix_bytes = pool_bytes;
        }
        // the search's results are whole and fetchable from here on; the load
        // table is touched only once every prefix is known to be stored
        require_prefix_pool("search loads", used, pool_bytes);
        if (!keep) reset_load_table(ix, 1, 0, 0);
        if (!nq) return;
        hipStream_t s = g->stream;
        if (demand) ix->ld_demand.upload(demand, nq, s);
        const uint32_t* dem = demand ? ix->ld_demand.p : nullptr;
        // the suffix walk's cost / hops / fin go nowhere: the index's hold the
        // search's.  cnt: the walk's sums (finished, moves, cost: wave_stats),
        // then the prefix kernel's adds and its pairs without an edge
        DevBuf<uint64_t> w_cost;
        DevBuf<uint32_t> w_hops;
        DevBuf<uint8_t> w_fin;
        DevBuf<unsigned long long> cnt;
        w_cost.alloc(nq);
        w_hops.alloc(nq);
        w_fin.alloc(nq);
        cnt.alloc(5);
        HIP_CHECK(hipMemsetAsync(cnt.p, 0, 5 * sizeof(unsigned long long), s));
        const uint32_t* adj_w = ix->walk_adj();
        Events<2> ev(g);
        HIP_CHECK(hipEventRecord(ev.e[0], s));
        (void)hipGetLastError();
        launch_search_prefix_loads(adj_w, g->adj_shift, ix->spp_pool.p, ix->spp_off.p,
                                   ix->spp_pn.p, ix->qperm.p, dem, nq, g->n, ix->ld_tab.p,
                                   cnt.p + 3, s);
        // a query without a route has vcol = t: no move
        launch_table_loads_dense(adj_w, g->adj_shift, ix->dense.p, g->npad, g->tlb, ix->spp_vcol.p,
                                 ix->qt.p, ix->qrow.p, ix->qperm.p, dem, nq, -1, g->n, 1u, 0u,
                                 ix->ld_tab.p, w_cost.p, w_hops.p, w_fin.p, cnt.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev.e[1], s));
        unsigned long long h[5] = {0, 0, 0, 0, 0};
        HIP_CHECK(hipMemcpyAsync(h, cnt.p, sizeof h, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h[4]) {
            ix->loads_ready = false;  // some moves are missing from it
            throw Error(CPD_E_HIP, "search loads: internal error: " + std::to_string(h[4]) +
                                       " prefix moves name no edge of the adjacency searched");
        }
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        if (g->timing) {
            // per move one 8-B counter; the prefixes read, a row per prefix
            // move; the suffix walk's own bytes are not modelled
            Agg& ag = g->agg["search_loads"];
            ag.launches += 2;
            ag.ms += ms;
            ag.bytes += 8.0 * (double)(h[1] + h[3]) + 4.0 * (double)used +
                        8.0 * (double)((uint64_t)h[3] << g->adj_shift);
        }
        if (info) {
            info->moves = h[1] + h[3];
            info->prefix_moves = h[3];
            info->loads_ms = ms;
        }
    });
}

int cpd_query_search_counters(cpd_index* ix, uint32_t* counters) {
    return guarded([&] {
        CPD_REQUIRE(ix && counters, CPD_E_ARG, "null argument");
        ix->g->select();
        const uint32_t nq = ix->nq;
        if (!nq) return;
        CPD_REQUIRE(ix->searched && ix->qstats.n >= 5ull * nq, CPD_E_ARG,
                    "no search has run on these queries (cpd_query_prepare since, or only "
                    "table-search)");
        hipStream_t st = ix->g->stream;
        ix->qout.alloc(20ull * nq);
        launch_scatter_u32(ix->qstats.p, ix->qperm.p, nq, 5u, reinterpret_cast<uint32_t*>(ix->qout.p),
                           st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(counters, ix->qout.p, 20ull * nq, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

}  // extern "C"
