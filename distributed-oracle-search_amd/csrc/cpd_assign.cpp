// Loads to weights in HBM and the loop around it (cpd_index_weights_from_loads,
// cpd_index_get_weights / _weight_sets, cpd_query_assign).
#include "assign_kernels.hpp"
#include "cpd_gpu_internal.hpp"

namespace {

// What the entry points check before anything is touched.
void check_vdf(const cpd_vdf* f, bool with_div, const char* who) {
    const std::string w(who);
    CPD_REQUIRE(f, CPD_E_ARG, w + ": null delay function");
    CPD_REQUIRE(f->a_num <= 65535u, CPD_E_ARG,
                w + ": a_num " + std::to_string(f->a_num) + " above 65535");
    CPD_REQUIRE(f->a_den >= 1u && f->a_den <= 65535u, CPD_E_ARG,
                w + ": a_den " + std::to_string(f->a_den) + " outside 1..65535");
    CPD_REQUIRE(f->power >= 1u && f->power <= 4u, CPD_E_ARG,
                w + ": power " + std::to_string(f->power) + " outside 1..4");
    CPD_REQUIRE(!with_div || f->load_div >= 1u, CPD_E_ARG, w + ": load_div 0");
}

void check_capacity(const cpd_index* ix, const uint32_t* capacity, const char* who) {
    const std::string w(who);
    CPD_REQUIRE(capacity || ix->g->m == 0, CPD_E_ARG, w + ": null capacity");
    for (uint32_t e = 0; e < ix->g->m; ++e)
        CPD_REQUIRE(capacity[e] != 0u, CPD_E_ARG,
                    w + ": capacity 0 on edge " + std::to_string(e) + " (each must be >= 1)");
}

// The capacities to slot order.  Uploaded and permuted on every call: 4 m
// bytes and one small kernel, against keeping a copy on the index that would
// have to be compared with the caller's array before it could be trusted.
void upload_capacity(cpd_index* ix, const uint32_t* capacity) {
    cpd_graph* g = ix->g;
    ensure_slot_of_edge(g);
    {
        ArenaScope carve;
        ix->vdf_cap_in.alloc(g->m);
        ix->vdf_cap.alloc((size_t)g->n << g->adj_shift);
        ix->vdf_acc.alloc(3);
    }
    if (!g->m) return;
    HIP_CHECK(hipMemcpyAsync(ix->vdf_cap_in.p, capacity, (size_t)g->m * sizeof(uint32_t),
                             hipMemcpyHostToDevice, g->stream));
    (void)hipGetLastError();
    launch_capacity_scatter(ix->vdf_cap_in.p, g->slot_of_edge_d.p, g->m, ix->vdf_cap.p, g->stream);
    HIP_CHECK(hipGetLastError());
}

// The update over the resident table with the slot-order capacities in place:
// one plane into the current weights, K >= 2 planes into the weight sets.
void apply_vdf(cpd_index* ix, const cpd_vdf& f, cpd_vdf_info* info) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint64_t nslots = (uint64_t)g->n << g->adj_shift;
    const uint32_t planes = ix->ld_slices;
    const uint32_t kw = planes >= 2u ? weight_set_words(planes) : 0u;
    if (kw) {
        // the costs kernels take the zero record's index as u32
        CPD_REQUIRE(nslots < (1ull << 32), CPD_E_RANGE,
                    "weights from loads: more than 2^32 adjacency slots");
        if (ix->wsets.n < (nslots + 1u) * kw) ix->nsets = ix->wset_words = 0;  // made again below
        ArenaScope carve;
        ix->wsets.alloc((size_t)(nslots + 1u) * kw);
    } else {
        ArenaScope carve;
        ix->adj_sel.alloc((size_t)(2u * nslots));
    }
    HIP_CHECK(hipMemsetAsync(ix->vdf_acc.p, 0, 3 * sizeof(unsigned long long), s));
    Events<2> ev(g);
    HIP_CHECK(hipEventRecord(ev.e[0], s));
    (void)hipGetLastError();
    launch_vdf_update(ix->ld_tab.p, g->adj.p, ix->vdf_cap.p, nslots, planes, f, kw, ix->adj_sel.p,
                      ix->wsets.p, ix->vdf_acc.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    unsigned long long h[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(h, ix->vdf_acc.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (kw) {
        ix->nsets = planes;
        ix->wset_words = kw;
    } else {
        ix->custom_w = true;
        ix->c_ready = false;  // the search's incumbent tables follow the weights
    }
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    if (g->timing) {
        // per slot and plane: a counter read, a weight written; per slot the
        // free-flow pair and the capacity
        Agg& ag = g->agg["vdf_update"];
        ag.launches++;
        ag.ms += ms;
        ag.bytes += (double)nslots * (12.0 + 12.0 * planes);
    }
    if (info) {
        info->tstt_lo = h[0];
        info->tstt_hi = h[1];
        info->changed = h[2];
        info->planes = planes;
        info->vdf_ms = ms;
    }
}

// Weights in edge order out of a slot-order table (see launch_weights_gather).
void fetch_weights(cpd_index* ix, const uint32_t* src, uint32_t stride, uint32_t first,
                   uint32_t cols, uint32_t* w) {
    cpd_graph* g = ix->g;
    const size_t total = (size_t)g->m * cols;
    if (!total) return;
    g->select();
    ensure_slot_of_edge(g);
    hipStream_t s = g->stream;
    ix->vdf_out.alloc(total);
    (void)hipGetLastError();
    launch_weights_gather(src, g->slot_of_edge_d.p, g->m, stride, first, cols, ix->vdf_out.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(w, ix->vdf_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int cpd_index_weights_from_loads(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                                 cpd_vdf_info* info) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "weights from loads: null index");
        check_vdf(f, true, "weights from loads");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "weights from loads: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        CPD_REQUIRE(ix->loads_ready, CPD_E_ARG,
                    "weights from loads: no load table resident (cpd_query_loads, "
                    "cpd_query_timed or cpd_query_search_loads first)");
        check_capacity(ix, capacity, "weights from loads");
        ix->g->select();
        Events<2> ev(ix->g);
        HIP_CHECK(hipEventRecord(ev.e[0], ix->g->stream));
        upload_capacity(ix, capacity);
        HIP_CHECK(hipEventRecord(ev.e[1], ix->g->stream));
        apply_vdf(ix, *f, info);
        if (info) {  // the capacity permutation's device time belongs to the step
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
            info->vdf_ms += ms;
        }
    });
}

int cpd_index_get_weights(cpd_index* ix, uint32_t* w) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "get weights: null index");
        CPD_REQUIRE(w || ix->g->m == 0, CPD_E_ARG, "get weights: null argument");
        fetch_weights(ix, ix->custom_w ? ix->adj_sel.p : ix->g->adj.p, 2u, 1u, 1u, w);
    });
}

int cpd_index_get_weight_sets(cpd_index* ix, uint32_t* nsets, uint32_t* w) {
    return guarded([&] {
        CPD_REQUIRE(ix && nsets, CPD_E_ARG, "get weight sets: null argument");
        *nsets = ix->nsets;
        if (w && ix->nsets) fetch_weights(ix, ix->wsets.p, ix->wset_words, 0u, ix->nsets, w);
    });
}

int cpd_query_assign(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                     const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                     uint32_t iters, cpd_assign_iter* out) {
    return guarded([&] {
        CPD_REQUIRE(ix && out, CPD_E_ARG, "assign: null argument");
        CPD_REQUIRE(iters >= 1u && iters <= 65535u, CPD_E_ARG,
                    "assign: " + std::to_string(iters) + " iterations, 1 to 65535");
        check_vdf(f, false, "assign");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "assign: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        check_capacity(ix, capacity, "assign");
        for (uint32_t k = 0; k < iters; ++k) out[k] = cpd_assign_iter{};
        cpd_graph* g = ix->g;
        g->select();
        hipStream_t s = g->stream;
        const uint32_t nq = ix->nq;
        bool cap_ready = false;  // uploaded once, after the first loading succeeded
        float cap_ms = 0.f;
        for (uint32_t k = 1; k <= iters; ++k) {
            cpd_assign_iter& r = out[k - 1];
            cpd_search_stats ss{};
            cpd_search_loads_info li{};
            const int rc = cpd_query_search_loads(ix, opts, prefix_bytes, demand,
                                                  k == 1 ? 0u : CPD_LOADS_ACCUMULATE, &ss, &li);
            if (rc != CPD_OK) {
                const std::string why = cpd_last_error();
                if (k == 1) throw Error(rc, why);  // nothing has changed
                throw Error(rc, "assign: iteration " + std::to_string(k) + " of " +
                                    std::to_string(iters) + " failed, the table and weights are "
                                    "those of " + std::to_string(k - 1) + " iterations: " + why);
            }
            if (!cap_ready) {
                Events<2> ev(g);
                HIP_CHECK(hipEventRecord(ev.e[0], s));
                upload_capacity(ix, capacity);
                HIP_CHECK(hipEventRecord(ev.e[1], s));
                HIP_CHECK(hipStreamSynchronize(s));
                HIP_CHECK(hipEventElapsedTime(&cap_ms, ev.e[0], ev.e[1]));
                cap_ready = true;
            }
            // sptt over the search's cost / finished (sorted order; the demand
            // as search_loads uploaded it, read through qperm)
            HIP_CHECK(hipMemsetAsync(ix->vdf_acc.p, 0, 3 * sizeof(unsigned long long), s));
            (void)hipGetLastError();
            launch_sptt_reduce(ix->cost.p, ix->fin.p, ix->qperm.p,
                               demand && nq ? ix->ld_demand.p : nullptr, nq, ix->vdf_acc.p, s);
            HIP_CHECK(hipGetLastError());
            unsigned long long h[3] = {0, 0, 0};
            HIP_CHECK(hipMemcpyAsync(h, ix->vdf_acc.p, sizeof h, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            cpd_vdf fk = *f;
            fk.load_div = k;
            cpd_vdf_info vi{};
            apply_vdf(ix, fk, &vi);
            r.finished = h[2];
            r.sptt_lo = h[0];
            r.sptt_hi = h[1];
            r.tstt_lo = vi.tstt_lo;
            r.tstt_hi = vi.tstt_hi;
            r.moves = li.moves;
            r.changed = vi.changed;
            r.search_ms = ss.kernel_ms + ss.tables_ms;
            r.loads_ms = li.loads_ms;
            r.vdf_ms = vi.vdf_ms + (k == 1 ? cap_ms : 0.f);
        }
    });
}

}  // extern "C"
