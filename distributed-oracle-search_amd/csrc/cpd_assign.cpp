// Loads to weights in HBM and the loops around it (cpd_index_weights_from_loads,
// cpd_index_get_weights / _weight_sets, cpd_query_assign; the flow step and the
// conjugate step with cpd_query_assign_line / _assign_conj).
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

// What the flow step asks of the resident load table.
void check_flow_table(const cpd_index* ix, const char* who) {
    const std::string w(who);
    CPD_REQUIRE(ix->loads_ready, CPD_E_ARG,
                w + ": no load table resident (cpd_query_loads with nslices = 1 or "
                    "cpd_query_search_loads first)");
    CPD_REQUIRE(ix->ld_period == 0, CPD_E_ARG,
                w + ": the resident load table is a timed walk's (period " +
                    std::to_string(ix->ld_period) + "), the flow step needs one plane");
    CPD_REQUIRE(ix->ld_slices == 1u, CPD_E_ARG,
                w + ": the resident load table has " + std::to_string(ix->ld_slices) +
                    " slices, the flow step needs one plane");
}

// A step refused by its decide kernel, nothing applied: names the first edge
// whose counter is at or above 2^bits.
[[noreturn]] void refuse_range(cpd_index* ix, const char* who, unsigned bits) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    std::vector<uint64_t> loads(g->m);
    ix->ld_out.alloc(g->m);
    (void)hipGetLastError();
    launch_loads_gather(ix->ld_tab.p, g->slot_of_edge_d.p, g->m, g->n << g->adj_shift, 1u,
                        ix->ld_out.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(loads.data(), ix->ld_out.p, (size_t)g->m * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint32_t e = 0;
    while (e < g->m && loads[e] < (1ull << bits)) ++e;
    throw Error(CPD_E_RANGE, std::string(who) + ": load " +
                                 std::to_string(e < g->m ? loads[e] : 0ull) + " on edge " +
                                 std::to_string(e) + " (every counter must be below 2^" +
                                 std::to_string(bits) + ")");
}

// The flow step over the resident one-plane table with the slot-order
// capacities in place: every evaluate / decide pair of the line search and the
// apply pass are queued at once; the host reads the state once, afterwards.
void flow_step(cpd_index* ix, const cpd_vdf& f, uint32_t lambda_q16, cpd_flow_info* info) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint64_t nslots = (uint64_t)g->n << g->adj_shift;
    const bool init = !ix->flow_ready;  // no flow table: X = Y << 16 whatever lambda says
    {
        ArenaScope carve;
        ix->fl_tab.alloc((size_t)nslots);
        ix->fl_st.alloc(kFlowWords);
        ix->adj_sel.alloc((size_t)(2u * nslots));
    }
    if (init) HIP_CHECK(hipMemsetAsync(ix->fl_tab.p, 0, (size_t)nslots * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(ix->fl_st.p, 0, kFlowWords * sizeof(unsigned long long), s));
    const uint32_t want = init ? 65536u : lambda_q16;
    const uint32_t pairs = want <= 65536u ? 1u : 18u;
    Events<3> ev(g);
    HIP_CHECK(hipEventRecord(ev.e[0], s));
    (void)hipGetLastError();
    for (uint32_t i = 0; i < pairs; ++i) {
        launch_flow_line_eval(ix->ld_tab.p, ix->fl_tab.p, g->adj.p, ix->vdf_cap.p, nslots, f,
                              i == 0u, ix->fl_st.p, s);
        launch_flow_line_decide(want, ix->fl_st.p, s);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    launch_flow_apply(ix->ld_tab.p, ix->fl_tab.p, g->adj.p, ix->vdf_cap.p, nslots, f,
                      ix->adj_sel.p, ix->fl_st.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[2], s));
    unsigned long long h[kFlowWords] = {};
    HIP_CHECK(hipMemcpyAsync(h, ix->fl_st.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h[kFlowDone] != 1ull) refuse_range(ix, "flow step", 47u);
    ix->tg_tab.release();  // the step moved X without knowing S
    ix->target_ready = false;
    ix->flow_ready = true;
    ix->custom_w = true;
    ix->c_ready = false;  // the search's incumbent tables follow the weights
    float line_ms = 0.f, apply_ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&line_ms, ev.e[0], ev.e[1]));
    HIP_CHECK(hipEventElapsedTime(&apply_ms, ev.e[1], ev.e[2]));
    if (g->timing) {
        // per evaluation and slot: Y, X, the free-flow pair, the capacity (28
        // B); the apply also writes X and the selected pair
        Agg& ae = g->agg["flow_line_eval"];
        ae.launches += h[kFlowEvals];
        ae.ms += line_ms;
        ae.bytes += (double)nslots * 28.0 * (double)h[kFlowEvals];
        Agg& aa = g->agg["flow_apply"];
        aa.launches++;
        aa.ms += apply_ms;
        aa.bytes += (double)nslots * 44.0;
    }
    if (info) {
        *info = cpd_flow_info{};
        info->lambda_q16 = (uint32_t)h[kFlowLambda];
        if (!init) {  // the initialising step reports no evaluation
            info->evals = (uint32_t)h[kFlowEvals];
            info->g0_lo = h[kFlowG0];
            info->g0_hi = h[kFlowG0 + 1];
            info->xw0_lo = h[kFlowXw];
            info->xw0_hi = h[kFlowXw + 1];
        }
        info->tstt_lo = h[kFlowTstt];
        info->tstt_hi = h[kFlowTstt + 1];
        info->changed = h[kFlowTstt + 2];
        info->line_ms = line_ms;
        info->apply_ms = apply_ms;
    }
}

// The conjugate step, queued like the flow step: the sums, the alpha decision
// and the target pass, then the line search and the apply pass against the
// target table; the host reads the state once, afterwards.
void conj_step(cpd_index* ix, const cpd_vdf& f, uint32_t alpha_q16, uint32_t lambda_q16,
               cpd_conj_info* info) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint64_t nslots = (uint64_t)g->n << g->adj_shift;
    // no flow table: X = 0, S = X, alpha = 0 and lambda = 65536 give X = S = Y << 16
    const bool init = !ix->flow_ready;
    const bool has_s = !init && ix->target_ready;
    {
        ArenaScope carve;
        ix->fl_tab.alloc((size_t)nslots);
        ix->tg_tab.alloc((size_t)nslots);
        ix->fl_st.alloc(kConjWords);
        ix->adj_sel.alloc((size_t)(2u * nslots));
    }
    if (init) HIP_CHECK(hipMemsetAsync(ix->fl_tab.p, 0, (size_t)nslots * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(ix->fl_st.p, 0, kConjWords * sizeof(unsigned long long), s));
    const uint32_t want = init ? 65536u : lambda_q16;
    const uint32_t pairs = want <= 65536u ? 1u : 18u;
    const uint64_t* s_old = has_s ? ix->tg_tab.p : nullptr;
    Events<4> ev(g);
    HIP_CHECK(hipEventRecord(ev.e[0], s));
    (void)hipGetLastError();
    launch_conj_sums(ix->ld_tab.p, ix->fl_tab.p, s_old, g->adj.p, ix->vdf_cap.p, nslots, f,
                     ix->fl_st.p, s);
    launch_conj_decide(init ? 0u : alpha_q16, ix->fl_st.p, s);
    launch_conj_target(ix->ld_tab.p, ix->fl_tab.p, s_old, ix->tg_tab.p, nslots, ix->fl_st.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    for (uint32_t i = 0; i < pairs; ++i) {
        launch_flow_line_eval(ix->tg_tab.p, ix->fl_tab.p, g->adj.p, ix->vdf_cap.p, nslots, f, false,
                              ix->fl_st.p, s, true);
        launch_flow_line_decide(want, ix->fl_st.p, s);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[2], s));
    launch_flow_apply(ix->tg_tab.p, ix->fl_tab.p, g->adj.p, ix->vdf_cap.p, nslots, f,
                      ix->adj_sel.p, ix->fl_st.p, s, true);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[3], s));
    unsigned long long h[kConjWords] = {};
    HIP_CHECK(hipMemcpyAsync(h, ix->fl_st.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h[kFlowDone] != 1ull) refuse_range(ix, "conjugate step", 30u);
    ix->flow_ready = true;
    ix->target_ready = true;
    ix->custom_w = true;
    ix->c_ready = false;  // the search's incumbent tables follow the weights
    float conj_ms = 0.f, line_ms = 0.f, apply_ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&conj_ms, ev.e[0], ev.e[1]));
    HIP_CHECK(hipEventElapsedTime(&line_ms, ev.e[1], ev.e[2]));
    HIP_CHECK(hipEventElapsedTime(&apply_ms, ev.e[2], ev.e[3]));
    if (g->timing) {
        // the sums read Y, X, S, the free-flow pair and the capacity (36 B a
        // slot), the target pass reads Y and S (or X) and writes S (24 B); an
        // evaluation and the apply as the flow step's
        Agg& ac = g->agg["conj_sums_target"];
        ac.launches += 3;
        ac.ms += conj_ms;
        ac.bytes += (double)nslots * 60.0;
        Agg& ae = g->agg["flow_line_eval"];
        ae.launches += h[kFlowEvals];
        ae.ms += line_ms;
        ae.bytes += (double)nslots * 28.0 * (double)h[kFlowEvals];
        Agg& aa = g->agg["flow_apply"];
        aa.launches++;
        aa.ms += apply_ms;
        aa.bytes += (double)nslots * 44.0;
    }
    if (info) {
        *info = cpd_conj_info{};
        info->lambda_q16 = (uint32_t)h[kFlowLambda];
        if (!init) {  // the initialising step reports no evaluation and no sums
            info->alpha_q16 = (uint32_t)h[kConjAlpha];
            info->evals = (uint32_t)h[kFlowEvals];
            info->n_lo = h[kConjN];
            info->n_hi = h[kConjN + 1];
            info->m_lo = h[kConjM];
            info->m_hi = h[kConjM + 1];
            info->gy_lo = h[kConjGy];
            info->gy_hi = h[kConjGy + 1];
            info->xw0_lo = h[kFlowXw];
            info->xw0_hi = h[kFlowXw + 1];
            info->g0_lo = h[kFlowG0];
            info->g0_hi = h[kFlowG0 + 1];
        }
        info->tstt_lo = h[kFlowTstt];
        info->tstt_hi = h[kFlowTstt + 1];
        info->changed = h[kFlowTstt + 2];
        info->conj_ms = conj_ms;
        info->line_ms = line_ms;
        info->apply_ms = apply_ms;
    }
}

// A flow-order table (the flow or the target) in edge order, permuted on the
// GPU and copied out once.
void fetch_slot_table(cpd_index* ix, const uint64_t* tab, uint64_t* out, const char* who) {
    cpd_graph* g = ix->g;
    if (!g->m) return;
    CPD_REQUIRE(out, CPD_E_ARG, std::string(who) + ": null argument");
    g->select();
    hipStream_t s = g->stream;
    ix->fl_out.alloc(g->m);
    (void)hipGetLastError();
    launch_loads_gather(tab, g->slot_of_edge_d.p, g->m, g->n << g->adj_shift, 1u, ix->fl_out.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, ix->fl_out.p, (size_t)g->m * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// One round of the flow-table loops (cpd_query_assign_line, _assign_conj): a
// fresh loading under the current weights, the capacities uploaded and the
// flow state dropped once the first has succeeded, and sptt into h.
void loading_round(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                   const uint32_t* demand, const uint32_t* capacity, uint32_t k, uint32_t iters,
                   const std::string& who, cpd_search_stats& ss, cpd_search_loads_info& li,
                   unsigned long long (&h)[3], float& cap_ms) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint32_t nq = ix->nq;
    const int rc = cpd_query_search_loads(ix, opts, prefix_bytes, demand, 0u, &ss, &li);
    if (rc != CPD_OK) {
        const std::string why = cpd_last_error();
        if (k == 1) throw Error(rc, why);  // nothing has changed
        throw Error(rc, who + ": iteration " + std::to_string(k) + " of " + std::to_string(iters) +
                            " failed, the flow table and weights are those of " +
                            std::to_string(k - 1) + " iterations: " + why);
    }
    if (k == 1) {
        // the loop starts from an empty flow table; the capacities are
        // uploaded once, after the first loading succeeded
        ix->flow_ready = false;
        ix->target_ready = false;
        Events<2> ev(g);
        HIP_CHECK(hipEventRecord(ev.e[0], s));
        upload_capacity(ix, capacity);
        HIP_CHECK(hipEventRecord(ev.e[1], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipEventElapsedTime(&cap_ms, ev.e[0], ev.e[1]));
    }
    HIP_CHECK(hipMemsetAsync(ix->vdf_acc.p, 0, 3 * sizeof(unsigned long long), s));
    (void)hipGetLastError();
    launch_sptt_reduce(ix->cost.p, ix->fin.p, ix->qperm.p, demand && nq ? ix->ld_demand.p : nullptr,
                       nq, ix->vdf_acc.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h, ix->vdf_acc.p, sizeof h, hipMemcpyDeviceToHost, s));
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

int cpd_index_flow_step(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                        uint32_t lambda_q16, cpd_flow_info* info) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "flow step: null index");
        check_vdf(f, false, "flow step");
        CPD_REQUIRE(lambda_q16 <= 65536u || lambda_q16 == CPD_STEP_LINE, CPD_E_ARG,
                    "flow step: lambda_q16 " + std::to_string(lambda_q16) +
                        " is neither 0..65536 nor CPD_STEP_LINE");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "flow step: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        check_flow_table(ix, "flow step");
        check_capacity(ix, capacity, "flow step");
        ix->g->select();
        upload_capacity(ix, capacity);
        flow_step(ix, *f, lambda_q16, info);
    });
}

int cpd_index_flow_step_conj(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                             uint32_t alpha_q16, uint32_t lambda_q16, cpd_conj_info* info) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "conjugate step: null index");
        check_vdf(f, false, "conjugate step");
        CPD_REQUIRE(alpha_q16 <= CPD_ALPHA_MAX || alpha_q16 == CPD_ALPHA_CONJ, CPD_E_ARG,
                    "conjugate step: alpha_q16 " + std::to_string(alpha_q16) +
                        " is neither 0..64881 nor CPD_ALPHA_CONJ");
        CPD_REQUIRE(lambda_q16 <= 65536u || lambda_q16 == CPD_STEP_LINE, CPD_E_ARG,
                    "conjugate step: lambda_q16 " + std::to_string(lambda_q16) +
                        " is neither 0..65536 nor CPD_STEP_LINE");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "conjugate step: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        check_flow_table(ix, "conjugate step");
        check_capacity(ix, capacity, "conjugate step");
        ix->g->select();
        upload_capacity(ix, capacity);
        conj_step(ix, *f, alpha_q16, lambda_q16, info);
    });
}

int cpd_index_flow_fetch(cpd_index* ix, uint64_t* flow) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "flow fetch: null index");
        CPD_REQUIRE(ix->flow_ready, CPD_E_ARG,
                    "flow fetch: no flow table resident (cpd_index_flow_step first)");
        fetch_slot_table(ix, ix->fl_tab.p, flow, "flow fetch");
    });
}

int cpd_index_target_fetch(cpd_index* ix, uint64_t* s) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "target fetch: null index");
        CPD_REQUIRE(ix->flow_ready && ix->target_ready, CPD_E_ARG,
                    "target fetch: no target table resident (cpd_index_flow_step_conj first)");
        fetch_slot_table(ix, ix->tg_tab.p, s, "target fetch");
    });
}

int cpd_index_flow_clear(cpd_index* ix) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "flow clear: null index");
        ix->g->select();
        ix->fl_tab.release();
        ix->fl_out.release();
        ix->tg_tab.release();
        ix->flow_ready = false;
        ix->target_ready = false;
    });
}

int cpd_query_assign_line(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                          const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                          uint32_t iters, cpd_assign_line_iter* out, uint32_t* done) {
    return guarded([&] {
        CPD_REQUIRE(ix && out && done, CPD_E_ARG, "assign line: null argument");
        CPD_REQUIRE(iters >= 1u && iters <= 65535u, CPD_E_ARG,
                    "assign line: " + std::to_string(iters) + " iterations, 1 to 65535");
        check_vdf(f, false, "assign line");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "assign line: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        check_capacity(ix, capacity, "assign line");
        for (uint32_t k = 0; k < iters; ++k) out[k] = cpd_assign_line_iter{};
        *done = 0;
        ix->g->select();
        const uint32_t nq = ix->nq;
        float cap_ms = 0.f;
        for (uint32_t k = 1; k <= iters; ++k) {
            cpd_assign_line_iter& r = out[k - 1];
            cpd_search_stats ss{};
            cpd_search_loads_info li{};
            unsigned long long h[3] = {0, 0, 0};
            loading_round(ix, opts, prefix_bytes, demand, capacity, k, iters, "assign line", ss, li,
                          h, cap_ms);
            cpd_flow_info fi{};
            try {
                flow_step(ix, *f, CPD_STEP_LINE, &fi);
            } catch (const Error& e) {
                if (k == 1) throw;
                throw Error(e.code, "assign line: iteration " + std::to_string(k) + " of " +
                                        std::to_string(iters) + " failed, the flow table and "
                                        "weights are those of " + std::to_string(k - 1) +
                                        " iterations: " + e.what());
            }
            r.finished = h[2];
            r.sptt_lo = h[0];
            r.sptt_hi = h[1];
            r.tstt_lo = fi.tstt_lo;
            r.tstt_hi = fi.tstt_hi;
            r.moves = li.moves;
            r.changed = fi.changed;
            r.search_ms = ss.kernel_ms + ss.tables_ms;
            r.loads_ms = li.loads_ms;
            r.vdf_ms = fi.apply_ms + (k == 1 ? cap_ms : 0.f);
            r.lambda_q16 = fi.lambda_q16;
            r.evals = fi.evals;
            r.g0_lo = fi.g0_lo;
            r.g0_hi = fi.g0_hi;
            r.xw0_lo = fi.xw0_lo;
            r.xw0_hi = fi.xw0_hi;
            r.line_ms = fi.line_ms;
            *done = k;
            // lambda = 0: the weights stay, the next search would repeat this
            // one; the empty batch has nothing to iterate
            if ((k >= 2u && fi.lambda_q16 == 0u) || nq == 0u) break;
        }
    });
}

int cpd_query_assign_conj(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                          const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                          uint32_t iters, cpd_assign_conj_iter* out, uint32_t* done) {
    return guarded([&] {
        CPD_REQUIRE(ix && out && done, CPD_E_ARG, "assign conj: null argument");
        CPD_REQUIRE(iters >= 1u && iters <= 65535u, CPD_E_ARG,
                    "assign conj: " + std::to_string(iters) + " iterations, 1 to 65535");
        check_vdf(f, false, "assign conj");
        CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                    "assign conj: index incomplete (" + std::to_string(ix->added) + " of " +
                        std::to_string(ix->nrows) + " rows appended)");
        check_capacity(ix, capacity, "assign conj");
        for (uint32_t k = 0; k < iters; ++k) out[k] = cpd_assign_conj_iter{};
        *done = 0;
        ix->g->select();
        const uint32_t nq = ix->nq;
        float cap_ms = 0.f;
        bool restart = false;  // the last conjugate direction went nowhere
        for (uint32_t k = 1; k <= iters; ++k) {
            cpd_assign_conj_iter& r = out[k - 1];
            cpd_search_stats ss{};
            cpd_search_loads_info li{};
            unsigned long long h[3] = {0, 0, 0};
            loading_round(ix, opts, prefix_bytes, demand, capacity, k, iters, "assign conj", ss, li,
                          h, cap_ms);
            cpd_conj_info ci{};
            try {
                conj_step(ix, *f, restart ? 0u : CPD_ALPHA_CONJ, CPD_STEP_LINE, &ci);
            } catch (const Error& e) {
                if (k == 1) throw;
                throw Error(e.code, "assign conj: iteration " + std::to_string(k) + " of " +
                                        std::to_string(iters) + " failed, the flow table and "
                                        "weights are those of " + std::to_string(k - 1) +
                                        " iterations: " + e.what());
            }
            r.finished = h[2];
            r.sptt_lo = h[0];
            r.sptt_hi = h[1];
            r.tstt_lo = ci.tstt_lo;
            r.tstt_hi = ci.tstt_hi;
            r.moves = li.moves;
            r.changed = ci.changed;
            r.search_ms = ss.kernel_ms + ss.tables_ms;
            r.loads_ms = li.loads_ms;
            r.vdf_ms = ci.apply_ms + (k == 1 ? cap_ms : 0.f);
            r.lambda_q16 = ci.lambda_q16;
            r.evals = ci.evals;
            r.g0_lo = ci.g0_lo;
            r.g0_hi = ci.g0_hi;
            r.xw0_lo = ci.xw0_lo;
            r.xw0_hi = ci.xw0_hi;
            r.line_ms = ci.conj_ms + ci.line_ms;
            r.alpha_q16 = ci.alpha_q16;
            r.n_lo = ci.n_lo;
            r.n_hi = ci.n_hi;
            r.m_lo = ci.m_lo;
            r.m_hi = ci.m_hi;
            r.gy_lo = ci.gy_lo;
            r.gy_hi = ci.gy_hi;
            *done = k;
            // lambda = 0 on a plain direction: the weights stay and the next
            // search would repeat this one; on a conjugate direction the next
            // iteration restarts with alpha = 0.  The empty batch has nothing
            // to iterate.
            if ((k >= 2u && ci.lambda_q16 == 0u && ci.alpha_q16 == 0u) || nq == 0u) break;
            restart = ci.lambda_q16 == 0u && ci.alpha_q16 > 0u;
        }
    });
}

}  // extern "C"
