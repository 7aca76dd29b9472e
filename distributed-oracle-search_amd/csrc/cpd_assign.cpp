// Loads to weights in HBM and the loops around it (cpd_index_weights_from_loads,
// cpd_index_get_weights / _weight_sets; cpd_index_flow_step, _flow_step_conj
// and _flow_step_bi over one step routine; cpd_query_assign, _assign_line,
// _assign_conj and _assign_bi over one loop).
#include <cstddef>
#include <type_traits>

#include "assign_kernels.hpp"
#include "cpd_gpu_internal.hpp"

namespace {

// What the entry points check before anything is touched, each worded with
// the caller's name.
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

void check_complete(const cpd_index* ix, const char* who) {
    CPD_REQUIRE(ix->added == ix->nrows, CPD_E_ARG,
                std::string(who) + ": index incomplete (" + std::to_string(ix->added) + " of " +
                    std::to_string(ix->nrows) + " rows appended)");
}

void check_lambda(uint32_t lambda_q16, const char* who) {
    CPD_REQUIRE(lambda_q16 <= 65536u || lambda_q16 == CPD_STEP_LINE, CPD_E_ARG,
                std::string(who) + ": lambda_q16 " + std::to_string(lambda_q16) +
                    " is neither 0..65536 nor CPD_STEP_LINE");
}

void check_alpha(uint32_t alpha_q16, const char* who) {
    CPD_REQUIRE(alpha_q16 <= CPD_ALPHA_MAX || alpha_q16 == CPD_ALPHA_CONJ, CPD_E_ARG,
                std::string(who) + ": alpha_q16 " + std::to_string(alpha_q16) +
                    " is neither 0..64881 nor CPD_ALPHA_CONJ");
}

void check_iters(uint32_t iters, const char* who) {
    CPD_REQUIRE(iters >= 1u && iters <= 65535u, CPD_E_ARG,
                std::string(who) + ": " + std::to_string(iters) + " iterations, 1 to 65535");
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

// One timed interval into the graph's aggregate of that name (timing runs).
void add_agg(cpd_graph* g, const char* name, uint64_t launches, float ms, double bytes) {
    if (!g->timing) return;
    Agg& a = g->agg[name];
    a.launches += launches;
    a.ms += ms;
    a.bytes += bytes;
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
    // per slot and plane: a counter read, a weight written; per slot the
    // free-flow pair and the capacity
    add_agg(g, "vdf_update", 1, ms, (double)nslots * (12.0 + 12.0 * planes));
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

// A one-plane slot-order table of u64 (the loads, the flow or the target) in
// edge order, permuted on the GPU through `stage` and copied out once.
void fetch_slot_table(cpd_index* ix, const uint64_t* tab, DevBuf<uint64_t>& stage, uint64_t* out,
                      const char* who) {
    cpd_graph* g = ix->g;
    if (!g->m) return;
    CPD_REQUIRE(out, CPD_E_ARG, std::string(who) + ": null argument");
    g->select();
    hipStream_t s = g->stream;
    stage.alloc(g->m);
    (void)hipGetLastError();
    launch_loads_gather(tab, g->slot_of_edge_d.p, g->m, g->n << g->adj_shift, 1u, stage.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, stage.p, (size_t)g->m * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// A step refused by its decide kernel, nothing applied: names the first edge
// whose counter is at or above 2^bits.
[[noreturn]] void refuse_range(cpd_index* ix, const char* who, unsigned bits) {
    const uint32_t m = ix->g->m;
    std::vector<uint64_t> loads(m);
    fetch_slot_table(ix, ix->ld_tab.p, ix->ld_out, loads.data(), who);
    uint32_t e = 0;
    while (e < m && loads[e] < (1ull << bits)) ++e;
    throw Error(CPD_E_RANGE, std::string(who) + ": load " +
                                 std::to_string(e < m ? loads[e] : 0ull) + " on edge " +
                                 std::to_string(e) + " (every counter must be below 2^" +
                                 std::to_string(bits) + ")");
}

// The three steps over the flow table.
enum class Step { plain, conj, bi };
const char* step_name(Step k) {
    return k == Step::plain ? "flow step" : k == Step::conj ? "conjugate step" : "bi-conjugate step";
}

// One step over the resident one-plane table Y with the slot-order capacities
// in place, everything queued at once; the host reads the state once,
// afterwards.  The plain step (cpd_index_flow_step) is the line search's
// evaluate / decide pairs and the apply pass towards Y; it moves X without
// knowing S, so the target tables go.  The conjugate step
// (cpd_index_flow_step_conj) puts the sums, the alpha decision and the target
// pass in front and runs the same pairs and pass towards the target table S,
// over the state array grown to kConjWords; it drops S2.  The bi-conjugate step
// (cpd_index_flow_step_bi; a_q16 is nu, mu_q16 used by it alone) is the
// conjugate step without a flow table (branch 0); without a usable S2 (branch
// 1) the conjugate step whose target pass also keeps the old target in S2;
// else (branch 2) its own sums, decision and target pass over kBiWords.
// *info: a1 and b1 are the conjugate step's N and M, bi_ms its conj_ms; a
// plain step leaves alpha, the sums and bi_ms 0.
void flow_step(cpd_index* ix, const cpd_vdf& f, Step kind, uint32_t a_q16, uint32_t mu_q16,
               uint32_t lambda_q16, cpd_bi_info* info) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint64_t nslots = (uint64_t)g->n << g->adj_shift;
    const bool conj = kind != Step::plain;
    // no flow table: X = 0 and lambda = 65536 give X = Y << 16 whatever lambda
    // says (conjugate: S = X and alpha = 0 as well, so X = S = Y << 16)
    const bool init = !ix->flow_ready;
    const bool has_s = conj && !init && ix->target_ready;
    const uint32_t lp = ix->lambda_prev;
    const uint32_t branch =
        kind != Step::bi || init ? 0u : has_s && ix->target2_ready && lp != 65536u ? 2u : 1u;
    uint32_t alpha_q16 = a_q16;
    if (branch == 1u) {
        CPD_REQUIRE(a_q16 == CPD_BI_AUTO || a_q16 == 0u, CPD_E_ARG,
                    std::string(step_name(kind)) + ": nu_q16 " + std::to_string(a_q16) +
                        " without a usable second target (branch 1 takes 0 or CPD_BI_AUTO)");
        alpha_q16 = a_q16 == 0u ? 0u : CPD_ALPHA_CONJ;
    }
    const uint32_t words = kind == Step::bi ? kBiWords : conj ? kConjWords : kFlowWords;
    {
        ArenaScope carve;
        ix->fl_tab.alloc((size_t)nslots);
        if (conj) ix->tg_tab.alloc((size_t)nslots);
        if (branch) ix->tg2_tab.alloc((size_t)nslots);
        ix->fl_st.alloc(words);
        ix->adj_sel.alloc((size_t)(2u * nslots));
    }
    if (init) HIP_CHECK(hipMemsetAsync(ix->fl_tab.p, 0, (size_t)nslots * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(ix->fl_st.p, 0, words * sizeof(unsigned long long), s));
    const uint32_t want = init ? 65536u : lambda_q16;
    const uint32_t pairs = want <= 65536u ? 1u : 18u;
    const uint64_t* towards = conj ? ix->tg_tab.p : ix->ld_tab.p;  // Q16 when conj
    Events<4> ev(g);  // target passes | line search | apply; e[0] is not the plain step's
    (void)hipGetLastError();
    if (branch == 2u) {
        HIP_CHECK(hipEventRecord(ev.e[0], s));
        launch_bi_sums(ix->ld_tab.p, ix->fl_tab.p, ix->tg_tab.p, ix->tg2_tab.p, g->adj.p,
                       ix->vdf_cap.p, nslots, f, lp, ix->fl_st.p, s);
        launch_bi_decide(mu_q16, a_q16, lp, ix->fl_st.p, s);
        launch_bi_target(ix->ld_tab.p, ix->fl_tab.p, ix->tg_tab.p, ix->tg2_tab.p, nslots, true,
                         true, ix->fl_st.p, s);
        HIP_CHECK(hipGetLastError());
    } else if (conj) {
        const uint64_t* s_old = has_s ? ix->tg_tab.p : nullptr;
        HIP_CHECK(hipEventRecord(ev.e[0], s));
        launch_conj_sums(ix->ld_tab.p, ix->fl_tab.p, s_old, g->adj.p, ix->vdf_cap.p, nslots, f,
                         ix->fl_st.p, s);
        launch_conj_decide(init ? 0u : alpha_q16, ix->fl_st.p, s);
        if (branch == 1u)
            launch_bi_target(ix->ld_tab.p, ix->fl_tab.p, ix->tg_tab.p, ix->tg2_tab.p, nslots,
                             false, has_s, ix->fl_st.p, s);
        else
            launch_conj_target(ix->ld_tab.p, ix->fl_tab.p, s_old, ix->tg_tab.p, nslots,
                               ix->fl_st.p, s);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    for (uint32_t i = 0; i < pairs; ++i) {
        // `first` (the lambda = 0 pass also sums X * w(0) and takes the largest
        // Y) is the plain step's: the sums passes have done both
        launch_flow_line_eval(towards, ix->fl_tab.p, g->adj.p, ix->vdf_cap.p, nslots, f,
                              !conj && i == 0u, ix->fl_st.p, s, conj);
        launch_flow_line_decide(want, ix->fl_st.p, s);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[2], s));
    launch_flow_apply(towards, ix->fl_tab.p, g->adj.p, ix->vdf_cap.p, nslots, f, ix->adj_sel.p,
                      ix->fl_st.p, s, conj);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[3], s));
    // a shorter step's later words read as 0: they lie past the ones it copies
    static_assert(kConjN >= kFlowWords && kConjAlpha >= kFlowWords, "conjugate words overlap");
    static_assert(kBiA2 >= kConjWords && kBiBeta2 < kBiWords, "bi-conjugate words overlap");
    unsigned long long h[kBiWords] = {};
    HIP_CHECK(hipMemcpyAsync(h, ix->fl_st.p, words * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    // a counter at or above 2^47 (Y << 16 would pass 2^63) / 2^30 (the sums' terms)
    if (h[kFlowDone] != 1ull) refuse_range(ix, step_name(kind), conj ? 30u : 47u);
    if (!conj) ix->tg_tab.release();  // the step moved X without knowing S
    if (!branch) {  // ... or S1 without knowing S2
        ix->tg2_tab.release();
        ix->lambda_prev = 65536u;
    }
    if (kind == Step::bi) ix->lambda_prev = (uint32_t)h[kFlowLambda];
    ix->target_ready = conj;
    ix->target2_ready = branch != 0u;
    ix->flow_ready = true;
    ix->custom_w = true;
    ix->c_ready = false;  // the search's incumbent tables follow the weights
    float bi_ms = 0.f, line_ms = 0.f, apply_ms = 0.f;
    if (conj) HIP_CHECK(hipEventElapsedTime(&bi_ms, ev.e[0], ev.e[1]));
    HIP_CHECK(hipEventElapsedTime(&line_ms, ev.e[1], ev.e[2]));
    HIP_CHECK(hipEventElapsedTime(&apply_ms, ev.e[2], ev.e[3]));
    // the conjugate sums read Y, X, S, the free-flow pair and the capacity (36 B
    // a slot), the target pass reads Y and S (or X) and writes S (24 B); branch
    // 1 also writes S2 (8 B); branch 2's sums read S2 as well (44 B) and its
    // target pass reads Y, S1, S2 and writes S1, S2 (40 B); per evaluation and
    // slot: Y, X, the free-flow pair, the capacity (28 B); the apply also
    // writes X and the selected pair
    if (kind == Step::bi)
        add_agg(g, "bi_sums_target", 3, bi_ms,
                (double)nslots * (branch == 2u ? 84.0 : branch == 1u ? 68.0 : 60.0));
    else if (conj)
        add_agg(g, "conj_sums_target", 3, bi_ms, (double)nslots * 60.0);
    add_agg(g, "flow_line_eval", h[kFlowEvals], line_ms,
            (double)nslots * 28.0 * (double)h[kFlowEvals]);
    add_agg(g, "flow_apply", 1, apply_ms, (double)nslots * 44.0);
    *info = cpd_bi_info{};
    info->branch = branch;
    info->lambda_prev_q16 = lp;
    info->lambda_q16 = (uint32_t)h[kFlowLambda];
    if (!init) {  // the initialising step reports no evaluation and no sums
        info->evals = (uint32_t)h[kFlowEvals];
        info->a1_lo = h[kConjN];
        info->a1_hi = h[kConjN + 1];
        info->b1_lo = h[kConjM];
        info->b1_hi = h[kConjM + 1];
        info->a2_lo = h[kBiA2];
        info->a2_hi = h[kBiA2 + 1];
        info->b2_lo = h[kBiB2];
        info->b2_hi = h[kBiB2 + 1];
        info->gy_lo = h[kConjGy];
        info->gy_hi = h[kConjGy + 1];
        info->xw0_lo = h[kFlowXw];
        info->xw0_hi = h[kFlowXw + 1];
        info->g0_lo = h[kFlowG0];
        info->g0_hi = h[kFlowG0 + 1];
        if (branch == 2u) {
            info->mu_q16 = (uint32_t)h[kBiMu];
            info->nu_q16 = (uint32_t)h[kBiNu];
            info->beta0_q16 = (uint32_t)h[kBiBeta0];
            info->beta1_q16 = (uint32_t)h[kBiBeta1];
            info->beta2_q16 = (uint32_t)h[kBiBeta2];
        } else {
            info->alpha_q16 = (uint32_t)h[kConjAlpha];
            if (branch == 1u) {  // the conjugate target in the bi-conjugate step's terms
                info->beta0_q16 = 65536u - info->alpha_q16;
                info->beta1_q16 = info->alpha_q16;
            }
        }
    }
    info->tstt_lo = h[kFlowTstt];
    info->tstt_hi = h[kFlowTstt + 1];
    info->changed = h[kFlowTstt + 2];
    info->bi_ms = bi_ms;
    info->line_ms = line_ms;
    info->apply_ms = apply_ms;
}

void check_bi(uint32_t v, const char* name, const char* who) {
    CPD_REQUIRE(v <= CPD_BI_MAX || v == CPD_BI_AUTO, CPD_E_ARG,
                std::string(who) + ": " + name + " " + std::to_string(v) +
                    " is neither 0..8388607 nor CPD_BI_AUTO");
}

// cpd_index_flow_step / _flow_step_conj / _flow_step_bi: the checks, the
// capacities, one step.
void checked_step(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f, Step kind,
                  uint32_t a_q16, uint32_t mu_q16, uint32_t lambda_q16, cpd_bi_info* info) {
    const char* who = step_name(kind);
    CPD_REQUIRE(ix, CPD_E_ARG, std::string(who) + ": null index");
    check_vdf(f, false, who);
    if (kind == Step::conj) check_alpha(a_q16, who);
    if (kind == Step::bi) {
        check_bi(mu_q16, "mu_q16", who);
        check_bi(a_q16, "nu_q16", who);
    }
    check_lambda(lambda_q16, who);
    check_complete(ix, who);
    check_flow_table(ix, who);
    check_capacity(ix, capacity, who);
    ix->g->select();
    upload_capacity(ix, capacity);
    flow_step(ix, *f, kind, a_q16, mu_q16, lambda_q16, info);
}

cpd_conj_info conj_info_of(const cpd_bi_info& b) {
    cpd_conj_info c{};
    c.alpha_q16 = b.alpha_q16;
    c.lambda_q16 = b.lambda_q16;
    c.evals = b.evals;
    c.n_lo = b.a1_lo;
    c.n_hi = b.a1_hi;
    c.m_lo = b.b1_lo;
    c.m_hi = b.b1_hi;
    c.gy_lo = b.gy_lo;
    c.gy_hi = b.gy_hi;
    c.xw0_lo = b.xw0_lo;
    c.xw0_hi = b.xw0_hi;
    c.g0_lo = b.g0_lo;
    c.g0_hi = b.g0_hi;
    c.tstt_lo = b.tstt_lo;
    c.tstt_hi = b.tstt_hi;
    c.changed = b.changed;
    c.conj_ms = b.bi_ms;
    c.line_ms = b.line_ms;
    c.apply_ms = b.apply_ms;
    return c;
}

// The four rules of the assignment loop.
enum class Rule { msa, line, conj, bi };
const char* const kLoopName[] = {"assign", "assign line", "assign conj", "assign bi"};

// An error of iteration k >= 2: the k - 1 before it stand.
Error iteration_failed(int code, Rule rule, uint32_t k, uint32_t iters, const std::string& why) {
    return Error(code, std::string(kLoopName[(int)rule]) + ": iteration " + std::to_string(k) +
                           " of " + std::to_string(iters) + " failed, the " +
                           (rule == Rule::msa ? "table" : "flow table") +
                           " and weights are those of " + std::to_string(k - 1) +
                           " iterations: " + why);
}

// One round's loading: cpd_query_search_loads under the current weights — MSA
// adds to the table of the rounds before (flags), the flow rules load afresh —
// then, once the first has succeeded, the capacities uploaded (cap_ms) and for
// the flow rules (reset_flow) the flow state dropped; sptt into h.
void loading_round(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                   const uint32_t* demand, const uint32_t* capacity, Rule rule, uint32_t k,
                   uint32_t iters, uint32_t flags, bool reset_flow, cpd_search_stats& ss,
                   cpd_search_loads_info& li, unsigned long long (&h)[3], float& cap_ms) {
    cpd_graph* g = ix->g;
    hipStream_t s = g->stream;
    const uint32_t nq = ix->nq;
    const int rc = cpd_query_search_loads(ix, opts, prefix_bytes, demand, flags, &ss, &li);
    if (rc != CPD_OK) {
        const std::string why = cpd_last_error();
        if (k == 1) throw Error(rc, why);  // nothing has changed
        throw iteration_failed(rc, rule, k, iters, why);
    }
    if (k == 1) {
        if (reset_flow) {  // the loop starts from an empty flow table
            ix->flow_ready = false;
            ix->target_ready = false;
            ix->target2_ready = false;
            ix->lambda_prev = 65536u;
        }
        Events<2> ev(g);
        HIP_CHECK(hipEventRecord(ev.e[0], s));
        upload_capacity(ix, capacity);
        HIP_CHECK(hipEventRecord(ev.e[1], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipEventElapsedTime(&cap_ms, ev.e[0], ev.e[1]));
    }
    // sptt over the search's cost / finished (sorted order; the demand as
    // search_loads uploaded it, read through qperm)
    HIP_CHECK(hipMemsetAsync(ix->vdf_acc.p, 0, 3 * sizeof(unsigned long long), s));
    (void)hipGetLastError();
    launch_sptt_reduce(ix->cost.p, ix->fin.p, ix->qperm.p, demand && nq ? ix->ld_demand.p : nullptr,
                       nq, ix->vdf_acc.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h, ix->vdf_acc.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// A caller's record is the leading fields of cpd_assign_conj_iter, which the
// loop fills: cpd_assign_iter, then cpd_assign_line_iter's tail, then its own.
#define SAME_PLACE(A, field) \
    static_assert(offsetof(A, field) == offsetof(cpd_assign_conj_iter, field), #A "." #field)
#define SAME_PLACES(A)                                                                   \
    SAME_PLACE(A, finished); SAME_PLACE(A, sptt_lo); SAME_PLACE(A, sptt_hi);             \
    SAME_PLACE(A, tstt_lo); SAME_PLACE(A, tstt_hi); SAME_PLACE(A, moves);                \
    SAME_PLACE(A, changed); SAME_PLACE(A, search_ms); SAME_PLACE(A, loads_ms);           \
    SAME_PLACE(A, vdf_ms)
SAME_PLACES(cpd_assign_iter);
SAME_PLACES(cpd_assign_line_iter);
SAME_PLACE(cpd_assign_line_iter, lambda_q16);
SAME_PLACE(cpd_assign_line_iter, evals);
SAME_PLACE(cpd_assign_line_iter, g0_lo);
SAME_PLACE(cpd_assign_line_iter, g0_hi);
SAME_PLACE(cpd_assign_line_iter, xw0_lo);
SAME_PLACE(cpd_assign_line_iter, xw0_hi);
SAME_PLACE(cpd_assign_line_iter, line_ms);
#undef SAME_PLACES
#undef SAME_PLACE
static_assert(sizeof(cpd_assign_iter) == offsetof(cpd_assign_conj_iter, lambda_q16) &&
                  sizeof(cpd_assign_line_iter) == offsetof(cpd_assign_conj_iter, alpha_q16),
              "a shorter record ends where the next one's own fields begin");
// cpd_assign_bi_iter has its own tail after cpd_assign_line_iter's fields
static_assert(sizeof(cpd_assign_line_iter) == offsetof(cpd_assign_bi_iter, branch),
              "the bi-conjugate record's tail begins where cpd_assign_line_iter ends");

// cpd_query_assign, _assign_line, _assign_conj and _assign_bi.  Every
// iteration: a loading and sptt (loading_round), then the rule's update — MSA
// turns the summed table over k into weights (apply_vdf; no flow state, no
// early stop, its errors not wrapped), the others take a line-search step,
// plain, conjugate or bi-conjugate (flow_step).  The loop fills a
// cpd_assign_conj_iter and the bi-conjugate step's info; the bi-conjugate
// record takes the former's cpd_assign_line_iter part and its own tail from
// the latter.  done: null for MSA, which always makes `iters`.
template <class Rec>
void assign_loop(Rule rule, cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                 const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f, uint32_t iters,
                 Rec* out, uint32_t* done) {
    constexpr bool bi_rec = std::is_same<Rec, cpd_assign_bi_iter>::value;
    static_assert(bi_rec || sizeof(Rec) <= sizeof(cpd_assign_conj_iter), "not a loop record");
    const char* who = kLoopName[(int)rule];
    const bool msa = rule == Rule::msa;
    CPD_REQUIRE(ix && out && (done || msa), CPD_E_ARG, std::string(who) + ": null argument");
    check_iters(iters, who);
    check_vdf(f, false, who);
    check_complete(ix, who);
    check_capacity(ix, capacity, who);
    for (uint32_t k = 0; k < iters; ++k) out[k] = Rec{};
    if (done) *done = 0;
    ix->g->select();
    const uint32_t nq = ix->nq;
    float cap_ms = 0.f;    // the capacity upload, in record 1
    bool restart = false;  // the last (bi-)conjugate direction went nowhere
    for (uint32_t k = 1; k <= iters; ++k) {
        cpd_search_stats ss{};
        cpd_search_loads_info li{};
        unsigned long long h[3] = {0, 0, 0};
        loading_round(ix, opts, prefix_bytes, demand, capacity, rule, k, iters,
                      msa && k > 1 ? CPD_LOADS_ACCUMULATE : 0u, !msa, ss, li, h, cap_ms);
        cpd_assign_conj_iter r{};
        cpd_bi_info ci{};
        if (msa) {
            cpd_vdf fk = *f;
            fk.load_div = k;
            cpd_vdf_info vi{};
            apply_vdf(ix, fk, &vi);
            r.tstt_lo = vi.tstt_lo;
            r.tstt_hi = vi.tstt_hi;
            r.changed = vi.changed;
            r.vdf_ms = vi.vdf_ms;
        } else {
            try {
                if (rule == Rule::bi)
                    flow_step(ix, *f, Step::bi, restart ? 0u : CPD_BI_AUTO,
                              restart ? 0u : CPD_BI_AUTO, CPD_STEP_LINE, &ci);
                else
                    flow_step(ix, *f, rule == Rule::conj ? Step::conj : Step::plain,
                              restart ? 0u : CPD_ALPHA_CONJ, 0u, CPD_STEP_LINE, &ci);
            } catch (const Error& e) {
                if (k == 1) throw;
                throw iteration_failed(e.code, rule, k, iters, e.what());
            }
            r.tstt_lo = ci.tstt_lo;
            r.tstt_hi = ci.tstt_hi;
            r.changed = ci.changed;
            r.vdf_ms = ci.apply_ms;
            r.lambda_q16 = ci.lambda_q16;
            r.evals = ci.evals;
            r.g0_lo = ci.g0_lo;
            r.g0_hi = ci.g0_hi;
            r.xw0_lo = ci.xw0_lo;
            r.xw0_hi = ci.xw0_hi;
            r.line_ms = ci.bi_ms + ci.line_ms;
            r.alpha_q16 = ci.alpha_q16;
            r.n_lo = ci.a1_lo;
            r.n_hi = ci.a1_hi;
            r.m_lo = ci.b1_lo;
            r.m_hi = ci.b1_hi;
            r.gy_lo = ci.gy_lo;
            r.gy_hi = ci.gy_hi;
        }
        r.finished = h[2];
        r.sptt_lo = h[0];
        r.sptt_hi = h[1];
        r.moves = li.moves;
        r.search_ms = ss.kernel_ms + ss.tables_ms;
        r.loads_ms = li.loads_ms;
        r.vdf_ms += k == 1 ? cap_ms : 0.f;
        if constexpr (bi_rec) {
            cpd_assign_bi_iter rb{};
            std::memcpy(&rb, &r, sizeof(cpd_assign_line_iter));
            rb.branch = ci.branch;
            rb.mu_q16 = ci.mu_q16;
            rb.nu_q16 = ci.nu_q16;
            rb.beta0_q16 = ci.beta0_q16;
            rb.beta1_q16 = ci.beta1_q16;
            rb.beta2_q16 = ci.beta2_q16;
            rb.alpha_q16 = ci.alpha_q16;
            rb.a1_lo = ci.a1_lo;
            rb.a1_hi = ci.a1_hi;
            rb.b1_lo = ci.b1_lo;
            rb.b1_hi = ci.b1_hi;
            rb.a2_lo = ci.a2_lo;
            rb.a2_hi = ci.a2_hi;
            rb.b2_lo = ci.b2_lo;
            rb.b2_hi = ci.b2_hi;
            rb.gy_lo = ci.gy_lo;
            rb.gy_hi = ci.gy_hi;
            out[k - 1] = rb;
        } else {
            std::memcpy(&out[k - 1], &r, sizeof(Rec));
        }
        if (msa) continue;
        *done = k;
        // lambda = 0 on a plain direction (the line rule's alpha is always 0):
        // the weights stay and the next search would repeat this one; on a
        // conjugate direction the next iteration restarts with alpha = 0 (a
        // bi-conjugate one: mu = nu = 0).  The empty batch has nothing to iterate.
        const bool aimed = r.alpha_q16 > 0u || ci.mu_q16 > 0u || ci.nu_q16 > 0u;
        if ((k >= 2u && r.lambda_q16 == 0u && !aimed) || nq == 0u) break;
        restart = r.lambda_q16 == 0u && aimed;
    }
}

}  // namespace

extern "C" {

int cpd_index_weights_from_loads(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                                 cpd_vdf_info* info) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "weights from loads: null index");
        check_vdf(f, true, "weights from loads");
        check_complete(ix, "weights from loads");
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
        assign_loop(Rule::msa, ix, opts, prefix_bytes, demand, capacity, f, iters, out, nullptr);
    });
}

int cpd_index_flow_step(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                        uint32_t lambda_q16, cpd_flow_info* info) {
    return guarded([&] {
        cpd_bi_info ci{};
        checked_step(ix, capacity, f, Step::plain, 0u, 0u, lambda_q16, &ci);
        if (!info) return;
        *info = cpd_flow_info{};
        info->lambda_q16 = ci.lambda_q16;
        info->evals = ci.evals;
        info->g0_lo = ci.g0_lo;
        info->g0_hi = ci.g0_hi;
        info->xw0_lo = ci.xw0_lo;
        info->xw0_hi = ci.xw0_hi;
        info->tstt_lo = ci.tstt_lo;
        info->tstt_hi = ci.tstt_hi;
        info->changed = ci.changed;
        info->line_ms = ci.line_ms;
        info->apply_ms = ci.apply_ms;
    });
}

int cpd_index_flow_step_conj(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                             uint32_t alpha_q16, uint32_t lambda_q16, cpd_conj_info* info) {
    return guarded([&] {
        cpd_bi_info ci{};
        checked_step(ix, capacity, f, Step::conj, alpha_q16, 0u, lambda_q16, &ci);
        if (info) *info = conj_info_of(ci);
    });
}

int cpd_index_flow_step_bi(cpd_index* ix, const uint32_t* capacity, const cpd_vdf* f,
                           uint32_t mu_q16, uint32_t nu_q16, uint32_t lambda_q16,
                           cpd_bi_info* info) {
    return guarded([&] {
        cpd_bi_info ci{};
        checked_step(ix, capacity, f, Step::bi, nu_q16, mu_q16, lambda_q16, &ci);
        if (info) *info = ci;
    });
}

int cpd_index_flow_fetch(cpd_index* ix, uint64_t* flow) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "flow fetch: null index");
        CPD_REQUIRE(ix->flow_ready, CPD_E_ARG,
                    "flow fetch: no flow table resident (cpd_index_flow_step first)");
        fetch_slot_table(ix, ix->fl_tab.p, ix->fl_out, flow, "flow fetch");
    });
}

int cpd_index_target_fetch(cpd_index* ix, uint64_t* s) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "target fetch: null index");
        CPD_REQUIRE(ix->flow_ready && ix->target_ready, CPD_E_ARG,
                    "target fetch: no target table resident (cpd_index_flow_step_conj first)");
        fetch_slot_table(ix, ix->tg_tab.p, ix->fl_out, s, "target fetch");
    });
}

int cpd_index_target2_fetch(cpd_index* ix, uint64_t* s2) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "target2 fetch: null index");
        CPD_REQUIRE(ix->flow_ready && ix->target_ready && ix->target2_ready, CPD_E_ARG,
                    "target2 fetch: no second target table resident (cpd_index_flow_step_bi "
                    "twice first)");
        fetch_slot_table(ix, ix->tg2_tab.p, ix->fl_out, s2, "target2 fetch");
    });
}

int cpd_index_flow_clear(cpd_index* ix) {
    return guarded([&] {
        CPD_REQUIRE(ix, CPD_E_ARG, "flow clear: null index");
        ix->g->select();
        ix->fl_tab.release();
        ix->fl_out.release();
        ix->tg_tab.release();
        ix->tg2_tab.release();
        ix->flow_ready = false;
        ix->target_ready = false;
        ix->target2_ready = false;
        ix->lambda_prev = 65536u;
    });
}

int cpd_query_assign_line(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                          const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                          uint32_t iters, cpd_assign_line_iter* out, uint32_t* done) {
    return guarded([&] {
        assign_loop(Rule::line, ix, opts, prefix_bytes, demand, capacity, f, iters, out, done);
    });
}

int cpd_query_assign_conj(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                          const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                          uint32_t iters, cpd_assign_conj_iter* out, uint32_t* done) {
    return guarded([&] {
        assign_loop(Rule::conj, ix, opts, prefix_bytes, demand, capacity, f, iters, out, done);
    });
}

int cpd_query_assign_bi(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                        const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                        uint32_t iters, cpd_assign_bi_iter* out, uint32_t* done) {
    return guarded([&] {
        assign_loop(Rule::bi, ix, opts, prefix_bytes, demand, capacity, f, iters, out, done);
    });
}

}  // extern "C"
