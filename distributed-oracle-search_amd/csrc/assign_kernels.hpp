// Host-callable launchers for the gfx950 kernels in assign_kernels.hip: the
// slot-wise step from edge loads to weights (cpd_index_weights_from_loads),
// the weights' way back to edge order (cpd_index_get_weights / _weight_sets)
// the demand-weighted cost sum of a search (cpd_query_assign), the flow step,
// the conjugate step and the bi-conjugate step.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "cpd_api.h"

namespace cpd {

// cap_slot[slot_of_edge[e]] = capacity[e] for the m edges: the capacities in
// the load table's adjacency-slot order.  Slots past a column's out-degree
// are not written (the update never reads them).
void launch_capacity_scatter(const uint32_t* capacity, const uint32_t* slot_of_edge, uint32_t m,
                             uint32_t* cap_slot, hipStream_t s);

// The delay function of cpd_api.h ("The delay function") over every slot of
// `planes` planes of the load table tab (planes x nslots u64, nslots = n <<
// shift), from the free-flow adjacency adj_free ((dst, w0) per slot) and the
// slot-order capacities:
//   set_words == 0: one plane; adj_out (2 x nslots u32) gets (dst, w') per
//       slot, padding slots (dst 0xFFFFFFFF) copied from adj_free;
//   set_words == 4 or 8 (weight_set_words(planes)): wsets gets one record of
//       set_words u32 per slot, word j = w' of plane j, zeros past `planes`
//       and in padding slots, and the record of zeros after the last slot
//       (nslots + 1 records): the table launch_table_costs reads.
// acc[0], acc[1] += the low and high half of the sum of x * w' over the real
// slots of every plane (128-bit, carries exact: adds commute), acc[2] += the
// (plane, slot) pairs with w' != w0; the caller zeroes acc.
void launch_vdf_update(const uint64_t* tab, const uint32_t* adj_free, const uint32_t* cap_slot,
                       uint64_t nslots, uint32_t planes, cpd_vdf f, uint32_t set_words,
                       uint32_t* adj_out, uint32_t* wsets, unsigned long long* acc, hipStream_t s);

// out[j * m + e] = src[slot_of_edge[e] * stride + first + j], j < cols: the
// weights of a packed adjacency (stride 2, first 1, cols 1) or of a set table
// (stride = its record's words, first 0, cols = the sets) in edge order.
void launch_weights_gather(const uint32_t* src, const uint32_t* slot_of_edge, uint32_t m,
                           uint32_t stride, uint32_t first, uint32_t cols, uint32_t* out,
                           hipStream_t s);

// Over the nq sorted queries of a search (cost / fin as the search kernel left
// them, qperm[i] = the caller's index of sorted query i): acc[0], acc[1] += the
// 128-bit sum of demand[qperm[i]] (NULL: 1) * cost[i] over the queries with
// fin == 1, acc[2] += their number; the caller zeroes acc.
void launch_sptt_reduce(const uint64_t* cost, const uint8_t* fin, const uint32_t* qperm,
                        const uint32_t* demand, uint32_t nq, unsigned long long* acc,
                        hipStream_t s);

// The flow step (cpd_api.h "The flow step").  Its state is one array of
// kFlowWords u64 in device memory, zeroed by the caller before a step; the
// kernels below communicate through it alone, so a whole line search is queued
// without a host synchronise and read back once:
enum : uint32_t {
    kFlowG = 0,       // +0, +1: g(lambda) being summed (signed 128), +2 unused
    kFlowXw = 3,      // +0, +1: the sum of X * w(0) (unsigned 128), +2 unused
    kFlowMaxY = 6,    // the largest counter of Y
    kFlowTstt = 7,    // +0, +1: the sum of (X' >> 16) * w', +2: edges with w' != w0
    kFlowLo = 10,     // the bisection's bracket
    kFlowHi = 11,
    kFlowLambda = 12, // the lambda the next evaluation takes; the step once done
    kFlowDone = 13,   // 0: searching, 1: lambda is final, 2: refused (a counter >= 2^47)
    kFlowEvals = 14,  // evaluations of g made
    kFlowG0 = 15,     // +0, +1: g(0)
    kFlowPhase = 17,  // 0: g(0) is next, 1: g(65536), 2: g(mid)
    kFlowWords = 18,
    // the conjugate step's words follow the flow step's (kFlowXw and kFlowMaxY
    // are shared; kFlowDone == 2 there: a counter >= 2^30)
    kConjN = 18,      // +0, +1: N (signed 128), +2 unused
    kConjM = 21,      // +0, +1: M (unsigned 128), +2 unused
    kConjGy = 24,     // +0, +1: gy (signed 128), +2 unused
    kConjAlpha = 27,  // the alpha decided
    kConjWords = 28,
    // the bi-conjugate step's words follow (A1, B1 and gy take kConjN, kConjM
    // and kConjGy; a branch-1 step leaves the words below 0)
    kBiA2 = 28,       // +0, +1: A2 (signed 128), +2 unused
    kBiB2 = 31,       // +0, +1: B2 (signed 128), +2 unused
    kBiMu = 34,       // the mu and nu decided
    kBiNu = 35,
    kBiBeta0 = 36,    // the weights of Yq, S1 and S2 in the new target, Q16
    kBiBeta1 = 37,
    kBiBeta2 = 38,
    kBiWords = 39
};
// launch_flow_line_eval: st[kFlowG ..] += the sum over the real slots of D *
// w(lambda), D = (Y << 16) - X, lambda = st[kFlowLambda]; `first` (the lambda
// = 0 pass) also sums X * w(0) and takes the maximum of Y.  Returns at once
// when st[kFlowDone] is set.  Y, X: nslots u64 in slot order; adj_free and
// cap_slot as launch_vdf_update reads them.
// launch_flow_line_decide: one lane advances the record by the evaluation just
// made — the line rule of cpd_api.h for want > 65536, else lambda = want after
// g(0) — and zeroes st[kFlowG ..].  18 eval / decide pairs end every line
// search (g(0), g(65536), 16 halvings of 0..65536).
// launch_flow_apply: with st[kFlowDone] == 1, X <- X(lambda), adj_out <- (dst,
// w(lambda)) per real slot (padding slots copied from adj_free), st[kFlowTstt
// ..] += the sums; does nothing otherwise.
// q16_target (eval and apply): Y is a target table already in Q16 (the
// conjugate step's S), so D = Y - X; `first` is then never set.
void launch_flow_line_eval(const uint64_t* Y, const uint64_t* X, const uint32_t* adj_free,
                           const uint32_t* cap_slot, uint64_t nslots, cpd_vdf f, bool first,
                           unsigned long long* st, hipStream_t s, bool q16_target = false);
void launch_flow_line_decide(uint32_t want, unsigned long long* st, hipStream_t s);
void launch_flow_apply(const uint64_t* Y, uint64_t* X, const uint32_t* adj_free,
                       const uint32_t* cap_slot, uint64_t nslots, cpd_vdf f, uint32_t* adj_out,
                       unsigned long long* st, hipStream_t s, bool q16_target = false);

// The conjugate step (cpd_api.h "The conjugate step"), over the same state
// array grown to kConjWords, queued before the line search's pairs:
// launch_conj_sums: st[kConjN ..], st[kConjM ..], st[kConjGy ..], st[kFlowXw ..]
// += the four sums over the real slots, st[kFlowMaxY] = the largest counter of
// Y.  S: the target table (nslots u64, Q16), or nullptr when none is resident
// (S = X: N and M stay 0).
// launch_conj_decide: one lane; a counter >= 2^30 sets st[kFlowDone] = 2 (every
// later kernel of the step then does nothing), else st[kConjAlpha] = the
// header's rule over N and M (want == CPD_ALPHA_CONJ) or want itself.
// launch_conj_target: with st[kFlowDone] == 0, S[i] = Yq + floor(alpha * (S_old
// - Yq) / 2^16) on every slot; S_old may be S (in place) or nullptr (the old
// target is X).
void launch_conj_sums(const uint64_t* Y, const uint64_t* X, const uint64_t* S,
                      const uint32_t* adj_free, const uint32_t* cap_slot, uint64_t nslots,
                      cpd_vdf f, unsigned long long* st, hipStream_t s);
void launch_conj_decide(uint32_t want, unsigned long long* st, hipStream_t s);
void launch_conj_target(const uint64_t* Y, const uint64_t* X, const uint64_t* S_old, uint64_t* S,
                        uint64_t nslots, const unsigned long long* st, hipStream_t s);

// The bi-conjugate step (cpd_api.h "The bi-conjugate step"), over the same
// state array grown to kBiWords.  Branch 2 queues the three launches below in
// front of the line search's pairs; branch 1 queues launch_conj_sums and
// launch_conj_decide and then launch_bi_target with beta == false.
// launch_bi_sums: st[kConjN ..] += A1, st[kConjM ..] += B1, st[kBiA2 ..] += A2,
// st[kBiB2 ..] += B2, st[kConjGy ..] += gy, st[kFlowXw ..] += xw0 over the real
// slots, st[kFlowMaxY] = the largest counter of Y, in one pass.  S1, S2: the
// two target tables (nslots u64, Q16); lp: lambda_prev, below 65536.
// launch_bi_decide: one lane; a counter >= 2^30 sets st[kFlowDone] = 2 (every
// later kernel of the step then does nothing), else st[kBiMu], st[kBiNu] = the
// header's rules over the sums (want == CPD_BI_AUTO) or want itself, and
// st[kBiBeta0 .. kBiBeta2] from them.
// launch_bi_target: with st[kFlowDone] == 0, per slot S2 <- the old target and
// S1 <- the new one, in place.  beta: the old target is S1 and the new one
// floor((beta0 * Yq + beta1 * S1 + beta2 * S2) / 2^16) with the betas of st;
// else the conjugate step's: the old target is S1, or X when has_s1 is false,
// and the new one Yq + floor(alpha * (old - Yq) / 2^16), alpha = st[kConjAlpha].
void launch_bi_sums(const uint64_t* Y, const uint64_t* X, const uint64_t* S1, const uint64_t* S2,
                    const uint32_t* adj_free, const uint32_t* cap_slot, uint64_t nslots, cpd_vdf f,
                    uint32_t lp, unsigned long long* st, hipStream_t s);
void launch_bi_decide(uint32_t want_mu, uint32_t want_nu, uint32_t lp, unsigned long long* st,
                      hipStream_t s);
void launch_bi_target(const uint64_t* Y, const uint64_t* X, uint64_t* S1, uint64_t* S2,
                      uint64_t nslots, bool beta, bool has_s1, const unsigned long long* st,
                      hipStream_t s);

}  // namespace cpd
