// gfx950 kernels of the assignment loop (cpd_index_weights_from_loads,
// cpd_index_get_weights, cpd_query_assign): everything is slot-wise over
// tables already in HBM in one layout — the load table, the free-flow
// adjacency, the selected adjacency and the weight-set records all index a
// slot as (column << shift) + move — so no kernel here permutes anything but
// the capacities in and the weights out.
#include <hip/hip_runtime.h>

#include "assign_kernels.hpp"

namespace cpd {
namespace kern {

// A 128-bit unsigned sum kept as two u64 halves.
struct U128 {
    unsigned long long lo, hi;
};

__device__ __forceinline__ void add128(U128& a, unsigned long long lo, unsigned long long hi) {
    a.lo += lo;
    a.hi += hi + (a.lo < lo ? 1ull : 0ull);
}

// a += x * y, the product's high half from __umul64hi
__device__ __forceinline__ void mad128(U128& a, unsigned long long x, unsigned long long y) {
    add128(a, x * y, __umul64hi(x, y));
}

// The wave's sum in lane 0, then into acc[0] (low) and acc[1] (high): the low
// add's returned old value shows whether it wrapped, and the wrap is carried
// into the high half.  Every add commutes, so the total is exact whatever the
// order the waves arrive in.  cnt goes to acc[2] the same way.
__device__ __forceinline__ void wave_sum128(U128 a, unsigned long long cnt,
                                            unsigned long long* __restrict__ acc) {
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long lo = __shfl_down(a.lo, d, 64);
        const unsigned long long hi = __shfl_down(a.hi, d, 64);
        add128(a, lo, hi);
        cnt += __shfl_down(cnt, d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long hi = a.hi;
        if (a.lo) {
            const unsigned long long old = atomicAdd(&acc[0], a.lo);
            if (old + a.lo < old) ++hi;
        }
        if (hi) atomicAdd(&acc[1], hi);
        if (cnt) atomicAdd(&acc[2], cnt);
    }
}

// The delay function (cpd_api.h): w' of a slot with free-flow weight w0,
// capacity c >= 1 and volume x = counter / load_div.  Every intermediate fits
// 64 bits: r <= 2^20, p <= 2^32, w0 * p < 2^64, t < 2^48, t * a_num < 2^64.
__device__ __forceinline__ uint32_t vdf_weight(uint32_t w0, unsigned long long x, uint32_t c,
                                               const cpd_vdf& f) {
    if (x == 0ull) return w0;  // r = 0: nothing is added
    const unsigned long long r =
        x >= ((unsigned long long)c << 4) ? (1ull << 20) : (x << 16) / c;
    unsigned long long p = r;
    for (uint32_t i = 1; i < f.power; ++i) p = (p * r) >> 16;
    const unsigned long long t = ((unsigned long long)w0 * p) >> 16;
    const unsigned long long add = t * f.a_num / f.a_den;
    return add >= 0xFFFFFFFFull - w0 ? 0xFFFFFFFFu : w0 + (uint32_t)add;
}

__global__ __launch_bounds__(256) void capacity_scatter(const uint32_t* __restrict__ capacity,
                                                        const uint32_t* __restrict__ slot_of_edge,
                                                        uint32_t m, uint32_t* __restrict__ cap_slot) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < m) cap_slot[slot_of_edge[e]] = capacity[e];
}

// A lane per slot, grid-stride; KW = 0: the one-plane form into the selected
// adjacency, KW = 4 / 8: a weight-set record per slot and the closing record
// of zeros (slot index nslots).
template <uint32_t KW>
__global__ __launch_bounds__(256) void vdf_update(const unsigned long long* __restrict__ tab,
                                                  const uint2* __restrict__ adj_free,
                                                  const uint32_t* __restrict__ cap_slot,
                                                  unsigned long long nslots, uint32_t planes,
                                                  cpd_vdf f, uint2* __restrict__ adj_out,
                                                  uint4* __restrict__ wsets,
                                                  unsigned long long* __restrict__ acc) {
    U128 sum{0ull, 0ull};
    unsigned long long changed = 0;
    const unsigned long long end = KW ? nslots + 1ull : nslots;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < end;
         i += step) {
        uint32_t rec[KW ? KW : 1];
#pragma unroll
        for (uint32_t j = 0; j < (KW ? KW : 1u); ++j) rec[j] = 0u;
        uint2 a = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (i < nslots) a = adj_free[i];
        if (a.x != 0xFFFFFFFFu) {  // a real edge: padding slots keep their record
            const uint32_t c = cap_slot[i];
#pragma unroll
            for (uint32_t j = 0; j < (KW ? KW : 1u); ++j) {
                if (j >= planes) break;
                unsigned long long x = tab[(unsigned long long)j * nslots + i];
                if (f.load_div > 1u) x /= f.load_div;
                const uint32_t w = vdf_weight(a.y, x, c, f);
                rec[j] = w;
                mad128(sum, x, w);
                changed += w != a.y ? 1ull : 0ull;
            }
        }
        if constexpr (KW == 0u) {
            if (a.x != 0xFFFFFFFFu) a.y = rec[0];
            adj_out[i] = a;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < KW / 4u; ++q)
                wsets[i * (KW / 4u) + q] =
                    make_uint4(rec[4u * q], rec[4u * q + 1u], rec[4u * q + 2u], rec[4u * q + 3u]);
        }
    }
    wave_sum128(sum, changed, acc);
}

__global__ __launch_bounds__(256) void weights_gather(const uint32_t* __restrict__ src,
                                                      const uint32_t* __restrict__ slot_of_edge,
                                                      uint32_t m, uint32_t stride, uint32_t first,
                                                      uint32_t cols, uint32_t* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned long long)m * cols) return;
    const uint32_t j = (uint32_t)(i / m), e = (uint32_t)(i - (unsigned long long)j * m);
    out[i] = src[(unsigned long long)slot_of_edge[e] * stride + first + j];
}

__global__ __launch_bounds__(256) void sptt_reduce(const unsigned long long* __restrict__ cost,
                                                   const uint8_t* __restrict__ fin,
                                                   const uint32_t* __restrict__ qperm,
                                                   const uint32_t* __restrict__ demand, uint32_t nq,
                                                   unsigned long long* __restrict__ acc) {
    U128 sum{0ull, 0ull};
    unsigned long long finished = 0;
    const uint32_t step = gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq;
         i += step) {
        if (fin[i] != 1u) continue;
        const unsigned long long d = demand ? demand[qperm[i]] : 1ull;
        mad128(sum, d, cost[i]);
        ++finished;
    }
    wave_sum128(sum, finished, acc);
}

// --- the flow step (cpd_api.h "The flow step") -----------------------------

// a += sign(d) * |d| * w in two's complement: what wave_sum128 adds mod 2^128
__device__ __forceinline__ void mad128_signed(U128& a, long long d, unsigned long long w) {
    const unsigned long long mag = d < 0 ? 0ull - (unsigned long long)d : (unsigned long long)d;
    unsigned long long lo = mag * w, hi = __umul64hi(mag, w);
    if (d < 0) {  // minus (hi, lo)
        lo = 0ull - lo;
        hi = ~hi + (lo == 0ull ? 1ull : 0ull);
    }
    add128(a, lo, hi);
}

// X + floor(lam * d / 2^16), lam <= 65536: the product (up to 80 bits) is kept
// in two halves; for d < 0 the floor is minus the ceiling of the magnitude.
__device__ __forceinline__ unsigned long long flow_at(unsigned long long X, long long d,
                                                      unsigned long long lam) {
    const unsigned long long mag = d < 0 ? 0ull - (unsigned long long)d : (unsigned long long)d;
    unsigned long long lo = mag * lam, hi = __umul64hi(mag, lam);
    if (d < 0) {
        lo += 65535ull;
        hi += lo < 65535ull ? 1ull : 0ull;
    }
    const unsigned long long q = (lo >> 16) | (hi << 48);  // <= |d| < 2^63
    return d < 0 ? X - q : X + q;
}

// g(lambda) of the record in st (see FlowState in assign_kernels.hpp): a lane
// per slot, grid-stride.  Slots with D == 0 add nothing to g and skip the
// delay function.  first != 0 (the lambda = 0 pass): also the sum of X * w(0)
// into st[kFlowXw] and the largest counter of Y into st[kFlowMaxY].
// Q16T: Y is a target table already in Q16 (the conjugate step's S), D = Y - X.
template <bool Q16T>
__global__ __launch_bounds__(256) void flow_line_eval(const unsigned long long* __restrict__ Y,
                                                      const unsigned long long* __restrict__ X,
                                                      const uint2* __restrict__ adj_free,
                                                      const uint32_t* __restrict__ cap_slot,
                                                      unsigned long long nslots, cpd_vdf f,
                                                      uint32_t first,
                                                      unsigned long long* __restrict__ st) {
    if (st[kFlowDone] != 0ull) return;
    const unsigned long long lam = st[kFlowLambda];
    U128 g{0ull, 0ull}, xw{0ull, 0ull};
    unsigned long long ymax = 0;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += step) {
        const unsigned long long y = Y[i], x = X[i];
        if (first && y > ymax) ymax = y;
        // wraps for a counter the range check refuses: the sums are then unused
        const long long d = (long long)((Q16T ? y : y << 16) - x);
        if (d == 0 && !(first && x)) continue;
        const uint2 a = adj_free[i];
        if (a.x == 0xFFFFFFFFu) continue;  // padding: Y and X are 0 there anyway
        const unsigned long long xl = flow_at(x, d, lam);
        const uint32_t w = vdf_weight(a.y, xl >> 16, cap_slot[i], f);
        mad128_signed(g, d, w);
        if (first) mad128(xw, x, w);
    }
    wave_sum128(g, 0ull, st + kFlowG);
    if (first) {
        wave_sum128(xw, 0ull, st + kFlowXw);
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_down(ymax, d, 64);
            ymax = o > ymax ? o : ymax;
        }
        if ((threadIdx.x & 63u) == 0u && ymax) atomicMax(&st[kFlowMaxY], ymax);
    }
}

// One lane: reads g(lambda) from the accumulator, advances the record by one
// step of the line rule (or takes the caller's lambda when want <= 65536) and
// zeroes the accumulator for the next evaluation.  Plain stores from lane 0.
__global__ __launch_bounds__(64) void flow_line_decide(uint32_t want,
                                                       unsigned long long* __restrict__ st) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    if (st[kFlowDone] != 0ull) return;
    const bool neg = (long long)st[kFlowG + 1] < 0;  // g < 0
    const unsigned long long phase = st[kFlowPhase];
    st[kFlowEvals] += 1ull;
    if (phase == 0ull) {  // g(0)
        st[kFlowG0] = st[kFlowG];
        st[kFlowG0 + 1] = st[kFlowG + 1];
        if (st[kFlowMaxY] >= (1ull << 47)) {
            st[kFlowDone] = 2ull;  // refused: nothing is applied
        } else if (want <= 65536u) {
            st[kFlowLambda] = want;
            st[kFlowDone] = 1ull;
        } else if (!neg) {
            st[kFlowLambda] = 0ull;
            st[kFlowDone] = 1ull;
        } else {
            st[kFlowLambda] = 65536ull;
            st[kFlowPhase] = 1ull;
        }
    } else if (phase == 1ull) {  // g(65536)
        if (neg) {
            st[kFlowDone] = 1ull;
        } else {
            st[kFlowLo] = 0ull;
            st[kFlowHi] = 65536ull;
            st[kFlowLambda] = 32768ull;
            st[kFlowPhase] = 2ull;
        }
    } else {  // g(mid)
        unsigned long long lo = st[kFlowLo], hi = st[kFlowHi];
        if (neg) lo = st[kFlowLambda];
        else hi = st[kFlowLambda];
        st[kFlowLo] = lo;
        st[kFlowHi] = hi;
        if (hi - lo > 1ull) {
            st[kFlowLambda] = (lo + hi) >> 1;
        } else {
            st[kFlowLambda] = hi;
            st[kFlowDone] = 1ull;
        }
    }
    st[kFlowG] = st[kFlowG + 1] = st[kFlowG + 2] = 0ull;
}

// X <- X(lambda) and the selected adjacency <- (dst, w(lambda)) with the
// record's lambda; padding slots are copied from adj_free, their X left alone.
// The sum of (X >> 16) * w' and the changed count as vdf_update<0> forms them.
// Q16T as flow_line_eval's.
template <bool Q16T>
__global__ __launch_bounds__(256) void flow_apply(const unsigned long long* __restrict__ Y,
                                                  unsigned long long* __restrict__ X,
                                                  const uint2* __restrict__ adj_free,
                                                  const uint32_t* __restrict__ cap_slot,
                                                  unsigned long long nslots, cpd_vdf f,
                                                  uint2* __restrict__ adj_out,
                                                  unsigned long long* __restrict__ st) {
    if (st[kFlowDone] != 1ull) return;
    const unsigned long long lam = st[kFlowLambda];
    U128 sum{0ull, 0ull};
    unsigned long long changed = 0;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += step) {
        uint2 a = adj_free[i];
        if (a.x != 0xFFFFFFFFu) {
            const unsigned long long x = X[i];
            const unsigned long long y = Y[i];
            const long long d = (long long)((Q16T ? y : y << 16) - x);
            const unsigned long long xn = d ? flow_at(x, d, lam) : x;
            if (xn != x) X[i] = xn;
            const uint32_t w = vdf_weight(a.y, xn >> 16, cap_slot[i], f);
            mad128(sum, xn >> 16, w);
            changed += w != a.y ? 1ull : 0ull;
            a.y = w;
        }
        adj_out[i] = a;
    }
    wave_sum128(sum, changed, st + kFlowTstt);
}

// --- the conjugate step (cpd_api.h "The conjugate step") --------------------

// The slope h of the delay function at volume x, Q16 per unit volume,
// saturating.  r <= 2^20, q <= 2^28, t < 2^44, t * a_num * power < 2^62, and u
// < c << 16 < 2^48 where it is shifted.
__device__ __forceinline__ uint32_t vdf_slope(uint32_t w0, unsigned long long x, uint32_t c,
                                              const cpd_vdf& f) {
    const unsigned long long r =
        x >= ((unsigned long long)c << 4) ? (1ull << 20) : (x << 16) / c;
    unsigned long long q = f.power == 1u ? (1ull << 16) : r;
    for (uint32_t i = 2; i < f.power; ++i) q = (q * r) >> 16;
    const unsigned long long t = ((unsigned long long)w0 * q) >> 16;
    const unsigned long long u = t * f.a_num * f.power / f.a_den;
    return u >= ((unsigned long long)c << 16) ? 0xFFFFFFFFu : (uint32_t)((u << 16) / c);
}

// a += sign * |p| * |q| * h mod 2^128: the product of the magnitudes is kept in
// two halves before h multiplies it (below 2^92 in the header's range)
__device__ __forceinline__ void mad128_pqh(U128& a, long long p, long long q,
                                           unsigned long long h) {
    const unsigned long long mp = p < 0 ? 0ull - (unsigned long long)p : (unsigned long long)p;
    const unsigned long long mq = q < 0 ? 0ull - (unsigned long long)q : (unsigned long long)q;
    const unsigned long long plo = mp * mq, phi = __umul64hi(mp, mq);
    unsigned long long lo = plo * h, hi = __umul64hi(plo, h) + phi * h;
    if ((p < 0) != (q < 0)) {  // minus (hi, lo)
        lo = 0ull - lo;
        hi = ~hi + (lo == 0ull ? 1ull : 0ull);
    }
    add128(a, lo, hi);
}

// The step's four sums and the largest counter of Y: a lane per slot,
// grid-stride.  S == nullptr: no target table is resident, S is X, and N and M
// stay 0.  Slots with db == 0 skip the slope.
__global__ __launch_bounds__(256) void conj_sums(const unsigned long long* __restrict__ Y,
                                                 const unsigned long long* __restrict__ X,
                                                 const unsigned long long* __restrict__ S,
                                                 const uint2* __restrict__ adj_free,
                                                 const uint32_t* __restrict__ cap_slot,
                                                 unsigned long long nslots, cpd_vdf f,
                                                 unsigned long long* __restrict__ st) {
    U128 n{0ull, 0ull}, m{0ull, 0ull}, gy{0ull, 0ull}, xw{0ull, 0ull};
    unsigned long long ymax = 0;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += step) {
        const unsigned long long y = Y[i], x = X[i];
        if (y > ymax) ymax = y;
        // wraps for a counter the range check refuses: the sums are then unused
        const long long dy = (long long)((y << 16) - x);
        const long long ds = S ? (long long)(S[i] - x) : 0ll;
        if (dy == 0 && ds == 0 && x == 0ull) continue;
        const uint2 a = adj_free[i];
        if (a.x == 0xFFFFFFFFu) continue;  // padding: Y, X and S are 0 there anyway
        const uint32_t c = cap_slot[i];
        const long long db = ds >> 16, df = dy >> 16;  // arithmetic: the floor
        if (db) {
            const unsigned long long h = vdf_slope(a.y, x >> 16, c, f);
            mad128_pqh(n, db, df, h);
            mad128_pqh(m, db, db, h);
        }
        const uint32_t w = vdf_weight(a.y, x >> 16, c, f);
        mad128_signed(gy, dy, w);
        mad128(xw, x, w);
    }
    wave_sum128(n, 0ull, st + kConjN);
    wave_sum128(m, 0ull, st + kConjM);
    wave_sum128(gy, 0ull, st + kConjGy);
    wave_sum128(xw, 0ull, st + kFlowXw);
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_down(ymax, d, 64);
        ymax = o > ymax ? o : ymax;
    }
    if ((threadIdx.x & 63u) == 0u && ymax) atomicMax(&st[kFlowMaxY], ymax);
}

__device__ __forceinline__ U128 neg128(U128 a) {
    U128 r{0ull - a.lo, ~a.hi};
    if (r.lo == 0ull) ++r.hi;
    return r;
}

__device__ __forceinline__ bool ge128(const U128& a, const U128& b) {
    return a.hi != b.hi ? a.hi > b.hi : a.lo >= b.lo;
}

__device__ __forceinline__ U128 sub128(U128 a, const U128& b) {
    const unsigned long long borrow = a.lo < b.lo ? 1ull : 0ull;
    a.lo -= b.lo;
    a.hi -= b.hi + borrow;
    return a;
}

// One lane: refuses the step (st[kFlowDone] = 2) for a counter of Y at or
// above 2^30, else alpha from the sums by the header's rule (want ==
// CPD_ALPHA_CONJ) or the caller's.  The quotient is 16 shift-and-subtract
// steps on the magnitudes: |N| < |Dn| < 2^127 there, so the doubled remainder
// fits.  Plain stores from lane 0.
__global__ __launch_bounds__(64) void conj_decide(uint32_t want,
                                                  unsigned long long* __restrict__ st) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    if (st[kFlowMaxY] >= (1ull << 30)) {
        st[kFlowDone] = 2ull;  // refused: nothing is written
        return;
    }
    unsigned long long alpha = want;
    if (want == CPD_ALPHA_CONJ) {
        U128 n{st[kConjN], st[kConjN + 1]};
        U128 dn = sub128(n, U128{st[kConjM], st[kConjM + 1]});
        const bool nneg = (long long)n.hi < 0, dneg = (long long)dn.hi < 0;
        alpha = 0ull;
        if ((dn.lo | dn.hi) != 0ull && (n.lo | n.hi) != 0ull && nneg == dneg) {
            if (nneg) n = neg128(n);
            if (dneg) dn = neg128(dn);
            if (ge128(n, dn)) {
                alpha = CPD_ALPHA_MAX;
            } else {
                U128 rem = n;
                for (int i = 0; i < 16; ++i) {
                    rem.hi = (rem.hi << 1) | (rem.lo >> 63);
                    rem.lo <<= 1;
                    alpha <<= 1;
                    if (ge128(rem, dn)) {
                        rem = sub128(rem, dn);
                        alpha |= 1ull;
                    }
                }
                if (alpha > CPD_ALPHA_MAX) alpha = CPD_ALPHA_MAX;
            }
        }
    }
    st[kConjAlpha] = alpha;
}

// S <- Yq + floor(alpha * (S - Yq) / 2^16) on every slot once conj_decide has
// accepted the range; S_old == nullptr: no target table was resident, the old
// target is X.  Padding slots hold 0 in all three tables and get 0.
__global__ __launch_bounds__(256) void conj_target(const unsigned long long* __restrict__ Y,
                                                   const unsigned long long* __restrict__ X,
                                                   const unsigned long long* S_old,
                                                   unsigned long long* S, unsigned long long nslots,
                                                   const unsigned long long* __restrict__ st) {
    if (st[kFlowDone] != 0ull) return;
    const unsigned long long alpha = st[kConjAlpha];
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += step) {
        const unsigned long long yq = Y[i] << 16;
        const unsigned long long so = S_old ? S_old[i] : X[i];
        S[i] = flow_at(yq, (long long)(so - yq), alpha);
    }
}

// --- the bi-conjugate step (cpd_api.h "The bi-conjugate step") --------------

// The step's six sums and the largest counter of Y: a lane per slot,
// grid-stride, 44 bytes read per slot.  Slots with d1 == 0 and d2 == 0 skip the
// slope.
__global__ __launch_bounds__(256) void bi_sums(const unsigned long long* __restrict__ Y,
                                               const unsigned long long* __restrict__ X,
                                               const unsigned long long* __restrict__ S1,
                                               const unsigned long long* __restrict__ S2,
                                               const uint2* __restrict__ adj_free,
                                               const uint32_t* __restrict__ cap_slot,
                                               unsigned long long nslots, cpd_vdf f,
                                               unsigned long long lp,
                                               unsigned long long* __restrict__ st) {
    U128 a1{0ull, 0ull}, b1{0ull, 0ull}, a2{0ull, 0ull}, b2{0ull, 0ull}, gy{0ull, 0ull},
        xw{0ull, 0ull};
    unsigned long long ymax = 0;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += step) {
        const unsigned long long y = Y[i], x = X[i], s1 = S1[i], s2 = S2[i];
        if (y > ymax) ymax = y;
        if ((y | x | s1 | s2) == 0ull) continue;
        const uint2 a = adj_free[i];
        if (a.x == 0xFFFFFFFFu) continue;  // padding: all four tables are 0 there anyway
        const uint32_t c = cap_slot[i];
        // wraps for a counter the range check refuses: the sums are then unused
        const long long dy = (long long)((y << 16) - x);
        const long long d1 = (long long)(s1 - x) >> 16, df = dy >> 16;  // arithmetic: the floor
        const long long d2 = (long long)(lp * s1 + (65536ull - lp) * s2 - (x << 16)) >> 32;
        const long long e21 = (long long)(s2 - s1) >> 16;
        if (d1 | d2) {
            const unsigned long long h = vdf_slope(a.y, x >> 16, c, f);
            if (d1) {
                mad128_pqh(a1, d1, df, h);
                mad128_pqh(b1, d1, d1, h);
            }
            if (d2) {
                mad128_pqh(a2, d2, df, h);
                mad128_pqh(b2, d2, e21, h);
            }
        }
        const uint32_t w = vdf_weight(a.y, x >> 16, c, f);
        mad128_signed(gy, dy, w);
        mad128(xw, x, w);
    }
    wave_sum128(a1, 0ull, st + kConjN);
    wave_sum128(b1, 0ull, st + kConjM);
    wave_sum128(a2, 0ull, st + kBiA2);
    wave_sum128(b2, 0ull, st + kBiB2);
    wave_sum128(gy, 0ull, st + kConjGy);
    wave_sum128(xw, 0ull, st + kFlowXw);
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_down(ymax, d, 64);
        ymax = o > ymax ? o : ymax;
    }
    if ((threadIdx.x & 63u) == 0u && ymax) atomicMax(&st[kFlowMaxY], ymax);
}

// min(floor(a * 65536 / b), CPD_BI_MAX) for magnitudes a, b < 2^124, b != 0.
// The quotient reaches 2^23 exactly when a >= 128 b, that is (a >> 7) >= b;
// below that it is made bit by bit from the top bit of a down through 16
// fraction bits: the remainder stays below b, so doubled it is below 2^125.
__device__ __forceinline__ unsigned long long quot_q16(const U128& a, const U128& b) {
    const U128 a7{(a.lo >> 7) | (a.hi << 57), a.hi >> 7};
    if (ge128(a7, b)) return CPD_BI_MAX;
    const int top = a.hi ? 128 - __clzll((long long)a.hi) : a.lo ? 64 - __clzll((long long)a.lo) : 0;
    U128 rem{0ull, 0ull};
    unsigned long long q = 0;
    for (int i = top + 15; i >= 0; --i) {
        const int k = i - 16;  // the bit of a that comes down, none in the fraction
        const unsigned long long bit = k < 0 ? 0ull : k >= 64 ? (a.hi >> (k - 64)) & 1ull
                                                             : (a.lo >> k) & 1ull;
        rem.hi = (rem.hi << 1) | (rem.lo >> 63);
        rem.lo = (rem.lo << 1) | bit;
        q <<= 1;
        if (ge128(rem, b)) {
            rem = sub128(rem, b);
            q |= 1ull;
        }
    }
    return q;
}

// One lane: refuses the step (st[kFlowDone] = 2) for a counter of Y at or
// above 2^30, else mu and nu from the sums by the header's rules (want ==
// CPD_BI_AUTO) or the caller's, and the three betas.  Plain stores from lane 0.
__global__ __launch_bounds__(64) void bi_decide(uint32_t want_mu, uint32_t want_nu,
                                                unsigned long long lp,
                                                unsigned long long* __restrict__ st) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    if (st[kFlowMaxY] >= (1ull << 30)) {
        st[kFlowDone] = 2ull;  // refused: nothing is written
        return;
    }
    unsigned long long mu = want_mu, nu = want_nu;
    if (want_mu == CPD_BI_AUTO) {
        U128 a2{st[kBiA2], st[kBiA2 + 1]}, b2{st[kBiB2], st[kBiB2 + 1]};
        const bool aneg = (long long)a2.hi < 0, bneg = (long long)b2.hi < 0;
        mu = 0ull;
        if ((a2.lo | a2.hi) != 0ull && (b2.lo | b2.hi) != 0ull && aneg != bneg)
            mu = quot_q16(aneg ? neg128(a2) : a2, bneg ? neg128(b2) : b2);
    }
    if (want_nu == CPD_BI_AUTO) {
        const U128 a1{st[kConjN], st[kConjN + 1]}, b1{st[kConjM], st[kConjM + 1]};
        nu = 0ull;
        if ((b1.lo | b1.hi) != 0ull && (long long)a1.hi < 0) nu = quot_q16(neg128(a1), b1);
        nu += mu * lp / (65536ull - lp);  // mu < 2^23, lp < 2^16
        if (nu > CPD_BI_MAX) nu = CPD_BI_MAX;
    }
    const unsigned long long beta0 = (1ull << 32) / (65536ull + mu + nu);
    const unsigned long long beta2 = (mu * beta0) >> 16;
    st[kBiMu] = mu;
    st[kBiNu] = nu;
    st[kBiBeta0] = beta0;
    st[kBiBeta1] = 65536ull - beta0 - beta2;
    st[kBiBeta2] = beta2;
}

// S2 <- the old target, S1 <- the new one on every slot once the decision has
// accepted the range (see launch_bi_target).  BETA: the three-term sum is kept
// in two halves (each product is below 2^81) and shifted down once.  Padding
// slots hold 0 in every table and get 0.
template <bool BETA>
__global__ __launch_bounds__(256) void bi_target(const unsigned long long* __restrict__ Y,
                                                 const unsigned long long* __restrict__ X,
                                                 unsigned long long* __restrict__ S1,
                                                 unsigned long long* __restrict__ S2,
                                                 unsigned long long nslots, uint32_t has_s1,
                                                 const unsigned long long* __restrict__ st) {
    if (st[kFlowDone] != 0ull) return;
    const unsigned long long alpha = st[kConjAlpha];
    const unsigned long long beta0 = st[kBiBeta0], beta1 = st[kBiBeta1], beta2 = st[kBiBeta2];
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += step) {
        const unsigned long long yq = Y[i] << 16;
        if constexpr (BETA) {
            const unsigned long long s1 = S1[i], s2 = S2[i];
            U128 t{0ull, 0ull};
            mad128(t, yq, beta0);
            mad128(t, s1, beta1);
            mad128(t, s2, beta2);
            S2[i] = s1;
            S1[i] = (t.lo >> 16) | (t.hi << 48);
        } else {
            const unsigned long long so = has_s1 ? S1[i] : X[i];
            S2[i] = so;
            S1[i] = flow_at(yq, (long long)(so - yq), alpha);
        }
    }
}

}  // namespace kern

namespace {
// grid-stride launches: enough workgroups of 256 to fill the device, no more
uint32_t stride_grid(unsigned long long items) {
    const unsigned long long blocks = (items + 255ull) / 256ull;
    return (uint32_t)(blocks < 1ull ? 1ull : blocks > 4096ull ? 4096ull : blocks);
}
}  // namespace

void launch_capacity_scatter(const uint32_t* capacity, const uint32_t* slot_of_edge, uint32_t m,
                             uint32_t* cap_slot, hipStream_t s) {
    if (!m) return;
    hipLaunchKernelGGL(kern::capacity_scatter, dim3((m + 255u) / 256u), dim3(256), 0, s, capacity,
                       slot_of_edge, m, cap_slot);
}

void launch_vdf_update(const uint64_t* tab, const uint32_t* adj_free, const uint32_t* cap_slot,
                       uint64_t nslots, uint32_t planes, cpd_vdf f, uint32_t set_words,
                       uint32_t* adj_out, uint32_t* wsets, unsigned long long* acc, hipStream_t s) {
    const auto* t = reinterpret_cast<const unsigned long long*>(tab);
    const auto* af = reinterpret_cast<const uint2*>(adj_free);
    auto* ao = reinterpret_cast<uint2*>(adj_out);
    auto* ws = reinterpret_cast<uint4*>(wsets);
    const dim3 grid(stride_grid(nslots + 1ull)), blk(256);
    if (set_words == 0u)
        hipLaunchKernelGGL(kern::vdf_update<0>, grid, blk, 0, s, t, af, cap_slot, nslots, planes, f,
                           ao, ws, acc);
    else if (set_words == 4u)
        hipLaunchKernelGGL(kern::vdf_update<4>, grid, blk, 0, s, t, af, cap_slot, nslots, planes, f,
                           ao, ws, acc);
    else
        hipLaunchKernelGGL(kern::vdf_update<8>, grid, blk, 0, s, t, af, cap_slot, nslots, planes, f,
                           ao, ws, acc);
}

void launch_weights_gather(const uint32_t* src, const uint32_t* slot_of_edge, uint32_t m,
                           uint32_t stride, uint32_t first, uint32_t cols, uint32_t* out,
                           hipStream_t s) {
    const unsigned long long total = (unsigned long long)m * cols;
    if (!total) return;
    hipLaunchKernelGGL(kern::weights_gather, dim3((uint32_t)((total + 255ull) / 256ull)), dim3(256),
                       0, s, src, slot_of_edge, m, stride, first, cols, out);
}

void launch_sptt_reduce(const uint64_t* cost, const uint8_t* fin, const uint32_t* qperm,
                        const uint32_t* demand, uint32_t nq, unsigned long long* acc,
                        hipStream_t s) {
    if (!nq) return;
    hipLaunchKernelGGL(kern::sptt_reduce, dim3(stride_grid(nq)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(cost), fin, qperm, demand, nq,
                       acc);
}

void launch_flow_line_eval(const uint64_t* Y, const uint64_t* X, const uint32_t* adj_free,
                           const uint32_t* cap_slot, uint64_t nslots, cpd_vdf f, bool first,
                           unsigned long long* st, hipStream_t s, bool q16_target) {
    const auto* y = reinterpret_cast<const unsigned long long*>(Y);
    const auto* x = reinterpret_cast<const unsigned long long*>(X);
    const auto* af = reinterpret_cast<const uint2*>(adj_free);
    const dim3 grid(stride_grid(nslots)), blk(256);
    if (q16_target)
        hipLaunchKernelGGL(kern::flow_line_eval<true>, grid, blk, 0, s, y, x, af, cap_slot, nslots,
                           f, first ? 1u : 0u, st);
    else
        hipLaunchKernelGGL(kern::flow_line_eval<false>, grid, blk, 0, s, y, x, af, cap_slot, nslots,
                           f, first ? 1u : 0u, st);
}

void launch_flow_line_decide(uint32_t want, unsigned long long* st, hipStream_t s) {
    hipLaunchKernelGGL(kern::flow_line_decide, dim3(1), dim3(64), 0, s, want, st);
}

void launch_flow_apply(const uint64_t* Y, uint64_t* X, const uint32_t* adj_free,
                       const uint32_t* cap_slot, uint64_t nslots, cpd_vdf f, uint32_t* adj_out,
                       unsigned long long* st, hipStream_t s, bool q16_target) {
    const auto* y = reinterpret_cast<const unsigned long long*>(Y);
    auto* x = reinterpret_cast<unsigned long long*>(X);
    const auto* af = reinterpret_cast<const uint2*>(adj_free);
    auto* ao = reinterpret_cast<uint2*>(adj_out);
    const dim3 grid(stride_grid(nslots)), blk(256);
    if (q16_target)
        hipLaunchKernelGGL(kern::flow_apply<true>, grid, blk, 0, s, y, x, af, cap_slot, nslots, f,
                           ao, st);
    else
        hipLaunchKernelGGL(kern::flow_apply<false>, grid, blk, 0, s, y, x, af, cap_slot, nslots, f,
                           ao, st);
}

void launch_conj_sums(const uint64_t* Y, const uint64_t* X, const uint64_t* S,
                      const uint32_t* adj_free, const uint32_t* cap_slot, uint64_t nslots,
                      cpd_vdf f, unsigned long long* st, hipStream_t s) {
    hipLaunchKernelGGL(kern::conj_sums, dim3(stride_grid(nslots)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(Y),
                       reinterpret_cast<const unsigned long long*>(X),
                       reinterpret_cast<const unsigned long long*>(S),
                       reinterpret_cast<const uint2*>(adj_free), cap_slot, nslots, f, st);
}

void launch_conj_decide(uint32_t want, unsigned long long* st, hipStream_t s) {
    hipLaunchKernelGGL(kern::conj_decide, dim3(1), dim3(64), 0, s, want, st);
}

void launch_conj_target(const uint64_t* Y, const uint64_t* X, const uint64_t* S_old, uint64_t* S,
                        uint64_t nslots, const unsigned long long* st, hipStream_t s) {
    hipLaunchKernelGGL(kern::conj_target, dim3(stride_grid(nslots)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(Y),
                       reinterpret_cast<const unsigned long long*>(X),
                       reinterpret_cast<const unsigned long long*>(S_old),
                       reinterpret_cast<unsigned long long*>(S), nslots, st);
}

void launch_bi_sums(const uint64_t* Y, const uint64_t* X, const uint64_t* S1, const uint64_t* S2,
                    const uint32_t* adj_free, const uint32_t* cap_slot, uint64_t nslots, cpd_vdf f,
                    uint32_t lp, unsigned long long* st, hipStream_t s) {
    hipLaunchKernelGGL(kern::bi_sums, dim3(stride_grid(nslots)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(Y),
                       reinterpret_cast<const unsigned long long*>(X),
                       reinterpret_cast<const unsigned long long*>(S1),
                       reinterpret_cast<const unsigned long long*>(S2),
                       reinterpret_cast<const uint2*>(adj_free), cap_slot, nslots, f,
                       (unsigned long long)lp, st);
}

void launch_bi_decide(uint32_t want_mu, uint32_t want_nu, uint32_t lp, unsigned long long* st,
                      hipStream_t s) {
    hipLaunchKernelGGL(kern::bi_decide, dim3(1), dim3(64), 0, s, want_mu, want_nu,
                       (unsigned long long)lp, st);
}

void launch_bi_target(const uint64_t* Y, const uint64_t* X, uint64_t* S1, uint64_t* S2,
                      uint64_t nslots, bool beta, bool has_s1, const unsigned long long* st,
                      hipStream_t s) {
    const auto* y = reinterpret_cast<const unsigned long long*>(Y);
    const auto* x = reinterpret_cast<const unsigned long long*>(X);
    auto* s1 = reinterpret_cast<unsigned long long*>(S1);
    auto* s2 = reinterpret_cast<unsigned long long*>(S2);
    const dim3 grid(stride_grid(nslots)), blk(256);
    if (beta)
        hipLaunchKernelGGL(kern::bi_target<true>, grid, blk, 0, s, y, x, s1, s2, nslots, 1u, st);
    else
        hipLaunchKernelGGL(kern::bi_target<false>, grid, blk, 0, s, y, x, s1, s2, nslots,
                           has_s1 ? 1u : 0u, st);
}

}  // namespace cpd
