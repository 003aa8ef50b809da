// Plonk setup on the device: snarkjs' R1CS -> Plonk gate compiler in two passes (count, scan, emit), and the labels of the copy permutation.
//
// Input: the three constraint matrices in CANONICAL CSR form (the host builds it once per .r1cs): inside a row the wires ascend strictly
// (a wire named twice is merged) and no coefficient is zero; a term on wire 0 - the constant - therefore comes first.
// A row becomes one sum or multiplication gate, preceded by the "addition" gates that shorten its combinations: reduce(terms, maxC) of a
// combination of t > maxC terms makes a = t - maxC additions, each joining the two oldest entries of a queue into a new wire pushed at
// its end.  In closed form addition j reads elem(2j) and elem(2j + 1), where elem(e) = term e for e < t and (base + e - t, 1) after, and
// elem(2a) .. elem(t + a - 1) are left: the queue is a counter, so a lane streams its row once per pass and keeps no array.
// A lane per row: rows have very uneven lengths (1 to hundreds of terms), the lanes of a wave diverge and wait for their longest row.
#pragma once
#include "launchers.hpp"
#include "vec_kernels.hpp"

namespace cg {

// the terms of one combination after its constant: col/coeff[i .. e)
template <class F>
struct LcStream {
    const uint32_t* __restrict__ col; const F* __restrict__ coeff; uint32_t i, e;
    __device__ __forceinline__ bool next(uint32_t& wire, F& c) {
        if (i >= e) return false;
        wire = col[i]; c = ld_fp(coeff + i); i++;
        return true;
    }
};
// k * X - C by a two-pointer merge over the ascending wires; a wire whose terms cancel is skipped (that needs the field product)
template <class F>
struct JoinedStream {
    LcStream<F> x, c; F k;
    __device__ __forceinline__ bool next(uint32_t& wire, F& v) {
        for (;;) {
            const bool hx = x.i < x.e, hc = c.i < c.e;
            if (!hx && !hc) return false;
            const uint32_t wx = hx ? x.col[x.i] : 0xffffffffu, wc = hc ? c.col[c.i] : 0xffffffffu;
            if (wx < wc || !hc) { wire = wx; v = k * ld_fp(x.coeff + x.i); x.i++; return true; }
            if (wc < wx || !hx) { wire = wc; v = ld_fp(c.coeff + c.i).neg(); c.i++; return true; }
            v = k * ld_fp(x.coeff + x.i) - ld_fp(c.coeff + c.i); wire = wx; x.i++; c.i++;
            if (!v.is_zero()) return true;
        }
    }
};
// one combination of a row: its constant (zero when absent) and the stream of its terms
template <class F>
__device__ __forceinline__ LcStream<F> lc_open(const R1csMat& m, size_t row, F& k, bool& has_k) {
    uint32_t b = m.row_ptr[row]; const uint32_t e = m.row_ptr[row + 1];
    has_k = b < e && m.col[b] == 0;
    k = has_k ? ld_fp((const F*)m.coeff + b) : F::zero();
    return LcStream<F>{m.col, (const F*)m.coeff, b + (has_k ? 1u : 0u), e};
}
// what a row turns into: 0 = sum gate on C, 1 = sum gate on k_A * B - C, 2 = sum gate on k_B * A - C, 3 = multiplication gate
__device__ __forceinline__ int plonk_row_kind(uint32_t ta, bool ka, uint32_t tb, bool kb) {
    if ((!ta && !ka) || (!tb && !kb)) return 0;
    if (!ta) return 1;
    if (!tb) return 2;
    return 3;
}

// counts[row] = the additions the row makes.  blockDim.x == 256.
template <class F>
__global__ void __launch_bounds__(256) k_plonk_gate_count(R1csMat A, R1csMat B, R1csMat C, size_t n_rows, uint32_t* __restrict__ counts) {
    for (size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (size_t)gridDim.x * blockDim.x) {
        F k_a, k_b, k_c; bool ha, hb, hc;
        const LcStream<F> a = lc_open<F>(A, row, k_a, ha), b = lc_open<F>(B, row, k_b, hb), c = lc_open<F>(C, row, k_c, hc);
        const uint32_t ta = a.e - a.i, tb = b.e - b.i, tc = c.e - c.i;
        const int kind = plonk_row_kind(ta, ha, tb, hb);
        uint32_t n_add;
        if (kind == 3) n_add = (ta > 1 ? ta - 1 : 0) + (tb > 1 ? tb - 1 : 0) + (tc > 1 ? tc - 1 : 0);
        else {
            uint32_t t = tc;
            if (kind != 0) {
                JoinedStream<F> j{kind == 1 ? b : a, c, kind == 1 ? k_a : k_b};
                uint32_t wire; F v;
                for (t = 0; j.next(wire, v);) t++;
            }
            n_add = t > 3 ? t - 3 : 0;
        }
        counts[row] = n_add;
    }
}

template <class F>
__device__ __forceinline__ void plonk_put_gate(const PlonkGateOut& o, size_t g, uint32_t a, uint32_t b, uint32_t c, const F& qm, const F& ql, const F& qr, const F& qo, const F& qc) {
    o.map[0][g] = a; o.map[1][g] = b; o.map[2][g] = c;
    st_fp((F*)o.q[0] + g, qm); st_fp((F*)o.q[1] + g, ql); st_fp((F*)o.q[2] + g, qr); st_fp((F*)o.q[3] + g, qo); st_fp((F*)o.q[4] + g, qc);
}
// reduce(stream, MAXC) with n_add additions: writes their records and gates from addition `add` / gate row `g` / new wire `wire0` on (all
// three advanced), leaves the MAXC remaining entries in (lw, lv), padded with (wire 0, zero)
template <class F, int MAXC, class S>
__device__ __forceinline__ void plonk_reduce(S& s, uint32_t n_add, const PlonkGateOut& o, size_t& add, size_t& g, uint32_t& wire0, uint32_t (&lw)[MAXC], F (&lv)[MAXC]) {
    uint32_t made = 0;                       // synthetic entries handed out: wires wire0 .. wire0 + made - 1
    auto pop = [&](uint32_t& w, F& v) {      // the queue's head: the stream first, then the wires the additions made
        if (s.next(w, v)) return true;
        if (made >= n_add) return false;
        w = wire0 + made; v = F::one(); made++;
        return true;
    };
    for (uint32_t j = 0; j < n_add; j++) {
        uint32_t sl, sr; F cl, cr;
        pop(sl, cl); pop(sr, cr);            // (2j + 1 < t + j for every j < a = t - MAXC: both exist)
        o.add_ids[2 * add] = sl; o.add_ids[2 * add + 1] = sr;
        st_fp((F*)o.add_f + 2 * add, cl); st_fp((F*)o.add_f + 2 * add + 1, cr);
        plonk_put_gate<F>(o, g, sl, sr, wire0 + j, F::zero(), cl.neg(), cr.neg(), F::one(), F::zero());
        add++; g++;
    }
    _Pragma("unroll") for (int i = 0; i < MAXC; i++) { if (!pop(lw[i], lv[i])) { lw[i] = 0; lv[i] = F::zero(); } }
    wire0 += n_add;
}
// index < n_public: the public-input gate of signal index + 1.  Otherwise row = index - n_public: its additions from record offsets[row],
// new wire n_wires + offsets[row] and gate row n_public + row + offsets[row] on, then its own gate.  blockDim.x == 256.
template <class F>
__global__ void __launch_bounds__(256) k_plonk_gate_emit(R1csMat A, R1csMat B, R1csMat C, size_t n_rows, uint32_t n_wires, uint32_t n_public,
                                                        const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets, PlonkGateOut o) {
    const size_t total = n_rows + n_public;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        if (idx < n_public) { plonk_put_gate<F>(o, idx, (uint32_t)idx + 1, 0, 0, F::zero(), F::one(), F::zero(), F::zero(), F::zero()); continue; }
        const size_t row = idx - n_public;
        size_t add = offsets[row], g = idx + add;
        uint32_t wire0 = n_wires + (uint32_t)add;
        F k_a, k_b, k_c; bool ha, hb, hc;
        LcStream<F> a = lc_open<F>(A, row, k_a, ha), b = lc_open<F>(B, row, k_b, hb), c = lc_open<F>(C, row, k_c, hc);
        const uint32_t ta = a.e - a.i, tb = b.e - b.i, tc = c.e - c.i;
        const int kind = plonk_row_kind(ta, ha, tb, hb);
        if (kind == 3) {
            uint32_t wa[1], wb[1], wc[1]; F ca[1], cb[1], cc[1];
            plonk_reduce<F, 1>(a, ta - 1, o, add, g, wire0, wa, ca);
            plonk_reduce<F, 1>(b, tb - 1, o, add, g, wire0, wb, cb);
            plonk_reduce<F, 1>(c, tc > 1 ? tc - 1 : 0, o, add, g, wire0, wc, cc);
            plonk_put_gate<F>(o, g, wa[0], wb[0], wc[0], ca[0] * cb[0], ca[0] * k_b, k_a * cb[0], cc[0].neg(), k_a * k_b - k_c);
        } else {
            uint32_t w[3]; F v[3];
            const uint32_t n_add = counts[row];
            if (kind == 0) plonk_reduce<F, 3>(c, n_add, o, add, g, wire0, w, v);
            else {
                const F k = kind == 1 ? k_a : k_b;
                JoinedStream<F> j{kind == 1 ? b : a, c, k};
                plonk_reduce<F, 3>(j, n_add, o, add, g, wire0, w, v);
                k_c = k * (kind == 1 ? k_b : k_a) - k_c;
            }
            plonk_put_gate<F>(o, g, w[0], w[1], w[2], F::zero(), v[0], v[1], v[2], k_c);
        }
    }
}

// sigma[p] = k_(q / n) * w^(q mod n), q = prev[p], p < 3n (n = 2^log_n): the label of the position a wire was seen at before this one
template <class F>
__global__ void __launch_bounds__(256) k_plonk_sigma_labels(const uint32_t* __restrict__ prev, const F* __restrict__ wpow, int log_n, F k1, F k2, F* __restrict__ sigma) {
    const size_t total = (size_t)3 << log_n;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const uint32_t q = prev[p], col = q >> log_n;
        const F w = ld_fp(wpow + (q & (((uint32_t)1 << log_n) - 1)));
        st_fp(sigma + p, col == 0 ? w : (col == 1 ? k1 : k2) * w);
    }
}

}  // namespace cg
