// co-plonk elementwise kernels: the witness additions of round 1 (co-plonk/src/round1.rs:209-238), the factors of round 2's grand
// product (round2.rs:162-216) and the pointwise work of round 3 (round3.rs:234-470), each over every share component of a vector in one launch.  Public values enter the component that holds public
// addends (`pc`: plain / Shamir 0, REP3 party 0 -> a, party 1 -> b, party 2 -> none; rep3.rs:600-608), exactly as the generic chains
// of CoPlonk did with add_with_public.  Field arithmetic is exact, so summing in another order gives the same bits.
#pragma once
#include "vec_kernels.hpp"
#include "r1cs_kernels.hpp"

namespace cg {

// z[r] by selects, not by indexing the kernel arguments with a runtime index (which would copy them to scratch)
template <class F>
__device__ __forceinline__ F pick4(const F* z, int r) { return r == 0 ? z[0] : r == 1 ? z[1] : r == 2 ? z[2] : z[3]; }

// ---- round 1: one dependency level of the additions -----------------------------------------------------------------------------
// ext[n_priv + a] = f1 * w[id1] + f2 * w[id2] for the additions a = order[0..n) of one level; w[id] = pub[id] in component pc for
// id < n_inputs (0 in the other components), else ext[id - n_inputs].  Operands of a level lie in earlier levels or in the witness.
template <class F>
__global__ void __launch_bounds__(256) k_plonk_additions(const uint32_t* __restrict__ order, size_t n, const uint32_t* __restrict__ ids, const F* __restrict__ coeffs,
                                                         const F* __restrict__ pub, uint32_t n_inputs, int pc, F* __restrict__ ext_a, F* __restrict__ ext_b, size_t n_priv) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t a = order[t], id1 = ids[2 * a], id2 = ids[2 * a + 1];
        const F f1 = ld_fp(coeffs + 2 * a), f2 = ld_fp(coeffs + 2 * a + 1);
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            F* ext = j ? ext_b : ext_a;
            if (!ext) continue;
            const F w1 = id1 < n_inputs ? (j == pc ? ld_fp(pub + id1) : F::zero()) : ld_fp(ext + (id1 - n_inputs));
            const F w2 = id2 < n_inputs ? (j == pc ? ld_fp(pub + id2) : F::zero()) : ld_fp(ext + (id2 - n_inputs));
            st_fp(ext + n_priv + a, f1 * w1 + f2 * w2);
        }
    }
}

// ---- round 2 ------------------------------------------------------------------------------------------------------------------------
// The six factors of the grand product on the domain (round2.rs:162-216): num_w = buf_w + beta k_w omega^i + gamma and
// den_w = buf_w + beta sigma_w(omega^i) + gamma for w = a, b, c; the public addends in pc only.  omega^i = pw[i * pw_stride] (the
// omega4^i table with a stride of 4, or a table of its own), sigma_w(omega^i) = sigma[w][i * sigma_stride] (the 4n evaluations of the
// zkey with a stride of 4: no gathered copy).  coef = beta, beta k1, beta k2, gamma.  out: num_a, num_b, num_c, den_a, den_b, den_c.
template <class F> struct PlonkR2Args { const F* pw; size_t pw_stride; const F* sigma[3]; size_t sigma_stride; F coef[4]; const F* w[3][2]; F* out[6][2]; int k, pc; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_r2_factors(PlonkR2Args<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        F pf[3], pg[3];
        if (g.pc >= 0) {
            const F x = ld_fp(g.pw + i * g.pw_stride);
            _Pragma("unroll") for (int w = 0; w < 3; w++) { pf[w] = g.coef[w] * x + g.coef[3]; pg[w] = g.coef[0] * ld_fp(g.sigma[w] + i * g.sigma_stride) + g.coef[3]; }
        }
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            _Pragma("unroll") for (int w = 0; w < 3; w++) {
                const F v = ld_fp(g.w[w][j] + i);
                st_fp(g.out[w][j] + i, j == g.pc ? v + pf[w] : v);
                st_fp(g.out[3 + w][j] + i, j == g.pc ? v + pg[w] : v);
            }
        }
    }
}

// ---- round 3 ------------------------------------------------------------------------------------------------------------------------
// The blinding polynomials on the 4n-th roots (round3.rs:246-256, 307-322), x = pw[i] = omega4^i, xw = omega * x:
// ap = b1 x + b2, bp = b3 x + b4, cp = b5 x + b6, zp = b7 x^2 + b8 x + b9, zwp = b7 xw^2 + b8 xw + b9   (b[0..8] = b_1..b_9)
template <class F> struct PlonkBlindArgs { const F* pw; F omega; F b[2][9]; F* out[5][2]; int k; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_r3_blind(PlonkBlindArgs<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const F x = ld_fp(g.pw + i), x2 = x * x, xw = g.omega * x, xw2 = xw * xw;
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            const F* b = g.b[j];
            st_fp(g.out[0][j] + i, b[0] * x + b[1]);
            st_fp(g.out[1][j] + i, b[2] * x + b[3]);
            st_fp(g.out[2][j] + i, b[4] * x + b[5]);
            st_fp(g.out[3][j] + i, b[6] * x2 + b[8] + b[7] * x);
            st_fp(g.out[4][j] + i, b[6] * xw2 + b[8] + b[7] * xw);
        }
    }
}
// The six permutation factors (round3.rs:370-418): f_w = w + beta k_w x + gamma, g_w = w + beta sigma_w + gamma, the public parts in pc.
// coef = beta, beta k1, beta k2, gamma
template <class F> struct PlonkPermArgs { const F* pw; const F* sigma[3]; F coef[4]; const F* w[3][2]; F* out[6][2]; int k, pc; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_r3_perm(PlonkPermArgs<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const F x = ld_fp(g.pw + i);
        F pf[3], pg[3];
        _Pragma("unroll") for (int w = 0; w < 3; w++) { pf[w] = g.coef[w] * x + g.coef[3]; pg[w] = g.coef[0] * ld_fp(g.sigma[w] + i) + g.coef[3]; }
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            _Pragma("unroll") for (int w = 0; w < 3; w++) {
                const F v = ld_fp(g.w[w][j] + i);
                st_fp(g.out[w][j] + i, j == g.pc ? v + pf[w] : v);
                st_fp(g.out[3 + w][j] + i, j == g.pc ? v + pg[w] : v);
            }
        }
    }
}
// The gate constraint and its blinding twin (round3.rs:333-368):
// e1  = qm a b + ql a + qr b + qo c + qc - sum_l L_l a_l          (qc and the public-input term: a_l is the share of buffer_a[l])
// e1z = qm (a b' + a' b + Z1 a' b') + ql a' + qr b' + qo c'
// in: 0 buffer_a, 1 a b, 2 a b', 3 a' b, 4 a' b', 5 a, 6 b, 7 c, 8 a', 9 b', 10 c'
template <class F> struct PlonkGateArgs { const F* q[5]; const F* lag; size_t n_lag; const F* in[11][2]; F z1[4]; F* e1[2]; F* e1z[2]; int k, pc; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_r3_gate(PlonkGateArgs<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const F qm = ld_fp(g.q[0] + i), ql = ld_fp(g.q[1] + i), qr = ld_fp(g.q[2] + i), qo = ld_fp(g.q[3] + i);
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            auto in = [&](int s) { return ld_fp(g.in[s][j] + i); };
            F e = qm * in(1) + ql * in(5) + qr * in(6) + qo * in(7);
            if (j == g.pc) e = e + ld_fp(g.q[4] + i);
            F pi = F::zero();
            for (size_t l = 0; l < g.n_lag; l++) pi = pi + ld_fp(g.lag + l * n + i) * ld_fp(g.in[0][j] + l);
            st_fp(g.e1[j] + i, e - pi);
            const F a0 = in(2) + in(3) + pick4(g.z1, (int)(i & 3)) * in(4);
            st_fp(g.e1z[j] + i, qm * a0 + ql * in(8) + qr * in(9) + qo * in(10));
        }
    }
}
// The end of mul4vec_post (round3.rs:17-72): rz = p0 + p1 + Z1 (p2 + p3 + p4) + Z2 (p5 + p6) + Z3 p7 over the eight products
// S1 CD, AB S2 | A'B' CD, S1 S2, AB C'D' | S1 C'D', A'B' S2 | A'B' C'D'
template <class F> struct PlonkMul4Args { const F* p[8][2]; F z[3][4]; F* rz[2]; int k; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_mul4_tail(PlonkMul4Args<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i & 3);
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            auto p = [&](int s) { return ld_fp(g.p[s][j] + i); };
            st_fp(g.rz[j] + i, p(0) + p(1) + pick4(g.z[0], r) * (p(2) + p(3) + p(4)) + pick4(g.z[1], r) * (p(5) + p(6)) + pick4(g.z[2], r) * p(7));
        }
    }
}
// t = e1 + alpha (e2 - e3) + alpha^2 L1 (z - 1), tz = e1z + alpha (e2z - e3z) + alpha^2 L1 z'   (round3.rs:420-441; the 1 in pc)
// in: 0 e1, 1 e1z, 2 e2, 3 e3, 4 e2z, 5 e3z, 6 z, 7 z'
template <class F> struct PlonkTArgs { const F* l1; const F* in[8][2]; F alpha, alpha2; F* t[2]; F* tz[2]; int k, pc; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_r3_t(PlonkTArgs<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const F l = g.alpha2 * ld_fp(g.l1 + i);
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            auto in = [&](int s) { return ld_fp(g.in[s][j] + i); };
            F z = in(6);
            if (j == g.pc) z = z - F::one();
            st_fp(g.t[j] + i, in(0) + g.alpha * (in(2) - in(3)) + l * z);
            st_fp(g.tz[j] + i, in(1) + g.alpha * (in(4) - in(5)) + l * in(7));
        }
    }
}
// After the inverse NTTs of t and tz (round3.rs:443-453), per block of n coefficients: t0 = -t0, t_b = t_(b-1) - t_b (the division by
// X^n - 1), then t += tz.  One lane owns the four entries i, n + i, 2n + i, 3n + i.
template <class F> struct PlonkDivArgs { F* t[2]; const F* tz[2]; int k; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_r3_divide(PlonkDivArgs<F> g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        _Pragma("unroll") for (int j = 0; j < 2; j++) {
            if (j >= g.k) break;
            F run = F::zero();
            _Pragma("unroll") for (int b = 0; b < 4; b++) {
                const size_t o = (size_t)b * n + i;
                run = run - ld_fp(g.t[j] + o);
                st_fp(g.t[j] + o, run + ld_fp(g.tz[j] + o));
            }
        }
    }
}

// ---- a witness against the gates of a key, and exact comparisons of resident vectors ---------------------------------------------------
// The value of wire `id` as round 1 and k_plonk_additions read it: pub[id] for id < n_inputs (= n_public + 1; the caller keeps pub[0] = 0,
// types.rs:107-109), else the extended witness (private part, then the additions).
template <class F>
__device__ __forceinline__ F plonk_wire(uint32_t id, const F* __restrict__ pub, uint32_t n_inputs, const F* __restrict__ ext) {
    return id < n_inputs ? ld_fp(pub + id) : ld_fp(ext + (id - n_inputs));
}
// A lane per row i < n of the domain: res = qm a b + ql a + qr b + qo c + qc - (i < n_public ? w[i + 1] : 0) with a, b, c the wires
// map[0..2][i] for i < n_constraints and zero on the padding rows (which are checked too: a key with a selector there fails them for every
// witness).  q[s][i * q_stride]: the 4n evaluations of a session with a stride of 4, or a vector of its own.  A row that names a wire
// >= n_wires is counted as failing and nothing is read for it.  Ends as k_r1cs_check (r1cs_report).  blockDim.x == 256.
template <class F> struct PlonkCheckArgs { const uint32_t* map[3]; const F* q[5]; size_t q_stride; size_t n_constraints; const F* pub; uint32_t n_public; const F* ext; uint32_t n_wires; };
template <class F>
__global__ void __launch_bounds__(256) k_plonk_gate_check(PlonkCheckArgs<F> g, size_t n, unsigned long long* __restrict__ result) {
    unsigned long long count = 0, first = ~0ull;
    const uint32_t n_inputs = g.n_public + 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t o = i * g.q_stride;
        F res = ld_fp(g.q[4] + o);
        bool bad = false;
        if (i < g.n_constraints) {
            const uint32_t ia = g.map[0][i], ib = g.map[1][i], ic = g.map[2][i];
            bad = ia >= g.n_wires || ib >= g.n_wires || ic >= g.n_wires;
            if (!bad) {
                const F a = plonk_wire<F>(ia, g.pub, n_inputs, g.ext), b = plonk_wire<F>(ib, g.pub, n_inputs, g.ext);
                res = res + (ld_fp(g.q[0] + o) * b + ld_fp(g.q[1] + o)) * a + ld_fp(g.q[2] + o) * b + ld_fp(g.q[3] + o) * plonk_wire<F>(ic, g.pub, n_inputs, g.ext);
            }
        }
        if (i < g.n_public) res = res - ld_fp(g.pub + i + 1);
        if (bad || !res.is_zero()) { count++; first = i < first ? i : first; }         // rows ascend per lane: the first hit is the smallest
    }
    r1cs_report(count, first, result);
}
// The positions first <= i < n at which a[i * a_stride] != b[i * b_stride], or (ZERO) at which a[i * a_stride] != 0: count and smallest i.
// The elements are compared as stored (limb by limb).  Ends as k_r1cs_check.  blockDim.x == 256.
template <class F, bool ZERO>
__global__ void __launch_bounds__(256) k_vec_mismatch(const F* __restrict__ a, size_t a_stride, const F* __restrict__ b, size_t b_stride, size_t first_row, size_t n,
                                                      unsigned long long* __restrict__ result) {
    unsigned long long count = 0, first = ~0ull;
    for (size_t i = first_row + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const F x = ld_fp(a + i * a_stride);
        bool differ;
        if (ZERO) differ = !x.is_zero();
        else { const F y = ld_fp(b + i * b_stride); differ = x != y; }
        if (differ) { count++; first = i < first ? i : first; }
    }
    r1cs_report(count, first, result);
}

}  // namespace cg
