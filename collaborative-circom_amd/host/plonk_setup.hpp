// Plonk development keys from an .r1cs: snarkjs' `plonk setup` gate compiler on the GPU (csrc/plonk_setup_kernels.hpp), the key's polynomials
// by batched transforms, its points from seeded toxic waste.  DESIGN 6f.
#pragma once
#include "r1cs.hpp"

#include <algorithm>
#include <numeric>

namespace cgh {

// The canonical form the gate compiler takes: snarkjs keeps a combination as a map wire -> coefficient and walks it by ascending wire, so the
// file's term order must not matter.  A wire named twice has its coefficients summed (circom never writes that, and no shipped key pins it);
// terms whose coefficient is - or sums to - zero are dropped.  Integer work, field additions only where a wire repeats.
static void r1cs_canonicalise(R1csHandle& h) {
    if (h.canon.built) return;
    const R1cs& r = h.r; const Curve c = r.curve;
    const Fr zero = fr_from_u64(c, 0);
    std::vector<uint32_t> order;
    for (int m = 0; m < 3; m++) {
        std::vector<uint32_t>& rp = h.canon.row_ptr[m]; std::vector<uint32_t>& cl = h.canon.col[m]; std::vector<Fr>& co = h.canon.coeff[m];
        rp.assign(r.n_constraints + 1, 0); cl.clear(); co.clear(); cl.reserve(r.col[m].size()); co.reserve(r.col[m].size());
        const std::vector<uint32_t>& col = r.col[m];
        for (size_t i = 0; i < r.n_constraints; i++) {
            const uint32_t b = r.row_ptr[m][i], e = r.row_ptr[m][i + 1];
            order.resize(e - b); std::iota(order.begin(), order.end(), b);
            bool ascending = true;
            for (uint32_t k = b + 1; k < e && ascending; k++) ascending = col[k - 1] < col[k];
            if (!ascending) std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return col[x] < col[y]; });
            for (size_t k = 0; k < order.size();) {
                const uint32_t w = col[order[k]]; Fr v = r.coeff[m][order[k]];
                for (k++; k < order.size() && col[order[k]] == w; k++) v = fr_add(c, v, r.coeff[m][order[k]]);
                if (!fr_eq(v, zero)) { cl.push_back(w); co.push_back(v); }
            }
            rp[i + 1] = (uint32_t)cl.size();
        }
    }
    h.canon.built = true;
}
// the handle's context on `device` with the canonical matrices resident (call with the handle locked)
static R1csDevice& plonk_device(R1csHandle& h, int device) {
    r1cs_canonicalise(h);
    R1csDevice& d = h.dev[device];
    if (!d.ctx && cg_ctx_create(device, &d.ctx)) { d.ctx = nullptr; die("cg_ctx_create"); }
    for (int m = 0; m < 3; m++) {
        if (!d.canon_row_ptr[m]) d.canon_row_ptr[m] = dev_copy_of(d.ctx, h.canon.row_ptr[m].data(), h.canon.row_ptr[m].size() * 4);
        if (!d.canon_col[m]) d.canon_col[m] = dev_copy_of(d.ctx, h.canon.col[m].data(), h.canon.col[m].size() * 4);
        if (!d.canon_coeff[m]) d.canon_coeff[m] = dev_copy_of(d.ctx, h.canon.coeff[m].data(), h.canon.coeff[m].size() * 32);
    }
    return d;
}
struct PlonkCsrArgs { const uint32_t* rp[3]; const uint32_t* cl[3]; const void* co[3]; };
static PlonkCsrArgs plonk_csr_args(const R1csDevice& d) {
    PlonkCsrArgs a;
    for (int m = 0; m < 3; m++) { a.rp[m] = (const uint32_t*)d.canon_row_ptr[m]; a.cl[m] = (const uint32_t*)d.canon_col[m]; a.co[m] = d.canon_coeff[m]; }
    return a;
}
// The sizes of the key: the count pass (k_plonk_gate_count and the scan) and the domain rule of snarkjs, n = the smallest power of two that
// holds the gates, at least 8.  d_counts / d_offsets: n_constraints(r1cs) + 1 u32 each, left filled for the emit pass.
struct PlonkPlan { size_t n_additions = 0, n_constraints = 0, n_vars = 0, n = 8, log_n = 3; };
static PlonkPlan plonk_plan(const R1csHandle& h, const R1csDevice& d, void* d_counts, void* d_offsets) {
    const R1cs& r = h.r;
    const PlonkCsrArgs a = plonk_csr_args(d);
    PlonkPlan p;
    const size_t nnz = h.canon.col[0].size() + h.canon.col[1].size() + h.canon.col[2].size();
    CG(cg_plonk_gates_count_dev(d.ctx, r.curve.id, a.rp, a.cl, a.co, r.n_constraints, nnz, (uint32_t*)d_counts, (uint32_t*)d_offsets, &p.n_additions));
    p.n_vars = r.n_wires + p.n_additions;
    p.n_constraints = r.n_public + r.n_constraints + p.n_additions;
    if (p.n_vars >> 32) throw std::runtime_error("plonk setup: " + std::to_string(p.n_vars) + " signals (wires and additions) do not fit 32 bits");
    while (p.n < p.n_constraints) { p.n <<= 1; p.log_n++; }
    if (p.log_n > 24) throw std::runtime_error("plonk setup: " + std::to_string(p.n_constraints) + " gates need a domain beyond 2^24");
    if (p.log_n + 2 > (size_t)snarkjs_roots_cached(r.curve).two_adicity) throw std::runtime_error("plonk setup: the 4n evaluation domain exceeds the field's two-adic subgroup");
    return p;
}
static PlonkPlan r1cs_plonk_info(R1csHandle& h, int device) {
    std::lock_guard<std::mutex> lock(h.mu);
    R1csDevice& d = plonk_device(h, device);
    const size_t words = h.r.n_constraints + 1;
    void* c = nullptr; void* o = nullptr;
    CG(cg_dev_alloc(d.ctx, words * 4, &c)); DevBufGuard counts{d.ctx, c};
    CG(cg_dev_alloc(d.ctx, words * 4, &o)); DevBufGuard offsets{d.ctx, o};
    return plonk_plan(h, d, counts.p, offsets.p);
}
// k1, k2 with k1^n, k2^n, (k2 / k1)^n != 1: the search of synth_plonk_circuit (2 and 3 on every domain the fields allow)
static void plonk_coset_shifts(const Curve& c, size_t n, Fr& k1, Fr& k2) {
    const Fr one = fr_from_u64(c, 1);
    const uint64_t ne[1] = {(uint64_t)n};
    auto coset_ok = [&](const Fr& x) { return !fr_eq(fr_pow(c, x, ne, 1), one); };
    k1 = fr_from_u64(c, 2); k2 = fr_from_u64(c, 3);
    while (!coset_ok(k1)) k1 = fr_add(c, k1, one);
    while (!coset_ok(k2) || !coset_ok(fr_mul(c, k2, fr_inv(c, k1)))) k2 = fr_add(c, k2, one);
}

// A snarkjs-format Plonk .zkey (sections 1-14, the layout synth_plonk_circuit writes and read_plonk_zkey parses) for the circuit of an .r1cs,
// with p_tau = [tau^i]_1 from the given tau.  FOR DEVELOPMENT ONLY: whoever holds tau (the seed of cgh_setup_plonk_dev) can forge proofs
// for the key.  Header numbers, additions, wire maps and the q / sigma / Lagrange polynomials are those of snarkjs' `plonk setup`
// (byte-equal to the shipped keys); only the points depend on tau.
// On the device: the gates (count, scan, emit), the sigma rows (host: one pass over the 3n positions for the previous position of each
// signal; device: the labels), coefficients and 4n evaluations of the 8 + n_public polynomials by cg_ntt_dev in batches of 8, tau^i by
// fill + distribute_powers, p_tau and X_2 by cg_bases_from_scalars, the eight commitments by cg_msm_dev over p_tau.
// Sign and merge conventions no shipped key pins (no fixture has a constant-only A or B, or a repeated wire): a row with A = k is the sum
// gate of k * B - C rather than of C - k * B (the same equation; proofs of circuits with such rows verifying is what pins the relative sign),
// and repeated wires are summed.
// stage_seconds (optional, PLONK_SETUP_STAGES values): canonical form + upload + count pass, emit + download of maps and additions, sigma,
// transforms of the 8 polynomials with their download, p_tau + X_2 + the eight MSMs, transforms of the Lagrange polynomials, file writes.
constexpr int PLONK_SETUP_STAGES = 7;
static void setup_plonk_tau_dev(R1csHandle& h, int device, const Fr& tau, const std::string& zkey_path, double* stage_seconds = nullptr) {
    std::lock_guard<std::mutex> lock(h.mu);
    double stage[PLONK_SETUP_STAGES] = {0, 0, 0, 0, 0, 0, 0};
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_last = now();
    auto lap = [&](int i) { const auto t = now(); stage[i] += std::chrono::duration<double>(t - t_last).count(); t_last = t; };
    R1csDevice& d = plonk_device(h, device);
    cg_ctx* ctx = d.ctx;
    const R1cs& r = h.r; const Curve c = r.curve;
    const size_t rows = r.n_constraints, n_pub = r.n_public;
    auto dev = [&](size_t bytes) { void* p = nullptr; CG(cg_dev_alloc(ctx, std::max<size_t>(bytes, 16), &p)); return p; };
    DevBufGuard counts{ctx, dev((rows + 1) * 4)}, offsets{ctx, dev((rows + 1) * 4)};
    const PlonkPlan pl = plonk_plan(h, d, counts.p, offsets.p);
    const size_t n = pl.n, N = 4 * n, nc = pl.n_constraints, n_add = pl.n_additions;
    const Fr one = fr_from_u64(c, 1), zero = fr_from_u64(c, 0);
    if (fr_eq(tau, zero)) throw std::runtime_error("plonk setup: tau is zero");
    { Fr t = tau; for (size_t i = 0; i < pl.log_n; i++) t = fr_mul(c, t, t);
      if (fr_eq(t, one)) throw std::runtime_error("plonk setup: tau lies on the evaluation domain (tau^n = 1; choose another seed)"); }
    lap(0);
    Fr k1, k2; plonk_coset_shifts(c, n, k1, k2);
    const SnarkjsRoots& rt = snarkjs_roots_cached(c);
    const Fr omega = rt.roots[pl.log_n], omega4 = rt.roots[pl.log_n + 2];
    // gates: maps, q rows, additions
    DevBufGuard maps{ctx, dev(3 * nc * 4)}, polys{ctx, dev(8 * n * 32)}, add_ids{ctx, dev(2 * n_add * 4)}, add_f{ctx, dev(2 * n_add * 32)};
    auto poly = [&](size_t i) { return (void*)((char*)polys.p + i * n * 32); };
    {
        const PlonkCsrArgs a = plonk_csr_args(d);
        uint32_t* mp[3]; void* q[5];
        for (int w = 0; w < 3; w++) mp[w] = (uint32_t*)maps.p + w * nc;
        for (int i = 0; i < 5; i++) q[i] = poly(i);
        CG(cg_plonk_gates_emit_dev(ctx, c.id, a.rp, a.cl, a.co, rows, r.n_wires, n_pub, (const uint32_t*)counts.p, (const uint32_t*)offsets.p, n_add, n, mp, q,
                                   (uint32_t*)add_ids.p, add_f.p));
    }
    std::vector<uint32_t> map_h(3 * nc), ids_h(2 * n_add);
    std::vector<Fr> f_h(2 * n_add);
    CG(cg_dev_download(ctx, map_h.data(), maps.p, 3 * nc * 4));
    if (n_add) { CG(cg_dev_download(ctx, ids_h.data(), add_ids.p, 2 * n_add * 4)); CG(cg_dev_download(ctx, f_h.data(), add_f.p, 2 * n_add * 32)); }
    lap(1);
    // sigma: rows then columns; rows past the gates carry signal 0 in all three columns; a signal's first position takes its last
    {
        const uint32_t none = 0xffffffffu;
        std::vector<uint32_t> prev(3 * n), first(pl.n_vars, none), last(pl.n_vars, none);
        for (size_t i = 0; i < n; i++) for (size_t w = 0; w < 3; w++) {
            const uint32_t s = i < nc ? map_h[w * nc + i] : 0, p = (uint32_t)(w * n + i);
            if (last[s] == none) first[s] = p; else prev[p] = last[s];
            last[s] = p;
        }
        for (size_t s = 0; s < pl.n_vars; s++) if (first[s] != none) prev[first[s]] = last[s];
        DevBufGuard d_prev{ctx, dev_copy_of(ctx, prev.data(), prev.size() * 4)}, wpow{ctx, dev(n * 32)};
        CG(cg_vec_fill_dev(ctx, c.id, wpow.p, n, one.v));
        CG(cg_vec_distribute_powers_dev(ctx, c.id, wpow.p, n, omega.v, one.v));
        CG(cg_plonk_sigma_labels_dev(ctx, c.id, (const uint32_t*)d_prev.p, wpow.p, n, k1.v, k2.v, poly(5)));
        CG(cg_ctx_sync(ctx));                                                                    // (the two vectors are freed at the end of this scope)
    }
    lap(2);
    // k <= 8 polynomials, their rows in poly(0 .. k): coefficients in place, then per polynomial coefficients | 4n evaluations into out
    DevBufGuard evals{ctx, dev(8 * N * 32)};
    auto blocks = [&](int k, Bytes& out) {
        void* v[8]; void* e[8];
        for (int j = 0; j < k; j++) { v[j] = poly(j); e[j] = (char*)evals.p + (size_t)j * N * 32; }
        CG(cg_ntt_dev(ctx, c.id, v, k, n, omega.v, 1, nullptr));
        CG(cg_dev_memset_zero(ctx, evals.p, (size_t)k * N * 32));
        for (int j = 0; j < k; j++) CG(cg_vec_gather_strided_dev(ctx, c.id, e[j], v[j], n, 0, 1));
        CG(cg_ntt_dev(ctx, c.id, e, k, N, omega4.v, 0, nullptr));
        out.resize((size_t)k * 5 * n * 32);
        for (int j = 0; j < k; j++) {
            CG(cg_dev_download(ctx, out.data() + (size_t)j * 5 * n * 32, v[j], n * 32));
            CG(cg_dev_download(ctx, out.data() + (size_t)j * 5 * n * 32 + n * 32, e[j], N * 32));
        }
    };
    Bytes main_blocks; blocks(8, main_blocks);
    lap(3);
    // points: p_tau, X_2, the commitments q(tau) G1 as MSMs of the coefficient vectors over p_tau
    const size_t psz = c.aff(CG_G1);
    Bytes ptau((n + 6) * psz), x2(c.aff(CG_G2)), vk;
    {
        DevBufGuard tp{ctx, dev((n + 6) * 32)};
        CG(cg_vec_fill_dev(ctx, c.id, tp.p, n + 6, one.v));
        CG(cg_vec_distribute_powers_dev(ctx, c.id, tp.p, n + 6, tau.v, one.v));
        struct BasesGuard { cg_bases* b = nullptr; ~BasesGuard() { if (b) cg_bases_release(b); } } g1, g2;
        CG(cg_bases_from_scalars(ctx, c.id, CG_G1, tp.p, n + 6, &g1.b));
        CG(cg_bases_from_scalars(ctx, c.id, CG_G2, (const char*)tp.p + 32, 1, &g2.b));
        CG(cg_bases_download(ctx, g1.b, 0, n + 6, ptau.data()));
        CG(cg_bases_download(ctx, g2.b, 0, 1, x2.data()));
        for (size_t i = 0; i < 8; i++) {
            const void* sc[1] = {poly(i)};
            Point p{Bytes(c.jac(CG_G1)), CG_G1};
            CG(cg_msm_dev(ctx, g1.b, 0, n, sc, 1, p.b.data()));
            const Bytes a = pt_to_affine(c, p);
            vk.insert(vk.end(), a.begin(), a.end());
        }
    }
    lap(4);
    SectionWriter zk(zkey_path, "zkey", 1, 14);
    zk.begin(1, 4); zk.u32(2);                                                               // protocol: plonk
    zk.begin(2, 4 + c.fq() + 4 + 32 + 20 + 64 + 8 * psz + c.aff(CG_G2));
    zk.u32((uint32_t)c.fq()); zk.put(MOD_Q[c.id], c.fq()); zk.u32(32); zk.put(MOD_R[c.id], 32);
    zk.u32((uint32_t)pl.n_vars); zk.u32((uint32_t)n_pub); zk.u32((uint32_t)n); zk.u32((uint32_t)n_add); zk.u32((uint32_t)nc);
    zk.put(k1.v, 32); zk.put(k2.v, 32); zk.put(vk.data(), vk.size()); zk.put(x2.data(), x2.size());
    zk.begin(3, (uint64_t)n_add * 72);
    for (size_t a = 0; a < n_add; a++) { zk.u32(ids_h[2 * a]); zk.u32(ids_h[2 * a + 1]); zk.put(f_h[2 * a].v, 32); zk.put(f_h[2 * a + 1].v, 32); }
    for (int w = 0; w < 3; w++) { zk.begin(4 + w, (uint64_t)nc * 4); zk.put(map_h.data() + w * nc, nc * 4); }
    for (int i = 0; i < 5; i++) { zk.begin(7 + i, (uint64_t)5 * n * 32); zk.put(main_blocks.data() + (size_t)i * 5 * n * 32, 5 * n * 32); }
    zk.begin(12, (uint64_t)15 * n * 32); zk.put(main_blocks.data() + (size_t)25 * n * 32, 15 * n * 32);
    { Bytes().swap(main_blocks); }
    zk.begin(13, (uint64_t)n_pub * 5 * n * 32);
    for (size_t j0 = 0; j0 < n_pub; j0 += 8) {                                              // L_j: row j is one
        const int k = (int)std::min<size_t>(8, n_pub - j0);
        lap(6);
        CG(cg_dev_memset_zero(ctx, polys.p, (size_t)k * n * 32));
        for (int j = 0; j < k; j++) CG(cg_dev_upload(ctx, (char*)poly(j) + (j0 + j) * 32, one.v, 32));
        Bytes b; blocks(k, b);
        lap(5);
        zk.put(b.data(), b.size());
    }
    zk.begin(14, ptau.size()); zk.put(ptau.data(), ptau.size());
    zk.close();
    lap(6);
    if (stage_seconds) std::copy(stage, stage + PLONK_SETUP_STAGES, stage_seconds);
}
// tau = the first draw of setup_toxic's generator for the seed, so that a test can recompute the key's points
static void setup_plonk_dev(R1csHandle& h, int device, uint64_t seed, const std::string& zkey_path) {
    Fr toxic[5]; setup_toxic(h.r.curve, seed, toxic);
    setup_plonk_tau_dev(h, device, toxic[0], zkey_path);
}

}  // namespace cgh
