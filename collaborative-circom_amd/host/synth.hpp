// synthetic satisfiable circuit + valid Groth16 CRS written as .zkey / .wtns (bench and test tooling)
#pragma once
#include "groth16.hpp"
#include "plonk.hpp"

namespace cgh {

// ---- synthetic satisfiable circuit + valid Groth16 CRS (bench / test tooling; SURVEY.md §8d "synthetic R1CS generator") --------------
// Writes a snarkjs-format .zkey (sections 1-9, the layout read_zkey above parses: circom-types/src/groth16/zkey.rs:139-316) and a
// .wtns (witness.rs:51-91), so that sessions and file -> proof runs have a real file of any size to work on: the shipped fixtures stop
// at 213 constraints.  n_public = 1, num_constraints = m - 2, n_vars = m = domain size; constraint j:
//     (ca_j * w[j+1]) * (cb_j * w[sb_j]) = w[j+2],   sb_j = 1 + (7 j + 3) mod (j + 1)  (<= j + 1: the witness is computed forward).
// CRS from seeded toxic waste (tau, alpha, beta, gamma, delta): polynomial evaluations on the host (field arithmetic through the
// ABI's cg_fr_op, on a few threads), the five point tables by fixed-base batch multiplication on the GPU (cg_bases_from_scalars).
// Conventions the prover relies on (groth16.rs:141-204): section 4 carries the rows A[nc + i] = w_i for i <= n_public, and
//     h_query[i] = [ (tau^2m - 1) g w^i / (2 m delta (tau - g w^i)) ]_1,   g = w_2m:
// H = (AB - C)/Z is interpolated on the odd coset gH, where Z = g^m - 1 = -2, so the prover's h_i = (AB - C)(g w^i) needs no division.
static void batch_inverse(const Curve& c, std::vector<Fr>& v) {           // Montgomery's trick per slice; no zero elements
    parallel_for(v.size(), [&](size_t lo, size_t hi) {
        if (hi <= lo) return;
        std::vector<Fr> pre(hi - lo);
        Fr acc = fr_from_u64(c, 1);
        for (size_t i = lo; i < hi; i++) { pre[i - lo] = acc; acc = fr_mul(c, acc, v[i]); }
        Fr inv = fr_inv(c, acc);
        for (size_t i = hi; i-- > lo;) { const Fr t = fr_mul(c, inv, pre[i - lo]); inv = fr_mul(c, inv, v[i]); v[i] = t; }
    });
}
struct SplitMix { uint64_t s; uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); } };
static Fr random_nonzero_fr(const Curve& c, SplitMix& g) {
    for (;;) {
        Fr raw; for (int i = 0; i < 4; i++) raw.v[i] = g.next();
        raw.v[3] &= c.id == CG_BN254 ? 0x3fffffffffffffffull : 0x7fffffffffffffffull;
        bool lt = false, gt = false;
        for (int i = 3; i >= 0 && !lt && !gt; i--) { if (raw.v[i] < MOD_R[c.id][i]) lt = true; else if (raw.v[i] > MOD_R[c.id][i]) gt = true; }
        if (!lt || !(raw.v[0] | raw.v[1] | raw.v[2] | raw.v[3])) continue;
        Fr m; CG(cg_fr_from_canonical(c.id, raw.v, m.v, 1));
        return m;
    }
}
struct SectionWriter {     // sections are streamed: a 2^22-constraint zkey is 2 GB
    FILE* f;
    SectionWriter(const std::string& path, const char* magic, uint32_t version, uint32_t nsec) {
        f = fopen(path.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot write " + path);
        put(magic, 4); u32(version); u32(nsec);
    }
    ~SectionWriter() { if (f) fclose(f); }
    void put(const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) throw std::runtime_error("short write"); }
    void u32(uint32_t x) { put(&x, 4); }
    void u64(uint64_t x) { put(&x, 8); }
    void begin(uint32_t id, uint64_t bytes) { u32(id); u64(bytes); }
    void close() { if (f && fclose(f) != 0) { f = nullptr; throw std::runtime_error("close failed"); } f = nullptr; }
};
static void synth_circuit(int device, int curve_id, int log_m, uint64_t seed, const std::string& zkey_path, const std::string& wtns_path) {
    if (log_m < 2 || log_m > 26) throw std::runtime_error("log_m out of range");
    const Curve c{curve_id};
    const size_t m = (size_t)1 << log_m, nc = m - 2, n_pub = 1, n_vars = m, n_inp = n_pub + 1;
    SplitMix rng{seed * 0x2545f4914f6cdd1dull + 0x1234567};
    // circuit + witness (a serial chain by construction)
    std::vector<Fr> ca(nc), cb(nc), w(n_vars);
    std::vector<uint32_t> sb(nc);
    for (size_t j = 0; j < nc; j++) { ca[j] = random_nonzero_fr(c, rng); cb[j] = random_nonzero_fr(c, rng); sb[j] = (uint32_t)(1 + (7 * j + 3) % (j + 1)); }
    w[0] = fr_from_u64(c, 1); w[1] = random_nonzero_fr(c, rng);
    for (size_t j = 0; j < nc; j++) w[j + 2] = fr_mul(c, fr_mul(c, ca[j], w[j + 1]), fr_mul(c, cb[j], w[sb[j]]));
    // toxic waste, Lagrange values of the domain at tau
    const Fr tau = random_nonzero_fr(c, rng), alpha = random_nonzero_fr(c, rng), beta = random_nonzero_fr(c, rng), gamma = random_nonzero_fr(c, rng), delta = random_nonzero_fr(c, rng);
    const Domain dom = groth16_domain(c, (size_t)log_m, nc, n_inp);
    const Fr one = fr_from_u64(c, 1);
    Fr tau_m = tau; for (int i = 0; i < log_m; i++) tau_m = fr_mul(c, tau_m, tau_m);
    std::vector<Fr> wpow(m), lag(m), hexp(m);
    {   // w^j by slices: each slice starts from w^lo (square-and-multiply) and runs a product chain
        parallel_for(m, [&](size_t lo, size_t hi) {
            if (hi <= lo) return;
            uint64_t e[1] = {lo};
            Fr acc = fr_pow(c, dom.omega, e, 1);
            for (size_t j = lo; j < hi; j++) { wpow[j] = acc; acc = fr_mul(c, acc, dom.omega); }
        });
    }
    parallel_for(m, [&](size_t lo, size_t hi) { for (size_t j = lo; j < hi; j++) { lag[j] = fr_sub(c, tau, wpow[j]); hexp[j] = fr_sub(c, tau, fr_mul(c, dom.coset_g, wpow[j])); } });
    batch_inverse(c, lag); batch_inverse(c, hexp);
    const Fr zt_over_m = fr_mul(c, fr_sub(c, tau_m, one), fr_inv(c, fr_from_u64(c, (uint64_t)m)));
    const Fr hfac = fr_mul(c, fr_mul(c, fr_sub(c, fr_mul(c, tau_m, tau_m), one), fr_inv(c, fr_mul(c, fr_from_u64(c, 2 * (uint64_t)m), delta))), dom.coset_g);
    parallel_for(m, [&](size_t lo, size_t hi) { for (size_t j = lo; j < hi; j++) { lag[j] = fr_mul(c, fr_mul(c, zt_over_m, wpow[j]), lag[j]); hexp[j] = fr_mul(c, fr_mul(c, hfac, wpow[j]), hexp[j]); } });
    { std::vector<Fr>().swap(wpow); }
    // u_i = sum_j A[j][i] L_j(tau), v_i, and the C column (C[j][j+2] = 1)
    const Fr zero = fr_sub(c, one, one);
    std::vector<Fr> u(n_vars, zero), v(n_vars, zero), lic(n_vars);
    parallel_for(nc, [&](size_t lo, size_t hi) { for (size_t j = lo; j < hi; j++) u[j + 1] = fr_mul(c, ca[j], lag[j]); });
    for (size_t j = 0; j < nc; j++) v[sb[j]] = fr_add(c, v[sb[j]], fr_mul(c, cb[j], lag[j]));     // colliding targets: serial
    for (size_t i = 0; i < n_inp; i++) u[i] = fr_add(c, u[i], lag[nc + i]);
    const Fr ginv = fr_inv(c, gamma), dinv = fr_inv(c, delta);
    parallel_for(n_vars, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            Fr t = fr_add(c, fr_mul(c, beta, u[i]), fr_mul(c, alpha, v[i]));
            if (i >= 2) t = fr_add(c, t, lag[i - 2]);                                         // C column: w_i = L_(i-2) for i >= 2
            lic[i] = fr_mul(c, t, i <= n_pub ? ginv : dinv);
        }
    });
    // group elements on the GPU
    CtxGuard cg; if (cg_ctx_create(device, &cg.ctx)) die("cg_ctx_create");
    cg_ctx* ctx = cg.ctx;
    auto table = [&](const std::vector<Fr>& sc, int group) {
        DevBufGuard d{ctx, nullptr};
        CG(cg_dev_alloc(ctx, sc.size() * 32, &d.p));
        CG(cg_dev_upload(ctx, d.p, sc.data(), sc.size() * 32));
        cg_bases* b = nullptr; CG(cg_bases_from_scalars(ctx, c.id, group, d.p, sc.size(), &b));
        Bytes out(sc.size() * c.aff(group));
        const int rc = cg_bases_download(ctx, b, 0, sc.size(), out.data());
        cg_bases_release(b);
        if (rc) die("cg_bases_download");
        return out;
    };
    auto g1 = [&](const Fr& k) { return pt_to_affine(c, pt_mul(c, pt_generator(c, CG_G1), k)); };
    auto g2 = [&](const Fr& k) { return pt_to_affine(c, pt_mul(c, pt_generator(c, CG_G2), k)); };
    const uint32_t ncoef = (uint32_t)(2 * nc + n_inp);
    SectionWriter zk(zkey_path, "zkey", 1, 9);
    zk.begin(1, 4); zk.u32(1);                                                               // protocol: groth16
    zk.begin(2, 4 + c.fq() + 4 + 32 + 12 + 3 * c.aff(CG_G1) + 3 * c.aff(CG_G2));
    zk.u32((uint32_t)c.fq()); zk.put(MOD_Q[c.id], c.fq()); zk.u32(32); zk.put(MOD_R[c.id], 32);
    zk.u32((uint32_t)n_vars); zk.u32((uint32_t)n_pub); zk.u32((uint32_t)m);
    { Bytes a1 = g1(alpha), b1 = g1(beta), b2 = g2(beta), c2 = g2(gamma), d1 = g1(delta), d2 = g2(delta);
      zk.put(a1.data(), a1.size()); zk.put(b1.data(), b1.size()); zk.put(b2.data(), b2.size()); zk.put(c2.data(), c2.size()); zk.put(d1.data(), d1.size()); zk.put(d2.data(), d2.size()); }
    Bytes l_all = table(lic, CG_G1);
    { std::vector<Fr>().swap(lic); }
    zk.begin(3, n_inp * c.aff(CG_G1)); zk.put(l_all.data(), n_inp * c.aff(CG_G1));
    zk.begin(4, 4 + (uint64_t)ncoef * 44); zk.u32(ncoef);
    {   // value on disk = v * R^2: the Montgomery form of the Montgomery form (traits.rs:57-67 reduces once)
        auto rec = [&](uint32_t mat, uint32_t row, uint32_t sig, const Fr& val) { Fr d; CG(cg_fr_from_canonical(c.id, val.v, d.v, 1)); zk.u32(mat); zk.u32(row); zk.u32(sig); zk.put(d.v, 32); };
        for (size_t j = 0; j < nc; j++) { rec(0, (uint32_t)j, (uint32_t)(j + 1), ca[j]); rec(1, (uint32_t)j, sb[j], cb[j]); }
        for (size_t i = 0; i < n_inp; i++) rec(0, (uint32_t)(nc + i), (uint32_t)i, one);
    }
    { Bytes t = table(u, CG_G1); zk.begin(5, t.size()); zk.put(t.data(), t.size()); }
    { Bytes t = table(v, CG_G1); zk.begin(6, t.size()); zk.put(t.data(), t.size()); }
    { Bytes t = table(v, CG_G2); zk.begin(7, t.size()); zk.put(t.data(), t.size()); }
    zk.begin(8, (n_vars - n_inp) * c.aff(CG_G1)); zk.put(l_all.data() + n_inp * c.aff(CG_G1), (n_vars - n_inp) * c.aff(CG_G1));
    { Bytes t = table(hexp, CG_G1); zk.begin(9, t.size()); zk.put(t.data(), t.size()); }
    zk.close();
    SectionWriter wt(wtns_path, "wtns", 2, 2);
    wt.begin(1, 4 + 32 + 4); wt.u32(32); wt.put(MOD_R[c.id], 32); wt.u32((uint32_t)n_vars);
    wt.begin(2, (uint64_t)n_vars * 32);
    { std::vector<Fr> can(n_vars); CG(cg_fr_to_canonical(c.id, w.data(), can.data(), n_vars)); wt.put(can.data(), n_vars * 32); }
    wt.close();
}

// ---- synthetic satisfiable Plonk circuit (bench / test tooling) ------------------------------------------------------------------------
// A snarkjs-format Plonk .zkey (sections 1-14 as read_plonk_zkey parses them: circom-types/src/plonk/zkey.rs:83-255, header :373-424) and
// its .wtns, from seeded toxic waste tau, so that Plonk sessions have keys of any size: the shipped fixtures stop at domain 64.
// Signals: 0 = one, 1..n_public public, then n_priv private (4 seeds and one output per gate), then the additions.  Rows 0..n_public-1
// are the public-input gates (a = public j + 1, ql = 1, the row layout of round 3's pi -= L_j buffer_a[j]); the other rows up to
// n_constraints = n - max(1, n / 16) are multiplication (qm = 1, qo = -1), addition (ql = qr = 1, qo = -1) and constant gates (qo = 1,
// qc = -K), whose inputs a, b are drawn from every signal made before (fan-out: copy cycles longer than 2).  Addition a = f1 w[id1] +
// f2 w[id2]: id1 continues a chain of six (a % 6 != 0), id2 is a public input (a % 3 == 0) or a seed; gates read additions too.
// Padding rows and unused positions carry the identity permutation.  Field elements and points are stored as the readers take them
// (the shipped keys' encoding: Montgomery limbs, packed affine points); evaluations on the 4n roots are the library's NTT at
// omega4 = the (power + 2)-th snarkjs root, what CoPlonk::round3 assumes; vk = q(tau) G1, X_2 = tau G2.
static void synth_plonk_circuit(int device, int curve_id, int log_n, uint64_t seed, uint32_t n_public, uint32_t n_additions,
                                const std::string& zkey_path, const std::string& wtns_path) {
    if (log_n < 3 || log_n > 24) throw std::runtime_error("log_n out of range (3..24)");
    const Curve c{curve_id};
    const size_t n = (size_t)1 << log_n, N = 4 * n, nc = n - std::max<size_t>(1, n / 16);
    if (n_public < 1 || n_public + 2 > nc) throw std::runtime_error("n_public must be 1 .. n_constraints - 2");
    const size_t n_seed = 4, n_gates = nc - n_public, n_priv = n_seed + n_gates;
    const size_t n_vars = 1 + n_public + n_priv + n_additions, base = 1 + n_public;
    SplitMix rng{seed * 0x9e3779b97f4a7c15ull + 0x51ed270b};
    const Fr zero = fr_from_u64(c, 0), one = fr_from_u64(c, 1), minus_one = fr_sub(c, zero, one);
    std::vector<Fr> val(n_vars, zero);                                                // signal values (additions included)
    val[0] = one;
    for (size_t i = 1; i < base + n_seed; i++) val[i] = random_nonzero_fr(c, rng);
    // additions (computed first: they read public inputs, seeds and earlier additions only)
    const size_t add0 = base + n_priv;
    std::vector<PlonkZKey::Addition> adds(n_additions);
    for (size_t a = 0; a < n_additions; a++) {
        auto& e = adds[a];
        e.id1 = (a % 6) ? (uint32_t)(add0 + a - 1) : (uint32_t)(1 + rng.next() % (n_public + n_seed));
        e.id2 = (a % 3 == 0) ? (uint32_t)(1 + rng.next() % n_public) : (uint32_t)(base + rng.next() % n_seed);
        e.f1 = random_nonzero_fr(c, rng); e.f2 = random_nonzero_fr(c, rng);
        val[add0 + a] = fr_add(c, fr_mul(c, e.f1, val[e.id1]), fr_mul(c, e.f2, val[e.id2]));
    }
    // gates
    std::vector<uint32_t> map[3]; for (auto& m : map) m.assign(nc, 0);
    std::vector<Fr> q[5]; for (auto& v : q) v.assign(n, zero);                          // qm, ql, qr, qo, qc on the rows
    for (size_t j = 0; j < n_public; j++) { map[0][j] = (uint32_t)(1 + j); q[1][j] = one; }
    std::vector<uint32_t> pool; for (size_t i = 1; i < base + n_seed; i++) pool.push_back((uint32_t)i);
    for (size_t a = 0; a < n_additions; a++) pool.push_back((uint32_t)(add0 + a));
    for (size_t g = 0; g < n_gates; g++) {
        const size_t row = n_public + g; const uint32_t out = (uint32_t)(base + n_seed + g);
        const uint32_t sa = pool[rng.next() % pool.size()], sb = pool[rng.next() % pool.size()];
        map[0][row] = sa; map[1][row] = sb; map[2][row] = out;
        switch (rng.next() % 3) {
        case 0: q[0][row] = one; q[3][row] = minus_one; val[out] = fr_mul(c, val[sa], val[sb]); break;
        case 1: q[1][row] = one; q[2][row] = one; q[3][row] = minus_one; val[out] = fr_add(c, val[sa], val[sb]); break;
        default: { const Fr K = random_nonzero_fr(c, rng); q[3][row] = one; q[4][row] = fr_sub(c, zero, K); val[out] = K; }
        }
        pool.push_back(out);
    }
    // k1, k2: k1^n, k2^n, (k2 / k1)^n != 1 (the three cosets are disjoint)
    const uint64_t ne[1] = {(uint64_t)n};
    auto coset_ok = [&](const Fr& x) { return !fr_eq(fr_pow(c, x, ne, 1), one); };
    Fr k1 = fr_from_u64(c, 2), k2 = fr_from_u64(c, 3);
    while (!coset_ok(k1)) k1 = fr_add(c, k1, one);
    while (!coset_ok(k2) || !coset_ok(fr_mul(c, k2, fr_inv(c, k1)))) k2 = fr_add(c, k2, one);
    // the permutation: positions p = w n + i labelled k_w omega^i; the positions of one signal form one cycle
    const SnarkjsRoots rt = snarkjs_roots(c);
    const Fr omega = rt.roots[log_n], omega4 = rt.roots[log_n + 2];
    std::vector<Fr> wpow(n); { Fr acc = one; for (size_t i = 0; i < n; i++) { wpow[i] = acc; acc = fr_mul(c, acc, omega); } }
    const Fr kw[3] = {one, k1, k2};
    std::vector<uint32_t> next(3 * n); for (size_t p = 0; p < 3 * n; p++) next[p] = (uint32_t)p;
    {
        std::vector<int64_t> first(n_vars, -1), last(n_vars, -1);
        for (int w = 0; w < 3; w++) for (size_t i = 0; i < nc; i++) {
            const uint32_t s = map[w][i], p = (uint32_t)(w * n + i);
            if (first[s] < 0) first[s] = p; else next[last[s]] = p;
            last[s] = p;
        }
        for (size_t s = 0; s < n_vars; s++) if (first[s] >= 0) next[last[s]] = (uint32_t)first[s];
    }
    std::vector<Fr> sigma[3]; for (int w = 0; w < 3; w++) { sigma[w].resize(n); for (size_t i = 0; i < n; i++) { const uint32_t p = next[w * n + i]; sigma[w][i] = fr_mul(c, kw[p / n], wpow[p % n]); } }
    // polynomials: coefficients = iNTT of the row values, evaluations = NTT of the zero-padded coefficients on the 4n roots
    CtxGuard cg; if (cg_ctx_create(device, &cg.ctx)) die("cg_ctx_create");
    cg_ctx* ctx = cg.ctx;
    auto coef_eval = [&](const std::vector<Fr>& rows, std::vector<Fr>& co, std::vector<Fr>& ev) {
        co = rows; void* v[1] = {co.data()};
        CG(cg_ntt(ctx, c.id, v, 1, n, omega.v, 1, nullptr));
        ev.assign(N, zero); std::copy(co.begin(), co.end(), ev.begin()); void* e[1] = {ev.data()};
        CG(cg_ntt(ctx, c.id, e, 1, N, omega4.v, 0, nullptr));
    };
    // toxic waste: tau; p_tau = [tau^i]_1, i < n + 6; vk = q(tau) G1
    const Fr tau = random_nonzero_fr(c, rng);
    std::vector<Fr> tpow(n + 6); { Fr acc = one; for (auto& t : tpow) { t = acc; acc = fr_mul(c, acc, tau); } }
    auto at_tau = [&](const std::vector<Fr>& co) { Fr acc = zero; for (size_t i = 0; i < co.size(); i++) acc = fr_add(c, acc, fr_mul(c, co[i], tpow[i])); return acc; };
    auto g1 = [&](const Fr& k) { return pt_to_affine(c, pt_mul(c, pt_generator(c, CG_G1), k)); };
    std::vector<Fr> q_co[5], q_ev[5], s_co[3], s_ev[3];
    for (int i = 0; i < 5; i++) coef_eval(q[i], q_co[i], q_ev[i]);
    for (int w = 0; w < 3; w++) coef_eval(sigma[w], s_co[w], s_ev[w]);
    Bytes vk;
    for (int i = 0; i < 5; i++) { Bytes b = g1(at_tau(q_co[i])); vk.insert(vk.end(), b.begin(), b.end()); }
    for (int w = 0; w < 3; w++) { Bytes b = g1(at_tau(s_co[w])); vk.insert(vk.end(), b.begin(), b.end()); }
    const Bytes x2 = pt_to_affine(c, pt_mul(c, pt_generator(c, CG_G2), tau));
    Bytes ptau;
    {
        DevBufGuard d{ctx, nullptr};
        CG(cg_dev_alloc(ctx, tpow.size() * 32, &d.p)); CG(cg_dev_upload(ctx, d.p, tpow.data(), tpow.size() * 32));
        cg_bases* b = nullptr; CG(cg_bases_from_scalars(ctx, c.id, CG_G1, d.p, tpow.size(), &b));
        ptau.resize(tpow.size() * c.aff(CG_G1));
        const int rc = cg_bases_download(ctx, b, 0, tpow.size(), ptau.data());
        cg_bases_release(b);
        if (rc) die("cg_bases_download");
    }
    const size_t psz = c.aff(CG_G1);
    SectionWriter zk(zkey_path, "zkey", 1, 14);
    zk.begin(1, 4); zk.u32(2);                                                               // protocol: plonk
    zk.begin(2, 4 + c.fq() + 4 + 32 + 20 + 64 + 8 * psz + c.aff(CG_G2));
    zk.u32((uint32_t)c.fq()); zk.put(MOD_Q[c.id], c.fq()); zk.u32(32); zk.put(MOD_R[c.id], 32);
    zk.u32((uint32_t)n_vars); zk.u32(n_public); zk.u32((uint32_t)n); zk.u32(n_additions); zk.u32((uint32_t)nc);
    zk.put(k1.v, 32); zk.put(k2.v, 32); zk.put(vk.data(), vk.size()); zk.put(x2.data(), x2.size());
    zk.begin(3, (uint64_t)n_additions * 72);
    for (const auto& e : adds) { zk.u32(e.id1); zk.u32(e.id2); zk.put(e.f1.v, 32); zk.put(e.f2.v, 32); }
    for (int w = 0; w < 3; w++) { zk.begin(4 + w, (uint64_t)nc * 4); zk.put(map[w].data(), nc * 4); }
    for (int i = 0; i < 5; i++) { zk.begin(7 + i, (uint64_t)5 * n * 32); zk.put(q_co[i].data(), n * 32); zk.put(q_ev[i].data(), N * 32); }
    zk.begin(12, (uint64_t)15 * n * 32);
    for (int w = 0; w < 3; w++) { zk.put(s_co[w].data(), n * 32); zk.put(s_ev[w].data(), N * 32); }
    zk.begin(13, (uint64_t)n_public * 5 * n * 32);
    for (size_t j = 0; j < n_public; j++) {
        std::vector<Fr> rows(n, zero), co, ev; rows[j] = one;
        coef_eval(rows, co, ev); zk.put(co.data(), n * 32); zk.put(ev.data(), N * 32);
    }
    zk.begin(14, ptau.size()); zk.put(ptau.data(), ptau.size());
    zk.close();
    const size_t n_wit = n_vars - n_additions;                                              // .wtns: every signal but the additions
    SectionWriter wt(wtns_path, "wtns", 2, 2);
    wt.begin(1, 4 + 32 + 4); wt.u32(32); wt.put(MOD_R[c.id], 32); wt.u32((uint32_t)n_wit);
    wt.begin(2, (uint64_t)n_wit * 32);
    { std::vector<Fr> can(n_wit); CG(cg_fr_to_canonical(c.id, val.data(), can.data(), n_wit)); wt.put(can.data(), n_wit * 32); }
    wt.close();
}

}  // namespace cgh
