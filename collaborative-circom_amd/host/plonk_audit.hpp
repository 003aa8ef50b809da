// What a user of a Plonk key can ask without proving: which gate a plain witness breaks (cg_plonk_gate_check_dev over the session's resident
// maps and selectors), whether the key is the key `plonk setup` writes for its own contents and for a circuit (the audit), and which R1CS
// row a gate row came from.  DESIGN 6g.
#pragma once
#include "plonk_setup.hpp"
#include "plonk_verify.hpp"

namespace cgh {

constexpr uint64_t PLONK_NONE = ~0ull;

// The plain full witness (n_vars - n_additions elements: the leading one, the public inputs, the private witness) against every row of the
// key: upload, the resident addition schedule (one launch per dependency level), then one pass of the gate check over the resident wire
// maps and the selectors on the n rows.  No transform, no MSM, no randomness.  q_rows: n-row copies of the five selectors (every fourth of the
// resident 4n evaluations, gathered once by the session: the kernel is measurably faster on them, profiles/plonk_audit_timing.txt), or
// nullptr to read the evaluations where they lie with a stride of 4.
static void plonk_check_witness(cg_ctx* ctx, const PlonkResident& r, void* const* q_rows, const Fr* full_witness, uint64_t* n_bad, uint64_t* first_bad) {
    const PlonkZKey& z = r.z; const Curve& c = z.curve;
    const size_t n_in = z.n_public + 1, n_ext = r.n_priv + z.n_additions;
    auto dev = [&](size_t bytes) { void* p = nullptr; CG(cg_dev_alloc(ctx, std::max<size_t>(bytes, 32), &p)); return p; };
    DevBufGuard pub{ctx, dev(n_in * 32)}, ext{ctx, dev(n_ext * 32)}, res{ctx, dev(16)};
    std::vector<Fr> p(full_witness, full_witness + n_in);
    p[0] = fr_from_u64(c, 0);                                                              // types.rs:107-109, as CoPlonk forces it
    CG(cg_dev_upload(ctx, pub.p, p.data(), n_in * 32));
    if (r.n_priv) CG(cg_dev_upload(ctx, ext.p, full_witness + n_in, r.n_priv * 32));
    for (size_t l = 0; l + 1 < r.level_off.size(); l++)
        CG(cg_plonk_additions_dev(ctx, c.id, r.add_order + r.level_off[l], r.level_off[l + 1] - r.level_off[l], r.add_ids, r.add_coef, pub.p, (uint32_t)n_in, 0, ext.p, nullptr, r.n_priv));
    const uint32_t* maps[3] = {r.col[0], r.col[1], r.col[2]};
    const void* q[5];
    for (int i = 0; i < 5; i++) q[i] = q_rows ? q_rows[i] : r.q_eval[i];
    CG(cg_plonk_gate_check_dev(ctx, c.id, maps, z.n_constraints, q, q_rows ? 1 : 4, z.domain_size, pub.p, (uint32_t)z.n_public, ext.p, z.n_vars, res.p));
    uint64_t out[2];
    CG(cg_dev_download(ctx, out, res.p, 16));
    *n_bad = out[0]; *first_bad = out[1];
}

// Where gate row `gate_row` of the circuit's Plonk key comes from, read off the count pass's offsets (host work after that pass):
// out3 = kind (CGH_PLONK_GATE_*), the R1CS row, the index of the addition within that row; 2^64 - 1 where a field does not apply.
static void r1cs_plonk_gate_origin(R1csHandle& h, int device, uint64_t gate_row, uint64_t* out3) {
    std::lock_guard<std::mutex> lock(h.mu);
    R1csDevice& d = plonk_device(h, device);
    const size_t rows = h.r.n_constraints, n_pub = h.r.n_public;
    void* cp = nullptr; void* op = nullptr;
    CG(cg_dev_alloc(d.ctx, (rows + 1) * 4, &cp)); DevBufGuard counts{d.ctx, cp};
    CG(cg_dev_alloc(d.ctx, (rows + 1) * 4, &op)); DevBufGuard offsets{d.ctx, op};
    const PlonkPlan pl = plonk_plan(h, d, counts.p, offsets.p);
    if (gate_row >= pl.n) throw std::runtime_error("plonk gate origin: row " + std::to_string(gate_row) + " lies outside the domain of " + std::to_string(pl.n) + " rows");
    out3[1] = out3[2] = PLONK_NONE;
    if (gate_row < n_pub) { out3[0] = CGH_PLONK_GATE_PUBLIC; return; }
    if (gate_row >= pl.n_constraints) { out3[0] = CGH_PLONK_GATE_PADDING; return; }
    std::vector<uint32_t> off(rows + 1);
    CG(cg_dev_download(d.ctx, off.data(), offsets.p, (rows + 1) * 4));
    // R1CS row i owns the gate rows n_pub + i + off[i] .. n_pub + i + off[i + 1]: its additions, then its own gate (the starts ascend strictly)
    const uint64_t g = gate_row - n_pub;
    size_t lo = 0, hi = rows;                                                               // the last i with i + off[i] <= g
    while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if ((uint64_t)mid + off[mid] <= g) lo = mid; else hi = mid; }
    const uint64_t j = g - (lo + off[lo]), n_add = off[lo + 1] - off[lo];
    out3[1] = lo;
    if (j < n_add) { out3[0] = CGH_PLONK_GATE_ADDITION; out3[2] = j; } else out3[0] = CGH_PLONK_GATE_CONSTRAINT;
}

// ---- the audit -------------------------------------------------------------------------------------------------------------------------
// A Plonk key is a deterministic function of its circuit and of the SRS inside it, so all of it can be checked without a secret.  Every
// check but BLOCKS reads the COEFFICIENT forms, brought to the n rows by one forward n-point transform each; BLOCKS alone ties the 4n
// evaluations to the coefficients.  The checks are therefore independent: one defect sets predictable bits.  detail[2 * k], detail[2 * k + 1]
// for check k (bit 1 << k): which polynomial (0 .. 4 = Qm, Ql, Qr, Qo, Qc, 5 .. 7 = S1 .. S3, 8 + j = Lagrange j), zkey section or SRS part,
// and the first offending index; both 2^64 - 1 for a check that passed.
// stage_seconds (optional, PLONK_AUDIT_STAGES): header, transforms, comparisons, eight MSMs, two SRS MSMs, pairing, circuit.
constexpr int PLONK_AUDIT_STAGES = 7;
struct PlonkAudit {
    cg_ctx* ctx; const PlonkResident& r; const PlonkZKey& z; const Curve c; const size_t n, N, nc;
    uint32_t failed = 0; uint64_t* detail;
    DevBufGuard res;
    double stage[PLONK_AUDIT_STAGES] = {0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t_last;

    PlonkAudit(cg_ctx* cx, const PlonkResident& rs, uint64_t* det) : ctx(cx), r(rs), z(rs.z), c(rs.z.curve), n(rs.z.domain_size), N(4 * rs.z.domain_size), nc(rs.z.n_constraints),
                                                                      detail(det), res{cx, nullptr} {
        for (int i = 0; i < 2 * CGH_PLONK_AUDIT_CHECKS; i++) detail[i] = PLONK_NONE;
        res.p = dev(16);
        t_last = std::chrono::steady_clock::now();
    }
    void* dev(size_t bytes) { void* p = nullptr; CG(cg_dev_alloc(ctx, std::max<size_t>(bytes, 32), &p)); return p; }
    void lap(int i) { CG(cg_ctx_sync(ctx)); const auto t = std::chrono::steady_clock::now(); stage[i] += std::chrono::duration<double>(t - t_last).count(); t_last = t; }
    static int bit_index(uint32_t bit) { int k = 0; while (!((bit >> k) & 1)) k++; return k; }
    void fail(uint32_t bit, uint64_t which, uint64_t index) {                               // the first finding of a check is the one reported
        if (!(failed & bit)) { detail[2 * bit_index(bit)] = which; detail[2 * bit_index(bit) + 1] = index; }
        failed |= bit;
    }
    // cg_vec_mismatch_dev and its answer; b == nullptr: a against zero
    bool differ(uint32_t bit, uint64_t which, const void* a, size_t a_stride, const void* b, size_t b_stride, size_t first, size_t len) {
        CG(cg_vec_mismatch_dev(ctx, c.id, a, a_stride, b, b_stride, first, len, res.p));
        uint64_t out[2]; CG(cg_dev_download(ctx, out, res.p, 16));
        if (out[0]) fail(bit, which, out[1]);
        return out[0] != 0;
    }
    const void* coef_of(size_t p) const { return p < 5 ? r.q_coef[p] : p < 8 ? r.sigma_coef[p - 5] : (const uint8_t*)r.lagrange_coef + (p - 8) * n * 32; }
    const void* eval_of(size_t p) const { return p < 5 ? r.q_eval[p] : p < 8 ? r.sigma_eval[p - 5] : (const uint8_t*)r.lagrange + (p - 8) * N * 32; }

    // HEADER.  Throws where the sizes are meaningless and nothing else could be checked.
    std::vector<uint32_t> maps;                                                             // 3 x nc, from the device copy
    void header() {
        const size_t psz = c.aff(CG_G1), fq = c.fq();
        if (nc > n) throw std::runtime_error("plonk audit: the key has " + std::to_string(nc) + " gates on a domain of " + std::to_string(n) + " rows");
        Fr k1, k2; plonk_coset_shifts(c, n, k1, k2);
        if (!fr_eq(k1, z.k1)) fail(CGH_PLONK_AUDIT_HEADER, 2, 0);
        if (!fr_eq(k2, z.k2)) fail(CGH_PLONK_AUDIT_HEADER, 2, 1);
        const std::pair<uint32_t, size_t> want[] = {{2, 4 + fq + 4 + 32 + 20 + 64 + 8 * psz + c.aff(CG_G2)}, {3, z.n_additions * 72}, {4, nc * 4}, {5, nc * 4}, {6, nc * 4},
                                                    {7, 5 * n * 32}, {8, 5 * n * 32}, {9, 5 * n * 32}, {10, 5 * n * 32}, {11, 5 * n * 32}, {12, 15 * n * 32},
                                                    {13, z.n_public * 5 * n * 32}, {14, (n + 6) * psz}};
        for (const auto& w : want) { const auto it = z.section_bytes.find(w.first); if (it == z.section_bytes.end() || it->second != w.second) fail(CGH_PLONK_AUDIT_HEADER, w.first, it == z.section_bytes.end() ? 0 : it->second); }
        // (an addition that reads anything but an input or an earlier addition is refused when the session opens: PlonkResident::schedule_additions)
        maps.resize(3 * nc);
        for (int w = 0; w < 3; w++) if (nc) CG(cg_dev_download(ctx, maps.data() + w * nc, r.col[w], nc * 4));
        for (int w = 0; w < 3; w++) for (size_t i = 0; i < nc; i++)
            if (maps[w * nc + i] >= z.n_vars) throw std::runtime_error("plonk audit: map " + std::to_string(w) + " names wire " + std::to_string(maps[w * nc + i]) + " at row " + std::to_string(i) + " of " + std::to_string(z.n_vars) + " variables");
        lap(0);
    }
    // BLOCKS for the polynomials p0 .. p0 + k (k <= 8) and their values on the n rows into rows[j] (n elements each)
    void to_rows(size_t p0, int k, void* rows_buf, void* evals_buf, const Fr& omega, const Fr& omega4) {
        void* v[8]; void* e[8];
        for (int j = 0; j < k; j++) { v[j] = (uint8_t*)rows_buf + (size_t)j * n * 32; e[j] = (uint8_t*)evals_buf + (size_t)j * N * 32; }
        CG(cg_dev_memset_zero(ctx, evals_buf, (size_t)k * N * 32));
        for (int j = 0; j < k; j++) { CG(cg_vec_gather_strided_dev(ctx, c.id, e[j], coef_of(p0 + j), n, 0, 1)); CG(cg_vec_gather_strided_dev(ctx, c.id, v[j], coef_of(p0 + j), n, 0, 1)); }
        CG(cg_ntt_dev(ctx, c.id, e, k, N, omega4.v, 0, nullptr));
        CG(cg_ntt_dev(ctx, c.id, v, k, n, omega.v, 0, nullptr));
        lap(1);
        for (int j = 0; j < k; j++) differ(CGH_PLONK_AUDIT_BLOCKS, p0 + j, e[j], 1, eval_of(p0 + j), 1, 0, N);
        lap(2);
    }
    void sigma(const void* rows_buf, const Fr& omega) {
        const uint32_t none = 0xffffffffu;                                                  // rows then columns, as setup_plonk_tau_dev
        std::vector<uint32_t> prev(3 * n), first(z.n_vars, none), last(z.n_vars, none);
        for (size_t i = 0; i < n; i++) for (size_t w = 0; w < 3; w++) {
            const uint32_t s = i < nc ? maps[w * nc + i] : 0, p = (uint32_t)(w * n + i);
            if (last[s] == none) first[s] = p; else prev[p] = last[s];
            last[s] = p;
        }
        for (size_t s = 0; s < z.n_vars; s++) if (first[s] != none) prev[first[s]] = last[s];
        const Fr one = fr_from_u64(c, 1);
        DevBufGuard d_prev{ctx, dev_copy_of(ctx, prev.data(), prev.size() * 4)}, wpow{ctx, dev(n * 32)}, labels{ctx, dev(3 * n * 32)};
        CG(cg_vec_fill_dev(ctx, c.id, wpow.p, n, one.v));
        CG(cg_vec_distribute_powers_dev(ctx, c.id, wpow.p, n, omega.v, one.v));
        CG(cg_plonk_sigma_labels_dev(ctx, c.id, (const uint32_t*)d_prev.p, wpow.p, n, z.k1.v, z.k2.v, labels.p));
        for (size_t w = 0; w < 3; w++) differ(CGH_PLONK_AUDIT_SIGMA, 5 + w, (const uint8_t*)rows_buf + (5 + w) * n * 32, 1, (const uint8_t*)labels.p + w * n * 32, 1, 0, n);
        CG(cg_ctx_sync(ctx));
    }
    void commitments() {
        const size_t psz = c.aff(CG_G1);
        for (size_t i = 0; i < 8; i++) {
            const void* sc[1] = {coef_of(i)};
            Point p{Bytes(c.jac(CG_G1)), CG_G1};
            CG(cg_msm_dev(ctx, r.tau, 0, n, sc, 1, p.b.data()));
            const Bytes a = pt_to_affine(c, p);
            if (memcmp(a.data(), z.vk_g1.data() + i * psz, psz)) fail(CGH_PLONK_AUDIT_COMMITMENTS, i, PLONK_NONE);
        }
        lap(3);
    }
    // p_tau[i] = tau^i G_1 for one tau with X_2 = tau G_2: e(sum rho_i P_(i+1), G_2) e(-sum rho_i P_i, X_2) = 1 over i < n + 5
    void srs(const uint8_t* seed32) {
        const size_t psz = c.aff(CG_G1), m = n + 5;
        Bytes p0(psz); CG(cg_bases_download(ctx, r.tau, 0, 1, p0.data()));
        if (p0 != pt_to_affine(c, pt_generator(c, CG_G1))) fail(CGH_PLONK_AUDIT_SRS, 0, 0);
        uint8_t seed[32];                                                                   // drawn as plonk_verify_batch draws its coefficients
        if (seed32) memcpy(seed, seed32, 32);
        else { std::random_device rd; for (int i = 0; i < 8; i++) { const uint32_t w = rd(); memcpy(seed + 4 * i, &w, 4); } }
        ChaCha12 rng(seed);
        std::vector<Fr> rho(m), rho_m(m);
        for (size_t i = 0; i < m; i++) { rho[i].v[0] = i ? rng.next_u64() : 1; rho[i].v[1] = i ? rng.next_u64() : 0; rho[i].v[2] = rho[i].v[3] = 0; }
        CG(cg_fr_from_canonical(c.id, rho.data(), rho_m.data(), m));
        DevBufGuard d_rho{ctx, dev_copy_of(ctx, rho_m.data(), m * 32)};
        const void* sc[1] = {d_rho.p};
        Point hi{Bytes(c.jac(CG_G1)), CG_G1}, lo{Bytes(c.jac(CG_G1)), CG_G1};
        CG(cg_msm_dev(ctx, r.tau, 1, m, sc, 1, hi.b.data()));
        CG(cg_msm_dev(ctx, r.tau, 0, m, sc, 1, lo.b.data()));
        lap(4);
        int32_t x2_ok = 0; CG(cg_point_validate(c.id, CG_G2, z.x_2.data(), &x2_ok));
        int32_t ok = 0;
        if (x2_ok) {
            Bytes g1s = pt_to_affine(c, hi), g2s = pt_to_affine(c, pt_generator(c, CG_G2));
            const Bytes nlo = pt_to_affine(c, pt_neg(c, lo));
            g1s.insert(g1s.end(), nlo.begin(), nlo.end()); g2s.insert(g2s.end(), z.x_2.begin(), z.x_2.end());
            CG(cg_pairing_check(c.id, g1s.data(), g2s.data(), 2, &ok));
        }
        if (!ok) fail(CGH_PLONK_AUDIT_SRS, 1, PLONK_NONE);
        lap(5);
    }
    // the key against a fresh run of the gate compiler for the circuit: header numbers, sections 3 - 6, the five selectors on the rows.
    // The compiler runs on the handle's own context (same device); its outputs are complete before this context reads them.
    void circuit(R1csHandle& h, const void* rows_buf) {
        std::lock_guard<std::mutex> lock(h.mu);
        const R1cs& rc = h.r;
        if (rc.curve.id != c.id) { fail(CGH_PLONK_AUDIT_CIRCUIT, 2, PLONK_NONE); return; }
        R1csDevice& d = plonk_device(h, cg_ctx_device(ctx));
        cg_ctx* cx = d.ctx;
        auto rdev = [&](size_t bytes) { void* p = nullptr; CG(cg_dev_alloc(cx, std::max<size_t>(bytes, 32), &p)); return p; };
        const size_t rows = rc.n_constraints;
        DevBufGuard counts{cx, rdev((rows + 1) * 4)}, offsets{cx, rdev((rows + 1) * 4)};
        const PlonkPlan pl = plonk_plan(h, d, counts.p, offsets.p);
        const size_t have[5] = {z.n_vars, z.n_public, n, z.n_additions, nc}, want[5] = {pl.n_vars, rc.n_public, pl.n, pl.n_additions, pl.n_constraints};
        for (int i = 0; i < 5; i++) if (have[i] != want[i]) { fail(CGH_PLONK_AUDIT_CIRCUIT, 2, (uint64_t)i); return; }
        const size_t n_add = pl.n_additions;
        DevBufGuard fm{cx, rdev(3 * nc * 4)}, fq{cx, rdev(5 * n * 32)}, ids{cx, rdev(2 * n_add * 4)}, fs{cx, rdev(2 * n_add * 32)};
        {
            const PlonkCsrArgs a = plonk_csr_args(d);
            uint32_t* mp[3]; void* q[5];
            for (int w = 0; w < 3; w++) mp[w] = (uint32_t*)fm.p + w * nc;
            for (int i = 0; i < 5; i++) q[i] = (uint8_t*)fq.p + (size_t)i * n * 32;
            CG(cg_plonk_gates_emit_dev(cx, c.id, a.rp, a.cl, a.co, rows, rc.n_wires, rc.n_public, (const uint32_t*)counts.p, (const uint32_t*)offsets.p, n_add, n, mp, q, (uint32_t*)ids.p, fs.p));
            CG(cg_ctx_sync(cx));
        }
        // the integer sections (4 bytes an entry) are compared here, the field data on the device
        std::vector<uint32_t> ids_f(2 * n_add), ids_k(2 * n_add), maps_f(3 * nc);
        if (n_add) { CG(cg_dev_download(cx, ids_f.data(), ids.p, 2 * n_add * 4)); CG(cg_dev_download(ctx, ids_k.data(), r.add_ids, 2 * n_add * 4)); }
        for (size_t i = 0; i < 2 * n_add; i++) if (ids_f[i] != ids_k[i]) { fail(CGH_PLONK_AUDIT_CIRCUIT, 3, i / 2); break; }
        {   // two factors per addition: the index reported is the addition's
            CG(cg_vec_mismatch_dev(ctx, c.id, r.add_coef, 1, fs.p, 1, 0, 2 * n_add, res.p));
            uint64_t out[2]; CG(cg_dev_download(ctx, out, res.p, 16));
            if (out[0]) fail(CGH_PLONK_AUDIT_CIRCUIT, 3, out[1] / 2);
        }
        if (nc) CG(cg_dev_download(cx, maps_f.data(), fm.p, 3 * nc * 4));
        for (size_t w = 0; w < 3; w++) for (size_t i = 0; i < nc; i++) if (maps_f[w * nc + i] != maps[w * nc + i]) { fail(CGH_PLONK_AUDIT_CIRCUIT, 4 + w, i); i = nc; }
        for (size_t i = 0; i < 5; i++) differ(CGH_PLONK_AUDIT_CIRCUIT, 7 + i, (const uint8_t*)rows_buf + i * n * 32, 1, (const uint8_t*)fq.p + i * n * 32, 1, 0, n);
        CG(cg_ctx_sync(ctx));
    }
};

static void plonk_audit(cg_ctx* ctx, const PlonkResident& r, R1csHandle* r1cs, const uint8_t* seed32, uint32_t* failed, uint64_t* detail, double* stage_seconds) {
    PlonkAudit a(ctx, r, detail);
    const PlonkZKey& z = r.z; const Curve c = z.curve; const size_t n = a.n, N = a.N;
    a.header();
    const SnarkjsRoots& rt = snarkjs_roots_cached(c);
    const Fr omega = rt.roots[z.power], omega4 = rt.roots[z.power + 2], one = fr_from_u64(c, 1), zero = fr_from_u64(c, 0);
    DevBufGuard rows8{ctx, a.dev(8 * n * 32)}, rows_l{ctx, a.dev(8 * n * 32)}, evals{ctx, a.dev(8 * N * 32)}, unit{ctx, a.dev(n * 32)};
    a.to_rows(0, 8, rows8.p, evals.p, omega, omega4);
    // ROWS: the selectors vanish on the padding rows; Lagrange polynomial j is the unit vector of row j
    for (size_t i = 0; i < 5; i++) a.differ(CGH_PLONK_AUDIT_ROWS, i, (const uint8_t*)rows8.p + i * n * 32, 1, nullptr, 1, a.nc, n);
    a.sigma(rows8.p, omega);
    a.lap(2);
    CG(cg_dev_memset_zero(ctx, unit.p, n * 32));
    for (size_t j0 = 0; j0 < z.n_public; j0 += 8) {
        const int k = (int)std::min<size_t>(8, z.n_public - j0);
        a.to_rows(8 + j0, k, rows_l.p, evals.p, omega, omega4);
        for (int j = 0; j < k; j++) {
            CG(cg_dev_upload(ctx, (uint8_t*)unit.p + (j0 + j) * 32, one.v, 32));
            a.differ(CGH_PLONK_AUDIT_ROWS, 8 + j0 + j, (const uint8_t*)rows_l.p + (size_t)j * n * 32, 1, unit.p, 1, 0, n);
            CG(cg_dev_upload(ctx, (uint8_t*)unit.p + (j0 + j) * 32, zero.v, 32));
        }
        a.lap(2);
    }
    a.commitments();
    a.srs(seed32);
    if (r1cs) { a.circuit(*r1cs, rows8.p); a.lap(6); }
    *failed = a.failed;
    if (stage_seconds) std::copy(a.stage, a.stage + PLONK_AUDIT_STAGES, stage_seconds);
}

}  // namespace cgh
