// iden3 .r1cs reader, the zkey coefficient section it determines, the witness check on the GPU and a Groth16 development setup
// (format: circom-types/src/r1cs.rs is its specification in the reference, used there by split-witness for num_inputs)
#pragma once
#include "synth.hpp"

namespace cgh {

// ---- .r1cs, version 1 ------------------------------------------------------------------------------------------------------------------
// "r1cs" | u32 version | u32 sections | (u32 id, u64 bytes, payload)*.  Section 1: u32 field bytes, prime, u32 nWires, nPubOut, nPubIn,
// nPrvIn, u64 nLabels, u32 nConstraints.  Section 2: per constraint the linear combinations A, B, C, each u32 n | (u32 wire, value)^n with
// canonical little-endian values.  Section 3 (wire -> label) and unknown sections are skipped by their length.
struct R1cs {
    Curve curve;
    size_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, n_constraints = 0, n_public = 0, domain_size = 1, pow = 0;
    uint64_t n_labels = 0;
    std::vector<uint32_t> row_ptr[3], col[3];       // A, B, C in the file's term order
    std::vector<Fr> coeff[3];                        // Montgomery
};
static bool fr_raw_below_modulus(int curve_id, const uint64_t* v) {
    for (int i = 3; i >= 0; i--) { if (v[i] < MOD_R[curve_id][i]) return true; if (v[i] > MOD_R[curve_id][i]) return false; }
    return false;
}
static R1cs read_r1cs(int curve_id, const std::string& path) {
    if (curve_id != CG_BN254 && curve_id != CG_BLS12_381) throw std::runtime_error("r1cs: unknown curve");
    MappedFile mf(path);                                                         // (the descriptor is closed once mapped; unmapped on every way out)
    Cursor cur{mf.p, mf.n};
    if (mf.n < 12 || memcmp(mf.p, "r1cs", 4)) throw std::runtime_error("r1cs: not an r1cs file (magic)");
    cur.off = 4;
    const uint32_t version = cur.u32();
    if (version != 1) throw std::runtime_error("r1cs: version " + std::to_string(version) + " is not supported (1 is)");
    const uint32_t ns = cur.u32();
    Cursor sec[3] = {{nullptr, 0}, {nullptr, 0}, {nullptr, 0}};
    for (uint32_t i = 0; i < ns; i++) {
        if (cur.n - cur.off < 12) throw std::runtime_error("r1cs: section table ends outside the file");
        const uint32_t id = cur.u32(); const uint64_t len = cur.u64();
        if (len > cur.n - cur.off) throw std::runtime_error("r1cs: section " + std::to_string(id) + " ends outside the file");
        if (id == 1 || id == 2) {
            if (sec[id].p) throw std::runtime_error("r1cs: duplicate section " + std::to_string(id));
            sec[id] = Cursor{mf.p + cur.off, (size_t)len};
        }
        cur.off += (size_t)len;
    }
    if (!sec[1].p) throw std::runtime_error("r1cs: missing header section (1)");
    if (!sec[2].p) throw std::runtime_error("r1cs: missing constraint section (2)");
    R1cs r; r.curve = Curve{curve_id};
    {
        Cursor h = sec[1];
        if (h.n < 4) throw std::runtime_error("r1cs: header section too short");
        const uint32_t fs = h.u32();
        if (fs != 32) throw std::runtime_error("r1cs: field size " + std::to_string(fs) + ", expected 32");
        if (h.n != 64) throw std::runtime_error("r1cs: header section of " + std::to_string(h.n) + " bytes, expected 64");
        uint64_t prime[4]; h.bytes(prime, 32);
        if (memcmp(prime, MOD_R[curve_id], 32)) throw std::runtime_error("r1cs: the prime is not the curve's scalar field");
        r.n_wires = h.u32(); r.n_pub_out = h.u32(); r.n_pub_in = h.u32(); r.n_prv_in = h.u32(); r.n_labels = h.u64(); r.n_constraints = h.u32();
        r.n_public = r.n_pub_out + r.n_pub_in;
        if (r.n_public + 1 > r.n_wires) throw std::runtime_error("r1cs: " + std::to_string(r.n_public) + " public signals and the constant do not fit " + std::to_string(r.n_wires) + " wires");
    }
    while (r.domain_size < r.n_constraints + r.n_public + 1) { r.domain_size <<= 1; r.pow++; }      // groth16_domain's size
    {   // two passes over the constraint section: sizes and checks, then the fill
        Cursor s = sec[2];
        size_t nnz[3] = {0, 0, 0};
        for (size_t c = 0; c < r.n_constraints; c++) for (int m = 0; m < 3; m++) {
            if (s.n - s.off < 4) throw std::runtime_error("r1cs: constraint " + std::to_string(c) + " starts past the end of its section");
            const uint32_t n = s.u32();
            if ((uint64_t)n * 36 > s.n - s.off) throw std::runtime_error("r1cs: term count of constraint " + std::to_string(c) + " runs past its section");
            for (uint32_t t = 0; t < n; t++) {
                uint32_t wire; uint64_t v[4];
                memcpy(&wire, s.p + s.off, 4); memcpy(v, s.p + s.off + 4, 32); s.off += 36;
                if (wire >= r.n_wires) throw std::runtime_error("r1cs: wire " + std::to_string(wire) + " in constraint " + std::to_string(c) + " is not below nWires");
                if (!fr_raw_below_modulus(curve_id, v)) throw std::runtime_error("r1cs: coefficient in constraint " + std::to_string(c) + " is not below the modulus");
            }
            nnz[m] += n;
            if (nnz[m] >> 32) throw std::runtime_error("r1cs: more than 2^32 terms in one matrix");
        }
        if (s.off != s.n) throw std::runtime_error("r1cs: constraint section is longer than its constraints");
        s.off = 0;
        std::vector<Fr> raw[3];
        for (int m = 0; m < 3; m++) { r.row_ptr[m].assign(r.n_constraints + 1, 0); r.col[m].resize(nnz[m]); raw[m].resize(nnz[m]); r.coeff[m].resize(nnz[m]); }
        size_t k[3] = {0, 0, 0};
        for (size_t c = 0; c < r.n_constraints; c++) for (int m = 0; m < 3; m++) {
            const uint32_t n = s.u32();
            for (uint32_t t = 0; t < n; t++, k[m]++) { memcpy(&r.col[m][k[m]], s.p + s.off, 4); memcpy(raw[m][k[m]].v, s.p + s.off + 4, 32); s.off += 36; }
            r.row_ptr[m][c + 1] = (uint32_t)k[m];
        }
        for (int m = 0; m < 3; m++) if (nnz[m]) CG(cg_fr_from_canonical(curve_id, raw[m].data(), r.coeff[m].data(), nnz[m]));
    }
    return r;
}

// Section 4 of the Groth16 zkey this R1CS determines (zkey.rs:184-204): u32 count, then (u32 matrix, u32 row, u32 wire, value) with
// value = coef * R^2 (the Montgomery form of the Montgomery form).  Per constraint its A terms then its B terms, in the file's order;
// after the last constraint the rows A[nC + s][s] = 1, s = 0 .. nPublic.  Byte-equal to what snarkjs wrote into the shipped keys.
static Bytes r1cs_coeff_section(const R1cs& r) {
    const size_t n_inp = r.n_public + 1, ncoef = r.col[0].size() + r.col[1].size() + n_inp;
    if (ncoef >> 32) throw std::runtime_error("r1cs: coefficient section beyond 2^32 records");
    std::vector<Fr> twice[2];
    for (int m = 0; m < 2; m++) { twice[m].resize(r.coeff[m].size()); if (!twice[m].empty()) CG(cg_fr_from_canonical(r.curve.id, r.coeff[m].data(), twice[m].data(), twice[m].size())); }
    const Fr one = fr_from_u64(r.curve, 1); Fr one2; CG(cg_fr_from_canonical(r.curve.id, one.v, one2.v, 1));
    Bytes out(4 + ncoef * 44);
    uint8_t* p = out.data();
    auto u32 = [&](uint32_t x) { memcpy(p, &x, 4); p += 4; };
    auto rec = [&](uint32_t mat, uint32_t row, uint32_t wire, const Fr& v) { u32(mat); u32(row); u32(wire); memcpy(p, v.v, 32); p += 32; };
    u32((uint32_t)ncoef);
    for (size_t c = 0; c < r.n_constraints; c++) for (int m = 0; m < 2; m++)
        for (uint32_t k = r.row_ptr[m][c]; k < r.row_ptr[m][c + 1]; k++) rec((uint32_t)m, (uint32_t)c, r.col[m][k], twice[m][k]);
    for (size_t s = 0; s < n_inp; s++) rec(0, (uint32_t)(r.n_constraints + s), (uint32_t)s, one2);
    return out;
}

// ---- the handle behind cgh_r1cs_*: the parsed file and, per device it was checked on, a context with the three CSR matrices resident ----
struct R1csDevice {
    cg_ctx* ctx = nullptr;
    void* row_ptr[3] = {nullptr, nullptr, nullptr}; void* col[3] = {nullptr, nullptr, nullptr}; void* coeff[3] = {nullptr, nullptr, nullptr};
    void* witness = nullptr; void* result = nullptr;
    void* canon_row_ptr[3] = {nullptr, nullptr, nullptr}; void* canon_col[3] = {nullptr, nullptr, nullptr}; void* canon_coeff[3] = {nullptr, nullptr, nullptr};   // plonk_setup.hpp
};
// the matrices in the canonical form of the Plonk gate compiler (plonk_setup.hpp): inside a row the wires ascend, a wire named twice is one
// term, no coefficient is zero.  Built at the first Plonk call on the handle.
struct R1csCanonical { bool built = false; std::vector<uint32_t> row_ptr[3], col[3]; std::vector<Fr> coeff[3]; };
struct R1csHandle {
    R1cs r;
    R1csCanonical canon;
    std::mutex mu;
    std::map<int, R1csDevice> dev;
    ~R1csHandle() {
        for (auto& kv : dev) {
            R1csDevice& d = kv.second;
            for (int m = 0; m < 3; m++) for (void* p : {d.row_ptr[m], d.col[m], d.coeff[m], d.canon_row_ptr[m], d.canon_col[m], d.canon_coeff[m]}) if (p) cg_dev_free(d.ctx, p);
            if (d.witness) cg_dev_free(d.ctx, d.witness);
            if (d.result) cg_dev_free(d.ctx, d.result);
            if (d.ctx) cg_ctx_destroy(d.ctx);
        }
    }
};
static void* dev_copy_of(cg_ctx* ctx, const void* src, size_t bytes) {          // (an empty array still gets an address: 16 bytes)
    void* p = nullptr;
    CG(cg_dev_alloc(ctx, std::max<size_t>(bytes, 16), &p));
    if (bytes && cg_dev_upload(ctx, p, src, bytes)) { cg_dev_free(ctx, p); die("cg_dev_upload"); }
    return p;
}
// The plain, full witness (n_wires Montgomery elements, wire 0 = one) against every constraint, in one kernel pass: the number of rows with
// <A_i,w> * <B_i,w> != <C_i,w> and the smallest such row (2^64 - 1: none).  The CSR goes up once per handle and device.  Secret-shared
// witnesses are out of scope: the product of two shared sums needs a protocol round.
static void r1cs_check_witness(R1csHandle& h, int device, int form, const Fr* witness, uint64_t* n_bad, uint64_t* first_bad) {
    std::lock_guard<std::mutex> lock(h.mu);
    const R1cs& r = h.r;
    R1csDevice& d = h.dev[device];                       // (a half-made entry is finished by the next call or freed with the handle)
    if (!d.ctx && cg_ctx_create(device, &d.ctx)) { d.ctx = nullptr; die("cg_ctx_create"); }
    for (int m = 0; m < 3; m++) {
        if (!d.row_ptr[m]) d.row_ptr[m] = dev_copy_of(d.ctx, r.row_ptr[m].data(), r.row_ptr[m].size() * 4);
        if (!d.col[m]) d.col[m] = dev_copy_of(d.ctx, r.col[m].data(), r.col[m].size() * 4);
        if (!d.coeff[m]) d.coeff[m] = dev_copy_of(d.ctx, r.coeff[m].data(), r.coeff[m].size() * 32);
    }
    if (!d.witness) CG(cg_dev_alloc(d.ctx, std::max<size_t>(r.n_wires * 32, 16), &d.witness));
    if (!d.result) CG(cg_dev_alloc(d.ctx, 16, &d.result));
    CG(cg_dev_upload(d.ctx, d.witness, witness, r.n_wires * 32));
    const uint32_t* rp[3]; const uint32_t* cl[3]; const void* co[3];
    for (int m = 0; m < 3; m++) { rp[m] = (const uint32_t*)d.row_ptr[m]; cl[m] = (const uint32_t*)d.col[m]; co[m] = d.coeff[m]; }
    CG(cg_r1cs_check_dev(d.ctx, r.curve.id, rp, cl, co, r.n_constraints, r.col[0].size() + r.col[1].size() + r.col[2].size(), form, d.witness, d.result));
    uint64_t res[2];
    CG(cg_dev_download(d.ctx, res, d.result, 16));
    *n_bad = res[0]; *first_bad = res[1];
}

// ---- Groth16 development setup -----------------------------------------------------------------------------------------------------
// tau, alpha, beta, gamma, delta: the first five draws of synth_circuit's generator for this seed (Montgomery)
static void setup_toxic(const Curve& c, uint64_t seed, Fr out[5]) {
    SplitMix rng{seed * 0x2545f4914f6cdd1dull + 0x1234567};
    for (int i = 0; i < 5; i++) out[i] = random_nonzero_fr(c, rng);
}
// column-major form of a constraint matrix over n_wires columns; `extra` appends the rows A[nC + s][s] = 1, s < extra
struct Csc { std::vector<uint32_t> col_ptr, row; std::vector<Fr> coeff; };
static Csc r1cs_transpose(const R1cs& r, int m, size_t extra) {
    Csc t; t.col_ptr.assign(r.n_wires + 1, 0);
    for (uint32_t w : r.col[m]) t.col_ptr[w + 1]++;
    for (size_t s = 0; s < extra; s++) t.col_ptr[s + 1]++;
    for (size_t i = 0; i < r.n_wires; i++) t.col_ptr[i + 1] += t.col_ptr[i];
    t.row.resize(t.col_ptr.back()); t.coeff.resize(t.row.size());
    std::vector<uint32_t> fill(t.col_ptr.begin(), t.col_ptr.end() - 1);
    for (size_t c = 0; c < r.n_constraints; c++) for (uint32_t k = r.row_ptr[m][c]; k < r.row_ptr[m][c + 1]; k++) { const uint32_t at = fill[r.col[m][k]]++; t.row[at] = (uint32_t)c; t.coeff[at] = r.coeff[m][k]; }
    const Fr one = fr_from_u64(r.curve, 1);
    for (size_t s = 0; s < extra; s++) { const uint32_t at = fill[s]++; t.row[at] = (uint32_t)(r.n_constraints + s); t.coeff[at] = one; }
    return t;
}
// A snarkjs-format Groth16 .zkey (sections 1-9: the layout synth_circuit writes and read_zkey parses) for the circuit of an .r1cs, from seeded
// toxic waste.  FOR DEVELOPMENT ONLY: whoever holds the seed holds tau .. delta and can forge proofs for the key.
// On the device: w^j (fill + distribute_powers), L_j(tau) = (tau^m - 1) w^j / (m (tau - w^j)) and the H exponents
// (tau^2m - 1) g w^i / (2 m delta (tau - g w^i)) by affine maps, cg_vec_inverse_dev and products; the three column sums u, v, w by
// cg_qap_columns_dev (A with the public rows A[nC + i][i] = 1); (beta u_i + alpha v_i + w_i) / gamma or / delta by a linear combination and
// two affine maps; the five tables by cg_bases_from_scalars.
static void setup_groth16_dev(int device, const R1cs& r, uint64_t seed, const std::string& zkey_path) {
    const Curve c = r.curve;
    const size_t m = r.domain_size, nc = r.n_constraints, n_pub = r.n_public, n_inp = n_pub + 1, n_vars = r.n_wires;
    if (m >> 32) throw std::runtime_error("setup: domain beyond 2^32");
    Fr toxic[5]; setup_toxic(c, seed, toxic);
    const Fr tau = toxic[0], alpha = toxic[1], beta = toxic[2], gamma = toxic[3], delta = toxic[4];
    const Domain dom = groth16_domain(c, r.pow, nc, n_inp);
    const Fr one = fr_from_u64(c, 1), zero = fr_sub(c, one, one);
    Fr tau_m = tau; for (size_t i = 0; i < r.pow; i++) tau_m = fr_mul(c, tau_m, tau_m);
    const Fr tau_2m = fr_mul(c, tau_m, tau_m);
    if (fr_eq(tau_2m, one)) throw std::runtime_error("setup: tau lies on the evaluation domain or its coset (choose another seed)");
    const Fr zt_over_m = fr_mul(c, fr_sub(c, tau_m, one), fr_inv(c, fr_from_u64(c, (uint64_t)m)));
    const Fr hfac = fr_mul(c, fr_mul(c, fr_sub(c, tau_2m, one), fr_inv(c, fr_mul(c, fr_from_u64(c, 2 * (uint64_t)m), delta))), dom.coset_g);
    const Fr minus_one = fr_sub(c, zero, one), minus_g = fr_sub(c, zero, dom.coset_g);
    CtxGuard cg; if (cg_ctx_create(device, &cg.ctx)) die("cg_ctx_create");
    cg_ctx* ctx = cg.ctx;
    auto dev_vec = [&](size_t n) { void* p = nullptr; CG(cg_dev_alloc(ctx, std::max<size_t>(n * 32, 16), &p)); return p; };
    DevBufGuard wp{ctx, dev_vec(m)}, lag{ctx, dev_vec(m)}, hexp{ctx, dev_vec(m)}, tmp{ctx, dev_vec(m)};
    CG(cg_vec_fill_dev(ctx, c.id, wp.p, m, one.v));
    CG(cg_vec_distribute_powers_dev(ctx, c.id, wp.p, m, dom.omega.v, one.v));                   // w^j
    CG(cg_vec_affine_dev(ctx, c.id, lag.p, wp.p, m, minus_one.v, tau.v));                        // tau - w^j
    CG(cg_vec_affine_dev(ctx, c.id, hexp.p, wp.p, m, minus_g.v, tau.v));                         // tau - g w^j
    CG(cg_vec_inverse_dev(ctx, c.id, lag.p, lag.p, m));
    CG(cg_vec_inverse_dev(ctx, c.id, hexp.p, hexp.p, m));
    CG(cg_vec_mul_dev(ctx, c.id, tmp.p, lag.p, wp.p, m));
    CG(cg_vec_affine_dev(ctx, c.id, lag.p, tmp.p, m, zt_over_m.v, nullptr));                     // L_j(tau)
    CG(cg_vec_mul_dev(ctx, c.id, tmp.p, hexp.p, wp.p, m));
    CG(cg_vec_affine_dev(ctx, c.id, hexp.p, tmp.p, m, hfac.v, nullptr));                         // the H exponents
    DevBufGuard sums[3] = {{ctx, dev_vec(n_vars)}, {ctx, dev_vec(n_vars)}, {ctx, dev_vec(n_vars)}};
    for (int k = 0; k < 3; k++) {
        const Csc t = r1cs_transpose(r, k, k == 0 ? n_inp : 0);
        DevBufGuard cp{ctx, dev_copy_of(ctx, t.col_ptr.data(), t.col_ptr.size() * 4)}, rw{ctx, dev_copy_of(ctx, t.row.data(), t.row.size() * 4)},
                    co{ctx, dev_copy_of(ctx, t.coeff.data(), t.coeff.size() * 32)};
        CG(cg_qap_columns_dev(ctx, c.id, (const uint32_t*)cp.p, (const uint32_t*)rw.p, co.p, n_vars, 0, lag.p, sums[k].p));
        CG(cg_ctx_sync(ctx));                                                                     // (the matrix is freed at the end of this scope)
    }
    DevBufGuard lic_t{ctx, dev_vec(n_vars)}, lic{ctx, dev_vec(n_vars)};
    {
        const void* src[3] = {sums[0].p, sums[1].p, sums[2].p};
        const int64_t off[3] = {0, 0, 0}, stride[3] = {1, 1, 1};
        const Fr co[3] = {beta, alpha, one};
        CG(cg_vec_lincomb_dev(ctx, c.id, lic_t.p, 0, 1, n_vars, 3, src, off, stride, co));
        const Fr ginv = fr_inv(c, gamma), dinv = fr_inv(c, delta);
        CG(cg_vec_affine_dev(ctx, c.id, lic.p, lic_t.p, n_inp, ginv.v, nullptr));
        if (n_vars > n_inp) CG(cg_vec_affine_dev(ctx, c.id, (char*)lic.p + n_inp * 32, (const char*)lic_t.p + n_inp * 32, n_vars - n_inp, dinv.v, nullptr));
    }
    auto table = [&](const void* d_scalars, size_t n, int group) {
        cg_bases* b = nullptr; CG(cg_bases_from_scalars(ctx, c.id, group, d_scalars, n, &b));
        Bytes out(n * c.aff(group));
        const int rc = cg_bases_download(ctx, b, 0, n, out.data());
        cg_bases_release(b);
        if (rc) die("cg_bases_download");
        return out;
    };
    auto g1 = [&](const Fr& k) { return pt_to_affine(c, pt_mul(c, pt_generator(c, CG_G1), k)); };
    auto g2 = [&](const Fr& k) { return pt_to_affine(c, pt_mul(c, pt_generator(c, CG_G2), k)); };
    const Bytes coeffs = r1cs_coeff_section(r);
    SectionWriter zk(zkey_path, "zkey", 1, 9);
    zk.begin(1, 4); zk.u32(1);                                                               // protocol: groth16
    zk.begin(2, 4 + c.fq() + 4 + 32 + 12 + 3 * c.aff(CG_G1) + 3 * c.aff(CG_G2));
    zk.u32((uint32_t)c.fq()); zk.put(MOD_Q[c.id], c.fq()); zk.u32(32); zk.put(MOD_R[c.id], 32);
    zk.u32((uint32_t)n_vars); zk.u32((uint32_t)n_pub); zk.u32((uint32_t)m);
    { Bytes a1 = g1(alpha), b1 = g1(beta), b2 = g2(beta), c2 = g2(gamma), d1 = g1(delta), d2 = g2(delta);
      zk.put(a1.data(), a1.size()); zk.put(b1.data(), b1.size()); zk.put(b2.data(), b2.size()); zk.put(c2.data(), c2.size()); zk.put(d1.data(), d1.size()); zk.put(d2.data(), d2.size()); }
    const Bytes l_all = table(lic.p, n_vars, CG_G1);
    zk.begin(3, n_inp * c.aff(CG_G1)); zk.put(l_all.data(), n_inp * c.aff(CG_G1));
    zk.begin(4, coeffs.size()); zk.put(coeffs.data(), coeffs.size());
    { Bytes t = table(sums[0].p, n_vars, CG_G1); zk.begin(5, t.size()); zk.put(t.data(), t.size()); }
    { Bytes t = table(sums[1].p, n_vars, CG_G1); zk.begin(6, t.size()); zk.put(t.data(), t.size()); }
    { Bytes t = table(sums[1].p, n_vars, CG_G2); zk.begin(7, t.size()); zk.put(t.data(), t.size()); }
    zk.begin(8, (n_vars - n_inp) * c.aff(CG_G1)); zk.put(l_all.data() + n_inp * c.aff(CG_G1), (n_vars - n_inp) * c.aff(CG_G1));
    { Bytes t = table(hexp.p, m, CG_G1); zk.begin(9, t.size()); zk.put(t.data(), t.size()); }
    zk.close();
}

}  // namespace cgh
