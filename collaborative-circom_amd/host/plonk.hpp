// co-plonk rounds 1-5 (co-circom/co-plonk/src/round{1..5}.rs) over HipDriver, Plonk zkey reader, Keccak transcript
#pragma once
#include "groth16.hpp"

namespace cgh {

// ==================================================================================================== co-plonk, round 1
// First slice of the Plonk prover on the same kernels: [a]_1, [b]_1, [c]_1 = MSM(p_tau, blind(iNTT(wire values))).
// The reference pins the exact result for the blinding b_i = i (co-plonk/src/round1.rs:346-383).
struct PlonkZKey {   // circom-types/src/plonk/zkey.rs:18-42 (the fields round 1 reads)
    Curve curve;
    size_t n_vars = 0, n_public = 0, domain_size = 0, power = 0, n_additions = 0, n_constraints = 0;
    struct Addition { uint32_t id1, id2; Fr f1, f2; };
    std::vector<Addition> additions;
    std::vector<uint32_t> map[3];
    Bytes p_tau;        // domain_size + 6 packed G1 points
    Fr k1, k2;          // verifying key, zkey.rs:328-356
    Bytes vk_g1;        // qm, ql, qr, qo, qc, s1, s2, s3 (8 packed G1 points)
    Bytes x_2;          // [tau]_2 (packed G2 point): the verifier's (plonk_verify.hpp)
    std::vector<Fr> sigma_eval[3];   // 4 * domain_size evaluations of sigma1..3 (section 12, zkey.rs:116-135,170-180)
    std::vector<Fr> q_eval[5];       // qm, ql, qr, qo, qc on the extended domain (sections 7..11)
    std::vector<std::vector<Fr>> lagrange_eval;   // n_public polynomials on the extended domain (section 13)
    std::vector<Fr> q_coef[5], sigma_coef[3];     // coefficient forms (rounds 4 and 5)
    std::vector<std::vector<Fr>> lagrange_coef;   // the coefficient forms of section 13 (the key audit, plonk_audit.hpp)
    std::map<uint32_t, size_t> section_bytes;     // the length of every section as the file states it (the key audit)
};
static PlonkZKey read_plonk_zkey(int curve_id, const std::string& path) {   // zkey.rs:83-255, header :373-424
    Curve c{curve_id};
    Bytes buf = slurp(path);
    Cursor cur{buf.data(), buf.size()};
    char magic[5] = {0}; cur.bytes(magic, 4);
    if (std::string(magic) != "zkey") throw std::runtime_error("not a zkey file");
    cur.u32();
    uint32_t ns = cur.u32();
    std::map<uint32_t, std::pair<size_t, size_t>> sec;
    for (uint32_t i = 0; i < ns; i++) { uint32_t id = cur.u32(); uint64_t len = cur.u64(); cur.need(len); sec[id] = {cur.off, (size_t)len}; cur.off += len; }
    auto section = [&](uint32_t id) { auto it = sec.find(id); if (it == sec.end()) throw std::runtime_error("missing zkey section"); return Cursor{buf.data() + it->second.first, it->second.second}; };
    if (section(1).u32() != 2) throw std::runtime_error("not a plonk zkey");
    PlonkZKey z; z.curve = c;
    for (const auto& kv : sec) z.section_bytes[kv.first] = kv.second.second;
    Cursor h = section(2);
    if (h.u32() != c.fq()) throw std::runtime_error("unexpected base field byte size");
    uint64_t q[6] = {0}; h.bytes(q, c.fq());
    if (memcmp(q, MOD_Q[curve_id], c.fq())) throw std::runtime_error("invalid base prime in header");
    if (h.u32() != 32) throw std::runtime_error("unexpected scalar field byte size");
    uint64_t r[4]; h.bytes(r, 32);
    if (memcmp(r, MOD_R[curve_id], 32)) throw std::runtime_error("invalid scalar prime in header");
    z.n_vars = h.u32(); z.n_public = h.u32(); z.domain_size = h.u32(); z.n_additions = h.u32(); z.n_constraints = h.u32();
    if (!z.domain_size || (z.domain_size & (z.domain_size - 1))) throw std::runtime_error("Invalid domain size. Must be power of 2");
    while (((size_t)1 << z.power) < z.domain_size) z.power++;
    h.bytes(z.k1.v, 32); h.bytes(z.k2.v, 32);
    z.vk_g1.resize(8 * c.aff(CG_G1)); h.bytes(z.vk_g1.data(), z.vk_g1.size());
    z.x_2.resize(c.aff(CG_G2)); h.bytes(z.x_2.data(), z.x_2.size());
    {
        Cursor sg = section(12);
        for (int k = 0; k < 3; k++) {
            z.sigma_coef[k].resize(z.domain_size); sg.bytes(z.sigma_coef[k].data(), z.domain_size * 32);
            z.sigma_eval[k].resize(4 * z.domain_size);
            sg.bytes(z.sigma_eval[k].data(), 4 * z.domain_size * 32);
        }
    }
    for (int k = 0; k < 5; k++) { Cursor q = section(7 + k); z.q_coef[k].resize(z.domain_size); q.bytes(z.q_coef[k].data(), z.domain_size * 32); z.q_eval[k].resize(4 * z.domain_size); q.bytes(z.q_eval[k].data(), 4 * z.domain_size * 32); }
    { Cursor l = section(13); z.lagrange_eval.resize(z.n_public); z.lagrange_coef.resize(z.n_public); for (size_t j = 0; j < z.n_public; j++) { auto& v = z.lagrange_eval[j]; z.lagrange_coef[j].resize(z.domain_size); l.bytes(z.lagrange_coef[j].data(), z.domain_size * 32); v.resize(4 * z.domain_size); l.bytes(v.data(), 4 * z.domain_size * 32); } }
    { Cursor a = section(3); z.additions.resize(z.n_additions); for (auto& e : z.additions) { e.id1 = a.u32(); e.id2 = a.u32(); a.bytes(e.f1.v, 32); a.bytes(e.f2.v, 32); } }
    for (int k = 0; k < 3; k++) { Cursor m = section(4 + k); z.map[k].resize(z.n_constraints); for (auto& v : z.map[k]) v = m.u32(); }
    { Cursor t = section(14); z.p_tau.resize((z.domain_size + 6) * c.aff(CG_G1)); t.bytes(z.p_tau.data(), z.p_tau.size()); }
    return z;
}

// What a Plonk proof reads from the zkey, resident on the device: p_tau registered (and validated) once, the q and sigma polynomials in
// both forms, the Lagrange evaluations, the one-entry CSR rows that gather the wires in round 1, the omega4^i table of round 3 and the
// additions as a dependency-level schedule.  A session builds it once (co-circom.rs:546-590 reads the zkey once per prover process);
// the file entry points build a transient one per call.  `z` keeps the header: its big vectors are released once they are uploaded.
struct PlonkResident {
    PlonkZKey z;
    cg_ctx* ctx = nullptr;                    // the context the device copies were made with (and are freed with)
    cg_bases* tau = nullptr;
    void* q_eval[5] = {}; void* q_coef[5] = {}; void* sigma_eval[3] = {}; void* sigma_coef[3] = {};
    void* lagrange = nullptr;                 // n_public vectors of 4n evaluations, back to back
    void* lagrange_coef = nullptr;            // their n coefficients each, back to back (read by the key audit only)
    void* pw = nullptr;                       // omega4^i, i < 4n
    uint32_t* row_ptr = nullptr; uint32_t* col[3] = {}; void* ones = nullptr;   // round 1: wire w, row i = signal map[w][i] with coefficient one
    // additions (round1.rs:209-238): addition a writes extended-witness entry n_priv + a; level l = order[level_off[l] .. level_off[l + 1])
    uint32_t* add_order = nullptr; uint32_t* add_ids = nullptr; void* add_coef = nullptr;
    std::vector<size_t> level_off;
    size_t n_priv = 0;

    PlonkResident(cg_ctx* c0, PlonkZKey&& zk, int precompute, bool validate) : z(std::move(zk)), ctx(c0) {
        try { build(precompute, validate); } catch (...) { release(); throw; }
    }
    ~PlonkResident() { release(); }
    PlonkResident(const PlonkResident&) = delete; PlonkResident& operator=(const PlonkResident&) = delete;

private:
    std::vector<void*> owned;
    void* dev(size_t bytes) { void* p = nullptr; CG(cg_dev_alloc(ctx, std::max<size_t>(bytes, 32), &p)); owned.push_back(p); return p; }
    void* put(const void* h, size_t bytes) { void* p = dev(bytes); if (bytes) CG(cg_dev_upload(ctx, p, h, bytes)); return p; }
    template <class V> void* put(const V& v) { return put(v.data(), v.size() * sizeof(v[0])); }
    void release() {
        for (void* p : owned) cg_dev_free(ctx, p);
        owned.clear();
        if (tau) { cg_bases_release(tau); tau = nullptr; }
    }
    void build(int precompute, bool validate) {
        const Curve& c = z.curve; const size_t n = z.domain_size, N = 4 * n, nc = z.n_constraints;
        if (z.n_vars < z.n_additions + z.n_public + 1) throw std::runtime_error("zkey: fewer variables than additions and public inputs");
        if (z.n_public > n) throw std::runtime_error("zkey: more public inputs than rows");   // round 3 reads buffer_a[j] for every public input j
        n_priv = z.n_vars - z.n_additions - z.n_public - 1;
        CG(cg_bases_register(ctx, c.id, CG_G1, z.p_tau.data(), n + 6, c.aff(CG_G1), -1, &tau));
        if (validate) validate_bases(ctx, tau, "p_tau");                              // the zkey parser's per-point checks
        if (precompute) {                                                              // as cgh_session_open_ex: < 0 = chosen by size
            int window = precompute > 0 ? precompute : 0;
            if (precompute < 0) { const size_t m = n + 6; if (m <= ((size_t)1 << 8)) window = 8; else if (m <= ((size_t)1 << 9)) window = 10; else if (m <= ((size_t)1 << 13)) window = 13; }
            CG(cg_bases_precompute(ctx, tau, window));
        }
        Bytes().swap(z.p_tau);
        for (int i = 0; i < 5; i++) { q_eval[i] = put(z.q_eval[i]); q_coef[i] = put(z.q_coef[i]); std::vector<Fr>().swap(z.q_eval[i]); std::vector<Fr>().swap(z.q_coef[i]); }
        for (int i = 0; i < 3; i++) { sigma_eval[i] = put(z.sigma_eval[i]); sigma_coef[i] = put(z.sigma_coef[i]); std::vector<Fr>().swap(z.sigma_eval[i]); std::vector<Fr>().swap(z.sigma_coef[i]); }
        lagrange = dev(z.n_public * N * 32);
        for (size_t j = 0; j < z.n_public; j++) { CG(cg_dev_upload(ctx, (uint8_t*)lagrange + j * N * 32, z.lagrange_eval[j].data(), N * 32)); std::vector<Fr>().swap(z.lagrange_eval[j]); }
        lagrange_coef = dev(z.n_public * n * 32);
        for (size_t j = 0; j < z.n_public; j++) { CG(cg_dev_upload(ctx, (uint8_t*)lagrange_coef + j * n * 32, z.lagrange_coef[j].data(), n * 32)); std::vector<Fr>().swap(z.lagrange_coef[j]); }
        const Fr one = fr_from_u64(c, 1);
        pw = dev(N * 32); CG(cg_vec_fill_dev(ctx, c.id, pw, N, one.v)); CG(cg_vec_distribute_powers_dev(ctx, c.id, pw, N, snarkjs_roots(c).roots[z.power + 2].v, one.v));
        std::vector<uint32_t> rp(nc + 1); for (size_t i = 0; i <= nc; i++) rp[i] = (uint32_t)i;
        row_ptr = (uint32_t*)put(rp);
        for (int w = 0; w < 3; w++) { col[w] = (uint32_t*)put(z.map[w]); std::vector<uint32_t>().swap(z.map[w]); }
        ones = dev(std::max<size_t>(nc, 1) * 32); CG(cg_vec_fill_dev(ctx, c.id, ones, std::max<size_t>(nc, 1), one.v));
        schedule_additions();
        CG(cg_ctx_sync(ctx));                                                          // other contexts (the parties' own) read these
    }
    // level 0 = public inputs and the private witness; an addition lies one level above the deeper of its operands.  An operand that is
    // neither an input nor an EARLIER addition is what calculate_additions refuses (round1.rs:222-226).
    void schedule_additions() {
        const size_t na = z.additions.size(), base = z.n_public + 1;
        std::vector<uint32_t> lvl(na), ids(2 * na); std::vector<Fr> coef(2 * na);
        uint32_t top = 0;
        for (size_t a = 0; a < na; a++) {
            const auto& e = z.additions[a];
            uint32_t l = 0;
            for (uint32_t id : {e.id1, e.id2}) {
                if (id < base) continue;
                if (id >= z.n_vars || id - base >= n_priv + a) throw std::runtime_error("Cannot index into witness " + std::to_string(id));
                if (id - base >= n_priv) l = std::max(l, lvl[id - base - n_priv]);
            }
            lvl[a] = l + 1; top = std::max(top, l + 1);
            ids[2 * a] = e.id1; ids[2 * a + 1] = e.id2; coef[2 * a] = e.f1; coef[2 * a + 1] = e.f2;
        }
        level_off.assign(top + 1, 0);                                                  // counting sort by level
        for (size_t a = 0; a < na; a++) level_off[lvl[a]]++;
        for (uint32_t l = 1; l <= top; l++) level_off[l] += level_off[l - 1];
        std::vector<uint32_t> order(na); std::vector<size_t> fill(level_off.begin(), level_off.end() - 1);
        for (size_t a = 0; a < na; a++) order[fill[lvl[a] - 1]++] = (uint32_t)a;
        add_order = (uint32_t*)put(order); add_ids = (uint32_t*)put(ids); add_coef = put(coef);
        std::vector<PlonkZKey::Addition>().swap(z.additions);
    }
};

// Keccak-256 (pad 0x01) and the reference's transcript conventions (co-plonk/src/types.rs:122-176): big-endian canonical field
// bytes, 2 * byte_len zero bytes for the point at infinity, challenge = digest as a big-endian integer mod r
class Keccak256 {
    uint64_t a[25]; uint8_t blk[136]; size_t used = 0;
    static uint64_t rotl(uint64_t v, unsigned s) { return s ? (v << s) | (v >> (64 - s)) : v; }
    void f1600() {
        uint64_t lfsr = 1;
        for (int round = 0; round < 24; round++) {
            uint64_t col[5];
            for (int x = 0; x < 5; x++) col[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
            for (int x = 0; x < 5; x++) { const uint64_t d = col[(x + 4) % 5] ^ rotl(col[(x + 1) % 5], 1); for (int y = 0; y < 25; y += 5) a[y + x] ^= d; }
            // rho + pi along the standard lane walk
            int x = 1, y = 0; uint64_t cur = a[1];
            for (int t = 0; t < 24; t++) {
                const int nx = y, ny = (2 * x + 3 * y) % 5;
                const uint64_t nxt = a[nx + 5 * ny];
                a[nx + 5 * ny] = rotl(cur, ((t + 1) * (t + 2) / 2) % 64);
                cur = nxt; x = nx; y = ny;
            }
            for (int yy = 0; yy < 25; yy += 5) { uint64_t r[5]; for (int xx = 0; xx < 5; xx++) r[xx] = a[yy + xx]; for (int xx = 0; xx < 5; xx++) a[yy + xx] = r[xx] ^ (~r[(xx + 1) % 5] & r[(xx + 2) % 5]); }
            for (int j = 0; j < 7; j++) {                                               // iota via the degree-8 LFSR
                const bool bit = lfsr & 1; lfsr = (lfsr << 1) ^ ((lfsr >> 7) * 0x71); lfsr &= 0xff;
                if (bit) a[0] ^= (uint64_t)1 << ((1 << j) - 1);
            }
        }
    }
    void absorb() { for (int i = 0; i < 17; i++) { uint64_t w; memcpy(&w, blk + 8 * i, 8); a[i] ^= w; } f1600(); used = 0; }
public:
    Keccak256() { memset(a, 0, sizeof a); }
    void update(const uint8_t* p, size_t n) { while (n--) { blk[used++] = *p++; if (used == sizeof blk) absorb(); } }
    void finish(uint8_t out[32]) { memset(blk + used, 0, sizeof blk - used); blk[used] ^= 0x01; blk[sizeof blk - 1] ^= 0x80; absorb(); memcpy(out, a, 32); }
};
class PlonkTranscript {
    const Curve& c; Keccak256 h;
    void be_bytes(const uint64_t* canonical, size_t nbytes) { std::vector<uint8_t> be(nbytes); for (size_t i = 0; i < nbytes; i++) be[nbytes - 1 - i] = (uint8_t)(canonical[i / 8] >> (8 * (i % 8))); h.update(be.data(), nbytes); }
public:
    explicit PlonkTranscript(const Curve& cv) : c(cv) {}
    void add_scalar(const Fr& s) { uint64_t can[4]; CG(cg_fr_to_canonical(c.id, s.v, can, 1)); be_bytes(can, 32); }
    void add_point(const uint8_t* aff) {                                                // packed affine G1, (0,0) = infinity
        if (all_zero_bytes(aff, c.aff(CG_G1))) { std::vector<uint8_t> z(2 * c.fq(), 0); h.update(z.data(), z.size()); return; }
        uint64_t can[12]; CG(cg_fq_to_canonical(c.id, aff, can, 2));
        be_bytes(can, c.fq()); be_bytes(can + c.fq() / 8, c.fq());
    }
    Fr get_challenge() {
        uint8_t d[32]; h.finish(d);
        Fr acc = fr_from_u64(c, 0); const Fr b = fr_from_u64(c, 256);                  // from_be_bytes_mod_order
        for (int i = 0; i < 32; i++) acc = fr_add(c, fr_mul(c, acc, b), fr_from_u64(c, d[i]));
        return acc;
    }
};

// ==================================================================================================== co-plonk, all rounds, any driver
// The five rounds (co-plonk/src/round1..5.rs) written once over share-vector operations: per-component kernels for everything
// linear, the driver's protocols for products of two shared vectors (`mul_vec`), for `array_prod_mul` / `inv_many` (round2.rs:18-41,
// rep3.rs:544-558, shamir.rs:521-535) and for openings.  Plain, REP3 and Shamir run the same code; values that every party reconstructs (commitments,
// evaluations) are functions of the witness and of the opened blinding values only.
class CoPlonk {
public:
    HipDriver& d; const PlonkResident& r; const PlonkZKey& z; const cg_bases* tau;
    const Curve c; cg_ctx* ctx; const size_t n, N; const int k;
    Fr zero, one, omega, omega4, w2r;
    FieldShare b[11];
    std::vector<Fr> pub;                       // n_public + 1 values, entry 0 forced to 0 (types.rs:107-109)
    ShareVec buf[3], poly[3], evl[3], poly_z, eval_z, tpart[3];
    Point commit[3], commit_z, commit_t[3], commit_wxi, commit_wxiw;
    Fr beta, gamma, alpha, xi, v[5], ev_a, ev_b, ev_c, ev_s1, ev_s2, ev_zw;
    std::vector<ShareVec> tmp_vecs; std::vector<void*> tmp_ptrs;

    CoPlonk(HipDriver& drv, const PlonkResident& res, const std::vector<Fr>& public_inputs, const FieldShare* blind)
        : d(drv), r(res), z(res.z), tau(res.tau), c(drv.curve), ctx(drv.ctx), n(res.z.domain_size), N(4 * res.z.domain_size), k(drv.k()), pub(public_inputs) {
        if (pub.size() != z.n_public + 1) throw std::runtime_error("public input length does not match the zkey");
        zero = fr_from_u64(c, 0); one = fr_from_u64(c, 1);
        pub[0] = zero;
        const SnarkjsRoots rt = snarkjs_roots(c);
        omega = rt.roots[z.power]; omega4 = rt.roots[z.power + 2]; w2r = rt.roots[2];
        for (int i = 0; i < 11; i++) b[i] = blind[i];
    }
    ~CoPlonk() {
        release_tmp();
        for (ShareVec* sv : {&buf[0], &buf[1], &buf[2], &poly[0], &poly[1], &poly[2], &evl[0], &evl[1], &evl[2], &poly_z, &eval_z, &tpart[0], &tpart[1], &tpart[2]}) d.free_vec(*sv);
    }
    // ---- share-vector helpers ------------------------------------------------------------------------------------------------
    Fr neg(const Fr& v) const { return fr_sub(c, zero, v); }
    Fr M(const Fr& a, const Fr& x) const { return fr_mul(c, a, x); }
    Fr A(const Fr& a, const Fr& x) const { return fr_add(c, a, x); }
    static uint8_t* at(const ShareVec& s, int j, size_t off = 0) { return (uint8_t*)s.c[j] + off * 32; }
    ShareVec T(size_t len) { ShareVec v = d.alloc_vec(len); tmp_vecs.push_back(v); return v; }          // zeroed temporary, freed by release_tmp
    ShareVec keep(ShareVec v) { tmp_vecs.push_back(v); return v; }
    void* Tp(size_t len) { void* p = d.dalloc(len * 32); tmp_ptrs.push_back(p); return p; }
    void* upload(const std::vector<Fr>& h) { void* p = Tp(h.size()); CG(cg_dev_upload(ctx, p, h.data(), h.size() * 32)); return p; }
    void release_tmp() { for (auto& v : tmp_vecs) d.free_vec(v); tmp_vecs.clear(); for (void* p : tmp_ptrs) CG(cg_dev_free(ctx, p)); tmp_ptrs.clear(); }
    static ShareVec view(const ShareVec& s, size_t off, size_t len) { ShareVec v; v.n = len; for (int j = 0; j < 2; j++) v.c[j] = s.c[j] ? (uint8_t*)s.c[j] + off * 32 : nullptr; return v; }
    void copy(const ShareVec& o, const ShareVec& a, size_t len) { for (int j = 0; j < k; j++) CG(cg_vec_gather_strided_dev(ctx, c.id, o.c[j], a.c[j], len, 0, 1)); }
    void add(const ShareVec& o, const ShareVec& a, const ShareVec& x, size_t len) { for (int j = 0; j < k; j++) CG(cg_vec_add_dev(ctx, c.id, o.c[j], a.c[j], x.c[j], len)); }
    void sub(const ShareVec& o, const ShareVec& a, const ShareVec& x, size_t len) { for (int j = 0; j < k; j++) CG(cg_vec_sub_dev(ctx, c.id, o.c[j], a.c[j], x.c[j], len)); }
    void scale(const ShareVec& o, const ShareVec& a, const Fr& f, size_t len) { for (int j = 0; j < k; j++) CG(cg_vec_affine_dev(ctx, c.id, o.c[j], a.c[j], len, f.v, nullptr)); }   // mul_with_public
    void mulpub(const ShareVec& o, const ShareVec& a, const void* pv, size_t len) { for (int j = 0; j < k; j++) CG(cg_vec_mul_dev(ctx, c.id, o.c[j], a.c[j], pv, len)); }              // by a public vector
    void axpy(const ShareVec& o, const ShareVec& a, const Fr& f, size_t len) { ShareVec t = T(len); scale(t, a, f, len); add(o, o, t, len); }                                           // o += f * a
    void addpub_vec(const ShareVec& o, const ShareVec& a, const void* pv, size_t len) {                                               // add_with_public, element-wise
        const int pc = d.public_component();
        for (int j = 0; j < k; j++) { if (j == pc) CG(cg_vec_add_dev(ctx, c.id, o.c[j], a.c[j], pv, len)); else if (o.c[j] != a.c[j]) CG(cg_vec_gather_strided_dev(ctx, c.id, o.c[j], a.c[j], len, 0, 1)); }
    }
    void addpub_scalar(const ShareVec& o, const ShareVec& a, const Fr& f, size_t len) {
        const int pc = d.public_component();
        for (int j = 0; j < k; j++) { if (j == pc) CG(cg_vec_affine_dev(ctx, c.id, o.c[j], a.c[j], len, one.v, f.v)); else if (o.c[j] != a.c[j]) CG(cg_vec_gather_strided_dev(ctx, c.id, o.c[j], a.c[j], len, 0, 1)); }
    }
    void axpy_pub(const ShareVec& o, const void* pv, const Fr& f, size_t len) {                                                       // o += f * (public vector)
        const int pc = d.public_component(); if (pc < 0) return;
        void* t = Tp(len); CG(cg_vec_affine_dev(ctx, c.id, t, pv, len, f.v, nullptr)); CG(cg_vec_add_dev(ctx, c.id, o.c[pc], o.c[pc], t, len));
    }
    void affine_share(const ShareVec& o, const void* pv, const FieldShare& kk, const FieldShare& dd, size_t len) {                    // o = kk * (public vector) + dd, share-valued kk, dd
        for (int j = 0; j < k; j++) CG(cg_vec_affine_dev(ctx, c.id, o.c[j], pv, len, kk.c[j].v, dd.c[j].v));
    }
    FieldShare get(const ShareVec& s, size_t i) { FieldShare f; f.c[0] = f.c[1] = zero; for (int j = 0; j < k; j++) CG(cg_dev_download(ctx, f.c[j].v, at(s, j, i), 32)); return f; }
    void set(const ShareVec& s, size_t i, const FieldShare& f) { for (int j = 0; j < k; j++) CG(cg_dev_upload(ctx, at(s, j, i), f.c[j].v, 32)); }
    FieldShare fs_sub(const FieldShare& a, const FieldShare& x) const { FieldShare r; for (int j = 0; j < 2; j++) r.c[j] = fr_sub(c, a.c[j], x.c[j]); return r; }
    FieldShare fs_addpub(FieldShare a, const Fr& f) const { const int pc = d.public_component(); if (pc >= 0) a.c[pc] = fr_add(c, a.c[pc], f); return a; }
    ShareVec mul(const ShareVec& a, const ShareVec& x, size_t len) { ShareVec av = view(a, 0, len), xv = view(x, 0, len); return keep(d.mul_vec(av, xv)); }                // mul_vec / mul_many
    Point commit_open(const ShareVec& p, size_t len) {
        if (len > z.domain_size + 6) throw std::runtime_error("polynomial degree too large");
        const PointShare cm = d.msm_public_points(tau, CG_G1, 0, len, p);
        d.verify_received_vectors();       // what a peer sent for this round's products is refused BEFORE anything derived from it is opened (the reference refuses at deserialisation)
        return d.open_point(cm);
    }
    void ntt(const ShareVec& s, size_t len, const Fr& g, bool inverse) { void* ptrs[2] = {s.c[0], s.c[1]}; CG(cg_ntt_dev(ctx, c.id, ptrs, k, len, g.v, inverse ? 1 : 0, nullptr)); }
    // inv_many (rep3.rs:544-558 / plain): element-wise inverse of a shared vector
    ShareVec inv_many(const ShareVec& a, size_t len) {
        ShareVec out = T(len);
        if (d.mode == Mode::Plain) { CG(cg_vec_inverse_dev(ctx, c.id, out.c[0], a.c[0], len)); return out; }
        ShareVec r = keep(d.rand_vec(len));
        void* y = d.mul_open_vec(view(a, 0, len), r); tmp_ptrs.push_back(y);
        CG(cg_vec_inverse_dev(ctx, c.id, y, y, len));                                 // (a zero would make the reference fail with "cannot compute inverse of zero")
        mulpub(out, r, y, len);
        return out;
    }
    // array_prod_mul (round2.rs:18-41): shared prefix products in a constant number of rounds
    ShareVec array_prod_mul(const ShareVec& inp, size_t len) {
        if (d.mode == Mode::Plain) { ShareVec out = T(len); CG(cg_vec_prefix_prod_dev(ctx, c.id, out.c[0], inp.c[0], len)); return out; }
        ShareVec r = keep(d.rand_vec(len + 1));
        ShareVec r_inv = inv_many(r, len + 1);
        ShareVec r_inv0 = T(len);
        const FieldShare first = get(r_inv, 0);
        for (int j = 0; j < k; j++) CG(cg_vec_fill_dev(ctx, c.id, r_inv0.c[j], len, first.c[j].v));
        ShareVec unblind = mul(r_inv0, view(r, 1, len), len);
        ShareVec m = mul(view(r, 0, len), inp, len);
        void* open = d.mul_open_vec(m, view(r_inv, 1, len)); tmp_ptrs.push_back(open);
        CG(cg_vec_prefix_prod_dev(ctx, c.id, open, open, len));
        mulpub(unblind, unblind, open, len);
        return unblind;
    }
    Fr eval_pub_poly(const void* d_poly, size_t len, const Fr& x) {                    // Horner of a public polynomial as a scan
        void* t = Tp(len);
        CG(cg_vec_gather_strided_dev(ctx, c.id, t, d_poly, len, 0, 1));
        CG(cg_vec_distribute_powers_dev(ctx, c.id, t, len, x.v, one.v));
        CG(cg_vec_prefix_sum_dev(ctx, c.id, t, t, len));
        Fr r; CG(cg_dev_download(ctx, r.v, (const uint8_t*)t + (len - 1) * 32, 32));
        return r;
    }
    FieldShare eval_share_poly(const ShareVec& p, size_t len, const Fr& x) {           // evaluate_poly_public (rep3.rs:923-931)
        FieldShare f; f.c[0] = f.c[1] = zero;
        for (int j = 0; j < k; j++) f.c[j] = eval_pub_poly(p.c[j], len, x);
        return f;
    }
    void div_by_zerofier1(const ShareVec& p, size_t len, const Fr& point) {             // round5.rs:97-115 with n = 1; the caller drops the last entry
        const Fr pinv = fr_inv(c, point);
        for (int j = 0; j < k; j++) {
            CG(cg_vec_affine_dev(ctx, c.id, p.c[j], p.c[j], len, neg(pinv).v, nullptr));
            CG(cg_vec_distribute_powers_dev(ctx, c.id, p.c[j], len, point.v, one.v));
            CG(cg_vec_prefix_sum_dev(ctx, c.id, p.c[j], p.c[j], len));
            CG(cg_vec_distribute_powers_dev(ctx, c.id, p.c[j], len, pinv.v, one.v));
        }
    }
    void transcript_point(PlonkTranscript& t, const Point& p) { Bytes a = pt_to_affine(c, p); t.add_point(a.data()); }

    // ---- round 1 (round1.rs:118-312) ---------------------------------------------------------------------------------------------
    FieldShare trivial(const Fr& v) const { FieldShare f; f.c[0] = f.c[1] = zero; const int pc = d.public_component(); if (pc >= 0) f.c[pc] = v; return f; }
    // calculate_additions (:208-238) on the device: the private witness, then one launch per dependency level of the additions (every
    // share component in it; public operands in the public component only, as trivial() makes them)
    ShareVec extend_witness(const ShareVec& wit, const void* d_pub) {
        ShareVec ext = d.alloc_vec(r.n_priv + z.n_additions);
        if (r.n_priv) copy(ext, wit, r.n_priv);
        for (size_t l = 0; l + 1 < r.level_off.size(); l++)
            CG(cg_plonk_additions_dev(ctx, c.id, r.add_order + r.level_off[l], r.level_off[l + 1] - r.level_off[l], r.add_ids, r.add_coef, d_pub, (uint32_t)(z.n_public + 1),
                                      d.public_component(), ext.c[0], k == 2 ? ext.c[1] : nullptr, r.n_priv));
        return ext;
    }
    void round1(const ShareVec& private_witness) {
        const size_t nc = z.n_constraints;
        if (private_witness.n != r.n_priv) throw std::runtime_error("witness length does not match the zkey");
        void* d_pub = upload(pub);
        ShareVec ext = z.n_additions ? keep(extend_witness(private_witness, d_pub)) : private_witness;
        for (int w = 0; w < 3; w++) {
            poly[w] = d.alloc_vec(n + 2);
            // the wire buffers are gathers: one-entry CSR rows with coefficient one reuse the constraint-evaluation kernel (get_witness' public /
            // private split with the REP3 party asymmetry, lib.rs:113-137)
            CG(cg_spmv_csr_dev(ctx, c.id, r.row_ptr, r.col[w], r.ones, nc, d_pub, (uint32_t)(z.n_public + 1), d.party(), ext.c[0], ext.c[1], poly[w].c[0], poly[w].c[1]));
            buf[w] = d.alloc_vec(n); copy(buf[w], poly[w], n);
            ntt(poly[w], n, omega, true);                                                // :170-172
            evl[w] = d.alloc_vec(N); copy(evl[w], poly[w], n); ntt(evl[w], N, omega4, false);   // :174-177
            const FieldShare &b_hi = b[2 * w], &b_lo = b[2 * w + 1];                     // blind_coefficients (lib.rs:140-158)
            set(poly[w], 0, fs_sub(get(poly[w], 0), b_lo)); set(poly[w], 1, fs_sub(get(poly[w], 1), b_hi));
            set(poly[w], n, b_lo); set(poly[w], n + 1, b_hi);
        }
        PointShare cm[3];
        for (int w = 0; w < 3; w++) cm[w] = d.msm_public_points(tau, CG_G1, 0, n + 2, poly[w]);   // :276-290
        d.verify_received_vectors();
        for (int w = 0; w < 3; w++) commit[w] = d.open_point(cm[w]);                               // open_point_many (:292)
        release_tmp();
    }
    // ---- round 2 (round2.rs:146-298) ---------------------------------------------------------------------------------------------
    void round2() {
        {
            PlonkTranscript t(c);
            for (int i = 0; i < 8; i++) t.add_point(z.vk_g1.data() + i * c.aff(CG_G1));
            for (size_t i = 1; i < pub.size(); i++) t.add_scalar(pub[i]);
            for (int w = 0; w < 3; w++) transcript_point(t, commit[w]);
            beta = t.get_challenge();
            PlonkTranscript t2(c); t2.add_scalar(beta); gamma = t2.get_challenge();
        }
        // the six factors num_w = buf_w + beta k_w omega^i + gamma, den_w = buf_w + beta sigma_w(omega^i) + gamma (:162-216) in one launch over
        // every share component: omega^i = pw[4 i], sigma_w(omega^i) = sigma_eval[w][4 i], read where they lie.  The products keep their
        // operands and their order (num b, den b, num c, den c), so a party's masks, pairs and messages do not move.
        ShareVec f[3], g[3];
        for (int w = 0; w < 3; w++) { f[w] = U(n); g[w] = U(n); }
        { const Fr co[4] = {beta, M(beta, z.k1), M(beta, z.k2), gamma};
          const void* sg[3] = {r.sigma_eval[0], r.sigma_eval[1], r.sigma_eval[2]};
          const auto wires = table({&buf[0], &buf[1], &buf[2]}); const auto o = table({&f[0], &f[1], &f[2], &g[0], &g[1], &g[2]});
          CG(cg_plonk_r2_factors_dev(ctx, c.id, k, d.public_component(), n, r.pw, 4, sg, 4, co, wires.data(), o.data())); }
        ShareVec num = f[0], den = g[0];
        for (int w = 1; w < 3; w++) { num = mul(num, f[w], n); den = mul(den, g[w], n); }
        ShareVec num_p = array_prod_mul(num, n), den_p = array_prod_mul(den, n);           // :218-224
        ShareVec den_i = inv_many(den_p, n);                                               // :228
        ShareVec zb = mul(num_p, den_i, n);                                                // :229
        poly_z = d.alloc_vec(n + 3);
        if (n > 1) copy(view(poly_z, 1, n - 1), zb, n - 1);                                // rotate_right(1) (:230)
        copy(poly_z, view(zb, n - 1, 1), 1);
        ntt(poly_z, n, omega, true);                                                       // :235
        eval_z = d.alloc_vec(N); copy(eval_z, poly_z, n); ntt(eval_z, N, omega4, false);   // :238
        set(poly_z, 0, fs_sub(get(poly_z, 0), b[8])); set(poly_z, 1, fs_sub(get(poly_z, 1), b[7])); set(poly_z, 2, fs_sub(get(poly_z, 2), b[6]));
        set(poly_z, n, b[8]); set(poly_z, n + 1, b[7]); set(poly_z, n + 2, b[6]);
        commit_z = commit_open(poly_z, n + 3);                                             // :268-275
        release_tmp();
    }
    // ---- round 3 (round3.rs:234-527) ---------------------------------------------------------------------------------------------
    // The pointwise work is six fused kernels (plonk_kernels.hpp) over every share component; the products (mul_vec) are the ones of
    // mul4vec (:17-57) and of the gate constraint, made with the same operands in the same order as before, so that a REP3 party's masks,
    // messages and randomness positions do not move.
    ShareVec U(size_t len) { ShareVec v; v.n = len; for (int j = 0; j < k; j++) v.c[j] = d.dalloc(len * 32); tmp_vecs.push_back(v); return v; }   // uninitialised temporary
    static std::vector<void*> table(std::initializer_list<const ShareVec*> vs) { std::vector<void*> t; for (const ShareVec* v : vs) { t.push_back(v->c[0]); t.push_back(v->c[1]); } return t; }
    void round3() {
        if (z.n_public == 0) throw std::runtime_error("round 3 needs at least one public input (lagrange[0])");
        { PlonkTranscript t(c); t.add_scalar(beta); t.add_scalar(gamma); transcript_point(t, commit_z); alpha = t.get_challenge(); }   // :498-503
        const Fr two = fr_from_u64(c, 2);
        const Fr m2w = M(neg(two), w2r), tw = M(two, w2r);
        const Fr Z[12] = {zero, A(neg(one), w2r), neg(two), fr_sub(c, neg(one), w2r),      // get_z1..3 (:203-232)
                          zero, m2w, M(two, two), neg(m2w),
                          zero, A(two, tw), neg(M(M(two, two), two)), fr_sub(c, two, tw)};
        const ShareVec &a = evl[0], &bb = evl[1], &cc = evl[2], &ez = eval_z;
        const int pc = d.public_component();
        // the blinding polynomials on the 4n-th roots of unity (:246-256, :307-322)
        ShareVec ap = U(N), bp = U(N), cp = U(N), zp = U(N), zwp = U(N);
        { Fr bl[18]; for (int j = 0; j < k; j++) for (int t = 0; t < 9; t++) bl[9 * j + t] = b[t].c[j];
          const auto o = table({&ap, &bp, &cp, &zp, &zwp}); CG(cg_plonk_r3_blind_dev(ctx, c.id, k, N, r.pw, omega.v, bl, o.data())); }
        ShareVec zw = U(N);                                                                // z(X omega): eval_z rotated by 4 (:324-327)
        copy(zw, view(ez, 4, N - 4), N - 4); copy(view(zw, N - 4, 4), ez, 4);
        // gate constraint (:333-368), the public-input polynomial included (:352-358): pi -= L_j * buffer_a[j]
        ShareVec a_b = mul(a, bb, N), a_bp = mul(a, bp, N), ap_b = mul(bb, ap, N), ap_bp = mul(ap, bp, N);
        ShareVec e1 = U(N), e1z = U(N);
        { const void* q[5] = {r.q_eval[0], r.q_eval[1], r.q_eval[2], r.q_eval[3], r.q_eval[4]};
          const auto in = table({&buf[0], &a_b, &a_bp, &ap_b, &ap_bp, &a, &bb, &cc, &ap, &bp, &cp}); const auto o = table({&e1, &e1z});
          CG(cg_plonk_r3_gate_dev(ctx, c.id, k, pc, N, q, r.lagrange, z.n_public, in.data(), Z, o.data())); }
        // permutation constraints (:370-418)
        auto mul4 = [&](const ShareVec& Av, const ShareVec& Bv, const ShareVec& Cv, const ShareVec& Dv, const ShareVec& Dp, ShareVec& rr, ShareVec& rz) {   // mul4vec + mul4vec_post (:17-72)
            ShareVec AB = mul(Av, Bv, N);
            ShareVec S1 = mul(Av, bp, N); add(S1, S1, mul(ap, Bv, N), N);                  // A B' + A' B
            ShareVec CD = mul(Cv, Dv, N);
            ShareVec S2 = mul(Cv, Dp, N); add(S2, S2, mul(cp, Dv, N), N);                  // C D' + C' D
            ShareVec CpDp = mul(cp, Dp, N);
            rr = mul(AB, CD, N);
            const ShareVec p0 = mul(S1, CD, N), p1 = mul(AB, S2, N);
            const ShareVec p2 = mul(ap_bp, CD, N), p3 = mul(S1, S2, N), p4 = mul(AB, CpDp, N);
            const ShareVec p5 = mul(S1, CpDp, N), p6 = mul(ap_bp, S2, N);
            const ShareVec p7 = mul(ap_bp, CpDp, N);
            rz = U(N);
            const auto pr = table({&p0, &p1, &p2, &p3, &p4, &p5, &p6, &p7}); const auto o = table({&rz});
            CG(cg_plonk_mul4_tail_dev(ctx, c.id, k, N, pr.data(), Z, o.data()));
        };
        ShareVec e2, e2z, e3, e3z;
        {
            ShareVec fa = U(N), fb = U(N), fc = U(N), ga = U(N), gb = U(N), gc = U(N);
            const Fr co[4] = {beta, M(beta, z.k1), M(beta, z.k2), gamma};
            const void* sg[3] = {r.sigma_eval[0], r.sigma_eval[1], r.sigma_eval[2]};
            const auto w = table({&a, &bb, &cc}); const auto o = table({&fa, &fb, &fc, &ga, &gb, &gc});
            CG(cg_plonk_r3_perm_dev(ctx, c.id, k, pc, N, r.pw, sg, co, w.data(), o.data()));
            mul4(fa, fb, fc, ez, zp, e2, e2z);
            mul4(ga, gb, gc, zw, zwp, e3, e3z);
        }
        // t = e1 + alpha (e2 - e3) + alpha^2 L1 (z - 1), tz likewise from the blinding parts (:420-441)
        ShareVec Tv = U(N), TZ = U(N);
        { const auto in = table({&e1, &e1z, &e2, &e3, &e2z, &e3z, &ez, &zp}); const auto o = table({&Tv, &TZ});
          CG(cg_plonk_r3_t_dev(ctx, c.id, k, pc, N, r.lagrange, in.data(), alpha.v, o.data())); }
        ntt(Tv, N, omega4, true);                                                          // :442
        ntt(TZ, N, omega4, true);
        { void* t[2] = {Tv.c[0], Tv.c[1]}; const void* tz[2] = {TZ.c[0], TZ.c[1]};          // neg_vec_in_place_limit, division by X^n - 1, + tz (:443-453)
          CG(cg_plonk_r3_divide_dev(ctx, c.id, k, n, t, tz)); }
        const size_t len[3] = {n + 1, n + 1, n + 6};                                        // split (:455-470)
        for (int p = 0; p < 3; p++) { tpart[p] = d.alloc_vec(len[p]); copy(tpart[p], view(Tv, (size_t)p * n, p == 2 ? n + 6 : n), p == 2 ? n + 6 : n); }
        set(tpart[0], n, b[9]);
        set(tpart[1], 0, fs_sub(get(tpart[1], 0), b[9])); set(tpart[1], n, b[10]);
        set(tpart[2], 0, fs_sub(get(tpart[2], 0), b[10]));
        PointShare cm[3];
        for (int p = 0; p < 3; p++) { if (len[p] > z.domain_size + 6) throw std::runtime_error("polynomial degree too large"); cm[p] = d.msm_public_points(tau, CG_G1, 0, len[p], tpart[p]); }
        d.verify_received_vectors();
        for (int p = 0; p < 3; p++) commit_t[p] = d.open_point(cm[p]);                     // :507-522
        release_tmp();
    }
    // ---- rounds 4 and 5 (round4.rs:115-160, round5.rs:143-365) --------------------------------------------------------------------
    void round4() {
        { PlonkTranscript t(c); t.add_scalar(alpha); for (int p = 0; p < 3; p++) transcript_point(t, commit_t[p]); xi = t.get_challenge(); }
        const Fr xiw = M(xi, omega);
        std::vector<FieldShare> sh = {eval_share_poly(poly[0], n + 2, xi), eval_share_poly(poly[1], n + 2, xi), eval_share_poly(poly[2], n + 2, xi), eval_share_poly(poly_z, n + 3, xiw)};
        d.verify_received_vectors();
        const std::vector<Fr> opened = d.open_many(sh);                                    // :131
        ev_a = opened[0]; ev_b = opened[1]; ev_c = opened[2]; ev_zw = opened[3];
        ev_s1 = eval_pub_poly(r.sigma_coef[0], n, xi); ev_s2 = eval_pub_poly(r.sigma_coef[1], n, xi);
        release_tmp();
    }
    void round5() {
        { PlonkTranscript t(c); const Fr* items[7] = {&xi, &ev_a, &ev_b, &ev_c, &ev_s1, &ev_s2, &ev_zw}; for (const Fr* e : items) t.add_scalar(*e);
          v[0] = t.get_challenge(); for (int i = 1; i < 5; i++) v[i] = M(v[i - 1], v[0]); }                                          // :338-350
        const size_t len = n + 6;
        Fr xin = xi; for (size_t i = 0; i < z.power; i++) xin = M(xin, xin);               // lib.rs:160-184
        const Fr zh = fr_sub(c, xin, one);
        std::vector<Fr> l; { Fr wv = one; const Fr nn = fr_from_u64(c, (uint64_t)n); for (size_t i = 0; i < std::max<size_t>(1, z.n_public); i++) { l.push_back(M(M(wv, zh), fr_inv(c, M(nn, fr_sub(c, xi, wv))))); wv = M(wv, omega); } }
        Fr eval_pi = zero; for (size_t i = 1; i < pub.size() && i - 1 < l.size(); i++) eval_pi = fr_sub(c, eval_pi, M(l[i - 1], pub[i]));
        const Fr betaxi = M(beta, xi);
        const Fr e2 = M(M(M(A(A(ev_a, betaxi), gamma), A(A(ev_b, M(betaxi, z.k1)), gamma)), A(A(ev_c, M(betaxi, z.k2)), gamma)), alpha);
        const Fr e3 = M(M(M(A(A(ev_a, M(beta, ev_s1)), gamma), A(A(ev_b, M(beta, ev_s2)), gamma)), ev_zw), alpha);
        const Fr e4 = M(M(alpha, alpha), l[0]), e24 = A(e2, e4);
        ShareVec R = T(len);                                                               // compute_r (:143-260)
        axpy(R, poly_z, e24, n + 3);
        void* const* s_co = r.sigma_coef;
        { const Fr f[5] = {M(ev_a, ev_b), ev_a, ev_b, ev_c, one}; for (int i = 0; i < 5; i++) axpy_pub(R, r.q_coef[i], f[i], n); }
        axpy_pub(R, s_co[2], neg(M(e3, beta)), n);
        axpy(R, tpart[2], neg(M(zh, M(xin, xin))), n + 6); axpy(R, tpart[1], neg(M(zh, xin)), n + 1); axpy(R, tpart[0], neg(zh), n + 1);
        const Fr r0 = fr_sub(c, fr_sub(c, eval_pi, M(e3, A(ev_c, gamma))), e4);
        // compute_wxi (:263-311)
        for (int w = 0; w < 3; w++) axpy(R, poly[w], v[w], n + 2);
        axpy_pub(R, s_co[0], v[3], n); axpy_pub(R, s_co[1], v[4], n);
        const Fr corr = fr_sub(c, r0, A(A(A(A(M(v[0], ev_a), M(v[1], ev_b)), M(v[2], ev_c)), M(v[3], ev_s1)), M(v[4], ev_s2)));
        set(R, 0, fs_addpub(get(R, 0), corr));
        div_by_zerofier1(R, len, xi);
        // compute_wxiw (:314-327)
        ShareVec W = T(n + 3); copy(W, poly_z, n + 3);
        set(W, 0, fs_addpub(get(W, 0), neg(ev_zw)));
        div_by_zerofier1(W, n + 3, M(xi, omega));
        PointShare c1 = d.msm_public_points(tau, CG_G1, 0, len - 1, R), c2 = d.msm_public_points(tau, CG_G1, 0, n + 2, W);   // :351-358
        d.verify_received_vectors();
        commit_wxi = d.open_point(c1); commit_wxiw = d.open_point(c2);
        release_tmp();
    }
};


}  // namespace cgh
