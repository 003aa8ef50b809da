// C entry points: co-plonk (co-plonk/src/plonk.rs:133-271 drives round1..round5)
#include "plonk.hpp"
#include "plonk_verify.hpp"
#include "plonk_audit.hpp"
#include "capi_common.hpp"

#include <chrono>
#include <memory>
#include <mutex>

extern "C" {

// info: n_vars, n_public, domain_size, power, n_additions, n_constraints
int32_t cgh_plonk_zkey_info(int32_t curve, const char* path, size_t* info) {
    try {
        cgh::PlonkZKey z = cgh::read_plonk_zkey(curve, path);
        info[0] = z.n_vars; info[1] = z.n_public; info[2] = z.domain_size; info[3] = z.power; info[4] = z.n_additions; info[5] = z.n_constraints;
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
// ---- co-plonk entry points -------------------------------------------------------------------------------------------------------
namespace {
struct PlonkOut { uint64_t* commits; uint64_t* challenges; uint64_t* evals; uint64_t* t_polys; uint64_t* poly_z; };
// runs rounds 1..upto on `driver` and stores what has been computed (slot layout of cgh_plonk_prove_plain)
// round_seconds (optional): wall time of rounds 1..5, the stream drained once after each round
void plonk_run(cgh::HipDriver& driver, const cgh::PlonkResident& res, const std::vector<cgh::Fr>& pub, const cgh::ShareVec& wit, const cgh::FieldShare* b, int upto, const PlonkOut& o,
               double* round_seconds = nullptr) {
    using namespace cgh;
    auto last = std::chrono::steady_clock::now();
    auto lap = [&](int round) {
        if (!round_seconds) return;
        CG(cg_ctx_sync(driver.ctx));
        const auto now = std::chrono::steady_clock::now(); round_seconds[round - 1] = std::chrono::duration<double>(now - last).count(); last = now;
    };
    const Curve& c = res.z.curve; const size_t psz = c.aff(CG_G1);
    auto put = [&](int slot, const Point& p) { if (!o.commits) return; Bytes a = pt_to_affine(c, p); memcpy((uint8_t*)o.commits + slot * psz, a.data(), psz); };
    auto putf = [&](uint64_t* dst, int slot, const Fr& f) { if (dst) memcpy(dst + 4 * slot, f.v, 32); };
    CoPlonk pk(driver, res, pub, b);
    pk.round1(wit);
    for (int k = 0; k < 3; k++) put(k, pk.commit[k]);
    lap(1);
    if (upto >= 2) {
        pk.round2(); put(3, pk.commit_z); putf(o.challenges, 0, pk.beta); putf(o.challenges, 1, pk.gamma);
        if (o.poly_z) CG(cg_dev_download(driver.ctx, o.poly_z, pk.poly_z.c[0], pk.poly_z.n * 32));
        lap(2);
    }
    if (upto >= 3) {
        pk.round3(); for (int k = 0; k < 3; k++) put(4 + k, pk.commit_t[k]); putf(o.challenges, 2, pk.alpha);
        if (o.t_polys) { size_t off = 0; for (int k = 0; k < 3; k++) { CG(cg_dev_download(driver.ctx, o.t_polys + off * 4, pk.tpart[k].c[0], pk.tpart[k].n * 32)); off += pk.tpart[k].n; } }
        lap(3);
    }
    if (upto >= 4) {
        pk.round4(); putf(o.challenges, 3, pk.xi);
        const Fr ev[6] = {pk.ev_a, pk.ev_b, pk.ev_c, pk.ev_s1, pk.ev_s2, pk.ev_zw};
        for (int i = 0; i < 6; i++) putf(o.evals, i, ev[i]);
        lap(4);
    }
    if (upto >= 5) { pk.round5(); putf(o.challenges, 4, pk.v[0]); put(7, pk.commit_wxi); put(8, pk.commit_wxiw); lap(5); }
    driver.verify_received_vectors();                                              // range check of the vectors received from peers (counted on the device)
}
// the plain driver on `res`: full_witness = n_vars - n_additions elements (leading one, public inputs, private witness)
void plonk_prove_plain_on(cg_ctx* ctx, const cgh::PlonkResident& res, const uint64_t* full_witness, const uint64_t* blind, int upto, const PlonkOut& o) {
    using namespace cgh;
    const PlonkZKey& z = res.z;
    const Fr* w = (const Fr*)full_witness;
    std::vector<Fr> pub(w, w + z.n_public + 1);
    HipDriver driver(ctx, z.curve, Mode::Plain, nullptr);
    ShareVec wit = driver.upload_vec(w + z.n_public + 1, nullptr, res.n_priv);
    FieldShare b[11]; for (int i = 0; i < 11; i++) { memcpy(b[i].c[0].v, blind + 4 * i, 32); b[i].c[1] = b[i].c[0]; }
    try { plonk_run(driver, res, pub, wit, b, upto, o); } catch (...) { driver.free_vec(wit); throw; }
    driver.free_vec(wit);
}
// ONE REP3 party on `res` with the caller's network and randomness (cgh_plonk_prove_rep3_party_ex, cgh_plonk_session_prove_rep3_party)
void plonk_prove_rep3_party_on(cg_ctx* ctx, const cgh::PlonkResident& res, const uint64_t* pub_in, const uint64_t* wit_a, const uint64_t* wit_b,
                               const uint64_t* blind_a, const uint64_t* blind_b, const cgh_rep3_net* net_cb, const cgh_rep3_rand* rnd_cb,
                               const cgh_rep3_chacha* streams_cb, int upto, const PlonkOut& o) {
    using namespace cgh;
    const PlonkZKey& z = res.z;
    std::vector<Fr> pub((const Fr*)pub_in, (const Fr*)pub_in + z.n_public + 1);
    CallbackNetwork net(*net_cb);
    CallbackRand rnd(*rnd_cb);
    rnd.describe_streams(streams_cb);
    HipDriver driver(ctx, z.curve, Mode::Rep3, &net);
    driver.rsrc = &rnd;
    FieldShare b[11];
    for (int t = 0; t < 11; t++) {
        if (blind_a) { memcpy(b[t].c[0].v, blind_a + 4 * t, 32); memcpy(b[t].c[1].v, blind_b + 4 * t, 32); }
        else b[t] = driver.rand();
    }
    ShareVec wit = driver.upload_vec((const Fr*)wit_a, (const Fr*)wit_b, res.n_priv);
    try { plonk_run(driver, res, pub, wit, b, upto, o); }
    catch (...) { driver.free_vec(wit); throw; }
    driver.free_vec(wit);
    rnd.settle();
}
// ---- ONE Shamir party (co-circom.rs:507-527 with the plonk prover): the caller's any-to-any network, its private randomness as a callback
// table or as a seed of the library's own ChaCha12 stream
// Double sharings ONE co-plonk proof consumes on a domain of n rows (N = 4n), read off CoPlonk's calls — every exchanging mul_vec of m
// elements and every rand_vec(m) pops m pairs, a scalar rand() one; the degree-2t openings (mul_open_vec), the point openings and
// rounds 1, 4 and 5 pop none:
//   round 2 (round2.rs:162-229)   4 n            num b, den b, num c, den c
//                                 2 (4 n + 2)    array_prod_mul x 2: rand_vec(n + 1), inv_many's rand_vec(n + 1), two mul_vec of n
//                                 2 n            inv_many(den)'s rand_vec(n), z = num * den^-1
//   round 3 (round3.rs:17-72, 333-418)  36 N     the gate constraint's 4 products and 2 x 16 of mul4vec, each of N = 4 n elements
//   blindings drawn inside        11             b_1..b_11 with rand() (round1.rs:93-99)
// = 158 n + 4 (+ 11).  It depends on the zkey through the domain size only: neither n_public, the additions nor the threshold enter.
size_t plonk_shamir_pairs(const cgh::PlonkZKey& z, bool with_blinding) { return 158 * z.domain_size + 4 + (with_blinding ? 11 : 0); }
// round_seconds[6]: preprocessing, rounds 1..5 (round 1 includes drawing the blindings and the witness upload); pair_stats[4]: pairs
// consumed, pairs left, lazy buffer_triples batches, pairs read from the device-resident block
void plonk_prove_shamir_party_on(cg_ctx* ctx, const cgh::PlonkResident& res, int32_t threshold, const uint64_t* pub_in, const uint64_t* wit_in, const uint64_t* blind,
                                 const cgh_shamir_net* net_cb, const cgh_shamir_rand* rnd_cb, const uint8_t* seed32, size_t preprocess, int upto, const PlonkOut& o,
                                 double* round_seconds, size_t* pair_stats) {
    using namespace cgh;
    const PlonkZKey& z = res.z;
    std::vector<Fr> pub((const Fr*)pub_in, (const Fr*)pub_in + z.n_public + 1);
    CallbackShamirNet net(*net_cb);
    HipDriver driver(ctx, z.curve, Mode::Shamir, nullptr);
    driver.become_shamir_party(&net, threshold, ShamirRandom(rnd_cb, seed32));         // ShamirProtocol::new, shamir.rs:211-246
    if (round_seconds) for (int i = 0; i < 6; i++) round_seconds[i] = 0;
    const auto t0 = std::chrono::steady_clock::now();
    driver.sh.preprocess(preprocess);                                                  // shamir.rs:248-250; 0 = lazy batches of 1024
    if (round_seconds) { CG(cg_ctx_sync(ctx)); round_seconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    FieldShare b[11];
    for (int q = 0; q < 11; q++) {
        if (blind) { memcpy(b[q].c[0].v, blind + 4 * q, 32); b[q].c[1] = b[q].c[0]; }
        else b[q] = driver.rand();                                                      // round1.rs:93-99, before anything else
    }
    ShareVec wit = driver.upload_vec((const Fr*)wit_in, nullptr, res.n_priv);
    try { plonk_run(driver, res, pub, wit, b, upto, o, round_seconds ? round_seconds + 1 : nullptr); }
    catch (...) { driver.free_vec(wit); throw; }
    driver.free_vec(wit);
    if (pair_stats) { const PairStack& ps = driver.sh.pairs; pair_stats[0] = ps.consumed; pair_stats[1] = ps.size(); pair_stats[2] = ps.lazy_batches; pair_stats[3] = ps.from_device; }
}
}  // namespace
// PlainHipDriver through rounds 1..upto (<= 5).  full_witness = n_vars - n_additions Montgomery elements (Groth16-style, leading one);
// blind = 11 Fr; commits = 9 packed G1 (a, b, c, z, t1, t2, t3, wxi, wxiw; zero = not reached), challenges = beta, gamma, alpha, xi, v;
// evals = a, b, c, s1, s2, zw; optional: t_polys = t1 (n+1) | t2 (n+1) | t3 (n+6), poly_z (n+3)
int32_t cgh_plonk_prove_plain(int32_t device, int32_t curve, const char* zkey_path, const uint64_t* full_witness, const uint64_t* blind, int32_t upto,
                              uint64_t* commits, uint64_t* challenges, uint64_t* evals, uint64_t* t_polys, uint64_t* poly_z) {
    cg_ctx* ctx = nullptr;
    try {
        using namespace cgh;
        PlonkZKey zk = read_plonk_zkey(curve, zkey_path);
        if (cg_ctx_create(device, &ctx)) die("cg_ctx_create");
        const Curve c = zk.curve;
        if (commits) memset(commits, 0, 9 * c.aff(CG_G1)); if (challenges) memset(challenges, 0, 5 * 32); if (evals) memset(evals, 0, 6 * 32);
        {
            PlonkResident res(ctx, std::move(zk), 0, validate_by_default());          // transient: this call's copy of the zkey on the device
            plonk_prove_plain_on(ctx, res, full_witness, blind, upto, PlonkOut{commits, challenges, evals, t_polys, poly_z});
        }
        cg_ctx_destroy(ctx);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); if (ctx) cg_ctx_destroy(ctx); return 1; }
}
// Keccak256 transcript hook (tests): kinds[i] 0 = scalar (Fr), 1 = packed G1 point
int32_t cgh_plonk_transcript(int32_t curve, const int32_t* kinds, const uint64_t* const* payloads, int32_t n_items, uint64_t* out_challenge) {
    try {
        using namespace cgh;
        Curve c{curve};
        PlonkTranscript t(c);
        for (int i = 0; i < n_items; i++) { if (kinds[i] == 0) { Fr s; memcpy(s.v, payloads[i], 32); t.add_scalar(s); } else t.add_point((const uint8_t*)payloads[i]); }
        Fr r = t.get_challenge(); memcpy(out_challenge, r.v, 32);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
// ShamirHipProtocol x n (threshold t) through rounds 1..upto.  wit[i] / blind[i] = party i's Shamir shares of the private witness and of
// b_1..b_11; streams[i] = party i's private randomness.  Outputs as for cgh_plonk_prove_rep3, n parties.
int32_t cgh_plonk_prove_shamir(int32_t device, int32_t curve, const char* zkey_path, int32_t n, int32_t t, const uint64_t* pub_in, const uint64_t* const* wit,
                               const uint64_t* const* blind, const uint64_t* const* streams, size_t stream_len, int32_t upto,
                               uint64_t* out_commits, uint64_t* out_evals, uint64_t* out_challenges) {
    try {
        using namespace cgh;
        if (n < 3) throw std::runtime_error("Shamir protocol requires at least 3 parties");
        PlonkZKey z = read_plonk_zkey(curve, zkey_path);
        const Curve c = z.curve;
        const size_t n_priv = z.n_vars - z.n_additions - z.n_public - 1, psz = c.aff(CG_G1);
        std::vector<Fr> pub((const Fr*)pub_in, (const Fr*)pub_in + z.n_public + 1);
        memset(out_commits, 0, (size_t)n * 9 * psz); if (out_evals) memset(out_evals, 0, (size_t)n * 6 * 32); if (out_challenges) memset(out_challenges, 0, (size_t)n * 5 * 32);
        cg_ctx* ctx0 = nullptr;
        if (cg_ctx_create(device, &ctx0)) die("cg_ctx_create");
        std::unique_ptr<PlonkResident> res;
        try { res.reset(new PlonkResident(ctx0, std::move(z), 0, validate_by_default())); } catch (...) { cg_ctx_destroy(ctx0); throw; }
        InProcShamirHub hub(n);
        std::vector<std::string> errs(n);
        std::vector<std::thread> th;
        for (int i = 0; i < n; i++) th.emplace_back([&, i] {
            cg_ctx* ctx = nullptr;
            try {
                if (cg_ctx_create(device, &ctx)) die("cg_ctx_create");
                InProcShamirNet net(&hub, i);
                {
                    HipDriver driver(ctx, c, Mode::Shamir, nullptr);
                    driver.become_shamir_party(&net, t, ShamirRandom((const Fr*)streams[i], stream_len));
                    ShareVec w = driver.upload_vec((const Fr*)wit[i], nullptr, n_priv);
                    FieldShare b[11]; for (int q = 0; q < 11; q++) { memcpy(b[q].c[0].v, blind[i] + 4 * q, 32); b[q].c[1] = b[q].c[0]; }
                    plonk_run(driver, *res, pub, w, b, upto, PlonkOut{(uint64_t*)((uint8_t*)out_commits + (size_t)i * 9 * psz), out_challenges ? out_challenges + i * 20 : nullptr,
                                                                        out_evals ? out_evals + i * 24 : nullptr, nullptr, nullptr});
                    driver.free_vec(w);
                }
                cg_ctx_destroy(ctx);
            } catch (const std::exception& e) { errs[i] = e.what(); hub.abort(); if (ctx) cg_ctx_destroy(ctx); }
        });
        for (auto& x : th) x.join();
        res.reset();
        cg_ctx_destroy(ctx0);
        if (report_party_errors(errs, n)) return 1;
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
// Rep3HipProtocol x 3 (three threads, in-process network) through rounds 1..upto.  blind_a[i] / blind_b[i] = party i's (a, b) shares of
// b_1..b_11; streams[i] = S_i (party i: rng1 = S_i, rng2 = S_{i-1}; rounds 2 and 3 consume masks and random shares).
// out_commits = 3 parties x 9 packed G1, out_evals = 3 x 6 Fr, out_challenges = 3 x 5 Fr (every party must report the same values)
int32_t cgh_plonk_prove_rep3(int32_t device, int32_t curve, const char* zkey_path, const uint64_t* pub_in, const uint64_t* const* wit_a, const uint64_t* const* wit_b,
                             const uint64_t* const* blind_a, const uint64_t* const* blind_b, const uint64_t* const* streams, size_t stream_len, int32_t upto,
                             uint64_t* out_commits, uint64_t* out_evals, uint64_t* out_challenges) {
    try {
        using namespace cgh;
        PlonkZKey z = read_plonk_zkey(curve, zkey_path);
        const Curve c = z.curve;
        const size_t n_priv = z.n_vars - z.n_additions - z.n_public - 1, psz = c.aff(CG_G1);
        std::vector<Fr> pub((const Fr*)pub_in, (const Fr*)pub_in + z.n_public + 1);
        memset(out_commits, 0, 3 * 9 * psz); if (out_evals) memset(out_evals, 0, 3 * 6 * 32); if (out_challenges) memset(out_challenges, 0, 3 * 5 * 32);
        cg_ctx* ctx0 = nullptr;
        if (cg_ctx_create(device, &ctx0)) die("cg_ctx_create");
        std::unique_ptr<PlonkResident> res;
        try { res.reset(new PlonkResident(ctx0, std::move(z), 0, validate_by_default())); } catch (...) { cg_ctx_destroy(ctx0); throw; }
        InProcHub hub;
        std::string errs[3];
        std::vector<std::thread> th;
        for (int i = 0; i < 3; i++) th.emplace_back([&, i] {
            cg_ctx* ctx = nullptr;
            try {
                if (cg_ctx_create(device, &ctx)) die("cg_ctx_create");
                InProcNetwork net(&hub, i);
                {
                    HipDriver driver(ctx, c, Mode::Rep3, &net);
                    if (streams) { driver.rng1 = (const Fr*)streams[i]; driver.rng2 = (const Fr*)streams[(i + 2) % 3]; driver.rng_len = stream_len; }
                    ShareVec wit = driver.upload_vec((const Fr*)wit_a[i], (const Fr*)wit_b[i], n_priv);
                    FieldShare b[11]; for (int t = 0; t < 11; t++) { memcpy(b[t].c[0].v, blind_a[i] + 4 * t, 32); memcpy(b[t].c[1].v, blind_b[i] + 4 * t, 32); }
                    plonk_run(driver, *res, pub, wit, b, upto, PlonkOut{(uint64_t*)((uint8_t*)out_commits + (size_t)i * 9 * psz), out_challenges ? out_challenges + i * 20 : nullptr,
                                                                          out_evals ? out_evals + i * 24 : nullptr, nullptr, nullptr});
                    driver.free_vec(wit);
                }
                cg_ctx_destroy(ctx);
            } catch (const std::exception& e) { errs[i] = e.what(); hub.abort(); if (ctx) cg_ctx_destroy(ctx); }
        });
        for (auto& t : th) t.join();
        res.reset();
        cg_ctx_destroy(ctx0);
        if (report_party_errors(errs, 3)) return 1;
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}


// ONE REP3 party of co-plonk with the caller's network and correlated randomness (co-circom.rs:560-600 builds a Rep3Protocol and hands it to
// CoPlonk::prove; the tables are those of cgh_session_prove_rep3_party).  blind_a / blind_b = this party's shares of b_1..b_11, or both NULL to
// draw them with rand() in the reference's order (round1.rs:93-99) before anything else.  Outputs: 9 packed G1, 6 evaluations, 5 challenges.
int32_t cgh_plonk_prove_rep3_party(int32_t device, int32_t curve, const char* zkey_path, const uint64_t* pub_in, const uint64_t* wit_a, const uint64_t* wit_b,
                                   const uint64_t* blind_a, const uint64_t* blind_b, const cgh_rep3_net* net_cb, const cgh_rep3_rand* rnd_cb, int32_t upto,
                                   uint64_t* out_commits, uint64_t* out_evals, uint64_t* out_challenges) {
    return cgh_plonk_prove_rep3_party_ex(device, curve, zkey_path, pub_in, wit_a, wit_b, blind_a, blind_b, net_cb, rnd_cb, nullptr, upto, out_commits, out_evals, out_challenges);
}
// streams_cb != NULL: the masking vectors of the rounds' mul_vec calls (round2.rs / round3.rs) are drawn on the GPU from the described generators
int32_t cgh_plonk_prove_rep3_party_ex(int32_t device, int32_t curve, const char* zkey_path, const uint64_t* pub_in, const uint64_t* wit_a, const uint64_t* wit_b,
                                      const uint64_t* blind_a, const uint64_t* blind_b, const cgh_rep3_net* net_cb, const cgh_rep3_rand* rnd_cb,
                                      const cgh_rep3_chacha* streams_cb, int32_t upto, uint64_t* out_commits, uint64_t* out_evals, uint64_t* out_challenges) {
    cg_ctx* ctx = nullptr;
    try {
        using namespace cgh;
        if (!zkey_path || !pub_in || !wit_a || !wit_b || !net_cb || !rnd_cb || !out_commits) throw std::runtime_error("cgh_plonk_prove_rep3_party: null argument");
        if ((blind_a == nullptr) != (blind_b == nullptr)) throw std::runtime_error("cgh_plonk_prove_rep3_party: blind_a and blind_b go together");
        if (upto < 1 || upto > 5) throw std::runtime_error("cgh_plonk_prove_rep3_party: upto must be 1..5");
        PlonkZKey z = read_plonk_zkey(curve, zkey_path);
        const size_t psz = z.curve.aff(CG_G1);
        memset(out_commits, 0, 9 * psz); if (out_evals) memset(out_evals, 0, 6 * 32); if (out_challenges) memset(out_challenges, 0, 5 * 32);
        if (cg_ctx_create(device, &ctx)) die("cg_ctx_create");
        {
            PlonkResident res(ctx, std::move(z), 0, validate_by_default());
            plonk_prove_rep3_party_on(ctx, res, pub_in, wit_a, wit_b, blind_a, blind_b, net_cb, rnd_cb, streams_cb, upto, PlonkOut{out_commits, out_challenges, out_evals, nullptr, nullptr});
        }
        cg_ctx_destroy(ctx);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); if (ctx) cg_ctx_destroy(ctx); return 1; }
}

// ONE Shamir party of n (net->num_parties) with threshold t through rounds 1..upto on a transient copy of the zkey
int32_t cgh_plonk_prove_shamir_party(int32_t device, int32_t curve, const char* zkey_path, int32_t threshold, const uint64_t* pub_in, const uint64_t* wit, const uint64_t* blind,
                                     const cgh_shamir_net* net, const cgh_shamir_rand* rnd, size_t preprocess, int32_t upto, uint64_t* out_commits, uint64_t* out_evals,
                                     uint64_t* out_challenges, double* seconds, double* round_seconds, size_t* pair_stats) {
    cg_ctx* ctx = nullptr;
    try {
        using namespace cgh;
        if (!zkey_path || !rnd) throw std::runtime_error("cgh_plonk_prove_shamir_party: null argument");
        shamir_party_args("cgh_plonk_prove_shamir_party", threshold, net, rnd, nullptr, pub_in, wit, out_commits);
        if (upto < 1 || upto > 5) throw std::runtime_error("cgh_plonk_prove_shamir_party: upto must be 1..5");
        PlonkZKey z = read_plonk_zkey(curve, zkey_path);
        const size_t psz = z.curve.aff(CG_G1);
        memset(out_commits, 0, 9 * psz); if (out_evals) memset(out_evals, 0, 6 * 32); if (out_challenges) memset(out_challenges, 0, 5 * 32);
        if (cg_ctx_create(device, &ctx)) die("cg_ctx_create");
        const auto t0 = std::chrono::steady_clock::now();
        {
            PlonkResident res(ctx, std::move(z), 0, validate_by_default());
            plonk_prove_shamir_party_on(ctx, res, threshold, pub_in, wit, blind, net, rnd, nullptr, preprocess, upto, PlonkOut{out_commits, out_challenges, out_evals, nullptr, nullptr},
                                        round_seconds, pair_stats);
        }
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        cg_ctx_destroy(ctx);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); if (ctx) { cg_ctx_sync(ctx); cg_ctx_destroy(ctx); } return 1; }
}

// ---- co-plonk proving sessions: the zkey is read, uploaded and p_tau registered (validated, optionally given per-window tables) ONCE
// (co-circom.rs:546-590 does that work once per prover process); proofs then read the resident copy (PlonkResident).  One proof at a time
// per session; parties of one process open a session each.
struct cgh_plonk_session {
    cg_ctx* ctx = nullptr;
    std::unique_ptr<cgh::PlonkResident> res;
    std::unique_ptr<cgh::PlonkVerifyingKey> vk;                                          // cgh_plonk_session_verify: prepared from the zkey's header at first use (under vk_mu)
    std::mutex mu, vk_mu;
    void* q_rows[5] = {};                                                                // cgh_plonk_session_check_witness: the selectors on the n rows, gathered at first use (under mu)
    ~cgh_plonk_session() { for (void* p : q_rows) if (p) cg_dev_free(ctx, p); res.reset(); if (ctx) cg_ctx_destroy(ctx); }
};
namespace {
cgh_plonk_session* plonk_session(void* s, const char* who) { if (!s) throw std::runtime_error(std::string(who) + ": null session"); return (cgh_plonk_session*)s; }
// a failed proof may leave work on the context's stream: wait for it (errors included) before the session serves the next proof
void plonk_session_settle(cgh_plonk_session* s) { if (s && s->ctx) cg_ctx_sync(s->ctx); }
}  // namespace
int32_t cgh_plonk_session_open(int32_t device, int32_t curve, const char* zkey_path, int32_t precompute, uint32_t flags, void** out_session) {
    cgh_plonk_session* s = nullptr;
    try {
        using namespace cgh;
        if (!zkey_path || !out_session) throw std::runtime_error("cgh_plonk_session_open: null argument");
        *out_session = nullptr;
        PlonkZKey z = read_plonk_zkey(curve, zkey_path);
        s = new cgh_plonk_session();
        if (cg_ctx_create(device, &s->ctx)) die("cg_ctx_create");
        s->res.reset(new PlonkResident(s->ctx, std::move(z), precompute, !(flags & CGH_SESSION_SKIP_VALIDATION)));
        *out_session = s;
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); delete s; return 1; }
}
int32_t cgh_plonk_session_info(void* session, size_t* info) {
    try {
        const cgh_plonk_session* s = plonk_session(session, "cgh_plonk_session_info");
        if (!info) throw std::runtime_error("cgh_plonk_session_info: null argument");
        const cgh::PlonkZKey& z = s->res->z;
        info[0] = z.n_vars; info[1] = z.n_public; info[2] = z.domain_size; info[3] = z.power; info[4] = z.n_additions; info[5] = z.n_constraints;
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_plonk_session_close(void* session) {
    delete (cgh_plonk_session*)session;
    return 0;
}
int32_t cgh_plonk_session_verify(void* session, const uint64_t* commits, const uint64_t* evals, const uint64_t* pub, int32_t* ok) {
    try {
        cgh_plonk_session* s = plonk_session(session, "cgh_plonk_session_verify");
        const cgh::PlonkZKey& z = s->res->z;
        if (!commits || !evals || !ok || (z.n_public && !pub)) throw std::runtime_error("cgh_plonk_session_verify: null argument");
        { std::lock_guard<std::mutex> l(s->vk_mu); if (!s->vk) s->vk.reset(new cgh::PlonkVerifyingKey(cgh::plonk_vk_from_zkey_data(z))); }
        *ok = cgh::plonk_verify(*s->vk, (const uint8_t*)commits, evals, pub, z.n_public) ? 1 : 0; return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_plonk_session_prove_plain(void* session, const uint64_t* full_witness, const uint64_t* blind, uint64_t* commits, uint64_t* evals, uint64_t* challenges, double* seconds) {
    cgh_plonk_session* s = nullptr;
    try {
        s = plonk_session(session, "cgh_plonk_session_prove_plain");
        if (!full_witness || !blind || !commits) throw std::runtime_error("cgh_plonk_session_prove_plain: null argument");
        std::lock_guard<std::mutex> lock(s->mu);
        const auto t0 = std::chrono::steady_clock::now();
        memset(commits, 0, 9 * s->res->z.curve.aff(CG_G1)); if (evals) memset(evals, 0, 6 * 32); if (challenges) memset(challenges, 0, 5 * 32);
        plonk_prove_plain_on(s->ctx, *s->res, full_witness, blind, 5, PlonkOut{commits, challenges, evals, nullptr, nullptr});
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); plonk_session_settle(s); return 1; }
}
int32_t cgh_plonk_session_check_witness(void* session, const uint64_t* full_witness, uint64_t* n_bad, uint64_t* first_bad) {
    cgh_plonk_session* s = nullptr;
    try {
        s = plonk_session(session, "cgh_plonk_session_check_witness");
        if (!full_witness || !n_bad || !first_bad) throw std::runtime_error("cgh_plonk_session_check_witness: null argument");
        std::lock_guard<std::mutex> lock(s->mu);
        const size_t n = s->res->z.domain_size;
        for (int i = 0; i < 5; i++) if (!s->q_rows[i]) {                               // 5 n elements, kept until close
            void* p = nullptr;
            if (cg_dev_alloc(s->ctx, n * 32, &p)) cgh::die("cg_dev_alloc");
            if (cg_vec_gather_strided_dev(s->ctx, s->res->z.curve.id, p, s->res->q_eval[i], n, 0, 4)) { cg_dev_free(s->ctx, p); cgh::die("cg_vec_gather_strided_dev"); }
            s->q_rows[i] = p;
        }
        cgh::plonk_check_witness(s->ctx, *s->res, s->q_rows, (const cgh::Fr*)full_witness, n_bad, first_bad);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); plonk_session_settle(s); return 1; }
}
int32_t cgh_plonk_session_audit_timed(void* session, void* r1cs, const uint8_t* seed32, uint32_t* failed, uint64_t* detail, double* stage_seconds) {
    cgh_plonk_session* s = nullptr;
    try {
        s = plonk_session(session, "cgh_plonk_session_audit");
        if (!failed || !detail) throw std::runtime_error("cgh_plonk_session_audit: null argument");
        std::lock_guard<std::mutex> lock(s->mu);
        cgh::plonk_audit(s->ctx, *s->res, (cgh::R1csHandle*)r1cs, seed32, failed, detail, stage_seconds);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); plonk_session_settle(s); return 1; }
}
int32_t cgh_plonk_session_audit(void* session, void* r1cs, const uint8_t* seed32, uint32_t* failed, uint64_t* detail) {
    return cgh_plonk_session_audit_timed(session, r1cs, seed32, failed, detail, nullptr);
}
int32_t cgh_plonk_session_prove_rep3_party(void* session, const uint64_t* pub_in, const uint64_t* wit_a, const uint64_t* wit_b, const uint64_t* blind_a, const uint64_t* blind_b,
                                           const cgh_rep3_net* net, const cgh_rep3_rand* rnd, const cgh_rep3_chacha* streams, uint64_t* commits, uint64_t* evals,
                                           uint64_t* challenges, double* seconds) {
    cgh_plonk_session* s = nullptr;
    try {
        s = plonk_session(session, "cgh_plonk_session_prove_rep3_party");
        if (!pub_in || !wit_a || !wit_b || !net || !rnd || !commits) throw std::runtime_error("cgh_plonk_session_prove_rep3_party: null argument");
        if ((blind_a == nullptr) != (blind_b == nullptr)) throw std::runtime_error("cgh_plonk_session_prove_rep3_party: blind_a and blind_b go together");
        std::lock_guard<std::mutex> lock(s->mu);
        const auto t0 = std::chrono::steady_clock::now();
        memset(commits, 0, 9 * s->res->z.curve.aff(CG_G1)); if (evals) memset(evals, 0, 6 * 32); if (challenges) memset(challenges, 0, 5 * 32);
        plonk_prove_rep3_party_on(s->ctx, *s->res, pub_in, wit_a, wit_b, blind_a, blind_b, net, rnd, streams, 5, PlonkOut{commits, challenges, evals, nullptr, nullptr});
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); plonk_session_settle(s); return 1; }
}
// ONE Shamir party on a session (the twin of cgh_session_prove_shamir_party{,_seeded}); rnd or seed32, never both
static int32_t plonk_session_shamir_party(const char* who, void* session, int32_t threshold, const uint64_t* pub_in, const uint64_t* wit, const uint64_t* blind, const cgh_shamir_net* net,
                                          const cgh_shamir_rand* rnd, const uint8_t* seed32, size_t preprocess, uint64_t* commits, uint64_t* evals, uint64_t* challenges,
                                          double* seconds, double* round_seconds, size_t* pair_stats) {
    cgh_plonk_session* s = nullptr;
    try {
        shamir_party_args(who, threshold, net, rnd, seed32, pub_in, wit, commits);
        s = plonk_session(session, who);
        std::lock_guard<std::mutex> lock(s->mu);
        const auto t0 = std::chrono::steady_clock::now();
        memset(commits, 0, 9 * s->res->z.curve.aff(CG_G1)); if (evals) memset(evals, 0, 6 * 32); if (challenges) memset(challenges, 0, 5 * 32);
        plonk_prove_shamir_party_on(s->ctx, *s->res, threshold, pub_in, wit, blind, net, rnd, seed32, preprocess, 5, PlonkOut{commits, challenges, evals, nullptr, nullptr}, round_seconds, pair_stats);
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); plonk_session_settle(s); return 1; }
}
int32_t cgh_plonk_session_prove_shamir_party(void* session, int32_t threshold, const uint64_t* pub_in, const uint64_t* wit, const uint64_t* blind, const cgh_shamir_net* net,
                                             const cgh_shamir_rand* rnd, size_t preprocess, uint64_t* commits, uint64_t* evals, uint64_t* challenges,
                                             double* seconds, double* round_seconds, size_t* pair_stats) {
    if (!rnd) { g_host_err = "cgh_plonk_session_prove_shamir_party: null argument"; return 1; }
    return plonk_session_shamir_party("cgh_plonk_session_prove_shamir_party", session, threshold, pub_in, wit, blind, net, rnd, nullptr, preprocess, commits, evals, challenges, seconds, round_seconds, pair_stats);
}
int32_t cgh_plonk_session_prove_shamir_party_seeded(void* session, int32_t threshold, const uint64_t* pub_in, const uint64_t* wit, const uint64_t* blind, const cgh_shamir_net* net,
                                                    const uint8_t* seed32, size_t preprocess, uint64_t* commits, uint64_t* evals, uint64_t* challenges,
                                                    double* seconds, double* round_seconds, size_t* pair_stats) {
    if (!seed32) { g_host_err = "cgh_plonk_session_prove_shamir_party_seeded: null argument"; return 1; }
    return plonk_session_shamir_party("cgh_plonk_session_prove_shamir_party_seeded", session, threshold, pub_in, wit, blind, net, nullptr, seed32, preprocess, commits, evals, challenges, seconds, round_seconds, pair_stats);
}
int32_t cgh_plonk_session_shamir_pairs(void* session, int32_t threshold, int32_t with_blinding, size_t* out_pairs) {
    try {
        if (!out_pairs) throw std::runtime_error("cgh_plonk_session_shamir_pairs: null argument");
        if (threshold < 0) throw std::runtime_error("cgh_plonk_session_shamir_pairs: negative threshold");
        const cgh_plonk_session* s = plonk_session(session, "cgh_plonk_session_shamir_pairs");
        *out_pairs = plonk_shamir_pairs(s->res->z, with_blinding != 0);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}

}  // extern "C"
