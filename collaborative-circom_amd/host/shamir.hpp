// One Shamir party (mpc-core/src/protocols/shamir.rs): its private randomness, the LIFO of buffered double sharings and the protocol steps
// over them.  Included by driver.hpp between DriverBase, which the steps use for the device, and HipDriver, whose Mode::Shamir branches call in.
#pragma once
namespace cgh {
// ---- the party's PRIVATE randomness (`RngType::from_entropy()`, shamir.rs:211-246: no peer reproduces its draws), in this order of precedence: a ChaCha12
// generator seeded by the caller for this proof and positioned here (long draws are made on the device, short ones on the host: ONE stream); the caller's RNG behind a callback; a stream of drawn values
struct ShamirRandom {
    ChaCha12 gen; bool seeded = false; const cgh_shamir_rand* cb = nullptr;
    const Fr* stream = nullptr; size_t stream_len = 0, cursor = 0;
    ShamirRandom(const Fr* s = nullptr, size_t n = 0) : stream(s), stream_len(n) {}
    ShamirRandom(const cgh_shamir_rand* c, const uint8_t* seed32) : cb(c) { if (seed32) { gen = ChaCha12(seed32); seeded = true; } }
    void need(size_t n) const { if (!seeded && !cb && cursor + n > stream_len) throw std::runtime_error("randomness stream exhausted"); }   // only a stream can run out
    void draw(const Curve& curve, size_t n, Fr* out) {
        if (seeded) { for (size_t i = 0; i < n; i++) gen.fr_rand(MOD_R[curve.id], curve.id == CG_BN254 ? 254 : 255, out[i].v); return; }
        if (cb) { if (const int32_t rc = cb->random_field_elements(cb->user, n, (uint64_t*)out)) throw std::runtime_error("randomness source: random_field_elements failed with code " + std::to_string(rc)); return; }
        need(n); memcpy(out, stream + cursor, n * 32); cursor += n;
    }
    // the next n draws into a device buffer: made there (seeded, from DEVICE_MASKS_MIN on: the generator's position follows), or made here and uploaded; a stream goes up from where it lies
    void draw_dev(DriverBase& d, size_t n, void* d_out) {
        if (seeded && n >= d.DEVICE_MASKS_MIN) { uint64_t after = 0; CG(cg_chacha12_fr_rand_dev(d.ctx, d.curve.id, (const uint8_t*)gen.key, gen.word_pos, n, d_out, &after)); gen.word_pos = after; }
        else if (seeded || cb) { std::vector<Fr> tmp(n); draw(d.curve, n, tmp.data()); CG(cg_dev_upload(d.ctx, d_out, tmp.data(), n * 32)); }
        else { need(n); CG(cg_dev_upload(d.ctx, d_out, stream + cursor, n * 32)); cursor += n; }
    }
};

// ---- the LIFO of double sharings (r_t, r_2t), shamir.rs:873-880.  Invariant: the host vectors hold every entry, EXCEPT that while !on_host the entries
// [base, base + dn) — one preprocessed block — are valid in d_rt / d_r2t only and unwritten on the host (FrLazyVec: resize() does not touch them).  Entries
// above the block are host entries; pops never move `base`: the block's live part is [base, min(size(), base + dn)).  Nothing outside this class reads these fields.
class PairStack {
    cg_ctx* ctx; FrLazyVec r_t, r_2t;
    void* d_rt = nullptr; void* d_r2t = nullptr; size_t base = 0, dn = 0; bool on_host = true;
    void shrink(size_t n, bool from_dev) { r_t.resize(r_t.size() - n); r_2t.resize(r_2t.size() - n); consumed += n; if (from_dev) from_device += n; }
public:
    // pair_stats of the co-plonk party entries: pairs popped, lazy batches made by ShamirParty::get_pair, pairs read from the device-resident block without passing through the host
    size_t consumed = 0, lazy_batches = 0, from_device = 0;
    explicit PairStack(cg_ctx* c) : ctx(c) {}
    size_t size() const { return r_t.size(); }
    void append_host(const std::vector<Fr>& t, const std::vector<Fr>& t2) { r_t.insert(r_t.end(), t.begin(), t.end()); r_2t.insert(r_2t.end(), t2.begin(), t2.end()); }
    void release() { if (d_rt) { cg_dev_free(ctx, d_rt); cg_dev_free(ctx, d_r2t); d_rt = d_r2t = nullptr; } dn = 0; on_host = true; }
    void materialize() {                                                               // the block's live part moves to the host: one download per half
        const size_t live = on_host ? 0 : std::min(dn, size() > base ? size() - base : 0);
        if (live) { CG(cg_dev_download(ctx, r_t.data() + base, d_rt, live * 32)); CG(cg_dev_download(ctx, r_2t.data() + base, d_r2t, live * 32)); }
        on_host = true;
    }
    // n new pairs that stay on the device (taken over: release() frees them); an earlier block moves to the host first
    void adopt_device_block(void* rt, void* r2t, size_t n) {
        materialize(); release();
        r_t.resize(size() + n); r_2t.resize(r_t.size());                               // (before the block changes hands: nothing below throws)
        base = size() - n; dn = n; d_rt = rt; d_r2t = r2t; on_host = false;
    }
    std::pair<Fr, Fr> pop() {                                                          // the top pair (not empty); a device-only entry costs two 32-byte downloads
        const size_t idx = size() - 1;
        if (!on_host && idx >= base && idx < base + dn) { CG(cg_dev_download(ctx, &r_t[idx], (const Fr*)d_rt + (idx - base), 32)); CG(cg_dev_download(ctx, &r_2t[idx], (const Fr*)d_r2t + (idx - base), 32)); }
        std::pair<Fr, Fr> pr{r_t.back(), r_2t.back()}; shrink(1, false); return pr;
    }
    // the top n pairs when the device block holds them ALL: popped, handed out as views for lincomb (pop i = block entry off - i: stride -1).  false: nothing popped, the caller pops on the host
    struct DevView { const void* rt; const void* r2t; int64_t off; };
    bool pop_vec_dev(size_t n, DevView& v) {
        const size_t top = size();
        if (on_host || top < n || top - n < base || top > base + dn) return false;
        v = DevView{d_rt, d_r2t, (int64_t)(top - 1 - base)}; shrink(n, true); return true;
    }
};

// ---- ShamirProtocol (shamir.rs:196-246): threshold, Lagrange tables, network, randomness, pairs, and the steps that use them
struct ShamirParty {
    DriverBase& d; const Curve& curve;
    ShamirNet* net = nullptr; int t = 0; std::vector<Fr> open_lagrange_t, open_lagrange_2t, mul_lagrange_2t;
    ShamirRandom rnd; PairStack pairs;
    static constexpr size_t BATCH = 1024;                                             // ShamirRng::BATCH_SIZE
    explicit ShamirParty(DriverBase& drv) : d(drv), curve(drv.curve), pairs(drv.ctx) {}
    // ONE page-locked block for the messages of degree_reduce_vec / mul_open_vec, grown to the longest vector seen: every copy through it is synchronous, so the next call may reuse it
    Fr* stage_buf = nullptr; size_t stage_n = 0;
    Fr* stage(size_t n) {
        if (n > stage_n) { if (stage_buf) { CG(cg_host_free(stage_buf)); stage_buf = nullptr; stage_n = 0; } void* p; CG(cg_host_alloc(std::max<size_t>(n, 1) * 32, &p)); stage_buf = (Fr*)p; stage_n = n; }
        return stage_buf;
    }
    void release() { pairs.release(); if (stage_buf) { cg_host_free(stage_buf); stage_buf = nullptr; stage_n = 0; } }   // HipDriver::shutdown
    // ShamirCore::share of `len` device-resident secrets for every receiver in one launch (cg_shamir_share_dev)
    void share_dev(const void* secrets, const void* coeffs, int64_t coeff_off, int64_t coeff_stride, size_t len, int degree, const std::vector<void*>& outs, int64_t out_off, int64_t out_stride) {
        CG(cg_shamir_share_dev(d.ctx, curve.id, secrets, coeffs, coeff_off, coeff_stride, len, degree, (int32_t)outs.size(), outs.data(), out_off, out_stride));
    }
    Fr next_rand() { Fr x; rnd.draw(curve, 1, &x); return x; }
    std::vector<Fr> lagrange_from_coeff(const std::vector<size_t>& pts) const {       // shamir_core.rs:56-75
        std::vector<Fr> res;
        for (size_t i : pts) {
            Fr num = fr_from_u64(curve, 1), den = num; const Fr fi = fr_from_u64(curve, i);
            for (size_t j : pts) if (i != j) { const Fr fj = fr_from_u64(curve, j); num = fr_mul(curve, num, fj); den = fr_mul(curve, den, fr_sub(curve, fj, fi)); }
            res.push_back(fr_mul(curve, num, fr_inv(curve, den)));
        }
        return res;
    }
    void init(ShamirNet* n, int threshold, const ShamirRandom& source) {               // ShamirProtocol::new, shamir.rs:211-246
        net = n; t = threshold; rnd = source;
        const int np = n->num_parties(), id = n->id();
        if (2 * threshold + 1 > np) throw std::runtime_error("Threshold too large for number of parties");
        auto table = [&](int count, bool senders) { std::vector<size_t> p; for (int i = 0; i < count; i++) p.push_back(senders ? (size_t)((id + np - i) % np + 1) : (size_t)i + 1); return lagrange_from_coeff(p); };
        open_lagrange_t = table(threshold + 1, true); open_lagrange_2t = table(2 * threshold + 1, true); mul_lagrange_2t = table(2 * threshold + 1, false);
    }
    std::vector<Fr> share(const Fr& secret, const Fr* coeffs, int degree) {            // shamir_core.rs:8-31, the coefficients already drawn
        const int np = net->num_parties();
        std::vector<Fr> shares;
        for (int pidx = 1; pidx <= np; pidx++) {
            Fr sh = secret; const Fr x = fr_from_u64(curve, (uint64_t)pidx); Fr xp = x;
            for (int k = 0; k < degree; k++) { sh = fr_add(curve, sh, fr_mul(curve, xp, coeffs[k])); xp = fr_mul(curve, xp, x); }
            shares.push_back(sh);
        }
        return shares;
    }
    std::vector<Fr> vandermonde_mul(const std::vector<Fr>& in) {                      // shamir.rs:904-921 (t + 1 values)
        const int np = net->num_parties();
        std::vector<Fr> row(np), cur(np), out;
        for (int i = 0; i < np; i++) { row[i] = fr_from_u64(curve, (uint64_t)i + 1); cur[i] = row[i]; }
        Fr s0 = fr_from_u64(curve, 0); for (const Fr& v : in) s0 = fr_add(curve, s0, v);
        out.push_back(s0);
        for (int k = 1; k <= t; k++) {
            Fr acc = fr_from_u64(curve, 0);
            for (int i = 0; i < np; i++) { acc = fr_add(curve, acc, fr_mul(curve, cur[i], in[i])); cur[i] = fr_mul(curve, cur[i], row[i]); }
            out.push_back(acc);
        }
        return out;
    }
    void buffer_triples(size_t amount) {                                               // shamir.rs:923-1010
        const int np = net->num_parties(), me = net->id();
        // the reference's draw order — amount secrets, then per secret t + 2t coefficients — taken in ONE call of the randomness source
        // (a callback per draw cost a lazily fed proof millions of calls)
        const size_t t3 = 3 * (size_t)t;
        std::vector<Fr> r(amount * (1 + t3)); rnd.draw(curve, r.size(), r.data());
        std::vector<std::vector<Fr>> send(np);
        for (size_t k = 0; k < amount; k++) {
            const Fr* co = r.data() + amount + k * t3;
            auto a = share(r[k], co, t), b = share(r[k], co + t, 2 * t);
            for (int to = 0; to < np; to++) { send[to].push_back(a[to]); send[to].push_back(b[to]); }
        }
        for (int to = 0; to < np; to++) if (to != me) net->send(to, send[to].data(), send[to].size() * 32);
        std::vector<std::vector<Fr>> got(np);
        for (int from = 0; from < np; from++) { if (from == me) got[from] = send[me]; else { got[from].resize(2 * amount); net->recv(from, got[from].data(), 2 * amount * 32); d.check_received(got[from].data(), 2 * amount); } }
        for (size_t k = 0; k < amount; k++) {
            std::vector<Fr> in_t(np), in_2t(np);
            for (int from = 0; from < np; from++) { in_t[from] = got[from][2 * k]; in_2t[from] = got[from][2 * k + 1]; }
            pairs.append_host(vandermonde_mul(in_t), vandermonde_mul(in_2t));
        }
    }
    // ShamirProtocol::preprocess (shamir.rs:248-250) = buffer_triples(amount) (shamir.rs:923-1010) with the share algebra on the
    // device: the same draws in the same order (amount secrets, then per secret t + 2t coefficients), the same values appended to the
    // pairs, one message per peer.  The lazily refilled batches of 1024 (get_pair) stay on the host.
    void preprocess(size_t amount) {
        if (!amount) return;
        const int np = net->num_parties(), me = net->id();
        const size_t draws = amount * (size_t)(1 + 3 * t);
        rnd.need(draws);                                                               // before anything is allocated
        DriverBase::Marks mk("shamir preprocess", me == 0);
        DriverBase::DevTmp held(d);                                                    // every buffer of the step (the callbacks below may throw); the two outputs leave it for the pairs at the end
        void* d_rnd = held.get(draws * 32);
        rnd.draw_dev(d, draws, d_rnd);
        mk.mark("upload draws");
        std::vector<void*> d_got(np);
        for (int from = 0; from < np; from++) d_got[from] = held.get(2 * amount * 32);
        Fr* const buf = d.mask_scratch(2 * amount);                                    // page-locked staging (parked by the host cache between proofs): the copies are plain DMA
        // ShamirCore::share for every receiver's point in two launches (degree t into the even, degree 2t into the odd entries): secret k's
        // coefficients are draws amount + 3t k .. + 3t - 1, read where they lie.  Receiver `to`'s message is built in d_got[to], which is
        // overwritten by what `to` sends back once it has left.
        share_dev(d_rnd, d_rnd, (int64_t)amount, 3 * t, amount, t, d_got, 0, 2);
        share_dev(d_rnd, d_rnd, (int64_t)amount + t, 3 * t, amount, 2 * t, d_got, 1, 2);
        for (int to = 0; to < np; to++) if (to != me) { CG(cg_dev_download(d.ctx, buf, d_got[to], 2 * amount * 32)); net->send(to, buf, 2 * amount * 32); }
        mk.mark("share+send");
        for (int from = 0; from < np; from++) if (from != me) { net->recv(from, buf, 2 * amount * 32); CG(cg_dev_upload(d.ctx, d_got[from], buf, 2 * amount * 32)); d.check_received_dev(d_got[from], 2 * amount); }
        mk.mark("recv+upload");
        // Vandermonde rows 1, x, .., x^t over the senders' points (shamir.rs:904-921): t + 1 outputs per secret
        const size_t outn = amount * (size_t)(t + 1);
        void* d_rt = held.get(outn * 32); void* d_r2t = held.get(outn * 32);
        std::vector<Fr> pw(np, fr_from_u64(curve, 1));
        for (int kk = 0; kk <= t; kk++) {
            std::vector<DriverBase::Term> a, b;
            for (int from = 0; from < np; from++) { a.push_back({d_got[from], 0, 2, pw[from]}); b.push_back({d_got[from], 1, 2, pw[from]}); }
            d.lincomb(d_rt, kk, t + 1, amount, a); d.lincomb(d_r2t, kk, t + 1, amount, b);
            for (int from = 0; from < np; from++) pw[from] = fr_mul(curve, pw[from], fr_from_u64(curve, (uint64_t)from + 1));
        }
        pairs.adopt_device_block(d_rt, d_r2t, outn); held.take(d_rt); held.take(d_r2t); held.free_now();
        mk.mark("vandermonde+free");
    }
    // shamir.rs:1012-1025 (LIFO); an empty stack is refilled by one lazy batch, made on the host
    std::pair<Fr, Fr> get_pair() { if (!pairs.size()) { pairs.release(); buffer_triples(BATCH); pairs.lazy_batches++; } return pairs.pop(); }
    // degree_reduce_vec, shamir.rs:302-384.  `local` holds this party's products on the device and is consumed.
    ShareVec degree_reduce_vec(ShareVec local) {
        const int np = net->num_parties(), me = net->id();
        const size_t len = local.n;
        // the len pairs on top of the stack, top first; read straight from the device when the preprocessed block holds them all
        PairStack::DevView top; const bool on_dev = pairs.pop_vec_dev(len, top);
        const Fr one = fr_from_u64(curve, 1);
        std::vector<Fr> rt(on_dev ? 0 : len), r2t(rt.size());
        DriverBase::Marks mk(me == 0 ? "degree_reduce_vec king" : "degree_reduce_vec party 1", me <= 1);
        DriverBase::DevTmp held(d);                                                    // released when the step ends, also when a callback fails
        void* tmp = held.get(len * 32);
        if (on_dev) {
            d.lincomb(local.c[0], 0, 1, len, {{local.c[0], 0, 1, one}, {top.r2t, top.off, -1, one}});   // input += r_2t
        } else {
            pairs.materialize();
            for (size_t k = 0; k < len; k++) { auto pr = get_pair(); rt[k] = pr.first; r2t[k] = pr.second; }
            CG(cg_dev_upload(d.ctx, tmp, r2t.data(), len * 32));
            CG(cg_vec_add_dev(d.ctx, curve.id, local.c[0], local.c[0], tmp, len));    // input += r_2t
        }
        Fr* const buf = stage(len);                                                    // page-locked staging of the messages to / from the king
        mk.mark("add r_2t");
        if (me == 0) {                                                                 // KING_ID: interpolate at 0 from parties 0..2t, re-share with degree t
            CG(cg_vec_affine_dev(d.ctx, curve.id, local.c[0], local.c[0], len, mul_lagrange_2t[0].v, nullptr));   // acc = input * lagrange_0
            for (int other = 1; other <= 2 * t; other++) {
                net->recv(other, buf, len * 32);
                CG(cg_dev_upload(d.ctx, tmp, buf, len * 32)); d.check_received_dev(tmp, len);
                CG(cg_vec_affine_dev(d.ctx, curve.id, tmp, tmp, len, mul_lagrange_2t[other].v, nullptr));
                CG(cg_vec_add_dev(d.ctx, curve.id, local.c[0], local.c[0], tmp, len));
            }
            mk.mark("recv+interpolate");
            // ShamirCore::share per element: coefficients are drawn element by element (t per element) — draw k * t + d is coefficient d of
            // element k, and the share kernel reads them in that layout: all np shares in one launch, the king's own in place
            void* d_all = nullptr;
            if (t) { d_all = held.get(len * (size_t)t * 32); rnd.draw_dev(d, len * (size_t)t, d_all); }
            std::vector<void*> outs(np);
            outs[0] = local.c[0];
            for (int to = 1; to < np; to++) outs[to] = held.get(len * 32);
            share_dev(local.c[0], d_all, 0, t, len, t, outs, 0, 1);
            for (int to = np - 1; to >= 1; to--) { CG(cg_dev_download(d.ctx, buf, outs[to], len * 32)); net->send(to, buf, len * 32); }
            mk.mark("reshare+send");
        } else {
            if (me <= 2 * t) { CG(cg_dev_download(d.ctx, buf, local.c[0], len * 32)); net->send(0, buf, len * 32); }   // only if my items are required
            mk.mark("download+send");
            net->recv(0, buf, len * 32);
            mk.mark("wait for king");
            CG(cg_dev_upload(d.ctx, local.c[0], buf, len * 32)); d.check_received_dev(local.c[0], len);
            mk.mark("upload");
        }
        if (on_dev) d.lincomb(tmp, 0, 1, len, {{top.rt, top.off, -1, one}});
        else CG(cg_dev_upload(d.ctx, tmp, rt.data(), len * 32));
        CG(cg_vec_sub_dev(d.ctx, curve.id, local.c[0], local.c[0], tmp, len));        // share - r_t
        mk.mark("sub r_t");
        return local;
    }
    Fr degree_reduce(Fr input) {                                                       // shamir.rs:252-300
        const int np = net->num_parties(), me = net->id();
        auto pr = get_pair();
        input = fr_add(curve, input, pr.second);
        Fr my_share;
        if (me == 0) {
            Fr acc = fr_mul(curve, input, mul_lagrange_2t[0]);
            for (int other = 1; other <= 2 * t; other++) { Fr r; net->recv(other, r.v, 32); d.check_received(r.v, 1); acc = fr_add(curve, acc, fr_mul(curve, r, mul_lagrange_2t[other])); }
            std::vector<Fr> coeffs; for (int k = 0; k < t; k++) coeffs.push_back(next_rand());
            auto shares = share(acc, coeffs.data(), t);
            for (int to = 0; to < np; to++) { if (to == me) my_share = shares[to]; else net->send(to, shares[to].v, 32); }
        } else {
            if (me <= 2 * t) net->send(0, input.v, 32);
            net->recv(0, my_share.v, 32); d.check_received(my_share.v, 1);
        }
        return fr_sub(curve, my_share, pr.first);
    }
    Point degree_reduce_point(Point input) {                                           // shamir.rs:386-436; C::rand stand-in: G * next_rand()
        const int np = net->num_parties(), me = net->id();
        const int g = input.group;
        auto pr = get_pair();
        input = pt_add(curve, input, pt_mul_generator(curve, g, pr.second));
        Point my_share = pt_inf(curve, g);
        const size_t psz = curve.aff(g);
        if (me == 0) {
            Point acc = pt_mul(curve, input, mul_lagrange_2t[0]);
            for (int other = 1; other <= 2 * t; other++) { Bytes a(psz); net->recv(other, a.data(), psz); acc = pt_add(curve, acc, pt_mul(curve, d.received_point(g, a.data()), mul_lagrange_2t[other])); }
            std::vector<Point> coeffs; for (int k = 0; k < t; k++) coeffs.push_back(pt_mul_generator(curve, g, next_rand()));
            for (int to = 0; to < np; to++) {
                Point sh = acc; const Fr x = fr_from_u64(curve, (uint64_t)to + 1); Fr xp = x;
                for (const Point& cf : coeffs) { sh = pt_add(curve, sh, pt_mul(curve, cf, xp)); xp = fr_mul(curve, xp, x); }
                if (to == me) my_share = sh; else { Bytes a = pt_to_affine(curve, sh); net->send(to, a.data(), a.size()); }
            }
        } else {
            if (me <= 2 * t) { Bytes a = pt_to_affine(curve, input); net->send(0, a.data(), a.size()); }
            Bytes a(psz); net->recv(0, a.data(), psz); my_share = d.received_point(g, a.data());
        }
        return pt_sub(curve, my_share, pt_mul_generator(curve, g, pr.first));
    }
    // rand x n (shamir.rs:570-573): the r_t halves of the top n pairs, top first.  All in the device block: one launch, no value crosses PCIe.  Otherwise they come back in `host` for the driver to upload
    ShareVec rand_vec(size_t n, std::vector<Fr>& host) {
        ShareVec v; PairStack::DevView top;
        if (n && pairs.pop_vec_dev(n, top)) {
            v.n = n; v.c[0] = d.dalloc(n * 32);
            d.lincomb(v.c[0], 0, 1, n, {{top.rt, top.off, -1, fr_from_u64(curve, 1)}});
            return v;
        }
        if (n > 1) pairs.materialize();                                                // (one download of the block instead of two 32-byte copies per pair)
        host.resize(n); for (size_t i = 0; i < n; i++) host[i] = get_pair().first;
        return v;
    }
    // `out` = this party's degree-2t products on the device, opened in place from 2t + 1 shares (shamir.rs:684-711): broadcast_next(2t) + reconstruction (shamir/network.rs:233-266) with the Lagrange
    // combination on the device, messages staged in page-locked memory; `staged`: what arrives is range-checked on the device behind its upload (verify_received_vectors), as mul_vec_finish does
    void mul_open_vec(void* out, size_t n, bool staged) {
        const int np = net->num_parties(), me = net->id(), num = (int)open_lagrange_2t.size();
        DriverBase::DevTmp got(d);
        Fr* const buf = stage(n);
        CG(cg_dev_download(d.ctx, buf, out, n * 32));
        for (int sft = 1; sft < num; sft++) net->send((me + sft) % np, buf, n * 32);
        std::vector<DriverBase::Term> terms{{out, 0, 1, open_lagrange_2t[0]}};
        for (int r = 1; r < num; r++) {
            net->recv((me + np - r) % np, buf, n * 32);
            if (!staged) d.check_received(buf, n);
            void* p = got.get(n * 32); CG(cg_dev_upload(d.ctx, p, buf, n * 32));
            if (staged) d.check_received_dev(p, n);
            terms.push_back({p, 0, 1, open_lagrange_2t[r]});
        }
        d.lincomb(out, 0, 1, n, terms);
    }
    // broadcast_next(t) of a vector + reconstruction (shamir/network.rs:233-266, shamir.rs:581-601)
    std::vector<Fr> open_vec(const std::vector<Fr>& mine) {
        const std::vector<Fr>& lagrange = open_lagrange_t; const int np = net->num_parties(), me = net->id(), num = (int)lagrange.size();
        const size_t n = mine.size();
        for (int sft = 1; sft < num; sft++) net->send((me + sft) % np, mine.data(), n * 32);
        std::vector<Fr> out(n), got(n);
        for (size_t i = 0; i < n; i++) out[i] = fr_mul(curve, mine[i], lagrange[0]);
        for (int r = 1; r < num; r++) { net->recv((me + np - r) % np, got.data(), n * 32); d.check_received(got.data(), n); for (size_t i = 0; i < n; i++) out[i] = fr_add(curve, out[i], fr_mul(curve, got[i], lagrange[r])); }
        return out;
    }
    // broadcast_next(t + 1) + reconstruct_point (network.rs:233-266, shamir.rs:778-782)
    Point open_point(const Point& mine) {
        const int np = net->num_parties(), me = net->id();
        Bytes a = pt_to_affine(curve, mine);
        for (int sft = 1; sft <= t; sft++) net->send((me + sft) % np, a.data(), a.size());
        Point res = pt_mul(curve, mine, open_lagrange_t[0]);
        for (int r = 1; r <= t; r++) { Bytes b(a.size()); net->recv((me + np - r) % np, b.data(), b.size()); res = pt_add(curve, res, pt_mul(curve, d.received_point(mine.group, b.data()), open_lagrange_t[r])); }
        return res;
    }
    // a G1 and a G2 point opened together, shamir.rs:808-824 (one message per point here): both points are sent first, the G2 point's own term (a 254-bit product, as
    // long as the whole G1 opening) runs on a helper under the G1 opening; the messages keep their order on every channel (G1 then G2)
    std::pair<Point, Point> open_two_points(const Point& a, const Point& b) {
        const int np = net->num_parties(), me = net->id();
        const Bytes m1 = pt_to_affine(curve, a), m2 = pt_to_affine(curve, b);
        for (int sft = 1; sft <= t; sft++) { net->send((me + sft) % np, m1.data(), m1.size()); net->send((me + sft) % np, m2.data(), m2.size()); }
        auto own2 = Helpers::get().run([&] { return pt_mul(curve, b, open_lagrange_t[0]); });
        struct Joined { std::future<Point>& f; ~Joined() { if (f.valid()) f.wait(); } } joined{own2};     // (the helper reads this frame)
        Point r1 = pt_mul(curve, a, open_lagrange_t[0]);
        std::vector<Point> theirs2;
        for (int r = 1; r <= t; r++) {
            Bytes b1(m1.size()), b2(m2.size());
            net->recv((me + np - r) % np, b1.data(), b1.size()); net->recv((me + np - r) % np, b2.data(), b2.size());
            theirs2.push_back(d.received_point(CG_G2, b2.data()));
            r1 = pt_add(curve, r1, pt_mul(curve, d.received_point(CG_G1, b1.data()), open_lagrange_t[r]));
        }
        Point r2 = own2.get();
        for (int r = 1; r <= t; r++) r2 = pt_add(curve, r2, pt_mul(curve, theirs2[(size_t)r - 1], open_lagrange_t[r]));
        return {r1, r2};
    }
};
}  // namespace cgh
