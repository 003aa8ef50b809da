// Sanitizer run (AddressSanitizer + UndefinedBehaviorSanitizer) of the host pairing and the host verifier, outside Python: the host side of
// csrc/capi_pairing.hip (csrc/pairing.hpp compiled for the host) and host/capi_verify.cpp are compiled INTO this binary with
// -fsanitize=address,undefined (tests/sanitize/pairing.mk); everything else comes from the release library.  No GPU is touched.
//   usage: pairing_main <golden dir>
// Per curve, on the poseidon fixture: the key opens from the JSON file and from the zkey with the same e(alpha, beta), the shipped proof
// verifies, a proof with A and C exchanged and one with a point off the curve do not, a wrong public-input count is an error,
// e(P, Q) e(-P, Q) == 1, and a Miller loop followed by the final exponentiation is the pairing.
// Exit code 0 = every check passed and no sanitizer report (a report aborts the process).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "cogroth16_hip.h"
#include "cogroth16_host.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s\n", what); failures++; } else printf("ok: %s\n", what); } while (0)

static std::string slurp(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: pairing_main <golden dir>\n"); return 2; }
    const std::string golden = argv[1];
    for (int curve = 0; curve < 2; curve++) {
        const std::string dir = golden + "/groth16/" + (curve == 0 ? "bn254" : "bls12_381") + "/poseidon/";
        const size_t fq = curve == 0 ? 4 : 6;                       // u64 words per base-field element
        void *vk = nullptr, *vz = nullptr;
        EXPECT(cgh_vk_from_json(curve, (dir + "verification_key.json").c_str(), &vk) == 0, "verifying key from JSON");
        EXPECT(cgh_vk_from_zkey(curve, (dir + "circuit.zkey").c_str(), &vz) == 0, "verifying key from the zkey");
        if (!vk || !vz) { printf("%s\n", cgh_last_error()); return 1; }
        std::vector<uint64_t> ab(12 * fq), ab2(12 * fq);
        EXPECT(cgh_vk_alphabeta(vk, ab.data()) == 0 && cgh_vk_alphabeta(vz, ab2.data()) == 0 && ab == ab2, "e(alpha, beta) agrees between the two sources");
        size_t info[2] = {0, 0};
        EXPECT(cgh_vk_info(vk, info) == 0 && info[0] == (size_t)curve, "key info");
        std::vector<uint64_t> proof(8 * fq);
        EXPECT(cgh_proof_from_json(curve, slurp(dir + "circom.proof").c_str(), proof.data()) == 0, "proof from JSON");
        // public.json: a list of decimal strings; parsed through the proof codec's number reader by way of cg_fr_from_canonical
        std::vector<uint64_t> pub;
        {
            const std::string js = slurp(dir + "public.json");
            for (size_t pos = js.find('"'); pos != std::string::npos; pos = js.find('"', pos + 1)) {
                const size_t end = js.find('"', pos + 1);
                uint64_t can[4] = {0, 0, 0, 0};
                for (size_t i = pos + 1; i < end; i++) {        // decimal -> four little-endian words
                    unsigned __int128 carry = (unsigned)(js[i] - '0');
                    for (int l = 0; l < 4; l++) { const unsigned __int128 t = (unsigned __int128)can[l] * 10 + carry; can[l] = (uint64_t)t; carry = t >> 64; }
                }
                uint64_t mont[4];
                EXPECT(cg_fr_from_canonical(curve, can, mont, 1) == 0, "public input to Montgomery form");
                pub.insert(pub.end(), mont, mont + 4);
                pos = end;
            }
        }
        EXPECT(pub.size() == 4 * info[1], "as many public inputs as the key expects");
        int32_t ok = -1;
        EXPECT(cgh_groth16_verify(vk, proof.data(), pub.data(), pub.size() / 4, &ok) == 0 && ok == 1, "the shipped proof verifies");
        EXPECT(cgh_groth16_verify(vz, proof.data(), pub.data(), pub.size() / 4, &ok) == 0 && ok == 1, "the shipped proof verifies under the zkey's key");
        std::vector<uint64_t> swapped(proof);
        memcpy(swapped.data(), proof.data() + 6 * fq, 2 * fq * 8); memcpy(swapped.data() + 6 * fq, proof.data(), 2 * fq * 8);
        EXPECT(cgh_groth16_verify(vk, swapped.data(), pub.data(), pub.size() / 4, &ok) == 0 && ok == 0, "A and C exchanged: rejected");
        std::vector<uint64_t> off(proof); off[fq] ^= 1;             // y of A, one bit
        EXPECT(cgh_groth16_verify(vk, off.data(), pub.data(), pub.size() / 4, &ok) == 0 && ok == 0, "a point off the curve: rejected");
        EXPECT(cgh_groth16_verify(vk, proof.data(), pub.data(), pub.size() / 4 + 1, &ok) != 0, "a wrong public-input count is an error");
        // the pairing itself on the proof's A and B
        std::vector<uint64_t> e(12 * fq), m(12 * fq), e2(12 * fq);
        EXPECT(cg_pairing(curve, proof.data(), proof.data() + 2 * fq, e.data()) == 0, "cg_pairing");
        EXPECT(cg_miller_loop(curve, proof.data(), proof.data() + 2 * fq, 1, m.data()) == 0 && cg_final_exp(curve, m.data(), e2.data()) == 0 && e == e2, "Miller loop + final exponentiation = pairing");
        std::vector<uint64_t> jac(3 * fq), neg(3 * fq), g1s(4 * fq), g2s(8 * fq);
        EXPECT(cg_point_from_affine(curve, CG_G1, proof.data(), jac.data()) == 0 && cg_point_neg(curve, CG_G1, jac.data(), neg.data()) == 0, "negate A");
        memcpy(g1s.data(), proof.data(), 2 * fq * 8);
        EXPECT(cg_point_to_affine(curve, CG_G1, neg.data(), g1s.data() + 2 * fq) == 0, "-A affine");
        memcpy(g2s.data(), proof.data() + 2 * fq, 4 * fq * 8); memcpy(g2s.data() + 4 * fq, proof.data() + 2 * fq, 4 * fq * 8);
        EXPECT(cg_pairing_check(curve, g1s.data(), g2s.data(), 2, &ok) == 0 && ok == 1, "e(A, B) e(-A, B) == 1");
        EXPECT(cg_pairing_check(curve, g1s.data(), g2s.data(), 1, &ok) == 0 && ok == 0, "e(A, B) != 1");
        cgh_vk_free(vk); cgh_vk_free(vz);
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
