// C entry points: Groth16 verification (verifying-key handles, single proofs on the host, batches on the GPU)
#include "verify.hpp"
#include "capi_common.hpp"

extern "C" {

int32_t cgh_vk_from_json(int32_t curve, const char* path, void** out_vk) {
    try {
        if (!path || !out_vk) throw std::runtime_error("cgh_vk_from_json: null argument");
        *out_vk = new cgh::VerifyingKey(cgh::vk_from_json(curve, path)); return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_vk_from_zkey(int32_t curve, const char* path, void** out_vk) {
    try {
        if (!path || !out_vk) throw std::runtime_error("cgh_vk_from_zkey: null argument");
        *out_vk = new cgh::VerifyingKey(cgh::vk_from_zkey_data(cgh::read_zkey(curve, path, true))); return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_vk_info(void* vk, size_t* info) {
    if (!vk || !info) { g_host_err = "cgh_vk_info: null argument"; return 1; }
    const auto* k = (const cgh::VerifyingKey*)vk;
    info[0] = (size_t)k->c.id; info[1] = k->n_ic - 1; return 0;
}
int32_t cgh_vk_alphabeta(void* vk, uint64_t* out_fp12) {
    if (!vk || !out_fp12) { g_host_err = "cgh_vk_alphabeta: null argument"; return 1; }
    const auto* k = (const cgh::VerifyingKey*)vk;
    memcpy(out_fp12, k->alphabeta.data(), k->alphabeta.size()); return 0;
}
int32_t cgh_vk_free(void* vk) { delete (cgh::VerifyingKey*)vk; return 0; }

int32_t cgh_groth16_verify(void* vk, const uint64_t* proof, const uint64_t* pub, size_t n_pub, int32_t* ok) {
    try {
        if (!vk || !proof || (n_pub && !pub) || !ok) throw std::runtime_error("cgh_groth16_verify: null argument");
        *ok = cgh::groth16_verify(*(const cgh::VerifyingKey*)vk, (const uint8_t*)proof, pub, n_pub) ? 1 : 0; return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_groth16_verify_batch_timed(int32_t device, void* vk, const uint64_t* proofs, const uint64_t* pubs, size_t n_pub, size_t n_proofs, const uint8_t* seed32,
                                       int32_t* ok, uint8_t* per_proof, double* seconds) {
    try {
        if (!vk || !ok || (n_proofs && (!proofs || (n_pub && !pubs)))) throw std::runtime_error("cgh_groth16_verify_batch: null argument");
        *ok = cgh::groth16_verify_batch(device, *(const cgh::VerifyingKey*)vk, (const uint8_t*)proofs, pubs, n_pub, n_proofs, seed32, per_proof, seconds) ? 1 : 0; return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_groth16_verify_batch(int32_t device, void* vk, const uint64_t* proofs, const uint64_t* pubs, size_t n_pub, size_t n_proofs, const uint8_t* seed32,
                                 int32_t* ok, uint8_t* per_proof) {
    return cgh_groth16_verify_batch_timed(device, vk, proofs, pubs, n_pub, n_proofs, seed32, ok, per_proof, nullptr);
}

}  // extern "C"
