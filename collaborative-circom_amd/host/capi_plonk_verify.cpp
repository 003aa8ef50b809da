// C entry points: Plonk verification (verifying-key handles, single proofs on the host, batches on the GPU)
#include "plonk_verify.hpp"
#include "capi_common.hpp"

extern "C" {

int32_t cgh_plonk_vk_from_json(int32_t curve, const char* path, void** out_vk) {
    try {
        if (!path || !out_vk) throw std::runtime_error("cgh_plonk_vk_from_json: null argument");
        *out_vk = new cgh::PlonkVerifyingKey(cgh::plonk_vk_from_json(curve, path)); return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_plonk_vk_from_zkey(int32_t curve, const char* path, void** out_vk) {
    try {
        if (!path || !out_vk) throw std::runtime_error("cgh_plonk_vk_from_zkey: null argument");
        *out_vk = new cgh::PlonkVerifyingKey(cgh::plonk_vk_from_zkey_data(cgh::read_plonk_zkey(curve, path))); return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_plonk_vk_info(void* vk, size_t* info) {
    if (!vk || !info) { g_host_err = "cgh_plonk_vk_info: null argument"; return 1; }
    const auto* k = (const cgh::PlonkVerifyingKey*)vk;
    info[0] = (size_t)k->c.id; info[1] = k->n_public; info[2] = k->power; return 0;
}
int32_t cgh_plonk_vk_fields(void* vk, uint64_t* out) {
    if (!vk || !out) { g_host_err = "cgh_plonk_vk_fields: null argument"; return 1; }
    const auto* k = (const cgh::PlonkVerifyingKey*)vk;
    uint8_t* p = (uint8_t*)out;
    memcpy(p, k->pts.data(), k->pts.size()); p += k->pts.size();
    memcpy(p, k->x2.data(), k->x2.size()); p += k->x2.size();
    memcpy(p, k->k1.v, 32); memcpy(p + 32, k->k2.v, 32); memcpy(p + 64, k->omega.v, 32); return 0;
}
int32_t cgh_plonk_vk_free(void* vk) { delete (cgh::PlonkVerifyingKey*)vk; return 0; }

int32_t cgh_plonk_verify(void* vk, const uint64_t* commits, const uint64_t* evals, const uint64_t* pub, size_t n_pub, int32_t* ok) {
    try {
        if (!vk || !commits || !evals || (n_pub && !pub) || !ok) throw std::runtime_error("cgh_plonk_verify: null argument");
        *ok = cgh::plonk_verify(*(const cgh::PlonkVerifyingKey*)vk, (const uint8_t*)commits, evals, pub, n_pub) ? 1 : 0; return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_plonk_verify_batch_timed(int32_t device, void* vk, const uint64_t* commits, const uint64_t* evals, const uint64_t* pubs, size_t n_pub, size_t n_proofs,
                                     const uint8_t* seed32, int32_t* ok, uint8_t* per_proof, double* seconds) {
    try {
        if (!vk || !ok || (n_proofs && (!commits || !evals || (n_pub && !pubs)))) throw std::runtime_error("cgh_plonk_verify_batch: null argument");
        *ok = cgh::plonk_verify_batch(device, *(const cgh::PlonkVerifyingKey*)vk, (const uint8_t*)commits, evals, pubs, n_pub, n_proofs, seed32, per_proof, seconds) ? 1 : 0; return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_plonk_verify_batch(int32_t device, void* vk, const uint64_t* commits, const uint64_t* evals, const uint64_t* pubs, size_t n_pub, size_t n_proofs,
                               const uint8_t* seed32, int32_t* ok, uint8_t* per_proof) {
    return cgh_plonk_verify_batch_timed(device, vk, commits, evals, pubs, n_pub, n_proofs, seed32, ok, per_proof, nullptr);
}

}  // extern "C"
