// C entry points: .r1cs handles, the witness check, the Groth16 and Plonk development setups (include/cogroth16_host.h)
#include "plonk_setup.hpp"
#include "plonk_audit.hpp"
#include "capi_common.hpp"

extern "C" {

int32_t cgh_r1cs_open(int32_t curve, const char* path, void** out_r1cs) {
    try {
        if (!path || !out_r1cs) throw std::runtime_error("cgh_r1cs_open: null argument");
        *out_r1cs = nullptr;
        auto h = std::make_unique<cgh::R1csHandle>();
        h->r = cgh::read_r1cs(curve, path);
        *out_r1cs = h.release();
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
// info: n_wires, n_public, n_constraints, domain_size, nnz(A), nnz(B), nnz(C)
int32_t cgh_r1cs_info(void* r1cs, size_t* info) {
    if (!r1cs || !info) { g_host_err = "cgh_r1cs_info: null argument"; return 1; }
    const cgh::R1cs& r = ((cgh::R1csHandle*)r1cs)->r;
    info[0] = r.n_wires; info[1] = r.n_public; info[2] = r.n_constraints; info[3] = r.domain_size;
    for (int m = 0; m < 3; m++) info[4 + m] = r.col[m].size();
    return 0;
}
int32_t cgh_r1cs_close(void* r1cs) { delete (cgh::R1csHandle*)r1cs; return 0; }
int32_t cgh_r1cs_coeff_section(void* r1cs, uint8_t* out, size_t cap, size_t* n_bytes) {
    try {
        if (!r1cs || !n_bytes) throw std::runtime_error("cgh_r1cs_coeff_section: null argument");
        const cgh::R1cs& r = ((cgh::R1csHandle*)r1cs)->r;
        *n_bytes = 4 + (r.col[0].size() + r.col[1].size() + r.n_public + 1) * 44;
        if (!out) return 0;
        if (cap < *n_bytes) throw std::runtime_error("cgh_r1cs_coeff_section: buffer too small");
        const cgh::Bytes b = cgh::r1cs_coeff_section(r);
        memcpy(out, b.data(), b.size());
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_r1cs_check_witness_form(int32_t device, void* r1cs, int32_t form, const uint64_t* full_witness, uint64_t* n_bad, uint64_t* first_bad) {
    try {
        if (!r1cs || !full_witness || !n_bad || !first_bad) throw std::runtime_error("cgh_r1cs_check_witness: null argument");
        cgh::r1cs_check_witness(*(cgh::R1csHandle*)r1cs, device, form, (const cgh::Fr*)full_witness, n_bad, first_bad);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_r1cs_check_witness(int32_t device, void* r1cs, const uint64_t* full_witness, uint64_t* n_bad, uint64_t* first_bad) {
    return cgh_r1cs_check_witness_form(device, r1cs, 0, full_witness, n_bad, first_bad);
}
int32_t cgh_setup_groth16_dev(int32_t device, void* r1cs, uint64_t seed, const char* zkey_path) {
    try {
        if (!r1cs || !zkey_path) throw std::runtime_error("cgh_setup_groth16_dev: null argument");
        cgh::setup_groth16_dev(device, ((cgh::R1csHandle*)r1cs)->r, seed, zkey_path);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_setup_toxic(int32_t curve, uint64_t seed, uint64_t* out5) {
    try {
        if (!out5) throw std::runtime_error("cgh_setup_toxic: null argument");
        if (curve != CG_BN254 && curve != CG_BLS12_381) throw std::runtime_error("cgh_setup_toxic: unknown curve");
        cgh::Fr t[5]; cgh::setup_toxic(cgh::Curve{curve}, seed, t);
        memcpy(out5, t, sizeof t);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_r1cs_plonk_info(int32_t device, void* r1cs, size_t* out4) {
    try {
        if (!r1cs || !out4) throw std::runtime_error("cgh_r1cs_plonk_info: null argument");
        const cgh::PlonkPlan p = cgh::r1cs_plonk_info(*(cgh::R1csHandle*)r1cs, device);
        out4[0] = p.n_additions; out4[1] = p.n_constraints; out4[2] = p.n_vars; out4[3] = p.n;
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_r1cs_plonk_gate_origin(int32_t device, void* r1cs, uint64_t gate_row, uint64_t* out3) {
    try {
        if (!r1cs || !out3) throw std::runtime_error("cgh_r1cs_plonk_gate_origin: null argument");
        cgh::r1cs_plonk_gate_origin(*(cgh::R1csHandle*)r1cs, device, gate_row, out3);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_setup_plonk_dev(int32_t device, void* r1cs, uint64_t seed, const char* zkey_path) {
    try {
        if (!r1cs || !zkey_path) throw std::runtime_error("cgh_setup_plonk_dev: null argument");
        cgh::setup_plonk_dev(*(cgh::R1csHandle*)r1cs, device, seed, zkey_path);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}
int32_t cgh_setup_plonk_tau_dev(int32_t device, void* r1cs, const uint64_t* tau, const char* zkey_path, double* stage_seconds) {
    try {
        if (!r1cs || !tau || !zkey_path) throw std::runtime_error("cgh_setup_plonk_tau_dev: null argument");
        cgh::Fr t; memcpy(t.v, tau, 32);
        int32_t canonical = 0;
        if (cg_fr_is_canonical(((cgh::R1csHandle*)r1cs)->r.curve.id, t.v, 1, &canonical) || !canonical) throw std::runtime_error("cgh_setup_plonk_tau_dev: tau is not below the modulus");
        cgh::setup_plonk_tau_dev(*(cgh::R1csHandle*)r1cs, device, t, zkey_path, stage_seconds);
        return 0;
    } catch (const std::exception& e) { g_host_err = e.what(); return 1; }
}

}  // extern "C"
