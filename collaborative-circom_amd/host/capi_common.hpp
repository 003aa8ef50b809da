// shared by the C entry-point translation units: the thread-local error text and the per-party error report
#pragma once
#include <string>
extern thread_local std::string g_host_err;   // defined in capi_tools.cpp
// what the Shamir party entries refuse before a session, a file or a device is looked at (`who`: the entry's name, in front of its messages)
static void shamir_party_args(const char* who, int32_t threshold, const cgh_shamir_net* net, const cgh_shamir_rand* rnd, const uint8_t* seed32, const void* pub_in, const void* wit, const void* out) {
    const std::string w(who);
    if (!pub_in || !wit || !net || (!rnd && !seed32) || !out) throw std::runtime_error(w + ": null argument");
    if (rnd && !rnd->random_field_elements) throw std::runtime_error("cgh_shamir_rand: random_field_elements is required");
    if (net->num_parties < 3) throw std::runtime_error(w + ": Shamir protocol requires at least 3 parties");
    if (threshold < 0 || 2 * (int64_t)threshold + 1 > net->num_parties) throw std::runtime_error(w + ": Threshold too large for number of parties");
}
// first real failure among the parties (the others only report that somebody else died)
template <class Errs> static bool report_party_errors(const Errs& errs, int n) {
    int pick = -1;
    for (int i = 0; i < n; i++) if (!errs[i].empty() && (pick < 0 || (errs[pick] == "another party failed" && errs[i] != "another party failed"))) pick = i;
    if (pick < 0) return false;
    g_host_err = "party " + std::to_string(pick) + ": " + errs[pick];
    return true;
}
