// ethcnn_ldp_sessions_plan.cpp -- the host-only entries of ethcnn_ldp_sessions_* (include/ethcnn.h): the layout of a step and the
// byte formula.  No HIP in this file (ethcnn_ldp_sessions_plan.h).
#include "ethcnn_ldp_sessions_plan.h"

#include <algorithm>

#include "ethcnn_spec.h"

using namespace ethcnn;

int ldp_sessions_layout(const int* nctus, int n, int max_ctus_per_pass, int* first_group, int64_t* total, int* pass_groups) {
    if (!nctus || n < 1 || n > kLdpSessionsMax || max_ctus_per_pass < 0) return ETHCNN_ERR_ARG;
    const int cap = max_ctus_per_pass ? std::min(max_ctus_per_pass, kMaxCtusPerPass) : kMaxCtusPerPass;
    if (cap < 16) return ETHCNN_ERR_ARG;
    int64_t g = 0;
    for (int j = 0; j < n; ++j)
        if (nctus[j] < 1) return ETHCNN_ERR_ARG;
    for (int j = 0; j < n; ++j) {
        if (first_group) first_group[j] = (int)g;
        g += ((int64_t)nctus[j] + 15) / 16;
    }
    if (g > INT32_MAX / 16) return ETHCNN_ERR_ARG;  // (32 pictures of 2^31 CTUs: the group numbers are ints)
    *total = g;
    *pass_groups = cap / 16;
    return 0;
}

extern "C" int64_t ethcnn_ldp_sessions_bytes(const int* widths, const int* heights, int n) {
    if (!widths || !heights || n < 1 || n > kLdpSessionsMax) return ETHCNN_ERR_ARG;
    int64_t bytes = 0;
    for (int j = 0; j < n; ++j) {
        if (widths[j] <= 0 || heights[j] <= 0) return ETHCNN_ERR_ARG;
        const int64_t nctu = (((int64_t)widths[j] + 63) / 64) * (((int64_t)heights[j] + 63) / 64);
        if (nctu > INT32_MAX / 16) return ETHCNN_ERR_ARG;  // (what ethcnn_ldp_sessions_open refuses; 32 such pictures stay far inside int64)
        bytes += (nctu + 15) / 16 * 16 * (kNVec + 2 * kNVec) * 4;  // a vector and a (c, h) state per row of whole groups
    }
    return bytes;
}

extern "C" int ethcnn_ldp_sessions_plan(const int* nctus, int n, int max_ctus_per_pass, int* first_group_out, int* npasses_out, int* pass_groups_out,
                                        int max_passes) {
    if (max_passes < 0 || (max_passes && !pass_groups_out)) return ETHCNN_ERR_ARG;
    int gpp = 0;
    int64_t groups = 0;
    if (ldp_sessions_layout(nctus, n, max_ctus_per_pass, first_group_out, &groups, &gpp)) return ETHCNN_ERR_ARG;
    const int64_t npasses = (groups + gpp - 1) / gpp;
    if (npasses_out) *npasses_out = (int)npasses;
    for (int64_t p = 0; p < npasses && p < max_passes; ++p) pass_groups_out[p] = (int)std::min<int64_t>(gpp, groups - p * gpp);
    return ETHCNN_OK;
}
