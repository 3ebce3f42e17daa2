// ethcnn_ldp_sessions_plan.h -- internal: the layout of one ethcnn_ldp_sessions step (include/ethcnn.h, ethcnn_ldp_sessions_plan).
// Host only, no HIP: ethcnn_ldp_sessions_plan.cpp is also compiled into a stand-alone program (tools/ldp_sessions_plan_check.cpp).
#pragma once
#include <cstdint>

constexpr int kLdpSessionsMax = 32;  // sessions open at once = frames of a call = rows of the recurrence launch

// first_group[j] (may be null) for n pictures of nctus[j] CTUs, *total: all their 16-CTU groups, *pass_groups: the groups of a full
// pass under max_ctus_per_pass (0: the default cap).  0, or ETHCNN_ERR_ARG.
int ldp_sessions_layout(const int* nctus, int n, int max_ctus_per_pass, int* first_group, int64_t* total, int* pass_groups);
