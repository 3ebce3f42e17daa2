// ethcnn_ldp_group.h -- internal: the object behind ethcnn_ldp_group_* (include/ethcnn.h "config #5 offline, group form").
// K sequences of one geometry go through the offline Low-Delay-P chain together: the front-end per member (seq_front into the member's
// slice of the vector buffer), then ONE recurrence launch per run of frames and ONE gate launch per chunk for all members
// (seq_recur in ethcnn_ctx.h, ethcnn_lstm_seq.h).  The context's own bundle, resident state and sequence buffers are neither used nor changed.
#pragma once
#include <string>
#include <vector>

#include "ethcnn_lstm_seq.h"

struct ethcnn_ctx;
struct ethcnn_ldp_group {
    ethcnn_ctx* c = nullptr;
    int k = 0;
    int chunk = 0;  // frames per chunk, 0 = default (256 MB of vectors for the whole group)
    std::string err;
    struct Member {
        bool have = false;        // a bundle is loaded
        std::vector<float> blob;  // its payload as stored
        float* d_lstm = nullptr;  // payload + packed kernels in HBM (upload_lstm_image), held from load time
        int state_nctu = -1;      // CTU count of the resident (c, h) state; -1: none
    } m[ethcnn::kLstmSeqGroupMax];
    float* d_vec = nullptr;    // [k][F][nctu][448]: member m's slice starts at m * F * nctu * 448 (F: the chunk of the call)
    size_t vec_cap = 0;        // bytes
    float* d_state = nullptr;  // [k][state_cap][2][448]: one resident state per member, advanced in place
    int state_cap = 0;         // CTUs per member, a multiple of 16
};
