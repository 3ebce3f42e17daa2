// ethcnn_ldp_batch.h -- internal: the object behind ethcnn_ldp_batch_* (include/ethcnn.h "config #5 offline, batch form").
// Up to 32 sequences of different geometry, length and first frame number go through the offline Low-Delay-P chain together: the
// front-end per sequence (seq_front into the sequence's slice of the vector buffer), then ONE recurrence launch and ONE gate launch
// per chunk for all sequences that still have frames (ethcnn_lstm_seq.h, batch form).  Bundles are held apart from the sequences:
// several sequences of one QP band name the same image.  The context's own bundle, resident state and sequence buffers are neither
// used nor changed.
#pragma once
#include <string>
#include <vector>

#include "ethcnn_lstm_seq.h"

constexpr int kLdpBatchBundles = 8;

struct ethcnn_ctx;
struct ethcnn_ldp_batch {
    ethcnn_ctx* c = nullptr;
    int nb = 0;     // bundles
    int chunk = 0;  // frames per chunk, 0 = default (256 MB of vectors for all sequences of the call)
    std::string err;
    struct Bundle {
        bool have = false;
        std::vector<float> blob;  // the payload as stored
        float* d_lstm = nullptr;  // payload + packed kernels in HBM (upload_lstm_image), held from load time
    } b[kLdpBatchBundles];
    struct Seq {
        float* d_state = nullptr;  // the resident (c, h) state of this sequence index, [cap][2][448], advanced in place
        int cap = 0;               // CTUs, a multiple of 16
        int state_nctu = -1;       // CTU count of the resident state; -1: none
    } s[ethcnn::kLstmSeqBatchMax];
    float* d_vec = nullptr;  // the chunk's vectors, sequence after sequence: [min(nframes_j, Fc)][nctu_j][448]
    size_t vec_cap = 0;      // bytes
};
