// ethcnn_train_host.h -- the two host objects of ETH-CNN training.  A trainer (ethcnn_train.cpp) is one model's state: options,
// weights, workspaces, QP list.  The engine (ethcnn_train_group.cpp) is everything that enqueues a step, for K >= 1 trainers at
// once: a trainer group IS an engine over its K members, a solo trainer holds an engine over itself with K = 1.
#pragma once
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_train.h"
#include "ethcnn_train_util.h"

struct ethcnn_trainer {
    ethcnn_ctx* c = nullptr;
    ethcnn_train_options opt{};
    int B = 0, cap = 0;  // batch; rows of every per-sample buffer (>= the evaluation chunk)
    ethcnn::train::NetOffsets o{};
    std::string err;
    // weights, accumulators, gradient (blob layout)
    float *W = nullptr, *acc = nullptr, *grad = nullptr;
    // per-sample buffers, cap rows
    int32_t *idx = nullptr, *qp = nullptr, *idx_in = nullptr, *qp_in = nullptr;
    float *lab = nullptr, *trunk = nullptr, *F = nullptr, *Z1 = nullptr, *A1 = nullptr, *M1 = nullptr, *H1 = nullptr, *A2 = nullptr,
          *M2 = nullptr, *H2 = nullptr, *P = nullptr, *dZ3 = nullptr, *dZ2 = nullptr, *dZ1 = nullptr, *dF = nullptr, *part = nullptr,
          *stats = nullptr;
    int qps[52] = {0};
    int nqps = 0;
    int net = ethcnn::train::kNetAi, tune = 0;  // ethcnn_train_options.net / .tune
    ethcnn::train::TuneMask mask{};             // the tensors tune 1..3 optimises (n == 0: all)
    ethcnn_train_group* eng = nullptr;          // the engine that steps this trainer: its group, or (solo) one of its own
    bool solo = false;                          // eng is this trainer's to destroy
    std::vector<void*> allocs;
};

struct ethcnn_train_group {
    ethcnn_ctx* c = nullptr;
    int K = 0, B = 0, cap = 0, net = ethcnn::train::kNetAi, tune = 0;
    bool group = true;  // false: the engine of a solo trainer (messages name no member and speak of ethcnn_train_*)
    std::vector<ethcnn_trainer*> m;
    ethcnn::train::Member* d_tab = nullptr;  // the member table of a training step
    bool stale = true;                       // a QP list changed since the table was uploaded
    ethcnn::train::GemmGroup *d_fwd = nullptr, *d_bwd = nullptr, *d_eval = nullptr;  // [K] each, side by side
    int t_fwd = 0, t_bwd = 0, t_eval = 0;                                            // tiles of ONE member
    // the two sample sets, owned once
    uint8_t* data[2] = {nullptr, nullptr};
    int64_t nrec[2] = {0, 0};
    int slot_of_qp[2][52];  // LDP, per set: the slot of each of its four QPs, -1 elsewhere
    int slot_qps[2][4] = {{0}};
    std::string err;
};

// a trainer without an engine, and its end (ethcnn_train.cpp); on failure the context holds the message
int train_member_create(ethcnn_ctx* c, const ethcnn_train_options* opt, ethcnn_trainer** out);
void train_member_destroy(ethcnn_trainer* t);
// the descriptor groups of m rows (ethcnn_train.cpp)
ethcnn::train::GemmGroup train_fc1_group(const ethcnn_trainer* t, int m);
ethcnn::train::GemmGroup train_bwd_group(const ethcnn_trainer* t, int m);
// an engine over `members` (all created by train_member_create on c, alike in net, batch and tuning mode), and its end, which leaves
// the members alone (ethcnn_train_group.cpp); on failure the context holds the message
int train_engine_create(ethcnn_ctx* c, const std::vector<ethcnn_trainer*>& members, bool group, ethcnn_train_group** out);
void train_engine_destroy(ethcnn_train_group* g);
