// ethcnn_train_host.h -- the trainer object, shared between the solo trainer's host side (ethcnn_train.cpp) and the trainer group
// (ethcnn_train_group.cpp), whose members are trainers of this kind.
#pragma once
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_train.h"

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
    ethcnn::train::GemmGroup *g_fwd = nullptr, *g_bwd = nullptr, *g_eval = nullptr;  // device tables
    int t_fwd = 0, t_bwd = 0, t_eval = 0;
    uint8_t* data[2] = {nullptr, nullptr};
    int64_t nrec[2] = {0, 0};
    int qps[52] = {0};
    int nqps = 0;
    int net = ethcnn::train::kNetAi, tune = 0;  // ethcnn_train_options.net / .tune
    ethcnn::train::TuneMask mask{};             // the tensors tune 1..3 optimises (n == 0: all)
    int slot_of_qp[2][52];       // LDP, per set: the slot of each of its four QPs, -1 elsewhere
    int slot_qps[2][4] = {{0}};
    std::vector<void*> allocs;
};

// the descriptor groups of m rows and the learning rate of a step (ethcnn_train.cpp)
ethcnn::train::GemmGroup train_fc1_group(const ethcnn_trainer* t, int m);
ethcnn::train::GemmGroup train_bwd_group(const ethcnn_trainer* t, int m);
float train_lr_at(const ethcnn_trainer* t, int64_t step);
