// ethcnn_lstm_train_host.h -- the ETH-LSTM trainer object, shared between the solo trainer's host side (ethcnn_lstm_train.cpp) and the
// LSTM trainer group (ethcnn_lstm_train_group.cpp), whose members are trainers of this kind.
#pragma once
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_lstm_train.h"

struct ethcnn_lstm_trainer {
    ethcnn_ctx* c = nullptr;
    ethcnn_lstm_train_options opt{};
    int B = 0, cap = 0;  // batch; samples the per-row buffers hold (>= the evaluation chunk)
    float qp_scale = 1.f;
    ethcnn::lstm_train::LstmOffsets o{};
    std::string err;
    float *W = nullptr, *acc = nullptr, *grad = nullptr, *stats = nullptr;
    double* part = nullptr;
    int32_t *idx = nullptr, *idx_in = nullptr;
    ethcnn::lstm_train::LstmBufs u{};
    ethcnn::train::GemmGroup *g_fwd = nullptr, *g_bwd = nullptr, *g_eval = nullptr;
    int t_fwd = 0, t_bwd = 0, t_eval = 0;
    uint8_t* data[2] = {nullptr, nullptr};
    int64_t nrec[2] = {0, 0};
    int qps[52] = {0};
    int nqps = 0;        // 0: every sample is kept
    int last_rows = 0;   // rows of the last step / the last evaluation piece (debug buffers)
    std::vector<void*> allocs;
};

// the descriptor groups of `rows` rows and the learning rate of a step (ethcnn_lstm_train.cpp)
ethcnn::train::GemmGroup lstm_proj_group(const ethcnn_lstm_trainer* t, int rows);
ethcnn::train::GemmGroup lstm_grad_group(const ethcnn_lstm_trainer* t, int rows);
float lstm_lr_at(const ethcnn_lstm_trainer* t, int64_t step);
