// ethcnn_lstm_train_host.h -- the two host objects of ETH-LSTM training.  A trainer (ethcnn_lstm_train.cpp) is one model's state:
// options, weights, workspaces, QP list.  The engine (ethcnn_lstm_train_group.cpp) is everything that enqueues a step and the sample
// sets, for K >= 1 trainers at once: a trainer group IS an engine over its K members, a solo trainer holds an engine over itself
// with K = 1.
#pragma once
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_lstm_train.h"
#include "ethcnn_train_util.h"

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
    int qps[52] = {0};
    int nqps = 0;        // 0: every sample is kept
    int last_rows = 0;   // rows of the last step / the last evaluation piece (debug buffers)
    ethcnn_lstm_train_group* eng = nullptr;  // the engine that steps this trainer: its group, or (solo) one of its own
    bool solo = false;                       // eng is this trainer's to destroy
    std::vector<void*> allocs;
};

struct ethcnn_lstm_train_group {
    ethcnn_ctx* c = nullptr;
    int K = 0, B = 0, cap = 0;
    bool group = true;  // false: the engine of a solo trainer (messages name no member and speak of ethcnn_lstm_train_*; an adopted
                        // sample set is compacted to the records the trainer keeps)
    std::vector<ethcnn_lstm_trainer*> m;
    ethcnn::lstm_train::LstmMember* d_tab = nullptr;  // the tables of a training step
    ethcnn::train::Member* d_loss = nullptr;          // k_group_loss reads P, lab, stats and dZ3 of its table; the rest stays zero
    bool stale = true;                                // a set changed since the tables were uploaded
    ethcnn::train::GemmGroup *d_fwd = nullptr, *d_bwd = nullptr, *d_eval = nullptr;  // [K] each, side by side
    int t_fwd = 0, t_bwd = 0, t_eval = 0;                                            // tiles of ONE member
    uint8_t* data[2] = {nullptr, nullptr};  // the shared records of a set
    int64_t nall[2] = {0, 0};
    int64_t* d_keep[2][ethcnn::train::kMaxMembers] = {};  // a member's kept records, in file order; NULL: all nall of them
    int64_t nkept[2][ethcnn::train::kMaxMembers] = {};
    std::string err;
};

// a trainer without an engine, and its end (ethcnn_lstm_train.cpp); on failure the context holds the message
int lstm_member_create(ethcnn_ctx* c, const ethcnn_lstm_train_options* opt, ethcnn_lstm_trainer** out);
void lstm_member_destroy(ethcnn_lstm_trainer* t);
// the descriptor groups of `rows` rows (ethcnn_lstm_train.cpp)
ethcnn::train::GemmGroup lstm_proj_group(const ethcnn_lstm_trainer* t, int rows);
ethcnn::train::GemmGroup lstm_grad_group(const ethcnn_lstm_trainer* t, int rows);
// an engine over `members` (all created by lstm_member_create on c with one batch size), and its end, which leaves the members alone
// (ethcnn_lstm_train_group.cpp); on failure the context holds the message
int lstm_engine_create(ethcnn_ctx* c, const std::vector<ethcnn_lstm_trainer*>& members, bool group, ethcnn_lstm_train_group** out);
void lstm_engine_destroy(ethcnn_lstm_train_group* g);
