// ethcnn_risk.cpp -- host side of the expected wrong decisions (include/ethcnn.h "partition-search simulation: expected wrong
// decisions"): the simulator's reliability table, the evaluation around k_sim_risk and the ladder build around k_ladder_step_risk
// (ethcnn_risk.hip), and the host-only tables: identity, the monotone fit to a calibrator's histogram, and the table file.
#include "ethcnn_ctx.h"
#include "ethcnn_ladder_walk.h"
#include "ethcnn_risk.h"

using ethcnn::risk::kBins;
using ethcnn::risk::kOne;
using ethcnn::risk::kRelWords;

namespace {
constexpr int64_t kMaxCand = 1 << 26;
const char kMagic[] = "ethcnn-reliability 1";

void identity(uint32_t* rel) {
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < kBins; ++b) rel[l * kBins + b] = (uint32_t)b * 1024u;
}

// the simulator's table in HBM, made on first use: a simulator starts with the identity
int ensure_rel(ethcnn_sim* k) {
    if (k->d_rel) return 0;
    ethcnn_ctx* c = k->c;
    Scratch d;
    if (int rc = d.alloc(c, kRelWords * 4, "reliability table")) return rc;
    std::vector<uint32_t> rel(kRelWords);
    identity(rel.data());
    hipError_t e = hipMemcpyAsync(d.at(), rel.data(), kRelWords * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(c, ETHCNN_ERR_DEVICE, "reliability table: %s", hipGetErrorString(e));
    k->d_rel = d.release<unsigned>();
    return 0;
}

// the walk's kind for k_ladder_step_risk: a move is weighed by the expected wrong decisions it adds
struct ByRisk {
    typedef ethcnn::risk::StepArgs Args;
    typedef ethcnn_ladder_rung_risk Rung;
    static constexpr int kTableFields = ethcnn::risk::kTableFields;
    u128 cap;  // max_risk_ppm * counted CTUs * kOne
    static void launch(hipStream_t s, const Args& a, int cus) { ethcnn::risk::launch_step(s, a, cus); }
    // (every node of the full search lands in BOTH: its risk is zero under any table)
    int rung0(ethcnn_sim* k, const ethcnn_sim_counts&, Rung& r0, unsigned long long* harm) const {
        ethcnn_sim_risk full;
        if (int rc = ethcnn_risk_eval(k, &r0.thr, 1, &full)) return rc;
        for (int l = 0; l < 3; ++l) {
            r0.exp_wrong_split[l] = full.exp_wrong_split[l];
            r0.exp_wrong_stop[l] = full.exp_wrong_stop[l];
            *harm += full.exp_wrong_split[l] + full.exp_wrong_stop[l];
        }
        return 0;
    }
    void fill(Args& a, const ethcnn_sim* k) const {
        a.rel = k->d_rel;
        a.cap_lo = (unsigned long long)cap;
        a.cap_hi = (unsigned long long)(cap >> 64);
    }
};
}  // namespace

extern "C" int ethcnn_risk_identity(uint32_t* rel) {
    if (!rel) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_risk_identity: null argument");
    identity(rel);
    return ETHCNN_OK;
}

extern "C" int ethcnn_risk_from_hist(const uint64_t* hist, uint32_t* rel) {
    if (!hist || !rel) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_risk_from_hist: null argument");
    struct Block {
        u128 S, T;
        int first, last;
    };
    std::vector<Block> st;
    for (int l = 0; l < 3; ++l) {
        const uint64_t *h0 = hist + (size_t)(l * 2) * kBins, *h1 = h0 + kBins;
        uint32_t* out = rel + l * kBins;
        st.clear();
        for (int b = 0; b < kBins; ++b) {
            st.push_back({(u128)h1[b], (u128)h1[b] + h0[b], b, b});
            while (st.size() >= 2) {
                Block &top = st[st.size() - 1], &below = st[st.size() - 2];
                // (node counts: a level's total lies far below 2^64, so the products fit in 128 bits)
                if (!(top.T == 0 || below.T == 0 || below.S * top.T > top.S * below.T)) break;
                below.S += top.S;
                below.T += top.T;
                below.last = top.last;
                st.pop_back();
            }
        }
        if (st.size() == 1 && st[0].T == 0) {  // a level without any sample
            for (int b = 0; b < kBins; ++b) out[b] = (uint32_t)b * 1024u;
            continue;
        }
        for (const Block& k : st) {
            // floor(S * 2^20 / T) without leaving 128 bits: S = q T + r
            const u128 q = k.S / k.T, r = k.S % k.T;
            const uint32_t v = (uint32_t)(q * kOne + (r << 20) / k.T);
            for (int b = k.first; b <= k.last; ++b) out[b] = v;
        }
    }
    return ETHCNN_OK;
}

extern "C" int ethcnn_risk_write(const char* path, const uint32_t* rel) {
    if (!path || !rel) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_risk_write: null argument");
    for (int i = 0; i < kRelWords; ++i)
        if (rel[i] > kOne)
            return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_risk_write: level %d, bin %d: %u is above ETHCNN_RISK_ONE = %u", i / kBins, i % kBins, rel[i], kOne);
    std::string text = std::string(kMagic) + "\n";
    for (int i = 0; i < kRelWords; ++i) text += std::to_string(rel[i]) + (i % kBins == kBins - 1 ? '\n' : ' ');
    return write_text_atomic(path, text);
}

extern "C" int ethcnn_risk_read(const char* path, uint32_t* rel) {
    if (!path || !rel) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_risk_read: null argument");
    FILE* f = std::fopen(path, "r");
    if (!f) return set_err(nullptr, ETHCNN_ERR_IO, "cannot open %s: %s", path, std::strerror(errno));
    std::string text;
    char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) {
        text.append(buf, got);
        if (text.size() > (size_t)1 << 20) break;  // (a table is at most 3075 tokens of 7 digits)
    }
    const bool io_bad = std::ferror(f) != 0;
    std::fclose(f);
    if (io_bad) return set_err(nullptr, ETHCNN_ERR_IO, "read of %s failed", path);
    const size_t eol = text.find('\n');
    if (eol == std::string::npos || text.compare(0, eol, kMagic) != 0)
        return set_err(nullptr, ETHCNN_ERR_FORMAT, "%s: the first line of a reliability table is \"%s\"", path, kMagic);
    std::vector<uint32_t> v;
    v.reserve(kRelWords);
    size_t at = eol + 1;
    const auto blank = [](char ch) { return ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r'; };
    for (;;) {
        while (at < text.size() && blank(text[at])) ++at;
        if (at == text.size()) break;
        uint64_t x = 0;
        size_t digits = 0;
        while (at < text.size() && text[at] >= '0' && text[at] <= '9' && digits < 9) x = x * 10 + (uint64_t)(text[at++] - '0'), ++digits;
        if (digits == 0 || (at < text.size() && !blank(text[at])))
            return set_err(nullptr, ETHCNN_ERR_FORMAT, "%s: value %zu is no decimal integer in 0..%u", path, v.size(), kOne);
        if (x > kOne) return set_err(nullptr, ETHCNN_ERR_FORMAT, "%s: level %zu, bin %zu: %llu is above %u", path, v.size() / kBins, v.size() % kBins, (unsigned long long)x, kOne);
        if ((int)v.size() == kRelWords) return set_err(nullptr, ETHCNN_ERR_FORMAT, "%s: more than 3 x %d values", path, kBins);
        v.push_back((uint32_t)x);
    }
    if ((int)v.size() != kRelWords) return set_err(nullptr, ETHCNN_ERR_FORMAT, "%s: %zu values where a table has 3 x %d", path, v.size(), kBins);
    std::memcpy(rel, v.data(), kRelWords * 4);
    return ETHCNN_OK;
}

extern "C" int ethcnn_risk_set_reliability(ethcnn_sim* k, const uint32_t* rel) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    std::vector<uint32_t> own(kRelWords);
    if (rel) {
        for (int i = 0; i < kRelWords; ++i)
            if (rel[i] > kOne)
                return set_err(c, ETHCNN_ERR_ARG, "reliability table, level %d, bin %d: %u is above ETHCNN_RISK_ONE = %u", i / kBins, i % kBins, rel[i], kOne);
        std::memcpy(own.data(), rel, kRelWords * 4);
    } else {
        identity(own.data());
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover this copy
    if (int rc = ensure_rel(k)) return rc;
    HIPCHK(c, hipMemcpyAsync(k->d_rel, own.data(), kRelWords * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

extern "C" int ethcnn_risk_eval(ethcnn_sim* k, const ethcnn_sim_thr* cand, int64_t ncand, ethcnn_sim_risk* out) {
    static_assert(sizeof(ethcnn_sim_risk) == ethcnn::risk::kFields * 8 && sizeof(ethcnn_sim_thr) == 24, "the kernel writes these layouts");
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (ncand < 0 || ncand > kMaxCand) return set_err(c, ETHCNN_ERR_ARG, "candidate count %lld outside 0..%lld", (long long)ncand, (long long)kMaxCand);
    if (ncand == 0) return ETHCNN_OK;
    if (!cand || !out) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    for (int64_t i = 0; i < ncand; ++i)
        if (int rc = ethcnn::sim::check_cand(c, cand[i], (long long)i)) return rc;
    std::memset(out, 0, (size_t)ncand * sizeof *out);
    if (k->ctus == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    if (int rc = ensure_rel(k)) return rc;
    const size_t cand_bytes = (size_t)ncand * 24, out_bytes = (size_t)ncand * sizeof *out;
    Scratch d;  // candidates, then their sums: one allocation, both 8-byte aligned
    if (int rc = d.alloc(c, cand_bytes + out_bytes, "expected wrong decisions")) return rc;
    hipError_t e = hipMemcpyAsync(d.at(), cand, cand_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d.at(cand_bytes), 0, out_bytes, c->stream);
    if (e == hipSuccess) {
        ethcnn::risk::launch_risk(c->stream, k->d_recs, (long)k->ctus, d.at<const int>(), (long)ncand, k->d_rel, d.at<unsigned long long>(cand_bytes), cus_of(c));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d.at(cand_bytes), out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "expected wrong decisions: %s", hipGetErrorString(e));
    }
    return ETHCNN_OK;
}

extern "C" int ethcnn_risk_ladder_build(ethcnn_sim* k, const uint64_t weight[4], int grid, int64_t max_rungs, uint64_t max_risk_ppm,
                                        ethcnn_ladder_rung_risk* rungs_out, int64_t* nrungs_out) {
    static_assert(sizeof(ethcnn_ladder_rung_risk) == 112, "the kernel writes this layout");
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (!rungs_out || !nrungs_out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_risk_ladder_build: null output");
    if (ethcnn_ladder_check(weight, grid, max_rungs, 0)) return set_err(c, ETHCNN_ERR_ARG, "%s", ethcnn_last_error(nullptr));
    const uint64_t counted = (uint64_t)k->ctus - k->rejected;
    if (counted == 0) return set_err(c, ETHCNN_ERR_ARG, "a ladder is built from CTUs with valid probabilities: the set holds none");
    return ethcnn::ladder::walk(k, ByRisk{(u128)max_risk_ppm * counted * kOne}, weight, grid, max_rungs, rungs_out, nrungs_out);  // (below 2^64 * 2^31 * 2^20)
}
