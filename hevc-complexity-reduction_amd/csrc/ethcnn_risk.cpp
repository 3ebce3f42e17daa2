// ethcnn_risk.cpp -- host side of the expected wrong decisions (include/ethcnn.h "partition-search simulation: expected wrong
// decisions"): the simulator's reliability table, the evaluation around k_sim_risk and the ladder build around k_ladder_step_risk
// (ethcnn_risk.hip), and the host-only tables: identity, the monotone fit to a calibrator's histogram, and the table file.
#include "ethcnn_ctx.h"
#include "ethcnn_budget.h"
#include "ethcnn_ladder.h"
#include "ethcnn_risk.h"
#include "ethcnn_sim.h"

using ethcnn::budget::kMaxRungs;
using ethcnn::risk::kBins;
using ethcnn::risk::kOne;
using ethcnn::risk::kRelWords;

namespace {
typedef unsigned __int128 u128;
constexpr int64_t kMaxCand = 1 << 26;
const uint64_t kDefaultWeight[4] = {64, 16, 4, 1};
const char kMagic[] = "ethcnn-reliability 1";

int cus_of(const ethcnn_ctx* c) { return c->cus > 0 ? c->cus : 256; }

void identity(uint32_t* rel) {
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < kBins; ++b) rel[l * kBins + b] = (uint32_t)b * 1024u;
}

// the simulator's table in HBM, made on first use: a simulator starts with the identity
int ensure_rel(ethcnn_sim* k) {
    if (k->d_rel) return 0;
    ethcnn_ctx* c = k->c;
    unsigned* p = nullptr;
    if (hipMalloc((void**)&p, kRelWords * 4) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_NOMEM, "reliability table: %d bytes do not fit in device memory", kRelWords * 4);
    }
    std::vector<uint32_t> rel(kRelWords);
    identity(rel.data());
    hipError_t e = hipMemcpyAsync(p, rel.data(), kRelWords * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return set_err(c, ETHCNN_ERR_DEVICE, "reliability table: %s", hipGetErrorString(e));
    }
    k->d_rel = p;
    return 0;
}
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
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());  // never a partial table file
    FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) return set_err(nullptr, ETHCNN_ERR_IO, "cannot open %s for writing: %s", tmp.c_str(), std::strerror(errno));
    int rc = 0;
    if (std::fprintf(f, "%s\n", kMagic) < 0) rc = set_err(nullptr, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
    for (int i = 0; i < kRelWords && !rc; ++i)
        if (std::fprintf(f, "%u%c", rel[i], i % kBins == kBins - 1 ? '\n' : ' ') < 0)
            rc = set_err(nullptr, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
    if (std::fclose(f) != 0 && !rc) rc = set_err(nullptr, ETHCNN_ERR_IO, "close of %s failed", tmp.c_str());
    if (!rc && std::rename(tmp.c_str(), path) != 0) rc = set_err(nullptr, ETHCNN_ERR_IO, "rename %s -> %s failed: %s", tmp.c_str(), path, std::strerror(errno));
    if (rc) std::remove(tmp.c_str());
    return rc;
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
    uint8_t* d = nullptr;  // candidates, then their sums: one allocation, both 8-byte aligned
    if (hipMalloc((void**)&d, cand_bytes + out_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_NOMEM, "expected wrong decisions: %llu bytes for %lld candidates do not fit in device memory",
                       (unsigned long long)(cand_bytes + out_bytes), (long long)ncand);
    }
    hipError_t e = hipMemcpyAsync(d, cand, cand_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d + cand_bytes, 0, out_bytes, c->stream);
    if (e == hipSuccess) {
        ethcnn::risk::launch_risk(c->stream, k->d_recs, (long)k->ctus, reinterpret_cast<const int*>(d), (long)ncand, k->d_rel,
                                  reinterpret_cast<unsigned long long*>(d + cand_bytes), cus_of(c));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + cand_bytes, out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "expected wrong decisions: %s", hipGetErrorString(e));
    }
    return ETHCNN_OK;
}

extern "C" int ethcnn_risk_ladder_build(ethcnn_sim* k, const uint64_t weight[4], int grid, int64_t max_rungs, uint64_t max_risk_ppm,
                                        ethcnn_ladder_rung_risk* rungs_out, int64_t* nrungs_out) {
    using namespace ethcnn::ladder;
    static_assert(sizeof(ethcnn_ladder_rung_risk) == 112, "the kernel writes this layout");
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (!rungs_out || !nrungs_out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_risk_ladder_build: null output");
    if (ethcnn_ladder_check(weight, grid, max_rungs, 0)) return set_err(c, ETHCNN_ERR_ARG, "%s", ethcnn_last_error(nullptr));
    const uint64_t counted = (uint64_t)k->ctus - k->rejected;
    if (counted == 0) return set_err(c, ETHCNN_ERR_ARG, "a ladder is built from CTUs with valid probabilities: the set holds none");
    const uint64_t* w = weight ? weight : kDefaultWeight;
    // a CTU has at most 1, 4, 16 and 64 checked CUs of the four sizes: the largest cost any rung can have on this set
    const u128 bound = (u128)k->ctus * ((u128)w[0] + (u128)4 * w[1] + (u128)16 * w[2] + (u128)64 * w[3]);
    if (bound >> 64) return set_err(c, ETHCNN_ERR_ARG, "the cost of a set of %lld CTUs may not fit in 64 bits under these weights", (long long)k->ctus);

    // rung 0, the full search, by the simulator's own evaluations (every node lands in BOTH: its risk is zero under any table)
    std::vector<ethcnn_ladder_rung_risk> rungs((size_t)max_rungs);
    std::memset(rungs.data(), 0, rungs.size() * sizeof rungs[0]);
    ethcnn_ladder_rung_risk& r0 = rungs[0];
    r0.thr = ethcnn_sim_thr{{1024, 1024, 1024}, {-1, -1, -1}};
    r0.coord = -1;
    r0.value = 0;
    ethcnn_sim_counts full;
    ethcnn_sim_risk full_risk;
    if (int rc = ethcnn_sim_eval(k, &r0.thr, 1, ETHCNN_SIM_GATES_NONE, &full)) return rc;
    if (int rc = ethcnn_risk_eval(k, &r0.thr, 1, &full_risk)) return rc;
    unsigned long long st[kStateWords] = {0};
    for (int d = 0; d < 4; ++d) {
        r0.checked[d] = full.checked[d];
        st[kStateCost] += w[d] * full.checked[d];
    }
    for (int l = 0; l < 3; ++l) {
        r0.exp_wrong_split[l] = full_risk.exp_wrong_split[l];
        r0.exp_wrong_stop[l] = full_risk.exp_wrong_stop[l];
        st[kStateBad] += full_risk.exp_wrong_split[l] + full_risk.exp_wrong_stop[l];
    }
    st[kStateRungs] = 1;
    st[kStateDone] = max_rungs == 1;
    for (int l = 0; l < 3; ++l) st[kStateUp + l] = 1024ull, st[kStateDown + l] = (unsigned long long)-1ll;

    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover these launches
    const int slots = slots_of(grid);
    const size_t table_bytes = (size_t)6 * slots * ethcnn::risk::kTableFields * 8, state_bytes = kStateWords * 8,
                 rung_bytes = (size_t)max_rungs * sizeof(ethcnn_ladder_rung_risk);
    uint8_t* d = nullptr;  // table, state, rungs: one allocation, each part 8-byte aligned
    if (hipMalloc((void**)&d, table_bytes + state_bytes + rung_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_NOMEM, "ladder search: %llu bytes of table, state and rungs do not fit in device memory",
                       (unsigned long long)(table_bytes + state_bytes + rung_bytes));
    }
    ethcnn::risk::StepArgs a;
    a.recs = k->d_recs;
    a.n = (long)k->ctus;
    a.table = reinterpret_cast<unsigned long long*>(d);
    a.state = reinterpret_cast<unsigned long long*>(d + table_bytes);
    a.rungs = reinterpret_cast<ethcnn_ladder_rung_risk*>(d + table_bytes + state_bytes);
    a.rel = k->d_rel;
    for (int i = 0; i < 4; ++i) a.weight[i] = w[i];
    const u128 cap = (u128)max_risk_ppm * counted * kOne;  // (below 2^64 * 2^31 * 2^20)
    a.cap_lo = (unsigned long long)cap;
    a.cap_hi = (unsigned long long)(cap >> 64);
    a.grid = grid;
    a.slots = slots;
    a.values = values_of(grid);
    a.max_rungs = (int)max_rungs;

    hipError_t e = hipMemsetAsync(d, 0, table_bytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.state, st, state_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.rungs, &r0, sizeof r0, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    // steps in batches: a step that finds the done flag set exits at once, so a batch may run past the end of the walk
    while (e == hipSuccess && !st[kStateDone]) {
        const int64_t left = max_rungs - (int64_t)st[kStateRungs];
        for (int64_t i = 0; i < std::min<int64_t>(kBatch, left); ++i) ethcnn::risk::launch_step(c->stream, a, cus_of(c));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(st, a.state, state_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !st[kStateDone] && (int64_t)st[kStateRungs] + left <= max_rungs) {  // every step appends a rung or sets the flag
            (void)hipFree(d);
            return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: a batch of steps left the walk at %llu rungs without ending it", st[kStateRungs]);
        }
    }
    const int64_t n = (int64_t)st[kStateRungs];
    if (e == hipSuccess && (n < 1 || n > max_rungs || st[kStateTicket])) {
        (void)hipFree(d);
        return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: the state block came back with %lld rungs and ticket %llu", (long long)n, st[kStateTicket]);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rungs.data(), a.rungs, (size_t)n * sizeof(ethcnn_ladder_rung_risk), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: %s", hipGetErrorString(e));
    }
    std::memcpy(rungs_out, rungs.data(), (size_t)n * sizeof(ethcnn_ladder_rung_risk));
    *nrungs_out = n;
    return ETHCNN_OK;
}
