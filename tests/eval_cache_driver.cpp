// Stand-alone driver of csrc/eval_cache.h for tests/test_eval_cache_host.py (host compiler, no HIP): the key, the hash, the miss
// ranks and the kernels' order of operations on the CPU, under the header's rules or wrong ones put in through its template
// parameters.  One command per input line, one output line each; floats travel as their bit patterns in hexadecimal.
//   key S want_logits n_buckets ways  row[6 P]              -> canonical hash bucket tag victim key[K]
//   unpack S key[K]                                          -> want_logits row[6 P]
//   rank rule flags                                          -> count rank[n]      (flags: one digit a row; rule 0 right, 1 an
//                                                                                   inclusive scan, 2 a carry dropped between chunks)
//   new variant S entries ways                               -> ok                 (variant 0 the header's rules, 1 a degenerate hash,
//                                                             2 a degenerate hash and "a tag match is a hit", 3 evict regardless of epoch)
//   probe want_logits n  rows[n][6 P]                        -> n_miss flags[n] miss_row[n_miss]
//   commit  outputs[n_miss][A + 3]                           -> policy and value of every row of the probe [n][A + 3]
//   clear                                                    -> ok
//   stats                                                    -> the 8 counters
//   table                                                    -> tag word and key of every entry that is not empty: index tag key[K] ;
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../tamago_amd/csrc/eval_cache.h"

namespace ec = tg_ecache;

struct OneBucketHash : ec::HashRule {
    static uint64_t term(int, uint32_t) { return 0; }
    static uint64_t finish(uint64_t) { return 0x1234567800000000ull; }
};
struct TagIsHit {
    static bool hit(bool tag_equal, bool) { return tag_equal; }
};
struct EvictAnyEpoch : ec::InsertRule {
    static bool may_evict(uint64_t, uint32_t) { return true; }
};
struct InclusiveRule : ec::RankRule {
    static int32_t before(int32_t inclusive, int32_t) { return inclusive; }
};
struct DroppedCarryRule : ec::RankRule {
    static int32_t next_carry(int32_t, int32_t chunk_total) { return chunk_total; }
};

struct Session {
    virtual ~Session() {}
    virtual int32_t probe(const uint32_t *planes, int n, bool logits, uint32_t *policy, uint32_t *value) = 0;
    virtual void commit(const uint32_t *mp, const uint32_t *mv, int32_t n_miss, uint32_t *policy, uint32_t *value) = 0;
    virtual void clear() = 0;
    virtual const uint64_t *counters() = 0;
    virtual const std::vector<uint8_t> &flags() = 0;
    virtual const std::vector<int32_t> &miss_rows() = 0;
    virtual const std::vector<uint32_t> &table() = 0;
};
template <class RP>
struct SessionOf : Session {
    RP r;
    SessionOf(int P, uint32_t entries, uint32_t ways) : r(P, entries, ways) {}
    int32_t probe(const uint32_t *planes, int n, bool logits, uint32_t *policy, uint32_t *value) override {
        return r.probe(planes, n, logits, policy, value);
    }
    void commit(const uint32_t *mp, const uint32_t *mv, int32_t n_miss, uint32_t *policy, uint32_t *value) override {
        r.commit(mp, mv, n_miss, policy, value);
    }
    void clear() override { r.clear(); }
    const uint64_t *counters() override { return r.counters; }
    const std::vector<uint8_t> &flags() override { return r.flag; }
    const std::vector<int32_t> &miss_rows() override { return r.miss_row; }
    const std::vector<uint32_t> &table() override { return r.table; }
};

static bool read_hex(uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (scanf("%x", &out[i]) != 1) return false;
    return true;
}

int main() {
    std::unique_ptr<Session> session;
    int S = 0, P = 0, A = 0, K = 0, n = 0, n_miss = 0;
    std::vector<uint32_t> policy, value;
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        const std::string c(cmd);
        if (c == "key") {
            int s, logits;
            unsigned nb, ways;
            if (scanf("%d %d %u %u", &s, &logits, &nb, &ways) != 4 || s < 1 || s > 25 || nb < 1 || ways < 1) return 2;
            const int p = s * s, k = ec::key_words(p);
            std::vector<uint32_t> row((size_t)ec::kPlanes * p), key(k);
            if (!read_hex(row.data(), row.size())) return 2;
            const bool ok = ec::pack_row(row.data(), p, logits != 0, key.data());
            const uint64_t h = ec::hash_key(key.data(), k);
            printf("%d %llx %u %x %u", ok ? 1 : 0, (unsigned long long)h, ec::bucket_of(h, nb), ec::tag_of(h), ec::victim_of(h, ways));
            for (int i = 0; i < k; ++i) printf(" %x", key[i]);
            printf("\n");
        } else if (c == "unpack") {
            int s;
            if (scanf("%d", &s) != 1 || s < 1 || s > 25) return 2;
            const int p = s * s, k = ec::key_words(p);
            std::vector<uint32_t> row((size_t)ec::kPlanes * p), key(k);
            if (!read_hex(key.data(), key.size())) return 2;
            bool logits = false;
            ec::unpack_row(key.data(), p, row.data(), &logits);
            printf("%d", logits ? 1 : 0);
            for (uint32_t w : row) printf(" %x", w);
            printf("\n");
        } else if (c == "rank") {
            int rule;
            static char buf[1 << 21];
            if (scanf("%d %2097151s", &rule, buf) != 2 || rule < 0 || rule > 2) return 2;
            const std::string text(buf);
            std::vector<uint8_t> flag(text.size());
            for (size_t i = 0; i < text.size(); ++i) flag[i] = (uint8_t)(text[i] - '0');
            std::vector<int32_t> rank(flag.size());
            const int T = (int)flag.size();
            const int32_t count = rule == 0   ? ec::rank_replay<ec::RankRule>(flag.data(), T, rank.data())
                                  : rule == 1 ? ec::rank_replay<InclusiveRule>(flag.data(), T, rank.data())
                                              : ec::rank_replay<DroppedCarryRule>(flag.data(), T, rank.data());
            printf("%d", count);
            for (int32_t r : rank) printf(" %d", r);
            printf("\n");
        } else if (c == "new") {
            int variant;
            unsigned entries, ways;
            if (scanf("%d %d %u %u", &variant, &S, &entries, &ways) != 4) return 2;
            if (S < 1 || S > 25 || ways < 1 || ways > (unsigned)ec::kMaxWays || entries < ways || entries % ways) return 2;
            P = S * S, A = P + 1, K = ec::key_words(P);
            if (variant == 0) session.reset(new SessionOf<ec::Replay<>>(P, entries, ways));
            else if (variant == 1) session.reset(new SessionOf<ec::Replay<OneBucketHash>>(P, entries, ways));
            else if (variant == 2) session.reset(new SessionOf<ec::Replay<OneBucketHash, TagIsHit>>(P, entries, ways));
            else if (variant == 3) session.reset(new SessionOf<ec::Replay<ec::HashRule, ec::HitRule, EvictAnyEpoch>>(P, entries, ways));
            else return 2;
            n = n_miss = 0;
            printf("ok\n");
        } else if (c == "probe") {
            int logits;
            if (!session || scanf("%d %d", &logits, &n) != 2 || n < 1 || n > ec::kMaxBatch) return 2;
            std::vector<uint32_t> planes((size_t)n * ec::kPlanes * P);
            if (!read_hex(planes.data(), planes.size())) return 2;
            policy.assign((size_t)n * A, 0xdeadbeefu);
            value.assign((size_t)n * 3, 0xdeadbeefu);
            n_miss = session->probe(planes.data(), n, logits != 0, policy.data(), value.data());
            printf("%d", n_miss);
            for (uint8_t f : session->flags()) printf(" %d", (int)f);
            for (int m = 0; m < n_miss && m < n; ++m) printf(" %d", session->miss_rows()[m]);
            printf("\n");
        } else if (c == "commit") {
            if (!session || n < 1) return 2;
            const int rows = n_miss < 0 ? 0 : n_miss > n ? n : n_miss;
            std::vector<uint32_t> out((size_t)rows * (A + 3)), mp((size_t)rows * A), mv((size_t)rows * 3);
            if (!read_hex(out.data(), out.size())) return 2;
            for (int m = 0; m < rows; ++m) {
                for (int i = 0; i < A; ++i) mp[(size_t)m * A + i] = out[(size_t)m * (A + 3) + i];
                for (int i = 0; i < 3; ++i) mv[(size_t)m * 3 + i] = out[(size_t)m * (A + 3) + A + i];
            }
            session->commit(mp.data(), mv.data(), rows, policy.data(), value.data());
            for (int r = 0; r < n; ++r) {
                for (int i = 0; i < A; ++i) printf("%x ", policy[(size_t)r * A + i]);
                for (int i = 0; i < 3; ++i) printf("%x ", value[(size_t)r * 3 + i]);
            }
            printf("\n");
            n = 0;
        } else if (c == "clear") {
            if (!session) return 2;
            session->clear();
            printf("ok\n");
        } else if (c == "stats") {
            if (!session) return 2;
            for (int i = 0; i < ec::kCounters; ++i) printf("%llu ", (unsigned long long)session->counters()[i]);
            printf("\n");
        } else if (c == "table") {
            if (!session) return 2;
            const std::vector<uint32_t> &t = session->table();
            const size_t E = (size_t)ec::entry_words(P);
            for (size_t e = 0; e * E < t.size(); ++e) {
                const uint64_t tag = ((uint64_t)t[e * E + 1] << 32) | t[e * E];
                if (!tag) continue;
                printf("%zu %llx", e, (unsigned long long)tag);
                for (int i = 0; i < K; ++i) printf(" %x", t[e * E + 2 + i]);
                printf(" ; ");
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
