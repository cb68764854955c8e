// Evaluation cache: the rules of a device hash table that serves network outputs for input planes it has seen.
// Pure arithmetic, no HIP: eval_cache.hip compiles this text for the device, tests/eval_cache_driver.cpp for the host
// (tests/test_eval_cache_host.py), so the CPU checks the very rules the kernels apply.  The rule structs are template
// parameters: the tests put wrong rules in and show that the corpus tells them from the right ones.
//
// Key.  A row [6][P] is CANONICAL when every value of planes 0-4 is exactly 0.0f or 1.0f (bit patterns: -0.0f is not) and plane
// 5 is uniformly +1.0f or uniformly -1.0f.  Its key is the bit image of planes 0-4, one bit per point - words_per_plane(P)
// words a plane, point p in bit p % 32 of word p / 32, tail bits zero - and one meta word: bit 0 the colour (plane 5 is +1),
// bit 1 want_logits.  Two canonical rows have equal keys iff they are equal float for float and ask for the same outputs.  A
// row that is not canonical is UNCACHEABLE: always evaluated, never inserted.
//
// Table.  n_buckets buckets of W ways; an entry is [tag word, 64 bits][key words][A policy floats][3 value floats], padded to
// 16 bytes.  The tag word holds the hash tag (high half, never 0) and the EPOCH - the number of the commit call that wrote it,
// from 1 - in its low half; the word 0 is an empty way.
//
// Hit: the tag matches AND every key word matches.  Tag equality alone is never a hit.
//
// Insert: one decision per way in way order, from the tag word OBSERVED there (a load, or what a failed compare-and-swap
// returned): empty -> claim it (compare-and-swap 0 -> own word); same tag -> a twin is resident or being written: skip; other
// tag -> next way.  With no way free, ONE victim way chosen from the hash: evict it (compare-and-swap observed -> own) only if
// its epoch is not the current call's, otherwise drop the insert.  At most W + 1 compare-and-swaps, no loop that waits.
//
// Why one way is never evicted twice within one commit launch: an eviction swaps in a word that carries the CURRENT epoch.  A
// later evictor observes that epoch and drops; a concurrent one holds the old word as its expected value and its swap fails.
// Ways are never emptied within a commit, so a way that a row passed by as "other tag" never turns into a free way behind it,
// and twins - which walk the same ways in the same order towards the same victim - end at the first twin's word: one entry.
//
// Miss ranks: a row that needs the network (miss or uncacheable) gets the number of such rows before it (stable order); the
// scan is live_rank.h's: a workgroup of kChunk threads takes the rows a chunk at a time, `carry` goes from chunk to chunk.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define TG_EC_FN __host__ __device__ inline
#else
#define TG_EC_FN inline
#endif

namespace tg_ecache {

constexpr int kLanes = 64;
constexpr int kPlanes = 6, kKeyPlanes = 5;
constexpr int kMaxWays = 64;                  // the probe compares a bucket's tags in one pass: a way per lane
constexpr int kMaxKeyWords = 64;              // ... and a key word per lane (19x19: 61)
constexpr int kMaxBatch = 1 << 20;
constexpr int kChunk = 1024;
constexpr int kWaves = kChunk / kLanes;
constexpr int kCounters = 8;
enum Counter { kLookups = 0, kHits, kUncacheable, kInserts, kTwinSkips, kEvictions, kDropped, kTagOnly };
enum Flag : uint8_t { kHit = 0, kMiss = 1, kUncached = 2 };

constexpr uint32_t kBitsZero = 0x00000000u, kBitsOne = 0x3f800000u, kBitsMinusOne = 0xbf800000u;

TG_EC_FN int words_per_plane(int P) { return (P + 31) / 32; }
TG_EC_FN int key_words(int P) { return kKeyPlanes * words_per_plane(P) + 1; }
TG_EC_FN int entry_words(int P) { return (2 + key_words(P) + (P + 1) + 3 + 3) / 4 * 4; }     // (32-bit words; 16-byte multiple)
TG_EC_FN uint32_t meta_word(bool black, bool want_logits) { return (black ? 1u : 0u) | (want_logits ? 2u : 0u); }

// ---- hash, bucket, tag, victim ----
struct HashRule {
    static TG_EC_FN uint64_t mix(uint64_t x) {                                   // splitmix64's finaliser
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    }
    // key word i's term; the hash is finish(sum of the terms, wrap-around): the lanes of a wavefront take a word each
    static TG_EC_FN uint64_t term(int i, uint32_t word) { return mix(((uint64_t)(uint32_t)(i + 1) << 32) | word); }
    static TG_EC_FN uint64_t finish(uint64_t sum) { return mix(sum + 0x9E3779B97F4A7C15ull); }
};
TG_EC_FN uint32_t bucket_of(uint64_t h, uint32_t n_buckets) { return (uint32_t)(h & 0xffffffffull) % n_buckets; }
TG_EC_FN uint32_t tag_of(uint64_t h) { const uint32_t t = (uint32_t)(h >> 32); return t ? t : 1u; }
TG_EC_FN uint32_t victim_of(uint64_t h, uint32_t ways) { return (uint32_t)(h >> 40) % ways; }
TG_EC_FN uint64_t tag_word(uint32_t tag, uint32_t epoch) { return ((uint64_t)tag << 32) | epoch; }
TG_EC_FN uint32_t word_tag(uint64_t w) { return (uint32_t)(w >> 32); }
TG_EC_FN uint32_t word_epoch(uint64_t w) { return (uint32_t)w; }

template <class H = HashRule>
TG_EC_FN uint64_t hash_key(const uint32_t *key, int n) {
    uint64_t sum = 0;
    for (int i = 0; i < n; ++i) sum += H::term(i, key[i]);
    return H::finish(sum);
}

// ---- hit and insert rules ----
struct HitRule {
    static TG_EC_FN bool hit(bool tag_equal, bool key_equal) { return tag_equal && key_equal; }
};
enum Decision { kClaim, kSkip, kNext };
struct InsertRule {
    static TG_EC_FN Decision way(uint64_t observed, uint32_t tag) {
        return observed == 0 ? kClaim : word_tag(observed) == tag ? kSkip : kNext;
    }
    static TG_EC_FN bool may_evict(uint64_t observed, uint32_t epoch) { return word_epoch(observed) != epoch; }
};
enum Outcome { kInserted, kTwin, kEvicted, kDrop };

// The walk over a bucket's ways.  `load(way)` reads a tag word, `cas(way, expected, desired)` returns what was there (the
// swap happened iff that is `expected`): atomics on the device, plain memory in the host replay.  *way_out: the way that was
// claimed (kInserted, kEvicted).
template <class I = InsertRule, class Load, class Cas>
TG_EC_FN Outcome insert_walk(uint32_t ways, uint32_t victim, uint32_t tag, uint32_t epoch, Load load, Cas cas, uint32_t *way_out) {
    const uint64_t mine = tag_word(tag, epoch);
    uint64_t at_victim = 0;
    for (uint32_t w = 0; w < ways; ++w) {
        uint64_t seen = load(w);
        Decision d = I::way(seen, tag);
        if (d == kClaim) {
            seen = cas(w, 0, mine);
            if (seen == 0) { *way_out = w; return kInserted; }
            d = I::way(seen, tag);                         // (somebody claimed it meanwhile: decide again from their word)
            if (d == kClaim) d = kNext;                    // (cannot happen: ways are never emptied within a commit)
        }
        if (d == kSkip) return kTwin;
        if (w == victim) at_victim = seen;
    }
    if (!I::may_evict(at_victim, epoch)) return kDrop;
    const uint64_t seen = cas(victim, at_victim, mine);
    if (seen == at_victim) { *way_out = victim; return kEvicted; }
    return word_tag(seen) == tag ? kTwin : kDrop;
}

// ---- the key of a row ----
TG_EC_FN bool point_ok(uint32_t bits) { return bits == kBitsZero || bits == kBitsOne; }

// key[key_words(P)] of row [6][P] (float bit patterns); false: the row is uncacheable (key is then not to be used)
inline bool pack_row(const uint32_t *row, int P, bool want_logits, uint32_t *key) {
    const int wpp = words_per_plane(P);
    for (int i = 0; i < kKeyPlanes * wpp; ++i) key[i] = 0;
    bool ok = true;
    for (int pl = 0; pl < kKeyPlanes; ++pl)
        for (int p = 0; p < P; ++p) {
            const uint32_t b = row[pl * P + p];
            ok = ok && point_ok(b);
            if (b == kBitsOne) key[pl * wpp + p / 32] |= 1u << (p % 32);
        }
    bool pos = true, neg = true;
    for (int p = 0; p < P; ++p) {
        pos = pos && row[kKeyPlanes * P + p] == kBitsOne;
        neg = neg && row[kKeyPlanes * P + p] == kBitsMinusOne;
    }
    key[kKeyPlanes * wpp] = meta_word(pos, want_logits);
    return ok && (pos || neg);
}
inline void unpack_row(const uint32_t *key, int P, uint32_t *row, bool *want_logits) {
    const int wpp = words_per_plane(P);
    for (int pl = 0; pl < kKeyPlanes; ++pl)
        for (int p = 0; p < P; ++p) row[pl * P + p] = (key[pl * wpp + p / 32] >> (p % 32)) & 1u ? kBitsOne : kBitsZero;
    const uint32_t meta = key[kKeyPlanes * wpp];
    for (int p = 0; p < P; ++p) row[kKeyPlanes * P + p] = meta & 1u ? kBitsOne : kBitsMinusOne;
    *want_logits = (meta & 2u) != 0;
}

// ---- miss ranks (the scan of live_rank.h over the rows that need the network) ----
struct RankRule {
    static TG_EC_FN int32_t before(int32_t inclusive, int32_t own) { return inclusive - own; }
    static TG_EC_FN int32_t rank(int32_t own, int32_t carry, int32_t waves_before, int32_t lanes_before) {
        return own ? carry + waves_before + lanes_before : -1;
    }
    static TG_EC_FN int32_t next_carry(int32_t carry, int32_t chunk_total) { return carry + chunk_total; }
};
TG_EC_FN int32_t needs_network(uint8_t flag) { return flag != kHit ? 1 : 0; }

template <class R = RankRule>
inline int32_t rank_replay(const uint8_t *flag, int n, int32_t *rank) {
    int32_t carry = 0;
    std::vector<int32_t> inclusive(kChunk);
    for (int c0 = 0; c0 < n; c0 += kChunk) {
        int32_t wave_total[kWaves];
        for (int w = 0; w < kWaves; ++w) {
            int32_t run = 0;
            for (int l = 0; l < kLanes; ++l) {
                const int t = c0 + w * kLanes + l;
                run += t < n ? needs_network(flag[t]) : 0;
                inclusive[w * kLanes + l] = run;
            }
            wave_total[w] = run;
        }
        int32_t waves_before = 0;
        for (int w = 0; w < kWaves; ++w) {
            for (int l = 0; l < kLanes; ++l) {
                const int t = c0 + w * kLanes + l;
                if (t >= n) break;
                const int32_t own = needs_network(flag[t]);
                rank[t] = R::rank(own, carry, waves_before, R::before(inclusive[w * kLanes + l], own));
            }
            waves_before += wave_total[w];
        }
        carry = R::next_carry(carry, waves_before);
    }
    return carry;
}

// ---- the table and the calls on the host, in the kernels' order of operations, rows in row order ----
template <class H = HashRule, class Hit = HitRule, class I = InsertRule, class R = RankRule>
struct Replay {
    int P, A, K, E;
    uint32_t ways, n_buckets, epoch = 0;
    std::vector<uint32_t> table;                   // entries * E words
    uint64_t counters[kCounters] = {};
    // the probe in flight
    std::vector<uint8_t> flag;
    std::vector<int32_t> rank;
    std::vector<int32_t> miss_row;
    std::vector<uint32_t> miss_planes;
    bool want_logits = false;

    Replay(int P_, uint32_t entries, uint32_t ways_)
        : P(P_), A(P_ + 1), K(key_words(P_)), E(entry_words(P_)), ways(ways_), n_buckets(entries / ways_), table((size_t)entries * E, 0) {}

    uint32_t *entry(uint32_t bucket, uint32_t way) { return table.data() + ((size_t)bucket * ways + way) * E; }
    static uint64_t read_tag(const uint32_t *e) { uint64_t w; std::memcpy(&w, e, 8); return w; }
    void clear() { std::fill(table.begin(), table.end(), 0u); }

    // planes [n][6][P], policy [n][A], value [n][3] (bit patterns): fills the hit rows; returns n_miss
    int32_t probe(const uint32_t *planes, int n, bool logits, uint32_t *policy, uint32_t *value) {
        want_logits = logits;
        flag.assign(n, kMiss);
        std::vector<uint32_t> key(K);
        for (int r = 0; r < n; ++r) {
            counters[kLookups]++;
            if (!pack_row(planes + (size_t)r * kPlanes * P, P, logits, key.data())) {
                flag[r] = kUncached;
                counters[kUncacheable]++;
                continue;
            }
            const uint64_t h = hash_key<H>(key.data(), K);
            const uint32_t b = bucket_of(h, n_buckets), tag = tag_of(h);
            for (uint32_t w = 0; w < ways; ++w) {
                const uint32_t *e = entry(b, w);
                const bool tag_equal = read_tag(e) != 0 && word_tag(read_tag(e)) == tag;
                if (!tag_equal) continue;
                const bool key_equal = std::memcmp(e + 2, key.data(), K * 4) == 0;
                if (Hit::hit(tag_equal, key_equal)) {
                    std::memcpy(policy + (size_t)r * A, e + 2 + K, A * 4);
                    std::memcpy(value + (size_t)r * 3, e + 2 + K + A, 3 * 4);
                    flag[r] = kHit;
                    counters[kHits]++;
                    break;
                }
                counters[kTagOnly]++;
            }
        }
        rank.assign(n, -1);
        const int32_t n_miss = rank_replay<R>(flag.data(), n, rank.data());
        miss_row.assign(n, -1);
        miss_planes.assign((size_t)n * kPlanes * P, 0);
        for (int r = 0; r < n; ++r)
            if (rank[r] >= 0 && rank[r] < n) {             // (a wrong rank rule may rank out of range: the replay stays in bounds)
                miss_row[rank[r]] = r;
                std::memcpy(miss_planes.data() + (size_t)rank[r] * kPlanes * P, planes + (size_t)r * kPlanes * P, (size_t)kPlanes * P * 4);
            }
        return n_miss;
    }

    // miss_policy [n_miss][A], miss_value [n_miss][3]: scattered to the rows, cacheable misses inserted
    void commit(const uint32_t *miss_policy, const uint32_t *miss_value, int32_t n_miss, uint32_t *policy, uint32_t *value) {
        ++epoch;
        std::vector<uint32_t> key(K);
        for (int32_t m = 0; m < n_miss; ++m) {
            const int32_t r = miss_row[m];
            if (r < 0) continue;
            std::memcpy(policy + (size_t)r * A, miss_policy + (size_t)m * A, A * 4);
            std::memcpy(value + (size_t)r * 3, miss_value + (size_t)m * 3, 3 * 4);
            if (flag[r] != kMiss) continue;
            pack_row(miss_planes.data() + (size_t)m * kPlanes * P, P, want_logits, key.data());
            const uint64_t h = hash_key<H>(key.data(), K);
            const uint32_t b = bucket_of(h, n_buckets), tag = tag_of(h);
            uint32_t way = 0;
            const Outcome o = insert_walk<I>(
                ways, victim_of(h, ways), tag, epoch, [&](uint32_t w) { return read_tag(entry(b, w)); },
                [&](uint32_t w, uint64_t expected, uint64_t desired) {
                    const uint64_t seen = read_tag(entry(b, w));
                    if (seen == expected) std::memcpy(entry(b, w), &desired, 8);
                    return seen;
                },
                &way);
            counters[o == kInserted ? kInserts : o == kEvicted ? kEvictions : o == kTwin ? kTwinSkips : kDropped]++;
            if (o == kEvicted) counters[kInserts]++;       // (an eviction is an insert that displaced an entry)
            if (o == kInserted || o == kEvicted) {
                uint32_t *e = entry(b, way);
                std::memcpy(e + 2, key.data(), K * 4);
                std::memcpy(e + 2 + K, miss_policy + (size_t)m * A, A * 4);
                std::memcpy(e + 2 + K + A, miss_value + (size_t)m * 3, 3 * 4);
            }
        }
    }
};

}  // namespace tg_ecache
