// Host driver of csrc/tree_dump.h (tests/test_tree_dump_host.py builds and runs it; no HIP).  It compiles the very header the
// kernels compile and answers, as JSON on stdout:
//   layout                      the constants and the child-array list the header expands
//   offsets <n> <total>         node_offset(n), every row's offset, record_bytes
//   scan <counts file>          first_child and total of the scan replay under the right rule and two wrong ones
//   tree <tree file> <record>   the digest under the right rule and two wrong ones; the packed record written to <record>
// counts file: int32 n, then n int32.  tree file: int32 A, num_nodes, current_root, err, to_move, 0, 0, 0; num_nodes NodeRec;
// then every child array of the pool's list, [num_nodes][A] in its own element type.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../tamago_amd/csrc/tree_dump.h"

using namespace tg_dump;

// ---- wrong rules ----
struct InclusiveScan : ScanRule {                         // a node's own children counted in front of it
    static int32_t before(int32_t inclusive, int32_t) { return inclusive; }
};
struct DroppedCarry : ScanRule {                          // every chunk starts from nothing
    static int64_t next_carry(int64_t, int32_t) { return 0; }
};
struct NoChildIndex : DigestRule {                        // a term that does not know which child it belongs to
    static uint64_t term(uint64_t seed, int field, int32_t node, int32_t, uint64_t bits) { return DigestRule::term(seed, field, node, 0, bits); }
};
struct StaleTail : DigestRule {                           // the whole pool row, stale entries included
    static int32_t used(int32_t, int32_t A) { return A; }
};

static std::vector<unsigned char> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<unsigned char> data;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + got);
    fclose(f);
    return data;
}

static void need(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "bad input: %s\n", what); exit(2); }
}

template <class R>
static void print_scan(const char *name, const std::vector<int32_t> &counts, bool last) {
    std::vector<int64_t> first(counts.size());
    const int64_t total = scan_replay<R>(counts.data(), (int)counts.size(), first.data());
    printf("\"%s\": {\"total\": %" PRId64 ", \"first\": [", name, total);
    for (size_t i = 0; i < first.size(); ++i) printf("%s%" PRId64, i ? "," : "", first[i]);
    printf("]}%s", last ? "" : ", ");
}

template <class D>
static void print_digest(const char *name, const HostTree &t, bool last) {
    uint64_t d[2];
    digest_replay<D>(t, d);
    printf("\"%s\": [\"%016" PRIx64 "\", \"%016" PRIx64 "\"]%s", name, d[0], d[1], last ? "" : ", ");
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "layout") {
        printf("{\"head_words\": %d, \"node_bytes\": %zu, \"lanes\": %d, \"chunk\": %d, \"field_arrays\": %d, ", (int)kHeadWords,
               sizeof(DumpNode), kLanes, kChunk, (int)kFieldArrays);
        printf("\"seeds\": [\"%016" PRIx64 "\", \"%016" PRIx64 "\"], \"arrays\": [", kSeed[0], kSeed[1]);
        bool any = false;
        for (int k = 0; k < tg_pool::kNumArrays; ++k) {
            if (!tg_pool::kArrays[k].per_child) continue;
            printf("%s[\"%s\", %zu, %d]", any ? ", " : "", tg_pool::kArrays[k].name, tg_pool::kArrays[k].elem_bytes, k);
            any = true;
        }
        printf("]}\n");
        return 0;
    }
    if (cmd == "offsets" && argc == 4) {
        const size_t n = strtoull(argv[2], nullptr, 10), total = strtoull(argv[3], nullptr, 10);
        printf("{\"nodes_end\": %zu, \"rows\": {", node_offset(n));
        bool any = false;
        for (int k = 0; k < tg_pool::kNumArrays; ++k) {
            if (!tg_pool::kArrays[k].per_child) continue;
            printf("%s\"%s\": %zu", any ? ", " : "", tg_pool::kArrays[k].name, row_offset(k, n, total));
            any = true;
        }
        printf("}, \"bytes\": %zu}\n", record_bytes(n, total));
        return 0;
    }
    if (cmd == "scan" && argc == 3) {
        const std::vector<unsigned char> data = read_file(argv[2]);
        need(data.size() >= 4, "counts file too short");
        int32_t n;
        std::memcpy(&n, data.data(), 4);
        need(n >= 0 && data.size() == 4 + (size_t)n * 4, "counts file size");
        std::vector<int32_t> counts(n);
        if (n) std::memcpy(counts.data(), data.data() + 4, (size_t)n * 4);
        printf("{");
        print_scan<ScanRule>("right", counts, false);
        print_scan<InclusiveScan>("inclusive", counts, false);
        print_scan<DroppedCarry>("dropped_carry", counts, true);
        printf("}\n");
        return 0;
    }
    if (cmd == "tree" && argc == 4) {
        const std::vector<unsigned char> data = read_file(argv[2]);
        need(data.size() >= 32, "tree file too short");
        int32_t head[8];
        std::memcpy(head, data.data(), 32);
        HostTree t;
        t.A = head[0], t.num_nodes = head[1], t.current_root = head[2], t.err = head[3], t.to_move = head[4];
        need(t.A >= 1 && t.A <= 1023 && t.num_nodes >= 0 && t.num_nodes <= (1 << 24), "tree head");
        const size_t n = (size_t)t.num_nodes, per = n * (size_t)t.A;
        need(data.size() == 32 + n * sizeof(tg_pool::NodeRec) + per * (tg_pool::bytes_per_node(t.A) - sizeof(tg_pool::NodeRec)) / t.A, "tree file size");
        size_t at = 32;
        t.node.resize(n);
        if (n) std::memcpy(t.node.data(), data.data() + at, n * sizeof(tg_pool::NodeRec));
        at += n * sizeof(tg_pool::NodeRec);
#define LOAD(member, E, per_child, remap)                                        \
        t.member.resize(per);                                                    \
        if (per) std::memcpy(t.member.data(), data.data() + at, per * sizeof(E)); \
        at += per * sizeof(E);
        TG_NODE_POOL_CHILD_ARRAYS(LOAD)
#undef LOAD
        const std::vector<unsigned char> rec = pack_replay<ScanRule>(t);
        FILE *f = fopen(argv[3], "wb");
        need(f != nullptr, "cannot write the record");
        if (!rec.empty()) fwrite(rec.data(), 1, rec.size(), f);
        fclose(f);
        printf("{");
        print_digest<DigestRule>("right", t, false);
        print_digest<NoChildIndex>("no_child_index", t, false);
        print_digest<StaleTail>("stale_tail", t, false);
        printf("\"record_bytes\": %zu}\n", rec.size());
        return 0;
    }
    fprintf(stderr, "usage: tree_dump_driver layout | offsets <n> <total> | scan <counts> | tree <tree> <record>\n");
    return 2;
}
