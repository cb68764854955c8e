// Host driver of csrc/tree_load.h (tests/test_tree_load_host.py builds and runs it; no HIP).  It compiles the very header the
// library compiles and answers, as JSON on stdout:
//   rules                                the rule codes of check_record by name
//   check <record> <A> <W> <N>           check_record's verdict on the bytes of <record>
//   roundtrip <tree file> <W> <record>   the tree packed (tree_dump.h pack_replay, written to <record>), checked, and unpacked
//                                        over a stale pool under the right fill rule and two wrong ones
// tree file: tests/tree_dump_driver.cpp's format.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../tamago_amd/csrc/tree_load.h"

using namespace tg_dump;
using namespace tg_load;

// ---- wrong rules ----
struct WholePasses : FillRule {                           // 64 entries a pass from the record, whatever `children` says
    static bool from_record(int32_t k, int32_t children) { return k < (children + kLanes - 1) / kLanes * kLanes; }
};
struct KeptTail : FillRule {                              // the tail left as it was
    static bool writes_tail() { return false; }
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

static void print_verdict(const Verdict &v) { printf("{\"rule\": %d, \"node\": %d, \"child\": %d}", v.rule, v.node, v.child); }

// a pool of `nodes` nodes whose every byte is stale
static HostTree stale_pool(int32_t A, size_t nodes) {
    HostTree t;
    t.A = A, t.num_nodes = (int32_t)nodes, t.to_move = 0x5A5A5A5A, t.err = 0x5A5A5A5A;
    t.node.resize(nodes);
    if (nodes) std::memset(t.node.data(), 0x5A, nodes * sizeof(tg_pool::NodeRec));
#define STALE(member, E, per_child, remap) \
    t.member.resize(nodes * (size_t)A);    \
    if (nodes) std::memset(t.member.data(), 0x5A, nodes * (size_t)A * sizeof(E));
    TG_NODE_POOL_CHILD_ARRAYS(STALE)
#undef STALE
    return t;
}

static bool tails_canonical(const HostTree &t) {
    for (int32_t i = 0; i < t.num_nodes; ++i)
        for (int32_t k = t.node[i].children; k < t.A; ++k) {
#define TAIL(member, E, per_child, remap)                                      \
            {                                                                  \
                const E want = tail_value<E>(tg_pool::k_##member);             \
                if (std::memcmp(&t.member[(size_t)i * t.A + k], &want, sizeof(E)) != 0) return false; \
            }
            TG_NODE_POOL_CHILD_ARRAYS(TAIL)
#undef TAIL
        }
    return true;
}

static bool same_rows(const HostTree &a, const HostTree &b) {
    const size_t n = (size_t)a.num_nodes;
    if (a.num_nodes != b.num_nodes || (n && std::memcmp(a.node.data(), b.node.data(), n * sizeof(tg_pool::NodeRec)) != 0)) return false;
#define SAME(member, E, per_child, remap) \
    if (n && std::memcmp(a.member.data(), b.member.data(), n * (size_t)a.A * sizeof(E)) != 0) return false;
    TG_NODE_POOL_CHILD_ARRAYS(SAME)
#undef SAME
    return true;
}

template <class F>
static HostTree unpacked(const std::vector<unsigned char> &rec, int32_t A, size_t nodes) {
    HostTree t = stale_pool(A, nodes + 3);                // (a pool larger than the tree: stale nodes beyond num_nodes)
    unpack_replay<F>(rec.data(), t);
    return t;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "rules") {
        printf("{\"ok\": %d, \"length\": %d, \"head_pad\": %d, \"num_nodes\": %d, \"current_root\": %d, \"err_word\": %d, \"to_move\": %d, "
               "\"children\": %d, \"first_child\": %d, \"node_pad\": %d, \"node_count\": %d, \"total\": %d, \"child_index\": %d, "
               "\"edges\": %d, \"parent\": %d, \"root\": %d, \"action\": %d, \"child_count\": %d, \"rules\": %d}\n",
               kOk, kLength, kHeadPad, kNumNodes, kCurrentRoot, kErrWord, kToMove, kChildren, kFirstChild, kNodePad, kNodeCount, kTotal,
               kChildIndex, kEdges, kParent, kRoot, kAction, kChildCount, kRules);
        return 0;
    }
    if (cmd == "check" && argc == 6) {
        const std::vector<unsigned char> rec = read_file(argv[2]);
        print_verdict(check_record(rec.data(), rec.size(), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
        printf("\n");
        return 0;
    }
    if (cmd == "roundtrip" && argc == 5) {
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
        FILE *f = fopen(argv[4], "wb");
        need(f != nullptr, "cannot write the record");
        if (!rec.empty()) fwrite(rec.data(), 1, rec.size(), f);
        fclose(f);
        uint64_t want[2], got[2];
        digest_replay<DigestRule>(t, want);
        printf("{\"record_bytes\": %zu, \"check\": ", rec.size());
        print_verdict(check_record(rec.data(), rec.size(), t.A, atoi(argv[3]), t.num_nodes));
        printf(", \"too_small\": ");
        print_verdict(check_record(rec.data(), rec.size(), t.A, atoi(argv[3]), t.num_nodes - 1));
        const HostTree right = unpacked<FillRule>(rec, t.A, n);
        digest_replay<DigestRule>(right, got);
        printf(", \"digest\": [\"%016" PRIx64 "\", \"%016" PRIx64 "\"], \"unpacked_digest\": [\"%016" PRIx64 "\", \"%016" PRIx64 "\"]", want[0],
               want[1], got[0], got[1]);
        printf(", \"repacked_equal\": %s, \"tree_words\": [%d, %d, %d, %d]", pack_replay<ScanRule>(right) == rec ? "true" : "false",
               right.num_nodes, right.current_root, right.err, right.to_move);
        printf(", \"right\": {\"tails_canonical\": %s}", tails_canonical(right) ? "true" : "false");
        const HostTree whole = unpacked<WholePasses>(rec, t.A, n), kept = unpacked<KeptTail>(rec, t.A, n);
        printf(", \"whole_passes\": {\"tails_canonical\": %s, \"same_as_right\": %s}", tails_canonical(whole) ? "true" : "false",
               same_rows(whole, right) ? "true" : "false");
        printf(", \"kept_tail\": {\"tails_canonical\": %s, \"same_as_right\": %s}}\n", tails_canonical(kept) ? "true" : "false",
               same_rows(kept, right) ? "true" : "false");
        return 0;
    }
    fprintf(stderr, "usage: tree_load_driver rules | check <record> <A> <W> <N> | roundtrip <tree> <W> <record>\n");
    return 2;
}
