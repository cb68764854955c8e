// The read-out records of the device search: what travels device -> host packed into one copy, stated once (DESIGN.md 3
// "Read-out records").  No HIP and nothing from search.hip: tests/test_readout_host.py compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "node_pool.h"

namespace tg_readout {

// ---- sticky error flags of a tree (SearchDev::err, the `err` word of every record; bits 8 and up: the site, for debugging) ----
enum : int32_t { kErrPoolFull = 1, kErrRngEmpty = 2, kErrPipeline = 4, kErrReroot = 8, kErrOccupied = 16 };

// the message of a tree whose flag word is set ("" for 0: nothing to report)
inline std::string error_text(int tree, int32_t err) {
    if (!err) return "";
    char buf[256];
    snprintf(buf, sizeof(buf), "tree %d: %s%s%s%s(err 0x%x)", tree, (err & kErrPoolFull) ? "node pool full " : "",
             (err & kErrRngEmpty) ? "random window exhausted " : (err & kErrPipeline) ? "selection pipeline stalled or path too deep " : "",
             (err & kErrReroot) ? "new root beyond the tree's nodes " : "",
             (err & kErrOccupied) ? "root advanced onto a point that is not empty " : "", (unsigned)err);
    return buf;
}

// ---- a record: head words (int32), then per-child rows of A elements in their list's order - first the int32 rows, then
// (8-byte aligned) the float64 rows.  -> where row `id` starts (N: where the rows end) ----
struct Row {
    const char *name;
    size_t elem_bytes;
};
constexpr size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }
template <size_t N>
constexpr size_t row_offset(const Row (&rows)[N], int head_words, int id, size_t A) {
    size_t at = (size_t)head_words * 4;
    for (int wide = 0; wide < 2; ++wide) {
        if (wide) at = align8(at);
        for (int k = 0; k < (int)N; ++k) {
            if ((rows[k].elem_bytes == 8) != (wide == 1)) continue;
            if (k == id) return at;
            at += A * rows[k].elem_bytes;
        }
    }
    return at;
}
#define TG_READOUT_ROW(name, E, ...) {#name, sizeof(E)},

}  // namespace tg_readout

// Root record, one per tree (gather_roots_kernel / finish_roots_kernel write it through write_root_record;
// parse_root_records reads it: tg_search_read_root_stats, tg_search_read_roots, every self-play move).
// X(row, element type, SearchDev member it copies from the root's children); the host's destination is <row>_host.
#define TG_ROOT_RECORD_ROWS(X)          \
    X(visits, int32_t, ch_visits)       \
    X(virtual_loss, int32_t, ch_vl)     \
    X(action, int32_t, action)          \
    X(value_sum, double, ch_vsum)       \
    X(policy, double, ch_policy)

// Analysis record, one per tree (read_analysis_kernel writes, tg_search_read_analysis reads): the rows, then
// pv[A][max_depth] (int16, padded to 8 bytes).  X(row, element type); the host's destination is <row>_host.
#define TG_ANALYSIS_RECORD_ROWS(X) \
    X(action, int32_t)             \
    X(visits, int32_t)             \
    X(pv_len, int32_t)             \
    X(resume, int32_t)             \
    X(value_sum, double)           \
    X(policy, double)

// Self-play (finish_roots_kernel, the move decided on the device): behind the T root records, one RootTail per tree.  (At
// global scope, where finish_roots_kernel's signature has always named it: the kernel's symbol stays what it was.)
struct RootTail {
    int32_t best, kind, pos, pad;           // chosen root child, tg_readout::MoveKind, its point (0 = pass; -1: idle)
    int64_t cursor, pad2;                   // the tree's draw cursor behind the phases
};
static_assert(sizeof(RootTail) == 32, "the tail keeps the 8-byte alignment of what follows the root records");

// Best-move record, one per tree (best_moves_kernel writes, tg_search_best_moves hands the [T] array to the caller as it is:
// include/tamago_hip.h restates the layout as tg_best_move): the last four lines of search_best_move (mcts/tree.py:76-77,
// :87-105) - what a PUCT match driver needs of a root, in place of the root record's seven rows.
struct BestMove {
    int32_t num_children;                   // of the root (0: the tree took no part, see status)
    int32_t move;                           // padded coordinate, 0 = PASS, -1 = RESIGN
    int32_t best;                           // the chosen root child: first maximum of the visits (0 for a one-child root)
    int32_t visits;                         // ... its visits
    double value_sum;                       // ... its value sum
    int32_t node_visits;                    // the root's own visits
    int32_t status;                         // tg_readout::BestStatus bits
};
static_assert(sizeof(BestMove) == 32, "32 bytes per tree, value_sum 8-byte aligned");

// Advance record, one per tree (advance_kernel and advance_nodes_kernel write, tg_search_advance hands the [T] array to the
// caller as it is: include/tamago_hip.h restates the layout as tg_advance_record): what became of a tree whose root was
// advanced by a move.
struct AdvanceRec {
    int32_t kept_visits;                    // node_visits of the new root; -1: the tree is fresh (or was left alone, see status)
    int32_t kept_nodes;                     // nodes of the kept subtree (0 for a fresh tree)
    int32_t num_children;                   // of the new root (0 for a fresh tree: its expansion will say)
    int32_t status;                         // tg_readout::AdvanceStatus bits
};
static_assert(sizeof(AdvanceRec) == 16, "16 bytes per tree");

namespace tg_readout {

// AdvanceRec::status: 0 = the move was played.  kAdvanceLeftAlone: the caller's move was -1, nothing read, nothing played;
// kAdvanceOccupied: the move's point is not empty - nothing played, the tree's sticky error word set
enum AdvanceStatus : int32_t { kAdvanceLeftAlone = 1, kAdvanceOccupied = 2 };

// BestMove::status: 0 = decided.  kBestSatOut: the caller's sit_out flag was set, nothing read, nothing played;
// kBestNoRoot: the root is not expanded (nothing played); kBestTreeError: the tree's sticky error word is set
enum BestStatus : int32_t { kBestSatOut = 1, kBestNoRoot = 2, kBestTreeError = 4 };

enum RootHead : int { kRootChildren, kRootVisits, kRootRawBits, kRootErr, kRootHeadWords };
constexpr Row kRootRows[] = {TG_ROOT_RECORD_ROWS(TG_READOUT_ROW)};
#define TG_ROOT_ID(name, E, member) kRoot_##name,
enum RootRow : int { TG_ROOT_RECORD_ROWS(TG_ROOT_ID) kRootNumRows };
#undef TG_ROOT_ID
constexpr size_t root_record_offset(int id, size_t A) { return row_offset(kRootRows, kRootHeadWords, id, A); }
constexpr size_t root_record_bytes(size_t A) { return root_record_offset(kRootNumRows, A); }

// the tails' place, what RootTail::kind says
enum MoveKind : int32_t { kMove = 0, kResign = 1, kSecondPass = 2, kMoveLimit = 3, kIdle = 4 };
constexpr size_t root_tail_offset(size_t T, size_t A, size_t t = 0) { return T * root_record_bytes(A) + t * sizeof(RootTail); }
constexpr size_t root_records_bytes(size_t T, size_t A) { return root_tail_offset(T, A, T); }
// ... and what the host tells it about each board: state [T][kStateWords]
enum StateWord : int { kStateFlags, kStatePasses, kStatePlayed, kStateWords = 4 };     // flags; passes in a row; moves played; 0
enum StateFlag : int32_t { kStateIdle = 1, kStateNeverResign = 2 };                    // takes no part (parked / just started)

enum AnaHead : int { kAnaChildren, kAnaVisits, kAnaVsumBits, kAnaErr, kAnaHeadWords };
constexpr int kAnaWaves = 4;                 // root children per workgroup of read_analysis_kernel
constexpr int kAnaMaxDepth = 1024;
constexpr Row kAnaRows[] = {TG_ANALYSIS_RECORD_ROWS(TG_READOUT_ROW)};
#define TG_ANA_ID(name, E) kAna_##name,
enum AnaRow : int { TG_ANALYSIS_RECORD_ROWS(TG_ANA_ID) kAnaNumRows };
#undef TG_ANA_ID
constexpr size_t analysis_record_offset(int id, size_t A) { return row_offset(kAnaRows, kAnaHeadWords, id, A); }
constexpr size_t analysis_pv_offset(size_t A) { return align8(analysis_record_offset(kAnaNumRows, A)); }
constexpr size_t analysis_record_bytes(size_t A, size_t max_depth) { return analysis_pv_offset(A) + align8(2 * A * max_depth); }
#undef TG_READOUT_ROW

}  // namespace tg_readout
