// The random streams' bookkeeping, without a device: which generation launch is asked for (Piece), what a window holds and
// what its transitions make the caller do (WindowBook), when a request starts a new window (feed_rule), what the host knows
// of each tree's stream (StreamBook) and the two sizes a launch needs (scratch_pitch, snap_plan).  Indices, counts and flags
// only - csrc/search.hip (tg_search::Streams, tg_search::Windows) carries the answers out with HIP calls,
// tests/stream_windows_driver.cpp against a CPU model of the generation kernels.  Host code: the host compiler takes it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tg_streams {

constexpr int kMtN = 624, kSnapEvery = 32;       // (csrc/legacy_rng_device.h: words of a state block, blocks between snapshots)

// ---- what one generation launch is asked for (the fields of tg_rng::FillArgs that differ from launch to launch) ----
enum class Kind {
    Window,     // columns [first, first + count) of window buffer `buf`, rows of `pitch`
    Commit,     // nothing generated: the consumed draws are committed to the base state
    Noise,      // `count` Gumbel values per tree into the root noise rows; the base state moves behind them
};
struct Piece {
    Kind kind = Kind::Commit;
    int buf = 0;
    bool from_cont = false;         // go on behind the last piece (no lag is taken); else: from the base state, lag committed first
    int64_t pitch = 0, first = 0, count = 0;
};

// scratch row of a tree: the piece's words from word 0 of the block it starts in (<= 623 words in front, <= 623 behind)
inline int64_t scratch_pitch(int64_t count) { return 2 * count + 2 * kMtN; }

// State snapshots every kSnapEvery blocks of the whole window (few trees; no_snap: switched off): a later commit of the
// consumed draws starts from the nearest one.  `cap` snapshots per tree are allocated; grow: the launch needs `want` - the
// buffer is replaced, and with it EVERY tree's snapshot count is cleared (NEEDED: the growing launch itself commits the lag of
// the window before it, and would start from a snapshot that is no longer there).
struct SnapPlan {
    bool on;
    int want;
    bool grow;
};
inline SnapPlan snap_plan(int T, bool no_snap, const Piece &p, int64_t cap) {
    if (T > 64 || no_snap) return {false, 0, false};
    const int64_t window = p.kind == Kind::Noise ? 0 : std::max(p.pitch, p.count);
    const int want = (int)((2 * window / kMtN + 2) / kSnapEvery + 1);
    return {true, want, want > cap};
}

// ---- the streams the host seeded, per tree: seeded at all, seed not uploaded yet (dirty), draws consumed since the
// device state was last brought up to date (lag) ----
class StreamBook {
public:
    static constexpr int kNoneSeeded = -2;
    void create(int T) { if (st_.empty()) st_.resize((size_t)T); }
    int trees() const { return (int)st_.size(); }
    void seed(int t) { st_[t] = One{true, true, 0}; }
    bool seeded(int t) const { return t >= 0 && t < trees() && st_[t].seeded; }
    bool unused(int t) const { return st_[t].dirty && st_[t].lag == 0; }      // never used since it was seeded: the seed IS the state
    // the lag a generation launch from the base state commits; skip: the tree takes no part, its lag stays here
    int64_t take_lag(int t, bool skip) {
        const int64_t lag = skip ? 0 : st_[t].lag;
        if (!skip) st_[t].lag = 0;
        return lag;
    }
    void add_consumed(int t, int64_t draws, bool skip) { if (!skip) st_[t].lag += draws; }
    // The next run [*t0, *t1) of consecutive dirty trees at or behind `from`, marked clean: one upload each, and the snapshot
    // counts of exactly these trees are cleared (they belonged to the old streams).  That clear is DEFENSIVE: a fresh seed has
    // no lag, so its first launch reads no snapshot, and a window rewrites every snapshot a commit of its own consumption
    // can select - no legal order shows a stale one.  false: none left.
    bool next_dirty_run(int from, int *t0, int *t1) {
        const int T = trees();
        while (from < T && !st_[from].dirty) ++from;
        if (from >= T) return false;
        *t0 = from;
        for (; from < T && st_[from].dirty; ++from) st_[from].dirty = false;
        *t1 = from;
        return true;
    }
    // -1: every tree of the T (skip[t] != 0: not looked at) is seeded; kNoneSeeded: no tree ever was; else the first that is not
    int first_unseeded(int T, const uint8_t *skip) const {
        if (trees() != T) return kNoneSeeded;
        for (int t = 0; t < T; ++t)
            if (!(skip && skip[t]) && !st_[t].seeded) return t;
        return -1;
    }

private:
    struct One {
        bool seeded = false, dirty = false;
        int64_t lag = 0;
    };
    std::vector<One> st_;
};

// ---- when a request starts a new window ----
// The next window of `need` draws per tree, unless the one in place still covers the request (`left`) and `force` is off.
// first > 0: in parts - the first `first` draws of every row now, the rest by WindowBook::extend / complete_rest.
// Few trees (a single search tree): a window of `need` draws is a bound - a mini-batch consumes a fraction of it - and every
// regeneration costs the launch that waits for it ~25 us.  Generate `overgen` windows' worth instead: the first `need`
// draws now, the rest behind the first launch that uses them (deferred to the install), and the following mini-batches
// find their draws there.  The draws are the stream's, whatever the window they were generated in.
// (one tree, ms per move at 9x9 / 19x19 with state snapshots: x2 1.475 / 10.94, x3 1.483 / 10.92, x4 1.464 / 10.91, x8 1.595 / 10.97)
constexpr int kOvergenMaxTrees = 16, kOvergenDefault = 2;
constexpr int64_t kOvergenMinNeed = 2048, kOvergenMaxNeed = (int64_t)1 << 20;
struct Feed {
    bool start;
    int64_t pitch, cols, eager;     // WindowBook::start's arguments
};
inline Feed feed_rule(int T, int64_t need, bool force, int64_t first, int64_t left, int overgen) {
    if (need == 0 || (!force && left >= need)) return {false, 0, 0, 0};
    int64_t eager = 0;
    if (first == 0 && T <= kOvergenMaxTrees && need >= kOvergenMinNeed && need <= kOvergenMaxNeed) {
        eager = first = need;
        need *= overgen;
    }
    return {true, need, first > 0 && first < need ? first : need, eager};
}

// ---- what a transition of the window book makes its caller do, in this order ----
struct Action {
    enum What {
        Generate,       // launch `piece` (the buffer first grown to its pitch), record the buffer's event, then generated(piece)
        Wait,           // the launch stream waits for buffer `buf`'s event
        Publish,        // the kernels read buffer `buf` with `pitch` draws per tree from now on
        ResetCursors,   // both device cursors go back to 0, on the launch stream
    } what;
    Piece piece;
    int buf;
    int64_t pitch;
};
struct Actions {
    Action a[5];
    int n = 0;
    void add(Action::What what, int buf, int64_t pitch = 0, const Piece &piece = Piece{}) { a[n++] = Action{what, piece, buf, pitch}; }
    const Action *begin() const { return a; }
    const Action *end() const { return a + n; }
};

// The window state and its transitions.  A window is [T][pitch] draws, filled on the generation stream - generated from the
// library's streams (start) or copied from the host (accept) - into the buffer no launch reads.  It is PENDING until a
// selection launch installs it (install: the launch's stream waits for the buffer's event, the kernels get buffer and
// pitch, both cursors go back to 0), ACTIVE from then on, and replaced by the next install.
// A generated window may be IN PARTS: columns [0, done) are there, `todo` more are to come (self-play: the window of a
// move's phases is 1.7 MB at 16 boards; a chained PUCT search: one window for all its mini-batches) - piece by piece,
// each waited for by the launch that needs it (extend), the rest in one go (complete_rest: the next install waits).  Few
// trees: a whole-window request is over-generated (feed_rule) and the rest DEFERRED to the install, behind the wait of the
// launch that only needs the first part.
// THE INVARIANT: every piece goes on from the generator state the piece before it left (the continuation state), and every
// generation launch from the base state that is no noise draw rewrites that state.  So while todo > 0 the continuation
// state is this window's: whoever launches from the base state - a new window, the commit of a state read, the noise
// (which moves the base state under the continuation's block count) - first completes the rest or drops it (settle /
// complete_rest / abandon / start).  The launcher asks refuses(piece) and launches nothing from the base state while todo > 0.
// Consumption: the device cursors count from the install; `used` is each tree's cursor at the last record(), `left` the
// tail of `cap` no tree has read - what a later request may still be served from (0: abandoned, the next feed starts a
// new window).
class WindowBook {
public:
    void create(int T) { T_ = T; }
    bool refuses(const Piece &p) const { return !p.from_cont && todo_ > 0; }
    // Start a window of `pitch` draws per tree: columns [0, cols) now; cols < pitch: in parts.  eager > 0: the whole-window
    // request an over-generated window serves - its rest is deferred to the install, and eager_due() asks for the next one
    // ahead of that request.  Precondition: settle() - no installed window has columns to come.  A deferred rest still open
    // belongs to a window that was never installed, whose buffer this window takes: it is dropped.
    Actions start(int64_t pitch, int64_t cols, int64_t eager) {
        Actions acts;
        drop_deferred();
        starting_eager_ = eager;
        acts.add(Action::Generate, 1 - active_, 0, Piece{Kind::Window, 1 - active_, false, pitch, 0, cols});   // never the window a running kernel may read
        return acts;
    }
    // A Generate action's launch went out: the window it starts is the pending one; a continued piece's columns are there.
    void generated(const Piece &p) {
        if (p.kind != Kind::Window) return;
        if (p.from_cont) {
            todo_ -= p.count;
            done_ += p.count;
            return;
        }
        pending_ = part_buf_ = p.buf;
        pending_pitch_ = cap_ = left_ = p.pitch;
        used_.assign((size_t)T_, 0);
        done_ = p.count;
        todo_ = p.pitch - p.count;
        eager_ = starting_eager_;
        deferred_ = eager_ > 0 && todo_ > 0;
    }
    // The columns up to `upto` (clamped to the window) of the window in parts, and the launch stream waits for them.  The
    // device cursor of a tree never passes the columns its launched selections may consume, so a launch only needs the
    // pieces up to its own.  Precondition: none (nothing to do without a window in parts, or with the columns there already).
    Actions extend(int64_t upto) {
        Actions acts;
        upto = std::min(upto, done_ + todo_);
        if (!todo_ || upto <= done_) return acts;
        acts.add(Action::Generate, part_buf_, 0, piece(upto));
        acts.add(Action::Wait, part_buf_);
        return acts;
    }
    // Complete the rest, deferred or not; the next selection launch waits for it.  Precondition: none.
    Actions complete_rest() {
        Actions acts;
        deferred_ = false;
        if (!todo_) return acts;
        wait_rest_ = true;
        acts.add(Action::Generate, part_buf_, 0, piece(done_ + todo_));
        return acts;
    }
    // What a request that may be served from the window in place does: a rest that is not deferred is completed - a
    // launch may be reading the window.  Precondition: none.
    Actions settle() { return deferred_ ? Actions{} : complete_rest(); }
    // Install ahead of a selection launch: the newest window becomes the active one.  Precondition: none (without a
    // pending window only the wait for a completed rest is left to do).
    Actions install() {
        Actions acts;
        if (pending_ < 0) {
            if (wait_rest_) acts.add(Action::Wait, active_);              // second part of the ACTIVE window
            wait_rest_ = false;
            return acts;
        }
        active_ = pending_;
        active_pitch_ = pending_pitch_;
        pending_ = -1;
        wait_rest_ = false;
        acts.add(Action::Wait, active_);                                  // (every piece filled so far, a completed rest included)
        acts.add(Action::Publish, active_, active_pitch_);
        acts.add(Action::ResetCursors, active_);
        if (deferred_)                                                    // (the over-generated rest, behind this launch's wait)
            for (const Action &a : complete_rest()) acts.a[acts.n++] = a;
        return acts;
    }
    // Record consumption: cursor[t] is tree t's device cursor, delta[t] becomes the draws since the last record.  Returns
    // the first tree (skip[t] != 0: not looked at) whose cursor went back or past the window - nothing is recorded
    // then -, -1 otherwise.  Precondition: cursors of the active window.
    int record(const int64_t *cursor, const uint8_t *skip, int T, int64_t *delta) {
        if (used_.size() != (size_t)T) used_.assign((size_t)T, 0);
        for (int t = 0; t < T; ++t) {
            delta[t] = cursor[t] - used_[t];                   // the device cursor is cumulative within a window
            if (!(skip && skip[t]) && (delta[t] < 0 || cursor[t] > cap_)) return t;
        }
        used_.assign(cursor, cursor + T);
        left_ = cap_ - (T > 0 ? *std::max_element(cursor, cursor + T) : 0);
        return -1;
    }
    // Abandon: the streams leave the window (a reseed, the noise, the debug walk) - no later request is served from it, the
    // next feed starts a new one.  A deferred rest is dropped: its window was never installed, no launch reads those
    // columns, and every driver feeds before its next selection.  Precondition: settle() where a launch from the base
    // state follows (the noise).
    void abandon() {
        left_ = 0;
        drop_deferred();
    }
    // Accept a host-uploaded window of `count` draws per tree, copied into free_buffer(), as the pending one.  It takes the
    // buffer of a generated window that was never installed: that one's deferred rest is dropped.
    int free_buffer() const { return 1 - active_; }
    void accept(int64_t count) {
        drop_deferred();
        pending_ = free_buffer();
        pending_pitch_ = count;
    }

    bool in_parts() const { return todo_ > 0; }                    // was the last window split (and not completed yet)
    int active() const { return active_; }                         // (its event: what the active window's second part is behind)
    int64_t capacity() const { return cap_; }                      // (for messages)
    int64_t left() const { return left_; }
    // Few trees: the request to regenerate ahead for now - when the next mini-batch will not find its draws in this window,
    // the next one is generated under the forward pass and backup that are running (not with trees left out: self-play)
    int64_t eager_due(bool skipping) const { return !skipping && left_ < eager_ ? eager_ : 0; }
    // the buffer and pitch a reader of the newest window sees: the pending one, else the active one
    int newest(int64_t *pitch) const {
        *pitch = pending_ >= 0 ? pending_pitch_ : active_pitch_;
        return pending_ >= 0 ? pending_ : active_;
    }

private:
    Piece piece(int64_t upto) const { return Piece{Kind::Window, part_buf_, true, done_ + todo_, done_, upto - done_}; }   // columns [done, upto)
    void drop_deferred() {
        if (deferred_) { todo_ = 0; deferred_ = false; }
    }
    int T_ = 0;
    int active_ = 0, pending_ = -1;
    int64_t active_pitch_ = 0, pending_pitch_ = 0;
    int part_buf_ = 0;                        // the window in parts: its buffer, columns there, columns to come
    int64_t done_ = 0, todo_ = 0;
    bool deferred_ = false;                   // ... and its rest goes out at the install
    bool wait_rest_ = false;                  // the active window's rest was completed: the next selection launch waits
    int64_t eager_ = 0, starting_eager_ = 0;
    int64_t cap_ = 0, left_ = 0;
    std::vector<int64_t> used_;
};

}  // namespace tg_streams
