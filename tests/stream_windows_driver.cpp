// Stand-alone driver of csrc/stream_windows.h for tests/test_stream_windows_host.py (host compiler, no HIP): the stream book,
// the window book and the feed rule, carried out against a CPU model of what the two generation kernels do to the generator
// state (restated from rng_words_kernel / rng_draws_kernel of csrc/legacy_rng_device.h; the twist is csrc/legacy_stream.h's).
// A window holds the 53-bit INTEGERS of its draws (random_sample() * 2^53, exact) - no logarithm.  A script of driver-level
// operations comes in on stdin, one per line; out go every draw a tree consumed ("draws tree value..."), every state read
// ("state tree pos hash") and every refusal ("refused").  Nothing here knows what the draws should be: the test holds them
// against numpy.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../tamago_amd/csrc/legacy_stream.h"
#include "../tamago_amd/csrc/stream_windows.h"

using namespace tg_streams;

static const uint64_t kNotThere = ~0ull;             // a column that was never generated, or that the launch stream did not wait for

static uint32_t temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    return y ^ (y >> 18);
}

// ---- the device: generator states, snapshots, the two window buffers, the cursors ----
struct Device {
    int T = 0, A = 0;
    std::vector<tg::Mt19937> base, cont;             // numpy's lazy convention: pos 624 = "twist before the next word"
    std::vector<long long> cont_blk;
    std::vector<int> snap_n;
    std::vector<uint32_t> snap;                      // [T][snap_cap][624]
    int64_t snap_cap = 0;
    std::vector<uint64_t> buf[2];
    int64_t filled[2] = {0, 0}, waited[2] = {0, 0};  // columns behind each buffer's event; of those, what the launch stream waited for
    int rng = 0;                                     // what the kernels read: buffer, pitch, cursors
    int64_t rng_cap = 0;
    std::vector<int64_t> cursor;

    // rng_words_kernel + rng_draws_kernel for tree t; noise_out: the Gumbel mode's draws
    void launch(const Piece &p, int t, long long lag, bool snaps, std::vector<uint64_t> *noise_out) {
        const bool noise = p.kind == Kind::Noise;
        tg::Mt19937 m = p.from_cont ? cont[t] : base[t];
        int pos = m.pos;
        const long long abs0 = p.from_cont ? cont_blk[t] : 0;
        int n_snap = snaps ? snap_n[t] : 0;
        if (p.from_cont) lag = 0;
        if (lag > 0) {                                               // commit what the searches consumed: base moves
            const long long end = pos + 2 * lag, be = (end - 1) / kMtN;
            long long at = 0;
            if (snaps) {
                const long long k = std::min<long long>(be / kSnapEvery, n_snap);
                if (k > 0) {
                    std::memcpy(m.key, &snap[((size_t)t * snap_cap + (size_t)(k - 1)) * kMtN], sizeof(m.key));
                    at = k * kSnapEvery;
                }
            }
            for (; at < be; ++at) m.regenerate();
            pos = (int)(end - kMtN * be);
            m.pos = pos;
            base[t] = m;
            n_snap = 0;
        }
        const long long end = pos + 2 * p.count, n_blocks = p.count > 0 ? (end - 1) / kMtN + 1 : 0;
        std::vector<uint32_t> words((size_t)(n_blocks * kMtN));
        for (long long b = 0; b < n_blocks; ++b) {
            if (b > 0) {
                m.regenerate();
                const long long abs_b = abs0 + b, idx = abs_b / kSnapEvery - 1;
                if (snaps && !noise && abs_b % kSnapEvery == 0 && idx < snap_cap) {
                    std::memcpy(&snap[((size_t)t * snap_cap + (size_t)idx) * kMtN], m.key, sizeof(m.key));
                    n_snap = std::max(n_snap, (int)(idx + 1));
                }
            }
            for (int i = 0; i < kMtN; ++i) words[(size_t)(kMtN * b + i)] = temper(m.key[i]);
        }
        m.pos = p.count > 0 ? (int)(end - kMtN * (n_blocks - 1)) : pos;
        (noise ? base : cont)[t] = m;
        if (noise) n_snap = 0;
        if (snaps) snap_n[t] = n_snap;
        if (!noise) cont_blk[t] = abs0 + (n_blocks > 0 ? n_blocks - 1 : 0);
        for (long long j = 0; j < p.count; ++j) {
            const uint32_t *w = &words[(size_t)(pos + 2 * j)];
            const uint64_t bits = ((uint64_t)(w[0] >> 5) << 26) | (uint64_t)(w[1] >> 6);
            if (noise) noise_out->push_back(bits);
            else buf[p.buf][(size_t)(t * p.pitch + p.first + j)] = bits;
        }
    }
};

static void print_draws(int t, const std::vector<uint64_t> &v) {
    printf("draws %d", t);
    for (uint64_t x : v) printf(" %" PRIu64, x);
    printf("\n");
}

// ---- the host side, as csrc/search.hip's tg_search::Streams and tg_search::Windows carry the books out ----
struct Host {
    Device dev;
    StreamBook streams;
    WindowBook windows;
    std::vector<tg::Mt19937> seeds;
    int overgen = kOvergenDefault;
    bool no_snap = false, state_completes = true;

    void create(int T, int A) {
        dev.T = T, dev.A = A;
        tg::Mt19937 zero;
        std::memset(zero.key, 0, sizeof(zero.key));
        dev.base.assign(T, zero), dev.cont.assign(T, zero), seeds.assign(T, zero);
        dev.cont_blk.assign(T, 0), dev.snap_n.assign(T, 0), dev.cursor.assign(T, 0);
        windows.create(T);
    }
    void seed(int t, const tg::Mt19937 &m) {
        streams.create(dev.T);
        seeds[t] = m;
        streams.seed(t);
        windows.abandon();
    }
    // tg_search::Streams::generate.  false: refused
    bool generate(const Piece &p, const uint8_t *skip) {
        const int T = dev.T;
        for (int t0, t1 = 0; streams.next_dirty_run(t1, &t0, &t1);)
            for (int t = t0; t < t1; ++t) dev.base[t] = seeds[t], dev.snap_n[t] = 0;
        std::vector<long long> lag(T, 0);
        if (!p.from_cont)
            for (int t = 0; t < T; ++t) lag[t] = streams.take_lag(t, skip && skip[t]);
        if (windows.refuses(p)) {
            printf("refused\n");
            return false;
        }
        const SnapPlan snaps = snap_plan(T, no_snap, p, dev.snap_cap);
        if (snaps.on && snaps.grow) {
            dev.snap.assign((size_t)T * snaps.want * kMtN, 0xdeadbeefu);      // (a new allocation: whatever was there is gone)
            dev.snap_cap = snaps.want;
            std::fill(dev.snap_n.begin(), dev.snap_n.end(), 0);
        }
        std::vector<uint64_t> noise;
        for (int t = 0; t < T; ++t) {
            if (p.kind == Kind::Noise && skip && skip[t]) continue;
            noise.clear();
            dev.launch(p, t, lag[t], snaps.on, &noise);
            if (p.kind == Kind::Noise) print_draws(t, noise);
        }
        return true;
    }
    // tg_search::Windows::carry_out
    bool carry_out(const Actions &acts) {
        for (const Action &a : acts) {
            switch (a.what) {
            case Action::Generate:
                if (dev.buf[a.buf].size() < (size_t)(dev.T * a.piece.pitch) || !a.piece.from_cont) {
                    dev.buf[a.buf].assign((size_t)(dev.T * a.piece.pitch), kNotThere);
                    dev.filled[a.buf] = dev.waited[a.buf] = 0;
                }
                if (!generate(a.piece, nullptr)) return false;
                dev.filled[a.buf] = a.piece.first + a.piece.count;
                windows.generated(a.piece);
                break;
            case Action::Wait: dev.waited[a.buf] = dev.filled[a.buf]; break;
            case Action::Publish: dev.rng = a.buf, dev.rng_cap = a.pitch; break;
            case Action::ResetCursors: std::fill(dev.cursor.begin(), dev.cursor.end(), 0); break;
            }
        }
        return true;
    }
    // feed_streams_impl
    bool feed(int64_t need, bool force, int64_t first) {
        if (!carry_out(windows.settle())) return false;
        const Feed f = feed_rule(dev.T, need, force, first, windows.left(), overgen);
        return !f.start || carry_out(windows.start(f.pitch, f.cols, f.eager));
    }
    // a selection launch: tree t reads n[t] draws at its cursor
    void select(const std::vector<int64_t> &n) {
        std::vector<uint64_t> got;
        for (int t = 0; t < dev.T; ++t) {
            got.clear();
            for (int64_t j = 0; j < n[t]; ++j) {
                const int64_t c = dev.cursor[t]++;
                const bool there = c < dev.rng_cap && c < dev.waited[dev.rng];
                got.push_back(there ? dev.buf[dev.rng][(size_t)(t * dev.rng_cap + c)] : kNotThere);
            }
            if (n[t] > 0) print_draws(t, got);
        }
    }
    // advance_streams_impl
    bool collect(const uint8_t *skip) {
        std::vector<int64_t> delta(dev.T);
        const int bad = windows.record(dev.cursor.data(), skip, dev.T, delta.data());
        if (bad >= 0) {
            printf("bad_cursor %d\n", bad);
            return false;
        }
        for (int t = 0; t < dev.T; ++t) streams.add_consumed(t, delta[t], skip && skip[t]);
        const int64_t need = windows.eager_due(skip != nullptr);
        return !need || feed(need, false, 0);
    }
    // draw_noise_impl
    bool noise(const uint8_t *skip) {
        if (!carry_out(windows.settle())) return false;
        windows.abandon();
        Piece p;
        p.kind = Kind::Noise;
        p.count = dev.A;
        return generate(p, skip);
    }
    // tg_search_stream_state
    bool state(int t) {
        tg::Mt19937 m = seeds[t];
        if (!streams.unused(t)) {
            if (state_completes && !carry_out(windows.complete_rest())) return false;
            if (!generate(Piece{}, nullptr)) return false;
            m = dev.base[t];
        }
        uint64_t h = 1469598103934665603ull;                             // FNV-1a over the key's words
        for (uint32_t w : m.key) h = (h ^ w) * 1099511628211ull;
        printf("state %d %d %" PRIu64 "\n", t, m.pos, h);
        return true;
    }
    // tg_search_set_rng: row t of the host's window holds marker + t * count + column
    void accept(int64_t count, uint64_t marker) {
        const int b = windows.free_buffer();
        dev.buf[b].assign((size_t)(dev.T * count), 0);
        for (size_t i = 0; i < dev.buf[b].size(); ++i) dev.buf[b][i] = marker + i;
        dev.filled[b] = count, dev.waited[b] = 0;
        windows.accept(count);
    }
};

int main() {
    Host h;
    char line[16384];
    std::vector<uint8_t> skip;
    // the rest of the line as one number per tree; "-": none (a null skip pointer)
    auto per_tree = [&](char *rest, std::vector<int64_t> *out) {
        out->clear();
        for (char *tok = std::strtok(rest, " \n"); tok; tok = std::strtok(nullptr, " \n")) {
            if (!std::strcmp(tok, "-")) return false;
            out->push_back(std::strtoll(tok, nullptr, 10));
        }
        return true;
    };
    auto skip_of = [&](char *rest) -> const uint8_t * {
        std::vector<int64_t> v;
        if (!per_tree(rest, &v)) return nullptr;
        skip.assign(v.begin(), v.end());
        return skip.data();
    };
    while (std::fgets(line, sizeof line, stdin)) {
        char op[32];
        int at = 0;
        if (std::sscanf(line, "%31s%n", op, &at) != 1) continue;
        char *rest = line + at;
        const std::string o = op;
        long long a = 0, b = 0, c = 0;
        bool ok = true;
        if (o == "case") {                                   // a new handle: case T A overgen no_snap state_completes
            int T, A, og, ns, sc;
            std::sscanf(rest, "%d %d %d %d %d", &T, &A, &og, &ns, &sc);
            h = Host{};
            h.create(T, A);
            h.overgen = og, h.no_snap = ns != 0, h.state_completes = sc != 0;
            printf("%s", line);
        } else if (o == "seed") {                            // seed tree pos word...: numpy's get_state() layout
            std::vector<int64_t> v;
            per_tree(rest, &v);
            tg::Mt19937 m;
            for (int i = 0; i < kMtN; ++i) m.key[i] = (uint32_t)v[(size_t)i + 2];
            m.pos = (int)v[1];
            h.seed((int)v[0], m);
        } else if (o == "feed") {
            std::sscanf(rest, "%lld %lld %lld", &a, &b, &c);
            ok = h.feed(a, b != 0, c);
        } else if (o == "extend") {
            std::sscanf(rest, "%lld", &a);
            ok = h.carry_out(h.windows.extend(a));
        } else if (o == "complete") {
            ok = h.carry_out(h.windows.complete_rest());
        } else if (o == "install") {
            ok = h.carry_out(h.windows.install());
        } else if (o == "select") {
            std::vector<int64_t> n;
            per_tree(rest, &n);
            h.select(n);
        } else if (o == "collect") {
            ok = h.collect(skip_of(rest));
        } else if (o == "noise") {
            ok = h.noise(skip_of(rest));
        } else if (o == "state") {
            std::sscanf(rest, "%lld", &a);
            ok = h.state((int)a);
        } else if (o == "accept") {
            std::sscanf(rest, "%lld %lld", &a, &b);
            h.accept(a, (uint64_t)b);
        } else {
            fprintf(stderr, "unknown operation: %s", line);
            return 2;
        }
        if (!ok) printf("failed %s\n", op);
    }
    return 0;
}
