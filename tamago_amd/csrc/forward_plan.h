// Which forward kernel a launch gets, on which grid: pure functions of the launch's shape, the network's measured spreads, the
// launching thread's caps and the knobs' values (DESIGN.md 4.1 "How a launch is chosen" states the rules in this order).  No HIP,
// nothing from net_device.h: net_forward.hip reads the knobs in one place (forward_context) and looks up the instantiation a plan
// names, tg_net_kernel_name and tg_net_executed_flops_per_position render the same plan, tests/test_forward_plan_host.py
// compiles this alone.
#pragma once
#include <cstdlib>
#include <cstring>

namespace tg {
// Per-launch grid caps of the forward family, owned by the launching THREAD (search.hip's play_move_chain scopes them around the sub-group launches of one self-play move):
//   guard   > 0: the exact-fp32 kernel queued behind a split launch as its range guard takes at most this many workgroups.  Each
//                needs a CU to itself even to read a clear flag: with several streams sharing the device (self-play sub-groups) a
//                full-size guard launch waits for the other streams' forward passes to drain.  The rare real fallback is slower.
//   forward > 0: workgroups a forward launch may take (CUs left to other streams' tree kernels)
// (Round 6: these caps are a property of the LAUNCH, not of the network: a handle shared by group threads carries no such state.)
struct LaunchCaps { int guard = 0, forward = 0; };
LaunchCaps &launch_caps();               // net_forward.hip: the calling thread's
struct LaunchCapsScope {
    LaunchCaps saved;
    LaunchCapsScope(int guard, int forward) : saved(launch_caps()) { launch_caps() = LaunchCaps{guard, forward}; }
    ~LaunchCapsScope() { launch_caps() = saved; }
    LaunchCapsScope(const LaunchCapsScope &) = delete;
    LaunchCapsScope &operator=(const LaunchCapsScope &) = delete;
};
}  // namespace tg

namespace tg_fwd {

// TG_FWD_ALGO = w1d (the 9x9 default: Winograd F(2,3) along x on f16 x 2 operand pieces, net_forward_w1d.hip) | split16 (direct
// 3x3 convolution on f16 x 2 operand pieces, 3 MFMAs per product-sum) | w1dband (the 19x19 default: the one-axis tower, a board
// over two workgroups) | wino (exact fp32 Winograd tower, also the fallback behind the f16 range guard) | direct (exact fp32
// direct convolution).  Any other string: no f16 family and not `direct` - the exact Winograd rule.
enum class Algo { Unset, W1d, Split16, W1dBand, Wino, Direct, Other };
inline Algo parse_algo(const char *s) {
    if (!s) return Algo::Unset;
    if (!strcmp(s, "w1d")) return Algo::W1d;
    if (!strcmp(s, "split16")) return Algo::Split16;
    if (!strcmp(s, "w1dband")) return Algo::W1dBand;
    if (!strcmp(s, "wino")) return Algo::Wino;
    if (!strcmp(s, "direct")) return Algo::Direct;
    return Algo::Other;
}
inline int parse_int(const char *s, int unset) { return s ? atoi(s) : unset; }
// TG_FWD_BANDS: -1 unset; 0 / 2 / 4 force a band count; a negative number that WAS set counts as set (-2: the pair kernel is off,
// as for every set value, the band count automatic)
inline int parse_bands(const char *s) {
    if (!s) return -1;
    const int v = atoi(s);
    return v < 0 ? -2 : v;
}

// Every forward knob, as values (read in one place: net_forward.hip forward_context)
struct ForwardKnobs {
    Algo algo = Algo::Unset;         // TG_FWD_ALGO
    int bands = -1;                  // TG_FWD_BANDS (parse_bands)
    int group = 0;                   // TG_FWD_GROUP: 1 or 3 boards per workgroup of the 9x9 direct kernel (anything else: unset)
    int wino = 0;                    // TG_FWD_WINO: 81 / 82 / 83 or 1 / 2 / 3 boards per workgroup of the 9x9 Winograd kernel
    bool no_tail = false;            // TG_FWD_NO_TAIL: no second launch for a ragged tail
    bool spread_guard_off = false;   // TG_FWD_SPREAD_GUARD=0 (the precision ladder measures beyond the limits)
    int fwd_cus = 0;                 // TG_FWD_CUS: at most n workgroups for the split kernels (0: unset)
    int split_span = 0;              // TG_SPLIT_SPAN: 2 / 3 / 4 / 8 choose a span variant of the 9x9 three-board split kernel
    // tests and experiments: launch arguments, no part of the choice
    int band_mute = -1;              // TG_BAND_TEST_MUTE=b: band b of the banded kernel keeps its sequence number to itself
    bool pair_mute = false;          // TG_WB_TEST_MUTE: band 1 of the pair kernel does
    bool flag_memset = false;        // TG_FWD_FLAG_MEMSET: the memset node in front of a guarded launch back
};

struct PlanInputs {
    int S = 9;                       // board size
    int batch = 1;
    int num_cus = 256;
    double spread_w1d = 1.0, spread_split = 1.0;   // tg_net_channel_spread of the two weight images
    bool shared_device = false;      // TG_SHARED_DEVICE / tg_net_set_shared_device
    unsigned band_timeouts = 0;      // bounded waits of cross-workgroup kernels that gave up on this network so far
    tg::LaunchCaps caps;             // the launching thread's
};

// Load-time guard (ChannelSpread, net_weights.h): an f16 family is chosen only for a network whose tower layers keep their
// input channels within a measured spread of each other.  Otherwise the next safer kernel takes over - one-axis Winograd (w1d,
// pair) -> direct split -> exact fp32 - whatever TG_FWD_ALGO asks for: the contract (logits as close to fp64 as the reference's
// fp32 path, err < 4 err_ref + 1e-6) is not left silently.  DESIGN.md 4.1 "How far the channels of a layer may spread".
// The limits are read from profiles/forward_precision_ladder.json (tools/forward_precision_ladder.py on networks whose mid-block
// channels are rescaled over 2^S, every family against the fp64 forward, "guard": false), err_hip / bound per rung:
//   one-axis Winograd (low pieces unscaled): 2^8 (spread 357) is the last rung every launch meets, 0.59 at worst; 2^9 (spread 726)
//     the first that one does not (19x19 pair kernel 1.24; 9x9 from 2^10, 1.54), about x 2 per rung from there on.
//   direct split (low pieces x 2048): 2^19 (spread 5.3e5) the last, 0.62 at worst; 2^20 (spread 1.05e6) the first (19x19: 1.18).
// Each limit lies a factor 4 below the spread of the first rung that fails, rounded down to a power of two (the ladder draws
// its exponents at random): 726 / 4 -> 128, 1.05e6 / 4 -> 2^18.  make_state_dict networks measure 1.0 - 1.7.
constexpr double kSpreadLimitW1d = 128.0, kSpreadLimitSplit = 262144.0;

enum class Family { Direct, Wino, Split9, W1d9, Split13, Split19, Band19, Pair19 };
// why a launch did not get the f16 family it would have had (the caller says so once per process)
enum class Demoted { None, SpreadW1d, SpreadSplit, BandTimeouts };

// One launch's kernel, chosen ONCE per call: the kernel's name, the FLOP figure bench.py prices the matrix pipe with and the
// launch sequence are three switches over the same plan.
struct ForwardPlan {
    Family family;
    int S;
    int group;       // boards per workgroup
    int bands;       // Band19: 2 or 4 workgroups per board
    int tail;        // > 0: the last `tail` positions go out as a second launch; either launch has a plan of its own (head_of / tail_of)
    bool guarded;    // an f16 kernel, the exact-fp32 Winograd kernel <S, group> queued behind it as its range guard
    int grid;        // workgroups of the launch (tail > 0: of the head launch)
    int guard_grid;  // ... and of the guard launch behind it (0: none)
    int span;        // the split kernel's SPANQ
    Demoted demoted;
};

// exact direct kernel: FwdCfg<S, G>::WAVES_PER_SIMD (net_device.h, from the kernel's LDS bytes; net_forward.hip asserts the rows)
struct DirectRow { int S, group, waves_per_simd; };
constexpr DirectRow kDirectRows[] = {{9, 1, 2}, {9, 3, 2}, {13, 1, 2}, {19, 1, 1}};
constexpr int direct_waves_per_simd(int S, int group) {
    for (const DirectRow &r : kDirectRows)
        if (r.S == S && r.group == group) return r.waves_per_simd;
    return 0;
}

inline int min_int(int a, int b) { return a < b ? a : b; }
inline int capped(int n, int cap) { return cap > 0 && cap < n ? cap : n; }

inline ForwardPlan plan_forward(const PlanInputs &in, const ForwardKnobs &k) {
    const int S = in.S, batch = in.batch, cus = in.num_cus;
    ForwardPlan p{Family::Direct, S, 1, 0, 0, false, 0, 0, 6, Demoted::None};
    const auto groups = [&](int n) { return (n + p.group - 1) / p.group; };
    // 1. the load-time spread guard, asked in the order split -> one-axis; the first limit that is passed names the demotion
    const bool split_fits = in.spread_split <= kSpreadLimitSplit || k.spread_guard_off;
    const bool w1d_fits = (in.spread_split <= kSpreadLimitSplit && in.spread_w1d <= kSpreadLimitW1d) || k.spread_guard_off;
    // 2. an f16 family at all?  13x13 only when split16 is asked for by name, 9x9 and 19x19 unless an exact algorithm (or an
    // unknown one) is
    const bool f16_asked = S == 13 ? k.algo == Algo::Split16
                                   : (k.algo == Algo::Unset || k.algo == Algo::Split16 || k.algo == Algo::W1d || k.algo == Algo::W1dBand);
    if (f16_asked && !split_fits) p.demoted = Demoted::SpreadSplit;
    if (!f16_asked || !split_fits) {
        // 3. exact fp32.  Winograd: 19x19 always (global scratch), 9x9 with 1 / 2 / 3 boards per workgroup by launch size
        // (measured: B <= 256: 173 us, direct 194; B = 512: 308 / 347; B >= 768: 98 % vs 83 % of the fp32 MFMA peak); direct:
        // when asked for, and 13x13.  Direct 9x9: one board per workgroup fills more CUs, three above 2 x CUs (243 of 256 MFMA rows)
        int wino = 0;
        if (k.algo != Algo::Direct && S == 19) wino = 1;
        else if (k.algo != Algo::Direct && S == 9) {
            const int g = k.wino % 10;
            wino = g >= 1 && g <= 3 ? g : (batch <= cus ? 1 : (batch <= 2 * cus ? 2 : 3));
        }
        if (wino) {
            p.family = Family::Wino;
            p.group = wino;
            p.grid = min_int(groups(batch), cus);                  // (a launch of its own: no cap)
        } else {
            p.group = S != 9 ? 1 : (k.group == 1 || k.group == 3 ? k.group : (batch > 2 * cus ? 3 : 1));
            p.grid = min_int(groups(batch), cus * direct_waves_per_simd(S, p.group));
        }
        return p;
    }
    p.guarded = true;
    if (S == 13) p.family = Family::Split13;
    else if (S == 19) {
        // 4. 19x19.  The pair kernel needs both workgroups of a pair resident: not on a device shared with other processes, not
        // after a bounded wait gave up once - unless asked for by name.  The choice must NOT depend on the caps (a game must not
        // depend on how its boards were grouped: the pair and the direct kernels round differently); its GRID honours them.
        bool pair = k.algo == Algo::Unset || k.algo == Algo::W1dBand;
        if (pair && !w1d_fits) pair = false, p.demoted = Demoted::SpreadW1d;
        if (pair && k.algo == Algo::Unset) {
            if (k.bands != -1 || in.shared_device) pair = false;   // (TG_FWD_BANDS: the banded direct kernel was asked for by name)
            else if (in.band_timeouts > 0) pair = false, p.demoted = Demoted::BandTimeouts;
        }
        if (pair) {
            p.family = Family::Pair19;
            int pairs = min_int(batch, capped(cus, in.caps.forward) / 2);
            if (pairs >= 8) pairs &= ~7;                           // partners on the same XCD (consecutive workgroups go round the eight)
            p.grid = 2 * pairs;
        } else {
            // the banded direct kernel: every workgroup of a launch must be resident at once.  Off under a forward cap (CUs are
            // held back for other streams' kernels); unforced, off on a shared device and after a time-out; under a guard cap
            // (the sub-group streams of a self-play move are in flight exactly then) a launch takes a quarter of the CUs.
            const int forced = k.bands, room = in.caps.guard > 0 ? cus / 4 : cus;
            if (forced == 0 || in.caps.forward > 0 || (forced < 0 && (in.shared_device || in.band_timeouts > 0))) p.bands = 0;
            else if ((forced == 4 || forced < 0) && batch * 4 <= room) p.bands = 4;
            else if ((forced == 2 || forced == 4 || forced < 0) && batch * 2 <= room) p.bands = 2;
            p.family = p.bands ? Family::Band19 : Family::Split19;
        }
    } else {
        // 5. 9x9: three boards per workgroup for launches above the CU count, same bits; a ragged tail - up to one round of
        // one-board workgroups left over behind whole rounds of three-board ones - goes out as a second launch.  A round is
        // counted in the workgroups a launch may take (forward cap), for either family.
        const bool w1d = (k.algo == Algo::Unset || k.algo == Algo::W1d) && w1d_fits;
        if (!w1d && (k.algo == Algo::Unset || k.algo == Algo::W1d)) p.demoted = Demoted::SpreadW1d;
        p.family = w1d ? Family::W1d9 : Family::Split9;
        p.group = batch > cus ? 3 : 1;
        const int wgs = capped(cus, in.caps.forward), round = 3 * wgs, rem = batch % round;
        if (!k.no_tail && batch > round && rem > 0 && rem <= wgs) p.tail = rem;
    }
    // 6. grids.  One-axis 9x9: the forward cap; split kernels: TG_FWD_CUS only; banded: its workgroups; the guard launch: the guard cap
    const int n = groups(batch - p.tail);
    if (p.family == Family::W1d9) p.grid = capped(min_int(n, cus), in.caps.forward);
    else if (p.family == Family::Band19) p.grid = batch * p.bands;
    else if (p.family != Family::Pair19) p.grid = min_int(n, capped(cus, k.fwd_cus));
    if (p.family == Family::Split9 && p.group == 3 && (k.split_span == 2 || k.split_span == 3 || k.split_span == 4 || k.split_span == 8))
        p.span = k.split_span;
    p.guard_grid = capped(min_int(n, cus), in.caps.guard);
    return p;
}

// the two launches of a plan with a ragged tail
inline PlanInputs head_of(PlanInputs in, const ForwardPlan &p) { in.batch -= p.tail; return in; }
inline PlanInputs tail_of(PlanInputs in, const ForwardPlan &p) { in.batch = p.tail; return in; }

inline const char *kernel_name(const ForwardPlan &p) {
    switch (p.family) {
    case Family::Pair19: return "dualnet_fwd_w1dband_kernel + dualnet_heads19_kernel";
    case Family::Band19: return p.bands == 4 ? "dualnet_fwd_band_kernel<4>" : "dualnet_fwd_band_kernel<2>";
    case Family::Split19: return "dualnet_fwd_split_kernel<19, 1, f16x2>";
    case Family::Split13: return "dualnet_fwd_split_kernel<13, 1, f16x2> + dualnet_fwd_wino8_kernel<13, 1> (range guard, per board)";
    case Family::W1d9:
        if (p.tail > 0) return "dualnet_fwd_w1d_kernel<3> + dualnet_fwd_w1d_kernel<1> (ragged tail)";      // two launches: name both
        return p.group == 3 ? "dualnet_fwd_w1d_kernel<3>" : "dualnet_fwd_w1d_kernel<1>";
    case Family::Split9:
        if (p.tail > 0) return "dualnet_fwd_split_kernel<9, 3, f16x2> + dualnet_fwd_split_kernel<9, 1, f16x2> (ragged tail)";
        return p.group == 3 ? "dualnet_fwd_split_kernel<9, 3, f16x2>" : "dualnet_fwd_split_kernel<9, 1, f16x2>";
    case Family::Wino:
        if (p.S == 19) return "dualnet_fwd_wino8_kernel<19, 1, global scratch>";
        return p.group == 3 ? "dualnet_fwd_wino8_kernel<9, 3>" : (p.group == 2 ? "dualnet_fwd_wino8_kernel<9, 2>" : "dualnet_fwd_wino8_kernel<9, 1>");
    case Family::Direct:
        if (p.S != 9) return p.S == 19 ? "dualnet_fwd_kernel<19, 1>" : "dualnet_fwd_kernel<13, 1>";
        return p.group == 3 ? "dualnet_fwd_kernel<9, 3>" : "dualnet_fwd_kernel<9, 1>";
    }
    return "";
}

// What the matrix pipe executes per position: FLOPs of the MFMAs issued, the dense peak of their precision (TFLOP/s), the format
struct Executed { double flops, peak; const char *dtype; };
inline Executed executed(const PlanInputs &in, const ForwardKnobs &k) {
    const ForwardPlan p = plan_forward(in, k);
    if (p.tail > 0) {                                   // two launches: the positions' weighted mean
        Executed head = executed(head_of(in, p), k);
        const double rest = executed(tail_of(in, p), k).flops;
        head.flops = (head.flops * (in.batch - p.tail) + rest * p.tail) / in.batch;
        return head;
    }
    const int S = p.S, P = S * S, g = p.group;
    Executed e{0.0, 2500.0, "f16 (2 operand pieces, fp32 accumulate)"};
    switch (p.family) {
    case Family::Pair19:
        // per board and layer: 6 stages x 72 + 48 MFMAs per wave in either band (band 1's row-9 stage runs on the zero row); stem: 2 x 16 row tiles x 4 x 2 x 3
        e.flops = (12.0 * 4 * (480 + 480) + 2.0 * 16 * 4 * 2 * 3) * 16384.0;
        e.dtype = "f16 (2 operand pieces, Winograd F(2,3) along x, fp32 accumulate)";
        break;
    case Family::W1d9: {
        // per workgroup pass: stem as below + 12 layers x 4 waves x (three boards: 25 (row, tap) pairs | one board: 3 row tiles x 3
        // taps) x 4 channel tiles x 2 k-chunks x 3 products
        const int rtw = ((g * P + 15) / 16 + 3) / 4;
        e.flops = (2.0 * 4 * 4 * rtw * 3 + 12.0 * 4 * (g == 3 ? 25 : 9) * 4 * 2 * 3) * 16384.0 / g;
        e.dtype = "f16 (2 operand pieces, Winograd F(2,3) along x, fp32 accumulate)";
        break;
    }
    case Family::Split9: case Family::Split13: case Family::Split19: case Family::Band19: {
        // per workgroup pass: (2 stem + 12 * 18) k-chunks x (4 cout tiles x row tiles) x 3 products of
        // v_mfma_f32_16x16x32_f16 (16 384 FLOP each)
        const int row_tiles = S == 19 ? 24 : (S == 13 ? 12 : (g == 3 ? 16 : 6));   // 4 waves x 6 | 4 x 3 | 4 x 4 | 3 x 2
        e.flops = (2.0 + 12.0 * 18.0) * 4.0 * row_tiles * 3.0 * 16384.0 / g;
        break;
    }
    case Family::Wino: {
        // v_mfma_f32_16x16x4_f32 (2048 FLOP): per layer 16 points x 4 cout tiles x row tiles x 16 k-steps; stem direct
        const int tiles = g * ((S + 1) / 2) * ((S + 1) / 2), rt = (tiles + 15) / 16, mt = (g * P + 15) / 16;
        e = {(12.0 * 16 * 4 * rt * 16 + 9.0 * 2 * 4 * mt) * 2048.0 / g, 157.3, "f32"};
        break;
    }
    case Family::Direct: {
        const int mt = (g * P + 15) / 16;
        e = {(12.0 * 9 * 16 * 4 * mt + 9.0 * 2 * 4 * mt) * 2048.0 / g, 157.3, "f32"};
        break;
    }
    }
    return e;
}

}  // namespace tg_fwd
