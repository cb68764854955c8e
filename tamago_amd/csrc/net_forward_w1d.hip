// DualNet forward for gfx950: the residual tower as Winograd F(2,3) along ONE axis on split operands (round 4; its own file
// since round 5 - the 2-D Winograd tower it grew out of is in the git history: commit 04640d1, tools/experiments/kernels/).
//
// net_forward_split.hip runs the fp32 3x3 convolutions on the 16-bit matrix pipe as three f16 products per fp32 product
// (a = ah + al, w = wh + wl:  a w ~ ah wh + ah wl + al wh) and is bound by the MFMA count (857 per wave and layer for three
// boards); 2-D Winograd F(2x2,3x3) issues 480 but 5.3 VALU instructions beside each and is bound by instruction issue.
// Transforming along x only sits between: 600 MFMAs per wave and layer, one transform pass per side - 1.3 VALU instructions
// per MFMA, inside what an MFMA's 16 cycles hide.  Shared with the kernels of this family:
//   * V = B^T d is computed in fp32 (one add per value, exact inputs) and split AFTERWARDS into two f16 pieces; the weights
//     U = G g are computed in fp64 on the host with the batch-norm scale folded in, scaled by a power of two per layer and
//     split there.  Logit error against the reference's fp64 forward: the class of the reference's own fp32 path.
//   * the LOW pieces are kept UNSCALED (al = rn16(a - ah), no 2^11): v_mfma_f32_16x16x32_f16 keeps f16 subnormals, so the
//     cross terms have the right magnitude by themselves and ONE accumulator set takes all three products.
//   * wave w of the four owns transform POINT w: its weight fragments of a layer stay in registers (AGPRs, requested by
//     inline asm with explicit waits - tests/test_isa_waits.py checks the emitted code), the sum over the points goes
//     through a 32 KB LDS exchange, wave w' finishes output channels [16 w', 16 w' + 16).
//   * activations stay in LDS as fp32 [position][64 channels] (block input X - also the residual - and the intermediate
//     H), 16-byte chunk index XOR-swizzled by a function of the position under which the reads of sixteen units are
//     conflict-free for every cell.
// Stem (6 -> 64 channels) and heads are the direct split kernel's (im2col'ed K = 64 product; 1x1 convolutions and policy
// FC on the 16-bit pipe), reading / writing the fp32 images.  f16 range guard as there: |V| <= 2 |d| must stay below 65504,
// so an input plane value, a stem or a layer output beyond 16000 - or a policy 1x1-convolution feature beyond kHeadRangeLimit -
// raises the flag and the group's bit, and the exact-fp32 kernel redoes the marked groups.
// Reference: nn/network/res_block.py:8-38, nn/network/dual_net.py:41-52.
#include "w1d_common.h"

// W1_ABL (experiments only, tools/experiments/wb_ablation.sh: results are wrong, the timing says what a class of riders costs in the
// three-board variant): 1 no weight requests, 2 no input transforms, 4 no cell reads, 8 no epilogue arithmetic, 16 no exchange
// traffic, 32 no row barrier, 128 no MFMAs, 256 no heads, 512 no stem
#ifndef W1_ABL
#define W1_ABL 0
#endif

namespace {


template <int G>
struct WsCfg {
    static constexpr int S = 9, P = 81, A = 82, M = G * P;
    static constexpr int MT = (M + 15) / 16;              // row tiles of 16 positions (stem, heads)
    static constexpr int NT = G * 25;                     // Winograd tiles (5 x 5 per board)
    static constexpr int NRT = (NT + 15) / 16;            // row tiles of 16 Winograd tiles
    static constexpr int NTHR = 256, NW = 4;
    // activation buffers: fp32 [row][16 x 16 B]; row M = dump row (stores of positions outside the board), row M + 1 =
    // zero row (patch cells outside the board, 256-byte aligned: a read keeps the bank of its natural address)
    static constexpr int ROWS = M + 2;
    static constexpr int BUF = ROWS * 256;
    static constexpr int DUMP_REL = M * 256, ZERO_REL = (M + 1) * 256;
    static constexpr int X_OFF = 0, H_OFF = BUF;
    static constexpr int EX_OFF = 2 * BUF;                // exchange: [wave 4][z 2][ct 4][lane 64][16 B]
    static constexpr int EX_BYTES = 32768;
    // head tables, staged once per workgroup
    static constexpr int HD1_OFF = EX_OFF + EX_BYTES;     // 1x1 fragment image 4 KB + table 128 B
    static constexpr int HB_OFF = HD1_OFF + 4096 + 128;   // policy FC bias [A] (padded to 84)
    static constexpr int VW_OFF = HB_OFF + 84 * 4;        // value FC weights [3][P] + bias [3] (padded)
    static constexpr int LDS_BYTES = VW_OFF + ((3 * P + 3 + 3) & ~3) * 4;
    // stem overlay (over H and the exchange): im2col'ed input as f16-pair images [piece 2][kc 2][row][64 B] + planes
    static constexpr int ZOFF = ((M + 1) * 64 + 255) & ~255;
    static constexpr int IMG = ZOFF + 256;
    static constexpr int SI_OFF = H_OFF;
    static constexpr int STAGE = SI_OFF + 4 * IMG;
    static constexpr int RTW = (MT + NW - 1) / NW;        // stem: row tiles per wave
    // planes, staged as split words (f16 high piece | scaled low piece << 16), one 11 x 11 image per board and plane: the
    // board with a border of zero words, so that a tap outside the board reads a zero operand without a test
    static constexpr int PW = 11 * 11;
    static constexpr int SS_OFF = (STAGE + G * 6 * PW * 4 + 15) & ~15;  // stem batch-norm scale [64] + shift [64] (w1d kernel)
    // head overlay (over H): policy features as f16 pairs 12 KB, scratch
    static constexpr int HQ_OFF = H_OFF;
    static constexpr int AUX = H_OFF + 12288;
    static_assert(SS_OFF + 512 <= EX_OFF + EX_BYTES, "stem overlay");
    static_assert(AUX + G * (P + 96 + 4) * 4 <= H_OFF + M * 256, "head overlay");
    static_assert(LDS_BYTES <= 163840, "LDS");
};

// 16-byte chunk XOR of activation row R (position 81 b + 9 y + x), spread over chunk-index bits 0, 2, 3 (bit 1 is the one in
// which the two lane groups of a ds_read_b128 cycle differ).  The kernel's sixteen MFMA columns are the units
// u = 5 board + t (outputs x = 2t, 2t + 1 of ONE board row); a unit's cells x = 2t - 1 .. 2t + 2 have (x + 1) / 2 = t or t + 1,
// so g = (5 board + (x + 1) / 2) mod 8 is distinct over the eight units of either half of a ds_read_b128 cycle
__host__ __device__ inline int w1_swz(int R) {
    const int b = R >= 162 ? 2 : (R >= 81 ? 1 : 0);
    const int p = R - 81 * b, y = (p * 57) >> 9, x = p - 9 * y;
    const int g = (5 * b + ((x + 1) >> 1)) & 7;
    return (g & 1) | ((g & 6) << 1);
}

// ... one board per workgroup (units u = 5 (row mod 3) + t): g = ((x + 1) / 2 + 5 (y mod 3)) mod 8
__host__ __device__ inline int w1g1_swz(int R) {
    const int y = (R * 57) >> 9, x = R - 9 * y;
    const int g = (((x + 1) >> 1) + 5 * (y % 3)) & 7;
    return (g & 1) | ((g & 6) << 1);
}

// e / 81 and e / 40 of a staging element index (e < 1792) as a multiply and a shift, as (p * 57) >> 9 is p / 9 of a cell
__host__ __device__ constexpr int w1_div81(int e) { return (e * 1619) >> 17; }
__host__ __device__ constexpr int w1_div40(int e) { return (e * 1639) >> 16; }
constexpr bool w1_div_ok() {
    for (int e = 0; e < 1792; ++e)
        if (w1_div81(e) != e / 81 || w1_div40(e) != e / 40) return false;
    return true;
}
static_assert(w1_div_ok(), "staging: element index -> plane image");

// Request schedule of the three-board variant (round 5).  A wave's 48 fragments of a layer are 48 KB; four waves' requests
// pass through the CU's vector L1 at 64 B per clock, i.e. 16 clocks - one MFMA - per request and wave.  Round 4 issued 32 of
// the 48 inside row 8 (768 clocks of MFMAs, 2 048 of L1): row 8 took 2 200 - 2 700 ticks, row 0 and row 1 waited for what
// was still in flight.  A fragment can only be requested once its register is free, so the schedule follows the uses:
//   kind 0: tap 1 of the next layer -> the spare slot S1N (free all layer): rows 1 - 6, 3 / 3 / 3 / 3 / 2 / 2
//   kind 1: tap 2, k-chunk 1 of the next layer -> its OTHER buffer (ua[2][1] for even layers, the VGPR fragments ux for odd
//           ones: double-buffered since round 5, 32 VGPRs): rows 5 - 6, in the order the next layer's row 0 uses them
//   kind 2: tap 2, k-chunk 0 of the next layer -> ua[2][0], freed by row 7's last MFMAs: row 7 from slice 53, row 8's first
//   kind 3: tap 0 of the next layer -> ua[0], freed by row 8's first 24 MFMAs: row 8 from slice 13 (12 fragments)
//   kind 4: tap 0 / k-chunk 1 / high pieces of THIS layer (the four fragments row 8 of the previous layer freed last): row 0
// -> -1, or 16 kind + fragment (8 kc + 4 piece + ct).  Issue order = wait order (w1_wait_* below).
constexpr int w1_sched(int y, int m) {
    if (y >= 1 && y <= 4 && (m == 46 || m == 52 || m == 58)) return 3 * (y - 1) + (m - 46) / 6;
    if ((y == 5 || y == 6) && (m == 46 || m == 52)) return 12 + 2 * (y - 5) + (m - 46) / 6;
    if ((y == 5 || y == 6) && (m == 49 || m == 55 || m == 61 || m == 67)) {
        const int i = 4 * (y - 5) + (m - 49) / 6;              // 0 .. 3: low pieces (used first), 4 .. 7: high pieces
        return 16 + (i < 4 ? 12 + i : 8 + (i - 4));
    }
    if (y == 7 && m >= 53 && m <= 69 && (m - 53) % 4 == 0) { const int i = (m - 53) / 4; return 32 + (i < 4 ? 4 + i : 0); }
    if (y == 8 && (m == 1 || m == 5 || m == 9)) return 32 + 1 + (m - 1) / 4;
    if (y == 8 && m >= 13 && m <= 46 && (m - 13) % 3 == 0) {
        const int i = (m - 13) / 3;                            // 0 .. 11: (kc 0, low), (kc 0, high), (kc 1, low)
        return 48 + (i < 4 ? 4 + i : (i < 8 ? i - 4 : 12 + (i - 8)));
    }
    if (y == 0 && (m == 1 || m == 4 || m == 7 || m == 10)) return 64 + 8 + (m - 1) / 3;
    return -1;
}
// Requests behind the last one a wait is for (in issue order): the layer top needs tap 1 (last: row 6, slice 52), row 0's
// slice 24 needs tap 2 (last: row 8, slice 9), row 1 needs tap 0 (last: row 0, slice 10: nothing behind it)
constexpr int w1_count_from(int y0, int m0) {                  // scheduled requests strictly behind (y0, m0), up to the end of row 8
    int n = 0;
    for (int y = y0; y <= 8; ++y)
        for (int m = (y == y0 ? m0 + 1 : 0); m < 72; ++m)
            if (y != 0 && w1_sched(y, m) >= 0) ++n;
    return n;
}
constexpr int kW1WaitTop = w1_count_from(6, 52);               // 23: tap 1 has arrived
constexpr int kW1WaitTap2 = w1_count_from(8, 9) + 2 + 4;       // 18: + the layer's shift and scale, + row 0's four requests
static_assert(kW1WaitTop == 23 && kW1WaitTap2 == 18, "request schedule and wait counts");

// Rider placement of the three-board variant: which slice of output row y carries what, besides its MFMA and the weight
// requests above (those keep their slices; the riders go around them).  An MFMA holds the SIMD's vector issue for 8 of its
// 16 cycles and issue costs add (a VALU instruction 4): two VALU instructions or two LDS instructions beside an MFMA cost
// next to nothing, every further one is paid in full - so the riders are cut into steps of two and spread over the row
// (tools/slice_costs.py prints the emitted slices).  Row y carries
//   * the exchange + epilogue of row y - 1 (w1_epi_at, the same slices in every row): 2-5 exchange writes (an accumulator
//     is written six MFMAs before its store reads it: no hazard padding), 11 barrier, 12-15 exchange reads, 16-17 residual
//     reads, 19-38 sums / shift / residual / ReLU two instructions at a time (layers without a residual: 19-34), 39 / 41
//     range guard of the two cells, 40 / 42 their stores;
//   * the eight cell reads of input row y + 3 (w1_rd_at): rows 1-7 in 0-1, 6, 16-18 (16 and 17 beside the residual reads)
//     and 43-44 - none in the four slices ahead of the barrier, whose wait is for every LDS operation of the wave; rows 0
//     and 8 (48 slices) beside the exchange traffic;
//   * the input transform of V row y + 3 from those cells, twenty steps of two instructions (w1_tr_at): rows 1-7 in the
//     row's tail, from slice 45, in the slices without a weight request; row 0 in 18-23, every other slice of 24-42 and
//     43-47; row 8 from slice 18 in the slices without a request, beside the arithmetic.
// Rows 6, 7 and 8 read and transform the NEXT layer's rows 0, 1 and 2 (this layer's output rows 0 - 2, complete since
// row 3).  V slots (vslot: row 0 -> 4, row r -> r & 3) - the slot a row's transform writes must have lost its last reader,
// tap 0 of the output row behind its previous holder:
//   row 0 -> V row 3, slot 3 (held V row 7 of the previous layer: last read by its row 8, tap 0)      free all of row 0
//   row y = 1 .. 5 -> V row y + 3, slot (y + 3) & 3 (held V row y - 1: last read by row y, slices 0-23)  free from slice 24
//   row 6 -> next V row 0, slot 4 (held V row 0: last read by row 1)                                  free
//   row 7 -> next V row 1, slot 1 (held V row 5: last read by row 6, tap 0)                           free all of row 7
//   row 8 -> next V row 2, slot 2 (held V row 6: last read by row 7, tap 0)                           free all of row 8
// Store-to-read pairs across waves: a cell read of input row r is at least four row barriers behind the store of that row
// (output row r of the previous layer is stored under its row r + 1, row 8 under this layer's row 0, read under row 5;
// rows 6 - 8 read output rows 0 - 2, stored under rows 1 - 3), and the next store into a cell that was read is at least
// four rows ahead - so a cell read may sit in front of its row's barrier.  The exchange reads stay behind it.
constexpr int kW1TrSteps = 20;
enum : int {
    kEpiWrite = 0, kEpiBarrier = 4, kEpiRead = 5, kEpiRes = 9, kEpiArith = 11, kEpiArithSlices = 20,
    kEpiGuard0 = 31, kEpiStore0 = 32, kEpiGuard1 = 33, kEpiStore1 = 34
};
constexpr int w1_epi_at(int m) {
    if (m >= 2 && m < 6) return kEpiWrite + (m - 2);
    if (m == 11) return kEpiBarrier;
    if (m >= 12 && m < 16) return kEpiRead + (m - 12);
    if (m == 16 || m == 17) return kEpiRes + (m - 16);
    if (m >= 19 && m < 19 + kEpiArithSlices) return kEpiArith + (m - 19);
    if (m >= 39 && m < 43) return kEpiGuard0 + (m - 39);
    return -1;
}
constexpr int w1_rd_at(int y, int m) {
    constexpr int at[3][8] = {{0, 6, 12, 13, 14, 15, 16, 17}, {0, 1, 6, 16, 17, 18, 43, 44}, {0, 2, 3, 6, 12, 14, 15, 17}};
    const int k = y == 0 ? 0 : (y == 8 ? 2 : 1);
    for (int i = 0; i < 8; ++i)
        if (at[k][i] == m) return i;
    return -1;
}
constexpr bool w1_tr_slice(int y, int m) {
    if (w1_sched(y, m) >= 0) return false;
    if (y == 0) return m >= 18 && !(m >= 24 && m < 43 && !(m & 1));
    return m >= (y == 8 ? 18 : 45);
}
constexpr int w1_tr_at(int y, int m) {
    if (!w1_tr_slice(y, m)) return -1;
    int n = 0;
    for (int k = 0; k < m; ++k)
        if (w1_tr_slice(y, k)) ++n;
    return n < kW1TrSteps ? n : -1;
}
constexpr bool w1_place_ok() {
    for (int y = 0; y <= 8; ++y) {
        const int nm = (y == 0 || y == 8) ? 48 : 72;
        int reads = 0, steps = 0, first_step = nm;
        for (int m = 0; m < nm; ++m) {
            if (w1_rd_at(y, m) >= 0) {
                if (w1_sched(y, m) >= 0 || w1_rd_at(y, m) != reads) return false;     // no request in a read's slice; in order
                ++reads;
            }
            if (w1_tr_at(y, m) >= 0) {
                if (w1_tr_at(y, m) != steps) return false;
                if (steps == 0) first_step = m;
                ++steps;
            }
            if (y >= 1 && y <= 7 && w1_sched(y, m) >= 0 && w1_epi_at(m) >= 0) return false;
        }
        if (reads != 8 || steps != kW1TrSteps) return false;
        // transform group j (steps 5 j ..) needs reads 2 j, 2 j + 1: at least two slices ahead
        for (int m = 0; m < nm; ++m)
            for (int k = 0; k < m + 2 && k < nm; ++k)
                if (w1_rd_at(y, m) >= 0 && w1_tr_at(y, k) >= 0 && w1_tr_at(y, k) / 5 == w1_rd_at(y, m) / 2) return false;
        // no LDS read may still be on its way at the row barrier's wait (slice 11): none in the four slices ahead of it
        for (int m = 7; m < 11; ++m)
            if (w1_rd_at(y, m) >= 0) return false;
        if (y >= 1 && y <= 5 && first_step < 24) return false;                        // the slot is free from slice 24
    }
    return true;
}
static_assert(w1_place_ok(), "rider placement: eight reads and twenty transform steps a row, around the weight requests");

// Heads on the 16-bit matrix pipe (as split_common.h: run_heads_mfma), reading the block output from the fp32 image X:
// a B fragment (position li of a 16-row tile, channels 32 kc + 8 lg ..) is two 16-byte reads + the operand split.
template <int G, typename C, int SWZ>
__device__ __forceinline__ void run_heads_x32(unsigned char *smem, const NetDev &net, int b0, int batch, int want_logits,
                                              float *__restrict__ policy, float *__restrict__ value, int tid, int wave,
                                              long long *tl, int *overflow, int *group_bits, int grp) {
    constexpr int P = C::P, A = C::A, M = C::M, NTHR = C::NTHR;
    constexpr int NW = NTHR / 64, NT = 6, KS = 6, NTW = (NT + NW - 1) / NW;
    using F = FmtF16;
    asm volatile("" : "+v"(tid));
    __builtin_assume(tid >= 0 && tid < NTHR);                  // (an asm result: without this the strided loops below stay loops)
    const int lane = tid & 63, li = lane & 15, lg = lane >> 4;
    auto stamp = [&](int i) { if (tl && tid == 0) tl[i] = (long long)__builtin_amdgcn_s_memtime(); };
    // (__shfl_xor derives its addresses from a lane id that hipcc computes once per kernel and keeps in scratch)
    auto lane_xor = [&](float v, int o) {
        return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, __builtin_bit_cast(int, v)));
    };
    float *hval = reinterpret_cast<float *>(smem + C::AUX);   // [G][P]
    float *plog = hval + G * P;                               // [G][NT * 16]
    float *vlog = plog + G * NT * 16;                         // [G][4]
    const float down2 = net.pfc_tab[0], down2x = down2 * (1.f / 2048.f);   // (requested here: behind the barrier its L2 round trip is exposed)
    i32x4v fw[NTW][KS][2];
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
        const int nt = wave + u * NW;
        const unsigned char *base = net.pfc_img + (size_t)(nt < NT ? nt : 0) * KS * 2048 + lane * 16;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int p = 0; p < 2; ++p) gmem_load_frag(fw[u][s][p], base, (s * 2 + p) * 1024);
    }
    // the K padding of the feature image (columns 2P .. 191 of boards < G, both pieces: the stem overlay dirtied it) as whole
    // dwords: sixteen threads a (piece, board) row, fifteen dwords each
    static_assert((2 * P) % 2 == 0 && (192 - 2 * P) == 30 && NTHR >= 128, "feature padding as dwords");
    if (tid < 128 && (tid & 15) < 15 && ((tid >> 4) & 3) < G)
        *reinterpret_cast<unsigned *>(smem + C::HQ_OFF + ((tid >> 6) * 16 + ((tid >> 4) & 3)) * 384 + 2 * P * 2 + (tid & 15) * 4) = 0u;
    i32x4v ha[2][2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
        for (int p = 0; p < 2; ++p) lds_load_frag<0>(ha[kc][p], smem, C::HD1_OFF + (kc * 2 + p) * 1024 + lane * 16);
    const f32x4 ini = *reinterpret_cast<const f32x4 *>(smem + C::HD1_OFF + 4096 + lg * 16);
    const float down1 = *reinterpret_cast<const float *>(smem + C::HD1_OFF + 4096 + 64), down1x = down1 * (1.f / 2048.f);
    constexpr int TPW = (C::MT + NW - 1) / NW;
    i32x4v fb[TPW][2][2];                                  // [tile][piece][kc]
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int t = wave + q * NW;
        const int row = (t < C::MT ? t : wave) * 16 + li;
        const int rr = row < M ? row : M + 1;              // zero row
        const int sw = row < M ? (SWZ == 2 ? w1g1_swz(row) : w1_swz(row)) : 0;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            const int a0 = C::X_OFF + rr * 256 + (((kc * 8 + lg * 2) ^ sw) << 4);
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(smem + a0);
            const f32x4 v1 = *reinterpret_cast<const f32x4 *>(smem + (a0 ^ 16));
            uint2 p0[2], p1[2];
            split4<F>(v0, p0);
            split4<F>(v1, p1);
            fb[q][0][kc] = i32x4v{(int)p0[0].x, (int)p0[0].y, (int)p1[0].x, (int)p1[0].y};
            fb[q][1][kc] = i32x4v{(int)p0[1].x, (int)p0[1].y, (int)p1[1].x, (int)p1[1].y};
        }
    }
    float hv[TPW][3];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        f32x4 a0 = ini, a1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            a0 = mfma16<F>(ha[kc][0], fb[q][0][kc], a0);
            a1 = mfma16<F>(ha[kc][1], fb[q][0][kc], a1);
            a1 = mfma16<F>(ha[kc][0], fb[q][1][kc], a1);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) hv[q][j] = fmaxf(fmaf(a1[j], down1x, a0[j] * down1), 0.f);
    }
    // the lanes lg == 0 hold the three head channels of their position: ONE exec-mask region for all of a wave's tiles
    // (a tile beyond the last is wave-uniform; a row beyond the group's positions - the last tile only - goes to row 15 of
    // the feature image, a board that is never read into a kept output column, and to spare words behind the logits)
    static_assert(C::AUX + G * (P + 96 + 4) * 4 + 16 * 4 <= C::H_OFF + M * 256, "head overlay: dump words");
    if (lg == 0) {
        _Float16 *hq = reinterpret_cast<_Float16 *>(smem + C::HQ_OFF);
        bool hot = false;                                      // a policy feature of the group whose high f16 piece would not be finite
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            const int t = wave + q * NW;
            if (t < C::MT) {
                const int row = t * 16 + li;
                const int bl = (row >= P ? 1 : 0) + (row >= 2 * P ? 1 : 0);
                const bool in = row < M;
                hot |= in && !(fmaxf(hv[q][0], hv[q][1]) < kHeadRangeLimit);
                const int fo = in ? bl * 192 + (row - bl * P) : 15 * 192 + li;          // feature (j = 0): [board][k]
                const int vo = in ? row : G * (P + 96 + 4) + li;                        // hval[bl * P + pp] = hval[row]
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const _Float16 h = (_Float16)hv[q][j];
                    const _Float16 l = (_Float16)((hv[q][j] - (float)h) * 2048.f);
                    hq[fo + j * P] = h;
                    hq[16 * 192 + fo + j * P] = l;
                }
                hval[vo] = hv[q][2];
            }
        }
        // the head phase's f16 range guard: the tower's amax never sees these 64-term sums
        if (hot) raise_range_flag(overflow, group_bits, grp);
    }
    stamp(0);
    __syncthreads();
    stamp(1);
    // the feature fragments (the same for every output tile of the wave): all twelve requested before the first MFMA - one LDS
    // round trip exposed, not six (the tower's weight registers are dead here)
    i32x4v fh[KS], fl[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int off = C::HQ_OFF + (li * 192 + s * 32 + lg * 8) * 2;
        lds_load_frag<0>(fh[s], smem, off);
        lds_load_frag<16 * 192 * 2>(fl[s], smem, off);
    }
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
        const int nt = wave + u * NW;
        if (nt < NT) {
            // (logit slots A .. 95 of a board's row exist and are never read: no guard on the last tile; the bias words behind
            // A are the ticket and the value FC's table - finite or not, they only reach those slots)
            static_assert(C::HB_OFF + NT * 16 * 4 <= C::LDS_BYTES, "policy FC: the bias words of the last tile are inside LDS");
            static_assert(NT * 16 >= A && C::AUX + (G * P + G * NT * 16 + G * 4) * 4 <= C::H_OFF + M * 256,
                          "policy FC: a board's logit row holds every slot of the last tile");
            float bias[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bias[j] = reinterpret_cast<const float *>(smem + C::HB_OFF)[nt * 16 + lg * 4 + j];
            f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                a0 = mfma16<F>(fw[u][s][0], fh[s], a0);
                a1 = mfma16<F>(fw[u][s][1], fh[s], a1);
                a1 = mfma16<F>(fw[u][s][0], fl[s], a1);
            }
            if (li < G) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    plog[li * NT * 16 + nt * 16 + lg * 4 + j] = fmaf(a1[j], down2x, a0[j] * down2) + bias[j];
            }
        }
    }
    static_assert(G * 3 <= NTHR / 16, "value FC: sixteen lanes an output");
    if (const int o = tid >> 4; o < G * 3) {
        const int part = tid & 15, bl = (o >= 3 ? 1 : 0) + (o >= 6 ? 1 : 0), c = o - bl * 3;
        const float *h = hval + bl * P;
        const float *wv = reinterpret_cast<const float *>(smem + C::VW_OFF) + c * P;
        float sv = 0.f;
#pragma unroll
        for (int i = 0; i < (P + 15) / 16; ++i) {
            const int j = part + i * 16;
            if (j < P) sv = fmaf(h[j], wv[j], sv);
        }
        sv += lane_xor(sv, 8);
        sv += lane_xor(sv, 4);
        sv += lane_xor(sv, 2);
        sv += lane_xor(sv, 1);
        if (part == 0) vlog[bl * 4 + c] = sv + reinterpret_cast<const float *>(smem + C::VW_OFF)[3 * P + c];
    }
    stamp(2);
    __syncthreads();
    for (int bl = wave; bl < G; bl += NW) {
        const int b = b0 + bl;
        if (b >= batch) continue;
        const float l0 = plog[bl * NT * 16 + lane];
        const float l1 = lane + 64 < A ? plog[bl * NT * 16 + lane + 64] : -INFINITY;
        float m = fmaxf(l0, l1);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, lane_xor(m, o));
        const float e0 = expf(l0 - m), e1 = lane + 64 < A ? expf(l1 - m) : 0.f;
        float sum = e0 + e1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += lane_xor(sum, o);
        const float inv = 1.f / sum;
        __builtin_nontemporal_store(want_logits ? l0 : e0 * inv, &policy[(size_t)b * A + lane]);
        if (lane + 64 < A) __builtin_nontemporal_store(want_logits ? l1 : e1 * inv, &policy[(size_t)b * A + lane + 64]);
        if (lane < 3) {
            const float v0 = vlog[bl * 4], v1 = vlog[bl * 4 + 1], v2 = vlog[bl * 4 + 2];
            const float vm = fmaxf(v0, fmaxf(v1, v2));
            const float x0 = expf(v0 - vm), x1 = expf(v1 - vm), x2 = expf(v2 - vm);
            const float es = x0 + x1 + x2;
            const float mine = lane == 0 ? x0 : (lane == 1 ? x1 : x2);
            value[(size_t)b * 3 + lane] = mine / es;
        }
    }
}

// The 9x9 tower as Winograd F(2,3) along x only (the 9x9 default; TG_FWD_ALGO=w1d): 600 MFMAs per wave and layer for three
// boards (2-D Winograd: 480, direct: 857), one transform pass per side.  G = 3 boards per workgroup for throughput launches,
// G = 1 for launches up to the CU count - same bits either way.
// PROF: s_memtime stamps of workgroup 0 / wave 0: [0] group start, [1] input staged, [2] stem done, [3..14] layer done, [15] heads done, [64..66] inside the heads: 1x1 convolutions done, barrier passed, FCs done
template <int G, bool PROF>
__global__ __launch_bounds__(256, 1) void dualnet_fwd_w1d_kernel(
    NetDev net, const float *__restrict__ planes, int batch, int want_logits,
    float *__restrict__ policy, float *__restrict__ value, int *__restrict__ overflow, int *__restrict__ group_bits) {
    using C = WsCfg<G>;
    using F = FmtF16;
    constexpr int P = C::P, M = C::M, NTHR = C::NTHR, RTW = C::RTW, IMG = C::IMG;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;

    if (static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char *)smem)) != 0u)
        __builtin_trap();                                      // absolute LDS addressing below
    // ---- once per workgroup: zero + dump rows, head tables ----
    for (int e = tid; e < 2 * 2 * 64; e += NTHR) {             // rows M, M + 1 of X and H
        const int buf = e >> 7, r = (e >> 6) & 1, c = e & 63;
        reinterpret_cast<float *>(smem + buf * C::BUF + (M + r) * 256)[c] = 0.f;
    }
    for (int e = tid; e < C::A; e += NTHR) reinterpret_cast<float *>(smem + C::HB_OFF)[e] = net.pfc_b[e];
    for (int e = tid; e < 3 * P + 3; e += NTHR)
        reinterpret_cast<float *>(smem + C::VW_OFF)[e] = e < 3 * P ? net.vfc_w[e] : net.vfc_b[e - 3 * P];
    stage_head_tables<C, NTHR>(smem, net, tid);

    int stamp_i = 0;
    auto stamp = [&]() {
        if constexpr (PROF)
            if (blockIdx.x == 0 && wave == 0 && stamp_i < 40 && fresh_lane() == 0) net.timeline[stamp_i++] = (long long)__builtin_amdgcn_s_memtime();
    };
    int ovf = 0;
    const int n_groups = (batch + G - 1) / G;
    constexpr int NPL = (G * 6 * P + NTHR - 1) / NTHR;
    float pre[NPL];
    float ssv;                                                 // the stem's batch-norm scale (threads 0 .. 63) / shift (64 .. 127): travels with the planes
    auto fetch_planes = [&](int grp2) __attribute__((always_inline)) {
        const int ft = wave * 64 + fresh_lane();
        ssv = ft < 64 ? net.sscale[ft] : (ft < 128 ? net.shift[ft - 64] : 0.f);
        // (the group's boards inside the batch are a prefix of its elements: one wave-uniform limit, no division per element)
        const int left = batch - grp2 * G;
        const int lim = grp2 < n_groups ? (left < G ? left : G) * 6 * P : 0;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const int e = ft + i * NTHR;
            pre[i] = e < lim ? __builtin_nontemporal_load(&planes[(size_t)grp2 * G * 6 * P + e]) : 0.f;
        }
    };
    fetch_planes(blockIdx.x);
    const float sgn = wave == 1 ? 1.f : -1.f;                  // row pass of point row w: d[ra] + sgn d[rb]
    static_assert(G == 3 || G == 1, "dualnet_fwd_w1d_kernel: one or three boards per workgroup");
    // This wave's weight fragments of a layer, [slot 4][kc 2][piece 2][ct 4]: slots 0 / 2 = taps ky 0 / 2, slots 1 and 3 take
    // tap 1 of even / odd layers in turn (the spare one is filled for the next layer while this one runs).  AGPRs, requested
    // by inline asm (see the kernel above): explicit waits, in-order returns.
    i32x4v ua[4][2][2][4];
    const int wlane = lane * 16;
    {
        const unsigned char *w0 = net.w1_w + (size_t)wave * 49152;
        w1_request_tap<1>(ua, w0 + 16384, wlane);
        if constexpr (G == 3) {
            // (the order the first layer waits for them in - that of the steady-state schedule w1_sched: tap 2 with k-chunk 1
            // first, tap 0 without the four fragments row 0 of every layer requests itself)
            static_for<8>([&](auto I_) { constexpr int i = decltype(I_)::value; w1_request<2>(ua, w0 + 2 * 16384, wlane, std::integral_constant<int, (i < 4 ? 12 + i : 8 + (i - 4))>{}); });
            static_for<8>([&](auto I_) { constexpr int i = decltype(I_)::value; w1_request<2>(ua, w0 + 2 * 16384, wlane, std::integral_constant<int, (i < 4 ? 4 + i : i - 4)>{}); });
            static_for<12>([&](auto I_) { constexpr int i = decltype(I_)::value; w1_request<0>(ua, w0, wlane, std::integral_constant<int, (i < 4 ? 4 + i : (i < 8 ? i - 4 : 12 + (i - 8)))>{}); });
        } else {
            w1_request_tap<0>(ua, w0, wlane);
            w1_request_tap<2>(ua, w0 + 2 * 16384, wlane);
        }
    }

    // Groups beyond a workgroup's first are handed out by a ticket counter (overflow[1], zeroed with the range flag): a
    // workgroup that starts late - its CU was running another stream's tree kernel - takes fewer groups instead of
    // holding the launch up with a full static share.  The ticket travels through a spare word of the bias table.
    int *const ticket_lds = reinterpret_cast<int *>(smem + C::HB_OFF + 83 * 4);
    for (int grp = blockIdx.x; grp < n_groups;) {
        const int b0 = grp * G;
        if (wave == 0 && fresh_lane() == 0) *ticket_lds = overflow ? (int)gridDim.x + atomicAdd(overflow + 1, 1) : grp + (int)gridDim.x;
        stamp();
        // ================= stem: planes -> im2col'ed f16-pair images (K = 9 taps x 6 planes, padded to 64) =================
        // (its 16 weight fragments are requested first: their L2 round trip runs under the staging pass)
        i32x4v fa[2][2][4];                                      // [kc][piece][ct]
        bool pbig = false;                                       // an input plane value beyond the guard's limit (or NaN)
        {
            const int wvg = fresh_lane() * 16;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        gmem_load_frag(fa[kc][p][c], net.wsplit + (size_t)kc * 8192, wvg + (p * 4 + c) * 1024);
        }
        {
            unsigned *st = reinterpret_cast<unsigned *>(smem + C::STAGE);
            const int stid = wave * 64 + fresh_lane();
            __builtin_assume(stid >= 0 && stid < NTHR);          // (the lane id is an asm result: without this every guard below becomes a loop)
            // every plane value is split ONCE (split4<FmtF16>'s arithmetic: hi = rn16(v), lo = rn16((v - hi) * 2048)) and
            // staged as one word at cell (y + 1, x + 1) of its plane's bordered image
#pragma unroll
            for (int i = 0; i < NPL; ++i) {
                const int e = stid + i * NTHR;
                const int pc = w1_div81(e), p = e - pc * P, y = (p * 57) >> 9;         // board * 6 + plane, cell
                const _Float16 h = (_Float16)pre[i];
                const _Float16 l = (_Float16)((pre[i] - (float)h) * 2048.f);
                pbig |= !(fabsf(pre[i]) < (float)kWsRangeLimit);
                const unsigned w = (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
                if (e < G * 6 * P) st[pc * C::PW + p + 2 * y + 12] = w;
            }
            // the border: words 0 .. 11 (row 0, left of row 1), the pairs right of row r / left of row r + 1 (r = 1 .. 8),
            // words 109 .. 120 (right of row 9, row 10): 40 words per plane
#pragma unroll
            for (int i = 0; i < (G * 6 * 40 + NTHR - 1) / NTHR; ++i) {
                const int e = stid + i * NTHR;
                const int pc = w1_div40(e), j = e - pc * 40, k = j - 12;
                const int idx = j < 12 ? j : (j < 28 ? 11 * (k >> 1) + 21 + (k & 1) : j + 81);
                if (e < G * 6 * 40) st[pc * C::PW + idx] = 0u;
            }
            static_assert(NTHR == 4 * 64, "zero blocks of the four images: one word a thread");
            reinterpret_cast<unsigned *>(smem + C::SI_OFF + (stid >> 6) * IMG + C::ZOFF)[stid & 63] = 0u;
            // (scale / shift through the overlay: sixteen exposed L2 round trips per group when the stem's epilogue fetched them itself)
            if (stid < 128) reinterpret_cast<float *>(smem + C::SS_OFF)[stid] = ssv;
            __syncthreads();
            // im2col: word gathers at compile-time offsets from the row's cell + byte permutes that separate the pieces
            // (k = 6 tap + plane; k >= 54: exact zeros)
            static_assert(M <= NTHR, "im2col: one row a thread");
            if (const int row = stid; row < M) {
                const int bl = (row >= P ? 1 : 0) + (row >= 2 * P ? 1 : 0), p = row - bl * P, y = (p * 57) >> 9;
                const unsigned *src = st + bl * 6 * C::PW + p + 2 * y + 12;
                const int swz = (row >> 1) & 3;
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) {
                    unsigned hi[4], lo[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = sl * 8 + 2 * j;              // (54 is even: a pair is inside or outside as a whole)
                        if (k < 54) {
                            const int t0 = k / 6, c0 = k - t0 * 6, t1 = (k + 1) / 6, c1 = k + 1 - t1 * 6;
                            const unsigned w0 = src[c0 * C::PW + (t0 / 3 - 1) * 11 + (t0 % 3 - 1)];
                            const unsigned w1 = src[c1 * C::PW + (t1 / 3 - 1) * 11 + (t1 % 3 - 1)];
                            hi[j] = __builtin_amdgcn_perm(w1, w0, 0x05040100u);
                            lo[j] = __builtin_amdgcn_perm(w1, w0, 0x07060302u);
                        } else {
                            hi[j] = 0u;
                            lo[j] = 0u;
                        }
                    }
                    const int kc = sl >> 2, slot = (sl & 3) ^ swz;
                    *reinterpret_cast<uint4 *>(smem + C::SI_OFF + (0 * 2 + kc) * IMG + row * 64 + slot * 16) = uint4{hi[0], hi[1], hi[2], hi[3]};
                    *reinterpret_cast<uint4 *>(smem + C::SI_OFF + (1 * 2 + kc) * IMG + row * 64 + slot * 16) = uint4{lo[0], lo[1], lo[2], lo[3]};
                }
            }
        }
        __syncthreads();
        stamp();
        // (the planes are split into f16 pieces too, and a ReLU swallows the NaN of an Inf - Inf: they are part of the range guard)
        float amax = pbig ? INFINITY : 0.f;
        {
            // stem product: 2 k-chunks x 4 channel tiles x RTW row tiles x 3 f16 products (two accumulator sets, scaled
            // low pieces: the direct split kernel's image and weights), batch norm, ReLU -> X (fp32, swizzled)
            const int slane = fresh_lane();                      // (per group: what hangs off the lane id is recomputed, not spilled)
            const int sli = slane & 15, slg = slane >> 4;
            // scale and shift once per group; the fragments of row tile r + 1 are requested before the MFMAs of tile r (the
            // stores of tile r's epilogue would keep hipcc from moving them up by itself): one LDS round trip exposed
            f32x4 sc[4], sh[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sc[c] = *reinterpret_cast<const f32x4 *>(smem + C::SS_OFF + (c * 16 + slg * 4) * 4);
                sh[c] = *reinterpret_cast<const f32x4 *>(smem + C::SS_OFF + 256 + (c * 16 + slg * 4) * 4);
            }
            i32x4v fb[2][2][2];                                  // [tile parity][piece][kc]
            auto tile_row = [&](int r) {
                int row = (wave * RTW + r) * 16 + sli;
                asm volatile("" : "+v"(row));
                return row;
            };
            auto load_tile = [&](int row, i32x4v (&f)[2][2]) {
                const int nat = row * 64 + ((slg ^ ((row >> 1) & 3)) << 4);
                const int addr = C::SI_OFF + (row < M ? nat : C::ZOFF + (nat & 255));
                lds_load_frag<0 * IMG>(f[0][0], smem, addr);
                lds_load_frag<1 * IMG>(f[0][1], smem, addr);
                lds_load_frag<2 * IMG>(f[1][0], smem, addr);
                lds_load_frag<3 * IMG>(f[1][1], smem, addr);
            };
            int row = tile_row(0);
            load_tile(row, fb[0]);
#pragma unroll
            for (int r = 0; r < RTW; ++r) {
                int row_next = row;
                if (r + 1 < RTW) {
                    row_next = tile_row(r + 1);
                    load_tile(row_next, fb[(r + 1) & 1]);
                }
                const int orow = row < M ? row : M;
                const int osw = row < M ? (G == 1 ? w1g1_swz(row) : w1_swz(row)) : 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc) {
                        a0 = mfma16<F>(fa[kc][0][c], fb[r & 1][0][kc], a0);
                        a1 = mfma16<F>(fa[kc][1][c], fb[r & 1][0][kc], a1);
                        a1 = mfma16<F>(fa[kc][0][c], fb[r & 1][1][kc], a1);
                    }
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float t = fmaf(a1[j], 1.f / 2048.f, a0[j]);
                        t = fmaf(t, sc[c][j], sh[c][j]);
                        v[j] = fmaxf(t, 0.f);
                    }
                    amax = fmaxf(fmaxf(amax, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
                    *reinterpret_cast<f32x4 *>(smem + C::X_OFF + orow * 256 + (((c * 4 + slg) ^ osw) << 4)) = v;
                }
                row = row_next;
            }
        }
        __syncthreads();                                        // X complete; the overlay is free again
        if (wave == 0) reinterpret_cast<float *>(smem + C::H_OFF + (M + 1) * 256)[fresh_lane()] = 0.f;   // H's zero row was under it
        stamp();

        // ================= tower: 12 layers, Winograd F(2,3) along x, the three taps along y direct =================
        // Output row y of all three boards is one MFMA column set (unit u = 5 board + t: outputs (y, 2t), (y, 2t + 1)); wave w
        // owns transform point w: its V_w rows (f16 hi / lo pieces, 16 registers a row) live in registers and serve three
        // output rows each - tap ky of row y multiplies V_w[y + ky - 1] -, its 48 weight fragments of the layer in AGPRs.
        // M_w goes through the LDS exchange; wave w' finishes output channels [16 w', 16 w' + 16): out0 = m0 + m1 + m2,
        // out1 = m1 - m2 - m3, shift, residual, ReLU.  Everything but the MFMAs of row y rides along them: exchange + epilogue
        // of row y - 1, cell reads and input transform of a row ahead (three boards: row y + 3), weight requests of the next layer.
        if constexpr (G == 1) {
            // ================= one board per workgroup: MFMA column u = 5 yi + t, row tile j = output rows 3j + yi =================
            // Same arithmetic per output as the three-board variant below, in the same order (taps ky = 0, 1, 2 - rows outside the
            // board contribute exact zeros instead of being skipped; k-chunks; cross terms first): results do not depend on which of
            // the two a position went through.  A row tile needs three V rows per lane (input rows 3j + yi - 1 .. + 1), none shared
            // with the next row tile: 120 VALU of input transform per 72 MFMAs instead of 40.
            const int glane = fresh_lane(), gli = glane & 15, glg = glane >> 4, wlane = glane * 16;   // (per group: not to be hoisted out of the group loop)
            const int uyi = gli / 5, ut = gli - 5 * uyi;
            const bool uv = gli < 15;
            const int xa = wave == 0 ? 2 * ut - 1 : (wave == 2 ? 2 * ut + 1 : 2 * ut);
            const int xb = wave == 0 ? 2 * ut + 1 : (wave == 1 ? 2 * ut + 1 : (wave == 2 ? 2 * ut : 2 * ut + 2));
            // cell (row 3j + yi + q, column x) at row tile 0: address (may lie above the image: q = -1, yi = 0 - never read), stride per row tile
            auto cell1 = [&](int x, int q, int chunk, int invalid_rel, int &adr, int &str) {
                const bool ok = uv && x >= 0 && x < 9;
                const int r0 = uyi + q, rm = (r0 + 3) % 3;
                const int g = (((x + 1) >> 1) + 5 * rm) & 7, sw = (g & 1) | ((g & 6) << 1);
                adr = (ok ? (9 * r0 + x) * 256 : invalid_rel) + ((chunk ^ sw) << 4);
                str = ok ? 27 * 256 : 0;
            };
            int cA[3], cB[3], sA, sB, sdummy, curO0, curO1, curR0, curR1, strO0, strO1, strR0, strR1;
            cell1(xa, -1, glg * 2, C::ZERO_REL, cA[0], sA);
            cell1(xa, 0, glg * 2, C::ZERO_REL, cA[1], sdummy);
            cell1(xa, 1, glg * 2, C::ZERO_REL, cA[2], sdummy);
            cell1(xb, -1, glg * 2, C::ZERO_REL, cB[0], sB);
            cell1(xb, 0, glg * 2, C::ZERO_REL, cB[1], sdummy);
            cell1(xb, 1, glg * 2, C::ZERO_REL, cB[2], sdummy);
            cell1(2 * ut, 0, wave * 4 + glg, C::DUMP_REL, curO0, strO0);
            cell1(2 * ut + 1, 0, wave * 4 + glg, C::DUMP_REL, curO1, strO1);
            cell1(2 * ut, 0, wave * 4 + glg, C::ZERO_REL, curR0, strR0);
            cell1(2 * ut + 1, 0, wave * 4 + glg, C::ZERO_REL, curR1, strR1);
            f32x4 dq[2][2][2];
            i32x4v vh[2][3][2], vl[2][3][2];                           // [row tile parity][q + 1][kc]
            f32x4 acc[2][4];
            f32x4 ez[4], eres[2], ev[2];
            float tvv[4];
            unsigned thh[2];
            // one of the eight cell reads of (row tile J, relative row Q)
            auto rd = [&](auto IN_, auto J_, auto Q_, auto I_) __attribute__((always_inline)) {
                constexpr int IN = decltype(IN_)::value, j = decltype(J_)::value, qi = decltype(Q_)::value, i = decltype(I_)::value;
                constexpr int cb = i >> 2, kc = (i >> 1) & 1, h = i & 1;
                int a = (cb ? cB[qi] + j * sB : cA[qi] + j * sA);
                // rows -1 / 9: the zero row, same chunk (the low byte of the address: rows are 256 bytes)
                if constexpr (j == 0 && qi == 0) a = uyi == 0 ? C::ZERO_REL + (a & 255) : a;
                if constexpr (j == 2 && qi == 2) a = uyi == 2 ? C::ZERO_REL + (a & 255) : a;
                dq[cb][kc][h] = lds_f32x4_at<IN>(a ^ ((kc << 7) | (h << 4)));
            };
            // sub-step I (0 .. 15) of the input transform of relative row Q into V buffer P
            auto tr = [&](auto P_, auto Q_, auto I_) __attribute__((always_inline)) {
                constexpr int pb = decltype(P_)::value, qi = decltype(Q_)::value, i = decltype(I_)::value, kc = i >> 3, h = (i >> 2) & 1, q = i & 3;
                if constexpr (q == 0) {
                    tvv[0] = fmaf(dq[1][kc][h][0], sgn, dq[0][kc][h][0]);
                    tvv[1] = fmaf(dq[1][kc][h][1], sgn, dq[0][kc][h][1]);
                } else if constexpr (q == 1) {
                    tvv[2] = fmaf(dq[1][kc][h][2], sgn, dq[0][kc][h][2]);
                    tvv[3] = fmaf(dq[1][kc][h][3], sgn, dq[0][kc][h][3]);
                } else if constexpr (q == 2) {
                    thh[0] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{tvv[0], tvv[1]}, f16x2));
                    vh[pb][qi][kc][2 * h] = (int)thh[0];
                    vl[pb][qi][kc][2 * h] = (int)low_pieces(tvv[0], tvv[1], thh[0]);
                } else {
                    thh[1] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{tvv[2], tvv[3]}, f16x2));
                    vh[pb][qi][kc][2 * h + 1] = (int)thh[1];
                    vl[pb][qi][kc][2 * h + 1] = (int)low_pieces(tvv[2], tvv[3], thh[1]);
                }
            };
            f32x4 pshf;                                            // the previous layer's epilogue constants (its row tile 2 rides in this layer's row tile 0)
            float pdown;
            // Schedule of a row tile's 72 slices (one MFMA each + what rides along):  0-3 exchange writes of the PREVIOUS row tile
            // (row tile 0: of the previous LAYER's row tile 2 - output buffer = this layer's input, the other residual flag, constants
            // pshf / pdown; a group's first layer: a null epilogue - zero accumulators and constants, zero-row reads, dump-row stores),
            // 10 barrier, 11-12 exchange reads, 13 residual reads, 19-34 sums / shift / residual / ReLU, 35-36 stores | 11-18 cell
            // reads and 19-26 transform of this row tile's OWN third V row (input rows 3j + yi + 1: the last of them was stored
            // under the previous row tile and is visible behind this row tile's barrier) | 27-34 / 35-50 and 51-58 / 59-71 cell reads
            // and transforms of the NEXT row tile's first two V rows (row tile 2: of the next layer's row tile 0, from this layer's
            // output rows -1 .. 2, complete since row tile 1) | weight requests.  No barrier and no prologue at the layer boundary:
            // between a store and any other wave's read of it lies at least one row-tile barrier.
            auto layer_fn = [&](auto IN_, auto OUT_, auto RES_, int layer) __attribute__((always_inline)) {
                constexpr int IN = decltype(IN_)::value, OUT = decltype(OUT_)::value;
                constexpr bool RES = decltype(RES_)::value;
                constexpr int PAR = RES ? 1 : 0;
                constexpr int S1 = PAR ? 3 : 1, S1N = PAR ? 1 : 3;
                const int next_layer = layer + 1 < kTowerLayers ? layer + 1 : 0;
                const unsigned char *wnext = net.w1_w + ((size_t)next_layer * 4 + wave) * 49152;
                f32x4 shf = *reinterpret_cast<const f32x4 *>(net.w1_shift + layer * 64 + wave * 16 + glg * 4);
                float down = net.w1_down[layer];
                int exw = C::EX_OFF + wave * 4096 + glane * 16, exr = C::EX_OFF + wave * 1024 + glane * 16;
                asm volatile("" : "+v"(exw), "+v"(exr));
                if constexpr (!RES) {
                    if (layer == 0) {
                        // a group's first layer: nothing was prepared under a previous layer - the first two V rows of row tile 0
                        static_for<2>([&](auto Q_) {
                            static_for<8>([&](auto I_) { rd(IN_, std::integral_constant<int, 0>{}, Q_, I_); });
                            static_for<16>([&](auto I_) { tr(std::integral_constant<int, PAR>{}, Q_, I_); });
                        });
                    }
                }
                // taps 1 and 0 must have arrived (requested in that order; behind them tap 2's 16 requests, the shift and the scale)
                asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);                 // (an MFMA is no memory operation: nothing else keeps it behind the wait)
                // exchange + epilogue of a row tile: PREV = row tile 2 of the previous layer, else row tile J of this one
                auto epi = [&](auto PREV_, auto J_, auto I_) __attribute__((always_inline)) {
                    constexpr bool PREV = decltype(PREV_)::value;
                    constexpr int j = PREV ? 2 : decltype(J_)::value, i = decltype(I_)::value;
                    constexpr int par = PREV ? 1 - PAR : (j + PAR) & 1;
                    constexpr int OB = PREV ? IN : OUT;
                    constexpr bool RS = PREV ? !RES : RES;
                    const bool null_epi = PREV && layer == 0;
                    if constexpr (i < 4) {
                        lds_f32x4_put<par * 16384 + i * 1024>(exw, acc[par][i]);
                    } else if constexpr (i == 10) {
                        __syncthreads();
                    } else if constexpr (i == 11 || i == 12) {
                        ez[2 * (i - 11)] = lds_f32x4_at<par * 16384 + (2 * (i - 11)) * 4096>(exr);
                        ez[2 * (i - 11) + 1] = lds_f32x4_at<par * 16384 + (2 * (i - 11) + 1) * 4096>(exr);
                    } else if constexpr (i == 13) {
                        if constexpr (RS) {
                            const int zr = C::ZERO_REL + (glane * 16) % 256;
                            eres[0] = lds_f32x4_at<OB>(null_epi ? zr : curR0 + j * strR0);
                            eres[1] = lds_f32x4_at<OB>(null_epi ? zr : curR1 + j * strR1);
                        }
                    } else if constexpr (i >= 19 && i < 35) {
                        constexpr int k = i - 19, cc = k >> 3, e = (k >> 1) & 3, part = k & 1;
                        if constexpr (part == 0) {
                            ev[cc][e] = cc == 0 ? (ez[0][e] + ez[1][e]) + ez[2][e] : (ez[1][e] - ez[2][e]) - ez[3][e];
                        } else {
                            float tt = fmaf(ev[cc][e], PREV ? pdown : down, PREV ? pshf[e] : shf[e]);
                            if constexpr (RS) tt += eres[cc][e];
                            ev[cc][e] = fmaxf(tt, 0.f);
                        }
                    } else if constexpr (i == 35) {
                        amax = fmaxf(fmaxf(amax, ev[0][0]), ev[0][1]);
                        amax = fmaxf(fmaxf(amax, ev[0][2]), ev[0][3]);
                        lds_f32x4_put<OB>(null_epi ? C::DUMP_REL + (glane * 16) % 256 : curO0 + j * strO0, ev[0]);
                    } else if constexpr (i == 36) {
                        amax = fmaxf(fmaxf(amax, ev[1][0]), ev[1][1]);
                        amax = fmaxf(fmaxf(amax, ev[1][2]), ev[1][3]);
                        lds_f32x4_put<OB>(null_epi ? C::DUMP_REL + (glane * 16) % 256 : curO1 + j * strO1, ev[1]);
                    }
                };
                static_for<3>([&](auto J_) {
                    constexpr int j = decltype(J_)::value, par = (j + PAR) & 1, nb = 1 - par;
                    using PB = std::integral_constant<int, par>;
                    using NB = std::integral_constant<int, nb>;
                    using Q0 = std::integral_constant<int, 0>;
                    using Q1 = std::integral_constant<int, 1>;
                    using Q2 = std::integral_constant<int, 2>;
                    static_for<72>([&](auto M_) {
                        constexpr int m = decltype(M_)::value, ky = m / 24, q = m % 24, kc = q / 12, st = (q / 4) % 3, c = q % 4;
                        constexpr int slot = ky == 1 ? S1 : ky;
                        // tap 2, the shift and the scale (the next layer's requests start behind this wait: it would wait for them too)
                        if constexpr (j == 0 && m == 48) {
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            use_here(shf, down);
                            __builtin_amdgcn_sched_barrier(0);      // (hipcc had moved the first tap-2 MFMA in front of the wait: an MFMA is no memory operation)
                        }
                        if constexpr (st == 0)
                            acc[par][c] = mfma16<F>(ua[slot][kc][1][c], vh[par][ky][kc], m < 4 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[par][c]);
                        else if constexpr (st == 1) acc[par][c] = mfma16<F>(ua[slot][kc][0][c], vl[par][ky][kc], acc[par][c]);
                        else acc[par][c] = mfma16<F>(ua[slot][kc][0][c], vh[par][ky][kc], acc[par][c]);
                        // ---- what rides along ----
                        if constexpr (m < 37) {
                            if constexpr (j == 0) epi(std::true_type{}, J_, M_);
                            else epi(std::false_type{}, std::integral_constant<int, j - 1>{}, M_);
                        }
                        // this row tile's own third V row
                        if constexpr (m >= 11 && m < 19) rd(IN_, J_, Q2{}, std::integral_constant<int, m - 11>{});
                        if constexpr (m >= 19 && m < 27) { tr(PB{}, Q2{}, std::integral_constant<int, 2 * (m - 19)>{}); tr(PB{}, Q2{}, std::integral_constant<int, 2 * (m - 19) + 1>{}); }
                        // the next row tile's first two V rows (row tile 2: the next layer's row tile 0, from this layer's output)
                        if constexpr (m >= 27 && m < 35) {
                            if constexpr (j <= 1) rd(IN_, std::integral_constant<int, j + 1>{}, Q0{}, std::integral_constant<int, m - 27>{});
                            else rd(OUT_, Q0{}, Q0{}, std::integral_constant<int, m - 27>{});
                        }
                        if constexpr (m >= 35 && m < 51) tr(NB{}, Q0{}, std::integral_constant<int, m - 35>{});
                        if constexpr (m >= 51 && m < 59) {
                            if constexpr (j <= 1) rd(IN_, std::integral_constant<int, j + 1>{}, Q1{}, std::integral_constant<int, m - 51>{});
                            else rd(OUT_, Q0{}, Q1{}, std::integral_constant<int, m - 51>{});
                        }
                        if constexpr (m >= 59 && m < 62) { tr(NB{}, Q1{}, std::integral_constant<int, 2 * (m - 59)>{}); tr(NB{}, Q1{}, std::integral_constant<int, 2 * (m - 59) + 1>{}); }
                        if constexpr (m >= 62) tr(NB{}, Q1{}, std::integral_constant<int, m - 56>{});
                        // next layer's weights: tap 1 into the spare slot under row tiles 0 and 1, tap 0 right behind row tile 2's
                        // tap-0 MFMAs (the next layer needs it first), tap 2 behind the last MFMA
                        if constexpr (j <= 1 && m >= 50 && m < 72 && (m - 50) % 3 == 0) {
                            constexpr int f = j * 8 + (m - 50) / 3;
                            w1_request<S1N>(ua, wnext + 16384, wlane, std::integral_constant<int, f>{});
                        }
                        if constexpr (j == 2 && m >= 24 && m < 40) w1_request<0>(ua, wnext, wlane, std::integral_constant<int, m - 24>{});
                        __builtin_amdgcn_sched_barrier(0);
                    });
                });
                w1_request_tap<2>(ua, wnext + 2 * 16384, wlane);
                pshf = shf;
                pdown = down;
                if (!(amax < (float)kWsRangeLimit)) ovf = 1;            // f16 range guard (also catches NaN)
                stamp();
            };
            using IX = std::integral_constant<int, C::X_OFF>;
            using IH = std::integral_constant<int, C::H_OFF>;
            if (!(amax < (float)kWsRangeLimit)) ovf = 1;
            {
                // layer 0's null epilogue
                float z0, z1, z2, z3;
                asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0" : "=v"(z0), "=v"(z1), "=v"(z2), "=v"(z3));
                pshf = f32x4{z0, z1, z2, z3};
                pdown = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[1][c] = pshf;
            }
#pragma unroll 1
            for (int blk = 0; blk < kBlocks; ++blk) {
                layer_fn(IX{}, IH{}, std::false_type{}, 2 * blk);
                layer_fn(IH{}, IX{}, std::true_type{}, 2 * blk + 1);
            }
            {
                // the tower's last row tile (layer 11, output X, residual): on its own
                const int exw = C::EX_OFF + wave * 4096 + glane * 16, exr = C::EX_OFF + wave * 1024 + glane * 16;
                constexpr int par = (2 + 1) & 1;
                static_for<4>([&](auto I_) { lds_f32x4_put<par * 16384 + decltype(I_)::value * 1024>(exw, acc[par][decltype(I_)::value]); });
                eres[0] = lds_f32x4_at<C::X_OFF>(curR0 + 2 * strR0);
                eres[1] = lds_f32x4_at<C::X_OFF>(curR1 + 2 * strR1);
                __syncthreads();
                static_for<4>([&](auto I_) { ez[decltype(I_)::value] = lds_f32x4_at<par * 16384 + decltype(I_)::value * 4096>(exr); });
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float o0 = (ez[0][e] + ez[1][e]) + ez[2][e], o1 = (ez[1][e] - ez[2][e]) - ez[3][e];
                    ev[0][e] = fmaxf(fmaf(o0, pdown, pshf[e]) + eres[0][e], 0.f);
                    ev[1][e] = fmaxf(fmaf(o1, pdown, pshf[e]) + eres[1][e], 0.f);
                    amax = fmaxf(fmaxf(amax, ev[0][e]), ev[1][e]);
                }
                lds_f32x4_put<C::X_OFF>(curO0 + 2 * strO0, ev[0]);
                lds_f32x4_put<C::X_OFF>(curO1 + 2 * strO1, ev[1]);
                if (!(amax < (float)kWsRangeLimit)) ovf = 1;
                __syncthreads();
            }
        } else {
            // ---- per-lane geometry: MFMA column u = 5 board + t (15 = padding), k-group lg; wave = transform point
            // (per group, behind the stem: kept alive through stem and heads these twelve registers spill) ----
            const int glane = fresh_lane(), gli = glane & 15, glg = glane >> 4, wlane = glane * 16;   // (per group: not to be hoisted out of the group loop)
            const int ub = gli / 5, ut = gli - 5 * ub;
            const bool uv = gli < 15;
            // the two cells of point `wave`: V = d[xa] + sgn d[xb]
            const int xa = wave == 0 ? 2 * ut - 1 : (wave == 2 ? 2 * ut + 1 : 2 * ut);
            const int xb = wave == 0 ? 2 * ut + 1 : (wave == 1 ? 2 * ut + 1 : (wave == 2 ? 2 * ut : 2 * ut + 2));
            auto cell = [&](int x, int chunk, int invalid_rel, int &adr, int &str) {
                const bool ok = uv && x >= 0 && x < 9;
                // (cells outside the board - and the padding column - keep the chunk their class would give them: the reads of a
                // ds_read_b128 cycle stay on sixteen distinct chunks, zero row included)
                const int g = (5 * ub + ((x + 1) >> 1)) & 7, sw = (g & 1) | ((g & 6) << 1);
                adr = (ok ? (81 * ub + x) * 256 : invalid_rel) + ((chunk ^ sw) << 4);
                str = ok ? 9 * 256 : 0;
            };
            int curA, strA, curB, strB, curO0, strO0, curO1, strO1, curR0, curR1, strR0, strR1;      // cursors (row 0) and row strides
            cell(xa, glg * 2, C::ZERO_REL, curA, strA);
            cell(xb, glg * 2, C::ZERO_REL, curB, strB);
            cell(2 * ut, wave * 4 + glg, C::DUMP_REL, curO0, strO0);        // stores of the channels 16 wave + 4 lg ..
            cell(2 * ut + 1, wave * 4 + glg, C::DUMP_REL, curO1, strO1);
            cell(2 * ut, wave * 4 + glg, C::ZERO_REL, curR0, strR0);        // residual reads (outside the board: zeros)
            cell(2 * ut + 1, wave * 4 + glg, C::ZERO_REL, curR1, strR1);
            f32x4 dq[2][2][2];                                     // cells read ahead: [cell a / b][kc][channel half]
            i32x4v vh[5][2], vl[5][2];                             // V rows: slot 4 = row 0, slot r & 3 = rows 1 .. 8; [kc]
            f32x4 acc[2][4];                                       // [row parity][channel tile]
            f32x4 ez[4], eres[2], ev[2];
            float tvv[4];
            unsigned thh[2];
            i32x4v ux[2][4];                                       // tap 2 / k-chunk 1 of ODD layers, [piece][ct] (even layers: ua[2][1]; see w1_sched)
            auto vslot = [](int r) constexpr { return r == 0 ? 4 : (r & 3); };
            // one of the eight cell reads of the row at curA / curB: (kc, half) group by group in the order the transform takes them,
            // cells a and b; the group whose address needs no XOR comes last and takes the cursor steps instead
            auto khalf = [](int j) constexpr { return (j + 1) & 3; };     // group j of reads / transform steps -> 2 kc + half
            auto rd = [&](auto IN_, auto I_) __attribute__((always_inline)) {
                constexpr int IN = decltype(IN_)::value, i = decltype(I_)::value, cb = i & 1, kc = khalf(i >> 1) >> 1, h = khalf(i >> 1) & 1;
                const int a0 = (cb ? curB : curA) ^ ((kc << 7) | (h << 4));
                if constexpr (!(W1_ABL & 4)) dq[cb][kc][h] = lds_f32x4_at<IN>(a0);
                if constexpr (i == 6) curA += strA;
                if constexpr (i == 7) curB += strB;
            };
            // input transform of one row in twenty steps of two instructions: per (kc, half) t = d_a + sgn d_b (2 x 2 values),
            // the two registers of high pieces, the first halves of the two registers of low pieces, their second halves
            auto tr = [&](auto R_, auto I_) __attribute__((always_inline)) {
                constexpr int r = decltype(R_)::value, i = decltype(I_)::value, kc = khalf(i / 5) >> 1, h = khalf(i / 5) & 1, q = i % 5, s = vslot(r);
                static_assert(i < kW1TrSteps, "input transform: twenty steps");
                if constexpr (W1_ABL & 2) {
                } else if constexpr (q == 0) {
                    tvv[0] = fmaf(dq[1][kc][h][0], sgn, dq[0][kc][h][0]);
                    tvv[1] = fmaf(dq[1][kc][h][1], sgn, dq[0][kc][h][1]);
                } else if constexpr (q == 1) {
                    tvv[2] = fmaf(dq[1][kc][h][2], sgn, dq[0][kc][h][2]);
                    tvv[3] = fmaf(dq[1][kc][h][3], sgn, dq[0][kc][h][3]);
                } else if constexpr (q == 2) {
                    thh[0] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{tvv[0], tvv[1]}, f16x2));
                    thh[1] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{tvv[2], tvv[3]}, f16x2));
                    vh[s][kc][2 * h] = (int)thh[0];
                    vh[s][kc][2 * h + 1] = (int)thh[1];
                } else if constexpr (q == 3) {
                    vl[s][kc][2 * h] = (int)low_piece_first(tvv[0], thh[0]);
                    vl[s][kc][2 * h + 1] = (int)low_piece_first(tvv[2], thh[1]);
                } else {
                    vl[s][kc][2 * h] = (int)low_piece_second((unsigned)vl[s][kc][2 * h], tvv[1], thh[0]);
                    vl[s][kc][2 * h + 1] = (int)low_piece_second((unsigned)vl[s][kc][2 * h + 1], tvv[3], thh[1]);
                }
            };
            f32x4 pshf = f32x4{0.f, 0.f, 0.f, 0.f};                // the previous layer's epilogue constants (its row 8 rides in this layer's row 0)
            float pdown = 0.f;
            int pO0 = C::DUMP_REL + (glane * 16) % 256, pO1 = pO0, pR0 = C::ZERO_REL + (glane * 16) % 256, pR1 = pR0;   // its row-8 cells (layer 0: dump / zero rows)
            // Schedule of a row's slices (one MFMA each + what rides along): the placement tables w1_epi_at / w1_rd_at / w1_tr_at
            // and w1_sched above - exchange + epilogue of row y - 1 | cell reads and input transform of row y + 3 | weight
            // requests.  Row 8's exchange + epilogue ride in the NEXT layer's row 0 (layer 0: a null epilogue - zero accumulators,
            // zero constants, dump-row stores); the next layer's V rows 0, 1 and 2 are transformed under rows 6, 7 and 8 (its
            // input rows 0 - 2 are complete since row 3).  No barrier at the layer boundary: between a store and any other wave's
            // read of it lie at least four row barriers.
            auto layer_fn = [&](auto IN_, auto OUT_, auto RES_, int layer) __attribute__((always_inline)) {
                constexpr int IN = decltype(IN_)::value, OUT = decltype(OUT_)::value;
                constexpr bool RES = decltype(RES_)::value;
                constexpr int PAR = RES ? 1 : 0;                   // conv2 of a block = odd layer
                constexpr int S1 = PAR ? 3 : 1, S1N = PAR ? 1 : 3; // AGPR slot of tap ky = 1 in this / the next layer (taps 0, 2: slots 0, 2)
                const int next_layer = layer + 1 < kTowerLayers ? layer + 1 : 0;
                const unsigned char *wnext = net.w1_w + ((size_t)next_layer * 4 + wave) * 49152;
                const unsigned char *wcur = net.w1_w + ((size_t)layer * 4 + wave) * 49152;
                int exw = C::EX_OFF + wave * 4096 + glane * 16, exr = C::EX_OFF + wave * 1024 + glane * 16;
                asm volatile("" : "+v"(exw), "+v"(exr));
                if (layer == 0) {
                    // a group's first layer: nothing was prepared under a previous layer - V rows 0, 1 and 2
                    // (cursors: set at the top of the group; they end at row 3, whose cells row 0 reads)
                    static_for<3>([&](auto R_) {
                        static_for<8>([&](auto I_) { rd(IN_, I_); });
                        static_for<kW1TrSteps>([&](auto I_) { tr(R_, I_); });
                    });
                }
                // this layer's tap 1 must have arrived (behind its last request: the 23 of rows 6 - 8, w1_sched)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kW1WaitTop) : "memory");
                __builtin_amdgcn_sched_barrier(0);                 // (an MFMA is no memory operation: nothing else keeps it behind the wait)
                // shift and scale of this layer: requested HERE (two vector loads the wait counts below include), first used
                // by row 0's epilogue of row 1, i.e. behind the vmcnt(0) at the top of row 1
                const f32x4 shf = *reinterpret_cast<const f32x4 *>(net.w1_shift + layer * 64 + wave * 16 + glg * 4);
                float down;
                {
                    const float *dp = net.w1_down + layer;
                    int zoff = 0;
                    asm volatile("" : "+v"(zoff));                 // a VECTOR load whatever hipcc proves about the address: the count must not depend on it
                    asm volatile("global_load_dword %0, %1, %2" : "=v"(down) : "v"(zoff), "s"(dp) : "memory");
                }
                // exchange + epilogue of a row: PREV = row 8 of the previous layer (output buffer = this layer's input, the other
                // residual flag, constants pshf / pdown, cells at row 8), else row Y of this layer (cells at curO / curR)
                auto epi = [&](auto PREV_, auto Y_, auto I_) __attribute__((always_inline)) {
                    constexpr bool PREV = decltype(PREV_)::value;
                    constexpr int y = decltype(Y_)::value, i = decltype(I_)::value;
                    constexpr int par = PREV ? (8 + 1 - PAR) & 1 : (y + PAR) & 1;
                    constexpr int OB = PREV ? IN : OUT;
                    constexpr bool RS = PREV ? !RES : RES;
                    if constexpr (i < kEpiWrite + 4) {
                        if constexpr (!(W1_ABL & 16)) lds_f32x4_put<par * 16384 + i * 1024>(exw, acc[par][i]);
                    } else if constexpr (i == kEpiBarrier) {
                        if constexpr (!(W1_ABL & 32)) __syncthreads();
                    } else if constexpr (i < kEpiRead + 4) {
                        if constexpr (!(W1_ABL & 16)) ez[i - kEpiRead] = lds_f32x4_at<par * 16384 + (i - kEpiRead) * 4096>(exr);
                    } else if constexpr (i == kEpiRes) {
                        if constexpr (RS) eres[0] = lds_f32x4_at<OB>(PREV ? pR0 : curR0);
                        if constexpr (!PREV) curR0 += strR0;       // (also without a residual: the next layer's deferred row needs them at row 8)
                    } else if constexpr (i == kEpiRes + 1) {
                        if constexpr (RS) eres[1] = lds_f32x4_at<OB>(PREV ? pR1 : curR1);
                        if constexpr (!PREV) curR1 += strR1;
                    } else if constexpr (i < kEpiArith + kEpiArithSlices) {
                        // one instruction of a cell's arithmetic: per value two for the sum over the points, shift and scale, the
                        // residual (RS), ReLU - in the order and with the operands of out = max(fma(sum, down, shift) + res, 0)
                        constexpr int NPE = RS ? 5 : 4;
                        auto op = [&](auto K_) __attribute__((always_inline)) {
                            constexpr int k = decltype(K_)::value, el = k / NPE, o = k % NPE, cc = el >> 2, e = el & 3;
                            if constexpr (el >= 8 || (W1_ABL & 8)) {
                            } else if constexpr (o == 0) {
                                ev[cc][e] = cc == 0 ? ez[0][e] + ez[1][e] : ez[1][e] - ez[2][e];
                            } else if constexpr (o == 1) {
                                ev[cc][e] = cc == 0 ? ev[cc][e] + ez[2][e] : ev[cc][e] - ez[3][e];
                            } else if constexpr (o == 2) {
                                ev[cc][e] = fmaf(ev[cc][e], PREV ? pdown : down, PREV ? pshf[e] : shf[e]);
                            } else if constexpr (RS && o == 3) {
                                ev[cc][e] += eres[cc][e];
                            } else {
                                ev[cc][e] = fmaxf(ev[cc][e], 0.f);
                            }
                        };
                        op(std::integral_constant<int, 2 * (i - kEpiArith)>{});
                        op(std::integral_constant<int, 2 * (i - kEpiArith) + 1>{});
                    } else if constexpr (i == kEpiGuard0) {
                        amax = fmaxf(fmaxf(amax, ev[0][0]), ev[0][1]);
                        amax = fmaxf(fmaxf(amax, ev[0][2]), ev[0][3]);
                    } else if constexpr (i == kEpiStore0) {
                        lds_f32x4_put<OB>(PREV ? pO0 : curO0, ev[0]);
                        if constexpr (!PREV) curO0 += strO0;
                    } else if constexpr (i == kEpiGuard1) {
                        amax = fmaxf(fmaxf(amax, ev[1][0]), ev[1][1]);
                        amax = fmaxf(fmaxf(amax, ev[1][2]), ev[1][3]);
                    } else if constexpr (i == kEpiStore1) {
                        lds_f32x4_put<OB>(PREV ? pO1 : curO1, ev[1]);
                        if constexpr (!PREV) curO1 += strO1;
                    }
                };
                static_for<9>([&](auto Y_) {
                    constexpr int y = decltype(Y_)::value, par = (y + PAR) & 1;
                    constexpr int NT = (y == 0 || y == 8) ? 2 : 3, NM = 24 * NT, KY0 = y == 0 ? 1 : 0;
                    if constexpr (PROF)
                        if (blockIdx.x == 0 && wave == 0 && glane == 0 && (layer == 2 || layer == 3) && grp == (int)blockIdx.x)
                            net.timeline[40 + 12 * (layer - 2) + y] = (long long)__builtin_amdgcn_s_memtime();
                    // tap 0 - its last four fragments were requested in row 0 - and with it the layer's shift and scale
                    if constexpr (y == 1) {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (y == 6) { curA -= 9 * strA; curB -= 9 * strB; }              // from here on: the next layer's rows 0 .. 2
                    static_for<NM>([&](auto M_) {
                        constexpr int m = decltype(M_)::value, ti = m / 24, q = m % 24, kc = q / 12, st = (q / 4) % 3, c = q % 4;
                        constexpr int ky = KY0 + ti, r = y + ky - 1, s = vslot(r), slot = ky == 1 ? S1 : ky;
                        constexpr bool UX = PAR == 1 && ky == 2 && kc == 1;      // odd layers: tap 2 / k-chunk 1 from the VGPR fragments
                        // tap 2 (row 0: the second tap): its last request was row 8's slice 9 of the previous layer
                        if constexpr (y == 0 && m == 24) {
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kW1WaitTap2) : "memory");
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if constexpr (W1_ABL & 128) {
                        } else if constexpr (st == 0)
                            acc[par][c] = mfma16<F>(UX ? ux[1][c] : ua[slot][kc][1][c], vh[s][kc], m < 4 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[par][c]);
                        else if constexpr (st == 1) acc[par][c] = mfma16<F>(UX ? ux[0][c] : ua[slot][kc][0][c], vl[s][kc], acc[par][c]);
                        else acc[par][c] = mfma16<F>(UX ? ux[0][c] : ua[slot][kc][0][c], vh[s][kc], acc[par][c]);
                        // ---- what rides along: BEHIND its MFMA (in one scheduling region hipcc puts a slice's riders in front of
                        // the MFMA or behind it as it likes, and two slices' riders end up in one gap) ----
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (constexpr int e = w1_epi_at(m); e >= 0) {
                            if constexpr (y == 0) epi(std::true_type{}, Y_, std::integral_constant<int, e>{});
                            else epi(std::false_type{}, std::integral_constant<int, y - 1>{}, std::integral_constant<int, e>{});
                        }
                        if constexpr (constexpr int i = w1_rd_at(y, m); i >= 0) {
                            if constexpr (y + 3 <= 8) rd(IN_, std::integral_constant<int, i>{});
                            else rd(OUT_, std::integral_constant<int, i>{});                     // rows 6 .. 8: the next layer's rows 0 .. 2
                        }
                        if constexpr (constexpr int i = w1_tr_at(y, m); i >= 0)
                            tr(std::integral_constant<int, (y + 3 <= 8 ? y + 3 : y - 6)>{}, std::integral_constant<int, i>{});
                        // weight requests (w1_sched): each behind the last use of the register it goes to
                        {
                            constexpr int code = w1_sched(y, m), kind = code >> 4;
                            using FR = std::integral_constant<int, (code & 15)>;
                            if constexpr (code >= 0 && !(W1_ABL & 1)) {
                                if constexpr (kind == 0) w1_request<S1N>(ua, wnext + 16384, wlane, FR{});
                                else if constexpr (kind == 1) {
                                    // (the next layer is odd when this one is even: its tap 2 / k-chunk 1 goes to the VGPR fragments)
                                    if constexpr (PAR == 0) w1_request_v(ux[(FR::value >> 2) & 1][FR::value & 3], wnext + 2 * 16384, wlane, FR{});
                                    else w1_request<2>(ua, wnext + 2 * 16384, wlane, FR{});
                                } else if constexpr (kind == 2) w1_request<2>(ua, wnext + 2 * 16384, wlane, FR{});
                                else if constexpr (kind == 3) w1_request<0>(ua, wnext, wlane, FR{});
                                else w1_request<0>(ua, wcur, wlane, FR{});
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    });
                });
                if constexpr (PROF)
                    if (blockIdx.x == 0 && wave == 0 && glane == 0 && (layer == 2 || layer == 3) && grp == (int)blockIdx.x)
                        net.timeline[40 + 12 * (layer - 2) + 9] = (long long)__builtin_amdgcn_s_memtime();
                pshf = shf;
                pdown = down;
                // the cursors stand at row 8 (eight rows stored): that is where the deferred epilogue goes; back to row 0 for the next layer
                pO0 = curO0; pO1 = curO1; pR0 = curR0; pR1 = curR1;
                curO0 -= 8 * strO0; curO1 -= 8 * strO1; curR0 -= 8 * strR0; curR1 -= 8 * strR1;
                if (!(amax < (float)kWsRangeLimit)) ovf = 1;            // f16 range guard (also catches NaN)
                stamp();
            };
            using IX = std::integral_constant<int, C::X_OFF>;
            using IH = std::integral_constant<int, C::H_OFF>;
            if (!(amax < (float)kWsRangeLimit)) ovf = 1;
            // row 8's cells (the deferred epilogue) and layer 0's null epilogue
            {
                float z0, z1, z2, z3;
                asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0" : "=v"(z0), "=v"(z1), "=v"(z2), "=v"(z3));
                pshf = f32x4{z0, z1, z2, z3};
                pdown = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[1][c] = pshf;
            }
#pragma unroll 1
            for (int blk = 0; blk < kBlocks; ++blk) {
                layer_fn(IX{}, IH{}, std::false_type{}, 2 * blk);
                layer_fn(IH{}, IX{}, std::true_type{}, 2 * blk + 1);
            }
            {
                // the tower's last row (layer 11, output X, residual): on its own
                const int exw = C::EX_OFF + wave * 4096 + glane * 16, exr = C::EX_OFF + wave * 1024 + glane * 16;
                constexpr int par = (8 + 1) & 1;
                static_for<4>([&](auto I_) { lds_f32x4_put<par * 16384 + decltype(I_)::value * 1024>(exw, acc[par][decltype(I_)::value]); });
                eres[0] = lds_f32x4_at<C::X_OFF>(pR0);
                eres[1] = lds_f32x4_at<C::X_OFF>(pR1);
                __syncthreads();
                static_for<4>([&](auto I_) { ez[decltype(I_)::value] = lds_f32x4_at<par * 16384 + decltype(I_)::value * 4096>(exr); });
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float o0 = (ez[0][e] + ez[1][e]) + ez[2][e], o1 = (ez[1][e] - ez[2][e]) - ez[3][e];
                    ev[0][e] = fmaxf(fmaf(o0, pdown, pshf[e]) + eres[0][e], 0.f);
                    ev[1][e] = fmaxf(fmaf(o1, pdown, pshf[e]) + eres[1][e], 0.f);
                    amax = fmaxf(fmaxf(amax, ev[0][e]), ev[1][e]);
                }
                lds_f32x4_put<C::X_OFF>(pO0, ev[0]);
                lds_f32x4_put<C::X_OFF>(pO1, ev[1]);
                if (!(amax < (float)kWsRangeLimit)) ovf = 1;
                __syncthreads();
            }
        }
        // a group that left the f16 range says so: the exact kernel behind this launch redoes the marked groups only
        if (group_bits && !(amax < (float)kWsRangeLimit)) atomicOr(group_bits + (grp >> 5), 1 << (grp & 31));
        // next group's input planes: requested here, consumed after the heads
        const int next = __builtin_amdgcn_readfirstlane(*ticket_lds);   // (written before the stem's barriers)
        fetch_planes(next);
        if constexpr (!(W1_ABL & 256))
        run_heads_x32<G, C, (G == 1 ? 2 : 1)>(smem, net, b0, batch, want_logits, policy, value, wave * 64 + fresh_lane(), wave,
                                              PROF && blockIdx.x == 0 && grp == (int)blockIdx.x ? net.timeline + 64 : nullptr,   // [64..66]: 1x1 convolutions done, barrier passed, FCs done
                                              overflow, group_bits, grp);
        __syncthreads();
        stamp();
        grp = next;
    }
    if (ovf && overflow) atomicOr(overflow, 1);
}

template <int G, bool PROF = false>
int launch_w1d(tg_net *net, int grid, const tg::ForwardArgs &a) {
    using C = WsCfg<G>;
    if (!PROF && net->dev.timeline) return launch_w1d<G, true>(net, grid, a);
    auto kern = dualnet_fwd_w1d_kernel<G, PROF>;
    static std::atomic<uint64_t> configured{0};
    if (tg::first_on_device(configured, net->device))
        TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NTHR), C::LDS_BYTES, a.stream, net->dev, a.planes, a.batch, a.want_logits,
                       a.policy, a.value, a.flag, a.bits);
    TG_HIP(hipGetLastError());
    return TG_OK;
}

}  // namespace

namespace tg {

// dualnet_fwd_w1d_kernel's weights (w1d_image, net_weights.h); the image does not depend on the board size
int w1d_prepare(tg_net *net, const float *params, const ParamLayout &L, const ExactImages &exact) {
    const W1dImage im = w1d_image(params, L, exact.scale, exact.shift);
    net->spread_w1d = im.spread;
    int rc;
    if ((rc = tg::upload(net, im.w1_w, &net->dev.w1_w)) || (rc = tg::upload(net, im.w1_shift, &net->dev.w1_shift))) return rc;
    return tg::upload(net, im.w1_down, &net->dev.w1_down);
}

int w1d_forward(tg_net *net, const tg_fwd::ForwardPlan &plan, const ForwardArgs &a) {
    if (net->board_size != 9) return tg::fail(TG_ERR_ARG, "w1d forward: 9x9 only");
    if (plan.group == 3) return launch_w1d<3>(net, plan.grid, a);
    return launch_w1d<1>(net, plan.grid, a);
}

}  // namespace tg
