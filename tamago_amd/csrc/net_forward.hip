// DualNet forward for gfx950 (MI355X): one fused, persistent kernel for the whole network.
//
// Replaces nn/network/dual_net.py:41-106 (+ res_block.py:36-39, head/policy_head.py:33-39,
// head/value_head.py:33-39) as run by mcts/tree.py:280-285.
//
// Design (see DESIGN.md "forward kernel"):
//  * A workgroup (4 wavefronts) owns G boards and carries them through all 13 3x3
//    convolutions + both heads.  Activations never leave the CU: one fp32 LDS buffer
//    [G*P rows][64 ch] (row stride 72 floats = conflict-free ds_read_b128 A fragments), the
//    layer result lives in MFMA accumulators until every wave has finished reading the
//    layer input, then overwrites it in place; the residual-block input stays in VGPRs.
//  * Each 3x3 conv is an implicit GEMM  M = G*P rows, N = 64, K = 9 taps x 64 ch  on
//    v_mfma_f32_16x16x4_f32 (exact fp32, the only fp32 matrix path on gfx950).  Wave w owns
//    output channels [16w,16w+16): B fragments (weights) are pre-shuffled on the host into
//    fragment order, so one coalesced global_load_dwordx4 (1 KiB per wave, L2 resident)
//    feeds four MFMAs per M-tile; A fragments are one ds_read_b128 per four MFMAs.
//    Zero padding is an address select to a zero row (no branches).
//  * BatchNorm is folded to a per-channel scale/shift applied in the epilogue together with
//    the residual add and ReLU.
//  * Heads (1x1 conv + BN + ReLU + FC + softmax) run on the VALU from the same LDS buffer.
#include "net_device.h"
#include "net_weights.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>

namespace tg {
// net_forward_split.hip
int split_prepare(tg_net *net, const float *params, const ParamLayout &L, const ExactImages &exact);
int split_forward(tg_net *net, const tg_fwd::ForwardPlan &plan, const ForwardArgs &a);
int heads_prepare(tg_net *net, const float *params, const ParamLayout &L, const ExactImages &exact);
// net_forward_w1d.hip: the tower as Winograd F(2,3) along x on split operands (the 9x9 default)
int w1d_prepare(tg_net *net, const float *params, const ParamLayout &L, const ExactImages &exact);
int w1d_forward(tg_net *net, const tg_fwd::ForwardPlan &plan, const ForwardArgs &a);
// net_forward_w1dband.hip: 19x19, one-axis Winograd tower, a board over two workgroups + the batched heads kernel
int w1dband_forward(tg_net *net, const tg_fwd::ForwardPlan &plan, const ForwardArgs &a);
// net_forward_band.hip: a 19x19 board spread over 2 / 4 workgroups (small launches)
int band_forward(tg_net *net, const tg_fwd::ForwardPlan &plan, const ForwardArgs &a);
}  // namespace tg

namespace {

constexpr int kBandFlagInts = 2 * 512;                     // (two per workgroup of a banded launch, at most num_cus workgroups)

template <int S, int G>
__global__ __launch_bounds__(256, (FwdCfg<S, G>::WAVES_PER_SIMD)) void dualnet_fwd_kernel(
    NetDev net, const float *__restrict__ planes, int batch, int want_logits,
    float *__restrict__ policy, float *__restrict__ value) {
    using C = FwdCfg<S, G>;
    constexpr int P = C::P, M = C::M, MT = C::MT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = tid >> 6;   // output-channel tile
    const int lane = tid & 63;
    const int li = lane & 15;    // A row / B,C column within a tile
    const int lg = lane >> 4;    // k index within an MFMA

    // ---- per-lane constants ----------------------------------------------------------
    // tap validity for row (mt*16 + li): bit t of mask[mt]
    unsigned mask[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int r = mt * 16 + li;
        const int bl = r / P;
        const int p = r - bl * P;
        const int y = p / S, x = p - y * S;
        unsigned m = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            if (r < M && yy >= 0 && yy < S && xx >= 0 && xx < S) m |= 1u << t;
        }
        mask[mt] = m;
    }
    const int lane_act = li * kRowBytes + lg * 16;   // + mt*16*288 + tap offset + s*64
    const int lane_zero = C::ZROW + lg * 16;
    const int lane_in8 = C::AUX + li * 32 + lg * 4;  // + mt*16*32 + tap offset (+16 for k-step 1)
    const int lane_zero8 = C::ZERO8 + lg * 4;

    // zero rows (written once, never overwritten)
    for (int e = tid; e < kRowFloats; e += 256) reinterpret_cast<float *>(smem + C::ZROW)[e] = 0.f;
    if (tid < 8) reinterpret_cast<float *>(smem + C::ZERO8)[tid] = 0.f;

    int stamp_i = 0;
    auto stamp = [&]() {
        if (net.timeline && blockIdx.x == 0 && tid == 0 && stamp_i < 64)
            net.timeline[stamp_i++] = (long long)__builtin_amdgcn_s_memtime();
    };
    const int n_groups = (batch + G - 1) / G;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int b0 = grp * G;
        stamp();                                  // 0: group start

        stage_planes<S, G>(smem, planes, b0, batch, tid);
        __syncthreads();

        f32x4 acc[MT];
        f32x4 res[MT];

        // ---- layer 0: 6(8) -> 64, K = 9 taps x 2 k-steps -----------------------------------
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const float2 *w0 = reinterpret_cast<const float2 *>(net.w0frag) + wave * 9 * 64 + lane;
            float2 bnext = w0[0];
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                const float2 bcur = bnext;
                bnext = w0[(tap < 8 ? tap + 1 : 8) * 64];
                const int toff = ((tap / 3 - 1) * S + (tap % 3 - 1)) * 32;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const bool ok = (mask[mt] >> tap) & 1u;
                    const int a = ok ? lane_in8 + mt * 16 * 32 + toff : lane_zero8;
                    const float a0 = lds_f32(smem, a);
                    const float a1 = lds_f32(smem, a + 16);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcur.x, a0, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcur.y, a1, acc[mt], 0, 0, 0);
                }
            }
        }

        stamp();                                  // 1: stem MFMAs issued
        // ---- epilogue + layers 1..12 -----------------------------------------------------------
#pragma unroll 1
        for (int layer = 0; layer < kConvLayers; ++layer) {
            if (layer > 0) {
                // conv `layer` reads the activation buffer written by the previous epilogue
                __syncthreads();
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 *wl = reinterpret_cast<const f32x4 *>(net.wfrag) +
                                  ((size_t)((layer - 1) * 4 + wave) * 9) * 4 * 64 + lane;
                // Software pipeline.  K is walked as 36 groups of 16 input channels (9 taps x 4);
                // the B fragment of group g+1 (one global_load_dwordx4, L2 resident) is in flight
                // while group g computes.  Inside a group the M-tiles are processed in chunks
                // of CH: the A fragments of chunk c+1 are loaded ahead of the MFMAs of chunk c,
                // and consecutive MFMAs hit different accumulators (the same accumulator comes
                // back every CH MFMAs = CH*32 cycles, beyond the 40-cycle dependent latency).
                constexpr int CH = 4;
                constexpr int NCH = (MT + CH - 1) / CH;
                f32x4 bnext = wl[0];
#pragma unroll 1
                for (int tap = 0; tap < 9; ++tap) {
                    const int toff = ((tap / 3 - 1) * S + (tap % 3 - 1)) * kRowBytes;
                    int addr[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const bool ok = (mask[mt] >> tap) & 1u;
                        addr[mt] = ok ? lane_act + mt * 16 * kRowBytes + toff : lane_zero;
                    }
                    f32x4 acur[CH], anext[CH];
#pragma unroll
                    for (int m = 0; m < CH; ++m)
                        if (m < MT) acur[m] = lds_f32x4(smem, addr[m]);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const f32x4 bcur = bnext;
                        const int gn = tap * 4 + s + 1;
                        bnext = wl[(gn < 36 ? gn : 35) * 64];
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const bool last = (s == 3 && c == NCH - 1);
                            if (!last) {
                                const int c2 = (c + 1) % NCH, s2 = s + (c + 1) / NCH;
#pragma unroll
                                for (int m = 0; m < CH; ++m)
                                    if (c2 * CH + m < MT) anext[m] = lds_f32x4(smem, addr[c2 * CH + m] + s2 * 64);
                            }
                            // keep the prefetch ahead of the MFMA block (hipcc otherwise sinks the
                            // loads to just before their first use and exposes the LDS latency)
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
#pragma unroll
                                for (int m = 0; m < CH; ++m) {
                                    const int mt = c * CH + m;
                                    if (mt < MT)
                                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcur[j], acur[m][j], acc[mt], 0, 0, 0);
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int m = 0; m < CH; ++m) acur[m] = anext[m];
                        }
                    }
                }
                stamp();                          // layer MFMAs issued (before the barrier)
                // every wave must be done reading before anyone overwrites the buffer
                __syncthreads();
                stamp();                          // barrier passed
            }
            // epilogue: BN scale/shift (+ residual) + ReLU.  The MFMAs are issued with the weights
            // as the A operand and the activations as B, so D is [cout][position]: C/D column
            // (lane & 15) = position within the M-tile, C/D rows 4*(lane>>4)+j = four CONSECUTIVE
            // output channels -> one 16-byte LDS store per M-tile instead of four 4-byte ones.
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(net.scale + layer * 64 + wave * 16 + lg * 4);
            const f32x4 sh = *reinterpret_cast<const f32x4 *>(net.shift + layer * 64 + wave * 16 + lg * 4);
            const bool block_out = (layer & 1) == 0;       // stem (0) and every conv2 (2,4,..,12)
            const bool add_res = block_out && layer > 0;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = fmaf(acc[mt][j], sc[j], sh[j]);
                    if (add_res) t += res[mt][j];
                    v[j] = fmaxf(t, 0.f);
                }
                if (block_out) res[mt] = v;
                const int r = mt * 16 + li;
                if (r < M)
                    *reinterpret_cast<f32x4 *>(smem + r * kRowBytes + wave * 64 + lg * 16) = v;
            }
        }
        __syncthreads();
        stamp();                                  // all epilogues done

        run_heads<S, G>(smem, net, b0, batch, want_logits, policy, value, tid);
        __syncthreads();
        stamp();                                  // heads done
    }
}


// ======================================================================================
// Winograd F(2x2,3x3) residual tower (same fusion, same LDS residency as the direct kernel).
//
// For every 2x2 output tile the 3x3 correlation becomes 16 element-wise products in the
// transform domain; summed over input channels these are 16 independent GEMMs
//   M_xi[cout][tile] = sum_cin U_xi[cout][cin] * V_xi[cin][tile],  xi = 0..15,
// with V = B^T d B (input transform, adds only), U = G g G^T (host) and Y = A^T M A (output
// transform, adds only).  A 9x9 board has 25 tiles (the 10th row/column is discarded), so the
// MFMA rows per board drop from 81 x 9 taps to 25 x 16 points: 1.8x fewer MFMAs in exact
// fp32 (the transforms only add; the weights pick up factors 1/2 and 1/4).
//
// The workgroup keeps TWO activation buffers in LDS (block input X and intermediate H), so
// neither the layer outputs nor the residual have to live in registers: every row-tile's
// 2x2 outputs are finished (BN, residual, ReLU) and written to the other buffer as soon as
// its 16 accumulators are complete, and a layer needs a single barrier.  Lane (li, lg) loads
// the patch of tile rt*16+li (channels 16s+4lg..+3) and - because the weights are the MFMA A
// operand - also receives that tile's outputs for channels 16w+4lg..+3.
// Work unit = (row-tile, 16 input channels): 16 ds_read_b128 -> in-register input transform
// -> 64 MFMAs into 16 accumulators.
template <int S, int G, bool GS = false>
struct WinoCfg {
    static constexpr int P = S * S;
    static constexpr int A = P + 1;
    static constexpr int M = G * P;
    static constexpr int MT = (M + 15) / 16;
    static constexpr int TY = (S + 1) / 2;          // tiles per side (5)
    static constexpr int TPB = TY * TY;             // tiles per board (25)
    static constexpr int NT = G * TPB;
    static constexpr int RT = (NT + 15) / 16;       // row-tiles of 16 Winograd tiles
    static constexpr int ROW_BYTES = kWinoRowBytes;
    // GS ("global scratch", 19x19): two 98 KB buffers do not fit into 160 KB of LDS, so LDS holds
    // only the input of the current layer; layer outputs go to a per-workgroup scratch image in
    // global memory (L2-resident) and are copied back into LDS behind the layer barrier
    static constexpr int NBUF = GS ? 1 : 2;
    static constexpr int BUF_A = 0;
    static constexpr int BUF_B = GS ? 0 : M * kWinoRowBytes;
    static constexpr int ZROW = NBUF * M * kWinoRowBytes;
    static constexpr int AUX = ZROW + kWinoRowBytes;          // in8 staging / head scratch
    static constexpr int AUX_BYTES = M * 32;
    static constexpr int ZERO8 = AUX + AUX_BYTES;
    static constexpr int LDS_BYTES = ZERO8 + 32;
};

// ---- Winograd tower, 8 waves per workgroup (2 per SIMD) --------------------------------------
// Wave (w, h): output channels [16w, 16w+16), half h = 0 takes row-tiles {0,1,2}, h = 1 takes
// {3,4} (75 tiles).  A wave alternates "16 patch reads + input transform" with "64 MFMAs".
// What costs time here is instruction ISSUE: a wave is held for the 8 passes of each MFMA it
// issues and everything else it issues comes on top (tools/microbench/mfma_coissue.hip), so
// the loop is trimmed for instruction count: packed subtractions (sub4), patch addresses from
// per-lane geometry computed once (3 VALU each per row-tile, one add per slice), a weight
// ring that runs on across row-tiles.
template <int S, int G, bool GS = false>
__global__ __launch_bounds__(512, 2) void dualnet_fwd_wino8_kernel(
    NetDev net, const float *__restrict__ planes, int batch, int want_logits,
    float *__restrict__ policy, float *__restrict__ value, const int *__restrict__ guard, int *__restrict__ group_bits,
    int *__restrict__ clear_next) {
    using C = WinoCfg<S, G, GS>;
    // (guard launches of the 9x9 f16 kernels: the flag words of the stream's NEXT launch are cleared here - two sets alternate -
    // instead of by a 5 us memset node in front of every forward pass; nobody reads that set during this launch)
    if (clear_next != nullptr && blockIdx.x == 0 && threadIdx.x < 2) clear_next[threadIdx.x] = 0;
    // fallback launch behind the split-operand kernel: runs only if that kernel raised its range flag - and, when that kernel
    // says WHICH groups left the f16 range (bit 0 of the flag + one bit per group in group_bits; bit 1 of the flag = redo
    // everything: a band gave up waiting), only over those groups: a single hot position costs one group's redo, not the batch's
    bool only_marked = false;
    if (guard != nullptr) {
        const int gf = __builtin_nontemporal_load(guard);
        if (gf == 0) return;
        only_marked = group_bits != nullptr && !(gf & 2);
        if (blockIdx.x == 0 && threadIdx.x == 0 && net.fallbacks) atomicAdd(net.fallbacks, 1ull);
    }
    constexpr int P = C::P, M = C::M, MT = C::MT;
    constexpr int TY = C::TY, TPB = C::TPB, NT = C::NT, RT = C::RT;
    constexpr int MTH = (MT + 1) / 2;                 // stem M-tiles per half
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int wave = wid & 3;                         // output-channel tile
    const int half = wid >> 2;
    const int lane = tid & 63;
    const int li = lane & 15;
    const int lg = lane >> 4;

    const int lane_zero = C::ZROW + lg * 16;
    const int lane_in8 = C::AUX + li * 32 + lg * 4;
    const int lane_zero8 = C::ZERO8 + lg * 4;

    // profiling stamps (tg_net_profile_phases), workgroup 0: first lane of wave 0 (half 0, three
    // row-tiles) -> [0,64), first lane of wave 4 (half 1, two row-tiles, same SIMD) -> [64,128)
    int stamp_i = 0;
    auto stamp = [&]() {
        if (net.timeline && blockIdx.x == 0 && (tid == 0 || tid == 256) && stamp_i < 64)
            net.timeline[(tid == 0 ? 0 : 64) + stamp_i++] = (long long)__builtin_amdgcn_s_memtime();
    };
    for (int e = tid; e < kWinoRowFloats; e += 512) reinterpret_cast<float *>(smem + C::ZROW)[e] = 0.f;
    if (tid < 8) reinterpret_cast<float *>(smem + C::ZERO8)[tid] = 0.f;

    // row-tile split between the two halves: half 0 takes the first (RT+1)/2 row-tiles.  Per-lane
    // geometry of this wave's row-tiles, computed once: buffer-relative address of the patch origin
    // (with the lane's channel sub-slice) and the 16 "inside the board" bits of the 4x4 patch
    constexpr int RTH = (RT + 1) / 2;
    const int rt_begin = half == 0 ? 0 : RTH;
    const int n_own = half == 0 ? RTH : RT - RTH;
    int base_rel[RTH];
    int base_row[RTH];                                // row index of the patch origin (global scratch addressing)
    unsigned valid[RTH];
#pragma unroll
    for (int r = 0; r < RTH; ++r) {
        const int t = (rt_begin + r) * 16 + li;
        const int bl = t / TPB;
        const int tl = t - bl * TPB;
        const int ty = tl / TY, tx = tl - ty * TY;
        const int y0 = 2 * ty - 1, x0 = 2 * tx - 1;
        unsigned m = 0;
#pragma unroll
        for (int pq = 0; pq < 16; ++pq) {
            const int y = y0 + pq / 4, x = x0 + pq % 4;
            if (r < n_own && t < NT && y >= 0 && y < S && x >= 0 && x < S) m |= 1u << pq;
        }
        valid[r] = m;
        base_row[r] = (r < n_own && t < NT) ? bl * P + y0 * S + x0 : 0;
        base_rel[r] = base_row[r] * kWinoRowBytes + lg * 16;
    }
    // global scratch images of this workgroup: X (block input / output) and H (intermediate)
    float *gx = GS ? net.scratch + (size_t)blockIdx.x * 2 * M * 64 : nullptr;
    float *gh = GS ? gx + (size_t)M * 64 : nullptr;
    const int n_groups = (batch + G - 1) / G;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int b0 = grp * G;
        if (guard != nullptr) {
            // (uniform: every thread reads the same word; the owner of the group - this workgroup - clears the bit behind the
            // barrier, so the bitmap is all zero again when the launch ends)
            int marked = 1;
            if (group_bits != nullptr) {
                marked = (__builtin_nontemporal_load(group_bits + (grp >> 5)) >> (grp & 31)) & 1;
                __syncthreads();
                if (marked && tid == 0) atomicAnd(group_bits + (grp >> 5), ~(1 << (grp & 31)));
            }
            if (only_marked && !marked) continue;
            if (tid == 0 && net.fallbacks) atomicAdd(net.fallbacks + 1, (unsigned long long)(batch - b0 < G ? batch - b0 : G));
        }
        stamp();                                  // 0: group start
        stage_planes<S, G, C, 512>(smem, planes, b0, batch, tid);
        __syncthreads();

        // ---- stem: direct 6(8) -> 64 conv into buffer A; each half takes MTH M-tiles -------------
        {
            f32x4 acc[MTH];
#pragma unroll
            for (int m = 0; m < MTH; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float2 *w0 = reinterpret_cast<const float2 *>(net.w0frag) + wave * 9 * 64 + lane;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                const float2 bcur = w0[tap * 64];
                const int toff = ((tap / 3 - 1) * S + (tap % 3 - 1)) * 32;
#pragma unroll
                for (int m = 0; m < MTH; ++m) {
                    const int mt = half * MTH + m;
                    const int r = mt * 16 + li;
                    const int pb = r % P;
                    const int yy = pb / S + tap / 3 - 1, xx = pb % S + tap % 3 - 1;
                    const bool ok = r < M && yy >= 0 && yy < S && xx >= 0 && xx < S;
                    const int a = ok ? lane_in8 + mt * 16 * 32 + toff : lane_zero8;
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcur.x, lds_f32(smem, a), acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcur.y, lds_f32(smem, a + 16), acc[m], 0, 0, 0);
                }
            }
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(net.scale + wave * 16 + lg * 4);
            const f32x4 sh = *reinterpret_cast<const f32x4 *>(net.shift + wave * 16 + lg * 4);
#pragma unroll
            for (int m = 0; m < MTH; ++m) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(acc[m][j], sc[j], sh[j]), 0.f);
                const int r = (half * MTH + m) * 16 + li;
                if (r < M) *reinterpret_cast<f32x4 *>(smem + C::BUF_A + r * kWinoRowBytes + wave * 64 + lg * 16) = v;
                if (GS && r < M) *reinterpret_cast<f32x4 *>(gx + (size_t)r * 64 + wave * 16 + lg * 4) = v;
            }
        }
        __syncthreads();
        stamp();                                  // 1: stem done

#pragma unroll 1
        for (int layer = 1; layer < kConvLayers; ++layer) {
            const bool conv2 = (layer & 1) == 0;
            const int in_off = GS ? C::BUF_A : (conv2 ? C::BUF_B : C::BUF_A);
            const int out_off = conv2 ? C::BUF_A : C::BUF_B;
            float *gout = conv2 ? gx : gh;            // (GS) conv1 writes H, conv2 adds X and overwrites it
            const f32x4 *wl = reinterpret_cast<const f32x4 *>(net.wwino) +
                              ((size_t)((layer - 1) * 4 + wave) * 16) * 4 * 64 + lane;
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(net.scale + layer * 64 + wave * 16 + lg * 4);
            const f32x4 sh = *reinterpret_cast<const f32x4 *>(net.shift + layer * 64 + wave * 16 + lg * 4);
            // weight fragments: ring of 4 steps (one step = a pair of Winograd points = 8 MFMAs),
            // fetched three steps (~770 MFMA-pipe cycles) ahead of their use - an L2 hit takes ~500.
            // The (slice, step) sequence of a row-tile is the same for every row-tile, so the ring
            // simply wraps from the last step of one row-tile to the first of the next.
            f32x4 wq[4][2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                wq[r][0] = wl[(2 * r) * 64];
                wq[r][1] = wl[(2 * r + 1) * 64];
            }
#pragma unroll 1
            for (int it = 0; it < n_own; ++it) {
                // patch addresses of this row-tile: 3 VALU each from the per-lane geometry
                int brel = base_rel[0], brow = base_row[0];
                unsigned vm = valid[0];
#pragma unroll
                for (int r = 1; r < RTH; ++r) {
                    brel = it == r ? base_rel[r] : brel;
                    brow = it == r ? base_row[r] : brow;
                    vm = it == r ? valid[r] : vm;
                }
                const int base = in_off + brel;
                int a16[16];
#pragma unroll
                for (int pq = 0; pq < 16; ++pq) {
                    const int ok = ((int)(vm << (31 - pq))) >> 31;                  // -1 inside the board
                    const int addr = base + ((pq / 4) * S + (pq % 4)) * kWinoRowBytes;
                    a16[pq] = (addr & ok) | (lane_zero & ~ok);
                }
                f32x4 macc[16];
                // one work unit = (row-tile, 16-channel slice s).  The first slice is a second copy
                // of the body whose MFMAs start from a zero literal (no 64-register clearing sweep).
                auto unit = [&](const int s, auto first_tag) {
                    constexpr bool FIRST = decltype(first_tag)::value;
                    f32x4 d[16];
#pragma unroll
                    for (int pq = 0; pq < 16; ++pq) {
                        d[pq] = lds_f32x4(smem, a16[pq]);
                        a16[pq] += 64;                       // next 16-channel slice (the zero row is 272 B wide)
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {            // V = B^T d B, columns then rows
                        const f32x4 d0 = d[q], d1 = d[4 + q], d2 = d[8 + q], d3 = d[12 + q];
                        d[q] = sub4(d0, d2);
                        d[4 + q] = d1 + d2;
                        d[8 + q] = sub4(d2, d1);
                        d[12 + q] = sub4(d1, d3);
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const f32x4 t0 = d[4 * a], t1 = d[4 * a + 1], t2 = d[4 * a + 2], t3 = d[4 * a + 3];
                        d[4 * a] = sub4(t0, t2);
                        d[4 * a + 1] = t1 + t2;
                        d[4 * a + 2] = sub4(t2, t1);
                        d[4 * a + 3] = sub4(t1, t3);
                    }
                    // the wave that is in its MFMA phase goes first on this SIMD; its partner is in
                    // its load + transform phase and fills the issue slots the MFMAs leave
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int st = 0; st < 8; ++st) {
                        const int xp = 2 * st;
                        {   // fetch the pair used three steps from now (wraps into the next slice / row-tile)
                            const int f = st + 3;
                            const int nx = 2 * (f & 7);
                            const int ns = f < 8 ? s : ((s + 1) & 3);
                            wq[f & 3][0] = wl[(ns * 16 + nx) * 64];
                            wq[f & 3][1] = wl[(ns * 16 + nx + 1) * 64];
                        }
                        __builtin_amdgcn_sched_barrier(0);       // keep the fetch at the head of its step
                        const f32x4 b0v = wq[st & 3][0], b1v = wq[st & 3][1];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const f32x4 c0 = (FIRST && j == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : macc[xp];
                            const f32x4 c1 = (FIRST && j == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : macc[xp + 1];
                            macc[xp] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0v[j], d[xp][j], c0, 0, 0, 0);
                            macc[xp + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1v[j], d[xp + 1][j], c1, 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    __builtin_amdgcn_s_setprio(0);
                };
                unit(0, std::true_type{});
#pragma unroll 1
                for (int s = 1; s < 4; ++s) unit(s, std::false_type{});
                // (GS) the block input of the four output cells comes from the scratch image: request it
                // before the output transform so that its latency overlaps the transform
                f32x4 resid[4];
                if (GS && conv2) {
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        const int py = 1 + (o >> 1), px = 1 + (o & 1);
                        const bool ok = (vm >> (py * 4 + px)) & 1u;
                        resid[o] = ok ? *reinterpret_cast<const f32x4 *>(gout + (size_t)(brow + py * S + px) * 64 + wave * 16 + lg * 4)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {                // Y = A^T M A
                    const f32x4 m0 = macc[b] + macc[4 + b] + macc[8 + b];
                    const f32x4 m1 = sub4(sub4(macc[4 + b], macc[8 + b]), macc[12 + b]);
                    macc[b] = m0;
                    macc[4 + b] = m1;
                }
                f32x4 yv[4];
                yv[0] = macc[0] + macc[1] + macc[2];
                yv[1] = sub4(sub4(macc[1], macc[2]), macc[3]);
                yv[2] = macc[4] + macc[5] + macc[6];
                yv[3] = sub4(sub4(macc[5], macc[6]), macc[7]);
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int py = 1 + (o >> 1), px = 1 + (o & 1);     // output o sits on patch cell (py, px)
                    if ((vm >> (py * 4 + px)) & 1u) {
                        f32x4 v;
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = fmaf(yv[o][j], sc[j], sh[j]);
                        if (GS) {
                            f32x4 *dst = reinterpret_cast<f32x4 *>(gout + (size_t)(brow + py * S + px) * 64 + wave * 16 + lg * 4);
                            if (conv2) v += resid[o];
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                            *dst = v;
                        } else {
                            unsigned char *dst = smem + out_off + brel + (py * S + px) * kWinoRowBytes + wave * 64;
                            if (conv2) v += *reinterpret_cast<const f32x4 *>(dst);
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                            *reinterpret_cast<f32x4 *>(dst) = v;
                        }
                    }
                }
            }
            stamp();                              // 2 + 2k: layer work of this wave done
            if (GS) {
                // outputs are in the scratch image: make them visible, wait until every wave has
                // finished reading the LDS input, then load them as the next layer's input
                // workgroup scope is enough (all waves share this CU's write-through L1); an agent-scope
                // fence writes back / invalidates L2 state and cost 3x the whole layer
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __syncthreads();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const f32x4 *src = reinterpret_cast<const f32x4 *>(gout);
                for (int e = tid; e < M * 16; e += 512)
                    *reinterpret_cast<f32x4 *>(smem + C::BUF_A + (e >> 4) * kWinoRowBytes + (e & 15) * 16) =
                        __builtin_nontemporal_load(src + e);
            }
            __syncthreads();
            stamp();                              // 3 + 2k: barrier passed
        }
        run_heads<S, G, C, 512>(smem, net, b0, batch, want_logits, policy, value, tid);
        __syncthreads();
        stamp();                                  // 26: heads done
    }
}

}  // namespace

// ======================================================================================
// host side
// ======================================================================================
namespace {

using tg::ForwardArgs;
using tg_fwd::Family;
using tg_fwd::ForwardPlan;

// (the grids are the plan's: forward_plan.h)
template <int S, int G>
int launch(tg_net *net, int grid, const ForwardArgs &a) {
    using C = FwdCfg<S, G>;
    static_assert(tg_fwd::direct_waves_per_simd(S, G) == C::WAVES_PER_SIMD, "forward_plan.h restates the direct kernel's workgroups per CU");
    auto kern = dualnet_fwd_kernel<S, G>;
    static std::atomic<uint64_t> configured{0};
    if (tg::first_on_device(configured, net->device))
        TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), C::LDS_BYTES, a.stream, net->dev, a.planes, a.batch,
                       a.want_logits, a.policy, a.value);
    TG_HIP(hipGetLastError());
    return TG_OK;
}

// a.flag set: the launch is the range guard behind an f16 launch (one 8-wave workgroup per CU either way)
template <int S, int G, bool GS = false>
int launch_wino8(tg_net *net, int grid, const ForwardArgs &a) {
    using C = WinoCfg<S, G, GS>;
    auto kern = dualnet_fwd_wino8_kernel<S, G, GS>;
    static std::atomic<uint64_t> configured{0};
    if (tg::first_on_device(configured, net->device))
        TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
    NetDev dev = net->dev;
    if (GS)
        if (int rc = tg::stream_scratch(net, a.stream, &dev.scratch)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), C::LDS_BYTES, a.stream, dev, a.planes, a.batch,
                       a.want_logits, a.policy, a.value, a.flag, a.bits, a.clear_next);
    TG_HIP(hipGetLastError());
    return TG_OK;
}

// Every exact-fp32 kernel that is built: what a plan can name, as a launch of its own or (Winograd) as a range guard
struct ExactRow {
    bool wino;
    int S, group;
    int (*launch)(tg_net *, int grid, const ForwardArgs &);
};
const ExactRow kExactRows[] = {
    {true, 19, 1, launch_wino8<19, 1, true>}, {false, 19, 1, launch<19, 1>}, {true, 9, 3, launch_wino8<9, 3>},
    {true, 9, 1, launch_wino8<9, 1>},         {true, 9, 2, launch_wino8<9, 2>}, {true, 13, 1, launch_wino8<13, 1>},
    {false, 13, 1, launch<13, 1>},            {false, 9, 3, launch<9, 3>},    {false, 9, 1, launch<9, 1>},
};

}  // namespace

namespace tg {
// Grid caps of the launches a thread queues (forward_plan.h): per launching thread, so a network handle shared by several group
// threads of a shard carries no launch state (round 6; until then two atomics on the handle, last writer wins).
LaunchCaps &launch_caps() {
    static thread_local LaunchCaps caps = [] {
        LaunchCaps c;
        if (const char *env = tg::knob("TG_FWD_TEST_GUARD_CAP")) c.guard = atoi(env);      // (experiments: caps outside a self-play move)
        return c;
    }();
    return caps;
}
}  // namespace tg

extern "C" {

size_t tg_net_param_count(int board_size) { return tg::make_layout(board_size).total; }

double tg_net_flops_per_position(int board_size) {
    const double p = (double)board_size * board_size, a = p + 1;
    double macs = p * 64 * 6 * 9 + 12.0 * p * 64 * 64 * 9;   // padding taps counted
    macs += p * 64 * 2 + 2 * p * a + p * 64 + p * 3;
    return 2.0 * macs;
}

int tg_net_board_size(const tg_net *net) { return net ? net->board_size : 0; }

int tg_net_create(int board_size, int device, const float *params, size_t n_params, tg_net **out) {
    if (!out || !params) return tg::fail(TG_ERR_ARG, "tg_net_create: null argument");
    // 9 and 19 have the f16-pipe towers; 13 runs on the exact-fp32 direct kernel (dualnet_fwd_kernel<13, 1>: generic in the
    // board size, fp32 MFMA) - the reference's results within the same 1e-4, a fraction of the speed - unless TG_FWD_ALGO=split16
    // asks for the split-operand tower (dualnet_fwd_split_kernel<13, 1>; its weight image is built below for every size)
    if (board_size != 9 && board_size != 19 && board_size != 13)
        return tg::fail(TG_ERR_ARG, "tg_net_create: board size %d not built (9, 13 and 19 are)", board_size);
    if (n_params != tg_net_param_count(board_size))
        return tg::fail(TG_ERR_ARG, "tg_net_create: expected %zu parameters, got %zu",
                        tg_net_param_count(board_size), n_params);
    TG_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    TG_HIP(hipGetDeviceProperties(&prop, device));
    std::unique_ptr<tg_net> owner(new tg_net);         // (every early return below releases what the handle owns so far)
    tg_net *net = owner.get();
    net->board_size = board_size;
    net->device = device;
    net->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

    const int P = board_size * board_size;
    const tg::ParamLayout L = tg::make_layout(board_size);
    const tg::ExactImages exact = tg::exact_images(params, L, board_size);
    int rc = TG_OK;
    {
        tg::DevBuf<unsigned char> counters;
        if ((rc = counters.alloc_zeroed(2 * sizeof(unsigned long long)))) return rc;
        net->dev.fallbacks = reinterpret_cast<unsigned long long *>(counters.get());
        net->allocs.push_back(std::move(counters));
    }
    if (board_size == 19) {
        if ((rc = net->band_timeouts.alloc(1, hipHostMallocMapped))) return rc;
        *net->band_timeouts.get() = 0u;
        net->dev.band_timeouts = net->band_timeouts.dev();
        // a GTP / engine process that shares its GPU with other processes and never calls tg_net_set_shared_device
        if (const char *env = getenv("TG_SHARED_DEVICE")) net->shared_device = atoi(env) != 0;
    }

    // scratch images of the 19x19 Winograd kernel: 2 x [P][64] floats per workgroup, allocated per
    // launch stream on first use (tg::stream_scratch)
    if (board_size == 19) net->scratch_floats = (size_t)net->num_cus * 2 * P * 64;
    using tg::upload;
    if ((rc = upload(net, exact.w0frag, &net->dev.w0frag)) || (rc = upload(net, exact.wfrag, &net->dev.wfrag)) ||
        (rc = upload(net, exact.wwino, &net->dev.wwino)) || (rc = upload(net, exact.scale, &net->dev.scale)) ||
        (rc = upload(net, exact.shift, &net->dev.shift)) || (rc = upload(net, exact.hp_w, &net->dev.hp_w)) ||
        (rc = upload(net, exact.hv_w, &net->dev.hv_w)) || (rc = upload(net, exact.head_ss, &net->dev.head_ss)) ||
        (rc = upload(net, exact.pfc_wT, &net->dev.pfc_wT)) || (rc = upload(net, exact.pfc_b, &net->dev.pfc_b)) ||
        (rc = upload(net, exact.vfc_w, &net->dev.vfc_w)) || (rc = upload(net, exact.vfc_b, &net->dev.vfc_b)) ||
        (board_size == 9 && (rc = tg::heads_prepare(net, params, L, exact))) ||
        (rc = tg::split_prepare(net, params, L, exact)) || (rc = tg::w1d_prepare(net, params, L, exact)))
        return rc;
    *out = owner.release();
    return TG_OK;
}

int tg_net_destroy(tg_net *net) {
    if (!net) return TG_OK;
    (void)hipSetDevice(net->device);
    delete net;                                        // (its members release what they own)
    return TG_OK;
}

// What plan_forward (forward_plan.h) is asked with: the network's shape and state, this thread's caps, and every forward knob -
// read HERE and nowhere else under csrc/net_forward*.hip (but TG_SHARED_DEVICE at tg_net_create and launch_caps' own start
// value).  TG_FWD_ALGO, TG_FWD_BANDS, TG_FWD_GROUP, TG_FWD_WINO, TG_SPLIT_SPAN and the three test switches at every call (tests
// change them between calls), TG_FWD_NO_TAIL, TG_FWD_SPREAD_GUARD and TG_FWD_CUS once per process - the launch path and the
// name / FLOP queries must agree on them; all through tg::knob but TG_FWD_ALGO, which a deployment sets.  The band time-out
// counter, which the device may change at any moment, and the caps are read once per plan: the kernel, its grid and its flag
// words come from the same reading.
struct ForwardContext { tg_fwd::PlanInputs in; tg_fwd::ForwardKnobs knobs; };

static ForwardContext forward_context(const tg_net *net, int batch) {
    static const tg_fwd::ForwardKnobs once = [] {
        tg_fwd::ForwardKnobs k;
        k.no_tail = tg::knob("TG_FWD_NO_TAIL") != nullptr;
        k.spread_guard_off = tg_fwd::parse_int(tg::knob("TG_FWD_SPREAD_GUARD"), 1) == 0;
        k.fwd_cus = tg_fwd::parse_int(tg::knob("TG_FWD_CUS"), 0);
        return k;
    }();
    ForwardContext c;
    c.knobs = once;
    c.knobs.algo = tg_fwd::parse_algo(getenv("TG_FWD_ALGO"));
    c.knobs.bands = tg_fwd::parse_bands(tg::knob("TG_FWD_BANDS"));
    c.knobs.group = tg_fwd::parse_int(tg::knob("TG_FWD_GROUP"), 0);
    c.knobs.wino = tg_fwd::parse_int(tg::knob("TG_FWD_WINO"), 0);
    c.knobs.split_span = tg_fwd::parse_int(tg::knob("TG_SPLIT_SPAN"), 0);
    c.knobs.band_mute = tg_fwd::parse_int(tg::knob("TG_BAND_TEST_MUTE"), -1);
    c.knobs.pair_mute = tg::knob("TG_WB_TEST_MUTE") != nullptr;
    c.knobs.flag_memset = tg::knob("TG_FWD_FLAG_MEMSET") != nullptr;
    c.in.S = net->board_size;
    c.in.batch = batch;
    c.in.num_cus = net->num_cus;
    c.in.spread_w1d = net->spread_w1d;
    c.in.spread_split = net->spread_split;
    c.in.shared_device = net->shared_device;
    c.in.band_timeouts = net->band_timeouts_seen();
    c.in.caps = tg::launch_caps();
    return c;
}

// The plan of a call, and - once per process each - the word about a network that was kept off the f16 family it would have had
static ForwardPlan plan_call(const ForwardContext &c) {
    const ForwardPlan plan = tg_fwd::plan_forward(c.in, c.knobs);
    static std::atomic<bool> warned[4] = {};
    if (plan.demoted == tg_fwd::Demoted::None || warned[(int)plan.demoted].exchange(true)) return plan;
    if (plan.demoted == tg_fwd::Demoted::BandTimeouts) {
        // The switch is permanent for this network and changes the rounding of every later 19x19 pass (the timed-out launch itself
        // was redone in exact fp32): a game played across the switch is not bit-reproducible.
        fprintf(stderr, "[tamago_hip] warning: a 19x19 band-pair forward launch ran into its bounded wait (%u time-outs); this network "
                "stays on one-workgroup kernels from here on (different rounding, within the 1e-4 contract).  TG_SHARED_DEVICE=1 "
                "or tg_net_set_shared_device avoids the pair kernel from the start.\n", c.in.band_timeouts);
        return plan;
    }
    const bool w1d = plan.demoted == tg_fwd::Demoted::SpreadW1d;
    fprintf(stderr, "[tamago_hip] warning: the input channels of a tower layer of this network spread over a factor %.3g (limit of the %s "
            "f16 kernels: %.3g); beyond the limit their results leave the fp32-class contract, so this network's forward passes run "
            "on the next safer kernel (tg_net_kernel_name says which; slower).\n", w1d ? c.in.spread_w1d : c.in.spread_split,
            w1d ? "one-axis Winograd" : "direct split", w1d ? tg_fwd::kSpreadLimitW1d : tg_fwd::kSpreadLimitSplit);
    return plan;
}

const char *tg_net_kernel_name(const tg_net *net, int batch) {
    if (!net) return "";
    return tg_fwd::kernel_name(plan_call(forward_context(net, batch)));
}

double tg_net_executed_flops_per_position(const tg_net *net, int batch, double *peak_tflops, const char **dtype) {
    if (!net) return 0.0;
    const ForwardContext c = forward_context(net, batch);
    (void)plan_call(c);                                    // (a demoted network is told so by whichever query sees it first)
    const tg_fwd::Executed e = tg_fwd::executed(c.in, c.knobs);
    if (peak_tflops) *peak_tflops = e.peak;
    if (dtype) *dtype = e.dtype;
    return e.flops;
}

// The exact-fp32 kernels: a launch of their own, or the Winograd kernel <S, group> queued behind an f16 launch as its range guard.
static int launch_exact(tg_net *net, bool wino, int group, int grid, const ForwardArgs &a) {
    for (const ExactRow &r : kExactRows)
        if (r.wino == wino && r.S == net->board_size && r.group == group) return r.launch(net, grid, a);
    return tg::fail(TG_ERR_STATE, "forward: no exact kernel <%d, %d> (%s) is built", net->board_size, group, wino ? "Winograd" : "direct");
}


// The words an f16 launch and the guard launch behind it talk through, leased from the launch stream's state.
//   [range flag, group tickets] x 2: a stream's launches alternate between the two sets, and the guard launch behind
//   launch k clears the set of launch k + 1 (no memset node in front of a forward pass: ~8 us per launch with its gap -
//   five per single-tree move, a dozen per self-play move).  Rounds 3 and 4 took the memset out twice and put it back
//   twice: the 2 048-tree bench lost 20 % without it, because the node happened to let the next mini-batch's 344 MB
//   random window - then uploaded from the host - slip under the forward pass.  That upload is gone (round 6).
//   19x19 one-workgroup and banded direct kernels: a set of their own behind the two ([range flag, -, the banded kernel's
//   sequence numbers]), cleared in front of every launch.
//   bits: the one-axis kernels and the 13x13 kernel mark the groups that left the range - the exact kernel redoes those only;
//   the direct split kernels raise the flag alone: the whole batch.  At least one bit per group, all zero between launches
//   (allocated zeroed; every consumer clears what it read).  Growing the bitmap frees the old one: hipFree waits for the
//   device, nothing can still be using it.
struct GuardLease { int *words = nullptr, *flag = nullptr, *flag_next = nullptr, *bits = nullptr; size_t bit_words = 0; unsigned seq = 0; };

static int lease_guard(tg_net *net, hipStream_t st, const ForwardPlan &plan, int batch, bool flag_memset, GuardLease *out) {
    // (cleared in the launching stream's order: hipMemset on device memory returns before the fill has run, and the null
    // stream it runs on does not order a non-blocking stream - a first launch there took its group tickets from whatever
    // the allocation held)
    const auto zeroed = [st](tg::DevBuf<int> &buf, size_t count) {
        if (int rc = buf.reserve(count)) return rc;
        if (const hipError_t e = hipMemsetAsync(buf.get(), 0, count * sizeof(int), st); e != hipSuccess) {
            buf.reset();
            return tg::fail(TG_ERR_HIP, "forward guard words: hipMemsetAsync failed: %s", hipGetErrorString(e));
        }
        return (int)TG_OK;
    };
    GuardLease g;
    {
        std::lock_guard<std::mutex> lock(net->scratch_mu);
        tg_net::StreamState &ss = net->streams[st];
        if (!ss.flags.get())
            if (int rc = zeroed(ss.flags, net->board_size == 19 ? 4 + 2 + kBandFlagInts : 4)) return rc;
        g.words = ss.flags.get();
        g.seq = ss.seq;
        if (plan.family == Family::Pair19 || plan.family == Family::W1d9 || plan.family == Family::Split13) {
            g.bit_words = (size_t)((batch + plan.group - 1) / plan.group + 31) / 32;
            if (ss.bits.capacity() < g.bit_words)
                if (int rc = zeroed(ss.bits, g.bit_words < 2048 ? 2048 : g.bit_words)) return rc;
            g.bits = ss.bits.get();
        }
    }
    if (plan.family == Family::Split19 || plan.family == Family::Band19) {
        g.flag = g.words + 4;
        TG_HIP(hipMemsetAsync(g.flag, 0, (plan.bands ? 2 + kBandFlagInts : 2) * sizeof(int), st));
    } else {
        g.flag = g.words + 2 * (g.seq & 1u);
        g.flag_next = g.words + 2 * ((g.seq + 1u) & 1u);
        if (flag_memset) TG_HIP(hipMemsetAsync(g.flag, 0, 2 * sizeof(int), st));   // (TG_FWD_FLAG_MEMSET, experiments: the node back)
    }
    *out = g;
    return TG_OK;
}

// rc: what queueing the f16 launch and its guard launch returned.  Both queued: the stream's sequence number advances.  Not:
// it stays where it was, and - the f16 launch may have raised the flag and marked groups that no redo will consume - both
// alternating sets and the bitmap are cleared in stream order, so that the next launch starts clean (best effort: the
// stream may be broken).
static int settle_guard(tg_net *net, hipStream_t st, const GuardLease &g, int rc) {
    if (rc == TG_OK) {
        std::lock_guard<std::mutex> lock(net->scratch_mu);
        net->streams[st].seq = g.seq + 1u;
        return TG_OK;
    }
    (void)hipMemsetAsync(g.words, 0, 4 * sizeof(int), st);
    if (g.bits) (void)hipMemsetAsync(g.bits, 0, g.bit_words * sizeof(int), st);
    return rc;
}

int tg_net_forward_dev(tg_net *net, const float *planes_dev, int batch, int want_logits,
                       float *policy_dev, float *value_dev, void *stream) {
    if (batch < 0) return tg::fail(TG_ERR_ARG, "tg_net_forward_dev: negative batch");
    if (batch == 0) return TG_OK;
    if (!net || !planes_dev || !policy_dev || !value_dev)
        return tg::fail(TG_ERR_ARG, "tg_net_forward_dev: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ForwardContext ctx = forward_context(net, batch);
    const ForwardPlan plan = plan_call(ctx);
    if (plan.tail > 0) {
        // Tail of a batch that is not a whole number of rounds: a round = one 3-board workgroup on each of the CUs
        // (142 us); up to num_cus leftover positions are cheaper as ONE round of 1-board workgroups (80 us) than as
        // one more, mostly empty round of 3-board workgroups - the two launches follow each other on the stream.
        // (Self-play phases: 16 boards x 100 / 108 leaves = 2 rounds + 64 / 192 positions.)
        const int head = batch - plan.tail;
        const size_t P = 81, A = 82;
        if (int rc = tg_net_forward_dev(net, planes_dev, head, want_logits, policy_dev, value_dev, stream)) return rc;
        return tg_net_forward_dev(net, planes_dev + (size_t)head * 6 * P, plan.tail, want_logits,
                                  policy_dev + (size_t)head * A, value_dev + (size_t)head * 3, stream);
    }
    ForwardArgs a{planes_dev, batch, want_logits, policy_dev, value_dev, st};
    if (!plan.guarded) return launch_exact(net, plan.family == Family::Wino, plan.group, plan.grid, a);
    // f16 kernel on the 16-bit matrix pipe.  A range flag (per launch stream) makes the exact-fp32 Winograd kernel, queued
    // right behind, redo the batch - or the groups marked in the bitmap - if a layer output left the f16 range; with the flag
    // clear that launch exits at once.
    GuardLease g;
    if (int rc = lease_guard(net, st, plan, batch, ctx.knobs.flag_memset, &g)) return rc;
    a.flag = g.flag, a.bits = g.bits, a.clear_next = g.flag_next, a.band_flags = g.flag + 2;
    a.band_mute = ctx.knobs.band_mute, a.pair_mute = ctx.knobs.pair_mute;
    int rc = TG_OK;
    switch (plan.family) {
    case Family::Pair19: rc = tg::w1dband_forward(net, plan, a); break;
    case Family::Band19: rc = tg::band_forward(net, plan, a); break;
    case Family::W1d9: rc = tg::w1d_forward(net, plan, a); break;
    default: rc = tg::split_forward(net, plan, a); break;   // Split9, Split13, Split19
    }
    if (rc == TG_OK) rc = launch_exact(net, true, plan.group, plan.guard_grid, a);
    return settle_guard(net, st, g, rc);
}

int tg_net_range_fallbacks(tg_net *net, unsigned long long *count) {
    if (!net || !count) return tg::fail(TG_ERR_ARG, "tg_net_range_fallbacks: null argument");
    TG_HIP(hipSetDevice(net->device));
    TG_HIP(hipDeviceSynchronize());
    TG_HIP(hipMemcpy(count, net->dev.fallbacks, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return TG_OK;
}

int tg_net_range_fallback_positions(tg_net *net, unsigned long long *count) {
    if (!net || !count) return tg::fail(TG_ERR_ARG, "tg_net_range_fallback_positions: null argument");
    TG_HIP(hipSetDevice(net->device));
    TG_HIP(hipDeviceSynchronize());
    TG_HIP(hipMemcpy(count, net->dev.fallbacks + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return TG_OK;
}

int tg_net_band_timeouts(tg_net *net, unsigned long long *count) {
    if (!net || !count) return tg::fail(TG_ERR_ARG, "tg_net_band_timeouts: null argument");
    TG_HIP(hipSetDevice(net->device));
    TG_HIP(hipDeviceSynchronize());
    *count = net->band_timeouts_seen();
    return TG_OK;
}

double tg_net_channel_spread(const tg_net *net, int image) {
    if (!net) return 0.0;
    return image == 0 ? net->spread_w1d : net->spread_split;
}

int tg_net_set_shared_device(tg_net *net, int shared) {
    if (!net) return tg::fail(TG_ERR_ARG, "tg_net_set_shared_device: null argument");
    net->shared_device = shared != 0;
    return TG_OK;
}

int tg_net_profile_phases(tg_net *net, const float *planes_dev, int batch, float *policy_dev, float *value_dev,
                          long long *stamps_host, int n_stamps) {
    if (!net || !planes_dev || !policy_dev || !value_dev || !stamps_host || n_stamps < 1 || n_stamps > 128)
        return tg::fail(TG_ERR_ARG, "tg_net_profile_phases: bad argument");
    TG_HIP(hipSetDevice(net->device));
    long long *tl = nullptr;
    TG_HIP(hipMalloc(reinterpret_cast<void **>(&tl), 128 * sizeof(long long)));
    TG_HIP(hipMemset(tl, 0, 128 * sizeof(long long)));
    net->dev.timeline = tl;
    int rc = tg_net_forward_dev(net, planes_dev, batch, 0, policy_dev, value_dev, nullptr);
    net->dev.timeline = nullptr;
    if (rc == TG_OK) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(stamps_host, tl, n_stamps * sizeof(long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = tg::fail(TG_ERR_HIP, "tg_net_profile_phases: %s", hipGetErrorString(e));
    }
    (void)hipFree(tl);
    return rc;
}

int tg_net_forward_host(tg_net *net, const float *planes_host, int batch, int want_logits,
                        float *policy_host, float *value_host) {
    if (batch <= 0) return batch == 0 ? TG_OK : tg::fail(TG_ERR_ARG, "negative batch");
    if (!net || !planes_host || !policy_host || !value_host)
        return tg::fail(TG_ERR_ARG, "tg_net_forward_host: null argument");
    std::lock_guard<std::mutex> lock(net->host_mu);
    TG_HIP(hipSetDevice(net->device));
    const size_t P = (size_t)net->board_size * net->board_size, A = P + 1;
    int rc;
    if ((rc = net->st_planes.reserve(batch * 6 * P)) || (rc = net->st_policy.reserve(batch * A)) || (rc = net->st_value.reserve(batch * 3)))
        return rc;
    TG_HIP(hipMemcpy(net->st_planes.get(), planes_host, batch * 6 * P * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = tg_net_forward_dev(net, net->st_planes.get(), batch, want_logits, net->st_policy.get(), net->st_value.get(), nullptr))) return rc;
    TG_HIP(hipMemcpy(policy_host, net->st_policy.get(), batch * A * sizeof(float), hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(value_host, net->st_value.get(), batch * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return TG_OK;
}

}  // extern "C"
