/*
 * tamago_hip.h - C ABI of libtamago_hip.so, the MI355X (gfx950) implementation of
 * TamaGo's batched MCTS leaf-evaluation path.
 *
 * The reference (kobanium/TamaGo @ 2024-12-20) is 100 % Python and has no FFI of its
 * own; each entry point below replaces the Python function(s) cited next to it, and is
 * what a ctypes binding inside the reference would call (see INTEGRATION.md for the
 * exact stubs).  Conventions:
 *   - every function returns 0 on success, a negative tg_status on failure; the
 *     message is available from tg_last_error() (thread-local);
 *   - handles are opaque; a handle is bound to one HIP device and is NOT thread-safe;
 *   - "host" pointers are caller-owned host memory, "dev" pointers are caller-owned
 *     device memory on the handle's device (e.g. torch tensors' data_ptr());
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls that
 *     take a stream only ENQUEUE work; the *_host convenience calls synchronise.
 *   - board coordinates follow the reference: pos = x + y*(S+2) on the padded board,
 *     PASS = 0, RESIGN = -1 (board/constant.py:4-31); colours EMPTY 0 / BLACK 1 /
 *     WHITE 2 / OUT_OF_BOARD 3 (board/stone.py:5-11).
 */
#ifndef TAMAGO_HIP_H
#define TAMAGO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum tg_status {
    TG_OK = 0,
    TG_ERR_ARG = -1,      /* bad argument                          */
    TG_ERR_HIP = -2,      /* HIP runtime error (no GPU, OOM, ...)  */
    TG_ERR_STATE = -3,    /* call sequence violated                */
    TG_ERR_OVERFLOW = -4  /* node pool / RNG window exhausted      */
} tg_status;

/* ---- library ------------------------------------------------------------------------ */
int tg_abi_version(void);                 /* increases on every incompatible change      */
const char *tg_last_error(void);          /* message of the last failing call            */
int tg_device_count(int *count);          /* replaces nn/utility.py:12-24 get_torch_device */

/* ---- DualNet forward (nn/network/dual_net.py:41-106, res_block.py:8-38,
 *      head/policy_head.py:7-39, head/value_head.py:7-39) ------------------------------- */
typedef struct tg_net tg_net;

/* Number of floats tg_net_create expects for a board size: the reference state_dict
 * (nn/utility.py:139-159) flattened in this key order, num_batches_tracked skipped:
 *   conv_layer.weight [64,6,3,3]; bn_layer.{weight,bias,running_mean,running_var} [64];
 *   for b in 0..5: blocks.b.conv1.weight, blocks.b.conv2.weight [64,64,3,3],
 *                  blocks.b.bn1.{w,b,mean,var}, blocks.b.bn2.{w,b,mean,var} [64];
 *   policy_head.conv_layer.weight [2,64,1,1]; policy_head.bn_layer.{w,b,mean,var} [2];
 *   policy_head.fc_layer.weight [A,2P]; policy_head.fc_layer.bias [A];
 *   value_head.conv_layer.weight [1,64,1,1]; value_head.bn_layer.{w,b,mean,var} [1];
 *   value_head.fc_layer.weight [3,P]; value_head.fc_layer.bias [3].       (P=S*S, A=P+1) */
size_t tg_net_param_count(int board_size);

/* Build a network on `device` from raw (un-folded) fp32 parameters; BatchNorm (eval
 * mode, eps 1e-5 stem / 2e-5 elsewhere) is folded and the 3x3 weights are re-ordered
 * into MFMA fragment order on the host.  Replaces load_network, nn/utility.py:139-159. */
int tg_net_create(int board_size, int device, const float *params, size_t n_params,
                  tg_net **out);
int tg_net_destroy(tg_net *net);
int tg_net_board_size(const tg_net *net);

/* Forward pass on device-resident planes [B,6,S,S] fp32 -> policy [B,A], value [B,3].
 * want_logits = 0: softmax(policy), softmax(value)     (DualNet.inference, :81-91)
 * want_logits = 1: raw policy logits, softmax(value)   (inference_with_policy_logits, :94-106) */
int tg_net_forward_dev(tg_net *net, const float *planes_dev, int batch, int want_logits,
                       float *policy_dev, float *value_dev, void *stream);
/* Same with host buffers (H2D, kernel, D2H, synchronise) - the reference's own boundary:
 * host tensor in, host tensors out. */
int tg_net_forward_host(tg_net *net, const float *planes_host, int batch, int want_logits,
                        float *policy_host, float *value_host);
/* Profiling aid: one forward pass with workgroup 0 writing s_memtime stamps at its phase
 * boundaries (group start, stem, per layer: work done / barrier passed, heads done).
 * Direct kernel: wave 0 -> stamps [0,64).  Winograd kernel: wave 0 -> [0,64) and wave 4 (the
 * other wave of the same SIMD) -> [64,128).  n_stamps <= 128.  Synchronises. */
int tg_net_profile_phases(tg_net *net, const float *planes_dev, int batch, float *policy_dev,
                          float *value_dev, long long *stamps_host, int n_stamps);
/* Name (for rocprof) and algorithmic FLOPs per position of the dominant kernel. */
const char *tg_net_kernel_name(const tg_net *net, int batch);
double tg_net_flops_per_position(int board_size);
/* What the kernel tg_net_forward_dev picks for `batch` actually EXECUTES on the matrix pipe, per position:
 * FLOPs of the issued MFMA instructions including tile padding and operand splitting (split-operand f16
 * kernel: 3 MFMAs per product-sum over the direct 3x3 convolution, 243 of 256 rows used; Winograd fp32
 * kernel: 25 tiles x 16 points, 75 of 80 tiles used; direct fp32 kernel: 9 taps).  *peak_tflops receives
 * the dense matrix peak of the precision those instructions run in (MI355X: 2500 f16, 157.3 fp32),
 * *dtype its name.  The roofline fraction of the forward kernel is executed FLOP/s over that peak. */
double tg_net_executed_flops_per_position(const tg_net *net, int batch, double *peak_tflops,
                                          const char **dtype);
/* The split-operand kernels compute in f16 pieces: a layer output beyond the f16 range raises a flag on the device and the
 * exact-fp32 kernel queued behind every launch redoes that batch (same results, ~2.5x the time; no host round trip).
 * *count receives the number of forward launches of this network that were redone so far - a network whose activations
 * run hot shows up here instead of only as a slower search.  Synchronises the device.  (No reference counterpart: the
 * reference computes in fp32 throughout, nn/network/dual_net.py:41-52.) */
int tg_net_range_fallbacks(tg_net *net, unsigned long long *count);
/* ... and how many POSITIONS the exact-fp32 kernel redid in those launches.  The one-axis Winograd kernels (the defaults at both
 * board sizes) mark the workgroup passes - 3 boards (1 in small launches) at 9x9, one board at 19x19 - whose activations left
 * the f16 range, and the exact kernel redoes those only: one hot position in a launch of half a million costs three positions'
 * redo, not the launch's.  (The direct split kernels and a band's time-out redo the whole launch.)  Synchronises the device. */
int tg_net_range_fallback_positions(tg_net *net, unsigned long long *count);
/* 19x19: launches of up to 128 boards spread a board over 2 / 4 workgroups that exchange halo rows through L2 with BOUNDED
 * waits.  *count receives how many of those waits gave up so far (each ends in the exact-fp32 redo above, so it is also
 * part of tg_net_range_fallbacks' count - this one tells the two causes apart).  After the first one the network keeps to
 * the one-workgroup kernel: somebody else's kernels hold this GPU's compute units.  Synchronises the device. */
int tg_net_band_timeouts(tg_net *net, unsigned long long *count);
/* shared != 0: other PROCESSES drive this GPU too (the reference's `--process N` on one device, nn/utility.py:22,
 * selfplay_main.py:44-65 with more workers than GPUs).  Kernels that need several workgroups of one launch resident at the
 * same time (the banded 19x19 forward) are not chosen then.  Results do not depend on this switch. */
int tg_net_set_shared_device(tg_net *net, int shared);
/* Load-time guard of the f16 towers.  A weight image has ONE power-of-two scaling per layer and the activations none per
 * channel, so a tower layer whose input channels differ widely in magnitude (an input channel with weights 2^S times another's
 * carries activations about 2^S times smaller) loses low-piece bits on both operands.  Returns the largest spread of a
 * tower layer - largest weight of an input channel, the largest of the 64 over the smallest non-zero one - in image 0 (one-axis
 * Winograd: 9x9 default, 19x19 pair kernel; batch norm folded in, low pieces unscaled) or 1 (direct split kernels; raw weights,
 * low pieces x 2048): about 1 for an ordinary network.  Beyond a measured limit (net_forward.hip, kSpreadLimit*) the family
 * is not chosen for this network whatever TG_FWD_ALGO says - one-axis Winograd -> direct split -> exact fp32 - one warning
 * line goes to stderr, and tg_net_kernel_name / tg_net_executed_flops_per_position report the kernel that runs. */
double tg_net_channel_spread(const tg_net *net, int image);

/* ---- featurise (nn/feature.py:10-57 + go_board.py:468-478) -------------------------- */
/* cells_dev: uint8 [B, P] on-board cell colours, row-major from the top-left point;
 * to_move: int8 [B] (1 black / 2 white); prev_move: int32 [B] padded-board coordinate of
 * the previous move (0 = PASS); moves: int32 [B] the board's move counter (starts at 1).
 * Writes fp32 planes [B,6,S,S]. */
int tg_featurize_dev(int board_size, const uint8_t *cells_dev, const int8_t *to_move_dev,
                     const int32_t *prev_move_dev, const int32_t *moves_dev, int batch,
                     float *planes_dev, void *stream);

/* Same with a board symmetry per position (sym_dev int8 [B], 0..7 as in go_board.py:80-104;
 * NULL = identity): the training-side call generate_input_planes(board, color, sym) of
 * nn/data_generator.py:108,125. */
int tg_featurize_sym_dev(int board_size, const uint8_t *cells_dev, const int8_t *to_move_dev,
                         const int32_t *prev_move_dev, const int32_t *moves_dev,
                         const int8_t *sym_dev, int batch, float *planes_dev, void *stream);

/* ---- batched tree search (mcts/tree.py, mcts/node.py, mcts/pucb/pucb.py,
 *      mcts/batch_data.py, board/ as called from the search) --------------------------- */
typedef struct tg_search tg_search;

typedef struct tg_search_config {
    int32_t board_size;      /* S: 9 or 19 (any 5..19)                                    */
    int32_t num_trees;       /* T independent search trees ("boards") driven in lock-step */
    int32_t tree_size;       /* nodes per tree (MCTSTree tree_size, tree.py:29)           */
    int32_t batch_size;      /* leaves per tree per mini-batch (NN_BATCH_SIZE)            */
    int32_t cgos_mode;       /* node.py:153-155                                           */
    int32_t check_superko;   /* GoBoard(check_superko=...), go_board.py:285-301           */
    int32_t device;
    int32_t reserved;
} tg_search_config;

/* Root position of one tree, as the reference's GoBoard holds it. */
typedef struct tg_root_position {
    const uint8_t *cells;        /* [(S+2)^2] padded board, colours incl. OUT_OF_BOARD    */
    const uint64_t *hash_history;/* [moves] positional hashes by move index (slot 0 = 0);
                                    may be NULL when check_superko == 0                    */
    uint64_t hash;               /* current positional hash                               */
    int32_t moves;               /* GoBoard.moves (1 = empty game)                         */
    int32_t ko_pos, ko_move;     /* go_board.py:173-177                                   */
    int32_t prev_move;           /* record.pos[moves-1] (0 = PASS / none)                 */
    int32_t prev_prev_move;      /* record.pos[moves-2]                                   */
    int32_t to_move;             /* 1 black / 2 white                                     */
} tg_root_position;

int tg_search_create(const tg_search_config *cfg, tg_search **out);
int tg_search_destroy(tg_search *s);

/* Zobrist keys uint64 [4][(S+2)^2] used for positional superko (board/zobrist_hash.py);
 * the caller owns the key table so that its own GoBoard hashes stay consistent. */
int tg_search_set_zobrist(tg_search *s, const uint64_t *keys, size_t n);

/* Stage the root position of tree `t` (copied; uploaded in bulk by the next
 * tg_search_root_planes, which resets the tree: tree.py:49-54 / :330-336). */
int tg_search_set_root(tg_search *s, int tree, const tg_root_position *pos);

/* Feed the per-tree random streams.  The reference draws the Dirichlet "tentative"
 * prior (tree.py:509-519) and Gumbel noise (node.py:275-278) from numpy's global
 * legacy MT19937 stream; bit-exact parity needs the host's libm log(), so the host
 * turns uniform doubles u_i into e_i = -log(1-u_i) and hands them over in stream
 * order: tree t consumes exp_stream[t*stride + cursor ...].  `count` values per tree.
 * The window is uploaded on a private copy stream into the inactive one of two device
 * windows and becomes active at the next root_planes / select call, so the host can
 * prepare mini-batch j+1 while the forward pass of mini-batch j is still running. */
int tg_search_set_rng(tg_search *s, const double *exp_stream_host, size_t stride, size_t count);
/* Doubles each tree consumed from the active window (host array [T]); waits only for the
 * last root_planes / select kernel, not for the forward or backup queued behind it. */
int tg_search_rng_consumed(tg_search *s, int64_t *consumed_host);

/* PUCT: run `max_leaves` (<= batch_size) descents per tree (tree.py:199-244 search_mcts:
 * select by PUCB, play, virtual loss, expand, featurise, queue).  Leaf planes go to
 * planes_dev [T, max_leaves, 6, S, S]; n_leaves_dev[T] (may be NULL) receives the number
 * queued per tree (== max_leaves unless the tree hit an error or is halted). */
int tg_search_select_puct(tg_search *s, int max_leaves, float *planes_dev, int32_t *n_leaves_dev,
                          void *stream);
/* n_batches PUCT mini-batches (leaves_host[b] descents per tree each) queued back to back on `stream`: one random window from the
 * library's streams for all of them (tg_search_feed_streams semantics, force_window as its `force`), then per mini-batch
 * tg_search_select_puct, tg_net_forward_dev (want_logits 0) and tg_search_backup - the launches of the per-mini-batch calls
 * without the host round trip between them.  For searches whose course does not depend on what a mini-batch found (the
 * reference's STRICT_PLAYOUT: no early stop, mcts/time_manager.py:160-161; mcts/tree.py:146-152).  policy_dev [T * batch_size, A],
 * value_dev [T * batch_size, 3] and planes_dev are reused by every mini-batch.  Afterwards: tg_search_advance_streams. */
int tg_search_puct_chain(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, int force_window,
                         float *planes_dev, float *policy_dev, float *value_dev, void *stream);

/* Halt words: one per tree.  While a tree's word is set, tg_search_select_puct (every kernel it launches) passes the tree by
 * exactly as it does a tree whose sticky error word is set - no descent, no node or virtual loss written, no draw taken
 * (its cursor stays), no plane written, 0 leaves queued, so tg_search_backup has nothing to do for it.  It is no error: the
 * Gumbel selection and every read-out ignore the word.  tg_search_root_planes clears every tree's word (it resets every
 * tree); a position staged with tg_search_set_root going up, tg_search_set_roots_from_records and tg_search_reroot clear the
 * words of the trees they give a root, and no other tree's.  A forward pass over a mini-batch still covers a halted tree's
 * plane slots, which hold what was there.
 * tg_search_set_halt: halt_host[T], non-zero = halt the tree, zero = leave its word alone.
 * tg_search_read_halt: waits for the launch stream; halt_host[T] 1 / 0, stopped_at_host[T] the root's visits when the stop
 * rule halted the tree (0: not halted, or halted by the host - a clear resets it with the word); either may be NULL. */
int tg_search_set_halt(tg_search *s, const uint8_t *halt_host, void *stream);
int tg_search_read_halt(tg_search *s, uint8_t *halt_host, int32_t *stopped_at_host);
/* One launch of the early-stop rule of a CONSTANT_PLAYOUT search (mcts/time_manager.py:146-163 is_move_decided) for every tree:
 * first, second = the two largest visit counts of the root's children (equal leaders: second == first); the tree is halted iff
 * total_host[t] - root visits < first - second.  Trees already halted, in error or without a root are left alone.  live_host
 * (NULL: the call does not wait) receives the number of trees the rule looked at and left running.  total_host[t] >= 1. */
int tg_search_stop_rule(tg_search *s, const int32_t *total_host, int32_t *live_host, void *stream);
/* tg_search_puct_chain with early stops: the rule is queued behind the backup of every FULL mini-batch (leaves_host[b] ==
 * leaves_host[0]) that has mini-batches to follow - where MCTSTree.search tests it (mcts/tree.py:150-152) - and after every
 * poll_every mini-batches the host waits for the live count and returns once it is 0 (poll_every >= n_batches: everything is
 * queued, nothing waited for).  *batches_run_host (may be NULL): the mini-batches queued.  The window covers all n_batches, as
 * the chain's; draws a halted tree did not take stay in it, and tg_search_advance_streams reports what each tree consumed.
 * TG_ERR_ARG: a NULL pointer, poll_every < 1, a total < 1; TG_ERR_STATE: no tg_search_root_planes since a root was set,
 * replaced or moved through this API (a host-side guard: what the device holds is not read). */
int tg_search_puct_chain_early(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, const int32_t *total_host,
                               int poll_every, int force_window, float *planes_dev, float *policy_dev, float *value_dev,
                               void *stream, int32_t *batches_run_host);

/* Idle trees compacted out of the forward passes of lock-step PUCT (opt-in - nothing above changes).  A tree is
 * LIVE when tg_search_select_puct would search it: no sticky error, no halt word, a root.  A live tree's rank is the number of
 * live trees before it; a tree that is not live has rank -1.  In the COMPACT layout tree t's leaf j of a mini-batch of
 * max_leaves descents has its planes, and the network its outputs, at row rank[t] * max_leaves + j, so a forward pass over
 * live * max_leaves positions covers every tree that searches.  Queue entries keep their places.
 * tg_search_compact_live: one launch that writes every tree's rank and the live count, behind everything queued on `stream`;
 * live_host (NULL: the call does not wait) receives the count.  The ranks are FRESH until a call writes halt words or resets
 * a root: tg_search_set_halt, tg_search_stop_rule, tg_search_root_planes, a staged root going up,
 * tg_search_set_roots_from_records, tg_search_reroot.  Nothing is allocated before the first call.
 * tg_search_read_live_rank: rank_host[T], a read-out for tests (waits for the launch stream, allocates nothing;
 * TG_ERR_STATE: no ranks were ever computed).
 * tg_search_select_puct_compact: tg_search_select_puct in the compact layout.  TG_ERR_STATE, before anything is launched, when
 * the ranks are not fresh.  shrunk_ok != 0: ranks are accepted that went stale ONLY through calls that set halt words
 * (tg_search_set_halt, tg_search_stop_rule) - the live set has only lost trees since, so every tree that searches still has
 * its rank and a tree halted since keeps an idle slot (the mini-batches between two polls of an early-stop search); ranks
 * from before a root reset are refused either way.  A tree that searches without a rank cannot occur.
 * tg_search_backup_compact: tg_search_backup of a compact selection (slots_per_tree: its max_leaves).  TG_ERR_ARG unless the
 * last selection was a compact one of the whole engine (not a Gumbel selection, not a move's sub-groups), and for the packed
 * and unique codes (0, -1) of slots_per_tree; tg_search_backup in turn refuses a strided backup of a compact selection. */
int tg_search_compact_live(tg_search *s, int32_t *live_host, void *stream);
int tg_search_read_live_rank(tg_search *s, int32_t *rank_host);
int tg_search_select_puct_compact(tg_search *s, int max_leaves, int shrunk_ok, float *planes_dev, int32_t *n_leaves_dev, void *stream);
int tg_search_backup_compact(tg_search *s, const float *policy_dev, const float *value_dev, int slots_per_tree, int use_logit,
                             void *stream);
/* tg_search_puct_chain (total_host NULL; poll_every ignored) or tg_search_puct_chain_early (total_host[T]) with compaction: the
 * call computes the ranks and reads the live count once before its first mini-batch, and at every poll it launches the rank
 * kernel behind the rule and reads ITS count, which stands in for the rule's live counter.  Ranks are never recomputed between
 * polls: within the call halt words are only set, so a tree that still searches has a rank below the count in force, and one
 * halted since the last poll keeps an idle slot until the next.  Every forward pass covers count * leaves_host[b] positions;
 * a count of 0 queues none.  *positions_host (may be NULL): the positions the call's forward passes covered. */
int tg_search_puct_chain_compact(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, const int32_t *total_host,
                                 int poll_every, int force_window, float *planes_dev, float *policy_dev, float *value_dev,
                                 void *stream, int32_t *batches_run_host, int64_t *positions_host);

/* Grouped ranks: the trees of several networks in one lock-step launch (opt-in - nothing above changes).
 * tg_search_group_live stands in for tg_search_compact_live: group_host[T] gives every tree a group in [0, n_groups),
 * 1 <= n_groups <= 64, and one launch behind everything queued on `stream` writes
 *     rank[t] = offset[group[t]] + the live trees of group[t] before tree t          (-1 for a tree that is not live)
 * with count[g] the live trees of group g and offset[g] the sum of count[g'] over g' < g - the live trees sorted by group, the
 * order of the trees kept within one.  The table is the one tg_search_compact_live writes: tg_search_select_puct_compact,
 * tg_search_backup_compact and tg_search_read_live_rank work on it unchanged, group g's leaves of a mini-batch of k descents
 * lie in the rows [offset[g] * k, (offset[g] + count[g]) * k), and FRESH / stale mean what they mean there.  The handle
 * remembers that the table in force is a grouped one; any call that computes plain live ranks replaces it
 * (tg_search_compact_live, the polls of tg_search_puct_chain_compact and tg_search_puct_chain_budget).  count_host[n_groups]
 * receives the counts: the call waits for `stream` once.  TG_ERR_ARG, before anything is launched: n_groups outside [1, 64],
 * a group id outside [0, n_groups).
 * tg_search_gather_rows_by_rank / tg_search_scatter_rows_by_rank stand in for the copy a host would make between the root
 * evaluation's rows (tg_search_root_planes: tree t at row t, tg_search_backup(slots_per_tree 1) reads row t) and a segment per
 * group: gather dst[rank[t]] = src[t], scatter dst[t] = src[rank[t]], rows of row_floats floats (6 S S planes, S S + 1
 * policy values, 3 value floats), both buffers T rows, a tree of rank -1 skipped.  TG_ERR_STATE without ranks in force.
 * tg_search_puct_chain_groups stands in for one tg_search_puct_chain_compact(total_host NULL) per network: per mini-batch ONE
 * compact selection by the grouped ranks in force, for every group g with count[g] > 0 one
 * tg_net_forward_dev(nets[g], count[g] * leaves_host[b] positions) on the rows from offset[g] * leaves_host[b] on, into the
 * policy and value rows of the same segment, ONE compact backup.  Strict: no early total, no budgets (TG_ERR_ARG while
 * budgets are in force).  The ranks are not recomputed.  *positions_host (may be NULL): the positions the forward passes
 * covered.  Refused before anything is launched - TG_ERR_ARG: n_groups outside [1, 64] or not the table's, a NULL network
 * for a group that has live trees (a group without live trees may have none), a network of another board size;
 * TG_ERR_STATE: the ranks in force are not fresh grouped ranks (the message says what replaced or outdated them). */
int tg_search_group_live(tg_search *s, const int32_t *group_host, int n_groups, int32_t *count_host, void *stream);
int tg_search_gather_rows_by_rank(tg_search *s, const float *src_dev, float *dst_dev, int row_floats, void *stream);
int tg_search_scatter_rows_by_rank(tg_search *s, const float *src_dev, float *dst_dev, int row_floats, void *stream);
int tg_search_puct_chain_groups(tg_search *s, tg_net *const *nets, int n_groups, const int32_t *leaves_host, int n_batches,
                                int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                                int64_t *positions_host);

/* Reset every tree to its root position, expand the root (consumes the root's Dirichlet
 * draw) and write the root planes [T,6,S,S] (tree.py:49-53); one leaf per tree is queued. */
int tg_search_root_planes(tg_search *s, float *planes_dev, void *stream);
/* Everything the Gumbel move choice and the improved policy need (node.py:281-346), for the
 * roots of all trees in one call; arrays are [T] / [T][A]; any pointer may be NULL. */
int tg_search_read_root_stats(tg_search *s, int32_t *num_children_host, int32_t *node_visits_host,
                              float *raw_value_host, int32_t *action_host, int32_t *visits_host,
                              int32_t *virtual_loss_host, double *value_sum_host,
                              double *policy_host);
/* Profiling aid: with enable != 0 the PUCT selection kernel accumulates s_memtime cycles of
 * tree 0 per phase into 16 counters (0 board reset, 1 PUCB select, 2 put_stone, 3 edge
 * bookkeeping, 4 expansion, 5 planes + queue, 7 = number of tree levels walked, 8-10
 * expansion detail: candidates / Dirichlet sum / node init); the call returns the counters
 * accumulated so far (cycles_host [16], may be NULL) and clears them. */
int tg_search_profile(tg_search *s, int enable, long long *cycles_host);
/* The kernel a launch of the whole engine would get, as `kernel<template parameters> grid=G block=B` in out[cap]: family 0
 * tg_search_select_puct(max_leaves = max_n), 1 tg_search_select_gumbel whose busiest tree makes max_n descents (unique != 0:
 * slots_per_tree -1), 2 tg_search_backup (unique likewise; max_n ignored).  The name of the plan the launcher itself would get
 * from the same call (DESIGN.md 4.4 "Search launch plans"); launches nothing - family 0 may make the handle's one occupancy query. */
int tg_search_launch_name(tg_search *s, int family, int max_n, int unique, char *out, size_t cap);
/* Play moves_host[t] (padded coordinate, 0 = PASS, -1 = leave the tree alone, -2 = the move of the most
 * visited child of the tree's root, node.py:167-175 get_best_move_index, chosen on the device: no
 * read-back between two searches) on the ROOT position of every tree on the device (GoBoard.put_stone,
 * go_board.py:131-185) and flip the side to move: self-play boards stay resident between searches. */
int tg_search_play(tg_search *s, const int32_t *moves_host, void *stream);
/* The move of a PUCT search, decided on the device for every tree in one launch (one wavefront per tree): the end of
 * search_best_move, mcts/tree.py:76-77 and :87-105 -
 *     if root.num_children == 1: return PASS                                   (whatever the root's statistics say)
 *     next_index = root.get_best_move_index()                                  (node.py:169-177: np.argmax, first maximum)
 *     if root.calculate_value_evaluation(next_index) < RESIGN_THRESHOLD: return RESIGN
 *     return root.action[next_index]                                           (node.py:364-369: value_sum / visits in float64,
 *                                                                               IEEE division; 0.5 for a child without visits)
 * - in place of tg_search_read_root_stats (seven [T][A] arrays, about 28 A bytes per tree) and a host loop: 32 bytes per tree.
 * records_host [T] receives one tg_best_move per tree.  resign_threshold: the reference's RESIGN_THRESHOLD is 0.05; 0.0
 * switches resignation off (a value is never negative).  play 1: the move is then played on the tree's root position exactly
 * as tg_search_play(move) plays it (RESIGN plays nothing); play 0: nothing is changed - called right after the root
 * evaluation this is how a driver learns which roots have one child.  sit_out_host [T] (may be NULL): trees with a non-zero
 * flag are neither read nor played, their record is zero but for status = TG_BEST_SAT_OUT.  Queued on `stream`; the call
 * waits for the records.  A tree whose root is not expanded: TG_ERR_STATE; a tree with its sticky error word set: that
 * error; neither is played.  TG_ERR_ARG: null handle or records, play not 0 / 1, a threshold that is not a number. */
typedef struct tg_best_move {
    int32_t num_children;        /* of the root                                                      */
    int32_t move;                /* padded coordinate, 0 = PASS, -1 = RESIGN                         */
    int32_t best;                /* the chosen root child (0 for a one-child root)                   */
    int32_t visits;              /* children_visits[best]                                            */
    double value_sum;            /* children_value_sum[best]                                         */
    int32_t node_visits;         /* the root's node_visits                                           */
    int32_t status;              /* 0 = decided; TG_BEST_* bits otherwise                            */
} tg_best_move;
enum { TG_BEST_SAT_OUT = 1, TG_BEST_NO_ROOT = 2, TG_BEST_TREE_ERROR = 4 };
int tg_search_best_moves(tg_search *s, double resign_threshold, int play, const uint8_t *sit_out_host,
                         tg_best_move *records_host, void *stream);
/* GoBoard.count_score (go_board.py:561-608: stones in atari count as dead, an empty point takes the colour of its direct
 * neighbours) of `boards` padded boards cells_host [boards][(S+2)^2] as tg_search_read_positions returns them: black minus
 * white, komi not subtracted.  Host arithmetic, no device needed: what the self-play handle scores its finished games with. */
int tg_search_count_scores(const uint8_t *cells_host, int board_size, int boards, int32_t *scores_host);
/* Tree reuse (no reference counterpart - the reference rebuilds its tree every move, mcts/tree.py:49-54 - and off unless a
 * caller asks for it): for every tree with new_root_host[t] >= 0 the subtree under that node becomes the whole tree, in
 * place in the pool.  The new root is node 0; the other nodes keep their relative creation order (new index = rank among
 * the subtree's nodes); child indices and parent links are remapped; every statistic is kept bit for bit; num_nodes
 * becomes the subtree's size.  The root is not expanded or evaluated again.  A position staged for such a tree by
 * tg_search_set_root becomes its root position (without the reset tg_search_root_planes does); otherwise the tree keeps
 * its position.  The leaf queue is emptied and the root noise cleared.  new_root_host[t] = -1 leaves tree t (and its
 * staged position) alone.  Enqueued on `stream` (no host synchronisation); extra device memory: 4 bytes per pool node.
 * The next selection launch continues the search; feed its random window as for any mini-batch. */
int tg_search_reroot(tg_search *s, const int32_t *new_root_host, void *stream);
/* ---- tree reuse in lock-step PUCT matches (no reference counterpart, off unless a caller asks for it) ----
 * tg_search_advance: every tree's root advanced by one move, on the device, in one call - what MCTSTree(reuse_tree=True) does
 * per tree with one read-back per ply.  moves_host [T]: padded coordinates, 0 = PASS, -1 leaves the tree and its position
 * alone (anything else outside [0, (S+2)^2): TG_ERR_ARG, nothing launched).  For every other tree, one wavefront each:
 *   1. the root edge whose action is the move is looked up;
 *   2. the move is played on the tree's root position exactly as tg_search_play plays it (cells, hash, ko, prev / prevprev,
 *      the hash history, the side to move; a staged position is flushed first and played on);
 *   3. if that edge has an expanded child, the subtree under it becomes the tree exactly as tg_search_reroot makes it (the
 *      same kernels: new root = node 0, creation order kept, every statistic kept bit for bit, the leaf queue emptied, the
 *      root noise cleared); the root is not expanded or evaluated again;
 *   4. otherwise - the move is no root action, its edge is unexpanded (a one-child root that answered PASS without a search
 *      has only such edges), the tree has no root or its sticky error word is set - the tree becomes FRESH: num_nodes 0, its
 *      leaf queue emptied; the move is still played.
 * The halt word of every advanced tree is cleared and the live ranks go stale, as for tg_search_reroot.  A move onto a point
 * that is not empty is not played: the tree's sticky error word is set and nothing else of it changes; with records_host the
 * call then returns that error (TG_ERR_OVERFLOW), without it the next call that checks the error words does.
 * records_host [T] (may be NULL: the call is then only enqueued on `stream` and does not wait): one tg_advance_record per
 * tree.  After the call the chained searches refuse to run until a root launch (tg_search_root_planes_fresh). */
typedef struct tg_advance_record {
    int32_t kept_visits;         /* node_visits of the new root; -1: the tree is fresh, or was left alone        */
    int32_t kept_nodes;          /* nodes of the kept subtree (0 for a fresh tree)                               */
    int32_t num_children;        /* of the new root (0 for a fresh tree: tg_search_root_planes_fresh expands it) */
    int32_t status;              /* 0 = advanced; TG_ADVANCE_* bits otherwise                                    */
} tg_advance_record;
enum { TG_ADVANCE_LEFT_ALONE = 1, TG_ADVANCE_OCCUPIED = 2 };
int tg_search_advance(tg_search *s, const int32_t *moves_host, tg_advance_record *records_host, void *stream);
/* tg_search_root_planes for the FRESH trees only: a tree with num_nodes == 0 (fresh after tg_search_advance, a root set by
 * tg_search_set_root or from a record) is reset, expanded, featurised and its leaf queued exactly as tg_search_root_planes
 * does it - same draws, plane row t - and its halt word is cleared.  Of a tree with num_nodes > 0 nothing is written: no
 * node, no noise, no draw, no plane (row t keeps what it held), its halt word and draw cursor stay, and its leaf count is 0,
 * so the tg_search_backup(slots_per_tree = 1) behind the forward pass has nothing to do for it.  Counts as the root launch
 * the chained searches ask for. */
int tg_search_root_planes_fresh(tg_search *s, float *planes_dev, void *stream);
/* Per-tree visit budgets of the PUCT selection (csrc/visit_budget.h).  total_host [T] (each >= 1, else TG_ERR_ARG): from the
 * next PUCT selection launch on - tg_search_select_puct, its compact variant, every chain - tree t makes
 *   n = clamp(total_host[t] - its root's node_visits, 0, max_leaves)
 * descents instead of max_leaves, read once at kernel entry (a selection changes virtual losses, never visits): n leaves are
 * queued (tg_search_read_queue, n_leaves_dev), the root gets n virtual losses, a tree with n == 0 is passed by like a halted
 * one.  max_leaves stays the row stride of planes and outputs (leaf j of tree t at row t * max_leaves + j, or its rank's
 * rows in the compact layout), and the launch plan is max_leaves' (tg_search_launch_name).  The totals go up on `stream`
 * behind the launches that read the old ones.  total_host NULL: budgets off - every launch is what it was.
 * tg_search_budget_rule: halts every tree whose budget is spent (total - root visits <= 0), so that compaction
 * drops it - tg_search_stop_rule's conventions: trees halted, in error or without a root are left alone and are not live;
 * *live_host (may be NULL: no wait) = the trees left running.  TG_ERR_STATE without budgets in force.
 * tg_search_puct_chain_budget: tg_search_puct_chain with the budgets in force and the budget rule behind every backup; every
 * poll_every mini-batches the host looks whether a tree is still live and stops queueing when none is; compact 1: the
 * compact layout, re-ranked at every look exactly as tg_search_puct_chain_compact does with an early total (a tree halted
 * since the last look keeps an idle slot).  n_batches / leaves_host: what a FRESH tree needs.  *batches_run_host,
 * *positions_host (may be NULL): mini-batches queued, positions launched.  Needs a root launch since a root moved
 * (TG_ERR_STATE) and budgets in force (TG_ERR_STATE).  Budgets together with an early-stop total - tg_search_puct_chain_early,
 * tg_search_puct_chain_compact with total_host - are refused: TG_ERR_ARG. */
int tg_search_set_budget(tg_search *s, const int32_t *total_host, void *stream);
int tg_search_budget_rule(tg_search *s, int32_t *live_host, void *stream);
int tg_search_puct_chain_budget(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, int poll_every, int compact,
                                int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                                int32_t *batches_run_host, int64_t *positions_host);
/* Current root positions: cells uint8 [T][(S+2)^2], GoBoard.moves [T], side to move [T]
 * (any pointer may be NULL). Synchronises. */
int tg_search_read_positions(tg_search *s, uint8_t *cells_host, int32_t *moves_host,
                             int32_t *to_move_host);
/* What tg_search_read_positions does not give of ONE tree's current root on the device: *hash, meta8 = {moves, ko_pos,
 * ko_move, prev, prevprev, to_move, num_nodes, hist_len}, and the first min(hist_len, hist_cap) words of its hash history
 * in hist_host (the fields SearchEngine.set_root hands over, engine.py:197-209; any pointer may be NULL with hist_cap 0).
 * An observer: it reads nothing else and changes nothing.  Synchronises. */
int tg_search_read_root_state(tg_search *s, int tree, uint64_t *hash, int32_t *meta8, uint64_t *hist_host, int hist_cap);
/* Roots straight from game records: what mcts/analysis.py:188-207 (game_positions) and nn/data_generator.py:349-368
 * (_sampled_positions: a host replay and a deep copy per position) followed by one SearchEngine.set_root per position
 * (engine.py:197-209) put there, written by one kernel launch - one wavefront per record replays it once on the LDS board
 * (GoBoard.put_stone, go_board.py:131-185, under the handle's Zobrist keys) and writes the root of each of its trees as the
 * replay passes that tree's ply.  Board sizes 9, 13 and 19 (others: TG_ERR_ARG).
 *   moves_host: the records' moves, concatenated (padded coordinates, 0 = PASS); record g owns moves_host[offsets_host[g]
 *     .. offsets_host[g + 1]) (offsets_host [games + 1], starting at 0) and the same range of colors_host (1 black, 2
 *     white; NULL: colours alternate from black).
 *   root_game_host / root_ply_host [T]: tree t gets record root_game_host[t] (-1: the tree is left alone) at the position
 *     BEFORE its move root_ply_host[t] (0-based; ply == the record's length: the final position).  Several trees may
 *     share a position.
 *   The root: cells, hash, moves, ko_pos, ko_move, prev, prevprev of a GoBoard(check_superko of the handle) that has
 *     played the first `ply` moves with those colours; the hash history rec_hash[:min(moves, max_records)] with
 *     check_superko, one slot without; num_nodes 0; the tree's sticky error word cleared.  to_move: the colour of move
 *     `ply` where colours are given and ply < length, else alternating from black, and for the final position
 *     GoBoard.get_to_move() (the opponent of the last move's colour; black for an empty record).
 *   flags_host [T] out: 0 = the root was written (or the tree left alone), 1 = it was not and the tree's root - a
 *     position staged for it included - is what it was before the call.  A tree is flagged when the replay meets, before
 *     the tree's ply, a move that GoBoard.put_stone is not specified for (not a coordinate of the board, or a point that
 *     is not empty: tg_replay_run's rule; trees at plies up to and including that move's are written), when its record
 *     has more than max_records = 3 * S * S moves (tg_replay_run's rule), or when its own ply is >= max_records: from
 *     there the host board has stopped recording moves (go_board.py _save), so prev_move and get_to_move have nothing
 *     to read - a record of exactly max_records moves gives every position but its final one.  The caller sets flagged
 *     trees up from a host board (tg_search_set_root).
 *   Ordering: the records go up through pinned staging, the launch and the read-back of the flags are queued on `stream`,
 *     and the call waits for them.  The later call wins per tree: a position staged by tg_search_set_root for a tree
 *     written here is dropped, a tg_search_set_root after this call replaces the root at the next flush.  Like staged
 *     positions the roots take effect at the next tg_search_root_planes.  Together with tg_search_reroot on the same tree:
 *     not supported (the reroot takes its new position from the staged ones only).
 *   TG_ERR_ARG before anything is launched: null pointers, offsets that do not start at 0 or decrease, a game index >=
 *     games, a ply outside [0, length], a colour other than 1 or 2. */
int tg_search_set_roots_from_records(tg_search *s, const int32_t *moves_host, const int8_t *colors_host,
                                     const int64_t *offsets_host /* [games + 1] */, int games,
                                     const int32_t *root_game_host /* [T] */, const int32_t *root_ply_host /* [T] */,
                                     int32_t *flags_host /* [T] */, void *stream);
/* ---- library-owned random streams ---------------------------------------------------------
 * Alternative to tg_search_set_rng / tg_search_rng_consumed / tg_search_set_noise for hosts that
 * do not want to generate the draws themselves: the library continues numpy's legacy stream
 * (RandomState: MT19937, random_sample, standard_exponential = -log(1-u), gumbel = -log(-log(1-u)))
 * from a given generator state - what np.random.dirichlet(ones(n)) (mcts/tree.py:518) and
 * np.random.gumbel(size=A) (mcts/node.py:278) consume - one stream per tree.
 * seed_stream: mt_key = the 624 words, mt_pos = the index of np.random.get_state()[1:3].
 * stream_state: generator state after everything the tree has consumed so far (hand it back with
 *   np.random.set_state(('MT19937', key, pos, 0, 0.0))).
 * feed_streams: make `need` draws per tree available to the next root / select launch (no-op
 *   while the generated window still covers `need` for every tree, unless force != 0); the window is
 *   generated by a kernel on a stream of the library's own and overlaps running kernels.
 * advance_streams: after a root / select launch - wait for it, move every stream by what its tree
 *   consumed (optionally reported in consumed_host [T]).
 * draw_noise: set_gumbel_noise for every root from the next A draws of each stream (generated on the
 *   device, ordered like tg_search_set_noise's upload; copy returned in noise_host [T][A] unless NULL). */
int tg_search_seed_stream(tg_search *s, int tree, const uint32_t *mt_key, int mt_pos);
/* Every tree's stream at once: tree t starts from np.random.RandomState(seeds_host[t]).get_state() (seeds in [0, 2^32):
 * numpy seeds its legacy generator with MT19937's init_genrand, the recurrence tg_policy_seed_states starts from) - in
 * place of T RandomState objects and T tg_search_seed_stream calls per chunk (mcts/reanalyse.py searched_chunks through
 * engine.py:197-209); the states go up in one copy ahead of the next generation launch. */
int tg_search_seed_streams(tg_search *s, const uint32_t *seeds_host /* [T] */);
int tg_search_stream_state(tg_search *s, int tree, uint32_t *mt_key_out, int *mt_pos_out);
int tg_search_feed_streams(tg_search *s, size_t need, int force);
int tg_search_advance_streams(tg_search *s, int64_t *consumed_host);
int tg_search_draw_noise(tg_search *s, double *noise_host);
/* Since round 6 the streams live ON THE DEVICE (csrc/legacy_rng_device.h: MT19937, random_sample and glibc's table-driven
 * double-precision log - the build numpy's legacy distributions reach through libm on an FMA-capable x86-64 - restated
 * operation by operation): windows and noise are generated there, the host only counts what was consumed.
 * Host-only helpers (no device needed) that run the SAME restated arithmetic on the host, for the CPU tests:
 *   tg_legacy_exponentials: the next n legacy standard_exponential draws of the generator (mt_key, *mt_pos), updated in place;
 *   tg_glibc_log: out[i] = log(x[i]) (positive normal arguments) - held against Python's math.log (= libm) bit for bit. */
int tg_legacy_exponentials(uint32_t *mt_key, int *mt_pos, size_t n, double *out);
int tg_glibc_log(const double *x, size_t n, double *out);
/* A HIP stream owned by the handle (created on first request, destroyed with it; hipStreamNonBlocking) for callers that run
 * several handles side by side - the lanes of a self-play shard (selfplay/worker.py) - and want each on a stream of its own
 * without going through a host framework's stream pool. */
int tg_search_own_stream(tg_search *s, void **stream_out);
/* Test hooks of the device streams (tests/test_gpu_rng.py): read columns [first, first + count) of tree `tree`'s row of the
 * most recently generated window; walk the streams as a search would - per step a window of steps[i] + slack draws, whole
 * (part 0) or in pieces of `part` draws, steps[i] of which count as consumed - without running a search. */
int tg_search_debug_read_window(tg_search *s, int tree, size_t first, size_t count, double *out_host);
int tg_search_debug_stream_walk(tg_search *s, const int64_t *steps, int n_steps, int64_t slack, int64_t part);
/* Gumbel root noise, float64 [T][A] (node.py:275-278 set_gumbel_noise), to be set after the
 * root evaluation of a Gumbel move. */
int tg_search_set_noise(tg_search *s, const double *noise_host);
/* One sequential-halving phase (tree.py:375-383): per tree, for count_threshold in
 * 1..max_count[t], num_considered[t] descents (root: node.py:324-346, below: :349-361);
 * every descent queues one leaf.  Planes [T, slots_per_tree, 6, S, S]; trees whose phase
 * is (0, 0) idle.  slots_per_tree = 0 selects the PACKED layout: the leaves of tree t start at
 * plane sum_{u<t} num_considered[u] * max_count[u], so the forward pass covers exactly the
 * queued leaves (one tree with a single root candidate runs 1 x visits levels and would
 * otherwise stretch every tree's slot range).  Follow with the forward pass and
 * tg_search_backup(same slots_per_tree, use_logit = 1).
 * slots_per_tree = -1 selects the UNIQUE layout (no reference counterpart: tree.py:412-416 queues, and tree.py:273-315
 * evaluates, one leaf per descent): nothing moves within a phase, so all descents through one root child end on the same
 * leaf, and only the DISTINCT leaves of a tree get planes - in the order of their first descents, at the start of the
 * tree's plane range.  Tree t owns cap[t] = min(num_considered[t] * max_count[t], 17) plane slots (17: the most root
 * children a phase enters, node.py:324-346) starting at sum_{u<t} cap[u]; slots behind its last distinct leaf hold a copy
 * of its first one.  Queue entries, paths and virtual losses are those of every other layout; each queued leaf remembers
 * which plane holds its position.  A launch that runs on the one-wavefront kernel (a tree with more than 512 descents, a
 * pool beyond 2^21 nodes, TG_SELECT_SERIAL) saves nothing: cap[t] = num_considered[t] * max_count[t].  Follow with
 * tg_search_unique_planes, the forward pass over that many planes and tg_search_backup(-1, use_logit = 1): same trees. */
int tg_search_select_gumbel(tg_search *s, const int32_t *num_considered_host,
                            const int32_t *max_count_host, int slots_per_tree,
                            float *planes_dev, void *stream);
/* Write NN outputs back and back up values (tree.py:273-315 process_mini_batch).
 * policy_dev [T, slots_per_tree, A], value_dev [T, slots_per_tree, 3] in the slot order
 * of the preceding call (slots_per_tree = its max_leaves, 1 after root_planes, 0 after a packed
 * tg_search_select_gumbel: policy_dev [total, A], value_dev [total, 3]; -1 after a unique one: policy_dev
 * [planes, A], value_dev [planes, 3] - every leaf reads the outputs of the plane that holds its position, in the
 * reference's leaf order; without a preceding unique selection: TG_ERR_ARG);
 * use_logit as in tree.py:293-294. */
int tg_search_backup(tg_search *s, const float *policy_dev, const float *value_dev,
                     int slots_per_tree, int use_logit, void *stream);
/* After a UNIQUE tg_search_select_gumbel (slots_per_tree -1): *total_host = planes the forward pass must cover,
 * cap_host [T] (may be NULL) = each tree's plane range, tree t's starting at sum_{u<t} cap_host[u] (the mini-batch of
 * tree.py:273-315 with each distinct leaf of tree.py:412-416 once).  Host arithmetic on the phase description: no
 * synchronisation.  TG_ERR_STATE when the last selection was not a unique one. */
int tg_search_unique_planes(tg_search *s, int64_t *total_host, int32_t *cap_host /* [T], may be NULL */);

/* Path of queued leaf `slot` of tree `tree` after a selection launch, root first:
 * (node index, child index) per level - the `path` list of search_mcts (tree.py:199-244) that
 * search_with_callback (tree.py:177-196) hands to its callback.  Valid for the slots the last
 * selection launch queued, until the next one.  Synchronises. */
int tg_search_read_path(tg_search *s, int tree, int slot, int32_t *nodes_host, int32_t *edges_host,
                        int capacity, int32_t *length_host);
/* Leaf queue of tree `tree` as the last selection launch left it (mcts/batch_data.py:7-34, the
 * `node_index` list of BatchQueue): count_host = leaves queued, node_index_host[i] = node that
 * receives leaf i's policy (-1 = the reference's node[-1] slot, tree.py:222-233 when the leaf was
 * already expanded).  The matching `input_plane` entries are the planes the selection wrote, the
 * `path` entries come from tg_search_read_path.  Valid until the next selection launch.  Synchronises. */
int tg_search_read_queue(tg_search *s, int tree, int32_t *node_index_host, int capacity,
                         int32_t *count_host);
/* Grow the node pool of every tree to new_tree_size nodes, keeping the trees (the reference doubles
 * its node list in place when it fills up, mcts/tree.py:254-258).  No-op if the pool is already that
 * large.  Synchronises the device. */
int tg_search_grow(tg_search *s, int new_tree_size);
/* Read-side of MCTSNode for node `node` of tree `t` (node.py:21-39); any pointer may be
 * NULL.  Arrays have A entries. Synchronises the stream used by the last call. */
int tg_search_read_node(tg_search *s, int tree, int node, int32_t *num_children,
                        int32_t *node_visits, int32_t *node_virtual_loss, int32_t *action,
                        int32_t *children_index,
                        int32_t *children_visits, int32_t *children_virtual_loss,
                        double *children_value_sum, double *children_policy,
                        double *children_value, float *node_value_sum, float *raw_value);
/* Parent node and the parent's child slot of node `node` of tree `tree` (-1, -1 for the root).  Synchronises. */
int tg_search_read_node_links(tg_search *s, int tree, int node, int32_t *parent, int32_t *pedge);
/* Analysis read-out of every tree in one launch + one copy (no reference counterpart: the reference walks its principal
 * variations node by node on the host, mcts/tree.py:432-473 get_pv_lists / get_best_move_sequence, for the analysis
 * strings of mcts/node.py:399-482).  root_host [T][4]: num_children, node_visits, node_value_sum (float32 bits), the
 * tree's sticky error flags (as tg_search_read_node reports them; the numbers of a tree with flags set are not
 * meaningful).  action / children_visits / pv_len / resume [T][A] int32, children_value_sum / children_policy [T][A]
 * float64, pv [T][A][max_depth] int16 (padded coordinates).  For every root child i < num_children with visits > 0:
 * pv[t][i][:pv_len] = get_best_move_sequence([action[i]], children_index[i]) (children_index -1 looked up as node
 * tree_size - 1, like the host's node[-1]), cut after max_depth moves; resume = the node at which the host continues the
 * walk with tg_search_read_node when it was cut, -1 when the PV is complete.  Other children: pv_len 0, resume -1.
 * 1 <= max_depth <= 1024.  Enqueued on `stream`, then synchronises. */
int tg_search_read_analysis(tg_search *s, int max_depth, int32_t *root_host, int32_t *action_host,
                            int32_t *visits_host, double *value_sum_host, double *policy_host,
                            int16_t *pv_host, int32_t *pv_len_host, int32_t *resume_host, void *stream);
/* Improved policy of every root in one launch (replaces mcts/node.py:281-321 calculate_completed_q_value(use_mixed_value=True)
 * + calculate_improved_policy on a root read back to the host, and the "%.3e" text round trip of sgf/selfplay_record.py:56 ->
 * nn/feature.py:80-102).  rows_dev [T][S*S+1] float32, DEVICE memory, network output order (board points row-major, PASS
 * last): the improved policy of root child i, computed in float64 in the reference's order of operations and rounded once,
 * at the slot of action[i]; (float)1e-18 at every slot without a child (feature.py's value for a move that was no
 * candidate).  Every root must be expanded (tg_search_root_planes + tg_search_backup, searched or not): a tree whose root is
 * not - a position staged by tg_search_set_root, a handle that never ran - is TG_ERR_ARG, and the rows are not to be used.
 * Enqueued on `stream`, then synchronises. */
int tg_search_read_improved_policy(tg_search *s, float *rows_dev /* [T][S*S+1] */, void *stream);
/* num_nodes of the tree that tg_search_read_node read last, as of that read (same record, no device access). */
int tg_search_node_record_num_nodes(tg_search *s, int32_t *num_nodes_host);
int tg_search_num_nodes(tg_search *s, int32_t *num_nodes_host /* [T] */);
/* ---- whole-tree read-out: all nodes of any set of trees in a fixed number of launches and one copy ----
 * `trees` lists n tree indices: any subset in any order; NULL: all trees of the handle in order (n is not read).  An empty
 * list, an index out of range and a duplicate are TG_ERR_ARG before anything is launched.  The trees are read as the device
 * holds them (like tg_search_read_node): a tree that never had a root has num_nodes 0, an empty record and the digest of the
 * empty tree; a tree whose sticky error word is set is read all the same - the word travels in its record's head, the caller
 * decides.  All three enqueue on `stream`, then synchronise; none changes a tree.
 *
 * Record of one tree (8-byte aligned; csrc/tree_dump.h states the layout once): a head of 8 int32 - num_nodes, current_root
 * (0: a reroot compacts the kept subtree to the front), the error word, the side to move (1 black, 2 white), the total number
 * of children (64 bits, low word first), 0, 0 -, then num_nodes node records of 40 bytes - node_visits, virtual_loss,
 * node_value_sum and raw_value (float32 bits), num_children, parent, the parent's child slot, 0 (int32 each) and first_child
 * (int64): where the node's entries start in every row -, then one row of `total` entries per child array: children_index,
 * children_visits, children_virtual_loss, action (int32), then, 8-byte aligned, children_value_sum, children_policy,
 * children_value (float64).  A row holds the first num_children entries of node 0, then of node 1, ...: what lies at or
 * beyond num_children in the pool is stale by design and is not read.
 *
 * What a dump of these trees needs (replaces the sizing loop of mcts/tree.py:496 over mcts/node.py:221-243): num_nodes_host
 * [n], children_host [n] (int64).  A record takes 32 + 40 num_nodes + 16 children bytes, rounded up to 8, + 24 children. */
int tg_search_dump_sizes(tg_search *s, const int32_t *trees, int n, int64_t *num_nodes_host, int64_t *children_host,
                         void *stream);
/* The packed records (replaces MCTSTree.to_dict, mcts/tree.py:489-506, and MCTSNode.to_dict, mcts/node.py:221-253, per node):
 * record j at records_host + offsets_host[j], offsets_host [n + 1] (the last: the bytes written).  A capacity that is too
 * small is TG_ERR_ARG, the size needed is in tg_last_error, and nothing is written to records_host. */
int tg_search_dump_trees(tg_search *s, const int32_t *trees, int n, unsigned char *records_host, size_t capacity,
                         int64_t *offsets_host, void *stream);
/* Digest of every listed tree without packing anything (no reference counterpart: the reference compares dumps,
 * mcts/dump.py:10-33, node by node): digests_host [n][2] uint64, two words of one rule under two seeds over num_nodes,
 * current_root, every node's five scalars and every child array's entries below num_children, each with its node and child
 * index and by its bit pattern (csrc/tree_dump.h; tamago_amd/mcts/dump.py digest_of restates it for a dumped tree). */
int tg_search_tree_digests(tg_search *s, const int32_t *trees, int n, uint64_t *digests_host /* [n][2] */, void *stream);
/* ---- whole-tree write-in: packed records back into the pool (inverts MCTSTree.to_dict, mcts/tree.py:476-506, and the dump
 * of mcts/dump.py:10-33; the reference has no reader of its own dumps) ----
 * Record j at records_host + offsets_host[j], offsets_host [n + 1], in the layout above.  A record is admissible when
 * (csrc/tree_load.h states the rules once, in this order): its length is exactly its head's, nodes' and rows'; the head's pad
 * words are 0, 0 <= num_nodes <= tree_size, current_root 0, the error word 0, to_move 1 or 2 (an empty record: any); every
 * node has 1 <= num_children <= S*S+1, first_child the exclusive scan of num_children, pad 0, visits and virtual loss >= 0;
 * total is the sum of num_children; every children_index entry is -1 or lies in (its node, num_nodes), every node but node 0
 * is named by exactly one edge and carries that edge as parent / slot, node 0 carries -1 / -1; every action is the pass (0) or
 * the padded coordinate of an on-board point; children_visits and children_virtual_loss are >= 0.  Floats may hold any bits.
 *
 * The check alone: no handle, no GPU.  TG_ERR_ARG names the rule (its number in csrc/tree_load.h and its text), the list
 * entry, the node and the child in tg_last_error. */
int tg_search_check_records(int board_size, int tree_size, const unsigned char *records_host,
                            const int64_t *offsets_host /* [n + 1] */, int n);
/* Record j becomes tree trees[j] (the list conventions of the read-out: any subset in any order, NULL: all trees; an empty
 * list, an index out of range and a duplicate are TG_ERR_ARG).  Every record is checked on the host first: one inadmissible
 * record refuses the whole call before anything is uploaded or launched.  Then a position staged by tg_search_set_root for a
 * listed tree is uploaded (other trees' stay staged), the records go up in one copy, and one launch writes every node: its
 * scalars, the first num_children entries of every child array, and beyond them what a fresh expansion leaves (children_index
 * -1, everything else 0), so a loaded node cannot be told from an expanded one.  A loaded tree gets its num_nodes, an empty
 * leaf queue, a zero noise row (on the device and in the host's mirror: tg_search_set_noise puts one back) and clear error and
 * halt words.  flags_host [n]: 1 where the record's side to move is not that of the tree's root position - that tree is left
 * exactly as it was, the others load.  Enqueued on `stream`, then synchronises.
 *
 * Not touched: the root position (tg_search_set_root), the streams and cursors (tg_search_seed_stream), budgets and rank
 * tables in force, other trees, any evaluation cache.  A virtual loss in a record is stored as it is.  Nothing checks that a
 * tree belongs to its root position - that its actions are legal there and its statistics those of that position: what the
 * kernels do with a tree that does not is not specified, as for a history given to tg_search_set_root that is not the
 * position's. */
int tg_search_load_trees(tg_search *s, const int32_t *trees, int n, const unsigned char *records_host,
                         const int64_t *offsets_host /* [n + 1] */, int32_t *flags_host /* [n] */, void *stream);
/* Root statistics of all trees in one call: num_children [T], action [T][A],
 * children_visits [T][A] (what get_best_move reads, node.py:169-184). Synchronises. */
int tg_search_read_roots(tg_search *s, int32_t *num_children_host, int32_t *action_host,
                         int32_t *visits_host);

/* ---- self-play shard bookkeeping (selfplay/worker.py:50-90, sgf/selfplay_record.py:45-110) -----------
 * Everything the reference's worker does per move and per board AROUND the search, for all T boards of a
 * search handle in one host call per move (C++, host threads): sequential-halving schedule
 * (mcts/sequential_halving.py), final root choice (tree.py:344, node.py:324-346), resign rule
 * (tree.py:351-354), improved-policy comment with ".3e" values (node.py:281-321, selfplay_record.py:45-65),
 * two-pass end with count_score (go_board.py:561-608), maximum length (worker.py:44), the SGF file
 * <save_dir>/<index>.sgf byte for byte as selfplay_record.py:67-110 writes it.
 * Per move the caller does: tg_search_root_planes / forward / tg_search_backup, tg_search_draw_noise,
 * tg_selfplay_schedule, one tg_search_select_gumbel / forward / tg_search_backup per phase,
 * tg_selfplay_finish_move, tg_search_play(moves); slots whose game finished get tg_search_set_root +
 * tg_search_seed_stream + tg_selfplay_start_game (or index -1 to park them). */
typedef struct tg_selfplay tg_selfplay;
/* komi_text: the komi as the SGF shall spell it (the reference prints Python's repr, e.g. "7.0").  save_dir "" (empty):
 * no record files are written; the results stay readable through tg_selfplay_game_result. */
int tg_selfplay_create(tg_search *s, const char *save_dir, int visits, double komi, const char *komi_text,
                       tg_selfplay **out);
int tg_selfplay_destroy(tg_selfplay *sp);
int tg_selfplay_start_game(tg_selfplay *sp, int slot, int index, int never_resign);
/* Phases of the coming move for every board: num_considered / max_count host arrays [max_phases][T] (zero
 * where a board has no such phase or is parked), *n_phases_host = phases of the longest schedule. */
int tg_selfplay_schedule(tg_selfplay *sp, int32_t *num_considered_host, int32_t *max_count_host,
                         int max_phases, int32_t *n_phases_host);
/* After the last phase: moves_host[T] = move to play on each board (-1 = none: parked, resigned or game
 * over), finished_host[T] = 1 where the game ended (its file is written), stats_host[2] = {games finished,
 * moves decided} by this call (may be NULL). */
int tg_selfplay_finish_move(tg_selfplay *sp, int32_t *moves_host, int32_t *finished_host,
                            int64_t *stats_host);
/* The whole move above in ONE call when the evaluator is a tg_net (root evaluation, noise, schedule, every
 * phase with its forward pass, tg_selfplay_finish_move, tg_search_play): nothing but library code runs
 * between the launches.  Caller's device buffers: planes [T*batch_size,6,S,S], policy [T*batch_size,A],
 * value [T*batch_size,3].  finished_host[T] as above; stats_host[3] = {games finished, moves decided, leaf
 * evaluations} of this move (may be NULL).
 * Default scheme ("chained"): the device decides the move itself (final choice, resign rule, game end - the host's
 * arithmetic, which the host repeats on the same statistics and compares), plays it and expands + evaluates the
 * next root without the host; the call returns once the root RECORDS have arrived, with that root evaluation still
 * running, and the next call starts from it.  Consequences a caller sees: the first call of a handle only evaluates
 * roots (no move, nothing finished); a slot whose game was just started (tg_selfplay_start_game) sits out one call;
 * below 385 boards the phases run in 2 - 4 sub-groups of boards on streams of the library's own (joined into
 * `stream` before the call returns control of the buffers).  Games, records and draw order per game are the same in
 * every scheme.  TG_SP_CHAIN=0: the move decided on the host (three round trips per move); TG_SP_SUBGROUPS=n /
 * TG_SP_FWD_CAP=n override the grouping.  With an observer the boards stay in one group. */
int tg_selfplay_play_move(tg_selfplay *sp, tg_net *net, float *planes_dev, float *policy_dev,
                          float *value_dev, void *stream, int32_t *finished_host, int64_t *stats_host);
/* The two halves of a chained tg_selfplay_play_move, for a caller that keeps several handles (lanes of one shard: each its own
 * tg_search, buffers and stream) in flight from one host thread - selfplay/worker.py:46-90 plays its games one after the other;
 * games are independent, so lanes need not be on the same move.  `begin` queues the whole move (phases, decision, the moves
 * played, next root evaluation) on `stream` and returns; `end` waits for that move's root records, does the bookkeeping
 * (records, finished games, SGF) and fills finished_host[T] / stats_host[3] as tg_selfplay_play_move does.  Between a handle's
 * `begin` and `end` only other handles may be driven; slots are refilled (tg_selfplay_start_game) after `end`.  The buffers
 * belong to the library until `end` returns.  Not with an observer or TG_SP_CHAIN=0 (TG_ERR_STATE). */
int tg_selfplay_move_begin(tg_selfplay *sp, tg_net *net, float *planes_dev, float *policy_dev, float *value_dev, void *stream);
int tg_selfplay_move_end(tg_selfplay *sp, int32_t *finished_host, int64_t *stats_host);
/* The one-call move and the first half of a chained move with one evaluator per colour (a match: black's moves searched
 * by one network, white's by another).  net_to_move runs the call's phases (round-trip scheme: and the root evaluation
 * they start from); net_next runs the chained scheme's closing evaluation of the roots the NEXT call searches from.
 * net_to_move == net_next is tg_selfplay_play_move / tg_selfplay_move_begin: same launches, no further rule.  With two
 * different handles a call moves ONE colour, checked before anything is launched (TG_ERR_STATE, the message names the
 * slot):
 *   - every board that searches in the call has the same side to move;
 *   - chained scheme: every board whose root the call evaluates for the next call has the other side to move - the
 *     boards that moved do; a slot just started (tg_selfplay_start_game: black to move) may therefore sit out only a
 *     call in which white moves (or in which nothing moves: a handle's first call), where net_next is black's network;
 *   - round-trip scheme: a started slot searches at once, so it is started only when the next call is black's.
 *   - the two networks take turns: a call's net_to_move is the net_next of the call before (also where no board searches).
 * Which of the two is black's is the caller's word in a handle's first call - the library has no notion of whose network
 * is whose -, so what is enforced is consistency from there on, not the naming itself.  The caller alternates the two
 * handles call by call and starts games accordingly (tamago_amd/selfplay/match.py: slot_may_start, which needs the
 * handle's scheme: tg_selfplay_chained).  tg_selfplay_move_end is unchanged. */
int tg_selfplay_play_move2(tg_selfplay *sp, tg_net *net_to_move, tg_net *net_next, float *planes_dev, float *policy_dev,
                           float *value_dev, void *stream, int32_t *finished_host, int64_t *stats_host);
int tg_selfplay_move_begin2(tg_selfplay *sp, tg_net *net_to_move, tg_net *net_next, float *planes_dev, float *policy_dev,
                            float *value_dev, void *stream);
/* The names the records carry in PB[] / PW[]; NULL keeps a side's default ("TamaGo-Black" / "TamaGo-White", the
 * reference's).  No ']', backslash or line break (TG_ERR_ARG). */
int tg_selfplay_set_players(tg_selfplay *sp, const char *black, const char *white);
/* *chained_host = 1 if the handle's one-call moves run the chained scheme, 0 for the round-trip scheme.  A handle that has
 * not moved yet is told what its first tg_selfplay_play_move(2) would decide (chained, unless TG_DEBUG_KNOBS=1 and
 * TG_SP_CHAIN=0) and keeps to the answer.  sp == NULL: what a new handle would be told; needs no device. */
int tg_selfplay_chained(tg_selfplay *sp, int *chained_host);
/* The result of the game that ended in `slot`, without reading its file back: result_host[4] = {game index, winner (1 black,
 * 2 white, 3 draw, 0 none: the move limit was reached), 1 if it ended by resignation, moves played}, *score_host = count_score
 * - komi (0 unless the game ended with two passes).  Valid from the call that reports finished[slot] until the slot is
 * restarted (TG_ERR_STATE otherwise).  An empty save_dir (tg_selfplay_create) keeps the results and writes no files. */
int tg_selfplay_game_result(tg_selfplay *sp, int slot, int32_t *result_host, double *score_host);
/* on != 0: tg_selfplay_play_move and tg_selfplay_move_begin / _end run every phase in the UNIQUE leaf layout
 * (tg_search_select_gumbel with slots_per_tree -1) in every scheme - chained, TG_SP_CHAIN=0, sub-groups, with an observer -
 * and size each forward launch by the plane ranges: the leaves tree.py:375-384 queues once per descent are evaluated once
 * per distinct position.  Same trees, games and SGF bytes as long as the network takes no f16 range fallback (a hot
 * position's exact redo covers the positions launched with it, and those differ between layouts - the caveat the
 * sub-group schemes carry).  stats_host[2] keeps counting QUEUED leaves.  Off by default; between moves only. */
int tg_selfplay_set_unique_leaves(tg_selfplay *sp, int on);
/* Positions this handle's moves have handed to the network so far (root evaluations and phases; the reference evaluates
 * every queued leaf, tree.py:273-315): the sum of stats_host[2] unless the UNIQUE layout is on. */
int tg_selfplay_forward_positions(tg_selfplay *sp, int64_t *count_host);
/* Audit hook of tg_selfplay_play_move (parity tests replay what the one-call path evaluated into the CPU oracle,
 * mini-batch by mini-batch: mcts/tree.py:273-315 process_mini_batch is where the reference would be tapped).
 * The observer is called on the calling thread
 *   kind 0: after a mini-batch's forward pass and backup were ENQUEUED on `stream` and before the next selection
 *           overwrites the buffers - synchronise `stream`, then planes_dev [positions,6,S,S], policy_dev
 *           [positions,A], value_dev [positions,3] hold that mini-batch.  phase = -1: root evaluation, one leaf
 *           per board in board order; phase >= 0: sequential-halving phase, PACKED layout - the leaves of board t
 *           start at sum_{u<t} num_considered[u] * max_count[u] (host arrays [trees]); with
 *           tg_selfplay_set_unique_leaves on: UNIQUE layout, positions = planes forwarded - board t's distinct
 *           leaves start at sum_{u<t} cap[u], cap[u] = min(num_considered[u] * max_count[u], 17) (the product itself
 *           when a board makes more than 512 descents or TG_SELECT_SERIAL is set), and one leaf's outputs serve all
 *           descents through its root child;
 *   kind 1: after the moves of all boards were decided (tg_selfplay_finish_move) and before they are played: root
 *           statistics of every board as host arrays num_children [trees], action / children_visits [trees][A],
 *           children_value_sum [trees][A], moves [trees] (-1 = none), finished [trees].
 * Pointers are valid until the observer returns.  fn = NULL removes the observer.  Results do not depend on it. */
typedef struct tg_selfplay_event {
    int32_t kind, phase, trees, positions;
    const int32_t *num_considered, *max_count;                 /* kind 0, phase >= 0 */
    const float *planes_dev, *policy_dev, *value_dev;          /* kind 0 */
    void *stream;
    const int32_t *num_children, *action, *children_visits;    /* kind 1 */
    const double *children_value_sum;
    const int32_t *moves, *finished;
} tg_selfplay_event;
typedef void (*tg_selfplay_observer)(void *user, const tg_selfplay_event *event);
int tg_selfplay_set_observer(tg_selfplay *sp, tg_selfplay_observer fn, void *user);

/* ---- policy-only play (nn/policy_player.py:13-46, gtp/client.py:206-211) --------------------------------------
 * One move per board from ONE forward pass, for all T boards of a search handle at once: the legal points
 * (GoBoard.is_legal, go_board.py:260-304: no eye or self-atari filter) and PASS are the candidates
 * (policy_player.py:32-36), those whose policy exceeds a tenth of the best are kept (:38-41, compared in float64 as
 * Python does), and one is drawn with random.choices (:46) - CPython's arithmetic operation by operation: sequential
 * float64 running sum, one random() of the board's MT19937 stream, bisect_right.  The handle borrows the boards (root
 * positions) of the tg_search it was created on and owns the streams; destroy it before the tg_search. */
typedef struct tg_policy tg_policy;
int tg_policy_create(tg_search *s, tg_policy **out);
int tg_policy_destroy(tg_policy *p);
/* Board `board` draws from this generator state from now on: mt_key = the 624 words, mt_pos = the position, i.e.
 * random.getstate()[1][:624] and [624] (the layout of tg_search_seed_stream; policy_player.py:46 draws from the
 * global `random` module).  tg_policy_state: the state after the draws made so far (random.setstate); synchronises. */
int tg_policy_seed(tg_policy *p, int board, const uint32_t *mt_key, int mt_pos);
int tg_policy_state(tg_policy *p, int board, uint32_t *mt_key_out, int *mt_pos_out);
/* Board `board` is a GoBoard(check_superko=False) (check_superko = 0) although the search handle checks positional
 * superko (go_board.py:285-301): its moves are not tested against the history.  For batches of positions that come from
 * boards of both kinds; turning the check ON needs a handle created with check_superko.  Synchronises. */
int tg_policy_set_superko(tg_policy *p, int board, int check_superko);
/* Planes [T,6,S,S] of the current root position of every board for its side to move, symmetry 0
 * (generate_input_planes(board, color), policy_player.py:25).  Unlike tg_search_root_planes: no tree is reset, no
 * root expanded, no draw consumed.  Enqueued on `stream`. */
int tg_policy_planes(tg_policy *p, float *planes_dev, void *stream);
/* The move of every board (policy_player.py:29-46) from policy_dev [T,A] (softmax, tg_net_forward_dev with
 * want_logits 0); one random() per board.  answer_pass != 0: PASS when the board's previous move was a pass
 * (gtp/client.py:209-211; the draw is consumed all the same).  play != 0: the move is then played on the board
 * (GoBoard.put_stone, go_board.py:131-185, as tg_search_play does) and the side to move flips.  moves_dev [T]
 * (device, may be NULL) receives the moves in stream order; moves_host [T] (may be NULL) makes the call wait for them. */
int tg_policy_moves(tg_policy *p, const float *policy_dev, int play, int answer_pass, int32_t *moves_dev,
                    int32_t *moves_host, void *stream);
/* Whole games from the empty board, policy against policy (the loop of selfplay/worker.py:44-87 with
 * generate_move_from_policy for the move and the rule of gtp/client.py:209-211 when answer_pass != 0): `games` games
 * on the T boards, slot t playing games t, t + T, ...; game g draws from mt_states_host[g] ([games][625]: 624 words +
 * position, uploaded once).  A game ends after two passes or max_moves moves (worker.py:44,56,76).  A slot takes its
 * next game at an even ply only, so all live boards have the same side to move: ply 0, 2, ... is black's.
 *   tg_policy_games_ply: one ply of every live board with `net` (black's network at even plies, white's at odd ones):
 *     forward pass and move kernel ENQUEUED on `stream`; planes_dev [T,6,S,S], policy_dev [T,A], value_dev [T,3] are
 *     the caller's and must be the same buffers for every ply of a run (the move kernel leaves the next ply's planes
 *     there).  policy_keep_dev (may be NULL): [T,A] copy of this ply's policy, in stream order.  Plies enqueued after the
 *     last game ended do nothing.
 *   tg_policy_games_finished: games over so far, read from host-mapped memory WITHOUT waiting for the stream (a lower
 *     bound while plies are in flight).
 *   tg_policy_games_results: waits for the stream; moves_host [games][max_moves] (padded coordinates, 0 = PASS),
 *     lengths_host [games], reasons_host [games] (1 two passes, 2 max_moves, 0 not finished), scores_host [games] =
 *     GoBoard.count_score() of the final board (go_board.py:561-608; the caller subtracts the komi, worker.py:81),
 *     cells_host [games][(S+2)^2] the final boards; *plies_host = plies enqueued; any pointer may be NULL. */
int tg_policy_games_begin(tg_policy *p, int games, int max_moves, int answer_pass, const uint32_t *mt_states_host);
/* Host-only helper (no device needed): states_out[g] ([n][625]) = random.Random(seeds[g]).getstate()[1], for seeds in
 * [0, 2^32) - CPython's random.seed(int) is MT19937's init_by_array on the seed's 32-bit words - so that thousands of
 * per-game streams need no Python object each. */
int tg_policy_seed_states(const uint32_t *seeds, size_t n, uint32_t *states_out);
int tg_policy_games_ply(tg_policy *p, tg_net *net, float *planes_dev, float *policy_dev, float *value_dev,
                        float *policy_keep_dev, void *stream);
int tg_policy_games_finished(tg_policy *p, int32_t *finished_host);
int tg_policy_games_results(tg_policy *p, int32_t *moves_host, int32_t *lengths_host, int32_t *reasons_host,
                            int32_t *scores_host, uint8_t *cells_host, int64_t *plies_host);

/* ---- training samples from game records (nn/data_generator.py:37-149) ----------------------------------------
 * The replay half of the data generators on the device: one wavefront per game record replays it from the empty
 * board (GoBoard.put_stone, go_board.py:131-185, colours alternating from black as data_generator.py:55-63 and
 * :122-134 do whatever the SGF tags say) and, before the move of every sampled ply, writes the input planes of the
 * side to move under the sample's board symmetry (generate_input_planes, nn/feature.py:10-57: the bytes of
 * tg_featurize_sym_dev on that position).  Which plies and symmetries are sampled is the caller's choice, so the
 * random-number call order of data_generator.py:108-110 stays on the host.  The handle owns its staging and device
 * buffers; board sizes 9, 13 and 19 (others: TG_ERR_ARG).
 *   tg_replay_run: moves_host = the games' moves, concatenated (padded coordinates, 0 = PASS); game g owns
 *     moves_host[offsets_host[g] .. offsets_host[g + 1]) and the samples sample_offsets_host[g] ..
 *     sample_offsets_host[g + 1) of sample_ply_host / sample_sym_host (0-based ply < the game's moves, non-decreasing
 *     within a game; symmetry 0..7; both offset arrays [games + 1], starting at 0).  Sample i's planes go to
 *     planes_dev[i] ([samples,6,S,S] fp32, device memory).  flags_host[g] (host, [games]) = 0, or 1 when the game has a
 *     move that is no coordinate of the board or lands on a point that is not empty: the replay of that game stops
 *     there, its remaining rows are not written, and the caller redoes the game on the host board.  Uploads once,
 *     launches once on `stream` and waits for it. */
typedef struct tg_replay tg_replay;
int tg_replay_create(int board_size, int device, tg_replay **out);
int tg_replay_destroy(tg_replay *r);
int tg_replay_run(tg_replay *r, const int32_t *moves_host, const int64_t *offsets_host, int games,
                  const int32_t *sample_ply_host, const int8_t *sample_sym_host,
                  const int64_t *sample_offsets_host /* [games+1] */,
                  float *planes_dev /* [samples,6,S,S] */, int32_t *flags_host /* [games] */, void *stream);

/* ---- training step (nn/learn.py:318-403, nn/loss.py:9-55; modules of nn/network/) ---------------------------
 * One mini-batch of the reference's GPU trainers as hand-written HIP kernels (forward with batch statistics,
 * backward, torch.optim.SGD(momentum 0.9, weight_decay 1e-4, nesterov=True) update, batch-norm running
 * statistics), fp32.  The trainer owns a device copy of the parameters in the tg_net_create blob order
 * (running_mean / running_var included; num_batches_tracked is the caller's counter) and a momentum blob of
 * the same layout.  board_size 9 or 19 (other sizes: TG_ERR_ARG); batch = positions per step (>= 2).
 *   tg_trainer_step: planes [B,6,9,9] fp32, policy targets [B,82] fp32, value classes [B] int64, all device
 *     memory; sl_mode 0 = RL objective (KL(target || softmax) batch mean + value_weight * cross entropy,
 *     learn.py:360-376), 1 = supervised (-sum t log(softmax + 1e-8), learn.py:150-180); ENQUEUES the step.
 *   tg_trainer_read_losses: device-accumulated sums of (total, policy, value) loss over the steps since the
 *     last reset, one read for many steps. */
typedef struct tg_trainer tg_trainer;
int tg_trainer_create(int board_size, int device, int batch, const float *params_host, size_t n_params,
                      tg_trainer **out);
int tg_trainer_destroy(tg_trainer *t);
int tg_trainer_step(tg_trainer *t, const float *planes_dev, const float *policy_dev,
                    const long long *value_dev, int sl_mode, float value_weight, float lr, void *stream);
int tg_trainer_read_losses(tg_trainer *t, double *sums_host /* [3] */, int reset);
/* parameters (and, unless NULL, the momentum buffers) back to the host; n = tg_net_param_count(board_size) */
int tg_trainer_get_params(tg_trainer *t, float *params_host, float *momentum_host, size_t n);
/* test aid: one saved tensor of the last step, NHWC fp32 [B][board_size^2][64]: which 0 = Z_index (convolution output
 * before its batch norm, index 0..12), 1 = Y_index (block output, 0..6), 2 = D_index (dL/d batch-norm output, ReLU mask
 * applied, 0..12); an index outside its range is TG_ERR_ARG.  The heads' tensors (index ignored; P = board_size^2, A = P + 1):
 * 4 = hact [B][3 P] (ReLU of the head batch norms as the FC layers read it: policy channel c at c P + p, value at 2 P + p),
 * 5 = hD [B][P][4] (dL/d head batch-norm output, ReLU mask applied: policy 0, policy 1, value, one pad float),
 * 6 = dlog [B][A + 3] (dL/d logits: A policy, 3 value).  which = 3 belongs to builds with -DTG_TRAIN_PROF (phase clocks). */
int tg_trainer_debug_read(tg_trainer *t, int which, int index, float *out_host);
/* resume: momentum buffers of a loaded optimiser state (the next step is then not a "first" step) */
int tg_trainer_set_momentum(tg_trainer *t, const float *momentum_host, size_t n);

/* ---- evaluation cache (the rules: csrc/eval_cache.h; no reference counterpart) ------------------
 * A hash table in device memory that serves network outputs for input planes it has seen, keyed by the exact planes: a row
 * whose planes 0-4 hold only 0.0f / 1.0f and whose plane 5 is uniformly +1.0f or -1.0f is cacheable, every other row is
 * evaluated on every call and never inserted.  A hit returns the bits that were committed for an equal row (and the same
 * want_logits).  `entries` entries in buckets of `ways` ways.  One cache is used from one stream at a time; the caller
 * clears it when the weights behind the outputs change.  Board sizes 9, 13 and 19.
 *   create: TG_ERR_ARG for another size, ways outside 1..64 (what the probe compares in one pass), entries that are not a
 *     positive multiple of ways.
 *   probe: fills the rows of policy_dev [batch,A] / value_dev [batch,3] that hit, waits for `stream` ONCE and returns the
 *     number of rows that need the network in *n_miss and the cache's dense buffer of their planes [n_miss,6,S,S], in row
 *     order, in *miss_planes_dev (valid until the next probe).  planes_dev: 8-byte aligned.
 *   commit: the outputs of miss k (miss_policy_dev [n_miss,A], miss_value_dev [n_miss,3]) go to its row and, where the row is
 *     cacheable, into the table.  Nothing missed: launches nothing (the miss pointers may be NULL).
 *   forward: probe, tg_net_forward_dev over the misses, commit.  TG_ERR_ARG when the network's board size is not the cache's.
 *   TG_ERR_STATE, before anything is launched: a commit without a probe, a second probe (or a clear) before the commit, a
 *     commit with other output pointers than its probe's.
 *   stats: out[8] = rows looked up, hits, uncacheable rows, inserts (evictions included), twin skips (an equal row was
 *     resident or being inserted), evictions, dropped inserts, tag matches whose key differed; reset != 0 zeroes them.
 *     Synchronises the device.
 *   debug_read (test aid): entry `index` (bucket * ways + way): its tag word (0: empty; hash tag << 32 | number of the commit
 *     that wrote it), key words (5 * ceil(P / 32) + 1), policy [A] and value [3].  Synchronises the device. */
typedef struct tg_evalcache tg_evalcache;
int tg_evalcache_create(int board_size, int device, long long entries, int ways, tg_evalcache **out);
int tg_evalcache_destroy(tg_evalcache *c);
int tg_evalcache_clear(tg_evalcache *c, void *stream);
int tg_evalcache_probe(tg_evalcache *c, const float *planes_dev, int batch, int want_logits, float *policy_dev,
                       float *value_dev, void *stream, int32_t *n_miss, const float **miss_planes_dev);
int tg_evalcache_commit(tg_evalcache *c, const float *miss_policy_dev, const float *miss_value_dev, float *policy_dev,
                        float *value_dev, void *stream);
int tg_evalcache_forward(tg_evalcache *c, tg_net *net, const float *planes_dev, int batch, int want_logits,
                         float *policy_dev, float *value_dev, void *stream);
/* the rows the last probe (a forward's included) found in need of the network; no device work */
int tg_evalcache_last_misses(tg_evalcache *c, int32_t *n_miss);
int tg_evalcache_stats(tg_evalcache *c, uint64_t *out /* [8] */, int reset);
/* timing-only path (measurement; off by default, and then no event is created or recorded): on != 0 puts timed events around
 * every launch of the following probes and commits; read_timing waits for the last timed probe (and its commit, if one was
 * launched since) and returns ms[4] = the probe, rank, gather and commit kernels' times (commit 0 when none ran).
 * TG_ERR_STATE when no probe was timed. */
int tg_evalcache_set_timing(tg_evalcache *c, int on);
int tg_evalcache_read_timing(tg_evalcache *c, float *ms /* [4] */);
int tg_evalcache_debug_read(tg_evalcache *c, long long index, uint64_t *tag, uint32_t *key, float *policy, float *value);

/* ---- evaluation on game records (the rules: csrc/row_score.h; no reference counterpart) ----------
 * How well a network predicts the moves and results of held-out records, and how much of its policy falls on points the
 * tree never expands (MCTSNode.update_policy, mcts/node.py:86-93, copies the probabilities of expand_node's candidates
 * without renormalising).  Planes, network outputs, masks and row records stay in device memory.
 *   tg_replay_run_cand: tg_replay_run (same arguments, same flags, the same plane bytes; planes_dev may be NULL: no planes)
 *     that also writes, for every sample, the bit image of expand_node's candidate list (mcts/tree.py:260-264: legal, no
 *     self-atari of seven or more stones, no own complete eye, PASS) for the side to move: cand_dev [samples][ceil(A / 32)]
 *     uint32, bit a of word a / 32 set iff action a is a candidate; actions are row-major board points 0 .. P - 1 in the
 *     UNROTATED board whatever the sample's symmetry, PASS = P is always set, the bits from A on are zero.  superko != 0:
 *     positional superko as GoBoard(check_superko=True) (the handle's own Zobrist keys; results do not depend on them).
 *     The rows of a flagged game from the stopping move on are not written.
 *   tg_score_rows: n rows of policy_dev [n,A] / value_dev [n,3] (softmax, tg_net_forward_dev with want_logits 0) against
 *     move_dev [n] (action index of the move played), class_dev [n] (value label 0 / 1 / 2 from the mover's side,
 *     nn/data_generator.py) and ply_dev [n]; cand_dev [n][ceil(A / 32)] or NULL.  Writes rows_dev [n] and ADDS the rows to
 *     table_dev [n_buckets], bucket = min(ply / bucket_width, n_buckets - 1) (clear != 0: the table is zeroed first).
 *     Enqueues on `stream` and returns.  rank = actions with a larger probability + actions before the move with an equal
 *     one (rank 0 = numpy's argmax).  A row with a move or class out of range or a NaN is flagged invalid and adds to
 *     nothing but its bucket's invalid count.  No floating-point atomics: equal calls give equal table bits.
 *     TG_ERR_ARG: null pointers (cand_dev excepted), n < 0, actions < 2, bucket_width < 1, n_buckets < 1. */
#define TG_SCORE_MOVE_IS_CANDIDATE 1u /* (never set without masks) */
#define TG_SCORE_VALUE_HIT 2u         /* the first maximum of the three values is the class */
#define TG_SCORE_INVALID 4u
#define TG_SCORE_HAS_MASK 8u
typedef struct tg_score_row {
    double cand_mass; /* sum of (double)policy[a] over the set mask bits; 0 without masks */
    double brier;     /* (score - expected)^2: score 1 / 0.5 / 0 for class 2 / 1 / 0, expected = value[2] + 0.5 value[1] */
    uint32_t p_move;  /* bits of policy[move] */
    int32_t rank;
    uint32_t v_label; /* bits of value[class] */
    uint32_t flags;
    int32_t bucket;
    int32_t reserved;
} tg_score_row;
typedef struct tg_score_bucket {
    uint64_t count[6]; /* rows, rank 0, rank < 5, move not a candidate, value hits, invalid rows */
    double sum[4];     /* -log(p_move + 1e-8), cand_mass, -log(v_label + 1e-8), brier: fp64, log = tg_glibc_log's */
} tg_score_bucket;
int tg_replay_run_cand(tg_replay *r, const int32_t *moves_host, const int64_t *offsets_host, int games,
                       const int32_t *sample_ply_host, const int8_t *sample_sym_host,
                       const int64_t *sample_offsets_host /* [games+1] */, float *planes_dev /* [samples,6,S,S] or NULL */,
                       int32_t *flags_host /* [games] */, int superko, uint32_t *cand_dev /* [samples][ceil(A/32)] */,
                       void *stream);
int tg_score_rows(const float *policy_dev, const float *value_dev, const uint32_t *cand_dev, const int32_t *move_dev,
                  const int32_t *class_dev, const int32_t *ply_dev, int n, int actions, int bucket_width, int n_buckets,
                  tg_score_row *rows_dev, tg_score_bucket *table_dev, int clear, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMAGO_HIP_H */
