"""MCTSTree on MI355X - the reference's search API (mcts/tree.py:26-105,318-356,424-430)
over the device-resident search engine.

``MCTSTree(network, tree_size, batch_size, cgos_mode)`` / ``search_best_move`` / ``search``
/ ``get_root`` keep the reference's signatures and semantics: the caller's board is never
modified, the tree is rebuilt on every call, the return value is a padded-board
coordinate (PASS = 0, RESIGN = -1), and the Dirichlet / Gumbel draws come out of numpy's
GLOBAL legacy generator, whose state is advanced exactly as the reference would advance it.

``reuse_tree=True`` (off by default; no reference counterpart) keeps the subtree under the
position searched next when the board's history extends the last searched root's by expanded
child edges: the device compacts it in place (SearchEngine.reroot) and the search tops the root
up to the visit budget instead of rebuilding the tree.
"""
from typing import Any, Dict

import numpy as np

from tamago_amd.board.constant import PASS, RESIGN
from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import Stone, color_value
from tamago_amd.mcts.batch_data import BatchQueue
from tamago_amd.mcts.constant import MCTS_TREE_SIZE, NN_BATCH_SIZE, RESIGN_THRESHOLD, \
    PLAYOUTS, MAX_CONSIDERED_NODES
from tamago_amd.mcts.sequential_halving import get_candidates_and_visit_pairs
from tamago_amd.mcts.engine import SearchEngine, evaluator_for
from tamago_amd.mcts.node import MCTSNode
from tamago_amd.mcts.time_manager import TimeControl, TimeManager


class _NodeList:
    """``tree.node[i]`` -> host snapshot of node i (negative indices as in a list)."""

    def __init__(self, tree):
        self._tree = tree

    def __len__(self):
        return self._tree.tree_size

    def __getitem__(self, index: int) -> MCTSNode:
        if index < 0:
            index += self._tree.tree_size
        return self._tree._engine_for(None).read_node(0, index)


class MCTSTree:
    def __init__(self, network, tree_size: int = MCTS_TREE_SIZE, batch_size: int = NN_BATCH_SIZE,
                 cgos_mode: bool = False, device_index: int = 0, reuse_tree: bool = False,
                 unique_leaves: bool = False, device_early_stop: bool = False, poll_every=None,
                 eval_cache=None):
        self.network = network
        # (off by default) entries of an evaluation cache that serves positions whose outputs it holds - the
        # subtree under the move that is played is searched again a ply later: same trees, same moves, the searches go
        # mini-batch by mini-batch.  One cache per board size, kept across moves and games.
        self.eval_cache = int(eval_cache) if eval_cache else 0
        self._eval_caches = {}
        self.tree_size = tree_size
        self.batch_size = batch_size
        self.cgos_mode = cgos_mode
        self.device_index = device_index
        self.num_nodes = 0
        self.root = 0
        self.current_root = 0
        self.to_move = Stone.BLACK
        self._dump_to_move = Stone.BLACK           # to_dict's "to_move": the colour of the last search() / ponder() (mcts/tree.py:139)
        self.node = _NodeList(self)
        self.ponder_max_nodes = 1 << 22            # 4 M nodes = 13 GB of 9x9 pool: cap of ponder's growth
        self._engine = None
        self._engine_key = None
        self._gumbel_root = False
        self.reuse_tree = reuse_tree
        self._last_root = None                     # reuse_tree: (history, side to move, komi, engine key) of the last PUCT root
        self.reused_visits = 0                     # reuse_tree: root visits the last search started from
        # (off by default; no reference counterpart) generate_move_with_sequential_halving evaluates each distinct leaf of
        # a phase once instead of once per descent (SearchEngine.gumbel_phase(unique=True)): same tree, same move
        self.unique_leaves = unique_leaves
        # (off by default) a CONSTANT_PLAYOUT search evaluates its early-stop test on the device, behind each mini-batch's
        # backup, instead of reading the root back per mini-batch (SearchEngine.puct_chain(early_total=...)): same tree,
        # same move, same stream position.  poll_every: how often the host looks whether the search has stopped
        # (None: SearchEngine.DEFAULT_POLL_EVERY mini-batches, 0: never - everything is queued)
        self.device_early_stop = device_early_stop
        self.poll_every = poll_every

    @property
    def batch_queue(self) -> BatchQueue:
        """mcts/batch_data.py:7-34 view of the DEVICE leaf queue (input planes, paths, node indices
        of the leaves waiting for the network).  Like the reference's, it is empty whenever a
        search call has returned (every mini-batch is flushed before, tree.py:150-152,315)."""
        if self._engine is None:
            return BatchQueue()
        return self._engine.read_queue(0)

    # ------------------------------------------------------------------------------------
    def _evaluator(self):
        return evaluator_for(self.network, self.device_index)

    def _cached(self, evaluator, board_size: int):
        """The engine's evaluator behind this tree's evaluation cache for the board size (eval_cache=entries; else as it is)."""
        if not self.eval_cache:
            return evaluator
        from tamago_amd.nn.eval_cache import CachedEvaluator, EvalCache
        if board_size not in self._eval_caches:
            self._eval_caches[board_size] = EvalCache(board_size, self.eval_cache, device_index=self.device_index)
        return CachedEvaluator(evaluator, self._eval_caches[board_size])

    def _engine_for(self, board, batch_size=None):
        if board is None:
            if self._engine is None:
                raise RuntimeError("no search has run yet")
            return self._engine
        batch = batch_size or self.batch_size
        net_size = getattr(self.network, "board_size", None)
        if net_size is not None and net_size != board.board_size:
            raise ValueError(f"network is built for {net_size}x{net_size}, board is "
                             f"{board.board_size}x{board.board_size}")
        key = (board.board_size, bool(board.check_superko), batch, self.cgos_mode, self.tree_size)
        if self._engine is None or key != self._engine_key:
            if self._engine is not None:
                self._engine.close()
            self._engine = SearchEngine(board.board_size, 1, self.tree_size, batch,
                                        self._cached(self._evaluator(), board.board_size), self.cgos_mode, board.check_superko,
                                        self.device_index)
            self._engine_key = key
        return self._engine

    def close(self):
        """Release the engine and the evaluation caches now (otherwise: when the objects are collected).  The tree can be
        used again; it builds what it needs."""
        if self._engine is not None:
            self._engine.close()
            self._engine, self._engine_key, self._last_root = None, None, None
        for cache in self._eval_caches.values():
            cache.close()
        self._eval_caches = {}

    def _commit_rng(self, engine):
        """Leave numpy's global generator where the reference would have left it."""
        np.random.set_state(engine.streams[0].final_state())

    # ---- tree reuse (reuse_tree=True) ------------------------------------------------------
    @staticmethod
    def _history(board):
        """(handicap stones, ((colour, move), ...)) of the board, None when the move record is full."""
        if board.moves >= board.max_records:
            return None
        return (tuple(board.handicap_pos),
                tuple((int(board.rec_color[i]), int(board.rec_pos[i])) for i in range(1, board.moves)))

    def forget_tree(self):
        """The next search rebuilds its tree (undo, a new game, a changed komi ...)."""
        self._last_root = None

    def _remember_root(self, board, color):
        history = self._history(board) if self.reuse_tree else None
        self._last_root = None if history is None else \
            (history, color_value(color), float(board.get_komi()), self._engine_key)

    def _reusable_node(self, engine, board, color) -> int:
        """Node of the last searched tree at the board's position, -1 if the tree cannot be reused."""
        last, self._last_root = self._last_root, None
        if last is None:
            return -1
        history = self._history(board)
        old_history, to_move, komi, key = last
        if history is None or key != self._engine_key or komi != float(board.get_komi()) or history[0] != old_history[0]:
            return -1
        done, moves = old_history[1], history[1]
        if moves[:len(done)] != done:
            return -1
        node = 0
        for c, pos in moves[len(done):]:
            if c != to_move:
                return -1
            node = engine.find_child(0, node, pos)
            if node < 0:
                return -1
            to_move = 3 - to_move
        return node if to_move == color_value(color) else -1

    def _prepare_root(self, engine, board, color) -> bool:
        """_initialize_search, or (reuse_tree) the subtree of the previous search made the tree.  True if reused."""
        node = self._reusable_node(engine, board, color) if self.reuse_tree else -1
        if node < 0:
            self.reused_visits = 0
            engine.set_root(0, board, color, np.random.get_state())
            engine.root_eval(use_logit=False)                          # _initialize_search
            return False
        engine.set_root(0, board, color, np.random.get_state())
        engine.reroot([node])
        root = engine.read_node(0, 0)
        engine.node_bound = root.tree_num_nodes
        engine.root_children = np.array([root.num_children], dtype=np.int64)
        self.reused_visits = int(root.node_visits)
        return True

    def get_root(self) -> MCTSNode:
        root = self._engine_for(None).read_node(0, self.current_root)
        noise = getattr(self._engine, "noise", None)
        if noise is not None and self._gumbel_root:
            root.noise = noise[0].copy()
        return root

    # ---- whole-tree dump (mcts/tree.py:476-506) ----------------------------------------------
    DUMP_MAX_NODES = 1 << 18

    def to_dict(self, max_nodes: int = DUMP_MAX_NODES) -> Dict[str, Any]:
        """mcts/tree.py:489-506: the tree as plain Python values (tamago_amd/mcts/dump.py tree_to_dict says which), every
        node read out of the device pool in a fixed number of launches (SearchEngine.dump_trees).  Before any search: the
        empty tree.  max_nodes: a tree of more nodes raises instead of being turned into Python lists (a ponder-grown pool
        holds millions of nodes).

        One deviation from the reference: its expand() does not clear children_policy (mcts/node.py:41-59), so node objects
        that a second search reuses keep stale policies beyond num_children; here that tail is zero.  The dump of a tree's
        first search equals the reference's in every element, later searches everywhere except that tail."""
        from tamago_amd.mcts import dump
        # (the reference sets its to_move in search() alone, tree.py:139: a sequential-halving search and a root whose only
        # candidate is the pass leave it as it was)
        to_move = "black" if self._dump_to_move == Stone.BLACK else "white"
        if self._engine is None:
            return dump.empty_tree_dict(self.batch_size, self.cgos_mode, to_move)
        nodes = int(self._engine.dump_sizes([0])[0][0])
        if nodes > max_nodes:
            raise ValueError(f"the tree holds {nodes} nodes, more than max_nodes = {max_nodes}: a dump of it as Python "
                             f"lists would take about {nodes * self._engine.A * 60 >> 20} MiB - pass a larger max_nodes "
                             "to dump it all the same")
        noise = getattr(self._engine, "noise", None)
        packed = self._engine.dump_trees([0])[0]
        return dump.tree_to_dict(packed, self._engine.A, self.batch_size, self.cgos_mode,
                                 noise=noise[0] if noise is not None and self._gumbel_root else None, to_move=to_move)

    def dump_to_json(self, board: GoBoard, superko: bool, max_nodes: int = DUMP_MAX_NODES) -> str:
        """mcts/tree.py:476-486."""
        from tamago_amd.mcts import dump
        return dump.dump_mcts_to_json(self.to_dict(max_nodes), board, superko)

    # ---- whole-tree load (no reference counterpart: the reference cannot read its own dumps) ----
    def load_dict(self, tree_dict: Dict[str, Any], board: GoBoard, color, verify: bool = True) -> None:
        """to_dict()'s inverse: the tree of a tree dict (ours or the reference's) becomes this MCTSTree's tree at `board`'s
        position with `color` to move, in the engine _engine_for builds for the board.  The root is remembered: with
        reuse_tree=True the next search_best_move on that position tops the loaded root up to its visit budget, without it
        the next search rebuilds as ever.  verify: every node's position is reached by replaying its path from the root on a
        GoBoard and every action must be the pass or legal there (dump.verify_tree), else ValueError before anything reaches
        the device.  A tree with a virtual loss anywhere is refused: a dump taken between a selection and its backup cannot
        be continued.  The dict's root noise row is put back when it holds anything (a sequential-halving dump).

        The dict's "to_move" is not read here - `color` is the side to move - because the reference sets it in search()
        alone (mcts/tree.py:139): a sequential-halving dump says "black" whatever moved."""
        from tamago_amd.mcts import dump
        packed = dump.packed_of_dict(tree_dict)
        side = color if isinstance(color, Stone) else Stone(color_value(color))
        packed["to_move"] = color_value(side)
        if packed["num_nodes"] and (np.any(packed["virtual_loss"] != 0) or np.any(packed["children_virtual_loss"] != 0)):
            raise ValueError("the tree holds virtual losses: it was dumped between a selection and its backup")
        if tree_dict.get("current_root", 0) != 0:
            raise ValueError("only trees whose current_root is node 0 can be loaded")
        if verify:
            dump.verify_tree(packed, board, side)
        from tamago_amd import lib as _lib
        records = dump.make_record(packed)
        offsets = np.array([0, records.size], dtype=np.int64)
        # (the check needs no engine: a tree that cannot enter leaves this MCTSTree's engine and tree as they were)
        _lib.check(_lib.load().tg_search_check_records(board.get_board_size(), self.tree_size, records.ctypes.data,
                                                       offsets.ctypes.data, 1), "tg_search_check_records")
        engine = self._engine_for(board)
        engine.set_root(0, board, side)
        engine.load_trees([packed], [0])
        noise = np.asarray(tree_dict["node"][0].get("noise", []), dtype=np.float64) if packed["num_nodes"] else np.zeros(0)
        self._gumbel_root = bool(noise.size == engine.A and np.any(noise != 0.0))
        if self._gumbel_root:
            engine.noise = noise.reshape(1, engine.A).copy()
            _lib.check(engine.lib.tg_search_set_noise(engine.handle, engine.noise.ctypes.data), "tg_search_set_noise")
        self.to_move = side
        self._dump_to_move = Stone.WHITE if tree_dict.get("to_move") == "white" else Stone.BLACK
        self.num_nodes = int(packed["num_nodes"])
        self.reused_visits = 0
        self._remember_root(board, side)

    def load_json(self, text: str, color=None, verify: bool = True):
        """dump_to_json()'s inverse (mcts/dump.py:10-33 read back): -> (board, color).  The board is set up from the text's
        history, komi and superko.  color defaults to the dump's "to_move" - note the reference's quirk (load_dict): pass
        the colour for a sequential-halving dump of a white move."""
        from tamago_amd.mcts import dump
        tree_dict, board, _ = dump.load_mcts_from_json(text)
        if color is None:
            color = Stone.WHITE if tree_dict.get("to_move") == "white" else Stone.BLACK
        self.load_dict(tree_dict, board, color, verify=verify)
        return board, color

    # ------------------------------------------------------------------------------------
    def search_best_move(self, board: GoBoard, color, time_manager: TimeManager,
                         analysis_query: Dict[str, Any] = None) -> int:
        """mcts/tree.py:57-105.  The reference doubles its node list when it fills up
        (tree.py:254-258); the device pool is grown in place the same way between mini-batches
        (SearchEngine.ensure_capacity -> tg_search_grow), so a search is never repeated and the
        clock keeps running over a growth."""
        return self._search_best_move(board, color, time_manager, analysis_query)

    def _sync_size(self, engine):
        """tree_size follows the pool (len(tree.node) after the reference's doubling)."""
        if engine.N != self.tree_size:
            self.tree_size = engine.N
            key = self._engine_key
            self._engine_key = key[:4] + (engine.N,)

    def _search_best_move(self, board, color, time_manager, analysis_query):
        engine = self._engine_for(board)
        self._gumbel_root = False
        self.to_move = color if isinstance(color, Stone) else Stone(color_value(color))
        self._prepare_root(engine, board, color)
        time_manager.start_timer()
        if int(engine.root_children[0]) == 1:                              # tree.py:76-77 (the root's child count off the draw cursor)
            self.num_nodes = int(engine.num_nodes()[0])
            self._commit_rng(engine)
            self._remember_root(board, color)
            return PASS
        self.search(board, color, time_manager, analysis_query or {}, _engine=engine, _visits=self.reused_visits)
        root = engine.read_node(0, 0)
        self.num_nodes = root.tree_num_nodes
        self._sync_size(engine)
        self._commit_rng(engine)
        self._remember_root(board, color)
        search_time = time_manager.calculate_consumption_time()
        time_manager.set_search_speed(root.node_visits - self.reused_visits, max(search_time, 1e-9))
        time_manager.substract_consumption_time(color, search_time)
        next_index = root.get_best_move_index()
        if root.calculate_value_evaluation(next_index) < RESIGN_THRESHOLD:
            return RESIGN
        return root.action[next_index]

    def search(self, board: GoBoard, color, time_manager: TimeManager,
               analysis_query: Dict[str, Any] = None, _engine=None, _visits: int = 0):
        """mcts/tree.py:130-152: `threshold` descents in mini-batches of batch_size; the
        early-stop test (time_manager.py:135-163) runs after every mini-batch, which is
        where its inputs change.  `_visits`: root visits a reused tree starts with - the threshold
        is a total, so threshold - _visits descents run (the early-stop test is total-based already)."""
        engine = _engine or self._engine_for(board)
        self._dump_to_move = color if isinstance(color, Stone) else Stone(color_value(color))
        total = time_manager.get_num_visits_threshold(color)
        threshold = max(0, total - _visits)
        if _visits and threshold > 0 and time_manager.mode != TimeControl.STRICT_PLAYOUT and not analysis_query and \
                time_manager.is_move_decided(engine.read_node(0, 0), total):
            # the reference tests after every descent (tree.py:150): a reused root that already decides the move stops
            # after the first one (a fresh root never does - it has no visits)
            threshold = 1
        done = 0
        # tree.py:168-174 prints the final analysis (interval 0) at the end of search() - BEFORE search_best_move flushes the
        # last, partial mini-batch (tree.py:84-85): its leaves are selected (virtual losses in place) but not yet evaluated
        # or backed up, and the printed visit counts do not include them
        late_analysis = bool(analysis_query) and analysis_query.get("interval", 0) == 0
        pending = False
        if threshold > 0 and time_manager.mode == TimeControl.STRICT_PLAYOUT and not analysis_query and engine.can_chain(threshold):
            # nothing between the mini-batches depends on their results (no early stop, the 10 000 s limit never ends it): queue them all
            batches = [self.batch_size] * (threshold // self.batch_size)
            if threshold % self.batch_size:
                batches.append(threshold % self.batch_size)
            engine.puct_chain(batches)
            done = threshold
        elif threshold > 0 and self.device_early_stop and time_manager.mode == TimeControl.CONSTANT_PLAYOUT and not analysis_query \
                and _visits == 0:
            # the early-stop test is the only thing between the mini-batches (the 10 000 s limit never ends the search): it runs
            # on the device, which halts the tree where the loop below would break - the launches queued behind do nothing.
            # Queued in one call where engine.can_chain holds; mini-batch by mini-batch otherwise, the device's test in between
            batches = [self.batch_size] * (threshold // self.batch_size)
            if threshold % self.batch_size:
                batches.append(threshold % self.batch_size)
            engine.puct_chain(batches, early_total=total, poll_every=self.poll_every)
            done = threshold
        while done < threshold:
            leaves = min(self.batch_size, threshold - done)
            engine.ensure_capacity(leaves)
            if late_analysis and leaves < self.batch_size and done + leaves == threshold:
                engine.puct_select(leaves)
                pending = True
            else:
                engine.puct_batch(leaves)
            done += leaves
            if leaves == self.batch_size and done < threshold:
                if time_manager.is_time_over():
                    break
                # STRICT_PLAYOUT never decides early (time_manager.py:160-161): no root read-back
                if time_manager.mode != TimeControl.STRICT_PLAYOUT and \
                        time_manager.is_move_decided(engine.read_node(0, 0), total):
                    break
        if analysis_query and analysis_query.get("interval", 0) == 0:      # tree.py:170-174
            import sys
            sys.stdout.write(engine.read_node(0, 0).get_analysis(board, analysis_query.get("mode", "lz"),
                                                                 self.get_pv_lists))
            sys.stdout.flush()
        if pending:
            engine.puct_flush()

    def ponder(self, board: GoBoard, color, analysis_query: Dict[str, Any]):
        """mcts/tree.py:108-127: search without a visit limit until input arrives on stdin
        (``analysis_query["ponder"]``), printing analysis every ``interval`` seconds.  The
        reference polls stdin after every descent; here the poll sits between mini-batches (a
        batch in flight is finished), input that is already waiting stops after one descent.
        The node pool doubles when the next mini-batch might not fit (tree.py:254-258), up to
        `ponder_max_nodes` nodes (the reference is bounded by host memory only)."""
        import select
        import sys
        import time
        engine = self._engine_for(board)
        self._gumbel_root = False
        self.to_move = color if isinstance(color, Stone) else Stone(color_value(color))
        self._dump_to_move = self.to_move
        self._prepare_root(engine, board, color)
        query = analysis_query or {}
        interval = query.get("interval", 0)
        mode = query.get("mode", "lz")
        clock = time.time()

        def stdin_ready():
            if not query.get("ponder", False):
                return False
            ready, _, _ = select.select([sys.stdin], [], [], 0)
            return bool(ready)

        if engine.read_node(0, 0).get_num_children() > 1:
            while True:
                if engine.node_bound + self.batch_size > engine.N:
                    engine.node_bound = int(engine.num_nodes()[0])
                    if engine.node_bound + self.batch_size > engine.N and \
                            engine.N * 2 > self.ponder_max_nodes:
                        break
                engine.ensure_capacity(self.batch_size)
                waiting = stdin_ready()
                engine.puct_batch(1 if waiting else self.batch_size)
                if waiting or stdin_ready():
                    break
                if query and interval > 0 and time.time() - clock > interval:
                    clock = time.time()
                    sys.stdout.write(engine.read_node(0, 0).get_analysis(board, mode, self.get_pv_lists))
                    sys.stdout.flush()
        if query and interval == 0:                                    # tree.py:170-174
            sys.stdout.write(engine.read_node(0, 0).get_analysis(board, mode, self.get_pv_lists))
            sys.stdout.flush()
        self.num_nodes = int(engine.num_nodes()[0])
        self._sync_size(engine)
        self._commit_rng(engine)
        self._remember_root(board, color)

    def search_with_callback(self, board: GoBoard, color, callback):
        """mcts/tree.py:177-196: one descent at a time (mini-batches of one leaf); the callback
        gets the descent's [(node index, child index), ...] and ends the search by returning True."""
        engine = self._engine_for(board, batch_size=1)
        self._gumbel_root = False
        self._last_root = None
        self.to_move = color if isinstance(color, Stone) else Stone(color_value(color))
        engine.set_root(0, board, color, np.random.get_state())
        engine.root_eval(use_logit=False)
        while True:
            engine.ensure_capacity(1)
            engine.puct_batch(1)
            if callback(engine.read_path(0, 0)):
                break
        self.num_nodes = int(engine.num_nodes()[0])
        self._sync_size(engine)
        self._commit_rng(engine)

    # ---- principal variations (mcts/tree.py:432-473) -----------------------------------------
    def get_pv_lists(self, root: MCTSNode, coord) -> Dict[str, Any]:
        pv = {}
        for i in range(root.num_children):
            if root.children_visits[i] > 0:
                seq = self.get_best_move_sequence([root.action[i]], int(root.children_index[i]))
                pv[coord.convert_to_gtp_format(root.action[i])] = \
                    [coord.convert_to_gtp_format(p) for p in seq]
        return pv

    def get_best_move_sequence(self, pv_list, index: int):
        node = self.node[index]
        if node.node_visits == 0:
            return pv_list
        best = node.get_best_move_index()
        pv_list.append(node.action[best])
        nxt = int(node.children_index[best])
        if nxt == -1:
            return pv_list
        return self.get_best_move_sequence(pv_list, nxt)

    # ------------------------------------------------------------------------------------
    def generate_move_with_sequential_halving(self, board: GoBoard, color, time_manager: TimeManager,
                                              never_resign: bool) -> int:
        """mcts/tree.py:318-356 (Gumbel AlphaZero root + sequential halving)."""
        import time as _time
        start = _time.time()
        visits = time_manager.get_num_visits_threshold(color)
        # every phase is one mini-batch of num_considered * max_count leaves (<= visits)
        engine = self._engine_for(board, batch_size=max(visits, 1))
        self._gumbel_root = True
        self._last_root = None
        engine.set_root(0, board, color, np.random.get_state())
        engine.root_eval(use_logit=True)
        engine.set_gumbel_noise()
        nc = engine.root_children                  # (child count off the draw cursor: no read-back behind the root evaluation)
        base = int(nc[0]) if nc[0] < MAX_CONSIDERED_NODES else MAX_CONSIDERED_NODES
        for num_considered, max_count in get_candidates_and_visit_pairs(base, visits).items():
            engine.ensure_capacity(num_considered * max_count)
            engine.gumbel_phase([num_considered], [max_count], unique=self.unique_leaves)
        root = self.get_root()
        self.num_nodes = root.tree_num_nodes
        self._commit_rng(engine)
        next_index = root.select_move_by_sequential_halving_for_root(PLAYOUTS)
        value = root.calculate_value_evaluation(next_index)
        time_manager.set_search_speed(root.node_visits, max(_time.time() - start, 1e-9))
        if not never_resign and value < 0.05:
            return RESIGN
        return root.get_child_move(next_index)
