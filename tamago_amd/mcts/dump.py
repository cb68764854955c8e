"""Whole-tree dumps (mcts/dump.py:10-168 of the reference, and the ``to_dict`` pair mcts/tree.py:489-506 /
mcts/node.py:221-253) over the device's packed tree records (csrc/tree_dump.h).

Three forms of one tree:

* the *record*: the bytes ``tg_search_dump_trees`` returns (``parse_record`` reads them);
* the *packed tree*: a dict of numpy arrays - the tree's scalars, one entry per node of every node scalar, and one flat row
  per child array that holds the first ``num_children`` entries of node 0, then of node 1, ... (``first_child`` says where a
  node's entries start).  ``SearchEngine.dump_trees`` returns these; ``pack_nodes`` builds one from node objects on the host;
* the *tree dict*: the reference's ``MCTSTree.to_dict()`` shape, plain Python values ready for ``json.dumps``
  (``tree_to_dict``).

Scalar conversion of ``tree_to_dict``: counts and indices are Python ints, float64 entries Python floats, ``raw_value`` and
``node_value_sum`` the Python float of their float32 (the reference holds a numpy float32 there once a value has been backed up;
the conversion is exact).  Arrays have the full length S*S+1 with canonical tails beyond ``num_children``:
``children_index`` -1 (NOT_EXPANDED), everything else 0.

One known deviation.  The reference's ``expand`` does not clear ``children_policy`` (mcts/node.py:41-59), so a node OBJECT that
a second search of the same ``MCTSTree`` reuses keeps stale policies beyond ``num_children``; ours are zero.  The dump of an
``MCTSTree``'s first search equals the reference's in every element, later searches everywhere except that tail.
"""
import json
from typing import Any, Dict, List, Optional

import numpy as np

from tamago_amd.board.coordinate import Coordinate
from tamago_amd.board.go_board import GoBoard, copy_board
from tamago_amd.board.stone import Stone
from tamago_amd.mcts.constant import NOT_EXPANDED

PROGRAM_NAME = "TamaGo"            # program.py:3-5
VERSION = "0.10.0"
PROTOCOL_VERSION = "2"

# ---- the layout of csrc/tree_dump.h, restated (tests/test_tree_dump_host.py holds the two together) ----------------------
HEAD_WORDS = 8                     # num_nodes, current_root, err, to_move, total children (low, high), 0, 0
NODE_DTYPE = np.dtype([("node_visits", "<i4"), ("virtual_loss", "<i4"), ("node_value_sum", "<f4"), ("raw_value", "<f4"),
                       ("num_children", "<i4"), ("parent", "<i4"), ("pedge", "<i4"), ("pad", "<i4"), ("first_child", "<i8")])
# the pool's child arrays in node_pool.h's order: (key of the tree dict, pool member, element type in a record)
CHILD_ARRAYS = (("children_index", "ch_index", np.int32), ("children_visits", "ch_visits", np.int32),
                ("children_virtual_loss", "ch_vl", np.int32), ("children_value_sum", "ch_vsum", np.float64),
                ("children_policy", "ch_policy", np.float64), ("children_value", "ch_value", np.float64),
                ("action", "action", np.int32))
NODE_SCALARS = ("node_visits", "virtual_loss", "node_value_sum", "raw_value", "num_children")
# digest fields (tg_dump::Field) and seeds
FIELD_NUM_NODES, FIELD_CURRENT_ROOT, FIELD_NODE_SCALARS, FIELD_ARRAYS = 0, 1, 2, 16
SEEDS = (0x243F6A8885A308D3, 0x13198A2E03707344)


def node_offset(i: int) -> int:
    return HEAD_WORDS * 4 + i * NODE_DTYPE.itemsize


def row_offsets(n: int, total: int) -> Dict[str, int]:
    """Where each row starts in the record of a tree of n nodes and `total` children; "end": the record's size."""
    at = node_offset(n)
    out = {}
    for wide in (False, True):
        if wide:
            at = (at + 7) & ~7
        for key, _, dtype in CHILD_ARRAYS:
            if (np.dtype(dtype).itemsize == 8) == wide:
                out[key] = at
                at += total * (8 if wide else 4)
    out["end"] = (at + 7) & ~7
    return out


def record_bytes(n: int, total: int) -> int:
    return row_offsets(n, total)["end"]


def parse_record(buf) -> Dict[str, Any]:
    """One record (bytes-like, starting at the record) -> packed tree.  The arrays are copies."""
    buf = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    head = buf[:HEAD_WORDS * 4].view("<i4")
    n = int(head[0])
    total = int(np.uint32(head[4])) | (int(np.uint32(head[5])) << 32)
    nodes = buf[node_offset(0):node_offset(n)].view(NODE_DTYPE)
    tree = {"num_nodes": n, "current_root": int(head[1]), "err": int(head[2]), "to_move": int(head[3]), "total_children": total}
    for name in NODE_DTYPE.names:
        if name != "pad":
            tree[name] = nodes[name].copy()
    at = row_offsets(n, total)
    for key, _, dtype in CHILD_ARRAYS:
        size = np.dtype(dtype).itemsize
        tree[key] = buf[at[key]:at[key] + total * size].view(np.dtype(dtype).newbyteorder("<")).copy()
    return tree


def pack_nodes(nodes, num_nodes: int, current_root: int = 0, to_move: int = 1) -> Dict[str, Any]:
    """Packed tree of the first num_nodes node objects (MCTSNode attributes: the host half of the read-out, for trees that
    live on the host)."""
    nc = np.array([int(nodes[i].num_children) for i in range(num_nodes)], dtype=np.int32)
    first = np.zeros(num_nodes, dtype=np.int64)
    if num_nodes:
        first[1:] = np.cumsum(nc.astype(np.int64))[:-1]
    tree = {"num_nodes": int(num_nodes), "current_root": int(current_root), "err": 0, "to_move": int(to_move),
            "total_children": int(nc.sum()), "num_children": nc, "first_child": first,
            "node_visits": np.array([int(nodes[i].node_visits) for i in range(num_nodes)], dtype=np.int32),
            "virtual_loss": np.array([int(nodes[i].virtual_loss) for i in range(num_nodes)], dtype=np.int32),
            "node_value_sum": np.array([np.float32(nodes[i].node_value_sum) for i in range(num_nodes)], dtype=np.float32),
            "raw_value": np.array([np.float32(nodes[i].raw_value) for i in range(num_nodes)], dtype=np.float32),
            "parent": np.full(num_nodes, -1, dtype=np.int32), "pedge": np.full(num_nodes, -1, dtype=np.int32)}
    for key, _, dtype in CHILD_ARRAYS:
        rows = [np.asarray(getattr(nodes[i], key)[:nc[i]], dtype=dtype) for i in range(num_nodes)]
        tree[key] = np.concatenate(rows) if rows else np.zeros(0, dtype=dtype)
    return tree


def _node_dict(tree: Dict[str, Any], i: int, num_actions: int, noise) -> Dict[str, Any]:
    nc = int(tree["num_children"][i])
    lo = int(tree["first_child"][i])
    state = {                                                                   # the thirteen keys of mcts/node.py:227-241
        "node_visits": int(tree["node_visits"][i]),
        "virtual_loss": int(tree["virtual_loss"][i]),
        "node_value_sum": float(tree["node_value_sum"][i]),
        "raw_value": float(tree["raw_value"][i]),
    }
    for key in ("action", "children_index", "children_value", "children_visits", "children_policy",
                "children_virtual_loss", "children_value_sum"):
        tail = NOT_EXPANDED if key == "children_index" else (0.0 if tree[key].dtype.kind == "f" else 0)
        state[key] = tree[key][lo:lo + nc].tolist() + [tail] * (num_actions - nc)
    state["noise"] = [float(v) for v in noise] if noise is not None else [0.0] * num_actions
    state["num_children"] = nc
    return state


def tree_to_dict(tree: Dict[str, Any], num_actions: int, batch_size: int, cgos_mode: bool, noise=None,
                 to_move: Optional[str] = None) -> Dict[str, Any]:
    """mcts/tree.py:489-506 over a packed tree.  noise: the root's Gumbel noise row [num_actions] (MCTSNode.noise of the root
    view), None for zeros; every other node's noise is zero.  to_move: 'black' / 'white' (default: the packed tree's side)."""
    root = tree["current_root"]
    return {
        "node": [_node_dict(tree, i, num_actions, noise if i == root else None) for i in range(tree["num_nodes"])],
        "num_nodes": tree["num_nodes"],
        "root": 0,
        "current_root": root,
        "batch_size": batch_size,
        "cgos_mode": cgos_mode,
        "to_move": to_move or ("white" if tree["to_move"] == Stone.WHITE.value else "black"),
    }


def empty_tree_dict(batch_size: int, cgos_mode: bool, to_move: str = "black") -> Dict[str, Any]:
    """to_dict() of an MCTSTree that has not searched (mcts/tree.py:39-55: num_nodes 0)."""
    return {"node": [], "num_nodes": 0, "root": 0, "current_root": 0, "batch_size": batch_size, "cgos_mode": cgos_mode,
            "to_move": to_move}


# ---- the digest of csrc/tree_dump.h in numpy ------------------------------------------------------------------------------
def _mix(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _bits(values: np.ndarray) -> np.ndarray:
    """Values by their bit patterns, zero-extended to 64 bits: int32 / float32 as 32 bits, float64 as 64."""
    values = np.ascontiguousarray(values)
    if values.dtype.itemsize == 8:
        return values.view(np.uint64)
    return values.view(np.uint32).astype(np.uint64)


def _terms(seed: int, field: int, node: np.ndarray, child: np.ndarray, bits: np.ndarray) -> np.uint64:
    with np.errstate(over="ignore"):
        key = (np.uint64(field) << np.uint64(42)) | (node.astype(np.uint64) << np.uint64(10)) | child.astype(np.uint64)
        return np.sum(_mix(_mix(key ^ np.uint64(seed)) + bits), dtype=np.uint64)


def digest_of_packed(tree: Dict[str, Any]) -> np.ndarray:
    """[2] uint64: tg_search_tree_digests' words of a packed tree."""
    n = tree["num_nodes"]
    nodes = np.arange(n, dtype=np.int64)
    zeros = np.zeros(n, dtype=np.int64)
    nc = tree["num_children"].astype(np.int64)
    owner = np.repeat(nodes, nc)
    child = np.arange(int(nc.sum()), dtype=np.int64) - np.repeat(tree["first_child"].astype(np.int64), nc)
    zero = np.zeros(1, dtype=np.int64)
    out = np.zeros(2, dtype=np.uint64)
    for w, seed in enumerate(SEEDS):
        with np.errstate(over="ignore"):
            total = _terms(seed, FIELD_NUM_NODES, zero, zero, _bits(np.array([n], dtype=np.int32)))
            total += _terms(seed, FIELD_CURRENT_ROOT, zero, zero, _bits(np.array([tree["current_root"]], dtype=np.int32)))
            for k, name in enumerate(NODE_SCALARS):
                dtype = np.float32 if name in ("node_value_sum", "raw_value") else np.int32
                total += _terms(seed, FIELD_NODE_SCALARS + k, nodes, zeros, _bits(tree[name].astype(dtype)))
            for k, (key, _, dtype) in enumerate(CHILD_ARRAYS):
                total += _terms(seed, FIELD_ARRAYS + k, owner, child, _bits(tree[key].astype(dtype)))
            out[w] = _mix(np.array([total + np.uint64(seed)], dtype=np.uint64))[0]
    return out


class _DictNode:
    def __init__(self, state):
        self.__dict__.update(state)


def digest_of(tree_dict: Dict[str, Any]) -> np.ndarray:
    """[2] uint64: the device digest of the tree a tree dict describes (entries beyond num_children are not read)."""
    nodes = [_DictNode(state) for state in tree_dict["node"]]
    return digest_of_packed(pack_nodes(nodes, tree_dict["num_nodes"], tree_dict["current_root"]))


# ---- mcts/dump.py ---------------------------------------------------------------------------------------------------------
def _stone_to_str(color) -> str:                                                # dump.py:142-143
    return "black" if color == Stone.BLACK else "white"


def _str_to_stone(text: str) -> Stone:                                          # dump.py:145-146
    return Stone.BLACK if text == "black" else Stone.WHITE


def _opposite(color: str) -> str:                                               # dump.py:113-114
    return "white" if color == "black" else "black"


def _black_winrate(value, last_move_color: str):                                # dump.py:116-117
    return value if last_move_color == "black" else 1.0 - value


def dump_mcts_to_json(tree_dict: Dict[str, Any], board: GoBoard, superko: bool) -> str:
    """dump.py:10-33: the tree dict and what is needed to set its root position up again, as one JSON text."""
    state = {
        "dump_version": 2,
        "tree": tree_dict,
        "board_size": board.get_board_size(),
        "komi": board.get_komi(),
        "move_history": [(_stone_to_str(color), int(pos)) for color, pos, _ in board.get_move_history()],    # dump.py:119-128
        "handicap_history": [int(pos) for pos in board.get_handicap_history()],
        "superko": superko,
        "name": PROGRAM_NAME,
        "version": VERSION,
        "protocol_version": PROTOCOL_VERSION,
    }
    return json.dumps(state)


def _board_after(root_board: GoBoard, first_color: Stone, gtp_moves: List[str]) -> str:
    """dump.py:148-168: the board diagram behind a line of moves from the root."""
    coord = Coordinate(board_size=root_board.get_board_size())
    board = GoBoard(board_size=root_board.get_board_size(), komi=root_board.get_komi(), check_superko=root_board.check_superko)
    copy_board(dst=board, src=root_board)
    color = first_color
    for move in gtp_moves:
        board.put_stone(coord.convert_from_gtp_format(move), color)
        color = Stone.get_opponent_color(color)
    return board.get_board_string()


def enrich_mcts_dict(state: Dict[str, Any]) -> None:
    """dump.py:35-111: adds, in place, what a viewer wants per node - its index, parent and slot among the siblings, the
    siblings' rank by visits (order), level, the moves and ranks along its path, the side to move, the board diagram and, for
    every node but the root, the parent's statistics of its edge with mean value and the two black win rates - and the
    breadth-first list of the nodes (parents first, siblings by rank) as tree["sorted_indices_list"]."""
    root_board = GoBoard(board_size=state["board_size"], komi=state["komi"], check_superko=state["superko"])
    root_board.set_history([(_str_to_stone(color), pos, None) for color, pos in state["move_history"]],       # dump.py:130-140
                           state["handicap_history"])
    coord = Coordinate(board_size=root_board.get_board_size())
    tree = state["tree"]
    node = tree["node"]

    for index, item in enumerate(node):                                         # dump.py:51-62
        item["index"] = index
        for slot, child_index in enumerate(item["children_index"]):
            if child_index == NOT_EXPANDED:
                continue
            child = node[child_index]
            child["parent_index"] = index
            child["index_in_brother"] = slot
            assert index < child_index, "Parent index must be less than child index."
            assert child_index < tree["num_nodes"], "Child index must be less than num_nodes."

    order_list = []                                                             # dump.py:65-80
    tree["sorted_indices_list"] = order_list
    queue = [node[tree["current_root"]]] if node else []
    while queue:
        item = queue.pop(0)
        order_list.append(item["index"])
        expanded = [i for i in item["children_index"] if i != NOT_EXPANDED]
        item["expanded_children_index"] = expanded
        children = sorted((node[i] for i in expanded), key=lambda child: child["node_visits"], reverse=True)
        for order, child in enumerate(children):
            child["order"] = order
        queue += children

    first_color = _str_to_stone(tree["to_move"])                                # dump.py:83-111
    for item in node:
        if "parent_index" not in item:
            item["level"] = 0
            item["orders_along_path"] = []
            item["gtp_moves_along_path"] = []
            item["to_move"] = tree["to_move"]
            item["board_string"] = root_board.get_board_string()
            continue
        parent = node[item["parent_index"]]
        slot = item["index_in_brother"]
        gtp_move = coord.convert_to_gtp_format(parent["action"][slot])
        item["level"] = parent["level"] + 1
        item["orders_along_path"] = [*parent["orders_along_path"], item["order"]]
        item["to_move"] = _opposite(parent["to_move"])
        item["gtp_moves_along_path"] = [*parent["gtp_moves_along_path"], gtp_move]
        item["board_string"] = _board_after(root_board, first_color, item["gtp_moves_along_path"])
        item["policy"] = parent["children_policy"][slot]
        item["visits"] = parent["children_visits"][slot]
        item["value"] = parent["children_value"][slot]
        item["value_sum"] = parent["children_value_sum"][slot]
        item["gtp_move"] = gtp_move
        item["mean_value"] = item["value_sum"] / item["visits"]
        last_move_color = _opposite(item["to_move"])
        item["raw_black_winrate"] = _black_winrate(item["value"], last_move_color)
        item["mean_black_winrate"] = _black_winrate(item["mean_value"], last_move_color)


# ---- the way back: tree dict -> packed tree -> record --------------------------------------------------------
def make_record(tree: Dict[str, Any]) -> np.ndarray:
    """Packed tree -> the bytes of its record (uint8 array): parse_record's inverse, tg_search_load_trees' input."""
    n, total = int(tree["num_nodes"]), int(tree["total_children"])
    at = row_offsets(n, total)
    buf = np.zeros(at["end"], dtype=np.uint8)
    head = buf[:HEAD_WORDS * 4].view("<i4")
    head[0], head[1], head[2], head[3] = n, int(tree["current_root"]), int(tree["err"]), int(tree["to_move"])
    head[4:6] = np.array([total & 0xFFFFFFFF, total >> 32], dtype=np.uint32).view(np.int32)
    nodes = buf[node_offset(0):node_offset(n)].view(NODE_DTYPE)
    for name in NODE_DTYPE.names:
        if name != "pad":
            nodes[name] = tree[name]
    for key, _, dtype in CHILD_ARRAYS:
        size = np.dtype(dtype).itemsize
        row = np.ascontiguousarray(tree[key], dtype=np.dtype(dtype).newbyteorder("<"))
        if row.size != total:
            raise ValueError(f"make_record: {key} holds {row.size} entries, total_children is {total}")
        buf[at[key]:at[key] + total * size] = row.view(np.uint8)
    return buf


def link_parents(tree: Dict[str, Any]) -> Dict[str, Any]:
    """parent / pedge of every node from children_index, in place (pack_nodes leaves them -1: node objects do not know their
    parents).  A node two edges name keeps the last; tg_search_check_records refuses such a tree."""
    nc = tree["num_children"].astype(np.int64)
    owner = np.repeat(np.arange(tree["num_nodes"], dtype=np.int64), nc)
    slot = np.arange(int(nc.sum()), dtype=np.int64) - np.repeat(tree["first_child"].astype(np.int64), nc)
    index = tree["children_index"].astype(np.int64)
    named = (index > 0) & (index < tree["num_nodes"])
    parent = np.full(tree["num_nodes"], -1, dtype=np.int32)
    pedge = np.full(tree["num_nodes"], -1, dtype=np.int32)
    parent[index[named]] = owner[named]
    pedge[index[named]] = slot[named]
    tree["parent"], tree["pedge"] = parent, pedge
    return tree


def packed_of_dict(tree_dict: Dict[str, Any]) -> Dict[str, Any]:
    """Tree dict (MCTSTree.to_dict's shape, ours or the reference's) -> packed tree with parents linked.  Entries at or beyond
    num_children are not read; "to_move" is the dict's."""
    nodes = [_DictNode(state) for state in tree_dict["node"]]
    to_move = Stone.WHITE.value if tree_dict.get("to_move") == "white" else Stone.BLACK.value
    return link_parents(pack_nodes(nodes, tree_dict["num_nodes"], tree_dict["current_root"], to_move))


def load_mcts_from_json(text: str):
    """dump_mcts_to_json's inverse: (tree dict, GoBoard set up by set_history with the dump's komi, superko)."""
    state = json.loads(text)
    if state.get("dump_version") != 2:
        raise ValueError(f"dump_version {state.get('dump_version')!r}: only version 2 dumps are read")
    for key in ("tree", "board_size", "komi", "move_history", "handicap_history", "superko"):
        if key not in state:
            raise ValueError(f"the dump has no {key!r}")
    superko = bool(state["superko"])
    board = GoBoard(board_size=int(state["board_size"]), komi=state["komi"], check_superko=superko)
    board.set_history([(_str_to_stone(color), pos, None) for color, pos in state["move_history"]], state["handicap_history"])
    tree = state["tree"]
    for key in ("node", "num_nodes", "current_root", "to_move"):
        if key not in tree:
            raise ValueError(f"the dump's tree has no {key!r}")
    if tree["num_nodes"] != len(tree["node"]) and tree["num_nodes"] > len(tree["node"]):
        raise ValueError(f"the dump's tree names {tree['num_nodes']} nodes and holds {len(tree['node'])}")
    return tree, board, superko


def verify_tree(tree: Dict[str, Any], board: GoBoard, color) -> None:
    """Every node's position reached by replaying its path from the root on a GoBoard: every action of every node must be the
    pass or legal for the side to move there, else ValueError.  tree: a packed tree with parents linked; board: the root
    position (not modified); color: the side to move at the root."""
    from tamago_amd.board.constant import PASS
    n = int(tree["num_nodes"])
    if n == 0:
        return
    first = tree["first_child"]
    nc = tree["num_children"]
    index, action = tree["children_index"], tree["action"]
    root_color = color if isinstance(color, Stone) else Stone(int(color))

    def fresh():
        b = GoBoard(board_size=board.get_board_size(), komi=board.get_komi(), check_superko=board.check_superko)
        copy_board(dst=b, src=board)
        return b

    # depth-first from the root, one board per level on the way down
    stack = [(0, fresh(), root_color)]
    seen = 0
    while stack:
        i, b, side = stack.pop()
        seen += 1
        lo = int(first[i])
        for k in range(int(nc[i])):
            move = int(action[lo + k])
            if move != PASS and not b.is_legal(move, side):
                raise ValueError(f"node {i}, child {k}: action {move} is not legal for {_stone_to_str(side)} at the node's position")
            child = int(index[lo + k])
            if child != NOT_EXPANDED:
                if not i < child < n:
                    raise ValueError(f"node {i}, child {k}: child index {child}")
                nb = GoBoard(board_size=b.get_board_size(), komi=b.get_komi(), check_superko=b.check_superko)
                copy_board(dst=nb, src=b)
                nb.put_stone(move, side)
                stack.append((child, nb, Stone.get_opponent_color(side)))
    if seen != n:
        raise ValueError(f"{n - seen} nodes of the tree are not reachable from the root")
