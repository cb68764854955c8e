"""What tree reuse (MCTSTree(reuse_tree=True), tg_search_reroot) must compute, restated on the oracle side: the subtree
under the new root, compacted in creation order, and the search that continues it.  Shared by
tests/test_tree_reuse_host.py (CPU) and tests/test_gpu_tree_reuse.py (GPU)."""
import numpy as np


def subtree_nodes(children, num_children, root):
    """Sorted node indices of the subtree under `root`; children[i] / num_children[i] as the pool holds them."""
    seen, stack = [], [int(root)]
    while stack:
        node = stack.pop()
        seen.append(node)
        for c in children[node][:num_children[node]]:
            if c >= 0:
                stack.append(int(c))
    return sorted(seen)


def compact_arrays(nodes, root):
    """numpy compaction of a read-back pool.  `nodes`: dict of per-node arrays over the tree's num_nodes nodes -
    'children_index' [n][A] plus any other [n][...] field, 'parent' / 'pedge' [n], 'num_children' [n].  Returns the
    same dict for the compacted tree: rank order of the kept indices, child indices and parents remapped, the new
    root's parent / edge -1, every other field copied."""
    keep = subtree_nodes(nodes["children_index"], nodes["num_children"], root)
    remap = np.full(len(nodes["parent"]), -1, dtype=np.int64)
    remap[keep] = np.arange(len(keep))
    out = {k: np.asarray(v)[keep].copy() for k, v in nodes.items()}
    ci = out["children_index"]
    out["children_index"] = np.where(ci >= 0, remap[np.maximum(ci, 0)], -1).astype(ci.dtype)
    parent = out["parent"]
    out["parent"] = np.where(parent >= 0, remap[np.maximum(parent, 0)], -1).astype(parent.dtype)
    out["parent"][0] = -1
    out["pedge"][0] = -1
    return out


def compact_oracle_tree(otree, root):
    """The oracle tree's subtree under node `root` becomes the whole tree (new root = node 0, creation order kept)."""
    from oracle.node import Node
    children = [n.children_index for n in otree.node[:otree.num_nodes]]
    counts = [n.num_children for n in otree.node[:otree.num_nodes]]
    keep = subtree_nodes(children, counts, root)
    remap = {old: new for new, old in enumerate(keep)}
    kept = [otree.node[i] for i in keep]
    for node in kept:
        ci = node.children_index
        for e in range(node.num_children):
            if ci[e] >= 0:
                ci[e] = remap[int(ci[e])]
    otree.node = kept + [Node(otree.num_actions) for _ in range(len(otree.node) - len(kept))]
    otree.num_nodes = len(kept)
    otree.current_root = 0


def oracle_child(otree, node, move):
    """Expanded child of `node` reached by `move`, -1 if none."""
    nd = otree.node[node]
    for i in range(nd.num_children):
        if nd.action[i] == move:
            return int(nd.children_index[i])
    return -1


def emulate_search(otree, board, color, time_manager, reuse_root=None):
    """oracle search_best_move (mcts/tree.py:57-105) with tree reuse: with `reuse_root` the subtree under that node is
    compacted and the root is neither expanded nor evaluated again (no random draws); then max(0, threshold - root
    visits) descents with the reference's per-descent early-stop test against the TOTAL threshold, and the flush."""
    from oracle.tree import PASS, RESIGN, RESIGN_THRESHOLD
    if reuse_root is None:
        otree._initialize_search(board, color)
    else:
        compact_oracle_tree(otree, reuse_root)
    time_manager.start_timer()
    root = otree.node[0]
    if root.num_children == 1:
        return PASS
    threshold = time_manager.get_num_visits_threshold(color)
    search_board = board.clone()
    for _ in range(max(0, threshold - root.node_visits)):
        search_board.copy_from(board)
        otree.search_mcts(search_board, color, 0, [])
        if time_manager.is_time_over() or time_manager.is_move_decided(root, threshold):
            break
    if len(otree.batch_queue.node_index) > 0:
        otree.process_mini_batch(board)
    best = root.best_move_index()
    if root.value_evaluation(best) < RESIGN_THRESHOLD:
        return RESIGN
    return root.action[best]
