"""Search checkpoints: SearchEngine.snapshot()'s list of per-tree snapshots in one .npz file, arrays only (no
pickled objects), and back for SearchEngine.restore().

A snapshot holds what a continuation of the tree needs: the packed tree, the root position (cells, scalars, hash history), the
random stream's state, the root noise row and the halt word.  It does not hold an evaluation cache, visit budgets or the
live-rank table: the engine that restores sets those up as it would for a search of its own."""
import numpy as np

_ROOT_KEYS = ("moves", "ko_pos", "ko_move", "prev", "prevprev", "to_move", "num_nodes", "hist_len")
_TREE_SCALARS = ("num_nodes", "current_root", "err", "to_move", "total_children")


def save(path, snapshots) -> None:
    arrays = {"count": np.array([len(snapshots)], dtype=np.int64)}
    for j, snap in enumerate(snapshots):
        pre = f"t{j}_"
        tree = snap["tree"]
        arrays[pre + "tree_scalars"] = np.array([int(tree[k]) for k in _TREE_SCALARS], dtype=np.int64)
        for key, value in tree.items():
            if key not in _TREE_SCALARS:
                arrays[pre + "tree_" + key] = np.asarray(value)
        arrays[pre + "cells"] = np.asarray(snap["cells"], dtype=np.uint8)
        arrays[pre + "root"] = np.array([int(snap["root"][k]) for k in _ROOT_KEYS], dtype=np.int64)
        arrays[pre + "hash"] = np.array([int(snap["root"]["hash"])], dtype=np.uint64)
        arrays[pre + "history"] = np.asarray(snap["history"], dtype=np.uint64)
        seeded = snap["stream_key"] is not None
        arrays[pre + "stream_key"] = np.asarray(snap["stream_key"], dtype=np.uint32) if seeded else np.zeros(0, dtype=np.uint32)
        arrays[pre + "stream_pos"] = np.array([int(snap["stream_pos"]) if seeded else -1], dtype=np.int64)
        arrays[pre + "noise"] = np.asarray(snap["noise"], dtype=np.float64)
        arrays[pre + "halt"] = np.array([int(snap["halt"])], dtype=np.int64)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load(path):
    out = []
    with np.load(path, allow_pickle=False) as data:
        for j in range(int(data["count"][0])):
            pre = f"t{j}_"
            tree = {k: int(v) for k, v in zip(_TREE_SCALARS, data[pre + "tree_scalars"])}
            for name in data.files:
                if name.startswith(pre + "tree_") and name != pre + "tree_scalars":
                    tree[name[len(pre) + 5:]] = data[name].copy()
            root = {k: int(v) for k, v in zip(_ROOT_KEYS, data[pre + "root"])}
            root["hash"] = int(data[pre + "hash"][0])
            key = data[pre + "stream_key"].copy()
            out.append({"tree": tree, "cells": data[pre + "cells"].copy(), "root": root, "history": data[pre + "history"].copy(),
                        "stream_key": key if key.size else None, "stream_pos": int(data[pre + "stream_pos"][0]),
                        "noise": data[pre + "noise"].copy(), "halt": int(data[pre + "halt"][0])})
    return out
