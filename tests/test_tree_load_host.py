"""The whole-tree write-in on the CPU: csrc/tree_load.h - which packed records may enter a pool and how a record
becomes pool rows, the very text the library compiles - built alone into tests/tree_load_driver.cpp with the host compiler and
held to tamago_amd/mcts/dump.py (make_record, parse_record, digest_of_packed); one record per rule that breaks only that rule;
the proof that the corpus tells the right fill rule from two wrong ones; the C entry point tg_search_check_records; the JSON
reader on the reference's own text; the host verify; the driver once more under the address and undefined-behaviour
sanitizers.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from tamago_amd.mcts import dump
from tests import _tree_dump_cases as cases
from tests.test_tree_dump_host import _compiler, _run, packed_of, random_tree, tree_file

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "driver")
    subprocess.check_call([_compiler(), "-std=c++17"] + flags + [os.path.join(HERE, "tree_load_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "tree_load", ["-O1"])


@pytest.fixture(scope="module")
def rules(driver):
    return _run(driver, "rules")


def board_of(A):
    return {82: 9, 170: 13, 362: 19}[A]


def on_board_points(S):
    W = S + 2
    return np.array([y * W + x for y in range(1, S + 1) for x in range(1, S + 1)], dtype=np.int32)


def admissible_tree(rnd, A, n):
    """test_tree_dump_host.random_tree's pool (stale tails included) made admissible: every node has a child, the child
    indices form a tree in creation order with parent / pedge to match, actions are the pass or on-board points, counts are
    not negative.  Floats keep their special values."""
    tree = random_tree(rnd, A, n)
    node, arrays = tree["node"], tree["arrays"]
    node["children"] = np.maximum(node["children"], 1)
    if n > 2:
        node["children"][n // 2] = A - 1 if A % 64 else A - 3       # (a row whose last lane pass is partly tail)
    children = node["children"]
    points = np.concatenate([[0], on_board_points(board_of(A))])
    arrays["action"][:] = points[rnd.randint(0, points.size, (n, A))].astype(np.int16)
    arrays["ch_visits"][:] = np.abs(arrays["ch_visits"])
    arrays["ch_vl"][:] = np.abs(arrays["ch_vl"])
    used = np.arange(A)[None, :] < children[:, None]
    arrays["ch_index"][used] = -1                                    # (the tails stay stale)
    node["parent"][:], node["pedge"][:] = -1, -1
    free = {0: list(rnd.permutation(int(children[0])))} if n else {}
    for i in range(1, n):
        p = int(rnd.choice(sorted(free)))
        e = int(free[p].pop())
        if not free[p]:
            del free[p]
        arrays["ch_index"][p, e] = i
        node["parent"][i], node["pedge"][i] = p, e
        free[i] = list(rnd.permutation(int(children[i])))
    tree["to_move"] = 1 + n % 2
    return tree


CORPUS = ((82, 0), (82, 1), (82, 2), (82, 65), (82, 1025), (170, 2), (170, 65), (362, 1), (362, 65), (362, 200))


def corpus():
    return [admissible_tree(np.random.RandomState(1000 * A + n), A, n) for A, n in CORPUS]


def packed(tree):
    p = packed_of(tree)
    p["parent"], p["pedge"] = tree["node"]["parent"].copy(), tree["node"]["pedge"].copy()
    return p


def roundtrip(exe, tmp_path, tree):
    record = tmp_path / "record.bin"
    out = _run(exe, "roundtrip", tree_file(tmp_path, tree), board_of(tree["A"]) + 2, record)
    out["record"] = np.frombuffer(record.read_bytes(), dtype=np.uint8)
    return out


def check(exe, tmp_path, record, A, N):
    path = tmp_path / "check.bin"
    path.write_bytes(np.asarray(record, dtype=np.uint8).tobytes())
    return _run(exe, "check", path, A, board_of(A) + 2, N)


# ---- round trips ----------------------------------------------------------------------------------------------------------
def test_round_trips_over_the_corpus(driver, tmp_path):
    """make_record(packed) is the bytes of the header's pack_replay; parse_record inverts make_record; pack_replay inverts
    unpack_replay; the digest of the unpacked pool is digest_of_packed of the parsed record.  Every record the corpus packs is
    accepted, and refused by a pool one node smaller."""
    for tree in corpus():
        out = roundtrip(driver, tmp_path, tree)
        want = packed(tree)
        mine = dump.make_record(want)
        assert out["record_bytes"] == mine.size and np.array_equal(mine, out["record"])
        back = dump.parse_record(mine)
        assert set(back) == set(want)
        for key, value in want.items():
            if isinstance(value, np.ndarray):
                assert back[key].dtype == value.dtype and np.array_equal(back[key].view(np.uint8), value.view(np.uint8)), key
            else:
                assert back[key] == value, key
        assert out["check"] == {"rule": 0, "node": -1, "child": -1}
        assert out["repacked_equal"] is True
        assert out["tree_words"] == [tree["num_nodes"], 0, 0, tree["to_move"]]
        assert [int(w, 16) for w in out["unpacked_digest"]] == [int(w, 16) for w in out["digest"]] == \
            dump.digest_of_packed(dump.parse_record(out["record"])).tolist()
        if tree["num_nodes"]:
            assert out["too_small"]["rule"] != 0


def test_link_parents_finds_the_edges():
    for tree in corpus():
        p = packed_of(tree)                                           # (pack_nodes: parents -1)
        dump.link_parents(p)
        assert np.array_equal(p["parent"], tree["node"]["parent"]) and np.array_equal(p["pedge"], tree["node"]["pedge"])


# ---- tails ----------------------------------------------------------------------------------------------------------------
def test_the_corpus_tells_the_fill_rule_from_two_wrong_ones(driver, tmp_path):
    """Unpacked over a stale pool, every tail is canonical (children_index -1, everything else +0).  A rule that takes whole
    lane passes from the record puts other entries beyond `children` wherever a node's count is no multiple of 64 and below
    A; a rule that leaves the tail as it was keeps the stale pool wherever a node has fewer than A children."""
    shown = {"whole_passes": 0, "kept_tail": 0}
    for tree in corpus():
        out = roundtrip(driver, tmp_path, tree)
        assert out["right"]["tails_canonical"] is True
        c, A = tree["node"]["children"], tree["A"]
        can_show = {"whole_passes": bool(np.any((c % 64 != 0) & (c < A))), "kept_tail": bool(np.any(c < A))}
        for rule, can in can_show.items():
            assert out[rule]["same_as_right"] is (not can), (rule, tree["A"], tree["num_nodes"])
            assert out[rule]["tails_canonical"] is (not can)
            shown[rule] += can
    assert shown["whole_passes"] >= 6 and shown["kept_tail"] >= 6


# ---- refusals -------------------------------------------------------------------------------------------------------------
def record_views(rec):
    """Writable views of a record's head, nodes and rows."""
    head = rec[:dump.HEAD_WORDS * 4].view("<i4")
    n = int(head[0])
    total = int(np.uint32(head[4])) | (int(np.uint32(head[5])) << 32)
    at = dump.row_offsets(n, total)
    rows = {key: rec[at[key]:at[key] + total * np.dtype(dtype).itemsize].view(np.dtype(dtype)) for key, _, dtype in dump.CHILD_ARRAYS}
    return head, rec[dump.node_offset(0):dump.node_offset(n)].view(dump.NODE_DTYPE), rows


def corruptions(tree):
    """(name, rule, node, child, corrupted record) - each record breaks the named rule and no rule checked before it."""
    A, n = tree["A"], tree["num_nodes"]
    base = dump.make_record(packed(tree))
    W = board_of(A) + 2
    _, nodes0, rows0 = record_views(base.copy())
    first = nodes0["first_child"]
    # an expanded edge (p, e) -> c of a node p >= 1 (p - 1 is a node), and a free slot of another node in front of c
    index = rows0["children_index"]
    owner = np.repeat(np.arange(n), nodes0["num_children"])
    slot = np.arange(index.size) - np.repeat(first, nodes0["num_children"])
    edges = np.flatnonzero((index >= 2) & (owner >= 1))
    at_edge = int(edges[0])
    p, e, c = int(owner[at_edge]), int(slot[at_edge]), int(index[at_edge])
    free_at = int(np.flatnonzero((index == -1) & (owner < c) & (owner != p))[0])
    out = []

    def case(name, rule, node, child, change):
        rec = base.copy()
        res = change(rec, *record_views(rec))
        out.append((name, rule, node, child, rec if res is None else res))

    def set_total(delta):
        def change(rec, head, nodes, rows):
            head[4] += delta
        return change

    case("length + 8", "length", -1, -1, lambda rec, h, nd, r: np.concatenate([rec, np.zeros(8, dtype=np.uint8)]))
    case("length - 8", "length", -1, -1, lambda rec, h, nd, r: rec[:-8].copy())
    case("total + 1", "total", -1, -1, set_total(1))
    case("total - 1", "total", -1, -1, set_total(-1))

    def children(i, v):
        def change(rec, head, nodes, rows):
            nodes["num_children"][i] = v
        return change
    case("children 0", "children", 3, -1, children(3, 0))
    case("children A + 1", "children", 3, -1, children(3, A + 1))

    def first_shift(rec, head, nodes, rows):
        nodes["first_child"][4] += 1
    case("first_child shifted", "first_child", 4, -1, first_shift)

    def child_index(v):
        def change(rec, head, nodes, rows):
            rows["children_index"][at_edge] = v
        return change
    case("child == parent", "child_index", p, e, child_index(p))
    case("child == parent - 1", "child_index", p, e, child_index(p - 1))
    case("child == num_nodes", "child_index", p, e, child_index(n))

    def two_edges(rec, head, nodes, rows):
        rows["children_index"][free_at] = c
    # (whichever of the two edges comes first in the walk names the node; the second is the violation)
    case("named by two edges", "edges", c, -1, two_edges)
    case("named by none", "edges", c, -1, child_index(-1))

    def parent_elsewhere(rec, head, nodes, rows):
        nodes["parent"][c] = p + 1 if p + 1 < c else p - 1
    case("parent elsewhere", "parent", c, -1, parent_elsewhere)

    def pedge_elsewhere(rec, head, nodes, rows):
        nodes["pedge"][c] = e + 1
    case("pedge elsewhere", "parent", c, -1, pedge_elsewhere)

    def root_parent(rec, head, nodes, rows):
        nodes["parent"][0] = 0
    case("root with a parent", "root", 0, -1, root_parent)

    def action(v):
        def change(rec, head, nodes, rows):
            rows["action"][int(first[2]) + 1 if nodes0["num_children"][2] > 1 else int(first[2])] = v
        return change
    k2 = 1 if nodes0["num_children"][2] > 1 else 0
    case("action on the border", "action", 2, k2, action(W + 0))
    case("action on the far border", "action", 2, k2, action(2 * W - 1))
    case("action at NC", "action", 2, k2, action(W * W))
    case("action negative", "action", 2, k2, action(-5))

    def neg(field, where):
        def change(rec, head, nodes, rows):
            (nodes if where == "node" else rows)[field][5 if where == "node" else int(first[5])] = -1
        return change
    case("negative node visits", "node_count", 5, -1, neg("node_visits", "node"))
    case("negative node virtual loss", "node_count", 5, -1, neg("virtual_loss", "node"))
    case("negative child visits", "child_count", 5, 0, neg("children_visits", "row"))
    case("negative child virtual loss", "child_count", 5, 0, neg("children_virtual_loss", "row"))

    def node_pad(rec, head, nodes, rows):
        nodes["pad"][6] = 1
    case("node pad", "node_pad", 6, -1, node_pad)

    def head_word(w, v):
        def change(rec, head, nodes, rows):
            head[w] = v
        return change
    case("head pad 0", "head_pad", -1, -1, head_word(6, 1))
    case("head pad 1", "head_pad", -1, -1, head_word(7, -1))
    case("current_root 1", "current_root", -1, -1, head_word(1, 1))
    case("error word", "err_word", -1, -1, head_word(2, 4))
    case("to_move 0", "to_move", -1, -1, head_word(3, 0))
    case("to_move 3", "to_move", -1, -1, head_word(3, 3))
    case("num_nodes negative", "num_nodes", -1, -1, head_word(0, -1))
    return base, out


@pytest.fixture(scope="module")
def refusal_cases():
    tree = admissible_tree(np.random.RandomState(77), 82, 40)
    base, cases_ = corruptions(tree)
    return tree, base, cases_


def test_every_rule_has_a_record_that_breaks_only_it(driver, rules, refusal_cases, tmp_path):
    tree, base, cases_ = refusal_cases
    A, n = tree["A"], tree["num_nodes"]
    assert check(driver, tmp_path, base, A, n) == {"rule": 0, "node": -1, "child": -1}
    assert check(driver, tmp_path, base, A, n - 1)["rule"] == rules["num_nodes"]            # num_nodes > tree_size
    assert check(driver, tmp_path, base[:16], A, n)["rule"] == rules["length"]              # shorter than the head
    seen = set()
    for name, rule, node, child, rec in cases_:
        got = check(driver, tmp_path, rec, A, n)
        assert got == {"rule": rules[rule], "node": node, "child": child}, (name, got)
        seen.add(rule)
    assert seen | {"ok", "rules"} == set(rules)                       # every rule of the header has its record
    # an empty record may carry any side to move
    empty = dump.make_record(packed(admissible_tree(np.random.RandomState(1), 82, 0)))
    empty[:32].view("<i4")[3] = 0
    assert check(driver, tmp_path, empty, A, n)["rule"] == 0


def test_the_c_entry_point_gives_the_same_verdicts(refusal_cases):
    """tg_search_check_records through the library, without a handle or a GPU: every record of the corpus passes, every
    corrupted record is TG_ERR_ARG with the rule's number, the list entry, the node and the child in tg_last_error."""
    from tamago_amd import build, lib as tl
    build.build(verbose=False)
    lib = tl.load()
    tree, base, cases_ = refusal_cases
    text = open(os.path.join(os.path.dirname(HERE), "tamago_amd", "csrc", "tree_load.h")).read()
    names = text.split("enum Rule : int {")[1].split("}")[0].replace("\n", " ").split(",")
    number = {name.strip(): k for k, name in enumerate(names)}

    def call(records, size, tree_size):
        blob = np.concatenate(records)
        offsets = np.zeros(len(records) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([r.size for r in records])
        rc = lib.tg_search_check_records(size, tree_size, blob.ctypes.data, offsets.ctypes.data, len(records))
        return rc, lib.tg_last_error().decode()

    for t in corpus():
        rec = dump.make_record(packed(t))
        assert call([rec, rec], board_of(t["A"]), max(t["num_nodes"], 1))[0] == 0
    camel = {"length": "kLength", "total": "kTotal", "children": "kChildren", "first_child": "kFirstChild", "child_index": "kChildIndex",
             "edges": "kEdges", "parent": "kParent", "root": "kRoot", "action": "kAction", "node_count": "kNodeCount",
             "child_count": "kChildCount", "node_pad": "kNodePad", "head_pad": "kHeadPad", "current_root": "kCurrentRoot",
             "err_word": "kErrWord", "to_move": "kToMove", "num_nodes": "kNumNodes"}
    for name, rule, node, child, rec in cases_:
        rc, msg = call([base, rec, base], 9, tree["num_nodes"])
        assert rc == -1 and f"list entry 1: rule {number[camel[rule]]}, node {node}, child {child}:" in msg, (name, msg)
    rc, msg = call([base], 9, tree["num_nodes"] - 1)
    assert rc == -1 and f"rule {number['kNumNodes']}," in msg
    assert call([base], 11, 64)[0] == -1 and lib.tg_search_check_records(9, 64, None, None, 1) == -1


# ---- JSON -----------------------------------------------------------------------------------------------------------------
def small_text():
    return cases.fixture(9)["small"]["json"]


def test_the_references_text_reads_back():
    """load_mcts_from_json of the reference's own dump: the tree dict is the parsed text's, the board carries the text's
    history, komi and superko, and dump_mcts_to_json of the two is the text again."""
    text = small_text()
    state = json.loads(text)
    tree, board, superko = dump.load_mcts_from_json(text)
    assert tree == state["tree"] and superko is True and board.check_superko
    assert board.get_komi() == state["komi"] and board.get_board_size() == state["board_size"]
    assert [[dump._stone_to_str(c), int(p)] for c, p, _ in board.get_move_history()] == state["move_history"]
    assert dump.dump_mcts_to_json(tree, board, superko) == text
    want = cases.product_board(9, cases.small_case()["ply"], True)
    assert np.array_equal(np.asarray(board.cells), np.asarray(want.cells)) and int(board.hash) == int(want.hash)
    # the dict -> packed -> record -> packed -> dict round trip, and the record is admissible
    p = dump.packed_of_dict(tree)
    rec = dump.make_record(p)
    again = dump.tree_to_dict(dump.parse_record(rec), 82, tree["batch_size"], tree["cgos_mode"])
    assert again == tree
    assert dump.digest_of_packed(p).tolist() == dump.digest_of(tree).tolist()
    with pytest.raises(ValueError):
        dump.load_mcts_from_json(text.replace('"dump_version": 2', '"dump_version": 1'))
    with pytest.raises(ValueError):
        dump.load_mcts_from_json(text[:len(text) // 2])


def test_host_verify():
    """verify_tree accepts the reference's tree on its position and refuses it once one action is an occupied point."""
    tree, board, _ = dump.load_mcts_from_json(small_text())
    p = dump.packed_of_dict(tree)
    dump.verify_tree(p, board, 1)
    occupied = int(json.loads(small_text())["move_history"][0][1])
    assert int(np.asarray(board.cells)[occupied]) in (1, 2)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    bad["action"][3] = occupied
    with pytest.raises(ValueError, match="node 0, child 3"):
        dump.verify_tree(bad, board, 1)
    deep = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    last = int(p["num_nodes"]) - 1
    deep["action"][int(p["first_child"][last])] = occupied
    with pytest.raises(ValueError, match=f"node {last}, child 0"):
        dump.verify_tree(deep, board, 1)


def test_checkpoint_files_hold_arrays_only(tmp_path):
    from tamago_amd.mcts import checkpoint
    tree, board, _ = dump.load_mcts_from_json(small_text())
    p = dump.packed_of_dict(tree)
    snap = {"tree": p, "cells": np.asarray(board.cells, dtype=np.uint8), "history": np.arange(12, dtype=np.uint64) << np.uint64(40),
            "root": {"moves": 13, "ko_pos": 0, "ko_move": 0, "prev": 59, "prevprev": 27, "to_move": 1, "num_nodes": 11, "hist_len": 12,
                     "hash": (1 << 63) + 5},
            "stream_key": np.arange(624, dtype=np.uint32), "stream_pos": 17, "noise": np.linspace(0, 1, 82), "halt": 1}
    unseeded = {**snap, "stream_key": None, "stream_pos": -1, "halt": 0}
    path = tmp_path / "search.npz"
    checkpoint.save(path, [snap, unseeded])
    with np.load(path, allow_pickle=False) as data:
        assert all(data[name].dtype != object for name in data.files)
    back = checkpoint.load(path)
    assert len(back) == 2 and back[1]["stream_key"] is None and back[0]["stream_pos"] == 17 and back[0]["halt"] == 1
    assert back[0]["root"] == snap["root"] and np.array_equal(back[0]["history"], snap["history"])
    assert np.array_equal(dump.make_record(back[0]["tree"]), dump.make_record(p))
    assert np.array_equal(back[0]["noise"], snap["noise"]) and np.array_equal(back[0]["stream_key"], snap["stream_key"])


# ---- sanitizers -----------------------------------------------------------------------------------------------------------
def test_the_driver_under_sanitizers(tmp_path_factory, tmp_path, rules, refusal_cases):
    """The driver as a stand-alone program with -fsanitize=address,undefined over the corpus and over every corrupted
    record: the check reads no byte beyond a record whatever its words say."""
    cxx = _compiler()
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path_factory.mktemp("san") / "t")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    assert probe.returncode == 0, "the host compiler cannot link -fsanitize=address,undefined: " + probe.stderr[-500:]
    san = _build(tmp_path_factory, "tree_load_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _run(san, "rules") == rules
    for tree in corpus():
        out = roundtrip(san, tmp_path, tree)
        assert out["check"]["rule"] == 0 and out["repacked_equal"] is True and out["right"]["tails_canonical"] is True
    tree, base, cases_ = refusal_cases
    for name, rule, node, child, rec in cases_:
        assert check(san, tmp_path, rec, tree["A"], tree["num_nodes"])["rule"] == rules[rule], name
    # words that promise more than the bytes hold: a huge total, a huge node count
    for word, value in ((4, 1 << 30), (5, 1), (0, 1 << 20)):
        rec = base.copy()
        rec[:32].view("<i4")[word] = value
        assert check(san, tmp_path, rec, tree["A"], 1 << 24)["rule"] != 0
