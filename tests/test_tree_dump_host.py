"""The whole-tree read-out on the CPU: csrc/tree_dump.h - the packed record's layout, the scan that places each
node's children (the carry between chunks included) and the digest rule, the very text the kernels compile - built alone into
tests/tree_dump_driver.cpp with the host compiler and held to numpy.cumsum, to Python restatements of the layout and to
tamago_amd/mcts/dump.py's digest_of; the proof that the corpus tells the right rules from four wrong ones; the driver once more
under the address and undefined-behaviour sanitizers.  No GPU."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tamago_amd.mcts import dump

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tamago_amd", "csrc")
NODE_REC = np.dtype([("visits", "<i4"), ("vl", "<i4"), ("vsum", "<f4"), ("raw", "<f4"), ("children", "<i4"), ("parent", "<i4"),
                     ("pedge", "<i4"), ("pad", "<i4")])
# element types of the POOL (csrc/node_pool.h), by member
POOL_TYPES = {"ch_index": np.int32, "ch_visits": np.int32, "ch_vl": np.int32, "ch_vsum": np.float64, "ch_policy": np.float64,
              "ch_value": np.float64, "action": np.int16}


def _compiler():
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    return cxx


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "driver")
    subprocess.check_call([_compiler(), "-std=c++17"] + flags + [os.path.join(HERE, "tree_dump_driver.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "tree_dump", ["-O1"])


def chunk_size():
    return int(re.search(r"constexpr int kChunk = (\d+);", open(os.path.join(CSRC, "tree_dump.h")).read()).group(1))


# ---- the layout -----------------------------------------------------------------------------------------------------------
def test_the_python_restatement_names_the_headers_arrays(driver):
    """dump.py restates what the header expands from TG_NODE_POOL_CHILD_ARRAYS: the same arrays in the same order, the same
    element widths in a record (up to four bytes widened to int32), the same node record, head, seeds and field numbers."""
    layout = _run(driver, "layout")
    assert [(name, k) for name, _, k in layout["arrays"]] == [(member, k) for k, (_, member, _) in enumerate(dump.CHILD_ARRAYS)]
    for (name, size, _), (_, _, dtype) in zip(layout["arrays"], dump.CHILD_ARRAYS):
        assert size == np.dtype(POOL_TYPES[name]).itemsize and np.dtype(dtype).itemsize == (8 if size == 8 else 4)
    assert layout["head_words"] == dump.HEAD_WORDS and layout["node_bytes"] == dump.NODE_DTYPE.itemsize
    assert [int(s, 16) for s in layout["seeds"]] == list(dump.SEEDS)
    assert layout["field_arrays"] == dump.FIELD_ARRAYS and layout["chunk"] == chunk_size()


@pytest.mark.parametrize("A", [82, 170, 362])
def test_record_offsets_against_the_restatement(driver, A):
    """Trees of 0, 1, 3 and 2 500 nodes whose nodes have up to A children: an odd total leaves the 4-byte rows off an 8-byte
    boundary, which the 8-byte rows make up for."""
    rnd = np.random.RandomState(A)
    for n in (0, 1, 3, 2500):
        for total in sorted({0, n, n * A, int(rnd.randint(0, A + 1, n).sum()) | 1 if n else 0}):
            got = _run(driver, "offsets", n, total)
            want = dump.row_offsets(n, total)
            assert got["nodes_end"] == dump.node_offset(n) == 32 + 40 * n
            assert got["rows"] == {member: want[key] for key, member, _ in dump.CHILD_ARRAYS}
            assert got["bytes"] == want["end"] == dump.record_bytes(n, total)
            assert all(want[key] % 8 == 0 for key, _, dtype in dump.CHILD_ARRAYS if np.dtype(dtype).itemsize == 8)
            assert want["end"] % 8 == 0 and want["end"] == ((32 + 40 * n + 16 * total + 7) & ~7) + 24 * total


# ---- the scan -------------------------------------------------------------------------------------------------------------
def scan_corpus():
    """Child counts of trees of 0 .. 2 chunks + 1 nodes: sizes at the wavefront and the chunk borders, counts of every size a
    board gives (1 .. 362) and all-zero / all-full rows."""
    chunk = chunk_size()
    out = []
    for n in (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 2 * chunk + 500):
        rnd = np.random.RandomState(n + 7)
        out.append(rnd.randint(0, 363, n).astype(np.int32))
        out.append(np.full(n, 362, dtype=np.int32))
        out.append(np.ones(n, dtype=np.int32))
    return out


def run_scan(exe, tmp_path, counts):
    path = tmp_path / "counts.bin"
    path.write_bytes(np.int32(len(counts)).tobytes() + counts.astype("<i4").tobytes())
    return _run(exe, "scan", path)


def test_the_scan_against_cumsum(driver, tmp_path):
    for counts in scan_corpus():
        got = run_scan(driver, tmp_path, counts)["right"]
        inclusive = np.cumsum(counts.astype(np.int64))
        assert got["total"] == int(counts.sum(dtype=np.int64))
        assert np.array_equal(np.array(got["first"], dtype=np.int64), inclusive - counts)


def test_the_corpus_tells_the_scan_from_two_wrong_ones(driver, tmp_path):
    """An inclusive scan starts every node with children one node late; a carry dropped between chunks restarts the offsets at
    the second chunk, so only trees beyond one chunk can show it."""
    chunk = chunk_size()
    wrong = {"inclusive": set(), "dropped_carry": set()}
    for counts in scan_corpus():
        got = run_scan(driver, tmp_path, counts)
        want = (np.cumsum(counts.astype(np.int64)) - counts).tolist()
        for rule in wrong:
            if got[rule]["first"] != want:                    # (the offsets: a dropped carry loses the total of any tree)
                wrong[rule].add(len(counts))
    assert {1, 65, chunk + 1} <= wrong["inclusive"]
    assert wrong["dropped_carry"] and min(wrong["dropped_carry"]) > chunk
    assert {chunk + 1, 2 * chunk + 1} <= wrong["dropped_carry"]


# ---- trees ----------------------------------------------------------------------------------------------------------------
def random_tree(rnd, A, n, stale=True):
    """A pool of n nodes ([n][A] per child array, the tail beyond `children` holding stale values) with special floats among
    the entries: -0.0, infinities, denormals."""
    children = rnd.randint(0, A + 1, n).astype(np.int32)
    if n:
        children[0] = A                                       # a full row: ceil(A / 64) lane passes
        children[-1] = 0
    node = np.zeros(n, dtype=NODE_REC)
    node["visits"] = rnd.randint(0, 1 << 20, n)
    node["vl"] = rnd.randint(0, 8, n)
    node["vsum"] = rnd.standard_normal(n).astype(np.float32)
    node["raw"] = rnd.random_sample(n).astype(np.float32)
    node["children"] = children
    node["parent"] = rnd.randint(-1, max(n, 1), n)
    node["pedge"] = rnd.randint(-1, A, n)
    arrays = {}
    for _, member, _ in dump.CHILD_ARRAYS:
        dtype = POOL_TYPES[member]
        if np.dtype(dtype).kind == "f":
            a = rnd.standard_normal((n, A))
            special = rnd.random_sample((n, A))
            a[special < 0.05] = -0.0
            a[(special >= 0.05) & (special < 0.1)] = 0.0
            a[(special >= 0.1) & (special < 0.12)] = np.inf
            a[(special >= 0.12) & (special < 0.14)] = 5e-324
        else:
            a = rnd.randint(-1, 400, (n, A))
        a = a.astype(dtype)
        if not stale:
            a[np.arange(A)[None, :] >= children[:, None]] = 0
        arrays[member] = a
    return {"A": A, "num_nodes": n, "current_root": 0, "err": 0, "to_move": 1 + n % 2, "node": node, "arrays": arrays}


def tree_file(tmp_path, tree, name="tree.bin"):
    head = np.array([tree["A"], tree["num_nodes"], tree["current_root"], tree["err"], tree["to_move"], 0, 0, 0], dtype="<i4")
    data = head.tobytes() + tree["node"].tobytes()
    for _, member, _ in dump.CHILD_ARRAYS:
        data += np.ascontiguousarray(tree["arrays"][member]).tobytes()
    path = tmp_path / name
    path.write_bytes(data)
    return path


def run_tree(exe, tmp_path, tree):
    record = tmp_path / "record.bin"
    out = _run(exe, "tree", tree_file(tmp_path, tree), record)
    out["record"] = np.frombuffer(record.read_bytes(), dtype=np.uint8)
    for rule in ("right", "no_child_index", "stale_tail"):
        out[rule] = [int(w, 16) for w in out[rule]]
    return out


class PoolNode:
    """MCTSNode attributes of node i of a random pool."""

    def __init__(self, tree, i):
        rec = tree["node"][i]
        self.num_children, self.node_visits, self.virtual_loss = int(rec["children"]), int(rec["visits"]), int(rec["vl"])
        self.node_value_sum, self.raw_value = rec["vsum"], rec["raw"]
        for key, member, _ in dump.CHILD_ARRAYS:
            setattr(self, key, tree["arrays"][member][i])


def packed_of(tree):
    return dump.pack_nodes([PoolNode(tree, i) for i in range(tree["num_nodes"])], tree["num_nodes"], tree["current_root"],
                           tree["to_move"])


def tree_corpus():
    chunk = chunk_size()
    return [random_tree(np.random.RandomState(100 * A + n), A, n) for A, n in
            ((82, 0), (82, 1), (82, 3), (82, 200), (170, 70), (362, 40), (82, 2 * chunk + 52))]


def test_the_record_parses_to_the_pool(driver, tmp_path):
    """The packed record of the header's host replay, read by dump.parse_record - the reader of the device's records: every
    scalar and every entry below `children` of the pool, nothing of the stale tails."""
    for tree in tree_corpus():
        out = run_tree(driver, tmp_path, tree)
        got, want = dump.parse_record(out["record"]), packed_of(tree)
        assert out["record_bytes"] == dump.record_bytes(want["num_nodes"], want["total_children"]) == out["record"].size
        assert (got["num_nodes"], got["current_root"], got["err"], got["to_move"], got["total_children"]) == \
            (want["num_nodes"], 0, 0, tree["to_move"], want["total_children"])
        for key in ("node_visits", "virtual_loss", "num_children", "first_child") + tuple(k for k, _, _ in dump.CHILD_ARRAYS):
            assert np.array_equal(got[key], want[key]), key
        for key in ("node_value_sum", "raw_value"):
            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
        assert np.array_equal(got["parent"], tree["node"]["parent"]) and np.array_equal(got["pedge"], tree["node"]["pedge"])


def test_the_digest_against_digest_of(driver, tmp_path):
    """The header's digest of random pools equals dump.digest_of of their tree dicts and dump.digest_of_packed of the parsed
    records; distinct trees have distinct digests."""
    seen = set()
    for tree in tree_corpus():
        out = run_tree(driver, tmp_path, tree)
        packed = dump.parse_record(out["record"])
        tree_dict = dump.tree_to_dict(packed, tree["A"], 1, False)
        assert out["right"] == dump.digest_of_packed(packed).tolist() == dump.digest_of(tree_dict).tolist()
        seen.add(tuple(out["right"]))
    assert len(seen) == len(tree_corpus())


def test_values_enter_the_digest_by_their_bits(driver, tmp_path):
    """-0.0 for 0.0 in one used entry, and in one node's value sum, changes both words; so does one more visit."""
    tree = random_tree(np.random.RandomState(5), 82, 12, stale=False)
    tree["arrays"]["ch_vsum"][3, 0] = 0.0
    tree["node"]["vsum"][4] = 0.0
    tree["node"]["children"][3] = max(int(tree["node"]["children"][3]), 1)
    base = run_tree(driver, tmp_path, tree)["right"]
    for change in ("entry", "scalar", "visit"):
        other = {**tree, "node": tree["node"].copy(), "arrays": {k: v.copy() for k, v in tree["arrays"].items()}}
        if change == "entry":
            other["arrays"]["ch_vsum"][3, 0] = -0.0
        elif change == "scalar":
            other["node"]["vsum"][4] = -0.0
        else:
            other["node"]["visits"][7] += 1
        got = run_tree(driver, tmp_path, other)["right"]
        assert got[0] != base[0] and got[1] != base[1], change
        assert got == dump.digest_of_packed(packed_of(other)).tolist()


def test_the_corpus_tells_the_digest_from_two_wrong_ones(driver, tmp_path):
    """A term without the child index does not see two children of a node swap their values; a digest that reads the whole
    pool row changes with the stale tail.  The right rule sees the first and not the second."""
    tree = random_tree(np.random.RandomState(11), 82, 30)
    tree["node"]["children"][5] = 40
    tree["arrays"]["ch_visits"][5, 2], tree["arrays"]["ch_visits"][5, 9] = 17, 3
    base = run_tree(driver, tmp_path, tree)
    swapped = {**tree, "arrays": {k: v.copy() for k, v in tree["arrays"].items()}}
    swapped["arrays"]["ch_visits"][5, 2], swapped["arrays"]["ch_visits"][5, 9] = 3, 17
    out = run_tree(driver, tmp_path, swapped)
    assert out["no_child_index"] == base["no_child_index"]                # the wrong rule: unseen
    assert out["right"][0] != base["right"][0] and out["right"][1] != base["right"][1]
    stale = {**tree, "arrays": {k: v.copy() for k, v in tree["arrays"].items()}}
    stale["arrays"]["ch_policy"][5, 40:] += 1.0                            # beyond `children`: not the tree's
    out = run_tree(driver, tmp_path, stale)
    assert out["stale_tail"] != base["stale_tail"]                        # the wrong rule: the tail is read
    assert out["right"] == base["right"] and np.array_equal(out["record"], base["record"])


# ---- sanitizers -----------------------------------------------------------------------------------------------------------
def test_the_driver_under_sanitizers(tmp_path_factory, tmp_path):
    """The driver as a stand-alone program with -fsanitize=address,undefined: the layout, scans at the chunk borders, and the
    pack and digest replays of an empty tree, a one-node tree, a full 362-child row and a tree beyond two chunks."""
    cxx = _compiler()
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path_factory.mktemp("san") / "t")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    assert probe.returncode == 0, "the host compiler cannot link -fsanitize=address,undefined: " + probe.stderr[-500:]
    san = _build(tmp_path_factory, "tree_dump_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _run(san, "layout")
    _run(san, "offsets", 2500, 12345)
    chunk = chunk_size()
    for counts in scan_corpus():
        if len(counts) in (0, 1, 65, chunk + 1, 2 * chunk + 1):
            got = run_scan(san, tmp_path, counts)["right"]
            assert got["total"] == int(counts.sum(dtype=np.int64))
    for A, n in ((82, 0), (82, 1), (362, 5), (82, 2 * chunk + 52)):
        tree = random_tree(np.random.RandomState(A + n), A, n)
        out = run_tree(san, tmp_path, tree)
        assert out["right"] == dump.digest_of_packed(packed_of(tree)).tolist()
