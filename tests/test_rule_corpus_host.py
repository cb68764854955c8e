"""CPU side of the board-rule corpus (tests/_rule_corpus.py): the corpus holds what it is meant to hold, the oracle board and
the host board agree with the reference-written fixture on it, the comparison code of tests/test_gpu_board_rules.py
passes on a correct stand-in and fails on five wrong ones, and the roots of the short searches are well chosen."""
import numpy as np
import pytest

import _rule_corpus as rc
from oracle.board import BLACK, GoBoard as OracleBoard, opponent


@pytest.mark.parametrize("size", rc.SIZES)
def test_corpus_is_the_fixture_and_meets_its_minimums(size):
    entries = rc.corpus(size)
    fx = rc.load_fixture(size)
    assert entries == fx.entries                                       # records, colours to move and names
    assert rc.tree_roots(size) == fx.tree_roots
    assert len(entries) <= rc.LIMITS[size]
    targets = sorted(int(fx.n_moves[i]) - rc.hmax(size) for i, e in enumerate(entries) if rc.is_history_entry(e))
    assert targets == sorted(rc.HISTORY_OFFSETS)
    assert all(len(e.moves) <= rc.PLAY_CAP_19 for e in entries if size == 19 and not rc.is_history_entry(e))
    counts = rc.coverage(entries)
    print(f"coverage at {size}x{size}: {dict(sorted(counts.items()))}")
    for key, least in rc.MINIMUMS.items():
        assert counts[key] >= least, (key, counts[key], least)
    # every crafted record shows what it was written for
    w = size + 2
    for spec in rc.CRAFTED:
        entry = next(e for e in entries if e.name == "crafted:" + spec["name"])
        board = rc.replay(entry)
        for kind, (x, y) in spec.get("expect", ()):
            assert kind in rc.point_categories(board, x + y * w, entry.to_move), (spec["name"], kind, x, y)
        if "expect_move" in spec:
            before = rc.Entry(size, entry.moves[:-1], rc.color_after(entry.moves[:-1]), "")
            assert spec["expect_move"] in rc.move_categories(rc.replay(before), entry.moves[-1], before.to_move), spec["name"]


@pytest.mark.parametrize("size", rc.SIZES)
def test_every_move_of_the_corpus_is_legal(size):
    """put_stone checks nothing, on the device as in the reference: the records must not rely on that.  (Ko and suicide; the
    fights were played under superko, which padding a record with passes does not change.)"""
    seen = set()
    for entry in rc.load_fixture(size).entries:
        board = OracleBoard(size, 7.0, False)
        color, key = BLACK, 0
        for pos in entry.moves:
            key = hash((key, pos))
            if pos and key not in seen:
                assert board.is_legal(pos, color), (entry.name, board.moves, pos)
            seen.add(key)
            board.put_stone(pos, color)
            color = opponent(color)


@pytest.mark.parametrize("size", rc.SIZES)
def test_oracle_board_equals_the_reference_on_the_corpus(size):
    fx = rc.load_fixture(size)
    for flag in (False, True):
        reader = rc.OracleReader(fx.entries, superko=flag)
        rc.check_roots(fx.entries, fx.cand[int(flag)], reader.root_actions())
    for i, entry in enumerate(fx.entries):
        board = rc.replay(entry)
        assert board.get_board_data() == [int(v) for v in fx.cells[i]], entry.name
        assert (board.ko_pos, board.ko_move, board.moves) == (fx.ko_pos[i], fx.ko_move[i], fx.n_moves[i]), entry.name


@pytest.mark.parametrize("size", rc.SIZES)
def test_host_board_equals_the_oracle_on_the_corpus(size):
    """tamago_amd.board.go_board.GoBoard is what SearchEngine.set_root reads: cells, ko scalars, hash and hash history of
    every entry, and the legal points with superko off and on."""
    from tamago_amd.board.go_board import GoBoard, zobrist_keys
    fx = rc.load_fixture(size)
    for i, entry in enumerate(fx.entries):
        host = GoBoard(size, 7.0, True)
        oracle = OracleBoard(size, 7.0, True)
        oracle.zobrist = zobrist_keys(size)
        color = BLACK
        for pos in entry.moves:
            host.put_stone(pos, color)
            oracle.put_stone(pos, color)
            color = opponent(color)
        assert bytes(host.cells) == bytes(oracle.board), entry.name
        assert (host.ko_pos, host.ko_move, host.moves) == (oracle.ko_pos, oracle.ko_move, oracle.moves), entry.name
        assert int(host.hash) == int(oracle.hash) == int(fx.hash[i]), entry.name
        assert np.array_equal(host.rec_hash, oracle.rec_hash), entry.name
        assert host.prev_move(1) == (oracle.rec_pos[oracle.moves - 1] if oracle.moves - 1 < oracle.max_records else 0)
        for flag in (False, True):
            host.check_superko = oracle.check_superko = flag
            assert host.get_all_legal_pos(color) == oracle.get_all_legal_pos(color), (entry.name, flag)


@pytest.mark.parametrize("name", sorted(rc.PERTURBATIONS))
@pytest.mark.parametrize("size", rc.SIZES)
def test_root_comparison_fails_on_a_wrong_rule(size, name):
    """A stand-in whose candidate rule is wrong in one way does not get through the root comparison of the GPU tests (both
    superko flags, as they run it: with superko on, the ko rule forbids nothing that superko does not) at any size.  Crafted
    records and ko forks go first: they are what most of these rules show on."""
    fx = rc.load_fixture(size)
    order = list(range(len(fx.entries)))[::-1]
    entries = [fx.entries[i] for i in order]
    with pytest.raises(rc.CorpusMismatch):
        for flag in (True, False):
            reader = rc.OracleReader(entries, superko=flag, board_cls=rc.PERTURBATIONS[name])
            rc.check_roots(entries, [fx.cand[int(flag)][i] for i in order], reader.root_actions())


@pytest.fixture(scope="module")
def oracle_trees():
    cache = {}

    def get(size):
        if size not in cache:
            fx = rc.load_fixture(size)
            roots = [fx.entries[i] for i in fx.tree_roots]
            reader = rc.OracleReader(roots)
            for tree in range(len(roots)):
                reader.search(tree)
            cache[size] = (roots, reader)
        return cache[size]
    return get


@pytest.mark.parametrize("size", rc.SIZES)
def test_tree_comparison_passes_on_the_oracle_and_the_roots_are_well_chosen(size, oracle_trees):
    """The node walk and the leaf-plane check on oracle.tree.MCTSTree + StubNet (root evaluation, mini-batches of 16, 16 and
    9 descents), and what those trees expand: nodes with a ko-forbidden point at every size, nodes after a capture and with a
    slow self-atari point at 9x9 and 19x19, roots where the side to move can take a ko."""
    roots, reader = oracle_trees(size)
    assert len(roots) == rc.N_TREE_ROOTS[size] and len(set(e.moves for e in roots)) == len(roots)
    reached = []
    for tree, entry in enumerate(roots):
        reached.append(rc.walk_tree(entry, reader.nodes(tree)))
        assert len(reader.leaves(tree)) == 1 + 41
        rc.check_leaves(entry, reached[-1], reader.leaves(tree))
    got = rc.expanded_coverage(reached)
    print(f"expanded by the oracle at {size}x{size}: {dict(got)}")
    for key, least in rc.EXPANDED_MINIMUMS[size].items():
        assert got[key] >= least, (key, got[key], least)
    takes = 0
    for entry in roots:
        board = rc.replay(entry)
        takes += any("ko_set" in rc.move_categories(board, pos, entry.to_move)
                     for pos in board.search_candidates(entry.to_move)[:-1])
    assert takes >= 2, takes


@pytest.mark.parametrize("name", ["superko_ignored", "self_atari_threshold_8"])
def test_tree_comparison_fails_on_a_wrong_rule(name, oracle_trees):
    """Below the roots too: trees grown at 9x9 under a wrong rule do not get through the node walk, and a tree whose leaf
    planes belong to another node does not get through the plane check."""
    roots, good = oracle_trees(9)
    reader = rc.OracleReader(roots, board_cls=rc.PERTURBATIONS[name])
    with pytest.raises(rc.CorpusMismatch):
        for tree, entry in enumerate(roots):
            reader.search(tree)
            rc.walk_tree(entry, reader.nodes(tree))
    reached = rc.walk_tree(roots[0], good.nodes(0))
    leaves = good.leaves(0)
    swapped = [(leaves[2][0], leaves[1][1])] + list(leaves[2:])
    with pytest.raises(rc.CorpusMismatch):
        rc.check_leaves(roots[0], reached, swapped)
