"""The evaluation cache on the device (csrc/eval_cache.hip, tamago_amd/nn/eval_cache.py) against the bit-exact
StubNet, the dict model and the oracle counts of tests/test_eval_cache_host.py, and against the same calls without a cache.
Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from tests import _eval_cache_cases as ec
from tests import _puct_match_cases as pc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
NAMES = ("lookups", "hits", "uncacheable", "inserts", "twin_skips", "evictions", "dropped", "tag_only_matches")


def real_rows(S, n, seed):
    """n feature-plane rows [n,6,S,S] (numpy) of random boards of both colours, from featurize_batch."""
    from tamago_amd.nn.feature import featurize_batch
    rnd = np.random.RandomState(seed)
    cells = rnd.choice([0, 1, 2], size=(n, S * S), p=[0.5, 0.25, 0.25]).astype(np.uint8)
    to_move = rnd.choice([1, 2], size=n)
    x, y = rnd.randint(S, size=n), rnd.randint(S, size=n)
    prev = np.where(rnd.random_sample(n) < 0.15, 0, (x + 1) + (y + 1) * (S + 2))
    moves = rnd.randint(0, 40, size=n)
    rows = featurize_batch(S, cells, to_move, prev, moves).cpu().numpy()
    assert all(ec.canonical(r.reshape(6, -1)) for r in rows[:8])
    return rows


def stub(rows, want_logits, salt=0):
    from oracle.stubnet import stub_outputs
    policy, logits, value = stub_outputs(rows, salt)
    return (logits if want_logits else policy), value


class Harness:
    """probe / StubNet on the misses / commit, by hand: what CachedEvaluator does, with every step open to the test."""

    def __init__(self, S, entries, ways=8, salt=0):
        from tamago_amd.nn.eval_cache import EvalCache
        self.S, self.salt = S, salt
        self.cache = EvalCache(S, entries, ways)

    def call(self, rows, want_logits):
        """-> (policy, value, n_miss, miss_planes as numpy)"""
        import torch
        dev = self.cache.device
        planes = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
        n, A = len(rows), self.S * self.S + 1
        policy = torch.full((n, A), float("nan"), device=dev)
        value = torch.full((n, 3), float("nan"), device=dev)
        n_miss, miss_planes = self.cache.probe(planes, want_logits, policy, value)
        if n_miss:
            missed = miss_planes.cpu().numpy().copy()
            mp, mv = stub(missed, want_logits, self.salt)
            self.cache.commit(torch.from_numpy(mp).to(dev), torch.from_numpy(mv).to(dev), policy, value)
        else:
            missed = np.zeros((0,) + rows.shape[1:], dtype=np.float32)
            self.cache.commit(None, None, policy, value)
        return policy.cpu().numpy(), value.cpu().numpy(), n_miss, missed

    def check(self, rows, want_logits, flags):
        policy, value, n_miss, missed = self.call(rows, want_logits)
        want_policy, want_value = stub(rows, want_logits, self.salt)
        assert policy.tobytes() == want_policy.tobytes() and value.tobytes() == want_value.tobytes()
        need = np.nonzero(np.asarray(flags) != ec.HIT)[0]
        assert n_miss == len(need)
        assert missed.tobytes() == np.ascontiguousarray(rows[need]).tobytes()          # the missed rows, in stable order


# ---- 1. probe and commit around StubNet -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("S", [9, 13, 19])
def test_probe_and_commit_around_stubnet(S, batch):
    rnd = np.random.RandomState(1000 * S + batch)
    pool = real_rows(S, 2 * batch, 7 * S + batch)
    old, new = pool[:batch], list(pool[batch:])
    h = Harness(S, 4096)
    model = ec.DictModel()
    try:
        h.check(old, False, model.call(old, False))                  # call 1 misses everywhere
        assert model.stats["hits"] == 0
        second = []
        for i in range(batch):                                       # call 2: old rows, new rows and in-call twins
            u = rnd.random_sample()
            second.append(old[rnd.randint(batch)] if u < 0.4 or batch == 1 else second[rnd.randint(i)] if u < 0.6 and i else new.pop())
        second = np.stack(second)
        h.check(second, False, model.call(second, False))
        h.check(second, True, model.call(second, True))              # the other outputs: another key, nothing is known
        h.check(second, True, model.call(second, True))              # ... and now everything is
        stats = h.cache.stats()
        assert stats["evictions"] == stats["dropped"] == stats["tag_only_matches"] == 0
        assert {k: stats[k] for k in model.stats} == model.stats
        assert stats["hits"] >= batch
    finally:
        h.cache.close()


# ---- 2. rows that are not canonical --------------------------------------------------------------------------------------------
def test_uncacheable_rows_are_evaluated_and_never_resident():
    S, entries = 9, 64
    rows = real_rows(S, 24, 5)
    odd = [1, 4, 7, 10, 13, 16, 23]
    rows[1, 0, 0, 0] = 0.5
    rows[4, 2, 8, 8] = 2.0
    rows[7, 4, 3, 3] = -1.0
    rows[10, 5, 8, 8] = -rows[10, 5, 8, 8]                           # a mixed plane 5
    rows[13] = 0.0                                                   # the zero row of a compacted launch
    rows[16, 5] = 0.0
    rows[23, 3, 4, 4] = -0.0
    h = Harness(S, entries, ways=8)
    model = ec.DictModel()
    try:
        for _ in range(3):
            flags = model.call(rows, False)
            assert [i for i, f in enumerate(flags) if f == ec.UNCACHED] == odd
            h.check(rows, False, flags)
        stats = h.cache.stats()
        assert stats["uncacheable"] == 3 * len(odd) and stats["hits"] == 2 * (24 - len(odd)) and stats["inserts"] == 24 - len(odd)
        keys = {tuple(ec.pack(rows[i].reshape(6, -1), False)) for i in range(24) if i not in odd}
        resident = [h.cache.debug_read(i) for i in range(entries)]
        assert {tuple(k) for tag, k, _, _ in resident if tag} == keys and sum(1 for e in resident if e[0]) == len(keys)
    finally:
        h.cache.close()


# ---- 3. eviction -----------------------------------------------------------------------------------------------------------------
def test_a_table_ten_times_too_small():
    S, ways = 9, 4
    entries = 2 * ways
    rows = real_rows(S, 10 * entries, 11)
    h = Harness(S, entries, ways)
    try:
        for lo in range(0, len(rows), 16):
            policy, value, n_miss, _ = h.call(rows[lo:lo + 16], False)
            want = stub(rows[lo:lo + 16], False)
            assert policy.tobytes() == want[0].tobytes() and value.tobytes() == want[1].tobytes() and n_miss == 16
        for lo in range(0, len(rows), 40):                            # queried again: exact whatever is still resident
            policy, value, n_miss, _ = h.call(rows[lo:lo + 40], False)
            want = stub(rows[lo:lo + 40], False)
            assert policy.tobytes() == want[0].tobytes() and value.tobytes() == want[1].tobytes()
        stats = h.cache.stats()
        assert stats["inserts"] + stats["twin_skips"] + stats["dropped"] == stats["lookups"] - stats["hits"] - stats["uncacheable"]
        assert stats["evictions"] > 0 and stats["uncacheable"] == 0
        by_key = {tuple(ec.pack(r.reshape(6, -1), False)): i for i, r in enumerate(rows)}
        want_policy, want_value = stub(rows, False)
        seen = set()
        for i in range(entries):
            tag, key, policy, value = h.cache.debug_read(i)
            assert tag != 0                                           # the table is full
            row = by_key[tuple(key)]                                  # every resident key is one of the rows ...
            assert row not in seen
            seen.add(row)
            hsh = ec.hash_key(key)
            assert (i // ways, tag >> 32) == ec.placement(hsh, 2, ways)[:2]
            assert policy.tobytes() == want_policy[row].tobytes() and value.tobytes() == want_value[row].tobytes()   # ... with its outputs
    finally:
        h.cache.close()


# ---- 4. clear ------------------------------------------------------------------------------------------------------------------------
def test_clear():
    rows = real_rows(9, 20, 13)
    h = Harness(9, 1024)
    try:
        assert h.call(rows, False)[2] == 20 and h.call(rows, False)[2] == 0
        h.cache.clear()
        assert h.call(rows, False)[2] == 20 and h.call(rows, False)[2] == 0
    finally:
        h.cache.close()


def test_new_weights_clear_the_cache():
    import torch
    from oracle.net import make_state_dict
    from tamago_amd.mcts.engine import DeviceEvaluator, evaluator_for
    from tamago_amd.nn.eval_cache import CachedEvaluator, EvalCache
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(make_state_dict(9, 3, 1.3))
    cache = EvalCache(9, 1024)
    try:
        evaluator = evaluator_for(net, 0, cache)
        assert type(evaluator) is CachedEvaluator and type(evaluator.inner) is DeviceEvaluator
        planes = torch.from_numpy(real_rows(9, 20, 17)).cuda()
        first = [t.clone() for t in evaluator(planes, False)]
        again = evaluator(planes, False)
        assert evaluator.batches == [20] and evaluator.handed == 40
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        net.load_state_dict(make_state_dict(9, 4, 1.3))
        fresh = evaluator(planes, False)
        assert evaluator.batches == [20, 20]                          # everything missed: the table was another network's
        want = net.forward_device(planes, False)
        assert torch.equal(fresh[0], want[0]) and torch.equal(fresh[1], want[1]) and not torch.equal(fresh[0], first[0])
        # the table remembers whose outputs it holds, not the evaluator: an evaluator built AFTER an upload (a tree that
        # rebuilds its engine) still finds the old weights' table cleared, and one built without an upload finds it warm
        warm = evaluator_for(net, 0, cache)
        warm(planes, False)
        assert warm.batches == []
        net.load_state_dict(make_state_dict(9, 5, 1.3))
        late = evaluator_for(net, 0, cache)
        out = late(planes, False)
        want = net.forward_device(planes, False)
        assert late.batches == [20] and torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        # ... and another network object never reads this one's table
        other = DualNet(torch.device("cuda:0"), 9)
        other.load_state_dict(make_state_dict(9, 6, 1.3))
        foreign = evaluator_for(other, 0, cache)
        out = foreign(planes, False)
        want = other.forward_device(planes, False)
        assert foreign.batches == [20] and torch.equal(out[0], want[0])
        assert net.range_fallbacks() == 0 and other.range_fallbacks() == 0
    finally:
        cache.close()


def test_a_tree_that_rebuilds_its_engine_after_new_weights():
    """MCTSTree(eval_cache=...) keeps its cache across engines: search, new weights, a search with another batch size (a new
    engine and evaluator) - the second search is the one a fresh tree makes under the new weights."""
    import torch
    from oracle.net import make_state_dict
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(make_state_dict(9, 3, 1.3))

    def search(tree, batch):
        tree.batch_size = batch
        np.random.seed(11)
        move = tree.search_best_move(GoBoard(9), 1, TimeManager(TimeControl.STRICT_PLAYOUT, 48), {})
        root = tree.get_root()
        return int(move), root.children_visits[:root.num_children].tolist(), root.children_value_sum[:root.num_children].tobytes()
    tree = MCTSTree(net, tree_size=64, batch_size=8, eval_cache=4096)
    try:
        search(tree, 8)
        net.load_state_dict(make_state_dict(9, 4, 1.3))
        got = search(tree, 4)
        assert len(tree._eval_caches) == 1
    finally:
        tree.close()
    assert tree._eval_caches == {} and tree._engine is None
    fresh = MCTSTree(net, tree_size=64, batch_size=4)
    try:
        assert got == search(fresh, 4) and net.range_fallbacks() == 0
    finally:
        fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()
    h = ctypes.c_void_p()
    for size, entries, ways in ((11, 64, 8), (9, 64, 0), (9, 64, 65), (9, 0, 8), (9, 60, 8), (9, -8, 8)):
        assert lib.tg_evalcache_create(size, 0, entries, ways, ctypes.byref(h)) == ERR_ARG and h.value is None
    assert lib.tg_evalcache_destroy(None) == 0
    assert lib.tg_evalcache_create(9, 0, 64, 8, ctypes.byref(h)) == 0
    try:
        planes = torch.from_numpy(real_rows(9, 4, 19)).cuda()
        policy, value = torch.zeros((4, 82), device="cuda"), torch.zeros((4, 3), device="cuda")
        other = torch.zeros((4, 82), device="cuda")
        n, ptr = ctypes.c_int32(-1), ctypes.c_void_p()
        args = (policy.data_ptr(), value.data_ptr(), None, ctypes.byref(n), ctypes.byref(ptr))
        assert lib.tg_evalcache_commit(h, policy.data_ptr(), value.data_ptr(), policy.data_ptr(), value.data_ptr(), None) == ERR_STATE
        ms = np.zeros(4, dtype=np.float32)
        assert lib.tg_evalcache_read_timing(h, ms.ctypes.data) == ERR_STATE          # (the timing-only path is off: nothing was timed)
        assert lib.tg_evalcache_probe(h, None, 4, 0, *args) == ERR_ARG
        assert lib.tg_evalcache_probe(h, planes.data_ptr(), 0, 0, *args) == ERR_ARG
        assert lib.tg_evalcache_probe(h, planes.data_ptr(), (1 << 20) + 1, 0, *args) == ERR_ARG
        assert lib.tg_evalcache_probe(h, planes.data_ptr(), 4, 0, None, value.data_ptr(), None, ctypes.byref(n), ctypes.byref(ptr)) == ERR_ARG
        assert lib.tg_evalcache_probe(h, planes.data_ptr(), 4, 0, policy.data_ptr(), value.data_ptr(), None, None, ctypes.byref(ptr)) == ERR_ARG
        stats = np.zeros(8, dtype=np.uint64)
        assert lib.tg_evalcache_stats(h, stats.ctypes.data, 0) == 0 and not stats.any()        # no row was looked up
        # a 13x13 network on a 9x9 cache
        from tamago_amd.nn.network.dual_net import DualNet
        net13 = DualNet(torch.device("cuda:0"), 13)
        assert lib.tg_evalcache_forward(h, net13.handle, planes.data_ptr(), 4, 0, policy.data_ptr(), value.data_ptr(), None) == ERR_ARG
        assert lib.tg_evalcache_stats(h, stats.ctypes.data, 0) == 0 and not stats.any()
        # probe twice; commit with other rows than the probe's
        torch.cuda.synchronize()
        assert lib.tg_evalcache_probe(h, planes.data_ptr(), 4, 0, *args) == 0 and n.value == 4
        assert lib.tg_evalcache_probe(h, planes.data_ptr(), 4, 0, *args) == ERR_STATE
        assert lib.tg_evalcache_clear(h, None) == ERR_STATE
        assert lib.tg_evalcache_commit(h, policy.data_ptr(), value.data_ptr(), other.data_ptr(), value.data_ptr(), None) == ERR_STATE
        assert lib.tg_evalcache_commit(h, None, None, policy.data_ptr(), value.data_ptr(), None) == ERR_ARG
        assert lib.tg_evalcache_stats(h, stats.ctypes.data, 0) == 0 and stats.tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
        assert lib.tg_evalcache_commit(h, other.data_ptr(), value.data_ptr(), policy.data_ptr(), value.data_ptr(), None) == 0
        assert lib.tg_evalcache_stats(h, stats.ctypes.data, 1) == 0 and stats.tolist() == [4, 0, 0, 4, 0, 0, 0, 0]
        assert lib.tg_evalcache_stats(h, stats.ctypes.data, 0) == 0 and not stats.any()        # reset
        tag = ctypes.c_uint64()
        assert lib.tg_evalcache_debug_read(h, 64, ctypes.byref(tag), None, None, None) == ERR_ARG
    finally:
        assert lib.tg_evalcache_destroy(h) == 0


# ---- 6. tg_evalcache_forward against tg_net_forward_dev -----------------------------------------------------------------------------
@pytest.mark.parametrize("S,batch,known", [(9, 200, 50), (9, 300, 100), (9, 600, 100), (9, 600, 400), (13, 40, 10), (19, 24, 6)])
def test_forward_equals_the_network(S, batch, known):
    """A scaled DualNet (make_state_dict, no f16 range fallback - asserted): the rows of one launch of `batch`, bit for bit, from a cache that already holds `known` of them
    (evaluated in a launch of `known`) and evaluates the rest in a launch of batch - known: 9x9 launches on both sides of
    the three-boards / one-board switch at the CU count (batch 300 / 600 against misses 200 / 500 / 200 and known 50 / 100 /
    400), 13x13 and 19x19.  Counted while no f16 range fallback was taken."""
    import torch
    from tamago_amd.mcts.engine import evaluator_for
    from tamago_amd.nn.eval_cache import EvalCache
    from tamago_amd.nn.network.dual_net import DualNet
    from oracle.net import make_state_dict
    net = DualNet(torch.device("cuda:0"), S)
    net.load_state_dict(make_state_dict(S, 3, 1.3))                  # (the scaled network of the other DualNet tests)
    cache = EvalCache(S, 8192)
    try:
        planes = torch.from_numpy(real_rows(S, batch, 23 + S)).cuda()
        for want_logits in (False, True):
            want = net.forward_device(planes, want_logits)
            evaluator = evaluator_for(net, 0, cache)
            pick = torch.from_numpy(np.random.RandomState(batch).permutation(batch)[:known].copy()).cuda()
            part = evaluator(planes[pick].contiguous(), want_logits)
            full = evaluator(planes, want_logits)
            assert evaluator.batches == [known, batch - known] and evaluator.handed == known + batch
            assert net.range_fallbacks() == 0                        # (this network stays in the f16 range: the comparison counts)
            assert torch.equal(part[0], want[0][pick]) and torch.equal(part[1], want[1][pick])
            assert torch.equal(full[0], want[0]) and torch.equal(full[1], want[1])
        stats = cache.stats()
        assert stats["hits"] == 2 * known and stats["inserts"] == 2 * batch and stats["lookups"] == 2 * (batch + known)
    finally:
        cache.close()


# ---- 7. trees ------------------------------------------------------------------------------------------------------------------------
def _engine(cached, entries=4096):
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    from tamago_amd.nn.eval_cache import CachedEvaluator, EvalCache
    evaluator = HostEvaluator(StubNet(7), torch.device("cuda", 0))
    cache = None
    if cached:
        cache = EvalCache(9, entries)
        evaluator = CachedEvaluator(evaluator, cache)
    return SearchEngine(9, 3, 60 + 16, 8, evaluator), cache


def _search_states(eng, visits=60, batch=8):
    """root statistics and the leaf queues after each mini-batch's selection"""
    out = []
    eng.root_eval(False)
    left = visits
    while left > 0:
        k = min(batch, left)
        eng.puct_select(k)
        queues = [eng.read_queue(t) for t in range(eng.T)]
        out.append([([int(i) for i in q.node_index], q.path, np.asarray(q.input_plane).tobytes()) for q in queues])
        eng.puct_flush()
        stats = eng.read_root_stats()
        out.append({k2: v.tobytes() for k2, v in stats.items()})
        left -= k
    return out


def test_trees_with_and_without_the_cache():
    """3 trees, 60 visits in mini-batches of 8, two consecutive moves (play the most visited move, search again): the same
    leaf queues and root statistics after every mini-batch with and without the cache, and the second search is served rows
    (how many, against the oracle: the next test, on the one tree the oracle searches)."""
    from tamago_amd.board.go_board import GoBoard
    seed, visits, batch = ec.TWO_MOVES
    runs = {}
    for cached in (False, True):
        eng, cache = _engine(cached)
        try:
            boards = [GoBoard(9), GoBoard(9), GoBoard(9)]
            boards[1].put_stone(boards[1].onboard_pos[40], 1)
            boards[2].put_stone(boards[2].onboard_pos[20], 1)
            boards[2].put_stone(boards[2].onboard_pos[60], 2)
            for t, b in enumerate(boards):
                eng.set_root(t, b, 1 if b.moves % 2 == 0 else 2, np.random.RandomState(seed + t).get_state())
            first = _search_states(eng, visits, batch)
            hits1 = cache.stats()["hits"] if cached else 0
            eng.play(np.full(3, -2, dtype=np.int32))
            second = _search_states(eng, visits, batch)
            runs[cached] = (first, second, eng.num_nodes().tolist())
            if cached:
                stats = cache.stats()
                assert stats["hits"] - hits1 > 0 and stats["uncacheable"] == 0
                assert sum(eng.evaluator.batches) == eng.forward_positions - stats["hits"] < eng.forward_positions
        finally:
            eng.close()
            if cache is not None:
                cache.close()
    assert runs[True] == runs[False]


def test_two_searches_of_one_tree_hit_what_the_oracle_counts():
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    from tamago_amd.nn.eval_cache import CachedEvaluator, EvalCache
    seed, visits, batch = ec.TWO_MOVES
    first, second, ((rows1, served1), (rows2, served2)) = ec.oracle_two_moves()
    cache = EvalCache(9, 4096)
    eng = SearchEngine(9, 1, visits + 16, batch, CachedEvaluator(HostEvaluator(StubNet(7), torch.device("cuda", 0)), cache))
    try:
        eng.set_root(0, GoBoard(9), 1, np.random.RandomState(seed).get_state())
        moves = []
        for want_rows, want_served in ((rows1, served1), (rows2, served2)):
            eng.root_eval(False)
            for k in [batch] * (visits // batch) + ([visits % batch] if visits % batch else []):
                eng.puct_batch(k)
            stats = cache.stats()
            assert (stats["lookups"], stats["hits"]) == (want_rows, want_served)
            moves.append(int(eng.best_moves(0.0, True)["move"][0]))
        assert moves == [first, second] and served2 - served1 > 0
        assert sum(eng.evaluator.batches) == rows2 - served2
    finally:
        eng.close()
        cache.close()


@pytest.mark.parametrize("layout", ["packed", "unique"])
def test_a_gumbel_phase_through_the_cache(layout):
    """Logits, the want_logits key bit and the packed / unique leaf layouts: the same trees with and without the cache."""
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    from tamago_amd.nn.eval_cache import CachedEvaluator, EvalCache

    def run(cached):
        evaluator = HostEvaluator(StubNet(3), torch.device("cuda:0"))
        cache = EvalCache(9, 4096) if cached else None
        eng = SearchEngine(9, 4, 160, 48, CachedEvaluator(evaluator, cache) if cached else evaluator)
        try:
            boards = [GoBoard(9) for _ in range(4)]
            boards[1].put_stone(boards[1].onboard_pos[40], 1)
            boards[3].put_stone(boards[3].onboard_pos[10], 1)
            for t, b in enumerate(boards):
                eng.set_root(t, b, 1 if b.moves % 2 == 0 else 2, np.random.RandomState(10 + t).get_state())
            eng.root_eval(use_logit=True)
            eng.set_gumbel_noise()
            kwargs = dict(unique=True) if layout == "unique" else dict(packed=True)
            eng.gumbel_phase([8, 0, 1, 4], [3, 0, 40, 5], **kwargs)
            eng.gumbel_phase([4, 8, 0, 2], [5, 3, 0, 9], **kwargs)
            stats = {k: v.tobytes() for k, v in eng.read_root_stats().items()}
            out = (stats, eng.num_nodes().tolist(), [s.final_state()[1].tobytes() for s in eng.streams])
            if cached:
                c = cache.stats()
                assert c["lookups"] == eng.forward_positions and c["hits"] + sum(eng.evaluator.batches) == c["lookups"]
                assert c["hits"] > 0                                  # (trees 0 and 2 search the same empty board)
            return out
        finally:
            eng.close()
            if cache is not None:
                cache.close()
    assert run(True) == run(False)


# ---- 8. puct_match --------------------------------------------------------------------------------------------------------------------
def _setups(shared):
    from tamago_amd.selfplay.puct_match import EngineSetup
    from tests._match_cases import make_net
    black = make_net(pc.S301)
    white = black if shared else make_net(pc.S302)
    return EngineSetup(black, *pc.BLACK_SEARCH), EngineSetup(white, *pc.WHITE_SEARCH)


def test_puct_match_three_boards_equal_the_oracle_games():
    from tamago_amd.selfplay.puct_match import puct_match
    import tempfile
    import os
    seeds = [1, 2, 3]
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _setups(False)
        out = puct_match(a, b, 3, boards=3, seeds=seeds, save_dir=tmp, eval_cache=1 << 14)
        for g, seed in enumerate(seeds):
            text, (moves, ending), state = pc.oracle_puct_game(seed, pc.S301, pc.S302)
            assert open(os.path.join(tmp, f"{g}.sgf")).read() == text
            result = out["results"][g]
            want = pc.oracle_result(text, moves, ending)
            assert {k: result[k] for k in want} == want
            assert pc.same_stream(result["stream"], state)
    stats = out["eval_cache_stats"]
    assert stats["caches"] == 2 and stats["hits"] > 0            # (a bucket may overflow at any occupancy: evictions are allowed)
    assert stats["inserts"] + stats["twin_skips"] + stats["dropped"] == stats["lookups"] - stats["hits"] - stats["uncacheable"]
    assert out["evaluated_positions"] == stats["lookups"] - stats["hits"] < out["forward_positions"]
    # one shared network object on both sides: one cache, and it serves more
    a, b = _setups(True)
    shared = puct_match(a, b, 3, boards=3, seeds=seeds, eval_cache=1 << 14)
    s2 = shared["eval_cache_stats"]                                  # (its games against the oracle: the one-board test below)
    assert s2["caches"] == 1 and s2["hits"] / s2["lookups"] > stats["hits"] / stats["lookups"]


@pytest.mark.parametrize("shared", [False, True], ids=["two_networks", "one_network"])
def test_puct_match_on_one_board_evaluates_what_the_cpu_test_counts(shared):
    """On ONE board a lock-step match makes the oracle's evaluator calls one for one: the rows handed over and the rows served
    are the CPU test's figures (tests/test_eval_cache_host.py EXPECTED_MATCH)."""
    from tamago_amd.selfplay.puct_match import puct_match
    from tests.test_eval_cache_host import EXPECTED_MATCH
    text, moves, ending, state, _ = ec.oracle_match_logs(shared)
    a, b = _setups(shared)
    out = puct_match(a, b, 1, boards=1, seeds=[ec.MATCH_SEED], eval_cache=1 << 14)
    assert out["results"][0]["moves"] == moves and pc.same_stream(out["results"][0]["stream"], state)
    rows, served = EXPECTED_MATCH[shared]
    stats = out["eval_cache_stats"]
    assert (stats["lookups"], stats["hits"]) == (rows, served) == ec.oracle_match_counts(shared)
    assert out["forward_positions"] == rows and out["evaluated_positions"] == rows - served
    assert stats["caches"] == (1 if shared else 2)


# ---- 9. analyze_positions -------------------------------------------------------------------------------------------------------------
def test_analyze_positions_of_one_record():
    """The plies of one short record side by side: the same output with and without the cache, and positions are served."""
    import re
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.analysis import analyze_positions
    text = pc.oracle_puct_game(1, pc.S301, pc.S302)[0]
    played = re.findall(r";([BW])\[([a-z]{2})\]", text)[:10]
    moves = [0 if sgf == "tt" else (ord(sgf[0]) - ord("a") + 1) + (ord(sgf[1]) - ord("a") + 1) * 11 for _, sgf in played]
    colors = [1 if c == "B" else 2 for c, _ in played]
    plies = len(moves) + 1
    # (the plies once more in a second chunk of trees, seeds and all: whatever the first chunk leaves unshared, these are served)
    positions = [(0, k) for k in range(plies)] * 2
    kwargs = dict(batch_size=8, records=[(moves, colors)], board_size=9, max_trees=plies, seeds=list(range(plies)) * 2)
    plain = analyze_positions(StubNet(5), positions, 40, **kwargs)
    cached = analyze_positions(StubNet(5), positions, 40, eval_cache=4096, **kwargs)
    report = cached.cache_report
    assert [(a.best_move, a.visits, a.value_sum, a.status) for a in plain] == \
        [(a.best_move, a.visits, a.value_sum, a.status) for a in cached]
    stats = report["eval_cache_stats"]
    assert stats["hits"] > 0 and report["evaluated_positions"] == report["forward_positions"] - stats["hits"]
