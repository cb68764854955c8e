"""The random streams' bookkeeping on the CPU: csrc/stream_windows.h (stream book, window book, feed rule, launch sizes),
compiled alone into tests/stream_windows_driver.cpp with the host compiler and carried out there against a CPU model of the
generation kernels.  Every script below is a sequence of driver-level operations as search.hip's entry points issue them;
what comes back - every draw a tree consumed (as the 53-bit integer random_sample() * 2^53), every state read, every refusal -
is held against numpy's RandomState alone: position by position from each tree's seed state, get_state() after the draws the
host accounted for.  A column that was never generated, or that the launch never waited for, comes back as 2^64 - 1."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gpu_rng import _states as _gpu_test_states

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 312                                        # draws in a state block of 624 words


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("stream_windows") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(HERE, "stream_windows_driver.cpp"), "-o", exe])

    def run(scripts):
        """Every script through one driver process; asserts each one's output line by line."""
        text = "".join(s.text() for s in scripts)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        got = res.stdout.splitlines()
        want = [line for s in scripts for line in s.expected]
        for k, (g, w) in enumerate(zip(got, want)):
            if g != w:
                case = [x for x in want[:k + 1] if x.startswith("case")][-1]
                pytest.fail(f"line {k} of {case!r}: got {g[:120]!r}, expected {w[:120]!r}")
        assert len(got) == len(want), (len(got), len(want), got[len(want):][:3], want[len(got):][:3])
    return run


_cache = {}


def _states(count):
    """tests/test_gpu_rng.py's start states (fresh, mid-block, odd word, pos 623 by index), made once"""
    if "states" not in _cache:
        _cache["states"] = _gpu_test_states(70)
    assert count <= 70
    return _cache["states"][:count]


def _fnv(key):
    h = 1469598103934665603
    for w in key.tolist():
        h = ((h ^ w) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


class Script:
    """A driver script and, from numpy alone, the lines the driver must print for it."""

    def __init__(self, name, trees, actions=10, overgen=2, no_snap=False, state_completes=True):
        self.T, self.A = trees, actions
        # (the driver reads the five numbers and echoes the line: the name rides along)
        self.lines = [f"case {trees} {actions} {overgen} {int(no_snap)} {int(state_completes)} {name}"]
        self.expected = [self.lines[0]]
        self.rs = [None] * trees                   # the stream at the position the DEVICE has read up to
        self.acc = [None] * trees                  # ... at the position the HOST has accounted for (collect, noise)
        self.pending = [0] * trees                 # draws read and not collected yet
        self.force = True                          # the driver's "invalidated" state: the next feed forces a new window
        self.host_at = None                        # reading a host-accepted window: [marker, count, cursor per tree]

    def text(self):
        return "\n".join(self.lines) + "\n"

    def _draws(self, t, n):
        return " ".join(map(str, (self.rs[t].random_sample(n) * 9007199254740992.0).astype(np.uint64).tolist()))

    def seed(self, t, state):
        self.rs[t], self.acc[t] = np.random.RandomState(), np.random.RandomState()
        self.rs[t].set_state(state)
        self.acc[t].set_state(state)
        self.pending[t] = 0
        self.force = True
        words = _cache.get(state[1].tobytes()) or _cache.setdefault(state[1].tobytes(), " ".join(map(str, state[1].tolist())))
        self.lines.append(f"seed {t} {int(state[2])} {words}")

    def seed_all(self, first=0):
        for t, state in enumerate(_states(first + self.T)[first:]):
            self.seed(t, state)

    def feed(self, need, first=0, force=None):
        self.lines.append(f"feed {need} {int(self.force if force is None else force)} {first}")
        self.force = False

    def op(self, text):
        self.lines.append(text)

    def install(self):
        self.lines.append("install")
        if self.host_at:
            self.host_at[2] = [0] * self.T

    def select(self, n):
        n = [n] * self.T if isinstance(n, int) else list(n)
        self.lines.append("select " + " ".join(map(str, n)))
        for t in range(self.T):
            if n[t] and self.host_at:
                marker, count, cur = self.host_at
                self.expected.append(f"draws {t} " + " ".join(str(marker + t * count + c) for c in range(cur[t], cur[t] + n[t])))
                cur[t] += n[t]
            elif n[t]:
                self.expected.append(f"draws {t} {self._draws(t, n[t])}")
                self.pending[t] += n[t]

    def collect(self, skip=None):
        self.lines.append("collect " + ("-" if skip is None else " ".join(map(str, skip))))
        for t in range(self.T):
            if not (skip and skip[t]) and self.pending[t]:
                self.acc[t].random_sample(self.pending[t])
            self.pending[t] = 0

    def noise(self, skip=None):
        self.lines.append("noise " + ("-" if skip is None else " ".join(map(str, skip))))
        self.force = True                          # (the noise sits between two windows)
        for t in range(self.T):
            if not (skip and skip[t]):
                assert self.pending[t] == 0
                self.expected.append(f"draws {t} {self._draws(t, self.A)}")
                self.acc[t].random_sample(self.A)

    def state(self, t):
        self.lines.append(f"state {t}")
        st = self.acc[t].get_state()
        self.expected.append(f"state {t} {int(st[2])} {_fnv(st[1])}")

    def accept(self, count, marker):
        self.lines.append(f"accept {count} {marker}")
        self.host_at = [marker, count, [0] * self.T]

    def leave_host_window(self):
        self.host_at = None
        self.force = True

    def states(self):
        for t in range(self.T):
            self.state(t)

    # ---- the drivers' orders ----
    def mini_batch(self, need, n):
        """engine.puct_batch / gumbel_phase: feed, selection launch (install), cursor read-back"""
        self.feed(need)
        self.install()
        self.select(n)
        self.collect()

    def chain(self, shares, takes, probe=None):
        """tg_search_puct_chain: one window for all mini-batches, the first share now, one extend per mini-batch, the rest at
        the end; probe(k): called between mini-batch k's extend and its install"""
        self.feed(sum(shares), first=shares[0] if len(shares) > 1 else 0)
        upto = 0
        for k, (share, take) in enumerate(zip(shares, takes)):
            upto += share
            if k:
                self.op(f"extend {upto}")
            if probe:
                probe(k)
            self.install()
            self.select(take)
        self.op("complete")
        self.collect()

    def selfplay_move(self, fresh, phases, root_take, started=True):
        """chain_begin: cursors collected with skip, noise with skip, the phases' window + the next root's prior in parts,
        installed by the first phase, completed behind it; no phase: the early install.  fresh[t]: the slot was reseeded"""
        if started:
            self.collect(fresh)
        self.noise(fresh)
        window = sum(phases)
        self.feed(window + self.A, first=phases[0] if phases else 0, force=True)
        for k, share in enumerate(phases):
            self.install()
            self.select([0 if fresh[t] else share for t in range(self.T)])
            if k == 0:
                self.op("complete")
        if not phases:
            self.op("complete")
            self.install()
        self.install()                             # tg_search_root_planes: the next roots' expansion, behind the phases
        self.select(root_take)


def _fixed_scripts(state_completes=True):
    out = []

    def new(name, trees, **kw):
        s = Script(name, trees, state_completes=state_completes, **kw)
        out.append(s)
        return s

    # ---- trees and needs on both sides of the over-generation rule, every kind of start state, mini-batches past column `need` ----
    for trees in (1, 2, 3, 17):
        for need in (2047, 2048, 4096):
            s = new(f"mini_batches_T{trees}_need{need}", trees)
            s.seed_all()
            takes = ([700] * 7) if trees < 17 else [need, 1, need - 1]
            for k, n in enumerate(takes):
                s.mini_batch(need, [max(0, n - 3 * t) for t in range(trees)])
                if k % 3 == 1:
                    s.states()
            s.states()
    # ---- ADVICE scenario 1: a state read between the feed and the install, the deferred rest open ----
    for trees in (1, 3):
        for overgen in (1, 2, 3):
            s = new(f"state_read_before_install_T{trees}_x{overgen}", trees, overgen=overgen)
            s.seed_all(first=trees)
            s.mini_batch(2048, 500)                # (something to commit)
            s.feed(2048, force=True)
            s.states()
            s.install()
            s.select(900)
            s.collect()
            for _ in range(4):                     # on past column `need`, into the rest
                s.mini_batch(2048, 900)
            s.states()
    # ---- ADVICE scenario 2: a state read between the install and the rest's completion ----
    for trees in (1, 2, 17):
        s = new(f"state_read_before_completion_T{trees}", trees)
        s.seed_all()
        s.mini_batch(300, 300)
        s.chain([1000, 1000, 1000], [1000, 990, 1000], probe=lambda k, s=s: s.states() if k else None)
        s.feed(3000, first=1000, force=True)
        s.install()
        s.select(1000)
        s.states()                                 # the rest still to come
        s.op("complete")
        s.install()
        s.select(2000)                             # past the first part
        s.collect()
        s.states()
    # ---- the chained-PUCT order: a window in parts, one extend per mini-batch, complete at the end ----
    for trees, share in ((1, 820), (3, 313), (17, 100)):
        s = new(f"puct_chain_T{trees}", trees, actions=82)
        s.seed_all()
        s.mini_batch(82 * 2, [82 - t for t in range(trees)])          # the root evaluation and a first mini-batch
        for n_batches in (1, 2, 5):
            s.chain([share] * n_batches, [[share - (t + k) % 7 for t in range(trees)] for k in range(n_batches)])
            s.states()
    # ---- the self-play chained-move order ----
    for trees in (1, 3, 17):
        s = new(f"selfplay_moves_T{trees}", trees, actions=82)
        s.seed_all()
        none, every = [0] * trees, [1] * trees
        s.selfplay_move(every, [], [82 - t % 5 for t in range(trees)], started=False)     # the first call: roots only
        s.selfplay_move(none, [600, 400, 200], [80] * trees)
        s.seed(trees - 1, _states(40)[39])         # its game ended while the device had gone on to the next root
        fresh = none[:-1] + [1]
        s.selfplay_move(fresh, [500, 250], [81] * trees)
        s.selfplay_move(none, [], [79] * trees)    # a move with no phase: the early install
        s.selfplay_move(none, [2100, 300], [82] * trees)
        s.collect(none)
        s.states()
    # ---- a host-accepted window takes the buffer of a generated one that was never installed ----
    for trees in (1, 2):
        s = new(f"accept_T{trees}", trees)
        s.seed_all()
        s.mini_batch(2048, 100)
        s.feed(2048, force=True)                   # (one or two trees: over-generated, its rest deferred to an install that never comes)
        s.accept(120, 1 << 60)
        s.install()
        s.select(120)
        s.leave_host_window()
        s.states()
        for _ in range(3):
            s.mini_batch(2048, 1100)
        s.states()
    # ---- a prefetched window (few trees: its rest deferred) that is never installed, and what may follow it ----
    for trees in (1, 3):
        for then in ("noise", "reseed", "feed"):
            s = new(f"prefetch_then_{then}_T{trees}", trees)
            s.seed_all()
            s.mini_batch(2048, 500)
            s.feed(2048, force=True)               # engine.prefetch_rng
            if then == "noise":
                s.noise()                          # engine.set_gumbel_noise: a launch from the base state
            elif then == "reseed":
                s.seed(trees - 1, _states(20)[19])
            else:
                s.feed(2048, force=True)           # a new window takes the buffer
            for _ in range(3):
                s.mini_batch(2048, 1100)
            s.states()
    # ---- the noise with a tree left out that has collected draws to commit: they stay its, the next window commits them ----
    for trees in (2, 17):
        s = new(f"noise_skips_a_tree_with_lag_T{trees}", trees)
        s.seed_all()
        s.mini_batch(2048, [500 + t for t in range(trees)])
        skip = [int(t == 1) for t in range(trees)]
        s.noise(skip)
        s.state(1)
        s.mini_batch(2048, 700)
        s.noise(skip)
        s.mini_batch(2048, 300)
        s.states()
    # ---- a window in parts whose rest no one asked for: the next request is served from it, and completes it first ----
    for trees in (1, 17):
        s = new(f"open_rest_then_served_T{trees}", trees)
        s.seed_all()
        s.feed(3000, first=1000)
        s.install()
        s.select(900)
        s.collect()
        s.mini_batch(500, 500)                     # (2000 columns left: no new window; columns 900 .. 1400 of this one)
        s.mini_batch(2048, 100)
        s.states()
    # ---- snapshots: on and off, the buffer growing mid-run, a tree reseeded between commits ----
    for no_snap in (False, True):
        s = new(f"snapshots_off{int(no_snap)}", 2, no_snap=no_snap)
        s.seed_all()
        s.mini_batch(40 * BLOCK, [35 * BLOCK + 5, 1])                  # snapshot 0 (32 blocks on) is there, the commit passes it
        # A larger window: the buffer grows in the very launch that commits those 35 blocks - tree 0's count still says "one
        # snapshot" and the new buffer holds none.  (No state read in between: its commit would zero the counts first.  Without
        # snap_plan's clear on growth tree 0 starts from 0xdeadbeef words here.)
        s.mini_batch(70 * BLOCK, [69 * BLOCK, 33 * BLOCK])
        s.seed(1, _states(12)[11])                                     # tree 1 leaves its stream with the commit still to come
        # same size: tree 0 commits past snapshots 0 and 1 of the window before.  Tree 1's count is cleared with its seed, which
        # no order can tell from leaving it: a fresh seed commits nothing, and this window rewrites what its own commit can select
        s.mini_batch(70 * BLOCK, [65 * BLOCK + 7, 66 * BLOCK])
        s.states()
        s.mini_batch(10, 10)
        s.states()
    s = new("snapshots_above_64_trees", 65, actions=3)
    s.seed_all()
    s.mini_batch(33 * BLOCK, [33 * BLOCK if t == 64 else 5 for t in range(65)])
    s.state(64)
    s.state(0)
    return out


def _random_script(k):
    """A legal sequence as a driver would issue it: engine-style blocks (mini-batches, chains, noise, reseeds, host windows) or
    self-play moves, with state reads dropped in between operations."""
    rnd = random.Random(5000 + k)
    trees = rnd.choice((1, 1, 2, 3, 3, 17))
    s = Script(f"random_{k}", trees, actions=rnd.choice((3, 10, 82)), overgen=rnd.choice((1, 2, 2, 3)), no_snap=rnd.random() < 0.3)
    s.seed_all(first=rnd.randrange(8))
    need_of = lambda: rnd.choice((40, 313, 700, 2047, 2048, 4096) if trees < 17 else (40, 313, 700, 2048))
    take_of = lambda need: [rnd.randrange(min(need, 200) + 1) if rnd.random() < 0.8 else rnd.randrange(need + 1) for _ in range(trees)]
    maybe_state = lambda *_: s.state(rnd.randrange(trees)) if rnd.random() < 0.3 else None
    if k % 2:
        fresh = [1] * trees
        for move in range(rnd.randrange(2, 6)):
            phases = [rnd.choice((60, 300, 900)) for _ in range(rnd.randrange(0, 4))]
            s.selfplay_move(fresh, phases, [rnd.randrange(1, s.A + 1) for _ in range(trees)], started=move > 0)
            maybe_state()
            fresh = [int(rnd.random() < 0.25) for _ in range(trees)]
            for t in range(trees):
                if fresh[t]:
                    s.seed(t, _states(30 + t)[rnd.randrange(30 + t)])
        s.collect(fresh)
    else:
        for _ in range(rnd.randrange(3, 9)):
            kind = rnd.random()
            if kind < 0.45:
                need = need_of()
                shape = rnd.random()
                if shape < 0.15:
                    s.feed(need_of(), force=True)  # prefetched; the request that follows is served from it or takes its buffer
                first = need // 2 if 0.15 <= shape < 0.3 else 0      # in parts, the rest left to whoever asks next
                s.feed(need, first=first, force=True if shape < 0.08 else None)
                maybe_state()
                s.install()
                s.select([min(n, first) for n in take_of(need)] if first else take_of(need))
                maybe_state()
                s.collect()
            elif kind < 0.7:
                shares = [rnd.choice((41, 312, 650)) for _ in range(rnd.randrange(1, 5))]
                s.chain(shares, [[rnd.randrange(share + 1) for _ in range(trees)] for share in shares], probe=maybe_state)
            elif kind < 0.8:
                if rnd.random() < 0.4:
                    s.feed(need_of(), force=True)  # prefetched, never installed
                s.noise([int(rnd.random() < 0.4) for _ in range(trees)] if rnd.random() < 0.5 else None)   # (trees left out keep their lag)
            elif kind < 0.9:
                if rnd.random() < 0.4:
                    s.feed(need_of(), force=True)  # prefetched, never installed
                s.seed(rnd.randrange(trees), _states(20)[rnd.randrange(20)])
            else:
                if rnd.random() < 0.5:
                    s.feed(need_of(), force=True)  # a generated window that is never installed
                s.accept(50, (1 << 60) + k)
                s.install()
                s.select([rnd.randrange(51) for _ in range(trees)])
                s.leave_host_window()
            maybe_state()
    s.states()
    return s


def test_fixed_orders_draw_numpys_streams(driver):
    """Trees 1, 2, 3, 17; needs 2047, 2048, 4096; the two ADVICE scenarios; the chained-PUCT and the self-play chained-move
    orders; a host-accepted window; a prefetched window that is never installed; the noise past a tree with lag; a rest left
    open; over-generation 1, 2, 3; snapshots on, off, growing, with a tree reseeded between commits."""
    driver(_fixed_scripts())


def test_random_legal_sequences_draw_numpys_streams(driver):
    scripts = [_random_script(k) for k in range(200)]
    assert len(scripts) == 200
    driver(scripts)


def test_a_base_launch_with_columns_to_come_is_refused(driver):
    """What the state read did before it completed the rest first (state_completes off: the commit goes out from the base
    state with the window's columns still to come) - deferred rest open, and between the install and the completion."""
    scripts = []
    for trees, first in ((1, 0), (3, 0), (17, 1000)):
        s = Script(f"refused_T{trees}", trees, state_completes=False)
        s.seed_all()
        s.mini_batch(500, 400)
        s.feed(3000, first=first, force=True)
        s.op("state 0")
        s.expected += ["refused", "failed state"]
        scripts.append(s)
    driver(scripts)
