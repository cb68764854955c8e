"""Stand-in evaluators for the regions StubNet never reaches (TEST INFRASTRUCTURE - see oracle/__init__.py).

StubNet's outputs have one statistical shape: no policy entry is zero, no value is exactly 0, 0.5 or 1, the
logits lie in [-4, 4) and the searches stay shallow.  The three evaluators here follow its API (inference,
inference_with_policy_logits, a ``calls`` list, the same return types) and keep its guarantee - every output
is a float32 constant or ONE IEEE operation on integers, bit-identical on every machine - with other shapes:

  LineNet   all prior on one point: the search walks one line far below the 48 recorded path levels, ends in
            finished games that are queued again and again, and backs up exact values (0.5 or 1).
  FlatNet   every prior 1/128, values 0.25 / 0.75: siblings tie exactly, sums are exact, quotients are not.
  SpikyNet  three quarters of the priors exactly zero, one-hot values, logits in [-32, 32).

Plane layout: oracle/feature.py (plane 0 marks the empty points).
"""
import numpy as np
import torch

from oracle.stubnet import _mix, plane_hash


def _shape(planes: np.ndarray):
    b = planes.shape[0]
    p = planes.shape[2] * planes.shape[3]
    return b, p, p + 1


def line_outputs(planes: np.ndarray, mode: str):
    """Policy 1.0 on the first empty point in row-major order (on pass if the board is full), 0.0 elsewhere;
    logits +10 there and -10 elsewhere; value (0,1,0) for "half", (1,0,0) for "win"."""
    b, p, a = _shape(planes)
    empty = planes[:, 0].reshape(b, p) > 0.5
    first = np.where(empty.any(axis=1), np.argmax(empty, axis=1), p)
    policy = np.zeros((b, a), dtype=np.float32)
    policy[np.arange(b), first] = np.float32(1.0)
    logits = np.full((b, a), -10.0, dtype=np.float32)
    logits[np.arange(b), first] = np.float32(10.0)
    value = np.zeros((b, 3), dtype=np.float32)
    value[:, {"half": 1, "win": 0}[mode]] = np.float32(1.0)
    return policy, logits, value


def flat_outputs(planes: np.ndarray):
    """Policy 1/128 everywhere, logits 0; value (0.25, 0, 0.75) with an even number of stones on the board,
    (0.75, 0, 0.25) with an odd one."""
    b, p, a = _shape(planes)
    stones = p - np.rint(planes[:, 0].reshape(b, p)).astype(np.int64).sum(axis=1)
    policy = np.full((b, a), 1.0 / 128.0, dtype=np.float32)
    logits = np.zeros((b, a), dtype=np.float32)
    value = np.zeros((b, 3), dtype=np.float32)
    odd = (stones % 2) == 1
    value[:, 0] = np.where(odd, np.float32(0.75), np.float32(0.25))
    value[:, 2] = np.where(odd, np.float32(0.25), np.float32(0.75))
    return policy, logits, value


def spiky_outputs(planes: np.ndarray, salt: int = 0):
    """Hash-driven: a policy entry is exactly 0 unless its hash is 0 mod 4 (pass is never 0), else k/total with a
    small integer k - 1 for seven in eight, so that equal priors abound, 2..7 for the rest; logits n/4 - 32 for n in
    0..255; value one-hot on a hashed class."""
    b, p, a = _shape(planes)
    h = plane_hash(planes)
    with np.errstate(over="ignore"):
        ha = _mix(h[:, None] + np.arange(1, a + 1, dtype=np.uint64)[None, :]
                  * np.uint64(0xD1B54A32D192ED03) + np.uint64(salt))
        hv = _mix(h + np.uint64(977) + np.uint64(salt))
    few = (ha >> np.uint64(8)) % np.uint64(8) == 0
    k = np.where(few, ((ha >> np.uint64(12)) % np.uint64(6)).astype(np.int64) + 2, 1)          # 1 mostly, else 2..7
    k[:, :p] = np.where(ha[:, :p] % np.uint64(4) == 0, k[:, :p], 0)                                # pass is never 0
    total = k.sum(axis=1, keepdims=True)
    policy = k.astype(np.float32) / total.astype(np.float32)
    logits = ((ha >> np.uint64(20)) % np.uint64(256)).astype(np.float32) / np.float32(4.0) - np.float32(32.0)
    value = np.zeros((b, 3), dtype=np.float32)
    value[np.arange(b), (hv % np.uint64(3)).astype(np.int64)] = np.float32(1.0)
    return policy, logits, value


class _Net:
    """Drop-in for DualNet.inference / inference_with_policy_logits (as oracle.stubnet.StubNet)."""

    def __init__(self):
        self.calls = []

    def outputs(self, planes: np.ndarray):
        raise NotImplementedError

    def inference(self, planes: torch.Tensor):
        policy, _, value = self.outputs(planes.numpy())
        self.calls.append(planes.shape[0])
        return torch.from_numpy(policy), torch.from_numpy(value)

    def inference_with_policy_logits(self, planes: torch.Tensor):
        _, logits, value = self.outputs(planes.numpy())
        self.calls.append(planes.shape[0])
        return torch.from_numpy(logits), torch.from_numpy(value)


class LineNet(_Net):
    def __init__(self, mode: str = "half"):
        super().__init__()
        assert mode in ("half", "win")
        self.mode = mode

    def outputs(self, planes):
        return line_outputs(planes, self.mode)


class FlatNet(_Net):
    def outputs(self, planes):
        return flat_outputs(planes)


class SpikyNet(_Net):
    def __init__(self, salt: int = 0):
        super().__init__()
        self.salt = salt

    def outputs(self, planes):
        return spiky_outputs(planes, self.salt)


class LeafLog:
    """Wraps an evaluator and notes, mini-batch by mini-batch, which leaves were queued for it: `leaves` is a list of
    [(node index, depth), ...] per call.  watch(tree) reads them off a tree with the reference's batch_queue (the
    reference's and the oracle's MCTSTree); watch(probe=...) takes any callable that returns the pairs."""

    def __init__(self, network):
        self.network = network
        self.leaves = []
        self._probe = None

    @property
    def calls(self):
        return self.network.calls

    def watch(self, tree=None, probe=None):
        if probe is None:
            def probe():
                queue = tree.batch_queue
                return [(int(node), len(path)) for node, path in zip(queue.node_index, queue.path)]
        self._probe = probe

    def inference(self, planes):
        self.leaves.append(self._probe())
        return self.network.inference(planes)

    def inference_with_policy_logits(self, planes):
        self.leaves.append(self._probe())
        return self.network.inference_with_policy_logits(planes)


def make_net(name: str, salt: int = 0):
    """Evaluator by the name the hard-tree fixtures record: line_half, line_win, flat, spiky."""
    if name == "line_half":
        return LineNet("half")
    if name == "line_win":
        return LineNet("win")
    if name == "flat":
        return FlatNet()
    if name == "spiky":
        return SpikyNet(salt)
    raise ValueError(name)
