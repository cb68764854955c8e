"""Sequential-halving schedule (host integer logic; mirror of the mctx schedule used by
mcts/sequential_halving.py:7-60)."""
import functools
import math
from typing import Dict, Tuple


def get_sequence_of_considered_visits(max_num_considered_actions: int,
                                      num_simulations: int) -> Tuple[int, ...]:
    if max_num_considered_actions <= 1:
        return tuple(range(num_simulations))
    log2max = int(math.ceil(math.log2(max_num_considered_actions)))
    out = []
    visits = [0] * max_num_considered_actions
    width = max_num_considered_actions
    while len(out) < num_simulations:
        rounds = max(1, int(num_simulations / (log2max * width)))
        for _ in range(rounds):
            out.extend(visits[:width])
            visits[:width] = [v + 1 for v in visits[:width]]
        width = max(2, width // 2)
    return tuple(out[:num_simulations])


def get_candidates_and_visit_pairs(max_num_considered_actions: int,
                                   num_simulations: int) -> Dict[int, int]:
    """{number of considered actions: number of levels} in phase order."""
    return dict(_pairs_cached(max_num_considered_actions, num_simulations))


@functools.lru_cache(maxsize=256)
def _pairs_cached(max_num_considered_actions: int, num_simulations: int):
    seq = get_sequence_of_considered_visits(max_num_considered_actions, num_simulations)
    width_at_level = [0] * (max(seq) + 1)
    for level in seq:
        width_at_level[level] += 1
    pairs: Dict[int, int] = {}
    for width in width_at_level:
        pairs[width] = pairs.get(width, 0) + 1
    return tuple(pairs.items())


# the most root children one phase enters (mcts/node.py:324-346: at most 16 considered actions, plus child 0, which takes the
# descents that find no child under the count threshold) - kUniqueE of the library
UNIQUE_E = 17
# descents per tree beyond which a phase runs on the one-wavefront selection kernel, which saves nothing
UNIQUE_PIPE_MAX = 512


def unique_plane_caps(num_considered, max_count, E: int = UNIQUE_E, pipelined=None):
    """Plane slots per tree of one phase in the UNIQUE leaf layout - the library's arithmetic (tg_search_unique_planes):
    cap[t] = min(num_considered[t] * max_count[t], E) when the launch takes the pipelined selection kernel, the product
    itself when it does not.  `pipelined`: None = decided by the launch's busiest tree (<= UNIQUE_PIPE_MAX descents; a
    pool beyond 2^21 nodes or TG_SELECT_SERIAL also force the one-wavefront kernel - pass False then)."""
    n = [int(a) * int(b) for a, b in zip(num_considered, max_count)]
    if pipelined is None:
        pipelined = max(n, default=0) <= UNIQUE_PIPE_MAX
    return [min(v, E) if pipelined else v for v in n]
