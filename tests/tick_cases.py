"""Cases that hold all eight instantiations of af_tick_kernel<KW, W64, MEMO> to the C oracle on searches that really search, under any
per-launch work budget.  Plain numpy + `oracle`, no GPU: the case table and the reference side.  Shared by
tests/test_tick_cases_cpu.py (the conditions the cases exist for, from the oracle alone) and tests/test_gpu_tick_partition.py.

Why the simulation counts are what they are (the 2 L rule).  In training mode the root's forced visits (player.py:264-276) pick among
the children with fewer than two visits until every legal cell has two.  With L legal cells, as long as simulation_per_step < 2 L every
simulation is one select at the root plus one expansion: the PUCT score, the noise mixed into it, W / N, a back-up over more than one
edge, the child cache and the tie-break among equal scores never run.  A training-mode case that is meant to search therefore has
simulation_per_step > 2 C (C = board cells); SHALLOW is the shape that does not, kept as a test of that arithmetic.

Both boards run in training mode with the 24-bit pseudo-net (tests/pseudonet.py, vbits = 24: an fp32 running sum of such values
rounds where an fp64 one does not), handed to the oracle as a pv_fn callback for both stores.
"""
import collections

import numpy as np

import oracle
import pseudonet
from conftest import make_cfg, run_in_threads

# name -> board, search settings, evaluator, noise-stream keys, games, memo geometry (a small table: entries are replaced)
Case = collections.namedtuple("Case", "name S goal sims cap salt peak seed first G log2_buckets max_stones kw2")
CASES = {
    "kw2": Case("kw2", 6, 4, 100, 130, 31, 8192, 30, 40, 8, 5, 6, 4),
    "kw4": Case("kw4", 12, 3, 300, 400, 31, 8192, 3, 40, 8, 5, 6, 8),      # 12 is the smallest board with four key words
}
VBITS = 24
HYPER2 = dict(c_puct=1.5, dirichlet_alpha=0.15)       # the second hyper-parameter set (one budget only on the GPU)
# the finding the cases answer: test_selfplay_engine_value_f64_four_word_boards_match_pipe_oracle_run's shape never descends
SHALLOW = dict(board_size=12, goal=4, simulation_per_step=24, upper_simulation_per_step=30, salt=31, peak=8192, seed=12, games=4)
TRACE_MOVES = 3
TRACE_GAMES = 4


def cfg_of(case, hyper=None):
    return make_cfg(board_size=case.S, goal=case.goal, simulation_per_step=case.sims, upper_simulation_per_step=case.cap,
                    **(hyper or {}))


def pv_np(case):
    """pseudonet.pseudonet_np(x, salt, peak, VBITS) for one position per call, with the per-cell tables computed once (an oracle
    episode asks for tens of thousands of leaves, one at a time); test_tick_cases_cpu holds it to pseudonet_np bit for bit."""
    C = case.S * case.S
    c = np.arange(C, dtype=np.int64)
    mix = pseudonet._mix32_np
    tab = np.concatenate([mix(c + 1), mix(c + 1001), mix(c + 2001)])
    mc = mix(c + 3001)
    vmask, vhalf, vscale = (1 << VBITS) - 1, 1 << (VBITS - 1), np.float32(1.0 / (1 << VBITS))

    def pv(x):
        bits = np.asarray(x).reshape(-1) != 0
        assert bits.size == 3 * C
        h = (case.salt + int(tab[bits].sum())) & pseudonet.M32
        m = mix(h ^ mc)
        k = 1 + (m & 0x3FF) + np.where(((m >> 10) & 7) == 0, case.peak, 0)
        mv = int(mix(np.array([h ^ 0x9E3779B9], np.int64))[0])
        value = np.float32((mv & vmask) - vhalf) * vscale
        return (k.astype(np.float32) * np.float32(1.0 / 131072.0))[None], np.array([value], np.float32)

    return pv


def pv_torch(case):
    return lambda x: pseudonet.pseudonet_torch(x, case.salt, case.peak, VBITS)


def _hyper_key(hyper):
    return tuple(sorted((hyper or {}).items()))


def oracle_player(case, game, value_f64, hyper=None, pv=None):
    """The oracle's player of engine slot `game` (noise stream first + game)."""
    return oracle.OraclePlayer(cfg_of(case, hyper), training=True, rng_mode=oracle.RNG_PHILOX, seed=case.seed,
                               game_id=case.first + game, value_f64=value_f64, pv_fn=pv or pv_np(case))


def leaf_id(planes):
    """(stones, packed bits of the three planes) of one leaf as the net sees it: position and last move."""
    b = np.asarray(planes).reshape(3, -1) != 0
    return int(b[0].sum() + b[1].sum()), np.packbits(b).tobytes()


_episodes, _traces = {}, {}


def episodes(name, value_f64, hyper=None):
    """The oracle's first episode (OraclePlayer.run) of every game of the case -> list over games of dict(records, actions, visits,
    final_value, stats, ties, leaves): stats / ties are the oracle's counters after the episode, leaves the set of leaf_id()s the
    game had evaluated.  Computed once and never changed."""
    key = (name, bool(value_f64), _hyper_key(hyper))
    if key not in _episodes:
        case = CASES[name]

        def one(g):
            leaves = set()
            net = pv_np(case)

            def pv(x):
                leaves.add(leaf_id(x[0]))
                return net(x)

            orc = oracle_player(case, g, value_f64, hyper, pv)
            recs, extra = orc.run()
            out = dict(records=recs, actions=extra["actions"], visits=extra["visits"], final_value=extra["final_value"],
                       stats=orc.stats(), ties=orc.tie_stats(), leaves=leaves)
            orc.close()
            return out

        _episodes[key] = run_in_threads(one, range(case.G))
    return _episodes[key]


class _Tree:
    """What test_gpu_parity._compare_tree asks of an oracle player: its tree_dump()."""

    def __init__(self, dump):
        self._dump = dump

    def tree_dump(self):
        return self._dump


def trace(name, value_f64):
    """Player.get_action move by move from the empty board, TRACE_MOVES moves (fewer if the game ends), for the first TRACE_GAMES
    games -> list over games of dict(moves=[dict(state, last, cell, policy, visits, tau)], tree=<tree_dump() holder of the final
    tree>, state / last = the position after the last traced move).  reset() first: the engine's first root of a game is installed
    with reset_tree, which advances the episode counter of the noise streams."""
    key = (name, bool(value_f64))
    if key not in _traces:
        case = CASES[name]
        S = case.S

        def one(g):
            orc = oracle_player(case, g, value_f64)
            orc.reset()
            board = np.zeros((S, S), np.int8)
            state, last, moves = oracle.board_to_state(board), None, []
            for _ in range(TRACE_MOVES):
                pol, act, vis = orc.get_action(state, last, False)
                moves.append(dict(state=state, last=last, cell=act[0] * S + act[1], policy=pol, visits=vis, tau=orc.tau))
                board = oracle.step(board, act)
                state, last = oracle.board_to_state(board), act
                if oracle.is_game_over(board, case.goal)[0]:
                    break
            out = dict(moves=moves, tree=_Tree(orc.tree_dump()), state=state, last=last)
            orc.close()
            return out

        _traces[key] = run_in_threads(one, range(TRACE_GAMES))
    return _traces[key]


def shallow_stats():
    """stats() of the SHALLOW shape's first episodes, fp64 store as in the test it comes from."""
    kw = dict(SHALLOW)
    salt, peak, seed, games = kw.pop("salt"), kw.pop("peak"), kw.pop("seed"), kw.pop("games")
    cfg = make_cfg(**kw)

    def one(g):
        orc = oracle.OraclePlayer(cfg, training=True, rng_mode=oracle.RNG_PHILOX, seed=seed, game_id=g, value_f64=True,
                                  pv_fn=lambda x: pseudonet.pseudonet_np(x, salt, peak, VBITS))
        recs, _ = orc.run()
        st = orc.stats()
        orc.close()
        return len(recs), st

    return cfg, run_in_threads(one, range(games))
