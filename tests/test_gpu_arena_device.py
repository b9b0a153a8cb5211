"""The device-resident arena (alphafive_amd.arena.DeviceArena, af_engine.h af_match_*) against its yardsticks: the host-driven
play_matches on the same arguments and two oracle players per game.  Everything compared is an integer: bit-exact, no tolerance."""
import ctypes

import numpy as np
import pytest

import oracle
import pseudonet
from conftest import make_cfg

pytestmark = pytest.mark.gpu

NETS = [(101, 16384), (202, 4096)]
SEEDS = (5, 6)
KEYS = ("wins", "draws", "moves", "lengths")


def _pvs(nets=NETS):
    return [(lambda x, sp=sp: pseudonet.pseudonet_torch(x, sp[0], sp[1])) for sp in nets]


def _cfg(S, goal, sims, upper):
    return make_cfg(board_size=S, goal=goal, simulation_per_step=sims, upper_simulation_per_step=upper)


# name -> (S, goal, G, sims, upper, max_plies, nets)
SHAPES = {
    "s6_kw2_both_sides_win": (6, 4, 10, 40, 60, None, NETS),
    "s3_full_board_draw": (3, 3, 8, 20, 30, None, [(101, 0), (202, 0)]),
    "s11_odd_g_ended_and_stopped": (11, 5, 5, 30, 40, 40, NETS),
    "s15_kw4": (15, 5, 3, 24, 32, 60, NETS),
}
_yard = {}


def _yardstick(name):
    """play_matches on the shape, computed once per session and never changed."""
    if name not in _yard:
        from alphafive_amd import arena
        S, goal, G, sims, upper, max_plies, nets = SHAPES[name]
        pv = _pvs(nets)
        _yard[name] = arena.play_matches(_cfg(S, goal, sims, upper), pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1], max_plies=max_plies)
    return _yard[name]


def _finished(out, goal, S):
    """per game: did it end (win or draw) rather than stop at max_plies — replayed on the host from the move list"""
    from alphafive_amd import utils
    res = []
    for mv in out["moves"]:
        board = np.zeros((S, S), np.int8)
        done = False
        for c in mv:
            board = utils.step(board, (c // S, c % S))
            done, _ = utils.is_game_over(board, goal)
        res.append(bool(done))
    return res


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_arena_equals_play_matches(name, graph):
    from alphafive_amd import arena
    S, goal, G, sims, upper, max_plies, nets = SHAPES[name]
    want = _yardstick(name)
    # the branch this shape is here for is taken — by the yardstick, so that other seeds cannot quietly empty the case
    if name == "s3_full_board_draw":
        assert want["draws"] >= 1
    elif name == "s6_kw2_both_sides_win":
        assert want["wins"][0] >= 1 and want["wins"][1] >= 1
    elif name == "s11_odd_g_ended_and_stopped":
        fin = _finished(want, goal, S)
        assert any(fin) and not all(fin)
        assert all(n == max_plies for n, f in zip(want["lengths"], fin) if not f)
    pv = _pvs(nets)
    got = arena.play_matches_device(_cfg(S, goal, sims, upper), pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1], max_plies=max_plies,
                                    graph=graph)
    print(name, "graph" if graph else "eager", "yardstick", want["wins"], want["draws"], want["lengths"], "device", got["wins"],
          got["draws"], got["lengths"])
    for k in KEYS:
        assert got[k] == want[k], k
    assert set(got) == set(want)


def test_device_arena_matches_per_game_oracle_players():
    """No play_matches in between: the protocol of test_gpu_parity.test_batched_arena_matches_per_game_oracle_players."""
    from alphafive_amd import arena, utils
    S, goal, G = 6, 4, 10
    cfg = _cfg(S, goal, 40, 60)
    pv = _pvs()
    out = arena.play_matches_device(cfg, pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1])
    wins, draws = [0, 0], 0
    for i in range(G):
        players = [oracle.OraclePlayer(cfg, training=False, rng_mode=oracle.RNG_PHILOX, seed=s, game_id=i,
                                       pseudo_salt=sp[0], pseudo_peak=sp[1]) for s, sp in zip(SEEDS, NETS)]
        for pl in players:
            pl.reset()
        board = np.zeros((S, S), np.int8)
        state, action, cur, over, seq = utils.board_to_state(board), None, i % 2, False, []
        while not over:
            _, action, _ = players[cur].get_action(state, action, random_a=True)
            seq.append(action[0] * S + action[1])
            board = utils.step(utils.state_to_board(state, S), action)
            state = utils.board_to_state(board)
            over, v = utils.is_game_over(board, goal)
            cur = (cur + 1) % 2
        assert seq == out["moves"][i], f"game {i}"
        if v == 0.0:
            draws += 1
        else:
            wins[(cur + 1) % 2] += 1
    assert wins == out["wins"] and draws == out["draws"]
    assert out["lengths"] == [len(m) for m in out["moves"]]


def test_device_arena_replays_a_captured_graph():
    from alphafive_amd import arena
    S, goal, G, sims, upper, max_plies, nets = SHAPES["s6_kw2_both_sides_win"]
    pv = _pvs(nets)
    a = arena.DeviceArena(_cfg(S, goal, sims, upper), pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1])
    try:
        got = a.run(G, graph=True, rounds_per_replay=8)
        assert a.replays > 0
        assert a.eager_rounds - 1 == 0                   # the warm-up round in front of the capture and no other
        assert a.rounds == 1 + 8 * a.replays
        assert got["moves"] == _yardstick("s6_kw2_both_sides_win")["moves"]
        a.run(G, graph=True, rounds_per_replay=8)        # the graph is kept: no eager round at all
        assert a.replays > 0 and a.eager_rounds == 0
    finally:
        a.close()


def test_device_arena_reuse_equals_fresh_arenas():
    """af_match_start resets everything a match depends on: two runs on one arena = one run on each of two fresh arenas."""
    from alphafive_amd import arena
    S, goal, G, sims, upper, _, nets = SHAPES["s6_kw2_both_sides_win"]
    cfg = _cfg(S, goal, sims, upper)
    runs = [dict(n_games=G, max_plies=None), dict(n_games=G - 3, max_plies=12)]
    pv = _pvs(nets)
    a = arena.DeviceArena(cfg, pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1])
    try:
        reused = [a.run(**kw) for kw in runs]
    finally:
        a.close()
    for kw, got in zip(runs, reused):
        b = arena.DeviceArena(cfg, pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1])
        try:
            fresh = b.run(**kw)
        finally:
            b.close()
        assert got == fresh
    assert reused[0] == _yardstick("s6_kw2_both_sides_win")
    assert len(reused[1]["moves"]) == G - 3 and max(reused[1]["lengths"]) <= 12


def test_device_arena_reports_engine_error_and_recovers():
    """node_cap=58 at 6x6 with 50/60 simulations (test_gpu_parity.test_engine_fails_loudly_on_full_store): AF_ERR_NODE_CAP, an error
    code.  The failing game ends the match: run() raises naming the code before its loop bound, and the process goes on.
    Whether a store of 58 nodes overflows depends on the game: at the start of a move the collector keeps the subtree of the new root,
    and that plus up to 50 new simulations passes 58 only when the opponent's reply was a well-visited grandchild.  So the match has
    32 games, not the 4 the board would need; pytest.raises is the coverage condition (no overflow = the test fails, it does not pass
    quietly)."""
    from alphafive_amd import arena, engine as eng
    cfg = _cfg(6, 4, 50, 60)
    pv = _pvs()
    G = 32
    a = arena.DeviceArena(cfg, pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1], node_cap=58)
    try:
        with pytest.raises(eng.EngineError) as ei:
            a.run(G)
        assert "code -3" in str(ei.value) and "transposition store full" in str(ei.value)
        assert a.rounds <= 36 * (2 * 60 + arena.TICK_SLACK)
    finally:
        a.close()
    with pytest.raises(eng.EngineError, match="code -3"):
        arena.play_matches_device(cfg, pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1], node_cap=58, graph=False)
    S, goal, G, sims, upper, max_plies, nets = SHAPES["s6_kw2_both_sides_win"]
    got = arena.play_matches_device(_cfg(S, goal, sims, upper), pv[0], pv[1], G, seed0=SEEDS[0], seed1=SEEDS[1])
    assert got == _yardstick("s6_kw2_both_sides_win")


def test_match_create_checks_its_arguments():
    from alphafive_amd import engine as eng
    L = eng.lib()
    cfg6, cfg7 = _cfg(6, 4, 20, 30), _cfg(7, 4, 20, 30)
    mk = lambda cfg, G, mode: eng.Engine(cfg, G, mode=mode, training=False, seed=1)     # noqa: E731
    ext = mk(cfg6, 4, eng.MODE_EXTERNAL)
    others = dict(selfplay=mk(cfg6, 4, eng.MODE_SELFPLAY), unequal_g=mk(cfg6, 5, eng.MODE_EXTERNAL),
                  unequal_board=mk(cfg7, 4, eng.MODE_EXTERNAL), goal=mk(_cfg(6, 5, 20, 30), 4, eng.MODE_EXTERNAL))
    try:
        for name, other in others.items():
            for pair in ((ext, other), (other, ext)):
                h = ctypes.c_void_p()
                assert L.af_match_create(pair[0]._h, pair[1]._h, ctypes.byref(h)) == -1, name      # AF_ERR_ARG
                assert not h.value
        ok = mk(cfg6, 4, eng.MODE_EXTERNAL)
        others["ok"] = ok
        h = ctypes.c_void_p()
        assert L.af_match_create(ext._h, ok._h, ctypes.byref(h)) == 0 and h.value
        assert L.af_match_step(h, None) == -1                  # not started
        assert L.af_match_start(h, None, 5, 0) == -1           # more games than slots
        assert L.af_match_start(h, None, 4, 37) == -1          # more plies than cells
        L.af_match_destroy(h)
    finally:
        ext.close()
        for e in others.values():
            e.close()
