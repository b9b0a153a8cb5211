"""The deep bf16 net behind the reference's call surface: Player(cfg, pv_fn=deep.eval) on the hand-written kernels under a HIP
graph against the C oracle fed leaf by leaf through a second evaluator of the same net, across weight updates, with several
consumers on one net, and in the arena and the checkpoint ladder.  Everything compared is bits, moves or counts: no tolerance."""
import numpy as np
import pytest

import oracle
from conftest import make_cfg
from test_gpu_realnet import _drive
from tower_gpu import planes, same_bits

pytestmark = pytest.mark.gpu
BLOCKS, W = 2, 128


def _deep(S, seed):
    from alphafive_amd.network_deep import DeepResNet
    return DeepResNet(S, blocks=BLOCKS, width=W, device="cuda", seed=seed)


def _np_eval(ev):
    """numpy float32[B,3,S,S] -> (prob, value) numpy copies through a device evaluator: what the oracle is fed with."""
    import torch

    def f(x):
        p, v = ev(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
        return p.cpu().numpy().copy(), v.cpu().numpy().copy()
    return f


def _on_device(net):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in net.variables.items()}


@pytest.mark.parametrize("S, sims, cap, moves, training", [(11, 60, 80, 3, True), (15, 40, 52, 2, True), (11, 60, 80, 3, False)],
                         ids=["11x11-training", "15x15-training", "11x11-play"])
def test_player_over_deep_eval_matches_the_oracle(S, sims, cap, moves, training):
    """Player(pv_fn=deep.eval): the leaves stay on the device and go through an evaluator of the Player's own (batch 1: the
    tile-parallel tower kernel where the library found it faster), 16 x (tick + forward) replayed as a HIP graph.  Moves, visit
    vectors, policy bits and the whole tree equal the oracle's, which is fed by a second evaluator of the same net."""
    from alphafive_amd.player import Player
    from test_gpu_parity import _compare_tree
    deep = _deep(S, 3)
    try:
        cfg = make_cfg(board_size=S, simulation_per_step=sims, upper_simulation_per_step=cap)
        pl = Player(cfg, training=training, pv_fn=deep.eval, seed=11, game_id=2)
        assert pl.backend == "hip" and pl._pv_owner is deep
        orc = oracle.OraclePlayer(cfg, training=training, rng_mode=oracle.RNG_PHILOX, seed=11, game_id=2, pv_fn=_np_eval(deep.evaluator(1)))
        _drive(pl, orc, training, moves, S=S)
        assert pl._graph is not None and pl._graph[1] is not None           # the HIP-graph path ran
        _compare_tree(pl._engine.tree_dump(0), orc, S)
        assert len(pl.tree) == orc.tree_size()
        pl.close()
    finally:
        deep.close()


def test_deep_player_follows_weight_updates_in_place(tmp_path):
    """test_gpu_realnet.test_player_graph_path_follows_a_weight_update for the deep net: after set_variables_device from fp32
    tensors, and again after load_npz, the Player equals the oracle fed by an evaluator of ANOTHER net that holds the new weights;
    the Player's evaluator and its bound outputs are the objects they were, and the graph was captured again."""
    from alphafive_amd.player import Player
    from test_gpu_parity import _compare_tree
    deep, second, third = _deep(11, 3), _deep(11, 4), _deep(11, 5)
    try:
        feeds = [_np_eval(net.evaluator(1)) for net in (deep, second, third)]
        feed = [feeds[0]]
        cfg = make_cfg(simulation_per_step=60, upper_simulation_per_step=80)
        pl = Player(cfg, training=True, pv_fn=deep.eval, seed=5, game_id=7)
        orc = oracle.OraclePlayer(cfg, training=True, rng_mode=oracle.RNG_PHILOX, seed=5, game_id=7, pv_fn=lambda x: feed[0](x))
        ev, tower = pl._pv_device, pl._pv_device.tower
        assert tower.policy is pl._policy and tower.value is pl._value
        state, last = _drive(pl, orc, True, 2)
        g0 = pl._graph
        deep.set_variables_device(_on_device(second))
        feed[0] = feeds[1]
        state, last = _drive(pl, orc, True, 2, state=state, last=last)
        g1 = pl._graph
        assert g1[0] != g0[0] and g1[1] is not g0[1]                        # dropped and captured again
        path = str(tmp_path / "third.npz")
        third.save_npz(path)
        deep.load_npz(path)
        feed[0] = feeds[2]
        _drive(pl, orc, True, 2, state=state, last=last)
        assert pl._graph[0] != g1[0]
        assert pl._pv_device is ev and ev.tower is tower and tower.policy is pl._policy and tower.value is pl._value
        _compare_tree(pl._engine.tree_dump(0), orc, 11)
        pl.close()
    finally:
        for net in (deep, second, third):
            net.close()


def test_two_players_and_an_engine_evaluator_share_one_deep_net():
    """Every consumer has its own tower: two Players on one net, moved alternately, each equal to its own oracle, and an evaluator
    from select_backend("hip", 8) made before them gives afterwards the bits it gave before."""
    from alphafive_amd.player import Player
    deep = _deep(11, 8)
    try:
        x = planes(8, seed=2, S=11)
        pv = deep.select_backend("hip", 8)
        before = tuple(t.clone() for t in pv(x))
        cfg = make_cfg(simulation_per_step=40, upper_simulation_per_step=52)
        pls = [Player(cfg, training=True, pv_fn=deep.eval, seed=21 + i, game_id=i) for i in range(2)]
        assert len({id(p._pv_device.tower) for p in pls} | {id(deep._tower)}) == 3
        orcs = [oracle.OraclePlayer(cfg, training=True, rng_mode=oracle.RNG_PHILOX, seed=21 + i, game_id=i,
                                    pv_fn=_np_eval(deep.evaluator(1))) for i in range(2)]
        at = [(None, None), (None, None)]
        for _ in range(2):
            for i in (0, 1):
                at[i] = _drive(pls[i], orcs[i], True, 1, state=at[i][0], last=at[i][1])
        assert all(p.backend == "hip" and p._graph is not None for p in pls)
        after = tuple(t.clone() for t in pv(x))
        assert same_bits(after, before)
        one = tuple(t.clone() for t in deep.evaluator(1)(x[3:4].contiguous()))
        assert same_bits(one, (before[0][3:4], before[1][3:4]))
        for p in pls:
            p.close()
    finally:
        deep.close()


KEYS = ("wins", "draws", "moves", "lengths")


def test_arena_and_ladder_over_deep_nets(tmp_path):
    """play_matches_device over evaluator(8) of two deep nets = play_matches over the same evaluators, to the cell; ladder() with a
    net_factory over three deep checkpoints = the bracket played by hand with play_matches_device on the same pairs."""
    from alphafive_amd import arena
    from alphafive_amd.network_deep import DeepResNet
    cfg = make_cfg(simulation_per_step=30, upper_simulation_per_step=40)
    nets = [_deep(11, s) for s in (31, 32, 33)]
    try:
        evs = [net.evaluator(8) for net in nets]
        want = arena.play_matches(cfg, evs[0], evs[1], 8, seed0=5, seed1=6)
        got = arena.play_matches_device(cfg, evs[0], evs[1], 8, seed0=5, seed1=6)
        print("deep arena: play_matches", want["wins"], want["draws"], want["lengths"], "device", got["wins"], got["draws"], got["lengths"])
        for k in KEYS:
            assert got[k] == want[k], k
        paths = []
        for i, net in enumerate(nets):
            paths.append(str(tmp_path / ("ckpt%d.npz" % i)))
            net.save_npz(paths[-1])
        games = 4
        bracket = arena.ladder(cfg, paths, games=games, log=None, net_factory=lambda: DeepResNet(11, BLOCKS, W, device="cuda"))
        hand, low, high = [], 0, len(paths) - 1
        while low < high:
            r = arena.play_matches_device(cfg, nets[low].evaluator(games), nets[high].evaluator(games), games)
            hand.append((paths[low], paths[high], r["wins"][0], r["wins"][1], r["draws"]))
            if r["wins"][0] < r["wins"][1]:
                low += 1
            else:
                high -= 1
        assert bracket == hand and len(bracket) == 2
    finally:
        for net in nets:
            net.close()
