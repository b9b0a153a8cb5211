"""The engine's three device forms of utils.py:199-235 is_game_over (alphafive_amd/csrc/af_engine.hip: the two-sided whole-board
scan of a root and of a committed move, the wave-wide scan through the last stone of a descent with goal <= 8, the one-sided
whole-board scan of a descent with goal > 8) over the whole range af_engine_create accepts, decision by decision, on the crafted
boards of tests/terminal_cases.py; the C oracle's rule function is the authority (tests/test_rules_envelope.py pins it to the
unmodified reference on exactly these boards).  Then whole self-play episodes at (board, goal) pairs no other test runs."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle
import pseudonet
import terminal_cases as tc
from conftest import make_cfg

pytestmark = pytest.mark.gpu

AF_ERR_NO_ROOT = -4
LEAF_VALUE = 0.25
MAX_TICKS = 8           # a move of two simulations parks twice at most: three ticks


def _keys(boards, S):
    """int8 boards [n][S][S] -> position keys uint64[n][2 KW]: mine bitboard, then theirs (include/af_engine.h)."""
    kw = 2 if S * S <= 128 else 4
    flat = np.stack([b.reshape(-1) for b in boards])
    out = np.zeros((len(boards), 2 * kw), np.uint64)
    for half, colour in enumerate((1, -1)):
        bits = np.zeros((len(boards), 64 * kw), np.uint8)
        bits[:, :S * S] = flat == colour
        out[:, half * kw:(half + 1) * kw] = np.packbits(bits, axis=1, bitorder="little").view("<u8")
    return out


def _engine(S, goal, G):
    from alphafive_amd import engine as eng
    cfg = make_cfg(board_size=S, goal=goal, simulation_per_step=2, upper_simulation_per_step=2)
    return eng.Engine(cfg, G, mode=eng.MODE_EXTERNAL, training=False, seed=1, node_cap=10)      # (create's rule: sims + 8)


def _status_words(e):
    """The per-game status words, also when some of them are error codes (Engine.status raises on the first of those)."""
    from alphafive_amd import engine as eng
    st = np.zeros(e.G, np.int32)
    rc = eng.lib().af_engine_status(e._h, None, st.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc <= 0 and rc in (0, AF_ERR_NO_ROOT), rc
    return st


def _run_moves(e, policy, value, planes):
    from alphafive_amd import engine as eng
    for tick in range(MAX_TICKS):
        e.tick(policy.data_ptr(), value.data_ptr(), planes.data_ptr())
        st = _status_words(e)
        if ((st == eng.STATUS_MOVE_DONE) | (st < 0)).all():
            return st, tick + 1
    raise AssertionError("moves of two simulations not finished after %d ticks: status words %s" % (MAX_TICKS, np.unique(st)))


@pytest.mark.parametrize("S,goal", tc.PAIRS)
def test_descent_decides_every_crafted_child_like_the_oracle(S, goal):
    """The test is the evaluator: game g's root is the position before the crafted move, the policy row is 1.0 on that move and
    the value 0.25, so simulation 1 expands the root and simulation 2 steps to the crafted child (the only edge with a positive
    score, player.py:261-279: no tie, no draw) and runs the terminal test under scrutiny.  Expected after update_tree
    (player.py:166-184; the value flips once on the way up): a won child leaves n = 1, w = +1 on the root edge and one node, a
    drawn one n = 1, w = 0 and one node, an undecided one is parked, evaluated and expanded: n = 1, w = -0.25, two nodes."""
    import torch
    from alphafive_amd import engine as eng
    t0 = time.time()
    cases = tc.cases(S, goal)
    G, Cc = len(cases), S * S
    lasts = np.array([c.last for c in cases], np.int32)
    want = [oracle.is_game_over(c.child, goal) for c in cases]
    root_keys = _keys([tc.root_of(c) for c in cases], S)
    # the child as the side to move there sees it IS `child` (utils.py:275 step flips the colours): its key as the store holds it
    child_keys = _keys([c.child for c in cases], S)
    e = _engine(S, goal, G)
    e.set_roots(np.arange(G), root_keys, np.full(G, -1), reset_tree=True)
    pol = torch.zeros((G, Cc), dtype=torch.float32, device="cuda")
    pol[torch.arange(G), torch.from_numpy(lasts.astype(np.int64))] = 1.0
    val = torch.full((G,), LEAF_VALUE, dtype=torch.float32, device="cuda")
    planes = torch.zeros((G, 3, S, S), dtype=torch.float32, device="cuda")
    st, ticks = _run_moves(e, pol, val, planes)
    assert (st == eng.STATUS_MOVE_DONE).all(), np.unique(st)
    act, hp, _, vis, _ = e.move_results(np.arange(G))
    bad = []
    for g, (c, (over, value)) in enumerate(zip(cases, want)):
        d = e.tree_dump(g)
        onehot = np.zeros(Cc, np.int32)
        onehot[c.last] = 1
        w = np.zeros(Cc, np.float32)
        w[c.last] += np.float32(-value if over else -LEAF_VALUE)        # (a running sum from 0.0: a draw's -0.0 leaves +0.0)
        why = []
        if act[g] != c.last or not (vis[g] == onehot).all():
            why.append("move %d visits %s" % (act[g], np.flatnonzero(vis[g]).tolist()))
        if len(d["sum_n"]) != (1 if over else 2):
            why.append("%d nodes" % len(d["sum_n"]))
        if len(d["sum_n"]) >= 1:
            if not (d["keys"][0] == root_keys[g]).all() or d["sum_n"][0] != 1:
                why.append("root node key / sum_n %d" % d["sum_n"][0])
            if not (d["n"][0] == onehot).all() or d["w"][0].tobytes() != w.tobytes():
                why.append("root edge n %s w %s" % (d["n"][0][c.last], d["w"][0][c.last]))
            if d["f32"][0][c.last] != (0 if over else 1) or not (d["p"][0] == onehot.astype(np.float32)).all():
                why.append("root edge dtype flag / priors")
        if len(d["sum_n"]) >= 2 and (not (d["keys"][1] == child_keys[g]).all() or d["n"][1].any() or d["sum_n"][1] != 0):
            why.append("second node is not the unvisited child")
        if why:
            bad.append("(%d, %d) oracle %s: %s -- %s" % (S, goal, (over, value), "; ".join(why), tc.describe(c)))
    n_term = sum(o for o, _ in want)
    ct = e.counters()
    e.close()
    by_cls = {k: sum(c.cls == k for c in cases) for k in tc.CLASSES}
    print("\n[terminal envelope] descent (%d, %d) path %s: %d cases %s, %d terminal, %d ticks, %.2f s"
          % (S, goal, "through-last wave scan" if goal <= 8 else "one-sided board scan", G, by_cls, n_term, ticks, time.time() - t0))
    assert not bad, "%d of %d decisions differ:\n%s" % (len(bad), G, "\n".join(bad[:12]))
    assert ct["terminals"] == n_term and ct["sims"] == 2 * G and ct["selects"] == G and ct["expands"] == 2 * G - n_term, ct


@pytest.mark.parametrize("S,goal", tc.PAIRS)
def test_root_scan_refuses_exactly_the_decided_roots(S, goal):
    """The two-sided scan of an EXTERNAL root: a position handed over with a line of the side to move, of the opponent, of both
    (the scan order decides) or a full board is terminal in every simulation, so the move ends in AF_ERR_NO_ROOT (the reference dies
    in calc_policy there); every other root finishes its move."""
    import torch
    from alphafive_amd import engine as eng
    t0 = time.time()
    roots = tc.roots(S, goal)
    G, Cc = len(roots), S * S
    want = [oracle.is_game_over(r.board, goal) for r in roots]
    e = _engine(S, goal, G)
    e.set_roots(np.arange(G), _keys([r.board for r in roots], S), np.full(G, -1), reset_tree=True)
    pol = torch.full((G, Cc), 1.0 / Cc, dtype=torch.float32, device="cuda")
    val = torch.zeros((G,), dtype=torch.float32, device="cuda")
    planes = torch.zeros((G, 3, S, S), dtype=torch.float32, device="cuda")
    st, ticks = _run_moves(e, pol, val, planes)
    ct = e.counters()
    e.close()
    bad = ["(%d, %d) root %s/%s oracle %s status %d state %s" % (S, goal, r.kind, r.tag, w, s, tc.state_of(r.board))
           for r, w, s in zip(roots, want, st) if s != (AF_ERR_NO_ROOT if w[0] else eng.STATUS_MOVE_DONE)]
    n_term = sum(o for o, _ in want)
    print("\n[terminal envelope] roots (%d, %d): %d roots %s, %d decided, %d ticks, %.2f s"
          % (S, goal, G, {k: sum(r.kind == k for r in roots) for k in tc.ROOT_KINDS}, n_term, ticks, time.time() - t0))
    assert not bad, "%d of %d roots differ:\n%s" % (len(bad), G, "\n".join(bad[:12]))
    assert 0 < n_term < G and ct["terminals"] >= 2 * n_term and ct["plies"] == G - n_term, ct


@pytest.mark.parametrize("S,goal", [(2, 2), (8, 6), (10, 8), (11, 9), (12, 5), (13, 7), (14, 10), (16, 9)])
def test_selfplay_episodes_match_oracle_at_unvisited_pairs(S, goal):
    """Whole training episodes (the committed-move scan ends them) at pairs no other test runs, HIP engine vs oracle bit for bit.
    The high-goal pairs mostly run to a full board: drawn episodes of 144..256 plies through the goal > 8 descent and the
    partial-word board mask.  Seed 77 is chosen so (the oracle alone shows it) that the first episodes of games 0 and 3 at
    (14, 10) and of game 3 at (16, 9) are draws."""
    from alphafive_amd.engine import SelfPlayEngine, assemble_episode
    t0 = time.time()
    cfg = make_cfg(board_size=S, goal=goal, simulation_per_step=16, upper_simulation_per_step=24)
    G, compared = 8, (0, 3, 6)
    salt, peak, seed = 900, 4096, 77
    sp = SelfPlayEngine(cfg, G, lambda x: pseudonet.pseudonet_torch(x, salt, peak), device=0, seed=seed)
    got = {}
    for _ in range(160):                              # an episode is at most C plies of 16 simulations, a tick each
        sp.run_ticks(64)
        sp.check()
        for raw in sp.pop_raw(cap=64):
            got.setdefault(raw["game"], []).append(raw)
        if all(len(got.get(g, [])) >= 1 for g in compared):
            break
    assert all(len(got.get(g, [])) >= 1 for g in compared), "a compared game never finished an episode"
    long_or_drawn, n_eps = 0, 0
    for g in compared:
        orc = oracle.OraclePlayer(cfg, training=True, rng_mode=oracle.RNG_PHILOX, seed=seed, game_id=g,
                                  pseudo_salt=salt, pseudo_peak=peak)
        for raw in got[g][:2]:
            orec, extra = orc.run()
            assert raw["T"] == len(orec) and (raw["actions"] == extra["actions"]).all(), f"game {g} seq {raw['seq']}"
            assert (raw["visits"] == extra["visits"]).all() and raw["final_value"] == extra["final_value"]
            rec, result = assemble_episode(raw, S, cfg.gamma)
            for (s, p, la, v, w), (os_, op, ola, ov, ow) in zip(rec, orec):
                assert s == os_ and la == ola and v == ov and w == ow
                assert (p.view(np.uint32) == op.view(np.uint32)).all()
            long_or_drawn += result == 0 or raw["T"] >= S * S - 8
            n_eps += 1
    sp.close()
    print("\n[terminal envelope] episodes (%d, %d): %d compared, %d drawn or within 8 plies of a full board, %d ticks, %.2f s"
          % (S, goal, n_eps, long_or_drawn, sp.ticks, time.time() - t0))
    if (S, goal) in ((14, 10), (16, 9)):
        assert long_or_drawn >= 1, "no compared episode ran to (nearly) a full board"
