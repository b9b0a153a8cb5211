"""The conditions tests/tick_cases.py's cases exist for, checked from the C oracle alone (no GPU), so that another seed, salt or board
cannot quietly empty them: the searches descend (PUCT, noise, W / N, multi-edge back-ups and the child cache all run), simulations
end in terminal positions, uniform picks have several candidates, episodes end before the board is full, the fp64 store holds sums
an fp32 store would have rounded, and games share small positions (the evaluation memo has something to hit)."""
import numpy as np
import pytest

import tick_cases as tc

VARIANTS = [(name, f64, hyper) for name in tc.CASES for f64 in (False, True) for hyper in (None, tc.HYPER2)]
IDS = ["%s-%s-%s" % (n, "f64" if f else "f32", "hyper2" if h else "default") for n, f, h in VARIANTS]


@pytest.mark.parametrize("name,value_f64,hyper", VARIANTS, ids=IDS)
def test_every_game_of_a_case_searches_below_the_root(name, value_f64, hyper):
    case = tc.CASES[name]
    C = case.S * case.S
    assert case.sims > 2 * C and case.cap > case.sims              # the 2 L rule: PUCT runs at the root of every move
    eps = tc.episodes(name, value_f64, hyper)
    assert len(eps) == case.G
    ties = dict(select=0, forced=0, best=0)
    for g, e in enumerate(eps):
        st, T = e["stats"], len(e["records"])
        print(name, value_f64, hyper, "game", g, "T", T, st, e["ties"])
        assert st["plies"] == T and st["sims"] == st["expands"] + st["terminals"]
        assert st["selects"] >= 1.25 * st["sims"], (g, st)
        assert st["terminals"] > 0, (g, st)
        assert 0 < T < C, (g, T)                                   # ends before the board is full: by a line, not a draw
        assert e["final_value"] == -1.0
        for k in ties:
            ties[k] += e["ties"][k]
    # uniform picks with more than one candidate: the forced-visit pick (:264-276) and the pick among the most visited root
    # children (:102) in every variant; the pick among equal PUCT scores is rare enough to be a condition of the whole case (below)
    assert ties["forced"] > 0 and ties["best"] > 0, ties


@pytest.mark.parametrize("name", list(tc.CASES))
def test_a_case_holds_a_pick_among_equal_puct_scores(name):
    """Under Dirichlet noise (mixed into every edge of every node, player.py:247-253) two edges of one select share an fp32 score
    about once in 200,000 selects (measured on the oracle over 40 seeds per board: 0..3 per 300,000), so the seeds of the case table
    were taken from an oracle scan for episodes that hold such a pick: the tie-break of :277-279 runs somewhere in the case, with
    both stores."""
    for f64 in (False, True):
        n = sum(e["ties"]["select"] for hyper in (None, tc.HYPER2) for e in tc.episodes(name, f64, hyper))
        print(name, "f64" if f64 else "f32", "picks among equal scores:", n)
        assert n >= 1


@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_hyper_parameter_sets_and_the_games_of_a_case_differ(name):
    d, h = tc.episodes(name, False), tc.episodes(name, False, tc.HYPER2)
    assert any(len(a["records"]) != len(b["records"]) or (a["actions"] != b["actions"]).any() for a, b in zip(d, h))
    games = tc.episodes(name, False)
    assert len({tuple(e["actions"]) for e in games}) == len(games)          # every game is its own game


@pytest.mark.parametrize("name", list(tc.CASES))
def test_fp64_rows_hold_sums_an_fp32_store_would_have_rounded(name):
    rounded = edges = 0
    for t in tc.trace(name, True):
        w = t["tree"].tree_dump()["w64"]
        rounded += int((w != w.astype(np.float32)).sum())
        edges += int((w != 0).sum())
    print(name, "fp64 W values not representable in fp32:", rounded, "of", edges, "non-zero")
    assert rounded > 0
    for t in tc.trace(name, False):
        assert "w64" not in t["tree"].tree_dump()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_traces_run_their_moves_and_search_below_the_root(name):
    case = tc.CASES[name]
    for f64 in (False, True):
        for t in tc.trace(name, f64):
            assert 1 <= len(t["moves"]) <= tc.TRACE_MOVES
            d = t["tree"].tree_dump()
            assert len(d["sum_n"]) > len(t["moves"]) * case.S * case.S          # more nodes than the roots' children: depth >= 2
            # (the first simulation of a game expands the empty root without a select: sims - 1 visits on the first move)
            assert all(m["policy"] is not None and m["visits"].sum() >= case.sims - 1 for m in t["moves"])


@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_one_position_evaluator_is_the_pseudo_net(name):
    import pseudonet
    case = tc.CASES[name]
    rng = np.random.RandomState(case.S)
    pv = tc.pv_np(case)
    C = case.S * case.S
    for stones in (0, 1, 2, 7, C // 2, C):
        x = np.zeros((1, 3, C), np.float32)
        cells = rng.permutation(C)[:stones]
        x[0, 0, cells[::2]] = 1
        x[0, 1, cells[1::2]] = 1
        if stones > 1:
            x[0, 2, cells[1]] = 1
        x = x.reshape(1, 3, case.S, case.S)
        p, v = pv(x)
        wp, wv = pseudonet.pseudonet_np(x, case.salt, case.peak, tc.VBITS)
        assert p.dtype == wp.dtype == np.float32 and v.dtype == wv.dtype == np.float32
        assert p.tobytes() == wp.tobytes() and v.tobytes() == wv.tobytes()
        pt, vt = tc.pv_torch(case)(__import__("torch").from_numpy(x))
        assert pt.numpy().tobytes() == wp.tobytes() and vt.numpy().tobytes() == wv.tobytes()


@pytest.mark.parametrize("name,value_f64", [(n, f) for n in tc.CASES for f in (False, True)])
def test_games_share_small_positions_for_the_memo(name, value_f64):
    """At least two games had the same non-empty position with at most max_stones stones and the same last move evaluated (the empty
    board, which every game shares, is left out)."""
    case = tc.CASES[name]
    small = [{l for l in e["leaves"] if 0 < l[0] <= case.max_stones} for e in tc.episodes(name, value_f64)]
    pairs = sum(1 for a in range(case.G) for b in range(a) if small[a] & small[b])
    distinct = len(set().union(*small))
    print(name, value_f64, "game pairs sharing a small leaf:", pairs, "distinct small leaves:", distinct)
    assert pairs >= 1
    assert distinct > (4 << case.log2_buckets)                     # more small leaves than the table holds: entries are replaced


def test_the_12x12_shape_at_24_simulations_never_descends():
    """The finding the cases answer: at simulation_per_step < 2 L every simulation is one select at the root and one expansion
    (the first simulation of an episode expands the empty root without a select), so selects == sims - 1 over a whole episode."""
    cfg, games = tc.shallow_stats()
    assert cfg.simulation_per_step < 2 * (cfg.board_size ** 2 - max(T for T, _ in games))
    for T, st in games:
        assert st["selects"] == st["sims"] - 1, st
        assert st["sims"] == T * cfg.simulation_per_step
